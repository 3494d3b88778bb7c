"""The input states of tests/test_hip_freeze_paths.py, chosen and justified on the CPU (not ``gpu`` marked).

An env whose state turns non-finite inside a simulation step is frozen (include/rcg.h, RCG_FIELD_STATUS).  The oracle has no
freeze, so the GPU file pins the rule differentially; what it relies on about its inputs is asserted here with the oracle's RK4
(``O.rk4_step``, float64) and a float32 NumPy restatement of the same step:

* bad-now states - finite, non-finite after the first step (the recipe of test_vectorised_env_step_equals_the_scalar_kernel):
  3wrobot alpha = 0, v = 3e38 (f32) / 1.7e308 (f64): k1 + 2 k2 + 2 k3 + k4 of x overflows; 2tank h2 = 1e30 / 1e200: K3 h2^2 does.
  Sys3WRobotNI CANNOT overflow from a finite state under clipped actions: |dx|, |dy| <= |v| <= 25 and |dalpha| <= 5 whatever the
  state, so a step moves a component by at most 0.25 - next to a component large enough to overflow that is less than half an
  ulp, and the component stays where it is.  It gets the NaN-on-entry kind only.
* a bad-later state of the tank - finite for n >= 1 whole ticks, non-finite in tick n + 1 under any held action inside the
  bounds, AT THE PRESET dt_sim = 0.1 (no larger step is needed): dh2/dt ~ K3 / tau2 h2^2, and once dt K3 / tau2 h2 >> 1 one RK4
  step raises h2 to about its 16th power (four nested squares), so the window is narrow: searched on a log grid, n asserted.
* NaN-on-entry: one component NaN, STATUS 0.
* benign replacements (``rand_states``) stay finite for the whole run.
* from a frozen state every candidate's ``_actor_cost`` is non-finite (NaN counts as +inf: index 0 wins with +inf)."""
import numpy as np
import pytest

from oracle import rcg_oracle as O
from tests.helpers import PRESETS, oracle_cfg, rand_actions, rand_states

REAL = {"f32": np.float32, "f64": np.float64}


# ---------------------------------------------------------------------------------------------------------------------
# the states
# ---------------------------------------------------------------------------------------------------------------------
def bad_now_state(name, dtype):
    """Finite in ``dtype``; non-finite after one RK4 step of the preset's dt_sim under any action inside the bounds."""
    if name == "3wrobot":
        return np.array([1.0, -2.0, 0.0, 3e38 if dtype == "f32" else 1.7e308, 0.5])
    if name == "2tank":
        return np.array([1.0, 1e30 if dtype == "f32" else 1e200])
    raise ValueError(f"{name} cannot overflow from a finite state (module docstring)")


def nan_entry_state(name):
    """One component NaN (the last: the heading / omega / h2), everything else benign."""
    x = np.array(PRESETS[name]["x0"], dtype=float)
    x[-1] = np.nan
    return x


def state_dyn_r(name, x, u, real):
    """``O.state_dyn`` restated in ``real`` arithmetic (one env or a batch, last axis = component)."""
    x = np.asarray(x, dtype=real)
    u = np.asarray(u, dtype=real)
    p = [real(v) for v in PRESETS[name]["pars"]]
    one = real(1)
    if name == "3wrobot":
        return np.stack([x[..., 3] * np.cos(x[..., 2]), x[..., 3] * np.sin(x[..., 2]), x[..., 4], one / p[0] * u[..., 0],
                         one / p[1] * u[..., 1]], axis=-1).astype(real)
    if name == "3wrobotNI":
        return np.stack([u[..., 0] * np.cos(x[..., 2]), u[..., 0] * np.sin(x[..., 2]), u[..., 1] + 0 * x[..., 2]], axis=-1).astype(real)
    return np.stack([one / p[0] * (-x[..., 0] + p[2] * u[..., 0]),
                     one / p[1] * (-x[..., 1] + p[3] * x[..., 0] + p[4] * x[..., 1] ** 2)], axis=-1).astype(real)


def rk4_r(name, x, u, h, real):
    """``O.rk4_step`` restated in ``real`` arithmetic, the action clipped to the preset's bounds."""
    b = np.array(PRESETS[name]["bnds"], dtype=real)
    x = np.asarray(x, dtype=real)
    u = np.clip(np.asarray(u, dtype=real), b[:, 0], b[:, 1])
    h = real(h)
    with np.errstate(all="ignore"):
        k1 = state_dyn_r(name, x, u, real)
        k2 = state_dyn_r(name, x + real(0.5) * h * k1, u, real)
        k3 = state_dyn_r(name, x + real(0.5) * h * k2, u, real)
        k4 = state_dyn_r(name, x + h * k3, u, real)
        return (x + h / real(6) * (k1 + real(2) * k2 + real(2) * k3 + k4)).astype(real)


def finite_ticks(name, x, u, dtype, limit=8, dt=None):
    """Whole ticks (one RK4 substep of the preset's dt_sim each) the state stays finite under the held action ``u``."""
    real = REAL[dtype]
    dt = PRESETS[name]["dt"] if dt is None else dt
    x = np.asarray(x, dtype=real)
    for n in range(limit):
        x = rk4_r(name, x, u, dt, real)
        if not np.all(np.isfinite(x)):
            return n
    return limit


_GRID = np.logspace(1, 8, 141)  # h2 = 10 .. 1e8, 20 points per decade


def _later_profile(dtype):
    """n(h2) on the log grid: the smallest over the two extreme held actions (they must agree where a state is used)."""
    lo = np.array([finite_ticks("2tank", [1.0, h2], [0.0], dtype) for h2 in _GRID])
    hi = np.array([finite_ticks("2tank", [1.0, h2], [1.0], dtype) for h2 in _GRID])
    return lo, hi


def bad_later_state(dtype):
    """(state, n): a tank state that stays finite for n >= 1 ticks and is non-finite in tick n + 1 for every held action in the
    bounds - the middle of the longest run of grid points that share one n in 1 .. 4 (so that a rounding of the GPU's fused
    arithmetic does not move it out of the window)."""
    lo, hi = _later_profile(dtype)
    best = None
    i = 0
    while i < len(_GRID):
        j = i
        while j + 1 < len(_GRID) and lo[j + 1] == lo[i] and hi[j + 1] == hi[i]:
            j += 1
        if lo[i] == hi[i] and 1 <= lo[i] <= 4 and (best is None or j - i > best[1] - best[0]):
            best = (i, j)
        i = j + 1
    assert best is not None, "no bad-later window on the grid at the preset dt_sim"
    mid = (best[0] + best[1]) // 2
    return np.array([1.0, float(REAL[dtype](_GRID[mid]))]), int(lo[mid])


def freeze_batch(name, dtype, B, seed, later=False):
    """The batch of the GPU file: (x_bad, x_clean, bad_now indices, nan index, preset-status index, bad-later index or None).
    bad-now envs at 0, 7, 63, 64 and B - 1 (first lane, last env of a K = 8 tile, both sides of a wave boundary, the ragged
    end; Sys3WRobotNI: NaN-on-entry there too), a NaN-on-entry env at 20, an env whose STATUS the caller presets at 33, and
    - ``later``, the tank only - a bad-later env at 40."""
    rng = np.random.default_rng(seed)
    clean = rand_states(rng, name, B).astype(REAL[dtype]).astype(np.float64)
    bad = clean.copy()
    now = np.array(sorted({0, 7, 63 % B, 64 % B, B - 1}))
    for i in now:
        bad[i] = nan_entry_state(name) if name == "3wrobotNI" else bad_now_state(name, dtype)
    nan_at, pre_at = 20 % B, 33 % B
    bad[nan_at] = nan_entry_state(name)
    later_at = None
    if later:
        assert name == "2tank"
        later_at = 40 % B
        bad[later_at] = bad_later_state(dtype)[0]
    return bad, clean, now, nan_at, pre_at, later_at


# ---------------------------------------------------------------------------------------------------------------------
# what the GPU file relies on
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["3wrobot", "3wrobotNI", "2tank"])
def test_float32_restatement_follows_the_oracle(name):
    rng = np.random.default_rng(1)
    x = rand_states(rng, name, 64)
    u = rand_actions(rng, name, (64,), overshoot=1.2)
    cfg = oracle_cfg(name)
    ref = O.rk4_step(cfg.sys_id, x, u, cfg.pars, cfg.ctrl_bnds, cfg.dt_sim)
    got64 = rk4_r(name, x, u, cfg.dt_sim, np.float64)
    got32 = rk4_r(name, x, u, cfg.dt_sim, np.float32)
    assert np.max(np.abs(got64 - ref) / np.maximum(np.abs(ref), 1.0)) < 1e-14
    assert np.max(np.abs(got32 - ref) / np.maximum(np.abs(ref), 1.0)) < 1e-5


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("name", ["3wrobot", "2tank"])
def test_bad_now_states_are_finite_and_leave_the_first_step_non_finite(name, dtype):
    real = REAL[dtype]
    x = bad_now_state(name, dtype)
    assert np.all(np.isfinite(x.astype(real)))
    cfg = oracle_cfg(name)
    b = np.array(PRESETS[name]["bnds"], dtype=float)
    for u in (b[:, 0], b[:, 1], b.mean(axis=1), b[:, 0] / 10.0):
        assert finite_ticks(name, x, u, dtype) == 0, (name, dtype, u)
        if dtype == "f64":  # the oracle's own step
            with np.errstate(all="ignore"):
                assert not np.all(np.isfinite(O.rk4_step(cfg.sys_id, x, u, cfg.pars, cfg.ctrl_bnds, cfg.dt_sim)))


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_kinematic_robot_cannot_overflow_from_a_finite_state(dtype):
    real = REAL[dtype]
    big = float(np.finfo(real).max)
    b = np.array(PRESETS["3wrobotNI"]["bnds"], dtype=float)
    for x in ([big, -big, big], [0.9 * big, big, -0.9 * big], [big, big, 1.0]):
        for u in (b[:, 0], b[:, 1], 3.0 * b[:, 1]):  # (beyond the bounds: clipped)
            assert finite_ticks("3wrobotNI", x, u, dtype, limit=3) == 3


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_bad_later_state_freezes_in_a_later_tick_at_the_preset_step(dtype):
    x, n = bad_later_state(dtype)
    assert 1 <= n <= 4
    assert np.all(np.isfinite(x.astype(REAL[dtype])))
    for u in ([0.0], [0.3], [1.0], [7.0]):  # the held action moves h1 alone; K2 h1 is nothing next to K3 h2^2
        assert finite_ticks("2tank", x, u, dtype) == n, (dtype, u)
    # the window has room on both sides: a few per cent of h2 either way does not change n
    for f in (0.97, 1.03):
        assert finite_ticks("2tank", x * np.array([1.0, f]), [0.5], dtype) == n
    if dtype == "f64":  # the oracle's own step agrees
        cfg = oracle_cfg("2tank")
        y = x.copy()
        with np.errstate(all="ignore"):
            for t in range(n + 1):
                assert np.all(np.isfinite(y)), t
                y = O.rk4_step(cfg.sys_id, y, [0.5], cfg.pars, cfg.ctrl_bnds, cfg.dt_sim)
        assert not np.all(np.isfinite(y))


@pytest.mark.parametrize("name", ["3wrobot", "3wrobotNI", "2tank"])
def test_nan_on_entry_states_stay_non_finite(name):
    x = nan_entry_state(name)
    assert np.isnan(x).sum() == 1
    for dtype in ("f32", "f64"):
        assert finite_ticks(name, x, np.array(PRESETS[name]["bnds"], dtype=float)[:, 0] / 10.0, dtype) == 0


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("name", ["3wrobot", "3wrobotNI", "2tank"])
def test_benign_states_stay_finite_for_the_whole_run(name, dtype):
    """Six ticks (the longest run of the GPU file: five in one launch, a reset, one more) under the worst held action."""
    bad, clean, now, nan_at, pre_at, later_at = freeze_batch(name, dtype, 150, seed=3, later=name == "2tank")
    b = np.array(PRESETS[name]["bnds"], dtype=float)
    for u in (b[:, 0], b[:, 1]):
        assert finite_ticks(name, clean, np.broadcast_to(u, (150, len(u))), dtype, limit=6) == 6
    healthy = np.ones(150, bool)
    healthy[list(now) + [nan_at] + ([later_at] if later_at is not None else [])] = False
    np.testing.assert_array_equal(bad[healthy], clean[healthy])
    assert np.all(np.isfinite(bad[pre_at]))  # the env frozen by the caller holds a benign state


def _mpc_cost_r(name, cand, x, real):
    """``O.actor_cost`` (MPC, gamma = 1, the preset's diagonal R1) restated in ``real``: cand [K, N, du] from state x."""
    p = PRESETS[name]
    R1 = np.array(p["R1"], dtype=real)
    tgt = np.zeros(len(x), dtype=real) if p["target"] is None else np.array(p["target"], dtype=real)
    h = real(p["dt"] * p["mult"])
    cand = np.asarray(cand, dtype=real)
    K, Nh, du = cand.shape
    s = np.broadcast_to(np.asarray(x, dtype=real), (K, len(x))).copy()
    J = np.zeros(K, dtype=real)
    with np.errstate(all="ignore"):
        for k in range(Nh):
            if k > 0:
                s = (s + h * state_dyn_r(name, s, cand[:, k - 1], real)).astype(real)
            chi = np.concatenate([s - tgt, cand[:, k]], axis=-1)
            J = J + np.sum(R1 * chi * chi, axis=-1)
    return J


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("name", ["3wrobot", "3wrobotNI", "2tank"])
def test_every_candidate_costs_non_finite_from_a_frozen_state(name, dtype):
    """NaN counts as +inf and the lowest index wins (include/rcg.h, rcg_actor_argmin): index 0, +inf."""
    rng = np.random.default_rng(4)
    Nh = 5
    states = [nan_entry_state(name)] + ([bad_now_state(name, dtype)] if name != "3wrobotNI" else [])
    for K in (3, 8, 16, 40):
        cand = rand_actions(rng, name, (K, Nh))
        for x in states:
            J = _mpc_cost_r(name, cand, x, REAL[dtype])
            assert not np.any(np.isfinite(J)), (name, dtype, K, x)
            if dtype == "f64":  # the oracle's _actor_cost itself, in every mode
                for mode, kw in (("MPC", {}), ("RQL", dict(buffer_size=6)), ("SQL", dict(buffer_size=6))):
                    cfg = oracle_cfg(name, n_actor=Nh, mode=O.MODE_IDS[mode], **kw)
                    with np.errstate(all="ignore"):
                        Jo = O.actor_cost(cand, x[None], x[None], cfg, w_critic=np.ones(cfg.dc))
                    assert not np.any(np.isfinite(Jo)), (name, mode, K)
                    bj, bi = O.argmin_first(Jo[None])
                    if mode == "MPC":
                        assert bi[0] == 0 and bj[0] == np.inf
