"""k_actor_dma's zero-weight instance (rcg_actor_dma.hpp, template parameter ZW), on the GPU.  A float64 MPC handle of a robot
with the preset's zero stage weights and gamma = 1 runs the streamed decision on an instance that does not accumulate the cost
terms of the zero-weighted components (3wrobot: v, omega, F, M; 3wrobotNI: the two actions) and tests them for NaN / inf once -
on the observation, the last rolled-out state and the last action.

  * dispatch: which handles take it (rcg_last_launch_zero_w), and that kernel and variant are reported as before;
  * the same bits as the plain accumulation: the same values 8 bytes off 16-byte alignment are served by k_actor, whose
    streamed gamma = 1 accumulation sums every component - action, best_J, best_idx and accum must be equal bit for bit;
  * NaN / inf in the inputs: best_idx is numpy's argmin over the oracle's J with NaN -> +inf, exactly; best_J is +inf exactly
    where the oracle's is, else the oracle's at the suite's float64 tolerance (the oracle's libm trig and the kernel's
    polynomial differ in the last bits, so no two implementations share J's bits) - and bit for bit k_actor's."""
import numpy as np
import pytest

from oracle import rcg_oracle as O
from tests.helpers import PRESETS, TOL, assert_kernel, both, oracle_cfg, rand_actions, rand_states

pytestmark = pytest.mark.gpu

MASK = {"3wrobot": 0x78, "3wrobotNI": 0x18}
ROBOTS = list(MASK)
OUT_FIELDS = ("FIELD_STATE", "FIELD_ACTION", "FIELD_BEST_J", "FIELD_BEST_IDX", "FIELD_ACCUM", "FIELD_STEP_IDX")


def offset_view(eng, a):
    """The values of ``a`` on the device, 8 bytes off 16-byte alignment (a view into an allocation one element longer)."""
    from rcognita_amd.engine import DeviceArray

    a = np.ascontiguousarray(a, dtype=eng.real)
    assert a.dtype.itemsize == 8
    base = eng.to_device(np.concatenate([np.zeros(1, a.dtype), a.ravel()]))
    assert base.ptr % 16 == 0
    v = DeviceArray.__new__(DeviceArray)
    v.engine, v.dtype, v.scratch, v._cap = eng, a.dtype, False, 0
    v.shape, v.nbytes, v.ptr, v._view_of = a.shape, a.nbytes, base.ptr + 8, base
    return v


def same_bits(name, B, K, Nh, x, cand, what, expect_mask=True, obs=None, **kw):
    """Tick and rcg_actor_argmin on the aligned tensor (k_actor_dma) and on the same values off alignment (k_actor): equal
    outputs.  ``expect_mask`` False: the dispatch is not asked for (a library without the query)."""
    from rcognita_amd import _native as N

    dma, _ = both(name, B, "f64", n_actor=Nh, **kw)
    ref, _ = both(name, B, "f64", n_actor=Nh, **kw)
    dc, dr = dma.to_device(cand), offset_view(ref, cand)
    for e in (dma, ref):
        e.set_state(x)
    a_dma = dma.actor_argmin(dc, obs=obs)
    assert_kernel(dma, "k_actor_dma", N.DMA_MPC_G1)
    if expect_mask:
        assert dma.last_launch_zero_w() == MASK[name], what
    a_ref = ref.actor_argmin(dr, obs=obs)
    assert_kernel(ref, "k_actor")
    if expect_mask:
        assert ref.last_launch_zero_w() == 0, what
    for u, v, f in zip(a_dma, a_ref, ("action", "best_J", "best_idx")):
        assert np.array_equal(u, v, equal_nan=True), f"{what}: rcg_actor_argmin {f}"
    for t in range(2):
        dma.control_tick(dc)
        assert_kernel(dma, "k_actor_dma", N.DMA_MPC_G1)
        if expect_mask:
            assert dma.last_launch_zero_w() == MASK[name], what
        ref.control_tick(dr)
        assert_kernel(ref, "k_actor")
        for f in OUT_FIELDS:
            assert np.array_equal(dma.get_field(getattr(N, f)), ref.get_field(getattr(N, f)), equal_nan=True), f"{what}: tick {t} {f}"
    out = a_dma + (dma,)
    ref.close()
    return out


def test_which_handles_take_the_zero_weight_instance():
    from rcognita_amd import _native as N

    rng = np.random.default_rng(9)
    B, K, Nh = 64, 256, 10
    for name in ROBOTS:
        x = rand_states(rng, name, B)
        cand = rand_actions(rng, name, (B, K, Nh))
        r1 = np.array(PRESETS[name]["R1"], dtype=float)
        r1v = r1.copy()
        r1v[3] = 0.5  # 3wrobot: a weight on v; 3wrobotNI: on the first action
        for dtype, kw, variant, mask in (("f64", {}, N.DMA_MPC_G1, MASK[name]), ("f32", {}, N.DMA_MPC_G1, 0),
                                         ("f64", dict(gamma=0.9), N.DMA_MPC, 0),
                                         ("f64", dict(R1=np.diag(r1v)), N.DMA_MPC_G1, 0)):
            eng, _ = both(name, B, dtype, n_actor=Nh, **kw)
            eng.set_state(x.astype(eng.real))
            dc = eng.to_device(cand)
            eng.control_tick(dc)
            assert_kernel(eng, "k_actor_dma", variant)
            assert eng.last_launch_zero_w() == mask, (name, dtype, kw)
            eng.actor_argmin(dc)
            assert_kernel(eng, "k_actor_dma", variant)
            assert eng.last_launch_zero_w() == mask, (name, dtype, kw)
            eng.actor_cost(dc)  # operator mode: J's bits are an output, the plain instance writes them
            assert_kernel(eng, "k_actor_dma", variant)
            assert eng.last_launch_zero_w() == 0, (name, dtype, kw)
            eng.close()
    tank, _ = both("2tank", B, "f64", n_actor=Nh)
    tank.set_state(rand_states(rng, "2tank", B))
    tank.control_tick(tank.to_device(rand_actions(rng, "2tank", (B, K, Nh))))
    assert_kernel(tank, "k_actor_dma", N.DMA_MPC_G1)
    assert tank.last_launch_zero_w() == 0
    tank.close()


@pytest.mark.parametrize("K", [40, 64, 96, 256])  # single ragged tile, one tile, ragged last tile, four tiles (rows of >= 40 bytes)
@pytest.mark.parametrize("Nh", [1, 2, 3, 10])    # the horizons that take a part of the shared prefix, and one beyond it
@pytest.mark.parametrize("name", ROBOTS)
def test_same_bits_as_the_plain_accumulation(name, Nh, K):
    rng = np.random.default_rng(100 * Nh + K)
    B = 48
    x = rand_states(rng, name, B)
    cand = rand_actions(rng, name, (B, K, Nh))
    *_, eng = same_bits(name, B, K, Nh, x, cand, f"{name} N={Nh} K={K}")
    eng.close()


def test_same_bits_two_envs_per_wave_ragged_last_wave():
    rng = np.random.default_rng(16389)
    B, K, Nh = 16389, 64, 3
    x = rand_states(rng, "3wrobot", B)
    cand = rand_actions(rng, "3wrobot", (B, K, Nh))
    *_, eng = same_bits("3wrobot", B, K, Nh, x, cand, "3wrobot B=16389")
    ll = eng.last_launch()
    assert ll["envs_per_wave"] == 2 and B % 2 == 1, ll
    eng.close()


def _expected(cfg, x, cand, obs=None):
    """numpy's argmin over the oracle's J with NaN -> +inf"""
    o = x if obs is None else obs  # (without state_sys the rollout starts from the observation)
    J = O.actor_cost(cand, o[:, None, :], o[:, None, :], cfg)
    Jc = np.where(np.isnan(J), np.inf, J)
    bi = np.argmin(Jc, axis=1).astype(np.int32)
    return bi, Jc[np.arange(len(bi)), bi]


def _check_decision(bj, bi, bi_or, bj_or, what):
    np.testing.assert_array_equal(bi, bi_or, err_msg=what)
    inf = np.isinf(bj_or)
    np.testing.assert_array_equal(bj[inf], bj_or[inf], err_msg=what)
    err = float(np.max(np.abs(bj - bj_or)[~inf] / np.maximum(np.abs(bj_or[~inf]), 1.0)))
    print(f"{what}: best_J max rel err vs oracle {err:.3e}")
    assert err <= TOL["f64"], (what, err)


@pytest.mark.parametrize("K", [96, 256])
@pytest.mark.parametrize("name", ROBOTS)
def test_nan_and_inf_in_the_candidates(name, K):
    """NaN, +inf, -inf one at a time: the first action of a row, both components of u[N-2] (they enter the last state), both
    components of u[N-1] (they enter nothing: the instance's own term), the last real of an env's rows; an env whose rows are
    all NaN (index 0, +inf) and one whose costs are all +inf.  One poisoned row among K random ones is seldom the row that
    would have won, so each value is also put into EVERY row of an env, at u[N-2] and at u[N-1], component by component: on the
    3-wheel robot only the test of the last state (u[N-2] = F, M enter v, omega there) or of the last action can make these
    costs NaN - without it the env would decide for a finite cost instead of index 0 with +inf."""
    rng = np.random.default_rng(K)
    Nh = 10
    vals = (np.nan, np.inf, -np.inf)
    pos = [(3, 0, 0), (7, Nh - 2, 0), (K // 2 + 1, Nh - 2, 1), (K - 2, Nh - 1, 0), (11, Nh - 1, 1), (K - 1, Nh - 1, 1)]
    every = [(Nh - 2, 0), (Nh - 2, 1), (Nh - 1, 0), (Nh - 1, 1)]
    B = len(vals) * (len(pos) + len(every)) + 4
    x = rand_states(rng, name, B)
    cand = rand_actions(rng, name, (B, K, Nh))
    e = 0
    for v in vals:
        for (r, k, c) in pos:
            cand[e, r, k, c] = v
            e += 1
    cand[e] = np.nan
    cand[e + 1, :, 0, 0] = np.inf
    cand[e + 2, :, Nh - 1, 1] = -np.inf  # every row's last action: only the instance's own term sees it
    b = e + 3
    for v in vals:
        for (k, c) in every:
            cand[b, :, k, c] = v
            b += 1
    what = f"{name} K={K} nan/inf"
    act, bj, bi, eng = same_bits(name, B, K, Nh, x, cand, what)
    bi_or, bj_or = _expected(oracle_cfg(name, n_actor=Nh), x, cand)
    _check_decision(bj, bi, bi_or, bj_or, what)
    assert bi[e] == 0 and bj[e] == np.inf
    assert bi[e + 1] == 0 and bj[e + 1] == np.inf
    assert bi[e + 2] == 0 and bj[e + 2] == np.inf
    poisoned = np.array([p[0] for p in pos] * len(vals))
    assert not np.any(bi[:e] == poisoned)
    b = e + 3
    for v in vals:
        for (k, c) in every:
            assert bi[b] == 0 and bj[b] == np.inf, (name, K, v, k, c, bi[b], bj[b])
            b += 1
    assert b == B - 1 and np.isfinite(bj[B - 1])  # (the last env is clean)
    eng.close()


@pytest.mark.parametrize("K", [96, 256])
@pytest.mark.parametrize("Nh", [1, 10])
def test_an_observation_with_an_infinite_zero_weighted_component(Nh, K):
    """rcg_actor_argmin with a caller's observation whose v is +inf (weight 0): every cost is NaN in the reference - 0 * inf -
    so the env decides for index 0 with +inf.  Nactor = 1: the observation is the last state as well."""
    rng = np.random.default_rng(K + Nh)
    B = 8
    x = rand_states(rng, "3wrobot", B)
    obs = x.copy()
    obs[2, 3] = np.inf
    obs[5, 4] = -np.inf
    cand = rand_actions(rng, "3wrobot", (B, K, Nh))
    what = f"3wrobot N={Nh} K={K} obs inf"
    act, bj, bi, eng = same_bits("3wrobot", B, K, Nh, x, cand, what, obs=obs)
    bi_or, bj_or = _expected(oracle_cfg("3wrobot", n_actor=Nh), x, cand, obs=obs)
    _check_decision(bj, bi, bi_or, bj_or, what)
    for b in (2, 5):
        assert bi[b] == 0 and bj[b] == np.inf
    assert np.all(np.isfinite(np.delete(bj, [2, 5])))
    eng.close()


def _registered_copy_compare():
    """The child (no torch: tests/test_hip_user_system.py): Sys3WRobot registered from its own source under another name, float64,
    K = 256 - the run-time-compiled zero-weight instance against the built-in one."""
    from rcognita_amd import _native as N
    from tests.test_hip_user_system import _robot_source

    info = N.register_system("UserRobotZW", _robot_source("UserRobotZW"), 5, 2, 2)
    rng = np.random.default_rng(5)
    B, K, Nh = 96, 256, 10
    x = rand_states(rng, "3wrobot", B)
    cand = rand_actions(rng, "3wrobot", (B, K, Nh))
    cand[7, :, Nh - 1, 0] = np.inf  # (the instance's own test of the last action)
    a, _ = both("3wrobot", B, "f64", n_actor=Nh)
    b, _ = both("3wrobot", B, "f64", n_actor=Nh, engine_only=dict(sys_id=info["sys_id"]))
    for e in (a, b):
        e.set_state(x)
    ra, rb = a.actor_argmin(cand), b.actor_argmin(cand)
    for e in (a, b):
        assert_kernel(e, "k_actor_dma", N.DMA_MPC_G1)
        assert e.last_launch_zero_w() == 0x78, e.last_launch_zero_w()
    for u, v, f in zip(ra, rb, ("action", "best_J", "best_idx")):
        assert np.array_equal(u, v, equal_nan=True), f
    assert rb[2][7] == 0 and rb[1][7] == np.inf
    b.actor_cost(cand)  # a J output: the plain instance
    assert b.last_launch_zero_w() == 0
    for e in (a, b):
        e.control_tick(cand)
        assert e.last_launch_zero_w() == 0x78
    for f in OUT_FIELDS:
        assert np.array_equal(a.get_field(getattr(N, f)), b.get_field(getattr(N, f)), equal_nan=True), f
    progs = [p for p in N.system_programs(info["sys_id"]) if "k_actor_dma<" in p] if hasattr(N, "system_programs") else []
    print("registered copy on the zero-weight instance: equal", progs)


def test_a_registered_copy_of_the_robot_runs_the_same_instance():
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k != "PYTHONPATH"}
    code = "import sys; sys.path.insert(0, %r); import tests.test_hip_dma_zero_weight as t; t._registered_copy_compare(); " \
           "assert 'torch' not in sys.modules" % root
    r = subprocess.run([sys.executable, "-c", code], cwd=root, env=env, capture_output=True, text=True, timeout=600)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "equal" in r.stdout
