"""T ticks per launch on systems compiled at run time (rcg.h: the policy member TICKS) on the GPU.

The yardstick is the one tests/test_hip_ticks.py holds the built-in systems to: T ticks in ONE launch (rcg_control_ticks, or
rcg_control_tick_n with a caller's tensor) leave every field bit-identical to T single ticks on a second handle of the same
system.  (Single ticks on registered systems are held to the oracle, the restatement and F14 / F15 by test_hip_user_system*.py.)

1. The pendulum without an output map (DS = 2, DU = 1), MPC, generated grid.
2. The pendulum with y = (sin th, cos th, om) (DY = 3 != DS): the cases only k_ticks' `out` branch can get right - generated and
   streamed.
3. RQL / SQL on the `out` pendulum with CRITIC + TICKS (k_ticks_mem), generated and streamed.
4. An env whose state overflows in the first RK4 step: frozen and flagged as after single ticks.
5. Sys3WRobot and Sys2Tank, re-registered from their own source with TICKS + CRITIC under other names, against the built-in
   handles over a subset of test_hip_ticks.py's parametrisations: every field as bits and equal launch records.  In a child
   process that does not import torch, as test_hip_user_system.py does.
6. Refusals, with every field and rcg_tick_count unchanged.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.test_user_system_critic_register import load_f15  # noqa: E402
from tests.test_user_system_out_register import load_f14  # noqa: E402
from tests.test_user_system_register import PENDULUM  # noqa: E402
from tests.test_user_system_ticks_register import (BND, PEND_PARS, pendulum_out_ticks_source, pendulum_ticks_source,  # noqa: E402
                                                   with_ticks)

pytestmark = pytest.mark.gpu

FIELDS = ["FIELD_STATE", "FIELD_STATE_PREV", "FIELD_ACTION", "FIELD_ACCUM", "FIELD_STEP_IDX", "FIELD_STATUS", "FIELD_BEST_J",
          "FIELD_BEST_IDX"]
CRITIC_FIELDS = FIELDS + ["FIELD_W_CRITIC", "FIELD_W_PREV", "FIELD_OBS_BUF", "FIELD_ACT_BUF"]
AFTER_RESET = ["FIELD_RETURNS", "FIELD_EPISODE_IDX"]
STREAMED, MEM = 4, 16  # rcg_last_launch's variant word of k_ticks: bit 0 generic, bit 1 target, 4 streamed, 8 k_ticks_pk, 16 k_ticks_mem

_REG = {}


def _system(kind):
    """Each system registered once per module: 'plain' (TICKS), 'out' (output map + CRITIC + TICKS), 'no ticks' (the plain
    pendulum as test_user_system_register.py registers it) and 'out no ticks' (output map + CRITIC)."""
    from rcognita_amd import _native as N
    from tests.test_user_system_critic_register import pendulum_critic_source

    if kind not in _REG:
        name, src = {"plain": ("PendulumKG", pendulum_ticks_source("PendulumKG")),
                     "out": ("PendulumYKG", pendulum_out_ticks_source("PendulumYKG", critic=True)),
                     "no ticks": ("PendulumT", PENDULUM),
                     "out no ticks": ("PendulumYC", pendulum_critic_source("PendulumYC"))}[kind]
        _REG[kind] = N.register_system(name, src, 2, 1, 3)
        assert _REG[kind]["has_ticks"] is (kind in ("plain", "out"))
    return _REG[kind]


def _engine(kind, dtype, B, Nh, R1, **kw):
    from rcognita_amd import Engine, EngineConfig

    cfg = dict(sys_id=_system(kind)["sys_id"], batch=B, dtype=dtype, Nactor=Nh, pars=PEND_PARS, ctrl_bnds=BND, R1=R1, dt_sim=0.01,
               sampling_time=0.02, pred_step_size=0.02)
    cfg.update(kw)
    return Engine(EngineConfig(**cfg))


def _states(rng, B):
    return np.stack([rng.uniform(-3, 3, B), rng.uniform(-2, 2, B)], axis=-1)


def _same(many, one, fields, what):
    from rcognita_amd import _native as N

    for f in fields:
        u, v = many.get_field(getattr(N, f)), one.get_field(getattr(N, f))
        assert u.dtype == v.dtype and u.shape == v.shape and u.tobytes() == v.tobytes(), (what, f, int(np.sum(u != v)))


def _snapshot(e, fields):
    from rcognita_amd import _native as N

    return {f: e.get_field(getattr(N, f)).copy() for f in fields}, N.lib().rcg_tick_count(e._h)


def _unchanged(e, snap, what):
    from rcognita_amd import _native as N

    for f, v in snap[0].items():
        assert e.get_field(getattr(N, f)).tobytes() == v.tobytes(), (what, f)
    assert N.lib().rcg_tick_count(e._h) == snap[1], what


_FULL3 = np.random.default_rng(30).uniform(-1, 1, (3, 3))


def _mpc_cases(kind):
    """(what, K, B, keywords) of the MPC cases: the shapes of test_hip_ticks.py's generated-grid matrix on the pendulum.  R1 is
    (dy + 1)^2: diagonal, or full (the generic instance; the `out` pendulum takes F14's)."""
    if kind == "out":
        meta, z = load_f14()
        diag, full, target = z["a_R1"][0], z["a_R1"][2], z["a_target"][4]
        assert meta["cases"][2]["cost"] == "full" and np.count_nonzero(full - np.diag(np.diag(full)))
    else:
        diag, full, target = np.diag([10.0, 1.0, 0.1]), _FULL3 @ _FULL3.T, np.array([0.4, -0.2])
    return [("K64", 64, 1024, dict(R1=diag)),
            ("K256 substeps gamma", 256, 300, dict(R1=diag, substeps_per_tick=3, gamma=0.97)),
            ("K16 ref_lag", 16, 1030, dict(R1=diag, ref_lag=True)),
            ("K5 full R1", 5, 19, dict(R1=full)),
            ("K64 target", 64, 77, dict(R1=diag, observation_target=target, gamma=0.95)),
            # (the stage cost charged at every RK4 substep: at out(x) for a system with an output map)
            ("K32 accum every substep", 32, 130, dict(R1=diag, accum_every_substep=True, substeps_per_tick=2))]


def _generated(kind, what, K, B, kw, dtype):
    from rcognita_amd import _native as N
    from tests.helpers import assert_kernel

    T, Nh = 7, 6
    kw = dict(kw)
    R1 = kw.pop("R1")
    one, many = _engine(kind, dtype, B, Nh, R1, **kw), _engine(kind, dtype, B, Nh, R1, **kw)
    x0 = _states(np.random.default_rng(K + B), B)
    for e in (one, many):
        e.set_state(x0)
    for _ in range(T):
        one.control_tick(None, K=K)
    many.control_ticks(T, K)
    ll = assert_kernel(many, "k_ticks")
    generic, tgt = "full" in what, "target" in what
    assert ll["variant"] == (1 if generic else 0) | (2 if tgt else 0), ll
    assert one.last_launch(N.KERNEL_ACTOR)["kernel"] != "k_ticks"
    _same(many, one, FIELDS, what)
    assert N.lib().rcg_tick_count(many._h) == N.lib().rcg_tick_count(one._h) == T
    assert np.any(many.get_field(N.FIELD_ACCUM) != 0) and np.any(many.get_state() != x0.astype(many.real))
    # and it continues identically: 3 more in one launch against 3 more single ticks, then an episode reset
    for _ in range(3):
        one.control_tick(None, K=K)
    many.control_ticks(3, K)
    for e in (one, many):
        e.episode_reset()
    one.control_tick(None, K=K)
    many.control_ticks(1, K)
    _same(many, one, FIELDS + AFTER_RESET, what + ", continued")
    one.close()
    many.close()


# ---- 1. the pendulum without an output map -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("case", range(6))
def test_pendulum_T_ticks_in_one_launch_equal_T_single_ticks(case, dtype):
    _generated("plain", *_mpc_cases("plain")[case], dtype)


# ---- 2. the pendulum with y = (sin th, cos th, om) -----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("case", range(6))
def test_out_pendulum_T_ticks_in_one_launch_equal_T_single_ticks(case, dtype):
    """DY = 3 != DS = 2: y_0 = out(x) for the rollouts, accum_update at out(x) (and, accum_every_substep, inside the env step)."""
    _generated("out", *_mpc_cases("out")[case], dtype)


def test_the_out_branch_is_what_these_cases_check():
    """The observation is not the state: with F14's weights the stage cost at y = out(x) differs from the one a kernel that took
    the state for the observation would charge, for every env of the shapes above."""
    from tests.test_user_system_out_register import pend_out

    _, z = load_f14()
    x = _states(np.random.default_rng(64 + 1024), 1024)
    y = pend_out(x)
    R1 = z["a_R1"][0]
    assert y.shape[1] == 3 and np.all(np.abs(np.einsum("bi,i,bi->b", y, np.diag(R1)[:3], y)
                                             - np.einsum("bi,i,bi->b", x, np.diag(R1)[:2], x)) > 0)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("what,K,B", [
    ("rows resident in LDS", 64, 300),
    ("a ragged tile", 48, 77),
    ("packed single ticks", 16, 130),
    ("re-staged every tick", 1024, 9),    # (float64: 48 KB of rows per wave; float32: 24 KB, resident - the next case)
    ("re-staged every tick f32", 2048, 9),
])
def test_out_pendulum_streamed_T_ticks_equal_T_single_ticks(what, K, B, dtype):
    """rcg_control_tick_n with a caller's tensor: one launch of k_ticks' streamed instance against T single ticks on the streamed
    production kernels."""
    from rcognita_amd import _native as N
    from tests.helpers import assert_kernel

    _, z = load_f14()
    T, Nh = 6, 6
    rng = np.random.default_rng(K * 7 + B)
    one, many = (_engine("out", dtype, B, Nh, z["a_R1"][0], gamma=0.97) for _ in range(2))
    x0 = _states(rng, B)
    c = rng.uniform(BND[0, 0], BND[0, 1], (B, K, Nh, 1)).astype(one.real)
    ca, cb = one.to_device(c), many.to_device(c)
    for e in (one, many):
        e.set_state(x0)
    for _ in range(T):
        one.control_tick(ca, K=K)
    many.control_tick(cb, K=K, T=T)
    ll = assert_kernel(many, "k_ticks")
    assert ll["variant"] == STREAMED, ll
    lone = one.last_launch(N.KERNEL_ACTOR)
    assert lone["kernel"] != "k_ticks", lone  # single ticks must not report k_ticks
    if what == "packed single ticks":
        assert lone["kernel"] == "k_actor_dma_packed", lone
    _same(many, one, FIELDS, what)
    assert N.lib().rcg_tick_count(many._h) == N.lib().rcg_tick_count(one._h) == T
    # the two entry points continue from each other's state
    many.control_tick(cb, K=K)
    one.control_tick(ca, K=K, T=1)
    _same(many, one, FIELDS, what + ", continued")
    one.close()
    many.close()


# ---- 3. RQL / SQL on the `out` pendulum ----------------------------------------------------------------------------------------
def _critic_engine(dtype, B, mode, cs, **kw):
    meta, _ = load_f15()
    cfg = dict(mode=mode, critic_struct=cs, Ncritic=4, buffer_size=6, gamma=meta["gamma"],
               observation_target=np.array(meta["target"]), sampling_time=meta["sampling_time"], pred_step_size=meta["pred_step_size"])
    cfg.update(kw)
    return _engine("out", dtype, B, 5, np.diag(meta["R1"]), **cfg)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("mode,cs,K,B,kw", [
    ("RQL", "quad-nomix", 64, 300, dict(Ncritic=4, buffer_size=6)),
    ("SQL", "quad-mix", 16, 130, dict(Ncritic=6, buffer_size=8)),                 # 4 envs per wave, 5 TD rows
    ("SQL", "quad-nomix", 64, 77, dict(Ncritic=4, buffer_size=6, critic_every_ticks=3)),
    ("RQL", "quad-nomix", 32, 515, dict(Ncritic=4, buffer_size=6, ref_lag=True)),
])
def test_out_pendulum_critic_mode_T_ticks_equal_T_single_ticks(mode, cs, K, B, kw, dtype):
    """k_ticks_mem on a registered system: the handles carry F15's target, which the policy's preset (TGT = false) does not have -
    the instance is compiled for the handle's own setting.  Split 2 + 3, so that the critic period's phase and the ring position
    cross a launch boundary."""
    from rcognita_amd import _native as N
    from tests.helpers import assert_kernel

    one, many = (_critic_engine(dtype, B, mode, cs, **kw) for _ in range(2))
    x0 = _states(np.random.default_rng(K + B), B) * 0.5
    for e in (one, many):
        e.set_state(x0)
    w0 = many.get_field(N.FIELD_W_CRITIC).copy()
    for _ in range(5):
        one.control_tick(None, K=K)
    many.control_ticks(2, K)
    many.control_ticks(3, K)
    ll = assert_kernel(many, "k_ticks")
    assert ll["variant"] == MEM | 1 | 2, ll
    assert_kernel(one, "k_critic_fit", kind=N.KERNEL_CRITIC)
    assert one.last_launch(N.KERNEL_ACTOR)["kernel"] != "k_ticks"
    _same(many, one, CRITIC_FIELDS, (mode, cs))
    assert N.lib().rcg_tick_count(many._h) == N.lib().rcg_tick_count(one._h) == 5
    assert not np.array_equal(many.get_field(N.FIELD_W_CRITIC), w0)  # the fit moved the weights
    # an episode reset, then rcg_control_tick_n's route to the same kernel
    for e in (one, many):
        e.episode_reset()
    for _ in range(4):
        one.control_tick(None, K=K)
    many.control_tick(None, K=K, T=4)
    assert_kernel(many, "k_ticks")
    _same(many, one, CRITIC_FIELDS + AFTER_RESET, (mode, cs, "continued"))
    one.close()
    many.close()


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("mode,K,B", [("RQL", 64, 300), ("SQL", 33, 40), ("RQL", 8, 77)])
def test_out_pendulum_streamed_critic_mode_T_ticks_equal_T_single_ticks(mode, K, B, dtype):
    """rcg_control_tick_n with a caller's tensor on an RQL / SQL handle: one launch of k_ticks_mem's streamed instance against
    single ticks on k_actor_dma / k_actor_dma_packed / k_actor.  No target: the streamed decision phase is tied to the
    preset-cost instances of the single ticks, which exist for the policy's own target setting."""
    from rcognita_amd import _native as N
    from tests.helpers import assert_kernel

    T = 5
    rng = np.random.default_rng(K * 11 + B)
    one, many = (_critic_engine(dtype, B, mode, "quad-nomix", observation_target=None) for _ in range(2))
    x0 = _states(rng, B) * 0.5
    c = rng.uniform(BND[0, 0], BND[0, 1], (B, K, 5, 1)).astype(one.real)
    ca, cb = one.to_device(c), many.to_device(c)
    for e in (one, many):
        e.set_state(x0)
    w0 = many.get_field(N.FIELD_W_CRITIC).copy()
    for _ in range(T):
        one.control_tick(ca, K=K)
    many.control_tick(cb, K=K, T=2)
    many.control_tick(cb, K=K, T=3)
    ll = assert_kernel(many, "k_ticks")
    assert ll["variant"] == MEM | STREAMED | 1, ll
    assert one.last_launch(N.KERNEL_ACTOR)["kernel"] in ("k_actor_dma", "k_actor_dma_packed", "k_actor")
    _same(many, one, CRITIC_FIELDS, (mode, K))
    assert N.lib().rcg_tick_count(many._h) == N.lib().rcg_tick_count(one._h) == T
    assert not np.array_equal(many.get_field(N.FIELD_W_CRITIC), w0)
    one.close()
    many.close()


# ---- 4. freeze -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["plain", "out"])
def test_T_ticks_freeze_a_nonfinite_env_as_single_ticks_do(kind):
    from rcognita_amd import _native as N

    B, K, T, Nh = 64, 64, 6, 5
    R1 = _mpc_cases(kind)[0][3]["R1"]
    one, many, clean = (_engine(kind, "f64", B, Nh, R1) for _ in range(3))
    x0 = _states(np.random.default_rng(2), B)
    xc = x0.copy()
    x0[7, 1] = 1e308  # overflows inside the first RK4 step: frozen at its last finite state, flagged
    one.set_state(x0)
    many.set_state(x0)
    clean.set_state(xc)
    for _ in range(T):
        one.control_tick(None, K=K)
    many.control_ticks(T, K)
    clean.control_ticks(T, K)
    _same(many, one, FIELDS, kind)
    ok = np.arange(B) != 7
    st = many.get_field(N.FIELD_STATUS)
    assert st[7] == 1 and not st[ok].any()
    np.testing.assert_array_equal(many.get_state()[7], x0[7])
    np.testing.assert_array_equal(many.get_field(N.FIELD_STEP_IDX), np.full(B, T, np.int32))
    for f in FIELDS:  # the other envs are unaffected
        u, v = many.get_field(getattr(N, f)), clean.get_field(getattr(N, f))
        assert u[ok].tobytes() == v[ok].tobytes(), f


# ---- 5. copies of two built-in systems -----------------------------------------------------------------------------------------
def _copy_source(struct, name):
    from tests.test_hip_user_system_critic import _copy_source as with_critic_copy

    return with_ticks(with_critic_copy(struct, name))


def _copies_compare():
    """The child: built-in Sys3WRobot / Sys2Tank against their renamed copies with TICKS + CRITIC, T ticks in one launch on both;
    raises on the first difference."""
    from oracle import rcg_oracle as O
    from rcognita_amd import Engine
    from rcognita_amd import _native as N

    from tests.helpers import engine_cfg, rand_states

    copies = {"3wrobot": N.register_system("UserRobotK", _copy_source("Sys3WRobot", "UserRobotK"), 5, 2, 2),
              "2tank": N.register_system("UserTankK", _copy_source("Sys2Tank", "UserTankK"), 2, 1, 5)}
    assert all(i["has_ticks"] and i["has_critic"] and not i["has_out"] for i in copies.values())
    rql = dict(n_critic=4, buffer_size=6)
    # (system, what, K, B, streamed, keywords): rows of test_hip_ticks.py's matrices - per system one generated, one streamed, one
    # critic-mode generated and one critic-mode streamed case; the robot's quad-lin (35 weights: the four-lane ML phase)
    cases = [
        ("3wrobot", "gen", 64, 1024, False, {}),
        ("3wrobot", "gen K256", 256, 300, False, dict(substeps_per_tick=3, gamma=0.97)),
        # the one exception to "equal launch records": float32, preset cost, K >= 256, gamma = 1 - the built-in picks k_ticks_pk, a
        # shell hand-packed for it that a registered system does not get; the copy runs k_ticks and only the bits must agree
        ("3wrobot", "gen pk", 256, 300, False, {}),
        ("3wrobot", "streamed", 16, 1030, True, dict(ref_lag=True)),
        ("3wrobot", "critic gen", 64, 515, False, dict(mode=O.MODE_RQL, critic_struct=O.CRITIC_QUAD_NOMIX, ref_lag=True, **rql)),
        ("3wrobot", "critic streamed quad-lin", 64, 130, True, dict(mode=O.MODE_RQL, critic_struct=O.CRITIC_QUAD_LIN, **rql)),
        ("2tank", "gen", 32, 515, False, {}),
        ("2tank", "gen generic", 5, 19, False, dict(stage_obj_struct=O.STAGE_BIQUADRATIC, R2=np.diag([1.0, 2.0, 0.5]))),
        ("2tank", "streamed", 48, 515, True, {}),
        ("2tank", "critic gen", 64, 1024, False, dict(mode=O.MODE_SQL, critic_struct=O.CRITIC_QUAD_LIN, n_critic=3, buffer_size=5,
                                                    critic_every_ticks=3)),
        ("2tank", "critic streamed", 16, 130, True, dict(mode=O.MODE_RQL, critic_struct=O.CRITIC_QUAD_NOMIX, ref_lag=True, **rql)),
    ]
    checked, seen = 0, set()
    for name, what, K, B, streamed, kw in cases:
        for dtype in ("f32", "f64"):
            tag = (name, what, dtype)
            critic = "mode" in kw
            T, Nh = 7, (5 if critic or streamed else 6)
            rng = np.random.default_rng(K + B)

            def make(sid):
                c = engine_cfg(name, B, dtype, n_actor=Nh, **kw)
                c.sys_id = sid
                return Engine(c)

            a, b = make(N.SYS_IDS[name]), make(copies[name]["sys_id"])
            x0 = rand_states(rng, name, B) * (0.5 if critic and name != "2tank" else 1.0)
            ca = cb = None
            if streamed:
                bn = np.asarray(a.cfg.ctrl_bnds, dtype=float)
                c = (bn[:, 0] + (bn[:, 1] - bn[:, 0]) * rng.random((B, K, Nh, a.du))).astype(a.real)
                ca, cb = a.to_device(c), b.to_device(c)
            fields = (CRITIC_FIELDS if critic else FIELDS)
            for e in (a, b):
                e.set_state(x0)
            for step in ((T,), (2, 3)):  # (2 + 3: the critic period's phase and the ring position cross a launch boundary)
                for n in step:
                    if streamed:
                        a.control_tick(ca, K=K, T=n)
                        b.control_tick(cb, K=K, T=n)
                    else:
                        a.control_ticks(n, K)
                        b.control_ticks(n, K)
                    for f in fields:
                        u, v = a.get_field(getattr(N, f)), b.get_field(getattr(N, f))
                        assert u.dtype == v.dtype and u.shape == v.shape and u.tobytes() == v.tobytes(), (tag, f)
                    la, lb = a.last_launch(N.KERNEL_ACTOR), b.last_launch(N.KERNEL_ACTOR)
                    assert la["kernel"] == lb["kernel"] == "k_ticks", (tag, la, lb)
                    if what == "gen pk" and dtype == "f32":
                        assert la["variant"] == 8 and lb["variant"] == 0, (tag, la, lb)
                    else:
                        assert la == lb, (tag, la, lb)
                        assert bool(la["variant"] & MEM) == critic and bool(la["variant"] & STREAMED) == streamed, (tag, la)
                    seen.add((dtype, lb["variant"]))
                    checked += 1
            assert N.lib().rcg_tick_count(a._h) == N.lib().rcg_tick_count(b._h) == T + 5, tag
            if critic:
                assert not np.allclose(b.get_field(N.FIELD_W_CRITIC), 1.0), tag
            a.close()
            b.close()
    n_programs = 0
    for i in copies.values():  # one program per instance, compiled once and listed
        programs = [(p, e) for p, e in N.system_programs(i["sys_id"]) if "k_ticks" in e]
        assert len(programs) == len(set(programs)) >= 8, programs
        assert all(p == i["name"] + ("_ticks_mem.hip" if "k_ticks_mem" in e else "_ticks.hip") for p, e in programs), programs
        assert any("k_ticks_mem<rcg::RcgRtcSys, float, 0, 3, false, true, true>" in e for _, e in programs) == (i["name"] == "UserRobotK")
        n_programs += len(programs)
    print("copies bit-identical:", checked, "comparisons;", sorted(seen), n_programs, "tick programs")


def test_copies_with_ticks_are_bit_identical_to_the_builtins():
    env = {k: v for k, v in os.environ.items() if k != "PYTHONPATH"}
    code = "import sys; sys.path.insert(0, %r); import tests.test_hip_user_system_ticks as t; t._copies_compare(); " \
           "assert 'torch' not in sys.modules" % ROOT
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=2400)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "bit-identical" in r.stdout


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    import ctypes as C

    from rcognita_amd import _native as N
    from tests.helpers import assert_kernel

    L = N.lib()
    B, K = 64, 16
    R1 = np.diag([10.0, 1.0, 0.1])
    x0 = _states(np.random.default_rng(9), B)

    # a policy without TICKS: rcg_control_ticks is refused, rcg_control_tick_n loops single ticks
    e = _engine("no ticks", "f32", B, 5, R1)
    e.set_state(x0)
    snap = _snapshot(e, FIELDS)
    assert L.rcg_control_ticks(e._h, 3, K) == N.ERR_UNSUPPORTED
    assert "TICKS" in N.last_error(e._h)
    _unchanged(e, snap, "control_ticks without TICKS")
    e.control_tick(None, K=K, T=3)
    assert L.rcg_tick_count(e._h) == 3
    assert_kernel(e, "k_actor")
    assert_kernel(e, "k_sim", kind=N.KERNEL_SIM)
    ref = _engine("plain", "f32", B, 5, R1)
    ref.set_state(x0)
    ref.control_ticks(3, K)
    _same(e, ref, FIELDS, "the loop of single ticks")
    e.close()

    # ... in RQL too (CRITIC without TICKS): generated and streamed stay loops of single ticks
    e = _engine("out no ticks", "f32", B, 5, np.diag(load_f15()[0]["R1"]), mode="RQL", critic_struct="quad-nomix", Ncritic=4,
                buffer_size=6)
    e.set_state(x0)
    snap = _snapshot(e, CRITIC_FIELDS)
    assert L.rcg_control_ticks(e._h, 3, K) == N.ERR_UNSUPPORTED
    _unchanged(e, snap, "RQL control_ticks without TICKS")
    e.control_tick(None, K=K, T=2)
    assert_kernel(e, "k_actor")
    cand = e.to_device(np.random.default_rng(5).uniform(-5, 5, (B, 64, 5, 1)).astype(e.real))
    e.control_tick(cand, K=64, T=2)
    assert e.last_launch(N.KERNEL_ACTOR)["kernel"] != "k_ticks" and L.rcg_tick_count(e._h) == 4
    e.close()

    # a TICKS policy: RQL with an empty TD stack (Ncritic = 1), T = 0, a K the generated grid does not have
    e = _critic_engine("f32", B, "RQL", "quad-nomix", Ncritic=1, buffer_size=5)
    e.set_state(x0)
    snap = _snapshot(e, CRITIC_FIELDS)
    assert L.rcg_control_ticks(e._h, 3, K) == N.ERR_UNSUPPORTED
    _unchanged(e, snap, "Ncritic = 1")
    assert L.rcg_control_ticks(e._h, 0, K) == N.ERR_BAD_ARG
    _unchanged(e, snap, "T = 0")
    e.close()

    e = _engine("out", "f64", B, 5, load_f14()[1]["a_R1"][0])
    e.set_state(x0)
    snap = _snapshot(e, FIELDS)
    assert L.rcg_control_ticks(e._h, 0, K) == N.ERR_BAD_ARG
    assert L.rcg_control_ticks(e._h, 2, 0) == N.ERR_BAD_ARG
    _unchanged(e, snap, "T = 0 / K = 0")
    # rcg_loop_step stays refused on a TICKS policy
    out = (C.c_double * (B * 16))()
    act = (C.c_double * B)()
    assert L.rcg_loop_step(e._h, C.cast(act, C.c_void_p), 0.01, 1, 0, 5, C.cast(out, C.c_void_p)) == N.ERR_UNSUPPORTED
    assert L.rcg_loop_step_begin(e._h, C.cast(act, C.c_void_p), 0.01, 1, N.LOOP_DECIDE, 5) == N.ERR_UNSUPPORTED
    _unchanged(e, snap, "rcg_loop_step")
    e.close()

    # ... and the two-halves tick (rcg_set_tick_parts 2) on a TICKS + CRITIC policy
    e = _critic_engine("f64", B, "RQL", "quad-nomix", observation_target=None)
    e.set_state(x0)
    snap = _snapshot(e, CRITIC_FIELDS)
    e.set_tick_parts(2)
    cand = e.to_device(np.random.default_rng(5).uniform(-5, 5, (B, 64, 5, 1)))
    assert L.rcg_control_tick(e._h, C.c_void_p(cand.ptr), 64) == N.ERR_UNSUPPORTED
    _unchanged(e, snap, "split tick")
    e.close()
