"""The nominal control law on systems compiled at run time (rcg.h: the policy member `nominal`) and T nominal ticks per launch
(rcg_control_ticks_nominal, k_ticks_nominal) on the GPU.  Policies and twins: tests/nominal_laws.py; their inputs are checked on
the CPU by test_user_system_nominal_register.py.

1. Engine.nominal_action / the Lyapunov value of (a), (b), (c) against the NumPy twins.
2. Twenty single nominal ticks of (a), (b), (c) against the twin loop; a target on (b); three ticks of (a) under the disturbance model.
3. Copies (d) of the two robots against the built-ins: outputs and six ticks as bits, equal launch records (a child process without
   torch: test_hip_user_system.py says why).
4. T ticks in one launch against T single ticks on a twin handle, every field as bits, and who gets the single launch.
5. A frozen env.   6. Refusals with nothing moved.   7. CtrlNominal in the reference's loop order.   8. Rate.

Tolerances (none of them fitted to a result).  The law, f64: 1e-12 (rel_err_norm), what the same twins' float64 right-hand sides are
held to in test_hip_user_system_corners.py (RHS_TOL).  f32 handles: one float32 ulp of the float32 rounding of the twin's float64
value at the float32-rounded inputs - the float64 error is far below half an ulp, so more is another law.  Closed loop: state and
action at RK4_TOL (1e-10 / 2e-4: the k_sim runs of those twins; the action is a function of that state), accum at TOL (1e-11 /
1e-5: their stage costs).
"""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.nominal_laws import (BND, C2_GAIN, CPARS, DT, GAIN, PEND_PARS, C2Twin, PendTwin, bad_state, c2_batch,  # noqa: E402
                                corner_c2, f32_round, pend_batch, pendulum_nominal_source, pendulum_out_nominal_source,
                                robot_copy_source, twin_tick, ulp32_distance)
from tests.test_user_system_register import PENDULUM  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = {"f64": 1e-11, "f32": 1e-5}
RK4_TOL = {"f64": 1e-10, "f32": 2e-4}
LAW_TOL = 1e-12
FIELDS = ["FIELD_STATE", "FIELD_STATE_PREV", "FIELD_ACTION", "FIELD_ACCUM", "FIELD_STEP_IDX", "FIELD_STATUS", "FIELD_BEST_J",
          "FIELD_BEST_IDX", "FIELD_ACTION_SQN"]
SIGMA, MU, TAU = [2.0], [0.5], [1.5]
TARGET_B = np.array([0.1, 0.9, -0.2])
_REG = {}
POLICIES = {"a": ("PendulumNom", lambda n: pendulum_nominal_source(n)),
            "a_noticks": ("PendulumNomNoLf", lambda n: pendulum_nominal_source(n, lf=False, ticks=False)),
            "a_dist": ("PendulumNomD", lambda n: pendulum_nominal_source(n, disturb=True)),
            "b": ("PendulumYNom", pendulum_out_nominal_source),
            "plain": ("PendulumT", lambda n: PENDULUM)}


def reg(key):
    from rcognita_amd import _native as N

    if key not in _REG:
        if key == "c":
            src, S = corner_c2()
            _REG[key] = N.register_system(S.name, src, S.ds, S.du, S.np)
        else:
            name, make = POLICIES[key]
            _REG[key] = N.register_system(name, make(name), 2, 1, 3)
    return _REG[key]


def twin_of(key):
    return C2Twin() if key == "c" else PendTwin(out=key == "b", disturb=key == "a_dist")


def law_args(key):
    """(ctrl_gain, ctrl_pars) of a policy's law."""
    return (C2_GAIN, ()) if key == "c" else (GAIN, CPARS)


def R1_of(key):
    S = twin_of(key)
    return np.diag(np.linspace(10.0, 0.5, S.dy + S.du))


def _engine(key, dtype, B, **kw):
    from rcognita_amd import Engine, EngineConfig

    info, S = reg(key), twin_of(key)
    cfg = dict(sys_id=info["sys_id"], batch=B, dtype=dtype, Nactor=5, pars=S.pars, ctrl_bnds=S.bnds, R1=R1_of(key), dt_sim=DT,
               sampling_time=DT, pred_step_size=2 * DT)
    if key == "c":
        cfg["per_env_pars"] = True
    cfg.update(kw)
    return Engine(EngineConfig(**cfg))


def _start(key, e, B):
    """Start states (and, (c), per-env parameters) set on the handle; returns them as the handle holds them (float64 values)."""
    from rcognita_amd import _native as N

    r = f32_round if e.cfg.dtype == "f32" else (lambda a: np.asarray(a, dtype=np.float64))
    if key == "c":
        x, p = c2_batch(B)
        e.set_field(N.FIELD_PARS, p)
        e.set_state(x)
        return r(x), r(p)
    x = pend_batch(B)
    e.set_state(x)
    return r(x), r(np.array(PEND_PARS))


def _held_action(S, B, dtype):
    """The action a fresh handle holds: action_min / 10 (controllers.py:973-975), as its element type rounds it."""
    a0 = S.bnds[:, 0] / 10.0
    return np.tile(f32_round(a0) if dtype == "f32" else a0, (B, 1))


def _tick_count(e):
    from rcognita_amd import _native as N

    return int(N.lib().rcg_tick_count(e._h))


def _err(a, b):
    from tests.helpers import rel_err_norm

    return rel_err_norm(a, b)


def _snapshot(e, fields=FIELDS):
    from rcognita_amd import _native as N

    return {f: e.get_field(getattr(N, f)).copy() for f in fields}


def _same_fields(a, b, what, fields=FIELDS):
    sa, sb = _snapshot(a, fields), _snapshot(b, fields)
    for f in fields:
        assert sa[f].dtype == sb[f].dtype and sa[f].tobytes() == sb[f].tobytes(), (what, f, int(np.sum(sa[f] != sb[f])))


def _single_ticks(e, T, gain, cpars):
    """T calls of rcg_control_tick_nominal (k_sim* then k_nominal each)."""
    from rcognita_amd import _native as N

    pars = (C.c_double * len(cpars))(*cpars) if len(cpars) else None
    for _ in range(T):
        N.check(N.lib().rcg_control_tick_nominal(e._h, float(gain), pars), e._h)


def _ticks(e, T, gain, cpars):
    """rcg_control_ticks_nominal (the Engine routes T > 1 there; T = 1 is the single tick it always was)."""
    from rcognita_amd import _native as N

    if T > 1:
        e.control_tick_nominal(gain, ctrl_pars=cpars, T=T)
    else:
        pars = (C.c_double * len(cpars))(*cpars) if len(cpars) else None
        N.check(N.lib().rcg_control_ticks_nominal(e._h, 1, float(gain), pars), e._h)


# ---- 1. the law against the twins ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("B", [70, 150])
@pytest.mark.parametrize("key", ["a", "b", "c"])
def test_nominal_action_against_the_twin(key, B, dtype):
    from rcognita_amd import _native as N

    S, (gain, cp) = twin_of(key), law_args(key)
    e = _engine(key, dtype, B)
    x, p = _start(key, e, B)
    r = f32_round if dtype == "f32" else (lambda a: np.asarray(a, dtype=np.float64))
    y = r(S.out(x))  # the observation handed in, as the handle's element type holds it
    u_want = S.law(y, gain, cp, p)
    for clip in (False, True):
        want = S.clip(u_want) if clip else u_want
        got = e.nominal_action(y, gain, ctrl_pars=cp, clip=clip)
        assert got.shape == (B, S.du)
        if dtype == "f64":
            err = _err(got, want)
            print(f"law {key} B={B} f64 clip={clip}: {err:.3e}")
            assert err < LAW_TOL, (clip, err)
        else:
            d = ulp32_distance(got, want)
            print(f"law {key} B={B} f32 clip={clip}: {d.max():.3f} ulp")
            assert np.all(d <= 1.0), (clip, d.max())
        assert np.any(S.clip(u_want) != u_want) and (not clip or np.all(got == S.clip(got.astype(float))))
        assert e.last_launch()["kernel"] == "k_nominal" and e.last_launch()["variant"] == 0
    if key == "c":
        with pytest.raises(N.NativeError) as ei:
            e.nominal_action(y, gain, want_lyap=True)
        assert ei.value.code == N.ERR_UNSUPPORTED and "nominal_lf" in str(ei.value)
    else:
        a2, L = e.nominal_action(y, gain, ctrl_pars=cp, want_lyap=True)
        Lw = S.lf(y, gain, cp)
        if dtype == "f64":
            assert _err(L, Lw) < LAW_TOL and np.array_equal(a2, e.nominal_action(y, gain, ctrl_pars=cp))
        else:
            assert np.all(ulp32_distance(L, Lw) <= 1.0)
        with pytest.raises(N.NativeError) as ei:
            e.nominal_action(y, gain, ctrl_pars=None)
        assert ei.value.code == N.ERR_BAD_ARG and "NOMINAL_NP" in str(ei.value)
    progs = [ex for pr, ex in N.system_programs(reg(key)["sys_id"]) if pr.endswith("_nominal.hip")]
    assert f"rcg::k_nominal<rcg::RcgRtcSys, {'double' if dtype == 'f64' else 'float'}>" in progs, progs
    e.close()


# ---- 2. single ticks against the twin loop ----------------------------------------------------------------------------------------
def _loop_case(key, dtype, B, T=20, target=None):
    from rcognita_amd import _native as N

    S, (gain, cp) = twin_of(key), law_args(key)
    kw = {} if target is None else dict(observation_target=target)
    e = _engine(key, dtype, B, **kw)
    x, p = _start(key, e, B)
    u, acc = _held_action(S, B, dtype), np.zeros(B)
    for t in range(T):
        e.control_tick_nominal(gain, ctrl_pars=cp)
        x, u, acc = twin_tick(S, x, u, acc, gain, cp, R1_of(key), target=target, pars=p if (key == "c" or dtype == "f32") else None)
    errs = {"state": _err(e.get_state(), x), "action": _err(e.get_field(N.FIELD_ACTION), u), "accum": _err(e.get_field(N.FIELD_ACCUM), acc)}
    print(f"loop {key} B={B} {dtype} target={target is not None}: {errs}")
    assert errs["state"] < RK4_TOL[dtype] and errs["action"] < RK4_TOL[dtype] and errs["accum"] < TOL[dtype], errs
    np.testing.assert_array_equal(e.get_field(N.FIELD_STEP_IDX), np.full(B, T, np.int32))
    assert _tick_count(e) == T
    assert e.last_launch()["kernel"] == "k_nominal" and e.last_launch(N.KERNEL_SIM)["kernel"] == "k_sim"
    e.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("B", [70, 150])
@pytest.mark.parametrize("key", ["a", "b", "c"])
def test_twenty_nominal_ticks_against_the_twin_loop(key, B, dtype):
    _loop_case(key, dtype, B)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_twenty_nominal_ticks_with_a_target(dtype):
    _loop_case("b", dtype, 70, target=TARGET_B)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_three_nominal_ticks_under_the_disturbance_model(dtype):
    """The env step is k_sim_dist: against the composition of tests/user_systems.py::rhs_full (rhs, then `disturb`, and the filter)."""
    from rcognita_amd import _native as N

    B, key = 70, "a_dist"
    S, (gain, cp) = twin_of(key), law_args(key)
    e = _engine(key, dtype, B, is_disturb=True, pars_disturb=[SIGMA, MU, TAU], disturb_init=[0.3], seed=5)
    r = f32_round if dtype == "f32" else (lambda a: np.asarray(a, dtype=np.float64))
    x, p = _start(key, e, B)
    q, sub = np.broadcast_to(r([0.3]), (B, 1)), np.zeros(B, np.int32)
    u, acc = _held_action(S, B, dtype), np.zeros(B)
    for _ in range(3):
        e.control_tick_nominal(gain, ctrl_pars=cp)
        x, u, acc, q, sub = twin_tick(S, x, u, acc, gain, cp, R1_of(key), pars=p if dtype == "f32" else None,
                                      dist=dict(q=q, sub=sub, ep=np.zeros(B, np.int32), sigma=r(SIGMA), mu=r(MU), tau=r(TAU), seed=5))
    assert e.last_launch(N.KERNEL_SIM)["kernel"] == "k_sim_dist" and e.last_launch()["kernel"] == "k_nominal"
    errs = {"state": _err(e.get_state(), x), "disturb": _err(e.get_field(N.FIELD_DISTURB), q),
            "action": _err(e.get_field(N.FIELD_ACTION), u), "accum": _err(e.get_field(N.FIELD_ACCUM), acc)}
    print(f"disturbed loop {dtype}: {errs}")
    assert max(errs["state"], errs["disturb"], errs["action"]) < RK4_TOL[dtype] and errs["accum"] < TOL[dtype], errs
    np.testing.assert_array_equal(e.get_field(N.FIELD_SUBSTEP_IDX), sub)
    e.close()


# ---- 3. (and the copies' share of 4.) copies of the robots against the built-ins, in a child process -----------------------------------
def _copies_compare():
    """The child: Sys3WRobotNI / Sys3WRobot against copies whose `nominal` restates the built-in law; raises on the first difference."""
    from rcognita_amd import Engine
    from rcognita_amd import _native as N
    from tests.helpers import PRESETS, engine_cfg, rand_states

    copies = {"3wrobotNI": N.register_system("UserRobotNINom", robot_copy_source("Sys3WRobotNI", "UserRobotNINom"), 3, 2, 0),
              "3wrobot": N.register_system("UserRobotNom", robot_copy_source("Sys3WRobot", "UserRobotNom"), 5, 2, 2)}
    assert all(i["nominal"] == 1 and i["has_ticks"] for i in copies.values())
    assert copies["3wrobot"]["nominal_np"] == 2 and copies["3wrobotNI"]["nominal_np"] == 0
    checked = 0
    for name, gain in (("3wrobotNI", 0.5), ("3wrobot", 5.0)):
        cp = tuple(PRESETS[name]["pars"])
        for dtype in ("f64", "f32"):
            for B in (70, 150):
                def make(sid):
                    c = engine_cfg(name, B, dtype)
                    c.sys_id = sid
                    return Engine(c)

                a, b, b1 = make(N.SYS_IDS[name]), make(copies[name]["sys_id"]), make(copies[name]["sys_id"])
                x0 = rand_states(np.random.default_rng(3), name, B)
                for clip in (False, True):
                    ua = a.nominal_action(x0, gain, ctrl_pars=cp or None, clip=clip)
                    ub = b.nominal_action(x0, gain, ctrl_pars=cp, clip=clip)
                    assert ua.tobytes() == ub.tobytes(), (name, dtype, B, clip, int(np.sum(ua != ub)))
                for e in (a, b, b1):
                    e.set_state(x0)
                for t in range(6):  # single ticks: fields and launch records
                    a.control_tick_nominal(gain, ctrl_pars=cp or None)
                    b.control_tick_nominal(gain, ctrl_pars=cp)
                    for f in FIELDS:
                        assert a.get_field(getattr(N, f)).tobytes() == b.get_field(getattr(N, f)).tobytes(), (name, dtype, B, t, f)
                    for kind in (N.KERNEL_ACTOR, N.KERNEL_SIM):
                        assert a.last_launch(kind) == b.last_launch(kind), (name, dtype, B, t, kind)
                # the copy's six ticks in ONE launch (a policy with `nominal` and TICKS): the same bits
                b1.control_tick_nominal(gain, ctrl_pars=cp, T=6)
                ll = b1.last_launch()
                assert ll["kernel"] == "k_nominal" and ll["variant"] & 1, ll
                for f in FIELDS:
                    assert a.get_field(getattr(N, f)).tobytes() == b1.get_field(getattr(N, f)).tobytes(), (name, dtype, B, "T=6", f)
                checked += 1
                for e in (a, b, b1):
                    e.close()
    print("copies bit-identical:", checked, "handles")


def test_copies_of_the_robots_are_bit_identical_to_the_builtins():
    env = {k: v for k, v in os.environ.items() if k != "PYTHONPATH"}
    code = "import sys; sys.path.insert(0, %r); import tests.test_hip_user_system_nominal as t; t._copies_compare(); " \
           "assert 'torch' not in sys.modules" % ROOT
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "bit-identical" in r.stdout


# ---- 4. T ticks in one launch against T single ticks ------------------------------------------------------------------------------
def _builtin_engine(name, dtype, B, **kw):
    from rcognita_amd import Engine
    from tests.helpers import engine_cfg

    return Engine(engine_cfg(name, B, dtype, **kw))


def _ticks_case(make, start, gain, cp, T, persistent, what):
    from rcognita_amd import _native as N

    one, many = make(), make()
    for e in (one, many):
        start(e)
    for rnd in range(2):  # the second round after an episode reset on both
        _single_ticks(one, T, gain, cp)
        _ticks(many, T, gain, cp)
        ll = many.last_launch()
        assert ll["kernel"] == "k_nominal" and bool(ll["variant"] & 1) == persistent, (what, ll)
        assert one.last_launch()["variant"] == 0
        _same_fields(one, many, (what, rnd))
        assert _tick_count(many) == T and _tick_count(one) == T, (what, _tick_count(many))
        np.testing.assert_array_equal(many.get_field(N.FIELD_STEP_IDX), np.full(many.B, T, np.int32))
        for e in (one, many):
            e.episode_reset()
    one.close()
    many.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("T", [1, 2, 7])
@pytest.mark.parametrize("B", [70, 150])
@pytest.mark.parametrize("key", ["a", "b", "c"])
def test_T_ticks_in_one_launch_equal_T_single_ticks(key, B, T, dtype):
    gain, cp = law_args(key)
    kw = dict(observation_target=TARGET_B) if (key == "b" and B == 150) else {}
    _ticks_case(lambda: _engine(key, dtype, B, **kw), lambda e: _start(key, e, B), gain, cp, T, True, (key, B, T, dtype))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("T", [1, 2, 7])
@pytest.mark.parametrize("B", [70, 150])
@pytest.mark.parametrize("name,gain", [("3wrobotNI", 0.5), ("3wrobot", 5.0)])
def test_T_ticks_in_one_launch_equal_T_single_ticks_builtin(name, gain, B, T, dtype):
    from tests.helpers import PRESETS, rand_states

    x0 = rand_states(np.random.default_rng(3), name, B)
    _ticks_case(lambda: _builtin_engine(name, dtype, B), lambda e: e.set_state(x0), gain, tuple(PRESETS[name]["pars"]) or (), T, True,
                (name, B, T, dtype))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_without_TICKS_and_under_the_disturbance_model_the_ticks_are_single_ticks(dtype):
    gain, cp = law_args("a")
    _ticks_case(lambda: _engine("a_noticks", dtype, 70), lambda e: _start("a_noticks", e, 70), gain, cp, 7, False, "no TICKS")
    dist = dict(is_disturb=True, pars_disturb=[SIGMA, MU, TAU], seed=5)
    _ticks_case(lambda: _engine("a_dist", dtype, 70, **dist), lambda e: _start("a_dist", e, 70), gain, cp, 2, False, "disturbed")
    _ticks_case(lambda: _disturbed_builtin(dtype), lambda e: e.set_state(np.tile([1.0, -2.0, 0.5], (70, 1))), 0.5, (), 2, False, "disturbed built-in")


def _disturbed_builtin(dtype):
    from rcognita_amd import Engine
    from tests.helpers import engine_cfg

    c = engine_cfg("3wrobotNI", 70, dtype)
    c.is_disturb, c.pars_disturb, c.seed = True, [[2.0, 1.0], [0.5, -0.25], [1.5, 0.7]], 5
    return Engine(c)


# ---- 5. a frozen env ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_a_frozen_env_in_one_launch_as_in_single_ticks(dtype):
    """(a) at B = 150 with the bad state (finite; its first RK4 step is not) in env 37 and in env 149, the last lane of the ragged
    wave: frozen by the first tick's env step, then not stepped, still decided for, counted and charged - T = 7 in one launch
    as 7 single ticks.  (The pendulum offers no later freeze at the preset step: its clean states stay finite under every held
    action - test_user_system_loop_register.py - so a tank-style freeze at a later tick does not exist for it.)"""
    from rcognita_amd import _native as N

    B, T, bad = 150, 7, [37, 149]
    gain, cp = law_args("a")
    x0 = pend_batch(B)
    xb = x0.copy()
    xb[bad] = bad_state(dtype)
    one, many, clean = (_engine("a", dtype, B) for _ in range(3))
    for e, x in ((one, xb), (many, xb), (clean, x0)):
        e.set_state(x)
    _single_ticks(one, T, gain, cp)
    _ticks(many, T, gain, cp)
    _ticks(clean, T, gain, cp)
    assert many.last_launch()["variant"] & 1
    _same_fields(one, many, "frozen")
    st = many.get_field(N.FIELD_STATUS)
    want = np.zeros(B, np.uint32)
    want[bad] = 1
    np.testing.assert_array_equal(st, want)
    np.testing.assert_array_equal(many.get_field(N.FIELD_STEP_IDX), np.full(B, T, np.int32))  # counted
    assert many.get_state()[bad].tobytes() == xb.astype(many.real)[bad].tobytes()  # not stepped
    assert np.all(np.isfinite(many.get_field(N.FIELD_ACTION)[bad]))  # decided for: the clipped law of the frozen state
    assert not np.any(np.isfinite(many.get_field(N.FIELD_ACCUM)[bad]))  # charged: the frozen rate's square overflows
    ok = np.setdiff1d(np.arange(B), bad)
    for f in FIELDS:  # the neighbours are the clean batch's envs
        assert many.get_field(getattr(N, f))[ok].tobytes() == clean.get_field(getattr(N, f))[ok].tobytes(), f
    for e in (one, many, clean):
        e.close()


# ---- 6. refusals with nothing moved -----------------------------------------------------------------------------------------------
def test_refusals_move_nothing():
    from rcognita_amd import _native as N
    from tests.helpers import rand_states

    L = N.lib()
    two = (C.c_double * 2)(*CPARS)
    # a policy without the member: all three entry points, by name
    e = _engine("plain", "f64", 70)
    e.set_state(pend_batch(70))
    dev = e.empty((2, 70))
    snap = _snapshot(e)
    calls = {"rcg_nominal_action": lambda: L.rcg_nominal_action(e._h, C.c_void_p(dev.ptr), C.c_void_p(dev.ptr), None, 70, GAIN, two, 0),
             "rcg_control_tick_nominal": lambda: L.rcg_control_tick_nominal(e._h, GAIN, two),
             "rcg_control_ticks_nominal": lambda: L.rcg_control_ticks_nominal(e._h, 3, GAIN, two)}
    for who, call in calls.items():
        assert call() == N.ERR_UNSUPPORTED, who
        msg = N.last_error(e._h)
        assert who in msg and "nominal" in msg.replace(who, "") and "PendulumT" in msg, msg
        now = _snapshot(e)
        assert all(now[f].tobytes() == snap[f].tobytes() for f in FIELDS), who
        assert _tick_count(e) == 0
    e.close()
    # Sys2Tank; T = 0 on a handle that has the law
    tank = _builtin_engine("2tank", "f64", 70)
    tank.set_state(rand_states(np.random.default_rng(1), "2tank", 70))
    snap = _snapshot(tank)
    assert L.rcg_control_ticks_nominal(tank._h, 3, 1.0, None) == N.ERR_UNSUPPORTED
    assert L.rcg_control_tick_nominal(tank._h, 1.0, None) == N.ERR_UNSUPPORTED
    assert all(_snapshot(tank)[f].tobytes() == snap[f].tobytes() for f in FIELDS)
    tank.close()
    for make in (lambda: _engine("a", "f64", 70), lambda: _builtin_engine("3wrobotNI", "f64", 70)):
        e = make()
        snap = _snapshot(e)
        for T in (0, -3):
            assert L.rcg_control_ticks_nominal(e._h, T, GAIN, two) == N.ERR_BAD_ARG
        assert all(_snapshot(e)[f].tobytes() == snap[f].tobytes() for f in FIELDS) and _tick_count(e) == 0
        e.close()
    # missing controller parameters are refused before the env is stepped
    e = _engine("a", "f64", 70)
    e.set_state(pend_batch(70))
    snap = _snapshot(e)
    assert L.rcg_control_tick_nominal(e._h, GAIN, None) == N.ERR_BAD_ARG
    assert L.rcg_control_ticks_nominal(e._h, 2, GAIN, None) == N.ERR_BAD_ARG
    assert all(_snapshot(e)[f].tobytes() == snap[f].tobytes() for f in FIELDS)
    e.close()


# ---- 7. CtrlNominal in the reference's loop order ------------------------------------------------------------------------------------
def test_ctrl_nominal_in_the_reference_loop():
    from rcognita_amd import controllers
    from rcognita_amd.systems import System

    class PendulumNom(System):
        hip_policy = pendulum_nominal_source("PendulumNom")

    class PendulumT(System):
        hip_policy = PENDULUM

    mk = lambda cls: cls(sys_type="diff_eqn", dim_state=2, dim_input=1, dim_output=2, dim_disturb=0, pars=PEND_PARS,  # noqa: E731
                         ctrl_bnds=BND)
    sys_ = mk(PendulumNom)
    with pytest.raises(NotImplementedError, match="nominal"):
        controllers.CtrlNominal(mk(PendulumT), GAIN, CPARS)
    with pytest.raises(ValueError, match="NOMINAL_NP"):
        controllers.CtrlNominal(sys_, GAIN, ())
    ctrl = controllers.CtrlNominal(sys_, GAIN, CPARS, ctrl_bnds=BND, t0=0, sampling_time=DT)
    assert ctrl.action_curr.shape == (1,)
    S = PendTwin()
    # presets/main_3wrobot.py:415-468: sim step under the held action, observe, ctrl_selector, receive_action
    x = pend_batch(1)[0]
    xs, u, t = x[None].copy(), np.zeros((1, 1)), 0.0
    for k in range(50):
        xs, u_tw, _ = twin_tick(S, xs, u, np.zeros(1), GAIN, CPARS, np.eye(3))
        t += DT
        act = controllers.ctrl_selector(t, xs[0], np.zeros(1), ctrl, None, "nominal")
        assert act.shape == (1,) and _err(act, u_tw[0]) < LAW_TOL, k
        u = u_tw
    assert np.all(np.abs(u) <= 5.0) and abs(t - 0.5) < 1e-9
    # between samples the action is held; the unclipped law and the Lyapunov value; batched observations; reset
    held = ctrl.compute_action(t + 0.25 * DT, np.array([0.3, -0.1]))
    assert np.array_equal(held, act)
    yb = pend_batch(9)
    assert _err(ctrl.compute_action_vanila(yb), S.law(yb, GAIN, CPARS)) < LAW_TOL and ctrl.action_curr.shape == (9, 1)
    assert _err(ctrl.compute_LF(yb), S.lf(yb, GAIN, CPARS)) < LAW_TOL
    assert _err(ctrl.compute_action(t + 2 * DT, yb), S.clip(S.law(yb, GAIN, CPARS))) < LAW_TOL
    ctrl.reset(0.0)
    assert ctrl.ctrl_clock == 0.0 and np.array_equal(ctrl.action_curr, np.zeros(1))


# ---- 8. rate ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["3wrobotNI", "a"])
def test_one_launch_is_not_slower_than_the_loop_of_single_ticks(which):
    """B = 1024, T = 64, median of five on the same build: the one-launch form removes 2 T - 1 launches and does the same
    arithmetic, so a ratio below 1 is a defect.  No other bar."""
    B, T = 1024, 64
    if which == "a":
        e, (gain, cp) = _engine("a", "f32", B), law_args("a")
        e.set_state(pend_batch(B))
    else:
        from tests.helpers import rand_states

        e, gain, cp = _builtin_engine(which, "f32", B), 0.5, ()
        e.set_state(rand_states(np.random.default_rng(3), which, B))

    def timed(fn):
        fn()
        e.synchronize()
        ts = []
        for _ in range(5):
            t0 = time.perf_counter()
            fn()
            e.synchronize()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts))

    t_loop = timed(lambda: _single_ticks(e, T, gain, cp))
    t_one = timed(lambda: _ticks(e, T, gain, cp))
    assert e.last_launch()["variant"] & 1
    print(f"{which}: {T} single ticks {t_loop * 1e6:.0f} us, one launch {t_one * 1e6:.0f} us, ratio {t_loop / t_one:.2f}")
    assert t_loop / t_one >= 1.0, (t_loop, t_one)
    e.close()
