"""The nominal control law on systems compiled at run time (rcg.h: the policy member `nominal`): what a registration reports,
refuses and compiles - hipRTC compiles without a device, so these run on CPU - and, in NumPy, the conditions of the inputs that
test_hip_user_system_nominal.py runs on the GPU."""
import numpy as np
import pytest

from rcognita_amd import _native as N
from tests.nominal_laws import (BND, C2_GAIN, CPARS, DT, GAIN, PEND_PARS, C2Twin, PendTwin, bad_state, c2_batch, corner_c2, pend_batch,
                                pendulum_nominal_source, pendulum_out_nominal_source, twin_tick)
from tests.test_user_system_loop_register import pend_rk4
from tests.test_user_system_register import PENDULUM, _register
from tests.test_user_system_ticks_register import with_ticks


def _mask(sid):
    v = N.C.c_int32(-1)
    rc = N.lib().rcg_system_has_nominal(sid, N.C.byref(v))
    return rc, v.value


def test_the_symbols_are_exported_and_the_version_stays_125():
    for s in ("rcg_system_has_nominal", "rcg_control_ticks_nominal"):
        assert s in N.SYMBOLS and hasattr(N.lib(), s)
    assert N.RCG_VERSION == 125 and N.lib().rcg_version() == 125


def test_registration_reports_the_law():
    a = N.register_system("PendulumNom", pendulum_nominal_source("PendulumNom"), 2, 1, 3)
    assert a["nominal"] == 3 and a["nominal_np"] == 2 and a["has_ticks"] and _mask(a["sys_id"]) == (N.OK, 3)
    nolf = N.register_system("PendulumNomNoLf", pendulum_nominal_source("PendulumNomNoLf", lf=False, ticks=False), 2, 1, 3)
    assert nolf["nominal"] == 1 and nolf["nominal_np"] == 2 and not nolf["has_ticks"] and _mask(nolf["sys_id"]) == (N.OK, 1)
    b = N.register_system("PendulumYNom", pendulum_out_nominal_source("PendulumYNom"), 2, 1, 3)
    assert b["nominal"] == 3 and b["dy"] == 3 and b["has_out"] and _mask(b["sys_id"]) == (N.OK, 3)
    src, S = corner_c2()
    c = N.register_system(S.name, src, S.ds, S.du, S.np)
    assert c["nominal"] == 1 and c["nominal_np"] == 0 and _mask(c["sys_id"]) == (N.OK, 1)
    plain = N.register_system("PendulumT", PENDULUM, 2, 1, 3)
    assert plain["nominal"] == 0 and plain["nominal_np"] == 0 and _mask(plain["sys_id"]) == (N.OK, 0)
    assert _mask(N.SYS_3WROBOT) == (N.OK, 3) and _mask(N.SYS_3WROBOT_NI) == (N.OK, 3) and _mask(N.SYS_2TANK) == (N.OK, 0)
    assert _mask(7)[0] == N.ERR_BAD_ARG and _mask(-1)[0] == N.ERR_BAD_ARG and _mask(N.SYS_USER_BASE + 4096)[0] == N.ERR_BAD_ARG
    assert N.lib().rcg_system_has_nominal(N.SYS_3WROBOT, None) == N.ERR_BAD_ARG
    assert N.lib().rcg_system_has_nominal(a["sys_id"], None) == N.ERR_BAD_ARG


def test_hip_info_carries_the_law():
    from rcognita_amd.systems import System

    class PendulumNom(System):
        hip_policy = pendulum_nominal_source("PendulumNom")

    class PendulumT(System):
        hip_policy = PENDULUM

    for cls, mask, n in ((PendulumNom, 3, 2), (PendulumT, 0, 0)):
        cls(sys_type="diff_eqn", dim_state=2, dim_input=1, dim_output=2, dim_disturb=0, pars=PEND_PARS, ctrl_bnds=BND)
        assert cls._hip_info["nominal"] == mask and cls._hip_info["nominal_np"] == n


def test_nominal_np_beyond_eight_is_unsupported():
    rc, _, log = _register("PendulumNom9", pendulum_nominal_source("PendulumNom9", nominal_np=9), 2, 1, 3)
    assert rc == N.ERR_UNSUPPORTED and "NOMINAL_NP" in log, log
    rc, _, _ = _register("PendulumNom8", pendulum_nominal_source("PendulumNom8", nominal_np=8), 2, 1, 3)
    assert rc == N.OK


@pytest.mark.parametrize("name,kw,member", [("PendulumLfOnly", dict(law=False, nominal_np=None), "nominal_lf"),
                                            ("PendulumNpOnly", dict(law=False, lf=False), "NOMINAL_NP")])
def test_a_member_without_the_law_is_refused_by_name(name, kw, member):
    from rcognita_amd.systems import System

    src = pendulum_nominal_source(name, **kw)
    rc, _, log = _register(name, src, 2, 1, 3)
    assert rc == N.ERR_BAD_ARG and f"{name} defines {member} but no nominal member" in log, log
    cls = type(name, (System,), dict(hip_policy=src))
    with pytest.raises(ValueError, match=f"defines {member} but no nominal member"):
        cls(sys_type="diff_eqn", dim_state=2, dim_input=1, dim_output=2, dim_disturb=0, pars=PEND_PARS, ctrl_bnds=BND)


def test_the_member_adds_nothing_to_a_registration():
    """rcg_system_programs right after rcg_register_system: the same core expressions with and without the law (k_nominal and
    k_ticks_nominal are compiled the first time a handle needs them)."""
    ia = N.register_system("PendulumNom", pendulum_nominal_source("PendulumNom"), 2, 1, 3)
    ib = N.register_system("PendulumK", with_ticks(PENDULUM.replace("PendulumT", "PendulumK")), 2, 1, 3)
    core = lambda i: [(p.replace(i["name"], "X"), e) for p, e in N.system_programs(i["sys_id"])  # noqa: E731
                      if p in (i["name"] + "_f32.hip", i["name"] + "_f64.hip")]
    assert len(core(ib)) > 20 and not any("nominal" in e for _, e in core(ia))
    assert core(ia) == core(ib)
    pa = N.system_programs(ia["sys_id"])
    assert all("_f32.hip" not in p and "_f64.hip" not in p for p, _ in pa[len(core(ia)):])


# ---- the GPU file's inputs, in NumPy ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [70, 150])
def test_the_clip_is_active_on_some_envs_and_inactive_on_others(B):
    for S, x, gain, cp, p in ((PendTwin(), pend_batch(B), GAIN, CPARS, None), (PendTwin(out=True), pend_batch(B), GAIN, CPARS, None),
                              (C2Twin(), *c2_batch(B)[:1], C2_GAIN, (), c2_batch(B)[1])):
        u = S.law(S.out(x), gain, cp, p)
        clipped = np.any(u != S.clip(u), axis=-1)
        assert 0.1 * B < clipped.sum() < 0.9 * B, (type(S).__name__, clipped.sum())


def test_the_lyapunov_value_falls_over_the_closed_loop_of_the_pendulum():
    S = PendTwin()
    big = PendTwin()
    big.bnds = np.array([[-1e3, 1e3]])  # the unclipped law: V' = -gain om^2 <= 0 along it (c2 scales V, c1 th^2 is its potential)
    x = pend_batch(70)
    R1 = np.diag([10.0, 1.0, 0.5])
    for T in (big, S):
        xs, u, acc = x.copy(), np.zeros((70, 1)), np.zeros(70)
        xs, u, acc = twin_tick(T, xs, u, acc, GAIN, CPARS, R1)  # (the first tick holds the zero start action)
        v0 = T.lf(xs, GAIN, (CPARS[0], 1.0))
        for _ in range(200):
            xs, u, acc = twin_tick(T, xs, u, acc, GAIN, CPARS, R1)
        v1 = T.lf(xs, GAIN, (CPARS[0], 1.0))
        if T is big:
            assert np.all(v1 < v0)
        assert np.mean(v1) < 0.5 * np.mean(v0)
    assert np.allclose(S.lf(x, GAIN, CPARS), CPARS[1] * S.lf(x, GAIN, (CPARS[0], 1.0)) + (1 - CPARS[1]) * 0.5 * x[:, 1] ** 2)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_the_bad_state_leaves_the_first_step_non_finite(dtype):
    real = np.float32 if dtype == "f32" else np.float64
    x = bad_state(dtype).astype(real)
    assert np.all(np.isfinite(x))
    assert not np.all(np.isfinite(pend_rk4(x[None], np.array([[0.0]]), DT, real)))
    assert np.all(np.isfinite(pend_rk4(pend_batch(150).astype(real), np.full((150, 1), 5.0), DT, real)))
