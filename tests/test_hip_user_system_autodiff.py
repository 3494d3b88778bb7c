"""Derived adjoints (rcg.h: the policy member AUTODIFF) on the GPU: jac_T / out_jac_T generated from rhs / out on forward-mode
dual numbers (rcg_dual.hpp), and everything that asks for jac_T running on them.

1. rcg_jac_T: the derived members against the NumPy twins (the pendulum, the corners C1-C4 of tests/user_systems.py), the
   hand-written members of the same policies and the three built-ins (oracle.rcg_oracle.state_jac_T) by the same call.
2. The optimiser on derived members against the oracle's per-iteration twin (pendulum, C1).
3. The optimiser on C2, C3, C4 (both members derived) from the reference's F17 (s) starts against SLSQP.
4. A hand-written member wins; the derived run is deterministic.
5. One critic mode: RQL on derived C3.
6. The fused loop step on the LOOP pendulum whose jac_T is derived.
7. Refusals of a policy with neither the member nor the opt-in: unchanged.

Tolerances are the project's for the same quantities (test_hip_user_system.py, test_hip_user_system_corners.py): the HW forms of
the operators 1e-12 / 2e-5, costs 1e-11 / 1e-5, the oracle twin's as test_pendulum_optimizer_against_the_oracle_twin has them.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.test_hip_user_system_corners import RHS_TOL, TOL, _engine, _err, _note, _r, _snapshot, _unchanged  # noqa: E402
from tests.test_hip_user_system_corners import FIELDS as CORNER_FIELDS  # noqa: E402
from tests.test_user_system_register import PENDULUM  # noqa: E402
from tests.user_systems import actor_cost, case_cost, corner, load_f17, search_weights  # noqa: E402
from tests.user_systems_autodiff import corner_ad, pendulum_ad, pendulum_loop_ad, with_autodiff  # noqa: E402

pytestmark = pytest.mark.gpu

PEND_PARS = [1.3, 9.81, 0.7]
BND = np.array([[-5.0, 5.0]])
KEYS = ("C1", "C2", "C3", "C4")
_REG = {}


def reg(key):
    """Each policy registered once per process.  pend / C1 .. C4: rhs (and out) alone, with AUTODIFF; pend-hand / C1-hand ..:
    the same policies with their hand-written members; pend-both: hand-written jac_T kept, AUTODIFF added; loop: the LOOP + SEARCH
    pendulum without jac_T, with AUTODIFF; neither: no jac_T, no opt-in."""
    from rcognita_amd import _native as N

    if key not in _REG:
        if key in KEYS:
            src, S = corner_ad(key)
            _REG[key] = N.register_system(S.name, src, S.ds, S.du, S.np)
        elif key.endswith("-hand") and key[:2] in KEYS:
            _REG[key] = corner(key[:2]).register()
        else:
            nojac = PENDULUM[: PENDULUM.index("  template <typename real, bool HW = false>\n  __device__ __forceinline__ static "
                                              "void jac_T")] + "};\n"
            name, src = {"pend": ("PendulumAD", pendulum_ad("PendulumAD")),
                         "pend-hand": ("PendulumG", PENDULUM.replace("PendulumT", "PendulumG")),
                         "pend-both": ("PendulumHAD", with_autodiff(PENDULUM.replace("PendulumT", "PendulumHAD"))),
                         "loop": ("PendulumLAD", pendulum_loop_ad("PendulumLAD")),
                         "neither": ("PendulumNoJac", nojac.replace("PendulumT", "PendulumNoJac"))}[key]
            _REG[key] = N.register_system(name, src, 2, 1, 3)
    return _REG[key]


def _pend_engine(key, dtype, B, Nh=10, **kw):
    from rcognita_amd import Engine, EngineConfig

    cfg = dict(sys_id=reg(key)["sys_id"], batch=B, dtype=dtype, Nactor=Nh, pars=PEND_PARS, ctrl_bnds=BND, R1=np.diag([10.0, 1.0, 0.1]),
               dt_sim=0.01, sampling_time=0.01, pred_step_size=0.02)
    cfg.update(kw)
    return Engine(EngineConfig(**cfg))


def _corner_engine(key, dtype, B, Nh, R1, hand=False, **kw):
    k = key + "-hand" if hand else key
    return _engine({key: reg(k)}, key, dtype, B, Nh, R1, **kw)


def _pend_states(rng, n):
    return np.stack([rng.uniform(-3, 3, n), rng.uniform(-2, 2, n)], axis=-1)


def _pend_jac_T(x, lam, pars=PEND_PARS):
    """pend_oracle's formulas (test_hip_user_system.py), batched."""
    m, g, l = pars
    return (np.stack([-g / l * np.cos(x[:, 0]) * lam[:, 1], lam[:, 0]], axis=-1), lam[:, 1:2] / (m * l * l))


def _worst(d, ref):
    return float(np.max(np.abs(np.asarray(d, dtype=float) - ref) / np.maximum(np.abs(ref), 1.0)))


# ---- 1. rcg_jac_T ------------------------------------------------------------------------------------------------------------------
N_POINTS = 257


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_jac_T_of_the_pendulum_against_the_numpy_twin(dtype):
    rng = np.random.default_rng(11)
    x, u = _pend_states(rng, N_POINTS), rng.uniform(-5, 5, (N_POINTS, 1))
    lam, gy = rng.uniform(-1, 1, (N_POINTS, 2)), rng.uniform(-1, 1, (N_POINTS, 2))
    got = {}
    for key in ("pend", "pend-hand"):
        e = _pend_engine(key, dtype, 8)
        r = _r(e)
        ax, bu, gx = e.jac_T(x, u, lam, gy)
        ax_ref, bu_ref = _pend_jac_T(r(x), r(lam))
        err = max(_worst(ax, ax_ref), _worst(bu, bu_ref))
        _note("autodiff 1 jac_T", key, dtype, "(ax, bu)", err)
        assert err < RHS_TOL[dtype], (key, err)
        np.testing.assert_array_equal(gx, gy.astype(e.real))  # no output map: the observation is the state
        ax2, bu2 = e.jac_T(x, u, lam)  # without gy
        np.testing.assert_array_equal(ax2, ax)
        np.testing.assert_array_equal(bu2, bu)
        got[key] = (ax, bu)
        e.close()
    assert reg("pend")["autodiff"] == 1 and reg("pend-hand")["autodiff"] == 0
    _note("autodiff 1 jac_T", "pend", dtype, "derived against hand-written", max(_worst(got["pend"][0], got["pend-hand"][0]),
                                                                               _worst(got["pend"][1], got["pend-hand"][1])))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("key", KEYS)
def test_jac_T_of_the_corners_against_the_numpy_twins(key, dtype):
    """Both members derived (C1 has no output map), per-env parameters on C2 (n is the handle's batch)."""
    from rcognita_amd import _native as N

    S = corner(key)
    rng = np.random.default_rng([12, KEYS.index(key)])
    n = N_POINTS
    x, u = S.rand_states(rng, n), S.rand_actions(rng, (n,))
    lam, gy = rng.uniform(-1, 1, (n, S.ds)), rng.uniform(-1, 1, (n, S.dy))
    pars = np.array(S.pars) * rng.uniform(0.8, 1.2, (n, S.np)) if key == "C2" else None
    R1 = np.eye(S.dy + S.du)
    assert reg(key)["autodiff"] == (3 if S.has_out else 1) and reg(key + "-hand")["autodiff"] == 0
    for hand in (False, True):
        e = _corner_engine(key, dtype, n, 5, R1, hand=hand, per_env_pars=pars is not None)
        r = _r(e)
        if pars is not None:
            e.set_field(N.FIELD_PARS, pars)
        ax, bu, gx = e.jac_T(x, u, lam, gy)
        ax_ref, bu_ref = S.jac_T(r(x), r(u), r(lam), r(pars))
        gx_ref = S.out_jac_T(r(x), r(gy))
        errs = (_worst(ax, ax_ref), _worst(bu, bu_ref), _worst(gx, gx_ref))
        _note("autodiff 1 jac_T", key, dtype, f"{'hand-written' if hand else 'derived'} (ax, bu, gx) {errs}", max(errs))
        assert max(errs) < RHS_TOL[dtype], (key, hand, errs)
        if pars is not None:  # the nominal parameters give other products
            assert _worst(ax, S.jac_T(r(x), r(u), r(lam))[0]) > 1e3 * RHS_TOL[dtype]
        e.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", ["3wrobot", "3wrobotNI", "2tank"])
def test_jac_T_of_the_builtins_against_the_oracle(name, dtype):
    from oracle import rcg_oracle as O
    from rcognita_amd import Engine
    from tests.helpers import PRESETS, engine_cfg, rand_actions, rand_states

    rng = np.random.default_rng(13)
    n = N_POINTS
    e = Engine(engine_cfg(name, 8, dtype))
    r = _r(e)
    x, u = rand_states(rng, name, n), rand_actions(rng, name, (n,))
    lam, gy = rng.uniform(-1, 1, (n, e.ds)), rng.uniform(-1, 1, (n, e.ds))
    ax, bu, gx = e.jac_T(x, u, lam, gy)
    ref = [O.state_jac_T(PRESETS[name]["sys_id"], r(x)[i], r(u)[i], PRESETS[name]["pars"], r(lam)[i]) for i in range(n)]
    ax_ref, bu_ref = np.stack([a for a, _ in ref]), np.stack([b for _, b in ref])
    err = max(_worst(ax, ax_ref), _worst(bu, bu_ref))
    _note("autodiff 1 jac_T", name, dtype, "built-in (ax, bu)", err)
    assert err < RHS_TOL[dtype], err
    np.testing.assert_array_equal(gx, gy.astype(e.real))
    e.close()


# ---- 2. the optimiser against the oracle's twin ------------------------------------------------------------------------------------
def _patch_oracle(monkeypatch, sid, dims, dyn, jac):
    """The oracle with one more system (as test_hip_user_system.py::pend_oracle patches the pendulum in; nothing under oracle/
    changes)."""
    from oracle import rcg_oracle as O

    dyn0, jac0 = O.state_dyn, O.state_jac_T
    monkeypatch.setattr(O, "state_dyn", lambda s, x, u, p: dyn(x, u, p) if s == sid else dyn0(s, x, u, p))
    monkeypatch.setattr(O, "state_jac_T", lambda s, x, u, p, lam: jac(x, u, p, lam) if s == sid else jac0(s, x, u, p, lam))
    monkeypatch.setitem(O.SYS_DIMS, sid, dims)
    return O


def _pend_dyn(state, action, pars):
    x, u, p = (np.asarray(v, dtype=np.float64) for v in (state, action, pars))
    m, g, l = p[..., 0], p[..., 1], p[..., 2]
    d = np.zeros(np.broadcast_shapes(x.shape[:-1], u.shape[:-1], p.shape[:-1]) + (2,))
    d[..., 0] = x[..., 1]
    d[..., 1] = u[..., 0] / (m * l * l) - g / l * np.sin(x[..., 0])
    return d


def _check_against_the_twin(O, e, cfg, x, dtype, memory, what):
    e.set_state(x)
    e.set_optimizer(memory)
    act, U, J, its = e.actor_optimize(iters=10)
    from tests.helpers import assert_kernel

    assert_kernel(e, "k_actor_opt")
    np.testing.assert_array_equal(act, U[:, 0, :])
    xr = _r(e)(x)
    err = _err(J, O.actor_cost(U.astype(np.float64), xr, xr, cfg))
    _note("autodiff 2 twin", what, dtype, f"memory {memory} BEST_J", err)
    assert err < (1e-10 if dtype == "f64" else 1e-5), err
    U_or, J_or, its_or = O.actor_optimize(cfg, xr, xr, O.action_sqn_init(cfg), iters=10, memory=memory)
    eJ, eU = _err(J, J_or), float(np.max(np.abs(U - U_or) / 5.0))
    _note("autodiff 2 twin", what, dtype, f"memory {memory} J against the oracle twin (U {eU:.3e})", eJ)
    if dtype == "f64":
        assert np.all(np.abs(its - its_or) <= 3)
        assert eJ < 1e-9 and eU < 1e-5, (eJ, eU)
    else:
        assert eJ < 2e-4, eJ


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("memory", [0, 4])
def test_pendulum_optimizer_on_the_derived_jac_T_against_the_oracle_twin(dtype, memory, monkeypatch):
    sid = reg("pend")["sys_id"]
    O = _patch_oracle(monkeypatch, sid, (2, 1, 3), _pend_dyn,
                      lambda x, u, p, lam: (np.array([-p[1] / p[2] * np.cos(x[0]) * lam[1], lam[0]]),
                                            np.array([lam[1] / (p[0] * p[2] * p[2])])))
    B, Nh = 64, 10
    e = _pend_engine("pend", dtype, B, Nh)
    cfg = O.OracleCfg(sys_id=sid, n_actor=Nh, gamma=1.0, pred_step_size=0.02, dt_sim=0.01, sampling_time=0.01, pars=PEND_PARS,
                      ctrl_bnds=BND, R1=np.diag([10.0, 1.0, 0.1]))
    _check_against_the_twin(O, e, cfg, _pend_states(np.random.default_rng(6), B), dtype, memory, "pend")
    e.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("memory", [0, 4])
def test_c1_optimizer_on_the_derived_jac_T_against_the_oracle_twin(dtype, memory, monkeypatch):
    meta, z = load_f17()
    S, sid = corner("C1"), reg("C1")["sys_id"]
    O = _patch_oracle(monkeypatch, sid, (1, 1, 0), lambda x, u, p: S.rhs(np.asarray(x, float), np.asarray(u, float)),
                      lambda x, u, p, lam: S.jac_T(x, u, lam))
    B, Nh, R1 = 64, 10, z["C1_R1_diag"]
    e = _corner_engine("C1", dtype, B, Nh, R1)
    cfg = O.OracleCfg(sys_id=sid, n_actor=Nh, pred_step_size=meta["pred_step_size"], dt_sim=0.01, sampling_time=meta["sampling_time"],
                      pars=[], ctrl_bnds=S.bnds, R1=R1)
    _check_against_the_twin(O, e, cfg, S.rand_states(np.random.default_rng(61), B), dtype, memory, "C1")
    e.close()


# ---- 3. the optimiser with both members derived, against SLSQP ---------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("memory", [0, 4])
@pytest.mark.parametrize("key", ["C2", "C3", "C4"])
def test_optimizer_on_derived_members_against_slsqp_on_the_f17_starts(key, memory, dtype):
    """test_hip_user_system_corners.py::test_optimizer_against_slsqp_on_the_f17_starts on the policies without their adjoint
    members: the same inputs, the same bars."""
    from tests.helpers import assert_kernel

    meta, z = load_f17()
    S = corner(key)
    assert reg(key)["autodiff"] == 3
    x, R1, Nh = z[f"{key}_s_state"], z[f"{key}_R1_diag"], meta["Nactor"]
    B = len(x)
    assert B == 8
    e = _corner_engine(key, dtype, B, Nh, R1)
    r = _r(e)
    e.set_state(x)
    e.set_optimizer(memory)
    cost = lambda U: actor_cost(S, U[:, None].astype(float), S.out(r(x)), r(x), R1, 1.0, None, meta["pred_step_size"])[:, 0]  # noqa: E731
    Js = {}
    for iters in (5, 30):
        act, U, J, _ = e.actor_optimize(iters=iters)
        assert_kernel(e, "k_actor_opt")
        np.testing.assert_array_equal(act, U[:, 0, :])
        assert np.all(U >= S.bnds[:, 0] - 1e-4) and np.all(U <= S.bnds[:, 1] + 1e-4)
        err = _err(J, cost(U))
        _note("autodiff 3 optimiser", key, dtype, f"memory {memory} iters {iters} BEST_J", err)
        assert err < TOL[dtype], (iters, err)
        Js[iters] = J.astype(float)
    J0 = z[f"{key}_s_J_init"]
    slack = 4 * TOL[dtype] * np.maximum(np.abs(J0), 1.0)
    assert np.all(Js[30] <= Js[5] + slack) and np.all(Js[5] <= J0 + slack)
    Jopt = z[f"{key}_s_J_opt"]
    gap = (Js[30] - Jopt) / np.abs(Jopt)
    _note("autodiff 3 optimiser", key, dtype, f"memory {memory} worst J / J_slsqp - 1", float(np.max(gap)))
    assert np.all(Js[30] <= Jopt + np.abs(Jopt) * 5e-3), gap
    e.close()


# ---- 4. hand-written wins; the derived run is deterministic ------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_a_hand_written_jac_T_wins_over_the_opt_in(dtype):
    """The policy that keeps jac_T and adds AUTODIFF runs its own member: the bits of the registration without the opt-in."""
    assert reg("pend-both")["autodiff"] == 0 and reg("pend-both")["has_jac"]
    B = 64
    x = _pend_states(np.random.default_rng(6), B)
    a, b = _pend_engine("pend-both", dtype, B), _pend_engine("pend-hand", dtype, B)
    rng = np.random.default_rng(3)
    pts = (_pend_states(rng, N_POINTS), rng.uniform(-5, 5, (N_POINTS, 1)), rng.uniform(-1, 1, (N_POINTS, 2)))
    for u, v in zip(a.jac_T(*pts), b.jac_T(*pts)):
        assert u.tobytes() == v.tobytes()
    for e in (a, b):
        e.set_state(x)
    for memory in (0, 4):
        for iters in (5, 30):
            for e in (a, b):
                e.set_optimizer(memory)
            for u, v in zip(a.actor_optimize(iters), b.actor_optimize(iters)):
                assert u.tobytes() == v.tobytes(), (memory, iters)
    a.close()
    b.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_the_derived_run_is_deterministic(dtype):
    meta, z = load_f17()
    x, R1 = z["C2_s_state"], z["C2_R1_diag"]
    runs = []
    for _ in range(2):
        e = _corner_engine("C2", dtype, len(x), meta["Nactor"], R1)
        e.set_state(x)
        e.set_optimizer(4)
        runs.append([e.actor_optimize(5), e.actor_optimize(30)])
        e.close()
    for ra, rb in zip(*runs):
        for u, v in zip(ra, rb):
            assert u.tobytes() == v.tobytes()


# ---- 5. one critic mode ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_rql_optimizer_on_derived_c3(dtype):
    """RQL, quad-nomix: dQ/dy of the terminal critic reaches the sequence through the derived out_jac_T."""
    from rcognita_amd import _native as N
    from tests.helpers import assert_kernel

    meta, z = load_f17()
    S, cs = corner("C3"), "quad-nomix"
    B, Nh = 29, meta["Nactor"]
    x = S.rand_states(np.random.default_rng([7, 2]), B)
    w = search_weights("C3", cs, B)
    c = dict(mode="RQL", cs=cs, R1=z["C3_R1_diag"], gamma=meta["gamma_critic"], target=None, w=None)
    e = _corner_engine("C3", dtype, B, Nh, c["R1"], mode="RQL", critic_struct=cs, Ncritic=meta["Ncritic"],
                       buffer_size=meta["buffer_size"], gamma=c["gamma"])
    r = _r(e)
    e.set_field(N.FIELD_W_CRITIC, w)
    e.set_state(x)
    cost = lambda U: case_cost(S, c, meta, U[:, None].astype(float), xs=r(x), ys=S.out(r(x)), w=r(w))[:, 0]  # noqa: E731
    act, U, J, _ = e.actor_optimize(iters=10)
    assert_kernel(e, "k_actor_opt")
    err = _err(J, cost(U))
    _note("autodiff 5 RQL", "C3", dtype, "BEST_J", err)
    assert err < TOL[dtype], err
    J0 = cost(np.tile(S.bnds[:, 0] / 10.0, (B, Nh, 1)).astype(e.real))  # the reference's start (action_sqn_init)
    slack = 4 * TOL[dtype] * np.maximum(np.abs(J0), 1.0)
    assert np.all(J.astype(float) <= J0 + slack)
    assert np.any(J.astype(float) < J0 - 1e-3 * np.abs(J0))  # (it moved)
    e.close()


# ---- 6. the fused loop -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("B", [1, 33])
def test_loop_step_decides_on_the_derived_jac_T(B, dtype):
    """The LOOP pendulum without jac_T is served steps only (test_hip_user_system_loop.py); with AUTODIFF its fused decision runs,
    and every row of 20 iterations equals the separate calls bit for bit."""
    from rcognita_amd import _native as N
    from tests.test_hip_user_system_loop import DT, _compare
    from tests.test_user_system_loop_register import clean_states

    info = reg("loop")
    assert info["has_loop"] and info["has_jac"] and info["autodiff"] == 1
    kw = dict(Nh=5, R1=np.diag(np.linspace(10.0, 0.5, 3)), dt_sim=DT, sampling_time=DT, pred_step_size=2 * DT)
    a, b = _pend_engine("loop", dtype, B, **kw), _pend_engine("loop", dtype, B, **kw)
    x0 = clean_states(B)
    for e in (a, b):
        e.set_state(x0)
    _compare(a, b, np.tile(BND[:, 0] / 10.0, (B, 1)), DT / 2, "MPC", nits=20, tag=f"autodiff loop B={B} {dtype}")
    ll = a.last_launch(N.KERNEL_ACTOR)
    assert ll["kernel"] == "k_actor_opt" and ll["variant"] & 8, ll
    real = "double" if dtype == "f64" else "float"
    progs = [ex for p, ex in N.system_programs(info["sys_id"]) if p.endswith("_loop.hip")]
    assert f"rcg::k_actor_opt<rcg::RcgRtcSys, {real}, false, false, false, true>" in progs, progs
    a.close()
    b.close()


def test_drop_in_loop_fuses_on_the_derived_jac_T():
    """Simulator + CtrlOptPred(actor_opt='auto') on the same policy: the controller takes the optimiser and the loop fuses; every
    row equals the run by the separate calls."""
    from rcognita_amd.systems import System
    from tests import test_hip_user_system_loop as L

    class PendulumLAD(System):
        hip_policy = pendulum_loop_ad("PendulumLAD")

    L._classes()["autodiff"] = PendulumLAD
    try:
        my_sys, my_ctrl, my_sim = L._objects("autodiff", "MPC", "quad-nomix")
        assert PendulumLAD._hip_info["autodiff"] == 1 and my_ctrl._can_fuse(my_sim) is True
        T = 20
        fused, c1 = L._run("autodiff", "MPC", "quad-nomix", True, T)
        plain, c0 = L._run("autodiff", "MPC", "quad-nomix", False, T)
    finally:
        del L._classes()["autodiff"]
    np.testing.assert_array_equal(fused, plain)
    assert c0.fused_steps == 0 and c0.fused_decisions == 0
    assert c1.fused_steps >= T - 2 and c1.fused_decisions >= T // 2 - 1, (c1.fused_steps, c1.fused_decisions)
    assert np.ptp(fused[:, 1]) > 1e-3  # the pendulum moved


def test_ctrl_opt_pred_takes_the_optimiser_with_the_opt_in_and_refuses_without():
    from rcognita_amd.controllers import CtrlOptPred
    from rcognita_amd.systems import System

    class PendulumAD(System):
        hip_policy = pendulum_ad("PendulumAD")

    class PendulumNoJac(System):
        hip_policy = PENDULUM[: PENDULUM.index("  template <typename real, bool HW = false>\n  __device__ __forceinline__ static void "
                                               "jac_T")].replace("PendulumT", "PendulumNoJac") + "};\n"

    def ctrl(cls, **kw):
        s = cls(sys_type="diff_eqn", dim_state=2, dim_input=1, dim_output=2, dim_disturb=0, pars=PEND_PARS, ctrl_bnds=BND)
        return CtrlOptPred(1, 2, mode="MPC", ctrl_bnds=BND, Nactor=10, sys_rhs=s._state_dyn, sys_out=s.out, state_sys=np.zeros(2),
                           stage_obj_pars=[np.diag([10.0, 1.0, 0.0])], **kw)

    for how in ("auto", "gradient"):
        c = ctrl(PendulumAD, actor_opt=how)
        a = c.compute_action(0.0, np.array([0.5, 0.0]))
        assert np.all(np.isfinite(a)) and c._rt_fuse is False  # (decides; no LOOP in this policy)
    assert PendulumAD._hip_info["autodiff"] == 1
    with pytest.raises(NotImplementedError, match="AUTODIFF"):
        ctrl(PendulumNoJac, actor_opt="auto")


# ---- 7. refusals unchanged ---------------------------------------------------------------------------------------------------------
def test_a_policy_with_neither_member_nor_opt_in_is_refused_and_nothing_moves():
    from rcognita_amd import _native as N

    info = reg("neither")
    assert not info["has_jac"] and info["autodiff"] == 0
    B = 16
    e = _pend_engine("neither", "f64", B)
    e.set_state(_pend_states(np.random.default_rng(2), B))
    e.sim_step(1)
    snap = _snapshot(e, CORNER_FIELDS)
    rng = np.random.default_rng(4)
    calls = {"rcg_actor_optimize": lambda: e.actor_optimize(5), "rcg_control_tick_opt": lambda: e.control_tick_opt(5),
             "rcg_jac_T": lambda: e.jac_T(_pend_states(rng, B), rng.uniform(-5, 5, (B, 1)), rng.uniform(-1, 1, (B, 2)))}
    for who, call in calls.items():
        with pytest.raises(N.NativeError) as ei:
            call()
        assert ei.value.code == N.ERR_UNSUPPORTED and "jac_T" in str(ei.value) and "PendulumNoJac" in str(ei.value), (who, str(ei.value))
        _unchanged(e, snap, who)
    assert "AUTODIFF" in N.last_error(e._h)  # (rcg_jac_T's text names the opt-in)
    assert not any("k_jac_T" in ex or "k_actor_opt" in ex for _, ex in N.system_programs(info["sys_id"]))
    e.close()
