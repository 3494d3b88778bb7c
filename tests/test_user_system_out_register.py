"""Systems compiled at run time with an output map y = out(x) (rcg.h: DY, out, out_jac_T): registration on CPU, and the NumPy
restatement of the reference's _actor_cost with `out` that the GPU tests (test_hip_user_system_out.py) compare against, pinned
here on the reference's own results (tests/golden/F14_output_map_pendulum.npz, tools/gen_output_map_fixture.py)."""
import json
import os

import numpy as np
import pytest

from rcognita_amd import _native as N
from tests.test_user_system_register import PENDULUM

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "F14_output_map_pendulum.npz")

# the output map of the fixture: y = (sin th, cos th, om), its adjoint gx = (d out / d x)^T gy
_OUT_MEMBERS = r"""
  template <typename real, bool HW = false>
  __device__ __forceinline__ static void out(const Pre<real>&, const real* x, real* y) {
    real s, c;
    sincos_sel<real, HW>(x[0], &s, &c);
    y[0] = s;
    y[1] = c;
    y[2] = x[1];
  }
"""
_OUT_JAC_MEMBERS = r"""
  template <typename real, bool HW = false>
  __device__ __forceinline__ static void out_jac_T(const Pre<real>&, const real* x, const real* gy, real* gx) {
    real s, c;
    sincos_sel<real, HW>(x[0], &s, &c);
    gx[0] = c * gy[0] - s * gy[1];
    gx[1] = gy[2];
  }
"""


def pendulum_out_source(name, dy=3, out=True, out_jac=True):
    """The pendulum of test_user_system_register.py with `static constexpr int DY = dy;` and the members asked for."""
    src = PENDULUM.replace("PendulumT", name)
    src = src.replace("static constexpr int DS = 2, DU = 1, NP = 3;", "static constexpr int DS = 2, DU = 1, NP = 3;\n"
                      f"  static constexpr int DY = {dy};")
    tail = src.rindex("};")
    return src[:tail] + (_OUT_MEMBERS if out else "") + (_OUT_JAC_MEMBERS if out_jac else "") + src[tail:]


PENDULUM_OUT = pendulum_out_source("PendulumY")


# ---- NumPy restatement of the reference ------------------------------------------------------------------------------------
def pend_rhs(x, u, pars):
    m, g, l = pars
    return np.array([x[1], -g / l * np.sin(x[0]) + u[0] / (m * l * l)])


def pend_out(x):
    x = np.asarray(x, dtype=float)
    return np.stack([np.sin(x[..., 0]), np.cos(x[..., 0]), x[..., 1]], axis=-1)


def actor_cost_out(x0, y0, seq, R1, gamma, target, h, pars):
    """CtrlOptPred._actor_cost, MPC (controllers.py:1284-1303) with sys_out = pend_out: observation_sqn[0] = observation,
    observation_sqn[k] = sys_out(state) after each Euler step (:1290-1296); J = sum_k gamma^k stage_obj (:1300-1303) over
    chi = [y - target, u] (:1069-1072), chi @ R1 @ chi (:1076-1078)."""
    u = np.asarray(seq, dtype=float).reshape(-1, 1)
    x = np.asarray(x0, dtype=float)
    ys = [np.asarray(y0, dtype=float)]
    for k in range(1, len(u)):
        x = x + h * pend_rhs(x, u[k - 1], pars)
        ys.append(pend_out(x))
    J = 0.0
    for k in range(len(u)):
        chi = np.concatenate([ys[k] if target is None else ys[k] - target, u[k]])
        J += gamma ** k * (chi @ R1 @ chi)
    return J


def load_f14():
    z = np.load(GOLDEN)
    return json.loads(str(z["meta"])), z


# ---- registration ----------------------------------------------------------------------------------------------------------
def _register(name, src, ds=2, du=1, np_=3):
    sid = N.C.c_int32(-1)
    rc = N.lib().rcg_register_system(name.encode(), src.encode(), ds, du, np_, N.C.byref(sid))
    return rc, sid.value, N.last_error(None)


def _output_info(sid):
    dy, o, oj = N.C.c_int32(-1), N.C.c_int32(-1), N.C.c_int32(-1)
    rc = N.lib().rcg_system_output_info(sid, N.C.byref(dy), N.C.byref(o), N.C.byref(oj))
    return rc, (dy.value, o.value, oj.value)


def test_registration_reports_the_output_map():
    info = N.register_system("PendulumY", PENDULUM_OUT, 2, 1, 3)
    assert (info["dy"], info["has_out"], info["has_out_jac"], info["has_jac"]) == (3, True, True, True)
    assert N.SYS_DIMS[info["sys_id"]] == (2, 1, 3) and N.sys_dy(info["sys_id"]) == 3
    assert _output_info(info["sys_id"]) == (N.OK, (3, 1, 1))
    info = N.register_system("PendulumYNoJac", pendulum_out_source("PendulumYNoJac", out_jac=False), 2, 1, 3)
    assert (info["dy"], info["has_out"], info["has_out_jac"], info["has_jac"]) == (3, True, False, True)
    # an output map of the state's own dimension
    info = N.register_system("PendulumY2", pendulum_out_source("PendulumY2", dy=2).replace("y[2] = x[1];", ""), 2, 1, 3)
    assert (info["dy"], info["has_out"]) == (2, True)


def test_builtins_and_plain_policies_observe_their_state():
    for sid, ds in ((N.SYS_3WROBOT, 5), (N.SYS_3WROBOT_NI, 3), (N.SYS_2TANK, 2)):
        assert _output_info(sid) == (N.OK, (ds, 0, 0))
    info = N.register_system("PendulumT", PENDULUM, 2, 1, 3)
    assert (info["dy"], info["has_out"], info["has_out_jac"]) == (2, False, False)
    assert _output_info(info["sys_id"]) == (N.OK, (2, 0, 0))
    assert N.lib().rcg_system_output_info(N.SYS_USER_BASE + 999, None, None, None) == N.ERR_BAD_ARG


def test_dy_beyond_the_limit_is_unsupported_and_dy_without_out_is_bad_arg():
    rc, _, log = _register("PendulumY6", pendulum_out_source("PendulumY6", dy=N.MAX_DS + 1))
    assert rc == N.ERR_UNSUPPORTED, log
    rc, _, log = _register("PendulumY0", pendulum_out_source("PendulumY0", dy=0))
    assert rc == N.ERR_UNSUPPORTED, log
    rc, _, log = _register("PendulumYNoOut", pendulum_out_source("PendulumYNoOut", out=False, out_jac=False))
    assert rc == N.ERR_BAD_ARG
    assert "DY differs from DS" in log and "PendulumYNoOut" in log, log


def test_hip_policy_class_takes_dim_output_from_the_policy():
    from rcognita_amd.systems import System

    class PendulumOutSys(System):
        hip_policy = pendulum_out_source("PendulumOutSys")

    s = PendulumOutSys(sys_type="diff_eqn", dim_state=2, dim_input=1, dim_output=3, dim_disturb=0, pars=[1.3, 9.81, 0.7])
    assert (s.dim_state, s.dim_output) == (2, 3)
    assert PendulumOutSys._hip_info["has_out"]
    for dy in (2, 4):
        with pytest.raises(ValueError):
            PendulumOutSys(sys_type="diff_eqn", dim_state=2, dim_input=1, dim_output=dy, dim_disturb=0, pars=[1.3, 9.81, 0.7])

    class PendulumOutPy(System):  # a Python out cannot run on the device: the policy's member is the way
        hip_policy = pendulum_out_source("PendulumOutPy")

        def out(self, state, action=[]):
            return pend_out(state)

    with pytest.raises(NotImplementedError, match="hip_policy") as e:
        PendulumOutPy(sys_type="diff_eqn", dim_state=2, dim_input=1, dim_output=3, dim_disturb=0, pars=[1.3, 9.81, 0.7])
    assert "`out` member" in str(e.value)


# ---- the restatement against the reference --------------------------------------------------------------------------------
def test_restatement_reproduces_the_reference_actor_cost_with_out():
    meta, z = load_f14()
    h, pars = meta["pred_step_size"], meta["pars"]
    assert len(meta["cases"]) == z["a_J"].shape[0] == 12
    lags = set()
    for ci, case in enumerate(meta["cases"]):
        target = z["a_target"][ci] if case["cost"] == "target" else None
        lags.add(case["lag"])
        for i in range(z["a_J"].shape[1]):
            J = actor_cost_out(z["a_state_sys"][ci, i], z["a_obs"][ci, i], z["a_seq"][ci, i], z["a_R1"][ci], case["gamma"],
                               target, h, pars)
            ref = z["a_J"][ci, i]
            assert abs(J - ref) <= 1e-13 * max(1.0, abs(ref)), (case, i, J, ref)
        if not case["lag"]:  # observation = out(state_sys)
            np.testing.assert_allclose(z["a_obs"][ci], pend_out(z["a_state_sys"][ci]), rtol=0, atol=1e-15)
    assert lags == {False, True}
    # (b): the SLSQP optimum is a cost of the same function
    for i in range(len(z["b_J_opt"])):
        x = z["b_state"][i]
        J = actor_cost_out(x, pend_out(x), z["b_seq_opt"][i], z["b_R1"], 1.0, None, h, pars)
        assert abs(J - z["b_J_opt"][i]) <= 1e-13 * max(1.0, abs(z["b_J_opt"][i]))
        assert z["b_J_opt"][i] <= z["b_J_init"][i]


def test_ctrl_without_out_jac_needs_candidates_at_construction():
    """A policy with out and jac_T but no out_jac_T has no optimiser: CtrlOptPred refuses the optimiser path when it is built
    (before any device work), as it does for a policy without jac_T."""
    from rcognita_amd.controllers import CtrlOptPred
    from rcognita_amd.systems import System

    class PendulumOutNoJacSys(System):
        hip_policy = pendulum_out_source("PendulumOutNoJacSys", out_jac=False)

    s = PendulumOutNoJacSys(sys_type="diff_eqn", dim_state=2, dim_input=1, dim_output=3, dim_disturb=0, pars=[1.3, 9.81, 0.7],
                            ctrl_bnds=np.array([[-5.0, 5.0]]))
    info = PendulumOutNoJacSys._hip_info
    assert info["has_jac"] and info["has_out"] and not info["has_out_jac"]
    with pytest.raises(NotImplementedError, match="out_jac_T"):
        CtrlOptPred(1, 3, mode="MPC", ctrl_bnds=np.array([[-5.0, 5.0]]), Nactor=10, sys_rhs=s._state_dyn, sys_out=s.out,
                    state_sys=np.zeros(2), stage_obj_pars=[np.diag([5.0, 5.0, 0.5, 0.1])], actor_opt="auto")
