"""RQL / SQL on systems compiled at run time (rcg.h: the policy member CRITIC): registration on CPU, and the NumPy restatement of
the reference's _critic, _critic_cost and RQL / SQL _actor_cost with an output map that the GPU tests
(test_hip_user_system_critic.py) compare against, pinned here on the reference's own results
(tests/golden/F15_user_system_critic.npz, tools/gen_user_system_critic_fixture.py)."""
import json
import os

import numpy as np
import pytest

from rcognita_amd import _native as N
from rcognita_amd.engine import EngineConfig
from tests.test_user_system_out_register import pend_out, pend_rhs, pendulum_out_source
from tests.test_user_system_register import PENDULUM

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "F15_user_system_critic.npz")
STRUCTS = ("quad-lin", "quadratic", "quad-nomix", "quad-mix")
CRITIC_MEMBER = "  static constexpr bool CRITIC = true;\n"


def with_critic(src):
    """A policy source with the opt-in member added behind its dimensions."""
    i = src.index("static constexpr int DS")
    j = src.index("\n", i) + 1
    return src[:j] + CRITIC_MEMBER + src[j:]


def pendulum_critic_source(name, tgt=False):
    """The pendulum with y = (sin th, cos th, om) (F14) that opts in to the critic kernels; `tgt`: with `TGT = true`, the
    member that says its handles usually carry an observation target (the k_actor_dma instances are compiled for that setting)."""
    src = with_critic(pendulum_out_source(name))
    return src.replace(CRITIC_MEMBER, CRITIC_MEMBER + "  static constexpr bool TGT = true;\n") if tgt else src


def load_f15():
    z = np.load(GOLDEN)
    return json.loads(str(z["meta"])), z


# ---- NumPy restatement of the reference ------------------------------------------------------------------------------------
def dim_critic(cs, dy, du):
    """controllers.py:1024-1039 with dim_output + dim_input."""
    n = dy + du
    return {"quad-lin": n * (n + 1) // 2 + n, "quadratic": n * (n + 1) // 2, "quad-nomix": n, "quad-mix": dy + dy * du + du}[cs]


def critic_regressor(cs, y, u, target):
    """controllers.py:1200-1212: over chi = [y - target, u]; quad-mix over the raw observation."""
    y, u = np.asarray(y, dtype=float), np.asarray(u, dtype=float)
    chi = np.concatenate([y if target is None else y - target, u])
    if cs in ("quad-lin", "quadratic"):
        tri = np.outer(chi, chi)[np.triu_indices(len(chi))]  # uptria2vec: row-major upper triangle (utilities.py:81-96)
        return np.concatenate([tri, chi]) if cs == "quad-lin" else tri
    if cs == "quad-nomix":
        return chi * chi
    return np.concatenate([y ** 2, np.kron(y, u), u ** 2])


def critic(cs, y, u, w, target):
    return float(np.asarray(w, dtype=float) @ critic_regressor(cs, y, u, target))


def stage(y, u, R1, target):
    chi = np.concatenate([np.asarray(y, float) if target is None else np.asarray(y, float) - target, np.asarray(u, float)])
    return float(chi @ R1 @ chi)


def critic_cost(cs, w, w_prev, obs_buf, act_buf, n_critic, gamma, R1, target):
    """controllers.py:1216-1245 on the oldest Ncritic buffer rows."""
    Jc = 0.0
    for k in range(n_critic - 1, 0, -1):
        e = (critic(cs, obs_buf[k - 1], act_buf[k - 1], w, target) - gamma * critic(cs, obs_buf[k], act_buf[k], w_prev, target)
             - stage(obs_buf[k - 1], act_buf[k - 1], R1, target))
        Jc += 0.5 * e * e
    return Jc


def td_system(cs, w_prev, obs_buf, act_buf, n_critic, gamma, R1, target):
    """_critic_cost as a linear least squares, Jc(w) = 1/2 |A w - b|^2 (oracle/rcg_oracle.py::critic_td_system)."""
    A = np.stack([critic_regressor(cs, obs_buf[r], act_buf[r], target) for r in range(n_critic - 1)])
    b = np.array([gamma * critic(cs, obs_buf[r + 1], act_buf[r + 1], w_prev, target) + stage(obs_buf[r], act_buf[r], R1, target)
                  for r in range(n_critic - 1)])
    return A, b


def actor_cost_critic(mode, cs, x0, y0, seq, w, R1, gamma, target, h, pars):
    """CtrlOptPred._actor_cost in RQL / SQL (controllers.py:1284-1328) with sys_out = pend_out."""
    u = np.asarray(seq, dtype=float).reshape(-1, 1)
    x = np.asarray(x0, dtype=float)
    ys = [np.asarray(y0, dtype=float)]
    for k in range(1, len(u)):
        x = x + h * pend_rhs(x, u[k - 1], pars)
        ys.append(pend_out(x))
    J = 0.0
    if mode == "RQL":
        for k in range(len(u) - 1):
            J += gamma ** k * stage(ys[k], u[k], R1, target)
        return J + critic(cs, ys[-1], u[-1], w, target)
    for k in range(len(u)):
        J += critic(cs, ys[k], u[k], w, target)
    return J


def _close(a, b, tol=1e-12):
    return abs(a - b) <= tol * max(1.0, abs(b))


def test_restatement_reproduces_the_reference_critic_with_out():
    meta, z = load_f15()
    tgt, R1, g, nc = np.array(meta["target"]), np.diag(meta["R1"]), meta["gamma"], meta["Ncritic"]
    h, pars = meta["pred_step_size"], meta["pars"]
    rows = 0
    for cs in STRUCTS:
        k = cs.replace("-", "_")
        assert meta["dim_critic"][cs] == dim_critic(cs, 3, 1) == z[f"c_{k}_w"].shape[1]
        for i in range(len(z[f"c_{k}_Q"])):
            assert _close(critic(cs, z[f"c_{k}_obs"][i], z[f"c_{k}_act"][i], z[f"c_{k}_w"][i], tgt), z[f"c_{k}_Q"][i]), (cs, i)
            rows += 1
        for i in range(len(z[f"d_{k}_Jc"])):
            Jc = critic_cost(cs, z[f"d_{k}_w"][i], z[f"d_{k}_w_prev"][i], z[f"d_{k}_obs_buf"][i], z[f"d_{k}_act_buf"][i], nc, g, R1, tgt)
            assert _close(Jc, z[f"d_{k}_Jc"][i]), (cs, i)
            A, b = td_system(cs, z[f"d_{k}_w_prev"][i], z[f"d_{k}_obs_buf"][i], z[f"d_{k}_act_buf"][i], nc, g, R1, tgt)
            r = A @ z[f"d_{k}_w"][i] - b
            assert _close(0.5 * float(r @ r), z[f"d_{k}_Jc"][i], 1e-11), (cs, i)
            rows += 1
        for mode in ("RQL", "SQL"):
            p = f"e_{mode}_{k}"
            assert not np.allclose(z[p + "_obs"], pend_out(z[p + "_state_sys"]))  # state_sys != the observed state
            for i in range(len(z[p + "_J"])):
                J = actor_cost_critic(mode, cs, z[p + "_state_sys"][i], z[p + "_obs"][i], z[p + "_seq"][i], z[p + "_w"][i], R1, g, tgt,
                                      h, pars)
                assert _close(J, z[p + "_J"][i]), (mode, cs, i)
                rows += 1
        # (f): SLSQP's Jc is the cost of its w, never above the start point's; (g): SLSQP's optimum is a cost of the same function
        for i in range(len(z[f"f_{k}_Jc"])):
            Jc = critic_cost(cs, z[f"f_{k}_w"][i], z[f"f_{k}_w_prev"][i], z[f"f_{k}_obs_buf"][i], z[f"f_{k}_act_buf"][i], nc, g, R1, tgt)
            assert _close(Jc, z[f"f_{k}_Jc"][i], 1e-11) and z[f"f_{k}_Jc"][i] <= z[f"f_{k}_Jc_init"][i] * (1 + 1e-9), (cs, i)
            rows += 1
        for i in range(len(z[f"g_{k}_J_opt"])):
            x = z[f"g_{k}_state"][i]
            J = actor_cost_critic("RQL", cs, x, pend_out(x), z[f"g_{k}_seq_opt"][i], z[f"g_{k}_w"][i], R1, g, tgt, h, pars)
            assert _close(J, z[f"g_{k}_J_opt"][i]) and z[f"g_{k}_J_opt"][i] <= z[f"g_{k}_J_init"][i], (cs, i)
            rows += 1
    assert rows >= 400


# ---- registration ----------------------------------------------------------------------------------------------------------
def _has_critic(sid):
    v = N.C.c_int32(-1)
    rc = N.lib().rcg_system_has_critic(sid, N.C.byref(v))
    return rc, v.value


def test_registration_reports_has_critic():
    info = N.register_system("PendulumYC", pendulum_critic_source("PendulumYC"), 2, 1, 3)
    assert info["has_critic"] and info["has_out"] and info["dy"] == 3
    assert _has_critic(info["sys_id"]) == (N.OK, 1)
    plain = N.register_system("PendulumT", PENDULUM, 2, 1, 3)
    assert not plain["has_critic"] and _has_critic(plain["sys_id"]) == (N.OK, 0)
    # CRITIC = false is the default spelled out
    off = N.register_system("PendulumCOff", with_critic(PENDULUM.replace("PendulumT", "PendulumCOff")).replace("= true", "= false"), 2, 1, 3)
    assert not off["has_critic"]
    for sid in (N.SYS_3WROBOT, N.SYS_3WROBOT_NI, N.SYS_2TANK):
        assert _has_critic(sid) == (N.OK, 1)
    assert N.lib().rcg_system_has_critic(N.SYS_USER_BASE + 999, None) == N.ERR_BAD_ARG


def _registration_expressions(has_out, has_jac):
    """The name expressions a registration compiled before CRITIC existed, in their order: per element type k_rhs, k_stage_obj,
    k_sim x target, k_out with an output map, k_actor (streamed / generated x generic / diagonal x target, and the DIRECT
    long-row form), k_actor_opt x 8 when the optimiser's adjoint is complete."""
    S = "rcg::RcgRtcSys"
    tf = lambda b: "true" if b else "false"  # noqa: E731
    out = []
    for prog, real in (("_f32.hip", "float"), ("_f64.hip", "double")):
        e = [f"rcg::k_rhs<{S}, {real}>", f"rcg::k_stage_obj<{S}, {real}>", f"rcg::k_sim<{S}, {real}, false>",
             f"rcg::k_sim<{S}, {real}, true>"]
        if has_out:
            e.append(f"rcg::k_out<{S}, {real}>")
        for g in (False, True):
            for t in (False, True):
                for s in (False, True):
                    e.append(f"rcg::k_actor<{S}, {real}, {tf(g)}, {tf(t)}, {tf(s)}>")
                if g:
                    e.append(f"rcg::k_actor<{S}, {real}, true, {tf(t)}, true, false, true>")
        if has_jac:
            for sel in range(8):
                e.append(f"rcg::k_actor_opt<{S}, {real}, {tf(sel & 2)}, {tf(sel & 4)}, {tf(sel & 1)}>")
        out += [(prog, x) for x in e]
    return out


def test_a_policy_without_critic_compiles_what_it_compiled_before():
    for name, src, has_out in (("PendulumT", PENDULUM, False), ("PendulumY", pendulum_out_source("PendulumY"), True)):
        info = N.register_system(name, src, 2, 1, 3)
        want = [(name + p, e) for p, e in _registration_expressions(has_out, True)]
        assert N.system_programs(info["sys_id"]) == want
    # ... and the opt-in adds nothing to the registration either: the critic programs are compiled on first use
    info = N.register_system("PendulumYC", pendulum_critic_source("PendulumYC"), 2, 1, 3)
    assert N.system_programs(info["sys_id"]) == [("PendulumYC" + p, e) for p, e in _registration_expressions(True, True)]
    need = N.C.c_int64(0)
    assert N.lib().rcg_system_programs(N.SYS_2TANK, None, 0, N.C.byref(need)) == N.ERR_BAD_ARG


def _create(sid, mode, critic_struct="quad-nomix"):
    cfg = EngineConfig(sys_id=sid, batch=64, dtype="f64", Nactor=10, mode=mode, critic_struct=critic_struct, Ncritic=4,
                       buffer_size=10, pars=[1.3, 9.81, 0.7], ctrl_bnds=np.array([[-5.0, 5.0]]),
                       R1=np.eye(N.sys_dy(sid) + 1), dt_sim=0.01, sampling_time=0.01, pred_step_size=0.02).to_native()
    h = N.C.c_void_p()
    rc = N.lib().rcg_create(N.C.byref(cfg), N.C.byref(h))
    msg = N.last_error(None)
    if rc == N.OK:
        N.lib().rcg_destroy(h)
    return rc, msg


@pytest.mark.parametrize("mode", ["RQL", "SQL"])
def test_create_in_a_critic_mode_needs_the_opt_in(mode):
    plain = N.register_system("PendulumT", PENDULUM, 2, 1, 3)
    rc, msg = _create(plain["sys_id"], mode)
    assert rc == N.ERR_UNSUPPORTED and "MPC only" in msg, msg
    # with CRITIC the refusal is gone: the call gets as far as the device (none on a CPU machine)
    info = N.register_system("PendulumYC", pendulum_critic_source("PendulumYC"), 2, 1, 3)
    rc, msg = _create(info["sys_id"], mode)
    assert rc in (N.OK, N.ERR_NO_DEVICE), (rc, msg)


def test_an_oversized_dim_critic_cannot_reach_rcg_create():
    """An oversized dim_critic - beyond RCG_MAX_DC = 35, the rows of w_init / w_min / w_max - CANNOT be produced: inside the
    dimensions a registration accepts (DY <= 5, du <= 2) the largest is quad-lin over 7 = 35, and an output beyond them is stopped
    at registration, CRITIC or not (the refusal asserted below).  rcg_create's own guard on dim_critic, which names the number,
    is therefore a defensive check that no test can trigger; what is tested is the arithmetic that makes it unreachable."""
    assert max(dim_critic(cs, dy, du) for cs in STRUCTS for dy in range(1, N.MAX_DS + 1) for du in range(1, N.MAX_DU + 1)) == 35
    assert dim_critic("quad-lin", N.MAX_DS + 1, N.MAX_DU) > 35
    sid = N.C.c_int32(-1)
    src = with_critic(pendulum_out_source("PendulumYC6", dy=N.MAX_DS + 1))
    rc = N.lib().rcg_register_system(b"PendulumYC6", src.encode(), 2, 1, 3, N.C.byref(sid))
    assert rc == N.ERR_UNSUPPORTED and "DY = 6" in N.last_error(None)


def test_ctrl_opt_pred_accepts_critic_modes_only_with_the_opt_in():
    from rcognita_amd.controllers import CtrlOptPred
    from rcognita_amd.systems import System

    class PendulumPlainSys(System):
        hip_policy = PENDULUM.replace("PendulumT", "PendulumPlainSys")

    s = PendulumPlainSys(sys_type="diff_eqn", dim_state=2, dim_input=1, dim_output=2, dim_disturb=0, pars=[1.3, 9.81, 0.7],
                         ctrl_bnds=np.array([[-5.0, 5.0]]))
    assert not PendulumPlainSys._hip_info["has_critic"]
    with pytest.raises(NotImplementedError, match="CRITIC"):
        CtrlOptPred(1, 2, mode="RQL", ctrl_bnds=np.array([[-5.0, 5.0]]), Nactor=10, sys_rhs=s._state_dyn, sys_out=s.out,
                    state_sys=np.zeros(2), stage_obj_pars=[np.diag([10.0, 1.0, 0.0])], candidates=np.zeros((4, 10)))

    class PendulumCritSys(System):
        hip_policy = pendulum_critic_source("PendulumCritSys")

    PendulumCritSys(sys_type="diff_eqn", dim_state=2, dim_input=1, dim_output=3, dim_disturb=0, pars=[1.3, 9.81, 0.7])
    assert PendulumCritSys._hip_info["has_critic"] and PendulumCritSys._hip_info["dy"] == 3
