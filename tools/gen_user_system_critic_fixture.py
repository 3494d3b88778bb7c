#!/usr/bin/env python3
"""Write tests/golden/F15_user_system_critic.npz from the reference's own results (read-only import).

The pendulum of F14 (tools/gen_output_map_fixture.py): a ``System`` subclass of the reference with the output map
``out(x) = (sin x0, cos x0, x1)``, dim_state 2, dim_output 3.  The reference's critic is a linear model over the regressor of
chi = [y - target, u] (quad-mix: of the raw y), so its dimension is a function of dim_output + dim_input
(controllers.py:1024-1039, 1192-1214).  Recorded, for each of the four critic structures:

    (c) ``_critic`` of random (observation, action, w) triples, with a target;
    (d) ``_critic_cost`` of random (w, w_prev) on random buffers (Ncritic = 4, buffer_size = 10);
    (e) ``_actor_cost`` in RQL and SQL of random (state_sys, observation != out(state_sys), sequence, w), with a target;
    (f) ``_critic_optimizer``'s SLSQP on 16 TD stacks: its w and Jc = _critic_cost(w) (Ncritic = 4: three TD rows);
    (g) ``_actor_optimizer``'s SLSQP in RQL from 8 states (the recipe of F14's (b)): the cost it reaches.

Results only.  Runs only where the reference exists (the import recipe of oracle/gen_fixtures.py::import_reference), never on a
GPU machine:

    python tools/gen_user_system_critic_fixture.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.gen_fixtures import TargetArray, import_reference, save  # noqa: E402
from tools.gen_output_map_fixture import BND, DT, H, NACTOR, PARS, R1_DIAG, TARGET, pendulum_class, rand_states  # noqa: E402

STRUCTS = ("quad-lin", "quadratic", "quad-nomix", "quad-mix")
GAMMA = 0.95
NCRITIC, BUFFER = 4, 10
N_C, N_D, N_E, N_F, N_G = 32, 16, 16, 16, 8


def make(controllers, systems, mode, critic_struct, target=TARGET, gamma=GAMMA):
    P = pendulum_class(systems)
    sys_obj = P(sys_type="diff_eqn", dim_state=2, dim_input=1, dim_output=3, dim_disturb=0, pars=list(PARS),
                ctrl_bnds=np.array([[-BND, BND]]))
    ctrl = controllers.CtrlOptPred(
        1, 3, mode, ctrl_bnds=np.array([[-BND, BND]]), action_init=[], t0=0, sampling_time=DT, Nactor=NACTOR,
        pred_step_size=H, sys_rhs=sys_obj._state_dyn, sys_out=sys_obj.out, state_sys=np.zeros(2), prob_noise_pow=8,
        is_est_model=0, model_est_stage=2, model_est_period=DT, buffer_size=BUFFER, model_order=5, model_est_checks=0,
        gamma=gamma, Ncritic=NCRITIC, critic_period=DT, critic_struct=critic_struct, stage_obj_struct="quadratic",
        stage_obj_pars=[R1_DIAG], observation_target=[] if target is None else TargetArray(target))
    return sys_obj, ctrl


def rand_w(rng, ctrl, n):
    return rng.uniform(np.maximum(ctrl.Wmin, -2.0), np.minimum(ctrl.Wmax, 2.0), (n, ctrl.dim_critic))


def rand_buffers(rng, sys_obj, n):
    """n pairs of buffers as a closed loop leaves them: observations of states, bounded actions."""
    x = np.stack([rand_states(rng, BUFFER) for _ in range(n)])
    ob = np.stack([[sys_obj.out(x[i, k]) for k in range(BUFFER)] for i in range(n)])
    return ob, rng.uniform(-BND, BND, (n, BUFFER, 1))


def main():
    systems, _, controllers = import_reference()
    from scipy.optimize import Bounds, minimize

    rng = np.random.default_rng(20261017)
    arrays, dims = {}, {}
    for cs in STRUCTS:
        key = cs.replace("-", "_")
        sys_obj, ctrl = make(controllers, systems, "RQL", cs)
        dc = ctrl.dim_critic
        dims[cs] = int(dc)
        # (c)
        y = np.array([sys_obj.out(x) for x in rand_states(rng, N_C)]) + rng.normal(0, 0.1, (N_C, 3))
        u, w = rng.uniform(-BND, BND, (N_C, 1)), rand_w(rng, ctrl, N_C)
        arrays.update({f"c_{key}_obs": y, f"c_{key}_act": u, f"c_{key}_w": w,
                       f"c_{key}_Q": np.array([ctrl._critic(y[i], u[i], w[i]) for i in range(N_C)])})
        # (d)
        ob, ab = rand_buffers(rng, sys_obj, N_D)
        w, wp = rand_w(rng, ctrl, N_D), rand_w(rng, ctrl, N_D)
        Jc = np.zeros(N_D)
        for i in range(N_D):
            ctrl.observation_buffer, ctrl.action_buffer, ctrl.w_critic_prev = ob[i], ab[i], wp[i]
            Jc[i] = ctrl._critic_cost(w[i])
        arrays.update({f"d_{key}_obs_buf": ob, f"d_{key}_act_buf": ab, f"d_{key}_w": w, f"d_{key}_w_prev": wp, f"d_{key}_Jc": Jc})
        # (e)
        for mode in ("RQL", "SQL"):
            _, c2 = make(controllers, systems, mode, cs)
            xs, xo = rand_states(rng, N_E), rand_states(rng, N_E)
            yo = np.array([sys_obj.out(x) for x in xo])
            seq, w = rng.uniform(-BND, BND, (N_E, NACTOR)), rand_w(rng, c2, N_E)
            J = np.zeros(N_E)
            for i in range(N_E):
                c2.state_sys, c2.w_critic = xs[i], w[i]
                J[i] = c2._actor_cost(seq[i], yo[i])
            arrays.update({f"e_{mode}_{key}_state_sys": xs, f"e_{mode}_{key}_obs": yo, f"e_{mode}_{key}_seq": seq,
                           f"e_{mode}_{key}_w": w, f"e_{mode}_{key}_J": J})
        # (f)
        ob, ab = rand_buffers(rng, sys_obj, N_F)
        wp = rand_w(rng, ctrl, N_F)
        wfit, Jc, Jc0 = np.zeros((N_F, dc)), np.zeros(N_F), np.zeros(N_F)
        for i in range(N_F):
            ctrl.observation_buffer, ctrl.action_buffer, ctrl.w_critic_prev = ob[i], ab[i], wp[i]
            wfit[i] = ctrl._critic_optimizer()  # controllers.py:1248-1271
            Jc[i], Jc0[i] = ctrl._critic_cost(wfit[i]), ctrl._critic_cost(ctrl.w_critic_init)
        arrays.update({f"f_{key}_obs_buf": ob, f"f_{key}_act_buf": ab, f"f_{key}_w_prev": wp, f"f_{key}_w": wfit, f"f_{key}_Jc": Jc,
                       f"f_{key}_Jc_init": Jc0})
        # (g)
        xb, w = rand_states(rng, N_G), np.abs(rand_w(rng, ctrl, N_G))
        Jopt, uopt, Jinit = np.zeros(N_G), np.zeros((N_G, NACTOR)), np.zeros(N_G)
        for i in range(N_G):
            ctrl.state_sys, ctrl.w_critic = xb[i], w[i]
            yb = sys_obj.out(xb[i])
            init = np.reshape(ctrl.action_sqn_init, [NACTOR])
            res = minimize(lambda a: ctrl._actor_cost(a, yb), init, method="SLSQP", tol=1e-7,
                           bounds=Bounds(ctrl.action_sqn_min, ctrl.action_sqn_max, keep_feasible=True),
                           options={"maxiter": 300, "disp": False})  # controllers.py:1373-1398
            Jopt[i], uopt[i], Jinit[i] = res.fun, res.x, ctrl._actor_cost(init, yb)
        arrays.update({f"g_{key}_state": xb, f"g_{key}_w": w, f"g_{key}_J_opt": Jopt, f"g_{key}_seq_opt": uopt,
                       f"g_{key}_J_init": Jinit})
    meta = dict(system="pendulum with out = (sin th, cos th, om)", pars=list(PARS), bnds=[-BND, BND], Nactor=NACTOR,
                pred_step_size=H, sampling_time=DT, gamma=GAMMA, Ncritic=NCRITIC, buffer_size=BUFFER, structs=list(STRUCTS),
                dim_critic=dims, target=list(TARGET), R1=list(np.diag(R1_DIAG)),
                action_init=list(np.reshape(ctrl.action_sqn_init, [NACTOR])[:1]))
    save("F15_user_system_critic", meta, **arrays)


if __name__ == "__main__":
    main()
