#!/usr/bin/env python3
"""Write tests/golden/F14_output_map_pendulum.npz from the reference's own results (read-only import).

A pendulum ``System`` subclass of the reference, dynamics in NumPy, with an output map ``out(x) = (sin x0, cos x0, x1)``:
dim_state 2, dim_output 3.  The reference carries ``out`` through ``CtrlOptPred._actor_cost`` (controllers.py:1286-1296) and the
stage cost over chi = [y - target, u] (controllers.py:1063-1084), so what is recorded here pins a restatement of both.

    (a) ``_actor_cost`` of random (state_sys, observation, sequence) triples for gamma in {1, 0.9} x R1 diagonal / full /
        diagonal with a target x observation = out(state_sys) or another one (the REF_LAG shape);
    (b) ``_actor_optimizer``'s SLSQP (tol=1e-7, the recipe of oracle/gen_fixtures.py's F8) from 16 states.

Runs only where the reference exists (the import recipe of oracle/gen_fixtures.py::import_reference), never on a GPU machine:

    python tools/gen_output_map_fixture.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.gen_fixtures import TargetArray, import_reference, save  # noqa: E402

PARS = (1.3, 9.81, 0.7)  # m, g, l
BND = 5.0
NACTOR = 10
H = 0.02  # pred_step_size
DT = 0.02  # sampling_time
R1_DIAG = np.diag([5.0, 5.0, 0.5, 0.1])
R1_FULL = R1_DIAG + 0.05 * np.ones((4, 4)) + 0.02 * np.eye(4, k=1)  # not symmetric: the reference takes any matrix
TARGET = np.array([0.0, 1.0, 0.0])  # upright: sin 0, cos 0, no rate
N_A = 64
N_B = 16


def pendulum_class(systems):
    class Pendulum(systems.System):
        """rcognita System subclass: _state_dyn overridden, out overridden (systems.py:17-29, 185)."""

        def _state_dyn(self, t, state, action, disturb=[]):
            m, g, l = self.pars
            return np.array([state[1], -g / l * np.sin(state[0]) + action[0] / (m * l * l)])

        def out(self, state, action=[]):
            return np.array([np.sin(state[0]), np.cos(state[0]), state[1]])

    return Pendulum


def make(controllers, systems, R1, gamma, target):
    P = pendulum_class(systems)
    sys_obj = P(sys_type="diff_eqn", dim_state=2, dim_input=1, dim_output=3, dim_disturb=0, pars=list(PARS),
                ctrl_bnds=np.array([[-BND, BND]]))
    ctrl = controllers.CtrlOptPred(
        1, 3, "MPC", ctrl_bnds=np.array([[-BND, BND]]), action_init=[], t0=0, sampling_time=DT, Nactor=NACTOR,
        pred_step_size=H, sys_rhs=sys_obj._state_dyn, sys_out=sys_obj.out, state_sys=np.zeros(2), prob_noise_pow=8,
        is_est_model=0, model_est_stage=2, model_est_period=DT, buffer_size=10, model_order=5, model_est_checks=0, gamma=gamma,
        Ncritic=4, critic_period=DT, critic_struct="quad-nomix", stage_obj_struct="quadratic", stage_obj_pars=[R1],
        observation_target=[] if target is None else TargetArray(target))
    return sys_obj, ctrl


def rand_states(rng, n):
    return np.stack([rng.uniform(-np.pi, np.pi, n), rng.uniform(-3, 3, n)], axis=-1)


def main():
    systems, _, controllers = import_reference()
    rng = np.random.default_rng(20261016)
    cases = []
    for gamma in (1.0, 0.9):
        for cost in ("diag", "full", "target"):
            for lag in (False, True):
                cases.append((gamma, cost, lag))
    C = len(cases)
    xs, obs, seq, J = np.zeros((C, N_A, 2)), np.zeros((C, N_A, 3)), np.zeros((C, N_A, NACTOR)), np.zeros((C, N_A))
    R1s, tgts = np.zeros((C, 4, 4)), np.zeros((C, 3))
    for ci, (gamma, cost, lag) in enumerate(cases):
        R1 = R1_FULL if cost == "full" else R1_DIAG
        target = TARGET if cost == "target" else None
        sys_obj, ctrl = make(controllers, systems, R1, gamma, target)
        R1s[ci] = R1
        tgts[ci] = TARGET if target is not None else 0.0
        x = rand_states(rng, N_A)
        xo = rand_states(rng, N_A) if lag else x
        u = rng.uniform(-BND, BND, (N_A, NACTOR))
        for i in range(N_A):
            ctrl.state_sys = x[i]
            y = sys_obj.out(xo[i])
            xs[ci, i], obs[ci, i], seq[ci, i] = x[i], y, u[i]
            J[ci, i] = ctrl._actor_cost(u[i], y)  # controllers.py:1273-1328

    from scipy.optimize import Bounds, minimize

    sys_obj, ctrl = make(controllers, systems, R1_DIAG, 1.0, None)
    xb = rand_states(rng, N_B)
    Jopt, uopt, nfev, Jinit = np.zeros(N_B), np.zeros((N_B, NACTOR)), np.zeros(N_B, dtype=np.int64), np.zeros(N_B)
    for i in range(N_B):
        ctrl.state_sys = xb[i]
        y = sys_obj.out(xb[i])
        init = np.reshape(ctrl.action_sqn_init, [NACTOR])
        res = minimize(lambda a: ctrl._actor_cost(a, y), init, method="SLSQP", tol=1e-7,
                       bounds=Bounds(ctrl.action_sqn_min, ctrl.action_sqn_max, keep_feasible=True),
                       options={"maxiter": 300, "disp": False})  # controllers.py:1373-1398
        Jopt[i], uopt[i], nfev[i] = res.fun, res.x, res.nfev
        Jinit[i] = ctrl._actor_cost(init, y)
    meta = dict(system="pendulum with out = (sin th, cos th, om)", pars=list(PARS), bnds=[-BND, BND], Nactor=NACTOR,
                pred_step_size=H, sampling_time=DT, cases=[dict(gamma=g, cost=c, lag=l) for g, c, l in cases],
                action_init=list(np.reshape(ctrl.action_sqn_init, [NACTOR])[:1]), b_R1="diag", b_gamma=1.0)
    save("F14_output_map_pendulum", meta, a_state_sys=xs, a_obs=obs, a_seq=seq, a_J=J, a_R1=R1s, a_target=tgts,
         b_state=xb, b_J_opt=Jopt, b_seq_opt=uopt, b_nfev=nfev, b_J_init=Jinit, b_R1=R1_DIAG)


if __name__ == "__main__":
    main()
