#!/usr/bin/env python3
"""Write tests/golden/F17_user_system_corners.npz from the reference's own results (read-only import).

The four corner systems of tests/user_systems.py (C1 .. C4: the extremes of DS, DU, NP, DY, DD that rcg_register_system accepts) as
``System`` subclasses of the reference with ``_state_dyn``, ``out`` and ``_disturb_dyn`` overridden.  The class bodies below are
written out in scalar Python from the formulas in that module's docstring (its coefficient functions are imported, its array
code is not used), so that the twin there is pinned on a second statement of the same system.  Recorded per system:

    (r) ``closed_loop_rhs(0, [state, disturb])`` on 64 points with actions partly beyond the bounds, the noise replayed (F16);
    (o) ``out`` on the same 64 states;
    (a) ``_actor_cost`` on 16 points each: MPC gamma = 1 and 0.9 with a diagonal R1, MPC with a full non-symmetric R1 and a
        target (and ``stage_obj`` there), RQL x 4 and SQL x 4 critic structures (observation != out(state_sys));
    (c) ``_critic`` and (d) ``_critic_cost`` x 4 structures, with a target, 16 points each;
    (s) ``_actor_optimizer``'s SLSQP (the recipe of F14 (b)) in MPC from 8 states, Nactor = 5.

Runs only where the reference exists (the import recipe of oracle/gen_fixtures.py::import_reference), never on a GPU machine:

    python tools/gen_user_system_corners_fixture.py
"""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.gen_disturb_fixtures import OldEqArray  # noqa: E402
from oracle.gen_fixtures import TargetArray, import_reference, save  # noqa: E402
from tests.user_systems import CORNERS, STRUCTS, _a, _b, _E, _F, _g, _Y, corner  # noqa: E402

NACTOR, H, DT = 5, 0.1, 0.05
GAMMA_C = 0.95
NCRITIC, BUFFER = 4, 6
N_R, N_A, N_S = 64, 16, 8


def r1_diag(dy, du):
    return np.diag(([4.0, 3.0, 2.5, 2.0, 1.5][:dy]) + ([2.0, 2.5][:du]))


def r1_full(dy, du):
    n = dy + du
    i = np.arange(n)
    return r1_diag(dy, du) + 0.05 * np.ones((n, n)) + 0.02 * np.eye(n, k=1) + 0.004 * np.outer(i + 1, (i[::-1] + 1) ** 2) / n


def rd(a):
    """Inputs on the grid of 2^-10: exact in float32 as well, and the file stays small."""
    return np.round(np.asarray(a, dtype=float) * 1024.0) / 1024.0


def target(dy):
    return np.array([0.3 * (-1) ** m + 0.1 * m for m in range(dy)])


def system_class(systems, ds, du, np_, dy, dd):
    P = lambda r, i: 1.0 if np_ == 0 else r[i % np_]  # noqa: E731
    Q = lambda r, j: 1.0 if np_ == 0 else r[(ds + j) % np_]  # noqa: E731

    class Corner(systems.System):
        """rcognita System subclass: _state_dyn, out and _disturb_dyn overridden (systems.py:147-185)."""

        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            if self.is_disturb:
                self.sigma_disturb, self.mu_disturb, self.tau_disturb = self.pars_disturb  # systems.py:303-306

        def _state_dyn(self, t, state, action, disturb=[]):
            r = [p / (1.0 + p * p) for p in self.pars]
            d = np.zeros(ds)
            for i in range(ds):
                d[i] = -_a(i) * P(r, i) * math.sin(state[i]) + _b(i) * state[(i + 1) % ds] * math.cos(state[i])
                for j in range(du):
                    d[i] += _g(i, j) * Q(r, j) * action[j]
            if self.is_disturb and (disturb != []):  # systems.py:317
                d[ds - 1] += math.cos(state[0]) * disturb[0]
                if dd == 2:
                    d[0] += (1.0 + 0.5 * action[0]) * disturb[1]
            return d

        def _disturb_dyn(self, t, disturb):
            Dd = np.zeros(self.dim_disturb)
            for k in range(self.dim_disturb):  # systems.py:342-343
                Dd[k] = -self.tau_disturb[k] * (disturb[k] + self.sigma_disturb[k] * (systems.randn() + self.mu_disturb[k]))
            return Dd

        def out(self, state, action=[]):
            if dy is None:
                return state
            y = np.zeros(dy)
            for m in range(dy):
                y[m] = _Y * math.sin(state[m % ds] + 0.3 * m) + _F(m) * state[(m + 1) % ds] * state[(m + 3) % ds]
                for i in range(ds):
                    y[m] += _E(m, i) * state[i]
            return y

    return Corner


def make_ctrl(controllers, sys_obj, S, mode, R1, gamma, tgt, cs="quad-nomix"):
    return controllers.CtrlOptPred(
        S.du, S.dy, mode, ctrl_bnds=S.bnds, action_init=[], t0=0, sampling_time=DT, Nactor=NACTOR, pred_step_size=H,
        sys_rhs=sys_obj._state_dyn, sys_out=sys_obj.out, state_sys=np.zeros(S.ds), prob_noise_pow=8, is_est_model=0,
        model_est_stage=2, model_est_period=DT, buffer_size=BUFFER, model_order=5, model_est_checks=0, gamma=gamma,
        Ncritic=NCRITIC, critic_period=DT, critic_struct=cs, stage_obj_struct="quadratic", stage_obj_pars=[R1],
        observation_target=[] if tgt is None else TargetArray(tgt))


def main():
    systems, _, controllers = import_reference()
    from scipy.optimize import Bounds, minimize

    rng = np.random.default_rng(20261020)
    arrays, meta_sys = {}, {}
    for key, (name, ds, du, np_, dy, dd) in CORNERS.items():
        S = corner(key)
        cls = system_class(systems, ds, du, np_, dy, dd)
        p = key + "_"
        # (r), (o)
        sigma, mu, tau = rng.uniform(0.5, 3.0, dd), rng.uniform(-1.0, 1.0, dd), rng.uniform(0.2, 2.0, dd)
        sd = cls(sys_type="diff_eqn", dim_state=ds, dim_input=du, dim_output=S.dy, dim_disturb=dd, pars=list(S.pars),
                 ctrl_bnds=S.bnds, is_dyn_ctrl=0, is_disturb=1, pars_disturb=[sigma, mu, tau])
        assert sd._dim_full_state == ds + dd
        x, q = rd(S.rand_states(rng, N_R)), rd(rng.normal(0.0, 2.0, (N_R, dd)))
        u, xi = rd(S.rand_actions(rng, (N_R,), overshoot=1.5)), rd(rng.standard_normal((N_R, dd)))
        rhs, clipped, y = np.zeros((N_R, ds + dd)), np.zeros((N_R, du)), np.zeros((N_R, S.dy))
        for i in range(N_R):
            seq = iter(xi[i])
            systems.randn = lambda: next(seq)  # replayed noise, in the order the reference draws it (k = 0, 1, ...)
            sd.receive_action(u[i].copy())
            rhs[i] = sd.closed_loop_rhs(0.0, OldEqArray(np.concatenate([x[i], q[i]])))
            clipped[i] = sd.action
            y[i] = sd.out(x[i])
        assert np.any(clipped != u)
        arrays.update({p + "r_state": x, p + "r_disturb": q, p + "r_action": u, p + "r_xi": xi, p + "r_sigma": sigma, p + "r_mu": mu,
                       p + "r_tau": tau, p + "r_rhs_full": rhs, p + "r_action_clipped": clipped, p + "o_out": y})
        # (a)
        so = cls(sys_type="diff_eqn", dim_state=ds, dim_input=du, dim_output=S.dy, dim_disturb=0, pars=list(S.pars), ctrl_bnds=S.bnds)
        Rd, Rf, tg = r1_diag(S.dy, du), r1_full(S.dy, du), target(S.dy)
        cases = [("mpc_g1", "MPC", Rd, 1.0, None, None), ("mpc_g09", "MPC", Rd, 0.9, None, None), ("mpc_full_tgt", "MPC", Rf, 0.9, tg, None)]
        cases += [(f"{m}_{cs.replace('-', '_')}", m, Rd, GAMMA_C, None, cs) for m in ("RQL", "SQL") for cs in STRUCTS]
        dims = {}
        for tag, mode, R1, gamma, tgt, cs in cases:
            ctrl = make_ctrl(controllers, so, S, mode, R1, gamma, tgt, cs or "quad-nomix")
            xs, xo = rd(S.rand_states(rng, N_A)), S.rand_states(rng, N_A)
            yo = rd([so.out(v) for v in xo])
            sq = rd(S.rand_actions(rng, (N_A, NACTOR)))
            w = rd(rng.uniform(np.maximum(ctrl.Wmin, -2.0), np.minimum(ctrl.Wmax, 2.0), (N_A, ctrl.dim_critic)))
            J = np.zeros(N_A)
            for i in range(N_A):
                ctrl.state_sys, ctrl.w_critic = xs[i], w[i]
                J[i] = ctrl._actor_cost(sq[i].reshape(-1), yo[i])
            a = p + "a_" + tag
            arrays.update({a + "_state_sys": xs, a + "_obs": yo, a + "_seq": sq, a + "_J": J})
            if tag == "mpc_full_tgt":  # ... and stage_obj of (observation, first action) under the full R1 and the target
                arrays[a + "_stage"] = np.array([ctrl.stage_obj(yo[i], sq[i, 0]) for i in range(N_A)])
            if cs:
                arrays[a + "_w"] = w
                dims[cs] = int(ctrl.dim_critic)
        # (c), (d): with a target
        for cs in STRUCTS:
            ctrl = make_ctrl(controllers, so, S, "RQL", Rd, GAMMA_C, tg, cs)
            k = cs.replace("-", "_")
            yc = rd(np.array([so.out(v) for v in S.rand_states(rng, N_A)]) + rng.normal(0, 0.1, (N_A, S.dy)))
            uc = rd(S.rand_actions(rng, (N_A,)))
            wc = rd(rng.uniform(np.maximum(ctrl.Wmin, -2.0), np.minimum(ctrl.Wmax, 2.0), (N_A, ctrl.dim_critic)))
            arrays.update({f"{p}c_{k}_obs": yc, f"{p}c_{k}_act": uc, f"{p}c_{k}_w": wc,
                           f"{p}c_{k}_Q": np.array([ctrl._critic(yc[i], uc[i], wc[i]) for i in range(N_A)])})
            ob = rd([[so.out(v) for v in S.rand_states(rng, BUFFER)] for _ in range(N_A)])
            ab = rd(S.rand_actions(rng, (N_A, BUFFER)))
            w, wp = (rd(rng.uniform(np.maximum(ctrl.Wmin, -2.0), np.minimum(ctrl.Wmax, 2.0), (N_A, ctrl.dim_critic))) for _ in range(2))
            Jc = np.zeros(N_A)
            for i in range(N_A):
                ctrl.observation_buffer, ctrl.action_buffer, ctrl.w_critic_prev = ob[i], ab[i], wp[i]
                Jc[i] = ctrl._critic_cost(w[i])
            arrays.update({f"{p}d_{k}_obs_buf": ob, f"{p}d_{k}_act_buf": ab, f"{p}d_{k}_w": w, f"{p}d_{k}_w_prev": wp, f"{p}d_{k}_Jc": Jc})
        # (s)
        ctrl = make_ctrl(controllers, so, S, "MPC", Rd, 1.0, None)
        xb = rd(S.rand_states(rng, N_S))
        Jopt, uopt, Jinit = np.zeros(N_S), np.zeros((N_S, NACTOR, du)), np.zeros(N_S)
        init = np.reshape(ctrl.action_sqn_init, [NACTOR * du])
        for i in range(N_S):
            ctrl.state_sys = xb[i]
            yb = so.out(xb[i])
            res = minimize(lambda a: ctrl._actor_cost(a, yb), init, method="SLSQP", tol=1e-7,
                           bounds=Bounds(ctrl.action_sqn_min, ctrl.action_sqn_max, keep_feasible=True),
                           options={"maxiter": 300, "disp": False})  # controllers.py:1373-1398
            Jopt[i], uopt[i], Jinit[i] = res.fun, res.x.reshape(NACTOR, du), ctrl._actor_cost(init, yb)
        arrays.update({p + "s_state": xb, p + "s_J_opt": Jopt, p + "s_seq_opt": uopt, p + "s_J_init": Jinit,
                       p + "R1_diag": Rd, p + "R1_full": Rf, p + "target": tg})
        meta_sys[key] = dict(name=name, ds=ds, du=du, np=np_, dy=S.dy, has_out=dy is not None, dd=dd, pars=list(S.pars),
                             bnds=S.bnds.tolist(), dim_critic=dims, action_init=list(init[:du]))
    meta = dict(systems=meta_sys, Nactor=NACTOR, pred_step_size=H, sampling_time=DT, gamma_critic=GAMMA_C, Ncritic=NCRITIC,
                buffer_size=BUFFER, structs=list(STRUCTS),
                note="arrays per system under C1_ .. C4_; r: closed_loop_rhs on [state, disturb] with randn() replaced by xi; "
                     "a: _actor_cost (mpc_g1, mpc_g09: R1_diag; mpc_full_tgt: R1_full, gamma 0.9, target; RQL / SQL: R1_diag, "
                     "gamma_critic, no target); c, d: _critic, _critic_cost with R1_diag and target; s: SLSQP, MPC, R1_diag, gamma 1")
    save("F17_user_system_corners", meta, **arrays)


if __name__ == "__main__":
    main()
