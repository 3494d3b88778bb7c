#!/usr/bin/env python3
"""Write tests/golden/F16_disturb_pendulum.npz from the reference's own results (read-only import).

A pendulum ``System`` subclass of the reference with ``is_disturb=1``: the reference's extension point is "subclass ``System``,
override ``_state_dyn``" (systems.py:17-29), and with a disturbance ``_state_dyn(t, state, action, disturb)`` decides how it
enters (systems.py:308-323).  Here the disturbance is a torque scaled by the state, so that a kernel which did not hand the state
to the policy's ``disturb`` member could not reproduce it:

    DD = 1   d omega/dt += cos(theta) / (m l^2) * q_0
    DD = 2   ... and d theta/dt += q_1

``_disturb_dyn`` is the first-order filter the reference's own systems use (systems.py:325-345), written out for this class.
Recorded: ``closed_loop_rhs(0, [state, disturb])`` (systems.py:213-253) on 256 seeded random points for each DD, with the noise
``xi``, ``sigma`` / ``mu`` / ``tau`` and the clipped action.

The two workarounds of oracle/gen_disturb_fixtures.py apply here too.  ``OldEqArray`` is imported from there.  The noise replay
is the same monkeypatch - the module attribute ``rcognita.systems.randn`` replaced by a function that replays ``xi`` - and has
no function of its own in that script to import: the class below draws through ``systems.randn()`` exactly as the reference's
``_disturb_dyn`` does, so the replacement reaches it.

Runs only where the reference exists (the import recipe of oracle/gen_fixtures.py::import_reference), never on a GPU machine:

    python tools/gen_user_system_disturb_fixture.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.gen_disturb_fixtures import OldEqArray  # noqa: E402
from oracle.gen_fixtures import import_reference, save  # noqa: E402

PARS = (1.3, 9.81, 0.7)  # m, g, l
BND = 5.0
N = 256


def pendulum_class(systems, dd):
    class PendulumDisturbed(systems.System):
        """rcognita System subclass: _state_dyn and _disturb_dyn overridden (systems.py:147-183)."""

        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.sigma_disturb, self.mu_disturb, self.tau_disturb = self.pars_disturb  # systems.py:303-306

        def _state_dyn(self, t, state, action, disturb=[]):
            m, g, l = self.pars
            d = np.array([state[1], -g / l * np.sin(state[0]) + action[0] / (m * l * l)])
            if self.is_disturb and (disturb != []):  # systems.py:317
                d[1] += np.cos(state[0]) / (m * l * l) * disturb[0]
                if dd == 2:
                    d[0] += disturb[1]
            return d

        def _disturb_dyn(self, t, disturb):
            Ddisturb = np.zeros(self.dim_disturb)
            for k in range(0, self.dim_disturb):  # systems.py:342-343
                Ddisturb[k] = -self.tau_disturb[k] * (disturb[k] + self.sigma_disturb[k] * (systems.randn() + self.mu_disturb[k]))
            return Ddisturb

    return PendulumDisturbed


def main():
    systems, _, _ = import_reference()
    rng = np.random.default_rng(20261019)
    arrays = {}
    for dd in (1, 2):
        sigma, mu, tau = rng.uniform(0.5, 3.0, dd), rng.uniform(-1.0, 1.0, dd), rng.uniform(0.2, 2.0, dd)
        sys_obj = pendulum_class(systems, dd)(
            sys_type="diff_eqn", dim_state=2, dim_input=1, dim_output=2, dim_disturb=dd, pars=list(PARS),
            ctrl_bnds=np.array([[-BND, BND]]), is_dyn_ctrl=0, is_disturb=1, pars_disturb=[sigma, mu, tau])
        assert sys_obj._dim_full_state == 2 + dd
        x = np.stack([rng.uniform(-np.pi, np.pi, N), rng.uniform(-3, 3, N)], axis=-1)
        q = rng.normal(0.0, 5.0, (N, dd))
        u = rng.uniform(-1.5 * BND, 1.5 * BND, (N, 1))  # a third of them beyond the bounds
        xi = rng.standard_normal((N, dd))
        rhs, clipped = np.zeros((N, 2 + dd)), np.zeros((N, 1))
        for i in range(N):
            seq = iter(xi[i])
            systems.randn = lambda: next(seq)  # replayed noise, in the order the reference draws it (k = 0, 1, ...)
            sys_obj.receive_action(u[i].copy())
            rhs[i] = sys_obj.closed_loop_rhs(0.0, OldEqArray(np.concatenate([x[i], q[i]])))
            clipped[i] = sys_obj.action
        assert np.any(np.abs(u) > BND) and np.all(np.abs(clipped) <= BND)
        p = f"dd{dd}_"
        arrays.update({p + "state": x, p + "disturb": q, p + "action": u, p + "xi": xi, p + "sigma": sigma, p + "mu": mu,
                       p + "tau": tau, p + "rhs_full": rhs, p + "action_clipped": clipped})
    meta = dict(system="pendulum, disturbance = torque scaled by cos(theta) (DD = 2: and a rate on theta)", pars=list(PARS),
                bnds=[-BND, BND], n=N,
                note="rhs_full = closed_loop_rhs(0, [state, disturb]) with randn() replaced by xi; arrays per DD under dd1_ / dd2_")
    save("F16_disturb_pendulum", meta, **arrays)


if __name__ == "__main__":
    main()
