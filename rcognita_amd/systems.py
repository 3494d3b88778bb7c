"""Environment classes with the reference's interface (rcognita/systems.py), backed by librcg.

Same class names, constructor signature and method names as the reference, so a preset written for
``rcognita.systems`` runs against ``rcognita_amd.systems`` unchanged.  Differences:

* every method also accepts a leading batch axis (``state [B, ds]``, ``action [B, du]``);
* the arithmetic runs in the HIP kernels (``rcg_rhs``); there is no NumPy implementation here and no
  fallback - without the library or a GPU the calls raise;
* ``is_disturb=1`` (full state ``[state, disturb]``, rcognita/systems.py:140-145, 325-345) is on the native path
  (``rcg_rhs_full``, ``RCG_FLAG_DISTURB``).  The reference draws ``randn()`` from the unseeded global RNG inside every
  right-hand side; here the noise comes from the counter-based generator of rcg_disturb.hpp (key ``seed``): a
  ``System`` object called directly draws one vector per call, a ``Simulator`` one per RK4 substep and env;
* ``is_dyn_ctrl`` is rejected: no preset sets it and the reference's dynamic-controller branch is itself broken
  (SURVEY.md 8a row 1);
* your own system: instead of overriding ``_state_dyn`` in Python, a subclass sets ``hip_policy`` to the source of a policy
  struct in the shape of the built-ins (rcognita_amd/csrc/rcg_systems.hpp).  The class is compiled for the GPU on its first
  construction (``_native.register_system``) and runs the MPC path (RQL / SQL with ``CRITIC``, the device candidate search
  with ``SEARCH``, T ticks per launch with ``TICKS`` in the policy - ``_hip_info["has_ticks"]`` -, ``is_disturb=1`` with the
  members ``DD`` and ``disturb`` - ``_hip_info["dd"]``); INTEGRATION.md, "Your own system".
"""
from __future__ import annotations

import re

import numpy as np

from . import _native as N
from .engine import Engine, EngineConfig


class System:
    """Interface class of dynamical systems a.k.a. environments (rcognita/systems.py:17-253)."""

    _sys_id = None  # set by the concrete systems (a ``hip_policy`` class: by its registration)
    hip_policy = None  # source of a policy struct (``struct Name { ... };``): a system compiled at run time
    _hip_info = None  # the registration of a ``hip_policy`` class (``_native.register_system``)
    _ctrl_ref = None  # weak reference to the CtrlOptPred built around this system (_register_controller)
    name = "system"

    def __init__(self, sys_type, dim_state, dim_input, dim_output, dim_disturb, pars=[], ctrl_bnds=[], is_dyn_ctrl=0,
                 is_disturb=0, pars_disturb=[], dtype="f64", device=0, seed=0):
        if type(self).hip_policy is not None:
            if type(self).out is not System.out:
                raise NotImplementedError("a system compiled from hip_policy cannot override `out` in Python (there is no CPU "
                                          "path): give the policy an `out` member (and DY, out_jac_T; INTEGRATION.md)")
            self._register_hip_policy(dim_state, dim_input, pars)
            if is_disturb and not type(self)._hip_info["dd"]:
                raise NotImplementedError("a system compiled from hip_policy has no disturbance model (is_disturb=1) unless the "
                                          "policy has the `disturb` member (and DD; INTEGRATION.md)")
        if self._sys_id is None:
            raise NotImplementedError(
                "only the built-in systems (Sys3WRobot, Sys3WRobotNI, Sys2Tank) run on the native path; "
                "rcognita_amd has no Python fallback for user-defined dynamics")
        if sys_type != "diff_eqn":
            raise NotImplementedError("only sys_type='diff_eqn' is on the native path (SURVEY.md 8a row 2)")
        if is_dyn_ctrl:
            raise NotImplementedError("is_dyn_ctrl is out of scope (SURVEY.md 8a row 1)")
        ds, du, npar = N.SYS_DIMS[self._sys_id]
        dy = N.sys_dy(self._sys_id)  # a hip_policy's DY (its output map), else the state's dimension
        if is_disturb and dim_disturb != N.DIM_DISTURB[self._sys_id]:
            raise ValueError(f"{type(self).__name__} has dim_disturb = {N.DIM_DISTURB[self._sys_id]}")
        if (dim_state, dim_input, dim_output) != (ds, du, dy):
            raise ValueError(f"{type(self).__name__} has dims (state, input, output) = ({ds}, {du}, {dy})")
        self.sys_type = sys_type
        self.dim_state, self.dim_input, self.dim_output, self.dim_disturb = dim_state, dim_input, dim_output, dim_disturb
        self.pars = pars
        self.ctrl_bnds = np.zeros((du, 2)) if len(ctrl_bnds) == 0 else np.asarray(ctrl_bnds, dtype=float)
        self.is_dyn_ctrl, self.is_disturb, self.pars_disturb = is_dyn_ctrl, is_disturb, pars_disturb
        self._state = np.zeros(dim_state)
        self.action = np.zeros(dim_input)
        self._dim_full_state = dim_state + (dim_disturb if is_disturb else 0)  # systems.py:136-145
        if is_disturb and self._sys_id != N.SYS_2TANK:  # systems.py:303-306, 365-368 (a hip_policy with `disturb`: the same filter)
            self.sigma_disturb, self.mu_disturb, self.tau_disturb = pars_disturb[0], pars_disturb[1], pars_disturb[2]
        self.dtype, self.device, self.seed = dtype, device, int(seed)
        self._ops = None  # lazily created operator engine (batch 1: rcg_rhs takes any number of points)
        self._noise_calls = 0  # draws made by direct calls of _disturb_dyn / closed_loop_rhs on this object

    # ---- native plumbing ---------------------------------------------------------------------
    @classmethod
    def _register_hip_policy(cls, dim_state, dim_input, pars):
        """Compile the class's ``hip_policy`` once (the registry returns the same id for the same source).  The struct is the
        first ``struct <Name> {`` outside comments; its dimensions are its own ``DS`` / ``DU`` / ``NP`` where they are written
        as integer literals (``static constexpr int DS = 2, DU = 1, NP = 3;``), else the constructor's - which the compiler
        then checks against the struct (a mismatch is a ValueError, like the built-ins' dimension check)."""
        if cls.__dict__.get("_hip_info") is not None:
            return
        src = cls.hip_policy
        code = re.sub(r"//[^\n]*|/\*.*?\*/", " ", src, flags=re.S)  # the regexes below read code, not comments
        m = re.search(r"\bstruct\s+([A-Za-z_]\w*)\s*\{", code)
        if m is None:
            raise ValueError("hip_policy must define `struct <Name> { ... };`")
        body = code[m.end():]
        dims = []
        for key, given in (("DS", dim_state), ("DU", dim_input), ("NP", len(pars))):
            d = re.search(r"\b%s\s*=\s*(\d+)\s*[,;]" % key, body)
            dims.append(int(d.group(1)) if d else int(given))
        try:
            info = N.register_system(m.group(1), src, *dims)
        except N.NativeError as e:
            if e.code == N.ERR_BAD_ARG and "differs from the declared" in str(e):
                raise ValueError(f"{cls.__name__}: the dimensions (state, input, pars) = {tuple(dims)} do not match the struct "
                                 f"{m.group(1)}: {e}") from None
            if e.code == N.ERR_BAD_ARG and "but no nominal member" in str(e):  # NOMINAL_NP / nominal_lf without the law itself
                raise ValueError(f"{cls.__name__}: the nominal control law of {m.group(1)} is incomplete: {e}") from None
            raise
        cls._hip_info = info
        cls._sys_id = info["sys_id"]

    def _disturb_cfg(self):
        if not self.is_disturb:
            return {}
        pd = self.pars_disturb if len(self.pars_disturb) == 3 else [np.zeros(self.dim_disturb)] * 3
        return dict(is_disturb=True, pars_disturb=[np.asarray(v, dtype=float) for v in pd], seed=self.seed)

    def _engine(self) -> Engine:
        if self._ops is None:
            self._ops = Engine(EngineConfig(sys_id=self._sys_id, batch=1, dtype=self.dtype, device=self.device,
                                            pars=list(self.pars), ctrl_bnds=self.ctrl_bnds, **self._disturb_cfg()))
        return self._ops

    # ---- the fused loop step (rcg_loop_step): the System is what a Simulator and a CtrlOptPred have in common - the simulator is
    # built around `my_sys.closed_loop_rhs`, the controller around `my_sys._state_dyn` (presets/main_3wrobot.py:218-320) - so it is
    # where the two find each other
    def _register_controller(self, ctrl):
        import weakref

        self._ctrl_ref = weakref.ref(ctrl)

    def _fused_controller(self, sim):
        ref = getattr(self, "_ctrl_ref", None)
        ctrl = ref() if ref is not None else None
        return ctrl if (ctrl is not None and ctrl._can_fuse(sim)) else None

    def native_spec(self):
        """What a Simulator / CtrlOptPred needs to build its own handle for this system."""
        return dict(sys_id=self._sys_id, pars=list(self.pars), ctrl_bnds=self.ctrl_bnds, disturb=self._disturb_cfg())

    def _draw(self):
        """One noise vector ``[dim_disturb]`` for a direct call (the reference: ``randn()`` per component and call,
        systems.py:343): draw number ``_noise_calls`` of env 0, episode 0 of this object's generator."""
        eng = self._engine()
        eng.set_field(N.FIELD_SUBSTEP_IDX, np.array([self._noise_calls], dtype=np.int32))
        self._noise_calls += 1
        return eng.disturb_noise()[1][0, : self.dim_disturb].astype(float)

    def _call_rhs_full(self, state, disturb, action, xi, clip):
        state, disturb, action = (np.asarray(v, dtype=float) for v in (state, disturb, action))
        lead = np.broadcast_shapes(state.shape[:-1], disturb.shape[:-1], action.shape[:-1])
        bc = lambda a, d: np.broadcast_to(a, lead + (d,)).reshape(-1, d)
        s2, q2, a2 = bc(state, self.dim_state), bc(disturb, self.dim_disturb), bc(action, self.dim_input)
        x2 = np.broadcast_to(np.asarray(xi, dtype=float), q2.shape)
        d, dq, ca = self._engine().rhs_full(s2, q2, a2, x2, clip=clip)
        return (d.astype(float).reshape(lead + (self.dim_state,)), dq.astype(float).reshape(lead + (self.dim_disturb,)),
                ca.astype(float).reshape(lead + (self.dim_input,)))

    def _call_rhs(self, state, action, clip):
        state = np.asarray(state, dtype=float)
        action = np.asarray(action, dtype=float)
        lead = np.broadcast_shapes(state.shape[:-1], action.shape[:-1])
        s2 = np.broadcast_to(state, lead + (self.dim_state,)).reshape(-1, self.dim_state)
        a2 = np.broadcast_to(action, lead + (self.dim_input,)).reshape(-1, self.dim_input)
        d, ca = self._engine().rhs(s2, a2, clip=clip)
        return d.astype(float).reshape(lead + (self.dim_state,)), ca.astype(float).reshape(lead + (self.dim_input,))

    # ---- reference interface -----------------------------------------------------------------
    def _state_dyn(self, t, state, action, disturb=[]):
        """Right-hand side of the open-loop system (unclipped action), rcognita/systems.py:147-154; with
        ``is_disturb`` and a disturbance given it enters as in systems.py:317-319, 373-376."""
        if self.is_disturb and len(disturb):
            return self._call_rhs_full(state, disturb, action, np.zeros(self.dim_disturb), clip=False)[0]
        return self._call_rhs(state, action, clip=False)[0]

    def _disturb_dyn(self, t, disturb, xi=None):
        """rcognita/systems.py:325-345, 384-394 (2tank: zeros, :421-424).  ``xi`` = the value of ``randn()`` per
        component; default: the next draw of this object's generator."""
        if not self.is_disturb:
            raise ValueError("_disturb_dyn needs a system created with is_disturb=1")
        xi = self._draw() if xi is None else xi
        q = np.asarray(disturb, dtype=float)
        zs = np.zeros(q.shape[:-1] + (self.dim_state,))
        return self._call_rhs_full(zs, q, np.zeros(self.dim_input), xi, clip=False)[1]

    def _ctrl_dyn(self, t, action, observation):
        return np.zeros(self.dim_input)

    def out(self, state, action=[]):
        """System output (rcognita/systems.py:185-198): the state for the built-in systems; for a ``hip_policy`` with an
        ``out`` member, y = out(state) computed on the device (rcg_out), ``[dy]`` or ``[B, dy]``."""
        info = type(self)._hip_info
        if info is None or not info.get("has_out"):
            return state
        x = np.asarray(state, dtype=float)
        y = self._engine().out(x.reshape(-1, self.dim_state))
        return y.reshape(x.shape[:-1] + (self.dim_output,)).astype(float)

    def receive_action(self, action):
        """rcognita/systems.py:200-211."""
        self.action = action

    def closed_loop_rhs(self, t, state_full):
        """rcognita/systems.py:213-253: clip the stored action to ``ctrl_bnds`` (the reference clips the
        stored array in place; here the clipped value replaces ``self.action``), evaluate the dynamics,
        record ``_state``."""
        state_full = np.asarray(state_full, dtype=float)
        state = state_full[..., 0:self.dim_state]
        if self.is_disturb:  # full state [state, disturb]; one noise draw per call
            disturb = state_full[..., self.dim_state:self.dim_state + self.dim_disturb]
            d, dq, ca = self._call_rhs_full(state, disturb, self.action, self._draw(), clip=bool(self.ctrl_bnds.any()))
            self.action = ca
            self._state = state
            return np.concatenate([d, dq], axis=-1)
        d, ca = self._call_rhs(state, self.action, clip=bool(self.ctrl_bnds.any()))
        self.action = ca
        self._state = state
        return d


class Sys3WRobot(System):
    """Three-wheel robot with dynamical actuators (ENDI), rcognita/systems.py:255-351.
    state = (x, y, alpha, v, omega), action = (F, M), pars = (m, I)."""

    _sys_id = N.SYS_3WROBOT
    name = "3wrobot"


class Sys3WRobotNI(System):
    """Three-wheel robot with static actuators (non-holonomic integrator), rcognita/systems.py:353-399.
    state = (x, y, alpha), action = (v, omega)."""

    _sys_id = N.SYS_3WROBOT_NI
    name = "3wrobotNI"


class Sys2Tank(System):
    """Two-tank system with nonlinearity, rcognita/systems.py:401-428.
    state = (h1, h2), action = (u), pars = (tau1, tau2, K1, K2, K3)."""

    _sys_id = N.SYS_2TANK
    name = "2tank"
