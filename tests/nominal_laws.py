"""Nominal control laws for systems compiled at run time (rcg.h: the policy member `nominal`), each with its NumPy twin, and the
closed loop of rcg_control_tick_nominal restated on the twins.  test_user_system_nominal_register.py checks the inputs here on
the CPU; test_hip_user_system_nominal.py runs the policies on the GPU.

    (a) the pendulum (DS 2, DU 1, NP 3), NOMINAL_NP = 2:  u = m l^2 (g/l sin th - c1 th - gain om),
        nominal_lf = 1/2 om^2 + 1/2 c1 th^2 c2; with TICKS (and variants without it, and with a `disturb` member)
    (b) the pendulum observed through y = (sin th, cos th, om) (DY 3 > DS): the same law with th = atan2(y0, y1)
    (c) corner C2 of tests/user_systems.py (DS 5, DU 2, NP 5, DY 1, per-env parameters): a law that reads Pre, NOMINAL_NP = 0,
        no nominal_lf, appended by a text helper
    (d) copies of Sys3WRobotNI / Sys3WRobot whose `nominal` restates the built-in law (rcg_nominal.hpp's own functions)
"""
import os

import numpy as np

from tests.test_user_system_disturb_register import with_disturb
from tests.test_user_system_loop_register import BND, PEND_PARS, bad_state, clean_states  # noqa: F401
from tests.test_user_system_out_register import pend_out, pendulum_out_source
from tests.test_user_system_register import PENDULUM
from tests.test_user_system_ticks_register import with_ticks
from tests.user_systems import CORNERS, make_policy, sim_substeps, stage_b

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = 0.01
GAIN, CPARS = 2.0, (4.0, 1.5)  # the pendulum law's damping (ctrl_gain) and (c1, c2): stiffness, scale of the Lyapunov function
C2_GAIN = 16.0

NOMINAL_NP_MEMBER = "  static constexpr int NOMINAL_NP = %d;\n"
PEND_LAW = """  template <typename real>
  __device__ __forceinline__ static void nominal(const Pre<real>& q, const real* y, const real* c, real* u) {
    u[0] = (q.g_l * sin(y[0]) - c[1] * y[0] - c[0] * y[1]) / q.inv_ml2;
  }
"""
PEND_LF = """  template <typename real>
  __device__ __forceinline__ static real nominal_lf(const Pre<real>&, const real* y, const real* c) {
    return (real)0.5 * y[1] * y[1] + (real)0.5 * c[1] * y[0] * y[0] * c[2];
  }
"""
PEND_OUT_LAW = """  template <typename real>
  __device__ __forceinline__ static void nominal(const Pre<real>& q, const real* y, const real* c, real* u) {
    const real th = atan2(y[0], y[1]);
    u[0] = (q.g_l * y[0] - c[1] * th - c[0] * y[2]) / q.inv_ml2;
  }
"""
PEND_OUT_LF = """  template <typename real>
  __device__ __forceinline__ static real nominal_lf(const Pre<real>&, const real* y, const real* c) {
    const real th = atan2(y[0], y[1]);
    return (real)0.5 * y[2] * y[2] + (real)0.5 * c[1] * th * th * c[2];
  }
"""
# (c): reads the prepared parameters (Pre::r) - with per-env parameters every env has its own law
C2_LAW = """  template <typename real>
  __device__ __forceinline__ static void nominal(const Pre<real>& q, const real* y, const real* c, real* u) {
    u[0] = -c[0] * q.r[0] * y[0];
    u[1] = c[0] * q.r[3] * sin(y[0]) - q.r[1];
  }
"""


def with_nominal(src, law, lf="", nominal_np=None):
    """A policy source with the law's members appended before the struct's end, and NOMINAL_NP (if given) behind its dimensions
    (as with_loop adds LOOP)."""
    if nominal_np is not None:
        i = src.index("static constexpr int DS")
        j = src.index("\n", i) + 1
        src = src[:j] + NOMINAL_NP_MEMBER % nominal_np + src[j:]
    tail = src.rindex("};")
    return src[:tail] + law + lf + src[tail:]


def pendulum_nominal_source(name, ticks=True, lf=True, nominal_np=2, law=True, disturb=False):
    """(a); `ticks` / `lf` / `law` / `nominal_np` = None leave a member out (the registration's refusals), `disturb`: with DD = 1."""
    src = PENDULUM.replace("PendulumT", name)
    if disturb:
        src = with_disturb(src)
    if ticks:
        src = with_ticks(src)
    return with_nominal(src, PEND_LAW if law else "", PEND_LF if lf else "", nominal_np)


def pendulum_out_nominal_source(name):
    """(b), with TICKS."""
    return with_nominal(with_ticks(pendulum_out_source(name)), PEND_OUT_LAW, PEND_OUT_LF, 2)


_C2 = {}


def corner_c2():
    """(c): (source, the twin of tests/user_systems.py) of corner C2 under another name, with the law appended."""
    if not _C2:
        name, ds, du, np_, dy, dd = CORNERS["C2"]
        src, twin = make_policy(name + "Nom", ds, du, np_, dy, dd)
        _C2["v"] = (with_nominal(src, C2_LAW), twin)
    return _C2["v"]


def robot_copy_source(struct, name):
    """(d): the built-in policy under another name with TICKS and a `nominal` that restates the built-in law - rcg_nominal.hpp's
    own function of that system, with (m, I) as the two controller parameters of the dynamic robot.  The copy keeps L and theta
    alive as k_nominal's built-in instance does (it may store both), so that the function is compiled with the same users.  No
    nominal_lf: the copies stand for the law (mask 1); a second call of the law function from nominal_lf is a different
    compilation context, whose Lyapunov value need not equal the built-in's to the last bit."""
    src = open(os.path.join(ROOT, "rcognita_amd", "csrc", "rcg_systems.hpp")).read()
    i = src.index(f"struct {struct} {{")
    j = src.index("\n};\n", i) + 4
    src = with_ticks(src[i:j].replace(f"struct {struct} {{", f"struct {name} {{"))
    dyn = struct == "Sys3WRobot"
    mi = "c[1], c[2]" if dyn else "(real)0, (real)0"
    law = f"""  template <typename real>
  __device__ __forceinline__ static void nominal(const Pre<real>&, const real* y, const real* c, real* u) {{
    real L, th;
    Nominal<{struct}>::template act<real>(y, c[0], {mi}, u, &L, &th);
    asm volatile("" ::"v"(L), "v"(th));
  }}
"""
    return with_nominal(src, law, "", 2 if dyn else None)


# ---- the NumPy twins ------------------------------------------------------------------------------------------------------------
class PendTwin:
    """The pendulum in the shape of tests/user_systems.py::Twin (what sim_substeps and stage_b read), with its law."""
    ds, du, np, dd = 2, 1, 3, 0

    def __init__(self, out=False, disturb=False):
        self.has_out, self.dy = out, 3 if out else 2
        self.pars, self.bnds = list(PEND_PARS), np.array(BND, dtype=float)
        self.dd = 1 if disturb else 0

    def rhs(self, x, u, p=None):
        m, g, l = self.pars if p is None else np.moveaxis(np.asarray(p), -1, 0)
        x, u = np.asarray(x), np.asarray(u)
        return np.stack(np.broadcast_arrays(x[..., 1], u[..., 0] / (m * l * l) - g / l * np.sin(x[..., 0])), axis=-1)

    def disturb(self, x, u, w, d):
        """The member with_disturb appends: d[1] += cos(th) / (m l^2) w[0]."""
        m, _, l = self.pars
        d = np.array(np.broadcast_arrays(d, x)[0], dtype=float)
        d[..., 1] = d[..., 1] + np.cos(np.asarray(x)[..., 0]) / (m * l * l) * np.asarray(w)[..., 0]
        return d

    def out(self, x):
        return pend_out(x) if self.has_out else np.asarray(x)

    def clip(self, u):
        return np.clip(u, self.bnds[:, 0], self.bnds[:, 1])

    def law(self, y, gain, cpars, p=None):
        m, g, l = self.pars if p is None else np.moveaxis(np.asarray(p), -1, 0)
        y = np.asarray(y, dtype=float)
        if self.has_out:
            th, s, om = np.arctan2(y[..., 0], y[..., 1]), y[..., 0], y[..., 2]
        else:
            th, s, om = y[..., 0], np.sin(y[..., 0]), y[..., 1]
        return (m * l * l * (g / l * s - cpars[0] * th - gain * om))[..., None]

    def lf(self, y, gain, cpars, p=None):
        y = np.asarray(y, dtype=float)
        th, om = (np.arctan2(y[..., 0], y[..., 1]), y[..., 2]) if self.has_out else (y[..., 0], y[..., 1])
        return 0.5 * om * om + 0.5 * cpars[0] * th * th * cpars[1]


class C2Twin:
    """The law of (c) on the corner's twin."""

    def __init__(self):
        self.S = corner_c2()[1]

    def __getattr__(self, k):
        return getattr(self.S, k)

    def law(self, y, gain, cpars, p=None):
        r = self.S._r(self.S.pars if p is None else p)
        y = np.asarray(y, dtype=float)
        return np.stack(np.broadcast_arrays(-gain * r[..., 0] * y[..., 0], gain * r[..., 3] * np.sin(y[..., 0]) - r[..., 1]), axis=-1)


def twin_tick(S, x, u, accum, gain, cpars, R1, target=None, pars=None, n_sub=1, dt=DT, dist=None):
    """rcg_control_tick_nominal on a twin: the env step under the held action (sim_substeps), ACTION := the clipped law of out(STATE),
    ACCUM += stage_obj(out(STATE), ACTION) * sampling_time.  Returns (x, u, accum) and, disturbed, (q, sub) too."""
    step = sim_substeps(S, x, u, n_sub, dt, pars=pars, dist=dist)
    x = step[0]
    y = S.out(x)
    u = S.clip(S.law(y, gain, cpars, pars))
    accum = accum + stage_b(y, u, R1, target) * dt
    return (x, u, accum) if dist is None else (x, u, accum, step[1], step[3])


def f32_round(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def ulp32_distance(got, want64):
    """|got - float32(want64)| in units of float32 ulps at want64 (got: float32 values)."""
    w = np.asarray(want64, dtype=np.float64).astype(np.float32)
    ulp = np.spacing(np.abs(w)).astype(np.float64)
    return np.abs(np.asarray(got, dtype=np.float64) - w.astype(np.float64)) / ulp


# ---- the batches of the GPU file ---------------------------------------------------------------------------------------------------
def pend_batch(B, seed=11):
    """Start states of (a) / (b): angles inside (-pi, pi), so that atan2 of (b) returns the angle itself."""
    return clean_states(B, seed)


def c2_batch(B, seed=5):
    S = corner_c2()[1]
    rng = np.random.default_rng(seed)
    return S.rand_states(rng, B), np.array(S.pars) * rng.uniform(0.8, 1.2, (B, S.np))
