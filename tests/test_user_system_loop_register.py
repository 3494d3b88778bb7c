"""The fused loop step on systems compiled at run time (rcg.h: the policy member LOOP): what a registration reports and compiles -
hipRTC compiles without a device, so these run on CPU - and the NumPy pendulum that shows which start states freeze an env.  The
GPU side is test_hip_user_system_loop.py, which takes its policy sources and states from here."""
import numpy as np
import pytest

from rcognita_amd import _native as N
from tests.test_user_system_critic_register import pendulum_critic_source
from tests.test_user_system_register import PENDULUM
from tests.test_user_system_search_register import with_search

LOOP_MEMBER = "  static constexpr bool LOOP = true;\n"
PEND_PARS = [1.3, 9.81, 0.7]
BND = np.array([[-5.0, 5.0]])


def with_loop(src):
    """A policy source with the opt-in member added behind its dimensions (as with_critic adds CRITIC)."""
    i = src.index("static constexpr int DS")
    j = src.index("\n", i) + 1
    return src[:j] + LOOP_MEMBER + src[j:]


def pendulum_loop_source(name):
    """The pendulum of test_user_system_register.py (DS = 2, DU = 1, no output map) that opts in to the fused loop step."""
    return with_loop(PENDULUM.replace("PendulumT", name))


def pendulum_out_loop_source(name):
    """The pendulum with y = (sin th, cos th, om) (F14 / F15: DY = 3 > DS) with CRITIC and LOOP."""
    return with_loop(pendulum_critic_source(name))


def pendulum_loop_nojac_source(name):
    """The LOOP pendulum without jac_T (with SEARCH, so that a controller can decide): its steps are served, a fused decision
    is not."""
    src = with_search(pendulum_loop_source(name))
    return src[: src.index("  template <typename real, bool HW = false>\n  __device__ __forceinline__ static void jac_T")] + "};\n"


# ---- the NumPy pendulum: which start states freeze an env ---------------------------------------------------------------------
def bad_state(dtype):
    """Finite, and non-finite after the first RK4 step at any dt: k1 + 2 k2 + 2 k3 + k4 of the angle is six times a rate within a
    factor two of the element type's largest number (the recipe of test_freeze_states.py::bad_now_state)."""
    return np.array([0.0, 3e38 if dtype == "f32" else 1.7e308])


def clean_states(B, seed=11):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-3, 3, B), rng.uniform(-2, 2, B)], axis=-1)


def pend_rk4(x, u, dt, real, pars=PEND_PARS):
    """One classical RK4 step of the pendulum in the arithmetic of `real`, combined as the library combines it."""
    f = np.dtype(real).type
    m, g, l = (f(v) for v in pars)
    x, u, dt = np.asarray(x, dtype=real), np.asarray(u, dtype=real), f(dt)

    def rhs(s):
        return np.stack([s[..., 1], u[..., 0] / (m * l * l) - g / l * np.sin(s[..., 0])], axis=-1)

    with np.errstate(over="ignore", invalid="ignore"):
        k1 = rhs(x)
        k2 = rhs(x + f(0.5) * dt * k1)
        k3 = rhs(x + f(0.5) * dt * k2)
        k4 = rhs(x + dt * k3)
        return x + dt / f(6) * (((k1 + f(2) * k2) + f(2) * k3) + k4)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_the_bad_state_is_finite_and_its_first_step_is_not(dtype):
    real = np.float32 if dtype == "f32" else np.float64
    x = bad_state(dtype).astype(real)
    assert np.all(np.isfinite(x))
    for dt in (0.005, 0.01):
        assert not np.all(np.isfinite(pend_rk4(x[None], np.array([[-0.5]]), dt, real)))
    clean = clean_states(16)
    for u in (-5.0, 0.0, 5.0):
        assert np.all(np.isfinite(pend_rk4(clean, np.full((16, 1), u), 0.01, real)))


# ---- registration --------------------------------------------------------------------------------------------------------------
def _has_loop(sid):
    v = N.C.c_int32(-1)
    rc = N.lib().rcg_system_has_loop(sid, N.C.byref(v))
    return rc, v.value


def test_the_symbol_is_exported_and_the_version_stays_125():
    assert "rcg_system_has_loop" in N.SYMBOLS
    assert N.RCG_VERSION == 125 and N.lib().rcg_version() == 125


def test_registration_reports_has_loop():
    info = N.register_system("PendulumL", pendulum_loop_source("PendulumL"), 2, 1, 3)
    assert info["has_loop"] and info["has_jac"] and not info["has_out"] and not info["has_critic"] and not info["has_ticks"]
    assert _has_loop(info["sys_id"]) == (N.OK, 1)
    plain = N.register_system("PendulumT", PENDULUM, 2, 1, 3)
    assert not plain["has_loop"] and _has_loop(plain["sys_id"]) == (N.OK, 0)
    # LOOP = false is the default spelled out
    off = N.register_system("PendulumLOff", pendulum_loop_source("PendulumLOff").replace("LOOP = true", "LOOP = false"), 2, 1, 3)
    assert not off["has_loop"] and _has_loop(off["sys_id"]) == (N.OK, 0)
    # next to the other optional members, which it leaves as they are
    both = N.register_system("PendulumYCL", pendulum_out_loop_source("PendulumYCL"), 2, 1, 3)
    assert both["has_loop"] and both["has_critic"] and both["has_out"] and both["has_out_jac"] and both["dy"] == 3
    assert not both["has_search"] and not both["has_ticks"] and both["dd"] == 0
    assert _has_loop(both["sys_id"]) == (N.OK, 1)
    for sid in (N.SYS_3WROBOT, N.SYS_3WROBOT_NI, N.SYS_2TANK):
        assert _has_loop(sid) == (N.OK, 1)
    assert _has_loop(7)[0] == N.ERR_BAD_ARG
    assert _has_loop(-1)[0] == N.ERR_BAD_ARG
    assert _has_loop(N.SYS_USER_BASE + 4096)[0] == N.ERR_BAD_ARG
    assert N.lib().rcg_system_has_loop(N.SYS_3WROBOT, None) == N.ERR_BAD_ARG
    assert N.lib().rcg_system_has_loop(info["sys_id"], None) == N.ERR_BAD_ARG


def test_hip_info_carries_has_loop():
    from rcognita_amd.systems import System

    class PendulumL(System):
        hip_policy = pendulum_loop_source("PendulumL")  # (the registration above: same name, same source)

    class PendulumT(System):
        hip_policy = PENDULUM

    for cls, want in ((PendulumL, True), (PendulumT, False)):
        cls(sys_type="diff_eqn", dim_state=2, dim_input=1, dim_output=2, dim_disturb=0, pars=PEND_PARS, ctrl_bnds=BND)
        assert cls._hip_info["has_loop"] is want
        assert _has_loop(cls._hip_info["sys_id"]) == (N.OK, int(want))


@pytest.mark.parametrize("out", [False, True])
def test_the_opt_in_adds_nothing_to_a_registration(out):
    """rcg_system_programs right after rcg_register_system: the same expressions with and without LOOP (the loop program is
    compiled the first time a handle calls rcg_loop_step)."""
    if out:
        na, nb = "PendulumYCL", "PendulumYCL0"
        a, b = pendulum_out_loop_source(na), pendulum_critic_source(nb)
    else:
        na, nb = "PendulumL", "PendulumT"
        a, b = pendulum_loop_source(na), PENDULUM
    ia, ib = N.register_system(na, a, 2, 1, 3), N.register_system(nb, b, 2, 1, 3)
    assert ia["has_loop"] and not ib["has_loop"] and ia["has_out"] is out
    core = lambda i: [(p.replace(i["name"], "X"), e) for p, e in N.system_programs(i["sys_id"])  # noqa: E731
                      if p in (i["name"] + "_f32.hip", i["name"] + "_f64.hip")]
    pa, pb = N.system_programs(ia["sys_id"]), N.system_programs(ib["sys_id"])
    assert len(core(ib)) > 20 and not any("k_loop" in e or ("k_actor_opt" in e and e.count(",") == 5)
                                          for _, e in core(ia))  # (the LOOP instance carries a sixth template argument)
    assert core(ia) == core(ib)
    # beyond the two core programs there is only what a handle on a GPU has asked for since (another test of this process)
    if len(pa) == len(core(ia)) and len(pb) == len(core(ib)):
        assert [(p.replace(na, "X"), e) for p, e in pa] == [(p.replace(nb, "X"), e) for p, e in pb]
    else:
        assert all("_f32.hip" not in p and "_f64.hip" not in p for p, _ in pa[len(core(ia)):])
