"""T ticks per launch on systems compiled at run time (rcg.h: the policy member TICKS): what a registration reports and compiles -
hipRTC compiles without a device, so these run on CPU.  The GPU side is test_hip_user_system_ticks.py, which takes its policy
sources from here."""
import numpy as np
import pytest

from rcognita_amd import _native as N
from tests.test_user_system_critic_register import pendulum_critic_source
from tests.test_user_system_out_register import pendulum_out_source
from tests.test_user_system_register import PENDULUM

TICKS_MEMBER = "  static constexpr bool TICKS = true;\n"
PEND_PARS = [1.3, 9.81, 0.7]
BND = np.array([[-5.0, 5.0]])


def with_ticks(src):
    """A policy source with the opt-in member added behind its dimensions (as with_critic adds CRITIC)."""
    i = src.index("static constexpr int DS")
    j = src.index("\n", i) + 1
    return src[:j] + TICKS_MEMBER + src[j:]


def pendulum_ticks_source(name):
    """The pendulum of test_user_system_register.py (DS = 2, DU = 1, no output map) that opts in to T ticks per launch."""
    return with_ticks(PENDULUM.replace("PendulumT", name))


def pendulum_out_ticks_source(name, critic=False):
    """The pendulum with y = (sin th, cos th, om) (F14 / F15) that opts in to T ticks per launch, and to the critic kernels."""
    return with_ticks(pendulum_critic_source(name) if critic else pendulum_out_source(name))


def _has_ticks(sid):
    v = N.C.c_int32(-1)
    rc = N.lib().rcg_system_has_ticks(sid, N.C.byref(v))
    return rc, v.value


def test_the_library_reports_version_125():
    assert N.RCG_VERSION == 125 and N.lib().rcg_version() == 125


def test_registration_reports_has_ticks():
    info = N.register_system("PendulumK", pendulum_ticks_source("PendulumK"), 2, 1, 3)
    assert info["has_ticks"] and not info["has_out"] and not info["has_critic"] and not info["has_search"]
    assert _has_ticks(info["sys_id"]) == (N.OK, 1)
    plain = N.register_system("PendulumT", PENDULUM, 2, 1, 3)
    assert not plain["has_ticks"] and _has_ticks(plain["sys_id"]) == (N.OK, 0)
    # TICKS = false is the default spelled out
    off = N.register_system("PendulumKOff", pendulum_ticks_source("PendulumKOff").replace("TICKS = true", "TICKS = false"), 2, 1, 3)
    assert not off["has_ticks"] and _has_ticks(off["sys_id"]) == (N.OK, 0)
    # next to the other optional members, which it leaves as they are
    both = N.register_system("PendulumYKC", pendulum_out_ticks_source("PendulumYKC", critic=True), 2, 1, 3)
    assert both["has_ticks"] and both["has_critic"] and both["has_out"] and both["dy"] == 3 and not both["has_search"]
    for sid in (N.SYS_3WROBOT, N.SYS_3WROBOT_NI, N.SYS_2TANK):
        assert _has_ticks(sid) == (N.OK, 1)
    assert _has_ticks(7)[0] == N.ERR_BAD_ARG
    assert _has_ticks(N.SYS_USER_BASE + 4096)[0] == N.ERR_BAD_ARG
    assert N.lib().rcg_system_has_ticks(7, None) == N.ERR_BAD_ARG


def test_hip_info_carries_has_ticks():
    from rcognita_amd.systems import System

    class PendulumKInfo(System):
        hip_policy = pendulum_ticks_source("PendulumKInfo")

    class PendulumPlainKInfo(System):
        hip_policy = PENDULUM.replace("PendulumT", "PendulumPlainKInfo")

    for cls, want in ((PendulumKInfo, True), (PendulumPlainKInfo, False)):
        cls(sys_type="diff_eqn", dim_state=2, dim_input=1, dim_output=2, dim_disturb=0, pars=PEND_PARS, ctrl_bnds=BND)
        assert cls._hip_info["has_ticks"] is want
        assert _has_ticks(cls._hip_info["sys_id"]) == (N.OK, int(want))


@pytest.mark.parametrize("out", [False, True])
def test_the_opt_in_adds_nothing_to_a_registration(out):
    """rcg_system_programs right after rcg_register_system: the same expressions with and without TICKS (a k_ticks / k_ticks_mem
    program is compiled on first use)."""
    if out:
        a, b = pendulum_out_ticks_source("PendulumRegYK"), pendulum_out_source("PendulumRegYK0")
    else:
        a, b = pendulum_ticks_source("PendulumRegK"), PENDULUM.replace("PendulumT", "PendulumRegK0")
    na, nb = ("PendulumRegYK", "PendulumRegYK0") if out else ("PendulumRegK", "PendulumRegK0")
    ia, ib = N.register_system(na, a, 2, 1, 3), N.register_system(nb, b, 2, 1, 3)
    assert ia["has_ticks"] and not ib["has_ticks"] and ia["has_out"] is out
    pa, pb = N.system_programs(ia["sys_id"]), N.system_programs(ib["sys_id"])
    assert len(pb) > 20 and not any("k_ticks" in e for _, e in pa)
    assert [(p.replace(na, "X"), e) for p, e in pa] == [(p.replace(nb, "X"), e) for p, e in pb]
