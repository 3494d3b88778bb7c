"""Policies that opt in to derived adjoints (rcg.h: the policy member AUTODIFF), made from the sources the other
test_user_system_* files use by cutting their hand-written jac_T / out_jac_T out.  Shared by
test_user_system_autodiff_register.py (CPU) and test_hip_user_system_autodiff.py (GPU)."""
from tests.test_user_system_critic_register import pendulum_critic_source
from tests.test_user_system_loop_register import pendulum_loop_nojac_source
from tests.test_user_system_register import PENDULUM
from tests.user_systems import CORNERS, make_policy

AUTODIFF_MEMBER = "  static constexpr bool AUTODIFF = true;\n"
_HEAD = "  template <typename real, bool HW = false>\n"


def _cut_member(src, member):
    """`src` without the block of `member`: from its `template <typename real, bool HW = false>` line to the closing `  }`."""
    k = src.find(f" static void {member}(")
    if k < 0:
        return src
    i = src.rindex(_HEAD, 0, k)
    j = src.index("\n  }\n", k) + len("\n  }\n")
    return src[:i] + src[j:]


def with_autodiff(src, value="true"):
    """A policy source with the opt-in member added behind its dimensions (as with_loop adds LOOP)."""
    i = src.index("static constexpr int DS")
    j = src.index("\n", i) + 1
    return src[:j] + AUTODIFF_MEMBER.replace("true", value) + src[j:]


def autodiff_source(src, name, drop=("jac_T", "out_jac_T")):
    """`src` (one struct) renamed to `name`, without the members named in `drop`, with AUTODIFF = true."""
    old = src[src.index("struct ") + len("struct "):].split()[0]
    src = src.replace(old, name)
    for member in drop:
        src = _cut_member(src, member)
    return with_autodiff(src)


def pendulum_ad(name):
    """The pendulum of test_user_system_register.py with rhs alone, and the opt-in."""
    return autodiff_source(PENDULUM, name)


def pendulum_out_ad(name, drop=("jac_T", "out_jac_T")):
    """The pendulum with y = (sin th, cos th, om) and CRITIC (pendulum_critic_source) without its two adjoint members."""
    return autodiff_source(pendulum_critic_source("PendulumSrc"), name, drop)


def pendulum_loop_ad(name):
    """The LOOP + SEARCH pendulum without jac_T (pendulum_loop_nojac_source), plus the opt-in."""
    return with_autodiff(pendulum_loop_nojac_source(name))


def corner_ad(key, suffix="AD", drop=("jac_T", "out_jac_T")):
    """(source, twin) of the corner system `key` under the name <name><suffix> with the opt-in, its members in `drop` cut out."""
    name, ds, du, np_, dy, dd = CORNERS[key]
    src, twin = make_policy(name + suffix, ds, du, np_, dy, dd)
    return autodiff_source(src, name + suffix, drop), twin
