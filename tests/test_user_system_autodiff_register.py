"""Derived adjoints for systems compiled at run time (rcg.h: the policy member AUTODIFF): what a registration reports and
compiles - hipRTC compiles without a device, so these run on CPU.  The GPU side is test_hip_user_system_autodiff.py."""
import os

import numpy as np
import pytest

from rcognita_amd import _native as N
from tests.test_user_system_critic_register import pendulum_critic_source
from tests.test_user_system_register import PENDULUM
from tests.user_systems_autodiff import (corner_ad, pendulum_ad, pendulum_loop_ad, pendulum_out_ad,
                                         with_autodiff)

PEND_PARS = [1.3, 9.81, 0.7]
BND = np.array([[-5.0, 5.0]])


def _autodiff(sid):
    v = N.C.c_int32(-1)
    rc = N.lib().rcg_system_autodiff(sid, N.C.byref(v))
    return rc, v.value


def _register(name, src, ds, du, np_):
    sid = N.C.c_int32(-1)
    rc = N.lib().rcg_register_system(name.encode(), src.encode(), ds, du, np_, N.C.byref(sid))
    return rc, sid.value, N.last_error(None)


# ---- 1. symbols and version ------------------------------------------------------------------------------------------------------
def test_the_symbols_are_exported_and_the_version_stays_125():
    L = N.lib()
    assert "rcg_system_autodiff" in N.SYMBOLS
    # rcg_jac_T: bound with its signature like every entry point (tests/test_abi.py reads lower-case names out of rcg.h, so the
    # list it compares with holds those; this one is listed beside it)
    assert "rcg_jac_T" in N.SYMBOLS + N.SYMBOLS_MIXED_CASE
    for s in ("rcg_system_autodiff", "rcg_jac_T"):
        assert getattr(L, s).argtypes is not None
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rcg.h")).read()
    assert "int rcg_jac_T(rcg_handle* h," in hdr and "int rcg_system_autodiff(int32_t sys_id, int32_t* mask);" in hdr
    assert N.RCG_VERSION == 125 and L.rcg_version() == 125


# ---- 2. what registration reports -----------------------------------------------------------------------------------------------
def test_registration_reports_the_derived_members():
    a = N.register_system("PendulumAD", pendulum_ad("PendulumAD"), 2, 1, 3)
    assert a["has_jac"] and not a["has_out"] and not a["has_out_jac"] and a["autodiff"] == 1
    assert _autodiff(a["sys_id"]) == (N.OK, 1)
    jac = N.C.c_int32(-1)
    assert N.lib().rcg_system_info(a["sys_id"], None, None, None, N.C.byref(jac)) == N.OK and jac.value == 1
    b = N.register_system("PendulumYAD", pendulum_out_ad("PendulumYAD"), 2, 1, 3)
    assert b["has_jac"] and b["has_out"] and b["has_out_jac"] and b["dy"] == 3 and b["autodiff"] == 3
    assert _autodiff(b["sys_id"]) == (N.OK, 3)
    # one of the two written by hand: the other one is derived
    c = N.register_system("PendulumYAD2", pendulum_out_ad("PendulumYAD2", drop=("out_jac_T",)), 2, 1, 3)
    assert c["has_jac"] and c["has_out_jac"] and c["autodiff"] == 2
    # every instance a hand-written jac_T brings is compiled for the derived one
    for info in (a, b):
        for real in ("float", "double"):
            exprs = [e for _, e in N.system_programs(info["sys_id"])]
            assert sum(e.startswith(f"rcg::k_actor_opt<rcg::RcgRtcSys, {real},") for e in exprs) == 8


def test_hand_written_members_win():
    a = N.register_system("PendulumHAD", with_autodiff(PENDULUM.replace("PendulumT", "PendulumHAD")), 2, 1, 3)
    assert a["has_jac"] and a["autodiff"] == 0 and _autodiff(a["sys_id"]) == (N.OK, 0)
    b = N.register_system("PendulumYHAD", with_autodiff(pendulum_critic_source("PendulumYHAD")), 2, 1, 3)
    assert b["has_jac"] and b["has_out"] and b["has_out_jac"] and b["autodiff"] == 0


def test_without_the_opt_in_nothing_is_derived():
    nojac = PENDULUM[: PENDULUM.index("  template <typename real, bool HW = false>\n  __device__ __forceinline__ static void jac_T")]
    nojac += "};\n"
    off = N.register_system("PendulumADOff", with_autodiff(nojac.replace("PendulumT", "PendulumADOff"), "false"), 2, 1, 3)
    assert not off["has_jac"] and off["autodiff"] == 0 and _autodiff(off["sys_id"]) == (N.OK, 0)
    absent = N.register_system("PendulumNoJac", nojac.replace("PendulumT", "PendulumNoJac"), 2, 1, 3)
    assert not absent["has_jac"] and absent["autodiff"] == 0
    assert not any("k_jac_T" in e or "k_actor_opt" in e for _, e in N.system_programs(absent["sys_id"]))
    plain = N.register_system("PendulumT", PENDULUM, 2, 1, 3)
    assert plain["has_jac"] and plain["autodiff"] == 0


def test_builtins_and_bad_arguments():
    for sid in (N.SYS_3WROBOT, N.SYS_3WROBOT_NI, N.SYS_2TANK):
        assert _autodiff(sid) == (N.OK, 0)
    for sid in (7, -1, N.SYS_USER_BASE + 4096):
        assert _autodiff(sid)[0] == N.ERR_BAD_ARG
    assert N.lib().rcg_system_autodiff(N.SYS_3WROBOT, None) == N.ERR_BAD_ARG
    sid = N.register_system("PendulumAD", pendulum_ad("PendulumAD"), 2, 1, 3)["sys_id"]
    assert N.lib().rcg_system_autodiff(sid, None) == N.ERR_BAD_ARG


# ---- 3. corner sources -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,mask", [("C1", 1), ("C2", 3)])
def test_corner_sources_register(key, mask):
    """C1: DS 1, DU 1, NP 0 without an output map; C2: DS 5, DU 2 (seven tangents), Pre with `real r[5]`, DY 1."""
    src, S = corner_ad(key)
    assert "jac_T" not in src and "AUTODIFF = true" in src
    info = N.register_system(S.name, src, S.ds, S.du, S.np)
    assert info["has_jac"] and info["autodiff"] == mask and info["has_out"] is S.has_out
    assert info["has_out_jac"] is S.has_out


def test_an_empty_pre_registers():
    src = """
struct EmptyPreAD {
  static constexpr int DS = 2, DU = 1, NP = 0;
  static constexpr bool AUTODIFF = true;
  template <typename real>
  struct Pre {};
  template <typename real>
  __device__ __forceinline__ static Pre<real> prepare(const real*) {
    return {};
  }
  template <typename real, bool HW = false>
  __device__ __forceinline__ static void rhs(const Pre<real>&, const real* x, const real* u, real* d) {
    d[0] = x[1] * tanh(x[0]) + sqrt(x[0] * x[0] + (real)1);
    d[1] = u[0] / (x[1] * x[1] + (real)2) - fmin(x[0], x[1]) * exp(-x[0] * x[0]);
  }
};
"""
    info = N.register_system("EmptyPreAD", src, 2, 1, 0)
    assert info["has_jac"] and info["autodiff"] == 1


# ---- 4. compile errors -----------------------------------------------------------------------------------------------------------
def test_an_unsupported_function_is_a_compile_error():
    src = pendulum_ad("PendulumErf").replace("d[0] = x[1];", "d[0] = erf(x[0]);")
    assert "erf(x[0])" in src
    rc, _, log = _register("PendulumErf", src, 2, 1, 3)
    assert rc == N.ERR_BAD_ARG
    assert "erf" in log and "PendulumErf.policy" in log, log
    with pytest.raises(N.NativeError) as ei:
        N.register_system("PendulumErf", src, 2, 1, 3)
    assert ei.value.code == N.ERR_BAD_ARG
    # the same right-hand side without the opt-in compiles: erf is the device library's on float / double
    plain = src.replace("  static constexpr bool AUTODIFF = true;\n", "").replace("PendulumErf", "PendulumErfPlain")
    assert not N.register_system("PendulumErfPlain", plain, 2, 1, 3)["has_jac"]


def test_a_pre_with_an_int_member_is_a_compile_error_naming_pre():
    src = pendulum_ad("PendulumIntPre").replace("real g_l, inv_ml2;", "real g_l, inv_ml2;\n    int flag;")
    src = src.replace("return {p[1] / p[2], (real)1 / (p[0] * p[2] * p[2])};", "return {p[1] / p[2], (real)1 / (p[0] * p[2] * p[2]), 1};")
    assert "int flag;" in src and "), 1};" in src
    rc, _, log = _register("PendulumIntPre", src, 2, 1, 3)
    assert rc == N.ERR_BAD_ARG
    assert "AUTODIFF: Pre<real> must be empty or hold members of type real only" in log, log
    # ... and without the opt-in such a Pre is the policy's own business
    plain = src.replace("  static constexpr bool AUTODIFF = true;\n", "").replace("PendulumIntPre", "PendulumIntPrePlain")
    assert not N.register_system("PendulumIntPrePlain", plain, 2, 1, 3)["has_jac"]


# ---- 5. System ----------------------------------------------------------------------------------------------------------------------
def test_hip_info_carries_the_mask():
    """(CtrlOptPred creates a handle, which needs a device: test_hip_user_system_autodiff.py constructs the controllers.)"""
    from rcognita_amd.systems import System

    class PendulumAD(System):
        hip_policy = pendulum_ad("PendulumAD")

    class PendulumT(System):
        hip_policy = PENDULUM

    class PendulumLAD(System):
        hip_policy = pendulum_loop_ad("PendulumLAD")

    for cls, mask in ((PendulumAD, 1), (PendulumT, 0), (PendulumLAD, 1)):
        cls(sys_type="diff_eqn", dim_state=2, dim_input=1, dim_output=2, dim_disturb=0, pars=PEND_PARS, ctrl_bnds=BND)
        assert cls._hip_info["autodiff"] == mask and cls._hip_info["has_jac"]
        assert _autodiff(cls._hip_info["sys_id"]) == (N.OK, mask)
    assert PendulumLAD._hip_info["has_loop"] and PendulumLAD._hip_info["has_search"]
