"""Registering a system compiled at run time (rcg_register_system): hipRTC compiles without a device, so these run on CPU."""
import pytest

from rcognita_amd import _native as N

# the pendulum of INTEGRATION.md ("Your own system"): state (angle, angular rate), action (torque), pars (m, g, l)
PENDULUM = r"""
struct PendulumT {
  static constexpr int DS = 2, DU = 1, NP = 3;
  template <typename real>
  struct Pre {
    real g_l, inv_ml2;
  };
  template <typename real>
  __device__ __forceinline__ static Pre<real> prepare(const real* p) {
    return {p[1] / p[2], (real)1 / (p[0] * p[2] * p[2])};
  }
  template <typename real, bool HW = false>
  __device__ __forceinline__ static void rhs(const Pre<real>& q, const real* x, const real* u, real* d) {
    real s, c;
    sincos_sel<real, HW>(x[0], &s, &c);
    d[0] = x[1];
    d[1] = fma_r(q.inv_ml2, u[0], -q.g_l * s);
  }
  template <typename real, bool HW = false>
  __device__ __forceinline__ static void jac_T(const Pre<real>& q, const real* x, const real*, const real* lam, real* ax,
                                               real* bu) {
    real s, c;
    sincos_sel<real, HW>(x[0], &s, &c);
    ax[0] = -q.g_l * c * lam[1];
    ax[1] = lam[0];
    bu[0] = q.inv_ml2 * lam[1];
  }
};
"""


def _register(name, src, ds, du, np_):
    L = N.lib()
    sid = N.C.c_int32(-1)
    rc = L.rcg_register_system(name.encode(), src.encode(), ds, du, np_, N.C.byref(sid))
    return rc, sid.value, N.last_error(None)


def test_pendulum_registers_once_with_a_user_id():
    info = N.register_system("PendulumT", PENDULUM, 2, 1, 3)
    assert info["sys_id"] >= N.SYS_USER_BASE and info["has_jac"]
    assert N.SYS_DIMS[info["sys_id"]] == (2, 1, 3)
    major, _ = info["hiprtc"]
    assert major >= 6
    rc, sid, _ = _register("PendulumT", PENDULUM, 2, 1, 3)
    assert rc == N.OK and sid == info["sys_id"]
    ds, du, np_, jac = (N.C.c_int32() for _ in range(4))
    assert N.lib().rcg_system_info(sid, N.C.byref(ds), N.C.byref(du), N.C.byref(np_), N.C.byref(jac)) == N.OK
    assert (ds.value, du.value, np_.value, jac.value) == (2, 1, 3, 1)


def test_a_policy_without_jac_registers_without_the_optimiser():
    src = PENDULUM.replace("PendulumT", "PendulumNoJac")
    src = src[: src.index("  template <typename real, bool HW = false>\n  __device__ __forceinline__ static void jac_T")] + "};\n"
    info = N.register_system("PendulumNoJac", src, 2, 1, 3)
    assert info["sys_id"] >= N.SYS_USER_BASE and not info["has_jac"]


def test_a_syntax_error_is_bad_arg_with_the_line_in_the_log():
    src = PENDULUM.replace("PendulumT", "PendulumBroken").replace("d[0] = x[1];", "d[0] = x[1]\n    !!;")
    rc, _, log = _register("PendulumBroken", src, 2, 1, 3)
    assert rc == N.ERR_BAD_ARG
    line = next(i + 1 for i, t in enumerate(src.split("\n")) if "!!;" in t)
    assert f"PendulumBroken.policy:{line}:" in log, log


def test_declared_dims_must_match_the_struct():
    src = PENDULUM.replace("PendulumT", "PendulumDims")
    rc, _, log = _register("PendulumDims", src, 3, 1, 3)
    assert rc == N.ERR_BAD_ARG
    assert "DS differs from the declared ds" in log, log


def test_dims_beyond_the_limits_are_unsupported():
    src = PENDULUM.replace("PendulumT", "Pendulum6").replace("DS = 2", "DS = 6")
    rc, _, log = _register("Pendulum6", src, 6, 1, 3)
    assert rc == N.ERR_UNSUPPORTED, log
    rc, _, _ = _register("Pendulum6", src, 2, 3, 3)
    assert rc == N.ERR_UNSUPPORTED


def test_the_same_name_with_another_source_is_bad_arg():
    N.register_system("PendulumT", PENDULUM, 2, 1, 3)
    rc, _, log = _register("PendulumT", PENDULUM.replace("p[1] / p[2]", "p[1] / p[2] * (real)2"), 2, 1, 3)
    assert rc == N.ERR_BAD_ARG and "another source" in log


def test_bad_names_and_ids_are_refused():
    rc, _, _ = _register("not an identifier", PENDULUM, 2, 1, 3)
    assert rc == N.ERR_BAD_ARG
    for sid in (3, 15, N.SYS_USER_BASE + 999):
        assert N.lib().rcg_system_info(sid, None, None, None, None) == N.ERR_BAD_ARG


def test_hip_policy_class_with_the_wrong_dim_state_raises_value_error():
    from rcognita_amd.systems import System

    class Pendulum(System):
        hip_policy = PENDULUM

    with pytest.raises(ValueError):
        Pendulum(sys_type="diff_eqn", dim_state=3, dim_input=1, dim_output=3, dim_disturb=0, pars=[1.0, 9.81, 1.0])
    assert Pendulum._sys_id >= N.SYS_USER_BASE


def test_hip_policy_class_refuses_disturbance_and_out():
    from rcognita_amd.systems import System

    class PendulumD(System):
        hip_policy = PENDULUM

    with pytest.raises(NotImplementedError, match="hip_policy"):
        PendulumD(sys_type="diff_eqn", dim_state=2, dim_input=1, dim_output=2, dim_disturb=1, pars=[1.0, 9.81, 1.0],
                  is_disturb=1, pars_disturb=[[0.0], [0.0], [1.0]])

    class PendulumOut(System):
        hip_policy = PENDULUM

        def out(self, state, action=[]):
            return state[:1]

    with pytest.raises(NotImplementedError, match="hip_policy"):
        PendulumOut(sys_type="diff_eqn", dim_state=2, dim_input=1, dim_output=2, dim_disturb=0, pars=[1.0, 9.81, 1.0])


def test_hip_policy_dims_are_read_from_code_not_comments():
    from rcognita_amd.systems import System

    class PendulumC(System):  # a comment that names another struct and another DS comes first
        hip_policy = "// struct Decoy { DS = 3; }\n/* DS = 4, */" + PENDULUM.replace("PendulumT", "PendulumC")

    s = PendulumC(sys_type="diff_eqn", dim_state=2, dim_input=1, dim_output=2, dim_disturb=0, pars=[1.0, 9.81, 1.0])
    assert N.SYS_DIMS[PendulumC._sys_id] == (2, 1, 3) and s.dim_state == 2

    class PendulumE(System):  # dimensions as expressions: the constructor's are declared and the compiler checks them
        hip_policy = PENDULUM.replace("PendulumT", "PendulumE").replace("DS = 2", "DS = 1 + 1")

    with pytest.raises(ValueError, match="do not match"):
        PendulumE(sys_type="diff_eqn", dim_state=3, dim_input=1, dim_output=3, dim_disturb=0, pars=[1.0, 9.81, 1.0])
