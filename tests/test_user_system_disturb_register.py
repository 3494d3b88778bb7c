"""The disturbance model of systems compiled at run time (rcg.h: the policy members DD and `disturb`): what a registration
reports and compiles - hipRTC compiles without a device, so these run on CPU - and the NumPy restatement of the disturbed
pendulum that the GPU tests (test_hip_user_system_disturb.py) compare against, pinned here on the reference's own results
(tests/golden/F16_disturb_pendulum.npz, tools/gen_user_system_disturb_fixture.py)."""
import json
import os

import numpy as np
import pytest

from rcognita_amd import _native as N
from tests.test_user_system_out_register import pend_out, pendulum_out_source
from tests.test_user_system_register import PENDULUM
from tests.test_user_system_ticks_register import BND, PEND_PARS, with_ticks

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "F16_disturb_pendulum.npz")

# the disturbance is a torque, scaled by the state so that the `x` argument matters; DD = 2: and a rate on the angle
_DISTURB_MEMBER = r"""
  template <typename real>
  __device__ __forceinline__ static void disturb(const Pre<real>& q, const real* x, const real*, const real* w, real* d) {
    d[1] = fma_r(q.inv_ml2 * cos(x[0]), w[0], d[1]);%s
  }
"""
_DD2_LINE = "\n    d[0] += w[1];"


def with_disturb(src, dd=1, member=True, declare=True, body=None):
    """A policy source with `static constexpr int DD = dd;` behind its dimensions (as with_ticks adds TICKS) and the `disturb`
    member before the struct's closing brace; `body`: another member text."""
    if declare:
        i = src.index("static constexpr int DS")
        j = src.index("\n", i) + 1
        src = src[:j] + f"  static constexpr int DD = {dd};\n" + src[j:]
    if member:
        tail = src.rindex("};")
        src = src[:tail] + (body if body is not None else _DISTURB_MEMBER % (_DD2_LINE if dd == 2 else "")) + src[tail:]
    return src


def pendulum_disturb_source(name, dd=1, ticks=False, out=False):
    """The pendulum of test_user_system_register.py (or, `out`, the one with y = (sin th, cos th, om)) with the disturbance model,
    and TICKS if asked for."""
    src = with_disturb(pendulum_out_source(name) if out else PENDULUM.replace("PendulumT", name), dd)
    return with_ticks(src) if ticks else src


# ---- NumPy restatement -------------------------------------------------------------------------------------------------------
def pend_rhs_full(x, q, u, xi, sigma, mu, tau, pars=PEND_PARS):
    """closed_loop_rhs on [state, disturb] with the (already clipped) action: _state_dyn(t, x, u, q) of the fixture's class and the
    filter dq_k/dt = -tau_k (q_k + sigma_k (xi_k + mu_k)) (systems.py:343).  x [..., 2], q / xi [..., dd], u [..., 1]."""
    m, g, l = pars
    dd = q.shape[-1]
    d0 = x[..., 1] + (q[..., 1] if dd == 2 else 0.0)
    d1 = -g / l * np.sin(x[..., 0]) + u[..., 0] / (m * l * l) + np.cos(x[..., 0]) / (m * l * l) * q[..., 0]
    dq = -np.asarray(tau)[:dd] * (q + np.asarray(sigma)[:dd] * (xi[..., :dd] + np.asarray(mu)[:dd]))
    return np.stack([d0, d1], axis=-1), dq


def pend_sim_substeps(x, q, u, sub, ep, n_substeps, dt, sigma, mu, tau, seed=0, env_id_base=0, pars=PEND_PARS, stage=None):
    """Twin of rcg_sim_step on a disturbed pendulum handle: the action clipped to BND, per substep one noise draw per env
    (oracle.disturb_oracle.disturb_noise) held over the four RK4 stages, the combination order of rk4_step_full.  `stage(x, u)`:
    the stage cost charged after every substep (accum_every_substep), summed into the third result.  Returns (x, q, acc, sub)."""
    from oracle.disturb_oracle import disturb_noise

    a = np.clip(u, BND[:, 0], BND[:, 1])
    ids = env_id_base + np.arange(x.shape[0], dtype=np.int64)
    acc = np.zeros(x.shape[0])
    sub = np.asarray(sub, dtype=np.int32).copy()
    f = lambda xx, qq: pend_rhs_full(xx, qq, a, xi, sigma, mu, tau, pars)
    for _ in range(n_substeps):
        xi = disturb_noise(seed, ids, ep, sub)
        k1x, k1q = f(x, q)
        k2x, k2q = f(x + 0.5 * dt * k1x, q + 0.5 * dt * k1q)
        k3x, k3q = f(x + 0.5 * dt * k2x, q + 0.5 * dt * k2q)
        k4x, k4q = f(x + dt * k3x, q + dt * k3q)
        x = x + dt / 6 * (((k1x + 2 * k2x) + 2 * k3x) + k4x)
        q = q + dt / 6 * (((k1q + 2 * k2q) + 2 * k3q) + k4q)
        sub = sub + np.int32(1)
        if stage is not None:
            acc = acc + stage(x, a)
    return x, q, acc, sub


def load_f16():
    z = np.load(GOLDEN)
    return json.loads(str(z["meta"])), z


# ---- registration ------------------------------------------------------------------------------------------------------------
def _register(name, src, ds=2, du=1, np_=3):
    sid = N.C.c_int32(-1)
    rc = N.lib().rcg_register_system(name.encode(), src.encode(), ds, du, np_, N.C.byref(sid))
    return rc, sid.value, N.last_error(None)


def _disturb_dim(sid):
    v = N.C.c_int32(-7)
    rc = N.lib().rcg_system_disturb_dim(sid, N.C.byref(v))
    return rc, v.value


def test_registration_reports_dd():
    one = N.register_system("PendulumD1", pendulum_disturb_source("PendulumD1"), 2, 1, 3)
    two = N.register_system("PendulumD2", pendulum_disturb_source("PendulumD2", dd=2), 2, 1, 3)
    plain = N.register_system("PendulumT", PENDULUM, 2, 1, 3)
    assert (one["dd"], two["dd"], plain["dd"]) == (1, 2, 0)
    assert not one["has_ticks"] and not one["has_out"] and one["has_jac"]
    assert N.DIM_DISTURB[one["sys_id"]] == 1 and N.DIM_DISTURB[two["sys_id"]] == 2 and plain["sys_id"] not in N.DIM_DISTURB
    both = N.register_system("PendulumYDK", pendulum_disturb_source("PendulumYDK", ticks=True, out=True), 2, 1, 3)
    assert both["dd"] == 1 and both["has_ticks"] and both["has_out"] and both["dy"] == 3


def test_rcg_system_disturb_dim():
    one = N.register_system("PendulumD1", pendulum_disturb_source("PendulumD1"), 2, 1, 3)
    two = N.register_system("PendulumD2", pendulum_disturb_source("PendulumD2", dd=2), 2, 1, 3)
    plain = N.register_system("PendulumT", PENDULUM, 2, 1, 3)
    assert _disturb_dim(one["sys_id"]) == (N.OK, 1)
    assert _disturb_dim(two["sys_id"]) == (N.OK, 2)
    assert _disturb_dim(plain["sys_id"]) == (N.OK, 0)
    assert [_disturb_dim(s) for s in (N.SYS_3WROBOT, N.SYS_3WROBOT_NI, N.SYS_2TANK)] == [(N.OK, 2), (N.OK, 2), (N.OK, 1)]
    for sid in (3, 7, -1, N.SYS_USER_BASE + 4096):
        assert _disturb_dim(sid)[0] == N.ERR_BAD_ARG
    assert N.lib().rcg_system_disturb_dim(N.SYS_3WROBOT, None) == N.ERR_BAD_ARG
    assert N.lib().rcg_system_disturb_dim(7, None) == N.ERR_BAD_ARG
    assert "rcg_system_disturb_dim" in N.SYMBOLS and N.RCG_VERSION == 125  # (the symbol is how a caller detects the feature)


def test_dd_beyond_two_is_unsupported_and_half_an_opt_in_is_bad_arg():
    plain = PENDULUM.replace("PendulumT", "PendulumD3")
    rc, _, log = _register("PendulumD3", with_disturb(plain, dd=3))
    assert rc == N.ERR_UNSUPPORTED and "DD" in log, log
    rc, _, log = _register("PendulumD0", with_disturb(PENDULUM.replace("PendulumT", "PendulumD0"), dd=0))
    assert rc == N.ERR_UNSUPPORTED, log
    rc, _, log = _register("PendulumDOnly", with_disturb(PENDULUM.replace("PendulumT", "PendulumDOnly"), member=False))
    assert rc == N.ERR_BAD_ARG
    assert "PendulumDOnly defines DD but no disturb member" in log, log
    rc, _, log = _register("PendulumNoDD", with_disturb(PENDULUM.replace("PendulumT", "PendulumNoDD"), declare=False))
    assert rc == N.ERR_BAD_ARG
    assert "PendulumNoDD defines disturb but no DD member" in log, log


@pytest.mark.parametrize("out", [False, True])
def test_the_opt_in_adds_nothing_to_a_registration(out):
    """rcg_system_programs right after rcg_register_system: the same expressions with and without DD / disturb (the disturb
    program - k_sim_dist, k_rhs_full - is compiled on first use)."""
    na, nb = ("PendulumRegYD", "PendulumRegYD0") if out else ("PendulumRegD", "PendulumRegD0")
    a = pendulum_disturb_source(na, out=out)
    b = pendulum_out_source(nb) if out else PENDULUM.replace("PendulumT", nb)
    ia, ib = N.register_system(na, a, 2, 1, 3), N.register_system(nb, b, 2, 1, 3)
    assert ia["dd"] == 1 and ib["dd"] == 0 and ia["has_out"] is out
    pa, pb = N.system_programs(ia["sys_id"]), N.system_programs(ib["sys_id"])
    assert len(pb) > 20 and not any("k_sim_dist" in e or "k_rhs_full" in e for _, e in pa)
    assert [(p.replace(na, "X"), e) for p, e in pa] == [(p.replace(nb, "X"), e) for p, e in pb]


def _pendulum(cls, **kw):
    args = dict(sys_type="diff_eqn", dim_state=2, dim_input=1, dim_output=2, dim_disturb=1, pars=PEND_PARS, ctrl_bnds=BND,
                is_disturb=1, pars_disturb=[[2.0], [0.5], [1.5]])
    args.update(kw)
    return cls(**args)


def test_hip_policy_class_accepts_is_disturb():
    from rcognita_amd.systems import System

    class PendulumDSys(System):
        hip_policy = pendulum_disturb_source("PendulumDSys")

    s = _pendulum(PendulumDSys)
    assert PendulumDSys._hip_info["dd"] == 1 and N.DIM_DISTURB[PendulumDSys._sys_id] == 1
    assert s._dim_full_state == 3 and s.is_disturb and s.dim_disturb == 1
    assert (s.sigma_disturb, s.mu_disturb, s.tau_disturb) == ([2.0], [0.5], [1.5])
    with pytest.raises(ValueError, match="dim_disturb = 1"):
        _pendulum(PendulumDSys, dim_disturb=2, pars_disturb=[[2.0, 1.0], [0.5, 0.0], [1.5, 1.0]])
    assert _pendulum(PendulumDSys, is_disturb=0, dim_disturb=0, pars_disturb=[])._dim_full_state == 2
    # the engine's config for such a system carries the flag and the filter's parameters
    from rcognita_amd import EngineConfig

    c = EngineConfig(sys_id=PendulumDSys._sys_id, batch=4, dtype="f64", pars=PEND_PARS, ctrl_bnds=BND, is_disturb=True,
                     pars_disturb=[[2.0], [0.5], [1.5]], disturb_init=[0.25], seed=3).to_native()
    assert c.flags & N.FLAG_DISTURB and list(c.pars_disturb) == [2.0, 0.0, 0.5, 0.0, 1.5, 0.0] and c.disturb_init[0] == 0.25


def test_a_hip_policy_without_disturb_still_refuses_is_disturb():
    from rcognita_amd import EngineConfig
    from rcognita_amd.systems import System

    class PendulumPlainD(System):
        hip_policy = PENDULUM.replace("PendulumT", "PendulumPlainD")

    with pytest.raises(NotImplementedError, match="hip_policy") as e:
        _pendulum(PendulumPlainD)
    assert "`disturb` member" in str(e.value)
    with pytest.raises(NotImplementedError, match="disturb"):
        EngineConfig(sys_id=PendulumPlainD._sys_id, batch=4, pars=PEND_PARS, ctrl_bnds=BND, is_disturb=True,
                     pars_disturb=[[2.0], [0.5], [1.5]]).to_native()


# ---- the restatement against the reference ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dd", [1, 2])
def test_restatement_reproduces_the_reference_rhs_full(dd):
    meta, z = load_f16()
    p = f"dd{dd}_"
    assert z[p + "state"].shape == (meta["n"], 2) == (256, 2) and z[p + "disturb"].shape == (256, dd)
    a = np.clip(z[p + "action"], BND[:, 0], BND[:, 1])
    np.testing.assert_array_equal(a, z[p + "action_clipped"])
    assert np.any(a != z[p + "action"])
    dx, dq = pend_rhs_full(z[p + "state"], z[p + "disturb"], a, z[p + "xi"], z[p + "sigma"], z[p + "mu"], z[p + "tau"], meta["pars"])
    ref = z[p + "rhs_full"]
    assert meta["pars"] == PEND_PARS
    assert np.max(np.abs(dx - ref[:, :2]) / np.maximum(1.0, np.abs(ref[:, :2]))) <= 1e-13
    assert np.max(np.abs(dq - ref[:, 2:]) / np.maximum(1.0, np.abs(ref[:, 2:]))) <= 1e-13
    # the state argument matters: without the cos(theta) scaling the torque row is another one
    flat = ref[:, 1] - (np.cos(z[p + "state"][:, 0]) - 1.0) / (PEND_PARS[0] * PEND_PARS[2] ** 2) * z[p + "disturb"][:, 0]
    assert np.median(np.abs(flat - ref[:, 1])) > 0.1


def test_the_out_pendulum_restatement_charges_at_out_of_x():
    """pend_sim_substeps with a stage cost at y = out(x) (DY = 3): what test_hip_user_system_disturb.py holds FIELD_ACCUM to
    differs from a cost charged at the state."""
    rng = np.random.default_rng(4)
    x = np.stack([rng.uniform(-3, 3, 16), rng.uniform(-2, 2, 16)], axis=-1)
    w = np.array([5.0, 5.0, 0.5, 0.1])
    at_y = lambda xx, a: np.einsum("bi,i,bi->b", np.concatenate([pend_out(xx), a], -1), w, np.concatenate([pend_out(xx), a], -1))
    at_x = lambda xx, a: np.einsum("bi,i,bi->b", np.concatenate([xx, a], -1), w[[0, 1, 3]], np.concatenate([xx, a], -1))
    args = (x, np.zeros((16, 1)), np.ones((16, 1)), np.zeros(16, np.int32), np.zeros(16, np.int32), 2, 0.01, [2.0], [0.5], [1.5])
    ay, ax = pend_sim_substeps(*args, stage=at_y)[2], pend_sim_substeps(*args, stage=at_x)[2]
    assert np.all(np.abs(ay - ax) > 1e-3)
