"""The disturbance model of systems compiled at run time (rcg.h: the policy members DD and `disturb`) on the GPU.

1. F16 (the reference's closed_loop_rhs on [state, disturb] of a pendulum subclass) through rcg_rhs_full, DD = 1 and 2.
2. Sys3WRobot and Sys3WRobotNI, re-registered from their own source with DD = 2, a `disturb` that restates Disturb<...>::apply and
   TICKS, against built-in handles with RCG_FLAG_DISTURB: every field as bits and equal launch records, in a child process that
   does not import torch.
3. The pendulum's env step against the NumPy restatement (test_user_system_disturb_register.py), noise from the oracle.
4. The stage cost of accum_every_substep under the disturbance model, charged at y = out(x) (DY = 3 != DS).
5. T ticks in one launch equal T single ticks, generated and streamed; RQL ticks per launch stay refused.
6. Shards reproduce their slice of the unsharded run.
7. An env whose disturbance overflows is frozen and flagged, the others step.
8. The mirror classes System(is_disturb=1) / Simulator(is_disturb=1) on a hip_policy.
9. Refusals.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.test_user_system_disturb_register import (load_f16, pend_rhs_full, pend_sim_substeps, pendulum_disturb_source,  # noqa: E402
                                                     with_disturb)
from tests.test_user_system_out_register import pend_out  # noqa: E402
from tests.test_user_system_register import PENDULUM  # noqa: E402
from tests.test_user_system_ticks_register import BND, PEND_PARS, pendulum_out_ticks_source, with_ticks  # noqa: E402

pytestmark = pytest.mark.gpu

FIELDS = ["FIELD_STATE", "FIELD_STATE_PREV", "FIELD_ACTION", "FIELD_ACCUM", "FIELD_STEP_IDX", "FIELD_STATUS", "FIELD_BEST_J",
          "FIELD_BEST_IDX", "FIELD_DISTURB", "FIELD_SUBSTEP_IDX"]
CRITIC_FIELDS = FIELDS + ["FIELD_W_CRITIC", "FIELD_W_PREV", "FIELD_OBS_BUF", "FIELD_ACT_BUF"]
AFTER_RESET = ["FIELD_RETURNS", "FIELD_EPISODE_IDX"]
SIGMA, MU, TAU = [2.0, 1.0], [0.5, -0.25], [1.5, 0.7]  # (test_hip_disturb.py's)
R1_PLAIN = np.diag([10.0, 1.0, 0.1])
R1_OUT = np.diag([5.0, 5.0, 0.5, 0.1])
DT = 0.01

_REG = {}


def _system(kind):
    """Each policy registered once per module: 'd1' (DD = 1, TICKS), 'd2' (DD = 2), 'out' (y = (sin th, cos th, om), CRITIC,
    TICKS, DD = 1) and 'plain' (the pendulum as test_user_system_register.py registers it: no disturbance model)."""
    from rcognita_amd import _native as N

    if kind not in _REG:
        name, src = {"d1": ("PendulumDK", pendulum_disturb_source("PendulumDK", ticks=True)),
                     "d2": ("PendulumD2", pendulum_disturb_source("PendulumD2", dd=2)),
                     "out": ("PendulumYDKC", with_disturb(pendulum_out_ticks_source("PendulumYDKC", critic=True))),
                     "plain": ("PendulumT", PENDULUM)}[kind]
        _REG[kind] = N.register_system(name, src, 2, 1, 3)
        assert _REG[kind]["dd"] == {"d1": 1, "d2": 2, "out": 1, "plain": 0}[kind]
    return _REG[kind]


def _engine(kind, dtype, B, Nh=6, **kw):
    from rcognita_amd import Engine, EngineConfig

    dd = _system(kind)["dd"]
    cfg = dict(sys_id=_system(kind)["sys_id"], batch=B, dtype=dtype, Nactor=Nh, pars=PEND_PARS, ctrl_bnds=BND,
               R1=R1_OUT if kind == "out" else R1_PLAIN, dt_sim=DT, sampling_time=0.02, pred_step_size=0.02, is_disturb=True,
               pars_disturb=[SIGMA[:dd], MU[:dd], TAU[:dd]], seed=5)
    cfg.update(kw)
    return Engine(EngineConfig(**cfg))


def _states(rng, B):
    return np.stack([rng.uniform(-3, 3, B), rng.uniform(-2, 2, B)], axis=-1)


def _same(a, b, fields, what):
    from rcognita_amd import _native as N

    for f in fields:
        u, v = a.get_field(getattr(N, f)), b.get_field(getattr(N, f))
        assert u.dtype == v.dtype and u.shape == v.shape and u.tobytes() == v.tobytes(), (what, f, int(np.sum(u != v)))


def _snapshot(e, fields):
    from rcognita_amd import _native as N

    return {f: e.get_field(getattr(N, f)).copy() for f in fields}, N.lib().rcg_tick_count(e._h)


def _unchanged(e, snap, what):
    from rcognita_amd import _native as N

    for f, v in snap[0].items():
        assert e.get_field(getattr(N, f)).tobytes() == v.tobytes(), (what, f)
    assert N.lib().rcg_tick_count(e._h) == snap[1], what


# ---- 1. F16 through rcg_rhs_full -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("dd", [1, 2])
def test_F16_rhs_full_matches_reference(dd, dtype):
    """closed_loop_rhs on [state, disturb] with the reference's own noise values: HIP == reference (the tolerances of
    test_hip_disturb.py::test_F11_rhs_full_matches_reference)."""
    from rcognita_amd import _native as N
    from tests.helpers import rel_err_norm

    _, z = load_f16()
    p = f"dd{dd}_"
    kind = "d1" if dd == 1 else "d2"
    n = z[p + "state"].shape[0]
    eng = _engine(kind, dtype, n, pars_disturb=[z[p + "sigma"], z[p + "mu"], z[p + "tau"]])
    dx, dq, a = eng.rhs_full(z[p + "state"], z[p + "disturb"], z[p + "action"], z[p + "xi"], clip=True)
    assert dx.shape == (n, 2) and dq.shape == (n, dd)
    tol = 1e-12 if dtype == "f64" else 1e-5
    e1, e2 = rel_err_norm(dx, z[p + "rhs_full"][:, :2]), rel_err_norm(dq, z[p + "rhs_full"][:, 2:], floor=1.0)
    print(f"F16 dd={dd} {dtype}: state rows {e1:.3e}, disturbance rows {e2:.3e}")
    assert e1 < tol
    assert e2 < tol
    np.testing.assert_allclose(a, z[p + "action_clipped"], rtol=1e-7 if dtype == "f32" else 0)
    programs = [(f, e) for f, e in N.system_programs(_system(kind)["sys_id"]) if "_disturb.hip" in f]
    real = "double" if dtype == "f64" else "float"
    assert (_system(kind)["name"] + "_disturb.hip", f"rcg::k_rhs_full<rcg::RcgRtcSys, {real}>") in programs, programs
    eng.close()


# ---- 2. copies of two built-in systems ---------------------------------------------------------------------------------------
_APPLY = {
    "Sys3WRobot": "    d[3] = q.inv_m * (u[0] + w[0]);\n    d[4] = q.inv_I * (u[1] + w[1]);\n",
    "Sys3WRobotNI": "    d[0] += w[0];\n    d[1] += w[0];\n    d[2] += w[1];\n",
}


def _copy_source(struct, name):
    """The built-in system's own source under another name, with DD = 2, a `disturb` that restates Disturb<struct>::apply, and
    TICKS."""
    src = open(os.path.join(ROOT, "rcognita_amd", "csrc", "rcg_systems.hpp")).read()
    i = src.index(f"struct {struct} {{")
    j = src.index("\n};\n", i) + 4
    body = ("\n  template <typename real>\n"
            "  __device__ __forceinline__ static void disturb(const Pre<real>& q, const real* x, const real* u, const real* w,\n"
            "                                                 real* d) {\n" + _APPLY[struct] + "  }\n")
    return with_ticks(with_disturb(src[i:j].replace(f"struct {struct} {{", f"struct {name} {{"), dd=2, body=body))


def _copies_compare():
    """The child: built-in Sys3WRobot / Sys3WRobotNI with RCG_FLAG_DISTURB against their renamed copies; raises on the first
    difference."""
    from rcognita_amd import Engine
    from rcognita_amd import _native as N

    from tests.helpers import engine_cfg, rand_actions, rand_states

    copies = {"3wrobot": N.register_system("UserRobotD", _copy_source("Sys3WRobot", "UserRobotD"), 5, 2, 2),
              "3wrobotNI": N.register_system("UserRobotNID", _copy_source("Sys3WRobotNI", "UserRobotNID"), 3, 2, 0)}
    assert all(i["dd"] == 2 and i["has_ticks"] and not i["has_out"] for i in copies.values())
    B, K, Nh = 300, 64, 6  # a ragged last block and wave
    fields = [getattr(N, f) for f in FIELDS]
    checked = 0
    for name, info in copies.items():
        ds = N.SYS_DIMS[N.SYS_IDS[name]][0]
        for dtype in ("f32", "f64"):
            tag = (name, dtype)
            rng = np.random.default_rng(300 + ds)

            def make(sid):
                c = engine_cfg(name, B, dtype, n_actor=Nh, substeps_per_tick=2)
                c.sys_id = sid
                c.is_disturb, c.pars_disturb, c.seed, c.env_id_base, c.disturb_init = True, [SIGMA, MU, TAU], 5, 1000, [0.3, -0.2]
                return Engine(c)

            a, b = make(N.SYS_IDS[name]), make(info["sys_id"])

            def same(what, extra=()):
                nonlocal checked
                for f in fields + [getattr(N, x) for x in extra]:
                    u, v = a.get_field(f), b.get_field(f)
                    assert u.dtype == v.dtype and u.shape == v.shape and u.tobytes() == v.tobytes(), (tag, what, f)
                for kind in (N.KERNEL_SIM, N.KERNEL_ACTOR):
                    assert a.last_launch(kind) == b.last_launch(kind), (tag, what, a.last_launch(kind), b.last_launch(kind))
                checked += 1

            x0 = rand_states(rng, name, B)
            u0 = rand_actions(rng, name, (B,), overshoot=1.5)  # a third of them beyond the bounds: clipped
            for e in (a, b):
                e.set_state(x0)
                e.set_field(N.FIELD_ACTION, u0)
                e.sim_step(3)
            same("rcg_sim_step")
            assert a.last_launch(N.KERNEL_SIM)["kernel"] == "k_sim_dist", a.last_launch(N.KERNEL_SIM)
            assert np.all(a.get_field(N.FIELD_SUBSTEP_IDX) == 3) and np.std(a.get_field(N.FIELD_DISTURB)) > 0
            xs, q = rand_states(rng, name, B), rng.normal(0.0, 5.0, (B, 2))
            us, xi = rand_actions(rng, name, (B,), overshoot=1.5), rng.standard_normal((B, 2))
            ra, rb = a.rhs_full(xs, q, us, xi, clip=True), b.rhs_full(xs, q, us, xi, clip=True)
            for u, v in zip(ra, rb):
                assert u.dtype == v.dtype and u.tobytes() == v.tobytes(), (tag, "rcg_rhs_full")
            for _ in range(5):
                a.control_tick(None, K=K)
                b.control_tick(None, K=K)
            same("single ticks")
            assert a.last_launch(N.KERNEL_SIM)["kernel"] == "k_sim_dist" and a.last_launch(N.KERNEL_ACTOR)["kernel"] != "k_ticks"
            a.control_ticks(7, K)
            b.control_ticks(7, K)
            same("rcg_control_ticks")
            assert a.last_launch(N.KERNEL_ACTOR)["kernel"] == "k_ticks", a.last_launch(N.KERNEL_ACTOR)
            assert np.all(a.get_field(N.FIELD_SUBSTEP_IDX) == 3 + 12 * 2)
            for e in (a, b):
                e.episode_reset()
                e.control_tick(None, K=K)
            same("after an episode reset", AFTER_RESET)
            assert np.all(b.get_field(N.FIELD_SUBSTEP_IDX) == 2) and np.all(b.get_field(N.FIELD_EPISODE_IDX) == 1)
            assert N.lib().rcg_tick_count(a._h) == N.lib().rcg_tick_count(b._h)
            a.close()
            b.close()
    print("copies bit-identical:", checked, "comparisons")


def test_copies_with_disturb_are_bit_identical_to_the_builtins():
    env = {k: v for k, v in os.environ.items() if k != "PYTHONPATH"}
    code = "import sys; sys.path.insert(0, %r); import tests.test_hip_user_system_disturb as t; t._copies_compare(); " \
           "assert 'torch' not in sys.modules" % ROOT
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=1200)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "bit-identical: 16 comparisons" in r.stdout


# ---- 3. the pendulum against the restatement -----------------------------------------------------------------------------------
def test_sim_step_with_disturbance_vs_restatement():
    """The shape and bounds of test_hip_disturb.py::test_sim_step_with_disturbance_vs_oracle."""
    from rcognita_amd import _native as N
    from tests.helpers import rel_err_norm

    rng = np.random.default_rng(3)
    B, T, S = 41, 9, 2
    eng = _engine("d1", "f64", B, env_id_base=1000, disturb_init=[0.3])
    x = _states(rng, B)
    q, sub, ep = np.full((B, 1), 0.3), np.zeros(B, np.int32), np.zeros(B, np.int32)
    eng.set_state(x)
    for t in range(T):
        u = rng.uniform(-1, 1, (B, 1)) * BND[0, 1] * 1.3  # some beyond the bounds: clipped
        eng.set_field(N.FIELD_ACTION, u)
        eng.sim_step(S)
        x, q, _, sub = pend_sim_substeps(x, q, u, sub, ep, S, DT, SIGMA[:1], MU[:1], TAU[:1], seed=5, env_id_base=1000)
        ex, eq = rel_err_norm(eng.get_state(), x), rel_err_norm(eng.get_field(N.FIELD_DISTURB), q, floor=1.0)
        print(f"step {t}: state {ex:.3e}, disturbance {eq:.3e}")
        assert ex < 1e-10, t
        assert eq < 1e-10, t
        np.testing.assert_array_equal(eng.get_field(N.FIELD_SUBSTEP_IDX), sub)
    assert eng.last_launch(N.KERNEL_SIM)["kernel"] == "k_sim_dist"
    assert np.std(eng.get_field(N.FIELD_DISTURB)) > 0.05
    eng.close()


# ---- 4. output map + accum_every_substep + disturbance -------------------------------------------------------------------------
def test_accum_every_substep_is_charged_at_out_of_x():
    """DY = 3 != DS = 2: env_substeps_dist forms chi = [out(x), u] (an instance that charged at x would not compile)."""
    from rcognita_amd import _native as N
    from tests.helpers import rel_err_norm

    rng = np.random.default_rng(4)
    B, T, S = 41, 4, 2
    eng = _engine("out", "f64", B, accum_every_substep=True, env_id_base=7)
    x = _states(rng, B)
    q, sub, ep, acc = np.zeros((B, 1)), np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B)
    w = np.diag(R1_OUT)

    def stage(xx, a):
        chi = np.concatenate([pend_out(xx), a], axis=-1)
        return np.einsum("bi,i,bi->b", chi, w, chi) * 0.02  # stage cost x sampling_time (controllers.py:1093)

    eng.set_state(x)
    for _ in range(T):
        u = rng.uniform(-1, 1, (B, 1)) * BND[0, 1] * 1.3
        eng.set_field(N.FIELD_ACTION, u)
        eng.sim_step(S)
        x, q, da, sub = pend_sim_substeps(x, q, u, sub, ep, S, DT, SIGMA[:1], MU[:1], TAU[:1], seed=5, env_id_base=7, stage=stage)
        acc = acc + da
    err = rel_err_norm(eng.get_field(N.FIELD_ACCUM), acc)
    print(f"accum at out(x): {err:.3e}")
    assert np.all(acc > 0) and err < 1e-10
    assert rel_err_norm(eng.get_state(), x) < 1e-10
    eng.close()


# ---- 5. T ticks in one launch ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("what,K,B", [("generated", 64, 130), ("streamed", 16, 77)])
def test_T_ticks_in_one_launch_equal_T_single_ticks(what, K, B, dtype):
    from rcognita_amd import _native as N
    from tests.helpers import assert_kernel

    T, Nh = 7, 6
    rng = np.random.default_rng(K + B)
    one, many = (_engine("d1", dtype, B, Nh, disturb_init=[0.3], env_id_base=64) for _ in range(2))
    x0 = _states(rng, B)
    ca = cb = None
    if what == "streamed":
        c = rng.uniform(BND[0, 0], BND[0, 1], (B, K, Nh, 1)).astype(one.real)
        ca, cb = one.to_device(c), many.to_device(c)
    for e in (one, many):
        e.set_state(x0)

    def run(n):
        for _ in range(n):
            one.control_tick(ca, K=K)
        if ca is None:
            many.control_ticks(n, K)
        else:
            many.control_tick(cb, K=K, T=n)

    run(T)
    ll = assert_kernel(many, "k_ticks")
    assert ll["variant"] == (4 if what == "streamed" else 0), ll
    assert one.last_launch(N.KERNEL_ACTOR)["kernel"] != "k_ticks"
    assert_kernel(one, "k_sim_dist", kind=N.KERNEL_SIM)
    _same(many, one, FIELDS, what)
    assert N.lib().rcg_tick_count(many._h) == N.lib().rcg_tick_count(one._h) == T
    np.testing.assert_array_equal(many.get_field(N.FIELD_SUBSTEP_IDX), np.full(B, T, np.int32))
    assert np.std(many.get_field(N.FIELD_DISTURB)) > 0 and np.any(many.get_state() != x0.astype(many.real))
    run(3)
    for e in (one, many):
        e.episode_reset()
    run(2)
    _same(many, one, FIELDS + AFTER_RESET, what + ", continued")
    one.close()
    many.close()


def test_rql_ticks_per_launch_stay_refused_under_the_disturbance_model():
    from rcognita_amd import _native as N

    B, K = 64, 16
    e = _engine("out", "f32", B, 5, mode="RQL", critic_struct="quad-nomix", Ncritic=4, buffer_size=6)
    e.set_state(_states(np.random.default_rng(9), B))
    e.control_tick(None, K=K)  # (single RQL ticks run: k_sim_dist, then push + fit, then the decision)
    assert e.last_launch(N.KERNEL_SIM)["kernel"] == "k_sim_dist"
    snap = _snapshot(e, CRITIC_FIELDS)
    assert N.lib().rcg_control_ticks(e._h, 3, K) == N.ERR_UNSUPPORTED
    assert "disturbance" in N.last_error(e._h)
    _unchanged(e, snap, "RQL control_ticks")
    e.control_tick(None, K=K, T=2)  # rcg_control_tick_n: the loop of single ticks
    assert N.lib().rcg_tick_count(e._h) == 3 and e.last_launch(N.KERNEL_ACTOR)["kernel"] != "k_ticks"
    e.close()


# ---- 6. shards -----------------------------------------------------------------------------------------------------------------
def test_shards_reproduce_their_slice_of_the_unsharded_run():
    from rcognita_amd import _native as N

    x0 = _states(np.random.default_rng(8), 64)
    full = _engine("d1", "f32", 64, seed=99)
    lo = _engine("d1", "f32", 32, seed=99, env_id_base=0)
    hi = _engine("d1", "f32", 32, seed=99, env_id_base=32)
    other = _engine("d1", "f32", 32, seed=100)
    for e, xs in ((full, x0), (lo, x0[:32]), (hi, x0[32:]), (other, x0[:32])):
        e.set_state(xs)
        for _ in range(20):
            e.control_tick(None, K=64)
    for f in (N.FIELD_STATE, N.FIELD_DISTURB, N.FIELD_ACTION, N.FIELD_ACCUM, N.FIELD_SUBSTEP_IDX):
        np.testing.assert_array_equal(full.get_field(f), np.concatenate([lo.get_field(f), hi.get_field(f)]))
    assert not np.array_equal(other.get_field(N.FIELD_DISTURB), lo.get_field(N.FIELD_DISTURB))
    for e in (full, lo, hi, other):
        e.close()


# ---- 7. freeze -----------------------------------------------------------------------------------------------------------------
def test_an_overflowing_disturbance_freezes_its_env_only():
    from rcognita_amd import _native as N
    from tests.helpers import rel_err_norm

    B, S = 64, 2
    rng = np.random.default_rng(2)
    eng = _engine("d1", "f64", B, pars_disturb=[[2.0], [0.5], [10.0]])
    x0, u = _states(rng, B), rng.uniform(-4, 4, (B, 1))
    q0 = rng.normal(0.0, 1.0, (B, 1))
    q0[7, 0] = 1e308  # tau (q + ...) = 1e309: the slope overflows in the first stage
    eng.set_state(x0)
    eng.set_field(N.FIELD_ACTION, u)
    eng.set_field(N.FIELD_DISTURB, q0)
    eng.sim_step(S)
    ok = np.arange(B) != 7
    st = eng.get_field(N.FIELD_STATUS)
    assert st[7] == 1 and not st[ok].any()
    np.testing.assert_array_equal(eng.get_state()[7], x0[7])
    np.testing.assert_array_equal(eng.get_field(N.FIELD_DISTURB)[7], q0[7])
    sub = eng.get_field(N.FIELD_SUBSTEP_IDX)
    assert sub[7] == 0 and np.all(sub[ok] == S)
    with np.errstate(over="ignore", invalid="ignore"):
        x, q, _, _ = pend_sim_substeps(x0, q0, u, np.zeros(B, np.int32), np.zeros(B, np.int32), S, DT, [2.0], [0.5], [10.0], seed=5)
    assert rel_err_norm(eng.get_state()[ok], x[ok]) < 1e-10
    assert rel_err_norm(eng.get_field(N.FIELD_DISTURB)[ok], q[ok], floor=1.0) < 1e-10
    eng.close()


# ---- 8. mirror classes -----------------------------------------------------------------------------------------------------------
def test_mirror_system_and_simulator_with_is_disturb():
    from rcognita_amd.simulator import Simulator
    from rcognita_amd.systems import System

    class PendulumMirror(System):
        hip_policy = pendulum_disturb_source("PendulumDK", ticks=True)  # (the source _system('d1') registers: the same id)

    sig, mu, tau = [2.0], [0.5], [1.5]

    def make(is_disturb, seed=3):
        s = PendulumMirror(sys_type="diff_eqn", dim_state=2, dim_input=1, dim_output=2, dim_disturb=1, pars=PEND_PARS,
                           ctrl_bnds=BND, is_dyn_ctrl=0, is_disturb=is_disturb, pars_disturb=[sig, mu, tau] if is_disturb else [],
                           seed=seed)
        sim = Simulator(sys_type="diff_eqn", closed_loop_rhs=s.closed_loop_rhs, sys_out=s.out, state_init=np.array([0.5, 0.0]),
                        disturb_init=np.array([0.5]) if is_disturb else [], action_init=np.zeros(1), t0=0, t1=1.0, dt=0.01,
                        max_step=0.005, first_step=1e-6, atol=1e-5, rtol=1e-3, is_disturb=is_disturb, is_dyn_ctrl=0)
        return s, sim

    s, sim = make(1)
    assert PendulumMirror._sys_id == _system("d1")["sys_id"] and s._dim_full_state == 3
    x, u, w, xi = np.array([0.7, -0.4]), np.array([1.5]), np.array([0.8]), np.array([-0.3])
    np.testing.assert_allclose(s._disturb_dyn(0, w, xi=xi), -tau[0] * (w + sig[0] * (xi + mu[0])), rtol=1e-12)
    dx, dq = pend_rhs_full(x, w, u, xi, sig, mu, tau)
    np.testing.assert_allclose(s._state_dyn(0, x, u, w), dx, rtol=1e-12, atol=1e-12)
    undisturbed = pend_rhs_full(x, np.zeros(1), u, xi, sig, mu, tau)[0]
    np.testing.assert_allclose(s._state_dyn(0, x, u), undisturbed, rtol=1e-12, atol=1e-12)
    assert abs(dx[1] - undisturbed[1]) > 0.1
    s.receive_action(np.array([9.0]))  # beyond the bounds: clipped to 5
    r1 = s.closed_loop_rhs(0.0, np.concatenate([x, w]))
    assert r1.shape == (3,) and s.action[0] == 5.0
    np.testing.assert_allclose(r1[:2], pend_rhs_full(x, w, np.array([5.0]), xi, sig, mu, tau)[0], rtol=1e-12, atol=1e-12)
    assert not np.array_equal(r1[2:], s.closed_loop_rhs(0.0, np.concatenate([x, w]))[2:])  # a fresh draw per call

    np.testing.assert_array_equal(sim.state_full_init, [0.5, 0.0, 0.5])
    (s2, sim2), (s0, sim0) = make(1), make(0)
    for obj in (s, s2, s0):
        obj.receive_action(np.array([2.0]))
    for _ in range(30):
        for m in (sim, sim2, sim0):
            m.sim_step()
    t, state, obs, full = sim.get_sim_step_data()
    assert abs(t - 0.30) < 1e-12 and state.shape == (2,) and obs.shape == (2,) and full.shape == (3,)
    np.testing.assert_array_equal(full[:2], state)
    assert full[2] != 0.5
    np.testing.assert_array_equal(sim2.get_sim_step_data()[3], full)  # the same seed: the same trajectory
    _, state0, _, full0 = sim0.get_sim_step_data()
    assert full0.shape == (2,) and np.all(np.abs(state0 - state) > 1e-6)
    with pytest.raises(ValueError):
        Simulator(sys_type="diff_eqn", closed_loop_rhs=s.closed_loop_rhs, sys_out=s.out, state_init=np.array([0.5, 0.0]), is_disturb=0)


# ---- 9. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals():
    import ctypes as C

    from rcognita_amd import EngineConfig
    from rcognita_amd import _native as N

    L = N.lib()
    # RCG_FLAG_DISTURB on a policy without `disturb`: refused at rcg_create
    c = EngineConfig(sys_id=_system("plain")["sys_id"], batch=8, dtype="f64", Nactor=5, pars=PEND_PARS, ctrl_bnds=BND,
                     R1=R1_PLAIN).to_native()
    c.flags |= N.FLAG_DISTURB
    h = C.c_void_p()
    assert L.rcg_create(C.byref(c), C.byref(h)) == N.ERR_UNSUPPORTED and not h.value
    assert "disturb" in N.last_error(None)
    with pytest.raises(NotImplementedError, match="disturb"):
        _engine("plain", "f64", 8, pars_disturb=[[1.0], [0.0], [1.0]])

    # rcg_loop_step and the nominal controller on a disturbed registered handle
    B = 8
    e = _engine("d1", "f64", B, 5)
    e.set_state(_states(np.random.default_rng(1), B))
    e.control_tick(None, K=16)
    snap = _snapshot(e, FIELDS)
    out = (C.c_double * (B * 16))()
    act = (C.c_double * B)()
    assert L.rcg_loop_step(e._h, C.cast(act, C.c_void_p), 0.01, 1, 0, 5, C.cast(out, C.c_void_p)) == N.ERR_UNSUPPORTED
    assert L.rcg_loop_step_begin(e._h, C.cast(act, C.c_void_p), 0.01, 1, N.LOOP_DECIDE, 5) == N.ERR_UNSUPPORTED
    assert L.rcg_control_tick_nominal(e._h, 1.0, None) == N.ERR_UNSUPPORTED
    buf = e.empty((2, B))
    assert L.rcg_nominal_action(e._h, C.c_void_p(buf.ptr), C.c_void_p(buf.ptr), None, B, 1.0, None, 1) == N.ERR_UNSUPPORTED
    _unchanged(e, snap, "rcg_loop_step / nominal")
    e.close()
