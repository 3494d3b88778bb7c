"""Registered systems with an output map y = out(x) on the GPU (rcg.h: DY, out, out_jac_T).

1. Sys3WRobot re-registered with an identity `out` (DY = 5) against the built-in: every output bit for bit, the same kernel,
   variant and envs per wave (test_hip_user_system.py's comparison, in a child process without torch).
2. The pendulum with y = (sin th, cos th, om): _actor_cost on every decision kernel it reaches against the reference's results
   (tests/golden/F14_output_map_pendulum.npz) and their restatement (test_user_system_out_register.py).
3. Ticks: self-driven and REF_LAG, with and without the fused env step - y_0 = out(STATE).
4. The optimiser with out_jac_T against the reference's SLSQP; without out_jac_T it is refused.
5. The observation path: rcg_out, System.out, the Simulator, a drop-in loop.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.test_user_system_out_register import actor_cost_out, load_f14, pend_out, pendulum_out_source  # noqa: E402

pytestmark = pytest.mark.gpu

BND = np.array([[-5.0, 5.0]])


def _with_identity_out(src):
    """A policy's source with DY = 5 and an identity out / out_jac_T (Sys3WRobot's dimensions)."""
    members = r"""
  static constexpr int DY = 5;
  template <typename real, bool HW = false>
  __device__ __forceinline__ static void out(const Pre<real>&, const real* x, real* y) {
    for (int c = 0; c < 5; ++c) y[c] = x[c];
  }
  template <typename real, bool HW = false>
  __device__ __forceinline__ static void out_jac_T(const Pre<real>&, const real*, const real* gy, real* gx) {
    for (int c = 0; c < 5; ++c) gx[c] = gy[c];
  }
"""
    tail = src.rindex("};")
    return src[:tail] + members + src[tail:]


def test_identity_out_robot_is_bit_identical_to_the_builtin():
    env = {k: v for k, v in os.environ.items() if k != "PYTHONPATH"}
    code = ("import sys; sys.path.insert(0, %r); import tests.test_hip_user_system as t; "
            "import tests.test_hip_user_system_out as o; src = t._robot_source; "
            "t._robot_source = lambda name: o._with_identity_out(src(name)); "
            "from rcognita_amd import _native as N; "
            "i = N.register_system('UserRobot', t._robot_source('UserRobot'), 5, 2, 2); "
            "assert (i['dy'], i['has_out'], i['has_out_jac']) == (5, True, True), i; "
            "t._robot_compare(); assert 'torch' not in sys.modules" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "bit-identical" in r.stdout


def _pendulum_out(name="PendulumYG", **kw):
    from rcognita_amd import _native as N

    return N.register_system(name, pendulum_out_source(name, **kw), 2, 1, 3)


def _engine(sid, dtype, B, meta, R1, gamma=1.0, target=None, Nh=None, **kw):
    from rcognita_amd import Engine, EngineConfig

    return Engine(EngineConfig(sys_id=sid, batch=B, dtype=dtype, Nactor=meta["Nactor"] if Nh is None else Nh, pars=meta["pars"],
                               ctrl_bnds=BND, R1=R1, gamma=gamma, observation_target=target, dt_sim=0.01,
                               sampling_time=meta["sampling_time"], pred_step_size=meta["pred_step_size"], **kw))


def _restated(xs, ys, cand, R1, gamma, target, meta):
    """J [B, K] of the restatement for states xs [B, 2], observations ys [B, 3], candidates [B, K, N]."""
    B, K = cand.shape[:2]
    return np.array([[actor_cost_out(xs[b], ys[b], cand[b, k], R1, gamma, target, meta["pred_step_size"], meta["pars"])
                      for k in range(K)] for b in range(B)])


@pytest.mark.parametrize("dtype,tol", [("f64", 1e-11), ("f32", 1e-5)])
def test_actor_cost_with_out_against_the_reference(dtype, tol):
    """Every F14(a) case on k_actor_dma_packed (K = 16), k_actor_dma (K = 256: DMA_MPC_G1 / DMA_MPC by gamma, DMA_MPC_GENF with
    the full R1), the generated grid (k_actor) and the DIRECT long-row form (Nactor 70).  Candidate 0 of every env is the
    fixture's sequence: its J is the reference's own."""
    from rcognita_amd import _native as N

    from tests.helpers import rel_err_norm

    meta, z = load_f14()
    sid = _pendulum_out()["sys_id"]
    rng = np.random.default_rng(11)
    Nh = meta["Nactor"]
    for ci, case in enumerate(meta["cases"]):
        gamma, R1 = case["gamma"], z["a_R1"][ci]
        target = z["a_target"][ci] if case["cost"] == "target" else None
        xs, ys, seq = z["a_state_sys"][ci], z["a_obs"][ci], z["a_seq"][ci]
        B = len(xs)
        e = _engine(sid, dtype, B, meta, R1, gamma, target)
        real = e.real
        xr, yr = xs.astype(real).astype(float), ys.astype(real).astype(float)
        for K in (16, 256):
            cand = rng.uniform(-5, 5, (B, K, Nh)).astype(real)
            cand[:, 0] = seq.astype(real)
            J = e.actor_cost(cand.reshape(B, K, Nh, 1), obs=ys, state_sys=xs)
            ll = e.last_launch()
            assert rel_err_norm(J[:, 0], z["a_J"][ci]) < max(tol, 1e-11), (case, K, ll)
            assert rel_err_norm(J, _restated(xr, yr, cand.astype(float), R1, gamma, target, meta)) < tol, (case, K, ll)
            if case["cost"] == "target":
                continue  # (a diagonal cost with a target the system's preset does not have stays on k_actor)
            if K == 16 and case["cost"] == "full":  # (k_actor_dma_packed serves the diagonal stage cost only)
                assert ll["kernel"] == "k_actor", (case, K, ll)
                continue
            if K == 16:
                want = ("k_actor_dma_packed", N.DMA_MPC_G1 if gamma == 1.0 else N.DMA_MPC)
            else:
                want = ("k_actor_dma", N.DMA_MPC_GENF if case["cost"] == "full" else (N.DMA_MPC_G1 if gamma == 1.0 else N.DMA_MPC))
            assert (ll["kernel"], ll["variant"]) == want, (case, K, ll)
        # the generated grid: K levels of the torque held over the horizon
        act, bj, bi = e.actor_argmin(None, K=64, obs=ys, state_sys=xs)
        assert e.last_launch()["kernel"] == "k_actor"
        grid = np.linspace(-5, 5, 64)
        Jg = _restated(xr, yr, np.broadcast_to(grid[None, :, None], (B, 64, Nh)), R1, gamma, target, meta)
        assert rel_err_norm(bj, Jg.min(axis=1)) < tol, case
        e.close()
        if ci % 4 == 0:  # the DIRECT long-row form: rows of 70 reals, beyond RCG_MAX_ROW
            e = _engine(sid, dtype, B, meta, R1, gamma, target, Nh=70)
            cand = rng.uniform(-5, 5, (B, 8, 70)).astype(real)
            J = e.actor_cost(cand.reshape(B, 8, 70, 1), obs=ys, state_sys=xs)
            assert e.last_launch()["variant"] & 16, e.last_launch()
            assert rel_err_norm(J, _restated(xr, yr, cand.astype(float), R1, gamma, target, meta)) < tol, case
            e.close()


@pytest.mark.parametrize("K", [16, 256])
@pytest.mark.parametrize("ref_lag", [False, True])
def test_ticks_observe_out_of_the_state(K, ref_lag):
    """rcg_control_tick: the state equals rcg_sim_step's bits; best_J and the action are the restatement's at
    y_0 = out(STATE) (from state_sys = STATE, or STATE_PREV under REF_LAG); accum is the stage cost at out(STATE)."""
    from rcognita_amd import _native as N

    from tests.helpers import rel_err_norm

    meta, z = load_f14()
    sid = _pendulum_out()["sys_id"]
    R1 = z["a_R1"][0]
    B, Nh = 512, meta["Nactor"]
    rng = np.random.default_rng(12)
    x0 = np.stack([rng.uniform(-3, 3, B), rng.uniform(-2, 2, B)], axis=-1)
    a0 = rng.uniform(-5, 5, (B, 1))
    cand = rng.uniform(-5, 5, (B, K, Nh, 1))
    e = _engine(sid, "f64", B, meta, R1, ref_lag=ref_lag)
    s = _engine(sid, "f64", B, meta, R1, ref_lag=ref_lag)
    for h in (e, s):
        h.set_state(x0)
        h.set_field(N.FIELD_ACTION, a0)
    e.control_tick(cand)
    ll = e.last_launch()
    s.sim_step(e.cfg.substeps_per_tick)
    x1 = s.get_state()
    np.testing.assert_array_equal(e.get_state(), x1)
    if K == 16:
        assert ll["kernel"] == "k_actor_dma_packed" and ll["variant"] & 16, ll  # the fused env step
    else:
        assert ll["kernel"] == "k_actor_dma", ll
    xs = s.get_field(N.FIELD_STATE_PREV) if ref_lag else x1
    y1 = pend_out(x1)
    J = _restated(xs, y1, cand[..., 0], R1, 1.0, None, meta)
    bj = e.get_field(N.FIELD_BEST_J)
    assert rel_err_norm(bj, J.min(axis=1)) < 1e-11
    act = e.get_field(N.FIELD_ACTION)
    np.testing.assert_array_equal(act[:, 0], cand[np.arange(B), np.argmin(J, axis=1), 0, 0])
    chi = np.concatenate([y1, act], axis=-1)
    accum = np.einsum("bi,ij,bj->b", chi, R1, chi) * meta["sampling_time"]
    assert rel_err_norm(e.get_field(N.FIELD_ACCUM), accum) < 1e-12
    e.close()
    s.close()


@pytest.mark.parametrize("dtype,tol", [("f64", 0.0), ("f32", 2e-4)])
@pytest.mark.parametrize("memory", [0, 4])
def test_optimizer_with_out_jac_against_slsqp(dtype, tol, memory):
    """30 iterations of rcg_actor_optimize from the reference's start against F14(b)'s SLSQP optimum (the bar of
    tests/test_hip_optimizer.py); the reported J is the restated J of the returned sequence."""
    from tests.helpers import rel_err_norm

    meta, z = load_f14()
    sid = _pendulum_out()["sys_id"]
    x = z["b_state"]
    B = len(x)
    e = _engine(sid, dtype, B, meta, z["b_R1"])
    e.set_state(x)
    e.set_optimizer(memory)
    act, U, J, _ = e.actor_optimize(iters=30)
    assert e.last_launch()["kernel"] == "k_actor_opt"
    xr = x.astype(e.real).astype(float)
    Jr = np.array([actor_cost_out(xr[b], pend_out(xr[b]), U[b, :, 0].astype(float), z["b_R1"], 1.0, None, meta["pred_step_size"],
                                  meta["pars"]) for b in range(B)])
    assert rel_err_norm(J, Jr) < (1e-10 if dtype == "f64" else tol)
    bar = z["b_J_opt"] * (1 + 5e-3 + tol)  # (f32: the cost itself is evaluated to ~1e-6)
    assert np.all(J <= bar), (J - z["b_J_opt"]) / z["b_J_opt"]
    e.close()


def test_optimizer_without_out_jac_is_refused_and_streaming_works():
    from rcognita_amd import _native as N

    meta, z = load_f14()
    info = _pendulum_out("PendulumYNJ", out_jac=False)
    assert info["has_jac"] and not info["has_out_jac"]
    B = 256
    e = _engine(info["sys_id"], "f64", B, meta, z["a_R1"][0])
    x0 = np.random.default_rng(13).uniform(-1, 1, (B, 2))
    e.set_state(x0)
    with pytest.raises(N.NativeError) as ei:
        e.actor_optimize(5)
    assert ei.value.code == N.ERR_UNSUPPORTED and "out_jac_T" in str(ei.value)
    assert np.array_equal(e.get_state(), x0)
    assert np.array_equal(e.get_field(N.FIELD_STEP_IDX), np.zeros(B, np.int32))
    cand = np.random.default_rng(14).uniform(-5, 5, (B, 64, meta["Nactor"], 1))
    act, bj, bi = e.actor_argmin(cand)
    J = _restated(x0, pend_out(x0), cand[..., 0], z["a_R1"][0], 1.0, None, meta)
    np.testing.assert_allclose(bj, J.min(axis=1), rtol=1e-11)
    e.close()


def test_observation_path_and_drop_in_loop():
    """rcg_out / System.out / the Simulator's observation against NumPy, then 50 iterations of the reference's loop body
    (System subclass + Simulator + CtrlOptPred over a fixed candidate set) against a NumPy restatement of the decision."""
    from rcognita_amd.controllers import CtrlOptPred
    from rcognita_amd.simulator import Simulator
    from rcognita_amd.systems import System

    meta, z = load_f14()
    sid = _pendulum_out()["sys_id"]
    rng = np.random.default_rng(15)
    x = np.stack([rng.uniform(-7, 7, 1000), rng.uniform(-3, 3, 1000)], axis=-1)
    e = _engine(sid, "f64", 1000, meta, z["a_R1"][0])
    np.testing.assert_allclose(e.out(x), pend_out(x), rtol=0, atol=1e-15)
    np.testing.assert_allclose(e.out(x[:7]), pend_out(x[:7]), rtol=0, atol=1e-15)  # (n other than the batch)
    e.close()

    class PendulumOut(System):
        hip_policy = pendulum_out_source("PendulumYG")

    sys_ = PendulumOut(sys_type="diff_eqn", dim_state=2, dim_input=1, dim_output=3, dim_disturb=0, pars=meta["pars"],
                       ctrl_bnds=BND)
    assert PendulumOut._sys_id == sid
    np.testing.assert_allclose(sys_.out(x[0]), pend_out(x[0]), rtol=0, atol=1e-15)
    np.testing.assert_allclose(sys_.out(x), pend_out(x), rtol=0, atol=1e-15)
    x0 = np.array([2.5, 0.0])
    N_, dt = 10, 0.05
    cand = rng.uniform(-5, 5, (64, N_))
    R1 = np.diag([5.0, 5.0, 0.5, 0.1])
    target = np.array([0.0, 1.0, 0.0])
    ctrl = CtrlOptPred(1, 3, mode="MPC", ctrl_bnds=BND, Nactor=N_, sampling_time=dt, pred_step_size=dt, sys_rhs=sys_._state_dyn,
                       sys_out=sys_.out, state_sys=x0, stage_obj_pars=[R1], observation_target=target, candidates=cand)
    sim = Simulator(sys_type="diff_eqn", closed_loop_rhs=sys_.closed_loop_rhs, sys_out=sys_.out, state_init=x0, t0=0, t1=100,
                    dt=dt, max_step=dt / 10, first_step=1e-6, atol=1e-5, rtol=1e-3, is_disturb=0, is_dyn_ctrl=0)
    np.testing.assert_allclose(sim.observation, pend_out(x0), rtol=0, atol=1e-15)
    moved = False
    for k in range(50):
        sim.sim_step()
        t, xk, y, _ = sim.get_sim_step_data()
        np.testing.assert_allclose(y, pend_out(xk), rtol=0, atol=1e-15, err_msg=str(k))
        xs = np.array(ctrl.state_sys, dtype=float)  # the state the loop handed the controller (receive_sys_state)
        a = ctrl.compute_action(t, y)
        J = [actor_cost_out(xs, y, cand[i], R1, 1.0, target, dt, meta["pars"]) for i in range(len(cand))]
        np.testing.assert_allclose(a, cand[int(np.argmin(J)), :1], rtol=0, atol=1e-12, err_msg=str(k))
        moved = moved or abs(xk[0] - x0[0]) > 1e-3
        sys_.receive_action(a)
        ctrl.receive_sys_state(sys_._state)
    assert moved
    sim.reset()
    np.testing.assert_allclose(sim.observation, pend_out(x0), rtol=0, atol=1e-15)


@pytest.mark.parametrize("target", [None, np.array([0.0, 1.0, 0.0])])
def test_accum_every_substep_charges_the_stage_cost_at_out(target):
    """k_sim under RCG_FLAG_ACCUM_EVERY_SUBSTEP: accum += stage_obj(out(x_s), u) * sampling_time after every RK4 substep s
    (env_substeps); the states are the single substeps' bits."""
    from rcognita_amd import _native as N

    from tests.helpers import rel_err_norm

    meta, z = load_f14()
    sid = _pendulum_out()["sys_id"]
    R1 = z["a_R1"][2]  # the full matrix
    B, n_sub = 1000, 3
    rng = np.random.default_rng(16)
    x0 = np.stack([rng.uniform(-3, 3, B), rng.uniform(-2, 2, B)], axis=-1)
    a0 = rng.uniform(-7, 7, (B, 1))  # beyond the bounds: the held action is clipped first
    e = _engine(sid, "f64", B, meta, R1, target=target, accum_every_substep=True)
    s = _engine(sid, "f64", B, meta, R1, target=target)
    for h in (e, s):
        h.set_state(x0)
        h.set_field(N.FIELD_ACTION, a0)
    e.sim_step(n_sub)
    assert e.last_launch(N.KERNEL_SIM)["kernel"] == "k_sim"
    u = np.clip(a0, BND[0, 0], BND[0, 1])
    acc = np.zeros(B)
    for _ in range(n_sub):
        s.sim_step(1)
        y = pend_out(s.get_state())
        chi = np.concatenate([y if target is None else y - target, u], axis=-1)
        acc += np.einsum("bi,ij,bj->b", chi, R1, chi) * meta["sampling_time"]
    np.testing.assert_array_equal(e.get_state(), s.get_state())
    assert rel_err_norm(e.get_field(N.FIELD_ACCUM), acc) < 1e-12
    e.close()
    s.close()
