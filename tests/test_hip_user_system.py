"""Systems compiled at run time (rcg_register_system) on the GPU.

1. Sys3WRobot, re-registered from its own source under another name, against the built-in handle: every output bit for bit, and
   the same kernel / variant / envs per wave (the built-in's f32 hand-packed generated grid, GenPk, is written for that one
   system: there outputs only).  Runs in a child process that does not import torch - torch-ROCm bundles an older hipRTC under
   the same soname, and a process that has initialised torch may resolve the library's runtime compiler to it.
2. A pendulum against NumPy (right-hand side, RK4) and against the oracle with the pendulum patched in as a system of its
   own: _actor_cost on every decision kernel, the optimiser's per-iteration twin, a 50-step drop-in loop against the oracle loop.
3. A pendulum without jac_T: streamed decisions work, the optimiser is refused.
4. What is not compiled for such a system is refused with the handle untouched.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.test_user_system_register import PENDULUM  # noqa: E402

PEND_PARS = [1.3, 9.81, 0.7]


def _robot_source(name):
    src = open(os.path.join(ROOT, "rcognita_amd", "csrc", "rcg_systems.hpp")).read()
    i = src.index("struct Sys3WRobot {")
    j = src.index("\n};\n", i) + 4
    return src[i:j].replace("struct Sys3WRobot {", f"struct {name} {{")


def _robot_compare():
    """The child: built-in Sys3WRobot against its renamed copy; raises on the first difference."""
    from rcognita_amd import Engine, EngineConfig
    from rcognita_amd import _native as N

    info = N.register_system("UserRobot", _robot_source("UserRobot"), 5, 2, 2)
    print("hiprtc", info["hiprtc"], "register %.1f s" % info["seconds"])
    B, Nh = 4096, 10
    bnds = np.array([[-300.0, 300.0], [-100.0, 100.0]])
    rng = np.random.default_rng(3)
    x0 = np.stack([rng.uniform(-10, 10, B), rng.uniform(-10, 10, B), rng.uniform(-np.pi, np.pi, B),
                   rng.uniform(-1, 1, B), rng.uniform(-1, 1, B)], axis=-1)
    R1d = np.diag([1.0, 10.0, 1.0, 0, 0, 0, 0])
    R1f = R1d + 0.05 * np.ones((7, 7))
    checked = 0
    for dtype in ("f64", "f32"):
        for R1, gamma in ((R1d, 1.0), (R1d, 0.9), (R1f, 1.0)):
            def make(sid):
                e = Engine(EngineConfig(sys_id=sid, batch=B, dtype=dtype, Nactor=Nh, pars=[10.0, 1.0], ctrl_bnds=bnds, R1=R1,
                                        gamma=gamma, dt_sim=0.01, sampling_time=0.01, pred_step_size=0.02))
                e.set_state(x0)
                return e

            a, b = make(N.SYS_3WROBOT), make(info["sys_id"])

            def same(x, y, what, launch=True, kind=N.KERNEL_ACTOR):
                nonlocal checked
                for u, v in zip(x if isinstance(x, tuple) else (x,), y if isinstance(y, tuple) else (y,)):
                    assert np.array_equal(np.asarray(u), np.asarray(v)), (dtype, what)
                if launch:
                    la, lb = a.last_launch(kind), b.last_launch(kind)
                    assert la == lb, (dtype, what, la, lb)
                checked += 1

            u = rng.uniform(-50, 50, (B, 2)).astype(a.real)
            same(a.rhs(x0, u, clip=True), b.rhs(x0, u, clip=True), "rhs", launch=False)
            for nsub in (1, 3):
                a.sim_step(nsub)
                b.sim_step(nsub)
                same(a.get_state(), b.get_state(), f"sim {nsub}", kind=N.KERNEL_SIM)
            for K in (256, 16, 48):
                cand = (bnds[:, 0] + (bnds[:, 1] - bnds[:, 0]) * rng.random((B, K, Nh, 2))).astype(a.real)
                same(a.actor_argmin(cand), b.actor_argmin(cand), f"argmin K={K}")
                same(a.actor_cost(cand), b.actor_cost(cand), f"cost K={K}")
            for K in (256, 64):  # the generated grid (f32 diagonal gamma = 1: GenPk on the built-in, outputs only)
                pk = dtype == "f32" and R1 is R1d and gamma == 1.0
                same(a.actor_argmin(None, K=K), b.actor_argmin(None, K=K), f"grid K={K}", launch=not pk)
            cand = (bnds[:, 0] + (bnds[:, 1] - bnds[:, 0]) * rng.random((B, 256, Nh, 2))).astype(a.real)
            for _ in range(2):
                a.control_tick(cand)
                b.control_tick(cand)
            same(a.get_state(), b.get_state(), "control_tick")
            same(a.get_field(N.FIELD_BEST_IDX), b.get_field(N.FIELD_BEST_IDX), "control_tick idx")
            for mem in (0, 4):
                for iters in (5, 30):
                    a.set_optimizer(mem)
                    b.set_optimizer(mem)
                    same(a.actor_optimize(iters), b.actor_optimize(iters), f"opt mem={mem} iters={iters}")
            a.close()
            b.close()
    print("robot copy bit-identical:", checked, "comparisons")


def test_sys3wrobot_copy_is_bit_identical_to_the_builtin():
    env = {k: v for k, v in os.environ.items() if k != "PYTHONPATH"}
    code = "import sys; sys.path.insert(0, %r); import tests.test_hip_user_system as t; t._robot_compare(); " \
           "assert 'torch' not in sys.modules" % ROOT
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "bit-identical" in r.stdout


pytestmark = pytest.mark.gpu


def _pend_rhs(x, u, p):
    m, g, l = p
    return np.stack([x[:, 1], u[:, 0] / (m * l * l) - g / l * np.sin(x[:, 0])], axis=-1)


def _pendulum(name="PendulumG", src=PENDULUM):
    from rcognita_amd import _native as N

    return N.register_system(name, src.replace("PendulumT", name), 2, 1, 3)


def _pend_engine(sid, dtype, B=1024, Nh=10, **kw):
    from rcognita_amd import Engine, EngineConfig

    cfg = dict(sys_id=sid, batch=B, dtype=dtype, Nactor=Nh, pars=PEND_PARS, ctrl_bnds=np.array([[-5.0, 5.0]]),
               R1=np.diag([10.0, 1.0, 0.1]), dt_sim=0.01, sampling_time=0.01, pred_step_size=0.02)
    cfg.update(kw)
    return Engine(EngineConfig(**cfg))


@pytest.mark.parametrize("dtype,tol", [("f64", 1e-12), ("f32", 2e-5)])
def test_pendulum_rhs_and_rk4_against_numpy(dtype, tol):
    info = _pendulum()
    rng = np.random.default_rng(0)
    B = 1024
    x0 = np.stack([rng.uniform(-3, 3, B), rng.uniform(-2, 2, B)], axis=-1)
    u = rng.uniform(-8, 8, (B, 1))
    e = _pend_engine(info["sys_id"], dtype, B=B)
    d, ca = e.rhs(x0, u, clip=True)
    uc = np.clip(u, -5, 5)
    ref = _pend_rhs(x0.astype(e.real).astype(float), uc.astype(e.real).astype(float), PEND_PARS)
    assert np.allclose(ca, uc.astype(e.real))
    assert np.max(np.abs(d - ref) / np.maximum(np.abs(ref), 1.0)) <= tol
    # 200 RK4 steps under a constant torque
    from rcognita_amd import _native as N

    e.set_state(x0)
    e.set_field(N.FIELD_ACTION, np.full((B, 1), 1.5))
    x = x0.astype(e.real).astype(float)
    h = 0.01
    uu = np.full((B, 1), 1.5)
    for _ in range(200):
        e.sim_step(1)
        k1 = _pend_rhs(x, uu, PEND_PARS)
        k2 = _pend_rhs(x + h / 2 * k1, uu, PEND_PARS)
        k3 = _pend_rhs(x + h / 2 * k2, uu, PEND_PARS)
        k4 = _pend_rhs(x + h * k3, uu, PEND_PARS)
        x = x + h / 6 * (k1 + 2 * k2 + 2 * k3 + k4)
    st = e.get_state()
    assert np.max(np.abs(st - x) / np.maximum(np.abs(x), 1.0)) <= (1e-10 if dtype == "f64" else 2e-4)
    assert e.last_launch(N.KERNEL_SIM)["kernel"] == "k_sim"
    e.close()


@pytest.fixture
def pend_oracle(monkeypatch):
    """The oracle with the pendulum as one more system: its own NumPy `_state_dyn` and `(A^T lam, B^T lam)` patched into
    oracle.rcg_oracle for the registered id (nothing under oracle/ changes)."""
    from oracle import rcg_oracle as O

    sid = _pendulum()["sys_id"]
    dyn0, jac0 = O.state_dyn, O.state_jac_T

    def state_dyn(sys_id, state, action, pars):
        if sys_id != sid:
            return dyn0(sys_id, state, action, pars)
        x, u, p = (np.asarray(v, dtype=np.float64) for v in (state, action, pars))
        m, g, l = p[..., 0], p[..., 1], p[..., 2]
        shape = np.broadcast_shapes(x.shape[:-1], u.shape[:-1], p.shape[:-1])
        d = np.zeros(shape + (2,))
        d[..., 0] = x[..., 1]
        d[..., 1] = u[..., 0] / (m * l * l) - g / l * np.sin(x[..., 0])
        return d

    def state_jac_T(sys_id, x, u, pars, lam):
        if sys_id != sid:
            return jac0(sys_id, x, u, pars, lam)
        m, g, l = pars
        return np.array([-g / l * np.cos(x[0]) * lam[1], lam[0]]), np.array([lam[1] / (m * l * l)])

    monkeypatch.setattr(O, "state_dyn", state_dyn)
    monkeypatch.setattr(O, "state_jac_T", state_jac_T)
    monkeypatch.setitem(O.SYS_DIMS, sid, (2, 1, 3))
    return O, sid


def _pend_pair(O, sid, dtype, B, gamma=1.0, Nh=10, R1=None):
    R1 = np.diag([10.0, 1.0, 0.1]) if R1 is None else R1
    e = _pend_engine(sid, dtype, B=B, Nh=Nh, gamma=gamma, R1=R1)
    cfg = O.OracleCfg(sys_id=sid, n_actor=Nh, gamma=gamma, pred_step_size=0.02, dt_sim=0.01, sampling_time=0.01,
                      pars=PEND_PARS, ctrl_bnds=np.array([[-5.0, 5.0]]), R1=R1)
    return e, cfg


@pytest.mark.parametrize("dtype,tol", [("f64", 1e-11), ("f32", 1e-5)])
@pytest.mark.parametrize("gamma", [1.0, 0.9])
def test_pendulum_actor_cost_against_the_oracle(pend_oracle, dtype, tol, gamma):
    """_actor_cost of the user policy (the HW rollouts) on every decision kernel it reaches: k_actor_dma_packed (K = 16),
    k_actor_dma (K = 256; DMA_MPC_G1 / DMA_MPC by gamma), a full R1 (DMA_MPC_GENF) and the generated grid (k_actor)."""
    O, sid = pend_oracle
    from rcognita_amd import _native as N

    from tests.helpers import rel_err_norm

    rng = np.random.default_rng(5)
    B = 2048
    x = np.stack([rng.uniform(-3, 3, B), rng.uniform(-2, 2, B)], axis=-1)
    R1f = np.diag([10.0, 1.0, 0.1]) + 0.2 * np.ones((3, 3))
    for R1, Ks in ((None, (16, 256)), (R1f, (256,))):
        e, cfg = _pend_pair(O, sid, dtype, B, gamma=gamma, R1=R1)
        e.set_state(x)
        xr = x.astype(e.real).astype(np.float64)
        for K in Ks:
            cand = rng.uniform(-5, 5, (B, K, 10, 1)).astype(e.real)
            J = e.actor_cost(cand)
            ll = e.last_launch()
            J_or = O.actor_cost(cand.astype(np.float64), xr[:, None], xr[:, None], cfg)
            assert rel_err_norm(J, J_or) < tol, (K, ll)
            want = ("k_actor_dma_packed", N.DMA_MPC_G1 if gamma == 1.0 else N.DMA_MPC) if K == 16 else (
                "k_actor_dma", N.DMA_MPC_GENF if R1 is not None else (N.DMA_MPC_G1 if gamma == 1.0 else N.DMA_MPC))
            assert (ll["kernel"], ll["variant"]) == want, (K, ll)
        # the generated grid: K levels of the torque held over the horizon
        for K in (64, 256):
            act, bj, bi = e.actor_argmin(None, K=K)
            assert e.last_launch()["kernel"] == "k_actor"
            grid = O.grid_candidates(cfg, K)
            J_or = O.actor_cost(np.broadcast_to(grid[None], (B,) + grid.shape), xr[:, None], xr[:, None], cfg)
            assert rel_err_norm(bj, J_or.min(axis=1)) < tol
            if dtype == "f64":
                assert np.array_equal(bi, np.argmin(J_or, axis=1))
        e.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("memory", [0, 4])
def test_pendulum_optimizer_against_the_oracle_twin(pend_oracle, dtype, memory):
    """rcg_actor_optimize with the policy's jac_T against the oracle's per-iteration twin (tolerances of
    tests/test_hip_optimizer.py)."""
    O, sid = pend_oracle
    from tests.helpers import rel_err_norm

    rng = np.random.default_rng(6)
    B = 64
    x = np.stack([rng.uniform(-3, 3, B), rng.uniform(-2, 2, B)], axis=-1)
    e, cfg = _pend_pair(O, sid, dtype, B)
    e.set_state(x)
    e.set_optimizer(memory)
    act, U, J, its = e.actor_optimize(iters=10)
    assert np.all(U >= -5 - 1e-4) and np.all(U <= 5 + 1e-4)
    np.testing.assert_array_equal(act, U[:, 0, :])
    xr = x.astype(e.real).astype(np.float64)
    assert rel_err_norm(J, O.actor_cost(U.astype(np.float64), xr, xr, cfg)) < (1e-10 if dtype == "f64" else 1e-5)
    U_or, J_or, its_or = O.actor_optimize(cfg, xr, xr, O.action_sqn_init(cfg), iters=10, memory=memory)
    if dtype == "f64":
        assert np.all(np.abs(its - its_or) <= 3)
        assert rel_err_norm(J, J_or) < 1e-9 and rel_err_norm(U, U_or, floor=5.0) < 1e-5
    else:
        assert rel_err_norm(J, J_or) < 2e-4
    e.close()


def test_pendulum_drop_in_loop_against_the_oracle_loop(pend_oracle):
    """50 iterations of the reference's loop body (System subclass + Simulator + CtrlOptPred over a fixed candidate set) against
    the oracle's loop: its own RK4 of the state and its own argmin of _actor_cost."""
    O, sid = pend_oracle
    from rcognita_amd.controllers import CtrlOptPred
    from rcognita_amd.simulator import Simulator
    from rcognita_amd.systems import System

    from tests.helpers import rel_err_norm

    class Pendulum(System):
        hip_policy = PENDULUM.replace("PendulumT", "PendulumG")

    bnds = np.array([[-5.0, 5.0]])
    sys_ = Pendulum(sys_type="diff_eqn", dim_state=2, dim_input=1, dim_output=2, dim_disturb=0, pars=PEND_PARS, ctrl_bnds=bnds)
    assert Pendulum._sys_id == sid
    x0 = np.array([0.5, 0.0])
    N_, dt = 10, 0.05
    cand = np.random.default_rng(7).uniform(-5, 5, (64, N_))
    R1 = np.diag([10.0, 1.0, 0.0])
    ctrl = CtrlOptPred(1, 2, mode="MPC", ctrl_bnds=bnds, Nactor=N_, sampling_time=dt, pred_step_size=dt, sys_rhs=sys_._state_dyn,
                       sys_out=sys_.out, state_sys=x0, stage_obj_pars=[R1], candidates=cand)
    sim = Simulator(sys_type="diff_eqn", closed_loop_rhs=sys_.closed_loop_rhs, sys_out=sys_.out, state_init=x0, t0=0, t1=100,
                    dt=dt, max_step=dt / 10, first_step=1e-6, atol=1e-5, rtol=1e-3, is_disturb=0, is_dyn_ctrl=0)
    cfg = O.OracleCfg(sys_id=sid, n_actor=N_, pred_step_size=dt, dt_sim=dt, sampling_time=dt, pars=PEND_PARS, ctrl_bnds=bnds, R1=R1)
    x_or, u_or = x0.copy(), np.zeros(1)
    for k in range(50):
        sim.sim_step()
        t, x, y, _ = sim.get_sim_step_data()
        x_or = O.rk4_step(sid, x_or, u_or, cfg.pars, cfg.ctrl_bnds, dt)
        assert rel_err_norm(x, x_or) < 1e-9, k
        xs = np.array(ctrl.state_sys, dtype=float)  # the state the loop handed the controller (receive_sys_state)
        a = ctrl.compute_action(t, y)
        J_or = O.actor_cost(cand.reshape(-1, N_, 1), x_or[None], xs[None], cfg)
        u_or = cand[int(np.argmin(J_or)), :1].copy()
        np.testing.assert_allclose(a, u_or, rtol=0, atol=1e-12, err_msg=str(k))
        sys_.receive_action(a)
        ctrl.receive_sys_state(sys_._state)


def test_pendulum_without_jac():
    from rcognita_amd import _native as N
    from rcognita_amd.controllers import CtrlOptPred
    from rcognita_amd.systems import System

    src = PENDULUM[: PENDULUM.index("  template <typename real, bool HW = false>\n  __device__ __forceinline__ static void jac_T")]
    info = _pendulum("PendulumNJ", src + "};\n")
    assert not info["has_jac"]
    e = _pend_engine(info["sys_id"], "f32")
    e.set_state(np.zeros((1024, 2)) + 0.5)
    cand = np.random.default_rng(2).uniform(-5, 5, (1024, 64, 10, 1)).astype(np.float32)
    act, bj, bi = e.actor_argmin(cand)
    assert np.all(np.isfinite(bj))
    with pytest.raises(N.NativeError) as ei:
        e.actor_optimize(5)
    assert ei.value.code == N.ERR_UNSUPPORTED
    e.close()

    class PendulumNJ(System):
        hip_policy = src.replace("PendulumT", "PendulumNJ") + "};\n"

    s = PendulumNJ(sys_type="diff_eqn", dim_state=2, dim_input=1, dim_output=2, dim_disturb=0, pars=PEND_PARS,
                   ctrl_bnds=np.array([[-5.0, 5.0]]))
    with pytest.raises(NotImplementedError):
        CtrlOptPred(1, 2, mode="MPC", ctrl_bnds=np.array([[-5.0, 5.0]]), Nactor=10, sys_rhs=s._state_dyn, sys_out=s.out,
                    state_sys=np.zeros(2), stage_obj_pars=[np.diag([10.0, 1.0, 0.0])], actor_opt="auto")
    with pytest.raises(NotImplementedError):
        CtrlOptPred(1, 2, mode="RQL", ctrl_bnds=np.array([[-5.0, 5.0]]), Nactor=10, sys_rhs=s._state_dyn, sys_out=s.out,
                    state_sys=np.zeros(2), stage_obj_pars=[np.diag([10.0, 1.0, 0.0])], candidates=np.zeros((4, 10)))


def test_refusals_leave_the_handle_untouched():
    import ctypes as C

    from rcognita_amd import _native as N

    info = _pendulum()
    L = N.lib()
    for kw in (dict(mode="RQL", buffer_size=4), dict(mode="SQL", buffer_size=4)):
        with pytest.raises(N.NativeError) as ei:
            _pend_engine(info["sys_id"], "f64", **kw)
        assert ei.value.code == N.ERR_UNSUPPORTED
    with pytest.raises((N.NativeError, NotImplementedError)):
        _pend_engine(info["sys_id"], "f64", is_disturb=True, pars_disturb=[[0.1], [0.0], [1.0]])
    e = _pend_engine(info["sys_id"], "f64", B=256)
    x0 = np.random.default_rng(4).uniform(-1, 1, (256, 2))
    e.set_state(x0)
    h = e._h
    out = (C.c_double * (256 * 8))()
    act = (C.c_double * 256)()
    dev = e.empty((256, 1))
    calls = {
        "control_ticks": lambda: L.rcg_control_ticks(h, 2, 16),
        "actor_search": lambda: L.rcg_actor_search(h, 64, 2, None, None, None, None, None, None, None),
        "nominal_action": lambda: L.rcg_nominal_action(h, C.c_void_p(dev.ptr), C.c_void_p(dev.ptr), None, 256, 1.0, None, 0),
        "control_tick_nominal": lambda: L.rcg_control_tick_nominal(h, 1.0, None),
        "loop_step_begin": lambda: L.rcg_loop_step_begin(h, C.cast(act, C.c_void_p), 0.01, 1, N.LOOP_DECIDE, 5),
        "loop_step": lambda: L.rcg_loop_step(h, C.cast(act, C.c_void_p), 0.01, 1, 0, 5, C.cast(out, C.c_void_p)),
    }
    for what, call in calls.items():
        assert call() == N.ERR_UNSUPPORTED, what
        assert np.array_equal(e.get_state(), x0), what
        assert np.array_equal(e.get_field(N.FIELD_STEP_IDX), np.zeros(256, np.int32)), what
    e.close()
