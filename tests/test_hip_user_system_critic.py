"""RQL / SQL on systems compiled at run time (rcg.h: the policy member CRITIC) on the GPU.

1. Sys3WRobot and Sys2Tank, re-registered from their own source with CRITIC under other names, against the built-in handles in
   RQL and SQL x the four critic structures x f32 / f64: operator J, argmin, action, rcg_critic, rcg_critic_cost and six
   closed-loop ticks with the fit in between - every output, W_CRITIC, W_PREV and both buffers bit for bit, and the same kernel,
   variant and envs per wave (rcg_last_launch) - on k_actor_dma (K = 256), k_actor_dma_packed or its fall-through (K = 16),
   k_actor (K = 6) and the three fit forms (Ncritic - 1 = 3, 6, 11).  In a child process that does not import torch, as
   test_hip_user_system.py does.
2. The pendulum with y = (sin th, cos th, om) - DY = 3, DS = 2 - against the reference's results
   (tests/golden/F15_user_system_critic.npz) and their restatement (test_user_system_critic_register.py): every quantity through
   the C ABI, closed-loop ticks through oracle/parity.py::check_tick, the fit's objective, the optimiser in RQL.
3. CtrlOptPred(mode="RQL") as a drop-in loop.
4. What stays refused on a CRITIC policy, with the handle untouched.
"""
import os
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.test_user_system_critic_register import (STRUCTS, actor_cost_critic, load_f15, pendulum_critic_source,  # noqa: E402
                                                    with_critic)
from tests.test_user_system_out_register import pend_out  # noqa: E402

BND = np.array([[-5.0, 5.0]])
TOL = {"f64": 1e-11, "f32": 1e-5}  # the project's operator tolerances (tests/helpers.py)


# ---- 1. copies of two built-in systems ---------------------------------------------------------------------------------------
def _copy_source(struct, name):
    src = open(os.path.join(ROOT, "rcognita_amd", "csrc", "rcg_systems.hpp")).read()
    i = src.index(f"struct {struct} {{")
    j = src.index("\n};\n", i) + 4
    return with_critic(src[i:j].replace(f"struct {struct} {{", f"struct {name} {{"))


def _copies_compare():
    """The child: built-in Sys3WRobot / Sys2Tank against their renamed copies with CRITIC; raises on the first difference."""
    from oracle import rcg_oracle as O
    from rcognita_amd import Engine
    from rcognita_amd import _native as N

    from tests.helpers import engine_cfg, rand_actions, rand_states

    copies = {"3wrobot": N.register_system("UserRobotC", _copy_source("Sys3WRobot", "UserRobotC"), 5, 2, 2),
              "2tank": N.register_system("UserTankC", _copy_source("Sys2Tank", "UserTankC"), 2, 1, 5)}
    assert all(i["has_critic"] and not i["has_out"] for i in copies.values())
    B, Nh, BS = 2048 + 64, 10, 14
    fields = (N.FIELD_STATE, N.FIELD_STATE_PREV, N.FIELD_ACTION, N.FIELD_BEST_J, N.FIELD_BEST_IDX, N.FIELD_ACCUM, N.FIELD_STEP_IDX,
              N.FIELD_W_CRITIC, N.FIELD_W_PREV, N.FIELD_OBS_BUF, N.FIELD_ACT_BUF)
    checked, kernels = 0, set()
    for name, info in copies.items():
        for dtype in ("f64", "f32"):
            for mode in (O.MODE_RQL, O.MODE_SQL):
                for cs in range(4):
                    rng = np.random.default_rng(100 * mode + 10 * cs + len(name))
                    tag = (name, dtype, mode, cs)

                    def make(sid, n_critic):
                        c = engine_cfg(name, B, dtype, n_actor=Nh, mode=mode, critic_struct=cs, gamma=0.95, n_critic=n_critic,
                                       buffer_size=BS)
                        c.sys_id = sid
                        return Engine(c)

                    def same(a, b, x, y, what, kinds=(N.KERNEL_ACTOR,)):
                        nonlocal checked
                        for u, v in zip(x if isinstance(x, tuple) else (x,), y if isinstance(y, tuple) else (y,)):
                            u, v = np.asarray(u), np.asarray(v)
                            assert u.dtype == v.dtype and u.shape == v.shape and u.tobytes() == v.tobytes(), (tag, what)
                        for kind in kinds:
                            la, lb = a.last_launch(kind), b.last_launch(kind)
                            assert la == lb, (tag, what, la, lb)
                            kernels.add((la["kernel"], la["variant"] & 2048 and "gen" or (la["variant"] & 1024 and "ml") or ""))
                        checked += 1

                    x0 = rand_states(rng, name, B)
                    # (Ncritic - 1, K of the closed loop): every fit form and every decision kernel
                    for n_critic, Kt in ((4, 256), (7, 16), (12, 6)):
                        a, b = make(N.SYS_IDS[name], n_critic), make(info["sys_id"], n_critic)
                        dc = a.dc
                        assert b.dc == dc
                        lo, hi = O.critic_bounds(cs, dc)
                        w = rng.uniform(np.maximum(lo, -2.0), np.minimum(hi, 2.0), (B, dc)).astype(a.real)
                        for e in (a, b):
                            e.set_state(x0)
                            e.set_field(N.FIELD_W_CRITIC, w)
                            e.set_field(N.FIELD_W_PREV, w[::-1].copy())
                        if n_critic == 4:  # the operators, on every decision kernel
                            for K in (256, 16, 6):
                                cand = rand_actions(rng, name, (B, K, Nh)).astype(a.real)
                                same(a, b, a.actor_cost(cand), b.actor_cost(cand), f"cost K={K}")
                                same(a, b, a.actor_argmin(cand), b.actor_argmin(cand), f"argmin K={K}")
                                w2 = rng.uniform(np.maximum(lo, -2.0), np.minimum(hi, 2.0), (B, dc)).astype(a.real)
                                same(a, b, a.actor_cost(cand, w=w2), b.actor_cost(cand, w=w2), f"cost K={K}, explicit w")
                            same(a, b, a.actor_argmin(None, K=9), b.actor_argmin(None, K=9), "generated grid K=9")  # (k_actor)
                            u = rand_actions(rng, name, (B,)).astype(a.real)
                            same(a, b, a.critic(x0, u, w), b.critic(x0, u, w), "critic", kinds=())
                            ob = np.stack([rand_states(rng, name, B) for _ in range(BS)], axis=1)
                            ab = rand_actions(rng, name, (B, BS))
                            for e in (a, b):
                                e.set_field(N.FIELD_OBS_BUF, ob)
                                e.set_field(N.FIELD_ACT_BUF, ab)
                            same(a, b, a.critic_cost(w), b.critic_cost(w), "critic_cost", kinds=())
                            same(a, b, a.critic_cost(), b.critic_cost(), "critic_cost of W_CRITIC", kinds=())
                        cand = rand_actions(rng, name, (B, Kt, Nh)).astype(a.real)
                        for t in range(6):
                            a.control_tick(cand)
                            b.control_tick(cand)
                            same(a, b, tuple(a.get_field(f) for f in fields), tuple(b.get_field(f) for f in fields),
                                 f"tick {t} m={n_critic - 1} K={Kt}", kinds=(N.KERNEL_ACTOR, N.KERNEL_CRITIC))
                        assert not np.array_equal(a.get_field(N.FIELD_W_CRITIC), w), (tag, "the fit moved the weights")
                        for t in range(2):  # ... and on the generated grid (k_actor)
                            a.control_tick(None, K=9)
                            b.control_tick(None, K=9)
                            same(a, b, tuple(a.get_field(f) for f in fields), tuple(b.get_field(f) for f in fields),
                                 f"grid tick {t} m={n_critic - 1}", kinds=(N.KERNEL_ACTOR, N.KERNEL_CRITIC))
                        a.close()
                        b.close()
    names = {k for k, _ in kernels}
    assert {"k_actor_dma", "k_actor_dma_packed", "k_actor", "k_critic_fit"} <= names, kernels
    assert ("k_critic_fit", "gen") in kernels and ("k_critic_fit", "ml") in kernels, kernels
    print("copies bit-identical:", checked, "comparisons;", sorted(kernels))


@pytest.mark.gpu
def test_copies_with_critic_are_bit_identical_to_the_builtins():
    env = {k: v for k, v in os.environ.items() if k != "PYTHONPATH"}
    code = "import sys; sys.path.insert(0, %r); import tests.test_hip_user_system_critic as t; t._copies_compare(); " \
           "assert 'torch' not in sys.modules" % ROOT
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=2400)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "bit-identical" in r.stdout


# ---- 2. the pendulum with an output map --------------------------------------------------------------------------------------
def _pendulum(name="PendulumYCG", tgt=True):
    """The pendulum of F15, registered with TGT = true (F15's cases carry a target: the preset-cost instances DMA_RQL_* /
    DMA_SQL_* serve them); without TGT the same handles take DMA_RQL_GEN_* in RQL and k_actor in SQL."""
    from rcognita_amd import _native as N

    return N.register_system(name, pendulum_critic_source(name, tgt=tgt), 2, 1, 3)


def _engine(sid, dtype, B, meta, mode, cs, K=None, **kw):
    from rcognita_amd import Engine, EngineConfig

    cfg = dict(sys_id=sid, batch=B, dtype=dtype, Nactor=meta["Nactor"], mode=mode, critic_struct=cs, Ncritic=meta["Ncritic"],
               buffer_size=meta["buffer_size"], gamma=meta["gamma"], pars=meta["pars"], ctrl_bnds=BND, R1=np.diag(meta["R1"]),
               observation_target=np.array(meta["target"]), dt_sim=0.01, sampling_time=meta["sampling_time"],
               pred_step_size=meta["pred_step_size"])
    cfg.update(kw)
    return Engine(EngineConfig(**cfg))


def _ocfg(meta, mode, cs, **kw):
    """What the oracle's critic functions read of a configuration (they take the dimensions from their arguments)."""
    from oracle import rcg_oracle as O

    d = dict(mode=O.MODE_IDS[mode], critic_struct=O.CRITIC_IDS[cs], target=np.array(meta["target"]), R1=np.diag(meta["R1"]), R2=None,
             stage_obj_struct=O.STAGE_QUADRATIC, n_critic=meta["Ncritic"], buffer_size=meta["buffer_size"], gamma=meta["gamma"],
             dc=meta["dim_critic"][cs], n_actor=meta["Nactor"], pred_step_size=meta["pred_step_size"], pars=np.array(meta["pars"]),
             sampling_time=meta["sampling_time"], dt_sim=0.01, substeps_per_tick=1, critic_every_ticks=1, ctrl_bnds=BND)
    d.update(kw)
    return types.SimpleNamespace(**d)


def _actor_cost_batched(cfg, cand, ys, xs, w):
    """The restatement's _actor_cost (actor_cost_critic) for candidates [B, K, N], vectorised over B and K with the oracle's
    stage cost and critic on [y, u]."""
    from oracle import rcg_oracle as O

    B, K, N = cand.shape
    x = np.broadcast_to(xs[:, None, :], (B, K, 2)).copy()
    y = np.broadcast_to(ys[:, None, :], (B, K, 3))
    J = np.zeros((B, K))
    for k in range(N):
        u = cand[:, :, k, None]
        if k > 0:
            m, g, l = cfg.pars
            up = cand[:, :, k - 1]
            x = x + cfg.pred_step_size * np.stack([x[..., 1], -g / l * np.sin(x[..., 0]) + up / (m * l * l)], axis=-1)
            y = pend_out(x)
        if cfg.mode == O.MODE_SQL or k == N - 1:
            J = J + O.critic(y, u, w[:, None, :], cfg)
        else:
            J = J + cfg.gamma ** k * O.stage_obj(y, u, cfg)
    return J


def _row_err(J, J_ref):
    """Signed critic weights make J a difference of large terms: the error is measured against the env's largest |J| (what an
    argmin over the row is sensitive to), as tests/test_hip_critic.py measures it."""
    return float(np.max(np.abs(J - J_ref) / np.max(np.abs(J_ref), axis=1, keepdims=True)))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("cs", STRUCTS)
def test_f15_operators_through_the_c_abi(cs, dtype):
    """_critic, _critic_cost and the RQL / SQL _actor_cost of F15 (the reference's own numbers) through rcg_critic,
    rcg_critic_cost and rcg_actor_cost on every decision kernel; the whole J of each launch against the restatement."""
    from rcognita_amd import _native as N

    from tests.helpers import rel_err_norm

    meta, z = load_f15()
    sid = _pendulum()["sys_id"]
    k = cs.replace("-", "_")
    tol = TOL[dtype]
    # (c) _critic: measured against the largest |Q| of the set, as tests/test_hip_parity.py measures F3
    Q = z[f"c_{k}_Q"]
    e = _engine(sid, dtype, len(Q), meta, "RQL", cs)
    assert e.dc == meta["dim_critic"][cs] and e.dy == 3 and e.ds == 2
    err = rel_err_norm(e.critic(z[f"c_{k}_obs"], z[f"c_{k}_act"], z[f"c_{k}_w"]), Q, floor=float(np.max(np.abs(Q))))
    print(f"critic {cs} {dtype}: {err:.3e}")
    assert err <= tol
    e.close()
    # (d) _critic_cost, measured against the largest Jc of the set
    Jc = z[f"d_{k}_Jc"]
    e = _engine(sid, dtype, len(Jc), meta, "RQL", cs)
    e.set_field(N.FIELD_OBS_BUF, z[f"d_{k}_obs_buf"])
    e.set_field(N.FIELD_ACT_BUF, z[f"d_{k}_act_buf"])
    e.set_field(N.FIELD_W_PREV, z[f"d_{k}_w_prev"])
    err = rel_err_norm(e.critic_cost(z[f"d_{k}_w"]), Jc, floor=float(np.max(np.abs(Jc))))
    print(f"critic_cost {cs} {dtype}: {err:.3e}")
    assert err <= tol
    e.close()
    # (e) _actor_cost: candidate 0 of every env is the fixture's sequence
    rng = np.random.default_rng(21)
    sid_gen = _pendulum("PendulumYCN", tgt=False)["sys_id"]
    for mode, sid_e in (("RQL", sid), ("SQL", sid), ("RQL", sid_gen), ("SQL", sid_gen)):
        p = f"e_{mode}_{k}"
        xs, ys, seq, w, Jref = (z[p + s] for s in ("_state_sys", "_obs", "_seq", "_w", "_J"))
        B, Nh = len(xs), meta["Nactor"]
        e = _engine(sid_e, dtype, B, meta, mode, cs)
        ocfg = _ocfg(meta, mode, cs)
        real = e.real
        r = lambda a: a.astype(real).astype(float)  # noqa: E731
        seen = set()
        for K in (256, 16, 6):
            cand = rng.uniform(-5, 5, (B, K, Nh)).astype(real)
            cand[:, 0] = seq.astype(real)
            J = e.actor_cost(cand.reshape(B, K, Nh, 1), obs=ys, state_sys=xs, w=w)
            ll = e.last_launch()
            seen.add(ll["kernel"])
            Jr = _actor_cost_batched(ocfg, cand.astype(float), r(ys), r(xs), r(w))
            scale = np.max(np.abs(Jr), axis=1)
            err0 = float(np.max(np.abs(J[:, 0] - Jref) / scale))
            err = _row_err(J, Jr)
            print(f"actor_cost {mode} {cs} {dtype} K={K} {ll['kernel']}/{ll['variant']}: vs F15 {err0:.3e}, vs restatement {err:.3e}")
            assert err0 <= tol and err <= tol, (mode, K, ll)
            if dtype == "f64":  # the restatement itself is F15's function
                i = int(rng.integers(B))
                Ji = actor_cost_critic(mode, cs, xs[i], ys[i], cand[i, 3], w[i], ocfg.R1, ocfg.gamma, ocfg.target, ocfg.pred_step_size,
                                       meta["pars"])
                assert abs(Ji - Jr[i, 3]) <= 1e-12 * max(1.0, abs(Ji))
            # (these structures have at most 14 weights: the packed instances exist in both element types)
            if sid_e == sid:
                want = ("k_actor_dma" if K == 256 else "k_actor_dma_packed", (N.DMA_RQL_0 if mode == "RQL" else N.DMA_SQL_0) + STRUCTS.index(cs))
            else:  # a target the policy's TGT does not announce: RQL on DMA_RQL_GEN_* from K = 20, the rest on k_actor
                want = ("k_actor_dma", N.DMA_RQL_GEN_0 + STRUCTS.index(cs)) if (mode == "RQL" and K == 256) else ("k_actor", ll["variant"])
            assert (ll["kernel"], ll["variant"]) == want, (mode, K, ll, want)
            act, bj, bi = e.actor_argmin(cand.reshape(B, K, Nh, 1), obs=ys, state_sys=xs)  # (the handle's W_CRITIC: ones)
            J1 = _actor_cost_batched(ocfg, cand.astype(float), r(ys), r(xs), np.ones_like(w))
            assert float(np.max(np.abs(bj - J1.min(axis=1)) / np.max(np.abs(J1), axis=1))) <= tol
        # the generated grid: 64 levels of the torque held over the horizon, on k_actor's critic terms
        e.set_field(N.FIELD_W_CRITIC, w)
        act, bj, bi = e.actor_argmin(None, K=64, obs=ys, state_sys=xs)
        assert e.last_launch()["kernel"] == "k_actor"
        grid = np.broadcast_to(np.linspace(-5, 5, 64).astype(real).astype(float)[None, :, None], (B, 64, Nh))
        Jg = _actor_cost_batched(ocfg, grid, r(ys), r(xs), r(w))
        assert float(np.max(np.abs(bj - Jg.min(axis=1)) / np.max(np.abs(Jg), axis=1))) <= tol, mode
        seen.add("k_actor")
        need = {"k_actor_dma", "k_actor_dma_packed", "k_actor"} if sid_e == sid else ({"k_actor_dma", "k_actor"} if mode == "RQL" else {"k_actor"})
        assert seen == need, (mode, seen)
        e.close()


def _restated_tick(cfg, env, cand, force_idx=None):
    """oracle.rcg_oracle.control_tick for the pendulum with y = out(x): the same order of steps - env step, push of
    (action_curr, out(state)), fit, _actor_cost from y_0 = out(state), argmin, accum at out(state)."""
    from oracle import rcg_oracle as O

    m, g, l = cfg.pars
    clip = lambda u: np.clip(u, BND[:, 0], BND[:, 1])  # noqa: E731

    def f(x, u):
        return np.stack([x[:, 1], -g / l * np.sin(x[:, 0]) + u[:, 0] / (m * l * l)], axis=-1)

    for _ in range(cfg.substeps_per_tick):  # classical RK4 under the held, clipped action
        x, u, h = env.state, clip(env.action), cfg.dt_sim
        k1 = f(x, u)
        k2 = f(x + 0.5 * h * k1, u)
        k3 = f(x + 0.5 * h * k2, u)
        k4 = f(x + h * k3, u)
        env.state_prev, env.state = x, x + (h / 6.0) * (k1 + 2.0 * k2 + 2.0 * k3 + k4)
    y = pend_out(env.state)
    env.act_buf, env.obs_buf = O.push_vec(env.act_buf, env.action), O.push_vec(env.obs_buf, y)
    env.w_critic = O.critic_fit(cfg, env.w_prev, env.obs_buf, env.act_buf)
    env.w_prev = env.w_critic
    env.tick_count += 1
    cand = np.asarray(cand, dtype=np.float64)
    J = _actor_cost_batched(cfg, cand[..., 0], y, env.state, env.w_critic)
    best_J, best_idx = O.argmin_first(J)
    if force_idx is not None:
        fi = np.asarray(force_idx)
        best_idx = np.where(fi >= 0, fi, best_idx).astype(np.int32)
        best_J = np.take_along_axis(np.where(np.isnan(J), np.inf, J), best_idx[:, None].astype(np.int64), axis=1)[:, 0]
    env.best_J, env.best_idx = best_J, best_idx
    env.action = np.take_along_axis(cand[:, :, 0, :], best_idx[:, None, None].astype(np.int64), axis=1)[:, 0, :]
    env.accum = env.accum + O.stage_obj(y, env.action, cfg) * cfg.sampling_time
    env.step_idx = env.step_idx + np.int32(1)
    return J


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("cs", STRUCTS)
@pytest.mark.parametrize("mode", ["RQL", "SQL"])
def test_closed_loop_ticks_against_the_restatement(mode, cs, dtype, monkeypatch):
    """Nine ticks - env step, push of out(STATE), fit, decision on k_actor_dma - each checked as a map from the same inputs by
    oracle/parity.py::check_tick with the restated tick in the oracle's place; a near-tied argmin is followed.  The
    tolerances are those of tests/test_hip_critic.py::test_rql_sql_control_tick_vs_oracle."""
    from oracle import parity as PAR
    from oracle import rcg_oracle as O
    from rcognita_amd import _native as N

    meta, _ = load_f15()
    sid = _pendulum()["sys_id"]
    monkeypatch.setattr(O, "control_tick", _restated_tick)
    rng = np.random.default_rng(31)
    B, K, T = 19, 64, 9
    e = _engine(sid, dtype, B, meta, mode, cs, buffer_size=6)
    cfg = _ocfg(meta, mode, cs, buffer_size=6)
    x0 = np.stack([rng.uniform(-3, 3, B), rng.uniform(-2, 2, B)], axis=-1).astype(e.real)
    e.set_state(x0)
    a0 = e.get_field(N.FIELD_ACTION).astype(float)
    env = O.EnvBatch(state=x0.astype(float), action=a0, accum=np.zeros(B), step_idx=np.zeros(B, np.int32),
                     episode_idx=np.zeros(B, np.int32), pars=cfg.pars, state_prev=x0.astype(float).copy(),
                     w_critic=np.ones((B, cfg.dc)), w_prev=np.ones((B, cfg.dc)), obs_buf=np.zeros((B, 6, 3)),
                     act_buf=np.zeros((B, 6, 1)))
    cand = rng.uniform(-5, 5, (B, K, meta["Nactor"], 1)).astype(e.real)
    rep = PAR.TickReport()
    for t in range(T):
        e.control_tick(cand)
        assert e.last_launch()["kernel"] == "k_actor_dma" and e.last_launch(N.KERNEL_CRITIC)["kernel"] == "k_critic_fit"
        np.testing.assert_allclose(e.get_field(N.FIELD_OBS_BUF)[:, -1], pend_out(e.get_state().astype(float)), rtol=0,
                                   atol=1e-15 if dtype == "f64" else 1e-6)
        env = PAR.check_tick(cfg, env, cand.astype(float), PAR.device_fields(e, N, critic=True),
                             tol=1e-9 if dtype == "f64" else 1e-5,
                             tol_over={"w_critic": 1e-6, "best_J": 1e-7} if dtype == "f64" else None, report=rep,
                             what=f"{mode} {cs} t={t}")
    assert rep.ticks == T
    print(f"ticks {mode} {cs} {dtype}:", rep.as_dict())
    e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("cs", STRUCTS)
def test_fit_objective_against_the_oracle_fit_and_slsqp(cs, dtype):
    """F15 (f): the TD stacks the reference's SLSQP fitted.  The fit on those buffers (rcg_critic_fit: no push - the newest row is
    an observation [3]) against oracle.rcg_oracle.critic_fit_single on the same TD system and against SLSQP's Jc: the
    comparison and band of tests/test_hip_critic.py::test_critic_fit_vs_oracle_and_reference_slsqp, on Jc."""
    from oracle import rcg_oracle as O
    from rcognita_amd import _native as N

    meta, z = load_f15()
    sid = _pendulum()["sys_id"]
    k = cs.replace("-", "_")
    ob, ab, wp = z[f"f_{k}_obs_buf"], z[f"f_{k}_act_buf"], z[f"f_{k}_w_prev"]
    e = _engine(sid, dtype, len(ob), meta, "RQL", cs)
    cfg = _ocfg(meta, "RQL", cs)
    e.set_field(N.FIELD_OBS_BUF, ob)
    e.set_field(N.FIELD_ACT_BUF, ab)
    e.set_field(N.FIELD_W_PREV, wp)
    e.critic_fit()
    assert e.last_launch(N.KERNEL_CRITIC)["kernel"] == "k_critic_fit"
    np.testing.assert_array_equal(e.get_field(N.FIELD_OBS_BUF), ob.astype(e.real))  # no push
    w = e.get_field(N.FIELD_W_CRITIC).astype(np.float64)
    np.testing.assert_array_equal(e.get_field(N.FIELD_W_PREV).astype(np.float64), w)
    rb = lambda a: a.astype(e.real).astype(np.float64)  # noqa: E731
    w_or = O.critic_fit(cfg, rb(wp), rb(ob), rb(ab))
    Jc = O.critic_cost(w, rb(wp), rb(ob), rb(ab), cfg)
    Jc_or = O.critic_cost(w_or, rb(wp), rb(ob), rb(ab), cfg)
    J0, Js = z[f"f_{k}_Jc_init"], z[f"f_{k}_Jc"]
    lo, hi = O.critic_bounds(cfg.critic_struct, cfg.dc)
    assert np.all(w >= lo - 1e-4) and np.all(w <= hi + 1e-3)
    slack = 1e-6 if dtype == "f64" else 1e-4
    print(f"fit {cs} {dtype}: max |Jc - Jc_or| / J0 {float(np.max(np.abs(Jc - Jc_or) / J0)):.3e}, "
          f"max (Jc - Js) / J0 {float(np.max((Jc - Js) / J0)):.3e}, max Jc / J0 {float(np.max(Jc / J0)):.3e}")
    assert np.all(np.abs(Jc - Jc_or) <= 1e-5 * J0 + 1e-9)
    assert np.all(Jc <= Js * (1 + slack) + slack * J0), float(np.max((Jc - Js) / J0))
    assert np.all(Jc <= J0 * (1 + slack))
    e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,tol", [("f64", 0.0), ("f32", 2e-4)])
@pytest.mark.parametrize("cs", STRUCTS)
def test_optimizer_in_rql_with_out_jac_against_slsqp(cs, dtype, tol):
    """30 iterations of rcg_actor_optimize in RQL - dQ/dy of the terminal critic through out_jac_T - from the reference's start
    against F15 (g)'s SLSQP cost, with the (1 + 5e-3) rule of test_hip_user_system_out.py; the reported J is the restated J of
    the returned sequence."""
    from rcognita_amd import _native as N

    from tests.helpers import rel_err_norm

    meta, z = load_f15()
    sid = _pendulum()["sys_id"]
    k = cs.replace("-", "_")
    x, w = z[f"g_{k}_state"], z[f"g_{k}_w"]
    B = len(x)
    e = _engine(sid, dtype, B, meta, "RQL", cs)
    cfg = _ocfg(meta, "RQL", cs)
    e.set_state(x)
    e.set_field(N.FIELD_W_CRITIC, w)
    act, U, J, _ = e.actor_optimize(iters=30)
    assert e.last_launch()["kernel"] == "k_actor_opt"
    xr, wr = x.astype(e.real).astype(float), w.astype(e.real).astype(float)
    Jr = _actor_cost_batched(cfg, U[:, None, :, 0].astype(float), pend_out(xr), xr, wr)[:, 0]
    assert rel_err_norm(J, Jr) < (1e-10 if dtype == "f64" else tol)
    Jopt = z[f"g_{k}_J_opt"]
    print(f"optimizer RQL {cs} {dtype}: max (J - J_slsqp) / |J_slsqp| {float(np.max((J - Jopt) / np.abs(Jopt))):.3e}")
    bar = Jopt + np.abs(Jopt) * (5e-3 + tol)  # (f32: the cost itself is evaluated to ~1e-6)
    assert np.all(J <= bar), (J - Jopt) / np.abs(Jopt)
    e.close()


# ---- 3. the drop-in controller -----------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_ctrl_opt_pred_rql_drop_in_loop_matches_the_restated_loop():
    """50 iterations of the reference's loop body (System subclass + Simulator + CtrlOptPred(mode="RQL") over a fixed candidate
    set) against the restated loop: push of (action_curr, observation), the fit of oracle.rcg_oracle on the controller's own
    buffers, the argmin of the restated RQL _actor_cost."""
    from oracle import rcg_oracle as O
    from rcognita_amd.controllers import CtrlOptPred
    from rcognita_amd.simulator import Simulator
    from rcognita_amd.systems import System

    meta, _ = load_f15()

    class PendulumCrit(System):
        hip_policy = pendulum_critic_source("PendulumYCG", tgt=True)  # (the registration of _pendulum(): same name, same source)

    sys_ = PendulumCrit(sys_type="diff_eqn", dim_state=2, dim_input=1, dim_output=3, dim_disturb=0, pars=meta["pars"], ctrl_bnds=BND)
    assert PendulumCrit._hip_info["has_critic"]
    x0 = np.array([2.5, 0.0])
    N_, dt, bs, nc, cs = 10, 0.05, 8, 4, "quad-nomix"
    rng = np.random.default_rng(41)
    cand = rng.uniform(-5, 5, (64, N_))
    R1, target = np.diag(meta["R1"]), np.array(meta["target"])
    ctrl = CtrlOptPred(1, 3, mode="RQL", ctrl_bnds=BND, Nactor=N_, sampling_time=dt, pred_step_size=dt, sys_rhs=sys_._state_dyn,
                       sys_out=sys_.out, state_sys=x0, stage_obj_pars=[R1], observation_target=target, candidates=cand,
                       buffer_size=bs, Ncritic=nc, critic_period=dt, critic_struct=cs, gamma=0.95)
    assert ctrl.dim_critic == 4 and ctrl.w_critic.shape == (4,) and ctrl.observation_buffer.shape == (bs, 3)
    sim = Simulator(sys_type="diff_eqn", closed_loop_rhs=sys_.closed_loop_rhs, sys_out=sys_.out, state_init=x0, t0=0, t1=100,
                    dt=dt, max_step=dt / 10, first_step=1e-6, atol=1e-5, rtol=1e-3, is_disturb=0, is_dyn_ctrl=0)
    cfg = _ocfg(meta, "RQL", cs, n_critic=nc, buffer_size=bs, gamma=0.95, pred_step_size=dt, dc=4)
    ob, ab, wp, a_prev = np.zeros((bs, 3)), np.zeros((bs, 1)), np.ones(4), np.array(ctrl.action_curr, dtype=float)
    moved = fitted = False
    for k in range(50):
        sim.sim_step()
        t, xk, y, _ = sim.get_sim_step_data()
        xs = np.array(ctrl.state_sys, dtype=float)
        a = ctrl.compute_action(t, y)
        ab, ob = O.push_vec(ab, a_prev), O.push_vec(ob, y)
        np.testing.assert_array_equal(ctrl.observation_buffer, ob)
        np.testing.assert_array_equal(ctrl.action_buffer, ab)
        w = O.critic_fit(cfg, wp[None], ob[None], ab[None])[0]
        Jw, Jc = O.critic_cost(ctrl.w_critic, wp, ob, ab, cfg), O.critic_cost(w, wp, ob, ab, cfg)
        J0 = O.critic_cost(np.ones(4), wp, ob, ab, cfg)
        assert abs(Jw - Jc) <= 1e-5 * J0 + 1e-9, k
        fitted = fitted or not np.allclose(ctrl.w_critic, 1.0)
        wp = np.array(ctrl.w_critic, dtype=float)  # (the restated loop continues from the controller's weights)
        J = [actor_cost_critic("RQL", cs, xs, y, cand[i], wp, R1, 0.95, target, dt, meta["pars"]) for i in range(len(cand))]
        np.testing.assert_allclose(a, cand[int(np.argmin(J)), :1], rtol=0, atol=1e-12, err_msg=str(k))
        assert abs(ctrl.last_J[0] - min(J)) <= 1e-9 * max(1.0, abs(min(J))), k
        moved = moved or abs(xk[0] - x0[0]) > 1e-3
        a_prev = np.array(a, dtype=float)
        sys_.receive_action(a)
        ctrl.receive_sys_state(sys_._state)
    assert moved and fitted
    ctrl.reset(0)  # only the clock and the current action (controllers.py:1046-1054): buffers and weights stay
    np.testing.assert_array_equal(ctrl.observation_buffer, ob)
    np.testing.assert_array_equal(ctrl.action_curr, BND[:, 0] / 10)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name,cs,n_critic", [("2tank", "quad-nomix", 4), ("3wrobot", "quad-lin", 4), ("3wrobotNI", "quadratic", 7),
                                              ("2tank", "quad-mix", 12)])
def test_critic_fit_on_a_builtin_equals_critic_update_on_shifted_buffers(name, cs, n_critic, dtype):
    """rcg_critic_fit (the fit alone, no push) on a built-in handle: the same bits as rcg_critic_update on the buffers shifted
    down by one with the newest row handed over through STATE / ACTION - on each fit form (3, 6 and 11 TD rows)."""
    from oracle import rcg_oracle as O
    from rcognita_amd import _native as N

    from tests.helpers import both, rand_actions, rand_states

    rng = np.random.default_rng(51)
    B, bs = 300, 14
    a, cfg = both(name, B, dtype, mode=O.MODE_RQL, critic_struct=O.CRITIC_IDS[cs], gamma=0.95, n_critic=n_critic, buffer_size=bs)
    b, _ = both(name, B, dtype, mode=O.MODE_RQL, critic_struct=O.CRITIC_IDS[cs], gamma=0.95, n_critic=n_critic, buffer_size=bs)
    ob = np.stack([rand_states(rng, name, B) for _ in range(bs)], axis=1)
    ab = rand_actions(rng, name, (B, bs))
    lo, hi = O.critic_bounds(cfg.critic_struct, cfg.dc)
    wp = rng.uniform(np.maximum(lo, -2.0), np.minimum(hi, 2.0), (B, cfg.dc))
    a.set_field(N.FIELD_OBS_BUF, ob)
    a.set_field(N.FIELD_ACT_BUF, ab)
    a.set_field(N.FIELD_W_PREV, wp)
    a.critic_fit()
    b.set_field(N.FIELD_OBS_BUF, np.concatenate([np.zeros_like(ob[:, :1]), ob[:, :-1]], axis=1))
    b.set_field(N.FIELD_ACT_BUF, np.concatenate([np.zeros_like(ab[:, :1]), ab[:, :-1]], axis=1))
    b.set_field(N.FIELD_STATE, ob[:, -1])
    b.set_field(N.FIELD_ACTION, ab[:, -1])
    b.set_field(N.FIELD_W_PREV, wp)
    b.critic_update(do_fit=True)
    for f in (N.FIELD_OBS_BUF, N.FIELD_ACT_BUF, N.FIELD_W_CRITIC, N.FIELD_W_PREV):
        u, v = a.get_field(f), b.get_field(f)
        assert u.tobytes() == v.tobytes(), (name, cs, f)
    assert not np.array_equal(a.get_field(N.FIELD_W_CRITIC), np.ones((B, cfg.dc), a.real))
    la, lb = a.last_launch(N.KERNEL_CRITIC), b.last_launch(N.KERNEL_CRITIC)
    assert la == lb and la["kernel"] == "k_critic_fit", (la, lb)
    a.close()
    b.close()


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_create_in_rql_and_what_stays_refused():
    import ctypes as C

    from rcognita_amd import _native as N

    meta, _ = load_f15()
    info = _pendulum()
    L = N.lib()
    B = 256
    e = _engine(info["sys_id"], "f64", B, meta, "RQL", "quad-nomix")  # (refused before CRITIC existed)
    x0 = np.random.default_rng(4).uniform(-1, 1, (B, 2))
    e.set_state(x0)
    fields = {f: e.get_field(f).copy() for f in (N.FIELD_STATE, N.FIELD_STEP_IDX, N.FIELD_OBS_BUF, N.FIELD_ACT_BUF, N.FIELD_W_CRITIC)}
    h = e._h
    out = (C.c_double * (B * 16))()
    act = (C.c_double * B)()
    dev = e.empty((B, 3))
    e.set_tick_parts(2)
    cand = e.to_device(np.random.default_rng(5).uniform(-5, 5, (B, 64, meta["Nactor"], 1)))
    calls = {
        "control_ticks": lambda: L.rcg_control_ticks(h, 2, 16),
        "actor_search": lambda: L.rcg_actor_search(h, 64, 2, None, None, None, None, None, None, None),
        "nominal_action": lambda: L.rcg_nominal_action(h, C.c_void_p(dev.ptr), C.c_void_p(dev.ptr), None, B, 1.0, None, 0),
        "control_tick_nominal": lambda: L.rcg_control_tick_nominal(h, 1.0, None),
        "loop_step_begin": lambda: L.rcg_loop_step_begin(h, C.cast(act, C.c_void_p), 0.01, 1, N.LOOP_DECIDE, 5),
        "loop_step": lambda: L.rcg_loop_step(h, C.cast(act, C.c_void_p), 0.01, 1, 0, 5, C.cast(out, C.c_void_p)),
        "control_tick_search": lambda: L.rcg_control_tick_search(h, 64, 2, 0),
        "split tick": lambda: L.rcg_control_tick(h, C.c_void_p(cand.ptr), 64),
    }
    for what, call in calls.items():
        assert call() == N.ERR_UNSUPPORTED, what
        for f, v in fields.items():
            assert np.array_equal(e.get_field(f), v), (what, f)
    e.set_tick_parts(0)
    e.control_tick(cand)  # ... and the whole tick runs
    assert np.array_equal(e.get_field(N.FIELD_STEP_IDX), np.ones(B, np.int32))
    e.close()
    with pytest.raises((N.NativeError, NotImplementedError)):
        _engine(info["sys_id"], "f64", B, meta, "RQL", "quad-nomix", is_disturb=True, pars_disturb=[[0.1], [0.0], [1.0]])
