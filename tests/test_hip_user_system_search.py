"""The device candidate search on systems compiled at run time (rcg.h: the policy member SEARCH) on the GPU.

1. Sys3WRobot and Sys2Tank, re-registered from their own source with SEARCH + CRITIC under other names, against the built-in
   handles: rcg_actor_search and three rcg_control_tick_search ticks, every output and field bit for bit and the same kernel,
   variant and envs per wave (rcg_last_launch), on every k_actor_search instance (register rows / LDS rows / generic, with and
   without critic weights).  In a child process that does not import torch, as test_hip_user_system.py does.
2. The pendulum without an output map (DS = 2, DU = 1, no jac_T) against the oracle with the pendulum patched in, replaying the
   rounds over the device's own candidates (the assertions of tests/test_hip_search.py).
3. The pendulum with y = (sin th, cos th, om) (DY = 3) against the restatement (test_user_system_search_register.py::pend_cost):
   an observation handed in, and self-driven (y_0 = out(STATE)); MPC with a diagonal R1, a full R1 and a target; RQL / SQL.
4. Closed loop: five rcg_control_tick_search ticks, each checked as a map from the device's own pre-tick fields.
5. CtrlOptPred(actor_opt="sampling") as a drop-in loop on a policy that has a right-hand side and nothing else.
6. The search against the reference's SLSQP costs (F14).
7. Refusals.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.helpers import TOL  # noqa: E402
from tests.test_user_system_critic_register import load_f15  # noqa: E402
from tests.test_user_system_out_register import load_f14, pend_out  # noqa: E402
from tests.test_user_system_search_register import (BND, F14_SEARCH_GAP, PEND_PARS, SEEDS, pend_cost, pendulum_out_search_source,  # noqa: E402
                                                    pendulum_search_source, search_inputs, search_replay, with_search)

pytestmark = pytest.mark.gpu

ROWS = 4  # rcg_last_launch's variant word of k_actor_search: bit 0 generic, bit 1 target, bit 2 register rows


# ---- 1. copies of two built-in systems ---------------------------------------------------------------------------------------
def _copy_source(struct, name):
    from tests.test_hip_user_system_critic import _copy_source as with_critic_copy

    return with_search(with_critic_copy(struct, name))


def _copies_compare():
    """The child: built-in Sys3WRobot / Sys2Tank against their renamed copies with SEARCH + CRITIC; raises on the first
    difference."""
    from oracle import rcg_oracle as O
    from rcognita_amd import Engine
    from rcognita_amd import _native as N

    from tests.helpers import PRESETS, engine_cfg, rand_states

    copies = {"3wrobot": N.register_system("UserRobotS", _copy_source("Sys3WRobot", "UserRobotS"), 5, 2, 2),
              "2tank": N.register_system("UserTankS", _copy_source("Sys2Tank", "UserTankS"), 2, 1, 5)}
    assert all(i["has_search"] and i["has_critic"] and not i["has_out"] for i in copies.values())
    B = 1024
    mpc_fields = (N.FIELD_STATE, N.FIELD_ACTION_SQN, N.FIELD_BEST_J, N.FIELD_BEST_IDX, N.FIELD_ACCUM, N.FIELD_STEP_IDX, N.FIELD_ACTION)
    rql_fields = mpc_fields + (N.FIELD_W_CRITIC, N.FIELD_OBS_BUF, N.FIELD_ACT_BUF)
    # (what, Nactor, K, keywords): register rows in both widths | in f32 only | LDS rows | generic | generic with weights;
    # K = 160: the held / per-step boundary 120 falls inside a tile
    shapes = [("rows5", 5, 64, {}), ("rows10", 10, 160, {}), ("lds6", 6, 64, {}), ("lds6 gamma", 6, 160, dict(gamma=0.9)),
              ("full R1", 10, 64, dict(full=True)),
              ("RQL", 10, 160, dict(mode=O.MODE_RQL, critic_struct=O.CRITIC_QUAD_NOMIX, n_critic=4, buffer_size=6, gamma=0.95))]
    checked, seen = 0, set()
    for name, info in copies.items():
        n = len(PRESETS[name]["R1"])
        # (the tank: du = 1, one held draw serves eight tiles - the ninth held tile, candidates 512 .., starts a second draw)
        for what, Nh, K, kw in shapes + ([("K704", 5, 704, {})] if name == "2tank" else []):
            for dtype in ("f64", "f32"):
                tag = (name, what, dtype)
                rng = np.random.default_rng(17)
                kw2 = {k: v for k, v in kw.items() if k != "full"}
                if kw.get("full"):
                    kw2["R1"] = np.diag(np.array(PRESETS[name]["R1"], dtype=float)) + 0.05 * np.ones((n, n))
                rql = kw.get("mode") == O.MODE_RQL

                def make(sid):
                    c = engine_cfg(name, B, dtype, n_actor=Nh, **kw2)
                    c.sys_id, c.seed = sid, 11
                    return Engine(c)

                a, b = make(N.SYS_IDS[name]), make(info["sys_id"])

                def same(x, y, what2):
                    nonlocal checked
                    for u, v in zip(x, y):
                        u, v = np.asarray(u), np.asarray(v)
                        assert u.dtype == v.dtype and u.shape == v.shape and u.tobytes() == v.tobytes(), (tag, what2)
                    la, lb = a.last_launch(N.KERNEL_ACTOR), b.last_launch(N.KERNEL_ACTOR)
                    assert la == lb and la["kernel"] == "k_actor_search", (tag, what2, la, lb)
                    if rql:
                        assert a.last_launch(N.KERNEL_CRITIC) == b.last_launch(N.KERNEL_CRITIC), (tag, what2)
                    checked += 1
                    return la

                x0 = rand_states(rng, name, B)
                obs = x0 + rng.uniform(-0.02, 0.02, x0.shape)
                for e in (a, b):
                    e.set_state(x0)
                    e.set_field(N.FIELD_STEP_IDX, np.arange(B, dtype=np.int32) % 7)
                    if rql:
                        e.set_field(N.FIELD_W_CRITIC, np.random.default_rng(18).uniform(0.1, 2, (B, a.dc)))
                ll = same(a.actor_search(K=K, rounds=2, obs=obs, state_sys=x0), b.actor_search(K=K, rounds=2, obs=obs, state_sys=x0),
                          "actor_search")
                rows = not kw and Nh in (3, 5, 10) and (dtype == "f32" or Nh <= 5)
                assert bool(ll["variant"] & ROWS) == rows, (tag, ll)
                assert bool(ll["variant"] & 1) == bool(kw.get("full") or rql), (tag, ll)
                seen.add((dtype, ll["variant"]))
                fields = rql_fields if rql else mpc_fields
                for t in range(3):
                    a.control_tick_search(K=K, rounds=2, warm_start=True)
                    b.control_tick_search(K=K, rounds=2, warm_start=True)
                    same(tuple(a.get_field(f) for f in fields), tuple(b.get_field(f) for f in fields), f"tick {t}")
                assert np.array_equal(a.get_field(N.FIELD_STEP_IDX), np.arange(B, dtype=np.int32) % 7 + 3), tag
                a.close()
                b.close()
    n_programs = 0
    for i in copies.values():  # one program per instance, compiled once and listed
        programs = [(p, e) for p, e in N.system_programs(i["sys_id"]) if "k_actor_search" in e]
        assert len(programs) == len(set(programs)) >= 6 and all(p == i["name"] + "_search.hip" for p, _ in programs), programs
        n_programs += len(programs)
    print("copies bit-identical:", checked, "comparisons;", sorted(seen), n_programs, "search programs")


def test_copies_with_search_are_bit_identical_to_the_builtins():
    env = {k: v for k, v in os.environ.items() if k != "PYTHONPATH"}
    code = "import sys; sys.path.insert(0, %r); import tests.test_hip_user_system_search as t; t._copies_compare(); " \
           "assert 'torch' not in sys.modules" % ROOT
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=2400)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "bit-identical" in r.stdout


# ---- shared ------------------------------------------------------------------------------------------------------------------
def _register(name, src):
    from rcognita_amd import _native as N

    return N.register_system(name, src, 2, 1, 3)


def _engine(sid, dtype, B, Nh, R1, gamma=1.0, target=None, h=0.02, **kw):
    from rcognita_amd import Engine, EngineConfig

    cfg = dict(sys_id=sid, batch=B, dtype=dtype, Nactor=Nh, pars=PEND_PARS, ctrl_bnds=BND, R1=R1, gamma=gamma,
               observation_target=target, dt_sim=0.01, sampling_time=0.02, pred_step_size=h)
    cfg.update(kw)
    return Engine(EngineConfig(**cfg))


def _device_sampler(eng, K):
    return lambda r, centre: eng.candidates_sample(K, round=r, centre=centre.astype(eng.real)).astype(np.float64)


def _u0(Nh, B):
    return np.full((B, Nh, 1), BND[0, 0] / 10.0)  # action_sqn_init (controllers.py:973-978)


def _check_search(eng, dtype, K, rounds, cost, obs, xs, what):
    """The assertions of tests/test_hip_search.py::test_actor_search_vs_oracle_on_the_device_candidates with `cost(cand [B, K, N])
    -> J [B, K]` in the oracle's place; obs None: self-driven from the handle's STATE."""
    from tests.helpers import assert_kernel, rel_err_norm

    B, Nh = eng.B, eng.N
    act, U, J, bi = eng.actor_search(K=K, rounds=rounds, obs=obs, state_sys=xs)
    ll = assert_kernel(eng, "k_actor_search")
    np.testing.assert_array_equal(act, U[:, 0, :])
    assert np.all(U >= BND[0, 0]) and np.all(U <= BND[0, 1])
    # the reported cost is the restated _actor_cost of the reported sequence
    J_chk = cost(U.astype(np.float64)[:, None, :, 0])[:, 0]
    err = rel_err_norm(J, J_chk)
    # the same search on the device's own candidates
    U_or, J_or, bi_or = search_replay(_device_sampler(eng, K), cost, _u0(Nh, B), rounds)
    same = np.all(U.astype(np.float64) == U_or, axis=(1, 2))
    print(f"search {what} {dtype} {ll['variant']}: |J - J(U)| {err:.3e}, share of envs on the replay's sequence {np.mean(same):.3f}")
    assert err < TOL[dtype], what
    if dtype == "f64":
        np.testing.assert_array_equal(bi, bi_or)
        np.testing.assert_array_equal(U, U_or)
        assert rel_err_norm(J, J_or) < 1e-11, what
    else:  # a float32 argmin may take the other side of a near-tie in some round: the cost reached must agree
        assert np.mean(same) > 0.8, what
        assert np.all(np.abs(J - J_or) <= 4 * TOL[dtype] * np.maximum(np.abs(J_or), 1.0) + 1e-3 * np.abs(J_or) * ~same), what
    # more rounds never hurt (candidate 0 is the incumbent), one round never ends above action_sqn_init's cost
    _, _, J1, _ = eng.actor_search(K=K, rounds=1, obs=obs, state_sys=xs)
    J0 = cost(_u0(Nh, B)[:, None, :, 0])[:, 0]
    slack = 4 * TOL[dtype] * np.maximum(np.abs(J0), 1.0)
    assert np.all(J1 <= J0 + slack) and np.all(J <= J1 + slack), what
    return ll


# ---- 2. the pendulum without an output map -----------------------------------------------------------------------------------
@pytest.fixture
def pend_search_oracle(monkeypatch):
    """The oracle with the SEARCH pendulum (no jac_T) as one more system, as test_hip_user_system.py::pend_oracle teaches it the
    pendulum: its NumPy `_state_dyn` patched into oracle.rcg_oracle for the registered id (nothing under oracle/ changes)."""
    from oracle import rcg_oracle as O

    sid = _register("PendulumSG", pendulum_search_source("PendulumSG"))["sys_id"]
    dyn0 = O.state_dyn

    def state_dyn(sys_id, state, action, pars):
        if sys_id != sid:
            return dyn0(sys_id, state, action, pars)
        x, u, p = (np.asarray(v, dtype=np.float64) for v in (state, action, pars))
        m, g, l = p[..., 0], p[..., 1], p[..., 2]
        d = np.zeros(np.broadcast_shapes(x.shape[:-1], u.shape[:-1], p.shape[:-1]) + (2,))
        d[..., 0] = x[..., 1]
        d[..., 1] = u[..., 0] / (m * l * l) - g / l * np.sin(x[..., 0])
        return d

    monkeypatch.setattr(O, "state_dyn", state_dyn)
    monkeypatch.setitem(O.SYS_DIMS, sid, (2, 1, 3))
    return O, sid


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_pendulum_search_vs_oracle_on_the_device_candidates(pend_search_oracle, dtype):
    """B = 29, K = 192, Nactor = 6, rounds = 3, a STEP_IDX of its own per env.  float32: the seed's CPU dry run - the oracle's
    search over its own candidates with the costs in numpy float32 against float64 - changes the winning sequence of 3.4 % of
    the envs (test_user_system_search_register.py::test_the_float32_seeds_are_far_from_ties; the cap below is 20 %)."""
    O, sid = pend_search_oracle
    from oracle import search_oracle as S
    from rcognita_amd import _native as N

    from tests.helpers import rel_err_norm

    B, K, Nh, rounds = 29, 192, 6, 3
    R1 = np.diag([10.0, 1.0, 0.1])
    x, obs, _ = search_inputs(SEEDS["plain"], B)
    eng = _engine(sid, dtype, B, Nh, R1, gamma=0.96, seed=7)
    cfg = O.OracleCfg(sys_id=sid, n_actor=Nh, gamma=0.96, pred_step_size=0.02, dt_sim=0.01, sampling_time=0.02, pars=PEND_PARS,
                      ctrl_bnds=BND, R1=R1)
    eng.set_field(N.FIELD_STEP_IDX, np.arange(B, dtype=np.int32))
    obs_r, x_r = (a.astype(eng.real).astype(np.float64) for a in (obs, x))
    cost = lambda cand: O.actor_cost(cand[..., None], obs_r[:, None], x_r[:, None], cfg)  # noqa: E731
    ll = _check_search(eng, dtype, K, rounds, cost, obs, x, "pendulum")
    assert ll["variant"] == 0, ll  # LDS rows, diagonal stage cost, no target
    # ... and the oracle's own twin of the whole search on the device's candidates (oracle/search_oracle.py::actor_search)
    act, U, J, bi = eng.actor_search(K=K, rounds=rounds, obs=obs, state_sys=x)
    U_or, J_or, bi_or = S.actor_search(cfg, obs_r, x_r, K, rounds, 7, np.arange(B), np.zeros(B, int), np.arange(B),
                                       sampler=_device_sampler(eng, K))
    if dtype == "f64":
        np.testing.assert_array_equal(bi, bi_or)
        np.testing.assert_array_equal(U, U_or)
        assert rel_err_norm(J, J_or) < 1e-11
    # the producer's stream is the oracle's: the device's candidates agree with the oracle's own to 1e-5 sigma
    c = eng.candidates_sample(K, round=1, centre=U)
    c_or = S.candidates_sample(cfg, 7, np.arange(B), np.zeros(B, int), np.arange(B), K, 1, centre=U.astype(np.float64))
    assert np.all(np.abs(c - c_or) <= 1e-5 * 2.5 + (0 if dtype == "f64" else 1.2e-7 * 5))
    eng.close()


# ---- 3. the pendulum with y = (sin th, cos th, om) ---------------------------------------------------------------------------
def _out_policy():
    return _register("PendulumYSG", pendulum_out_search_source("PendulumYSG"))


def _out_critic_policy():
    return _register("PendulumYSCG", pendulum_out_search_source("PendulumYSCG", critic=True))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("long", [False, True])
@pytest.mark.parametrize("cost_kind", ["diag", "full", "target"])
def test_out_pendulum_search_mpc_vs_the_restatement(cost_kind, long, dtype):
    """MPC on F14's stage costs: Nactor = 5 with gamma = 1 (the diagonal cost: register rows in both widths), Nactor = F14's 10
    with gamma = 0.9 (register rows in float32 only); once with an observation handed in, once self-driven (obs = None:
    y_0 = out(STATE)).  float32: the dry run changes the winner of 0 - 6.9 % of the envs, case by case (the cap is 20 %)."""
    from rcognita_amd import _native as N

    meta, z = load_f14()
    ci = {"diag": 0, "full": 2, "target": 4}[cost_kind] + (6 if long else 0)
    case = meta["cases"][ci]
    assert case["cost"] == cost_kind
    R1, gamma = z["a_R1"][ci], case["gamma"]
    target = z["a_target"][ci] if cost_kind == "target" else None
    Nh = meta["Nactor"] if long else 5
    B, K, rounds = 29, 192, 3
    sid = _out_policy()["sys_id"]
    x, xl, _ = search_inputs(SEEDS[f"out {cost_kind} {int(long)}"], B)
    eng = _engine(sid, dtype, B, Nh, R1, gamma=gamma, target=target, h=meta["pred_step_size"], seed=7)
    assert (eng.dy, eng.ds) == (3, 2)
    eng.set_field(N.FIELD_STEP_IDX, np.arange(B, dtype=np.int32))
    r = lambda a: a.astype(eng.real).astype(np.float64)  # noqa: E731
    for obs in (pend_out(xl), None):
        eng.set_state(x)
        ys = r(obs) if obs is not None else pend_out(r(x))
        cost = lambda cand: pend_cost(cand, ys, r(x), R1, gamma, target, meta["pred_step_size"], PEND_PARS)  # noqa: E731
        ll = _check_search(eng, dtype, K, rounds, cost, obs, x if obs is not None else None,
                           f"out {cost_kind} N={Nh} {'obs' if obs is not None else 'self-driven'}")
        rows = cost_kind == "diag" and (dtype == "f32" or Nh == 5)
        assert ll["variant"] == (1 if cost_kind == "full" else 0) | (2 if cost_kind == "target" else 0) | (ROWS if rows else 0), ll
    with pytest.raises(N.NativeError) as ei:  # an observation [3] is not a state: it needs state_sys
        eng.actor_search(K=K, rounds=1, obs=pend_out(xl))
    assert ei.value.code == N.ERR_BAD_ARG
    eng.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("cs", ["quad-nomix", "quad-mix"])
@pytest.mark.parametrize("mode", ["RQL", "SQL"])
def test_out_pendulum_search_rql_sql_vs_the_restatement(mode, cs, dtype):
    """CRITIC + SEARCH: the generic instance with critic weights drawn in [0.1, 2] on F15's cost (a target, gamma = 0.95).
    float32: the dry run changes the winner of at most 3.4 % of the envs (the cap is 20 %)."""
    from rcognita_amd import _native as N

    meta, _ = load_f15()
    R1, target, gamma, Nh = np.diag(meta["R1"]), np.array(meta["target"]), meta["gamma"], meta["Nactor"]
    B, K, rounds = 29, 192, 3
    sid = _out_critic_policy()["sys_id"]
    x, xl, w = search_inputs(SEEDS[f"{mode} {cs}"], B)
    w = w[:, : meta["dim_critic"][cs]]
    eng = _engine(sid, dtype, B, Nh, R1, gamma=gamma, target=target, h=meta["pred_step_size"], seed=7, mode=mode, critic_struct=cs,
                  Ncritic=meta["Ncritic"], buffer_size=meta["buffer_size"])
    assert eng.dc == w.shape[1]
    eng.set_field(N.FIELD_STEP_IDX, np.arange(B, dtype=np.int32))
    eng.set_field(N.FIELD_W_CRITIC, w)
    r = lambda a: a.astype(eng.real).astype(np.float64)  # noqa: E731
    for obs in (pend_out(xl), None):
        eng.set_state(x)
        ys = r(obs) if obs is not None else pend_out(r(x))
        cost = lambda cand: pend_cost(cand, ys, r(x), R1, gamma, target, meta["pred_step_size"], PEND_PARS, mode=mode, cs=cs,  # noqa: E731
                                      w=r(w))
        ll = _check_search(eng, dtype, K, rounds, cost, obs, x if obs is not None else None,
                           f"{mode} {cs} {'obs' if obs is not None else 'self-driven'}")
        assert ll["variant"] == 3, ll  # generic, target
    eng.close()


# ---- 4. closed loop ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,ref_lag", [("MPC", False), ("RQL", False), ("MPC", True)])
def test_out_pendulum_control_tick_search_closed_loop(mode, ref_lag):
    """Five ticks of rcg_control_tick_search (warm start on) in float64, every tick checked as a map from the device's own
    pre-tick fields: the state is rcg_sim_step's bits, RQL: the buffers take (ACTION, out(STATE)) and the weights are the
    oracle's fit, the winner is the replay's over the device's own candidates from y_0 = out(STATE) (rolled out from STATE_PREV
    under REF_LAG), ACTION = U[:, 0], ACCUM grows by the stage cost at out(STATE) x sampling_time."""
    from oracle import rcg_oracle as O
    from rcognita_amd import _native as N

    from tests.helpers import assert_kernel, rel_err_norm
    from tests.test_hip_user_system_critic import _ocfg

    meta, _ = load_f15()
    R1, target, h = np.diag(meta["R1"]), np.array(meta["target"]), meta["pred_step_size"]
    critic = mode != "MPC"
    cs, gamma = "quad-nomix", (0.95 if critic else 1.0)
    B, K, Nh, rounds, T, bs = 29, 128, 5, 2, 5, 6
    sid = (_out_critic_policy() if critic else _out_policy())["sys_id"]
    kw = dict(mode=mode, critic_struct=cs, Ncritic=4, buffer_size=bs) if critic else {}
    eng = _engine(sid, "f64", B, Nh, R1, gamma=gamma, target=target, h=h, seed=99, ref_lag=ref_lag, **kw)
    twin = _engine(sid, "f64", B, Nh, R1, gamma=gamma, target=target, h=h, ref_lag=ref_lag)  # rcg_sim_step's bits
    ocfg = _ocfg(meta, mode, cs, n_critic=4, buffer_size=bs, gamma=gamma, dc=4) if critic else None
    x0, _, _ = search_inputs(12, B)
    eng.set_state(x0)
    prev = None
    for t in range(T):
        pre = {f: eng.get_field(f).copy() for f in (N.FIELD_STATE, N.FIELD_ACTION, N.FIELD_ACCUM, N.FIELD_STEP_IDX)}
        if critic:
            pre.update({f: eng.get_field(f).astype(np.float64) for f in (N.FIELD_W_PREV, N.FIELD_OBS_BUF, N.FIELD_ACT_BUF)})
        eng.control_tick_search(K=K, rounds=rounds, warm_start=True)
        ll = assert_kernel(eng, "k_actor_search")
        assert ll["variant"] == ((1 if critic else 0) | 2), ll
        twin.set_field(N.FIELD_STATE, pre[N.FIELD_STATE])
        twin.set_field(N.FIELD_ACTION, pre[N.FIELD_ACTION])
        twin.sim_step(eng.cfg.substeps_per_tick)
        x1 = eng.get_state()
        np.testing.assert_array_equal(x1, twin.get_state(), err_msg=str(t))
        y1 = pend_out(x1)
        xs = pre[N.FIELD_STATE] if ref_lag else x1
        if ref_lag:
            np.testing.assert_array_equal(eng.get_field(N.FIELD_STATE_PREV), pre[N.FIELD_STATE])
        w = None
        if critic:
            ob, ab = O.push_vec(pre[N.FIELD_OBS_BUF], y1), O.push_vec(pre[N.FIELD_ACT_BUF], pre[N.FIELD_ACTION])
            np.testing.assert_allclose(eng.get_field(N.FIELD_OBS_BUF), ob, rtol=0, atol=1e-15)
            np.testing.assert_array_equal(eng.get_field(N.FIELD_ACT_BUF), ab)
            assert assert_kernel(eng, "k_critic_fit", kind=N.KERNEL_CRITIC)
            w = eng.get_field(N.FIELD_W_CRITIC).astype(np.float64)
            w_or = O.critic_fit(ocfg, pre[N.FIELD_W_PREV], ob, ab)
            assert rel_err_norm(w, w_or, floor=1.0) < 1e-6, t
        # candidates of this tick: STEP_IDX was pre[STEP_IDX] when they were drawn
        eng.set_field(N.FIELD_STEP_IDX, pre[N.FIELD_STEP_IDX])
        centre = None if prev is None else np.concatenate([prev[:, 1:], prev[:, -1:]], axis=1)
        cost = lambda cand: pend_cost(cand, y1, xs, R1, gamma, target, h, PEND_PARS, mode=mode, cs=cs, w=w)  # noqa: E731
        U_or, J_or, bi_or = search_replay(_device_sampler(eng, K), cost, _u0(Nh, B), rounds, centre=centre)
        eng.set_field(N.FIELD_STEP_IDX, pre[N.FIELD_STEP_IDX] + 1)
        U = eng.get_field(N.FIELD_ACTION_SQN)
        np.testing.assert_array_equal(eng.get_field(N.FIELD_BEST_IDX), bi_or, err_msg=str(t))
        np.testing.assert_array_equal(U, U_or, err_msg=str(t))
        assert rel_err_norm(eng.get_field(N.FIELD_BEST_J), J_or) < 1e-10, t
        act = eng.get_field(N.FIELD_ACTION)
        np.testing.assert_array_equal(act, U[:, 0, :])
        chi = np.concatenate([y1 - target, act], axis=-1)
        accum = pre[N.FIELD_ACCUM] + np.einsum("bi,ij,bj->b", chi, R1, chi) * eng.cfg.sampling_time
        assert rel_err_norm(eng.get_field(N.FIELD_ACCUM), accum, floor=float(np.max(np.abs(accum)) + 1e-9)) < 1e-12, t
        prev = U.astype(np.float64)
    np.testing.assert_array_equal(eng.get_field(N.FIELD_STEP_IDX), np.full(B, T, np.int32))
    assert not np.array_equal(eng.get_state(), x0)
    eng.close()
    twin.close()


# ---- 5. the drop-in controller -----------------------------------------------------------------------------------------------
def test_ctrl_opt_pred_sampling_drop_in_loop():
    """50 iterations of the reference's loop body with CtrlOptPred(mode="MPC", actor_opt="sampling") on a policy that has a
    right-hand side and nothing else: every decision is a k_actor_search launch, and the accumulated cost ends below that of
    the same loop holding action_init."""
    from rcognita_amd.controllers import CtrlOptPred
    from rcognita_amd.simulator import Simulator
    from rcognita_amd.systems import System

    class PendulumSearch(System):
        hip_policy = pendulum_search_source("PendulumSG")  # (the registration of pend_search_oracle: same name, same source)

    x0 = np.array([2.5, 0.0])
    N_, dt = 10, 0.05
    R1 = np.diag([10.0, 1.0, 0.1])

    def loop(decide):
        sys_ = PendulumSearch(sys_type="diff_eqn", dim_state=2, dim_input=1, dim_output=2, dim_disturb=0, pars=PEND_PARS,
                              ctrl_bnds=BND)
        info = PendulumSearch._hip_info
        assert info["has_search"] and not info["has_jac"]
        ctrl = CtrlOptPred(1, 2, mode="MPC", ctrl_bnds=BND, Nactor=N_, sampling_time=dt, pred_step_size=dt, sys_rhs=sys_._state_dyn,
                           sys_out=sys_.out, state_sys=x0, stage_obj_pars=[R1], actor_opt="sampling", n_candidates=128, rounds=3,
                           seed=3)
        sim = Simulator(sys_type="diff_eqn", closed_loop_rhs=sys_.closed_loop_rhs, sys_out=sys_.out, state_init=x0, t0=0, t1=100,
                        dt=dt, max_step=dt / 10, first_step=1e-6, atol=1e-5, rtol=1e-3, is_disturb=0, is_dyn_ctrl=0)
        a_init = np.array(ctrl.action_curr, dtype=float)
        np.testing.assert_array_equal(a_init, BND[:, 0] / 10)
        decisions = 0
        for k in range(50):
            sim.sim_step()
            t, x, y, _ = sim.get_sim_step_data()
            if decide:
                a = ctrl.compute_action(t, y)
                ll = ctrl._eng_raw.last_launch()
                assert ll["kernel"] == "k_actor_search", (k, ll)
                assert ctrl._search_draw == k + 1 and ctrl.last_idx is not None  # one launch per decision
                assert BND[0, 0] <= a[0] <= BND[0, 1]
                decisions += 1
            else:
                a = a_init
            sys_.receive_action(a)
            ctrl.receive_sys_state(sys_._state)
            ctrl.upd_accum_obj(y, a)
        return float(ctrl.accum_obj_val), decisions

    J_search, n = loop(True)
    J_held, _ = loop(False)
    print(f"accumulated cost: search {J_search:.4f}, action_init held {J_held:.4f}")
    assert n == 50 and J_search < J_held


# ---- 6. quality against the reference ----------------------------------------------------------------------------------------
def test_search_quality_vs_reference_slsqp_on_f14():
    """F14 (b): the 16 decisions SLSQP made for the pendulum with the output map.  Six rounds of 256 device-generated candidates
    against the stored SLSQP costs.  The bound is measured, not chosen: the CPU replay of the same search - the oracle's own
    candidates (oracle/search_oracle.py::candidates_sample, seed 0) and the restatement - ends at most 0.336 % above SLSQP's cost
    (F14_SEARCH_GAP, pinned by test_user_system_search_register.py::test_f14_search_gap_on_the_cpu_replay); the device must stay
    within twice that gap (its float32 normals differ from the oracle's by up to 1e-5 sigma per candidate)."""
    meta, z = load_f14()
    x = z["b_state"]
    sid = _out_policy()["sys_id"]
    eng = _engine(sid, "f64", len(x), meta["Nactor"], z["b_R1"], h=meta["pred_step_size"], seed=0)
    eng.set_state(x)
    act, U, J, bi = eng.actor_search(K=256, rounds=6)
    assert np.all(J <= z["b_J_init"] * (1 + 1e-12))
    gap = J / z["b_J_opt"] - 1
    print(f"\nsearch on F14: J / J_slsqp - 1 median {np.median(gap):.5f} max {np.max(gap):.5f} (CPU replay: {F14_SEARCH_GAP:.5f})")
    assert np.max(gap) <= 2 * F14_SEARCH_GAP
    eng.close()


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------
def test_search_refusals():
    from rcognita_amd import _native as N

    from tests.test_hip_user_system_critic import _engine as critic_engine
    from tests.test_hip_user_system_critic import _pendulum as critic_pendulum

    meta, _ = load_f15()
    B = 64
    # a CRITIC policy without SEARCH, in RQL: both entry points refuse and nothing moves
    e = critic_engine(critic_pendulum()["sys_id"], "f64", B, meta, "RQL", "quad-nomix")
    e.set_state(np.random.default_rng(4).uniform(-1, 1, (B, 2)))
    fields = {f: e.get_field(f).copy() for f in (N.FIELD_STATE, N.FIELD_STEP_IDX, N.FIELD_W_CRITIC, N.FIELD_OBS_BUF, N.FIELD_ACT_BUF)}
    L = N.lib()
    for what, call in (("actor_search", lambda: L.rcg_actor_search(e._h, 64, 2, None, None, None, None, None, None, None)),
                       ("control_tick_search", lambda: L.rcg_control_tick_search(e._h, 64, 2, 0))):
        assert call() == N.ERR_UNSUPPORTED, what
        assert "SEARCH" in N.last_error(e._h), what
        for f, v in fields.items():
            assert np.array_equal(e.get_field(f), v), (what, f)
    e.close()
    # a SEARCH policy: the entry points' own argument checks
    e = _engine(_out_policy()["sys_id"], "f64", B, 5, np.diag(meta["R1"]))
    x0 = np.random.default_rng(5).uniform(-1, 1, (B, 2))
    e.set_state(x0)
    for kw in (dict(K=32, rounds=2), dict(K=128, rounds=0)):
        with pytest.raises(N.NativeError) as ei:
            e.control_tick_search(**kw)
        assert ei.value.code == N.ERR_BAD_ARG
        with pytest.raises(N.NativeError) as ei:
            e.actor_search(**kw)
        assert ei.value.code == N.ERR_BAD_ARG
    np.testing.assert_array_equal(e.get_state(), x0)
    np.testing.assert_array_equal(e.get_field(N.FIELD_STEP_IDX), np.zeros(B, np.int32))
    e.close()
    # RQL search needs CRITIC as well: rcg_create refuses the mode for a SEARCH policy without it
    with pytest.raises(N.NativeError) as ei:
        _engine(_out_policy()["sys_id"], "f64", B, 5, np.diag(meta["R1"]), mode="RQL", buffer_size=6)
    assert ei.value.code == N.ERR_UNSUPPORTED
