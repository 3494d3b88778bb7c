"""Every tick path of a handle with the disturbance model (RCG_FLAG_DISTURB) against an independent closed-loop oracle (GPU).

The oracle's disturbed loop is a composition: ``rcg_oracle.control_tick(..., sim=disturb_oracle.stepper(dcfg))`` - the undisturbed
tick with the disturbed env step (pinned alone by tests/test_hip_disturb.py) in place of the plain one.  tests/test_disturb_oracle.py
asserts on the CPU, for the seeds and shapes used here, that the oracle's best-to-second gap clears the tolerances (so ``ties == 0``
is a fair demand of the float64 runs) and that the disturbance moves the loop at all.

  a  rcg_control_tick (grid, k_actor_dma, k_actor_dma_packed; MPC with and without ref_lag, RQL, SQL): float64 free-running, float32
     every tick as a map (oracle/parity.py); the disturbance state to the same tolerance, the noise counter bit for bit
  b  T ticks in one launch (k_ticks, generated and streamed): float64 against T oracle ticks; float32 against its own single ticks
     bit for bit, those single ticks checked against the oracle tick by tick in the same test
  c  accum_every_substep with three substeps, an observation target, per-env parameters
  d  rcg_control_tick_opt / _search / _nominal, the structure of their undisturbed tests with the stepper on the oracle side; the
     search's candidate stream does not move with the noise (another key of the same seed)
  e  counter and step-length invariants: n substeps in one call = n calls, rcg_sim_step_h, the episode-1 stream after a reset
  f  the freeze rule, by the three-handle method of tests/test_hip_freeze_paths.py (its Trio): a finite state with an overflowing
     DISTURBANCE freezes its env and nobody else's - nothing is written, the noise counter included

Every test asserts the kernels it claims through rcg_last_launch.  ``REPORT_DISTURB=1 pytest -s`` prints the worst error per path and
dtype (kept as profiles/disturb_closed_loop.txt).  B <= 150, K <= 128, T <= 6 throughout.  Measured on an MI355X: the whole file
(113 cases) in 1.7 s, the slowest case 0.2 s (the first one, which brings the device up).  No path disagreed with the oracle and no
kernel was changed."""
import dataclasses
import os

import numpy as np
import pytest

from oracle import disturb_oracle as DO
from oracle import nominal_oracle as NO
from oracle import parity as PAR
from oracle import rcg_oracle as O
from oracle import search_oracle as S
from tests import disturb_closed_loop_inputs as I
from tests.helpers import PRESETS, TOL, assert_kernel, both, oracle_cfg, rand_actions, rand_states, rel_err_norm
from tests.test_freeze_states import REAL
from tests.test_hip_freeze_paths import Trio, _same

pytestmark = pytest.mark.gpu

DTYPES = ["f64", "f32"]
WORST = {}  # (path, dtype) -> {quantity: worst error}


def _note(path, dtype, errs):
    w = WORST.setdefault((path, dtype), {})
    for k, v in errs.items():
        w[k] = max(w.get(k, 0.0), float(v))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if os.environ.get("REPORT_DISTURB"):
        for (path, dtype), w in sorted(WORST.items()):
            print(f"\n[disturb] {path:<28} {dtype}  " + "  ".join(f"{k} {v:.2e}" for k, v in sorted(w.items())), end="")
        print()


def _make(name, B, dtype, x0, pars=None, dist=None, **kw):
    """(engine, oracle cfg, oracle env with its disturbance state, DisturbCfg) of one disturbed case."""
    from rcognita_amd import _native as N

    eng, cfg = both(name, B, dtype, engine_only=dict(I.DIST if dist is None else dist), **kw)
    if pars is not None:
        eng.set_field(N.FIELD_PARS, pars)
    eng.set_state(x0)
    d = I.dcfg()
    env = O.new_batch(cfg, np.asarray(x0, dtype=np.float64), pars=pars)
    DO.attach(cfg, env, d)
    return eng, cfg, env, d


def _tols(dtype, critic):
    """The project's existing tolerances: MPC 1e-10 / TOL['f32'] (test_hip_parity.py), RQL / SQL 1e-9 with the weights at 1e-6 and
    best_J at 1e-7 / 1e-5 (test_hip_critic.py)."""
    if not critic:
        return (1e-10 if dtype == "f64" else TOL["f32"]), None
    return (1e-9 if dtype == "f64" else 1e-5), ({"w_critic": 1e-6, "best_J": 1e-7} if dtype == "f64" else None)


def _follow(eng, cfg, env, d, cand, dcand, K, T, dtype, critic, what, path):
    """T single ticks, each against the oracle: float64 free-running with no tie allowed, float32 every tick as a map."""
    from rcognita_amd import _native as N

    tol, over = _tols(dtype, critic)
    rep = PAR.TickReport()
    c64 = np.asarray(cand, dtype=np.float64)
    for t in range(T):
        eng.control_tick(dcand, K=K)
        env = PAR.check_tick(cfg, env, c64, PAR.device_fields(eng, N, with_prev=True, critic=critic, disturb=True), tol=tol,
                             tol_over=over, report=rep, resync=dtype == "f32", what=f"{what} t={t}", sim=DO.stepper(d))
    assert rep.ticks == T
    if dtype == "f64":
        assert rep.ties == 0, rep.as_dict()
    _note(path, dtype, rep.worst)
    return env


def _case_id(c):
    return f"{c[0]}-K{c[1]}-{'streamed' if c[2] else 'grid'}"


# ---------------------------------------------------------------------------------------------------------------------
# a. rcg_control_tick
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tag,kw", I.MODE_KW, ids=[t for t, _ in I.MODE_KW])
@pytest.mark.parametrize("name,K,streamed,kernel", I.TICK_CASES, ids=[_case_id(c) for c in I.TICK_CASES])
def test_control_tick_with_the_disturbance_model_vs_oracle(name, K, streamed, kernel, tag, kw, dtype):
    from rcognita_amd import _native as N

    critic = not tag.startswith("MPC")
    kws = dict(n_actor=I.NH_A, substeps_per_tick=I.S_A, **kw)
    x0, cand = I.tick_inputs(name, K, streamed, real=REAL[dtype], cfg=oracle_cfg(name, **kws), seed_off=I.seed_off(name, K, tag))
    eng, cfg, env, d = _make(name, I.B_A, dtype, x0, **kws)
    dcand = eng.to_device(cand) if streamed else None
    _follow(eng, cfg, env, d, cand, dcand, K, I.T_A, dtype, critic, f"{name} K={K} {tag} {dtype}", f"control_tick {tag}")
    assert_kernel(eng, "k_sim_dist", kind=N.KERNEL_SIM)
    if critic:  # the unfused branch of the critic phase: k_sim_dist, then the push and the fit without an env step
        v = assert_kernel(eng, "k_critic_fit", kind=N.KERNEL_CRITIC)["variant"]
        assert not (v & 256) and (v & 512), v
        assert not np.allclose(eng.get_field(N.FIELD_W_CRITIC), 1.0)
    else:
        ll = assert_kernel(eng, kernel)
        if kernel == "k_actor":
            assert not (ll["variant"] & 4), ll
        if kernel == "k_actor_dma_packed":
            assert not (ll["variant"] & 16), ll  # no fused env step under the disturbance model
    np.testing.assert_array_equal(eng.get_field(N.FIELD_SUBSTEP_IDX), np.full(I.B_A, I.S_A * I.T_A, np.int32))
    np.testing.assert_array_equal(eng.get_field(N.FIELD_STEP_IDX), np.full(I.B_A, I.T_A, np.int32))
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# b. T ticks in one launch
# ---------------------------------------------------------------------------------------------------------------------
TICK_FIELDS = ["FIELD_STATE", "FIELD_STATE_PREV", "FIELD_ACTION", "FIELD_ACCUM", "FIELD_STEP_IDX", "FIELD_STATUS", "FIELD_BEST_J",
               "FIELD_BEST_IDX", "FIELD_DISTURB", "FIELD_SUBSTEP_IDX"]


def _free_run_errors(eng, env, N):
    """A float64 handle against the oracle env after the same number of free-running ticks."""
    errs = {
        "state": rel_err_norm(eng.get_state(), env.state),
        "state_prev": rel_err_norm(eng.get_field(N.FIELD_STATE_PREV), env.state_prev),
        "action": rel_err_norm(eng.get_field(N.FIELD_ACTION), env.action),
        "best_J": rel_err_norm(eng.get_field(N.FIELD_BEST_J), env.best_J),
        "accum": rel_err_norm(eng.get_field(N.FIELD_ACCUM), env.accum, floor=max(float(np.max(np.abs(env.accum))), 1e-30)),
        "disturb": rel_err_norm(eng.get_field(N.FIELD_DISTURB), env.disturb, floor=1.0),
    }
    np.testing.assert_array_equal(eng.get_field(N.FIELD_BEST_IDX), env.best_idx)
    np.testing.assert_array_equal(eng.get_field(N.FIELD_STEP_IDX), env.step_idx)
    np.testing.assert_array_equal(eng.get_field(N.FIELD_SUBSTEP_IDX), env.substep_idx)
    return errs


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,K,streamed", I.TICKS_CASES, ids=[_case_id(c) for c in I.TICKS_CASES])
def test_T_ticks_in_one_launch_with_the_disturbance_model_vs_oracle(name, K, streamed, dtype):
    from rcognita_amd import _native as N

    B, T = I.B_B, I.T_B
    x0, cand = I.tick_inputs(name, K, streamed, B=B, Nh=I.NH_B, real=REAL[dtype], cfg=oracle_cfg(name, **I.TICKS_KW))
    many, cfg, env, d = _make(name, B, dtype, x0, **I.TICKS_KW)
    dc = many.to_device(cand) if streamed else None
    if streamed:
        many.control_tick(dc, K=K, T=T)
    else:
        many.control_ticks(T, K)
    ll = assert_kernel(many, "k_ticks")
    assert bool(ll["variant"] & 4) == streamed and not (ll["variant"] & 8), ll
    path = f"T ticks {'streamed' if streamed else 'grid'}"
    if dtype == "f64":
        c64 = np.asarray(cand, dtype=np.float64)
        for _ in range(T):
            O.control_tick(cfg, env, c64, sim=DO.stepper(d))
        errs = _free_run_errors(many, env, N)
        _note(path, dtype, errs)
        for k, v in errs.items():
            assert v <= 1e-10, f"{k} differs from the oracle by {v:.3e} after {T} ticks in one launch"
    else:  # no per-tick resync inside one launch: the handle's own single ticks, which are held to the oracle tick by tick here
        one, _, env1, _ = _make(name, B, dtype, x0, **I.TICKS_KW)
        _follow(one, cfg, env1, d, cand, one.to_device(cand) if streamed else None, K, T, dtype, False, f"{name} K={K} single ticks",
                path + " (single ticks)")
        assert_kernel(one, "k_sim_dist", kind=N.KERNEL_SIM)
        assert one.last_launch(N.KERNEL_ACTOR)["kernel"] != "k_ticks"
        for f in TICK_FIELDS:
            _same(many.get_field(getattr(N, f)), one.get_field(getattr(N, f)), f)
        one.close()
    np.testing.assert_array_equal(many.get_field(N.FIELD_SUBSTEP_IDX), np.full(B, I.S_B * T, np.int32))
    assert not many.get_field(N.FIELD_STATUS).any()
    many.close()


# ---------------------------------------------------------------------------------------------------------------------
# c. corners
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which", list(I.CORNERS))
def test_corner_under_the_disturbance_model_vs_oracle(which, dtype):
    from rcognita_amd import _native as N

    real = REAL[dtype]
    name, kw, x0, pars = I.corner_inputs(which, real=real)
    if pars is not None:
        pars = pars.astype(real).astype(np.float64)
    eng, cfg, env, d = _make(name, I.B_C, dtype, x0, pars=pars, **kw)
    cand = O.grid_candidates(cfg, I.K_C)
    _follow(eng, cfg, env, d, cand, None, I.K_C, I.T_C, dtype, False, f"{which} {dtype}", f"corner {which}")
    assert_kernel(eng, "k_sim_dist", kind=N.KERNEL_SIM)
    assert_kernel(eng, "k_actor")
    np.testing.assert_array_equal(eng.get_field(N.FIELD_SUBSTEP_IDX), np.full(I.B_C, cfg.substeps_per_tick * I.T_C, np.int32))
    if which == "accum_every_substep":  # charged once per substep, with the held action
        assert cfg.substeps_per_tick == 3 and np.all(eng.get_field(N.FIELD_ACCUM) > 0)
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# d. the optimiser, the search and the nominal controller as the decision
# ---------------------------------------------------------------------------------------------------------------------
def _resync(env, eng, N, critic=False):
    env.state = eng.get_state().astype(np.float64)
    env.state_prev = eng.get_field(N.FIELD_STATE_PREV).astype(np.float64)
    env.action = eng.get_field(N.FIELD_ACTION).astype(np.float64)
    env.accum = eng.get_field(N.FIELD_ACCUM).astype(np.float64)
    env.disturb = eng.get_field(N.FIELD_DISTURB).astype(np.float64)
    if critic:
        for k, f in (("w_critic", N.FIELD_W_CRITIC), ("w_prev", N.FIELD_W_PREV), ("obs_buf", N.FIELD_OBS_BUF), ("act_buf", N.FIELD_ACT_BUF)):
            setattr(env, k, eng.get_field(f).astype(np.float64))


def _check_disturb(eng, env, N, what):
    e = rel_err_norm(eng.get_field(N.FIELD_DISTURB), env.disturb, floor=1.0)
    assert e < 1e-10, f"{what}: disturbance state differs by {e:.3e}"
    np.testing.assert_array_equal(eng.get_field(N.FIELD_SUBSTEP_IDX), env.substep_idx, err_msg=what)
    return e


CRITIC_KW = dict(critic_struct=O.CRITIC_QUAD_NOMIX, n_critic=4, buffer_size=6, gamma=0.95)


@pytest.mark.parametrize("name,mode", [("3wrobot", "MPC"), ("3wrobotNI", "RQL")])
def test_control_tick_opt_with_the_disturbance_model_vs_oracle(name, mode):
    """test_control_tick_opt_closed_loop_vs_oracle with the disturbed step on both sides (float64, every tick as a map)."""
    from rcognita_amd import _native as Nn

    rng = np.random.default_rng(31)
    B, T, critic = 9, 4, mode != "MPC"
    kw = dict(n_actor=6 if not critic else 4, substeps_per_tick=2, gamma=0.98)
    if critic:
        kw.update(mode=O.MODE_IDS[mode], **CRITIC_KW)
    x0 = rand_states(rng, name, B) * (0.5 if critic else 1.0)
    eng, cfg, env, d = _make(name, B, "f64", x0, **kw)
    for t in range(T):
        eng.control_tick_opt(iters=6, warm_start=True)
        O.control_tick_opt(cfg, env, 6, warm_start=True, sim=DO.stepper(d))
        assert_kernel(eng, "k_actor_opt")
        assert_kernel(eng, "k_sim_dist", kind=Nn.KERNEL_SIM)
        errs = {"state": rel_err_norm(eng.get_state(), env.state), "disturb": _check_disturb(eng, env, Nn, f"opt t={t}")}
        assert errs["state"] < 1e-9, t
        if critic:
            ew = rel_err_norm(eng.get_field(Nn.FIELD_W_CRITIC), env.w_critic)
            assert ew < 1e-6, (t, ew)
            errs["w_critic"] = ew
            # pushed after the step: the new observation and the action held over it (the oracle's rows, not the device's)
            errs["obs_buf"] = rel_err_norm(eng.get_field(Nn.FIELD_OBS_BUF), env.obs_buf)
            errs["act_buf"] = rel_err_norm(eng.get_field(Nn.FIELD_ACT_BUF), env.act_buf)
            assert errs["obs_buf"] < 1e-9 and errs["act_buf"] < 1e-9, (t, errs)
        assert np.all(np.abs(eng.get_field(Nn.FIELD_BEST_IDX) - env.best_idx) <= 3)  # iterations used
        errs["best_J"] = rel_err_norm(eng.get_field(Nn.FIELD_BEST_J), env.best_J)
        errs["action_sqn"] = rel_err_norm(eng.get_field(Nn.FIELD_ACTION_SQN), env.action_sqn, floor=float(np.max(cfg.ctrl_bnds)))
        errs["accum"] = rel_err_norm(eng.get_field(Nn.FIELD_ACCUM), env.accum, floor=float(np.max(np.abs(env.accum))))
        assert errs["best_J"] < 1e-7 and errs["action_sqn"] < 1e-4 and errs["accum"] < 1e-6, (t, errs)
        np.testing.assert_array_equal(eng.get_field(Nn.FIELD_STEP_IDX), env.step_idx)
        _note(f"control_tick_opt {mode}", "f64", errs)
        _resync(env, eng, Nn, critic)
        env.action_sqn = eng.get_field(Nn.FIELD_ACTION_SQN).astype(np.float64)
    np.testing.assert_array_equal(eng.get_field(Nn.FIELD_SUBSTEP_IDX), np.full(B, 2 * T, np.int32))
    eng.close()


def test_control_tick_search_with_the_disturbance_model_vs_oracle():
    """test_control_tick_search_closed_loop_vs_oracle on a disturbed handle: the oracle's side of the tick steps with
    disturb_oracle.sim_substeps.  The candidate stream shares the handle's seed with the noise under another key: a disturbed and
    an undisturbed handle with the same seed, env ids, EPISODE_IDX and STEP_IDX draw the same candidates, bit for bit."""
    from rcognita_amd import _native as N

    rng = np.random.default_rng(12)
    name, B, K, Nh, rounds, T = "3wrobot", 9, 128, 5, 2, 4
    x0 = rand_states(rng, name, B) * 0.4
    eng, cfg, env, d = _make(name, B, "f64", x0, n_actor=Nh, substeps_per_tick=2)
    plain, _ = both(name, B, "f64", n_actor=Nh, substeps_per_tick=2, engine_only=dict(seed=I.SEED, env_id_base=I.ENV_ID_BASE))
    ids = I.ENV_ID_BASE + np.arange(B)
    sampler = lambda r, centre: eng.candidates_sample(K, round=r, centre=centre.astype(eng.real)).astype(np.float64)  # noqa: E731
    prev = None
    for t in range(T):
        step_before = eng.get_field(N.FIELD_STEP_IDX).copy()
        DO.sim_substeps(cfg, env, d, cfg.substeps_per_tick)
        eng.control_tick_search(K=K, rounds=rounds, warm_start=True)
        assert_kernel(eng, "k_actor_search")
        assert_kernel(eng, "k_sim_dist", kind=N.KERNEL_SIM)
        es = rel_err_norm(eng.get_state(), env.state)
        assert es < 1e-9, t
        ed = _check_disturb(eng, env, N, f"search t={t}")
        centre = None if prev is None else np.concatenate([prev[:, 1:], prev[:, -1:]], axis=1)
        eng.set_field(N.FIELD_STEP_IDX, step_before)  # the candidates of this tick were drawn at STEP_IDX = step_before
        plain.set_field(N.FIELD_STEP_IDX, step_before)
        for r in range(rounds):
            ce = O.action_sqn_init(cfg) if centre is None else centre
            ce = np.broadcast_to(ce, (B, Nh, cfg.du))
            _same(eng.candidates_sample(K, round=r, centre=ce), plain.candidates_sample(K, round=r, centre=ce), f"candidates t={t} round {r}")
        U_or, J_or, bi_or = S.actor_search(cfg, env.state, env.state, K, rounds, I.SEED, ids, np.zeros(B, int), step_before,
                                           centre=centre, sampler=sampler)
        eng.set_field(N.FIELD_STEP_IDX, step_before + 1)
        U = eng.get_field(N.FIELD_ACTION_SQN)
        np.testing.assert_array_equal(eng.get_field(N.FIELD_BEST_IDX), bi_or)
        np.testing.assert_array_equal(U, U_or)
        ej = rel_err_norm(eng.get_field(N.FIELD_BEST_J), J_or)
        assert ej < 1e-10
        np.testing.assert_array_equal(eng.get_field(N.FIELD_ACTION), U[:, 0, :])
        env.action = U[:, 0, :].astype(np.float64)
        env.accum = env.accum + O.stage_obj(env.state, env.action, cfg) * cfg.sampling_time
        ea = rel_err_norm(eng.get_field(N.FIELD_ACCUM), env.accum, floor=float(np.max(np.abs(env.accum)) + 1e-9))
        assert ea < 1e-9
        _note("control_tick_search MPC", "f64", {"state": es, "disturb": ed, "best_J": ej, "accum": ea})
        env.tick_count += 1
        env.state = eng.get_state().astype(np.float64)
        env.state_prev = eng.get_field(N.FIELD_STATE_PREV).astype(np.float64)
        env.disturb = eng.get_field(N.FIELD_DISTURB).astype(np.float64)
        prev = U.astype(np.float64)
    np.testing.assert_array_equal(eng.get_field(N.FIELD_STEP_IDX), np.full(B, T, np.int32))
    np.testing.assert_array_equal(eng.get_field(N.FIELD_SUBSTEP_IDX), np.full(B, 2 * T, np.int32))
    for e in (eng, plain):
        e.close()


def test_control_tick_nominal_with_the_disturbance_model_vs_oracle():
    """test_control_tick_nominal_vs_oracle (the kinematic robot's closed-form law) with the disturbed step on both sides."""
    from rcognita_amd import _native as N

    rng = np.random.default_rng(5)
    name, gain, B, T = "3wrobotNI", 0.5, 37, 4
    x0 = rand_states(rng, name, B)
    eng, cfg, env, d = _make(name, B, "f64", x0, substeps_per_tick=2)
    for t in range(T):
        eng.control_tick_nominal(gain)
        NO.control_tick_nominal(cfg, env, gain, 10.0, 1.0, sim=DO.stepper(d))
        assert_kernel(eng, "k_nominal")
        assert_kernel(eng, "k_sim_dist", kind=N.KERNEL_SIM)
        a = eng.get_field(N.FIELD_ACTION)
        es = rel_err_norm(eng.get_state(), env.state)
        assert es < 1e-9
        ed = _check_disturb(eng, env, N, f"nominal t={t}")
        assert np.all(np.abs(a - env.action) <= 1e-9 * (np.abs(env.action) + 1)), t
        ea = rel_err_norm(eng.get_field(N.FIELD_ACCUM), env.accum, floor=float(np.max(np.abs(env.accum))))
        assert ea < 1e-9
        np.testing.assert_array_equal(eng.get_field(N.FIELD_STEP_IDX), env.step_idx)
        _note("control_tick_nominal", "f64", {"state": es, "disturb": ed, "accum": ea, "action": rel_err_norm(a, env.action)})
    assert np.max(np.abs(env.disturb - np.array(I.DISTURB_INIT))) > 0.05
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# e. counter and step-length invariants
# ---------------------------------------------------------------------------------------------------------------------
B_E = 41
SIM_FIELDS = ["FIELD_STATE", "FIELD_STATE_PREV", "FIELD_DISTURB", "FIELD_SUBSTEP_IDX", "FIELD_STATUS"]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["3wrobot", "3wrobotNI", "2tank"])
def test_six_substeps_in_one_call_equal_six_calls(name, dtype):
    from rcognita_amd import _native as N

    rng = np.random.default_rng(6)
    x0 = rand_states(rng, name, B_E)
    u = rand_actions(rng, name, (B_E,), overshoot=1.3)
    a, _, _, _ = _make(name, B_E, dtype, x0)
    b, _, _, _ = _make(name, B_E, dtype, x0)
    for e in (a, b):
        e.set_field(N.FIELD_ACTION, u)
    a.sim_step(6)
    for _ in range(6):
        b.sim_step(1)
    for e in (a, b):
        assert_kernel(e, "k_sim_dist", kind=N.KERNEL_SIM)
    for f in SIM_FIELDS:
        _same(a.get_field(getattr(N, f)), b.get_field(getattr(N, f)), f)
    np.testing.assert_array_equal(a.get_field(N.FIELD_SUBSTEP_IDX), np.full(B_E, 6, np.int32))
    for e in (a, b):
        e.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["3wrobot", "3wrobotNI"])
def test_sim_step_of_a_given_length_vs_oracle_and_dt_sim_is_restored(name, dtype):
    """rcg_sim_step_h(3, h) = three oracle substeps of h / 3, the noise counter advancing by 3; the handle's own dt_sim is back for
    the next rcg_sim_step.  Each call as a map from the device's values."""
    from rcognita_amd import _native as N

    rng = np.random.default_rng(9)
    real = REAL[dtype]
    x0 = rand_states(rng, name, B_E).astype(real)
    u = rand_actions(rng, name, (B_E,), overshoot=1.3).astype(real)
    eng, cfg, env, d = _make(name, B_E, dtype, x0)
    eng.set_field(N.FIELD_ACTION, u)
    env.action = u.astype(np.float64)
    h = 0.045
    tol = 1e-10 if dtype == "f64" else TOL["f32"]
    cfg_h = dataclasses.replace(cfg, dt_sim=h / 3)
    for what, call, c, n in (("sim_step_h", lambda: eng.sim_step(3, step=h), cfg_h, 3), ("sim_step after it", lambda: eng.sim_step(1), cfg, 1)):
        call()
        assert_kernel(eng, "k_sim_dist", kind=N.KERNEL_SIM)
        DO.sim_substeps(c, env, d, n)
        errs = {"state": rel_err_norm(eng.get_state(), env.state),
                "state_prev": rel_err_norm(eng.get_field(N.FIELD_STATE_PREV), env.state_prev),
                "disturb": rel_err_norm(eng.get_field(N.FIELD_DISTURB), env.disturb, floor=1.0)}
        _note(what, dtype, errs)
        for k, v in errs.items():
            assert v <= tol, f"{what}: {k} differs from the oracle by {v:.3e}"
        np.testing.assert_array_equal(eng.get_field(N.FIELD_SUBSTEP_IDX), env.substep_idx)
        env.state = eng.get_state().astype(np.float64)
        env.disturb = eng.get_field(N.FIELD_DISTURB).astype(np.float64)
    np.testing.assert_array_equal(eng.get_field(N.FIELD_SUBSTEP_IDX), np.full(B_E, 4, np.int32))
    # the two step lengths are told apart: the oracle at the configured step from the same inputs is elsewhere
    assert h / 3 != cfg.dt_sim
    eng.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["3wrobot", "3wrobotNI"])
def test_ticks_after_an_episode_reset_follow_the_oracles_episode_1_stream(name, dtype):
    from rcognita_amd import _native as N

    K, Nh = 16, 5
    kws = dict(n_actor=Nh, substeps_per_tick=2)
    x0, cand = I.tick_inputs(name, K, False, B=B_E, Nh=Nh, real=REAL[dtype], cfg=oracle_cfg(name, **kws), seed_off=5)
    eng, cfg, env, d = _make(name, B_E, dtype, x0, **kws)
    env = _follow(eng, cfg, env, d, cand, None, K, 2, dtype, False, f"{name} episode 0", "episode 0")
    q0 = eng.get_field(N.FIELD_DISTURB).copy()
    eng.episode_reset()
    DO.episode_reset(cfg, env, d, np.asarray(x0, dtype=np.float64))
    np.testing.assert_array_equal(eng.get_field(N.FIELD_DISTURB), np.tile(np.array(I.DISTURB_INIT, dtype=eng.real), (B_E, 1)))
    np.testing.assert_array_equal(eng.get_field(N.FIELD_SUBSTEP_IDX), np.zeros(B_E, np.int32))
    np.testing.assert_array_equal(eng.get_field(N.FIELD_EPISODE_IDX), env.episode_idx)
    if dtype == "f32":  # as a map: the oracle's accum / returns bookkeeping restarts from the device's values too
        env.accum = eng.get_field(N.FIELD_ACCUM).astype(np.float64)
    # (the first two ticks of episode 1 leave another disturbance than those of episode 0 did: the stream moved on)
    env = _follow(eng, cfg, env, d, cand, None, K, 2, dtype, False, f"{name} episode 1", "after episode_reset")
    assert not np.array_equal(eng.get_field(N.FIELD_DISTURB), q0)
    _follow(eng, cfg, env, d, cand, None, K, 3, dtype, False, f"{name} episode 1", "after episode_reset")
    np.testing.assert_array_equal(eng.get_field(N.FIELD_SUBSTEP_IDX), np.full(B_E, 10, np.int32))
    np.testing.assert_array_equal(eng.get_field(N.FIELD_STEP_IDX), np.full(B_E, 5, np.int32))
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# f. the freeze rule on the disturbed paths
# ---------------------------------------------------------------------------------------------------------------------
S_F = 2
DIST_F = dict(I.DIST, pars_disturb=[[30.0, 10.0], [0.5, -0.2], [10.0, 10.0]])  # tau = 10: -tau (q + ...) overflows in the first stage
HUGE = {"f64": 1e308, "f32": 3e38}
DIST_FIELDS = ["FIELD_DISTURB", "FIELD_SUBSTEP_IDX"]


class DistTrio(Trio):
    """The three handles of tests/test_hip_freeze_paths.py with the disturbance model on.  The bad-now envs (0, 7, 63, 64, B - 1)
    hold a FINITE state - the clean batch's - and a disturbance that overflows inside the first RK4 stage; the NaN-on-entry env
    and the env whose STATUS the caller presets are the base class's."""

    def __init__(self, name, dtype, **kw):
        from rcognita_amd import _native as N

        super().__init__(name, dtype, engine_only=DIST_F, substeps_per_tick=S_F, **kw)
        self.x_bad[self.now] = self.x_clean[self.now]
        dd = DO.DIM_DISTURB[self.cfg.sys_id]
        self.q_clean = np.tile(np.array(I.DISTURB_INIT[:dd]), (self.B, 1))
        self.q_bad = self.q_clean.copy()
        self.q_bad[self.now] = HUGE[dtype]
        assert np.all(np.isfinite(self.q_bad.astype(self.real))) and np.all(np.isfinite(self.x_bad[self.now]))
        for which in ("bad", "pre"):
            self.h[which].set_state(self.x_bad, also_init=False)
            self.h[which].set_field(N.FIELD_DISTURB, self.q_bad)
        self.fields = self.fields + DIST_FIELDS

    def check(self, ticks, what, extra=(), stepped=None):
        """P1 + P2 on every field, and the frozen envs themselves: nothing written (the noise counter included), flagged, counted."""
        got = self.check_isolation(fields=self.fields + list(extra), what=what)
        fz = self.frozen
        x_set, q_set = self.x_bad.astype(self.real), self.q_bad.astype(self.real)
        _same(got["FIELD_STATE"][fz], x_set[fz], f"{what}: STATE of a frozen env moved")
        _same(got["FIELD_STATE_PREV"][fz], x_set[fz], f"{what}: STATE_PREV of a frozen env moved")
        _same(got["FIELD_DISTURB"][fz], q_set[fz], f"{what}: DISTURB of a frozen env moved")
        sub = np.full(self.B, S_F * ticks if stepped is None else stepped, np.int32)
        sub[fz] = 0
        np.testing.assert_array_equal(got["FIELD_SUBSTEP_IDX"], sub, err_msg=f"{what}: SUBSTEP_IDX (a frozen env's must not advance)")
        want = np.zeros(self.B, np.uint32)
        want[fz] = 1
        np.testing.assert_array_equal(got["FIELD_STATUS"], want, err_msg=f"{what}: STATUS")
        healthy = np.setdiff1d(np.arange(self.B), fz)
        assert np.all(np.isfinite(got["FIELD_STATE"][healthy])) and np.all(np.any(got["FIELD_STATE"][healthy] != x_set[healthy], axis=1))
        return got

    def check_decided(self, ticks, cand, K, got):
        """P3 of tests/test_hip_freeze_paths.py for envs frozen with a finite state: decided for from the frozen state
        (= rcg_actor_argmin on a fresh handle holding it), counted, charged once per tick with that decision."""
        from rcognita_amd import _native as N

        fz = self.frozen
        np.testing.assert_array_equal(got["FIELD_STEP_IDX"], np.full(self.B, ticks, np.int32), err_msg="STEP_IDX")
        ref = self.fresh()
        ref.set_field(N.FIELD_STATE, got["FIELD_STATE"])
        if self.critic:
            ref.set_field(N.FIELD_W_CRITIC, got["FIELD_W_CRITIC"])
        act, bj, bi = ref.actor_argmin(cand, K=K)
        _same(got["FIELD_ACTION"][fz], act[fz], "ACTION != rcg_actor_argmin from the frozen state")
        np.testing.assert_array_equal(got["FIELD_BEST_IDX"][fz], bi[fz], err_msg="BEST_IDX")
        np.testing.assert_allclose(got["FIELD_BEST_J"][fz], bj[fz], rtol=TOL[self.dtype])
        fin = np.array([i for i in fz if i != self.nan_at])
        if not self.critic:  # the same decision every tick: same state, same candidates
            stage = ref.stage_obj(got["FIELD_STATE"][fin], got["FIELD_ACTION"][fin])
            inc = (stage * self.real(self.cfg.sampling_time * (S_F if self.cfg.accum_every_substep else 1))).astype(self.real)
            acc = np.zeros(len(fin), self.real)
            for _ in range(ticks):
                acc = (acc + inc).astype(self.real)
            np.testing.assert_allclose(got["FIELD_ACCUM"][fin], acc, rtol=TOL[self.dtype], err_msg="ACCUM of a frozen env")
        assert np.all(got["FIELD_ACCUM"][fin] > 0)
        ref.close()


ROBOTS = ["3wrobot", "3wrobotNI"]
RQL_F = dict(mode=O.MODE_RQL, critic_struct=O.CRITIC_QUAD_NOMIX, n_critic=4, buffer_size=6)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ROBOTS)
def test_sim_step_with_an_overflowing_disturbance_freezes_alone(name, dtype):
    from rcognita_amd import _native as N

    t = DistTrio(name, dtype)
    u = rand_actions(np.random.default_rng(3), name, (t.B,))
    for e in t.h.values():
        e.set_field(N.FIELD_ACTION, u)
    t.run(lambda e: [e.sim_step(S_F) for _ in range(2)])  # the second call starts from the flag the first one set
    for e in t.h.values():
        assert_kernel(e, "k_sim_dist", kind=N.KERNEL_SIM)
    got = t.check(2, "sim_step")
    np.testing.assert_array_equal(got["FIELD_STEP_IDX"], 0)
    t.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", ["MPC", "RQL"])
@pytest.mark.parametrize("streamed", [False, True], ids=["grid", "streamed"])
@pytest.mark.parametrize("name", ROBOTS)
def test_disturbed_control_tick_freezes_alone(name, streamed, mode, dtype):
    from rcognita_amd import _native as N

    K, ticks = 16, 3
    t = DistTrio(name, dtype, **(RQL_F if mode == "RQL" else {}))
    cand = rand_actions(np.random.default_rng(K), name, (t.B, K, 5)).astype(t.real) if streamed else None
    t.run(lambda e: [e.control_tick(cand, K=K) for _ in range(ticks)])
    for e in t.h.values():
        assert_kernel(e, "k_sim_dist", kind=N.KERNEL_SIM)
        ll = e.last_launch(N.KERNEL_ACTOR)
        assert ll["kernel"] in ("k_actor", "k_actor_dma", "k_actor_dma_packed") and not (ll["kernel"] == "k_actor_dma_packed" and ll["variant"] & 16), ll
        if mode == "RQL":
            assert not (assert_kernel(e, "k_critic_fit", kind=N.KERNEL_CRITIC)["variant"] & 256)
    got = t.check(ticks, f"control_tick {mode}")
    t.check_decided(ticks, cand, K, got)
    if mode == "RQL":  # pushed: the frozen observation, once per tick
        bs = RQL_F["buffer_size"]
        for k in range(ticks):
            _same(got["FIELD_OBS_BUF"][t.frozen, bs - ticks + k], t.x_bad.astype(t.real)[t.frozen], f"pushed observation of tick {k}")
    t.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("streamed", [False, True], ids=["grid", "streamed"])
@pytest.mark.parametrize("name", ROBOTS)
def test_disturbed_T_ticks_in_one_launch_freeze_alone(name, streamed, dtype):
    K, T = 16, 3
    t = DistTrio(name, dtype)
    cand = rand_actions(np.random.default_rng(K + 1), name, (t.B, K, 5)).astype(t.real) if streamed else None
    t.run((lambda e: e.control_tick(cand, K=K, T=T)) if streamed else (lambda e: e.control_ticks(T, K)))
    for e in t.h.values():
        ll = assert_kernel(e, "k_ticks")
        assert bool(ll["variant"] & 4) == streamed, ll
    got = t.check(T, "T ticks in one launch")
    t.check_decided(T, cand, K, got)
    t.close()


def _check_action_in_bounds(t, got):
    b = np.array(PRESETS[t.name]["bnds"], dtype=float)
    a = got["FIELD_ACTION"][t.frozen].astype(np.float64)
    assert np.all(np.isfinite(a)) and np.all(a >= b[:, 0]) and np.all(a <= b[:, 1]), a


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("path", ["opt", "search", "nominal"])
@pytest.mark.parametrize("name", ROBOTS)
def test_disturbed_opt_search_and_nominal_ticks_freeze_alone(name, path, dtype):
    from rcognita_amd import _native as N

    ticks = 2
    t = DistTrio(name, dtype)
    go = {"opt": lambda e: [e.control_tick_opt(iters=4, warm_start=k > 0) for k in range(ticks)],
          "search": lambda e: [e.control_tick_search(K=64, rounds=2, warm_start=k > 0) for k in range(ticks)],
          "nominal": lambda e: [e.control_tick_nominal(0.5) for _ in range(ticks)]}[path]
    t.run(go)
    for e in t.h.values():
        assert_kernel(e, {"opt": "k_actor_opt", "search": "k_actor_search", "nominal": "k_nominal"}[path])
        assert_kernel(e, "k_sim_dist", kind=N.KERNEL_SIM)
    got = t.check(ticks, path, extra=[] if path == "nominal" else ["FIELD_ACTION_SQN"])
    np.testing.assert_array_equal(got["FIELD_STEP_IDX"], np.full(t.B, ticks, np.int32))
    fin = np.array([i for i in t.frozen if i != t.nan_at])
    assert np.all(got["FIELD_ACCUM"][fin] > 0)  # charged
    if path != "nominal":
        _check_action_in_bounds(t, got)
    t.close()


def test_an_infinite_disturbance_of_the_tank_does_not_reach_its_state():
    """Sys2Tank's disturbance is inert (systems.py:412-424): q = inf on one env leaves every state finite and every other env on
    the oracle's trajectory."""
    from rcognita_amd import _native as N

    B = 20
    x0 = rand_states(np.random.default_rng(2), "2tank", B)
    eng, cfg, env, d = _make("2tank", B, "f64", x0)
    q = np.full((B, 1), I.DISTURB_INIT[0])
    q[7] = np.inf
    eng.set_field(N.FIELD_DISTURB, q)
    eng.sim_step(2)
    DO.sim_substeps(cfg, env, d, 2)
    assert np.all(np.isfinite(eng.get_state()))
    ok = np.arange(B) != 7
    assert rel_err_norm(eng.get_state()[ok], env.state[ok]) < 1e-10
    assert not eng.get_field(N.FIELD_STATUS)[ok].any()
    eng.close()
