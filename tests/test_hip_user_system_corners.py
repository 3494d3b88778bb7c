"""Run-time-compiled systems at the corners of DS, DU, DY, NP, DD on the GPU (tests/user_systems.py):

    C1  DS 1, DU 1, NP 0, no output map, DD 1      smallest everything, NP = 0, dc = 2, 3, 5
    C2  DS 5, DU 2, NP 5, DY 1, DD 2               all maxima with the smallest output, DY << DS
    C3  DS 4, DU 2, NP 1, DY 2, DD 1               DS = 4, DY < DS, dc = 8 just under the four-lane fit
    C4  DS 3, DU 1, NP 4, DY 5, DD 2               DY = RCG_MAX_DS > DS, NP > DS, dc = 21, 27

Every kernel template a registered policy reaches, against the reference's own results (tests/golden/F17_user_system_corners.npz)
and the float64 NumPy restatement that test_user_system_corners.py pins on them.  Tolerances are the project's: operators and
costs 1e-11 / 1e-5 (rel_err_norm), right-hand sides 1e-12 / 2e-5, RK4 runs 1e-10 / 2e-4 (test_hip_user_system.py), ticks through
oracle/parity.py::check_tick as test_hip_user_system_critic.py runs them; "same bits" is equality of the bytes.  The kernel that
served a call is read from rcg_last_launch: no case passes on a fallback.

1. Operators: rcg_rhs, rcg_out, rcg_rhs_full, rcg_stage_obj.
2. Env step: k_sim, k_sim_dist with the cost charged at out(x) after every substep; a non-finite env freezes alone.
3. _actor_cost on every decision kernel, argmin with and without a caller's observation, REF_LAG.
4. Per-env parameters through a user's prepare(); NP = 0 with the flag set.
5. RQL / SQL x 4 structures: operators, closed-loop ticks with the fit, the fit form on either side of dc = 9.
6. The optimiser with jac_T + out_jac_T against SLSQP and (C1) the oracle's twin.
7. The device search on the device's own candidates.
8. T ticks per launch = T single ticks, bit for bit.
9. The mirror classes on C2.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.user_systems import (ARGMIN_SHAPES, KEYS, MPC_CASES, STRUCTS, actor_cost, argmin_gap, argmin_inputs,  # noqa: E402
                                case_cost, corner, dim_critic, f17_case, load_f17, oracle_cfg, restated_tick, search_inputs,
                                search_weights, sim_substeps, stage_b)

pytestmark = pytest.mark.gpu

TOL = {"f64": 1e-11, "f32": 1e-5}
RHS_TOL = {"f64": 1e-12, "f32": 2e-5}
RK4_TOL = {"f64": 1e-10, "f32": 2e-4}
DT_SIM = 0.01
FIT_ML, FIT_GEN = 1024, 2048  # rcg_last_launch's variant word of k_critic_fit: four lanes per env | the HBM-scratch form
FIELDS = ["FIELD_STATE", "FIELD_STATE_PREV", "FIELD_ACTION", "FIELD_ACCUM", "FIELD_STEP_IDX", "FIELD_STATUS", "FIELD_BEST_J",
          "FIELD_BEST_IDX"]
CRITIC_FIELDS = FIELDS + ["FIELD_W_CRITIC", "FIELD_W_PREV", "FIELD_OBS_BUF", "FIELD_ACT_BUF"]
DISTURB_FIELDS = FIELDS + ["FIELD_DISTURB", "FIELD_SUBSTEP_IDX"]


@pytest.fixture(scope="module")
def reg():
    """Each corner registered once per module."""
    return {k: corner(k).register() for k in KEYS}


def _engine(reg, key, dtype, B, Nh, R1, **kw):
    from rcognita_amd import Engine, EngineConfig

    meta, _ = load_f17()
    S = corner(key)
    cfg = dict(sys_id=reg[key]["sys_id"], batch=B, dtype=dtype, Nactor=Nh, pars=S.pars, ctrl_bnds=S.bnds, R1=R1, dt_sim=DT_SIM,
               sampling_time=meta["sampling_time"], pred_step_size=meta["pred_step_size"])
    cfg.update(kw)
    return Engine(EngineConfig(**cfg))


def _r(e):
    return lambda a: None if a is None else np.asarray(a).astype(e.real).astype(np.float64)


def _err(a, b):
    from tests.helpers import rel_err_norm

    return rel_err_norm(a, b)


def _row_err(J, J_ref):
    """Against the env's largest |J|: what an argmin over the row is sensitive to (signed critic weights make J a difference
    of large terms; tests/test_hip_critic.py measures it so)."""
    return float(np.max(np.abs(J - J_ref) / np.maximum(np.max(np.abs(J_ref), axis=1, keepdims=True), 1.0)))


def _note(group, key, dtype, what, err, ll=None):
    k = "" if ll is None else f" {ll['kernel']}/{ll['variant']}"
    print(f"corners {group} {key} {dtype} {what}{k}: {err:.3e}")


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


def _check_argmin(act, bj, bi, J_ref, cand, dtype, what, device_made=False):
    """The device's choice against the restated costs J_ref [B, K]: float64 - the index; float32 - the index wherever the env's
    best-to-second gap exceeds 4 x the tolerance, and elsewhere a near tie is followed: the chosen candidate's restated cost is
    within 4 x the tolerance of the best; the reported cost and action are the chosen candidate's."""
    from oracle import rcg_oracle as O

    tol = TOL[dtype]
    rows = np.arange(len(bi))
    Jb, ib = O.argmin_first(J_ref)
    scale = np.maximum(np.max(np.abs(J_ref), axis=1), 1.0)
    Jd = J_ref[rows, bi]
    if dtype == "f64":
        np.testing.assert_array_equal(bi, ib, err_msg=str(what))
    else:
        clear = argmin_gap(J_ref) > 4 * tol
        np.testing.assert_array_equal(bi[clear], ib[clear], err_msg=str(what))
    assert np.all(Jd - Jb <= 4 * tol * scale), (what, float(np.max((Jd - Jb) / scale)))
    err = float(np.max(np.abs(bj - Jd) / scale))
    assert err < tol, (what, err)
    if device_made:  # (the level grid lo + i * step, made on the device in its own width: float32 levels lie within one
        # unit in the last place of the range, 2^-23 (hi - lo) <= 1.2e-6, of the float64 levels - absolute, a level may be near zero)
        np.testing.assert_allclose(act, np.asarray(cand)[rows, bi, 0, :], rtol=0, atol=1e-15 if dtype == "f64" else 1.2e-6, err_msg=str(what))
    else:
        np.testing.assert_array_equal(act, np.asarray(cand)[rows, bi, 0, :], err_msg=str(what))
    return err


# ---- 1. operators ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("key", KEYS)
def test_operators_against_f17(reg, key, dtype):
    """rcg_rhs with clipping, rcg_out, rcg_stage_obj (a full non-symmetric R1 and a target) and rcg_rhs_full on F17's points: its
    inputs lie on the grid of 2^-10, exact in float32.  F17 records closed_loop_rhs on [state, disturb] only: rcg_rhs_full is
    held to it directly, rcg_rhs (no disturbance) to the twin, which test_user_system_corners.py pins on the same record at
    1e-13."""
    meta, z = load_f17()
    S, p = corner(key), key + "_r_"
    x, q, u, xi, a = (z[p + s] for s in ("state", "disturb", "action", "xi", "action_clipped"))
    c = f17_case(meta, z, key, "mpc_full_tgt")
    e = _engine(reg, key, dtype, 64, 5, c["R1"], observation_target=c["target"])
    assert (e.ds, e.du, e.npar, e.dy, e.dd) == (S.ds, S.du, S.np, S.dy, S.dd)
    d, ca = e.rhs(x, u, clip=True)
    np.testing.assert_array_equal(ca, a.astype(e.real))
    errs = {"rhs": _err(d, S.rhs(x, a)), "out": _err(e.out(x), z[key + "_o_out"]),
            "out n=7": _err(e.out(x[:7]), z[key + "_o_out"][:7]),
            "stage_obj": _err(e.stage_obj(c["ys"], c["seq"][:, 0]), z[f"{key}_a_mpc_full_tgt_stage"])}
    e.close()
    ed = _engine(reg, key, dtype, 64, 5, c["R1"], is_disturb=True, pars_disturb=[z[p + "sigma"], z[p + "mu"], z[p + "tau"]])
    d, dq, ca = ed.rhs_full(x, q, u, xi, clip=True)
    np.testing.assert_array_equal(ca, a.astype(ed.real))
    ref = z[p + "rhs_full"]
    errs["rhs_full"] = max(_err(d, ref[:, :S.ds]), _err(dq, ref[:, S.ds:]))
    ed.close()
    for what, err in errs.items():
        _note("1 operators", key, dtype, what, err)
        assert err < (RHS_TOL[dtype] if what.startswith("rhs") else TOL[dtype]), (what, err)


# ---- 2. env step -------------------------------------------------------------------------------------------------------------------
def _stage_dt(S, R1, target, dt):
    return lambda xx, a: stage_b(S.out(xx), a, R1, target) * dt


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("key", KEYS)
def test_k_sim_20_substeps_charge_the_cost_at_out_of_x(reg, key, dtype):
    from rcognita_amd import _native as N
    from tests.helpers import assert_kernel

    meta, z = load_f17()
    S = corner(key)
    c = f17_case(meta, z, key, "mpc_full_tgt")
    B, n_sub = 193, 20
    rng = np.random.default_rng(21)
    x0, a0 = S.rand_states(rng, B), S.rand_actions(rng, (B,), overshoot=1.3)
    e = _engine(reg, key, dtype, B, 5, c["R1"], observation_target=c["target"], accum_every_substep=True)
    r = _r(e)
    e.set_state(x0)
    e.set_field(N.FIELD_ACTION, a0)
    e.sim_step(n_sub)
    assert_kernel(e, "k_sim", kind=N.KERNEL_SIM)
    x, acc = sim_substeps(S, r(x0), r(a0), n_sub, DT_SIM, stage=_stage_dt(S, c["R1"], c["target"], meta["sampling_time"]))
    ex, ea = _err(e.get_state(), x), _err(e.get_field(N.FIELD_ACCUM), acc)
    _note("2 env step", key, dtype, "k_sim state", ex)
    _note("2 env step", key, dtype, "k_sim accum", ea)
    assert np.any(np.abs(S.clip(a0) - a0) > 0) and np.all(acc > 0)
    assert ex < RK4_TOL[dtype] and ea < RK4_TOL[dtype]
    e.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("key", KEYS)
def test_k_sim_dist_18_substeps_against_the_restatement(reg, key, dtype):
    from rcognita_amd import _native as N
    from tests.helpers import assert_kernel

    meta, z = load_f17()
    S, p = corner(key), key + "_r_"
    c = f17_case(meta, z, key, "mpc_g09")
    B = 193
    rng = np.random.default_rng(22)
    x, q0 = S.rand_states(rng, B), [0.3, -0.2][:S.dd]
    sig, mu, tau = z[p + "sigma"], z[p + "mu"], z[p + "tau"]
    e = _engine(reg, key, dtype, B, 5, c["R1"], accum_every_substep=True, is_disturb=True, pars_disturb=[sig, mu, tau],
                disturb_init=q0, seed=5, env_id_base=1000)
    r = _r(e)
    e.set_state(x)
    x, q, sub, acc = r(x), np.broadcast_to(r(q0), (B, S.dd)), np.zeros(B, np.int32), np.zeros(B)
    stage = _stage_dt(S, c["R1"], None, meta["sampling_time"])
    for n_sub in (7, 11):
        u = S.rand_actions(rng, (B,), overshoot=1.3)
        e.set_field(N.FIELD_ACTION, u)
        e.sim_step(n_sub)
        x, q, da, sub = sim_substeps(S, x, r(u), n_sub, DT_SIM, stage=stage,
                                     dist=dict(q=q, sub=sub, ep=np.zeros(B, np.int32), sigma=r(sig), mu=r(mu), tau=r(tau), seed=5,
                                               env_id_base=1000))
        acc = acc + da
    assert_kernel(e, "k_sim_dist", kind=N.KERNEL_SIM)
    np.testing.assert_array_equal(e.get_field(N.FIELD_SUBSTEP_IDX), sub)
    errs = {"state": _err(e.get_state(), x), "disturbance": _err(e.get_field(N.FIELD_DISTURB), q),
            "accum": _err(e.get_field(N.FIELD_ACCUM), acc)}
    for what, err in errs.items():
        _note("2 env step", key, dtype, "k_sim_dist " + what, err)
        assert err < RK4_TOL[dtype], (what, err)
    assert np.std(e.get_field(N.FIELD_DISTURB)) > 0.01
    e.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("key", KEYS)
def test_a_non_finite_env_freezes_alone(reg, key, dtype):
    from rcognita_amd import _native as N

    meta, z = load_f17()
    S = corner(key)
    B = 193
    rng = np.random.default_rng(23)
    x0 = S.rand_states(rng, B)
    bad = x0.copy()
    bad[70, S.ds - 1] = np.nan
    R1 = z[key + "_R1_diag"]
    a, clean = _engine(reg, key, dtype, B, 5, R1), _engine(reg, key, dtype, B, 5, R1)
    a.set_state(bad)
    clean.set_state(x0)
    for e in (a, clean):
        e.sim_step(3)
    st = a.get_field(N.FIELD_STATUS)
    ok = np.arange(B) != 70
    assert st[70] == 1 and not st[ok].any() and not clean.get_field(N.FIELD_STATUS).any()
    assert a.get_state()[70].tobytes() == bad[70].astype(a.real).tobytes()  # left as it was
    assert a.get_state()[ok].tobytes() == clean.get_state()[ok].tobytes()
    a.close()
    clean.close()


# ---- 3. _actor_cost on every decision kernel -------------------------------------------------------------------------------------
def _stream_kernel(S, esz, K, Nh, tag, gamma):
    """DESIGN.md section 4's table for a caller's tensor on an MPC handle of a policy without TGT."""
    from rcognita_amd import _native as N

    R = Nh * S.du
    slab16 = (K * R * esz) % 16 == 0
    full = tag == "mpc_full_tgt"
    if R > 64:
        return "k_actor", None
    if K >= 33 and slab16 and R <= 40:
        return "k_actor_dma", N.DMA_MPC_GENF if full else (N.DMA_MPC_G1 if gamma == 1.0 else N.DMA_MPC)
    if 4 <= K <= 32 and slab16 and R <= 40 and not full:
        return "k_actor_dma_packed", N.DMA_MPC_G1 if gamma == 1.0 else N.DMA_MPC
    return "k_actor", None


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("tag", MPC_CASES)
@pytest.mark.parametrize("key", KEYS)
def test_actor_cost_on_every_decision_kernel(reg, key, tag, dtype):
    """The 16 F17 points are envs 0 .. 15 of a batch of 77 (candidate 0 of each: the fixture's sequence, its J the reference's
    own); the whole J of every launch against the restatement.  K = 256 (four tiles), 40 (one ragged tile), 16 and 6 (packed; 6
    does not divide 64; C1 / C4 in float32: 6 rows of 5 floats are no whole 16-byte pieces - k_actor), 3 (k_actor), the
    generated grid and the DIRECT long rows."""
    from oracle import rcg_oracle as O
    from rcognita_amd import _native as N

    meta, z = load_f17()
    S = corner(key)
    c = f17_case(meta, z, key, tag)
    B, Nh = 77, meta["Nactor"]
    rng = np.random.default_rng(31)
    xs, ys = S.rand_states(rng, B), S.out(S.rand_states(rng, B))
    xs[:16], ys[:16] = c["xs"], c["ys"]
    e = _engine(reg, key, dtype, B, Nh, c["R1"], gamma=c["gamma"], observation_target=c["target"])
    r = _r(e)
    seen = set()
    for K in (256, 40, 16, 6, 3):
        cand = S.rand_actions(rng, (B, K, Nh)).astype(e.real)
        cand[:16, 0] = c["seq"]
        J = e.actor_cost(cand, obs=ys, state_sys=xs)
        ll = e.last_launch()
        Jr = case_cost(S, c, meta, cand.astype(float), xs=r(xs), ys=r(ys))
        e0, e1 = _err(J[:16, 0], c["J"]), _err(J, Jr)
        _note("3 actor cost", key, dtype, f"{tag} K={K}", max(e0, e1), ll)
        assert e0 < TOL[dtype] and e1 < TOL[dtype], (K, ll, e0, e1)
        want = _stream_kernel(S, np.dtype(e.real).itemsize, K, Nh, tag, c["gamma"])
        assert ll["kernel"] == want[0] and (want[1] is None or ll["variant"] == want[1]), (K, ll, want)
        seen.add(ll["kernel"])
        act, bj, bi = e.actor_argmin(cand, obs=ys, state_sys=xs)
        _check_argmin(act, bj, bi, Jr, cand, dtype, (tag, K))
    assert {"k_actor_dma", "k_actor"} <= seen and (tag == "mpc_full_tgt" or "k_actor_dma_packed" in seen), seen
    # the generated grid (k_actor): K levels per input held over the horizon
    K = 64
    act, bj, bi = e.actor_argmin(None, K=K, obs=ys, state_sys=xs)
    assert e.last_launch()["kernel"] == "k_actor", e.last_launch()
    grid = O.grid_candidates(oracle_cfg(S, "MPC", "quad-nomix", c["R1"], c["gamma"], c["target"], Nh, meta["pred_step_size"],
                                        meta["sampling_time"]), K)
    gridb = np.broadcast_to(r(grid)[None], (B,) + grid.shape)
    eg = _check_argmin(act, bj, bi, case_cost(S, c, meta, gridb, xs=r(xs), ys=r(ys)), gridb, dtype, (tag, "grid"), device_made=True)
    _note("3 actor cost", key, dtype, f"{tag} generated grid", eg, e.last_launch())
    e.close()
    if tag == "mpc_g1":  # a diagonal R1 WITH a target (F17 has it only with the full R1): the policy has no TGT, so k_actor's
        # streamed target instance serves it, against the restatement
        tg = z[f"{key}_target"]
        e = _engine(reg, key, dtype, B, Nh, c["R1"], gamma=c["gamma"], observation_target=tg)
        cand = S.rand_actions(rng, (B, 256, Nh)).astype(e.real)
        J = e.actor_cost(cand, obs=ys, state_sys=xs)
        ll = e.last_launch()
        assert (ll["kernel"], ll["variant"]) == ("k_actor", 2 | 4), ll
        et = _err(J, case_cost(S, c, meta, cand.astype(float), xs=r(xs), ys=r(ys), target=tg))
        _note("3 actor cost", key, dtype, "diagonal R1 with a target K=256", et, ll)
        assert et < TOL[dtype]
        e.close()
    # DIRECT: rows beyond 64 reals
    Nl = 70 if S.du == 1 else 33
    e = _engine(reg, key, dtype, B, Nl, c["R1"], gamma=c["gamma"], observation_target=c["target"])
    cand = S.rand_actions(rng, (B, 8, Nl)).astype(e.real)
    J = e.actor_cost(cand, obs=ys, state_sys=xs)
    ll = e.last_launch()
    assert ll["kernel"] == "k_actor" and ll["variant"] & 16, ll
    ed = _row_err(J, case_cost(S, c, meta, cand.astype(float), xs=r(xs), ys=r(ys)))
    _note("3 actor cost", key, dtype, f"{tag} DIRECT N={Nl}", ed, ll)
    assert ed < TOL[dtype]
    e.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("key", KEYS)
def test_argmin_from_the_state_and_from_a_callers_observation(reg, key, dtype):
    """obs = NULL: y_0 = out(STATE) (the obs_x path); a caller's observation that differs from out(state_sys) is used as given.  The
    batches are those of test_user_system_corners.py's float32 dry run."""
    meta, z = load_f17()
    S = corner(key)
    for tag in ("mpc_g1", "mpc_full_tgt"):
        c = f17_case(meta, z, key, tag)
        for B, K, Nh in ARGMIN_SHAPES:
            x, y, cand, _ = argmin_inputs(key, B, K, Nh)
            e = _engine(reg, key, dtype, B, Nh, c["R1"], gamma=c["gamma"], observation_target=c["target"])
            r = _r(e)
            cand = cand.astype(e.real)
            e.set_state(x)
            act, bj, bi = e.actor_argmin(cand)
            ll = e.last_launch()
            e0 = _check_argmin(act, bj, bi, case_cost(S, c, meta, cand.astype(float), xs=r(x), ys=S.out(r(x))), cand, dtype,
                               (tag, K, "from the state"))
            act, bj, bi = e.actor_argmin(cand, obs=y, state_sys=x)
            e1 = _check_argmin(act, bj, bi, case_cost(S, c, meta, cand.astype(float), xs=r(x), ys=r(y)), cand, dtype,
                               (tag, K, "caller's observation"))
            _note("3 argmin", key, dtype, f"{tag} K={K} N={Nh}", max(e0, e1), ll)
            assert ll["kernel"] == _stream_kernel(S, np.dtype(e.real).itemsize, K, Nh, tag, c["gamma"])[0], ll
            e.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("K", [16, 256])
@pytest.mark.parametrize("key", KEYS)
def test_a_tick_under_ref_lag_rolls_out_from_the_state_before_the_step(reg, key, K, dtype):
    """rcg_control_tick with REF_LAG: the state equals rcg_sim_step's bits, y_0 = out(STATE), the rollout starts at STATE_PREV."""
    from rcognita_amd import _native as N

    meta, z = load_f17()
    S = corner(key)
    c = f17_case(meta, z, key, "mpc_g1")
    B, Nh = 77, 5
    rng = np.random.default_rng(33)
    x0, a0 = S.rand_states(rng, B), S.rand_actions(rng, (B,))
    e, s = (_engine(reg, key, dtype, B, Nh, c["R1"], ref_lag=True, substeps_per_tick=2) for _ in range(2))
    cand = S.rand_actions(rng, (B, K, Nh)).astype(e.real)
    for h in (e, s):
        h.set_state(x0)
        h.set_field(N.FIELD_ACTION, a0)
    e.control_tick(cand)
    ll = e.last_launch()
    s.sim_step(2)
    x1, xp = s.get_state(), s.get_field(N.FIELD_STATE_PREV)
    assert e.get_state().tobytes() == x1.tobytes() and not np.array_equal(xp, x1)
    assert ll["kernel"] == ("k_actor_dma_packed" if K == 16 else "k_actor_dma"), ll
    y1 = S.out(x1.astype(float))
    J = case_cost(S, c, meta, cand.astype(float), xs=xp.astype(float), ys=y1)
    act = e.get_field(N.FIELD_ACTION)
    err = _check_argmin(act, e.get_field(N.FIELD_BEST_J), e.get_field(N.FIELD_BEST_IDX), J, cand, dtype, (key, K))
    _note("3 ref_lag", key, dtype, f"K={K}", err, ll)
    accum = stage_b(y1, act.astype(float), c["R1"], None) * meta["sampling_time"]
    assert _err(e.get_field(N.FIELD_ACCUM), accum) < (1e-12 if dtype == "f64" else TOL[dtype])
    e.close()
    s.close()


# ---- 4. per-env parameters -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("key", ["C2", "C3", "C4"])
def test_per_env_parameters_through_the_policys_prepare(reg, key, dtype, monkeypatch):
    """RCG_FLAG_PER_ENV_PARS on a user's policy: parameters within 20 % of nominal per env on k_actor_dma, k_actor_dma_packed,
    k_actor, k_sim, k_actor_opt and, five ticks closed loop, k_ticks - against the restatement with the same per-env parameters."""
    from oracle import parity as PAR
    from oracle import rcg_oracle as O
    from rcognita_amd import _native as N
    from tests.helpers import assert_kernel

    meta, z = load_f17()
    S = corner(key)
    c = f17_case(meta, z, key, "mpc_g09")
    seen = set()
    for B, K, Nh in ARGMIN_SHAPES:  # (K = 3: k_actor)
        x, y, cand, pars = argmin_inputs(key, B, K, Nh)
        e = _engine(reg, key, dtype, B, Nh, c["R1"], gamma=c["gamma"], per_env_pars=True)
        r = _r(e)
        cand = cand.astype(e.real)
        e.set_field(N.FIELD_PARS, pars)
        np.testing.assert_array_equal(e.get_field(N.FIELD_PARS), pars.astype(e.real))
        J = e.actor_cost(cand, obs=y, state_sys=x)
        ll = e.last_launch()
        seen.add(ll["kernel"])
        Jr = case_cost(S, c, meta, cand.astype(float), xs=r(x), ys=r(y), pars=r(pars))
        err = _err(J, Jr)
        _note("4 per-env pars", key, dtype, f"K={K} N={Nh}", err, ll)
        assert err < TOL[dtype], (K, ll)
        J_nom = case_cost(S, c, meta, cand.astype(float), xs=r(x), ys=r(y))
        assert _err(J_nom, Jr) > 1e3 * TOL[dtype]  # (the nominal parameters give other costs)
        e.set_state(x)
        act, bj, bi = e.actor_argmin(cand)
        _check_argmin(act, bj, bi, case_cost(S, c, meta, cand.astype(float), xs=r(x), ys=S.out(r(x)), pars=r(pars)), cand, dtype, K)
        if K == 256:  # k_sim and the optimiser (k_actor_opt parks the parameters in LDS) with per-env parameters
            e.set_field(N.FIELD_ACTION, cand[:, 0, 0])
            e.sim_step(4)
            xr, _ = sim_substeps(S, r(x), cand[:, 0, 0].astype(float), 4, DT_SIM, pars=r(pars))
            es = _err(e.get_state(), xr)
            assert es < RK4_TOL[dtype], es
            e.set_state(x)
            for memory in (0, 4):
                e.set_optimizer(memory)
                _, U, Jo, _ = e.actor_optimize(iters=10)
                assert_kernel(e, "k_actor_opt")
                Ju = case_cost(S, c, meta, U[:, None].astype(float), xs=r(x), ys=S.out(r(x)), pars=r(pars))[:, 0]
                eo = _err(Jo, Ju)
                _note("4 per-env pars", key, dtype, f"k_actor_opt memory {memory}", eo)
                assert eo < TOL[dtype], eo
        e.close()
    assert seen == {"k_actor_dma", "k_actor_dma_packed", "k_actor"}, seen
    # five ticks closed loop: single ticks on k_actor_dma against the restated tick, then the same five in ONE launch (k_ticks)
    B, K, Nh, T = 77, 256, 5, 5
    x, _, cand, pars = argmin_inputs(key, B, K, Nh, seed=1)
    one, many = (_engine(reg, key, dtype, B, Nh, c["R1"], gamma=c["gamma"], per_env_pars=True) for _ in range(2))
    r = _r(one)
    cand = cand.astype(one.real)
    for e in (one, many):
        e.set_state(x)
        e.set_field(N.FIELD_PARS, pars)
    cfg = oracle_cfg(S, "MPC", "quad-nomix", c["R1"], c["gamma"], None, Nh, meta["pred_step_size"], meta["sampling_time"])
    cfg.dt_sim = DT_SIM
    env = O.EnvBatch(state=r(x), action=one.get_field(N.FIELD_ACTION).astype(float), accum=np.zeros(B), step_idx=np.zeros(B, np.int32),
                     episode_idx=np.zeros(B, np.int32), pars=r(pars), state_prev=r(x))
    rep = PAR.TickReport()
    monkeypatch.setattr(O, "control_tick", restated_tick(S))
    for t in range(T):
        one.control_tick(cand)
        assert_kernel(one, "k_actor_dma")
        env = PAR.check_tick(cfg, env, cand.astype(float), PAR.device_fields(one, N), tol=1e-9 if dtype == "f64" else 1e-5,
                             report=rep, what=f"{key} per-env pars t={t}")
    print(f"corners 4 per-env pars {key} {dtype} ticks:", rep.as_dict())
    cb = many.to_device(cand)
    many.control_tick(cb, K=K, T=T)
    assert_kernel(many, "k_ticks")
    _same(many, one, FIELDS, (key, "k_ticks with per-env parameters"))
    one.close()
    many.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_per_env_flag_on_a_system_without_parameters_is_ignored(reg, dtype):
    """C1 (NP = 0) with RCG_FLAG_PER_ENV_PARS: accepted and ignored (include/rcg.h) - RCG_FIELD_PARS is not allocated, and
    every result is the bits of a handle without the flag."""
    from rcognita_amd import _native as N

    meta, z = load_f17()
    S = corner("C1")
    c = f17_case(meta, z, "C1", "mpc_g1")
    B, K, Nh = 77, 256, 5
    x, y, cand, pars = argmin_inputs("C1", B, K, Nh)
    assert pars is None
    a, b = _engine(reg, "C1", dtype, B, Nh, c["R1"], per_env_pars=True), _engine(reg, "C1", dtype, B, Nh, c["R1"])
    assert N.lib().rcg_field_bytes(a._h, N.FIELD_PARS) == 0
    buf = np.zeros(B, a.real)
    assert N.lib().rcg_set_field(a._h, N.FIELD_PARS, buf.ctypes.data, N.HOST) == N.ERR_BAD_ARG
    assert N.lib().rcg_get_field(a._h, N.FIELD_PARS, buf.ctypes.data, N.HOST) == N.ERR_BAD_ARG
    cand = cand.astype(a.real)
    for e in (a, b):
        e.set_state(x)
    assert a.actor_cost(cand).tobytes() == b.actor_cost(cand).tobytes()
    assert a.last_launch() == b.last_launch() and a.last_launch()["kernel"] == "k_actor_dma"
    assert a.actor_cost(cand[:, :16]).tobytes() == b.actor_cost(cand[:, :16]).tobytes()
    assert a.last_launch()["kernel"] == "k_actor_dma_packed"
    for e in (a, b):
        e.set_optimizer(4)
    for u, v in zip(a.actor_optimize(5), b.actor_optimize(5)):
        assert u.tobytes() == v.tobytes()
    for e in (a, b):
        e.control_tick(cand)
        e.control_ticks(3, 64)
    assert a.last_launch()["kernel"] == "k_ticks"
    _same(a, b, FIELDS, "NP = 0 with the flag")
    J = a.actor_cost(cand, obs=y, state_sys=x)
    assert _err(J, case_cost(S, c, meta, cand.astype(float), xs=_r(a)(x), ys=_r(a)(y))) < TOL[dtype]
    a.close()
    b.close()


# ---- 5. RQL / SQL ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("cs", STRUCTS)
@pytest.mark.parametrize("key", KEYS)
def test_critic_operators_against_f17(reg, key, cs, dtype):
    """rcg_critic and rcg_critic_cost (with a target) and the streamed RQL / SQL _actor_cost (K = 256: k_actor_dma's DMA_RQL_* /
    DMA_SQL_* instances; K = 16: packed where an instance exists) on F17's points, embedded as in section 3."""
    from rcognita_amd import _native as N

    meta, z = load_f17()
    S = corner(key)
    k = cs.replace("-", "_")
    tol = TOL[dtype]
    tg, R1 = z[f"{key}_target"], z[f"{key}_R1_diag"]
    kw = dict(mode="RQL", critic_struct=cs, Ncritic=meta["Ncritic"], buffer_size=meta["buffer_size"], gamma=meta["gamma_critic"])
    e = _engine(reg, key, dtype, 16, 5, R1, observation_target=tg, **kw)
    assert e.dc == dim_critic(cs, S.dy, S.du) == meta["systems"][key]["dim_critic"][cs]
    Q = z[f"{key}_c_{k}_Q"]
    eq = float(np.max(np.abs(e.critic(z[f"{key}_c_{k}_obs"], z[f"{key}_c_{k}_act"], z[f"{key}_c_{k}_w"]) - Q)) / np.max(np.abs(Q)))
    e.set_field(N.FIELD_OBS_BUF, z[f"{key}_d_{k}_obs_buf"])
    e.set_field(N.FIELD_ACT_BUF, z[f"{key}_d_{k}_act_buf"])
    e.set_field(N.FIELD_W_PREV, z[f"{key}_d_{k}_w_prev"])
    Jc = z[f"{key}_d_{k}_Jc"]
    ec = float(np.max(np.abs(e.critic_cost(z[f"{key}_d_{k}_w"]) - Jc)) / np.max(np.abs(Jc)))
    _note("5 critic", key, dtype, f"{cs} rcg_critic", eq)
    _note("5 critic", key, dtype, f"{cs} rcg_critic_cost", ec)
    assert eq <= tol and ec <= tol, (eq, ec)
    e.close()
    rng = np.random.default_rng(51)
    B, Nh = 77, meta["Nactor"]
    for mode in ("RQL", "SQL"):
        c = f17_case(meta, z, key, f"{mode}_{k}")
        xs, ys = S.rand_states(rng, B), S.out(S.rand_states(rng, B))
        w = rng.uniform(0.1, 2.0, (B, dim_critic(cs, S.dy, S.du)))
        xs[:16], ys[:16], w[:16] = c["xs"], c["ys"], c["w"]
        e = _engine(reg, key, dtype, B, Nh, R1, **dict(kw, mode=mode))
        r = _r(e)
        for K in (256, 16):
            cand = S.rand_actions(rng, (B, K, Nh)).astype(e.real)
            cand[:16, 0] = c["seq"]
            J = e.actor_cost(cand, obs=ys, state_sys=xs, w=w)
            ll = e.last_launch()
            Jr = case_cost(S, c, meta, cand.astype(float), xs=r(xs), ys=r(ys), w=r(w))
            e0 = float(np.max(np.abs(J[:16, 0] - c["J"]) / np.maximum(np.max(np.abs(Jr[:16]), axis=1), 1.0)))
            e1 = _row_err(J, Jr)
            _note("5 critic", key, dtype, f"{mode} {cs} K={K}", max(e0, e1), ll)
            assert e0 <= tol and e1 <= tol, (mode, K, ll, e0, e1)
            if K == 256:
                assert (ll["kernel"], ll["variant"]) == ("k_actor_dma", (N.DMA_RQL_0 if mode == "RQL" else N.DMA_SQL_0) + STRUCTS.index(cs)), ll
            else:  # (the packed instances hold at most 36 dwords of weights; beyond, the launcher goes on to k_actor)
                dwords = e.dc * (1 if dtype == "f32" else 2)
                assert ll["kernel"] == ("k_actor_dma_packed" if dwords <= 36 else "k_actor"), (ll, dwords)
        e.close()


def _critic_env(O, cfg, e, x0, B, S, bs):
    from rcognita_amd import _native as N

    return O.EnvBatch(state=x0.astype(float), action=e.get_field(N.FIELD_ACTION).astype(float), accum=np.zeros(B),
                      step_idx=np.zeros(B, np.int32), episode_idx=np.zeros(B, np.int32), pars=cfg.pars, state_prev=x0.astype(float).copy(),
                      w_critic=np.ones((B, cfg.dc)), w_prev=np.ones((B, cfg.dc)), obs_buf=np.zeros((B, bs, S.dy)),
                      act_buf=np.zeros((B, bs, S.du)))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("cs", STRUCTS)
@pytest.mark.parametrize("mode", ["RQL", "SQL"])
@pytest.mark.parametrize("key", KEYS)
def test_closed_loop_ticks_with_the_fit_against_the_restated_tick(reg, key, mode, cs, dtype, monkeypatch):
    """Four ticks - env step, push of out(STATE), fit, decision - at K = 256 and K = 16, each checked as a map from the same
    inputs by oracle/parity.py::check_tick with the restated tick in the oracle's place (weights and both buffers included; a
    near-tied argmin is followed).  Tolerances: test_hip_user_system_critic.py::test_closed_loop_ticks_against_the_restatement.
    The fit runs one lane per env up to 8 weights and four lanes per env (k_critic_fit_ml) from 9: C3's quad-mix (8) and C4's
    (11) sit on either side."""
    from oracle import parity as PAR
    from oracle import rcg_oracle as O
    from rcognita_amd import _native as N

    meta, z = load_f17()
    S = corner(key)
    monkeypatch.setattr(O, "control_tick", restated_tick(S))
    R1, bs = z[f"{key}_R1_diag"], meta["buffer_size"]
    rng = np.random.default_rng(52)
    B, Nh, T = 19, 5, 4
    for K in (256, 16):
        e = _engine(reg, key, dtype, B, Nh, R1, mode=mode, critic_struct=cs, Ncritic=meta["Ncritic"], buffer_size=bs,
                    gamma=meta["gamma_critic"])
        cfg = oracle_cfg(S, mode, cs, R1, meta["gamma_critic"], None, Nh, meta["pred_step_size"], meta["sampling_time"],
                         n_critic=meta["Ncritic"], buffer_size=bs)
        cfg.dt_sim = DT_SIM
        x0 = (0.5 * S.rand_states(rng, B)).astype(e.real)
        e.set_state(x0)
        env = _critic_env(O, cfg, e, x0, B, S, bs)
        cand = S.rand_actions(rng, (B, K, Nh)).astype(e.real)
        rep = PAR.TickReport()
        for t in range(T):
            e.control_tick(cand)
            lf = e.last_launch(N.KERNEL_CRITIC)
            assert lf["kernel"] == "k_critic_fit" and bool(lf["variant"] & FIT_ML) == (e.dc >= 9) and not lf["variant"] & FIT_GEN, (lf, e.dc)
            env = PAR.check_tick(cfg, env, cand.astype(float), PAR.device_fields(e, N, critic=True),
                                 tol=1e-9 if dtype == "f64" else 1e-5,
                                 tol_over={"w_critic": 1e-6, "best_J": 1e-7} if dtype == "f64" else None, report=rep,
                                 what=f"{key} {mode} {cs} K={K} t={t}")
        assert rep.ticks == T
        print(f"corners 5 ticks {key} {mode} {cs} {dtype} K={K} {e.last_launch()['kernel']}/{e.last_launch()['variant']} "
              f"fit {lf['variant']}:", rep.as_dict())
        e.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("key", ["C3", "C4"])
def test_the_fit_over_three_waves_and_one_lane(reg, key, dtype, monkeypatch):
    """B = 193 (three waves and one lane of the one-lane fit, a ragged last wave of the four-lane fit): rcg_critic and
    rcg_critic_cost on a random batch against the oracle's functions, then two quad-mix ticks with the fit - C3 (8 weights) on
    k_critic_fit's one lane per env, C4 (11) on k_critic_fit_ml - against the restated tick."""
    from oracle import parity as PAR
    from oracle import rcg_oracle as O
    from rcognita_amd import _native as N

    meta, z = load_f17()
    S = corner(key)
    monkeypatch.setattr(O, "control_tick", restated_tick(S))
    R1, bs, cs = z[f"{key}_R1_diag"], meta["buffer_size"], "quad-mix"
    rng = np.random.default_rng(54)
    B, Nh, K = 193, 5, 16
    e = _engine(reg, key, dtype, B, Nh, R1, mode="RQL", critic_struct=cs, Ncritic=meta["Ncritic"], buffer_size=bs,
                gamma=meta["gamma_critic"])
    cfg = oracle_cfg(S, "RQL", cs, R1, meta["gamma_critic"], None, Nh, meta["pred_step_size"], meta["sampling_time"],
                     n_critic=meta["Ncritic"], buffer_size=bs)
    cfg.dt_sim = DT_SIM
    r = _r(e)
    y, u, w, wp = S.out(S.rand_states(rng, B)), S.rand_actions(rng, (B,)), rng.uniform(-2, 2, (B, e.dc)), rng.uniform(-2, 2, (B, e.dc))
    Q = O.critic(r(y), r(u), r(w), cfg)
    eq = float(np.max(np.abs(e.critic(y, u, w) - Q)) / np.max(np.abs(Q)))
    ob, ab = S.out(S.rand_states(rng, B * bs)).reshape(B, bs, S.dy), S.rand_actions(rng, (B, bs))
    e.set_field(N.FIELD_OBS_BUF, ob)
    e.set_field(N.FIELD_ACT_BUF, ab)
    e.set_field(N.FIELD_W_PREV, wp)
    Jc = O.critic_cost(r(w), r(wp), r(ob), r(ab), cfg)
    ec = float(np.max(np.abs(e.critic_cost(w) - Jc)) / np.max(np.abs(Jc)))
    _note("5 critic", key, dtype, f"{cs} B=193 rcg_critic", eq)
    _note("5 critic", key, dtype, f"{cs} B=193 rcg_critic_cost", ec)
    assert eq <= TOL[dtype] and ec <= TOL[dtype], (eq, ec)
    e.close()
    e = _engine(reg, key, dtype, B, Nh, R1, mode="RQL", critic_struct=cs, Ncritic=meta["Ncritic"], buffer_size=bs,
                gamma=meta["gamma_critic"])
    x0 = (0.5 * S.rand_states(rng, B)).astype(e.real)
    e.set_state(x0)
    env = _critic_env(O, cfg, e, x0, B, S, bs)
    cand = S.rand_actions(rng, (B, K, Nh)).astype(e.real)
    rep = PAR.TickReport()
    for t in range(2):
        e.control_tick(cand)
        lf = e.last_launch(N.KERNEL_CRITIC)
        assert lf["kernel"] == "k_critic_fit" and bool(lf["variant"] & FIT_ML) == (key == "C4") and not lf["variant"] & FIT_GEN, lf
        env = PAR.check_tick(cfg, env, cand.astype(float), PAR.device_fields(e, N, critic=True), tol=1e-9 if dtype == "f64" else 1e-5,
                             tol_over={"w_critic": 1e-6, "best_J": 1e-7} if dtype == "f64" else None, report=rep,
                             what=f"{key} B=193 t={t}")
    print(f"corners 5 ticks {key} RQL {cs} {dtype} K={K} B=193 {e.last_launch()['kernel']}/{e.last_launch()['variant']} "
          f"fit {lf['variant']}:", rep.as_dict())
    e.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_eleven_td_rows_on_c2_take_the_general_fit(reg, dtype, monkeypatch):
    """Ncritic - 1 = 11 on C2 (DY = 1): k_critic_fit_gen, three ticks against the restated tick."""
    from oracle import parity as PAR
    from oracle import rcg_oracle as O
    from rcognita_amd import _native as N

    meta, z = load_f17()
    S = corner("C2")
    monkeypatch.setattr(O, "control_tick", restated_tick(S))
    R1, bs, nc, cs = z["C2_R1_diag"], 14, 12, "quad-nomix"
    rng = np.random.default_rng(53)
    B, Nh, K = 19, 5, 64
    e = _engine(reg, "C2", dtype, B, Nh, R1, mode="RQL", critic_struct=cs, Ncritic=nc, buffer_size=bs, gamma=meta["gamma_critic"])
    cfg = oracle_cfg(S, "RQL", cs, R1, meta["gamma_critic"], None, Nh, meta["pred_step_size"], meta["sampling_time"], n_critic=nc,
                     buffer_size=bs)
    cfg.dt_sim = DT_SIM
    x0 = (0.5 * S.rand_states(rng, B)).astype(e.real)
    e.set_state(x0)
    # buffers as a closed loop leaves them, so that all eleven rows carry data from the first tick on
    ob, ab = S.out(0.5 * S.rand_states(rng, B * bs)).reshape(B, bs, S.dy), S.rand_actions(rng, (B, bs))
    e.set_field(N.FIELD_OBS_BUF, ob)
    e.set_field(N.FIELD_ACT_BUF, ab)
    env = _critic_env(O, cfg, e, x0, B, S, bs)
    env.obs_buf, env.act_buf = _r(e)(ob), _r(e)(ab)
    cand = S.rand_actions(rng, (B, K, Nh)).astype(e.real)
    rep = PAR.TickReport()
    for t in range(3):
        e.control_tick(cand)
        lf = e.last_launch(N.KERNEL_CRITIC)
        assert lf["kernel"] == "k_critic_fit" and lf["variant"] & FIT_GEN, lf
        # (more rows than weights: the bounds of tests/test_hip_critic.py::test_closed_loop_with_eleven_td_rows_vs_oracle)
        env = PAR.check_tick(cfg, env, cand.astype(float), PAR.device_fields(e, N, critic=True), tol=1e-9 if dtype == "f64" else 1e-5,
                             tol_over={"w_critic": 5e-5, "best_J": 1e-6} if dtype == "f64" else None, report=rep,
                             what=f"C2 gen fit t={t}")
    print(f"corners 5 gen fit C2 {dtype}:", rep.as_dict())
    e.close()


# ---- 6. the optimiser --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("memory", [0, 4])
@pytest.mark.parametrize("key", KEYS)
def test_optimizer_against_slsqp_on_the_f17_starts(reg, key, memory, dtype):
    """rcg_actor_optimize with jac_T and out_jac_T from the reference's start on F17 (s)'s eight states: the reported J is the
    restated cost of the returned sequence, J(30) <= J(5) <= J(start), and J(30) is at most 0.5 % above SLSQP's (the bar of
    tests/test_hip_optimizer.py)."""
    from tests.helpers import assert_kernel

    meta, z = load_f17()
    S = corner(key)
    x, R1, Nh = z[f"{key}_s_state"], z[f"{key}_R1_diag"], meta["Nactor"]
    B = len(x)
    e = _engine(reg, key, dtype, B, Nh, R1)
    r = _r(e)
    e.set_state(x)
    e.set_optimizer(memory)
    cost = lambda U: actor_cost(S, U[:, None].astype(float), S.out(r(x)), r(x), R1, 1.0, None, meta["pred_step_size"])[:, 0]  # noqa: E731
    Js = {}
    for iters in (5, 30):
        act, U, J, _ = e.actor_optimize(iters=iters)
        assert_kernel(e, "k_actor_opt")
        np.testing.assert_array_equal(act, U[:, 0, :])
        assert np.all(U >= S.bnds[:, 0] - 1e-4) and np.all(U <= S.bnds[:, 1] + 1e-4)
        err = _err(J, cost(U))
        _note("6 optimiser", key, dtype, f"memory {memory} iters {iters} BEST_J", err)
        assert err < TOL[dtype], (iters, err)
        Js[iters] = J.astype(float)
    J0 = z[f"{key}_s_J_init"]
    slack = 4 * TOL[dtype] * np.maximum(np.abs(J0), 1.0)
    assert np.all(Js[30] <= Js[5] + slack) and np.all(Js[5] <= J0 + slack)
    Jopt = z[f"{key}_s_J_opt"]
    gap = (Js[30] - Jopt) / np.abs(Jopt)
    _note("6 optimiser", key, dtype, f"memory {memory} worst J / J_slsqp - 1", float(np.max(gap)))
    assert np.all(Js[30] <= Jopt + np.abs(Jopt) * 5e-3), gap
    e.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("memory", [0, 4])
def test_c1_optimizer_against_the_oracle_twin(reg, dtype, memory, monkeypatch):
    """C1 has no output map: patched into oracle.rcg_oracle as test_hip_user_system.py::pend_oracle patches the pendulum in, the
    oracle's per-iteration twin runs unchanged (tolerances of test_pendulum_optimizer_against_the_oracle_twin)."""
    from oracle import rcg_oracle as O

    meta, z = load_f17()
    S, sid = corner("C1"), reg["C1"]["sys_id"]
    dyn0, jac0 = O.state_dyn, O.state_jac_T
    monkeypatch.setattr(O, "state_dyn", lambda s, x, u, p: S.rhs(np.asarray(x, float), np.asarray(u, float)) if s == sid else dyn0(s, x, u, p))
    monkeypatch.setattr(O, "state_jac_T", lambda s, x, u, p, lam: S.jac_T(x, u, lam) if s == sid else jac0(s, x, u, p, lam))
    monkeypatch.setitem(O.SYS_DIMS, sid, (1, 1, 0))
    R1 = z["C1_R1_diag"]
    rng = np.random.default_rng(61)
    B, Nh = 64, 10
    x = S.rand_states(rng, B)
    e = _engine(reg, "C1", dtype, B, Nh, R1)
    cfg = O.OracleCfg(sys_id=sid, n_actor=Nh, pred_step_size=meta["pred_step_size"], dt_sim=DT_SIM, sampling_time=meta["sampling_time"],
                      pars=[], ctrl_bnds=S.bnds, R1=R1)
    e.set_state(x)
    e.set_optimizer(memory)
    act, U, J, its = e.actor_optimize(iters=10)
    xr = _r(e)(x)
    assert _err(J, O.actor_cost(U.astype(np.float64), xr, xr, cfg)) < (1e-10 if dtype == "f64" else 1e-5)
    U_or, J_or, its_or = O.actor_optimize(cfg, xr, xr, O.action_sqn_init(cfg), iters=10, memory=memory)
    if dtype == "f64":
        assert np.all(np.abs(its - its_or) <= 3)
        assert _err(J, J_or) < 1e-9 and float(np.max(np.abs(U - U_or) / 5.0)) < 1e-5
    else:
        assert _err(J, J_or) < 2e-4
    _note("6 optimiser", "C1", dtype, f"memory {memory} J against the oracle twin", _err(J, J_or))
    e.close()


# ---- 7. the search -----------------------------------------------------------------------------------------------------------------
ROWS = 4  # rcg_last_launch's variant word of k_actor_search: bit 0 generic, bit 1 target, bit 2 register rows


def _search(eng, S, dtype, K, rounds, cost, obs, xs, what):
    """test_hip_user_system_search.py::_check_search for any (du, bounds): rcg_actor_search against search_replay over the
    device's own candidates."""
    from oracle import rcg_oracle as O
    from tests.helpers import assert_kernel

    B, Nh = eng.B, eng.N
    act, U, J, bi = eng.actor_search(K=K, rounds=rounds, obs=obs, state_sys=xs)
    ll = assert_kernel(eng, "k_actor_search")
    np.testing.assert_array_equal(act, U[:, 0, :])
    assert np.all(U >= S.bnds[:, 0]) and np.all(U <= S.bnds[:, 1])
    err = _err(J, cost(U.astype(np.float64)[:, None])[:, 0])
    u0 = np.broadcast_to(S.bnds[:, 0] / 10.0, (B, Nh, S.du))  # action_sqn_init (controllers.py:973-978)
    sampler = lambda r, centre: eng.candidates_sample(K, round=r, centre=centre.astype(eng.real)).astype(np.float64)  # noqa: E731
    c = np.array(u0, dtype=np.float64)
    for rd in range(rounds):  # (test_user_system_search_register.py::search_replay with candidates [B, K, N, du])
        cand = sampler(rd, c)
        J_or, bi_or = O.argmin_first(cost(cand))
        c = cand[np.arange(B), bi_or]
    U_or = c
    same = np.all(U.astype(np.float64) == U_or, axis=(1, 2))
    _note("7 search", S.name, dtype, f"{what} share on the replay's sequence {np.mean(same):.3f}; |J - J(U)|", err, ll)
    assert err < TOL[dtype], what
    if dtype == "f64":
        np.testing.assert_array_equal(bi, bi_or)
        np.testing.assert_array_equal(U, U_or)
        assert _err(J, J_or) < 1e-11, what
    else:  # a float32 argmin may take the other side of a near tie in some round: the cost reached must agree
        assert np.mean(same) > 0.8, what
        assert np.all(np.abs(J - J_or) <= 4 * TOL[dtype] * np.maximum(np.abs(J_or), 1.0) + 1e-3 * np.abs(J_or) * ~same), what
    return ll


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("Nh", [5, 10, 7])
@pytest.mark.parametrize("key", KEYS)
def test_search_mpc_on_the_devices_own_candidates(reg, key, Nh, dtype):
    """MPC with the diagonal R1: Nactor = 5 and 10 are the register-row instances where search_plan gives them (the variant word
    says which ran), 7 the LDS rows; once with an observation handed in, once from the state.  DU = 2 draws included (C2, C3).
    float32: the seeds are those test_user_system_corners.py's dry run cleared."""
    from rcognita_amd import _native as N

    meta, z = load_f17()
    S = corner(key)
    c = f17_case(meta, z, key, "mpc_g1")
    B, K, rounds = 29, 192, 3
    x, xl = search_inputs(key, B)
    eng = _engine(reg, key, dtype, B, Nh, c["R1"], seed=7)
    eng.set_field(N.FIELD_STEP_IDX, np.arange(B, dtype=np.int32))
    r = _r(eng)
    variants = set()
    for obs in (S.out(xl), None):
        eng.set_state(x)
        ys = r(obs) if obs is not None else S.out(r(x))
        cost = lambda cand: case_cost(S, c, meta, cand, xs=r(x), ys=ys)  # noqa: E731
        ll = _search(eng, S, dtype, K, rounds, cost, obs, x if obs is not None else None,
                     f"N={Nh} {'obs' if obs is not None else 'from the state'}")
        variants.add(ll["variant"])
    # search_plan: register rows at Nactor 5 and 10 whatever DU is, LDS rows in float64 at 10; diagonal cost, no target
    rows = Nh in (5, 10) and not (dtype == "f64" and Nh == 10)
    assert variants == {ROWS if rows else 0}, (variants, Nh, dtype)
    eng.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("cs", ["quad-mix", "quad-lin"])
def test_search_rql_on_c3(reg, cs, dtype):
    meta, z = load_f17()
    S = corner("C3")
    c = f17_case(meta, z, "C3", "RQL_" + cs.replace("-", "_"))
    B, K, rounds, Nh = 29, 192, 3, 5
    x, xl = search_inputs("C3", B)
    w = search_weights("C3", cs, B)
    from rcognita_amd import _native as N

    eng = _engine(reg, "C3", dtype, B, Nh, c["R1"], mode="RQL", critic_struct=cs, Ncritic=meta["Ncritic"], buffer_size=meta["buffer_size"],
                  gamma=c["gamma"], seed=7)
    eng.set_field(N.FIELD_STEP_IDX, np.arange(B, dtype=np.int32))
    eng.set_field(N.FIELD_W_CRITIC, w)
    eng.set_state(x)
    r = _r(eng)
    cost = lambda cand: case_cost(S, c, meta, cand, xs=r(x), ys=r(S.out(xl)), w=r(w))  # noqa: E731
    ll = _search(eng, S, dtype, K, rounds, cost, S.out(xl), x, f"RQL {cs}")
    assert ll["variant"] == 1, ll  # generic, no target, LDS rows
    eng.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("key", KEYS)
def test_control_tick_search_three_ticks(reg, key, dtype):
    """rcg_control_tick_search, each tick as a map from the device's own pre-tick fields: env step (the bits of rcg_sim_step),
    then the search from y_0 = out(STATE) against the replay over the device's candidates; accum at out(STATE).  float64: the
    replay's index, sequence and cost.  float32 (the first tick's dry run: test_user_system_corners.py): the reported cost is the
    restated cost of the reported sequence, and the rule of the operator case for envs that took the other side of a near tie."""
    from oracle import rcg_oracle as O
    from rcognita_amd import _native as N
    from tests.helpers import assert_kernel

    meta, z = load_f17()
    S = corner(key)
    c = f17_case(meta, z, key, "mpc_g1")
    B, K, rounds, Nh = 29, 64, 2, 5
    tol = TOL[dtype]
    x0, _ = search_inputs(key, B)
    eng, twin = _engine(reg, key, dtype, B, Nh, c["R1"], seed=99), _engine(reg, key, dtype, B, Nh, c["R1"])
    eng.set_state(x0)
    for t in range(3):
        pre = {f: eng.get_field(f).copy() for f in (N.FIELD_STATE, N.FIELD_ACTION, N.FIELD_ACCUM, N.FIELD_STEP_IDX)}
        eng.control_tick_search(K=K, rounds=rounds)
        ll = assert_kernel(eng, "k_actor_search")
        assert ll["variant"] == ROWS, ll  # Nactor = 5: register rows in both widths
        twin.set_field(N.FIELD_STATE, pre[N.FIELD_STATE])
        twin.set_field(N.FIELD_ACTION, pre[N.FIELD_ACTION])
        twin.sim_step(1)
        x1 = eng.get_state()
        assert x1.tobytes() == twin.get_state().tobytes(), t
        x1 = x1.astype(float)
        cost = lambda cand: case_cost(S, c, meta, cand, xs=x1, ys=S.out(x1))  # noqa: E731
        # candidates of this tick: STEP_IDX was pre[STEP_IDX] when they were drawn
        eng.set_field(N.FIELD_STEP_IDX, pre[N.FIELD_STEP_IDX])
        cen = np.broadcast_to(S.bnds[:, 0] / 10.0, (B, Nh, S.du)).astype(float)
        for rd in range(rounds):
            cand = eng.candidates_sample(K, round=rd, centre=cen.astype(eng.real)).astype(float)
            J_or, bi_or = O.argmin_first(cost(cand))
            cen = cand[np.arange(B), bi_or]
        eng.set_field(N.FIELD_STEP_IDX, pre[N.FIELD_STEP_IDX] + 1)
        U, J = eng.get_field(N.FIELD_ACTION_SQN).astype(float), eng.get_field(N.FIELD_BEST_J).astype(float)
        err = _err(J, cost(U[:, None])[:, 0])
        same = np.all(U == cen, axis=(1, 2))
        _note("7 search", key, dtype, f"control_tick_search t={t} share on the replay's sequence {np.mean(same):.3f}; |J - J(U)|", err, ll)
        assert err < tol, t
        if dtype == "f64":
            np.testing.assert_array_equal(eng.get_field(N.FIELD_BEST_IDX), bi_or, err_msg=str(t))
            np.testing.assert_array_equal(U, cen, err_msg=str(t))
            assert _err(J, J_or) < 1e-10, t
        else:
            assert np.mean(same) > 0.8, t
            assert np.all(np.abs(J - J_or) <= 4 * tol * np.maximum(np.abs(J_or), 1.0) + 1e-3 * np.abs(J_or) * ~same), t
        act = eng.get_field(N.FIELD_ACTION)
        np.testing.assert_array_equal(act, eng.get_field(N.FIELD_ACTION_SQN)[:, 0, :])
        accum = pre[N.FIELD_ACCUM].astype(float) + stage_b(S.out(x1), act.astype(float), c["R1"], None) * meta["sampling_time"]
        assert _err(eng.get_field(N.FIELD_ACCUM), accum) < (1e-12 if dtype == "f64" else tol), t
    np.testing.assert_array_equal(eng.get_field(N.FIELD_STEP_IDX), np.full(B, 3, np.int32))
    eng.close()
    twin.close()


# ---- 8. T ticks per launch ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("what", ["generated", "streamed", "RQL quad-nomix", "disturbed"])
@pytest.mark.parametrize("key", KEYS)
def test_seven_ticks_in_one_launch_equal_seven_single_ticks(reg, key, what, dtype):
    """rcg_control_ticks(T = 7) (streamed: rcg_control_tick_n with a caller's tensor) leaves every field - weights and buffers
    included - with the bits of seven single ticks."""
    from rcognita_amd import _native as N
    from tests.helpers import assert_kernel

    meta, z = load_f17()
    S, p = corner(key), key + "_r_"
    R1 = z[f"{key}_R1_diag"]
    T, Nh, B = 7, 5, 77
    K = 16 if what == "streamed" else 64
    rng = np.random.default_rng(81)
    kw, fields = {}, FIELDS
    if what == "RQL quad-nomix":
        kw, fields = dict(mode="RQL", critic_struct="quad-nomix", Ncritic=4, buffer_size=6, gamma=meta["gamma_critic"]), CRITIC_FIELDS
    if what == "disturbed":
        kw = dict(is_disturb=True, pars_disturb=[z[p + "sigma"], z[p + "mu"], z[p + "tau"]], disturb_init=[0.3, -0.2][:S.dd], seed=5,
                  env_id_base=64)
        fields = DISTURB_FIELDS
    one, many = (_engine(reg, key, dtype, B, Nh, R1, **kw) for _ in range(2))
    x0 = 0.5 * S.rand_states(rng, B)
    ca = cb = None
    if what == "streamed":
        cnd = S.rand_actions(rng, (B, K, Nh)).astype(one.real)
        ca, cb = one.to_device(cnd), many.to_device(cnd)
    for e in (one, many):
        e.set_state(x0)
    for _ in range(T):
        one.control_tick(ca, K=K)
    if ca is None:
        many.control_ticks(T, K)
    else:
        many.control_tick(cb, K=K, T=T)
    ll = assert_kernel(many, "k_ticks")
    assert ll["variant"] == {"generated": 0, "streamed": 4, "RQL quad-nomix": 16 | 1, "disturbed": 0}[what], ll
    assert one.last_launch(N.KERNEL_ACTOR)["kernel"] != "k_ticks"
    if what == "disturbed":
        assert_kernel(one, "k_sim_dist", kind=N.KERNEL_SIM)
        assert np.std(many.get_field(N.FIELD_DISTURB)) > 0
    _same(many, one, fields, (key, what))
    assert N.lib().rcg_tick_count(many._h) == N.lib().rcg_tick_count(one._h) == T
    assert np.any(many.get_field(N.FIELD_ACCUM) != 0) and np.any(many.get_state() != x0.astype(many.real))
    if what == "RQL quad-nomix":
        assert not np.allclose(many.get_field(N.FIELD_W_CRITIC), 1.0)
    one.close()
    many.close()


@pytest.mark.parametrize("key", KEYS)
def test_rql_ticks_per_launch_stay_refused_under_the_disturbance(reg, key):
    from rcognita_amd import _native as N

    meta, z = load_f17()
    S, p = corner(key), key + "_r_"
    B, K = 64, 16
    e = _engine(reg, key, "f32", B, 5, z[f"{key}_R1_diag"], mode="RQL", critic_struct="quad-nomix", Ncritic=4, buffer_size=6,
                is_disturb=True, pars_disturb=[z[p + "sigma"], z[p + "mu"], z[p + "tau"]])
    e.set_state(S.rand_states(np.random.default_rng(9), B))
    e.control_tick(None, K=K)
    assert e.last_launch(N.KERNEL_SIM)["kernel"] == "k_sim_dist"
    snap = _snapshot(e, CRITIC_FIELDS + ["FIELD_DISTURB", "FIELD_SUBSTEP_IDX"])
    assert N.lib().rcg_control_ticks(e._h, 3, K) == N.ERR_UNSUPPORTED
    assert "disturbance" in N.last_error(e._h)
    _unchanged(e, snap, "RQL control_ticks under the disturbance")
    e.close()


# ---- 9. the mirror classes on C2 ---------------------------------------------------------------------------------------------------
def test_mirror_classes_on_c2_against_the_restated_loop(reg):
    """A System subclass with hip_policy, the Simulator and CtrlOptPred(mode="MPC") for 20 steps against the restated loop: its own
    RK4 of the state, out() of it (dim_output 1) and the argmin of the restated _actor_cost (the tolerances of
    test_hip_user_system.py::test_pendulum_drop_in_loop_against_the_oracle_loop)."""
    from rcognita_amd.controllers import CtrlOptPred
    from rcognita_amd.simulator import Simulator
    from rcognita_amd.systems import System

    meta, z = load_f17()
    S = corner("C2")

    class CornerC2(System):
        hip_policy = S.source

    sys_ = CornerC2(sys_type="diff_eqn", dim_state=5, dim_input=2, dim_output=1, dim_disturb=0, pars=S.pars, ctrl_bnds=S.bnds)
    assert CornerC2._sys_id == reg["C2"]["sys_id"] and sys_.dim_output == 1 and CornerC2._hip_info["dy"] == 1
    rng = np.random.default_rng(91)
    x0 = S.rand_states(rng, 1)[0]
    N_, dt = 5, 0.05
    cand = S.rand_actions(rng, (64, N_))
    R1 = z["C2_R1_diag"]
    ctrl = CtrlOptPred(2, 1, mode="MPC", ctrl_bnds=S.bnds, Nactor=N_, sampling_time=dt, pred_step_size=dt, sys_rhs=sys_._state_dyn,
                       sys_out=sys_.out, state_sys=x0, stage_obj_pars=[R1], candidates=cand.reshape(64, N_ * 2))
    sim = Simulator(sys_type="diff_eqn", closed_loop_rhs=sys_.closed_loop_rhs, sys_out=sys_.out, state_init=x0, t0=0, t1=100,
                    dt=dt, max_step=dt / 10, first_step=1e-6, atol=1e-5, rtol=1e-3, is_disturb=0, is_dyn_ctrl=0)
    np.testing.assert_allclose(sys_.out(x0), S.out(x0), rtol=1e-14)
    x_or, u_or = x0.copy(), np.zeros(2)  # (the system holds no action before the first receive_action)
    moved = False
    for k in range(20):
        sim.sim_step()
        t, x, y, _ = sim.get_sim_step_data()
        x_or, _ = sim_substeps(S, x_or[None], u_or[None], 1, dt)
        x_or = x_or[0]
        assert _err(x, x_or) < 1e-9, k
        assert np.shape(y) == (1,) and _err(y, S.out(x_or)) < 1e-9, k
        xs = np.array(ctrl.state_sys, dtype=float)  # the state the loop handed the controller (receive_sys_state)
        a = ctrl.compute_action(t, y)
        J = actor_cost(S, cand[None], np.asarray(y, float)[None], xs[None], R1, 1.0, None, dt)[0]
        u_or = cand[int(np.argmin(J)), 0].copy()
        np.testing.assert_allclose(a, u_or, rtol=0, atol=1e-12, err_msg=str(k))
        moved = moved or float(np.max(np.abs(x - x0))) > 1e-3
        sys_.receive_action(a)
        ctrl.receive_sys_state(sys_._state)
    assert moved
