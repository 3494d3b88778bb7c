"""Run-time-compiled systems at the corners of DS, DU, DY, NP, DD (tests/user_systems.py: C1 .. C4): what their registrations
report - hipRTC compiles without a device, so these run on CPU - the NumPy twin against the reference's own results
(tests/golden/F17_user_system_corners.npz, tools/gen_user_system_corners_fixture.py), the twin's adjoints against central
differences, and the two properties the GPU tests (test_hip_user_system_corners.py) lean on: every index of every input moves
the cost, and the float32 decisions they compare are far from ties."""
import numpy as np
import pytest

from rcognita_amd import _native as N
from tests.test_user_system_critic_register import critic, critic_cost, critic_regressor, td_system
from tests.user_systems import (ARGMIN_SHAPES, CORNERS, KEYS, MPC_CASES, STRUCTS, actor_cost, argmin_costs, argmin_gap, case_cost,
                                corner, dim_critic, f17_case, load_f17, make_policy, regressor, rhs_full, search_inputs,
                                search_weights, sim_substeps)

CRITIC_TAGS = tuple(f"{m}_{cs.replace('-', '_')}" for m in ("RQL", "SQL") for cs in STRUCTS)
F32_TOL = 1e-5  # the GPU tests' float32 tolerance on costs (tests/helpers.py::TOL)


@pytest.fixture(scope="module")
def infos():
    return {k: corner(k).register() for k in KEYS}


def _int(fn, sid, n):
    v = [N.C.c_int32(-1) for _ in range(n)]
    assert fn(sid, *(N.C.byref(x) for x in v)) == N.OK
    return tuple(x.value for x in v)


@pytest.mark.parametrize("key", KEYS)
def test_each_corner_registers_and_reports_its_dimensions(infos, key):
    name, ds, du, np_, dy, dd = CORNERS[key]
    info, L = infos[key], N.lib()
    sid = info["sys_id"]
    assert sid >= N.SYS_USER_BASE
    assert _int(L.rcg_system_info, sid, 4) == (ds, du, np_, 1)
    assert _int(L.rcg_system_output_info, sid, 3) == (ds if dy is None else dy, int(dy is not None), int(dy is not None))
    assert _int(L.rcg_system_disturb_dim, sid, 1) == (dd,)
    assert _int(L.rcg_system_has_critic, sid, 1) == _int(L.rcg_system_has_search, sid, 1) == _int(L.rcg_system_has_ticks, sid, 1) == (1,)
    assert info["has_critic"] and info["has_search"] and info["has_ticks"] and info["has_jac"]
    assert (info["dy"], info["has_out"], info["has_out_jac"], info["dd"]) == (ds if dy is None else dy, dy is not None, dy is not None, dd)
    assert N.SYS_DIMS[sid] == (ds, du, np_) and N.sys_dy(sid) == (ds if dy is None else dy) and N.DIM_DISTURB[sid] == dd


def test_the_corners_carry_the_critic_sizes_no_other_system_has():
    """dc = 2, 8, 21, 27 come from legal user dimensions only; 8 is the last size on the one-lane fit, 11 the first beyond."""
    dcs = {k: sorted({dim_critic(cs, corner(k).dy, corner(k).du) for cs in STRUCTS}) for k in KEYS}
    assert dcs == {"C1": [2, 3, 5], "C2": [3, 5, 6, 9], "C3": [4, 8, 10, 14], "C4": [6, 11, 21, 27]}
    assert dim_critic("quad-mix", 2, 2) == 8 and dim_critic("quad-mix", 5, 1) == 11 and dim_critic("quad-mix", 1, 2) == 5
    meta, _ = load_f17()
    for k in KEYS:
        assert meta["systems"][k]["dim_critic"] == {cs: dim_critic(cs, corner(k).dy, corner(k).du) for cs in STRUCTS}


def test_make_policy_serves_every_legal_dimension():
    """The family is generic: the sources differ where the dimensions do, and an NP = 0 policy reads no parameter."""
    src, S = make_policy("FamilyProbe", 2, 2, 0, dy=4, dd=2)
    assert "p[" not in src and "DY = 4" in src and "DD = 2" in src and S.dy == 4 and S.pars == []
    src, S = make_policy("FamilyProbe2", 3, 1, 2)
    assert "DY" not in src and "disturb" not in src and S.dy == 3
    x = np.random.default_rng(0).uniform(-2, 2, (7, 3))
    assert np.array_equal(S.out(x), x)


# ---- the twin against the reference ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", KEYS)
def test_twin_reproduces_the_reference_rhs_full_and_out(key):
    _, z = load_f17()
    S, p = corner(key), key + "_r_"
    a = S.clip(z[p + "action"])
    np.testing.assert_array_equal(a, z[p + "action_clipped"])
    assert np.any(a != z[p + "action"])
    d, dq = rhs_full(S, z[p + "state"], z[p + "disturb"], a, z[p + "xi"], z[p + "sigma"], z[p + "mu"], z[p + "tau"])
    ref = z[p + "rhs_full"]
    assert ref.shape == (64, S.ds + S.dd)
    assert np.max(np.abs(d - ref[:, :S.ds]) / np.maximum(1.0, np.abs(ref[:, :S.ds]))) <= 1e-13
    assert np.max(np.abs(dq - ref[:, S.ds:]) / np.maximum(1.0, np.abs(ref[:, S.ds:]))) <= 1e-13
    y = S.out(z[p + "state"])
    assert y.shape == (64, S.dy) and np.max(np.abs(y - z[key + "_o_out"]) / np.maximum(1.0, np.abs(y))) <= 1e-13
    # the disturbance enters through the state (and, DD = 2, the action): without those factors the rows are other ones
    flat = S.rhs(z[p + "state"], a) + 0.0
    flat[:, S.ds - 1] += z[p + "disturb"][:, 0]
    assert np.median(np.abs(flat[:, S.ds - 1] - ref[:, S.ds - 1])) > 0.05


@pytest.mark.parametrize("key", KEYS)
def test_twin_reproduces_the_reference_actor_cost_critic_and_critic_cost(key):
    meta, z = load_f17()
    S = corner(key)
    for tag in MPC_CASES + CRITIC_TAGS:
        c = f17_case(meta, z, key, tag)
        assert len(c["J"]) == 16 and not np.allclose(c["ys"], S.out(c["xs"]))  # (observation != out(state_sys))
        J = case_cost(S, c, meta, c["seq"][:, None])[:, 0]
        assert np.max(np.abs(J - c["J"]) / np.maximum(1.0, np.abs(c["J"]))) <= 1e-12, (key, tag)
    tg, R1, g, nc = z[f"{key}_target"], z[f"{key}_R1_diag"], meta["gamma_critic"], meta["Ncritic"]
    for cs in STRUCTS:
        k = cs.replace("-", "_")
        ob, ab, w, wp = (z[f"{key}_d_{k}_{s}"] for s in ("obs_buf", "act_buf", "w", "w_prev"))
        for i in range(16):
            yc, uc, wc = z[f"{key}_c_{k}_obs"][i], z[f"{key}_c_{k}_act"][i], z[f"{key}_c_{k}_w"][i]
            Q = z[f"{key}_c_{k}_Q"][i]
            assert abs(critic(cs, yc, uc, wc, tg) - Q) <= 1e-12 * max(1.0, abs(Q)), (key, cs, i)
            # the batched regressor of user_systems.py is the one of test_user_system_critic_register.py
            np.testing.assert_allclose(regressor(cs, np.concatenate([yc - tg, uc]), yc, uc), critic_regressor(cs, yc, uc, tg), rtol=1e-15)
            Jc = z[f"{key}_d_{k}_Jc"][i]
            assert abs(critic_cost(cs, w[i], wp[i], ob[i], ab[i], nc, g, R1, tg) - Jc) <= 1e-12 * max(1.0, abs(Jc)), (key, cs, i)
            A, b = td_system(cs, wp[i], ob[i], ab[i], nc, g, R1, tg)
            r = A @ w[i] - b
            assert abs(0.5 * float(r @ r) - Jc) <= 1e-11 * max(1.0, abs(Jc)), (key, cs, i)
    # (s): SLSQP's optimum is a cost of the same function, below its start
    xs = z[f"{key}_s_state"]
    J = actor_cost(S, z[f"{key}_s_seq_opt"][:, None], S.out(xs), xs, R1, 1.0, None, meta["pred_step_size"])[:, 0]
    assert np.max(np.abs(J - z[f"{key}_s_J_opt"]) / np.maximum(1.0, J)) <= 1e-12
    assert np.all(z[f"{key}_s_J_opt"] <= z[f"{key}_s_J_init"])


# ---- the adjoints ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", KEYS)
def test_jac_T_and_out_jac_T_agree_with_central_differences(key):
    S = corner(key)
    rng = np.random.default_rng(17)
    n, e = 32, 1e-5
    x, u = S.rand_states(rng, n), S.rand_actions(rng, (n,))
    lam, gy = rng.uniform(-1, 1, (n, S.ds)), rng.uniform(-1, 1, (n, S.dy))
    p = np.array(S.pars) * rng.uniform(0.8, 1.2, (n, S.np)) if S.np else None
    ax, bu = S.jac_T(x, u, lam, p)
    gx = S.out_jac_T(x, gy)
    fd_ax, fd_bu, fd_gx = np.zeros_like(ax), np.zeros_like(bu), np.zeros_like(gx)
    for k in range(S.ds):
        dx = np.zeros(S.ds)
        dx[k] = e
        fd_ax[:, k] = np.sum(lam * (S.rhs(x + dx, u, p) - S.rhs(x - dx, u, p)), axis=-1) / (2 * e)
        fd_gx[:, k] = np.sum(gy * (S.out(x + dx) - S.out(x - dx)), axis=-1) / (2 * e)
    for j in range(S.du):
        du_ = np.zeros(S.du)
        du_[j] = e
        fd_bu[:, j] = np.sum(lam * (S.rhs(x, u + du_, p) - S.rhs(x, u - du_, p)), axis=-1) / (2 * e)
    for a, b in ((ax, fd_ax), (bu, fd_bu), (gx, fd_gx)):
        assert np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))) <= 1e-6


# ---- every index matters -------------------------------------------------------------------------------------------------------
def _moves(S, c, meta, pars):
    """For each single entry of (state, observation, action of step 0 and of step N - 2, parameter, target, R1) moved by 1e-3: the
    largest |dJ| and |dJ| / max(|J|, 1) over the F17 points of case `c` -> {what: (absolute, relative)}."""
    cand = c["seq"][:, None]
    J0 = case_cost(S, c, meta, cand, pars=pars)[:, 0]
    out = {}

    def note(what, J):
        d = np.abs(J[:, 0] - J0)
        out[what] = (float(d.max()), float(np.max(d / np.maximum(np.abs(J0), 1.0))))

    for i in range(S.ds):
        xs = c["xs"].copy()
        xs[:, i] += 1e-3
        note(f"state {i}", case_cost(S, c, meta, cand, xs=xs, pars=pars))
    for i in range(S.dy):
        ys = c["ys"].copy()
        ys[:, i] += 1e-3
        note(f"obs {i}", case_cost(S, c, meta, cand, ys=ys, pars=pars))
    for step in (0, cand.shape[2] - 2):
        for j in range(S.du):
            cd = cand.copy()
            cd[:, :, step, j] += 1e-3
            note(f"action {step},{j}", case_cost(S, c, meta, cd, pars=pars))
    for k in range(S.np):
        p = np.array(pars, dtype=float)
        p[k] += 1e-3
        note(f"par {k}", case_cost(S, c, meta, cand, pars=p))
    n = S.dy + S.du
    if c["target"] is not None:
        for i in range(S.dy):
            t = c["target"].copy()
            t[i] += 1e-3
            note(f"target {i}", case_cost(S, c, meta, cand, pars=pars, target=t))
    for i in range(n):
        for j in range(n):
            if c["R1"][i, j] == 0.0:
                continue  # (a diagonal R1: its zeros are the structure, not entries)
            R = c["R1"].copy()
            R[i, j] += 1e-3
            note(f"R1 {i},{j}", case_cost(S, c, meta, cand, pars=pars, R1=R))
    return out


@pytest.mark.parametrize("key", KEYS)
def test_every_index_matters(key):
    """A kernel that dropped, swapped or mis-strided one component must show far above the float32 tolerance: moving any single
    entry by 1e-3 moves _actor_cost of the F17 points by at least 1e3 x that tolerance (1e-2).  The GPU tolerance is relative to
    the cost (100 .. 1700 here), so the move is also held to >= the tolerance relative to max(|J|, 1): a kernel that loses an
    index changes that input by its whole size, a thousand times this step, and the cost is smooth in it - the loss then shows
    at about 1e3 x the tolerance.  The full-R1 case with a target carries every entry of R1 and of the target; the disturbance
    components are checked on rhs_full (they do not enter a rollout)."""
    meta, z = load_f17()
    S = corner(key)
    worst = {}
    for tag in ("mpc_g1", "mpc_full_tgt"):
        c = f17_case(meta, z, key, tag)
        for what, (a, r) in _moves(S, c, meta, S.pars).items():
            worst[(tag, what)] = (a, r)
            assert a >= 1e3 * F32_TOL, (key, tag, what, a)
            assert r >= F32_TOL, (key, tag, what, r)
    lo = min(worst, key=lambda k: worst[k][0])
    print(f"{key}: {len(worst)} entries; smallest move {worst[lo][0]:.3e} (relative {worst[lo][1]:.3e}) at {lo}")
    p = key + "_r_"
    a = S.clip(z[p + "action"])
    args = (z[p + "xi"], z[p + "sigma"], z[p + "mu"], z[p + "tau"])
    d0, _ = rhs_full(S, z[p + "state"], z[p + "disturb"], a, *args)
    for k in range(S.dd):
        q = z[p + "disturb"].copy()
        q[:, k] += 1e-3
        d1, _ = rhs_full(S, z[p + "state"], q, a, *args)
        assert np.max(np.abs(d1 - d0)) >= 1e3 * 2e-5 / 100, (key, k)  # (1e-3 through |cos x0| or 1 + 0.5 u0: 10 x the rhs tolerance)
        assert np.count_nonzero(np.any(d1 != d0, axis=0)) == 1  # (it enters one row)


# ---- float32 near ties ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", KEYS)
def test_the_float32_argmin_batches_are_far_from_ties(key):
    """Every batch the GPU file takes an argmin of (user_systems.py::argmin_costs: both MPC cost forms from the state and from a
    caller's observation, the discounted form with per-env parameters): the seeds (ARGMIN_SEEDS) leave every env's
    best-to-second gap above the float32 tolerance, and a numpy float32 evaluation changes no more than 5 % of the winners.  The
    GPU file asserts the float32 index wherever an env's gap exceeds 4 x the tolerance and follows the device's choice elsewhere."""
    for B, K, Nh in ARGMIN_SHAPES:
        J64, J32 = argmin_costs(key, B, K, Nh), argmin_costs(key, B, K, Nh, dtype=np.float32)
        assert len(J64) == (5 if corner(key).np else 4)
        for what in J64:
            gap = float(argmin_gap(J64[what]).min())
            share = float(np.mean(np.argmin(J64[what], axis=1) != np.argmin(J32[what], axis=1)))
            print(f"{key} K={K} N={Nh} {what}: {100 * share:.1f} % change their winner in float32, smallest gap {gap:.2e}")
            assert gap > F32_TOL, (key, K, Nh, what, gap)
            assert share <= 0.05, (key, K, Nh, what)


def float32_search_dry_run(key, Nh, B=29, K=192, rounds=3, tag="mpc_g1", seed=7, step=None, from_state=False):
    """Share of envs whose winning sequence changes when the costs of the search (the oracle's own candidates rounded to float32,
    the GPU test's seed and STEP_IDX - the env index, or `step` for all) are computed in numpy float32 instead of float64
    (test_user_system_search_register.py::float32_dry_run for any du), and the smallest best-to-second gap of the last round.
    `from_state`: the first rcg_control_tick_search of the GPU file - one env step from the start, then y_0 = out(STATE)."""
    import types

    from oracle import rcg_oracle as O
    from oracle import search_oracle as SO

    meta, z = load_f17()
    S = corner(key)
    c = f17_case(meta, z, key, tag)
    x, xl = search_inputs(key, B)
    r = lambda a: np.asarray(a).astype(np.float32).astype(np.float64)  # noqa: E731
    x, ys = r(x), r(S.out(xl))
    if from_state:
        x, _ = sim_substeps(S, x, np.broadcast_to(S.bnds[:, 0] / 10.0, (B, S.du)), 1, 0.01)
        x = r(x)
        ys = S.out(x)
    w = None if c["cs"] is None else r(search_weights(key, c["cs"], B))
    cfg = types.SimpleNamespace(n_actor=Nh, du=S.du, ctrl_bnds=S.bnds)
    ids = np.arange(B)
    steps = ids if step is None else np.full(B, step)
    out, gap = [], None
    for dtype in (np.float64, np.float32):
        cen = np.broadcast_to(S.bnds[:, 0] / 10.0, (B, Nh, S.du)).astype(float)
        for rd in range(rounds):
            cand = r(SO.candidates_sample(cfg, seed, ids, np.zeros(B, int), steps, K, rd, centre=cen))
            J = np.asarray(case_cost(S, c, meta, cand, xs=x, ys=ys, w=w, dtype=dtype), dtype=np.float64)
            _, bi = O.argmin_first(J)
            cen = cand[ids, bi]
        gap = float(argmin_gap(J).min()) if gap is None else gap
        out.append(cen)
    return float(np.mean(np.any(out[0] != out[1], axis=(1, 2)))), gap


@pytest.mark.parametrize("key", KEYS)
def test_the_float32_search_seeds_are_far_from_ties(key):
    """The float32 search cases of the GPU file cap the share of envs that leave the float64 replay's sequence at 20 %: their
    seeds are chosen so that this dry run changes under 10 %, half the cap.  (A search keeps its incumbent as candidate 0 of the
    next round, so late rounds hold near-equal costs by construction: the gap is printed, the share is what is held.)"""
    for Nh in (5, 10, 7):
        share, gap = float32_search_dry_run(key, Nh)
        print(f"{key} N={Nh}: {100 * share:.1f} % of the envs change their winner in float32, last round's smallest gap {gap:.2e}")
        assert share < 0.10, (key, Nh)
    share, gap = float32_search_dry_run(key, 5, K=64, rounds=2, seed=99, step=0, from_state=True)
    print(f"{key} first tick of the tick search: {100 * share:.1f} % change their winner, smallest gap {gap:.2e}")
    assert share < 0.10, key
    if key == "C3":  # the RQL search cases
        for cs in ("quad-mix", "quad-lin"):
            share, _ = float32_search_dry_run(key, 5, tag="RQL_" + cs.replace("-", "_"))
            print(f"{key} RQL {cs}: {100 * share:.1f} % of the envs change their winner in float32")
            assert share < 0.10, (key, cs)
