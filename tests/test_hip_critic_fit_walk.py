"""The critic fit's active-set walk on the device, driven through every branch (``gpu`` marked).  The inputs - eight stack families
side by side in one batch of 70 envs, six boxes / start points - and what the walk does on them are justified on the CPU in
tests/test_critic_fit_walk.py; here every device form of the walk fits them:

  k_critic_fit<.., 3>      <= 3 TD rows, fewer than 9 weights     k_critic_fit_ml<.., 3>   <= 3 rows, 9 weights or more: four lanes
  k_critic_fit<.., 8>      4 .. 8 rows, one lane per env          k_critic_fit_gen         more rows: stack and factor in HBM
  k_ticks_mem              its critic phase, with one lane and with four lanes per env (T ticks in one launch)

The yardsticks are independent of the walk: feasibility, "never worse than the start", and the gap of the REGULARISED objective to
``critic_fit_exact`` (the KKT-verified minimiser in 50-digit arithmetic).  The oracle twin is compared in ``w`` only where the
CPU file's criterion says the minimiser is well separated.  The box and the start point of a handle are fields of ``rcg_cfg``
that ``EngineConfig.to_native`` fills with the structure's preset; ``BoxedConfig`` overwrites them."""

import numpy as np
import pytest

from oracle import rcg_oracle as O
from tests.helpers import assert_kernel, rand_states, rel_err_norm
from tests.critic_fit_walk_inputs import (B_WALK, BOX_FAMILIES, DC, GAP_FACTOR_DEVICE, GAP_MEASURED, GPU_CASES, NAN_ENVS, REAL,
                                          STACK_FAMILIES, boxed_engine, walk_batch, walk_box, walk_reference)
from tests.test_hip_critic import _load_buffers

pytestmark = pytest.mark.gpu

def expected_form(m, dc):
    """(four lanes, any-m, rows of the register instance) of rcg_last_launch's variant word (rcg_sysops.hpp::fit_plan)."""
    return (m <= 3 and dc >= 9, m > 8, 3 if m <= 3 else (0 if m > 8 else 8))


def assert_form(eng, m, dc):
    from rcognita_amd import _native as N

    ll = assert_kernel(eng, "k_critic_fit", kind=N.KERNEL_CRITIC)
    v = ll["variant"]
    assert (bool(v & 1024), bool(v & 2048), (v >> 4) & 15) == expected_form(m, dc), ll
    assert ll["envs_per_wave"] == (16 if v & 1024 else 64), ll


def test_the_cases_cover_every_single_tick_form_with_every_box():
    """Every (box, dtype) pair on each of the four single-tick forms."""
    seen = {}
    for name, cs, m, box, dtype in GPU_CASES:
        seen.setdefault(expected_form(m, DC[(name, cs)]), set()).add((box, dtype))
    assert len(seen) == 4, seen.keys()
    for form, got in seen.items():
        assert got == {(b, d) for b in BOX_FAMILIES for d in ("f32", "f64")}, (form, got)


def _float_rounding_bounds(ref, e, w32, G):
    """What storing ``w`` as float may add, env ``e``: with |dw_i| <= 2^-24 |w_i| (``w32`` = the stored values),
    (dF, dJc): F(w + dw) - F(w*) <= G + L + Q + 2 sqrt(G Q) where G bounds F(w) - F(w*) of the unrounded feasible w, L = sum |g*_i|
    |dw_i| with g* the exact minimiser's gradient, Q = 1/2 |A dw|^2 + mu/2 |dw|^2 (for feasible w: g*.(w - w*) >= 0, so F(w) -
    F(w*) >= 1/2 (w - w*)^T H (w - w*), which bounds the cross term by Cauchy-Schwarz); and Jc(w + dw) - Jc(w) <= |r|.|A||dw| + 1/2
    (|A||dw|)^2 with r = A (w + dw) - b."""
    ex = ref.exact[e]
    A, b = ref.A[e], ref.b[e]
    dw = np.abs(w32) * 2.0 ** -24 * (1 + 2.0 ** -20)
    ws = ex.w
    mu = float(ex.mu)
    g = A.T @ (A @ ws - b) + mu * (ws - ref.w0)  # float64 evaluation of g*: its own error is second order here
    gs = np.abs(A).T @ np.abs(A @ ws - b) + mu * np.abs(ws - ref.w0)
    L = float(np.sum((np.abs(g) + 1e-12 * gs) * dw))
    Adw = np.abs(A) @ dw
    Q = 0.5 * float(Adw @ Adw) + 0.5 * mu * float(dw @ dw)
    r = np.abs(A @ w32 - b)
    return G + L + Q + 2.0 * np.sqrt(G * Q), float(r @ Adw) + 0.5 * float(Adw @ Adw)


@pytest.mark.parametrize("name,cs,m,box,dtype", GPU_CASES)
def test_device_walk_against_the_exact_minimiser(name, cs, m, box, dtype):
    from rcognita_amd import _native as N

    ref = walk_reference(name, cs, m, box, dtype)
    cfg, B, dc = ref.cfg, B_WALK, ref.cfg.dc
    real = REAL[dtype]
    eng = boxed_engine(name, B, dtype, cs, m, (ref.w0, ref.lo, ref.hi))
    # ---- launch 1: two envs with a NaN in the buffers, in between walks of every length ----
    ob_nan = ref.ob.copy()
    ob_nan[NAN_ENVS[0], 1, 0] = np.nan
    ob_nan[NAN_ENVS[1], 0, -1] = np.nan
    _load_buffers(eng, N, ob_nan, ref.ab, ref.wp)
    eng.critic_update(do_fit=True)
    assert_form(eng, m, dc)
    w_nan = eng.get_field(N.FIELD_W_CRITIC)
    # ---- launch 2: the same batch, every env finite ----
    _load_buffers(eng, N, ref.ob, ref.ab, ref.wp)
    eng.critic_update(do_fit=True)
    assert_form(eng, m, dc)
    np.testing.assert_array_equal(eng.get_field(N.FIELD_OBS_BUF), ref.ob.astype(real))  # push_vec
    np.testing.assert_array_equal(eng.get_field(N.FIELD_ACT_BUF), ref.ab.astype(real))
    w_dev = eng.get_field(N.FIELD_W_CRITIC)
    np.testing.assert_array_equal(eng.get_field(N.FIELD_W_PREV), w_dev)
    assert w_dev.dtype == real
    # NaN buffers: the safeguard's clip(w_init) as bits; every other env as if its neighbour had been finite
    keep = np.ones(B, bool)
    keep[list(NAN_ENVS)] = False
    np.testing.assert_array_equal(w_nan[~keep], np.broadcast_to(ref.w_start.astype(real), (2, dc)))
    np.testing.assert_array_equal(w_nan[keep], w_dev[keep])

    w = w_dev.astype(np.float64)
    assert np.all(np.isfinite(w))
    # feasible: exactly in float64; in float32 within the rounding of the bounds themselves (rounding is monotone)
    lo_r, hi_r = ref.lo.astype(real), ref.hi.astype(real)
    assert np.all(w_dev >= lo_r) and np.all(w_dev <= hi_r)
    pinned = ref.lo == ref.hi
    np.testing.assert_array_equal(w_dev[:, pinned], np.broadcast_to(lo_r[pinned], (B, int(pinned.sum()))))

    tolw = (1e-6 if m <= dc else 5e-5) if dtype == "f64" else 2e-4  # (tests/test_hip_critic.py: more rows than weights, f32 storage)
    ld = np.longdouble  # (both costs the same way, in the widest host type: the comparison below is not about this file's rounding)
    cost = lambda v: 0.5 * np.sum((np.einsum("eri,ei->er", ref.A.astype(ld), v.astype(ld)) - ref.b.astype(ld)) ** 2, axis=1)
    Jc, J0 = cost(w), cost(np.broadcast_to(ref.w_start, w.shape))
    worst = dict(gap=0.0, limit=0.0, env=-1, dw=0.0)  # the largest gap relative to F(clip(w_init)), for the record
    n_sep = 0
    for e in range(B):
        have_exact = e in ref.exact
        G = GAP_FACTOR_DEVICE * GAP_MEASURED[box] * float(ref.F0[e]) if have_exact else 0.0
        dF, dJ = (G, 0.0)
        if dtype == "f32" and have_exact:
            dF, dJ = _float_rounding_bounds(ref, e, w[e], G)
        elif dtype == "f32":
            Adw = np.abs(ref.A[e]) @ (np.abs(w[e]) * 2.0 ** -24 * (1 + 2.0 ** -20))
            dJ = float(np.abs(ref.A[e] @ w[e] - ref.b[e]) @ Adw) + 0.5 * float(Adw @ Adw)
        # never worse than the start (the header's promise); 1e-12: this file's own float64 evaluation of the two costs
        assert Jc[e] <= J0[e] * (1 + 1e-12) + dJ, (e, STACK_FAMILIES[ref.fam[e]], Jc[e], J0[e])
        if not have_exact:
            continue
        # the regularised objective against the exact minimiser
        num = float(ref.exact[e].objective(w[e]) - ref.Fstar[e])
        if dtype == "f64":
            assert num >= -1e-40 * float(ref.F0[e]), (e, num)  # feasible, so not below the minimum
        if ref.F0[e] > 0 and num / float(ref.F0[e]) > worst["gap"]:
            worst.update(gap=num / float(ref.F0[e]), limit=dF / float(ref.F0[e]), env=e, iters=ref.traces[e]["iters"])
        assert num <= dF, (e, STACK_FAMILIES[ref.fam[e]], num, dF, float(ref.F0[e]), ref.traces[e]["iters"])
        # the oracle twin in w: only where the minimiser is well separated - the oracle's walk and the exact one end on the same
        # active set and the walk took no zero-length step (test_critic_fit_walk.py::WalkReference.well_separated); elsewhere the
        # device may end on another vertex of (almost) equal cost and only the objective yardsticks above apply
        if ref.well_separated(e):
            n_sep += 1
            err = rel_err_norm(w[e], ref.w_or[e])
            worst["dw"] = max(worst["dw"], err)
            assert err < tolw, (e, STACK_FAMILIES[ref.fam[e]], err)
    print(f"{name} {cs} m={m} {box} {dtype}: {len(ref.exact)} exact envs, {n_sep} well separated, worst {worst}")
    if box not in ("pinned_third", "pinned_all"):
        assert n_sep >= len(ref.exact) // 2, n_sep


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name,cs,m", [("2tank", "quadratic", 8), ("2tank", "quad-lin", 3)])
def test_ticks_in_one_launch_walk_like_single_ticks(name, cs, m, dtype):
    """k_ticks_mem's critic phase - one lane per env (8-row instance) and four lanes per env (9 weights, 3 rows) - on the pinned-
    third box with the builder's batch (eight stack families side by side): T = 4 ticks in one launch leave the weights and both
    buffers as four single ticks do, bit for bit (rcg_control_ticks' header), and the first of those fits goes through the
    zero-length-step branches."""
    from rcognita_amd import _native as N

    B, T, K = B_WALK, 4, 9
    cfg, ob, ab, wp, fam = walk_batch(name, cs, m, seed=7, dtype=dtype)
    dc = cfg.dc
    box = walk_box("pinned_third", cs, dc)
    x0 = rand_states(np.random.default_rng(31 + m), name, B)
    engs = []
    for _ in range(2):
        e = boxed_engine(name, B, dtype, cs, m, box)
        e.set_state(x0)
        e.set_field(N.FIELD_OBS_BUF, ob)
        e.set_field(N.FIELD_ACT_BUF, ab)
        e.set_field(N.FIELD_W_PREV, wp)
        e.set_field(N.FIELD_W_CRITIC, wp)
        engs.append(e)
    one, many = engs
    one.control_tick(None, K=K)
    assert_form(one, m, dc)
    # the first tick's fit, on the stack the push left (the builder's rows moved up by one, the new observation last): the oracle's
    # walk there takes the degenerate branches, and where the minimiser is well separated (as in the test above) the device agrees in w
    rb = lambda a: a.astype(np.float64)
    w1 = rb(one.get_field(N.FIELD_W_CRITIC))
    ob1, ab1 = rb(one.get_field(N.FIELD_OBS_BUF)), rb(one.get_field(N.FIELD_ACT_BUF))
    np.testing.assert_array_equal(ob1[:, :-1], ob[:, 1:])
    traces = []
    w_or = O.critic_fit(cfg, wp, ob1, ab1, w_init=box[0], lo=box[1], hi=box[2], trace=traces)
    for key in ("zero_step", "blocked", "skip_blocked", "fix_lo", "fix_hi", "release"):
        assert sum(t[key] for t in traces) > 0, key
    A1, b1 = O.critic_td_system(wp, ob1, ab1, cfg)
    pinned = box[1] == box[2]
    tolw = (1e-6 if m <= dc else 5e-5) if dtype == "f64" else 2e-4  # (as test_hip_critic.py)
    n_sep = 0
    for e, t in enumerate(traces):
        if t["zero_step"] or not np.all(np.isfinite(A1[e])):
            continue
        ex = O.critic_fit_exact(A1[e], b1[e], box[0], box[1], box[2], guess=(t["free"], t["at_hi"]))
        if np.array_equal(t["free"] & ~pinned, ex.free) and np.array_equal(t["at_hi"] & ~pinned & ~t["free"], ex.at_hi):
            n_sep += 1
            assert rel_err_norm(w1[e], w_or[e]) < tolw, (e, STACK_FAMILIES[fam[e]])
    assert n_sep > 0
    for _ in range(T - 1):
        one.control_tick(None, K=K)
    many.control_ticks(T, K)
    ll = assert_kernel(many, "k_ticks")
    # bit 4: k_ticks_mem.  rcg_last_launch's word has NO bit for the lanes of its critic phase (rcg_sysops.hpp::ticks_mem_plan): which
    # of the two instances ran follows from (dc >= 9 and rows <= 3) alone, the same rule that gave the single ticks the form
    # assert_form saw above - what is asserted here is that the two parametrisations lie on either side of that rule
    assert ll["variant"] & 16, ll
    assert expected_form(m, dc)[0] == ((name, cs, m) == ("2tank", "quad-lin", 3))
    assert one.last_launch(N.KERNEL_ACTOR)["kernel"] != "k_ticks"
    for f in ("FIELD_W_CRITIC", "FIELD_W_PREV", "FIELD_OBS_BUF", "FIELD_ACT_BUF", "FIELD_STATE", "FIELD_ACTION"):
        np.testing.assert_array_equal(many.get_field(getattr(N, f)), one.get_field(getattr(N, f)), err_msg=f)
    w = many.get_field(N.FIELD_W_CRITIC)
    assert np.all(w >= box[1].astype(w.dtype)) and np.all(w <= box[2].astype(w.dtype)) and np.all(w[:, pinned] == 1.0)
    assert not np.array_equal(w, w1.astype(w.dtype))  # the later ticks refitted
