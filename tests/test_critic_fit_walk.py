"""The inputs of tests/test_hip_critic_fit_walk.py, chosen and justified on the CPU (not ``gpu`` marked), and the float64 oracle's
critic fit against the minimiser its definition promises.

The critic fit is "the unique minimiser of 1/2 |A w - b|^2 + mu/2 |w - w_init|^2 in the box" (oracle/rcg_oracle.py::
critic_fit_single), computed by a primal active-set walk that exists once in Python and six times on the device.  Device against
oracle compares the walk with itself, and on the suite's usual inputs (random states and actions, W_PREV on [0.5, 1.5], the
structure's uniform box, w_init = 1) the walk takes one iteration and touches no bound on three structures out of five.  This file

* builds, from a seed, ONE batch per (structure, TD rows) in which envs of eight stack families sit next to each other
  (``walk_batch``), and six boxes / start points to fit it in (``walk_box``) - the box is configuration, so one per handle;
* counts what the oracle's walk does on them (``critic_fit_single(trace=...)``) and asserts that every branch of the walk is
  taken in the family that is there for it, and that a (structure, rows) batch mixes one-iteration walks with long ones;
* compares the oracle's result with ``critic_fit_exact`` - the minimiser in 50-digit arithmetic, KKT-verified - in the
  REGULARISED objective F: gap = (F(w) - F(w*)) / F(clip(w_init)), measured (``GAP_MEASURED``, profiles/critic_fit_walk.txt,
  written by oracle/experiments/critic_fit_walk_profile.py) and asserted at four times the measured worst, the factor covering
  seeds not drawn here.

Branches no input reaches - the pivot floor, the iteration cap, the safeguard on finite data - are named in the profile and in
DESIGN.md section 7 as defensive; no test here pretends to cover them.  The ``blocked`` mask is REACHED (pinned weights: a
released weight is pushed straight back by a zero-length step) but redundant on every input found: the push-back sets the weight's
``at_hi`` flag to the side its multiplier points to, which already satisfies the sign test, and without the skip all 648 fits of
the cases that block a variable end on the same bits.  Its counters are asserted non-zero to show that the line ran - on the
device too -, not that it matters; zero-length steps WITHOUT a pin (the tight box) never block.

Long walks.  The walk fixes or releases one variable per iteration, so its length grows with the number of weights: W_PREV on
+-1e3 gives up to 67 iterations at 35 weights and 8-17 at 6-11 weights.  Where the stack families alone do not reach 20
iterations (3 dc if that is smaller) the batch carries ONE more env of the W_PREV family, drawn from a seed that a search over
seeds found (``LONG_WALK_SEED``; W_PREV on +-1e5, which puts the minimiser on a vertex of the box): still an input from a seed."""
import numpy as np
import pytest

from oracle import rcg_oracle as O
from tests.critic_fit_walk_inputs import (BOX_FAMILIES, CASES, CELLS, DC, F_EVAL_EPS, GAP_FACTOR_ORACLE, GAP_MEASURED, GPU_CASES,
                                          STACK_FAMILIES, long_walk_need, walk_cfg_kw, walk_reference)


# ---------------------------------------------------------------------------------------------------------------------
# (a) what the walk does on these inputs
# ---------------------------------------------------------------------------------------------------------------------
def _count(ref, key, fams=None):
    sel = range(len(ref.traces)) if fams is None else [e for e in range(len(ref.traces)) if STACK_FAMILIES[ref.fam[e]] in fams]
    return sum(ref.traces[e][key] for e in sel)


@pytest.mark.parametrize("name,cs,m", CELLS)
def test_a_batch_mixes_one_iteration_walks_with_long_ones(name, cs, m):
    """In the preset box: the suite's family still takes one iteration somewhere in the batch, next to walks of at least 20
    iterations (3 dc if that is smaller), fixes at both bounds and releases - on the form that serves this row count."""
    ref = walk_reference(name, cs, m, "preset")
    assert ref.cfg.dc == DC[(name, cs)]
    assert ref.iters.min() == 1, ref.iters.min()
    assert ref.iters.max() >= long_walk_need(ref.cfg.dc), (ref.iters.max(), long_walk_need(ref.cfg.dc))
    assert ref.iters.max() < O.fit_max_iters(ref.cfg.dc)
    for key in ("fix_lo", "fix_hi") + (("release",) if m > 1 else ()):  # (one row: variables only ever leave the free set)
        assert _count(ref, key) > 0, key
    # the long walks are neighbours of short ones inside a group of 16 envs
    e = int(np.argmax(ref.iters))
    grp = ref.iters[16 * (e // 16):16 * (e // 16) + 16]
    assert grp.min() == 1


@pytest.mark.parametrize("name,cs,m,box", sorted({c[:4] for c in CASES}))
def test_every_branch_is_taken_in_the_family_that_is_there_for_it(name, cs, m, box):
    ref = walk_reference(name, cs, m, box)
    n = len(ref.traces)
    if box == "preset":
        assert _count(ref, "start_bound") == 0
        assert _count(ref, "fix_lo", ("wprev_1e3",)) > 0 and _count(ref, "fix_hi", ("wprev_1e3",)) > 0
        if name != "2tank":  # (the tank's target keeps chi, and with it the trace of A A^T, away from zero)
            assert _count(ref, "mu_floor", ("zero",)) == sum(STACK_FAMILIES[f] == "zero" for f in ref.fam)
        assert _count(ref, "mu_floor") == _count(ref, "mu_floor", ("zero",))
    if box == "tight":
        assert _count(ref, "fix_lo") > 0 and _count(ref, "fix_hi") > 0 and _count(ref, "release") > 0
        assert _count(ref, "blocked") == 0  # (zero-length steps happen here too, but never on the variable just released)
    if box in ("pinned_third", "pinned_all"):
        assert _count(ref, "start_bound") == n
        for key in ("zero_step", "blocked", "skip_blocked"):  # (blocked / skip_blocked: the line runs - it is redundant here, module docstring)
            assert _count(ref, key) > 0, key
        if box == "pinned_all":  # nothing can move: every fix is a zero-length step on a variable just released
            assert _count(ref, "zero_step") == _count(ref, "fix_lo") + _count(ref, "fix_hi") == _count(ref, "release")
    if box in ("graded", "init_outside"):  # the walk starts with nothing free
        assert _count(ref, "start_bound") == n
        assert _count(ref, "release") > 0
    # the defensive branches (module docstring): not reached by any input here
    for key in ("pivot_floor", "cap", "safeguard"):
        assert _count(ref, key) == 0, key


# ---------------------------------------------------------------------------------------------------------------------
# (b) the oracle against the exact minimiser
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cs,m,box,dtype", CASES)
def test_oracle_fit_against_the_exact_minimiser(name, cs, m, box, dtype):
    ref = walk_reference(name, cs, m, box, dtype)
    w = ref.w_or
    assert np.all(w >= ref.lo) and np.all(w <= ref.hi)
    pinned = ref.lo == ref.hi
    np.testing.assert_array_equal(w[:, pinned], np.broadcast_to(ref.lo[pinned], w[:, pinned].shape))
    assert len(ref.envs) >= 16 and ref.envs.max() >= 64 and len({int(f) for f in ref.fam[ref.envs]}) == len(STACK_FAMILIES)
    gaps = np.array([ref.gap[e] for e in ref.envs])
    worst = int(ref.envs[np.argmax(gaps)])
    print(f"{name} {cs} m={m} {box} {dtype}: worst gap {gaps.max():.3e} (env {worst}, {STACK_FAMILIES[ref.fam[worst]]}), "
          f"min {gaps.min():.3e}")
    assert gaps.min() >= -F_EVAL_EPS, gaps.min()
    assert gaps.max() <= GAP_FACTOR_ORACLE * GAP_MEASURED[box], (gaps.max(), worst)


def test_exact_minimiser_is_independent_of_its_guess_and_verifies_itself():
    """critic_fit_exact from the oracle's active set, from "everything free" and from "everything on its lower bound" ends on the
    same point; against scipy's bounded-variable least squares on the augmented system it agrees to that solver's accuracy."""
    from scipy.optimize import lsq_linear

    for name, cs, m, box in (("2tank", "quad-lin", 3, "preset"), ("3wrobot", "quad-nomix", 8, "graded"),
                             ("3wrobotNI", "quad-mix", 11, "tight")):
        ref = walk_reference(name, cs, m, box)
        dc = ref.cfg.dc
        for e in (1, 2, 4, 9):
            ex = ref.exact[e]
            for guess in ((np.ones(dc, bool), np.zeros(dc, bool)), (np.zeros(dc, bool), np.zeros(dc, bool))):
                ex2 = O.critic_fit_exact(ref.A[e], ref.b[e], ref.w0, ref.lo, ref.hi, guess=guess)
                np.testing.assert_array_equal(ex2.w, ex.w)
            mu = float(ex.mu)
            Aa = np.vstack([ref.A[e], np.sqrt(mu) * np.eye(dc)])
            ba = np.concatenate([ref.b[e], np.sqrt(mu) * ref.w0])
            r = lsq_linear(Aa, ba, bounds=(ref.lo, ref.hi), method="bvls", tol=1e-15, max_iter=4000)
            Fs = float(ex.objective(np.clip(r.x, ref.lo, ref.hi)) - ex.objective(ex.w_mp))  # (bvls leaves the box by an ulp)
            assert Fs >= 0.0 and Fs <= 1e-6 * float(ref.F0[e]), (name, e, Fs)
    with pytest.raises(ArithmeticError):
        O.critic_fit_exact(np.array([[np.nan, 1.0]]), np.array([1.0]), np.ones(2), np.zeros(2), np.ones(2))


def test_tracing_leaves_the_fit_bit_for_bit():
    for name, cs, m, box in (("2tank", "quadratic", 3, "pinned_third"), ("3wrobotNI", "quad-mix", 8, "init_outside")):
        ref = walk_reference(name, cs, m, box)
        w = O.critic_fit(ref.cfg, ref.wp, ref.ob, ref.ab, w_init=ref.w0, lo=ref.lo, hi=ref.hi)
        np.testing.assert_array_equal(w, ref.w_or)
        st = []
        O.critic_fit(ref.cfg, ref.wp[:8], ref.ob[:8], ref.ab[:8], w_init=ref.w0, lo=ref.lo, hi=ref.hi, stats=st)
        assert st == [t["iters"] for t in ref.traces[:8]]
    ref = walk_reference("2tank", "quadratic", 3, "preset")
    np.testing.assert_array_equal(O.critic_fit(ref.cfg, ref.wp, ref.ob, ref.ab), ref.w_or)  # the defaults are the preset box


# ---------------------------------------------------------------------------------------------------------------------
# rcg_create refuses a box the fit cannot walk in (before it touches a device)
# ---------------------------------------------------------------------------------------------------------------------
def test_create_refuses_an_empty_or_non_finite_critic_box():
    import ctypes

    from rcognita_amd import _native as N
    from tests.helpers import engine_cfg

    L = N.lib()

    def create(mode, edit):
        c = engine_cfg("2tank", 4, "f64", **dict(walk_cfg_kw("quadratic", 3), mode=O.MODE_IDS[mode])).to_native()
        edit(c)
        h = ctypes.c_void_p()
        rc = L.rcg_create(ctypes.byref(c), ctypes.byref(h))
        err = L.rcg_last_error(None).decode()
        if rc == N.OK:
            L.rcg_destroy(h)
        return rc, err

    def setter(field, i, v):
        def edit(c):
            getattr(c, field)[i] = v
        return edit

    def inverted(c):
        c.w_min[4], c.w_max[4] = 2.0, 1.0

    for mode in ("RQL", "SQL"):
        rc, err = create(mode, inverted)
        assert rc == N.ERR_BAD_ARG and "w_min[4]" in err and "w_max[4]" in err, err
        for field in ("w_min", "w_max", "w_init"):
            for v in (float("nan"), float("inf"), -float("inf")):
                rc, err = create(mode, setter(field, 5, v))
                assert rc == N.ERR_BAD_ARG and f"{field}[5]" in err and "finite" in err, (field, v, err)
    # legal: a pinned weight, a start outside the box, junk beyond dim_critic, and anything at all on an MPC handle - these get past
    # the argument checks (to a handle on a machine with a GPU, to "no device" on one without)
    past = (N.OK, N.ERR_NO_DEVICE)

    def pin(c):
        c.w_min[2] = c.w_max[2] = 0.25

    assert create("RQL", pin)[0] in past
    assert create("RQL", setter("w_init", 0, 1e6))[0] in past
    assert create("RQL", setter("w_min", 6, float("nan")))[0] in past  # (dim_critic = 6: entry 6 is not a weight)
    assert create("MPC", inverted)[0] in past
