"""k_actor_dma's tile hand-over and shared rollout prefix (rcg_actor_dma.hpp), on the GPU: the shapes that take its different
paths - horizons shorter than the prefix (Nactor = 1, 2) and beyond it, full and ragged tiles, one and several tiles per env,
several envs per wave with a ragged last wave, a tick split over two launches (env_lo / env_hi), the one-step state lag,
per-env parameters, NaN / inf rows, large headings - on the three systems in both element widths.  Every case asserts the
kernel the library reports; decisions are compared with the oracle through oracle.parity at the suite's tolerances (1e-11 in
f64, 1e-5 in f32, tie-aware best_idx) and, where rcg_control_tick_n(T = 1) serves the shape, bit for bit with it."""
import numpy as np
import pytest

from oracle import parity as PAR
from oracle import rcg_oracle as O
from tests.helpers import SYSTEMS, TOL, assert_kernel, both, rand_actions, rand_states

pytestmark = pytest.mark.gpu

DTYPES = ["f32", "f64"]
FIELDS = ("FIELD_STATE", "FIELD_STATE_PREV", "FIELD_ACTION", "FIELD_ACCUM", "FIELD_BEST_J", "FIELD_BEST_IDX", "FIELD_STEP_IDX")


def _variant(N, gamma):
    return N.DMA_MPC_G1 if gamma == 1.0 else N.DMA_MPC


def _operator_and_argmin(eng, cfg, x, cand, dtype, what, pars=None):
    """J of every row against the oracle (NaN exactly where the oracle's is not finite), the kernel's argmin = numpy's on its
    own costs (ties -> lower index, NaN = +inf), the winner's first action."""
    B = x.shape[0]
    dc = eng.to_device(cand)
    J = eng.actor_cost(dc)
    x64, c64 = x.astype(np.float64), cand.astype(np.float64)
    J_or = O.actor_cost(c64, x64[:, None, :], x64[:, None, :], cfg) if pars is None else None
    if J_or is not None:
        fin = np.isfinite(J_or)
        assert np.array_equal(np.isfinite(J), fin), what
        scale = np.max(np.abs(np.where(fin, J_or, 0.0)), axis=1, keepdims=True)
        scale = np.broadcast_to(np.where(scale > 0, scale, 1.0), J.shape)
        err = float(np.max(np.abs(J - J_or)[fin] / scale[fin]))
        print(f"{what}: operator max rel err {err:.3e}")
        assert err <= TOL[dtype], (what, err)
    act, bj, bi = eng.actor_argmin(dc)
    Jc = np.where(np.isnan(J), np.inf, J)
    np.testing.assert_array_equal(bi, np.argmin(Jc, axis=1).astype(np.int32), err_msg=what)
    np.testing.assert_array_equal(bj, Jc[np.arange(B), bi], err_msg=what)
    ok = np.isfinite(bj)
    np.testing.assert_array_equal(act[ok], cand[np.arange(B), bi, 0, :][ok], err_msg=what)
    return dc


def _tick_n1(eng, dc, K):
    """rcg_control_tick_n with T = 1 (Engine.control_tick sends T = 1 to rcg_control_tick)."""
    from rcognita_amd import _native as N

    keep = []
    pc, K = eng._cand(dc, keep, K)
    N.check(N.lib().rcg_control_tick_n(eng._h, pc, K, 1), eng._h)
    eng.synchronize()


def _closed_loop(name, B, dtype, K, x, cand, ticks, what, variant_gamma=1.0, pars=None, **kw):
    """`ticks` control ticks on k_actor_dma, every env and tick against the oracle as a map from the same inputs; a twin handle
    takes the same ticks through rcg_control_tick_n(T = 1), a third through one call with T = ticks: the same bits."""
    from rcognita_amd import _native as N

    eng, cfg = both(name, B, dtype, **kw)
    twin, _ = both(name, B, dtype, **kw)
    for e in (eng, twin):
        if pars is not None:
            e.set_field(N.FIELD_PARS, pars.astype(e.real))
        e.set_state(x)
    p64 = None if pars is None else pars.astype(eng.real).astype(np.float64)
    env = O.new_batch(cfg, x.astype(np.float64), pars=p64) if p64 is not None else O.new_batch(cfg, x.astype(np.float64))
    dc, dt = eng.to_device(cand), twin.to_device(cand)
    rep = PAR.TickReport()
    lag = bool(kw.get("ref_lag"))
    for t in range(ticks):
        eng.control_tick(dc, K=K)
        assert_kernel(eng, "k_actor_dma", _variant(N, variant_gamma))
        env = PAR.check_tick(cfg, env, cand.astype(np.float64), PAR.device_fields(eng, N, with_prev=lag), tol=TOL[dtype],
                             report=rep, what=f"{what} t={t}")
        _tick_n1(twin, dt, K)
    print(f"{what}: {rep.as_dict()}")
    # ... and a third takes them in ONE call (T = ticks): k_ticks where it serves the handle - the independent kernel that is
    # pinned bit for bit against this one - else the library's loop of single ticks
    many, _ = both(name, B, dtype, **kw)
    if pars is not None:
        many.set_field(N.FIELD_PARS, pars.astype(many.real))
    many.set_state(x)
    many.control_tick(many.to_device(cand), K=K, T=ticks)
    print(f"{what}: T = {ticks} in one call ran on {many.last_launch(N.KERNEL_ACTOR)['kernel']}")
    for f in FIELDS:
        np.testing.assert_array_equal(twin.get_field(getattr(N, f)), eng.get_field(getattr(N, f)), err_msg=f"{what} {f}")
        np.testing.assert_array_equal(many.get_field(getattr(N, f)), eng.get_field(getattr(N, f)), err_msg=f"{what} {f} (T)")
    np.testing.assert_array_equal(eng.get_field(N.FIELD_STEP_IDX), np.full(B, ticks, np.int32))
    return eng, cfg


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", [256, 100, 36])  # whole tiles (64, 128 or 256 rows per tile, by row length); ragged; one ragged tile
@pytest.mark.parametrize("Nh", [1, 2, 3, 10, 20])
@pytest.mark.parametrize("name", SYSTEMS)
def test_horizons_and_tiles(name, Nh, K, dtype):
    """Nactor = 1 (no step), 2 (one step: the shared trig of the start only), 3 (the whole prefix, nothing behind it), 10, 20;
    K a multiple of the tile, K = 100 (full tiles + a ragged one, or one ragged tile of four rows per lane) and K = 36.  The
    discounted instance (DMA_MPC) takes every other case."""
    from rcognita_amd import _native as N

    gamma = 1.0 if (Nh + K // 4) % 2 else 0.93
    rng = np.random.default_rng(1000 * Nh + K)
    B = 67
    what = f"{name} N={Nh} K={K} {dtype} gamma={gamma}"
    eng, cfg = both(name, B, dtype, n_actor=Nh, gamma=gamma)
    x = rand_states(rng, name, B).astype(eng.real)
    cand = rand_actions(rng, name, (B, K, Nh)).astype(eng.real)
    cand[3, K - 1] = cand[3, 1]  # an exact tie across tiles / lanes: the lower index wins
    eng.set_state(x)
    _operator_and_argmin(eng, cfg, x, cand, dtype, what)
    assert_kernel(eng, "k_actor_dma", _variant(N, gamma))
    _closed_loop(name, B, dtype, K, x, cand, 2, what, variant_gamma=gamma, n_actor=Nh, gamma=gamma)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,B,K,Nh", [("3wrobot", 16384 + 5, 36, 3), ("3wrobot", 32768 + 3, 64, 2), ("3wrobotNI", 16384 + 1, 100, 2),
                                         ("2tank", 32768 + 7, 36, 4)])
def test_batch_that_is_no_multiple_of_the_envs_per_wave(name, B, K, Nh, dtype):
    """From 16 384 envs on a wave owns 2, 4 ... consecutive envs and adopts one after the other; the last wave owns fewer."""
    rng = np.random.default_rng(B + K)
    what = f"{name} B={B} K={K} N={Nh} {dtype}"
    x = rand_states(rng, name, B)
    x = x.astype(np.float32 if dtype == "f32" else np.float64)
    cand = rand_actions(rng, name, (B, K, Nh)).astype(x.dtype)
    eng, _ = _closed_loop(name, B, dtype, K, x, cand, 2, what, n_actor=Nh)
    ll = assert_kernel(eng, "k_actor_dma")
    assert ll["envs_per_wave"] > 1 and B % ll["envs_per_wave"] != 0, ll


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,K,Nh", [("3wrobot", 100, 10), ("3wrobot", 64, 2), ("3wrobotNI", 256, 3), ("2tank", 36, 20)])
def test_state_lag_and_per_env_parameters(name, K, Nh, dtype):
    """RCG_FLAG_REF_LAG: the rollout starts from STATE_PREV while y_0 is the observation - the shared prefix is built from
    the former, the shared cost terms of y_0 from the latter.  Per-env parameters: the derived values are recomputed for every
    env a wave adopts."""
    from rcognita_amd import _native as N

    rng = np.random.default_rng(K + Nh)
    B = 16384 + 11  # two envs per wave: adoption of a second env inside the tile loop
    kw = dict(n_actor=Nh, ref_lag=True)
    pars = None
    if name != "3wrobotNI":  # (the kinematic robot has no parameters)
        kw["per_env_pars"] = True
        pars = (np.stack([rng.uniform(5, 20, B), rng.uniform(0.5, 2, B)], axis=-1) if name == "3wrobot"
                else np.asarray([18.4, 24.4, 1.3, 1.0, 0.2])[None] * rng.uniform(0.8, 1.25, (B, 5)))
    x = rand_states(rng, name, B).astype(np.float32 if dtype == "f32" else np.float64)
    cand = rand_actions(rng, name, (B, K, Nh)).astype(x.dtype)
    eng, _ = _closed_loop(name, B, dtype, K, x, cand, 3, f"{name} K={K} N={Nh} {dtype} lag + pars", pars=pars, **kw)
    assert eng.last_launch(N.KERNEL_ACTOR)["envs_per_wave"] > 1


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,K,Nh", [("3wrobot", 100, 10), ("3wrobotNI", 64, 3), ("2tank", 256, 5)])
def test_rows_with_nan_and_inf(name, K, Nh, dtype):
    """A NaN or +-inf anywhere in a row makes its cost NaN or inf: never selected unless nothing else is there (then index 0,
    +inf); the neighbours in the tile and the env's shared prefix are not disturbed."""
    from rcognita_amd import _native as N

    rng = np.random.default_rng(K)
    B = 70
    eng, cfg = both(name, B, dtype, n_actor=Nh)
    x = rand_states(rng, name, B).astype(eng.real)
    cand = rand_actions(rng, name, (B, K, Nh)).astype(eng.real)
    cand[1, 0, 0, 0] = np.nan           # the first action of the first row
    cand[2, K - 1, Nh - 1, -1] = np.nan  # the last real of the env's rows
    cand[3, 5, 0, 0] = np.inf
    cand[4, 6, Nh // 2, 0] = -np.inf
    cand[5] = np.nan                    # every row
    cand[6, :, 0, 0] = np.inf           # every cost +inf
    eng.set_state(x)
    dc = _operator_and_argmin(eng, cfg, x, cand, dtype, f"{name} K={K} {dtype} nan/inf")
    assert_kernel(eng, "k_actor_dma", N.DMA_MPC_G1)
    act, bj, bi = eng.actor_argmin(dc)
    assert bi[5] == 0 and np.isinf(bj[5]) and bj[5] > 0
    assert bi[1] != 0 and bi[2] != K - 1
    assert np.isinf(bj[6]) and bi[6] == 0
    J = eng.actor_cost(dc)
    clean = np.delete(np.arange(B), [1, 2, 3, 4, 5, 6])
    assert np.all(np.isfinite(J[clean])) and np.all(np.isfinite(np.delete(J[1], 0)))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,K,Nh", [("3wrobot", 256, 10), ("3wrobot", 36, 2), ("3wrobotNI", 100, 10)])
def test_headings_of_a_thousand_radians(name, K, Nh, dtype):
    """alpha_0 = +-1e3 rad and beyond: the shared trig of the start and of the first step goes through the same argument
    reduction as the rollout's own (f32: at the accuracy of float32 at that magnitude - the state is rounded to float32 before
    either side sees it)."""
    from rcognita_amd import _native as N

    rng = np.random.default_rng(Nh)
    B = 64
    eng, cfg = both(name, B, dtype, n_actor=Nh)
    x = rand_states(rng, name, B)
    x[:, 2] = rng.uniform(-1, 1, B) * 1e3
    x[0, 2], x[1, 2] = 1e3, -1e3
    x = x.astype(eng.real)
    cand = rand_actions(rng, name, (B, K, Nh)).astype(eng.real)
    eng.set_state(x)
    _operator_and_argmin(eng, cfg, x, cand, dtype, f"{name} K={K} N={Nh} {dtype} 1e3 rad")
    assert_kernel(eng, "k_actor_dma", N.DMA_MPC_G1)
    _closed_loop(name, B, dtype, K, x, cand, 2, f"{name} K={K} N={Nh} {dtype} 1e3 rad", n_actor=Nh)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,mode,cs,B,K,Nh", [
    ("3wrobot", "RQL", "quad-nomix", 3072 + 5, 100, 10),
    ("3wrobotNI", "SQL", "quad-mix", 2560, 64, 3),
    ("2tank", "RQL", "quadratic", 5000, 36, 20),
])
def test_a_handle_that_splits_its_tick(name, mode, cs, B, K, Nh, dtype):
    """rcg_set_tick_parts(2): the decision of each half of the batch is a launch of its own with env_lo / env_hi set.  Bit for
    bit the unsplit tick, which is checked against the oracle (ticks with a critic fit: the suite's tolerance for them,
    1e-9 in f64 - the weights solve a regularised least-squares problem, tests/test_hip_critic.py)."""
    from rcognita_amd import _native as N

    kw = dict(mode=O.MODE_IDS[mode], critic_struct=O.CRITIC_IDS[cs], n_critic=4, buffer_size=8, n_actor=Nh, gamma=0.95)
    rng = np.random.default_rng(B)
    x0 = rand_states(rng, name, B)
    one, cfg = both(name, B, dtype, **kw)
    two, _ = both(name, B, dtype, **kw)
    two.set_tick_parts(2)
    x0 = x0.astype(one.real)
    env = O.new_batch(cfg, x0.astype(np.float64))
    for e in (one, two):
        e.set_tick_parts(2 if e is two else 1)
        e.set_state(x0)
    rep = PAR.TickReport()
    for t in range(4):
        cand = rand_actions(rng, name, (B, K, Nh)).astype(one.real)
        for e in (one, two):
            e.control_tick(cand)
        for e, split in ((one, False), (two, True)):
            ll = e.last_launch(N.KERNEL_ACTOR)
            assert ll["kernel"] == "k_actor_dma" and ll["split"] == split, ll
        env = PAR.check_tick(cfg, env, cand.astype(np.float64), PAR.device_fields(one, N, critic=True),
                             tol=1e-9 if dtype == "f64" else 1e-5, report=rep, what=f"{name} {mode} {dtype} t={t}")
    print(rep.as_dict())
    for f in FIELDS + ("FIELD_W_CRITIC", "FIELD_W_PREV", "FIELD_OBS_BUF", "FIELD_ACT_BUF"):
        np.testing.assert_array_equal(two.get_field(getattr(N, f)), one.get_field(getattr(N, f)), err_msg=f)
