"""One freeze rule on every tick path (GPU).  An env whose state turns non-finite inside a simulation step is frozen: STATE and
STATE_PREV stay at the last finite values, bit 0 of STATUS is set and the env is never stepped again (include/rcg.h,
RCG_FIELD_STATUS).  The rule is written out wherever an env is stepped - k_sim, the fused step of k_actor_dma_packed,
k_critic_fit*, loop_head (k_loop, k_actor_opt's LOOP instance), k_ticks / k_ticks_pk / k_ticks_mem - and most of these kernels
share work across the lanes of a wave (packed tiles with a segmented argmin, the shared rollout prefix of k_actor_dma, four lanes
per env in k_critic_fit_ml, 16 envs per wave in k_actor_opt, the readlane hand-over of k_ticks_pk).  The oracle has no freeze, so
the contract is pinned differentially on three handles of identical configuration and candidates:

  bad    bad-now envs at 0, 7, 63, 64 and B - 1, a NaN-on-entry env at 20, an env whose STATUS is preset to 1 at 33
  clean  the same batch with benign states at the bad indices
  pre    as bad, the bad-now envs' STATUS already 1

  P1  isolation: every other env of bad equals clean, bit for bit, in every field - no exclusions
  P2  freezing in this tick = frozen before it: every field of the bad-now envs in bad equals pre
  P3  the frozen env itself: not stepped (STATE, STATE_PREV as set, STATUS 1 and nobody else's), still decided for from its
      frozen state (= rcg_actor_argmin on a fresh handle holding that state: index 0 and +inf in MPC), counted (STEP_IDX), charged
      (ACCUM += stage_obj(y, ACTION) * sampling_time: +inf on the tank, finite on the robot, whose huge component has weight 0)
      and, in RQL / SQL, pushed (frozen observation, held action) and fitted (= rcg_critic_update on the same buffers)

The states come from tests/test_freeze_states.py, which justifies them on the CPU.  Every test asserts the kernel it claims
through rcg_last_launch.  B = 150: 16-env, 64-env and 8-env-tile waves all end in a ragged wave.  Measured on an MI355X: the
whole file (107 cases) in 2.1 s, the slowest case 0.2 s.  No path broke the rule; no kernel was changed."""
import numpy as np
import pytest

from oracle import rcg_oracle as O
from tests.helpers import PRESETS, TOL, assert_kernel, both, rand_actions, rand_states
from tests.test_freeze_states import REAL, bad_later_state, freeze_batch

pytestmark = pytest.mark.gpu

B, NH = 150, 5
DTYPES = ["f32", "f64"]
MPC_FIELDS = ["FIELD_STATE", "FIELD_STATE_PREV", "FIELD_STATUS", "FIELD_ACTION", "FIELD_ACCUM", "FIELD_STEP_IDX", "FIELD_BEST_J",
              "FIELD_BEST_IDX"]
CRITIC_FIELDS = MPC_FIELDS + ["FIELD_W_CRITIC", "FIELD_W_PREV", "FIELD_OBS_BUF", "FIELD_ACT_BUF"]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same(a, b, msg):
    np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=msg)


def _snap(eng, fields):
    from rcognita_amd import _native as N

    return {f: eng.get_field(getattr(N, f)) for f in fields}


class Trio:
    """bad / clean / pre handles of one case and the batch they hold."""

    def __init__(self, name, dtype, batch=B, seed=7, later=False, extra_bad=(), **kw):
        from rcognita_amd import _native as N

        self.name, self.dtype, self.B, self.kw = name, dtype, batch, kw
        xb, xc, now, nan_at, pre_at, later_at = freeze_batch(name, dtype, batch, seed, later=later)
        for i in extra_bad:
            xb[i] = xb[now[0]]
        now = np.array(sorted(set(now) | set(extra_bad)))
        self.x_bad, self.x_clean, self.now, self.nan_at, self.pre_at, self.later_at = xb, xc, now, nan_at, pre_at, later_at
        self.critic = kw.get("mode", O.MODE_MPC) != O.MODE_MPC
        self.fields = list(CRITIC_FIELDS if self.critic else MPC_FIELDS)
        rng = np.random.default_rng(seed + 1)
        self.pars = np.stack([rng.uniform(5, 20, batch), rng.uniform(0.5, 2, batch)], axis=-1) if kw.get("per_env_pars") else None
        self.h = {}
        self.kws = dict(n_actor=NH)
        self.kws.update(kw)
        for which in ("bad", "clean", "pre"):
            e, self.cfg = both(name, batch, dtype, **self.kws)
            e.set_state(xc if which == "clean" else xb, also_init=False)
            e.set_field(N.FIELD_STATE_INIT, xc)  # benign: an episode reset brings every env back
            st = np.zeros(batch, np.uint32)
            st[pre_at] = 1
            if which == "pre":
                st[now] = 1
            e.set_field(N.FIELD_STATUS, st)
            if self.pars is not None:
                e.set_field(N.FIELD_PARS, self.pars)
            self.h[which] = e
        self.real = self.h["bad"].real
        # envs whose state differs between bad and clean; envs frozen from the first tick on
        self.differ = np.array(sorted(set(now) | {nan_at} | ({later_at} if later_at is not None else set())))
        self.frozen = np.array(sorted(set(now) | {nan_at, pre_at}))

    def fresh(self):
        """A fourth handle of the same configuration (P3's reference calls)."""
        from rcognita_amd import _native as N

        e, _ = both(self.name, self.B, self.dtype, **self.kws)
        if self.pars is not None:
            e.set_field(N.FIELD_PARS, self.pars)
        return e

    def run(self, fn):
        """fn(engine) on all three handles; returns the three results."""
        return {k: fn(e) for k, e in self.h.items()}

    def close(self):
        for e in self.h.values():
            e.close()

    # ---- P1 / P2 ------------------------------------------------------------------------------------------------------
    def check_isolation(self, fields=None, what=""):
        bad, clean, pre = (_snap(self.h[k], fields or self.fields) for k in ("bad", "clean", "pre"))
        others = np.setdiff1d(np.arange(self.B), self.differ)
        for f in bad:
            _same(bad[f][others], clean[f][others], f"P1 {what} {f}: a healthy env differs from the clean batch")
            _same(bad[f][self.now], pre[f][self.now], f"P2 {what} {f}: freezing in this tick != frozen before it")
            # (and the rest of pre is bad's: the preset flag of one env changes nobody else)
            _same(bad[f], pre[f], f"P2 {what} {f}: the whole batch")
        return bad

    # ---- P3 -----------------------------------------------------------------------------------------------------------
    def check_frozen(self, ticks, cand, K, got=None, accum0=None, frozen_later=False):
        from rcognita_amd import _native as N

        bad = self.h["bad"]
        got = got or _snap(bad, self.fields)
        fz = self.frozen
        x_set = self.x_bad.astype(self.real)
        _same(got["FIELD_STATE"][fz], x_set[fz], "P3 STATE of a frozen env moved")
        _same(got["FIELD_STATE_PREV"][fz], x_set[fz], "P3 STATE_PREV of a frozen env moved")
        want = np.zeros(self.B, np.uint32)
        want[fz] = 1
        if frozen_later:
            want[self.later_at] = 1
        np.testing.assert_array_equal(got["FIELD_STATUS"], want, err_msg="P3 STATUS")
        np.testing.assert_array_equal(got["FIELD_STEP_IDX"], np.full(self.B, ticks, np.int32), err_msg="P3 STEP_IDX")
        # decided for from the frozen state: rcg_actor_argmin on a fresh handle that holds it
        ref = self.fresh()
        ref.set_field(N.FIELD_STATE, got["FIELD_STATE"])
        ref.set_field(N.FIELD_STATE_PREV, got["FIELD_STATE_PREV"])
        if self.critic:
            ref.set_field(N.FIELD_W_CRITIC, got["FIELD_W_CRITIC"])
        act, bj, bi = ref.actor_argmin(cand, K=K)
        hard = np.array(sorted(set(self.now) | {self.nan_at}))  # non-finite costs: nothing to round
        _same(got["FIELD_ACTION"][hard], act[hard], "P3 ACTION != rcg_actor_argmin from the frozen state")
        _same(got["FIELD_BEST_J"][hard], bj[hard], "P3 BEST_J != rcg_actor_argmin from the frozen state")
        np.testing.assert_array_equal(got["FIELD_BEST_IDX"][fz], bi[fz], err_msg="P3 BEST_IDX")
        _same(got["FIELD_ACTION"][[self.pre_at]], act[[self.pre_at]], "P3 ACTION of the env frozen by the caller")
        np.testing.assert_allclose(got["FIELD_BEST_J"][self.pre_at], bj[self.pre_at], rtol=TOL[self.dtype])
        if not self.critic:
            np.testing.assert_array_equal(bi[hard], 0)
            assert np.all(bj[hard] == np.inf), bj[hard]
        # charged: ACCUM += stage_obj(y, ACTION) * sampling_time every tick, in the handle's dtype.  The decision is the same
        # every tick - same state, same candidates; in RQL / SQL only where the costs are non-finite whatever the weights
        ch = hard if self.critic else fz
        stage = ref.stage_obj(got["FIELD_STATE"][ch], got["FIELD_ACTION"][ch])
        assert stage.dtype == self.real
        with np.errstate(all="ignore"):
            inc = (stage * self.real(self.cfg.sampling_time)).astype(self.real)
            acc = np.zeros(len(ch), self.real) if accum0 is None else accum0[ch].astype(self.real)
            for _ in range(ticks):
                acc = (acc + inc).astype(self.real)
        np.testing.assert_allclose(got["FIELD_ACCUM"][ch], acc, rtol=TOL[self.dtype], err_msg="P3 ACCUM")
        k = list(ch).index(self.now[0])
        if self.name == "2tank":
            assert acc[k] == np.inf, acc[k]
        elif self.name == "3wrobot":
            assert np.isfinite(acc[k]), acc[k]  # (the huge component has weight 0)
        ref.close()
        return got


def _cand(rng, t, K, n_actor=NH):
    return rand_actions(rng, t.name, (t.B, K, n_actor)).astype(t.real)


# ---------------------------------------------------------------------------------------------------------------------
# 1. MPC, streamed candidates
# ---------------------------------------------------------------------------------------------------------------------
def _kw_id(kw):
    return "-".join(f"{k}" for k in kw) or "plain"


STREAMED = [
    # K, kw, kernel, check(ll)
    (40, {}, "k_actor_dma"),
    (40, dict(ref_lag=True), "k_actor_dma"),
    (8, {}, "k_actor_dma_packed"),
    (8, dict(ref_lag=True), "k_actor_dma_packed"),
    (16, {}, "k_actor_dma_packed"),
    (3, {}, "k_actor"),
]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["3wrobot", "2tank"])
@pytest.mark.parametrize("K,kw,kernel", STREAMED, ids=[f"K{K}-{_kw_id(kw)}" for K, kw, _ in STREAMED])
def test_streamed_mpc_tick_freezes_alone(K, kw, kernel, name, dtype):
    from rcognita_amd import _native as N

    t = Trio(name, dtype, **kw)
    cand = _cand(np.random.default_rng(K), t, K)
    ticks = 2  # the second tick starts from the flag the first one set
    t.run(lambda e: [e.control_tick(cand, K=K) for _ in range(ticks)])
    for e in t.h.values():
        ll = assert_kernel(e, kernel)
        if kernel == "k_actor_dma_packed":
            assert ll["variant"] & 16, ll  # the env step ran inside the launch (the fused step)
        else:
            assert_kernel(e, "k_sim", kind=N.KERNEL_SIM)
        if kernel == "k_actor":
            assert ll["variant"] & 4, ll
    if kernel == "k_actor_dma" and name == "3wrobot" and not kw:
        zw = t.h["bad"].last_launch_zero_w()
        assert zw == (0x78 if dtype == "f64" else 0), hex(zw)  # f64: the zero-weight instance
    got = t.check_isolation(what=f"K={K}")
    t.check_frozen(ticks, cand, K, got)
    t.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_streamed_mpc_tick_with_long_rows_freezes_alone(dtype):
    """Nactor = 40 on the robot: rows of 80 reals (> RCG_MAX_ROW) - k_actor's DIRECT form."""
    K, Nh = 8, 40
    t = Trio("3wrobot", dtype, n_actor=Nh)
    cand = _cand(np.random.default_rng(40), t, K, Nh)
    t.run(lambda e: [e.control_tick(cand, K=K) for _ in range(2)])
    for e in t.h.values():
        ll = assert_kernel(e, "k_actor")
        assert ll["variant"] & 16, ll
    got = t.check_isolation(what="DIRECT")
    t.check_frozen(2, cand, K, got)
    t.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_streamed_mpc_tick_with_per_env_parameters_freezes_alone(dtype):
    K = 8
    t = Trio("3wrobot", dtype, per_env_pars=True)
    cand = _cand(np.random.default_rng(41), t, K)
    t.run(lambda e: [e.control_tick(cand, K=K) for _ in range(2)])
    for e in t.h.values():
        assert assert_kernel(e, "k_actor_dma_packed")["variant"] & 16
    got = t.check_isolation(what="per-env pars")
    t.check_frozen(2, cand, K, got)
    t.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. MPC, generated grid
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,K", [("3wrobot", 256), ("3wrobot", 16), ("2tank", 32), ("3wrobotNI", 64)])
def test_generated_grid_tick_freezes_alone(name, K, dtype):
    t = Trio(name, dtype)
    t.run(lambda e: [e.control_tick(None, K=K) for _ in range(2)])
    pk = name == "3wrobot" and K == 256 and dtype == "f32"
    for e in t.h.values():
        if pk:
            assert_kernel(e, "k_ticks", variant=8)  # k_ticks_pk: env step and decision in one launch
        else:
            assert not (assert_kernel(e, "k_actor")["variant"] & 4)
    got = t.check_isolation(what=f"grid K={K}")
    t.check_frozen(2, None, K, got)
    t.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. RQL / SQL ticks
# ---------------------------------------------------------------------------------------------------------------------
CRITIC_CASES = [
    # name, mode, structure, Ncritic, buffer_size, K, decision kernel, (fit rows, four lanes, any-rows form)
    ("2tank", "RQL", "quad-nomix", 4, 6, 40, "k_actor_dma", (3, False, False)),
    ("3wrobot", "SQL", "quad-nomix", 6, 8, 8, "k_actor_dma_packed", (8, False, False)),
    ("2tank", "RQL", "quad-lin", 4, 6, 40, "k_actor_dma", (3, True, False)),       # 9 weights: four lanes per env
    ("3wrobot", "RQL", "quadratic", 4, 6, 40, "k_actor_dma", (3, True, False)),    # 28 weights
    ("2tank", "SQL", "quadratic", 12, 13, 8, "k_actor_dma_packed", (0, False, True)),  # 11 TD rows: k_critic_fit_gen
]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,mode,cs,nc,bs,K,kernel,fit", CRITIC_CASES,
                         ids=[f"{c[0]}-{c[1]}-{c[2]}-m{c[3] - 1}-K{c[5]}" for c in CRITIC_CASES])
def test_critic_mode_tick_freezes_alone(name, mode, cs, nc, bs, K, kernel, fit, dtype):
    from rcognita_amd import _native as N

    t = Trio(name, dtype, mode=O.MODE_IDS[mode], critic_struct=O.CRITIC_IDS[cs], n_critic=nc, buffer_size=bs)
    cand = _cand(np.random.default_rng(nc + K), t, K)
    ticks = 3  # a frozen env's row is pushed again and again, and the fit runs on a buffer that holds it
    # both buffers start full of benign rows (the same in the three handles): every fit is a real one from the first tick on -
    # the TD stack reads the OLDEST rows, which on a fresh handle are zeros for buffer_size ticks
    rb = np.random.default_rng(bs)
    ob0 = np.stack([rand_states(rb, name, t.B) * 0.5 for _ in range(bs)], axis=1)
    ab0 = rand_actions(rb, name, (t.B, bs))
    for e in t.h.values():
        e.set_field(N.FIELD_OBS_BUF, ob0)
        e.set_field(N.FIELD_ACT_BUF, ab0)
    bad = t.h["bad"]
    held, before_last = [], None
    for k in range(ticks):
        if k == ticks - 1:
            before_last = _snap(bad, ["FIELD_OBS_BUF", "FIELD_ACT_BUF", "FIELD_W_CRITIC", "FIELD_W_PREV", "FIELD_ACTION", "FIELD_STATE"])
        held.append(bad.get_field(N.FIELD_ACTION))
        bad.control_tick(cand, K=K)
    for which in ("clean", "pre"):
        for _ in range(ticks):
            t.h[which].control_tick(cand, K=K)
    rows, ml, gen = fit
    for e in t.h.values():
        assert_kernel(e, kernel)
        ll = assert_kernel(e, "k_critic_fit", kind=N.KERNEL_CRITIC)
        v = ll["variant"]
        assert (v >> 4) & 15 == rows and bool(v & 1024) == ml and bool(v & 2048) == gen and (v & 256) and (v & 512), ll
    got = t.check_isolation(what=f"{mode} {cs}")
    t.check_frozen(ticks, cand, K, got)
    # pushed: the frozen observation and the action held over the step, once per tick
    fz = t.frozen
    x_set = t.x_bad.astype(t.real)
    for k in range(ticks):
        r = bs - ticks + k
        _same(got["FIELD_OBS_BUF"][fz, r], x_set[fz], f"P3 pushed observation of tick {k}")
        _same(got["FIELD_ACT_BUF"][fz, r], held[k][fz], f"P3 pushed action of tick {k}")
    # fitted: rcg_critic_update on a handle with the same buffers (start-point convention for non-finite buffers)
    ref = t.fresh()
    ref.set_field(N.FIELD_STATE, before_last["FIELD_STATE"])
    for f in ("FIELD_OBS_BUF", "FIELD_ACT_BUF", "FIELD_W_CRITIC", "FIELD_W_PREV", "FIELD_ACTION"):
        ref.set_field(getattr(N, f), before_last[f])
    ref.critic_update(do_fit=True)
    for f in ("FIELD_W_CRITIC", "FIELD_W_PREV"):
        _same(got[f][fz], ref.get_field(getattr(N, f))[fz], f"P3 {f} != rcg_critic_update on the same buffers")
    assert np.all(np.isfinite(got["FIELD_W_CRITIC"]))
    healthy = np.setdiff1d(np.arange(t.B), np.union1d(t.differ, [t.pre_at]))
    assert not np.allclose(got["FIELD_W_CRITIC"][healthy], 1.0)  # the healthy envs were fitted
    ref.close()
    t.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. T ticks per call = T single ticks, the envs that freeze included
# ---------------------------------------------------------------------------------------------------------------------
TICKS_CASES = [
    # name, K, streamed, kw, variant bits that must be set, dtypes
    ("3wrobot", 64, False, {}, 0, DTYPES),                       # k_ticks, generated
    ("2tank", 32, False, {}, 0, DTYPES),
    ("3wrobot", 16, True, {}, 4, DTYPES),                        # k_ticks, rows staged once and re-walked
    ("2tank", 40, True, {}, 4, DTYPES),
    ("3wrobot", 256, False, {}, 8, ["f32"]),                     # k_ticks_pk
    ("2tank", 32, False, dict(mode=O.MODE_RQL, critic_struct=O.CRITIC_IDS["quad-nomix"], n_critic=4, buffer_size=6), 16, DTYPES),
    ("2tank", 32, False, dict(mode=O.MODE_SQL, critic_struct=O.CRITIC_IDS["quad-lin"], n_critic=4, buffer_size=6), 16, DTYPES),
    ("2tank", 40, True, dict(mode=O.MODE_RQL, critic_struct=O.CRITIC_IDS["quad-lin"], n_critic=4, buffer_size=6), 20, DTYPES),
    ("3wrobot", 16, False, dict(mode=O.MODE_RQL, critic_struct=O.CRITIC_IDS["quadratic"], n_critic=4, buffer_size=6), 16, DTYPES),
]
TICKS_PARAMS = [pytest.param(*c[:5], d, id=f"{c[0]}-K{c[1]}-{'streamed' if c[2] else 'grid'}-{'mem' if c[4] & 16 else ('pk' if c[4] & 8 else 'ticks')}"
                             f"{'-ml' if c[3].get('critic_struct') in (O.CRITIC_IDS['quad-lin'], O.CRITIC_IDS['quadratic']) else ''}-{d}")
                for c in TICKS_CASES for d in c[5]]


@pytest.mark.parametrize("name,K,streamed,kw,bits,dtype", TICKS_PARAMS)
def test_T_ticks_in_one_call_equal_T_single_ticks_with_envs_that_freeze(name, K, streamed, kw, bits, dtype):
    """All fields of all envs as bits, the bad ones included; the one stated exception (rcg.h, rcg_control_ticks): Sys2Tank's
    BEST_J to a rounding.  The tank batch also holds a bad-later env, which freezes in a tick that is not the launch's first."""
    from rcognita_amd import _native as N

    T = 5
    tank = name == "2tank"
    t = Trio(name, dtype, later=tank, **kw)
    one, many = t.h["bad"], t.h["pre"]
    many.set_field(N.FIELD_STATUS, one.get_field(N.FIELD_STATUS))  # two identical bad handles
    cand = _cand(np.random.default_rng(K + T), t, K) if streamed else None
    ca, cb = (one.to_device(cand), many.to_device(cand)) if streamed else (None, None)
    fields = t.fields + ["FIELD_EPISODE_IDX", "FIELD_RETURNS"]

    def compare(what):
        a, b = _snap(one, fields), _snap(many, fields)
        for f in fields:
            if tank and f == "FIELD_BEST_J":
                np.testing.assert_allclose(b[f], a[f], rtol=TOL[dtype], err_msg=f"{what} {f}")
            else:
                _same(b[f], a[f], f"{what} {f}")
        return b

    for _ in range(T):
        one.control_tick(ca, K=K)
    if streamed:
        many.control_tick(cb, K=K, T=T)
    else:
        many.control_ticks(T, K)
    ll = assert_kernel(many, "k_ticks")
    assert ll["variant"] & bits == bits and bool(ll["variant"] & 16) == t.critic and bool(ll["variant"] & 8) == bool(bits & 8), ll
    if t.critic:
        v = one.last_launch(N.KERNEL_CRITIC)["variant"]
        assert bool(v & 1024) == (t.cfg.dc >= 9), v  # four lanes per env in the single ticks' fit <=> in k_ticks_mem's
    got = compare("T ticks")
    want = np.zeros(t.B, np.uint32)
    want[t.frozen] = 1
    if tank:
        n_later = bad_later_state(dtype)[1]
        assert 1 <= n_later < T
        want[t.later_at] = 1
        assert np.all(np.isfinite(got["FIELD_STATE"][t.later_at]))
        assert np.any(got["FIELD_STATE"][t.later_at] != t.x_bad.astype(t.real)[t.later_at])  # it did step before it froze
    np.testing.assert_array_equal(got["FIELD_STATUS"], want)
    np.testing.assert_array_equal(got["FIELD_STEP_IDX"], np.full(t.B, T, np.int32))
    _same(got["FIELD_STATE"][t.frozen], t.x_bad.astype(t.real)[t.frozen], "frozen STATE")
    # an episode reset clears the flag (STATE_INIT is benign): every env steps again, and the two handles still agree
    for e in (one, many):
        e.episode_reset()
    np.testing.assert_array_equal(many.get_field(N.FIELD_STATUS), 0)
    one.control_tick(ca, K=K)
    if streamed:
        many.control_tick(cb, K=K, T=1)
    else:
        many.control_ticks(1, K)
    got = compare("after the reset")
    np.testing.assert_array_equal(got["FIELD_STATUS"], 0)
    assert np.all(np.any(got["FIELD_STATE"] != t.x_clean.astype(t.real), axis=1))  # every env stepped from STATE_INIT
    assert np.all(np.isfinite(got["FIELD_STATE"]))
    t.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. the optimiser, the search and the nominal controller as the decision
# ---------------------------------------------------------------------------------------------------------------------
def _check_action_in_bounds(t, got):
    b = np.array(PRESETS[t.name]["bnds"], dtype=float)
    a = got["FIELD_ACTION"][t.frozen].astype(np.float64)
    assert np.all(np.isfinite(a)), f"a frozen env's ACTION is not finite: {a}"
    assert np.all(a >= b[:, 0]) and np.all(a <= b[:, 1]), a


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
@pytest.mark.parametrize("memory", [0, 4], ids=["sd", "pairs"])
@pytest.mark.parametrize("name,kw", [("3wrobot", {}), ("2tank", {}),
                                     ("2tank", dict(mode=O.MODE_RQL, critic_struct=O.CRITIC_IDS["quadratic"], n_critic=4, buffer_size=6))],
                         ids=["3wrobot-MPC", "2tank-MPC", "2tank-RQL"])
def test_optimiser_tick_freezes_alone(name, kw, memory, warm, dtype):
    iters, ticks = 4, 2
    t = Trio(name, dtype, **kw)

    def go(e):
        e.set_optimizer(memory)
        for _ in range(ticks):
            e.control_tick_opt(iters=iters, warm_start=warm)

    t.run(go)
    for e in t.h.values():
        ll = assert_kernel(e, "k_actor_opt")
        assert bool(ll["variant"] & 4) == (memory > 0), ll
    got = t.check_isolation(fields=t.fields + ["FIELD_ACTION_SQN"], what=f"opt memory={memory} warm={warm}")
    n_iter = got["FIELD_BEST_IDX"]
    assert np.all(n_iter >= 0) and np.all(n_iter <= iters), n_iter
    _check_action_in_bounds(t, got)
    x_set = t.x_bad.astype(t.real)
    _same(got["FIELD_STATE"][t.frozen], x_set[t.frozen], "frozen STATE")
    want = np.zeros(t.B, np.uint32)
    want[t.frozen] = 1
    np.testing.assert_array_equal(got["FIELD_STATUS"], want)
    np.testing.assert_array_equal(got["FIELD_STEP_IDX"], np.full(t.B, ticks, np.int32))
    t.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["3wrobot", "2tank"])
def test_search_tick_freezes_alone(name, dtype):
    ticks = 2
    t = Trio(name, dtype)
    t.run(lambda e: [e.control_tick_search(K=64, rounds=2, warm_start=k > 0) for k in range(ticks)])
    for e in t.h.values():
        assert_kernel(e, "k_actor_search")
    got = t.check_isolation(fields=t.fields + ["FIELD_ACTION_SQN"], what="search")
    _check_action_in_bounds(t, got)
    _same(got["FIELD_STATE"][t.frozen], t.x_bad.astype(t.real)[t.frozen], "frozen STATE")
    want = np.zeros(t.B, np.uint32)
    want[t.frozen] = 1
    np.testing.assert_array_equal(got["FIELD_STATUS"], want)
    np.testing.assert_array_equal(got["FIELD_STEP_IDX"], np.full(t.B, ticks, np.int32))
    t.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["3wrobot", "3wrobotNI"])
def test_nominal_tick_freezes_alone(name, dtype):
    t = Trio(name, dtype)
    t.run(lambda e: [e.control_tick_nominal(0.5) for _ in range(2)])
    for e in t.h.values():
        assert_kernel(e, "k_nominal")
    got = t.check_isolation(what="nominal")
    want = np.zeros(t.B, np.uint32)
    want[t.frozen] = 1
    np.testing.assert_array_equal(got["FIELD_STATUS"], want)
    _same(got["FIELD_STATE"][t.frozen], t.x_bad.astype(t.real)[t.frozen], "frozen STATE")
    t.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. rcg_loop_step = the separate calls, the frozen envs' rows included
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,mode,cs", [("3wrobot", "MPC", "quad-nomix"), ("2tank", "MPC", "quad-nomix"), ("2tank", "RQL", "quadratic"),
                                          ("3wrobot", "SQL", "quad-mix")])
def test_loop_step_with_frozen_envs_equals_the_separate_calls(name, mode, cs, dtype):
    from rcognita_amd import _native as N

    Bs, iters = 32, 4
    crit = mode != "MPC"
    kw = dict(mode=O.MODE_IDS[mode], critic_struct=O.CRITIC_IDS[cs], n_critic=4, buffer_size=6) if crit else {}
    t = Trio(name, dtype, batch=Bs, **kw)
    a, b, c = t.h["bad"], t.h["pre"], t.h["clean"]  # one call, the separate calls, begin + end: three identical bad handles
    for e in (b, c):
        e.set_state(t.x_bad, also_init=False)
        e.set_field(N.FIELD_STATUS, a.get_field(N.FIELD_STATUS))
    cfg = t.cfg
    act = np.tile(cfg.ctrl_bnds[:, 0] / 10.0, (Bs, 1))
    h = cfg.dt_sim
    seen = set()
    for it in range(4):
        decide, push, fit = it % 2 == 1, crit and it >= 1, crit and it >= 2
        ra = a.loop_step(act, h, 1, decide=decide, push=push, fit=fit, iters=iters)
        if decide:
            ll = assert_kernel(a, "k_actor_opt")
            assert bool(ll["variant"] & 8) == (not crit), ll  # MPC: head and tail in the optimiser's own launch (LOOP)
            seen.add("LOOP" if ll["variant"] & 8 else "three launches")
        elif not crit:
            seen.add("k_loop")
        c.loop_step_begin(act, h, 1, decide=decide, push=push, fit=fit, iters=iters)
        rc = c.loop_step_end()
        # the separate calls
        b.set_field(N.FIELD_ACTION, act)
        b.sim_step(1, step=h)
        if push:
            b.critic_update(do_fit=fit)
        xs, st_b = b.get_field(N.FIELD_STATE_PREV), b.get_state()
        if decide:
            a_b, u_b, bj_b, _ = b.actor_optimize(iters=iters, obs=st_b, state_sys=xs)
            b.set_field(N.FIELD_ACTION, a_b)
        else:
            a_b = act.astype(b.real)
        stage_b = b.stage_obj(st_b, a_b)
        for tag, r in (("one call", ra), ("begin + end", rc)):
            st, ac, stage, bj, w = r
            _same(st, st_b.astype(np.float64), f"{tag}: state it={it}")
            _same(ac, np.asarray(a_b, dtype=np.float64), f"{tag}: action it={it}")
            _same(stage, stage_b.astype(np.float64), f"{tag}: stage cost it={it}")
            if decide:
                _same(bj, bj_b.astype(np.float64), f"{tag}: best J it={it}")
            else:
                assert np.all(np.isnan(bj))
            if crit:
                _same(w, b.get_field(N.FIELD_W_CRITIC).astype(np.float64), f"{tag}: weights it={it}")
        fields = ["FIELD_STATE", "FIELD_STATE_PREV", "FIELD_STATUS"] + (
            ["FIELD_W_CRITIC", "FIELD_W_PREV", "FIELD_OBS_BUF", "FIELD_ACT_BUF"] if crit else [])
        sa, sb, sc = _snap(a, fields), _snap(b, fields), _snap(c, fields)
        for f in fields:
            _same(sa[f], sb[f], f"{f} it={it}: one call against the separate calls")
            _same(sc[f], sb[f], f"{f} it={it}: begin + end against the separate calls")
        if decide:
            _same(np.asarray(a.get_field(N.FIELD_ACTION_SQN)).reshape(u_b.shape), u_b, f"ACTION_SQN it={it}")
        act = np.asarray(ra[1], dtype=np.float64).copy()
    assert seen == ({"three launches"} if crit else {"k_loop", "LOOP"}), seen
    want = np.zeros(Bs, np.uint32)
    want[t.frozen] = 1
    np.testing.assert_array_equal(a.get_field(N.FIELD_STATUS), want)
    _same(a.get_state()[t.frozen], t.x_bad.astype(t.real)[t.frozen], "frozen STATE")
    t.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. a tick in two halves, a bad env in each
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,cs", [("2tank", "quadratic"), ("3wrobot", "quad-nomix")])
def test_split_tick_with_frozen_envs_equals_the_unsplit_tick(name, cs, dtype):
    from rcognita_amd import _native as N

    Bb, K = 2100, 40  # halves [0, 1024) and [1024, 2100)
    t = Trio(name, dtype, batch=Bb, extra_bad=(1023, 1024), mode=O.MODE_RQL, critic_struct=O.CRITIC_IDS[cs], n_critic=4, buffer_size=6)
    one, two = t.h["bad"], t.h["pre"]
    two.set_field(N.FIELD_STATUS, one.get_field(N.FIELD_STATUS))
    one.set_tick_parts(1)
    two.set_tick_parts(2)
    cand = _cand(np.random.default_rng(77), t, K)
    for k in range(3):
        one.control_tick(cand, K=K)
        two.control_tick(cand, K=K)
        if k == 0:
            for e, split in ((one, False), (two, True)):
                for kind in (N.KERNEL_ACTOR, N.KERNEL_CRITIC):
                    assert e.last_launch(kind)["split"] == split, (kind, e.last_launch(kind))
                assert_kernel(e, "k_actor_dma")
        two.join()
    a, b = _snap(one, t.fields), _snap(two, t.fields)
    for f in t.fields:
        _same(b[f], a[f], f"split tick {f}")
    want = np.zeros(Bb, np.uint32)
    want[t.frozen] = 1
    np.testing.assert_array_equal(b["FIELD_STATUS"], want)
    assert (t.frozen < 1024).any() and (t.frozen >= 1024).any()
    _same(b["FIELD_STATE"][t.frozen], t.x_bad.astype(t.real)[t.frozen], "frozen STATE")
    t.close()
