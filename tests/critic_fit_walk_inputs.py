"""Shared by tests/test_critic_fit_walk.py (CPU), tests/test_hip_critic_fit_walk.py (GPU) and
oracle/experiments/critic_fit_walk_profile.py: the ONE builder of the critic-fit walk's inputs (``walk_batch``, ``walk_box``), the
cases, and ``WalkReference`` - the oracle's fit with its traces and the exact minimisers of one (structure, rows, box, dtype).  What
the inputs are for, and why, is told in tests/test_critic_fit_walk.py."""
import dataclasses
import functools

import numpy as np

from oracle import rcg_oracle as O
from tests.helpers import engine_cfg, oracle_cfg, rand_actions, rand_states

REAL = {"f32": np.float32, "f64": np.float64}

# dim_critic on both sides of kFitLanesMinDc = 9 (rcg_sysops.hpp: one lane per env below, four lanes from there on at <= 3 rows)
STRUCTURES = (("2tank", "quadratic"), ("2tank", "quad-lin"), ("3wrobot", "quad-nomix"), ("3wrobot", "quad-lin"),
              ("3wrobotNI", "quad-mix"))
DC = {("2tank", "quadratic"): 6, ("2tank", "quad-lin"): 9, ("3wrobot", "quad-nomix"): 7, ("3wrobot", "quad-lin"): 35,
      ("3wrobotNI", "quad-mix"): 11}
# TD rows: one count per device form (<= 3: k_critic_fit<3> / k_critic_fit_ml, 4 .. 8: k_critic_fit<8>, beyond: k_critic_fit_gen),
# and the two ends of the legal range once each
CELLS = tuple((n, cs, m) for n, cs in STRUCTURES for m in (3, 8, 11)) + (("3wrobot", "quad-lin", 1), ("3wrobotNI", "quad-mix", 19))
STACK_FAMILIES = ("random", "wprev_1e3", "wprev_neg50", "rows_equal", "alt_rows_equal", "zero", "tiny", "mixed_scale")
BOX_FAMILIES = ("preset", "tight", "pinned_third", "pinned_all", "graded", "init_outside")
B_WALK = 70  # two waves, the second ragged; on the four-lane form five waves, the last with 6 of 16 quads

# (structure, rows) -> seed of the extra long-walk env (tests/test_critic_fit_walk.py); found by oracle/experiments/critic_fit_walk_profile.py
# as (seed, equal_from): equal_from = k > 0 makes buffer rows k, k + 1, ... equal to row k - 3 (with 6 weights and 8 or 11 rows no walk
# of 18 iterations turned up in 60 000 seeds unless the stack is rank deficient)
LONG_WALK_SEED = {
    ("2tank", "quadratic", 3): (12023, 0), ("2tank", "quadratic", 8): (14903, 3), ("2tank", "quadratic", 11): (5730, 4),
    ("2tank", "quad-lin", 3): (36, 0), ("2tank", "quad-lin", 8): (97, 0), ("2tank", "quad-lin", 11): (53, 0),
    ("3wrobot", "quad-nomix", 3): (124, 0), ("3wrobot", "quad-nomix", 8): (1315, 0), ("3wrobot", "quad-nomix", 11): (1817, 0),
    ("3wrobotNI", "quad-mix", 3): (1, 0), ("3wrobotNI", "quad-mix", 8): (3, 0), ("3wrobotNI", "quad-mix", 11): (1, 0),
    ("3wrobot", "quad-lin", 1): (0, 0), ("3wrobotNI", "quad-mix", 19): (22, 0),
}


def long_walk_need(dc):
    return min(20, 3 * dc)


def walk_cfg_kw(cs, m):
    """Keyword set (oracle naming, tests/helpers.py::both) of a handle that fits ``m`` TD rows of structure ``cs``."""
    return dict(mode=O.MODE_RQL, gamma=0.95, critic_struct=O.CRITIC_IDS[cs], n_critic=m + 1, buffer_size=m + 2)


def walk_box(family, cs, dc):
    """(w_init, w_min, w_max) ``[dc]`` of a box family."""
    lo, hi = O.critic_bounds(O.CRITIC_IDS[cs], dc)
    w0 = np.ones(dc)
    i = np.arange(dc)
    if family == "tight":
        lo, hi = np.full(dc, 0.9), np.full(dc, 1.1)
    elif family == "pinned_third":  # w_min = w_max for every third weight, at the start value
        lo, hi = np.where(i % 3 == 0, 1.0, lo), np.where(i % 3 == 0, 1.0, hi)
    elif family == "pinned_all":    # ... for every weight, away from the start value
        lo, hi = np.full(dc, 0.7), np.full(dc, 0.7)
    elif family == "graded":        # a different interval per weight, the start alternating between its two ends
        lo = np.linspace(-2.0, 0.5, dc)
        hi = lo + np.linspace(0.01, 3.0, dc)[::-1]
        w0 = np.where(i % 2 == 0, lo, hi)
    elif family == "init_outside":  # the start outside the preset box, on alternating sides
        w0 = np.where(i % 2 == 0, lo - 5.0, hi + 5.0)
    elif family != "preset":
        raise ValueError(family)
    return w0, lo, hi


NAN_ENVS = (34, 66)  # next to wprev_1e3 envs (33, 65) and near one-iteration envs, in the middle of wave 0 and in the ragged wave 1


def boxed_engine(name, B, dtype, cs, m, box, **kw):
    """Engine whose rcg_cfg carries ``box = (w_init, w_min, w_max)`` instead of the structure's preset."""
    from rcognita_amd import Engine, EngineConfig

    @dataclasses.dataclass
    class BoxedConfig(EngineConfig):
        w_box: tuple = None

        def to_native(self):
            c = super().to_native()
            for i, (w0, lo, hi) in enumerate(zip(*self.w_box)):
                c.w_init[i], c.w_min[i], c.w_max[i] = w0, lo, hi
            return c

    ec = engine_cfg(name, B, dtype, **dict(walk_cfg_kw(cs, m), **kw))
    return Engine(BoxedConfig(**{f.name: getattr(ec, f.name) for f in dataclasses.fields(ec)}, w_box=box))


def long_walk_env(name, cs, m, seed, equal_from=0):
    """One env of the W_PREV family with W_PREV on +-1e5: (obs_buf [bs, dy], act_buf [bs, du], w_prev [dc])."""
    cfg = oracle_cfg(name, **walk_cfg_kw(cs, m))
    rng = np.random.default_rng([seed, m, cfg.dc])
    ob = rand_states(rng, name, cfg.buffer_size)
    ab = rand_actions(rng, name, (cfg.buffer_size,))
    wp = rng.uniform(-1e5, 1e5, cfg.dc)
    if equal_from:
        ob[equal_from:], ab[equal_from:] = ob[equal_from - 3], ab[equal_from - 3]
    return ob, ab, wp


def walk_batch(name, cs, m, seed, B=B_WALK, dtype="f64"):
    """The batch of one (structure, rows): ``(cfg, obs_buf [B, bs, dy], act_buf [B, bs, du], w_prev [B, dc], family [B])``, the
    arrays rounded to ``dtype`` and returned as float64 (what the device holds and the oracle is given).  Env ``e`` belongs to
    stack family ``e % 8``, so neighbours in a wave - and in a group of 16 envs, one wave of the four-lane form - are of
    different families:

      random          the suite's family: rand_states / rand_actions, W_PREV uniform on [0.5, 1.5]
      wprev_1e3       W_PREV uniform on +-1e3                  wprev_neg50   W_PREV = -50 x the random one
      rows_equal      every buffer row equal to the first      alt_rows_equal  every other row equal to the first
      zero            all-zero buffers                         tiny          buffers x 1e-6
      mixed_scale     observation component 0 x 1e3, component 1 x 1e-3

    The last env of the wprev_1e3 family is replaced by ``long_walk_env`` where LONG_WALK_SEED has an entry."""
    rng = np.random.default_rng(seed)
    cfg = oracle_cfg(name, **walk_cfg_kw(cs, m))
    bs = cfg.buffer_size
    ob = np.stack([rand_states(rng, name, bs) for _ in range(B)])
    ab = rand_actions(rng, name, (B, bs))
    wp = rng.uniform(0.5, 1.5, (B, cfg.dc))
    big = rng.uniform(-1e3, 1e3, (B, cfg.dc))
    fam = np.arange(B) % len(STACK_FAMILIES)
    for e in range(B):
        f = STACK_FAMILIES[fam[e]]
        if f == "wprev_1e3":
            wp[e] = big[e]
        elif f == "wprev_neg50":
            wp[e] = -50.0 * wp[e]
        elif f == "rows_equal":
            ob[e], ab[e] = ob[e, :1], ab[e, :1]
        elif f == "alt_rows_equal":
            ob[e, ::2], ab[e, ::2] = ob[e, :1], ab[e, :1]
        elif f == "zero":
            ob[e], ab[e] = 0.0, 0.0
        elif f == "tiny":
            ob[e], ab[e] = 1e-6 * ob[e], 1e-6 * ab[e]
        elif f == "mixed_scale":
            ob[e, :, 0] *= 1e3
            ob[e, :, 1] *= 1e-3
    if (name, cs, m) in LONG_WALK_SEED:
        e = int(np.flatnonzero(fam == STACK_FAMILIES.index("wprev_1e3"))[-1])
        ob[e], ab[e], wp[e] = long_walk_env(name, cs, m, *LONG_WALK_SEED[(name, cs, m)])
    rb = lambda a: a.astype(REAL[dtype]).astype(np.float64)
    return cfg, rb(ob), rb(ab), rb(wp), fam


def exact_envs(B, dc):
    """The envs whose exact minimiser is computed: all of them, or - 35 weights, where one costs a tenth of a second - four
    groups of eight (one env per stack family each) spread over both waves."""
    if dc < 20:
        return np.arange(B)
    return np.array([e for e in range(B) if e // 8 in (0, 3, 6, 8)])


class WalkReference:
    """Everything the CPU and GPU files share about one (structure, rows, box, dtype): the batch, the oracle's fit with its
    traces, the exact minimisers and the oracle's gap to them."""

    def __init__(self, name, cs, m, box, dtype, seed):
        self.cfg, self.ob, self.ab, self.wp, self.fam = walk_batch(name, cs, m, seed, dtype=dtype)
        dc = self.cfg.dc
        self.w0, self.lo, self.hi = walk_box(box, cs, dc)
        self.A, self.b = O.critic_td_system(self.wp, self.ob, self.ab, self.cfg)
        self.traces = []
        self.w_or = O.critic_fit(self.cfg, self.wp, self.ob, self.ab, w_init=self.w0, lo=self.lo, hi=self.hi, trace=self.traces)
        self.iters = np.array([t["iters"] for t in self.traces])
        self.w_start = np.clip(self.w0, self.lo, self.hi)
        self.envs = exact_envs(len(self.fam), dc)
        self.exact = {}
        self.F0, self.Fstar, self.gap = {}, {}, {}
        for e in self.envs:
            t = self.traces[e]
            ex = O.critic_fit_exact(self.A[e], self.b[e], self.w0, self.lo, self.hi, guess=(t["free"], t["at_hi"]))
            self.exact[e] = ex
            self.F0[e], self.Fstar[e] = ex.objective(self.w_start), ex.objective(ex.w_mp)
            self.gap[e] = self.gap_of(e, self.w_or[e])

    def gap_of(self, e, w):
        """(F(w) - F(w*)) / F(clip(w_init)) of env ``e`` in extended precision, as a float (0 / 0 = 0)."""
        num = self.exact[e].objective(w) - self.Fstar[e]
        return 0.0 if num == 0 else float(num / self.F0[e]) if self.F0[e] > 0 else float("inf") * (1 if num > 0 else -1)

    def well_separated(self, e):
        """The minimiser of env ``e`` is well separated: the oracle's walk and the exact one end on the same active set, and
        the walk took no zero-length step."""
        t, ex = self.traces[e], self.exact[e]
        pinned = self.lo == self.hi
        same = np.array_equal(t["free"] & ~pinned, ex.free) and np.array_equal(t["at_hi"] & ~pinned & ~t["free"], ex.at_hi)
        return bool(same and t["zero_step"] == 0 and t["cap"] == 0 and t["safeguard"] == 0)


@functools.lru_cache(maxsize=None)  # (a session holds ~75 of them, a few MB each at most)
def walk_reference(name, cs, m, box, dtype="f64", seed=7):
    return WalkReference(name, cs, m, box, dtype, seed)


# The GPU file's cases, (structure, rows, box, dtype): every box in both dtypes on one (structure, rows) per device form - the
# cheap ones: an exact reference of 70 envs costs 0.3 s at 6-11 weights and 5 s at 35 -, and the other cells with one box each
_EVERY_BOX = (("2tank", "quadratic", 3), ("2tank", "quad-lin", 3), ("3wrobot", "quad-nomix", 8), ("3wrobotNI", "quad-mix", 11))
GPU_CASES = tuple(c + (box, dt) for c in _EVERY_BOX for box in BOX_FAMILIES for dt in ("f64", "f32")) + (
    ("3wrobot", "quad-lin", 3, "pinned_third", "f64"), ("3wrobot", "quad-lin", 3, "pinned_third", "f32"),
    ("3wrobot", "quad-lin", 8, "preset", "f64"), ("3wrobot", "quad-lin", 11, "tight", "f32"),
    ("3wrobot", "quad-lin", 1, "graded", "f64"), ("3wrobotNI", "quad-mix", 19, "pinned_third", "f64"),
    ("3wrobotNI", "quad-mix", 19, "init_outside", "f32"), ("3wrobot", "quad-nomix", 3, "tight", "f32"),
    ("3wrobotNI", "quad-mix", 3, "pinned_all", "f32"), ("2tank", "quadratic", 8, "graded", "f32"),
    ("2tank", "quad-lin", 8, "tight", "f32"), ("3wrobotNI", "quad-mix", 8, "pinned_all", "f32"),
    ("2tank", "quadratic", 11, "graded", "f32"), ("2tank", "quad-lin", 11, "tight", "f32"),
    ("3wrobot", "quad-nomix", 11, "pinned_all", "f32"))
# here: the same (structure, rows, box) with float64 inputs, the preset box on every (structure, rows), and the float32 rounding of
# the inputs - what a float32 handle's oracle is given - on the cheap ones
CASES = tuple(sorted({c[:4] + ("f64",) for c in GPU_CASES} | {c + ("preset", "f64") for c in CELLS}
                     | {c for c in GPU_CASES if c[4] == "f32" and DC[c[:2]] < 20}))

# worst gap of the float64 oracle to the exact minimiser per box family, measured on CASES and GPU_CASES at seed 7
# (profiles/critic_fit_walk.txt: rounding level - the walk ends ON the minimiser; pinned_all: w = w* exactly); the tests assert four
# times this - the factor covers seeds not drawn here
GAP_MEASURED = {"preset": 1.050e-14, "tight": 4.272e-16, "pinned_third": 1.795e-15, "pinned_all": 0.0, "graded": 1.125e-15,
                "init_outside": 1.461e-15}
GAP_FACTOR_ORACLE = 4.0
GAP_FACTOR_DEVICE = 8.0  # the device: the same algorithm at the same width, other fusions and summation order
# F(w) >= F(w*): both are evaluated in 50 digits from float64 data, so the difference is exact to ~1e-45 relative
F_EVAL_EPS = 1e-40

