"""What the critic fit's active-set walk does on the inputs of tests/test_critic_fit_walk.py, and what no input reaches.

    python -m oracle.experiments.critic_fit_walk_profile [--seeds 3000] [--procs 4] > profiles/critic_fit_walk.txt
    python -m oracle.experiments.critic_fit_walk_profile --long-walk 2tank quadratic 8 [--equal-from 3]

Part 1 - the test's own cases (CASES and GPU_CASES, seed 7): per box family the branch counters of
``critic_fit_single(trace=...)`` summed over the envs, the longest walk, and the float64 oracle's worst gap to
``critic_fit_exact`` in the regularised objective, (F(w) - F(w*)) / F(clip(w_init)).  The worst gaps are the constants
``GAP_MEASURED`` of the test file.

Part 2 - random search for the branches the cases do not reach (pivot floor, iteration cap, safeguard on finite data): ``--seeds``
batches of 16 envs (two per stack family) from ``walk_batch``, seed s on (structure, rows) number s mod 17 in box family
(s div 17) mod 6, every counter summed.

``--long-walk``: the search that found ``LONG_WALK_SEED`` - the first seeds whose ``long_walk_env`` walks at least 20 iterations
(3 dc if smaller) in the preset box."""
import argparse
import collections
import multiprocessing
import sys

import numpy as np

from oracle import rcg_oracle as O
from tests import critic_fit_walk_inputs as W


def _search_one(s):
    name, cs, m = W.CELLS[s % len(W.CELLS)]
    box = W.BOX_FAMILIES[(s // len(W.CELLS)) % len(W.BOX_FAMILIES)]
    cfg, ob, ab, wp, fam = W.walk_batch(name, cs, m, seed=1000 + s, B=16)
    w0, lo, hi = W.walk_box(box, cs, cfg.dc)
    traces = []
    O.critic_fit(cfg, wp, ob, ab, w_init=w0, lo=lo, hi=hi, trace=traces)
    c = collections.Counter()
    for t in traces:
        for k in O.FIT_TRACE_KEYS:
            c[k] += t[k]
    c["fits"] = len(traces)
    c["cap_share_max"] = max(t["iters"] / O.fit_max_iters(cfg.dc) for t in traces)
    return c


def search(seeds, procs):
    total = collections.Counter()
    share = 0.0
    with multiprocessing.Pool(procs) as pool:
        for c in pool.imap_unordered(_search_one, range(seeds), chunksize=8):
            share = max(share, c.pop("cap_share_max"))
            total.update(c)
    return total, share


def cases_profile():
    per_box = {b: collections.Counter() for b in W.BOX_FAMILIES}
    gap = {b: (0.0, None) for b in W.BOX_FAMILIES}
    gmin = 0.0
    for case in sorted(set(W.CASES) | set(W.GPU_CASES)):
        name, cs, m, box, dtype = case
        ref = W.walk_reference(name, cs, m, box, dtype)
        for t in ref.traces:
            for k in O.FIT_TRACE_KEYS:
                per_box[box][k] += t[k]
        per_box[box]["fits"] += len(ref.traces)
        per_box[box]["iters_max"] = max(per_box[box]["iters_max"], int(ref.iters.max()))
        per_box[box]["exact"] += len(ref.exact)
        per_box[box]["well_separated"] += sum(ref.well_separated(e) for e in ref.exact)
        for e, g in ref.gap.items():
            gmin = min(gmin, g)
            if g > gap[box][0]:
                gap[box] = (g, case + (int(e), W.STACK_FAMILIES[ref.fam[e]], int(ref.iters[e])))
        W.walk_reference.cache_clear()
    return per_box, gap, gmin


def blocked_matters():
    """(fits of the cases that block a variable, those whose result changes when the release scan does not skip blocked variables)."""
    src = open(O.__file__).read()
    body = src[src.index("def critic_fit_single("):src.index("def critic_fit(cfg")]
    assert "if free[i] or blocked[i]:" in body
    ns = dict(O.__dict__)
    exec(body.replace("if free[i] or blocked[i]:", "if free[i]:").replace("def critic_fit_single(", "def no_skip("), ns)
    n = changed = 0
    for case in sorted({c[:4] for c in set(W.CASES) | set(W.GPU_CASES)}):
        ref = W.walk_reference(*case)
        for e, t in enumerate(ref.traces):
            if t["blocked"]:
                n += 1
                changed += not np.array_equal(ns["no_skip"](ref.A[e], ref.b[e], ref.w0, ref.lo, ref.hi), ref.w_or[e])
        W.walk_reference.cache_clear()
    return n, changed


def long_walk(name, cs, m, equal_from, limit=60000, want=3):
    cfg = W.oracle_cfg(name, **W.walk_cfg_kw(cs, m))
    w0, lo, hi = W.walk_box("preset", cs, cfg.dc)
    hits = []
    for seed in range(limit):
        ob, ab, wp = W.long_walk_env(name, cs, m, seed, equal_from)
        A, b = O.critic_td_system(wp[None], ob[None], ab[None], cfg)
        st = []
        O.critic_fit_single(A[0], b[0], w0, lo, hi, stats=st)
        if st[0] >= W.long_walk_need(cfg.dc):
            hits.append((seed, st[0]))
            print(f"{name} {cs} m={m} equal_from={equal_from}: seed {seed} walks {st[0]} iterations", flush=True)
            if len(hits) >= want:
                break
    return hits


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=3000)
    ap.add_argument("--procs", type=int, default=4)
    ap.add_argument("--long-walk", nargs=3, metavar=("SYSTEM", "STRUCTURE", "ROWS"))
    ap.add_argument("--equal-from", type=int, default=0)
    a = ap.parse_args()
    if a.long_walk:
        long_walk(a.long_walk[0], a.long_walk[1], int(a.long_walk[2]), a.equal_from)
        return
    keys = [k for k in O.FIT_TRACE_KEYS if k != "iters"]
    print("critic fit: what the active-set walk does (oracle/experiments/critic_fit_walk_profile.py)")
    print(f"\n1. the cases of tests/test_critic_fit_walk.py and tests/test_hip_critic_fit_walk.py, {W.B_WALK} envs each, seed 7")
    per_box, gap, gmin = cases_profile()
    for box in W.BOX_FAMILIES:
        c = per_box[box]
        print(f"\n  box family {box}: {c['fits']} fits, {c['iters']} iterations, longest walk {c['iters_max']}")
        print("    " + ", ".join(f"{k} {c[k]}" for k in keys))
        print(f"    exact minimisers {c['exact']}, of which well separated (same active set, no zero-length step) {c['well_separated']}")
        print(f"    worst gap of the float64 oracle to the exact minimiser: {gap[box][0]:.3e}  at {gap[box][1]}")
    print(f"\n  smallest gap (F(w) >= F(w*) must hold): {gmin:.3e}")
    print("\n  GAP_MEASURED = {" + ", ".join(f'"{b}": {gap[b][0]:.1e}' for b in W.BOX_FAMILIES) + "}")
    n, changed = blocked_matters()
    print(f"\n  the blocked mask: {n} fits (float64 inputs) block a variable, every one through a pinned weight; with the release scan's")
    print(f"  skip of blocked variables taken out, {changed} of them change their result - "
          + ("REDUNDANT on every input found" if changed == 0 else "it matters"))
    print(f"\n2. random search: {a.seeds} batches of 16 envs over the 17 (structure, rows) and the 6 box families")
    total, share = search(a.seeds, a.procs)
    print(f"  {total['fits']} fits, {total['iters']} iterations")
    print("  " + ", ".join(f"{k} {total[k]}" for k in keys))
    print(f"  longest walk as a share of its cap 3 dc + 10: {share:.2f}")
    for k, what in (("pivot_floor", "the pivot floor"), ("cap", "the iteration cap"), ("safeguard", "the safeguard on finite data")):
        print(f"  {what}: " + ("NOT REACHED - a defensive branch" if total[k] == 0 else f"reached {total[k]} times"))


if __name__ == "__main__":
    sys.exit(main())
