#!/usr/bin/env python3
"""Do two builds of librcg leave the same BITS behind the critic update?  (The companion of tools/ab_lib.py, which compares
their speed.)  One child process per library binds it with _native.use_library, runs the inputs below and writes a SHA-256 of
every field the critic update touches; the parent compares the two tables and prints one line per case.

    python tools/ab_bits.py --a <parent build>/librcg.so --b rcognita_amd/lib/librcg.so [--out DIR]

Inputs:
  walk     every case of tests.critic_fit_walk_inputs.GPU_CASES as tests/test_hip_critic_fit_walk.py launches it (70 envs, the
           four single-tick forms x six boxes x f32 / f64): the launch with the two NaN envs and the all-finite one
  loop     closed loop, B = 70, 12 control ticks (env step + push + fit): 2tank RQL quadratic and 3wrobot SQL quad-lin at
           Ncritic 4, 8 and 12 (buffer_size 20: k_critic_fit<3> / k_critic_fit_ml, k_critic_fit<8>, k_critic_fit_gen), f32 / f64
  ring     rcg_control_ticks with T = 7 on buffer_size 5 (k_ticks_mem's ring push and its un-rotation by 7 mod 5 rows), with one
           lane per env (2tank quadratic) and with four (2tank quad-lin), f32 / f64
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FIELDS = ("W_CRITIC", "W_PREV", "OBS_BUF", "ACT_BUF", "STATE", "STATE_PREV", "STATUS", "ACCUM")


def child(lib, out):
    from rcognita_amd import _native as N

    N.use_library(lib)
    from rcognita_amd import Engine
    from rcognita_amd.pool import preset_engine_config
    from tests.critic_fit_walk_inputs import B_WALK, GPU_CASES, NAN_ENVS, boxed_engine, walk_batch, walk_box
    from tests.helpers import load_buffers, rand_states

    table = {}

    def record(case, eng):
        kern = eng.last_launch(N.KERNEL_CRITIC)
        table[case] = {"kernel": f"{kern['kernel']}/{kern['variant']}"}
        for f in FIELDS:
            a = np.ascontiguousarray(eng.get_field(getattr(N, "FIELD_" + f)))
            table[case][f] = hashlib.sha256(a.tobytes()).hexdigest()[:16] + f":{a.dtype}{list(a.shape)}"

    for name, cs, m, box, dtype in GPU_CASES:
        cfg, ob, ab, wp, _ = walk_batch(name, cs, m, 7, dtype=dtype)
        eng = boxed_engine(name, B_WALK, dtype, cs, m, walk_box(box, cs, cfg.dc))
        ob_nan = ob.copy()
        ob_nan[NAN_ENVS[0], 1, 0] = np.nan
        ob_nan[NAN_ENVS[1], 0, -1] = np.nan
        for tag, o in (("nan", ob_nan), ("finite", ob)):
            load_buffers(eng, N, o, ab, wp)
            eng.critic_update(do_fit=True)
            record(f"walk {name} {cs} m={m} {box} {dtype} {tag}", eng)

    B = B_WALK
    for name, mode, cs in (("2tank", "RQL", "quadratic"), ("3wrobot", "SQL", "quad-lin")):
        for ncritic in (4, 8, 12):
            for dtype in ("f32", "f64"):
                eng = Engine(preset_engine_config(name, B, Nactor=6, mode=mode, critic_struct=cs, Ncritic=ncritic, buffer_size=20,
                                                  dtype=dtype))
                eng.set_state(rand_states(np.random.default_rng(5), name, B))
                for _ in range(12):
                    eng.control_tick(None, K=16)
                record(f"loop {name} {mode} {cs} Ncritic={ncritic} {dtype}", eng)

    for cs in ("quadratic", "quad-lin"):
        for dtype in ("f32", "f64"):
            eng = Engine(preset_engine_config("2tank", B, Nactor=6, mode="RQL", critic_struct=cs, Ncritic=4, buffer_size=5,
                                              dtype=dtype))
            eng.set_state(rand_states(np.random.default_rng(6), "2tank", B))
            eng.control_ticks(7, 9)
            kern = eng.last_launch(N.KERNEL_ACTOR)
            assert kern["kernel"] == "k_ticks" and kern["variant"] & 16, kern  # k_ticks_mem
            record(f"ring 2tank RQL {cs} T=7 buffer_size=5 {dtype}", eng)
            table[f"ring 2tank RQL {cs} T=7 buffer_size=5 {dtype}"]["kernel"] = f"{kern['kernel']}/{kern['variant']}"

    with open(out, "w") as f:
        json.dump(table, f, indent=1)
    print(f"{len(table)} cases -> {out}")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--a", required=True)
    p.add_argument("--b", default=os.path.join(ROOT, "rcognita_amd", "lib", "librcg.so"))
    p.add_argument("--out", default=os.path.join(ROOT, "build", "ab_bits"), help="directory of the two tables")
    p.add_argument("--timeout", type=int, default=420, help="seconds per child")
    p.add_argument("--child", nargs=2, default=None)
    a = p.parse_args()
    if a.child:
        return child(*a.child)
    os.makedirs(a.out, exist_ok=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("RCG_")}
    tables = {}
    for tag, lib in (("A", a.a), ("B", a.b)):  # one after the other; a child that fails ends the comparison
        out = os.path.join(a.out, f"ab_bits_{tag}.json")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--a", a.a, "--child", os.path.abspath(lib), out], env=env,
                           timeout=a.timeout, capture_output=True, text=True)
        print(f"{tag} {lib}: exit {r.returncode} {r.stdout.strip()[-200:]}", flush=True)
        if r.returncode != 0:
            print(r.stderr[-2000:])
            return 2
        with open(out) as f:
            tables[tag] = json.load(f)
    A, Bt = tables["A"], tables["B"]
    assert A.keys() == Bt.keys()
    bad = 0
    for case in A:
        diff = [f for f in FIELDS + ("kernel",) if A[case][f] != Bt[case][f]]
        bad += bool(diff)
        print(f"{'DIFFERS ' + ','.join(diff) if diff else 'equal'}  {case}  [{A[case]['kernel']}]")
    print(f"{len(A)} cases x {len(FIELDS)} fields: {len(A) - bad} cases byte-equal in every field, {bad} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
