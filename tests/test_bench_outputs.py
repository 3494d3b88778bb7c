"""bench.py --dump-outputs and the plain run: what the last timed step left a caller, written as .npy in the handle's
element width; the same arguments give the same arrays bit for bit; a plain run does the headline's work only (--full adds
the parity check, the secondary regimes, the CPU baselines and the cross-check)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


class _Handle:
    """Just enough of rcognita_amd.Engine for bench.write_outputs: sizes and the field layouts."""

    def __init__(self, B, real, critic=False):
        from rcognita_amd.engine import Engine

        self._FIELD_DIMS, self._FIELD_INT = Engine._FIELD_DIMS, Engine._FIELD_INT
        self._meta = Engine._field_meta
        self.B, self.real, self.ds, self.du, self.dc, self.N = B, real, 5, 2, 3, 10
        self.critic = critic

    def _field_meta(self, f):
        return self._meta(self, f)


def _device_copies(h, rng):
    """Host arrays in the caller's shapes and the bytes the device holds for them (the layout rcg_get_field copies)."""
    import torch

    import bench
    from rcognita_amd import _native as N

    host, bufs = {}, {}
    for name, attr in bench.OUTPUT_FIELDS:
        f = getattr(N, attr)
        if f == N.FIELD_W_CRITIC and not h.critic:
            continue
        shape, dt, h2d, _ = h._field_meta(f)
        n = (h.B,) if len(shape) == 1 else (h.B, shape[0])  # the caller's [B] / [B, d]; the device holds [d, B]
        a = (rng.integers(0, 256, n) if np.issubdtype(dt, np.integer) else rng.standard_normal(n)).astype(dt)
        host[name] = a
        dev = np.ascontiguousarray(h2d(a), dtype=dt)
        bufs[f] = torch.from_numpy(dev.view(np.uint8).reshape(-1).copy())
    return host, bufs


@pytest.mark.parametrize("real", [np.float32, np.float64])
def test_write_outputs_gives_the_callers_arrays(tmp_path, real):
    import bench

    h = _Handle(300, real, critic=True)
    host, bufs = _device_copies(h, np.random.default_rng(0))
    got = bench.write_outputs(str(tmp_path), [h], [bufs])
    assert set(got) == set(host) == {"state", "action", "best_J", "best_idx", "accum", "w_critic"}
    for name, a in host.items():
        z = np.load(tmp_path / f"{name}.npy")
        assert z.dtype in (np.float32, np.float64) and z.shape[0] == h.B and list(z.shape) == got[name]
        if name == "best_idx":
            assert z.dtype == np.float64 and np.array_equal(z, a.astype(np.float64))
        else:
            assert z.dtype == real and np.array_equal(z, a)


def test_write_outputs_samples_the_same_envs_of_every_array_under_the_limit(tmp_path, monkeypatch):
    import bench

    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 40_000)
    hs = [_Handle(1000, np.float64), _Handle(700, np.float32)]
    made = [_device_copies(h, np.random.default_rng(i)) for i, h in enumerate(hs)]
    runs = []
    for k in range(2):
        d = tmp_path / str(k)
        runs.append(bench.write_outputs(str(d), hs, [b for _, b in made]))
        total = sum(os.path.getsize(d / f"{n}.npy") - 128 for n in runs[-1])  # (.npy header: 128 bytes)
        assert total <= bench.DUMP_LIMIT_BYTES
    assert runs[0] == runs[1]
    for i, (h, (host, _)) in enumerate(zip(hs, made)):
        idx = np.load(tmp_path / "0" / f"handle{i}_env_index.npy")
        assert idx.dtype == np.float64 and 0 < idx.size < h.B and np.all(np.diff(idx) > 0)
        assert np.array_equal(idx, np.load(tmp_path / "1" / f"handle{i}_env_index.npy"))  # a fixed, seeded sample
        for name, a in host.items():
            z = np.load(tmp_path / "0" / f"handle{i}_{name}.npy")
            assert np.array_equal(z, a[idx.astype(np.int64)].astype(z.dtype))


def _plain(out_dir, extra=()):
    env = {k: v for k, v in os.environ.items() if not k.startswith("RCG_")}
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, BENCH, "--gpus", "1", "--steps", "7", "--warmup", "3", "--batch", "8192", "--candidates", "64",
           "--dump-outputs", str(out_dir)] + list(extra)
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_plain_runs_dump_the_same_outputs_and_do_the_headlines_work_only(tmp_path):
    a = _plain(tmp_path / "a")
    b = _plain(tmp_path / "b")
    for line in (a, b):
        for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert k in line, k
        assert line["steps"] == 7 and line["warmup"] == 3 and line["ms_per_step"] > 0 and line["dtype"] == "f64"
        for k in ("parity", "secondary", "cpu_baseline", "value_closed_loop"):
            assert k not in line, k
        assert line["timing"]["unbracketed_ms_per_step"] is None
        assert line["outputs"]["after_ticks"] == 32 + 3 + 7
    # the pre-spin runs for as long as the clock needs, and still the timed path is the same ticks from the same inputs
    assert a["outputs"]["arrays"] == b["outputs"]["arrays"]
    assert a["outputs"]["arrays"]["state"] == [8192, 5]
    for name in a["outputs"]["arrays"]:
        x, y = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert x.dtype in (np.float32, np.float64) and np.array_equal(x, y), name
    assert np.all(np.isfinite(np.load(tmp_path / "a" / "state.npy")))
