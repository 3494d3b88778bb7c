"""T = 64 nominal ticks both ways - 64 calls of rcg_control_tick_nominal (k_sim then k_nominal each) against ONE launch of
k_ticks_nominal (rcg_control_ticks_nominal) - at B = 1024 and 65 536, for Sys3WRobotNI, Sys3WRobot and a pendulum registered at run
time with the member `nominal` and TICKS, in f32 and f64; and the first-use compile of that policy's two nominal programs.

    python3 tools/nominal_ticks_probe.py [--out profiles/nominal_ticks_probe.txt]

Wall time per call sequence, stream drained, median of seven after one warm-up.  Does not import torch (torch-ROCm bundles an
older hipRTC)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PENDULUM = r"""
struct PendulumProbe {
  static constexpr int DS = 2, DU = 1, NP = 3;
  static constexpr bool TICKS = true;
  static constexpr int NOMINAL_NP = 2;
  template <typename real>
  struct Pre {
    real g_l, inv_ml2;
  };
  template <typename real>
  __device__ __forceinline__ static Pre<real> prepare(const real* p) {
    return {p[1] / p[2], (real)1 / (p[0] * p[2] * p[2])};
  }
  template <typename real, bool HW = false>
  __device__ __forceinline__ static void rhs(const Pre<real>& q, const real* x, const real* u, real* d) {
    real s, c;
    sincos_sel<real, HW>(x[0], &s, &c);
    d[0] = x[1];
    d[1] = fma_r(q.inv_ml2, u[0], -q.g_l * s);
  }
  template <typename real>
  __device__ __forceinline__ static void nominal(const Pre<real>& q, const real* y, const real* c, real* u) {
    u[0] = (q.g_l * sin(y[0]) - c[1] * y[0] - c[0] * y[1]) / q.inv_ml2;
  }
};
"""
T = 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nominal_ticks_probe.txt"))
    args = ap.parse_args()
    from rcognita_amd import Engine, EngineConfig
    from rcognita_amd import _native as N

    lines = [f"nominal ticks: T = {T} single ticks (k_sim + k_nominal each) against one launch (k_ticks_nominal); wall time per {T} ticks,",
             "stream drained, median of 7 after one warm-up", ""]
    info = N.register_system("PendulumProbe", PENDULUM, 2, 1, 3)
    lines.append(f"registration of the pendulum (probe + two core programs): {info['seconds']:.2f} s, hipRTC {info['hiprtc']}")
    presets = {"3wrobotNI": dict(sys_id=N.SYS_3WROBOT_NI, pars=[], ctrl_bnds=np.array([[-25.0, 25], [-5, 5]]), gain=0.5, cp=(),
                                 x0=[5, 5, -3 * np.pi / 4]),
               "3wrobot": dict(sys_id=N.SYS_3WROBOT, pars=[10.0, 1.0], ctrl_bnds=np.array([[-300.0, 300], [-100, 100]]), gain=5.0,
                               cp=(10.0, 1.0), x0=[5, 5, -3 * np.pi / 4, 0, 0]),
               "pendulum (registered)": dict(sys_id=info["sys_id"], pars=[1.3, 9.81, 0.7], ctrl_bnds=np.array([[-5.0, 5.0]]), gain=2.0,
                                             cp=(4.0, 1.5), x0=[2.0, -1.0])}
    first = True
    for name, p in presets.items():
        for dtype in ("f32", "f64"):
            for B in (1024, 65536):
                n = len(p["x0"]) + p["ctrl_bnds"].shape[0]
                e = Engine(EngineConfig(sys_id=p["sys_id"], batch=B, dtype=dtype, pars=p["pars"], ctrl_bnds=p["ctrl_bnds"],
                                        R1=np.diag(np.linspace(10.0, 0.5, n)), dt_sim=0.01, sampling_time=0.01, pred_step_size=0.02))
                rng = np.random.default_rng(1)
                e.set_state(np.asarray(p["x0"]) + rng.uniform(-0.5, 0.5, (B, len(p["x0"]))))
                if name.startswith("pendulum") and B == 1024:  # the first use of an element type compiles the two programs
                    t0 = time.perf_counter()
                    e.control_tick_nominal(p["gain"], ctrl_pars=p["cp"])
                    e.synchronize()
                    t1 = time.perf_counter()
                    e.control_tick_nominal(p["gain"], ctrl_pars=p["cp"], T=2)
                    e.synchronize()
                    t2 = time.perf_counter()
                    lines.append(f"first use, {dtype}: k_nominal program {t1 - t0:.2f} s, k_ticks_nominal program {t2 - t1:.2f} s")
                    first = False

                def timed(fn):
                    fn()
                    e.synchronize()
                    ts = []
                    for _ in range(7):
                        t0 = time.perf_counter()
                        fn()
                        e.synchronize()
                        ts.append(time.perf_counter() - t0)
                    return float(np.median(ts)) * 1e6

                def loop():
                    for _ in range(T):
                        e.control_tick_nominal(p["gain"], ctrl_pars=p["cp"])

                t_loop = timed(loop)
                t_one = timed(lambda: e.control_tick_nominal(p["gain"], ctrl_pars=p["cp"], T=T))
                ll = e.last_launch()
                assert ll["kernel"] == "k_nominal" and ll["variant"] & 1, ll
                lines.append(f"{name:22s} {dtype} B = {B:6d}: single ticks {t_loop:9.0f} us, one launch {t_one:9.0f} us, "
                             f"ratio {t_loop / t_one:5.2f}")
                e.close()
    assert not first
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
