#!/usr/bin/env python3
"""A system compiled at run time (rcg_register_system) next to a built-in one of the same kernel shape.

Registers the pendulum of INTEGRATION.md (DS 2, DU 1, NP 3; wall time of the call = probe + f32 + f64 core programs), creates
one handle per element type and times the first streamed decision (it compiles k_actor_dma at the handle's row length), then
times the streamed f64 tick at 65 536 envs x 256 candidates x Nactor 10 from the dispatches' own stamps (rcg_profile) on the
pendulum, on the small-angle pendulum (no trigonometry) and on Sys2Tank (same DS / DU, same kernel shape), as a fraction of
8 TB/s of candidate bytes.  The same for the pendulum with an output map y = (sin th, cos th, om) (DY = 3, out, out_jac_T;
DESIGN.md §13.1): its registration, its first streamed tick and its streamed f64 tick next to the pendulum without one.
RQL (policies with CRITIC): the first-use compile time of a critic program and of a DMA_RQL_* instance; the
streamed f64 RQL tick of a Sys2Tank copy interleaved with the built-in Sys2Tank (the same code shape: any gap beyond the
run-to-run spread is a finding); the same tick of the pendulum with the output map.
The device search (policies with SEARCH): the first-use compile time of the k_actor_search program and the time
of one rcg_control_tick_search round for the pendulum with and without the output map, f32 and f64, each next to the built-in
Sys2Tank at the same shape.
T ticks per launch (policies with TICKS): the first-use compile time of a k_ticks and of a k_ticks_mem program,
and the rate of rcg_control_ticks(T = 512) against 512 single ticks on the same handle at B = 1024, K = 64, Nactor = 10, f32 and
f64, interleaved, for the pendulum, the pendulum with the output map and a Sys2Tank copy next to the built-in Sys2Tank.
The disturbance model (policies with DD / disturb): the first-use compile time of the disturb program
(k_sim_dist, k_rhs_full) and, from the dispatches' own stamps, the disturbed env step (k_sim_dist) of the pendulum at 65 536
envs next to the undisturbed k_sim of a handle of the same shape, f32 and f64, interleaved.
The fused loop step (policies with LOOP): the first-use compile time of the loop program, and the simulation
steps per second of the B = 1 drop-in loop (tools/b1_profile.py's bracket) for the pendulum (MPC), the pendulum with the output
map (MPC, RQL) and a Sys2Tank copy next to the built-in Sys2Tank - fused, with Simulator.fuse = False and, when the root of
another checkout with a built library is given, on that checkout (the parent commit), interleaved, medians of five.
Derived adjoints (policies with AUTODIFF): the wall time of rcg_register_system for the pendulum and the corner
system C2 (tests/user_systems.py: DS 5, DU 2, NP 5, DY 1 with out) with hand-written jac_T / out_jac_T and with the members
derived; the k_actor_opt dispatch at B envs, Nactor, 5 iterations, 0 and 4 curvature pairs, f32 and f64, hand-written against
derived, interleaved, medians of five from the dispatches' own stamps; and the registers and scratch of the two instances, read
from an offline compile (hipcc -S, the library's options) of a unit that instantiates k_actor_opt for the policy as the runtime
adapter does - the one part that needs no GPU (`autodiff-resources`).
GPU box only; no torch.

    python tools/user_system_probe.py [B] [K] [Nactor] [search | ticks | disturb | autodiff]      (that section alone)
    python tools/user_system_probe.py 0 0 10 autodiff-resources
    python tools/user_system_probe.py 1 1 5 loop [root of another checkout]
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if len(sys.argv) > 5 and sys.argv[4] == "loop-worker":  # a worker of the loop section serves the checkout it is given
    ROOT = os.path.abspath(sys.argv[5])
sys.path.insert(0, ROOT)
from rcognita_amd import Engine, EngineConfig  # noqa: E402
from rcognita_amd import _native as N  # noqa: E402

# the pendulum of INTEGRATION.md §5: state (angle, rate), action (torque), pars (m, g, l)
PENDULUM = r"""
struct PendulumT {
  static constexpr int DS = 2, DU = 1, NP = 3;
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
  template <typename real, bool HW = false>
  __device__ __forceinline__ static void jac_T(const Pre<real>& q, const real* x, const real*, const real* lam, real* ax,
                                               real* bu) {
    real s, c;
    sincos_sel<real, HW>(x[0], &s, &c);
    ax[0] = -q.g_l * c * lam[1];
    ax[1] = lam[0];
    bu[0] = q.inv_ml2 * lam[1];
  }
};
"""
# the same shape without trigonometry (the small-angle pendulum, sin x ~ x): separates the cost of the f64 sine in the rollout
# from everything else the runtime path does
PENDULUM_LIN = PENDULUM.replace("sincos_sel<real, HW>(x[0], &s, &c);", "s = x[0];\n    c = (real)1;")
# with an output map: y = (sin th, cos th, om), the cost on (sin th, cos th) instead of th^2
PENDULUM_OUT = PENDULUM.replace("static constexpr int DS = 2, DU = 1, NP = 3;",
                                "static constexpr int DS = 2, DU = 1, NP = 3;\n  static constexpr int DY = 3;").replace("\n};\n", r'''
  template <typename real, bool HW = false>
  __device__ __forceinline__ static void out(const Pre<real>&, const real* x, real* y) {
    real s, c;
    sincos_sel<real, HW>(x[0], &s, &c);
    y[0] = s;
    y[1] = c;
    y[2] = x[1];
  }
  template <typename real, bool HW = false>
  __device__ __forceinline__ static void out_jac_T(const Pre<real>&, const real* x, const real* gy, real* gx) {
    real s, c;
    sincos_sel<real, HW>(x[0], &s, &c);
    gx[0] = c * gy[0] - s * gy[1];
    gx[1] = gy[2];
  }
};
''')
R1_OUT = np.diag([5.0, 5.0, 0.5, 0.1])

B = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
K = int(sys.argv[2]) if len(sys.argv) > 2 else 256
NH = int(sys.argv[3]) if len(sys.argv) > 3 else 10
PEAK = 8e12
ONLY = sys.argv[4] if len(sys.argv) > 4 else ""


# ---- the device search on policies with SEARCH ---------------------------------------------------------------
def with_search(src):
    i = src.index("static constexpr int DS")
    j = src.index("\n", i) + 1
    return src[:j] + "  static constexpr bool SEARCH = true;\n" + src[j:]


def search_rows():
    pend = N.register_system("PendulumSearchProbe", with_search(PENDULUM.replace("PendulumT", "PendulumSearchProbe")), 2, 1, 3)
    pout = N.register_system("PendulumOutSearchProbe", with_search(PENDULUM_OUT.replace("PendulumT", "PendulumOutSearchProbe")), 2, 1, 3)
    assert pend["has_search"] and pout["has_search"]
    rng = np.random.default_rng(1)
    pb = np.array([[-5.0, 5.0]])
    cases = (("pendulum (runtime)", pend["sys_id"], [1.3, 9.81, 0.7], np.diag([10.0, 1.0, 0.1]), None, pb, 0.01),
             ("pendulum with out (runtime)", pout["sys_id"], [1.3, 9.81, 0.7], R1_OUT, None, pb, 0.01),
             ("Sys2Tank (built-in)", N.SYS_2TANK, [18.4, 24.4, 1.3, 1.0, 0.2], np.diag([10.0, 10.0, 1.0]), [0.5, 0.5],
              np.array([[0.0, 1.0]]), 0.1))
    for dtype in ("f32", "f64"):
        engines = []
        for name, sid, pars, R1, tgt, bnds, dt in cases:
            e = Engine(EngineConfig(sys_id=sid, batch=B, dtype=dtype, Nactor=NH, pars=pars, ctrl_bnds=bnds, R1=R1,
                                    observation_target=tgt, dt_sim=dt, sampling_time=dt, pred_step_size=2 * dt))
            e.set_state(rng.uniform(0, 1, (B, 2)))
            t0 = time.perf_counter()
            e.control_tick_search(K=K, rounds=1, warm_start=True)
            e.synchronize()
            first = time.perf_counter() - t0
            n_prog = len([1 for _, x in N.system_programs(sid) if "k_actor_search" in x]) if sid >= N.SYS_USER_BASE else 0
            for _ in range(5):
                e.control_tick_search(K=K, rounds=1, warm_start=True)
            e.synchronize()
            e.profile([N.KERNEL_ACTOR])
            engines.append((name, e, first, n_prog))
        for _ in range(5):  # interleaved: ten ticks of each handle in turn
            for name, e, first, n_prog in engines:
                for _ in range(10):
                    e.control_tick_search(K=K, rounds=1, warm_start=True)
                e.synchronize()
        for name, e, first, n_prog in engines:
            t = e.profile_samples(N.KERNEL_ACTOR) * 1e-3
            ll = e.last_launch()
            blocks = np.median(t.reshape(5, -1), axis=1) * 1e6
            print(f"search {dtype} {name:28s} {ll['kernel']} variant {ll['variant']}: first tick "
                  f"{first:.2f} s ({'compiles the search program; ' + str(n_prog) + ' so far' if n_prog else 'nothing to compile'}), one round of "
                  f"{K} at {B} envs x Nactor {NH}: {np.median(t) * 1e6:.1f} us (medians of the five blocks {blocks.min():.1f} .. "
                  f"{blocks.max():.1f})")
            e.close()


# ---- T ticks per launch on policies with TICKS ----------------------------------------------------------------
def with_members(src, members):
    i = src.index("static constexpr int DS")
    j = src.index("\n", i) + 1
    return src[:j] + "".join(f"  static constexpr bool {m} = true;\n" for m in members) + src[j:]


def ticks_rows(Bt=1024, Kt=64, T=512):
    tank_src = open(os.path.join(ROOT, "rcognita_amd", "csrc", "rcg_systems.hpp")).read()
    i = tank_src.index("struct Sys2Tank {")
    tank_src = tank_src[i:tank_src.index("\n};\n", i) + 4].replace("struct Sys2Tank {", "struct TankTicksProbe {")
    pend = N.register_system("PendulumTicksProbe", with_members(PENDULUM.replace("PendulumT", "PendulumTicksProbe"), ["TICKS"]), 2, 1, 3)
    pout = N.register_system("PendulumOutTicksProbe",
                             with_members(PENDULUM_OUT.replace("PendulumT", "PendulumOutTicksProbe"), ["TICKS", "CRITIC"]), 2, 1, 3)
    tank = N.register_system("TankTicksProbe", with_members(tank_src, ["TICKS", "CRITIC"]), 2, 1, 5)
    assert pend["has_ticks"] and pout["has_ticks"] and tank["has_ticks"]
    rng = np.random.default_rng(2)
    pb, tb = np.array([[-5.0, 5.0]]), np.array([[0.0, 1.0]])
    tank_pars, tank_R1, tank_tgt = [18.4, 24.4, 1.3, 1.0, 0.2], np.diag([10.0, 10.0, 1.0]), [0.5, 0.5]
    cases = (("pendulum (runtime)", pend["sys_id"], [1.3, 9.81, 0.7], np.diag([10.0, 1.0, 0.1]), None, pb, 0.01),
             ("pendulum with out (runtime)", pout["sys_id"], [1.3, 9.81, 0.7], R1_OUT, None, pb, 0.01),
             ("Sys2Tank copy (runtime)", tank["sys_id"], tank_pars, tank_R1, tank_tgt, tb, 0.1),
             ("Sys2Tank (built-in)", N.SYS_2TANK, tank_pars, tank_R1, tank_tgt, tb, 0.1))
    # first use of a k_ticks_mem program: an RQL handle of the pendulum with out and of the Sys2Tank copy
    for name, sid, pars, R1, tgt, bnds, dt in cases[1:3]:
        e = Engine(EngineConfig(sys_id=sid, batch=Bt, dtype="f64", Nactor=NH, mode="RQL", critic_struct="quad-nomix", Ncritic=4,
                                buffer_size=10, gamma=0.95, pars=pars, ctrl_bnds=bnds, R1=R1, observation_target=tgt, dt_sim=dt,
                                sampling_time=dt, pred_step_size=2 * dt))
        e.set_state(rng.uniform(0, 1, (Bt, 2)))
        t0 = time.perf_counter()
        e.control_ticks(4, Kt)
        e.synchronize()
        ll = e.last_launch()
        print(f"ticks f64 RQL {name:28s} {ll['kernel']} variant {ll['variant']}: first rcg_control_ticks (compiles the k_ticks_mem "
              f"program) {time.perf_counter() - t0:.2f} s")
        e.close()
    for dtype in ("f32", "f64"):
        engines = []
        for name, sid, pars, R1, tgt, bnds, dt in cases:
            e = Engine(EngineConfig(sys_id=sid, batch=Bt, dtype=dtype, Nactor=NH, pars=pars, ctrl_bnds=bnds, R1=R1,
                                    observation_target=tgt, dt_sim=dt, sampling_time=dt, pred_step_size=2 * dt))
            e.set_state(rng.uniform(0, 1, (Bt, 2)))
            t0 = time.perf_counter()
            e.control_ticks(4, Kt)
            e.synchronize()
            first = time.perf_counter() - t0
            ll = e.last_launch()
            e.control_tick(None, K=Kt)  # (the single tick's kernels are part of the core programs)
            e.synchronize()
            engines.append((name, e, first, ll, {"one launch": [], "single ticks": []}))
        for _ in range(5):  # interleaved: both entry points on every handle in turn
            for name, e, first, ll, rates in engines:
                for tag in ("one launch", "single ticks"):
                    t0 = time.perf_counter()
                    if tag == "one launch":
                        e.control_ticks(T, Kt)
                    else:
                        for _ in range(T):
                            e.control_tick(None, K=Kt)
                    e.synchronize()
                    rates[tag].append(T * Bt / (time.perf_counter() - t0))
        for name, e, first, ll, rates in engines:
            a, b = np.median(rates["one launch"]), np.median(rates["single ticks"])
            print(f"ticks {dtype} {name:28s} {ll['kernel']} variant {ll['variant']}: first rcg_control_ticks {first:.2f} s "
                  f"({'compiles the k_ticks program' if name.endswith('(runtime)') else 'nothing to compile'}); T = {T} at {Bt} envs x K {Kt} x "
                  f"Nactor {NH}: one launch {a:.3e} env.control-steps/s ({min(rates['one launch']):.3e} .. {max(rates['one launch']):.3e}), "
                  f"{T} single ticks {b:.3e} ({min(rates['single ticks']):.3e} .. {max(rates['single ticks']):.3e}), ratio {a / b:.2f}")
            e.close()


# ---- the disturbance model on policies with DD / disturb ------------------------------------------------------
DISTURB_MEMBER = r'''
  template <typename real>
  __device__ __forceinline__ static void disturb(const Pre<real>& q, const real* x, const real*, const real* w, real* d) {
    d[1] = fma_r(q.inv_ml2 * cos(x[0]), w[0], d[1]);
  }
};
'''


def disturb_rows(Bd=65536, n_sub=1, reps=50):
    src = PENDULUM.replace("PendulumT", "PendulumDisturbProbe").replace(
        "static constexpr int DS = 2, DU = 1, NP = 3;", "static constexpr int DS = 2, DU = 1, NP = 3;\n  static constexpr int DD = 1;")
    pend = N.register_system("PendulumDisturbProbe", src.replace("\n};\n", DISTURB_MEMBER), 2, 1, 3)
    assert pend["dd"] == 1
    rng = np.random.default_rng(3)
    for dtype in ("f32", "f64"):
        engines = []
        for tag, dist in (("k_sim_dist (disturbed)", True), ("k_sim (undisturbed)", False)):
            kw = dict(is_disturb=True, pars_disturb=[[2.0], [0.5], [1.5]], seed=1) if dist else {}
            e = Engine(EngineConfig(sys_id=pend["sys_id"], batch=Bd, dtype=dtype, Nactor=NH, pars=[1.3, 9.81, 0.7],
                                    ctrl_bnds=np.array([[-5.0, 5.0]]), R1=np.diag([10.0, 1.0, 0.1]), dt_sim=0.01, sampling_time=0.01,
                                    pred_step_size=0.02, **kw))
            e.set_state(rng.uniform(-1, 1, (Bd, 2)))
            e.set_field(N.FIELD_ACTION, rng.uniform(-5, 5, (Bd, 1)))
            t0 = time.perf_counter()
            e.sim_step(n_sub)
            e.synchronize()
            first = time.perf_counter() - t0
            for _ in range(5):
                e.sim_step(n_sub)
            e.synchronize()
            e.profile([N.KERNEL_SIM])
            engines.append((tag, e, first))
        for _ in range(5):  # interleaved: ten env steps of each handle in turn
            for tag, e, first in engines:
                for _ in range(reps // 5):
                    e.sim_step(n_sub)
                e.synchronize()
        for tag, e, first in engines:
            t = e.profile_samples(N.KERNEL_SIM) * 1e-3
            blocks = np.median(t.reshape(5, -1), axis=1) * 1e6
            ll = e.last_launch(N.KERNEL_SIM)
            print(f"disturb {dtype} {tag:24s} {ll['kernel']}: first rcg_sim_step {first:.2f} s "
                  f"({'compiles the disturb program' if 'dist' in ll['kernel'] else 'nothing to compile'}); {n_sub} substep(s) at {Bd} envs: "
                  f"{np.median(t) * 1e6:.2f} us (medians of the five blocks {blocks.min():.2f} .. {blocks.max():.2f})")
            e.close()


# ---- the fused loop step on policies with LOOP ----------------------------------------------------------------
LOOP_CASES = (("pendulum", "MPC"), ("pendulum with out", "MPC"), ("pendulum with out", "RQL"), ("Sys2Tank copy", "MPC"),
              ("Sys2Tank (built-in)", "MPC"))


def loop_objects(name, mode):
    """System, controller and simulator of one case, wired as the presets wire them (simulation steps of dt / 2)."""
    from rcognita_amd import controllers, simulator, systems

    tank_src = open(os.path.join(ROOT, "rcognita_amd", "csrc", "rcg_systems.hpp")).read()
    i = tank_src.index("struct Sys2Tank {")
    tank_src = tank_src[i:tank_src.index("\n};\n", i) + 4].replace("struct Sys2Tank {", "struct TankLoopProbe {")

    class PendulumLoopProbe(systems.System):
        hip_policy = with_members(PENDULUM.replace("PendulumT", "PendulumLoopProbe"), ["LOOP"])

    class PendulumOutLoopProbe(systems.System):
        hip_policy = with_members(PENDULUM_OUT.replace("PendulumT", "PendulumOutLoopProbe"), ["LOOP", "CRITIC"])

    class TankLoopProbe(systems.System):
        hip_policy = with_members(tank_src, ["LOOP", "CRITIC"])

    pend = dict(pars=[1.3, 9.81, 0.7], bnds=np.array([[-5.0, 5.0]]), dt=0.05, x0=np.array([2.5, 0.0]), a0=[], tgt=[])
    tank = dict(pars=[18.4, 24.4, 1.3, 1.0, 0.2], bnds=np.array([[0.0, 1.0]]), dt=0.1, x0=np.array([2.0, -2.0]), a0=[0.5],
                tgt=np.array([0.5, 0.5]), dy=2, R1=np.diag([10.0, 10.0, 1.0]))
    c = {"pendulum": dict(pend, cls=PendulumLoopProbe, dy=2, R1=np.diag([10.0, 1.0, 0.1])),
         "pendulum with out": dict(pend, cls=PendulumOutLoopProbe, dy=3, R1=R1_OUT),
         "Sys2Tank copy": dict(tank, cls=TankLoopProbe), "Sys2Tank (built-in)": dict(tank, cls=systems.Sys2Tank)}[name]
    plant = c["cls"](sys_type="diff_eqn", dim_state=2, dim_input=1, dim_output=c["dy"], dim_disturb=1 if "Tank" in name else 0,
                     pars=c["pars"], ctrl_bnds=c["bnds"])
    dt = c["dt"]
    ctrl = controllers.CtrlOptPred(1, c["dy"], mode, ctrl_bnds=c["bnds"], action_init=c["a0"], t0=0, sampling_time=dt, Nactor=5,
                                   pred_step_size=2 * dt, sys_rhs=plant._state_dyn, sys_out=plant.out, state_sys=c["x0"],
                                   buffer_size=10, gamma=1, Ncritic=4, critic_period=dt, critic_struct="quad-nomix",
                                   stage_obj_struct="quadratic", stage_obj_pars=[c["R1"]], observation_target=c["tgt"], opt_iters=30)
    sim = simulator.Simulator(sys_type="diff_eqn", closed_loop_rhs=plant.closed_loop_rhs, sys_out=plant.out, state_init=c["x0"],
                              action_init=np.zeros(1), t0=0, t1=1e9, dt=dt / 2, max_step=dt / 2, first_step=1e-6, atol=1e-5,
                              rtol=1e-3, is_disturb=0, is_dyn_ctrl=0)
    return plant, ctrl, sim


def loop_rate(name, mode, fuse, steps):
    """tools/b1_profile.py's bracket: the calls of the reference's loop body in its order, `steps` simulation steps."""
    from rcognita_amd import controllers

    plant, ctrl, sim = loop_objects(name, mode)
    sim.fuse = fuse
    held = np.zeros(1)

    def body(n):
        for _ in range(n):
            sim.sim_step()
            t, _, obs, full = sim.get_sim_step_data()
            u = controllers.ctrl_selector(t, obs, held, None, ctrl, mode)
            plant.receive_action(u)
            ctrl.receive_sys_state(plant._state)
            ctrl.upd_accum_obj(obs, u)
            ctrl.stage_obj(obs, u)

    t0 = time.perf_counter()
    body(20)  # (first use: the loop program of this tree's fused run is compiled here)
    first = time.perf_counter() - t0
    t0 = time.perf_counter()
    body(steps)
    return steps / (time.perf_counter() - t0), ctrl.fused_steps, first


def loop_worker():
    """Serves `<case index> <fuse 0|1> <steps>` lines on stdin with `<rate> <fused steps> <seconds of the first 20 steps>`."""
    print("ready", flush=True)
    for line in sys.stdin:
        i, fuse, steps = (int(v) for v in line.split())
        rate, fused, first = loop_rate(*LOOP_CASES[i], bool(fuse), steps)
        print(f"{rate:.6e} {fused} {first:.3f}", flush=True)


def loop_rows(other_root=None, steps=2000, rounds=5):
    import subprocess

    def worker(root):
        w = subprocess.Popen([sys.executable, os.path.abspath(__file__), "1", "1", "5", "loop-worker", root], stdin=subprocess.PIPE,
                             stdout=subprocess.PIPE, text=True, cwd=root)
        assert w.stdout.readline().strip() == "ready"
        return w

    def ask(w, i, fuse, n):
        w.stdin.write(f"{i} {int(fuse)} {n}\n")
        w.stdin.flush()
        rate, fused, first = w.stdout.readline().split()
        return float(rate), int(fused), float(first)

    here = worker(ROOT)
    there = worker(os.path.abspath(other_root)) if other_root else None
    ways = [("fused", here, True), ("fuse = False", here, False)] + ([("other checkout", there, True)] if there else [])
    for i, (name, mode) in enumerate(LOOP_CASES):  # first use: registration, then the loop program with the first fused steps
        t0 = time.perf_counter()
        _, fused, first = ask(here, i, True, 20)
        total = time.perf_counter() - t0
        _, _, again = ask(here, i, True, 20)
        print(f"loop {name:22s} {mode}: first 20 fused steps {first:.2f} s (registration and handles before them {total - first:.2f} s), "
              f"the same again {again:.3f} s: first use of the loop program ~ {first - again:.2f} s; {fused} of 40 steps fused")
        for _, w, fuse in ways[1:]:
            ask(w, i, fuse, 20)
    rates = {(i, tag): [] for i in range(len(LOOP_CASES)) for tag, _, _ in ways}
    fused_n = {}
    for _ in range(rounds):  # interleaved: every way of every case in turn
        for i in range(len(LOOP_CASES)):
            for tag, w, fuse in ways:
                r, f, _ = ask(w, i, fuse, steps)
                rates[(i, tag)].append(r)
                fused_n[(i, tag)] = f
    for i, (name, mode) in enumerate(LOOP_CASES):
        parts = [f"{tag} {np.median(rates[(i, tag)]):.3e} ({min(rates[(i, tag)]):.3e} .. {max(rates[(i, tag)]):.3e}; "
                 f"{fused_n[(i, tag)]} of {steps + 20} steps fused)" for tag, _, _ in ways]
        print(f"loop {name:22s} {mode} B = 1, sim steps/s, median of {rounds} (min .. max): " + "; ".join(parts))
    for w in (here, there):
        if w:
            w.stdin.close()
            w.wait(timeout=60)


# ---- derived adjoints on policies with AUTODIFF ---------------------------------------------------------------
def autodiff_policies():
    """{case: (hand-written source, derived source, ds, du, np, pars, bnds, dy)}; the struct is named AdProbe<case><H|D>."""
    from tests.user_systems import CORNERS, make_policy
    from tests.user_systems_autodiff import autodiff_source

    out = {}
    hand = PENDULUM.replace("PendulumT", "AdProbePendH")
    out["pendulum"] = (hand, autodiff_source(hand, "AdProbePendD"), 2, 1, 3, [1.3, 9.81, 0.7], np.array([[-5.0, 5.0]]), 2)
    _, ds, du, np_, dy, dd = CORNERS["C2"]
    src, twin = make_policy("AdProbeC2H", ds, du, np_, dy, 0)
    out["C2"] = (src, autodiff_source(src, "AdProbeC2D"), ds, du, np_, twin.pars, twin.bnds, dy)
    return out


def autodiff_resources():
    """VGPRs and private-segment bytes of k_actor_opt<.., TGT false, GENERIC g, PAIRS p> (and the LOOP instance) for each policy,
    from `hipcc -S` of a unit shaped like the runtime compiler's: the kernel headers, the policy, an adapter struct that derives
    from it and - derived variant - takes jac_T / out_jac_T from rcg_dual.hpp."""
    import re
    import subprocess
    import tempfile

    csrc = os.path.join(ROOT, "rcognita_amd", "csrc")
    worst = 0
    for case, (hand, derived, ds, du, np_, pars, bnds, dy) in autodiff_policies().items():
        has_out = " static void out(" in hand
        for tag, src in (("hand-written", hand), ("derived", derived)):
            name = src[src.index("struct ") + 7:].split()[0]
            mix = ""
            if tag == "derived":
                mix = ("  template <typename real, bool HW = false>\n"
                       "  __device__ __forceinline__ static void jac_T(const typename P::template Pre<real>& q, const real* x, "
                       "const real* u, const real* lam, real* ax, real* bu) { ad_jac_T<P, real, HW>(q, x, u, lam, ax, bu); }\n")
                if has_out:
                    mix += ("  template <typename real, bool HW = false>\n"
                            "  __device__ __forceinline__ static void out_jac_T(const typename P::template Pre<real>& q, const real* x, "
                            f"const real* gy, real* gx) {{ ad_out_jac_T<P, real, HW, {dy}>(q, x, gy, gx); }}\n")
            inst = "".join(f"template __global__ void k_actor_opt<ProbeSys, {r}, false, {g}, {pr}{lp}>(const OptArgs<{r}>, const KParams<{r}>);\n"
                           for r in ("float", "double") for g, pr, lp in (("false", "false", ""), ("true", "true", ""),
                                                                          ("false", "false", ", true")))
            unit = ('#include "rcg_actor_dma_packed.hpp"\n#include "rcg_actor_opt.hpp"\n#include "rcg_dual.hpp"\nnamespace rcg {\n' + src +
                    f"struct ProbeSys : {name} {{\n  using P = {name};\n  static constexpr bool TGT = false;\n"
                    "  static constexpr unsigned ZW_PRESET = 0u, SHARED_U1 = 0u;\n"
                    f"  static constexpr bool HAS_OUT = {'true' if has_out else 'false'};\n  static constexpr int DY = {dy};\n" + mix +
                    "};\n" + inst + "}\n")
            with tempfile.TemporaryDirectory() as d:
                f = os.path.join(d, "unit.hip")
                open(f, "w").write(unit)
                subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=fast", "--offload-device-only",
                                       "-I" + csrc, "-I" + os.path.join(ROOT, "include"), "-S", f, "-o", os.path.join(d, "unit.s")])
                asm = open(os.path.join(d, "unit.s")).read()
            for meta in asm[asm.index("amdhsa.kernels:"):].split("\n  - ")[1:]:  # one entry per kernel, keys in alphabetical order
                kern = re.search(r"\.name:\s+(\S+)", meta)
                if kern is None or "k_actor_opt" not in kern.group(1):
                    continue
                kern = kern.group(1)
                get = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", meta).group(1))  # noqa: E731
                real = "f64" if "ProbeSysEd" in kern else "f32"
                flags = kern[kern.index("ProbeSysE") + 10:].split("EEv")[0]
                form = {"Lb0ELb0ELb0ELb0E": "MPC diagonal (no pairs)", "Lb0ELb1ELb1ELb0E": "generic with pairs",
                        "Lb0ELb0ELb0ELb1E": "LOOP (MPC diagonal)"}.get(flags, flags)
                scratch = get("private_segment_fixed_size")
                worst = max(worst, scratch if tag == "derived" else 0)
                print(f"autodiff resources {case:9s} {tag:12s} {real} k_actor_opt {form:24s}: {get('vgpr_count')} VGPRs, "
                      f"{get('sgpr_count')} SGPRs, private segment {scratch} B, LDS (static) {get('group_segment_fixed_size')} B")
    print("autodiff resources: offline compile (hipcc -S) of the adapter-shaped unit; derived instances' largest private segment: "
          f"{worst} B")


def autodiff_rows(iters=5, reps=5):
    rng = np.random.default_rng(5)
    for case, (hand, derived, ds, du, np_, pars, bnds, dy) in autodiff_policies().items():
        infos = {}
        for tag, src in (("hand-written", hand), ("derived", derived)):
            name = src[src.index("struct ") + 7:].split()[0]
            infos[tag] = N.register_system(name, src, ds, du, np_)
            print(f"autodiff {case:9s} {tag:12s}: rcg_register_system {infos[tag]['seconds']:.2f} s, autodiff mask {infos[tag]['autodiff']}")
        assert infos["hand-written"]["autodiff"] == 0 and infos["derived"]["autodiff"] == (3 if infos["derived"]["has_out"] else 1)
        x0 = rng.uniform(-2, 2, (B, ds))
        for dtype in ("f32", "f64"):
            for memory in (0, 4):
                engines = []
                for tag in ("hand-written", "derived"):
                    e = Engine(EngineConfig(sys_id=infos[tag]["sys_id"], batch=B, dtype=dtype, Nactor=NH, pars=pars, ctrl_bnds=bnds,
                                            R1=np.diag(np.linspace(10.0, 0.5, dy + du)), dt_sim=0.01, sampling_time=0.01, pred_step_size=0.02))
                    e.set_state(x0)
                    e.set_optimizer(memory)
                    e.actor_optimize(iters)  # (warm-up: loads the code object)
                    e.synchronize()
                    e.profile([N.KERNEL_ACTOR])
                    engines.append((tag, e))
                for _ in range(reps):  # interleaved
                    for tag, e in engines:
                        e.actor_optimize(iters)
                        e.synchronize()
                med = {}
                for tag, e in engines:
                    t = e.profile_samples(N.KERNEL_ACTOR)
                    med[tag] = float(np.median(t))
                    ll = e.last_launch(N.KERNEL_ACTOR)
                    print(f"autodiff {case:9s} {tag:12s} {dtype} memory {memory} {ll['kernel']}/{ll['variant']} at {B} envs, Nactor {NH}, "
                          f"{iters} iterations: median of {len(t)} {med[tag]:.3f} ms (min {t.min():.3f} .. max {t.max():.3f})")
                    e.close()
                print(f"autodiff {case:9s} {dtype} memory {memory}: derived / hand-written = {med['derived'] / med['hand-written']:.3f}")


if ONLY == "autodiff-resources":
    autodiff_resources()
    sys.exit(0)
if ONLY == "autodiff":
    autodiff_rows()
    autodiff_resources()
    sys.exit(0)
if ONLY == "loop-worker":
    loop_worker()
    sys.exit(0)
if ONLY == "loop":
    loop_rows(sys.argv[5] if len(sys.argv) > 5 else None)
    sys.exit(0)
if ONLY == "search":
    search_rows()
    sys.exit(0)
if ONLY == "disturb":
    disturb_rows()
    sys.exit(0)
if ONLY == "ticks":
    ticks_rows()
    sys.exit(0)

info = N.register_system("PendulumProbe", PENDULUM.replace("PendulumT", "PendulumProbe"), 2, 1, 3)
print(f"hiprtc {info['hiprtc']}: rcg_register_system {info['seconds']:.2f} s (probe + f32 + f64 core programs)")
lin = N.register_system("PendulumLinProbe", PENDULUM_LIN.replace("PendulumT", "PendulumLinProbe"), 2, 1, 3)
out = N.register_system("PendulumOutProbe", PENDULUM_OUT.replace("PendulumT", "PendulumOutProbe"), 2, 1, 3)
print(f"with out (DY {out['dy']}): rcg_register_system {out['seconds']:.2f} s (probe + f32 + f64 core programs, k_out)")


def engine(sid, dtype, pars, R1=None):
    return Engine(EngineConfig(sys_id=sid, batch=B, dtype=dtype, Nactor=NH, pars=pars, ctrl_bnds=np.array([[-5.0, 5.0]]),
                               R1=np.diag([10.0, 1.0, 0.1]) if R1 is None else R1, dt_sim=0.01, sampling_time=0.01,
                               pred_step_size=0.02))


rng = np.random.default_rng(0)
for label, sid, R1 in (("", info["sys_id"], None), ("with out, ", out["sys_id"], R1_OUT)):
    for dtype in ("f32", "f64"):
        e = engine(sid, dtype, [1.3, 9.81, 0.7], R1)
        e.set_state(rng.uniform(-1, 1, (B, 2)))
        cand = e.to_device(rng.uniform(-5, 5, (B, K, NH, 1)))
        t0 = time.perf_counter()
        e.control_tick(cand)
        e.synchronize()
        print(f"{label}{dtype}: first streamed tick (compiles {e.last_launch()['kernel']} at R = {NH}) "
              f"{time.perf_counter() - t0:.2f} s")
        e.close()

rows = []
for name, sid, pars, R1 in (("pendulum (runtime)", info["sys_id"], [1.3, 9.81, 0.7], None),
                            ("pendulum with out", out["sys_id"], [1.3, 9.81, 0.7], R1_OUT),
                            ("small-angle (runtime)", lin["sys_id"], [1.3, 9.81, 0.7], None),
                            ("Sys2Tank (built-in)", N.SYS_2TANK, [15.0, 15.0, 1.0, 1.0, 0.1], None)):
    e = engine(sid, "f64", pars, R1)
    e.set_state(rng.uniform(0, 1, (B, 2)))
    cand = e.to_device(rng.uniform(-5, 5, (B, K, NH, 1)))
    for _ in range(5):
        e.control_tick(cand)
    e.synchronize()
    e.profile([N.KERNEL_ACTOR])
    for _ in range(50):
        e.control_tick(cand)
    e.synchronize()
    t = np.median(e.profile_samples(N.KERNEL_ACTOR)) * 1e-3
    frac = B * K * NH * 8 / t / PEAK
    rows.append((name, e.last_launch(), t, frac))
    e.close()
for name, ll, t, frac in rows:
    print(f"{name:22s} {ll['kernel']} variant {ll['variant']} gpw {ll['envs_per_wave']}: decision {t * 1e6:.1f} us, "
          f"{frac:.3f} of 8 TB/s")


# ---- RQL on policies with CRITIC -----------------------------------------------------------------------------
def with_critic(src, extra=""):
    i = src.index("static constexpr int DS")
    j = src.index("\n", i) + 1
    return src[:j] + "  static constexpr bool CRITIC = true;\n" + extra + src[j:]


def tank_copy(name):
    src = open(os.path.join(ROOT, "rcognita_amd", "csrc", "rcg_systems.hpp")).read()
    i = src.index("struct Sys2Tank {")
    return with_critic(src[i:src.index("\n};\n", i) + 4].replace("struct Sys2Tank {", f"struct {name} {{"))


tank = N.register_system("TankCriticProbe", tank_copy("TankCriticProbe"), 2, 1, 5)
outc = N.register_system("PendulumOutCriticProbe", with_critic(PENDULUM_OUT.replace("PendulumT", "PendulumOutCriticProbe"),
                                                                "  static constexpr bool TGT = true;\n"), 2, 1, 3)
assert tank["has_critic"] and outc["has_critic"]
TANK_PARS, TANK_R1, TANK_TGT, TANK_BND = [18.4, 24.4, 1.3, 1.0, 0.2], np.diag([10.0, 10.0, 1.0]), [0.5, 0.5], np.array([[0.0, 1.0]])


def rql_engine(sid, pars, R1, target, bnds, dt):
    e = Engine(EngineConfig(sys_id=sid, batch=B, dtype="f64", Nactor=NH, mode="RQL", critic_struct="quad-nomix", Ncritic=4,
                            buffer_size=10, gamma=0.95, pars=pars, ctrl_bnds=bnds, R1=R1, observation_target=target, dt_sim=dt,
                            sampling_time=dt, pred_step_size=2 * dt))
    e.set_tick_parts(1)  # the built-in handle would split a tick of this size on a stream of its own: like for like
    return e


engines = []
for name, sid, pars, R1, tgt, bnds, lo, hi in (
        ("Sys2Tank copy (runtime)", tank["sys_id"], TANK_PARS, TANK_R1, TANK_TGT, TANK_BND, 0.0, 1.0),
        ("Sys2Tank (built-in)", N.SYS_2TANK, TANK_PARS, TANK_R1, TANK_TGT, TANK_BND, 0.0, 1.0),
        ("pendulum with out (runtime)", outc["sys_id"], [1.3, 9.81, 0.7], R1_OUT, [0.0, 1.0, 0.0], np.array([[-5.0, 5.0]]), -5.0, 5.0)):
    e = rql_engine(sid, pars, R1, tgt, bnds, 0.1 if len(pars) == 5 else 0.01)
    e.set_state(rng.uniform(0, 1, (B, 2)))
    cand = e.to_device(rng.uniform(lo, hi, (B, K, NH, 1)))
    t0 = time.perf_counter()
    e.critic_cost()
    e.synchronize()
    t1 = time.perf_counter()
    e.control_tick(cand)
    e.synchronize()
    t2 = time.perf_counter()
    ll = e.last_launch()
    print(f"{name}: first rcg_critic_cost (compiles the critic program: k_critic, k_critic_cost, k_critic_fit) {t1 - t0:.2f} s; "
          f"first RQL tick (compiles {ll['kernel']} variant {ll['variant']} at R = {NH}) {t2 - t1:.2f} s")
    for _ in range(5):
        e.control_tick(cand)
    e.synchronize()
    e.profile([N.KERNEL_ACTOR, N.KERNEL_CRITIC])
    engines.append((name, e, cand))
for _ in range(5):  # interleaved: ten ticks of each handle in turn
    for name, e, cand in engines:
        for _ in range(10):
            e.control_tick(cand)
        e.synchronize()
for name, e, cand in engines:
    ta, tc = e.profile_samples(N.KERNEL_ACTOR) * 1e-3, e.profile_samples(N.KERNEL_CRITIC) * 1e-3
    la, lc = e.last_launch(), e.last_launch(N.KERNEL_CRITIC)
    blocks = np.median(ta.reshape(5, -1), axis=1) * 1e6
    print(f"{name:28s} {la['kernel']} variant {la['variant']} gpw {la['envs_per_wave']}: decision {np.median(ta) * 1e6:.1f} us "
          f"({B * K * NH * 8 / np.median(ta) / PEAK:.3f} of 8 TB/s; medians of the five blocks {blocks.min():.1f} .. {blocks.max():.1f}), "
          f"{lc['kernel']} variant {lc['variant']}: env step + push + fit {np.median(tc) * 1e6:.1f} us")
    e.close()

search_rows()
ticks_rows()
disturb_rows()
