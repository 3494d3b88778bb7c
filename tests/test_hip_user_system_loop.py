"""rcg_loop_step on systems compiled at run time (rcg.h: the policy member LOOP) on the GPU.

1. Engine.loop_step against the separate calls on a twin handle, bit for bit: pendulum, the pendulum with y = (sin th, cos th, om)
   (DY = 3 > DS) in MPC / RQL / SQL and with a target, the corners C2 (DY = 1, per-env parameters) and C4 (DY = 5).
2. Copies of Sys3WRobot and Sys2Tank with LOOP + CRITIC against the built-ins: rows as bits, equal launch records.  Runs in a
   child process that does not import torch (test_hip_user_system.py says why).
3. The reference's loop on the mirror classes with Simulator.fuse on and off.
4. A frozen env.
5. Refusals, and the pinned-buffer boundary.
6. The size test of the built-ins (Sys3WRobot at B = 171).
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.test_user_system_critic_register import load_f15  # noqa: E402
from tests.test_user_system_loop_register import (BND, PEND_PARS, bad_state, clean_states, pendulum_loop_nojac_source,  # noqa: E402
                                                  pendulum_loop_source, pendulum_out_loop_source, with_loop)
from tests.test_user_system_register import PENDULUM  # noqa: E402
from tests.user_systems import CORNERS, make_policy  # noqa: E402

pytestmark = pytest.mark.gpu

DT = 0.01
FIELDS = ["FIELD_STATE", "FIELD_STATE_PREV", "FIELD_ACTION", "FIELD_ACCUM", "FIELD_STEP_IDX", "FIELD_STATUS", "FIELD_BEST_J",
          "FIELD_BEST_IDX", "FIELD_ACTION_SQN"]
_REG, _TWIN = {}, {}


def _corner(key):
    """The corner system `key` of tests/user_systems.py under another name, with LOOP: (source, NumPy twin)."""
    if key not in _TWIN:
        name, ds, du, np_, dy, dd = CORNERS[key]
        src, twin = make_policy(name + "L", ds, du, np_, dy, dd)
        _TWIN[key] = (with_loop(src), twin)
    return _TWIN[key]


def reg(key):
    """Each policy registered once per process: pend / out / nojac / plain (no LOOP) / C2 / C4."""
    from rcognita_amd import _native as N

    if key not in _REG:
        if key in CORNERS:
            src, S = _corner(key)
            _REG[key] = N.register_system(S.name, src, S.ds, S.du, S.np)
        else:
            name, src = {"pend": ("PendulumL", pendulum_loop_source("PendulumL")),
                         "out": ("PendulumYCL", pendulum_out_loop_source("PendulumYCL")),
                         "nojac": ("PendulumLNoJac", pendulum_loop_nojac_source("PendulumLNoJac")),
                         "plain": ("PendulumT", PENDULUM)}[key]
            _REG[key] = N.register_system(name, src, 2, 1, 3)
    return _REG[key]


def _engine(key, dtype, B, mode="MPC", cs="quad-nomix", **kw):
    from rcognita_amd import Engine, EngineConfig

    info = reg(key)
    if key in CORNERS:
        S = _corner(key)[1]
        pars, bnds, n = S.pars, S.bnds, S.dy + S.du
    else:
        pars, bnds, n = PEND_PARS, BND, info["dy"] + 1
    cfg = dict(sys_id=info["sys_id"], batch=B, dtype=dtype, Nactor=5, mode=mode, critic_struct=cs, Ncritic=4, buffer_size=6,
               pars=pars, ctrl_bnds=bnds, R1=np.diag(np.linspace(10.0, 0.5, n)), dt_sim=DT, sampling_time=DT,
               pred_step_size=2 * DT, gamma=1.0 if mode == "MPC" else 0.95)
    cfg.update(kw)
    return Engine(EngineConfig(**cfg))


def _states(key, B, seed=3):
    if key in CORNERS:
        return _corner(key)[1].rand_states(np.random.default_rng(seed), B)
    return clean_states(B, seed)


def _separate_calls(b, act, h, n_sub, decide, push, fit, iters):
    """One loop iteration by the separate entry points on the handle `b`: (state, action, stage, best_J or None, sequence or None,
    observation), in the handle's element type."""
    from rcognita_amd import _native as N

    b.set_field(N.FIELD_ACTION, act)
    b.sim_step(n_sub, step=h)
    if push:
        b.critic_update(do_fit=fit)
    xs = b.get_field(N.FIELD_STATE_PREV)
    st = b.get_state()
    y = b.out(st)
    if decide:
        a_b, u_b, bj, _ = b.actor_optimize(iters=iters, obs=y, state_sys=xs)
        b.set_field(N.FIELD_ACTION, a_b)
    else:
        a_b, u_b, bj = np.asarray(act).astype(b.real), None, None
    return st, a_b, b.stage_obj(y, a_b), bj, u_b, y


def _compare(a, b, act, h, mode, n_sub=1, nits=9, iters=6, plan=None, tag=""):
    """`nits` iterations of Engine.loop_step on `a` against the separate calls on `b` - plain step / push / decide / fit
    alternating as test_hip_loop_step.py alternates them - every number as bits."""
    from rcognita_amd import _native as N

    crit = mode != "MPC"
    has_out = a._loop_dims[2]
    for it in range(nits):
        decide, push, fit = plan(it) if plan else (it % 2 == 1, crit and it % 2 == 1, crit and it % 4 == 1)
        st, ac, stage, bj, w, y = a.loop_step(act, h, n_sub, decide=decide, push=push, fit=fit, iters=iters, with_obs=True)
        if decide:  # the plain MPC decision does the iteration's head and tail in its own launch (variant bit 3)
            ll = a.last_launch(N.KERNEL_ACTOR)
            assert ll["kernel"] == "k_actor_opt" and bool(ll["variant"] & 8) == (mode == "MPC"), (tag, ll)
        st_b, a_b, stage_b, bj_b, u_b, y_b = _separate_calls(b, act, h, n_sub, decide, push, fit, iters)
        what = f"{tag} it={it}"
        np.testing.assert_array_equal(st, st_b.astype(np.float64), err_msg="state " + what)
        np.testing.assert_array_equal(ac, np.asarray(a_b, dtype=np.float64), err_msg="action " + what)
        np.testing.assert_array_equal(stage, stage_b.astype(np.float64), err_msg="stage " + what)
        if decide:
            np.testing.assert_array_equal(bj, bj_b.astype(np.float64), err_msg="best_J " + what)
            np.testing.assert_array_equal(np.asarray(a.get_field(N.FIELD_ACTION_SQN)).reshape(u_b.shape), u_b, err_msg=what)
        else:
            assert np.all(np.isnan(bj)), what
        if crit:
            np.testing.assert_array_equal(w, b.get_field(N.FIELD_W_CRITIC).astype(np.float64), err_msg="w " + what)
            for f in (N.FIELD_OBS_BUF, N.FIELD_ACT_BUF, N.FIELD_W_PREV):
                np.testing.assert_array_equal(a.get_field(f), b.get_field(f), err_msg=what)
        else:
            assert w is None
        # the row's observation: Engine.out of the twin's state (without a map: the state)
        assert y.shape == (a.B, a.dy) and (has_out or np.array_equal(y, st, equal_nan=True))
        np.testing.assert_array_equal(y, y_b.astype(np.float64), err_msg="observation " + what)
        for f in ("FIELD_STATE", "FIELD_STATE_PREV", "FIELD_ACTION", "FIELD_STATUS"):
            np.testing.assert_array_equal(a.get_field(getattr(N, f)), b.get_field(getattr(N, f)), err_msg=f + " " + what)
        act = np.asarray(ac, dtype=np.float64).copy()  # the loop hands the decision back: System.receive_action
    return act


def _pair(key, dtype, B, mode="MPC", cs="quad-nomix", **kw):
    a, b = _engine(key, dtype, B, mode, cs, **kw), _engine(key, dtype, B, mode, cs, **kw)
    x0 = _states(key, B)
    a.set_state(x0)
    b.set_state(x0)
    return a, b


F15_TARGET = object()
CASES = [("pend", "MPC", "quad-nomix", 1, {}), ("pend", "MPC", "quad-nomix", 7, {}), ("out", "MPC", "quad-nomix", 3, {}),
         ("out", "RQL", "quadratic", 2, {}), ("out", "SQL", "quad-mix", 3, {}),
         ("out", "RQL", "quad-nomix", 2, dict(observation_target=F15_TARGET)),
         ("C2", "MPC", "quad-nomix", 5, dict(per_env_pars=True)), ("C4", "MPC", "quad-nomix", 2, {})]


# ---- 1. loop_step equals the separate calls ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("key,mode,cs,B,kw", CASES, ids=[f"{c[0]}-{c[1]}-{c[2]}-B{c[3]}{'-x' if c[4] else ''}" for c in CASES])
def test_loop_step_equals_the_separate_calls(key, mode, cs, B, kw, dtype):
    from rcognita_amd import _native as N

    kw = dict(kw)
    if kw.get("observation_target") is F15_TARGET:
        kw["observation_target"] = np.array(load_f15()[0]["target"])
    a, b = _pair(key, dtype, B, mode, cs, **kw)
    if kw.get("per_env_pars"):  # per-env parameters through the policy's prepare(): within 20 % of nominal
        S = _corner(key)[1]
        pars = np.array(S.pars) * np.random.default_rng(5).uniform(0.8, 1.2, (B, S.np))
        for e in (a, b):
            e.set_field(N.FIELD_PARS, pars)
    bnds = np.asarray(a.cfg.ctrl_bnds, dtype=float)
    _compare(a, b, np.tile(bnds[:, 0] / 10.0, (B, 1)), DT / 2, mode, tag=f"{key} {mode} {dtype}")
    if a._loop_dims[2]:  # an output map: the row is dy doubles longer, and the program is listed
        assert a._loop_dims[0] == a._loop_dims[1] + a.dy
    progs = [(p, e) for p, e in N.system_programs(reg(key)["sys_id"]) if p.endswith("_loop.hip")]
    real = "double" if dtype == "f64" else "float"
    assert any(e == f"rcg::k_loop<rcg::RcgRtcSys, {real}>" for _, e in progs), progs
    assert any(e.startswith(f"rcg::k_actor_opt<rcg::RcgRtcSys, {real}, ") and e.endswith("false, false, true>") for _, e in progs)
    opt = [e for _, e in progs if "k_actor_opt" in e]  # one program per (element type, target setting), compiled once
    assert len(opt) == len(set(opt))


def test_loop_step_with_two_substeps():
    """Engine level: n_substeps = 2 - the decision rolls out from STATE_PREV, the state before the LAST substep, on both sides."""
    a, b = _pair("out", "f64", 3)
    _compare(a, b, np.tile(BND[:, 0] / 10.0, (3, 1)), DT, "MPC", n_sub=2, nits=5, tag="two substeps")


# ---- 2. copies of the built-ins -------------------------------------------------------------------------------------------------
def _copy_source(struct, name):
    from tests.test_hip_user_system_critic import _copy_source as with_critic_copy

    return with_loop(with_critic_copy(struct, name))


def _copies_compare():
    """The child: built-in Sys3WRobot / Sys2Tank against their renamed copies with LOOP + CRITIC; raises on the first difference."""
    from oracle import rcg_oracle as O
    from rcognita_amd import Engine
    from rcognita_amd import _native as N
    from tests.helpers import engine_cfg, rand_states

    copies = {"3wrobot": N.register_system("UserRobotL", _copy_source("Sys3WRobot", "UserRobotL"), 5, 2, 2),
              "2tank": N.register_system("UserTankL", _copy_source("Sys2Tank", "UserTankL"), 2, 1, 5)}
    assert all(i["has_loop"] and i["has_critic"] and not i["has_out"] for i in copies.values())
    checked = 0
    for name in ("3wrobot", "2tank"):
        for mode, cs, B in (("MPC", "quad-nomix", 1), ("MPC", "quad-nomix", 7), ("RQL", "quadratic", 3)):
            for dtype in ("f32", "f64"):
                tag = (name, mode, B, dtype)

                def make(sid):
                    c = engine_cfg(name, B, dtype, n_actor=5, mode=O.MODE_IDS[mode], critic_struct=O.CRITIC_IDS[cs], n_critic=4,
                                   buffer_size=6)
                    c.sys_id = sid
                    return Engine(c)

                a, b = make(N.SYS_IDS[name]), make(copies[name]["sys_id"])
                x0 = rand_states(np.random.default_rng(3), name, B)
                for e in (a, b):
                    e.set_state(x0)
                act = np.tile(np.asarray(a.cfg.ctrl_bnds, dtype=float)[:, 0] / 10.0, (B, 1))
                crit = mode != "MPC"
                for it in range(9):
                    k = dict(decide=it % 2 == 1, push=crit and it % 2 == 1, fit=crit and it % 4 == 1, iters=6)
                    ra, rb = a.loop_step(act, a.cfg.dt_sim / 2, 1, **k), b.loop_step(act, a.cfg.dt_sim / 2, 1, **k)
                    for u, v in zip(ra, rb):
                        assert (u is None and v is None) or u.tobytes() == v.tobytes(), (tag, it)
                    for kind in (N.KERNEL_ACTOR, N.KERNEL_SIM, N.KERNEL_CRITIC):
                        assert a.last_launch(kind) == b.last_launch(kind), (tag, it, kind, a.last_launch(kind), b.last_launch(kind))
                    for f in FIELDS + (["FIELD_W_CRITIC", "FIELD_W_PREV", "FIELD_OBS_BUF", "FIELD_ACT_BUF"] if crit else []):
                        assert a.get_field(getattr(N, f)).tobytes() == b.get_field(getattr(N, f)).tobytes(), (tag, it, f)
                    act = np.array(ra[1])
                    checked += 1
                if not crit:
                    assert a.last_launch(N.KERNEL_ACTOR)["variant"] & 8
                a.close()
                b.close()
    print("copies bit-identical:", checked, "loop steps")


def test_copies_with_loop_are_bit_identical_to_the_builtins():
    env = {k: v for k, v in os.environ.items() if k != "PYTHONPATH"}
    code = "import sys; sys.path.insert(0, %r); import tests.test_hip_user_system_loop as t; t._copies_compare(); " \
           "assert 'torch' not in sys.modules" % ROOT
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "bit-identical" in r.stdout


# ---- 3. the reference's loop on the mirror classes -----------------------------------------------------------------------------
def _classes():
    from rcognita_amd.systems import System

    if "cls" not in _REG:
        class PendulumL(System):
            hip_policy = pendulum_loop_source("PendulumL")

        class PendulumYCL(System):
            hip_policy = pendulum_out_loop_source("PendulumYCL")

        class PendulumLNoJac(System):
            hip_policy = pendulum_loop_nojac_source("PendulumLNoJac")

        _REG["cls"] = {"pend": PendulumL, "out": PendulumYCL, "nojac": PendulumLNoJac}
    return _REG["cls"]


def _objects(key, mode, cs, B=None, n_substeps=1, dtype="f64", **ctrl_kw):
    """System, controller and simulator wired as the reference's presets wire them: simulation steps of dt / 2."""
    from rcognita_amd import controllers, simulator

    cls = _classes()[key]
    dy = 3 if key == "out" else 2
    my_sys = cls(sys_type="diff_eqn", dim_state=2, dim_input=1, dim_output=dy, dim_disturb=0, pars=PEND_PARS, ctrl_bnds=BND,
                 dtype=dtype)
    x0 = np.array([2.5, 0.0])
    if B is not None:
        x0 = x0 + np.random.default_rng(9).uniform(-0.5, 0.5, (B, 2))
    dt = 0.05
    ctrl_kw.setdefault("opt_iters", 8)
    my_ctrl = controllers.CtrlOptPred(1, dy, mode, ctrl_bnds=BND, t0=0, sampling_time=dt, Nactor=5, pred_step_size=dt,
                                      sys_rhs=my_sys._state_dyn, sys_out=my_sys.out, state_sys=x0, buffer_size=10, gamma=1,
                                      Ncritic=4, critic_period=dt, critic_struct=cs, stage_obj_struct="quadratic",
                                      stage_obj_pars=[np.diag(np.linspace(10.0, 0.5, dy + 1))], dtype=dtype, **ctrl_kw)
    my_sim = simulator.Simulator(sys_type="diff_eqn", closed_loop_rhs=my_sys.closed_loop_rhs, sys_out=my_sys.out, state_init=x0,
                                 action_init=np.zeros(1), t0=0, t1=100, dt=dt / 2, max_step=dt / 2, first_step=1e-6, atol=1e-5,
                                 rtol=1e-3, is_disturb=0, is_dyn_ctrl=0, n_substeps=n_substeps, dtype=dtype)
    return my_sys, my_ctrl, my_sim


def _run(key, mode, cs, fuse, T, B=None, speculate=True, meddle=None, **kw):
    from rcognita_amd import controllers

    my_sys, my_ctrl, my_sim = _objects(key, mode, cs, B=B, **kw)
    my_sim.fuse = fuse
    my_ctrl.speculate = speculate
    rows = []
    for k in range(T):  # presets/main_3wrobot.py:419-446
        if meddle is not None:
            meddle(k, my_sys, my_ctrl, my_sim, rows)
        my_sim.sim_step()
        t, state, observation, state_full = my_sim.get_sim_step_data()
        action = controllers.ctrl_selector(t, observation, np.zeros(1), None, my_ctrl, mode)
        my_sys.receive_action(action)
        my_ctrl.receive_sys_state(my_sys._state)
        my_ctrl.upd_accum_obj(observation, action)
        rows.append(np.concatenate([[t], np.ravel(state_full), np.ravel(observation), np.ravel(action),
                                    np.ravel(my_ctrl.stage_obj(observation, action)), np.ravel(my_ctrl.accum_obj_val),
                                    np.ravel(np.broadcast_to(my_ctrl.w_critic, (my_ctrl.B, my_ctrl.dim_critic)))]))
    return np.stack(rows), my_ctrl


@pytest.mark.parametrize("key,mode,cs,B", [("pend", "MPC", "quad-nomix", None), ("pend", "MPC", "quad-nomix", 4),
                                           ("out", "MPC", "quad-nomix", None), ("out", "RQL", "quadratic", None)])
def test_drop_in_loop_is_the_same_with_and_without_the_fused_step(key, mode, cs, B):
    """test_hip_loop_step.py's yardstick on compiled systems: every row [t, state, observation, action, stage_obj, accum_obj,
    w_critic] identical, the fused run really served its iterations by one call, speculation changes no number."""
    T = 30
    fused, c1 = _run(key, mode, cs, True, T, B=B)
    plain, c0 = _run(key, mode, cs, False, T, B=B)
    nospec, c2 = _run(key, mode, cs, True, T, B=B, speculate=False)
    np.testing.assert_array_equal(fused, plain)
    np.testing.assert_array_equal(nospec, plain)
    assert c0.fused_steps == 0 and c0.fused_decisions == 0
    assert c1.fused_steps >= T - 2 and c1.fused_decisions >= T // 2 - 1, (c1.fused_steps, c1.fused_decisions)
    assert c2.fused_steps == c1.fused_steps and c2.fused_decisions == c1.fused_decisions and c2.spec_hits == 0
    assert c1.spec_hits >= T - 3, (c1.spec_hits, c1.spec_drops)
    np.testing.assert_array_equal(np.asarray(c1._prev_opt).reshape(np.asarray(c0._prev_opt).shape), c0._prev_opt)
    np.testing.assert_array_equal(c1.observation_buffer, c0.observation_buffer)
    np.testing.assert_array_equal(c1.action_buffer, c0.action_buffer)
    assert np.ptp(fused[:, 1]) > 1e-3  # the pendulum moved


def _set_state(sim, f):
    sim.state_full = np.asarray(sim.state_full, dtype=float) * f
    sim.state = sim.state_full[..., 0:sim.dim_state]
    sim.observation = sim.sys_out(sim.state)


MEDDLERS = {
    "another-action": lambda k, s, c, m, rows: s.receive_action(np.asarray(s.action, dtype=float) * 0.5) if k in (5, 6, 12) else None,
    "reset": lambda k, s, c, m, rows: (m.reset(), c.reset(0)) if k == 10 else None,
    "set-state": lambda k, s, c, m, rows: _set_state(m, 1.001) if k in (7, 13) else None,
}


@pytest.mark.parametrize("what", sorted(MEDDLERS))
def test_a_step_started_ahead_that_is_not_asked_for_is_dropped(what):
    """Three of test_hip_loop_step.py's meddlers on the pendulum with an output map: the step started ahead is dropped, every row
    equals the run without it."""
    T = 18
    ahead, c2 = _run("out", "MPC", "quad-nomix", True, T, meddle=MEDDLERS[what])
    plain, c0 = _run("out", "MPC", "quad-nomix", False, T, meddle=MEDDLERS[what])
    np.testing.assert_array_equal(ahead, plain)
    assert c2.spec_drops >= 1 and c2.spec_hits >= T // 2, (what, c2.spec_hits, c2.spec_drops)


def test_two_substeps_per_step_run_by_the_separate_calls():
    """Simulator(n_substeps=2) on a compiled system: the device would roll a fused decision out from the state before the last
    substep, compute_action accepts one against the state before the whole step - not fused, and the same rows."""
    T = 10
    a, c1 = _run("out", "MPC", "quad-nomix", True, T, n_substeps=2)
    b, c0 = _run("out", "MPC", "quad-nomix", False, T, n_substeps=2)
    assert c1.fused_steps == 0 and c0.fused_steps == 0
    np.testing.assert_array_equal(a, b)


# ---- 4. a frozen env ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_a_frozen_env_is_not_stepped_and_is_decided_for(dtype):
    from rcognita_amd import _native as N

    B, bad_at = 5, 2
    a, b = _pair("out", dtype, B)
    x0 = clean_states(B)
    x0[bad_at] = bad_state(dtype)
    for e in (a, b):
        e.set_state(x0)
    _compare(a, b, np.tile(BND[:, 0] / 10.0, (B, 1)), DT / 2, "MPC", nits=4, plan=lambda it: (it == 2, False, False), tag="frozen")
    for e in (a, b):
        status = e.get_field(N.FIELD_STATUS)
        assert status[bad_at] & 1 and not np.any(np.delete(status, bad_at) & 1)
        np.testing.assert_array_equal(e.get_state()[bad_at], x0[bad_at].astype(e.real))  # not stepped
    others = np.delete(np.arange(B), bad_at)
    assert np.all(a.get_state()[others] != x0[others].astype(a.real))
    sqn = a.get_field(N.FIELD_ACTION_SQN).reshape(B, -1)
    assert np.all(np.isfinite(sqn)) and np.all(np.abs(sqn) <= 5.0)  # decided for: a finite sequence inside the box


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------
def _snapshot(e):
    from rcognita_amd import _native as N

    return {f: e.get_field(getattr(N, f)).copy() for f in FIELDS}, N.lib().rcg_tick_count(e._h)


def test_a_policy_without_loop_is_refused_and_nothing_moves():
    from rcognita_amd import _native as N

    L, B = N.lib(), 4
    e = _engine("plain", "f64", B)
    e.set_state(clean_states(B))
    e.actor_optimize(iters=3)
    snap, ticks = _snapshot(e)
    out, act = (C.c_double * (B * 16))(), (C.c_double * B)()
    for flags in (0, N.LOOP_DECIDE):
        assert L.rcg_loop_step_begin(e._h, C.cast(act, C.c_void_p), DT, 1, flags, 5) == N.ERR_UNSUPPORTED
        assert "LOOP" in N.last_error(e._h) and "PendulumT" in N.last_error(e._h)
        assert L.rcg_loop_step_end(e._h, C.cast(out, C.c_void_p)) == N.ERR_BAD_ARG  # nothing is pending
        assert L.rcg_loop_step(e._h, C.cast(act, C.c_void_p), DT, 1, flags, 5, C.cast(out, C.c_void_p)) == N.ERR_UNSUPPORTED
        assert "LOOP" in N.last_error(e._h)
    now, ticks_now = _snapshot(e)
    assert ticks_now == ticks
    for f in FIELDS:
        np.testing.assert_array_equal(now[f], snap[f], err_msg=f)
    assert not any(p.endswith("_loop.hip") for p, _ in N.system_programs(reg("plain")["sys_id"]))


def test_loop_without_jac_serves_steps_and_refuses_decisions():
    from rcognita_amd import _native as N

    B = 3
    a, b = _engine("nojac", "f64", B), _engine("nojac", "f64", B)
    x0 = clean_states(B)
    for e in (a, b):
        e.set_state(x0)
    act = np.tile(BND[:, 0] / 10.0, (B, 1))
    for it in range(3):  # plain steps are served and equal the separate calls
        st, ac, stage, bj, w = a.loop_step(act, DT / 2)
        st_b, a_b, stage_b, _, _, _ = _separate_calls(b, act, DT / 2, 1, False, False, False, 0)
        np.testing.assert_array_equal(st, st_b)
        np.testing.assert_array_equal(stage, stage_b)
        assert np.all(np.isnan(bj)) and w is None
        act = act * 0.5
    snap, _ = _snapshot(a)
    with pytest.raises(N.NativeError) as ei:
        a.loop_step(act, DT / 2, decide=True, iters=5)
    assert ei.value.code == N.ERR_UNSUPPORTED and "jac_T" in str(ei.value)
    with pytest.raises(N.NativeError) as ei:
        a.loop_step_end()
    assert ei.value.code == N.ERR_BAD_ARG
    now, _ = _snapshot(a)
    for f in FIELDS:
        np.testing.assert_array_equal(now[f], snap[f], err_msg=f)
    progs = [e for p, e in N.system_programs(reg("nojac")["sys_id"]) if p.endswith("_loop.hip")]
    assert progs == ["rcg::k_loop<rcg::RcgRtcSys, double>"]


@pytest.mark.parametrize("how", ["sampling", "candidates"])
def test_drop_in_loop_without_jac_runs_unfused(how):
    """LOOP (+ SEARCH) without jac_T: no fused decision exists, so the controller does not fuse - it decides by the device search
    or by the argmin over candidates=, through the separate calls."""
    kw = dict(actor_opt="sampling", n_candidates=64, rounds=2) if how == "sampling" else dict(
        candidates=np.random.default_rng(4).uniform(-5, 5, (64, 5, 1)))
    my_sys, my_ctrl, my_sim = _objects("nojac", "MPC", "quad-nomix", **kw)
    assert my_ctrl._can_fuse(my_sim) is False
    rows, c = _run("nojac", "MPC", "quad-nomix", True, 8, **kw)
    rows0, c0 = _run("nojac", "MPC", "quad-nomix", False, 8, **kw)
    assert c.fused_steps == 0 and c.fused_decisions == 0 and c.spec_hits == 0
    np.testing.assert_array_equal(rows, rows0)
    assert np.ptp(rows[:, 1]) > 1e-3


def test_a_handle_with_the_disturbance_model_is_refused():
    from rcognita_amd import _native as N

    B = 4
    e = _engine("C2", "f64", B, is_disturb=True, pars_disturb=[[1.0, 1.0], [0.0, 0.0], [1.0, 1.0]])
    e.set_state(_states("C2", B))
    snap, _ = _snapshot(e)
    with pytest.raises(N.NativeError) as ei:
        e.loop_step(None, DT)
    assert ei.value.code == N.ERR_UNSUPPORTED and "disturbance" in str(ei.value)
    now, _ = _snapshot(e)
    for f in FIELDS:
        np.testing.assert_array_equal(now[f], snap[f], err_msg=f)


def test_the_pinned_buffer_boundary_of_the_out_pendulum():
    """MPC row of the pendulum with an output map: 2 + 1 + 2 + 3 = 8 doubles, + the action handed in + the sequence number = 10
    per env: 204 envs fit the 16-KB buffer, 205 do not - natively and in CtrlOptPred._can_fuse."""
    from rcognita_amd import _native as N

    for B, fits in ((204, True), (205, False)):
        assert (B * 10 * 8 <= 16384) is fits
        e = _engine("out", "f64", B)
        e.set_state(clean_states(B))
        assert e._loop_dims[0] == 8
        act = np.zeros((B, 1))
        if fits:
            st, _, _, _, _, y = e.loop_step(act, DT, with_obs=True)
            np.testing.assert_array_equal(y, e.out(st))
        else:
            with pytest.raises(N.NativeError) as ei:
                e.loop_step(act, DT)
            assert ei.value.code == N.ERR_UNSUPPORTED and "pinned" in str(ei.value)
        e.close()
        my_sys, my_ctrl, my_sim = _objects("out", "MPC", "quad-nomix", B=B)
        assert my_ctrl._can_fuse(my_sim) is fits
    rows, c = _run("out", "MPC", "quad-nomix", True, 3, B=205)  # ... and the loop at 205 runs by the separate calls
    assert c.fused_steps == 0 and rows.shape[0] == 3 and np.all(np.isfinite(rows))


# ---- 6. the size test of the built-ins ------------------------------------------------------------------------------------------
def test_sys3wrobot_loop_at_171_envs_runs_by_the_separate_calls():
    """12 doubles per env (row 9, action 2, sequence number 1): the native bound is 170 envs.  At 171 the drop-in loop runs - by
    the separate calls - and equals the fuse = False run."""
    from tests.test_hip_loop_step import _run as run_builtin

    fused, c1 = run_builtin("3wrobot", "MPC", "quad-nomix", True, 3, B=171)
    plain, c0 = run_builtin("3wrobot", "MPC", "quad-nomix", False, 3, B=171)
    assert c1.fused_steps == 0 and c0.fused_steps == 0
    np.testing.assert_array_equal(fused, plain)
    ok, c = run_builtin("3wrobot", "MPC", "quad-nomix", True, 3, B=170)
    assert c.fused_steps == 3 and np.all(np.isfinite(ok))
