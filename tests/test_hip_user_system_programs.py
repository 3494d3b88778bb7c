"""The programs a system compiled at run time compiles on first use (rcg_rtc.hip: lazy_function, RtcSystem::lazy) on the GPU.

One pendulum with an output map that opts in to CRITIC, SEARCH and TICKS, and the five kinds of program a handle of it can ask
for: a k_actor_dma instance, the critic program, a k_actor_search instance, a k_ticks and a k_ticks_mem instance.  For each kind:
the first handle's call appends exactly the program's lines to rcg_system_programs - its own file, the name expressions written
out below - and a second handle of the same configuration finds the program (nothing is appended) and computes the same bits.
The shapes are the smallest at which each path exists: float32, 64 envs, Nactor = 5, K = 64.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.test_user_system_search_register import with_search  # noqa: E402
from tests.test_user_system_ticks_register import BND, PEND_PARS, pendulum_out_ticks_source  # noqa: E402

pytestmark = pytest.mark.gpu

NAME = "PendulumYP"
B, NH, K = 64, 5, 64
FIELDS = ["FIELD_STATE", "FIELD_STATE_PREV", "FIELD_ACTION", "FIELD_ACCUM", "FIELD_STEP_IDX", "FIELD_STATUS", "FIELD_BEST_J",
          "FIELD_BEST_IDX"]
CRITIC_FIELDS = FIELDS + ["FIELD_W_CRITIC", "FIELD_W_PREV", "FIELD_OBS_BUF", "FIELD_ACT_BUF"]
SYS = "rcg::RcgRtcSys"

# kind -> (the file, the lines' name expressions in order, RQL handle?, the kernel rcg_last_launch must name)
PROGRAMS = {
    # <Sys, real, R = Nactor * du, TGT, variant = DMA_MPC_G1>
    "dma": ("_dma.hip", [f"rcg::k_actor_dma<{SYS}, float, 5, false, 0>"], False, "k_actor_dma"),
    # quad-nomix = 2; Ncritic - 1 = 3 TD rows and 4 weights: the one-lane fit of three rows
    "critic": ("_critic.hip", [f"rcg::k_critic<{SYS}, float>", f"rcg::k_critic_cost<{SYS}, float>",
                               f"rcg::k_critic_fit<{SYS}, float, 2, 3>"], True, "k_critic_fit"),
    # <Sys, real, GENERIC, TGT, NC = Nactor: register rows>
    "search": ("_search.hip", [f"rcg::k_actor_search<{SYS}, float, false, false, 5>"], False, "k_actor_search"),
    # <Sys, real, GENERIC, TGT, STREAM>
    "ticks": ("_ticks.hip", [f"rcg::k_ticks<{SYS}, float, false, false, false>"], False, "k_ticks"),
    # <Sys, real, CS, MAXM, TGT, ML, STREAM>
    "ticks_mem": ("_ticks_mem.hip", [f"rcg::k_ticks_mem<{SYS}, float, 2, 3, false, false, false>"], True, "k_ticks"),
}

_REG = {}


def _system():
    from rcognita_amd import _native as N

    if not _REG:
        _REG.update(N.register_system(NAME, with_search(pendulum_out_ticks_source(NAME, critic=True)), 2, 1, 3))
        assert _REG["has_out"] and _REG["has_critic"] and _REG["has_search"] and _REG["has_ticks"]
    return _REG["sys_id"]


def _engine(rql):
    from rcognita_amd import Engine, EngineConfig

    cfg = dict(sys_id=_system(), batch=B, dtype="f32", Nactor=NH, pars=PEND_PARS, ctrl_bnds=BND, R1=np.diag([10.0, 3.0, 1.0, 0.1]),
               dt_sim=0.01, sampling_time=0.02, pred_step_size=0.02)
    if rql:
        cfg.update(mode="RQL", critic_struct="quad-nomix", Ncritic=4, buffer_size=10, gamma=0.95)
    e = Engine(EngineConfig(**cfg))
    rng = np.random.default_rng(11)
    e.set_state(np.stack([rng.uniform(-1.5, 1.5, B), rng.uniform(-1, 1, B)], axis=-1))
    return e


def _call(kind, e, cand):
    """The call of a kind on one handle -> what it wrote, as {name: array}."""
    from rcognita_amd import _native as N

    out = {}
    if kind == "dma":
        e.control_tick(e.to_device(cand), K=K)
    elif kind == "critic":
        e.critic_update()
    elif kind == "search":
        out = dict(zip(("action", "u_best", "best_J", "best_idx"), e.actor_search(K=K, rounds=2)))
    else:
        e.control_ticks(3, K)
    for f in (CRITIC_FIELDS if PROGRAMS[kind][2] else FIELDS):
        out[f] = e.get_field(getattr(N, f))
    return out


@pytest.mark.parametrize("kind", list(PROGRAMS))
def test_first_use_compiles_one_program_and_the_next_handle_finds_it(kind):
    from rcognita_amd import _native as N

    suffix, exprs, rql, kernel = PROGRAMS[kind]
    sid = _system()
    cand = np.random.default_rng(5).uniform(BND[0, 0], BND[0, 1], (B, K, NH, 1)).astype(np.float32)
    launch_kind = N.KERNEL_CRITIC if kind == "critic" else N.KERNEL_ACTOR
    a, b = _engine(rql), _engine(rql)

    before = N.system_programs(sid)
    wrote_a = _call(kind, a, cand)
    after = N.system_programs(sid)
    assert a.last_launch(launch_kind)["kernel"] == kernel, a.last_launch(launch_kind)
    assert after == before + [(NAME + suffix, e) for e in exprs], after[len(before):]
    assert len(set(after)) == len(after), after

    wrote_b = _call(kind, b, cand)
    assert b.last_launch(launch_kind) == a.last_launch(launch_kind)
    assert N.system_programs(sid) == after
    assert wrote_a.keys() == wrote_b.keys()
    for f in wrote_a:
        u, v = np.asarray(wrote_a[f]), np.asarray(wrote_b[f])
        assert u.dtype == v.dtype and u.shape == v.shape and u.tobytes() == v.tobytes(), (kind, f)
    if kind != "critic":  # (the call did something: the decision is not the handle's initial action)
        act = wrote_a["action"] if kind == "search" else wrote_a["FIELD_ACTION"]
        assert np.any(act != 0), kind

    if kind == "ticks":  # the instance does not depend on T
        a.control_ticks(5, K)
        assert a.last_launch(N.KERNEL_ACTOR)["kernel"] == "k_ticks"
        assert N.system_programs(sid) == after
    a.close()
    b.close()
