"""The cases and inputs of tests/test_hip_disturb_closed_loop.py (GPU), shared with tests/test_disturb_oracle.py (CPU), which
asserts on exactly these seeds and shapes what the GPU file relies on: the oracle's best-to-second gap (the float64 runs assert
``ties == 0``) and that the disturbance changes the closed loop at all.  No test in here; imports nothing from the package."""
import numpy as np

from oracle import disturb_oracle as DO
from oracle import rcg_oracle as O
from tests.helpers import oracle_cfg, rand_actions, rand_states

# the disturbance model of every case (the values of test_hip_ticks.py's disturbed cases; env ids beyond the batch)
PARS_DISTURB = [[30.0, 10.0], [0.5, -0.2], [2.0, 1.5]]
DISTURB_INIT = [1.0, -2.0]
SEED, ENV_ID_BASE = 31, 1000
DIST = dict(is_disturb=True, pars_disturb=PARS_DISTURB, disturb_init=DISTURB_INIT, seed=SEED, env_id_base=ENV_ID_BASE)


def dcfg(**over):
    kw = dict(seed=SEED, env_id_base=ENV_ID_BASE, disturb_init=DISTURB_INIT)
    kw.update(over)
    return DO.DisturbCfg(*PARS_DISTURB, **kw)


# ---- (a) rcg_control_tick -----------------------------------------------------------------------------------------------------
B_A, NH_A, S_A, T_A = 13, 6, 2, 6
TICK_CASES = [  # name, K, streamed, decision kernel of an MPC handle
    ("3wrobot", 64, False, "k_actor"),
    ("3wrobot", 16, True, "k_actor_dma_packed"),
    ("3wrobotNI", 100, True, "k_actor_dma"),
    ("2tank", 32, False, "k_actor"),
    ("2tank", 16, True, "k_actor_dma_packed"),
]
CRITIC = dict(n_critic=4, buffer_size=6, gamma=0.95)
MODES = {  # mode -> [(id, oracle / engine keywords)]
    "MPC": [("MPC", dict(gamma=0.99)), ("MPC-ref_lag", dict(gamma=0.99, ref_lag=True))],
    "RQL": [("RQL", dict(mode=O.MODE_RQL, critic_struct=O.CRITIC_QUAD_NOMIX, **CRITIC))],
    "SQL": [("SQL", dict(mode=O.MODE_SQL, critic_struct=O.CRITIC_QUAD_MIX, **CRITIC))],
}
MODE_KW = [(tag, kw) for m in MODES.values() for tag, kw in m]
# best_J tolerance of the float64 run of a case (MPC 1e-10; RQL / SQL 1e-7, tests/test_hip_critic.py)
BEST_J_TOL = {"MPC": 1e-10, "MPC-ref_lag": 1e-10, "RQL": 1e-7, "SQL": 1e-7}
# rng = default_rng(SEED_OFF + K).  One case has a seed of its own: with 11 the oracle's smallest best-to-second gap of
# (3wrobot, grid K = 64, RQL) is 5.8e-7 of the env's largest cost, below the 1e-6 the float64 run needs (10 x its best_J
# tolerance; tests/test_disturb_oracle.py asserts it) - the fitted critic of tick 3 nearly ties two grid points on one env; of
# 200 seeds tried, 103 leaves the widest gap there (3.0e-6)
SEED_OFF = {("3wrobot", 64, "RQL"): 103}


def seed_off(name, K, tag):
    return SEED_OFF.get((name, K, tag), 11)


def tick_inputs(name, K, streamed, B=B_A, Nh=NH_A, real=np.float64, cfg=None, seed_off=11):
    """(x0 [B, ds], cand): the draws of test_control_tick_closed_loop_vs_oracle, rounded to the handle's element type."""
    rng = np.random.default_rng(seed_off + K)
    x0 = rand_states(rng, name, B).astype(real)
    if streamed:
        cand = rand_actions(rng, name, (B, K, Nh)).astype(real)
    else:
        cand = O.grid_candidates(cfg if cfg is not None else oracle_cfg(name, n_actor=Nh), K)
    return x0, cand


# ---- (b) T ticks in one launch ------------------------------------------------------------------------------------------------
B_B, NH_B, S_B, T_B = 70, 5, 2, 5
TICKS_CASES = [("3wrobot", 64, False), ("3wrobot", 16, True), ("3wrobotNI", 64, False), ("3wrobotNI", 16, True)]
TICKS_KW = dict(n_actor=NH_B, substeps_per_tick=S_B)

# ---- (c) corners --------------------------------------------------------------------------------------------------------------
B_C, NH_C, K_C, T_C = 9, 5, 16, 4
CORNERS = {
    "accum_every_substep": ("3wrobot", dict(accum_every_substep=True, substeps_per_tick=3)),
    "target": ("3wrobotNI", dict(target=[0.5, -1.0, 0.25], substeps_per_tick=2)),
    "per_env_pars": ("3wrobot", dict(per_env_pars=True, substeps_per_tick=2)),
}


def corner_inputs(which, real=np.float64):
    """(name, keywords, x0, per-env parameters or None): m and I drawn per env as test_per_env_parameters draws them."""
    name, kw = CORNERS[which]
    rng = np.random.default_rng(8 + len(which))
    pars = np.stack([rng.uniform(5, 20, B_C), rng.uniform(0.5, 2, B_C)], axis=-1) if kw.get("per_env_pars") else None
    x0 = rand_states(rng, name, B_C).astype(real)
    return name, dict(n_actor=NH_C, **kw), x0, pars


def oracle_kw(kw):
    return {k: v for k, v in kw.items() if k not in ("per_env_pars", "action_init")}


# ---- the oracle's run of a case -----------------------------------------------------------------------------------------------
def oracle_run(cfg, x0, cand, T, disturbed=True, pars=None):
    """T oracle ticks.  Returns (env, best_idx [T, B], gap [T, B]): gap = (second best - best) / the env's largest finite |J|."""
    env = O.new_batch(cfg, np.asarray(x0, dtype=np.float64), pars=pars)
    d = dcfg()
    DO.attach(cfg, env, d)
    sim = DO.stepper(d) if disturbed else None
    idx, gap = [], []
    for _ in range(T):
        J = O.control_tick(cfg, env, np.asarray(cand, dtype=np.float64), sim=sim)
        Jc = np.where(np.isfinite(J), J, np.inf)
        two = np.partition(Jc, 1, axis=1)[:, :2]
        scale = np.max(np.abs(np.where(np.isfinite(J), J, 0.0)), axis=1)
        gap.append((two[:, 1] - two[:, 0]) / scale)
        idx.append(env.best_idx.copy())
    return env, np.array(idx), np.array(gap)
