"""oracle/disturb_oracle.py: the disturbed right-hand side against the reference's outputs
(tests/golden/F11_disturb_*.npz), and the counter-based generator against the published Philox4x32-10 known answers
(Random123 kat_vectors).  CPU only."""
import numpy as np
import pytest

from oracle import disturb_oracle as DO
from oracle import rcg_oracle as O
from tests import disturb_closed_loop_inputs as I
from tests.conftest import load_golden
from tests.helpers import PRESETS, SYSTEMS, oracle_cfg, rand_states


def test_philox4x32_10_known_answers():
    kat = [
        ((0x00000000,) * 4, (0x00000000,) * 2, (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
        ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
        ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
         (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
    ]
    ctr = np.array([k[0] for k in kat], dtype=np.uint32)
    key = np.array([k[1] for k in kat], dtype=np.uint32)
    out = DO.philox4x32_10(ctr, key)
    np.testing.assert_array_equal(out, np.array([k[2] for k in kat], dtype=np.uint32))


def test_noise_is_a_function_of_seed_env_episode_substep_only():
    ids = np.arange(1000, dtype=np.int64)
    z = np.zeros(1000, dtype=np.int32)
    a = DO.disturb_noise(7, ids, z, z + 3)
    # an env's draw does not depend on which batch / shard it sits in
    b = DO.disturb_noise(7, ids[500:], z[500:], z[500:] + 3)
    np.testing.assert_array_equal(a[500:], b)
    assert not np.array_equal(a, DO.disturb_noise(8, ids, z, z + 3))
    assert not np.array_equal(a, DO.disturb_noise(7, ids, z + 1, z + 3))
    assert not np.array_equal(a, DO.disturb_noise(7, ids, z, z + 4))
    # 64-bit env ids reach the second counter word
    assert not np.array_equal(DO.noise_bits(7, ids, z, z), DO.noise_bits(7, ids + (1 << 32), z, z))
    # standard normal moments over 2e5 draws
    big = DO.disturb_noise(1, np.arange(100000, dtype=np.int64), np.zeros(100000, np.int32), np.zeros(100000, np.int32))
    assert abs(big.mean()) < 0.01 and abs(big.std() - 1) < 0.01 and np.all(np.isfinite(big))
    assert abs(np.mean(big[:, 0] * big[:, 1])) < 0.01


@pytest.mark.parametrize("name", SYSTEMS)
def test_F11_disturbed_rhs_matches_reference(name):
    meta, z = load_golden(f"F11_disturb_{name}")
    sys_id = PRESETS[name]["sys_id"]
    pars = np.array(meta["pars"], dtype=np.float64) if len(meta["pars"]) else np.zeros(0)
    bnds = np.array(meta["bnds"], dtype=np.float64)
    dx, dq, a = DO.closed_loop_rhs_full(sys_id, z["state"], z["disturb"], z["action"], z["xi"], pars, bnds,
                                        z["sigma"], z["mu"], z["tau"])
    ds = z["state"].shape[1]
    np.testing.assert_allclose(dx, z["rhs_full"][:, :ds], rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(dq, z["rhs_full"][:, ds:], rtol=1e-13, atol=1e-13)
    np.testing.assert_array_equal(a, z["action_clipped"])
    assert DO.DIM_DISTURB[sys_id] == meta["dim_disturb"] == z["disturb"].shape[1]
    if name == "2tank":
        assert np.all(z["rhs_full"][:, ds:] == 0)  # the reference's 2tank disturbance is inert
    else:
        assert np.any(np.abs(z["action"]) > bnds[:, 1])  # the clip was exercised


def test_ou_process_statistics_of_the_substep_scheme():
    """Holding xi over a substep makes q an AR(1) process; its stationary mean is -sigma*mu, as for the SDE."""
    cfg_sys = O.SYS_3WROBOT_NI
    sigma, mu, tau = np.array([2.0, 1.0]), np.array([0.5, -0.25]), np.array([1.5, 0.7])
    B, T, dt = 4000, 400, 0.05
    q = np.zeros((B, 2))
    x = np.zeros((B, 3))
    u = np.zeros((B, 2))
    ids = np.arange(B, dtype=np.int64)
    ep = np.zeros(B, dtype=np.int32)
    for t in range(T):
        xi = DO.disturb_noise(3, ids, ep, np.full(B, t, dtype=np.int32))
        x, q = DO.rk4_step_full(cfg_sys, x, q, u, xi, np.zeros(0), np.zeros((2, 2)), sigma, mu, tau, dt)
    np.testing.assert_allclose(q.mean(axis=0), -sigma * mu, atol=0.12)
    assert np.all(np.isfinite(x))


# ---------------------------------------------------------------------------------------------------------------------
# the disturbed closed loop = the undisturbed composition with another env step (control_tick(..., sim=DO.stepper(d))):
# what tests/test_hip_disturb_closed_loop.py relies on about the oracle and about its own inputs
# ---------------------------------------------------------------------------------------------------------------------
ENV_FIELDS = ["state", "state_prev", "action", "accum", "step_idx", "episode_idx", "best_J", "best_idx", "w_critic", "w_prev",
              "obs_buf", "act_buf"]


@pytest.mark.parametrize("mode", ["MPC", "RQL"])
@pytest.mark.parametrize("name", SYSTEMS)
def test_an_inert_disturbance_model_leaves_the_closed_loop_bit_equal(name, mode):
    """sigma = 0, disturb_init = 0, any tau: q stays 0 and every EnvBatch field of control_tick(..., sim=stepper) is the
    undisturbed control_tick's, bit for bit; control_tick_opt and control_tick_nominal take the same hook."""
    from oracle import nominal_oracle as NO

    rng = np.random.default_rng(5)
    B, K, T = 11, 16, 4
    kw = dict(n_actor=4, substeps_per_tick=2)
    if mode == "RQL":
        kw.update(mode=O.MODE_RQL, critic_struct=O.CRITIC_QUAD_NOMIX, n_critic=4, buffer_size=6, gamma=0.95)
    cfg = oracle_cfg(name, **kw)
    d = DO.DisturbCfg([0.0, 0.0], [0.3, -0.4], [2.0, 1.5], seed=9, env_id_base=77)
    x0 = rand_states(rng, name, B)
    cand = O.grid_candidates(cfg, K)

    def run(tick, sim):
        env = O.new_batch(cfg, x0)
        DO.attach(cfg, env, d)
        for _ in range(T):
            tick(env, sim)
        return env

    ticks = [lambda env, sim: O.control_tick(cfg, env, cand, sim=sim), lambda env, sim: O.control_tick_opt(cfg, env, 3, sim=sim)]
    if name != "2tank" and mode == "MPC":
        ticks.append(lambda env, sim: NO.control_tick_nominal(cfg, env, 0.5, 10.0, 1.0, sim=sim))
    for tick in ticks:
        a, b = run(tick, None), run(tick, DO.stepper(d))
        for f in ENV_FIELDS:
            np.testing.assert_array_equal(getattr(a, f), getattr(b, f), err_msg=f)
        np.testing.assert_array_equal(b.disturb, np.zeros_like(b.disturb))
        np.testing.assert_array_equal(b.substep_idx, np.full(B, 2 * T, np.int32))  # the counter advances per substep
        np.testing.assert_array_equal(a.substep_idx, np.zeros(B, np.int32))


def test_a_constant_disturbance_shifts_the_action_of_the_dynamic_robot():
    """Sys3WRobot, tau = 0: q never moves and enters as (F + q_0) / m, (M + q_1) / I - the disturbed step under u is the
    undisturbed step under u + q while u + q stays inside the bounds.  Exactly: both sides add the same two numbers."""
    rng = np.random.default_rng(21)
    B, S = 41, 5
    cfg = oracle_cfg("3wrobot")
    d = DO.DisturbCfg([3.0, 2.0], [0.5, -0.2], [0.0, 0.0], seed=4)
    x0 = rand_states(rng, "3wrobot", B)
    u = rng.uniform(-1, 1, (B, 2)) * [100.0, 30.0]
    q = rng.uniform(-1, 1, (B, 2)) * [50.0, 20.0]
    assert np.all(np.abs(u + q) <= cfg.ctrl_bnds[:, 1])
    a, b = O.new_batch(cfg, x0, action0=u), O.new_batch(cfg, x0, action0=u + q)
    DO.attach(cfg, a, d)
    a.disturb = q.copy()
    DO.sim_substeps(cfg, a, d, S)
    O.sim_substeps(cfg, b, S)
    np.testing.assert_array_equal(a.state, b.state)
    np.testing.assert_array_equal(a.state_prev, b.state_prev)
    np.testing.assert_array_equal(a.disturb, q)
    np.testing.assert_array_equal(a.substep_idx, np.full(B, S, np.int32))


def test_episode_reset_twin_restores_the_disturbance_and_restarts_the_counter():
    cfg = oracle_cfg("3wrobotNI")
    d = I.dcfg()
    x0 = rand_states(np.random.default_rng(1), "3wrobotNI", 7)
    env = O.new_batch(cfg, x0)
    DO.attach(cfg, env, d)
    DO.sim_substeps(cfg, env, d, 3)
    q_ep0 = env.disturb.copy()
    DO.episode_reset(cfg, env, d, x0)
    np.testing.assert_array_equal(env.disturb, np.tile(I.DISTURB_INIT, (7, 1)))
    np.testing.assert_array_equal(env.substep_idx, np.zeros(7, np.int32))
    np.testing.assert_array_equal(env.episode_idx, np.ones(7, np.int32))
    np.testing.assert_array_equal(env.state, x0)
    DO.sim_substeps(cfg, env, d, 3)
    assert not np.array_equal(env.disturb, q_ep0)  # the episode index is part of the noise counter


def _gap_cases():
    """Every float64 free run of the GPU file that relies on the device taking the oracle's best_idx."""
    out = []
    for name, K, streamed, _ in I.TICK_CASES:
        for tag, kw in I.MODE_KW:
            okw = dict(n_actor=I.NH_A, substeps_per_tick=I.S_A, **kw)
            out.append(pytest.param(name, K, streamed, okw, I.B_A, I.T_A, I.seed_off(name, K, tag), I.BEST_J_TOL[tag], None,
                                    id=f"a-{name}-K{K}-{'streamed' if streamed else 'grid'}-{tag}"))
    for name, K, streamed in I.TICKS_CASES:
        out.append(pytest.param(name, K, streamed, dict(I.TICKS_KW), I.B_B, I.T_B, 11, 1e-10, None,
                                id=f"b-{name}-K{K}-{'streamed' if streamed else 'grid'}"))
    for which in I.CORNERS:
        out.append(pytest.param(I.CORNERS[which][0], I.K_C, False, None, I.B_C, I.T_C, 11, 1e-10, which, id=f"c-{which}"))
    return out


@pytest.mark.parametrize("name,K,streamed,okw,B,T,seed_off,tol,corner", _gap_cases())
def test_gap_between_best_and_second_clears_the_tolerance_on_the_gpu_inputs(name, K, streamed, okw, B, T, seed_off, tol, corner):
    """A float64 device run is required to take the oracle's candidate on every env and tick (``ties == 0``).  That is a
    fair demand only where the oracle's own best and second-best costs are further apart than the rounding the cost is
    held to: at least 10 x the case's best_J tolerance, relative to the env's largest cost (the scale parity.check_tick uses)."""
    pars = None
    if corner is not None:
        name, kw, x0, pars = I.corner_inputs(corner)
        cfg = oracle_cfg(name, **I.oracle_kw(kw))
        cand = O.grid_candidates(cfg, K)
    else:
        cfg = oracle_cfg(name, **okw)
        x0, cand = I.tick_inputs(name, K, streamed, B=B, Nh=cfg.n_actor, cfg=cfg, seed_off=seed_off)
    _, _, gap = I.oracle_run(cfg, x0, cand, T, pars=pars)
    assert gap.shape == (T, B) and np.all(np.isfinite(gap))
    print(f"smallest gap {gap.min():.3e} (bound {10 * tol:.1e})")
    assert gap.min() >= 10 * tol, (gap.min(), np.unravel_index(np.argmin(gap), gap.shape))


@pytest.mark.parametrize("tag,kw", I.MODE_KW, ids=[t for t, _ in I.MODE_KW])
@pytest.mark.parametrize("name,K,streamed,_k", I.TICK_CASES, ids=[f"{c[0]}-K{c[1]}-{'streamed' if c[2] else 'grid'}" for c in I.TICK_CASES])
def test_the_disturbance_changes_the_closed_loop_of_the_gpu_inputs(name, K, streamed, _k, tag, kw):
    """Non-vacuity: on the robots the disturbed oracle run differs from the undisturbed one - the state after T ticks by
    more than 0.1 and, with a generated grid, the chosen candidate on at least one env and tick (asserted per robot and mode;
    not on the ref_lag twin of the MPC case, whose decisions from the state one substep back happen to coincide: 0 of 78); the
    tank's is the same run."""
    cfg = oracle_cfg(name, n_actor=I.NH_A, substeps_per_tick=I.S_A, **kw)
    x0, cand = I.tick_inputs(name, K, streamed, cfg=cfg, seed_off=I.seed_off(name, K, tag))
    a, ia, _ = I.oracle_run(cfg, x0, cand, I.T_A, disturbed=True)
    b, ib, _ = I.oracle_run(cfg, x0, cand, I.T_A, disturbed=False)
    if name == "2tank":
        for f in ENV_FIELDS:
            np.testing.assert_array_equal(getattr(a, f), getattr(b, f), err_msg=f)
        np.testing.assert_array_equal(a.disturb, np.full((I.B_A, 1), I.DISTURB_INIT[0]))
        return
    diff = float(np.max(np.abs(a.state - b.state)))
    print(f"state differs by {diff:.3g}, best_idx on {np.mean(ia != ib):.1%} of the env-ticks")
    assert diff > 0.1
    if not streamed and not kw.get("ref_lag"):
        assert np.any(ia != ib)
