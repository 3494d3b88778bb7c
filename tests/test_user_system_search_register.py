"""The device candidate search on systems compiled at run time (rcg.h: the policy member SEARCH): what a registration reports and
compiles, and what CtrlOptPred accepts - hipRTC compiles without a device, so these run on CPU.  The GPU side is
test_hip_user_system_search.py, which takes its policy sources from here."""
import numpy as np
import pytest

from rcognita_amd import _native as N
from tests.test_user_system_critic_register import pendulum_critic_source
from tests.test_user_system_out_register import pendulum_out_source
from tests.test_user_system_register import PENDULUM

SEARCH_MEMBER = "  static constexpr bool SEARCH = true;\n"
PEND_PARS = [1.3, 9.81, 0.7]
BND = np.array([[-5.0, 5.0]])


def with_search(src):
    """A policy source with the opt-in member added behind its dimensions (as with_critic adds CRITIC)."""
    i = src.index("static constexpr int DS")
    j = src.index("\n", i) + 1
    return src[:j] + SEARCH_MEMBER + src[j:]


def without_jac(src):
    """The plain pendulum's source without its jac_T: a right-hand side and nothing else."""
    return src[: src.index("  template <typename real, bool HW = false>\n  __device__ __forceinline__ static void jac_T")] + "};\n"


def pendulum_search_source(name, jac=False):
    """The pendulum of test_user_system_register.py (DS = 2, DU = 1, no output map) that opts in to the search."""
    src = PENDULUM.replace("PendulumT", name)
    return with_search(src if jac else without_jac(src))


def pendulum_out_search_source(name, critic=False):
    """The pendulum with y = (sin th, cos th, om) (F14 / F15) that opts in to the search, and to the critic kernels."""
    return with_search(pendulum_critic_source(name) if critic else pendulum_out_source(name))


# ---- NumPy restatement of the decision: the reference's _actor_cost for the pendulum, vectorised, and the rounds of the search ---
_FEATURES = ("quad-lin", "quadratic", "quad-nomix", "quad-mix")


def _regressor(cs, chi, y, u):
    """controllers.py:1200-1212 over chi = [y - target, u] [..., n]; quad-mix over the raw observation."""
    if cs in ("quad-lin", "quadratic"):
        iu, ju = np.triu_indices(chi.shape[-1])  # uptria2vec: the row-major upper triangle (utilities.py:81-96)
        tri = chi[..., iu] * chi[..., ju]
        return np.concatenate([tri, chi], axis=-1) if cs == "quad-lin" else tri
    if cs == "quad-nomix":
        return chi * chi
    return np.concatenate([y * y, (y[..., :, None] * u[..., None, :]).reshape(y.shape[:-1] + (-1,)), u * u], axis=-1)


def pend_cost(cand, ys, xs, R1, gamma, target, h, pars, mode="MPC", cs=None, w=None, out=True, dtype=np.float64):
    """CtrlOptPred._actor_cost (controllers.py:1284-1328) of the pendulum for candidates [B, K, N] from states xs [B, 2] and
    observations ys [B, dy] -> J [B, K]: actor_cost_out (MPC) and actor_cost_critic (RQL / SQL) of the output-map tests, restated
    over arrays (pinned on them below); `out`: y = (sin th, cos th, om), else y = x.  `dtype`: the arithmetic's width (the
    float32 dry run of the GPU tests' seeds)."""
    f = np.dtype(dtype).type
    cand = np.asarray(cand, dtype=dtype)
    B, K, N = cand.shape
    m, g, l = (f(v) for v in pars)
    x = np.broadcast_to(np.asarray(xs, dtype=dtype)[:, None, :], (B, K, 2)).copy()
    y = np.broadcast_to(np.asarray(ys, dtype=dtype)[:, None, :], (B, K, np.shape(ys)[-1]))
    R1 = np.asarray(R1, dtype=dtype)
    tgt = None if target is None else np.asarray(target, dtype=dtype)
    wk = None if w is None else np.asarray(w, dtype=dtype)[:, None, :]
    J, gk = np.zeros((B, K), dtype=dtype), f(1)
    for k in range(N):
        u = cand[:, :, k, None]
        if k > 0:
            up = cand[:, :, k - 1]
            x = x + f(h) * np.stack([x[..., 1], -g / l * np.sin(x[..., 0]) + up / (m * l * l)], axis=-1)
            y = np.stack([np.sin(x[..., 0]), np.cos(x[..., 0]), x[..., 1]], axis=-1) if out else x
        chi = np.concatenate([y if tgt is None else y - tgt, u], axis=-1)
        if mode == "MPC" or (mode == "RQL" and k < N - 1):
            J = J + gk * np.einsum("...i,ij,...j->...", chi, R1, chi)
        else:
            J = J + np.sum(wk * _regressor(cs, chi, y, u), axis=-1)
        gk = gk * f(gamma)
    return J


def search_replay(sampler, cost, u0, rounds, centre=None):
    """The rounds of rcg_actor_search (oracle/search_oracle.py::actor_search) over `sampler(round, centre [B, N, du]) ->
    [B, K, N, du]` with `cost(cand [B, K, N]) -> J [B, K]` -> (sequence [B, N, du], J [B], index [B]) of the last round."""
    from oracle import rcg_oracle as O

    c = np.array(u0 if centre is None else centre, dtype=np.float64)
    bj = bi = None
    for r in range(int(rounds)):
        cand = np.asarray(sampler(r, c), dtype=np.float64)
        bj, bi = O.argmin_first(np.asarray(cost(cand[..., 0]), dtype=np.float64))
        c = cand[np.arange(len(c)), bi]
    return c, bj, bi


def oracle_sampler(K, seed, env_id, episode_idx, step_idx, Nh, action_init=None):
    """`sampler` of search_replay from the oracle's own producer (oracle/search_oracle.py::candidates_sample) for the pendulum."""
    import types

    from oracle import search_oracle as S

    cfg = types.SimpleNamespace(n_actor=Nh, du=1, ctrl_bnds=BND)
    return lambda r, c: S.candidates_sample(cfg, seed, env_id, episode_idx, step_idx, K, r, centre=c, action_init=action_init)


def test_pend_cost_is_the_restatement_of_the_output_map_tests():
    from tests.test_user_system_critic_register import actor_cost_critic, load_f15
    from tests.test_user_system_out_register import actor_cost_out, load_f14

    meta, z = load_f14()
    h, pars = meta["pred_step_size"], meta["pars"]
    for ci, case in enumerate(meta["cases"]):
        target = z["a_target"][ci] if case["cost"] == "target" else None
        xs, ys, seq = z["a_state_sys"][ci, :8], z["a_obs"][ci, :8], z["a_seq"][ci, :8]
        J = pend_cost(seq[:, None, :], ys, xs, z["a_R1"][ci], case["gamma"], target, h, pars)[:, 0]
        ref = [actor_cost_out(xs[i], ys[i], seq[i], z["a_R1"][ci], case["gamma"], target, h, pars) for i in range(8)]
        np.testing.assert_allclose(J, ref, rtol=1e-13)
        np.testing.assert_allclose(J, z["a_J"][ci, :8], rtol=1e-12)
    meta, z = load_f15()
    tgt, R1, g = np.array(meta["target"]), np.diag(meta["R1"]), meta["gamma"]
    for cs in _FEATURES:
        for mode in ("RQL", "SQL"):
            p = f"e_{mode}_{cs.replace('-', '_')}"
            xs, ys, seq, w = (z[p + s][:8] for s in ("_state_sys", "_obs", "_seq", "_w"))
            J = pend_cost(seq[:, None, :], ys, xs, R1, g, tgt, h, pars, mode=mode, cs=cs, w=w)[:, 0]
            ref = [actor_cost_critic(mode, cs, xs[i], ys[i], seq[i], w[i], R1, g, tgt, h, pars) for i in range(8)]
            np.testing.assert_allclose(J, ref, rtol=1e-12)
            np.testing.assert_allclose(J, z[p + "_J"][:8], rtol=1e-11)
    # without an output map: y = x
    x = np.array([[0.4, -0.3]])
    seq = np.linspace(-1, 1, 6)[None, None, :]
    J = pend_cost(seq, x, x, np.diag([10.0, 1.0, 0.1]), 0.9, None, 0.02, PEND_PARS, out=False)[0, 0]
    xx, ref = x[0].copy(), 0.0
    for k in range(6):
        if k:
            xx = xx + 0.02 * np.array([xx[1], -9.81 / 0.7 * np.sin(xx[0]) + seq[0, 0, k - 1] / (1.3 * 0.49)])
        ref += 0.9 ** k * (10 * xx[0] ** 2 + xx[1] ** 2 + 0.1 * seq[0, 0, k] ** 2)
    assert abs(J - ref) <= 1e-13 * ref


# ---- the inputs of the GPU tests (test_hip_user_system_search.py), and their dry runs on the CPU -----------------------------------
SEEDS = {"plain": 10, "out diag 0": 8, "out diag 1": 8, "out full 0": 8, "out full 1": 8, "out target 0": 8, "out target 1": 8,
         "RQL quad-nomix": 8, "RQL quad-mix": 8, "SQL quad-nomix": 8, "SQL quad-mix": 8}
F14_SEARCH_GAP = 0.0033613  # worst J / J_slsqp - 1 of the CPU replay on F14 (b), K = 256, rounds = 6, seed 0 (pinned below)


def search_inputs(seed, B=29):
    """States x [B, 2], lagged states x + dx (the observation of a decision is out() of those) and critic weights in [0.1, 2]."""
    rng = np.random.default_rng(seed)
    x = np.stack([rng.uniform(-3, 3, B), rng.uniform(-2, 2, B)], axis=-1)
    return x, x + rng.uniform(-0.02, 0.02, x.shape), rng.uniform(0.1, 2, (B, 14))


def _gpu_case(key):
    """The arguments of pend_cost and the horizon of the GPU test whose seed is SEEDS[key]."""
    from tests.test_user_system_critic_register import load_f15
    from tests.test_user_system_out_register import load_f14, pend_out

    x, xl, w = search_inputs(SEEDS[key])
    if key == "plain":
        return dict(ys=xl, xs=x, R1=np.diag([10.0, 1.0, 0.1]), gamma=0.96, target=None, h=0.02, pars=PEND_PARS, out=False), 6
    if key.startswith("out"):
        meta, z = load_f14()
        _, kind, long = key.split()
        ci = {"diag": 0, "full": 2, "target": 4}[kind] + 6 * int(long)
        return dict(ys=pend_out(xl), xs=x, R1=z["a_R1"][ci], gamma=meta["cases"][ci]["gamma"],
                    target=z["a_target"][ci] if kind == "target" else None, h=meta["pred_step_size"], pars=PEND_PARS), \
            (meta["Nactor"] if int(long) else 5)
    meta, _ = load_f15()
    mode, cs = key.split()
    return dict(ys=pend_out(xl), xs=x, R1=np.diag(meta["R1"]), gamma=meta["gamma"], target=np.array(meta["target"]),
                h=meta["pred_step_size"], pars=PEND_PARS, mode=mode, cs=cs, w=w[:, : meta["dim_critic"][cs]]), meta["Nactor"]


def float32_dry_run(key, B=29, K=192, rounds=3):
    """Share of envs whose winning sequence changes when the costs of the search (the oracle's own candidates rounded to float32,
    the GPU test's seed 7 and STEP_IDX = env index) are computed in numpy float32 instead of float64."""
    kw, Nh = _gpu_case(key)
    u0 = np.full((B, Nh, 1), BND[0, 0] / 10.0)
    sampler = oracle_sampler(K, 7, np.arange(B), np.zeros(B, int), np.arange(B), Nh)
    r32 = lambda a: None if a is None else np.asarray(a, dtype=np.float32)  # noqa: E731
    # (both searches over the candidates a float32 handle produces: rounded to float32, as the GPU test replays them)
    sampler = lambda r, c, s=sampler: s(r, c).astype(np.float32).astype(np.float64)  # noqa: E731
    kw = dict(kw, ys=r32(kw["ys"]).astype(np.float64), xs=r32(kw["xs"]).astype(np.float64),
              w=None if kw.get("w") is None else r32(kw["w"]).astype(np.float64))
    U64, _, _ = search_replay(sampler, lambda c: pend_cost(c, **kw), u0, rounds)
    U32, _, _ = search_replay(sampler, lambda c: pend_cost(c, dtype=np.float32, **kw), u0, rounds)
    return float(np.mean(np.any(U64 != U32, axis=(1, 2))))


@pytest.mark.parametrize("key", sorted(SEEDS))
def test_the_float32_seeds_are_far_from_ties(key):
    """The float32 GPU tests cap the share of envs that leave the float64 replay's sequence at 20 %: their seeds are chosen so
    that this dry run changes under 10 %, half the cap."""
    share = float32_dry_run(key)
    print(f"{key}: {100 * share:.1f} % of the envs change their winner in float32")
    assert share < 0.10


def f14_search_gap():
    from tests.test_user_system_out_register import load_f14, pend_out

    meta, z = load_f14()
    x, B, Nh = z["b_state"], len(z["b_state"]), meta["Nactor"]
    cost = lambda c: pend_cost(c, pend_out(x), x, z["b_R1"], 1.0, None, meta["pred_step_size"], meta["pars"])  # noqa: E731
    sampler = oracle_sampler(256, 0, np.arange(B), np.zeros(B, int), np.zeros(B, int), Nh, action_init=meta["action_init"])
    _, J, _ = search_replay(sampler, cost, np.full((B, Nh, 1), meta["action_init"][0]), 6)
    return J / z["b_J_opt"] - 1


def test_f14_search_gap_on_the_cpu_replay():
    """The measurement behind test_hip_user_system_search.py::test_search_quality_vs_reference_slsqp_on_f14's bound."""
    gap = f14_search_gap()
    print(f"F14 (b), K = 256, rounds = 6: J / J_slsqp - 1 median {np.median(gap):.5f} max {np.max(gap):.5f}")
    assert abs(np.max(gap) - F14_SEARCH_GAP) <= 5e-6


def _has_search(sid):
    v = N.C.c_int32(-1)
    rc = N.lib().rcg_system_has_search(sid, N.C.byref(v))
    return rc, v.value


def test_registration_reports_has_search():
    info = N.register_system("PendulumS", pendulum_search_source("PendulumS"), 2, 1, 3)
    assert info["has_search"] and not info["has_jac"] and not info["has_out"] and not info["has_critic"]
    assert _has_search(info["sys_id"]) == (N.OK, 1)
    plain = N.register_system("PendulumT", PENDULUM, 2, 1, 3)
    assert not plain["has_search"] and _has_search(plain["sys_id"]) == (N.OK, 0)
    # SEARCH = false is the default spelled out
    off = N.register_system("PendulumSOff", pendulum_search_source("PendulumSOff").replace("SEARCH = true", "SEARCH = false"), 2, 1, 3)
    assert not off["has_search"] and _has_search(off["sys_id"]) == (N.OK, 0)
    # next to the other optional members
    both = N.register_system("PendulumYSC", pendulum_out_search_source("PendulumYSC", critic=True), 2, 1, 3)
    assert both["has_search"] and both["has_critic"] and both["has_out"] and both["dy"] == 3
    for sid in (N.SYS_3WROBOT, N.SYS_3WROBOT_NI, N.SYS_2TANK):
        assert _has_search(sid) == (N.OK, 1)
    assert _has_search(7)[0] == N.ERR_BAD_ARG
    assert N.lib().rcg_system_has_search(7, None) == N.ERR_BAD_ARG


def test_hip_info_carries_has_search():
    from rcognita_amd.systems import System

    class PendulumSInfo(System):
        hip_policy = pendulum_search_source("PendulumSInfo")

    class PendulumPlainInfo(System):
        hip_policy = PENDULUM.replace("PendulumT", "PendulumPlainInfo")

    for cls, want in ((PendulumSInfo, True), (PendulumPlainInfo, False)):
        cls(sys_type="diff_eqn", dim_state=2, dim_input=1, dim_output=2, dim_disturb=0, pars=PEND_PARS, ctrl_bnds=BND)
        assert cls._hip_info["has_search"] is want


@pytest.mark.parametrize("out", [False, True])
def test_the_opt_in_adds_nothing_to_a_registration(out):
    """rcg_system_programs right after rcg_register_system: the same expressions with and without SEARCH (the search program is
    compiled on first use)."""
    if out:
        a, b = pendulum_out_search_source("PendulumRegYS"), pendulum_out_source("PendulumRegY")
    else:
        a, b = pendulum_search_source("PendulumRegS", jac=True), PENDULUM.replace("PendulumT", "PendulumReg")
    na, nb = ("PendulumRegYS", "PendulumRegY") if out else ("PendulumRegS", "PendulumReg")
    ia, ib = N.register_system(na, a, 2, 1, 3), N.register_system(nb, b, 2, 1, 3)
    assert ia["has_search"] and not ib["has_search"]
    pa, pb = N.system_programs(ia["sys_id"]), N.system_programs(ib["sys_id"])
    assert len(pb) > 20 and not any("k_actor_search" in e for _, e in pa)
    assert [(p.replace(na, "X"), e) for p, e in pa] == [(p.replace(nb, "X"), e) for p, e in pb]


def _ctrl(sys_, actor_opt):
    from rcognita_amd.controllers import CtrlOptPred

    return CtrlOptPred(1, 2, mode="MPC", ctrl_bnds=BND, Nactor=10, sys_rhs=sys_._state_dyn, sys_out=sys_.out,
                       state_sys=np.zeros(2), stage_obj_pars=[np.diag([10.0, 1.0, 0.0])], actor_opt=actor_opt)


@pytest.mark.parametrize("actor_opt", ["sampling", "auto"])
def test_ctrl_opt_pred_accepts_a_search_policy_without_jac(actor_opt):
    from rcognita_amd.systems import System

    class PendulumSCtrl(System):
        hip_policy = pendulum_search_source("PendulumSCtrl")

    s = PendulumSCtrl(sys_type="diff_eqn", dim_state=2, dim_input=1, dim_output=2, dim_disturb=0, pars=PEND_PARS, ctrl_bnds=BND)
    assert PendulumSCtrl._hip_info["has_search"] and not PendulumSCtrl._hip_info["has_jac"]
    try:  # the refusal is gone: the call gets as far as the device (none on a CPU machine)
        ctrl = _ctrl(s, actor_opt)
    except N.NativeError as e:
        assert e.code == N.ERR_NO_DEVICE, e
    else:
        assert not ctrl._use_gradient  # 'auto' without jac_T: the search


@pytest.mark.parametrize("actor_opt", ["sampling", "auto", "gradient"])
def test_ctrl_opt_pred_without_search_and_jac_names_the_opt_in(actor_opt):
    from rcognita_amd.systems import System

    class PendulumNoSCtrl(System):
        hip_policy = without_jac(PENDULUM.replace("PendulumT", "PendulumNoSCtrl"))

    s = PendulumNoSCtrl(sys_type="diff_eqn", dim_state=2, dim_input=1, dim_output=2, dim_disturb=0, pars=PEND_PARS, ctrl_bnds=BND)
    with pytest.raises(NotImplementedError, match="SEARCH") as ei:
        _ctrl(s, actor_opt)
    assert "jac_T" in str(ei.value)


def test_sampling_on_a_policy_with_jac_but_no_search_is_refused_and_auto_keeps_the_optimiser():
    from rcognita_amd.systems import System

    class PendulumJacCtrl(System):
        hip_policy = PENDULUM.replace("PendulumT", "PendulumJacCtrl")

    s = PendulumJacCtrl(sys_type="diff_eqn", dim_state=2, dim_input=1, dim_output=2, dim_disturb=0, pars=PEND_PARS, ctrl_bnds=BND)
    with pytest.raises(NotImplementedError, match="SEARCH"):
        _ctrl(s, "sampling")
    try:
        ctrl = _ctrl(s, "auto")
    except N.NativeError as e:
        assert e.code == N.ERR_NO_DEVICE, e
    else:
        assert ctrl._use_gradient
