"""k_actor_dma's float64 wave argmin (rcg_math.hpp: wave_min_f64 + wave_min_u32 - DPP stages and v_readlane, no LDS), on the
GPU: lower cost, then lower index.  An env's minimum cost is made to appear twice - a duplicated row - in different tiles and
lanes, above and below the original; a ragged tile's lanes without a row never win, not even when every cost is +inf."""
import numpy as np
import pytest

from tests.helpers import SYSTEMS, assert_kernel, both, rand_actions, rand_states

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("K", [40, 96, 256])  # one ragged tile; a full tile and a ragged one; four tiles
@pytest.mark.parametrize("name", SYSTEMS)
def test_the_lower_index_of_a_tie_wins(name, K):
    rng = np.random.default_rng(K)
    B, Nh = 24, 10
    eng, _ = both(name, B, "f64", n_actor=Nh)
    x = rand_states(rng, name, B)
    cand = rand_actions(rng, name, (B, K, Nh))
    eng.set_state(x)
    J = eng.actor_cost(eng.to_device(cand))
    first = np.argmin(J, axis=1)
    twin = np.empty(B, dtype=np.int64)
    for b in range(B):
        m = int(first[b])
        # another tile where K has one, another lane always; even envs: behind the minimum, odd envs: in front of it
        p = (m + 64 + 7) % K if b % 2 == 0 else (m - 64 - 7) % K
        if b >= B - 4:  # ... and the two ends of the env's rows: lane 0 of the first tile, the last row of the (ragged) last one
            p = 0 if b % 2 else K - 1
        if p == m:
            p = (m + 1) % K
        cand[b, p] = cand[b, m]
        twin[b] = p
    cand[B - 5, :, 0, 0] = np.inf  # every cost +inf: index 0 (a lane without a row holds +inf as well and must not win)
    dc = eng.to_device(cand)
    J2 = eng.actor_cost(dc)
    tied = np.arange(B) != B - 5
    assert np.array_equal(J2[np.arange(B), twin][tied], J2[np.arange(B), first][tied])
    Jc = np.where(np.isnan(J2), np.inf, J2)
    want = np.argmin(Jc, axis=1).astype(np.int32)
    assert np.array_equal(want[tied], np.minimum(first, twin)[tied])
    act, bj, bi = eng.actor_argmin(dc)
    assert_kernel(eng, "k_actor_dma")
    # the robots: the zero-weight instance, whose argmin is the register one; the tank: the plain instance's butterfly
    assert eng.last_launch_zero_w() == {"3wrobot": 0x78, "3wrobotNI": 0x18, "2tank": 0}[name]
    np.testing.assert_array_equal(bi, want)
    np.testing.assert_array_equal(bj, Jc[np.arange(B), want])
    assert bi[B - 5] == 0 and bj[B - 5] == np.inf
    ok = np.isfinite(bj)
    np.testing.assert_array_equal(act[ok], cand[np.arange(B), want, 0, :][ok])
    eng.close()
