// rcg_critic_fit_ml.hpp - k_critic_fit_ml: the critic update with FOUR LANES PER ENV
// (replacement of CtrlOptPred._critic_optimizer, rcognita/controllers.py:1248-1271; same build-defined fit as
// rcg_critic_fit.hpp / oracle/rcg_oracle.py::critic_fit_single: the unique minimiser of the w_init-regularised bounded
// least squares, by the primal active-set walk).  The walk is rcg_critic_fit.hpp's critic_walk on the register stack; this file
// holds its four-lane policy, FitFourLanes, and the kernel.
//
// Why: k_critic_fit (lane == env) lasts as long as the longest walk of the batch, one iteration being ~680 mostly dependent
// VALU instructions of a lone wave.  Here the VARIABLES of an env are dealt over the four lanes of a quad
// (variable i lives in lane i mod 4, slot i div 4), so the per-variable work of an iteration - restricted columns, z, the
// ratio test, the step, the multipliers - is a quarter as long per lane, the m x m system is formed by quad sums
// ((p0 + p1) + (p2 + p3) through two DPP quad permutes: every lane of the quad ends with the same bits) and solved
// redundantly, and the decisions (first bound hit, most wrong-signed multiplier) are quad reductions with the walk's
// tie rules (smallest ratio / largest score, then lowest index).  A wave holds 16 envs instead of 64: four times the
// waves, each a quarter as long and with the maximum walk of 16 envs instead of 64.
// The TD stack (A, b) is built exactly as for k_critic_fit - all four lanes run critic_step_push and critic_td_stack, lane 0 of
// the quad stores - so the problem instance is the same bits; what differs is the ASSOCIATION of the sums over variables: the
// weights agree with k_critic_fit and with the float64 oracle to the tolerances of the parity tests on the same inputs (the whole
// critic test set passes with this form forced for every structure: 324 tests, --rcg-lib + RCG_FIT_LANES=4), not bit for
// bit; on rank-deficient stacks a last-bit difference can end the walk on another vertex of equal cost, which 40 free-running
// ticks amplify (profiles/r04_fit_four_lanes.txt).
// Where it runs: the structures with kFitLanesMinDc weights or more (rcg_sysops.hpp::launch_fit3).  Measured at 20 weights and
// beyond: there the one-lane walk, up to 3 dc + 10 iterations of ~2000 instructions for the slowest lane of a wave, takes 2.3 ms
// for 32 768 envs and this form 0.41 ms; with few weights the redundant solve and the quad reductions make it the slower form
// (configs[2], 6 weights: 65 -> 88 us).
// Rows: m <= 3 (the exact-m instance; every preset).
#pragma once
#include "rcg_critic_fit.hpp"

namespace rcg {

constexpr int FIT_L = 4;  // lanes per env

__device__ __forceinline__ double quad_xchg(double x, int ctrl) {  // ctrl 0xB1: lanes 0<->1, 2<->3; 0x4E: 0<->2, 1<->3
  const unsigned long long b = (unsigned long long)__double_as_longlong(x);
  unsigned lo, hi;
  if (ctrl == 0xB1) {
    lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)b, 0xB1, 0xF, 0xF, false);
    hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(b >> 32), 0xB1, 0xF, 0xF, false);
  } else {
    lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)b, 0x4E, 0xF, 0xF, false);
    hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(b >> 32), 0x4E, 0xF, 0xF, false);
  }
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
__device__ __forceinline__ int quad_xchg(int x, int ctrl) {
  return ctrl == 0xB1 ? __builtin_amdgcn_update_dpp(0, x, 0xB1, 0xF, 0xF, false)
                      : __builtin_amdgcn_update_dpp(0, x, 0x4E, 0xF, 0xF, false);
}
// (p0 + p1) + (p2 + p3), the same bits in the four lanes (addition commutes exactly)
__device__ __forceinline__ double quad_sum(double x) {
  x += quad_xchg(x, 0xB1);
  return x + quad_xchg(x, 0x4E);
}

// critic_walk's Lanes policy for a quad: this is lane s of the env's four
struct FitFourLanes {
  static constexpr int LANES = FIT_L;
  const int s;
  typedef unsigned mask_t;  // (up to 9 slots)
  __device__ __forceinline__ explicit FitFourLanes(const int lane) : s(lane) {}
  // a sum over the variables: this lane's partial from 0, the quad sum, then the first term
  __device__ __forceinline__ static double start(const double) { return 0.0; }
  __device__ __forceinline__ static double end(const double partial, const double x) { return x + quad_sum(partial); }
  __device__ __forceinline__ static double sum(const double partial) { return quad_sum(partial); }
  // the smallest ratio nb / db of the quad, by cross multiplication; ties -> lowest variable index: what the sequential scan
  // of the one-lane walk picks
  __device__ __forceinline__ static void first(double& nb, double& db, int& jmin) {
#pragma unroll
    for (int st = 0; st < 2; ++st) {
      const int ctrl = st == 0 ? 0xB1 : 0x4E;
      const double on = quad_xchg(nb, ctrl), od = quad_xchg(db, ctrl);
      const int oj = quad_xchg(jmin, ctrl);
      const double l = on * db, r = nb * od;  // other < mine  <=>  on / od < nb / db
      // total order: whenever neither ratio is strictly smaller - equal, or a NaN product from non-finite
      // buffers (0 * inf) - the lower index wins in BOTH partners, so the quad always agrees on (nb, db, jmin)
      const bool take = oj >= 0 && (jmin < 0 || l < r || (!(r < l) && oj < jmin));
      nb = take ? on : nb;
      db = take ? od : db;
      jmin = take ? oj : jmin;
    }
  }
  // the largest score of the quad, ties -> lowest index (the sequential scan keeps the first maximum)
  __device__ __forceinline__ static void largest(double& best_score, int& best) {
#pragma unroll
    for (int st = 0; st < 2; ++st) {
      const int ctrl = st == 0 ? 0xB1 : 0x4E;
      const double os = quad_xchg(best_score, ctrl);
      const int ob = quad_xchg(best, ctrl);
      const bool take = ob >= 0 && (best < 0 || os > best_score || (!(best_score > os) && ob < best));  // total, as above
      best_score = take ? os : best_score;
      best = take ? ob : best;
    }
  }
};

// one quad per env: blocks of 64 threads = 16 envs
template <typename Sys, typename real, int CS, int MAXM>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2))) void k_critic_fit_ml(const FitArgs<real> F, const KParams<double> P, const KParams<real> Pr) {
  const long b = F.env_lo + (long)blockIdx.x * (blockDim.x / FIT_L) + (threadIdx.x / FIT_L);
  if (b >= (F.env_hi > 0 ? (long)F.env_hi : P.B)) return;  // (whole quads leave together: the DPP exchanges of the walk stay inside a quad)
  critic_update_env<Sys, real, CS, MAXM>(F, P, Pr, b, FitFourLanes((int)(threadIdx.x & (FIT_L - 1))));
}

}  // namespace rcg
