// rcg_critic_fit_gen.hpp - k_critic_fit_gen: the critic fit for ANY number of TD rows (Ncritic - 1 > 8).
//
// The reference only clips Ncritic to buffer_size - 1 (rcognita/controllers.py:1015) and its class default is buffer_size = 20
// (:828), so `--Ncritic 12 --buffer_size 20` is a legal run: a TD stack of 11 rows, up to 19 with the default buffer.  The
// exact-m kernels (rcg_critic_fit.hpp: m <= 3 and m <= 8, everything in registers) cannot hold such a stack; this one runs the
// SAME active-set walk - rcg_critic_fit.hpp's critic_walk, one lane per env, sums in the same order - on FitScratchStack: the
// m x dc stack, the m x m factor and the five m-vectors of an env in a per-handle scratch tensor in HBM (allocated on first
// use: (m dc + m^2 + 5 m) doubles per env, env index innermost, so every access of a wave is one contiguous 512-byte segment
// served by L2), the row count a run-time value, and only the per-variable state (w, z, two accumulators) in registers.
// lane == env.  Speed is secondary here (the walk rebuilds the m x m Gram matrix of the free columns every
// iteration: m (m + 1) / 2 x dc fused multiply-adds on operands that come from L2); every preset and every BASELINE config has
// Ncritic - 1 <= 3 and stays on the register kernels.
#pragma once
#include "rcg_critic_fit.hpp"

namespace rcg {

// doubles of scratch per env
__host__ __device__ constexpr long fit_gen_scratch_doubles(int m, int dc) { return (long)m * dc + (long)m * m + 5L * m; }

// critic_walk's Stack policy for any number of rows: element k of env `env` at S[k * B + env]; w_init and the box are wave-uniform
// scalar loads.  Its loops over rows are plain loops with r outermost, so a pass reads a row of A once.
template <int DC>
struct FitScratchStack {
  static constexpr int NROWS = 0;  // (run-time row count)
  double* const S;
  const double* const wcfg;
  const long B, env;
  const int m;
  const long oL, oB, oLam, oD, oR, oRes;  // (A at 0)
  double tr = 0.0;                       // row-major trace of A A^T, gathered as the rows arrive

  __device__ __forceinline__ FitScratchStack(double* const S_, const double* const wcfg_, const long B_, const long env_, const int m_)
      : S(S_), wcfg(wcfg_), B(B_), env(env_), m(m_), oL((long)m_ * DC), oB(oL + (long)m_ * m_), oLam(oB + m_), oD(oLam + m_),
        oR(oD + m_), oRes(oR + m_) {}
  __device__ __forceinline__ double& at(const long k) const { return S[k * B + env]; }
  // critic_td_stack's sink
  __device__ __forceinline__ void put_row(const int r, const double (&phi)[DC], const double rho) {
#pragma unroll
    for (int i = 0; i < DC; ++i) {
      at((long)r * DC + i) = phi[i];
      tr = fma_r(phi[i], phi[i], tr);
    }
    at(oB + r) = 0.0 + rho;  // (the register stacks add rho to a zero: -0 becomes +0 there, so here too)
  }
  __device__ __forceinline__ void add_target(const int r, const double v) { at(oB + r) = at(oB + r) + v; }

  __device__ __forceinline__ int rows() const { return m; }
  __device__ __forceinline__ double a(const int r, const int k) const { return at((long)r * DC + k); }
  __device__ __forceinline__ double b(const int r) const { return at(oB + r); }
  __device__ __forceinline__ double& L(const int r, const int q) { return at(oL + (long)r * m + q); }
  __device__ __forceinline__ double& lam(const int r) { return at(oLam + r); }
  __device__ __forceinline__ double& dg(const int r) { return at(oD + r); }
  __device__ __forceinline__ double& rc(const int r) { return at(oR + r); }
  __device__ __forceinline__ double& res(const int r) { return at(oRes + r); }
  __device__ __forceinline__ double w0(const int k) const { return wcfg[k]; }
  __device__ __forceinline__ double lo(const int k) const { return wcfg[40 + k]; }
  __device__ __forceinline__ double hi(const int k) const { return wcfg[80 + k]; }
  // acc_k = init(k), then term(r, k, a(r, k), acc_k) for r = 0 .. m - 1, then use(k, acc_k): row by row
  template <int NACC, typename Init, typename Term, typename Use>
  __device__ __forceinline__ void over_rows(Init init, Term term, Use use) {
    double acc[DC][NACC];
#pragma unroll
    for (int k = 0; k < DC; ++k) init(k, acc[k]);
    for (int r = 0; r < m; ++r) {
#pragma unroll
      for (int k = 0; k < DC; ++k) term(r, k, a(r, k), acc[k]);
    }
#pragma unroll
    for (int k = 0; k < DC; ++k) use(k, acc[k]);
  }
};

template <typename Sys, typename real, int CS>
__global__ __launch_bounds__(64) void k_critic_fit_gen(const FitArgs<real> F, const KParams<double> P, const KParams<real> Pr,
                                                       double* const S) {
  constexpr int DY = sys_dy<Sys>(), DU = Sys::DU, DC = CriticDim<CS, DY, DU>::value;
  constexpr int KEEP = 2;  // rows the push keeps in registers for the TD stack: few, the walk needs the registers
  const long b = F.env_lo + (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= (F.env_hi > 0 ? (long)F.env_hi : P.B)) return;
  const int m = P.n_critic - 1;  // rows of the TD stack (>= 1, checked on the host)
  CriticKept<real, DC, DY, DU, KEEP> K;
  critic_step_push<Sys, real, CS, KEEP>(F, P, Pr, b, true, K);
  if (!F.do_fit) return;
  FitScratchStack<DC> St(S, F.wcfg, P.B, b, m);
  critic_td_stack<Sys, real, CS, KEEP>(F, P, Pr, b, K, St);
  critic_walk<DC, real>(F, P.B, b, FitOneLane(), St, FIT_MU_REL * (St.tr / (double)m));
}

}  // namespace rcg
