// rcg_critic_fit.hpp - k_critic_fit: replacement of CtrlOptPred._critic_optimizer
// (rcognita/controllers.py:1248-1271) for a batch of envs, lane == env.
//
// Problem per env (controllers.py:1216-1245 written as a linear least squares, see
// oracle/rcg_oracle.py::critic_td_system):   Jc(w) = 1/2 |A w - b|^2,  Wmin <= w <= Wmax,
//   row r (= the reference's term k = r + 1):  A[r] = phi(y_r, u_r),
//   b[r] = gamma * w_prev . phi(y_{r+1}, u_{r+1}) + rho(y_r, u_r),   r = 0 .. Ncritic - 2,
// on the OLDEST Ncritic buffer rows.  The reference runs SLSQP from w_init = ones; its iterates are
// path dependent, so the build defines the fit as the unique minimiser of
//   1/2 |A w - b|^2 + mu/2 |w - w_init|^2   in the box,  mu = 1e-8 * trace(A A^T) / m,
// computed by a primal active-set method (bounded-variable least squares): each iteration solves the
// problem on the free variables exactly through the m x m system (A_F A_F^T + mu I) lam = rhs
// (root-free Cholesky L D L^T), then either moves towards that point until the first bound is hit and fixes that
// variable, or accepts it and releases the bound variable with the most wrong-signed multiplier
// (none: optimal).  Feasible and monotone, so the result is never worse than w_init.  This mirrors
// oracle/rcg_oracle.py::critic_fit_single statement by statement; all arithmetic is float64 whatever
// the handle's dtype (the systems are tiny - m <= 8, dc <= 35 - and badly scaled).  The active set is
// held in lane-private masks and every loop over variables is unrolled with a predicate, so no
// array is indexed dynamically.
//
// The walk is stated ONCE, critic_walk below, for every fit kernel - k_critic_fit<.., 3> and <.., 8> here, k_critic_fit_ml
// (rcg_critic_fit_ml.hpp), k_critic_fit_gen (rcg_critic_fit_gen.hpp) and the critic phase of k_ticks_mem (rcg_ticks.hpp) -
// under two policies: Lanes (one lane per env or four) and Stack (registers with a compile-time row count, or the HBM scratch
// with a run-time one); see the comment in front of FitOneLane.
//
// Cost (profiles/r02_*; tools/critic_fit_probe.py): 10 us per launch at B = 131072 while the oldest buffer rows are still
// zeros, 56-62 us in the steady state of an RQL closed loop (quadratic critic, m = 3): ~7000 VALU instructions per wave of
// which 2100 are f64 fma, 40 % of the issue slots - a wave runs as many active-set iterations as its slowest lane (11-13
// where the mean over envs is 2.2).  Tried in round 2: root-free L D L^T instead of L L^T (kept: 3 reciprocals instead
// of 12 divides / square roots per solve, 3 % faster); warm-starting the walk from the previous fit (not adopted: on
// rank-deficient stacks the end point depends on the start); running the NEXT tick's fit on a second stream while the
// actor kernel runs - legal because the TD stack reads only the oldest rows - which hid the fit but slowed the actor
// kernel by almost as much (configs[2] RQL tick 0.380 -> 0.371 ms generated, 0.549 -> 0.547 ms streamed): dropped.
#pragma once
#include "rcg_kernels.hpp"

namespace rcg {

constexpr double FIT_MU_REL = 1e-8;
constexpr double FIT_KKT_TOL = 1e-10;
__host__ __device__ constexpr int fit_max_iters(int dc) { return 3 * dc + 10; }

template <int CS, int DS, int DU>
struct CriticDim {
  static constexpr int n = DS + DU;
  static constexpr int value = CS == RCG_CRITIC_QUAD_LIN    ? n * (n + 1) / 2 + n
                               : CS == RCG_CRITIC_QUADRATIC ? n * (n + 1) / 2
                               : CS == RCG_CRITIC_QUAD_NOMIX ? n
                                                             : DS + DS * DU + DU;
};

// regressor of _critic (controllers.py:1204-1212) with compile-time structure
template <int CS, int DS, int DU>
__device__ __forceinline__ void critic_phi(const double* chi, const double* y, const double* u, double* phi) {
  constexpr int N = DS + DU;
  int idx = 0;
  if (CS == RCG_CRITIC_QUAD_LIN || CS == RCG_CRITIC_QUADRATIC) {
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
      for (int j = i; j < N; ++j) phi[idx++] = chi[i] * chi[j];
    if (CS == RCG_CRITIC_QUAD_LIN) {
#pragma unroll
      for (int i = 0; i < N; ++i) phi[idx++] = chi[i];
    }
  } else if (CS == RCG_CRITIC_QUAD_NOMIX) {
#pragma unroll
    for (int i = 0; i < N; ++i) phi[i] = chi[i] * chi[i];
  } else {
#pragma unroll
    for (int i = 0; i < DS; ++i) phi[idx++] = y[i] * y[i];
#pragma unroll
    for (int i = 0; i < DS; ++i)
#pragma unroll
      for (int c = 0; c < DU; ++c) phi[idx++] = y[i] * u[c];
#pragma unroll
    for (int c = 0; c < DU; ++c) phi[idx++] = u[c] * u[c];
  }
}

template <typename real>
struct FitArgs {
  real* w_critic;         // [dc][B] out
  real* w_prev;           // [dc][B] in (TD target weights), out (:= fitted w)
  real* obs_buf;          // [buffer_size][dy][B]
  real* act_buf;          // [buffer_size][du][B]
  const double* wcfg;     // [3][40]: w_init, w_min, w_max
  // Everything an RQL / SQL tick does between two decisions is lane == env work on the same few numbers, so
  // rcg_control_tick issues it as ONE launch (three dependent launches cost ~7 us of dispatch gap each at this size,
  // plus the former push kernel's own 11 us): do_sim: Simulator.sim_step (env_substeps, the code k_sim runs); do_push:
  // push_vec of (action_curr, obs) (utilities.py:78-79); do_fit: the fit.  Same arithmetic as the separate launches.
  int do_sim, do_push, do_fit;
  SimArgs<real> sim;      // do_sim
  const real* state;      // [ds][B] do_push: the observation to push (= sim.state)
  const real* action;     // [du][B] do_push: the held action (action_curr)
  int env_lo, env_hi;     // the envs [env_lo, env_hi) this launch serves (env_hi == 0: the whole batch)
  // k_ticks_mem only (0 elsewhere): the two buffers as RINGS while the launch runs - ring = 1 + the physical row this push overwrites
  // (the oldest); logical row r after the push is physical row (ring + r) mod buffer_size.  The physical shift of a push is two
  // dependent load -> store passes over the rows (buffer_size 10: ~3 us of a 20 us tick on a wave that runs alone on its SIMD);
  // the launch rotates the rows back into place after its last tick (critic_ring_unrotate), so every launch starts and ends canonical.
  int ring;
};

// A loop over TD rows (or the entries of the m x m factor), i = lo .. hi - 1.  N > 0: the stack is in registers, N bounds hi at
// compile time and the loop is unrolled in full as N predicated steps - no register array may be indexed at run time, and a
// bound that depends on an enclosing loop's index must not keep this one from unrolling; N == 0: a plain loop.
#define RCG_FIT_INL __attribute__((always_inline))
template <int N, typename Fn>
__device__ __forceinline__ void fit_for(const int lo, const int hi, Fn f) {
  if constexpr (N > 0) {
#pragma unroll
    for (int i = 0; i < N; ++i)
      if (i >= lo && i < hi) f(i);
  } else {
    for (int i = lo; i < hi; ++i) f(i);
  }
}
template <int N, typename Fn>
__device__ __forceinline__ void fit_for_down(const int hi, const int lo, Fn f) {  // i = hi - 1 .. lo
  if constexpr (N > 0) {
#pragma unroll
    for (int i = N - 1; i >= 0; --i)
      if (i >= lo && i < hi) f(i);
  } else {
    for (int i = hi - 1; i >= lo; --i) f(i);
  }
}

// The part of an env's critic update that precedes the solver, in its two jobs: critic_step_push - [env step] -> [push] - and
// critic_td_stack - the TD stack (A, b) from the oldest buffer rows.

// rows of the pushed buffers that stay in registers for the TD stack (logical rows 0 .. KEEP - 1 once the push is done)
__host__ __device__ constexpr int fit_keep_rows(int maxm) { return maxm + 1 <= 4 ? maxm + 1 : 4; }

// what critic_step_push leaves for critic_td_stack: the TD target weights and the kept rows
template <typename real, int DC, int DY, int DU, int KEEP>
struct CriticKept {
  real wpr[DC];
  real ko[KEEP][DY], ka[KEEP][DU];
};

// physical row of the row that is logical row r once this call's push is done (FitArgs::ring)
template <typename real>
__device__ __forceinline__ int critic_phys_row(const FitArgs<real>& F, const KParams<real>& Pr, const int r) {
  if (!F.ring) return r;
  const int p = F.ring + r;
  return p >= Pr.buffer_size ? p - Pr.buffer_size : p;
}

// [env step] -> [push].  `store`: this lane writes the env's state / buffers back (false for the lanes that only help with the
// env's solve, k_critic_fit_ml).
template <typename Sys, typename real, int CS, int KEEP>
__device__ __forceinline__ void critic_step_push(const FitArgs<real>& F, const KParams<double>& P, const KParams<real>& Pr,
                                                 const long b, const bool store,
                                                 CriticKept<real, CriticDim<CS, sys_dy<Sys>(), Sys::DU>::value, sys_dy<Sys>(), Sys::DU, KEEP>& K) {
  constexpr int DS = Sys::DS, DY = sys_dy<Sys>(), DU = Sys::DU, DC = CriticDim<CS, DY, DU>::value;
  constexpr bool OUT = HasOut<Sys>::value;  // the buffers hold observations y = out(x): [buffer_size][DY][B]
  const long B = P.B;
  const int bs = Pr.buffer_size;

  // ---- every load the prologue needs is requested here, before any arithmetic: the env step, the shift of the two
  // buffers and the TD stack used to be three dependent round trips to memory (and the row-by-row shift one per row:
  // the compiler cannot prove that the store to row r leaves row r + 2 alone) ----------------------------------------
  real (&wpr)[DC] = K.wpr;
  if (F.do_fit) {
#pragma unroll
    for (int i = 0; i < DC; ++i) wpr[i] = F.w_prev[(long)i * B + b];
  }
  // do_push: old rows 1 .. KEEP (= new rows 0 .. KEEP - 1); else rows 0 .. KEEP - 1
  real (&ko)[KEEP][DY] = K.ko;
  real (&ka)[KEEP][DU] = K.ka;
  const int koff = F.do_push ? 1 : 0;
  const int ring = F.ring;  // > 0: ring mode (with do_push)
#pragma unroll
  for (int k = 0; k < KEEP; ++k)
    if (k + koff < bs) {
      const int pr = ring ? critic_phys_row(F, Pr, k) : k + koff;
#pragma unroll
      for (int c = 0; c < DY; ++c) ko[k][c] = F.obs_buf[((long)pr * DY + c) * B + b];
#pragma unroll
      for (int c = 0; c < DU; ++c) ka[k][c] = F.act_buf[((long)pr * DU + c) * B + b];
    }

  if (F.do_sim || F.do_push) {
    real xs[DS], xp[DS], ua[DU];
#pragma unroll
    for (int c = 0; c < DS; ++c) xp[c] = xs[c] = F.state[(long)c * B + b];
#pragma unroll
    for (int c = 0; c < DU; ++c) ua[c] = F.action[(long)c * B + b];
    if (F.do_sim) {  // k_sim
      uint32_t st = F.sim.status[b];
      if (!(st & 1u)) {
        const auto pre = load_pre<Sys, real>(Pr, F.sim.pars_env, b);
        real accum = Pr.accum_every_substep ? F.sim.accum[b] : (real)0;
        const bool tgt = Pr.has_target != 0;
        const bool ok = tgt ? env_substeps<Sys, real, true>(Pr, pre, F.sim.n_sub, xs, xp, ua, st, accum)
                            : env_substeps<Sys, real, false>(Pr, pre, F.sim.n_sub, xs, xp, ua, st, accum);
        if (!ok) {
          if (store) F.sim.status[b] = st;  // became non-finite: frozen at its last finite state
        } else {
#pragma unroll
          for (int c = 0; c < DS; ++c) {
            if (store) F.sim.state[(long)c * B + b] = xs[c];
            if (store) F.sim.state_prev[(long)c * B + b] = xp[c];
          }
          if (store) if (Pr.accum_every_substep) F.sim.accum[b] = accum;
        }
      }
    }
    // what is pushed is the observation of the (new) state: y = out(x) as k_out and upd_accum_obj form it (identity without `out`)
    real yb[OUT ? DY : 1];
    const real* ys = xs;
    if constexpr (OUT) {
      const auto pre_o = load_pre<Sys, real>(Pr, F.sim.pars_env, b);
      sys_out<Sys, real, false>(pre_o, xs, yb);
      ys = yb;
    }
    if (F.do_push && ring) {  // ring mode: the new row takes the oldest row's place, nothing else moves
#pragma unroll
      for (int c = 0; c < DY; ++c) if (store) F.obs_buf[((long)(ring - 1) * DY + c) * B + b] = ys[c];
#pragma unroll
      for (int c = 0; c < DU; ++c) if (store) F.act_buf[((long)(ring - 1) * DU + c) * B + b] = ua[c];
#pragma unroll
      for (int k = 0; k < KEEP; ++k) {
        const bool newest = k == bs - 1;
#pragma unroll
        for (int c = 0; c < DY; ++c) ko[k][c] = newest ? ys[c] : ko[k][c];
#pragma unroll
        for (int c = 0; c < DU; ++c) ka[k][c] = newest ? ua[c] : ka[k][c];
      }
    } else if (F.do_push) {  // push_vec on both buffers: drop row 0, append (obs, action_curr) at the bottom (utilities.py:78-79)
#pragma unroll
      for (int k = 0; k < KEEP; ++k)
        if (k + 1 < bs) {
#pragma unroll
          for (int c = 0; c < DY; ++c) if (store) F.obs_buf[((long)k * DY + c) * B + b] = ko[k][c];
#pragma unroll
          for (int c = 0; c < DU; ++c) if (store) F.act_buf[((long)k * DU + c) * B + b] = ka[k][c];
        }
      // the rest of the shift four rows at a time, all loads of a pass before its stores
      constexpr int CH = 4;
      for (int r0 = KEEP; r0 < bs - 1; r0 += CH) {
        real ro[CH][DY], ra[CH][DU];
#pragma unroll
        for (int k = 0; k < CH; ++k)
          if (r0 + k < bs - 1) {
#pragma unroll
            for (int c = 0; c < DY; ++c) ro[k][c] = F.obs_buf[((long)(r0 + k + 1) * DY + c) * B + b];
#pragma unroll
            for (int c = 0; c < DU; ++c) ra[k][c] = F.act_buf[((long)(r0 + k + 1) * DU + c) * B + b];
          }
#pragma unroll
        for (int k = 0; k < CH; ++k)
          if (r0 + k < bs - 1) {
#pragma unroll
            for (int c = 0; c < DY; ++c) if (store) F.obs_buf[((long)(r0 + k) * DY + c) * B + b] = ro[k][c];
#pragma unroll
            for (int c = 0; c < DU; ++c) if (store) F.act_buf[((long)(r0 + k) * DU + c) * B + b] = ra[k][c];
          }
      }
#pragma unroll
      for (int c = 0; c < DY; ++c) if (store) F.obs_buf[((long)(bs - 1) * DY + c) * B + b] = ys[c];
#pragma unroll
      for (int c = 0; c < DU; ++c) if (store) F.act_buf[((long)(bs - 1) * DU + c) * B + b] = ua[c];
#pragma unroll
      for (int k = 0; k < KEEP; ++k) {  // (buffer_size <= KEEP: the row just pushed is one of the kept rows; a select, so that the index stays static)
        const bool newest = k == bs - 1;
#pragma unroll
        for (int c = 0; c < DY; ++c) ko[k][c] = newest ? ys[c] : ko[k][c];
#pragma unroll
        for (int c = 0; c < DU; ++c) ka[k][c] = newest ? ua[c] : ka[k][c];
      }
    }
  }
}

// The TD stack from buffer rows 0 .. m (the oldest rows, controllers.py:1231-1234): rows below KEEP come from the kept
// registers, the others from the buffers (written by this lane's push: same-address order, served by L2).  The stack receives
// them: S.put_row(r, phi, rho) stores the regressor of TD row r < m and sets b[r] = rho(y_r, u_r); S.add_target(r, v) adds
// gamma * w_prev . phi(row r + 1) to b[r].  (The register stacks bound r by their compile-time row count, unrolled.)
template <typename Sys, typename real, int CS, int KEEP, typename Stack>
__device__ __forceinline__ void critic_td_stack(const FitArgs<real>& F, const KParams<double>& P, const KParams<real>& Pr,
                                                const long b,
                                                const CriticKept<real, CriticDim<CS, sys_dy<Sys>(), Sys::DU>::value, sys_dy<Sys>(), Sys::DU, KEEP>& K,
                                                Stack& S) {
  constexpr int DY = sys_dy<Sys>(), DU = Sys::DU, NCHI = DY + DU, DC = CriticDim<CS, DY, DU>::value;
  const long B = P.B;
  const int m = P.n_critic - 1;  // rows of the TD stack, >= 1 (and <= the register stacks' row count: checked on the host)
  auto td_row = [&](const int r, const double (&y)[DY], const double (&u)[DU]) RCG_FIT_INL {
    double chi[NCHI], phi[DC];
    if (P.has_target)
      make_chi<DY, DU, true, double>(P, y, u, chi);
    else
      make_chi<DY, DU, false, double>(P, y, u, chi);
    critic_phi<CS, DY, DU>(chi, y, u, phi);
    if (r > 0) {  // gamma * w_prev . phi(row r) belongs to TD row r - 1
      double q = 0.0;
#pragma unroll
      for (int i = 0; i < DC; ++i) q = fma_r((double)K.wpr[i], phi[i], q);
      S.add_target(r - 1, P.gamma * q);
    }
    if (r < m) S.put_row(r, phi, stage_any<NCHI, double>(P, chi));
  };
#pragma unroll
  for (int r = 0; r < KEEP; ++r)
    if (r <= m) {
      double y[DY], u[DU];
#pragma unroll
      for (int c = 0; c < DY; ++c) y[c] = (double)K.ko[r][c];
#pragma unroll
      for (int c = 0; c < DU; ++c) u[c] = (double)K.ka[r][c];
      td_row(r, y, u);
    }
  fit_for<(Stack::NROWS > 0 ? Stack::NROWS + 1 : 0)>(KEEP, S.rows() + 1, [&](const int r) RCG_FIT_INL {
    if (r <= m) {
      double y[DY], u[DU];
      const int pr = critic_phys_row(F, Pr, r);
#pragma unroll
      for (int c = 0; c < DY; ++c) y[c] = (double)F.obs_buf[((long)pr * DY + c) * B + b];
#pragma unroll
      for (int c = 0; c < DU; ++c) u[c] = (double)F.act_buf[((long)pr * DU + c) * B + b];
      td_row(r, y, u);
    }
  });
}

// After `pushes` ring-mode pushes physical row p of env b holds logical row (p - pushes) mod buffer_size: rotate both buffers left by
// pushes mod buffer_size, in place (cycle by cycle; all components of a row travel together), by the lane that stored them.
template <typename Sys, typename real>
__device__ __forceinline__ void critic_ring_unrotate(const FitArgs<real>& F, const KParams<real>& Pr, const long b, const int pushes) {
  constexpr int DY = sys_dy<Sys>(), DU = Sys::DU;
  const long B = Pr.B;
  const int bs = Pr.buffer_size, sh = pushes % bs;
  if (sh == 0) return;
  int g = bs, r = sh;  // gcd(bs, sh) = the number of cycles
  while (r) {
    const int q = g % r;
    g = r;
    r = q;
  }
  for (int s = 0; s < g; ++s) {
    real to[DY], ta[DU];
#pragma unroll
    for (int c = 0; c < DY; ++c) to[c] = F.obs_buf[((long)s * DY + c) * B + b];
#pragma unroll
    for (int c = 0; c < DU; ++c) ta[c] = F.act_buf[((long)s * DU + c) * B + b];
    int j = s;
    for (;;) {
      int nx = j + sh;
      if (nx >= bs) nx -= bs;
      if (nx == s) break;
      real vo[DY], va[DU];
#pragma unroll
      for (int c = 0; c < DY; ++c) vo[c] = F.obs_buf[((long)nx * DY + c) * B + b];
#pragma unroll
      for (int c = 0; c < DU; ++c) va[c] = F.act_buf[((long)nx * DU + c) * B + b];
#pragma unroll
      for (int c = 0; c < DY; ++c) F.obs_buf[((long)j * DY + c) * B + b] = vo[c];
#pragma unroll
      for (int c = 0; c < DU; ++c) F.act_buf[((long)j * DU + c) * B + b] = va[c];
      j = nx;
    }
#pragma unroll
    for (int c = 0; c < DY; ++c) F.obs_buf[((long)j * DY + c) * B + b] = to[c];
#pragma unroll
    for (int c = 0; c < DU; ++c) F.act_buf[((long)j * DU + c) * B + b] = ta[c];
  }
}

// ---------------------------------------------------------------------------------------------
// The walk: ONE statement of it, critic_walk, behind every fit kernel; two small policies say what differs.
//
// Lanes - how many lanes share an env.  Slot k of lane s holds variable k * LANES + s, NV = ceil(dc / LANES) slots per lane (a slot
//   beyond dc: a variable fixed at 0 with a zero column - it never moves).  A sum over the variables is end(partial, x), the
//   partial begun at start(x); sum(partial) is the same without a first term.  The two decisions of an iteration - the first
//   bound hit, the most wrong-signed multiplier - end in first() / largest() over the env's lanes.  A mask bit is changed by
//   the lane that owns the slot.  FitOneLane below; FitFourLanes in rcg_critic_fit_ml.hpp.
// Stack - where A, b, the factor and the m-vectors live, and where w_init and the box come from: a(r, k), b(r), L(r, q),
//   lam(r), dg(r), rc(r), res(r), w0(k), lo(k), hi(k); rows() and NROWS say how its row loops run (fit_for); over_rows() runs
//   the per-variable sums over the rows - r ascending for every variable, the loop order the stack's own.  FitRegStack below
//   (compile-time row count, rows >= m exact zeros, everything unrolled); FitScratchStack in rcg_critic_fit_gen.hpp.
// The association of every sum is each form's own and is part of what it computes: a form keeps its bits.
// ---------------------------------------------------------------------------------------------
struct FitOneLane {
  static constexpr int LANES = 1;
  static constexpr int s = 0;
  typedef unsigned long long mask_t;  // (up to 35 variables)
  __device__ __forceinline__ static double start(const double x) { return x; }
  __device__ __forceinline__ static double end(const double partial, const double) { return partial; }
  __device__ __forceinline__ static double sum(const double partial) { return partial; }
  __device__ __forceinline__ static void first(double&, double&, int&) {}
  __device__ __forceinline__ static void largest(double&, int&) {}
};

// The stack of the exact-m kernels, in registers: this lane's NV columns of A [MAXM][dc] (rows >= m zero), b, the factor, and
// its slots of w_init and the box.
template <int MAXM, int DC, typename Lanes>
struct FitRegStack {
  static constexpr int NROWS = MAXM;  // (compile-time row count)
  static constexpr int NV = (DC + Lanes::LANES - 1) / Lanes::LANES;
  const Lanes Ln;
  // the arrays are the caller's, one object each (critic_update_env): the compiler turns each into registers as soon as ITS
  // loops are unrolled; as members of one object they would all wait for the deepest nest of the solve
  double (&A_)[MAXM][NV], (&b_)[MAXM], (&w0_)[NV], (&lo_)[NV], (&hi_)[NV];
  double (&L_)[MAXM][MAXM], (&lam_)[MAXM], (&dg_)[MAXM], (&rc_)[MAXM], (&res_)[MAXM];

  __device__ __forceinline__ FitRegStack(const Lanes ln, double (&A)[MAXM][NV], double (&b)[MAXM], double (&w0)[NV], double (&lo)[NV],
                                         double (&hi)[NV], double (&L)[MAXM][MAXM], double (&lam)[MAXM], double (&dg)[MAXM],
                                         double (&rc)[MAXM], double (&res)[MAXM])
      : Ln(ln), A_(A), b_(b), w0_(w0), lo_(lo), hi_(hi), L_(L), lam_(lam), dg_(dg), rc_(rc), res_(res) {
#pragma unroll
    for (int r = 0; r < MAXM; ++r) {
      b_[r] = 0.0;
#pragma unroll
      for (int k = 0; k < NV; ++k) A_[r][k] = 0.0;
    }
  }
  // w_init and the box: this lane's slots (an empty slot: zeros)
  __device__ __forceinline__ void load_box(const double* wcfg) {
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const bool mine = k * Lanes::LANES + Ln.s < DC;
      const int i = mine ? k * Lanes::LANES + Ln.s : 0;
      const double v0 = wcfg[i], vl = wcfg[40 + i], vh = wcfg[80 + i];
      w0_[k] = mine ? v0 : 0.0;
      lo_[k] = mine ? vl : 0.0;
      hi_[k] = mine ? vh : 0.0;
    }
  }
  // critic_td_stack's sink (r runs to MAXM in the unrolled loop: the bound keeps the indices static)
  __device__ __forceinline__ void put_row(const int r, const double (&phi)[DC], const double rho) {
    if (r < MAXM) {
#pragma unroll
      for (int k = 0; k < NV; ++k) {
        double v = 0.0;
#pragma unroll
        for (int t = 0; t < Lanes::LANES; ++t)
          if (k * Lanes::LANES + t < DC) v = Ln.s == t ? phi[k * Lanes::LANES + t] : v;
        A_[r][k] = v;
      }
      b_[r] += rho;
    }
  }
  __device__ __forceinline__ void add_target(const int r, const double v) { b_[r < MAXM ? r : 0] += v; }

  __device__ __forceinline__ static constexpr int rows() { return MAXM; }
  __device__ __forceinline__ double a(const int r, const int k) const { return A_[r][k]; }
  __device__ __forceinline__ double b(const int r) const { return b_[r]; }
  __device__ __forceinline__ double& L(const int r, const int q) { return L_[r][q]; }
  __device__ __forceinline__ double& lam(const int r) { return lam_[r]; }
  __device__ __forceinline__ double& dg(const int r) { return dg_[r]; }
  __device__ __forceinline__ double& rc(const int r) { return rc_[r]; }
  __device__ __forceinline__ double& res(const int r) { return res_[r]; }
  __device__ __forceinline__ double w0(const int k) const { return w0_[k]; }
  __device__ __forceinline__ double lo(const int k) const { return lo_[k]; }
  __device__ __forceinline__ double hi(const int k) const { return hi_[k]; }
  // acc_k = init(k), then term(r, k, a(r, k), acc_k) for r = 0 .. rows() - 1, then use(k, acc_k): variable by variable
  template <int NACC, typename Init, typename Term, typename Use>
  __device__ __forceinline__ void over_rows(Init init, Term term, Use use) {
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      double acc[NACC];
      init(k, acc);
#pragma unroll
      for (int r = 0; r < MAXM; ++r) term(r, k, A_[r][k], acc);
      use(k, acc);
    }
  }
  // trace(A A^T): the row-major trace of this lane's columns, summed over the env's lanes
  __device__ __forceinline__ double trace() const {
    double tr = 0.0;
#pragma unroll
    for (int r = 0; r < MAXM; ++r)
#pragma unroll
      for (int k = 0; k < NV; ++k) tr = fma_r(A_[r][k], A_[r][k], tr);  // rows >= m and empty slots are zero
    return Ln.sum(tr);
  }
};

// The primal active-set walk on the stack S with the regularisation weight mu (floored here), to the safeguard and the store
// of this lane's weights.  Mirrors oracle/rcg_oracle.py::critic_fit_single statement by statement.
//
// Cost model, measured on the one-lane register form at B = 131072 (2tank, quadratic critic, steady state of an RQL loop,
// tools/critic_fit_probe.py with the walk capped at c iterations): 14 us + 3.6 us x c up to c = 8, 66 us uncapped (the longest
// walk of the batch): with B / 64 = 2 waves per SIMD the kernel lasts as long as its slowest wave, and a wave runs as many
// iterations as its slowest lane.  Per-variable work is straight-line code on selects and the ratio test divides once; one
// iteration is ~680 VALU instructions of which 250 are float64 arithmetic and 160 are the halves of 64-bit selects.
// Re-packing unfinished walks into dense waves between levels of iterations (LDS hand-over, blocks of 256 envs) was
// built and measured in round 2: 34 % fewer instructions per wave, bit-identical weights, the same duration - dropped.
template <int DC, typename real, typename Lanes, typename Stack>
__device__ __forceinline__ void critic_walk(const FitArgs<real>& F, const long B, const long b, const Lanes Ln, Stack& S, double mu) {
  constexpr int LN = Lanes::LANES, NV = (DC + LN - 1) / LN;
  constexpr int NR = Stack::NROWS;
  typedef typename Lanes::mask_t mask_t;
  constexpr mask_t one = 1;
  const int m = S.rows();
  if (!(mu > 1e-30)) mu = 1e-30;
  auto var = [&](const int k) RCG_FIT_INL -> int { return k * LN + Ln.s; };  // (var(k) >= DC: an empty slot)
  // (the box is read into locals before any select on it: a read inside an arm of ?: may be compiled as a branch)
  auto start_point = [&](const int k) RCG_FIT_INL -> double {
    const double w0k = S.w0(k), lok = S.lo(k), hik = S.hi(k);
    return w0k < lok ? lok : (w0k > hik ? hik : w0k);
  };

  double w[NV], z[NV];
  mask_t fm = 0, at_hi = 0, blocked = 0;  // free / fixed-at-upper / not-to-release masks over this lane's slots
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const double lok = S.lo(k), hik = S.hi(k);
    w[k] = start_point(k);
    z[k] = w[k];
    if (var(k) < DC) {
      if (w[k] > lok && w[k] < hik)
        fm |= one << k;
      else if (w[k] >= hik)
        at_hi |= one << k;
    }
  }
  int last_freed = -1;  // variable index (the same in all lanes of the env)

  for (int it = 0; it < fit_max_iters(DC); ++it) {
    // rhs = b - A_B w_B - A_F w0_F,  M = A_F A_F^T + mu I  (register rows >= m: M = mu I, rhs = 0 -> lam = 0).  A_F = the free
    // columns, a bound one counting as a zero column: adding an exact zero leaves the sums' bits unchanged
    fit_for<NR>(0, m, [&](const int r) RCG_FIT_INL {
      double sp = Ln.start(S.b(r)), ar[NV];
#pragma unroll
      for (int k = 0; k < NV; ++k) {
        const bool fr = (fm >> k) & one;
        const double a = S.a(r, k);
        sp = fma_r(-a, fr ? S.w0(k) : w[k], sp);
        ar[k] = fr ? a : 0.0;
      }
      S.lam(r) = Ln.end(sp, S.b(r));
      fit_for<NR>(0, r + 1, [&](const int q) RCG_FIT_INL {
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < NV; ++k) {
          const bool fr = (fm >> k) & one;
          const double aq = q == r ? ar[k] : (fr ? S.a(q, k) : 0.0);
          acc = fma_r(ar[k], aq, acc);
        }
        S.L(r, q) = Ln.sum(acc) + (r == q ? mu : 0.0);
      });
    });
    // root-free Cholesky M = L D L^T (unit lower L): one reciprocal per pivot, no sqrt, no other division - the kernel is
    // bound by f64 instruction issue and a divide / square root is 10-20 instructions (round 1: L L^T, 3 m of each).  With
    // several lanes per env every lane holds the same M: the same solve in each
    const double floor_piv = mu * 1e-6;
    fit_for<NR>(0, m, [&](const int j) RCG_FIT_INL {
      double dj = S.L(j, j);
      fit_for<NR>(0, j, [&](const int k) RCG_FIT_INL {
        const double l = S.L(j, k);
        dj -= (l * l) * S.dg(k);
      });
      if (!(dj > floor_piv)) dj = floor_piv;
      S.dg(j) = dj;
      const double rcj = 1.0 / dj;
      S.rc(j) = rcj;
      fit_for<NR>(j + 1, m, [&](const int i) RCG_FIT_INL {
        double sv = S.L(i, j);
        fit_for<NR>(0, j, [&](const int k) RCG_FIT_INL { sv -= (S.L(i, k) * S.L(j, k)) * S.dg(k); });
        S.L(i, j) = sv * rcj;
      });
    });
    fit_for<NR>(0, m, [&](const int i) RCG_FIT_INL {  // forward: L y = rhs
      double sv = S.lam(i);
      fit_for<NR>(0, i, [&](const int k) RCG_FIT_INL { sv -= S.L(i, k) * S.lam(k); });
      S.lam(i) = sv;
    });
    fit_for<NR>(0, m, [&](const int i) RCG_FIT_INL { S.lam(i) = S.lam(i) * S.rc(i); });  // D z = y
    fit_for_down<NR>(m, 0, [&](const int i) RCG_FIT_INL {  // backward: L^T lam = z
      double sv = S.lam(i);
      fit_for<NR>(i + 1, m, [&](const int k) RCG_FIT_INL { sv -= S.L(k, i) * S.lam(k); });
      S.lam(i) = sv;
    });
    // z_F = w0_F + A_F^T lam and the ratio test towards it: the step to the bound z_i crosses is a_i = n_i / d_i with
    // n_i = |bound_i - w_i| <= d_i = |z_i - w_i|; the smallest a_i (lowest variable index on ties) is found by comparing
    // n_i d_best with n_best d_i - no division - over this lane's slots in index order, then over the env's lanes
    // (Lanes::first), and alpha = n_best / d_best is the one division of the iteration
    double nb = 2.0, db = 1.0;
    int jmin = -1;
    S.template over_rows<1>([&](const int, double (&c)[1]) RCG_FIT_INL { c[0] = 0.0; },
                            [&](const int r, const int, const double a, double (&c)[1]) RCG_FIT_INL { c[0] = fma_r(a, S.lam(r), c[0]); },
                            [&](const int k, const double (&c)[1]) RCG_FIT_INL {
                              const bool fr = (fm >> k) & one;
                              const double lok = S.lo(k), hik = S.hi(k);
                              const double zi = S.w0(k) + c[0];
                              z[k] = fr ? zi : z[k];
                              const bool vlo = zi < lok, vhi = zi > hik;
                              const double ni = fabs((vlo ? lok : hik) - w[k]), di = fabs(zi - w[k]);
                              if (fr && (vlo || vhi) && ni * db < nb * di) {
                                nb = ni;
                                db = di;
                                jmin = var(k);
                              }
                            });
    Ln.first(nb, db, jmin);
    if (jmin >= 0) {  // move towards z until the first bound, fix that variable (its owner does)
      double alpha = nb / db;
      if (!(alpha > 0.0)) alpha = 0.0;
#pragma unroll
      for (int k = 0; k < NV; ++k) {
        const bool fr = (fm >> k) & one;
        const double lok = S.lo(k), hik = S.hi(k);
        double v = w[k] + alpha * (z[k] - w[k]);
        v = v < lok ? lok : (v > hik ? hik : v);
        const bool up = z[k] > hik;
        if (var(k) == jmin) {
          v = up ? hik : lok;
          at_hi = up ? (at_hi | (one << k)) : (at_hi & ~(one << k));
        }
        w[k] = fr ? v : w[k];
      }
      const bool owner = (jmin % LN) == Ln.s;
      if (owner) fm &= ~(one << (jmin / LN));
      if (alpha > 0.0)
        blocked = 0;
      else if (jmin == last_freed && owner)
        blocked |= one << (jmin / LN);
      last_freed = -1;
      continue;
    }
    // accept z; the residual, then per variable the multiplier g_i = mu (w_i - w0_i) + sum_r A[r][i] res[r] and its scale;
    // release the bound variable with the largest wrong-signed one (lowest index on ties: Lanes::largest keeps the first)
#pragma unroll
    for (int k = 0; k < NV; ++k) w[k] = ((fm >> k) & one) ? z[k] : w[k];
    fit_for<NR>(0, m, [&](const int r) RCG_FIT_INL {
      double sp = Ln.start(-S.b(r));
#pragma unroll
      for (int k = 0; k < NV; ++k) sp = fma_r(S.a(r, k), w[k], sp);
      S.res(r) = Ln.end(sp, -S.b(r));
    });
    int best = -1;
    double best_score = 0.0;
    S.template over_rows<2>([&](const int k, double (&gs)[2]) RCG_FIT_INL {
                              gs[0] = mu * (w[k] - S.w0(k));
                              gs[1] = fabs(gs[0]);
                            },
                            [&](const int r, const int, const double a, double (&gs)[2]) RCG_FIT_INL {
                              const double t = a * S.res(r);
                              gs[0] += t;
                              gs[1] += fabs(t);
                            },
                            [&](const int k, const double (&gs)[2]) RCG_FIT_INL {
                              const double score = ((at_hi >> k) & one) ? gs[0] : -gs[0];
                              if (var(k) < DC && !(((fm | blocked) >> k) & one) && score > FIT_KKT_TOL * gs[1] && score > best_score) {
                                best = var(k);
                                best_score = score;
                              }
                            });
    Ln.largest(best_score, best);
    if (best < 0) break;
    if ((best % LN) == Ln.s) fm |= one << (best / LN);
    last_freed = best;
  }

  // safeguard (non-finite buffers): keep the start point unless Jc(w) <= Jc(w_init)
  double Pw = 0.0, P0 = 0.0;
  fit_for<NR>(0, m, [&](const int r) RCG_FIT_INL {
    double sp = Ln.start(-S.b(r)), sp0 = sp;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const double a = S.a(r, k);
      sp = fma_r(a, w[k], sp);
      sp0 = fma_r(a, start_point(k), sp0);
    }
    const double sr = Ln.end(sp, -S.b(r)), sr0 = Ln.end(sp0, -S.b(r));
    Pw = fma_r(sr, sr, Pw);
    P0 = fma_r(sr0, sr0, P0);
  });
  const bool keep = Pw <= P0;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    if (var(k) < DC) {
      const double v = keep ? w[k] : start_point(k);
      F.w_critic[(long)var(k) * B + b] = (real)v;
      F.w_prev[(long)var(k) * B + b] = (real)v;  // w_critic_prev = w_critic (controllers.py:1471)
    }
  }
}

// Everything of one env: [env step] -> [push] -> [fit], in and out through the handle's tensors, by the env's LANES lanes (this
// one is lane s of them; lane 0 stores the env's state and buffers).  One lane: the body of k_critic_fit (lane == env) and of
// the critic phase of k_ticks_mem (rcg_ticks.hpp: the lanes that stand for the wave's envs); four: of k_critic_fit_ml and of
// k_ticks_mem's four-lane form.  Every lane runs the step, the push and b (the same bits whatever the lanes) but keeps only
// ITS columns of the regressor rows - round 6: with the whole 3 x 35 stack and three 35-entry box arrays per lane the
// four-lane kernel needed 256 VGPRs + 134 AGPRs (one wave per SIMD).
template <typename Sys, typename real, int CS, int MAXM, typename Lanes = FitOneLane>
__device__ __forceinline__ void critic_update_env(const FitArgs<real>& F, const KParams<double>& P, const KParams<real>& Pr,
                                                  const long b, const Lanes Ln = Lanes()) {
  constexpr int DY = sys_dy<Sys>(), DU = Sys::DU, DC = CriticDim<CS, DY, DU>::value, KEEP = fit_keep_rows(MAXM);
  CriticKept<real, DC, DY, DU, KEEP> K;
  critic_step_push<Sys, real, CS, KEEP>(F, P, Pr, b, Ln.s == 0, K);
  if (!F.do_fit) return;
  constexpr int NV = FitRegStack<MAXM, DC, Lanes>::NV;
  double A[MAXM][NV], bv[MAXM], w0[NV], lo[NV], hi[NV], L[MAXM][MAXM], lam[MAXM], dg[MAXM], rc[MAXM], res[MAXM];
  FitRegStack<MAXM, DC, Lanes> S(Ln, A, bv, w0, lo, hi, L, lam, dg, rc, res);
  critic_td_stack<Sys, real, CS, KEEP>(F, P, Pr, b, K, S);
  S.load_box(F.wcfg);
  const int m = P.n_critic - 1;  // rows of the TD stack, 1 <= m <= MAXM (checked on the host)
  critic_walk<DC, real>(F, P.B, b, Ln, S, FIT_MU_REL * (S.trace() / (double)m));
}

template <typename Sys, typename real, int CS, int MAXM>
__global__ __launch_bounds__(64) void k_critic_fit(const FitArgs<real> F, const KParams<double> P, const KParams<real> Pr) {
  const long b = F.env_lo + (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= (F.env_hi > 0 ? (long)F.env_hi : P.B)) return;
  critic_update_env<Sys, real, CS, MAXM>(F, P, Pr, b);
}

#undef RCG_FIT_INL

}  // namespace rcg
