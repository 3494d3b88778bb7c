// rcg_nominal.hpp - k_nominal: the reference's nominal (benchmark / fallback) controllers for a batch of envs,
// lane == env.
//
//   CtrlNominal3WRobotNI  rcognita/controllers.py:1757-1956  closed form: disassembled subgradient of a CLF in
//                         non-holonomic coordinates, kappa = -cbrt(zeta . g_k), action = gain * kappa mapped back
//   CtrlNominal3WRobot    rcognita/controllers.py:1495-1755  nonsmooth backstepping on top of it; needs
//                         theta* = argmin_theta Fc(xNI, eta, theta)
//
// The reference finds theta* with SciPy trust-constr from theta = 0 (controllers.py:1618-1627): a LOCAL search.  The
// build defines it as: on the 64-point grid of Fc's period walk downhill from theta = 0 to a grid-local minimum, then 40
// golden-section steps around it, midpoint wrapped to [-pi, pi] - exactly oracle/nominal_oracle.py::theta_star, which
// is pinned against the reference's own outputs (tests/golden/F10_nominal_*.npz: the reference's minimiser on 93 % of the
// states; round 1 took the global minimum of the scan, which is the reference's basin on only 72 %).  Arithmetic follows the reference's expressions term by term (including the
// 0 * zeta products of its np.dot, which matter only for inf/NaN propagation).  The law takes cube roots of sums
// that cancel (it is not Lipschitz there), so it is always evaluated in float64, whatever the handle's dtype: an f32
// handle returns the f64 law of its f32 states, rounded once.  Sys2Tank has no nominal controller in the reference:
// unsupported.
#pragma once
#define RCG_NOMINAL_HPP 1
#include "rcg_kernels.hpp"

namespace rcg {

// theta* of CtrlNominal3WRobot (round 6): compass search from theta = 0, the statements of oracle/nominal_oracle.py::theta_star
constexpr double NOM_THETA_STEP0 = 0.25, NOM_THETA_TOL = 1e-9;
constexpr int NOM_THETA_MAX_ITERS = 200;

template <typename real>
__device__ __forceinline__ real sgn_r(real v) {
  return (real)((v > (real)0) - (v < (real)0));  // np.sign: 0 at 0 (NaN -> 0 here, harmless: it multiplies a NaN)
}
__device__ __forceinline__ float cbrt_r(float v) { return ::cbrtf(v); }
__device__ __forceinline__ double cbrt_r(double v) { return ::cbrt(v); }
__device__ __forceinline__ float sqrt_r(float v) { return ::sqrtf(v); }
__device__ __forceinline__ double sqrt_r(double v) { return ::sqrt(v); }
// sin / cos of the theta search (|theta| <= pi + one grid step; ~104 evaluations of Fc per env): float64 on the
// Cody-Waite + minimax form of the rollouts (2.3e-16, rcg_math.hpp) instead of the device libm's sincos: k_nominal
// 73 -> 65 us per 65536 envs (the rest is two cube roots and four divisions per evaluation)
template <typename real>
__device__ __forceinline__ void nom_sincos(real x, real* s, real* c) {
  sincos_r<real>(x, s, c);
}
template <>
__device__ __forceinline__ void nom_sincos<double>(double x, double* s, double* c) {
  sincos_fast(x, s, c);
}
__device__ __forceinline__ float abs_r(float v) { return ::fabsf(v); }
__device__ __forceinline__ double abs_r(double v) { return ::fabs(v); }
__device__ __forceinline__ float floor_r(float v) { return ::floorf(v); }
__device__ __forceinline__ double floor_r(double v) { return ::floor(v); }

// _Cart2NH (controllers.py:1636-1668, 1877-1893)
template <typename real>
__device__ __forceinline__ void nom_cart2nh(real xc, real yc, real al, real* xn, real* yc_ca_m_xc_sa) {
  real s, c;
  sincos_r<real>(al, &s, &c);
  const real p = xc * c + yc * s, q = yc * c - xc * s;
  xn[0] = al;
  xn[1] = p;
  xn[2] = -(real)2 * q - al * p;
  *yc_ca_m_xc_sa = q;
}

// _kappa (controllers.py:1592-1608): kappa_k = -sign(d_k) |d_k|^(1/3), d = zeta . (1, 0, x2) / zeta . (0, 1, -x1)
template <typename real>
__device__ __forceinline__ void nom_kappa(const real* xn, const real* z, real* kap) {
  const real d0 = z[0] * (real)1 + z[1] * (real)0 + z[2] * xn[1];
  const real d1 = z[0] * (real)0 + z[1] * (real)1 + z[2] * (-xn[0]);
  kap[0] = -cbrt_r(d0);
  kap[1] = -cbrt_r(d1);
}

// _zeta(xNI, theta) (controllers.py:1551-1590) with sqrt|x3| and |x3|^3 precomputed
template <typename real>
__device__ __forceinline__ void nom_zeta_theta(const real* xn, real sq3, real a3, real ct, real st, real* z, real* sig_out) {
  const real sig = xn[0] * ct + xn[1] * st + sq3;
  const real sig3 = sig * sig * sig;
  z[0] = (real)4 * xn[0] * xn[0] * xn[0] - (real)2 * a3 * ct / sig3;
  z[1] = (real)4 * xn[1] * xn[1] * xn[1] - (real)2 * a3 * st / sig3;
  z[2] = ((real)3 * xn[0] * ct + (real)3 * xn[1] * st + (real)2 * sq3) * (xn[2] * xn[2]) * sgn_r(xn[2]) / sig3;
  *sig_out = sig;
}

// _Fc (controllers.py:1610-1623); non-finite -> +inf (a pole of sigma~ or 0/0)
template <typename real>
__device__ __forceinline__ real nom_Fc(const real* xn, const real* eta, real sq3, real a3, real x14x24, real theta) {
  real st, ct, z[3], kap[2], sig;
  nom_sincos<real>(theta, &st, &ct);
  nom_zeta_theta<real>(xn, sq3, a3, ct, st, z, &sig);
  nom_kappa<real>(xn, z, kap);
  const real e0 = eta[0] - kap[0], e1 = eta[1] - kap[1];
  const real F = x14x24 + a3 / (sig * sig) + (real)0.5 * (e0 * e0 + e1 * e1);
  return finite_r<real>(F) ? F : inf_r<real>();
}

// Nominal<Sys>: the law of a system.  Two shapes:
//   the built-in robots  act<real>(x, gain, m, I, u, L, theta), written here;
//   `policy`             a system registered at run time whose policy has the member `nominal` (rcg.h): rcg_rtc.hip's adapter
//                        generates Nominal<RcgRtcSys> from the policy's members in every unit that includes this header -
//                        law(q, y, c, u) and, `has_lf`, lf(q, y, c), on Pre<double>, with c[0] = ctrl_gain and c[1 .. NP] =
//                        ctrl_pars.  Like the built-in laws it is evaluated in float64 whatever the handle's element type.
template <typename Sys>
struct Nominal {
  static constexpr bool supported = false, policy = false;
  template <typename real>
  __device__ static void act(const real*, real, real, real, real*, real*, real*) {}
};

template <>
struct Nominal<Sys3WRobotNI> {
  static constexpr bool supported = true, policy = false;
  // compute_action_vanila (controllers.py:1937-1947) and compute_LF (:1949-1955)
  template <typename real>
  __device__ static void act(const real* x, real gain, real, real, real* u, real* L, real* th_out) {
    *th_out = (real)0;  // the closed-form controller has no theta search
    real xn[3], q;
    nom_cart2nh<real>(x[0], x[1], x[2], xn, &q);
    const real r = sqrt_r(xn[0] * xn[0] + xn[1] * xn[1]);
    const real ax3 = abs_r(xn[2]);
    const real sq3 = sqrt_r(ax3), a3 = ax3 * ax3 * ax3;
    const real sigma = r + sq3;
    real z[3];
    if (xn[0] == (real)0 && xn[1] == (real)0) {  // nablaF at theta = 0 (controllers.py:1816-1829)
      real sig;
      nom_zeta_theta<real>(xn, sq3, a3, (real)1, (real)0, z, &sig);
    } else {  // analytic nablaL (controllers.py:1808-1812)
      const real s3 = sigma * sigma * sigma, r3 = r * r * r;
      const real w = a3 / s3 * (real)1 / r3 * (real)2;
      z[0] = (real)4 * xn[0] * xn[0] * xn[0] + w * xn[0];
      z[1] = (real)4 * xn[1] * xn[1] * xn[1] + w * xn[1];
      z[2] = (real)3 * ax3 * ax3 * sgn_r(xn[2]) + a3 / s3 * (real)1 / sq3 * sgn_r(xn[2]);
    }
    real kap[2];
    nom_kappa<real>(xn, z, kap);
    const real n0 = gain * kap[0], n1 = gain * kap[1];
    u[0] = n1 + (real)0.5 * n0 * (xn[2] + xn[0] * xn[1]);  // _NH2ctrl_Cart (controllers.py:1895-1904)
    u[1] = n0;
    *L = xn[0] * xn[0] * xn[0] * xn[0] + xn[1] * xn[1] * xn[1] * xn[1] + a3 / (sigma * sigma);
  }
};

template <>
struct Nominal<Sys3WRobot> {
  static constexpr bool supported = true, policy = false;
  // compute_action_vanila (controllers.py:1733-1748) with the build's theta search; L = Fc(theta*) (compute_LF)
  template <typename real>
  __device__ static void act(const real* x, real gain, real m, real I, real* u, real* L, real* th_out) {
    real xn[3], q, eta[2];
    nom_cart2nh<real>(x[0], x[1], x[2], xn, &q);
    eta[0] = x[4];
    eta[1] = q * x[4] + x[3];
    const real ax3 = abs_r(xn[2]);
    const real sq3 = sqrt_r(ax3), a3 = ax3 * ax3 * ax3;
    const real x14x24 = xn[0] * xn[0] * xn[0] * xn[0] + xn[1] * xn[1] * xn[1] * xn[1];
    const real PI = (real)3.141592653589793238462643383279502884;
    // compass search from theta = 0 (where the reference's trust-constr starts): look one step s to both sides, move to the lower
    // side if it is lower than the current point (the left one on a tie), else halve s; non-finite values count as +inf
    auto fin = [&](real th) -> real {
      const real v = nom_Fc<real>(xn, eta, sq3, a3, x14x24, th);
      return finite_r<real>(v) ? v : inf_r<real>();
    };
    real th = (real)0, f = fin((real)0), s = (real)NOM_THETA_STEP0;
    for (int it = 0; it < NOM_THETA_MAX_ITERS && s > (real)NOM_THETA_TOL; ++it) {
      const real fl = fin(th - s), fr = fin(th + s);
      if (fl < f && fl <= fr) {
        th -= s;
        f = fl;
      } else if (fr < f) {
        th += s;
        f = fr;
      } else {
        s *= (real)0.5;
      }
    }
    th = th - (real)2 * PI * floor_r((th + PI) / ((real)2 * PI));
    *th_out = th;
    real st, ct, z[3], kap[2], sig;
    nom_sincos<real>(th, &st, &ct);
    nom_zeta_theta<real>(xn, sq3, a3, ct, st, z, &sig);
    nom_kappa<real>(xn, z, kap);
    const real e0 = eta[0] - kap[0], e1 = eta[1] - kap[1];
    const real n0 = -gain * e0, n1 = -gain * e1;
    // _NH2ctrl_Cart (controllers.py:1670-1691)
    u[0] = m * (n1 + xn[1] * eta[0] * eta[0] + (real)0.5 * (xn[0] * xn[1] * n0 + n0 * xn[2]));
    u[1] = I * n0;
    *L = x14x24 + a3 / (sig * sig) + (real)0.5 * (e0 * e0 + e1 * e1);
  }
};

// ---- the law of a policy (Nominal<Sys>::policy), shared by k_nominal and k_ticks_nominal (rcg_ticks.hpp) --------------------
constexpr int NOM_MAX_NP = 8;  // NOMINAL_NP of a policy: 0 .. 8 (rcg.h)

// Pre<double> of env b: prepare<double> of the handle's parameters - the env's, with per-env parameters - widened
template <typename Sys, typename real>
__device__ __forceinline__ typename Sys::template Pre<double> load_pre_wide(const KParams<real>& P, const real* pars_env, long b) {
  double pv[Sys::NP > 0 ? Sys::NP : 1];
#pragma unroll
  for (int i = 0; i < Sys::NP; ++i) pv[i] = (double)(pars_env ? pars_env[(long)i * P.B + b] : P.pars[i]);
  return Sys::template prepare<double>(pv);
}

// u = the law of one env, clipped (`clip`) and rounded once to the handle's element type; *L = nominal_lf (`want_lf`, a policy
// that has it), else 0.  `in`: the observation [DY] or - obs_x, a system with an output map: a tick - the state [DS], of which
// y = out<double>(state) is taken.  The law's inputs and outputs are pinned (pin_value): what the compiler may contract inside the
// member is then the same in every kernel that inlines it, and k_ticks_nominal's bits equal k_nominal's.
template <typename Sys, typename real>
__device__ __forceinline__ void nominal_policy(const KParams<real>& P, const typename Sys::template Pre<double>& q, const double* c,
                                               const real* in, int obs_x, int clip, bool want_lf, real* u, double* L) {
  constexpr int DS = Sys::DS, DU = Sys::DU, DY = sys_dy<Sys>();
  double yd[DY], ud[DU];
  bool from_state = false;
  if constexpr (HasOut<Sys>::value) from_state = obs_x != 0;
  if (from_state) {
    if constexpr (HasOut<Sys>::value) {
      double xd[DS];
#pragma unroll
      for (int k = 0; k < DS; ++k) xd[k] = (double)in[k];
      Sys::template out<double, false>(q, xd, yd);
    }
  } else {
#pragma unroll
    for (int k = 0; k < DY; ++k) yd[k] = (double)in[k];
  }
#pragma unroll
  for (int k = 0; k < DY; ++k) pin_value(yd[k]);
#pragma unroll
  for (int k = 0; k < DU; ++k) ud[k] = 0;
  Nominal<Sys>::law(q, yd, c, ud);
#pragma unroll
  for (int k = 0; k < DU; ++k) {
    pin_value(ud[k]);
    if (clip && P.clip) ud[k] = clamp_r<double>(ud[k], (double)P.lo[k], (double)P.hi[k]);
    u[k] = (real)ud[k];
  }
  *L = 0;
  if constexpr (Nominal<Sys>::has_lf) {
    if (want_lf) {
      // on a pinned copy of y: the two members then share no subexpression, and the law's bits do not depend on whether the
      // policy has nominal_lf or on whether the value is asked for (k_ticks_nominal never asks)
      double yl[DY];
#pragma unroll
      for (int k = 0; k < DY; ++k) {
        yl[k] = yd[k];
        pin_value(yl[k]);
      }
      double v = Nominal<Sys>::lf(q, yl, c);
      pin_value(v);
      *L = v;
    }
  }
}

// upd_accum_obj (controllers.py:1086-1093) as k_nominal states it, at the observation y [DY] and the rounded action
template <typename Sys, typename real>
__device__ __forceinline__ real nominal_charge(const KParams<real>& P, const real* y, const real* u, real accum) {
  constexpr int DY = sys_dy<Sys>(), DU = Sys::DU, NCHI = DY + DU;
  real chi[NCHI];
  if (P.has_target)
    make_chi<DY, DU, true, real>(P, y, u, chi);
  else
    make_chi<DY, DU, false, real>(P, y, u, chi);
  accum += stage_any<NCHI, real>(P, chi) * P.sampling_time;
  return accum;
}

template <typename real>
struct NomArgs {
  const real* obs;    // [ds][n]; a policy: [dy][n], or (obs_x) the state [ds][n]
  real* action;       // [du][n] out (or nullptr)
  real* lyap;         // [n] out: compute_LF (or nullptr)
  real* theta;        // [n] out: theta* of _minimizer_theta (or nullptr; 0 for the closed-form NI controller)
  real* accum;        // tick: accum += rho(obs, action) * sampling_time (or nullptr)
  int32_t* step_idx;  // tick: += 1 (or nullptr)
  long n;
  double gain, m, I;
  int clip;
  // a policy's law (Nominal<Sys>::policy)
  int obs_x;                 // `obs` holds states: y = out(state) (a tick of a system with an output map)
  const real* pars_env;      // [np][n] or nullptr
  double c[NOM_MAX_NP + 1];  // ctrl_gain, ctrl_pars
};

template <typename Sys, typename real>
__global__ __launch_bounds__(256) void k_nominal(const NomArgs<real> A, const KParams<real> P) {
  constexpr int DS = Sys::DS, DU = Sys::DU, NCHI = DS + DU;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n) return;
  if constexpr (Nominal<Sys>::policy) {
    constexpr int DY = sys_dy<Sys>();
    int obs_x = 0;
    if constexpr (HasOut<Sys>::value) obs_x = A.obs_x;
    real in[sys_dxy<Sys>()], u[DU];
    load_obs_raw<Sys, real>(A.obs, obs_x, A.n, i, in);
    const auto qd = load_pre_wide<Sys, real>(P, A.pars_env, i);
    double L;
    nominal_policy<Sys, real>(P, qd, A.c, in, obs_x, A.clip, A.lyap != nullptr, u, &L);
    if (A.action) {
#pragma unroll
      for (int c = 0; c < DU; ++c) A.action[(long)c * A.n + i] = u[c];
    }
    if (A.lyap) A.lyap[i] = (real)L;
    if (A.theta) A.theta[i] = (real)0;
    if (A.accum) {  // at y = out(STATE) as every tick kernel forms it (obs_of_raw)
      real y[DY];
      obs_of_raw<Sys, real>(load_pre<Sys, real>(P, A.pars_env, i), obs_x, in, y);
      A.accum[i] = nominal_charge<Sys, real>(P, y, u, A.accum[i]);
    }
    if (A.step_idx) A.step_idx[i] += 1;
  } else {
    real x[DS], u[DU];
    double xd[DS], ud[DU], L, th;
#pragma unroll
    for (int c = 0; c < DS; ++c) {
      x[c] = A.obs[(long)c * A.n + i];
      xd[c] = (double)x[c];
    }
    Nominal<Sys>::template act<double>(xd, A.gain, A.m, A.I, ud, &L, &th);
#pragma unroll
    for (int c = 0; c < DU; ++c) {
      // compute_action clips (controllers.py:1712-1714), compute_action_vanila does not
      if (A.clip && P.clip) ud[c] = clamp_r<double>(ud[c], (double)P.lo[c], (double)P.hi[c]);
      u[c] = (real)ud[c];
    }
    if (A.action) {
#pragma unroll
      for (int c = 0; c < DU; ++c) A.action[(long)c * A.n + i] = u[c];
    }
    if (A.lyap) A.lyap[i] = (real)L;
    if (A.theta) A.theta[i] = (real)th;
    if (A.accum) {  // upd_accum_obj (controllers.py:1086-1093)
      real chi[NCHI];
      if (P.has_target)
        make_chi<DS, DU, true, real>(P, x, u, chi);
      else
        make_chi<DS, DU, false, real>(P, x, u, chi);
      A.accum[i] += stage_any<NCHI, real>(P, chi) * P.sampling_time;
    }
    if (A.step_idx) A.step_idx[i] += 1;
  }
}

}  // namespace rcg
