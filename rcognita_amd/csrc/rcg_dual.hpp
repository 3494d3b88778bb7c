// rcg_dual.hpp - forward-mode dual numbers for the adjoint members of a policy registered at run time (AUTODIFF).
//
// A policy's rhs and out are templates on `real`.  Instantiated on Dual<real, W> - one value and W tangents - with the identity
// seeded on the inputs, one evaluation yields the whole Jacobian, exact up to rounding; ad_jac_T / ad_out_jac_T contract it with
// lam / gy into what k_actor_opt's sweep asks of jac_T / out_jac_T.  Duals live only inside those two functions: the rollouts
// and the line search keep calling rhs<real, true>.
//
// Rounding.  Every tangent is produced by an explicit fma_r (tangent_axpy) or by a sum of tangents, never by a bare product:
// under -ffp-contract=fast a bare product followed by a sum is fused or not per call site, and the LOOP and non-LOOP instances
// of k_actor_opt must compute the same bits.  The value of every operation is the operation on the values, so a policy's own
// choices (fma_r written out, or left to the compiler) hold for the value path as they do in rhs<real>.
//
// Sparsity.  The seeds are literal 0 / 1 and a constant such as (real)0.5 has zero tangents.  After inlining and unrolling these
// are compile-time constants; a term whose tangent factor is a known zero is dropped (tangent_axpy, tangent_sum).  For finite
// operands the result is the same number (a sum loses at most the sign of a zero); what it saves is the arithmetic and the
// registers of a dense W-wide Jacobian where the system's own is sparse.
//
// Functions on a dual: + - * / (dual with dual, dual with T), unary -, compound assignments, the six comparisons (on values),
// fma_r, sincos_sel, sincos_r, clamp_r, finite_r, sin cos tan tanh exp log sqrt fabs fmin fmax atan atan2, pow(dual, T) (and pow(dual, dual) for an exponent written as (real)2.5).
// fabs / fmin / fmax / clamp_r take the branch the values select.  Anything else called on `real` does not compile.
#pragma once
#include "rcg_math.hpp"

namespace rcg {

// the device math library's functions stay visible beside the overloads for duals declared below (a policy inside namespace
// rcg calls them unqualified on float / double, too)
using ::atan;
using ::atan2;
using ::cos;
using ::exp;
using ::fabs;
using ::fmax;
using ::fmin;
using ::log;
using ::pow;
using ::sin;
using ::sqrt;
using ::tan;
using ::tanh;

namespace dual_detail {
template <bool B, typename T = void>
struct enable_if {};
template <typename T>
struct enable_if<true, T> {
  using type = T;
};
template <typename T>
__device__ __forceinline__ bool known_zero(T x) {
  return __builtin_constant_p(x) && x == (T)0;
}
// a * t + c for a tangent t: nothing when t is a known zero, else one fma
template <typename T>
__device__ __forceinline__ T tangent_axpy(T a, T t, T c) {
  if (known_zero(t)) return c;
  return fma_r(a, t, c);
}
template <typename T>
__device__ __forceinline__ T tangent_sum(T a, T b) {
  if (known_zero(b)) return a;
  if (known_zero(a)) return b;
  return a + b;
}
template <typename T>
__device__ __forceinline__ T tangent_diff(T a, T b) {
  if (known_zero(b)) return a;
  if (known_zero(a)) return -b;
  return a - b;
}
// the device math library by element type (float forms for float)
#define RCG_DUAL_M1(NAME)                                                      \
  __device__ __forceinline__ float m_##NAME(float x) { return ::NAME##f(x); } \
  __device__ __forceinline__ double m_##NAME(double x) { return ::NAME(x); }
RCG_DUAL_M1(sin)
RCG_DUAL_M1(cos)
RCG_DUAL_M1(tan)
RCG_DUAL_M1(tanh)
RCG_DUAL_M1(exp)
RCG_DUAL_M1(log)
RCG_DUAL_M1(sqrt)
RCG_DUAL_M1(atan)
#undef RCG_DUAL_M1
__device__ __forceinline__ float m_atan2(float y, float x) { return ::atan2f(y, x); }
__device__ __forceinline__ double m_atan2(double y, double x) { return ::atan2(y, x); }
__device__ __forceinline__ float m_pow(float x, float p) { return ::powf(x, p); }
__device__ __forceinline__ double m_pow(double x, double p) { return ::pow(x, p); }
}  // namespace dual_detail

template <typename T, int W>
struct Dual {
  using value_type = T;
  static constexpr int width = W;
  T v;
  T t[W];

  Dual() = default;
  template <typename A, typename = typename dual_detail::enable_if<__is_arithmetic(A)>::type>
  __device__ __forceinline__ explicit Dual(A a) : v((T)a) {
#pragma unroll
    for (int j = 0; j < W; ++j) t[j] = (T)0;
  }
  template <typename A, typename = typename dual_detail::enable_if<__is_arithmetic(A)>::type>
  __device__ __forceinline__ Dual& operator=(A a) {
    *this = Dual(a);
    return *this;
  }

  // f(x) with value fv and derivative df at x.v
  __device__ __forceinline__ static Dual chain(const Dual& x, T fv, T df) {
    Dual r;
    r.v = fv;
#pragma unroll
    for (int j = 0; j < W; ++j) r.t[j] = dual_detail::tangent_axpy(df, x.t[j], (T)0);
    return r;
  }

  __device__ __forceinline__ friend Dual operator-(const Dual& a) {
    Dual r;
    r.v = -a.v;
#pragma unroll
    for (int j = 0; j < W; ++j) r.t[j] = -a.t[j];
    return r;
  }
  __device__ __forceinline__ friend Dual operator+(const Dual& a) { return a; }

  __device__ __forceinline__ friend Dual operator+(const Dual& a, const Dual& b) {
    Dual r;
    r.v = a.v + b.v;
#pragma unroll
    for (int j = 0; j < W; ++j) r.t[j] = dual_detail::tangent_sum(a.t[j], b.t[j]);
    return r;
  }
  __device__ __forceinline__ friend Dual operator+(const Dual& a, T s) {
    Dual r = a;
    r.v = a.v + s;
    return r;
  }
  __device__ __forceinline__ friend Dual operator+(T s, const Dual& a) {
    Dual r = a;
    r.v = s + a.v;
    return r;
  }
  __device__ __forceinline__ friend Dual operator-(const Dual& a, const Dual& b) {
    Dual r;
    r.v = a.v - b.v;
#pragma unroll
    for (int j = 0; j < W; ++j) r.t[j] = dual_detail::tangent_diff(a.t[j], b.t[j]);
    return r;
  }
  __device__ __forceinline__ friend Dual operator-(const Dual& a, T s) {
    Dual r = a;
    r.v = a.v - s;
    return r;
  }
  __device__ __forceinline__ friend Dual operator-(T s, const Dual& a) {
    Dual r = -a;
    r.v = s - a.v;
    return r;
  }
  __device__ __forceinline__ friend Dual operator*(const Dual& a, const Dual& b) {
    Dual r;
    r.v = a.v * b.v;
#pragma unroll
    for (int j = 0; j < W; ++j)
      r.t[j] = dual_detail::tangent_axpy(a.v, b.t[j], dual_detail::tangent_axpy(b.v, a.t[j], (T)0));
    return r;
  }
  __device__ __forceinline__ friend Dual operator*(const Dual& a, T s) { return chain(a, a.v * s, s); }
  __device__ __forceinline__ friend Dual operator*(T s, const Dual& a) { return chain(a, s * a.v, s); }
  // a / b: the tangent of the quotient q is (a' - q b') / b
  __device__ __forceinline__ friend Dual operator/(const Dual& a, const Dual& b) {
    Dual r;
    r.v = a.v / b.v;
    const T inv = (T)1 / b.v;
#pragma unroll
    for (int j = 0; j < W; ++j)
      r.t[j] = dual_detail::tangent_axpy(inv, dual_detail::tangent_axpy(-r.v, b.t[j], a.t[j]), (T)0);
    return r;
  }
  __device__ __forceinline__ friend Dual operator/(const Dual& a, T s) { return chain(a, a.v / s, (T)1 / s); }
  __device__ __forceinline__ friend Dual operator/(T s, const Dual& b) {
    const T q = s / b.v;
    return chain(b, q, -q / b.v);
  }
  __device__ __forceinline__ Dual& operator+=(const Dual& b) { return *this = *this + b; }
  __device__ __forceinline__ Dual& operator-=(const Dual& b) { return *this = *this - b; }
  __device__ __forceinline__ Dual& operator*=(const Dual& b) { return *this = *this * b; }
  __device__ __forceinline__ Dual& operator/=(const Dual& b) { return *this = *this / b; }
  __device__ __forceinline__ Dual& operator+=(T s) { return *this = *this + s; }
  __device__ __forceinline__ Dual& operator-=(T s) { return *this = *this - s; }
  __device__ __forceinline__ Dual& operator*=(T s) { return *this = *this * s; }
  __device__ __forceinline__ Dual& operator/=(T s) { return *this = *this / s; }

#define RCG_DUAL_CMP(OP)                                                                                   \
  __device__ __forceinline__ friend bool operator OP(const Dual& a, const Dual& b) { return a.v OP b.v; } \
  __device__ __forceinline__ friend bool operator OP(const Dual& a, T s) { return a.v OP s; }             \
  __device__ __forceinline__ friend bool operator OP(T s, const Dual& a) { return s OP a.v; }
  RCG_DUAL_CMP(<)
  RCG_DUAL_CMP(>)
  RCG_DUAL_CMP(<=)
  RCG_DUAL_CMP(>=)
  RCG_DUAL_CMP(==)
  RCG_DUAL_CMP(!=)
#undef RCG_DUAL_CMP

  // a * b + c, the value with one rounding as fma_r(T, T, T) has it; T operands carry no tangent
  __device__ __forceinline__ friend Dual fma_r(const Dual& a, const Dual& b, const Dual& c) {
    Dual r;
    r.v = fma_r(a.v, b.v, c.v);
#pragma unroll
    for (int j = 0; j < W; ++j)
      r.t[j] = dual_detail::tangent_axpy(a.v, b.t[j], dual_detail::tangent_axpy(b.v, a.t[j], c.t[j]));
    return r;
  }
  __device__ __forceinline__ friend Dual fma_r(const Dual& a, const Dual& b, T c) { return fma_r(a, b, Dual(c)); }
  __device__ __forceinline__ friend Dual fma_r(const Dual& a, T b, const Dual& c) { return fma_r(a, Dual(b), c); }
  __device__ __forceinline__ friend Dual fma_r(T a, const Dual& b, const Dual& c) { return fma_r(Dual(a), b, c); }
  __device__ __forceinline__ friend Dual fma_r(const Dual& a, T b, T c) { return fma_r(a, Dual(b), Dual(c)); }
  __device__ __forceinline__ friend Dual fma_r(T a, const Dual& b, T c) { return fma_r(Dual(a), b, Dual(c)); }
  __device__ __forceinline__ friend Dual fma_r(T a, T b, const Dual& c) { return fma_r(Dual(a), Dual(b), c); }

  __device__ __forceinline__ friend Dual sin(const Dual& x) { return chain(x, dual_detail::m_sin(x.v), dual_detail::m_cos(x.v)); }
  __device__ __forceinline__ friend Dual cos(const Dual& x) { return chain(x, dual_detail::m_cos(x.v), -dual_detail::m_sin(x.v)); }
  __device__ __forceinline__ friend Dual tan(const Dual& x) {
    const T f = dual_detail::m_tan(x.v);
    return chain(x, f, fma_r(f, f, (T)1));
  }
  __device__ __forceinline__ friend Dual tanh(const Dual& x) {
    const T f = dual_detail::m_tanh(x.v);
    return chain(x, f, fma_r(-f, f, (T)1));
  }
  __device__ __forceinline__ friend Dual exp(const Dual& x) {
    const T f = dual_detail::m_exp(x.v);
    return chain(x, f, f);
  }
  __device__ __forceinline__ friend Dual log(const Dual& x) { return chain(x, dual_detail::m_log(x.v), (T)1 / x.v); }
  __device__ __forceinline__ friend Dual sqrt(const Dual& x) {
    const T f = dual_detail::m_sqrt(x.v);
    return chain(x, f, (T)0.5 / f);
  }
  __device__ __forceinline__ friend Dual atan(const Dual& x) { return chain(x, dual_detail::m_atan(x.v), (T)1 / fma_r(x.v, x.v, (T)1)); }
  // atan2(y, x): (x y' - y x') / (x^2 + y^2)
  __device__ __forceinline__ friend Dual atan2(const Dual& y, const Dual& x) {
    Dual r;
    r.v = dual_detail::m_atan2(y.v, x.v);
    const T inv = (T)1 / fma_r(x.v, x.v, y.v * y.v);
    const T gy = x.v * inv, gx = -y.v * inv;
#pragma unroll
    for (int j = 0; j < W; ++j) r.t[j] = dual_detail::tangent_axpy(gy, y.t[j], dual_detail::tangent_axpy(gx, x.t[j], (T)0));
    return r;
  }
  // x^p for a constant exponent
  __device__ __forceinline__ friend Dual pow(const Dual& x, T p) {
    return chain(x, dual_detail::m_pow(x.v, p), p * dual_detail::m_pow(x.v, p - (T)1));
  }
  // ... and written as a dual, (real)2.5: its tangents are known zeros and the log term goes with them
  __device__ __forceinline__ friend Dual pow(const Dual& x, const Dual& p) {
    Dual r;
    r.v = dual_detail::m_pow(x.v, p.v);
    const T gx = p.v * dual_detail::m_pow(x.v, p.v - (T)1), gp = r.v * dual_detail::m_log(x.v);
#pragma unroll
    for (int j = 0; j < W; ++j) r.t[j] = dual_detail::tangent_axpy(gx, x.t[j], dual_detail::tangent_axpy(gp, p.t[j], (T)0));
    return r;
  }
  __device__ __forceinline__ friend Dual fabs(const Dual& x) { return x.v < (T)0 ? -x : x; }
  __device__ __forceinline__ friend Dual fmin(const Dual& a, const Dual& b) { return b.v < a.v ? b : a; }
  __device__ __forceinline__ friend Dual fmax(const Dual& a, const Dual& b) { return b.v > a.v ? b : a; }
  __device__ __forceinline__ friend Dual fmin(const Dual& a, T b) { return b < a.v ? Dual(b) : a; }
  __device__ __forceinline__ friend Dual fmin(T a, const Dual& b) { return b.v < a ? b : Dual(a); }
  __device__ __forceinline__ friend Dual fmax(const Dual& a, T b) { return b > a.v ? Dual(b) : a; }
  __device__ __forceinline__ friend Dual fmax(T a, const Dual& b) { return b.v > a ? b : Dual(a); }
};

template <typename T, int W>
struct is_dual<Dual<T, W>> {
  static constexpr bool value = true;
};

// (sin, cos) of a dual: the value through sincos_sel<T, HW> of the value - the rollouts' trig when HW
template <bool HW, typename D>
__device__ __forceinline__ void dual_sincos(const D& x, D* s, D* c) {
  using T = typename D::value_type;
  T sv, cv;
  sincos_sel<T, HW>(x.v, &sv, &cv);
  const D ds = D::chain(x, sv, cv), dc = D::chain(x, cv, -sv);
  *s = ds;
  *c = dc;
}

// finite_r<real>(v) on a dual: of the value (more specialised than rcg_math.hpp's, which float / double keep)
template <typename D, typename T = typename D::value_type, int W = D::width>
__device__ __forceinline__ bool finite_r(Dual<T, W> v) {
  return __builtin_isfinite(v.v);
}

// Pre<real> -> Pre<D>, field by field with zero tangents (a parameter is no variable of the derivative): Pre<real> is empty or
// an aggregate of `real` alone, which the sizes tell
template <class S, typename real, typename D>
__device__ __forceinline__ typename S::template Pre<D> lift_pre(const typename S::template Pre<real>& q) {
  using PR = typename S::template Pre<real>;
  using PD = typename S::template Pre<D>;
  PD qd;
  if constexpr (!__is_empty(PR)) {
    constexpr int n = (int)(sizeof(PR) / sizeof(real));
    static_assert(sizeof(PR) == n * sizeof(real) && sizeof(PD) == n * sizeof(D),
                  "AUTODIFF: Pre<real> must be empty or hold members of type real only (arrays included): its fields are lifted "
                  "to dual numbers one by one");
    real a[n];
    D b[n];
    __builtin_memcpy(a, &q, sizeof(PR));
#pragma unroll
    for (int i = 0; i < n; ++i) b[i] = D(a[i]);
    __builtin_memcpy(&qd, b, sizeof(PD));
  }
  return qd;
}

// (A^T lam, B^T lam) of S::rhs at (x, u): one evaluation on DS + DU tangents, the identity seeded on (x, u); the sums run in
// index order
template <class S, typename real, bool HW>
__device__ __forceinline__ void ad_jac_T(const typename S::template Pre<real>& q, const real* x, const real* u, const real* lam,
                                         real* ax, real* bu) {
  constexpr int DS = S::DS, DU = S::DU, W = DS + DU;
  using D = Dual<real, W>;
  D xd[DS], ud[DU], dd[DS];
#pragma unroll
  for (int i = 0; i < DS; ++i) {
    xd[i] = D(x[i]);
    xd[i].t[i] = (real)1;
  }
#pragma unroll
  for (int i = 0; i < DU; ++i) {
    ud[i] = D(u[i]);
    ud[i].t[DS + i] = (real)1;
  }
  const auto qd = lift_pre<S, real, D>(q);
  S::template rhs<D, HW>(qd, xd, ud, dd);
#pragma unroll
  for (int j = 0; j < W; ++j) {
    real acc = (real)0;
#pragma unroll
    for (int i = 0; i < DS; ++i) acc = dual_detail::tangent_axpy(lam[i], dd[i].t[j], acc);
    if (j < DS)
      ax[j] = acc;
    else
      bu[j - DS] = acc;
  }
}

// gx = (d out / d x)^T gy of S::out at x: one evaluation on DS tangents
template <class S, typename real, bool HW, int DY = S::DY>
__device__ __forceinline__ void ad_out_jac_T(const typename S::template Pre<real>& q, const real* x, const real* gy, real* gx) {
  constexpr int DS = S::DS;
  using D = Dual<real, DS>;
  D xd[DS], yd[DY];
#pragma unroll
  for (int i = 0; i < DS; ++i) {
    xd[i] = D(x[i]);
    xd[i].t[i] = (real)1;
  }
  const auto qd = lift_pre<S, real, D>(q);
  S::template out<D, HW>(qd, xd, yd);
#pragma unroll
  for (int j = 0; j < DS; ++j) {
    real acc = (real)0;
#pragma unroll
    for (int m = 0; m < DY; ++m) acc = dual_detail::tangent_axpy(gy[m], yd[m].t[j], acc);
    gx[j] = acc;
  }
}

}  // namespace rcg
