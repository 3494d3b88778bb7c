// rcg_rtc.hip - systems registered at run time (rcg_register_system, include/rcg.h).
//
// A registered system is a policy struct in the shape of the built-ins (rcg_systems.hpp), given as source text.  The library
// compiles it with hipRTC for gfx950 against the kernel headers it was built from - embedded at build time
// (tools/embed_rtc_headers.py), so nothing reads the source tree at run time - with the Makefile's options, and launches the
// instances through hipModuleLaunchKernel:
//   at registration  a small probe program (the policy's optional members), then the f32 and f64 core programs: k_rhs,
//                    k_stage_obj, k_sim, k_actor (streamed / generated x generic / diagonal stage cost x target, and the DIRECT
//                    long-row form), k_actor_opt without LOOP when the policy has jac_T (and out_jac_T if it has out), k_out
//                    when the policy has an output map `out` (DY = dim_output; every kernel then observes y = out(x));
//   on first use     k_actor_dma / k_actor_dma_packed at the handle's row length and variant: one small program each, cached;
//   per device       a code object is loaded (hipModuleLoadData) the first time a handle on that device launches from it.
// The grid, residency and LDS request of every decision launch come from actor_plan / opt_plan (rcg_sysops.hpp), the functions
// the built-in launchers use.  What is not compiled is refused with RCG_ERR_UNSUPPORTED before anything is enqueued: the critic
// kernels, the nominal controllers, the device search, T ticks per launch and rcg_loop_step (rcg_create refuses RQL / SQL and
// the disturbance model for these systems).  One mutex guards the registry and every cache, the compiler runs outside it,
// and a handle keeps the functions it has resolved; nothing is ever unregistered or unloaded (handles point into the registry).
#include <hip/hiprtc.h>

#include <cctype>
#include <map>
#include <memory>
#include <mutex>
#include <tuple>

#include "rcg_rtc_headers.inc"  // kRtcHeaderCount, kRtcHeaderNames, kRtcHeaderTexts (generated under build/)
#include "rcg_sysops.hpp"

using namespace rcg;

namespace {

struct RtcProgram {
  std::string code;                                  // code object for gfx950
  std::map<std::string, std::string> lowered;        // name expression -> lowered name
  std::map<int, hipModule_t> module;                 // device -> loaded code object
  std::map<std::pair<int, std::string>, hipFunction_t> fn;
};

}  // namespace

struct RtcSystem {
  int id;
  std::string name, src;
  RtcDims dims;
  bool tgt;                 // the policy's TGT (default false): which k_actor_dma instance serves a handle with a target
  RtcProgram core[2];       // [0] float, [1] double
  std::map<std::tuple<int, int, int, int>, std::unique_ptr<RtcProgram>> dma;  // (f64, packed, R, variant)
};

namespace {

std::mutex g_mu;  // the registry and every cache below it
std::vector<std::unique_ptr<RtcSystem>> g_sys;

const char* const kSysExpr = "rcg::RcgRtcSys";
// the Makefile's device options (HIPFLAGS), without RCG_DEV
const char* const kOpts[] = {"--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=fast"};

template <typename real>
const char* real_name() {
  return sizeof(real) == 8 ? "double" : "float";
}

bool is_identifier(const char* s) {
  if (!s || !(isalpha((unsigned char)s[0]) || s[0] == '_')) return false;
  for (const char* p = s; *p; ++p)
    if (!(isalnum((unsigned char)*p) || *p == '_')) return false;
  return strlen(s) < 128;
}

// The generated unit: the kernel headers, the policy (its own file name and line numbers in hipRTC's log), the adapter that
// supplies the optional members and the checks of the declared dimensions.
std::string unit_source(const RtcSystem& S) {
  char dims[1536];
  snprintf(dims, sizeof dims,
           "static_assert(RcgRtcSys::DS == %d, \"rcg_register_system: %s::DS differs from the declared ds\");\n"
           "static_assert(RcgRtcSys::DU == %d, \"rcg_register_system: %s::DU differs from the declared du\");\n"
           "static_assert(RcgRtcSys::NP == %d, \"rcg_register_system: %s::NP differs from the declared np\");\n"
           "static_assert(RcgRtcSys::HAS_OUT || RcgRtcSys::DY == RcgRtcSys::DS, \"rcg_register_system: %s::DY differs from DS "
           "but %s defines no out (without an output map the observation is the state)\");\n",
           S.dims.ds, S.name.c_str(), S.dims.du, S.name.c_str(), S.dims.np, S.name.c_str(), S.name.c_str(), S.name.c_str());
  const std::string& N = S.name;
  return "#include \"rcg_actor_dma_packed.hpp\"\n#include \"rcg_actor_opt.hpp\"\nnamespace rcg {\n#line 1 \"" + N + ".policy\"\n" +
         S.src +
         "\n#line 1 \"rcg_rtc_adapter\"\n"
         "namespace rtc {\n"
         "template <class...> using void_t = void;\n"
         "template <class S, class = void> struct tgt { static constexpr bool v = false; };\n"
         "template <class S> struct tgt<S, void_t<decltype(S::TGT)>> { static constexpr bool v = S::TGT; };\n"
         "template <class S, class = void> struct zw { static constexpr unsigned v = 0u; };\n"
         "template <class S> struct zw<S, void_t<decltype(S::ZW_PRESET)>> { static constexpr unsigned v = S::ZW_PRESET; };\n"
         "template <class S, class = void> struct su1 { static constexpr unsigned v = 0u; };\n"
         "template <class S> struct su1<S, void_t<decltype(S::SHARED_U1)>> { static constexpr unsigned v = S::SHARED_U1; };\n"
         "template <class S, class = void> struct jac { static constexpr bool v = false; };\n"
         "template <class S> struct jac<S, void_t<decltype(&S::template jac_T<float, true>)>> { static constexpr bool v = true; };\n"
         "template <class S, class = void> struct out { static constexpr bool v = false; };\n"
         "template <class S> struct out<S, void_t<decltype(&S::template out<float, true>)>> { static constexpr bool v = true; };\n"
         "template <class S, class = void> struct ojac { static constexpr bool v = false; };\n"
         "template <class S> struct ojac<S, void_t<decltype(&S::template out_jac_T<float, true>)>> { static constexpr bool v = true; };\n"
         "template <class S, class = void> struct dy { static constexpr int v = S::DS; };\n"
         "template <class S> struct dy<S, void_t<decltype(S::DY)>> { static constexpr int v = S::DY; };\n"
         "template <bool TGT, bool JAC, int DY, bool OUT, bool OJAC> __global__ void k_rtc_probe() {}\n"
         "}  // namespace rtc\n"
         "struct RcgRtcSys : " + N + " {\n"
         "  static constexpr bool TGT = rtc::tgt<" + N + ">::v;\n"
         "  static constexpr unsigned ZW_PRESET = rtc::zw<" + N + ">::v;\n"
         "  static constexpr unsigned SHARED_U1 = rtc::su1<" + N + ">::v;\n"
         "  static constexpr bool HAS_OUT = rtc::out<" + N + ">::v;\n"
         "  static constexpr int DY = rtc::dy<" + N + ">::v;\n"
         "};\n" +
         dims + "}  // namespace rcg\n";
}

// Compile `src` and look up the lowered names of `exprs`.  Returns RCG_OK, or RCG_ERR_BAD_ARG with hipRTC's log in *log.
int compile(const std::string& src, const std::string& file, const std::vector<std::string>& exprs, RtcProgram* out,
            std::string* log) {
  std::vector<const char*> names, texts;
  for (int i = 0; i < kRtcHeaderCount; ++i) {
    names.push_back(kRtcHeaderNames[i]);
    texts.push_back(kRtcHeaderTexts[i]);
  }
  // the kernel headers include the HIP runtime headers, which hipRTC does not need (it declares the device builtins itself)
  for (const char* stub : {"hip/hip_runtime.h", "hip/hip_ext.h"}) {
    names.push_back(stub);
    texts.push_back("\n");
  }
  hiprtcProgram prog;
  if (hiprtcCreateProgram(&prog, src.c_str(), file.c_str(), (int)names.size(), texts.data(), names.data()) != HIPRTC_SUCCESS) {
    *log = "hiprtcCreateProgram failed";
    return RCG_ERR_HIP;
  }
  for (const auto& e : exprs) hiprtcAddNameExpression(prog, e.c_str());
  const hiprtcResult rc = hiprtcCompileProgram(prog, (int)(sizeof kOpts / sizeof kOpts[0]), kOpts);
  size_t n = 0;
  hiprtcGetProgramLogSize(prog, &n);
  std::string text(n, '\0');
  if (n) hiprtcGetProgramLog(prog, &text[0]);
  while (!text.empty() && text.back() == '\0') text.pop_back();
  if (rc != HIPRTC_SUCCESS) {
    *log = std::string(hiprtcGetErrorString(rc)) + ":\n" + text;
    hiprtcDestroyProgram(&prog);
    return RCG_ERR_BAD_ARG;
  }
  n = 0;
  hiprtcGetCodeSize(prog, &n);
  out->code.assign(n, '\0');
  if (n) hiprtcGetCode(prog, &out->code[0]);
  for (const auto& e : exprs) {
    const char* low = nullptr;
    if (hiprtcGetLoweredName(prog, e.c_str(), &low) != HIPRTC_SUCCESS || !low) {
      *log = "hiprtcGetLoweredName: no instance " + e;
      hiprtcDestroyProgram(&prog);
      return RCG_ERR_HIP;
    }
    out->lowered[e] = low;
  }
  hiprtcDestroyProgram(&prog);
  return n ? RCG_OK : RCG_ERR_HIP;
}

std::string tf(bool b) { return b ? "true" : "false"; }

template <typename real>
std::string expr_rhs() {
  return std::string("rcg::k_rhs<") + kSysExpr + ", " + real_name<real>() + ">";
}
template <typename real>
std::string expr_stage_obj() {
  return std::string("rcg::k_stage_obj<") + kSysExpr + ", " + real_name<real>() + ">";
}
template <typename real>
std::string expr_out() {
  return std::string("rcg::k_out<") + kSysExpr + ", " + real_name<real>() + ">";
}
template <typename real>
std::string expr_sim(bool tgt) {
  return std::string("rcg::k_sim<") + kSysExpr + ", " + real_name<real>() + ", " + tf(tgt) + ">";
}
template <typename real>
std::string expr_actor(bool gen, bool tgt, bool str, bool direct) {
  return std::string("rcg::k_actor<") + kSysExpr + ", " + real_name<real>() + ", " + tf(gen) + ", " + tf(tgt) + ", " + tf(str) +
         (direct ? ", false, true>" : ">");
}
template <typename real>
std::string expr_opt(bool tgt, bool gen, bool pairs) {
  return std::string("rcg::k_actor_opt<") + kSysExpr + ", " + real_name<real>() + ", " + tf(tgt) + ", " + tf(gen) + ", " + tf(pairs) +
         ">";
}
// k_actor_dma's TGT parameter is the system's own for the preset-cost variants, true for DMA_MPC_GEND / GENF (rcg_dma_launch.hpp)
template <typename real>
std::string expr_dma(bool packed, int R, int variant, bool sys_tgt) {
  const bool tgt = (!packed && variant >= DMA_MPC_GEND) ? true : sys_tgt;
  return std::string(packed ? "rcg::k_actor_dma_packed<" : "rcg::k_actor_dma<") + kSysExpr + ", " + real_name<real>() + ", " +
         std::to_string(R) + ", " + tf(tgt) + ", " + std::to_string(variant) + ">";
}

template <typename real>
std::vector<std::string> core_exprs(const RtcDims& d) {
  const bool has_jac = d.has_jac && (!d.has_out || d.has_out_jac);  // (the optimiser's adjoint needs both with an output map)
  std::vector<std::string> e{expr_rhs<real>(), expr_stage_obj<real>(), expr_sim<real>(false), expr_sim<real>(true)};
  if (d.has_out) e.push_back(expr_out<real>());
  for (int g = 0; g < 2; ++g)
    for (int t = 0; t < 2; ++t) {
      for (int s = 0; s < 2; ++s) e.push_back(expr_actor<real>(g, t, s, false));
      if (g) e.push_back(expr_actor<real>(true, t, true, true));
    }
  if (has_jac)
    for (int sel = 0; sel < 8; ++sel) e.push_back(expr_opt<real>(sel & 2, sel & 4, sel & 1));
  return e;
}

// the function `expr` of program `P` on the handle's device (the caller holds g_mu)
int function(rcg_handle* h, RtcProgram& P, const std::string& expr, hipFunction_t* fn) {
  const int dev = h->cfg.device;
  auto it = P.fn.find({dev, expr});
  if (it != P.fn.end()) {
    *fn = it->second;
    return RCG_OK;
  }
  auto low = P.lowered.find(expr);
  if (low == P.lowered.end()) return rcg_fail(h, RCG_ERR_HIP, "runtime system: no compiled instance %s", expr.c_str());
  if (!P.module.count(dev)) {
    hipModule_t m = nullptr;
    HIPCHK(h, hipModuleLoadData(&m, P.code.data()));
    P.module[dev] = m;
  }
  hipFunction_t f = nullptr;
  HIPCHK(h, hipModuleGetFunction(&f, P.module[dev], low->second.c_str()));
  P.fn[{dev, expr}] = f;
  *fn = f;
  return RCG_OK;
}

// A handle keeps the functions it has resolved (h->rtc_fn): after the first launch of an instance, a launch takes no lock.
// (A registered system's name, source, dimensions and TGT never change once it is published: read without the lock.)
template <typename real>
int core_function(rcg_handle* h, const std::string& expr, hipFunction_t* fn) {
  auto hit = h->rtc_fn.find(expr);
  if (hit != h->rtc_fn.end()) {
    *fn = hit->second;
    return RCG_OK;
  }
  std::lock_guard<std::mutex> lock(g_mu);
  RtcSystem& S = *const_cast<RtcSystem*>(h->rtc);
  const int rc = function(h, S.core[sizeof(real) == 8 ? 1 : 0], expr, fn);
  if (rc == RCG_OK) h->rtc_fn[expr] = *fn;
  return rc;
}

// k_actor_dma / k_actor_dma_packed at the handle's row length: compiled the first time a handle of this (system, element type)
// asks for it - outside the lock, so that launches of other handles do not wait for the compiler - then cached
template <typename real>
int dma_function(rcg_handle* h, bool packed, int R, int variant, hipFunction_t* fn) {
  RtcSystem& S = *const_cast<RtcSystem*>(h->rtc);
  const std::string expr = expr_dma<real>(packed, R, variant, S.tgt);
  auto hit = h->rtc_fn.find(expr);
  if (hit != h->rtc_fn.end()) {
    *fn = hit->second;
    return RCG_OK;
  }
  const auto key = std::make_tuple(sizeof(real) == 8 ? 1 : 0, packed ? 1 : 0, R, variant);
  bool have;
  {
    std::lock_guard<std::mutex> lock(g_mu);
    have = S.dma.count(key) != 0;
  }
  std::unique_ptr<RtcProgram> P;
  if (!have) {
    P.reset(new RtcProgram);
    std::string log;
    const int rc = compile(unit_source(S), S.name + "_dma.hip", {expr}, P.get(), &log);
    if (rc) {
      h->err = "runtime system " + S.name + ": compiling " + expr + ": " + log;
      return RCG_ERR_HIP;
    }
  }
  std::lock_guard<std::mutex> lock(g_mu);
  auto it = S.dma.find(key);
  if (it == S.dma.end()) it = S.dma.emplace(key, std::move(P)).first;  // (another thread may have published it meanwhile)
  const int rc = function(h, *it->second, expr, fn);
  if (rc == RCG_OK) h->rtc_fn[expr] = *fn;
  return rc;
}

// one launch on the handle's stream; inside a due ProfScope it carries the scope's event pair (rcg_profile)
int launch(rcg_handle* h, hipFunction_t f, dim3 grid, dim3 block, size_t lds, void** args) {
  const ProfPair pp = prof_take(h);
  hipError_t e;
  if (pp.a)
    e = hipExtModuleLaunchKernel(f, grid.x * block.x, grid.y * block.y, grid.z * block.z, block.x, block.y, block.z, lds,
                                 h->stream, args, nullptr, pp.a, pp.b, 0);
  else
    e = hipModuleLaunchKernel(f, grid.x, grid.y, grid.z, block.x, block.y, block.z, (unsigned)lds, h->stream, args, nullptr);
  if (e != hipSuccess) return rcg_fail(h, RCG_ERR_HIP, "runtime system: kernel launch failed: %s", hipGetErrorString(e));
  return RCG_OK;
}

int refuse(rcg_handle* h, const char* who) {
  return rcg_fail(h, RCG_ERR_UNSUPPORTED, "%s: not available for a system registered at run time (%s)", who,
                  h->rtc ? h->rtc->name.c_str() : "?");
}

// ---- the table -----------------------------------------------------------------------------------------------------------
int rtc_rhs(rcg_handle* h, const void* state, const void* action, void* dstate, void* clipped, int32_t n, int32_t clip) {
  return by_dtype(h, [&](auto r) {
    using real = decltype(r);
    hipFunction_t f;
    int rc = core_function<real>(h, expr_rhs<real>(), &f);
    if (rc) return rc;
    const real* st = (const real*)state;
    const real* ac = (const real*)action;
    real* ds = (real*)dstate;
    real* cl = (real*)clipped;
    const real* pe = (h->f[RCG_FIELD_PARS] && n == h->cfg.batch) ? (const real*)h->f[RCG_FIELD_PARS] : nullptr;
    long nn = n;
    int ci = clip;
    KParams<real> P = params<real>(h);
    void* args[] = {&st, &ac, &ds, &cl, &pe, &nn, &ci, &P};
    return launch(h, f, dim3(blocks_for(n)), dim3(256), 0, args);
  });
}

int rtc_stage_obj(rcg_handle* h, const void* obs, const void* act, void* out, int32_t n) {
  return by_dtype(h, [&](auto r) {
    using real = decltype(r);
    hipFunction_t f;
    int rc = core_function<real>(h, expr_stage_obj<real>(), &f);
    if (rc) return rc;
    const real* o = (const real*)obs;
    const real* a = (const real*)act;
    real* y = (real*)out;
    long nn = n;
    KParams<real> P = params<real>(h);
    void* args[] = {&o, &a, &y, &nn, &P};
    return launch(h, f, dim3(blocks_for(n)), dim3(256), 0, args);
  });
}

// the env step: k_sim (lane = env) at every batch size - k_sim_v, which the built-in light systems take from 2^18 envs on,
// computes the same bits
template <typename real>
int sim_step(rcg_handle* h, int32_t n_substeps) {
  hipFunction_t f;
  int rc = core_function<real>(h, expr_sim<real>((h->cfg.flags & RCG_FLAG_HAS_TARGET) != 0), &f);
  if (rc) return rc;
  SimArgs<real> A = sim_args<real>(h, n_substeps);
  KParams<real> P = params<real>(h);
  void* args[] = {&A, &P};
  ProfScope prof_scope(h, RCG_KERNEL_SIM);
  note_launch(h, RCG_KERNEL_SIM, RCG_KID_SIM, 0, 64);
  return launch(h, f, dim3(blocks_for(h->cfg.batch)), dim3(256), 0, args);
}

int rtc_sim_step(rcg_handle* h, int32_t n_substeps) {
  return by_dtype(h, [&](auto r) { return sim_step<decltype(r)>(h, n_substeps); });
}

// The decision step: the kernel launch_actor (rcg_sysops.hpp) picks for the same plan, except the instances written for one
// built-in system (GenPk, k_ticks_pk).  The instance is resolved - and compiled, the first time - before anything is enqueued.
template <typename real>
int actor(rcg_handle* h, const char* who, const void* cand, int K, const void* obs, const void* state_sys, const void* w, void* J,
          void* action, void* best_J, int32_t* best_idx, bool tick, bool sim_first) {
  const RtcSystem& S = *h->rtc;
  ActorArgs<real> A;
  ActorPlan L;
  int rc = actor_plan<real>(h, who, S.dims.ds, S.dims.du, S.tgt, cand, K, obs, state_sys, w, J, action, best_J, best_idx, tick,
                            sim_first, A, L);
  if (rc) return rc;
  if (h->probe == 1) {
    h->probe = (L.dma_ok && !L.pack_ok) ? 3 : 2;
    return RCG_OK;
  }
  if (h->sub_hi > 0 && !(L.dma_ok && !L.pack_ok))
    return rcg_fail(h, RCG_ERR_UNSUPPORTED, "%s: a split tick needs the k_actor_dma shape", who);
  // (MPC only: the variants are DMA_MPC_G1 / DMA_MPC - the packed ones, diagonal stage cost - and DMA_MPC_GEND / GENF)
  const bool packed = L.pack_ok, dma = !packed && L.dma_ok;
  hipFunction_t f;
  if (packed || dma)
    rc = dma_function<real>(h, packed, L.R, L.variant, &f);
  else
    rc = core_function<real>(h, expr_actor<real>(L.long_row || L.generic, L.tgt, cand != nullptr, L.long_row), &f);
  if (rc) return rc;
  const bool fuse_sim = packed && L.fuse_sim;
  if (sim_first && !fuse_sim) {
    rc = sim_step<real>(h, h->cfg.substeps_per_tick);
    if (rc) return rc;
  }
  KParams<real> P = params<real>(h);
  ProfScope prof_scope(h, RCG_KERNEL_ACTOR);
  if (packed) {
    ActorArgs<real> Ap = packed_args(h, A, L);
    void* args[] = {&Ap, &P};
    rc = launch(h, f, L.pack_grid, dim3(256), L.pack_lds, args);
    if (rc == RCG_OK) note_launch(h, RCG_KERNEL_ACTOR, RCG_KID_ACTOR_DMA_PACKED, L.variant | (fuse_sim ? 16 : 0), (int)L.pack_gpw);
    return rc;
  }
  if (dma) {
    ActorArgs<real> Ad = dma_args(h, A, L);
    void* args[] = {&Ad, &P};
    rc = launch(h, f, L.dma_grid, dim3(256), L.dma_lds, args);
    if (rc == RCG_OK) note_launch(h, RCG_KERNEL_ACTOR, RCG_KID_ACTOR_DMA, L.variant, (int)L.dma_gpw);
    return rc;
  }
  void* args[] = {&A, &P};
  rc = launch(h, f, dim3(L.blocks), dim3(64 * L.wpb), L.long_row ? 0 : L.lds, args);
  if (rc == RCG_OK)
    note_launch(h, RCG_KERNEL_ACTOR, RCG_KID_ACTOR,
                L.long_row ? (1 | (L.tgt ? 2 : 0) | 4 | 16) : ((L.generic ? 1 : 0) | (L.tgt ? 2 : 0) | (cand ? 4 : 0)), A.G);
  return rc;
}

int rtc_actor(rcg_handle* h, const char* who, const void* cand, int K, const void* obs, const void* state_sys, const void* w,
              void* J, void* action, void* best_J, int32_t* best_idx, bool tick, bool sim_first) {
  return by_dtype(h, [&](auto r) {
    return actor<decltype(r)>(h, who, cand, K, obs, state_sys, w, J, action, best_J, best_idx, tick, sim_first);
  });
}

int rtc_optimize(rcg_handle* h, int32_t iters, const void* obs, const void* state_sys, const void* u_init, int shift, void* u_opt,
                 void* action, void* best_J, int32_t* n_iter, bool tick, bool sim_first) {
  if (!h->rtc->dims.has_jac)
    return rcg_fail(h, RCG_ERR_UNSUPPORTED, "rcg_actor_optimize: the policy %s defines no jac_T (the optimiser's adjoint sweep)",
                    h->rtc->name.c_str());
  if (h->rtc->dims.has_out && !h->rtc->dims.has_out_jac)
    return rcg_fail(h, RCG_ERR_UNSUPPORTED,
                    "rcg_actor_optimize: the policy %s defines out but no out_jac_T (the adjoint of its output map)",
                    h->rtc->name.c_str());
  if (h->loop_io.on) return refuse(h, "rcg_loop_step");
  return by_dtype(h, [&](auto r) {
    using real = decltype(r);
    const rcg_cfg& c = h->cfg;
    OptArgs<real> A;
    int wpb;
    size_t lds;
    int rc = opt_plan<real>(h, h->du, iters, obs, state_sys, u_init, shift, u_opt, action, best_J, n_iter, tick, A, wpb, lds);
    if (rc) return rc;
    KParams<real> P = params<real>(h);
    const bool generic = !(c.mode == RCG_MODE_MPC && P.stage_kind == 0);
    const bool tgt = c.flags & RCG_FLAG_HAS_TARGET;
    const bool pairs = A.memory > 0;
    hipFunction_t f;
    rc = core_function<real>(h, expr_opt<real>(tgt, generic, pairs), &f);
    if (rc) return rc;
    if (tick && sim_first) {
      rc = sim_step<real>(h, c.substeps_per_tick);
      if (rc) return rc;
    }
    // (beyond 64 KB of dynamic LDS the built-in launcher calls hipFuncSetAttribute, which has no module-function form and
    // admits any size up to the CU's 160 KB on this platform: the module launch takes the size as it is)
    ProfScope prof_scope(h, RCG_KERNEL_ACTOR);
    void* args[] = {&A, &P};
    rc = launch(h, f, dim3(blocks_for(c.batch, wpb * OPT_G)), dim3(64 * wpb), lds, args);
    if (rc == RCG_OK)
      note_launch(h, RCG_KERNEL_ACTOR, RCG_KID_ACTOR_OPT, (generic ? 1 : 0) | (tgt ? 2 : 0) | (pairs ? 4 : 0), OPT_G);
    return rc;
  });
}

int rtc_critic(rcg_handle* h, const void*, const void*, const void*, void*, int32_t) { return refuse(h, "rcg_critic"); }
int rtc_critic_cost(rcg_handle* h, const void*, void*) { return refuse(h, "rcg_critic_cost"); }
int rtc_critic_update(rcg_handle* h, int32_t, int32_t, int32_t) { return refuse(h, "the critic update"); }
int rtc_nominal(rcg_handle* h, const void*, void*, void*, void*, int32_t, double, const double*, int32_t, bool) {
  return refuse(h, "the nominal controller");
}
int rtc_ticks(rcg_handle* h, int32_t, int32_t, const void*) { return refuse(h, "rcg_control_ticks"); }
int rtc_rhs_full(rcg_handle* h, const void*, const void*, const void*, const void*, void*, void*, void*, int32_t, int32_t) {
  return refuse(h, "rcg_rhs_full");
}
int rtc_search(rcg_handle* h, int32_t, int32_t, int32_t, const void*, const void*, const void*, int, void*, void*, void*, int32_t*,
               bool, bool) {
  return refuse(h, "rcg_actor_search");
}
int rtc_loop(rcg_handle* h, const double*, int32_t, int32_t, int32_t, int32_t, int32_t, double*, double*, double) {
  return refuse(h, "rcg_loop_step");
}

// the probe program: which optional members the policy has (the values travel in the lowered name of an empty kernel:
// k_rtc_probe<TGT, JAC, DY, OUT, OJAC> mangles its arguments as Lb0E / Lb1E and Li<n>E / Lin<n>E)
int probe(RtcSystem& S, std::string* log) {
  const std::string pol = "rcg::" + S.name;
  const std::string e = std::string("rcg::rtc::k_rtc_probe<") + kSysExpr + "::TGT, rcg::rtc::jac<" + pol + ">::v, " + kSysExpr +
                        "::DY, " + kSysExpr + "::HAS_OUT, rcg::rtc::ojac<" + pol + ">::v>";
  RtcProgram P;
  const int rc = compile(unit_source(S), S.name + "_probe.hip", {e}, &P, log);
  if (rc) return rc;
  const std::string& low = P.lowered[e];
  long v[5];
  size_t p = low.find("IL");
  int n = 0;
  for (p = p == std::string::npos ? p : p + 1; p != std::string::npos && n < 5 && p + 2 < low.size() && low[p] == 'L'; ++n) {
    const char t = low[p + 1];
    size_t q = p + 2;
    const bool neg = t == 'i' && low[q] == 'n';
    if (neg) ++q;
    long x = 0;
    while (q < low.size() && isdigit((unsigned char)low[q])) x = 10 * x + (low[q++] - '0');
    if ((t != 'b' && t != 'i') || q >= low.size() || low[q] != 'E') break;
    v[n] = neg ? -x : x;
    p = q + 1;
  }
  if (n != 5) {
    *log = "cannot read the probe instance " + low;
    return RCG_ERR_HIP;
  }
  S.tgt = v[0] != 0;
  S.dims.has_jac = v[1] != 0;
  S.dims.dy = (int)v[2];
  S.dims.has_out = v[3] != 0;
  S.dims.has_out_jac = S.dims.has_out && v[4] != 0;
  return RCG_OK;
}

}  // namespace

#if !defined(__HIP_DEVICE_COMPILE__)  // (the table of host function pointers exists in the host pass only)
const SysVTable kVtRtc = {&rtc_rhs,     &rtc_stage_obj, &rtc_critic,   &rtc_critic_cost, &rtc_actor,
                          &rtc_sim_step, &rtc_critic_update, &rtc_optimize, &rtc_nominal, &rtc_ticks,
                          &rtc_rhs_full, &rtc_search,    &rtc_ticks,    &rtc_loop};
#endif

int rtc_out(rcg_handle* h, const void* state, void* obs, int32_t n) {
  return by_dtype(h, [&](auto r) {
    using real = decltype(r);
    hipFunction_t f;
    int rc = core_function<real>(h, expr_out<real>(), &f);
    if (rc) return rc;
    const real* st = (const real*)state;
    real* y = (real*)obs;
    const real* pe = (h->f[RCG_FIELD_PARS] && n == h->cfg.batch) ? (const real*)h->f[RCG_FIELD_PARS] : nullptr;
    long nn = n;
    KParams<real> P = params<real>(h);
    void* args[] = {&st, &y, &pe, &nn, &P};
    return launch(h, f, dim3(blocks_for(n)), dim3(256), 0, args);
  });
}

const RtcSystem* rtc_lookup(int sys_id, RtcDims* dims) {
  std::lock_guard<std::mutex> lock(g_mu);
  const int i = sys_id - RCG_SYS_USER_BASE;
  if (i < 0 || i >= (int)g_sys.size()) return nullptr;
  if (dims) *dims = g_sys[i]->dims;
  return g_sys[i].get();
}

extern "C" {

int rcg_register_system(const char* name, const char* policy_src, int32_t ds, int32_t du, int32_t np, int32_t* sys_id) {
  if (!name || !policy_src || !sys_id) return rcg_fail(nullptr, RCG_ERR_BAD_ARG, "rcg_register_system: null argument");
  if (!is_identifier(name))
    return rcg_fail(nullptr, RCG_ERR_BAD_ARG, "rcg_register_system: the name must be the policy struct's C++ identifier");
  if (ds < 1 || du < 1 || np < 0) return rcg_fail(nullptr, RCG_ERR_BAD_ARG, "rcg_register_system: need ds >= 1, du >= 1, np >= 0");
  if (ds > RCG_MAX_DS || du > RCG_MAX_DU || np > RCG_MAX_PARS)
    return rcg_fail(nullptr, RCG_ERR_UNSUPPORTED, "rcg_register_system: ds %d, du %d, np %d beyond the limits %d, %d, %d", ds, du, np,
                    RCG_MAX_DS, RCG_MAX_DU, RCG_MAX_PARS);
  // the same name again: the registered id, or a refusal (checked before and, for a concurrent registration, after compiling)
  auto known = [&](int* rc) -> bool {
    for (const auto& s : g_sys) {
      if (s->name != name) continue;
      if (s->src != policy_src || s->dims.ds != ds || s->dims.du != du || s->dims.np != np) {
        *rc = rcg_fail(nullptr, RCG_ERR_BAD_ARG, "rcg_register_system: %s is registered already, with another source or dimensions",
                       name);
      } else {
        *sys_id = s->id;
        *rc = RCG_OK;
      }
      return true;
    }
    return false;
  };
  int rc = RCG_OK;
  {
    std::lock_guard<std::mutex> lock(g_mu);
    if (known(&rc)) return rc;
  }
  // compiled without the lock: launches of the systems registered so far do not wait for the compiler
  std::unique_ptr<RtcSystem> S(new RtcSystem);
  S->name = name;
  S->src = policy_src;
  S->dims = RtcDims{ds, du, np, false, ds, false, false};
  S->tgt = false;
  std::string log;
  rc = probe(*S, &log);
  // dim_output: chi = [y - target, u] must fit RCG_MAX_CHI and the target KParams::target (a DY other than DS without `out` is
  // refused by the adapter's static_assert above, with hipRTC's log)
  if (rc == RCG_OK && (S->dims.dy < 1 || S->dims.dy > RCG_MAX_DS))
    return rcg_fail(nullptr, RCG_ERR_UNSUPPORTED, "rcg_register_system: %s::DY = %d beyond 1 .. %d", name, S->dims.dy, RCG_MAX_DS);
  if (rc == RCG_OK) rc = compile(unit_source(*S), S->name + "_f32.hip", core_exprs<float>(S->dims), &S->core[0], &log);
  if (rc == RCG_OK) rc = compile(unit_source(*S), S->name + "_f64.hip", core_exprs<double>(S->dims), &S->core[1], &log);
  if (rc) {
    rcg_set_thread_error(std::string("rcg_register_system: ") + name + ": " + log);
    return rc;
  }
  std::lock_guard<std::mutex> lock(g_mu);
  if (known(&rc)) return rc;
  S->id = RCG_SYS_USER_BASE + (int)g_sys.size();
  *sys_id = S->id;
  g_sys.push_back(std::move(S));
  return RCG_OK;
}

int rcg_rtc_version(int32_t* major, int32_t* minor) {
  int a = 0, b = 0;
  if (hiprtcVersion(&a, &b) != HIPRTC_SUCCESS) return rcg_fail(nullptr, RCG_ERR_HIP, "rcg_rtc_version: hiprtcVersion failed");
  if (major) *major = a;
  if (minor) *minor = b;
  return RCG_OK;
}

}  // extern "C"
