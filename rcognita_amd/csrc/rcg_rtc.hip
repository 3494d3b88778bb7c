// rcg_rtc.hip - systems registered at run time (rcg_register_system, include/rcg.h).
//
// A registered system is a policy struct in the shape of the built-ins (rcg_systems.hpp), given as source text.  The library
// compiles it with hipRTC for gfx950 against the kernel headers it was built from - embedded at build time
// (tools/embed_rtc_headers.py), so nothing reads the source tree at run time - with the Makefile's options, and launches the
// instances through hipModuleLaunchKernel:
//   at registration  a small probe program (the policy's optional members), then the f32 and f64 core programs: k_rhs,
//                    k_stage_obj, k_sim, k_actor (streamed / generated x generic / diagonal stage cost x target, and the DIRECT
//                    long-row form), k_actor_opt without its LOOP form when the policy has jac_T (and out_jac_T if it has out), k_out
//                    when the policy has an output map `out` (DY = dim_output; every kernel then observes y = out(x));
//   on first use     one small program per instance, through one routine (lazy_function) and one cache (RtcSystem::lazy) keyed
//                    by the name expression that selects the instance:
//                    k_actor_dma / k_actor_dma_packed at the handle's row length and variant (<name>_dma.hip);
//                    for a policy that opts in with `static constexpr bool CRITIC = true`, the critic program of a handle's
//                    (element type, critic structure, fit form): k_critic, k_critic_cost and the fit kernel fit_plan picks,
//                    keyed by the fit kernel (<name>_critic.hip);
//                    for a policy that opts in with `static constexpr bool SEARCH = true`, the k_actor_search instance
//                    search_plan picks for a handle (<name>_search.hip);
//                    for a policy that opts in with `static constexpr bool TICKS = true`, the k_ticks instance ticks_plan picks
//                    (<name>_ticks.hip) and the k_ticks_mem instance ticks_mem_plan picks (<name>_ticks_mem.hip);
//                    for a policy that opts in to the disturbance model with `static constexpr int DD` and the member `disturb`,
//                    the disturb program of an element type, the first time a handle with RCG_FLAG_DISTURB steps an env or asks
//                    for rcg_rhs_full: k_sim_dist (with and without a target) and k_rhs_full (<name>_disturb.hip).  The adapter
//                    generates Disturb<RcgRtcSys> from the two members in every unit that includes rcg_disturb.hpp, so the
//                    k_ticks instances of such a policy run the disturbed env step too (TicksArgs::dist);
//                    for a policy that opts in with `static constexpr bool LOOP = true`, the loop program of a handle's element
//                    type and target setting, the first time the handle calls rcg_loop_step(_begin): k_loop and, when the policy
//                    has jac_T (and out_jac_T with out), the LOOP instance of k_actor_opt (<name>_loop.hip);
//                    for a policy with jac_T (and out_jac_T with out), k_jac_T of an element type the first time a handle calls
//                    rcg_jac_T (<name>_jac.hip);
//   A policy that opts in with `static constexpr bool AUTODIFF = true` has the adjoint members it does not write itself: the adapter
//   derives jac_T / out_jac_T from rhs / out on forward-mode dual numbers (rcg_dual.hpp), the probe reports them as members, and
//   everything above that asks for jac_T serves the policy as it serves one with hand-written members (rcg_system_autodiff).
//   per device       a code object is loaded (hipModuleLoadData) the first time a handle on that device launches from it.
// The grid, residency and LDS request of every decision launch come from actor_plan / opt_plan / search_plan / ticks_plan /
// ticks_mem_plan (rcg_sysops.hpp), the functions the built-in launchers use, those of the critic update from fit_plan.  What is
// not compiled is refused with RCG_ERR_UNSUPPORTED before anything is enqueued: the critic kernels of a policy without CRITIC
// (rcg_create refuses RQL / SQL for it), the device search of a policy without SEARCH, T ticks per launch of a policy without
// TICKS, rcg_loop_step of a policy without LOOP (and its decision without jac_T), the nominal controllers of a policy without
// the member `nominal` (with it: k_nominal as <name>_nominal.hip per element type, and - with TICKS - the k_ticks_nominal
// instance of a handle as <name>_ticks_nominal.hip, both compiled on first use); rcg_create refuses
// the disturbance model for a policy without `disturb`, and under it RQL / SQL through k_ticks_mem, the two-halves tick and the
// fused env step stay refused or unfused as for the built-in systems.  One mutex
// guards the registry and every cache, the compiler runs outside it, and a handle keeps the functions it has resolved; nothing
// is ever unregistered or unloaded (handles point into the registry).
#include <hip/hiprtc.h>

#include <cctype>
#include <map>
#include <memory>
#include <mutex>

#include "rcg_rtc_headers.inc"  // kRtcHeaderCount, kRtcHeaderNames, kRtcHeaderTexts (generated under build/)
#include "rcg_sysops.hpp"

using namespace rcg;

namespace {

struct RtcProgram {
  std::string code;                                  // code object for gfx950
  std::map<std::string, std::string> lowered;        // name expression -> lowered name
  // (filled as devices first launch from the program, under g_mu: not part of what a registered system is)
  mutable std::map<int, hipModule_t> module;         // device -> loaded code object
  mutable std::map<std::pair<int, std::string>, hipFunction_t> fn;
};

}  // namespace

struct RtcSystem {
  int id;
  std::string name, src;
  RtcDims dims;
  bool tgt;                 // the policy's TGT (default false): which k_actor_dma instance serves a handle with a target
  unsigned zw;              // the policy's ZW_PRESET (default 0): the zero-weight instance of k_actor_dma's DMA_MPC_G1 (float64)
  RtcProgram core[2];       // [0] float, [1] double
  // the programs compiled on first use (lazy_function), by the name expression that defines each: the instance itself, or the
  // fit kernel of a critic program
  std::map<std::string, std::unique_ptr<RtcProgram>> lazy;
  std::vector<std::string> compiled;  // "<program>\t<name expression>" of everything compiled so far (rcg_system_programs)
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

// The generated unit: the kernel headers of its flavour (Core: the probe, the core programs and the k_actor_dma instances), the
// policy (its own file name and line numbers in hipRTC's log), the adapter that supplies the optional members and the checks of
// the declared dimensions.
enum class Unit { Core, Critic, Search, Ticks, Disturb, Loop, Nominal };  // (Loop: the Core unit's headers hold k_loop and k_actor_opt)
std::string unit_source(const RtcSystem& S, Unit unit) {
  const bool critic = unit == Unit::Critic, search = unit == Unit::Search, ticks = unit == Unit::Ticks;
  const bool disturb = unit == Unit::Disturb;
  char dims[2560];
  snprintf(dims, sizeof dims,
           "static_assert(RcgRtcSys::DS == %d, \"rcg_register_system: %s::DS differs from the declared ds\");\n"
           "static_assert(RcgRtcSys::DU == %d, \"rcg_register_system: %s::DU differs from the declared du\");\n"
           "static_assert(RcgRtcSys::NP == %d, \"rcg_register_system: %s::NP differs from the declared np\");\n"
           "static_assert(RcgRtcSys::HAS_OUT || RcgRtcSys::DY == RcgRtcSys::DS, \"rcg_register_system: %s::DY differs from DS "
           "but %s defines no out (without an output map the observation is the state)\");\n"
           "static_assert(!rtc::dd<%s>::has || rtc::dist<%s>::v, \"rcg_register_system: %s defines DD but no disturb member "
           "(the disturbance model needs both: template <typename real> static void disturb(q, x, u, w, d))\");\n"
           "static_assert(!rtc::dist<%s>::v || rtc::dd<%s>::has, \"rcg_register_system: %s defines disturb but no DD member "
           "(the disturbance model needs both: static constexpr int DD = 1 or 2)\");\n",
           S.dims.ds, S.name.c_str(), S.dims.du, S.name.c_str(), S.dims.np, S.name.c_str(), S.name.c_str(), S.name.c_str(),
           S.name.c_str(), S.name.c_str(), S.name.c_str(), S.name.c_str(), S.name.c_str(), S.name.c_str());
  const std::string& N = S.name;
  // the nominal law's members come together (the DD / disturb rule): NOMINAL_NP or nominal_lf without nominal names what is missing
  const std::string nom_rules =
      "static_assert(!rtc::nomnp<" + N + ">::has || rtc::nom<" + N + ">::v, \"rcg_register_system: " + N +
      " defines NOMINAL_NP but no nominal member (the nominal control law: template <typename real> static void nominal(q, y, c, u))\");\n"
      "static_assert(!rtc::nomlf<" + N + ">::v || rtc::nom<" + N + ">::v, \"rcg_register_system: " + N +
      " defines nominal_lf but no nominal member (the nominal control law: template <typename real> static void nominal(q, y, c, u))\");\n";
  return std::string(critic ? "#include \"rcg_critic_fit_ml.hpp\"\n#include \"rcg_critic_fit_gen.hpp\"\n" : "") +
         (search ? "#include \"rcg_search.hpp\"\n" : "") +
         (ticks ? "#include \"rcg_critic_fit_ml.hpp\"\n#include \"rcg_ticks.hpp\"\n" : "") +
         (disturb ? "#include \"rcg_disturb.hpp\"\n" : "") +
         // (rcg_nominal.hpp in every unit: a policy's `nominal` may call the library's own law functions, and its text is compiled in all)
         "#include \"rcg_actor_dma_packed.hpp\"\n#include \"rcg_actor_opt.hpp\"\n#include \"rcg_dual.hpp\"\n#include \"rcg_nominal.hpp\"\nnamespace rcg {\n#line 1 \"" + N + ".policy\"\n" +
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
         "template <class S, class = void> struct crit { static constexpr bool v = false; };\n"
         "template <class S> struct crit<S, void_t<decltype(S::CRITIC)>> { static constexpr bool v = S::CRITIC; };\n"
         "template <class S, class = void> struct srch { static constexpr bool v = false; };\n"
         "template <class S> struct srch<S, void_t<decltype(S::SEARCH)>> { static constexpr bool v = S::SEARCH; };\n"
         "template <class S, class = void> struct tck { static constexpr bool v = false; };\n"
         "template <class S> struct tck<S, void_t<decltype(S::TICKS)>> { static constexpr bool v = S::TICKS; };\n"
         "template <class S, class = void> struct dd { static constexpr bool has = false; static constexpr int v = 0; };\n"
         "template <class S> struct dd<S, void_t<decltype(S::DD)>> { static constexpr bool has = true; static constexpr int v = S::DD; };\n"
         "template <class S, class = void> struct dist { static constexpr bool v = false; };\n"
         "template <class S> struct dist<S, void_t<decltype(&S::template disturb<float>)>> { static constexpr bool v = true; };\n"
         "template <class S> struct ddv { static constexpr int v = dist<S>::v ? (dd<S>::v == 0 ? -1 : dd<S>::v) : 0; };\n"
         "template <class S, class = void> struct lp { static constexpr bool v = false; };\n"
         "template <class S> struct lp<S, void_t<decltype(S::LOOP)>> { static constexpr bool v = S::LOOP; };\n"
         "template <class S, class = void> struct ad { static constexpr bool v = false; };\n"
         "template <class S> struct ad<S, void_t<decltype(S::AUTODIFF)>> { static constexpr bool v = S::AUTODIFF; };\n"
         "template <class S, class = void> struct nom { static constexpr bool v = false; };\n"
         "template <class S> struct nom<S, void_t<decltype(&S::template nominal<double>)>> { static constexpr bool v = true; };\n"
         "template <class S, class = void> struct nomlf { static constexpr bool v = false; };\n"
         "template <class S> struct nomlf<S, void_t<decltype(&S::template nominal_lf<double>)>> { static constexpr bool v = true; };\n"
         "template <class S, class = void> struct nomnp { static constexpr bool has = false; static constexpr int v = 0; };\n"
         "template <class S> struct nomnp<S, void_t<decltype(S::NOMINAL_NP)>> { static constexpr bool has = true; static constexpr int v = S::NOMINAL_NP; };\n"
         // the adjoint members a policy with AUTODIFF does not write, derived from its rhs / out (rcg_dual.hpp); RcgRtcSys inherits
         // them beside the policy, so a member the policy writes is the only one of its name
         "template <class S, bool ON> struct ad_jac {};\n"
         "template <class S> struct ad_jac<S, true> {\n"
         "  template <typename real, bool HW = false>\n"
         "  __device__ __forceinline__ static void jac_T(const typename S::template Pre<real>& q, const real* x, const real* u,\n"
         "                                               const real* lam, real* ax, real* bu) {\n"
         "    ad_jac_T<S, real, HW>(q, x, u, lam, ax, bu);\n"
         "  }\n"
         "};\n"
         "template <class S, bool ON> struct ad_ojac {};\n"
         "template <class S> struct ad_ojac<S, true> {\n"
         "  template <typename real, bool HW = false>\n"
         "  __device__ __forceinline__ static void out_jac_T(const typename S::template Pre<real>& q, const real* x, const real* gy,\n"
         "                                                   real* gx) {\n"
         "    ad_out_jac_T<S, real, HW, dy<S>::v>(q, x, gy, gx);\n"
         "  }\n"
         "};\n"
         "template <bool TGT, bool JAC, int DY, bool OUT, bool OJAC, bool CRIT, bool SRCH, bool TCK, unsigned ZW, int DD, bool LP, "
         "bool AD, int NOM, int NNP> __global__ void k_rtc_probe() {}\n"
         "}  // namespace rtc\n"
         "struct RcgRtcSys : " + N + ", rtc::ad_jac<" + N + ", rtc::ad<" + N + ">::v && !rtc::jac<" + N + ">::v>,\n"
         "                   rtc::ad_ojac<" + N + ", rtc::ad<" + N + ">::v && rtc::out<" + N + ">::v && !rtc::ojac<" + N + ">::v> {\n"
         "  static constexpr bool TGT = rtc::tgt<" + N + ">::v;\n"
         "  static constexpr unsigned ZW_PRESET = rtc::zw<" + N + ">::v;\n"
         "  static constexpr unsigned SHARED_U1 = rtc::su1<" + N + ">::v;\n"
         "  static constexpr bool HAS_OUT = rtc::out<" + N + ">::v;\n"
         "  static constexpr int DY = rtc::dy<" + N + ">::v;\n"
         "};\n" +
         // Disturb<RcgRtcSys>, in every unit that includes rcg_disturb.hpp (k_ticks and k_actor_search name it): the policy's DD
         // and `disturb`, or - a policy that does not opt in - an inert one shaped like Disturb<Sys2Tank> (rcg_create refuses the
         // disturbance model for it, so TicksArgs::dist is 0 and env_substeps_dist never runs)
         "#ifdef RCG_DISTURB_HPP\n"
         "namespace rtc {\n"
         "template <class S, bool ON> struct disturb_of {\n"
         "  static constexpr int DD = 1;\n"
         "  static constexpr bool inert = true;\n"
         "  template <typename real>\n"
         "  __device__ __forceinline__ static void apply(const typename S::template Pre<real>&, const real*, const real*, const real*,\n"
         "                                               real*) {}\n"
         "};\n"
         "template <class S> struct disturb_of<S, true> {\n"
         "  static constexpr int DD = S::DD;\n"
         "  static constexpr bool inert = false;\n"
         "  template <typename real>\n"
         "  __device__ __forceinline__ static void apply(const typename S::template Pre<real>& q, const real* x, const real* u,\n"
         "                                               const real* w, real* d) {\n"
         "    S::template disturb<real>(q, x, u, w, d);\n"
         "  }\n"
         "};\n"
         "}  // namespace rtc\n"
         "template <> struct Disturb<RcgRtcSys> : rtc::disturb_of<" + N + ", (rtc::ddv<" + N + ">::v > 0)> {};\n"
         "#endif\n"
         // Nominal<RcgRtcSys>, in every unit that includes rcg_nominal.hpp (the nominal program; rcg_ticks.hpp names it): the policy's
         // `nominal` / `nominal_lf` on double, or - a policy without the member - an unsupported one that does nothing (the entry
         // points refuse such a policy by name before anything is launched)
         "#ifdef RCG_NOMINAL_HPP\n"
         "namespace rtc {\n"
         "template <class S, bool ON, bool LF> struct nominal_of {\n"
         "  static constexpr bool supported = false, policy = true, has_lf = false;\n"
         "  __device__ __forceinline__ static void law(const typename S::template Pre<double>&, const double*, const double*, double*) {}\n"
         "};\n"
         "template <class S, bool LF> struct nominal_of<S, true, LF> {\n"
         "  static constexpr bool supported = true, policy = true, has_lf = LF;\n"
         "  __device__ __forceinline__ static void law(const typename S::template Pre<double>& q, const double* y, const double* c,\n"
         "                                             double* u) {\n"
         "    S::template nominal<double>(q, y, c, u);\n"
         "  }\n"
         "  __device__ __forceinline__ static double lf(const typename S::template Pre<double>& q, const double* y, const double* c) {\n"
         "    if constexpr (LF) return S::template nominal_lf<double>(q, y, c); else return 0.0;\n"
         "  }\n"
         "};\n"
         "}  // namespace rtc\n"
         "template <> struct Nominal<RcgRtcSys> : rtc::nominal_of<" + N + ", rtc::nom<" + N + ">::v, rtc::nomlf<" + N + ">::v> {};\n"
         "#endif\n" +
         dims + nom_rules + "}  // namespace rcg\n";
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
std::string expr_jac_T() {
  return std::string("rcg::k_jac_T<") + kSysExpr + ", " + real_name<real>() + ">";
}
template <typename real>
std::string expr_sim(bool tgt) {
  return std::string("rcg::k_sim<") + kSysExpr + ", " + real_name<real>() + ", " + tf(tgt) + ">";
}
template <typename real>
std::string expr_sim_dist(bool tgt) {
  return std::string("rcg::k_sim_dist<") + kSysExpr + ", " + real_name<real>() + ", " + tf(tgt) + ">";
}
template <typename real>
std::string expr_nominal() {
  return std::string("rcg::k_nominal<") + kSysExpr + ", " + real_name<real>() + ">";
}
template <typename real>
std::string expr_ticks_nominal(bool tgt) {
  return std::string("rcg::k_ticks_nominal<") + kSysExpr + ", " + real_name<real>() + ", " + tf(tgt) + ">";
}
template <typename real>
std::string expr_rhs_full() {
  return std::string("rcg::k_rhs_full<") + kSysExpr + ", " + real_name<real>() + ">";
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
// the loop program (rcg_loop_step): the glue kernel, and the LOOP instance of the plain MPC decision (op_optimize's)
template <typename real>
std::string expr_loop() {
  return std::string("rcg::k_loop<") + kSysExpr + ", " + real_name<real>() + ">";
}
template <typename real>
std::string expr_opt_loop(bool tgt) {
  return std::string("rcg::k_actor_opt<") + kSysExpr + ", " + real_name<real>() + ", " + tf(tgt) + ", false, false, true>";
}
// k_actor_dma's TGT parameter is the system's own for the preset-cost variants, true for DMA_MPC_GEND / GENF (rcg_dma_launch.hpp);
// zw != 0: the zero-weight instance of DMA_MPC_G1 (rcg_actor_dma.hpp::dma_zero_w) - a registered copy of a robot resolves to
// the instance the built-in one runs
template <typename real>
std::string expr_dma(bool packed, int R, int variant, bool sys_tgt, unsigned zw) {
  const bool tgt = (!packed && variant >= DMA_MPC_GEND) ? true : sys_tgt;
  return std::string(packed ? "rcg::k_actor_dma_packed<" : "rcg::k_actor_dma<") + kSysExpr + ", " + real_name<real>() + ", " +
         std::to_string(R) + ", " + tf(tgt) + ", " + std::to_string(variant) + (zw ? ", " + std::to_string(zw) + "u>" : ">");
}

template <typename real>
std::string expr_critic() {
  return std::string("rcg::k_critic<") + kSysExpr + ", " + real_name<real>() + ">";
}
template <typename real>
std::string expr_critic_cost() {
  return std::string("rcg::k_critic_cost<") + kSysExpr + ", " + real_name<real>() + ">";
}
// the fit kernel of a form (rcg_sysops.hpp::fit_plan)
template <typename real>
std::string expr_fit(int cs, int form) {
  const std::string head = std::string("<") + kSysExpr + ", " + real_name<real>() + ", " + std::to_string(cs);
  if (form == FIT_FORM_GEN) return "rcg::k_critic_fit_gen" + head + ">";
  if (form == FIT_FORM_3ML) return "rcg::k_critic_fit_ml" + head + ", 3>";
  return "rcg::k_critic_fit" + head + ", " + std::to_string(form == FIT_FORM_3 ? 3 : kFitMaxRows) + ">";
}
// the k_actor_search instance of a plan (rcg_sysops.hpp::search_plan): the register-row instances take the policy's own TGT
template <typename real>
std::string expr_search(bool generic, bool tgt, int nc) {
  return std::string("rcg::k_actor_search<") + kSysExpr + ", " + real_name<real>() + ", " + tf(generic) + ", " + tf(tgt) + ", " +
         std::to_string(nc) + ">";
}

// the k_ticks / k_ticks_mem instance of a plan (rcg_sysops.hpp::ticks_plan, ticks_mem_plan)
template <typename real>
std::string expr_ticks(const TicksPlan& L) {
  return std::string("rcg::k_ticks<") + kSysExpr + ", " + real_name<real>() + ", " + tf(L.generic) + ", " + tf(L.tgt) + ", " +
         tf(L.stream) + ">";
}
template <typename real>
std::string expr_ticks_mem(const TicksMemPlan& L) {
  return std::string("rcg::k_ticks_mem<") + kSysExpr + ", " + real_name<real>() + ", " + std::to_string(L.cs) + ", " +
         std::to_string(L.maxm) + ", " + tf(L.tgt) + ", " + tf(L.ml) + ", " + tf(L.stream) + ">";
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
int function(rcg_handle* h, const RtcProgram& P, const std::string& expr, hipFunction_t* fn) {
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
  const int rc = function(h, h->rtc->core[sizeof(real) == 8 ? 1 : 0], expr, fn);
  if (rc == RCG_OK) h->rtc_fn[expr] = *fn;
  return rc;
}

// A program compiled on first use: the unit of flavour `unit` with the name expressions `exprs`, as <name>_<kind>.hip.  The last
// expression defines the program and is its key in RtcSystem::lazy, so the instance that is selected and the entry that is
// cached cannot differ.  *fn is the function of exprs[want].  The program is compiled the first time a handle asks for it -
// outside the lock, so that launches of other handles do not wait for the compiler - and published under it unless another
// thread has published it meanwhile (this one's is then dropped); rcg_system_programs lists it from then on.  A compile error is
// compile()'s code - RCG_ERR_BAD_ARG when the source is at fault (a member of the policy the program instantiates for the first
// time) - with hipRTC's log in the handle's error text.
int lazy_function(rcg_handle* h, Unit unit, const char* kind, const std::vector<std::string>& exprs, size_t want,
                  hipFunction_t* fn) {
  const std::string& expr = exprs[want];
  auto hit = h->rtc_fn.find(expr);
  if (hit != h->rtc_fn.end()) {
    *fn = hit->second;
    return RCG_OK;
  }
  RtcSystem& S = *const_cast<RtcSystem*>(h->rtc);
  const std::string& key = exprs.back();
  bool have;
  {
    std::lock_guard<std::mutex> lock(g_mu);
    have = S.lazy.count(key) != 0;
  }
  const std::string file = S.name + "_" + kind + ".hip";
  std::unique_ptr<RtcProgram> P;
  if (!have) {
    P.reset(new RtcProgram);
    std::string log;
    const int rc = compile(unit_source(S, unit), file, exprs, P.get(), &log);
    if (rc) {
      const std::string what = exprs.size() == 1 ? key : std::string("the ") + kind + " program (" + key + ")";
      h->err = "runtime system " + S.name + ": compiling " + what + ": " + log;
      return rc;
    }
  }
  std::lock_guard<std::mutex> lock(g_mu);
  auto it = S.lazy.find(key);
  if (it == S.lazy.end()) {  // (else another thread has published it meanwhile)
    it = S.lazy.emplace(key, std::move(P)).first;
    for (const auto& e : exprs) S.compiled.push_back(file + "\t" + e);
  }
  const int rc = function(h, *it->second, expr, fn);
  if (rc == RCG_OK) h->rtc_fn[expr] = *fn;
  return rc;
}

// The k_actor_dma and critic programs answer a compile error with RCG_ERR_HIP, the later ones (search, ticks) with compile()'s
// RCG_ERR_BAD_ARG.  Kept on purpose: the codes are part of the library's behaviour, whichever of the two is the better one.
int compile_error_is_hip(int rc) { return rc == RCG_ERR_BAD_ARG ? RCG_ERR_HIP : rc; }

// k_actor_dma / k_actor_dma_packed at the handle's row length
template <typename real>
int dma_function(rcg_handle* h, bool packed, int R, int variant, unsigned zw, hipFunction_t* fn) {
  const int rc = lazy_function(h, Unit::Core, "dma", {expr_dma<real>(packed, R, variant, h->rtc->tgt, zw)}, 0, fn);
  return compile_error_is_hip(rc);
}

// The critic program of the handle's (element type, critic structure) and of fit form `form`: k_critic, k_critic_cost and that
// form's fit kernel; `want`: which of the three
enum { CRITIC_VALUE = 0, CRITIC_COST = 1, CRITIC_FIT = 2 };
template <typename real>
int critic_function(rcg_handle* h, int form, int want, hipFunction_t* fn) {
  if (!h->rtc->dims.has_critic) return RCG_ERR_UNSUPPORTED;  // (the callers refuse by name first)
  const std::vector<std::string> exprs{expr_critic<real>(), expr_critic_cost<real>(),
                                       expr_fit<real>(h->cfg.critic_struct, form)};
  return compile_error_is_hip(lazy_function(h, Unit::Critic, "critic", exprs, want, fn));
}
// ... of the form the handle's critic update takes (fit_plan): what a tick resolves before it enqueues anything
int critic_fit_function(rcg_handle* h, hipFunction_t* fn) {
  return by_dtype(h, [&](auto r) {
    return critic_function<decltype(r)>(h, fit_form_of(h->cfg.n_critic - 1, h->dc, false), CRITIC_FIT, fn);
  });
}

// the k_actor_search instance of a plan (search_plan gives nc > 0 only where tgt == Sys::TGT)
template <typename real>
int search_function(rcg_handle* h, const SearchPlan& L, hipFunction_t* fn) {
  return lazy_function(h, Unit::Search, "search", {expr_search<real>(L.generic, L.tgt, L.nc)}, 0, fn);
}

// The disturb program of an element type - k_sim_dist without and with a target, k_rhs_full - for a policy with DD / disturb
// (rcg_create has refused RCG_FLAG_DISTURB for any other); `want`: which of the three
enum { DISTURB_SIM = 0, DISTURB_SIM_TGT = 1, DISTURB_RHS_FULL = 2 };
template <typename real>
int disturb_function(rcg_handle* h, int want, hipFunction_t* fn) {
  if (h->rtc->dims.dd < 1) return RCG_ERR_UNSUPPORTED;  // (the callers refuse by name first)
  const std::vector<std::string> exprs{expr_sim_dist<real>(false), expr_sim_dist<real>(true), expr_rhs_full<real>()};
  return lazy_function(h, Unit::Disturb, "disturb", exprs, want, fn);
}

// The loop program of a handle's (element type, target setting) for a policy with LOOP: k_loop and - when the policy has jac_T (and
// out_jac_T with out) - the LOOP instance of k_actor_opt at that target setting, which is then the expression that keys the
// program; `want`: which of the two
enum { LOOP_GLUE = 0, LOOP_OPT = 1 };
bool rtc_has_opt(const RtcDims& d) { return d.has_jac && (!d.has_out || d.has_out_jac); }
template <typename real>
int loop_function(rcg_handle* h, int want, hipFunction_t* fn) {
  if (!h->rtc->dims.has_loop) return RCG_ERR_UNSUPPORTED;  // (the callers refuse by name first)
  std::vector<std::string> exprs{expr_loop<real>()};
  if (rtc_has_opt(h->rtc->dims)) exprs.push_back(expr_opt_loop<real>((h->cfg.flags & RCG_FLAG_HAS_TARGET) != 0));
  if ((size_t)want >= exprs.size()) return RCG_ERR_UNSUPPORTED;
  return lazy_function(h, Unit::Loop, "loop", exprs, (size_t)want, fn);
}

// a member of the table that the policy did not opt in to with `member` (CRITIC, SEARCH, TICKS, LOOP)
int refuse_opt_in(rcg_handle* h, const char* who, const char* member) {
  return rcg_fail(h, RCG_ERR_UNSUPPORTED,
                  "%s: not available for a system registered at run time whose policy does not opt in with %s (%s)", who, member,
                  h->rtc ? h->rtc->name.c_str() : "?");
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
    const real* pe = pars_env_of<real>(h, n);
    long nn = n;
    int ci = clip;
    KParams<real> P = params<real>(h);
    void* args[] = {&st, &ac, &ds, &cl, &pe, &nn, &ci, &P};
    return launch(h, f, dim3(blocks_for(n)), dim3(256), 0, args);
  });
}

// rcg_jac_T: k_jac_T of an element type, a program of its own compiled on first use (<name>_jac.hip; the registration compiles
// what it compiled before) for a policy that has the members - its own or, AUTODIFF, the derived ones
int rtc_jac_T(rcg_handle* h, const void* state, const void* action, const void* lam, void* ax, void* bu, const void* gy, void* gx,
              int32_t n) {
  const RtcDims& d = h->rtc->dims;
  if (!d.has_jac)
    return rcg_fail(h, RCG_ERR_UNSUPPORTED, "rcg_jac_T: the policy %s defines no jac_T and does not opt in with AUTODIFF",
                    h->rtc->name.c_str());
  if (d.has_out && !d.has_out_jac)
    return rcg_fail(h, RCG_ERR_UNSUPPORTED, "rcg_jac_T: the policy %s defines out but no out_jac_T and does not opt in with AUTODIFF",
                    h->rtc->name.c_str());
  return by_dtype(h, [&](auto r) {
    using real = decltype(r);
    hipFunction_t f;
    int rc = lazy_function(h, Unit::Core, "jac", {expr_jac_T<real>()}, 0, &f);
    if (rc) return rc;
    const real* st = (const real*)state;
    const real* ac = (const real*)action;
    const real* la = (const real*)lam;
    real* a = (real*)ax;
    real* b = (real*)bu;
    const real* g = (const real*)gy;
    real* o = (real*)gx;
    const real* pe = pars_env_of<real>(h, n);
    long nn = n;
    KParams<real> P = params<real>(h);
    void* args[] = {&st, &ac, &la, &a, &b, &g, &o, &pe, &nn, &P};
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
// computes the same bits; a handle with RCG_FLAG_DISTURB: k_sim_dist of the disturb program (compiled on first use, before the
// launch: the env step is the first thing every caller enqueues), with the arguments op_sim_step fills
template <typename real>
int sim_step(rcg_handle* h, int32_t n_substeps) {
  hipFunction_t f;
  const bool tgt = (h->cfg.flags & RCG_FLAG_HAS_TARGET) != 0;
  SimArgs<real> A = sim_args<real>(h, n_substeps);
  KParams<real> P = params<real>(h);
  if (h->cfg.flags & RCG_FLAG_DISTURB) {
    int rc = disturb_function<real>(h, tgt ? DISTURB_SIM_TGT : DISTURB_SIM, &f);
    if (rc) return rc;
    SimDistArgs<real> D;
    D.S = A;
    D.disturb = (real*)h->f[RCG_FIELD_DISTURB];
    D.substep_idx = (int32_t*)h->f[RCG_FIELD_SUBSTEP_IDX];
    D.episode_idx = (const int32_t*)h->f[RCG_FIELD_EPISODE_IDX];
    D.D = disturb_pars(h);
    void* args[] = {&D, &P};
    ProfScope prof_scope(h, RCG_KERNEL_SIM);
    note_launch(h, RCG_KERNEL_SIM, RCG_KID_SIM_DIST, 0, 64);
    return launch(h, f, dim3(blocks_for(h->cfg.batch)), dim3(256), 0, args);
  }
  int rc = core_function<real>(h, expr_sim<real>(tgt), &f);
  if (rc) return rc;
  void* args[] = {&A, &P};
  ProfScope prof_scope(h, RCG_KERNEL_SIM);
  note_launch(h, RCG_KERNEL_SIM, RCG_KID_SIM, 0, 64);
  return launch(h, f, dim3(blocks_for(h->cfg.batch)), dim3(256), 0, args);
}

int rtc_sim_step(rcg_handle* h, int32_t n_substeps) {
  return by_dtype(h, [&](auto r) { return sim_step<decltype(r)>(h, n_substeps); });
}

// The instance that serves a plan: which of the three decision kernels, and its function (compiled on first use).  Shared by the
// launcher below and by rtc_prepare_tick, which resolves a tick's instance before the tick enqueues anything.
// (the packed RQL / SQL variants have an instance only while the critic weights fit a lane's registers, packed_critic_ok: beyond
// that the shape goes on to k_actor_dma / k_actor, as launch_actor's does when launch_dma_packed finds no instance)
struct ActorPick {
  bool packed, dma;
  unsigned zero_w;  // k_actor_dma: the mask of the zero-weight instance, 0: the plain one
  hipFunction_t f;
};
template <typename real>
int resolve_actor_instance(rcg_handle* h, const ActorArgs<real>& A, const ActorPlan& L, bool streamed, ActorPick* p) {
  p->packed = L.pack_ok && !(L.variant >= DMA_RQL_0 && !packed_critic_ok(h->dc, (int)sizeof(real)));
  p->dma = !p->packed && L.dma_ok;
  const RtcSystem& S = *h->rtc;
  p->zero_w = (p->dma && sizeof(real) == 8 && !S.dims.has_out) ? dma_zero_w<real>(S.zw, L.variant, A, params<real>(h)) : 0u;
  if (p->packed || p->dma) return dma_function<real>(h, p->packed, L.R, L.variant, p->zero_w, &p->f);
  return core_function<real>(h, expr_actor<real>(L.long_row || L.generic, L.tgt, streamed, L.long_row), &p->f);
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
  if (rc || actor_plan_answers(h, who, L, rc)) return rc;
  ActorPick pick;
  rc = resolve_actor_instance<real>(h, A, L, cand != nullptr, &pick);
  if (rc) return rc;
  const bool packed = pick.packed, dma = pick.dma;
  hipFunction_t const f = pick.f;
  // (a fused env step that was planned for a packed instance that does not exist runs as its own launch, first)
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
    if (rc == RCG_OK) {
      note_launch(h, RCG_KERNEL_ACTOR, RCG_KID_ACTOR_DMA, L.variant, (int)L.dma_gpw);
      h->last[RCG_KERNEL_ACTOR].zero_w = pick.zero_w;
    }
    return rc;
  }
  void* args[] = {&A, &P};
  rc = launch(h, f, dim3(L.blocks), dim3(64 * L.wpb), L.long_row ? 0 : L.lds, args);
  if (rc == RCG_OK) note_launch(h, RCG_KERNEL_ACTOR, RCG_KID_ACTOR, L.word, A.G);
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
  const bool loop = h->loop_io.on;  // rcg_loop_step's one-launch sample (op_optimize): head and tail of the iteration in this launch
  if (loop && !h->rtc->dims.has_loop) return refuse_opt_in(h, "rcg_loop_step", "LOOP");
  return by_dtype(h, [&](auto r) {
    using real = decltype(r);
    OptArgs<real> A;
    OptPlan L;
    int rc = opt_plan<real>(h, h->du, iters, obs, state_sys, u_init, shift, u_opt, action, best_J, n_iter, tick, A, L);
    if (rc) return rc;
    KParams<real> P = params<real>(h);
    hipFunction_t f;
    if (loop) {  // the LOOP instance: plain MPC on the handle's own fields alone, as op_optimize asks
      if (L.generic || L.pairs || obs || state_sys != h->f[RCG_FIELD_STATE_PREV] || u_init || tick)
        return rcg_fail(h, RCG_ERR_UNSUPPORTED, "rcg_loop_step: the one-launch sample is the plain MPC instance on the handle's own fields");
      fill_loop_args<real>(h, A.loop, h->loop_io.act_in, h->loop_io.n_substeps, 1, 1, 1, h->loop_io.dc, h->loop_io.out,
                           h->loop_io.flag, h->loop_io.seq);
      rc = loop_function<real>(h, LOOP_OPT, &f);
    } else {
      rc = core_function<real>(h, expr_opt<real>(L.tgt, L.generic, L.pairs), &f);
    }
    if (rc) return rc;
    if (tick && sim_first) {
      rc = sim_step<real>(h, h->cfg.substeps_per_tick);
      if (rc) return rc;
    }
    // (beyond 64 KB of dynamic LDS the built-in launcher calls hipFuncSetAttribute, which has no module-function form and
    // admits any size up to the CU's 160 KB on this platform: the module launch takes the size as it is)
    ProfScope prof_scope(h, RCG_KERNEL_ACTOR);
    void* args[] = {&A, &P};
    rc = launch(h, f, L.grid, L.block, L.lds, args);
    if (rc == RCG_OK) note_launch(h, RCG_KERNEL_ACTOR, RCG_KID_ACTOR_OPT, L.variant | (loop ? 8 : 0), OPT_G);
    return rc;
  });
}

// ---- the critic entry points: op_critic, op_critic_cost and op_critic_update (rcg_sysops.hpp) on the critic program -----------
int rtc_critic(rcg_handle* h, const void* obs, const void* act, const void* w, void* out, int32_t n) {
  if (!h->rtc->dims.has_critic) return refuse(h, "rcg_critic");
  return by_dtype(h, [&](auto r) {
    using real = decltype(r);
    hipFunction_t f;
    int rc = critic_function<real>(h, fit_form_of(h->cfg.n_critic - 1, h->dc, false), CRITIC_VALUE, &f);
    if (rc) return rc;
    const real* o = (const real*)obs;
    const real* a = (const real*)act;
    const real* ww = (const real*)w;
    real* y = (real*)out;
    long nn = n;
    KParams<real> P = params<real>(h);
    void* args[] = {&o, &a, &ww, &y, &nn, &P};
    return launch(h, f, dim3(blocks_for(n)), dim3(256), 0, args);
  });
}

int rtc_critic_cost(rcg_handle* h, const void* w, void* Jc) {
  if (!h->rtc->dims.has_critic) return refuse(h, "rcg_critic_cost");
  return by_dtype(h, [&](auto r) {
    using real = decltype(r);
    hipFunction_t f;
    int rc = critic_function<real>(h, fit_form_of(h->cfg.n_critic - 1, h->dc, false), CRITIC_COST, &f);
    if (rc) return rc;
    const real* ww = w ? (const real*)w : (const real*)h->f[RCG_FIELD_W_CRITIC];
    const real* wp = (const real*)h->f[RCG_FIELD_W_PREV];
    const real* ob = (const real*)h->f[RCG_FIELD_OBS_BUF];
    const real* ab = (const real*)h->f[RCG_FIELD_ACT_BUF];
    real* jc = (real*)Jc;
    KParams<real> P = params<real>(h);
    void* args[] = {&ww, &wp, &ob, &ab, &jc, &P};
    return launch(h, f, dim3(blocks_for(h->cfg.batch)), dim3(256), 0, args);
  });
}

int rtc_critic_update(rcg_handle* h, int32_t n_substeps, int32_t do_push, int32_t do_fit) {
  if (!h->rtc->dims.has_critic) return refuse(h, "the critic update");
  return by_dtype(h, [&](auto r) {
    using real = decltype(r);
    // the form, the grid and the variant word of op_critic_update; the function is resolved before the scratch tensor of
    // k_critic_fit_gen is sized and before anything is enqueued
    hipFunction_t f;
    int rc = critic_fit_function(h, &f);
    if (rc) return rc;
    ProfScope prof_scope(h, RCG_KERNEL_CRITIC);
    FitArgs<real> F;
    FitPlan L;
    rc = fit_plan<real>(h, n_substeps, do_push, do_fit, false, F, L);
    if (rc) return rc;
    KParams<double> P64 = h->p64;
    KParams<real> P = params<real>(h);
    double* scratch = (double*)h->fit_scratch;
    void* args[] = {&F, &P64, &P, &scratch};  // (the fourth is k_critic_fit_gen's alone)
    rc = launch(h, f, L.grid, L.block, 0, args);
    if (rc == RCG_OK) note_launch(h, RCG_KERNEL_CRITIC, RCG_KID_CRITIC_FIT, L.variant, L.epw);
    return rc;
  });
}
// The nominal law of a policy with the member `nominal`: k_nominal with the law behind Nominal<RcgRtcSys>, a program of its own per
// element type compiled on first use (<name>_nominal.hip), and k_ticks_nominal, the instance of an (element type, target setting)
// in the Ticks unit (<name>_ticks_nominal.hip).  The entry points have refused and resolved through rtc_prepare_nominal.
template <typename real>
int nominal_function(rcg_handle* h, hipFunction_t* fn) {
  return lazy_function(h, Unit::Nominal, "nominal", {expr_nominal<real>()}, 0, fn);
}
int rtc_nominal(rcg_handle* h, const void* obs, void* action, void* lyap, void* theta, int32_t n, double gain, const double* ctrl_pars,
                int32_t clip, bool tick) {
  const RtcDims& d = h->rtc->dims;
  if (!(d.nominal & 1)) return refuse_opt_in(h, "the nominal controller", "the member nominal");
  return by_dtype(h, [&](auto r) {
    using real = decltype(r);
    hipFunction_t f;
    int rc = nominal_function<real>(h, &f);
    if (rc) return rc;
    const rcg_cfg& c = h->cfg;
    NomArgs<real> A;
    memset(&A, 0, sizeof A);
    A.obs = (const real*)obs;
    A.action = (real*)action;
    A.lyap = (real*)lyap;
    A.theta = (real*)theta;
    A.accum = (tick && !(c.flags & RCG_FLAG_ACCUM_EVERY_SUBSTEP)) ? (real*)h->f[RCG_FIELD_ACCUM] : nullptr;
    A.step_idx = tick ? (int32_t*)h->f[RCG_FIELD_STEP_IDX] : nullptr;
    A.n = n;
    A.gain = gain;
    A.clip = clip;
    A.obs_x = (tick && d.has_out) ? 1 : 0;  // a tick observes out(STATE)
    A.pars_env = pars_env_of<real>(h, n);
    A.c[0] = gain;
    for (int i = 0; i < d.nominal_np; ++i) A.c[1 + i] = ctrl_pars[i];
    KParams<real> P = params<real>(h);
    ProfScope prof_scope(h, RCG_KERNEL_ACTOR);
    void* args[] = {&A, &P};
    rc = launch(h, f, dim3(blocks_for(n)), dim3(256), 0, args);
    if (rc == RCG_OK) note_launch(h, RCG_KERNEL_ACTOR, RCG_KID_NOMINAL, 0, 64);
    return rc;
  });
}
int rtc_ticks_nominal(rcg_handle* h, int32_t T, double gain, const double* ctrl_pars) {
  const RtcDims& d = h->rtc->dims;
  if (!(d.nominal & 1)) return refuse_opt_in(h, "rcg_control_ticks_nominal", "the member nominal");
  if (!d.has_ticks) return refuse_opt_in(h, "rcg_control_ticks_nominal", "TICKS");
  return by_dtype(h, [&](auto r) {
    using real = decltype(r);
    TicksNomArgs<real> A;
    TicksNomPlan L;
    ticks_nominal_plan<real>(h, T, gain, A, L);
    for (int i = 0; i < d.nominal_np; ++i) A.c[1 + i] = ctrl_pars[i];
    hipFunction_t f;
    int rc = lazy_function(h, Unit::Ticks, "ticks_nominal", {expr_ticks_nominal<real>(L.tgt)}, 0, &f);
    if (rc) return rc;
    KParams<real> P = params<real>(h);
    ProfScope prof_scope(h, RCG_KERNEL_ACTOR);
    void* args[] = {&A, &P};
    rc = launch(h, f, L.grid, L.block, 0, args);
    if (rc == RCG_OK) note_launch(h, RCG_KERNEL_ACTOR, RCG_KID_NOMINAL, 1, 64);
    return rc;
  });
}
// T ticks in one launch: op_ticks' / op_ticks_mem's plan (ticks_plan, ticks_mem_plan) on the program compiled for its instance -
// except the shell written for one built-in system (k_ticks_pk).  The instance is resolved - and compiled, the first time -
// before anything is enqueued.
int rtc_ticks(rcg_handle* h, int32_t T, int32_t K, const void* cand) {
  if (!h->rtc->dims.has_ticks) return refuse_opt_in(h, "rcg_control_ticks", "TICKS");
  return by_dtype(h, [&](auto r) {
    using real = decltype(r);
    const RtcSystem& S = *h->rtc;
    TicksArgs<real> A;
    TicksPlan L;
    int rc = ticks_plan<real>(h, S.dims.du, T, K, cand, A, L);
    if (rc) return rc;
    hipFunction_t f;
    rc = lazy_function(h, Unit::Ticks, "ticks", {expr_ticks<real>(L)}, 0, &f);
    if (rc) return rc;
    KParams<real> P = params<real>(h);
    ProfScope prof_scope(h, RCG_KERNEL_ACTOR);
    // (an LDS request beyond 64 KB - the rows of four waves resident for all T ticks - goes into the module launch as it is,
    // as k_actor_dma's does: rtc_optimize)
    void* args[] = {&A, &P};
    rc = launch(h, f, L.grid, L.block, L.lds, args);
    if (rc == RCG_OK) note_launch(h, RCG_KERNEL_ACTOR, RCG_KID_TICKS, L.variant, A.G);
    return rc;
  });
}
int rtc_ticks_mem(rcg_handle* h, int32_t T, int32_t K, const void* cand) {
  if (!h->rtc->dims.has_ticks) return refuse_opt_in(h, "rcg_control_ticks", "TICKS");
  if (!h->rtc->dims.has_critic) return refuse_opt_in(h, "rcg_control_ticks", "CRITIC");
  return by_dtype(h, [&](auto r) {
    using real = decltype(r);
    const RtcSystem& S = *h->rtc;
    TicksMemArgs<real> M;
    TicksMemPlan L;
    int rc = ticks_mem_plan<real>(h, S.dims.du, S.tgt, true, T, K, cand, M, L);
    if (rc) return rc;
    hipFunction_t f;
    rc = lazy_function(h, Unit::Ticks, "ticks_mem", {expr_ticks_mem<real>(L)}, 0, &f);
    if (rc) return rc;
    KParams<double> P64 = h->p64;
    KParams<real> P = params<real>(h);
    ProfScope prof_scope(h, RCG_KERNEL_ACTOR);
    void* args[] = {&M, &P64, &P};
    rc = launch(h, f, L.grid, L.block, L.lds, args);
    if (rc == RCG_OK) note_launch(h, RCG_KERNEL_ACTOR, RCG_KID_TICKS, L.variant, M.A.G);
    return rc;
  });
}
// closed_loop_rhs on the full state [state, disturb], noise given: op_rhs_full on the disturb program (rcg_rhs_full has checked
// RCG_FLAG_DISTURB, which rcg_create grants a policy with DD / disturb only)
int rtc_rhs_full(rcg_handle* h, const void* state, const void* disturb, const void* action, const void* xi, void* dstate,
                 void* ddisturb, void* clipped, int32_t n, int32_t clip) {
  if (h->rtc->dims.dd < 1) return refuse(h, "rcg_rhs_full");
  return by_dtype(h, [&](auto r) {
    using real = decltype(r);
    hipFunction_t f;
    int rc = disturb_function<real>(h, DISTURB_RHS_FULL, &f);
    if (rc) return rc;
    const real* st = (const real*)state;
    const real* q = (const real*)disturb;
    const real* ac = (const real*)action;
    const real* x = (const real*)xi;
    real* ds = (real*)dstate;
    real* dq = (real*)ddisturb;
    real* cl = (real*)clipped;
    const real* pe = pars_env_of<real>(h, n);
    long nn = n;
    int ci = clip;
    DisturbPars D = disturb_pars(h);
    KParams<real> P = params<real>(h);
    void* args[] = {&st, &q, &ac, &x, &ds, &dq, &cl, &pe, &nn, &ci, &D, &P};
    return launch(h, f, dim3(blocks_for(n)), dim3(256), 0, args);
  });
}
// The device search: op_search's plan (search_plan) on the program compiled for its instance.  The instance is resolved - and
// compiled, the first time - before anything is enqueued.
int rtc_search(rcg_handle* h, int32_t K, int32_t rounds, int32_t round0, const void* obs, const void* state_sys, const void* centre,
               int shift, void* u_best, void* action, void* best_J, int32_t* best_idx, bool tick, bool sim_first) {
  if (!h->rtc->dims.has_search) return refuse_opt_in(h, "rcg_actor_search", "SEARCH");
  return by_dtype(h, [&](auto r) {
    using real = decltype(r);
    const RtcSystem& S = *h->rtc;
    SearchArgs<real> A;
    SearchPlan L;
    int rc = search_plan<real>(h, S.dims.du, S.tgt, K, rounds, round0, obs, state_sys, centre, shift, u_best, action, best_J,
                               best_idx, tick, A, L);
    if (rc) return rc;
    hipFunction_t f;
    rc = search_function<real>(h, L, &f);
    if (rc) return rc;
    if (tick && sim_first) {
      rc = sim_step<real>(h, h->cfg.substeps_per_tick);
      if (rc) return rc;
    }
    KParams<real> P = params<real>(h);
    ProfScope prof_scope(h, RCG_KERNEL_ACTOR);
    void* args[] = {&A, &P};
    rc = launch(h, f, L.grid, L.block, L.lds, args);
    if (rc == RCG_OK) note_launch(h, RCG_KERNEL_ACTOR, RCG_KID_ACTOR_SEARCH, L.variant, 1);
    return rc;
  });
}
// rcg_loop_step's glue kernel: op_loop's arguments (fill_loop_args) and grid on the loop program's k_loop
int rtc_loop(rcg_handle* h, const double* act_in, int32_t n_substeps, int32_t do_sim, int32_t do_tail, int32_t decided, int32_t dc,
             double* out, double* flag, double seq) {
  if (!h->rtc->dims.has_loop) return refuse_opt_in(h, "rcg_loop_step", "LOOP");
  return by_dtype(h, [&](auto r) {
    using real = decltype(r);
    hipFunction_t f;
    int rc = loop_function<real>(h, LOOP_GLUE, &f);
    if (rc) return rc;
    LoopArgs<real> A;
    fill_loop_args<real>(h, A, act_in, n_substeps, do_sim, do_tail, decided, dc, out, flag, seq);
    KParams<real> P = params<real>(h);
    void* args[] = {&A, &P};
    return launch(h, f, dim3(blocks_for(h->cfg.batch, 64)), dim3(64), 0, args);
  });
}

// the probe program: which optional members the policy has (the values travel in the lowered name of an empty kernel:
// k_rtc_probe<TGT, JAC, DY, OUT, OJAC, CRIT, SRCH, TCK, ZW, DD, LP, AD> mangles its arguments as Lb0E / Lb1E, Li<n>E / Lin<n>E and Lj<n>E;
// DD: the policy's DD when it has `disturb`, else 0; LP: the policy's LOOP; AD: its AUTODIFF)
int probe(RtcSystem& S, std::string* log) {
  const std::string pol = "rcg::" + S.name;
  const std::string e = std::string("rcg::rtc::k_rtc_probe<") + kSysExpr + "::TGT, rcg::rtc::jac<" + pol + ">::v, " + kSysExpr +
                        "::DY, " + kSysExpr + "::HAS_OUT, rcg::rtc::ojac<" + pol + ">::v, rcg::rtc::crit<" + pol + ">::v, rcg::rtc::srch<" + pol +
                        ">::v, rcg::rtc::tck<" + pol + ">::v, " + kSysExpr + "::ZW_PRESET, rcg::rtc::ddv<" + pol + ">::v, rcg::rtc::lp<" + pol + ">::v, rcg::rtc::ad<" + pol + ">::v, (rcg::rtc::nom<" + pol +
                        ">::v ? 1 : 0) | (rcg::rtc::nomlf<" + pol + ">::v ? 2 : 0), rcg::rtc::nomnp<" + pol + ">::v>";
  RtcProgram P;
  const int rc = compile(unit_source(S, Unit::Core), S.name + "_probe.hip", {e}, &P, log);
  if (rc) return rc;
  const std::string& low = P.lowered[e];
  long v[14];
  size_t p = low.find("IL");
  int n = 0;
  for (p = p == std::string::npos ? p : p + 1; p != std::string::npos && n < 14 && p + 2 < low.size() && low[p] == 'L'; ++n) {
    const char t = low[p + 1];
    size_t q = p + 2;
    const bool neg = t == 'i' && low[q] == 'n';
    if (neg) ++q;
    long x = 0;
    while (q < low.size() && isdigit((unsigned char)low[q])) x = 10 * x + (low[q++] - '0');
    if ((t != 'b' && t != 'i' && t != 'j') || q >= low.size() || low[q] != 'E') break;
    v[n] = neg ? -x : x;
    p = q + 1;
  }
  if (n != 14) {
    *log = "cannot read the probe instance " + low;
    return RCG_ERR_HIP;
  }
  S.tgt = v[0] != 0;
  S.dims.has_jac = v[1] != 0;
  S.dims.dy = (int)v[2];
  S.dims.has_out = v[3] != 0;
  S.dims.has_out_jac = S.dims.has_out && v[4] != 0;
  S.dims.has_critic = v[5] != 0;
  S.dims.has_search = v[6] != 0;
  S.dims.has_ticks = v[7] != 0;
  S.zw = (unsigned)v[8];
  S.dims.dd = (int)v[9];
  S.dims.has_loop = v[10] != 0;
  // AUTODIFF: a member the policy does not write is derived (the adapter's mixins), and counts as one it has from here on
  const bool ad = v[11] != 0;
  S.dims.autodiff = (ad && !S.dims.has_jac ? 1 : 0) | (ad && S.dims.has_out && !S.dims.has_out_jac ? 2 : 0);
  S.dims.has_jac = S.dims.has_jac || ad;
  S.dims.has_out_jac = S.dims.has_out_jac || (S.dims.has_out && ad);
  S.dims.nominal = (int)v[12];
  S.dims.nominal_np = (int)v[13];
  return RCG_OK;
}

}  // namespace

#if !defined(__HIP_DEVICE_COMPILE__)  // (the table of host function pointers exists in the host pass only)
const SysVTable kVtRtc = {&rtc_rhs,     &rtc_stage_obj, &rtc_critic,   &rtc_critic_cost, &rtc_actor,
                          &rtc_sim_step, &rtc_critic_update, &rtc_optimize, &rtc_nominal, &rtc_ticks,
                          &rtc_rhs_full, &rtc_search,    &rtc_ticks_mem, &rtc_loop, &rtc_jac_T, &rtc_ticks_nominal};
#endif

int rtc_out(rcg_handle* h, const void* state, void* obs, int32_t n) {
  return by_dtype(h, [&](auto r) {
    using real = decltype(r);
    hipFunction_t f;
    int rc = core_function<real>(h, expr_out<real>(), &f);
    if (rc) return rc;
    const real* st = (const real*)state;
    real* y = (real*)obs;
    const real* pe = pars_env_of<real>(h, n);
    long nn = n;
    KParams<real> P = params<real>(h);
    void* args[] = {&st, &y, &pe, &nn, &P};
    return launch(h, f, dim3(blocks_for(n)), dim3(256), 0, args);
  });
}

// rcg_control_tick, RQL / SQL: every instance the tick launches - the critic program's fit kernel and the decision kernel of this
// (cand, K) - resolved, and compiled on first use, before the tick enqueues anything
int rtc_prepare_tick(rcg_handle* h, const void* cand, int32_t K) {
  if (!h->rtc->dims.has_critic) return refuse_opt_in(h, "rcg_control_tick", "CRITIC");
  hipFunction_t fit;
  int rc = critic_fit_function(h, &fit);
  if (rc) return rc;
  return by_dtype(h, [&](auto r) {  // the tick's own plan (the arguments rcg_control_tick hands the launcher), and its instance
    using real = decltype(r);
    const RtcSystem& S = *h->rtc;
    ActorArgs<real> A;
    ActorPlan L;
    int rc2 = actor_plan<real>(h, "rcg_control_tick", S.dims.ds, S.dims.du, S.tgt, cand, K, nullptr, nullptr, nullptr, nullptr,
                               h->f[RCG_FIELD_ACTION], h->f[RCG_FIELD_BEST_J], (int32_t*)h->f[RCG_FIELD_BEST_IDX], true, false, A, L);
    if (rc2) return rc2;
    ActorPick pick;
    return resolve_actor_instance<real>(h, A, L, cand != nullptr, &pick);
  });
}

// rcg_control_tick_search: the refusal of a policy without SEARCH, then every instance the tick launches - the search instance of
// the tick's own plan and, RQL / SQL, the critic program's fit kernel - resolved, and compiled on first use, before the tick
// enqueues anything: a compile failure leaves every field of the handle as it was
int rtc_prepare_tick_search(rcg_handle* h, int32_t K, int32_t rounds, int32_t warm) {
  if (!h->rtc->dims.has_search) return refuse_opt_in(h, "rcg_control_tick_search", "SEARCH");
  if (h->cfg.mode != RCG_MODE_MPC) {
    if (!h->rtc->dims.has_critic) return refuse_opt_in(h, "rcg_control_tick_search", "CRITIC");
    hipFunction_t fit;
    const int rc = critic_fit_function(h, &fit);
    if (rc) return rc;
  }
  return by_dtype(h, [&](auto r) {
    using real = decltype(r);
    const RtcSystem& S = *h->rtc;
    SearchArgs<real> A;
    SearchPlan L;
    void* sqn = h->f[RCG_FIELD_ACTION_SQN];
    int rc = search_plan<real>(h, S.dims.du, S.tgt, K, rounds, 0, nullptr, nullptr, warm ? sqn : nullptr, warm ? 1 : 0, sqn,
                               h->f[RCG_FIELD_ACTION], h->f[RCG_FIELD_BEST_J], (int32_t*)h->f[RCG_FIELD_BEST_IDX], true, A, L);
    if (rc) return rc;
    hipFunction_t f;
    return search_function<real>(h, L, &f);
  });
}

// rcg_control_tick_opt, RQL / SQL: the optimiser's own refusals and the critic program, before the critic phase enqueues anything
// (the optimiser's instances belong to the core programs compiled at registration)
int rtc_prepare_tick_opt(rcg_handle* h) {
  const RtcDims& d = h->rtc->dims;
  if (!d.has_critic) return refuse_opt_in(h, "rcg_control_tick_opt", "CRITIC");
  if (!d.has_jac || (d.has_out && !d.has_out_jac))
    return rcg_fail(h, RCG_ERR_UNSUPPORTED, "rcg_control_tick_opt: the policy %s defines no jac_T%s (the optimiser's adjoint sweep)",
                    h->rtc->name.c_str(), d.has_out ? " / out_jac_T" : "");
  hipFunction_t fit;
  return critic_fit_function(h, &fit);
}

int rtc_prepare_nominal(rcg_handle* h, const char* who, bool want_lyap, const double* ctrl_pars, int ticks) {
  const RtcDims& d = h->rtc->dims;
  if (!(d.nominal & 1)) return refuse_opt_in(h, who, "the member nominal");
  if (want_lyap && !(d.nominal & 2))
    return rcg_fail(h, RCG_ERR_UNSUPPORTED, "%s: the policy %s defines no nominal_lf (the Lyapunov function of its nominal law)", who,
                    h->rtc->name.c_str());
  if (d.nominal_np > 0 && !ctrl_pars)
    return rcg_fail(h, RCG_ERR_BAD_ARG, "%s: ctrl_pars must point to the %d controller parameters of %s (NOMINAL_NP)", who,
                    d.nominal_np, h->rtc->name.c_str());
  return by_dtype(h, [&](auto r) {
    using real = decltype(r);
    hipFunction_t f;
    if (ticks < 2) return nominal_function<real>(h, &f);
    if (!d.has_ticks) return refuse_opt_in(h, who, "TICKS");
    return lazy_function(h, Unit::Ticks, "ticks_nominal", {expr_ticks_nominal<real>((h->cfg.flags & RCG_FLAG_HAS_TARGET) != 0)}, 0, &f);
  });
}

int rtc_loop_refusals(rcg_handle* h, bool decide) {
  const RtcDims& d = h->rtc->dims;
  if (!d.has_loop) return refuse_opt_in(h, "rcg_loop_step", "LOOP");
  if (decide && !d.has_jac)
    return rcg_fail(h, RCG_ERR_UNSUPPORTED, "rcg_loop_step: RCG_LOOP_DECIDE needs jac_T in the policy %s (the optimiser's adjoint sweep)",
                    h->rtc->name.c_str());
  if (decide && d.has_out && !d.has_out_jac)
    return rcg_fail(h, RCG_ERR_UNSUPPORTED,
                    "rcg_loop_step: RCG_LOOP_DECIDE needs out_jac_T in the policy %s (it defines out: the adjoint of its output map)",
                    h->rtc->name.c_str());
  return RCG_OK;
}

int rtc_prepare_loop(rcg_handle* h, bool push) {
  hipFunction_t f;
  int rc = by_dtype(h, [&](auto r) { return loop_function<decltype(r)>(h, LOOP_GLUE, &f); });
  if (rc || !push) return rc;
  if (!h->rtc->dims.has_critic) return refuse_opt_in(h, "rcg_loop_step", "CRITIC");
  return critic_fit_function(h, &f);
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
  S->dims.ds = ds;
  S->dims.du = du;
  S->dims.np = np;
  S->dims.dy = ds;  // (the probe reads the policy's own DY and its optional members)
  S->tgt = false;
  std::string log;
  rc = probe(*S, &log);
  // dim_output: chi = [y - target, u] must fit RCG_MAX_CHI and the target KParams::target (a DY other than DS without `out` is
  // refused by the adapter's static_assert above, with hipRTC's log)
  if (rc == RCG_OK && (S->dims.dy < 1 || S->dims.dy > RCG_MAX_DS))
    return rcg_fail(nullptr, RCG_ERR_UNSUPPORTED, "rcg_register_system: %s::DY = %d beyond 1 .. %d", name, S->dims.dy, RCG_MAX_DS);
  // dim_disturb: DisturbPars, rcg_cfg::pars_disturb / disturb_init and the two normals of a Philox draw are sized for 2
  if (rc == RCG_OK && (S->dims.dd < 0 || S->dims.dd > 2))
    return rcg_fail(nullptr, RCG_ERR_UNSUPPORTED, "rcg_register_system: %s::DD = %d beyond 1 .. 2", name, S->dims.dd);
  // NOMINAL_NP: NomArgs::c / TicksNomArgs::c hold the gain and NOM_MAX_NP parameters
  if (rc == RCG_OK && (S->dims.nominal_np < 0 || S->dims.nominal_np > NOM_MAX_NP))
    return rcg_fail(nullptr, RCG_ERR_UNSUPPORTED, "rcg_register_system: %s::NOMINAL_NP = %d beyond 0 .. %d", name, S->dims.nominal_np,
                    NOM_MAX_NP);
  const std::string unit = unit_source(*S, Unit::Core);
  if (rc == RCG_OK) rc = compile(unit, S->name + "_f32.hip", core_exprs<float>(S->dims), &S->core[0], &log);
  if (rc == RCG_OK) rc = compile(unit, S->name + "_f64.hip", core_exprs<double>(S->dims), &S->core[1], &log);
  if (rc) {
    rcg_set_thread_error(std::string("rcg_register_system: ") + name + ": " + log);
    return rc;
  }
  for (const auto& e : core_exprs<float>(S->dims)) S->compiled.push_back(S->name + "_f32.hip\t" + e);
  for (const auto& e : core_exprs<double>(S->dims)) S->compiled.push_back(S->name + "_f64.hip\t" + e);
  std::lock_guard<std::mutex> lock(g_mu);
  if (known(&rc)) return rc;
  S->id = RCG_SYS_USER_BASE + (int)g_sys.size();
  *sys_id = S->id;
  g_sys.push_back(std::move(S));
  return RCG_OK;
}

int rcg_system_programs(int32_t sys_id, char* buf, int64_t cap, int64_t* need) {
  std::lock_guard<std::mutex> lock(g_mu);
  const int i = sys_id - RCG_SYS_USER_BASE;
  if (i < 0 || i >= (int)g_sys.size()) return rcg_fail(nullptr, RCG_ERR_BAD_ARG, "rcg_system_programs: bad sys_id %d", sys_id);
  std::string text;
  for (const auto& line : g_sys[i]->compiled) text += line + "\n";
  if (need) *need = (int64_t)text.size() + 1;
  if (buf && cap > 0) {
    const size_t n = text.size() < (size_t)cap - 1 ? text.size() : (size_t)cap - 1;
    memcpy(buf, text.data(), n);
    buf[n] = '\0';
  }
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
