// The library core and the convolutions of libgennet_hip.so.  Core: the error text, the launch check, the profiling events, the library
// switches and the RNG base of a captured step.  Convolutions: argument checking, tap-table construction and the kernel-family selection of
// every Conv1D and Dense entry point (select_conv / select_dgrad / select_wgrad: one table below); a Dense layer is the 1-tap conv.  Every
// other entry point of include/gennet_hip.h is defined beside its kernels, in the file that holds them.  No torch types, no allocation, no
// synchronisation.
#include <stdarg.h>
#include <algorithm>
#include <mutex>
#include <vector>
#include <stdlib.h>
#include "common.h"

namespace gn {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s: %s", what, hipGetErrorString(e));
    return GN_ELAUNCH;
  }
  return GN_OK;
}

// ---- profiling: HIP events around the MFMA launches, on the stream they are launched on ------------------
struct ProfRec {
  hipEvent_t a, b;
  double flop;
  int kind;
  double bytes;
};
static bool g_prof_on = false;
static std::vector<ProfRec> g_prof;
static std::vector<hipEvent_t> g_pool;
static hipEvent_t g_cur;
static std::mutex g_prof_mu;

static hipEvent_t get_event() {
  if (!g_pool.empty()) {
    hipEvent_t e = g_pool.back();
    g_pool.pop_back();
    return e;
  }
  hipEvent_t e;
  (void)hipEventCreate(&e);
  return e;
}

static thread_local const uint64_t* g_rng_base = nullptr;
const uint64_t* rng_base() { return g_rng_base; }

void prof_begin(hipStream_t s) {
  if (!g_prof_on) return;
  g_cur = get_event();
  (void)hipEventRecord(g_cur, s);
}

void prof_end(hipStream_t s, double flop, int kind, double bytes) {
  if (!g_prof_on) return;
  hipEvent_t b = get_event();
  (void)hipEventRecord(b, s);
  std::lock_guard<std::mutex> lk(g_prof_mu);
  g_prof.push_back({g_cur, b, flop, kind, bytes});
}

const Switches& switches() {
  static const Switches sw = [] {
    auto on = [](const char* name) { return getenv(name) != nullptr; };
    const char* gflop = getenv("GN_BF16X3_MIN_GFLOP");
    return Switches{on("GN_CONV_NOPIPE"),  on("GN_CONV_NODMA"),   on("GN_CONV_NOMERGE"),    on("GN_CONV_NONARROW"), on("GN_CONV_NOPATCH"),
                    on("GN_WGRAD_NOPIPE"), on("GN_BF16X3_NO_MERGE"), gflop ? atof(gflop) : 50.0};
  }();
  return sw;
}

// ---- kernel-family selection ----------------------------------------------------------------------------------------------------------------
// Conv arithmetic (gn_set_conv_math): 0 = direct fp32 MFMA kernels only; 1 = opt-in bf16 x 3 operand split; 2 = transform-domain fp32 (the
// engine's default).  select_conv (forward, each phase of a data gradient, Dense data gradient), select_dgrad (the merged stride-2 data gradient)
// and select_wgrad decide the family from the launch's shape, the conv math and the switches alone -- never from a workspace size -- so forward,
// data gradient and weight gradient of a layer use the same arithmetic.  The launch code then checks that the workspace holds what the chosen
// family needs (GN_EWORKSPACE with the size otherwise) and never re-selects.
//
//   family   directions (math)      shape rule, besides the kernel's own *_supported / *_kind           workspace (conv-math | caller's)
//   small    fwd, dgrad, wgrad      Cin <= 4 or Cout <= 4                                               - | wgrad_small_workspace_bytes
//   wino     fwd, wgrad (2)         5 taps, stride 1, Cin >= 32 (fwd); 6 Cin Cout floats <= 64 MiB      6 Cin Cout floats | wgrad_wino_workspace_bytes
//   wino_s2  fwd, dgrad, wgrad (2)  5 taps, stride 2; 7 Cin Cout floats <= 64 MiB                       7 Cin Cout floats | wgrad_wino_s2_workspace_bytes
//   bf16x3   fwd, dgrad, wgrad (1)  Cin, Cout >= 256 and GN_BF16X3_MIN_GFLOP (split_worth_it)          the split operands | wgrad_workspace_bytes
//   merged   dgrad                  stride 2, 5 taps, few tiles; not bf16x3, NOMERGE, NOPIPE or NODMA   - | -
//   direct   everything else        conv_mfma_dispatch / wgrad_mfma_dispatch pick tile and member       - | wgrad_workspace_bytes
//   anyc     fwd, dgrad, wgrad      the _any entry points only (any_channels) and needs_any(Cin, Cout):   - | wgrad_anyc_workspace_bytes
//            (every math)           the pairs every family above refuses; a strided data gradient
//                                   runs as phases, each one anyc launch
static int g_conv_math = 0;
static void* g_conv_ws = nullptr;
static size_t g_conv_ws_bytes = 0;
constexpr size_t kWinoKernelBytes = 64ull << 20;      // largest transformed kernel of the transform-domain families = the workspace math 2 needs

// Size gate of the opt-in split, the one predicate for all its launches.  The split pass costs ~10 bytes per input element per launch, the conv
// gains ~0.02 ps per element and output channel, so small-Cout layers gain little and small-Cin layers (few K chunks) lose to the prologue; below
// ~50 GFLOP a launch does not keep the 256-row blocks of the split kernels busy for more than a round or two and the split pass in front of it is
// pure latency (at the reference script's own batch 8 every launch is below it: the opt-in then changes nothing there instead of costing 1 %).
static bool split_worth_it(int B, int M, int ntaps, int Cin, int Cout) {
  constexpr int min_cin = 256, min_cout = 256;
  return Cin >= min_cin && Cout >= min_cout && 2.0 * B * (double)M * ntaps * Cin * Cout >= switches().bf16x3_min_gflop * 1e9;
}
// ... of a forward / data-gradient launch; w_taps > 0: a phase (or both) of a w_taps-tap layer's strided data gradient, decided on the whole layer
static bool split_worth_it(const ConvArgs& a, int w_taps) {
  return w_taps > 0 ? split_worth_it(a.B, (a.Ly + 1) / 2, w_taps, a.Cin, a.Cout) : split_worth_it(a.B, a.M, a.t.ntaps, a.Cin, a.Cout);
}

// The channel pairs that end in an error on every family above, read off the dispatchers themselves: Cin <= 4 goes to the small-Cin kernels
// whatever Cout is, and they need Cout % 4 == 0 (so 4 -> 3 is refused although 3 <= 4); otherwise Cout <= 4 goes to the small-Cout kernels,
// which need Cin % 4 == 0; everything else needs both counts multiples of 4.  The weight gradient picks its small side the same way.  A data
// gradient runs the swapped pair, so a layer may need the anyc kernels in one direction only (3 -> 4: forward strict, data gradient 4 -> 3 not).
// Without the any_channels flag of the _any entry points such pairs still end in that error.
static bool needs_any(int Cin, int Cout) {
  const bool strict = Cin <= 4 ? Cout % 4 == 0 : Cout <= 4 ? Cin % 4 == 0 : (Cin % 4 == 0 && Cout % 4 == 0);
  return !strict;
}

enum ConvFamily { CONV_SMALL, CONV_WINO, CONV_WINO_S2, CONV_BF16X3, CONV_DIRECT, CONV_ANYC };

// forward, one data-gradient phase, Dense data gradient
static ConvFamily select_conv(const ConvArgs& a, int w_taps) {
  if (a.any_channels && needs_any(a.Cin, a.Cout)) return CONV_ANYC;
  if (a.Cin <= 4 || a.Cout <= 4) return CONV_SMALL;
  if (g_conv_math == 2 && a.Cin >= 32 && conv_wino_supported(a) && conv_wino_workspace_bytes(a.Cin, a.Cout) <= kWinoKernelBytes) return CONV_WINO;
  if (g_conv_math == 2 && conv_wino_s2_kind(a) == 1 && conv_wino_s2_workspace_bytes(a.Cin, a.Cout) <= kWinoKernelBytes) return CONV_WINO_S2;      // stride-2 forward: F(2,3) + F(2,2)
  if (g_conv_math == 1 && split_worth_it(a, w_taps) && conv_bf16x3_supported(a)) return CONV_BF16X3;
  return CONV_DIRECT;
}

enum DgradFamily { DGRAD_WINO_S2, DGRAD_BF16X3_MERGED, DGRAD_MERGED, DGRAD_PHASES };

// the data gradient of a stride-2, 5-tap layer; a = its merged two-phase form (dgrad_impl).  DGRAD_PHASES: one select_conv launch per phase
static DgradFamily select_dgrad(const ConvArgs& a) {
  if (a.any_channels && needs_any(a.Cin, a.Cout)) return DGRAD_PHASES;
  if (a.Ly < 2 || a.Cin <= 4 || a.Cout <= 4) return DGRAD_PHASES;
  if (g_conv_math == 2 && conv_wino_s2_kind(a) == 2 && conv_wino_s2_workspace_bytes(a.Cin, a.Cout) <= kWinoKernelBytes) return DGRAD_WINO_S2;      // both phases, F(2,3) and F(2,2)
  const Switches& sw = switches();
  const bool split = g_conv_math == 1 && split_worth_it(a, 5);
  if (split) return !sw.bf16x3_no_merge && conv_bf16x3_merged_kind(a) ? DGRAD_BF16X3_MERGED : DGRAD_PHASES;
  // the merged member of the pipelined LDS-DMA family: every switch that takes that family out takes it out too
  if (!sw.conv_nomerge && !sw.conv_nopipe && !sw.conv_nodma && conv_pipe_merged_supported(a)) return DGRAD_MERGED;
  return DGRAD_PHASES;
}

enum WgradFamily { WGRAD_SMALL, WGRAD_WINO, WGRAD_WINO_S2, WGRAD_BF16X3, WGRAD_DIRECT, WGRAD_ANYC };

static WgradFamily select_wgrad(const WgradArgs& a) {
  if (a.any_channels && needs_any(a.Cin, a.Cout)) return WGRAD_ANYC;
  if (a.Cin <= 4 || a.Cout <= 4) return WGRAD_SMALL;
  if (g_conv_math == 2 && wgrad_wino_supported(a) && conv_wino_workspace_bytes(a.Cin, a.Cout) <= kWinoKernelBytes) return WGRAD_WINO;
  if (g_conv_math == 2 && wgrad_wino_s2_supported(a) && conv_wino_s2_workspace_bytes(a.Cin, a.Cout) <= kWinoKernelBytes) return WGRAD_WINO_S2;
  if (g_conv_math == 1 && split_worth_it(a.B, a.M, a.ntaps, a.Cin, a.Cout) && wgrad_bf16x3_supported(a)) return WGRAD_BF16X3;
  return WGRAD_DIRECT;
}

// what the weight-gradient family needs of the CALLER's workspace (the bias-gradient pass needs bias_grad_ws on top, not beside)
static size_t wgrad_ws_need(WgradFamily f, const WgradArgs& a) {
  switch (f) {
    // (a pair the small kernels refuse -- reached only without any_channels: its size has no meaning (a large side below 4 divides by zero in
    //  it) and wgrad_small_dispatch refuses the pair before it looks at the workspace)
    case WGRAD_SMALL: return needs_any(a.Cin, a.Cout) ? 0 : wgrad_small_workspace_bytes(a.B, a.M, a.Cin, a.Cout, a.ntaps);
    case WGRAD_WINO: return wgrad_wino_workspace_bytes(a.B, a.M, a.Cin, a.Cout);          // six point slabs per split
    case WGRAD_WINO_S2: return wgrad_wino_s2_workspace_bytes(a.B, a.M, a.Cin, a.Cout);    // seven
    case WGRAD_ANYC: return wgrad_anyc_workspace_bytes(a.B, a.M, a.Cin, a.Cout, a.ntaps);
    default: return wgrad_workspace_bytes(a.B, a.M, a.Cin, a.Cout, a.ntaps);              // direct and bf16x3: the same partial slabs
  }
}

static int ws_check(const char* what, size_t need, size_t have) {      // what = "conv-math" (GENNET_CONV_WS_GB, ops.set_conv_math) or the entry point
  if (need <= have) return GN_OK;
  set_error("%s workspace: the selected kernel needs %zu bytes, the workspace has %zu", what, need, have);
  return GN_EWORKSPACE;
}

// The phases of one strided data gradient read the same dy and kernel: under the opt-in split the first phase splits them (ALL w_taps taps, so the
// planes' layout does not depend on the phase), the later ones reuse the planes (8 of the 28 split passes of a BASELINE step are such repeats).
struct Phases { int w_taps; bool have_split; };

// one forward / data-gradient-phase launch on the family select_conv picks; ph: the phase state of a strided data gradient, else NULL
static int conv_run(const ConvArgs& a, hipStream_t s, Phases* ph = nullptr) {
  const ConvFamily f = select_conv(a, ph ? ph->w_taps : 0);
  int w_taps = ph ? ph->w_taps : 0;                      // taps of the kernel the split covers
  for (int j = 0; !ph && j < a.t.ntaps; ++j) w_taps = std::max(w_taps, a.t.widx[j] + 1);
  const size_t need = f == CONV_WINO ? conv_wino_workspace_bytes(a.Cin, a.Cout) : f == CONV_WINO_S2 ? conv_wino_s2_workspace_bytes(a.Cin, a.Cout)
                      : f == CONV_BF16X3 ? conv_bf16x3_workspace_bytes(a.B, a.Lin, a.Cin, a.Cout, w_taps) : 0;
  if (int rc = ws_check("conv-math", need, g_conv_ws_bytes)) return rc;
  switch (f) {
    case CONV_SMALL: return a.Cin <= 4 ? conv_smallcin_dispatch(a, s) : conv_smallcout_dispatch(a, s);
    case CONV_WINO: return conv_wino_run(a, g_conv_ws, g_conv_ws_bytes, s);
    case CONV_WINO_S2: return conv_wino_s2_run(a, g_conv_ws, g_conv_ws_bytes, s);
    case CONV_BF16X3:
      if (!(ph && ph->have_split)) {
        int rc = conv_bf16x3_split(a, w_taps, g_conv_ws, g_conv_ws_bytes, true, true, s);
        if (rc) return rc;
        if (ph) ph->have_split = true;
      }
      return conv_bf16x3_run(a, w_taps, g_conv_ws, s);
    case CONV_ANYC: return conv_anyc_dispatch(a, s);
    default: return conv_mfma_dispatch(a, s);
  }
}

// ConvArgs of a forward launch (Dense: B = 1, L = Lout = the batch, k = 1)
static ConvArgs fwd_args(const float* x, const float* w, const float* bias, float* y, int B, int L, int Cin, int Cout, int k, int stride, int pad_left,
                         int Lout, int act, float act_param) {
  ConvArgs a = {};
  a.x = x; a.w = w; a.bias = bias; a.y = y;
  a.B = B; a.Lin = L; a.Cin = Cin; a.Cout = Cout; a.M = Lout; a.Ly = Lout;
  a.t.ntaps = k; a.t.in_stride = stride; a.t.out_stride = 1;
  for (int j = 0; j < k; ++j) { a.t.off[j] = j - pad_left; a.t.widx[j] = j; }
  a.act = act; a.act_param = act_param;
  return a;
}

static int set_conv_math_impl(int mode, void* workspace, size_t workspace_bytes) {
  GN_REQUIRE(mode >= 0 && mode <= 2, "set_conv_math: mode %d (0 = direct fp32, 1 = bf16x3, 2 = transform-domain fp32)", mode);
  GN_REQUIRE(mode == 0 || workspace, "set_conv_math: modes 1 and 2 need a device workspace");
  if (mode == 2 && workspace_bytes < kWinoKernelBytes) {
    set_error("set_conv_math: the transform-domain math needs a workspace of %zu bytes, got %zu", kWinoKernelBytes, workspace_bytes);
    return GN_EWORKSPACE;
  }
  g_conv_math = mode;
  g_conv_ws = mode ? workspace : nullptr;
  g_conv_ws_bytes = mode ? workspace_bytes : 0;
  return GN_OK;
}

// Dense layers whose width is not one the matrix-core kernels take (in % 4 or out % 4, beyond the small-output heads): one fp32 GEMM
// C[m, n] = act(sum_k A(m, k) B(k, n) + bias[n]) with A(m, k) = A[m sam + k sak], B(k, n) = B[k sbk + n sbn], so the forward, the data gradient
// (B = w read transposed) and the weight gradient (A = x read transposed) are the same kernel.  16 x 16 output tiles through LDS; each output is one
// fmaf chain in k order (the zero padding of the last k tile adds exact zeros), so results do not depend on the launch.
__global__ __launch_bounds__(256) void dense_any_kernel(const float* __restrict__ A, const float* __restrict__ Bm, const float* __restrict__ bias,
                                                        float* __restrict__ C, int M, int N, int K, size_t sam, size_t sak, size_t sbk, size_t sbn, int act,
                                                        float p) {
  __shared__ float As[16][17], Bs[16][17];
  const int tx = threadIdx.x % 16, ty = threadIdx.x / 16;
  const int m = blockIdx.y * 16 + ty, n = blockIdx.x * 16 + tx;
  float acc = 0.f;
  for (int k0 = 0; k0 < K; k0 += 16) {
    const int ka = k0 + tx, kb = k0 + ty;
    As[ty][tx] = (m < M && ka < K) ? A[(size_t)m * sam + (size_t)ka * sak] : 0.f;
    Bs[ty][tx] = (kb < K && n < N) ? Bm[(size_t)kb * sbk + (size_t)n * sbn] : 0.f;
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) acc = fmaf(As[ty][kk], Bs[kk][tx], acc);
    __syncthreads();
  }
  if (m < M && n < N) C[(size_t)m * N + n] = act_apply(bias ? acc + bias[n] : acc, act, p);
}
static int dense_any_gemm(const float* A, const float* Bm, const float* bias, float* C, int M, int N, int K, size_t sam, size_t sak, size_t sbk, size_t sbn,
                          int act, float p, hipStream_t s) {
  if (M <= 0 || N <= 0) return GN_OK;
  if ((M + 15) / 16 > 65535) { set_error("dense: %d rows exceed the grid", M); return GN_EINVAL; }
  hipLaunchKernelGGL(dense_any_kernel, dim3(cdiv(N, 16), cdiv(M, 16)), dim3(256), 0, s, A, Bm, bias, C, M, N, K, sam, sak, sbk, sbn, act, p);
  return check_launch("dense_any");
}
static bool dense_any_shape(int in, int out) { return (in % 4 || out % 4) && !(out <= 4 && in % 4 == 0); }

}  // namespace gn

using namespace gn;

extern "C" {

const char* gn_last_error(void) { return g_err; }
int gn_version(void) { return 100; }

// the device word every Philox kernel adds to its counter offset: what a captured hipGraph of a train step needs (a by-value argument is frozen at capture)
int gn_set_rng_base(const uint64_t* base_dev) {
  g_rng_base = base_dev;
  return GN_OK;
}

int gn_prof_enable(int on) {
  g_prof_on = on != 0;
  return GN_OK;
}
int gn_prof_reset(void) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  for (auto& r : g_prof) {
    g_pool.push_back(r.a);
    g_pool.push_back(r.b);
  }
  g_prof.clear();
  return GN_OK;
}
int gn_prof_collect(int kind, double* out) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  double ms = 0, flop = 0, cnt = 0, bytes = 0;
  for (auto& r : g_prof) {
    if (kind >= 0 && r.kind != kind) continue;
    cnt += 1;
    if (hipEventSynchronize(r.b) != hipSuccess) { set_error("prof: event sync failed"); return GN_ELAUNCH; }
    float t = 0;
    if (hipEventElapsedTime(&t, r.a, r.b) != hipSuccess) { set_error("prof: elapsed failed"); return GN_ELAUNCH; }
    ms += t;
    flop += r.flop;
    bytes += r.bytes;
  }
  out[0] = cnt;
  out[1] = ms;
  out[2] = flop;
  out[3] = bytes;
  return GN_OK;
}

// ---------------------------------------------------------------------------------------------------------
static int fwd_impl(const float* x, const float* w, const float* bias, float* y, int B, int L, int Cin, int Cout, int k, int stride, int pad_left, int Lout,
                    int act, float act_param, bool any_channels, void* stream) {
  GN_REQUIRE(x && w && y, "conv1d_fwd: null pointer");
  GN_REQUIRE(B >= 0 && L > 0 && Cin > 0 && Cout > 0 && k >= 1 && k <= 8 && stride >= 1 && Lout > 0, "conv1d_fwd: bad shape");
  GN_REQUIRE(pad_left >= 0 && stride * (Lout - 1) + k - pad_left <= L + k, "conv1d_fwd: Lout %d inconsistent with L %d k %d stride %d", Lout, L, k, stride);
  if (B == 0) return GN_OK;
  ConvArgs a = fwd_args(x, w, bias, y, B, L, Cin, Cout, k, stride, pad_left, Lout, act, act_param);
  a.any_channels = any_channels;
  return conv_run(a, (hipStream_t)stream);
}

int gn_conv1d_fwd(const float* x, const float* w, const float* bias, float* y, int B, int L, int Cin, int Cout, int k, int stride, int pad_left, int Lout,
                  int act, float act_param, void* stream) {
  return fwd_impl(x, w, bias, y, B, L, Cin, Cout, k, stride, pad_left, Lout, act, act_param, false, stream);
}
int gn_conv1d_fwd_any(const float* x, const float* w, const float* bias, float* y, int B, int L, int Cin, int Cout, int k, int stride, int pad_left, int Lout,
                      int act, float act_param, void* stream) {
  return fwd_impl(x, w, bias, y, B, L, Cin, Cout, k, stride, pad_left, Lout, act, act_param, true, stream);
}
int gn_conv1d_needs_any(int Cin, int Cout) { return needs_any(Cin, Cout) ? 1 : 0; }

int gn_set_conv_math(int mode, void* workspace, size_t workspace_bytes) { return set_conv_math_impl(mode, workspace, workspace_bytes); }

size_t gn_conv1d_bf16x3_workspace(int B, int L, int Cin, int Cout, int k) { return conv_bf16x3_workspace_bytes(B, L, Cin, Cout, k); }

size_t gn_conv1d_fwd_stats_workspace(int B, int Lout, int Cout) {
  // per-block partials: one row of 2 * Cout doubles per (batch element, row tile); the smallest row tile any launch_conv_pipe instantiation uses
  // is 64 rows (the narrow-wave blocks with one wave in M, conv_pipe.hip conv_pipe_try: nwm == 1)
  const size_t fused = (size_t)B * (size_t)((Lout + 63) / 64) * 2 * (size_t)Cout * sizeof(double);
  const size_t plain = colred_workspace_bytes((size_t)B * Lout, Cout);
  return (fused > plain ? fused : plain) + 256;
}

int gn_conv1d_fwd_stats(const float* x, const float* w, const float* bias, float* y, double* sums, void* ws, size_t ws_bytes, int B, int L, int Cin, int Cout, int k,
                        int stride, int pad_left, int Lout, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  GN_REQUIRE(x && w && y && sums && ws, "conv1d_fwd_stats: null pointer");
  GN_REQUIRE(B > 0 && L > 0 && Cin > 0 && Cout > 0 && Cout % 4 == 0 && k >= 1 && k <= 8 && stride >= 1 && Lout > 0, "conv1d_fwd_stats: bad shape");
  GN_REQUIRE(pad_left >= 0 && stride * (Lout - 1) + k - pad_left <= L + k, "conv1d_fwd_stats: Lout %d inconsistent with L %d k %d stride %d", Lout, L, k, stride);
  if (int rc = ws_check("conv1d_fwd_stats", gn_conv1d_fwd_stats_workspace(B, Lout, Cout), ws_bytes)) return rc;
  ConvArgs a = fwd_args(x, w, bias, y, B, L, Cin, Cout, k, stride, pad_left, Lout, GN_ACT_LINEAR, 0.f);
  int done = 0;
  a.stat_part = (double*)ws; a.stat_sums = sums; a.stat_done = &done;
  int rc = conv_run(a, s);
  if (rc || done) return rc;
  ColRedArgs r = {};                                     // the launched kernel had no statistics epilogue: one separate pass over y
  r.a = y; r.rows = (size_t)B * Lout; r.C = Cout;
  return colred_run(1, r, ws, ws_bytes, sums, nullptr, s);
}

int gn_conv1d_fwd_bf16x3(const float* x, const float* w, const float* bias, float* y, void* ws, size_t ws_bytes, int B, int L, int Cin, int Cout, int k, int stride,
                         int pad_left, int Lout, int act, float act_param, int resplit, void* stream) {
  GN_REQUIRE(x && w && y && ws, "conv1d_fwd_bf16x3: null pointer");
  GN_REQUIRE(B >= 0 && L > 0 && Cin > 0 && Cout > 0 && k >= 1 && k <= 5 && stride >= 1 && Lout > 0 && pad_left >= 0, "conv1d_fwd_bf16x3: bad shape");
  if (B == 0) return GN_OK;
  ConvArgs a = fwd_args(x, w, bias, y, B, L, Cin, Cout, k, stride, pad_left, Lout, act, act_param);
  GN_REQUIRE(conv_bf16x3_supported(a), "conv1d_fwd_bf16x3: needs Cin %% 16 == 0, Cout %% 64 == 0, k <= 5, stride 1");
  if (resplit) {
    int rc = conv_bf16x3_split(a, k, ws, ws_bytes, true, true, (hipStream_t)stream);
    if (rc) return rc;
  }
  return conv_bf16x3_run(a, k, ws, (hipStream_t)stream);
}

size_t gn_conv1d_wino_workspace(int Cin, int Cout) { return conv_wino_workspace_bytes(Cin, Cout); }

int gn_conv1d_fwd_wino(const float* x, const float* w, const float* bias, float* y, void* ws, size_t ws_bytes, int B, int L, int Cin, int Cout, int k, int stride,
                       int pad_left, int Lout, int act, float act_param, void* stream) {
  GN_REQUIRE(x && w && y && ws, "conv1d_fwd_wino: null pointer");
  GN_REQUIRE(B >= 0 && L > 0 && Cin > 0 && Cout > 0 && k == 5 && stride == 1 && Lout > 0 && pad_left >= 0, "conv1d_fwd_wino: 5 taps, unit stride");
  if (B == 0) return GN_OK;
  ConvArgs a = fwd_args(x, w, bias, y, B, L, Cin, Cout, k, stride, pad_left, Lout, act, act_param);
  return conv_wino_run(a, ws, ws_bytes, (hipStream_t)stream);
}

int gn_conv1d_fwd_dropout(const float* x, const float* w, const float* bias, const uint8_t* mask, float* y, int B, int L, int Cin, int Cout, int k, int stride,
                          int pad_left, int Lout, int act, float act_param, float rate, void* stream) {
  GN_REQUIRE(x && w && y && mask, "conv1d_fwd_dropout: null pointer");
  GN_REQUIRE(B >= 0 && L > 0 && Cin > 0 && Cout > 4 && Cout % 4 == 0 && k >= 1 && k <= 5 && stride >= 1 && Lout > 0 && pad_left >= 0, "conv1d_fwd_dropout: bad shape");
  GN_REQUIRE(rate >= 0.f && rate < 1.f, "conv1d_fwd_dropout: bad rate %f", rate);
  if (B == 0) return GN_OK;
  ConvArgs a = fwd_args(x, w, bias, y, B, L, Cin, Cout, k, stride, pad_left, Lout, act, act_param);
  a.mask = mask; a.keep_scale = 1.0f / (1.0f - rate);
  return conv_run(a, (hipStream_t)stream);
}

static int dgrad_impl(const float* dy, const float* wt, float* dx, int B, int L, int Cin, int Cout, int k, int stride, int pad_left, int Lout, const float* gy,
                      const uint8_t* gmask, int gact, float gparam, float grate, void* stream, bool any_channels = false) {
  GN_REQUIRE(dy && wt && dx, "conv1d_dgrad: null pointer");
  GN_REQUIRE(B >= 0 && L > 0 && Cin > 0 && Cout > 0 && k >= 1 && k <= 8 && stride >= 1 && Lout > 0 && pad_left >= 0, "conv1d_dgrad: bad shape");
  if (B == 0) return GN_OK;
  // dx[b, tau, ci] = sum_{k', co} dy[b, t, co] * wt[k', co, ci]  with  stride*t + k' - pad_left == tau.
  // Output phase p = tau mod stride uses the taps with (p + pad_left - k') divisible by stride, at dy row m + (p+pad_left-k')/stride.
  // p < 0: both output phases of a stride-2, 5-tap layer in one launch, the taps in kernel order (tap kk belongs to phase (kk + pad_left) & 1)
  auto phase_args = [&](int p) {
    ConvArgs a = {};
    a.x = dy; a.w = wt; a.bias = nullptr; a.y = dx;
    a.B = B; a.Lin = Lout; a.Cin = Cout; a.Cout = Cin; a.Ly = L;
    a.t.in_stride = 1; a.t.out_stride = stride;
    a.act = GN_ACT_LINEAR;
    a.any_channels = any_channels;
    a.gy = gy; a.gmask = gmask; a.gact = gact; a.gparam = gparam; a.gscale = 1.0f / (1.0f - grate);
    a.M = (L - std::max(p, 0) + stride - 1) / stride;
    a.t.out_off = p < 0 ? pad_left & 1 : p;                  // merged: the phase of the even taps (kk = 0, 2, 4); the odd ones write out_off_odd
    if (p < 0) a.t.out_off_odd = 1 - (pad_left & 1);
    for (int kk = 0; kk < k; ++kk) {
      const int d = (p < 0 ? (kk + pad_left) & 1 : p) + pad_left - kk;
      if (((d % stride) + stride) % stride) continue;
      a.t.off[a.t.ntaps] = (d >= 0) ? d / stride : -((-d) / stride);
      a.t.widx[a.t.ntaps++] = kk;
    }
    return a;
  };
  hipStream_t s = (hipStream_t)stream;
  if (stride == 2 && k == 5) {
    const ConvArgs a = phase_args(-1);
    const DgradFamily f = select_dgrad(a);
    const size_t need = f == DGRAD_WINO_S2 ? conv_wino_s2_workspace_bytes(a.Cin, a.Cout)
                        : f == DGRAD_BF16X3_MERGED ? conv_bf16x3_workspace_bytes(a.B, a.Lin, a.Cin, a.Cout, 5) : 0;
    if (int rc = ws_check("conv-math", need, g_conv_ws_bytes)) return rc;
    if (f == DGRAD_WINO_S2) return conv_wino_s2_run(a, g_conv_ws, g_conv_ws_bytes, s);
    if (f == DGRAD_MERGED) return conv_pipe_run_merged(a, s);
    if (f == DGRAD_BF16X3_MERGED) {
      int rc = conv_bf16x3_split(a, 5, g_conv_ws, g_conv_ws_bytes, true, true, s);
      return rc ? rc : conv_bf16x3_run_merged(a, g_conv_ws, s);
    }
  }
  // k < stride (k >= stride gives every phase a tap): no tap reaches the input rows of some phases, whose gradient is zero (and stays zero under a
  // fused producer derivative): dx is cleared once, the phases that have taps then write their own rows
  if (k < stride) {
    (void)hipMemsetAsync(dx, 0, (size_t)B * L * Cin * sizeof(float), s);
    if (int rc = check_launch("conv1d_dgrad (clearing dx)")) return rc;
  }
  Phases ph = {stride > 1 ? k : 0, false};
  for (int p = 0; p < stride && p < L; ++p) {
    const ConvArgs a = phase_args(p);
    if (a.t.ntaps == 0) continue;
    int rc = conv_run(a, s, stride > 1 ? &ph : nullptr);
    if (rc) return rc;
  }
  return GN_OK;
}

int gn_conv1d_dgrad(const float* dy, const float* wt, float* dx, int B, int L, int Cin, int Cout, int k, int stride, int pad_left, int Lout, void* stream) {
  return dgrad_impl(dy, wt, dx, B, L, Cin, Cout, k, stride, pad_left, Lout, nullptr, nullptr, GN_ACT_LINEAR, 0.f, 0.f, stream);
}

int gn_conv1d_dgrad_any(const float* dy, const float* wt, float* dx, int B, int L, int Cin, int Cout, int k, int stride, int pad_left, int Lout, void* stream) {
  return dgrad_impl(dy, wt, dx, B, L, Cin, Cout, k, stride, pad_left, Lout, nullptr, nullptr, GN_ACT_LINEAR, 0.f, 0.f, stream, true);
}

int gn_conv1d_dgrad_fused(const float* dy, const float* wt, float* dx, int B, int L, int Cin, int Cout, int k, int stride, int pad_left, int Lout,
                          const float* y_prev, const uint8_t* mask_prev, int act_prev, float act_param_prev, float rate_prev, void* stream) {
  GN_REQUIRE(y_prev, "conv1d_dgrad_fused: y_prev is NULL");
  GN_REQUIRE(Cin > 4 && Cout > 4, "conv1d_dgrad_fused: only the MFMA path fuses the producer's activation gradient (Cin %d, Cout %d)", Cin, Cout);
  GN_REQUIRE(rate_prev >= 0.f && rate_prev < 1.f, "conv1d_dgrad_fused: bad rate");
  return dgrad_impl(dy, wt, dx, B, L, Cin, Cout, k, stride, pad_left, Lout, y_prev, mask_prev, act_prev, act_param_prev, mask_prev ? rate_prev : 0.f, stream);
}

static WgradArgs wgrad_args(const float* x, const float* dy, void* ws, int B, int L, int Cin, int Cout, int k, int stride, int pad_left, int Lout) {
  WgradArgs a = {};
  a.x = x; a.dy = dy; a.part = (float*)ws;
  a.B = B; a.Lin = L; a.Cin = Cin; a.Cout = Cout; a.M = Lout; a.ntaps = k; a.in_stride = stride;
  for (int j = 0; j < k && j < 8; ++j) a.off[j] = j - pad_left;
  return a;
}

size_t gn_conv1d_wgrad_workspace(int B, int L, int Cin, int Cout, int k, int stride, int Lout) {
  WgradArgs a = wgrad_args(nullptr, nullptr, nullptr, B, L, Cin, Cout, k, stride, 0, Lout);      // (the need does not depend on pad_left)
  a.any_channels = 1;       // a pair only gn_conv1d_wgrad_any takes gets that kernel's size; the flag changes nothing for every other pair
  return std::max(wgrad_ws_need(select_wgrad(a), a), bias_grad_ws((size_t)B * Lout, Cout)) + 256;
}

static int wgrad_impl(const float* x, const float* dy, float* dw, float* db, void* ws, size_t ws_bytes, int B, int L, int Cin, int Cout, int k, int stride,
                      int pad_left, int Lout, bool any_channels, void* stream) {
  GN_REQUIRE(x && dy && dw && ws, "conv1d_wgrad: null pointer");
  GN_REQUIRE(B > 0 && L > 0 && Cin > 0 && Cout > 0 && k >= 1 && k <= 5 && stride >= 1 && Lout > 0 && pad_left >= 0, "conv1d_wgrad: bad shape");
  hipStream_t s = (hipStream_t)stream;
  WgradArgs a = wgrad_args(x, dy, ws, B, L, Cin, Cout, k, stride, pad_left, Lout);
  a.db = db;
  a.any_channels = any_channels;
  const WgradFamily f = select_wgrad(a);
  // what gn_conv1d_wgrad_workspace advertises for this call, to the byte: the family's slabs or the bias-gradient pass, whichever is larger
  int rc = ws_check("conv1d_wgrad", std::max(wgrad_ws_need(f, a), bias_grad_ws((size_t)B * Lout, Cout)) + 256, ws_bytes);
  if (rc) return rc;
  switch (f) {
    case WGRAD_SMALL: {
      WgradSmallArgs sa = {x, dy, (float*)ws, B, L, Cin, Cout, Lout, k, stride};
      std::copy(a.off, a.off + k, sa.off);
      rc = wgrad_small_dispatch(sa, dw, ws_bytes, s);
      break;
    }
    case WGRAD_WINO: rc = wgrad_wino_run(a, dw, s); break;           // transform domain; the bias gradient takes the separate pass below
    case WGRAD_WINO_S2: rc = wgrad_wino_s2_run(a, dw, s); break;
    case WGRAD_ANYC: rc = wgrad_anyc_dispatch(a, dw, ws_bytes, s); break;
    case WGRAD_BF16X3:
      rc = ws_check("conv-math", wgrad_bf16x3_workspace_bytes(B, Lout, Cin, Cout, stride), g_conv_ws_bytes);
      if (!rc) rc = wgrad_bf16x3_dispatch(a, dw, g_conv_ws, g_conv_ws_bytes, s);
      break;
    default:
      rc = wgrad_mfma_dispatch(a, dw, ws_bytes, s);
      if (!rc && a.db_done) return GN_OK;                  // the weight-gradient kernel summed the bias gradient on the way
  }
  if (rc) return rc;
  return db ? bias_grad(dy, db, (size_t)B * Lout, Cout, ws, ws_bytes, s) : GN_OK;
}

int gn_conv1d_wgrad(const float* x, const float* dy, float* dw, float* db, void* ws, size_t ws_bytes, int B, int L, int Cin, int Cout, int k, int stride,
                    int pad_left, int Lout, void* stream) {
  return wgrad_impl(x, dy, dw, db, ws, ws_bytes, B, L, Cin, Cout, k, stride, pad_left, Lout, false, stream);
}
int gn_conv1d_wgrad_any(const float* x, const float* dy, float* dw, float* db, void* ws, size_t ws_bytes, int B, int L, int Cin, int Cout, int k, int stride,
                        int pad_left, int Lout, void* stream) {
  return wgrad_impl(x, dy, dw, db, ws, ws_bytes, B, L, Cin, Cout, k, stride, pad_left, Lout, true, stream);
}

int gn_dense_fwd(const float* x, const float* w, const float* bias, float* y, int B, int in, int out, int act, float act_param, void* stream) {
  GN_REQUIRE(x && w && y && B >= 0 && in > 0 && out > 0, "dense_fwd: bad arguments");
  if (B == 0) return GN_OK;
  if (dense_any_shape(in, out))
    return dense_any_gemm(x, w, bias, y, B, out, in, (size_t)in, 1, (size_t)out, 1, act, act_param, (hipStream_t)stream);
  if (out <= 4) return dense_small_fwd(x, w, bias, y, B, in, out, act, act_param, (hipStream_t)stream);
  return conv_mfma_dispatch(fwd_args(x, w, bias, y, 1, B, in, out, 1, 1, 0, B, act, act_param), (hipStream_t)stream);
}

size_t gn_dense_bwd_workspace(int B, int in, int out) {
  if (out <= 4) return 256;
  if (dense_any_shape(in, out)) return bias_grad_ws((size_t)B, out) + 256;
  size_t w = wgrad_workspace_bytes(1, B, in, out, 1);
  size_t b = bias_grad_ws((size_t)B, out);
  return (w > b ? w : b) + (size_t)in * out * sizeof(float) + 256;
}

int gn_dense_bwd_fused(const float* x, const float* w, const float* dy, float* dx, float* dw, float* db, int B, int in, int out, const uint8_t* mask_prev,
                       int act_prev, float act_param_prev, float rate_prev, void* stream) {
  GN_REQUIRE(x && w && dy && dx && dw && B > 0 && in > 0 && out >= 1 && out <= 4, "dense_bwd_fused: bad arguments (small-output heads only)");
  GN_REQUIRE(rate_prev >= 0.f && rate_prev < 1.f, "dense_bwd_fused: bad rate");
  return dense_small_bwd(x, w, dy, dx, dw, db, B, in, out, (hipStream_t)stream, act_prev, act_param_prev, mask_prev, 1.0f / (1.0f - (mask_prev ? rate_prev : 0.f)));
}

int gn_dense_bwd(const float* x, const float* w, const float* dy, float* dx, float* dw, float* db, void* ws, size_t ws_bytes, int B, int in, int out, void* stream) {
  GN_REQUIRE(x && w && dy && dw && B > 0 && in > 0 && out > 0, "dense_bwd: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  if (dense_any_shape(in, out)) {
    // dx = dy w^T, dw = x^T dy, db = column sums of dy (bias_grad: fixed order for out > 4)
    GN_REQUIRE(ws, "dense_bwd: null workspace");
    if (int rc = ws_check("dense_bwd", gn_dense_bwd_workspace(B, in, out), ws_bytes)) return rc;
    int rc = dx ? dense_any_gemm(dy, w, nullptr, dx, B, in, out, (size_t)out, 1, 1, (size_t)out, GN_ACT_LINEAR, 0.f, s) : GN_OK;
    if (!rc) rc = dense_any_gemm(x, dy, nullptr, dw, in, out, B, 1, (size_t)in, (size_t)out, 1, GN_ACT_LINEAR, 0.f, s);
    if (!rc && db) rc = bias_grad(dy, db, (size_t)B, out, ws, ws_bytes, s);
    return rc;
  }
  if (out <= 4) return dense_small_bwd(x, w, dy, dx, dw, db, B, in, out, s);
  GN_REQUIRE(ws, "dense_bwd: null workspace");
  if (int rc = ws_check("dense_bwd", gn_dense_bwd_workspace(B, in, out), ws_bytes)) return rc;
  const size_t wt_bytes = (size_t)in * out * sizeof(float);
  float* wt = (float*)ws;
  void* ws2 = (char*)ws + wt_bytes;
  const size_t ws2_bytes = ws_bytes - wt_bytes;
  int rc;
  if (dx) {
    rc = transpose_w(w, wt, 1, in, out, s);
    if (rc) return rc;
    rc = conv_run(fwd_args(dy, wt, nullptr, dx, 1, B, out, in, 1, 1, 0, B, GN_ACT_LINEAR, 0.f), s);
    if (rc) return rc;
  }
  WgradArgs g = wgrad_args(x, dy, ws2, 1, B, in, out, 1, 1, 0, B);
  rc = wgrad_mfma_dispatch(g, dw, ws2_bytes, s);
  if (rc) return rc;
  if (db) rc = bias_grad(dy, db, (size_t)B, out, ws2, ws2_bytes, s);
  return rc;
}

}  // extern "C"
