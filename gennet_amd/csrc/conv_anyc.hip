// The `anyc` family: 1-D convolution and its weight gradient for channel pairs no other family takes (gn_conv1d_needs_any: what the small-Cin,
// small-Cout and direct dispatchers refuse), on the same exact-fp32 matrix-core instruction as the direct family
// (v_mfma_f32_32x32x2_f32: every output is one fmaf chain).  Reached only through the gn_conv1d_*_any entry points (capi.hip, select_conv /
// select_wgrad).
//
// Same contract as conv_mfma.hip:
//     y[b, os*m + o0, n] = act(bias[n] + sum_j sum_c x[b, is*m + off[j], c] * w[widx[j], c, n]),   rows outside [0, Lin) read 0
// so the forward, the unit-stride data gradient and every phase of a strided one are this one kernel.  What differs from the direct family is
// the staging: a row of x starts at t * Cin floats, which is 16-byte aligned only when Cin % 4 == 0, so nothing here moves a float4 or uses
// LDS-DMA.  Every staged element is ONE float with its own guard (row inside [0, Lin), channel < Cin, column < Cout), zero otherwise, written
// into the LDS image the direct kernels use ([rows][KC+1] slab, de-interleaved by row parity for in_stride 2; [tap][KC][TN] weights); the
// epilogue stores guarded scalars.  The plain epilogue only (bias, activation): the fused keep-mask, producer gradient and statistics have no
// _any entry point.
#include <algorithm>
#include "common.h"

namespace gn {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// Block = 4 waves stacked in M, each 32 rows x 64 columns (two 32x32 tiles): 128 x 64 outputs.  K-chunks of 8 channels, two LDS stages, one
// barrier per chunk: the loads of chunk c+1 are issued into registers before the MFMAs of chunk c and written to the other stage after them.
template <int NTAPS>
__global__ __launch_bounds__(256) void conv_anyc_kernel(ConvArgs a, int m_tiles, int n_tiles) {
  constexpr int TM = 128, TN = 64, NT = 256, KC = 8, RS = KC + 1;
  extern __shared__ __attribute__((aligned(16))) float smem[];

  const int tid = threadIdx.x, lane = tid & 63, wm = tid >> 6;
  const int i32 = lane & 31, h = lane >> 5;
  const int bid = blockIdx.x;
  const int n_tile = bid % n_tiles;
  const int rest = bid / n_tiles;
  const int m_tile = rest % m_tiles;
  const int b = rest / m_tiles;
  const int m0 = m_tile * TM, n0 = n_tile * TN;

  const int is = a.t.in_stride;
  int minoff = a.t.off[0], maxoff = a.t.off[0];
#pragma unroll
  for (int j = 1; j < NTAPS; ++j) {
    minoff = min(minoff, a.t.off[j]);
    maxoff = max(maxoff, a.t.off[j]);
  }
  const int R = is * (TM - 1) + (maxoff - minoff) + 1;      // input rows one tile reads
  const int Rper = (R + is - 1) / is;
  const int slab_floats = is * Rper * RS;
  const int buf_floats = slab_floats + NTAPS * KC * TN;     // one stage: [slab | weights]

  f32x16 acc[2];
#pragma unroll
  for (int nt = 0; nt < 2; ++nt)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[nt][r] = 0.f;

  const int t_base = is * m0 + minoff;
  const float* xb = a.x + (size_t)b * a.Lin * a.Cin;

  constexpr int S_ITEMS = ((2 * (TM - 1) + 5) * KC + NT - 1) / NT;      // in_stride 2, 5 taps: the largest slab
  constexpr int W_ITEMS = (NTAPS * KC * TN + NT - 1) / NT;
  float sreg[S_ITEMS], wreg[W_ITEMS];
  const int s_count = R * KC;
  constexpr int w_count = NTAPS * KC * TN;

  auto load_chunk = [&](int c0) {
#pragma unroll
    for (int it = 0; it < S_ITEMS; ++it) {
      const int id = tid + it * NT;
      const int r = id / KC, c = c0 + id % KC;
      const int t = t_base + r;
      float v = 0.f;
      if (id < s_count && t >= 0 && t < a.Lin && c < a.Cin) v = xb[(size_t)t * a.Cin + c];
      sreg[it] = v;
    }
#pragma unroll
    for (int it = 0; it < W_ITEMS; ++it) {
      const int id = tid + it * NT;
      const int n = n0 + id % TN;
      const int c = c0 + (id / TN) % KC;
      const int j = id / (TN * KC);
      int wi = a.t.widx[0];
#pragma unroll
      for (int jj = 1; jj < NTAPS; ++jj) wi = j == jj ? a.t.widx[jj] : wi;
      float v = 0.f;
      if (id < w_count && c < a.Cin && n < a.Cout) v = a.w[((size_t)wi * a.Cin + c) * a.Cout + n];
      wreg[it] = v;
    }
  };
  auto store_chunk = [&](float* stage) {
#pragma unroll
    for (int it = 0; it < S_ITEMS; ++it) {
      const int id = tid + it * NT;
      const int r = id / KC, c = id % KC;
      const int lr = (is == 1) ? r : ((r & 1) * Rper + (r >> 1));
      if (id < s_count) stage[lr * RS + c] = sreg[it];
    }
#pragma unroll
    for (int it = 0; it < W_ITEMS; ++it) {
      const int id = tid + it * NT;
      if (id < w_count) stage[slab_floats + id] = wreg[it];               // [tap][KC][TN] is id order
    }
  };

  const int n_chunks = (a.Cin + KC - 1) / KC;
  load_chunk(0);
  store_chunk(smem);
  __syncthreads();
  for (int ch = 0; ch < n_chunks; ++ch) {
    const float* slab = smem + (ch & 1) * buf_floats;
    const float* wl = slab + slab_floats;
    const bool has_next = ch + 1 < n_chunks;
    if (has_next) load_chunk((ch + 1) * KC);
#pragma unroll
    for (int j = 0; j < NTAPS; ++j) {
      const int d = a.t.off[j] - minoff;
      const int rowbase = (is == 1) ? d : ((d & 1) * Rper + (d >> 1));
      const float* ap = slab + (rowbase + wm * 32 + i32) * RS + h;
      const float* bp = wl + (j * KC + h) * TN + i32;
#pragma unroll
      for (int q = 0; q < KC / 2; ++q) {
        const float av = ap[2 * q];
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bp[2 * q * TN + nt * 32], acc[nt], 0, 0, 0);
      }
    }
    if (has_next) store_chunk(smem + ((ch + 1) & 1) * buf_floats);      // the stage chunk ch-1 was read from: every wave is past the barrier below
    __syncthreads();
  }

  // epilogue: C/D layout of the 32x32 tile: col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5)
  float* yb = a.y + (size_t)b * a.Ly * a.Cout;
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) {
    const int n = n0 + nt * 32 + i32;
    if (n >= a.Cout) continue;
    const float bias = a.bias ? a.bias[n] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
      if (m < a.M) yb[(size_t)(a.t.out_stride * m + a.t.out_off) * a.Cout + n] = act_apply(acc[nt][r] + bias, a.act, a.act_param);
    }
  }
}

template <int NTAPS>
static int launch_conv_anyc(const ConvArgs& a, hipStream_t s) {
  constexpr int TM = 128, TN = 64, KC = 8;
  const int is = a.t.in_stride;
  int minoff = a.t.off[0], maxoff = a.t.off[0];
  for (int j = 1; j < NTAPS; ++j) {
    minoff = std::min(minoff, a.t.off[j]);
    maxoff = std::max(maxoff, a.t.off[j]);
  }
  const int R = is * (TM - 1) + (maxoff - minoff) + 1;
  const int Rper = (R + is - 1) / is;
  // the kernel's staging registers are sized for in_stride 2 with taps spanning 5 rows: a wider tap table would leave slab rows unwritten
  GN_REQUIRE(maxoff - minoff + 1 <= 5, "conv_anyc: taps span %d rows (at most 5)", maxoff - minoff + 1);
  const size_t lds = 2 * sizeof(float) * ((size_t)is * Rper * (KC + 1) + (size_t)NTAPS * KC * TN);
  if (lds > 64 * 1024) {
    set_error("conv_anyc: LDS tile %zu B exceeds 64 KiB (tap span %d)", lds, maxoff - minoff + 1);
    return GN_EINVAL;
  }
  const int m_tiles = (a.M + TM - 1) / TM, n_tiles = (a.Cout + TN - 1) / TN;
  const size_t blocks = (size_t)m_tiles * n_tiles * a.B;
  if (blocks == 0 || blocks > 0x7fffffffull) {
    set_error("conv_anyc: bad grid %zu", blocks);
    return GN_EINVAL;
  }
  prof_begin(s);
  hipLaunchKernelGGL((conv_anyc_kernel<NTAPS>), dim3((unsigned)blocks), dim3(256), lds, s, a, m_tiles, n_tiles);
  prof_end(s, 2.0 * a.B * (double)a.M * NTAPS * a.Cin * a.Cout, 9, 4.0 * ((double)a.B * a.Lin * a.Cin + (double)NTAPS * a.Cin * a.Cout + (double)a.B * a.M * a.Cout));
  return check_launch("conv_anyc");
}

int conv_anyc_dispatch(const ConvArgs& a, hipStream_t s) {
  GN_REQUIRE(a.t.in_stride == 1 || a.t.in_stride == 2, "conv_anyc: in_stride %d unsupported (Cin %d, Cout %d: strides 1 and 2)", a.t.in_stride, a.Cin, a.Cout);
  GN_REQUIRE(a.t.ntaps >= 1 && a.t.ntaps <= 5, "conv_anyc: ntaps %d unsupported (1..5)", a.t.ntaps);
  GN_REQUIRE(!a.mask && !a.gy && !a.gmask && !a.stat_part, "conv_anyc: no fused dropout, producer gradient or statistics (Cin %d, Cout %d)", a.Cin, a.Cout);
  switch (a.t.ntaps) {
    case 1: return launch_conv_anyc<1>(a, s);
    case 2: return launch_conv_anyc<2>(a, s);
    case 3: return launch_conv_anyc<3>(a, s);
    case 4: return launch_conv_anyc<4>(a, s);
    default: return launch_conv_anyc<5>(a, s);
  }
}

// ---------------------------------------------------------------------------------------------
// Weight gradient: dw[j, c, n] = sum_{b,m} x[b, is*m + off[j], c] * dy[b, m, n]   (GEMM: M = Cin, N = Cout, K = (b, m)), as wgrad_mfma_kernel:
// block = one (64 Cin, 64 Cout, K-split) on 2 x 2 waves, NTAPS accumulator tiles per wave over the one staged x slab, K-chunks of 32 rows,
// partial slabs [split][tap][Cin][Cout] in the caller's workspace summed in split order (two runs are bit-identical).  Scalar, guarded staging.
// ---------------------------------------------------------------------------------------------
template <int NTAPS>
__global__ __launch_bounds__(256) void wgrad_anyc_kernel(WgradArgs a) {
  constexpr int KT = 32, TC = 64, TN = 64, NT = 256;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wc = wave >> 1, wn = wave & 1;
  const int i32 = lane & 31, h = lane >> 5;
  const int c0 = blockIdx.x * TC, n0 = blockIdx.y * TN, split = blockIdx.z;
  const int is = a.in_stride;

  int minoff = a.off[0], maxoff = a.off[0];
#pragma unroll
  for (int j = 1; j < NTAPS; ++j) {
    minoff = min(minoff, a.off[j]);
    maxoff = max(maxoff, a.off[j]);
  }
  const int R = is * (KT - 1) + (maxoff - minoff) + 1;
  float* slab = smem;               // [R][TC]
  float* dyl = smem + R * TC;       // [KT][TN]

  f32x16 acc[NTAPS];
#pragma unroll
  for (int j = 0; j < NTAPS; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

  const int cpb = (a.M + KT - 1) / KT;                     // K-chunks per batch element
  const int c_lo = split * a.chunks_per_split, c_hi = min(a.B * cpb, c_lo + a.chunks_per_split);
  const int n_chunks = max(c_hi - c_lo, 0);

  constexpr int S_ITEMS = ((2 * (KT - 1) + 5) * TC + NT - 1) / NT;
  constexpr int D_ITEMS = KT * TN / NT;
  float sreg[S_ITEMS], dreg[D_ITEMS];
  const int s_count = R * TC;

  auto load_chunk = [&](int ch) {
    const int b = (c_lo + ch) / cpb, m0 = ((c_lo + ch) % cpb) * KT;
    const float* xb = a.x + (size_t)b * a.Lin * a.Cin;
    const float* dyb = a.dy + (size_t)b * a.M * a.Cout;
    const int t_base = is * m0 + minoff;
#pragma unroll
    for (int it = 0; it < S_ITEMS; ++it) {
      const int id = tid + it * NT;
      const int t = t_base + id / TC, c = c0 + id % TC;
      float v = 0.f;
      if (id < s_count && t >= 0 && t < a.Lin && c < a.Cin) v = xb[(size_t)t * a.Cin + c];
      sreg[it] = v;
    }
#pragma unroll
    for (int it = 0; it < D_ITEMS; ++it) {
      const int id = tid + it * NT;
      const int m = m0 + id / TN, n = n0 + id % TN;
      float v = 0.f;
      if (m < a.M && n < a.Cout) v = dyb[(size_t)m * a.Cout + n];
      dreg[it] = v;
    }
  };
  auto store_chunk = [&]() {
#pragma unroll
    for (int it = 0; it < S_ITEMS; ++it) {
      const int id = tid + it * NT;
      if (id < s_count) slab[id] = sreg[it];               // [R][TC] is id order
    }
#pragma unroll
    for (int it = 0; it < D_ITEMS; ++it) dyl[tid + it * NT] = dreg[it];      // [KT][TN] is id order
  };

  if (n_chunks > 0) {
    load_chunk(0);
    store_chunk();
  }
  __syncthreads();
  for (int ch = 0; ch < n_chunks; ++ch) {
    const bool has_next = ch + 1 < n_chunks;
    if (has_next) load_chunk(ch + 1);
    const float* bp = dyl + h * TN + wn * 32 + i32;
#pragma unroll
    for (int q = 0; q < KT / 2; ++q) {
      const float bv = bp[2 * q * TN];
#pragma unroll
      for (int j = 0; j < NTAPS; ++j) {
        const float av = slab[(is * (2 * q + h) + (a.off[j] - minoff)) * TC + wc * 32 + i32];
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[j], 0, 0, 0);
      }
    }
    if (has_next) {
      __syncthreads();
      store_chunk();
      __syncthreads();
    }
  }

  const int n = n0 + wn * 32 + i32;
  if (n >= a.Cout) return;
#pragma unroll
  for (int j = 0; j < NTAPS; ++j) {
    float* pj = a.part + ((size_t)split * NTAPS + j) * a.Cin * a.Cout;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int c = c0 + wc * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
      if (c < a.Cin) pj[(size_t)c * a.Cout + n] = acc[j][r];
    }
  }
}

// dw[e] = sum_s part[s][e], s ascending
__global__ void wgrad_anyc_reduce_kernel(const float* __restrict__ part, float* __restrict__ dw, size_t n, int splits) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float s = part[i];
#pragma unroll 4
  for (int k = 1; k < splits; ++k) s += part[(size_t)k * n + i];
  dw[i] = s;
}

size_t wgrad_anyc_workspace_bytes(int B, int M, int Cin, int Cout, int ntaps) {
  int s, cps;
  wgrad_split_plan(B, M, Cin, Cout, 64, 64, &s, &cps);
  return (size_t)s * ntaps * Cin * Cout * sizeof(float);
}

template <int NTAPS>
static void launch_wgrad_anyc(const WgradArgs& a, int splits, hipStream_t s) {
  constexpr int KT = 32, TC = 64, TN = 64;
  int minoff = a.off[0], maxoff = a.off[0];
  for (int j = 1; j < NTAPS; ++j) {
    minoff = std::min(minoff, a.off[j]);
    maxoff = std::max(maxoff, a.off[j]);
  }
  const int R = a.in_stride * (KT - 1) + (maxoff - minoff) + 1;
  const size_t lds = sizeof(float) * ((size_t)R * TC + (size_t)KT * TN);
  hipLaunchKernelGGL((wgrad_anyc_kernel<NTAPS>), dim3(cdiv(a.Cin, TC), cdiv(a.Cout, TN), splits), dim3(256), lds, s, a);
}

int wgrad_anyc_dispatch(WgradArgs& a, float* dw, size_t ws_bytes, hipStream_t s) {
  GN_REQUIRE(a.in_stride == 1 || a.in_stride == 2, "wgrad_anyc: in_stride %d unsupported (Cin %d, Cout %d: strides 1 and 2)", a.in_stride, a.Cin, a.Cout);
  GN_REQUIRE(a.ntaps >= 1 && a.ntaps <= 5, "wgrad_anyc: ntaps %d unsupported (1..5)", a.ntaps);
  {
    int lo = a.off[0], hi = a.off[0];      // the staging registers are sized for in_stride 2 with taps spanning 5 rows
    for (int j = 1; j < a.ntaps; ++j) { lo = std::min(lo, a.off[j]); hi = std::max(hi, a.off[j]); }
    GN_REQUIRE(hi - lo + 1 <= 5, "wgrad_anyc: taps span %d rows (at most 5)", hi - lo + 1);
  }
  if (ws_bytes < wgrad_anyc_workspace_bytes(a.B, a.M, a.Cin, a.Cout, a.ntaps)) {
    set_error("wgrad_anyc: workspace too small");
    return GN_EWORKSPACE;
  }
  int splits;
  wgrad_split_plan(a.B, a.M, a.Cin, a.Cout, 64, 64, &splits, &a.chunks_per_split);
  GN_REQUIRE(splits >= 1 && splits <= 65535 && cdiv(a.Cout, 64) <= 65535, "wgrad_anyc: bad grid (%d splits)", splits);
  prof_begin(s);
  switch (a.ntaps) {
    case 1: launch_wgrad_anyc<1>(a, splits, s); break;
    case 2: launch_wgrad_anyc<2>(a, splits, s); break;
    case 3: launch_wgrad_anyc<3>(a, splits, s); break;
    case 4: launch_wgrad_anyc<4>(a, splits, s); break;
    default: launch_wgrad_anyc<5>(a, splits, s); break;
  }
  prof_end(s, 2.0 * a.B * (double)a.M * a.ntaps * a.Cin * a.Cout, 10,
           4.0 * ((double)a.B * a.Lin * a.Cin + (double)a.B * a.M * a.Cout + (double)a.ntaps * a.Cin * a.Cout));
  int rc = check_launch("wgrad_anyc");
  if (rc) return rc;
  const size_t n = (size_t)a.ntaps * a.Cin * a.Cout;
  hipLaunchKernelGGL(wgrad_anyc_reduce_kernel, dim3(cdiv(n, 256)), dim3(256), 0, s, a.part, dw, n, splits);
  return check_launch("wgrad_anyc_reduce");
}

}  // namespace gn
