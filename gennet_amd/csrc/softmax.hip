// Softmax along one axis (keras activations.softmax / layers.Softmax(axis)), forward and the gradient through the OUTPUT:
//   y  = exp(x - max_p x) / sum_p exp(x - max_p x)          dx = y * (dy - sum_p dy * y)
// on the (outer, P, inner) view of csrc/bn_axis.hip: element (o, p, i) at (o*P + p)*inner + i, P the softmax axis.  The reduction stays inside
// one (o, i) column, so a row never leaves the unit that owns it and nothing is exchanged between blocks: no workspace, no atomics.
//
// Regimes, by shape alone (the seams are the constants below):
//   inner == 1, a row is P contiguous floats
//     P <= 1024         `rows`: a sub-group of W = min(64, pow2ceil(P)) lanes owns a row, 64 / W rows per wave, NJ = pow2ceil(P / 64) <= 16
//                       values per lane in registers (W < 64: one).  8 bytes / element forward, 12 backward.
//     P <= 4096         `block`: one block of 256 lanes per row, the row (backward: y and dy) parked in LDS.  8 / 12 bytes.
//     P >  4096         `stream`: one block per row, tiles of 2048 values; a running maximum and a sum rescaled once per tile, then a second
//                       read of x that writes y.  12 bytes forward (two reads, one write), 20 backward.
//   inner > 1
//     inner >= 16       `axis`: a lane owns an (o, i) column (a float4 of four columns where inner % 4 == 0 and the pointers are 16-byte
//                       aligned), consecutive lanes consecutive addresses, and walks p with stride inner in chunks of CH = 16 (float4: 8)
//                       positions held in registers.  P <= CH: 8 / 12 bytes; beyond, the running maximum / rescaled sum per chunk and
//                       a second read: 12 / 20 bytes.
//     inner <  16       `split`: the per-lane walk would put fewer than 16 consecutive floats under a wave, so a wave owns one o and its lanes
//                       are (pp, i), pp < S = 64 / inner: S * inner consecutive floats per load, P split over the S lanes of a column and
//                       reduced with cross-lane reads, in chunks of CH = 16 positions a lane (P <= 4 * S: 4).  P <= 16 * S: 8 / 12 bytes,
//                       beyond 12 / 20.
// Reductions are fp32 in a fixed order: a lane adds its values in index order, lanes combine in an xor butterfly (offsets 1, 2 .. W/2; both
// partners form a + b, so every lane holds the same bits), the four waves of a block as (w0 + w1) + (w2 + w3), the S lanes of a split column
// in lane order.  The maximum is exact in any order.  exp is expf (<= 1 ulp), the quotient one correctly rounded division.  Two runs give
// identical bits.  y may alias x and dx may alias dy: a lane reads what it writes before it writes it, and never reads another lane's output.
#include <math.h>

#include "common.h"
#include "lane_reduce.h"

namespace gn {
namespace {

constexpr int SM_ROWS_MAX_P = 1024;      // rows -> block
constexpr int SM_BLOCK_MAX_P = 4096;     // block -> stream
constexpr int SM_TILE = 2048;            // stream: values per tile (8 per lane)
constexpr int SM_SPLIT_INNER = 16;       // inner < 16: split, else axis
constexpr int SM_GRID_CAP = 2048;        // blocks of 256; the rest by grid stride

// group_reduce<W, MAX>: the fixed-order all-reduce over aligned sub-groups of W lanes (csrc/lane_reduce.h)

__device__ __forceinline__ float block_max(float v, float* red) {
  v = group_reduce<64, true>(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  v = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  __syncthreads();
  return v;
}
__device__ __forceinline__ float block_sum(float v, float* red) {
  v = group_reduce<64, false>(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  v = (red[0] + red[1]) + (red[2] + red[3]);
  __syncthreads();
  return v;
}

// ---------------------------------------------------------------------------------------------
// rows: W lanes per row, NJ values per lane (column sl + W*j).  a = x | dy, yin = y (backward only).
// Every lane stays in the loop and in the shuffles; a lane without a row or a column loads nothing and stores nothing.
// ---------------------------------------------------------------------------------------------
template <int W, int NJ, bool BWD>
__global__ __launch_bounds__(256) void softmax_rows_kernel(const float* a, const float* yin, float* out, size_t outer, int P) {
  constexpr int RPW = 64 / W;
  // forward: U row groups per trip, every load issued before the first use and the U dependent chains (cross-lane steps, expf, division) free
  // to interleave; a group past the end computes on pads and stores nothing.  The backward's short chain reaches the copy rate with one.
  constexpr int U = BWD || NJ >= 8 ? 1 : 8 / NJ;
  const unsigned lane = threadIdx.x & 63, sl = lane % W;
  const size_t nwaves = (size_t)gridDim.x * 4;
  const size_t groups = (outer + RPW - 1) / RPW;
  for (size_t g0 = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6); g0 < groups; g0 += nwaves * U) {
    float v[U][NJ], u[U][NJ];
    bool ok[U][NJ];
    size_t base[U];
#pragma unroll
    for (int k = 0; k < U; ++k) {
      const size_t row = (g0 + k * nwaves) * RPW + lane / W;      // a group past the end has no row
      const bool rok = row < outer;
      base[k] = (rok ? row : 0) * (size_t)P;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const unsigned c = sl + W * j;
        ok[k][j] = rok && c < (unsigned)P;
        v[k][j] = ok[k][j] ? a[base[k] + c] : (BWD ? 0.f : -INFINITY);
        if (BWD) u[k][j] = ok[k][j] ? yin[base[k] + c] : 0.f;
      }
    }
#pragma unroll
    for (int k = 0; k < U; ++k) {
      if (!BWD) {
        float m = v[k][0];
#pragma unroll
        for (int j = 1; j < NJ; ++j) m = fmaxf(m, v[k][j]);
        m = group_reduce<W, true>(m);
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          v[k][j] = ok[k][j] ? expf(v[k][j] - m) : 0.f;
          s = j == 0 ? v[k][0] : s + v[k][j];
        }
        s = group_reduce<W, false>(s);
#pragma unroll
        for (int j = 0; j < NJ; ++j)
          if (ok[k][j]) out[base[k] + sl + W * j] = v[k][j] / s;
      } else {
        float t = 0.f;
#pragma unroll
        for (int j = 0; j < NJ; ++j) t = j == 0 ? v[k][0] * u[k][0] : t + v[k][j] * u[k][j];
        t = group_reduce<W, false>(t);
#pragma unroll
        for (int j = 0; j < NJ; ++j)
          if (ok[k][j]) out[base[k] + sl + W * j] = u[k][j] * (v[k][j] - t);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// block: one block per row, 1024 < P <= 4096, the row in LDS (a lane parks and re-reads its own indices tid + 256*k)
// ---------------------------------------------------------------------------------------------
template <bool BWD>
__global__ __launch_bounds__(256) void softmax_block_kernel(const float* a, const float* yin, float* out, size_t outer, int P) {
  __shared__ float buf[BWD ? 2 * SM_BLOCK_MAX_P : SM_BLOCK_MAX_P];
  __shared__ float red[4];
  const int tid = threadIdx.x;
  for (size_t row = blockIdx.x; row < outer; row += gridDim.x) {
    const size_t base = row * (size_t)P;
    if (!BWD) {
      float m = -INFINITY;
      for (int i = tid; i < P; i += 256) {
        const float t = a[base + i];
        buf[i] = t;
        m = fmaxf(m, t);
      }
      m = block_max(m, red);
      float s = 0.f;
      for (int i = tid; i < P; i += 256) {
        const float e = expf(buf[i] - m);
        buf[i] = e;
        s = i == tid ? e : s + e;
      }
      s = block_sum(s, red);
      for (int i = tid; i < P; i += 256) out[base + i] = buf[i] / s;
    } else {
      float t = 0.f;
      for (int i = tid; i < P; i += 256) {
        const float g = a[base + i], y = yin[base + i];
        buf[i] = g;
        buf[SM_BLOCK_MAX_P + i] = y;
        t = i == tid ? g * y : t + g * y;
      }
      t = block_sum(t, red);
      for (int i = tid; i < P; i += 256) out[base + i] = buf[SM_BLOCK_MAX_P + i] * (buf[i] - t);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// stream: one block per row, P > 4096.  Forward: per tile of 2048 values the block's exact maximum, then every lane rescales its sum
// by exp(M_old - M_new) -- once per tile, however the data are ordered -- and adds its 8 exponentials; a second read writes y.
// ---------------------------------------------------------------------------------------------
template <bool BWD>
__global__ __launch_bounds__(256) void softmax_stream_kernel(const float* a, const float* yin, float* out, size_t outer, int P) {
  __shared__ float red[4];
  const int tid = threadIdx.x;
  for (size_t row = blockIdx.x; row < outer; row += gridDim.x) {
    const size_t base = row * (size_t)P;
    if (!BWD) {
      float M = -INFINITY, s = 0.f;
      for (int t0 = 0; t0 < P; t0 += SM_TILE) {
        float v[SM_TILE / 256];
        float cm = -INFINITY;
#pragma unroll
        for (int u = 0; u < SM_TILE / 256; ++u) {
          const int i = t0 + u * 256 + tid;
          v[u] = i < P ? a[base + i] : -INFINITY;
          cm = fmaxf(cm, v[u]);
        }
        const float Mn = fmaxf(M, block_max(cm, red));
        float ts = 0.f;
#pragma unroll
        for (int u = 0; u < SM_TILE / 256; ++u) {
          const float e = expf(v[u] - Mn);                 // a pad is -inf: +0
          ts = u == 0 ? e : ts + e;
        }
        s = t0 == 0 ? ts : s * expf(M - Mn) + ts;
        M = Mn;
      }
      s = block_sum(s, red);
      for (int i = tid; i < P; i += 256) out[base + i] = expf(a[base + i] - M) / s;
    } else {
      float t = 0.f;
      for (int i = tid; i < P; i += 256) {
        const float p = a[base + i] * yin[base + i];
        t = i == tid ? p : t + p;
      }
      t = block_sum(t, red);
      for (int i = tid; i < P; i += 256) out[base + i] = yin[base + i] * (a[base + i] - t);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// axis (SPLIT false): a lane owns VEC adjacent columns of one o and every p.  split (SPLIT true, VEC 1): a wave owns one o, lane = pp*inner + i
// owns the positions pp, pp + S, ... of column i; the S lanes of a column combine by reading lanes i, i + inner, ... in that order.
// ---------------------------------------------------------------------------------------------
template <int VEC>
__device__ __forceinline__ void sm_load(const float* p, float (&v)[VEC]) {
  if constexpr (VEC == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
    v[0] = *p;
  }
}
template <int VEC>
__device__ __forceinline__ void sm_store(float* p, const float (&v)[VEC]) {
  if constexpr (VEC == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  else *p = v[0];
}
__device__ __forceinline__ float column_max(float v, int i, int S, int inner) {
  float r = -INFINITY;
  for (int k = 0; k < S; ++k) r = fmaxf(r, __shfl(v, i + k * inner, 64));
  return r;
}
__device__ __forceinline__ float column_sum(float v, int i, int S, int inner) {
  float r = __shfl(v, i, 64);
  for (int k = 1; k < S; ++k) r += __shfl(v, i + k * inner, 64);
  return r;
}

// one column set: positions p0, p0 + pstep, ... < P at base + p * inner; `active` false: a lane that only takes part in the cross-lane reads
template <int VEC, int CH, bool SPLIT, bool BWD>
__device__ __forceinline__ void softmax_column(const float* a, const float* yin, float* out, size_t base, int p0, int pstep, int P, int inner, bool active,
                                               int ci, int S) {
  const int per = CH * pstep;
  const bool fits = P <= per;
  float v[CH][VEC], w[CH][VEC], acc[VEC], M[VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) { acc[e] = 0.f; M[e] = -INFINITY; }
  for (int pc = 0; pc < P; pc += per) {
    float cm[VEC], ts[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) cm[e] = -INFINITY;
#pragma unroll
    for (int u = 0; u < CH; ++u) {
      const int p = pc + p0 + u * pstep;
      if (active && p < P) {
        sm_load<VEC>(a + base + (size_t)p * inner, v[u]);
        if (BWD) sm_load<VEC>(yin + base + (size_t)p * inner, w[u]);
      } else {
#pragma unroll
        for (int e = 0; e < VEC; ++e) { v[u][e] = BWD ? 0.f : -INFINITY; w[u][e] = 0.f; }
      }
#pragma unroll
      for (int e = 0; e < VEC; ++e) cm[e] = fmaxf(cm[e], v[u][e]);
    }
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      if (!BWD) {
        if (SPLIT) cm[e] = column_max(cm[e], ci, S, inner);
        const float Mn = fmaxf(M[e], cm[e]);
#pragma unroll
        for (int u = 0; u < CH; ++u) {
          v[u][e] = expf(v[u][e] - Mn);                    // a pad is -inf: +0
          ts[e] = u == 0 ? v[0][e] : ts[e] + v[u][e];
        }
        acc[e] = pc == 0 ? ts[e] : acc[e] * expf(M[e] - Mn) + ts[e];
        M[e] = Mn;
      } else {
#pragma unroll
        for (int u = 0; u < CH; ++u) ts[e] = u == 0 ? v[0][e] * w[0][e] : ts[e] + v[u][e] * w[u][e];
        acc[e] = pc == 0 ? ts[e] : acc[e] + ts[e];
      }
    }
    if (fits) {                                            // the one chunk is the column: write from the registers
      float tot[VEC];
#pragma unroll
      for (int e = 0; e < VEC; ++e) tot[e] = SPLIT ? column_sum(acc[e], ci, S, inner) : acc[e];
#pragma unroll
      for (int u = 0; u < CH; ++u) {
        const int p = p0 + u * pstep;
        if (active && p < P) {
          float o[VEC];
#pragma unroll
          for (int e = 0; e < VEC; ++e) o[e] = BWD ? w[u][e] * (v[u][e] - tot[e]) : v[u][e] / tot[e];
          sm_store<VEC>(out + base + (size_t)p * inner, o);
        }
      }
      return;
    }
  }
  float tot[VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) tot[e] = SPLIT ? column_sum(acc[e], ci, S, inner) : acc[e];
  if (!active) return;
  for (int p = p0; p < P; p += pstep) {
    float x[VEC], y[VEC], o[VEC];
    sm_load<VEC>(a + base + (size_t)p * inner, x);
    if (BWD) sm_load<VEC>(yin + base + (size_t)p * inner, y);
#pragma unroll
    for (int e = 0; e < VEC; ++e) o[e] = BWD ? y[e] * (x[e] - tot[e]) : expf(x[e] - M[e]) / tot[e];
    sm_store<VEC>(out + base + (size_t)p * inner, o);
  }
}

template <int VEC, bool BWD>
__global__ __launch_bounds__(256) void softmax_axis_kernel(const float* a, const float* yin, float* out, size_t outer, int P, int inner) {
  const size_t iv = (size_t)(inner / VEC), ncol = outer * iv, stride = (size_t)gridDim.x * 256;
  for (size_t col = (size_t)blockIdx.x * 256 + threadIdx.x; col < ncol; col += stride) {
    const size_t o = col / iv, i = col % iv;
    softmax_column<VEC, VEC == 4 ? 8 : 16, false, BWD>(a, yin, out, o * (size_t)P * inner + i * VEC, 0, 1, P, inner, true, 0, 1);
  }
}

// CH = 4 where the column fits 4 positions a lane (P <= 4 S: no exponentials of pads), else 16
template <int CH, bool BWD>
__global__ __launch_bounds__(256) void softmax_split_kernel(const float* a, const float* yin, float* out, size_t outer, int P, int inner) {
  const int lane = threadIdx.x & 63, S = 64 / inner;
  const size_t nwaves = (size_t)gridDim.x * 4;
  for (size_t o = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6); o < outer; o += nwaves)
    softmax_column<1, CH, true, BWD>(a, yin, out, o * (size_t)P * inner + lane % inner, lane / inner, S, P, inner, lane < S * inner, lane % inner, S);
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

unsigned capped(size_t blocks) { return (unsigned)(blocks < 1 ? 1 : blocks > (size_t)SM_GRID_CAP ? (size_t)SM_GRID_CAP : blocks); }

template <int W, int NJ, bool BWD>
void launch_rows(const float* a, const float* yin, float* out, size_t outer, int P, hipStream_t s) {
  const size_t groups = (outer + 64 / W - 1) / (64 / W);
  hipLaunchKernelGGL((softmax_rows_kernel<W, NJ, BWD>), dim3(capped((groups + 3) / 4)), dim3(256), 0, s, a, yin, out, outer, P);
}

template <bool BWD>
int run(const float* a, const float* yin, float* out, size_t outer, int P, int inner, hipStream_t s) {
  if (inner == 1) {
    if (P <= 1) launch_rows<1, 1, BWD>(a, yin, out, outer, P, s);
    else if (P <= 2) launch_rows<2, 1, BWD>(a, yin, out, outer, P, s);
    else if (P <= 4) launch_rows<4, 1, BWD>(a, yin, out, outer, P, s);
    else if (P <= 8) launch_rows<8, 1, BWD>(a, yin, out, outer, P, s);
    else if (P <= 16) launch_rows<16, 1, BWD>(a, yin, out, outer, P, s);
    else if (P <= 32) launch_rows<32, 1, BWD>(a, yin, out, outer, P, s);
    else if (P <= 64) launch_rows<64, 1, BWD>(a, yin, out, outer, P, s);
    else if (P <= 128) launch_rows<64, 2, BWD>(a, yin, out, outer, P, s);
    else if (P <= 256) launch_rows<64, 4, BWD>(a, yin, out, outer, P, s);
    else if (P <= 512) launch_rows<64, 8, BWD>(a, yin, out, outer, P, s);
    else if (P <= SM_ROWS_MAX_P) launch_rows<64, 16, BWD>(a, yin, out, outer, P, s);
    else if (P <= SM_BLOCK_MAX_P) hipLaunchKernelGGL(softmax_block_kernel<BWD>, dim3(capped(outer)), dim3(256), 0, s, a, yin, out, outer, P);
    else hipLaunchKernelGGL(softmax_stream_kernel<BWD>, dim3(capped(outer)), dim3(256), 0, s, a, yin, out, outer, P);
  } else if (inner < SM_SPLIT_INNER) {
    if (P <= 4 * (64 / inner)) hipLaunchKernelGGL((softmax_split_kernel<4, BWD>), dim3(capped((outer + 3) / 4)), dim3(256), 0, s, a, yin, out, outer, P, inner);
    else hipLaunchKernelGGL((softmax_split_kernel<16, BWD>), dim3(capped((outer + 3) / 4)), dim3(256), 0, s, a, yin, out, outer, P, inner);
  } else if (inner % 4 == 0 && aligned16(a) && aligned16(out) && (!BWD || aligned16(yin))) {
    hipLaunchKernelGGL((softmax_axis_kernel<4, BWD>), dim3(capped((outer * (size_t)(inner / 4) + 255) / 256)), dim3(256), 0, s, a, yin, out, outer, P, inner);
  } else {
    hipLaunchKernelGGL((softmax_axis_kernel<1, BWD>), dim3(capped((outer * (size_t)inner + 255) / 256)), dim3(256), 0, s, a, yin, out, outer, P, inner);
  }
  return check_launch(BWD ? "softmax_bwd" : "softmax_fwd");
}

bool shape_ok(size_t outer, int P, int inner) {
  return outer >= 1 && P >= 1 && inner >= 1 && (uint64_t)P * (uint64_t)inner < 0x80000000ull && outer <= ((size_t)1 << 62) / ((size_t)P * (size_t)inner);
}

}  // namespace
}  // namespace gn

using namespace gn;

extern "C" {

int gn_softmax_fwd(const float* x, float* y, size_t outer, int P, int inner, void* stream) {
  GN_REQUIRE(x && y, "softmax_fwd: null pointer");
  GN_REQUIRE(shape_ok(outer, P, inner), "softmax_fwd: bad shape (outer %zu, P %d, inner %d): all >= 1, P * inner < 2^31, outer * P * inner < 2^62", outer, P,
             inner);
  return run<false>(x, nullptr, y, outer, P, inner, (hipStream_t)stream);
}

int gn_softmax_bwd(const float* dy, const float* y, float* dx, size_t outer, int P, int inner, void* stream) {
  GN_REQUIRE(dy && y && dx, "softmax_bwd: null pointer");
  GN_REQUIRE(shape_ok(outer, P, inner), "softmax_bwd: bad shape (outer %zu, P %d, inner %d): all >= 1, P * inner < 2^31, outer * P * inner < 2^62", outer, P,
             inner);
  return run<true>(dy, y, dx, outer, P, inner, (hipStream_t)stream);
}

}  // extern "C"
