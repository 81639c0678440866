// Layer normalisation over the trailing axes (keras layers.LayerNormalization) on the (rows, N) view, N contiguous:
//   mean_r = sum_c x / N    var_r = sum_c (x - mean_r)^2 / N    rstd_r = 1 / sqrt(var_r + eps)    xhat = (x - mean_r) rstd_r    y = xhat gamma + beta
//   g = dy gamma    dx = rstd_r ((g - mean_c g) - xhat mean_c (g xhat))    dgamma[c] = sum_r dy xhat    dbeta[c] = sum_r dy
// The variance is the centred second pass over the values the first pass read, never E[x^2] - E[x]^2.  A reduction never leaves the unit that
// owns the row; only the weight gradients cross rows, as one fp32 (2, N) partial per block in plain stores, summed in fp64 in a fixed order by
// ln_final_kernel (the shape of colred_final_kernel in csrc/bn.hip, which reads fp64 partials: twice the bytes for sums that were formed in
// fp32).  No atomics; the grid is a function of (rows, N) alone (csrc/layernorm_geom.h).
//
// A lane owns quads, four adjacent columns: one 16-byte access where N % 4 == 0 and every pointer is 16-byte aligned, else four guarded 4-byte
// accesses of the same kernel -- the same columns in the same lanes, so a row's bits do not depend on the alignment.  Regimes, by N alone:
//   N <= 1024   `rows`:   a sub-group of W = min(64, pow2ceil(ceil(N / 4))) lanes owns a row, 64 / W rows a wave, NJ = ceil(N / 256) quads a lane in
//                         registers; U = 4 / NJ row groups a trip, every load issued before the first use.  8 bytes / element forward, 12 backward.
//   N <= 4096   `block`:  one block of 256 lanes per row, up to four quads a lane -- the row lives in the block's registers, LDS carries the four
//                         wave sums only.  8 / 12 bytes.
//   N >  4096   `stream`: one block per row.  Forward: three reads of x (sum; centred squares; y) -- the centred pass is a second READ, the row
//                         sums stay fp32 -- and one write: 16 bytes, 8 of them re-reads of a row of at least 16 KiB the block has just read.
//                         Backward: the row means of g and g xhat first (one read of dy and x; two floats a row into the workspace), then per
//                         chunk of 4096 columns all rows of the block again, so that a lane's accumulators stay in registers: 20 bytes.
// Reductions are fp32 in a fixed order that depends on N alone: a lane adds its values in index order, the lanes of a sub-group combine in an
// xor butterfly (csrc/lane_reduce.h), the four waves of a block as (w0 + w1) + (w2 + w3).  The weight-gradient accumulators of a lane add the
// rows it visits in visiting order; the sub-groups of a wave combine in sub-group order, the waves as above.  Two runs give identical bits, and
// a row's y and dx do not depend on rows, the grid or the launch.  y may alias x and dx may alias dy.
#include <math.h>

#include "common.h"
#include "lane_reduce.h"
#include "layernorm_geom.h"

namespace gn {
namespace {

static_assert(LN_ROWS_MAX_N == GN_LN_ROWS_MAX_N && LN_BLOCK_MAX_N == GN_LN_BLOCK_MAX_N && LN_FWD_GRID_CAP == GN_LN_FWD_GRID_CAP &&
                  LN_BWD_GRID_CAP == GN_LN_BWD_GRID_CAP && LN_BWD_GRID_CAP_WIDE == GN_LN_BWD_GRID_CAP_WIDE,
              "include/gennet_hip.h repeats the seams of layernorm_geom.h");
static_assert(LN_ROWS_MAX_N == 64 * 4 * 4 && LN_BLOCK_MAX_N == LN_BLOCK * 4 * 4 && LN_CHUNK == LN_BLOCK * 4 * 4, "four quads a lane");

// the quad at columns c .. c + 3 of the N floats at p: columns past N read as 0 and are not stored
template <bool VEC>
__device__ __forceinline__ void ln_load(const float* p, int c, int N, float (&v)[4]) {
  if constexpr (VEC) {
    const float4 t = c < N ? *reinterpret_cast<const float4*>(p + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = c + e < N ? p[c + e] : 0.f;
  }
}
template <bool VEC>
__device__ __forceinline__ void ln_store(float* p, int c, int N, const float (&v)[4]) {
  if constexpr (VEC) {
    if (c < N) *reinterpret_cast<float4*>(p + c) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (c + e < N) p[c + e] = v[e];
  }
}
// a parameter vector, `fill` where it is absent
template <bool VEC>
__device__ __forceinline__ void ln_param(const float* p, int c, int N, float fill, float (&v)[4]) {
  if (p) {
    ln_load<VEC>(p, c, N, v);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = fill;
  }
}

// the block's sum of a (and of b): wave butterflies, then (w0 + w1) + (w2 + w3); every lane gets the same bits
__device__ __forceinline__ void block_sum2(float& a, float& b, float (*red)[4]) {
  a = group_reduce<64, false>(a);
  b = group_reduce<64, false>(b);
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = a;
    red[1][threadIdx.x >> 6] = b;
  }
  __syncthreads();
  a = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
  b = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
  __syncthreads();
}
__device__ __forceinline__ float block_sum(float a, float (*red)[4]) {
  float b = 0.f;
  block_sum2(a, b, red);
  return a;
}

// mean and rstd of the NQ quads v a unit holds (columns c0 + 4 (first + step j) + e; pads are 0), reduced by `sum`; v becomes x - mean (pads 0)
template <int NQ, typename Sum>
__device__ __forceinline__ void ln_moments(float (&v)[NQ][4], int first, int step, int N, float eps, Sum sum, float& mu, float& r) {
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < NQ; ++j)
#pragma unroll
    for (int e = 0; e < 4; ++e) s += v[j][e];
  mu = sum(s) / (float)N;
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < NQ; ++j)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float d = 4 * (first + step * j) + e < N ? v[j][e] - mu : 0.f;
      v[j][e] = d;
      q += d * d;
    }
  r = 1.f / sqrtf(sum(q) / (float)N + eps);
}

// one row of the backward held in NQ quads: xv becomes xhat, gv stays dy; the lane's partial sums of g and g xhat; the accumulators take the row
template <int NQ>
__device__ __forceinline__ void ln_bwd_sums(float (&xv)[NQ][4], const float (&gv)[NQ][4], const float (&ga)[NQ][4], float mu, float r, float& s1,
                                            float& s2, float (&ag)[NQ][4], float (&ab)[NQ][4]) {
  s1 = 0.f;
  s2 = 0.f;
#pragma unroll
  for (int j = 0; j < NQ; ++j)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float xh = (xv[j][e] - mu) * r, g = gv[j][e] * ga[j][e];          // a pad has dy = 0: it adds 0 everywhere
      xv[j][e] = xh;
      s1 += g;
      s2 += g * xh;
      ag[j][e] += gv[j][e] * xh;
      ab[j][e] += gv[j][e];
    }
}
__device__ __forceinline__ void ln_dx(const float (&xh)[4], const float (&dy)[4], const float (&ga)[4], float r, float m1, float m2, float (&o)[4]) {
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = r * ((dy[e] * ga[e] - m1) - xh[e] * m2);
}

// ---------------------------------------------------------------------------------------------
// rows: W lanes per row, NJ quads per lane (quad sl + W j), U row groups a trip.  Every lane stays in the loop and in the cross-lane steps; a lane
// without a row or a column loads nothing and stores nothing.
// ---------------------------------------------------------------------------------------------
template <int W, int NJ, bool VEC>
__global__ __launch_bounds__(LN_BLOCK) void ln_rows_fwd_kernel(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd,
                                                               size_t rows, int N, float eps) {
  constexpr int U = ln_u(NJ);
  const int lane = threadIdx.x & 63, sl = lane % W, wave = threadIdx.x >> 6;
  const size_t groups = ln_groups(rows, N);
  float ga[NJ][4], be[NJ][4];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    ln_param<VEC>(gamma, 4 * (sl + W * j), N, 1.f, ga[j]);
    ln_param<VEC>(beta, 4 * (sl + W * j), N, 0.f, be[j]);
  }
  for (size_t t = 0; ln_rows_group(blockIdx.x, wave, t, 0, gridDim.x, U) < groups; ++t) {
    float v[U][NJ][4];
    size_t row[U];
#pragma unroll
    for (int k = 0; k < U; ++k) {
      row[k] = ln_rows_row(ln_rows_group(blockIdx.x, wave, t, k, gridDim.x, U), lane, N);
#pragma unroll
      for (int j = 0; j < NJ; ++j) ln_load<VEC>(x + (row[k] < rows ? row[k] : 0) * (size_t)N, row[k] < rows ? 4 * (sl + W * j) : N, N, v[k][j]);
    }
#pragma unroll
    for (int k = 0; k < U; ++k) {
      float mu, r;
      ln_moments<NJ>(v[k], sl, W, N, eps, [](float s) { return group_reduce<W, false>(s); }, mu, r);
      if (row[k] < rows) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          float o[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] = fmaf(v[k][j][e] * r, ga[j][e], be[j][e]);
          ln_store<VEC>(y + row[k] * (size_t)N, 4 * (sl + W * j), N, o);
        }
        if (mean && sl == 0) {
          mean[row[k]] = mu;
          rstd[row[k]] = r;
        }
      }
    }
  }
}

template <int W, int NJ, bool VEC>
__global__ __launch_bounds__(LN_BLOCK) void ln_rows_bwd_kernel(const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd,
                                                               float* dx, float* part, size_t rows, int N) {
  constexpr int U = ln_u(NJ), RPW = 64 / W, COLS = 4 * W * NJ;
  __shared__ float red[4][2][COLS];
  const int lane = threadIdx.x & 63, sl = lane % W, wave = threadIdx.x >> 6;
  const size_t groups = ln_groups(rows, N);
  float ga[NJ][4], ag[NJ][4], ab[NJ][4];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    ln_param<VEC>(gamma, 4 * (sl + W * j), N, 1.f, ga[j]);
#pragma unroll
    for (int e = 0; e < 4; ++e) ag[j][e] = ab[j][e] = 0.f;
  }
  for (size_t t = 0; ln_rows_group(blockIdx.x, wave, t, 0, gridDim.x, U) < groups; ++t) {
    float xv[U][NJ][4], gv[U][NJ][4], mu[U], r[U];
    size_t row[U];
#pragma unroll
    for (int k = 0; k < U; ++k) {
      row[k] = ln_rows_row(ln_rows_group(blockIdx.x, wave, t, k, gridDim.x, U), lane, N);
      const bool ok = row[k] < rows;
      const size_t base = (ok ? row[k] : 0) * (size_t)N;
      mu[k] = ok ? mean[row[k]] : 0.f;
      r[k] = ok ? rstd[row[k]] : 0.f;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        ln_load<VEC>(x + base, ok ? 4 * (sl + W * j) : N, N, xv[k][j]);
        ln_load<VEC>(dy + base, ok ? 4 * (sl + W * j) : N, N, gv[k][j]);
      }
    }
#pragma unroll
    for (int k = 0; k < U; ++k) {
      float s1, s2;
      ln_bwd_sums<NJ>(xv[k], gv[k], ga, mu[k], r[k], s1, s2, ag, ab);
      const float m1 = group_reduce<W, false>(s1) / (float)N, m2 = group_reduce<W, false>(s2) / (float)N;
      if (dx && row[k] < rows) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          float o[4];
          ln_dx(xv[k][j], gv[k][j], ga[j], r[k], m1, m2, o);
          ln_store<VEC>(dx + row[k] * (size_t)N, 4 * (sl + W * j), N, o);
        }
      }
    }
  }
  if (!part) return;
  // the 64 / W sub-groups of the wave in sub-group order, then the four waves
#pragma unroll
  for (int j = 0; j < NJ; ++j)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float a = __shfl(ag[j][e], sl, 64), b = __shfl(ab[j][e], sl, 64);
      for (int k = 1; k < RPW; ++k) {
        a += __shfl(ag[j][e], sl + k * W, 64);
        b += __shfl(ab[j][e], sl + k * W, 64);
      }
      if (lane < W) {
        red[wave][0][4 * (sl + W * j) + e] = a;
        red[wave][1][4 * (sl + W * j) + e] = b;
      }
    }
  __syncthreads();
  for (int c = threadIdx.x; c < N; c += LN_BLOCK)
#pragma unroll
    for (int which = 0; which < 2; ++which)
      part[ln_part_slot(which, blockIdx.x, c, gridDim.x, N)] = (red[0][which][c] + red[1][which][c]) + (red[2][which][c] + red[3][which][c]);
}

// ---------------------------------------------------------------------------------------------
// block: one block per row, 1024 < N <= 4096; lane tid owns the quads tid + 256 k, k < 4
// ---------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(LN_BLOCK) void ln_block_fwd_kernel(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd,
                                                                size_t rows, int N, float eps) {
  __shared__ float red[2][4];
  const int tid = threadIdx.x;
  float ga[4][4], be[4][4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    ln_param<VEC>(gamma, 4 * (tid + LN_BLOCK * k), N, 1.f, ga[k]);
    ln_param<VEC>(beta, 4 * (tid + LN_BLOCK * k), N, 0.f, be[k]);
  }
  for (size_t row = blockIdx.x; row < rows; row += gridDim.x) {
    float v[4][4], mu, r;
#pragma unroll
    for (int k = 0; k < 4; ++k) ln_load<VEC>(x + row * (size_t)N, 4 * (tid + LN_BLOCK * k), N, v[k]);
    ln_moments<4>(v, tid, LN_BLOCK, N, eps, [&](float s) { return block_sum(s, red); }, mu, r);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float o[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = fmaf(v[k][e] * r, ga[k][e], be[k][e]);
      ln_store<VEC>(y + row * (size_t)N, 4 * (tid + LN_BLOCK * k), N, o);
    }
    if (mean && tid == 0) {
      mean[row] = mu;
      rstd[row] = r;
    }
  }
}

template <bool VEC>
__global__ __launch_bounds__(LN_BLOCK) void ln_block_bwd_kernel(const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd,
                                                                float* dx, float* part, size_t rows, int N) {
  __shared__ float red[2][4];
  const int tid = threadIdx.x;
  float ga[4][4], ag[4][4], ab[4][4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    ln_param<VEC>(gamma, 4 * (tid + LN_BLOCK * k), N, 1.f, ga[k]);
#pragma unroll
    for (int e = 0; e < 4; ++e) ag[k][e] = ab[k][e] = 0.f;
  }
  for (size_t row = blockIdx.x; row < rows; row += gridDim.x) {
    float xv[4][4], gv[4][4], s1, s2;
    const float mu = mean[row], r = rstd[row];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      ln_load<VEC>(x + row * (size_t)N, 4 * (tid + LN_BLOCK * k), N, xv[k]);
      ln_load<VEC>(dy + row * (size_t)N, 4 * (tid + LN_BLOCK * k), N, gv[k]);
    }
    ln_bwd_sums<4>(xv, gv, ga, mu, r, s1, s2, ag, ab);
    block_sum2(s1, s2, red);
    const float m1 = s1 / (float)N, m2 = s2 / (float)N;
    if (dx) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float o[4];
        ln_dx(xv[k], gv[k], ga[k], r, m1, m2, o);
        ln_store<VEC>(dx + row * (size_t)N, 4 * (tid + LN_BLOCK * k), N, o);
      }
    }
  }
  if (!part) return;
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int c = 4 * (tid + LN_BLOCK * k) + e;
      if (c < N) {
        part[ln_part_slot(0, blockIdx.x, c, gridDim.x, N)] = ag[k][e];
        part[ln_part_slot(1, blockIdx.x, c, gridDim.x, N)] = ab[k][e];
      }
    }
}

// ---------------------------------------------------------------------------------------------
// stream: one block per row, N > 4096; lane tid owns the quads tid + 256 i and adds them in that order
// ---------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(LN_BLOCK) void ln_stream_fwd_kernel(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd,
                                                                 size_t rows, int N, float eps) {
  __shared__ float red[2][4];
  const int tid = threadIdx.x;
  for (size_t row = blockIdx.x; row < rows; row += gridDim.x) {
    const float* xr = x + row * (size_t)N;
    float v[4], s = 0.f;
    for (int c = 4 * tid; c < N; c += 4 * LN_BLOCK) {
      ln_load<VEC>(xr, c, N, v);
#pragma unroll
      for (int e = 0; e < 4; ++e) s += v[e];
    }
    const float mu = block_sum(s, red) / (float)N;
    float q = 0.f;
    for (int c = 4 * tid; c < N; c += 4 * LN_BLOCK) {
      ln_load<VEC>(xr, c, N, v);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float d = c + e < N ? v[e] - mu : 0.f;
        q += d * d;
      }
    }
    const float r = 1.f / sqrtf(block_sum(q, red) / (float)N + eps);
    for (int c = 4 * tid; c < N; c += 4 * LN_BLOCK) {
      float g[4], b[4], o[4];
      ln_load<VEC>(xr, c, N, v);
      ln_param<VEC>(gamma, c, N, 1.f, g);
      ln_param<VEC>(beta, c, N, 0.f, b);
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = fmaf((v[e] - mu) * r, g[e], b[e]);
      ln_store<VEC>(y + row * (size_t)N, c, N, o);
    }
    if (mean && tid == 0) {
      mean[row] = mu;
      rstd[row] = r;
    }
  }
}

// stat: two floats a row (the means of g and g xhat), written by this block in its first sweep and read by it in the second
template <bool VEC>
__global__ __launch_bounds__(LN_BLOCK) void ln_stream_bwd_kernel(const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd,
                                                                 float* dx, float* stat, float* part, size_t rows, int N) {
  __shared__ float red[2][4];
  const int tid = threadIdx.x;
  if (dx) {
    for (size_t row = blockIdx.x; row < rows; row += gridDim.x) {
      const float mu = mean[row], r = rstd[row];
      float s1 = 0.f, s2 = 0.f;
      for (int c = 4 * tid; c < N; c += 4 * LN_BLOCK) {
        float xv[4], gv[4], ga[4];
        ln_load<VEC>(x + row * (size_t)N, c, N, xv);
        ln_load<VEC>(dy + row * (size_t)N, c, N, gv);
        ln_param<VEC>(gamma, c, N, 1.f, ga);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float g = gv[e] * ga[e];
          s1 += g;
          s2 += g * ((xv[e] - mu) * r);
        }
      }
      block_sum2(s1, s2, red);
      if (tid == 0) {
        stat[2 * row] = s1 / (float)N;
        stat[2 * row + 1] = s2 / (float)N;
      }
    }
    __syncthreads();          // lane 0's stores, for the block's other lanes
  }
  for (int c0 = 0; c0 < N; c0 += LN_CHUNK) {
    float ga[4][4], ag[4][4], ab[4][4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      ln_param<VEC>(gamma, c0 + 4 * (tid + LN_BLOCK * k), N, 1.f, ga[k]);
#pragma unroll
      for (int e = 0; e < 4; ++e) ag[k][e] = ab[k][e] = 0.f;
    }
    for (size_t row = blockIdx.x; row < rows; row += gridDim.x) {
      float xv[4][4], gv[4][4], s1, s2;
      const float mu = mean[row], r = rstd[row];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        ln_load<VEC>(x + row * (size_t)N, c0 + 4 * (tid + LN_BLOCK * k), N, xv[k]);
        ln_load<VEC>(dy + row * (size_t)N, c0 + 4 * (tid + LN_BLOCK * k), N, gv[k]);
      }
      ln_bwd_sums<4>(xv, gv, ga, mu, r, s1, s2, ag, ab);
      if (dx) {
        const float m1 = stat[2 * row], m2 = stat[2 * row + 1];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          float o[4];
          ln_dx(xv[k], gv[k], ga[k], r, m1, m2, o);
          ln_store<VEC>(dx + row * (size_t)N, c0 + 4 * (tid + LN_BLOCK * k), N, o);
        }
      }
    }
    if (part) {
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int c = c0 + 4 * (tid + LN_BLOCK * k) + e;
          if (c < N) {
            part[ln_part_slot(0, blockIdx.x, c, gridDim.x, N)] = ag[k][e];
            part[ln_part_slot(1, blockIdx.x, c, gridDim.x, N)] = ab[k][e];
          }
        }
    }
  }
}

// dgamma (blockIdx.y 0) and dbeta (1): out[c] = the sum over the blocks of part[which][b][c] in fp64 -- the 256 / COLS lanes of a column take
// the blocks lane, lane + 256 / COLS, ... in that order, then the lanes are added in lane order -- rounded once to fp32
template <int COLS>
__global__ __launch_bounds__(256) void ln_final_kernel(const float* __restrict__ part, float* dgamma, float* dbeta, int N, int blocks) {
  constexpr int LANES = 256 / COLS;
  __shared__ double red[LANES][COLS + 1];
  float* out = blockIdx.y ? dbeta : dgamma;
  if (!out) return;
  const int col = threadIdx.x % COLS, lane = threadIdx.x / COLS, c = blockIdx.x * COLS + col;
  double s = 0.0;
  if (c < N)
    for (int b = lane; b < blocks; b += LANES) s += (double)part[ln_part_slot(blockIdx.y, b, c, blocks, N)];
  red[lane][col] = s;
  __syncthreads();
  if (lane == 0 && c < N) {
    double t = red[0][col];
    for (int l = 1; l < LANES; ++l) t += red[l][col];
    out[c] = (float)t;
  }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// the rows kernel of an N <= 1024: W and NJ as layernorm_geom.h gives them
#define LN_ROWS_CASE(KERNEL, W, NJ, ...) hipLaunchKernelGGL((KERNEL<W, NJ, VEC>), dim3(grid), dim3(LN_BLOCK), 0, s, __VA_ARGS__)
#define LN_ROWS_LAUNCH(KERNEL, ...)                                   \
  do {                                                                \
    const int w = ln_w(N), nj = ln_nj(N);                             \
    if (w == 1) LN_ROWS_CASE(KERNEL, 1, 1, __VA_ARGS__);              \
    else if (w == 2) LN_ROWS_CASE(KERNEL, 2, 1, __VA_ARGS__);         \
    else if (w == 4) LN_ROWS_CASE(KERNEL, 4, 1, __VA_ARGS__);         \
    else if (w == 8) LN_ROWS_CASE(KERNEL, 8, 1, __VA_ARGS__);         \
    else if (w == 16) LN_ROWS_CASE(KERNEL, 16, 1, __VA_ARGS__);       \
    else if (w == 32) LN_ROWS_CASE(KERNEL, 32, 1, __VA_ARGS__);       \
    else if (nj == 1) LN_ROWS_CASE(KERNEL, 64, 1, __VA_ARGS__);       \
    else if (nj == 2) LN_ROWS_CASE(KERNEL, 64, 2, __VA_ARGS__);       \
    else if (nj == 3) LN_ROWS_CASE(KERNEL, 64, 3, __VA_ARGS__);       \
    else LN_ROWS_CASE(KERNEL, 64, 4, __VA_ARGS__);                    \
  } while (0)

template <bool VEC>
void launch_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd, size_t rows, int N, float eps, hipStream_t s) {
  const unsigned grid = ln_grid(rows, N, LN_FWD_GRID_CAP);
  if (ln_regime(N) == 0) LN_ROWS_LAUNCH(ln_rows_fwd_kernel, x, gamma, beta, y, mean, rstd, rows, N, eps);
  else if (ln_regime(N) == 1) hipLaunchKernelGGL(ln_block_fwd_kernel<VEC>, dim3(grid), dim3(LN_BLOCK), 0, s, x, gamma, beta, y, mean, rstd, rows, N, eps);
  else hipLaunchKernelGGL(ln_stream_fwd_kernel<VEC>, dim3(grid), dim3(LN_BLOCK), 0, s, x, gamma, beta, y, mean, rstd, rows, N, eps);
}

template <bool VEC>
void launch_bwd(const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd, float* dx, float* stat, float* part,
                size_t rows, int N, hipStream_t s) {
  const unsigned grid = ln_grid(rows, N, ln_bwd_cap(N));
  if (ln_regime(N) == 0) LN_ROWS_LAUNCH(ln_rows_bwd_kernel, dy, x, gamma, mean, rstd, dx, part, rows, N);
  else if (ln_regime(N) == 1) hipLaunchKernelGGL(ln_block_bwd_kernel<VEC>, dim3(grid), dim3(LN_BLOCK), 0, s, dy, x, gamma, mean, rstd, dx, part, rows, N);
  else hipLaunchKernelGGL(ln_stream_bwd_kernel<VEC>, dim3(grid), dim3(LN_BLOCK), 0, s, dy, x, gamma, mean, rstd, dx, stat, part, rows, N);
}

bool shape_ok(size_t rows, int N) { return rows >= 1 && N >= 1 && rows < ((size_t)1 << 62) / (size_t)N; }

}  // namespace
}  // namespace gn

using namespace gn;

extern "C" {

int gn_layernorm_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd, size_t rows, int N, float eps,
                     void* stream) {
  GN_REQUIRE(x && y, "layernorm_fwd: null pointer (x and y are required)");
  GN_REQUIRE(shape_ok(rows, N), "layernorm_fwd: bad shape (rows %zu, N %d): both >= 1, rows * N < 2^62", rows, N);
  GN_REQUIRE(eps >= 0.f && isfinite(eps), "layernorm_fwd: eps %g is negative or not finite", (double)eps);
  GN_REQUIRE(!mean == !rstd, "layernorm_fwd: mean and rstd are given together (the training phase) or both NULL");
  const bool vec = N % 4 == 0 && aligned16(x) && aligned16(y) && aligned16(gamma) && aligned16(beta);
  if (vec) launch_fwd<true>(x, gamma, beta, y, mean, rstd, rows, N, eps, (hipStream_t)stream);
  else launch_fwd<false>(x, gamma, beta, y, mean, rstd, rows, N, eps, (hipStream_t)stream);
  return check_launch("layernorm_fwd");
}

size_t gn_layernorm_bwd_workspace(size_t rows, int N) { return shape_ok(rows, N) ? ln_ws_floats(rows, N) * sizeof(float) : 0; }

int gn_layernorm_bwd(const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd, float* dx, float* dgamma, float* dbeta,
                     void* ws, size_t ws_bytes, size_t rows, int N, void* stream) {
  GN_REQUIRE(dy && x && mean && rstd, "layernorm_bwd: null pointer (dy, x, mean and rstd are required)");
  GN_REQUIRE(shape_ok(rows, N), "layernorm_bwd: bad shape (rows %zu, N %d): both >= 1, rows * N < 2^62", rows, N);
  GN_REQUIRE(gamma || !dgamma, "layernorm_bwd: dgamma without gamma (scale=False has no gamma to differentiate)");
  const bool weights = dgamma || dbeta, need_ws = weights || (dx && ln_regime(N) == 2);
  if (!dx && !weights) return GN_OK;
  if (need_ws) {
    GN_REQUIRE(ws, "layernorm_bwd: null pointer (the workspace is required for dgamma / dbeta, and for dx where N > %d)", LN_BLOCK_MAX_N);
    GN_REQUIRE(((uintptr_t)ws & 3) == 0, "layernorm_bwd: the workspace holds floats and must be 4-byte aligned");
    const size_t need = gn_layernorm_bwd_workspace(rows, N);
    if (ws_bytes < need) {
      set_error("layernorm_bwd: workspace too small (ws_bytes %zu, gn_layernorm_bwd_workspace = %zu)", ws_bytes, need);
      return GN_EWORKSPACE;
    }
  }
  float* stat = (float*)ws;
  float* part = weights ? stat + ln_ws_stat_floats(rows, N) : nullptr;
  hipStream_t s = (hipStream_t)stream;
  const bool vec = N % 4 == 0 && aligned16(dy) && aligned16(x) && aligned16(dx) && aligned16(gamma);
  if (vec) launch_bwd<true>(dy, x, gamma, mean, rstd, dx, stat, part, rows, N, s);
  else launch_bwd<false>(dy, x, gamma, mean, rstd, dx, stat, part, rows, N, s);
  int rc = check_launch("layernorm_bwd");
  if (rc || !weights) return rc;
  const int blocks = (int)ln_grid(rows, N, ln_bwd_cap(N));
  if (blocks >= 256) hipLaunchKernelGGL(ln_final_kernel<8>, dim3(cdiv(N, 8), 2), dim3(256), 0, s, part, dgamma, dbeta, N, blocks);
  else hipLaunchKernelGGL(ln_final_kernel<32>, dim3(cdiv(N, 32), 2), dim3(256), 0, s, part, dgamma, dbeta, N, blocks);
  return check_launch("layernorm_bwd (sum of the partials)");
}

}  // extern "C"
