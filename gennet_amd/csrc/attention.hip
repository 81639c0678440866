// Fused dot-product attention (tf.keras 2.x layers/dense_attention.py Attention): forward and all gradients without a (Tq, Tk) tensor in memory.
//
//   s[i, j] = scale * sum_c q[i, c] k[j, c]      p = softmax_j(s), under `causal` over j <= i only      out[i, :] = sum_j p[i, j] v[j, :]
//   q (B, Tq, d), k (B, Tk, d), v (B, Tk, dv), out (B, Tq, dv), lse (B, Tq) = m + log(l), all contiguous fp32; scale is a DEVICE pointer (NULL = 1), read
//   by every kernel, so a captured step replays with the updated weight.
//
// All products run on v_mfma_f32_32x32x2_f32 (C/D map: col = lane & 31, row = attn_rowmap(reg, lane >> 5), attention_geom.h).  Every kernel has 256 lanes
// as four waves; a block owns ATTN_BQ = 128 rows of one batch entry, a wave 32 of them, and walks the other side in ascending tiles of ATTN_BK = 64 rows
// staged through LDS (zeros outside the extents, 16-byte global loads where the base pointer is 16-byte aligned and the row length a multiple of 4, guarded
// 4-byte loads otherwise).  The row a block owns is always the COLUMN of the accumulators, i.e. a lane: its operand fragment (q; dO; k; v) sits in
// registers for the whole walk, its row statistics are per-lane scalars, and a transposed score tile in the C/D map IS a B operand whose k index is
// permuted (register r of half h is row attn_rowmap(r, h)), so P and dS feed the next product from registers and the other operand is read from LDS at
// the permuted row: nothing is re-laid through LDS.
//
//   attn_fwd_kernel   owns query rows.  Per key tile: S^T = K Q^T (K column-major in LDS), scale, mask, tile maximum (in-lane over 32 values, one
//                     exchange between the lane halves), m' = max(m, tile max), alpha = expf(m - m'), p = expf(s - m'), l = l alpha + sum p,
//                     O^T *= alpha once per tile, O^T += V^T P^T (V row-major in LDS).  Writes out = O / l and, in the training phase, lse.
//   attn_delta_kernel delta[i] = sum_c dO[i, c] out[i, c]: a lane per row, one fma chain over c ascending from +0, the order of the matrix cores' dP (where a
//                     row's p sits on one key, delta is that dP bit for bit and dS cancels exactly).
//   attn_dq_kernel    owns query rows, walks key tiles: S^T and dP^T = V dO^T (K, V column-major), p = expf(scale s - lse), dS = p (dP - delta),
//                     dQ^T += K^T dS^T (the same K tile read along its columns), and the row partial of the scale gradient sum_j dS (q . k), one float a
//                     query row, which the caller sums with the fixed-order column reduction.  dQ = scale * accumulator.
//   attn_dkv_kernel   owns key rows, walks query tiles: S = Q K^T and dP = dO V^T (Q, dO column-major; lse, delta of the tile in LDS), dV^T += dO^T P,
//                     dK^T += Q^T dS.  dK = scale * accumulator.
//   Under `causal` entry (i, j) takes part iff j <= i: a masked p is the constant 0 (so is its dS), tiles wholly above the diagonal are not visited, and a
//   wave skips the sub-tiles that are masked for all of its rows.
//
// NUMERICS.  No atomics, no split over the walked axis, tile sizes are constants.  A row's results are a fixed sequence of fp32 operations over its own
// operand row and that batch entry's other operands, tile after tile in ascending order (inside a tile the 32 x 32 x 2 MFMA is an fma chain in its k
// order; P V and the gradient products take their k in the permuted order above, a constant of the kernel).  So a result does not depend on the batch
// size, on the position in the launch or on the grid; two runs give identical bits; a sample computed alone has the bits it has in a batch.  exp is expf,
// log is logf, out = O / l is a division.  Padding (rows past the extents, columns past d, dv) is an exact +0 in LDS and in the register fragments.
#include <math.h>

#include "attention_geom.h"
#include "common.h"

static_assert(gn::ATTN_BQ == GN_ATTN_BQ && gn::ATTN_BK == GN_ATTN_BK && gn::ATTN_MAX_D == GN_ATTN_MAX_D, "attention_geom.h and gennet_hip.h disagree");

namespace gn {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// ATTN_BK rows r0 .. of a row-major (R, ncols) matrix, DP = 32 DT columns -> LDS, zeros outside.  CMAJOR: [c][row] rows of ATTN_KS, else [row][c] rows of attn_vs.
template <int DT, bool CMAJOR>
__device__ __forceinline__ void attn_stage(float* __restrict__ lds, const float* __restrict__ p, int r0, int R, int ncols, bool vec) {
#pragma unroll
  for (int i = 0; i < 2 * DT; ++i) {
    const int f = threadIdx.x + 256 * i;
    const int row = attn_stage_row(f, DT), c = attn_stage_col(f, DT), r = r0 + row;
    float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r < R && c < ncols) {
      const float* g = p + (long long)r * ncols + c;
      if (vec) {                                   // ncols is a multiple of 4: c + 3 < ncols
        t = *reinterpret_cast<const float4*>(g);
      } else {
        t.x = g[0];
        if (c + 1 < ncols) t.y = g[1];
        if (c + 2 < ncols) t.z = g[2];
        if (c + 3 < ncols) t.w = g[3];
      }
    }
    if (CMAJOR) {
      float* s = lds + attn_cmajor_at(c, row);
      s[0] = t.x;
      s[ATTN_KS] = t.y;
      s[2 * ATTN_KS] = t.z;
      s[3 * ATTN_KS] = t.w;
    } else {
      *reinterpret_cast<float4*>(lds + attn_rmajor_at(row, c, DT)) = t;
    }
  }
}

// the B-operand fragment of a block-owned row: f[kk] = x[row, 2 kk + h], zeros outside
template <int DT>
__device__ __forceinline__ void attn_frag(float (&f)[16 * DT], const float* __restrict__ p, int row, int R, int ncols, int h) {
#pragma unroll
  for (int kk = 0; kk < 16 * DT; ++kk) {
    const int c = 2 * kk + h;
    f[kk] = (row < R && c < ncols) ? p[(long long)row * ncols + c] : 0.f;
  }
}

// acc (32 x 32, rows = the tile's rows sub .. sub + 31, columns = the wave's own rows) = T . F^T for a column-major tile T and a register fragment F
template <int DT>
__device__ __forceinline__ f32x16 attn_scores(const float* __restrict__ tile, const float (&f)[16 * DT], int sub, int fr, int h) {
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  const float* a = tile + attn_cmajor_at(h, sub + fr);
#pragma unroll
  for (int kk = 0; kk < 16 * DT; ++kk) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[2 * kk * ATTN_KS], f[kk], acc, 0, 0, 0);
  return acc;
}

// acc[u] (rows = columns c of the tile, columns = the wave's own rows) += T^T . W for a column-major tile T and W in the C/D map (rows sub .. sub + 31)
template <int DT>
__device__ __forceinline__ void attn_accum_cmajor(f32x16 (&acc)[DT], const float* __restrict__ tile, const f32x16& w, int sub, int fr, int h) {
#pragma unroll
  for (int u = 0; u < DT; ++u) {
    const float* a = tile + attn_cmajor_at(32 * u + fr, sub + 4 * h);
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[attn_rowmap(r, 0)], w[r], acc[u], 0, 0, 0);
  }
}

struct AttnArgs {
  const float* q;
  const float* k;
  const float* v;
  const float* scale;     // device scalar or NULL (1)
  const float* out;       // backward
  const float* lse;       // backward
  const float* dout;      // backward
  float* delta;           // backward: (B Tq)
  float* o;               // forward: out
  float* l;               // forward: lse or NULL
  float* dq;
  float* dk;
  float* dv;
  float* dsrows;          // (B Tq) or NULL
  int B, Tq, Tk, d, dvn, causal;
};

template <int DT>
__global__ __launch_bounds__(256) void attn_fwd_kernel(AttnArgs g, unsigned tiles, bool kvec, bool vvec) {
  extern __shared__ __attribute__((aligned(16))) float attn_lds[];
  float* Kc = attn_lds;
  float* Vr = attn_lds + attn_cmajor_floats(DT);
  const unsigned b = blockIdx.x / tiles;
  const int i0 = (int)(blockIdx.x % tiles) * ATTN_BQ;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, fr = lane & 31, h = lane >> 5;
  const int iw = i0 + 32 * wave, i = iw + fr;
  const float sc = g.scale ? *g.scale : 1.f;
  const float* __restrict__ q = g.q + (long long)b * g.Tq * g.d;
  const float* __restrict__ k = g.k + (long long)b * g.Tk * g.d;
  const float* __restrict__ v = g.v + (long long)b * g.Tk * g.dvn;

  float qf[16 * DT];
  attn_frag<DT>(qf, q, i, g.Tq, g.d, h);
  f32x16 O[DT];
#pragma unroll
  for (int u = 0; u < DT; ++u)
#pragma unroll
    for (int r = 0; r < 16; ++r) O[u][r] = 0.f;
  float m = -INFINITY, l = 0.f;

  const int blk_last = min(i0 + ATTN_BQ, g.Tq) - 1, wave_last = min(iw + 31, g.Tq - 1);
  int ntiles = (g.Tk + ATTN_BK - 1) / ATTN_BK;
  if (g.causal) ntiles = min(ntiles, blk_last / ATTN_BK + 1);            // key tiles wholly above the block's diagonal are not visited
  for (int kt = 0; kt < ntiles; ++kt) {
    const int j0 = kt * ATTN_BK;
    __syncthreads();                                                      // every wave has left the previous tile
    attn_stage<DT, true>(Kc, k, j0, g.Tk, g.d, kvec);
    attn_stage<DT, false>(Vr, v, j0, g.Tk, g.dvn, vvec);
    __syncthreads();
    if (iw >= g.Tq || (g.causal && j0 > wave_last)) continue;             // wave-uniform: no row of this wave sees the tile (the barriers are above)

    f32x16 S[2];
    float mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      S[t] = attn_scores<DT>(Kc, qf, 32 * t, fr, h);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int j = j0 + 32 * t + attn_rowmap(r, h);
        const bool ok = j < g.Tk && (!g.causal || j <= i);
        const float s = ok ? S[t][r] * sc : -INFINITY;
        S[t][r] = s;
        mx = fmaxf(mx, s);
      }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float mn = fmaxf(m, mx);                                        // finite: tile 0 holds key 0, which every row sees
    const float alpha = expf(m - mn);                                     // first tile: expf(-inf) = 0
    float rs = 0.f;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float p = expf(S[t][r] - mn);                               // masked: expf(-inf) = +0
        S[t][r] = p;
        rs += p;
      }
    rs += __shfl_xor(rs, 32, 64);
    l = fmaf(l, alpha, rs);
    m = mn;
#pragma unroll
    for (int u = 0; u < DT; ++u) {
#pragma unroll
      for (int r = 0; r < 16; ++r) O[u][r] *= alpha;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const float* a = Vr + attn_rmajor_at(32 * t + 4 * h, 32 * u + fr, DT);
#pragma unroll
        for (int r = 0; r < 16; ++r) O[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[attn_rowmap(r, 0) * attn_vs(DT)], S[t][r], O[u], 0, 0, 0);
      }
    }
  }

  if (i < g.Tq) {
    float* __restrict__ o = g.o + ((long long)b * g.Tq + i) * g.dvn;
#pragma unroll
    for (int u = 0; u < DT; ++u)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int c = 32 * u + attn_rowmap(r, h);
        if (c < g.dvn) o[c] = O[u][r] / l;
      }
    if (g.l && h == 0) g.l[(long long)b * g.Tq + i] = m + logf(l);
  }
}

__global__ __launch_bounds__(256) void attn_delta_kernel(const float* __restrict__ dout, const float* __restrict__ out, float* __restrict__ delta, size_t rows,
                                                         int dvn) {
  // a lane per row, ONE fma chain over c ascending from +0: the order in which the matrix cores form dP[i, j] = sum_c dO[i, c] v[j, c], so where a row's
  // p sits on one key (out = v[j] there) delta equals that dP bit for bit and dS = p (dP - delta) cancels exactly, as the composed softmax gradient does
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t o = (size_t)blockIdx.x * 256 + threadIdx.x; o < rows; o += stride) {
    const float* __restrict__ a = dout + o * dvn;
    const float* __restrict__ b = out + o * dvn;
    float acc = 0.f;
    for (int c = 0; c < dvn; ++c) acc = fmaf(a[c], b[c], acc);
    delta[o] = acc;
  }
}

template <int DT>
__global__ __launch_bounds__(256) void attn_dq_kernel(AttnArgs g, unsigned tiles, bool kvec, bool vvec) {
  extern __shared__ __attribute__((aligned(16))) float attn_lds[];
  float* Kc = attn_lds;
  float* Vc = attn_lds + attn_cmajor_floats(DT);
  const unsigned b = blockIdx.x / tiles;
  const int i0 = (int)(blockIdx.x % tiles) * ATTN_BQ;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, fr = lane & 31, h = lane >> 5;
  const int iw = i0 + 32 * wave, i = iw + fr;
  const float sc = g.scale ? *g.scale : 1.f;
  const float* __restrict__ k = g.k + (long long)b * g.Tk * g.d;
  const float* __restrict__ v = g.v + (long long)b * g.Tk * g.dvn;
  const long long row = (long long)b * g.Tq + i;

  float qf[16 * DT], gf[16 * DT];
  attn_frag<DT>(qf, g.q + (long long)b * g.Tq * g.d, i, g.Tq, g.d, h);
  attn_frag<DT>(gf, g.dout + (long long)b * g.Tq * g.dvn, i, g.Tq, g.dvn, h);
  const float lse = i < g.Tq ? g.lse[row] : INFINITY;                     // a row past Tq: p = expf(-inf) = 0
  const float del = i < g.Tq ? g.delta[row] : 0.f;
  f32x16 A[DT];
#pragma unroll
  for (int u = 0; u < DT; ++u)
#pragma unroll
    for (int r = 0; r < 16; ++r) A[u][r] = 0.f;
  float dsc = 0.f;

  const int blk_last = min(i0 + ATTN_BQ, g.Tq) - 1, wave_last = min(iw + 31, g.Tq - 1);
  int ntiles = (g.Tk + ATTN_BK - 1) / ATTN_BK;
  if (g.causal) ntiles = min(ntiles, blk_last / ATTN_BK + 1);
  for (int kt = 0; kt < ntiles; ++kt) {
    const int j0 = kt * ATTN_BK;
    __syncthreads();
    attn_stage<DT, true>(Kc, k, j0, g.Tk, g.d, kvec);
    attn_stage<DT, true>(Vc, v, j0, g.Tk, g.dvn, vvec);
    __syncthreads();
    if (iw >= g.Tq) continue;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      if (g.causal && j0 + 32 * t > wave_last) continue;                  // wave-uniform
      f32x16 S = attn_scores<DT>(Kc, qf, 32 * t, fr, h);
      const f32x16 P = attn_scores<DT>(Vc, gf, 32 * t, fr, h);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int j = j0 + 32 * t + attn_rowmap(r, h);
        const bool ok = j < g.Tk && (!g.causal || j <= i);
        const float p = ok ? expf(fmaf(S[r], sc, -lse)) : 0.f;
        const float ds = p * (P[r] - del);
        dsc = fmaf(ds, S[r], dsc);
        S[r] = ds;
      }
      attn_accum_cmajor<DT>(A, Kc, S, 32 * t, fr, h);
    }
  }
  dsc += __shfl_xor(dsc, 32, 64);

  if (i < g.Tq) {
    if (g.dq) {
      float* __restrict__ o = g.dq + row * g.d;
#pragma unroll
      for (int u = 0; u < DT; ++u)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int c = 32 * u + attn_rowmap(r, h);
          if (c < g.d) o[c] = sc * A[u][r];
        }
    }
    if (g.dsrows && h == 0) g.dsrows[row] = dsc;
  }
}

template <int DT>
__global__ __launch_bounds__(256) void attn_dkv_kernel(AttnArgs g, unsigned tiles, bool qvec, bool gvec) {
  extern __shared__ __attribute__((aligned(16))) float attn_lds[];
  float* Qc = attn_lds;
  float* Gc = attn_lds + attn_cmajor_floats(DT);
  float* Ls = Gc + attn_cmajor_floats(DT);
  float* Ds = Ls + ATTN_BK;
  const unsigned b = blockIdx.x / tiles;
  const int j0 = (int)(blockIdx.x % tiles) * ATTN_BQ;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, fr = lane & 31, h = lane >> 5;
  const int jw = j0 + 32 * wave, j = jw + fr;
  const float sc = g.scale ? *g.scale : 1.f;
  const float* __restrict__ q = g.q + (long long)b * g.Tq * g.d;
  const float* __restrict__ dout = g.dout + (long long)b * g.Tq * g.dvn;

  float kf[16 * DT], vf[16 * DT];
  attn_frag<DT>(kf, g.k + (long long)b * g.Tk * g.d, j, g.Tk, g.d, h);
  attn_frag<DT>(vf, g.v + (long long)b * g.Tk * g.dvn, j, g.Tk, g.dvn, h);
  f32x16 DK[DT], DV[DT];
#pragma unroll
  for (int u = 0; u < DT; ++u)
#pragma unroll
    for (int r = 0; r < 16; ++r) DK[u][r] = DV[u][r] = 0.f;

  const int ntiles = (g.Tq + ATTN_BK - 1) / ATTN_BK;
  for (int qt = g.causal ? j0 / ATTN_BK : 0; qt < ntiles; ++qt) {          // query tiles wholly above the block's diagonal (i < j0) are not visited
    const int i0 = qt * ATTN_BK;
    __syncthreads();
    attn_stage<DT, true>(Qc, q, i0, g.Tq, g.d, qvec);
    attn_stage<DT, true>(Gc, dout, i0, g.Tq, g.dvn, gvec);
    if (threadIdx.x < ATTN_BK) {
      const int ii = i0 + (int)threadIdx.x;
      Ls[threadIdx.x] = ii < g.Tq ? g.lse[(long long)b * g.Tq + ii] : INFINITY;      // a row past Tq: p = expf(-inf) = 0
      Ds[threadIdx.x] = ii < g.Tq ? g.delta[(long long)b * g.Tq + ii] : 0.f;
    }
    __syncthreads();
    if (jw >= g.Tk) continue;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      if (g.causal && i0 + 32 * t + 31 < jw) continue;                     // wave-uniform: every row of the sub-tile lies before every key of the wave
      f32x16 S = attn_scores<DT>(Qc, kf, 32 * t, fr, h);
      const f32x16 P = attn_scores<DT>(Gc, vf, 32 * t, fr, h);
      f32x16 Pr;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int il = 32 * t + attn_rowmap(r, h);
        const bool ok = j < g.Tk && (!g.causal || j <= i0 + il);
        const float p = ok ? expf(fmaf(S[r], sc, -Ls[il])) : 0.f;
        Pr[r] = p;
        S[r] = p * (P[r] - Ds[il]);
      }
      attn_accum_cmajor<DT>(DV, Gc, Pr, 32 * t, fr, h);
      attn_accum_cmajor<DT>(DK, Qc, S, 32 * t, fr, h);
    }
  }

  if (j < g.Tk) {
    const long long row = (long long)b * g.Tk + j;
#pragma unroll
    for (int u = 0; u < DT; ++u)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int c = 32 * u + attn_rowmap(r, h);
        if (g.dk && c < g.d) g.dk[row * g.d + c] = sc * DK[u][r];
        if (g.dv && c < g.dvn) g.dv[row * g.dvn + c] = DV[u][r];
      }
  }
}

bool attn_vec(const float* p, int ncols) { return ((uintptr_t)p & 15) == 0 && ncols % 4 == 0; }

enum { ATTN_FWD, ATTN_DQ, ATTN_DKV };

template <int DT>
void attn_launch(int which, const AttnArgs& g, unsigned tiles, hipStream_t s) {
  static unsigned long long done[3] = {0, 0, 0};
  const dim3 grid(tiles * (unsigned)g.B), block(256);
  if (which == ATTN_FWD) {
    allow_big_lds((const void*)attn_fwd_kernel<DT>, &done[0]);
    hipLaunchKernelGGL((attn_fwd_kernel<DT>), grid, block, sizeof(float) * attn_fwd_lds_floats(DT), s, g, tiles, attn_vec(g.k, g.d), attn_vec(g.v, g.dvn));
  } else if (which == ATTN_DQ) {
    allow_big_lds((const void*)attn_dq_kernel<DT>, &done[1]);
    hipLaunchKernelGGL((attn_dq_kernel<DT>), grid, block, sizeof(float) * attn_dq_lds_floats(DT), s, g, tiles, attn_vec(g.k, g.d), attn_vec(g.v, g.dvn));
  } else {
    allow_big_lds((const void*)attn_dkv_kernel<DT>, &done[2]);
    hipLaunchKernelGGL((attn_dkv_kernel<DT>), grid, block, sizeof(float) * attn_dkv_lds_floats(DT), s, g, tiles, attn_vec(g.q, g.d), attn_vec(g.dout, g.dvn));
  }
}

void attn_dispatch(int which, const AttnArgs& g, unsigned tiles, hipStream_t s) {
  switch (attn_dt(g.d, g.dvn)) {
    case 1: attn_launch<1>(which, g, tiles, s); break;
    case 2: attn_launch<2>(which, g, tiles, s); break;
    case 3: attn_launch<3>(which, g, tiles, s); break;
    default: attn_launch<4>(which, g, tiles, s); break;
  }
}

int attn_check(const char* what, int B, int Tq, int Tk, int d, int dv) {
  GN_REQUIRE(B >= 0, "%s: negative batch size %d", what, B);
  GN_REQUIRE(Tq >= 1 && Tk >= 1, "%s: Tq = %d, Tk = %d, at least 1 each", what, Tq, Tk);
  GN_REQUIRE(d >= 1 && dv >= 1 && d <= ATTN_MAX_D && dv <= ATTN_MAX_D, "%s: d = %d, dv = %d outside 1 .. %d, the widths the kernels hold on chip", what, d, dv,
             ATTN_MAX_D);
  const unsigned long long tq = cdiv((size_t)Tq, ATTN_BQ), tk = cdiv((size_t)Tk, ATTN_BQ);
  GN_REQUIRE((tq > tk ? tq : tk) * (unsigned long long)B < 0x80000000ull, "%s: %d batch entries of %d x %d rows exceed the grid (2^31 - 1 blocks)", what, B, Tq, Tk);
  return GN_OK;
}

}  // namespace
}  // namespace gn

using namespace gn;

extern "C" {

size_t gn_attention_workspace(int B, int Tq) { return B < 1 || Tq < 1 ? 0 : sizeof(float) * (size_t)B * (size_t)Tq; }

int gn_attention_fwd(const float* q, const float* k, const float* v, const float* scale, float* out, float* lse, int B, int Tq, int Tk, int d, int dv, int causal,
                     void* stream) {
  const int rc = attn_check("attention_fwd", B, Tq, Tk, d, dv);
  if (rc) return rc;
  if (B == 0) return GN_OK;
  GN_REQUIRE(q && k && v && out, "attention_fwd: null pointer");
  AttnArgs g = {};
  g.q = q; g.k = k; g.v = v; g.scale = scale; g.o = out; g.l = lse;
  g.B = B; g.Tq = Tq; g.Tk = Tk; g.d = d; g.dvn = dv; g.causal = causal != 0;
  attn_dispatch(ATTN_FWD, g, cdiv((size_t)Tq, ATTN_BQ), (hipStream_t)stream);
  return check_launch("attention_fwd");
}

int gn_attention_bwd(const float* q, const float* k, const float* v, const float* scale, const float* out, const float* lse, const float* dout, float* dq, float* dk,
                     float* dv_out, float* dscale_rows, void* ws, size_t ws_bytes, int B, int Tq, int Tk, int d, int dv, int causal, void* stream) {
  const int rc = attn_check("attention_bwd", B, Tq, Tk, d, dv);
  if (rc) return rc;
  if (B == 0 || !(dq || dk || dv_out || dscale_rows)) return GN_OK;
  GN_REQUIRE(q && k && v && out && lse && dout && ws, "attention_bwd: null pointer");
  if (ws_bytes < gn_attention_workspace(B, Tq)) {
    set_error("attention_bwd: workspace of %zu bytes, %zu needed", ws_bytes, gn_attention_workspace(B, Tq));
    return GN_EWORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  AttnArgs g = {};
  g.q = q; g.k = k; g.v = v; g.scale = scale; g.out = out; g.lse = lse; g.dout = dout; g.delta = (float*)ws;
  g.dq = dq; g.dk = dk; g.dv = dv_out; g.dsrows = dscale_rows;
  g.B = B; g.Tq = Tq; g.Tk = Tk; g.d = d; g.dvn = dv; g.causal = causal != 0;
  const size_t rows = (size_t)B * (size_t)Tq;
  hipLaunchKernelGGL(attn_delta_kernel, dim3(stream_grid(rows)), dim3(256), 0, s, dout, out, g.delta, rows, dv);
  int e = check_launch("attention_delta");
  if (e) return e;
  if (dk || dv_out) {
    attn_dispatch(ATTN_DKV, g, cdiv((size_t)Tk, ATTN_BQ), s);
    e = check_launch("attention_dkv");
    if (e) return e;
  }
  if (dq || dscale_rows) {
    attn_dispatch(ATTN_DQ, g, cdiv((size_t)Tq, ATTN_BQ), s);
    e = check_launch("attention_dq");
  }
  return e;
}

}  // extern "C"
