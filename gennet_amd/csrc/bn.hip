// BatchNormalization over the last axis, and the fixed-order fp64 column reduction it is built on.  This file owns that reduction
// (colred_run / colred_finalize: per-chunk partials in plain stores, summed in one order, so repeated runs are bit-identical); the bias
// gradients (bias_grad, also called by the convolution and Dense weight gradients in capi.hip) and the statistics epilogues of the
// convolutions (conv_pipe.hip and its kin, through colred_finalize) use it from here.  The BN backward kernels and colred_kernel<2> share
// the device helpers bn_bwd_g* and lazy_dy*, which is why statistics, apply and backward passes sit in one file.
#include "common.h"

namespace gn {

// ---------------------------------------------------------------------------------------------
// column reductions in fp64 (BatchNorm statistics, bias gradients):  x viewed as (rows, C), C % 4 == 0
// grid = (column blocks, row chunks); thread = one float4 column group x one row lane; partials [chunk][NV][C] fp64.
// MODE 0: sum x                (bias gradient)
// MODE 1: sum x, sum x^2       (BN forward statistics)
// MODE 2: sum g, sum g*xhat    (BN backward statistics; g = dy through dropout and activation)
// ---------------------------------------------------------------------------------------------

// value of g for one element (shared by backward pass 1 and 2)
__device__ __forceinline__ float bn_bwd_g(float dy, float y, uint8_t keep, int act, float p, float keep_scale) {
  if (!keep) return 0.f;
  const float yact = y / keep_scale;  // undo the inverted-dropout scale to recover the activation output
  return dy * keep_scale * act_grad_from_y(yact, act, p);
}

// the same with the activation output itself (recomputed from the pre-BN tensor) instead of the stored, dropout-scaled layer output
__device__ __forceinline__ float bn_bwd_g_act(float dy, float yact, uint8_t keep, int act, float p, float keep_scale) {
  if (!keep) return 0.f;
  return dy * keep_scale * act_grad_from_y(yact, act, p);
}

// LazyDy (common.h): the 4 channels 4q..4q+3 of one row of the data gradient of a 1-filter stride-1 conv with k <= 5 taps, from its
// output gradient g and kernel; wq holds the thread's kernel columns (taps past k are zero).
__device__ __forceinline__ void lazy_dy_taps(const LazyDy& z, int C, int q, float wq[5][4]) {
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    float4 w4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (j < z.k) w4 = *reinterpret_cast<const float4*>(z.w + (size_t)j * C + 4 * q);
    wq[j][0] = w4.x; wq[j][1] = w4.y; wq[j][2] = w4.z; wq[j][3] = w4.w;
  }
}
// A wave's window on g: lane l holds g[b, base + l] (0 outside [0, Lout)).  With C / 4 lanes per row a multiple of 64 the row is the same
// for all lanes of a wave, rows advance along the segment, and one 64-wide load serves ~60 / RL rows; the k values of a row come out
// of it by v_readlane.  (k vector loads of one address per row cost the address path as much as the 16-byte row loads themselves
// and doubled the kernels' time; scalar loads are not available next to the kernel's own global stores.)
struct LazyWin {
  float win;
  int base;
  unsigned b;
};
template <bool UNI>
__device__ __forceinline__ void lazy_dy4(const LazyDy& z, unsigned b, int t, const float wq[5][4], float v[4], LazyWin& w) {
  float gv[5];
  if (UNI) {
    b = __builtin_amdgcn_readfirstlane(b);
    t = __builtin_amdgcn_readfirstlane(t);
    const int uhi = t + z.pad_left, ulo = uhi - (z.k - 1);
    if (b != w.b || ulo < w.base || uhi >= w.base + 64) {              // wave-uniform
      w.b = b;
      w.base = ulo;
      const int idx = ulo + (int)(threadIdx.x & 63);
      w.win = (idx >= 0 && idx < z.Lout) ? z.g[(size_t)b * z.Lout + idx] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < 5; ++j)
      gv[j] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(w.win), max(uhi - j - w.base, 0)));      // taps past k: weight 0
  } else {
    const float* gb = z.g + (size_t)b * z.Lout;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      const int u = t - j + z.pad_left;
      const int uc = min(max(u, 0), z.Lout - 1);
      const float g = gb[uc];
      gv[j] = (u == uc) ? g : 0.f;
    }
  }
  v[0] = v[1] = v[2] = v[3] = 0.f;
#pragma unroll
  for (int j = 0; j < 5; ++j)
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = fmaf(gv[j], wq[j][e], v[e]);
}
// (segment, position) of row r; the row loops then step both without dividing
__device__ __forceinline__ void lazy_dy_pos(const LazyDy& z, size_t r, unsigned* b, int* t) {
  *b = (unsigned)(r / (unsigned)z.L);
  *t = (int)(r - (size_t)*b * z.L);
}
__device__ __forceinline__ void lazy_dy_step(const LazyDy& z, int step, unsigned* b, int* t) {
  *t += step;
  while (*t >= z.L) { *t -= z.L; ++*b; }
}

template <int MODE>
__global__ __launch_bounds__(256) void colred_kernel(ColRedArgs a) {
  constexpr int NV = MODE == 0 ? 1 : 2;
  const int NQ = a.C >> 2;
  const int NQc = NQ < 256 ? NQ : 256;
  const int RL = 256 / NQc;
  const int tid = threadIdx.x, ql = tid % NQc, rl = tid / NQc;
  const int q = blockIdx.x * NQc + ql;
  double s[NV][4];
#pragma unroll
  for (int v = 0; v < NV; ++v)
#pragma unroll
    for (int e = 0; e < 4; ++e) s[v][e] = 0.0;
  const size_t r_lo = (size_t)blockIdx.y * a.rows_per_chunk;
  const size_t r_hi = r_lo + a.rows_per_chunk < a.rows ? r_lo + a.rows_per_chunk : a.rows;
  if (rl < RL && q < NQ) {
    float mu[4] = {0, 0, 0, 0}, is[4] = {0, 0, 0, 0}, sc[4] = {0, 0, 0, 0}, sh[4] = {0, 0, 0, 0};
    if (MODE == 2) {
      const float4 m4 = *reinterpret_cast<const float4*>(a.mean + 4 * q), i4 = *reinterpret_cast<const float4*>(a.invstd + 4 * q);
      mu[0] = m4.x; mu[1] = m4.y; mu[2] = m4.z; mu[3] = m4.w;
      is[0] = i4.x; is[1] = i4.y; is[2] = i4.z; is[3] = i4.w;
      if (a.scale) {
        const float4 c4 = *reinterpret_cast<const float4*>(a.scale + 4 * q), h4 = *reinterpret_cast<const float4*>(a.shift + 4 * q);
        sc[0] = c4.x; sc[1] = c4.y; sc[2] = c4.z; sc[3] = c4.w;
        sh[0] = h4.x; sh[1] = h4.y; sh[2] = h4.z; sh[3] = h4.w;
      }
    }
    float wq[5][4];
    LazyWin lw = {0.f, 0, 0xffffffffu};
    const bool lazy = MODE == 2 && a.lz.g != nullptr;
    unsigned lb = 0;
    int lt = 0;
    if (lazy) {
      lazy_dy_taps(a.lz, a.C, q, wq);
      lazy_dy_pos(a.lz, r_lo + rl, &lb, &lt);
    }
    // U rows per trip with all their loads issued before the first use.  Measured on the generator's largest BatchNormalization
    // (1 M rows x 1024 channels): U = 4 is SLOWER than U = 1 (146 VGPRs, 3 waves per SIMD: 6.6 against 6.2 ms for the backward pair) --
    // the pass is bound by its arithmetic (tanh recomputation, fp64 sums), not by load latency.
    constexpr int U = 2;
    for (size_t r = r_lo + rl; r < r_hi; r += (size_t)RL * U) {
      float4 v4[U], x4[U], y4[U];
      uchar4 m4[U];
      bool ok[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const size_t ru = r + (size_t)u * RL;
        ok[u] = ru < r_hi;
        const size_t o = (ok[u] ? ru : r) * a.C + 4 * q;
        if (!lazy) v4[u] = *reinterpret_cast<const float4*>(a.a + o);
        if (MODE == 2) {
          x4[u] = *reinterpret_cast<const float4*>(a.xpre + o);
          if (!a.scale) y4[u] = *reinterpret_cast<const float4*>(a.y + o);
          m4[u] = a.mask ? *reinterpret_cast<const uchar4*>(a.mask + o) : make_uchar4(1, 1, 1, 1);
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (!ok[u]) break;
        float v[4];
        if (lazy) {
          if (((NQc | NQ) & 63) == 0) lazy_dy4<true>(a.lz, lb, lt, wq, v, lw);
          else lazy_dy4<false>(a.lz, lb, lt, wq, v, lw);
          lazy_dy_step(a.lz, RL, &lb, &lt);
        } else {
          v[0] = v4[u].x; v[1] = v4[u].y; v[2] = v4[u].z; v[3] = v4[u].w;
        }
        if (MODE == 0) {
#pragma unroll
          for (int e = 0; e < 4; ++e) s[0][e] += (double)v[e];
        } else if (MODE == 1) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            s[0][e] += (double)v[e];
            s[1][e] += (double)v[e] * (double)v[e];
          }
        } else {
          const float xv[4] = {x4[u].x, x4[u].y, x4[u].z, x4[u].w};
          float yv[4];
          if (a.scale) {        // activation output recomputed from the pre-BN tensor: one 4-byte read per element less
#pragma unroll
            for (int e = 0; e < 4; ++e) yv[e] = act_apply(fmaf(xv[e], sc[e], sh[e]), a.act, a.act_param);
          } else {
            yv[0] = y4[u].x; yv[1] = y4[u].y; yv[2] = y4[u].z; yv[3] = y4[u].w;
          }
          const uint8_t k[4] = {m4[u].x, m4[u].y, m4[u].z, m4[u].w};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float g = a.scale ? bn_bwd_g_act(v[e], yv[e], k[e], a.act, a.act_param, a.keep_scale)
                                    : bn_bwd_g(v[e], yv[e], k[e], a.act, a.act_param, a.keep_scale);
            const float xh = (xv[e] - mu[e]) * is[e];
            s[0][e] += (double)g;
            s[NV - 1][e] += (double)g * (double)xh;
          }
        }
      }
    }
  }
  __shared__ double red[256 * 4];
#pragma unroll
  for (int v = 0; v < NV; ++v) {
#pragma unroll
    for (int e = 0; e < 4; ++e) red[tid * 4 + e] = s[v][e];
    __syncthreads();
    if (rl == 0 && q < NQ) {
      double t[4] = {red[ql * 4], red[ql * 4 + 1], red[ql * 4 + 2], red[ql * 4 + 3]};
      for (int k = 1; k < RL; ++k)
#pragma unroll
        for (int e = 0; e < 4; ++e) t[e] += red[(k * NQc + ql) * 4 + e];
      double* d = a.part + ((size_t)blockIdx.y * NV + v) * a.C + 4 * q;
#pragma unroll
      for (int e = 0; e < 4; ++e) d[e] = t[e];
    }
    __syncthreads();
  }
}

// C % 4 != 0: the same reduction with a thread on ONE column (scalar loads) x one row lane; grid = (column blocks, row chunks), partials
// [chunk][NV][C] as above, so colred_final_kernel sums them in the same fixed order.  (No on-the-fly conv gradient here: lazy_dy_check
// requires C % 4 == 0.)
template <int MODE>
__global__ __launch_bounds__(256) void colred_anyc_kernel(ColRedArgs a) {
  constexpr int NV = MODE == 0 ? 1 : 2;
  const int NCc = a.C < 256 ? a.C : 256;
  const int RL = 256 / NCc;
  const int tid = threadIdx.x, cl = tid % NCc, rl = tid / NCc;
  const int c = blockIdx.x * NCc + cl;
  double s[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) s[v] = 0.0;
  const size_t r_lo = (size_t)blockIdx.y * a.rows_per_chunk;
  const size_t r_hi = r_lo + a.rows_per_chunk < a.rows ? r_lo + a.rows_per_chunk : a.rows;
  if (rl < RL && c < a.C) {
    float mu = 0.f, is = 0.f, sc = 0.f, sh = 0.f;
    if (MODE == 2) {
      mu = a.mean[c]; is = a.invstd[c];
      if (a.scale) { sc = a.scale[c]; sh = a.shift[c]; }
    }
    for (size_t r = r_lo + rl; r < r_hi; r += RL) {
      const size_t o = r * a.C + c;
      const float v = a.a[o];
      if (MODE == 0) {
        s[0] += (double)v;
      } else if (MODE == 1) {
        s[0] += (double)v;
        s[NV - 1] += (double)v * (double)v;
      } else {
        const float xv = a.xpre[o];
        const uint8_t k = a.mask ? a.mask[o] : (uint8_t)1;
        const float g = a.scale ? bn_bwd_g_act(v, act_apply(fmaf(xv, sc, sh), a.act, a.act_param), k, a.act, a.act_param, a.keep_scale)
                                : bn_bwd_g(v, a.y[o], k, a.act, a.act_param, a.keep_scale);
        const float xh = (xv - mu) * is;
        s[0] += (double)g;
        s[NV - 1] += (double)g * (double)xh;
      }
    }
  }
  __shared__ double red[256];
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    red[tid] = s[v];
    __syncthreads();
    if (rl == 0 && c < a.C) {
      double t = red[cl];
      for (int k = 1; k < RL; ++k) t += red[k * NCc + cl];
      a.part[((size_t)blockIdx.y * NV + v) * a.C + c] = t;
    }
    __syncthreads();
  }
}

// sum the chunk partials: block = 32 columns x 8 chunk lanes; lane l adds chunks l, l+8, ... then the 8 lane sums are added in
// lane order (fixed order -> bitwise reproducible)
template <typename OUT, int COLS>
__global__ __launch_bounds__(256) void colred_final_kernel(const double* __restrict__ part, OUT* __restrict__ out, size_t n, int chunks) {
  constexpr int LANES = 256 / COLS;
  const int col = threadIdx.x % COLS, lane = threadIdx.x / COLS;
  const size_t i = (size_t)blockIdx.x * COLS + col;
  double s = 0.0;
  if (i < n)
    for (int k = lane; k < chunks; k += LANES) s += part[(size_t)k * n + i];
  __shared__ double red[LANES][COLS + 1];
  red[lane][col] = s;
  __syncthreads();
  if (lane == 0 && i < n) {
    double t = red[0][col];
    for (int l = 1; l < LANES; ++l) t += red[l][col];
    out[i] = (OUT)t;
  }
}
// 32 columns x 8 lanes per block; with many partial rows and few columns (the per-block partials of the conv epilogue: 4096 rows x 2048
// columns ran on 64 blocks) 8 columns x 32 lanes, four times the blocks and a quarter of the serial adds per thread
template <typename OUT>
static void colred_final_launch(const double* part, OUT* out, size_t n, int chunks, hipStream_t s) {
  if (chunks >= 256 && n <= 16384) hipLaunchKernelGGL((colred_final_kernel<OUT, 8>), dim3(cdiv(n, 8)), dim3(256), 0, s, part, out, n, chunks);
  else hipLaunchKernelGGL((colred_final_kernel<OUT, 32>), dim3(cdiv(n, 32)), dim3(256), 0, s, part, out, n, chunks);
}

static int colred_chunks(size_t rows, int C) {
  if (C % 4) {                                          // colred_anyc_kernel: one column per thread, RL rows per block
    const int NCc = C < 256 ? C : 256, RL = 256 / NCc;
    const int gx = (C + NCc - 1) / NCc;
    int chunks = (1024 + gx - 1) / gx;
    const size_t max_chunks = (rows + (size_t)RL * 4 - 1) / ((size_t)RL * 4);
    if ((size_t)chunks > max_chunks) chunks = (int)max_chunks;
    return chunks < 1 ? 1 : chunks;
  }
  const int NQ = C / 4, NQc = NQ < 256 ? NQ : 256, RL = 256 / NQc;
  const int gx = (NQ + NQc - 1) / NQc;
  int chunks = (1024 + gx - 1) / gx;
  const size_t max_chunks = (rows + (size_t)RL * 4 - 1) / ((size_t)RL * 4);
  if ((size_t)chunks > max_chunks) chunks = (int)max_chunks;
  if (chunks < 1) chunks = 1;
  return chunks;
}
size_t colred_workspace_bytes(size_t rows, int C) { return (size_t)colred_chunks(rows, C) * 2 * C * sizeof(double); }

// out_f64 (NV*C doubles) or out_f32 (MODE 0 only) receives the reduced sums
int colred_run(int mode, ColRedArgs a, void* ws, size_t ws_bytes, double* out_f64, float* out_f32, hipStream_t s) {
  if (a.C < 1) { set_error("column reduction: C %d", a.C); return GN_EINVAL; }
  if (a.C % 4 && a.lz.g) { set_error("column reduction: the on-the-fly conv gradient needs C %% 4 == 0"); return GN_EINVAL; }
  if (a.rows == 0) { set_error("column reduction: no rows"); return GN_EINVAL; }
  const int chunks = colred_chunks(a.rows, a.C);
  const int NV = mode == 0 ? 1 : 2;
  if (ws_bytes < (size_t)chunks * NV * a.C * sizeof(double)) { set_error("column reduction: workspace too small"); return GN_EWORKSPACE; }
  a.part = (double*)ws;
  a.rows_per_chunk = (int)((a.rows + chunks - 1) / chunks);
  if (a.C % 4) {
    const int NCc = a.C < 256 ? a.C : 256;
    dim3 grid((a.C + NCc - 1) / NCc, chunks);
    if (mode == 0) hipLaunchKernelGGL(colred_anyc_kernel<0>, grid, dim3(256), 0, s, a);
    else if (mode == 1) hipLaunchKernelGGL(colred_anyc_kernel<1>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(colred_anyc_kernel<2>, grid, dim3(256), 0, s, a);
  } else {
    const int NQ = a.C / 4, NQc = NQ < 256 ? NQ : 256;
    dim3 grid((NQ + NQc - 1) / NQc, chunks);
    if (mode == 0) hipLaunchKernelGGL(colred_kernel<0>, grid, dim3(256), 0, s, a);
    else if (mode == 1) hipLaunchKernelGGL(colred_kernel<1>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(colred_kernel<2>, grid, dim3(256), 0, s, a);
  }
  int rc = check_launch("colred");
  if (rc) return rc;
  const size_t n = (size_t)NV * a.C;
  if (out_f32) colred_final_launch((const double*)ws, out_f32, n, chunks, s);
  else colred_final_launch((const double*)ws, out_f64, n, chunks, s);
  return check_launch("colred_final");
}

int colred_finalize(const double* part, double* out_f64, size_t n, int chunks, hipStream_t s) {
  colred_final_launch(part, out_f64, n, chunks, s);
  return check_launch("colred_final");
}
int colred_finalize_f32(const double* part, float* out_f32, size_t n, int chunks, hipStream_t s) {
  colred_final_launch(part, out_f32, n, chunks, s);
  return check_launch("colred_final");
}

// small C (< 4 or not a multiple of 4) column sums: fp64 block partials + fp64 atomics
__global__ void colsum_anyc_kernel(const float* __restrict__ x, double* __restrict__ acc, size_t n, int C) {
  double s[4] = {0, 0, 0, 0};
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int c = (int)(i % C);
    const double v = (double)x[i];
    s[0] += c == 0 ? v : 0.0; s[1] += c == 1 ? v : 0.0; s[2] += c == 2 ? v : 0.0; s[3] += c == 3 ? v : 0.0;
  }
  __shared__ double red[4][256];
  for (int c = 0; c < 4; ++c) red[c][threadIdx.x] = s[c];
  __syncthreads();
  for (int sft = 128; sft >= 1; sft >>= 1) {
    if (threadIdx.x < sft)
      for (int c = 0; c < 4; ++c) red[c][threadIdx.x] += red[c][threadIdx.x + sft];
    __syncthreads();
  }
  if (threadIdx.x < C) atomicAdd(&acc[threadIdx.x], red[threadIdx.x][0]);
}
__global__ void f64_to_f32_small_kernel(const double* __restrict__ a, float* __restrict__ o, int n) {
  if ((int)threadIdx.x < n) o[threadIdx.x] = (float)a[threadIdx.x];
}

// db[c] = sum over rows of dy[row, c]; ws needs colred_workspace_bytes(rows, C) (C % 4 == 0 or C > 4) or 32 bytes otherwise.  C > 4 runs
// the fixed-order column reduction (colred_run: its any-C kernel when C % 4 != 0), so repeated runs are bit-identical.
int bias_grad(const float* dy, float* db, size_t rows, int C, void* ws, size_t ws_bytes, hipStream_t s) {
  if (C % 4 == 0 || C > 4) {
    ColRedArgs r = {};
    r.a = dy; r.rows = rows; r.C = C;
    return colred_run(0, r, ws, ws_bytes, nullptr, db, s);
  }
  if (ws_bytes < 32) { set_error("bias_grad: workspace too small"); return GN_EWORKSPACE; }
  (void)hipMemsetAsync(ws, 0, 32, s);
  size_t g = (rows * C + 255) / 256;
  if (g > 1024) g = 1024;
  hipLaunchKernelGGL(colsum_anyc_kernel, dim3((unsigned)g), dim3(256), 0, s, dy, (double*)ws, rows * C, C);
  hipLaunchKernelGGL(f64_to_f32_small_kernel, dim3(1), dim3(64), 0, s, (const double*)ws, db, C);
  return check_launch("bias_grad");
}

size_t bias_grad_ws(size_t rows, int C) { return C % 4 == 0 || C > 4 ? colred_workspace_bytes(rows, C) : 32; }

// ---------------------------------------------------------------------------------------------
// BatchNorm finalize / apply / backward-apply
// ---------------------------------------------------------------------------------------------
// moving statistics, two forms of TF's assign_moving_average (fp32 variables, like TF's):
//   zd_step == 0 : plain EMA (zero_debias=False):  v -= (v - value) * (1 - m)
//   zd_step >= 1 : zero_debias=True (keras 2.2.4's TF backend): biased -= (biased - value) * (1 - m);  v -= v - biased / (1 - m^step)
//                  with `biased` a shadow accumulator that starts at zero and zd_step the already incremented local_step
__global__ void bn_finalize_kernel(const double* __restrict__ sums, double count, const float* __restrict__ gamma, const float* __restrict__ beta,
                                   float eps, float momentum, float* __restrict__ mm, float* __restrict__ mv, float* __restrict__ bm,
                                   float* __restrict__ bv, float zd_step, float* __restrict__ scale,
                                   float* __restrict__ shift, float* __restrict__ smean, float* __restrict__ sinv, int C, const int32_t* __restrict__ zd_step_dev) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  if (zd_step_dev) zd_step = (float)*zd_step_dev;
  const double mean = sums[c] / count;
  double var = sums[C + c] / count - mean * mean;
  if (var < 0) var = 0;
  const float meanf = (float)mean, varf = (float)var;
  const float inv = 1.0f / sqrtf(varf + eps);
  const float sc = gamma[c] * inv;
  scale[c] = sc;
  shift[c] = beta[c] - meanf * sc;
  smean[c] = meanf;
  sinv[c] = inv;
  if (mm) {
    const float corr = (float)(count / (count - (1.0 + (double)eps)));
    const float decay = (float)(1.0 - (double)momentum);
    const float varc = varf * corr;
    if (bm) {
      const float nbm = bm[c] - (bm[c] - meanf) * decay;
      const float nbv = bv[c] - (bv[c] - varc) * decay;
      bm[c] = nbm;
      bv[c] = nbv;
      const float unb = 1.0f - powf(1.0f - decay, zd_step);
      mm[c] = mm[c] - (mm[c] - nbm / unb);
      mv[c] = mv[c] - (mv[c] - nbv / unb);
    } else {
      mm[c] = mm[c] - (mm[c] - meanf) * decay;
      mv[c] = mv[c] - (mv[c] - varc) * decay;
    }
  }
}
static int bn_finalize(const double* sums, double count, const float* gamma, const float* beta, float eps, float momentum, float* mm, float* mv,
                float* bm, float* bv, float zd_step, float* scale, float* shift, float* smean, float* sinv, int C, hipStream_t s, const int32_t* zd_step_dev = nullptr) {
  hipLaunchKernelGGL(bn_finalize_kernel, dim3(cdiv(C, 256)), dim3(256), 0, s, sums, count, gamma, beta, eps, momentum, mm, mv, bm, bv, zd_step, scale, shift,
                     smean, sinv, C, zd_step_dev);
  return check_launch("bn_finalize");
}

__global__ void bn_infer_coeffs_kernel(const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ mm,
                                       const float* __restrict__ mv, float eps, float* __restrict__ scale, float* __restrict__ shift, int C) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float sc = gamma[c] / sqrtf(mv[c] + eps);
  scale[c] = sc;
  shift[c] = beta[c] - mm[c] * sc;
}

__global__ void bn_apply_kernel(const float4* __restrict__ x, const float4* __restrict__ scale, const float4* __restrict__ shift,
                                const uchar4* __restrict__ mask, float4* __restrict__ y, size_t n4, int C4, int act, float p, float keep_scale) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    const int c = (int)(i % C4);
    const float4 v = x[i], sc = scale[c], sh = shift[c];
    float4 o;
    o.x = act_apply(fmaf(v.x, sc.x, sh.x), act, p); o.y = act_apply(fmaf(v.y, sc.y, sh.y), act, p);
    o.z = act_apply(fmaf(v.z, sc.z, sh.z), act, p); o.w = act_apply(fmaf(v.w, sc.w, sh.w), act, p);
    if (mask) {
      const uchar4 m = mask[i];
      o.x = m.x ? o.x * keep_scale : 0.f; o.y = m.y ? o.y * keep_scale : 0.f;
      o.z = m.z ? o.z * keep_scale : 0.f; o.w = m.w ? o.w * keep_scale : 0.f;
    }
    y[i] = o;
  }
}
// C % 4 != 0: one element per thread, the same arithmetic
__global__ void bn_apply_anyc_kernel(const float* __restrict__ x, const float* __restrict__ scale, const float* __restrict__ shift,
                                     const uint8_t* __restrict__ mask, float* __restrict__ y, size_t n, int C, int act, float p, float keep_scale) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int c = (int)(i % C);
    float o = act_apply(fmaf(x[i], scale[c], shift[c]), act, p);
    if (mask) o = mask[i] ? o * keep_scale : 0.f;
    y[i] = o;
  }
}

__global__ void bn_bwd_apply_kernel(const float* __restrict__ dy, const float* __restrict__ y, const float* __restrict__ x, const uint8_t* __restrict__ mask,
                                    const float* __restrict__ gamma, const float* __restrict__ mean, const float* __restrict__ invstd,
                                    const double* __restrict__ dsums, double count, float* __restrict__ dx, size_t n, int C, int act, float p, float keep_scale,
                                    const float* __restrict__ scale, const float* __restrict__ shift) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int c = (int)(i % C);
    const uint8_t keep = mask ? mask[i] : (uint8_t)1;
    const float g = scale ? bn_bwd_g_act(dy[i], act_apply(fmaf(x[i], scale[c], shift[c]), act, p), keep, act, p, keep_scale)   // as the v4 kernel
                          : bn_bwd_g(dy[i], y[i], keep, act, p, keep_scale);
    const float inv = invstd[c];
    const float xh = (x[i] - mean[c]) * inv;
    const float mg = (float)(dsums[c] / count), mgx = (float)(dsums[C + c] / count);
    dx[i] = gamma[c] * inv * (g - mg - xh * mgx);
  }
}
// C % 4 == 0: a thread owns ONE group of four channels (its seven per-channel constants stay in registers: no modulo, no fp64
// division per element) and walks the rows of its chunk with 16-byte loads / stores; with scale / shift the activation output
// is recomputed from x instead of read (17 -> 13 bytes per element).  Same arithmetic per element as the scalar kernel.
__global__ __launch_bounds__(256) void bn_bwd_apply_v4_kernel(const float* __restrict__ dy, const float* __restrict__ y, const float* __restrict__ x,
                                                              const uint8_t* __restrict__ mask, const float* __restrict__ gamma, const float* __restrict__ mean,
                                                              const float* __restrict__ invstd, const double* __restrict__ dsums, double count,
                                                              const float* __restrict__ scale, const float* __restrict__ shift, float* __restrict__ dx,
                                                              size_t rows, int C, int rows_per_chunk, int act, float p, float keep_scale, LazyDy lz) {
  const int NQ = C >> 2;
  const int NQc = NQ < 256 ? NQ : 256;
  const int RL = 256 / NQc;
  const int tid = threadIdx.x, ql = tid % NQc, rl = tid / NQc;
  const int qblocks = (NQ + NQc - 1) / NQc;
  const int q = (blockIdx.x % qblocks) * NQc + ql;
  const size_t r_lo = (size_t)(blockIdx.x / qblocks) * rows_per_chunk;
  const size_t r_hi = r_lo + rows_per_chunk < rows ? r_lo + rows_per_chunk : rows;
  if (rl >= RL || q >= NQ) return;
  float gi[4], mu[4], is[4], mg[4], mgx[4], sc[4] = {0, 0, 0, 0}, sh[4] = {0, 0, 0, 0};
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int c = 4 * q + e;
    is[e] = invstd[c]; mu[e] = mean[c]; gi[e] = gamma[c] * is[e];
    mg[e] = (float)(dsums[c] / count); mgx[e] = (float)(dsums[C + c] / count);
    if (scale) { sc[e] = scale[c]; sh[e] = shift[c]; }
  }
  float wq[5][4];
  LazyWin lw = {0.f, 0, 0xffffffffu};
  unsigned lb = 0;
  int lt = 0;
  if (lz.g) {
    lazy_dy_taps(lz, C, q, wq);
    lazy_dy_pos(lz, r_lo + rl, &lb, &lt);
  }
  constexpr int U = 2;                                   // rows per trip, loads first (see colred_kernel: more is slower)
  const bool uni = ((NQc | NQ) & 63) == 0;
  for (size_t r = r_lo + rl; r < r_hi; r += (size_t)RL * U) {
    float4 d4[U], x4[U], y4[U];
    uchar4 m4[U];
    bool ok[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const size_t ru = r + (size_t)u * RL;
      ok[u] = ru < r_hi;
      const size_t o = (ok[u] ? ru : r) * C + 4 * q;
      x4[u] = *reinterpret_cast<const float4*>(x + o);
      if (!lz.g) d4[u] = *reinterpret_cast<const float4*>(dy + o);
      if (!scale) y4[u] = *reinterpret_cast<const float4*>(y + o);
      m4[u] = mask ? *reinterpret_cast<const uchar4*>(mask + o) : make_uchar4(1, 1, 1, 1);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (!ok[u]) break;
      const size_t o = (r + (size_t)u * RL) * C + 4 * q;
      const float xv[4] = {x4[u].x, x4[u].y, x4[u].z, x4[u].w};
      float dv[4];
      if (lz.g) {
        if (uni) lazy_dy4<true>(lz, lb, lt, wq, dv, lw);
        else lazy_dy4<false>(lz, lb, lt, wq, dv, lw);
        lazy_dy_step(lz, RL, &lb, &lt);
      } else {
        dv[0] = d4[u].x; dv[1] = d4[u].y; dv[2] = d4[u].z; dv[3] = d4[u].w;
      }
      float yv[4] = {0, 0, 0, 0};
      if (!scale) { yv[0] = y4[u].x; yv[1] = y4[u].y; yv[2] = y4[u].z; yv[3] = y4[u].w; }
      const uint8_t k[4] = {m4[u].x, m4[u].y, m4[u].z, m4[u].w};
      float ov[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float g = scale ? bn_bwd_g_act(dv[e], act_apply(fmaf(xv[e], sc[e], sh[e]), act, p), k[e], act, p, keep_scale)
                              : bn_bwd_g(dv[e], yv[e], k[e], act, p, keep_scale);
        const float xh = (xv[e] - mu[e]) * is[e];
        ov[e] = gi[e] * (g - mg[e] - xh * mgx[e]);
      }
      *reinterpret_cast<float4*>(dx + o) = make_float4(ov[0], ov[1], ov[2], ov[3]);
    }
  }
}
__global__ void bn_param_grads_kernel(const double* __restrict__ dsums_local, float* __restrict__ dgamma, float* __restrict__ dbeta, int C) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  dbeta[c] = (float)dsums_local[c];
  dgamma[c] = (float)dsums_local[C + c];
}
static int bn_bwd_apply(const float* dy, const float* y, const float* x, const uint8_t* mask, const float* gamma, const float* mean, const float* invstd,
                 const double* dsums_global, double count, const double* dsums_local, float* dx, float* dgamma, float* dbeta, size_t rows, int C,
                 int act, float p, float rate, const float* scale, const float* shift, hipStream_t s, const LazyDy* lz = nullptr) {
  const size_t n = rows * C;
  if (!n) return GN_OK;
  LazyDy z = {};
  if (lz) z = *lz;
  if (z.g && (C % 4 || !scale)) { set_error("bn_bwd_apply: the on-the-fly conv gradient needs C %% 4 == 0 and scale / shift"); return GN_EINVAL; }
  if (C % 4 == 0) {
    const int NQ = C / 4, NQc = NQ < 256 ? NQ : 256, RL = 256 / NQc, qblocks = cdiv(NQ, NQc);
    size_t chunks = 8192 / qblocks;                       // ~8k blocks: 32 per CU
    if (chunks < 1) chunks = 1;
    size_t rpc = (rows + chunks - 1) / chunks;
    rpc = ((rpc + RL - 1) / RL) * RL;
    if (rpc < (size_t)RL) rpc = RL;
    chunks = (rows + rpc - 1) / rpc;
    hipLaunchKernelGGL(bn_bwd_apply_v4_kernel, dim3((unsigned)(chunks * qblocks)), dim3(256), 0, s, dy, y, x, mask, gamma, mean, invstd, dsums_global, count, scale,
                       shift, dx, rows, C, (int)rpc, act, p, 1.0f / (1.0f - rate), z);
  } else {
    if (!y && !scale) { set_error("bn_bwd_apply: C %d %% 4 != 0 needs the stored layer output y or scale / shift", C); return GN_EINVAL; }
    hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(stream_grid(n)), dim3(256), 0, s, dy, y, x, mask, gamma, mean, invstd, dsums_global, count, dx, n, C, act, p,
                       1.0f / (1.0f - rate), y ? nullptr : scale, y ? nullptr : shift);     // a stored output is read as before
  }
  int rc = check_launch("bn_bwd_apply");
  if (rc) return rc;
  hipLaunchKernelGGL(bn_param_grads_kernel, dim3(cdiv(C, 256)), dim3(256), 0, s, dsums_local, dgamma, dbeta, C);
  return check_launch("bn_param_grads");
}

// the conv description of the *_conv1 entry points (LazyDy, common.h)
static int lazy_dy_check(const char* who, const float* g, const float* w, int L, int Lout, int k, int pad_left, size_t rows, int C, const float* scale,
                         const float* shift, LazyDy* z) {
  GN_REQUIRE(g && w && L > 0 && Lout > 0 && k >= 1 && k <= 5 && pad_left >= 0, "%s: bad conv description (1 filter, 1..5 taps, stride 1)", who);
  GN_REQUIRE(C % 4 == 0 && scale && shift, "%s: needs C %% 4 == 0 and the forward pass' scale / shift", who);
  GN_REQUIRE(rows % (size_t)L == 0 && rows / (size_t)L < 0x7fffffffull, "%s: rows %zu is not a whole number of length-%d segments", who, rows, L);
  z->g = g; z->w = w; z->L = L; z->Lout = Lout; z->k = k; z->pad_left = pad_left;
  return GN_OK;
}

}  // namespace gn

using namespace gn;

extern "C" {

size_t gn_bn_stats_workspace(size_t rows, int C) { return colred_workspace_bytes(rows, C) + 256; }

int gn_bn_stats(const float* x, size_t rows, int C, double* sums, void* ws, size_t ws_bytes, void* stream) {
  GN_REQUIRE(x && sums && ws && rows > 0 && C > 0, "bn_stats: bad arguments");
  ColRedArgs r = {};
  r.a = x; r.rows = rows; r.C = C;
  return colred_run(1, r, ws, ws_bytes, sums, nullptr, (hipStream_t)stream);
}

int gn_bn_finalize(const double* sums, double count, const float* gamma, const float* beta, float eps, float momentum, float* moving_mean, float* moving_var,
                   float* scale, float* shift, float* save_mean, float* save_invstd, int C, void* stream) {
  GN_REQUIRE(sums && gamma && beta && scale && shift && save_mean && save_invstd && C > 0 && count > 1.0, "bn_finalize: bad arguments");
  GN_REQUIRE((moving_mean == nullptr) == (moving_var == nullptr), "bn_finalize: moving_mean/moving_var must both be given or both be NULL");
  return bn_finalize(sums, count, gamma, beta, eps, momentum, moving_mean, moving_var, nullptr, nullptr, 0.f, scale, shift, save_mean, save_invstd, C,
                     (hipStream_t)stream);
}
int gn_bn_finalize_zero_debias(const double* sums, double count, const float* gamma, const float* beta, float eps, float momentum, float* moving_mean,
                               float* moving_var, float* biased_mean, float* biased_var, int local_step, float* scale, float* shift, float* save_mean,
                               float* save_invstd, int C, void* stream) {
  GN_REQUIRE(sums && gamma && beta && scale && shift && save_mean && save_invstd && C > 0 && count > 1.0, "bn_finalize_zero_debias: bad arguments");
  GN_REQUIRE(moving_mean && moving_var && biased_mean && biased_var && local_step >= 1,
             "bn_finalize_zero_debias: needs moving_mean/var, the biased accumulators and the incremented local_step (>= 1, got %d)", local_step);
  return bn_finalize(sums, count, gamma, beta, eps, momentum, moving_mean, moving_var, biased_mean, biased_var, (float)local_step, scale, shift, save_mean,
                     save_invstd, C, (hipStream_t)stream);
}
// local_step from device memory: what a captured hipGraph of a train step needs (a by-value argument is frozen at capture)
int gn_bn_finalize_zero_debias_dyn(const double* sums, double count, const float* gamma, const float* beta, float eps, float momentum, float* moving_mean,
                                   float* moving_var, float* biased_mean, float* biased_var, const int32_t* local_step_dev, float* scale, float* shift,
                                   float* save_mean, float* save_invstd, int C, void* stream) {
  GN_REQUIRE(sums && gamma && beta && scale && shift && save_mean && save_invstd && C > 0 && count > 1.0, "bn_finalize_zero_debias_dyn: bad arguments");
  GN_REQUIRE(moving_mean && moving_var && biased_mean && biased_var && local_step_dev, "bn_finalize_zero_debias_dyn: needs moving statistics, accumulators, step");
  return bn_finalize(sums, count, gamma, beta, eps, momentum, moving_mean, moving_var, biased_mean, biased_var, 1.f, scale, shift, save_mean, save_invstd, C,
                     (hipStream_t)stream, local_step_dev);
}

int gn_bn_infer_coeffs(const float* gamma, const float* beta, const float* moving_mean, const float* moving_var, float eps, float* scale, float* shift, int C,
                       void* stream) {
  GN_REQUIRE(gamma && beta && moving_mean && moving_var && scale && shift && C > 0, "bn_infer_coeffs: bad arguments");
  hipLaunchKernelGGL(bn_infer_coeffs_kernel, dim3(cdiv(C, 256)), dim3(256), 0, (hipStream_t)stream, gamma, beta, moving_mean, moving_var, eps, scale, shift, C);
  return check_launch("bn_infer_coeffs");
}

int gn_bn_apply(const float* x, const float* scale, const float* shift, const uint8_t* mask, float* y, size_t rows, int C, int act, float p, float rate,
                void* stream) {
  GN_REQUIRE(x && scale && shift && y && C > 0, "bn_apply: bad arguments");
  GN_REQUIRE(rate >= 0.f && rate < 1.f && (mask || rate == 0.f), "bn_apply: dropout rate %f without mask", rate);
  hipStream_t s = (hipStream_t)stream;
  const float keep_scale = 1.0f / (1.0f - (mask ? rate : 0.f));
  if (C % 4) {
    const size_t n = rows * C;
    if (!n) return GN_OK;
    hipLaunchKernelGGL(bn_apply_anyc_kernel, dim3(stream_grid(n)), dim3(256), 0, s, x, scale, shift, mask, y, n, C, act, p, keep_scale);
    return check_launch("bn_apply");
  }
  const size_t n4 = rows * (C / 4);
  if (!n4) return GN_OK;
  hipLaunchKernelGGL(bn_apply_kernel, dim3(stream_grid(n4)), dim3(256), 0, s, (const float4*)x, (const float4*)scale, (const float4*)shift, (const uchar4*)mask,
                     (float4*)y, n4, C / 4, act, p, keep_scale);
  return check_launch("bn_apply");
}

int gn_bn_bwd_stats(const float* dy, const float* y, const float* x, const uint8_t* mask, const float* save_mean, const float* save_invstd, double* dsums, void* ws,
                    size_t ws_bytes, size_t rows, int C, int act, float p, float rate, const float* scale, const float* shift, void* stream) {
  GN_REQUIRE(dy && x && save_mean && save_invstd && dsums && ws && rows > 0 && C > 0, "bn_bwd_stats: bad arguments");
  GN_REQUIRE((scale == nullptr) == (shift == nullptr) && (y || scale), "bn_bwd_stats: needs the layer output y, or scale AND shift to recompute it");
  ColRedArgs r = {};
  r.a = dy; r.y = y; r.xpre = x; r.mask = mask; r.mean = save_mean; r.invstd = save_invstd; r.scale = scale; r.shift = shift;
  r.rows = rows; r.C = C; r.act = act; r.act_param = p; r.keep_scale = 1.0f / (1.0f - (mask ? rate : 0.f));
  return colred_run(2, r, ws, ws_bytes, dsums, nullptr, (hipStream_t)stream);
}
int gn_bn_bwd_apply(const float* dy, const float* y, const float* x, const uint8_t* mask, const float* gamma, const float* save_mean, const float* save_invstd,
                    const double* dsums_global, double count, const double* dsums_local, float* dx, float* dgamma, float* dbeta, size_t rows, int C, int act,
                    float p, float rate, const float* scale, const float* shift, void* stream) {
  GN_REQUIRE(dy && x && gamma && save_mean && save_invstd && dsums_global && dsums_local && dx && dgamma && dbeta && C > 0, "bn_bwd_apply: bad arguments");
  GN_REQUIRE((scale == nullptr) == (shift == nullptr) && (y || scale), "bn_bwd_apply: needs the layer output y, or scale AND shift to recompute it");
  return bn_bwd_apply(dy, y, x, mask, gamma, save_mean, save_invstd, dsums_global, count, dsums_local, dx, dgamma, dbeta, rows, C, act, p, mask ? rate : 0.f, scale,
                      shift, (hipStream_t)stream);
}

int gn_bn_bwd_stats_conv1(const float* g, const float* w, int L, int Lout, int k, int pad_left, const float* x, const uint8_t* mask, const float* save_mean,
                          const float* save_invstd, double* dsums, void* ws, size_t ws_bytes, size_t rows, int C, int act, float p, float rate,
                          const float* scale, const float* shift, void* stream) {
  GN_REQUIRE(x && save_mean && save_invstd && dsums && ws && rows > 0 && C > 0, "bn_bwd_stats_conv1: bad arguments");
  ColRedArgs r = {};
  int rc = lazy_dy_check("bn_bwd_stats_conv1", g, w, L, Lout, k, pad_left, rows, C, scale, shift, &r.lz);
  if (rc) return rc;
  r.a = nullptr; r.y = nullptr; r.xpre = x; r.mask = mask; r.mean = save_mean; r.invstd = save_invstd; r.scale = scale; r.shift = shift;
  r.rows = rows; r.C = C; r.act = act; r.act_param = p; r.keep_scale = 1.0f / (1.0f - (mask ? rate : 0.f));
  return colred_run(2, r, ws, ws_bytes, dsums, nullptr, (hipStream_t)stream);
}
int gn_bn_bwd_apply_conv1(const float* g, const float* w, int L, int Lout, int k, int pad_left, const float* x, const uint8_t* mask, const float* gamma,
                          const float* save_mean, const float* save_invstd, const double* dsums_global, double count, const double* dsums_local, float* dx,
                          float* dgamma, float* dbeta, size_t rows, int C, int act, float p, float rate, const float* scale, const float* shift, void* stream) {
  GN_REQUIRE(x && gamma && save_mean && save_invstd && dsums_global && dsums_local && dx && dgamma && dbeta && C > 0, "bn_bwd_apply_conv1: bad arguments");
  LazyDy z = {};
  int rc = lazy_dy_check("bn_bwd_apply_conv1", g, w, L, Lout, k, pad_left, rows, C, scale, shift, &z);
  if (rc) return rc;
  return bn_bwd_apply(nullptr, nullptr, x, mask, gamma, save_mean, save_invstd, dsums_global, count, dsums_local, dx, dgamma, dbeta, rows, C, act, p,
                      mask ? rate : 0.f, scale, shift, (hipStream_t)stream, &z);
}

size_t gn_bias_grad_workspace(size_t rows, int C) { return bias_grad_ws(rows, C) + 256; }

int gn_bias_grad(const float* dy, float* db, void* ws, size_t ws_bytes, size_t rows, int C, void* stream) {
  GN_REQUIRE(dy && db && ws && rows > 0 && C > 0, "bias_grad: bad arguments");
  return bias_grad(dy, db, rows, C, ws, ws_bytes, (hipStream_t)stream);
}

}  // extern "C"
