// Keras pooling layers: MaxPooling1D/2D, AveragePooling1D/2D over any pool, stride and padding, and the four global layers.
// Channels-last: (B, H, W, C) for the windowed passes (the 1-D layers are W = 1), (B, P, C) -> (B, C) for the global ones (P = L or H*W).
// pool.hip keeps the (2,1)/(2,1)/'valid' maximum the discriminator runs; everything else is here.
//
// Windowed, Keras 2.2.4 on TensorFlow: output (ho, wo) reads rows [ho*sh - pad_top, ho*sh - pad_top + ph) x columns [wo*sw - pad_left, ... + pw)
// clipped to the tensor.  Maximum: padded cells never win (the running maximum starts from the window's first in-bounds cell; a window of -inf
// gives -inf); its gradient goes to the FIRST maximum in row-major (h, w) order (the update is v > m, as pool.hip's), contributions of
// overlapping windows add.  Average: fp32 sum in row-major order, one division by the number of IN-BOUNDS cells; gradient dy / count summed
// over the covering windows.  Both backward passes are gathers: a thread owns VEC floats of dx and walks the <= ceil(ph/sh) * ceil(pw/sw)
// windows that cover them in ascending (ho, wo) order -- no atomics, cells in stride gaps and behind the last full window get a stored zero,
// and the maximum's backward recomputes each window's first maximum from x (no index tensor).
// Global: average = fp64 sum over P in a fixed order / P, gradient dy / P; maximum = tf.reduce_max, whose gradient is dy / n_ties to EVERY
// position equal to the maximum (not the first-maximum rule): a counting reduction, then a distributing pass.
// C % 4 == 0 on 16-byte aligned tensors: float4 loads and stores; otherwise scalar (checked per launch).  All passes HBM-bound streams.
#include "common.h"

namespace gn {
namespace {

template <int VEC>
__device__ __forceinline__ void load_v(const float* __restrict__ p, float (&v)[VEC]) {
  if constexpr (VEC == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
    v[0] = *p;
  }
}
template <int VEC>
__device__ __forceinline__ void store_v(float* __restrict__ p, const float (&v)[VEC]) {
  if constexpr (VEC == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  else *p = v[0];
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

struct PoolGeo {
  int H, W, Ho, Wo, ph, pw, sh, sw, pt, pl;
};

// ---------------------------------------------------------------------------------------------
// grid-stride position (b, h, w, c) of a unit index over (B, Hd, Wd, Cv): divided once per thread in front of the loop (the start and the
// grid's stride), then stepped digit by digit with one carry each -- no division in the loop.  Every digit and step is below its extent
// (< 2^31), so digit + step + carry stays below 2^32 and one subtraction brings it back.
// ---------------------------------------------------------------------------------------------
struct Odo {
  unsigned c, w, h, b, sc, sw, sh, sb;
};
__device__ __forceinline__ void odo_split(size_t i, unsigned Cv, unsigned Wd, unsigned Hd, unsigned* c, unsigned* w, unsigned* h, unsigned* b) {
  const size_t q = i / Cv;
  *c = (unsigned)(i - q * Cv);
  const size_t r = q / Wd;
  *w = (unsigned)(q - r * Wd);
  const size_t bb = r / Hd;
  *h = (unsigned)(r - bb * Hd);
  *b = (unsigned)bb;
}
__device__ __forceinline__ Odo odo_init(unsigned Cv, unsigned Wd, unsigned Hd) {
  Odo o;
  odo_split((size_t)blockIdx.x * 256 + threadIdx.x, Cv, Wd, Hd, &o.c, &o.w, &o.h, &o.b);
  odo_split((size_t)gridDim.x * 256, Cv, Wd, Hd, &o.sc, &o.sw, &o.sh, &o.sb);
  return o;
}
__device__ __forceinline__ void odo_step(Odo& o, unsigned Cv, unsigned Wd, unsigned Hd) {
  o.c += o.sc;
  if (o.c >= Cv) { o.c -= Cv; ++o.w; }
  o.w += o.sw;
  if (o.w >= Wd) { o.w -= Wd; ++o.h; }
  o.h += o.sh;
  if (o.h >= Hd) { o.h -= Hd; ++o.b; }
  o.b += o.sb;
}

// ---------------------------------------------------------------------------------------------
// windowed forward: one unit of y per thread and trip
// ---------------------------------------------------------------------------------------------
template <int MODE, int VEC>
__global__ __launch_bounds__(256) void pool2d_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, size_t nv, int Cv, PoolGeo g) {
  Odo o = odo_init(Cv, g.Wo, g.Ho);
  const size_t C = (size_t)Cv * VEC, stride = (size_t)gridDim.x * 256;
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < nv; idx += stride) {
    const int h0 = (int)o.h * g.sh - g.pt, w0 = (int)o.w * g.sw - g.pl;
    const int hs = h0 > 0 ? h0 : 0, he = h0 + g.ph < g.H ? h0 + g.ph : g.H;
    const int ws = w0 > 0 ? w0 : 0, we = w0 + g.pw < g.W ? w0 + g.pw : g.W;         // hs < he and ws < we: checked by the launcher
    const float* xb = x + (size_t)o.b * g.H * g.W * C + (size_t)o.c * VEC;
    float acc[VEC];
    bool first = true;
    for (int h = hs; h < he; ++h) {
      const float* xr = xb + (size_t)h * g.W * C;
      for (int w = ws; w < we; ++w) {
        float v[VEC];
        load_v<VEC>(xr + (size_t)w * C, v);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          if (first) acc[e] = v[e];
          else if (MODE == GN_POOL_MAX) acc[e] = v[e] > acc[e] ? v[e] : acc[e];
          else acc[e] += v[e];
        }
        first = false;
      }
    }
    if (MODE == GN_POOL_AVG) {
      const float cnt = (float)((he - hs) * (we - ws));
#pragma unroll
      for (int e = 0; e < VEC; ++e) acc[e] = acc[e] / cnt;
    }
    store_v<VEC>(y + idx * VEC, acc);
    odo_step(o, Cv, g.Wo, g.Ho);
  }
}

// a / s for the strides that occur (uniform branch), a >= 0
__device__ __forceinline__ int div_stride(int a, int s) { return s == 1 ? a : s == 2 ? a >> 1 : (int)((unsigned)a / (unsigned)s); }

// the outputs [lo, hi] whose window covers input coordinate t (tp = t + pad): o*s <= tp < o*s + p, o < n_out; false: none
__device__ __forceinline__ bool covering(int tp, int p, int s, int n_out, int* lo, int* hi) {
  int h = div_stride(tp, s);
  if (h > n_out - 1) h = n_out - 1;
  if (h * s + p <= tp) return false;
  int l = h;
  while (l > 0 && (l - 1) * s + p > tp) --l;
  *lo = l; *hi = h;
  return true;
}

// ---------------------------------------------------------------------------------------------
// windowed backward: one unit of dx per thread and trip
// ---------------------------------------------------------------------------------------------
template <int MODE, int VEC>
__global__ __launch_bounds__(256) void pool2d_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x, float* __restrict__ dx, size_t nv, int Cv,
                                                         PoolGeo g) {
  Odo o = odo_init(Cv, g.W, g.H);
  const size_t C = (size_t)Cv * VEC, stride = (size_t)gridDim.x * 256;
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < nv; idx += stride) {
    float acc[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] = 0.f;
    int ho_lo = 0, ho_hi = -1, wo_lo = 0, wo_hi = -1;
    const bool covered = covering((int)o.h + g.pt, g.ph, g.sh, g.Ho, &ho_lo, &ho_hi) && covering((int)o.w + g.pl, g.pw, g.sw, g.Wo, &wo_lo, &wo_hi);
    if (covered) {
      const float* dyb = dy + (size_t)o.b * g.Ho * g.Wo * C + (size_t)o.c * VEC;
      const float* xb = MODE == GN_POOL_MAX ? x + (size_t)o.b * g.H * g.W * C + (size_t)o.c * VEC : nullptr;
      bool any = false;
      for (int ho = ho_lo; ho <= ho_hi; ++ho) {
        const int h0 = ho * g.sh - g.pt;
        const int hs = h0 > 0 ? h0 : 0, he = h0 + g.ph < g.H ? h0 + g.ph : g.H;
        for (int wo = wo_lo; wo <= wo_hi; ++wo) {
          const int w0 = wo * g.sw - g.pl;
          const int ws = w0 > 0 ? w0 : 0, we = w0 + g.pw < g.W ? w0 + g.pw : g.W;
          float t[VEC];
          load_v<VEC>(dyb + ((size_t)ho * g.Wo + wo) * C, t);
          if (MODE == GN_POOL_AVG) {
            const float cnt = (float)((he - hs) * (we - ws));
#pragma unroll
            for (int e = 0; e < VEC; ++e) t[e] = t[e] / cnt;
          } else {
            // this window's first maximum, as the forward found it; `mine` = this cell's place in the scan
            const int mine = ((int)o.h - hs) * (we - ws) + ((int)o.w - ws);
            float m[VEC];
            int arg[VEC], k = 0;
            for (int h = hs; h < he; ++h) {
              const float* xr = xb + (size_t)h * g.W * C;
              for (int w = ws; w < we; ++w, ++k) {
                float v[VEC];
                load_v<VEC>(xr + (size_t)w * C, v);
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                  if (k == 0 || v[e] > m[e]) { m[e] = v[e]; arg[e] = k; }
                }
              }
            }
#pragma unroll
            for (int e = 0; e < VEC; ++e) t[e] = arg[e] == mine ? t[e] : 0.f;
          }
#pragma unroll
          for (int e = 0; e < VEC; ++e) acc[e] = any ? acc[e] + t[e] : t[e];
          any = true;
        }
      }
    }
    store_v<VEC>(dx + idx * VEC, acc);
    odo_step(o, Cv, g.W, g.H);
  }
}

// ---------------------------------------------------------------------------------------------
// global reductions over P of (B, P, C), the pattern of colred_kernel (bn.hip): grid = (column blocks, chunks of P, B); a block's 256 lanes
// are NQc column units x RL row lanes, a lane runs over the rows p_lo + rl, + RL, ... of its chunk; the row lanes are combined through LDS
// in lane order, the chunks by global_final_kernel in chunk order: a fixed order, no atomics, the same bits on every run.
// MODE 0: fp64 sum of x.  MODE 1: maximum of x (from -inf, update v > m).  MODE 2: fp64 count of x == y[b, c] (the ties of the maximum).
// One chunk: the result is finished here (out); more: part[(chunk * B + b) * C + c] as doubles.
// ---------------------------------------------------------------------------------------------
enum { GRED_SUM = 0, GRED_MAX = 1, GRED_TIES = 2 };

template <int MODE>
__device__ __forceinline__ float global_finish(double t, const float* __restrict__ dy, size_t i, int P) {
  if (MODE == GRED_SUM) return (float)(t / (double)P);
  if (MODE == GRED_MAX) return (float)t;
  return (float)((double)dy[i] / t);                        // dy / n_ties: t >= 1 (the maximum is one of the values) unless x holds a NaN
}

template <int MODE, int VEC>
__global__ __launch_bounds__(256) void global_reduce_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ dy,
                                                            float* __restrict__ out, double* __restrict__ part, int B, int P, int C, int rows_per_chunk) {
  const int NQ = C / VEC, NQc = NQ < 256 ? NQ : 256, RL = 256 / NQc;
  const int tid = threadIdx.x, ql = tid % NQc, rl = tid / NQc;
  const int q = blockIdx.x * NQc + ql, b = blockIdx.z;
  const bool active = rl < RL && q < NQ;
  double s[VEC];
  float ym[VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) { s[e] = MODE == GRED_MAX ? -(double)INFINITY : 0.0; ym[e] = 0.f; }
  if (active) {
    if (MODE == GRED_TIES) load_v<VEC>(y + (size_t)b * C + (size_t)q * VEC, ym);
    const int p_lo = blockIdx.y * rows_per_chunk, p_hi = p_lo + rows_per_chunk < P ? p_lo + rows_per_chunk : P;
    const float* xb = x + (size_t)b * P * C + (size_t)q * VEC;
    float m[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) m[e] = -INFINITY;
    constexpr int U = 2;                                    // rows per trip, loads first (colred_kernel: more is slower)
    for (int p = p_lo + rl; p < p_hi; p += RL * U) {
      float v[U][VEC];
      bool ok[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        ok[u] = p + u * RL < p_hi;
        load_v<VEC>(xb + (size_t)(ok[u] ? p + u * RL : p) * C, v[u]);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (!ok[u]) break;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          if (MODE == GRED_SUM) s[e] += (double)v[u][e];
          else if (MODE == GRED_MAX) m[e] = v[u][e] > m[e] ? v[u][e] : m[e];
          else s[e] += v[u][e] == ym[e] ? 1.0 : 0.0;
        }
      }
    }
    if (MODE == GRED_MAX) {
#pragma unroll
      for (int e = 0; e < VEC; ++e) s[e] = (double)m[e];
    }
  }
  __shared__ double red[256 * VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) red[tid * VEC + e] = s[e];
  __syncthreads();
  if (rl == 0 && q < NQ) {
    double t[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) t[e] = red[ql * VEC + e];
    for (int k = 1; k < RL; ++k) {
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        const double u = red[(k * NQc + ql) * VEC + e];
        if (MODE == GRED_MAX) t[e] = u > t[e] ? u : t[e];
        else t[e] += u;
      }
    }
    const size_t i = (size_t)b * C + (size_t)q * VEC;
    if (gridDim.y == 1) {
#pragma unroll
      for (int e = 0; e < VEC; ++e) out[i + e] = global_finish<MODE>(t[e], dy, i + e, P);
    } else {
      double* d = part + (size_t)blockIdx.y * B * C + i;
#pragma unroll
      for (int e = 0; e < VEC; ++e) d[e] = t[e];
    }
  }
}

// the chunks of one (b, c) in chunk order
template <int MODE>
__global__ __launch_bounds__(256) void global_final_kernel(const double* __restrict__ part, const float* __restrict__ dy, float* __restrict__ out, size_t n,
                                                           int chunks, int P) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double t = part[i];
  for (int k = 1; k < chunks; ++k) {
    const double u = part[(size_t)k * n + i];
    if (MODE == GRED_MAX) t = u > t ? u : t;
    else t += u;
  }
  out[i] = global_finish<MODE>(t, dy, i, P);
}

// global backward, the distributing pass: the grid of the reduction with chunks chosen for the stores alone.  A lane holds its (b, c) value
// once: dy / P (one rounding: the division is made in fp64) or coef = dy / n_ties of the counting pass, stored where x equals the maximum.
template <int MODE, int VEC>
__global__ __launch_bounds__(256) void global_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ y,
                                                         const float* __restrict__ coef, float* __restrict__ dx, int P, int C, int rows_per_chunk) {
  const int NQ = C / VEC, NQc = NQ < 256 ? NQ : 256, RL = 256 / NQc;
  const int tid = threadIdx.x, ql = tid % NQc, rl = tid / NQc;
  const int q = blockIdx.x * NQc + ql, b = blockIdx.z;
  if (rl >= RL || q >= NQ) return;
  const size_t i = (size_t)b * C + (size_t)q * VEC;
  float cf[VEC], ym[VEC];
  if (MODE == GN_POOL_AVG) {
    load_v<VEC>(dy + i, cf);
#pragma unroll
    for (int e = 0; e < VEC; ++e) { cf[e] = (float)((double)cf[e] / (double)P); ym[e] = 0.f; }
  } else {
    load_v<VEC>(coef + i, cf);
    load_v<VEC>(y + i, ym);
  }
  const int p_lo = blockIdx.y * rows_per_chunk, p_hi = p_lo + rows_per_chunk < P ? p_lo + rows_per_chunk : P;
  const size_t base = (size_t)b * P * C + (size_t)q * VEC;
  for (int p = p_lo + rl; p < p_hi; p += RL) {
    float o[VEC];
    if (MODE == GN_POOL_AVG) {
#pragma unroll
      for (int e = 0; e < VEC; ++e) o[e] = cf[e];
    } else {
      float v[VEC];
      load_v<VEC>(x + base + (size_t)p * C, v);
#pragma unroll
      for (int e = 0; e < VEC; ++e) o[e] = v[e] == ym[e] ? cf[e] : 0.f;
    }
    store_v<VEC>(dx + base + (size_t)p * C, o);
  }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
// one axis of the window geometry: every output's window holds an in-bounds cell
bool axis_ok(int n, int p, int s, int pad, int n_out) {
  return n > 0 && p > 0 && s > 0 && pad >= 0 && pad < p && n_out > 0 && (long long)(n_out - 1) * s - pad <= (long long)n - 1 &&
         (long long)(n_out - 1) * s + p < 0x7fffffffll;
}

struct GlobalPlan {
  int NQc, RL, gx, chunks, rows_per_chunk;
};
// chunks of P per (b, column block): one when B * column blocks fill the chip, else towards `target` blocks with at least 4 rows per row
// lane.  By the shape alone -- the workspace size depends on it -- so C % 4 == 0 counts float4 units whatever the alignment turns out to be.
GlobalPlan global_plan(int B, int P, int C, int target) {
  GlobalPlan g;
  const int NQ = C % 4 == 0 ? C / 4 : C;
  g.NQc = NQ < 256 ? NQ : 256;
  g.RL = 256 / g.NQc;
  g.gx = (NQ + g.NQc - 1) / g.NQc;
  const long long blocks = (long long)g.gx * (B > 0 ? B : 1);
  long long chunks = blocks >= 512 ? 1 : (target + blocks - 1) / blocks;
  const long long by_rows = ((long long)P + (long long)g.RL * 4 - 1) / ((long long)g.RL * 4);
  if (chunks > by_rows) chunks = by_rows;
  if (chunks < 1) chunks = 1;
  g.rows_per_chunk = (int)(((long long)P + chunks - 1) / chunks);
  g.chunks = (P + g.rows_per_chunk - 1) / g.rows_per_chunk;
  return g;
}
// the scalar kernels on a C % 4 == 0 shape (misaligned pointers) keep the plan's chunks; their column blocks follow from C
int scalar_gx(int C) { return (C + 255) / 256; }

bool global_shape_ok(int B, int P, int C) { return B >= 0 && P > 0 && C > 0 && (long long)B * C < 0x7fffffffll && B <= 65535; }

size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }
size_t global_coef_bytes(int B, int C) { return align16((size_t)B * C * sizeof(float)); }
size_t global_ws_bytes(int B, int P, int C) {
  const GlobalPlan g = global_plan(B, P, C, 1024);
  return global_coef_bytes(B, C) + (g.chunks > 1 ? (size_t)g.chunks * B * C * sizeof(double) : 0);
}

// MODE of GRED_*: out (B, C) floats; ws past the coefficient block holds the partials
template <int MODE>
int global_reduce(const char* what, const float* x, const float* y, const float* dy, float* out, void* ws, int B, int P, int C, hipStream_t s) {
  const GlobalPlan g = global_plan(B, P, C, 1024);
  double* part = (double*)((char*)ws + global_coef_bytes(B, C));
  const bool v4 = C % 4 == 0 && aligned16(x) && aligned16(out) && aligned16(y) && aligned16(dy);
  const dim3 grid(v4 || C % 4 ? g.gx : scalar_gx(C), g.chunks, B), block(256);
  if (v4) hipLaunchKernelGGL((global_reduce_kernel<MODE, 4>), grid, block, 0, s, x, y, dy, out, part, B, P, C, g.rows_per_chunk);
  else hipLaunchKernelGGL((global_reduce_kernel<MODE, 1>), grid, block, 0, s, x, y, dy, out, part, B, P, C, g.rows_per_chunk);
  int rc = check_launch(what);
  if (rc || g.chunks == 1) return rc;
  const size_t n = (size_t)B * C;
  hipLaunchKernelGGL(global_final_kernel<MODE>, dim3(cdiv(n, 256)), dim3(256), 0, s, part, dy, out, n, g.chunks, P);
  return check_launch(what);
}

template <int MODE>
void global_bwd_launch(const float* dy, const float* x, const float* y, const float* coef, float* dx, int B, int P, int C, hipStream_t s) {
  const GlobalPlan g = global_plan(B, P, C, 2048);
  const bool v4 = C % 4 == 0 && aligned16(dy) && aligned16(dx) && aligned16(x) && aligned16(y) && aligned16(coef);
  const dim3 grid(v4 || C % 4 ? g.gx : scalar_gx(C), g.chunks, B), block(256);
  if (v4) hipLaunchKernelGGL((global_bwd_kernel<MODE, 4>), grid, block, 0, s, dy, x, y, coef, dx, P, C, g.rows_per_chunk);
  else hipLaunchKernelGGL((global_bwd_kernel<MODE, 1>), grid, block, 0, s, dy, x, y, coef, dx, P, C, g.rows_per_chunk);
}

}  // namespace
}  // namespace gn

using namespace gn;

#define GN_POOL_GEOMETRY(what)                                                                                                                       \
  GN_REQUIRE(mode == GN_POOL_MAX || mode == GN_POOL_AVG, what ": unknown mode %d", mode);                                                            \
  GN_REQUIRE(B >= 0 && C > 0, what ": bad shape (B %d, C %d)", B, C);                                                                                \
  GN_REQUIRE(axis_ok(H, ph, sh, pad_top, Ho), what ": rows: H %d, pool %d, stride %d, pad %d, Ho %d (all sizes > 0, 0 <= pad < pool, every window "  \
             "holds a row of the input)", H, ph, sh, pad_top, Ho);                                                                                   \
  GN_REQUIRE(axis_ok(W, pw, sw, pad_left, Wo), what ": columns: W %d, pool %d, stride %d, pad %d, Wo %d (all sizes > 0, 0 <= pad < pool, every "     \
             "window holds a column of the input)", W, pw, sw, pad_left, Wo);                                                                        \
  const PoolGeo geo = {H, W, Ho, Wo, ph, pw, sh, sw, pad_top, pad_left}

extern "C" {

int gn_pool2d_fwd(int mode, const float* x, float* y, int B, int H, int W, int C, int ph, int pw, int sh, int sw, int pad_top, int pad_left, int Ho, int Wo,
                  void* stream) {
  GN_REQUIRE(x && y, "pool2d_fwd: null pointer");
  GN_POOL_GEOMETRY("pool2d_fwd");
  if (B == 0) return GN_OK;
  const bool v4 = C % 4 == 0 && aligned16(x) && aligned16(y);
  const int Cv = v4 ? C / 4 : C;
  const size_t nv = (size_t)B * Ho * Wo * Cv;
  const dim3 grid(stream_grid(nv)), block(256);
  hipStream_t s = (hipStream_t)stream;
  if (mode == GN_POOL_MAX) {
    if (v4) hipLaunchKernelGGL((pool2d_fwd_kernel<GN_POOL_MAX, 4>), grid, block, 0, s, x, y, nv, Cv, geo);
    else hipLaunchKernelGGL((pool2d_fwd_kernel<GN_POOL_MAX, 1>), grid, block, 0, s, x, y, nv, Cv, geo);
  } else {
    if (v4) hipLaunchKernelGGL((pool2d_fwd_kernel<GN_POOL_AVG, 4>), grid, block, 0, s, x, y, nv, Cv, geo);
    else hipLaunchKernelGGL((pool2d_fwd_kernel<GN_POOL_AVG, 1>), grid, block, 0, s, x, y, nv, Cv, geo);
  }
  return check_launch("pool2d_fwd");
}

int gn_pool2d_bwd(int mode, const float* dy, const float* x, float* dx, int B, int H, int W, int C, int ph, int pw, int sh, int sw, int pad_top, int pad_left,
                  int Ho, int Wo, void* stream) {
  GN_REQUIRE(dy && dx && (x || mode == GN_POOL_AVG), "pool2d_bwd: null pointer");
  GN_POOL_GEOMETRY("pool2d_bwd");
  if (B == 0) return GN_OK;
  const bool v4 = C % 4 == 0 && aligned16(dy) && aligned16(dx) && (mode == GN_POOL_AVG || aligned16(x));
  const int Cv = v4 ? C / 4 : C;
  const size_t nv = (size_t)B * H * W * Cv;
  const dim3 grid(stream_grid(nv)), block(256);
  hipStream_t s = (hipStream_t)stream;
  if (mode == GN_POOL_MAX) {
    if (v4) hipLaunchKernelGGL((pool2d_bwd_kernel<GN_POOL_MAX, 4>), grid, block, 0, s, dy, x, dx, nv, Cv, geo);
    else hipLaunchKernelGGL((pool2d_bwd_kernel<GN_POOL_MAX, 1>), grid, block, 0, s, dy, x, dx, nv, Cv, geo);
  } else {
    if (v4) hipLaunchKernelGGL((pool2d_bwd_kernel<GN_POOL_AVG, 4>), grid, block, 0, s, dy, x, dx, nv, Cv, geo);
    else hipLaunchKernelGGL((pool2d_bwd_kernel<GN_POOL_AVG, 1>), grid, block, 0, s, dy, x, dx, nv, Cv, geo);
  }
  return check_launch("pool2d_bwd");
}

size_t gn_global_pool_workspace(int B, int P, int C) {
  if (!global_shape_ok(B, P, C)) return 0;
  return global_ws_bytes(B, P, C);
}

int gn_global_pool_fwd(int mode, const float* x, float* y, void* ws, size_t ws_bytes, int B, int P, int C, void* stream) {
  GN_REQUIRE(x && y && ws, "global_pool_fwd: null pointer");
  GN_REQUIRE(mode == GN_POOL_MAX || mode == GN_POOL_AVG, "global_pool_fwd: unknown mode %d", mode);
  GN_REQUIRE(global_shape_ok(B, P, C), "global_pool_fwd: bad shape (B %d, P %d, C %d): 0 <= B <= 65535, P and C >= 1, B * C < 2^31", B, P, C);
  if (B == 0) return GN_OK;
  if (ws_bytes < global_ws_bytes(B, P, C) || !aligned16(ws)) {
    set_error("global_pool_fwd: workspace of %zu bytes, needs %zu, 16-byte aligned", ws_bytes, global_ws_bytes(B, P, C));
    return GN_EWORKSPACE;
  }
  if (mode == GN_POOL_AVG) return global_reduce<GRED_SUM>("global_pool_fwd", x, nullptr, nullptr, y, ws, B, P, C, (hipStream_t)stream);
  return global_reduce<GRED_MAX>("global_pool_fwd", x, nullptr, nullptr, y, ws, B, P, C, (hipStream_t)stream);
}

int gn_global_pool_bwd(int mode, const float* dy, const float* x, const float* y, float* dx, void* ws, size_t ws_bytes, int B, int P, int C, void* stream) {
  GN_REQUIRE(dy && dx && ws && ((x && y) || mode == GN_POOL_AVG), "global_pool_bwd: null pointer");
  GN_REQUIRE(mode == GN_POOL_MAX || mode == GN_POOL_AVG, "global_pool_bwd: unknown mode %d", mode);
  GN_REQUIRE(global_shape_ok(B, P, C), "global_pool_bwd: bad shape (B %d, P %d, C %d): 0 <= B <= 65535, P and C >= 1, B * C < 2^31", B, P, C);
  if (B == 0) return GN_OK;
  if (ws_bytes < global_ws_bytes(B, P, C) || !aligned16(ws)) {
    set_error("global_pool_bwd: workspace of %zu bytes, needs %zu, 16-byte aligned", ws_bytes, global_ws_bytes(B, P, C));
    return GN_EWORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  if (mode == GN_POOL_AVG) {
    global_bwd_launch<GN_POOL_AVG>(dy, nullptr, nullptr, nullptr, dx, B, P, C, s);
    return check_launch("global_pool_bwd");
  }
  float* coef = (float*)ws;                                  // dy / n_ties per (b, c)
  const int rc = global_reduce<GRED_TIES>("global_pool_bwd ties", x, y, dy, coef, ws, B, P, C, s);
  if (rc) return rc;
  global_bwd_launch<GN_POOL_MAX>(dy, x, y, coef, dx, B, P, C, s);
  return check_launch("global_pool_bwd");
}

}  // extern "C"
