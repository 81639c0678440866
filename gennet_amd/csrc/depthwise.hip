// The depthwise half of keras.layers.SeparableConv1D (keras 2.2.4 layers/convolutional.py, K.separable_conv1d -> tf.nn.depthwise_conv2d): forward,
// data gradient and weight gradient as three streaming kernels; DESIGN 8r.  Channels-last fp32:
//
//   x (B, L, C)    w (k, C, dm) = keras' depthwise_kernel    y (B, Lout, C dm), output channel co = c dm + m
//   y[b, l, c dm + m]  = sum_t x[b, l s - pad_left + t d, c] * w[t, c, m]                  (x outside [0, L) is 0)
//   dx[b, i, c]        = sum_{t, m : (i + pad_left - t d) % s == 0, l = (i + pad_left - t d) / s in [0, Lout)} dy[b, l, c dm + m] * w[t, c, m]
//   dw[t, c, m]        = sum_{b, l} x[b, l s - pad_left + t d, c] * dy[b, l, c dm + m]
//
// There is no reduction over channels, so nothing here is a matrix product: 2 k flop a loaded float, bound by memory.  The pointwise half of the
// layer is a k = 1 product on the matrix-core kernels the library already has (gennet_amd/separable.py).
//
// OWNERSHIP.  One thread owns its outputs, nothing is shared between threads, no atomics.  The channel axis is the contiguous one and the fastest
// index of the work items, so the lanes of a wave read and write consecutive addresses.  w is (k, C dm) in memory: the weights of the V output
// channels co .. co + V - 1 of a tap are V consecutive floats.
//   vector path (V = DW_VEC = 4): C dm % 4 == 0 (data gradient: C % 4 == 0) and 16-byte aligned pointers: 16-byte loads and stores of x, w, y, dy,
//     dx wherever four channels are consecutive in memory (x and dy under dm == 1, w and y always).  dm == 2: the two x of four outputs are one
//     8-byte load, the eight dy and w of four inputs two 16-byte loads each.  dm > 2: the four x (forward, weight gradient) or the 4 dm dy and w
//     (data gradient) are scalar loads beside the 16-byte stores.
//   scalar path (V = 1): every other channel count, and unaligned pointers.  The same kernels, instantiated for V = 1.
//   forward: an item is (b, row group, row lane rs, channel group), the channel group fastest, then the row lane.  A thread owns the DW_ROWS = 4
//     output rows lg 4 RS + r RS + rs and loads a tap's weights once for them; RS = 64 / (channel groups a row), at least 1 (dw_fwd_row_lanes),
//     so that a wave whose row holds fewer than 64 channel groups spans RS consecutive rows: one contiguous stretch of x and of y.
//   data gradient: an item is (b, input row i, channel group).
//   Both run min(ceil(items / 256), 2048) blocks of 256 threads with a grid-stride loop (dw_stream_grid).  The k overlapping windows of x (dy) are
//   read k times by neighbouring items of the same block within a few hundred cycles: the first read comes from HBM, the others from L1 / L2.
//   weight gradient: grid (ctiles, parts).  The B Lout rows are cut into `parts` ranges of rpp rows (dw_wgrad_parts: by shape alone), a block owns
//     one range and NC channel groups, its 256 threads are NC channel lanes x RL row lanes; row lane q walks the rows r0 + q, r0 + q + RL, ...
//     For k > DW_WG_TAPS = 8 the range is swept ceil(k / 8) times, 8 taps' sums in registers a sweep (the sweeps after the first read L2).
//
// NUMERICS.  Everything is fp32 fmaf; the library builds with -ffp-contract=off.
//   y:  ONE chain acc = fmaf(x, w, acc) from +0 over t = 0 .. k-1; taps that fall into the padding are skipped (they would add an exact +0).
//   dx: ONE chain from +0 over t = 0 .. k-1 and, inside a tap, m = 0 .. dm-1; pairs whose row is no output row are skipped.
//   dw: a thread's chain from +0 over its rows in ascending order (at most ceil(rpp / RL) terms; padding skipped); the RL row lanes' sums are
//       added in fp64 in lane order q = 0 .. RL-1 and stored as the block's partial; gn::colred_finalize_f32 (csrc/bn.hip, the final pass of
//       the fixed-order fp64 column reduction behind gn_bias_grad) sums the `parts` partials in fp64 in its fixed order and rounds once to fp32.
//   A sample's y and dx depend on that sample's x (dy) and on w alone: not on B, not on the block or thread they fall in, not on the launch.
//   dw is bit-identical from run to run; its partition depends on (B Lout, k C dm) and, through RL, on the path (V).
//
// WORKSPACE (weight gradient only): parts x (k C dm) doubles, gn_dwconv1d_wgrad_workspace; every element is written before it is read.
#include "common.h"
#include "depthwise_geom.h"

namespace gn {
namespace {

struct DwShape {
  int B, L, C, k, dm, stride, dilation, pad_left, Lout;
  int CO;          // C dm
};

template <int V>
struct DwVec {
  float v[V];
};

template <int V>
__device__ __forceinline__ DwVec<V> dw_load(const float* p) {
  DwVec<V> r;
  if constexpr (V == 4) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    r.v[0] = q.x; r.v[1] = q.y; r.v[2] = q.z; r.v[3] = q.w;
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j) r.v[j] = p[j];
  }
  return r;
}

template <int V>
__device__ __forceinline__ void dw_store(float* p, const float* a) {
  if constexpr (V == 4) {
    *reinterpret_cast<float4*>(p) = make_float4(a[0], a[1], a[2], a[3]);
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j) p[j] = a[j];
  }
}

// the V input channels of the output channels co .. co + V - 1 of row xr: consecutive under dm == 1, two consecutive ones, each twice, under
// dm == 2 on the vector path (co % 4 == 0, so co / 2 is even: an 8-byte aligned pair).  DM: dm where it is 1 or (V == 4) 2, else 0 (any dm).
template <int V, int DM>
__device__ __forceinline__ DwVec<V> dw_load_x(const float* xr, int co, const int* ci) {
  if constexpr (DM == 1) {
    return dw_load<V>(xr + co);
  } else if constexpr (DM == 2 && V == 4) {
    const float2 q = *reinterpret_cast<const float2*>(xr + co / 2);
    DwVec<V> r;
    r.v[0] = q.x; r.v[1] = q.x; r.v[2] = q.y; r.v[3] = q.y;
    return r;
  } else {
    DwVec<V> r;
#pragma unroll
    for (int j = 0; j < V; ++j) r.v[j] = xr[ci[j]];
    return r;
  }
}

template <int V, int DM>
__global__ __launch_bounds__(DW_BLOCK) void dwconv1d_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w, float* __restrict__ y, DwShape g) {
  const unsigned long long nvec = (unsigned long long)(g.CO / V);
  const int RS = dw_fwd_row_lanes((long long)nvec, g.Lout);
  const unsigned long long lgroups = (unsigned long long)((g.Lout + DW_ROWS * RS - 1) / (DW_ROWS * RS));
  const unsigned long long items = (unsigned long long)g.B * lgroups * RS * nvec;
  for (unsigned long long item = (unsigned long long)blockIdx.x * DW_BLOCK + threadIdx.x; item < items; item += (unsigned long long)gridDim.x * DW_BLOCK) {
    const int co = (int)(item % nvec) * V;
    unsigned long long rest = item / nvec;
    const int rs = (int)(rest % RS);
    rest /= RS;
    const int l0 = (int)(rest % lgroups) * DW_ROWS * RS + rs;         // the thread's rows: l0 + r RS
    const unsigned long long b = rest / lgroups;
    int ci[V];
#pragma unroll
    for (int j = 0; j < V; ++j) ci[j] = DM == 1 ? co + j : (co + j) / g.dm;
    float acc[DW_ROWS][V];
#pragma unroll
    for (int r = 0; r < DW_ROWS; ++r)
#pragma unroll
      for (int j = 0; j < V; ++j) acc[r][j] = 0.f;
    const float* xb = x + b * (unsigned long long)g.L * g.C;
    for (int t = 0; t < g.k; ++t) {
      const DwVec<V> wv = dw_load<V>(w + (size_t)t * g.CO + co);
#pragma unroll
      for (int r = 0; r < DW_ROWS; ++r) {
        const long long p = dw_in_row(l0 + r * RS, g.stride, g.pad_left, t, g.dilation);
        if (l0 + r * RS < g.Lout && p >= 0 && p < g.L) {
          const DwVec<V> xv = dw_load_x<V, DM>(xb + p * g.C, co, ci);
#pragma unroll
          for (int j = 0; j < V; ++j) acc[r][j] = fmaf(xv.v[j], wv.v[j], acc[r][j]);
        }
      }
    }
    float* yb = y + (b * (unsigned long long)g.Lout + l0) * g.CO + co;
#pragma unroll
    for (int r = 0; r < DW_ROWS; ++r)
      if (l0 + r * RS < g.Lout) dw_store<V>(yb + (size_t)r * RS * g.CO, acc[r]);
  }
}

template <int V, int DM>
__global__ __launch_bounds__(DW_BLOCK) void dwconv1d_dgrad_kernel(const float* __restrict__ dy, const float* __restrict__ w, float* __restrict__ dx, DwShape g) {
  const unsigned long long nvec = (unsigned long long)(g.C / V);
  const unsigned long long items = (unsigned long long)g.B * g.L * nvec;
  for (unsigned long long item = (unsigned long long)blockIdx.x * DW_BLOCK + threadIdx.x; item < items; item += (unsigned long long)gridDim.x * DW_BLOCK) {
    const int c = (int)(item % nvec) * V;
    const unsigned long long rest = item / nvec;
    const int i = (int)(rest % g.L);
    const unsigned long long b = rest / g.L;
    float acc[V];
#pragma unroll
    for (int j = 0; j < V; ++j) acc[j] = 0.f;
    for (int t = 0; t < g.k; ++t) {
      const long long num = (long long)i + g.pad_left - (long long)t * g.dilation;       // l s of the output row that reads input row i at tap t
      if (num < 0) break;                                                               // and of every later tap
      if (num % g.stride) continue;
      const long long l = num / g.stride;
      if (l >= g.Lout) continue;
      const float* dyr = dy + (b * (unsigned long long)g.Lout + l) * g.CO;
      const float* wr = w + (size_t)t * g.CO;
      if constexpr (DM == 1) {
        const DwVec<V> dv = dw_load<V>(dyr + c), wv = dw_load<V>(wr + c);
#pragma unroll
        for (int j = 0; j < V; ++j) acc[j] = fmaf(dv.v[j], wv.v[j], acc[j]);
      } else if constexpr (DM == 2 && V == 4) {       // the 8 output channels of the 4 input channels are consecutive, 32-byte aligned
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const DwVec<4> dv = dw_load<4>(dyr + 2 * c + 4 * h), wv = dw_load<4>(wr + 2 * c + 4 * h);
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[2 * h + e / 2] = fmaf(dv.v[e], wv.v[e], acc[2 * h + e / 2]);
        }
      } else {
#pragma unroll
        for (int j = 0; j < V; ++j)
          for (int m = 0; m < g.dm; ++m) {
            const size_t o = (size_t)(c + j) * g.dm + m;
            acc[j] = fmaf(dyr[o], wr[o], acc[j]);
          }
      }
    }
    dw_store<V>(dx + (b * (unsigned long long)g.L + i) * g.C + c, acc);
  }
}

template <int V, int DM>
__global__ __launch_bounds__(DW_BLOCK) void dwconv1d_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dy, double* __restrict__ part, DwShape g,
                                                                  int NC, int RL, unsigned long long rows, unsigned long long rpp) {
  __shared__ float red[DW_WG_TAPS * V][DW_BLOCK];
  const int tid = threadIdx.x, cl = tid % NC, rl = tid / NC;
  const long long nvec = g.CO / V;
  const long long cv = (long long)blockIdx.x * NC + cl;
  const bool active = rl < RL && cv < nvec;
  const int co = active ? (int)cv * V : 0;
  int ci[V];
#pragma unroll
  for (int j = 0; j < V; ++j) ci[j] = DM == 1 ? co + j : (co + j) / g.dm;
  const unsigned long long r0 = (unsigned long long)blockIdx.y * rpp;
  const unsigned long long r1 = r0 + rpp < rows ? r0 + rpp : rows;
  const size_t n = (size_t)g.k * g.CO;
  for (int t0 = 0; t0 < g.k; t0 += DW_WG_TAPS) {
    float acc[DW_WG_TAPS][V];
#pragma unroll
    for (int tt = 0; tt < DW_WG_TAPS; ++tt)
#pragma unroll
      for (int j = 0; j < V; ++j) acc[tt][j] = 0.f;
    if (active) {
      for (unsigned long long r = r0 + rl; r < r1; r += RL) {
        const unsigned long long b = r / g.Lout;
        const long long l = (long long)(r - b * g.Lout);
        const DwVec<V> dv = dw_load<V>(dy + r * g.CO + co);
        const float* xb = x + b * (unsigned long long)g.L * g.C;
#pragma unroll
        for (int tt = 0; tt < DW_WG_TAPS; ++tt) {
          const long long p = dw_in_row(l, g.stride, g.pad_left, t0 + tt, g.dilation);
          if (t0 + tt < g.k && p >= 0 && p < g.L) {
            const DwVec<V> xv = dw_load_x<V, DM>(xb + p * g.C, co, ci);
#pragma unroll
            for (int j = 0; j < V; ++j) acc[tt][j] = fmaf(xv.v[j], dv.v[j], acc[tt][j]);
          }
        }
      }
    }
#pragma unroll
    for (int tt = 0; tt < DW_WG_TAPS; ++tt)
#pragma unroll
      for (int j = 0; j < V; ++j) red[tt * V + j][tid] = acc[tt][j];
    __syncthreads();
    // the RL row lanes of every (tap, channel) of the block in lane order, in fp64; the DW_WG_TAPS V NC sums are spread over the 256 threads
    for (int o = tid; o < DW_WG_TAPS * V * NC; o += DW_BLOCK) {
      const int tj = o / NC, c2 = o % NC, t = t0 + tj / V;
      const long long cv2 = (long long)blockIdx.x * NC + c2;
      if (t < g.k && cv2 < nvec) {
        double s = (double)red[tj][c2];
        for (int q = 1; q < RL; ++q) s += (double)red[tj][q * NC + c2];
        part[(size_t)blockIdx.y * n + (size_t)t * g.CO + (size_t)cv2 * V + tj % V] = s;
      }
    }
    __syncthreads();
  }
}

bool dw_aligned16(const void* a, const void* b, const void* c) {
  return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0;
}

// 0: launch, 1: nothing to do (B == 0), GN_EINVAL: refused
int dw_check(const char* what, int B, int L, int C, int k, int dm, int stride, int dilation, int pad_left, int Lout) {
  GN_REQUIRE(B >= 0 && L >= 1 && C >= 1 && k >= 1 && dm >= 1 && Lout >= 1,
             "%s: bad shape (B %d, L %d, C %d, k %d, dm %d, Lout %d): B >= 0, the others >= 1", what, B, L, C, k, dm, Lout);
  GN_REQUIRE(stride >= 1 && dilation >= 1 && pad_left >= 0, "%s: bad geometry (stride %d, dilation %d, pad_left %d): stride, dilation >= 1, pad_left >= 0",
             what, stride, dilation, pad_left);
  const unsigned long long co = (unsigned long long)C * (unsigned long long)dm;
  GN_REQUIRE(co < (1ull << 31) && co * (unsigned long long)k < (1ull << 31), "%s: k * C * dm = %d * %d * %d does not fit 2^31 - 1", what, k, C, dm);
  const unsigned long long lim = 1ull << 62;
  GN_REQUIRE((unsigned long long)B * (unsigned long long)L < lim / (unsigned long long)C && (unsigned long long)B * (unsigned long long)Lout < lim / co,
             "%s: B * L * C or B * Lout * C * dm spans 2^62 elements or more", what);
  return B == 0 ? 1 : 0;
}

}  // namespace
}  // namespace gn

using namespace gn;

// one of the five instantiations of `kernel`: V = 4 where `vec`; DM = dm where dm is 1 or (V = 4) 2, else 0, the form for any dm
#define DW_LAUNCH(kernel, vec, dm, grid, s, ...)                                                            \
  do {                                                                                                      \
    if (vec) {                                                                                              \
      if ((dm) == 1) hipLaunchKernelGGL((kernel<DW_VEC, 1>), grid, dim3(DW_BLOCK), 0, s, __VA_ARGS__);      \
      else if ((dm) == 2) hipLaunchKernelGGL((kernel<DW_VEC, 2>), grid, dim3(DW_BLOCK), 0, s, __VA_ARGS__); \
      else hipLaunchKernelGGL((kernel<DW_VEC, 0>), grid, dim3(DW_BLOCK), 0, s, __VA_ARGS__);                \
    } else {                                                                                                \
      if ((dm) == 1) hipLaunchKernelGGL((kernel<1, 1>), grid, dim3(DW_BLOCK), 0, s, __VA_ARGS__);           \
      else hipLaunchKernelGGL((kernel<1, 0>), grid, dim3(DW_BLOCK), 0, s, __VA_ARGS__);                     \
    }                                                                                                       \
  } while (0)

extern "C" {

int gn_dwconv1d_fwd(const float* x, const float* w, float* y, int B, int L, int C, int k, int dm, int stride, int dilation, int pad_left, int Lout,
                    void* stream) {
  const int rc = dw_check("dwconv1d_fwd", B, L, C, k, dm, stride, dilation, pad_left, Lout);
  if (rc) return rc < 0 ? rc : GN_OK;
  GN_REQUIRE(x && w && y, "dwconv1d_fwd: null pointer (x, w and y are required)");
  const DwShape g = {B, L, C, k, dm, stride, dilation, pad_left, Lout, C * dm};
  const bool vec = g.CO % DW_VEC == 0 && dw_aligned16(x, w, y);
  const dim3 grid(dw_stream_grid(dw_fwd_items(B, Lout, C, dm, vec ? DW_VEC : 1)));
  DW_LAUNCH(dwconv1d_fwd_kernel, vec, dm, grid, (hipStream_t)stream, x, w, y, g);
  return check_launch("dwconv1d_fwd");
}

int gn_dwconv1d_dgrad(const float* dy, const float* w, float* dx, int B, int L, int C, int k, int dm, int stride, int dilation, int pad_left, int Lout,
                      void* stream) {
  const int rc = dw_check("dwconv1d_dgrad", B, L, C, k, dm, stride, dilation, pad_left, Lout);
  if (rc) return rc < 0 ? rc : GN_OK;
  GN_REQUIRE(dy && w && dx, "dwconv1d_dgrad: null pointer (dy, w and dx are required)");
  const DwShape g = {B, L, C, k, dm, stride, dilation, pad_left, Lout, C * dm};
  const bool vec = C % DW_VEC == 0 && dw_aligned16(dy, w, dx);
  const dim3 grid(dw_stream_grid(dw_dgrad_items(B, L, C, vec ? DW_VEC : 1)));
  DW_LAUNCH(dwconv1d_dgrad_kernel, vec, dm, grid, (hipStream_t)stream, dy, w, dx, g);
  return check_launch("dwconv1d_dgrad");
}

size_t gn_dwconv1d_wgrad_workspace(int B, int Lout, int C, int k, int dm) {
  if (B < 1 || Lout < 1 || C < 1 || k < 1 || dm < 1) return 0;
  const unsigned long long co = (unsigned long long)C * (unsigned long long)dm;
  if (co >= (1ull << 31) || co * (unsigned long long)k >= (1ull << 31)) return 0;
  return dw_wgrad_geom(B, Lout, C, k, dm, 1).ws_bytes;
}

int gn_dwconv1d_wgrad(const float* x, const float* dy, float* dw, void* ws, size_t ws_bytes, int B, int L, int C, int k, int dm, int stride, int dilation,
                      int pad_left, int Lout, void* stream) {
  const int rc = dw_check("dwconv1d_wgrad", B, L, C, k, dm, stride, dilation, pad_left, Lout);
  if (rc) return rc < 0 ? rc : GN_OK;
  GN_REQUIRE(x && dy && dw && ws, "dwconv1d_wgrad: null pointer (x, dy, dw and the workspace are required)");
  GN_REQUIRE(((uintptr_t)ws & 7) == 0, "dwconv1d_wgrad: the workspace holds doubles and must be 8-byte aligned");
  const size_t n = (size_t)k * C * dm;
  const DwShape g = {B, L, C, k, dm, stride, dilation, pad_left, Lout, C * dm};
  const bool vec = g.CO % DW_VEC == 0 && dw_aligned16(x, dy, nullptr);
  const DwWgradGeom m = dw_wgrad_geom(B, Lout, C, k, dm, vec ? DW_VEC : 1);
  if (ws_bytes < m.ws_bytes) {
    set_error("dwconv1d_wgrad: workspace too small (%zu bytes, gn_dwconv1d_wgrad_workspace = %zu)", ws_bytes, m.ws_bytes);
    return GN_EWORKSPACE;
  }
  const dim3 grid(m.ctiles, m.parts);
  DW_LAUNCH(dwconv1d_wgrad_kernel, vec, dm, grid, (hipStream_t)stream, x, dy, (double*)ws, g, m.NC, m.RL, m.rows, m.rpp);
  const int rl = check_launch("dwconv1d_wgrad");
  if (rl) return rl;
  return colred_finalize_f32((const double*)ws, dw, n, m.parts, (hipStream_t)stream);
}

}  // extern "C"
