// Sequence plumbing: keras.layers.Permute, RepeatVector, Cropping1D and ZeroPadding1D as memory-bound passes, and their entry points.
//
//   gn_permute     y = x with its axes permuted (axis i of y is axis perm[i] of x), rank 2 .. 4, contiguous fp32.  Axes of extent 1 are dropped
//                  and axes that stay adjacent and in order are merged first, so the kernels see the smallest rank.  Then
//                    * nothing is left to permute: a device-to-device copy;
//                    * the innermost axis stays innermost: a row copy.  A lane owns one unit (float4 when the inner extent is a multiple of 4
//                      and both tensors are 16-byte aligned, else one float) of y, consecutive lanes run along the inner axis, and the row
//                      it reads is found from the (at most three) outer coordinates of y and their strides in x;
//                    * the innermost axis changes: a tiled transposition of the (new-inner, old-inner) plane through LDS, one 32 x 32 tile a
//                      block, batched over the (at most two) remaining axes.  The tile is read along x's innermost axis and written along
//                      y's, 32 consecutive floats a half wave either way; the tile row is 33 floats, so that the column read of a half wave
//                      ((tx * 33 + c) mod 32 = (tx + c) mod 32) touches 32 different banks as the row write does.  Partial tiles at both
//                      edges are guarded lane by lane.
//                  The backward of a permutation is the same entry with the inverse permutation.
//   gn_repeat_fwd  y[b, j, :] = x[b, :], a lane owns one unit of y.
//   gn_repeat_bwd  dx[b, c] = sum_j dy[b, j, c], in fp64, j ascending, rounded once.  A lane owns one unit of dx (consecutive lanes along c).  Where
//                  B C is small and n large, j is cut into S equal chunks (repeat_splits: by B, n, C alone): a lane sums one chunk into an fp64
//                  partial in the workspace and a second pass adds the S partials in ascending order.  No atomics: bit-identical run to run.
//   gn_shift1d     y[b, l, :] = x[b, l - offset, :] inside [0, Lin), +0 elsewhere: ZeroPadding1D (offset = left), Cropping1D (offset = -left),
//                  and each one's backward, which is the other's forward.  A lane owns one unit of y.
//  * unit indices are size_t; an index that fits 32 bits is divided in 32 bits (dilate.hip's divmod).
//  * no host synchronisation, no device table: the shape records are kernel arguments by value, so a captured step replays the launches as recorded.
#include "common.h"

namespace gn {

// a / b and a % b of a size_t by a positive int: 32-bit arithmetic wherever the dividend fits
__device__ __forceinline__ size_t seq_divmod(size_t a, int b, int* rem) {
  if ((a >> 32) == 0) {
    const uint32_t q = (uint32_t)a / (uint32_t)b;
    *rem = (int)((uint32_t)a - q * (uint32_t)b);
    return q;
  }
  const size_t q = a / (size_t)b;
  *rem = (int)(a - q * (size_t)b);
  return q;
}

template <typename T>
__device__ __forceinline__ T seq_zero();
template <>
__device__ __forceinline__ float seq_zero<float>() { return 0.f; }
template <>
__device__ __forceinline__ float4 seq_zero<float4>() { return make_float4(0.f, 0.f, 0.f, 0.f); }

static inline bool seq_vec(const void* a, const void* b, long long C) { return C % 4 == 0 && (((uintptr_t)a | (uintptr_t)b) & 15) == 0; }

// ---------------------------------------------------------------------------------------------
// permute
// ---------------------------------------------------------------------------------------------
// inner axis stays: y (n[0], n[1], n[2], C) <- x, the row of y's outer coordinates (i0, i1, i2) starts at i0 sin[0] + i1 sin[1] + i2 sin[2] in x (units of T)
struct PermRows {
  int n[3];
  size_t sin[3];
};

template <typename T>
__global__ __launch_bounds__(256) void permute_rows_kernel(const T* __restrict__ x, T* __restrict__ y, size_t total, int C, PermRows p) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  for (size_t u = tid; u < total; u += stride) {
    int c, i2, i1;
    size_t row = seq_divmod(u, C, &c);
    row = seq_divmod(row, p.n[2], &i2);
    const size_t i0 = seq_divmod(row, p.n[1], &i1);
    y[u] = x[i0 * p.sin[0] + (size_t)i1 * p.sin[1] + (size_t)i2 * p.sin[2] + (size_t)c];
  }
}

// inner axis changes: a = y's innermost axis (extent na, stride sin_a in x, 1 in y), b = x's innermost axis (extent nb, stride 1 in x, sout_b in y);
// the batch axes (n0, n1) with their strides in x and in y; ta, tb: tiles along a and b
struct PermPlane {
  int na, nb, n1, ta, tb;
  size_t sin_a, sout_b, sin0, sin1, sout0, sout1;
};

// tile edge; a block of 256 lanes moves the tile in 4 trips of 8 rows.  A 64 x 64 tile (256-byte rows, 16 trips) measured 5 % faster on 537 MB
// tensors and 2 % slower on the 17 MB workload shape: not worth a second form
static constexpr int PT = 32;

__global__ __launch_bounds__(256) void permute_plane_kernel(const float* __restrict__ x, float* __restrict__ y, PermPlane p) {
  __shared__ float tile[PT][PT + 1];
  int tbi, tai, i1;
  size_t blk = seq_divmod(blockIdx.x, p.tb, &tbi);
  blk = seq_divmod(blk, p.ta, &tai);
  const size_t i0 = seq_divmod(blk, p.n1, &i1);
  const float* xb = x + i0 * p.sin0 + (size_t)i1 * p.sin1;
  float* yb = y + i0 * p.sout0 + (size_t)i1 * p.sout1;
  const int tx = threadIdx.x & (PT - 1), ty = threadIdx.x / PT;
  const int a0 = tai * PT, b0 = tbi * PT;
#pragma unroll
  for (int r = ty; r < PT; r += 256 / PT) {
    const int a = a0 + r, b = b0 + tx;
    if (a < p.na && b < p.nb) tile[r][tx] = xb[(size_t)a * p.sin_a + (size_t)b];
  }
  __syncthreads();
#pragma unroll
  for (int r = ty; r < PT; r += 256 / PT) {
    const int b = b0 + r, a = a0 + tx;
    if (a < p.na && b < p.nb) yb[(size_t)b * p.sout_b + (size_t)a] = tile[tx][r];
  }
}

// ---------------------------------------------------------------------------------------------
// repeat
// ---------------------------------------------------------------------------------------------
// C: units per row
template <typename T>
__global__ __launch_bounds__(256) void repeat_fwd_kernel(const T* __restrict__ x, T* __restrict__ y, size_t total, int n, int C) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  for (size_t u = tid; u < total; u += stride) {
    int c, j;
    const size_t b = seq_divmod(seq_divmod(u, C, &c), n, &j);
    y[u] = x[b * (size_t)C + (size_t)c];
  }
}

struct Acc4 {
  double v[4];
};
__device__ __forceinline__ void acc_add(double& a, float v) { a += (double)v; }
__device__ __forceinline__ void acc_add(Acc4& a, const float4& v) {
  a.v[0] += (double)v.x; a.v[1] += (double)v.y; a.v[2] += (double)v.z; a.v[3] += (double)v.w;
}
__device__ __forceinline__ void acc_add(double& a, double v) { a += v; }
__device__ __forceinline__ void acc_add(Acc4& a, const Acc4& v) {
#pragma unroll
  for (int q = 0; q < 4; ++q) a.v[q] += v.v[q];
}
__device__ __forceinline__ float acc_round(const double& a) { return (float)a; }
__device__ __forceinline__ float4 acc_round(const Acc4& a) { return make_float4((float)a.v[0], (float)a.v[1], (float)a.v[2], (float)a.v[3]); }

// items = B * C units of dx; split s sums j in [s chunk, min(n, (s + 1) chunk)).  S == 1: dx is written; else part[(s * items) + item] (fp64)
template <typename T, typename A>
__global__ __launch_bounds__(256) void repeat_bwd_kernel(const T* __restrict__ dy, T* __restrict__ dx, A* __restrict__ part, size_t items, int n, int C,
                                                         int S, int chunk) {
  const size_t total = items * (size_t)S, tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  for (size_t u = tid; u < total; u += stride) {
    const size_t s = u / items, item = u - s * items;
    int c;
    const size_t b = seq_divmod(item, C, &c);
    const int j0 = (int)s * chunk, j1 = j0 + chunk < n ? j0 + chunk : n;
    const T* src = dy + (b * (size_t)n + (size_t)j0) * (size_t)C + (size_t)c;
    A acc = {};
    for (int j = j0; j < j1; ++j, src += C) acc_add(acc, *src);
    if (S == 1) dx[item] = acc_round(acc);
    else part[u] = acc;
  }
}

template <typename T, typename A>
__global__ __launch_bounds__(256) void repeat_bwd_sum_kernel(const A* __restrict__ part, T* __restrict__ dx, size_t items, int S) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  for (size_t item = tid; item < items; item += stride) {
    A acc = {};
    for (int s = 0; s < S; ++s) acc_add(acc, part[(size_t)s * items + item]);
    dx[item] = acc_round(acc);
  }
}

// In how many chunks of j a (B, n, C) gradient is summed, and the chunk length: by the shape alone.  One lane per element of dx is enough once
// there are 65536 of them; below that the chunks bring the lane count up to it, at most 64 chunks and at least 32 terms a chunk.
static void repeat_splits(long long B, int n, int C, int* S, int* chunk) {
  const long long items = B * C;
  long long s = items > 0 ? 65536 / items : 1;
  if (s > 64) s = 64;
  if (s > n / 32) s = n / 32;
  if (s < 1) s = 1;
  *chunk = (int)((n + s - 1) / s);
  *S = (n + *chunk - 1) / *chunk;
}

static int repeat_args(const char* what, const void* a, const void* b, int B, int n, int C) {
  GN_REQUIRE(a && b, "%s: null pointer", what);
  GN_REQUIRE(B >= 0 && n >= 1 && C >= 1, "%s: B %d must be >= 0, n %d and C %d >= 1", what, B, n, C);
  GN_REQUIRE((long long)n * C < (1ll << 31), "%s: n C = %lld does not fit 31 bits", what, (long long)n * C);
  return GN_OK;
}

// ---------------------------------------------------------------------------------------------
// shift
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void shift1d_kernel(const T* __restrict__ x, T* __restrict__ y, size_t total, int Lin, int Lout, int C, int offset) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  for (size_t u = tid; u < total; u += stride) {
    int c, l;
    const size_t b = seq_divmod(seq_divmod(u, C, &c), Lout, &l);
    const long long i = (long long)l - offset;
    y[u] = (i >= 0 && i < Lin) ? x[(b * (size_t)Lin + (size_t)i) * (size_t)C + (size_t)c] : seq_zero<T>();
  }
}

}  // namespace gn

using namespace gn;

extern "C" {

int gn_permute(const float* x, float* y, const int* extents_host, const int* perm_host, int R, void* stream) {
  GN_REQUIRE(x && y && extents_host && perm_host, "permute: null pointer");
  GN_REQUIRE(x != y, "permute: out of place only (y == x)");
  GN_REQUIRE(R >= 2 && R <= 4, "permute: rank %d, 2 .. 4 are supported (the batch axis included)", R);
  bool seen[4] = {false, false, false, false};
  size_t total = 1;
  for (int i = 0; i < R; ++i) {
    GN_REQUIRE(extents_host[i] >= 0, "permute: extent %d of axis %d is negative", extents_host[i], i);
    GN_REQUIRE(perm_host[i] >= 0 && perm_host[i] < R && !seen[perm_host[i]], "permute: perm is not a permutation of 0 .. %d (entry %d is %d)", R - 1, i,
               perm_host[i]);
    seen[perm_host[i]] = true;
    GN_REQUIRE(!extents_host[i] || total <= ((size_t)1 << 61) / (size_t)extents_host[i], "permute: the tensor has 2^61 elements or more");
    total *= (size_t)extents_host[i];
  }
  if (!total) return GN_OK;
  hipStream_t s = (hipStream_t)stream;
  // strides of x's axes; then y's axes in order, those of extent 1 dropped, an axis that follows its predecessor in x as well merged into it
  size_t sx[4];
  sx[R - 1] = 1;
  for (int i = R - 2; i >= 0; --i) sx[i] = sx[i + 1] * (size_t)extents_host[i + 1];
  int rank_in_x[4], cnt = 0;             // the position of an axis among x's axes of extent > 1
  for (int i = 0; i < R; ++i) rank_in_x[i] = extents_host[i] == 1 ? -1 : cnt++;
  size_t n[4], sin[4];
  int r = 0, last = -2;
  for (int i = 0; i < R; ++i) {
    const int ax = perm_host[i];
    if (extents_host[ax] == 1) continue;
    if (r && rank_in_x[ax] == last + 1) {
      n[r - 1] *= (size_t)extents_host[ax];
      sin[r - 1] = sx[ax];
    } else {
      n[r] = (size_t)extents_host[ax];
      sin[r] = sx[ax];
      ++r;
    }
    last = rank_in_x[ax];
  }
  if (r <= 1) {
    if (hipMemcpyAsync(y, x, total * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess) {
      set_error("permute: the device-to-device copy failed");
      return GN_ELAUNCH;
    }
    return GN_OK;
  }
  for (int i = 0; i < r; ++i) GN_REQUIRE(n[i] < ((size_t)1 << 31), "permute: a merged axis of %zu elements does not fit 31 bits", n[i]);
  if (sin[r - 1] == 1) {
    // the innermost axis stays: rows of n[r - 1] floats
    const bool vec = seq_vec(x, y, (long long)n[r - 1]);
    const size_t unit = vec ? 4 : 1;
    PermRows p = {{1, 1, 1}, {0, 0, 0}};
    for (int i = 0; i < r - 1; ++i) {
      p.n[3 - (r - 1) + i] = (int)n[i];
      p.sin[3 - (r - 1) + i] = sin[i] / unit;            // every stride of an outer axis is a multiple of the inner extent
    }
    const size_t units = total / unit;
    const int C = (int)(n[r - 1] / unit);
    if (vec) hipLaunchKernelGGL(permute_rows_kernel<float4>, dim3(stream_grid(units)), dim3(256), 0, s, (const float4*)x, (float4*)y, units, C, p);
    else hipLaunchKernelGGL(permute_rows_kernel<float>, dim3(stream_grid(units)), dim3(256), 0, s, x, y, units, C, p);
    return check_launch("permute (rows)");
  }
  // the innermost axis changes: a = y's innermost axis, b = x's; what is left (at most two axes) is the batch, in y's order
  size_t sy[4];
  sy[r - 1] = 1;
  for (int i = r - 2; i >= 0; --i) sy[i] = sy[i + 1] * n[i + 1];
  int jb = -1;
  for (int i = 0; i < r - 1; ++i)
    if (sin[i] == 1) jb = i;
  GN_REQUIRE(jb >= 0, "permute: internal error, x's innermost axis was not found");
  PermPlane p = {};
  p.na = (int)n[r - 1]; p.sin_a = sin[r - 1];
  p.nb = (int)n[jb]; p.sout_b = sy[jb];
  size_t n0 = 1;
  p.n1 = 1;
  int nbatch = 0;
  for (int i = r - 2; i >= 0; --i) {       // the batch axis nearest the plane becomes (n1, sin1, sout1)
    if (i == jb) continue;
    if (nbatch == 0) { p.n1 = (int)n[i]; p.sin1 = sin[i]; p.sout1 = sy[i]; }
    else { n0 = n[i]; p.sin0 = sin[i]; p.sout0 = sy[i]; }
    ++nbatch;
  }
  p.ta = (p.na + PT - 1) / PT;
  p.tb = (p.nb + PT - 1) / PT;
  const size_t blocks = n0 * (size_t)p.n1 * (size_t)p.ta * (size_t)p.tb;
  GN_REQUIRE(blocks < ((size_t)1 << 31), "permute: %zu tiles exceed the grid", blocks);
  hipLaunchKernelGGL(permute_plane_kernel, dim3((unsigned)blocks), dim3(256), 0, s, x, y, p);
  return check_launch("permute (plane)");
}

int gn_repeat_fwd(const float* x, float* y, int B, int n, int C, void* stream) {
  const int rc = repeat_args("repeat_fwd", x, y, B, n, C);
  if (rc != GN_OK) return rc;
  if (!B) return GN_OK;
  hipStream_t s = (hipStream_t)stream;
  const size_t rows = (size_t)B * (size_t)n;
  if (seq_vec(x, y, C)) {
    const size_t total = rows * (size_t)(C / 4);
    hipLaunchKernelGGL(repeat_fwd_kernel<float4>, dim3(stream_grid(total)), dim3(256), 0, s, (const float4*)x, (float4*)y, total, n, C / 4);
  } else {
    const size_t total = rows * (size_t)C;
    hipLaunchKernelGGL(repeat_fwd_kernel<float>, dim3(stream_grid(total)), dim3(256), 0, s, x, y, total, n, C);
  }
  return check_launch("repeat_fwd");
}

size_t gn_repeat_bwd_workspace(int B, int n, int C) {
  if (B < 1 || n < 1 || C < 1) return 0;
  int S, chunk;
  repeat_splits(B, n, C, &S, &chunk);
  return S > 1 ? (size_t)S * (size_t)B * (size_t)C * sizeof(double) : 0;
}

int gn_repeat_bwd(const float* dy, float* dx, void* ws, size_t ws_bytes, int B, int n, int C, void* stream) {
  const int rc = repeat_args("repeat_bwd", dy, dx, B, n, C);
  if (rc != GN_OK) return rc;
  if (!B) return GN_OK;
  int S, chunk;
  repeat_splits(B, n, C, &S, &chunk);
  if (S > 1) {
    GN_REQUIRE(ws && ((uintptr_t)ws & 7) == 0, "repeat_bwd: the workspace is NULL or not 8-byte aligned");
    const size_t need = gn_repeat_bwd_workspace(B, n, C);
    if (ws_bytes < need) {
      set_error("repeat_bwd: workspace of %zu bytes, %zu are needed (gn_repeat_bwd_workspace)", ws_bytes, need);
      return GN_EWORKSPACE;
    }
  }
  hipStream_t s = (hipStream_t)stream;
  if (seq_vec(dy, dx, C)) {
    const size_t items = (size_t)B * (size_t)(C / 4);
    hipLaunchKernelGGL((repeat_bwd_kernel<float4, Acc4>), dim3(stream_grid(items * S)), dim3(256), 0, s, (const float4*)dy, (float4*)dx, (Acc4*)ws, items, n,
                       C / 4, S, chunk);
    if (S > 1) hipLaunchKernelGGL((repeat_bwd_sum_kernel<float4, Acc4>), dim3(stream_grid(items)), dim3(256), 0, s, (const Acc4*)ws, (float4*)dx, items, S);
  } else {
    const size_t items = (size_t)B * (size_t)C;
    hipLaunchKernelGGL((repeat_bwd_kernel<float, double>), dim3(stream_grid(items * S)), dim3(256), 0, s, dy, dx, (double*)ws, items, n, C, S, chunk);
    if (S > 1) hipLaunchKernelGGL((repeat_bwd_sum_kernel<float, double>), dim3(stream_grid(items)), dim3(256), 0, s, (const double*)ws, dx, items, S);
  }
  return check_launch("repeat_bwd");
}

int gn_shift1d(const float* x, float* y, int B, int Lin, int Lout, int C, int offset, void* stream) {
  GN_REQUIRE(x && y, "shift1d: null pointer");
  GN_REQUIRE(x != y, "shift1d: out of place only (y == x)");
  GN_REQUIRE(B >= 0 && Lin >= 1 && Lout >= 1 && C >= 1, "shift1d: B %d must be >= 0, Lin %d, Lout %d and C %d >= 1", B, Lin, Lout, C);
  if (!B) return GN_OK;
  hipStream_t s = (hipStream_t)stream;
  const size_t rows = (size_t)B * (size_t)Lout;
  if (seq_vec(x, y, C)) {
    const size_t total = rows * (size_t)(C / 4);
    hipLaunchKernelGGL(shift1d_kernel<float4>, dim3(stream_grid(total)), dim3(256), 0, s, (const float4*)x, (float4*)y, total, Lin, Lout, C / 4, offset);
  } else {
    const size_t total = rows * (size_t)C;
    hipLaunchKernelGGL(shift1d_kernel<float>, dim3(stream_grid(total)), dim3(256), 0, s, x, y, total, Lin, Lout, C, offset);
  }
  return check_launch("shift1d");
}

}  // extern "C"
