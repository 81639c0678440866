// Keras 2.2.4 merge layers (layers/merge.py) and their entry points: Add, Subtract, Multiply, Average, Maximum, Minimum as one streaming pass over up
// to GN_MERGE_MAX_INPUTS inputs, the input gradients of Multiply / Maximum / Minimum, an out-of-place scale, and Concatenate over the (outer, w_i) views.
//
//  * element-wise: a grid-stride loop, float4 body, scalar head and tail for any length (optim.hip's scheme): when the arrays are not mutually
//    16-byte aligned the pass is all-scalar.  The grid is merge_grid's: at most 512 blocks for 16-byte items, 2048 for 4-byte ones
//    (Concatenate: 2048 for both).  Every lane first loads its element of every input (independent loads in flight), then folds them
//    LEFT TO RIGHT in fp32, as Keras' _merge_function loops: ((x0 o x1) o x2) ...; Average divides the sum once by (float)k.
//  * Maximum / Minimum keep the earlier value on a tie (b > a ? b : a), so +-0 ties are decided too, and their gradient goes, whole, to the FIRST
//    input that attains the extremum (TensorFlow's _MaximumMinimumGrad under Keras' chain of K.maximum: xmask = x >= y), an exact +0 to the others.
//  * Concatenate: one launch; a lane owns one unit (float4 when every width is a multiple of 4 and every pointer 16-byte aligned, else one float) of
//    y (forward: gather) or of dy (backward: scatter into the wanted dx_i) and steps its (row, column) position by the grid's stride.
//  * the pointer tables are HOST arrays read when the entry point runs and handed to the kernel by value: no device table, no copy, no
//    synchronisation, no atomics; a captured step replays the launch as it was recorded.
#include "common.h"

namespace gn {

static constexpr int MAXK = GN_MERGE_MAX_INPUTS;

struct MergeTab {
  const float* x[MAXK];
};

__device__ __forceinline__ float f4_get(const float4& q, int c) { return c == 0 ? q.x : c == 1 ? q.y : c == 2 ? q.z : q.w; }
__device__ __forceinline__ void f4_set(float4& q, int c, float v) {
  if (c == 0) q.x = v; else if (c == 1) q.y = v; else if (c == 2) q.z = v; else q.w = v;
}

template <int MODE>
__device__ __forceinline__ float merge2(float a, float b) {
  switch (MODE) {
    case GN_MERGE_SUB: return a - b;
    case GN_MERGE_MUL: return a * b;
    case GN_MERGE_MAX: return b > a ? b : a;
    case GN_MERGE_MIN: return b < a ? b : a;
    default: return a + b;                        // ADD, AVG
  }
}

// x0 o x1 o ... o x_{k-1}, left to right
template <int MODE>
__device__ __forceinline__ float merge_elem(const float (&v)[MAXK], int k, float kf) {
  float a = v[0];
#pragma unroll
  for (int j = 1; j < MAXK; ++j)
    if (j < k) a = merge2<MODE>(a, v[j]);
  return MODE == GN_MERGE_AVG ? a / kf : a;
}

// MUL: g * (product over j != which, left to right from the first such j); MAX / MIN: g where `which` is the first input at the extremum, else +0
template <int MODE>
__device__ __forceinline__ float merge_grad_elem(float g, const float (&v)[MAXK], int k, int which) {
  if (MODE == GN_MERGE_MUL) {
    float prod = 1.f;
    bool first = true;
#pragma unroll
    for (int j = 0; j < MAXK; ++j)
      if (j < k && j != which) {
        prod = first ? v[j] : prod * v[j];
        first = false;
      }
    return first ? g : g * prod;
  }
  float m = v[0];
  int w = 0;
#pragma unroll
  for (int j = 1; j < MAXK; ++j)
    if (j < k && (MODE == GN_MERGE_MAX ? v[j] > m : v[j] < m)) {
      m = v[j];
      w = j;
    }
  return w == which ? g : 0.f;
}

// [0, head) and [head + 4 nvec, n): scalar; [head, head + 4 nvec): float4 (every array is 16-byte aligned at element `head`)
template <int MODE>
__global__ __launch_bounds__(256) void merge_fwd_kernel(MergeTab p, int k, float* y, size_t n, size_t head, size_t nvec) {
  const float kf = (float)k;
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = tid; i < nvec; i += stride) {
    float4 t[MAXK] = {};
#pragma unroll
    for (int j = 0; j < MAXK; ++j)
      if (j < k) t[j] = reinterpret_cast<const float4*>(p.x[j] + head)[i];
    float4 o;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float v[MAXK];
#pragma unroll
      for (int j = 0; j < MAXK; ++j) v[j] = f4_get(t[j], c);
      f4_set(o, c, merge_elem<MODE>(v, k, kf));
    }
    reinterpret_cast<float4*>(y + head)[i] = o;
  }
  const size_t tail0 = head + 4 * nvec, nrem = head + (n - tail0);
  for (size_t r = tid; r < nrem; r += stride) {
    const size_t e = r < head ? r : tail0 + (r - head);
    float v[MAXK] = {};
#pragma unroll
    for (int j = 0; j < MAXK; ++j)
      if (j < k) v[j] = p.x[j][e];
    y[e] = merge_elem<MODE>(v, k, kf);
  }
}

// Multiply does not read x[which]
template <int MODE>
__global__ __launch_bounds__(256) void merge_bwd_kernel(const float* dy, MergeTab p, int k, int which, float* dx, size_t n, size_t head, size_t nvec) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = tid; i < nvec; i += stride) {
    const float4 g = reinterpret_cast<const float4*>(dy + head)[i];
    float4 t[MAXK] = {};
#pragma unroll
    for (int j = 0; j < MAXK; ++j)
      if (j < k && (MODE != GN_MERGE_MUL || j != which)) t[j] = reinterpret_cast<const float4*>(p.x[j] + head)[i];
    float4 o;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float v[MAXK];
#pragma unroll
      for (int j = 0; j < MAXK; ++j) v[j] = f4_get(t[j], c);
      f4_set(o, c, merge_grad_elem<MODE>(f4_get(g, c), v, k, which));
    }
    reinterpret_cast<float4*>(dx + head)[i] = o;
  }
  const size_t tail0 = head + 4 * nvec, nrem = head + (n - tail0);
  for (size_t r = tid; r < nrem; r += stride) {
    const size_t e = r < head ? r : tail0 + (r - head);
    float v[MAXK] = {};
#pragma unroll
    for (int j = 0; j < MAXK; ++j)
      if (j < k && (MODE != GN_MERGE_MUL || j != which)) v[j] = p.x[j][e];
    dx[e] = merge_grad_elem<MODE>(dy[e], v, k, which);
  }
}

__global__ __launch_bounds__(256) void scale_kernel(const float* __restrict__ x, float a, float* __restrict__ y, size_t n, size_t head, size_t nvec) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = tid; i < nvec; i += stride) {
    float4 v = reinterpret_cast<const float4*>(x + head)[i];
    v.x = a * v.x; v.y = a * v.y; v.z = a * v.z; v.w = a * v.w;
    reinterpret_cast<float4*>(y + head)[i] = v;
  }
  const size_t tail0 = head + 4 * nvec, nrem = head + (n - tail0);
  for (size_t r = tid; r < nrem; r += stride) {
    const size_t e = r < head ? r : tail0 + (r - head);
    y[e] = a * x[e];
  }
}

// Grid of the passes of this file.  stream_grid counts ITEMS (2048 blocks of 256 lanes per trip), sized for 4-byte items: a trip of 16-byte items
// puts four times the bytes in flight.  Measured at 256 MiB per array: Add of two inputs with the float4 body runs at 5.1-5.5 TB/s
// under that cap, 5.8 TB/s at 512 blocks (the bytes per trip of a scalar pass at 2048, which also runs at 5.8), 5.6 at 1024.  So a float4 body
// takes at most 512 blocks, a scalar pass stream_grid's 2048.  Concatenate keeps stream_grid for both unit sizes: its float4 gather of two 64-float
// wide inputs measured 5.0 TB/s at 2048 blocks and 4.4 at 512.
static constexpr unsigned VEC_BLOCKS = 512;
static inline unsigned merge_grid(size_t nvec, size_t n) {
  if (!nvec) return stream_grid(n);
  const size_t g = (nvec + 255) / 256;
  return g < VEC_BLOCKS ? (unsigned)g : VEC_BLOCKS;
}

// elements before the first 16-byte boundary, or n when the arrays are not mutually aligned (all-scalar pass): optim.hip's vec_head over a table
static size_t merge_vec_head(size_t n, const void* const* ptrs, int count) {
  const uintptr_t mis = (uintptr_t)ptrs[0] & 15;
  for (int j = 0; j < count; ++j)
    if (((uintptr_t)ptrs[j] & 15) != mis) return n;
  if (mis & 3) return n;
  const size_t h = ((16 - mis) & 15) / 4;
  return h < n ? h : n;
}

// ---------------------------------------------------------------------------------------------
// Concatenate: y (outer, W) = [x_0 (outer, w_0) | x_1 (outer, w_1) | ...], W = sum w_i; widths and offsets in units of T
// ---------------------------------------------------------------------------------------------
struct ConcatTab {
  float* p[MAXK];          // forward: the inputs (read only); backward: the dx_i, NULL = not wanted
  int w[MAXK], off[MAXK];
  int k;
};

template <typename T, bool FWD>
__global__ __launch_bounds__(256) void concat_kernel(ConcatTab tab, T* yy, size_t outer, int W) {
  const size_t total = outer * (size_t)W, tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  if (tid >= total) return;
  size_t r = tid / W;                            // the one division: after it the position advances by the stride's (rows, columns)
  int c = (int)(tid % W);
  const size_t dr = stride / W;
  const int dc = (int)(stride % W);
  for (size_t i = tid; i < total; i += stride) {
    T* base = reinterpret_cast<T*>(tab.p[0]);
    int w = tab.w[0], off = 0;
#pragma unroll
    for (int q = 1; q < MAXK; ++q)
      if (q < tab.k && c >= tab.off[q]) {
        base = reinterpret_cast<T*>(tab.p[q]);
        w = tab.w[q];
        off = tab.off[q];
      }
    const size_t e = r * (size_t)w + (size_t)(c - off);
    if (FWD) yy[i] = base[e];
    else if (base) base[e] = yy[i];
    c += dc;
    r += dr;
    if (c >= W) {
      c -= W;
      ++r;
    }
  }
}

// the table of a call, its total width, and whether the float4 form applies; GN_EINVAL through `what` on a bad argument
static int concat_table(const char* what, float* const* ptrs, bool null_ok, const int* widths, int k, const void* whole, ConcatTab* tab, long long* W, bool* vec) {
  GN_REQUIRE(ptrs && widths && whole, "%s: null pointer", what);
  GN_REQUIRE(k >= 1 && k <= MAXK, "%s: %d inputs, 1 .. %d are supported", what, k, MAXK);
  *W = 0;
  *vec = ((uintptr_t)whole & 15) == 0;
  for (int j = 0; j < k; ++j) {
    GN_REQUIRE(null_ok || ptrs[j], "%s: input %d is a null pointer", what, j);
    GN_REQUIRE(widths[j] > 0, "%s: width %d of input %d must be positive", what, widths[j], j);
    *W += widths[j];
    if ((widths[j] & 3) || ((uintptr_t)ptrs[j] & 15)) *vec = false;
  }
  GN_REQUIRE(*W < (1ll << 31), "%s: total width %lld does not fit 31 bits", what, *W);
  const int unit = *vec ? 4 : 1;
  int off = 0;
  *tab = ConcatTab{};
  tab->k = k;
  for (int j = 0; j < k; ++j) {
    tab->p[j] = ptrs[j];
    tab->w[j] = widths[j] / unit;
    tab->off[j] = off;
    off += widths[j] / unit;
  }
  return GN_OK;
}

template <bool FWD>
static int concat_launch(const ConcatTab& tab, float* whole, size_t outer, long long W, bool vec, hipStream_t s) {
  if (vec) hipLaunchKernelGGL((concat_kernel<float4, FWD>), dim3(stream_grid(outer * (size_t)(W / 4))), dim3(256), 0, s, tab, (float4*)whole, outer, (int)(W / 4));
  else hipLaunchKernelGGL((concat_kernel<float, FWD>), dim3(stream_grid(outer * (size_t)W)), dim3(256), 0, s, tab, whole, outer, (int)W);
  return check_launch(FWD ? "concat_fwd" : "concat_bwd");
}

}  // namespace gn

using namespace gn;

extern "C" {

int gn_merge_fwd(int mode, const float* const* xs_host, int n_inputs, float* y, size_t n, void* stream) {
  GN_REQUIRE(xs_host && y, "merge_fwd: null pointer");
  GN_REQUIRE(mode >= GN_MERGE_ADD && mode <= GN_MERGE_MIN, "merge_fwd: unknown mode %d", mode);
  GN_REQUIRE(n_inputs >= 1 && n_inputs <= MAXK, "merge_fwd: %d inputs, 1 .. %d are supported", n_inputs, MAXK);
  GN_REQUIRE(mode != GN_MERGE_SUB || n_inputs == 2, "merge_fwd: Subtract takes exactly 2 inputs, got %d", n_inputs);
  MergeTab tab = {};
  const void* all[MAXK + 1] = {y};
  for (int j = 0; j < n_inputs; ++j) {
    GN_REQUIRE(xs_host[j], "merge_fwd: input %d is a null pointer", j);
    tab.x[j] = xs_host[j];
    all[j + 1] = xs_host[j];
  }
  if (!n) return GN_OK;
  const size_t head = merge_vec_head(n, all, n_inputs + 1);
  const size_t nvec = (n - head) / 4;
  const dim3 grid(merge_grid(nvec, n)), block(256);
  hipStream_t s = (hipStream_t)stream;
  switch (mode) {
    case GN_MERGE_ADD: hipLaunchKernelGGL(merge_fwd_kernel<GN_MERGE_ADD>, grid, block, 0, s, tab, n_inputs, y, n, head, nvec); break;
    case GN_MERGE_SUB: hipLaunchKernelGGL(merge_fwd_kernel<GN_MERGE_SUB>, grid, block, 0, s, tab, n_inputs, y, n, head, nvec); break;
    case GN_MERGE_MUL: hipLaunchKernelGGL(merge_fwd_kernel<GN_MERGE_MUL>, grid, block, 0, s, tab, n_inputs, y, n, head, nvec); break;
    case GN_MERGE_AVG: hipLaunchKernelGGL(merge_fwd_kernel<GN_MERGE_AVG>, grid, block, 0, s, tab, n_inputs, y, n, head, nvec); break;
    case GN_MERGE_MAX: hipLaunchKernelGGL(merge_fwd_kernel<GN_MERGE_MAX>, grid, block, 0, s, tab, n_inputs, y, n, head, nvec); break;
    case GN_MERGE_MIN: hipLaunchKernelGGL(merge_fwd_kernel<GN_MERGE_MIN>, grid, block, 0, s, tab, n_inputs, y, n, head, nvec); break;
  }
  return check_launch("merge_fwd");
}

int gn_merge_bwd(int mode, const float* dy, const float* const* xs_host, int n_inputs, int which, float* dx, size_t n, void* stream) {
  GN_REQUIRE(dy && xs_host && dx, "merge_bwd: null pointer");
  GN_REQUIRE(mode >= GN_MERGE_ADD && mode <= GN_MERGE_MIN, "merge_bwd: unknown mode %d", mode);
  GN_REQUIRE(mode == GN_MERGE_MUL || mode == GN_MERGE_MAX || mode == GN_MERGE_MIN,
             "merge_bwd: mode %d has no kernel (Add: dx = dy; Subtract, Average: gn_scale by -1 or 1 / k)", mode);
  GN_REQUIRE(n_inputs >= 1 && n_inputs <= MAXK, "merge_bwd: %d inputs, 1 .. %d are supported", n_inputs, MAXK);
  GN_REQUIRE(which >= 0 && which < n_inputs, "merge_bwd: input %d of %d", which, n_inputs);
  MergeTab tab = {};
  const void* all[MAXK + 2] = {dx, dy};
  int cnt = 2;
  for (int j = 0; j < n_inputs; ++j) {
    GN_REQUIRE(xs_host[j], "merge_bwd: input %d is a null pointer", j);
    tab.x[j] = xs_host[j];
    if (mode != GN_MERGE_MUL || j != which) all[cnt++] = xs_host[j];
  }
  if (!n) return GN_OK;
  const size_t head = merge_vec_head(n, all, cnt);
  const size_t nvec = (n - head) / 4;
  const dim3 grid(merge_grid(nvec, n)), block(256);
  hipStream_t s = (hipStream_t)stream;
  switch (mode) {
    case GN_MERGE_MUL: hipLaunchKernelGGL(merge_bwd_kernel<GN_MERGE_MUL>, grid, block, 0, s, dy, tab, n_inputs, which, dx, n, head, nvec); break;
    case GN_MERGE_MAX: hipLaunchKernelGGL(merge_bwd_kernel<GN_MERGE_MAX>, grid, block, 0, s, dy, tab, n_inputs, which, dx, n, head, nvec); break;
    case GN_MERGE_MIN: hipLaunchKernelGGL(merge_bwd_kernel<GN_MERGE_MIN>, grid, block, 0, s, dy, tab, n_inputs, which, dx, n, head, nvec); break;
  }
  return check_launch("merge_bwd");
}

int gn_scale(const float* x, float a, float* y, size_t n, void* stream) {
  GN_REQUIRE(x && y, "scale: null pointer");
  GN_REQUIRE(x != y, "scale: out of place only (y == x)");
  if (!n) return GN_OK;
  const void* all[2] = {y, x};
  const size_t head = merge_vec_head(n, all, 2);
  const size_t nvec = (n - head) / 4;
  hipLaunchKernelGGL(scale_kernel, dim3(merge_grid(nvec, n)), dim3(256), 0, (hipStream_t)stream, x, a, y, n, head, nvec);
  return check_launch("scale");
}

int gn_concat_fwd(const float* const* xs_host, const int* widths_host, int n_inputs, float* y, size_t outer, void* stream) {
  ConcatTab tab;
  long long W;
  bool vec;
  // the forward kernel only reads through the table
  const int rc = concat_table("concat_fwd", const_cast<float* const*>(xs_host), false, widths_host, n_inputs, y, &tab, &W, &vec);
  if (rc != GN_OK) return rc;
  if (!outer) return GN_OK;
  return concat_launch<true>(tab, y, outer, W, vec, (hipStream_t)stream);
}

int gn_concat_bwd(const float* dy, float* const* dxs_host, const int* widths_host, int n_inputs, size_t outer, void* stream) {
  ConcatTab tab;
  long long W;
  bool vec;
  const int rc = concat_table("concat_bwd", dxs_host, true, widths_host, n_inputs, dy, &tab, &W, &vec);
  if (rc != GN_OK) return rc;
  if (!outer) return GN_OK;
  return concat_launch<false>(tab, const_cast<float*>(dy), outer, W, vec, (hipStream_t)stream);
}

}  // extern "C"
