// Conv1D(dilation_rate=d, padding='causal'): the two passes around the library's own undilated convs, and their entry points.
//
// A stride-1 conv with dilation d reads, for the output row l, the input rows l - pl + j*d: all of one residue class mod d.  So the zero-padded
// input splits into d phase sequences, each of which an UNDILATED conv maps onto the same phase of the output:
//   split   x (B, L, C) -> xs (B*d, M, C):  xs[b*d + p, m, :] = x[b, m*d + p - off, :] inside [0, L), +0 outside (the padding, and the
//           rows that only round M up); an input row past the M rows is dropped.  Every element of xs is written.
//   merge   xs (B*d, M, C) -> x (B, L, C):  x[b, i, :] = xs[b*d + (i + off) % d, (i + off) / d, :] -- the adjoint of the split, as a gather.
//  * a lane owns one unit (float4 when C % 4 == 0 and both tensors are 16-byte aligned, else one float) of the OUTPUT and steps it by the grid's
//    stride: consecutive lanes run along C, so both the row it writes and the row it gathers are contiguous; no atomics, nothing is written twice.
//  * unit indices are size_t (B*d*M*C passes 2^31 at workload sizes); an index that fits 32 bits is divided in 32 bits.
//  * the grid is stream_grid's, as Concatenate's gather keeps it for both unit sizes (merge.hip).
#include "common.h"

namespace gn {

// a / b and a % b of a size_t by a positive int: 32-bit arithmetic wherever the dividend fits (every shape the layers meet but the largest)
__device__ __forceinline__ size_t divmod(size_t a, int b, int* rem) {
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
__device__ __forceinline__ T zero_unit();
template <>
__device__ __forceinline__ float zero_unit<float>() { return 0.f; }
template <>
__device__ __forceinline__ float4 zero_unit<float4>() { return make_float4(0.f, 0.f, 0.f, 0.f); }

// C: units per row
template <typename T>
__global__ __launch_bounds__(256) void dilate_split_kernel(const T* __restrict__ x, T* __restrict__ xs, size_t total, int L, int C, int d, int off, int M) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  for (size_t u = tid; u < total; u += stride) {
    int c, m, p;
    const size_t row = divmod(u, C, &c);             // row = (b*d + p)*M + m
    const size_t bp = divmod(row, M, &m);
    const size_t b = divmod(bp, d, &p);
    const long long i = (long long)m * d + p - off;
    xs[u] = (i >= 0 && i < L) ? x[(b * (size_t)L + (size_t)i) * (size_t)C + (size_t)c] : zero_unit<T>();
  }
}

template <typename T>
__global__ __launch_bounds__(256) void dilate_merge_kernel(const T* __restrict__ xs, T* __restrict__ x, size_t total, int L, int C, int d, int off, int M) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  for (size_t u = tid; u < total; u += stride) {
    int c, i, p;
    const size_t row = divmod(u, C, &c);             // row = b*L + i
    const size_t b = divmod(row, L, &i);
    const size_t m = divmod((size_t)i + (size_t)off, d, &p);      // < M: the entry point checked the last row
    x[u] = xs[((b * (size_t)d + (size_t)p) * (size_t)M + m) * (size_t)C + (size_t)c];
  }
}

static int dilate_args(const char* what, const void* a, const void* b, int B, int L, int C, int d, int off, int M) {
  GN_REQUIRE(a && b, "%s: null pointer", what);
  GN_REQUIRE(B >= 1 && L >= 1 && C >= 1 && d >= 1 && M >= 1, "%s: B %d, L %d, C %d, d %d, M %d must all be >= 1", what, B, L, C, d, M);
  GN_REQUIRE(off >= 0, "%s: off %d must be >= 0", what, off);
  return GN_OK;
}

static inline bool dilate_vec(const void* a, const void* b, int C) { return C % 4 == 0 && (((uintptr_t)a | (uintptr_t)b) & 15) == 0; }

}  // namespace gn

using namespace gn;

extern "C" {

int gn_dilate_split(const float* x, float* xs, int B, int L, int C, int d, int off, int M, void* stream) {
  const int rc = dilate_args("dilate_split", x, xs, B, L, C, d, off, M);
  if (rc != GN_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  const size_t rows = (size_t)B * (size_t)d * (size_t)M;
  if (dilate_vec(x, xs, C)) {
    const size_t total = rows * (size_t)(C / 4);
    hipLaunchKernelGGL(dilate_split_kernel<float4>, dim3(stream_grid(total)), dim3(256), 0, s, (const float4*)x, (float4*)xs, total, L, C / 4, d, off, M);
  } else {
    const size_t total = rows * (size_t)C;
    hipLaunchKernelGGL(dilate_split_kernel<float>, dim3(stream_grid(total)), dim3(256), 0, s, x, xs, total, L, C, d, off, M);
  }
  return check_launch("dilate_split");
}

int gn_dilate_merge(const float* xs, float* x, int B, int L, int C, int d, int off, int M, void* stream) {
  const int rc = dilate_args("dilate_merge", xs, x, B, L, C, d, off, M);
  if (rc != GN_OK) return rc;
  GN_REQUIRE(((long long)L - 1 + off) / d < M, "dilate_merge: row %lld of a phase is read for L %d, off %d, d %d, but xs has M = %d rows",
             ((long long)L - 1 + off) / d, L, off, d, M);
  hipStream_t s = (hipStream_t)stream;
  const size_t rows = (size_t)B * (size_t)L;
  if (dilate_vec(xs, x, C)) {
    const size_t total = rows * (size_t)(C / 4);
    hipLaunchKernelGGL(dilate_merge_kernel<float4>, dim3(stream_grid(total)), dim3(256), 0, s, (const float4*)xs, (float4*)x, total, L, C / 4, d, off, M);
  } else {
    const size_t total = rows * (size_t)C;
    hipLaunchKernelGGL(dilate_merge_kernel<float>, dim3(stream_grid(total)), dim3(256), 0, s, xs, x, total, L, C, d, off, M);
  }
  return check_launch("dilate_merge");
}

}  // extern "C"
