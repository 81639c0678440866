// Keras weight and activity regularizers: the penalty l1 * sum|x| + l2 * sum x^2 of a tensor and its gradient l1 * sign(x) + 2 * l2 * x,
// sign(+-0) = 0, as streaming passes, and their entry points.
//
// ONE kernel body, two optional parts, x read once:
//   PEN    every lane sums l1 |x| + l2 x^2 of its units in fp64 (terms formed in fp64 from the fp32 x and the fp32 coefficients); a block adds its
//          256 lane sums in a fixed order and writes ONE fp64 partial with a plain store.  reg_finish (one block) adds all partials of a step --
//          every regularized weight and every activity penalty, laid side by side by the caller -- in a fixed order and rounds once to fp32.
//   GRAD   gout[i] = gin[i] + (l1 * sign(x[i]) + 2 * l2 * x[i]) in fp32, three roundings (the product, the inner sum, the outer sum); the
//          l1 part is exactly 0 where x == +-0.  gout may be gin (in place: the weight gradients, an activity gradient nothing else holds).
//  * a lane owns units (float4 where every tensor of the pass has the same 16-byte phase: a scalar head up to the boundary, the float4 body, a
//    scalar tail; otherwise one float each) and steps them by the grid's stride.  Indices are size_t.
//  * the grid is stream_grid(ceil(n / 4)): it depends on n only, whatever the alignment picks, so the number of partials does too.
//  * no atomics; two runs give the same bits.
#include "common.h"

namespace gn {

// fixed-order block sum: wave64 butterfly, then the four wave sums in order (optim.hip's)
__device__ __forceinline__ double reg_block_sum(double v) {
  __shared__ double red[4];
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

__device__ __forceinline__ double reg_term(float x, double l1, double l2) {
  const double v = (double)x;
  return l1 * fabs(v) + l2 * (v * v);
}

__device__ __forceinline__ float reg_grad(float g, float x, float l1, float two_l2) {
  const float s = x > 0.f ? l1 : (x < 0.f ? -l1 : 0.f);          // l1 * sign(x), sign(+-0) = 0 (a NaN x gives 0 here and NaN from the product)
  return g + (s + two_l2 * x);
}

template <bool PEN, bool GRAD>
__global__ __launch_bounds__(256) void reg_kernel(const float* __restrict__ x, const float* gin, float* gout, size_t n, size_t head, size_t nvec,
                                                  float l1, float l2, double* __restrict__ partials) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  const double d1 = (double)l1, d2 = (double)l2;
  const float two_l2 = 2.f * l2;
  double acc = 0.0;
  const float4* x4 = reinterpret_cast<const float4*>(x + head);
  for (size_t i = tid; i < nvec; i += stride) {
    const float4 v = x4[i];
    if (PEN) acc += (reg_term(v.x, d1, d2) + reg_term(v.y, d1, d2)) + (reg_term(v.z, d1, d2) + reg_term(v.w, d1, d2));
    if (GRAD) {
      const float4 g = reinterpret_cast<const float4*>(gin + head)[i];
      reinterpret_cast<float4*>(gout + head)[i] = make_float4(reg_grad(g.x, v.x, l1, two_l2), reg_grad(g.y, v.y, l1, two_l2),
                                                              reg_grad(g.z, v.z, l1, two_l2), reg_grad(g.w, v.w, l1, two_l2));
    }
  }
  // the scalar units: [0, head) and [head + 4 nvec, n) -- all of the tensor when the phases differ (head == n, nvec == 0)
  const size_t tail0 = head + 4 * nvec, nrem = head + (n - tail0);
  for (size_t r = tid; r < nrem; r += stride) {
    const size_t i = r < head ? r : tail0 + (r - head);
    const float v = x[i];
    if (PEN) acc += reg_term(v, d1, d2);
    if (GRAD) gout[i] = reg_grad(gin[i], v, l1, two_l2);
  }
  if (PEN) {
    const double s = reg_block_sum(acc);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
  }
}

__global__ __launch_bounds__(256) void reg_finish_kernel(const double* __restrict__ partials, size_t count, float* __restrict__ out) {
  double acc = 0.0;
  for (size_t i = threadIdx.x; i < count; i += 256) acc += partials[i];
  const double s = reg_block_sum(acc);
  if (threadIdx.x == 0) *out = (float)s;
}

// elements before the first 16-byte boundary, or n when the tensors do not share a 16-byte phase (all-scalar pass)
static size_t reg_vec_head(size_t n, const void* a, const void* b, const void* c) {
  const uintptr_t mis = (uintptr_t)a & 15;
  if ((b && ((uintptr_t)b & 15) != mis) || (c && ((uintptr_t)c & 15) != mis) || (mis & 3)) return n;
  const size_t h = ((16 - mis) & 15) / 4;
  return h < n ? h : n;
}

static inline unsigned reg_grid(size_t n) { return stream_grid((n + 3) / 4); }

static int reg_coeffs(const char* what, float l1, float l2) {
  // a NaN fails l >= 0
  GN_REQUIRE(l1 >= 0.f && l2 >= 0.f && l1 <= 3.0e38f && l2 <= 1.5e38f, "%s: l1 %g, l2 %g must be finite and >= 0", what, (double)l1, (double)l2);
  return GN_OK;
}

}  // namespace gn

using namespace gn;

extern "C" {

size_t gn_reg_partials(size_t n) { return n ? reg_grid(n) : 0; }

int gn_reg_pass(const float* x, float* g, size_t n, float l1, float l2, double* partials, size_t n_partials, void* stream) {
  GN_REQUIRE(x && partials, "reg_pass: null pointer");
  GN_REQUIRE(n > 0, "reg_pass: n == 0");
  const int rc = reg_coeffs("reg_pass", l1, l2);
  if (rc != GN_OK) return rc;
  GN_REQUIRE(((uintptr_t)partials & 7) == 0, "reg_pass: the partial workspace is not 8-byte aligned");
  GN_REQUIRE(n_partials >= gn_reg_partials(n), "reg_pass: a workspace of %zu partials for n = %zu, which writes %zu", n_partials, n, gn_reg_partials(n));
  const size_t head = reg_vec_head(n, x, g, nullptr), nvec = (n - head) / 4;
  hipStream_t s = (hipStream_t)stream;
  if (g)
    hipLaunchKernelGGL((reg_kernel<true, true>), dim3(reg_grid(n)), dim3(256), 0, s, x, g, g, n, head, nvec, l1, l2, partials);
  else
    hipLaunchKernelGGL((reg_kernel<true, false>), dim3(reg_grid(n)), dim3(256), 0, s, x, nullptr, nullptr, n, head, nvec, l1, l2, partials);
  return check_launch("reg_pass");
}

int gn_reg_grad(const float* y, const float* gin, float* gout, size_t n, float l1, float l2, void* stream) {
  GN_REQUIRE(y && gin && gout, "reg_grad: null pointer");
  GN_REQUIRE(n > 0, "reg_grad: n == 0");
  const int rc = reg_coeffs("reg_grad", l1, l2);
  if (rc != GN_OK) return rc;
  const size_t head = reg_vec_head(n, y, gin, gout), nvec = (n - head) / 4;
  hipLaunchKernelGGL((reg_kernel<false, true>), dim3(reg_grid(n)), dim3(256), 0, (hipStream_t)stream, y, gin, gout, n, head, nvec, l1, l2, nullptr);
  return check_launch("reg_grad");
}

int gn_reg_finish(const double* partials, size_t count, float* out, void* stream) {
  GN_REQUIRE(partials && out, "reg_finish: null pointer");
  GN_REQUIRE(count > 0, "reg_finish: no partials");
  hipLaunchKernelGGL(reg_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partials, count, out);
  return check_launch("reg_finish");
}

}  // extern "C"
