// Keras 2.2.4 optimizers: the default Adam pass (adam_kernel, the engine's own update), the other rules (SGD, RMSprop, Adagrad, Adadelta,
// Adamax, Adam with decay / amsgrad / clipping) as one fused HBM-bound update pass templated on the rule, and the deterministic clip-norm
// reduction in front of it.
//
//  * optim_kernel<RULE>: reads p, g and the rule's state once, writes p and the state once (float4 body, scalar head / tail for any
//    length and alignment).  g is scaled by the clip-norm factor (device memory) and clipped to +-clipvalue first, Keras' order.
//  * clip norm, no host synchronisation and no atomics: optim_sumsq writes one fp64 partial sum of g^2 per block into fixed slots,
//    optim_clip_factor (one block) adds the slots in a fixed order and writes clipnorm / norm (or 1).  A replayed graph and every
//    data-parallel rank (gradients already all-reduced) therefore see the same factor bit for bit.
#include <initializer_list>
#include "common.h"

namespace gn {

struct OptArgs {
  float *p, *s0, *s1, *s2;      // parameters and up to three state arrays (the rule's own: m | a | a, d | m, u | m, v | m, v, vhat)
  const float* g;
  size_t n;
  float lr;                     // lr_eff or lr_t of this step, unless lr_dev is set (captured step: read at run time)
  const float* lr_dev;
  float h0, h1, eps;            // momentum | rho | beta_1, beta_2
  int nesterov;
  const float* clip_scale;      // clipnorm / norm (or 1) in device memory; null: no clip norm
  float clipvalue;              // > 0: clip g to [-clipvalue, clipvalue] after the clip-norm scale
};

struct OptK {
  float lr, h0, h1, om0, om1, eps, scale, clipvalue;
  int nesterov;
};

// one element of the update; the padding of the library's segments (p = g = state = 0) stays 0 under every rule
template <int RULE>
__device__ __forceinline__ void opt_elem(float& p, float g, float& s0, float& s1, float& s2, const OptK& k) {
  g = g * k.scale;
  if (k.clipvalue > 0.f) g = fminf(fmaxf(g, -k.clipvalue), k.clipvalue);
  if (RULE == GN_OPT_SGD) {                       // v = momentum m - lr g; m = v; p += nesterov ? momentum v - lr g : v
    const float v = k.h0 * s0 - k.lr * g;
    s0 = v;
    p = k.nesterov ? p + k.h0 * v - k.lr * g : p + v;
  } else if (RULE == GN_OPT_RMSPROP) {            // a = rho a + (1 - rho) g^2; p -= lr g / (sqrt(a) + eps)
    const float a = k.h0 * s0 + k.om0 * (g * g);
    s0 = a;
    p = p - k.lr * g / (sqrtf(a) + k.eps);
  } else if (RULE == GN_OPT_ADAGRAD) {            // a += g^2; p -= lr g / (sqrt(a) + eps)
    const float a = s0 + g * g;
    s0 = a;
    p = p - k.lr * g / (sqrtf(a) + k.eps);
  } else if (RULE == GN_OPT_ADADELTA) {           // a = rho a + (1 - rho) g^2; u = g sqrt(d + eps) / sqrt(a + eps); p -= lr u; d = rho d + (1 - rho) u^2
    const float a = k.h0 * s0 + k.om0 * (g * g);
    const float u = g * sqrtf(s1 + k.eps) / sqrtf(a + k.eps);
    s0 = a;
    p = p - k.lr * u;
    s1 = k.h0 * s1 + k.om0 * (u * u);
  } else if (RULE == GN_OPT_ADAMAX) {             // m = b1 m + (1 - b1) g; u = max(b2 u, |g|); p -= lr_t m / (u + eps)
    const float m = k.h0 * s0 + k.om0 * g;
    const float u = fmaxf(k.h1 * s1, fabsf(g));
    s0 = m; s1 = u;
    p = p - k.lr * m / (u + k.eps);
  } else {                                        // Adam: m, v as the default pass; amsgrad: vhat = max(vhat, v) takes v's place under the root
    const float m = k.h0 * s0 + k.om0 * g;
    const float v = k.h1 * s1 + k.om1 * g * g;
    s0 = m; s1 = v;
    float den = v;
    if (RULE == GN_OPT_AMSGRAD) { den = fmaxf(s2, v); s2 = den; }
    p = p - k.lr * m / (sqrtf(den) + k.eps);
  }
}

template <int RULE> struct OptState { static constexpr int n = RULE == GN_OPT_AMSGRAD ? 3 : (RULE == GN_OPT_ADADELTA || RULE == GN_OPT_ADAMAX || RULE == GN_OPT_ADAM) ? 2 : 1; };

// [0, head) and [head + 4 nvec, n): scalar; [head, head + 4 nvec): float4 (every array is 16-byte aligned at element `head`)
template <int RULE>
__global__ __launch_bounds__(256) void optim_kernel(OptArgs a, size_t head, size_t nvec) {
  constexpr int NS = OptState<RULE>::n;
  OptK k;
  k.lr = a.lr_dev ? *a.lr_dev : a.lr;
  k.scale = a.clip_scale ? *a.clip_scale : 1.f;
  k.h0 = a.h0; k.h1 = a.h1; k.om0 = 1.f - a.h0; k.om1 = 1.f - a.h1; k.eps = a.eps; k.clipvalue = a.clipvalue; k.nesterov = a.nesterov;
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  float4* p4 = reinterpret_cast<float4*>(a.p + head);
  const float4* g4 = reinterpret_cast<const float4*>(a.g + head);
  float4* s04 = reinterpret_cast<float4*>(a.s0 + head);
  float4* s14 = NS > 1 ? reinterpret_cast<float4*>(a.s1 + head) : nullptr;
  float4* s24 = NS > 2 ? reinterpret_cast<float4*>(a.s2 + head) : nullptr;
  for (size_t i = tid; i < nvec; i += stride) {
    float4 p = p4[i];
    const float4 g = g4[i];
    float4 x = s04[i], y = {}, z = {};
    if (NS > 1) y = s14[i];
    if (NS > 2) z = s24[i];
    opt_elem<RULE>(p.x, g.x, x.x, y.x, z.x, k);
    opt_elem<RULE>(p.y, g.y, x.y, y.y, z.y, k);
    opt_elem<RULE>(p.z, g.z, x.z, y.z, z.z, k);
    opt_elem<RULE>(p.w, g.w, x.w, y.w, z.w, k);
    p4[i] = p; s04[i] = x;
    if (NS > 1) s14[i] = y;
    if (NS > 2) s24[i] = z;
  }
  const size_t tail0 = head + 4 * nvec, nrem = head + (a.n - tail0);
  for (size_t r = tid; r < nrem; r += stride) {
    const size_t j = r < head ? r : tail0 + (r - head);
    float y = 0.f, z = 0.f;
    if (NS > 1) y = a.s1[j];
    if (NS > 2) z = a.s2[j];
    opt_elem<RULE>(a.p[j], a.g[j], a.s0[j], y, z, k);
    if (NS > 1) a.s1[j] = y;
    if (NS > 2) a.s2[j] = z;
  }
}

// elements before the first 16-byte boundary, or n when the arrays are not mutually aligned (all-scalar pass)
static size_t vec_head(size_t n, std::initializer_list<const void*> ptrs) {
  const uintptr_t mis = (uintptr_t)*ptrs.begin() & 15;
  for (const void* q : ptrs)
    if (q && ((uintptr_t)q & 15) != mis) return n;
  if (mis & 3) return n;
  const size_t h = ((16 - mis) & 15) / 4;
  return h < n ? h : n;
}

// ---------------------------------------------------------------------------------------------
// clip norm: fixed-slot fp64 partials, fixed-order finalize
// ---------------------------------------------------------------------------------------------
static constexpr int SUMSQ_MAX_BLOCKS = 1024;

// fixed-order block sum: wave64 butterfly, then the four wave sums in order
__device__ __forceinline__ double block_sum_256(double v) {
  __shared__ double red[4];
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(256) void optim_sumsq_kernel(const float* __restrict__ g, size_t n, size_t head, size_t nvec, double* __restrict__ partials) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  const float4* g4 = reinterpret_cast<const float4*>(g + head);
  double acc = 0.0;
  for (size_t i = tid; i < nvec; i += stride) {
    const float4 v = g4[i];
    acc += ((double)v.x * v.x + (double)v.y * v.y) + ((double)v.z * v.z + (double)v.w * v.w);
  }
  const size_t tail0 = head + 4 * nvec, nrem = head + (n - tail0);
  for (size_t r = tid; r < nrem; r += stride) {
    const double v = g[r < head ? r : tail0 + (r - head)];
    acc += v * v;
  }
  const double s = block_sum_256(acc);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void optim_clip_factor_kernel(const double* __restrict__ partials, size_t count, float clipnorm, float* __restrict__ factor) {
  double acc = 0.0;
  for (size_t i = threadIdx.x; i < count; i += 256) acc += partials[i];
  const double s = block_sum_256(acc);
  if (threadIdx.x == 0) {
    const float norm = (float)sqrt(s);                          // Keras: g <- g * clipnorm / norm when norm >= clipnorm
    *factor = norm >= clipnorm ? clipnorm / norm : 1.f;
  }
}

// ---------------------------------------------------------------------------------------------
// the default Adam (keras form), one fused pass over the flat parameter segment; lr_t by value, or from device memory for a captured step
// ---------------------------------------------------------------------------------------------
__global__ void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, size_t n, float lr_t, float b1,
                            float b2, float eps, const float* __restrict__ lr_t_dev) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  if (lr_t_dev) lr_t = *lr_t_dev;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float gi = g[i];
    const float mi = b1 * m[i] + (1.f - b1) * gi;
    const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
    m[i] = mi; v[i] = vi;
    p[i] -= lr_t * mi / (sqrtf(vi) + eps);
  }
}
static int adam_step(float* p, const float* g, float* m, float* v, size_t n, float lr_t, const float* lr_t_dev, float b1, float b2, float eps, hipStream_t s) {
  if (!n) return GN_OK;
  hipLaunchKernelGGL(adam_kernel, dim3(stream_grid(n)), dim3(256), 0, s, p, g, m, v, n, lr_t, b1, b2, eps, lr_t_dev);
  return check_launch("adam");
}

}  // namespace gn

using namespace gn;

extern "C" {

int gn_optim_step(int rule, float* p, const float* g, float* s0, float* s1, float* s2, size_t n, float lr, const float* lr_dev, float h0, float h1,
                  float eps, int nesterov, const float* clip_scale, float clipvalue, void* stream) {
  GN_REQUIRE(rule >= GN_OPT_SGD && rule <= GN_OPT_AMSGRAD, "optim_step: unknown rule %d", rule);
  if (!n) return GN_OK;
  const int ns = rule == GN_OPT_AMSGRAD ? 3 : (rule == GN_OPT_ADADELTA || rule == GN_OPT_ADAMAX || rule == GN_OPT_ADAM) ? 2 : 1;
  GN_REQUIRE(p && g && s0 && (ns < 2 || s1) && (ns < 3 || s2), "optim_step: null pointer (rule %d keeps %d state arrays)", rule, ns);
  GN_REQUIRE(eps >= 0.f && clipvalue >= 0.f && h0 >= 0.f && h1 >= 0.f, "optim_step: negative hyper-parameter");
  GN_REQUIRE(rule == GN_OPT_SGD || rule == GN_OPT_ADAGRAD || h0 <= 1.f, "optim_step: rho / beta_1 %g outside [0, 1]", h0);
  GN_REQUIRE((rule != GN_OPT_ADAMAX && rule != GN_OPT_ADAM && rule != GN_OPT_AMSGRAD) || h1 <= 1.f, "optim_step: beta_2 %g outside [0, 1]", h1);
  OptArgs a = {};
  a.p = p; a.g = g; a.s0 = s0; a.s1 = ns > 1 ? s1 : nullptr; a.s2 = ns > 2 ? s2 : nullptr; a.n = n;
  a.lr = lr; a.lr_dev = lr_dev; a.h0 = h0; a.h1 = h1; a.eps = eps; a.nesterov = nesterov ? 1 : 0; a.clip_scale = clip_scale; a.clipvalue = clipvalue;
  const size_t head = vec_head(a.n, {a.p, a.g, a.s0, a.s1, a.s2});
  const size_t nvec = (a.n - head) / 4;
  const dim3 grid(stream_grid(nvec ? nvec : a.n)), block(256);
  hipStream_t s = (hipStream_t)stream;
  switch (rule) {
    case GN_OPT_SGD: hipLaunchKernelGGL(optim_kernel<GN_OPT_SGD>, grid, block, 0, s, a, head, nvec); break;
    case GN_OPT_RMSPROP: hipLaunchKernelGGL(optim_kernel<GN_OPT_RMSPROP>, grid, block, 0, s, a, head, nvec); break;
    case GN_OPT_ADAGRAD: hipLaunchKernelGGL(optim_kernel<GN_OPT_ADAGRAD>, grid, block, 0, s, a, head, nvec); break;
    case GN_OPT_ADADELTA: hipLaunchKernelGGL(optim_kernel<GN_OPT_ADADELTA>, grid, block, 0, s, a, head, nvec); break;
    case GN_OPT_ADAMAX: hipLaunchKernelGGL(optim_kernel<GN_OPT_ADAMAX>, grid, block, 0, s, a, head, nvec); break;
    case GN_OPT_ADAM: hipLaunchKernelGGL(optim_kernel<GN_OPT_ADAM>, grid, block, 0, s, a, head, nvec); break;
    case GN_OPT_AMSGRAD: hipLaunchKernelGGL(optim_kernel<GN_OPT_AMSGRAD>, grid, block, 0, s, a, head, nvec); break;
  }
  return check_launch("optim_step");
}

size_t gn_optim_sumsq_slots(size_t n) {
  const size_t b = cdiv(n / 4 + 1, 256);
  return b < 1 ? 1 : (b > SUMSQ_MAX_BLOCKS ? SUMSQ_MAX_BLOCKS : b);
}
int gn_optim_sumsq(const float* g, size_t n, double* partials, void* stream) {
  GN_REQUIRE(partials && (g || !n), "optim_sumsq: null pointer");
  const size_t head = vec_head(n, {g});
  const size_t nvec = (n - head) / 4;
  hipLaunchKernelGGL(optim_sumsq_kernel, dim3((unsigned)gn_optim_sumsq_slots(n)), dim3(256), 0, (hipStream_t)stream, g, n, head, nvec, partials);
  return check_launch("optim_sumsq");
}
int gn_optim_clip_factor(const double* partials, size_t count, float clipnorm, float* factor, void* stream) {
  GN_REQUIRE(partials && factor && count > 0, "optim_clip_factor: null pointer or no partials");
  GN_REQUIRE(clipnorm > 0.f, "optim_clip_factor: clipnorm %g must be > 0", clipnorm);
  hipLaunchKernelGGL(optim_clip_factor_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partials, count, clipnorm, factor);
  return check_launch("optim_clip_factor");
}

int gn_adam_step(float* p, const float* g, float* m, float* v, size_t n, float lr_t, float b1, float b2, float eps, void* stream) {
  GN_REQUIRE(p && g && m && v, "adam_step: null pointer");
  return adam_step(p, g, m, v, n, lr_t, nullptr, b1, b2, eps, (hipStream_t)stream);
}
int gn_adam_step_dyn(float* p, const float* g, float* m, float* v, size_t n, const float* lr_t_dev, float b1, float b2, float eps, void* stream) {
  GN_REQUIRE(p && g && m && v && lr_t_dev, "adam_step_dyn: null pointer");
  return adam_step(p, g, m, v, n, 0.f, lr_t_dev, b1, b2, eps, (hipStream_t)stream);
}

}  // extern "C"
