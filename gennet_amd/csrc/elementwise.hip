// Streaming (HBM-bound) kernels and their entry points: activations, dropout, upsample, the two stack layers, the discriminator batch,
// gather, axpy and the RNG fills.  All are grid-stride loops sized to ~8 blocks/CU, float4-vectorised where the layout allows; UpSampling1D takes
// any channel count and any 4-byte aligned base on one-float units (16-byte units only when C % 4 == 0 and both pointers are 16-byte aligned).
#include "common.h"

namespace gn {

// ---------------------------------------------------------------------------------------------
// activations
// ---------------------------------------------------------------------------------------------
__global__ void act_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, size_t n, int act, float p) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const size_t n4 = n >> 2;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    float4 v = reinterpret_cast<const float4*>(x)[i];
    v.x = act_apply(v.x, act, p); v.y = act_apply(v.y, act, p); v.z = act_apply(v.z, act, p); v.w = act_apply(v.w, act, p);
    reinterpret_cast<float4*>(y)[i] = v;
  }
  for (size_t i = (n4 << 2) + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) y[i] = act_apply(x[i], act, p);
}

__global__ void act_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y, float* __restrict__ dx, size_t n, int act, float p) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const size_t n4 = n >> 2;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    const float4 g = reinterpret_cast<const float4*>(dy)[i];
    const float4 v = reinterpret_cast<const float4*>(y)[i];
    float4 o;
    o.x = g.x * act_grad_from_y(v.x, act, p); o.y = g.y * act_grad_from_y(v.y, act, p);
    o.z = g.z * act_grad_from_y(v.z, act, p); o.w = g.w * act_grad_from_y(v.w, act, p);
    reinterpret_cast<float4*>(dx)[i] = o;
  }
  for (size_t i = (n4 << 2) + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) dx[i] = dy[i] * act_grad_from_y(y[i], act, p);
}

// fused backward of [activation -> inverted dropout] expressed through the layer output y (post-dropout):
// dx = mask ? dy * keep_scale * act'(y / keep_scale) : 0
__global__ void act_dropout_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y, const uint8_t* __restrict__ mask, float* __restrict__ dx,
                                       size_t n, int act, float p, float keep_scale) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const size_t n4 = n >> 2;
  const float inv = 1.0f / keep_scale;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    const float4 g = reinterpret_cast<const float4*>(dy)[i];
    const float4 v = reinterpret_cast<const float4*>(y)[i];
    const uchar4 k = reinterpret_cast<const uchar4*>(mask)[i];
    float4 o;
    o.x = k.x ? g.x * keep_scale * act_grad_from_y(v.x * inv, act, p) : 0.f; o.y = k.y ? g.y * keep_scale * act_grad_from_y(v.y * inv, act, p) : 0.f;
    o.z = k.z ? g.z * keep_scale * act_grad_from_y(v.z * inv, act, p) : 0.f; o.w = k.w ? g.w * keep_scale * act_grad_from_y(v.w * inv, act, p) : 0.f;
    reinterpret_cast<float4*>(dx)[i] = o;
  }
  for (size_t i = (n4 << 2) + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    dx[i] = mask[i] ? dy[i] * keep_scale * act_grad_from_y(y[i] * inv, act, p) : 0.f;
}

// ---------------------------------------------------------------------------------------------
// dropout: one Philox call yields 4 uniforms -> 4 consecutive mask bytes
// ---------------------------------------------------------------------------------------------
__global__ void dropout_mask_kernel(uint8_t* __restrict__ mask, size_t n, float rate, uint64_t seed, uint64_t offset, const uint64_t* __restrict__ base) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const size_t n4 = (n + 3) >> 2;
  if (base) offset += *base;
  const bool aligned = (reinterpret_cast<uintptr_t>(mask) & 3) == 0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    const Philox4 r = philox4x32_10(offset + i, seed);
    if (aligned && 4 * i + 3 < n) {                          // the four bytes as one dword store (byte stores: 4 instructions, a quarter of each sector)
      unsigned w = 0;
#pragma unroll
      for (int e = 0; e < 4; ++e) w |= (u01_24(r.v[e]) >= rate ? 1u : 0u) << (8 * e);
      reinterpret_cast<unsigned*>(mask)[i] = w;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const size_t k = 4 * i + e;
        if (k < n) mask[k] = u01_24(r.v[e]) >= rate ? 1 : 0;
      }
    }
  }
}

__global__ void dropout_apply_kernel(const float* __restrict__ x, const uint8_t* __restrict__ mask, float* __restrict__ y, size_t n, float scale) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) y[i] = mask[i] ? x[i] * scale : 0.f;
}

// ---------------------------------------------------------------------------------------------
// UpSampling1D(2), MyLayer stack, gather, axpy, RNG fills
// ---------------------------------------------------------------------------------------------
// One lane owns one unit of the UN-upsampled tensor: a float4 when C % 4 == 0 and both tensors are 16-byte aligned, else one float (any channel
// count, any 4-byte aligned base; as dilate.hip chooses).  C: units per row.
__device__ __forceinline__ float add_unit(float a, float b) { return a + b; }
__device__ __forceinline__ float4 add_unit(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

template <typename T>
__global__ void upsample2_fwd_kernel(const T* __restrict__ x, T* __restrict__ y, size_t rows, int C) {
  const size_t n = rows * C, stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const size_t r = i / C, c = i % C;
    const T v = x[i];
    y[(2 * r) * C + c] = v;
    y[(2 * r + 1) * C + c] = v;
  }
}
template <typename T>
__global__ void upsample2_bwd_kernel(const T* __restrict__ dy, T* __restrict__ dx, size_t rows, int C) {
  const size_t n = rows * C, stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const size_t r = i / C, c = i % C;
    dx[i] = add_unit(dy[(2 * r) * C + c], dy[(2 * r + 1) * C + c]);
  }
}
static inline bool upsample2_vec(const void* a, const void* b, int C) { return C % 4 == 0 && (((uintptr_t)a | (uintptr_t)b) & 15) == 0; }

__global__ void subtract_stack_fwd_kernel(const float* __restrict__ x, const float* __restrict__ ev, float2* __restrict__ img, size_t total, int n) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const float v = x[i];
    img[i] = make_float2(v, ev[i % n] - v);
  }
}
__global__ void subtract_stack_bwd_kernel(const float2* __restrict__ d, float* __restrict__ dx, size_t total) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const float2 v = d[i];
    dx[i] = v.x - v.y;
  }
}
// user-defined Layer.call of the form K.stack([a0*x + b0, a1*x + b1], axis=2) (keras/backend.py lowers it here); MyLayer is (1, 0, -1, event)
__global__ void affine_stack_fwd_kernel(const float* __restrict__ x, const float* __restrict__ b0, const float* __restrict__ b1, float a0, float a1,
                                        float2* __restrict__ img, size_t total, int n) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const float v = x[i];
    const int t = (int)(i % n);
    img[i] = make_float2(a0 * v + (b0 ? b0[t] : 0.f), a1 * v + (b1 ? b1[t] : 0.f));
  }
}
__global__ void affine_stack_bwd_kernel(const float2* __restrict__ d, float a0, float a1, float* __restrict__ dx, size_t total) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const float2 v = d[i];
    dx[i] = a0 * v.x + a1 * v.y;
  }
}

// bbhMahoGANy.py:1268-1289: discriminator batch [real | fake] as width-2 images, fake half in reversed sample order
__global__ void assemble_d_batch_kernel(const float* __restrict__ real, const float* __restrict__ noise, const float* __restrict__ fake,
                                        const float* __restrict__ ev, float2* __restrict__ sX, int B, int n) {
  const size_t total = (size_t)2 * B * n, stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int row = (int)(i / n), t = (int)(i % n);
    if (row < B) {
      sX[i] = make_float2(real[(size_t)row * n + t], noise[(size_t)row * n + t]);
    } else {
      const float f = fake[(size_t)(2 * B - 1 - row) * n + t];
      sX[i] = make_float2(f, ev[t] - f);
    }
  }
}

__global__ void gather_rows_kernel(const float* __restrict__ src, const int64_t* __restrict__ idx, float* __restrict__ out, size_t rows, int width) {
  const size_t total = rows * width, stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const size_t r = i / width, c = i % width;
    out[i] = src[(size_t)idx[r] * width + c];
  }
}

__global__ void axpy_kernel(float* __restrict__ y, const float* __restrict__ x, float a, size_t n) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) y[i] = fmaf(a, x[i], y[i]);
}

// [lo, hi): u <= 1 - 2^-24, but lo + (hi - lo) * u can still round up to hi (e.g. (20, 35), (0.5, 1)), so the value is held at top = the largest
// float below hi (computed by the host); a value already below hi keeps its bits
__global__ void fill_uniform_kernel(float* __restrict__ out, size_t n, float lo, float hi, float top, uint64_t seed, uint64_t offset,
                                    const uint64_t* __restrict__ base) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const size_t n4 = (n + 3) >> 2;
  if (base) offset += *base;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    const Philox4 r = philox4x32_10(offset + i, seed);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const size_t k = 4 * i + e;
      if (k < n) out[k] = fminf(lo + (hi - lo) * u01_24(r.v[e]), top);
    }
  }
}
// Box-Muller on two 24-bit uniforms per pair; u1 in (0,1] so log is finite
__global__ void fill_normal_kernel(float* __restrict__ out, size_t n, float mean, float sd, uint64_t seed, uint64_t offset, const uint64_t* __restrict__ base,
                                   const float* __restrict__ sd_dev) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const size_t n4 = (n + 3) >> 2;
  if (base) offset += *base;
  if (sd_dev) sd = *sd_dev;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    const Philox4 r = philox4x32_10(offset + i, seed);
    float z[4];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const float u1 = 1.0f - u01_24(r.v[2 * e]);
      const float u2 = u01_24(r.v[2 * e + 1]);
      const float rad = sqrtf(-2.0f * logf(u1));
      float sn, cs;
      sincosf(6.283185307179586f * u2, &sn, &cs);
      z[2 * e] = rad * cs;
      z[2 * e + 1] = rad * sn;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const size_t k = 4 * i + e;
      if (k < n) out[k] = mean + sd * z[e];
    }
  }
}

static int fill_normal(float* out, size_t n, float mean, float sd, const float* sd_dev, uint64_t seed, uint64_t offset, hipStream_t s) {
  if (!n) return GN_OK;
  hipLaunchKernelGGL(fill_normal_kernel, dim3(stream_grid(n / 4 + 1)), dim3(256), 0, s, out, n, mean, sd, seed, offset, rng_base(), sd_dev);
  return check_launch("fill_normal");
}

}  // namespace gn

using namespace gn;

extern "C" {

int gn_act_fwd(const float* x, float* y, size_t n, int act, float p, void* stream) {
  GN_REQUIRE(x && y, "act_fwd: null pointer");
  if (n == 0) return GN_OK;
  hipLaunchKernelGGL(act_fwd_kernel, dim3(stream_grid(n / 4 + 1)), dim3(256), 0, (hipStream_t)stream, x, y, n, act, p);
  return check_launch("act_fwd");
}
int gn_act_bwd(const float* dy, const float* y, float* dx, size_t n, int act, float p, void* stream) {
  GN_REQUIRE(dy && y && dx, "act_bwd: null pointer");
  if (n == 0) return GN_OK;
  hipLaunchKernelGGL(act_bwd_kernel, dim3(stream_grid(n / 4 + 1)), dim3(256), 0, (hipStream_t)stream, dy, y, dx, n, act, p);
  return check_launch("act_bwd");
}
int gn_act_dropout_bwd(const float* dy, const float* y, const uint8_t* mask, float* dx, size_t n, int act, float p, float rate, void* stream) {
  GN_REQUIRE(dy && y && mask && dx && rate >= 0.f && rate < 1.f, "act_dropout_bwd: bad arguments");
  if (n == 0) return GN_OK;
  hipLaunchKernelGGL(act_dropout_bwd_kernel, dim3(stream_grid(n / 4 + 1)), dim3(256), 0, (hipStream_t)stream, dy, y, mask, dx, n, act, p, 1.0f / (1.0f - rate));
  return check_launch("act_dropout_bwd");
}

int gn_dropout_mask(uint8_t* mask, size_t n, float rate, uint64_t seed, uint64_t offset, void* stream) {
  GN_REQUIRE(mask && rate >= 0.f && rate < 1.f, "dropout_mask: bad arguments");
  if (n == 0) return GN_OK;
  hipLaunchKernelGGL(dropout_mask_kernel, dim3(stream_grid(n / 4 + 1)), dim3(256), 0, (hipStream_t)stream, mask, n, rate, seed, offset, rng_base());
  return check_launch("dropout_mask");
}
int gn_dropout_apply(const float* x, const uint8_t* mask, float* y, size_t n, float rate, void* stream) {
  GN_REQUIRE(x && mask && y && rate >= 0.f && rate < 1.f, "dropout_apply: bad arguments");
  if (n == 0) return GN_OK;
  hipLaunchKernelGGL(dropout_apply_kernel, dim3(stream_grid(n)), dim3(256), 0, (hipStream_t)stream, x, mask, y, n, 1.0f / (1.0f - rate));
  return check_launch("dropout_apply");
}

int gn_upsample2_fwd(const float* x, float* y, int B, int L, int C, void* stream) {
  GN_REQUIRE(x && y, "upsample2_fwd: null pointer");
  GN_REQUIRE(C >= 1, "upsample2: C %d < 1", C);
  const size_t rows = (size_t)B * L;
  if (!rows) return GN_OK;
  if (upsample2_vec(x, y, C))
    hipLaunchKernelGGL(upsample2_fwd_kernel<float4>, dim3(stream_grid(rows * (C / 4))), dim3(256), 0, (hipStream_t)stream, (const float4*)x, (float4*)y, rows, C / 4);
  else
    hipLaunchKernelGGL(upsample2_fwd_kernel<float>, dim3(stream_grid(rows * C)), dim3(256), 0, (hipStream_t)stream, x, y, rows, C);
  return check_launch("upsample2_fwd");
}
int gn_upsample2_bwd(const float* dy, float* dx, int B, int L, int C, void* stream) {
  GN_REQUIRE(dy && dx, "upsample2_bwd: null pointer");
  GN_REQUIRE(C >= 1, "upsample2: C %d < 1", C);
  const size_t rows = (size_t)B * L;
  if (!rows) return GN_OK;
  if (upsample2_vec(dy, dx, C))
    hipLaunchKernelGGL(upsample2_bwd_kernel<float4>, dim3(stream_grid(rows * (C / 4))), dim3(256), 0, (hipStream_t)stream, (const float4*)dy, (float4*)dx, rows, C / 4);
  else
    hipLaunchKernelGGL(upsample2_bwd_kernel<float>, dim3(stream_grid(rows * C)), dim3(256), 0, (hipStream_t)stream, dy, dx, rows, C);
  return check_launch("upsample2_bwd");
}

int gn_subtract_stack_fwd(const float* x, const float* event, float* img, int B, int n, void* stream) {
  GN_REQUIRE(x && event && img, "subtract_stack_fwd: null pointer");
  const size_t total = (size_t)B * n;
  if (!total) return GN_OK;
  hipLaunchKernelGGL(subtract_stack_fwd_kernel, dim3(stream_grid(total)), dim3(256), 0, (hipStream_t)stream, x, event, (float2*)img, total, n);
  return check_launch("subtract_stack_fwd");
}
int gn_subtract_stack_bwd(const float* dimg, float* dx, int B, int n, void* stream) {
  GN_REQUIRE(dimg && dx, "subtract_stack_bwd: null pointer");
  const size_t total = (size_t)B * n;
  if (!total) return GN_OK;
  hipLaunchKernelGGL(subtract_stack_bwd_kernel, dim3(stream_grid(total)), dim3(256), 0, (hipStream_t)stream, (const float2*)dimg, dx, total);
  return check_launch("subtract_stack_bwd");
}
int gn_affine_stack_fwd(const float* x, const float* b0, const float* b1, float a0, float a1, float* img, int B, int n, void* stream) {
  GN_REQUIRE(x && img && B >= 0 && n > 0, "affine_stack_fwd: bad arguments");
  const size_t total = (size_t)B * n;
  if (!total) return GN_OK;
  hipLaunchKernelGGL(affine_stack_fwd_kernel, dim3(stream_grid(total)), dim3(256), 0, (hipStream_t)stream, x, b0, b1, a0, a1, (float2*)img, total, n);
  return check_launch("affine_stack_fwd");
}
int gn_affine_stack_bwd(const float* dimg, float a0, float a1, float* dx, int B, int n, void* stream) {
  GN_REQUIRE(dimg && dx && B >= 0 && n > 0, "affine_stack_bwd: bad arguments");
  const size_t total = (size_t)B * n;
  if (!total) return GN_OK;
  hipLaunchKernelGGL(affine_stack_bwd_kernel, dim3(stream_grid(total)), dim3(256), 0, (hipStream_t)stream, (const float2*)dimg, a0, a1, dx, total);
  return check_launch("affine_stack_bwd");
}
int gn_assemble_d_batch(const float* real, const float* noise, const float* fake, const float* event, float* sX, int B, int n, void* stream) {
  GN_REQUIRE(real && noise && fake && event && sX && B >= 0 && n > 0, "assemble_d_batch: bad arguments");
  if (!B) return GN_OK;
  hipLaunchKernelGGL(assemble_d_batch_kernel, dim3(stream_grid((size_t)2 * B * n)), dim3(256), 0, (hipStream_t)stream, real, noise, fake, event, (float2*)sX, B, n);
  return check_launch("assemble_d_batch");
}

int gn_gather_rows(const float* src, const int64_t* idx, float* out, int rows, int width, void* stream) {
  GN_REQUIRE(src && idx && out && rows >= 0 && width > 0, "gather_rows: bad arguments");
  const size_t total = (size_t)rows * width;
  if (!total) return GN_OK;
  hipLaunchKernelGGL(gather_rows_kernel, dim3(stream_grid(total)), dim3(256), 0, (hipStream_t)stream, src, idx, out, (size_t)rows, width);
  return check_launch("gather_rows");
}
int gn_axpy(float* y, const float* x, float a, size_t n, void* stream) {
  GN_REQUIRE(y && x, "axpy: null pointer");
  if (!n) return GN_OK;
  hipLaunchKernelGGL(axpy_kernel, dim3(stream_grid(n)), dim3(256), 0, (hipStream_t)stream, y, x, a, n);
  return check_launch("axpy");
}

int gn_fill_uniform(float* out, size_t n, float lo, float hi, uint64_t seed, uint64_t offset, void* stream) {
  GN_REQUIRE(out, "fill_uniform: null pointer");
  if (!n) return GN_OK;
  hipLaunchKernelGGL(fill_uniform_kernel, dim3(stream_grid(n / 4 + 1)), dim3(256), 0, (hipStream_t)stream, out, n, lo, hi, lo < hi ? nextafterf(hi, lo) : INFINITY, seed,
                     offset, rng_base());
  return check_launch("fill_uniform");
}
int gn_fill_normal(float* out, size_t n, float mean, float sd, uint64_t seed, uint64_t offset, void* stream) {
  GN_REQUIRE(out, "fill_normal: null pointer");
  return fill_normal(out, n, mean, sd, nullptr, seed, offset, (hipStream_t)stream);
}
// sd from device memory: what a captured hipGraph of a train step needs (a by-value argument is frozen at capture)
int gn_fill_normal_dyn(float* out, size_t n, float mean, const float* sd_dev, uint64_t seed, uint64_t offset, void* stream) {
  GN_REQUIRE(out && sd_dev, "fill_normal_dyn: null pointer");
  return fill_normal(out, n, mean, 0.f, sd_dev, seed, offset, (hipStream_t)stream);
}

}  // extern "C"
