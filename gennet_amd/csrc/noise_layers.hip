// Keras 2.2.4 noise layers (layers/noise.py): GaussianNoise, GaussianDropout, AlphaDropout.  Each entry is one streaming pass that draws its
// random numbers in the same pass, on dropout_mask_kernel's layout: element k uses Philox4x32-10 counter (offset + k/4), lane k%4; one Philox
// call per float4 group.  The normal draw is fill_normal_kernel's (Box-Muller on lanes (0,1) and (2,3)) and the keep test is dropout_mask_kernel's
// (u01_24 >= rate), bit for bit, so the layers can be checked against gn_fill_normal / gn_dropout_mask.  The backward passes regenerate the
// draw from (seed, offset) instead of reading a stored multiplier.  x == y (in place) is allowed.
#include "common.h"

namespace gn {

// fill_normal_kernel's four N(0,1) values of one Philox call, the same expressions in the same order
__device__ __forceinline__ void normal4(const Philox4& r, float z[4]) {
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
}

enum NoiseOp { NOISE_ADD = 0, NOISE_MUL = 1, ALPHA_FWD = 2, ALPHA_BWD = 3 };

// NOISE_ADD: y = x + p0 z;  NOISE_MUL: y = x (1 + p0 z);  ALPHA_FWD: y = keep ? p0 x + p1 : p0 p2 + p1;  ALPHA_BWD: y = keep ? p0 x : 0
template <int OP>
__global__ void noise_kernel(const float* x, float* y, size_t n, float p0, float p1, float p2, float rate, uint64_t seed, uint64_t offset,
                             const uint64_t* __restrict__ base) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const size_t n4 = (n + 3) >> 2;
  if (base) offset += *base;
  const bool aligned = ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15) == 0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    const Philox4 r = philox4x32_10(offset + i, seed);
    float v[4];
    if (aligned && 4 * i + 3 < n) {
      const float4 a = reinterpret_cast<const float4*>(x)[i];
      v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = 4 * i + e < n ? x[4 * i + e] : 0.f;
    }
    if (OP == NOISE_ADD || OP == NOISE_MUL) {
      float z[4];
      normal4(r, z);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = OP == NOISE_ADD ? v[e] + p0 * z[e] : v[e] * (1.0f + p0 * z[e]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool keep = u01_24(r.v[e]) >= rate;
        v[e] = OP == ALPHA_FWD ? (keep ? p0 * v[e] + p1 : p0 * p2 + p1) : (keep ? p0 * v[e] : 0.f);
      }
    }
    if (aligned && 4 * i + 3 < n) {
      reinterpret_cast<float4*>(y)[i] = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (4 * i + e < n) y[4 * i + e] = v[e];
    }
  }
}

template <int OP>
static int noise_launch(const char* what, const float* x, float* y, size_t n, float p0, float p1, float p2, float rate, uint64_t seed,
                        uint64_t offset, hipStream_t s) {
  if (!n) return GN_OK;
  hipLaunchKernelGGL(noise_kernel<OP>, dim3(stream_grid(n / 4 + 1)), dim3(256), 0, s, x, y, n, p0, p1, p2, rate, seed, offset, rng_base());
  return check_launch(what);
}

}  // namespace gn

using namespace gn;

extern "C" {

int gn_gaussian_noise_fwd(const float* x, float* y, size_t n, float stddev, uint64_t seed, uint64_t offset, void* stream) {
  GN_REQUIRE((x && y) || !n, "gaussian_noise_fwd: null pointer");
  return noise_launch<NOISE_ADD>("gaussian_noise_fwd", x, y, n, stddev, 0.f, 0.f, 0.f, seed, offset, (hipStream_t)stream);
}
int gn_gaussian_dropout_apply(const float* x, float* y, size_t n, float sd, uint64_t seed, uint64_t offset, void* stream) {
  GN_REQUIRE((x && y) || !n, "gaussian_dropout_apply: null pointer");
  return noise_launch<NOISE_MUL>("gaussian_dropout_apply", x, y, n, sd, 0.f, 0.f, 0.f, seed, offset, (hipStream_t)stream);
}
int gn_alpha_dropout_fwd(const float* x, float* y, size_t n, float rate, float a, float b, float alpha_p, uint64_t seed, uint64_t offset, void* stream) {
  GN_REQUIRE(((x && y) || !n) && rate > 0.f && rate < 1.f, "alpha_dropout_fwd: bad arguments");
  return noise_launch<ALPHA_FWD>("alpha_dropout_fwd", x, y, n, a, b, alpha_p, rate, seed, offset, (hipStream_t)stream);
}
int gn_alpha_dropout_bwd(const float* dy, float* dx, size_t n, float rate, float a, uint64_t seed, uint64_t offset, void* stream) {
  GN_REQUIRE(((dy && dx) || !n) && rate > 0.f && rate < 1.f, "alpha_dropout_bwd: bad arguments");
  return noise_launch<ALPHA_BWD>("alpha_dropout_bwd", dy, dx, n, a, 0.f, 0.f, rate, seed, offset, (hipStream_t)stream);
}

}  // extern "C"
