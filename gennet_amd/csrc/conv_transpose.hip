// Conv2DTranspose (kernel (1, kw), strides (1, s)) runs as the data gradient of the adjoint Conv1D (layers.Conv2DTranspose): the GEMM-shaped
// work goes through gn_conv1d_dgrad / gn_conv1d_fwd / gn_conv1d_wgrad on the existing kernel families.  The data-gradient kernels write no
// bias, so the layer's forward ends in the pass below:
//   y = act(x + bias[c]),  and with a Dropout fused behind it  y = keep ? y / (1 - rate) : 0
// in place over the (rows, C) output, any C.  A thread owns four consecutive elements (one 16-byte access; the tensor base is 16-byte
// aligned and rows * C need not be a multiple of 4, so the last group is done element by element).  With gen != 0 the keep-mask is drawn
// in the same pass exactly as gn_dropout_mask draws it (element k: Philox4x32-10 counter offset + k / 4, lane k % 4, keep iff u >= rate)
// and written out for the backward pass; otherwise a given mask (or none) is read.
#include "common.h"

namespace gn {

template <bool C4>
__global__ __launch_bounds__(256) void bias_act_drop_kernel(float* __restrict__ y, const float* __restrict__ bias, uint8_t* __restrict__ mask, size_t n,
                                                            int C, int act, float p, float rate, float keep_scale, int gen, uint64_t seed, uint64_t offset,
                                                            const uint64_t* __restrict__ base) {
  const size_t n4 = (n + 3) >> 2, stride = (size_t)gridDim.x * blockDim.x;
  if (gen && base) offset += *base;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    const size_t k0 = 4 * i;
    const bool full = k0 + 3 < n;
    float v[4];
    if (full) {
      const float4 v4 = reinterpret_cast<const float4*>(y)[i];
      v[0] = v4.x; v[1] = v4.y; v[2] = v4.z; v[3] = v4.w;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = k0 + e < n ? y[k0 + e] : 0.f;
    }
    float b[4];
    if (C4) {
      const float4 b4 = reinterpret_cast<const float4*>(bias)[(int)(k0 % (size_t)C) >> 2];
      b[0] = b4.x; b[1] = b4.y; b[2] = b4.z; b[3] = b4.w;
    } else {
      int c = (int)(k0 % (size_t)C);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        b[e] = bias[c];
        c = c + 1 == C ? 0 : c + 1;
      }
    }
    uint8_t m[4] = {1, 1, 1, 1};
    if (gen) {
      const Philox4 r = philox4x32_10(offset + i, seed);
#pragma unroll
      for (int e = 0; e < 4; ++e) m[e] = u01_24(r.v[e]) >= rate ? 1 : 0;
    } else if (mask) {
#pragma unroll
      for (int e = 0; e < 4; ++e) m[e] = k0 + e < n ? mask[k0 + e] : 0;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v[e] = act_apply(v[e] + b[e], act, p);
      if (mask) v[e] = m[e] ? v[e] * keep_scale : 0.f;
    }
    if (full) {
      reinterpret_cast<float4*>(y)[i] = make_float4(v[0], v[1], v[2], v[3]);
      if (gen) reinterpret_cast<unsigned*>(mask)[i] = (unsigned)m[0] | ((unsigned)m[1] << 8) | ((unsigned)m[2] << 16) | ((unsigned)m[3] << 24);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (k0 + e < n) {
          y[k0 + e] = v[e];
          if (gen) mask[k0 + e] = m[e];
        }
    }
  }
}

}  // namespace gn

extern "C" int gn_bias_act_dropout(float* y, const float* bias, uint8_t* mask, size_t rows, int C, int act, float act_param, float rate, int gen,
                                   uint64_t seed, uint64_t offset, void* stream) {
  GN_REQUIRE(y && bias && C > 0, "bias_act_dropout: null pointer or C %d", C);
  GN_REQUIRE(rate >= 0.f && rate < 1.f && (mask || (rate == 0.f && !gen)), "bias_act_dropout: dropout rate %f needs a mask buffer", rate);
  const size_t n = rows * (size_t)C;
  if (!n) return GN_OK;
  GN_REQUIRE(!gen || (reinterpret_cast<uintptr_t>(mask) & 3) == 0, "bias_act_dropout: the mask buffer to draw into must be 4-byte aligned");
  const hipStream_t s = (hipStream_t)stream;
  const unsigned grid = gn::stream_grid((n + 3) / 4);
  const float keep_scale = 1.0f / (1.0f - (mask ? rate : 0.f));
  if (C % 4 == 0)
    hipLaunchKernelGGL(gn::bias_act_drop_kernel<true>, dim3(grid), dim3(256), 0, s, y, bias, mask, n, C, act, act_param, rate, keep_scale, gen, seed, offset,
                       gen ? gn::rng_base() : nullptr);
  else
    hipLaunchKernelGGL(gn::bias_act_drop_kernel<false>, dim3(grid), dim3(256), 0, s, y, bias, mask, n, C, act, act_param, rate, keep_scale, gen, seed, offset,
                       gen ? gn::rng_base() : nullptr);
  return gn::check_launch("bias_act_dropout");
}
