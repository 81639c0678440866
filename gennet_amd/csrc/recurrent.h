// What the recurrence kernels share (csrc/lstm.hip; csrc/gru.hip): the activations under the codes of enum gn_lstm_act, their
// derivatives through the output value, and the two launches that write the zero-padded copies of a recurrent kernel U (u, G u) of G gate blocks.
#pragma once
#include <math.h>

#include "common.h"

namespace gn {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float lstm_sigmoid(float x) { return act_apply(x, GN_ACT_SIGMOID, 0.f); }

__device__ __forceinline__ float lstm_act(float x, int code) {
  switch (code) {
    case GN_LSTM_TANH: return gn_tanhf(x);
    case GN_LSTM_SIGMOID: return lstm_sigmoid(x);
    case GN_LSTM_RELU: return fmaxf(x, 0.f);
    case GN_LSTM_HARD_SIGMOID: return fminf(fmaxf(0.2f * x + 0.5f, 0.f), 1.f);
    default: return x;
  }
}

// the derivative through the OUTPUT value y = act(x)
__device__ __forceinline__ float lstm_act_grad(float y, int code) {
  switch (code) {
    case GN_LSTM_TANH: return 1.f - y * y;
    case GN_LSTM_SIGMOID: return y * (1.f - y);
    case GN_LSTM_RELU: return y > 0.f ? 1.f : 0.f;
    case GN_LSTM_HARD_SIGMOID: return (y > 0.f && y < 1.f) ? 0.2f : 0.f;
    default: return 1.f;
  }
}

// up[k * SU + q * UP + j] = U[k][q u + j] for the G gate blocks q, +0 outside u (and in the columns of a row beyond G UP)
__global__ __launch_bounds__(256) void lstm_pad_u_kernel(const float* __restrict__ U, float* __restrict__ up, int u, int KP, int UP, int SU, int G) {
  const int n = KP * SU;
  for (int e = blockIdx.x * 256 + threadIdx.x; e < n; e += gridDim.x * 256) {
    const int k = e / SU, col = e % SU, q = col / UP, j = col % UP;
    up[e] = (k < u && q < G && j < u) ? U[(size_t)k * G * u + q * u + j] : 0.f;
  }
}

// utp[(q * KP + k) * SUT + j] = U[j][q u + k] for the G gate blocks q, +0 outside u
__global__ __launch_bounds__(256) void lstm_pad_ut_kernel(const float* __restrict__ U, float* __restrict__ utp, int u, int KP, int SUT, int G) {
  const int n = G * KP * SUT;
  for (int e = blockIdx.x * 256 + threadIdx.x; e < n; e += gridDim.x * 256) {
    const int row = e / SUT, j = e % SUT, q = row / KP, k = row % KP;
    utp[e] = (k < u && j < u) ? U[(size_t)j * G * u + q * u + k] : 0.f;
  }
}

bool lstm_code_ok(int code, bool recurrent) {
  return recurrent ? (code == GN_LSTM_HARD_SIGMOID || code == GN_LSTM_SIGMOID)
                   : (code == GN_LSTM_TANH || code == GN_LSTM_SIGMOID || code == GN_LSTM_RELU || code == GN_LSTM_LINEAR);
}

}  // namespace
}  // namespace gn
