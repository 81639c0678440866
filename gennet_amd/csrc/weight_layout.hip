// Weight-layout passes, run once per step on a layer's kernel or its gradient: the tap-wise transpose the data gradients read, the width-2
// Conv2D fold / unfold and the UpSampling1D(2) -> Conv1D fold / unfold.
#include "common.h"

namespace gn {

__global__ void transpose_w_kernel(const float* __restrict__ w, float* __restrict__ wt, int k, int Cin, int Cout) {
  __shared__ float tile[32][33];
  const int j = blockIdx.z;
  const int c0 = blockIdx.y * 32, n0 = blockIdx.x * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  for (int r = ty; r < 32; r += 8) {
    const int c = c0 + r, n = n0 + tx;
    tile[r][tx] = (c < Cin && n < Cout) ? w[((size_t)j * Cin + c) * Cout + n] : 0.f;
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int n = n0 + r, c = c0 + tx;
    if (n < Cout && c < Cin) wt[((size_t)j * Cout + n) * Cin + c] = tile[tx][r];
  }
}
int transpose_w(const float* w, float* wt, int k, int Cin, int Cout, hipStream_t s) {
  hipLaunchKernelGGL(transpose_w_kernel, dim3(cdiv(Cout, 32), cdiv(Cin, 32), k), dim3(256), 0, s, w, wt, k, Cin, Cout);
  return check_launch("transpose_w");
}

__global__ void conv2d_w2_fold_kernel(const float* __restrict__ w, const float* __restrict__ bias, float* __restrict__ wf, float* __restrict__ bf, int kh, int Cin, int Cout) {
  const size_t total = (size_t)kh * 2 * Cin * 2 * Cout, stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int co = (int)(i % (2 * Cout));
    const int ci = (int)((i / (2 * Cout)) % (2 * Cin));
    const int h = (int)(i / ((size_t)4 * Cin * Cout));
    const int wo = co / Cout, c2 = co % Cout, wi = ci / Cin, c = ci % Cin;
    wf[i] = w[(((size_t)h * 5 + (wi - wo + 2)) * Cin + c) * Cout + c2];
  }
  if (bias && blockIdx.x == 0)
    for (int o = threadIdx.x; o < 2 * Cout; o += blockDim.x) bf[o] = bias[o % Cout];
}
__global__ void conv2d_w2_unfold_kernel(const float* __restrict__ dwf, const float* __restrict__ dbf, float* __restrict__ dw, float* __restrict__ db, int kh, int Cin, int Cout) {
  const size_t total = (size_t)kh * 5 * Cin * Cout, stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int c2 = (int)(i % Cout);
    const int c = (int)((i / Cout) % Cin);
    const int kw = (int)((i / ((size_t)Cin * Cout)) % 5);
    const int h = (int)(i / ((size_t)5 * Cin * Cout));
    float s = 0.f;
    for (int wi = 0; wi < 2; ++wi) {
      const int wo = wi + 2 - kw;
      if (wo < 0 || wo > 1) continue;
      s += dwf[((size_t)h * 2 * Cin + wi * Cin + c) * (2 * Cout) + wo * Cout + c2];
    }
    dw[i] = s;
  }
  if (db && blockIdx.x == 0)
    for (int o = threadIdx.x; o < Cout; o += blockDim.x) db[o] = dbf[o] + dbf[Cout + o];
}

// UpSampling1D(2) -> Conv1D(k=5, 'same') folded into a 3-tap stride-1 conv on the un-upsampled input:
//   stride 2:  y[t]    = W0 x[t-1] + (W1+W2) x[t] + (W3+W4) x[t+1]                                   wf (3, Cin, Cout)
//   stride 1:  y[2s]   = (W0+W1) x[s-1] + (W2+W3) x[s] + W4 x[s+1]   (columns [0, Cout) of wf)         wf (3, Cin, 2*Cout)
//              y[2s+1] = W0 x[s-1] + (W1+W2) x[s] + (W3+W4) x[s+1]   (columns [Cout, 2*Cout))
// the (Lin, 2*Cout) output of the stride-1 form IS the (2*Lin, Cout) tensor in memory.  tap k of W lands on folded tap UP2_TAB[phase][k].
__device__ __constant__ int UP2_TAB[2][5] = {{0, 0, 1, 1, 2}, {0, 1, 1, 2, 2}};
__global__ void up2_fold_kernel(const float* __restrict__ w, const float* __restrict__ bias, float* __restrict__ wf, float* __restrict__ bf, int Cin, int Cout, int stride) {
  const int phases = stride == 1 ? 2 : 1, Cf = phases * Cout;
  const size_t total = (size_t)3 * Cin * Cf, step = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += step) {
    const int o = (int)(i % Cf);
    const int c = (int)((i / Cf) % Cin);
    const int j = (int)(i / ((size_t)Cin * Cf));
    const int ph = stride == 1 ? o / Cout : 1, n = o % Cout;
    float v = 0.f;
#pragma unroll
    for (int k = 0; k < 5; ++k)
      if (UP2_TAB[ph][k] == j) v += w[((size_t)k * Cin + c) * Cout + n];
    wf[i] = v;
  }
  if (bias && blockIdx.x == 0)
    for (int o = threadIdx.x; o < Cf; o += blockDim.x) bf[o] = bias[o % Cout];
}
__global__ void up2_unfold_kernel(const float* __restrict__ dwf, const float* __restrict__ dbf, float* __restrict__ dw, float* __restrict__ db, int Cin, int Cout, int stride) {
  const int Cf = (stride == 1 ? 2 : 1) * Cout;
  const size_t total = (size_t)5 * Cin * Cout, step = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += step) {
    const int n = (int)(i % Cout);
    const int c = (int)((i / Cout) % Cin);
    const int k = (int)(i / ((size_t)Cin * Cout));
    float v = dwf[((size_t)UP2_TAB[1][k] * Cin + c) * Cf + (stride == 1 ? Cout : 0) + n];
    if (stride == 1) v = dwf[((size_t)UP2_TAB[0][k] * Cin + c) * Cf + n] + v;
    dw[i] = v;
  }
  if (db && blockIdx.x == 0)
    for (int o = threadIdx.x; o < Cout; o += blockDim.x) db[o] = stride == 1 ? dbf[o] + dbf[Cout + o] : dbf[o];
}

}  // namespace gn

using namespace gn;

extern "C" {

int gn_conv1d_transpose_w(const float* w, float* wt, int k, int Cin, int Cout, void* stream) {
  GN_REQUIRE(w && wt && k >= 1 && Cin > 0 && Cout > 0, "transpose_w: bad arguments");
  return transpose_w(w, wt, k, Cin, Cout, (hipStream_t)stream);
}

int gn_conv2d_w2_fold(const float* w, const float* bias, float* wf, float* biasf, int kh, int Cin, int Cout, void* stream) {
  GN_REQUIRE(w && wf && kh >= 1 && Cin > 0 && Cout > 0, "conv2d_w2_fold: bad arguments");
  hipLaunchKernelGGL(conv2d_w2_fold_kernel, dim3(stream_grid((size_t)kh * 4 * Cin * Cout)), dim3(256), 0, (hipStream_t)stream, w, bias, wf, biasf, kh, Cin, Cout);
  return check_launch("conv2d_w2_fold");
}
int gn_conv2d_w2_unfold_grad(const float* dwf, const float* dbf, float* dw, float* db, int kh, int Cin, int Cout, void* stream) {
  GN_REQUIRE(dwf && dw && kh >= 1 && Cin > 0 && Cout > 0, "conv2d_w2_unfold_grad: bad arguments");
  hipLaunchKernelGGL(conv2d_w2_unfold_kernel, dim3(stream_grid((size_t)kh * 5 * Cin * Cout)), dim3(256), 0, (hipStream_t)stream, dwf, dbf, dw, db, kh, Cin, Cout);
  return check_launch("conv2d_w2_unfold");
}

int gn_conv1d_up2_fold(const float* w, const float* bias, float* wf, float* biasf, int Cin, int Cout, int stride, void* stream) {
  GN_REQUIRE(w && wf && Cin > 0 && Cout > 0 && (stride == 1 || stride == 2), "conv1d_up2_fold: bad arguments (5-tap 'same' conv, stride 1 or 2)");
  hipLaunchKernelGGL(up2_fold_kernel, dim3(stream_grid((size_t)6 * Cin * Cout)), dim3(256), 0, (hipStream_t)stream, w, bias, wf, biasf, Cin, Cout, stride);
  return check_launch("up2_fold");
}
int gn_conv1d_up2_unfold_grad(const float* dwf, const float* dbf, float* dw, float* db, int Cin, int Cout, int stride, void* stream) {
  GN_REQUIRE(dwf && dw && Cin > 0 && Cout > 0 && (stride == 1 || stride == 2) && (!db || dbf), "conv1d_up2_unfold_grad: bad arguments");
  hipLaunchKernelGGL(up2_unfold_kernel, dim3(stream_grid((size_t)5 * Cin * Cout)), dim3(256), 0, (hipStream_t)stream, dwf, dbf, dw, db, Cin, Cout, stride);
  return check_launch("up2_unfold");
}

}  // extern "C"
