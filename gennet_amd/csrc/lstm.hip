// keras.layers.LSTM (keras 2.2.4 layers/recurrent.py, LSTMCell): the recurrence as one persistent kernel a direction; DESIGN 8o.
//
//   z_t = zx_t + h_{t-1} . U + b        zx = X . W for all steps comes in (one gn_bmm over B T rows), gate columns i, f, c, o of width u
//   i = ra(z_i)  f = ra(z_f)  g = act(z_c)  o = ra(z_o)        c_t = f c_{t-1} + i g        h_t = o act(c_t)
//
// OWNERSHIP.  The recurrence couples the units of one sample and never two samples, so a block owns LSTM_ROWS = 16 batch rows and walks all T
// steps alone: no block waits on another one, no grid barrier, no cooperative launch, no atomics.  grid = ceil(B / 16) blocks.
//
// TILING.  The step product (16, u) x (u, 4u) runs on v_mfma_f32_16x16x4_f32 (A[row = lane & 15][k = lane >> 4], B[k = lane >> 4][col = lane & 15],
// C[row = 4 (lane >> 4) + reg][col = lane & 15]).  A wave owns NT tiles of 16 units (tile = wave + nwaves i) and forms the FOUR gate columns of its
// units in four accumulators, so a lane holds z_i, z_f, z_c, z_o of the same (row, unit) and the gate arithmetic, c_t and h_t never leave its
// registers; c lives in registers for the whole sequence (4 NT a lane).  h lies in LDS as hs[row][k] with a row of KP + 1 floats (KP = u up to a
// multiple of 8; odd row length: the 16 rows of a fragment read fall on 16 banks), twice: step t reads one copy and writes the other, ONE barrier a
// step.  nwaves = ceil(ntiles / NT) <= 8, NT = ceil(ntiles / 8) <= 4 (lstm_geom.h).
//   backward: the same ownership, t walks down.  A lane holds dh and dc of its (row, unit) in registers, forms the four dz of the step from the
// stored gates and c, writes them to global memory and to LDS (dzs[row][gate KP + k], a row of 4 KP + 1 floats), and after a barrier the wave forms
// dh_{t-1} = dz_t . U^T for its units as one chain over the 4 KP gate columns; a second barrier frees dzs for the next step.
//
// U.  The entry points first write a zero-padded copy of U into the workspace (one small launch): forward Up[k][gate UP + j] with a row of
// SU = 4 UP + 16 floats, backward the transpose Ut[gate KP + k][j] with a row of SUT = UP | 16 floats (UP = u up to a multiple of 16), so the
// B fragments are 16 consecutive floats a k row, no guard stands in the loops, and everything outside u is an exact +0.  Which path a u takes is
// decided in ONE place, lstm_geom():
//   forward   u <= 88: the padded U is copied into LDS once a block (the state and U fit 160 KiB);  89 <= u <= 512: U streams from L2 every step
//   backward  u <= 80: U^T in LDS;  81 <= u <= 512: streamed
//
// NUMERICS.  Every z is ONE fp32 fma chain over k = 0 .. u-1 from +0 (the f32 MFMA is bit for bit that chain), then + zx, then + b; dh_{t-1} one chain
// over the gate columns i, f, c, o in k order, then dy_{t-1} + that.  The padding adds fma(+0, +0, c) = c.  Row m of an MFMA result depends on row m of
// A alone, so a sample's outputs and gradients do not depend on B, on the tile it falls in or on the launch; rows of a tile beyond B run on zeros and
// are never stored.  tanh and sigmoid are gn_tanhf and the sigmoid of common.h; hard_sigmoid is min(max(0.2 x + 0.5, 0), 1) with the product and
// the sum rounded separately, its derivative 0.2 where the stored gate is strictly between 0 and 1.
//
// STORED for the backward (training flag): the activated gates (B, T, 4u) and c (B, T, u) at the INPUT time index of their step, and hprev (B, T, u):
// the h that entered the step at that input time (h0 at the first one).  With them dz lands at the input time index as well, so dW = X^T dz,
// dU = hprev^T dz and dX = dz W^T are one product each over B T rows whatever the direction.  h itself is written in processing order, as keras
// returns it.
//
// A PAIR OF DIRECTIONS (keras Bidirectional).  The two kernels take a second grid dimension: blockIdx.y is the direction d, which picks
// its own zx, padded U, bias, stored tensors and h / dy base pointer from the two-entry table of the arguments; direction 0 walks with `reverse`,
// direction 1 with its negation.  h and dy go through a row stride ld >= u (one (B, T, 2u) buffer at columns 0 and u, or two buffers), direction 0
// at position s of step s, direction 1 at position T-1-s; with `seq` off only the last processed step is written, into a (B, ld) row buffer.
// gn_lstm_fwd / gn_lstm_bwd launch one direction with ld = u; gn_lstm_pair_fwd / _bwd launch two, the padded U of both in the workspace.
#include <math.h>

#include "common.h"
#include "lstm_geom.h"
#include "recurrent.h"          // the activations and the launches that pad U, shared with csrc/gru.hip

namespace gn {
namespace {

struct LstmFwdDir {
  const float* zx;      // (B, T, 4u)
  const float* up;      // padded U: KP rows of SU floats
  const float* bias;    // (4u)
  const float* h0;      // (B, u) or NULL
  const float* c0;
  float* h;             // seq: (B, T, ld) rows of which the direction owns u columns; else (B, ld), the last processed step
  float* gates;         // (B, T, 4u), input time order; training only
  float* c;             // (B, T, u)
  float* hprev;         // (B, T, u)
};

// blockIdx.y is the direction: 0 walks with `reverse` and writes step s at position s, 1 walks with !reverse and writes it at position T-1-s
struct LstmFwdArgs {
  LstmFwdDir d[2];
  int B, T, u, KP, UP, SU, ntiles, act, ract, reverse, training, ld, seq;
};

template <int NT, bool ULDS>
__global__ __launch_bounds__(64 * LSTM_MAX_WAVES) void lstm_fwd_kernel(LstmFwdArgs g) {
  const bool second = blockIdx.y != 0;
  const LstmFwdDir p = second ? g.d[1] : g.d[0];
  const bool reverse = second ? !g.reverse : (g.reverse != 0);
  const size_t h_row = g.seq ? (size_t)g.T * g.ld : (size_t)g.ld;              // floats between two samples of h
  extern __shared__ __attribute__((aligned(16))) float lstm_lds[];
  const int SH = g.KP + 1;
  float* hs0 = lstm_lds;
  float* hs1 = lstm_lds + LSTM_ROWS * SH;
  float* us = lstm_lds + 2 * LSTM_ROWS * SH;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int fc = lane & 15, fq = lane >> 4;
  const size_t b0 = (size_t)blockIdx.x * LSTM_ROWS;
  const size_t u = (size_t)g.u, T = (size_t)g.T;

  for (int e = threadIdx.x; e < LSTM_ROWS * SH; e += blockDim.x) {
    const int row = e / SH, k = e % SH;
    hs0[e] = (p.h0 && k < g.u && b0 + row < (size_t)g.B) ? p.h0[(b0 + row) * u + k] : 0.f;
    hs1[e] = 0.f;
  }
  if (ULDS)
    for (int e = threadIdx.x; e < g.KP * g.SU; e += blockDim.x) us[e] = p.up[e];
  const float* __restrict__ ub = ULDS ? (const float*)us : p.up;

  float creg[NT][4], bias[NT][4];
  const size_t t_first = reverse ? T - 1 : 0;
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    const int tile = wave + nw * i, j = tile * LSTM_TILE + fc;
    const bool jok = tile < g.ntiles && j < g.u;
#pragma unroll
    for (int q = 0; q < 4; ++q) bias[i][q] = jok ? p.bias[q * g.u + j] : 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const size_t row = b0 + 4 * fq + r;
      const bool ok = jok && row < (size_t)g.B;
      creg[i][r] = (ok && p.c0) ? p.c0[row * u + j] : 0.f;
      if (ok && g.training) p.hprev[(row * T + t_first) * u + j] = p.h0 ? p.h0[row * u + j] : 0.f;
    }
  }
  __syncthreads();

  for (int s = 0; s < g.T; ++s) {
    const size_t t_in = reverse ? T - 1 - s : (size_t)s;
    const size_t t_next = reverse ? t_in - 1 : t_in + 1;          // read only while s + 1 < T
    const float* cur = (s & 1) ? hs1 : hs0;
    float* nxt = (s & 1) ? hs0 : hs1;
    const bool h_out = g.seq || s == g.T - 1;
    const size_t h_pos = g.seq ? (size_t)(second ? g.T - 1 - s : s) * g.ld : 0;
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      const int tile = wave + nw * i;
      if (tile < g.ntiles) {                                        // the same for all lanes of a wave
        const int j0 = tile * LSTM_TILE, j = j0 + fc;
        const bool jok = j < g.u;
        float zv[4][4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const size_t row = b0 + 4 * fq + r;
          const bool ok = jok && row < (size_t)g.B;
#pragma unroll
          for (int q = 0; q < 4; ++q) zv[q][r] = ok ? p.zx[((row * T + t_in) * 4 + q) * u + j] : 0.f;
        }
        f32x4 acc[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
        const float* ap = cur + fc * SH + fq;
        const float* bp = ub + fq * g.SU + j;
        for (int k0 = 0; k0 < g.KP; k0 += 8) {                       // KP is a multiple of 8: two k groups of 4 a turn, loads first
          const float* bk = bp + (size_t)k0 * g.SU;
          float a[2], b[2][4];
#pragma unroll
          for (int kk = 0; kk < 2; ++kk) {
            a[kk] = ap[k0 + 4 * kk];
#pragma unroll
            for (int q = 0; q < 4; ++q) b[kk][q] = bk[(size_t)4 * kk * g.SU + q * g.UP];
          }
#pragma unroll
          for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[kk], b[kk][q], acc[q], 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const size_t row = b0 + 4 * fq + r;
          const float gi = lstm_act((acc[0][r] + zv[0][r]) + bias[i][0], g.ract);
          const float gf = lstm_act((acc[1][r] + zv[1][r]) + bias[i][1], g.ract);
          const float gg = lstm_act((acc[2][r] + zv[2][r]) + bias[i][2], g.act);
          const float go = lstm_act((acc[3][r] + zv[3][r]) + bias[i][3], g.ract);
          const float cn = gf * creg[i][r] + gi * gg;
          const float hn = go * lstm_act(cn, g.act);
          creg[i][r] = cn;
          if (jok) {
            nxt[(4 * fq + r) * SH + j] = hn;
            if (row < (size_t)g.B) {
              if (h_out) p.h[row * h_row + h_pos + j] = hn;
              if (g.training) {
                float* gp = p.gates + (row * T + t_in) * 4 * u + j;
                gp[0] = gi;
                gp[u] = gf;
                gp[2 * u] = gg;
                gp[3 * u] = go;
                p.c[(row * T + t_in) * u + j] = cn;
                if (s + 1 < g.T) p.hprev[(row * T + t_next) * u + j] = hn;
              }
            }
          }
        }
      }
    }
    __syncthreads();          // h_t is complete in nxt, and every wave has left cur, which step t + 1 overwrites
  }
}

struct LstmBwdDir {
  const float* dy;      // dy_seq: (B, T, ld) rows at the positions the forward wrote; else (B, ld) for the last step
  const float* gates;
  const float* c;
  const float* c0;
  const float* utp;     // padded U^T: 4 KP rows of SUT floats
  float* dz;            // (B, T, 4u), input time order
  float* dh0;           // (B, u) or NULL
  float* dc0;
};

// blockIdx.y is the direction, as in the forward
struct LstmBwdArgs {
  LstmBwdDir d[2];
  int B, T, u, KP, UP, SUT, ntiles, act, ract, reverse, dy_seq, ld;
};

template <int NT, bool ULDS>
__global__ __launch_bounds__(64 * LSTM_MAX_WAVES) void lstm_bwd_kernel(LstmBwdArgs g) {
  const bool second = blockIdx.y != 0;
  const LstmBwdDir p = second ? g.d[1] : g.d[0];
  const bool reverse = second ? !g.reverse : (g.reverse != 0);
  const size_t dy_row = g.dy_seq ? (size_t)g.T * g.ld : (size_t)g.ld;          // floats between two samples of dy
  extern __shared__ __attribute__((aligned(16))) float lstm_lds[];
  const int SD = 4 * g.KP + 1;
  float* dzs = lstm_lds;
  float* us = lstm_lds + LSTM_ROWS * SD;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int fc = lane & 15, fq = lane >> 4;
  const size_t b0 = (size_t)blockIdx.x * LSTM_ROWS;
  const size_t u = (size_t)g.u, T = (size_t)g.T;

  for (int e = threadIdx.x; e < LSTM_ROWS * SD; e += blockDim.x) dzs[e] = 0.f;
  if (ULDS)
    for (int e = threadIdx.x; e < 4 * g.KP * g.SUT; e += blockDim.x) us[e] = p.utp[e];
  const float* __restrict__ ub = ULDS ? (const float*)us : p.utp;

  float dh[NT][4], dc[NT][4];
#pragma unroll
  for (int i = 0; i < NT; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) dh[i][r] = dc[i][r] = 0.f;
  __syncthreads();

  for (int s = g.T - 1; s >= 0; --s) {
    const size_t t_in = reverse ? T - 1 - s : (size_t)s;
    const size_t t_prev = reverse ? t_in + 1 : t_in - 1;          // read only while s > 0
    const bool dy_in = g.dy_seq || s == g.T - 1;
    const size_t dy_pos = g.dy_seq ? (size_t)(second ? g.T - 1 - s : s) * g.ld : 0;
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      const int tile = wave + nw * i, j = tile * LSTM_TILE + fc;
      if (tile < g.ntiles && j < g.u) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const size_t row = b0 + 4 * fq + r;
          if (row < (size_t)g.B) {                                  // rows beyond B keep their +0 in dzs
            const float* gp = p.gates + (row * T + t_in) * 4 * u + j;
            const float gi = gp[0], gf = gp[u], gg = gp[2 * u], go = gp[3 * u];
            const float cs = p.c[(row * T + t_in) * u + j];
            const float cp = s > 0 ? p.c[(row * T + t_prev) * u + j] : (p.c0 ? p.c0[row * u + j] : 0.f);
            const float dyv = dy_in ? p.dy[row * dy_row + dy_pos + j] : 0.f;
            const float dhv = dyv + dh[i][r];
            const float tc = lstm_act(cs, g.act);
            const float dcv = dc[i][r] + (dhv * go) * lstm_act_grad(tc, g.act);
            const float dzi = (dcv * gg) * lstm_act_grad(gi, g.ract);
            const float dzf = (dcv * cp) * lstm_act_grad(gf, g.ract);
            const float dzg = (dcv * gi) * lstm_act_grad(gg, g.act);
            const float dzo = (dhv * tc) * lstm_act_grad(go, g.ract);
            dc[i][r] = dcv * gf;
            float* zp = p.dz + (row * T + t_in) * 4 * u + j;
            zp[0] = dzi;
            zp[u] = dzf;
            zp[2 * u] = dzg;
            zp[3 * u] = dzo;
            float* ls = dzs + (4 * fq + r) * SD + j;
            ls[0] = dzi;
            ls[g.KP] = dzf;
            ls[2 * g.KP] = dzg;
            ls[3 * g.KP] = dzo;
          }
        }
      }
    }
    __syncthreads();          // dz_t is complete in dzs
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      const int tile = wave + nw * i;
      if (tile < g.ntiles) {
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
        const float* ap = dzs + fc * SD + fq;
        const float* bp = ub + fq * g.SUT + tile * LSTM_TILE + fc;
        for (int k0 = 0; k0 < 4 * g.KP; k0 += 32) {                  // 4 KP is a multiple of 32: eight k groups of 4 a turn, loads first
          float a[8], b[8];
#pragma unroll
          for (int kk = 0; kk < 8; ++kk) {
            a[kk] = ap[k0 + 4 * kk];
            b[kk] = bp[(size_t)(k0 + 4 * kk) * g.SUT];
          }
#pragma unroll
          for (int kk = 0; kk < 8; ++kk) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[kk], b[kk], acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) dh[i][r] = acc[r];
      }
    }
    __syncthreads();          // every wave has left dzs, which step t - 1 overwrites
  }

#pragma unroll
  for (int i = 0; i < NT; ++i) {
    const int tile = wave + nw * i, j = tile * LSTM_TILE + fc;
    if (tile < g.ntiles && j < g.u) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const size_t row = b0 + 4 * fq + r;
        if (row < (size_t)g.B) {
          if (p.dh0) p.dh0[row * u + j] = dh[i][r];
          if (p.dc0) p.dc0[row * u + j] = dc[i][r];
        }
      }
    }
  }
}

template <int NT, bool ULDS>
void launch_fwd(const LstmFwdArgs& a, const LstmGeom& m, int ndir, hipStream_t s) {
  static unsigned long long big = 0;
  allow_big_lds((const void*)lstm_fwd_kernel<NT, ULDS>, &big);
  hipLaunchKernelGGL((lstm_fwd_kernel<NT, ULDS>), dim3(cdiv(a.B, LSTM_ROWS), ndir), dim3(64 * m.nwaves), m.fwd_lds_bytes, s, a);
}

template <int NT, bool ULDS>
void launch_bwd(const LstmBwdArgs& a, const LstmGeom& m, int ndir, hipStream_t s) {
  static unsigned long long big = 0;
  allow_big_lds((const void*)lstm_bwd_kernel<NT, ULDS>, &big);
  hipLaunchKernelGGL((lstm_bwd_kernel<NT, ULDS>), dim3(cdiv(a.B, LSTM_ROWS), ndir), dim3(64 * m.nwaves), m.bwd_lds_bytes, s, a);
}

// pads the U of the ndir directions into the workspace, one copy after the other, and launches the ndir directions as ONE grid
void run_fwd(LstmFwdArgs a, const float* const* U, int ndir, const LstmGeom& m, float* ws, hipStream_t s) {
  for (int d = 0; d < ndir; ++d) {
    float* up = ws + d * m.fwd_ws_floats;
    hipLaunchKernelGGL(lstm_pad_u_kernel, dim3(stream_grid(m.fwd_ws_floats)), dim3(256), 0, s, U[d], up, a.u, m.KP, m.UP, m.SU, 4);
    a.d[d].up = up;
  }
  if (m.fwd_u_lds) launch_fwd<1, true>(a, m, ndir, s);     // u <= 88: six tiles at the most, one a wave
  else if (m.NT == 1) launch_fwd<1, false>(a, m, ndir, s);
  else if (m.NT == 2) launch_fwd<2, false>(a, m, ndir, s);
  else if (m.NT == 3) launch_fwd<3, false>(a, m, ndir, s);
  else launch_fwd<4, false>(a, m, ndir, s);
}

void run_bwd(LstmBwdArgs a, const float* const* U, int ndir, const LstmGeom& m, float* ws, hipStream_t s) {
  for (int d = 0; d < ndir; ++d) {
    float* utp = ws + d * m.bwd_ws_floats;
    hipLaunchKernelGGL(lstm_pad_ut_kernel, dim3(stream_grid(m.bwd_ws_floats)), dim3(256), 0, s, U[d], utp, a.u, m.KP, m.SUT, 4);
    a.d[d].utp = utp;
  }
  if (m.bwd_u_lds) launch_bwd<1, true>(a, m, ndir, s);     // u <= 80: five tiles at the most, one a wave
  else if (m.NT == 1) launch_bwd<1, false>(a, m, ndir, s);
  else if (m.NT == 2) launch_bwd<2, false>(a, m, ndir, s);
  else if (m.NT == 3) launch_bwd<3, false>(a, m, ndir, s);
  else launch_bwd<4, false>(a, m, ndir, s);
}

// 0: launch, 1: nothing to do, GN_EINVAL: refused
int lstm_check(const char* what, int B, int T, int u, int act, int ract) {
  GN_REQUIRE(B >= 0 && T >= 1 && u >= 1, "%s: bad shape (B %d, T %d, u %d): B >= 0, T >= 1, u >= 1", what, B, T, u);
  GN_REQUIRE(u <= LSTM_MAX_U, "%s: u = %d, at most %d units run (a block carries all units of its samples on chip)", what, u, LSTM_MAX_U);
  GN_REQUIRE(lstm_code_ok(act, false), "%s: unknown activation code %d (GN_LSTM_TANH, _SIGMOID, _RELU, _LINEAR)", what, act);
  GN_REQUIRE(lstm_code_ok(ract, true), "%s: unknown recurrent activation code %d (GN_LSTM_HARD_SIGMOID, GN_LSTM_SIGMOID)", what, ract);
  GN_REQUIRE((unsigned long long)B * (unsigned long long)T < (1ull << 62) / (4ull * LSTM_MAX_U), "%s: B * T * 4u spans 2^62 elements or more", what);
  return B == 0 ? 1 : 0;
}

}  // namespace
}  // namespace gn

using namespace gn;

extern "C" {

size_t gn_lstm_fwd_workspace(int u) { return (u < 1 || u > LSTM_MAX_U) ? 0 : lstm_geom(u).fwd_ws_floats * sizeof(float); }

size_t gn_lstm_bwd_workspace(int u) { return (u < 1 || u > LSTM_MAX_U) ? 0 : lstm_geom(u).bwd_ws_floats * sizeof(float); }

int gn_lstm_fwd(const float* zx, const float* U, const float* bias, const float* h0, const float* c0, float* h, float* gates, float* c, float* hprev,
                void* ws, size_t ws_bytes, int B, int T, int u, int act, int ract, int reverse, int training, void* stream) {
  const int rc = lstm_check("lstm_fwd", B, T, u, act, ract);
  if (rc) return rc < 0 ? rc : GN_OK;
  GN_REQUIRE(zx && U && bias && h && ws, "lstm_fwd: null pointer (zx, U, bias, h and the workspace are required)");
  GN_REQUIRE(!training || (gates && c && hprev), "lstm_fwd: null pointer (the training phase stores gates, c and hprev)");
  const LstmGeom m = lstm_geom(u);
  if (ws_bytes < m.fwd_ws_floats * sizeof(float)) {
    set_error("lstm_fwd: workspace too small (%zu bytes, gn_lstm_fwd_workspace(%d) = %zu)", ws_bytes, u, m.fwd_ws_floats * sizeof(float));
    return GN_EWORKSPACE;
  }
  const LstmFwdDir d = {zx, nullptr, bias, h0, c0, h, gates, c, hprev};
  const LstmFwdArgs a = {{d, d}, B, T, u, m.KP, m.UP, m.SU, m.ntiles, act, ract, reverse != 0, training != 0, u, 1};
  run_fwd(a, &U, 1, m, (float*)ws, (hipStream_t)stream);
  return check_launch("lstm_fwd");
}

int gn_lstm_bwd(const float* dy, const float* gates, const float* c, const float* c0, const float* U, float* dz, float* dh0, float* dc0, void* ws,
                size_t ws_bytes, int B, int T, int u, int act, int ract, int reverse, int dy_seq, void* stream) {
  const int rc = lstm_check("lstm_bwd", B, T, u, act, ract);
  if (rc) return rc < 0 ? rc : GN_OK;
  GN_REQUIRE(dy && gates && c && U && dz && ws, "lstm_bwd: null pointer (dy, gates, c, U, dz and the workspace are required)");
  const LstmGeom m = lstm_geom(u);
  if (ws_bytes < m.bwd_ws_floats * sizeof(float)) {
    set_error("lstm_bwd: workspace too small (%zu bytes, gn_lstm_bwd_workspace(%d) = %zu)", ws_bytes, u, m.bwd_ws_floats * sizeof(float));
    return GN_EWORKSPACE;
  }
  const LstmBwdDir d = {dy, gates, c, c0, nullptr, dz, dh0, dc0};
  const LstmBwdArgs a = {{d, d}, B, T, u, m.KP, m.UP, m.SUT, m.ntiles, act, ract, reverse != 0, dy_seq != 0, u};
  run_bwd(a, &U, 1, m, (float*)ws, (hipStream_t)stream);
  return check_launch("lstm_bwd");
}

int gn_lstm_pair_fwd(const float* const* zx, const float* const* U, const float* const* bias, float* const* h, float* const* gates, float* const* c,
                     float* const* hprev, void* ws, size_t ws_bytes, int B, int T, int u, int ld, int act, int ract, int reverse0, int seq, int training,
                     void* stream) {
  const int rc = lstm_check("lstm_pair_fwd", B, T, u, act, ract);
  if (rc < 0) return rc;
  GN_REQUIRE(ld >= u, "lstm_pair_fwd: ld = %d, a row of h holds at least u = %d floats", ld, u);
  if (rc) return GN_OK;
  GN_REQUIRE(zx && U && bias && h && ws, "lstm_pair_fwd: null table (zx, U, bias, h and the workspace are required)");
  GN_REQUIRE(!training || (gates && c && hprev), "lstm_pair_fwd: null table (the training phase stores gates, c and hprev)");
  for (int d = 0; d < 2; ++d) {
    GN_REQUIRE(zx[d] && U[d] && bias[d] && h[d], "lstm_pair_fwd: null pointer in direction %d (zx, U, bias and h are required)", d);
    GN_REQUIRE(!training || (gates[d] && c[d] && hprev[d]), "lstm_pair_fwd: null pointer in direction %d (the training phase stores gates, c and hprev)", d);
  }
  const LstmGeom m = lstm_geom(u);
  if (ws_bytes < 2 * m.fwd_ws_floats * sizeof(float)) {
    set_error("lstm_pair_fwd: workspace too small (%zu bytes, 2 gn_lstm_fwd_workspace(%d) = %zu)", ws_bytes, u, 2 * m.fwd_ws_floats * sizeof(float));
    return GN_EWORKSPACE;
  }
  LstmFwdArgs a = {{}, B, T, u, m.KP, m.UP, m.SU, m.ntiles, act, ract, reverse0 != 0, training != 0, ld, seq != 0};
  for (int d = 0; d < 2; ++d)
    a.d[d] = {zx[d], nullptr, bias[d], nullptr, nullptr, h[d], training ? gates[d] : nullptr, training ? c[d] : nullptr, training ? hprev[d] : nullptr};
  run_fwd(a, U, 2, m, (float*)ws, (hipStream_t)stream);
  return check_launch("lstm_pair_fwd");
}

int gn_lstm_pair_bwd(const float* const* dy, const float* const* gates, const float* const* c, const float* const* U, float* const* dz, void* ws,
                     size_t ws_bytes, int B, int T, int u, int ld, int act, int ract, int reverse0, int dy_seq, void* stream) {
  const int rc = lstm_check("lstm_pair_bwd", B, T, u, act, ract);
  if (rc < 0) return rc;
  GN_REQUIRE(ld >= u, "lstm_pair_bwd: ld = %d, a row of dy holds at least u = %d floats", ld, u);
  if (rc) return GN_OK;
  GN_REQUIRE(dy && gates && c && U && dz && ws, "lstm_pair_bwd: null table (dy, gates, c, U, dz and the workspace are required)");
  for (int d = 0; d < 2; ++d)
    GN_REQUIRE(dy[d] && gates[d] && c[d] && U[d] && dz[d], "lstm_pair_bwd: null pointer in direction %d (dy, gates, c, U and dz are required)", d);
  const LstmGeom m = lstm_geom(u);
  if (ws_bytes < 2 * m.bwd_ws_floats * sizeof(float)) {
    set_error("lstm_pair_bwd: workspace too small (%zu bytes, 2 gn_lstm_bwd_workspace(%d) = %zu)", ws_bytes, u, 2 * m.bwd_ws_floats * sizeof(float));
    return GN_EWORKSPACE;
  }
  LstmBwdArgs a = {{}, B, T, u, m.KP, m.UP, m.SUT, m.ntiles, act, ract, reverse0 != 0, dy_seq != 0, ld};
  for (int d = 0; d < 2; ++d) a.d[d] = {dy[d], gates[d], c[d], nullptr, nullptr, dz[d], nullptr, nullptr};
  run_bwd(a, U, 2, m, (float*)ws, (hipStream_t)stream);
  return check_launch("lstm_pair_bwd");
}

}  // extern "C"
