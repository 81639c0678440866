// keras.layers.SimpleRNN (keras 2.2.4 layers/recurrent.py, SimpleRNNCell): the recurrence as one persistent kernel a direction; DESIGN 8s.
//
//   h_t = act((zx_t + b) + h_{t-1} . U)             zx = X . W for all steps comes in (one gn_bmm over B T rows); U is (u, u); h_0 = 0 or given
//
// OWNERSHIP and TILING are LSTM's and GRU's (csrc/lstm.hip, csrc/gru.hip): a block owns LSTM_ROWS = 16 batch rows and walks all T steps alone -- no
// block waits on another one, no grid barrier, no cooperative launch, no atomics; grid = ceil(B / 16) x directions.  The step product runs on
// v_mfma_f32_16x16x4_f32; a wave owns NT tiles of 16 units (tile = wave + nwaves i).  It is the scheme's limiting case: one gate block, so a
// step is ONE 16 x u by u x u product with one accumulator a tile, one activation and one barrier.
//   forward: h lies in LDS twice as the A operand, hs[row][k] with a row of SH = KP + 1 floats; a step reads one copy and writes the other.  h_t
// depends on h_{t-1} through the product alone, so no lane keeps h in registers between steps.
//   backward: t walks down; a lane holds dh of its (row, unit).  dz_t = (dy_t + dh) act'(h_t), the derivative through the output value, goes to
// dz (B, T, u) and to LDS, dzs[row][k] with a row of SD = KP + 1 floats; barrier; dh_{t-1} = dz_t . U^T, one chain over the KP rows of U^T.
// dzs lies in LDS twice as well: step t writes the copy the chain of step t + 1 does not read, so the backward also has one barrier a step (a
// wave that writes copy c again has passed the barrier between, which no wave passes before it has finished the chain that read c).
//
// U.  The entry points first write a zero-padded copy of U into the workspace (recurrent.h with G = 1): forward Up[k][j] with a row of
// SU = UP | 16 floats, backward the transpose Ut[k][j] with a row of SUT = UP | 16 floats.  rnn_geom() (rnn_geom.h) decides in ONE place which path
// a u takes: u <= 176: the padded matrix is copied into LDS once a block, forward and backward (up to 11 tiles: two a wave above 128 units);
// 177 <= u <= 512: it streams from L2.
//
// NUMERICS.  The recurrent pre-activation is ONE fp32 fma chain over k = 0 .. u-1 from +0, then + (zx + b).  dh_{t-1} is one chain over k.  Row m
// of an MFMA result depends on row m of A alone, so a sample's results do not depend on B, on its tile or on the launch; rows of a tile beyond B
// run on zeros and are never stored.
//
// STORED for the backward (training flag), at the INPUT time index of the step: hs (B, T, u) = h_t, which act' reads (a tensor of its own: the
// layer's output is in processing order and may be the last step alone); hprev (B, T, u), the h that entered the step, the left operand of dU.
//
// A PAIR OF DIRECTIONS (keras Bidirectional): as in csrc/lstm.hip.  blockIdx.y is the direction d and picks its operands from the
// two-entry table of the arguments; direction 1 walks the other way and writes step s at position T-1-s; h and dy go through a row stride ld.
// gn_rnn_fwd / gn_rnn_bwd launch one direction with ld = u; gn_rnn_pair_fwd / _bwd launch two.
#include <math.h>

#include "common.h"
#include "recurrent.h"
#include "rnn_geom.h"

namespace gn {
namespace {

struct RnnFwdDir {
  const float* zx;      // (B, T, u)
  const float* up;      // padded U: KP rows of SU floats
  const float* bias;    // (u)
  const float* h0;      // (B, u) or NULL
  float* h;             // seq: (B, T, ld) rows of which the direction owns u columns; else (B, ld), the last processed step
  float* hs;            // (B, T, u), input time order; training only
  float* hprev;         // (B, T, u)
};

// blockIdx.y is the direction: 0 walks with `reverse` and writes step s at position s, 1 walks with !reverse and writes it at position T-1-s
struct RnnFwdArgs {
  RnnFwdDir d[2];
  int B, T, u, KP, SU, ntiles, act, reverse, training, ld, seq;
};

// A (16 rows of LDS, k in [0, KP)) . B (KP rows of S floats, 16 columns) as one chain from +0: two k groups of 4 a turn, loads first
__device__ __forceinline__ f32x4 rnn_chain(const float* ap, const float* bp, int KP, int S) {
  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < KP; k0 += 8) {                               // KP is a multiple of 8
    float a[2], b[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      a[kk] = ap[k0 + 4 * kk];
      b[kk] = bp[(size_t)(k0 + 4 * kk) * S];
    }
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[kk], b[kk], acc, 0, 0, 0);
  }
  return acc;
}

template <int NT, bool ULDS>
__global__ __launch_bounds__(64 * LSTM_MAX_WAVES) void rnn_fwd_kernel(RnnFwdArgs g) {
  const bool second = blockIdx.y != 0;
  const RnnFwdDir p = second ? g.d[1] : g.d[0];
  const bool reverse = second ? !g.reverse : (g.reverse != 0);
  const size_t h_row = g.seq ? (size_t)g.T * g.ld : (size_t)g.ld;              // floats between two samples of h
  extern __shared__ __attribute__((aligned(16))) float rnn_lds[];
  const int SH = g.KP + 1;
  float* hs0 = rnn_lds;
  float* hs1 = rnn_lds + LSTM_ROWS * SH;
  float* us = rnn_lds + 2 * LSTM_ROWS * SH;
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

  size_t ro[4];                                   // (row T) u of the lane's four rows: an element of step t is ro + t u + j
#pragma unroll
  for (int r = 0; r < 4; ++r) ro[r] = (b0 + 4 * fq + r) * T * u;
  float bias[NT];
  const size_t t_first = reverse ? T - 1 : 0;
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    const int tile = wave + nw * i, j = tile * LSTM_TILE + fc;
    const bool jok = tile < g.ntiles && j < g.u;
    bias[i] = jok ? p.bias[j] : 0.f;
    if (jok && g.training) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const size_t row = b0 + 4 * fq + r;
        if (row < (size_t)g.B) p.hprev[ro[r] + t_first * u + j] = p.h0 ? p.h0[row * u + j] : 0.f;
      }
    }
  }
  __syncthreads();

  for (int s = 0; s < g.T; ++s) {
    const size_t t_in = reverse ? T - 1 - s : (size_t)s;
    const size_t e_in = t_in * u;                                   // the step's elements at the input time
    const size_t e_next = reverse ? e_in - u : e_in + u;            // used only while s + 1 < T
    const bool h_out = g.seq || s == g.T - 1;
    const size_t h_pos = g.seq ? (size_t)(second ? g.T - 1 - s : s) * g.ld : 0;
    // the lane's row and column guards are formed anew every step from two registers the compiler cannot see through, as in csrc/gru.hip:
    // hoisted out of the loop each guard would sit in a scalar register pair for the whole sequence
    int lrow = 4 * fq, lcol = fc;
    asm volatile("" : "+v"(lrow), "+v"(lcol));
    bool rok[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) rok[r] = b0 + lrow + r < (size_t)g.B;
    const float* cur = (s & 1) ? hs1 : hs0;
    float* nxt = (s & 1) ? hs0 : hs1;
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      const int tile = wave + nw * i;
      if (tile < g.ntiles) {                                          // the same for all lanes of a wave
        const int j = tile * LSTM_TILE + lcol;
        const bool jok = j < g.u;
        float zv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) zv[r] = (jok && rok[r]) ? p.zx[ro[r] + e_in + j] : 0.f;
        const f32x4 acc = rnn_chain(cur + fc * SH + fq, ub + fq * g.SU + j, g.KP, g.SU);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float hn = lstm_act(acc[r] + (zv[r] + bias[i]), g.act);
          if (jok) {
            nxt[(4 * fq + r) * SH + j] = hn;
            if (rok[r]) {
              if (h_out) p.h[(b0 + lrow + r) * h_row + h_pos + j] = hn;
              if (g.training) {
                p.hs[ro[r] + e_in + j] = hn;
                if (s + 1 < g.T) p.hprev[ro[r] + e_next + j] = hn;
              }
            }
          }
        }
      }
    }
    __syncthreads();          // h_t is complete in nxt, and every wave has left cur, which step t + 1 overwrites
  }
}

struct RnnBwdDir {
  const float* dy;      // dy_seq: (B, T, ld) rows at the positions the forward wrote; else (B, ld) for the last step
  const float* hs;      // (B, T, u): h_t as stored
  const float* utp;     // padded U^T: KP rows of SUT floats
  float* dz;            // (B, T, u), input time order
  float* dh0;           // (B, u) or NULL
};

// blockIdx.y is the direction, as in the forward
struct RnnBwdArgs {
  RnnBwdDir d[2];
  int B, T, u, KP, SUT, ntiles, act, reverse, dy_seq, ld;
};

template <int NT, bool ULDS>
__global__ __launch_bounds__(64 * LSTM_MAX_WAVES) void rnn_bwd_kernel(RnnBwdArgs g) {
  const bool second = blockIdx.y != 0;
  const RnnBwdDir p = second ? g.d[1] : g.d[0];
  const bool reverse = second ? !g.reverse : (g.reverse != 0);
  const size_t dy_row = g.dy_seq ? (size_t)g.T * g.ld : (size_t)g.ld;          // floats between two samples of dy
  extern __shared__ __attribute__((aligned(16))) float rnn_lds[];
  const int SD = g.KP + 1;
  float* dzs0 = rnn_lds;
  float* dzs1 = rnn_lds + LSTM_ROWS * SD;
  float* us = rnn_lds + 2 * LSTM_ROWS * SD;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int fc = lane & 15, fq = lane >> 4;
  const size_t b0 = (size_t)blockIdx.x * LSTM_ROWS;
  const size_t u = (size_t)g.u, T = (size_t)g.T;

  for (int e = threadIdx.x; e < 2 * LSTM_ROWS * SD; e += blockDim.x) dzs0[e] = 0.f;       // both copies
  if (ULDS)
    for (int e = threadIdx.x; e < g.KP * g.SUT; e += blockDim.x) us[e] = p.utp[e];
  const float* __restrict__ ub = ULDS ? (const float*)us : p.utp;

  size_t ro[4];                                   // (row T) u of the lane's four rows, as in the forward
  bool rok[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const size_t row = b0 + 4 * fq + r;
    rok[r] = row < (size_t)g.B;
    ro[r] = row * T * u;
  }
  float dh[NT][4];
#pragma unroll
  for (int i = 0; i < NT; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) dh[i][r] = 0.f;
  __syncthreads();

  for (int s = g.T - 1; s >= 0; --s) {
    const size_t t_in = reverse ? T - 1 - s : (size_t)s;
    const size_t e_in = t_in * u;                                   // the step's elements at the input time
    const bool dy_in = g.dy_seq || s == g.T - 1;
    const size_t dy_pos = g.dy_seq ? (size_t)(second ? g.T - 1 - s : s) * g.ld : 0;
    float* dzs = (s & 1) ? dzs1 : dzs0;
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      const int tile = wave + nw * i, j = tile * LSTM_TILE + fc;
      if (tile < g.ntiles && j < g.u) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if (rok[r]) {                                             // rows beyond B keep their +0 in dzs, and a dh of +0
            const float hv = p.hs[ro[r] + e_in + j];
            const float dyv = dy_in ? p.dy[(b0 + 4 * fq + r) * dy_row + dy_pos + j] : 0.f;
            const float dzv = (dyv + dh[i][r]) * lstm_act_grad(hv, g.act);
            p.dz[ro[r] + e_in + j] = dzv;
            dzs[(4 * fq + r) * SD + j] = dzv;
          }
        }
      }
    }
    __syncthreads();          // dz_t is complete in dzs, and every wave has left the other copy, which step t - 1 overwrites
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      const int tile = wave + nw * i;
      if (tile < g.ntiles) {
        const f32x4 acc = rnn_chain(dzs + fc * SD + fq, ub + fq * g.SUT + tile * LSTM_TILE + fc, g.KP, g.SUT);
#pragma unroll
        for (int r = 0; r < 4; ++r) dh[i][r] = acc[r];
      }
    }
  }

  if (p.dh0) {
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      const int tile = wave + nw * i, j = tile * LSTM_TILE + fc;
      if (tile < g.ntiles && j < g.u) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if (rok[r]) p.dh0[(b0 + 4 * fq + r) * u + j] = dh[i][r];
        }
      }
    }
  }
}

template <int NT, bool ULDS>
void launch_fwd(const RnnFwdArgs& a, const RnnGeom& m, int ndir, hipStream_t s) {
  static unsigned long long big = 0;
  allow_big_lds((const void*)rnn_fwd_kernel<NT, ULDS>, &big);
  hipLaunchKernelGGL((rnn_fwd_kernel<NT, ULDS>), dim3(cdiv(a.B, LSTM_ROWS), ndir), dim3(64 * m.nwaves), m.fwd_lds_bytes, s, a);
}

template <int NT, bool ULDS>
void launch_bwd(const RnnBwdArgs& a, const RnnGeom& m, int ndir, hipStream_t s) {
  static unsigned long long big = 0;
  allow_big_lds((const void*)rnn_bwd_kernel<NT, ULDS>, &big);
  hipLaunchKernelGGL((rnn_bwd_kernel<NT, ULDS>), dim3(cdiv(a.B, LSTM_ROWS), ndir), dim3(64 * m.nwaves), m.bwd_lds_bytes, s, a);
}

void pick_fwd(const RnnFwdArgs& a, const RnnGeom& m, int ndir, hipStream_t s) {
  if (m.fwd_u_lds && m.NT == 1) launch_fwd<1, true>(a, m, ndir, s);
  else if (m.fwd_u_lds) launch_fwd<2, true>(a, m, ndir, s);         // 129 <= u <= 176: nine to eleven tiles
  else if (m.NT == 2) launch_fwd<2, false>(a, m, ndir, s);          // a streamed u has at least twelve tiles
  else if (m.NT == 3) launch_fwd<3, false>(a, m, ndir, s);
  else launch_fwd<4, false>(a, m, ndir, s);
}

void pick_bwd(const RnnBwdArgs& a, const RnnGeom& m, int ndir, hipStream_t s) {
  if (m.bwd_u_lds && m.NT == 1) launch_bwd<1, true>(a, m, ndir, s);
  else if (m.bwd_u_lds) launch_bwd<2, true>(a, m, ndir, s);
  else if (m.NT == 2) launch_bwd<2, false>(a, m, ndir, s);
  else if (m.NT == 3) launch_bwd<3, false>(a, m, ndir, s);
  else launch_bwd<4, false>(a, m, ndir, s);
}

// pads the U of the ndir directions into the workspace, one copy after the other, and launches the ndir directions as ONE grid
void run_fwd(RnnFwdArgs a, const float* const* U, int ndir, const RnnGeom& m, float* ws, hipStream_t s) {
  for (int d = 0; d < ndir; ++d) {
    float* up = ws + d * m.fwd_ws_floats;
    hipLaunchKernelGGL(lstm_pad_u_kernel, dim3(stream_grid(m.fwd_ws_floats)), dim3(256), 0, s, U[d], up, a.u, m.KP, m.UP, m.SU, RNN_GATES);
    a.d[d].up = up;
  }
  pick_fwd(a, m, ndir, s);
}

void run_bwd(RnnBwdArgs a, const float* const* U, int ndir, const RnnGeom& m, float* ws, hipStream_t s) {
  for (int d = 0; d < ndir; ++d) {
    float* utp = ws + d * m.bwd_ws_floats;
    hipLaunchKernelGGL(lstm_pad_ut_kernel, dim3(stream_grid(m.bwd_ws_floats)), dim3(256), 0, s, U[d], utp, a.u, m.KP, m.SUT, RNN_GATES);
    a.d[d].utp = utp;
  }
  pick_bwd(a, m, ndir, s);
}

// 0: launch, 1: nothing to do, GN_EINVAL: refused
int rnn_check(const char* what, int B, int T, int u, int act) {
  GN_REQUIRE(B >= 0 && T >= 1 && u >= 1, "%s: bad shape (B %d, T %d, u %d): B >= 0, T >= 1, u >= 1", what, B, T, u);
  GN_REQUIRE(u <= LSTM_MAX_U, "%s: u = %d, at most %d units run (a block carries all units of its samples on chip)", what, u, LSTM_MAX_U);
  GN_REQUIRE(lstm_code_ok(act, false), "%s: unknown activation code %d (GN_LSTM_TANH, _SIGMOID, _RELU, _LINEAR)", what, act);
  GN_REQUIRE((unsigned long long)B * (unsigned long long)T < (1ull << 62) / (unsigned long long)LSTM_MAX_U, "%s: B * T * u spans 2^62 elements or more", what);
  return B == 0 ? 1 : 0;
}

}  // namespace
}  // namespace gn

using namespace gn;

extern "C" {

size_t gn_rnn_fwd_workspace(int u) { return (u < 1 || u > LSTM_MAX_U) ? 0 : rnn_geom(u).fwd_ws_floats * sizeof(float); }

size_t gn_rnn_bwd_workspace(int u) { return (u < 1 || u > LSTM_MAX_U) ? 0 : rnn_geom(u).bwd_ws_floats * sizeof(float); }

int gn_rnn_fwd(const float* zx, const float* U, const float* bias, const float* h0, float* h, float* hs, float* hprev, void* ws, size_t ws_bytes, int B,
               int T, int u, int act, int reverse, int training, void* stream) {
  const int rc = rnn_check("rnn_fwd", B, T, u, act);
  if (rc) return rc < 0 ? rc : GN_OK;
  GN_REQUIRE(zx && U && bias && h && ws, "rnn_fwd: null pointer (zx, U, bias, h and the workspace are required)");
  GN_REQUIRE(!training || (hs && hprev), "rnn_fwd: null pointer (the training phase stores hs and hprev)");
  const RnnGeom m = rnn_geom(u);
  if (ws_bytes < m.fwd_ws_floats * sizeof(float)) {
    set_error("rnn_fwd: workspace too small (%zu bytes, gn_rnn_fwd_workspace(%d) = %zu)", ws_bytes, u, m.fwd_ws_floats * sizeof(float));
    return GN_EWORKSPACE;
  }
  const RnnFwdDir d = {zx, nullptr, bias, h0, h, hs, hprev};
  const RnnFwdArgs a = {{d, d}, B, T, u, m.KP, m.SU, m.ntiles, act, reverse != 0, training != 0, u, 1};
  run_fwd(a, &U, 1, m, (float*)ws, (hipStream_t)stream);
  return check_launch("rnn_fwd");
}

int gn_rnn_bwd(const float* dy, const float* hs, const float* U, float* dz, float* dh0, void* ws, size_t ws_bytes, int B, int T, int u, int act,
               int reverse, int dy_seq, void* stream) {
  const int rc = rnn_check("rnn_bwd", B, T, u, act);
  if (rc) return rc < 0 ? rc : GN_OK;
  GN_REQUIRE(dy && hs && U && dz && ws, "rnn_bwd: null pointer (dy, hs, U, dz and the workspace are required)");
  const RnnGeom m = rnn_geom(u);
  if (ws_bytes < m.bwd_ws_floats * sizeof(float)) {
    set_error("rnn_bwd: workspace too small (%zu bytes, gn_rnn_bwd_workspace(%d) = %zu)", ws_bytes, u, m.bwd_ws_floats * sizeof(float));
    return GN_EWORKSPACE;
  }
  const RnnBwdDir d = {dy, hs, nullptr, dz, dh0};
  const RnnBwdArgs a = {{d, d}, B, T, u, m.KP, m.SUT, m.ntiles, act, reverse != 0, dy_seq != 0, u};
  run_bwd(a, &U, 1, m, (float*)ws, (hipStream_t)stream);
  return check_launch("rnn_bwd");
}

int gn_rnn_pair_fwd(const float* const* zx, const float* const* U, const float* const* bias, float* const* h, float* const* hs, float* const* hprev,
                    void* ws, size_t ws_bytes, int B, int T, int u, int ld, int act, int reverse0, int seq, int training, void* stream) {
  const int rc = rnn_check("rnn_pair_fwd", B, T, u, act);
  if (rc < 0) return rc;
  GN_REQUIRE(ld >= u, "rnn_pair_fwd: ld = %d, a row of h holds at least u = %d floats", ld, u);
  if (rc) return GN_OK;
  GN_REQUIRE(zx && U && bias && h && ws, "rnn_pair_fwd: null table (zx, U, bias, h and the workspace are required)");
  GN_REQUIRE(!training || (hs && hprev), "rnn_pair_fwd: null table (the training phase stores hs and hprev)");
  for (int d = 0; d < 2; ++d) {
    GN_REQUIRE(zx[d] && U[d] && bias[d] && h[d], "rnn_pair_fwd: null pointer in direction %d (zx, U, bias and h are required)", d);
    GN_REQUIRE(!training || (hs[d] && hprev[d]), "rnn_pair_fwd: null pointer in direction %d (the training phase stores hs and hprev)", d);
  }
  const RnnGeom m = rnn_geom(u);
  if (ws_bytes < 2 * m.fwd_ws_floats * sizeof(float)) {
    set_error("rnn_pair_fwd: workspace too small (%zu bytes, 2 gn_rnn_fwd_workspace(%d) = %zu)", ws_bytes, u, 2 * m.fwd_ws_floats * sizeof(float));
    return GN_EWORKSPACE;
  }
  RnnFwdArgs a = {{}, B, T, u, m.KP, m.SU, m.ntiles, act, reverse0 != 0, training != 0, ld, seq != 0};
  for (int d = 0; d < 2; ++d) a.d[d] = {zx[d], nullptr, bias[d], nullptr, h[d], training ? hs[d] : nullptr, training ? hprev[d] : nullptr};
  run_fwd(a, U, 2, m, (float*)ws, (hipStream_t)stream);
  return check_launch("rnn_pair_fwd");
}

int gn_rnn_pair_bwd(const float* const* dy, const float* const* hs, const float* const* U, float* const* dz, void* ws, size_t ws_bytes, int B, int T,
                    int u, int ld, int act, int reverse0, int dy_seq, void* stream) {
  const int rc = rnn_check("rnn_pair_bwd", B, T, u, act);
  if (rc < 0) return rc;
  GN_REQUIRE(ld >= u, "rnn_pair_bwd: ld = %d, a row of dy holds at least u = %d floats", ld, u);
  if (rc) return GN_OK;
  GN_REQUIRE(dy && hs && U && dz && ws, "rnn_pair_bwd: null table (dy, hs, U, dz and the workspace are required)");
  for (int d = 0; d < 2; ++d)
    GN_REQUIRE(dy[d] && hs[d] && U[d] && dz[d], "rnn_pair_bwd: null pointer in direction %d (dy, hs, U and dz are required)", d);
  const RnnGeom m = rnn_geom(u);
  if (ws_bytes < 2 * m.bwd_ws_floats * sizeof(float)) {
    set_error("rnn_pair_bwd: workspace too small (%zu bytes, 2 gn_rnn_bwd_workspace(%d) = %zu)", ws_bytes, u, 2 * m.bwd_ws_floats * sizeof(float));
    return GN_EWORKSPACE;
  }
  RnnBwdArgs a = {{}, B, T, u, m.KP, m.SUT, m.ntiles, act, reverse0 != 0, dy_seq != 0, ld};
  for (int d = 0; d < 2; ++d) a.d[d] = {dy[d], hs[d], nullptr, dz[d], nullptr};
  run_bwd(a, U, 2, m, (float*)ws, (hipStream_t)stream);
  return check_launch("rnn_pair_bwd");
}

}  // extern "C"
