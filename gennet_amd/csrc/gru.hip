// keras.layers.GRU (keras 2.2.4 layers/recurrent.py, GRUCell), both reset_after forms: the recurrence as one persistent kernel a direction; DESIGN 8p.
//
//   a_t = zx_t + b                                  zx = X . W for all steps comes in (one gn_bmm over B T rows), gate columns z, r, h of width u
//   reset_after = 0:  m = h_{t-1} . U[:, :2u]        z = ra(a_z + m_z)   r = ra(a_r + m_r)      hh = act(a_h + (r h_{t-1}) . U_h)
//   reset_after = 1:  m = h_{t-1} . U + rb           z = ra(a_z + m_z)   r = ra(a_r + m_r)      q = m_h     hh = act(a_h + r q)
//   h_t = z h_{t-1} + (1 - z) hh
//
// OWNERSHIP and TILING are LSTM's (csrc/lstm.hip): a block owns LSTM_ROWS = 16 batch rows and walks all T steps alone -- no block waits on another
// one, no grid barrier, no cooperative launch, no atomics; grid = ceil(B / 16).  The step products run on v_mfma_f32_16x16x4_f32; a wave owns NT
// tiles of 16 units (tile = wave + nwaves i) and a lane holds z, r, the candidate and h_{t-1} of the same (row, unit): h lives in registers for
// the whole sequence (4 NT a lane), and in LDS as the A operand, hs[row][k] with a row of SH = KP + 1 floats.
//   forward, reset_after = 1: ONE product with three accumulators; h lies in LDS twice, a step reads one copy and writes the other: one barrier a
// step.
//   forward, reset_after = 0: TWO dependent products.  Product 1 over U[:, :2u] gives z and r; r h_{t-1} goes to the second LDS row buffer; barrier;
// product 2 over U_h reads that buffer and gives hh and h_t, which overwrites the FIRST buffer (every wave left it at the barrier); barrier.  So
// both forms keep two row buffers.
//   backward: t walks down; a lane holds dh of its (row, unit).  The step's gradients lie in LDS as dzs[row][gate KP + k], a row of SD = 3 KP + 1.
// reset_after = 1: the lane forms dz = [da_z, da_r, da_h] and dzr = [da_z, da_r, dq], dzr goes to LDS; barrier; dh_{t-1} = dhv z + dzr . U^T, one
// chain over the 3 KP rows of U^T; barrier.   reset_after = 0: da_h goes to the h block of dzs; barrier; d(rh) = da_h . U_h^T, a KP chain;
// da_r = d(rh) h_{t-1} ra'(r); [da_z, da_r] go to the z and r blocks; barrier; dh_{t-1} = (dhv z + d(rh) r) + [da_z, da_r] . U[:, :2u]^T, a 2 KP
// chain.  No third barrier: the next step's first phase writes the h block alone, which the 2 KP chain does not read, and its second phase,
// which writes the z and r blocks, lies behind that step's first barrier, which no wave passes before every wave has finished the chain.
//
// U.  The entry points first write a zero-padded copy of U into the workspace (recurrent.h): forward Up[k][gate UP + j] with a row of SU = 3 UP | 16
// floats, backward the transpose Ut[gate KP + k][j] with a row of SUT = UP | 16 floats.  gru_geom() (gru_geom.h) decides in ONE place which path
// a u takes: u <= 104: the padded matrix is copied into LDS once a block, forward and backward; 105 <= u <= 512: it streams from L2.
//
// NUMERICS.  Every recurrent pre-activation is ONE fp32 fma chain over k = 0 .. u-1 from +0, then + rb where there is one, then + (zx + b).  The
// candidate of reset_after = 1 is act((zx_h + b_h) + r q), q = chain + rb_h.  h_t = z h + (1 - z) hh with every product and sum rounded on its own.
// dh_{t-1}: one chain over the gate columns in k order added to dhv z (+ d(rh) r).  Row m of an MFMA result depends on row m of A alone, so a
// sample's results do not depend on B, on its tile or on the launch; rows of a tile beyond B run on zeros and are never stored.
//
// STORED for the backward (training flag), at the INPUT time index of the step: gates (B, T, 3u) = z, r, hh; hprev (B, T, u), the h that entered
// the step; aux (B, T, u) = r h_{t-1} (reset_after = 0: the left operand of dU's h block) or q (reset_after = 1).
//
// A PAIR OF DIRECTIONS (keras Bidirectional): as in csrc/lstm.hip.  blockIdx.y is the direction d and picks its operands from the
// two-entry table of the arguments; direction 1 walks the other way and writes step s at position T-1-s; h and dy go through a row stride ld.
// gn_gru_fwd / gn_gru_bwd launch one direction with ld = u; gn_gru_pair_fwd / _bwd launch two.
#include <math.h>

#include "common.h"
#include "gru_geom.h"
#include "recurrent.h"

namespace gn {
namespace {

struct GruFwdDir {
  const float* zx;      // (B, T, 3u)
  const float* up;      // padded U: KP rows of SU floats
  const float* bias;    // (3u)
  const float* rbias;   // (3u), reset_after only
  const float* h0;      // (B, u) or NULL
  float* h;             // seq: (B, T, ld) rows of which the direction owns u columns; else (B, ld), the last processed step
  float* gates;         // (B, T, 3u), input time order; training only
  float* hprev;         // (B, T, u)
  float* aux;           // (B, T, u)
};

// blockIdx.y is the direction: 0 walks with `reverse` and writes step s at position s, 1 walks with !reverse and writes it at position T-1-s
struct GruFwdArgs {
  GruFwdDir d[2];
  int B, T, u, KP, UP, SU, ntiles, act, ract, reverse, training, ld, seq;
};

// acc[q] += A (16 rows of LDS, k in [0, KP)) . B (gate block q of NQ consecutive ones, 16 columns): two k groups of 4 a turn, loads first
template <int NQ>
__device__ __forceinline__ void gru_fwd_chain(f32x4 (&acc)[NQ], const float* ap, const float* bp, int KP, int SU, int UP) {
  for (int k0 = 0; k0 < KP; k0 += 8) {                               // KP is a multiple of 8
    const float* bk = bp + (size_t)k0 * SU;
    float a[2], b[2][NQ];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      a[kk] = ap[k0 + 4 * kk];
#pragma unroll
      for (int q = 0; q < NQ; ++q) b[kk][q] = bk[(size_t)4 * kk * SU + q * UP];
    }
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int q = 0; q < NQ; ++q) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[kk], b[kk][q], acc[q], 0, 0, 0);
  }
}

template <int NT, bool ULDS, bool RA>
__global__ __launch_bounds__(64 * LSTM_MAX_WAVES) void gru_fwd_kernel(GruFwdArgs g) {
  const bool second = blockIdx.y != 0;
  const GruFwdDir p = second ? g.d[1] : g.d[0];
  const bool reverse = second ? !g.reverse : (g.reverse != 0);
  const size_t h_row = g.seq ? (size_t)g.T * g.ld : (size_t)g.ld;              // floats between two samples of h
  extern __shared__ __attribute__((aligned(16))) float gru_lds[];
  const int SH = g.KP + 1;
  float* hs0 = gru_lds;
  float* hs1 = gru_lds + LSTM_ROWS * SH;          // RA: the second copy of h;  !RA: r h_{t-1}
  float* us = gru_lds + 2 * LSTM_ROWS * SH;
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
  float hreg[NT][4], bias[NT][3], rb[NT][3];
  const size_t t_first = reverse ? T - 1 : 0;
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    const int tile = wave + nw * i, j = tile * LSTM_TILE + fc;
    const bool jok = tile < g.ntiles && j < g.u;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      bias[i][q] = jok ? p.bias[q * g.u + j] : 0.f;
      rb[i][q] = (RA && jok) ? p.rbias[q * g.u + j] : 0.f;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool ok = jok && b0 + 4 * fq + r < (size_t)g.B;
      hreg[i][r] = (ok && p.h0) ? p.h0[(b0 + 4 * fq + r) * u + j] : 0.f;
      if (ok && g.training) p.hprev[ro[r] + t_first * u + j] = hreg[i][r];
    }
  }
  __syncthreads();

  for (int s = 0; s < g.T; ++s) {
    const size_t t_in = reverse ? T - 1 - s : (size_t)s;
    const size_t e_in = t_in * u;                                   // the step's elements at the input time
    const size_t e_next = reverse ? e_in - u : e_in + u;            // used only while s + 1 < T
    const bool h_out = g.seq || s == g.T - 1;
    const size_t h_pos = g.seq ? (size_t)(second ? g.T - 1 - s : s) * g.ld : 0;
    // The lane's row and column guards are formed anew every step from two registers the compiler cannot see through: hoisted out of the loop
    // each of the 5 NT guards would sit in a scalar register pair for the whole sequence, and the four-tile forms would spill scalar registers.
    int lrow = 4 * fq, lcol = fc;
    asm volatile("" : "+v"(lrow), "+v"(lcol));
    bool rok[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) rok[r] = b0 + lrow + r < (size_t)g.B;
    if (RA) {
      const float* cur = (s & 1) ? hs1 : hs0;
      float* nxt = (s & 1) ? hs0 : hs1;
#pragma unroll
      for (int i = 0; i < NT; ++i) {
        const int tile = wave + nw * i;
        if (tile < g.ntiles) {                                        // the same for all lanes of a wave
          const int j = tile * LSTM_TILE + lcol;
          const bool jok = j < g.u;
          float zv[3][4];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const bool ok = jok && rok[r];
#pragma unroll
            for (int q = 0; q < 3; ++q) zv[q][r] = ok ? p.zx[(ro[r] + e_in) * 3 + q * u + j] : 0.f;
          }
          f32x4 acc[3];
#pragma unroll
          for (int q = 0; q < 3; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
          gru_fwd_chain<3>(acc, cur + fc * SH + fq, ub + fq * g.SU + j, g.KP, g.SU, g.UP);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float hp = hreg[i][r];
            const float gz = lstm_act((acc[0][r] + rb[i][0]) + (zv[0][r] + bias[i][0]), g.ract);
            const float gr = lstm_act((acc[1][r] + rb[i][1]) + (zv[1][r] + bias[i][1]), g.ract);
            const float qv = acc[2][r] + rb[i][2];
            const float hh = lstm_act((zv[2][r] + bias[i][2]) + gr * qv, g.act);
            const float hn = gz * hp + (1.f - gz) * hh;
            hreg[i][r] = hn;
            if (jok) {
              nxt[(4 * fq + r) * SH + j] = hn;
              if (rok[r]) {
                if (h_out) p.h[(b0 + lrow + r) * h_row + h_pos + j] = hn;
                if (g.training) {
                  float* gp = p.gates + (ro[r] + e_in) * 3 + j;
                  gp[0] = gz;
                  gp[u] = gr;
                  gp[2 * u] = hh;
                  p.aux[ro[r] + e_in + j] = qv;
                  if (s + 1 < g.T) p.hprev[ro[r] + e_next + j] = hn;
                }
              }
            }
          }
        }
      }
      __syncthreads();        // h_t is complete in nxt, and every wave has left cur, which step t + 1 overwrites
    } else {
      float zreg[NT][4], ah[NT][4];
#pragma unroll
      for (int i = 0; i < NT; ++i) {
        const int tile = wave + nw * i;
        if (tile < g.ntiles) {
          const int j = tile * LSTM_TILE + lcol;
          const bool jok = j < g.u;
          float zv[2][4];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const bool ok = jok && rok[r];
#pragma unroll
            for (int q = 0; q < 2; ++q) zv[q][r] = ok ? p.zx[(ro[r] + e_in) * 3 + q * u + j] : 0.f;
            ah[i][r] = (ok ? p.zx[(ro[r] + e_in) * 3 + 2 * u + j] : 0.f) + bias[i][2];          // wanted behind the barrier
          }
          f32x4 acc[2];
#pragma unroll
          for (int q = 0; q < 2; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
          gru_fwd_chain<2>(acc, hs0 + fc * SH + fq, ub + fq * g.SU + j, g.KP, g.SU, g.UP);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float gz = lstm_act(acc[0][r] + (zv[0][r] + bias[i][0]), g.ract);
            const float gr = lstm_act(acc[1][r] + (zv[1][r] + bias[i][1]), g.ract);
            const float rh = gr * hreg[i][r];
            zreg[i][r] = gz;
            if (jok) {
              hs1[(4 * fq + r) * SH + j] = rh;
              if (rok[r] && g.training) {
                float* gp = p.gates + (ro[r] + e_in) * 3 + j;
                gp[0] = gz;
                gp[u] = gr;
                p.aux[ro[r] + e_in + j] = rh;
              }
            }
          }
        }
      }
      __syncthreads();        // r h_{t-1} is complete in hs1, and every wave has left hs0, which the second phase overwrites
#pragma unroll
      for (int i = 0; i < NT; ++i) {
        const int tile = wave + nw * i;
        if (tile < g.ntiles) {
          const int j = tile * LSTM_TILE + lcol;
          const bool jok = j < g.u;
          f32x4 acc[1];
          acc[0] = f32x4{0.f, 0.f, 0.f, 0.f};
          gru_fwd_chain<1>(acc, hs1 + fc * SH + fq, ub + fq * g.SU + 2 * g.UP + j, g.KP, g.SU, g.UP);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float gz = zreg[i][r];
            const float hh = lstm_act(acc[0][r] + ah[i][r], g.act);
            const float hn = gz * hreg[i][r] + (1.f - gz) * hh;
            hreg[i][r] = hn;
            if (jok) {
              hs0[(4 * fq + r) * SH + j] = hn;
              if (rok[r]) {
                if (h_out) p.h[(b0 + lrow + r) * h_row + h_pos + j] = hn;
                if (g.training) {
                  p.gates[(ro[r] + e_in) * 3 + 2 * u + j] = hh;
                  if (s + 1 < g.T) p.hprev[ro[r] + e_next + j] = hn;
                }
              }
            }
          }
        }
      }
      __syncthreads();        // h_t is complete in hs0, and every wave has left hs1, which step t + 1 overwrites
    }
  }
}

struct GruBwdDir {
  const float* dy;      // dy_seq: (B, T, ld) rows at the positions the forward wrote; else (B, ld) for the last step
  const float* gates;
  const float* hprev;
  const float* aux;     // q, read under reset_after only
  const float* utp;     // padded U^T: 3 KP rows of SUT floats
  float* dz;            // (B, T, 3u), input time order: da_z, da_r, da_h
  float* dzr;           // (B, T, 3u): da_z, da_r, dq; reset_after only
  float* dh0;           // (B, u) or NULL
};

// blockIdx.y is the direction, as in the forward
struct GruBwdArgs {
  GruBwdDir d[2];
  int B, T, u, KP, UP, SUT, ntiles, act, ract, reverse, dy_seq, ld;
};

// A (16 rows of LDS, columns [kbeg, kend)) . U^T (rows [kbeg, kend), 16 columns) as one chain from +0: G k groups of 4 a turn, loads first
template <int G>
__device__ __forceinline__ f32x4 gru_bwd_chain(const float* ap, const float* bp, int SUT, int kbeg, int kend) {
  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = kbeg; k0 < kend; k0 += 4 * G) {                      // kend - kbeg is a multiple of 4 G
    float a[G], b[G];
#pragma unroll
    for (int kk = 0; kk < G; ++kk) {
      a[kk] = ap[k0 + 4 * kk];
      b[kk] = bp[(size_t)(k0 + 4 * kk) * SUT];
    }
#pragma unroll
    for (int kk = 0; kk < G; ++kk) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[kk], b[kk], acc, 0, 0, 0);
  }
  return acc;
}

template <int NT, bool ULDS, bool RA>
__global__ __launch_bounds__(64 * LSTM_MAX_WAVES) void gru_bwd_kernel(GruBwdArgs g) {
  const bool second = blockIdx.y != 0;
  const GruBwdDir p = second ? g.d[1] : g.d[0];
  const bool reverse = second ? !g.reverse : (g.reverse != 0);
  const size_t dy_row = g.dy_seq ? (size_t)g.T * g.ld : (size_t)g.ld;          // floats between two samples of dy
  extern __shared__ __attribute__((aligned(16))) float gru_lds[];
  const int SD = 3 * g.KP + 1;
  float* dzs = gru_lds;
  float* us = gru_lds + LSTM_ROWS * SD;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int fc = lane & 15, fq = lane >> 4;
  const size_t b0 = (size_t)blockIdx.x * LSTM_ROWS;
  const size_t u = (size_t)g.u, T = (size_t)g.T;

  for (int e = threadIdx.x; e < LSTM_ROWS * SD; e += blockDim.x) dzs[e] = 0.f;
  if (ULDS)
    for (int e = threadIdx.x; e < 3 * g.KP * g.SUT; e += blockDim.x) us[e] = p.utp[e];
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
    float daz[NT][4], hpv[NT][4], grv[NT][4];                         // !RA: what the second phase wants of the first
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      const int tile = wave + nw * i, j = tile * LSTM_TILE + fc;
      if (tile < g.ntiles && j < g.u) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if (rok[r]) {                                             // rows beyond B keep their +0 in dzs, and a dh of +0
            const float* gp = p.gates + (ro[r] + e_in) * 3 + j;
            const float gz = gp[0], gr = gp[u], hh = gp[2 * u];
            const float hp = p.hprev[ro[r] + e_in + j];
            const float dyv = dy_in ? p.dy[(b0 + 4 * fq + r) * dy_row + dy_pos + j] : 0.f;
            const float dhv = dyv + dh[i][r];
            const float da_z = (dhv * (hp - hh)) * lstm_act_grad(gz, g.ract);
            const float da_h = (dhv * (1.f - gz)) * lstm_act_grad(hh, g.act);
            dh[i][r] = dhv * gz;
            float* zp = p.dz + (ro[r] + e_in) * 3 + j;
            float* ls = dzs + (4 * fq + r) * SD + j;
            zp[0] = da_z;
            zp[2 * u] = da_h;
            if (RA) {
              const float qv = p.aux[ro[r] + e_in + j];
              const float da_r = (da_h * qv) * lstm_act_grad(gr, g.ract);
              const float dq = da_h * gr;
              zp[u] = da_r;
              float* rp = p.dzr + (ro[r] + e_in) * 3 + j;
              rp[0] = da_z;
              rp[u] = da_r;
              rp[2 * u] = dq;
              ls[0] = da_z;
              ls[g.KP] = da_r;
              ls[2 * g.KP] = dq;
            } else {
              ls[2 * g.KP] = da_h;
              daz[i][r] = da_z;
              hpv[i][r] = hp;
              grv[i][r] = gr;
            }
          }
        }
      }
    }
    __syncthreads();          // RA: dzr_t is complete in dzs;  !RA: da_h is complete in the h block
    if (!RA) {
#pragma unroll
      for (int i = 0; i < NT; ++i) {
        const int tile = wave + nw * i, j = tile * LSTM_TILE + fc;
        if (tile < g.ntiles) {
          const f32x4 drh = gru_bwd_chain<2>(dzs + fc * SD + fq, ub + fq * g.SUT + tile * LSTM_TILE + fc, g.SUT, 2 * g.KP, 3 * g.KP);
          if (j < g.u) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              if (rok[r]) {
                const float da_r = (drh[r] * hpv[i][r]) * lstm_act_grad(grv[i][r], g.ract);
                dh[i][r] = dh[i][r] + drh[r] * grv[i][r];
                p.dz[(ro[r] + e_in) * 3 + u + j] = da_r;
                float* ls = dzs + (4 * fq + r) * SD + j;
                ls[0] = daz[i][r];
                ls[g.KP] = da_r;
              }
            }
          }
        }
      }
      __syncthreads();        // [da_z, da_r] are complete in the z and r blocks, and every wave has left the h block
    }
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      const int tile = wave + nw * i;
      if (tile < g.ntiles) {
        const float* ap = dzs + fc * SD + fq;
        const float* bp = ub + fq * g.SUT + tile * LSTM_TILE + fc;
        const f32x4 acc = RA ? gru_bwd_chain<6>(ap, bp, g.SUT, 0, 3 * g.KP) : gru_bwd_chain<4>(ap, bp, g.SUT, 0, 2 * g.KP);
#pragma unroll
        for (int r = 0; r < 4; ++r) dh[i][r] = dh[i][r] + acc[r];
      }
    }
    if (RA) __syncthreads();  // every wave has left dzs, which step t - 1 overwrites (!RA: see the head of the file)
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

template <int NT, bool ULDS, bool RA>
void launch_fwd(const GruFwdArgs& a, const GruGeom& m, int ndir, hipStream_t s) {
  static unsigned long long big = 0;
  allow_big_lds((const void*)gru_fwd_kernel<NT, ULDS, RA>, &big);
  hipLaunchKernelGGL((gru_fwd_kernel<NT, ULDS, RA>), dim3(cdiv(a.B, LSTM_ROWS), ndir), dim3(64 * m.nwaves), m.fwd_lds_bytes, s, a);
}

template <int NT, bool ULDS, bool RA>
void launch_bwd(const GruBwdArgs& a, const GruGeom& m, int ndir, hipStream_t s) {
  static unsigned long long big = 0;
  allow_big_lds((const void*)gru_bwd_kernel<NT, ULDS, RA>, &big);
  hipLaunchKernelGGL((gru_bwd_kernel<NT, ULDS, RA>), dim3(cdiv(a.B, LSTM_ROWS), ndir), dim3(64 * m.nwaves), m.bwd_lds_bytes, s, a);
}

template <bool RA>
void pick_fwd(const GruFwdArgs& a, const GruGeom& m, int ndir, hipStream_t s) {
  if (m.fwd_u_lds) launch_fwd<1, true, RA>(a, m, ndir, s);        // u <= 104: seven tiles at the most, one a wave
  else if (m.NT == 1) launch_fwd<1, false, RA>(a, m, ndir, s);
  else if (m.NT == 2) launch_fwd<2, false, RA>(a, m, ndir, s);
  else if (m.NT == 3) launch_fwd<3, false, RA>(a, m, ndir, s);
  else launch_fwd<4, false, RA>(a, m, ndir, s);
}

template <bool RA>
void pick_bwd(const GruBwdArgs& a, const GruGeom& m, int ndir, hipStream_t s) {
  if (m.bwd_u_lds) launch_bwd<1, true, RA>(a, m, ndir, s);
  else if (m.NT == 1) launch_bwd<1, false, RA>(a, m, ndir, s);
  else if (m.NT == 2) launch_bwd<2, false, RA>(a, m, ndir, s);
  else if (m.NT == 3) launch_bwd<3, false, RA>(a, m, ndir, s);
  else launch_bwd<4, false, RA>(a, m, ndir, s);
}

// pads the U of the ndir directions into the workspace, one copy after the other, and launches the ndir directions as ONE grid
void run_fwd(GruFwdArgs a, const float* const* U, int ndir, int reset_after, const GruGeom& m, float* ws, hipStream_t s) {
  for (int d = 0; d < ndir; ++d) {
    float* up = ws + d * m.fwd_ws_floats;
    hipLaunchKernelGGL(lstm_pad_u_kernel, dim3(stream_grid(m.fwd_ws_floats)), dim3(256), 0, s, U[d], up, a.u, m.KP, m.UP, m.SU, GRU_GATES);
    a.d[d].up = up;
  }
  if (reset_after) pick_fwd<true>(a, m, ndir, s);
  else pick_fwd<false>(a, m, ndir, s);
}

void run_bwd(GruBwdArgs a, const float* const* U, int ndir, int reset_after, const GruGeom& m, float* ws, hipStream_t s) {
  for (int d = 0; d < ndir; ++d) {
    float* utp = ws + d * m.bwd_ws_floats;
    hipLaunchKernelGGL(lstm_pad_ut_kernel, dim3(stream_grid(m.bwd_ws_floats)), dim3(256), 0, s, U[d], utp, a.u, m.KP, m.SUT, GRU_GATES);
    a.d[d].utp = utp;
  }
  if (reset_after) pick_bwd<true>(a, m, ndir, s);
  else pick_bwd<false>(a, m, ndir, s);
}

// 0: launch, 1: nothing to do, GN_EINVAL: refused
int gru_check(const char* what, int B, int T, int u, int act, int ract, int reset_after) {
  GN_REQUIRE(B >= 0 && T >= 1 && u >= 1, "%s: bad shape (B %d, T %d, u %d): B >= 0, T >= 1, u >= 1", what, B, T, u);
  GN_REQUIRE(u <= LSTM_MAX_U, "%s: u = %d, at most %d units run (a block carries all units of its samples on chip)", what, u, LSTM_MAX_U);
  GN_REQUIRE(lstm_code_ok(act, false), "%s: unknown activation code %d (GN_LSTM_TANH, _SIGMOID, _RELU, _LINEAR)", what, act);
  GN_REQUIRE(lstm_code_ok(ract, true), "%s: unknown recurrent activation code %d (GN_LSTM_HARD_SIGMOID, GN_LSTM_SIGMOID)", what, ract);
  GN_REQUIRE(reset_after == 0 || reset_after == 1, "%s: reset_after = %d, 0 or 1", what, reset_after);
  GN_REQUIRE((unsigned long long)B * (unsigned long long)T < (1ull << 62) / (3ull * LSTM_MAX_U), "%s: B * T * 3u spans 2^62 elements or more", what);
  return B == 0 ? 1 : 0;
}

}  // namespace
}  // namespace gn

using namespace gn;

extern "C" {

size_t gn_gru_fwd_workspace(int u) { return (u < 1 || u > LSTM_MAX_U) ? 0 : gru_geom(u).fwd_ws_floats * sizeof(float); }

size_t gn_gru_bwd_workspace(int u) { return (u < 1 || u > LSTM_MAX_U) ? 0 : gru_geom(u).bwd_ws_floats * sizeof(float); }

int gn_gru_fwd(const float* zx, const float* U, const float* bias, const float* rbias, const float* h0, float* h, float* gates, float* hprev, float* aux,
               void* ws, size_t ws_bytes, int B, int T, int u, int act, int ract, int reset_after, int reverse, int training, void* stream) {
  const int rc = gru_check("gru_fwd", B, T, u, act, ract, reset_after);
  if (rc) return rc < 0 ? rc : GN_OK;
  GN_REQUIRE(zx && U && bias && h && ws, "gru_fwd: null pointer (zx, U, bias, h and the workspace are required)");
  GN_REQUIRE(!reset_after || rbias, "gru_fwd: null pointer (reset_after takes the recurrent bias rbias)");
  GN_REQUIRE(!training || (gates && hprev && aux), "gru_fwd: null pointer (the training phase stores gates, hprev and aux)");
  const GruGeom m = gru_geom(u);
  if (ws_bytes < m.fwd_ws_floats * sizeof(float)) {
    set_error("gru_fwd: workspace too small (%zu bytes, gn_gru_fwd_workspace(%d) = %zu)", ws_bytes, u, m.fwd_ws_floats * sizeof(float));
    return GN_EWORKSPACE;
  }
  const GruFwdDir d = {zx, nullptr, bias, rbias, h0, h, gates, hprev, aux};
  const GruFwdArgs a = {{d, d}, B, T, u, m.KP, m.UP, m.SU, m.ntiles, act, ract, reverse != 0, training != 0, u, 1};
  run_fwd(a, &U, 1, reset_after, m, (float*)ws, (hipStream_t)stream);
  return check_launch("gru_fwd");
}

int gn_gru_bwd(const float* dy, const float* gates, const float* hprev, const float* aux, const float* U, float* dz, float* dzr, float* dh0, void* ws,
               size_t ws_bytes, int B, int T, int u, int act, int ract, int reset_after, int reverse, int dy_seq, void* stream) {
  const int rc = gru_check("gru_bwd", B, T, u, act, ract, reset_after);
  if (rc) return rc < 0 ? rc : GN_OK;
  GN_REQUIRE(dy && gates && hprev && aux && U && dz && ws, "gru_bwd: null pointer (dy, gates, hprev, aux, U, dz and the workspace are required)");
  GN_REQUIRE(!reset_after || dzr, "gru_bwd: null pointer (reset_after writes dzr)");
  const GruGeom m = gru_geom(u);
  if (ws_bytes < m.bwd_ws_floats * sizeof(float)) {
    set_error("gru_bwd: workspace too small (%zu bytes, gn_gru_bwd_workspace(%d) = %zu)", ws_bytes, u, m.bwd_ws_floats * sizeof(float));
    return GN_EWORKSPACE;
  }
  const GruBwdDir d = {dy, gates, hprev, aux, nullptr, dz, dzr, dh0};
  const GruBwdArgs a = {{d, d}, B, T, u, m.KP, m.UP, m.SUT, m.ntiles, act, ract, reverse != 0, dy_seq != 0, u};
  run_bwd(a, &U, 1, reset_after, m, (float*)ws, (hipStream_t)stream);
  return check_launch("gru_bwd");
}

int gn_gru_pair_fwd(const float* const* zx, const float* const* U, const float* const* bias, const float* const* rbias, float* const* h, float* const* gates,
                    float* const* hprev, float* const* aux, void* ws, size_t ws_bytes, int B, int T, int u, int ld, int act, int ract, int reset_after,
                    int reverse0, int seq, int training, void* stream) {
  const int rc = gru_check("gru_pair_fwd", B, T, u, act, ract, reset_after);
  if (rc < 0) return rc;
  GN_REQUIRE(ld >= u, "gru_pair_fwd: ld = %d, a row of h holds at least u = %d floats", ld, u);
  if (rc) return GN_OK;
  GN_REQUIRE(zx && U && bias && h && ws, "gru_pair_fwd: null table (zx, U, bias, h and the workspace are required)");
  GN_REQUIRE(!reset_after || rbias, "gru_pair_fwd: null table (reset_after takes the recurrent biases rbias)");
  GN_REQUIRE(!training || (gates && hprev && aux), "gru_pair_fwd: null table (the training phase stores gates, hprev and aux)");
  for (int d = 0; d < 2; ++d) {
    GN_REQUIRE(zx[d] && U[d] && bias[d] && h[d], "gru_pair_fwd: null pointer in direction %d (zx, U, bias and h are required)", d);
    GN_REQUIRE(!reset_after || rbias[d], "gru_pair_fwd: null pointer in direction %d (reset_after takes the recurrent bias rbias)", d);
    GN_REQUIRE(!training || (gates[d] && hprev[d] && aux[d]), "gru_pair_fwd: null pointer in direction %d (the training phase stores gates, hprev and aux)", d);
  }
  const GruGeom m = gru_geom(u);
  if (ws_bytes < 2 * m.fwd_ws_floats * sizeof(float)) {
    set_error("gru_pair_fwd: workspace too small (%zu bytes, 2 gn_gru_fwd_workspace(%d) = %zu)", ws_bytes, u, 2 * m.fwd_ws_floats * sizeof(float));
    return GN_EWORKSPACE;
  }
  GruFwdArgs a = {{}, B, T, u, m.KP, m.UP, m.SU, m.ntiles, act, ract, reverse0 != 0, training != 0, ld, seq != 0};
  for (int d = 0; d < 2; ++d)
    a.d[d] = {zx[d], nullptr, bias[d], reset_after ? rbias[d] : nullptr, nullptr, h[d], training ? gates[d] : nullptr, training ? hprev[d] : nullptr,
              training ? aux[d] : nullptr};
  run_fwd(a, U, 2, reset_after, m, (float*)ws, (hipStream_t)stream);
  return check_launch("gru_pair_fwd");
}

int gn_gru_pair_bwd(const float* const* dy, const float* const* gates, const float* const* hprev, const float* const* aux, const float* const* U,
                    float* const* dz, float* const* dzr, void* ws, size_t ws_bytes, int B, int T, int u, int ld, int act, int ract, int reset_after,
                    int reverse0, int dy_seq, void* stream) {
  const int rc = gru_check("gru_pair_bwd", B, T, u, act, ract, reset_after);
  if (rc < 0) return rc;
  GN_REQUIRE(ld >= u, "gru_pair_bwd: ld = %d, a row of dy holds at least u = %d floats", ld, u);
  if (rc) return GN_OK;
  GN_REQUIRE(dy && gates && hprev && aux && U && dz && ws, "gru_pair_bwd: null table (dy, gates, hprev, aux, U, dz and the workspace are required)");
  GN_REQUIRE(!reset_after || dzr, "gru_pair_bwd: null table (reset_after writes dzr)");
  for (int d = 0; d < 2; ++d) {
    GN_REQUIRE(dy[d] && gates[d] && hprev[d] && aux[d] && U[d] && dz[d],
               "gru_pair_bwd: null pointer in direction %d (dy, gates, hprev, aux, U and dz are required)", d);
    GN_REQUIRE(!reset_after || dzr[d], "gru_pair_bwd: null pointer in direction %d (reset_after writes dzr)", d);
  }
  const GruGeom m = gru_geom(u);
  if (ws_bytes < 2 * m.bwd_ws_floats * sizeof(float)) {
    set_error("gru_pair_bwd: workspace too small (%zu bytes, 2 gn_gru_bwd_workspace(%d) = %zu)", ws_bytes, u, 2 * m.bwd_ws_floats * sizeof(float));
    return GN_EWORKSPACE;
  }
  GruBwdArgs a = {{}, B, T, u, m.KP, m.UP, m.SUT, m.ntiles, act, ract, reverse0 != 0, dy_seq != 0, ld};
  for (int d = 0; d < 2; ++d) a.d[d] = {dy[d], gates[d], hprev[d], aux[d], nullptr, dz[d], reset_after ? dzr[d] : nullptr, nullptr};
  run_bwd(a, U, 2, reset_after, m, (float*)ws, (hipStream_t)stream);
  return check_launch("gru_pair_bwd");
}

}  // extern "C"
