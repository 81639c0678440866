// Walks the launch geometry of the SimpleRNN recurrence kernels (gennet_amd/csrc/rnn_geom.h, the header csrc/rnn.hip includes) on the host for
// every u = 1 .. 512: every index the kernels and the two padding launches form into the padded matrices and into the LDS buffers is formed here,
// the same way, into host buffers of exactly the size the geometry states, and read or written there -- so the address sanitizer sees an index
// outside its buffer, the undefined-behaviour sanitizer an overflow on the way to it, and the explicit checks say which one it was.  Built and run
// by tests/test_rnn_cpu.py under -fsanitize=address,undefined.  Exit status 0 and a last line "walked 512 geometries" when all is inside.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "rnn_geom.h"

using namespace gn;

#define CHECK(cond)                                                              \
  do {                                                                           \
    if (!(cond)) {                                                               \
      fprintf(stderr, "u = %d: %s fails (line %d)\n", g.u, #cond, __LINE__);     \
      exit(1);                                                                   \
    }                                                                            \
  } while (0)

static double walk(const RnnGeom& g) {
  double sink = 0;
  const int u = g.u, KP = g.KP, UP = g.UP, SU = g.SU, SUT = g.SUT, SH = g.SH, SD = g.SD;
  CHECK(RNN_GATES == 1);
  CHECK(KP % 8 == 0 && KP >= u && KP < u + 8 && UP % 16 == 0 && UP >= u && UP < u + 16 && KP <= UP);
  CHECK(SU >= UP && SU % 32 == 16 && SUT >= UP && SUT % 32 == 16 && SH == KP + 1 && SD == KP + 1);
  CHECK(g.ntiles * LSTM_TILE == UP && g.NT >= 1 && g.NT <= LSTM_MAX_NT && g.nwaves >= 1 && g.nwaves <= LSTM_MAX_WAVES && g.NT * g.nwaves >= g.ntiles);
  CHECK((g.NT - 1) * g.nwaves < g.ntiles);                                       // no wave without a tile in its first NT - 1 turns
  CHECK(g.fwd_lds_bytes <= LSTM_LDS_BYTES && g.bwd_lds_bytes <= LSTM_LDS_BYTES);
  CHECK(!g.fwd_u_lds || g.NT <= 2);                                              // the U-in-LDS kernels are built for one and two tiles a wave
  CHECK(!g.bwd_u_lds || g.NT <= 2);
  CHECK(g.fwd_u_lds || g.NT >= 2);                                               // and the streamed ones for two to four
  CHECK(g.bwd_u_lds || g.NT >= 2);
  CHECK(g.fwd_ws_floats == (size_t)KP * SU && g.bwd_ws_floats == (size_t)KP * SUT);

  std::vector<float> U((size_t)u * u, 1.f), up(g.fwd_ws_floats, 0.f), utp(g.bwd_ws_floats, 0.f);
  std::vector<float> fwd_lds(g.fwd_lds_bytes / sizeof(float), 0.f), bwd_lds(g.bwd_lds_bytes / sizeof(float), 0.f);

  // the padding launches (recurrent.h), G = 1
  for (size_t e = 0; e < g.fwd_ws_floats; ++e) {
    const int k = (int)(e / SU), col = (int)(e % SU), q = col / UP, j = col % UP;
    up[e] = (k < u && q < RNN_GATES && j < u) ? U[(size_t)k * RNN_GATES * u + q * u + j] : 0.f;
  }
  for (size_t e = 0; e < g.bwd_ws_floats; ++e) {
    const int row = (int)(e / SUT), j = (int)(e % SUT), q = row / KP, k = row % KP;
    CHECK(q < RNN_GATES);
    utp[e] = (k < u && j < u) ? U[(size_t)j * RNN_GATES * u + q * u + k] : 0.f;
  }

  // forward: two row buffers, then U when it is held in LDS
  float* hs0 = fwd_lds.data();
  float* hs1 = hs0 + LSTM_ROWS * SH;
  float* us = hs0 + 2 * LSTM_ROWS * SH;
  CHECK((size_t)2 * LSTM_ROWS * SH * sizeof(float) == g.fwd_state_bytes);
  if (g.fwd_u_lds) {
    CHECK(g.fwd_lds_bytes == g.fwd_state_bytes + g.fwd_ws_floats * sizeof(float));
    for (size_t e = 0; e < g.fwd_ws_floats; ++e) us[e] = up[e];
  } else {
    CHECK(g.fwd_lds_bytes == g.fwd_state_bytes);
  }
  for (int e = 0; e < LSTM_ROWS * SH; ++e) {                                      // the initial state: row e / SH, column e % SH
    CHECK(e / SH < LSTM_ROWS && e % SH <= KP);
    hs0[e] = hs1[e] = 0.f;
  }
  const float* ub = g.fwd_u_lds ? us : up.data();
  const size_t ub_n = g.fwd_ws_floats;
  for (int wave = 0; wave < g.nwaves; ++wave)
    for (int i = 0; i < g.NT; ++i) {
      const int tile = wave + g.nwaves * i;
      if (tile >= g.ntiles) continue;
      for (int lane = 0; lane < 64; ++lane) {
        const int fc = lane & 15, fq = lane >> 4, j = tile * LSTM_TILE + fc;
        for (int k0 = 0; k0 < KP; k0 += 8)
          for (int kk = 0; kk < 2; ++kk) {
            const size_t a = (size_t)fc * SH + fq + k0 + 4 * kk;
            CHECK(a < (size_t)LSTM_ROWS * SH);
            sink += hs0[a] + hs1[a];
            const size_t b = (size_t)fq * SU + j + (size_t)(k0 + 4 * kk) * SU;
            CHECK(b < ub_n);
            sink += ub[b];
            CHECK(j < u || ub[b] == 0.f);                                        // a column beyond u is +0
            CHECK(k0 + 4 * kk + fq < u || ub[b] == 0.f);                         // and so is a row beyond u
          }
        if (j < u)
          for (int r = 0; r < 4; ++r) {
            const size_t w = (size_t)(4 * fq + r) * SH + j;
            CHECK(w < (size_t)LSTM_ROWS * SH);
            hs0[w] = hs1[w] = 1.f;
          }
      }
    }

  // backward: the two gradient row buffers, then U^T when it is held in LDS
  float* dzs0 = bwd_lds.data();
  float* dzs1 = dzs0 + LSTM_ROWS * SD;
  float* ust = dzs0 + 2 * LSTM_ROWS * SD;
  CHECK((size_t)2 * LSTM_ROWS * SD * sizeof(float) == g.bwd_state_bytes);
  if (g.bwd_u_lds) {
    CHECK(g.bwd_lds_bytes == g.bwd_state_bytes + g.bwd_ws_floats * sizeof(float));
    for (size_t e = 0; e < g.bwd_ws_floats; ++e) ust[e] = utp[e];
  } else {
    CHECK(g.bwd_lds_bytes == g.bwd_state_bytes);
  }
  for (int e = 0; e < 2 * LSTM_ROWS * SD; ++e) dzs0[e] = 0.f;                     // both copies in one sweep from the first
  const float* ubt = g.bwd_u_lds ? ust : utp.data();
  for (int wave = 0; wave < g.nwaves; ++wave)
    for (int i = 0; i < g.NT; ++i) {
      const int tile = wave + g.nwaves * i;
      if (tile >= g.ntiles) continue;
      for (int lane = 0; lane < 64; ++lane) {
        const int fc = lane & 15, fq = lane >> 4, j = tile * LSTM_TILE + fc;
        if (j < u)
          for (int r = 0; r < 4; ++r) {
            const size_t w = (size_t)(4 * fq + r) * SD + j;
            CHECK(w < (size_t)LSTM_ROWS * SD);
            dzs0[w] = dzs1[w] = 1.f;
          }
        for (int k0 = 0; k0 < KP; k0 += 8)
          for (int kk = 0; kk < 2; ++kk) {
            const size_t a = (size_t)fc * SD + fq + k0 + 4 * kk;
            const size_t b = (size_t)fq * SUT + tile * LSTM_TILE + fc + (size_t)(k0 + 4 * kk) * SUT;
            CHECK(a < (size_t)LSTM_ROWS * SD && b < g.bwd_ws_floats);
            sink += dzs0[a] + dzs1[a] + ubt[b];
            CHECK(j < u || ubt[b] == 0.f);
            CHECK(k0 + 4 * kk + fq < u || ubt[b] == 0.f);
          }
      }
    }
  return sink;
}

int main() {
  double sink = 0;
  int lds_fwd = 0, lds_bwd = 0;
  for (int u = 1; u <= LSTM_MAX_U; ++u) {
    const RnnGeom g = rnn_geom(u);
    sink += walk(g);
    if (g.fwd_u_lds) lds_fwd = u;
    if (g.bwd_u_lds) lds_bwd = u;
  }
  printf("U in LDS up to u = %d forward, %d backward (%g)\n", lds_fwd, lds_bwd, sink);
  printf("walked %d geometries\n", LSTM_MAX_U);
  return 0;
}
