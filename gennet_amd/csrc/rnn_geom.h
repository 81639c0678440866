// Launch geometry of the SimpleRNN recurrence kernels (csrc/rnn.hip): plain host arithmetic, no HIP, so it can be compiled and
// exercised on its own (tests/tools/rnn_geom_walk.cpp walks it under the host sanitizers).  The block shape is LSTM's (lstm_geom.h): 16 batch
// rows, tiles of 16 units, at most 8 waves of at most 4 tiles, up to 512 units.  One gate block: the padded U is a third of GRU's, so it lies in
// LDS up to u = 176, forward and backward, and a block of up to 11 tiles then runs two tiles a wave.
#pragma once
#include <stddef.h>

#include "lstm_geom.h"

namespace gn {

constexpr int RNN_GATES = 1;                      // one gate block: the recurrent kernel is (u, u)

struct RnnGeom {
  int u;
  int KP;          // u up to a multiple of 8: k extent of the product (rows KP > k >= u are +0)
  int UP;          // u up to a multiple of 16: columns (columns UP > j >= u are +0)
  int SU;          // forward: floats a row of the padded U, UP | 16 (an odd multiple of 16: the four k rows of a fragment on different banks)
  int SUT;         // backward: floats a row of the padded U^T, UP | 16
  int SH;          // floats a row of an LDS state buffer of the forward, KP + 1
  int SD;          // floats a row of an LDS gradient buffer of the backward, KP + 1
  int ntiles;      // unit tiles: UP / 16
  int NT;          // tiles a wave
  int nwaves;      // waves a block: ceil(ntiles / NT) <= 8
  size_t fwd_ws_floats, bwd_ws_floats;            // the padded U (KP x SU) and U^T (KP x SUT)
  size_t fwd_state_bytes, bwd_state_bytes;        // h twice, 2 x 16 x SH;  dz twice, 2 x 16 x SD: a step reads one copy and the next writes the other
  bool fwd_u_lds, bwd_u_lds;                      // the padded matrix fits into LDS beside the state
  size_t fwd_lds_bytes, bwd_lds_bytes;            // dynamic LDS of the launch
};

// 1 <= u <= LSTM_MAX_U
inline RnnGeom rnn_geom(int u) {
  RnnGeom g;
  g.u = u;
  g.KP = (u + 7) / 8 * 8;
  g.UP = (u + 15) / 16 * 16;
  g.SU = (RNN_GATES * g.UP) | 16;
  g.SUT = g.UP | 16;
  g.SH = g.KP + 1;
  g.SD = RNN_GATES * g.KP + 1;
  g.ntiles = g.UP / LSTM_TILE;
  g.NT = (g.ntiles + LSTM_MAX_WAVES - 1) / LSTM_MAX_WAVES;
  g.nwaves = (g.ntiles + g.NT - 1) / g.NT;
  g.fwd_ws_floats = (size_t)g.KP * g.SU;
  g.bwd_ws_floats = (size_t)RNN_GATES * g.KP * g.SUT;
  g.fwd_state_bytes = (size_t)2 * LSTM_ROWS * g.SH * sizeof(float);
  g.bwd_state_bytes = (size_t)2 * LSTM_ROWS * g.SD * sizeof(float);
  g.fwd_u_lds = g.fwd_state_bytes + g.fwd_ws_floats * sizeof(float) <= LSTM_LDS_BYTES;
  g.bwd_u_lds = g.bwd_state_bytes + g.bwd_ws_floats * sizeof(float) <= LSTM_LDS_BYTES;
  g.fwd_lds_bytes = g.fwd_state_bytes + (g.fwd_u_lds ? g.fwd_ws_floats * sizeof(float) : 0);
  g.bwd_lds_bytes = g.bwd_state_bytes + (g.bwd_u_lds ? g.bwd_ws_floats * sizeof(float) : 0);
  return g;
}

}  // namespace gn
