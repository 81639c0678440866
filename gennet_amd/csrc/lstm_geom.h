// Launch geometry of the LSTM recurrence kernels (csrc/lstm.hip): plain host arithmetic, no HIP, so it can be compiled and
// exercised on its own (under a host sanitizer, for instance).
#pragma once
#include <stddef.h>

namespace gn {

constexpr int LSTM_ROWS = 16;                     // batch rows a block carries through the sequence: one 16 x 16 x 4 MFMA tile of rows
constexpr int LSTM_TILE = 16;                     // units a wave tile covers
constexpr int LSTM_MAX_U = 512;                   // units the entry points accept
constexpr int LSTM_MAX_WAVES = 8;                 // waves a block
constexpr int LSTM_MAX_NT = 4;                    // unit tiles a wave
constexpr size_t LSTM_LDS_BYTES = 160 * 1024;     // LDS of a CU

struct LstmGeom {
  int u;
  int KP;          // u up to a multiple of 8: k extent of a gate block (rows KP > k >= u are +0)
  int UP;          // u up to a multiple of 16: columns of a gate block (columns UP > j >= u are +0)
  int SU;          // forward: floats a row of the padded U, 4 UP + 16 (the 16 put the four k rows of a fragment on different banks)
  int SUT;         // backward: floats a row of the padded U^T, UP | 16 (an odd multiple of 16)
  int ntiles;      // unit tiles: UP / 16
  int NT;          // tiles a wave
  int nwaves;      // waves a block: ceil(ntiles / NT) <= 8
  size_t fwd_ws_floats, bwd_ws_floats;            // the padded U (KP x SU) and U^T (4 KP x SUT)
  size_t fwd_state_bytes, bwd_state_bytes;        // h, twice: 2 x 16 x (KP + 1);  dz: 16 x (4 KP + 1)
  bool fwd_u_lds, bwd_u_lds;                      // the padded matrix fits into LDS beside the state
  size_t fwd_lds_bytes, bwd_lds_bytes;            // dynamic LDS of the launch
};

// 1 <= u <= LSTM_MAX_U
inline LstmGeom lstm_geom(int u) {
  LstmGeom g;
  g.u = u;
  g.KP = (u + 7) / 8 * 8;
  g.UP = (u + 15) / 16 * 16;
  g.SU = 4 * g.UP + 16;
  g.SUT = g.UP | 16;
  g.ntiles = g.UP / LSTM_TILE;
  g.NT = (g.ntiles + LSTM_MAX_WAVES - 1) / LSTM_MAX_WAVES;
  g.nwaves = (g.ntiles + g.NT - 1) / g.NT;
  g.fwd_ws_floats = (size_t)g.KP * g.SU;
  g.bwd_ws_floats = (size_t)4 * g.KP * g.SUT;
  g.fwd_state_bytes = (size_t)2 * LSTM_ROWS * (g.KP + 1) * sizeof(float);
  g.bwd_state_bytes = (size_t)LSTM_ROWS * (4 * g.KP + 1) * sizeof(float);
  g.fwd_u_lds = g.fwd_state_bytes + g.fwd_ws_floats * sizeof(float) <= LSTM_LDS_BYTES;
  g.bwd_u_lds = g.bwd_state_bytes + g.bwd_ws_floats * sizeof(float) <= LSTM_LDS_BYTES;
  g.fwd_lds_bytes = g.fwd_state_bytes + (g.fwd_u_lds ? g.fwd_ws_floats * sizeof(float) : 0);
  g.bwd_lds_bytes = g.bwd_state_bytes + (g.bwd_u_lds ? g.bwd_ws_floats * sizeof(float) : 0);
  return g;
}

}  // namespace gn
