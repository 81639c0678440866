// Launch geometry of the depthwise convolution kernels (csrc/depthwise.hip): plain host arithmetic, no HIP, so it can be compiled and
// exercised on its own (tests/tools/depthwise_geom_walk.cpp walks it under the host sanitizers).  The tile constants, the grid rule of the three
// streaming passes, the row partition of the weight gradient and its workspace size stand here and nowhere else.
#pragma once
#include <stddef.h>

#if defined(__HIPCC__)
#define GN_DW_HD __host__ __device__
#else
#define GN_DW_HD
#endif

namespace gn {

constexpr int DW_BLOCK = 256;                     // threads a block, all three kernels
constexpr int DW_VEC = 4;                         // channels a thread on the vector path (16 bytes a lane); 1 on the scalar path
constexpr int DW_ROWS = 4;                        // forward: output rows a thread owns (a tap's weights are loaded once for them), RS rows apart
constexpr int DW_WAVE = 64;                       // lanes a wave: the forward lays RS = 64 / (channel groups) consecutive rows side by side in it
constexpr int DW_GRID_CAP = 256 * 8;              // blocks of a streaming pass: 8 a CU, the rest by the grid-stride loop
constexpr int DW_WG_TAPS = 8;                     // weight gradient: taps a sweep over the block's rows accumulates in registers
constexpr int DW_WG_MIN_ROWS = 64;                // weight gradient: rows a part holds at least (but for the last part)
constexpr int DW_WG_MAX_PARTS = 2048;             // weight gradient: row parts at the most (the grid's second dimension)
constexpr size_t DW_WG_WS_CAP = (size_t)16 << 20; // weight gradient: bytes of partial sums at the most (but one part always fits)

// blocks of a grid-stride pass over n_items items, one a thread: min(ceil(n_items / 256), 2048), at least 1
inline unsigned dw_stream_grid(unsigned long long n_items) {
  unsigned long long g = (n_items + DW_BLOCK - 1) / DW_BLOCK;
  if (g > (unsigned long long)DW_GRID_CAP) g = DW_GRID_CAP;
  return g < 1 ? 1u : (unsigned)g;
}

// forward: row lanes RS.  With fewer than 64 channel groups a row, RS = 64 / groups consecutive output rows lie side by side in a wave (its
// 64 lanes then read and write one contiguous stretch), but no more than the rows there are for the DW_ROWS-fold blocking: a thread owns the rows
// lg DW_ROWS RS + r RS + rs, r = 0 .. DW_ROWS-1, of its row group lg and row lane rs.  nvec = C dm / V >= 1, Lout >= 1.
GN_DW_HD inline int dw_fwd_row_lanes(long long nvec, int Lout) {
  long long rs = DW_WAVE / nvec;
  const long long most = (Lout + DW_ROWS - 1) / DW_ROWS;
  if (rs > most) rs = most;
  return rs < 1 ? 1 : (int)rs;
}

// forward: an item is (sample, row group, row lane, group of V output channels), the channel group fastest, then the row lane
inline unsigned long long dw_fwd_items(int B, int Lout, int C, int dm, int V) {
  const long long nvec = (long long)C * dm / V;
  const int RS = dw_fwd_row_lanes(nvec, Lout);
  return (unsigned long long)B * (unsigned long long)((Lout + DW_ROWS * RS - 1) / (DW_ROWS * RS)) * (unsigned long long)RS * (unsigned long long)nvec;
}

// data gradient: an item is (sample, input row, group of V input channels), the channel group fastest
inline unsigned long long dw_dgrad_items(int B, int L, int C, int V) {
  return (unsigned long long)B * (unsigned long long)L * (unsigned long long)(C / V);
}

struct DwWgradGeom {
  int V;                    // output channels a thread
  int NC;                   // channel lanes of a block: min(C dm / V, 256)
  int RL;                   // row lanes of a block: 256 / NC (threads NC RL .. 255 idle)
  int ctiles;               // blocks along the channels: ceil(C dm / V / NC); grid = (ctiles, parts)
  int parts;                // row parts: part p owns rows p rpp .. min((p + 1) rpp, rows) - 1 of the B Lout rows; none is empty
  unsigned long long rows;  // B Lout
  unsigned long long rpp;   // rows a part
  size_t ws_bytes;          // parts x (k C dm) doubles
};

// row parts of the weight gradient by shape alone (not by V, so the workspace does not depend on the alignment of the pointers):
// ceil(rows / 64), at most 2048, at most what keeps parts * n * 8 bytes inside 16 MiB, at least 1; then rpp = ceil(rows / that) and
// parts = ceil(rows / rpp), so no part is empty.  rows >= 1, n = k C dm >= 1.
inline void dw_wgrad_parts(unsigned long long rows, unsigned long long n, int* parts, unsigned long long* rpp) {
  unsigned long long p = (rows + DW_WG_MIN_ROWS - 1) / DW_WG_MIN_ROWS;
  if (p > (unsigned long long)DW_WG_MAX_PARTS) p = DW_WG_MAX_PARTS;
  const unsigned long long by_ws = DW_WG_WS_CAP / (n * sizeof(double));
  if (p > by_ws) p = by_ws;
  if (p < 1) p = 1;
  *rpp = (rows + p - 1) / p;
  *parts = (int)((rows + *rpp - 1) / *rpp);
}

// B, Lout, C, k, dm >= 1, k C dm < 2^31; V is 1, or DW_VEC where C dm % DW_VEC == 0
inline DwWgradGeom dw_wgrad_geom(int B, int Lout, int C, int k, int dm, int V) {
  DwWgradGeom g;
  g.V = V;
  g.rows = (unsigned long long)B * (unsigned long long)Lout;
  const unsigned long long n = (unsigned long long)k * C * dm;
  dw_wgrad_parts(g.rows, n, &g.parts, &g.rpp);
  const long long nvec = (long long)C * dm / V;
  g.NC = nvec < DW_BLOCK ? (int)nvec : DW_BLOCK;
  g.RL = DW_BLOCK / g.NC;
  g.ctiles = (int)((nvec + g.NC - 1) / g.NC);
  g.ws_bytes = (size_t)g.parts * (size_t)n * sizeof(double);
  return g;
}

// the input row of output row l at tap t; outside [0, L) it is padding
GN_DW_HD inline long long dw_in_row(long long l, int stride, int pad_left, int t, int dilation) {
  return l * stride - pad_left + (long long)t * dilation;
}

}  // namespace gn
