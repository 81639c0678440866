// Regime seams, grids, row ownership and workspace layout of csrc/layernorm.hip (keras layers.LayerNormalization).  Plain constexpr C++
// (usable on host and device): the kernel file includes it, and so does tests/tools/layernorm_geom_walk.cpp, a host program that walks every
// grid around the seams and checks that each row is owned once and each partial slot of the backward workspace written once.
// include/gennet_hip.h repeats the five seam constants as GN_LN_* defines for Python; the kernel file asserts that they agree.
#pragma once
#include <stddef.h>

namespace gn {

constexpr int LN_BLOCK = 256;            // lanes of a block: four waves of 64
constexpr int LN_ROWS_MAX_N = 1024;      // rows -> block
constexpr int LN_BLOCK_MAX_N = 4096;     // block -> stream
constexpr int LN_FWD_GRID_CAP = 2048;    // blocks of the forward; the rest by grid stride
constexpr int LN_BWD_GRID_CAP = 1024;    // blocks of the backward, each of which writes a (2, N) partial: the rows regime ...
constexpr int LN_BWD_GRID_CAP_WIDE = 512;// ... and the block and stream regimes, whose partials are the longer ones
constexpr int LN_CHUNK = LN_BLOCK_MAX_N; // stream backward: columns a block holds accumulators for at a time (4 quads a lane)

// A lane owns quads: four adjacent columns 4 q .. 4 q + 3, one 16-byte load where the row is aligned, four guarded 4-byte loads where not.
constexpr int ln_quads(int N) { return (N + 3) / 4; }
constexpr int ln_regime(int N) { return N <= LN_ROWS_MAX_N ? 0 : N <= LN_BLOCK_MAX_N ? 1 : 2; }      // 0 rows, 1 block, 2 stream

// rows: a sub-group of W = min(64, pow2ceil(quads)) lanes owns a row, lane sl the quads sl + W j, j < NJ; 64 / W rows a wave; U row groups a trip
constexpr int ln_w(int N) {
  int w = 1;
  while (w < 64 && w < ln_quads(N)) w *= 2;
  return w;
}
constexpr int ln_nj(int N) { return (ln_quads(N) + 63) / 64; }            // 1 .. 4 in the rows regime
constexpr int ln_u(int NJ) { return NJ >= 3 ? 1 : 4 / NJ; }               // at most four quads of x a lane in flight
constexpr int ln_rpw(int N) { return 64 / ln_w(N); }
constexpr size_t ln_groups(size_t rows, int N) { return (rows + ln_rpw(N) - 1) / ln_rpw(N); }

// rows: one wave per row group; block, stream: one block per row
constexpr unsigned ln_grid(size_t rows, int N, int cap) {
  const size_t blocks = ln_regime(N) == 0 ? (ln_groups(rows, N) + 3) / 4 : rows;
  return (unsigned)(blocks < 1 ? 1 : blocks > (size_t)cap ? (size_t)cap : blocks);
}
// rows: the group wave `wave` of block `block` works on in trip t, slot k < U, and the row lane `lane` has in it (>= rows: none)
constexpr size_t ln_rows_group(unsigned block, int wave, size_t t, int k, unsigned grid, int U) {
  return (size_t)block * 4 + wave + (t * U + k) * ((size_t)grid * 4);
}
constexpr size_t ln_rows_row(size_t group, int lane, int N) { return group * ln_rpw(N) + lane / ln_w(N); }
// block, stream: the row block `block` works on in trip t
constexpr size_t ln_block_row(unsigned block, size_t t, unsigned grid) { return (size_t)block + t * grid; }

constexpr int ln_bwd_cap(int N) { return ln_regime(N) == 0 ? LN_BWD_GRID_CAP : LN_BWD_GRID_CAP_WIDE; }

// backward workspace, in floats: (stream only) two a row, the row means of g and of g xhat; then the partials [2][grid][N] of dgamma and dbeta,
// one (2, N) per block
constexpr size_t ln_ws_stat_floats(size_t rows, int N) { return ln_regime(N) == 2 ? 2 * rows : 0; }
constexpr size_t ln_ws_floats(size_t rows, int N) { return ln_ws_stat_floats(rows, N) + 2 * (size_t)ln_grid(rows, N, ln_bwd_cap(N)) * (size_t)N; }
constexpr size_t ln_part_slot(int which, unsigned block, int c, unsigned grid, int N) { return ((size_t)which * grid + block) * (size_t)N + c; }

}  // namespace gn
