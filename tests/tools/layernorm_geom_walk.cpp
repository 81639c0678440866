// Stand-alone host walk of csrc/layernorm_geom.h, the header csrc/layernorm.hip takes its regimes, grids, row ownership and workspace layout from.
// For a list of (rows, N) around every seam it plays the loops of the forward and the backward kernels as the header states them -- block, wave,
// trip, slot and lane of the rows regime, block and trip of the other two -- and checks that every row is owned exactly once, that every lane of
// a row's sub-group owns a different set of quads which together cover the N columns once, and that the blocks of the backward write every
// partial slot of gn_layernorm_bwd_workspace exactly once and none outside it (the slots live in a heap buffer of exactly that size).
// Built with the host compiler under the address and undefined-behaviour sanitizers.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "layernorm_geom.h"

using namespace gn;

static int fail(const char* what, size_t rows, int N) {
  std::printf("FAILED: %s at rows = %zu, N = %d\n", what, rows, N);
  return 1;
}

// the rows every unit of a launch of `grid` blocks owns: counts per row
static int walk_rows(size_t rows, int N, int cap, std::vector<int>& owned) {
  const unsigned grid = ln_grid(rows, N, cap);
  if (grid < 1 || grid > (unsigned)cap) return fail("grid outside 1 .. cap", rows, N);
  owned.assign(rows, 0);
  if (ln_regime(N) == 0) {
    const int W = ln_w(N), NJ = ln_nj(N), U = ln_u(NJ);
    const size_t groups = ln_groups(rows, N);
    if (W < 1 || W > 64 || (W & (W - 1)) || NJ < 1 || NJ > 4 || U * NJ > 4 || U < 1) return fail("W, NJ or U", rows, N);
    if (4 * W * NJ < N || (NJ > 1 && W != 64) || (W > 1 && 4 * (W / 2) * NJ >= N && NJ == 1)) return fail("a sub-group does not fit its row", rows, N);
    for (unsigned b = 0; b < grid; ++b)
      for (int wave = 0; wave < 4; ++wave)
        for (size_t t = 0; ln_rows_group(b, wave, t, 0, grid, U) < groups; ++t)
          for (int k = 0; k < U; ++k)
            for (int lane = 0; lane < 64; ++lane) {
              const size_t row = ln_rows_row(ln_rows_group(b, wave, t, k, grid, U), lane, N);
              if (row < rows && lane % W == 0) owned.at(row) += 1;          // the W lanes of a sub-group share the row: count it once
            }
    // the quads of a row over the lanes of its sub-group
    std::vector<int> cols(N, 0);
    for (int sl = 0; sl < W; ++sl)
      for (int j = 0; j < NJ; ++j)
        for (int e = 0; e < 4; ++e)
          if (4 * (sl + W * j) + e < N) cols.at(4 * (sl + W * j) + e) += 1;
    for (int c : cols)
      if (c != 1) return fail("a column owned not once", rows, N);
  } else {
    if (ln_regime(N) == 1 && 4 * 4 * LN_BLOCK < N) return fail("a block does not fit its row", rows, N);
    for (unsigned b = 0; b < grid; ++b)
      for (size_t t = 0; ln_block_row(b, t, grid) < rows; ++t) owned.at(ln_block_row(b, t, grid)) += 1;
  }
  for (int c : owned)
    if (c != 1) return fail("a row owned not once", rows, N);
  return 0;
}

static int walk(size_t rows, int N) {
  std::vector<int> owned;
  if (walk_rows(rows, N, LN_FWD_GRID_CAP, owned) || walk_rows(rows, N, ln_bwd_cap(N), owned)) return 1;
  // the backward workspace: the row statistics of the stream regime, then one (2, N) partial per block
  const unsigned grid = ln_grid(rows, N, ln_bwd_cap(N));
  const size_t stat = ln_ws_stat_floats(rows, N);
  std::vector<unsigned char> ws(ln_ws_floats(rows, N), 0);
  if (stat != (ln_regime(N) == 2 ? 2 * rows : 0)) return fail("statistics of the stream regime", rows, N);
  for (size_t r = 0; r < rows && stat; ++r) ws.at(2 * r) += 1, ws.at(2 * r + 1) += 1;
  for (unsigned b = 0; b < grid; ++b) {
    if (ln_regime(N) == 2) {
      for (int c0 = 0; c0 < N; c0 += LN_CHUNK)
        for (int tid = 0; tid < LN_BLOCK; ++tid)
          for (int k = 0; k < 4; ++k)
            for (int e = 0; e < 4; ++e) {
              const int c = c0 + 4 * (tid + LN_BLOCK * k) + e;
              if (c < N)
                for (int which = 0; which < 2; ++which) ws.at(stat + ln_part_slot(which, b, c, grid, N)) += 1;
            }
    } else {
      for (int c = 0; c < N; ++c)
        for (int which = 0; which < 2; ++which) ws.at(stat + ln_part_slot(which, b, c, grid, N)) += 1;
    }
  }
  for (int c : ws)
    if (c != 1) return fail("a workspace slot written not once", rows, N);
  std::printf("rows %zu N %d: regime %d, W %d, NJ %d, grids %u / %u, workspace %zu bytes\n", rows, N, ln_regime(N), ln_w(N), ln_nj(N),
              ln_grid(rows, N, LN_FWD_GRID_CAP), grid, ws.size() * sizeof(float));
  return 0;
}

int main() {
  static_assert(ln_regime(LN_ROWS_MAX_N) == 0 && ln_regime(LN_ROWS_MAX_N + 1) == 1 && ln_regime(LN_BLOCK_MAX_N) == 1 && ln_regime(LN_BLOCK_MAX_N + 1) == 2,
                "the seams");
  static_assert(ln_w(1) == 1 && ln_w(4) == 1 && ln_w(5) == 2 && ln_w(64) == 16 && ln_w(253) == 64 && ln_w(1024) == 64 && ln_nj(256) == 1 &&
                    ln_nj(257) == 2 && ln_nj(1024) == 4 && ln_u(1) == 4 && ln_u(2) == 2 && ln_u(3) == 1 && ln_u(4) == 1,
                "sub-groups");
  const int Ns[] = {1, 2, 3, 4, 5, 8, 9, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 512, 513, 768, 769, LN_ROWS_MAX_N - 1, LN_ROWS_MAX_N,
                    LN_ROWS_MAX_N + 1, 2049, LN_BLOCK_MAX_N - 1, LN_BLOCK_MAX_N, LN_BLOCK_MAX_N + 1, 2 * LN_CHUNK, 2 * LN_CHUNK + 5};
  int walked = 0;
  for (int N : Ns) {
    // 1, 3, one more than a wave holds, one more than one trip of each capped grid holds
    const size_t per_wave = ln_regime(N) == 0 ? (size_t)ln_rpw(N) : 1, per_block = ln_regime(N) == 0 ? 4 * per_wave * ln_u(ln_nj(N)) : 1;
    const size_t rows_list[] = {1, 3, per_wave + 1, per_block * ln_bwd_cap(N) + 1, per_block * LN_FWD_GRID_CAP + 1};
    for (size_t rows : rows_list) {
      if ((double)rows * N > 2e7) continue;          // the walk visits every (row, column) of the workspace: keep it to seconds
      if (walk(rows, N)) return 1;
      ++walked;
    }
  }
  std::printf("walked %d geometries\n", walked);
  return 0;
}
