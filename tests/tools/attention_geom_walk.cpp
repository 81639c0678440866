// Stand-alone host walk of csrc/attention_geom.h, the header csrc/attention.hip takes its LDS layout from: for every column-tile count DT = 1 .. 4 it
// forms, inside heap buffers of exactly the sizes the launches ask for, every LDS index the three kernels form -- the staging stores of all 256 lanes
// (column-major and row-major), the A-operand reads of the score products, of the accumulating products along the columns of a column-major tile, and of
// P V along the rows of the row-major tile -- and checks that staging writes every cell a read touches exactly once and that the reads of one MFMA step
// cover the k slots (rows) of a 32-row sub-tile exactly once.  Built with the host compiler under the address and undefined-behaviour sanitizers.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "attention_geom.h"

using namespace gn;

static int fail(const char* what, int DT) {
  std::printf("FAILED: %s at DT = %d\n", what, DT);
  return 1;
}

// the stores of attn_stage: returns the cells written (counts), `cmajor` as the kernel's template flag
static void stage(std::vector<int>& cells, int base, int DT, bool cmajor) {
  for (int i = 0; i < 2 * DT; ++i)
    for (int tid = 0; tid < 256; ++tid) {
      const int f = tid + 256 * i, row = attn_stage_row(f, DT), c = attn_stage_col(f, DT);
      for (int e = 0; e < 4; ++e) cells.at(base + (cmajor ? attn_cmajor_at(c + e, row) : attn_rmajor_at(row, c + e, DT))) += 1;
    }
}

int main() {
  static_assert(ATTN_BQ == 4 * 32 && ATTN_BK == 2 * 32, "four waves of 32 rows; two sub-tiles of 32 rows");
  static_assert(attn_dt(ATTN_MAX_D, 1) == 4 && attn_dt(1, 1) == 1 && attn_dt(33, 32) == 2, "column tiles");
  for (int DT = 1; DT <= 4; ++DT) {
    if (attn_stage_pieces(DT) != 256 * 2 * DT) return fail("staging rounds", DT);
    if ((attn_cmajor_floats(DT) * 4) % 16 || (attn_vs(DT) * 4) % 16) return fail("16-byte alignment of the row-major tile", DT);
    const int sizes[3] = {attn_fwd_lds_floats(DT), attn_dq_lds_floats(DT), attn_dkv_lds_floats(DT)};
    for (int kern = 0; kern < 3; ++kern) {
      std::vector<int> cells(sizes[kern], 0);
      const int second = attn_cmajor_floats(DT);
      stage(cells, 0, DT, true);
      stage(cells, second, DT, kern != 0);
      if (kern == 2)
        for (int tid = 0; tid < ATTN_BK; ++tid) {
          cells.at(2 * second + tid) += 1;
          cells.at(2 * second + ATTN_BK + tid) += 1;
        }
      for (int lane = 0; lane < 64; ++lane) {
        const int fr = lane & 31, h = lane >> 5;
        for (int t = 0; t < 2; ++t) {
          for (int kk = 0; kk < 16 * DT; ++kk)                                    // attn_scores on both column-major tiles
            for (int tile = 0; tile < (kern == 0 ? 1 : 2); ++tile)
              if (cells.at(tile * second + attn_cmajor_at(h, 32 * t + fr) + 2 * kk * ATTN_KS) != 1) return fail("score read of an unwritten cell", DT);
          for (int u = 0; u < DT; ++u)
            for (int r = 0; r < 16; ++r) {
              if (kern == 0) {                                                      // P V: the row-major tile
                if (cells.at(second + attn_rmajor_at(32 * t + 4 * h, 32 * u + fr, DT) + attn_rowmap(r, 0) * attn_vs(DT)) != 1) return fail("V read", DT);
              } else {                                                              // attn_accum_cmajor
                for (int tile = 0; tile < (kern == 1 ? 1 : 2); ++tile)
                  if (cells.at(tile * second + attn_cmajor_at(32 * u + fr, 32 * t + 4 * h) + attn_rowmap(r, 0)) != 1) return fail("accumulating read", DT);
              }
            }
        }
      }
      // every cell of the used columns is written once, the padding column of a row (ATTN_KS - ATTN_BK, attn_vs - 32 DT) never
      long written = 0;
      for (int v : cells) {
        if (v > 1) return fail("a cell staged twice", DT);
        written += v;
      }
      const long want = 2L * ATTN_BK * 32 * DT + (kern == 2 ? 2 * ATTN_BK : 0);
      if (written != want) return fail("staged cells", DT);
    }
    bool seen[32] = {};
    for (int h = 0; h < 2; ++h)
      for (int r = 0; r < 16; ++r) {
        const int row = attn_rowmap(r, h);
        if (row < 0 || row >= 32 || seen[row] || row != attn_rowmap(r, 0) + 4 * h) return fail("rowmap is not a permutation of 32 rows", DT);
        seen[row] = true;
      }
    std::printf("DT %d: LDS bytes forward %d, dq %d, dkv %d\n", DT, 4 * attn_fwd_lds_floats(DT), 4 * attn_dq_lds_floats(DT), 4 * attn_dkv_lds_floats(DT));
    if (4 * attn_dkv_lds_floats(DT) > 160 * 1024 || 4 * attn_fwd_lds_floats(DT) > 160 * 1024) return fail("more than 160 KiB of LDS", DT);
  }
  std::printf("walked 4 geometries\n");
  return 0;
}
