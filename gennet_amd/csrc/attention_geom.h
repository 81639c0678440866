// Tile constants and LDS index arithmetic of csrc/attention.hip (keras layers.Attention).  Plain constexpr C++ (usable on host and device): the
// kernel file includes it, and so
// does tests/tools/attention_geom_walk.cpp, a host program that forms every LDS index of every kernel inside buffers of the stated sizes.
#pragma once

namespace gn {

constexpr int ATTN_BQ = 128;          // rows a block owns (query rows forward and in the dQ kernel, key rows in the dK / dV kernel): four waves of 32
constexpr int ATTN_BK = 64;           // rows of a staged tile (keys forward and in the dQ kernel, queries in the dK / dV kernel): two sub-tiles of 32
constexpr int ATTN_MAX_D = 128;       // largest d and dv
constexpr int ATTN_KS = ATTN_BK + 1;  // row length of a column-major tile [c][row]: odd, so 32 lanes along c at one row hit 32 banks

// column tiles of 32 that hold max(d, dv): the template parameter DT of every kernel; the padded width is DP = 32 DT
constexpr int attn_dt(int d, int dv) { return ((d > dv ? d : dv) + 31) / 32; }
constexpr int attn_vs(int DT) { return 32 * DT + 4; }                      // row length of the row-major V tile [row][c]: 16-byte rows
constexpr int attn_cmajor_floats(int DT) { return 32 * DT * ATTN_KS; }      // a column-major tile
constexpr int attn_rmajor_floats(int DT) { return ATTN_BK * attn_vs(DT); }  // the row-major tile

// the row that accumulator register r (0 .. 15) of lane half h (0, 1) holds in a 32 x 32 C/D tile; the column is lane & 31
constexpr int attn_rowmap(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// staging: piece f (0 .. 16 DP - 1, 256 lanes x 2 DT rounds) is four columns 4 cq .. 4 cq + 3 of row f / (DP / 4)
constexpr int attn_stage_pieces(int DT) { return ATTN_BK * 8 * DT; }
constexpr int attn_stage_row(int f, int DT) { return f / (8 * DT); }
constexpr int attn_stage_col(int f, int DT) { return (f % (8 * DT)) * 4; }
constexpr int attn_cmajor_at(int c, int row) { return c * ATTN_KS + row; }
constexpr int attn_rmajor_at(int row, int c, int DT) { return row * attn_vs(DT) + c; }

// dynamic LDS of each kernel, in floats
constexpr int attn_fwd_lds_floats(int DT) { return attn_cmajor_floats(DT) + attn_rmajor_floats(DT); }      // K [c][j], V [j][c]
constexpr int attn_dq_lds_floats(int DT) { return 2 * attn_cmajor_floats(DT); }                            // K [c][j], V [c][j]
constexpr int attn_dkv_lds_floats(int DT) { return 2 * attn_cmajor_floats(DT) + 2 * ATTN_BK; }             // Q [c][i], dO [c][i], lse, delta

}  // namespace gn
