// Epilogue shared by the hand-scheduled fp32 conv kernel (conv_pipe.hip) and the wide-tile bf16-split kernel (conv_bf16x3.hip): both leave a
// wave's outputs as 32 x 32 MFMA accumulator tiles acc[WMT][WN] (WMT = 2 row tiles per wave; 1 in the transform-domain kernel, conv_wino.hip) (rows m_base + mt*32 + (r & 3) + 8 (r >> 2) + 4 h, columns n_base + nt*32 + i32).
#pragma once
#include "common.h"
#ifndef GN_STORE_AUX
#define GN_STORE_AUX 0      // cache policy of the output stores.  2 (nt, streaming) was measured: conv +0.5 %, but the weight gradient that reads
                            // the tensor next lost 2.7 % (144.8 -> 140.9 TFLOP/s): the write-back copies in L2 / Infinity Cache are worth keeping
#endif

namespace gn {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// Epilogue of the pipelined kernel.  The activation kind and the fused variants are dispatched ONCE per wave (template parameters), so
// the 64 outputs of a lane are straight-line code: the generic epilogue of conv_mfma_kernel re-decides the activation per element and,
// fully unrolled, is ~22k instructions of branches and waits (15 us per block against ~1 us here; measured with s_memrealtime stamps).
// Addresses: one buffer descriptor per batch element, a per-lane byte offset (column, row-within-quad) and a scalar row offset per
// register, so no 64-bit address arithmetic; rows past the end of the output (m >= M) fall outside the descriptor's range and are
// dropped by the hardware bounds check (out row = out_stride*m + out_off >= Ly exactly when m >= M).
// MODE 0: y = act(acc + bias);  MODE 1: ... then the fused Dropout keep-mask;  MODE 2: data gradient times the producer's act'(gy);
// MODE 3: MODE 2 through the producer's dropout.
struct EpiSrd {
  __amdgpu_buffer_rsrc_t y, m, g;      // output, u8 mask (MODE 1: a.mask, MODE 3: a.gmask), producer output gy (MODE >= 2) of batch element b
  float ginv;
};
template <int MODE>
__device__ __forceinline__ EpiSrd epi_srd(const ConvArgs& a, int b) {
  EpiSrd s;
  const uintptr_t yp = (uintptr_t)(a.y + (size_t)b * a.Ly * a.Cout);
  const unsigned ylo = __builtin_amdgcn_readfirstlane((unsigned)yp), yhi = __builtin_amdgcn_readfirstlane((unsigned)(yp >> 32));
  const int ybytes = __builtin_amdgcn_readfirstlane(a.Ly * a.Cout * 4);
  s.y = __builtin_amdgcn_make_buffer_rsrc((void*)(((uintptr_t)yhi << 32) | ylo), 0, ybytes, 0x00020000);
  s.m = s.y; s.g = s.y;
  if (MODE == 1 || MODE == 3) {                            // u8 masks: same element indexing, one byte per element
    const uintptr_t mp = (uintptr_t)((MODE == 1 ? a.mask : a.gmask) + (size_t)b * a.Ly * a.Cout);
    const unsigned mlo = __builtin_amdgcn_readfirstlane((unsigned)mp), mhi = __builtin_amdgcn_readfirstlane((unsigned)(mp >> 32));
    s.m = __builtin_amdgcn_make_buffer_rsrc((void*)(((uintptr_t)mhi << 32) | mlo), 0, ybytes >> 2, 0x00020000);
  }
  if (MODE >= 2) {
    const uintptr_t gp = (uintptr_t)(a.gy + (size_t)b * a.Ly * a.Cout);
    const unsigned glo = __builtin_amdgcn_readfirstlane((unsigned)gp), ghi = __builtin_amdgcn_readfirstlane((unsigned)(gp >> 32));
    s.g = __builtin_amdgcn_make_buffer_rsrc((void*)(((uintptr_t)ghi << 32) | glo), 0, ybytes, 0x00020000);
  }
  s.ginv = (MODE == 3) ? 1.0f / a.gscale : 1.0f;
  return s;
}
// one output element: v = accumulator + bias; voff = per-lane element offset, soff = wave-uniform element offset inside the batch element
template <int ACT, int MODE, int GACT>
__device__ __forceinline__ void epi_store(const ConvArgs& a, const EpiSrd& s, float v, int voff, int soff) {
  if (ACT == GN_ACT_RELU) v = fmaxf(v, 0.f);
  else if (ACT == GN_ACT_LEAKY) v = v > 0.f ? v : a.act_param * v;
  else if (ACT == GN_ACT_TANH) v = gn_tanhf(v);
  else if (ACT != GN_ACT_LINEAR) v = act_apply(v, a.act, a.act_param);         // rare kinds: runtime switch
  if (MODE == 1) {
    const unsigned k = __builtin_amdgcn_raw_buffer_load_b8(s.m, voff, soff, 0);
    v = k ? v * a.keep_scale : 0.f;
  }
  if (MODE >= 2) {
    const float gv = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(s.g, voff * 4, soff * 4, 0));
    if (MODE == 3) {
      const unsigned k = __builtin_amdgcn_raw_buffer_load_b8(s.m, voff, soff, 0);
      const float y0 = gv * s.ginv;
      const float dg = GACT == GN_ACT_LEAKY ? (y0 > 0.f ? 1.f : a.gparam) : act_grad_from_y(y0, a.gact, a.gparam);
      v = k ? v * a.gscale * dg : 0.f;
    } else {
      v *= GACT == GN_ACT_RELU ? (gv > 0.f ? 1.f : 0.f) : act_grad_from_y(gv, a.gact, a.gparam);
    }
  }
  __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), s.y, voff * 4, soff * 4, GN_STORE_AUX);
}
// The arithmetic of epi_store alone, for the epilogue that loads and stores four elements at once (tile16_wide_epilogue): k = the element's keep byte
// (MODE 1, 3), gv = the producer's output there (MODE >= 2).  The same operations in the same order, so the same bits; the two stay in step.  (epi_store
// keeps its own copy: built on this function the direct kernels' ISA came out different, and they are not to change.)
template <int ACT, int MODE, int GACT>
__device__ __forceinline__ float epi_value(const ConvArgs& a, const EpiSrd& s, float v, unsigned k, float gv) {
  if (ACT == GN_ACT_RELU) v = fmaxf(v, 0.f);
  else if (ACT == GN_ACT_LEAKY) v = v > 0.f ? v : a.act_param * v;
  else if (ACT == GN_ACT_TANH) v = gn_tanhf(v);
  else if (ACT != GN_ACT_LINEAR) v = act_apply(v, a.act, a.act_param);
  if (MODE == 1) v = k ? v * a.keep_scale : 0.f;
  if (MODE == 3) {
    const float y0 = gv * s.ginv;
    const float dg = GACT == GN_ACT_LEAKY ? (y0 > 0.f ? 1.f : a.gparam) : act_grad_from_y(y0, a.gact, a.gparam);
    v = k ? v * a.gscale * dg : 0.f;
  } else if (MODE == 2) {
    v *= GACT == GN_ACT_RELU ? (gv > 0.f ? 1.f : 0.f) : act_grad_from_y(gv, a.gact, a.gparam);
  }
  return v;
}

template <int ACT, int MODE, int GACT, int WN, int WMT = 2>
__device__ __forceinline__ void pipe_epilogue(const ConvArgs& a, const f32x16 (&acc)[WMT][WN], int b, int m_base, int n_base, int i32, int h, int out_off) {
  const EpiSrd srd = epi_srd<MODE>(a, b);
  const int rowstride = a.t.out_stride * a.Cout;           // elements between consecutive m
#pragma unroll
  for (int nt = 0; nt < WN; ++nt) {
    const int n = n_base + nt * 32 + i32;
    const float bias = a.bias ? a.bias[n] : 0.f;
    const int voff = rowstride * (4 * h) + out_off * a.Cout + n;                   // element offset of (row 4h, column n)
#pragma unroll
    for (int mt = 0; mt < WMT; ++mt) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int soff = rowstride * (m_base + mt * 32 + (r & 3) + 8 * (r >> 2));   // wave-uniform
        epi_store<ACT, MODE, GACT>(a, srd, acc[mt][nt][r] + bias, voff, soff);
      }
    }
  }
}

// The same for a wave tile of 16 x 16 accumulator tiles (v_mfma_f32_16x16x4_f32: lane (n16 = lane & 15, kq = lane >> 4) holds rows 4 kq + r,
// r = 0..3, of column n16): acc[NT4] = NT4 column tiles of 16 rows starting at m_base (conv_wino.hip).
typedef float f32x4e __attribute__((ext_vector_type(4)));
template <int ACT, int MODE, int GACT, int NT4>
__device__ __forceinline__ void tile16_epilogue(const ConvArgs& a, const f32x4e (&acc)[NT4], int b, int m_base, int n_base, int n16, int kq, int out_off) {
  const EpiSrd srd = epi_srd<MODE>(a, b);
  const int rowstride = a.t.out_stride * a.Cout;
#pragma unroll
  for (int ct = 0; ct < NT4; ++ct) {
    const int n = n_base + ct * 16 + n16;
    const float bias = a.bias ? a.bias[n] : 0.f;
    const int voff = rowstride * (4 * kq) + out_off * a.Cout + n;
#pragma unroll
    for (int r = 0; r < 4; ++r) epi_store<ACT, MODE, GACT>(a, srd, acc[ct][r] + bias, voff, rowstride * (m_base + r));
  }
}
template <int NT4>
__device__ __forceinline__ void tile16_epilogue_dispatch(const ConvArgs& a, const f32x4e (&acc)[NT4], int b, int m_base, int n_base, int n16, int kq, int out_off,
                                                         int mode) {
#define GN_EPI(A_, M_, G_) tile16_epilogue<A_, M_, G_, NT4>(a, acc, b, m_base, n_base, n16, kq, out_off)
  if (mode == 0) {
    switch (a.act) {
      case GN_ACT_LINEAR: GN_EPI(GN_ACT_LINEAR, 0, -1); break;
      case GN_ACT_RELU: GN_EPI(GN_ACT_RELU, 0, -1); break;
      case GN_ACT_LEAKY: GN_EPI(GN_ACT_LEAKY, 0, -1); break;
      case GN_ACT_TANH: GN_EPI(GN_ACT_TANH, 0, -1); break;
      default: GN_EPI(-1, 0, -1); break;
    }
  } else if (mode == 1) {
    if (a.act == GN_ACT_LEAKY) GN_EPI(GN_ACT_LEAKY, 1, -1);
    else GN_EPI(-1, 1, -1);
  } else if (mode == 2) {
    if (a.act == GN_ACT_LINEAR && a.gact == GN_ACT_RELU) GN_EPI(GN_ACT_LINEAR, 2, GN_ACT_RELU);
    else GN_EPI(-1, 2, -1);
  } else {
    if (a.act == GN_ACT_LINEAR && a.gact == GN_ACT_LEAKY) GN_EPI(GN_ACT_LINEAR, 3, GN_ACT_LEAKY);
    else GN_EPI(-1, 3, -1);
  }
#undef GN_EPI
}

// The 16-byte form of tile16_epilogue for TWO such tiles (the output phases off0 and off1 of the same 16 rows), through LDS: in the accumulator
// layout one buffer instruction covers 4 rows x 64 bytes; turned through a wave-private LDS region (2 x 16 rows x 64 columns, 8 KiB: `wreg`, free
// once the block is past the K loop's last barrier) one covers 4 rows x 256 bytes -- 16 lanes a row -- so a wave issues 8 stores (8 gy loads, 8 mask
// loads of four keep bytes) instead of 32.  A row is 256 bytes of LDS: the ds_write_b32 of the accumulator layout are 2-way (free on a 4-cycle
// instruction), the ds_read_b128 lane groups (MI355X: 0-3, 12-15, 20-27 | ...) each cover the 64 banks once.  Bias is added on the way in and
// epi_value runs on the four elements, so every element is computed by the operations of epi_store in their order: the same bits at the same
// addresses.  Needs the bases of y and gy 16-byte aligned and the mask's 4-byte aligned (Cout % 64 == 0 keeps every row so): the launch checks.
typedef unsigned u32x4e __attribute__((ext_vector_type(4)));
constexpr int kWideEpiFloats = 2 * 16 * 64;      // LDS floats of one wave's region
template <int ACT, int MODE, int GACT>
__device__ __forceinline__ void tile16_wide_epilogue(const ConvArgs& a, const f32x4e (&o0)[4], const f32x4e (&o1)[4], float* wreg, int b, int m_base, int n_base,
                                                     int lane, int off0, int off1) {
  const EpiSrd srd = epi_srd<MODE>(a, b);
  const int rowstride = a.t.out_stride * a.Cout;
  const int n16 = lane & 15, kq = lane >> 4;
  float* wr = wreg + (4 * kq) * 64 + n16;
  float bias[4] = {0.f, 0.f, 0.f, 0.f};
  if (a.bias) {                                           // the four loads in flight together
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) bias[ct] = a.bias[n_base + ct * 16 + n16];
  }
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      wr[r * 64 + ct * 16] = o0[ct][r] + bias[ct];
      wr[1024 + r * 64 + ct * 16] = o1[ct][r] + bias[ct];
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // (the LDS serves a wave's operations in order: this keeps the compiler from moving the reads up)
  const int c4 = 4 * n16;                                  // this lane's four columns of row 4 g + kq
  const float* rd = wreg + kq * 64 + c4;
  const int voff = rowstride * kq + n_base + c4;
#pragma unroll
  for (int ph = 0; ph < 2; ++ph) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      f32x4e v = *reinterpret_cast<const f32x4e*>(rd + ph * 1024 + g * 256);
      const int soff = rowstride * (m_base + 4 * g) + (ph ? off1 : off0) * a.Cout;      // wave-uniform
      unsigned k4 = 0;
      u32x4e g4 = {0u, 0u, 0u, 0u};
      if (MODE == 1 || MODE == 3) k4 = __builtin_amdgcn_raw_buffer_load_b32(srd.m, voff, soff, 0);
      if (MODE >= 2) g4 = __builtin_amdgcn_raw_buffer_load_b128(srd.g, voff * 4, soff * 4, 0);
      u32x4e o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float ve = v[e];                             // (scalars first: __builtin_bit_cast of a vector ELEMENT reads element 0 whatever the index)
        const unsigned ge = g4[e];
        o[e] = __builtin_bit_cast(unsigned, epi_value<ACT, MODE, GACT>(a, srd, ve, (k4 >> (8 * e)) & 0xffu, __builtin_bit_cast(float, ge)));
      }
      __builtin_amdgcn_raw_buffer_store_b128(o, srd.y, voff * 4, soff * 4, GN_STORE_AUX);
    }
  }
}
__device__ __forceinline__ void tile16_wide_epilogue_dispatch(const ConvArgs& a, const f32x4e (&o0)[4], const f32x4e (&o1)[4], float* wreg, int b, int m_base,
                                                              int n_base, int lane, int off0, int off1, int mode) {
#define GN_EPI(A_, M_, G_) tile16_wide_epilogue<A_, M_, G_>(a, o0, o1, wreg, b, m_base, n_base, lane, off0, off1)
  if (mode == 0) {
    switch (a.act) {
      case GN_ACT_LINEAR: GN_EPI(GN_ACT_LINEAR, 0, -1); break;
      case GN_ACT_RELU: GN_EPI(GN_ACT_RELU, 0, -1); break;
      case GN_ACT_LEAKY: GN_EPI(GN_ACT_LEAKY, 0, -1); break;
      case GN_ACT_TANH: GN_EPI(GN_ACT_TANH, 0, -1); break;
      default: GN_EPI(-1, 0, -1); break;
    }
  } else if (mode == 1) {
    if (a.act == GN_ACT_LEAKY) GN_EPI(GN_ACT_LEAKY, 1, -1);
    else GN_EPI(-1, 1, -1);
  } else if (mode == 2) {
    if (a.act == GN_ACT_LINEAR && a.gact == GN_ACT_RELU) GN_EPI(GN_ACT_LINEAR, 2, GN_ACT_RELU);
    else GN_EPI(-1, 2, -1);
  } else {
    if (a.act == GN_ACT_LINEAR && a.gact == GN_ACT_LEAKY) GN_EPI(GN_ACT_LINEAR, 3, GN_ACT_LEAKY);
    else GN_EPI(-1, 3, -1);
  }
#undef GN_EPI
}
// host side of the above: the base addresses a launch's 16-byte epilogue needs
static inline bool wide_epilogue_aligned(const ConvArgs& a) {
  const uintptr_t mk = (uintptr_t)(a.gy ? a.gmask : a.mask);
  return (uintptr_t)a.y % 16 == 0 && (uintptr_t)a.gy % 16 == 0 && mk % 4 == 0;
}

// uniform dispatch, decided once per wave; every case is straight-line code.  Specialised: the forms the three networks run (forward
// linear / relu / LeakyReLU / tanh, LeakyReLU + dropout, data gradient through relu, through LeakyReLU + dropout); the rest take the
// variants that decide the activation per element.
template <int WN, int WMT = 2>
__device__ __forceinline__ void pipe_epilogue_dispatch(const ConvArgs& a, const f32x16 (&acc)[WMT][WN], int b, int m_base, int n_base, int i32, int h, int out_off,
                                                       int mode) {
#define GN_EPI(A_, M_, G_) pipe_epilogue<A_, M_, G_, WN, WMT>(a, acc, b, m_base, n_base, i32, h, out_off)
  if (mode == 0) {
    switch (a.act) {
      case GN_ACT_LINEAR: GN_EPI(GN_ACT_LINEAR, 0, -1); break;
      case GN_ACT_RELU: GN_EPI(GN_ACT_RELU, 0, -1); break;
      case GN_ACT_LEAKY: GN_EPI(GN_ACT_LEAKY, 0, -1); break;
      case GN_ACT_TANH: GN_EPI(GN_ACT_TANH, 0, -1); break;
      default: GN_EPI(-1, 0, -1); break;
    }
  } else if (mode == 1) {
    if (a.act == GN_ACT_LEAKY) GN_EPI(GN_ACT_LEAKY, 1, -1);
    else GN_EPI(-1, 1, -1);
  } else if (mode == 2) {
    if (a.act == GN_ACT_LINEAR && a.gact == GN_ACT_RELU) GN_EPI(GN_ACT_LINEAR, 2, GN_ACT_RELU);
    else GN_EPI(-1, 2, -1);
  } else {
    if (a.act == GN_ACT_LINEAR && a.gact == GN_ACT_LEAKY) GN_EPI(GN_ACT_LINEAR, 3, GN_ACT_LEAKY);
    else GN_EPI(-1, 3, -1);
  }
#undef GN_EPI
}

// Block -> tile of the tiled conv launches (conv_pipe.hip, conv_wino.hip, conv_wino_s2.hip).  Plain order is (slab, column tile) with the column tile fastest: block i runs on
// XCD i mod 8, so every XCD meets every input slab and the slab crosses the fabric 8 times.  Patch order (patch >= 0) hands each XCD, out of every 512
// consecutive blocks, the 64 blocks of ONE patch of (64 / PN) slabs x PN column tiles (PN = 8, or 4 when there are only 4 column tiles) -- the set an
// XCD has in flight at two blocks per CU -- so its L2 serves each slab chunk to PN blocks and each weight chunk to 64 / PN.
// patch = log2(column tiles / PN) | log2(PN) << 8.  Blocks past the last whole 512 keep the plain order (both orders cover the same leading slabs).
// Measured on G 512 -> 1024 (conv_pipe.hip): FETCH_SIZE -25 %, +0.3 % on the step.  A slab is m_tiles row tiles of one batch element.
struct BlockTile {
  int n_tile, m_tile, b;
};
__device__ __forceinline__ BlockTile xcd_block_tile(int patch, int m_tiles, int n_tiles) {
  const int bid = blockIdx.x;
  int n_lin, slab;
  if (patch >= 0 && bid < (int)(gridDim.x & ~511u)) {
    const int ps = patch & 255, pn = patch >> 8;
    const int r = bid & 511, p = (bid >> 9) * 8 + (r & 7), idx = r >> 3;
    slab = ((p >> ps) << (6 - pn)) + (idx >> pn);
    n_lin = ((p & ((1 << ps) - 1)) << pn) + (idx & ((1 << pn) - 1));
  } else {
    n_lin = bid % n_tiles;
    slab = bid / n_tiles;
  }
  BlockTile t;
  t.n_tile = __builtin_amdgcn_readfirstlane(n_lin);
  const int slab_s = __builtin_amdgcn_readfirstlane(slab);
  t.m_tile = slab_s % m_tiles;
  t.b = slab_s / m_tiles;
  return t;
}
// the patch argument of a launch with n_tiles column tiles; -1 (plain order) when no patch shape fits
static inline int xcd_patch(int n_tiles) {
  const int pn = n_tiles % 8 == 0 ? 3 : (n_tiles == 4 ? 2 : -1);
  const int ng = pn >= 0 ? n_tiles >> pn : 0;
  return pn >= 0 && ng <= 8 && (ng & (ng - 1)) == 0 ? __builtin_ctz(ng) | (pn << 8) : -1;
}

}  // namespace gn
