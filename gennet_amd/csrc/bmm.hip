// Batched fp32 matrix product (keras layers/merge.py Dot through K.batch_dot) and the L2 normalisation of Dot(normalize=True).
//
//   gn_bmm      c[(bt*M + m)*N + n] = sum_k a[bt*a_batch + m*a_m + k*a_k] * b[bt*b_batch + k*b_k + n*b_n]          strides in elements, c contiguous
//
// The forward product and both gradients of Dot are this one entry point under different strides: for each operand one of its two matrix
// strides is 1 and the other the row length, so nothing is transposed in memory and every result is written in its owner's layout.
//
// Kernels, chosen in ONE place (bmm_path) by shape alone:
//   mfma   M >= 2 and N >= 2.  256 lanes, four waves as 2 x 2, a wave owns TM x TN tiles of 32 x 32 on v_mfma_f32_32x32x2_f32 (16 accumulator
//          registers a tile, the C/D map col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)).  The block tile is 64 TM x 64 TN:
//          128 a side where the extent is beyond 64 and the grid still has 1024 blocks, else 64 (run_mfma): 128 x 128, 128 x 64, 64 x 128, 64 x 64.
//          K goes in chunks of BK = 16 through LDS, two buffers, one barrier a chunk: the next chunk's global loads are issued before the MFMAs
//          of this one and parked in LDS after them.  Both operands lie k-major in LDS, As[k][m] and Bs[k][n], rows of 64 T + 4 floats:
//            * the fragment read As[k0 + (lane >> 5)][m0 + (lane & 31)] is 32 consecutive floats per 32-lane group: no conflict under any row length;
//            * an operand that is contiguous along m (n) arrives as float4 of four m at one k and is parked with one 16-byte store
//              (rows are multiples of 16 bytes);
//            * an operand that is contiguous along k arrives as float4 of four k at one m, four lanes a row, and is parked with four 4-byte stores
//              at rows 4 kq + j: banks (16 kq + 4 j + m) mod 32 with m = 0 .. 7 inside a 32-lane group, two lanes a bank, which a 4-byte store
//              absorbs (its register transfer is the longer part); a row of 64 T floats (pad 0) would put all four kq on one bank.
//          Either way consecutive lanes read consecutive 16-byte pieces along whichever stride is 1.  The 16-byte load is taken only when the base
//          pointer is 16-byte aligned and the batch stride and the row length are multiples of 4; otherwise, and at the edges, guarded 4-byte loads.
//          Everything outside M, N, K is an exact +0 in LDS, so any M, N, K >= 1 runs.
//   thin   M == 1 or N == 1 (the rank-2 Dot, attention pooling, their gradients): a matrix-core tile would be 1/32 full and the work is bound by
//          memory.  The product is a matrix X (rows r = m or n) times a vector.  Rows contiguous in k: a wave per output, lane l adds k = l, l + 64, ..
//          in order and the 64 partials meet in an xor butterfly (1, 2, .. 32; both partners form a + b).  Rows strided in k (r contiguous): a lane per
//          output walks k in order, consecutive lanes consecutive addresses.
//   valu   gn_bmm_valu, never selected: capi.hip's dense_any 16 x 16 VALU tile with a batch index, the yardstick of scripts/bmm_microbench.py and
//          a second implementation for the tests.
//
// NUMERICS.  No split-K, no atomics.  In the mfma and valu kernels, and in the thin kernel's lane-per-output form, every output is ONE fp32 fma chain
// in k order starting from +0: c = fma(a_{K-1}, b_{K-1}, ... fma(a_1, b_1, fma(a_0, b_0, +0))) (the f32 MFMA is bit for bit that chain, one rounding
// a product, no wider accumulator).  The zero padding adds fma(+0, +0, c) = c exactly (c is never -0: the chain starts at +0).  So an output depends
// on its own row of a and column of b only: not on the tile, the batch size, the position in the launch, or which of these kernels computed it.  The
// thin kernel's wave-per-output form fixes its order by K alone (64 chains of stride 64, then the butterfly): equally independent of the launch, but
// not the k-order chain.  Two runs give identical bits.
//
//   gn_l2norm_fwd / _bwd   tf.nn.l2_normalize on the (outer, P, inner) view of softmax.hip: s = sum_p x^2, inv = 1 / sqrt(max(s, 1e-12)), y = x * inv;
//          dx = inv * (dy - y * sum_p dy * y), and where s was clamped (s < 1e-12: inv is the constant 1e6) dx = inv * dy.  The clamped case is told
//          by inv itself: inv == 1e6f, the fp32 value of 1 / sqrt(1e-12f), iff s was below the floor or within a few ulp above it, where the rounded
//          inverse root is the same number (the forward value is the same; at the tie TensorFlow's maximum hands its gradient to either side as
//          well).  inner == 1: a wave per row, lanes stride p, butterfly; inner > 1: a lane per (o, i) column walks p in order.  Fixed-order fp32
//          sums, no atomics.
#include <math.h>

#include "common.h"

namespace gn {
namespace {

constexpr int BMM_BK = 16;               // k per LDS chunk
constexpr int BMM_PAD = 4;               // floats behind a row of 64 T
constexpr int BMM_GRID_CAP = 4096;       // thin / l2norm: blocks of 256, the rest by grid stride
constexpr unsigned long long BMM_FILL_BLOCKS = 1024;      // mfma: fewer blocks than this (4 a CU) take the 64-wide tile

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct BmmArgs {
  const float* a;
  const float* b;
  float* c;
  int batch, M, N, K;
  long long a_batch, a_m, a_k, b_batch, b_k, b_n;
};

// One operand's chunk: ROWS = 64 T positions along m (n) by BK along k, as ROWS * BK / 4 float4 over 256 lanes.
// kcontig false: piece f is four m at k = f / (ROWS / 4); true: four k at m = f / 4.  `s1` is the stride that is not 1.
template <int ROWS>
struct Stage {
  static constexpr int NV = ROWS * BMM_BK / 4 / 256;
  float4 v[NV];

  __device__ __forceinline__ void load(const float* __restrict__ p, long long s1, bool kcontig, bool vec, int r0, int R, int k0, int K) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int f = threadIdx.x + 256 * i;
      float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
      if (!kcontig) {
        const int k = k0 + f / (ROWS / 4), r = r0 + (f % (ROWS / 4)) * 4;
        if (k < K && r < R) {
          const float* q = p + (long long)k * s1 + r;
          if (vec && r + 3 < R) {
            t = *reinterpret_cast<const float4*>(q);
          } else {
            t.x = q[0];
            if (r + 1 < R) t.y = q[1];
            if (r + 2 < R) t.z = q[2];
            if (r + 3 < R) t.w = q[3];
          }
        }
      } else {
        const int r = r0 + f / 4, k = k0 + (f % 4) * 4;
        if (r < R && k < K) {
          const float* q = p + (long long)r * s1 + k;
          if (vec && k + 3 < K) {
            t = *reinterpret_cast<const float4*>(q);
          } else {
            t.x = q[0];
            if (k + 1 < K) t.y = q[1];
            if (k + 2 < K) t.z = q[2];
            if (k + 3 < K) t.w = q[3];
          }
        }
      }
      v[i] = t;
    }
  }

  __device__ __forceinline__ void park(float* lds, bool kcontig) const {
    constexpr int S = ROWS + BMM_PAD;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int f = threadIdx.x + 256 * i;
      if (!kcontig) {
        *reinterpret_cast<float4*>(lds + (f / (ROWS / 4)) * S + (f % (ROWS / 4)) * 4) = v[i];
      } else {
        float* q = lds + (f % 4) * 4 * S + f / 4;
        q[0] = v[i].x;
        q[S] = v[i].y;
        q[2 * S] = v[i].z;
        q[3 * S] = v[i].w;
      }
    }
  }
};

template <int TM, int TN>
__global__ __launch_bounds__(256) void bmm_mfma_kernel(BmmArgs g, unsigned tiles_m, unsigned tiles_n, bool a_kc, bool b_kc, bool a_vec, bool b_vec) {
  constexpr int BM = 64 * TM, BN = 64 * TN, SA = BM + BMM_PAD, SB = BN + BMM_PAD;
  __shared__ __attribute__((aligned(16))) float As[2][BMM_BK * SA];
  __shared__ __attribute__((aligned(16))) float Bs[2][BMM_BK * SB];
  const unsigned per = tiles_m * tiles_n, bt = blockIdx.x / per, tile = blockIdx.x % per;
  const int m0 = (int)(tile / tiles_n) * BM, n0 = (int)(tile % tiles_n) * BN;
  const float* __restrict__ a = g.a + (long long)bt * g.a_batch;
  const float* __restrict__ b = g.b + (long long)bt * g.b_batch;
  const long long a_s1 = a_kc ? g.a_m : g.a_k, b_s1 = b_kc ? g.b_n : g.b_k;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = (wave >> 1) * 32 * TM, wn = (wave & 1) * 32 * TN;       // the wave's corner inside the block tile
  const int fr = lane & 31, fk = lane >> 5;

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  Stage<BM> sa;
  Stage<BN> sb;
  sa.load(a, a_s1, a_kc, a_vec, m0, g.M, 0, g.K);
  sb.load(b, b_s1, b_kc, b_vec, n0, g.N, 0, g.K);
  sa.park(As[0], a_kc);
  sb.park(Bs[0], b_kc);
  __syncthreads();
  const int chunks = (g.K + BMM_BK - 1) / BMM_BK;
  for (int c = 0; c < chunks; ++c) {
    const bool more = c + 1 < chunks;
    if (more) {
      sa.load(a, a_s1, a_kc, a_vec, m0, g.M, (c + 1) * BMM_BK, g.K);
      sb.load(b, b_s1, b_kc, b_vec, n0, g.N, (c + 1) * BMM_BK, g.K);
    }
    const float* as = As[c & 1] + fk * SA + wm + fr;
    const float* bs = Bs[c & 1] + fk * SB + wn + fr;
#pragma unroll
    for (int kk = 0; kk < BMM_BK; kk += 2) {
      float av[TM], bv[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) av[i] = as[kk * SA + 32 * i];
#pragma unroll
      for (int j = 0; j < TN; ++j) bv[j] = bs[kk * SB + 32 * j];
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[j], acc[i][j], 0, 0, 0);
    }
    if (more) {                                    // the other buffer: every wave left it at the barrier that ended chunk c - 1
      sa.park(As[(c + 1) & 1], a_kc);
      sb.park(Bs[(c + 1) & 1], b_kc);
    }
    __syncthreads();
  }

  float* __restrict__ cb = g.c + (long long)bt * g.M * g.N;
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int n = n0 + wn + 32 * j + fr;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * fk;
        if (m < g.M && n < g.N) cb[(long long)m * g.N + n] = acc[i][j][r];
      }
    }
}

// capi.hip's dense_any tile, batched: one output a lane, fmaf in k order
__global__ __launch_bounds__(256) void bmm_valu_kernel(BmmArgs g, unsigned tiles_m, unsigned tiles_n) {
  __shared__ float As[16][17], Bs[16][17];
  const unsigned per = tiles_m * tiles_n, bt = blockIdx.x / per, tile = blockIdx.x % per;
  const int tx = threadIdx.x % 16, ty = threadIdx.x / 16;
  const int m = (int)(tile / tiles_n) * 16 + ty, n = (int)(tile % tiles_n) * 16 + tx;
  const float* __restrict__ a = g.a + (long long)bt * g.a_batch;
  const float* __restrict__ b = g.b + (long long)bt * g.b_batch;
  float acc = 0.f;
  for (int k0 = 0; k0 < g.K; k0 += 16) {
    const int ka = k0 + tx, kb = k0 + ty;
    As[ty][tx] = (m < g.M && ka < g.K) ? a[(long long)m * g.a_m + (long long)ka * g.a_k] : 0.f;
    Bs[ty][tx] = (kb < g.K && n < g.N) ? b[(long long)kb * g.b_k + (long long)n * g.b_n] : 0.f;
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) acc = fmaf(As[ty][kk], Bs[kk][tx], acc);
    __syncthreads();
  }
  if (m < g.M && n < g.N) g.c[((long long)bt * g.M + m) * g.N + n] = acc;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int d = 1; d < 64; d *= 2) v += __shfl_xor(v, d, 64);
  return v;
}

// thin: out[bt*R + r] = sum_k x[bt*x_batch + r*x_r + k*x_k] * v[bt*v_batch + k*v_k]
struct ThinArgs {
  const float* x;
  const float* v;
  float* c;
  size_t total;            // batch * R
  int R, K;
  long long x_batch, x_r, x_k, v_batch, v_k;
};

// a wave per output, x_k == 1
__global__ __launch_bounds__(256) void bmm_thin_rows_kernel(ThinArgs g) {
  const int lane = threadIdx.x & 63;
  const size_t nwaves = (size_t)gridDim.x * 4;
  for (size_t o = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6); o < g.total; o += nwaves) {
    const long long bt = (long long)(o / g.R), r = (long long)(o % g.R);
    const float* __restrict__ x = g.x + bt * g.x_batch + r * g.x_r;
    const float* __restrict__ v = g.v + bt * g.v_batch;
    float acc = 0.f;
    for (int k = lane; k < g.K; k += 64) acc = fmaf(x[k], v[(long long)k * g.v_k], acc);
    acc = wave_sum(acc);
    if (lane == 0) g.c[o] = acc;
  }
}

// a lane per output, x_r == 1
__global__ __launch_bounds__(256) void bmm_thin_cols_kernel(ThinArgs g) {
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t o = (size_t)blockIdx.x * 256 + threadIdx.x; o < g.total; o += stride) {
    const long long bt = (long long)(o / g.R), r = (long long)(o % g.R);
    const float* __restrict__ x = g.x + bt * g.x_batch + r;
    const float* __restrict__ v = g.v + bt * g.v_batch;
    float acc = 0.f;
    for (int k = 0; k < g.K; ++k) acc = fmaf(x[(long long)k * g.x_k], v[(long long)k * g.v_k], acc);
    g.c[o] = acc;
  }
}

unsigned capped(size_t blocks) { return (unsigned)(blocks < 1 ? 1 : blocks > (size_t)BMM_GRID_CAP ? (size_t)BMM_GRID_CAP : blocks); }

// THE switch between the kernels of gn_bmm: a product with a single row or a single column is a matrix-vector product
enum BmmPath { BMM_THIN, BMM_MFMA };
BmmPath bmm_path(int M, int N) { return M == 1 || N == 1 ? BMM_THIN : BMM_MFMA; }

bool vec_ok(const float* p, long long batch_stride, long long s1, int batch) {
  return ((uintptr_t)p & 15) == 0 && s1 % 4 == 0 && (batch <= 1 || batch_stride % 4 == 0);
}

template <int TM, int TN>
void launch_mfma(const BmmArgs& g, unsigned tm, unsigned tn, hipStream_t s) {
  const bool a_kc = g.a_k == 1 && !(g.a_m == 1 && g.M > 1), b_kc = g.b_k == 1 && !(g.b_n == 1 && g.N > 1);
  hipLaunchKernelGGL((bmm_mfma_kernel<TM, TN>), dim3(tm * tn * (unsigned)g.batch), dim3(256), 0, s, g, tm, tn, a_kc, b_kc,
                     vec_ok(g.a, g.a_batch, a_kc ? g.a_m : g.a_k, g.batch), vec_ok(g.b, g.b_batch, b_kc ? g.b_n : g.b_k, g.batch));
}

int run_mfma(const BmmArgs& g, hipStream_t s) {
  // 128 per side where the extent is beyond 64, unless that leaves fewer than BMM_FILL_BLOCKS blocks: a block keeps 16 KiB of loads in flight, and
  // one or two blocks a CU leave the latency of a chunk's global loads exposed (attention's a . v at N = C = 64 .. 128).  Then N, then M
  // goes to 64.  By shape alone; the result does not depend on the tile.
  int bm = g.M <= 64 ? 64 : 128, bn = g.N <= 64 ? 64 : 128;
  const auto blocks = [&](int m, int n) { return (unsigned long long)cdiv(g.M, m) * cdiv(g.N, n) * (unsigned long long)g.batch; };
  if (bn == 128 && blocks(bm, bn) < BMM_FILL_BLOCKS) bn = 64;
  if (bm == 128 && blocks(bm, bn) < BMM_FILL_BLOCKS) bm = 64;
  const unsigned tm = cdiv(g.M, bm), tn = cdiv(g.N, bn);
  GN_REQUIRE((unsigned long long)tm * tn * (unsigned long long)g.batch < 0x80000000ull, "bmm: %u x %u tiles x %d batch entries exceed the grid (2^31 - 1 blocks)",
             tm, tn, g.batch);
  if (bm == 128 && bn == 128) launch_mfma<2, 2>(g, tm, tn, s);
  else if (bm == 128) launch_mfma<2, 1>(g, tm, tn, s);
  else if (bn == 128) launch_mfma<1, 2>(g, tm, tn, s);
  else launch_mfma<1, 1>(g, tm, tn, s);
  return check_launch("bmm");
}

int run_thin(const BmmArgs& g, hipStream_t s) {
  ThinArgs t;
  t.c = g.c;
  t.K = g.K;
  if (g.N == 1) {               // c[bt, m] = sum_k a[bt, m, k] b[bt, k]
    t.x = g.a; t.x_batch = g.a_batch; t.x_r = g.a_m; t.x_k = g.a_k; t.R = g.M;
    t.v = g.b; t.v_batch = g.b_batch; t.v_k = g.b_k;
  } else {                      // M == 1: c[bt, n] = sum_k b[bt, k, n] a[bt, k]
    t.x = g.b; t.x_batch = g.b_batch; t.x_r = g.b_n; t.x_k = g.b_k; t.R = g.N;
    t.v = g.a; t.v_batch = g.a_batch; t.v_k = g.a_k;
  }
  t.total = (size_t)g.batch * (size_t)t.R;
  if (t.x_r == 1 && (t.x_k != 1 || t.K == 1)) hipLaunchKernelGGL(bmm_thin_cols_kernel, dim3(capped((t.total + 255) / 256)), dim3(256), 0, s, t);
  else hipLaunchKernelGGL(bmm_thin_rows_kernel, dim3(capped((t.total + 3) / 4)), dim3(256), 0, s, t);
  return check_launch("bmm_thin");
}

// 0: launch, 1: nothing to do (GN_OK), GN_EINVAL: refused
int bmm_check(const char* what, const BmmArgs& g) {
  GN_REQUIRE(g.batch >= 0 && g.M >= 0 && g.N >= 0, "%s: negative size (batch %d, M %d, N %d)", what, g.batch, g.M, g.N);
  GN_REQUIRE(g.K >= 1, "%s: K = %d, at least 1 (an empty sum has no kernel)", what, g.K);
  if (g.batch == 0 || g.M == 0 || g.N == 0) return 1;
  GN_REQUIRE(g.a_batch > 0 && g.a_m > 0 && g.a_k > 0 && g.b_batch > 0 && g.b_k > 0 && g.b_n > 0,
             "%s: strides must be positive (a: %lld %lld %lld, b: %lld %lld %lld)", what, g.a_batch, g.a_m, g.a_k, g.b_batch, g.b_k, g.b_n);
  GN_REQUIRE((g.a_m == 1 && g.a_k >= g.M) || (g.a_k == 1 && g.a_m >= g.K),
             "%s: a's strides (m %lld, k %lld) for M %d, K %d: one must be 1 and the other at least the extent of the contiguous axis", what, g.a_m, g.a_k, g.M,
             g.K);
  GN_REQUIRE((g.b_n == 1 && g.b_k >= g.N) || (g.b_k == 1 && g.b_n >= g.K),
             "%s: b's strides (k %lld, n %lld) for K %d, N %d: one must be 1 and the other at least the extent of the contiguous axis", what, g.b_k, g.b_n, g.K,
             g.N);
  GN_REQUIRE(g.a && g.b && g.c, "%s: null pointer", what);
  const unsigned __int128 lim = (unsigned __int128)1 << 62;
  const unsigned __int128 ea = (unsigned __int128)(g.batch - 1) * g.a_batch + (unsigned __int128)(g.M - 1) * g.a_m + (unsigned __int128)(g.K - 1) * g.a_k;
  const unsigned __int128 eb = (unsigned __int128)(g.batch - 1) * g.b_batch + (unsigned __int128)(g.K - 1) * g.b_k + (unsigned __int128)(g.N - 1) * g.b_n;
  const unsigned __int128 ec = (unsigned __int128)g.batch * g.M * g.N;
  GN_REQUIRE(ea < lim && eb < lim && ec < lim, "%s: an operand spans 2^62 elements or more", what);
  return 0;
}

// ---------------------------------------------------------------------------------------------
// l2 normalisation
// ---------------------------------------------------------------------------------------------
constexpr float L2_EPS = 1e-12f;

constexpr float L2_INV_MAX = 1e6f;      // 1 / sqrt(1e-12f) rounded to fp32: (float)1e-12 = 9.99999996e-13, its inverse root 1000000.002, half an ulp is 0.03
__device__ __forceinline__ float l2_inv(float s) { return s < L2_EPS ? L2_INV_MAX : 1.f / sqrtf(s); }
__device__ __forceinline__ bool l2_clamped(float inv) { return inv == L2_INV_MAX; }

// inner == 1: a wave per row
template <bool BWD>
__global__ __launch_bounds__(256) void l2norm_rows_kernel(const float* __restrict__ a, const float* __restrict__ yin, const float* __restrict__ invin,
                                                          float* __restrict__ out, float* __restrict__ invout, size_t outer, int P) {
  const int lane = threadIdx.x & 63;
  const size_t nwaves = (size_t)gridDim.x * 4;
  for (size_t o = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6); o < outer; o += nwaves) {
    const size_t base = o * (size_t)P;
    float acc = 0.f;
    if (!BWD) {
      for (int p = lane; p < P; p += 64) acc = fmaf(a[base + p], a[base + p], acc);
      const float inv = l2_inv(wave_sum(acc));
      for (int p = lane; p < P; p += 64) out[base + p] = a[base + p] * inv;
      if (lane == 0) invout[o] = inv;
    } else {
      const float inv = invin[o];
      if (!l2_clamped(inv))
        for (int p = lane; p < P; p += 64) acc = fmaf(a[base + p], yin[base + p], acc);
      const float t = wave_sum(acc);
      for (int p = lane; p < P; p += 64) out[base + p] = l2_clamped(inv) ? inv * a[base + p] : inv * (a[base + p] - yin[base + p] * t);
    }
  }
}

// inner > 1: a lane per (o, i) column
template <bool BWD>
__global__ __launch_bounds__(256) void l2norm_axis_kernel(const float* __restrict__ a, const float* __restrict__ yin, const float* __restrict__ invin,
                                                          float* __restrict__ out, float* __restrict__ invout, size_t outer, int P, int inner) {
  const size_t ncol = outer * (size_t)inner, stride = (size_t)gridDim.x * 256;
  for (size_t col = (size_t)blockIdx.x * 256 + threadIdx.x; col < ncol; col += stride) {
    const size_t base = (col / inner) * (size_t)P * inner + col % inner;
    float acc = 0.f;
    if (!BWD) {
      for (int p = 0; p < P; ++p) {
        const float x = a[base + (size_t)p * inner];
        acc = fmaf(x, x, acc);
      }
      const float inv = l2_inv(acc);
      for (int p = 0; p < P; ++p) out[base + (size_t)p * inner] = a[base + (size_t)p * inner] * inv;
      invout[col] = inv;
    } else {
      const float inv = invin[col];
      const bool cl = l2_clamped(inv);
      if (!cl)
        for (int p = 0; p < P; ++p) acc = fmaf(a[base + (size_t)p * inner], yin[base + (size_t)p * inner], acc);
      for (int p = 0; p < P; ++p) {
        const size_t e = base + (size_t)p * inner;
        out[e] = cl ? inv * a[e] : inv * (a[e] - yin[e] * acc);
      }
    }
  }
}

template <bool BWD>
int l2norm_run(const float* a, const float* yin, const float* invin, float* out, float* invout, size_t outer, int P, int inner, hipStream_t s) {
  if (inner == 1) hipLaunchKernelGGL(l2norm_rows_kernel<BWD>, dim3(capped((outer + 3) / 4)), dim3(256), 0, s, a, yin, invin, out, invout, outer, P);
  else hipLaunchKernelGGL(l2norm_axis_kernel<BWD>, dim3(capped((outer * (size_t)inner + 255) / 256)), dim3(256), 0, s, a, yin, invin, out, invout, outer, P, inner);
  return check_launch(BWD ? "l2norm_bwd" : "l2norm_fwd");
}

bool l2_shape_ok(size_t outer, int P, int inner) {
  return P >= 1 && inner >= 1 && (uint64_t)P * (uint64_t)inner < 0x80000000ull && outer <= ((size_t)1 << 62) / ((size_t)P * (size_t)inner);
}

}  // namespace
}  // namespace gn

using namespace gn;

extern "C" {

int gn_bmm(const float* a, const float* b, float* c, int batch, int M, int N, int K, long long a_batch, long long a_m, long long a_k, long long b_batch,
           long long b_k, long long b_n, void* stream) {
  const BmmArgs g = {a, b, c, batch, M, N, K, a_batch, a_m, a_k, b_batch, b_k, b_n};
  const int rc = bmm_check("bmm", g);
  if (rc) return rc < 0 ? rc : GN_OK;
  return bmm_path(M, N) == BMM_THIN ? run_thin(g, (hipStream_t)stream) : run_mfma(g, (hipStream_t)stream);
}

int gn_bmm_valu(const float* a, const float* b, float* c, int batch, int M, int N, int K, long long a_batch, long long a_m, long long a_k, long long b_batch,
                long long b_k, long long b_n, void* stream) {
  const BmmArgs g = {a, b, c, batch, M, N, K, a_batch, a_m, a_k, b_batch, b_k, b_n};
  const int rc = bmm_check("bmm_valu", g);
  if (rc) return rc < 0 ? rc : GN_OK;
  const unsigned tm = cdiv(M, 16), tn = cdiv(N, 16);
  GN_REQUIRE((unsigned long long)tm * tn * (unsigned long long)batch < 0x80000000ull, "bmm_valu: %u x %u tiles x %d batch entries exceed the grid (2^31 - 1 blocks)",
             tm, tn, batch);
  hipLaunchKernelGGL(bmm_valu_kernel, dim3(tm * tn * (unsigned)batch), dim3(256), 0, (hipStream_t)stream, g, tm, tn);
  return check_launch("bmm_valu");
}

int gn_l2norm_fwd(const float* x, float* y, float* inv, size_t outer, int P, int inner, void* stream) {
  GN_REQUIRE(l2_shape_ok(outer, P, inner), "l2norm_fwd: bad shape (outer %zu, P %d, inner %d): P, inner >= 1, P * inner < 2^31, outer * P * inner < 2^62", outer, P,
             inner);
  if (!outer) return GN_OK;
  GN_REQUIRE(x && y && inv, "l2norm_fwd: null pointer");
  return l2norm_run<false>(x, nullptr, nullptr, y, inv, outer, P, inner, (hipStream_t)stream);
}

int gn_l2norm_bwd(const float* dy, const float* y, const float* inv, float* dx, size_t outer, int P, int inner, void* stream) {
  GN_REQUIRE(l2_shape_ok(outer, P, inner), "l2norm_bwd: bad shape (outer %zu, P %d, inner %d): P, inner >= 1, P * inner < 2^31, outer * P * inner < 2^62", outer, P,
             inner);
  if (!outer) return GN_OK;
  GN_REQUIRE(dy && y && inv && dx, "l2norm_bwd: null pointer");
  return l2norm_run<true>(dy, y, inv, dx, nullptr, outer, P, inner, (hipStream_t)stream);
}

}  // extern "C"
