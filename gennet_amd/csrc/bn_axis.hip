// BatchNormalization over an axis that is not the last one (keras BatchNormalization(axis=1) on (B, L, C): one parameter per position l).
//
// The tensor is viewed as (outer, P, inner): element (o, p, i) lives at (o*P + p)*inner + i, P the normalised axis, outer everything in
// front of it (the batch included), inner everything behind it.  A parameter p owns `outer` contiguous runs of `inner` floats, P*inner
// floats apart -- not the columns that colred_kernel (bn.hip) sums, and a different parameter index in the streaming passes.
// Four passes, no activation, no dropout mask, nothing fused:
//   stats      sums  = [sum x | sum x^2]         per p, fp64     4 bytes / element
//   apply      y     = fma(x, scale[p], shift[p])                 8 bytes / element
//   bwd_stats  dsums = [sum dy | sum dy*xhat]    per p, fp64     8 bytes / element
//   bwd_apply  dx    = gamma*invstd*(dy - dsum/n - xhat*dsum_xhat/n)   12 bytes / element
// inner % 4 == 0 (and 16-byte aligned tensors): float4 loads / stores -- every run starts 16-byte aligned and no float4 straddles two
// positions; otherwise scalar.  The two reductions keep a fixed summation order (per-lane fp64 pair in loop order, wave-64 shuffle tree,
// the four waves in wave order through LDS, one partial per block, colred_finalize over the chunks in order): no atomics, so two runs
// give identical bits.
#include "common.h"

namespace gn {
namespace {

template <int VEC>
__device__ __forceinline__ void load_v(const float* __restrict__ p, float (&v)[VEC]) {
  if constexpr (VEC == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
    v[0] = *p;
  }
}
template <int VEC>
__device__ __forceinline__ void store_v(float* __restrict__ p, const float (&v)[VEC]) {
  if constexpr (VEC == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  else *p = v[0];
}

// ---------------------------------------------------------------------------------------------
// reductions: block = (position p, chunk of o); its 256 lanes run over the flattened (o within the chunk, i) index in units of VEC floats,
// so consecutive lanes read consecutive addresses inside each run.  A lane steps its (o, i) pair by 256 units without dividing.
// MODE 1: a = x:  sum a, sum a^2.   MODE 2: a = dy:  sum a, sum a * xhat, xhat = (x - mean[p]) * invstd[p].
// part[(chunk*2 + v)*P + p]: the layout colred_finalize sums over chunks with n = 2P.
// ---------------------------------------------------------------------------------------------
template <int MODE, int VEC>
__global__ __launch_bounds__(256) void bn_axis_stats_kernel(const float* __restrict__ a, const float* __restrict__ x, const float* __restrict__ mean,
                                                            const float* __restrict__ invstd, double* __restrict__ part, size_t outer, int P, int inner,
                                                            size_t o_per_chunk) {
  constexpr int U = 4;                                     // units per trip, loads first
  const int p = (int)(blockIdx.x % (unsigned)P);
  const size_t chunk = blockIdx.x / (unsigned)P;
  const unsigned iv = (unsigned)inner / VEC;
  const size_t o_lo = chunk * o_per_chunk;
  const size_t o_hi = o_lo + o_per_chunk < outer ? o_lo + o_per_chunk : outer;
  const unsigned so = 256u / iv, si = 256u % iv;
  const unsigned tid = threadIdx.x;
  size_t o = o_lo + (size_t)(tid / iv);
  unsigned i = tid % iv;
  float mu = 0.f, is = 0.f;
  if (MODE == 2) { mu = mean[p]; is = invstd[p]; }
  const size_t row = (size_t)P * inner;                    // floats from (o, p, i) to (o + 1, p, i)
  const size_t base = (size_t)p * inner;
  double s0 = 0.0, s1 = 0.0;
  while (o < o_hi) {
    size_t off[U];
    bool ok[U];
    float av[U][VEC], xv[U][VEC];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      ok[u] = o < o_hi;
      off[u] = (ok[u] ? o : o_lo) * row + base + (size_t)(ok[u] ? i : 0u) * VEC;      // a lane past its end re-reads an address of the chunk
      i += si; o += so;
      if (i >= iv) { i -= iv; ++o; }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      load_v<VEC>(a + off[u], av[u]);
      if (MODE == 2) load_v<VEC>(x + off[u], xv[u]);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (!ok[u]) break;
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        const float v = av[u][e];
        s0 += (double)v;
        if (MODE == 1) {
          s1 += (double)v * (double)v;
        } else {
          const float xh = (xv[u][e] - mu) * is;
          s1 += (double)v * (double)xh;
        }
      }
    }
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    s0 += __shfl_down(s0, d, 64);
    s1 += __shfl_down(s1, d, 64);
  }
  __shared__ double red[2][4];
  if ((tid & 63) == 0) { red[0][tid >> 6] = s0; red[1][tid >> 6] = s1; }
  __syncthreads();
  if (tid == 0) {
    part[(chunk * 2 + 0) * P + p] = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
    part[(chunk * 2 + 1) * P + p] = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
  }
}

// ---------------------------------------------------------------------------------------------
// streaming passes: grid-stride over the nv = outer * P * inner / VEC units.  A thread's unit index advances by the grid's stride; its
// (p, i) pair advances by (stride mod P*inner/VEC) split into whole positions and a rest, with one carry and one wrap: no division in
// the loop, 32-bit ones in front of it.
// ---------------------------------------------------------------------------------------------
struct AxisPos {
  unsigned p, i, sp, si;                                   // unsigned: i + si and p + sp + 1 stay below 2^32 for P * inner < 2^31
};
__device__ __forceinline__ AxisPos axis_pos_init(int P, int iv) {
  const unsigned piv = (unsigned)P * (unsigned)iv;         // < 2^31 (checked by the launcher)
  const unsigned stride = gridDim.x * 256u;                // stream_grid: <= 2^19
  const unsigned r = (blockIdx.x * 256u + threadIdx.x) % piv, sm = stride % piv;
  AxisPos a;
  a.p = r / (unsigned)iv; a.i = r % (unsigned)iv;
  a.sp = sm / (unsigned)iv; a.si = sm % (unsigned)iv;
  return a;
}
__device__ __forceinline__ void axis_pos_step(AxisPos& a, int P, int iv) {
  a.i += a.si; a.p += a.sp;
  if (a.i >= (unsigned)iv) { a.i -= (unsigned)iv; ++a.p; }
  if (a.p >= (unsigned)P) a.p -= (unsigned)P;                                  // p <= P - 1, sp <= P - 1, one carry: below 2P
}

template <int VEC>
__global__ __launch_bounds__(256) void bn_axis_apply_kernel(const float* __restrict__ x, const float* __restrict__ scale, const float* __restrict__ shift,
                                                            float* __restrict__ y, size_t nv, int P, int iv) {
  AxisPos a = axis_pos_init(P, iv);
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < nv; idx += stride) {
    const float sc = scale[a.p], sh = shift[a.p];
    float v[VEC], o[VEC];
    load_v<VEC>(x + idx * VEC, v);
#pragma unroll
    for (int e = 0; e < VEC; ++e) o[e] = fmaf(v[e], sc, sh);
    store_v<VEC>(y + idx * VEC, o);
    axis_pos_step(a, P, iv);
  }
}

// per position, once: coef = [gamma*invstd | dsum/n | dsum_xhat/n] (fp32, the constants gn_bn_bwd_apply's float4 kernel keeps in registers)
// and the parameter gradients of this rank
__global__ void bn_axis_bwd_coef_kernel(const float* __restrict__ gamma, const float* __restrict__ invstd, const double* __restrict__ dsums_global, double count,
                                        const double* __restrict__ dsums_local, float* __restrict__ coef, float* __restrict__ dgamma, float* __restrict__ dbeta,
                                        int P) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  coef[p] = gamma[p] * invstd[p];
  coef[P + p] = (float)(dsums_global[p] / count);
  coef[2 * (size_t)P + p] = (float)(dsums_global[P + p] / count);
  dbeta[p] = (float)dsums_local[p];
  dgamma[p] = (float)dsums_local[P + p];
}

template <int VEC>
__global__ __launch_bounds__(256) void bn_axis_bwd_apply_kernel(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ mean,
                                                                const float* __restrict__ invstd, const float* __restrict__ coef, float* __restrict__ dx,
                                                                size_t nv, int P, int iv) {
  AxisPos a = axis_pos_init(P, iv);
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < nv; idx += stride) {
    const float mu = mean[a.p], is = invstd[a.p], gi = coef[a.p], mg = coef[P + a.p], mgx = coef[2 * (size_t)P + a.p];
    float g[VEC], v[VEC], o[VEC];
    load_v<VEC>(dy + idx * VEC, g);
    load_v<VEC>(x + idx * VEC, v);
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      const float xh = (v[e] - mu) * is;
      o[e] = gi * (g[e] - mg - xh * mgx);
    }
    store_v<VEC>(dx + idx * VEC, o);
    axis_pos_step(a, P, iv);
  }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// chunks of o per position: a few blocks per CU, near 2048 blocks in all, and at least ~1024 units (4 per lane) per block.  Decided by the
// shape alone (the workspace size depends on it), not by the alignment that picks float4 or scalar loads.
size_t axis_chunks(size_t outer, int P, int inner) {
  const size_t iv = inner % 4 == 0 ? inner / 4 : inner;
  size_t chunks = 2048 / (size_t)P;
  const size_t by_work = (outer * iv + 1023) / 1024;
  if (chunks > by_work) chunks = by_work;
  if (chunks > outer) chunks = outer;
  if (chunks < 1) chunks = 1;
  const size_t opc = (outer + chunks - 1) / chunks;
  return (outer + opc - 1) / opc;
}

bool shape_ok(size_t outer, int P, int inner) { return outer >= 1 && P >= 1 && inner >= 1 && (uint64_t)P * (uint64_t)inner < 0x80000000ull; }

// a = x (mode 1) or dy (mode 2)
int axis_reduce(int mode, const float* a, const float* x, const float* mean, const float* invstd, double* out, void* ws, size_t ws_bytes, size_t outer, int P,
                int inner, hipStream_t s) {
  const size_t chunks = axis_chunks(outer, P, inner);
  if (ws_bytes < chunks * 2 * (size_t)P * sizeof(double)) {
    set_error("bn_axis: workspace of %zu bytes, needs %zu", ws_bytes, chunks * 2 * (size_t)P * sizeof(double));
    return GN_EWORKSPACE;
  }
  const size_t opc = (outer + chunks - 1) / chunks;
  const bool v4 = inner % 4 == 0 && aligned16(a) && (mode == 1 || aligned16(x));
  double* part = (double*)ws;
  const dim3 grid((unsigned)(chunks * (size_t)P)), block(256);
  if (mode == 1) {
    if (v4) hipLaunchKernelGGL((bn_axis_stats_kernel<1, 4>), grid, block, 0, s, a, x, mean, invstd, part, outer, P, inner, opc);
    else hipLaunchKernelGGL((bn_axis_stats_kernel<1, 1>), grid, block, 0, s, a, x, mean, invstd, part, outer, P, inner, opc);
  } else {
    if (v4) hipLaunchKernelGGL((bn_axis_stats_kernel<2, 4>), grid, block, 0, s, a, x, mean, invstd, part, outer, P, inner, opc);
    else hipLaunchKernelGGL((bn_axis_stats_kernel<2, 1>), grid, block, 0, s, a, x, mean, invstd, part, outer, P, inner, opc);
  }
  const int rc = check_launch(mode == 1 ? "bn_axis_stats" : "bn_axis_bwd_stats");
  if (rc) return rc;
  return colred_finalize(part, out, 2 * (size_t)P, (int)chunks, s);
}

}  // namespace
}  // namespace gn

using namespace gn;

extern "C" {

size_t gn_bn_axis_stats_workspace(size_t outer, int P, int inner) {
  if (!shape_ok(outer, P, inner)) return 0;
  return axis_chunks(outer, P, inner) * 2 * (size_t)P * sizeof(double);
}

int gn_bn_axis_stats(const float* x, size_t outer, int P, int inner, double* sums, void* ws, size_t ws_bytes, void* stream) {
  GN_REQUIRE(x && sums && ws, "bn_axis_stats: null pointer");
  GN_REQUIRE(shape_ok(outer, P, inner), "bn_axis_stats: bad shape (outer %zu, P %d, inner %d): all >= 1 and P * inner < 2^31", outer, P, inner);
  return axis_reduce(1, x, nullptr, nullptr, nullptr, sums, ws, ws_bytes, outer, P, inner, (hipStream_t)stream);
}

int gn_bn_axis_apply(const float* x, const float* scale, const float* shift, float* y, size_t outer, int P, int inner, void* stream) {
  GN_REQUIRE(x && scale && shift && y, "bn_axis_apply: null pointer");
  GN_REQUIRE(shape_ok(outer, P, inner), "bn_axis_apply: bad shape (outer %zu, P %d, inner %d): all >= 1 and P * inner < 2^31", outer, P, inner);
  const bool v4 = inner % 4 == 0 && aligned16(x) && aligned16(y);
  const int iv = v4 ? inner / 4 : inner;
  const size_t nv = outer * (size_t)P * iv;
  if (v4) hipLaunchKernelGGL(bn_axis_apply_kernel<4>, dim3(stream_grid(nv)), dim3(256), 0, (hipStream_t)stream, x, scale, shift, y, nv, P, iv);
  else hipLaunchKernelGGL(bn_axis_apply_kernel<1>, dim3(stream_grid(nv)), dim3(256), 0, (hipStream_t)stream, x, scale, shift, y, nv, P, iv);
  return check_launch("bn_axis_apply");
}

int gn_bn_axis_bwd_stats(const float* dy, const float* x, const float* save_mean, const float* save_invstd, double* dsums, void* ws, size_t ws_bytes,
                         size_t outer, int P, int inner, void* stream) {
  GN_REQUIRE(dy && x && save_mean && save_invstd && dsums && ws, "bn_axis_bwd_stats: null pointer");
  GN_REQUIRE(shape_ok(outer, P, inner), "bn_axis_bwd_stats: bad shape (outer %zu, P %d, inner %d): all >= 1 and P * inner < 2^31", outer, P, inner);
  return axis_reduce(2, dy, x, save_mean, save_invstd, dsums, ws, ws_bytes, outer, P, inner, (hipStream_t)stream);
}

int gn_bn_axis_bwd_apply(const float* dy, const float* x, const float* gamma, const float* save_mean, const float* save_invstd, const double* dsums_global,
                         double count, const double* dsums_local, float* dx, float* dgamma, float* dbeta, void* ws, size_t ws_bytes, size_t outer, int P,
                         int inner, void* stream) {
  GN_REQUIRE(dy && x && gamma && save_mean && save_invstd && dsums_global && dsums_local && dx && dgamma && dbeta && ws, "bn_axis_bwd_apply: null pointer");
  GN_REQUIRE(shape_ok(outer, P, inner), "bn_axis_bwd_apply: bad shape (outer %zu, P %d, inner %d): all >= 1 and P * inner < 2^31", outer, P, inner);
  GN_REQUIRE(count >= 1.0, "bn_axis_bwd_apply: count %g", count);
  if (ws_bytes < 3 * (size_t)P * sizeof(float)) {
    set_error("bn_axis_bwd_apply: workspace of %zu bytes, needs %zu", ws_bytes, 3 * (size_t)P * sizeof(float));
    return GN_EWORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  float* coef = (float*)ws;
  hipLaunchKernelGGL(bn_axis_bwd_coef_kernel, dim3(cdiv(P, 256)), dim3(256), 0, s, gamma, save_invstd, dsums_global, count, dsums_local, coef, dgamma, dbeta, P);
  const int rc = check_launch("bn_axis_bwd_coef");
  if (rc) return rc;
  const bool v4 = inner % 4 == 0 && aligned16(dy) && aligned16(x) && aligned16(dx);
  const int iv = v4 ? inner / 4 : inner;
  const size_t nv = outer * (size_t)P * iv;
  if (v4) hipLaunchKernelGGL(bn_axis_bwd_apply_kernel<4>, dim3(stream_grid(nv)), dim3(256), 0, s, dy, x, save_mean, save_invstd, coef, dx, nv, P, iv);
  else hipLaunchKernelGGL(bn_axis_bwd_apply_kernel<1>, dim3(stream_grid(nv)), dim3(256), 0, s, dy, x, save_mean, save_invstd, coef, dx, nv, P, iv);
  return check_launch("bn_axis_bwd_apply");
}

}  // extern "C"
