// The Keras 2.2.4 losses (losses.py, TensorFlow backend) and their metric forms as ONE streaming pass over an output of any size:
// out[0] = sum over rows of the per-row term / denom, out[1] = #elements with round(p) == y, dp = d out[0] / dp (optional).
//
//  * element-wise kinds (every loss that is a mean, or for kullback_leibler_divergence a sum, of per-element terms): the grid scales with
//    rows * cols, a block owns a contiguous share whose start is a multiple of four elements, reads p, y and writes dp as float4 where the
//    three pointers share one 16-byte phase (scalar head / tail around it, all-scalar when they do not), and reduces its share to two fp64
//    partials [term sum, hits] in the workspace with plain stores;
//  * row-wise kinds (categorical_crossentropy, cosine_proximity, categorical_accuracy need sums over a row before a gradient exists): one
//    wave (cols <= 256) or one block owns a row, reduces the row sums, then sweeps the row again for dp; a group walks a contiguous range of
//    rows, so the partial count stays bounded;
//  * a second kernel of one block adds the partials in a fixed order and writes out.  No atomics anywhere: two runs give the same bits, and
//    the launch shape depends on (rows, cols) only.
//
// HBM-bound (12 bytes per element with dp, 8 without), so the arithmetic is done in fp64 on the fp32 inputs and dp is rounded to fp32 once:
// the terms that cancel (logcosh near d = 0, the log difference of mean_squared_logarithmic_error) keep their digits on any input, at no cost
// in time.  The clip bounds are the fp32 numbers Keras computes (eps = 1e-7f, 1 - eps in fp32).
// Conventions (TensorFlow's gradients): a clip passes gradient on its CLOSED interval; maximum(a, 0) gives a tie to a; sign(0) = 0.
//
// The WEIGHTED form (Keras' sample_weight) is the same pass with one weight per row and a normaliser read from device
// memory: out[0] = sum_r w_r l_r / count, out[2] = sum_r w_r hits_r / (count cols), dp scaled by w_r / count.  count = #{w != 0} comes from
// gn_weight_count (all-reduced between the two under data parallelism), so nothing of it is a by-value argument and a captured step replays
// with new weights.  Both forms are instantiations of one body (template parameter W); the unweighted kernels keep their signatures and code.
// An element of the element-wise kernels finds its row without a division in the loop: (row, column) once per thread from its first index,
// then add-and-carry, per element of a float4 and per sweep; with cols == 1 the row is the index and w is a third float4 stream.
#include "common.h"

namespace gn {

static constexpr int LOSS_MAX_BLOCKS = 2048;      // 8 blocks of 256 per CU, as stream_grid
static constexpr int LOSS_WAVE_COLS = 256;        // rows up to this length are owned by one wave, longer ones by a block

__device__ __forceinline__ double loss_eps() { return (double)1e-7f; }
__device__ __forceinline__ double loss_one_minus_eps() { return (double)(1.f - 1e-7f); }

// per-element term t and its derivative g = dt/dp (before the division by cols and denom)
template <int K>
__device__ __forceinline__ void loss_term(float pf, float yf, double& t, double& g) {
  const double p = (double)pf, y = (double)yf, d = p - y, eps = loss_eps();
  if (K == GN_LOSS_BINARY_CROSSENTROPY) {        // as loss_kernel<0> (below): TF's sigmoid cross-entropy on the logit of the clipped p
    const double pc = fmin(fmax(p, eps), loss_one_minus_eps());
    const double z = log(pc / (1.0 - pc));
    t = fmax(z, 0.0) - z * y + log1p(exp(-fabs(z)));
    const bool inside = (p >= eps) && (p <= loss_one_minus_eps());
    const double sg = 1.0 / (1.0 + exp(-z));
    g = inside ? (sg - y) / (pc * (1.0 - pc)) : 0.0;
  } else if (K == GN_LOSS_MEAN_SQUARED_ERROR) {
    t = d * d;
    g = 2.0 * d;
  } else if (K == GN_LOSS_MEAN_ABSOLUTE_ERROR) {
    t = fabs(d);
    g = d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : 0.0);
  } else if (K == GN_LOSS_MEAN_ABSOLUTE_PERCENTAGE_ERROR) {
    const double m = fmax(fabs(y), eps);
    t = 100.0 * fabs(d) / m;
    g = d > 0.0 ? 100.0 / m : (d < 0.0 ? -100.0 / m : 0.0);
  } else if (K == GN_LOSS_MEAN_SQUARED_LOGARITHMIC_ERROR) {
    const double pm = fmax(p, eps), ym = fmax(y, eps);
    const double l = log1p(pm) - log1p(ym);
    t = l * l;
    g = p >= eps ? 2.0 * l / (pm + 1.0) : 0.0;
  } else if (K == GN_LOSS_HINGE) {
    const double m = 1.0 - y * p;
    t = fmax(m, 0.0);
    g = m >= 0.0 ? -y : 0.0;
  } else if (K == GN_LOSS_SQUARED_HINGE) {
    const double h = fmax(1.0 - y * p, 0.0);
    t = h * h;
    g = -2.0 * y * h;
  } else if (K == GN_LOSS_LOGCOSH) {               // d + softplus(-2d) - log 2 = |d| + log1p(exp(-2|d|)) - log 2; tanh from the same exponential
    const double a = fabs(d), e = exp(-2.0 * a);
    t = a + log1p(e) - 0.69314718055994530942;
    const double th = (1.0 - e) / (1.0 + e);
    g = d < 0.0 ? -th : th;
  } else if (K == GN_LOSS_POISSON) {
    t = p - y * log(p + eps);
    g = 1.0 - y / (p + eps);
  } else {                                         // GN_LOSS_KULLBACK_LEIBLER_DIVERGENCE
    const double yc = fmin(fmax(y, eps), 1.0), pc = fmin(fmax(p, eps), 1.0);
    t = yc * log(yc / pc);
    g = (p >= eps && p <= 1.0) ? -yc / pc : 0.0;
  }
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// a block's [term sum, hits] into its two workspace slots: wave butterflies, then the four wave sums in order.  W: a third slot, the weighted hits
template <bool W>
__device__ __forceinline__ void loss_block_partial(double acc, unsigned hits, double whits, double* __restrict__ partials) {
  __shared__ double red[W ? 12 : 8];
  constexpr int S = W ? 3 : 2;
  acc = wave_sum(acc);
  const double h = wave_sum((double)hits);
  if (W) whits = wave_sum(whits);
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6] = acc; red[4 + (threadIdx.x >> 6)] = h;
    if (W) red[8 + (threadIdx.x >> 6)] = whits;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    partials[S * (size_t)blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
    partials[S * (size_t)blockIdx.x + 1] = ((red[4] + red[5]) + red[6]) + red[7];
    if (W) partials[S * (size_t)blockIdx.x + 2] = ((red[8] + red[9]) + red[10]) + red[11];
  }
}

// What the weighted kernels take beyond the unweighted ones.  q4 / r4 and q1 / r1: quotient and remainder of the two sweep strides (1024
// elements of the float4 loop, 256 of the scalar loop) by cols, for the add-and-carry of (row, column); wvec: w shares the phase of p, y, dp
// (cols == 1 only: there the row is the element index and w is read as float4 beside them).
struct LossWeights {
  const float* w;
  const double* count;
  int cols, r4, r1, wvec;
  long long q4, q1;
};

__device__ __forceinline__ LossWeights loss_weights() { return LossWeights(); }
__device__ __forceinline__ LossWeights loss_weights(const LossWeights& lw) { return lw; }
__device__ __forceinline__ double hit(float pf, float yf) { return rintf(pf) == yf ? 1.0 : 0.0; }

// mis: the common phase of p, y, dp inside a 16-byte line in elements (0..3), or -1 when they differ (all-scalar).  share % 4 == 0.
// The weighted form is the instantiation with one more kernel argument, a LossWeights (LW = {LossWeights}, and gscale is then the column
// divisor: cols, or 1 for the kind that sums over a row); the unweighted one (LW = {}) has the arguments and the code it always had, which
// is why the body is the kernel itself and not a function both call: inlining one changes the unweighted code.  C1: cols == 1 (weighted only).
template <int K, bool GRAD, bool C1, class... LW>
__global__ __launch_bounds__(256) void loss_elem_kernel(const float* __restrict__ p, const float* __restrict__ y, float* __restrict__ dp, size_t n, size_t share,
                                                        int mis, double gscale, double* __restrict__ partials, LW... lwp) {
  constexpr bool W = sizeof...(LW) != 0;
  const LossWeights lw = loss_weights(lwp...);
  const size_t a = (size_t)blockIdx.x * share;
  const size_t b = a + share < n ? a + share : n;
  size_t v0 = b, v1 = b;                           // [a, v0) scalar, [v0, v1) float4, [v1, b) scalar
  if (mis >= 0) {
    v0 = a + (size_t)((4 - mis) & 3);
    if (v0 > b) v0 = b;
    v1 = v0 + ((b - v0) & ~(size_t)3);
  }
  double acc = 0.0, whits = 0.0;
  unsigned hits = 0;
  const float* w = W ? lw.w : nullptr;
  const int cols = W ? lw.cols : 1;
  if (W) gscale = 1.0 / (*lw.count * gscale);
  size_t row = 0;
  int col = 0;
  if (W && !C1) {
    const size_t i0 = v0 + 4 * (size_t)threadIdx.x;
    row = i0 / (size_t)cols;
    col = (int)(i0 - row * (size_t)cols);
  }
  for (size_t i = v0 + 4 * (size_t)threadIdx.x; i < v1; i += 1024) {
    const float4 pv = *reinterpret_cast<const float4*>(p + i), yv = *reinterpret_cast<const float4*>(y + i);
    double t0, t1, t2, t3, g0, g1, g2, g3;
    loss_term<K>(pv.x, yv.x, t0, g0);
    loss_term<K>(pv.y, yv.y, t1, g1);
    loss_term<K>(pv.z, yv.z, t2, g2);
    loss_term<K>(pv.w, yv.w, t3, g3);
    if (W) {
      double w0, w1, w2, w3;
      if (C1) {
        if (lw.wvec) {
          const float4 wv = *reinterpret_cast<const float4*>(w + i);
          w0 = (double)wv.x; w1 = (double)wv.y; w2 = (double)wv.z; w3 = (double)wv.w;
        } else {
          w0 = (double)w[i]; w1 = (double)w[i + 1]; w2 = (double)w[i + 2]; w3 = (double)w[i + 3];
        }
      } else {                                     // the four elements' rows by add-and-carry: a float4 may straddle rows (cols 2, 3: up to three)
        size_t rr = row;
        int cc = col;
        w0 = (double)w[rr];
        if (++cc == cols) { cc = 0; ++rr; }
        w1 = (double)w[rr];
        if (++cc == cols) { cc = 0; ++rr; }
        w2 = (double)w[rr];
        if (++cc == cols) { cc = 0; ++rr; }
        w3 = (double)w[rr];
        row += (size_t)lw.q4;                      // the next sweep, 1024 elements on
        col += lw.r4;
        if (col >= cols) { col -= cols; ++row; }
      }
      acc += (w0 * t0 + w1 * t1) + (w2 * t2 + w3 * t3);
      whits += (w0 * hit(pv.x, yv.x) + w1 * hit(pv.y, yv.y)) + (w2 * hit(pv.z, yv.z) + w3 * hit(pv.w, yv.w));
      g0 *= w0; g1 *= w1; g2 *= w2; g3 *= w3;
    } else {
      acc += (t0 + t1) + (t2 + t3);
    }
    hits += (rintf(pv.x) == yv.x) + (rintf(pv.y) == yv.y) + (rintf(pv.z) == yv.z) + (rintf(pv.w) == yv.w);
    if (GRAD) *reinterpret_cast<float4*>(dp + i) = make_float4((float)(g0 * gscale), (float)(g1 * gscale), (float)(g2 * gscale), (float)(g3 * gscale));
  }
  const size_t nscal = (v0 - a) + (b - v1);
  // weighted: with mis >= 0 at most six scalar elements exist, one per thread; with mis < 0 the index advances by exactly 256 per sweep.  Either
  // way one division per thread, at its first element
  bool first = true;
  for (size_t r = threadIdx.x; r < nscal; r += 256) {
    const size_t i = r < v0 - a ? a + r : v1 + (r - (v0 - a));
    const float pf = p[i], yf = y[i];
    double t, g;
    loss_term<K>(pf, yf, t, g);
    if (W) {
      if (C1) {
        row = i;
      } else if (first) {
        row = i / (size_t)cols;
        col = (int)(i - row * (size_t)cols);
        first = false;
      } else {
        row += (size_t)lw.q1;
        col += lw.r1;
        if (col >= cols) { col -= cols; ++row; }
      }
      const double wr = (double)w[row];
      acc += wr * t;
      whits += wr * hit(pf, yf);
      g *= wr;
    } else {
      acc += t;
    }
    hits += rintf(pf) == yf;
    if (GRAD) dp[i] = (float)(g * gscale);
  }
  loss_block_partial<W>(acc, hits, whits, partials);
}

// sum over the owning group (a wave, or the block of four waves) of a row; every lane receives it
__device__ __forceinline__ double group_sum(double v, bool wave, double* red) {
  v = wave_sum(v);
  if (wave) return v;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// the FIRST position of the maximum of a row: larger value wins, equal values give the smaller index
__device__ __forceinline__ void argmax_merge(float& v, int& i, float ov, int oi) {
  if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}
__device__ __forceinline__ int group_argmax(float v, int i, bool wave, float* redv, int* redi) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const float ov = __shfl_xor(v, o, 64);
    const int oi = __shfl_xor(i, o, 64);
    argmax_merge(v, i, ov, oi);
  }
  if (wave) return i;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) { redv[threadIdx.x >> 6] = v; redi[threadIdx.x >> 6] = i; }
  __syncthreads();
  v = redv[0]; i = redi[0];
  for (int w = 1; w < 4; ++w) argmax_merge(v, i, redv[w], redi[w]);
  return i;
}

// Group g (wave g of the grid when `wave`, block g otherwise) owns rows [g * rpg, (g + 1) * rpg).  In block form the row loop is uniform
// over the block, so the barriers inside group_sum are reached by all of it; the wave form uses none before the final partial.
// W: the row's term, its hits and its gradient are scaled by w[r]; gscale is formed from the device count.
template <int K, bool GRAD, bool W>
__device__ __forceinline__ void loss_row_body(const float* p, const float* y, float* dp, long long rows, int cols,
                                              long long rpg, int wave_i, double gscale, double* partials, const float* w,
                                              const double* count) {
  __shared__ double red[4];
  __shared__ float redv[4];
  __shared__ int redi[4];
  const bool wave = wave_i != 0;
  const int lane = wave ? (threadIdx.x & 63) : threadIdx.x, G = wave ? 64 : 256;
  const long long gid = wave ? (long long)blockIdx.x * 4 + (threadIdx.x >> 6) : (long long)blockIdx.x;
  const long long r0 = gid * rpg, r1 = r0 + rpg < rows ? r0 + rpg : rows;
  const double eps = loss_eps(), hi = loss_one_minus_eps();
  double acc = 0.0, whits = 0.0;
  unsigned hits = 0;
  const double gbase = W ? 1.0 / *count : gscale;
  for (long long r = r0; r < r1; ++r) {
    const float* pr = p + (size_t)r * cols;
    const float* yr = y + (size_t)r * cols;
    float* dr = GRAD ? dp + (size_t)r * cols : nullptr;
    const double wr = W ? (double)w[r] : 1.0;
    const unsigned hits0 = hits;
    if (W) gscale = wr * gbase;
    if (K == GN_LOSS_CATEGORICAL_CROSSENTROPY) {
      double s = 0.0;
      for (int j = lane; j < cols; j += G) {
        const float pf = pr[j];
        s += (double)pf;
        hits += rintf(pf) == yr[j];
      }
      const double S = group_sum(s, wave, red);
      double t = 0.0, gq = 0.0;
      for (int j = lane; j < cols; j += G) {
        const double q = (double)pr[j] / S, yv = (double)yr[j];
        const double qc = fmin(fmax(q, eps), hi);
        t -= yv * log(qc);
        if (q >= eps && q <= hi) gq += -yv / qc * q;
      }
      const double T = group_sum(t, wave, red), GQ = group_sum(gq, wave, red);
      if (lane == 0) acc += W ? wr * T : T;
      if (GRAD)
        for (int j = lane; j < cols; j += G) {
          const double q = (double)pr[j] / S, yv = (double)yr[j];
          const double gk = (q >= eps && q <= hi) ? -yv / q : 0.0;
          dr[j] = (float)((gk - GQ) / S * gscale);
        }
    } else if (K == GN_LOSS_COSINE_PROXIMITY) {
      double spp = 0.0, syy = 0.0, spy = 0.0;
      for (int j = lane; j < cols; j += G) {
        const float pf = pr[j], yf = yr[j];
        const double pv = (double)pf, yv = (double)yf;
        spp += pv * pv; syy += yv * yv; spy += pv * yv;
        hits += rintf(pf) == yf;
      }
      const double SPP = group_sum(spp, wave, red), SYY = group_sum(syy, wave, red), SPY = group_sum(spy, wave, red);
      const double np = sqrt(fmax(SPP, 1e-12)), ny = sqrt(fmax(SYY, 1e-12));
      const double c = SPY / (np * ny);
      if (lane == 0) acc -= W ? wr * c : c;
      if (GRAD) {
        const double cc = SPP >= 1e-12 ? c : 0.0;                  // below the floor the norm is a constant: only the y-hat term is left
        for (int j = lane; j < cols; j += G)
          dr[j] = (float)(-((double)yr[j] / ny - cc * ((double)pr[j] / np)) / np * gscale);
      }
    } else {                                       // GN_LOSS_CATEGORICAL_ACCURACY: 1 where the first arg-max of p is the first arg-max of y
      float bp = -INFINITY, by = -INFINITY;
      int ip = 0x7fffffff, iy = 0x7fffffff;
      for (int j = lane; j < cols; j += G) {
        const float pf = pr[j], yf = yr[j];
        if (pf > bp) { bp = pf; ip = j; }
        if (yf > by) { by = yf; iy = j; }
        hits += rintf(pf) == yf;
        if (GRAD) dr[j] = 0.f;
      }
      ip = group_argmax(bp, ip, wave, redv, redi);
      iy = group_argmax(by, iy, wave, redv, redi);
      if (lane == 0 && ip == iy) acc += W ? wr : 1.0;
    }
    if (W) whits += wr * (double)(hits - hits0);
  }
  loss_block_partial<W>(acc, hits, whits, partials);
}

template <int K, bool GRAD>
__global__ __launch_bounds__(256) void loss_row_kernel(const float* __restrict__ p, const float* __restrict__ y, float* __restrict__ dp, long long rows, int cols,
                                                       long long rpg, int wave_i, double gscale, double* __restrict__ partials) {
  loss_row_body<K, GRAD, false>(p, y, dp, rows, cols, rpg, wave_i, gscale, partials, nullptr, nullptr);
}

template <int K, bool GRAD>
__global__ __launch_bounds__(256) void loss_row_weighted_kernel(const float* __restrict__ p, const float* __restrict__ y, float* __restrict__ dp, long long rows,
                                                                int cols, long long rpg, int wave_i, const float* __restrict__ w,
                                                                const double* __restrict__ count, double* __restrict__ partials) {
  loss_row_body<K, GRAD, true>(p, y, dp, rows, cols, rpg, wave_i, 0.0, partials, w, count);
}

// one block: the partials in a fixed order (strided per thread, wave butterfly, four wave sums), then the division
__global__ __launch_bounds__(256) void loss_finish_kernel(const double* __restrict__ partials, int count, double div, float* __restrict__ out) {
  __shared__ double red[8];
  double acc = 0.0, h = 0.0;
  for (int i = threadIdx.x; i < count; i += 256) { acc += partials[2 * i]; h += partials[2 * i + 1]; }
  acc = wave_sum(acc);
  h = wave_sum(h);
  if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = acc; red[4 + (threadIdx.x >> 6)] = h; }
  __syncthreads();
  if (threadIdx.x == 0) {
    out[0] = (float)((((red[0] + red[1]) + red[2]) + red[3]) / div);
    out[1] = (float)(((red[4] + red[5]) + red[6]) + red[7]);
  }
}

// the weighted finish: three partials per block, the divisions by the device count.  0 / 0 (every weight zero) is NaN, as in Keras
__global__ __launch_bounds__(256) void loss_finish_weighted_kernel(const double* __restrict__ partials, int nparts, const double* __restrict__ count, double coldiv,
                                                                   double cols, float* __restrict__ out) {
  __shared__ double red[12];
  double acc = 0.0, h = 0.0, wh = 0.0;
  for (int i = threadIdx.x; i < nparts; i += 256) { acc += partials[3 * i]; h += partials[3 * i + 1]; wh += partials[3 * i + 2]; }
  acc = wave_sum(acc);
  h = wave_sum(h);
  wh = wave_sum(wh);
  if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = acc; red[4 + (threadIdx.x >> 6)] = h; red[8 + (threadIdx.x >> 6)] = wh; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double c = *count;
    out[0] = (float)((((red[0] + red[1]) + red[2]) + red[3]) / (c * coldiv));
    out[1] = (float)(((red[4] + red[5]) + red[6]) + red[7]);
    out[2] = (float)((((red[8] + red[9]) + red[10]) + red[11]) / (c * cols));
  }
}

// #{w != 0}: a block counts a contiguous share of the rows (integers, so the order of the sum cannot matter; it is fixed all the same);
// one block writes the count itself, more leave 64-bit partials for the one-block finish
static constexpr long long COUNT_ROWS_PER_BLOCK = 4096;
static constexpr int COUNT_MAX_BLOCKS = 1024;

__device__ __forceinline__ unsigned long long block_count(unsigned long long c) {
  __shared__ unsigned long long redc[4];
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) c += __shfl_xor(c, o, 64);
  if ((threadIdx.x & 63) == 0) redc[threadIdx.x >> 6] = c;
  __syncthreads();
  return ((redc[0] + redc[1]) + redc[2]) + redc[3];
}
__global__ __launch_bounds__(256) void weight_count_kernel(const float* __restrict__ w, long long rows, long long share, unsigned long long* __restrict__ partials,
                                                           double* __restrict__ count) {
  const long long a = (long long)blockIdx.x * share, b = a + share < rows ? a + share : rows;
  unsigned long long c = 0;
  for (long long r = a + threadIdx.x; r < b; r += 256) c += w[r] != 0.f;
  c = block_count(c);
  if (threadIdx.x == 0) {
    if (gridDim.x == 1) *count = (double)c;
    else partials[blockIdx.x] = c;
  }
}
__global__ __launch_bounds__(256) void weight_count_finish_kernel(const unsigned long long* __restrict__ partials, int nparts, double* __restrict__ count) {
  unsigned long long c = 0;
  for (int i = threadIdx.x; i < nparts; i += 256) c += partials[i];
  c = block_count(c);
  if (threadIdx.x == 0) *count = (double)c;
}
static void count_shape(long long rows, unsigned& blocks, long long& share) {
  long long nb = (rows + COUNT_ROWS_PER_BLOCK - 1) / COUNT_ROWS_PER_BLOCK;
  if (nb > COUNT_MAX_BLOCKS) nb = COUNT_MAX_BLOCKS;
  share = (rows + nb - 1) / nb;
  blocks = (unsigned)((rows + share - 1) / share);
}

static bool loss_rowwise(int kind) {
  return kind == GN_LOSS_CATEGORICAL_CROSSENTROPY || kind == GN_LOSS_COSINE_PROXIMITY || kind == GN_LOSS_CATEGORICAL_ACCURACY;
}

// launch shape: a function of (rows, cols) and the kind's form alone
struct LossShape {
  unsigned blocks;
  size_t share;          // element-wise: elements per block (a multiple of 4)
  long long rpg;         // row-wise: rows per group
  int wave;              // row-wise: 1 = a wave owns a row
};
static LossShape loss_shape(bool rowwise, long long rows, int cols) {
  LossShape s = {1, 0, 0, 0};
  if (!rowwise) {
    const size_t n = (size_t)rows * (size_t)cols;
    size_t nb = (n + 1023) / 1024;
    if (nb > (size_t)LOSS_MAX_BLOCKS) nb = LOSS_MAX_BLOCKS;
    s.share = (((n + nb - 1) / nb) + 3) & ~(size_t)3;
    s.blocks = (unsigned)((n + s.share - 1) / s.share);
  } else {
    s.wave = cols <= LOSS_WAVE_COLS ? 1 : 0;
    const long long gpb = s.wave ? 4 : 1;
    long long nb = (rows + gpb - 1) / gpb;
    if (nb > LOSS_MAX_BLOCKS) nb = LOSS_MAX_BLOCKS;
    s.rpg = (rows + nb * gpb - 1) / (nb * gpb);
    s.blocks = (unsigned)((rows + s.rpg * gpb - 1) / (s.rpg * gpb));
  }
  return s;
}

template <int K>
static void loss_launch_elem(const LossShape& sh, const float* p, const float* y, float* dp, size_t n, int mis, double gscale, double* partials, hipStream_t s) {
  if (dp) hipLaunchKernelGGL((loss_elem_kernel<K, true, false>), dim3(sh.blocks), dim3(256), 0, s, p, y, dp, n, sh.share, mis, gscale, partials);
  else hipLaunchKernelGGL((loss_elem_kernel<K, false, false>), dim3(sh.blocks), dim3(256), 0, s, p, y, dp, n, sh.share, mis, gscale, partials);
}
template <int K>
static void loss_launch_row(const LossShape& sh, const float* p, const float* y, float* dp, long long rows, int cols, double gscale, double* partials, hipStream_t s) {
  if (dp) hipLaunchKernelGGL((loss_row_kernel<K, true>), dim3(sh.blocks), dim3(256), 0, s, p, y, dp, rows, cols, sh.rpg, sh.wave, gscale, partials);
  else hipLaunchKernelGGL((loss_row_kernel<K, false>), dim3(sh.blocks), dim3(256), 0, s, p, y, dp, rows, cols, sh.rpg, sh.wave, gscale, partials);
}
template <int K>
static void loss_launch_elem_weighted(const LossShape& sh, const float* p, const float* y, float* dp, size_t n, int mis, double coldiv, double* partials,
                                      const LossWeights& lw, hipStream_t s) {
#define GN_LOSS_W(G, C) hipLaunchKernelGGL((loss_elem_kernel<K, G, C, LossWeights>), dim3(sh.blocks), dim3(256), 0, s, p, y, dp, n, sh.share, mis, coldiv, partials, lw)
  if (lw.cols == 1) { if (dp) GN_LOSS_W(true, true); else GN_LOSS_W(false, true); }
  else { if (dp) GN_LOSS_W(true, false); else GN_LOSS_W(false, false); }
#undef GN_LOSS_W
}
template <int K>
static void loss_launch_row_weighted(const LossShape& sh, const float* p, const float* y, float* dp, long long rows, int cols, const float* w, const double* count,
                                     double* partials, hipStream_t s) {
  if (dp) hipLaunchKernelGGL((loss_row_weighted_kernel<K, true>), dim3(sh.blocks), dim3(256), 0, s, p, y, dp, rows, cols, sh.rpg, sh.wave, w, count, partials);
  else hipLaunchKernelGGL((loss_row_weighted_kernel<K, false>), dim3(sh.blocks), dim3(256), 0, s, p, y, dp, rows, cols, sh.rpg, sh.wave, w, count, partials);
}

// ---------------------------------------------------------------------------------------------
// the original BCE / MSE losses on a (B, 1) output: single block (B is a batch size, a few thousand at most).  Kept beside the pass above
// for their bits: ops.LOSS_PASS_MIN_ELEMENTS routes small batches here
// ---------------------------------------------------------------------------------------------
template <int KIND>  // 0 = BCE, 1 = MSE
__global__ __launch_bounds__(256) void loss_kernel(const float* __restrict__ p, const float* __restrict__ y, float* __restrict__ dp, float* __restrict__ out,
                                                   int B, int Bglobal) {
  const float eps = 1e-7f;
  float lsum = 0.f, hits = 0.f;
  for (int i = threadIdx.x; i < B; i += 256) {
    const float pv = p[i], yv = y[i];
    if (KIND == 0) {
      const float pc = fminf(fmaxf(pv, eps), 1.f - eps);
      const float z = logf(pc / (1.f - pc));
      lsum += fmaxf(z, 0.f) - z * yv + log1pf(expf(-fabsf(z)));
      const bool inside = (pv >= eps) && (pv <= 1.f - eps);
      const float sg = 1.f / (1.f + expf(-z));
      dp[i] = inside ? (sg - yv) / (pc * (1.f - pc)) / (float)Bglobal : 0.f;
    } else {
      const float d = pv - yv;
      lsum += d * d;
      dp[i] = 2.f * d / (float)Bglobal;
    }
    hits += (rintf(pv) == yv) ? 1.f : 0.f;
  }
  __shared__ float r0[256], r1[256];
  r0[threadIdx.x] = lsum; r1[threadIdx.x] = hits;
  __syncthreads();
  for (int sft = 128; sft >= 1; sft >>= 1) {
    if (threadIdx.x < sft) { r0[threadIdx.x] += r0[threadIdx.x + sft]; r1[threadIdx.x] += r1[threadIdx.x + sft]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) { out[0] = r0[0] / (float)Bglobal; out[1] = r1[0]; }
}
static int loss_run(int kind, const float* p, const float* y, float* dp, float* out, int B, int Bglobal, hipStream_t s) {
  GN_REQUIRE(B >= 1 && Bglobal >= B, "loss: bad batch sizes %d / %d", B, Bglobal);
  if (kind == 0) hipLaunchKernelGGL(loss_kernel<0>, dim3(1), dim3(256), 0, s, p, y, dp, out, B, Bglobal);
  else hipLaunchKernelGGL(loss_kernel<1>, dim3(1), dim3(256), 0, s, p, y, dp, out, B, Bglobal);
  return check_launch("loss");
}

}  // namespace gn

extern "C" size_t gn_loss_pass_workspace(long long rows, int cols) {
  if (rows < 1 || cols < 1) return 0;
  const unsigned a = gn::loss_shape(false, rows, cols).blocks, b = gn::loss_shape(true, rows, cols).blocks;
  return (size_t)(a > b ? a : b) * 2 * sizeof(double);
}

extern "C" int gn_loss_pass(int kind, const float* p, const float* y, float* dp, float* out, long long rows, int cols, double denom, void* ws, size_t ws_bytes,
                            void* stream) {
  using namespace gn;
  GN_REQUIRE(kind >= 0 && kind < GN_LOSS_KINDS, "loss_pass: unknown kind %d", kind);
  GN_REQUIRE(p && y && out, "loss_pass: null pointer");
  GN_REQUIRE(rows >= 1 && cols >= 1, "loss_pass: bad shape (%lld, %d)", rows, cols);
  GN_REQUIRE(denom >= (double)rows, "loss_pass: denom %g is below the %lld local rows", denom, rows);
  GN_REQUIRE(ws && ws_bytes >= gn_loss_pass_workspace(rows, cols) && ((uintptr_t)ws & 7) == 0, "loss_pass: workspace of %zu bytes, %zu needed (8-byte aligned)",
             ws_bytes, gn_loss_pass_workspace(rows, cols));
  hipStream_t s = (hipStream_t)stream;
  double* partials = (double*)ws;
  const bool rowwise = loss_rowwise(kind);
  const LossShape sh = loss_shape(rowwise, rows, cols);
  // a mean over the columns, except the two that Keras sums over a row (and the count of matching rows)
  const bool mean = !(kind == GN_LOSS_KULLBACK_LEIBLER_DIVERGENCE || rowwise);
  const double div = mean ? denom * (double)cols : denom, gscale = 1.0 / div;
  if (!rowwise) {
    const size_t n = (size_t)rows * (size_t)cols;
    const uintptr_t ph = (uintptr_t)p & 15;
    const bool same = ((uintptr_t)y & 15) == ph && (!dp || ((uintptr_t)dp & 15) == ph) && (ph & 3) == 0;
    const int mis = same ? (int)(ph / 4) : -1;
    switch (kind) {
#define GN_LOSS_CASE(K) case K: loss_launch_elem<K>(sh, p, y, dp, n, mis, gscale, partials, s); break;
      GN_LOSS_CASE(GN_LOSS_BINARY_CROSSENTROPY)
      GN_LOSS_CASE(GN_LOSS_MEAN_SQUARED_ERROR)
      GN_LOSS_CASE(GN_LOSS_MEAN_ABSOLUTE_ERROR)
      GN_LOSS_CASE(GN_LOSS_MEAN_ABSOLUTE_PERCENTAGE_ERROR)
      GN_LOSS_CASE(GN_LOSS_MEAN_SQUARED_LOGARITHMIC_ERROR)
      GN_LOSS_CASE(GN_LOSS_HINGE)
      GN_LOSS_CASE(GN_LOSS_SQUARED_HINGE)
      GN_LOSS_CASE(GN_LOSS_LOGCOSH)
      GN_LOSS_CASE(GN_LOSS_POISSON)
      GN_LOSS_CASE(GN_LOSS_KULLBACK_LEIBLER_DIVERGENCE)
#undef GN_LOSS_CASE
    }
  } else {
    switch (kind) {
      case GN_LOSS_CATEGORICAL_CROSSENTROPY: loss_launch_row<GN_LOSS_CATEGORICAL_CROSSENTROPY>(sh, p, y, dp, rows, cols, gscale, partials, s); break;
      case GN_LOSS_COSINE_PROXIMITY: loss_launch_row<GN_LOSS_COSINE_PROXIMITY>(sh, p, y, dp, rows, cols, gscale, partials, s); break;
      default: loss_launch_row<GN_LOSS_CATEGORICAL_ACCURACY>(sh, p, y, dp, rows, cols, gscale, partials, s); break;
    }
  }
  int rc = check_launch("loss_pass");
  if (rc) return rc;
  hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(256), 0, s, partials, (int)sh.blocks, div, out);
  return check_launch("loss_finish");
}

extern "C" size_t gn_weight_count_workspace(long long rows) {
  if (rows < 1) return 0;
  unsigned blocks;
  long long share;
  gn::count_shape(rows, blocks, share);
  return (size_t)blocks * sizeof(unsigned long long);
}

extern "C" int gn_weight_count(const float* w, long long rows, double* count, void* ws, size_t ws_bytes, void* stream) {
  using namespace gn;
  GN_REQUIRE(w && count, "weight_count: null pointer");
  GN_REQUIRE(rows >= 1, "weight_count: bad row count %lld", rows);
  GN_REQUIRE(ws && ws_bytes >= gn_weight_count_workspace(rows) && ((uintptr_t)ws & 7) == 0, "weight_count: workspace of %zu bytes, %zu needed (8-byte aligned)",
             ws_bytes, gn_weight_count_workspace(rows));
  hipStream_t s = (hipStream_t)stream;
  unsigned blocks;
  long long share;
  count_shape(rows, blocks, share);
  hipLaunchKernelGGL(weight_count_kernel, dim3(blocks), dim3(256), 0, s, w, rows, share, (unsigned long long*)ws, count);
  int rc = check_launch("weight_count");
  if (rc || blocks == 1) return rc;
  hipLaunchKernelGGL(weight_count_finish_kernel, dim3(1), dim3(256), 0, s, (const unsigned long long*)ws, (int)blocks, count);
  return check_launch("weight_count_finish");
}

extern "C" size_t gn_loss_pass_weighted_workspace(long long rows, int cols) {
  return gn_loss_pass_workspace(rows, cols) / 2 * 3;      // three partials per block: [weighted term sum, hits, weighted hits]
}

extern "C" int gn_loss_pass_weighted(int kind, const float* p, const float* y, const float* w, const double* count, float* dp, float* out, long long rows, int cols,
                                     void* ws, size_t ws_bytes, void* stream) {
  using namespace gn;
  GN_REQUIRE(kind >= 0 && kind < GN_LOSS_KINDS, "loss_pass_weighted: unknown kind %d", kind);
  GN_REQUIRE(p && y && w && count && out, "loss_pass_weighted: null pointer");
  GN_REQUIRE(rows >= 1 && cols >= 1, "loss_pass_weighted: bad shape (%lld, %d)", rows, cols);
  GN_REQUIRE(ws && ws_bytes >= gn_loss_pass_weighted_workspace(rows, cols) && ((uintptr_t)ws & 7) == 0,
             "loss_pass_weighted: workspace of %zu bytes, %zu needed (8-byte aligned)", ws_bytes, gn_loss_pass_weighted_workspace(rows, cols));
  hipStream_t s = (hipStream_t)stream;
  double* partials = (double*)ws;
  const bool rowwise = loss_rowwise(kind);
  const LossShape sh = loss_shape(rowwise, rows, cols);
  const bool mean = !(kind == GN_LOSS_KULLBACK_LEIBLER_DIVERGENCE || rowwise);
  const double coldiv = mean ? (double)cols : 1.0;
  if (!rowwise) {
    const size_t n = (size_t)rows * (size_t)cols;
    const uintptr_t ph = (uintptr_t)p & 15;
    const bool same = ((uintptr_t)y & 15) == ph && (!dp || ((uintptr_t)dp & 15) == ph) && (ph & 3) == 0;
    const int mis = same ? (int)(ph / 4) : -1;
    LossWeights lw;
    lw.w = w; lw.count = count; lw.cols = cols;
    lw.q4 = 1024 / cols; lw.r4 = 1024 % cols;
    lw.q1 = 256 / cols; lw.r1 = 256 % cols;
    lw.wvec = (cols == 1 && same && ((uintptr_t)w & 15) == ph) ? 1 : 0;
    switch (kind) {
#define GN_LOSS_CASE(K) case K: loss_launch_elem_weighted<K>(sh, p, y, dp, n, mis, coldiv, partials, lw, s); break;
      GN_LOSS_CASE(GN_LOSS_BINARY_CROSSENTROPY)
      GN_LOSS_CASE(GN_LOSS_MEAN_SQUARED_ERROR)
      GN_LOSS_CASE(GN_LOSS_MEAN_ABSOLUTE_ERROR)
      GN_LOSS_CASE(GN_LOSS_MEAN_ABSOLUTE_PERCENTAGE_ERROR)
      GN_LOSS_CASE(GN_LOSS_MEAN_SQUARED_LOGARITHMIC_ERROR)
      GN_LOSS_CASE(GN_LOSS_HINGE)
      GN_LOSS_CASE(GN_LOSS_SQUARED_HINGE)
      GN_LOSS_CASE(GN_LOSS_LOGCOSH)
      GN_LOSS_CASE(GN_LOSS_POISSON)
      GN_LOSS_CASE(GN_LOSS_KULLBACK_LEIBLER_DIVERGENCE)
#undef GN_LOSS_CASE
    }
  } else {
    switch (kind) {
      case GN_LOSS_CATEGORICAL_CROSSENTROPY: loss_launch_row_weighted<GN_LOSS_CATEGORICAL_CROSSENTROPY>(sh, p, y, dp, rows, cols, w, count, partials, s); break;
      case GN_LOSS_COSINE_PROXIMITY: loss_launch_row_weighted<GN_LOSS_COSINE_PROXIMITY>(sh, p, y, dp, rows, cols, w, count, partials, s); break;
      default: loss_launch_row_weighted<GN_LOSS_CATEGORICAL_ACCURACY>(sh, p, y, dp, rows, cols, w, count, partials, s); break;
    }
  }
  int rc = check_launch("loss_pass_weighted");
  if (rc) return rc;
  hipLaunchKernelGGL(loss_finish_weighted_kernel, dim3(1), dim3(256), 0, s, (const double*)partials, (int)sh.blocks, count, coldiv, (double)cols, out);
  return check_launch("loss_finish_weighted");
}

extern "C" int gn_bce_loss(const float* p, const float* y, float* dp, float* out, int B, int Bglobal, void* stream) {
  GN_REQUIRE(p && y && dp && out, "bce_loss: null pointer");
  return gn::loss_run(0, p, y, dp, out, B, Bglobal, (hipStream_t)stream);
}
extern "C" int gn_mse_loss(const float* p, const float* y, float* dp, float* out, int B, int Bglobal, void* stream) {
  GN_REQUIRE(p && y && dp && out, "mse_loss: null pointer");
  return gn::loss_run(1, p, y, dp, out, B, Bglobal, (hipStream_t)stream);
}
