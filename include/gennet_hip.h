/*
 * gennet_hip.h -- C ABI of libgennet_hip.so, the MI355X (gfx950) kernel library behind gennet_amd.
 *
 * The reference (hagabbar/GenNet, BBH_version/) has no native boundary of its own: every FLOP of its hot
 * path runs inside Keras 2.2.4 / TensorFlow 1.12 ops and numpy.  Each entry point below therefore cites
 * the reference call site whose arithmetic it replaces (file:line in /root/reference/BBH_version/), i.e.
 * the TF kernel that `model.add(<Layer>)` / `train_on_batch` / `predict` would have dispatched.
 *
 * Conventions
 *   - all pointers are DEVICE pointers (HBM) unless the name ends in _host; buffers are caller-owned
 *   - activations are channels-last fp32: (B, L, C) row-major, exactly Keras' layout
 *   - Conv1D kernels (k, Cin, Cout), Dense kernels (in, out), Conv2D kernels (kh, kw, Cin, Cout)
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*); no hidden syncs, no allocation
 *   - return 0 on success, a negative GN_E* code on bad arguments or launch failure (no exceptions)
 */
#ifndef GENNET_HIP_H
#define GENNET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GN_OK 0
#define GN_EINVAL (-1)   /* bad shape / unsupported configuration */
#define GN_ELAUNCH (-2)  /* hipLaunch / runtime error (see gn_last_error) */
#define GN_EWORKSPACE (-3) /* workspace too small */

/* activation kinds (Activation('relu'|'tanh'|'sigmoid'|'linear'), LeakyReLU(alpha), ReLU(max_value)):
 * bbhMahoGANy.py:238,254,...,293 (tanh/linear), :363-400 (relu, ReLU(max_value=1.0)), :440,448 (LeakyReLU 0.2), :495 (sigmoid) */
enum gn_act { GN_ACT_LINEAR = 0, GN_ACT_RELU = 1, GN_ACT_RELU_MAX = 2, GN_ACT_LEAKY = 3, GN_ACT_TANH = 4, GN_ACT_SIGMOID = 5 };

const char* gn_last_error(void);
int gn_version(void);

/* ---- Conv1D (bbhMahoGANy.py:250,259,267,275,283,292 generator; :362-371, :382-394 point-estimator; the
 *      width-2 Conv2D of :439,:447 after gn_conv2d_w2_fold) ----------------------------------------------
 * y[b,t,co] = act(bias[co] + sum_{k,ci} x[b, stride*t + k - pad_left, ci] * w[k,ci,co]), zero outside [0,L).
 * Lout is the caller-computed output length (TF SAME/VALID rule).  bias may be NULL.
 * Dispatches to the MFMA implicit-GEMM kernel (Cin >= 16), the small-Cin streaming kernel (Cin <= 4) or the
 * small-Cout reduction kernel (Cout <= 4). */
int gn_conv1d_fwd(const float* x, const float* w, const float* bias, float* y,
                  int B, int L, int Cin, int Cout, int k, int stride, int pad_left, int Lout,
                  int act, float act_param, void* stream);

/* EXPERIMENTAL, opt-in: the same forward convolution on the bf16 matrix cores with every fp32 operand split into three bf16
 * pieces (six v_mfma_f32_32x32x16_bf16 products, fp32 accumulation; error of the order of one fp32 rounding per product --
 * see gennet_amd/csrc/conv_bf16x3.hip).  Needs Cin % 16 == 0, Cout % 64 == 0, k <= 5, stride 1.  `ws` holds the split
 * operands (gn_conv1d_bf16x3_workspace bytes); resplit = 0 reuses the planes of the previous call (benchmarks only). */
size_t gn_conv1d_bf16x3_workspace(int B, int L, int Cin, int Cout, int k);
int gn_conv1d_fwd_bf16x3(const float* x, const float* w, const float* bias, float* y, void* ws, size_t ws_bytes,
                         int B, int L, int Cin, int Cout, int k, int stride, int pad_left, int Lout,
                         int act, float act_param, int resplit, void* stream);
/* Transform-domain fp32 convolution (Cook-Toom / Winograd F(2,5), gennet_amd/csrc/conv_wino.hip) for the unit-stride 5-tap layers --
 * generator Conv1D(128..1024, 5, padding='same') bbhMahoGANy.py:259-283, PE q branch Conv1D(128, 5) / Conv1D(256, 5) :382-384: six fp32
 * multiplies per two outputs instead of ten, every product still an exact fp32 fma on v_mfma_f32_32x32x2_f32.  Direct entry (tests, layer
 * benchmarks); `ws` receives the transformed kernel of this launch (gn_conv1d_wino_workspace bytes).  Needs k == 5, stride 1, Cin % 8 == 0,
 * Cout % 64 == 0. */
size_t gn_conv1d_wino_workspace(int Cin, int Cout);
int gn_conv1d_fwd_wino(const float* x, const float* w, const float* bias, float* y, void* ws, size_t ws_bytes,
                       int B, int L, int Cin, int Cout, int k, int stride, int pad_left, int Lout,
                       int act, float act_param, void* stream);
/* Process-wide opt-in: mode 1 routes every Conv1D forward / data-gradient launch that the bf16x3 kernel supports and that is
 * large enough to gain from it (Cin >= 256 and Cout >= 256, unit input stride) through it, operands split per launch into the
 * caller-owned device `workspace` (launches whose planes do not fit stay on the fp32 kernel); mode 0 (the default) restores
 * the exact-fp32 MFMA path everywhere.  The workspace must stay alive while mode 1 is set. */
int gn_set_conv_math(int mode, void* workspace, size_t workspace_bytes);

/* Same with a following Dropout fused into the epilogue (discriminator: Conv2D -> LeakyReLU -> Dropout(0.4), bbhMahoGANy.py:439-443,
 * :447-452): y = mask ? act(.)/(1-rate) : 0, mask = uint8 keep-mask of y's shape (gn_dropout_mask).  Cout > 4. */
int gn_conv1d_fwd_dropout(const float* x, const float* w, const float* bias, const uint8_t* mask, float* y,
                          int B, int L, int Cin, int Cout, int k, int stride, int pad_left, int Lout,
                          int act, float act_param, float rate, void* stream);
/* Linear Conv1D forward that also returns the BatchNorm statistics of its output, sums[0:Cout] = sum y, sums[Cout:2*Cout] = sum y^2
 * (fp64) -- the Conv1D -> BatchNormalization pairs of the generator (bbhMahoGANy.py:250-251, ..., :283-284).  On the pipelined MFMA
 * kernel the sums are accumulated in the epilogue (per-block fp64 partials, fixed-order final reduction): the separate statistics
 * pass over the output tensor disappears; other shapes run the convolution and then gn_bn_stats' pass, with the same result. */
size_t gn_conv1d_fwd_stats_workspace(int B, int Lout, int Cout);
int gn_conv1d_fwd_stats(const float* x, const float* w, const float* bias, float* y, double* sums, void* ws, size_t ws_bytes,
                        int B, int L, int Cin, int Cout, int k, int stride, int pad_left, int Lout, void* stream);

/* wt[k, co, ci] = w[k, ci, co]  (operand layout the dgrad GEMM consumes) */
int gn_conv1d_transpose_w(const float* w, float* wt, int k, int Cin, int Cout, void* stream);

/* dx[b,tau,ci] = sum_{k,co} dy[b,t,co] * w[k,ci,co] over stride*t + k - pad_left == tau.  wt from
 * gn_conv1d_transpose_w.  (Backward of the call sites above; TF Conv2DBackpropInput.)  k < stride: the rows tau no tap reaches are written
 * as zeros (dx is cleared first, then the phases that have taps run). */
int gn_conv1d_dgrad(const float* dy, const float* wt, float* dx,
                    int B, int L, int Cin, int Cout, int k, int stride, int pad_left, int Lout, void* stream);

/* Same, with the backward of the PRODUCER layer's [activation -> dropout] fused into the epilogue, so the gradient leaves the kernel
 * already multiplied by act'(.): dx = mask_prev ? dx/(1-rate) * act'(y_prev*(1-rate)) : 0 (mask_prev NULL: dx *= act'(y_prev)).
 * y_prev (B, L, Cin) is the producer's output (= this layer's input).  MFMA path only (Cin > 4 and Cout > 4). */
int gn_conv1d_dgrad_fused(const float* dy, const float* wt, float* dx,
                          int B, int L, int Cin, int Cout, int k, int stride, int pad_left, int Lout,
                          const float* y_prev, const uint8_t* mask_prev, int act_prev, float act_param_prev, float rate_prev, void* stream);

/* dw[k,ci,co] = sum_{b,t} x[b, stride*t + k - pad_left, ci] * dy[b,t,co];  db[co] = sum_{b,t} dy[b,t,co] (db may be NULL).
 * ws: workspace of at least gn_conv1d_wgrad_workspace(...) bytes (split-K partial slabs, summed in a fixed order,
 * so the result is bitwise reproducible).  (TF Conv2DBackpropFilter + BiasAddGrad.) */
size_t gn_conv1d_wgrad_workspace(int B, int L, int Cin, int Cout, int k, int stride, int Lout);
int gn_conv1d_wgrad(const float* x, const float* dy, float* dw, float* db, void* ws, size_t ws_bytes,
                    int B, int L, int Cin, int Cout, int k, int stride, int pad_left, int Lout, void* stream);

/* ---- any channel pair ------------------------------------------------------------------------------------
 * The entry points above are strict: Cin <= 4 needs Cout % 4 == 0 (the small-Cin kernels); otherwise Cout <= 4 needs Cin % 4 == 0 (the small-Cout
 * kernels); otherwise both must be multiples of 4.  Any other pair is GN_EINVAL (callers that size their layers for the aligned kernels hear
 * about it when a shape falls off them).  gn_conv1d_needs_any is that predicate for a forward or weight-gradient call of (Cin, Cout): 1 when
 * the strict entry point refuses the pair.  gn_conv1d_dgrad runs the swapped pair: it refuses when gn_conv1d_needs_any(Cout, Cin).  The _any entry points take the same parameters, run every pair the strict ones take
 * on the same kernels with the same bits, and the remaining pairs on the `anyc` kernels (csrc/conv_anyc.hip: exact fp32 on the matrix cores,
 * k <= 5, strides 1 and 2, bias and activation epilogue; the weight gradient's partial sums are reduced in a fixed order).  The fused variants
 * (dropout, producer gradient, statistics) have no _any form.  gn_conv1d_wgrad_workspace answers for every pair. */
int gn_conv1d_needs_any(int Cin, int Cout);
int gn_conv1d_fwd_any(const float* x, const float* w, const float* bias, float* y,
                      int B, int L, int Cin, int Cout, int k, int stride, int pad_left, int Lout,
                      int act, float act_param, void* stream);
int gn_conv1d_dgrad_any(const float* dy, const float* wt, float* dx,
                        int B, int L, int Cin, int Cout, int k, int stride, int pad_left, int Lout, void* stream);
int gn_conv1d_wgrad_any(const float* x, const float* dy, float* dw, float* db, void* ws, size_t ws_bytes,
                        int B, int L, int Cin, int Cout, int k, int stride, int pad_left, int Lout, void* stream);

/* ---- width-2 Conv2D fold (bbhMahoGANy.py:439,:447: Conv2D(C,(5,5),strides=(2,1),padding='same') on (n,2,Cin)) ----
 * wf[kh, w*Cin+c, w2*Cout+c2] = w[kh, w-w2+2, c, c2];   biasf = [bias, bias]
 * unfold_grad: dw[kh,kw,c,c2] = sum over the (w,w2) blocks with w-w2+2 == kw (0 for kw in {0,4}); db = dbf[:Cout]+dbf[Cout:] */
int gn_conv2d_w2_fold(const float* w, const float* bias, float* wf, float* biasf, int kh, int Cin, int Cout, void* stream);
int gn_conv2d_w2_unfold_grad(const float* dwf, const float* dbf, float* dw, float* db, int kh, int Cin, int Cout, void* stream);
/* Conv1D with 6 <= k <= 40 taps (`filtsize = 5 # 10 is best`, bbhMahoGANy.py:228, the Conv1D(.., filtsize, ..) of :250-292; the 16-tap layers of the
 * reference's saved Keras models) as an h-tap convolution over G*Cin channels with pad_left 0 (csrc/tap_fold.hip), G = ceil(k/5) groups of h = ceil(k/G)
 * taps (gn_conv1d_tap_groups): every further tap group becomes a further group of input channels over the input shifted by g*h rows, so the <= 5-tap
 * kernels above run it and accumulate the groups in their own K loop.
 *   gn_conv1d_tapfold_x:    x (B, L, Cin) -> x2 (B, L + pad_left, G*Cin), x2[b, j, g*Cin:(g+1)*Cin] = x[b, j - pad_left + g*h] (0 outside the input)
 *   gn_conv1d_tapfold_w:    w (k, Cin, Cout) -> w2 (h, G*Cin, Cout), w2[t, g*Cin:(g+1)*Cin] = w[t + g*h] (zero taps where t + g*h >= k)
 *   gn_conv1d_tapunfold_dw: the inverse, for the weight gradient: dw2 (h, G*Cin, Cout) -> dw (k, Cin, Cout)
 *   gn_conv1d_tapunfold_dx: dx2 (B, L + pad_left, G*Cin) -> dx (B, L, Cin), dx[b, l] = sum_g dx2[b, l + pad_left - g*h, g*Cin:(g+1)*Cin]
 * Then y = gn_conv1d_fwd*(x2, w2, bias, k' = h, stride, pad_left' = 0, L' = L + pad_left, Cin' = G*Cin) with the layer's own Lout. */
int gn_conv1d_tap_groups(int k, int* groups, int* taps);
int gn_conv1d_tapfold_x(const float* x, float* x2, int B, int L, int Cin, int k, int pad_left, void* stream);
int gn_conv1d_tapunfold_dx(const float* dx2, float* dx, int B, int L, int Cin, int k, int pad_left, void* stream);
int gn_conv1d_tapfold_w(const float* w, float* w2, int k, int Cin, int Cout, void* stream);
int gn_conv1d_tapunfold_dw(const float* dw2, float* dw, int k, int Cin, int Cout, void* stream);

/* ---- UpSampling1D(2) -> Conv1D(C, 5, strides=s, padding='same') fold (bbhMahoGANy.py:249-250 s=2, :258-259 s=1) ----
 * The pair equals a 3-tap stride-1 'same' conv (pad_left 1) on the UN-upsampled input x (B, L, Cin), so the upsampled tensor is
 * never written and 2 of 5 taps' multiplies go away:
 *   s=2:  y[t]    = W0 x[t-1] + (W1+W2) x[t] + (W3+W4) x[t+1]                     wf (3, Cin, Cout),   biasf = bias
 *   s=1:  y[2u]   = (W0+W1) x[u-1] + (W2+W3) x[u] + W4 x[u+1]     columns [0,Cout)
 *         y[2u+1] = W0 x[u-1] + (W1+W2) x[u] + (W3+W4) x[u+1]     columns [Cout,2Cout)  wf (3, Cin, 2*Cout), biasf = [bias, bias];
 *         the folded conv's (B, L, 2*Cout) output is the layer's (B, 2L, Cout) output in memory.
 * unfold_grad maps the folded conv's weight / bias gradient (gn_conv1d_wgrad on x and the same dy memory) back onto the 5 taps:
 * dW[k] = sum of the folded taps W[k] went into; db = dbf (s=2) or dbf[:Cout] + dbf[Cout:] (s=1). */
int gn_conv1d_up2_fold(const float* w, const float* bias, float* wf, float* biasf, int Cin, int Cout, int stride, void* stream);
int gn_conv1d_up2_unfold_grad(const float* dwf, const float* dbf, float* dw, float* db, int Cin, int Cout, int stride, void* stream);

/* ---- Dense (bbhMahoGANy.py:234 generator 100 -> 256*n_pix/2; :377,:399,:494 flatten -> 1 heads) -------------
 * y[b,o] = act(bias[o] + sum_i x[b,i] * w[i,o]).  Large `out` goes through the MFMA GEMM, out <= 4 through
 * the streaming dot-product kernel; widths neither takes (in % 4 or out % 4 nonzero) through one tiled fp32 GEMM kernel. */
int gn_dense_fwd(const float* x, const float* w, const float* bias, float* y, int B, int in, int out,
                 int act, float act_param, void* stream);
/* dw[i,o] = sum_b x[b,i]*dy[b,o]; db[o] = sum_b dy[b,o]; dx[b,i] = sum_o dy[b,o]*w[i,o] (dx may be NULL). */
size_t gn_dense_bwd_workspace(int B, int in, int out);
int gn_dense_bwd(const float* x, const float* w, const float* dy, float* dx, float* dw, float* db,
                 void* ws, size_t ws_bytes, int B, int in, int out, void* stream);

/* flatten -> Dense(out <= 4) backward with the producer's [activation -> dropout] backward fused (x IS the producer's output) */
int gn_dense_bwd_fused(const float* x, const float* w, const float* dy, float* dx, float* dw, float* db, int B, int in, int out,
                       const uint8_t* mask_prev, int act_prev, float act_param_prev, float rate_prev, void* stream);

/* ---- elementwise ----------------------------------------------------------------------------------------- */
/* y = act(x) (Activation / LeakyReLU / ReLU layers when not fused into the producing kernel) */
int gn_act_fwd(const float* x, float* y, size_t n, int act, float act_param, void* stream);
/* dx = dy * act'(.) expressed through the activation OUTPUT y; in-place (dx == dy) allowed */
int gn_act_bwd(const float* dy, const float* y, float* dx, size_t n, int act, float act_param, void* stream);
/* backward of [activation -> dropout] in one pass through the post-dropout output y: dx = mask ? dy/(1-rate) * act'(y*(1-rate)) : 0 */
int gn_act_dropout_bwd(const float* dy, const float* y, const uint8_t* mask, float* dx, size_t n, int act, float act_param, float rate, void* stream);
/* gn_bn_apply with the Dropout keep-mask GENERATED in the same pass (the draw of gn_dropout_mask, bit for bit) and written to
 * mask_out for the backward pass: y = mask ? act(x * scale + shift) / (1 - rate) : 0.  C % 4 == 0. */
int gn_bn_apply_dropgen(const float* x, const float* scale, const float* shift, uint8_t* mask_out, float* y, size_t rows, int C,
                        int act, float act_param, float rate, uint64_t seed, uint64_t offset, void* stream);
/* Conv2DTranspose epilogue (csrc/conv_transpose.hip), in place over the (rows, C) output of the adjoint conv's data gradient, any C:
 * y = act(y + bias[c]); with mask, y = keep ? y / (1 - rate) : 0.  gen != 0 draws the keep-mask into mask (4-byte aligned) in the same pass,
 * the draw of gn_dropout_mask bit for bit; gen == 0 reads mask (NULL: no dropout, rate must be 0). */
int gn_bias_act_dropout(float* y, const float* bias, uint8_t* mask, size_t rows, int C, int act, float act_param, float rate, int gen,
                        uint64_t seed, uint64_t offset, void* stream);
/* db[c] = sum over rows of dy[row, c] (the bias gradient of gn_dense_bwd / gn_conv1d_wgrad), any C: fixed summation order for C > 4 and for
 * C % 4 == 0; fp64 atomics for C in {1, 2, 3}.  ws: gn_bias_grad_workspace(rows, C) bytes. */
size_t gn_bias_grad_workspace(size_t rows, int C);
int gn_bias_grad(const float* dy, float* db, void* ws, size_t ws_bytes, size_t rows, int C, void* stream);
/* Inference-phase BatchNormalization folded into the preceding convolution (generator.predict, bbhMahoGANy.py:1248, :1330):
 * w_out[r, n] = w[r, n] * scale[n] (r over taps * Cin rows), bias_out[n] = bias[n] * scale[n] + shift[n], with scale / shift
 * from gn_bn_infer_coeffs; conv(x; w_out, bias_out) then equals BN_infer(conv(x; w, bias)).  Cout % 4 == 0; bias may be NULL. */
int gn_conv_fold_bn(const float* w, const float* bias, const float* scale, const float* shift, float* w_out, float* bias_out,
                    size_t rows, int Cout, void* stream);
/* PReLU (bbhMahoGANy.py:39; the act = 'prelu' branches at :237-286, :315-325): y[b,f] = x > 0 ? x : alpha[f] * x with one
 * alpha per feature of a sample (F features, F % 4 == 0).  Backward: dx = dy * (x > 0 ? 1 : x < 0 ? alpha : 0) (Keras'
 * relu(x) - alpha * relu(-x) has zero gradient at x == 0), dalpha[f] = sum_b dy[b,f] * min(x[b,f], 0); dx or dalpha may be NULL. */
int gn_prelu_fwd(const float* x, const float* alpha, float* y, int B, size_t F, void* stream);
int gn_prelu_bwd(const float* dy, const float* x, const float* alpha, float* dx, float* dalpha, int B, size_t F, void* stream);
/* Dropout (bbhMahoGANy.py:239,255,...,288 rate 0.2; :443,:452 rate 0.4): keep-mask generation (Philox4x32-10,
 * element i draws counter (offset + i/4), lane i%4; keep iff u >= rate) and application y = x*mask/(1-rate). */
int gn_dropout_mask(uint8_t* mask, size_t n, float rate, uint64_t seed, uint64_t offset, void* stream);
int gn_dropout_apply(const float* x, const uint8_t* mask, float* y, size_t n, float rate, void* stream);
/* UpSampling1D(size=2) (bbhMahoGANy.py:249,:258) and its adjoint: x (B, L, C) -> y (B, 2L, C), every row twice; dx = the sum of the two rows.
 * Any C >= 1: float4 units when C % 4 == 0 and both base pointers are 16-byte aligned, else floats. */
int gn_upsample2_fwd(const float* x, float* y, int B, int L, int C, void* stream);
int gn_upsample2_bwd(const float* dy, float* dx, int B, int L, int C, void* stream);
/* MaxPooling2D(pool_size=(2,1)) (the discriminator's `maxpool = True` configuration, bbhMahoGANy.py:426, :444-490): x (B, H, R) -> y (B, H/2, R), the
 * maximum over row pairs along H, R = W * C floats per row; an odd last row is dropped ('valid').  Backward: dy to the row that held the maximum (a tie:
 * the first row of the pair, as TensorFlow's max-pool gradient), zero elsewhere. */
int gn_maxpool_h2_fwd(const float* x, float* y, int B, int H, int R, void* stream);
int gn_maxpool_h2_bwd(const float* dy, const float* x, float* dx, int B, int H, int R, void* stream);
/* ---- Keras 2.2.4 pooling layers (gennet_amd/csrc/pooling.hip): MaxPooling1D / AveragePooling1D of the reference's
 * tests/burstMahoGANy.py, MaxPooling2D((2, 2)) of tests/ganymede.py, GlobalAveragePooling1D / 2D of 2_model_version/.../subtract_model.py ----
 * Windowed: x (B, H, W, C) -> y (B, Ho, Wo, C), channels last; the 1-D layers are W = pw = sw = 1, pad_left = 0, Wo = 1.  Output (ho, wo) reads
 * rows [ho*sh - pad_top, ho*sh - pad_top + ph) x columns [wo*sw - pad_left, wo*sw - pad_left + pw), clipped to the tensor; the caller computes
 * Ho, Wo and the pads by TensorFlow's rule ('valid': (H - ph) / sh + 1, pads 0, the rows behind the last full window are dropped; 'same':
 * ceil(H / sh), pad_top = max((Ho - 1) sh + ph - H, 0) / 2, the odd cell at the end).
 *   GN_POOL_MAX: padded cells never win; a window of -inf gives -inf.  Backward: dy to the FIRST maximum of the window in row-major (h, w)
 *                order (TensorFlow's max-pool gradient; gn_maxpool_h2_* is the (2,1)/(2,1) case, bit for bit), overlapping windows add.
 *   GN_POOL_AVG: fp32 sum in row-major order / the number of IN-BOUNDS cells (TensorFlow excludes the padding).  Backward: dy / count summed
 *                over the windows that cover the cell; x may be NULL.
 * Both backward passes are gathers over dx (no atomics: identical bits on every run; cells no window covers are written as zero).
 * Global: x (B, P, C) -> y (B, C), P = L or H*W.  GN_POOL_AVG: the fp64 sum over P in a fixed order, / P, rounded once; backward dy / P (x and
 * y may be NULL).  GN_POOL_MAX: K.max = tf.reduce_max, whose gradient is dy / n_ties to EVERY position equal to the maximum -- not the
 * first-maximum rule of the windowed layers.  ws: gn_global_pool_workspace(B, P, C) bytes, 16-byte aligned, serve both calls (the partials when
 * P is split across blocks, and dy / n_ties per (b, c)).
 * C % 4 == 0 on 16-byte aligned tensors runs with 16-byte loads and stores, anything else with scalar ones.  GN_EINVAL, nothing launched: a NULL
 * pointer (except as above), C, H, W, P, pool or stride < 1, an unknown mode, a pad outside [0, pool), Ho / Wo < 1 or so large that a window
 * holds no cell of the input.  B == 0 is GN_OK and launches nothing. */
enum gn_pool { GN_POOL_MAX = 0, GN_POOL_AVG = 1 };
int gn_pool2d_fwd(int mode, const float* x, float* y, int B, int H, int W, int C, int ph, int pw, int sh, int sw,
                  int pad_top, int pad_left, int Ho, int Wo, void* stream);
int gn_pool2d_bwd(int mode, const float* dy, const float* x, float* dx, int B, int H, int W, int C, int ph, int pw, int sh, int sw,
                  int pad_top, int pad_left, int Ho, int Wo, void* stream);
size_t gn_global_pool_workspace(int B, int P, int C);
int gn_global_pool_fwd(int mode, const float* x, float* y, void* ws, size_t ws_bytes, int B, int P, int C, void* stream);
int gn_global_pool_bwd(int mode, const float* dy, const float* x, const float* y, float* dx, void* ws, size_t ws_bytes, int B, int P, int C,
                       void* stream);
/* MyLayer (bbhMahoGANy.py:180-184): img[b,t,0] = x[b,t]; img[b,t,1] = event[t] - x[b,t];  adjoint dx = d0 - d1 */
int gn_subtract_stack_fwd(const float* x, const float* event, float* img, int B, int n, void* stream);
int gn_subtract_stack_bwd(const float* dimg, float* dx, int B, int n, void* stream);
/* A user-defined keras Layer whose call() is K.stack([a0*x + b0, a1*x + b1], axis=2) on x (B, n, 1) -- the form of the script's own
 * MyLayer.call (bbhMahoGANy.py:180-184: diff = self.const - x; K.stack([x, diff], axis=2) is a0 = 1, b0 = NULL, a1 = -1, b1 = const):
 *   img[b, t, 0] = a0*x[b,t] + b0[t],  img[b, t, 1] = a1*x[b,t] + b1[t]   (b0 / b1 may be NULL = 0);   dx = a0*dimg[...,0] + a1*dimg[...,1]. */
int gn_affine_stack_fwd(const float* x, const float* b0, const float* b1, float a0, float a1, float* img, int B, int n, void* stream);
int gn_affine_stack_bwd(const float* dimg, float a0, float a1, float* dx, int B, int n, void* stream);
/* discriminator batch assembly (bbhMahoGANy.py:1268-1289): sX (2B, n, 2, 1): rows [0,B) = [real[b,t], noise[b,t]], rows [B,2B) =
 * [fake[j,t], event[t]-fake[j,t]] with j = 2B-1-row (the reference's np.append prepends, so the fake half is in reversed order) */
int gn_assemble_d_batch(const float* real, const float* noise, const float* fake, const float* event, float* sX, int B, int n, void* stream);
/* uniform [lo, hi) and normal(mean,std) fills from Philox (host RNG replacement for bbhMahoGANy.py:1161,1247,1277,1295).  gn_fill_uniform, lo < hi:
 * element i = min(lo + (hi - lo) u, the largest float below hi), u = (word >> 8) / 2^24 of counter (offset + i/4), lane i%4 -- half-open for every
 * range, like numpy's uniform and Keras' random_uniform (the sum alone rounds up to hi at u = 1 - 2^-24 for ranges such as (20, 35)). */
int gn_fill_uniform(float* out, size_t n, float lo, float hi, uint64_t seed, uint64_t offset, void* stream);
int gn_fill_normal(float* out, size_t n, float mean, float std, uint64_t seed, uint64_t offset, void* stream);
/* Keras 2.2.4 noise layers (layers/noise.py), one pass each with the draw made in the same pass: element i uses Philox4x32-10 counter
 * (offset + i/4), lane i%4.  z is gn_fill_normal's N(0,1) draw bit for bit (gn_gaussian_noise_fwd at x = 0 equals gn_fill_normal(mean 0, std
 * stddev); gn_gaussian_dropout_apply at x = 1 equals gn_fill_normal(mean 1, std sd)); keep is gn_dropout_mask's test (u >= rate).
 *   GaussianNoise:   y = x + stddev z
 *   GaussianDropout: y = x (1 + sd z), sd = sqrt(rate / (1 - rate)); also the backward (dx = dy (1 + sd z)) with the forward's (seed, offset)
 *   AlphaDropout:    y = keep ? a x + b : a alpha_p + b;   backward dx = keep ? a dy : 0 with the forward's (seed, offset); 0 < rate < 1
 * x == y (in place) is allowed. */
int gn_gaussian_noise_fwd(const float* x, float* y, size_t n, float stddev, uint64_t seed, uint64_t offset, void* stream);
int gn_gaussian_dropout_apply(const float* x, float* y, size_t n, float sd, uint64_t seed, uint64_t offset, void* stream);
int gn_alpha_dropout_fwd(const float* x, float* y, size_t n, float rate, float a, float b, float alpha_p, uint64_t seed, uint64_t offset, void* stream);
int gn_alpha_dropout_bwd(const float* dy, float* dx, size_t n, float rate, float a, uint64_t seed, uint64_t offset, void* stream);
/* out[i,:] = src[idx[i],:] (random.sample batch gather, bbhMahoGANy.py:1156-1157, :1244) */
int gn_gather_rows(const float* src, const int64_t* idx, float* out, int rows, int width, void* stream);
/* y[i] += a * x[i] */
int gn_axpy(float* y, const float* x, float a, size_t n, void* stream);

/* ---- Keras 2.2.4 merge layers (gennet_amd/csrc/merge.hip): Add, Subtract, Multiply, Average, Maximum, Minimum and
 * Concatenate.  The reference forms `noise_signal - generated` and stacks it beside `generated` on the host at every iteration
 * (bbhMahoGANy.py:1268-1272); with these the same is written in the model: Concatenate(axis=-1)([g, Subtract()([event, g])]).
 * xs_host / dxs_host / widths_host are HOST arrays of n_inputs entries (1 .. GN_MERGE_MAX_INPUTS), read when the call is made: the device
 * pointers travel to the kernel by value, nothing is copied and nothing synchronises, so a captured step replays.
 * Element-wise, over n floats of any length and alignment (float4 body where y and every input are mutually 16-byte aligned, else an
 * all-scalar pass); buffers must not overlap in part:
 *   y = x0 o x1 o ... o x_{k-1} folded LEFT TO RIGHT in fp32, as keras' _merge_function loops.  GN_MERGE_AVG: that sum / (float)k, one
 *   division.  GN_MERGE_SUB: k == 2.  GN_MERGE_MAX / MIN: b > a ? b : a (b < a), the earlier value stays on a tie (+-0 included).
 *   gn_merge_bwd, the gradient of input `which`: GN_MERGE_MUL dx = dy * (product of x_j, j != which, left to right from the first such j;
 *   x[which] is not read); GN_MERGE_MAX / MIN dx = dy where `which` is the FIRST input that attains the extremum, +0 elsewhere (TensorFlow's
 *   _MaximumMinimumGrad under keras' chain of K.maximum).  The other modes have no kernel: Add dx = dy; Subtract, Average gn_scale by -1, 1 / k.
 *   gn_scale: y = a * x, out of place (the gradient that arrives is shared between the inputs and is never written).
 * Concatenate over the (outer, w_i) views, w_i = (extent of input i along the axis) * (product of the dimensions behind it):
 *   gn_concat_fwd gathers y (outer, sum w_i) = [x_0 | x_1 | ...] in one launch; gn_concat_bwd scatters dy (outer, sum w_i) into the dx_i in
 *   one launch, a NULL dx_i is skipped.  float4 units when every w_i % 4 == 0 and every pointer is 16-byte aligned, else floats.
 * GN_EINVAL, nothing launched: a NULL pointer (except a dx_i), n_inputs outside 1 .. GN_MERGE_MAX_INPUTS (Subtract: != 2), an unknown mode or
 * one without a backward kernel, `which` outside [0, n_inputs), a width < 1 or a total width >= 2^31.  n == 0 / outer == 0 is GN_OK. */
#define GN_MERGE_MAX_INPUTS 8
enum gn_merge { GN_MERGE_ADD = 0, GN_MERGE_SUB = 1, GN_MERGE_MUL = 2, GN_MERGE_AVG = 3, GN_MERGE_MAX = 4, GN_MERGE_MIN = 5 };
int gn_merge_fwd(int mode, const float* const* xs_host, int n_inputs, float* y, size_t n, void* stream);
int gn_merge_bwd(int mode, const float* dy, const float* const* xs_host, int n_inputs, int which, float* dx, size_t n, void* stream);
int gn_scale(const float* x, float a, float* y, size_t n, void* stream);
int gn_concat_fwd(const float* const* xs_host, const int* widths_host, int n_inputs, float* y, size_t outer, void* stream);
int gn_concat_bwd(const float* dy, float* const* dxs_host, const int* widths_host, int n_inputs, size_t outer, void* stream);

/* ---- Conv1D(dilation_rate=d, padding='causal') (gennet_amd/csrc/dilate.hip): a stride-1 conv with dilation d is d
 * independent undilated convs, one per phase (l mod d) of the zero-padded input.  Two memory-bound passes move a tensor into and out of
 * that phase layout; the convs between them are the library's own, on a d times larger batch.
 *   gn_dilate_split: x (B, L, C) -> xs (B*d, M, C).  With i = m*d + p - off: xs[b*d + p, m, :] = x[b, i, :] where 0 <= i < L, +0.0f
 *     elsewhere.  Every element of xs is written; an input row that falls outside the M rows is dropped.  d = 1: a copy behind `off` zero rows.
 *   gn_dilate_merge: xs (B*d, M, C) -> x (B, L, C), x[b, i, :] = xs[b*d + (i + off) % d, (i + off) / d, :]: the exact adjoint of the
 *     split, a gather (no atomics), every element of x written once.
 * float4 units when C % 4 == 0 and both base pointers are 16-byte aligned, else floats; element indices are size_t.
 * GN_EINVAL, nothing launched: a NULL pointer, any of B, L, C, d, M < 1, off < 0; for the merge (L - 1 + off) / d >= M (a row outside xs). */
int gn_dilate_split(const float* x, float* xs, int B, int L, int C, int d, int off, int M, void* stream);
int gn_dilate_merge(const float* xs, float* x, int B, int L, int C, int d, int off, int M, void* stream);

/* ---- BatchNormalization(momentum=0.99) (bbhMahoGANy.py:235 over 256*n_pix/2 features; :251,...,:284 over channels) ----
 * x is viewed as (rows, C).  Statistics are accumulated in fp64: sums[0:C] = sum x, sums[C:2C] = sum x^2.
 * Between gn_bn_stats and gn_bn_finalize a data-parallel caller all-reduces `sums` (SyncBN). */
size_t gn_bn_stats_workspace(size_t rows, int C);
int gn_bn_stats(const float* x, size_t rows, int C, double* sums, void* ws, size_t ws_bytes, void* stream);
/* mean = S1/n, var = S2/n - mean^2 (biased); scale = gamma/sqrt(var+eps), shift = beta - mean*scale;
 * moving statistics as a plain exponential average, TF's assign_moving_average(zero_debias=False):
 *   moving_mean -= (moving_mean - mean)*(1-m); moving_var -= (moving_var - var*n/(n-(1+eps)))*(1-m)   (keras normalization.py variance factor).
 * save_mean/save_invstd are kept for the backward pass. */
int gn_bn_finalize(const double* sums, double count, const float* gamma, const float* beta, float eps, float momentum,
                   float* moving_mean, float* moving_var, float* scale, float* shift,
                   float* save_mean, float* save_invstd, int C, void* stream);
/* the same with the moving statistics updated as keras 2.2.4's TF backend does (K.moving_average_update ->
 * tf moving_averages.assign_moving_average(x, value, momentum, zero_debias=True); bbhMahoGANy.py:223 momentum, :1248 the
 * generator.predict that consumes them): biased_* are shadow accumulators that start at ZERO,
 *   biased -= (biased - value)*(1-m);  moving -= moving - biased/(1 - m^local_step)
 * with local_step the ALREADY incremented update count (1 for the first update): the moving statistic is the debiased average
 * of the batch values and forgets its 0/1 initial value at the first update. */
int gn_bn_finalize_zero_debias(const double* sums, double count, const float* gamma, const float* beta, float eps, float momentum,
                               float* moving_mean, float* moving_var, float* biased_mean, float* biased_var, int local_step,
                               float* scale, float* shift, float* save_mean, float* save_invstd, int C, void* stream);
/* inference phase: scale/shift from the moving statistics */
int gn_bn_infer_coeffs(const float* gamma, const float* beta, const float* moving_mean, const float* moving_var,
                       float eps, float* scale, float* shift, int C, void* stream);
/* y = dropout(act(x*scale[c] + shift[c])) in one pass; mask may be NULL (no dropout / inference) */
int gn_bn_apply(const float* x, const float* scale, const float* shift, const uint8_t* mask, float* y,
                size_t rows, int C, int act, float act_param, float rate, void* stream);
/* backward pass 1: g = dy * mask/(1-rate) * act'(a), xhat = (x-mean)*invstd, with a = the activation output: taken from the stored
 * layer output (a = y/(mask scale)) or, when scale and shift (the forward pass' gn_bn_finalize outputs) are given, RECOMPUTED from
 * the pre-BN tensor as act(fma(x, scale, shift)) -- bit-identical to the forward and one 4-byte read per element less (y may then
 * be NULL).  dsums[0:C] = sum g, dsums[C:2C] = sum g*xhat (fp64).  A data-parallel caller all-reduces dsums. */
int gn_bn_bwd_stats(const float* dy, const float* y, const float* x, const uint8_t* mask,
                    const float* save_mean, const float* save_invstd, double* dsums, void* ws, size_t ws_bytes,
                    size_t rows, int C, int act, float act_param, float rate, const float* scale, const float* shift, void* stream);
/* backward pass 2: dx = gamma*invstd*(g - dsum/n - xhat*dsum_xhat/n); dgamma = dsums_local[C:2C], dbeta = dsums_local[0:C];
 * scale / shift as above. */
int gn_bn_bwd_apply(const float* dy, const float* y, const float* x, const uint8_t* mask,
                    const float* gamma, const float* save_mean, const float* save_invstd,
                    const double* dsums_global, double count, const double* dsums_local, float* dx, float* dgamma, float* dbeta,
                    size_t rows, int C, int act, float act_param, float rate, const float* scale, const float* shift, void* stream);

/* BatchNormalization backward when the layer's output feeds ONLY a Conv1D(1 filter, k <= 5 taps, stride 1) -- the generator's last
 * BatchNormalization -> tanh -> Dropout -> Conv1D(1, 5, padding='same') (bbhMahoGANy.py:284-292).  The gradient arriving at the BN
 * output is then that conv's data gradient  dz[b,t,c] = sum_j g[b, t - j + pad_left] * w[j,c]  (g (B, Lout): the conv's output
 * gradient, w (k, C): its kernel; terms with t - j + pad_left outside [0, Lout) are zero), rank-k in (t, c).  These two calls take
 * (g, w, L, Lout, k, pad_left) in place of dy and form dz where it is consumed, so gn_conv1d_dgrad never writes the (B, L, C) tensor
 * and the two passes never read it (12 bytes per element less: 4.3 GB x 3 per generator step at the BASELINE size).  rows = B * L.
 * Same results as gn_bn_bwd_stats / gn_bn_bwd_apply on the materialised dz up to the rounding of the k-term sum.
 * Needs C % 4 == 0 and scale / shift (the activation output is recomputed from x). */
int gn_bn_bwd_stats_conv1(const float* g, const float* w, int L, int Lout, int k, int pad_left, const float* x, const uint8_t* mask,
                          const float* save_mean, const float* save_invstd, double* dsums, void* ws, size_t ws_bytes, size_t rows, int C,
                          int act, float act_param, float rate, const float* scale, const float* shift, void* stream);
int gn_bn_bwd_apply_conv1(const float* g, const float* w, int L, int Lout, int k, int pad_left, const float* x, const uint8_t* mask,
                          const float* gamma, const float* save_mean, const float* save_invstd, const double* dsums_global, double count,
                          const double* dsums_local, float* dx, float* dgamma, float* dbeta, size_t rows, int C, int act, float act_param,
                          float rate, const float* scale, const float* shift, void* stream);

/* ---- BatchNormalization over an axis that is not the last one (csrc/bn_axis.hip): keras BatchNormalization(axis=1) on (B, L, C), one
 * gamma / beta / moving_mean / moving_variance per position l, statistics over the batch and the channels ----
 * x is viewed as (outer, P, inner): element (o, p, i) at (o*P + p)*inner + i; P the normalised axis, outer the product of the dimensions
 * in front of it (the batch included), inner the product of those behind it.  Any outer, P, inner >= 1 with P*inner < 2^31; inner % 4 == 0
 * on 16-byte aligned tensors runs with 16-byte loads and stores, anything else with scalar ones.  inner == 1 is the last-axis case
 * (rows = outer, C = P) that gn_bn_stats ... gn_bn_bwd_apply serve; it is accepted here and computes the same.
 * No activation, no dropout mask.  gn_bn_finalize(_zero_debias(_dyn)) and gn_bn_infer_coeffs run between the passes with C := P and
 * count = outer*inner (times the world size after the all-reduce of sums / dsums).
 * Bytes per element: stats reads 4; apply reads 4, writes 4; bwd_stats reads 8; bwd_apply reads 8, writes 4.
 * Both reductions sum in a fixed order (per-block fp64 partials in ws, then summed chunk by chunk): repeated runs give identical bits.
 * ws: gn_bn_axis_stats_workspace(outer, P, inner) bytes serve all three calls that take one. */
size_t gn_bn_axis_stats_workspace(size_t outer, int P, int inner);
/* sums[0:P] = sum over (o, i) of x, sums[P:2P] = sum of x^2 (fp64) */
int gn_bn_axis_stats(const float* x, size_t outer, int P, int inner, double* sums, void* ws, size_t ws_bytes, void* stream);
/* y = fma(x, scale[p], shift[p]): gn_bn_apply's expression; both phases */
int gn_bn_axis_apply(const float* x, const float* scale, const float* shift, float* y, size_t outer, int P, int inner, void* stream);
/* dsums[0:P] = sum dy, dsums[P:2P] = sum dy*xhat, xhat = (x - save_mean[p])*save_invstd[p] (fp64) */
int gn_bn_axis_bwd_stats(const float* dy, const float* x, const float* save_mean, const float* save_invstd, double* dsums, void* ws,
                         size_t ws_bytes, size_t outer, int P, int inner, void* stream);
/* dx = gamma[p]*invstd[p]*(dy - dsum[p]/n - xhat*dsum_xhat[p]/n) from dsums_global and count = n; dbeta = dsums_local[0:P],
 * dgamma = dsums_local[P:2P] as fp32.  ws (>= 12*P bytes) holds the three per-position constants, formed once in front of the pass. */
int gn_bn_axis_bwd_apply(const float* dy, const float* x, const float* gamma, const float* save_mean, const float* save_invstd,
                         const double* dsums_global, double count, const double* dsums_local, float* dx, float* dgamma, float* dbeta,
                         void* ws, size_t ws_bytes, size_t outer, int P, int inner, void* stream);

/* ---- softmax along one axis (csrc/softmax.hip; keras activations.softmax, layers.Softmax(axis)) on the same (outer, P, inner)
 * view: y = exp(x - max_p x) / sum_p exp(x - max_p x); dx = y * (dy - sum_p dy * y) from the stored output y.  inner == 1 is the channel
 * softmax of a dense or conv output.  No workspace.  fp32 reductions in a fixed order, no atomics: repeated runs give identical bits.
 * Bytes per element: forward 8 and backward 12 while a row fits the lanes that own it (inner == 1: P <= 4096; inner >= 16: P <= 16, float4
 * columns 8; inner < 16: P <= 16 * (64 / inner)), beyond that 12 and 20 (running maximum, sum rescaled once per tile, second read).
 * y may alias x, dx may alias dy.  Inputs are finite; a row holding +-3e38 gives exact 0 and 1.
 * GN_EINVAL, nothing launched: a NULL pointer, outer / P / inner < 1, P * inner >= 2^31, outer * P * inner >= 2^62. */
int gn_softmax_fwd(const float* x, float* y, size_t outer, int P, int inner, void* stream);
int gn_softmax_bwd(const float* dy, const float* y, float* dx, size_t outer, int P, int inner, void* stream);

/* ---- batched fp32 matrix product (csrc/bmm.hip; keras layers.Dot through K.batch_dot):
 *   c[(bt*M + m)*N + n] = sum_k a[bt*a_batch + m*a_m + k*a_k] * b[bt*b_batch + k*b_k + n*b_n]      strides in elements, c contiguous.
 * For each operand one of its two matrix strides is 1 and the other at least the extent of the contiguous axis, so the product, a . b^T,
 * a^T . b and a^T . b^T are this one call and Dot's gradients land in their owner's layout.  M, N >= 2 run on the fp32 matrix cores
 * (v_mfma_f32_32x32x2_f32, block tiles of 64 or 128 per side, K in chunks of 16 through LDS, 16-byte loads along the unit stride where the base
 * pointer is 16-byte aligned and the batch stride and row length are multiples of 4, scalar loads otherwise); M == 1 or N == 1 on a
 * matrix-vector kernel (a wave per output when the matrix rows are contiguous in k, else a lane per output).  No split-K, no atomics, no
 * workspace: on the matrix cores every output is one fp32 fma chain in k order from +0, so it does not depend on the tile, the batch or
 * the launch; the wave-per-output sum has a fixed order that depends on K alone.  gn_bmm_valu is the same contract on a 16 x 16 VALU tile
 * (one fmaf chain per lane: the same bits as the matrix-core kernel), kept as the yardstick of scripts/bmm_microbench.py; nothing selects it.
 * GN_EINVAL, nothing launched: a negative size, K < 1, a stride <= 0, a stride pair that is not {1, >= extent}, a NULL pointer with
 * non-zero work, more than 2^31 - 1 blocks, an operand spanning 2^62 elements.  batch == 0, M == 0 or N == 0 is GN_OK without a launch. */
int gn_bmm(const float* a, const float* b, float* c, int batch, int M, int N, int K, long long a_batch, long long a_m, long long a_k,
           long long b_batch, long long b_k, long long b_n, void* stream);
int gn_bmm_valu(const float* a, const float* b, float* c, int batch, int M, int N, int K, long long a_batch, long long a_m, long long a_k,
                long long b_batch, long long b_k, long long b_n, void* stream);

/* ---- L2 normalisation along one axis (csrc/bmm.hip; Dot(normalize=True): K.l2_normalize = tf.nn.l2_normalize) on the (outer, P, inner) view:
 *   s = sum_p x^2, inv[(o, i)] = 1 / sqrt(max(s, 1e-12)), y = x * inv;  dx = inv * (dy - y * sum_p dy * y), and dx = inv * dy where s was
 *   clamped (inv is then exactly 1e6f, which is how the backward tells).  inv holds outer * inner floats.  fp32 sums in a fixed order, no atomics.
 * GN_EINVAL, nothing launched: a NULL pointer, P / inner < 1, P * inner >= 2^31, outer * P * inner >= 2^62.  outer == 0 is GN_OK. */
int gn_l2norm_fwd(const float* x, float* y, float* inv, size_t outer, int P, int inner, void* stream);
int gn_l2norm_bwd(const float* dy, const float* y, const float* inv, float* dx, size_t outer, int P, int inner, void* stream);

/* ---- fused dot-product attention (csrc/attention.hip; tf.keras layers.Attention) over contiguous fp32 q (B, Tq, d), k (B, Tk, d),
 * v (B, Tk, dv):   s[i, j] = scale * sum_c q[i, c] k[j, c],   p = softmax_j(s),   out[i, :] = sum_j p[i, j] v[j, :]     out (B, Tq, dv).
 * `causal`: entry (i, j) takes part iff j <= i (the lower triangle of the (Tq, Tk) matrix; Tq != Tk allowed); a masked entry is exactly 0 in the row
 * sum and in every gradient, and tiles wholly above the diagonal are not visited.  `scale` is a DEVICE pointer to one float, NULL for 1: a captured
 * step replays with the updated value.  No (Tq, Tk) tensor is written: a block owns GN_ATTN_BQ rows of one batch entry and walks the other side in
 * ascending tiles of GN_ATTN_BK rows on v_mfma_f32_32x32x2_f32 with a running maximum and sum.  No atomics; a row's result does not depend on B, on
 * the launch or on the grid, and two runs give identical bits.  Any B, Tq, Tk >= 1; 1 <= d, dv <= GN_ATTN_MAX_D; 4-byte aligned pointers (16-byte
 * loads where a base pointer is 16-byte aligned and its row length a multiple of 4).
 * gn_attention_fwd: writes out and, where lse is not NULL (the training phase), lse (B, Tq) = row maximum + log(row sum).
 * gn_attention_bwd: from q, k, v, scale, out and lse as the forward left them and dout (B, Tq, dv), writes each of dq (B, Tq, d), dk (B, Tk, d),
 *   dv_out (B, Tk, dv) that is not NULL, and into dscale_rows (B Tq floats, may be NULL) one partial per query row of the gradient of `scale`,
 *   sum_j dS[i, j] (q_i . k_j): their sum is the gradient (gn_bias_grad over the (B Tq, 1) view).  p = expf(s - lse) is recomputed tile by tile.
 *   ws: gn_attention_workspace(B, Tq) bytes (delta[i] = sum_c dout[i, c] out[i, c]).
 * GN_EINVAL, nothing launched: a NULL pointer, B < 0, Tq or Tk < 1, d or dv outside 1 .. GN_ATTN_MAX_D, more than 2^31 - 1 blocks;
 * GN_EWORKSPACE: ws too small.  B == 0 (and a backward with no gradient asked for) is GN_OK without a launch. */
#define GN_ATTN_BQ 128
#define GN_ATTN_BK 64
#define GN_ATTN_MAX_D 128
size_t gn_attention_workspace(int B, int Tq);
int gn_attention_fwd(const float* q, const float* k, const float* v, const float* scale, float* out, float* lse, int B, int Tq, int Tk, int d, int dv,
                     int causal, void* stream);
int gn_attention_bwd(const float* q, const float* k, const float* v, const float* scale, const float* out, const float* lse, const float* dout, float* dq,
                     float* dk, float* dv_out, float* dscale_rows, void* ws, size_t ws_bytes, int B, int Tq, int Tk, int d, int dv, int causal,
                     void* stream);

/* ---- layer normalisation over the trailing axes (csrc/layernorm.hip; keras layers.LayerNormalization) on the contiguous fp32 (rows, N)
 * view, rows the batch and every leading axis, N the product of the normalised axes:
 *   mean_r = sum_c x / N,  var_r = sum_c (x - mean_r)^2 / N (biased),  rstd_r = 1 / sqrt(var_r + eps),  xhat = (x - mean_r) rstd_r,
 *   y = xhat gamma[c] + beta[c];   g = dy gamma,  dx = rstd_r ((g - mean_c g) - xhat mean_c (g xhat)),  dgamma[c] = sum_r dy xhat,  dbeta[c] = sum_r dy.
 * The variance is the centred second pass over the values of the first, never E[x^2] - E[x]^2.  Regimes by N alone: N <= GN_LN_ROWS_MAX_N a
 * sub-group of min(64, pow2ceil(ceil(N / 4))) lanes owns a row in registers; N <= GN_LN_BLOCK_MAX_N a block of 256 lanes owns it in registers;
 * beyond, a block streams it (the centred pass and the output pass read x again).  Bytes per element: 8 forward (+ 8 / N for mean and rstd) and
 * 12 backward in the first two regimes, 16 and 20 streamed.  16-byte accesses where N % 4 == 0 and every pointer is 16-byte aligned, else 4-byte
 * accesses of the same kernel: the same bits.  No atomics: fp32 reductions in an order fixed by N alone; the weight gradients leave each of the
 * blocks (at most GN_LN_BWD_GRID_CAP, GN_LN_BWD_GRID_CAP_WIDE where N > GN_LN_ROWS_MAX_N) as one fp32 (2, N) partial in the workspace and are summed
 * in fp64 in a fixed order over the blocks, rounded once.  A
 * row's y and dx do not depend on rows, on the grid or on the launch; two runs give identical bits.  y may alias x, dx may alias dy.
 * gn_layernorm_fwd: gamma NULL is scale=False (1), beta NULL is center=False (0); mean and rstd (rows floats each) are written where given -- the
 *   training phase -- and are both NULL in the inference phase.
 * gn_layernorm_bwd: from dy, x and the mean / rstd the forward wrote; each of dx, dgamma, dbeta is written where it is not NULL, in any
 *   combination (scale=False with center=True asks for dbeta alone), except dgamma without gamma; all three NULL is GN_OK without a launch;
 *   dgamma and dbeta both NULL (a frozen layer) writes no partials and launches no reduction.  ws: gn_layernorm_bwd_workspace(rows, N) bytes,
 *   4-byte aligned; it may be NULL where dgamma and dbeta are and N <= GN_LN_BLOCK_MAX_N.
 * GN_EINVAL, nothing launched: a required pointer NULL (forward x, y; backward dy, x, mean, rstd, and ws where needed), rows < 1, N < 1,
 * rows * N >= 2^62, eps negative or not finite, mean without rstd or rstd without mean, dgamma without gamma, a misaligned workspace;
 * GN_EWORKSPACE: ws_bytes below gn_layernorm_bwd_workspace (which is 0 for a shape the entry points refuse). */
#define GN_LN_ROWS_MAX_N 1024
#define GN_LN_BLOCK_MAX_N 4096
#define GN_LN_FWD_GRID_CAP 2048
#define GN_LN_BWD_GRID_CAP 1024
#define GN_LN_BWD_GRID_CAP_WIDE 512
int gn_layernorm_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd, size_t rows, int N, float eps,
                     void* stream);
size_t gn_layernorm_bwd_workspace(size_t rows, int N);
int gn_layernorm_bwd(const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd, float* dx, float* dgamma, float* dbeta,
                     void* ws, size_t ws_bytes, size_t rows, int N, void* stream);

/* ---- LSTM recurrence (csrc/lstm.hip; keras layers.LSTM, LSTMCell of keras 2.2.4).  Gate columns i, f, c, o of width u:
 *   z_t = zx_t + h_{t-1} . U + b;  i = ra(z_i), f = ra(z_f), g = act(z_c), o = ra(z_o);  c_t = f c_{t-1} + i g;  h_t = o act(c_t)
 * with act one of GN_LSTM_TANH, _SIGMOID, _RELU, _LINEAR and ra one of GN_LSTM_HARD_SIGMOID (min(max(0.2 x + 0.5, 0), 1)), GN_LSTM_SIGMOID.
 * One block carries 16 batch rows through all T steps: h and c stay on chip, the step product runs on v_mfma_f32_16x16x4_f32, no block waits
 * on another, no atomics.  Every z is one fp32 fma chain over k from +0, then + zx, then + b, so a sample's results do not depend on B, on its
 * tile or on the launch.  1 <= u <= 512; any B, T >= 1; 4-byte aligned pointers.
 * gn_lstm_fwd: zx (B, T, 4u) = X . W, U (u, 4u), bias (4u), h0 / c0 (B, u) or NULL (zeros).  Step s = 0 .. T-1 reads zx at the input time
 *   t = s, or T-1-s under `reverse`, and writes h[:, s] (processing order, as keras returns it).  With `training` it also stores, at the INPUT
 *   time t of the step, the activated gates (B, T, 4u), c (B, T, u) and hprev (B, T, u), the h that entered the step (h0 at the first).
 * gn_lstm_bwd: dy (B, T, u) in processing order (dy_seq) or (B, u) for the last step only; gates, c as stored, c0 as given to the forward.
 *   Walks the steps backwards, forms dh_{t-1} = dz_t . U^T on the matrix cores and writes dz (B, T, 4u) at the input time index, so
 *   dW = X^T dz, dU = hprev^T dz, dX = dz W^T and db are products over B T rows; dh0 / dc0 (B, u) when not NULL.
 * ws: gn_lstm_fwd_workspace(u) / gn_lstm_bwd_workspace(u) bytes (the zero-padded U / U^T the kernels read); 0 for a u out of range.
 * GN_EINVAL, nothing launched: a NULL pointer, T < 1, u < 1 or u > 512, an unknown activation code; GN_EWORKSPACE: ws too small.
 * B == 0 is GN_OK without a launch. */
enum gn_lstm_act { GN_LSTM_TANH = 0, GN_LSTM_SIGMOID = 1, GN_LSTM_RELU = 2, GN_LSTM_LINEAR = 3, GN_LSTM_HARD_SIGMOID = 4 };
size_t gn_lstm_fwd_workspace(int u);
size_t gn_lstm_bwd_workspace(int u);
int gn_lstm_fwd(const float* zx, const float* U, const float* bias, const float* h0, const float* c0, float* h, float* gates, float* c, float* hprev,
                void* ws, size_t ws_bytes, int B, int T, int u, int act, int ract, int reverse, int training, void* stream);
int gn_lstm_bwd(const float* dy, const float* gates, const float* c, const float* c0, const float* U, float* dz, float* dh0, float* dc0, void* ws,
                size_t ws_bytes, int B, int T, int u, int act, int ract, int reverse, int dy_seq, void* stream);

/* ---- a PAIR of LSTM directions in one launch (csrc/lstm.hip; keras layers.Bidirectional).  The kernels are gn_lstm_fwd's and
 * gn_lstm_bwd's with a second grid dimension: blockIdx.y is the direction d, the grid is ceil(B / 16) x 2 blocks, and no block waits on another.
 * Every per-direction operand comes as a HOST table of two device pointers.  Direction 0 walks with reverse = reverse0, direction 1 with
 * !reverse0; each direction is bit for bit what the single entry point gives on the same operands.  No initial state (h0 = c0 = 0).
 * h / dy are addressed through a row stride `ld` >= u in floats and the direction's base pointer: two (B, T, u) buffers with ld = u, or ONE
 *   (B, T, 2u) buffer with h[1] = h[0] + u and ld = 2u (the concatenated output; the directions own disjoint columns).  Direction 0 writes step
 *   s at position s, direction 1 at position T-1-s (keras' K.reverse of the backward half: by position, whatever reverse0 is).  seq == 0: only
 *   the last processed step of each direction is written, into a (B, ld) row buffer; dy_seq == 0: dy is that (B, ld) buffer.
 * zx, U, bias, gates, c, hprev, dz: per direction, contiguous, at the input time index, as in gn_lstm_fwd / gn_lstm_bwd.  gates, c and hprev
 *   (the tables, or their entries) may be NULL without `training`.
 * ws: TWICE gn_lstm_fwd_workspace(u) / gn_lstm_bwd_workspace(u) bytes: the padded U (U^T) of direction 0, then of direction 1.
 * GN_EINVAL, nothing launched: a NULL table or entry, ld < u, T < 1, u < 1 or u > 512, B < 0, an unknown activation code; GN_EWORKSPACE: ws too
 * small.  B == 0 is GN_OK without a launch. */
int gn_lstm_pair_fwd(const float* const* zx, const float* const* U, const float* const* bias, float* const* h, float* const* gates, float* const* c,
                     float* const* hprev, void* ws, size_t ws_bytes, int B, int T, int u, int ld, int act, int ract, int reverse0, int seq, int training,
                     void* stream);
int gn_lstm_pair_bwd(const float* const* dy, const float* const* gates, const float* const* c, const float* const* U, float* const* dz, void* ws,
                     size_t ws_bytes, int B, int T, int u, int ld, int act, int ract, int reverse0, int dy_seq, void* stream);

/* ---- GRU recurrence (csrc/gru.hip; keras layers.GRU, GRUCell of keras 2.2.4, both reset_after forms).  Gate columns z, r, h of width u:
 *   a_t = zx_t + b;  reset_after 0: m = h_{t-1} . U[:, :2u], z = ra(a_z + m_z), r = ra(a_r + m_r), hh = act(a_h + (r h_{t-1}) . U_h)
 *                    reset_after 1: m = h_{t-1} . U + rb,    z = ra(a_z + m_z), r = ra(a_r + m_r), q = m_h, hh = act(a_h + r q)
 *   h_t = z h_{t-1} + (1 - z) hh
 * with enum gn_lstm_act's activation codes: act TANH, SIGMOID, RELU or LINEAR, ra HARD_SIGMOID or SIGMOID.  Ownership and numerics are the
 * LSTM recurrence's: one block carries 16 batch rows through all T steps, h stays on chip, the products run on v_mfma_f32_16x16x4_f32, no block
 * waits on another, no atomics.  Every recurrent pre-activation is one fp32 fma chain over k from +0, then + rb where there is one, then
 * + (zx + b), so a sample's results do not depend on B, on its tile or on the launch.  1 <= u <= 512; any B, T >= 1; 4-byte aligned pointers.
 * gn_gru_fwd: zx (B, T, 3u) = X . W, U (u, 3u), bias (3u), rbias (3u; required exactly under reset_after, not looked at otherwise), h0 (B, u) or
 *   NULL (zeros).  Step s reads zx at the input time t = s, or T-1-s under `reverse`, and writes h[:, s] (processing order).  With `training` it
 *   also stores at the INPUT time t: gates (B, T, 3u) = z, r, hh; hprev (B, T, u), the h that entered the step; aux (B, T, u) = r h_{t-1}
 *   (reset_after 0) or q (reset_after 1).
 * gn_gru_bwd: dy (B, T, u) in processing order (dy_seq) or (B, u) for the last step only; gates, hprev, aux as stored.  Walks the steps backwards
 *   and writes at the input time index dz (B, T, 3u) = da_z, da_r, da_h (dW = X^T dz, dX = dz W^T, db = sum dz) and, under reset_after, dzr
 *   (B, T, 3u) = da_z, da_r, dq (dU = hprev^T dzr, d rb = sum dzr; required exactly then).  reset_after 0: dU[:, :2u] = hprev^T dz[:, :2u],
 *   dU[:, 2u:] = aux^T dz[:, 2u:].  dh0 (B, u) when not NULL.
 * ws: gn_gru_fwd_workspace(u) / gn_gru_bwd_workspace(u) bytes (the zero-padded U / U^T the kernels read); 0 for a u out of range.
 * GN_EINVAL, nothing launched: a NULL pointer, T < 1, u < 1 or u > 512, B < 0, an unknown activation code, reset_after not 0 or 1;
 * GN_EWORKSPACE: ws too small.  B == 0 is GN_OK without a launch. */
size_t gn_gru_fwd_workspace(int u);
size_t gn_gru_bwd_workspace(int u);
int gn_gru_fwd(const float* zx, const float* U, const float* bias, const float* rbias, const float* h0, float* h, float* gates, float* hprev, float* aux,
               void* ws, size_t ws_bytes, int B, int T, int u, int act, int ract, int reset_after, int reverse, int training, void* stream);
int gn_gru_bwd(const float* dy, const float* gates, const float* hprev, const float* aux, const float* U, float* dz, float* dzr, float* dh0, void* ws,
               size_t ws_bytes, int B, int T, int u, int act, int ract, int reset_after, int reverse, int dy_seq, void* stream);

/* ---- a PAIR of GRU directions in one launch (csrc/gru.hip; keras layers.Bidirectional): gn_lstm_pair_fwd / _bwd's contract on the
 * GRU kernels.  blockIdx.y is the direction; host tables of two device pointers; direction 0 walks with reverse0 and writes step s at position
 * s, direction 1 walks with !reverse0 and writes it at position T-1-s; h / dy through `ld` >= u (two (B, T, u) buffers, or one (B, T, 2u) buffer
 * at columns 0 and u with ld = 2u); seq / dy_seq == 0: a (B, ld) row buffer for the last processed step.  Each direction is bit for bit what
 * gn_gru_fwd / gn_gru_bwd gives on the same operands; no initial state.  rbias and dzr (tables and entries) are required exactly under
 * reset_after; gates, hprev and aux may be NULL without `training`.  The stored tensors, dz and dzr are per direction, contiguous, at the input
 * time index.
 * ws: TWICE gn_gru_fwd_workspace(u) / gn_gru_bwd_workspace(u) bytes, direction 0 first.
 * GN_EINVAL, nothing launched: a NULL table or entry, ld < u, T < 1, u < 1 or u > 512, B < 0, an unknown activation code, reset_after not 0 or 1;
 * GN_EWORKSPACE: ws too small.  B == 0 is GN_OK without a launch. */
int gn_gru_pair_fwd(const float* const* zx, const float* const* U, const float* const* bias, const float* const* rbias, float* const* h, float* const* gates,
                    float* const* hprev, float* const* aux, void* ws, size_t ws_bytes, int B, int T, int u, int ld, int act, int ract, int reset_after,
                    int reverse0, int seq, int training, void* stream);
int gn_gru_pair_bwd(const float* const* dy, const float* const* gates, const float* const* hprev, const float* const* aux, const float* const* U,
                    float* const* dz, float* const* dzr, void* ws, size_t ws_bytes, int B, int T, int u, int ld, int act, int ract, int reset_after,
                    int reverse0, int dy_seq, void* stream);

/* ---- SimpleRNN recurrence (csrc/rnn.hip; keras layers.SimpleRNN, SimpleRNNCell of keras 2.2.4).  One gate block of width u:
 *   h_t = act((zx_t + b) + h_{t-1} . U)
 * with enum gn_lstm_act's activation codes TANH, SIGMOID, RELU or LINEAR; there is no recurrent activation.  Ownership and numerics are the
 * LSTM and GRU recurrences': one block carries 16 batch rows through all T steps, h stays on chip, the product runs on v_mfma_f32_16x16x4_f32,
 * no block waits on another, no atomics.  The recurrent pre-activation is one fp32 fma chain over k from +0, then + (zx + b), and dh_{t-1} one
 * chain over k, so a sample's results do not depend on B, on its tile or on the launch.  1 <= u <= 512; any B, T >= 1; 4-byte aligned pointers.
 * gn_rnn_fwd: zx (B, T, u) = X . W, U (u, u), bias (u), h0 (B, u) or NULL (zeros).  Step s reads zx at the input time t = s, or T-1-s under
 *   `reverse`, and writes h[:, s] (processing order).  With `training` it also stores at the INPUT time t: hs (B, T, u) = h_t, which the
 *   backward's act' reads, and hprev (B, T, u), the h that entered the step (h0 at the first); without it nothing but h is written and hs and
 *   hprev may be NULL.
 * gn_rnn_bwd: dy (B, T, u) in processing order (dy_seq) or (B, u) for the last step only; hs as stored.  Walks the steps backwards,
 *   dz_t = (dy_t + dh_t) act'(h_t), dh_{t-1} = dz_t . U^T, and writes dz (B, T, u) at the input time index (dW = X^T dz, dU = hprev^T dz,
 *   dX = dz W^T, db = sum dz); dh0 (B, u) when not NULL.
 * ws: gn_rnn_fwd_workspace(u) / gn_rnn_bwd_workspace(u) bytes (the zero-padded U / U^T the kernels read); 0 for a u out of range.
 * GN_EINVAL, nothing launched: a NULL pointer, T < 1, u < 1 or u > 512, B < 0, an unknown or HARD_SIGMOID activation code; GN_EWORKSPACE: ws too
 * small.  B == 0 is GN_OK without a launch. */
size_t gn_rnn_fwd_workspace(int u);
size_t gn_rnn_bwd_workspace(int u);
int gn_rnn_fwd(const float* zx, const float* U, const float* bias, const float* h0, float* h, float* hs, float* hprev, void* ws, size_t ws_bytes, int B,
               int T, int u, int act, int reverse, int training, void* stream);
int gn_rnn_bwd(const float* dy, const float* hs, const float* U, float* dz, float* dh0, void* ws, size_t ws_bytes, int B, int T, int u, int act,
               int reverse, int dy_seq, void* stream);

/* ---- a PAIR of SimpleRNN directions in one launch (csrc/rnn.hip; keras layers.Bidirectional): gn_gru_pair_fwd / _bwd's contract on
 * the SimpleRNN kernels.  blockIdx.y is the direction; host tables of two device pointers; direction 0 walks with reverse0 and writes step s at
 * position s, direction 1 walks with !reverse0 and writes it at position T-1-s; h / dy through `ld` >= u (two (B, T, u) buffers, or one
 * (B, T, 2u) buffer at columns 0 and u with ld = 2u); seq / dy_seq == 0: a (B, ld) row buffer for the last processed step.  Each direction is
 * bit for bit what gn_rnn_fwd / gn_rnn_bwd gives on the same operands; no initial state.  hs and hprev (tables and entries) may be NULL without
 * `training`.  The stored tensors and dz are per direction, contiguous, at the input time index.
 * ws: TWICE gn_rnn_fwd_workspace(u) / gn_rnn_bwd_workspace(u) bytes, direction 0 first.
 * GN_EINVAL, nothing launched: a NULL table or entry, ld < u, T < 1, u < 1 or u > 512, B < 0, an unknown or HARD_SIGMOID activation code;
 * GN_EWORKSPACE: ws too small.  B == 0 is GN_OK without a launch. */
int gn_rnn_pair_fwd(const float* const* zx, const float* const* U, const float* const* bias, float* const* h, float* const* hs, float* const* hprev,
                    void* ws, size_t ws_bytes, int B, int T, int u, int ld, int act, int reverse0, int seq, int training, void* stream);
int gn_rnn_pair_bwd(const float* const* dy, const float* const* hs, const float* const* U, float* const* dz, void* ws, size_t ws_bytes, int B, int T,
                    int u, int ld, int act, int reverse0, int dy_seq, void* stream);

/* ---- depthwise 1-D convolution (csrc/depthwise.hip; the depthwise half of keras layers.SeparableConv1D).  Channels-last fp32:
 * x (B, L, C), w (k, C, dm) = keras' depthwise_kernel, y / dy (B, Lout, C dm) with output channel c dm + m (tf.nn.depthwise_conv2d's order):
 *   y[b, l, c dm + m] = sum_t x[b, l stride - pad_left + t dilation, c] * w[t, c, m]          (x outside [0, L) is 0)
 *   dx[b, i, c]       = sum over the (t, m) with (i + pad_left - t dilation) % stride == 0 and that quotient in [0, Lout) of dy * w   (gather form)
 *   dw[t, c, m]       = sum_{b, l} x[b, l stride - pad_left + t dilation, c] * dy[b, l, c dm + m]
 * Three streaming passes, a thread per output, no atomics; C dm % 4 == 0 (dgrad: C % 4 == 0) on 16-byte aligned pointers moves 16 bytes a lane,
 * anything else runs the scalar form of the same kernels.  Any C, k, dm, stride, dilation >= 1, pad_left >= 0, L, Lout >= 1 (rows outside the
 * input are padding whatever Lout is), stride > 1 together with dilation > 1 included.  Every y is one fp32 fmaf chain from +0 over t, every dx
 * one over (t, m) with t outer, both skipping the padding: a sample's y and dx do not depend on B, on the block or on the launch.
 * gn_dwconv1d_wgrad: a block sums its own rows (a thread's fp32 fmaf chain over its rows in ascending order, the row lanes added in fp64 in lane
 *   order) into ws, and the fixed-order fp64 pass behind gn_bias_grad sums the parts: bit-identical from run to run.
 *   ws: gn_dwconv1d_wgrad_workspace(B, Lout, C, k, dm) bytes, 8-byte aligned (host only; 0 for a shape out of range or B == 0).
 * GN_EINVAL, nothing launched: a NULL pointer, B < 0, any of L, C, k, dm, stride, dilation, Lout < 1, pad_left < 0, k * C * dm >= 2^31,
 * B * L * C or B * Lout * C * dm >= 2^62, a workspace that is not 8-byte aligned; GN_EWORKSPACE: ws too small.  B == 0 is GN_OK without a launch. */
size_t gn_dwconv1d_wgrad_workspace(int B, int Lout, int C, int k, int dm);
int gn_dwconv1d_fwd(const float* x, const float* w, float* y, int B, int L, int C, int k, int dm, int stride, int dilation, int pad_left, int Lout,
                    void* stream);
int gn_dwconv1d_dgrad(const float* dy, const float* w, float* dx, int B, int L, int C, int k, int dm, int stride, int dilation, int pad_left, int Lout,
                      void* stream);
int gn_dwconv1d_wgrad(const float* x, const float* dy, float* dw, void* ws, size_t ws_bytes, int B, int L, int C, int k, int dm, int stride, int dilation,
                      int pad_left, int Lout, void* stream);

/* ---- sequence plumbing (csrc/sequence.hip; keras layers.Permute, RepeatVector, Cropping1D, ZeroPadding1D).  Contiguous fp32, out of
 * place, memory-bound passes; no atomics, no host synchronisation; float4 units where the inner extent is a multiple of 4 and both tensors are
 * 16-byte aligned, else floats.
 *   gn_permute: axis i of y is axis perm[i] of x, for R = 2 .. 4 axes (the batch axis is axis 0); extents are x's.  extents_host and perm_host are
 *     HOST arrays of R ints, read when the entry point runs.  Axes of extent 1 are dropped and axes that stay adjacent and in order merged; then a
 *     device-to-device copy (nothing left to permute), a row copy (the innermost axis stays innermost) or a tiled transposition through LDS (it
 *     changes), batched over the remaining axes.  The backward of a permutation is this entry with the inverse permutation.
 *   gn_repeat_fwd: x (B, C) -> y (B, n, C), y[b, j, :] = x[b, :].
 *   gn_repeat_bwd: dy (B, n, C) -> dx (B, C), dx[b, c] = sum_j dy[b, j, c] in fp64, j ascending, rounded once; where B C is small and n large j is cut
 *     into chunks, by (B, n, C) alone, whose fp64 partial sums are added in ascending order: bit-identical from run to run.
 *     ws: gn_repeat_bwd_workspace(B, n, C) bytes, 8-byte aligned (0 bytes: ws may be NULL).
 *   gn_shift1d: x (B, Lin, C) -> y (B, Lout, C), y[b, l, :] = x[b, l - offset, :] where 0 <= l - offset < Lin, +0.0f elsewhere.  ZeroPadding1D is
 *     offset = left, Lout = left + Lin + right; Cropping1D offset = -left, Lout = Lin - left - right; the backward of each is the other's forward.
 * GN_EINVAL, nothing launched: a NULL pointer (except ws as above), y == x, R outside 2 .. 4, a perm that is no permutation of 0 .. R - 1, a negative
 * extent, 2^61 elements or more, a merged axis of 2^31 elements or more, B < 0, any of n, C, Lin, Lout < 1, n C >= 2^31; GN_EWORKSPACE: ws too
 * small.  An extent of 0 / B == 0 is GN_OK without a launch. */
int gn_permute(const float* x, float* y, const int* extents_host, const int* perm_host, int R, void* stream);
int gn_repeat_fwd(const float* x, float* y, int B, int n, int C, void* stream);
size_t gn_repeat_bwd_workspace(int B, int n, int C);
int gn_repeat_bwd(const float* dy, float* dx, void* ws, size_t ws_bytes, int B, int n, int C, void* stream);
int gn_shift1d(const float* x, float* y, int B, int Lin, int Lout, int C, int offset, void* stream);

/* ---- losses + metric (compile(loss='binary_crossentropy'|'mean_squared_error', metrics=['accuracy']),
 *      bbhMahoGANy.py:1101-1119) ---------------------------------------------------------------------------
 * p, y: (B, 1).  out[0] = loss (mean over the local B rows scaled by B/Bglobal), out[1] = #rows with round(p)==y;
 * dp = dLoss/dp with the mean taken over Bglobal rows (data-parallel ranks pass the global batch size). */
int gn_bce_loss(const float* p, const float* y, float* dp, float* out, int B, int Bglobal, void* stream);
int gn_mse_loss(const float* p, const float* y, float* dp, float* out, int B, int Bglobal, void* stream);

/* ---- every Keras 2.2.4 loss / metric of compile(loss=, metrics=) as one streaming pass over a (rows, cols) output of any size
 *      (gennet_amd/csrc/loss.hip; DESIGN.md section 8e lists the per-row terms and derivatives) -------------------------------
 * out[0] = sum over the local rows of the per-row term / denom (denom: the GLOBAL row count, data-parallel ranks pass B * world);
 * out[1] = #elements with round(p) == y.  dp (may be NULL: evaluation / metric form, only `out` is written) = d out[0] / dp, one
 * store per element.  GN_LOSS_CATEGORICAL_ACCURACY: out[0] = #rows whose first arg-max of p is the first arg-max of y / denom, dp = 0.
 * The grid scales with rows * cols; blocks write fp64 partials to `ws` (gn_loss_pass_workspace bytes, 8-byte aligned) with plain
 * stores and a one-block kernel adds them in a fixed order: no atomics, the same bits on every run, a launch shape that depends on
 * (rows, cols) only.  p, y, dp need 4-byte alignment only.  GN_EINVAL: unknown kind, rows < 1, cols < 1, denom < rows, a workspace
 * that is too small, NULL p / y / out. */
enum gn_loss {
  GN_LOSS_BINARY_CROSSENTROPY = 0, GN_LOSS_MEAN_SQUARED_ERROR = 1, GN_LOSS_MEAN_ABSOLUTE_ERROR = 2, GN_LOSS_MEAN_ABSOLUTE_PERCENTAGE_ERROR = 3,
  GN_LOSS_MEAN_SQUARED_LOGARITHMIC_ERROR = 4, GN_LOSS_HINGE = 5, GN_LOSS_SQUARED_HINGE = 6, GN_LOSS_LOGCOSH = 7, GN_LOSS_POISSON = 8,
  GN_LOSS_KULLBACK_LEIBLER_DIVERGENCE = 9, GN_LOSS_CATEGORICAL_CROSSENTROPY = 10, GN_LOSS_COSINE_PROXIMITY = 11,
  GN_LOSS_CATEGORICAL_ACCURACY = 12, GN_LOSS_KINDS = 13
};
size_t gn_loss_pass_workspace(long long rows, int cols);
int gn_loss_pass(int kind, const float* p, const float* y, float* dp, float* out, long long rows, int cols, double denom,
                 void* ws, size_t ws_bytes, void* stream);

/* ---- the weighted form of the pass: Keras' sample_weight / class_weight / weighted_metrics ----------
 * w: one float per local row.  count: ONE double in device memory, the number of non-zero weights of the GLOBAL batch, read by the
 * kernels (never by the host): gn_weight_count writes the local count, data-parallel ranks all-reduce it before the pass, and a
 * captured step replays with new weights.  gn_weight_count: exact, fixed-order, no atomics, a launch shape that depends on `rows`
 * only; its workspace holds gn_weight_count_workspace(rows) bytes, 8-byte aligned.
 * gn_loss_pass_weighted, out[3]: out[0] = sum over the local rows of w_r * (per-row term) / count; out[1] = #elements with
 * round(p) == y (unweighted, as gn_loss_pass); out[2] = sum over the local rows of w_r * (the row's hits) / (count * cols).
 * dp (may be NULL, the same `out` bits) = d out[0] / dp, one store per element, rows of weight zero included (+-0).  Negative
 * weights count as non-zero; count == 0 gives 0 / 0 = NaN, as Keras does.  Everything else as gn_loss_pass: fp64 terms on the fp32
 * inputs, one rounding, fp64 partials in `ws` (gn_loss_pass_weighted_workspace bytes, 8-byte aligned), the same bits on every run, a
 * grid that depends on (rows, cols) only; p, y, w, dp need 4-byte alignment only.  GN_EINVAL: unknown kind, rows < 1, cols < 1, a
 * workspace that is too small or misaligned, NULL p / y / w / count / out. */
size_t gn_weight_count_workspace(long long rows);
int gn_weight_count(const float* w, long long rows, double* count, void* ws, size_t ws_bytes, void* stream);
size_t gn_loss_pass_weighted_workspace(long long rows, int cols);
int gn_loss_pass_weighted(int kind, const float* p, const float* y, const float* w, const double* count, float* dp, float* out,
                          long long rows, int cols, void* ws, size_t ws_bytes, void* stream);

/* ---- Adam, keras form (bbhMahoGANy.py:1101,1107,1115,1119: Adam(lr=9e-5, beta_1=0.5)) ---------------------
 * m = b1*m + (1-b1)*g; v = b2*v + (1-b2)*g*g; p -= lr_t * m / (sqrt(v) + eps), lr_t = lr*sqrt(1-b2^t)/(1-b1^t) (host). */
int gn_adam_step(float* p, const float* g, float* m, float* v, size_t n, float lr_t, float b1, float b2, float eps, void* stream);

/* ---- Keras 2.2.4 optimizers beyond the default Adam pass --------------------------------------------------
 * bbhMahoGANy.py:43 imports RMSprop, Adagrad, Adadelta, Adamax; the earlier GenNet versions train with SGD(lr=lr)
 * (2_model_version/no_weight_code/noise_gan.py:75, subtract_model.py:211, ht_noise_subtract_version/nn.py:123), and the reference's
 * g_model.hdf5 (tests/golden/keras_h5/) was compiled with SGD.  One fused pass per segment: p, g and the rule's state are read once,
 * p and the state written once.  lr is this step's lr_eff = lr / (1 + decay * iterations) (SGD, RMSprop, Adagrad, Adadelta) or
 * lr_t = lr_eff sqrt(1 - b2^t) / (1 - b1^t) (Adam) | lr_eff / (1 - b1^t) (Adamax), computed on the host; with lr_dev != NULL it is read
 * from device memory instead (a captured step).  Before the rule, g <- g * (*clip_scale) when clip_scale != NULL, then
 * g <- clip(g, -clipvalue, clipvalue) when clipvalue > 0.  State arrays (s0, s1, s2) by rule, NULL where unused:
 *   GN_OPT_SGD      m              h0 = momentum (nesterov 0 | 1)
 *   GN_OPT_RMSPROP  a              h0 = rho
 *   GN_OPT_ADAGRAD  a
 *   GN_OPT_ADADELTA a, d           h0 = rho
 *   GN_OPT_ADAMAX   m, u           h0 = beta_1, h1 = beta_2
 *   GN_OPT_ADAM     m, v           h0 = beta_1, h1 = beta_2
 *   GN_OPT_AMSGRAD  m, v, vhat     h0 = beta_1, h1 = beta_2
 * n == 0 is a no-op; any n and alignment (float4 body where the arrays are mutually 16-byte aligned). */
enum gn_optim_rule { GN_OPT_SGD = 0, GN_OPT_RMSPROP = 1, GN_OPT_ADAGRAD = 2, GN_OPT_ADADELTA = 3, GN_OPT_ADAMAX = 4, GN_OPT_ADAM = 5, GN_OPT_AMSGRAD = 6 };
int gn_optim_step(int rule, float* p, const float* g, float* s0, float* s1, float* s2, size_t n, float lr, const float* lr_dev, float h0, float h1,
                  float eps, int nesterov, const float* clip_scale, float clipvalue, void* stream);
/* Keras' clipnorm (optimizers.py get_gradients) over ALL trained weights of a compiled model, without host synchronisation or atomics:
 * gn_optim_sumsq writes gn_optim_sumsq_slots(n) fp64 partial sums of g^2 of one segment to partials[0 ..); gn_optim_clip_factor adds
 * `count` partials in a fixed order and writes *factor = clipnorm / norm if norm >= clipnorm, else 1 (fp32; norm = sqrt(sum) in fp32). */
size_t gn_optim_sumsq_slots(size_t n);
int gn_optim_sumsq(const float* g, size_t n, double* partials, void* stream);
int gn_optim_clip_factor(const double* partials, size_t count, float clipnorm, float* factor, void* stream);

/* ---- Keras weight and activity regularizers (gennet_amd/csrc/regularizer.hip): regularizers.l1 / l2 / l1_l2 on a
 * weight (kernel_regularizer, bias_regularizer, beta_, gamma_, alpha_) or on a layer's output (activity_regularizer, ActivityRegularization).
 * The penalty of a tensor x of n floats is l1 * sum |x| + l2 * sum x^2, its gradient l1 * sign(x) + 2 * l2 * x with sign(+-0) = 0.
 *   gn_reg_pass    reads x once; writes gn_reg_partials(n) fp64 block partials of the penalty (terms formed in fp64) to partials[0 ..) with
 *                  plain stores and, with g != NULL, g[i] += l1 * sign(x[i]) + 2 * l2 * x[i] (fp32, three roundings).  g == NULL: penalty only
 *                  (a frozen weight, the test phase), nothing but the partials is written.
 *   gn_reg_grad    the gradient part alone (the activity backward): gout[i] = gin[i] + l1 * sign(y[i]) + 2 * l2 * y[i]; gout may be gin.
 *   gn_reg_finish  one block: adds `count` partials -- those of every penalty of a step, side by side -- in a fixed order and writes one
 *                  fp32 scalar, rounded once.
 * No atomics: two runs give the same bits.  The launch shape and gn_reg_partials depend on n only.  Any 4-byte alignment: 16-byte loads and
 * stores where the tensors of a pass share a 16-byte phase (a scalar head and tail around them), scalar ones otherwise.
 * GN_EINVAL, nothing launched: a NULL pointer (except gn_reg_pass' g), n == 0 (count == 0), a negative or non-finite l1 / l2, n_partials <
 * gn_reg_partials(n), partials not 8-byte aligned. */
size_t gn_reg_partials(size_t n);
int gn_reg_pass(const float* x, float* g, size_t n, float l1, float l2, double* partials, size_t n_partials, void* stream);
int gn_reg_grad(const float* y, const float* gin, float* gout, size_t n, float l1, float l2, void* stream);
int gn_reg_finish(const double* partials, size_t count, float* out, void* stream);

/* ---- hipGraph capture of a whole train step (bbhMahoGANy.py:1153-1168, :1241-1299 at the script's own batch size 8, where the loop is
 * launch-bound): every launch of the library is stream-ordered and allocation-free, so train_on_batch can be captured on the launch stream and
 * replayed.  Scalars that change from step to step would be frozen into the graph as by-value kernel arguments; these entry points read them
 * from device memory instead (the host refreshes one small block before each replay).
 * gn_set_rng_base: from now on (this host thread) every Philox kernel of the library -- gn_dropout_mask, gn_fill_uniform, gn_fill_normal(_dyn),
 * gn_bn_apply_dropgen, gn_gaussian_noise_fwd, gn_gaussian_dropout_apply, gn_alpha_dropout_fwd, gn_alpha_dropout_bwd -- adds *base_dev to its counter offset at run time; NULL switches it off.  With base = (stream position at replay) -
 * (stream position at capture) a replay draws exactly what the un-captured step would have drawn. */
int gn_set_rng_base(const uint64_t* base_dev);
/* gn_adam_step with lr_t = lr sqrt(1 - b2^t) / (1 - b1^t) read from device memory */
int gn_adam_step_dyn(float* p, const float* g, float* m, float* v, size_t n, const float* lr_t_dev, float b1, float b2, float eps, void* stream);
/* gn_fill_normal with the standard deviation read from device memory (the CNN loop's per-batch sigma ~ U(0, 5), bbhMahoGANy.py:1161) */
int gn_fill_normal_dyn(float* out, size_t n, float mean, const float* sd_dev, uint64_t seed, uint64_t offset, void* stream);
/* gn_bn_finalize_zero_debias with the (already incremented) local_step read from device memory */
int gn_bn_finalize_zero_debias_dyn(const double* sums, double count, const float* gamma, const float* beta, float eps, float momentum,
                                   float* moving_mean, float* moving_var, float* biased_mean, float* biased_var, const int32_t* local_step_dev,
                                   float* scale, float* shift, float* save_mean, float* save_invstd, int C, void* stream);

/* ---- profiling hooks used by bench.py: accumulate HIP-event time of every MFMA conv / wgrad launch ---------- */
int gn_prof_enable(int on);
int gn_prof_reset(void);
/* sums over launches since reset of one kernel family (kind 0 = conv_mfma_kernel: forward + data gradient,
 * 1 = wgrad_mfma_kernel, 9 = the anyc conv, 10 = the anyc weight gradient, 11 .. 17 = the small-channel
 * kernels of small_conv.hip, one kind each, -1 = all): out[0] = launches, out[1] = total ms, out[2] = total algorithmic FLOP,
 * out[3] = total algorithmic bytes (each operand read once, the result written once) */
int gn_prof_collect(int kind, double* out4_host);

/* ---- template synthesiser (gw_template_maker.py) --------------------------------------------------------- */
/* Closed-form frequency-domain IMR chirp (this library's own model, NOT LAL IMRPhenomPv2; replaces the call at
 * gw_template_maker.py:507-516) fused with whiten_data(...,'fd') (:243-286, :518-519):
 *   out_hp/out_hc[(b, f)] complex128 interleaved (re,im), Nf = N/2+1 bins, bin f <-> f*df; zero below f_low and at DC.
 *   scale[f] = sqrt(2*invpsd[f]/fs) precomputed by the caller from the PSD (0 where psd <= 0). */
int gn_chirp_fd_whitened(const double* m1, const double* m2, const double* scale, double* out_hp, double* out_hc,
                         int nb, int Nf, double df, double f_low, double dist_mpc, double iota, double phi0, void* stream);
/* Batched real FFTs with numpy semantics (np.fft.irfft at gw_template_maker.py:191,:283,:521-522,:775-777; np.fft.rfft
 * at :268).  irfft: X (nb, N/2+1) complex128 -> out (nb, N) float64, 1/N normalisation, imaginary parts of DC/Nyquist
 * ignored.  rfft: x (nb, N) -> X (nb, N/2+1).  N a power of two, 16 <= N <= 16384.
 * twiddle: N/2 complex128 values exp(+2*pi*i*k/N), k = 0..N/2-1, computed once by the caller (fp64 on the host). */
int gn_irfft_f64(const double* X, double* out, const double* twiddle, int nb, int N, void* stream);
int gn_rfft_f64(const double* x, double* X, const double* twiddle, int nb, int N, void* stream);
/* gen_bbh alignment (gw_template_maker.py:521-565) for a batch: given hp, hc = irfft(...) (nb, N):
 *   ref = argmax_n (hp^2+hc^2)[(n - fs) mod N-rolled]  (first maximum, as numpy.argmax after np.roll(.,-fs));
 *   out[b, n] = g * (Fp*hp + Fc*hc)_rolled[ref - idx[b] - peak_off + crop0 + n], n in [0, crop_len), 0 past the end.
 *   ref_out[b] receives ref. */
int gn_align_crop(const double* hp, const double* hc, const int32_t* idx, double* out, int32_t* ref_out,
                  int nb, int N, int roll, int crop0, int crop_len, int peak_off, double Fp, double Fc, double g, void* stream);
/* gen_bbh + the crop of sim_data for a batch, FUSED (gw_template_maker.py:507-565, :695): one workgroup per template evaluates the
 * whitened chirp spectrum once (the same closed form as gn_chirp_fd_whitened), obtains both polarisations from M = N/2-point
 * complex inverse FFTs resident in LDS, finds ref = argmax(hp^2 + hc^2) of the rolled series (first maximum) and writes
 *   out[b, n] = g * (Fp*hp + Fc*hc)_rolled[ref - idx[b] - peak_off + crop0 + n],  n in [0, crop_len), 0 past the end
 * to out_f64 and/or out_f32 (either may be NULL; not both) and ref to ref_idx (may be NULL).  No intermediate spectrum or time
 * series ever reaches HBM.  scale: (N/2+1,) whitening scale sqrt(2/(psd*fs)) (0 where psd <= 0; gw_template_maker.py:273-281);
 * twiddle as for gn_irfft_f64.  N in {1024, 2048, 4096, 8192, 16384}. */
int gn_synth_templates(const double* m1, const double* m2, const int32_t* idx, const double* scale, const double* twiddle,
                       double* out_f64, float* out_f32, int32_t* ref_idx, int nb, int N, int roll, int crop0, int crop_len,
                       int peak_off, double df, double f_low, double dist_mpc, double iota, double phi0, double Fp, double Fc, double g,
                       void* stream);
/* The same kernel with the PRIOR drawn inside it (BASELINE configs[4]: synthesis fused into the training loop): every template draws
 * (m1, m2) from gen_masses('hunt_constrain') (gw_template_maker.py:327-339: log-uniform component masses in [m_min, M_max - m_min]
 * subject to m1 + m2 < M_max, m1 >= m2, m2/m1 >= 0.5, 20 <= mc <= 35, by rejection) and idx uniformly from [idx_lo, idx_hi)
 * (gen_par :422-426) from a counter-based Philox stream: template b uses counters counter + 1024*b .. counter + 1024*b + 1023 of
 * stream `seed`, the lowest accepted trial wins, so a batch is a pure function of (seed, counter) and ranks / steps take disjoint
 * counter ranges (advance by 1024 per template).  Not the reference's MT19937 stream (statistical parity only).
 * labels (nb, 2) = [mc, m2/m1] fp32, m_out (nb, 2) = [m1, m2], idx_out (nb,): each may be NULL. */
int gn_synth_templates_prior(const double* scale, const double* twiddle, double* out_f64, float* out_f32, float* labels, double* m_out,
                             int32_t* idx_out, int32_t* ref_idx, int nb, int N, int roll, int crop0, int crop_len, int peak_off,
                             double df, double f_low, double dist_mpc, double iota, double phi0, double Fp, double Fc, double g,
                             uint64_t seed, uint64_t counter, int idx_lo, int idx_hi, double m_min, double M_max, void* stream);
/* PSD-coloured Gaussian noise generated AND whitened in one launch, one workgroup per row, nothing but the crop written (BASELINE
 * configs[4]): replaces gen_noise (gw_template_maker.py:161-193: amp = sqrt(0.25 T psd), 0 where psd == 0; re, im = amp * N(0,1), Nf draws
 * each, re block first; DC = 0; x = N * irfft(re + i im) * df) followed by whiten_data(x, flag='td') (:243-286: rfft(tukey(N, 1/8) * x) *
 * sqrt(2 invpsd / fs), DC = 0, irfft) and the crop [crop0, crop0 + crop_len) of sim_data (:695), all fp64 in LDS.
 * amp, wscale: (N/2+1) tables; window: (N) tukey(N, 1/8); twiddle as for gn_irfft_f64.  normals_in (nb, 2 (N/2+1)) = numpy's draws per row
 * [re block | im block], or NULL: Philox (bin k of row b = counter + b (N/2+1) + k of stream `seed`, Box-Muller -> (re, im)); normals_out
 * (same layout) or NULL receives the normals used.  add_f64 (nb, crop_len) or NULL: rows the noise is added to (template crops).
 * out_f64 / out_f32 (nb, crop_len): at least one.  N in {1024, 2048, 4096, 8192, 16384}. */
int gn_noise_whitened(const double* amp, const double* wscale, const double* window, const double* twiddle, const double* normals_in,
                      double* normals_out, const double* add_f64, double* out_f64, float* out_f32, int nb, int N, int crop0, int crop_len,
                      double df, uint64_t seed, uint64_t counter, void* stream);
/* gn_synth_templates / gn_synth_templates_prior (m1 == m2 == idx == NULL: prior mode) with that noise chain run by the SAME workgroup after
 * the template's crop is formed: out = template * g + whitened coloured noise, one launch per batch (BASELINE configs[4]: "template + noise
 * synth fused into the train loop").  scale doubles as the whitening scale of the noise; noise_amp, window as for gn_noise_whitened; the
 * noise stream is (noise_seed, noise_counter), row b bin k = noise_counter + b (N/2+1) + k.  crop_len <= N/4. */
int gn_synth_templates_noise(const double* m1, const double* m2, const int32_t* idx, const double* scale, const double* twiddle,
                             const double* noise_amp, const double* window, double* out_f64, float* out_f32, float* labels, double* m_out,
                             int32_t* idx_out, int32_t* ref_idx, int nb, int N, int roll, int crop0, int crop_len, int peak_off, double df,
                             double f_low, double dist_mpc, double iota, double phi0, double Fp, double Fc, double g, uint64_t seed,
                             uint64_t counter, int idx_lo, int idx_hi, double m_min, double M_max, uint64_t noise_seed,
                             uint64_t noise_counter, double* normals_out, void* stream);
/* gen_noise (gw_template_maker.py:161-193) spectrum: X[b,f] = amp[f]*(xi_re + i xi_im), DC = 0 (Philox normals, re block then im block) */
int gn_noise_fd(const double* amp, double* X, int nb, int Nf, uint64_t seed, uint64_t offset, void* stream);
/* x *= s (fp64), used for N*df and gw_norm_constant scalings; and fp64 -> fp32 narrowing with scale */
int gn_scale_f64(double* x, double s, size_t n, void* stream);
/* x[i] *= w[e % period], e = i (real x) or i/2 (complex_x: interleaved re/im): whiten_data's xf *= sqrt(2*invpsd/fs)
 * (:276) and the Tukey window of the 'td' path (:267-268) over a batch */
int gn_mul_f64(double* x, const double* w, size_t n, size_t period, int complex_x, void* stream);
int gn_f64_to_f32(const double* x, float* y, double s, size_t n, void* stream);

/* ---- posterior read-out score (bbhMahoGANy.py:811-873 overlap_tests; kernel.pdf(positions) at :861,:866) -------------
 * 2-D Gaussian KDE: out[p] = norm * sum_i exp(-0.5 * d^T Sinv d), d = pts[:,p] - data[:,i]; data (2,n), pts (2,m) row-major fp64;
 * Sinv = [[inv00, inv01],[inv01, inv11]] and norm = 1/(n*sqrt(det(2*pi*Sigma))) as scipy.stats.gaussian_kde defines them. */
int gn_kde2d_pdf(const double* data, int n, const double* pts, int m, double inv00, double inv01, double inv11, double norm,
                 double* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GENNET_HIP_H */
