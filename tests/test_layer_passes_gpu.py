"""GPU parity of the passes AROUND the convolutions, at the sizes where their code changes path: Dense on each of its three routes, the
fp64 column reductions and the BatchNormalization passes at uneven channel counts, the streaming passes across their grid-stride trip
and float4 tail, the one-block losses, and the device-scalar variants of three entry points.  References: oracle/keras_ref.py and
tests/layer_ref.py (fp64 numpy on the fp32 inputs).  Conventions (g / f32 / close) and tolerances are those of test_kernels_gpu.py: 2e-5
of the largest oracle magnitude for outputs and data gradients (fp32 fmaf chains of up to 4100 terms), 5e-5 for weight / bias gradients.

Which case reaches which seam (gennet_amd/csrc: capi.hip gn_dense_fwd / gn_dense_bwd, small_conv.hip; bn.hip for the column reductions, the bias
gradients and the BatchNormalization passes, elementwise.hip for the streaming passes, loss.hip for the one-block losses, optim.hip for
Adam).  The matrix-core
route is asserted with the launch counters; the small head and the any-shape GEMM have no counter (the tests only assert that they launch no
counted kernel), so which of the two a shape takes is read off gn_dense_fwd / gn_dense_bwd: dense_any_shape(in, out) first, then out <= 4.

Dense
  small head (out <= 4, in % 4 == 0: dense_small_fwd_kernel<OUT> / dense_small_bwd_kernel<OUT>; no counted launch)
    out 1, 2, 3, 4          every template member, forward and backward
    in 4                    one thread of the forward's 1024 and of the backward's one block has work
    in 1020                 255 of the backward block's 256 threads
    in 4096 / 4100          exactly one / the start of a second 4096-feature trip of the forward; 4 full backward blocks / a fifth with one thread
    B 1, 8, 9, 17           below, exactly, one past and two trips past the 8-row unroll of the backward (rows past B are clamped loads)
    prev=(...)              gn_dense_bwd_fused: the producer's [activation -> dropout] backward in the dx store, with and without a mask
  any-shape GEMM (in % 4 or out % 4, beyond the heads: dense_any_kernel, 16 x 16 tiles; no counted launch)
    (1,1,5)                 one row, one k, part of one tile          (15,17,33)  ragged M tile, k tile + 1, two column tiles + 1
    (16,16,6)               exact M and k tile, ragged N              (17,15,16)  M tile + 1, ragged k, exact N
    (33,50,3) (4,6,1)       out <= 4 with in % 4 != 0: NOT the small head; db on the small-C sum of bias_grad (colsum_anyc_kernel)
    (40,913,50)             the g_model layer's depth (58 k tiles, the last with one column)
  matrix-core route (in % 4 == 0 and out % 4 == 0, out > 4: conv_mfma / wgrad_mfma, launch counters 0 and 1)
    (1,4,8)                 the narrowest aligned widths; its data gradient has 4 output channels and runs on the small-channel kernel
    (33,8,12) (17,100,36)   half a K chunk / 6.25 K chunks of 16, column tiles a fraction of 64

Column reductions, C / 4 = NQ quads, NQc = min(NQ, 256) quads and RL = 256 / NQc row lanes per block (colred_kernel, bn_bwd_apply_v4_kernel)
    C 4                     NQ 1: 256 row lanes              C 12   NQ 3,  RL 85: thread 255 idle (rl >= RL)
    C 20                    NQ 5,  RL 51: 1 idle thread      C 100  NQ 25, RL 10: 6 idle threads
    C 1028                  NQ 257: a second quad-block holding ONE quad        C 1280  NQ 320: a second quad-block holding 64 of 256
    rows 2, 7               C <= 100: one chunk, fewer rows than row lanes; C >= 1028 (RL 1): 2 rows are one 2-row trip, 7 rows two chunks (4 + 3)
    rows 257, 3001          chunks = min(1024 / quad-blocks, ceil(rows / 4 RL)): C 4 -> 1, 3; C 12 -> 1, 9; C 20 -> 2, 15; C 100 -> 7, 76;
                            C 1028, 1280 -> 65, 512; the last chunk short wherever rows is no multiple of the chunk (e.g. C 100, 3001: 75 x 40 + 1)
    rows 2                  BatchNormalization's dx over 2 rows is gamma inv (g1 - g2) / 2 (1 - xhat^2): a near-total cancellation, so the
                            largest |dx| the 1e-4 tolerance is relative to is small; the worst measured error there is 8.1e-5 of it (C 4:
                            81 % of the bound, fp32 rounding of g - mean g - xhat mean(g xhat), not a kernel fault).  Read a later failure
                            of a rows = 2 case with that margin in mind.
  on-the-fly 1-filter conv gradient: every C here has NQ % 64 == 0, the wave-uniform window path (lazy_dy4<true>)
    C 256                   RL 4 (a wave per row lane)       C 768   NQc 192, RL 1: the fourth wave of each block idle
    C 1280                  second quad-block of one wave    C 2048  two full quad-blocks
    (96, 1024, 256)         colred_chunks gives 96 rows per chunk: each wave walks 24 rows 4 apart, so its 64-wide window on g is reloaded inside
                            the chunk, and 1024 is no multiple of 96, so chunks straddle segment ends (window reload on the segment change).
                            The window of bn_bwd_apply_v4_kernel would only slide with more than 64 rows per chunk and lane; its launch makes
                            ~8192 chunks, i.e. from ~2 M rows on -- out of reach of a unit test, and not emulated here.

Streaming passes (grid capped at 2048 blocks of 256 threads: 2^19 threads)
    n 1, 3                  tail only                        n 4  one float4, no tail            n 5, 1003  float4 body and tail
    n 2^21 + 5              2^19 + 1 float4 items: a second grid-stride trip, together with a one-element tail
    (3, 200003) (2, 300001) 600009 / 1200004 items of the stack / batch-assembly kernels: second and third trip, i % n across row ends
    700000 x 1              gather: a second trip

Losses (loss_kernel, one block of 256 threads)
    B 1, 255, 256, 257      one thread, one short of a full pass, exactly one, one element of a second pass
    100000                  the engine's flattened B * columns form: 391 terms per thread
"""
import numpy as np
import pytest
import torch

import conv_family as CF
import layer_ref as R
from oracle import keras_ref as K

pytestmark = pytest.mark.gpu

RTOL = 2e-5
ACTS = [('linear', 0.0), ('relu', 0.0), ('relu_max', 1.0), ('leaky', 0.2), ('tanh', 0.0), ('sigmoid', 0.0)]

def dev():
    return torch.device('cuda:0')


def g(a, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=dev())


def f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def close(t, ref, rtol=RTOL, atol=0.0):
    a = t.detach().cpu().numpy().astype(np.float64)
    ref = np.asarray(ref, np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    scale = max(np.abs(ref).max(), 1e-30)
    err = np.abs(a - ref).max()
    assert err <= rtol * scale + atol, 'max err %.3e vs scale %.3e (rel %.3e)' % (err, scale, err / scale)


def _no_counted_launch(counts):
    return all(v == 0 for v in counts.values())


# ---------------------------------------------------------------------------------------------- 1. Dense
SMALL_HEAD = [
    # out, in, B: every value of each axis at least three times
    (1, 4, 1), (2, 1020, 8), (3, 4096, 9), (4, 4100, 17),
    (1, 4100, 9), (2, 4, 17), (3, 1020, 1), (4, 4096, 8),
    (1, 4096, 17), (2, 4100, 1), (3, 4, 8), (4, 1020, 9),
]


@pytest.mark.parametrize("n_out,n_in,B", SMALL_HEAD)
def test_dense_small_head(n_out, n_in, B):
    """dense_small_fwd / dense_small_bwd for every head width, plain, without dx, and as gn_dense_bwd_fused: x IS dropout(act(z)) of the
    producer layer and dx must be the oracle chain dense dx -> dropout backward -> activation backward."""
    from gennet_amd import ops
    rng = np.random.RandomState(1000 * n_out + n_in + B)
    x = f32(rng.randn(B, n_in)); w = f32(rng.randn(n_in, n_out) / np.sqrt(n_in)); b = f32(rng.randn(n_out) * 0.3)
    z_ref = K.dense_fwd(x, w, b)
    xd, wd, bd = g(x), g(w), g(b)
    for act, p in ACTS:
        y, counts = CF.launches(lambda: ops.dense_fwd(xd, wd, bd, act, p))
        assert _no_counted_launch(counts), counts
        close(y, K.act_fwd(z_ref, act, p))
    close(ops.dense_fwd(xd, wd, None), K.dense_fwd(x, w, None))
    dy = f32(rng.randn(B, n_out))
    dx_ref, dw_ref, db_ref = K.dense_bwd(x, w, dy)
    dyd = g(dy)
    dx, dw, db = ops.dense_bwd(xd, wd, dyd)
    close(dx, dx_ref); close(dw, dw_ref, 5e-5); close(db, db_ref, 5e-5)
    dx2, dw2, db2 = ops.dense_bwd(xd, wd, dyd, need_dx=False)
    assert dx2 is None and torch.equal(dw2, dw) and torch.equal(db2, db)
    # the fused form: x is the producer's output
    z = f32(rng.randn(B, n_in))
    for act, p, rate, with_mask in (('relu', 0.0, 0.0, False), ('relu', 0.0, 0.2, True), ('leaky', 0.2, 0.2, True), ('tanh', 0.0, 0.3, True), ('linear', 0.0, 0.5, True)):
        mask = (rng.rand(B, n_in) >= rate).astype(np.uint8) if with_mask else None
        y_act = K.act_fwd(z, act, p)
        xp = f32(K.dropout_fwd(y_act, mask, rate) if with_mask else y_act)
        d_out, dwp_ref, dbp_ref = K.dense_bwd(xp, w, dy)
        d_act = d_out * mask / (1.0 - rate) if with_mask else d_out
        dz_ref = K.act_bwd(d_act, y_act, act, p)
        xpd = g(xp); md = g(mask, torch.uint8) if with_mask else None
        dz, dwp, dbp = ops.dense_bwd(xpd, wd, dyd, prev=(xpd, act, p, md, rate))
        close(dz, dz_ref)
        if with_mask:
            assert (dz.cpu().numpy()[mask == 0] == 0).all()
            close(dz, R.act_dropout_bwd(d_out, xp, mask, act, p, rate))       # the same, through the layer output
        close(dwp, dwp_ref, 5e-5); close(dbp, dbp_ref, 5e-5)


ANY_GEMM = [(1, 1, 5), (15, 17, 33), (16, 16, 6), (17, 15, 16), (33, 50, 3), (4, 6, 1), (40, 913, 50)]


@pytest.mark.parametrize("B,n_in,n_out", ANY_GEMM)
def test_dense_any_shape_gemm(B, n_in, n_out):
    """dense_any_kernel as forward (bias, activation), data gradient and weight gradient; db through bias_grad (its small-C sum for out <= 4).
    Each output is one k-ordered fmaf chain whatever the launch: a row computed alone is bit-identical to the same row of the batch."""
    from gennet_amd import ops
    rng = np.random.RandomState(B * 100 + n_in + n_out)
    x = f32(rng.uniform(-1, 1, (B, n_in))); w = f32(rng.randn(n_in, n_out) * 0.3); b = f32(rng.randn(n_out))
    z_ref = K.dense_fwd(x, w, b)
    xd, wd, bd = g(x), g(w), g(b)
    ys = {}
    for act, p in ACTS:
        ys[act], counts = CF.launches(lambda: ops.dense_fwd(xd, wd, bd, act, p))
        assert _no_counted_launch(counts), counts
        close(ys[act], K.act_fwd(z_ref, act, p))
    close(ops.dense_fwd(xd, wd, None), K.dense_fwd(x, w, None))
    dy = f32(rng.randn(B, n_out))
    dx_ref, dw_ref, db_ref = K.dense_bwd(x, w, dy)
    dyd = g(dy)
    (dx, dw, db), counts = CF.launches(lambda: ops.dense_bwd(xd, wd, dyd))
    assert _no_counted_launch(counts), counts
    close(dx, dx_ref); close(dw, dw_ref, 5e-5); close(db, db_ref, 5e-5)
    dx2, dw2, db2 = ops.dense_bwd(xd, wd, dyd, need_dx=False)
    assert dx2 is None
    # two runs, and a row on its own
    dx3, dw3, db3 = ops.dense_bwd(xd, wd, dyd)
    assert torch.equal(ops.dense_fwd(xd, wd, bd, 'tanh', 0.0), ys['tanh'])
    assert torch.equal(dx3, dx) and torch.equal(dw3, dw) and torch.equal(db3, db) and torch.equal(dw2, dw) and torch.equal(db2, db)
    x0, dy0 = xd[:1].contiguous(), dyd[:1].contiguous()
    assert torch.equal(ops.dense_fwd(x0, wd, bd, 'tanh', 0.0), ys['tanh'][:1])
    assert torch.equal(ops.dense_fwd(x0, wd, bd), ys['linear'][:1])
    assert torch.equal(ops.dense_bwd(x0, wd, dy0)[0], dx[:1])


@pytest.mark.parametrize("B,n_in,n_out", [(1, 4, 8), (33, 8, 12), (17, 100, 36)])
def test_dense_matrix_core_route_at_its_smallest_widths(B, n_in, n_out):
    """Aligned widths beyond the heads go to the MFMA conv kernels as a 1-tap conv (launch counter 0: conv, 1: weight gradient); the data
    gradient is the conv with the widths swapped, so with in <= 4 it is a small-channel launch (counted apart: conv_family.SMALL_KINDS)."""
    from gennet_amd import ops
    rng = np.random.RandomState(B + n_in + n_out)
    x = f32(rng.uniform(-1, 1, (B, n_in))); w = f32(rng.randn(n_in, n_out) * 0.3); b = f32(rng.randn(n_out))
    z_ref = K.dense_fwd(x, w, b)
    xd, wd, bd = g(x), g(w), g(b)
    for act, p in ACTS:
        y, counts = CF.launches(lambda: ops.dense_fwd(xd, wd, bd, act, p))
        assert counts[0] == 1 and sum(counts.values()) == 1, counts
        close(y, K.act_fwd(z_ref, act, p))
    dy = f32(rng.randn(B, n_out))
    dx_ref, dw_ref, db_ref = K.dense_bwd(x, w, dy)
    dyd = g(dy)
    (dx, dw, db), counts = CF.launches(lambda: ops.dense_bwd(xd, wd, dyd))
    assert counts[1] == 1 and counts[0] == (0 if n_in <= 4 else 1) and sum(counts.values()) == counts[0] + 1, counts
    close(dx, dx_ref); close(dw, dw_ref, 5e-5); close(db, db_ref, 5e-5)
    dx2, dw2, db2 = ops.dense_bwd(xd, wd, dyd, need_dx=False)
    assert dx2 is None and torch.equal(dw2, dw) and torch.equal(db2, db)


# ---------------------------------------------------------------------------------------------- 2. column reductions, BatchNormalization
@pytest.mark.parametrize("rows", [2, 7, 257, 3001])
@pytest.mark.parametrize("C", [4, 12, 20, 100, 1028, 1280])
def test_column_sums_and_batchnorm_at_uneven_channel_counts(C, rows):
    """bias_grad, bn_stats and the chain of test_kernels_gpu.test_batchnorm_train_fwd_bwd (its tolerances), with and without a dropout mask, from
    the stored layer output and with the output recomputed; every reduction and dx bit-identical on a second run."""
    from gennet_amd import ops
    rng = np.random.RandomState(C * 10000 + rows)
    x = f32(rng.randn(rows, C) * 1.5 + 0.7); gamma = f32(rng.rand(C) + 0.5); beta = f32(rng.randn(C) * 0.1)
    dy = f32(rng.randn(rows, C))
    x2, dy2 = g(x), g(dy)
    db = ops.bias_grad(dy2)
    close(db, dy.sum(0), 1e-6)
    assert torch.equal(ops.bias_grad(dy2), db)
    sums = ops.bn_stats(x2)
    s_ref = np.concatenate([x.sum(0), (x * x).sum(0)])
    s_err = np.abs(sums.cpu().numpy() - s_ref).max()
    assert s_err <= 1e-9 * max(1.0, np.abs(s_ref).max()), 'fp64 sums off by %.3e' % s_err
    assert torch.equal(ops.bn_stats(x2), sums)
    close(sums[:C], x.sum(0), 1e-6, 1e-3)
    y_bn, cache, mean, var = K.bn_train_fwd(x, gamma, beta)
    y_act = np.tanh(y_bn)
    mm0, mv0 = f32(rng.randn(C) * 0.1), f32(rng.rand(C) + 0.5)
    mm_ref, mv_ref = K.bn_moving_update(mm0, mv0, mean, var, rows, 0.99)
    mm, mv = g(mm0), g(mv0)
    scale, shift, smean, sinv = ops.bn_finalize(sums, rows, g(gamma), g(beta), K.BN_EPS, 0.99, mm, mv)
    close(smean, mean, 1e-5, 1e-6); close(mm, mm_ref, 1e-5); close(mv, mv_ref, 1e-5)
    gd = g(gamma)
    for rate in (0.0, 0.2):
        mask = (rng.rand(rows, C) >= rate).astype(np.uint8) if rate else None
        mt = g(mask, torch.uint8) if rate else None
        y_ref = K.dropout_fwd(y_act, mask, rate) if rate else y_act
        y = ops.bn_apply(x2, scale, shift, mt, 'tanh', 0.0, rate)
        close(y, y_ref, 2e-5)
        d_act = dy * mask / (1 - rate) if rate else dy
        dx_ref, dg_ref, db_ref = K.bn_train_bwd(K.act_bwd(d_act, y_act, 'tanh'), cache, gamma)
        dsums = ops.bn_bwd_stats(dy2, y, x2, mt, smean, sinv, 'tanh', 0.0, rate)
        dgamma = torch.empty(C, device=dev()); dbeta = torch.empty(C, device=dev())
        dx = ops.bn_bwd_apply(dy2, y, x2, mt, gd, smean, sinv, dsums, rows, dsums, dgamma, dbeta, 'tanh', 0.0, rate)
        close(dgamma, dg_ref, 1e-4); close(dbeta, db_ref, 1e-4)
        close(dx, dx_ref, 1e-4)
        assert torch.equal(ops.bn_bwd_stats(dy2, y, x2, mt, smean, sinv, 'tanh', 0.0, rate), dsums)
        assert torch.equal(ops.bn_bwd_apply(dy2, y, x2, mt, gd, smean, sinv, dsums, rows, dsums, dgamma, dbeta, 'tanh', 0.0, rate), dx)
        # the activation output recomputed from the pre-BN tensor, the stored output not read
        dsums2 = ops.bn_bwd_stats(dy2, None, x2, mt, smean, sinv, 'tanh', 0.0, rate, scale, shift)
        close(dsums2, dsums.cpu().numpy(), 1e-6)
        dgamma2 = torch.empty(C, device=dev()); dbeta2 = torch.empty(C, device=dev())
        dx2 = ops.bn_bwd_apply(dy2, None, x2, mt, gd, smean, sinv, dsums2, rows, dsums2, dgamma2, dbeta2, 'tanh', 0.0, rate, scale, shift)
        close(dgamma2, dg_ref, 1e-4); close(dbeta2, db_ref, 1e-4)
        close(dx2, dx_ref, 1e-4)
        assert torch.equal(ops.bn_bwd_stats(dy2, None, x2, mt, smean, sinv, 'tanh', 0.0, rate, scale, shift), dsums2)
        assert torch.equal(ops.bn_bwd_apply(dy2, None, x2, mt, gd, smean, sinv, dsums2, rows, dsums2, dgamma2, dbeta2, 'tanh', 0.0, rate, scale, shift), dx2)


def _conv1_forward(x2, rows, gamma, beta):
    from gennet_amd import ops
    C = x2.shape[1]
    sums = ops.bn_stats(x2)
    mm, mv = g(np.zeros(C)), g(np.ones(C))
    return ops.bn_finalize(sums, rows, g(gamma), g(beta), K.BN_EPS, 0.99, mm, mv)


@pytest.mark.parametrize("B,L,k,padding", [(2, 33, 5, 'same'), (4, 21, 3, 'valid'), (3, 40, 3, 'same'), (2, 7, 5, 'valid')])
@pytest.mark.parametrize("C", [256, 768, 1280, 2048])
def test_conv1_gradient_on_the_fly_over_wave_uniform_windows(C, B, L, k, padding):
    """gn_bn_bwd_stats_conv1 / gn_bn_bwd_apply_conv1 with C / 4 a multiple of 64 (the readlane window path), every block shape of it,
    against the oracle chain on the materialised gradient (the chain and tolerances of the test of that name in test_kernels_gpu.py)."""
    from gennet_amd import ops
    rng = np.random.RandomState(L + C + k)
    x = f32(rng.randn(B, L, C) * 1.5 + 0.3); gamma = f32(rng.rand(C) + 0.5); beta = f32(rng.randn(C) * 0.1)
    rate = 0.2
    mask = (rng.rand(B, L, C) >= rate).astype(np.uint8)
    w = f32(rng.randn(k, C, 1) * 0.2)
    y_bn, cache, mean, var = K.bn_train_fwd(x, gamma, beta)
    y_act = np.tanh(y_bn)
    y = K.dropout_fwd(y_act, mask, rate)
    z = K.conv1d_fwd(y, w, np.zeros(1), 1, padding)
    gz = f32(rng.randn(*z.shape))
    dz_ref, _, _ = K.conv1d_bwd(y, w, gz, 1, padding)
    dx_ref, dg_ref, db_ref = K.bn_train_bwd(K.act_bwd(dz_ref * mask / (1 - rate), y_act, 'tanh'), cache, gamma)

    rows = B * L
    x2 = g(x).reshape(rows, C)
    scale, shift, smean, sinv = _conv1_forward(x2, rows, gamma, beta)
    mt = g(mask.reshape(rows, C), torch.uint8)
    Lout, pl = ops.conv_geometry(L, k, 1, padding)
    cg = ops.ConvGrad1(g(gz), g(w), L, pl)
    assert cg.shape == (B, L, C) and cg.Lout == Lout
    dsums = ops.bn_bwd_stats_conv1(cg, x2, mt, smean, sinv, 'tanh', 0.0, rate, scale, shift)
    dgamma = torch.empty(C, device=dev()); dbeta = torch.empty(C, device=dev())
    dx = ops.bn_bwd_apply_conv1(cg, x2, mt, g(gamma), smean, sinv, dsums, rows, dsums, dgamma, dbeta, 'tanh', 0.0, rate, scale, shift)
    close(dgamma, dg_ref, 1e-4); close(dbeta, db_ref, 1e-4)
    close(dx, dx_ref.reshape(rows, C), 1e-4)
    dz = ops.conv1d_dgrad(g(gz), ops.conv1d_transpose_w(g(w)), L, 1, pl).reshape(rows, C)
    close(dz, dz_ref.reshape(rows, C), 5e-5)
    dsums_m = ops.bn_bwd_stats(dz, None, x2, mt, smean, sinv, 'tanh', 0.0, rate, scale, shift)
    close(dsums, dsums_m.cpu().numpy(), 1e-5, 1e-6)
    assert torch.equal(ops.bn_bwd_stats_conv1(cg, x2, mt, smean, sinv, 'tanh', 0.0, rate, scale, shift), dsums)


def test_conv1_gradient_on_the_fly_window_slides_and_segments_change_inside_chunks():
    """C = 256, B = 96, L = 1024, k = 5, 'same': 98304 rows in 1024 chunks of 96.  A wave of the statistics pass walks 24 rows of its chunk, 4
    apart: more than its 64-wide window on g holds, so the window is reloaded inside the chunk; and 1024 is no multiple of 96, so two chunks
    in three cross a segment end (the other reload condition, and lazy_dy_step's carry).  BatchNormalization backward and a 1-filter conv
    gradient are independent per channel, so the oracle runs on 16 channels (the first and the last quad and 8 between); the sums of ALL
    channels are compared with bn_bwd_stats fed the materialised gradient.  The apply kernel walks at most ~rows / 8192 rows per chunk: its
    window would only slide from ~2 M rows on, which no unit test can hold -- that path is not reached here and not emulated."""
    from gennet_amd import ops
    B, L, C, k, padding, rate = 96, 1024, 256, 5, 'same', 0.2
    rng = np.random.default_rng(96)
    x32 = rng.standard_normal((B, L, C), dtype=np.float32) * np.float32(1.5) + np.float32(0.3)
    mask = (rng.random((B, L, C), dtype=np.float32) >= rate).astype(np.uint8)
    gamma = f32(rng.random(C) + 0.5); beta = f32(rng.standard_normal(C) * 0.1)
    w = f32(rng.standard_normal((k, C, 1)) * 0.2)
    gz = f32(rng.standard_normal((B, L, 1)))
    cs = np.array([0, 1, 2, 3, 17, 64, 65, 100, 127, 128, 191, 200, 252, 253, 254, 255])
    xs = x32[:, :, cs].astype(np.float64); ms = mask[:, :, cs]
    y_bn, cache, mean, var = K.bn_train_fwd(xs, gamma[cs], beta[cs])
    y_act = np.tanh(y_bn)
    dz_ref, _, _ = K.conv1d_bwd(K.dropout_fwd(y_act, ms, rate), w[:, cs], gz, 1, padding)       # the data gradient needs gz and w alone
    dx_ref, dg_ref, db_ref = K.bn_train_bwd(K.act_bwd(dz_ref * ms / (1 - rate), y_act, 'tanh'), cache, gamma[cs])

    rows = B * L
    x2 = g(x32).reshape(rows, C)
    scale, shift, smean, sinv = _conv1_forward(x2, rows, gamma, beta)
    mt = g(mask.reshape(rows, C), torch.uint8)
    Lout, pl = ops.conv_geometry(L, k, 1, padding)
    cg = ops.ConvGrad1(g(gz), g(w), L, pl)
    dsums = ops.bn_bwd_stats_conv1(cg, x2, mt, smean, sinv, 'tanh', 0.0, rate, scale, shift)
    dgamma = torch.empty(C, device=dev()); dbeta = torch.empty(C, device=dev())
    dx = ops.bn_bwd_apply_conv1(cg, x2, mt, g(gamma), smean, sinv, dsums, rows, dsums, dgamma, dbeta, 'tanh', 0.0, rate, scale, shift)
    csd = torch.tensor(cs, device=dev())
    close(dgamma[csd], dg_ref, 1e-4); close(dbeta[csd], db_ref, 1e-4)
    close(dx[:, csd], dx_ref.reshape(rows, len(cs)), 1e-4)
    dz = ops.conv1d_dgrad(g(gz), ops.conv1d_transpose_w(g(w)), L, 1, pl).reshape(rows, C)
    close(dz[:, csd], dz_ref.reshape(rows, len(cs)), 5e-5)
    dsums_m = ops.bn_bwd_stats(dz, None, x2, mt, smean, sinv, 'tanh', 0.0, rate, scale, shift)
    close(dsums, dsums_m.cpu().numpy(), 1e-5, 1e-6)


# ---------------------------------------------------------------------------------------------- 3. streaming passes
STREAM_N = [1, 3, 4, 5, 1003, (1 << 21) + 5]


def _stream_inputs(n):
    """x on a 1/256 grid: no activation decision (0, and relu_max's cap 1) hangs on a rounding of the dropout scale.  Element 0 is an
    unsaturated point (x 0.5, dy 4): the 1e-6 of the activation passes is relative to the largest oracle magnitude, and fp32 evaluates
    dy (1 - y^2) to ~1e-7 of dy, not of the result -- with 1 to 5 elements, all of them on a saturated tanh, that largest magnitude would
    itself be a cancellation no fp32 kernel can meet.  The per-element bound of elem_close keeps every other element as sensitive as if
    it stood alone."""
    rng = np.random.RandomState(n % 100003)
    x = np.round(rng.randn(n) * 2 * 256) / 256
    dy = f32(rng.randn(n))
    mask = (rng.rand(n) >= 0.2).astype(np.uint8)
    x[0], dy[0] = 0.5, 4.0
    return x, dy, mask


def elem_close(t, ref, dy, keep_scale=1.0):
    """Each element of an activation gradient within 1e-6 of ITS OWN |dy| keep_scale (the derivative factors are at most 1), besides
    close()'s 1e-6 of the largest magnitude: a small-|dy| or saturated element is not hidden behind a large one."""
    err = np.abs(t.detach().cpu().numpy().astype(np.float64) - ref)
    bound = 1e-6 * np.abs(dy) * keep_scale
    i = int(np.argmax(err - bound))
    assert err[i] <= bound[i], 'element %d: err %.3e, bound %.3e (dy %.3e)' % (i, err[i], bound[i], dy[i])
    close(t, ref, 1e-6)


@pytest.mark.parametrize("act,p", ACTS)
@pytest.mark.parametrize("n", STREAM_N)
def test_activation_passes_across_the_grid_stride_trip_and_the_tail(n, act, p):
    """act_fwd, act_bwd and act_dropout_bwd (in place and out of place, rates 0 and 0.2, under a mask with zeros and under its complement,
    so that every element takes the kept and the dropped branch) at 1e-6, and each gradient element at 1e-6 of its own dy."""
    from gennet_amd import ops
    x, dy, mask = _stream_inputs(n)
    xd, dyd = g(x), g(dy)
    y = ops.act_fwd(xd, act, p)
    close(y, K.act_fwd(x, act, p), 1e-6)
    y64 = y.cpu().numpy().astype(np.float64)
    elem_close(ops.act_bwd(dyd, y, act, p), K.act_bwd(dy, y64, act, p), dy)
    dyc = dyd.clone()
    assert ops.act_bwd(dyc, y, act, p, inplace=True) is dyc
    elem_close(dyc, K.act_bwd(dy, y64, act, p), dy)
    for m in (mask, 1 - mask):
        md = g(m, torch.uint8)
        for rate in (0.0, 0.2):
            yl = ops.dropout_apply(y, md, rate)                                   # the layer output
            ref = R.act_dropout_bwd(dy, yl.cpu().numpy().astype(np.float64), m, act, p, rate)
            dx = ops.act_dropout_bwd(dyd, yl, md, act, p, rate)
            assert torch.equal(dyd, g(dy))                                        # out of place: dy untouched
            elem_close(dx, ref, dy, 1.0 / (1.0 - rate))
            assert (dx.cpu().numpy()[m == 0] == 0).all()
            dyc = dyd.clone()
            assert ops.act_dropout_bwd(dyc, yl, md, act, p, rate, inplace=True) is dyc
            assert torch.equal(dyc, dx)


@pytest.mark.parametrize("n", STREAM_N)
def test_dropout_apply_and_axpy(n):
    from gennet_amd import ops
    x, y0, mask = _stream_inputs(n)
    xd, md = g(x), g(mask, torch.uint8)
    for rate in (0.0, 0.2):
        close(ops.dropout_apply(xd, md, rate), K.dropout_fwd(x, mask, rate), 1e-6)
    for a in (1.0, -0.5):
        yd = g(y0)
        assert ops.axpy(yd, xd, a) is yd
        close(yd, y0 + a * x, 1e-7)
        assert torch.equal(xd, g(x))


@pytest.mark.parametrize("B,n", [(1, 1), (4, 33), (3, 200003)])
def test_subtract_stack_and_affine_stack(B, n):
    from gennet_amd import ops
    rng = np.random.RandomState(B + n)
    x = f32(rng.randn(B, n, 1)); ev = f32(rng.randn(n, 1)); dimg = f32(rng.randn(B, n, 2, 1))
    xd, dd = g(x), g(dimg)
    close(ops.subtract_stack_fwd(xd, g(ev)), K.mylayer_fwd(x, ev), 1e-7)
    close(ops.subtract_stack_bwd(dd), K.mylayer_bwd(dimg), 1e-6)
    a0, a1 = 0.75, -1.5
    b0, b1 = f32(rng.randn(n)), f32(rng.randn(n))
    for u0, u1 in ((b0, b1), (b0, None), (None, b1), (None, None)):
        img = ops.affine_stack_fwd(xd, a0, None if u0 is None else g(u0), a1, None if u1 is None else g(u1))
        assert tuple(img.shape) == (B, n, 2, 1)
        close(img, R.affine_stack_fwd(x, a0, u0, a1, u1), 1e-6)
    close(ops.affine_stack_bwd(dd, a0, a1), R.affine_stack_bwd(dimg, a0, a1), 1e-6)
    close(ops.affine_stack_fwd(xd, 1.0, None, -1.0, g(ev.reshape(-1))), K.mylayer_fwd(x, ev), 1e-7)       # MyLayer as the engine lowers it


@pytest.mark.parametrize("B,n", [(1, 5), (3, 33), (2, 300001)])
def test_assemble_d_batch_exact(B, n):
    """One copy or one subtraction per element: bit-identical to the same in fp32 numpy."""
    from gennet_amd import ops
    rng = np.random.RandomState(B * n % 65521)
    real, noise, fake = (rng.randn(B, n).astype(np.float32) for _ in range(3))
    event = rng.randn(n).astype(np.float32)
    want = R.assemble_d_batch(real, noise, fake, event)
    assert want.dtype == np.float32
    sX = ops.assemble_d_batch(g(real), g(noise), g(fake), g(event))
    assert tuple(sX.shape) == (2 * B, n, 2, 1) and np.array_equal(sX.cpu().numpy(), want)


@pytest.mark.parametrize("rows,width,src_rows", [(700000, 1, 1000), (5, 7, 3)])
def test_gather_rows_with_repeated_indices(rows, width, src_rows):
    from gennet_amd import ops
    rng = np.random.RandomState(rows)
    src = rng.randn(src_rows, width).astype(np.float32)
    idx = rng.randint(0, src_rows, rows)
    idx[:2] = src_rows - 1                                      # the last row, twice
    out = ops.gather_rows(g(src), g(idx, torch.int64))
    assert np.array_equal(out.cpu().numpy(), src[idx])


# ---------------------------------------------------------------------------------------------- 4. losses
P_EDGE = np.array([0.0, 1.0, 1e-7, 1 - 1e-7, 0.5], np.float32)
Y_EDGE = np.array([1.0, 0.0, 0.0, 1.0, 1.0])        # p = 0 and p = 1 WRONG (the largest terms; outside the clip: zero gradient), the clip bounds themselves right


def loss_close(got, ref, n):
    """The terms are non-negative; each thread adds ceil(n / 256) of them in fp32 before an 8-level tree: (ceil(n / 256) + 16) half-ulps,
    relative to the fp64 loss."""
    bound = (-(-n // 256) + 16) * 2.0 ** -24
    err = abs(got - ref) / ref
    assert err <= bound, 'loss %.9g against %.9g: relative error %.3e, bound %.3e' % (got, ref, err, bound)


@pytest.mark.parametrize("n,gfac", [(1, 1), (255, 1), (256, 1), (257, 1), (257, 2), (100000, 1), (100000, 2)])
def test_losses_across_the_block_and_in_the_flattened_form(n, gfac):
    """gn_bce_loss / gn_mse_loss over n elements with the mean taken over Bglobal = gfac * n (the data-parallel form): loss within
    (ceil(n / 256) + 16) 2^-24 of the fp64 value, gradient at 2e-5 (BCE) / 1e-6 (MSE), hit count exact."""
    from gennet_amd import ops
    rng = np.random.RandomState(n)
    p = rng.rand(n, 1).astype(np.float32); y = (rng.rand(n, 1) > 0.5).astype(np.float64)
    m = min(n, 5)
    p[:m, 0] = P_EDGE[:m]; y[:m, 0] = Y_EDGE[:m]
    p = p.astype(np.float64)
    l_ref, dp_ref = K.bce_loss(p, y)
    dp, out = ops.loss('binary_crossentropy', g(p), g(y), Bglobal=gfac * n)
    o = out.cpu().numpy().astype(np.float64)
    loss_close(o[0], l_ref / gfac, n)
    assert o[1] == np.sum(np.round(p) == y)
    close(dp, dp_ref / gfac, 2e-5)
    assert (dp.cpu().numpy()[:min(n, 2)] == 0).all()                      # p = 0, p = 1: outside the clip

    pm = f32(rng.randn(n, 1) * 3 + 25); ym = f32(rng.uniform(20, 35, (n, 1)))
    ym[::7] = np.round(pm[::7])                                              # some hits
    l_ref, dp_ref = K.mse_loss(pm, ym)
    dp, out = ops.loss('mean_squared_error', g(pm), g(ym), Bglobal=gfac * n)
    o = out.cpu().numpy().astype(np.float64)
    loss_close(o[0], l_ref / gfac, n)
    assert o[1] == np.sum(np.round(pm) == ym)
    close(dp, dp_ref / gfac, 1e-6)


# ---------------------------------------------------------------------------------------------- 5. device-scalar variants
def _dev_scalar(value, dtype):
    from gennet_amd import ops
    t = torch.tensor([value], dtype=dtype, device=dev())
    return t, ops.DevScalar(t.data_ptr())


def test_adam_step_from_a_device_scalar_is_the_by_value_step():
    from gennet_amd import ops
    rng = np.random.RandomState(21)
    n = (1 << 19) + 3                                               # a second grid-stride trip
    p0, m0, v0 = f32(rng.randn(n)), f32(rng.randn(n) * 0.01), f32(rng.rand(n) * 1e-4)
    pa, ma, va, pb, mb, vb = g(p0), g(m0), g(v0), g(p0), g(m0), g(v0)
    for t in (1, 2):
        gr = g(rng.randn(n) * 0.01)
        lr_t = float(np.float32(9e-5 * np.sqrt(1 - 0.999 ** t) / (1 - 0.5 ** t)))
        keep, lr_dev = _dev_scalar(lr_t, torch.float32)
        ops.adam_step(pa, gr, ma, va, lr_t, 0.5, 0.999, 1e-7)
        ops.adam_step(pb, gr, mb, vb, lr_dev, 0.5, 0.999, 1e-7)
        torch.cuda.synchronize()
        assert torch.equal(pa, pb) and torch.equal(ma, mb) and torch.equal(va, vb)
    assert not torch.equal(pa, g(p0))


@pytest.mark.parametrize("n", [5, (1 << 21) + 5])
def test_fill_normal_from_a_device_scalar_is_the_by_value_fill(n):
    from gennet_amd import ops
    sd = float(np.float32(2.7))
    keep, sd_dev = _dev_scalar(sd, torch.float32)
    a = ops.fill_normal((n,), 0.25, sd, 42, 7, dev())
    b = ops.fill_normal((n,), 0.25, sd_dev, 42, 7, dev())
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    assert n < 100 or abs(a.std().item() - sd) < 0.02


@pytest.mark.parametrize("C", [12, 100, 1280])
def test_bn_finalize_zero_debias_from_a_device_step_is_the_by_value_call(C):
    from gennet_amd import ops
    rng = np.random.RandomState(C)
    rows = 64
    x = g(rng.randn(rows, C) * 3.0 + 2.0)
    gamma, beta = g(rng.rand(C) + 0.5), g(rng.randn(C) * 0.1)
    sums = ops.bn_stats(x)
    state = [f32(rng.randn(C) * 0.1), f32(rng.rand(C) + 0.5), f32(rng.randn(C) * 0.01), f32(rng.rand(C) * 0.01)]
    for step in (1, 3, 500):
        a = [g(s) for s in state]; b = [g(s) for s in state]
        keep, step_dev = _dev_scalar(step, torch.int32)
        out_a = ops.bn_finalize(sums, rows, gamma, beta, K.BN_EPS, 0.99, a[0], a[1], (a[2], a[3], step))
        out_b = ops.bn_finalize(sums, rows, gamma, beta, K.BN_EPS, 0.99, b[0], b[1], (b[2], b[3], step_dev))
        torch.cuda.synchronize()
        for ta, tb in zip(list(out_a) + a, list(out_b) + b):
            assert torch.equal(ta, tb)
        assert not torch.equal(a[0], g(state[0]))
