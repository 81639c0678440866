"""GPU parity of the transform-domain fp32 convolution (csrc/conv_wino.hip: Cook-Toom F(2,5) for the unit-stride 5-tap layers of
generator_model bbhMahoGANy.py:259-283 and of signal_pe_model's q branch :382-386) against the fp64 oracle and against the direct kernels.

Bounds: the kernels' own 2e-5 of the largest oracle entry (tests/test_kernels_gpu.py RTOL), AND the gate of VERDICT r4 item 2 -- the error
against fp64 may not exceed 4 x the direct k-ordered fp32 chain's on the same operands (measured 1.2-1.8 x; profiles/r05_winograd_gate1.txt).
Everything goes through the C ABI (gn_conv1d_fwd*, gn_conv1d_dgrad*, gn_set_conv_math); the engine's default conv math is 'wino'.
"""
import numpy as np
import pytest
import torch

from oracle import keras_ref as K

pytestmark = pytest.mark.gpu

RTOL = 2e-5


def g(a, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=torch.device('cuda:0'))


def f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def errs(t, ref):
    a = t.detach().cpu().numpy().astype(np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    d = np.abs(a - ref)
    return d.max() / max(np.abs(ref).max(), 1e-30), np.sqrt(np.mean(d ** 2)) / max(np.sqrt(np.mean(ref ** 2)), 1e-30)


def launches(kind):
    from gennet_amd import ops
    return ops.prof_collect(kind)['launches']


WINO_CASES = [
    # B, L, Cin, Cout, padding, act
    (2, 64, 64, 64, 'same', 'linear'),          # one block of tiles
    (3, 130, 128, 256, 'same', 'tanh'),         # ragged row tiles (65 output pairs), four column tiles
    (2, 257, 64, 128, 'valid', 'relu'),         # odd output length: the last output pair has one row
    (5, 37, 32, 64, 'same', 'leaky'),           # the smallest channel count the dispatcher sends here, odd lengths
    (1, 1, 64, 64, 'same', 'linear'),           # a single output row
    (2, 5, 40, 192, 'valid', 'linear'),         # one output row per element, Cin = 5 chunks, three column tiles
    (1, 2048, 512, 1024, 'same', 'linear'),     # the generator's largest layer (bbhMahoGANy.py:279), one element
    (2, 2044, 128, 256, 'valid', 'relu'),       # the q branch's Conv1D(256, 5) (:384)
    (1, 300, 1024, 64, 'same', 'linear'),       # 128 channel chunks
]


@pytest.mark.parametrize("B,L,Cin,Cout,padding,act", WINO_CASES)
def test_forward_against_oracle_and_direct_kernel(B, L, Cin, Cout, padding, act):
    from gennet_amd import ops
    rng = np.random.RandomState(B * 1000 + L)
    x = f32(np.tanh(rng.randn(B, L, Cin)) * (rng.rand(B, L, Cin) > 0.2) / 0.8)          # what the generator's layers see: tanh outputs through Dropout(0.2)
    lim = np.sqrt(6.0 / (5 * (Cin + Cout)))
    w = f32(rng.uniform(-lim, lim, (5, Cin, Cout))); b = f32(rng.randn(Cout) * 0.1)
    Lout, pl = ops.conv_geometry(L, 5, 1, padding)
    ref = K.act_fwd(K.conv1d_fwd(x, w, b, 1, padding), act, 0.2)
    ops.prof_enable(True); ops.prof_reset()
    try:
        with ops.conv_math('wino'):
            yw = ops.conv1d_fwd(g(x), g(w), g(b), 1, pl, Lout, act, 0.2)
            assert launches(5) == 1 and launches(0) == 0                              # the transform-domain kernel really took it
            yw_direct_entry = ops.conv1d_fwd_wino(g(x), g(w), g(b), pl, Lout, act, 0.2)
        with ops.conv_math('fp32'):
            yd = ops.conv1d_fwd(g(x), g(w), g(b), 1, pl, Lout, act, 0.2)
            assert launches(0) == 1
    finally:
        ops.prof_enable(False)
    assert torch.equal(yw, yw_direct_entry)
    mw, rw = errs(yw, ref); md, rd = errs(yd, ref)
    assert mw <= RTOL, (mw, md)
    if Lout >= 16:                                                                    # (a handful of outputs is no sample of an rms)
        assert rw <= 4.0 * rd + 1e-8, (rw, rd)                                        # the gate: not more than 4 x the direct chain's error


def test_every_baseline_layer_shape_meets_the_gate():
    """The five layers the default dispatch sends to the kernel at BASELINE size (n_pix 2048), two elements each; error ratio to the direct kernel recorded."""
    from gennet_amd import ops
    rng = np.random.RandomState(3)
    for name, L, Cin, Cout, padding in (('G 128->256', 2048, 128, 256, 'same'), ('G 256->512', 2048, 256, 512, 'same'), ('G 512->1024', 2048, 512, 1024, 'same'),
                                        ('PE q 64->128', 2048, 64, 128, 'valid'), ('PE q 128->256', 2044, 128, 256, 'valid')):
        x = f32(rng.randn(2, L, Cin)); lim = np.sqrt(6.0 / (5 * (Cin + Cout)))
        w = f32(rng.uniform(-lim, lim, (5, Cin, Cout)))
        Lout, pl = ops.conv_geometry(L, 5, 1, padding)
        ref = K.conv1d_fwd(x, w, None, 1, padding)
        with ops.conv_math('wino'):
            yw = ops.conv1d_fwd(g(x), g(w), None, 1, pl, Lout)
        with ops.conv_math('fp32'):
            yd = ops.conv1d_fwd(g(x), g(w), None, 1, pl, Lout)
        (mw, rw), (md, rd) = errs(yw, ref), errs(yd, ref)
        print('%-14s transform-domain max %.2e rms %.2e | direct max %.2e rms %.2e | rms ratio %.2f' % (name, mw, rw, md, rd, rw / rd))
        assert mw <= RTOL and rw <= 4.0 * rd


@pytest.mark.parametrize("B,L,Cin,Cout,padding", [(3, 133, 64, 128, 'valid'), (2, 64, 128, 64, 'same'), (2, 301, 256, 128, 'same'), (1, 2040, 256, 128, 'valid')])
def test_data_gradient_plain_and_fused(B, L, Cin, Cout, padding):
    """dx of a unit-stride 5-tap layer = a 5-tap correlation of dy with the flipped, transposed kernel: the same kernel, taps in descending order; with the
    producer's activation / dropout backward in the epilogue (gn_conv1d_dgrad_fused) as the engine launches it."""
    from gennet_amd import ops
    rng = np.random.RandomState(L)
    x = f32(rng.randn(B, L, Cin)); w = f32(rng.randn(5, Cin, Cout) * 0.05)
    Lout, pl = ops.conv_geometry(L, 5, 1, padding)
    dy = f32(rng.randn(B, Lout, Cout))
    dx_ref, _, _ = K.conv1d_bwd(x, w, dy, 1, padding)
    wt = ops.conv1d_transpose_w(g(w))
    ops.prof_enable(True); ops.prof_reset()
    try:
        with ops.conv_math('wino'):
            dxw = ops.conv1d_dgrad(g(dy), wt, L, 1, pl)
            assert launches(5) == 1 and launches(0) == 0
        with ops.conv_math('fp32'):
            dxd = ops.conv1d_dgrad(g(dy), wt, L, 1, pl)
    finally:
        ops.prof_enable(False)
    (mw, rw), (md, rd) = errs(dxw, dx_ref), errs(dxd, dx_ref)
    assert mw <= RTOL and rw <= 4.0 * rd + 1e-8, (mw, rw, md, rd)
    # fused: through relu (the q branch) and through LeakyReLU + Dropout(0.4) -- the producer's output y_prev and keep-mask
    y_prev = f32(np.maximum(rng.randn(B, L, Cin), 0.0))
    ref_relu = dx_ref * (y_prev > 0)
    keep = (rng.rand(B, L, Cin) >= 0.4)
    pre = f32(rng.randn(B, L, Cin))
    y_leaky = f32(np.where(pre > 0, pre, np.float32(0.2) * pre) * keep / np.float32(0.6))
    ref_leaky = dx_ref * np.where(pre > 0, 1.0, float(np.float32(0.2))) * keep / float(np.float32(0.6))
    with ops.conv_math('wino'):
        dx1 = ops.conv1d_dgrad(g(dy), wt, L, 1, pl, prev=(g(y_prev), 'relu', 0.0, None, 0.0))
        dx2 = ops.conv1d_dgrad(g(dy), wt, L, 1, pl, prev=(g(y_leaky), 'leaky', 0.2, g(keep, torch.uint8), 0.4))
    assert errs(dx1, ref_relu)[0] <= RTOL and errs(dx2, ref_leaky)[0] <= 2 * RTOL


def test_fused_dropout_epilogue_and_batchnorm_statistics():
    from gennet_amd import ops
    rng = np.random.RandomState(9)
    B, L, Cin, Cout = 3, 150, 64, 128
    x = f32(rng.randn(B, L, Cin)); w = f32(rng.randn(5, Cin, Cout) * 0.05); b = f32(rng.randn(Cout))
    Lout, pl = ops.conv_geometry(L, 5, 1, 'same')
    pre = K.conv1d_fwd(x, w, b, 1, 'same')
    keep = rng.rand(B, Lout, Cout) >= 0.4
    ref = np.where(pre > 0, pre, float(np.float32(0.2)) * pre) * keep / float(np.float32(0.6))
    ops.prof_enable(True); ops.prof_reset()
    try:
        with ops.conv_math('wino'):
            y = ops.conv1d_fwd_dropout(g(x), g(w), g(b), g(keep, torch.uint8), 1, pl, Lout, 'leaky', 0.2, 0.4)
            ys, sums = ops.conv1d_fwd_stats(g(x), g(w), g(b), 1, pl, Lout)
            assert launches(5) == 2 and launches(0) == 0
        with ops.conv_math('fp32'):
            _, sums_d = ops.conv1d_fwd_stats(g(x), g(w), g(b), 1, pl, Lout)
    finally:
        ops.prof_enable(False)
    assert errs(y, ref)[0] <= 2 * RTOL
    assert errs(ys, pre)[0] <= RTOL
    # the statistics are fp64 sums of the fp32 outputs the kernel wrote: exact up to fp64 summation order
    yh = ys.cpu().numpy().astype(np.float64).reshape(-1, Cout)
    s = sums.cpu().numpy()
    assert np.allclose(s[:Cout], yh.sum(0), rtol=1e-12, atol=1e-9) and np.allclose(s[Cout:], (yh * yh).sum(0), rtol=1e-12)
    assert np.allclose(s, sums_d.cpu().numpy(), rtol=1e-5, atol=1e-4)
    # odd length: the statistics skip the row past the end of the last output pair
    x2 = f32(rng.randn(2, 77, Cin))
    Lo2, pl2 = ops.conv_geometry(77, 5, 1, 'same')
    with ops.conv_math('wino'):
        y2, s2 = ops.conv1d_fwd_stats(g(x2), g(w), g(b), 1, pl2, Lo2)
    yh2 = y2.cpu().numpy().astype(np.float64).reshape(-1, Cout)
    assert np.allclose(s2.cpu().numpy()[:Cout], yh2.sum(0), rtol=1e-12, atol=1e-9)


def test_a_batch_and_its_chunks_agree_bit_for_bit_and_runs_repeat():
    """The dispatcher chooses by the layer's shape alone: any batch size takes the same kernel with the same per-output arithmetic."""
    from gennet_amd import ops
    torch.manual_seed(0)
    dev = torch.device('cuda:0')
    with ops.conv_math('wino'):
        for (B, L, Cin, Cout, pl, Lout) in [(8, 64, 64, 128, 0, 60), (6, 2048, 128, 256, 2, 2048), (64, 300, 256, 128, 2, 300)]:
            x = torch.randn(B, L, Cin, device=dev); w = torch.randn(5, Cin, Cout, device=dev) * 0.05; b = torch.randn(Cout, device=dev)
            y = ops.conv1d_fwd(x, w, b, 1, pl, Lout, 'relu')
            h = B // 2
            y2 = torch.cat([ops.conv1d_fwd(x[:h].contiguous(), w, b, 1, pl, Lout, 'relu'), ops.conv1d_fwd(x[h:].contiguous(), w, b, 1, pl, Lout, 'relu')])
            assert torch.equal(y, y2) and torch.equal(y, ops.conv1d_fwd(x, w, b, 1, pl, Lout, 'relu'))


def test_dispatch_leaves_everything_else_on_the_direct_kernels():
    """2-4-tap, narrow or ragged-channel launches never reach the transform-domain kernels; GENNET_CONV_MATH=fp32 / ops.set_conv_math('fp32') takes it out."""
    from gennet_amd import ops
    dev = torch.device('cuda:0')
    ops.prof_enable(True)
    try:
        with ops.conv_math('wino'):
            for (Cin, Cout, k, s) in [(16, 128, 5, 2), (64, 128, 3, 1), (16, 128, 5, 1), (64, 96, 5, 1), (36, 64, 5, 1)]:
                ops.prof_reset()
                L = 80
                Lout, pl = ops.conv_geometry(L, k, s, 'same')
                ops.conv1d_fwd(torch.randn(2, L, Cin, device=dev), torch.randn(k, Cin, Cout, device=dev), None, s, pl, Lout)
                assert launches(5) == 0 and launches(7) == 0 and launches(0) == 1, (Cin, Cout, k, s)
        with ops.conv_math('fp32'):
            ops.prof_reset()
            ops.conv1d_fwd(torch.randn(2, 80, 64, device=dev), torch.randn(5, 64, 128, device=dev), None, 1, 2, 80)
            assert launches(5) == 0 and launches(0) == 1
    finally:
        ops.prof_enable(False)


@pytest.mark.parametrize("Cin,Cout,stride", [(1024, 2752, 1), (1024, 2368, 2)])
def test_a_transformed_kernel_above_64_mib_keeps_the_whole_layer_on_the_direct_kernels(Cin, Cout, stride):
    """The transform-domain families take a layer only if its transformed kernel (6 x Cin x Cout floats, 7 at stride 2) fits in 64 MiB, the same
    rule for forward, data gradient and weight gradient (csrc/capi.hip select_conv / select_dgrad / select_wgrad).  Just above it all three run on
    the direct kernels and equal the 'fp32' math bit for bit; 64 output channels fewer, the forward takes the transform domain."""
    from gennet_amd import ops
    pts = 6 if stride == 1 else 7
    assert pts * Cin * (Cout - 64) * 4 <= ops.WINO_WS_BYTES < pts * Cin * Cout * 4
    dev = torch.device('cuda:0')
    B, L = 2, 64
    Lout, pl = ops.conv_geometry(L, 5, stride, 'same')
    x = ops.fill_normal((B, L, Cin), 0.0, 1.0, 31, 0, dev)
    w = ops.fill_normal((5, Cin, Cout), 0.0, 0.02, 32, 0, dev)
    dy = ops.fill_normal((B, Lout, Cout), 0.0, 1.0, 33, 0, dev)

    def run():
        ops.prof_reset()
        out = [ops.conv1d_fwd(x, w, None, stride, pl, Lout), ops.conv1d_dgrad(dy, ops.conv1d_transpose_w(w), L, stride, pl)]
        out += list(ops.conv1d_wgrad(x, dy, 5, stride, pl))
        return [t.cpu().numpy() for t in out], [launches(k) for k in range(9)]

    ops.prof_enable(True)
    try:
        with ops.conv_math('wino'):
            got, n = run()
            ops.prof_reset()
            ops.conv1d_fwd(x, w[:, :, :Cout - 64].contiguous(), None, stride, pl, Lout)
            n_fit = launches(5 if stride == 1 else 7)
        with ops.conv_math('fp32'):
            ref, n_ref = run()
    finally:
        ops.prof_enable(False)
    assert n[5:] == [0, 0, 0, 0] and n == n_ref and n[0] >= 2 and n[1] == 1, (n, n_ref)
    assert n_fit == 1
    for a, b in zip(got, ref):
        assert np.array_equal(a, b)


def test_a_weight_gradient_workspace_too_small_for_its_kernel_is_an_error():
    """The transform-domain weight gradient used to fall back to the direct kernel when the caller's workspace could not hold its slabs; the kernel
    is now chosen by the layer's shape alone, and a workspace that holds only what the direct kernel would need is GN_EWORKSPACE (C ABI)."""
    from gennet_amd import _lib, ops
    dev = torch.device('cuda:0')
    B, L, Cin, Cout = 2, 256, 64, 128
    x = ops.fill_normal((B, L, Cin), 0.0, 1.0, 41, 0, dev)
    dy = ops.fill_normal((B, L, Cout), 0.0, 1.0, 42, 0, dev)
    dw = torch.empty((5, Cin, Cout), dtype=torch.float32, device=dev)
    db = torch.empty((Cout,), dtype=torch.float32, device=dev)
    args = (B, L, Cin, Cout, 5, 1, L)
    with ops.conv_math('fp32'):
        n_direct = _lib.size('gn_conv1d_wgrad_workspace', *args)
    with ops.conv_math('wino'):
        n_wino = _lib.size('gn_conv1d_wgrad_workspace', *args)
        assert n_wino > n_direct
        ws = torch.empty(n_wino, dtype=torch.uint8, device=dev)
        with pytest.raises(_lib.GennetHipError, match='workspace'):
            _lib.call('gn_conv1d_wgrad', ops._p(x), ops._p(dy), ops._p(dw), ops._p(db), ops._p(ws), n_direct, B, L, Cin, Cout, 5, 1, 2, L, ops._stream())
        _lib.call('gn_conv1d_wgrad', ops._p(x), ops._p(dy), ops._p(dw), ops._p(db), ops._p(ws), n_wino, B, L, Cin, Cout, 5, 1, 2, L, ops._stream())
        dw_ref, db_ref = ops.conv1d_wgrad(x, dy, 5, 1, 2)
    assert torch.equal(dw, dw_ref) and torch.equal(db, db_ref)


# ---------------------------------------------------------------------------------------------- stride-2 layers: F(2,3) + F(2,2) (csrc/conv_wino_s2.hip)
S2_CASES = [
    # B, L, Cin, Cout, padding          (pad_left parity decides which output phase the 3-tap half of the data gradient writes and where the 2-tap rows start)
    (2, 64, 64, 64, 'same'),            # pad_left 1
    (3, 133, 64, 128, 'valid'),         # pad_left 0, odd lengths: ragged last output pair
    (2, 151, 64, 64, 'same'),           # pad_left 2
    (2, 150, 128, 256, 'same'),
    (1, 300, 256, 128, 'valid'),
    (2, 6, 64, 64, 'valid'),            # one output row
    (2, 1, 64, 64, 'same'),             # one INPUT row: every tap but one reads padding
    (3, 3, 64, 128, 'same'),            # two output rows, three input rows
    (2, 1024, 512, 1024, 'same'),       # the discriminator's folded second Conv2D (bbhMahoGANy.py:447), two elements
    (1, 1018, 512, 1024, 'valid'),      # the q branch's Conv1D(1024, 5, strides=2) (:386)
]


@pytest.mark.parametrize("B,L,Cin,Cout,padding", S2_CASES)
def test_stride2_forward_and_data_gradient(B, L, Cin, Cout, padding):
    """A stride-2 5-tap convolution = a 3-tap + a 2-tap unit-stride convolution on the even / odd rows; its data gradient = two phases of 3 and 2 taps over
    the same dy rows, one launch.  Seven multiplies per output pair instead of ten; the transforms are additions, so the error may not exceed the direct
    kernel's by more than rounding noise (gate: 1.5 x rms; measured 0.6-0.9 x)."""
    from gennet_amd import ops
    rng = np.random.RandomState(7 * L + B)
    x = f32(rng.randn(B, L, Cin)); lim = np.sqrt(6.0 / (5 * (Cin + Cout)))
    w = f32(rng.uniform(-lim, lim, (5, Cin, Cout))); b = f32(rng.randn(Cout) * 0.1)
    Lout, pl = ops.conv_geometry(L, 5, 2, padding)
    pre = K.conv1d_fwd(x, w, b, 2, padding)
    ref = np.where(pre > 0, pre, float(np.float32(0.2)) * pre)
    dy = f32(rng.randn(B, Lout, Cout))
    dx_ref, _, _ = K.conv1d_bwd(x, w, dy, 2, padding)
    wt = ops.conv1d_transpose_w(g(w))
    y_prev = f32(np.maximum(rng.randn(B, L, Cin), 0.0))
    out = {}
    ops.prof_enable(True)
    try:
        for math in ('wino', 'fp32'):
            with ops.conv_math(math):
                ops.prof_reset()
                y = ops.conv1d_fwd(g(x), g(w), g(b), 2, pl, Lout, 'leaky', 0.2)
                dx = ops.conv1d_dgrad(g(dy), wt, L, 2, pl)
                dxf = ops.conv1d_dgrad(g(dy), wt, L, 2, pl, prev=(g(y_prev), 'relu', 0.0, None, 0.0))
                out[math] = (y, dx, dxf, launches(7))
    finally:
        ops.prof_enable(False)
    # forward, data gradient, fused data gradient took the transform-domain kernel (a data gradient onto fewer than two input rows stays on the direct kernel)
    assert out['wino'][3] == (3 if L >= 2 else 1) and out['fp32'][3] == 0
    (mw, rw), (md, rd) = errs(out['wino'][0], ref), errs(out['fp32'][0], ref)
    assert mw <= RTOL and (Lout < 16 or rw <= 1.5 * rd + 1e-8), (mw, rw, md, rd)
    (mw, rw), (md, rd) = errs(out['wino'][1], dx_ref), errs(out['fp32'][1], dx_ref)
    assert mw <= RTOL and (L < 16 or rw <= 1.5 * rd + 1e-8), (mw, rw, md, rd)
    assert errs(out['wino'][2], dx_ref * (y_prev > 0))[0] <= RTOL
    # a batch and its halves: the same kernel, bit for bit
    if B >= 2:
        with ops.conv_math('wino'):
            h = B // 2
            y2 = torch.cat([ops.conv1d_fwd(g(x[:h]), g(w), g(b), 2, pl, Lout, 'leaky', 0.2), ops.conv1d_fwd(g(x[h:]), g(w), g(b), 2, pl, Lout, 'leaky', 0.2)])
        assert torch.equal(y2, out['wino'][0])


def test_stride2_batchnorm_statistics_and_dropout_epilogue():
    from gennet_amd import ops
    rng = np.random.RandomState(19)
    B, L, Cin, Cout = 3, 150, 64, 128
    x = f32(rng.randn(B, L, Cin)); w = f32(rng.randn(5, Cin, Cout) * 0.05); b = f32(rng.randn(Cout))
    Lout, pl = ops.conv_geometry(L, 5, 2, 'same')
    pre = K.conv1d_fwd(x, w, b, 2, 'same')
    keep = rng.rand(B, Lout, Cout) >= 0.4
    ref = np.where(pre > 0, pre, float(np.float32(0.2)) * pre) * keep / float(np.float32(0.6))
    ops.prof_enable(True); ops.prof_reset()
    try:
        with ops.conv_math('wino'):
            y = ops.conv1d_fwd_dropout(g(x), g(w), g(b), g(keep, torch.uint8), 2, pl, Lout, 'leaky', 0.2, 0.4)
            ys, sums = ops.conv1d_fwd_stats(g(x), g(w), g(b), 2, pl, Lout)
            assert launches(7) == 2
    finally:
        ops.prof_enable(False)
    assert errs(y, ref)[0] <= 2 * RTOL and errs(ys, pre)[0] <= RTOL
    yh = ys.cpu().numpy().astype(np.float64).reshape(-1, Cout)
    s = sums.cpu().numpy()
    assert np.allclose(s[:Cout], yh.sum(0), rtol=1e-12, atol=1e-9) and np.allclose(s[Cout:], (yh * yh).sum(0), rtol=1e-12)


# ---------------------------------------------------------------------------------------------- weight gradients (csrc/wgrad_wino.hip, csrc/wgrad_wino_s2.hip)
WGRAD_CASES = [
    # B, L, Cin, Cout, stride, padding
    (2, 64, 64, 64, 1, 'same'), (3, 133, 64, 128, 1, 'valid'), (2, 301, 256, 128, 1, 'same'), (40, 517, 64, 64, 1, 'valid'),        # the last: several K splits
    (2, 64, 64, 64, 2, 'same'), (3, 133, 64, 128, 2, 'valid'), (2, 151, 64, 64, 2, 'same'), (1, 300, 256, 128, 2, 'valid'), (2, 6, 64, 64, 2, 'valid'),
    (40, 1018, 64, 128, 2, 'valid'),                                                                                                 # several K splits
    (2, 1, 64, 64, 2, 'same'), (3, 3, 64, 128, 2, 'same'), (2, 1, 64, 64, 1, 'same'), (3, 2, 64, 128, 1, 'same'),                    # fewer input rows than taps
    (2, 1024, 512, 1024, 2, 'same'),                                                                                                 # bbhMahoGANy.py:447 folded, two elements
]


@pytest.mark.parametrize("B,L,Cin,Cout,stride,padding", WGRAD_CASES)
def test_weight_gradient_against_oracle_and_direct_kernel(B, L, Cin, Cout, stride, padding):
    """dW = G^T [ sum over rows (B^T x) * (A dy) ]: the transposed algorithm, per-point partial sums in fp32, the inverse transform and the sum over the K
    splits in fp64 (one rounding per tap).  Unit stride: 6 multiplies per output pair instead of 10; stride 2: 7 instead of 10, additions only.  Against
    the fp64 oracle to the direct kernel's tolerance, rms no worse than 1.5 x (stride 1: 4 x, Gate 1's bound) the direct kernel's; the bias gradient is a
    separate fp64 pass; a repeat is bit-identical (fixed split plan, no atomics)."""
    from gennet_amd import ops
    rng = np.random.RandomState(11 * L + B + stride)
    x = f32(rng.randn(B, L, Cin))
    Lout, pl = ops.conv_geometry(L, 5, stride, padding)
    dy = f32(rng.randn(B, Lout, Cout))
    _, dw_ref, db_ref = K.conv1d_bwd(x, np.zeros((5, Cin, Cout)), dy, stride, padding)
    out = {}
    ops.prof_enable(True)
    try:
        for math in ('wino', 'fp32'):
            with ops.conv_math(math):
                ops.prof_reset()
                dw, db = ops.conv1d_wgrad(g(x), g(dy), 5, stride, pl)
                dw2, _ = ops.conv1d_wgrad(g(x), g(dy), 5, stride, pl)
                out[math] = (dw, db, launches(6 if stride == 1 else 8), launches(1))
                assert torch.equal(dw, dw2)
    finally:
        ops.prof_enable(False)
    assert out['wino'][2] == 2 and out['wino'][3] == 0 and out['fp32'][2] == 0 and out['fp32'][3] == 2
    (mw, rw), (md, rd) = errs(out['wino'][0], dw_ref), errs(out['fp32'][0], dw_ref)
    assert mw <= RTOL and rw <= (4.0 if stride == 1 else 1.5) * rd + 1e-8, (mw, rw, md, rd)
    assert errs(out['wino'][1], db_ref)[0] <= 1e-6


def test_random_shapes_agree_with_the_direct_kernels():
    """60 random launches (both strides and paddings, odd chunk counts, ragged row and column tiles, 1-row inputs) of forward, data gradient and weight
    gradient: transform-domain against direct kernels at the kernels' tolerance.  Both families are pinned on the oracle separately: the conv
    parity tables of tests/test_kernels_gpu.py, test_tapfold_gpu.py and test_edges_gpu.py run every case under 'fp32' and under 'wino'."""
    from gennet_amd import ops
    rng = np.random.RandomState(2025)
    dev = torch.device('cuda:0')
    worst = 0.0
    for it in range(60):
        stride = int(rng.choice([1, 2]))
        padding = str(rng.choice(['same', 'valid']))
        Cin = int(rng.choice([32, 40, 64, 72, 128, 192, 320]))
        Cout = int(rng.choice([64, 128, 192, 256]))
        B = int(rng.randint(1, 6))
        L = int(rng.randint(5 if padding == 'valid' else 1, 700))
        act = str(rng.choice(['linear', 'relu', 'tanh', 'leaky']))
        Lout, pl = ops.conv_geometry(L, 5, stride, padding)
        x = torch.tensor(rng.randn(B, L, Cin), dtype=torch.float32, device=dev)
        w = torch.tensor(rng.randn(5, Cin, Cout) * np.sqrt(2.0 / (5 * Cin)), dtype=torch.float32, device=dev)
        b = torch.tensor(rng.randn(Cout) * 0.1, dtype=torch.float32, device=dev)
        dy = torch.tensor(rng.randn(B, Lout, Cout), dtype=torch.float32, device=dev)
        wt = ops.conv1d_transpose_w(w)
        res = {}
        for math in ('wino', 'fp32'):
            with ops.conv_math(math):
                res[math] = (ops.conv1d_fwd(x, w, b, stride, pl, Lout, act, 0.2), ops.conv1d_dgrad(dy, wt, L, stride, pl), ops.conv1d_wgrad(x, dy, 5, stride, pl)[0])
        for k, (a_, d_) in enumerate(zip(res['wino'], res['fp32'])):
            e = float((a_ - d_).abs().max() / d_.abs().max().clamp_min(1e-30))
            worst = max(worst, e)
            assert e <= RTOL, (it, k, B, L, Cin, Cout, stride, padding, act, e)
    print('worst relative difference %.2e' % worst)


@pytest.mark.parametrize("Cin,Cout,L,stride,B", [(64, 128, 2048, 1, 256), (128, 256, 2044, 1, 256), (512, 1024, 2048, 1, 32), (256, 512, 2040, 2, 128), (512, 1024, 1018, 2, 64)])
def test_repeated_launches_are_bit_identical(Cin, Cout, L, stride, B):
    """Determinism stress (round 5): forward, data gradient and weight gradient of one launch repeated eight times must agree bit for bit -- no atomics, fixed
    split plans, fixed reduction orders; what this guards against is a RACE inside the hand-scheduled loops.  It was written after one was seen: with the
    transform's vector instructions grouped in runs behind an MFMA (scripts/valu_rate.hip: 7 instead of 16 cycles each) the F(2,5) forward kernel returned, once
    in a few launches, a wrong accumulator register PAIR in one wave -- invisible to every tolerance test, caught only by the bit-for-bit predict comparison of
    tests/test_bench_sizes_gpu.py.  Cause: LDS-DMA (buffer_load ... lds) at times writes into v[0:3], its unused VDATA field; the library now declares that clobber
    at every LDS-DMA statement (csrc/common.h, gn_buffer_load_lds) and the runs are in (profiles/r05_winograd_gate.txt has the record; soak:
    tests/tools/determinism_soak.py)."""
    from gennet_amd import ops
    dev = torch.device('cuda:0')
    x = ops.fill_normal((B, L, Cin), 0.0, 1.0, 3, 0, dev); w = ops.fill_normal((5, Cin, Cout), 0.0, 0.05, 4, 0, dev)
    Lout, pl = ops.conv_geometry(L, 5, stride, 'valid')
    dy = ops.fill_normal((B, Lout, Cout), 0.0, 1.0, 5, 0, dev)
    wt = ops.conv1d_transpose_w(w)
    with ops.conv_math('wino'):
        first = None
        for rep in range(8):
            got = (ops.conv1d_fwd(x, w, None, stride, pl, Lout, 'relu'), ops.conv1d_dgrad(dy, wt, L, stride, pl), ops.conv1d_wgrad(x, dy, 5, stride, pl)[0])
            if first is None:
                first = got
            else:
                for name, a, b in zip(('forward', 'data gradient', 'weight gradient'), got, first):
                    assert torch.equal(a, b), (name, rep, int((a != b).sum()), float((a - b).abs().max()))
