"""GPU tests of Conv1D(dilation_rate=d, padding='causal').

Section 1.  The two passes of csrc/dilate.hip through ops.dilate_split / ops.dilate_merge, bit-identical to tests/dilated_ref.py (copies and +0
fills; the sign of every zero is compared).  Inputs sit in NaN-surrounded buffers, outputs in sentinel-filled ones; a view starts 144 bytes in
(pad 36: 16-byte aligned) or 148 bytes in (pad 37: a C % 4 == 0 tensor then takes the scalar path).  A lane owns one unit of the output on at
most 2048 blocks of 256: 16 * 517 * 64 scalar units and 16 * 517 * 256 / 4 float4 units are a second trip.
Section 2.  The layer isolated from kernel numerics: a dilated / causal Conv1D is torch.equal in y, dx, dw, db to the undilated 'valid' Conv1D of
the same weights run on the HOST-computed split of the input, its outputs merged on the host -- the same kernels see the same operand bits.
Section 3.  The layer against torch fp64.  Bounds: those of the existing parity tests of the kernel each case reaches -- 2e-5 of the largest
reference entry for y and dx (tests/test_kernels_gpu.py RTOL, test_wino_gpu.py, test_tapfold_gpu.py, test_conv_anyc_gpu.py); dw and db 5e-5
(test_kernels_gpu.py: direct, transform-domain and small-channel kernels), 2e-5 on the any-channel kernels (test_conv_anyc_gpu.py), and for a
tap-folded layer (k > 5) on the strict kernels dw 2e-5, db 1e-6 (test_tapfold_gpu.py).  Those tests hand one dy to both sides; here the layer has an
activation, so the reference's upstream gradient of the pre-activation is dy * act'(y) at the y the GPU wrote (itself bounded above): the conv
gradients are then compared for the same incoming gradient, and a LeakyReLU branch decided within rounding of 0 cannot flip between the sides.
Section 4.  A residual stack of dilated causal convolutions: tests/test_merge_gpu.py's bounds for its residual models -- the loss 1e-6 relative,
SGD-updated weights 1e-4 of each tensor's largest entry (floor 1e-3) -- for each of three steps, the reference starting each step from the weights
the GPU holds (so each is that single-step bound); save / load; a captured step."""
import os
import types

import numpy as np
import pytest
import torch

import dilated_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5


def dev():
    return torch.device('cuda:0')


def g(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device=dev())


def f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


class Guarded(object):
    """A contiguous view `pad` floats into a larger flat buffer: inputs surrounded by NaN, outputs inside a sentinel-filled buffer."""

    def __init__(self, shape, value=None, pad=37):
        self.n, self.pad = int(np.prod(shape)), pad
        self.buf = torch.full((self.n + 2 * pad,), float('nan') if value is not None else SENTINEL, dtype=torch.float32, device=dev())
        self.t = self.buf[pad:pad + self.n].view(shape)
        if value is not None:
            self.t.copy_(torch.tensor(np.ascontiguousarray(value, np.float32), device=dev()))
        assert self.t.is_contiguous() and self.t.data_ptr() == self.buf.data_ptr() + 4 * pad and (self.t.data_ptr() % 16 == 0) == (pad % 4 == 0)

    def check(self, what):
        """the surroundings untouched, every element of the view written"""
        edges = torch.cat([self.buf[:self.pad], self.buf[self.pad + self.n:]])
        assert bool((edges == SENTINEL).all()), '%s: wrote outside its output' % what
        assert not bool((self.t == SENTINEL).any()), '%s: output elements left unwritten' % what
        assert not bool(torch.isnan(self.t).any()), '%s: NaN (an element outside an input was read)' % what
        return self.t.cpu().numpy()

    def untouched(self):
        return bool((self.buf == SENTINEL).all())


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a, b) and np.array_equal(np.signbit(a), np.signbit(b)) and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------
# section 1: the passes
# ---------------------------------------------------------------------------------------------------------------------
# B, L, C, d, off, M
PASSES = [(2, 11, 1, 3, 0, 4),              # one channel: scalar units; L % d != 0
          (2, 11, 4, 3, 3, 5),              # one float4 per row, off = 3
          (2, 11, 6, 3, 6, 6),              # odd width: scalar whatever the alignment; off = d * (k - 1), k = 3
          (3, 37, 64, 2, 8, 23),            # wide; off = d * (k - 1), k = 5
          (2, 9, 4, 1, 4, 13),              # d = 1, off > 0: the pad-only case
          (2, 9, 6, 1, 3, 12),
          (2, 5, 4, 7, 0, 3),               # d > L: whole phases empty, and M forced up to k = 3 (ceil(5 / 7) = 1)
          (2, 5, 6, 9, 16, 3),              # ... with off = d * (k - 1) + ..., ceil(21 / 9) = 3
          (1, 1, 1, 1, 0, 1),
          (2, 10, 4, 2, 3, 3),              # M short of the input: rows are dropped (split only)
          (8, 1030, 64, 2, 3, 517),         # 529408 scalar units (pad 37): a second trip
          (8, 1030, 256, 2, 3, 517)]        # 529408 float4 units: a second trip


def signed_zero_input(rng, shape):
    x = rng.randn(*shape).astype(np.float32)
    x[rng.rand(*shape) < 0.1] = 0.0
    x[rng.rand(*shape) < 0.1] = -0.0
    return x


@pytest.mark.parametrize('pads', [(36, 36), (37, 37), (36, 37)], ids=['aligned', 'offset-one-float', 'mixed'])
@pytest.mark.parametrize('B,L,C,d,off,M', PASSES, ids=['-'.join(map(str, c)) for c in PASSES])
def test_split_and_merge_are_bit_identical_to_the_reference(B, L, C, d, off, M, pads):
    from gennet_amd import ops
    rng = np.random.RandomState(L * 7 + C + d)
    x = signed_zero_input(rng, (B, L, C))
    ref = R.split(x, d, off, M)
    gx, out = Guarded(x.shape, x, pads[0]), Guarded(ref.shape, None, pads[1])
    assert ops.dilate_split(gx.t, d, off, M, out=out.t) is out.t
    xs = out.check('split')
    assert same_bits(xs, ref)                                              # the reference's fill is +0, its copies keep the sign of a zero
    filled = R.split(np.ones_like(x), d, off, M) == 0
    assert not np.signbit(xs[filled]).any() and not (xs[filled] != 0).any()
    if (L - 1 + off) // d >= M:
        return
    q = signed_zero_input(rng, (B * d, M, C))
    gq, back = Guarded(q.shape, q, pads[0]), Guarded(x.shape, None, pads[1])
    ops.dilate_merge(gq.t, B, d, off, L, out=back.t)
    assert same_bits(back.check('merge'), R.merge(q, B, d, off, L))
    # the round trip, on tensors the allocator aligned
    assert same_bits(ops.dilate_merge(ops.dilate_split(gx.t, d, off, M), B, d, off, L).cpu().numpy(), x)


def test_bad_arguments_are_errors_and_launch_nothing():
    from gennet_amd import _lib, ops
    B, L, C, d, off, M = 2, 11, 4, 3, 3, 5
    x = Guarded((B, L, C), np.ones((B, L, C), np.float32), 36)
    xs = Guarded((B * d, M, C), np.ones((B * d, M, C), np.float32), 36)
    out = Guarded((B * d, M, C), None, 36)
    s = torch.cuda.current_stream().cuda_stream
    px, pxs, po = x.t.data_ptr(), xs.t.data_ptr(), out.t.data_ptr()

    def refused(text, fn):
        with pytest.raises(_lib.GennetHipError) as e:
            fn()
        assert text in str(e.value) and '(%d)' % _lib.GN_EINVAL in str(e.value), str(e.value)
        torch.cuda.synchronize()
        assert out.untouched()

    def split(a, b, B, L, C, d, off, M):
        _lib.call('gn_dilate_split', a, b, B, L, C, d, off, M, s)

    def merge(a, b, B, L, C, d, off, M):
        _lib.call('gn_dilate_merge', a, b, B, L, C, d, off, M, s)

    for what, entry, src in (('dilate_split', split, px), ('dilate_merge', merge, pxs)):
        refused('%s: null pointer' % what, lambda: entry(None, po, B, L, C, d, off, M))
        refused('%s: null pointer' % what, lambda: entry(src, None, B, L, C, d, off, M))
        for bad in range(5):
            dims = [B, L, C, d, M]
            for v in (0, -1):
                dims[bad] = v
                refused('%s: B %d, L %d, C %d, d %d, M %d must all be >= 1' % ((what,) + tuple(dims)),
                        lambda: entry(src, po, dims[0], dims[1], dims[2], dims[3], off, dims[4]))
        refused('%s: off -1 must be >= 0' % what, lambda: entry(src, po, B, L, C, d, -1, M))
    # the merge reads row (L - 1 + off) / d of a phase: (11 - 1 + 3) / 3 = 4 < 5 is the last one there is
    refused('but xs has M = 4 rows', lambda: _lib.call('gn_dilate_merge', pxs, po, B, L, C, d, off, 4, s))
    refused('but xs has M = 5 rows', lambda: _lib.call('gn_dilate_merge', pxs, po, B, L + 2, C, d, off, 5, s))
    refused('but xs has M = 5 rows', lambda: _lib.call('gn_dilate_merge', pxs, po, B, L, C, d, off + 2, 5, s))
    with pytest.raises(ValueError):
        ops.dilate_merge(xs.t, B + 1, d, off, L)
    with pytest.raises(ValueError):
        ops.dilate_split(x.t.permute(1, 0, 2), d, off, M)                  # not contiguous
    _lib.call('gn_dilate_merge', pxs, po, B, L, C, d, off, M, s)           # the same arguments inside the bound run
    torch.cuda.synchronize()
    assert not out.untouched()


def test_indexing_beyond_2_to_31_elements():
    """(1, 2^25 + 1024, 64) holds 2^31 + 65536 floats, and so do its two phases: element offsets pass 2^31 in x and in xs (size_t, no 32-bit
    wrap), in the float4 path.  Both ends of both tensors are checked; the middle is whatever the allocator left (copies do not care)."""
    from gennet_amd import ops
    L, C, d, off = (1 << 25) + 1024, 64, 2, 3
    M = -(-(L + off) // d)
    x = torch.empty((1, L, C), dtype=torch.float32, device=dev())
    ends = torch.arange(16 * C, dtype=torch.float32, device=dev()).view(16, C)
    x[0, :16] = ends + 1.0
    x[0, -16:] = -(ends + 1.0)
    xs = ops.dilate_split(x, d, off, M)
    assert tuple(xs.shape) == (2, M, C) and xs.numel() > (1 << 31)
    for i in list(range(16)) + list(range(L - 16, L)):
        assert torch.equal(xs[(i + off) % d, (i + off) // d], x[0, i]), i
    assert float(xs[0, 0].abs().max()) == 0.0 and float(xs[1, 0].abs().max()) == 0.0 and float(xs[0, 1].abs().max()) == 0.0      # rows -3, -2, -1
    assert (L + off) % d == 1 and float(xs[1, M - 1].abs().max()) == 0.0                                                        # row L: past the end
    head, tail = x[0, :16].clone(), x[0, -16:].clone()
    del x
    back = ops.dilate_merge(xs, 1, d, off, L)
    assert torch.equal(back[0, :16], head) and torch.equal(back[0, -16:], tail)
    del xs, back
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------------
# sections 2 and 3: one layer
# ---------------------------------------------------------------------------------------------------------------------
ALL_KINDS = tuple(range(18))


def run_layer(layer, in_shape, x, w, b, dy):
    """-> (y, dx, dw, db, {counter kind: launches}) of one forward and backward of a Conv1D outside a model (no planner fusion on the node)"""
    from gennet_amd import ops
    from gennet_amd.engine import RunContext
    layer.build(in_shape)
    layer.kernel.assign(w); layer.bias.assign(b)
    layer.kernel.grad = torch.zeros(w.shape, dtype=torch.float32, device=dev())
    layer.bias.grad = torch.zeros(b.shape, dtype=torch.float32, device=dev())
    node = types.SimpleNamespace(index=0, fused_act=None, fused_drop=None, fold_up=None, infer_bn=None, lazy_bn=-1, fuse_prev=-1)
    ctx = RunContext(True)
    was = ops.prof_enabled()
    ops.prof_enable(True)
    try:
        ops.prof_reset()
        y = layer.forward(ctx, node, g(x))
        dx = layer.backward(ctx, node, g(dy), True, True)
        torch.cuda.synchronize()
        counts = {k: ops.prof_collect(k)['launches'] for k in ALL_KINDS}
    finally:
        ops.prof_enable(was)
    return y, dx, layer.kernel.grad, layer.bias.grad, {k: v for k, v in counts.items() if v}


# B, L, Cin, Cout, k, d, stride, padding; a counter kind the forward must show under 'wino' (csrc/common.h prof_end), None: not asserted
ISOLATED = [(2, 21, 2, 8, 3, 3, 1, 'causal', 11),         # small-Cin
            (2, 70, 64, 64, 5, 2, 1, 'same', 5),          # the transform-domain default
            (2, 37, 3, 5, 4, 2, 1, 'same', 9),            # the any-channel kernels
            (2, 45, 8, 8, 8, 3, 1, 'valid', None),        # tap fold: 2 groups of 4 taps over 16 channels
            (2, 60, 4, 4, 40, 2, 1, 'causal', None),      # 40 taps: 8 groups of 5 over 32 channels
            (2, 33, 8, 8, 3, 1, 2, 'causal', None)]       # causal without dilation at stride 2: the split only pads, nothing is merged


@pytest.mark.parametrize('math', ['wino', 'fp32'])
@pytest.mark.parametrize('B,L,Cin,Cout,k,d,stride,padding,kind', ISOLATED, ids=['-'.join(map(str, c[:8])) for c in ISOLATED])
def test_the_layer_is_the_undilated_valid_layer_on_the_split_input_bit_for_bit(B, L, Cin, Cout, k, d, stride, padding, kind, math):
    from gennet_amd import ops
    from gennet_amd.layers import Conv1D
    rng = np.random.RandomState(L + k + d)
    x = rng.randn(B, L, Cin).astype(np.float32)
    w = (rng.randn(k, Cin, Cout) / np.sqrt(k * Cin)).astype(np.float32)
    b = rng.randn(Cout).astype(np.float32)
    Lout, pl, pr = R.geometry(L, k, stride, padding, d)
    M = R.phase_rows(L, k, d, pl, pr)
    Lrun = (M - k) // stride + 1
    dy = rng.randn(B, Lout, Cout).astype(np.float32)
    with ops.conv_math(math):
        y, dx, dw, db, counts = run_layer(Conv1D(Cout, k, strides=stride, padding=padding, dilation_rate=d, activation='tanh'), (L, Cin), x, w, b, dy)
        ys, dxs, dw0, db0, counts0 = run_layer(Conv1D(Cout, k, strides=stride, padding='valid', activation='tanh'), (M, Cin),
                                               R.split(x, d, pl, M), w, b, R.split(dy, d, 0, Lrun))
    print(math, 'launches', counts)
    assert tuple(y.shape) == (B, Lout, Cout) and tuple(dx.shape) == (B, L, Cin) and tuple(ys.shape) == (B * d, Lrun, Cout)
    assert counts == counts0 and sum(counts.values()) >= 3                 # the same kernels, in all three directions
    if kind is not None and math == 'wino':
        assert counts.get(kind, 0) >= 1, counts
    assert same_bits(y.cpu().numpy(), R.merge(ys.cpu().numpy(), B, d, 0, Lout))
    assert same_bits(dx.cpu().numpy(), R.merge(dxs.cpu().numpy(), B, d, pl, L))
    assert torch.equal(dw, dw0) and torch.equal(db, db0)
    assert float(dw.abs().max()) > 0 and float(db.abs().max()) > 0 and float(dx.abs().max()) > 0


# the seven shapes of tests/test_dilated_cpu.py and 64 -> 64 on the transform-domain kernels: B, L, Cin, Cout, k, d, padding
AGAINST_TORCH = [(2, 37, 3, 5, 5, 2, 'same'), (1, 16, 4, 4, 3, 4, 'causal'), (3, 50, 2, 6, 8, 3, 'valid'), (2, 9, 1, 2, 2, 7, 'same'),
                 (2, 5, 2, 2, 3, 2, 'causal'), (1, 23, 4, 8, 5, 9, 'same'), (2, 40, 4, 4, 40, 1, 'causal'), (2, 130, 64, 64, 5, 2, 'causal')]


def rel(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-30)


@pytest.mark.parametrize('act,p', [('tanh', 0.0), ('leaky', 0.2)])
@pytest.mark.parametrize('B,L,Cin,Cout,k,d,padding', AGAINST_TORCH, ids=['-'.join(map(str, c)) for c in AGAINST_TORCH])
def test_the_layer_against_torch_fp64(B, L, Cin, Cout, k, d, padding, act, p):
    from gennet_amd import layers as Ly, ops
    rng = np.random.RandomState(L * 3 + k + d)
    x, w, b = f32(rng.randn(B, L, Cin)), f32(rng.randn(k, Cin, Cout) / np.sqrt(k * Cin)), f32(rng.randn(Cout))
    Lout = R.geometry(L, k, 1, padding, d)[0]
    dy = f32(rng.randn(B, Lout, Cout))
    layer = Ly.Conv1D(Cout, k, padding=padding, dilation_rate=d)
    node = types.SimpleNamespace(index=0, fused_act=(act, float(np.float32(p))), fused_drop=None, fold_up=None, infer_bn=None, lazy_bn=-1, fuse_prev=-1)
    from gennet_amd.engine import RunContext
    layer.build((L, Cin))
    layer.kernel.assign(w.astype(np.float32)); layer.bias.assign(b.astype(np.float32))
    layer.kernel.grad, layer.bias.grad = torch.zeros(w.shape, dtype=torch.float32, device=dev()), torch.zeros(b.shape, dtype=torch.float32, device=dev())
    ctx = RunContext(True)
    with ops.conv_math(ops.default_conv_math()):                           # the math a model runs: 64 -> 64 on the transform-domain kernels
        y = layer.forward(ctx, node, g(x))
        y_gpu = y.cpu().numpy().astype(np.float64)
        dx = layer.backward(ctx, node, g(dy), True, True)
    # the oracle: torch fp64, the activation's slope as float32 (the kernels' parameter)
    pp = float(np.float32(p))
    xt, wt, bt = (torch.tensor(a, requires_grad=True) for a in (x, w, b))
    y_ref = R.torch_layer(xt, wt, bt, 1, padding, d, act, pp).detach().numpy()
    z = R.torch_layer(xt, wt, bt, 1, padding, d)
    z.backward(torch.tensor(dy * R.act_grad_from_y(y_gpu, act, pp)))
    Cin_run = Cin * ops.tap_groups(k)[0] if k > 5 else Cin
    anyc = ops.conv_layer_needs_any(Cin_run, Cout)
    tol_dw, tol_db = (2e-5, 2e-5) if anyc else (2e-5, 1e-6) if k > 5 else (5e-5, 5e-5)
    errs = (rel(y_gpu, y_ref), rel(dx.cpu().numpy(), xt.grad.numpy()), rel(layer.kernel.grad.cpu().numpy(), wt.grad.numpy()),
            rel(layer.bias.grad.cpu().numpy(), bt.grad.numpy()))
    print('anyc' if anyc else 'strict', 'tap-folded' if k > 5 else '', 'y %.3g dx %.3g dw %.3g (bound %.0e) db %.3g (bound %.0e)'
          % (errs[0], errs[1], errs[2], tol_dw, errs[3], tol_db))
    assert errs[0] <= 2e-5 and errs[1] <= 2e-5 and errs[2] <= tol_dw and errs[3] <= tol_db, errs


# ---------------------------------------------------------------------------------------------------------------------
# section 4: a residual stack of dilated causal convolutions
# ---------------------------------------------------------------------------------------------------------------------
LR, RATE, DILATIONS = 0.05, 0.5, (1, 2, 4)


def stack_model():
    from gennet_amd import layers as Ly
    from gennet_amd.engine import Input, Model
    x0 = Input((32, 16))
    h, blocks = x0, []
    for i, d in enumerate(DILATIONS):
        conv = Ly.Conv1D(16, 3, padding='causal', dilation_rate=d, activation='tanh', name='conv_d%d' % d)
        drop, bn = Ly.Dropout(RATE, name='drop_d%d' % d), Ly.BatchNormalization(name='bn_d%d' % d)
        h = bn(Ly.Add()([drop(conv(h)), h]))
        blocks.append((conv, drop, bn))
    head = Ly.Dense(2, name='head')
    return Model(inputs=x0, outputs=head(Ly.GlobalAveragePooling1D()(h))), blocks, head


def stack_ref(P, x, masks):
    """the model in torch fp64, training phase: P {layer name: [tensors]}, masks {Dropout name: keep mask}"""
    h = x
    for d in DILATIONS:
        c = R.torch_layer(h, P['conv_d%d' % d][0], P['conv_d%d' % d][1], 1, 'causal', d, 'tanh')
        s = c * masks['drop_d%d' % d] / (1.0 - RATE) + h
        mean, var = s.mean((0, 1)), s.var((0, 1), unbiased=False)
        h = (s - mean) / torch.sqrt(var + 1e-3) * P['bn_d%d' % d][0] + P['bn_d%d' % d][1]
    return h.mean(1) @ P['head'][0] + P['head'][1]


def seed_weights(model, rng):
    """biases, gammas and betas off their 0 / 1 initial values"""
    for l in model.layers:
        ws = l.get_weights()
        if len(ws) == 2:
            l.set_weights([ws[0], (0.1 * rng.randn(*ws[1].shape)).astype(np.float32)])
        elif len(ws) == 4:
            l.set_weights([(1.0 + 0.1 * rng.randn(*ws[0].shape)).astype(np.float32), (0.1 * rng.randn(*ws[1].shape)).astype(np.float32)] + ws[2:])


def test_a_residual_stack_of_dilated_causal_convs_trains_like_torch_fp64():
    from gennet_amd.engine import SGD
    model, blocks, head = stack_model()
    rng = np.random.RandomState(11)
    seed_weights(model, rng)
    kinds = [type(n.layer).__name__ for n in model.nodes]
    assert kinds == ['Conv1D', 'Dropout', 'Add', 'BatchNormalization'] * 3 + ['GlobalAveragePooling1D', 'Dense']
    model.compile(optimizer=SGD(lr=LR), loss='mean_squared_error')
    model._plan()
    assert all(not n.absorbed and n.fused_drop is None and n.fuse_prev == -1 and n.infer_bn is None for n in model.nodes)      # every layer runs on its own
    x, t = rng.randn(4, 32, 16).astype(np.float32), rng.randn(4, 2).astype(np.float32)
    trained = [l for l in model.layers if l.weights]
    assert len(trained) == 7
    for step in range(3):
        masks = dict((drop.name, (rng.rand(4, 32, 16) >= RATE).astype(np.uint8)) for _, drop, _ in blocks)
        P = dict((l.name, [torch.tensor(a.astype(np.float64), requires_grad=True) for a in l.get_weights()[:2]]) for l in trained)
        out = stack_ref(P, torch.tensor(x.astype(np.float64)), dict((k, torch.tensor(v.astype(np.float64))) for k, v in masks.items()))
        loss_ref = ((out - torch.tensor(t.astype(np.float64))) ** 2).mean()
        loss_ref.backward()
        loss = float(np.ravel(model.train_on_batch(x, t, dropout_masks=masks))[0])
        print('step %d loss %.9g reference %.9g' % (step, loss, float(loss_ref.detach())))
        assert abs(loss - float(loss_ref.detach())) <= 1e-6 * abs(float(loss_ref.detach()))
        for l in trained:
            for name, got, ref in zip(('kernel / gamma', 'bias / beta'), l.get_weights()[:2], P[l.name]):
                w_ref = (ref.detach() - LR * ref.grad).numpy()
                werr = np.abs(got.astype(np.float64) - w_ref).max() / max(np.abs(w_ref).max(), 1e-3)
                moved = np.abs(LR * ref.grad.numpy()).max() / max(np.abs(w_ref).max(), 1e-3)
                print('step %d %s %s weight err %.3g (the step moved it by %.3g)' % (step, l.name, name, werr, moved))
                assert werr < 1e-4, (step, l.name, name, werr)
    assert max(float(np.abs(LR * v.grad.numpy()).max()) for ts in P.values() for v in ts) > 1e-3        # the steps are no rounding noise


def test_the_stack_saves_loads_and_predicts_identically(tmp_path):
    from gennet_amd.engine import SGD, load_model
    model, blocks, _ = stack_model()
    rng = np.random.RandomState(12)
    seed_weights(model, rng)
    x, t = rng.randn(4, 32, 16).astype(np.float32), rng.randn(4, 2).astype(np.float32)
    model.compile(optimizer=SGD(lr=LR), loss='mean_squared_error')
    model.train_on_batch(x, t)
    path = os.path.join(str(tmp_path), 'stack.h5')
    model.save(path)
    again = load_model(path)
    convs = [l for l in again.layers if type(l).__name__ == 'Conv1D']
    assert [(l.dilation, l.padding, l.phased) for l in convs] == [(d, 'causal', True) for d in DILATIONS]
    assert [n.inbound for n in again.nodes] == [n.inbound for n in model.nodes]
    y = model.predict(x)
    assert np.array_equal(y, again.predict(x)) and np.isfinite(y).all() and np.abs(y).max() > 0


def test_a_captured_step_of_the_stack_replays_bit_identically():
    """the stack as a hipGraph (engine.StepGraph), Dropout drawn on the device: eager step, capture, three replays against four eager steps of a
    twin that starts from the same weights and the same position of the device's random stream"""
    from gennet_amd import engine
    from gennet_amd.engine import SGD, to_device
    rng = np.random.RandomState(13)
    x, t = to_device(rng.randn(4, 32, 16).astype(np.float32)), to_device(rng.randn(4, 2).astype(np.float32))
    eager, _, _ = stack_model()
    seed_weights(eager, rng)
    graphed, _, _ = stack_model()
    graphed.set_weights(eager.get_weights())
    for m in (eager, graphed):
        m.compile(optimizer=SGD(lr=LR, momentum=0.5), loss='mean_squared_error')
    engine.set_device_seed(41)
    want = []
    for _ in range(4):
        want.append((eager.train_on_batch_device([x], [t]).cpu().numpy().copy(), [w.copy() for w in eager.get_weights()]))
    end = engine.device_rng().offset
    engine.set_device_seed(41)
    got = [(graphed.train_on_batch_device([x], [t]).cpu().numpy().copy(), [w.copy() for w in graphed.get_weights()])]
    sg = engine.StepGraph()
    torch.cuda.synchronize()
    sg.capture(lambda: graphed.train_on_batch_device([x], [t]))
    for _ in range(3):
        sg.wait_inputs_consumed()
        stats = sg.replay()
        torch.cuda.synchronize()
        got.append((stats.cpu().numpy().copy(), [w.copy() for w in graphed.get_weights()]))
    for step, ((s0, w0), (s1, w1)) in enumerate(zip(want, got)):
        assert np.array_equal(s0, s1), (step, s0, s1)
        assert all(np.array_equal(u, v) for u, v in zip(w0, w1)), step
    assert engine.device_rng().offset == end
    assert not np.array_equal(want[0][0], want[3][0])                      # the steps differ: a replay that did nothing would show
