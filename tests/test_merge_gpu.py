"""GPU parity of the merge layers: csrc/merge.hip through ops.merge_fwd / merge_bwd / scale / concat_fwd / concat_bwd against the numpy definition
tests/merge_ref.py (itself checked against torch autograd in tests/test_merge_cpu.py), and the seven layers at model level against torch fp64
autograd on the CPU.

Section 1.  Inputs sit in NaN-surrounded buffers, outputs in sentinel-filled ones; a view starts 148 bytes in (pad 37) or 144 bytes in (pad 36).
The element-wise kernels take a float4 body wherever y and every input are MUTUALLY 16-byte aligned: all views 144 bytes in (no head), all views
148 bytes in (a scalar head of 3 elements, then float4), and an all-scalar pass when one input is 148 and the others 144 bytes in.  The grid is
capped at 512 blocks of 256 = 131072 lanes for a float4 body and at 2048 blocks = 524288 lanes for an all-scalar pass, one item each and trip:
    n = 1, 3, 4, 7, 1030        shorter than the head, head only, head + one float4, tails, many float4 (k = 3); k = 2 and k = 8 at n = 1030
    n = 524295                  float4 body of 131073 items (pads 36 and 37: 524295 = 4 * 131073 + 3 = 3 + 4 * 131073): one lane takes a second trip
    n = 524293                  the all-scalar pass (mixed pads): five lanes take a second trip
Inputs: seeded normals with exact zeros from a 0.4-rate mask (so +0 and -0 both occur); for k >= 3 the first three quarters of the elements tie
inputs 0 and 2, then 1 and 2, then all three (k = 2: the first half ties both); the last element holds +-3e38 in input 0 and 0.5 elsewhere
(dy 0.5), so no sum, product or gradient of the reference overflows -- asserted on the reference.
Bound: forward and backward of all six modes bit-identical to merge_ref (comparisons, copies, single roundings, left-to-right chains; the build
has -ffp-contract=off), Average's one division included; Concatenate is copies: bit-identical.
Concatenate: one unit (float4 when every width % 4 == 0 and every pointer is 16-byte aligned, else one float) of y / dy per lane and trip, on at
most 2048 blocks = 524288 lanes for either unit: (1030, 256) + (1030, 255) is 526330 scalar units, (1030, 1024) + (1030, 1028) is 528390 float4
units (and 2113560 scalar ones 148 bytes in): a second trip each.

Section 2.  Bounds of tests/test_bn_axis_gpu.py's model tests as they stand: predict 1e-5 of the largest output, the loss 1e-6 relative, gradients
and SGD-updated weights 1e-4 of each tensor's largest entry (gradients no finer than 1e-3 of the model's largest gradient entry)."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import merge_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5


def dev():
    return torch.device('cuda:0')


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
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def elementwise_inputs(rng, n, k):
    xs = [(rng.randn(n) * (rng.rand(n) >= 0.4)).astype(np.float32) for _ in range(k)]
    if k >= 3:
        q = n // 4
        xs[2][:q] = xs[0][:q]
        xs[2][q:2 * q] = xs[1][q:2 * q]
        xs[1][2 * q:3 * q] = xs[0][2 * q:3 * q]
        xs[2][2 * q:3 * q] = xs[0][2 * q:3 * q]
    else:
        xs[1][:n // 2] = xs[0][:n // 2]
    dy = (rng.randn(n) * (rng.rand(n) >= 0.2)).astype(np.float32)
    xs[0][n - 1] = 3e38 if n % 2 else -3e38
    for x in xs[1:]:
        x[n - 1] = 0.5
    dy[n - 1] = 0.5
    return xs, dy


# n, k, pad of y (and dy / dx), pads of the inputs (None: all as y)
ELEMENTWISE = ([(n, 3, pad, None) for n in (1, 3, 4, 7, 1030) for pad in (37, 36)]
               + [(1030, 3, 36, (36, 37, 36)), (1030, 3, 37, (36, 36, 36)), (7, 2, 36, (37, 36))]
               + [(1030, k, pad, None) for k in (2, 8) for pad in (37, 36)]
               + [(524295, 2, 36, None), (524295, 3, 37, None), (524293, 3, 36, (36, 37, 36))])


@pytest.mark.parametrize('n,k,pad,xpads', ELEMENTWISE, ids=['n%d-k%d-pad%d%s' % (n, k, p, '' if xp is None else '-x' + '.'.join(map(str, xp)))
                                                            for n, k, p, xp in ELEMENTWISE])
def test_elementwise_passes_are_bit_identical_to_the_reference(n, k, pad, xpads):
    from gennet_amd import ops
    rng = np.random.RandomState(n % 9973 + 10 * k + pad)
    xs, dy = elementwise_inputs(rng, n, k)
    xpads = xpads or (pad,) * k
    gx = [Guarded((n,), x, p) for x, p in zip(xs, xpads)]
    gdy = Guarded((n,), dy, pad)
    if n >= 1030 and k >= 3:                                               # every tie pattern, and both zeros, are really there
        st = np.stack(xs[:3])
        assert ((st[0] == st[2]) & (st[0] != st[1])).any() and ((st[1] == st[2]) & (st[0] != st[1])).any() and ((st[0] == st[1]) & (st[1] == st[2])).any()
        assert (np.signbit(xs[0]) & (xs[0] == 0)).any() and (~np.signbit(xs[0]) & (xs[0] == 0)).any()
    for mode in R.MODES:
        kk = 2 if mode == 'sub' else k
        ref = R.merge_fwd(mode, xs[:kk])
        assert np.isfinite(ref).all(), mode
        out = Guarded((n,), None, pad)
        ops.merge_fwd(mode, [g.t for g in gx[:kk]], out=out.t)
        y = out.check('%s forward' % mode)
        assert same_bits(y, ref), (mode, 'forward', int((y.view(np.uint32) != ref.view(np.uint32)).sum()))
        for which in range(kk):
            gref = R.merge_bwd(mode, dy, xs[:kk], which)
            assert np.isfinite(gref).all(), (mode, which)
            out = Guarded((n,), None, pad)
            if mode in ('mul', 'max', 'min'):
                ops.merge_bwd(mode, gdy.t, [g.t for g in gx[:kk]], which, out=out.t)
            elif mode == 'add' or (mode == 'sub' and which == 0):
                continue                                                   # dx = dy: no kernel, the layer hands dy on
            else:
                ops.scale(gdy.t, -1.0 if mode == 'sub' else float(np.float32(1.0) / np.float32(kk)), out=out.t)
            g = out.check('%s backward %d' % (mode, which))
            assert same_bits(g, gref), (mode, 'backward', which, int((g.view(np.uint32) != gref.view(np.uint32)).sum()))


def test_the_same_tensor_twice_and_a_second_run():
    """Multiply()([x, x]) hands one address twice; two runs give identical bits."""
    from gennet_amd import ops
    rng = np.random.RandomState(5)
    x = rng.randn(1030).astype(np.float32)
    dy = rng.randn(1030).astype(np.float32)
    gx, gdy = Guarded((1030,), x, 36), Guarded((1030,), dy, 36)
    for mode in ('mul', 'add', 'max'):
        a = ops.merge_fwd(mode, [gx.t, gx.t]).cpu().numpy()
        assert same_bits(a, R.merge_fwd(mode, [x, x])) and same_bits(a, ops.merge_fwd(mode, [gx.t, gx.t]).cpu().numpy())
    for which in (0, 1):
        assert same_bits(ops.merge_bwd('mul', gdy.t, [gx.t, gx.t], which).cpu().numpy(), R.merge_bwd('mul', dy, [x, x], which))
        assert same_bits(ops.merge_bwd('max', gdy.t, [gx.t, gx.t], which).cpu().numpy(), dy if which == 0 else np.zeros_like(dy))


CONCAT = [([(4, 16, 1), (4, 16, 1)], -1),                                  # widths 1 + 1: the reference's two-channel discriminator input
          ([(3, 5, 4), (3, 5, 8)], -1),                                    # float4
          ([(3, 5, 4), (3, 7, 4)], 1),                                     # inner = 4: widths 20 + 28
          ([(2, 3, 6), (2, 3, 3), (2, 3, 1)], -1),                         # scalar, three inputs
          ([(2, 3, w) for w in (4, 8, 4, 4, 12, 4, 8, 4)], 2),             # eight inputs, float4
          ([(2, 3, w) for w in (1, 2, 3, 1, 5, 1, 2, 4)], -1),             # eight inputs, scalar
          ([(1030, 256), (1030, 255)], 1),                                 # 526330 scalar units: a second trip
          ([(1030, 1024), (1030, 1028)], -1)]                              # 528390 float4 units: a second trip


@pytest.mark.parametrize('pad', [37, 36])
@pytest.mark.parametrize('shapes,axis', CONCAT, ids=['+'.join('x'.join(map(str, s)) for s in c[0][:3]) + ('+..' if len(c[0]) > 3 else '') + '-axis%d' % c[1]
                                                     for c in CONCAT])
def test_concatenate_passes_are_bit_identical_to_the_reference(shapes, axis, pad):
    from gennet_amd import ops
    rng = np.random.RandomState(len(shapes) * 100 + pad)
    xs = [rng.randn(*s).astype(np.float32) for s in shapes]
    ref = R.concat_fwd(xs, axis)
    ax = axis if axis >= 0 else len(shapes[0]) + axis
    gx = [Guarded(s, x, pad) for s, x in zip(shapes, xs)]
    out = Guarded(ref.shape, None, pad)
    ops.concat_fwd([g.t for g in gx], ax, out=out.t)
    assert same_bits(out.check('concat forward'), ref)
    dy = rng.randn(*ref.shape).astype(np.float32)
    gdy = Guarded(ref.shape, dy, pad)
    douts = [Guarded(s, None, pad) for s in shapes]
    ops.concat_bwd(gdy.t, shapes, ax, outs=[g.t for g in douts])
    for g, r in zip(douts, R.concat_bwd(dy, shapes, axis)):
        assert same_bits(g.check('concat backward'), r)
    # one dx not wanted: its buffer stays at the sentinel, the others are written as before
    skip = len(shapes) // 2
    douts = [Guarded(s, None, pad) for s in shapes]
    got = ops.concat_bwd(gdy.t, shapes, ax, outs=[None if j == skip else g.t for j, g in enumerate(douts)])
    assert got[skip] is None and douts[skip].untouched()
    for j, (g, r) in enumerate(zip(douts, R.concat_bwd(dy, shapes, axis))):
        if j != skip:
            assert same_bits(g.check('concat backward without input %d' % skip), r)
    assert ops.concat_bwd(gdy.t, shapes, ax, wanted=[j == 0 for j in range(len(shapes))])[1] is None


def test_bad_arguments_are_errors_and_launch_nothing():
    from gennet_amd import _lib, ops
    n = 64
    x = [Guarded((n,), np.ones(n, np.float32), 36) for _ in range(9)]
    dy = Guarded((n,), np.ones(n, np.float32), 36)
    out = Guarded((n,), None, 36)
    s = torch.cuda.current_stream().cuda_stream
    tab = (ctypes.c_void_p * 9)(*[g.t.data_ptr() for g in x])
    holed = (ctypes.c_void_p * 9)(*[None if j == 1 else g.t.data_ptr() for j, g in enumerate(x)])
    w3, wbad = (ctypes.c_int * 3)(16, 16, 32), (ctypes.c_int * 3)(16, 0, 48)

    def refused(text, fn):
        with pytest.raises(_lib.GennetHipError) as e:
            fn()
        assert text in str(e.value), str(e.value)
        torch.cuda.synchronize()
        assert out.untouched()

    refused('null pointer', lambda: _lib.call('gn_merge_fwd', 0, None, 2, out.t.data_ptr(), n, s))
    refused('null pointer', lambda: _lib.call('gn_merge_fwd', 0, tab, 2, None, n, s))
    refused('input 1 is a null pointer', lambda: _lib.call('gn_merge_fwd', 0, holed, 2, out.t.data_ptr(), n, s))
    refused('0 inputs', lambda: _lib.call('gn_merge_fwd', 0, tab, 0, out.t.data_ptr(), n, s))
    refused('9 inputs', lambda: _lib.call('gn_merge_fwd', 0, tab, 9, out.t.data_ptr(), n, s))
    refused('exactly 2 inputs', lambda: _lib.call('gn_merge_fwd', ops.MERGE_MODES['sub'], tab, 3, out.t.data_ptr(), n, s))
    refused('unknown mode 6', lambda: _lib.call('gn_merge_fwd', 6, tab, 2, out.t.data_ptr(), n, s))
    refused('unknown mode -1', lambda: _lib.call('gn_merge_bwd', -1, dy.t.data_ptr(), tab, 2, 0, out.t.data_ptr(), n, s))
    refused('has no kernel', lambda: _lib.call('gn_merge_bwd', ops.MERGE_MODES['add'], dy.t.data_ptr(), tab, 2, 0, out.t.data_ptr(), n, s))
    refused('input 2 of 2', lambda: _lib.call('gn_merge_bwd', ops.MERGE_MODES['mul'], dy.t.data_ptr(), tab, 2, 2, out.t.data_ptr(), n, s))
    refused('input -1 of 2', lambda: _lib.call('gn_merge_bwd', ops.MERGE_MODES['max'], dy.t.data_ptr(), tab, 2, -1, out.t.data_ptr(), n, s))
    refused('null pointer', lambda: _lib.call('gn_merge_bwd', ops.MERGE_MODES['max'], None, tab, 2, 0, out.t.data_ptr(), n, s))
    refused('9 inputs', lambda: _lib.call('gn_merge_bwd', ops.MERGE_MODES['min'], dy.t.data_ptr(), tab, 9, 0, out.t.data_ptr(), n, s))
    refused('null pointer', lambda: _lib.call('gn_scale', None, 2.0, out.t.data_ptr(), n, s))
    refused('out of place', lambda: _lib.call('gn_scale', out.t.data_ptr(), 2.0, out.t.data_ptr(), n, s))
    refused('width 0 of input 1', lambda: _lib.call('gn_concat_fwd', tab, wbad, 3, out.t.data_ptr(), 1, s))
    refused('width 0 of input 1', lambda: _lib.call('gn_concat_bwd', out.t.data_ptr(), tab, wbad, 3, 1, s))
    refused('9 inputs', lambda: _lib.call('gn_concat_fwd', tab, w3, 9, out.t.data_ptr(), 1, s))
    refused('0 inputs', lambda: _lib.call('gn_concat_bwd', out.t.data_ptr(), tab, w3, 0, 1, s))
    refused('input 1 is a null pointer', lambda: _lib.call('gn_concat_fwd', holed, w3, 3, out.t.data_ptr(), 1, s))
    refused('null pointer', lambda: _lib.call('gn_concat_fwd', tab, None, 3, out.t.data_ptr(), 1, s))
    refused('null pointer', lambda: _lib.call('gn_concat_bwd', None, tab, w3, 3, 1, s))
    with pytest.raises(ValueError, match='GN_MERGE_MAX_INPUTS'):
        ops.merge_fwd('add', [g.t for g in x])
    # nothing to do is not an error, and launches nothing
    _lib.call('gn_merge_fwd', 0, tab, 2, out.t.data_ptr(), 0, s)
    _lib.call('gn_merge_bwd', ops.MERGE_MODES['mul'], dy.t.data_ptr(), tab, 2, 0, out.t.data_ptr(), 0, s)
    _lib.call('gn_scale', dy.t.data_ptr(), 2.0, out.t.data_ptr(), 0, s)
    _lib.call('gn_concat_fwd', tab, w3, 3, out.t.data_ptr(), 0, s)
    torch.cuda.synchronize()
    assert out.untouched()


# ---------------------------------------------------------------------------------------------------------------------
# section 2: models against torch fp64 autograd
# ---------------------------------------------------------------------------------------------------------------------
LR = 0.05


def rel(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-30)


def seed_biases(model, rng):
    for l in model.layers:
        ws = l.get_weights()
        if len(ws) == 2:
            l.set_weights([ws[0], (0.1 * rng.randn(*ws[1].shape)).astype(np.float32)])


def torch_params(layers):
    return dict((l.name, [torch.tensor(w.astype(np.float64), requires_grad=True) for w in l.get_weights()]) for l in layers if l.weights)


def conv1d_same(x, w, b):
    """keras Conv1D(padding='same', stride 1) on channels-last x (B, L, Cin), kernel (k, Cin, Cout), odd k"""
    return F.conv1d(x.permute(0, 2, 1), w.permute(2, 1, 0), padding=w.shape[0] // 2).permute(0, 2, 1) + b


def train_and_compare(model, ref_forward, xs, t, loss='mean_squared_error', what=''):
    """predict, then one SGD train_on_batch, against torch fp64: the bounds of tests/test_bn_axis_gpu.py's model tests"""
    from gennet_amd.engine import SGD
    model.compile(optimizer=SGD(lr=LR), loss=loss)
    layers = [l for l in model.layers if l.weights]
    P = torch_params(layers)
    xt = [torch.tensor(x.astype(np.float64)) for x in xs]
    tt = torch.tensor(t.astype(np.float64))
    feed = xs if len(xs) > 1 else xs[0]
    y = model.predict(feed, batch_size=len(t))
    with torch.no_grad():
        y_ref = ref_forward(P, *xt).numpy()
    print(what, 'predict err %.3g' % rel(y, y_ref))
    assert rel(y, y_ref) < 1e-5
    out = ref_forward(P, *xt)
    loss_ref = ((out - tt) ** 2).mean() if loss == 'mean_squared_error' else F.binary_cross_entropy(out, tt)
    loss_ref.backward()
    res = model.train_on_batch(feed, t)
    print(what, 'loss', res[0], float(loss_ref.detach()))
    assert abs(res[0] - float(loss_ref.detach())) <= 1e-6 * abs(float(loss_ref.detach()))
    g_floor = 1e-3 * max(float(v.grad.abs().max()) for ts in P.values() for v in ts)
    for l in layers:
        for p, ref in zip(l.params, P[l.name]):
            g_ref = ref.grad.numpy()
            gerr = np.abs(p.grad.detach().cpu().numpy().reshape(g_ref.shape) - g_ref).max() / max(np.abs(g_ref).max(), g_floor)
            w_ref = (ref.detach() - LR * ref.grad).numpy()
            werr = np.abs(p.numpy().astype(np.float64) - w_ref).max() / max(np.abs(w_ref).max(), 1e-3)
            print(what, l.name, p.name, 'grad err %.3g weight err %.3g' % (gerr, werr))
            assert gerr < 1e-4 and werr < 1e-4, (l.name, p.name, gerr, werr)
    return P


def residual_model():
    from gennet_amd import layers as Ly
    from gennet_amd.engine import Input, Model
    x0 = Input((5,))
    d_in, d_mid, d_out = Ly.Dense(8, activation='tanh'), Ly.Dense(8), Ly.Dense(1)
    h = d_in(x0)
    model = Model(inputs=x0, outputs=d_out(Ly.Add()([d_mid(h), h])))
    return model, (d_in, d_mid, d_out)


def test_residual_block_sums_the_gradient_of_a_tensor_that_feeds_a_layer_and_the_merge():
    """h = Dense(8, 'tanh')(x0); y = Add()([Dense(8)(h), h]); Dense(1) head.  Add hands ONE dy to both its inputs, and h's entry is that very
    tensor when the inner Dense's gradient arrives to be summed into it: the aliasing case.  The summed gradient at h (the input side of the
    block) is read off the first Dense's kernel and bias gradients, dL/dh through tanh'."""
    model, (d_in, d_mid, d_out) = residual_model()
    rng = np.random.RandomState(3)
    seed_biases(model, rng)
    assert [n.inbound for n in model.nodes] == [[-1], [0], [1, 0], [2]]

    def ref(P, x):
        h = torch.tanh(x @ P[d_in.name][0] + P[d_in.name][1])
        return ((h @ P[d_mid.name][0] + P[d_mid.name][1]) + h) @ P[d_out.name][0] + P[d_out.name][1]
    train_and_compare(model, ref, [rng.randn(6, 5).astype(np.float32)], rng.randn(6, 1).astype(np.float32), what='residual')


def test_residual_block_with_epilogues_that_overwrite_their_gradient():
    """Add()([Dense(8, 'tanh')(h), Dense(8, 'relu')(h), h]): both Dense layers run their activation backward IN PLACE on the dy they are handed,
    and all three inputs are handed the same one."""
    from gennet_amd import layers as Ly
    from gennet_amd.engine import Input, Model
    x0 = Input((5,))
    d_in, d_a, d_b, d_out = Ly.Dense(8, activation='tanh'), Ly.Dense(8, activation='tanh'), Ly.Dense(8, activation='relu'), Ly.Dense(1)
    h = d_in(x0)
    model = Model(inputs=x0, outputs=d_out(Ly.Add()([d_a(h), d_b(h), h])))
    rng = np.random.RandomState(4)
    seed_biases(model, rng)

    def ref(P, x):
        h = torch.tanh(x @ P[d_in.name][0] + P[d_in.name][1])
        a = torch.tanh(h @ P[d_a.name][0] + P[d_a.name][1])
        b = torch.relu(h @ P[d_b.name][0] + P[d_b.name][1])
        return ((a + b) + h) @ P[d_out.name][0] + P[d_out.name][1]
    train_and_compare(model, ref, [rng.randn(6, 5).astype(np.float32)], rng.randn(6, 1).astype(np.float32), what='residual, in-place epilogues')


def test_the_same_tensor_on_two_edges():
    """Multiply()([t, t]) and Add()([t, t]) on a Dense output: inbound [i, i], both gradients are summed."""
    from gennet_amd import layers as Ly
    from gennet_amd.engine import Input, Model
    x0 = Input((5,))
    d_in, d_out = Ly.Dense(4), Ly.Dense(1)
    t = d_in(x0)
    model = Model(inputs=x0, outputs=d_out(Ly.Add()([Ly.Multiply()([t, t]), Ly.Add()([t, t])])))
    assert [n.inbound for n in model.nodes] == [[-1], [0, 0], [0, 0], [1, 2], [3]]
    rng = np.random.RandomState(5)
    seed_biases(model, rng)

    def ref(P, x):
        t = x @ P[d_in.name][0] + P[d_in.name][1]
        return (t * t + (t + t)) @ P[d_out.name][0] + P[d_out.name][1]
    train_and_compare(model, ref, [rng.randn(6, 5).astype(np.float32)], rng.randn(6, 1).astype(np.float32), what='squaring')


def test_a_gradient_two_edges_hold_is_not_accumulated_into():
    """y = Dense_y(x), u = Dense_u(x); out = Dense(Concatenate([Dense_z(y), Dense_w(u), Add()([u, y])])).  Nodes: y 0, z 1, u 2, w 3, Add 4.  In the
    reverse sweep Add stores ONE dy for u and for y; then w's data gradient arrives for u while y's entry (the same memory) is still waiting
    for z's: a sum written in place into u's entry would reach y as well."""
    from gennet_amd import layers as Ly
    from gennet_amd.engine import Input, Model
    x0 = Input((5,))
    d_y, d_u, d_z, d_w, d_out = Ly.Dense(4, activation='tanh'), Ly.Dense(4, activation='tanh'), Ly.Dense(3), Ly.Dense(3), Ly.Dense(1)
    y, u = d_y(x0), d_u(x0)
    model = Model(inputs=x0, outputs=d_out(Ly.Concatenate()([d_z(y), d_w(u), Ly.Add()([u, y])])))
    assert [n.layer for n in model.nodes[:4]] == [d_y, d_z, d_u, d_w] and model.nodes[4].inbound == [2, 0]
    rng = np.random.RandomState(10)
    seed_biases(model, rng)

    def ref(P, x):
        y = torch.tanh(x @ P[d_y.name][0] + P[d_y.name][1])
        u = torch.tanh(x @ P[d_u.name][0] + P[d_u.name][1])
        j = torch.cat([y @ P[d_z.name][0] + P[d_z.name][1], u @ P[d_w.name][0] + P[d_w.name][1], u + y], dim=1)
        return j @ P[d_out.name][0] + P[d_out.name][1]
    train_and_compare(model, ref, [rng.randn(6, 5).astype(np.float32)], rng.randn(6, 1).astype(np.float32), what='fan')


def stacked_model(L=16):
    """bbhMahoGANy.py:1268-1272 as layers: [g, event - g] side by side, then a small discriminator"""
    from gennet_amd import layers as Ly
    from gennet_amd.engine import Input, Model
    z_in, event_in = Input((L, 4), name='z_in'), Input((L, 1), name='event_in')
    g_conv, d_conv, d_out = Ly.Conv1D(1, 5, padding='same'), Ly.Conv1D(4, 3, padding='same', activation='tanh'), Ly.Dense(1, activation='sigmoid')
    g = g_conv(z_in)
    cat = Ly.Concatenate(axis=-1)
    stacked = cat([g, Ly.Subtract()([event_in, g])])
    model = Model(inputs=[z_in, event_in], outputs=d_out(Ly.Flatten()(d_conv(stacked))))
    return model, (g_conv, d_conv, d_out), cat


def stacked_ref(layers):
    g_conv, d_conv, d_out = layers

    def ref(P, z, ev):
        g = conv1d_same(z, *P[g_conv.name])
        h = torch.tanh(conv1d_same(torch.cat([g, ev - g], dim=2), *P[d_conv.name]))
        return torch.sigmoid(h.reshape(h.shape[0], -1) @ P[d_out.name][0] + P[d_out.name][1])
    return ref


def stacked_data(rng, B=6, L=16):
    z = rng.randn(B, L, 4).astype(np.float32)
    event = np.tile(rng.randn(1, L, 1).astype(np.float32), (B, 1, 1))      # the measured event: the same for every row, MyLayer's constant
    t = (rng.rand(B, 1) > 0.5).astype(np.float32)
    return z, event, t


def test_subtract_and_concatenate_build_the_references_two_channel_input():
    from gennet_amd import ops
    from gennet_amd.engine import SGD
    model, layers, cat = stacked_model()
    rng = np.random.RandomState(6)
    seed_biases(model, rng)
    z, event, t = stacked_data(rng)
    assert [type(n.layer).__name__ for n in model.nodes] == ['Conv1D', 'Subtract', 'Concatenate', 'Conv1D', 'Flatten', 'Dense']
    assert model.nodes[1].inbound == [-2, 0] and model.nodes[2].inbound == [0, 1] and model.nodes[2].out_shape == (16, 2)
    train_and_compare(model, stacked_ref(layers), [z, event], t, loss='binary_crossentropy', what='stacked')
    # the (B, L, 2) intermediate is MyLayer's stack: x beside event - x, bit for bit
    model.compile(optimizer=SGD(lr=LR), loss='binary_crossentropy')
    cap = {}
    model.train_on_batch([z, event], t, capture=cap)
    g = cap[layers[0].name]
    assert tuple(cap[cat.name].shape) == (6, 16, 2)
    mine = ops.subtract_stack_fwd(g.reshape(6, 16).contiguous(), torch.tensor(event[0, :, 0], device=dev()))
    assert torch.equal(cap[cat.name], mine.reshape(6, 16, 2))


def test_maximum_minimum_and_average_of_three_branches_joined_by_concatenate():
    from gennet_amd import layers as Ly
    from gennet_amd.engine import Input, Model
    x0 = Input((5,))
    br = [Ly.Dense(4, activation='tanh'), Ly.Dense(4), Ly.Dense(4, activation='relu')]
    d_out = Ly.Dense(1)
    ts = [b(x0) for b in br]
    joined = Ly.Concatenate()([Ly.Maximum()(ts), Ly.Minimum()(ts), Ly.Average()(ts)])
    model = Model(inputs=x0, outputs=d_out(joined))
    assert model.nodes[6].out_shape == (12,)
    rng = np.random.RandomState(7)
    seed_biases(model, rng)

    def ref(P, x):
        a = torch.tanh(x @ P[br[0].name][0] + P[br[0].name][1])
        b = x @ P[br[1].name][0] + P[br[1].name][1]
        c = torch.relu(x @ P[br[2].name][0] + P[br[2].name][1])
        assert not ((a == b) | (b == c) | (a == c)).any()                   # no ties: torch.maximum would split their gradient
        j = torch.cat([torch.maximum(torch.maximum(a, b), c), torch.minimum(torch.minimum(a, b), c), ((a + b) + c) / 3], dim=1)
        return j @ P[d_out.name][0] + P[d_out.name][1]
    train_and_compare(model, ref, [rng.randn(6, 5).astype(np.float32)], rng.randn(6, 1).astype(np.float32), what='max / min / avg')


def test_save_and_load_round_trip(tmp_path):
    from gennet_amd.engine import SGD, load_model
    model, layers, _ = stacked_model()
    rng = np.random.RandomState(8)
    seed_biases(model, rng)
    z, event, t = stacked_data(rng)
    model.compile(optimizer=SGD(lr=LR), loss='binary_crossentropy')
    model.train_on_batch([z, event], t)
    path = os.path.join(str(tmp_path), 'stacked.h5')
    model.save(path)
    again = load_model(path)
    assert [type(n.layer).__name__ for n in again.nodes] == [type(n.layer).__name__ for n in model.nodes]
    assert [n.inbound for n in again.nodes] == [n.inbound for n in model.nodes]
    assert np.array_equal(model.predict([z, event]), again.predict([z, event]))
    a, b = model.train_on_batch([z, event], t), again.train_on_batch([z, event], t)
    assert a == b and all(np.array_equal(u, v) for u, v in zip(model.get_weights(), again.get_weights()))


def test_a_captured_step_of_the_residual_block_replays_bit_identically():
    """model (a) as a hipGraph (engine.StepGraph): eager step, capture, three replays against four eager steps of a twin"""
    from gennet_amd import engine
    from gennet_amd.engine import SGD, to_device
    rng = np.random.RandomState(9)
    x, t = to_device(rng.randn(6, 5).astype(np.float32)), to_device(rng.randn(6, 1).astype(np.float32))
    eager, _ = residual_model()
    seed_biases(eager, rng)
    graphed, _ = residual_model()
    graphed.set_weights(eager.get_weights())
    for m in (eager, graphed):
        m.compile(optimizer=SGD(lr=LR, momentum=0.5), loss='mean_squared_error')
    want = []
    for _ in range(4):
        want.append((eager.train_on_batch_device([x], [t]).cpu().numpy().copy(), [w.copy() for w in eager.get_weights()]))
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
    assert not np.array_equal(want[0][0], want[3][0])                      # the steps differ: a replay that did nothing would show
