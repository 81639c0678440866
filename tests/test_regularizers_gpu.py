"""GPU tests of the Keras weight and activity regularizers.

Section 1.  The passes of csrc/regularizer.hip alone, through ops.reg_pass / reg_grad / reg_finish, against tests/regularizer_ref.py.  Inputs sit in
NaN-surrounded buffers, outputs in sentinel-filled ones; a view starts 36 floats in (16-byte aligned: float4 units), 37 floats in (a scalar head,
the float4 body, a scalar tail), or x and g differ (scalar units).  The grid is stream_grid(ceil(n / 4)), capped at 2048 blocks of 256 lanes: 2^21 + 5
floats are 2^19 + 1 float4 units, a second trip of the grid-stride loop for one lane (and for every lane on the scalar path).
  gradient  against the fp64 g + l1 sign(x) + 2 l2 x on the fp32 inputs and fp32 coefficients, every element within 4 * 2^-24 * (|g| + l1 + 2 l2 |x|):
            three fp32 roundings (the product, the inner sum, the outer sum) and one to spare; exactly g where x == +-0.
  penalty   against math.fsum of the fp64 terms, relative error <= 2^-23: the one final fp32 rounding (2^-24) with as much again to spare for the
            fp64 accumulation, which is below n * 2^-53 < 2^-31 relative at these sizes (all terms are >= 0: nothing cancels).
Section 2.  One regularized layer through train_on_batch with SGD(lr=0.05) against torch fp64 autograd of loss + penalties, three steps, the reference
starting each step from the weights the GPU holds.  Bounds: those tests/test_dilated_gpu.py section 4 and tests/test_merge_gpu.py use for single
steps -- the loss 1e-6 relative, every updated tensor within 1e-4 of its largest reference entry (floor 1e-3).  The penalty is more than 1 % of the
loss in every case, so a dropped penalty cannot pass; the same layer without the keywords gives another loss and other weights.
Section 3.  Models: the test phase, a frozen layer, D(G(z)) with D frozen, two outputs with loss_weights, clipnorm, save / load, a captured step,
an unregularized model, and two ranks against one."""
import os
import pickle
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import regularizer_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -12345.5
LR = 0.05


def dev():
    return torch.device('cuda:0')


class Guarded(object):
    """A contiguous view `pad` elements into a larger flat buffer.  value given: an input, surrounded by NaN.  init given: an in / out tensor, and
    none of both an output, inside a buffer of sentinels."""

    def __init__(self, n, value=None, pad=37, init=None, dtype=torch.float32):
        self.n, self.pad, self.edge = int(n), pad, float('nan') if value is not None else SENTINEL
        self.buf = torch.full((self.n + 2 * pad,), self.edge, dtype=dtype, device=dev())
        self.t = self.buf[pad:pad + self.n]
        start = value if value is not None else init
        if start is not None:
            self.t.copy_(torch.tensor(np.ascontiguousarray(start), dtype=dtype, device=dev()))
        assert self.t.is_contiguous() and self.t.data_ptr() == self.buf.data_ptr() + self.buf.element_size() * pad

    def check(self, what, written=True):
        """the surroundings untouched and (an output) every element of the view written"""
        edges = torch.cat([self.buf[:self.pad], self.buf[self.pad + self.n:]])
        assert bool((edges == SENTINEL).all()), '%s: wrote outside its output' % what
        if written:
            assert not bool((self.t == SENTINEL).any()), '%s: output elements left unwritten' % what
        assert not bool(torch.isnan(self.t).any()), '%s: NaN (an element outside an input was read)' % what
        return self.t.cpu().numpy()

    def untouched(self):
        return bool((self.buf == SENTINEL).all())


def first_entry(res):
    return float(np.ravel(res)[0])


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


# ---------------------------------------------------------------------------------------------------------------------
# section 1: the passes
# ---------------------------------------------------------------------------------------------------------------------
NS = [1, 3, 4, 5, 255, 256, 257, 1027, (1 << 21) + 5]
LAMS = [(0.01, 0.0), (0.0, 0.01), (0.001, 0.02)]
PADS = [(36, 36), (37, 37), (36, 37)]
_INPUTS = {}


def pass_input(n):
    """(x, g, {(l1, l2): (fsum penalty, gradient reference, gradient bound)}) of size n: computed once, shared by the three alignments"""
    if n not in _INPUTS:
        rng = np.random.RandomState(n % 9973)
        x = rng.randn(n).astype(np.float32)
        x[rng.rand(n) < 0.1] = 0.0
        x[rng.rand(n) < 0.1] = -0.0
        if n >= 3:
            x[0], x[1], x[2] = 0.0, -0.0, -1.5
        else:
            x[0] = -0.75
        g = rng.randn(n).astype(np.float32)
        _INPUTS[n] = (x, g, dict((lam, (R.penalty(x, *lam),) + R.grad(g, x, *lam)) for lam in LAMS))
    return _INPUTS[n]


def test_the_grid_cap_is_where_the_second_trip_case_puts_it():
    from gennet_amd import ops
    assert ops.reg_partials(1 << 21) == 2048 == ops.reg_partials((1 << 21) + 5)       # 2048 blocks x 256 lanes x 4 floats = 2^21
    assert ops.reg_partials((1 << 21) - 1024) == 2047
    assert ((1 << 21) + 5) // 4 == 2048 * 256 + 1                                     # aligned: one float4 unit past one trip, and a tail of one


@pytest.mark.parametrize('pads', PADS, ids=['aligned', 'offset-one-float', 'mixed'])
@pytest.mark.parametrize('n', NS)
def test_penalty_and_gradient_in_one_pass(n, pads):
    from gennet_amd import ops
    x, g0, refs = pass_input(n)
    k = ops.reg_partials(n)
    gx = Guarded(n, x, pads[0])
    zero = x == 0
    for lam in LAMS:
        pen_ref, g_ref, g_bound = refs[lam]
        runs = []
        for _ in range(2):
            gg, parts, out = Guarded(n, None, pads[1], init=g0), Guarded(k, None, 3, dtype=torch.float64), Guarded(1, None, 2)
            ops.reg_pass(gx.t, gg.t, lam[0], lam[1], parts.t)
            ops.reg_finish(parts.t, out.t)
            runs.append((gg.check('reg_pass g', written=False), parts.check('reg_pass partials'), out.check('reg_finish')))
        got, p, pen = runs[0]
        err = np.abs(got.astype(np.float64) - g_ref)
        assert (err <= g_bound).all(), (n, lam, float((err / g_bound).max()))
        assert np.array_equal(bits(got[zero]), bits(g0[zero]))                     # sign(+-0) = 0 and 2 l2 (+-0) = +-0: g comes back as it was
        assert lam[0] == 0 or n < 3 or got[2] != g0[2]                             # ... and an element away from 0 did move
        assert (p >= 0).all()
        rel = abs(float(pen[0]) - pen_ref) / pen_ref
        print('n %d pads %s lam %s penalty %.9g reference %.17g rel %.3g' % (n, pads, lam, float(pen[0]), pen_ref, rel))
        assert rel <= 2.0 ** -23, (n, lam, rel)
        for a, b in zip(runs[0], runs[1]):                                        # two runs: the same bits
            assert np.array_equal(bits(a), bits(b))
        # the penalty alone (g == NULL): a sentinel-filled gradient buffer stays as it is, the penalty meets the same bound
        idle, parts, out = Guarded(n, None, pads[1]), Guarded(k, None, 3, dtype=torch.float64), Guarded(1, None, 2)
        ops.reg_pass(gx.t, None, lam[0], lam[1], parts.t)
        ops.reg_finish(parts.t, out.t)
        torch.cuda.synchronize()
        assert idle.untouched()
        parts.check('reg_pass partials (penalty only)')
        assert abs(float(out.check('reg_finish')[0]) - pen_ref) / pen_ref <= 2.0 ** -23


@pytest.mark.parametrize('pads', PADS + [(37, 36)], ids=['aligned', 'offset-one-float', 'mixed', 'mixed-the-other-way'])
@pytest.mark.parametrize('n', NS)
def test_the_gradient_only_entry_out_of_place_and_in_place(n, pads):
    from gennet_amd import ops
    y, g0, refs = pass_input(n)
    gy, gin = Guarded(n, y, pads[0]), Guarded(n, g0, pads[0])
    for lam in LAMS:
        _, g_ref, g_bound = refs[lam]
        out = Guarded(n, None, pads[1])
        assert ops.reg_grad(gy.t, gin.t, lam[0], lam[1]).data_ptr() != gin.t.data_ptr()      # a new tensor by default
        torch.cuda.synchronize()
        _lib_reg_grad(gy.t, gin.t, out.t, lam)
        got = out.check('reg_grad')                                                # every element written, nothing outside
        assert (np.abs(got.astype(np.float64) - g_ref) <= g_bound).all(), (n, lam)
        assert np.array_equal(bits(gin.t.cpu().numpy()), bits(g0))                 # out of place: the incoming gradient is left alone
        own = Guarded(n, None, pads[1], init=g0)
        assert ops.reg_grad(gy.t, own.t, lam[0], lam[1], inplace=True) is own.t
        assert np.array_equal(bits(own.check('reg_grad in place', written=False)), bits(got))      # element-wise: the same bits either way


def _lib_reg_grad(y, gin, gout, lam):
    from gennet_amd import _lib
    _lib.call('gn_reg_grad', y.data_ptr(), gin.data_ptr(), gout.data_ptr(), y.numel(), lam[0], lam[1], torch.cuda.current_stream().cuda_stream)


def test_bad_arguments_are_errors_and_launch_nothing():
    from gennet_amd import _lib, ops
    n = 1027
    x, g0, _ = pass_input(n)
    gx, out, parts, pen = Guarded(n, x, 36), Guarded(n, None, 36), Guarded(2, None, 2, dtype=torch.float64), Guarded(1, None, 2)
    s = torch.cuda.current_stream().cuda_stream
    px, po, pp, pf = gx.t.data_ptr(), out.t.data_ptr(), parts.t.data_ptr(), pen.t.data_ptr()
    nan = float('nan')

    def refused(text, fn):
        with pytest.raises(_lib.GennetHipError) as e:
            fn()
        assert text in str(e.value) and '(%d)' % _lib.GN_EINVAL in str(e.value), str(e.value)
        torch.cuda.synchronize()
        assert out.untouched() and parts.untouched() and pen.untouched()

    refused('reg_pass: null pointer', lambda: _lib.call('gn_reg_pass', None, po, n, 0.01, 0.0, pp, 2, s))
    refused('reg_pass: null pointer', lambda: _lib.call('gn_reg_pass', px, po, n, 0.01, 0.0, None, 2, s))
    refused('reg_pass: n == 0', lambda: _lib.call('gn_reg_pass', px, po, 0, 0.01, 0.0, pp, 2, s))
    refused('reg_pass: l1 -0.01', lambda: _lib.call('gn_reg_pass', px, po, n, -0.01, 0.0, pp, 2, s))
    refused('reg_pass: l1 0, l2 nan', lambda: _lib.call('gn_reg_pass', px, po, n, 0.0, nan, pp, 2, s))
    refused('reg_pass: a workspace of 1 partials for n = 1027, which writes 2', lambda: _lib.call('gn_reg_pass', px, po, n, 0.01, 0.0, pp, 1, s))
    refused('reg_grad: null pointer', lambda: _lib.call('gn_reg_grad', None, px, po, n, 0.01, 0.0, s))
    refused('reg_grad: null pointer', lambda: _lib.call('gn_reg_grad', px, None, po, n, 0.01, 0.0, s))
    refused('reg_grad: null pointer', lambda: _lib.call('gn_reg_grad', px, px, None, n, 0.01, 0.0, s))
    refused('reg_grad: n == 0', lambda: _lib.call('gn_reg_grad', px, px, po, 0, 0.01, 0.0, s))
    refused('reg_grad: l1 0, l2 -0.01', lambda: _lib.call('gn_reg_grad', px, px, po, n, 0.0, -0.01, s))
    refused('reg_grad: l1 nan', lambda: _lib.call('gn_reg_grad', px, px, po, n, nan, 0.0, s))
    refused('reg_finish: null pointer', lambda: _lib.call('gn_reg_finish', None, 2, pf, s))
    refused('reg_finish: null pointer', lambda: _lib.call('gn_reg_finish', pp, 2, None, s))
    refused('reg_finish: no partials', lambda: _lib.call('gn_reg_finish', pp, 0, pf, s))
    with pytest.raises(ValueError):
        ops.reg_pass(gx.t, out.t[:5], 0.01, 0.0, parts.t)
    with pytest.raises(ValueError):
        ops.reg_grad(gx.t, out.t[:5], 0.01, 0.0)
    _lib.call('gn_reg_pass', px, None, n, 0.01, 0.0, pp, 2, s)                     # the same arguments inside the bounds run
    _lib.call('gn_reg_finish', pp, 2, pf, s)
    torch.cuda.synchronize()
    assert not parts.untouched() and not pen.untouched() and out.untouched()


# ---------------------------------------------------------------------------------------------------------------------
# section 2: one layer against torch fp64 autograd
# ---------------------------------------------------------------------------------------------------------------------
THREE = dict(kernel_regularizer=(0.01, 0.02), bias_regularizer=(0.0, 0.1), activity_regularizer=(0.001, 0.0))
LINE_220 = dict(activity_regularizer=(0.001, 0.0), kernel_regularizer=(0.0, 0.01))          # subtract_model.py:220 at small size


def _regs(spec):
    from gennet_amd.keras import regularizers
    return dict((k, regularizers.l1_l2(*v)) for k, v in spec.items())


def _kernel_case(fn, act, spec):
    def ref(P, x):
        y = fn(x, P[0], P[1], act)
        return y, R.t_penalty(P[0], spec.get('kernel_regularizer')) + R.t_penalty(P[1], spec.get('bias_regularizer')) + R.t_penalty(
            y, spec.get('activity_regularizer'))
    return ref


def _cases():
    from gennet_amd import layers as L
    bn = dict(gamma_regularizer=(0.0, 0.1), beta_regularizer=(0.01, 0.0))
    pr = dict(alpha_regularizer=(0.0, 0.1))
    return {
        'dense': ((4, 6), lambda kw: L.Dense(8, activation='tanh', input_shape=(6,), **kw), THREE, _kernel_case(R.dense, 'tanh', THREE)),
        'conv1d': ((2, 21, 4), lambda kw: L.Conv1D(8, 3, activation='tanh', input_shape=(21, 4), **kw), THREE, _kernel_case(R.conv1d, 'tanh', THREE)),
        'conv2d': ((2, 8, 2, 4), lambda kw: L.Conv2D(4, (5, 5), padding='same', activation='tanh', input_shape=(8, 2, 4), **kw), THREE,
                   _kernel_case(R.conv2d_same, 'tanh', THREE)),
        'conv2d_transpose': ((2, 1, 9, 8), lambda kw: L.Conv2DTranspose(4, (1, 4), input_shape=(1, 9, 8), **kw), LINE_220,
                             _kernel_case(R.conv2d_transpose, None, LINE_220)),
        'batchnorm': ((4, 5, 8), lambda kw: L.BatchNormalization(input_shape=(5, 8), **kw), bn,
                      lambda P, x: (R.batchnorm(x, P[0], P[1]), R.t_penalty(P[0], bn['gamma_regularizer']) + R.t_penalty(P[1], bn['beta_regularizer']))),
        'prelu': ((4, 8), lambda kw: L.PReLU(input_shape=(8,), **kw), pr, lambda P, x: (R.prelu(x, P[0]), R.t_penalty(P[0], pr['alpha_regularizer']))),
    }


def seeded(shapes, rng, around=0.0):
    """weights off their initial values, about a fifth of the entries exactly zero (of either sign)"""
    out = []
    for shp in shapes:
        w = (around + 0.5 * rng.randn(*shp)).astype(np.float32)
        z = rng.rand(*shp)
        w[z < 0.1], w[z > 0.9] = 0.0, -0.0
        w.reshape(-1)[0] = 0.0
        if w.size > 1:
            w.reshape(-1)[-1] = -0.0
        out.append(w)
    return out


def _model(make, kw, weights):
    from gennet_amd.engine import SGD, Sequential
    m = Sequential([make(kw)])
    layer = m.layers[0]
    layer.set_weights(list(weights) + layer.get_weights()[len(weights):])
    m.compile(optimizer=SGD(lr=LR), loss='mean_squared_error')
    return m, layer


@pytest.mark.parametrize('case', ['dense', 'conv1d', 'conv2d', 'conv2d_transpose', 'batchnorm', 'prelu'])
def test_one_regularized_layer_trains_like_torch_fp64(case):
    shape, make, spec, ref = _cases()[case]
    rng = np.random.RandomState(len(case) * 31 + shape[-1])
    from gennet_amd.engine import Sequential
    probe = Sequential([make({})]).layers[0]                                       # built: the shapes of its trained weights
    ntrain = len(probe.params)
    w0 = seeded([p.shape for p in probe.params], rng, 1.0 if case == 'batchnorm' else 0.0)
    m, layer = _model(make, _regs(spec), w0)
    plain, plain_layer = _model(make, {}, w0)
    x = rng.randn(*shape).astype(np.float32)
    out_shape = (shape[0],) + tuple(m.nodes[0].out_shape)
    t = rng.randn(*out_shape).astype(np.float32)
    assert np.array_equal(m.predict(x), plain.predict(x))                          # predict never sees a regularizer
    for step in range(3):
        held = layer.get_weights()[:ntrain]
        assert step > 0 or all((w == 0).any() for w in held)                          # exact zeros: sign(0) = 0 is exercised
        P = [R.t64(w, True) for w in held]
        y, pen = ref(P, R.t64(x))
        data = R.mse(y, R.t64(t))
        total = data + pen
        total.backward()
        loss = float(np.ravel(m.train_on_batch(x, t))[0])
        want, share = float(total.detach()), float(pen.detach()) / float(total.detach())
        print('%s step %d loss %.9g reference %.9g (penalty share %.3g)' % (case, step, loss, want, share))
        assert share > 0.01                                                        # a dropped penalty cannot pass
        assert abs(loss - want) <= 1e-6 * abs(want), (case, step, loss, want)
        for got, p in zip(layer.get_weights()[:ntrain], P):
            w_ref = (p.detach() - LR * p.grad).numpy()
            werr = np.abs(got.astype(np.float64) - w_ref).max() / max(np.abs(w_ref).max(), 1e-3)
            print('%s step %d %s weight err %.3g' % (case, step, tuple(got.shape), werr))
            assert werr < 1e-4, (case, step, got.shape, werr)
        if step == 0:
            # the same layer with the keywords removed: another loss and other weights (the regularizers are not accepted and ignored)
            loss_plain = float(np.ravel(plain.train_on_batch(x, t))[0])
            assert abs(loss_plain - float(data.detach())) <= 1e-6 * abs(float(data.detach()))
            assert abs(loss - loss_plain) > 0.01 * abs(loss)
            assert any(np.abs(a - b).max() > 1e-4 for a, b in zip(layer.get_weights()[:ntrain], plain_layer.get_weights()[:ntrain]))


# ---------------------------------------------------------------------------------------------------------------------
# section 3: models
# ---------------------------------------------------------------------------------------------------------------------
def dense_net(regs=True, trainable=True, optimizer=None, seed=5):
    """(4, 6) -> Dense(8, tanh; the three regularizers) -> Dense(3): (model, the two layers, x, t)"""
    from gennet_amd import layers as L
    from gennet_amd.engine import SGD, Sequential
    rng = np.random.RandomState(seed)
    first = L.Dense(8, activation='tanh', input_shape=(6,), trainable=trainable, **(_regs(THREE) if regs else {}))
    head = L.Dense(3)
    m = Sequential([first, head])
    first.set_weights(seeded([(6, 8), (8,)], rng))
    head.set_weights(seeded([(8, 3), (3,)], rng))
    m.compile(optimizer=optimizer or SGD(lr=LR), loss='mean_squared_error')
    return m, first, head, rng.randn(4, 6).astype(np.float32), rng.randn(4, 3).astype(np.float32)


def dense_net_ref(first, head, x, t, rows=slice(None)):
    """torch fp64 loss and penalty of dense_net at the weights the layers hold: (P, data loss, penalty)"""
    P = [R.t64(w, True) for w in first.get_weights() + head.get_weights()]
    h = R.dense(R.t64(x[rows]), P[0], P[1], 'tanh')
    pen = R.t_penalty(P[0], THREE['kernel_regularizer']) + R.t_penalty(P[1], THREE['bias_regularizer']) + R.t_penalty(h, THREE['activity_regularizer'])
    return P, R.mse(R.dense(h, P[2], P[3]), R.t64(t[rows])), pen


def test_the_test_phase_adds_the_penalties_and_predict_does_not():
    m, first, head, x, t = dense_net()
    plain = dense_net(regs=False)[0]
    _, data, pen = dense_net_ref(first, head, x, t)
    want = float((data + pen).detach())
    got = first_entry(m.test_on_batch(x, t))
    assert float(pen.detach()) > 0.01 * want and abs(got - want) <= 1e-6 * want, (got, want)
    assert abs(first_entry(plain.test_on_batch(x, t)) - float(data.detach())) <= 1e-6 * float(data.detach())
    # evaluate: the mean of test_on_batch over the chunks, weighted by their rows; every chunk carries the weight penalties and its own rows' activity
    chunks = [dense_net_ref(first, head, x, t, slice(s, s + 3)) for s in (0, 3)]
    want_ev = sum(float((d + p).detach()) * nb for (_, d, p), nb in zip(chunks, (3, 1))) / 4.0
    got_ev = first_entry(m.evaluate(x, t, batch_size=3))
    assert abs(got_ev - want_ev) <= 1e-6 * want_ev, (got_ev, want_ev)
    assert np.array_equal(m.predict(x), plain.predict(x)) and np.array_equal(m.predict_on_batch(x), plain.predict_on_batch(x))
    before = [w.copy() for w in m.get_weights()]
    m.test_on_batch(x, t)
    assert all(np.array_equal(a, b) for a, b in zip(before, m.get_weights()))      # the test phase adds no gradient term to anything


def test_a_frozen_layers_penalty_counts_and_its_weights_stay():
    m, first, head, x, t = dense_net(trainable=False)
    assert [trained for _, trained in m._reg_params] == [False, False]
    P, data, pen = dense_net_ref(first, head, x, t)
    (data + pen).backward()
    frozen = [w.copy() for w in first.get_weights()]
    loss = first_entry(m.train_on_batch(x, t))
    want = float((data + pen).detach())
    assert float(pen.detach()) > 0.01 * want and abs(loss - want) <= 1e-6 * want, (loss, want)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(frozen, first.get_weights()))
    for got, p in zip(head.get_weights(), P[2:]):
        w_ref = (p.detach() - LR * p.grad).numpy()
        assert np.abs(got - w_ref).max() / max(np.abs(w_ref).max(), 1e-3) < 1e-4
    assert any(not np.array_equal(a, p.detach().numpy().astype(np.float32)) for a, p in zip(head.get_weights(), P[2:]))


def test_a_frozen_discriminators_penalty_is_in_the_composite_models_loss():
    from gennet_amd import layers as L
    from gennet_amd.engine import SGD, Sequential
    from gennet_amd.keras.regularizers import l2
    rng = np.random.RandomState(8)
    g_layer = L.Dense(8, activation='tanh', input_shape=(4,))
    d_layer = L.Dense(1, activation='sigmoid', input_shape=(8,), kernel_regularizer=l2(0.1))
    G, D = Sequential([g_layer]), Sequential([d_layer])
    g_layer.set_weights(seeded([(4, 8), (8,)], rng))
    d_layer.set_weights(seeded([(8, 1), (1,)], rng))
    D.compile(optimizer=SGD(lr=LR), loss='binary_crossentropy')
    D.trainable = False
    GAN = Sequential([G, D])
    GAN.compile(optimizer=SGD(lr=LR), loss='binary_crossentropy')
    assert [l.name for l in GAN.layers] == [g_layer.name, d_layer.name] and [(p.name, tr) for p, tr in GAN._reg_params] == [(d_layer.name + '/kernel', False)]
    z, ones = rng.randn(6, 4).astype(np.float32), np.ones((6, 1), np.float32)
    P = [R.t64(w, True) for w in g_layer.get_weights() + d_layer.get_weights()]
    p = R.dense(R.dense(R.t64(z), P[0], P[1], 'tanh'), P[2], P[3], 'sigmoid')
    data, pen = R.bce(p, R.t64(ones)), R.t_penalty(P[2], (0.0, 0.1))
    (data + pen).backward()
    d_before = [w.copy() for w in d_layer.get_weights()]
    loss = first_entry(GAN.train_on_batch(z, ones))
    want = float((data + pen).detach())
    assert float(pen.detach()) > 0.01 * want and abs(loss - want) <= 1e-6 * want, (loss, want)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(d_before, d_layer.get_weights()))
    for got, q in zip(g_layer.get_weights(), P[:2]):
        w_ref = (q.detach() - LR * q.grad).numpy()
        assert np.abs(got - w_ref).max() / max(np.abs(w_ref).max(), 1e-3) < 1e-4
    # D on its own trains its kernel with the penalty's gradient
    x, y = rng.randn(6, 8).astype(np.float32), rng.randint(0, 2, (6, 1)).astype(np.float32)
    Q = [R.t64(w, True) for w in d_layer.get_weights()]
    total = R.bce(R.dense(R.t64(x), Q[0], Q[1], 'sigmoid'), R.t64(y)) + R.t_penalty(Q[0], (0.0, 0.1))
    total.backward()
    loss = first_entry(D.train_on_batch(x, y))
    assert abs(loss - float(total.detach())) <= 1e-6 * float(total.detach())
    for got, q in zip(d_layer.get_weights(), Q):
        w_ref = (q.detach() - LR * q.grad).numpy()
        assert np.abs(got - w_ref).max() / max(np.abs(w_ref).max(), 1e-3) < 1e-4


def test_a_shared_gradient_is_not_overwritten_and_the_activity_regularization_layer_counts():
    """x -> Add([A(x), B(x)]) -> ActivityRegularization: Add hands ONE gradient tensor to both branches.  B, which regularizes its output, is
    reached first in the backward sweep while A's edge still holds that storage: B's term must go out of place, or A would train on it too."""
    from gennet_amd import layers as L
    from gennet_amd.engine import SGD, Input, Model
    from gennet_amd.keras.regularizers import l1_l2
    rng = np.random.RandomState(10)
    x = Input(shape=(6,))
    A, B, tail = L.Dense(8, activation='tanh'), L.Dense(8, activity_regularizer=l1_l2(0.01, 0.05)), L.ActivityRegularization(l2=0.02)
    m = Model(inputs=x, outputs=tail(L.Add()([A(x), B(x)])))
    assert [type(n.layer).__name__ for n in m.nodes] == ['Dense', 'Dense', 'Add', 'ActivityRegularization'] and m.nodes[1].layer is B
    for layer in (A, B):
        layer.set_weights(seeded([(6, 8), (8,)], rng))
    m.compile(optimizer=SGD(lr=LR), loss='mean_squared_error')
    assert [n.layer for n in m._reg_nodes] == [B, tail] and m._reg_params == []
    xs, t = rng.randn(4, 6).astype(np.float32), rng.randn(4, 8).astype(np.float32)
    for step in range(2):
        P = [R.t64(w, True) for w in A.get_weights() + B.get_weights()]
        hb = R.dense(R.t64(xs), P[2], P[3])
        s = R.dense(R.t64(xs), P[0], P[1], 'tanh') + hb
        data, pen = R.mse(s, R.t64(t)), R.t_penalty(hb, (0.01, 0.05)) + R.t_penalty(s, (0.0, 0.02))
        (data + pen).backward()
        loss, want = first_entry(m.train_on_batch(xs, t)), float((data + pen).detach())
        assert float(pen.detach()) > 0.01 * want and abs(loss - want) <= 1e-6 * want, (step, loss, want)
        for got, p in zip(A.get_weights() + B.get_weights(), P):
            w_ref = (p.detach() - LR * p.grad).numpy()
            assert np.abs(got - w_ref).max() / max(np.abs(w_ref).max(), 1e-3) < 1e-4, (step, got.shape)


def test_two_outputs_with_loss_weights_carry_the_penalty_once_in_entry_0():
    from gennet_amd import layers as L
    from gennet_amd.engine import SGD, Input, Model
    rng = np.random.RandomState(9)
    x = Input(shape=(6,))
    trunk = L.Dense(8, activation='tanh', **_regs(THREE))
    a, b = L.Dense(3), L.Dense(1, activation='sigmoid')
    h = trunk(x)
    m = Model(inputs=x, outputs=[a(h), b(h)])
    for layer, shapes in ((trunk, [(6, 8), (8,)]), (a, [(8, 3), (3,)]), (b, [(8, 1), (1,)])):
        layer.set_weights(seeded(shapes, rng))
    m.compile(optimizer=SGD(lr=LR), loss=['mean_squared_error', 'binary_crossentropy'], loss_weights=[1.0, 0.5], metrics=['accuracy'])
    xs, ta, tb = rng.randn(4, 6).astype(np.float32), rng.randn(4, 3).astype(np.float32), rng.randint(0, 2, (4, 1)).astype(np.float32)
    P = [R.t64(w) for l in (trunk, a, b) for w in l.get_weights()]
    hh = R.dense(R.t64(xs), P[0], P[1], 'tanh')
    la, lb = float(R.mse(R.dense(hh, P[2], P[3]), R.t64(ta))), float(R.bce(R.dense(hh, P[4], P[5], 'sigmoid'), R.t64(tb)))
    pen = float(R.t_penalty(P[0], THREE['kernel_regularizer']) + R.t_penalty(P[1], THREE['bias_regularizer']) + R.t_penalty(hh, THREE['activity_regularizer']))
    for res in (m.test_on_batch(xs, [ta, tb]), m.train_on_batch(xs, [ta, tb])):       # the test phase first: the same weights
        assert len(res) == len(m.metrics_names) == 5
        assert abs(res[1] - la) <= 1e-6 * la and abs(res[2] - lb) <= 1e-6 * lb      # the per-output entries exclude the penalty
        want = la + 0.5 * lb + pen
        assert pen > 0.01 * want and abs(res[0] - want) <= 1e-6 * want, (res, want)
        assert all(0.0 <= v <= 1.0 for v in res[3:])                                # ... and so do the metrics


def test_clipnorm_sees_the_regularizer_term():
    """keras clips the gradients of the TOTAL loss: the factor clipnorm / norm is formed from gradients that hold the regularizer terms"""
    from gennet_amd.engine import SGD
    m, first, head, x, t = dense_net(optimizer=SGD(lr=LR, clipnorm=0.1))
    P, data, pen = dense_net_ref(first, head, x, t)
    bare = torch.autograd.grad(data, P, retain_graph=True)
    (data + pen).backward()
    norm, norm_bare = float(torch.sqrt(sum((p.grad ** 2).sum() for p in P))), float(torch.sqrt(sum((b ** 2).sum() for b in bare)))
    assert norm > 0.1 and abs(norm - norm_bare) > 0.01 * norm                       # the clip is active, and the terms change its factor visibly
    loss = first_entry(m.train_on_batch(x, t))
    assert abs(loss - float((data + pen).detach())) <= 1e-6 * float((data + pen).detach())
    for got, p in zip(first.get_weights() + head.get_weights(), P):
        w_ref = (p.detach() - LR * (0.1 / norm) * p.grad).numpy()
        assert np.abs(got - w_ref).max() / max(np.abs(w_ref).max(), 1e-3) < 1e-4


def test_save_and_load_keep_the_regularizers(tmp_path):
    from gennet_amd import h5lite
    from gennet_amd.engine import load_model
    import json
    m, first, head, x, t = dense_net()
    m.train_on_batch(x, t)
    path = os.path.join(str(tmp_path), 'reg.h5')
    m.save(path)
    cfg = json.loads(h5lite.File(path).attrs['model_config'].decode('utf-8'))['config']['layers'][0]['config']
    f32 = lambda v: float(np.float32(v))                                           # noqa: E731
    assert cfg['kernel_regularizer'] == {'class_name': 'L1L2', 'config': {'l1': f32(0.01), 'l2': f32(0.02)}}
    assert cfg['bias_regularizer'] == {'class_name': 'L1L2', 'config': {'l1': 0.0, 'l2': f32(0.1)}}
    assert cfg['activity_regularizer'] == {'class_name': 'L1L2', 'config': {'l1': f32(0.001), 'l2': 0.0}}
    again = load_model(path)
    assert [(p.name, tr) for p, tr in again._reg_params] == [(p.name, tr) for p, tr in m._reg_params] and len(again._reg_nodes) == 1
    r0, r1 = m.train_on_batch(x, t), again.train_on_batch(x, t)
    assert r0 == r1
    assert all(np.array_equal(u, v) for u, v in zip(m.get_weights(), again.get_weights()))


def test_a_captured_step_of_a_regularized_model_replays_bit_identically():
    """the pattern of test_a_captured_step_of_the_stack_replays_bit_identically (tests/test_dilated_gpu.py): eager step, capture, three replays
    against four eager steps of a twin"""
    from gennet_amd import engine
    from gennet_amd.engine import SGD, to_device
    eager, _, _, x, t = dense_net(optimizer=SGD(lr=LR, momentum=0.5, clipnorm=1.0))
    graphed = dense_net(optimizer=SGD(lr=LR, momentum=0.5, clipnorm=1.0))[0]
    graphed.set_weights(eager.get_weights())
    x, t = to_device(x), to_device(t)
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
        assert s0.shape == (2, 2) and s0[1, 0] > 0 and s0[1, 1] == 0                # the statistics and the penalty row
        assert np.array_equal(s0, s1), (step, s0, s1)
        assert all(np.array_equal(u, v) for u, v in zip(w0, w1)), step
    assert not np.array_equal(want[0][0], want[3][0])                              # the steps differ: a replay that did nothing would show


def test_an_unregularized_model_launches_and_returns_what_it_did():
    """keywords given as None against keywords never given: the same plan, the same statistics shape and bits, the same profiled launches"""
    from gennet_amd import layers as L, ops
    from gennet_amd.engine import SGD, Sequential, to_device

    def build(kw1, kw2):
        from gennet_amd import engine
        rng = np.random.RandomState(3)
        engine.set_init_seed(7)                                                    # both models draw the same initial weights
        m = Sequential([L.Conv1D(8, 5, padding='same', input_shape=(16, 8), **kw1), L.LeakyReLU(0.2), L.BatchNormalization(**kw2), L.Flatten(),
                        L.Dense(1, activation='sigmoid', **kw1)])
        m.compile(optimizer=SGD(lr=LR), loss='binary_crossentropy', metrics=['accuracy'])
        return m, to_device(rng.randn(4, 16, 8).astype(np.float32)), to_device(rng.randint(0, 2, (4, 1)).astype(np.float32))
    none3 = dict(kernel_regularizer=None, bias_regularizer=None, activity_regularizer=None)
    results = []
    for kws in (({}, {}), (none3, dict(beta_regularizer=None, gamma_regularizer=None))):
        m, x, t = build(*kws)
        assert m._reg_params == [] and m._reg_nodes == []
        m.train_on_batch_device([x], [t])                                          # binds
        ops.prof_enable(True)
        try:
            ops.prof_reset()
            stats = m.train_on_batch_device([x], [t])
            test = m.test_on_batch_device([x], [t])
            torch.cuda.synchronize()
            launches = ops.prof_collect(-1)['launches']
        finally:
            ops.prof_enable(False)
        assert tuple(stats.shape) == (1, 2) == tuple(test.shape)
        results.append((launches, stats.cpu().numpy(), test.cpu().numpy(), [(n.fused_act, n.absorbed, n.fuse_prev) for n in m.nodes]))
    assert results[0][0] == results[1][0] > 0
    assert np.array_equal(results[0][1], results[1][1]) and np.array_equal(results[0][2], results[1][2]) and results[0][3] == results[1][3]


# ------------------------------------------------------------------------------------------------------------------ data parallel
WORKER = os.path.join(ROOT, 'tests', 'regularizer_dp_worker.py')


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _launch(out, world):
    """As tests/test_sample_weight_gpu.py starts its worker: directly for one rank, torch.distributed.run for more."""
    env = dict(os.environ)
    env.pop('RANK', None); env.pop('WORLD_SIZE', None); env.pop('LOCAL_RANK', None)
    if world == 1:
        cmd = [sys.executable, WORKER, out]
    else:
        cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(world), '--master-addr', '127.0.0.1',
               '--master-port', str(_free_port()), WORKER, out]
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    return [pickle.load(open('%s.%d' % (out, k), 'rb')) for k in range(world)]


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason='needs two GPUs')
def test_two_ranks_equal_one_rank_under_regularizers(tmp_path):
    """2 ranks x B / 2 rows against 1 rank x B rows of the same regularized model (weight and activity regularizers, three Adam steps and a test
    step).  The weight penalties enter once, not once per rank; the activity penalty is the sum over the global batch.  Losses to 1e-5 relative;
    weights to the tolerance tests/test_sample_weight_gpu.py documents (1e-4 relative + 2 % of the Adam step budget); the replicas bit-identical."""
    one = _launch(str(tmp_path / 'one'), 1)[0]
    two = _launch(str(tmp_path / 'two'), 2)
    assert one['penalty_share'] > 0.01
    for r in two:
        assert len(r['losses']) == len(one['losses']) == 4
        for a, b in zip(r['losses'], one['losses']):
            assert np.isfinite(a) and abs(a - b) <= 1e-5 * abs(b), (r['losses'], one['losses'])
        for w, wr in zip(r['weights'], one['weights']):
            assert np.isfinite(w).all()
            assert np.abs(w - wr).max() <= 1e-4 * np.abs(wr).max() + 0.02 * 2 * 9e-5, (w.shape, float(np.abs(w - wr).max()))
    assert two[0]['losses'] == two[1]['losses']
    assert all(np.array_equal(u, v) for u, v in zip(two[0]['weights'], two[1]['weights']))               # replicas stay bit-identical
