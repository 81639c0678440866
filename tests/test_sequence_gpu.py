"""The sequence layers on the GPU.

Section 1: the four entry points of csrc/sequence.hip against tests/sequence_ref.py on the smallest shapes at which each path can go wrong --
copies bit for bit, the fp64 sum of RepeatVector's gradient within its derived bound -- inside sentinel-surrounded buffers.
Section 2: Dense over the last axis is, bit for bit, the one-tap Conv1D it runs as, and TimeDistributed(Dense) is that Dense.
Section 3: three models against torch fp64 stepping through the references, their .h5 round trip and their captured step."""
import itertools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lstm_ref as R
import sequence_ref as S

pytestmark = pytest.mark.gpu

PAD = 64                          # floats around every guarded view: 256 bytes, so a view keeps the alignment of its buffer
SENTINEL = -12345.5


def dev():
    return torch.device('cuda')


class Guarded(object):
    """A contiguous view inside a larger flat buffer: inputs surrounded by NaN, outputs inside a sentinel-filled buffer.  shift: the view starts
    that many floats later (1: a base that is not 16-byte aligned)."""

    def __init__(self, shape, value=None, shift=0):
        n = int(np.prod(shape))
        self.n, self.lo = n, PAD + shift
        self.buf = torch.full((n + 2 * PAD + shift,), float('nan') if value is not None else SENTINEL, dtype=torch.float32, device=dev())
        self.t = self.buf[self.lo:self.lo + n].view(shape)
        if value is not None:
            self.t.copy_(torch.tensor(np.asarray(value, np.float32), device=dev()))
        assert self.t.is_contiguous() and (self.t.data_ptr() % 16 == 0) == (shift % 4 == 0)

    def check(self, what):
        """the surroundings untouched and every element of the view written"""
        edges = torch.cat([self.buf[:self.lo], self.buf[self.lo + self.n:]])
        assert bool((edges == SENTINEL).all()), '%s: wrote outside its output' % what
        assert not bool(torch.isnan(self.t).any()), '%s: an element outside an input was read' % what
        assert not bool((self.t == SENTINEL).any()), '%s: output elements left unwritten' % what
        return self.t.cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------
# section 1: the kernels
# ---------------------------------------------------------------------------------------------------------------------
PERMUTE_CASES = ([((3, 33, 18), (0, 2, 1)),                 # partial tiles at both edges
                  ((2, 64, 64), (0, 2, 1)),                 # full tiles
                  ((1, 1, 9), (0, 2, 1)), ((4, 130, 1), (0, 2, 1)),          # degenerate extents: nothing is left to permute
                  ((2, 8, 12), (0, 1, 2)),                  # the identity
                  ((2, 3, 5, 8), (0, 2, 1, 3)), ((2, 3, 5, 6), (0, 2, 1, 3)),  # the inner axis stays: 16-byte and 4-byte units
                  ((3, 70), (1, 0)), ((2, 3, 40, 35), (0, 3, 2, 1)), ((2, 3, 40, 35), (0, 3, 1, 2))]       # rank 2; two batch axes; a merged plane axis
                 + [((2, 5, 7, 6), (0,) + p) for p in itertools.permutations((1, 2, 3))])                # merged axes, inner stays, inner changes batched


@pytest.mark.parametrize('shape,perm', PERMUTE_CASES, ids=['%s-%s' % ('x'.join(map(str, s)), ''.join(map(str, p))) for s, p in PERMUTE_CASES])
def test_permute_is_exact_and_its_inverse_returns_the_input(shape, perm):
    from gennet_amd import ops
    rng = np.random.RandomState(sum(shape))
    x = rng.randn(*shape).astype(np.float32)
    ref = S.permute_fwd(x, perm)
    for shift in (0, 1):                                    # 1: both bases off the 16-byte grid, the all-scalar form
        X, Y = Guarded(shape, x, shift), Guarded(ref.shape, None, shift)
        assert ops.permute(X.t, perm, out=Y.t) is Y.t
        assert same_bits(Y.check('permute'), ref)
        assert torch.equal(ops.permute(X.t, perm), Y.t)
        back = Guarded(shape, None, shift)
        ops.permute(Y.t, S.inverse_perm(perm), out=back.t)
        assert same_bits(back.check('inverse permute'), x)


def test_permute_refuses_what_is_no_permutation():
    from gennet_amd import ops
    x = torch.zeros((2, 3, 4), device=dev())
    for bad in ((0, 1), (0, 1, 1), (0, 1, 3)):
        with pytest.raises(ValueError):
            ops.permute(x, bad)


SHIFT_SHAPES = [(3, 5, 3), (2, 5, 8), (1, 1, 4)]
SHIFT_PADS = [(0, 0), (2, 0), (0, 3), (1, 2)]


@pytest.mark.parametrize('left,right', SHIFT_PADS)
@pytest.mark.parametrize('B,L,C', SHIFT_SHAPES)
def test_shift1d_pads_with_plus_zero_crops_and_each_undoes_the_other(B, L, C, left, right):
    from gennet_amd import ops
    rng = np.random.RandomState(B * 100 + L * 10 + C + left + right)
    x = rng.randn(B, L, C).astype(np.float32)
    x[0, 0, 0] = -0.0                                         # a negative zero of the input is carried, the padding is +0
    for shift in (0, 1):
        X = Guarded(x.shape, x, shift)
        P = Guarded((B, left + L + right, C), None, shift)
        ops.shift1d(X.t, left, left + L + right, out=P.t)
        padded = P.check('pad')
        assert same_bits(padded, S.pad_fwd(x, left, right))
        border = np.concatenate([padded[:, :left], padded[:, left + L:]], axis=1)
        assert (border.view(np.uint32) == 0).all()            # exactly +0: no sign bit
        back = Guarded(x.shape, None, shift)
        ops.shift1d(P.t, -left, L, out=back.t)
        assert same_bits(back.check('crop of the padded'), x)
        if L - left - right >= 1:
            Cr = Guarded((B, L - left - right, C), None, shift)
            ops.shift1d(X.t, -left, L - left - right, out=Cr.t)
            assert same_bits(Cr.check('crop'), S.crop_fwd(x, left, right))
            G = Guarded(x.shape, None, shift)                 # the crop's backward: its gradient behind `left` rows of +0
            ops.shift1d(Cr.t, left, L, out=G.t)
            assert same_bits(G.check('crop backward'), S.crop_bwd(S.crop_fwd(x, left, right), left, right))


REPEAT_CASES = [(B, C, n) for (B, C) in ((3, 5), (2, 64)) for n in (1, 7, 130)]


@pytest.mark.parametrize('B,C,n', REPEAT_CASES)
def test_repeat_fwd_is_exact(B, C, n):
    from gennet_amd import ops
    x = np.random.RandomState(B + C + n).randn(B, C).astype(np.float32)
    for shift in (0, 1):
        X, Y = Guarded(x.shape, x, shift), Guarded((B, n, C), None, shift)
        ops.repeat_fwd(X.t, n, out=Y.t)
        assert same_bits(Y.check('repeat'), S.repeat_fwd(x, n))


@pytest.mark.parametrize('B,C,n', REPEAT_CASES + [(1, 3, 4100)])
def test_repeat_bwd_meets_the_derived_bound_and_repeats_itself(B, C, n):
    """|got - ref64| <= 2^-24 |ref64| + n 2^-52 sum_j |dy|: one rounding to fp32 of a sum accumulated in fp64"""
    from gennet_amd import ops
    rng = np.random.RandomState(B + C + n)
    dy = (rng.randn(B, n, C) * np.exp(rng.uniform(-3, 3, (B, n, C)))).astype(np.float32)
    ref = S.repeat_bwd(dy)
    bound = 2.0 ** -24 * np.abs(ref) + n * 2.0 ** -52 * np.abs(dy.astype(np.float64)).sum(1)
    for shift in (0, 1):
        DY, DX, DX2 = Guarded(dy.shape, dy, shift), Guarded((B, C), None, shift), Guarded((B, C), None, shift)
        ops.repeat_bwd(DY.t, out=DX.t)
        got = DX.check('repeat backward')
        err = np.abs(got.astype(np.float64) - ref)
        print('shift', shift, 'max err / bound %.3g' % (err / bound).max())
        assert (err <= bound).all()
        ops.repeat_bwd(DY.t, out=DX2.t)
        assert same_bits(DX2.check('repeat backward again'), got)
        if shift == 0:
            first = got
        else:
            assert same_bits(got, first)                      # the 16-byte and the 4-byte form add in the same order


# ---------------------------------------------------------------------------------------------------------------------
# section 2: Dense over the last axis = the one-tap Conv1D; TimeDistributed(Dense) = that Dense
# ---------------------------------------------------------------------------------------------------------------------
def run_layer(layer, x, dy):
    """forward and backward of a lone layer on device tensors -> y, dx, the weight gradients"""
    from gennet_amd import engine
    in_shape = tuple(x.shape[1:])
    layer._ensure_built(in_shape)
    node = engine.Node(layer, [0], layer._shape_after(in_shape))
    node.index = 0
    engine.group_params(layer.params)
    for p in layer.params:
        p.grad.zero_()
    ctx = engine.RunContext(True)
    y = layer.forward(ctx, node, x)
    dx = layer.backward(ctx, node, dy.clone(), True, True)
    assert not ctx.tape
    return y, dx, [p.grad.clone() for p in layer.params]


def rel(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-30)


DENSE_CASES = [((3, 7, 6), 5, 'linear'),         # every extent unaligned: the any-channel kernels
               ((2, 16, 64), 32, 'linear'),      # aligned: the matrix-core kernels
               ((4, 9, 8), 1, 'linear'),         # the small-output head
               ((3, 7, 6), 5, 'tanh'), ((2, 3, 4, 8), 12, 'relu')]       # an epilogue; rank 4


@pytest.mark.parametrize('shape,units,activation', DENSE_CASES, ids=['%s-%d-%s' % ('x'.join(map(str, s)), u, a) for s, u, a in DENSE_CASES])
def test_dense_on_a_sequence_is_the_one_tap_conv1d_bit_for_bit(shape, units, activation):
    """The layer it shares kernels with is Conv1D(units, 1) on the (B, positions, features) view, in all three directions.  Against
    the fp64 reference: 2e-5 of the largest value, the bound tests/test_conv_anyc_gpu.py:163, :176 and :187 hold that kernel family to (forward,
    data gradient, weight and bias gradient; its entry points run every channel pair, the aligned ones on the strict kernels with the same
    bits, :217)."""
    from gennet_amd import layers as Ly
    from gennet_amd.engine import to_device
    rng = np.random.RandomState(units + shape[-1])
    C = shape[-1]
    x = rng.randn(*shape).astype(np.float32)
    w = (rng.randn(C, units) / np.sqrt(C)).astype(np.float32)
    b = rng.randn(units).astype(np.float32)
    dy = rng.randn(*(shape[:-1] + (units,))).astype(np.float32)
    dense, wrapped, conv = Ly.Dense(units, activation=activation), Ly.TimeDistributed(Ly.Dense(units, activation=activation)), Ly.Conv1D(units, 1, activation=activation)
    x3, dy3 = x.reshape(shape[0], -1, C), dy.reshape(shape[0], -1, units)
    for layer, xin in ((dense, x), (wrapped, x), (conv, x3)):
        layer._ensure_built(tuple(xin.shape[1:]))
        layer.set_weights([w[None] if layer is conv else w, b])
    assert dense.per_position and wrapped.layer.per_position
    y, dx, (dw, db) = run_layer(dense, to_device(x), to_device(dy))
    yc, dxc, (dwc, dbc) = run_layer(conv, to_device(x3), to_device(dy3))
    assert tuple(y.shape) == shape[:-1] + (units,) and tuple(dx.shape) == shape
    assert torch.equal(y.reshape(yc.shape), yc) and torch.equal(dx.reshape(dxc.shape), dxc)
    assert torch.equal(dw, dwc[0]) and torch.equal(db, dbc)
    yw, dxw, (dww, dbw) = run_layer(wrapped, to_device(x), to_device(dy))
    assert torch.equal(yw, y) and torch.equal(dxw, dx) and torch.equal(dww, dw) and torch.equal(dbw, db)
    # the fp64 reference
    z = S.dense_fwd(x, w, b)
    y_ref = {'linear': z, 'tanh': np.tanh(z), 'relu': np.maximum(z, 0)}[activation]
    dz = dy * {'linear': np.ones_like(z), 'tanh': 1 - np.tanh(z) ** 2, 'relu': (z > 0).astype(np.float64)}[activation]
    dx_ref, dw_ref, db_ref = S.dense_bwd(x, w, dz)
    errs = [rel(y.cpu().numpy(), y_ref), rel(dx.cpu().numpy(), dx_ref), rel(dw.cpu().numpy(), dw_ref), rel(db.cpu().numpy(), db_ref)]
    print('y dx dw db err', ' '.join('%.3g' % e for e in errs))
    assert max(errs) < 2e-5


def test_a_frozen_dense_on_a_sequence_still_hands_on_the_data_gradient():
    from gennet_amd import engine, layers as Ly
    from gennet_amd.engine import to_device
    rng = np.random.RandomState(4)
    x, dy = rng.randn(3, 7, 6).astype(np.float32), rng.randn(3, 7, 5).astype(np.float32)
    layer = Ly.Dense(5)
    y, dx, _ = run_layer(layer, to_device(x), to_device(dy))
    node = engine.Node(layer, [0], (7, 5))
    node.index = 0
    ctx = engine.RunContext(True)
    layer.forward(ctx, node, to_device(x))
    assert torch.equal(layer.backward(ctx, node, to_device(dy), True, False), dx)
    ctx = engine.RunContext(False)                            # the inference phase keeps nothing
    assert torch.equal(layer.forward(ctx, node, to_device(x)), y) and not ctx.tape


# ---------------------------------------------------------------------------------------------------------------------
# section 3: models against torch fp64 stepping through sequence_ref.py and lstm_ref.py.  The procedure and every bound are those of the
# model-level LSTM tests, tests/test_lstm_gpu.py:441-483 (train_and_compare): predict within 1e-5 of the largest value (:454), each step's loss
# within 1e-6 relative (:468), every gradient and every weight after its step within 1e-4 (:481), over three SGD steps on mean squared error.
# ---------------------------------------------------------------------------------------------------------------------
LR = 0.05


def seed_biases(model, rng):
    for l in model.layers:
        ws = l.get_weights()
        if ws:
            l.set_weights(ws[:-1] + [(ws[-1] + 0.1 * rng.randn(*ws[-1].shape)).astype(np.float32)])


def train_and_compare(model, ref_forward, x, t, steps=3, what='', frozen=()):
    from gennet_amd.engine import SGD
    model.compile(optimizer=SGD(lr=LR), loss='mean_squared_error')
    layers = [l for l in model.layers if l.weights]
    P = dict((l.name, [torch.tensor(w.astype(np.float64), requires_grad=True) for w in l.get_weights()]) for l in layers)
    xt, tt = torch.tensor(x.astype(np.float64)), torch.tensor(t.astype(np.float64))
    y = model.predict(x, batch_size=len(t))
    with torch.no_grad():
        y_ref = ref_forward(P, xt).numpy()
    print(what, 'predict err %.3g' % rel(y, y_ref))
    assert rel(y, y_ref) < 1e-5
    losses = []
    for step in range(steps):
        for ts in P.values():
            for v in ts:
                v.grad = None
        loss_ref = ((ref_forward(P, xt) - tt) ** 2).mean()
        loss_ref.backward()
        res = model.train_on_batch(x, t)
        res = res[0] if isinstance(res, (list, tuple)) else res
        print(what, 'step', step, 'loss', res, float(loss_ref.detach()))
        assert abs(res - float(loss_ref.detach())) <= 1e-6 * abs(float(loss_ref.detach()))
        losses.append(float(loss_ref.detach()))
        g_floor = 1e-3 * max(float(v.grad.abs().max()) for ts in P.values() for v in ts)
        for l in layers:
            if l in frozen:
                continue
            for p, ref in zip(l.params, P[l.name]):
                g_ref = ref.grad.numpy()
                gerr = np.abs(p.grad.detach().cpu().numpy().reshape(g_ref.shape) - g_ref).max() / max(np.abs(g_ref).max(), g_floor)
                with torch.no_grad():
                    ref -= LR * ref.grad
                w_ref = ref.detach().numpy()
                werr = np.abs(p.numpy().astype(np.float64) - w_ref).max() / max(np.abs(w_ref).max(), 1e-3)
                print(what, step, l.name, p.name, 'grad err %.3g weight err %.3g' % (gerr, werr))
                assert gerr < 1e-4 and werr < 1e-4, (step, l.name, p.name, gerr, werr)
    assert len(set(losses)) == steps                                       # the steps differ


def lstm_ref(P, layer, x):
    W, U, b = P[layer.name]
    return R.torch_forward(x, W, U, b, None, None, layer.activation, layer.recurrent_activation, layer.return_sequences, layer.go_backwards)


def conv_ref(P, layer, x):
    w, b = P[layer.name]
    return F.conv1d(x.permute(0, 2, 1), w.permute(2, 1, 0)).permute(0, 2, 1) + b


def autoencoder(head_trainable=True):
    """Input((12, 3)) -> LSTM(8) -> RepeatVector(12) -> LSTM(8, return_sequences=True) -> TimeDistributed(Dense(3)); B = 5"""
    from gennet_amd import layers as Ly
    from gennet_amd.engine import Input, Model
    enc, dec = Ly.LSTM(8), Ly.LSTM(8, return_sequences=True)
    head = Ly.TimeDistributed(Ly.Dense(3, trainable=head_trainable))
    x = Input((12, 3))
    model = Model(inputs=x, outputs=head(dec(Ly.RepeatVector(12)(enc(x)))))

    def ref(P, x):
        h = lstm_ref(P, dec, S.torch_repeat(lstm_ref(P, enc, x), 12))
        return S.torch_dense(h, *P[head.name])
    rng = np.random.RandomState(41)
    return model, ref, rng.randn(5, 12, 3).astype(np.float32), rng.randn(5, 12, 3).astype(np.float32)


def attention_block():
    """x = Input((6, 4)); a = Permute((2, 1)) -> Dense(6, softmax) -> Permute((2, 1)); Multiply([x, a]) -> Flatten -> Dense(1); B = 3"""
    from gennet_amd import layers as Ly
    from gennet_amd.engine import Input, Model
    scores, head = Ly.Dense(6, activation='softmax'), Ly.Dense(1)
    x = Input((6, 4))
    a = Ly.Permute((2, 1))(scores(Ly.Permute((2, 1))(x)))
    model = Model(inputs=x, outputs=head(Ly.Flatten()(Ly.Multiply()([x, a]))))

    def ref(P, x):
        a = torch.softmax(S.torch_dense(S.torch_permute(x, (0, 2, 1)), *P[scores.name]), dim=-1)
        return (x * S.torch_permute(a, (0, 2, 1))).reshape(x.shape[0], -1) @ P[head.name][0] + P[head.name][1]
    rng = np.random.RandomState(42)
    return model, ref, rng.randn(3, 6, 4).astype(np.float32), rng.randn(3, 1).astype(np.float32)


def unet_skip():
    """Input((20, 4)) -> Conv1D(8, 3) = s (18) -> MaxPooling1D(2) (9) -> Conv1D(8, 3) (7) -> UpSampling1D(2) (14) -> ZeroPadding1D((1, 1)) (16),
    Concatenate with Cropping1D((1, 1))(s) (16) -> Conv1D(1, 1); B = 2"""
    from gennet_amd import layers as Ly
    from gennet_amd.engine import Input, Model
    down, mid, head = Ly.Conv1D(8, 3, padding='valid'), Ly.Conv1D(8, 3, padding='valid'), Ly.Conv1D(1, 1)
    x = Input((20, 4))
    s = down(x)
    up = Ly.ZeroPadding1D((1, 1))(Ly.UpSampling1D(2)(mid(Ly.MaxPooling1D(2)(s))))
    model = Model(inputs=x, outputs=head(Ly.Concatenate()([up, Ly.Cropping1D((1, 1))(s)])))
    assert [n.out_shape for n in model.nodes] == [(18, 8), (9, 8), (7, 8), (14, 8), (16, 8), (16, 8), (16, 16), (16, 1)]

    def ref(P, x):
        s = conv_ref(P, down, x)
        m = conv_ref(P, mid, F.max_pool1d(s.permute(0, 2, 1), 2).permute(0, 2, 1))
        up = S.torch_pad(m.repeat_interleave(2, dim=1), 1, 1)
        return conv_ref(P, head, torch.cat([up, S.torch_crop(s, 1, 1)], dim=2))
    rng = np.random.RandomState(43)
    return model, ref, rng.randn(2, 20, 4).astype(np.float32), rng.randn(2, 16, 1).astype(np.float32)


MODELS = {'autoencoder': autoencoder, 'attention': attention_block, 'unet': unet_skip}


@pytest.mark.parametrize('name', sorted(MODELS))
def test_the_model_trains_as_the_fp64_reference(name):
    model, ref, x, t = MODELS[name]()
    seed_biases(model, np.random.RandomState(7))
    train_and_compare(model, ref, x, t, what=name)


@pytest.mark.parametrize('name', sorted(MODELS))
def test_save_load_predict_is_bit_equal(name, tmp_path):
    from gennet_amd.engine import SGD, load_model
    model, _, x, t = MODELS[name]()
    seed_biases(model, np.random.RandomState(8))
    model.compile(optimizer=SGD(lr=LR), loss='mean_squared_error')
    model.train_on_batch(x, t)
    path = os.path.join(str(tmp_path), name + '.h5')
    model.save(path)
    again = load_model(path)
    assert [type(n.layer).__name__ for n in again.nodes] == [type(n.layer).__name__ for n in model.nodes]
    assert [l.get_config() for l in again.layers] == [l.get_config() for l in model.layers]
    assert same_bits(model.predict(x), again.predict(x))
    a, b = model.train_on_batch(x, t), again.train_on_batch(x, t)
    assert a == b and all(np.array_equal(u, v) for u, v in zip(model.get_weights(), again.get_weights()))


@pytest.mark.parametrize('name', sorted(MODELS))
def test_a_captured_step_replays_bit_identically(name):
    """eager step, capture (engine.StepGraph), two replays against three eager steps of a twin, as tests/test_lstm_gpu.py:607"""
    from gennet_amd import engine
    from gennet_amd.engine import SGD, to_device
    eager, _, x, t = MODELS[name]()
    graphed = MODELS[name]()[0]
    seed_biases(eager, np.random.RandomState(9))
    graphed.set_weights(eager.get_weights())
    for m in (eager, graphed):
        m.compile(optimizer=SGD(lr=LR, momentum=0.5), loss='mean_squared_error')
    xs, ts = eager._prep_inputs(x), eager._prep_targets(t, len(t))
    want = []
    for _ in range(3):
        want.append((eager.train_on_batch_device(xs, ts).cpu().numpy().copy(), [w.copy() for w in eager.get_weights()]))
    got = [(graphed.train_on_batch_device(xs, ts).cpu().numpy().copy(), [w.copy() for w in graphed.get_weights()])]
    sg = engine.StepGraph()
    torch.cuda.synchronize()
    sg.capture(lambda: graphed.train_on_batch_device(xs, ts))
    for _ in range(2):
        sg.wait_inputs_consumed()
        stats = sg.replay()
        torch.cuda.synchronize()
        got.append((stats.cpu().numpy().copy(), [w.copy() for w in graphed.get_weights()]))
    for step, ((s0, w0), (s1, w1)) in enumerate(zip(want, got)):
        assert np.array_equal(s0, s1), (step, s0, s1)
        assert all(np.array_equal(u, v) for u, v in zip(w0, w1)), step
    assert not np.array_equal(want[0][0], want[2][0])                      # the steps differ: a replay that did nothing would show


def test_a_frozen_time_distributed_head_keeps_its_weights_and_passes_the_gradient_on():
    model, ref, x, t = autoencoder(head_trainable=False)
    seed_biases(model, np.random.RandomState(10))
    head = model.layers[-1]
    assert type(head).__name__ == 'TimeDistributed' and not head.trainable
    before = [w.copy() for w in model.get_weights()]
    train_and_compare(model, ref, x, t, steps=1, what='frozen head', frozen=(head,))
    after = model.get_weights()
    assert all(same_bits(a, b) for a, b in zip(before[-2:], after[-2:]))                   # the head's kernel and bias
    assert all(not np.array_equal(a, b) for a, b in zip(before[:-2], after[:-2]))          # both LSTMs moved: the gradient passed the frozen head
