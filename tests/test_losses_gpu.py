"""The loss pass (gn_loss_pass, csrc/loss.hip) and what the engine builds on it, on the device: parity of every kind with the fp64 restatement
tests/loss_ref.py at the float32 inputs, the evaluation form, determinism, exact ties, argument checks, the routing between the one-block
kernel and the pass, training against torch fp64 autograd, loss weights, test_on_batch / evaluate / predict_on_batch, a captured step and
the .h5 round trip."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import loss_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0
# Caps.  The pass evaluates every term in fp64 on the float32 inputs and rounds dp and out to float32 once, so what is left is that rounding:
# 2^-24 relative per value.  The bounds of the design (2e-5 of max|dp|, the project's figure for its cross-entropy gradient; 1e-6 relative on
# the loss) are tightened to 4x the worst value measured on the device per kind, which is 4 * 2^-24 = 2.4e-7 for both.
CAP_GRAD = min(2e-5, 4 * 2.0 ** -24)
CAP_LOSS = min(1e-6, 4 * 2.0 ** -24)


def _inside(a, fill, off=1):
    """`a` as a view that starts 4 * off bytes past a 16-byte boundary inside a buffer filled with `fill`: (buffer, view)."""
    n = a.size
    buf = torch.full((n + 8,), fill, dtype=torch.float32, device='cuda')
    assert buf.data_ptr() % 16 == 0
    v = buf[off:off + n]
    v.copy_(torch.from_numpy(np.array(a, dtype=np.float32).ravel()))       # a copy: the cached inputs are read-only
    return buf, v.view(a.shape)


def _untouched(buf, off, n):
    return bool((buf[:off] == SENTINEL).all()) and bool((buf[off + n:] == SENTINEL).all())


@functools.lru_cache(maxsize=None)
def _case(kind, rows, cols):
    """Inputs and fp64 reference of one (kind, shape), computed once and shared: (p, y, {denom: (value, gradient)}, hits)."""
    p, y = R.generate(kind, rows, cols)
    ref = dict((dn, R.value_and_grad(kind, p, y, dn)) for dn in (rows, 2 * rows))
    for a in (p, y) + tuple(g for _, g in ref.values()):
        a.setflags(write=False)
    return p, y, ref, R.hits(p, y)


def _check(kind, out, dp, ref, hits, denom, tag):
    v, g = ref
    got = float(out[0])
    if kind == 'categorical_accuracy':
        assert got == float(np.float32(round(v * denom) / float(denom))), (tag, got, v)
        errl = 0.0
    else:
        errl = abs(got - v) / abs(v) if v != 0.0 else abs(got)      # a sum of exact zeros (every margin of a hinge satisfied) is zero
        assert errl <= CAP_LOSS, (tag, got, v, errl)
    assert float(out[1]) == float(np.float32(hits)), (tag, float(out[1]), hits)
    errg = 0.0
    if dp is not None:
        gmax = float(np.abs(g).max())
        errg = float(np.abs(dp.astype(np.float64) - g).max()) / gmax if gmax > 0 else float(np.abs(dp).max())
        assert errg <= CAP_GRAD, (tag, errg)
    return errl, errg


@pytest.mark.parametrize('kind', R.KINDS)
def test_kernel_parity(kind):
    from gennet_amd import ops
    worst_l = worst_g = 0.0
    for rows, cols in R.GPU_SHAPES:
        p, y, ref, hits = _case(kind, rows, cols)
        _, pv = _inside(p, float('nan'))
        _, yv = _inside(y, float('nan'))
        assert pv.data_ptr() % 16 == 4 and yv.data_ptr() % 16 == 4
        for denom in (rows, 2 * rows):
            dbuf, dv = _inside(np.full((rows, cols), SENTINEL, np.float32), SENTINEL)
            dp, out = ops.loss_pass(kind, pv, yv, denom, dp=dv)
            out = out.cpu().numpy()
            assert _untouched(dbuf, 1, rows * cols), (kind, rows, cols)
            el, eg = _check(kind, out, dv.cpu().numpy(), ref[denom], hits, denom, (kind, rows, cols, denom))
            worst_l, worst_g = max(worst_l, el), max(worst_g, eg)
    print('loss_pass parity %-32s worst relative loss error %.3e, worst gradient error / max|dp| %.3e' % (kind, worst_l, worst_g))


@pytest.mark.parametrize('kind', ('mean_squared_error', 'logcosh', 'categorical_crossentropy'))
def test_kernel_parity_mixed_and_aligned_phases(kind):
    """p, y and dp at different phases of a 16-byte line (the all-scalar path) and all aligned (float4 from the first element)."""
    from gennet_amd import ops
    for rows, cols in ((3, 1030), (100003, 1)):
        p, y, ref, hits = _case(kind, rows, cols)
        for offs in ((1, 2, 3), (0, 0, 0), (0, 0, 2)):
            _, pv = _inside(p, float('nan'), offs[0])
            _, yv = _inside(y, float('nan'), offs[1])
            dbuf, dv = _inside(np.full((rows, cols), SENTINEL, np.float32), SENTINEL, offs[2])
            _, out = ops.loss_pass(kind, pv, yv, rows, dp=dv)
            assert _untouched(dbuf, offs[2], rows * cols)
            _check(kind, out.cpu().numpy(), dv.cpu().numpy(), ref[rows], hits, rows, (kind, rows, cols, offs))


@pytest.mark.parametrize('kind', R.KINDS)
def test_evaluation_form_equals_the_gradient_form(kind):
    from gennet_amd import ops
    for rows, cols in ((5, 3), (3, 1030), (100003, 1)):
        p, y, _, _ = _case(kind, rows, cols)
        _, pv = _inside(p, float('nan'))
        _, yv = _inside(y, float('nan'))
        idle = torch.full((rows * cols + 8,), SENTINEL, dtype=torch.float32, device='cuda')      # handed to nobody
        _, with_grad = ops.loss_pass(kind, pv, yv, 2 * rows)
        none, without = ops.loss_pass(kind, pv, yv, 2 * rows, grad=False)
        assert none is None
        assert np.array_equal(with_grad.cpu().numpy().view(np.uint32), without.cpu().numpy().view(np.uint32)), (kind, rows, cols)
        assert bool((idle == SENTINEL).all())


@pytest.mark.parametrize('kind', ('mean_squared_error', 'binary_crossentropy', 'cosine_proximity', 'categorical_crossentropy'))
def test_two_runs_give_the_same_bits(kind):
    from gennet_amd import ops
    for rows, cols in ((100003, 1), (2, 70001)):
        p, y, _, _ = _case(kind, rows, cols)
        _, pv = _inside(p, float('nan'))
        _, yv = _inside(y, float('nan'))
        runs = []
        for _ in range(2):
            dp, out = ops.loss_pass(kind, pv, yv, rows)
            runs.append((out.cpu().numpy().view(np.uint32).copy(), dp.cpu().numpy().view(np.uint32).copy()))
        assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1]), (kind, rows, cols)


@pytest.mark.parametrize('case', R.tie_cases(), ids=lambda c: c[0])
def test_exact_ties_on_the_device(case):
    from gennet_amd import ops
    kind, p, y, want = case
    p, y = np.asarray(p, np.float32), np.asarray(y, np.float32)
    dp, _ = ops.loss_pass(kind, torch.from_numpy(p).cuda(), torch.from_numpy(y).cuda(), 1)
    assert np.array_equal(dp.cpu().numpy(), np.asarray(want, np.float64).astype(np.float32)), (kind, dp.cpu().numpy(), want)


def test_bad_arguments_are_refused_before_any_launch():
    from gennet_amd import _lib, ops
    L = _lib.lib()
    rows, cols = 300, 2
    p = torch.rand(rows, cols, device='cuda')
    y = torch.rand(rows, cols, device='cuda')
    dp = torch.full((rows, cols), SENTINEL, device='cuda')
    out = torch.full((2,), SENTINEL, device='cuda')
    need = _lib.size('gn_loss_pass_workspace', rows, cols)
    assert need >= 16
    ws = torch.zeros(need, dtype=torch.uint8, device='cuda')
    s = torch.cuda.current_stream().cuda_stream

    def call(kind=1, pp=p, yy=y, oo=out, r=rows, c=cols, denom=float(rows), nbytes=need):
        return L.gn_loss_pass(kind, pp.data_ptr() if pp is not None else None, yy.data_ptr() if yy is not None else None, dp.data_ptr(),
                              oo.data_ptr() if oo is not None else None, r, c, ctypes.c_double(denom), ws.data_ptr(), nbytes, s)

    for what, rc in (('kind', call(kind=99)), ('kind', call(kind=-1)), ('rows', call(r=0)), ('cols', call(c=0)), ('denom', call(denom=rows - 1.0)),
                     ('workspace', call(nbytes=need - 1)), ('p', call(pp=None)), ('y', call(yy=None)), ('out', call(oo=None))):
        assert rc == -1, (what, rc)                                  # GN_EINVAL
        assert L.gn_last_error()
    torch.cuda.synchronize()
    assert bool((dp == SENTINEL).all()) and bool((out == SENTINEL).all())
    with pytest.raises(_lib.GennetHipError):
        ops.loss_pass(99, p, y)
    assert call() == 0                                               # and the same call with good arguments runs
    torch.cuda.synchronize()
    assert not bool((out == SENTINEL).any())


# ------------------------------------------------------------------------------------------------------------------------- engine
def _dense_net(units=(8, 3), acts=('tanh', 'sigmoid'), n_in=16, seed=0):
    from gennet_amd import engine, layers
    m = engine.Sequential([layers.Dense(u, activation=a, **({'input_shape': (n_in,)} if i == 0 else {})) for i, (u, a) in enumerate(zip(units, acts))])
    rng = np.random.RandomState(seed)
    m.set_weights([(0.5 * rng.randn(*w.shape)).astype(np.float32) for w in m.get_weights()])
    return m


def test_routing_small_mse_keeps_the_first_kernel(monkeypatch):
    from gennet_amd import engine, ops
    calls = []
    real = ops.loss_pass
    monkeypatch.setattr(ops, 'loss_pass', lambda *a, **k: calls.append(a[0]) or real(*a, **k))
    rng = np.random.RandomState(1)
    m = _dense_net((8,), ('linear',)).compile(loss='mean_squared_error', optimizer=engine.SGD(lr=0.01))
    x, y = rng.randn(64, 16).astype(np.float32), rng.randn(64, 8).astype(np.float32)
    cap = {}
    res = m.train_on_batch(x, y, capture=cap)
    assert calls == []
    pred = cap[m.layers[-1].name]
    _, out = ops.loss('mean_squared_error', pred.reshape(512, 1), torch.from_numpy(y).cuda().reshape(512, 1), 512)
    assert np.float32(res[0]) == out.cpu().numpy()[0]                # the bits of the one-block kernel


def test_routing_large_mse_takes_the_pass(monkeypatch):
    from gennet_amd import engine, ops
    calls = []
    real = ops.loss_pass
    monkeypatch.setattr(ops, 'loss_pass', lambda *a, **k: calls.append(a[0]) or real(*a, **k))
    rows = 64 if ops.LOSS_PASS_MIN_ELEMENTS <= 262144 else 128
    assert rows * 4096 >= ops.LOSS_PASS_MIN_ELEMENTS
    rng = np.random.RandomState(2)
    m = _dense_net((4096,), ('linear',)).compile(loss='mean_squared_error', optimizer=engine.SGD(lr=0.01))
    x, y = rng.randn(rows, 16).astype(np.float32), rng.randn(rows, 4096).astype(np.float32)
    cap = {}
    res = m.train_on_batch(x, y, capture=cap)
    assert calls == ['mean_squared_error']
    pred = cap[m.layers[-1].name].cpu().numpy()
    v, _ = R.value_and_grad('mean_squared_error', pred, y, rows)
    assert abs(res[0] - v) <= CAP_LOSS * v, (res[0], v)


def _torch_sgd(ws, x, ys, kinds, weights, lr, steps, heads):
    """Three plain SGD steps of the small net in torch fp64: ws = [W1, b1, (Wk, bk) per head]; heads = activation per head."""
    ws = [torch.tensor(w, dtype=torch.float64, requires_grad=True) for w in ws]
    xt = torch.tensor(x, dtype=torch.float64)
    hist = []
    lr = float(np.float32(lr))
    for _ in range(steps):
        h = torch.tanh(xt @ ws[0] + ws[1])
        per = []
        for k, (kind, act) in enumerate(zip(kinds, heads)):
            o = h @ ws[2 + 2 * k] + ws[3 + 2 * k]
            o = torch.sigmoid(o) if act == 'sigmoid' else o
            per.append(R.torch_value(kind, o, torch.tensor(ys[k], dtype=torch.float64), x.shape[0]))
        total = sum(w * l for w, l in zip(weights, per))
        for w in ws:
            w.grad = None
        total.backward()
        with torch.no_grad():
            for w in ws:
                w -= lr * w.grad
        hist.append([float(total.detach())] + [float(l.detach()) for l in per])
    return hist, [w.detach().numpy() for w in ws]


def _targets(kind, rng, rows, cols):
    if kind == 'hinge':
        return rng.choice([-1.0, 1.0], (rows, cols)).astype(np.float32)
    if kind == 'categorical_crossentropy':
        return np.eye(cols, dtype=np.float32)[rng.randint(0, cols, rows)]
    return rng.uniform(0.1, 0.9, (rows, cols)).astype(np.float32)


@pytest.mark.parametrize('kind', ('logcosh', 'hinge', 'categorical_crossentropy', 'cosine_proximity'))
def test_training_matches_torch_autograd(kind):
    from gennet_amd import engine
    rng = np.random.RandomState(5)
    m = _dense_net(seed=4).compile(loss=kind, optimizer=engine.SGD(lr=0.1))
    w0 = m.get_weights()
    x, y = rng.randn(12, 16).astype(np.float32), _targets(kind, rng, 12, 3)
    got = [m.train_on_batch(x, y) for _ in range(3)]
    hist, wref = _torch_sgd(w0, x, [y], [kind], [1.0], 0.1, 3, ['sigmoid'])
    for g, h in zip(got, hist):
        assert len(g) == 1 and abs(g[0] - h[0]) <= 1e-5 * max(1.0, abs(h[0])), (kind, got, hist)
    for a, b in zip(m.get_weights(), wref):
        assert np.abs(a - b).max() <= 1e-5, (kind, np.abs(a - b).max())


def _two_head_net(seed=6):
    from gennet_amd import engine, layers
    x = engine.Input(shape=(16,))
    h = layers.Dense(8, activation='tanh')(x)
    m = engine.Model(inputs=x, outputs=[layers.Dense(3, activation='sigmoid')(h), layers.Dense(1)(h)])
    rng = np.random.RandomState(seed)
    m.set_weights([(0.5 * rng.randn(*w.shape)).astype(np.float32) for w in m.get_weights()])
    return m


def test_loss_weights_scale_gradient_and_total_not_the_entries():
    from gennet_amd import engine
    rng = np.random.RandomState(7)
    kinds, weights = ['logcosh', 'mean_squared_error'], [0.25, 2.0]
    m = _two_head_net().compile(loss=kinds, optimizer=engine.SGD(lr=0.1), loss_weights=weights)
    w0 = m.get_weights()
    x = rng.randn(12, 16).astype(np.float32)
    ys = [_targets('logcosh', rng, 12, 3), rng.randn(12, 1).astype(np.float32)]
    got = [m.train_on_batch(x, ys) for _ in range(3)]
    hist, wref = _torch_sgd(w0, x, ys, kinds, weights, 0.1, 3, ['sigmoid', 'linear'])
    for g, h in zip(got, hist):
        assert len(g) == 3
        assert g[0] == pytest.approx(0.25 * g[1] + 2.0 * g[2], rel=1e-12)       # the total is the weighted sum of the unweighted entries
        assert np.abs(np.asarray(g) - np.asarray(h)).max() <= 1e-5 * max(1.0, abs(h[0])), (got, hist)
    for a, b in zip(m.get_weights(), wref):                                     # the first layer saw the weighted gradient
        assert np.abs(a - b).max() <= 1e-5, np.abs(a - b).max()


def _bn_dropout_net():
    from gennet_amd import engine, layers
    m = engine.Sequential([layers.Dense(8, input_shape=(16,)), layers.BatchNormalization(), layers.Activation('tanh'), layers.Dropout(0.3),
                           layers.Dense(3, activation='sigmoid')])
    return m.compile(loss='logcosh', optimizer=engine.Adam(lr=1e-2), metrics=['accuracy', 'mae'])


def _state(m):
    return [w.copy() for w in m.get_weights()] + [np.array(a).copy() for a in m.optimizer.get_keras_weights(m._keras_train_order())]


def test_test_on_batch_is_the_inference_phase_and_changes_nothing():
    from gennet_amd import ops
    rng = np.random.RandomState(8)
    m = _bn_dropout_net()
    x, y = rng.randn(24, 16).astype(np.float32), rng.randint(0, 2, (24, 3)).astype(np.float32)
    m.train_on_batch(x, y)
    m.train_on_batch(x, y)                                           # moving statistics and Adam moments are no longer their initial values
    before = _state(m)
    res = m.test_on_batch(x, y)
    assert m.metrics_names == ['loss', 'acc', 'mean_absolute_error'] and len(res) == 3
    after = _state(m)
    assert len(before) == len(after) and all(np.array_equal(a, b) for a, b in zip(before, after))
    pred = m.predict(x)
    pd, yd = torch.from_numpy(pred).cuda(), torch.from_numpy(y).cuda()
    _, lo = ops.loss_pass('logcosh', pd, yd, 24, grad=False)
    _, ma = ops.loss_pass('mean_absolute_error', pd, yd, 24, grad=False)
    lo, ma = lo.cpu().numpy(), ma.cpu().numpy()
    assert res == [float(lo[0]), float(lo[1]) / (24 * 3), float(ma[0])]
    assert res[1] == R.metric('accuracy', pred, y) and abs(res[2] - R.metric('mae', pred, y)) <= CAP_LOSS * res[2]
    assert abs(res[0] - R.value_and_grad('logcosh', pred, y)[0]) <= CAP_LOSS * res[0]
    train = m.train_on_batch(x, y)                                   # the training phase (batch statistics, dropout) gives another number
    assert train[0] != res[0]


def test_evaluate_and_predict_on_batch():
    rng = np.random.RandomState(9)
    m = _bn_dropout_net()
    x, y = rng.randn(70, 16).astype(np.float32), rng.randint(0, 2, (70, 3)).astype(np.float32)
    m.train_on_batch(x[:32], y[:32])
    parts = [np.asarray(m.test_on_batch(x[s:s + 32], y[s:s + 32])) * len(x[s:s + 32]) for s in (0, 32, 64)]
    want = (parts[0] + parts[1] + parts[2]) / 70.0
    got = m.evaluate(x, y, batch_size=32)
    assert isinstance(got, list) and len(got) == 3
    assert np.allclose(got, want, rtol=1e-12, atol=0)
    assert np.array_equal(m.predict_on_batch(x[:20]), m.predict(x[:20]))
    assert np.abs(m.predict_on_batch(x) - m.predict(x, batch_size=32)).max() <= 1e-6
    assert m.predict_on_batch(x).shape == (70, 3)


def test_captured_steps_equal_eager_steps():
    from gennet_amd import engine
    rng = np.random.RandomState(10)
    x, y = rng.randn(12, 16).astype(np.float32), rng.uniform(0, 1, (12, 3)).astype(np.float32)

    def make():
        return _dense_net(seed=11).compile(loss='logcosh', optimizer=engine.Adam(lr=1e-2), metrics=['accuracy', 'mae'])

    a = make()
    eager = [a.train_on_batch(x, y) for _ in range(4)]
    b = make()
    xd, yd = engine.to_device(x), engine.to_device(y)
    got = [b.train_result(b.train_on_batch_device([xd], [yd]), 12)]               # binds the optimizer state
    sg = engine.StepGraph()
    torch.cuda.synchronize()
    sg.capture(lambda: b.train_on_batch_device([xd], [yd]))
    for _ in range(3):
        sg.wait_inputs_consumed()
        got.append(b.train_result(sg.replay(), 12))
    assert len(eager[0]) == 3 and got == eager                       # losses and both metrics, bit for bit
    assert all(np.array_equal(u, v) for u, v in zip(a.get_weights(), b.get_weights()))


def test_save_and_load_keep_loss_weights_and_metrics(tmp_path):
    from gennet_amd import engine
    rng = np.random.RandomState(12)
    x = rng.randn(12, 16).astype(np.float32)
    ys = [_targets('logcosh', rng, 12, 3), rng.randn(12, 1).astype(np.float32)]
    m = _two_head_net().compile(loss=['logcosh', 'mse'], optimizer=engine.Adam(lr=1e-2), metrics=['accuracy', 'mae'], loss_weights=[0.25, 2.0])
    m.train_on_batch(x, ys)
    path = str(tmp_path / 'model.h5')
    m.save(path)
    back = engine.load_model(path)
    assert back.loss == ['logcosh', 'mse'] and back.loss_weights == [0.25, 2.0] and back.metrics == ['accuracy', 'mae']
    assert back.metrics_names == m.metrics_names and len(m.metrics_names) == 7
    assert back.train_on_batch(x, ys) == m.train_on_batch(x, ys)     # the uninterrupted run, bit for bit
    assert all(np.array_equal(u, v) for u, v in zip(back.get_weights(), m.get_weights()))
