"""The weighted loss pass (gn_weight_count, gn_loss_pass_weighted, csrc/loss.hip) and Keras' sample_weight / class_weight / weighted_metrics
on it, on the device: parity of every kind with the fp64 restatement tests/loss_weight_ref.py, phases, the evaluation form, determinism, the
exact count, zero and all-zero weights, argument checks, training against torch fp64 autograd of Keras' expression, class_weight, a
two-output model, both metric lists, test_on_batch / evaluate / fit, routing, a captured step with a static weight tensor, the .h5 round trip
and two data-parallel ranks against one.

Worst values measured on an MI355X, kernel parity over loss_ref.GPU_SHAPES and both counts (loss error over the conditioning sum
sum |w_r l_r| / count; gradient error over max |dp|; error of out[2] over sum |w_r| hits_r / (count cols)): DESIGN.md section 8f."""
import functools
import os
import pickle
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import loss_ref as R
import loss_weight_ref as W

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 12345.0
# The weighted pass does the arithmetic of the unweighted one (fp64 terms on the float32 inputs, one rounding of dp and of out to float32), so
# its caps are those of tests/test_losses_gpu.py: 4 * 2^-24.  With negative weights the weighted sum cancels, so the loss error is taken
# over the conditioning sum, not over |loss|.
CAP = 4 * 2.0 ** -24


def _inside(a, fill, off=1):
    """`a` as a view that starts 4 * off bytes past a 16-byte boundary inside a buffer filled with `fill`: (buffer, view)."""
    n = a.size
    buf = torch.full((n + 8,), fill, dtype=torch.float32, device='cuda')
    assert buf.data_ptr() % 16 == 0
    v = buf[off:off + n]
    v.copy_(torch.from_numpy(np.array(a, dtype=np.float32).ravel()))
    return buf, v.view(a.shape)


def _untouched(buf, off, n):
    return bool((buf[:off] == SENTINEL).all()) and bool((buf[off + n:] == SENTINEL).all())


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()                      # a copy: the cached inputs are read-only


# twelve rows' weights of the engine tests: two zeros, two negative ones
SW12 = np.array([1.5, 0.0, -0.5, 2.0, 0.25, 4.0, 0.0, 1.0, 3.0, -1.25, 0.5, 2.5], np.float32)


def _count(c):
    return torch.tensor([float(c)], dtype=torch.float64, device='cuda')


@functools.lru_cache(maxsize=None)
def _case(kind, rows, cols):
    """Inputs and fp64 reference of one (kind, shape), computed once and shared:
    (p, y, w, local count, {count: (value, gradient, hit share, conditioning sum)}, hits, {count: hit conditioning})."""
    p, y = R.generate(kind, rows, cols)
    w = W.weights(rows)
    cnt = int(np.count_nonzero(w))
    ref = dict((c, W.weighted_value_and_grad(kind, p, y, w, c)) for c in (cnt, 2 * cnt))
    hc = dict((c, W.hit_conditioning(p, y, w, c)) for c in (cnt, 2 * cnt))
    for a in (p, y, w) + tuple(r[1] for r in ref.values()):
        a.setflags(write=False)
    return p, y, w, cnt, ref, R.hits(p, y), hc


def _check(out, dp, ref, hits, hcond, tag):
    v, g, share, cond = ref
    assert out.shape == (3,)
    el = abs(float(out[0]) - v) / cond if cond > 0 else abs(float(out[0]))
    assert el <= CAP, (tag, float(out[0]), v, cond, el)
    assert float(out[1]) == float(np.float32(hits)), (tag, float(out[1]), hits)
    eh = abs(float(out[2]) - share) / hcond if hcond > 0 else abs(float(out[2]))
    assert eh <= CAP, (tag, float(out[2]), share, hcond, eh)
    eg = 0.0
    if dp is not None:
        gmax = float(np.abs(g).max())
        eg = float(np.abs(dp.astype(np.float64) - g).max()) / gmax if gmax > 0 else float(np.abs(dp).max())
        assert eg <= CAP, (tag, eg)
    return el, eg, eh


@pytest.mark.parametrize('kind', R.KINDS)
def test_kernel_parity(kind):
    from gennet_amd import ops
    worst = [0.0, 0.0, 0.0]
    for rows, cols in R.GPU_SHAPES:
        p, y, w, cnt, ref, hits, hc = _case(kind, rows, cols)
        _, pv = _inside(p, float('nan'))
        _, yv = _inside(y, float('nan'))
        _, wv = _inside(w, float('nan'))
        assert pv.data_ptr() % 16 == 4 and yv.data_ptr() % 16 == 4 and wv.data_ptr() % 16 == 4
        for count in (cnt, 2 * cnt):                                 # the local count, then the data-parallel case
            dbuf, dv = _inside(np.full((rows, cols), SENTINEL, np.float32), SENTINEL)
            dp, out = ops.loss_pass_weighted(kind, pv, yv, wv, _count(count), dp=dv)
            out = out.cpu().numpy()
            assert _untouched(dbuf, 1, rows * cols), (kind, rows, cols)
            errs = _check(out, dv.cpu().numpy(), ref[count], hits, hc[count], (kind, rows, cols, count))
            worst = [max(a, b) for a, b in zip(worst, errs)]
    print('loss_pass_weighted parity %-32s worst loss error / conditioning sum %.3e, gradient error / max|dp| %.3e, hit share error %.3e'
          % ((kind,) + tuple(worst)))


@pytest.mark.parametrize('kind', ('mean_squared_error', 'logcosh', 'categorical_crossentropy'))
def test_kernel_parity_mixed_and_aligned_phases(kind):
    """p, y, w and dp at different phases of a 16-byte line (the all-scalar path), all aligned (float4 from the first element, w as float4
    beside them at cols == 1), and w alone off the common phase (float4 for p, y, dp; scalar weights)."""
    from gennet_amd import ops
    for rows, cols in ((3, 1030), (100003, 1)):
        p, y, w, cnt, ref, hits, hc = _case(kind, rows, cols)
        for offs in ((1, 2, 3, 0), (0, 0, 0, 0), (0, 0, 1, 2)):      # (p, y, w, dp)
            _, pv = _inside(p, float('nan'), offs[0])
            _, yv = _inside(y, float('nan'), offs[1])
            _, wv = _inside(w, float('nan'), offs[2])
            dbuf, dv = _inside(np.full((rows, cols), SENTINEL, np.float32), SENTINEL, offs[3])
            _, out = ops.loss_pass_weighted(kind, pv, yv, wv, _count(cnt), dp=dv)
            assert _untouched(dbuf, offs[3], rows * cols)
            _check(out.cpu().numpy(), dv.cpu().numpy(), ref[cnt], hits, hc[cnt], (kind, rows, cols, offs))
    # w at the phase of p, y, dp with all of them one element off: the float4 body starts three elements in
    p, y, w, cnt, ref, hits, hc = _case(kind, 100003, 1)
    views = [_inside(a, float('nan'), 1)[1] for a in (p, y, w)]
    dbuf, dv = _inside(np.full((100003, 1), SENTINEL, np.float32), SENTINEL, 1)
    _, out = ops.loss_pass_weighted(kind, views[0], views[1], views[2], _count(cnt), dp=dv)
    assert _untouched(dbuf, 1, 100003)
    _check(out.cpu().numpy(), dv.cpu().numpy(), ref[cnt], hits, hc[cnt], (kind, 'common phase 1'))


@pytest.mark.parametrize('kind', R.KINDS)
def test_evaluation_form_equals_the_gradient_form(kind):
    from gennet_amd import ops
    for rows, cols in ((5, 3), (3, 1030), (100003, 1)):
        p, y, w, cnt, _, _, _ = _case(kind, rows, cols)
        _, pv = _inside(p, float('nan'))
        _, yv = _inside(y, float('nan'))
        _, wv = _inside(w, float('nan'))
        idle = torch.full((rows * cols + 8,), SENTINEL, dtype=torch.float32, device='cuda')      # handed to nobody
        c = _count(2 * cnt)
        _, with_grad = ops.loss_pass_weighted(kind, pv, yv, wv, c)
        none, without = ops.loss_pass_weighted(kind, pv, yv, wv, c, grad=False)
        assert none is None
        assert np.array_equal(with_grad.cpu().numpy().view(np.uint32), without.cpu().numpy().view(np.uint32)), (kind, rows, cols)
        assert bool((idle == SENTINEL).all())


@pytest.mark.parametrize('kind', ('mean_squared_error', 'binary_crossentropy', 'cosine_proximity', 'categorical_crossentropy'))
def test_two_runs_give_the_same_bits(kind):
    from gennet_amd import ops
    for rows, cols in ((100003, 1), (2, 70001)):
        p, y, w, cnt, _, _, _ = _case(kind, rows, cols)
        _, pv = _inside(p, float('nan'))
        _, yv = _inside(y, float('nan'))
        _, wv = _inside(w, float('nan'))
        runs = []
        for _ in range(2):
            dp, out = ops.loss_pass_weighted(kind, pv, yv, wv, ops.weight_count(wv))
            runs.append((out.cpu().numpy().view(np.uint32).copy(), dp.cpu().numpy().view(np.uint32).copy()))
        assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1]), (kind, rows, cols)


def test_weight_count_is_exact():
    from gennet_amd import ops
    for rows in (1, 257, 4096, 4097, 100003):                        # one block that writes the count itself up to 4096 rows; partials and a finish beyond
        w = W.weights(rows)
        _, wv = _inside(w, float('nan'))                             # misaligned, NaN around it (a NaN would count as non-zero)
        got = ops.weight_count(wv)
        assert got.dtype == torch.float64 and got.shape == (1,)
        assert float(got) == float(np.count_nonzero(w)), (rows, float(got), np.count_nonzero(w))
    z = torch.zeros(5000, device='cuda')
    assert float(ops.weight_count(z)) == 0.0
    z[4999] = -0.0
    assert float(ops.weight_count(z)) == 0.0                         # -0 is zero
    z[17] = -1e-30
    assert float(ops.weight_count(z)) == 1.0                         # a negative weight counts
    slot = torch.full((3,), 7.0, dtype=torch.float64, device='cuda')
    ops.weight_count(z, slot[1:2])                                   # into a caller's slot (the engine's per-output counts)
    assert slot.tolist() == [7.0, 1.0, 7.0]


@pytest.mark.parametrize('kind', ('binary_crossentropy', 'kullback_leibler_divergence', 'cosine_proximity'))
def test_zero_weight_rows_get_a_zero_gradient_that_is_written(kind):
    from gennet_amd import ops
    for rows, cols in ((300, 2), (257, 1)):
        p, y, w, cnt, _, _, _ = _case(kind, rows, cols)
        assert (w == 0).any()
        dv = torch.full((rows, cols), SENTINEL, device='cuda')
        ops.loss_pass_weighted(kind, _dev(p), _dev(y), _dev(w), _count(cnt), dp=dv)
        d = dv.cpu().numpy()
        assert np.all(d[w == 0] == 0.0) and not np.any(d == SENTINEL)


def test_all_zero_weights_give_nan_as_keras():
    from gennet_amd import ops
    for kind, (rows, cols) in (('mean_squared_error', (300, 2)), ('categorical_crossentropy', (5, 3))):
        p, y, _, _, _, hits, _ = _case(kind, rows, cols)
        w = torch.zeros(rows, device='cuda')
        _, out = ops.loss_pass_weighted(kind, _dev(p), _dev(y), w, ops.weight_count(w))
        out = out.cpu().numpy()
        assert np.isnan(out[0]) and out[1] == np.float32(hits)       # 0 / 0; the raw hit count does not depend on the weights


@pytest.mark.parametrize('kind', R.KINDS)
def test_unit_weights_agree_with_the_unweighted_pass(kind):
    from gennet_amd import ops
    for rows, cols in ((300, 2), (3, 1030), (100003, 1)):
        p, y, _, _, _, hits, _ = _case(kind, rows, cols)
        pd, yd = _dev(p), _dev(y)
        ones = torch.ones(rows, device='cuda')
        d0, o0 = ops.loss_pass(kind, pd, yd, rows)
        d1, o1 = ops.loss_pass_weighted(kind, pd, yd, ones, ops.weight_count(ones))
        o0, o1, d0, d1 = o0.cpu().numpy().astype(np.float64), o1.cpu().numpy().astype(np.float64), d0.cpu().numpy().astype(np.float64), d1.cpu().numpy()
        cond = float(np.sum(np.abs(W.row_terms(kind, p, y)))) / rows
        assert abs(o0[0] - o1[0]) <= CAP * cond and o0[1] == o1[1], (kind, rows, cols, o0, o1)
        assert abs(o1[2] - hits / float(rows * cols)) <= CAP * hits / float(rows * cols)
        gmax = np.abs(d0).max()
        assert np.abs(d1 - d0).max() <= CAP * gmax, (kind, rows, cols)


def test_bad_arguments_are_refused_before_any_launch():
    from gennet_amd import _lib, ops
    L = _lib.lib()
    rows, cols = 300, 2
    p = torch.rand(rows, cols, device='cuda')
    y = torch.rand(rows, cols, device='cuda')
    w = torch.rand(rows, device='cuda') + 0.5
    cnt = torch.full((1,), SENTINEL, dtype=torch.float64, device='cuda')
    dp = torch.full((rows, cols), SENTINEL, device='cuda')
    out = torch.full((3,), SENTINEL, device='cuda')
    need = _lib.size('gn_loss_pass_weighted_workspace', rows, cols)
    cneed = _lib.size('gn_weight_count_workspace', rows)
    assert need >= 24 and cneed >= 8
    ws = torch.zeros(need + 8, dtype=torch.uint8, device='cuda')
    assert ws.data_ptr() % 8 == 0
    s = torch.cuda.current_stream().cuda_stream
    ptr = lambda t: t.data_ptr() if t is not None else None          # noqa: E731

    def call(kind=1, pp=p, yy=y, ww=w, cc=cnt, oo=out, r=rows, c=cols, wsp=ws.data_ptr(), nbytes=need):
        return L.gn_loss_pass_weighted(kind, ptr(pp), ptr(yy), ptr(ww), ptr(cc), dp.data_ptr(), ptr(oo), r, c, wsp, nbytes, s)

    def count(ww=w, cc=cnt, r=rows, wsp=ws.data_ptr(), nbytes=cneed):
        return L.gn_weight_count(ptr(ww), r, ptr(cc), wsp, nbytes, s)

    for what, rc in (('kind', call(kind=99)), ('kind', call(kind=-1)), ('rows', call(r=0)), ('cols', call(c=0)), ('workspace', call(nbytes=need - 1)),
                     ('workspace', call(wsp=None)), ('alignment', call(wsp=ws.data_ptr() + 4)), ('p', call(pp=None)), ('y', call(yy=None)),
                     ('w', call(ww=None)), ('count', call(cc=None)), ('out', call(oo=None)),
                     ('count: w', count(ww=None)), ('count: count', count(cc=None)), ('count: rows', count(r=0)), ('count: workspace', count(nbytes=cneed - 1)),
                     ('count: workspace', count(wsp=None)), ('count: alignment', count(wsp=ws.data_ptr() + 4))):
        assert rc == -1, (what, rc)                                  # GN_EINVAL
        assert L.gn_last_error()
    torch.cuda.synchronize()
    assert bool((dp == SENTINEL).all()) and bool((out == SENTINEL).all()) and bool((cnt == SENTINEL).all())
    with pytest.raises(_lib.GennetHipError):
        ops.loss_pass_weighted(99, p, y, w, ops.weight_count(w))
    with pytest.raises(ValueError):
        ops.loss_pass_weighted(1, p, y, w[:-1].contiguous(), ops.weight_count(w))
    with pytest.raises(ValueError):
        ops.loss_pass_weighted(1, p, y, w, torch.ones(1, device='cuda'))             # a float32 count
    assert count() == 0 and call() == 0                              # and the same calls with good arguments run
    torch.cuda.synchronize()
    assert float(cnt) == float(rows) and not bool((out == SENTINEL).any()) and not bool((dp == SENTINEL).any())


# ------------------------------------------------------------------------------------------------------------------------- engine
def _dense_net(units=(8, 3), acts=('tanh', 'sigmoid'), n_in=16, seed=0):
    from gennet_amd import engine, layers
    m = engine.Sequential([layers.Dense(u, activation=a, **({'input_shape': (n_in,)} if i == 0 else {})) for i, (u, a) in enumerate(zip(units, acts))])
    rng = np.random.RandomState(seed)
    m.set_weights([(0.5 * rng.randn(*w.shape)).astype(np.float32) for w in m.get_weights()])
    return m


def _two_head_net(seed=6):
    from gennet_amd import engine, layers
    x = engine.Input(shape=(16,))
    h = layers.Dense(8, activation='tanh')(x)
    m = engine.Model(inputs=x, outputs=[layers.Dense(3, activation='sigmoid')(h), layers.Dense(1)(h)])
    rng = np.random.RandomState(seed)
    m.set_weights([(0.5 * rng.randn(*w.shape)).astype(np.float32) for w in m.get_weights()])
    return m


def _targets(kind, rng, rows, cols):
    if kind == 'binary_crossentropy':
        return rng.randint(0, 2, (rows, cols)).astype(np.float32)
    if kind == 'categorical_crossentropy':
        return np.eye(cols, dtype=np.float32)[rng.randint(0, cols, rows)]
    return rng.uniform(0.1, 0.9, (rows, cols)).astype(np.float32)


def _torch_sgd(ws, x, ys, kinds, loss_weights, sws, lr, steps, heads):
    """Plain SGD steps of the small net in torch fp64 on Keras' own weighted expression mean(l * w / mean(w != 0)) per output (None: ones);
    ws = [W1, b1, (Wk, bk) per head]; heads = activation per head."""
    ws = [torch.tensor(w, dtype=torch.float64, requires_grad=True) for w in ws]
    xt = torch.tensor(x, dtype=torch.float64)
    rows = x.shape[0]
    hist = []
    lr = float(np.float32(lr))
    for _ in range(steps):
        h = torch.tanh(xt @ ws[0] + ws[1])
        per = []
        for k, (kind, act) in enumerate(zip(kinds, heads)):
            o = h @ ws[2 + 2 * k] + ws[3 + 2 * k]
            o = torch.sigmoid(o) if act == 'sigmoid' else o
            yt = torch.tensor(ys[k], dtype=torch.float64)
            l = torch.stack([R.torch_value(kind, o[r:r + 1], yt[r:r + 1], 1) for r in range(rows)])
            wt = torch.ones(rows, dtype=torch.float64) if sws[k] is None else torch.tensor(sws[k], dtype=torch.float64)
            per.append(torch.mean(l * wt / torch.mean((wt != 0).to(torch.float64))))
        total = sum(w * l for w, l in zip(loss_weights, per))
        for w in ws:
            w.grad = None
        total.backward()
        with torch.no_grad():
            for w in ws:
                w -= lr * w.grad
        hist.append([float(total.detach())] + [float(l.detach()) for l in per])
    return hist, [w.detach().numpy() for w in ws]


@pytest.mark.parametrize('kind,cols', (('binary_crossentropy', 1), ('logcosh', 3), ('categorical_crossentropy', 3)))
def test_weighted_training_matches_torch_autograd(kind, cols):
    """Three SGD steps under sample weights (zeros and a negative one among them); at the (12, 1) binary_crossentropy head the unweighted call
    runs the one-block kernel, the weighted one the pass."""
    from gennet_amd import engine
    rng = np.random.RandomState(5)
    m = _dense_net(units=(8, cols), seed=4).compile(loss=kind, optimizer=engine.SGD(lr=0.1))
    w0 = m.get_weights()
    x, y = rng.randn(12, 16).astype(np.float32), _targets(kind, rng, 12, cols)
    sw = SW12
    got = [m.train_on_batch(x, y, sample_weight=sw) for _ in range(3)]
    hist, wref = _torch_sgd(w0, x, [y], [kind], [1.0], [sw], 0.1, 3, ['sigmoid'])
    for g, h in zip(got, hist):
        assert len(g) == 1 and abs(g[0] - h[0]) <= 1e-5 * max(1.0, abs(h[0])), (kind, got, hist)
    for a, b in zip(m.get_weights(), wref):
        assert np.abs(a - b).max() <= 1e-5, (kind, np.abs(a - b).max())


def test_class_weight_is_the_equivalent_sample_weight_bit_for_bit():
    from gennet_amd import engine
    rng = np.random.RandomState(6)
    x = rng.randn(12, 16).astype(np.float32)
    labels = rng.randint(0, 3, 12)
    y = np.eye(3, dtype=np.float32)[labels]
    cw = {0: 0.5, 1: 0.0, 2: 3.0}
    a = _dense_net(seed=4).compile(loss='categorical_crossentropy', optimizer=engine.SGD(lr=0.1), metrics=['accuracy'])
    b = _dense_net(seed=4).compile(loss='categorical_crossentropy', optimizer=engine.SGD(lr=0.1), metrics=['accuracy'])
    ra = [a.train_on_batch(x, y, class_weight=cw) for _ in range(2)]
    rb = [b.train_on_batch(x, y, sample_weight=np.array([cw[int(c)] for c in labels], np.float32)) for _ in range(2)]
    assert ra == rb and all(np.array_equal(u, v) for u, v in zip(a.get_weights(), b.get_weights()))
    c = _dense_net(seed=4).compile(loss='categorical_crossentropy', optimizer=engine.SGD(lr=0.1), metrics=['accuracy'])
    assert c.train_on_batch(x, y) != ra[0]                           # and it is not the unweighted step
    # a (B, 1) target: the class is the value itself
    h1 = _dense_net(units=(8, 1), seed=4).compile(loss='binary_crossentropy', optimizer=engine.SGD(lr=0.1))
    h2 = _dense_net(units=(8, 1), seed=4).compile(loss='binary_crossentropy', optimizer=engine.SGD(lr=0.1))
    yb = rng.randint(0, 2, (12, 1)).astype(np.float32)
    assert h1.train_on_batch(x, yb, class_weight={0: 0.25, 1: 2.0}) == h2.train_on_batch(x, yb, sample_weight=np.where(yb[:, 0] == 1, 2.0, 0.25))
    assert all(np.array_equal(u, v) for u, v in zip(h1.get_weights(), h2.get_weights()))


def test_two_outputs_one_weighted_with_loss_weights():
    from gennet_amd import engine
    rng = np.random.RandomState(7)
    kinds, lw = ['logcosh', 'mean_squared_error'], [0.25, 2.0]
    m = _two_head_net().compile(loss=kinds, optimizer=engine.SGD(lr=0.1), loss_weights=lw)
    w0 = m.get_weights()
    x = rng.randn(12, 16).astype(np.float32)
    ys = [_targets('logcosh', rng, 12, 3), rng.randn(12, 1).astype(np.float32)]
    sw = W.weights(12, seed=3)
    got = [m.train_on_batch(x, ys, sample_weight=[sw, None]) for _ in range(3)]
    hist, wref = _torch_sgd(w0, x, ys, kinds, lw, [sw, None], 0.1, 3, ['sigmoid', 'linear'])
    for g, h in zip(got, hist):
        assert len(g) == 3
        assert g[0] == pytest.approx(0.25 * g[1] + 2.0 * g[2], rel=1e-12)
        assert np.abs(np.asarray(g) - np.asarray(h)).max() <= 1e-5 * max(1.0, abs(h[0])), (got, hist)
    for a, b in zip(m.get_weights(), wref):
        assert np.abs(a - b).max() <= 1e-5, np.abs(a - b).max()


def _state(m):
    return [w.copy() for w in m.get_weights()] + [np.array(a).copy() for a in m.optimizer.get_keras_weights(m._keras_train_order())]


def test_metrics_stay_unweighted_weighted_metrics_are_weighted_and_nothing_changes():
    from gennet_amd import engine
    rng = np.random.RandomState(8)
    m = _dense_net(seed=9).compile(loss='logcosh', optimizer=engine.Adam(lr=1e-2), metrics=['accuracy', 'mae'], weighted_metrics=['accuracy', 'mae'])
    assert m.metrics_names == ['loss', 'acc', 'mean_absolute_error', 'weighted_acc', 'weighted_mean_absolute_error']
    x, y = rng.randn(24, 16).astype(np.float32), rng.randint(0, 2, (24, 3)).astype(np.float32)
    sw = W.weights(24, seed=4)
    cnt = np.count_nonzero(sw)
    m.train_on_batch(x, y, sample_weight=sw)
    m.train_on_batch(x, y)
    before = _state(m)
    res = m.test_on_batch(x, y, sample_weight=sw)
    plain = m.test_on_batch(x, y)
    after = _state(m)
    assert len(before) == len(after) and all(np.array_equal(a, b) for a, b in zip(before, after))         # test_on_batch changes nothing
    pred = m.predict_on_batch(x)
    v, _, share, cond = W.weighted_value_and_grad('logcosh', pred, y, sw, cnt)
    assert len(res) == 5
    assert abs(res[0] - v) <= CAP * cond, (res[0], v)
    assert res[1] == R.metric('accuracy', pred, y)                                                          # metrics= ignore the weights (Keras 2.2.4)
    assert abs(res[2] - R.metric('mae', pred, y)) <= CAP * res[2]
    assert abs(res[3] - share) <= CAP * W.hit_conditioning(pred, y, sw, cnt) and share == pytest.approx(W.keras_metric('accuracy', pred, y, sw), rel=1e-13)
    mae_cond = float(np.sum(np.abs(sw.astype(np.float64) * W.row_terms('mae', pred, y)))) / cnt
    assert abs(res[4] - W.keras_metric('mae', pred, y, sw)) <= CAP * mae_cond
    assert res[3] != res[1] and res[4] != res[2]
    # without weights the weights are ones: each weighted metric is its plain one
    assert plain[1:3] == res[1:3] and plain[3] == pytest.approx(plain[1], rel=2e-7) and plain[4] == plain[2]
    assert abs(plain[0] - R.value_and_grad('logcosh', pred, y)[0]) <= CAP * plain[0]


def test_evaluate_takes_each_chunk_by_its_own_count():
    from gennet_amd import engine
    rng = np.random.RandomState(9)
    m = _dense_net(seed=10).compile(loss='mean_squared_error', optimizer=engine.SGD(lr=0.1), weighted_metrics=['mae'])
    x, y = rng.randn(70, 16).astype(np.float32), rng.uniform(0, 1, (70, 3)).astype(np.float32)
    sw = W.weights(70, seed=5)
    counts = [np.count_nonzero(sw[s:s + 32]) for s in (0, 32, 64)]
    assert len(set(c / float(n) for c, n in zip(counts, (32, 32, 6)))) > 1       # the chunks' non-zero fractions differ: one global count would show
    want, tol = np.zeros(2), np.zeros(2)
    for s, c in zip((0, 32, 64), counts):
        xs, ysl, ws = x[s:s + 32], y[s:s + 32], sw[s:s + 32]
        pred = m.predict_on_batch(xs)
        v, _, _, cond = W.weighted_value_and_grad('mean_squared_error', pred, ysl, ws, c)
        mv = W.keras_metric('mae', pred, ysl, ws)
        mc = float(np.sum(np.abs(ws.astype(np.float64) * W.row_terms('mae', pred, ysl)))) / c
        want += np.array([v, mv]) * len(xs) / 70.0
        tol += CAP * np.array([cond, mc]) * len(xs) / 70.0
    got = m.evaluate(x, y, batch_size=32, sample_weight=sw)
    assert m.metrics_names == ['loss', 'weighted_mean_absolute_error'] and len(got) == 2
    assert np.all(np.abs(np.asarray(got) - want) <= tol), (got, want, tol)
    parts = [np.asarray(m.test_on_batch(x[s:s + 32], y[s:s + 32], sample_weight=sw[s:s + 32])) * len(x[s:s + 32]) for s in (0, 32, 64)]
    assert np.allclose(got, (parts[0] + parts[1] + parts[2]) / 70.0, rtol=1e-12, atol=0)
    with pytest.raises(ValueError):
        m.evaluate(x, y, batch_size=32, sample_weight=sw[:69])


def test_fit_shuffles_the_weights_and_validates():
    from gennet_amd import engine
    rng = np.random.RandomState(10)
    x, y = rng.randn(40, 16).astype(np.float32), rng.uniform(0, 1, (40, 3)).astype(np.float32)
    vx, vy, vw = rng.randn(20, 16).astype(np.float32), rng.uniform(0, 1, (20, 3)).astype(np.float32), W.weights(20, seed=6)
    sw = W.weights(40, seed=7)

    def make():
        return _dense_net(seed=11).compile(loss='logcosh', optimizer=engine.SGD(lr=0.1), metrics=['mae'])

    a = make()
    hist = a.fit(x, y, batch_size=16, epochs=2, sample_weight=sw, validation_data=(vx, vy, vw))
    assert sorted(hist) == ['loss', 'val_loss', 'val_mean_absolute_error'] and all(len(v) == 2 for v in hist.values())
    assert hist['val_loss'][-1] == a.evaluate(vx, vy, batch_size=16, sample_weight=vw)[0]
    # the same epochs by hand: fit's own permutations, the weights permuted with the rows
    b = make()
    order = np.random.RandomState(0)
    for ep in range(2):
        idx = order.permutation(40)
        tot = sum(b.train_on_batch(x[idx[s:s + 16]], y[idx[s:s + 16]], sample_weight=sw[idx[s:s + 16]])[0] * len(idx[s:s + 16]) for s in (0, 16, 32))
        assert hist['loss'][ep] == tot / 40.0
    assert all(np.array_equal(u, v) for u, v in zip(a.get_weights(), b.get_weights()))
    c = make()
    h2 = c.fit(x, y, batch_size=16, epochs=1, validation_data=(vx, vy))
    assert sorted(h2) == ['loss', 'val_loss', 'val_mean_absolute_error'] and h2['val_loss'][0] == c.evaluate(vx, vy, batch_size=16)[0]
    assert sorted(make().fit(x, y, batch_size=16, epochs=1)) == ['loss']                                   # without validation_data: as before
    assert h2['loss'] != hist['loss'][:1]                             # sample_weight is no longer swallowed


def test_routing_weighted_calls_take_the_weighted_pass(monkeypatch):
    from gennet_amd import engine, ops
    calls = []
    for name in ('loss', 'loss_pass', 'loss_pass_weighted'):
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _n=name, _r=real, **k: calls.append((_n, a[0])) or _r(*a, **k))
    rng = np.random.RandomState(11)
    m = _dense_net(units=(8, 1), seed=12).compile(loss='binary_crossentropy', optimizer=engine.SGD(lr=0.01))
    x, y = rng.randn(12, 16).astype(np.float32), rng.randint(0, 2, (12, 1)).astype(np.float32)
    m.train_on_batch(x, y, sample_weight=W.weights(12))
    assert calls == [('loss_pass_weighted', 'binary_crossentropy')]  # never the one-block kernel, which has no weighted form
    del calls[:]
    m.train_on_batch(x, y)
    assert calls == [('loss', 'binary_crossentropy')]                # the unweighted call on the same model: the kernel it always ran
    del calls[:]
    m.test_on_batch(x, y, sample_weight=W.weights(12))
    assert calls == [('loss_pass_weighted', 'binary_crossentropy')]


def test_captured_step_replays_with_new_weights():
    from gennet_amd import engine, ops
    rng = np.random.RandomState(13)
    x, y = rng.randn(12, 16).astype(np.float32), rng.uniform(0, 1, (12, 3)).astype(np.float32)
    sws = [W.weights(12, seed=k) for k in (20, 21, 22, 23)]
    assert len(set(int(np.count_nonzero(w)) for w in sws)) > 1       # the count changes between replays: it cannot be a frozen argument

    def make():
        return _dense_net(seed=14).compile(loss='logcosh', optimizer=engine.Adam(lr=1e-2), metrics=['accuracy'], weighted_metrics=['accuracy', 'mae'])

    a = make()
    eager = [a.train_on_batch(x, y, sample_weight=w) for w in sws]
    b = make()
    xd, yd, wd = engine.to_device(x), engine.to_device(y), engine.to_device(sws[0])
    got = [b.train_result(b.train_on_batch_device([xd], [yd], sample_weights=[wd]), 12)]          # binds the optimizer state
    sg = engine.StepGraph()
    torch.cuda.synchronize()
    sg.capture(lambda: b.train_on_batch_device([xd], [yd], sample_weights=[wd]))
    key = (xd.device.type, xd.device.index)
    held = ops._ws[key]
    assert any(buf is held for buf in sg.scratch)                    # the graph holds the workspace it was handed ...
    ops.workspace(held.numel() + 1, xd.device)
    assert ops._ws[key] is not held                                  # ... also after a larger request has replaced it
    for w in sws[1:]:
        sg.wait_inputs_consumed()
        wd.copy_(torch.from_numpy(w))                                # the static weight tensor, overwritten between replays
        got.append(b.train_result(sg.replay(), 12))
    assert len(eager[0]) == 4 and got == eager                       # loss, accuracy and both weighted metrics, bit for bit
    assert all(np.array_equal(u, v) for u, v in zip(a.get_weights(), b.get_weights()))


def test_save_and_load_keep_weighted_metrics(tmp_path):
    from gennet_amd import engine
    rng = np.random.RandomState(12)
    x = rng.randn(12, 16).astype(np.float32)
    ys = [_targets('logcosh', rng, 12, 3), rng.randn(12, 1).astype(np.float32)]
    sw = [W.weights(12, seed=8), W.weights(12, seed=9)]
    m = _two_head_net().compile(loss=['logcosh', 'mse'], optimizer=engine.Adam(lr=1e-2), metrics=['mae'], weighted_metrics=['accuracy', 'mae'],
                                loss_weights=[0.25, 2.0])
    m.train_on_batch(x, ys, sample_weight=sw)
    path = str(tmp_path / 'model.h5')
    m.save(path)
    back = engine.load_model(path)
    assert back.weighted_metrics == ['accuracy', 'mae'] and back.metrics == ['mae'] and back.loss_weights == [0.25, 2.0]
    assert back.metrics_names == m.metrics_names and len(m.metrics_names) == 9
    assert back.train_on_batch(x, ys, sample_weight=sw) == m.train_on_batch(x, ys, sample_weight=sw)
    assert all(np.array_equal(u, v) for u, v in zip(back.get_weights(), m.get_weights()))


# ------------------------------------------------------------------------------------------------------------------ data parallel
WORKER = os.path.join(ROOT, 'tests', 'sample_weight_dp_worker.py')


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _launch(out, world):
    """As tests/test_dist.py starts its `gpu` mode: the worker directly for one rank, torch.distributed.run for more."""
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


def test_two_ranks_equal_one_rank_under_sample_weights(tmp_path):
    """2 ranks x B / 2 rows against 1 rank x B rows, rank 1's rows all of weight zero and rank 0's mixed: a LOCAL count would divide rank
    1's sums by zero.  Losses to 1e-5; weights to the tolerance tests/test_dist.py documents (1e-4 relative + 2 % of the Adam step budget);
    a weighted step makes exactly one all-reduce more than an unweighted one."""
    one = _launch(str(tmp_path / 'one'), 1)[0]
    two = _launch(str(tmp_path / 'two'), 2)
    for r in two:
        assert len(r['losses']) == len(one['losses'])
        for a, b in zip(r['losses'], one['losses']):
            assert len(a) == len(b)
            for u, v in zip(a, b):
                assert np.isfinite(u) and abs(u - v) <= 1e-5 * abs(v) + 1e-7, (r['losses'], one['losses'])
        for w, wr in zip(r['weights'], one['weights']):
            assert np.isfinite(w).all()
            assert np.abs(w - wr).max() <= 1e-4 * np.abs(wr).max() + 0.02 * 2 * 9e-5, (w.shape, float(np.abs(w - wr).max()))
        assert r['calls_weighted'] == r['calls_unweighted'] + 1, (r['calls_weighted'], r['calls_unweighted'])
    assert all(np.array_equal(u, v) for u, v in zip(two[0]['weights'], two[1]['weights']))               # replicas stay bit-identical
