"""Keras sample_weight / class_weight / weighted_metrics, CPU only: the fp64 restatement tests/loss_weight_ref.py against torch fp64 autograd
of Keras' own expression mean(l * w / mean(w != 0)) and against the unweighted restatement at w = 1, its vectorised per-row terms against
one-row slices, the weight generator, and the host logic of the public surface (standardisation and its errors, class_weight, metrics_names,
the .h5 training_config, header and library symbols)."""
import json
import os
import warnings

import numpy as np
import pytest
import torch

import loss_ref as R
import loss_weight_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((5, 3), (7, 1))


def _keras_expression(kind, p, y, w):
    """weighted_masked_objective of Keras 2.2.4 in torch fp64: score = l * w; score /= mean(w != 0); mean(score)."""
    l = torch.stack([R.torch_value(kind, p[r:r + 1], y[r:r + 1], 1) for r in range(p.shape[0])])
    return torch.mean(l * w / torch.mean((w != 0).to(torch.float64)))


@pytest.mark.parametrize('kind', R.LOSSES)
@pytest.mark.parametrize('shape', SHAPES)
def test_restatement_is_keras_expression(kind, shape):
    rows, cols = shape
    p32, y32 = R.generate(kind, rows, cols, seed=3)
    w32 = W.weights(rows, seed=5)
    assert np.count_nonzero(w32) < rows or rows < 4                  # a zero weight is among them: the batch size does NOT cancel against rows
    count = np.count_nonzero(w32)
    v, g, _, cond = W.weighted_value_and_grad(kind, p32, y32, w32, count)
    tp = torch.tensor(p32.astype(np.float64), requires_grad=True)
    tv = _keras_expression(kind, tp, torch.tensor(y32.astype(np.float64)), torch.tensor(w32.astype(np.float64)))
    tv.backward()
    assert abs(float(tv.detach()) - v) <= 1e-7 * max(1.0, abs(v)), (kind, float(tv.detach()), v)
    scale = max(1.0, float(np.abs(g).max()))
    assert np.abs(tp.grad.numpy() - g).max() <= 1e-7 * scale, (kind, np.abs(tp.grad.numpy() - g).max())
    assert cond >= abs(v) - 1e-12
    # twice the count (the data-parallel case: as many non-zero weights again on another rank) halves everything
    v2, g2, s2, c2 = W.weighted_value_and_grad(kind, p32, y32, w32, 2 * count)
    assert v2 == pytest.approx(v / 2, rel=1e-15) and np.allclose(g2, g / 2, rtol=1e-15, atol=0)


@pytest.mark.parametrize('kind', R.KINDS)
def test_unit_weights_give_the_unweighted_restatement(kind):
    for rows, cols in SHAPES + ((300, 2),):
        p, y = R.generate(kind, rows, cols, seed=1)
        for denom in (rows, 2 * rows):
            v, g, share, cond = W.weighted_value_and_grad(kind, p, y, np.ones(rows, np.float32), denom)
            v0, g0 = R.value_and_grad(kind, p, y, denom)
            assert v == pytest.approx(v0, rel=1e-13, abs=1e-15) and np.allclose(g, g0, rtol=1e-13, atol=1e-300)
            assert share == pytest.approx(R.hits(p, y) / float(denom * cols), rel=1e-13)


@pytest.mark.parametrize('kind', R.KINDS)
def test_vectorised_row_terms_are_the_one_row_slices(kind):
    for rows, cols in SHAPES + ((300, 2), (3, 1030)):
        p, y = R.generate(kind, rows, cols, seed=2)
        a, b = W.row_terms(kind, p, y), W.row_terms_by_slices(kind, p, y)
        assert a.shape == (rows,) and np.allclose(a, b, rtol=1e-13, atol=1e-15), (kind, rows, cols)
    p = np.array([[0.4, 1.5, 2.5], [0.6, 0.5, 7.0]], np.float32)
    y = np.array([[0.0, 2.0, 2.0], [1.0, 1.0, 7.0]], np.float32)
    assert W.row_hits(p, y).tolist() == [3.0, 2.0]                   # round half to even, as rintf


def test_weight_generator():
    for rows in (1, 2, 5, 257, 100003):
        w = W.weights(rows)
        assert w.dtype == np.float32 and w.shape == (rows,) and np.any(w != 0)
        nz = np.abs(w[w != 0])
        assert nz.min() >= 0.25 and nz.max() <= 4.0
        assert np.array_equal(w, W.weights(rows))                    # seeded
    w = W.weights(100003)
    assert 0.2 <= np.mean(w == 0) <= 0.3 and 0.1 <= np.mean(w < 0) <= 0.2


def test_negative_weights_count_and_all_zero_is_nan():
    p, y = R.generate('mean_squared_error', 4, 2)
    w = np.array([-2.0, 0.0, 1.0, 0.0], np.float32)
    v, g, share, cond = W.weighted_value_and_grad('mean_squared_error', p, y, w, 2)
    l = W.row_terms('mean_squared_error', p, y)
    assert v == pytest.approx((-2.0 * l[0] + l[2]) / 2.0) and cond == pytest.approx((2.0 * l[0] + l[2]) / 2.0)
    assert np.all(g[1] == 0) and np.all(g[3] == 0)
    v, g, share, cond = W.weighted_value_and_grad('mean_squared_error', p, y, np.zeros(4, np.float32), 0)
    assert np.isnan(v)                                               # 0 / 0, as Keras


# ----------------------------------------------------------------------------------------------------------------- host logic
def _one_output(units=3):
    from gennet_amd import engine, layers
    return engine.Sequential([layers.Dense(units, input_shape=(4,))])


def _two_outputs():
    from gennet_amd import engine, layers
    x = engine.Input(shape=(4,))
    return engine.Model(inputs=x, outputs=[layers.Dense(3)(x), layers.Dense(1)(x)])


def test_standardise_sample_weight():
    one, two = _one_output().compile(loss='mse', optimizer='sgd'), _two_outputs().compile(loss='mse', optimizer='sgd')
    y = np.zeros((5, 3), np.float32)
    assert one._prep_weights(None, None, y, 5) is None
    w = [1.0, 0.0, -2.0, 0.5, 4.0]
    got = one._prep_weights(w, None, y, 5)
    assert len(got) == 1 and got[0].dtype == np.float32 and got[0].tolist() == w
    assert one._prep_weights([np.asarray(w)], None, y, 5)[0].tolist() == w          # a list with the one output's entry
    got = two._prep_weights([np.asarray(w), None], None, [y, y[:, :1]], 5)
    assert got[0].tolist() == w and got[1] is None
    assert two._prep_weights([None, None], None, [y, y[:, :1]], 5) is None          # nothing weighted: today's path
    with pytest.raises(NotImplementedError):
        one._prep_weights({'dense': w}, None, y, 5)
    with pytest.raises(ValueError):
        one._prep_weights(w[:4], None, y, 5)                         # wrong length
    with pytest.raises(ValueError):
        one._prep_weights(np.ones((5, 1)), None, y, 5)               # wrong rank
    with pytest.raises(ValueError):
        one._prep_weights(np.float32(2.0), None, y, 5)
    with pytest.raises(ValueError):
        two._prep_weights(np.asarray(w), None, [y, y[:, :1]], 5)     # not a list on a two-output model
    with pytest.raises(ValueError):
        two._prep_weights([np.asarray(w)], None, [y, y[:, :1]], 5)


def test_class_weight_becomes_sample_weight():
    one = _one_output().compile(loss='categorical_crossentropy', optimizer='sgd')
    y = np.eye(3, dtype=np.float32)[[2, 0, 1, 2, 2]]
    got = one._prep_weights(None, {0: 0.5, 1: 2.0, 2: 0.0}, y, 5)
    assert len(got) == 1 and got[0].dtype == np.float32 and got[0].tolist() == [0.0, 0.5, 2.0, 0.0, 0.0]          # argmax of the row
    head = _one_output(1).compile(loss='binary_crossentropy', optimizer='sgd')
    got = head._prep_weights(None, {0: 0.25, 1: 3.0}, np.array([[1.0], [0.0], [0.0], [1.0]], np.float32), 4)
    assert got[0].tolist() == [3.0, 0.25, 0.25, 3.0]                                                              # y[:, 0] itself
    assert head._prep_weights(None, {0: 0.25, 1: 3.0}, np.array([1.0, 0.0, 0.0, 1.0]), 4)[0].tolist() == [3.0, 0.25, 0.25, 3.0]
    with pytest.raises(ValueError) as e:
        one._prep_weights(None, {0: 0.5, 2: 1.0}, y, 5)              # class 1 has no entry
    assert '1' in str(e.value)
    with pytest.raises(ValueError):
        _two_outputs().compile(loss='mse', optimizer='sgd')._prep_weights(None, {0: 1.0}, [y, y[:, :1]], 5)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        got = one._prep_weights(np.arange(5.0), {0: 0.5, 1: 2.0, 2: 0.0}, y, 5)
    assert got[0].tolist() == [0.0, 1.0, 2.0, 3.0, 4.0]              # sample_weight wins
    assert any(issubclass(r.category, UserWarning) and 'class_weight' in str(r.message) for r in rec)


def test_public_signatures_take_the_weights():
    import inspect
    from gennet_amd import engine
    for fn, names in ((engine.Model.train_on_batch, ('sample_weight', 'class_weight')), (engine.Model.test_on_batch, ('sample_weight',)),
                      (engine.Model.evaluate, ('sample_weight',)), (engine.Model.fit, ('sample_weight', 'class_weight', 'validation_data')),
                      (engine.Model.train_on_batch_device, ('sample_weights',)), (engine.Model.test_on_batch_device, ('sample_weights',)),
                      (engine.Model.compile, ('weighted_metrics', 'sample_weight_mode'))):
        ps = inspect.signature(fn).parameters
        assert all(n in ps and ps[n].default is None for n in names), (fn.__name__, names)
    assert list(inspect.signature(engine.Model.evaluate).parameters)[1:6] == ['x', 'y', 'batch_size', 'verbose', 'sample_weight']


def test_compile_weighted_metrics_and_sample_weight_mode():
    from gennet_amd import keras
    one, two = _one_output(), _two_outputs()
    m = one.compile(loss='mse', optimizer='sgd', metrics=['accuracy', 'mae'], weighted_metrics=['accuracy', 'mae'])
    assert m.weighted_metrics == ['accuracy', 'mae']
    assert m.metrics_names == ['loss', 'acc', 'mean_absolute_error', 'weighted_acc', 'weighted_mean_absolute_error']
    assert one.compile(loss='mse', optimizer='sgd', weighted_metrics=['acc']).metrics_names == ['loss', 'weighted_acc']
    assert one.compile(loss='mse', optimizer='sgd', weighted_metrics=['mape', keras.metrics.categorical_accuracy]).metrics_names == [
        'loss', 'weighted_mean_absolute_percentage_error', 'weighted_categorical_accuracy']
    assert two.compile(loss='mse', optimizer='sgd', metrics=['accuracy'], weighted_metrics=['accuracy', 'mae']).metrics_names == [
        'loss', 'out0_loss', 'out1_loss', 'out0_acc', 'out0_weighted_acc', 'out0_weighted_mean_absolute_error',
        'out1_acc', 'out1_weighted_acc', 'out1_weighted_mean_absolute_error']
    m = one.compile(loss='mse', optimizer='sgd', metrics=['accuracy'])           # compiling again without them drops them
    assert m.weighted_metrics == [] and m.metrics_names == ['loss', 'acc']
    with pytest.raises(NotImplementedError):
        one.compile(loss='mse', optimizer='sgd', weighted_metrics=['hinge'])
    with pytest.raises(NotImplementedError):
        one.compile(loss='mse', optimizer='sgd', sample_weight_mode='temporal')
    with pytest.raises(NotImplementedError):
        one.compile(loss='mse', optimizer='sgd', sample_weight_mode='anything')
    one.compile(loss='mse', optimizer='sgd', sample_weight_mode=None, target_tensors=None, some_future_keyword=1)    # any other keyword: accepted as before


def test_training_config_keeps_weighted_metrics_and_stays_byte_identical_without(tmp_path):
    from gennet_amd import engine, h5lite
    path = str(tmp_path / 'm.h5')
    m = _one_output().compile(loss='mse', optimizer='sgd', metrics=['accuracy'])
    m.save(path)
    raw = h5lite.File(path).attrs['training_config']
    raw = raw if isinstance(raw, bytes) else raw.encode('utf-8')
    want = json.dumps({'optimizer_config': {'class_name': 'SGD', 'config': m.optimizer.get_config()}, 'loss': 'mse', 'metrics': ['accuracy'],
                       'sample_weight_mode': None, 'loss_weights': None}).encode('utf-8')
    assert raw == want                                               # the record of a model compiled with the earlier arguments: its bytes
    assert b'weighted_metrics' not in raw
    assert engine.load_model(path).weighted_metrics == []
    m = _two_outputs().compile(loss=['logcosh', 'mae'], optimizer='sgd', metrics=['mae'], weighted_metrics=['accuracy', 'mse'])
    m.save(path)
    tc = h5lite.File(path).attrs['training_config']
    tc = json.loads(tc.decode('utf-8') if isinstance(tc, bytes) else tc)
    assert tc['weighted_metrics'] == ['accuracy', 'mse'] and tc['metrics'] == ['mae']
    back = engine.load_model(path)
    assert back.weighted_metrics == ['accuracy', 'mse'] and back.metrics == ['mae'] and back.metrics_names == m.metrics_names


def test_header_declares_and_library_exports_the_weighted_pass():
    from gennet_amd import _lib, ops
    text = open(os.path.join(ROOT, 'include', 'gennet_hip.h')).read()
    for sym in ('gn_weight_count', 'gn_weight_count_workspace', 'gn_loss_pass_weighted', 'gn_loss_pass_weighted_workspace'):
        assert sym + '(' in text and sym in _lib.exported_symbols()
        assert hasattr(_lib.lib(), sym), sym
    assert callable(ops.weight_count) and callable(ops.loss_pass_weighted)
    # three fp64 partials per block against two; the count's partials are one 64-bit integer per block of 4096 rows at the most
    for rows, cols in R.GPU_SHAPES:
        assert _lib.size('gn_loss_pass_weighted_workspace', rows, cols) * 2 == _lib.size('gn_loss_pass_workspace', rows, cols) * 3
        assert 8 <= _lib.size('gn_weight_count_workspace', rows) <= 8 * (rows // 4096 + 1)
    assert _lib.size('gn_weight_count_workspace', 0) == 0 and _lib.size('gn_loss_pass_weighted_workspace', 0, 3) == 0
