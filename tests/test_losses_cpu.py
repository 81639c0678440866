"""Keras losses and metrics beyond binary_crossentropy / mean_squared_error, CPU only: the fp64 restatement tests/loss_ref.py against central
finite differences and torch fp64 autograd of the same expressions, the tie and clip conventions on hand-written inputs, the generators of
the GPU parity test against their bounds, and the public surface (compile names, aliases and facade callables, loss_weights, metrics_names,
test_on_batch / evaluate / predict_on_batch, header and library symbols)."""
import os

import numpy as np
import pytest
import torch

import loss_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((5, 3), (4, 1))
GPU_SHAPES = R.GPU_SHAPES


@pytest.mark.parametrize('kind', R.LOSSES)
@pytest.mark.parametrize('shape', SHAPES)
def test_reference_gradient_is_the_derivative(kind, shape):
    """loss_ref's gradient against central finite differences of loss_ref's own value, and value and gradient against torch fp64 autograd of
    the same expression: 1e-7 of the gradient's scale (the inputs keep 1e-2 from every kink and clip bound, so both are smooth there)."""
    rows, cols = shape
    p32, y32 = R.generate(kind, rows, cols, seed=3)
    p, y = p32.astype(np.float64), y32.astype(np.float64)
    denom = 2 * rows
    v, g = R.value_and_grad(kind, p, y, denom)
    scale = max(1.0, float(np.abs(g).max()))
    h = 1e-5
    fd = np.zeros_like(p)
    for i in range(rows):
        for j in range(cols):
            a, b = p.copy(), p.copy()
            a[i, j] += h
            b[i, j] -= h
            fd[i, j] = (R.value_and_grad(kind, a, y, denom)[0] - R.value_and_grad(kind, b, y, denom)[0]) / (2 * h)
    assert np.abs(fd - g).max() <= 1e-7 * scale, (kind, np.abs(fd - g).max())
    tp = torch.tensor(p, dtype=torch.float64, requires_grad=True)
    tv = R.torch_value(kind, tp, torch.tensor(y, dtype=torch.float64), denom)
    tv.backward()
    tv = tv.detach()
    assert abs(float(tv) - v) <= 1e-7 * max(1.0, abs(v)), (kind, float(tv), v)
    assert np.abs(tp.grad.numpy() - g).max() <= 1e-7 * scale, (kind, np.abs(tp.grad.numpy() - g).max())


@pytest.mark.parametrize('case', R.tie_cases(), ids=lambda c: c[0])
def test_tie_and_clip_conventions(case):
    kind, p, y, want = case
    _, g = R.value_and_grad(kind, np.asarray(p, np.float32), np.asarray(y, np.float32), 1)
    assert np.array_equal(g, np.asarray(want, np.float64)), (kind, g, want)


def test_categorical_accuracy_takes_the_first_maximum():
    p = np.array([[0.5, 0.5, 0.1], [0.1, 0.7, 0.7], [0.3, 0.2, 0.1]], np.float32)
    y = np.array([[1, 0, 0], [0, 0, 1], [1, 1, 0]], np.float32)
    assert R.value_and_grad('categorical_accuracy', p, y, 3)[0] == pytest.approx(2.0 / 3.0)
    assert R.hits(np.array([[0.5, 1.5, 2.5, 0.4]]), np.array([[0, 2, 2, 1]])) == 3        # round half to even, as rintf


@pytest.mark.parametrize('kind', R.KINDS)
def test_generated_inputs_stay_inside_their_bounds(kind):
    for rows, cols in GPU_SHAPES + SHAPES:
        p, y = R.generate(kind, rows, cols)
        assert p.dtype == np.float32 and y.dtype == np.float32 and p.shape == y.shape == (rows, cols)
        assert np.isfinite(p).all() and np.isfinite(y).all()
        assert R.bounds_ok(kind, p, y), (kind, rows, cols)
        v, g = R.value_and_grad(kind, p, y, 2 * rows)
        assert np.isfinite(v) and np.isfinite(g).all()


# ----------------------------------------------------------------------------------------------------------------- public surface
def _one_output():
    from gennet_amd import engine, layers
    return engine.Sequential([layers.Dense(3, input_shape=(4,))])


def _two_outputs():
    from gennet_amd import engine, layers
    x = engine.Input(shape=(4,))
    return engine.Model(inputs=x, outputs=[layers.Dense(3)(x), layers.Dense(1)(x)])


def test_compile_accepts_logcosh():
    m = _one_output()
    m.compile(loss='logcosh', optimizer='sgd')                       # NotImplementedError before this feature
    assert m.loss == 'logcosh' and m._losses == ['logcosh']


def test_model_has_test_on_batch_evaluate_predict_on_batch():
    m = _one_output()
    assert callable(m.test_on_batch) and callable(m.evaluate) and callable(m.predict_on_batch)     # AttributeError before this feature


def test_compile_accepts_every_name_alias_and_callable():
    from gennet_amd import engine, keras, ops
    assert set(engine.LOSSES) == set(R.LOSSES) and R.ALIASES == ops.LOSS_ALIASES
    for name in R.LOSSES:
        m = _one_output().compile(loss=name, optimizer='sgd')
        assert m._losses == [name] and m.loss == name
        fn = getattr(keras.losses, name)
        m = _one_output().compile(loss=fn, optimizer='sgd')
        assert m._losses == [name] and m.loss is fn                  # model.loss keeps what the caller passed
    for alias, name in R.ALIASES.items():
        assert _one_output().compile(loss=alias, optimizer='sgd')._losses == [name]
        assert getattr(keras.losses, alias) is getattr(keras.losses, name)
        assert _one_output().compile(loss=getattr(keras.losses, alias), optimizer='sgd')._losses == [name]
    m = _two_outputs().compile(loss=['hinge', keras.losses.mae], optimizer='sgd')
    assert m._losses == ['hinge', 'mean_absolute_error']
    with pytest.raises(NotImplementedError) as e:
        _one_output().compile(loss='nonsense', optimizer='sgd')
    assert all(n in str(e.value) for n in R.LOSSES)                  # the full list
    with pytest.raises(NotImplementedError):
        _one_output().compile(loss='categorical_accuracy', optimizer='sgd')     # a metric, not a loss


def test_facade_modules_resolve():
    from gennet_amd.keras.losses import logcosh, mae, mean_absolute_error, kld, cosine
    from gennet_amd.keras.metrics import categorical_accuracy, mse, mape, msle
    from gennet_amd import keras
    assert logcosh.__name__ == 'logcosh' and mae is mean_absolute_error and mae.__name__ == 'mean_absolute_error'
    assert kld.__name__ == 'kullback_leibler_divergence' and cosine.__name__ == 'cosine_proximity'
    assert categorical_accuracy.__name__ == 'categorical_accuracy' and mse is keras.losses.mse and mape and msle
    assert not hasattr(keras.losses, 'categorical_accuracy') and not hasattr(keras.metrics, 'hinge')
    with pytest.raises(NotImplementedError):
        logcosh(None, None)                                          # a name for compile(), not a tensor function


def test_lower_loss_still_lowers_and_refuses():
    from gennet_amd.keras import backend as K
    m = _one_output().compile(loss=lambda t, q: K.mean(K.square(t - q) / 4.0, axis=-1), optimizer='sgd')
    assert m._losses == ['mean_squared_error'] and m._loss_scales == [0.25]
    with pytest.raises(NotImplementedError):
        _one_output().compile(loss=lambda t, q: K.mean(t - q, axis=-1), optimizer='sgd')


def test_loss_weights():
    m = _two_outputs().compile(loss='mse', optimizer='sgd', loss_weights=[0.25, 2])
    assert m.loss_weights == [0.25, 2.0]
    assert _two_outputs().compile(loss='mse', optimizer='sgd').loss_weights is None
    with pytest.raises(NotImplementedError):
        _two_outputs().compile(loss='mse', optimizer='sgd', loss_weights={'a': 1.0})
    with pytest.raises(ValueError):
        _two_outputs().compile(loss='mse', optimizer='sgd', loss_weights=[1.0])


def test_metrics_names():
    from gennet_amd import keras
    one, two = _one_output(), _two_outputs()
    assert one.metrics_names == ['loss'] and two.metrics_names == ['loss', 'out0_loss', 'out1_loss']
    assert one.compile(loss='mse', optimizer='sgd', metrics=['accuracy']).metrics_names == ['loss', 'acc']
    assert two.compile(loss='mse', optimizer='sgd', metrics=['accuracy']).metrics_names == ['loss', 'out0_loss', 'out1_loss', 'out0_acc', 'out1_acc']
    assert one.compile(loss='mse', optimizer='sgd').metrics_names == ['loss']
    assert one.compile(loss='mse', optimizer='sgd', metrics=['accuracy', 'mae']).metrics_names == ['loss', 'acc', 'mean_absolute_error']
    assert two.compile(loss='mse', optimizer='sgd', metrics=['accuracy', 'mae']).metrics_names == [
        'loss', 'out0_loss', 'out1_loss', 'out0_acc', 'out0_mean_absolute_error', 'out1_acc', 'out1_mean_absolute_error']
    m = one.compile(loss='hinge', optimizer='sgd', metrics=['categorical_accuracy', 'mse', 'mape', 'msle', 'cosine', keras.metrics.mae])
    assert m.metrics_names == ['loss', 'categorical_accuracy', 'mean_squared_error', 'mean_absolute_percentage_error', 'mean_squared_logarithmic_error',
                               'cosine_proximity', 'mean_absolute_error']
    with pytest.raises(NotImplementedError):
        one.compile(loss='mse', optimizer='sgd', metrics=['hinge'])


def test_training_config_records_loss_weights_and_metrics(tmp_path):
    import json
    from gennet_amd import engine, h5lite
    m = _two_outputs().compile(loss=['logcosh', 'mae'], optimizer='sgd', metrics=['accuracy', 'mae'], loss_weights=[0.25, 2.0])
    path = str(tmp_path / 'm.h5')
    m.save(path)
    tc = h5lite.File(path).attrs['training_config']
    tc = json.loads(tc.decode('utf-8') if isinstance(tc, bytes) else tc)
    assert tc['loss'] == ['logcosh', 'mae'] and tc['metrics'] == ['accuracy', 'mae'] and tc['loss_weights'] == [0.25, 2.0]
    back = engine.load_model(path)
    assert back.loss == ['logcosh', 'mae'] and back.metrics == ['accuracy', 'mae'] and back.loss_weights == [0.25, 2.0]
    assert back.metrics_names == m.metrics_names
    m2 = _one_output().compile(loss='mse', optimizer='sgd', metrics=['accuracy'])      # today's arguments: today's record
    m2.save(path)
    tc = h5lite.File(path).attrs['training_config']
    tc = json.loads(tc.decode('utf-8') if isinstance(tc, bytes) else tc)
    assert tc['loss'] == 'mse' and tc['metrics'] == ['accuracy'] and tc['loss_weights'] is None


def test_header_declares_and_library_exports_the_pass():
    from gennet_amd import _lib, ops
    text = open(os.path.join(ROOT, 'include', 'gennet_hip.h')).read()
    for sym in ('gn_loss_pass', 'gn_loss_pass_workspace'):
        assert sym + '(' in text and sym in _lib.exported_symbols()
        assert hasattr(_lib.lib(), sym), sym
    for name, k in ops.LOSS_KINDS.items():
        assert 'GN_LOSS_%s = %d' % (name.upper(), k) in text, name
    assert 'GN_LOSS_KINDS = %d' % len(ops.LOSS_KINDS) in text
    assert ops.LOSS_PASS_MIN_ELEMENTS >= 131072
