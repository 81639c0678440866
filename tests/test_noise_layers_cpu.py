"""GaussianNoise, GaussianDropout and AlphaDropout without a GPU: Keras 2.2.4 configs, .h5 / JSON round trips, refused arguments, the facade,
and the discriminator knob (bbh.signal_discriminator_model(input_noise=, dropout=)) -- with its defaults the model is exactly what it was."""
import json

import numpy as np
import pytest


def _model():
    from gennet_amd.keras.layers import AlphaDropout, Dense, GaussianDropout, GaussianNoise
    from gennet_amd.keras.models import Sequential
    m = Sequential()
    m.add(Dense(8, input_shape=(12,)))
    m.add(GaussianNoise(0.3))
    m.add(GaussianDropout(0.25))
    m.add(Dense(4))
    m.add(AlphaDropout(0.1))
    m.add(Dense(1))
    return m


def test_facade_resolves_the_noise_layers_to_real_classes():
    from gennet_amd import layers as L
    from gennet_amd.keras import layers as KL
    from gennet_amd.keras.layers import noise as KN
    for name in ('GaussianNoise', 'GaussianDropout', 'AlphaDropout'):
        assert getattr(KL, name) is getattr(L, name) and getattr(KN, name) is getattr(L, name)
    KL.GaussianNoise(1.0); KL.GaussianDropout(0.2); KL.AlphaDropout(0.2)
    from gennet_amd.keras.layers import GlobalAveragePooling1D       # still a placeholder
    with pytest.raises(NotImplementedError):
        GlobalAveragePooling1D()


def test_keras_configs():
    from gennet_amd import keras_io
    from gennet_amd.layers import AlphaDropout, GaussianDropout, GaussianNoise
    base = {'name', 'trainable'}
    c = keras_io.layer_config(GaussianNoise(0.5, name='gn'))
    assert set(c) == base | {'stddev'} and c['stddev'] == 0.5 and c['name'] == 'gn'
    for cls in (GaussianDropout, AlphaDropout):
        c = keras_io.layer_config(cls(0.4))
        assert set(c) == base | {'rate'} and c['rate'] == 0.4
    # the reader takes keras' optional keys when they hold their defaults
    a = keras_io._layer_from_config('AlphaDropout', {'name': 'ad', 'trainable': True, 'rate': 0.3, 'noise_shape': None, 'seed': None}, None)
    assert isinstance(a, AlphaDropout) and a.rate == 0.3 and a.name == 'ad'
    with pytest.raises(NotImplementedError):
        keras_io._layer_from_config('AlphaDropout', {'name': 'ad2', 'rate': 0.3, 'seed': 7}, None)


def test_refused_and_invalid_arguments():
    from gennet_amd.layers import AlphaDropout, GaussianDropout, GaussianNoise
    with pytest.raises(NotImplementedError):
        AlphaDropout(0.2, noise_shape=(None, 1))
    with pytest.raises(NotImplementedError):
        AlphaDropout(0.2, seed=3)
    for bad in (-1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError):
            GaussianNoise(bad)
    for cls in (GaussianDropout, AlphaDropout):
        with pytest.raises(ValueError):
            cls(float('nan'))
        with pytest.raises((TypeError, ValueError)):
            cls('x')
        for r in (0.0, 1.0, -0.5, 2.0):               # outside (0, 1): the identity, as keras' `if 0 < self.rate < 1`
            assert not cls(r)._active()
        assert cls(0.5)._active()
    for cls in (GaussianNoise, GaussianDropout, AlphaDropout):
        assert cls(0.5).drop_rate is None             # never fused into a conv / BatchNormalization epilogue as Bernoulli dropout


def test_alpha_dropout_constants_are_keras():
    from gennet_amd.layers import AlphaDropout, GaussianDropout
    rate = 0.4
    alpha_p = -1.6732632423543772848170429916717 * 1.0507009873554804934193349852946
    a = ((1 - rate) * (1 + rate * alpha_p ** 2)) ** -0.5
    l = AlphaDropout(rate)
    assert l.a == float(np.float32(a)) and l.b == float(np.float32(-a * alpha_p * rate)) and l.alpha_p == float(np.float32(alpha_p))
    # the affine map keeps zero mean and unit variance for N(0, 1) input (what keras chooses a and b for): exact moments in fp64
    mean = a * ((1 - rate) * 0.0 + rate * alpha_p) + (-a * alpha_p * rate)
    var = a ** 2 * ((1 - rate) * 1.0 + rate * alpha_p ** 2 - ((1 - rate) * 0.0 + rate * alpha_p) ** 2)
    assert abs(mean) < 1e-12 and abs(var - 1.0) < 1e-12
    assert GaussianDropout(rate).sd == float(np.float32(np.sqrt(rate / (1 - rate))))


def test_h5_and_json_round_trip(tmp_path):
    from gennet_amd.keras.models import load_model, model_from_json
    m = _model()
    kinds = [l.__class__.__name__ for l in m._top]
    assert kinds == ['Dense', 'GaussianNoise', 'GaussianDropout', 'Dense', 'AlphaDropout', 'Dense']
    path = str(tmp_path / 'm.h5')
    m.save(path, True)
    m2 = load_model(path)
    assert [l.__class__.__name__ for l in m2._top] == kinds
    assert m2._top[1].stddev == 0.3 and m2._top[2].rate == 0.25 and m2._top[4].rate == 0.1
    for a, b in zip(m.get_weights(), m2.get_weights()):
        assert np.array_equal(a, b)
    cfg = json.loads(m.to_json())
    assert [e['class_name'] for e in cfg['config']['layers']] == kinds
    m3 = model_from_json(m.to_json())
    assert [l.__class__.__name__ for l in m3._top] == kinds
    assert [(getattr(l, 'stddev', None), getattr(l, 'rate', None)) for l in m3._top] == [(getattr(l, 'stddev', None), getattr(l, 'rate', None)) for l in m._top]


def test_default_discriminator_is_unchanged():
    from gennet_amd import bbh
    m = bbh.signal_discriminator_model(64)
    assert [l.__class__.__name__ for l in m._top] == ['Conv2D', 'LeakyReLU', 'Dropout', 'Conv2D', 'LeakyReLU', 'Dropout', 'Flatten', 'Dense', 'Activation']
    assert m._config == ('signal_discriminator_model', 64, 2, False, False)
    assert m._top[0].input_shape_arg == (64, 2, 1)
    m2 = bbh.signal_discriminator_model(64, input_noise=0.0, dropout='dropout')
    assert m2._config == m._config and [l.__class__.__name__ for l in m2._top] == [l.__class__.__name__ for l in m._top]
    m3 = bbh.signal_discriminator_model(64, 4, True, True)
    assert m3._config == ('signal_discriminator_model', 64, 4, True, True)


@pytest.mark.parametrize('noise,dropout,kind', [(0.1, 'gaussian', 'GaussianDropout'), (0.0, 'alpha', 'AlphaDropout'), (0.5, 'dropout', 'Dropout')])
def test_discriminator_knob(noise, dropout, kind):
    from gennet_amd import bbh
    m = bbh.signal_discriminator_model(64, input_noise=noise, dropout=dropout)
    body = ['Conv2D', 'LeakyReLU', kind, 'Conv2D', 'LeakyReLU', kind, 'Flatten', 'Dense', 'Activation']
    names = [l.__class__.__name__ for l in m._top]
    assert names == (['GaussianNoise'] + body if noise > 0 else body)
    assert m._top[0].input_shape_arg == (64, 2, 1)
    if noise > 0:
        assert m._top[0].stddev == noise
    assert all(l.rate == 0.4 for l in m._top if l.__class__.__name__ == kind)
    assert m._config == ('signal_discriminator_model', 64, 2, False, False, noise, dropout)
    again = bbh.model_from_config(m._config)
    assert [l.__class__.__name__ for l in again._top] == names
    with pytest.raises(ValueError):
        bbh.signal_discriminator_model(64, dropout='bernoulli')


def test_training_script_exposes_the_knob():
    import os
    src = open(os.path.join(os.path.dirname(__file__), '..', 'scripts', 'bbh_train.py')).read()
    assert "'--d-input-noise'" in src and "'--d-dropout'" in src and 'd_config=d_config' in src
