"""Conv2DTranspose without a GPU: the facade, keras' deconv_length, the refused arguments, and the reference's generator file g_model.hdf5
(Keras 2.1.6: Reshape, four Conv2DTranspose + BatchNormalization, Flatten, two Dense heads, SGD) loaded, saved and loaded again."""
import os

import numpy as np
import pytest

from gennet_amd import h5lite, keras_io
from gennet_amd import layers as L

from test_h5 import GOLD, REF, keras_file

G = GOLD['g_model.hdf5']


def deconv_length(W, k, s, padding):
    """keras.utils.conv_utils.deconv_length (keras 2.2.4) without output_padding."""
    if padding == 'valid':
        return W * s + max(k - s, 0)
    return W * s


def test_facade_resolves_conv2d_transpose_to_the_real_layer():
    from gennet_amd.keras.layers import Conv2DTranspose as A
    from gennet_amd.keras.layers.convolutional import Conv2DTranspose as B
    assert A is B is L.Conv2DTranspose
    layer = A(8, (1, 4), strides=(1, 2), padding='same', activation='relu')
    assert (layer.filters, layer.k, layer.stride, layer.padding, layer.activation[0]) == (8, 4, 2, 'same', 'relu')
    from gennet_amd.keras.layers.convolutional import UpSampling2D, MaxPooling1D, AveragePooling1D
    for cls in (UpSampling2D, MaxPooling1D, AveragePooling1D):
        with pytest.raises(NotImplementedError):
            cls()


@pytest.mark.parametrize('padding', ['valid', 'same'])
@pytest.mark.parametrize('s', [1, 2])
def test_output_shape_is_deconv_length(padding, s):
    for k in (1, 2, 4, 5, 8, 16, 32, 40):
        if k < s:
            continue
        for W in (1, 2, 7, 64, 1000):
            layer = L.Conv2DTranspose(6, (1, k), strides=(1, s), padding=padding)
            assert layer.compute_output_shape((3, W, 5)) == (3, deconv_length(W, k, s, padding), 6)
            if padding == 'same':
                # the adjoint conv of the output length maps it back to W, with TF's 'SAME' left padding
                from gennet_amd import ops
                Wout = deconv_length(W, k, s, padding)
                out, pl = ops.conv_geometry(Wout, k, s, 'same')
                assert out == W and pl == max((W - 1) * s + k - Wout, 0) // 2


def test_weights_are_held_in_keras_layout_with_the_glorot_limit():
    from gennet_amd.engine import Input, Model
    inp = Input(shape=(2, 9, 3))
    out = L.Conv2DTranspose(8, (1, 7), strides=(1, 2), padding='same')(inp)
    m = Model(inputs=inp, outputs=out)
    layer = m.layers[-1]
    assert tuple(layer.kernel.shape) == (1, 7, 8, 3) and tuple(layer.bias.shape) == (8,)
    w = layer.kernel.numpy()
    assert np.abs(w).max() <= np.sqrt(6.0 / ((8 + 3) * 7))
    assert m.output_shape == (None, 2, 18, 8)
    # channel counts no conv kernel family takes (both not multiples of 4, or a side > 4 that is not one) are refused at build
    with pytest.raises(NotImplementedError, match='multiple of 4'):
        L.Conv2DTranspose(5, (1, 7))(Input(shape=(2, 9, 3)))


@pytest.mark.parametrize('kw', [
    dict(kernel_size=(2, 4)), dict(kernel_size=(1, 4), strides=(2, 1)), dict(kernel_size=(1, 4), strides=(1, 3)),
    dict(kernel_size=(1, 41)), dict(kernel_size=(1, 4), dilation_rate=(1, 2)), dict(kernel_size=(1, 4), output_padding=(0, 1)),
    dict(kernel_size=(1, 4), use_bias=False), dict(kernel_size=(1, 4), data_format='channels_first'), dict(kernel_size=(1, 1), strides=(1, 2)),
    dict(kernel_size=(1, 4), padding='causal'),
])
def test_refused_arguments_raise_naming_the_supported_case(kw):
    with pytest.raises(NotImplementedError, match='Conv2DTranspose'):
        L.Conv2DTranspose(4, **kw)


def test_config_reader_accepts_later_keras_keys_and_refuses_other_values():
    base = dict(G['model_config']['config']['layers'][3]['config'])
    layer = keras_io._layer_from_config('Conv2DTranspose', dict(base, output_padding=None, dilation_rate=[1, 1]), None)
    assert isinstance(layer, L.Conv2DTranspose) and layer.k == 4 and layer.filters == 128
    for bad in (dict(output_padding=[0, 1]), dict(dilation_rate=[1, 2])):
        with pytest.raises(NotImplementedError):
            keras_io._layer_from_config('Conv2DTranspose', dict(base, **bad), None)


def _g_model_path(tmp_path):
    path = str(tmp_path / 'g_model.hdf5')
    with open(path, 'wb') as fh:
        fh.write(keras_file('g_model.hdf5')[0])
    return path


def _class_names(m):
    return [[('InputLayer' if isinstance(l, keras_io.InputLayer) else l.__class__.__name__), l.name] for l in keras_io.top_layers(m)]


def test_load_model_on_the_reference_generator_file(tmp_path):
    """keras.models.load_model on the reference's g_model.hdf5: same layers, every weight equal to its dataset, the output shape and
    parameter count, SGD's lr and iteration count; and the weights-only best_g_weights.hdf5 fills the same architecture."""
    from gennet_amd.keras.models import load_model
    path = _g_model_path(tmp_path)
    m = load_model(path)
    assert _class_names(m) == G['model']['layers']
    f = h5lite.File(path)
    n = 0
    for l in keras_io.top_layers(m):
        for p in keras_io.keras_weights(l):
            assert np.array_equal(p.numpy(), f['model_weights'][l.name][p.name + ':0'].value), p.name
            n += 1
    assert n == 7 * 4 + 4 * 2 + 2 * 2
    convs = [4 * 128 + 128, 8 * 64 * 128 + 64, 16 * 32 * 64 + 32, 32 * 16 * 32 + 16]
    bns = 4 * (1 + 128 + 64 + 32 + 16 + 912 + 50)
    assert m.output_shape == (None, 50) and m.count_params() == sum(convs) + bns + 912 * 50 + 50 + 50 * 50 + 50
    assert m.loss == 'binary_crossentropy' and type(m.optimizer).__name__ == 'SGD'
    assert m.optimizer.lr == float(np.float32(0.004))
    pend = m._pending_optimizer_weights
    assert len(pend) == 27 and int(np.asarray(pend[0])) == int(f['optimizer_weights']['SGD']['iterations:0'].value)
    m.load_weights(os.path.join(REF, 'best_g_weights.hdf5'))
    fw = h5lite.File(os.path.join(REF, 'best_g_weights.hdf5'))
    l = [l for l in keras_io.top_layers(m) if l.name == 'conv2d_transpose_2'][0]
    assert np.array_equal(l.kernel.numpy(), fw['conv2d_transpose_2']['conv2d_transpose_2']['kernel:0'].value)


def test_save_then_load_keeps_config_and_weights(tmp_path):
    from gennet_amd.keras.models import load_model
    m = load_model(_g_model_path(tmp_path))
    out = str(tmp_path / 'again.hdf5')
    m.save(out)
    m2 = load_model(out)
    assert keras_io.model_config(m2) == keras_io.model_config(m)
    for a, b in zip(keras_io.top_layers(m), keras_io.top_layers(m2)):
        for p, q in zip(keras_io.keras_weights(a), keras_io.keras_weights(b)):
            assert np.array_equal(p.numpy(), q.numpy())
    recorded = [l['config'] for l in G['model_config']['config']['layers'] if l['class_name'] == 'Conv2DTranspose']
    mine = [e['config'] for e in keras_io.model_config(m2)['config']['layers'] if e['class_name'] == 'Conv2DTranspose']
    assert len(mine) == len(recorded) == 4
    for got, want in zip(mine, recorded):
        for k, v in want.items():
            assert got[k] == v, k
