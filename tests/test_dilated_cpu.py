"""CPU-only checks of Conv1D(dilation_rate=..., padding='causal'): the numpy restatement tests/dilated_ref.py (split -> undilated conv
-> merge) against torch.nn.functional.conv1d(dilation=d) and its autograd in fp64, the geometry, the layer's arguments and refusals, what the
planner is told, the Keras configs and the binding's declarations.  The passes and the layer on the GPU: tests/test_dilated_gpu.py."""
import json

import numpy as np
import pytest
import torch

import dilated_ref as R

# B, L, Cin, Cout, k, d, padding
SHAPES = [(2, 37, 3, 5, 5, 2, 'same'), (1, 16, 4, 4, 3, 4, 'causal'), (3, 50, 2, 6, 8, 3, 'valid'), (2, 9, 1, 2, 2, 7, 'same'),
          (2, 5, 2, 2, 3, 2, 'causal'), (1, 23, 4, 8, 5, 9, 'same'), (2, 40, 4, 4, 40, 1, 'causal')]


torch_layer = R.torch_layer          # explicit zero padding, torch.nn.functional.conv1d(dilation=d), the activation


@pytest.mark.parametrize('act,p', [('linear', 0.0), ('tanh', 0.0), ('leaky', 0.2)])
@pytest.mark.parametrize('B,L,Cin,Cout,k,d,padding', SHAPES, ids=['-'.join(map(str, s)) for s in SHAPES])
def test_the_phase_identity_equals_torch_dilated_conv_and_its_autograd(B, L, Cin, Cout, k, d, padding, act, p):
    rng = np.random.RandomState(L * 10 + k + d)
    x, w, b = rng.randn(B, L, Cin), rng.randn(k, Cin, Cout) / np.sqrt(k * Cin), rng.randn(Cout)
    Lout = R.geometry(L, k, 1, padding, d)[0]
    assert Lout >= 1
    dy = rng.randn(B, Lout, Cout)
    xt, wt, bt = (torch.tensor(a, requires_grad=True) for a in (x, w, b))
    yt = torch_layer(xt, wt, bt, 1, padding, d, act, p)
    yt.backward(torch.tensor(dy))
    y = R.layer_fwd(x, w, b, 1, padding, d, act, p)
    assert y.shape == tuple(yt.shape) == (B, Lout, Cout)
    dx, dw, db = R.layer_bwd(x, w, b, dy, 1, padding, d, act, p)
    for got, ref in ((y, yt.detach()), (dx, xt.grad), (dw, wt.grad), (db, bt.grad)):
        ref = ref.numpy()
        assert got.shape == ref.shape and np.abs(got - ref).max() <= 1e-12 * max(np.abs(ref).max(), 1.0)


def test_causal_stride_2_without_dilation_equals_torch():
    rng = np.random.RandomState(1)
    x, w, b = rng.randn(2, 21, 3), rng.randn(4, 3, 5), rng.randn(5)
    dy = rng.randn(2, 11, 5)
    xt, wt, bt = (torch.tensor(a, requires_grad=True) for a in (x, w, b))
    yt = torch_layer(xt, wt, bt, 2, 'causal', 1, 'tanh')
    yt.backward(torch.tensor(dy))
    assert np.abs(R.layer_fwd(x, w, b, 2, 'causal', 1, 'tanh') - yt.detach().numpy()).max() <= 1e-12
    for got, ref in zip(R.layer_bwd(x, w, b, dy, 2, 'causal', 1, 'tanh'), (xt.grad, wt.grad, bt.grad)):
        assert np.abs(got - ref.numpy()).max() <= 1e-12 * max(np.abs(ref.numpy()).max(), 1.0)


def test_split_and_merge_are_adjoint_permutations():
    rng = np.random.RandomState(2)
    for B, L, C, d, off, M in ((2, 11, 3, 3, 4, 6), (1, 5, 2, 7, 0, 2), (2, 9, 1, 1, 3, 12), (2, 10, 4, 2, 3, 3)):
        x, g = rng.randn(B, L, C), rng.randn(B * d, M, C)
        xs = R.split(x, d, off, M)
        assert xs.shape == (B * d, M, C) and not np.signbit(xs[xs == 0]).any()
        if (L - 1 + off) // d < M:
            assert np.array_equal(R.merge(xs, B, d, off, L), x)
            assert abs((xs * g).sum() - (x * R.merge(g, B, d, off, L)).sum()) <= 1e-12          # <split x, g> = <x, merge g>
        else:                                                                                   # rows beyond M are dropped
            assert xs.sum() != x.sum() and np.array_equal(xs[0, :, 0], [x[0, m * d - off, 0] if 0 <= m * d - off < L else 0.0 for m in range(M)])
    assert R.split(np.float32(rng.randn(1, 4, 2)), 2, 1, 3).dtype == np.float32


# L, k, stride, padding, d -> Lout, pad_left
GEOMETRY = [(64, 5, 1, 'valid', 4, 48, 0), (64, 5, 1, 'same', 4, 64, 8), (64, 5, 1, 'causal', 4, 64, 16), (64, 5, 2, 'causal', 1, 32, 4),
            (63, 5, 2, 'causal', 1, 32, 4), (9, 2, 1, 'same', 7, 9, 3), (50, 8, 1, 'valid', 3, 29, 0), (23, 5, 1, 'same', 9, 23, 18),
            (64, 5, 1, 'valid', 1, 60, 0), (64, 5, 2, 'same', 1, 32, 1), (7, 5, 1, 'same', 1, 7, 2)]


@pytest.mark.parametrize('L,k,s,padding,d,Lout,pl', GEOMETRY)
def test_geometry(L, k, s, padding, d, Lout, pl):
    from gennet_amd import ops
    assert ops.conv_geometry(L, k, s, padding, dilation=d) == (Lout, pl) == R.geometry(L, k, s, padding, d)[:2]
    if d == 1 and padding != 'causal':
        assert ops.conv_geometry(L, k, s, padding) == (Lout, pl)           # the existing callers' form
    with pytest.raises(ValueError):
        ops.conv_geometry(L, k, s, 'full', dilation=d)


def test_output_shapes_and_the_forms_of_dilation_rate():
    from gennet_amd.layers import Conv1D
    assert Conv1D(8, 5, dilation_rate=4).compute_output_shape((64, 4)) == (48, 8)
    assert Conv1D(8, 5, dilation_rate=4, padding='same').compute_output_shape((64, 4)) == (64, 8)
    assert Conv1D(8, 5, dilation_rate=4, padding='causal').compute_output_shape((64, 4)) == (64, 8)
    assert Conv1D(8, 5, padding='causal').compute_output_shape((64, 4)) == (64, 8)
    assert Conv1D(8, 5, strides=2, padding='causal').compute_output_shape((64, 4)) == (32, 8)
    assert Conv1D(8, 5).compute_output_shape((64, 4)) == (60, 8)
    for form in (4, (4,), [4]):
        layer = Conv1D(8, 5, dilation_rate=form)
        assert layer.dilation == 4 and layer.phased and layer.compute_output_shape((64, 4)) == (48, 8)
    assert Conv1D(8, 5).dilation == 1 and not Conv1D(8, 5).phased and not Conv1D(8, 5, padding='same', strides=2).phased
    assert Conv1D(8, 5, padding='causal').phased and Conv1D(8, 5, padding='causal').dilation == 1


def test_refusals():
    from gennet_amd.layers import Conv1D
    for bad in (0, -1, (0,), (2, 2)):
        with pytest.raises(ValueError):
            Conv1D(8, 5, dilation_rate=bad)
    with pytest.raises(ValueError):
        Conv1D(8, 5, strides=2, dilation_rate=2)
    with pytest.raises(ValueError):
        Conv1D(8, 5, strides=2, dilation_rate=2, padding='causal')
    Conv1D(8, 5, strides=2, dilation_rate=1, padding='causal')
    with pytest.raises(ValueError) as e:
        Conv1D(8, 5, dilation_rate=4).build((16, 4))                       # (16 - 16 - 1) // 1 + 1 = 0 rows
    assert '(16, 4)' in str(e.value)
    Conv1D(8, 5, dilation_rate=4).build((17, 4))
    Conv1D(8, 5, dilation_rate=40, padding='same').build((3, 4))           # d > L under 'same' and 'causal': Lout = L
    Conv1D(8, 5, dilation_rate=40, padding='causal').build((3, 4))
    with pytest.raises(NotImplementedError):
        Conv1D(8, 5, padding='full')


def planner_view(layer, Cin):
    return (layer.fusable_act, layer.fusable_drop, layer.offers_act_bwd, layer.can_absorb_prev_act_bwd, layer.can_fold_bn, layer.can_fold_upsample(),
            layer.can_defer_dgrad(Cin))


def test_what_the_planner_is_told():
    from gennet_amd.layers import Conv1D
    # plain layers: the values they have always had
    assert planner_view(Conv1D(64, 5, padding='same'), 64) == (True, True, True, True, True, True, False)
    assert planner_view(Conv1D(64, 5, strides=2, padding='same', activation='tanh'), 64) == (True, True, True, True, False, True, False)
    assert planner_view(Conv1D(64, 3, padding='valid'), 64) == (True, True, True, True, True, False, False)
    assert planner_view(Conv1D(1, 5, padding='same'), 64) == (True, True, True, True, False, True, True)
    assert planner_view(Conv1D(1, 5, padding='same', dilation_rate=(1,)), 64) == (True, True, True, True, False, True, True)
    built = Conv1D(5, 5, padding='same')
    built.build((32, 3))                                                   # 3 -> 5 runs on the any-channel kernels: no fused Dropout
    assert planner_view(built, 3) == (True, False, True, True, False, True, False)
    # dilated or causal: the activation epilogue stays (elementwise), every cross-layer fusion is declined
    for layer, Cin in ((Conv1D(64, 5, padding='same', dilation_rate=2), 64), (Conv1D(64, 5, padding='causal'), 64),
                       (Conv1D(1, 5, padding='same', dilation_rate=2), 64), (Conv1D(1, 5, padding='causal'), 64),
                       (Conv1D(64, 5, dilation_rate=3), 64)):
        assert planner_view(layer, Cin) == (True, False, False, False, False, False, False), (layer.padding, layer.dilation)


def test_the_plan_of_a_model_fuses_nothing_across_a_dilated_or_causal_layer():
    from gennet_amd import layers as L
    from gennet_amd.engine import Sequential
    ls = [L.Conv1D(8, 3, padding='same', activation='tanh', input_shape=(16, 8)), L.UpSampling1D(2),
          L.Conv1D(8, 5, padding='same', dilation_rate=2), L.LeakyReLU(0.2), L.Dropout(0.4),
          L.Conv1D(8, 3, padding='causal'), L.BatchNormalization(), L.Conv1D(1, 3, padding='causal', dilation_rate=2),
          L.Conv1D(8, 3, padding='same', activation='tanh'), L.Conv1D(8, 3, padding='same')]
    m = Sequential(ls)
    m._plan()
    up, dil, leaky, drop, causal, bn, one, tail1, tail2 = m.nodes[1:]
    assert not up.absorbed and dil.fold_up is None                         # the upsample is materialised
    assert dil.fused_act == ('leaky', L.LeakyReLU(0.2).alpha) and leaky.absorbed       # an activation layer still fuses: elementwise
    assert dil.fused_drop is None and not drop.absorbed                    # the Dropout runs on its own
    assert dil.fuse_prev == -1                                             # ... and absorbs no producer's activation backward
    assert causal.infer_bn is None and causal.fuse_prev == -1 and not bn.absorbed
    assert one.lazy_bn == -1 and one.fuse_prev == -1
    assert tail1.fuse_prev == -1                                           # its producer, the dilated layer, offers none
    assert tail2.fuse_prev == tail1.index                                  # two plain layers still fuse
    assert [n.out_shape for n in m.nodes] == [(16, 8), (32, 8), (32, 8), (32, 8), (32, 8), (32, 8), (32, 8), (32, 1), (32, 8), (32, 8)]


def test_config_round_trip():
    from gennet_amd import keras_io
    from gennet_amd.layers import Conv1D
    for layer, dil, pad in ((Conv1D(8, 5, dilation_rate=4, padding='causal', activation='tanh'), [4], 'causal'),
                            (Conv1D(8, 3, dilation_rate=(2,), padding='same'), [2], 'same'), (Conv1D(8, 3, padding='causal', strides=2), [1], 'causal'),
                            (Conv1D(8, 3), [1], 'valid'), (Conv1D(8, 5, padding='same', strides=2), [1], 'same')):
        cfg = keras_io.layer_config(layer)
        assert cfg['dilation_rate'] == dil and cfg['padding'] == pad and layer.get_config() == cfg
        back = keras_io._layer_from_config('Conv1D', json.loads(json.dumps(cfg)), None)
        assert (back.dilation, back.padding, back.stride, back.k, back.filters, back.activation) == \
            (layer.dilation, layer.padding, layer.stride, layer.k, layer.filters, layer.activation)
        assert keras_io.layer_config(back) == cfg
    old = dict(keras_io.layer_config(Conv1D(8, 3)))
    del old['dilation_rate']                                               # a config without the key: undilated
    assert keras_io._layer_from_config('Conv1D', old, None).dilation == 1


# typed in the form keras 2.2.4 writes (to_json of a Sequential)
KERAS_JSON = '''{"class_name": "Sequential", "config": {"name": "sequential_1", "layers": [
 {"class_name": "Conv1D", "config": {"name": "conv1d_1", "trainable": true, "batch_input_shape": [null, 64, 4], "dtype": "float32", "filters": 8,
  "kernel_size": [5], "strides": [1], "padding": "causal", "data_format": "channels_last", "dilation_rate": [4], "activation": "tanh", "use_bias": true,
  "kernel_initializer": {"class_name": "VarianceScaling", "config": {"scale": 1.0, "mode": "fan_avg", "distribution": "uniform", "seed": null}},
  "bias_initializer": {"class_name": "Zeros", "config": {}}, "kernel_regularizer": null, "bias_regularizer": null, "activity_regularizer": null,
  "kernel_constraint": null, "bias_constraint": null}},
 {"class_name": "Conv1D", "config": {"name": "conv1d_2", "trainable": true, "filters": 8,
  "kernel_size": [5], "strides": [1], "padding": "valid", "data_format": "channels_last", "dilation_rate": [4], "activation": "linear", "use_bias": true,
  "kernel_initializer": {"class_name": "VarianceScaling", "config": {"scale": 1.0, "mode": "fan_avg", "distribution": "uniform", "seed": null}},
  "bias_initializer": {"class_name": "Zeros", "config": {}}, "kernel_regularizer": null, "bias_regularizer": null, "activity_regularizer": null,
  "kernel_constraint": null, "bias_constraint": null}},
 {"class_name": "Conv1D", "config": {"name": "conv1d_3", "trainable": true, "filters": 2,
  "kernel_size": [3], "strides": [2], "padding": "same", "data_format": "channels_last", "dilation_rate": [1], "activation": "linear", "use_bias": true,
  "kernel_initializer": {"class_name": "VarianceScaling", "config": {"scale": 1.0, "mode": "fan_avg", "distribution": "uniform", "seed": null}},
  "bias_initializer": {"class_name": "Zeros", "config": {}}, "kernel_regularizer": null, "bias_regularizer": null, "activity_regularizer": null,
  "kernel_constraint": null, "bias_constraint": null}}]}, "keras_version": "2.2.4", "backend": "tensorflow"}'''


def test_a_keras_json_with_a_dilated_causal_conv_builds_and_is_written_back():
    from gennet_amd import keras_io
    from gennet_amd.keras.models import model_from_json
    m = model_from_json(KERAS_JSON)
    assert [(l.dilation, l.padding, l.stride, l.phased) for l in m.layers] == [(4, 'causal', 1, True), (4, 'valid', 1, True), (1, 'same', 2, False)]
    assert [n.out_shape for n in m.nodes] == [(64, 8), (48, 8), (24, 2)]                  # an undilated reading would give (64, 8), (60, 8), (30, 2)
    written = json.loads(m.to_json())['config']['layers']
    assert [(c['config']['dilation_rate'], c['config']['padding']) for c in written] == [([4], 'causal'), ([4], 'valid'), ([1], 'same')]
    again = model_from_json(m.to_json())
    assert [keras_io.layer_config(l) for l in again.layers] == [keras_io.layer_config(l) for l in m.layers]


def test_binding_declares_the_two_passes():
    from gennet_amd import _lib
    from gennet_amd._lib import i32, vp
    sig = (i32, [vp, vp, i32, i32, i32, i32, i32, i32, vp])
    assert _lib.DECLS['gn_dilate_split'] == sig and _lib.DECLS['gn_dilate_merge'] == sig
