"""The sequence layers without a GPU: Dense over the last axis, TimeDistributed(Dense), RepeatVector, Permute, Cropping1D and
ZeroPadding1D -- the facade paths, shape inference, refusals, Keras 2.2.4 configs through JSON and .h5, tests/sequence_ref.py against torch, and
what the four new entry points answer before they launch anything."""
import ctypes
import itertools
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sequence_ref as S


def test_every_facade_path_resolves_to_the_class():
    from gennet_amd import layers as L, sequence
    from gennet_amd.keras.layers import Cropping1D, Permute, RepeatVector, TimeDistributed, ZeroPadding1D
    from gennet_amd.keras.layers.convolutional import Cropping1D as C2, ZeroPadding1D as Z2
    from gennet_amd.keras.layers.core import Permute as P2, RepeatVector as R2
    from gennet_amd.keras.layers.wrappers import TimeDistributed as T2
    assert TimeDistributed is T2 is L.TimeDistributed is sequence.TimeDistributed
    assert RepeatVector is R2 is L.RepeatVector is sequence.RepeatVector
    assert Permute is P2 is L.Permute is sequence.Permute
    assert Cropping1D is C2 is L.Cropping1D is sequence.Cropping1D
    assert ZeroPadding1D is Z2 is L.ZeroPadding1D is sequence.ZeroPadding1D


# ---- shapes and refusals ---------------------------------------------------------------------------------------------------------------
def out_shape(layer, shape):
    from gennet_amd.engine import Input
    return tuple(layer(Input(shape)).shape)


def test_dense_acts_on_the_last_axis():
    from gennet_amd.layers import Dense
    d3, d4, d2 = Dense(5), Dense(5), Dense(5)
    assert out_shape(d3, (7, 6)) == (7, 5) and d3.kernel.shape == (6, 5) and d3.bias.shape == (5,) and d3.per_position
    assert out_shape(d4, (3, 4, 6)) == (3, 4, 5) and d4.kernel.shape == (6, 5) and d4.per_position
    assert out_shape(d2, (6,)) == (5,) and d2.kernel.shape == (6, 5) and not d2.per_position


def test_the_planner_fuses_nothing_onto_a_per_position_dense_and_everything_it_did_onto_a_rank_2_one():
    from gennet_amd.engine import Sequential
    from gennet_amd.layers import Activation, Conv1D, Dense, Flatten
    m = Sequential([Conv1D(8, 3, activation='relu', input_shape=(10, 4)), Dense(1), Activation('sigmoid')])
    m._plan()
    conv, dense, act = m.nodes
    assert dense.layer.per_position and dense.fused_act is None and not act.absorbed and dense.fuse_prev == -1
    assert not dense.layer.fusable_act and not dense.layer.offers_act_bwd and not dense.layer.can_absorb_prev_act_bwd
    m = Sequential([Conv1D(8, 3, activation='relu', input_shape=(10, 4)), Flatten(), Dense(1), Activation('sigmoid')])
    m._plan()
    conv, flat, dense, act = m.nodes
    assert not dense.layer.per_position and dense.fused_act == ('sigmoid', 0.0) and act.absorbed and dense.fuse_prev == conv.index
    assert dense.layer.fusable_act and dense.layer.offers_act_bwd and dense.layer.can_absorb_prev_act_bwd


def test_repeat_vector_shape():
    from gennet_amd.layers import RepeatVector
    assert out_shape(RepeatVector(7), (5,)) == (7, 5)
    with pytest.raises(ValueError):
        out_shape(RepeatVector(7), (4, 5))
    with pytest.raises(ValueError):
        RepeatVector(0)


def test_permute_shapes_for_every_permutation_of_ranks_3_and_4():
    from gennet_amd.layers import Permute
    for shape in ((5, 7), (5, 7, 6)):
        perms = list(itertools.permutations(range(1, len(shape) + 1)))
        assert len(perms) == (2 if len(shape) == 2 else 6)
        for dims in perms:
            layer = Permute(dims)
            assert out_shape(layer, shape) == tuple(shape[d - 1] for d in dims)
            assert bool(getattr(layer, 'shape_only', False)) == (dims == tuple(range(1, len(shape) + 1)))
    for bad in ((0, 1), (1, 1), (2, 3)):
        with pytest.raises(ValueError):
            Permute(bad)
    with pytest.raises(ValueError):
        out_shape(Permute((2, 1)), (3, 4, 5))
    with pytest.raises(NotImplementedError):
        Permute((1, 2, 3, 4))


def test_crop_and_pad_shapes_with_int_and_pair_arguments():
    from gennet_amd.layers import Cropping1D, ZeroPadding1D
    assert Cropping1D().cropping == (1, 1) and ZeroPadding1D().padding == (1, 1)
    assert Cropping1D(2).cropping == (2, 2) and Cropping1D((0, 3)).cropping == (0, 3) and Cropping1D([1, 2]).cropping == (1, 2)
    assert ZeroPadding1D(2).padding == (2, 2) and ZeroPadding1D((3, 0)).padding == (3, 0)
    assert out_shape(Cropping1D(2), (9, 4)) == (5, 4) and out_shape(Cropping1D((1, 3)), (9, 4)) == (5, 4)
    assert out_shape(ZeroPadding1D(2), (9, 4)) == (13, 4) and out_shape(ZeroPadding1D((1, 3)), (9, 4)) == (13, 4)
    for bad in ((1, 2, 3), -1, (1, -1), 'same', 1.5):
        with pytest.raises(ValueError):
            Cropping1D(bad)
        with pytest.raises(ValueError):
            ZeroPadding1D(bad)
    with pytest.raises(ValueError):
        out_shape(ZeroPadding1D(1), (9,))


def test_a_crop_that_leaves_no_sample_is_a_value_error():
    from gennet_amd.layers import Cropping1D
    assert out_shape(Cropping1D((4, 4)), (9, 4)) == (1, 4)
    for crop in ((4, 5), (9, 0), 5):
        with pytest.raises(ValueError, match='no sample is left'):
            out_shape(Cropping1D(crop), (9, 4))


def test_time_distributed_takes_a_dense_and_names_what_it_refuses():
    from gennet_amd.layers import Conv1D, Dense, LSTM, TimeDistributed
    with pytest.raises(NotImplementedError, match='Conv1D'):
        TimeDistributed(Conv1D(4, 3))
    with pytest.raises(NotImplementedError, match='LSTM'):
        TimeDistributed(LSTM(4))
    with pytest.raises(ValueError):
        TimeDistributed('dense')
    td = TimeDistributed(Dense(5, activation='tanh'), name='heads')
    assert out_shape(td, (7, 6)) == (7, 5) and out_shape(TimeDistributed(Dense(5)), (3, 4, 6)) == (3, 4, 5)
    assert [p.name for p in td.weights] == ['heads/kernel', 'heads/bias'] and [p.shape for p in td.weights] == [(6, 5), (5,)]
    assert td.layer.weights == [] and td.layer.kernel is td.weights[0] and td.layer.bias is td.weights[1]
    with pytest.raises(ValueError):
        out_shape(TimeDistributed(Dense(5)), (6,))


def test_time_distributed_honours_the_inner_layers_regularizers_and_trainable():
    from gennet_amd import regularizers
    from gennet_amd.layers import Dense, TimeDistributed
    td = TimeDistributed(Dense(3, kernel_regularizer=regularizers.l2(0.01), bias_regularizer=regularizers.l1(0.02),
                               activity_regularizer=regularizers.l1(0.03)))
    out_shape(td, (4, 2))
    k, b = td.weights
    assert k.regularizer.l2 == np.float32(0.01) and b.regularizer.l1 == np.float32(0.02) and td.activity_regularizer.l1 == np.float32(0.03)
    assert td.trainable and td.trainable_weights == [k, b]
    frozen = TimeDistributed(Dense(3, trainable=False))
    out_shape(frozen, (4, 2))
    assert not frozen.trainable and frozen.trainable_weights == [] and len(frozen.non_trainable_weights) == 2
    also = TimeDistributed(Dense(3), trainable=False)
    assert not also.trainable and not also.layer.trainable
    also.trainable = True
    assert also.layer.trainable


# ---- configs ------------------------------------------------------------------------------------------------------------------------------
def sequence_model():
    from gennet_amd.engine import Input, Model
    from gennet_amd.layers import Concatenate, Cropping1D, Dense, Permute, RepeatVector, TimeDistributed, ZeroPadding1D, LSTM
    x = Input((12, 3), name='strain')
    h = RepeatVector(12, name='again')(LSTM(8, name='enc')(x))
    h = TimeDistributed(Dense(3, activation='tanh', name='inner'), name='heads')(h)
    p = Permute((2, 1), name='swap')(h)
    p = Permute((2, 1), name='swap_back')(Dense(12, name='mix')(p))
    y = Concatenate(name='join')([ZeroPadding1D((2, 0), name='pad')(Cropping1D((1, 1), name='crop')(p)), x])
    return Model(inputs=x, outputs=y, name='sequence_model')


def test_get_config_holds_keras_keys_and_round_trips_through_json():
    from gennet_amd.engine import model_from_json
    m = sequence_model()
    assert m.output_shape == (None, 12, 6)
    cfg = dict((l.name, l.get_config()) for l in m.layers)
    assert cfg['again'] == {'name': 'again', 'trainable': True, 'n': 12}
    assert cfg['swap'] == {'name': 'swap', 'trainable': True, 'dims': [2, 1]}
    assert cfg['crop'] == {'name': 'crop', 'trainable': True, 'cropping': [1, 1]}
    assert cfg['pad'] == {'name': 'pad', 'trainable': True, 'padding': [2, 0]}
    assert sorted(cfg['heads']) == ['layer', 'name', 'trainable'] and sorted(cfg['heads']['layer']) == ['class_name', 'config']
    assert cfg['heads']['layer']['class_name'] == 'Dense' and cfg['heads']['layer']['config']['name'] == 'inner'
    assert cfg['heads']['layer']['config']['units'] == 3 and cfg['heads']['layer']['config']['activation'] == 'tanh'
    again = model_from_json(m.to_json())
    assert json.loads(again.to_json()) == json.loads(m.to_json())
    assert [type(l).__name__ for l in again.layers] == [type(l).__name__ for l in m.layers]
    assert [(p.name, p.shape) for p in again.weights] == [(p.name, p.shape) for p in m.weights]
    assert again.output_shape == m.output_shape


def test_a_functional_model_as_keras_2_2_4_writes_it_builds():
    """the five layers as keras 2.2.4's Model.to_json writes them (wrappers.py, core.py, convolutional.py get_config), typed by hand"""
    from gennet_amd.engine import model_from_json
    glorot = {"class_name": "VarianceScaling", "config": {"scale": 1.0, "mode": "fan_avg", "distribution": "uniform", "seed": None}}
    dense = {"name": "dense_1", "trainable": True, "units": 3, "activation": "linear", "use_bias": True, "kernel_initializer": glorot,
             "bias_initializer": {"class_name": "Zeros", "config": {}}, "kernel_regularizer": None, "bias_regularizer": None,
             "activity_regularizer": None, "kernel_constraint": None, "bias_constraint": None}
    head = dict(dense, name="dense_2", units=4, batch_input_shape=None)
    del head["batch_input_shape"]
    layers = [
        {"name": "input_1", "class_name": "InputLayer", "config": {"batch_input_shape": [None, 5], "dtype": "float32", "sparse": False, "name": "input_1"},
         "inbound_nodes": []},
        {"name": "repeat_vector_1", "class_name": "RepeatVector", "config": {"name": "repeat_vector_1", "trainable": True, "n": 7},
         "inbound_nodes": [[["input_1", 0, 0, {}]]]},
        {"name": "time_distributed_1", "class_name": "TimeDistributed",
         "config": {"name": "time_distributed_1", "trainable": True, "layer": {"class_name": "Dense", "config": dense}},
         "inbound_nodes": [[["repeat_vector_1", 0, 0, {}]]]},
        {"name": "permute_1", "class_name": "Permute", "config": {"name": "permute_1", "trainable": True, "dims": [2, 1]},
         "inbound_nodes": [[["time_distributed_1", 0, 0, {}]]]},
        {"name": "zero_padding1d_1", "class_name": "ZeroPadding1D", "config": {"name": "zero_padding1d_1", "trainable": True, "padding": [2, 1]},
         "inbound_nodes": [[["permute_1", 0, 0, {}]]]},
        {"name": "cropping1d_1", "class_name": "Cropping1D", "config": {"name": "cropping1d_1", "trainable": True, "cropping": [1, 1]},
         "inbound_nodes": [[["zero_padding1d_1", 0, 0, {}]]]},
        {"name": "dense_2", "class_name": "Dense", "config": head, "inbound_nodes": [[["cropping1d_1", 0, 0, {}]]]},
    ]
    text = json.dumps({"class_name": "Model", "config": {"name": "model_1", "layers": layers, "input_layers": [["input_1", 0, 0]],
                                                        "output_layers": [["dense_2", 0, 0]]}, "keras_version": "2.2.4", "backend": "tensorflow"})
    m = model_from_json(text)
    assert [type(n.layer).__name__ for n in m.nodes] == ['RepeatVector', 'TimeDistributed', 'Permute', 'ZeroPadding1D', 'Cropping1D', 'Dense']
    assert [n.out_shape for n in m.nodes] == [(7, 5), (7, 3), (3, 7), (6, 7), (4, 7), (4, 4)]
    td = m.nodes[1].layer
    assert [p.name for p in td.weights] == ['time_distributed_1/kernel', 'time_distributed_1/bias'] and td.layer.name == 'dense_1'
    assert m.nodes[3].layer.padding == (2, 1) and m.nodes[4].layer.cropping == (1, 1) and m.nodes[2].layer.dims == (2, 1)
    with pytest.raises(NotImplementedError, match='Conv1D'):
        conv = {"name": "conv1d_1", "trainable": True, "filters": 4, "kernel_size": [3], "strides": [1], "padding": "valid", "activation": "linear",
                "use_bias": True}
        bad = [dict(l) for l in layers]
        bad[2] = dict(bad[2], config={"name": "time_distributed_1", "trainable": True, "layer": {"class_name": "Conv1D", "config": conv}})
        model_from_json(json.dumps({"class_name": "Model", "config": {"name": "model_1", "layers": bad, "input_layers": [["input_1", 0, 0]],
                                                                     "output_layers": [["dense_2", 0, 0]]}}))


def test_h5_round_trip_on_the_host_stores_the_wrappers_weights_under_keras_names(tmp_path):
    from gennet_amd import h5lite
    from gennet_amd.keras.models import load_model
    m = sequence_model()
    rng = np.random.RandomState(3)
    m.set_weights([rng.randn(*w.shape).astype(np.float32) for w in m.get_weights()])
    path = str(tmp_path / 'sequence.h5')
    m.save(path, True)
    g = h5lite.File(path)['model_weights']['heads']
    td = [l for l in m.layers if l.name == 'heads'][0]
    assert [n.decode() if isinstance(n, bytes) else n for n in np.asarray(g.attrs['weight_names']).ravel().tolist()] == ['heads/kernel:0', 'heads/bias:0']
    assert np.array_equal(g['heads/kernel:0'].value, td.layer.kernel.numpy()) and np.array_equal(g['heads/bias:0'].value, td.layer.bias.numpy())
    again = load_model(path)
    assert json.loads(again.to_json()) == json.loads(m.to_json())
    assert all(np.array_equal(a, b) for a, b in zip(m.get_weights(), again.get_weights()))


# ---- sequence_ref.py against torch -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(3, 5), (2, 3, 4), (2, 5, 7, 6), (4, 13, 1)])
def test_the_permute_reference_is_torch_permute(shape):
    rng = np.random.RandomState(len(shape))
    x = rng.randn(*shape).astype(np.float32)
    for perm in itertools.permutations(range(len(shape))):
        y = S.permute_fwd(x, perm)
        assert y.dtype == np.float32 and np.array_equal(y, torch.tensor(x).permute(*perm).contiguous().numpy())
        assert np.array_equal(S.permute_fwd(y, S.inverse_perm(perm)), x)
        t = torch.tensor(x.astype(np.float64), requires_grad=True)
        g = rng.randn(*y.shape)
        t.permute(*perm).backward(torch.tensor(g))
        assert np.array_equal(S.permute_bwd(g, perm), t.grad.numpy())
        assert np.array_equal(S.permute_bwd(g, perm), S.permute_fwd(g, S.inverse_perm(perm)))


@pytest.mark.parametrize('B,L,C', [(3, 5, 3), (2, 5, 8), (1, 1, 4)])
@pytest.mark.parametrize('left,right', [(0, 0), (2, 0), (0, 3), (1, 2)])
def test_the_pad_and_crop_references_are_torch_pad_and_slicing(B, L, C, left, right):
    rng = np.random.RandomState(B + L + C)
    x = rng.randn(B, L, C).astype(np.float32)
    y = S.pad_fwd(x, left, right)
    assert np.array_equal(y, F.pad(torch.tensor(x), (0, 0, left, right)).numpy()) and not np.signbit(y[:, :left]).any() and not np.signbit(y[:, left + L:]).any()
    assert np.array_equal(S.crop_fwd(y, left, right), x)
    t = torch.tensor(x.astype(np.float64), requires_grad=True)
    g = rng.randn(*y.shape)
    F.pad(t, (0, 0, left, right)).backward(torch.tensor(g))
    assert np.array_equal(S.pad_bwd(g, left, right), t.grad.numpy())
    if L - left - right >= 1:
        c = S.crop_fwd(x, left, right)
        assert np.array_equal(c, x[:, left:L - right])
        t = torch.tensor(x.astype(np.float64), requires_grad=True)
        g = rng.randn(*c.shape)
        t[:, left:L - right].backward(torch.tensor(g))
        assert np.array_equal(S.crop_bwd(g, left, right), t.grad.numpy())


@pytest.mark.parametrize('B,C,n', [(3, 5, 1), (3, 5, 7), (2, 64, 130), (1, 3, 4100)])
def test_the_repeat_reference_is_torch_expand(B, C, n):
    rng = np.random.RandomState(n)
    x = rng.randn(B, C).astype(np.float32)
    y = S.repeat_fwd(x, n)
    assert np.array_equal(y, torch.tensor(x)[:, None, :].expand(B, n, C).contiguous().numpy())
    t = torch.tensor(x.astype(np.float64), requires_grad=True)
    g = rng.randn(B, n, C).astype(np.float32)
    t[:, None, :].expand(B, n, C).backward(torch.tensor(g.astype(np.float64)))
    got, ref = S.repeat_bwd(g), t.grad.numpy()
    # two float64 sums of the same n terms in different orders: each within n 2^-53 sum|g| of the exact sum
    assert got.dtype == np.float64 and (np.abs(got - ref) <= 2 * n * 2.0 ** -53 * np.abs(g.astype(np.float64)).sum(1)).all()


@pytest.mark.parametrize('shape,units', [((3, 7, 6), 5), ((2, 3, 4, 6), 2), ((4, 6), 3)])
def test_the_dense_reference_is_torch_matmul(shape, units):
    rng = np.random.RandomState(units)
    x, w, b = rng.randn(*shape), rng.randn(shape[-1], units), rng.randn(units)
    tx, tw, tb = (torch.tensor(v, requires_grad=True) for v in (x, w, b))
    out = tx @ tw + tb
    g = rng.randn(*out.shape)
    out.backward(torch.tensor(g))
    assert np.allclose(S.dense_fwd(x, w, b), out.detach().numpy(), rtol=0, atol=1e-13)
    for got, ref in zip(S.dense_bwd(x, w, g), (tx.grad, tw.grad, tb.grad)):
        assert np.allclose(got, ref.numpy(), rtol=0, atol=1e-12)


def test_the_torch_forms_of_the_reference_carry_its_own_gradients():
    rng = np.random.RandomState(9)
    x = torch.tensor(rng.randn(2, 5, 4), requires_grad=True)
    w, b = torch.tensor(rng.randn(4, 3), requires_grad=True), torch.tensor(rng.randn(3), requires_grad=True)
    y = S.torch_dense(S.torch_crop(S.torch_pad(S.torch_permute(S.torch_permute(x, (0, 2, 1)), (0, 2, 1)), 2, 1), 1, 0), w, b)
    z = S.torch_repeat(y[:, 0, :], 3)
    (y.sum() * 2 + (z * z).sum()).backward()
    x2, w2, b2 = (torch.tensor(v.detach().numpy(), requires_grad=True) for v in (x, w, b))
    y2 = F.pad(x2, (0, 0, 2, 1))[:, 1:] @ w2 + b2
    z2 = y2[:, 0, :][:, None, :].expand(2, 3, 3)
    (y2.sum() * 2 + (z2 * z2).sum()).backward()
    for a, r in ((x, x2), (w, w2), (b, b2)):
        assert np.allclose(a.grad.numpy(), r.grad.numpy(), rtol=0, atol=1e-12)


# ---- the entry points before any launch -------------------------------------------------------------------------------------------------------
def ints(*v):
    return (ctypes.c_int * len(v))(*v)


def test_the_header_declares_the_entry_points():
    from gennet_amd import _lib
    want = {'gn_permute': (_lib.i32, [_lib.vp, _lib.vp, _lib.vp, _lib.vp, _lib.i32, _lib.vp]),
            'gn_repeat_fwd': (_lib.i32, [_lib.vp, _lib.vp, _lib.i32, _lib.i32, _lib.i32, _lib.vp]),
            'gn_repeat_bwd_workspace': (_lib.sz, [_lib.i32] * 3),
            'gn_repeat_bwd': (_lib.i32, [_lib.vp, _lib.vp, _lib.vp, _lib.sz, _lib.i32, _lib.i32, _lib.i32, _lib.vp]),
            'gn_shift1d': (_lib.i32, [_lib.vp, _lib.vp] + [_lib.i32] * 5 + [_lib.vp])}
    for name, decl in want.items():
        assert _lib.DECLS[name] == decl, name
        assert hasattr(_lib.lib(), name), name


def test_the_entry_points_refuse_bad_arguments_before_any_launch():
    """no device is touched: the pointers are made-up addresses that a launch would fault on"""
    from gennet_amd import _lib
    L = _lib.lib()
    X, Y = 0x10000, 0x20000

    def refused(name, *args):
        rc = getattr(L, name)(*args)
        text = L.gn_last_error().decode()
        assert rc == _lib.GN_EINVAL and text, (name, args, rc, text)
        return text

    ext, perm = ints(2, 3, 4), ints(0, 2, 1)
    assert 'null' in refused('gn_permute', None, Y, ext, perm, 3, None)
    assert 'null' in refused('gn_permute', X, None, ext, perm, 3, None)
    assert 'null' in refused('gn_permute', X, Y, None, perm, 3, None)
    assert 'null' in refused('gn_permute', X, Y, ext, None, 3, None)
    assert 'out of place' in refused('gn_permute', X, X, ext, perm, 3, None)
    for R in (-1, 0, 1, 5):
        assert 'rank' in refused('gn_permute', X, Y, ints(2, 3, 4, 5, 6), ints(0, 1, 2, 3, 4), R, None)
    for bad in ((0, 1, 1), (0, 1, 3), (0, -1, 2), (1, 1, 1)):
        assert 'not a permutation' in refused('gn_permute', X, Y, ext, ints(*bad), 3, None)
    assert 'negative' in refused('gn_permute', X, Y, ints(2, -3, 4), perm, 3, None)
    assert 'negative' in refused('gn_permute', X, Y, ints(-2, 3), ints(1, 0), 2, None)
    assert '2^61' in refused('gn_permute', X, Y, ints(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1), perm, 3, None)
    assert L.gn_permute(X, Y, ints(0, 3, 4), perm, 3, None) == _lib.GN_OK                      # nothing to move: no launch

    assert 'null' in refused('gn_repeat_fwd', None, Y, 2, 3, 4, None) and 'null' in refused('gn_repeat_fwd', X, None, 2, 3, 4, None)
    assert 'null' in refused('gn_repeat_bwd', None, Y, None, 0, 2, 3, 4, None) and 'null' in refused('gn_repeat_bwd', X, None, None, 0, 2, 3, 4, None)
    for B, n, C in ((-1, 3, 4), (2, 0, 4), (2, 3, 0), (2, -3, 4), (2, 3, -4), (2, 2 ** 16, 2 ** 15)):
        refused('gn_repeat_fwd', X, Y, B, n, C, None)
        refused('gn_repeat_bwd', X, Y, None, 0, B, n, C, None)
    assert L.gn_repeat_fwd(X, Y, 0, 3, 4, None) == _lib.GN_OK and L.gn_repeat_bwd(X, Y, None, 0, 0, 3, 4, None) == _lib.GN_OK
    # a split sum needs its workspace: (1, 4100, 3) is summed in parts, (3, 7, 5) is not
    need = L.gn_repeat_bwd_workspace(1, 4100, 3)
    assert need > 0 and need % (3 * 8) == 0 and L.gn_repeat_bwd_workspace(3, 7, 5) == 0 and L.gn_repeat_bwd_workspace(0, 7, 5) == 0
    assert 'workspace' in refused('gn_repeat_bwd', X, Y, None, 0, 1, 4100, 3, None)
    assert 'workspace' in refused('gn_repeat_bwd', X, Y, 0x30004, need, 1, 4100, 3, None)          # not 8-byte aligned
    assert L.gn_repeat_bwd(X, Y, 0x30000, need - 1, 1, 4100, 3, None) == _lib.GN_EWORKSPACE

    assert 'null' in refused('gn_shift1d', None, Y, 2, 5, 7, 3, 1, None) and 'null' in refused('gn_shift1d', X, None, 2, 5, 7, 3, 1, None)
    assert 'out of place' in refused('gn_shift1d', X, X, 2, 5, 7, 3, 1, None)
    for B, Lin, Lout, C in ((-1, 5, 7, 3), (2, 0, 7, 3), (2, 5, 0, 3), (2, 5, 7, 0), (2, -5, 7, 3), (2, 5, -7, 3), (2, 5, 7, -3)):
        refused('gn_shift1d', X, Y, B, Lin, Lout, C, 1, None)
    assert L.gn_shift1d(X, Y, 0, 5, 7, 3, 1, None) == _lib.GN_OK


def test_the_split_of_the_repeat_gradient_depends_on_the_shape_alone():
    """gn_repeat_bwd_workspace = parts * B * C * 8 bytes for parts > 1: at most 64 parts, none below 32 terms a part or from 65536 elements of dx on"""
    from gennet_amd import _lib
    L = _lib.lib()

    def parts(B, n, C):
        ws = L.gn_repeat_bwd_workspace(B, n, C)
        return ws // (B * C * 8) if ws else 1

    assert parts(1, 4100, 3) == 64 and parts(3, 130, 5) == 4 and parts(2, 130, 64) == 4 and parts(3, 7, 5) == 1 and parts(2, 63, 64) == 1
    assert parts(64, 256, 128) == 8 and parts(64, 256, 1024) == 1 and parts(1, 64, 1) == 2
