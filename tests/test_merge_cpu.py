"""CPU-only checks of the merge layers (no kernel runs): tests/merge_ref.py against torch autograd in fp64 and against the tie rule itself;
shape inference, refusals, the planner around a node with several inbound edges, the Keras 2.2.4 config round trip, and the C ABI of
csrc/merge.hip as gennet_amd/_lib.py reads it from the header."""
import json

import numpy as np
import pytest
import torch

import merge_ref as R

EPS = 2.0 ** -24


def _inputs(rng, k, shape, scale=1.0):
    """k float32 arrays without ties (and without zeros: the product's gradient divides nothing, but |x| > 0.05 keeps every bound relative)"""
    xs = [(rng.uniform(0.05, 2.0, shape) * rng.choice([-1.0, 1.0], shape) * scale).astype(np.float32) for _ in range(k)]
    st = np.sort(np.stack(xs), axis=0)
    assert (st[1:] != st[:-1]).all()
    return xs


def _torch_fwd(mode, ts):
    acc = ts[0]
    for t in ts[1:]:
        acc = {'add': torch.add, 'avg': torch.add, 'sub': torch.sub, 'mul': torch.mul, 'max': torch.maximum, 'min': torch.minimum}[mode](acc, t)
    return acc / len(ts) if mode == 'avg' else acc


@pytest.mark.parametrize('mode,k', [(m, k) for m in R.MODES for k in (2, 3, 8) if m != 'sub' or k == 2])        # Subtract takes exactly two inputs
def test_reference_against_torch_autograd_in_fp64(mode, k):
    """fp32 left-to-right chains against the fp64 value: a sum of k terms is within (k - 1) 2^-24 of sum |x_j| (+ one rounding of the division),
    a product within (k - 1) roundings relative; a maximum is a copy (exact).  The gradients: dy times a product of k - 1 factors, k - 1
    roundings relative; copies and +0 for max / min; one rounding of 1 / k and one of the product for avg."""
    rng = np.random.RandomState(100 * k + R.MODES.index(mode))
    xs = _inputs(rng, k, (257,))
    dy = rng.randn(257).astype(np.float32)
    ts = [torch.tensor(x.astype(np.float64), requires_grad=True) for x in xs]
    y64 = _torch_fwd(mode, ts)
    y64.backward(torch.tensor(dy.astype(np.float64)))
    y = R.merge_fwd(mode, xs)
    assert y.dtype == np.float32 and y.shape == (257,)
    mag = np.sum([np.abs(x.astype(np.float64)) for x in xs], axis=0)
    if mode in ('max', 'min'):
        assert np.array_equal(y, y64.detach().numpy().astype(np.float32))
    elif mode == 'mul':
        assert (np.abs(y - y64.detach().numpy()) <= k * EPS * np.abs(y64.detach().numpy())).all()
    else:
        assert (np.abs(y - y64.detach().numpy()) <= (k + 1) * EPS * mag).all()
    for i in range(k):
        g = R.merge_bwd(mode, dy, xs, i)
        g64 = ts[i].grad.numpy()
        assert g.dtype == np.float32
        if mode in ('max', 'min', 'add', 'sub'):
            assert np.array_equal(g, g64.astype(np.float32)), (mode, i)
            if mode in ('max', 'min'):
                assert not np.signbit(g[g == 0]).any()                  # the losers get +0, whatever the sign of dy
        else:
            assert (np.abs(g - g64) <= (k + 1) * EPS * np.abs(g64)).all(), (mode, i)
    if mode in ('max', 'min'):
        assert np.array_equal(sum(R.merge_bwd(mode, dy, xs, i) for i in range(k)), dy)      # exactly one winner per element


def test_tie_rule_on_a_hand_written_example():
    """Three inputs, every tie pattern.  Keras chains out = K.maximum(K.maximum(x0, x1), x2); TensorFlow gives `out` the gradient where
    out >= x_j, so the whole dy lands on the FIRST input at the extremum (torch.maximum would split it evenly)."""
    x0 = np.array([1.0, 2.0, 5.0, 3.0, 0.0, -0.0, 7.0], np.float32)
    x1 = np.array([1.0, 1.0, 5.0, 4.0, -0.0, 0.0, 6.0], np.float32)
    x2 = np.array([1.0, 2.0, 4.0, 4.0, 0.0, 0.0, 7.0], np.float32)
    dy = np.array([10.0, 20.0, 30.0, 40.0, 50.0, 60.0, -70.0], np.float32)
    # maximum: all tied -> 0;  x0 = x2 -> 0;  x0 = x1 -> 0;  x1 = x2 -> 1;  +-0 all tied -> 0;  x0 = x2 -> 0
    assert R.first_extremum('max', [x0, x1, x2]).tolist() == [0, 0, 0, 1, 0, 0, 0]
    assert np.array_equal(R.merge_fwd('max', [x0, x1, x2]), np.array([1, 2, 5, 4, 0, -0.0, 7], np.float32))
    assert np.signbit(R.merge_fwd('max', [x0, x1, x2])).tolist() == [False] * 5 + [True, False]         # the earlier zero's sign stays
    assert np.array_equal(R.merge_bwd('max', dy, [x0, x1, x2], 0), np.array([10, 20, 30, 0, 50, 60, -70], np.float32))
    assert np.array_equal(R.merge_bwd('max', dy, [x0, x1, x2], 1), np.array([0, 0, 0, 40, 0, 0, 0], np.float32))
    assert np.array_equal(R.merge_bwd('max', dy, [x0, x1, x2], 2), np.zeros(7, np.float32))
    # minimum: all tied -> 0;  x1 alone -> 1;  x2 alone -> 2;  x0 alone -> 0;  zeros -> 0, 0;  x1 alone -> 1
    assert R.first_extremum('min', [x0, x1, x2]).tolist() == [0, 1, 2, 0, 0, 0, 1]
    assert np.array_equal(R.merge_bwd('min', dy, [x0, x1, x2], 2), np.array([0, 0, 30, 0, 0, 0, 0], np.float32))
    # the same rule written as TensorFlow's two-step chain
    out1 = np.maximum(x0, x1)
    g_out1, g_x2 = np.where(out1 >= x2, dy, 0), np.where(out1 >= x2, 0, dy)
    g_x0, g_x1 = np.where(x0 >= x1, g_out1, 0), np.where(x0 >= x1, 0, g_out1)
    for i, g in enumerate((g_x0, g_x1, g_x2)):
        assert np.array_equal(R.merge_bwd('max', dy, [x0, x1, x2], i), g.astype(np.float32))


def test_average_and_product_orders():
    """(x0 + x1 + x2) / 3 with the sum formed left to right in fp32 and one division -- not a sum of thirds, not a pairwise sum"""
    x = [np.array([1e8], np.float32), np.array([1.0], np.float32), np.array([-1e8], np.float32)]
    assert R.merge_fwd('avg', x)[0] == np.float32(0.0) and R.merge_fwd('add', x[::-1])[0] == np.float32(0.0)
    assert R.merge_fwd('add', [x[0], x[2], x[1]])[0] == np.float32(1.0)
    y = [np.array([3e38], np.float32), np.array([1e-30], np.float32), np.array([10.0], np.float32)]
    assert np.isfinite(R.merge_fwd('mul', y))[0] and np.isinf(R.merge_fwd('mul', [y[0], y[2], y[1]]))[0]
    assert R.merge_bwd('mul', np.ones(1, np.float32), y, 1)[0] == np.float32(np.inf)          # dy * (x0 * x2)
    assert R.merge_bwd('avg', np.float32([3.0]), x, 1)[0] == np.float32(3.0) * (np.float32(1.0) / np.float32(3.0))


@pytest.mark.parametrize('shapes,axis', [([(2, 5, 1), (2, 5, 1)], -1), ([(3, 5, 4), (3, 5, 8)], 2), ([(3, 5, 4), (3, 7, 4)], 1),
                                         ([(2, 3, 6), (2, 3, 3), (2, 3, 1)], -1), ([(2, 3, 2, 2), (2, 1, 2, 2)], -3)])
def test_concat_reference_against_torch(shapes, axis):
    rng = np.random.RandomState(len(shapes))
    xs = [rng.randn(*s).astype(np.float32) for s in shapes]
    ts = [torch.tensor(x.astype(np.float64), requires_grad=True) for x in xs]
    y64 = torch.cat(ts, dim=axis)
    y = R.concat_fwd(xs, axis)
    assert y.dtype == np.float32 and np.array_equal(y, y64.detach().numpy().astype(np.float32))
    dy = rng.randn(*y.shape).astype(np.float32)
    y64.backward(torch.tensor(dy.astype(np.float64)))
    for g, t in zip(R.concat_bwd(dy, shapes, axis), ts):
        assert g.dtype == np.float32 and np.array_equal(g, t.grad.numpy().astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------------
# layers on the host: shapes, refusals, the planner, configs
# ---------------------------------------------------------------------------------------------------------------------
ELEMENTWISE = ['Add', 'Subtract', 'Multiply', 'Average', 'Maximum', 'Minimum']


def test_shape_inference_and_names():
    from gennet_amd import layers as Ly
    from gennet_amd.engine import Input, Model
    from gennet_amd.keras import layers as KL
    from gennet_amd.keras.layers import merge as KM
    a, b, c = Input((5, 4)), Input((5, 4)), Input((5, 4))
    for name in ELEMENTWISE:
        cls = getattr(Ly, name)
        assert getattr(KL, name) is cls and getattr(KM, name) is cls and getattr(KM, name.lower()) is getattr(Ly, name.lower())
        layer = cls()
        assert layer.name.rsplit('_', 1)[0] == name.lower() and layer.is_merge and not layer.weights
        t = layer([a, b])
        assert t.shape == (5, 4) and t.inbound == (a, b) and t.layer is layer
        if name != 'Subtract':
            assert cls()([a, b, c]).shape == (5, 4) and cls()((a, a)).shape == (5, 4)
        f = getattr(Ly, name.lower())([a, b], name='joined_' + name)
        assert f.shape == (5, 4) and type(f.layer) is cls and f.layer.name == 'joined_' + name
    assert KM.Concatenate is Ly.Concatenate and KL.concatenate is Ly.concatenate
    assert Ly.Concatenate().name.startswith('concatenate_') and Ly.Concatenate().axis == -1
    x3, y3, z4 = Input((5, 4)), Input((7, 4)), Input((5, 8))
    for axis, ins, want in [(-1, [x3, z4], (5, 12)), (2, [x3, z4, x3], (5, 16)), (1, [x3, y3], (12, 4)), (-2, [y3, x3, y3], (19, 4)), (-1, [x3, x3], (5, 8))]:
        assert Ly.Concatenate(axis=axis)(ins).shape == want
        assert Ly.concatenate(ins, axis=axis).shape == want
    p, q = Input((3, 2, 2)), Input((1, 2, 2))
    assert Ly.Concatenate(axis=1)([p, q]).shape == (4, 2, 2) and Ly.Concatenate(axis=-3)([p, q]).shape == (4, 2, 2)
    flat = Ly.concatenate([Input((6,)), Input((3,)), Input((1,))])
    assert flat.shape == (10,)
    # Multiply()([t, t]): the same tensor on two edges
    t = Ly.Dense(4)(Input((3,)))
    m = Model(inputs=t.inbound[0], outputs=Ly.Multiply()([t, t]))
    assert m.nodes[-1].inbound == [0, 0] and m.output_shape == (None, 4)


def test_refusals():
    from gennet_amd import layers as Ly
    from gennet_amd import ops
    from gennet_amd.engine import Input
    a, b = Input((5, 4)), Input((5, 4))
    for cls in [getattr(Ly, n) for n in ELEMENTWISE] + [Ly.Concatenate]:
        for bad in (a, [a], (a,)):
            with pytest.raises(ValueError, match='at least 2 inputs'):
                cls()(bad)
    for layer in (Ly.Dense(3), Ly.Flatten(), Ly.Activation('tanh'), Ly.Conv1D(4, 3)):
        with pytest.raises(ValueError, match='single tensor'):
            layer([a, b])
    with pytest.raises(ValueError) as e:
        Ly.Add()([a, Input((5, 3))])
    assert '(None, 5, 4)' in str(e.value) and '(None, 5, 3)' in str(e.value)
    with pytest.raises(ValueError) as e:                                   # no broadcasting between ranks
        Ly.Multiply()([a, Input((4,))])
    assert '(None, 5, 4)' in str(e.value) and '(None, 4)' in str(e.value)
    with pytest.raises(ValueError) as e:                                   # equal except along the axis
        Ly.Concatenate(axis=-1)([a, Input((6, 4))])
    assert '(None, 5, 4)' in str(e.value) and '(None, 6, 4)' in str(e.value)
    with pytest.raises(ValueError, match='exactly 2 inputs'):
        Ly.Subtract()([a, b, a])
    assert ops.MERGE_MAX_INPUTS == 8
    assert Ly.Add()([a] * 8).shape == (5, 4) and Ly.Concatenate()([a] * 8).shape == (5, 32)
    for cls in (Ly.Add, Ly.Maximum, Ly.Concatenate):
        with pytest.raises(ValueError, match='at most 8'):
            cls()([a] * 9)
    with pytest.raises(ValueError, match='batch axis'):
        Ly.Concatenate(axis=0)
    for axis in (3, -3, 7):
        with pytest.raises(ValueError, match='axis'):
            Ly.Concatenate(axis=axis)([a, b])
    with pytest.raises(ValueError):
        Ly.Concatenate(axis=1.0)


def test_planner_around_a_merge_node():
    """No fusion reaches through a merge node, and Conv1D -> Activation -> Add keeps its fused epilogue."""
    from gennet_amd import layers as Ly
    from gennet_amd.engine import Input, Model
    x = Input((16, 8))
    c = Ly.Conv1D(8, 5, padding='same')(x)
    act = Ly.Activation('tanh')(c)
    s = Ly.Add()([act, x])
    drop = Ly.Dropout(0.2)(s)                                              # behind the merge: nothing absorbs it
    bn = Ly.BatchNormalization()(Ly.Add()([Ly.Conv1D(8, 5, padding='same')(drop), drop]))     # conv -> merge -> BN: no inference-phase fold
    up = Ly.UpSampling1D()(Ly.Multiply()([bn, bn]))
    head = Ly.Dense(1)(Ly.Flatten()(Ly.Maximum()([Ly.Conv1D(8, 5, padding='same', activation='relu')(up), up])))
    m = Model(inputs=x, outputs=head)
    m._plan()
    conv0, act0, add0 = m.nodes[0], m.nodes[1], m.nodes[2]
    assert conv0.fused_act == ('tanh', 0.0) and act0.absorbed and add0.inbound == [1, -1] and not add0.absorbed
    merges = [n for n in m.nodes if n.layer.is_merge]
    assert len(merges) == 4 and all(not n.absorbed and n.fused_act is None and n.fused_drop is None and n.fuse_prev < 0 and n.fold_up is None
                                    and n.infer_bn is None and n.lazy_bn < 0 for n in merges)
    for n in m.nodes:
        kind = type(n.layer).__name__
        if kind in ('Dropout', 'BatchNormalization', 'UpSampling1D', 'Flatten', 'Dense'):
            assert not n.absorbed, kind
        if kind == 'Conv1D' and n is not conv0:
            assert n.fused_act is None and n.fused_drop is None and n.infer_bn is None and n.fold_up is None and n.fuse_prev < 0 and n.lazy_bn < 0
        if kind == 'Dense':                                                # its producer chain ends at a merge node: no producer backward to absorb
            assert n.fuse_prev < 0
    # which epilogue overwrites the gradient it is handed: the engine copies a shared dy only for these
    assert conv0.layer.writes_dy(conv0) and not add0.layer.writes_dy(add0)
    lin = [n for n in m.nodes if type(n.layer).__name__ == 'Conv1D' and n.layer.activation[0] == 'linear' and n is not conv0]
    assert lin and not any(n.layer.writes_dy(n) for n in lin)


def _cfg_conv1d(name, filters, k):
    return {'name': name, 'trainable': True, 'filters': filters, 'kernel_size': [k], 'strides': [1], 'padding': 'same', 'data_format': 'channels_last',
            'dilation_rate': [1], 'activation': 'linear', 'use_bias': True,
            'kernel_initializer': {'class_name': 'VarianceScaling', 'config': {'scale': 1.0, 'mode': 'fan_avg', 'distribution': 'uniform', 'seed': None}},
            'bias_initializer': {'class_name': 'Zeros', 'config': {}}, 'kernel_regularizer': None, 'bias_regularizer': None,
            'activity_regularizer': None, 'kernel_constraint': None, 'bias_constraint': None}


def _cfg_input(name, shape):
    return {'name': name, 'class_name': 'InputLayer', 'inbound_nodes': [],
            'config': {'batch_input_shape': [None] + list(shape), 'dtype': 'float32', 'sparse': False, 'name': name}}


def test_config_round_trip_in_keras_layout():
    """A functional-model config written by hand as Keras 2.2.4 writes it (model.to_json()): two InputLayers, a Conv1D branch, Subtract and
    Concatenate(axis=-1) with two inbound references each, layers in keras' depth order."""
    from gennet_amd import keras_io
    from gennet_amd import layers as Ly
    from gennet_amd.engine import model_from_json
    cfg = {'class_name': 'Model', 'config': {
        'name': 'stacked', 'layers': [
            _cfg_input('z_in', (16, 1)),
            {'name': 'g_conv', 'class_name': 'Conv1D', 'config': _cfg_conv1d('g_conv', 1, 5), 'inbound_nodes': [[['z_in', 0, 0, {}]]]},
            _cfg_input('event_in', (16, 1)),
            {'name': 'subtract_7', 'class_name': 'Subtract', 'config': {'name': 'subtract_7', 'trainable': True},
             'inbound_nodes': [[['event_in', 0, 0, {}], ['g_conv', 0, 0, {}]]]},
            {'name': 'concatenate_7', 'class_name': 'Concatenate', 'config': {'name': 'concatenate_7', 'trainable': True, 'axis': -1},
             'inbound_nodes': [[['g_conv', 0, 0, {}], ['subtract_7', 0, 0, {}]]]}],
        'input_layers': [['z_in', 0, 0], ['event_in', 0, 0]], 'output_layers': [['concatenate_7', 0, 0]]}}
    model = model_from_json(json.dumps(cfg))
    assert keras_io.model_config(model) == cfg
    assert json.loads(model.to_json()) == cfg
    assert [type(n.layer).__name__ for n in model.nodes] == ['Conv1D', 'Subtract', 'Concatenate']
    assert [n.inbound for n in model.nodes] == [[-1], [-2, 0], [0, 1]] and model.output_shape == (None, 16, 2)
    assert model.input_shapes == [(16, 1), (16, 1)]
    for name in ELEMENTWISE:                                               # the six element-wise layers: the base config only
        layer = getattr(Ly, name)(name='m')
        assert layer.get_config() == {'name': 'm', 'trainable': True}
        again = keras_io._layer_from_config(name, layer.get_config(), None)
        assert type(again) is type(layer) and again.name == 'm'
    c = keras_io._layer_from_config('Concatenate', {'name': 'c', 'trainable': True, 'axis': 1}, None)
    assert type(c) is Ly.Concatenate and c.axis == 1 and c.get_config() == {'name': 'c', 'trainable': True, 'axis': 1}
    # a list on a layer that takes one tensor is refused on load, too
    bad = json.loads(json.dumps(cfg))
    bad['config']['layers'][3]['class_name'] = 'Flatten'
    bad['config']['layers'][3]['config'] = {'name': 'subtract_7', 'trainable': True, 'data_format': 'channels_last'}
    with pytest.raises(ValueError, match='single tensor'):
        model_from_json(json.dumps(bad))


def test_symbols_and_enum_codes_come_from_the_header():
    from gennet_amd import _lib, ops
    from gennet_amd._lib import f32, i32, sz, vp
    assert _lib.DECLS['gn_merge_fwd'] == (i32, [i32, vp, i32, vp, sz, vp])
    assert _lib.DECLS['gn_merge_bwd'] == (i32, [i32, vp, vp, i32, i32, vp, sz, vp])
    assert _lib.DECLS['gn_scale'] == (i32, [vp, f32, vp, sz, vp])
    assert _lib.DECLS['gn_concat_fwd'] == (i32, [vp, vp, i32, vp, sz, vp])
    assert _lib.DECLS['gn_concat_bwd'] == (i32, [vp, vp, vp, i32, sz, vp])
    assert [(k, v) for k, v in _lib.CONSTS.items() if k.startswith('GN_MERGE_')] == [
        ('GN_MERGE_MAX_INPUTS', 8), ('GN_MERGE_ADD', 0), ('GN_MERGE_SUB', 1), ('GN_MERGE_MUL', 2), ('GN_MERGE_AVG', 3), ('GN_MERGE_MAX', 4),
        ('GN_MERGE_MIN', 5)]
    assert ops.MERGE_MODES == {'add': 0, 'sub': 1, 'mul': 2, 'avg': 3, 'max': 4, 'min': 5} and ops.MERGE_MAX_INPUTS == 8
    assert tuple(ops.MERGE_MODES) == R.MODES
    L = _lib.lib()
    for name in ('gn_merge_fwd', 'gn_merge_bwd', 'gn_scale', 'gn_concat_fwd', 'gn_concat_bwd'):
        assert hasattr(L, name), name
