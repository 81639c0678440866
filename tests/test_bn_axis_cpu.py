"""CPU-only checks of BatchNormalization over any axis (layers.BatchNormalization(axis=...), csrc/bn_axis.hip) and of the planner's rule for a
layer's own activation followed by an activation layer: axis resolution and the (outer, P, inner) view, the fusion plan, the .h5 round trip
and the header's declarations.  No compute call: everything here is host logic."""
import json

import numpy as np
import pytest
import torch

from gennet_amd import _lib, engine, h5lite
from gennet_amd.engine import Sequential
from gennet_amd.layers import Activation, BatchNormalization, Conv1D, Conv2DTranspose, Dense, Dropout, Flatten, LeakyReLU, Reshape


def _built(axis, shape):
    bn = BatchNormalization(axis=axis)
    bn._ensure_built(shape)
    return bn


@pytest.mark.parametrize('shape, axis, view, last', [
    ((57, 6), 1, (1, 57, 6), False), ((57, 6), -2, (1, 57, 6), False), ((57, 6), 2, (57, 6, 1), True), ((57, 6), -1, (57, 6, 1), True),
    ((10, 1, 1), 1, (1, 10, 1), False), ((10, 1, 1), -3, (1, 10, 1), False),
    ((5, 7, 3), 1, (1, 5, 21), False), ((5, 7, 3), 2, (5, 7, 3), False), ((5, 7, 3), -2, (5, 7, 3), False), ((5, 7, 3), 3, (35, 3, 1), True),
    ((5, 7, 3), -1, (35, 3, 1), True), ((5, 7, 3), -3, (1, 5, 21), False)])
def test_axis_resolution_view_and_weight_shapes(shape, axis, view, last):
    bn = _built(axis, shape)
    assert bn.view == view and bn.axis == axis                     # (rows of outer per sample, P, inner); the axis stays as given
    P = view[1]
    assert [w.name.split('/')[-1] for w in bn.weights] == ['gamma', 'beta', 'moving_mean', 'moving_variance']
    assert all(w.shape == (P,) for w in bn.weights)
    assert bn.is_batchnorm is last and bn.fusable_act is last and bn.fusable_drop is last


@pytest.mark.parametrize('shape, axis', [((57, 6), 0), ((57, 6), 3), ((57, 6), -3), ((5, 7, 3), 0), ((5, 7, 3), 4), ((5, 7, 3), -4)])
def test_an_axis_outside_the_input_is_a_value_error_that_names_it(shape, axis):
    with pytest.raises(ValueError) as e:
        _built(axis, shape)
    assert ('axis=%d' % axis) in str(e.value) and str((None,) + shape) in str(e.value)


def _conv_bn_graph(axis):
    m = Sequential([Conv1D(8, 5, padding='same', input_shape=(32, 4)), BatchNormalization(axis=axis), Activation('tanh'), Dropout(0.2), Conv1D(1, 5, padding='same')])
    m._plan()
    return m, m.nodes


def test_plan_leaves_a_position_batchnorm_alone():
    m, nodes = _conv_bn_graph(1)
    conv, bn, act, drop, last = nodes
    assert conv.infer_bn is None and bn.fused_act is None and bn.fused_drop is None
    assert not any(n.absorbed for n in nodes) and all(n.lazy_bn == -1 for n in nodes)
    assert bn.layer.view == (1, 32, 8)


@pytest.mark.parametrize('axis', [-1, 2])
def test_plan_of_a_channel_batchnorm_is_unchanged(axis):
    m, nodes = _conv_bn_graph(axis)
    conv, bn, act, drop, last = nodes
    assert conv.infer_bn is bn and bn.fused_act == ('tanh', 0.0) and bn.fused_drop == (0.2, drop.layer)
    assert [n.absorbed for n in nodes] == [False, False, True, True, False] and last.lazy_bn == bn.index


def _pair_graphs():
    yield Sequential([Conv1D(8, 5, activation='tanh', input_shape=(32, 4)), LeakyReLU(0.2), Dropout(0.3)])
    yield Sequential([Dense(8, activation='tanh', input_shape=(16,)), LeakyReLU(0.2), Dropout(0.3)])
    yield Sequential([Conv2DTranspose(8, (1, 4), activation='relu', input_shape=(3, 5, 4)), LeakyReLU(0.2), Dropout(0.3)])


def test_plan_keeps_an_activation_layer_behind_a_layers_own_activation():
    for m in _pair_graphs():
        m._plan()
        layer, leaky, drop = m.nodes
        assert layer.fused_act is None and not leaky.absorbed, type(layer.layer).__name__
        assert layer.fused_drop is None and not drop.absorbed               # the Dropout follows the LeakyReLU node, which fuses nothing
    # a linear layer fuses as before: activation, then the Dropout behind it
    m = Sequential([Conv1D(8, 5, input_shape=(32, 4)), LeakyReLU(0.2), Dropout(0.3)])
    m._plan()
    conv, leaky, drop = m.nodes
    assert conv.fused_act == ('leaky', float(np.float32(0.2))) and leaky.absorbed and conv.fused_drop == (0.3, drop.layer) and drop.absorbed
    # and a Dropout directly behind a layer with its own activation still goes into that layer's epilogue
    m = Sequential([Conv1D(8, 5, activation='tanh', input_shape=(32, 4)), Dropout(0.3)])
    m._plan()
    assert m.nodes[0].fused_act is None and m.nodes[0].fused_drop == (0.3, m.nodes[1].layer) and m.nodes[1].absorbed


def test_h5_round_trip_keeps_the_axis_the_weights_and_the_zero_debias_section(tmp_path, monkeypatch):
    from gennet_amd.keras.models import load_model
    monkeypatch.setattr(engine, 'to_device', lambda a, dtype=torch.float32: torch.as_tensor(np.asarray(a), dtype=dtype))      # the section's tensors stay on the host
    rng = np.random.RandomState(5)
    m = Sequential([Reshape((-1, 1), input_shape=(24,)), Conv1D(6, 8), BatchNormalization(axis=1), BatchNormalization(), Flatten(), Dense(2)], name='pos_bn')
    bn1, bn2 = m.layers[2], m.layers[3]
    assert bn1.view == (1, 17, 6) and bn2.view == (17, 6, 1)
    for bn in (bn1, bn2):
        P = bn.view[1]
        bn.set_weights([rng.uniform(0.5, 1.5, P), rng.normal(0, 0.3, P), rng.normal(0, 0.5, P), rng.uniform(0.5, 2.0, P)])
    bn1.zero_debias = {'trainer': [torch.as_tensor(rng.normal(0, 1, 17), dtype=torch.float32), torch.as_tensor(rng.uniform(0, 1, 17), dtype=torch.float32), 4]}
    assert bn1.get_config()['axis'] == 1 and bn2.get_config()['axis'] == -1
    path = str(tmp_path / 'pos_bn.h5')
    m.save(path, True)
    cfg = json.loads(h5lite.File(path).attrs['model_config'].decode())
    assert [l['config']['axis'] for l in cfg['config']['layers'] if l['class_name'] == 'BatchNormalization'] == [1, -1]
    m2 = load_model(path)
    c1, c2 = m2.layers[2], m2.layers[3]
    assert c1.axis == 1 and c1.view == (1, 17, 6) and c2.axis == -1 and not c1.is_batchnorm and c2.is_batchnorm
    assert [w.shape for w in c1.weights] == [(17,)] * 4 and [w.shape for w in c2.weights] == [(6,)] * 4
    assert all(np.array_equal(a, b) for a, b in zip(m.get_weights(), m2.get_weights()))
    st, st0 = c1.zero_debias['trainer'], bn1.zero_debias['trainer']
    assert list(c1.zero_debias) == ['trainer'] and st[2] == 4 and torch.equal(st[0], st0[0]) and torch.equal(st[1], st0[1]) and st[0].shape == (17,)
    assert c2.zero_debias == {}


def test_header_declares_the_five_entry_points():
    want = {'gn_bn_axis_stats_workspace': (_lib.sz, 3), 'gn_bn_axis_stats': (_lib.i32, 8), 'gn_bn_axis_apply': (_lib.i32, 8),
            'gn_bn_axis_bwd_stats': (_lib.i32, 11), 'gn_bn_axis_bwd_apply': (_lib.i32, 17)}
    for name, (restype, nargs) in want.items():
        assert name in _lib.DECLS, name
        assert _lib.DECLS[name][0] is restype and len(_lib.DECLS[name][1]) == nargs, name
    assert _lib.DECLS['gn_bn_axis_stats'][1] == [_lib.vp, _lib.sz, _lib.i32, _lib.i32, _lib.vp, _lib.vp, _lib.sz, _lib.vp]
