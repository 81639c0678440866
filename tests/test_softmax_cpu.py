"""Host side of the softmax feature: the numpy definition against torch, the five spellings through configs, JSON and .h5, the
facade paths, the refusals, the C entry points' refusals (no launch, so no device), and what the planner does around a softmax: nothing."""
import json
import os

import numpy as np
import pytest
import torch

import softmax_models as M
import softmax_ref as R


# ---- the definition -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(5, 7), (4, 6, 5), (3, 4, 5, 6)], ids=['rank2', 'rank3', 'rank4'])
def test_the_definition_agrees_with_torch_on_every_axis(shape):
    rng = np.random.RandomState(len(shape))
    x = (3.0 * rng.randn(*shape)).astype(np.float32)
    dy = rng.randn(*shape).astype(np.float32)
    for axis in range(len(shape)):
        view = R.view_of(shape, axis)
        assert view == R.view_of(shape, axis - len(shape)) and int(np.prod(view)) == x.size and view[1] == shape[axis]
        xt = torch.tensor(x.astype(np.float64), requires_grad=True)
        yt = torch.softmax(xt, axis)
        yt.backward(torch.tensor(dy.astype(np.float64)))
        y, m, d = R.softmax_fwd(x, view)
        assert np.abs(y - yt.detach().numpy()).max() <= 1e-15
        assert np.array_equal(m, np.broadcast_to(x.astype(np.float64).max(axis=axis, keepdims=True), shape)) and np.array_equal(d, x - m)
        dx, mag = R.softmax_bwd(dy, yt.detach().numpy(), view)
        assert np.abs(dx - xt.grad.numpy()).max() <= 1e-15
        assert np.allclose(mag, np.broadcast_to(np.abs(dy * yt.detach().numpy()).sum(axis=axis, keepdims=True), shape), rtol=1e-14, atol=0)


def test_the_definition_on_rows_that_mix_the_largest_magnitudes():
    x = np.array([[3e38, -3e38, 0.0, 3e38], [-3e38, -3e38, -3e38, -3e38]], np.float32)
    y, _, _ = R.softmax_fwd(x, (2, 4, 1))
    assert np.array_equal(y, [[0.5, 0.0, 0.0, 0.5], [0.25, 0.25, 0.25, 0.25]])


# ---- the five spellings through config, JSON and .h5 ----------------------------------------------------------------------------------------
def _spellings():
    from gennet_amd import layers as L
    from gennet_amd.keras import activations
    return [('Dense', lambda: L.Dense(3, activation='softmax', input_shape=(6,), name='s')),
            ('Conv1D', lambda: L.Conv1D(8, 3, activation=activations.softmax, input_shape=(16, 4), name='s')),
            ('Conv2D', lambda: L.Conv2D(4, (5, 5), strides=(2, 1), padding='same', activation='softmax', input_shape=(8, 2, 4), name='s')),
            ('Conv2DTranspose', lambda: L.Conv2DTranspose(4, (1, 3), activation='softmax', input_shape=(1, 8, 4), name='s')),
            ('Activation', lambda: L.Activation('softmax', input_shape=(5, 6), name='s')),
            ('Softmax', lambda: L.Softmax(axis=1, input_shape=(5, 6), name='s'))]


def _is_softmax(layer):
    from gennet_amd import layers as L
    if isinstance(layer, L.Softmax):
        return layer.axis
    if isinstance(layer, L.Activation):
        return layer.softmax and layer.act_spec is None and -1
    return layer.activation == ('softmax', 0.0) and -1


@pytest.mark.parametrize('kind', [k for k, _ in _spellings()])
def test_every_spelling_round_trips_through_config_json_and_h5(kind, tmp_path):
    from gennet_amd import keras_io
    from gennet_amd.engine import Sequential, load_model, model_from_json
    make = dict(_spellings())[kind]
    layer = make()
    cfg = layer.get_config()
    assert (cfg['axis'] == 1) if kind == 'Softmax' else (cfg['activation'] == 'softmax')
    if kind == 'Softmax':
        assert cfg == {'name': 's', 'trainable': True, 'batch_input_shape': [None, 5, 6], 'dtype': 'float32', 'axis': 1}
    again = keras_io._layer_from_config(kind, json.loads(json.dumps(cfg)), None)
    assert type(again) is type(layer) and again.get_config() == cfg and _is_softmax(again) == (1 if kind == 'Softmax' else -1)
    model = Sequential([make()])
    want = (1 if kind == 'Softmax' else -1)
    m2 = model_from_json(model.to_json())
    assert json.loads(m2.to_json()) == json.loads(model.to_json()) and _is_softmax(m2.layers[0]) == want
    path = os.path.join(str(tmp_path), 'm.h5')
    model.save(path)
    m3 = load_model(path)
    assert json.loads(m3.to_json()) == json.loads(model.to_json()) and _is_softmax(m3.layers[0]) == want
    assert all(np.array_equal(u, v) for u, v in zip(model.get_weights(), m3.get_weights())) and m3.output_shape == model.output_shape


def test_a_hand_written_keras_json_with_a_softmax_head_loads():
    """as keras 2.2.4's Sequential.to_json() writes a classifier: the Dense config says "activation": "softmax", a Softmax layer its axis"""
    from gennet_amd import layers as L
    from gennet_amd.engine import model_from_json
    init = {'class_name': 'VarianceScaling', 'config': {'scale': 1.0, 'mode': 'fan_avg', 'distribution': 'uniform', 'seed': None}}
    dense = {'name': 'dense_1', 'trainable': True, 'batch_input_shape': [None, 10], 'dtype': 'float32', 'units': 4, 'activation': 'softmax',
             'use_bias': True, 'kernel_initializer': init, 'bias_initializer': {'class_name': 'Zeros', 'config': {}}, 'kernel_regularizer': None,
             'bias_regularizer': None, 'activity_regularizer': None, 'kernel_constraint': None, 'bias_constraint': None}
    text = json.dumps({'class_name': 'Sequential', 'config': {'name': 'sequential_1', 'layers': [
        {'class_name': 'Dense', 'config': dense}, {'class_name': 'Softmax', 'config': {'name': 'softmax_1', 'trainable': True, 'axis': -1}}]},
        'keras_version': '2.2.4', 'backend': 'tensorflow'})
    m = model_from_json(text)
    head, soft = m.layers
    assert type(head) is L.Dense and head.activation == ('softmax', 0.0) and head.units == 4 and type(soft) is L.Softmax and soft.axis == -1
    assert soft.view == (1, 4, 1) and m.output_shape == (None, 4)
    assert json.loads(m.to_json())['config']['layers'][0]['config'] == dense


def test_the_facade_paths_resolve_to_the_layers_classes():
    import gennet_amd.keras  # noqa: F401
    from gennet_amd import layers as L
    from gennet_amd.keras import activations
    from gennet_amd.keras.activations import linear, relu, sigmoid, softmax, tanh
    from gennet_amd.keras.layers import Softmax as top
    from gennet_amd.keras.layers.advanced_activations import Softmax as adv
    assert top is L.Softmax and adv is L.Softmax
    assert sorted(n for n in vars(activations) if not n.startswith('_')) == ['linear', 'relu', 'sigmoid', 'softmax', 'tanh']
    for fn, spec in ((softmax, 'softmax'), (relu, 'relu'), (tanh, 'tanh'), (sigmoid, 'sigmoid'), (linear, 'linear')):
        assert L.Dense(2, activation=fn).activation == (spec, 0.0) and L.Dense(2, activation=fn).get_config()['activation'] == spec
    assert L.Activation(softmax).softmax and L.Activation(relu).act_spec == ('relu', 0.0)
    with pytest.raises(NotImplementedError, match='softmax'):
        softmax(np.zeros((2, 3)))
    with pytest.raises(NotImplementedError, match='elu'):
        L.Dense(2, activation='elu')


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
def test_the_layers_refuse_what_keras_refuses_and_the_batch_axis():
    from gennet_amd import layers as L
    from gennet_amd.engine import Input
    with pytest.raises(ValueError, match=r'soft_1d \(Softmax\).*Cannot apply softmax to a tensor that is 1D'):
        L.Softmax(name='soft_1d')(Input(()))
    with pytest.raises(ValueError, match=r'act_1d \(Activation\).*Cannot apply softmax to a tensor that is 1D'):
        L.Activation('softmax', name='act_1d')(Input(()))
    for axis in (0, -3):
        with pytest.raises(ValueError, match=r'soft_b \(Softmax\).*batch axis.*across the samples.*across ranks'):
            L.Softmax(axis=axis, name='soft_b')(Input((5, 6)))
    for axis in (3, -4):
        with pytest.raises(ValueError, match=r'soft_r \(Softmax\).*axis %d .*1\.\.2 or -1\.\.-2' % axis):
            L.Softmax(axis=axis, name='soft_r')(Input((5, 6)))
    with pytest.raises(ValueError, match=r'soft_t \(Softmax\).*not one integer'):
        L.Softmax(axis=(1, 2), name='soft_t')
    ok = L.Softmax(axis=-2, name='soft_ok')
    assert ok(Input((5, 6))).shape == (5, 6) and ok.view == (1, 5, 6)
    assert L.Softmax(axis=2)(Input((5, 6))).layer.view == (5, 6, 1)


def test_the_entry_points_refuse_before_they_launch():
    """host-only checks: a refusal returns GN_EINVAL with its text and launches nothing, so it needs no device"""
    from gennet_amd import _lib
    L = _lib.lib()
    one = 4096          # stands for a pointer: never dereferenced on the host
    for args, text in (((None, one, 1, 2, 1, None), 'softmax_fwd: null pointer'), ((one, None, 1, 2, 1, None), 'softmax_fwd: null pointer'),
                       ((one, one, 0, 2, 1, None), 'softmax_fwd: bad shape (outer 0, P 2, inner 1)'),
                       ((one, one, 1, 0, 1, None), 'softmax_fwd: bad shape (outer 1, P 0, inner 1)'),
                       ((one, one, 1, 2, -1, None), 'softmax_fwd: bad shape (outer 1, P 2, inner -1)'),
                       ((one, one, 1, 65536, 32768, None), 'softmax_fwd: bad shape (outer 1, P 65536, inner 32768)'),
                       ((one, one, 1 << 40, 1 << 20, 1 << 10, None), 'softmax_fwd: bad shape (outer 1099511627776, P 1048576, inner 1024)')):
        assert L.gn_softmax_fwd(*args) == _lib.GN_EINVAL and L.gn_last_error().decode().startswith(text), (args, L.gn_last_error())
    for args, text in (((None, one, one, 1, 2, 1, None), 'softmax_bwd: null pointer'), ((one, None, one, 1, 2, 1, None), 'softmax_bwd: null pointer'),
                       ((one, one, None, 1, 2, 1, None), 'softmax_bwd: null pointer'),
                       ((one, one, one, 1, 1 << 16, 1 << 15, None), 'softmax_bwd: bad shape (outer 1, P 65536, inner 32768)')):
        assert L.gn_softmax_bwd(*args) == _lib.GN_EINVAL and L.gn_last_error().decode().startswith(text), (args, L.gn_last_error())


def test_softmax_is_no_activation_code_and_no_loss_kind():
    from gennet_amd import _lib, ops
    assert 'softmax' not in ops.ACT and 'softmax' not in ops.LOSS_KINDS and not any('SOFTMAX' in k for k in _lib.CONSTS)
    assert _lib.DECLS['gn_softmax_fwd'][1] == [_lib.vp, _lib.vp, _lib.sz, _lib.i32, _lib.i32, _lib.vp]
    assert _lib.DECLS['gn_softmax_bwd'][1] == [_lib.vp, _lib.vp, _lib.vp, _lib.sz, _lib.i32, _lib.i32, _lib.vp]


# ---- the planner ----------------------------------------------------------------------------------------------------------------------------
def _fields(m):
    m._plan()
    return [(type(n.layer).__name__, n.fused_act, None if n.fused_drop is None else n.fused_drop[0], n.absorbed, n.fuse_prev,
             None if n.infer_bn is None else n.infer_bn.index, None if n.fold_up is None else n.fold_up.index, n.lazy_bn) for n in m.nodes]


def _alone(kind):
    return (kind, None, None, False, -1, None, None, -1)


def test_the_planner_fuses_nothing_onto_or_around_a_softmax():
    plans = dict((k, _fields(M.MODELS[k]()[0])) for k in M.PLANNED)
    # (a) the head keeps its softmax and absorbs no producer's derivative; the tanh in front still fuses into its conv, as before
    assert plans['a'] == [('Conv1D', ('tanh', 0.0), None, False, -1, None, None, -1), ('Activation', None, None, True, -1, None, None, -1),
                          _alone('GlobalAveragePooling1D'), _alone('Dense')]
    # (b) Activation('softmax') is not absorbed by the Dense in front, the Dropout behind it runs on its own, and the last Dense absorbs nothing
    assert plans['b'] == [_alone('Dense'), _alone('Activation'), _alone('Dropout'), _alone('Dense')]
    # (c) the consumer's data gradient does not carry the softmax layer's derivative (fuse_prev stays -1)
    assert plans['c'] == [_alone('Conv1D'), _alone('Conv1D')]
    assert plans['d'] == [_alone('Conv1D'), _alone('Softmax'), _alone('Multiply'), _alone('GlobalAveragePooling1D'), _alone('Dense')]
    # (g) no inference fold (infer_bn), hence no statistics from the conv's epilogue either: Conv1D.forward takes both from node.infer_bn
    assert plans['g'] == [_alone('Conv1D'), _alone('BatchNormalization')]


def test_the_twins_without_softmax_do_fuse():
    """the same graphs with an element-wise activation in place of the softmax take every fusion the test above excludes: it is the softmax that
    keeps them out, not the shapes"""
    from gennet_amd import layers as L
    from gennet_amd.engine import Sequential
    b = _fields(Sequential([L.Dense(8, input_shape=(6,)), L.Activation('tanh'), L.Dropout(0.3), L.Dense(1)]))
    assert b[0][1] == ('tanh', 0.0) and b[1][3]
    head = _fields(Sequential([L.Dense(8, activation='tanh', input_shape=(6,)), L.Dense(1)]))
    assert head[1][4] == 0 and _fields(Sequential([L.Dense(8, activation='softmax', input_shape=(6,)), L.Dense(1)]))[1][4] == -1
    c = _fields(Sequential([L.Conv1D(8, 3, activation='tanh', input_shape=(16, 4)), L.Conv1D(4, 3)]))
    assert c[1][4] == 0
    g = _fields(Sequential([L.Conv1D(8, 5, padding='same', input_shape=(32, 4)), L.BatchNormalization()]))
    assert g[0][5] == 1
    drop = _fields(Sequential([L.Conv1D(8, 3, activation='tanh', input_shape=(16, 4)), L.Dropout(0.3)]))
    soft = _fields(Sequential([L.Conv1D(8, 3, activation='softmax', input_shape=(16, 4)), L.Dropout(0.3)]))
    assert drop[0][2] == 0.3 and drop[1][3] and soft == [_alone('Conv1D'), _alone('Dropout')]
    for make in (lambda a: L.Conv2D(4, (5, 5), strides=(2, 1), padding='same', activation=a, input_shape=(8, 2, 4)),
                 lambda a: L.Conv2DTranspose(4, (1, 3), activation=a, input_shape=(1, 8, 4))):
        assert _fields(Sequential([make('tanh'), L.Dropout(0.3)]))[0][2] == 0.3
        assert _fields(Sequential([make('softmax'), L.Dropout(0.3), L.Activation('relu')])) == [_alone(type(make(None)).__name__), _alone('Dropout'),
                                                                                                 _alone('Activation')]
    # a 1-filter softmax conv behind a BatchNormalization: no deferred data gradient
    lazy = lambda a: _fields(Sequential([L.Conv1D(8, 5, padding='same', input_shape=(32, 4)), L.BatchNormalization(), L.Activation('tanh'),       # noqa: E731
                                         L.Conv1D(1, 5, padding='same', activation=a)]))
    assert lazy(None)[3][7] == 1 and lazy('softmax')[3][7] == -1


BN_ = lambda: ('BatchNormalization', ('tanh', 0.0), 0.2, False, -1, None, None, -1)        # noqa: E731
GONE = lambda kind: (kind, None, None, True, -1, None, None, -1)                           # noqa: E731
CONV_RELU = lambda prev: ('Conv1D', ('relu', 0.0), None, False, prev, None, None, -1)      # noqa: E731
LEAKY = ('leaky', 0.20000000298023224)

# the planned node fields of bbh's three networks at n_pix = 256 as the commit before this feature plans them
GENERATOR = ([_alone('Dense'), BN_(), GONE('Activation'), GONE('Dropout'), _alone('Reshape'),
              GONE('UpSampling1D'), ('Conv1D', None, None, False, -1, 7, 5, -1), BN_(), GONE('Activation'), GONE('Dropout'),
              GONE('UpSampling1D'), ('Conv1D', None, None, False, -1, 12, 10, -1), BN_(), GONE('Activation'), GONE('Dropout')]
             + [f for bn in (16, 20, 24) for f in (('Conv1D', None, None, False, -1, bn, None, -1), BN_(), GONE('Activation'), GONE('Dropout'))]
             + [('Conv1D', ('linear', 0.0), None, False, -1, None, None, 24), GONE('Activation')])
DISCRIMINATOR = [('Conv2D', LEAKY, 0.4, False, -1, None, None, -1), GONE('LeakyReLU'), GONE('Dropout'),
                 ('Conv2D', LEAKY, 0.4, False, 0, None, None, -1), GONE('LeakyReLU'), GONE('Dropout'), _alone('Flatten'),
                 ('Dense', ('sigmoid', 0.0), None, False, 3, None, None, -1), GONE('Activation')]
PE = ([f for prev in (-1, 0, 2, 4) for f in (CONV_RELU(prev), GONE('Activation'))] + [_alone('Flatten'),
      ('Dense', ('relu', 0.0), None, False, 6, None, None, -1), GONE('Activation')]
      + [f for prev in (-1, 11, 13, 15, 17) for f in (CONV_RELU(prev), GONE('Activation'))] + [_alone('Flatten'),
      ('Dense', ('relu_max', 1.0), None, False, 19, None, None, -1), GONE('ReLU')])


def test_the_three_networks_plan_exactly_as_before():
    from gennet_amd import bbh
    assert _fields(bbh.generator_model(256)) == GENERATOR
    assert _fields(bbh.signal_discriminator_model(256)) == DISCRIMINATOR
    assert _fields(bbh.signal_pe_model(256)) == PE
