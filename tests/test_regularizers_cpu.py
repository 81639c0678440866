"""CPU-only checks of the Keras regularizers: the facade, the L1L2 objects and their configs, the six layer classes' configs both
ways, a hand-typed Keras JSON, the planner around an activity-regularized node, and the binding of the new entry points."""
import json

import numpy as np
import pytest

L2_001 = float(np.float32(0.01))          # 0.009999999776482582: the value Keras writes for l2(0.01)
L1_0001 = float(np.float32(0.001))


# ---- the facade and the objects -------------------------------------------------------------------------------------------------------------
def test_the_facade_import_lines_work():
    from gennet_amd.keras import regularizers
    from gennet_amd.keras.regularizers import L1L2, deserialize, get, l1, l1_l2, l2, serialize      # noqa: F401
    from gennet_amd.keras.layers import ActivityRegularization
    from gennet_amd.keras.layers.core import ActivityRegularization as FromCore
    from gennet_amd import layers, regularizers as home
    assert regularizers.l2 is home.l2 and regularizers.L1L2 is home.L1L2 and ActivityRegularization is FromCore is layers.ActivityRegularization


def test_l1_l2_l1_l2_and_their_float32_coefficients():
    from gennet_amd.keras.regularizers import L1L2, l1, l1_l2, l2
    assert l2(0.01).get_config() == {'l1': 0.0, 'l2': L2_001} and l2(0.01).get_config()['l2'] == float(np.float32(0.01)) != 0.01
    assert l1(0.001).get_config() == {'l1': L1_0001, 'l2': 0.0}
    assert l1_l2(0.001, 0.01).get_config() == {'l1': L1_0001, 'l2': L2_001}
    assert (l1().l1, l2().l2, l1_l2().l1, l1_l2().l2) == (L2_001,) * 4 and L1L2().get_config() == {'l1': 0.0, 'l2': 0.0}      # Keras' defaults
    assert all(type(v) is float for v in l1_l2(0.001, 0.01).get_config().values())
    assert l1_l2(0.001, 0.01) == L1L2(l1=0.001, l2=0.01) != l2(0.01)
    for bad in (-0.1, float('nan'), float('inf')):
        with pytest.raises(ValueError):
            l2(bad)


def test_get_serialize_and_deserialize_round_trip():
    from gennet_amd.keras import regularizers as R
    obj = R.l1_l2(0.001, 0.02)
    assert R.get(obj) is obj and R.get(None) is None and R.serialize(None) is None
    cfg = R.serialize(obj)
    assert cfg == {'class_name': 'L1L2', 'config': {'l1': L1_0001, 'l2': float(np.float32(0.02))}}
    assert R.deserialize(cfg) == obj and R.get(cfg) == obj and R.serialize(R.get(cfg)) == cfg
    assert json.loads(json.dumps(cfg)) == cfg
    assert (R.get('l1'), R.get('l2'), R.get('l1_l2')) == (R.l1(), R.l2(), R.l1_l2())
    for bad in ('l3', {'class_name': 'Orthogonal', 'config': {}}, 7):
        with pytest.raises(ValueError):
            R.get(bad)


def test_a_custom_callable_is_refused_by_name():
    from gennet_amd.keras import regularizers as R
    from gennet_amd.keras.layers import Dense

    def my_penalty(w):
        return 0.0

    class Mine(R.Regularizer):
        def __call__(self, x):
            return 0.0
    with pytest.raises(NotImplementedError, match='my_penalty'):
        R.get(my_penalty)
    with pytest.raises(NotImplementedError, match='Mine'):
        R.get(Mine())
    with pytest.raises(NotImplementedError, match='my_penalty'):
        Dense(4, kernel_regularizer=my_penalty)


# ---- configs ----------------------------------------------------------------------------------------------------------------------------------
def _d(l1, l2):
    return {'class_name': 'L1L2', 'config': {'l1': float(np.float32(l1)), 'l2': float(np.float32(l2))}}


def _six():
    from gennet_amd.keras import regularizers as R
    from gennet_amd import layers as L
    three = dict(kernel_regularizer=R.l1_l2(0.01, 0.02), bias_regularizer=R.l2(0.1), activity_regularizer=R.l1(0.001))
    want3 = dict(kernel_regularizer=_d(0.01, 0.02), bias_regularizer=_d(0, 0.1), activity_regularizer=_d(0.001, 0))
    return [('Dense', L.Dense(8, activation='tanh', **three), want3),
            ('Conv1D', L.Conv1D(8, 3, **three), want3),
            ('Conv2D', L.Conv2D(4, (5, 5), padding='same', **three), want3),
            ('Conv2DTranspose', L.Conv2DTranspose(4, (1, 4), activity_regularizer=R.l1(0.001), kernel_regularizer='l2'),
             dict(kernel_regularizer=_d(0, 0.01), bias_regularizer=None, activity_regularizer=_d(0.001, 0))),
            ('BatchNormalization', L.BatchNormalization(gamma_regularizer=R.l2(0.1), beta_regularizer=R.l1(0.01)),
             dict(gamma_regularizer=_d(0, 0.1), beta_regularizer=_d(0.01, 0))),
            ('PReLU', L.PReLU(alpha_regularizer=_d(0, 0.1)), dict(alpha_regularizer=_d(0, 0.1)))]


def test_layer_configs_carry_the_keras_dicts_and_come_back():
    from gennet_amd import keras_io
    for cls, layer, want in _six():
        cfg = keras_io.layer_config(layer)
        for k, v in want.items():
            assert cfg[k] == v, (cls, k, cfg[k])
        back = keras_io._layer_from_config(cls, json.loads(json.dumps(cfg)), None)
        assert type(back) is type(layer) and keras_io.layer_config(back) == cfg, cls
        for k, v in want.items():
            got = getattr(back, k)
            assert (got is None) if v is None else ((got.l1, got.l2) == (v['config']['l1'], v['config']['l2'])), (cls, k)
            assert v is None or (np.float32(got.l1) == got.l1 and np.float32(got.l2) == got.l2)        # the fp32 coefficient, held exactly


def test_the_regularizer_reaches_the_weight_it_names():
    from gennet_amd.engine import Input
    for cls, layer, want in _six():
        shape = {'Dense': (6,), 'Conv1D': (21, 4), 'Conv2D': (8, 2, 4), 'Conv2DTranspose': (1, 9, 8), 'BatchNormalization': (5, 8), 'PReLU': (8,)}[cls]
        layer(Input(shape))
        for p in layer.weights:
            key = p.name.rsplit('/', 1)[1] + '_regularizer'
            if want.get(key) is None:
                assert p.regularizer is None, p.name
            else:
                assert (p.regularizer.l1, p.regularizer.l2) == (want[key]['config']['l1'], want[key]['config']['l2']), p.name


def test_none_is_exactly_today():
    from gennet_amd import keras_io
    from gennet_amd import layers as L
    for a, b in ((L.Dense(8, name='d'), L.Dense(8, name='d', kernel_regularizer=None, bias_regularizer=None, activity_regularizer=None)),
                 (L.BatchNormalization(name='b'), L.BatchNormalization(name='b', beta_regularizer=None, gamma_regularizer=None)),
                 (L.PReLU(name='p'), L.PReLU(name='p', alpha_regularizer=None))):
        assert keras_io.layer_config(a) == keras_io.layer_config(b)
        assert all(v is None for k, v in keras_io.layer_config(a).items() if k.endswith('_regularizer'))
        assert a.activity_regularizer is None


def test_activity_regularization_round_trips():
    from gennet_amd import keras_io
    from gennet_amd.keras.layers import ActivityRegularization
    from gennet_amd.keras.models import Sequential, model_from_json
    from gennet_amd.layers import Dense
    a = ActivityRegularization(l1=0.001, l2=0.02, name='areg')
    cfg = keras_io.layer_config(a)
    assert cfg == {'name': 'areg', 'trainable': True, 'l1': L1_0001, 'l2': float(np.float32(0.02))}
    back = keras_io._layer_from_config('ActivityRegularization', cfg, None)
    assert (back.l1, back.l2) == (a.l1, a.l2) and back.activity_regularizer == a.activity_regularizer and keras_io.layer_config(back) == cfg
    assert ActivityRegularization().activity_regularizer is None and keras_io.layer_config(ActivityRegularization(name='z'))['l1'] == 0.0
    m = Sequential([Dense(4, input_shape=(3,)), a])
    again = model_from_json(m.to_json())
    assert [type(l).__name__ for l in again.layers] == ['Dense', 'ActivityRegularization'] and again.layers[1].l2 == a.l2
    assert again.nodes[1].out_shape == (4,) and a.count_params() == 0


# typed in the form keras 2.2.4 writes (to_json of a Sequential)
KERAS_JSON = '''{"class_name": "Sequential", "config": {"name": "sequential_1", "layers": [
 {"class_name": "Conv1D", "config": {"name": "conv1d_1", "trainable": true, "batch_input_shape": [null, 21, 4], "dtype": "float32", "filters": 8,
  "kernel_size": [3], "strides": [1], "padding": "valid", "data_format": "channels_last", "dilation_rate": [1], "activation": "tanh", "use_bias": true,
  "kernel_initializer": {"class_name": "VarianceScaling", "config": {"scale": 1.0, "mode": "fan_avg", "distribution": "uniform", "seed": null}},
  "bias_initializer": {"class_name": "Zeros", "config": {}},
  "kernel_regularizer": {"class_name": "L1L2", "config": {"l1": 0.0, "l2": 0.009999999776482582}}, "bias_regularizer": null,
  "activity_regularizer": {"class_name": "L1L2", "config": {"l1": 0.0010000000474974513, "l2": 0.0}},
  "kernel_constraint": null, "bias_constraint": null}},
 {"class_name": "BatchNormalization", "config": {"name": "batch_normalization_1", "trainable": true, "axis": -1, "momentum": 0.99, "epsilon": 0.001,
  "center": true, "scale": true, "beta_initializer": {"class_name": "Zeros", "config": {}}, "gamma_initializer": {"class_name": "Ones", "config": {}},
  "moving_mean_initializer": {"class_name": "Zeros", "config": {}}, "moving_variance_initializer": {"class_name": "Ones", "config": {}},
  "beta_regularizer": null, "gamma_regularizer": {"class_name": "L1L2", "config": {"l1": 0.0, "l2": 0.10000000149011612}},
  "beta_constraint": null, "gamma_constraint": null}},
 {"class_name": "ActivityRegularization", "config": {"name": "activity_regularization_1", "trainable": true, "l1": 0.0, "l2": 0.019999999552965164}},
 {"class_name": "Flatten", "config": {"name": "flatten_1", "trainable": true, "data_format": "channels_last"}},
 {"class_name": "Dense", "config": {"name": "dense_1", "trainable": false, "units": 1, "activation": "sigmoid", "use_bias": true,
  "kernel_initializer": {"class_name": "VarianceScaling", "config": {"scale": 1.0, "mode": "fan_avg", "distribution": "uniform", "seed": null}},
  "bias_initializer": {"class_name": "Zeros", "config": {}},
  "kernel_regularizer": {"class_name": "L1L2", "config": {"l1": 0.009999999776482582, "l2": 0.009999999776482582}},
  "bias_regularizer": {"class_name": "L1L2", "config": {"l1": 0.0, "l2": 0.10000000149011612}}, "activity_regularizer": null,
  "kernel_constraint": null, "bias_constraint": null}}]}, "keras_version": "2.2.4", "backend": "tensorflow"}'''


def test_a_keras_json_with_regularizers_builds_keeps_them_and_is_written_back():
    from gennet_amd.keras.models import model_from_json
    m = model_from_json(KERAS_JSON)
    conv, bn, areg, _, dense = m.layers
    assert (conv.kernel_regularizer.l1, conv.kernel_regularizer.l2) == (0.0, L2_001) and conv.bias_regularizer is None
    assert (conv.activity_regularizer.l1, conv.activity_regularizer.l2) == (L1_0001, 0.0)
    assert bn.beta_regularizer is None and bn.gamma_regularizer.l2 == float(np.float32(0.1)) and bn.gamma.regularizer is bn.gamma_regularizer
    assert (areg.l1, areg.l2) == (0.0, float(np.float32(0.02))) and areg.activity_regularizer.l2 == areg.l2
    assert (dense.kernel.regularizer.l1, dense.kernel.regularizer.l2, dense.bias.regularizer.l2) == (L2_001, L2_001, float(np.float32(0.1)))
    assert conv.kernel.regularizer is conv.kernel_regularizer and conv.bias.regularizer is None
    typed = json.loads(KERAS_JSON)['config']['layers']
    written = json.loads(m.to_json())['config']['layers']
    for t, w in zip(typed, written):
        for k in t['config']:
            if k.endswith('_regularizer') or k in ('l1', 'l2'):
                assert w['config'][k] == t['config'][k], (t['class_name'], k)
    # compile collects every regularized weight, the frozen Dense's included, and the two nodes that regularize their output
    m.compile(loss='binary_crossentropy', optimizer='sgd')
    assert [(p.name, trained) for p, trained in m._reg_params] == [('conv1d_1/kernel', True), ('batch_normalization_1/gamma', True),
                                                                   ('dense_1/kernel', False), ('dense_1/bias', False)]
    assert [n.layer.name for n in m._reg_nodes] == ['conv1d_1', 'activity_regularization_1']
    assert [l.name for l in m.layers] == ['conv1d_1', 'batch_normalization_1', 'activity_regularization_1', 'flatten_1', 'dense_1']      # no helper node


# ---- the planner --------------------------------------------------------------------------------------------------------------------------------
def _fields(m):
    m._plan()
    return [(type(n.layer).__name__, n.fused_act, None if n.fused_drop is None else n.fused_drop[0], n.absorbed, n.fuse_prev,
             None if n.infer_bn is None else n.infer_bn.index, None if n.fold_up is None else n.fold_up.index, n.lazy_bn) for n in m.nodes]


def _alone(kind):
    return (kind, None, None, False, -1, None, None, -1)


def _stack(reg, tail, activation=None):
    from gennet_amd import layers as L
    from gennet_amd.engine import Sequential
    return Sequential([L.Conv1D(8, 5, padding='same', input_shape=(16, 8), activity_regularizer=reg, activation=activation)] + tail())


def test_the_planner_fuses_nothing_onto_or_across_an_activity_regularized_node():
    from gennet_amd import layers as L
    from gennet_amd.keras.regularizers import l1
    act_drop = lambda: [L.LeakyReLU(0.2), L.Dropout(0.25), L.Conv1D(8, 5, padding='same')]        # noqa: E731
    bn = lambda: [L.BatchNormalization(), L.Conv1D(8, 5, padding='same')]                            # noqa: E731
    up = lambda: [L.UpSampling1D(2), L.Conv1D(8, 5, padding='same', activity_regularizer=l1(0.001))]   # noqa: E731
    # as today: the activation and the Dropout run in the conv's epilogue and the next conv's data gradient takes their derivative;
    # a BatchNormalization folds into the conv in the inference phase; an UpSampling1D folds into the conv behind it
    assert _fields(_stack(None, act_drop)) == [('Conv1D', ('leaky', float(np.float32(0.2))), 0.25, False, -1, None, None, -1),
                                               ('LeakyReLU', None, None, True, -1, None, None, -1), ('Dropout', None, None, True, -1, None, None, -1),
                                               ('Conv1D', None, None, False, 0, None, None, -1)]
    assert _fields(_stack(None, bn)) == [('Conv1D', None, None, False, -1, 1, None, -1), _alone('BatchNormalization'), _alone('Conv1D')]
    assert _fields(_stack(None, lambda: [L.UpSampling1D(2), L.Conv1D(8, 5, padding='same')])) == [
        _alone('Conv1D'), ('UpSampling1D', None, None, True, -1, None, None, -1), ('Conv1D', None, None, False, 0, None, 1, -1)]
    # with the regularizer: the node's own output is materialised, every layer behind it runs on its own and differentiates itself
    assert _fields(_stack(l1(0.001), act_drop)) == [_alone('Conv1D'), _alone('LeakyReLU'), _alone('Dropout'), _alone('Conv1D')]
    assert _fields(_stack(l1(0.001), bn)) == [_alone('Conv1D'), _alone('BatchNormalization'), _alone('Conv1D')]
    assert _fields(_stack(None, up)) == [_alone('Conv1D'), _alone('UpSampling1D'), _alone('Conv1D')]
    # an activation with a tanh of its own keeps it (it is the layer's output) and still offers nothing to the conv behind it
    one = lambda: [L.Conv1D(8, 5, padding='same')]                                                   # noqa: E731
    assert _fields(_stack(None, one, 'tanh')) == [_alone('Conv1D'), ('Conv1D', None, None, False, 0, None, None, -1)]
    assert _fields(_stack(l1(0.001), one, 'tanh')) == [_alone('Conv1D'), _alone('Conv1D')]
    # ActivityRegularization between a conv and its activation: the conv's own (linear) output is the regularized tensor
    from gennet_amd.engine import Sequential
    m = Sequential([L.Conv1D(8, 5, padding='same', input_shape=(16, 8)), L.ActivityRegularization(l2=0.01), L.LeakyReLU(0.2),
                    L.Conv1D(8, 5, padding='same')])
    assert _fields(m) == [_alone('Conv1D'), _alone('ActivityRegularization'), _alone('LeakyReLU'), _alone('Conv1D')]


def test_a_model_without_regularizers_plans_and_collects_as_before():
    from gennet_amd import layers as L
    with_none = _stack(None, lambda: [L.LeakyReLU(0.2), L.Dropout(0.25), L.BatchNormalization(), L.Flatten(), L.Dense(1, activation='sigmoid')])
    from gennet_amd.engine import Sequential
    never = Sequential([L.Conv1D(8, 5, padding='same', input_shape=(16, 8)), L.LeakyReLU(0.2), L.Dropout(0.25), L.BatchNormalization(), L.Flatten(),
                        L.Dense(1, activation='sigmoid')])
    assert _fields(with_none) == _fields(never)
    for m in (with_none, never):
        m.compile(loss='binary_crossentropy', optimizer='adam')
        assert m._reg_params == [] and m._reg_nodes == []


# ---- the binding --------------------------------------------------------------------------------------------------------------------------------
def test_binding_declares_the_regularizer_entry_points():
    from gennet_amd import _lib
    from gennet_amd._lib import f32, i32, sz, vp
    assert _lib.DECLS['gn_reg_partials'] == (sz, [sz])
    assert _lib.DECLS['gn_reg_pass'] == (i32, [vp, vp, sz, f32, f32, vp, sz, vp])
    assert _lib.DECLS['gn_reg_grad'] == (i32, [vp, vp, vp, sz, f32, f32, vp])
    assert _lib.DECLS['gn_reg_finish'] == (i32, [vp, sz, vp, vp])


def test_the_entry_points_refuse_before_they_launch():
    """host-only checks: a refusal returns GN_EINVAL with a text that names the entry point and launches nothing, so it needs no device"""
    from gennet_amd import _lib
    lib = _lib.lib()
    one = 4096          # stands for a pointer: never dereferenced on the host
    nan, inf = float('nan'), float('inf')
    assert _lib.size('gn_reg_partials', 1) == 1 and _lib.size('gn_reg_partials', 1024) == 1 and _lib.size('gn_reg_partials', 1025) == 2
    assert _lib.size('gn_reg_partials', (1 << 21) + 5) == 2048 == _lib.size('gn_reg_partials', 1 << 30)      # stream_grid's cap
    for args, text in (((None, one, 8, 0.01, 0.0, one, 1, None), 'reg_pass: null pointer'), ((one, one, 8, 0.01, 0.0, None, 1, None), 'reg_pass: null pointer'),
                       ((one, one, 0, 0.01, 0.0, one, 1, None), 'reg_pass: n == 0'), ((one, one, 8, -0.01, 0.0, one, 1, None), 'reg_pass: l1 -0.01'),
                       ((one, one, 8, 0.0, nan, one, 1, None), 'reg_pass: l1 0, l2 nan'), ((one, one, 8, inf, 0.0, one, 1, None), 'reg_pass: l1 inf'),
                       ((one, None, 1025, 0.01, 0.0, one, 1, None), 'reg_pass: a workspace of 1 partials for n = 1025, which writes 2'),
                       ((one, None, 8, 0.01, 0.0, one + 4, 1, None), 'reg_pass: the partial workspace is not 8-byte aligned')):
        assert lib.gn_reg_pass(*args) == _lib.GN_EINVAL and lib.gn_last_error().decode().startswith(text), (args, lib.gn_last_error())
    for args, text in (((None, one, one, 8, 0.01, 0.0, None), 'reg_grad: null pointer'), ((one, None, one, 8, 0.01, 0.0, None), 'reg_grad: null pointer'),
                       ((one, one, None, 8, 0.01, 0.0, None), 'reg_grad: null pointer'), ((one, one, one, 0, 0.01, 0.0, None), 'reg_grad: n == 0'),
                       ((one, one, one, 8, 0.0, -1.0, None), 'reg_grad: l1 0, l2 -1'), ((one, one, one, 8, nan, 0.0, None), 'reg_grad: l1 nan')):
        assert lib.gn_reg_grad(*args) == _lib.GN_EINVAL and lib.gn_last_error().decode().startswith(text), (args, lib.gn_last_error())
    for args, text in (((None, 4, one, None), 'reg_finish: null pointer'), ((one, 4, None, None), 'reg_finish: null pointer'),
                       ((one, 0, one, None), 'reg_finish: no partials')):
        assert lib.gn_reg_finish(*args) == _lib.GN_EINVAL and lib.gn_last_error().decode().startswith(text), (args, lib.gn_last_error())
