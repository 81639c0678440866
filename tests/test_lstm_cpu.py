"""keras layers.LSTM without a GPU: the fp64 definition tests/lstm_ref.py against torch.nn.LSTM and torch autograd, and the layer's host side --
shapes, weights, initializers, refusals, config and JSON, the facade, the header."""
import itertools
import json

import numpy as np
import pytest
import torch

import lstm_ref as R


def rel(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-300)


def draw(rng, B, T, Cin, u):
    return dict(x=rng.randn(B, T, Cin), W=rng.randn(Cin, 4 * u) / np.sqrt(Cin), U=rng.randn(u, 4 * u) / np.sqrt(u), b=0.3 * rng.randn(4 * u),
                h0=0.5 * rng.randn(B, u), c0=0.5 * rng.randn(B, u))


@pytest.mark.parametrize('go_backwards', [False, True])
def test_the_reference_is_torch_nn_lstm_in_fp64(go_backwards):
    """sigmoid gates and tanh: weight_ih = kernel^T, weight_hh = recurrent_kernel^T, bias_ih = bias, bias_hh = 0; torch's gate order is i, f, g, o too"""
    B, T, Cin, u = 3, 6, 4, 5
    d = draw(np.random.RandomState(1), B, T, Cin, u)
    y, k = R.forward(d['x'], d['W'], d['U'], d['b'], d['h0'], d['c0'], 'tanh', 'sigmoid', return_sequences=True, go_backwards=go_backwards)
    m = torch.nn.LSTM(Cin, u, batch_first=True).double()
    with torch.no_grad():
        m.weight_ih_l0.copy_(torch.tensor(d['W'].T))
        m.weight_hh_l0.copy_(torch.tensor(d['U'].T))
        m.bias_ih_l0.copy_(torch.tensor(d['b']))
        m.bias_hh_l0.zero_()
        x = torch.tensor(d['x'][:, ::-1].copy() if go_backwards else d['x'])
        out, (hn, cn) = m(x, (torch.tensor(d['h0'])[None], torch.tensor(d['c0'])[None]))
    assert rel(y, out.numpy()) < 1e-12 and rel(k['c'][:, -1], cn[0].numpy()) < 1e-12 and rel(y[:, -1], hn[0].numpy()) < 1e-12


PAIRS = list(itertools.product(R.ACTIVATIONS, R.RECURRENT_ACTIVATIONS))


@pytest.mark.parametrize('go_backwards', [False, True])
@pytest.mark.parametrize('return_sequences', [False, True])
@pytest.mark.parametrize('activation,recurrent_activation', PAIRS, ids=['%s-%s' % p for p in PAIRS])
def test_the_reference_gradients_are_torch_autograd_in_fp64(activation, recurrent_activation, return_sequences, go_backwards):
    B, T, Cin, u = 3, 5, 4, 6
    d = draw(np.random.RandomState(2), B, T, Cin, u)
    kw = dict(activation=activation, recurrent_activation=recurrent_activation, return_sequences=return_sequences, go_backwards=go_backwards)
    y, k = R.forward(d['x'], d['W'], d['U'], d['b'], d['h0'], d['c0'], **kw)
    if recurrent_activation == 'hard_sigmoid':            # some gate evaluations are saturated, none sits on a kink
        q = np.concatenate([k['z'][:, :, :2 * u], k['z'][:, :, 3 * u:]], 2)
        assert (np.abs(q) > 2.5).any() and np.abs(np.abs(q) - 2.5).min() > 1e-6
    dy = np.random.RandomState(3).randn(*y.shape)
    t = dict((n, torch.tensor(v, requires_grad=True)) for n, v in d.items())
    yt = R.torch_forward(t['x'], t['W'], t['U'], t['b'], t['h0'], t['c0'], **kw)
    assert rel(y, yt.detach().numpy()) < 1e-12
    (yt * torch.tensor(dy)).sum().backward()
    g = R.backward(k, dy)
    for mine, theirs in (('dx', 'x'), ('dW', 'W'), ('dU', 'U'), ('db', 'b'), ('dh0', 'h0'), ('dc0', 'c0')):
        assert rel(g[mine], t[theirs].grad.numpy()) < 1e-12, mine


def test_the_fp32_restatement_is_the_same_recurrence():
    d = draw(np.random.RandomState(4), 2, 9, 3, 7)
    y64, _ = R.forward(d['x'], d['W'], d['U'], d['b'], return_sequences=True)
    y32, k = R.forward(d['x'], d['W'], d['U'], d['b'], return_sequences=True, dtype=np.float32)
    assert y32.dtype == np.float32 and k['gates'].dtype == np.float32 and 0 < np.abs(y32 - y64).max() < 1e-5


# ---------------------------------------------------------------------------------------------------------------------
# the layer's host side
# ---------------------------------------------------------------------------------------------------------------------
def test_shapes_weight_order_names_and_initial_values():
    from gennet_amd import engine, layers as Ly
    engine.set_init_seed(7)
    x = engine.Input((9, 3))
    last, seq = Ly.LSTM(5, name='enc'), Ly.LSTM(4, return_sequences=True, unit_forget_bias=False)
    assert last(x).shape == (5,) and seq(x).shape == (9, 4)
    assert [p.name for p in last.weights] == ['enc/kernel', 'enc/recurrent_kernel', 'enc/bias']
    assert [p.shape for p in last.weights] == [(3, 20), (5, 20), (20,)] and last.count_params() == 4 * (3 * 5 + 5 * 5 + 5)
    W, U, b = last.get_weights()
    assert W.dtype == U.dtype == b.dtype == np.float32
    lim = np.sqrt(6.0 / (3 + 20))
    assert np.abs(W).max() <= lim and np.abs(W).max() > 0.5 * lim                      # Glorot uniform over (Cin, 4u)
    assert np.array_equal(b, np.repeat([0, 1, 0, 0], 5).astype(np.float32))            # ones in the f block
    assert not seq.get_weights()[2].any()
    for q in range(4):                                                                # four orthogonal u x u blocks
        Q = U[:, 5 * q:5 * q + 5].astype(np.float64)
        assert np.abs(Q.T @ Q - np.eye(5)).max() < 1e-6
    assert not np.allclose(U[:, :5], U[:, 5:10])
    engine.set_init_seed(7)                                                           # the generator glorot_uniform draws from
    again = Ly.LSTM(5)
    again(engine.Input((9, 3)))
    assert all(np.array_equal(a, b) for a, b in zip(again.get_weights(), last.get_weights()))
    with pytest.raises(ValueError, match='timesteps'):
        Ly.LSTM(3)(engine.Input((9,)))
    with pytest.raises(NotImplementedError, match='512'):
        Ly.LSTM(513)(engine.Input((4, 2)))


def test_regularizers_ride_on_the_weights():
    from gennet_amd import engine, layers as Ly, regularizers
    l = Ly.LSTM(3, kernel_regularizer=regularizers.l2(0.01), recurrent_regularizer='l1', bias_regularizer=regularizers.l1_l2(0.1, 0.2),
                activity_regularizer=regularizers.l2(0.5))
    l(engine.Input((4, 2)))
    assert [(p.regularizer.l1, p.regularizer.l2) for p in l.weights] == [(0.0, np.float32(0.01)), (np.float32(0.01), 0.0), (np.float32(0.1), np.float32(0.2))]
    assert l.activity_regularizer.l2 == np.float32(0.5)


REFUSED = [('dropout', dict(dropout=0.1)), ('recurrent_dropout', dict(recurrent_dropout=0.5)), ('stateful', dict(stateful=True)),
           ('return_state', dict(return_state=True)), ('use_bias', dict(use_bias=False)), ('activation', dict(activation='softsign')),
           ('recurrent_activation', dict(recurrent_activation='tanh')), ('recurrent_activation', dict(recurrent_activation='relu')),
           ('kernel_initializer', dict(kernel_initializer='he_normal')), ('recurrent_initializer', dict(recurrent_initializer='glorot_uniform')),
           ('bias_initializer', dict(bias_initializer='ones')), ('kernel_constraint', dict(kernel_constraint='max_norm')),
           ('recurrent_constraint', dict(recurrent_constraint={'class_name': 'MaxNorm', 'config': {}})), ('bias_constraint', dict(bias_constraint='non_neg')),
           ('recurrent_initializer', dict(recurrent_initializer={'class_name': 'Orthogonal', 'config': {'gain': 2.0, 'seed': None}}))]


@pytest.mark.parametrize('name,kw', REFUSED, ids=['%s-%d' % (n, i) for i, (n, _) in enumerate(REFUSED)])
def test_what_does_not_run_is_refused_by_name(name, kw):
    from gennet_amd import layers as Ly
    with pytest.raises(NotImplementedError, match=name):
        Ly.LSTM(4, **kw)


def test_accepted_spellings():
    from gennet_amd import layers as Ly
    from gennet_amd.keras import activations
    l = Ly.LSTM(4, activation=activations.relu, recurrent_activation='sigmoid', dropout=0.0, recurrent_dropout=0, stateful=False, return_state=False,
                kernel_constraint=None, implementation=2, unroll=True, kernel_initializer={'class_name': 'GlorotUniform', 'config': {'seed': None}})
    assert (l.activation, l.recurrent_activation, l.implementation, l.unroll) == ('relu', 'sigmoid', 2, True)
    assert Ly.LSTM(4, activation=None).activation == 'linear'
    with pytest.raises(ValueError, match='implementation'):
        Ly.LSTM(4, implementation=3)


KERAS_KEYS = {'name', 'trainable', 'return_sequences', 'return_state', 'go_backwards', 'stateful', 'unroll', 'units', 'activation',
              'recurrent_activation', 'use_bias', 'kernel_initializer', 'recurrent_initializer', 'bias_initializer', 'unit_forget_bias',
              'kernel_regularizer', 'recurrent_regularizer', 'bias_regularizer', 'activity_regularizer', 'kernel_constraint', 'recurrent_constraint',
              'bias_constraint', 'dropout', 'recurrent_dropout', 'implementation'}


def small_model():
    from gennet_amd import layers as Ly
    from gennet_amd.engine import Sequential
    m = Sequential()
    m.add(Ly.LSTM(5, input_shape=(7, 3), return_sequences=True, recurrent_regularizer='l2', implementation=2, unroll=True))
    m.add(Ly.LSTM(4, activation='relu', recurrent_activation='sigmoid', go_backwards=True, unit_forget_bias=False))
    m.add(Ly.Dense(1))
    return m


def test_config_round_trip():
    from gennet_amd.engine import model_from_json
    m = small_model()
    cfg = m.layers[0].get_config()
    assert set(cfg) == KERAS_KEYS | {'batch_input_shape', 'dtype'} and set(m.layers[1].get_config()) == KERAS_KEYS
    assert cfg['recurrent_initializer'] == {'class_name': 'Orthogonal', 'config': {'gain': 1.0, 'seed': None}}
    assert cfg['kernel_initializer']['class_name'] == 'VarianceScaling' and cfg['bias_initializer'] == {'class_name': 'Zeros', 'config': {}}
    assert (cfg['units'], cfg['activation'], cfg['recurrent_activation'], cfg['use_bias'], cfg['unit_forget_bias']) == (5, 'tanh', 'hard_sigmoid', True, True)
    assert (cfg['return_sequences'], cfg['return_state'], cfg['go_backwards'], cfg['stateful'], cfg['unroll']) == (True, False, False, False, True)
    assert (cfg['dropout'], cfg['recurrent_dropout'], cfg['implementation']) == (0.0, 0.0, 2)
    assert cfg['recurrent_regularizer']['class_name'] == 'L1L2' and cfg['kernel_regularizer'] is None and cfg['kernel_constraint'] is None
    again = model_from_json(m.to_json())
    assert json.loads(again.to_json()) == json.loads(m.to_json())
    assert [l.get_config() for l in again.layers] == [l.get_config() for l in m.layers]
    assert [p.shape for p in again.layers[1].weights] == [(5, 16), (4, 16), (16,)]


def test_a_layer_entry_as_keras_2_2_4_writes_it_loads():
    from gennet_amd.engine import model_from_json
    entry = {"class_name": "LSTM", "config": {
        "name": "lstm_7", "trainable": True, "batch_input_shape": [None, 12, 6], "dtype": "float32", "return_sequences": False, "return_state": False,
        "go_backwards": True, "stateful": False, "unroll": False, "units": 10, "activation": "tanh", "recurrent_activation": "hard_sigmoid",
        "use_bias": True, "kernel_initializer": {"class_name": "VarianceScaling", "config": {"scale": 1.0, "mode": "fan_avg", "distribution": "uniform",
                                                                                            "seed": None}},
        "recurrent_initializer": {"class_name": "Orthogonal", "config": {"gain": 1.0, "seed": None}},
        "bias_initializer": {"class_name": "Zeros", "config": {}}, "unit_forget_bias": True,
        "kernel_regularizer": {"class_name": "L1L2", "config": {"l1": 0.0, "l2": 0.0010000000474974513}}, "recurrent_regularizer": None,
        "bias_regularizer": None, "activity_regularizer": None, "kernel_constraint": None, "recurrent_constraint": None, "bias_constraint": None,
        "dropout": 0.0, "recurrent_dropout": 0.0, "implementation": 1}}
    text = json.dumps({"class_name": "Sequential", "config": {"name": "sequential_1", "layers": [entry]}, "keras_version": "2.2.4", "backend": "tensorflow"})
    m = model_from_json(text)
    l = m.layers[0]
    assert type(l).__name__ == 'LSTM' and (l.name, l.units, l.go_backwards, l.return_sequences) == ('lstm_7', 10, True, False)
    assert m.output_shape == (None, 10) and [p.shape for p in l.weights] == [(6, 40), (10, 40), (40,)]
    assert l.kernel.regularizer.l2 == np.float32(0.001)
    assert l.get_config() == entry['config']
    entry['config']['dropout'] = 0.25
    with pytest.raises(NotImplementedError, match='dropout'):
        model_from_json(json.dumps({"class_name": "Sequential", "config": {"name": "s", "layers": [entry]}}))


def test_the_facade_resolves():
    import gennet_amd.keras  # noqa: F401
    from gennet_amd import layers as Ly, recurrent
    from gennet_amd.keras.layers import LSTM as top
    from gennet_amd.keras.layers.recurrent import LSTM as deep
    import gennet_amd.keras.layers.recurrent as mod
    assert top is deep is Ly.LSTM is recurrent.LSTM is mod.LSTM
    assert 'LSTM' in gennet_amd.keras.__doc__


def test_the_planner_leaves_the_layer_alone():
    m = small_model()
    lstm_nodes = [n for n in m.nodes if type(n.layer).__name__ == 'LSTM']
    assert len(lstm_nodes) == 2 and all(n.fused_act is None and n.fused_drop is None for n in lstm_nodes)
    assert not any(n.layer.fusable_act or n.layer.fusable_drop or n.layer.writes_dy(n) for n in lstm_nodes)


def test_row_parts_of_the_weight_gradient_products():
    """the largest divisor of the rows up to 64 that leaves 256 rows a part and 64 MiB of partial results; by shape alone"""
    from gennet_amd.recurrent import row_splits
    assert [row_splits(r, c) for r, c in ((561, 100), (512, 60), (1024, 60), (8192, 64 * 256), (65536, 256 * 1024), (65536, 512 * 2048), (1000, 10),
                                          (257 * 3, 8))] == [1, 2, 4, 32, 64, 16, 2, 3]


def test_the_header_declares_the_entry_points():
    from gennet_amd import _lib, ops
    for name, ret, nargs in (('gn_lstm_fwd', _lib.i32, 19), ('gn_lstm_bwd', _lib.i32, 18), ('gn_lstm_fwd_workspace', _lib.sz, 1),
                             ('gn_lstm_bwd_workspace', _lib.sz, 1)):
        assert _lib.DECLS[name][0] is ret and len(_lib.DECLS[name][1]) == nargs, name
    assert ops.LSTM_ACT == {'tanh': 0, 'sigmoid': 1, 'relu': 2, 'linear': 3, 'hard_sigmoid': 4}
