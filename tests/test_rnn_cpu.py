"""keras layers.SimpleRNN without a GPU: the fp64 definition tests/rnn_ref.py against torch.nn.RNN and torch autograd, the layer's host side --
shapes, weights, initializers, refusals, config and JSON (alone and inside Bidirectional), the facade, the header --, the launch geometry walked
under the host sanitizers, and the promises of the GPU tests' integer case and seed rule."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import rnn_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def the_initial_weight_generator_is_left_as_found():
    """Initial weights come from ONE process-wide generator (engine._INIT_RNG), and tests elsewhere build their models from wherever it stands:
    the tests here put it back, so the files that run after this one draw what they drew before it existed."""
    from gennet_amd import engine
    rng = engine._INIT_RNG
    state = rng.get_state()
    yield
    rng.set_state(state)
    engine._INIT_RNG = rng


def rel(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-300)


def draw(rng, B, T, Cin, u):
    return dict(x=rng.randn(B, T, Cin), W=rng.randn(Cin, u) / np.sqrt(Cin), U=rng.randn(u, u) / np.sqrt(u), b=0.3 * rng.randn(u), h0=0.5 * rng.randn(B, u))


@pytest.mark.parametrize('go_backwards', [False, True])
@pytest.mark.parametrize('activation', ['tanh', 'relu'])
def test_the_reference_is_torch_nn_rnn_in_fp64(activation, go_backwards):
    """weight_ih = kernel^T, weight_hh = recurrent_kernel^T, bias_ih = b, bias_hh = 0; go_backwards is the time-reversed input"""
    B, T, Cin, u = 3, 6, 4, 5
    d = draw(np.random.RandomState(1), B, T, Cin, u)
    y, _ = R.forward(d['x'], d['W'], d['U'], d['b'], d['h0'], activation, return_sequences=True, go_backwards=go_backwards)
    m = torch.nn.RNN(Cin, u, nonlinearity=activation, batch_first=True).double()
    with torch.no_grad():
        m.weight_ih_l0.copy_(torch.tensor(d['W'].T.copy()))
        m.weight_hh_l0.copy_(torch.tensor(d['U'].T.copy()))
        m.bias_ih_l0.copy_(torch.tensor(d['b']))
        m.bias_hh_l0.zero_()
        x = torch.tensor(d['x'][:, ::-1].copy() if go_backwards else d['x'])
        out, hn = m(x, torch.tensor(d['h0'])[None])
    assert rel(y, out.numpy()) < 1e-12 and rel(y[:, -1], hn[0].numpy()) < 1e-12


@pytest.mark.parametrize('go_backwards', [False, True])
@pytest.mark.parametrize('return_sequences', [False, True])
@pytest.mark.parametrize('activation', R.ACTIVATIONS)
def test_the_reference_gradients_are_torch_autograd_in_fp64(activation, return_sequences, go_backwards):
    B, T, Cin, u = 3, 5, 4, 6
    d = draw(np.random.RandomState(2), B, T, Cin, u)
    kw = dict(activation=activation, return_sequences=return_sequences, go_backwards=go_backwards)
    y, k = R.forward(d['x'], d['W'], d['U'], d['b'], d['h0'], **kw)
    if activation == 'relu':                              # both sides of the kink are met, none sits on it
        assert (k['pre'] > 0).any() and (k['pre'] < 0).any() and np.abs(k['pre']).min() > 1e-6
    dy = np.random.RandomState(3).randn(*y.shape)
    t = dict((n, torch.tensor(v, requires_grad=True)) for n, v in d.items())
    yt = R.torch_forward(t['x'], t['W'], t['U'], t['b'], t['h0'], **kw)
    assert rel(y, yt.detach().numpy()) < 1e-12
    (yt * torch.tensor(dy)).sum().backward()
    g = R.backward(k, dy)
    for mine, theirs in [('dx', 'x'), ('dW', 'W'), ('dU', 'U'), ('db', 'b'), ('dh0', 'h0')]:
        assert rel(g[mine], t[theirs].grad.numpy()) < 1e-12, mine


def test_the_fp32_restatement_is_the_same_recurrence():
    d = draw(np.random.RandomState(4), 2, 9, 3, 7)
    y64, _ = R.forward(d['x'], d['W'], d['U'], d['b'], return_sequences=True)
    y32, k = R.forward(d['x'], d['W'], d['U'], d['b'], return_sequences=True, dtype=np.float32)
    assert y32.dtype == np.float32 and k['pre'].dtype == np.float32 and k['h_prev'].dtype == np.float32 and 0 < np.abs(y32 - y64).max() < 1e-5
    g = R.recurrence_backward(k, np.ones_like(y32))
    assert g['dz'].dtype == np.float32 and g['dh0'].dtype == np.float32


# ---------------------------------------------------------------------------------------------------------------------
# the layer's host side
# ---------------------------------------------------------------------------------------------------------------------
def test_shapes_weight_order_names_and_initial_values():
    from gennet_amd import engine, layers as Ly
    engine.set_init_seed(7)
    x = engine.Input((9, 3))
    last, seq = Ly.SimpleRNN(5, name='enc'), Ly.SimpleRNN(4, return_sequences=True)
    assert last(x).shape == (5,) and seq(x).shape == (9, 4)                            # keras' output shapes
    assert [p.name for p in last.weights] == ['enc/kernel', 'enc/recurrent_kernel', 'enc/bias']
    assert [p.shape for p in last.weights] == [(3, 5), (5, 5), (5,)] and last.count_params() == 3 * 5 + 5 * 5 + 5
    assert [p.shape for p in seq.weights] == [(3, 4), (4, 4), (4,)]
    W, U, b = last.get_weights()
    assert W.dtype == U.dtype == b.dtype == np.float32
    lim = np.sqrt(6.0 / (3 + 5))
    assert np.abs(W).max() <= lim and np.abs(W).max() > 0.5 * lim                      # Glorot uniform over (Cin, u)
    assert not b.any()
    assert np.abs(U.astype(np.float64).T @ U.astype(np.float64) - np.eye(5)).max() < 1e-6          # one orthogonal u x u block
    engine.set_init_seed(7)                                                           # the generator glorot_uniform draws from
    again = Ly.SimpleRNN(5)
    again(engine.Input((9, 3)))
    assert all(np.array_equal(a, b) for a, b in zip(again.get_weights(), last.get_weights()))
    with pytest.raises(ValueError, match='timesteps'):
        Ly.SimpleRNN(3)(engine.Input((9,)))
    with pytest.raises(NotImplementedError, match='512'):
        Ly.SimpleRNN(513)(engine.Input((4, 2)))


def test_the_draw_order_is_what_a_lone_layer_draws():
    """glorot_uniform (Cin, u) first, then the normal draw of the orthogonal block, from the one generator: the forward triple of a Bidirectional
    wrapper is what a lone layer draws, and the backward triple what a second lone layer draws after it"""
    from gennet_amd import engine, layers as Ly
    from gennet_amd.recurrent import orthogonal_blocks
    engine.set_init_seed(11)
    W, U = engine.glorot_uniform((3, 6)), orthogonal_blocks(6, 1)
    engine.set_init_seed(11)
    a, b = Ly.SimpleRNN(6), Ly.SimpleRNN(6)
    a(engine.Input((4, 3)))
    b(engine.Input((4, 3)))
    assert np.array_equal(a.get_weights()[0], W) and np.array_equal(a.get_weights()[1], U)
    engine.set_init_seed(11)
    bi = Ly.Bidirectional(Ly.SimpleRNN(6, name='cell'), name='bi')
    bi(engine.Input((4, 3)))
    assert [p.name for p in bi.weights] == ['bi/%s_cell/%s' % (d, n) for d in ('forward', 'backward') for n in ('kernel', 'recurrent_kernel', 'bias')]
    assert [p.shape for p in bi.weights] == [(3, 6), (6, 6), (6,)] * 2
    assert all(np.array_equal(v, w) for v, w in zip(bi.get_weights(), a.get_weights() + b.get_weights()))


def test_regularizers_ride_on_the_weights():
    from gennet_amd import engine, layers as Ly, regularizers
    l = Ly.SimpleRNN(3, kernel_regularizer=regularizers.l2(0.01), recurrent_regularizer='l1', bias_regularizer=regularizers.l1_l2(0.1, 0.2),
                     activity_regularizer=regularizers.l2(0.5))
    l(engine.Input((4, 2)))
    assert [(p.regularizer.l1, p.regularizer.l2) for p in l.weights] == [(0.0, np.float32(0.01)), (np.float32(0.01), 0.0), (np.float32(0.1), np.float32(0.2))]
    assert l.activity_regularizer.l2 == np.float32(0.5)


REFUSED = [('dropout', dict(dropout=0.1)), ('recurrent_dropout', dict(recurrent_dropout=0.5)), ('stateful', dict(stateful=True)),
           ('return_state', dict(return_state=True)), ('use_bias', dict(use_bias=False)), ('activation', dict(activation='softsign')),
           ('activation', dict(activation='hard_sigmoid')),
           ('kernel_initializer', dict(kernel_initializer='he_normal')), ('recurrent_initializer', dict(recurrent_initializer='glorot_uniform')),
           ('bias_initializer', dict(bias_initializer='ones')), ('kernel_constraint', dict(kernel_constraint='max_norm')),
           ('recurrent_constraint', dict(recurrent_constraint={'class_name': 'MaxNorm', 'config': {}})), ('bias_constraint', dict(bias_constraint='non_neg')),
           ('recurrent_initializer', dict(recurrent_initializer={'class_name': 'Orthogonal', 'config': {'gain': 2.0, 'seed': None}}))]


@pytest.mark.parametrize('name,kw', REFUSED, ids=['%s-%d' % (n, i) for i, (n, _) in enumerate(REFUSED)])
def test_what_does_not_run_is_refused_by_name(name, kw):
    from gennet_amd import layers as Ly
    with pytest.raises(NotImplementedError, match=r'SimpleRNN\(%s' % name):
        Ly.SimpleRNN(4, **kw)


def test_accepted_and_absent_spellings():
    from gennet_amd import layers as Ly
    from gennet_amd.keras import activations
    l = Ly.SimpleRNN(4, activation=activations.relu, dropout=0.0, recurrent_dropout=0, stateful=False, return_state=False, kernel_constraint=None,
                     unroll=True, kernel_initializer={'class_name': 'GlorotUniform', 'config': {'seed': None}})
    assert (l.activation, l.unroll, l.n_gates) == ('relu', True, 1)
    assert not hasattr(l, 'recurrent_activation') and not hasattr(l, 'implementation') and not hasattr(l, 'reset_after')
    assert Ly.SimpleRNN(4, activation=None).activation == 'linear' and Ly.SimpleRNN(4).activation == 'tanh'
    with pytest.raises(ValueError, match='at least 1'):
        Ly.SimpleRNN(0)
    for key in ('recurrent_activation', 'implementation', 'reset_after'):         # keras' SimpleRNN has none of them
        with pytest.raises(TypeError):
            Ly.SimpleRNN(4, **{key: 1})


def test_the_messages_of_lstm_and_gru_stand():
    from gennet_amd import layers as Ly
    with pytest.raises(NotImplementedError) as e:
        Ly.LSTM(4, recurrent_activation='tanh')
    assert str(e.value) == "LSTM(recurrent_activation='tanh'): one of hard_sigmoid, sigmoid"
    with pytest.raises(NotImplementedError) as e:
        Ly.GRU(4, recurrent_activation=None)
    assert str(e.value) == "GRU(recurrent_activation=None): one of hard_sigmoid, sigmoid"
    with pytest.raises(ValueError) as e:
        Ly.GRU(4, implementation=None)
    assert str(e.value) == "GRU(implementation=None): 1 or 2"
    assert (Ly.LSTM(4).recurrent_activation, Ly.LSTM(4).implementation, Ly.GRU(4, implementation=2).implementation) == ('hard_sigmoid', 1, 2)
    with pytest.raises(ValueError, match='Bidirectional'):
        Ly.Bidirectional(Ly.Dense(3))


# the keys of keras 2.2.4 SimpleRNN.get_config: GRU's without recurrent_activation, implementation and reset_after
KERAS_KEYS = {'name', 'trainable', 'return_sequences', 'return_state', 'go_backwards', 'stateful', 'unroll', 'units', 'activation', 'use_bias',
              'kernel_initializer', 'recurrent_initializer', 'bias_initializer', 'kernel_regularizer', 'recurrent_regularizer', 'bias_regularizer',
              'activity_regularizer', 'kernel_constraint', 'recurrent_constraint', 'bias_constraint', 'dropout', 'recurrent_dropout'}


def small_model():
    from gennet_amd import layers as Ly
    from gennet_amd.engine import Sequential
    m = Sequential()
    m.add(Ly.SimpleRNN(5, input_shape=(7, 3), return_sequences=True, recurrent_regularizer='l2', unroll=True))
    m.add(Ly.SimpleRNN(4, activation='relu', go_backwards=True))
    m.add(Ly.Dense(1))
    return m


def test_config_round_trip():
    from gennet_amd.engine import model_from_json
    m = small_model()
    cfg = m.layers[0].get_config()
    assert set(cfg) == KERAS_KEYS | {'batch_input_shape', 'dtype'} and set(m.layers[1].get_config()) == KERAS_KEYS
    assert cfg['recurrent_initializer'] == {'class_name': 'Orthogonal', 'config': {'gain': 1.0, 'seed': None}}
    assert cfg['kernel_initializer']['class_name'] == 'VarianceScaling' and cfg['bias_initializer'] == {'class_name': 'Zeros', 'config': {}}
    assert (cfg['units'], cfg['activation'], cfg['use_bias']) == (5, 'tanh', True)
    assert (cfg['return_sequences'], cfg['return_state'], cfg['go_backwards'], cfg['stateful'], cfg['unroll']) == (True, False, False, False, True)
    assert (cfg['dropout'], cfg['recurrent_dropout']) == (0.0, 0.0)
    assert cfg['recurrent_regularizer']['class_name'] == 'L1L2' and cfg['kernel_regularizer'] is None and cfg['kernel_constraint'] is None
    again = model_from_json(m.to_json())
    assert json.loads(again.to_json()) == json.loads(m.to_json())
    assert [l.get_config() for l in again.layers] == [l.get_config() for l in m.layers]
    assert [p.shape for p in again.layers[0].weights] == [(3, 5), (5, 5), (5,)]
    assert [p.shape for p in again.layers[1].weights] == [(5, 4), (4, 4), (4,)]


def keras_entry():
    """a SimpleRNN layer entry as keras 2.2.4 writes it"""
    return {"class_name": "SimpleRNN", "config": {
        "name": "simple_rnn_3", "trainable": True, "batch_input_shape": [None, 12, 6], "dtype": "float32", "return_sequences": False,
        "return_state": False, "go_backwards": True, "stateful": False, "unroll": False, "units": 10, "activation": "tanh", "use_bias": True,
        "kernel_initializer": {"class_name": "VarianceScaling", "config": {"scale": 1.0, "mode": "fan_avg", "distribution": "uniform", "seed": None}},
        "recurrent_initializer": {"class_name": "Orthogonal", "config": {"gain": 1.0, "seed": None}},
        "bias_initializer": {"class_name": "Zeros", "config": {}},
        "kernel_regularizer": {"class_name": "L1L2", "config": {"l1": 0.0, "l2": 0.0010000000474974513}}, "recurrent_regularizer": None,
        "bias_regularizer": None, "activity_regularizer": None, "kernel_constraint": None, "recurrent_constraint": None, "bias_constraint": None,
        "dropout": 0.0, "recurrent_dropout": 0.0}}


def test_a_layer_entry_as_keras_2_2_4_writes_it_loads():
    from gennet_amd.engine import model_from_json
    entry = keras_entry()
    text = json.dumps({"class_name": "Sequential", "config": {"name": "sequential_1", "layers": [entry]}, "keras_version": "2.2.4", "backend": "tensorflow"})
    m = model_from_json(text)
    l = m.layers[0]
    assert type(l).__name__ == 'SimpleRNN' and (l.name, l.units, l.go_backwards, l.return_sequences) == ('simple_rnn_3', 10, True, False)
    assert m.output_shape == (None, 10) and [p.shape for p in l.weights] == [(6, 10), (10, 10), (10,)]
    assert [p.name for p in l.weights] == ['simple_rnn_3/kernel', 'simple_rnn_3/recurrent_kernel', 'simple_rnn_3/bias']
    assert l.kernel.regularizer.l2 == np.float32(0.001)
    assert l.get_config() == entry['config']
    entry['config']['recurrent_dropout'] = 0.25
    with pytest.raises(NotImplementedError, match=r'SimpleRNN\(recurrent_dropout'):
        model_from_json(json.dumps({"class_name": "Sequential", "config": {"name": "s", "layers": [entry]}}))


def test_a_bidirectional_entry_as_keras_2_2_4_writes_it_loads():
    from gennet_amd.engine import model_from_json
    inner = keras_entry()
    inner['config'].pop('batch_input_shape')
    inner['config'].pop('dtype')
    inner['config']['return_sequences'] = True
    entry = {"class_name": "Bidirectional", "config": {"name": "bidirectional_1", "trainable": True, "batch_input_shape": [None, 12, 6], "dtype": "float32",
                                                       "layer": inner, "merge_mode": "sum"}}
    m = model_from_json(json.dumps({"class_name": "Sequential", "config": {"name": "sequential_1", "layers": [entry]}, "keras_version": "2.2.4"}))
    l = m.layers[0]
    assert type(l).__name__ == 'Bidirectional' and type(l.layer).__name__ == 'SimpleRNN' and l.merge_mode == 'sum' and l.layer.go_backwards
    assert m.output_shape == (None, 12, 10)
    assert [p.name for p in l.weights] == ['bidirectional_1/%s_simple_rnn_3/%s' % (d, n) for d in ('forward', 'backward')
                                           for n in ('kernel', 'recurrent_kernel', 'bias')]
    assert l.get_config() == entry['config']
    inner['config']['recurrent_dropout'] = 0.25
    with pytest.raises(NotImplementedError, match=r'SimpleRNN\(recurrent_dropout'):
        model_from_json(json.dumps({"class_name": "Sequential", "config": {"name": "s", "layers": [entry]}}))
    entry['config']['layer'] = {"class_name": "Dense", "config": {"name": "d", "units": 3}}
    with pytest.raises(ValueError, match='LSTM or a GRU'):
        model_from_json(json.dumps({"class_name": "Sequential", "config": {"name": "s", "layers": [entry]}}))


def test_the_facade_resolves():
    import gennet_amd.keras  # noqa: F401
    from gennet_amd import layers as Ly, recurrent
    from gennet_amd.keras.layers import SimpleRNN as top
    from gennet_amd.keras.layers.recurrent import SimpleRNN as deep
    import gennet_amd.keras.layers.recurrent as mod
    assert top is deep is Ly.SimpleRNN is recurrent.SimpleRNN is mod.SimpleRNN


def test_the_planner_leaves_the_layer_alone():
    m = small_model()
    nodes = [n for n in m.nodes if type(n.layer).__name__ == 'SimpleRNN']
    assert len(nodes) == 2 and all(n.fused_act is None and n.fused_drop is None for n in nodes)
    assert not any(n.layer.fusable_act or n.layer.fusable_drop or n.layer.writes_dy(n) for n in nodes)


def test_the_header_declares_the_entry_points():
    from gennet_amd import _lib
    vp, sz, i32 = _lib.vp, _lib.sz, _lib.i32
    for name in ('gn_rnn_fwd_workspace', 'gn_rnn_bwd_workspace'):
        assert _lib.DECLS[name][0] is sz and _lib.DECLS[name][1] == [i32], name
    assert all(_lib.DECLS[n][0] is i32 for n in ('gn_rnn_fwd', 'gn_rnn_bwd', 'gn_rnn_pair_fwd', 'gn_rnn_pair_bwd'))
    assert _lib.DECLS['gn_rnn_fwd'][1] == [vp] * 8 + [sz] + [i32] * 6 + [vp]
    assert _lib.DECLS['gn_rnn_bwd'][1] == [vp] * 6 + [sz] + [i32] * 6 + [vp]
    assert _lib.DECLS['gn_rnn_pair_fwd'][1] == [vp] * 7 + [sz] + [i32] * 8 + [vp]
    assert _lib.DECLS['gn_rnn_pair_bwd'][1] == [vp] * 5 + [sz] + [i32] * 7 + [vp]


# ---------------------------------------------------------------------------------------------------------------------
# the launch geometry
# ---------------------------------------------------------------------------------------------------------------------
def test_the_geometry_walk_is_clean_under_the_host_sanitizers(tmp_path):
    """tests/tools/rnn_geom_walk.cpp includes csrc/rnn_geom.h, the header the kernels' file includes, and forms for u = 1 .. 512 every index the
    kernels form into the padded matrices and the LDS buffers, inside host buffers of the stated sizes: built with the host C++ compiler under the
    address and undefined-behaviour sanitizers and run as a program of its own."""
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    exe = os.path.join(str(tmp_path), 'rnn_geom_walk')
    cmd = [cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-I', os.path.join(ROOT, 'gennet_amd', 'csrc'),
           os.path.join(ROOT, 'tests', 'tools', 'rnn_geom_walk.cpp'), '-o', exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == 'walked 512 geometries' and lines[0].startswith('U in LDS up to u = 176 forward, 176 backward'), r.stdout


# ---------------------------------------------------------------------------------------------------------------------
# the promises of the GPU tests' cases
# ---------------------------------------------------------------------------------------------------------------------
def test_the_shape_table_covers_the_set():
    S = R.SHAPES
    assert set(s[0] for s in S) == {1, 2, 15, 16, 17, 33} and set(s[1] for s in S) == {1, 2, 3, 17} and set(s[2] for s in S) == {1, 3, 16, 17}
    assert set(s[3] for s in S) == {1, 3, 4, 15, 16, 17, 31, 32, 33, 64, 128, 129, 130, 176, 177, 260, 512} and len(S) == len(set(S)) == 24
    assert all(s[0] <= 33 and s[1] <= 17 for s in S)


@pytest.mark.parametrize('shape', R.SHAPES, ids=R.IDS)
def test_every_integer_case_stays_below_2_to_the_24(shape):
    """the reference alone: every value of the integer case is an integer, every sum of absolute values lies below 2^24, at the shape's full T,
    and the recurrent path carries something (h differs from act(zx + b) and dh0 from zero wherever there is a second step or an h0)"""
    c = R.integer_case(shape)
    assert c['big'] < 2 ** 24, c['big']
    assert len(c['cases']) == 3 and [(rev, dy.ndim) for rev, dy, _, _ in c['cases']] == [(False, 3), (True, 3), (True, 2)]
    for reverse, dy, k, r in c['cases']:
        assert k['h'].shape == (shape[0], shape[1], shape[3])
        for v in (k['h'], k['h_prev'], r['dz'], r['dh0']):
            assert np.array_equal(v, np.rint(v))
    assert np.abs(c['U']).sum(0).max() <= 3 and np.abs(c['U']).sum(1).max() <= 3
    if shape[0] * shape[3] >= 16:
        assert np.abs(c['cases'][0][2]['h_prev'] @ c['U']).max() > 0 and np.abs(c['cases'][0][3]['dh0']).max() > 0


@pytest.mark.parametrize('activation', R.ACTIVATIONS)
@pytest.mark.parametrize('family', R.FAMILIES)
@pytest.mark.parametrize('shape', R.SHAPES, ids=R.IDS)
def test_every_sequence_case_has_a_seed(shape, family, activation):
    """the rule of tests/test_rnn_gpu.py's sequence test, from the reference alone: one of the seeds 0 .. 31 keeps every pre-activation at least 64
    times the fp32 restatement's largest pre-activation error away from a derivative jump"""
    case = R.sequence_case(shape, family, activation)
    assert case is not None, 'no seed in 0 .. 31 keeps the pre-activations away from the derivative jumps'
    k64, k32 = case['k64'], case['k32']
    assert R.kink_margin(k64) >= 64 * float(np.abs(k32['pre'] - k64['pre']).max()) > 0
    if family == 'saturating' and activation == 'tanh' and shape[1] > 1 and shape[0] * shape[1] * shape[3] >= 64:
        assert (np.abs(k64['h']) > 0.99).mean() > 0.05                # the family does saturate (one step from h = 0 has x W + b alone)
