"""keras layers.GRU without a GPU: the fp64 definition tests/gru_ref.py against torch.nn.GRU and torch autograd, the layer's host side -- shapes,
weights, initializers, refusals, config and JSON, the facade, the header --, the launch geometry walked under the host sanitizers, and the seed
rule of the GPU sequence test."""
import itertools
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import gru_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rel(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-300)


def draw(rng, B, T, Cin, u, reset_after):
    d = dict(x=rng.randn(B, T, Cin), W=rng.randn(Cin, 3 * u) / np.sqrt(Cin), U=rng.randn(u, 3 * u) / np.sqrt(u), b=0.3 * rng.randn(3 * u),
             h0=0.5 * rng.randn(B, u))
    if reset_after:
        d['rb'] = 0.3 * rng.randn(3 * u)
    return d


@pytest.mark.parametrize('go_backwards', [False, True])
def test_the_reference_is_torch_nn_gru_in_fp64(go_backwards):
    """reset_after=True with sigmoid gates and tanh is the form torch implements: its gate order is r, z, n, so the column blocks are permuted
    (z, r, h) -> (r, z, n); weight_ih = kernel^T, weight_hh = recurrent_kernel^T, bias_ih = b, bias_hh = rb"""
    B, T, Cin, u = 3, 6, 4, 5
    d = draw(np.random.RandomState(1), B, T, Cin, u, True)
    y, _ = R.forward(d['x'], d['W'], d['U'], d['b'], d['rb'], d['h0'], 'tanh', 'sigmoid', True, return_sequences=True, go_backwards=go_backwards)
    perm = np.concatenate([np.arange(u, 2 * u), np.arange(u), np.arange(2 * u, 3 * u)])
    m = torch.nn.GRU(Cin, u, batch_first=True).double()
    with torch.no_grad():
        m.weight_ih_l0.copy_(torch.tensor(d['W'][:, perm].T.copy()))
        m.weight_hh_l0.copy_(torch.tensor(d['U'][:, perm].T.copy()))
        m.bias_ih_l0.copy_(torch.tensor(d['b'][perm]))
        m.bias_hh_l0.copy_(torch.tensor(d['rb'][perm]))
        x = torch.tensor(d['x'][:, ::-1].copy() if go_backwards else d['x'])
        out, hn = m(x, torch.tensor(d['h0'])[None])
    assert rel(y, out.numpy()) < 1e-12 and rel(y[:, -1], hn[0].numpy()) < 1e-12


COMBOS = list(itertools.product(R.ACTIVATIONS, R.RECURRENT_ACTIVATIONS, (False, True)))


@pytest.mark.parametrize('go_backwards', [False, True])
@pytest.mark.parametrize('return_sequences', [False, True])
@pytest.mark.parametrize('activation,recurrent_activation,reset_after', COMBOS, ids=['%s-%s-ra%d' % c for c in COMBOS])
def test_the_reference_gradients_are_torch_autograd_in_fp64(activation, recurrent_activation, reset_after, return_sequences, go_backwards):
    B, T, Cin, u = 3, 5, 4, 6
    d = draw(np.random.RandomState(2), B, T, Cin, u, reset_after)
    d['b'][:2 * u] *= 6                      # some hard_sigmoid gates saturate
    kw = dict(activation=activation, recurrent_activation=recurrent_activation, reset_after=reset_after, return_sequences=return_sequences,
              go_backwards=go_backwards)
    y, k = R.forward(d['x'], d['W'], d['U'], d['b'], d.get('rb'), d['h0'], **kw)
    if recurrent_activation == 'hard_sigmoid':            # some gate evaluations are saturated, none sits on a kink
        q = k['pre'][:, :, :2 * u]
        assert (np.abs(q) > 2.5).any() and (np.abs(q) < 2.5).any() and np.abs(np.abs(q) - 2.5).min() > 1e-6
    dy = np.random.RandomState(3).randn(*y.shape)
    t = dict((n, torch.tensor(v, requires_grad=True)) for n, v in d.items())
    yt = R.torch_forward(t['x'], t['W'], t['U'], t['b'], t.get('rb'), t['h0'], **kw)
    assert rel(y, yt.detach().numpy()) < 1e-12
    (yt * torch.tensor(dy)).sum().backward()
    g = R.backward(k, dy)
    pairs = [('dx', 'x'), ('dW', 'W'), ('dU', 'U'), ('db', 'b'), ('dh0', 'h0')] + ([('drb', 'rb')] if reset_after else [])
    for mine, theirs in pairs:
        assert rel(g[mine], t[theirs].grad.numpy()) < 1e-12, mine


@pytest.mark.parametrize('reset_after', [False, True])
def test_the_fp32_restatement_is_the_same_recurrence(reset_after):
    d = draw(np.random.RandomState(4), 2, 9, 3, 7, reset_after)
    y64, _ = R.forward(d['x'], d['W'], d['U'], d['b'], d.get('rb'), reset_after=reset_after, return_sequences=True)
    y32, k = R.forward(d['x'], d['W'], d['U'], d['b'], d.get('rb'), reset_after=reset_after, return_sequences=True, dtype=np.float32)
    assert y32.dtype == np.float32 and k['gates'].dtype == np.float32 and k['aux'].dtype == np.float32 and 0 < np.abs(y32 - y64).max() < 1e-5
    g = R.recurrence_backward(k, np.ones_like(y32))
    assert g['dz'].dtype == np.float32 and g['dh0'].dtype == np.float32


# ---------------------------------------------------------------------------------------------------------------------
# the layer's host side
# ---------------------------------------------------------------------------------------------------------------------
def test_shapes_weight_order_names_and_initial_values():
    from gennet_amd import engine, layers as Ly
    engine.set_init_seed(7)
    x = engine.Input((9, 3))
    last, seq = Ly.GRU(5, name='enc'), Ly.GRU(4, return_sequences=True, reset_after=True)
    assert last(x).shape == (5,) and seq(x).shape == (9, 4)
    assert [p.name for p in last.weights] == ['enc/kernel', 'enc/recurrent_kernel', 'enc/bias']
    assert [p.shape for p in last.weights] == [(3, 15), (5, 15), (15,)] and last.count_params() == 3 * (3 * 5 + 5 * 5 + 5)
    assert [p.shape for p in seq.weights] == [(3, 12), (4, 12), (2, 12)] and seq.count_params() == 3 * (3 * 4 + 4 * 4 + 2 * 4)
    W, U, b = last.get_weights()
    assert W.dtype == U.dtype == b.dtype == np.float32
    lim = np.sqrt(6.0 / (3 + 15))
    assert np.abs(W).max() <= lim and np.abs(W).max() > 0.5 * lim                      # Glorot uniform over (Cin, 3u)
    assert not b.any() and not seq.get_weights()[2].any() and seq.get_weights()[2].shape == (2, 12)
    for q in range(3):                                                                # three orthogonal u x u blocks
        Q = U[:, 5 * q:5 * q + 5].astype(np.float64)
        assert np.abs(Q.T @ Q - np.eye(5)).max() < 1e-6
    assert not np.allclose(U[:, :5], U[:, 5:10])
    engine.set_init_seed(7)                                                           # the generator glorot_uniform draws from
    again = Ly.GRU(5)
    again(engine.Input((9, 3)))
    assert all(np.array_equal(a, b) for a, b in zip(again.get_weights(), last.get_weights()))
    with pytest.raises(ValueError, match='timesteps'):
        Ly.GRU(3)(engine.Input((9,)))
    with pytest.raises(NotImplementedError, match='512'):
        Ly.GRU(513)(engine.Input((4, 2)))


def test_regularizers_ride_on_the_weights():
    from gennet_amd import engine, layers as Ly, regularizers
    l = Ly.GRU(3, kernel_regularizer=regularizers.l2(0.01), recurrent_regularizer='l1', bias_regularizer=regularizers.l1_l2(0.1, 0.2),
               activity_regularizer=regularizers.l2(0.5), reset_after=True)
    l(engine.Input((4, 2)))
    assert [(p.regularizer.l1, p.regularizer.l2) for p in l.weights] == [(0.0, np.float32(0.01)), (np.float32(0.01), 0.0), (np.float32(0.1), np.float32(0.2))]
    assert l.activity_regularizer.l2 == np.float32(0.5) and l.bias.shape == (2, 9)          # the bias regularizer sees both rows


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
    with pytest.raises(NotImplementedError, match=r'GRU\(%s' % name):
        Ly.GRU(4, **kw)


def test_accepted_spellings():
    from gennet_amd import layers as Ly
    from gennet_amd.keras import activations
    l = Ly.GRU(4, activation=activations.relu, recurrent_activation='sigmoid', dropout=0.0, recurrent_dropout=0, stateful=False, return_state=False,
               kernel_constraint=None, implementation=2, unroll=True, kernel_initializer={'class_name': 'GlorotUniform', 'config': {'seed': None}},
               reset_after=1)
    assert (l.activation, l.recurrent_activation, l.implementation, l.unroll, l.reset_after) == ('relu', 'sigmoid', 2, True, True)
    assert Ly.GRU(4, activation=None).activation == 'linear' and Ly.GRU(4).reset_after is False
    with pytest.raises(ValueError, match='implementation'):
        Ly.GRU(4, implementation=3)
    with pytest.raises(ValueError, match='at least 1'):
        Ly.GRU(0)


# the keys of keras 2.2.4 GRU.get_config: LSTM's without unit_forget_bias, with reset_after
KERAS_KEYS = {'name', 'trainable', 'return_sequences', 'return_state', 'go_backwards', 'stateful', 'unroll', 'units', 'activation',
              'recurrent_activation', 'use_bias', 'kernel_initializer', 'recurrent_initializer', 'bias_initializer', 'kernel_regularizer',
              'recurrent_regularizer', 'bias_regularizer', 'activity_regularizer', 'kernel_constraint', 'recurrent_constraint', 'bias_constraint',
              'dropout', 'recurrent_dropout', 'implementation', 'reset_after'}


def small_model():
    from gennet_amd import layers as Ly
    from gennet_amd.engine import Sequential
    m = Sequential()
    m.add(Ly.GRU(5, input_shape=(7, 3), return_sequences=True, recurrent_regularizer='l2', implementation=2, unroll=True, reset_after=True))
    m.add(Ly.GRU(4, activation='relu', recurrent_activation='sigmoid', go_backwards=True))
    m.add(Ly.Dense(1))
    return m


def test_config_round_trip():
    from gennet_amd.engine import model_from_json
    m = small_model()
    cfg = m.layers[0].get_config()
    assert set(cfg) == KERAS_KEYS | {'batch_input_shape', 'dtype'} and set(m.layers[1].get_config()) == KERAS_KEYS
    assert cfg['recurrent_initializer'] == {'class_name': 'Orthogonal', 'config': {'gain': 1.0, 'seed': None}}
    assert cfg['kernel_initializer']['class_name'] == 'VarianceScaling' and cfg['bias_initializer'] == {'class_name': 'Zeros', 'config': {}}
    assert (cfg['units'], cfg['activation'], cfg['recurrent_activation'], cfg['use_bias'], cfg['reset_after']) == (5, 'tanh', 'hard_sigmoid', True, True)
    assert (cfg['return_sequences'], cfg['return_state'], cfg['go_backwards'], cfg['stateful'], cfg['unroll']) == (True, False, False, False, True)
    assert (cfg['dropout'], cfg['recurrent_dropout'], cfg['implementation']) == (0.0, 0.0, 2)
    assert cfg['recurrent_regularizer']['class_name'] == 'L1L2' and cfg['kernel_regularizer'] is None and cfg['kernel_constraint'] is None
    assert m.layers[1].get_config()['reset_after'] is False
    again = model_from_json(m.to_json())
    assert json.loads(again.to_json()) == json.loads(m.to_json())
    assert [l.get_config() for l in again.layers] == [l.get_config() for l in m.layers]
    assert [p.shape for p in again.layers[0].weights] == [(3, 15), (5, 15), (2, 15)]
    assert [p.shape for p in again.layers[1].weights] == [(5, 12), (4, 12), (12,)]


@pytest.mark.parametrize('reset_after', [False, True])
def test_a_layer_entry_as_keras_2_2_4_writes_it_loads(reset_after):
    from gennet_amd.engine import model_from_json
    entry = {"class_name": "GRU", "config": {
        "name": "gru_3", "trainable": True, "batch_input_shape": [None, 12, 6], "dtype": "float32", "return_sequences": False, "return_state": False,
        "go_backwards": True, "stateful": False, "unroll": False, "units": 10, "activation": "tanh", "recurrent_activation": "hard_sigmoid",
        "use_bias": True, "kernel_initializer": {"class_name": "VarianceScaling", "config": {"scale": 1.0, "mode": "fan_avg", "distribution": "uniform",
                                                                                            "seed": None}},
        "recurrent_initializer": {"class_name": "Orthogonal", "config": {"gain": 1.0, "seed": None}},
        "bias_initializer": {"class_name": "Zeros", "config": {}},
        "kernel_regularizer": {"class_name": "L1L2", "config": {"l1": 0.0, "l2": 0.0010000000474974513}}, "recurrent_regularizer": None,
        "bias_regularizer": None, "activity_regularizer": None, "kernel_constraint": None, "recurrent_constraint": None, "bias_constraint": None,
        "dropout": 0.0, "recurrent_dropout": 0.0, "implementation": 1, "reset_after": reset_after}}
    text = json.dumps({"class_name": "Sequential", "config": {"name": "sequential_1", "layers": [entry]}, "keras_version": "2.2.4", "backend": "tensorflow"})
    m = model_from_json(text)
    l = m.layers[0]
    assert type(l).__name__ == 'GRU' and (l.name, l.units, l.go_backwards, l.return_sequences, l.reset_after) == ('gru_3', 10, True, False, reset_after)
    assert m.output_shape == (None, 10) and [p.shape for p in l.weights] == [(6, 30), (10, 30), (2, 30) if reset_after else (30,)]
    assert l.kernel.regularizer.l2 == np.float32(0.001)
    assert l.get_config() == entry['config']
    entry['config']['recurrent_dropout'] = 0.25
    with pytest.raises(NotImplementedError, match='recurrent_dropout'):
        model_from_json(json.dumps({"class_name": "Sequential", "config": {"name": "s", "layers": [entry]}}))


def test_the_facade_resolves():
    import gennet_amd.keras  # noqa: F401
    from gennet_amd import layers as Ly, recurrent
    from gennet_amd.keras.layers import GRU as top
    from gennet_amd.keras.layers.recurrent import GRU as deep
    import gennet_amd.keras.layers.recurrent as mod
    assert top is deep is Ly.GRU is recurrent.GRU is mod.GRU
    assert 'GRU' in gennet_amd.keras.__doc__


def test_the_planner_leaves_the_layer_alone():
    m = small_model()
    nodes = [n for n in m.nodes if type(n.layer).__name__ == 'GRU']
    assert len(nodes) == 2 and all(n.fused_act is None and n.fused_drop is None for n in nodes)
    assert not any(n.layer.fusable_act or n.layer.fusable_drop or n.layer.writes_dy(n) for n in nodes)


def test_the_header_declares_the_entry_points():
    from gennet_amd import _lib
    for name, ret, nargs in (('gn_gru_fwd', _lib.i32, 20), ('gn_gru_bwd', _lib.i32, 19), ('gn_gru_fwd_workspace', _lib.sz, 1),
                             ('gn_gru_bwd_workspace', _lib.sz, 1)):
        assert _lib.DECLS[name][0] is ret and len(_lib.DECLS[name][1]) == nargs, name
    vp, sz, i32 = _lib.vp, _lib.sz, _lib.i32
    assert _lib.DECLS['gn_gru_fwd'][1] == [vp] * 10 + [sz] + [i32] * 8 + [vp]
    assert _lib.DECLS['gn_gru_bwd'][1] == [vp] * 9 + [sz] + [i32] * 8 + [vp]


# ---------------------------------------------------------------------------------------------------------------------
# the launch geometry
# ---------------------------------------------------------------------------------------------------------------------
def test_the_geometry_walk_is_clean_under_the_host_sanitizers(tmp_path):
    """tests/tools/gru_geom_walk.cpp includes csrc/gru_geom.h, the header the kernels' file includes, and forms for u = 1 .. 512 every index the
    kernels form into the padded matrices and the LDS state, inside host buffers of the stated sizes: built with the host C++ compiler under the
    address and undefined-behaviour sanitizers and run as a program of its own."""
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    exe = os.path.join(str(tmp_path), 'gru_geom_walk')
    cmd = [cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-I', os.path.join(ROOT, 'gennet_amd', 'csrc'),
           os.path.join(ROOT, 'tests', 'tools', 'gru_geom_walk.cpp'), '-o', exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == 'walked 512 geometries' and lines[0].startswith('U in LDS up to u = 104 forward, 104 backward'), r.stdout


# ---------------------------------------------------------------------------------------------------------------------
# the seed rule of the GPU sequence test
# ---------------------------------------------------------------------------------------------------------------------
def test_the_shape_table_covers_the_set():
    S = R.SHAPES
    assert set(s[0] for s in S) == {1, 2, 15, 16, 17, 33} and set(s[1] for s in S) == {1, 2, 3, 17} and set(s[2] for s in S) == {1, 3, 16, 17}
    assert set(s[3] for s in S) == {1, 3, 4, 15, 16, 17, 31, 32, 33, 64, 100, 104, 105, 112, 130, 260, 512} and len(S) == len(set(S)) == 24


@pytest.mark.parametrize('reset_after', [False, True], ids=['ra0', 'ra1'])
@pytest.mark.parametrize('family', ['keras', 'saturating'])
@pytest.mark.parametrize('shape', R.SHAPES, ids=R.IDS)
def test_every_sequence_case_has_a_seed(shape, family, reset_after):
    """the rule of tests/test_gru_gpu.py's sequence test, from the reference alone: one of the seeds 0 .. 31 keeps every pre-activation at least 64
    times the fp32 restatement's largest pre-activation error away from a derivative jump"""
    case = R.sequence_case(shape, family, reset_after)
    assert case is not None, 'no seed in 0 .. 31 keeps the pre-activations away from the derivative jumps'
    k64, k32 = case['k64'], case['k32']
    assert R.kink_margin(k64) >= 64 * float(np.abs(k32['pre'] - k64['pre']).max()) > 0
    u = shape[3]
    if family == 'saturating' and case['recurrent_activation'] == 'hard_sigmoid' and shape[1] > 1 and shape[0] * shape[1] * u >= 64:
        assert (np.abs(k64['pre'][:, :, :2 * u]) > 2.5).mean() > 0.05                 # the family does saturate (one step from h = 0 has x W + b alone)
