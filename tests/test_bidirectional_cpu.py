"""keras layers.Bidirectional without a GPU: the layer's host side -- shapes, the six weights and their draw, refusals, config and JSON, the .h5
weight layout, the facade, the header -- and the flip and merge of the fp64 restatement tests/bidirectional_ref.py on a hand-worked case."""
import json

import numpy as np
import pytest

import bidirectional_ref as BR
from gennet_amd import h5lite

MODES = ('concat', 'sum', 'mul', 'ave')


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


def wrap(inner, merge_mode='concat', shape=(9, 3), **kw):
    from gennet_amd import engine, layers as Ly
    l = Ly.Bidirectional(inner, merge_mode=merge_mode, **kw)
    return l, l(engine.Input(shape))


@pytest.mark.parametrize('return_sequences', [False, True])
@pytest.mark.parametrize('merge_mode', MODES)
@pytest.mark.parametrize('cell', ['LSTM', 'GRU'])
def test_output_shapes(cell, merge_mode, return_sequences):
    from gennet_amd import layers as Ly
    l, y = wrap(getattr(Ly, cell)(5, return_sequences=return_sequences), merge_mode)
    width = 10 if merge_mode == 'concat' else 5
    assert y.shape == ((9, width) if return_sequences else (width,))
    assert l.merge_mode == merge_mode and type(l.layer).__name__ == cell and not l.layer.built and not l.layer.weights


def test_what_is_no_recurrent_layer_and_an_unknown_merge_mode_are_value_errors():
    from gennet_amd import engine, layers as Ly
    with pytest.raises(ValueError, match='Bidirectional'):
        Ly.Bidirectional(Ly.Dense(4))
    with pytest.raises(ValueError, match='Bidirectional'):
        Ly.Bidirectional('lstm')
    built = Ly.LSTM(3)
    built(engine.Input((4, 2)))
    with pytest.raises(ValueError, match='already built'):
        Ly.Bidirectional(built)
    with pytest.raises(ValueError, match='merge mode'):
        Ly.Bidirectional(Ly.LSTM(3), merge_mode='max')
    with pytest.raises(ValueError, match='timesteps'):
        Ly.Bidirectional(Ly.LSTM(3))(engine.Input((9,)))
    with pytest.raises(NotImplementedError, match='512'):
        Ly.Bidirectional(Ly.GRU(513))(engine.Input((4, 2)))


def test_what_does_not_run_is_refused_by_name():
    from gennet_amd import layers as Ly, regularizers
    with pytest.raises(NotImplementedError, match=r'Bidirectional\(merge_mode=None'):
        Ly.Bidirectional(Ly.LSTM(3), merge_mode=None)
    with pytest.raises(NotImplementedError, match=r'Bidirectional\(weights='):
        Ly.Bidirectional(Ly.LSTM(3), weights=[np.zeros((2, 12), np.float32)] * 6)
    for cell in (Ly.LSTM, Ly.GRU):
        with pytest.raises(NotImplementedError, match='activity_regularizer'):
            Ly.Bidirectional(cell(3, activity_regularizer=regularizers.l2(0.1)))
    with pytest.raises(NotImplementedError, match=r'LSTM\(stateful'):         # the inner layer's own refusals stay the inner constructor's
        Ly.Bidirectional(Ly.LSTM(3, stateful=True))
    with pytest.raises(NotImplementedError, match=r'GRU\(recurrent_dropout'):
        Ly.Bidirectional(Ly.GRU(3, recurrent_dropout=0.5))
    assert Ly.Bidirectional(Ly.LSTM(3), weights=None).merge_mode == 'concat'


def test_the_six_weights_their_names_order_shapes_and_regularizers():
    from gennet_amd import layers as Ly, regularizers
    inner = Ly.GRU(4, name='enc', kernel_regularizer=regularizers.l2(0.01), recurrent_regularizer='l1', bias_regularizer=regularizers.l1_l2(0.1, 0.2),
                   reset_after=True)
    l, _ = wrap(inner, 'sum', name='both')
    names = ['both/%s_enc/%s' % (d, w) for d in ('forward', 'backward') for w in ('kernel', 'recurrent_kernel', 'bias')]
    assert [p.name for p in l.weights] == names and [p.name for p in l.trainable_weights] == names and not l.non_trainable_weights
    assert [p.shape for p in l.weights] == [(3, 12), (4, 12), (2, 12)] * 2 and l.count_params() == 2 * 3 * (3 * 4 + 4 * 4 + 2 * 4)
    assert [(p.regularizer.l1, p.regularizer.l2) for p in l.weights] == [(0.0, np.float32(0.01)), (np.float32(0.01), 0.0),
                                                                         (np.float32(0.1), np.float32(0.2))] * 2
    assert l.forward_weights == tuple(l.weights[:3]) and l.backward_weights == tuple(l.weights[3:])
    plain, _ = wrap(Ly.LSTM(5))
    assert plain.name.startswith('bidirectional_') and plain.layer.name.startswith('lstm_')
    assert [p.name for p in plain.weights] == ['%s/%s_%s/%s' % (plain.name, d, plain.layer.name, w) for d in ('forward', 'backward')
                                               for w in ('kernel', 'recurrent_kernel', 'bias')]
    assert all(p.regularizer is None for p in plain.weights)


@pytest.mark.parametrize('cell,kw', [('LSTM', {}), ('LSTM', dict(unit_forget_bias=False)), ('GRU', {}), ('GRU', dict(reset_after=True))])
def test_the_forward_triple_is_a_lone_inner_layers_draw_and_the_backward_triple_another(cell, kw):
    from gennet_amd import engine, layers as Ly
    u = 5
    engine.set_init_seed(11)
    l, _ = wrap(getattr(Ly, cell)(u, **kw))
    engine.set_init_seed(11)
    lone = getattr(Ly, cell)(u, **kw)
    lone(engine.Input((9, 3)))
    ws = l.get_weights()
    assert all(np.array_equal(a, b) for a, b in zip(ws[:3], lone.get_weights()))
    assert not np.array_equal(ws[0], ws[3]) and not np.array_equal(ws[1], ws[4])
    G = 4 if cell == 'LSTM' else 3
    for U in (ws[1], ws[4]):                                                          # orthogonal u x u blocks in both triples
        for q in range(G):
            Q = U[:, u * q:u * q + u].astype(np.float64)
            assert np.abs(Q.T @ Q - np.eye(u)).max() < 1e-6
    for b in (ws[2], ws[5]):
        if cell == 'LSTM':
            want = np.zeros(4 * u, np.float32)
            want[u:2 * u] = 0.0 if kw else 1.0                                        # unit_forget_bias on both triples
        else:
            want = np.zeros((2, 3 * u) if kw else (3 * u,), np.float32)               # the (2, 3u) bias of reset_after on both
        assert b.shape == want.shape and np.array_equal(b, want)


# the keys of keras 2.2.4 Bidirectional.get_config: Wrapper's name, trainable, layer and the merge_mode
KERAS_KEYS = {'name', 'trainable', 'layer', 'merge_mode'}


def small_model():
    from gennet_amd import layers as Ly
    from gennet_amd.engine import Sequential
    m = Sequential()
    m.add(Ly.Bidirectional(Ly.LSTM(5, return_sequences=True, recurrent_regularizer='l2', name='inner_a'), input_shape=(7, 3)))
    m.add(Ly.Bidirectional(Ly.GRU(4, go_backwards=True, reset_after=True), merge_mode='ave'))
    m.add(Ly.Dense(1))
    return m


def test_config_round_trip():
    from gennet_amd.engine import model_from_json
    m = small_model()
    cfg = m.layers[0].get_config()
    assert set(cfg) == KERAS_KEYS | {'batch_input_shape', 'dtype'} and set(m.layers[1].get_config()) == KERAS_KEYS
    assert cfg['merge_mode'] == 'concat' and cfg['layer']['class_name'] == 'LSTM' and set(cfg['layer']) == {'class_name', 'config'}
    inner = cfg['layer']['config']
    assert (inner['name'], inner['units'], inner['return_sequences'], inner['go_backwards']) == ('inner_a', 5, True, False)
    assert inner['recurrent_regularizer']['class_name'] == 'L1L2' and 'batch_input_shape' not in inner
    second = m.layers[1].get_config()
    assert second['merge_mode'] == 'ave' and second['layer']['class_name'] == 'GRU'
    assert second['layer']['config']['go_backwards'] is True and second['layer']['config']['reset_after'] is True      # as given, not the copies'
    again = model_from_json(m.to_json())
    assert json.loads(again.to_json()) == json.loads(m.to_json())
    assert [l.get_config() for l in again.layers] == [l.get_config() for l in m.layers]
    assert [[p.name for p in l.weights] for l in again.layers] == [[p.name for p in l.weights] for l in m.layers]
    assert [p.shape for p in again.layers[0].weights] == [(3, 20), (5, 20), (20,)] * 2
    assert [p.shape for p in again.layers[1].weights] == [(10, 12), (4, 12), (2, 12)] * 2
    assert again.layers[0].weights[1].regularizer.l2 == np.float32(0.01) and again.layers[0].weights[4].regularizer.l2 == np.float32(0.01)
    assert m.output_shape == again.output_shape == (None, 1) and [n.out_shape for n in again.nodes] == [(7, 10), (4,), (1,)]


@pytest.mark.parametrize('go_backwards', [False, True])
def test_a_layer_entry_as_keras_2_2_4_writes_it_loads(go_backwards):
    from gennet_amd.engine import model_from_json
    entry = {"class_name": "Bidirectional", "config": {
        "name": "bidirectional_7", "trainable": True, "batch_input_shape": [None, 12, 6], "dtype": "float32",
        "layer": {"class_name": "LSTM", "config": {
            "name": "lstm_9", "trainable": True, "return_sequences": True, "return_state": False, "go_backwards": go_backwards, "stateful": False,
            "unroll": False, "units": 10, "activation": "tanh", "recurrent_activation": "hard_sigmoid", "use_bias": True,
            "kernel_initializer": {"class_name": "VarianceScaling", "config": {"scale": 1.0, "mode": "fan_avg", "distribution": "uniform", "seed": None}},
            "recurrent_initializer": {"class_name": "Orthogonal", "config": {"gain": 1.0, "seed": None}},
            "bias_initializer": {"class_name": "Zeros", "config": {}}, "unit_forget_bias": True,
            "kernel_regularizer": {"class_name": "L1L2", "config": {"l1": 0.0, "l2": 0.0010000000474974513}}, "recurrent_regularizer": None,
            "bias_regularizer": None, "activity_regularizer": None, "kernel_constraint": None, "recurrent_constraint": None, "bias_constraint": None,
            "dropout": 0.0, "recurrent_dropout": 0.0, "implementation": 1}},
        "merge_mode": "sum"}}
    text = json.dumps({"class_name": "Sequential", "config": {"name": "sequential_1", "layers": [entry]}, "keras_version": "2.2.4", "backend": "tensorflow"})
    m = model_from_json(text)
    l = m.layers[0]
    assert type(l).__name__ == 'Bidirectional' and type(l.layer).__name__ == 'LSTM' and (l.name, l.merge_mode) == ('bidirectional_7', 'sum')
    assert (l.layer.name, l.layer.units, l.layer.go_backwards, l.layer.return_sequences) == ('lstm_9', 10, go_backwards, True)
    assert m.output_shape == (None, 12, 10) and [p.shape for p in l.weights] == [(6, 40), (10, 40), (40,)] * 2
    assert [p.name for p in l.weights][::3] == ['bidirectional_7/forward_lstm_9/kernel', 'bidirectional_7/backward_lstm_9/kernel']
    assert l.weights[0].regularizer.l2 == l.weights[3].regularizer.l2 == np.float32(0.001)
    got = l.get_config()
    assert got == entry['config'] and set(got['layer']['config']) == set(entry['config']['layer']['config'])
    entry['config']['layer']['config']['recurrent_dropout'] = 0.25
    with pytest.raises(NotImplementedError, match='recurrent_dropout'):
        model_from_json(json.dumps({"class_name": "Sequential", "config": {"name": "s", "layers": [entry]}}))
    entry['config']['layer'] = {"class_name": "Dense", "config": {"name": "dense_1", "units": 3}}
    with pytest.raises(ValueError, match='LSTM or a GRU'):
        model_from_json(json.dumps({"class_name": "Sequential", "config": {"name": "s", "layers": [entry]}}))


def test_h5_weights_on_the_host(tmp_path):
    """the six datasets under the wrapper's group, weight_names in keras' order, the values; a twin loads them"""
    m = small_model()
    rng = np.random.RandomState(3)
    for l in m.layers:
        l.set_weights([rng.randn(*w.shape).astype(np.float32) for w in l.get_weights()])
    path = str(tmp_path / 'bi.h5')
    m.save_weights(path, True)
    f = h5lite.File(path)
    assert [n.decode() for n in f.attrs['layer_names'].tolist()] == [l.name for l in m.layers]
    for l in m.layers[:2]:
        inner = l.layer.name
        want = ['%s/%s_%s/%s:0' % (l.name, d, inner, w) for d in ('forward', 'backward') for w in ('kernel', 'recurrent_kernel', 'bias')]
        assert [n.decode() for n in f[l.name].attrs['weight_names'].tolist()] == want
        for n, p in zip(want, l.weights):
            node = f[l.name]
            for part in n.split('/'):
                node = node[part]
            assert node.dtype == np.float32 and np.array_equal(node.value, p.numpy())
    twin = small_model()
    assert not all(np.array_equal(a, b) for a, b in zip(twin.get_weights(), m.get_weights()))
    twin.load_weights(path)
    assert all(np.array_equal(a, b) for a, b in zip(twin.get_weights(), m.get_weights()))
    from gennet_amd import layers as Ly
    from gennet_amd.engine import Sequential
    other = Sequential()
    other.add(Ly.Bidirectional(Ly.LSTM(5, return_sequences=True), input_shape=(7, 3)))
    other.add(Ly.Bidirectional(Ly.GRU(4), merge_mode='ave'))                          # the bias is (12,), not (2, 12)
    other.add(Ly.Dense(1))
    with pytest.raises(ValueError, match='shape'):
        other.load_weights(path)


def test_the_facade_resolves():
    import gennet_amd.keras  # noqa: F401
    from gennet_amd import layers as Ly, recurrent
    from gennet_amd.keras.layers import Bidirectional as top
    from gennet_amd.keras.layers.wrappers import Bidirectional as deep
    import gennet_amd.keras.layers.wrappers as mod
    assert top is deep is Ly.Bidirectional is recurrent.Bidirectional is mod.Bidirectional
    assert 'Bidirectional' in gennet_amd.keras.__doc__


def test_the_planner_leaves_the_layer_alone():
    m = small_model()
    nodes = [n for n in m.nodes if type(n.layer).__name__ == 'Bidirectional']
    assert len(nodes) == 2 and all(n.fused_act is None and n.fused_drop is None for n in nodes)
    assert not any(n.layer.fusable_act or n.layer.fusable_drop or n.layer.writes_dy(n) for n in nodes)


def test_the_header_declares_the_entry_points():
    from gennet_amd import _lib
    vp, sz, i32 = _lib.vp, _lib.sz, _lib.i32
    want = {'gn_lstm_pair_fwd': [vp] * 8 + [sz] + [i32] * 9 + [vp], 'gn_lstm_pair_bwd': [vp] * 6 + [sz] + [i32] * 8 + [vp],
            'gn_gru_pair_fwd': [vp] * 9 + [sz] + [i32] * 10 + [vp], 'gn_gru_pair_bwd': [vp] * 8 + [sz] + [i32] * 9 + [vp]}
    for name, args in want.items():
        assert _lib.DECLS[name][0] is i32 and _lib.DECLS[name][1] == args, name
    # the single-direction entry points keep their signatures
    assert [len(_lib.DECLS[n][1]) for n in ('gn_lstm_fwd', 'gn_lstm_bwd', 'gn_gru_fwd', 'gn_gru_bwd')] == [19, 18, 20, 19]


def test_the_references_flip_and_merge_on_a_hand_worked_case():
    """T = 2, u = 1, B = 1, Cin = 1, activation 'linear', sigmoid gates driven by biases of +-40 (1 or 0 to the last bit of fp64), W_c = 1, U = 0.
    LSTM with i = 1, f = 1, o = 1: c_t = c_{t-1} + x_t, h_t = c_t.  On x = (2, 5):
      forward copy   h = (2, 7)                       backward copy, processing order: h = (5, 7); flipped into time order: (7, 5)
    The backward copy takes W_c = 3: processing order (15, 21), time order (21, 15)."""
    x = np.array([[[2.0], [5.0]]])
    W = np.array([[0.0, 0.0, 1.0, 0.0]])
    U = np.zeros((1, 4))
    b = np.array([40.0, 40.0, 0.0, 40.0])
    weights = [W, U, b, 3 * W, U, b]
    kw = dict(activation='linear', recurrent_activation='sigmoid')
    seq = dict(kw, return_sequences=True)
    assert np.array_equal(BR.forward('lstm', x, weights, 'concat', **seq), [[[2.0, 21.0], [7.0, 15.0]]])
    assert np.array_equal(BR.forward('lstm', x, weights, 'sum', **seq), [[[23.0], [22.0]]])
    assert np.array_equal(BR.forward('lstm', x, weights, 'mul', **seq), [[[42.0], [105.0]]])
    assert np.array_equal(BR.forward('lstm', x, weights, 'ave', **seq), [[[11.5], [11.0]]])
    # without sequences each half is its LAST PROCESSED step: 7 and 21, and nothing is flipped
    assert np.array_equal(BR.forward('lstm', x, weights, 'concat', **kw), [[7.0, 21.0]])
    assert np.array_equal(BR.forward('lstm', x, weights, 'ave', **kw), [[14.0]])
    # an inner go_backwards=True: the forward copy walks backwards, (5, 7) in processing order, and stays so; the backward copy walks forwards,
    # (6, 21), and is flipped by position: (21, 6)
    assert np.array_equal(BR.forward('lstm', x, weights, 'concat', go_backwards=True, **seq), [[[5.0, 21.0], [7.0, 6.0]]])
    import torch
    t = BR.torch_forward('lstm', torch.tensor(x), [torch.tensor(w) for w in weights], 'concat', go_backwards=True, **seq)
    assert np.array_equal(t.numpy(), [[[5.0, 21.0], [7.0, 6.0]]])
    # GRU, z = 0 (bias -40), candidate linear: h_t = hh_t = x_t W_h, no memory: forward (2, 5), backward copy (3 * 5, 3 * 2) flipped: (6, 15)
    Wg = np.array([[0.0, 0.0, 1.0]])
    gw = [Wg, np.zeros((1, 3)), np.array([-40.0, 0.0, 0.0]), 3 * Wg, np.zeros((1, 3)), np.array([-40.0, 0.0, 0.0])]
    assert np.allclose(BR.forward('gru', x, gw, 'concat', **seq), [[[2.0, 6.0], [5.0, 15.0]]], rtol=0, atol=1e-15)
    assert np.allclose(BR.forward('gru', x, gw, 'mul', **seq), [[[12.0], [75.0]]], rtol=0, atol=1e-13)
