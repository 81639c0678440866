"""tf.keras layers.Attention without a GPU: the fp64 definition tests/attention_ref.py against a plain triple loop and against torch autograd,
construction, the refusals by name, shape inference, the config keys and the JSON round trip, the facade, the header's entry points and the
geometry walk of csrc/attention_geom.h under the host sanitizers."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import attention_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('causal', [False, True])
@pytest.mark.parametrize('shape', [(1, 1, 1, 1, 1), (2, 3, 5, 2, 3), (1, 5, 3, 4, 2), (2, 4, 4, 3, 3)], ids=lambda s: 'x'.join(map(str, s)))
def test_the_reference_is_the_triple_loop(shape, causal):
    B, Tq, Tk, d, dv = shape
    rng = np.random.RandomState(sum(shape))
    q, k, v = rng.randn(B, Tq, d), rng.randn(B, Tk, d), rng.randn(B, Tk, dv)
    out, lse, p = R.forward(q, k, v, 0.7, causal)
    assert np.abs(out - R.forward_loops(q, k, v, 0.7, causal)).max() <= 1e-13
    assert np.abs(p.sum(-1) - 1).max() <= 1e-14
    if causal:
        assert all(p[:, i, j] .max() == 0 for i in range(Tq) for j in range(Tk) if j > i)


@pytest.mark.parametrize('causal', [False, True])
@pytest.mark.parametrize('shape', [(2, 3, 5, 2, 3), (1, 5, 3, 4, 2), (3, 6, 6, 4, 4)], ids=lambda s: 'x'.join(map(str, s)))
def test_the_reference_gradients_are_torch_autograd(shape, causal):
    B, Tq, Tk, d, dv = shape
    rng = np.random.RandomState(sum(shape) + 1)
    q, k, v, dout = rng.randn(B, Tq, d), rng.randn(B, Tk, d), rng.randn(B, Tk, dv), rng.randn(B, Tq, dv)
    tq, tk, tv = (torch.tensor(t, requires_grad=True) for t in (q, k, v))
    ts = torch.tensor(0.6, dtype=torch.float64, requires_grad=True)
    s = ts * torch.matmul(tq, tk.transpose(1, 2))
    if causal:
        s = s.masked_fill(~torch.tensor(R.mask(Tq, Tk, True)), float('-inf'))
    out = torch.matmul(torch.softmax(s, -1), tv)
    out.backward(torch.tensor(dout))
    g = R.backward(q, k, v, dout, 0.6, causal)
    o, lse, _ = R.forward(q, k, v, 0.6, causal)
    assert np.abs(o - out.detach().numpy()).max() <= 1e-12
    assert np.abs(lse - torch.logsumexp(s, -1).detach().numpy()).max() <= 1e-12
    for name, t in (('dq', tq), ('dk', tk), ('dv', tv)):
        assert np.abs(g[name] - t.grad.numpy()).max() <= 1e-12 * max(1.0, np.abs(g[name]).max()), name
    assert abs(g['dscale'] - float(ts.grad)) <= 1e-12 * max(1.0, abs(g['dscale']))
    assert g['dscale_rows'].shape == (B * Tq,) and abs(g['dscale_rows'].sum() - g['dscale']) <= 1e-12 * max(1.0, abs(g['dscale']))


# ---------------------------------------------------------------------------------------------------------------------
# the layer
# ---------------------------------------------------------------------------------------------------------------------
def test_facade_names_are_the_layer():
    import gennet_amd.keras
    from gennet_amd import attention, keras, layers
    import gennet_amd.keras.layers.dense_attention as mod
    assert keras.layers.Attention is keras.layers.dense_attention.Attention is mod.Attention is layers.Attention is attention.Attention
    assert 'Attention' in gennet_amd.keras.__doc__


SHAPES = [([(6, 4), (5, 4)], (6, 4)),                          # [query, value]: key is value
          ([(6, 4), (5, 7), (5, 4)], (6, 7)),                  # Tq != Tk, dv != d
          ([(1, 128), (9, 128), (9, 128)], (1, 128)),
          ([(3, 6, 4), (3, 5, 7), (3, 5, 4)], (3, 6, 7)),      # rank 4: heads
          ([(2, 3, 6, 4), (2, 3, 6, 4)], (2, 3, 6, 4))]


@pytest.mark.parametrize('shapes,want', SHAPES)
def test_output_shapes(shapes, want):
    from gennet_amd import layers as Ly
    from gennet_amd.engine import Input
    for kw in ({}, {'use_scale': True, 'causal': True}):
        layer = Ly.Attention(**kw)
        out = layer([Input(s) for s in shapes])
        assert tuple(out.shape) == want
        assert [p.name for p in layer.weights] == ([layer.name + '/scale'] if kw else [])
        if kw:
            assert layer.weights[0].shape == () and layer.get_weights()[0] == np.float32(1.0) and layer.count_params() == 1
    assert Ly.Attention().is_merge and not Ly.Attention().writes_dy(None)


def test_refusals_by_name():
    from gennet_amd import layers as Ly
    from gennet_amd.engine import Input
    q, v, k = Input((6, 4)), Input((5, 7)), Input((5, 4))
    with pytest.raises(NotImplementedError, match='dropout'):
        Ly.Attention(dropout=0.1)
    Ly.Attention(dropout=0.0, dtype='float32')
    with pytest.raises(NotImplementedError, match='mask='):
        Ly.Attention()([q, v, k], mask=[None, None])
    with pytest.raises(ValueError, match='must be called on a list of inputs, namely'):
        Ly.Attention()(q)
    for bad in ([q], [q, v, k, k]):
        with pytest.raises(ValueError, match='accepts inputs list of length 2 or 3, namely .* Given length: %d' % len(bad)):
            Ly.Attention()(bad)
    with pytest.raises(ValueError, match='length 2 or 3'):
        Ly.Attention().compute_output_shape([(6, 4)] * 4)
    with pytest.raises(ValueError, match='Dimensions must be equal, but are 4 and 7'):
        Ly.Attention()([q, v])                                  # key = value has another d
    with pytest.raises(ValueError, match='Dimensions must be equal, but are 4 and 5'):
        Ly.Attention()([q, v, Input((5, 5))])
    with pytest.raises(ValueError, match='same number of positions Tk'):
        Ly.Attention()([q, v, Input((6, 4))])
    with pytest.raises(ValueError, match='axes between the batch and the last two must agree'):
        Ly.Attention()([Input((2, 6, 4)), Input((3, 5, 4))])
    with pytest.raises(ValueError, match='one rank, 3 or more'):
        Ly.Attention()([Input((2, 6, 4)), Input((5, 4))])
    with pytest.raises(ValueError, match='one rank, 3 or more'):
        Ly.Attention()([Input((4,)), Input((4,))])
    with pytest.raises(NotImplementedError, match='d = 129, dv = 8'):
        Ly.Attention()([Input((6, 129)), Input((5, 8)), Input((5, 129))])
    with pytest.raises(NotImplementedError, match='d = 8, dv = 130'):
        Ly.Attention()([Input((6, 8)), Input((5, 130)), Input((5, 8))])
    with pytest.raises(ValueError, match='takes a single tensor'):
        Ly.Dense(3)([q, k])


def layer_named(model, name):
    return [n.layer for n in model.nodes if n.layer.name == name][0]


def three_input_model(**kw):
    from gennet_amd import layers as Ly
    from gennet_amd.engine import Input, Model
    x = Input((10, 8), name='x')
    q, k, v = Ly.Conv1D(8, 1, name='cq')(x), Ly.Conv1D(8, 1, name='ck')(x), Ly.Conv1D(6, 1, name='cv')(x)
    ctx = Ly.Attention(name='att', **kw)([q, v, k])
    return Model(inputs=x, outputs=Ly.Dense(1, name='head')(Ly.GlobalAveragePooling1D(name='pool')(ctx)))


@pytest.mark.parametrize('kw', [{}, {'use_scale': True}, {'causal': True}, {'use_scale': True, 'causal': True}], ids=['plain', 'scale', 'causal', 'both'])
def test_config_keys_and_json_round_trip(kw):
    from gennet_amd.engine import model_from_json
    m = three_input_model(**kw)
    cfg = json.loads(m.to_json())
    entry = [l for l in cfg['config']['layers'] if l['class_name'] == 'Attention'][0]
    assert entry['config'] == {'name': 'att', 'trainable': True, 'use_scale': kw.get('use_scale', False), 'causal': kw.get('causal', False), 'dropout': 0.0}
    assert [r[0] for r in entry['inbound_nodes'][0]] == ['cq', 'cv', 'ck']            # [query, value, key], in call order
    assert layer_named(m, 'att').get_config() == entry['config']
    again = model_from_json(m.to_json())
    a = layer_named(again, 'att')
    assert type(a).__name__ == 'Attention' and a.use_scale is kw.get('use_scale', False) and a.causal is kw.get('causal', False)
    assert [n.inbound for n in again.nodes] == [n.inbound for n in m.nodes]
    assert [tuple(n.out_shape) for n in again.nodes] == [tuple(n.out_shape) for n in m.nodes]
    assert [p.name for p in a.weights] == (['att/scale'] if kw.get('use_scale') else [])
    assert json.loads(again.to_json()) == cfg
    assert m.count_params() == again.count_params() == 2 * 72 + 54 + 7 + (1 if kw.get('use_scale') else 0)


def test_a_hand_written_keras_entry_loads():
    """the entry tf.keras 2.x writes: dtype in the config, three inbound tensors, dropout 0.0"""
    from gennet_amd.engine import model_from_json
    inp = lambda name, shape: {'name': name, 'class_name': 'InputLayer', 'inbound_nodes': [],          # noqa: E731
                               'config': {'batch_input_shape': [None] + shape, 'dtype': 'float32', 'sparse': False, 'name': name}}
    cfg = {'class_name': 'Model', 'keras_version': '2.2.4-tf', 'backend': 'tensorflow', 'config': {
        'name': 'model', 'input_layers': [['q', 0, 0], ['v', 0, 0], ['k', 0, 0]], 'output_layers': [['attention', 0, 0]],
        'layers': [inp('q', [4, 6, 8]), inp('v', [4, 9, 5]), inp('k', [4, 9, 8]),
                   {'name': 'attention', 'class_name': 'Attention', 'config': {'name': 'attention', 'trainable': True, 'dtype': 'float32', 'causal': True,
                                                                                'dropout': 0.0, 'use_scale': True},
                    'inbound_nodes': [[['q', 0, 0, {}], ['v', 0, 0, {}], ['k', 0, 0, {}]]]}]}}
    m = model_from_json(json.dumps(cfg))
    a = layer_named(m, 'attention')
    assert a.use_scale and a.causal and m.nodes[0].inbound == [-1, -2, -3] and tuple(m.nodes[0].out_shape) == (4, 6, 5)
    assert [p.name for p in a.weights] == ['attention/scale']
    cfg['config']['layers'][3]['config']['dropout'] = 0.25
    with pytest.raises(NotImplementedError, match='dropout'):
        model_from_json(json.dumps(cfg))


def test_the_planner_leaves_the_layer_alone():
    from gennet_amd import layers as Ly
    from gennet_amd.engine import Input, Model
    x = Input((6, 4))
    c = Ly.Conv1D(4, 3, padding='same')(x)
    act = Ly.Activation('tanh')(c)
    att = Ly.Attention()([act, act])
    drop = Ly.Dropout(0.1)(Ly.Activation('relu')(att))
    m = Model(inputs=x, outputs=Ly.Dense(1)(Ly.Flatten()(drop)))
    m._plan()
    conv, a0, node, a1, dr = m.nodes[:5]
    assert conv.fused_act == ('tanh', 0.0) and a0.absorbed and node.inbound == [1, 1]
    assert not node.absorbed and node.fused_act is None and node.fused_drop is None and not a1.absorbed and not dr.absorbed
    assert all(n.fuse_prev < 0 for n in m.nodes[:5]) and not node.layer.fusable_act and not node.layer.fusable_drop


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI and the geometry
# ---------------------------------------------------------------------------------------------------------------------
def test_the_header_declares_the_entry_points():
    from gennet_amd import _lib, ops
    vp, sz, i32 = _lib.vp, _lib.sz, _lib.i32
    assert _lib.DECLS['gn_attention_workspace'] == (sz, [i32, i32])
    assert _lib.DECLS['gn_attention_fwd'] == (i32, [vp] * 6 + [i32] * 6 + [vp])                       # the 13 arguments ops.attention_fwd passes
    assert _lib.DECLS['gn_attention_bwd'] == (i32, [vp] * 12 + [sz] + [i32] * 6 + [vp])               # the 20 of ops.attention_bwd
    assert (ops.ATTENTION_BQ, ops.ATTENTION_BK, ops.ATTENTION_MAX_D) == (128, 64, 128)
    with open(os.path.join(ROOT, 'gennet_amd', 'csrc', 'attention_geom.h')) as f:
        text = f.read()
    for name, value in (('ATTN_BQ', ops.ATTENTION_BQ), ('ATTN_BK', ops.ATTENTION_BK), ('ATTN_MAX_D', ops.ATTENTION_MAX_D)):
        assert 'constexpr int %s = %d;' % (name, value) in text, name


def test_the_geometry_walk_is_clean_under_the_host_sanitizers(tmp_path):
    """tests/tools/attention_geom_walk.cpp includes csrc/attention_geom.h, the header the kernels' file includes, and forms every LDS index of the three
    kernels for every column-tile count inside buffers of the launched sizes: built with the host C++ compiler under the address and
    undefined-behaviour sanitizers and run as a program of its own."""
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    exe = os.path.join(str(tmp_path), 'attention_geom_walk')
    cmd = [cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-I', os.path.join(ROOT, 'gennet_amd', 'csrc'),
           os.path.join(ROOT, 'tests', 'tools', 'attention_geom_walk.cpp'), '-o', exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == 'walked 4 geometries' and lines[3].startswith('DT 4: LDS bytes forward 67072, dq 66560, dkv 67072'), r.stdout
