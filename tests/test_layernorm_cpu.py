"""tf.keras layers.LayerNormalization without a GPU: the fp64 definition tests/layernorm_ref.py against a plain loop and against torch autograd,
construction, shapes, the refusals by name, the config keys and the JSON round trip, the facade, the planner, the header's entry points, the
refusals of the C ABI (they come before any launch) and the geometry walk of csrc/layernorm_geom.h under the host sanitizers."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import layernorm_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [((1, 1), 1), ((2, 3), 1), ((3, 5, 4), 1), ((3, 5, 4), 2)]
IDS = ['1x1-last', '2x3-last', '3x5x4-last', '3x5x4-last-two']


# ---------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('scale,center', [(True, True), (False, True), (True, False), (False, False)])
@pytest.mark.parametrize('shape,naxes', SHAPES, ids=IDS)
def test_the_reference_is_the_plain_loop(shape, naxes, scale, center):
    rng = np.random.RandomState(sum(shape) + naxes)
    x = rng.randn(*shape) * 2 + 3
    gamma = rng.randn(*shape[len(shape) - naxes:]) if scale else None
    beta = rng.randn(*shape[len(shape) - naxes:]) if center else None
    y, mean, rstd, xhat = R.forward(x, gamma, beta, 1e-3, naxes)
    assert y.shape == x.shape and np.abs(y - R.forward_loops(x, gamma, beta, 1e-3, naxes)).max() <= 1e-13
    assert np.abs(xhat.mean(1)).max() <= 1e-14 and mean.shape == rstd.shape == (int(np.prod(shape[:len(shape) - naxes])),)


@pytest.mark.parametrize('scale,center', [(True, True), (False, True), (True, False), (False, False)])
@pytest.mark.parametrize('shape,naxes', SHAPES, ids=IDS)
def test_the_reference_gradients_are_torch_autograd(shape, naxes, scale, center):
    rng = np.random.RandomState(sum(shape) + naxes + 1)
    norm = shape[len(shape) - naxes:]
    x, dy = rng.randn(*shape) - 0.5, rng.randn(*shape)
    gamma, beta = (rng.randn(*norm) if scale else None), (rng.randn(*norm) if center else None)
    tx = torch.tensor(x, requires_grad=True)
    tg = torch.tensor(gamma, requires_grad=True) if scale else None
    tb = torch.tensor(beta, requires_grad=True) if center else None
    ty = torch.nn.functional.layer_norm(tx, norm, tg, tb, 1e-3)
    ty.backward(torch.tensor(dy))
    y, _, _, _ = R.forward(x, gamma, beta, 1e-3, naxes)
    g = R.backward(x, dy, gamma, 1e-3, naxes)
    assert np.abs(y - ty.detach().numpy()).max() <= 1e-12
    assert np.abs(g['dx'] - tx.grad.numpy()).max() <= 1e-12 * max(1.0, np.abs(g['dx']).max())
    if scale:
        assert g['dgamma'].shape == norm and np.abs(g['dgamma'] - tg.grad.numpy()).max() <= 1e-12 * max(1.0, np.abs(g['dgamma']).max())
    if center:
        assert g['dbeta'].shape == norm and np.abs(g['dbeta'] - tb.grad.numpy()).max() <= 1e-12 * max(1.0, np.abs(g['dbeta']).max())


def test_the_floors_scale_with_the_offset_of_a_row():
    rng = np.random.RandomState(3)
    x, dy, gamma = rng.randn(4, 16), rng.randn(4, 16), rng.randn(16)
    near, far = R.floors(x, dy, gamma, 1e-3), R.floors(x + 1000.0, dy, gamma, 1e-3)
    assert far['y'] > 100 * near['y'] and far['dx'] > 100 * near['dx'] and far['dgamma'] > 100 * near['dgamma'] and near['dbeta'] == far['dbeta'] == 0.0


# ---------------------------------------------------------------------------------------------------------------------
# the layer
# ---------------------------------------------------------------------------------------------------------------------
def test_facade_names_are_the_layer():
    import gennet_amd.keras
    from gennet_amd import keras, layernorm, layers
    import gennet_amd.keras.layers.normalization as mod
    assert keras.layers.LayerNormalization is keras.layers.normalization.LayerNormalization is mod.LayerNormalization is layers.LayerNormalization
    assert layers.LayerNormalization is layernorm.LayerNormalization
    assert 'LayerNormalization' in gennet_amd.keras.__doc__ and mod.BatchNormalization is layers.BatchNormalization


@pytest.mark.parametrize('shape,axis,want_axis,wshape', [((12,), -1, [1], (12,)), ((10, 12), -1, [2], (12,)), ((10, 12), 2, [2], (12,)),
                                                         ((10, 12), [-2, -1], [1, 2], (10, 12)), ((10, 12), (1, 2), [1, 2], (10, 12)),
                                                         ((2, 5, 8), [2, 3], [2, 3], (5, 8)), ((2, 5, 8), [1, -2, 3], [1, 2, 3], (2, 5, 8))])
def test_output_and_weight_shapes(shape, axis, want_axis, wshape):
    from gennet_amd import layers as Ly
    from gennet_amd.engine import Input
    for kw in ({}, {'scale': False}, {'center': False}, {'center': False, 'scale': False}):
        layer = Ly.LayerNormalization(axis=axis, **kw)
        out = layer(Input(shape))
        assert tuple(out.shape) == shape and layer.axis == want_axis and layer.N == int(np.prod(wshape))
        names = [n for n, on in (('gamma', kw.get('scale', True)), ('beta', kw.get('center', True))) if on]
        assert [p.name for p in layer.weights] == [layer.name + '/' + n for n in names]               # keras' order: gamma, then beta
        assert all(p.shape == wshape for p in layer.weights) and layer.count_params() == len(names) * int(np.prod(wshape))
        for p, w in zip(layer.weights, layer.get_weights()):
            assert np.array_equal(w, np.ones(wshape) if p.name.endswith('gamma') else np.zeros(wshape))
        assert not layer.non_trainable_weights and not layer.is_merge and not layer.writes_dy(None)
    assert Ly.LayerNormalization().name.startswith('layer_normalization_') and Ly.LayerNormalization().epsilon == 1e-3


def test_refusals_by_name():
    from gennet_amd import layers as Ly
    from gennet_amd.engine import Input
    x = Input((10, 12))
    for axis in (1, -2, [1], (-2,)):
        with pytest.raises(NotImplementedError, match=r'LayerNormalization\): axis .* only the trailing axes'):
            Ly.LayerNormalization(axis=axis)(x)
    with pytest.raises(NotImplementedError, match=r'my_norm \(LayerNormalization\): axis \(2, 1\)'):
        Ly.LayerNormalization(axis=[2, 1], name='my_norm')(x)                    # keras would lay gamma out as (12, 10): not ascending
    for axis in (0, -3, [0, 1, 2]):
        with pytest.raises(ValueError, match='batch axis'):
            Ly.LayerNormalization(axis=axis)(x)
    for axis in (3, -4):
        with pytest.raises(ValueError, match='Invalid axis: %d' % axis):
            Ly.LayerNormalization(axis=axis)(x)
    for axis in ([2, 2], [-1, 2]):
        with pytest.raises(ValueError, match='Duplicate axis'):
            Ly.LayerNormalization(axis=axis)(x)
    for axis in (1.0, 'last', [1, None], True, []):
        with pytest.raises(TypeError, match="int or a list/tuple of ints for the argument 'axis'"):
            Ly.LayerNormalization(axis=axis)
    with pytest.raises(ValueError, match='batch axis'):
        Ly.LayerNormalization(axis=0).compute_output_shape((10, 12))
    with pytest.raises(NotImplementedError, match='beta_initializer'):
        Ly.LayerNormalization(beta_initializer='ones')
    with pytest.raises(NotImplementedError, match='gamma_initializer'):
        Ly.LayerNormalization(gamma_initializer={'class_name': 'RandomNormal', 'config': {}})
    with pytest.raises(NotImplementedError, match='beta_constraint'):
        Ly.LayerNormalization(beta_constraint='non_neg')
    with pytest.raises(NotImplementedError, match='gamma_constraint'):
        Ly.LayerNormalization(gamma_constraint={'class_name': 'MaxNorm', 'config': {'max_value': 2, 'axis': 0}})
    with pytest.raises(ValueError, match='epsilon'):
        Ly.LayerNormalization(epsilon=-1.0)
    with pytest.raises(ValueError, match='takes a single tensor'):
        Ly.LayerNormalization()([x, x])
    Ly.LayerNormalization(beta_initializer={'class_name': 'Zeros', 'config': {}}, gamma_initializer='ones', dtype='float32', beta_constraint=None)


def layer_named(model, name):
    return [n.layer for n in model.nodes if n.layer.name == name][0]


def small_model(**kw):
    from gennet_amd import layers as Ly
    from gennet_amd.engine import Input, Model
    x = Input((10, 12), name='x')
    h = Ly.LayerNormalization(name='ln', **kw)(Ly.Dense(12, name='d0')(x))
    return Model(inputs=x, outputs=Ly.Dense(1, name='head')(Ly.GlobalAveragePooling1D(name='pool')(h)))


L2 = {'class_name': 'L1L2', 'config': {'l1': 0.0, 'l2': float(np.float32(0.01))}}


@pytest.mark.parametrize('kw,axis', [({}, [2]), ({'axis': [-2, -1]}, [1, 2]), ({'center': False}, [2]), ({'scale': False, 'epsilon': 1e-6}, [2]),
                                     ({'gamma_regularizer': 'l2', 'beta_regularizer': {'class_name': 'L1L2', 'config': {'l1': 0.5, 'l2': 0.0}}}, [2])],
                         ids=['plain', 'two-axes', 'no-center', 'no-scale', 'regularizers'])
def test_config_keys_and_json_round_trip(kw, axis):
    from gennet_amd.engine import model_from_json
    m = small_model(**kw)
    cfg = json.loads(m.to_json())
    entry = [l for l in cfg['config']['layers'] if l['class_name'] == 'LayerNormalization'][0]
    regs = {'gamma_regularizer': L2 if 'gamma_regularizer' in kw else None, 'beta_regularizer': kw.get('beta_regularizer')}
    assert entry['config'] == dict({'name': 'ln', 'trainable': True, 'axis': axis, 'epsilon': kw.get('epsilon', 1e-3), 'center': kw.get('center', True),
                                    'scale': kw.get('scale', True), 'beta_initializer': {'class_name': 'Zeros', 'config': {}},
                                    'gamma_initializer': {'class_name': 'Ones', 'config': {}}, 'beta_constraint': None, 'gamma_constraint': None}, **regs)
    assert layer_named(m, 'ln').get_config() == entry['config']
    again = model_from_json(m.to_json())
    a, b = layer_named(again, 'ln'), layer_named(m, 'ln')
    assert type(a).__name__ == 'LayerNormalization' and (a.axis, a.epsilon, a.center, a.scale) == (b.axis, b.epsilon, b.center, b.scale)
    assert [(p.name, p.shape) for p in a.weights] == [(p.name, p.shape) for p in b.weights]
    assert [p.regularizer for p in a.weights] == [p.regularizer for p in b.weights]
    assert [tuple(n.out_shape) for n in again.nodes] == [tuple(n.out_shape) for n in m.nodes]
    assert json.loads(again.to_json()) == cfg and m.count_params() == again.count_params()


@pytest.mark.parametrize('axis', [[2], -1, [1, 2]], ids=['list', 'int', 'two'])
def test_a_hand_written_keras_entry_loads(axis):
    """the entry tf.keras 2.x writes: dtype in the config, axis a list after build (an int where the model was never built)"""
    from gennet_amd.engine import model_from_json
    cfg = {'class_name': 'Model', 'keras_version': '2.2.4-tf', 'backend': 'tensorflow', 'config': {
        'name': 'model', 'input_layers': [['x', 0, 0]], 'output_layers': [['layer_normalization', 0, 0]],
        'layers': [{'name': 'x', 'class_name': 'InputLayer', 'inbound_nodes': [],
                    'config': {'batch_input_shape': [None, 7, 6], 'dtype': 'float32', 'sparse': False, 'name': 'x'}},
                   {'name': 'layer_normalization', 'class_name': 'LayerNormalization', 'inbound_nodes': [[['x', 0, 0, {}]]],
                    'config': {'name': 'layer_normalization', 'trainable': True, 'dtype': 'float32', 'axis': axis, 'epsilon': 0.001, 'center': True,
                               'scale': True, 'beta_initializer': {'class_name': 'Zeros', 'config': {}},
                               'gamma_initializer': {'class_name': 'Ones', 'config': {}}, 'beta_regularizer': None, 'gamma_regularizer': None,
                               'beta_constraint': None, 'gamma_constraint': None}}]}}
    m = model_from_json(json.dumps(cfg))
    ln = layer_named(m, 'layer_normalization')
    shape = (7, 6) if axis == [1, 2] else (6,)
    assert ln.axis == ([1, 2] if axis == [1, 2] else [2]) and tuple(m.nodes[0].out_shape) == (7, 6)
    assert [(p.name, p.shape) for p in ln.weights] == [('layer_normalization/gamma', shape), ('layer_normalization/beta', shape)]
    cfg['config']['layers'][1]['config']['gamma_constraint'] = {'class_name': 'NonNeg', 'config': {}}
    with pytest.raises(NotImplementedError, match='gamma_constraint'):
        model_from_json(json.dumps(cfg))


def test_the_planner_leaves_the_layer_alone():
    from gennet_amd import layers as Ly
    from gennet_amd.engine import Input, Model
    x = Input((6, 4))
    c = Ly.Conv1D(4, 3, padding='same')(x)
    ln = Ly.LayerNormalization()(c)
    drop = Ly.Dropout(0.1)(Ly.Activation('relu')(ln))
    m = Model(inputs=x, outputs=Ly.Dense(1)(Ly.Flatten()(drop)))
    m._plan()
    conv, node, act, dr = m.nodes[:4]
    assert type(node.layer).__name__ == 'LayerNormalization' and not getattr(node.layer, 'is_batchnorm', False)
    assert conv.fused_act is None and not node.absorbed and node.fused_act is None and node.fused_drop is None and not act.absorbed and not dr.absorbed
    assert all(n.fuse_prev < 0 for n in m.nodes[:4]) and not node.layer.fusable_act and not node.layer.fusable_drop


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI and the geometry
# ---------------------------------------------------------------------------------------------------------------------
def test_the_header_declares_the_entry_points():
    from gennet_amd import _lib, ops
    vp, sz, i32, f32 = _lib.vp, _lib.sz, _lib.i32, _lib.f32
    assert _lib.DECLS['gn_layernorm_fwd'] == (i32, [vp] * 6 + [sz, i32, f32, vp])                       # the 10 arguments ops.layernorm_fwd passes
    assert _lib.DECLS['gn_layernorm_bwd_workspace'] == (sz, [sz, i32])
    assert _lib.DECLS['gn_layernorm_bwd'] == (i32, [vp] * 9 + [sz, sz, i32, vp])                        # the 13 of ops.layernorm_bwd
    consts = (ops.LAYERNORM_ROWS_MAX_N, ops.LAYERNORM_BLOCK_MAX_N, ops.LAYERNORM_FWD_GRID_CAP, ops.LAYERNORM_BWD_GRID_CAP, ops.LAYERNORM_BWD_GRID_CAP_WIDE)
    assert consts == (1024, 4096, 2048, 1024, 512)
    with open(os.path.join(ROOT, 'gennet_amd', 'csrc', 'layernorm_geom.h')) as f:
        text = ' '.join(f.read().split())
    for name, value in zip(('LN_ROWS_MAX_N', 'LN_BLOCK_MAX_N', 'LN_FWD_GRID_CAP', 'LN_BWD_GRID_CAP', 'LN_BWD_GRID_CAP_WIDE'), consts):
        assert 'constexpr int %s = %d;' % (name, value) in text, name


def test_the_entry_points_refuse_before_any_launch():
    """every refusal of include/gennet_hip.h's layer normalisation block: the code, and gn_last_error names the argument.  The pointers are never
    dereferenced on the host, and a refused call launches nothing, so this runs without a device."""
    from gennet_amd import _lib
    L = _lib.lib()
    P = 4096                                        # a non-NULL pointer value
    fwd = dict(x=P, gamma=P, beta=P, y=P, mean=P, rstd=P, rows=3, N=5, eps=1e-3)
    bwd = dict(dy=P, x=P, gamma=P, mean=P, rstd=P, dx=P, dgamma=P, dbeta=P, ws=P, ws_bytes=1 << 20, rows=3, N=5)

    def run_fwd(**kw):
        g = dict(fwd, **kw)
        return int(L.gn_layernorm_fwd(g['x'], g['gamma'], g['beta'], g['y'], g['mean'], g['rstd'], g['rows'], g['N'], g['eps'], None))

    def run_bwd(**kw):
        g = dict(bwd, **kw)
        return int(L.gn_layernorm_bwd(g['dy'], g['x'], g['gamma'], g['mean'], g['rstd'], g['dx'], g['dgamma'], g['dbeta'], g['ws'], g['ws_bytes'], g['rows'],
                                      g['N'], None))

    def refused(rc, text, code=None):
        assert rc == (_lib.GN_EINVAL if code is None else code) and text in L.gn_last_error().decode(), (rc, L.gn_last_error())

    for name in ('x', 'y'):
        refused(run_fwd(**{name: None}), 'null pointer (x and y are required)')
    for name in ('dy', 'x', 'mean', 'rstd'):
        refused(run_bwd(**{name: None}), 'null pointer (dy, x, mean and rstd are required)')
    refused(run_bwd(ws=None), 'null pointer (the workspace is required')
    refused(run_bwd(ws=None, dgamma=None), 'null pointer (the workspace is required')
    refused(run_bwd(ws=None, dgamma=None, dbeta=None, N=4097), 'null pointer (the workspace is required')          # stream: the row statistics
    for run in (run_fwd, run_bwd):
        refused(run(rows=0), 'bad shape (rows 0, N 5)')
        refused(run(N=0), 'bad shape (rows 3, N 0)')
        refused(run(N=-4), 'bad shape (rows 3, N -4)')
        refused(run(rows=1 << 61, N=2), 'rows * N < 2^62')
        refused(run(rows=(1 << 64) - 1), 'rows * N < 2^62')                                                      # a negative count as size_t
    for eps in (-1e-3, float('nan'), float('inf'), float('-inf')):
        refused(run_fwd(eps=eps), 'eps %s is negative or not finite' % ('%g' % np.float32(eps)))
    refused(run_fwd(rstd=None), 'mean and rstd are given together')
    refused(run_fwd(mean=None), 'mean and rstd are given together')
    refused(run_bwd(gamma=None), 'dgamma without gamma')
    need = _lib.size('gn_layernorm_bwd_workspace', 3, 5)
    assert need == 4 * 2 * 1 * 5 and _lib.size('gn_layernorm_bwd_workspace', 0, 5) == 0 == _lib.size('gn_layernorm_bwd_workspace', 3, 0)
    refused(run_bwd(ws_bytes=need - 1), 'workspace too small (ws_bytes 39, gn_layernorm_bwd_workspace = 40)', _lib.GN_EWORKSPACE)
    refused(run_bwd(ws=P + 2), '4-byte aligned')
    # the workspace of the three regimes: one (2, N) float partial per block, and two floats a row where the row is streamed
    from gennet_amd import ops
    assert _lib.size('gn_layernorm_bwd_workspace', 10 ** 6, 64) == 4 * 2 * ops.LAYERNORM_BWD_GRID_CAP * 64
    assert _lib.size('gn_layernorm_bwd_workspace', 7, 4096) == 4 * 2 * 7 * 4096
    assert _lib.size('gn_layernorm_bwd_workspace', 10 ** 4, 4097) == 4 * (2 * 10 ** 4 + 2 * ops.LAYERNORM_BWD_GRID_CAP_WIDE * 4097)
    assert run_bwd(dx=None, dgamma=None, dbeta=None, ws=None) == _lib.GN_OK                                     # nothing asked for: no launch


def test_the_geometry_walk_is_clean_under_the_host_sanitizers(tmp_path):
    """tests/tools/layernorm_geom_walk.cpp includes csrc/layernorm_geom.h, the header the kernels' file includes, and plays the grids, the row
    ownership and the partial slots of the backward workspace around every seam: built with the host C++ compiler under the address and
    undefined-behaviour sanitizers and run as a program of its own."""
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    exe = os.path.join(str(tmp_path), 'layernorm_geom_walk')
    cmd = [cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-I', os.path.join(ROOT, 'gennet_amd', 'csrc'),
           os.path.join(ROOT, 'tests', 'tools', 'layernorm_geom_walk.cpp'), '-o', exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == 'walked 155 geometries' and lines[0].startswith('rows 1 N 1: regime 0, W 1, NJ 1, grids 1 / 1, workspace 8 bytes'), r.stdout
    assert any(l.startswith('rows 2049 N 8197: regime 2, W 64, NJ 33, grids 2048 / 512, workspace') for l in lines)
