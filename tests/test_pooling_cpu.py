"""CPU-only checks of the pooling layers: the numpy definition tests/pool_ref.py against torch fp64 autograd, hand-written tie cases,
output shapes, Keras configs, the constructor refusals, the facade names, the planner's view of the layers and the binding's declarations.
The kernels themselves are tested in tests/test_pooling_gpu.py against the same pool_ref."""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pool_ref as R

WINDOWED = ['MaxPooling1D', 'AveragePooling1D', 'MaxPooling2D', 'AveragePooling2D']
GLOBAL = ['GlobalAveragePooling1D', 'GlobalAveragePooling2D', 'GlobalMaxPooling1D', 'GlobalMaxPooling2D']

# B, H, W, C, pool, strides, padding
CASES = [(2, 9, 1, 3, (2, 1), (2, 1), 'valid'),        # 1-D, a dropped last row
         (2, 9, 1, 3, (3, 1), (2, 1), 'same'),         # overlap; total pad 2
         (2, 10, 1, 2, (3, 1), (2, 1), 'same'),        # total pad 1: the odd cell at the end
         (2, 11, 1, 2, (2, 1), (3, 1), 'valid'),       # gaps
         (2, 2, 1, 2, (3, 1), (3, 1), 'same'),         # H < pool
         (3, 7, 6, 4, (2, 2), (2, 2), 'valid'),
         (3, 7, 6, 4, (3, 2), (2, 1), 'same'),
         (2, 5, 4, 2, (5, 4), (5, 4), 'valid')]        # the pool is the whole extent


def tied_input(rng, shape):
    """exact ties: zeros from a 0.4-rate mask (a Dropout in front, as in test_maxpool_h2_bit_exact) and an all-zero sample"""
    x = rng.randn(*shape).astype(np.float32) * (rng.rand(*shape) >= 0.4)
    x[0] = 0.0
    return x.astype(np.float64)


def torch_pool(mode, x, pool, strides, padding):
    """(B, H, W, C) fp64 tensor -> pooled, by the recipe of the issue: -inf pads by TensorFlow's asymmetric rule and a valid max_pool2d; a
    sum-pool of x over a sum-pool of ones"""
    B, H, W, C = x.shape
    (Ho, pt), (Wo, pl) = R.pool_geometry(H, pool[0], strides[0], padding), R.pool_geometry(W, pool[1], strides[1], padding)
    pb, pr = max((Ho - 1) * strides[0] + pool[0] - H - pt, 0), max((Wo - 1) * strides[1] + pool[1] - W - pl, 0)
    xc = x.permute(0, 3, 1, 2)
    if mode == 'max':
        y = F.max_pool2d(F.pad(xc, (pl, pr, pt, pb), value=float('-inf')), pool, strides)
    else:
        def sum_pool(t):
            return F.avg_pool2d(F.pad(t, (pl, pr, pt, pb)), pool, strides) * (pool[0] * pool[1])
        y = sum_pool(xc) / sum_pool(torch.ones_like(xc))
    return y.permute(0, 2, 3, 1)


@pytest.mark.parametrize('mode', ['max', 'avg'])
@pytest.mark.parametrize('case', CASES, ids=[str(c) for c in CASES])
def test_windowed_reference_equals_torch_autograd(mode, case):
    B, H, W, C, pool, strides, padding = case
    rng = np.random.RandomState(H * 100 + W)
    x = tied_input(rng, (B, H, W, C))
    xt = torch.tensor(x, requires_grad=True)
    yt = torch_pool(mode, xt, pool, strides, padding)
    y = R.pool2d_fwd(mode, x, pool, strides, padding)
    assert y.shape == tuple(yt.shape) == R.out_shape(x.shape, pool, strides, padding)
    dy = rng.randn(*y.shape)
    yt.backward(torch.tensor(dy))
    dx = R.pool2d_bwd(mode, dy, x, pool, strides, padding)
    if mode == 'max':                  # comparisons, copies and sums of the same few terms
        assert np.array_equal(y, yt.detach().numpy())
        assert np.abs(dx - xt.grad.numpy()).max() <= 1e-15 * np.abs(dy).max() * R.covering_windows(x.shape, pool, strides, padding)
    else:
        assert np.abs(y - yt.detach().numpy()).max() <= 1e-15 * max(np.abs(x).max(), 1.0)
        assert np.abs(dx - xt.grad.numpy()).max() <= 1e-15 * np.abs(dy).max() * R.covering_windows(x.shape, pool, strides, padding)


@pytest.mark.parametrize('shape', [(2, 1, 1), (3, 5, 4), (2, 7, 3), (3, 40, 6)])
def test_global_reference_equals_torch_autograd(shape):
    rng = np.random.RandomState(sum(shape))
    x = tied_input(rng, shape)
    dy = rng.randn(shape[0], shape[2])
    for mode, fn in (('max', lambda t: t.amax(1)), ('avg', lambda t: t.mean(1))):
        xt = torch.tensor(x, requires_grad=True)
        yt = fn(xt)
        yt.backward(torch.tensor(dy))
        assert np.abs(R.global_fwd(mode, x) - yt.detach().numpy()).max() <= 1e-15
        assert np.abs(R.global_bwd(mode, dy, x) - xt.grad.numpy()).max() <= 1e-15 * np.abs(dy).max()


def test_the_two_tie_rules_by_hand():
    x = np.zeros((1, 4, 1, 1))
    dy = np.array([3.0, 5.0]).reshape(1, 2, 1, 1)
    assert R.pool2d_bwd('max', dy, x, (2, 1), (2, 1), 'valid').ravel().tolist() == [3.0, 0.0, 5.0, 0.0]         # MaxPooling1D(2): the first of each pair
    assert R.global_bwd('max', np.array([[8.0]]), x.reshape(1, 4, 1)).ravel().tolist() == [2.0, 2.0, 2.0, 2.0]   # GlobalMaxPooling1D: dy / 4 everywhere
    assert R.pool2d_bwd('avg', dy, x, (2, 1), (2, 1), 'valid').ravel().tolist() == [1.5, 1.5, 2.5, 2.5]
    # overlap adds: pool 3, stride 1 over [0, 1, 1, 0]: windows (0,1,1) -> index 1, (1,1,0) -> index 1
    x = np.array([0.0, 1.0, 1.0, 0.0]).reshape(1, 4, 1, 1)
    assert R.pool2d_bwd('max', dy, x, (3, 1), (1, 1), 'valid').ravel().tolist() == [0.0, 8.0, 0.0, 0.0]
    # 'same' with an odd total pad: 4 cells, pool 3, stride 2: windows [0, 2) ... no: total pad 1, floor half 0 in front: [0, 3) and [2, 4)
    assert R.pool2d_fwd('avg', np.array([1.0, 2.0, 3.0, 5.0]).reshape(1, 4, 1, 1), (3, 1), (2, 1), 'same').ravel().tolist() == [2.0, 4.0]


GEOMETRY = [(10, 2, 2, 'valid', 5, 0), (11, 2, 2, 'valid', 5, 0), (11, 3, 2, 'valid', 5, 0), (11, 2, 3, 'valid', 4, 0), (5, 5, 1, 'valid', 1, 0),
            (10, 2, 2, 'same', 5, 0), (11, 2, 2, 'same', 6, 0), (9, 3, 2, 'same', 5, 1), (10, 3, 2, 'same', 5, 0), (2, 3, 3, 'same', 1, 0),
            (1, 4, 2, 'same', 1, 1), (11, 2, 3, 'same', 4, 0), (7, 5, 1, 'same', 7, 2), (1, 1, 1, 'valid', 1, 0)]


@pytest.mark.parametrize('n,p,s,padding,n_out,pad', GEOMETRY)
def test_output_lengths_and_pads(n, p, s, padding, n_out, pad):
    from gennet_amd import layers as L, ops
    formula = (n - p) // s + 1 if padding == 'valid' else -(-n // s)
    total = 0 if padding == 'valid' else max((formula - 1) * s + p - n, 0)
    assert (n_out, pad) == (formula, total // 2)                                     # the table against the two formulas
    assert ops.pool_geometry(n, p, s, padding) == (n_out, pad) == R.pool_geometry(n, p, s, padding)
    for cls in (L.MaxPooling1D, L.AveragePooling1D):
        assert cls(p, s, padding).compute_output_shape((n, 3)) == (n_out, 3)
    for cls in (L.MaxPooling2D, L.AveragePooling2D):
        assert cls((p, 1), (s, 1), padding).compute_output_shape((n, 4, 3)) == (n_out, 4, 3)
        assert cls((1, p), (1, s), padding).compute_output_shape((4, n, 3)) == (4, n_out, 3)


def test_a_valid_pool_larger_than_its_input_and_wrong_ranks_are_value_errors():
    from gennet_amd import layers as L, ops
    with pytest.raises(ValueError):
        ops.pool_geometry(2, 3, 1, 'valid')
    for make, shape in ((lambda: L.MaxPooling1D(3), (2, 4)), (lambda: L.AveragePooling1D(5, 1), (4, 4)), (lambda: L.MaxPooling2D((2, 1)), (1, 2, 4)),
                        (lambda: L.MaxPooling2D((2, 3)), (4, 2, 4)), (lambda: L.AveragePooling2D(3), (2, 5, 1))):
        with pytest.raises(ValueError):
            make().compute_output_shape(shape)
    assert L.MaxPooling1D(3, padding='same').compute_output_shape((2, 4)) == (1, 4)      # n < p under 'same': one clipped window
    for cls, shape in ((L.MaxPooling1D, (4, 2, 3)), (L.AveragePooling1D, (4,)), (L.MaxPooling2D, (4, 3)), (L.AveragePooling2D, (4, 3)),
                       (L.GlobalAveragePooling1D, (4, 2, 3)), (L.GlobalMaxPooling1D, (3,)), (L.GlobalAveragePooling2D, (4, 3)),
                       (L.GlobalMaxPooling2D, (4, 3))):
        with pytest.raises(ValueError):
            cls().compute_output_shape(shape)
    assert L.GlobalAveragePooling1D().compute_output_shape((7, 3)) == (3,) and L.GlobalMaxPooling2D().compute_output_shape((7, 2, 5)) == (5,)


def test_constructor_refusals():
    from gennet_amd import layers as L
    for name in WINDOWED + GLOBAL:
        with pytest.raises(NotImplementedError):
            getattr(L, name)(data_format='channels_first')
        getattr(L, name)(data_format='channels_last')
    for name in WINDOWED:
        cls = getattr(L, name)
        for kw in ({'pool_size': 0}, {'pool_size': (2, 2, 2)}, {'strides': 0}, {'strides': (1, 2, 3)}, {'padding': 'full'}, {'pool_size': -1}):
            with pytest.raises(ValueError):
                cls(**kw)
    assert L.MaxPooling1D().pool_size == (2,) == L.MaxPooling1D().strides and L.AveragePooling1D(3).strides == (3,)
    assert L.MaxPooling2D().pool_size == (2, 2) == L.AveragePooling2D().strides and L.MaxPooling2D(3, 1).strides == (1, 1)


def test_config_round_trips_for_all_eight_classes():
    from gennet_amd import keras_io, layers as L
    made = [L.MaxPooling1D(3, 2, 'same'), L.AveragePooling1D(), L.MaxPooling2D((2, 1)), L.MaxPooling2D((3, 2), (2, 1), 'same'), L.AveragePooling2D(2, (1, 2))] \
        + [getattr(L, n)() for n in GLOBAL]
    for layer in made:
        name = type(layer).__name__
        cfg = keras_io.layer_config(layer)
        if name in WINDOWED:
            rank = 1 if name.endswith('1D') else 2
            assert set(cfg) == {'name', 'trainable', 'pool_size', 'strides', 'padding', 'data_format'}, cfg
            assert cfg['pool_size'] == list(layer.pool_size) and cfg['strides'] == list(layer.strides) and len(cfg['pool_size']) == len(cfg['strides']) == rank
            assert cfg['padding'] == layer.padding
        else:
            assert set(cfg) == {'name', 'trainable', 'data_format'}, cfg
        assert cfg['data_format'] == 'channels_last' and layer.get_config() == cfg
        back = keras_io._layer_from_config(name, json.loads(json.dumps(cfg)), None)
        assert type(back) is type(layer) and back.name == layer.name and keras_io.layer_config(back) == cfg
        with pytest.raises(NotImplementedError):
            keras_io._layer_from_config(name, dict(cfg, data_format='channels_first'), None)
    assert keras_io.layer_config(L.MaxPooling2D((2, 1)))['pool_size'] == [2, 1]


# typed in the form keras 2.2.4 writes (to_json of a Sequential); the first 1-D layer without data_format, as older keras wrote it
KERAS_JSON = '''{"class_name": "Sequential", "config": {"name": "sequential_1", "layers": [
 {"class_name": "Reshape", "config": {"name": "reshape_1", "trainable": true, "batch_input_shape": [null, 24], "dtype": "float32", "target_shape": [24, 1]}},
 {"class_name": "MaxPooling1D", "config": {"name": "max_pooling1d_1", "trainable": true, "strides": [2], "pool_size": [2], "padding": "valid"}},
 {"class_name": "AveragePooling1D", "config": {"name": "average_pooling1d_1", "trainable": true, "strides": [2], "pool_size": [3], "padding": "same",
  "data_format": "channels_last"}},
 {"class_name": "Reshape", "config": {"name": "reshape_2", "trainable": true, "target_shape": [3, 2, 1]}},
 {"class_name": "MaxPooling2D", "config": {"name": "max_pooling2d_1", "trainable": true, "pool_size": [2, 2], "padding": "same", "strides": [1, 1],
  "data_format": "channels_last"}},
 {"class_name": "AveragePooling2D", "config": {"name": "average_pooling2d_1", "trainable": true, "pool_size": [2, 1], "padding": "valid", "strides": [1, 1],
  "data_format": "channels_last"}},
 {"class_name": "%s", "config": {"name": "global_1", "trainable": true%s}}]}, "keras_version": "2.2.4", "backend": "tensorflow"}'''


@pytest.mark.parametrize('name', ['GlobalAveragePooling2D', 'GlobalMaxPooling2D'])
@pytest.mark.parametrize('data_format', ['', ', "data_format": "channels_last"'])
def test_a_keras_json_builds_with_and_without_data_format(name, data_format):
    from gennet_amd import layers as L
    from gennet_amd.keras.models import model_from_json
    m = model_from_json(KERAS_JSON % (name, data_format))
    kinds = [type(l).__name__ for l in m.layers]
    assert kinds == ['Reshape', 'MaxPooling1D', 'AveragePooling1D', 'Reshape', 'MaxPooling2D', 'AveragePooling2D', name]
    assert all(type(l) is getattr(L, k) for l, k in zip(m.layers, kinds))
    assert [n.out_shape for n in m.nodes] == [(24, 1), (12, 1), (6, 1), (3, 2, 1), (3, 2, 1), (2, 2, 1), (1,)]
    assert m.layers[2].pool_size == (3,) and m.layers[2].padding == 'same' and m.layers[4].strides == (1, 1)
    assert m.output_shape == (None, 1)
    with pytest.raises(NotImplementedError):
        model_from_json(KERAS_JSON % (name, ', "data_format": "channels_first"'))


def test_the_facade_resolves_the_new_names_and_keeps_the_three_import_placeholders():
    import importlib
    from gennet_amd import layers as L
    top = importlib.import_module('gennet_amd.keras.layers')
    for n in ('AveragePooling2D', 'GlobalAveragePooling2D', 'GlobalMaxPooling1D', 'GlobalMaxPooling2D', 'MaxPooling2D'):
        assert getattr(top, n) is getattr(L, n), n
    pooling = importlib.import_module('gennet_amd.keras.layers.pooling')
    for n in WINDOWED + GLOBAL:
        assert getattr(pooling, n) is getattr(L, n), n
    from gennet_amd.keras.layers.pooling import MaxPooling1D, GlobalAveragePooling1D
    assert MaxPooling1D(2).pool_size == (2,) and GlobalAveragePooling1D().compute_output_shape((5, 3)) == (3,)
    conv = importlib.import_module('gennet_amd.keras.layers.convolutional')
    for mod, n in ((conv, 'MaxPooling1D'), (conv, 'AveragePooling1D'), (top, 'GlobalAveragePooling1D')):
        with pytest.raises(NotImplementedError) as e:
            getattr(mod, n)()
        assert 'gennet_amd.layers.%s' % n in str(e.value) and 'load_model' in str(e.value)


def test_the_planner_sees_ordinary_layers_and_pool_2_1_keeps_its_own_kernels():
    from gennet_amd import layers as L
    from gennet_amd.engine import Sequential
    ls = [L.Reshape((32, 2, 1), input_shape=(64,)), L.Conv2D(4, (5, 5), strides=(1, 1), padding='same'), L.LeakyReLU(0.2), L.Dropout(0.4), L.MaxPooling2D((2, 1)),
          L.Conv2D(4, (5, 5), strides=(1, 1), padding='same', activation='tanh'), L.MaxPooling2D((2, 2)), L.AveragePooling2D((2, 1), padding='same'),
          L.Reshape((-1, 4)), L.MaxPooling1D(2), L.AveragePooling1D(3, 2, 'same'), L.GlobalMaxPooling1D(), L.Dense(1, activation='sigmoid')]
    m = Sequential(ls)
    m._plan()
    pools = [n for n in m.nodes if isinstance(n.layer, (L._Pooling, L._GlobalPooling))]
    assert len(pools) == 6
    for n in pools:
        assert not n.absorbed and n.fused_act is None and n.fused_drop is None and n.fuse_prev == -1 and n.fold_up is None and n.infer_bn is None and n.lazy_bn == -1
        assert not n.layer.fusable_act and not n.layer.fusable_drop and n.layer.act_spec is None and n.layer.drop_rate is None
        assert not getattr(n.layer, 'shape_only', False) and not getattr(n.layer, 'offers_act_bwd', False)
    assert [n.layer.h2 for n in pools[:5]] == [True, False, False, False, False]
    assert m.nodes[1].fused_act == ('leaky', L.LeakyReLU(0.2).alpha) and m.nodes[1].fused_drop[0] == 0.4          # the conv in front still takes both
    assert m.nodes[-1].fuse_prev == -1                                                                             # no backward fusion through a pooling layer
    assert [n.out_shape for n in pools] == [(16, 2, 4), (8, 1, 4), (4, 1, 4), (2, 4), (1, 4), (4,)]
    assert L.MaxPooling2D((2, 1), (2, 1)).h2 and L.MaxPooling2D([2, 1]).h2
    assert not any(l.h2 for l in (L.MaxPooling2D((2, 1), padding='same'), L.MaxPooling2D((2, 1), (1, 1)), L.AveragePooling2D((2, 1)), L.MaxPooling1D(2)))


def test_binding_declares_the_entry_points():
    from gennet_amd import _lib, ops
    from gennet_amd._lib import i32, sz, vp
    geo = [i32] * 12
    assert _lib.DECLS['gn_pool2d_fwd'] == (i32, [i32, vp, vp] + geo + [vp]) and len(_lib.DECLS['gn_pool2d_fwd'][1]) == 16
    assert _lib.DECLS['gn_pool2d_bwd'] == (i32, [i32, vp, vp, vp] + geo + [vp]) and len(_lib.DECLS['gn_pool2d_bwd'][1]) == 17
    assert _lib.DECLS['gn_global_pool_workspace'] == (sz, [i32, i32, i32])
    assert _lib.DECLS['gn_global_pool_fwd'] == (i32, [i32, vp, vp, vp, sz, i32, i32, i32, vp])
    assert _lib.DECLS['gn_global_pool_bwd'] == (i32, [i32, vp, vp, vp, vp, vp, sz, i32, i32, i32, vp])
    assert ops.POOL_MODES == {'max': 0, 'avg': 1}
    assert _lib.CONSTS['GN_POOL_MAX'] == 0 and _lib.CONSTS['GN_POOL_AVG'] == 1
