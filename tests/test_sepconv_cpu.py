"""keras layers.SeparableConv1D without a GPU: the fp64 definition tests/sepconv_ref.py against torch (F.pad + F.conv1d(groups=C) + a 1 x 1 conv)
and torch autograd, the layer's host side -- refusals, weights, regularizers, shapes, config and JSON, its module, the facade, the header --, and
the launch geometry of csrc/depthwise.hip walked under the host sanitizers over the GPU test's shape list."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import sepconv_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rel(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-300)


# (B, L, C, k, stride, dilation, dm, padding): even windows, strides 2 and 3, dilation 2, dm 1 and 3: the asymmetric 'same' pad and the c dm + m order
CASES = [(2, 9, 3, 4, 1, 1, 1, 'same'), (2, 10, 2, 4, 2, 1, 3, 'same'), (3, 11, 4, 3, 3, 1, 3, 'same'), (2, 12, 3, 2, 1, 2, 1, 'same'),
         (2, 13, 2, 3, 1, 2, 3, 'valid'), (1, 8, 5, 6, 2, 1, 1, 'valid'), (2, 3, 2, 8, 1, 1, 3, 'same'), (2, 7, 3, 5, 3, 1, 1, 'valid')]
CASE_IDS = ['b%d-l%d-c%d-k%d-s%d-d%d-m%d-%s' % c for c in CASES]


def test_the_same_rule_is_asymmetric_where_tf_is():
    assert R.geometry(9, 4, 1, 'same') == (9, 1, 2) and R.geometry(10, 4, 2, 'same') == (5, 1, 1) and R.geometry(11, 3, 3, 'same') == (4, 0, 1)
    assert R.geometry(12, 2, 1, 'same', 2) == (12, 1, 1) and R.geometry(7, 40, 1, 'same') == (7, 19, 20) and R.geometry(10, 1, 3, 'same') == (4, 0, 0)
    from gennet_amd import ops
    for B, L, C, k, s, d, dm, padding in CASES + R.SHAPES:
        assert ops.conv_geometry(L, k, s, padding, d) == R.geometry(L, k, s, padding, d)[:2]


@pytest.mark.parametrize('case', CASES, ids=CASE_IDS)
def test_the_reference_is_torch_in_fp64_forward_and_in_its_three_gradients(case):
    B, L, C, k, s, d, dm, padding = case
    rng = np.random.RandomState(3)
    F_ = 4
    x, w, p, b = rng.randn(B, L, C), rng.randn(k, C, dm), rng.randn(1, C * dm, F_), rng.randn(F_)
    xt, wt, pt, bt = (torch.tensor(a, requires_grad=True) for a in (x, w, p, b))
    # the depthwise half alone: a pointwise identity and no bias
    eye = torch.eye(C * dm, dtype=torch.float64)[None]
    t = R.torch_forward(xt, wt, eye, torch.zeros(C * dm, dtype=torch.float64), s, padding, d)
    t_ref = R.dw_fwd(x, w, s, padding, d)
    assert t_ref.shape == (B, R.geometry(L, k, s, padding, d)[0], C * dm) and rel(t_ref, t.detach().numpy()) < 1e-13
    dt = rng.randn(*t_ref.shape)
    t.backward(torch.tensor(dt))
    assert rel(R.dw_dgrad(dt, w, L, s, padding, d), xt.grad.numpy()) < 1e-13
    assert rel(R.dw_wgrad(x, dt, k, s, padding, d), wt.grad.numpy()) < 1e-13
    assert R.dgrad_terms(L, k, s, padding, d, dm) <= k * dm
    # the layer
    for act in ('linear', 'relu', 'tanh', 'sigmoid', 'softmax'):
        y = R.torch_forward(xt, wt, pt, bt, s, padding, d, act)
        assert rel(R.layer(x, w, p, b, s, padding, d, act), y.detach().numpy()) < 1e-13
    # the fp32 restatement is the same definition
    assert rel(R.dw_fwd(x, w, s, padding, d, np.float32), t_ref) < 1e-5


def test_the_channel_order_is_c_dm_plus_m():
    x = np.zeros((1, 3, 2))
    x[0, :, 1] = 1.0
    w = np.arange(1, 7, dtype=np.float64).reshape(1, 2, 3)                # w[0, c, m] = 1 + 3 c + m
    assert R.dw_fwd(x, w)[0, 0].tolist() == [0, 0, 0, 4, 5, 6]


# ---------------------------------------------------------------------------------------------------------------------
# the layer's host side
# ---------------------------------------------------------------------------------------------------------------------
GLOROT_DICT = {'class_name': 'VarianceScaling', 'config': {'scale': 1.0, 'mode': 'fan_avg', 'distribution': 'uniform', 'seed': None}}


def test_what_is_not_run_is_refused_by_name():
    from gennet_amd.layers import SeparableConv1D as S
    for kw, text in ((dict(use_bias=False), 'use_bias=False'), (dict(data_format='channels_first'), 'data_format'),
                     (dict(depthwise_constraint='max_norm'), 'depthwise_constraint'), (dict(pointwise_constraint={'class_name': 'NonNeg'}), 'pointwise_constraint'),
                     (dict(bias_constraint='non_neg'), 'bias_constraint'), (dict(depthwise_initializer='he_normal'), 'depthwise_initializer'),
                     (dict(pointwise_initializer={'class_name': 'VarianceScaling', 'config': {'mode': 'fan_in', 'distribution': 'normal'}}),
                      'pointwise_initializer'),
                     (dict(bias_initializer='ones'), 'bias_initializer'), (dict(padding='causal'), 'causal'), (dict(activation='elu'), 'activation')):
        with pytest.raises(NotImplementedError, match=text):
            S(4, 3, **kw)
    for kw, text in ((dict(depth_multiplier=0), 'depth_multiplier'), (dict(strides=2, dilation_rate=2), 'exclude each other'),
                     (dict(padding='full'), 'padding'), (dict(dilation_rate=(1, 2)), 'dilation_rate')):
        with pytest.raises(ValueError, match=text):
            S(4, 3, **kw)
    with pytest.raises(ValueError, match=r'expects \(batch, steps, channels\)'):
        S(4, 3)._ensure_built((5, 6, 7))
    with pytest.raises(ValueError, match='rows'):
        S(4, 5, dilation_rate=2)._ensure_built((8, 3))
    with pytest.raises(ValueError, match='rows'):
        S(4, 9).compute_output_shape((8, 3))


def test_the_accepted_spellings():
    from gennet_amd.layers import SeparableConv1D as S
    import gennet_amd.keras  # noqa: F401
    from gennet_amd.keras.activations import relu
    l = S(4, (3,), strides=[2], dilation_rate=(1,), data_format='channels_last', depthwise_initializer=GLOROT_DICT,
          pointwise_initializer={'class_name': 'GlorotUniform', 'config': {'seed': None}}, bias_initializer={'class_name': 'Zeros', 'config': {}},
          activation=relu, depthwise_regularizer='l2', pointwise_regularizer={'class_name': 'L1L2', 'config': {'l1': 0.5, 'l2': 0.0}})
    assert (l.filters, l.k, l.stride, l.dilation, l.depth_multiplier, l.padding, l.activation[0]) == (4, 3, 2, 1, 1, 'valid', 'relu')
    assert l.depthwise_regularizer.l2 == np.float32(0.01) and l.pointwise_regularizer.l1 == 0.5
    assert S(4, 3, activation=None).activation[0] == 'linear' and S(4, 3, activation='softmax').activation[0] == 'softmax'


def test_weights_shapes_names_order_and_regularizers():
    from gennet_amd import engine, regularizers
    from gennet_amd.layers import SeparableConv1D as S
    l = S(6, 4, depth_multiplier=3, depthwise_regularizer=regularizers.l2(0.25), pointwise_regularizer=regularizers.l1(0.5),
          bias_regularizer=regularizers.l1_l2(0.125, 0.0625), name='sep')
    engine.set_init_seed(11)
    l._ensure_built((20, 5))
    assert [p.name for p in l.weights] == ['sep/depthwise_kernel', 'sep/pointwise_kernel', 'sep/bias']
    assert [p.shape for p in l.weights] == [(4, 5, 3), (1, 15, 6), (6,)] and l.count_params() == 60 + 90 + 6
    d, p, b = l.weights
    assert (d.regularizer.l1, d.regularizer.l2) == (0.0, 0.25) and (p.regularizer.l1, p.regularizer.l2) == (0.5, 0.0)
    assert (b.regularizer.l1, b.regularizer.l2) == (0.125, 0.0625) and not b.numpy().any()
    # keras' VarianceScaling fans of these shapes: receptive field x channels on either side; the depthwise kernel is drawn first
    engine.set_init_seed(11)
    assert np.array_equal(d.numpy(), engine.glorot_uniform((4, 5, 3))) and np.array_equal(p.numpy(), engine.glorot_uniform((1, 15, 6)))
    assert np.abs(d.numpy()).max() <= np.sqrt(6.0 / (4 * 5 + 4 * 3)) and np.abs(p.numpy()).max() <= np.sqrt(6.0 / (15 + 6))
    assert S(6, 4).depthwise_regularizer is None


def test_compute_output_shape():
    from gennet_amd.layers import SeparableConv1D as S
    assert S(6, 4, padding='same').compute_output_shape((20, 5)) == (20, 6) and S(6, 4).compute_output_shape((20, 5)) == (17, 6)
    assert S(6, 4, strides=3, padding='same').compute_output_shape((20, 5)) == (7, 6) and S(6, 4, strides=3).compute_output_shape((20, 5)) == (6, 6)
    assert S(2, 3, dilation_rate=5, padding='same').compute_output_shape((7, 5)) == (7, 2) and S(2, 40, padding='same').compute_output_shape((7, 1)) == (7, 2)
    assert S(2, 3, dilation_rate=4).compute_output_shape((9, 5)) == (1, 2)


CONFIG_KEYS = {'name', 'trainable', 'filters', 'kernel_size', 'strides', 'padding', 'data_format', 'dilation_rate', 'activation', 'use_bias',
               'bias_initializer', 'bias_regularizer', 'activity_regularizer', 'bias_constraint', 'depth_multiplier', 'depthwise_initializer',
               'pointwise_initializer', 'depthwise_regularizer', 'pointwise_regularizer', 'depthwise_constraint', 'pointwise_constraint'}


def keras_entry(**over):
    """a SeparableConv1D entry as keras 2.2.4 writes it (model.to_json())"""
    cfg = {"name": "separable_conv1d_7", "trainable": True, "batch_input_shape": [None, 33, 3], "dtype": "float32", "filters": 16, "kernel_size": [5],
           "strides": [1], "padding": "same", "data_format": "channels_last", "dilation_rate": [2], "depth_multiplier": 2, "activation": "relu",
           "use_bias": True, "depthwise_initializer": GLOROT_DICT, "pointwise_initializer": GLOROT_DICT,
           "bias_initializer": {"class_name": "Zeros", "config": {}},
           "depthwise_regularizer": {"class_name": "L1L2", "config": {"l1": 0.0, "l2": 0.0010000000474974513}}, "pointwise_regularizer": None,
           "bias_regularizer": None, "activity_regularizer": None, "depthwise_constraint": None, "pointwise_constraint": None, "bias_constraint": None}
    cfg.update(over)
    return {"class_name": "SeparableConv1D", "config": cfg}


def test_the_config_has_exactly_keras_keys():
    from gennet_amd.layers import SeparableConv1D as S
    cfg = S(4, 3).get_config()
    assert set(cfg) == CONFIG_KEYS
    assert (cfg['kernel_size'], cfg['strides'], cfg['dilation_rate'], cfg['depth_multiplier'], cfg['data_format']) == ([3], [1], [1], 1, 'channels_last')
    assert cfg['depthwise_initializer'] == cfg['pointwise_initializer'] == GLOROT_DICT and cfg['use_bias'] is True
    assert set(S(4, 3, input_shape=(9, 2)).get_config()) == CONFIG_KEYS | {'batch_input_shape', 'dtype'}
    assert not any(k.startswith('kernel_') and k != 'kernel_size' for k in cfg) and 'rank' not in cfg


def test_a_keras_config_entry_builds_the_layer_and_round_trips():
    from gennet_amd.engine import model_from_json
    entry = keras_entry()
    text = json.dumps({"class_name": "Sequential", "config": {"name": "sequential_1", "layers": [entry]}, "keras_version": "2.2.4", "backend": "tensorflow"})
    m = model_from_json(text)
    l = m.layers[0]
    assert type(l).__name__ == 'SeparableConv1D' and (l.name, l.filters, l.k, l.stride, l.dilation, l.depth_multiplier, l.padding) == (
        'separable_conv1d_7', 16, 5, 1, 2, 2, 'same')
    assert m.output_shape == (None, 33, 16) and [p.shape for p in l.weights] == [(5, 3, 2), (1, 6, 16), (16,)]
    assert l.depthwise_kernel.regularizer.l2 == np.float32(0.001) and l.pointwise_kernel.regularizer is None
    assert l.get_config() == entry['config']
    again = model_from_json(m.to_json())
    assert again.layers[0].get_config() == entry['config'] and json.loads(again.to_json())['config'] == json.loads(m.to_json())['config']
    with pytest.raises(NotImplementedError, match='depthwise_constraint'):
        model_from_json(json.dumps({"class_name": "Sequential", "config": {"name": "s", "layers": [
            keras_entry(depthwise_constraint={"class_name": "MaxNorm", "config": {"max_value": 2, "axis": 0}})]}}))


def test_the_class_lives_in_its_own_module_and_is_no_conv1d():
    from gennet_amd import layers as Ly, separable
    assert Ly.SeparableConv1D is separable.SeparableConv1D and Ly.SeparableConv1D.__module__ == 'gennet_amd.separable' != Ly.__name__
    assert not issubclass(Ly.SeparableConv1D, Ly.Conv1D) and not isinstance(Ly.SeparableConv1D(4, 3), Ly.Conv1D)


def test_the_facade_resolves():
    import gennet_amd.keras  # noqa: F401
    from gennet_amd import layers as Ly
    from gennet_amd.keras.layers import SeparableConv1D as top
    from gennet_amd.keras.layers.convolutional import SeparableConv1D as deep
    assert top is deep is Ly.SeparableConv1D
    assert 'SeparableConv1D' in gennet_amd.keras.__doc__


def test_the_planner_leaves_the_layer_alone():
    from gennet_amd import layers as Ly
    from gennet_amd.engine import Sequential
    m = Sequential()
    for l in (Ly.SeparableConv1D(8, 3, input_shape=(16, 4)), Ly.Activation('relu'), Ly.Dropout(0.5), Ly.SeparableConv1D(8, 3, activation='tanh'),
              Ly.BatchNormalization(), Ly.Flatten(), Ly.Dense(1)):
        m.add(l)
    nodes = [n for n in m.nodes if type(n.layer).__name__ == 'SeparableConv1D']
    assert len(nodes) == 2 and all(n.fused_act is None and n.fused_drop is None and n.infer_bn is None for n in nodes)
    assert not any(n.layer.fusable_act or n.layer.fusable_drop or getattr(n.layer, 'can_fold_bn', False) for n in nodes)
    assert [n.layer.writes_dy(n) for n in nodes] == [False, True]          # the activation gradient runs in place on dy


def test_the_header_declares_the_entry_points():
    from gennet_amd import _lib
    vp, sz, i32 = _lib.vp, _lib.sz, _lib.i32
    assert _lib.DECLS['gn_dwconv1d_fwd'] == (i32, [vp] * 3 + [i32] * 9 + [vp])
    assert _lib.DECLS['gn_dwconv1d_dgrad'] == (i32, [vp] * 3 + [i32] * 9 + [vp])
    assert _lib.DECLS['gn_dwconv1d_wgrad'] == (i32, [vp] * 4 + [sz] + [i32] * 9 + [vp])
    assert _lib.DECLS['gn_dwconv1d_wgrad_workspace'] == (sz, [i32] * 5)


# ---------------------------------------------------------------------------------------------------------------------
# the launch geometry
# ---------------------------------------------------------------------------------------------------------------------
def geom_constants():
    import re
    text = open(os.path.join(ROOT, 'gennet_amd', 'csrc', 'depthwise_geom.h')).read()
    return dict((k, int(eval(v.replace('(size_t)', '')))) for k, v in re.findall(r'constexpr \w+ (DW_\w+) = ([^;]+);', text))


def test_the_workspace_query_answers_on_the_host():
    """gn_dwconv1d_wgrad_workspace is host arithmetic (no device call): parts x (k C dm) doubles, the parts by csrc/depthwise_geom.h's rule"""
    from gennet_amd import _lib
    K = geom_constants()
    big = [(64, 2048, 64, 16, 1, 1, 1, 'same'), (16, 8192, 256, 5, 1, 1, 1, 'same'), (256, 2048, 8, 16, 1, 1, 2, 'same'), (64, 8192, 256, 40, 1, 1, 3, 'same')]
    capped = []
    for B, L, C, k, s, d, dm, padding in R.SHAPES + big:          # the second and the last of `big`: the 16 MiB cap, not the row rule, sets the parts
        Lout = R.geometry(L, k, s, padding, d)[0]
        rows, n = B * Lout, k * C * dm
        capped.append(K['DW_WG_WS_CAP'] // (8 * n) < min(-(-rows // K['DW_WG_MIN_ROWS']), K['DW_WG_MAX_PARTS']))
        p = max(min(-(-rows // K['DW_WG_MIN_ROWS']), K['DW_WG_MAX_PARTS'], K['DW_WG_WS_CAP'] // (8 * n)), 1)
        rpp = -(-rows // p)
        assert _lib.size('gn_dwconv1d_wgrad_workspace', B, Lout, C, k, dm) == -(-rows // rpp) * n * 8
    assert capped[-4:] == [False, True, False, True] and not any(capped[:-4])
    assert _lib.size('gn_dwconv1d_wgrad_workspace', 0, 5, 4, 3, 1) == 0 and _lib.size('gn_dwconv1d_wgrad_workspace', 2, 5, 0, 3, 1) == 0
    assert _lib.size('gn_dwconv1d_wgrad_workspace', 2, 5, 1 << 20, 1 << 10, 2) == 0                # k C dm does not fit an int


def test_the_geometry_walk_is_clean_under_the_host_sanitizers(tmp_path):
    """tests/tools/depthwise_geom_walk.cpp includes csrc/depthwise_geom.h, the header the kernels' file includes, and forms for every shape of
    the GPU test, on the scalar and on the vector path, every index the three kernels form, inside host buffers of the stated sizes: built with
    the host C++ compiler under the address and undefined-behaviour sanitizers and run as a program of its own."""
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    exe = os.path.join(str(tmp_path), 'depthwise_geom_walk')
    cmd = [cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-I', os.path.join(ROOT, 'gennet_amd', 'csrc'),
           os.path.join(ROOT, 'tests', 'tools', 'depthwise_geom_walk.cpp'), '-o', exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    args, launches = [], 0
    for B, L, C, k, s, d, dm, padding in R.SHAPES:
        Lout, pl, _ = R.geometry(L, k, s, padding, d)
        args += [B, L, C, k, s, d, dm, pl, Lout]
        launches += 2 if C * dm % 4 == 0 else 1
    r = subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert r.stdout.strip().splitlines()[-1] == 'walked %d launches of each kernel' % launches, r.stdout
