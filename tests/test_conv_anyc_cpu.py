"""Host side of the any-channel convolutions, no device needed: the predicate the library exports, what the planner declines for a
channel pair that only the `anyc` kernels take, the stride rule at build, and the fp64 restatement of d_model against the definition."""
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_conv_needs_any_is_exactly_the_pairs_the_strict_entry_points_refuse():
    from gennet_amd import ops
    for pair in [(1, 50), (4, 50), (50, 4), (6, 10), (5, 5), (1, 1), (3, 3), (7, 64), (64, 7), (50, 30), (130, 258), (2, 6), (5, 8), (8, 5),
                 (4, 1), (4, 2), (4, 3), (2, 3)]:          # the last four: Cin <= 4 goes to the small-Cin kernels whatever Cout is, which need Cout % 4 == 0
        assert ops.conv_needs_any(*pair) is True, pair
    for pair in [(4, 48), (48, 4), (8, 12), (1, 4), (3, 4), (4, 4), (64, 64), (3, 8), (8, 3), (2, 16), (512, 1), (1, 1024)]:
        assert ops.conv_needs_any(*pair) is False, pair
    # a layer also runs the swapped pair, in its data gradient: 3 -> 4 is strict forward, ragged backward
    assert ops.conv_layer_needs_any(3, 4) and ops.conv_layer_needs_any(4, 3) and not ops.conv_layer_needs_any(8, 3) and not ops.conv_layer_needs_any(4, 8)
    for cin in range(1, 40):            # the dispatch of csrc/capi.hip conv_run and csrc/small_conv.hip, stated once more
        for cout in range(1, 40):       # (tests/test_conv_anyc_gpu.py checks the predicate against the dispatchers' own refusals)
            strict = cout % 4 == 0 if cin <= 4 else (cin % 4 == 0 if cout <= 4 else (cin % 4 == 0 and cout % 4 == 0))
            assert ops.conv_needs_any(cin, cout) == (not strict), (cin, cout)


def _net(filters, cin):
    from gennet_amd.engine import Sequential
    from gennet_amd.layers import Conv1D, Dropout, LeakyReLU
    m = Sequential([Conv1D(filters, 5, input_shape=(64, cin)), LeakyReLU(0.2), Dropout(0.3)])
    m._plan()
    return m


def test_planner_declines_the_fused_dropout_per_instance():
    leaky = ('leaky', float(np.float32(0.2)))
    m = _net(30, 8)                     # (8, 30): only the anyc kernels take it
    conv, act, drop = m.nodes
    assert conv.fused_act == leaky and act.absorbed                # the plain epilogue applies the activation
    assert conv.fused_drop is None and not drop.absorbed           # the Dropout layer runs on its own
    m = _net(32, 8)                     # aligned: both fused, as before
    conv, act, drop = m.nodes
    assert conv.fused_act == leaky and conv.fused_drop[0] == 0.3 and act.absorbed and drop.absorbed
    m = _net(32, 50)                    # aligned filters, ragged input channels
    conv, act, drop = m.nodes
    assert conv.fused_act == leaky and conv.fused_drop is None and not drop.absorbed


def test_tap_folded_pair_decides():
    """16 taps on 1 channel run as 4 taps on 4 channels: (4, 50) needs the anyc kernels, (4, 48) does not."""
    from gennet_amd.engine import Sequential
    from gennet_amd.layers import Conv1D, Dropout
    for filters, fused in ((50, False), (48, True)):
        m = Sequential([Conv1D(filters, 16, input_shape=(50, 1)), Dropout(0.25)])
        m._plan()
        assert (m.nodes[0].fused_drop is not None) == fused and m.nodes[1].absorbed == fused


def test_stride_above_two_on_an_any_channel_pair_is_refused_at_build():
    from gennet_amd.engine import Sequential
    from gennet_amd.layers import Conv1D
    with pytest.raises(NotImplementedError, match='strides'):
        Sequential([Conv1D(6, 4, strides=3, input_shape=(64, 2))])
    Sequential([Conv1D(8, 4, strides=3, input_shape=(64, 2))])      # the small-Cin kernels: any stride
    Sequential([Conv1D(6, 4, strides=2, input_shape=(64, 2))])      # the anyc kernels: strides 1 and 2
    with pytest.raises(NotImplementedError, match='strides'):
        Sequential([Conv1D(3, 4, strides=3, input_shape=(64, 4))])  # 4 -> 3: the small-Cin kernels need a multiple of 4 filters


def test_d_model_ref_forward_against_the_definition():
    import torch
    import d_model_ref as R
    rng = np.random.RandomState(0)
    weights = {'conv1d_1': [rng.randn(16, 1, 50) * 0.2, rng.randn(50) * 0.1], 'dense_3': [rng.randn(1750, 50) * 0.03, rng.randn(50) * 0.1],
               'dense_4': [rng.randn(50, 2) * 0.3, rng.randn(2) * 0.1]}
    x = rng.randn(7, 50)
    with torch.no_grad():
        got = R.forward(R.params_from(weights), x).numpy()
    want = R.forward_direct(weights, x)
    assert got.shape == (7, 2) and np.abs(got - want).max() < 1e-13
    # the loss: keras' clipped cross-entropy, mean over both columns
    y = np.array([[0.0, 1.0]] * 7)
    pc = np.clip(want, R.G.CLIP_LO, R.G.CLIP_HI)
    assert abs(float(R.bce(torch.tensor(want), torch.tensor(y))) - float(-(y * np.log(pc) + (1 - y) * np.log(1 - pc)).mean())) < 1e-14
    # alpha and Adam's hyper-parameters are the float32 values the file records
    gold = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'keras_h5_golden.json')))['d_model.hdf5']
    lk = [l['config'] for l in gold['model_config']['config']['layers'] if l['class_name'] == 'LeakyReLU']
    assert lk[0]['alpha'] == R.ALPHA
    oc = gold['training']['optimizer_config']['config']
    assert (oc['lr'], oc['beta_1'], oc['beta_2'], oc['epsilon']) == (R.ADAM['lr'], R.ADAM['beta_1'], R.ADAM['beta_2'], R.ADAM['epsilon'])
