"""The reference's generator g_model.hdf5 on the GPU: built with model_from_json from the golden model_config, the real best_g_weights.hdf5
loaded; predict and five SGD train_on_batch steps against the fp64 restatement (tests/g_model_ref.py), three captured training steps against
three eager ones bit for bit; and Dense over widths that are not multiples of 4 (its two Dense(50) heads)."""
import json
import os

import numpy as np
import pytest
import torch

import g_model_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'keras_h5_golden.json')))['g_model.hdf5']
WEIGHTS = os.path.join(ROOT, 'tests', 'golden', 'keras_h5', 'best_g_weights.hdf5')
LR = float(np.float32(0.004))


def build():
    from gennet_amd.engine import SGD, model_from_json
    from gennet_amd import keras_io
    m = model_from_json(json.dumps(GOLD['model_config']))
    m.load_weights(WEIGHTS)
    m.compile(optimizer=SGD(lr=0.004), loss='binary_crossentropy')
    weights = {l.name: [p.numpy() for p in keras_io.keras_weights(l)] for l in keras_io.top_layers(m) if keras_io.keras_weights(l)}
    return m, weights


def rel(a, ref):
    a = np.asarray(a, np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-30)


def test_predict_matches_fp64_restatement():
    m, weights = build()
    x = np.random.RandomState(0).randn(256, 1, 1).astype(np.float32)
    y = m.predict(x, batch_size=256)
    with torch.no_grad():
        ref = R.forward(R.params_from(weights), x.astype(np.float64), False).numpy()
    assert y.shape == (256, 50)
    assert rel(y, ref) < 1e-5


def test_five_sgd_steps_match_fp64_restatement():
    """Five train_on_batch steps with SGD(0.004) and binary cross-entropy over the 50 output columns: the Conv2DTranspose -> BatchNormalization
    pairs, BatchNormalization over 1 and 50 channels and the Dense(50) heads in training.  Each step is checked against the fp64 step taken from
    the weights the GPU model holds at that point: the generator's last layer is linear and keras' BCE clips it, so outputs near the clip edges
    make the trajectory itself ill-conditioned (run free, the fp32 and fp64 losses agreed to 5e-8 for two steps, then parted by 4e-5 at the
    third and 4e-3 at the fourth); re-anchoring keeps every step's loss and update comparable at fp32 precision."""
    from gennet_amd import keras_io
    m, _ = build()
    rng = np.random.RandomState(1)
    x = rng.randn(256, 1, 1).astype(np.float32)
    t = rng.uniform(0, 1, (256, 50)).astype(np.float32)
    tops = [l for l in keras_io.top_layers(m) if keras_io.keras_weights(l)]
    for step in range(5):
        P = R.params_from({l.name: [p.numpy() for p in keras_io.keras_weights(l)] for l in tops})
        ref = R.sgd_train(P, x.astype(np.float64), t.astype(np.float64), LR, 1)[0]
        loss = m.train_on_batch(x, t)[0]
        assert abs(loss - ref) <= 1e-6 * abs(ref), (step, loss, ref)
        for l in tops:
            names = ['gamma', 'beta', 'moving_mean', 'moving_variance'] if l.name.startswith('batch') else ['kernel', 'bias']
            for p, n in zip(keras_io.keras_weights(l), names):
                if not n.startswith('moving'):
                    # floor 1e-3 on the scale: batch_normalization_5's beta (~1e-8) has a zero gradient in exact arithmetic -- its per-channel
                    # shift is normalised away by the BatchNormalization over the flattened features -- and moves by rounding noise only
                    w_ref = P[(l.name, n)].detach().numpy()
                    err = np.abs(p.numpy().astype(np.float64) - w_ref).max() / max(np.abs(w_ref).max(), 1e-3)
                    assert err < 1e-4, (step, l.name, n, err)           # test_nets_gpu.py's tolerance on trained weights


def test_captured_training_steps_equal_eager_steps_bit_for_bit():
    from gennet_amd import keras_io
    from gennet_amd.engine import StepGraph, device
    rng = np.random.RandomState(2)
    xh = rng.randn(64, 1, 1).astype(np.float32)
    th = rng.uniform(0, 1, (64, 50)).astype(np.float32)
    eager, _ = build()
    graphed, _ = build()
    x = torch.tensor(xh, device=device()); t = torch.tensor(th, device=device())
    la = [eager.train_result(eager.train_on_batch_device([x], [t]), 64) for _ in range(4)]
    graphed.train_on_batch_device([x], [t])          # one eager step first: binds the parameter groups and scratch buffers the graph will hold
    la = la[1:]
    sg = StepGraph()
    torch.cuda.synchronize()
    sg.capture(lambda: graphed.train_on_batch_device([x], [t]))
    lb = []
    for i in range(3):
        if i:
            sg.wait_inputs_consumed()
        lb.append(graphed.train_result(sg.replay(), 64))
    assert la == lb
    for a, b in zip(keras_io.top_layers(eager), keras_io.top_layers(graphed)):
        for p, q in zip(keras_io.keras_weights(a), keras_io.keras_weights(b)):
            assert np.array_equal(p.numpy(), q.numpy()), (a.name, p.name)


@pytest.mark.parametrize('C', [1, 2, 3, 5, 50, 913])
@pytest.mark.parametrize('n_in', [64, 50])
def test_dense_gradients_over_any_width(C, n_in):
    """Dense(C) forward, data, weight and bias gradients against fp64, and two runs bit-identical (the 50 -> 50 head included)."""
    from gennet_amd import ops
    rng = np.random.RandomState(C + n_in)
    B = 300
    x = rng.randn(B, n_in).astype(np.float32); w = (rng.randn(n_in, C) * 0.1).astype(np.float32); b = rng.randn(C).astype(np.float32)
    dy = rng.randn(B, C).astype(np.float32)
    dev = torch.device('cuda:0')
    X, Wt, Bt, DY = (torch.tensor(v, device=dev) for v in (x, w, b, dy))
    y = ops.dense_fwd(X, Wt, Bt, 'relu')
    y_ref = np.maximum(x.astype(np.float64) @ w + b, 0)
    assert rel(y.cpu().numpy(), y_ref) < 2e-5
    dx, dw, db = ops.dense_bwd(X, Wt, DY)
    # fp32 fmaf chains over up to 913 terms: the project's conv tolerance, 2e-5 of the largest value
    assert rel(dx.cpu().numpy(), dy.astype(np.float64) @ w.T.astype(np.float64)) < 2e-5
    assert rel(dw.cpu().numpy(), x.T.astype(np.float64) @ dy) < 2e-5
    assert rel(db.cpu().numpy(), dy.astype(np.float64).sum(0)) < 1e-6
    dx2, dw2, db2 = ops.dense_bwd(X, Wt, DY)
    assert torch.equal(dx, dx2) and torch.equal(dw, dw2) and (C <= 4 or torch.equal(db, db2))
    assert torch.equal(y, ops.dense_fwd(X, Wt, Bt, 'relu'))
