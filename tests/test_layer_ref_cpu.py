"""tests/layer_ref.py (the references of tests/test_layer_passes_gpu.py) against torch float64 autograd, or against a plain loop.  No GPU."""
import numpy as np
import pytest
import torch

import layer_ref as R
from oracle import keras_ref as K


def _torch_act(z, kind, p):
    if kind == 'linear':
        return z
    if kind == 'relu':
        return torch.relu(z)
    if kind == 'relu_max':
        return torch.clamp(z, 0.0, p)
    if kind == 'leaky':
        return torch.nn.functional.leaky_relu(z, p)
    if kind == 'tanh':
        return torch.tanh(z)
    return torch.sigmoid(z)


@pytest.mark.parametrize("kind,p", [('linear', 0.0), ('relu', 0.0), ('relu_max', 1.0), ('leaky', 0.2), ('tanh', 0.0), ('sigmoid', 0.0)])
@pytest.mark.parametrize("rate", [0.0, 0.3])
def test_act_dropout_bwd_through_the_layer_output_is_the_autograd_gradient(kind, p, rate):
    rng = np.random.RandomState(3)
    z = rng.randn(7, 33) * 2
    mask = (rng.rand(7, 33) >= rate).astype(np.uint8)
    dy = rng.randn(7, 33)
    zt = torch.tensor(z, requires_grad=True)
    yt = _torch_act(zt, kind, p) * torch.tensor(mask, dtype=torch.float64) / (1.0 - rate)
    yt.backward(torch.tensor(dy))
    y = yt.detach().numpy()
    assert np.abs(y - K.dropout_fwd(K.act_fwd(z, kind, p), mask, rate)).max() <= 1e-15       # the oracle's forward is the one differentiated
    dz = R.act_dropout_bwd(dy, y, mask, kind, p, rate)
    assert dz.dtype == np.float64 and dz.shape == z.shape
    assert np.abs(dz - zt.grad.numpy()).max() <= 1e-13 * np.abs(dz).max()
    assert (dz[mask == 0] == 0).all()
    # and it is the two oracle steps one after the other
    step = K.act_bwd(dy * mask / (1.0 - rate), K.act_fwd(z, kind, p), kind, p)
    assert np.abs(dz - step).max() <= 1e-13 * np.abs(dz).max()


@pytest.mark.parametrize("b0_given,b1_given", [(True, True), (True, False), (False, True), (False, False)])
def test_affine_stack_forward_and_gradient(b0_given, b1_given):
    rng = np.random.RandomState(4)
    B, n = 3, 17
    x = rng.randn(B, n, 1); a0, a1 = 0.75, -1.5
    b0 = rng.randn(n) if b0_given else None
    b1 = rng.randn(n) if b1_given else None
    img = R.affine_stack_fwd(x, a0, b0, a1, b1)
    assert img.shape == (B, n, 2, 1)
    for b in range(B):                                             # plain loop
        for t in range(n):
            assert img[b, t, 0, 0] == a0 * x[b, t, 0] + (b0[t] if b0_given else 0.0)
            assert img[b, t, 1, 0] == a1 * x[b, t, 0] + (b1[t] if b1_given else 0.0)
    xt = torch.tensor(x, requires_grad=True)
    z0 = a0 * xt + (torch.tensor(b0).reshape(1, n, 1) if b0_given else 0.0)
    z1 = a1 * xt + (torch.tensor(b1).reshape(1, n, 1) if b1_given else 0.0)
    it = torch.stack([z0, z1], dim=2)
    assert np.array_equal(it.detach().numpy(), img)
    dimg = rng.randn(B, n, 2, 1)
    it.backward(torch.tensor(dimg))
    dx = R.affine_stack_bwd(dimg, a0, a1)
    assert dx.shape == (B, n, 1)
    assert np.abs(dx - xt.grad.numpy()).max() <= 1e-15


def test_affine_stack_restates_mylayer():
    rng = np.random.RandomState(5)
    x = rng.randn(4, 33, 1); ev = rng.randn(33, 1)
    assert np.array_equal(R.affine_stack_fwd(x, 1.0, None, -1.0, ev.reshape(-1)), K.mylayer_fwd(x, ev))
    dimg = rng.randn(4, 33, 2, 1)
    assert np.array_equal(R.affine_stack_bwd(dimg, 1.0, -1.0), K.mylayer_bwd(dimg))


@pytest.mark.parametrize("B,n", [(1, 5), (3, 33)])
def test_assemble_d_batch_against_the_prepend_loop(B, n):
    """The training loop builds the fake half by PREPENDING one image after the other to a list, so sample i ends at row 2B - 1 - i."""
    rng = np.random.RandomState(6)
    real, noise, fake = rng.randn(B, n), rng.randn(B, n), rng.randn(B, n)
    event = rng.randn(n)
    rows = []
    for i in range(B):
        rows.insert(0, np.stack([fake[i], event - fake[i]], axis=1))
    want = np.concatenate([np.stack([real, noise], axis=2), np.stack(rows, axis=0)], axis=0).reshape(2 * B, n, 2, 1)
    got = R.assemble_d_batch(real, noise, fake, event)
    assert got.shape == (2 * B, n, 2, 1) and np.array_equal(got, want)
    assert np.array_equal(got[B:, :, 0, 0], fake[::-1]) and np.array_equal(got[2 * B - 1, :, 1, 0], event - fake[0])
