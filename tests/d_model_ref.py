"""fp64 restatement (torch CPU, float64 autograd) of the reference's discriminator d_model.hdf5 (Keras 2.1.6):
Input(50) -> Reshape((50, 1)) -> Conv1D(50, 16, 'valid') -> LeakyReLU(float32(0.2)) -> Flatten -> Dense(50, tanh) -> Dense(2, sigmoid);
keras' binary cross-entropy (probabilities clipped to [1e-7, 1 - 1e-7] in float32, mean over the 2 columns and the batch); Adam with the float32
hyper-parameters the file's training_config records; and one step of the GAN built on it: the generator (tests/g_model_ref.py, training phase)
into the frozen discriminator, gradients to the generator only, plain SGD.  Independent of gennet_amd: weights in, numbers out."""
import numpy as np
import torch
import torch.nn.functional as F

import g_model_ref as G

ALPHA = float(np.float32(0.2))            # LeakyReLU's alpha as the file records it: 0.20000000298023224
ADAM = dict(lr=float(np.float32(0.004)), beta_1=float(np.float32(0.5)), beta_2=float(np.float32(0.999)), epsilon=1e-7)
LAYERS = ['conv1d_1', 'dense_3', 'dense_4']


def params_from(weights, requires_grad=True):
    """{layer name: [kernel, bias]} -> {(layer, 'kernel' | 'bias'): float64 tensor}"""
    return {(l, n): torch.tensor(np.asarray(w, np.float64), requires_grad=requires_grad) for l, ws in weights.items() for n, w in zip(['kernel', 'bias'], ws)}


def forward(P, x):
    """x: (B, 50) -> (B, 2) probabilities."""
    h = torch.as_tensor(x, dtype=torch.float64)
    B = h.shape[0]
    W = P[('conv1d_1', 'kernel')]                                                   # keras (16, 1, 50) -> torch (50, 1, 16); cross-correlation in both
    h = F.conv1d(h.reshape(B, 1, 50), W.permute(2, 1, 0)).permute(0, 2, 1) + P[('conv1d_1', 'bias')]      # (B, 35, 50), channels last
    h = torch.where(h > 0, h, ALPHA * h).reshape(B, -1)                              # Flatten: feature index t * 50 + c
    h = torch.tanh(h @ P[('dense_3', 'kernel')] + P[('dense_3', 'bias')])
    return torch.sigmoid(h @ P[('dense_4', 'kernel')] + P[('dense_4', 'bias')])


def bce(p, y):
    """mean over all B * 2 elements of -(y log p + (1 - y) log(1 - p)) on the clipped probabilities"""
    pc = torch.clamp(p, G.CLIP_LO, G.CLIP_HI)
    return -(y * torch.log(pc) + (1 - y) * torch.log(1 - pc)).mean()


class Adam(object):
    """keras.optimizers.Adam (2.1.6 / 2.2.4): lr_t = lr sqrt(1 - beta_2^t) / (1 - beta_1^t); p -= lr_t m / (sqrt(v) + epsilon).  The moments live
    across steps; the parameters are handed in per step (a test may re-anchor them)."""

    def __init__(self, **kw):
        self.c = dict(ADAM, **kw)
        self.t = 0
        self.m, self.v = {}, {}

    def step(self, P):
        c = self.c
        self.t += 1
        lr_t = c['lr'] * np.sqrt(1.0 - c['beta_2'] ** self.t) / (1.0 - c['beta_1'] ** self.t)
        with torch.no_grad():
            for k, p in P.items():
                g = p.grad
                m = c['beta_1'] * self.m.get(k, torch.zeros_like(p)) + (1.0 - c['beta_1']) * g
                v = c['beta_2'] * self.v.get(k, torch.zeros_like(p)) + (1.0 - c['beta_2']) * g * g
                self.m[k], self.v[k] = m, v
                p -= lr_t * m / (torch.sqrt(v) + c['epsilon'])


def train_step(P, opt, x, y):
    """One train_on_batch of the discriminator: the loss before the update; P updated in place."""
    for t in P.values():
        t.grad = None
    loss = bce(forward(P, x), torch.as_tensor(y, dtype=torch.float64))
    loss.backward()
    opt.step(P)
    return float(loss.detach())


def gan_step(PG, PD, z, y, lr):
    """One train_on_batch of GAN = D(G(z)) with D frozen: the generator in its training phase (batch statistics), the loss on the discriminator's
    output, SGD(lr) on the generator's trainable weights.  Returns the loss before the update; PG updated in place, PD untouched."""
    for t in PG.values():
        t.grad = None
    loss = bce(forward(PD, G.forward(PG, z, True)), torch.as_tensor(y, dtype=torch.float64))
    grads = torch.autograd.grad(loss, [t for t in PG.values() if t.requires_grad])
    with torch.no_grad():
        for t, g in zip([t for t in PG.values() if t.requires_grad], grads):
            t -= lr * g
    return float(loss.detach())


def forward_direct(weights, x):
    """The same forward as plain numpy loops over the definition (no conv routine, no autograd): what forward() is checked against."""
    Wc, bc = (np.asarray(a, np.float64) for a in weights['conv1d_1'])
    x = np.asarray(x, np.float64)
    B = x.shape[0]
    h = np.zeros((B, 35, 50))
    for t in range(35):
        for j in range(16):
            h[:, t, :] += x[:, t + j, None] * Wc[j, 0, :]
    h += bc
    h = np.where(h > 0, h, ALPHA * h).reshape(B, 1750)
    W3, b3 = (np.asarray(a, np.float64) for a in weights['dense_3'])
    W4, b4 = (np.asarray(a, np.float64) for a in weights['dense_4'])
    h = np.tanh(h @ W3 + b3)
    return 1.0 / (1.0 + np.exp(-(h @ W4 + b4)))
