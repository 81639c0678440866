"""fp64 restatement (torch CPU, float64 autograd) of the reference's generator g_model.hdf5 (Keras 2.1.6): Reshape((-1, 1, 1)),
BatchNormalization, four Conv2DTranspose(F, (1, k), 'valid', relu) + BatchNormalization with (F, k) = (128, 4), (64, 8), (32, 16), (16, 32),
Flatten, BatchNormalization, Dense(50, relu), BatchNormalization, Dense(50); binary cross-entropy from probabilities (keras' clip to
[1e-7, 1 - 1e-7] in float32, logit form); plain SGD.  Independent of gennet_amd: weights in, numbers out."""
import numpy as np
import torch
import torch.nn.functional as F

EPS_BN = 1e-3
# keras clips the probabilities to [epsilon, 1 - epsilon] in float32: the bounds as float32 values (1 - 1e-7 rounds to 1 - 2^-23), so the
# saturated outputs cost what they cost in keras and in the float32 loss kernel
CLIP_LO = float(np.float32(1e-7))
CLIP_HI = float(np.float32(1.0) - np.float32(1e-7))
CONVS = ['conv2d_transpose_%d' % i for i in range(1, 5)]
BNS = ['batch_normalization_%d' % i for i in range(1, 8)]


def params_from(weights):
    """{layer name: [np arrays in keras order]} -> {(layer, name): float64 tensor}"""
    out = {}
    for l, ws in weights.items():
        names = ['gamma', 'beta', 'moving_mean', 'moving_variance'] if l.startswith('batch') else ['kernel', 'bias']
        for n, w in zip(names, ws):
            out[(l, n)] = torch.tensor(np.asarray(w, np.float64), requires_grad=n not in ('moving_mean', 'moving_variance'))
    return out


def _bn(h, P, name, training):
    g, b = P[(name, 'gamma')], P[(name, 'beta')]
    if training:
        axes = tuple(range(h.dim() - 1))
        mean = h.mean(dim=axes)
        var = ((h - mean) ** 2).mean(dim=axes)
    else:
        mean, var = P[(name, 'moving_mean')], P[(name, 'moving_variance')]
    return (h - mean) / torch.sqrt(var + EPS_BN) * g + b


def forward(P, x, training):
    """x: (B, 1, 1) noise -> (B, 50)."""
    B = x.shape[0]
    h = torch.as_tensor(x, dtype=torch.float64).reshape(B, 1, 1, 1)
    h = _bn(h, P, BNS[0], training)
    for i, c in enumerate(CONVS):
        W, b = P[(c, 'kernel')], P[(c, 'bias')]
        h = torch.relu(F.conv_transpose2d(h.permute(0, 3, 1, 2), W.permute(3, 2, 0, 1), stride=(1, 1)).permute(0, 2, 3, 1) + b)
        h = _bn(h, P, BNS[i + 1], training)
    h = h.reshape(B, -1)
    h = _bn(h, P, BNS[5], training)
    h = torch.relu(h @ P[('dense_1', 'kernel')] + P[('dense_1', 'bias')])
    h = _bn(h, P, BNS[6], training)
    return h @ P[('dense_2', 'kernel')] + P[('dense_2', 'bias')]


def bce(p, y):
    pc = torch.clamp(p, CLIP_LO, CLIP_HI)
    z = torch.log(pc / (1 - pc))
    return (torch.clamp(z, min=0) - z * y + torch.log1p(torch.exp(-z.abs()))).mean()


def sgd_train(P, x, y, lr, steps):
    """`steps` train_on_batch steps on the same batch: returns the losses; P is updated in place."""
    yt = torch.as_tensor(y, dtype=torch.float64)
    losses = []
    for _ in range(steps):
        for t in P.values():
            t.grad = None
        loss = bce(forward(P, x, True), yt)
        loss.backward()
        losses.append(float(loss.detach()))
        with torch.no_grad():
            for t in P.values():
                if t.requires_grad:
                    t -= lr * t.grad
    return losses
