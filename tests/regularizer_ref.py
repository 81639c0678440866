"""Reference for the regularizer tests (numpy / torch fp64): the penalty and gradient of Keras 2.2.4's L1L2 on fp32 inputs with fp32 coefficients,
and the six layers of tests/test_regularizers_gpu.py restated in torch fp64 so that autograd differentiates loss + penalties."""
import math

import numpy as np
import torch
import torch.nn.functional as F


def lam(v):
    """the coefficient the kernels use: K.cast_to_floatx(v), widened again"""
    return float(np.float32(v))


def penalty(x, l1, l2):
    """math.fsum of the fp64 terms l1 |x| + l2 x^2 of the fp32 tensor x"""
    v = np.asarray(x, np.float32).astype(np.float64).ravel()
    return math.fsum((lam(l1) * np.abs(v) + lam(l2) * (v * v)).tolist())


def grad(g, x, l1, l2):
    """fp64 g + l1 sign(x) + 2 l2 x, sign(+-0) = 0, and the bound 4 * 2^-24 * (|g| + l1 + 2 l2 |x|) of three fp32 roundings and one to spare"""
    g, x = np.asarray(g, np.float32).astype(np.float64), np.asarray(x, np.float32).astype(np.float64)
    ref = g + lam(l1) * np.sign(x) + 2.0 * lam(l2) * x
    bound = 4.0 * 2.0 ** -24 * (np.abs(g) + lam(l1) + 2.0 * lam(l2) * np.abs(x))
    return ref, bound


def t_penalty(t, reg):
    """the penalty of a torch tensor under reg = (l1, l2) or None; torch's |.| has the subgradient 0 at 0, as Keras' K.abs has"""
    if reg is None:
        return 0.0
    return lam(reg[0]) * t.abs().sum() + lam(reg[1]) * (t * t).sum()


# ---- the layers, channels_last, weights in this project's (= Keras') layouts
def dense(x, w, b, act=None):
    return activate(x @ w + b, act)


def conv1d(x, w, b, act=None):
    """'valid', stride 1: x (B, L, Cin), w (k, Cin, Cout)"""
    return activate(F.conv1d(x.permute(0, 2, 1), w.permute(2, 1, 0), b).permute(0, 2, 1), act)


def conv2d_same(x, w, b, act=None):
    """'same', stride 1, odd kernel: x (B, H, W, Cin), w (kh, kw, Cin, Cout)"""
    kh, kw = w.shape[0], w.shape[1]
    return activate(F.conv2d(x.permute(0, 3, 1, 2), w.permute(3, 2, 0, 1), b, padding=(kh // 2, kw // 2)).permute(0, 2, 3, 1), act)


def conv2d_transpose(x, w, b, act=None):
    """'valid', strides (1, 1): x (B, H, W, Cin), w (1, kw, filters, Cin)"""
    return activate(F.conv_transpose2d(x.permute(0, 3, 1, 2), w.permute(3, 2, 0, 1), b).permute(0, 2, 3, 1), act)


def batchnorm(x, gamma, beta, eps=1e-3):
    """training phase, last axis: batch mean and biased variance"""
    axes = tuple(range(x.dim() - 1))
    mean, var = x.mean(axes), x.var(axes, unbiased=False)
    return (x - mean) / torch.sqrt(var + eps) * gamma + beta


def prelu(x, alpha):
    return torch.where(x > 0, x, alpha * x)


def activate(z, act):
    if act in (None, 'linear'):
        return z
    return {'tanh': torch.tanh, 'sigmoid': torch.sigmoid, 'relu': torch.relu}[act](z)


def bce(p, y):
    """keras binary_crossentropy on probabilities, clipped at the fp32 numbers epsilon = 1e-7 and 1 - epsilon, mean over everything"""
    p = p.clamp(float(np.float32(1e-7)), float(np.float32(1.0) - np.float32(1e-7)))
    return -(y * torch.log(p) + (1.0 - y) * torch.log(1.0 - p)).mean()


def mse(p, y):
    return ((p - y) ** 2).mean(-1).mean()


def t64(a, grad=False):
    return torch.tensor(np.asarray(a, np.float32).astype(np.float64), requires_grad=grad)
