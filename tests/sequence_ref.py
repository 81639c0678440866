"""fp64 numpy restatements of the sequence layers, forward and backward, as plain indexing: Permute, RepeatVector, ZeroPadding1D,
Cropping1D and Dense over the last axis.  Written from the layers' definitions in keras 2.2.4, not from the kernels; tests/test_sequence_cpu.py
holds every function against torch (permute, F.pad, slicing, expand, matmul and their autograd gradients).

The copies keep the dtype they are given (so a float32 result can be compared bit for bit); the sums are taken in float64.  `as_torch` turns a
(forward, backward) pair into a torch.autograd.Function, so a model-level reference steps through these restatements in both directions."""
import numpy as np


def permute_fwd(x, perm):
    """axis i of y is axis perm[i] of x (perm counts the batch axis)"""
    y = np.empty(tuple(x.shape[p] for p in perm), x.dtype)
    src = [0] * x.ndim
    for idx in np.ndindex(*y.shape):
        for i, p in enumerate(perm):
            src[p] = idx[i]
        y[idx] = x[tuple(src)]
    return y


def permute_bwd(dy, perm):
    """the gradient of permute_fwd: every element goes back where it came from"""
    shape = [0] * dy.ndim
    for i, p in enumerate(perm):
        shape[p] = dy.shape[i]
    dx = np.empty(tuple(shape), dy.dtype)
    src = [0] * dy.ndim
    for idx in np.ndindex(*dy.shape):
        for i, p in enumerate(perm):
            src[p] = idx[i]
        dx[tuple(src)] = dy[idx]
    return dx


def inverse_perm(perm):
    inv = [0] * len(perm)
    for i, p in enumerate(perm):
        inv[p] = i
    return inv


def repeat_fwd(x, n):
    B, C = x.shape
    y = np.empty((B, n, C), x.dtype)
    for b in range(B):
        for j in range(n):
            y[b, j, :] = x[b, :]
    return y


def repeat_bwd(dy):
    """dx[b, c] = sum_j dy[b, j, c] in float64, j ascending"""
    B, n, C = dy.shape
    dx = np.zeros((B, C), np.float64)
    for b in range(B):
        for j in range(n):
            dx[b, :] += dy[b, j, :].astype(np.float64)
    return dx


def pad_fwd(x, left, right):
    B, L, C = x.shape
    y = np.zeros((B, left + L + right, C), x.dtype)
    for b in range(B):
        for l in range(L):
            y[b, left + l, :] = x[b, l, :]
    return y


def crop_fwd(x, left, right):
    B, L, C = x.shape
    y = np.empty((B, L - left - right, C), x.dtype)
    for b in range(B):
        for l in range(L - left - right):
            y[b, l, :] = x[b, left + l, :]
    return y


def pad_bwd(dy, left, right):
    return crop_fwd(dy, left, right)


def crop_bwd(dy, left, right):
    return pad_fwd(dy, left, right)


def dense_fwd(x, w, b):
    """y[..., o] = b[o] + sum_i x[..., i] w[i, o] at every position in front of the last axis, float64"""
    x, w, b = np.asarray(x, np.float64), np.asarray(w, np.float64), np.asarray(b, np.float64)
    y = np.empty(x.shape[:-1] + (w.shape[1],), np.float64)
    for idx in np.ndindex(*x.shape[:-1]):
        for o in range(w.shape[1]):
            y[idx + (o,)] = b[o] + np.sum(x[idx] * w[:, o])
    return y


def dense_bwd(x, w, dy):
    """-> dx, dw, db"""
    x, w, dy = np.asarray(x, np.float64), np.asarray(w, np.float64), np.asarray(dy, np.float64)
    dx, dw, db = np.zeros_like(x), np.zeros_like(w), np.zeros(w.shape[1], np.float64)
    for idx in np.ndindex(*x.shape[:-1]):
        for i in range(w.shape[0]):
            dx[idx + (i,)] = np.sum(dy[idx] * w[i, :])
        dw += x[idx][:, None] * dy[idx][None, :]
        db += dy[idx]
    return dx, dw, db


def as_torch(forward, backward):
    """f(t) on a torch tensor: forward(numpy) going up, backward(numpy gradient) coming down"""
    import torch

    class Fn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, t):
            return torch.from_numpy(np.ascontiguousarray(forward(t.detach().numpy())))

        @staticmethod
        def backward(ctx, g):
            return torch.from_numpy(np.ascontiguousarray(backward(g.detach().numpy())))

    return Fn.apply


def torch_permute(t, perm):
    return as_torch(lambda x: permute_fwd(x, perm), lambda g: permute_bwd(g, perm))(t)


def torch_repeat(t, n):
    return as_torch(lambda x: repeat_fwd(x, n), lambda g: repeat_bwd(g))(t)


def torch_pad(t, left, right):
    return as_torch(lambda x: pad_fwd(x, left, right), lambda g: pad_bwd(g, left, right))(t)


def torch_crop(t, left, right):
    return as_torch(lambda x: crop_fwd(x, left, right), lambda g: crop_bwd(g, left, right))(t)


def torch_dense(t, w, b):
    """Dense over the last axis with gradients to t, w and b through dense_fwd / dense_bwd"""
    import torch

    class Fn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, t, w, b):
            ctx.save_for_backward(t, w)
            return torch.from_numpy(dense_fwd(t.detach().numpy(), w.detach().numpy(), b.detach().numpy()))

        @staticmethod
        def backward(ctx, g):
            t, w = ctx.saved_tensors
            return tuple(torch.from_numpy(np.ascontiguousarray(v)) for v in dense_bwd(t.detach().numpy(), w.detach().numpy(), g.detach().numpy()))

    return Fn.apply(t, w, b)
