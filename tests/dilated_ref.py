"""numpy restatement of Conv1D(dilation_rate=d, padding='same' | 'valid' | 'causal') as the library runs it: the two passes of
csrc/dilate.hip, the geometry, and the layer as split -> the undilated k-tap conv on 0 padding -> merge, forward and backward.

split and merge keep the dtype they are handed (float32 in: the bits the kernels must produce; float64 in: the layer reference); everything
else is fp64.  tests/test_dilated_cpu.py checks the layer functions against torch.nn.functional.conv1d(dilation=d) and its autograd."""
import numpy as np


def geometry(L, k, stride, padding, d=1):
    """(Lout, pad_left, pad_right) with tot = (k - 1) * d: 'valid' no padding, Lout = (L - tot - 1) // stride + 1; 'same' TensorFlow SAME on the
    effective kernel tot + 1 (stride 1: Lout = L, pad_left = tot // 2); 'causal' tot rows on the left, Lout = ceil(L / stride)."""
    tot = (k - 1) * d
    if padding == 'valid':
        return (L - tot - 1) // stride + 1, 0, 0
    if padding == 'causal':
        return -(-L // stride), tot, 0
    assert padding == 'same', padding
    Lout = -(-L // stride)
    total = max((Lout - 1) * stride + tot + 1 - L, 0)
    return Lout, total // 2, total - total // 2


def phase_rows(L, k, d, pl, pr):
    """M: rows of a phase sequence, enough for the padded input and for one window"""
    return max(-(-(L + pl + pr) // d), k)


def split(x, d, off, M):
    """x (B, L, C) -> xs (B*d, M, C): xs[b*d + p, m] = x[b, m*d + p - off] inside [0, L), +0 elsewhere; input rows beyond M rows are dropped"""
    B, L, C = x.shape
    xs = np.zeros((B * d, M, C), x.dtype)
    for b in range(B):
        for p in range(d):
            for m in range(M):
                i = m * d + p - off
                if 0 <= i < L:
                    xs[b * d + p, m] = x[b, i]
    return xs


def merge(xs, B, d, off, L):
    """xs (B*d, M, C) -> x (B, L, C): x[b, i] = xs[b*d + (i + off) % d, (i + off) // d]; the adjoint of split(x, d, off, M)"""
    Bd, M, C = xs.shape
    assert Bd == B * d and (L - 1 + off) // d < M
    x = np.empty((B, L, C), xs.dtype)
    for b in range(B):
        for i in range(L):
            x[b, i] = xs[b * d + (i + off) % d, (i + off) // d]
    return x


def act_fwd(z, act, p=0.0):
    if act == 'tanh':
        return np.tanh(z)
    if act == 'relu':
        return np.maximum(z, 0.0)
    if act == 'leaky':
        return np.where(z > 0, z, p * z)
    assert act == 'linear', act
    return z


def act_grad_from_y(y, act, p=0.0):
    if act == 'tanh':
        return 1.0 - y * y
    if act == 'relu':
        return (y > 0).astype(y.dtype)
    if act == 'leaky':
        return np.where(y > 0, 1.0, p)
    return np.ones_like(y)


def conv_valid(x, w, b, stride=1):
    """the undilated k-tap conv on 0 padding: x (B, M, Cin), w (k, Cin, Cout), b (Cout,) -> (B, (M - k) // stride + 1, Cout)"""
    k = w.shape[0]
    Lo = (x.shape[1] - k) // stride + 1
    y = np.zeros((x.shape[0], Lo, w.shape[2])) + b
    for j in range(k):
        y += x[:, j:j + (Lo - 1) * stride + 1:stride] @ w[j]
    return y


def conv_valid_bwd(x, w, dy, stride=1):
    """-> (dx, dw, db) of conv_valid"""
    k = w.shape[0]
    Lo = dy.shape[1]
    dx, dw = np.zeros_like(x), np.zeros_like(w)
    for j in range(k):
        rows = slice(j, j + (Lo - 1) * stride + 1, stride)
        dx[:, rows] += dy @ w[j].T
        dw[j] = np.einsum('bmc,bmn->cn', x[:, rows], dy)
    return dx, dw, dy.sum((0, 1))


def torch_layer(x, w, b, stride, padding, d, act='linear', p=0.0):
    """keras Conv1D on channels-last fp64 torch tensors, the oracle of both test files: explicit zero padding by geometry(), then
    torch.nn.functional.conv1d(dilation=d) without padding, then the activation"""
    import torch
    import torch.nn.functional as F
    _, pl, pr = geometry(x.shape[1], w.shape[0], stride, padding, d)
    z = F.conv1d(F.pad(x.permute(0, 2, 1), (pl, pr)), w.permute(2, 1, 0), b, stride=stride, dilation=d).permute(0, 2, 1)
    return torch.tanh(z) if act == 'tanh' else F.leaky_relu(z, p) if act == 'leaky' else torch.relu(z) if act == 'relu' else z


def layer_fwd(x, w, b, stride, padding, d, act='linear', p=0.0):
    """y (B, Lout, Cout) of the dilated layer, fp64"""
    B, L, _ = x.shape
    k = w.shape[0]
    Lout, pl, pr = geometry(L, k, stride, padding, d)
    assert Lout >= 1 and (d == 1 or stride == 1)
    xs = split(x, d, pl, phase_rows(L, k, d, pl, pr))
    ys = act_fwd(conv_valid(xs, w, b, stride), act, p)
    return merge(ys, B, d, 0, Lout)


def layer_bwd(x, w, b, dy, stride, padding, d, act='linear', p=0.0):
    """(dx, dw, db) of layer_fwd for the output gradient dy (B, Lout, Cout): the activation gradient through y in the layer's own layout, the
    phases of the result through the undilated conv's gradients, the data gradient's phases merged back behind the pl padding rows"""
    B, L, _ = x.shape
    k = w.shape[0]
    Lout, pl, pr = geometry(L, k, stride, padding, d)
    M = phase_rows(L, k, d, pl, pr)
    xs = split(x, d, pl, M)
    g = dy * act_grad_from_y(layer_fwd(x, w, b, stride, padding, d, act, p), act, p)
    dys = split(g, d, 0, (M - k) // stride + 1)
    dxs, dw, db = conv_valid_bwd(xs, w, dys, stride)
    return merge(dxs, B, d, pl, L), dw, db
