"""keras.layers.SeparableConv1D in numpy: the definition the HIP kernels of csrc/depthwise.hip are held against.  Run in fp64 (the default) it is
the reference; dtype=np.float32 gives a restatement in the kernels' precision.  tests/test_sepconv_cpu.py checks it against torch (F.pad +
F.conv1d(groups=C) + a 1 x 1 conv, and autograd for the three gradients).

Channels-last: x (B, L, C); depthwise kernel w (k, C, dm); t / dt (B, Lout, C dm) with output channel c dm + m (tf.nn.depthwise_conv2d's order);
pointwise kernel (1, C dm, filters); bias (filters)."""
import numpy as np


# (B, L, C, k, stride, dilation, dm, padding): the kernel shapes of tests/test_sepconv_gpu.py, which says what they straddle; the geometry walk of
# tests/test_sepconv_cpu.py forms every index of the three kernels over the same list
SHAPES = [
    (1, 1, 1, 1, 1, 1, 1, 'valid'), (3, 2, 3, 2, 1, 1, 2, 'same'), (17, 7, 4, 40, 1, 1, 1, 'same'), (1, 7, 5, 3, 2, 1, 3, 'same'),
    (3, 33, 8, 5, 1, 1, 1, 'same'), (1, 130, 8, 3, 2, 1, 1, 'valid'), (17, 33, 67, 3, 3, 1, 1, 'same'), (17, 257, 260, 2, 1, 2, 3, 'same'),
    (3, 130, 4, 16, 1, 1, 2, 'valid'), (1, 33, 1, 16, 1, 2, 1, 'same'), (3, 257, 3, 5, 2, 1, 1, 'valid'), (17, 2, 260, 1, 1, 1, 3, 'valid'),
    (1, 130, 5, 2, 3, 1, 2, 'valid'), (3, 7, 8, 3, 1, 5, 2, 'same'), (1, 33, 4, 5, 1, 5, 3, 'valid'), (17, 130, 1, 3, 2, 1, 3, 'same'),
    (3, 1, 67, 1, 1, 1, 1, 'same'), (1, 257, 8, 40, 1, 1, 1, 'valid'), (17, 257, 5, 16, 1, 1, 1, 'same'), (3, 33, 260, 2, 2, 1, 1, 'same'),
    (1, 2, 4, 2, 1, 1, 1, 'valid'), (3, 130, 67, 5, 3, 1, 2, 'valid'), (17, 7, 3, 3, 2, 2, 1, 'valid'), (1, 257, 1, 3, 1, 1, 2, 'same'),
]
IDS = ['b%d-l%d-c%d-k%d-s%d-d%d-m%d-%s' % s for s in SHAPES]


def geometry(L, k, stride, padding, dilation=1):
    """(Lout, pad_left, pad_right) of TF's padding rule on the effective window (k - 1) dilation + 1.  'same': Lout = ceil(L / stride), the total
    pad max((Lout - 1) stride + window - L, 0) with its floor half on the left (asymmetric for even windows and for strides)."""
    ke = (k - 1) * dilation + 1
    if padding == 'valid':
        return (L - ke) // stride + 1, 0, 0
    assert padding == 'same', padding
    Lout = -(-L // stride)
    total = max((Lout - 1) * stride + ke - L, 0)
    return Lout, total // 2, total - total // 2


def _taps(L, k, stride, padding, dilation):
    """per tap t: (the output rows l whose input row l stride - pad_left + t dilation lies inside [0, L), those input rows)"""
    Lout, pl, _ = geometry(L, k, stride, padding, dilation)
    l = np.arange(max(Lout, 0))
    for t in range(k):
        p = l * stride - pl + t * dilation
        ok = (p >= 0) & (p < L)
        yield t, l[ok], p[ok]


def dw_fwd(x, w, stride=1, padding='valid', dilation=1, dtype=np.float64):
    x, w = np.asarray(x, dtype), np.asarray(w, dtype)
    (B, L, C), (k, _, dm) = x.shape, w.shape
    y = np.zeros((B, geometry(L, k, stride, padding, dilation)[0], C * dm), dtype)
    for t, l, p in _taps(L, k, stride, padding, dilation):
        y[:, l] += (x[:, p, :, None] * w[t][None, None]).reshape(B, len(l), C * dm)
    return y


def dw_dgrad(dy, w, L, stride=1, padding='valid', dilation=1, dtype=np.float64):
    dy, w = np.asarray(dy, dtype), np.asarray(w, dtype)
    k, C, dm = w.shape
    B = dy.shape[0]
    dx = np.zeros((B, L, C), dtype)
    for t, l, p in _taps(L, k, stride, padding, dilation):              # the rows p of one tap are distinct
        dx[:, p] += (dy[:, l].reshape(B, len(l), C, dm) * w[t][None, None]).sum(-1)
    return dx


def dw_wgrad(x, dy, k, stride=1, padding='valid', dilation=1, dtype=np.float64):
    x, dy = np.asarray(x, dtype), np.asarray(dy, dtype)
    B, L, C = x.shape
    dm = dy.shape[2] // C
    dw = np.zeros((k, C, dm), dtype)
    for t, l, p in _taps(L, k, stride, padding, dilation):
        dw[t] = np.einsum('bnc,bncm->cm', x[:, p], dy[:, l].reshape(B, len(l), C, dm))
    return dw


def dgrad_terms(L, k, stride, padding, dilation, dm):
    """the largest number of (tap, m) pairs any dx element sums"""
    n = np.zeros(L, np.int64)
    for _, _, p in _taps(L, k, stride, padding, dilation):
        n[p] += dm
    return int(n.max()) if L else 0


ACTIVATIONS = {
    'linear': lambda z: z, None: lambda z: z,
    'relu': lambda z: np.maximum(z, 0),
    'tanh': np.tanh,
    'sigmoid': lambda z: 1 / (1 + np.exp(-z)),
    'softmax': lambda z: np.exp(z - z.max(-1, keepdims=True)) / np.exp(z - z.max(-1, keepdims=True)).sum(-1, keepdims=True),
}


def layer(x, depthwise_kernel, pointwise_kernel, bias, stride=1, padding='valid', dilation=1, activation=None, dtype=np.float64):
    t = dw_fwd(x, depthwise_kernel, stride, padding, dilation, dtype)
    return ACTIVATIONS[activation](t @ np.asarray(pointwise_kernel, dtype)[0] + np.asarray(bias, dtype))


def torch_forward(x, depthwise_kernel, pointwise_kernel, bias, stride=1, padding='valid', dilation=1, activation=None):
    """the layer on torch tensors, differentiable: F.pad + F.conv1d(groups=C) + a 1 x 1 F.conv1d in torch's channels-first layout"""
    import torch
    import torch.nn.functional as F
    k, C, dm = depthwise_kernel.shape
    _, pl, pr = geometry(x.shape[1], k, stride, padding, dilation)
    xc = F.pad(x.permute(0, 2, 1), (pl, pr))
    t = F.conv1d(xc, depthwise_kernel.permute(1, 2, 0).reshape(C * dm, 1, k), stride=stride, dilation=dilation, groups=C)
    z = F.conv1d(t, pointwise_kernel.permute(2, 1, 0), bias).permute(0, 2, 1)
    act = {'linear': lambda v: v, None: lambda v: v, 'relu': torch.relu, 'tanh': torch.tanh, 'sigmoid': torch.sigmoid,
           'softmax': lambda v: torch.softmax(v, -1)}[activation]
    return act(z)
