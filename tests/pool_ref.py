"""The definition of the pooling layers in plain numpy fp64 (loops over windows): what gennet_amd/csrc/pooling.hip is tested against.

Keras 2.2.4 on TensorFlow, channels last.  Windowed, x (B, H, W, C):
  'valid'  n_out = (n - p) // s + 1, no pad; the cells behind the last full window are dropped and get zero gradient
  'same'   n_out = ceil(n / s), total pad max((n_out - 1) s + p - n, 0), its floor half in front: the odd cell goes at the end
  max      padded cells never win; the gradient goes to the FIRST maximum of the window in row-major (h, w) order; overlapping windows add
  avg      the divisor is the number of in-bounds cells of the window; the gradient is dy / count summed over the covering windows
Global, x (B, P, C) -> (B, C): the mean over P with gradient dy / P; the maximum with gradient dy / n_ties at EVERY position equal to it
(tf.reduce_max), not the first-maximum rule."""
import numpy as np


def pool_geometry(n, p, s, padding):
    """(n_out, pad_before)"""
    if padding == 'valid':
        if n < p:
            raise ValueError('pool %d on %d cells' % (p, n))
        return (n - p) // s + 1, 0
    assert padding == 'same'
    n_out = -(-n // s)
    return n_out, max((n_out - 1) * s + p - n, 0) // 2


def _windows(H, W, pool, strides, padding):
    (Ho, pt), (Wo, pl) = pool_geometry(H, pool[0], strides[0], padding), pool_geometry(W, pool[1], strides[1], padding)
    for ho in range(Ho):
        h0 = ho * strides[0] - pt
        for wo in range(Wo):
            w0 = wo * strides[1] - pl
            yield ho, wo, max(h0, 0), min(h0 + pool[0], H), max(w0, 0), min(w0 + pool[1], W)


def out_shape(x_shape, pool, strides, padding):
    B, H, W, C = x_shape
    return (B, pool_geometry(H, pool[0], strides[0], padding)[0], pool_geometry(W, pool[1], strides[1], padding)[0], C)


def pool2d_fwd(mode, x, pool, strides, padding):
    x = np.asarray(x, np.float64)
    B, H, W, C = x.shape
    y = np.empty(out_shape(x.shape, pool, strides, padding))
    for ho, wo, hs, he, ws, we in _windows(H, W, pool, strides, padding):
        win = x[:, hs:he, ws:we, :].reshape(B, -1, C)
        y[:, ho, wo, :] = win.max(1) if mode == 'max' else win.sum(1) / win.shape[1]
    return y


def pool2d_bwd(mode, dy, x, pool, strides, padding):
    """x: the forward's input (its shape alone matters for 'avg')"""
    x, dy = np.asarray(x, np.float64), np.asarray(dy, np.float64)
    B, H, W, C = x.shape
    dx = np.zeros(x.shape)
    bi, ci = np.meshgrid(np.arange(B), np.arange(C), indexing='ij')
    for ho, wo, hs, he, ws, we in _windows(H, W, pool, strides, padding):
        nw = we - ws
        if mode == 'avg':
            dx[:, hs:he, ws:we, :] += dy[:, ho:ho + 1, wo:wo + 1, :] / ((he - hs) * nw)
        else:
            k = x[:, hs:he, ws:we, :].reshape(B, -1, C).argmax(1)          # numpy's argmax: the first maximum in row-major order
            np.add.at(dx, (bi, hs + k // nw, ws + k % nw, ci), dy[:, ho, wo, :])
    return dx


def covering_windows(x_shape, pool, strides, padding):
    """the largest number of windows that cover one cell"""
    _, H, W, _ = x_shape
    n = np.zeros((H, W), np.int64)
    for _, _, hs, he, ws, we in _windows(H, W, pool, strides, padding):
        n[hs:he, ws:we] += 1
    return int(n.max())


def global_fwd(mode, x):
    x = np.asarray(x, np.float64)
    return x.max(1) if mode == 'max' else x.mean(1)


def global_bwd(mode, dy, x):
    x, dy = np.asarray(x, np.float64), np.asarray(dy, np.float64)
    if mode == 'avg':
        return np.broadcast_to(dy[:, None, :] / x.shape[1], x.shape).copy()
    ties = x == x.max(1, keepdims=True)
    return ties * (dy / ties.sum(1))[:, None, :]
