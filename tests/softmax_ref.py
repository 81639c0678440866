"""numpy fp64 definition of the softmax passes of csrc/softmax.hip on the (outer, P, inner) view: element (o, p, i) of the flat tensor sits at
(o*P + p)*inner + i and the softmax runs along p.  Inputs are taken as they are (fp32 arrays are widened exactly), every operation is fp64.
Checked against torch.softmax and torch fp64 autograd in tests/test_softmax_cpu.py; the GPU tests compare the kernels with these two functions."""
import numpy as np


def view_of(shape, axis):
    """(outer, P, inner) of a softmax along `axis` (>= 0, or negative as numpy counts) of a tensor of `shape`."""
    axis = axis % len(shape)
    return (int(np.prod(shape[:axis], dtype=np.int64)), int(shape[axis]), int(np.prod(shape[axis + 1:], dtype=np.int64)))


def softmax_fwd(x, view):
    """-> (y, m, x - m) in fp64, each in x's shape: m the maximum of the element's own column, broadcast"""
    outer, P, inner = view
    x3 = np.asarray(x, np.float64).reshape(outer, P, inner)
    m = x3.max(axis=1, keepdims=True)
    with np.errstate(over='ignore'):
        d = x3 - m                          # -inf where +-3e38 meet: exp gives 0, as the limit does
    e = np.exp(d)
    y = e / e.sum(axis=1, keepdims=True)
    return y.reshape(np.shape(x)), np.broadcast_to(m, x3.shape).reshape(np.shape(x)), d.reshape(np.shape(x))


def softmax_bwd(dy, y, view):
    """-> (dx, sum_p |dy * y| broadcast) in fp64: dx = y * (dy - sum_p dy * y), from the output y as given"""
    outer, P, inner = view
    g = np.asarray(dy, np.float64).reshape(outer, P, inner)
    y3 = np.asarray(y, np.float64).reshape(outer, P, inner)
    t = (g * y3).sum(axis=1, keepdims=True)
    mag = np.abs(g * y3).sum(axis=1, keepdims=True)
    return (y3 * (g - t)).reshape(np.shape(dy)), np.broadcast_to(mag, g.shape).reshape(np.shape(dy))
