"""numpy fp64 definition of keras 2.2.4 layers.Dot (K.batch_dot, K.l2_normalize) and of the passes of csrc/bmm.hip, for tests/test_dot_cpu.py (which
checks it against torch.matmul autograd in fp64) and tests/test_dot_gpu.py.  Axes count the batch axis, as keras counts them; a rank-2 input is
its rank-3 view with a trailing extent of 1, as K.batch_dot expands it, and the extra axes are squeezed from the result."""
import numpy as np

L2_EPS = 1e-12


def l2norm_fwd(x, view, eps=L2_EPS):
    """(y, inv, clamped) on the (outer, P, inner) view: s = sum_p x^2, inv = 1 / sqrt(max(s, eps)), y = x * inv; clamped = s < eps"""
    outer, P, inner = view
    v = np.asarray(x, np.float64).reshape(outer, P, inner)
    s = np.einsum('opi,opi->oi', v, v)
    inv = 1.0 / np.sqrt(np.maximum(s, eps))
    return (v * inv[:, None, :]).reshape(np.shape(x)), inv, s < eps


def l2norm_bwd(dy, y, inv, clamped, view):
    """dx = inv * (dy - y * sum_p dy * y); where the sum of squares was clamped inv is a constant and dx = inv * dy"""
    outer, P, inner = view
    g = np.asarray(dy, np.float64).reshape(outer, P, inner)
    yv = np.asarray(y, np.float64).reshape(outer, P, inner)
    t = np.where(clamped, 0.0, np.einsum('opi,opi->oi', g, yv))
    return (inv[:, None, :] * (g - yv * t[:, None, :])).reshape(np.shape(dy))


def _axes(axes, ranks):
    if isinstance(axes, (int, np.integer)):
        return [axes % r for r in ranks] if axes < 0 else [int(axes)] * 2
    return [int(a) for a in axes]


def _view3(x):
    x = np.asarray(x, np.float64)
    return x.reshape(x.shape + (1,)) if x.ndim == 2 else x


def _spec(ax, free):
    """einsum subscripts of a rank-3 view contracted along `ax` with the free axis named `free`"""
    return 'bk' + free if ax == 1 else 'b' + free + 'k'


def norm_view(shape3, ax):
    B, d1, d2 = shape3
    return (B, d1, d2) if ax == 1 else (B * d1, d2, 1)


def out_shape(s1, s2, axes):
    """keras' Dot.compute_output_shape on full shapes (batch included)"""
    a1, a2 = _axes(axes, (len(s1), len(s2)))
    s1, s2 = list(s1), list(s2)
    s1.pop(a1)
    s2.pop(a2)
    s2.pop(0)
    out = s1 + s2
    return tuple(out + [1]) if len(out) == 1 else tuple(out)


def dot_fwd(x1, x2, axes, normalize=False):
    """(y, cache) of Dot(axes, normalize)([x1, x2])"""
    a1, a2 = _axes(axes, (np.ndim(x1), np.ndim(x2)))
    u, v = _view3(x1), _view3(x2)
    n1 = n2 = None
    if normalize:
        u, i1, c1 = l2norm_fwd(u, norm_view(u.shape, a1))
        v, i2, c2 = l2norm_fwd(v, norm_view(v.shape, a2))
        n1, n2 = (i1, c1), (i2, c2)
    y = np.einsum('%s,%s->bij' % (_spec(a1, 'i'), _spec(a2, 'j')), u, v)
    return y.reshape(out_shape(np.shape(x1), np.shape(x2), axes)), (u, v, a1, a2, n1, n2, np.shape(x1), np.shape(x2))


def dot_bwd(dy, cache):
    """(dx1, dx2) for the gradient dy of dot_fwd's output"""
    u, v, a1, a2, n1, n2, s1, s2 = cache
    M, N = u.shape[3 - a1], v.shape[3 - a2]
    g = np.asarray(dy, np.float64).reshape(u.shape[0], M, N)
    du = np.einsum('bij,%s->%s' % (_spec(a2, 'j'), _spec(a1, 'i')), g, v)
    dv = np.einsum('bij,%s->%s' % (_spec(a1, 'i'), _spec(a2, 'j')), g, u)
    if n1 is not None:
        du = l2norm_bwd(du, u, n1[0], n1[1], norm_view(u.shape, a1))
        dv = l2norm_bwd(dv, v, n2[0], n2[1], norm_view(v.shape, a2))
    return du.reshape(s1), dv.reshape(s2)


def bmm(a, b, trans_a=False, trans_b=False):
    """the product of ops.bmm in fp64 (int64 for integer arrays: exact)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == 'f':
        a, b = a.astype(np.float64), b.astype(np.float64)
    else:
        a, b = a.astype(np.int64), b.astype(np.int64)
    return np.einsum('%s,%s->bmn' % ('bkm' if trans_a else 'bmk', 'bnk' if trans_b else 'bkn'), a, b)
