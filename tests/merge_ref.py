"""numpy definition of the Keras 2.2.4 merge layers (layers/merge.py on TensorFlow), forward and backward, as csrc/merge.hip computes them:
fp32 throughout, folded LEFT TO RIGHT as keras' _merge_function loops, one rounding per operation.

  add / sub / mul     ((x0 o x1) o x2) ...; sub takes exactly two inputs
  avg                 the left-to-right sum, then one division by float32(k)
  max / min           acc = x > acc ? x : acc (x < acc): the earlier value stays on a tie, so +-0 ties are decided too
Gradients of input i:
  add                 dy;      sub: dy, -dy;      avg: dy * float32(1 / k)
  mul                 dy * (product of x_j, j != i, left to right from the first such j)
  max / min           the whole dy where i is the FIRST input that attains the extremum, +0 elsewhere: TensorFlow's _MaximumMinimumGrad under
                      keras' chain out = K.maximum(out, x_j) gives `out` the gradient where out >= x_j, and x_j only where it is strictly larger
  concat              the slice of dy along the axis
tests/test_merge_cpu.py checks this file against torch autograd in fp64 (inputs without ties) and the tie rule against a hand-written example."""
import numpy as np

MODES = ('add', 'sub', 'mul', 'avg', 'max', 'min')
F = np.float32


def _f32(xs):
    xs = [np.asarray(x, F) for x in xs]
    assert all(x.shape == xs[0].shape for x in xs)
    return xs


def merge_fwd(mode, xs):
    xs = _f32(xs)
    assert mode in MODES and (mode != 'sub' or len(xs) == 2)
    acc = xs[0].copy()
    with np.errstate(all='ignore'):
        for x in xs[1:]:
            if mode in ('add', 'avg'):
                acc = acc + x
            elif mode == 'sub':
                acc = acc - x
            elif mode == 'mul':
                acc = acc * x
            elif mode == 'max':
                acc = np.where(x > acc, x, acc)
            else:
                acc = np.where(x < acc, x, acc)
        if mode == 'avg':
            acc = acc / F(len(xs))
    assert acc.dtype == F
    return acc


def first_extremum(mode, xs):
    """index of the first input that attains the maximum ('max') or minimum ('min'), per element"""
    xs = _f32(xs)
    acc, win = xs[0].copy(), np.zeros(xs[0].shape, np.int64)
    for j, x in enumerate(xs[1:], 1):
        better = x > acc if mode == 'max' else x < acc
        acc = np.where(better, x, acc)
        win = np.where(better, j, win)
    return win


def merge_bwd(mode, dy, xs, which):
    xs, dy = _f32(xs), np.asarray(dy, F)
    k = len(xs)
    assert mode in MODES and 0 <= which < k and (mode != 'sub' or k == 2)
    with np.errstate(all='ignore'):
        if mode == 'add':
            return dy.copy()
        if mode == 'sub':
            return dy.copy() if which == 0 else -dy
        if mode == 'avg':
            return dy * (F(1.0) / F(k))
        if mode == 'mul':
            prod = None
            for j, x in enumerate(xs):
                if j != which:
                    prod = x.copy() if prod is None else prod * x
            return dy.copy() if prod is None else dy * prod
    return np.where(first_extremum(mode, xs) == which, dy, F(0.0)).astype(F)


def _axis(axis, rank):
    """axis counts the batch axis, as in keras; 1 <= axis < rank"""
    ax = axis + rank if axis < 0 else axis
    assert 1 <= ax < rank, (axis, rank)
    return ax


def concat_fwd(xs, axis=-1):
    xs = [np.asarray(x, F) for x in xs]
    return np.concatenate(xs, axis=_axis(axis, xs[0].ndim))


def concat_bwd(dy, shapes, axis=-1):
    dy = np.asarray(dy, F)
    ax = _axis(axis, dy.ndim)
    cuts = np.cumsum([s[ax] for s in shapes])[:-1]
    parts = np.split(dy, cuts, axis=ax)
    assert [p.shape for p in parts] == [tuple(s) for s in shapes]
    return [np.ascontiguousarray(p) for p in parts]
