"""fp64 restatement of the Keras 2.2.4 losses and metrics (keras/losses.py, keras/metrics.py, TensorFlow backend), written from the table of
DESIGN.md section 8e alone (no gennet_amd import).  value_and_grad(kind, p, y, denom) takes (rows, cols) arrays and returns
(sum over rows of the per-row term / denom, its derivative with respect to p): the contract of gn_loss_pass.

Conventions: a clip passes gradient on its closed interval; maximum(a, 0) gives a tie to a; sign(0) = 0.  The clip bounds are the float32
numbers Keras computes: eps = float32(1e-7), and 1 - eps formed in float32.

generate(kind, rows, cols, seed) draws the float32 inputs of the parity tests, per kind inside the region where this reference is well
conditioned; bounds_ok(kind, p, y) states that region (tests/test_losses_cpu.py checks the one against the other)."""
import numpy as np

EPS = float(np.float32(1e-7))
ONE_M_EPS = float(np.float32(1.0) - np.float32(1e-7))
COS_FLOOR = 1e-12

ALIASES = {'mse': 'mean_squared_error', 'mae': 'mean_absolute_error', 'mape': 'mean_absolute_percentage_error',
           'msle': 'mean_squared_logarithmic_error', 'kld': 'kullback_leibler_divergence', 'cosine': 'cosine_proximity'}
LOSSES = ('binary_crossentropy', 'mean_squared_error', 'mean_absolute_error', 'mean_absolute_percentage_error', 'mean_squared_logarithmic_error',
          'hinge', 'squared_hinge', 'logcosh', 'poisson', 'kullback_leibler_divergence', 'categorical_crossentropy', 'cosine_proximity')
KINDS = LOSSES + ('categorical_accuracy',)
MARGIN = 1e-3           # distance the generated inputs keep from every kink and clip bound


def value_and_grad(kind, p, y, denom=None):
    kind = ALIASES.get(kind, kind)
    p = np.asarray(p, np.float64)
    y = np.asarray(y, np.float64)
    rows, cols = p.shape
    denom = float(rows if denom is None else denom)
    d = p - y
    if kind == 'binary_crossentropy':       # TF's sigmoid cross-entropy on the logit of the clipped p
        pc = np.clip(p, EPS, ONE_M_EPS)
        row = np.mean(-(y * np.log(pc) + (1.0 - y) * np.log1p(-pc)), axis=1)
        g = np.where((p >= EPS) & (p <= ONE_M_EPS), (pc - y) / (pc * (1.0 - pc)), 0.0) / cols
    elif kind == 'mean_squared_error':
        row = np.mean(d * d, axis=1)
        g = 2.0 * d / cols
    elif kind == 'mean_absolute_error':
        row = np.mean(np.abs(d), axis=1)
        g = np.sign(d) / cols
    elif kind == 'mean_absolute_percentage_error':
        m = np.maximum(np.abs(y), EPS)
        row = 100.0 * np.mean(np.abs(d) / m, axis=1)
        g = 100.0 * np.sign(d) / m / cols
    elif kind == 'mean_squared_logarithmic_error':
        pm, ym = np.maximum(p, EPS), np.maximum(y, EPS)
        l = np.log1p(pm) - np.log1p(ym)
        row = np.mean(l * l, axis=1)
        g = np.where(p >= EPS, 2.0 * l / (pm + 1.0), 0.0) / cols
    elif kind == 'hinge':
        m = 1.0 - y * p
        row = np.mean(np.maximum(m, 0.0), axis=1)
        g = np.where(m >= 0.0, -y, 0.0) / cols
    elif kind == 'squared_hinge':
        h = np.maximum(1.0 - y * p, 0.0)
        row = np.mean(h * h, axis=1)
        g = -2.0 * y * h / cols
    elif kind == 'logcosh':                 # d + softplus(-2d) - log 2, softplus(x) = max(x, 0) + log1p(exp(-|x|))
        x = -2.0 * d
        row = np.mean(d + np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x))) - np.log(2.0), axis=1)
        g = np.tanh(d) / cols
    elif kind == 'poisson':
        row = np.mean(p - y * np.log(p + EPS), axis=1)
        g = (1.0 - y / (p + EPS)) / cols
    elif kind == 'kullback_leibler_divergence':
        yc, pc = np.clip(y, EPS, 1.0), np.clip(p, EPS, 1.0)
        row = np.sum(yc * np.log(yc / pc), axis=1)
        g = np.where((p >= EPS) & (p <= 1.0), -yc / pc, 0.0)
    elif kind == 'categorical_crossentropy':
        s = np.sum(p, axis=1, keepdims=True)
        q = p / s
        qc = np.clip(q, EPS, ONE_M_EPS)
        row = -np.sum(y * np.log(qc), axis=1)
        gj = np.where((q >= EPS) & (q <= ONE_M_EPS), -y / qc, 0.0)
        g = (gj - np.sum(gj * q, axis=1, keepdims=True)) / s
    elif kind == 'cosine_proximity':
        spp, syy = np.sum(p * p, axis=1, keepdims=True), np.sum(y * y, axis=1, keepdims=True)
        n_p, n_y = np.sqrt(np.maximum(spp, COS_FLOOR)), np.sqrt(np.maximum(syy, COS_FLOOR))
        ph, yh = p / n_p, y / n_y
        c = np.sum(ph * yh, axis=1, keepdims=True)
        row = -c[:, 0]
        g = -(yh - np.where(spp >= COS_FLOOR, c, 0.0) * ph) / n_p
    elif kind == 'categorical_accuracy':
        row = (np.argmax(p, axis=1) == np.argmax(y, axis=1)).astype(np.float64)      # numpy's argmax: the first maximum
        g = np.zeros_like(p)
    else:
        raise KeyError(kind)
    return float(np.sum(row) / denom), g / denom


def torch_value(kind, p, y, denom):
    """The table of DESIGN.md section 8e written with torch ops (autograd supplies the derivative)."""
    import torch
    kind = ALIASES.get(kind, kind)
    eps, hi = EPS, ONE_M_EPS
    d = p - y
    if kind == 'binary_crossentropy':
        pc = p.clamp(eps, hi)
        z = torch.log(pc / (1 - pc))
        row = (z.clamp(min=0) - z * y + torch.log1p(torch.exp(-z.abs()))).mean(1)
    elif kind == 'mean_squared_error':
        row = (d * d).mean(1)
    elif kind == 'mean_absolute_error':
        row = d.abs().mean(1)
    elif kind == 'mean_absolute_percentage_error':
        row = 100 * (d.abs() / y.abs().clamp(min=eps)).mean(1)
    elif kind == 'mean_squared_logarithmic_error':
        row = ((torch.log(p.clamp(min=eps) + 1) - torch.log(y.clamp(min=eps) + 1)) ** 2).mean(1)
    elif kind == 'hinge':
        row = (1 - y * p).clamp(min=0).mean(1)
    elif kind == 'squared_hinge':
        row = ((1 - y * p).clamp(min=0) ** 2).mean(1)
    elif kind == 'logcosh':
        row = (d + torch.nn.functional.softplus(-2 * d) - np.log(2.0)).mean(1)
    elif kind == 'poisson':
        row = (p - y * torch.log(p + eps)).mean(1)
    elif kind == 'kullback_leibler_divergence':
        yc, pc = y.clamp(eps, 1), p.clamp(eps, 1)
        row = (yc * torch.log(yc / pc)).sum(1)
    elif kind == 'categorical_crossentropy':
        q = p / p.sum(1, keepdim=True)
        row = -(y * torch.log(q.clamp(eps, hi))).sum(1)
    elif kind == 'cosine_proximity':
        ph = p / torch.sqrt((p * p).sum(1, keepdim=True).clamp(min=COS_FLOOR))
        yh = y / torch.sqrt((y * y).sum(1, keepdim=True).clamp(min=COS_FLOOR))
        row = -(ph * yh).sum(1)
    else:
        raise KeyError(kind)
    return row.sum() / denom


def hits(p, y):
    """The binary hit count of every loss call: #elements with round-half-even(p) == y, on the float32 values."""
    return int(np.sum(np.rint(np.asarray(p, np.float32)) == np.asarray(y, np.float32)))


def metric(kind, p, y, denom=None):
    """A compiled metric as Keras reports it: the loss form's value ('accuracy': hits / element count)."""
    if kind in ('accuracy', 'acc', 'binary_accuracy'):
        rows = np.asarray(p).shape[0]
        return hits(p, y) / (float(rows if denom is None else denom) * np.asarray(p).shape[1])
    return value_and_grad(kind, p, y, denom)[0]


# ------------------------------------------------------------------------------------------------------------- test inputs
def generate(kind, rows, cols, seed=0):
    """float32 (p, y) of shape (rows, cols) inside the well-conditioned region of `kind` (bounds_ok)."""
    kind = ALIASES.get(kind, kind)
    rng = np.random.RandomState((seed * 7919 + 104729 * KINDS.index(kind) + rows * 31 + cols) % (2 ** 31))
    shape = (rows, cols)

    def away(lo, hi):                        # y, then p at a distance of 0.25 .. 1.25 from it on either side
        y = rng.uniform(lo, hi, shape)
        return y + rng.choice([-1.0, 1.0], shape) * rng.uniform(0.25, 1.25, shape), y

    if kind in ('binary_crossentropy', 'kullback_leibler_divergence', 'poisson', 'categorical_crossentropy'):
        p, y = rng.uniform(0.05, 0.95, shape), rng.uniform(0.05, 0.95, shape)
        if kind == 'binary_crossentropy':
            y = rng.randint(0, 2, shape).astype(np.float64)
        if kind == 'categorical_crossentropy':                       # one-hot targets; q = p / sum(p) stays inside [eps, 1 - eps] by a wide margin
            y = np.eye(cols)[rng.randint(0, cols, rows)]
            if cols == 1:
                p = rng.uniform(0.05, 0.95, shape)                   # q == 1 > 1 - eps: the clipped branch, gradient 0
    elif kind in ('hinge', 'squared_hinge'):
        y = rng.choice([-1.0, 1.0], shape)
        m = rng.choice([-1.0, 1.0], shape) * rng.uniform(0.01, 1.5, shape)          # 1 - y p, at least 1e-2 from the kink at 0
        p = (1.0 - m) * y
    elif kind in ('logcosh', 'mean_absolute_error', 'mean_squared_error'):
        p, y = away(-1.0, 1.0)
    elif kind == 'mean_absolute_percentage_error':
        p, y = away(0.5, 2.0)
        y = y * rng.choice([-1.0, 1.0], shape)
        p = p * np.sign(y)
    elif kind == 'mean_squared_logarithmic_error':
        y = rng.uniform(0.1, 2.0, shape)
        p = y + rng.uniform(0.25, 1.25, shape)
    elif kind in ('cosine_proximity', 'categorical_accuracy'):
        p, y = rng.uniform(-1.0, 1.0, shape), rng.uniform(-1.0, 1.0, shape)
        if kind == 'categorical_accuracy':                            # sixteenths: maxima tie, so the FIRST one decides
            p, y = np.round(p * 16) / 16, np.round(y * 16) / 16
        if kind == 'cosine_proximity':                                # row norms of at least 0.1: one entry of every row is pushed out
            p[:, 0] = np.where(np.abs(p[:, 0]) < 0.2, 0.5, p[:, 0])
            y[:, 0] = np.where(np.abs(y[:, 0]) < 0.2, -0.5, y[:, 0])
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(p, np.float32), np.ascontiguousarray(y, np.float32)


def bounds_ok(kind, p, y):
    """The region the parity inputs must lie in (float32 arrays as generated)."""
    kind = ALIASES.get(kind, kind)
    p, y = np.asarray(p, np.float64), np.asarray(y, np.float64)
    d = np.abs(p - y)
    if kind in ('binary_crossentropy', 'kullback_leibler_divergence', 'poisson', 'categorical_crossentropy'):
        ok = p.min() >= 0.05 - 1e-6 and p.max() <= 0.95 + 1e-6
        if kind in ('kullback_leibler_divergence', 'poisson'):
            ok = ok and y.min() >= 0.05 - 1e-6 and y.max() <= 0.95 + 1e-6
        if kind == 'categorical_crossentropy' and p.shape[1] > 1:
            q = p / p.sum(axis=1, keepdims=True)
            ok = ok and q.min() >= EPS + MARGIN * 1e-3 and q.max() <= ONE_M_EPS - MARGIN
        return bool(ok)
    if kind in ('hinge', 'squared_hinge'):
        return bool(np.all(np.abs(y) == 1.0) and np.abs(1.0 - y * p).min() >= MARGIN)
    if kind in ('logcosh', 'mean_absolute_error', 'mean_absolute_percentage_error'):
        ok = d.min() >= 0.25 - 1e-6
        if kind == 'mean_absolute_percentage_error':
            ok = ok and np.abs(y).min() >= 0.5 - 1e-6
        return bool(ok)
    if kind == 'mean_squared_logarithmic_error':
        return bool(min(p.min(), y.min()) >= EPS + MARGIN)
    if kind == 'cosine_proximity':
        return bool(min(np.sqrt((p * p).sum(axis=1)).min(), np.sqrt((y * y).sum(axis=1)).min()) >= 0.1)
    return True


# one element, a block edge, d_model's head, a short row, a row longer than one sweep, a row longer than a block's share, several blocks with a
# ragged tail
GPU_SHAPES = ((1, 1), (257, 1), (300, 2), (5, 3), (3, 1030), (2, 70001), (100003, 1))


# the exact-tie inputs, shared with the device test: (kind, p, y, expected derivative before / denom)
def tie_cases():
    eps = np.float32(1e-7)
    below = np.nextafter(eps, np.float32(0))
    l = np.log1p(np.float64(eps)) - np.log1p(0.5)
    return [
        ('hinge', [[1.0, 1.0]], [[1.0, 1.0]], [[-0.5, -0.5]]),                        # 1 - y p == 0: maximum(a, 0) gives the tie to a, -y / cols
        ('mean_absolute_error', [[0.25, 1.5]], [[0.25, 1.0]], [[0.0, 0.5]]),         # sign(0) = 0
        ('mean_squared_logarithmic_error', [[eps, below]], [[0.5, 0.5]], [[2 * l / (1.0 + np.float64(eps)) / 2, 0.0]]),   # closed clip: p == eps passes
    ]
