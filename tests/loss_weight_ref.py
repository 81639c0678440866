"""fp64 restatement of the weighted loss contract (gn_loss_pass_weighted; Keras 2.2.4 weighted_masked_objective and standardize_weights),
built on tests/loss_ref.py and written from DESIGN.md section 8f alone (no gennet_amd import):

    loss      = sum_r w_r l_r / count                      l_r: the per-row term of DESIGN.md section 8e
    dp[r, j]  = w_r / count * d l_r / d p[r, j]
    hit share = sum_r w_r hits_r / (count cols)            hits_r = #{j : rint(p[r, j]) == y[r, j]}

count is the number of non-zero weights of the GLOBAL batch (a data-parallel rank holds a part of the rows), so it is an argument.
Keras writes the loss as mean(l w / mean(w != 0)): the batch size cancels.  Negative weights count as non-zero; count = 0 gives 0 / 0."""
import numpy as np

import loss_ref as R


def row_terms(kind, p, y):
    """The per-row terms l_r of a (rows, cols) pair, vectorised over the rows (tests/test_sample_weight_cpu.py checks them against
    loss_ref.value_and_grad on one-row slices)."""
    kind = R.ALIASES.get(kind, kind)
    p, y = np.asarray(p, np.float64), np.asarray(y, np.float64)
    d = p - y
    if kind == 'binary_crossentropy':
        pc = np.clip(p, R.EPS, R.ONE_M_EPS)
        return np.mean(-(y * np.log(pc) + (1.0 - y) * np.log1p(-pc)), axis=1)
    if kind == 'mean_squared_error':
        return np.mean(d * d, axis=1)
    if kind == 'mean_absolute_error':
        return np.mean(np.abs(d), axis=1)
    if kind == 'mean_absolute_percentage_error':
        return 100.0 * np.mean(np.abs(d) / np.maximum(np.abs(y), R.EPS), axis=1)
    if kind == 'mean_squared_logarithmic_error':
        l = np.log1p(np.maximum(p, R.EPS)) - np.log1p(np.maximum(y, R.EPS))
        return np.mean(l * l, axis=1)
    if kind == 'hinge':
        return np.mean(np.maximum(1.0 - y * p, 0.0), axis=1)
    if kind == 'squared_hinge':
        return np.mean(np.maximum(1.0 - y * p, 0.0) ** 2, axis=1)
    if kind == 'logcosh':
        x = -2.0 * d
        return np.mean(d + np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x))) - np.log(2.0), axis=1)
    if kind == 'poisson':
        return np.mean(p - y * np.log(p + R.EPS), axis=1)
    if kind == 'kullback_leibler_divergence':
        yc, pc = np.clip(y, R.EPS, 1.0), np.clip(p, R.EPS, 1.0)
        return np.sum(yc * np.log(yc / pc), axis=1)
    if kind == 'categorical_crossentropy':
        q = p / np.sum(p, axis=1, keepdims=True)
        return -np.sum(y * np.log(np.clip(q, R.EPS, R.ONE_M_EPS)), axis=1)
    if kind == 'cosine_proximity':
        n_p = np.sqrt(np.maximum(np.sum(p * p, axis=1), R.COS_FLOOR))
        n_y = np.sqrt(np.maximum(np.sum(y * y, axis=1), R.COS_FLOOR))
        return -np.sum(p * y, axis=1) / (n_p * n_y)
    if kind == 'categorical_accuracy':
        return (np.argmax(p, axis=1) == np.argmax(y, axis=1)).astype(np.float64)
    raise KeyError(kind)


def row_terms_by_slices(kind, p, y):
    """The same from loss_ref.value_and_grad on one-row slices: the definition, for small shapes."""
    return np.array([R.value_and_grad(kind, p[r:r + 1], y[r:r + 1], 1)[0] for r in range(np.asarray(p).shape[0])], np.float64)


def row_hits(p, y):
    return np.sum(np.rint(np.asarray(p, np.float32)) == np.asarray(y, np.float32), axis=1).astype(np.float64)


def weighted_value_and_grad(kind, p, y, w, count):
    """(value, dp, weighted hit share, conditioning sum sum_r |w_r l_r| / count) of float32 (rows, cols) p, y and (rows,) w."""
    p64, w = np.asarray(p, np.float64), np.asarray(w, np.float64)
    rows, cols = p64.shape
    assert w.shape == (rows,)
    count = float(count)
    l = row_terms(kind, p, y)
    # a row's term depends on that row alone, so the derivative of the unweighted SUM over the rows (denom = 1) is d l_r / d p[r, j]
    g = R.value_and_grad(kind, p, y, 1)[1]
    with np.errstate(divide='ignore', invalid='ignore'):
        value = np.float64(np.sum(w * l)) / np.float64(count)
        dp = (w / np.float64(count))[:, None] * g
        share = np.float64(np.sum(w * row_hits(p, y))) / np.float64(count * cols)
        cond = np.float64(np.sum(np.abs(w * l))) / np.float64(count)
    return float(value), dp, float(share), float(cond)


def hit_conditioning(p, y, w, count):
    """sum_r |w_r| hits_r / (count cols): what the error of the weighted hit share is measured against."""
    return float(np.sum(np.abs(np.asarray(w, np.float64)) * row_hits(p, y)) / (float(count) * np.asarray(p).shape[1]))


def weights(rows, seed=0):
    """float32 sample weights: about a quarter exact zeros, about a fifth of the rest negative, magnitudes in [0.25, 4], at least one
    non-zero."""
    rng = np.random.RandomState((seed * 104729 + 7919 * rows + 13) % (2 ** 31))
    w = rng.uniform(0.25, 4.0, rows) * np.where(rng.rand(rows) < 0.2, -1.0, 1.0)
    w[rng.rand(rows) < 0.25] = 0.0
    if not np.any(w):
        w[rows // 2] = 1.5
    return np.ascontiguousarray(w, np.float32)


def keras_metric(name, p, y, w):
    """A compiled weighted metric as Keras reports it on one batch: sum_r w_r m_r / #{w != 0}."""
    w = np.asarray(w, np.float64)
    cnt = float(np.count_nonzero(w))
    if name in ('accuracy', 'acc', 'binary_accuracy'):
        return float(np.sum(w * row_hits(p, y)) / (cnt * np.asarray(p).shape[1]))
    return float(np.sum(w * row_terms(name, p, y)) / cnt)
