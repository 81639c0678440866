"""numpy fp64 definition of keras layers.LayerNormalization over a trailing block of axes (csrc/layernorm.hip), forward and all
gradients, with gamma (scale) and beta (center) optional:
    mean = mean_c x,  var = mean_c (x - mean)^2 (biased),  rstd = 1 / sqrt(var + eps),  xhat = (x - mean) rstd,  y = xhat gamma + beta
    g = dy gamma,  dx = rstd (g - mean_c g - xhat mean_c (g xhat)),  dgamma = sum_rows dy xhat,  dbeta = sum_rows dy
`naxes` is the number of trailing axes normalised; gamma and beta have their shape.  Also the rounding floors of the parity tests
(tests/test_layernorm_gpu.py) and the model-level comparison against torch fp64 that those tests share."""
import numpy as np


def _split(x, naxes):
    x = np.asarray(x, np.float64)
    shape = x.shape[x.ndim - naxes:]
    return x.reshape(-1, int(np.prod(shape))), shape


def forward(x, gamma=None, beta=None, eps=1e-3, naxes=1):
    """-> (y like x, mean (rows,), rstd (rows,), xhat (rows, N))"""
    x2, shape = _split(x, naxes)
    mean = x2.mean(1)
    var = ((x2 - mean[:, None]) ** 2).mean(1)
    rstd = 1.0 / np.sqrt(var + eps)
    xhat = (x2 - mean[:, None]) * rstd[:, None]
    y = xhat.copy()
    if gamma is not None:
        y = y * np.asarray(gamma, np.float64).reshape(1, -1)
    if beta is not None:
        y = y + np.asarray(beta, np.float64).reshape(1, -1)
    return y.reshape(np.shape(x)), mean, rstd, xhat


def backward(x, dy, gamma=None, eps=1e-3, naxes=1):
    """-> dict dx (like x), dgamma, dbeta (the shape of the normalised axes)"""
    x2, shape = _split(x, naxes)
    dy2, _ = _split(dy, naxes)
    _, _, rstd, xhat = forward(x, None, None, eps, naxes)
    g = dy2 if gamma is None else dy2 * np.asarray(gamma, np.float64).reshape(1, -1)
    dx = rstd[:, None] * (g - g.mean(1, keepdims=True) - xhat * (g * xhat).mean(1, keepdims=True))
    return dict(dx=dx.reshape(np.shape(x)), dgamma=(dy2 * xhat).sum(0).reshape(shape), dbeta=dy2.sum(0).reshape(shape))


def forward_loops(x, gamma, beta, eps, naxes):
    """the same forward, element by element"""
    x2, shape = _split(x, naxes)
    n = x2.shape[1]
    g = np.ones(n) if gamma is None else np.asarray(gamma, np.float64).reshape(-1)
    b = np.zeros(n) if beta is None else np.asarray(beta, np.float64).reshape(-1)
    y = np.zeros_like(x2)
    for r in range(x2.shape[0]):
        mean = sum(x2[r, c] for c in range(n)) / n
        var = sum((x2[r, c] - mean) ** 2 for c in range(n)) / n
        for c in range(n):
            y[r, c] = (x2[r, c] - mean) / np.sqrt(var + eps) * g[c] + b[c]
    return y.reshape(np.shape(x))


def floors(x, dy, gamma, eps, naxes=1):
    """The rounding floor of the INPUTS, per tensor: a row at offset mu loses |mu| / sigma ulps in x - mean whatever the implementation does.
    With u = 2^-24, kappa_r = (|mean_r| + max_c |x_r|) rstd_r and X = max(1, max |xhat|):
        y: max_r u kappa_r max|gamma| X      dx: max_r 2 u kappa_r rstd_r max_c |dy gamma| X      dgamma: max_c sum_r u kappa_r |dy|      dbeta: 0"""
    u = 2.0 ** -24
    x2, _ = _split(x, naxes)
    dy2, _ = _split(dy, naxes)
    _, mean, rstd, xhat = forward(x, None, None, eps, naxes)
    g = np.ones(x2.shape[1]) if gamma is None else np.asarray(gamma, np.float64).reshape(-1)
    kappa = (np.abs(mean) + np.abs(x2).max(1)) * rstd
    X = max(1.0, float(np.abs(xhat).max()))
    return dict(y=float((u * kappa * np.abs(g).max() * X).max()),
                dx=float((2 * u * kappa * rstd * np.abs(dy2 * g[None, :]).max(1) * X).max()),
                dgamma=float((u * kappa[:, None] * np.abs(dy2)).sum(0).max()),
                dbeta=0.0)


# ---------------------------------------------------------------------------------------------------------------------
# models against torch fp64 autograd: the logic and bounds of tests/test_attention_gpu.py's train_and_compare, copied as they stand
# ---------------------------------------------------------------------------------------------------------------------
LR = 0.05


def rel(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-30)


def torch_params(layers):
    import torch
    return dict((l.name, [torch.tensor(w.astype(np.float64), requires_grad=True) for w in l.get_weights()]) for l in layers if l.weights)


def train_and_compare(model, ref_forward, xs, t, steps=3, what='', frozen=(), penalty=None):
    """predict, then `steps` SGD train_on_batch steps, against torch fp64 stepping the same way.  frozen: layers whose weights torch does not
    step either (their gradient is not compared: the model forms none); penalty(P): a regularization term added to torch's loss."""
    import torch
    from gennet_amd.engine import SGD
    model.compile(optimizer=SGD(lr=LR), loss='mean_squared_error')
    layers = [l for l in model.layers if l.weights]
    P = torch_params(layers)
    xt = [torch.tensor(x.astype(np.float64)) for x in xs]
    tt = torch.tensor(t.astype(np.float64))
    feed = xs if len(xs) > 1 else xs[0]
    y = model.predict(feed, batch_size=len(t))
    with torch.no_grad():
        y_ref = ref_forward(P, *xt).numpy()
    print(what, 'predict err %.3g' % rel(y, y_ref))
    assert rel(y, y_ref) < 1e-5
    losses = []
    for step in range(steps):
        for ts in P.values():
            for v in ts:
                v.grad = None
        loss_ref = ((ref_forward(P, *xt) - tt) ** 2).mean()
        if penalty is not None:
            loss_ref = loss_ref + penalty(P)
        loss_ref.backward()
        res = model.train_on_batch(feed, t)
        print(what, 'step', step, 'loss', res[0], float(loss_ref.detach()))
        assert abs(res[0] - float(loss_ref.detach())) <= 1e-6 * abs(float(loss_ref.detach()))
        losses.append(float(loss_ref.detach()))
        g_floor = 1e-3 * max(float(v.grad.abs().max()) for ts in P.values() for v in ts)
        for l in layers:
            if l in frozen:
                continue
            for p, ref in zip(l.params, P[l.name]):
                g_ref = ref.grad.numpy()
                gerr = np.abs(p.grad.detach().cpu().numpy().reshape(g_ref.shape) - g_ref).max() / max(np.abs(g_ref).max(), g_floor)
                with torch.no_grad():
                    ref -= LR * ref.grad
                w_ref = ref.detach().numpy()
                werr = np.abs(p.numpy().astype(np.float64) - w_ref).max() / max(np.abs(w_ref).max(), 1e-3)
                print(what, step, l.name, p.name, 'grad err %.3g weight err %.3g' % (gerr, werr))
                assert gerr < 1e-4 and werr < 1e-4, (step, l.name, p.name, gerr, werr)
    assert len(set(losses)) == steps                                       # the steps differ
    return P
