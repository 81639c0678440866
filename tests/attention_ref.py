"""fp64 numpy definition of keras layers.Attention (tf.keras 2.x layers/dense_attention.py) and of all its gradients, the reference of
tests/test_attention_cpu.py (which checks it against a plain triple loop and against torch autograd) and tests/test_attention_gpu.py.

  s[b, i, j] = scale * sum_c q[b, i, c] k[b, j, c];   causal: entry (i, j) takes part iff j <= i;   p = softmax_j(s);   out = p . v
  delta[i] = sum_c dout[i, c] out[i, c];  dv = p^T dout;  dp = dout v^T;  ds = p (dp - delta);  dq = scale ds k;  dk = scale ds^T q;
  dscale = sum ds (q k^T)            (no division by scale: the unscaled scores are a factor of their own)"""
import numpy as np


def mask(Tq, Tk, causal):
    return np.tril(np.ones((Tq, Tk), bool)) if causal else np.ones((Tq, Tk), bool)


def forward(q, k, v, scale=1.0, causal=False):
    """-> (out, lse, p) in fp64"""
    q, k, v = (np.asarray(t, np.float64) for t in (q, k, v))
    s = float(scale) * np.einsum('bic,bjc->bij', q, k)
    s = np.where(mask(q.shape[1], k.shape[1], causal)[None], s, -np.inf)
    m = s.max(-1, keepdims=True)
    e = np.exp(s - m)
    l = e.sum(-1, keepdims=True)
    p = e / l
    return np.einsum('bij,bjc->bic', p, v), (m + np.log(l))[..., 0], p


def backward(q, k, v, dout, scale=1.0, causal=False):
    """-> dict(dq, dk, dv, dscale, dscale_rows) in fp64"""
    q, k, v, dout = (np.asarray(t, np.float64) for t in (q, k, v, dout))
    out, _, p = forward(q, k, v, scale, causal)
    delta = (dout * out).sum(-1, keepdims=True)
    dp = np.einsum('bic,bjc->bij', dout, v)
    ds = p * (dp - delta)
    raw = np.einsum('bic,bjc->bij', q, k)
    rows = (ds * raw).sum(-1)
    return dict(dq=float(scale) * np.einsum('bij,bjc->bic', ds, k), dk=float(scale) * np.einsum('bij,bic->bjc', ds, q), dv=np.einsum('bij,bic->bjc', p, dout),
                dscale=rows.sum(), dscale_rows=rows.reshape(-1))


def forward_loops(q, k, v, scale=1.0, causal=False):
    """the definition as three plain loops (tiny shapes only)"""
    B, Tq, d = q.shape
    Tk, dv = v.shape[1], v.shape[2]
    out = np.zeros((B, Tq, dv))
    for b in range(B):
        for i in range(Tq):
            js = [j for j in range(Tk) if not causal or j <= i]
            s = [scale * sum(float(q[b, i, c]) * float(k[b, j, c]) for c in range(d)) for j in js]
            mx = max(s)
            w = [np.exp(x - mx) for x in s]
            for c in range(dv):
                out[b, i, c] = sum(wj * float(v[b, j, c]) for wj, j in zip(w, js)) / sum(w)
    return out
