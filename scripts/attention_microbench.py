#!/usr/bin/env python
"""Time keras layers.Attention's arithmetic over (B, T, d) with Tq = Tk = T and dv = d -- the forward in the training phase (gn_attention_fwd writing
out and lse) and forward + backward (gn_attention_bwd: delta, dK / dV, dQ and the scale partials) -- against two yardsticks in the same process:
  * composed  the path the README offered before: ops.bmm (q . k^T) -> ops.softmax_fwd -> ops.bmm (p . v), and backward two products for dv and dp,
              ops.softmax_bwd, two products for dq and dk; it writes and re-reads (B, T, T) tensors (non-causal only: it has no mask);
  * sdpa      torch.nn.functional.scaled_dot_product_attention in fp32 (scale = 1, is_causal as asked), its backward through autograd.
A sample is REPS launches between two device events; samples of the three paths alternate; 3 warm-up samples, then the median of 11.  Reported: ms,
algorithmic TFLOP/s (4 B T^2 d forward, 2.5 times that more for the backward's five products; half of both under causal), the share of the 157.3 TFLOP/s
fp32 matrix peak, and the bytes each path must move (every operand and result of every launch once).  Each case runs in a child process under a
time limit; one JSON line a row.
  python scripts/attention_microbench.py                  # (64, 256, 64), (16, 2048, 64), (4, 8192, 64), (16, 2048, 128), non-causal and causal
  python scripts/attention_microbench.py B T d causal     # one case (causal 0 or 1)"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(64, 256, 64), (16, 2048, 64), (4, 8192, 64), (16, 2048, 128)]
WARMUP, SAMPLES, REPS, TIMEOUT_S = 3, 11, 5, 150
PEAK_TFLOPS = 157.3


def sample_ms(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / REPS


def medians_ms(fns):
    """medians of alternating samples of every path"""
    import torch
    for _ in range(WARMUP):
        for fn in fns:
            sample_ms(fn)
    torch.cuda.synchronize()
    got = [[] for _ in fns]
    for _ in range(SAMPLES):
        for i, fn in enumerate(fns):
            got[i].append(sample_ms(fn))
    return [sorted(g)[SAMPLES // 2] for g in got]


def one(B, T, d, causal):
    import torch
    import torch.nn.functional as F
    sys.path.insert(0, ROOT)
    from gennet_amd import ops
    from gennet_amd.engine import device
    dev = device()
    g = torch.Generator(device=dev).manual_seed(0)
    q, k, v, dout = (torch.randn(B, T, d, device=dev, generator=g) * (d ** -0.25 if i < 2 else 1.0) for i in range(4))      # scores of unit variance
    view = (B * T, T, 1)

    def fused_fwd():
        return ops.attention_fwd(q, k, v, None, causal, training=True)

    def fused_both():
        out, lse = fused_fwd()
        return ops.attention_bwd(q, k, v, out, lse, dout, None, causal)

    def composed_fwd():
        p = ops.softmax_fwd(ops.bmm(q, k, trans_b=True), view, inplace=True)
        return p, ops.bmm(p, v)

    def composed_both():
        p, _ = composed_fwd()
        dv = ops.bmm(p, dout, trans_a=True)
        ds = ops.softmax_bwd(ops.bmm(dout, v, trans_b=True), p, view, inplace=True)
        return ops.bmm(ds, k), ops.bmm(ds, q, trans_a=True), dv

    tq, tk, tv = (t.clone().requires_grad_(True) for t in (q, k, v))

    def sdpa_fwd():
        with torch.no_grad():
            return F.scaled_dot_product_attention(q, k, v, is_causal=causal, scale=1.0)

    def sdpa_both():
        tq.grad = tk.grad = tv.grad = None
        F.scaled_dot_product_attention(tq, tk, tv, is_causal=causal, scale=1.0).backward(dout)

    # every path is first held against the others
    ref = sdpa_fwd()
    out, _ = fused_fwd()
    assert float((out - ref).abs().max()) <= 1e-4 * float(ref.abs().max()), 'fused forward differs from sdpa'
    sdpa_both()
    for got, want in zip(fused_both()[:3], (tq.grad, tk.grad, tv.grad)):
        assert float((got - want).abs().max()) <= 1e-3 * float(want.abs().max()), 'fused backward differs from sdpa'
    paths = [('fused', fused_fwd, fused_both), ('sdpa', sdpa_fwd, sdpa_both)]
    if not causal:
        assert float((composed_fwd()[1] - ref).abs().max()) <= 1e-4 * float(ref.abs().max())
        paths.insert(1, ('composed', composed_fwd, composed_both))
    flop_f = 4.0 * B * T * T * d * (0.5 if causal else 1.0)
    flop = {'fwd': flop_f, 'fwd+bwd': 3.5 * flop_f}
    td, tt = 4.0 * B * T * d, 4.0 * B * T * T
    nbytes = {('fused', 'fwd'): 4 * td + 4.0 * B * T, ('composed', 'fwd'): 4 * tt + 5 * td,
              # fused backward: delta reads dout, out; dK / dV reads q, k, v, dout and writes two; dQ reads the four and writes one (lse, delta: B T each)
              ('fused', 'fwd+bwd'): 4 * td + 2 * td + 6 * td + 5 * td + 4.0 * B * T * 6, ('composed', 'fwd+bwd'): 4 * tt + 5 * td + 7 * tt + 8 * td}
    print('attention B %d T %d d %d %s' % (B, T, d, 'causal' if causal else 'full'), flush=True)
    for which, idx in (('fwd', 1), ('fwd+bwd', 2)):
        ms = medians_ms([p[idx] for p in paths])
        for (name, _, _), t in zip(paths, ms):
            row = {'case': [B, T, d, int(causal)], 'pass': which, 'path': name, 'ms': t, 'TFLOPs': flop[which] / t * 1e-9,
                   'of_peak': flop[which] / t * 1e-9 / PEAK_TFLOPS, 'MB': nbytes.get((name, which), 0) * 1e-6, 'over_fused': t / ms[0]}
            print('  %-8s %-9s %9.3f ms  %7.2f TFLOP/s  %5.1f %% of peak  %9.1f MB  (%.2f x the fused time)'
                  % (which, name, t, row['TFLOPs'], 100 * row['of_peak'], row['MB'], row['over_fused']), flush=True)
            print(json.dumps(row), flush=True)


def main():
    args = sys.argv[1:]
    if args and args[0] == '--one':
        return one(int(args[1]), int(args[2]), int(args[3]), bool(int(args[4])))
    if args:
        if len(args) != 4:
            sys.exit(__doc__)
        cases = [tuple(int(a) for a in args)]
    else:
        cases = [s + (c,) for s in SHAPES for c in (0, 1)]
    for c in cases:
        try:          # a fresh child per case under a time limit; after a run that hangs or fails nothing more is started
            r = subprocess.run([sys.executable, os.path.abspath(__file__), '--one'] + [str(a) for a in c], timeout=TIMEOUT_S)
        except subprocess.TimeoutExpired:
            print('case %r: no result within %d s' % (c, TIMEOUT_S), flush=True)
            return 1
        if r.returncode:
            print('case %r: exit status %d' % (c, r.returncode), flush=True)
            return r.returncode
    return 0


if __name__ == '__main__':
    sys.exit(main())
