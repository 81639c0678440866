#!/usr/bin/env python
"""Time keras layers.LayerNormalization's arithmetic (csrc/layernorm.hip) over the (rows, N) view -- the forward in the training phase
(gn_layernorm_fwd writing y, mean and rstd) and forward + backward (gn_layernorm_bwd: dx, dgamma, dbeta) -- against two yardsticks in the same
process:
  * copy   a device-to-device copy of the same bytes, half read and half written: the bytes the algorithm needs, every operand once, computed from
           the shape -- 8 an element forward (x in, y out), 20 forward + backward (and dy, x in, dx out); the statistics and parameters are left out;
  * torch  fp32 torch.nn.functional.layer_norm, its backward through autograd.
A sample is REPS launches between two device events; samples of the paths alternate; 3 warm-up samples, then the median of 11.  Reported: ms, the
TB/s of the needed bytes, and the share of the copy's rate.  All cases run in one child process under a time limit; one JSON line a row.
  python scripts/layernorm_microbench.py                  # (64 * 2048, 64), (64 * 256, 128), (16 * 8192, 256), (512 * 128, 1024), (4096, 8192)
  python scripts/layernorm_microbench.py rows N           # one case"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(64 * 2048, 64), (64 * 256, 128), (16 * 8192, 256), (512 * 128, 1024), (4096, 8192)]
WARMUP, SAMPLES, REPS, TIMEOUT_S = 3, 11, 10, 300


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


def one(rows, N):
    import torch
    import torch.nn.functional as F
    from gennet_amd import ops
    from gennet_amd.engine import device
    dev = device()
    g = torch.Generator(device=dev).manual_seed(0)
    x, dy = (torch.randn(rows, N, device=dev, generator=g) for _ in range(2))
    gamma, beta = torch.rand(N, device=dev, generator=g) + 0.5, torch.randn(N, device=dev, generator=g)
    y, dgamma, dbeta = torch.empty_like(x), torch.empty_like(gamma), torch.empty_like(beta)
    regime = 'rows' if N <= ops.LAYERNORM_ROWS_MAX_N else 'block' if N <= ops.LAYERNORM_BLOCK_MAX_N else 'stream'

    def fused_fwd():
        return ops.layernorm_fwd(x, gamma, beta, N, 1e-3, training=True, out=y)

    def fused_both():
        _, mean, rstd = fused_fwd()
        return ops.layernorm_bwd(dy, x, gamma, mean, rstd, N, True, dgamma, dbeta)

    tx, tg, tb = (t.clone().requires_grad_(True) for t in (x, gamma, beta))

    def torch_fwd():
        with torch.no_grad():
            return F.layer_norm(x, (N,), gamma, beta, 1e-3)

    def torch_both():
        tx.grad = tg.grad = tb.grad = None
        F.layer_norm(tx, (N,), tg, tb, 1e-3).backward(dy)

    # every path is first held against the other
    ref = torch_fwd()
    assert float((fused_fwd()[0] - ref).abs().max()) <= 1e-4 * float(ref.abs().max()), 'the forward differs from torch'
    torch_both()
    for got, want in zip(fused_both(), (tx.grad, tg.grad, tb.grad)):
        assert float((got - want).abs().max()) <= 1e-3 * float(want.abs().max()), 'the backward differs from torch'
    nbytes = {'fwd': 8.0 * rows * N, 'fwd+bwd': 20.0 * rows * N}
    print('layernorm rows %d N %d (%s)' % (rows, N, regime), flush=True)
    for which, fused, theirs in (('fwd', fused_fwd, torch_fwd), ('fwd+bwd', fused_both, torch_both)):
        src = torch.empty(int(nbytes[which] // 8), dtype=torch.float32, device=dev).normal_(generator=g)
        dst = torch.empty_like(src)
        ms = medians_ms([fused, lambda: dst.copy_(src), theirs])
        del src, dst
        for name, t in zip(('fused', 'copy', 'torch'), ms):
            row = {'case': [rows, N], 'regime': regime, 'pass': which, 'path': name, 'ms': t, 'MB': nbytes[which] * 1e-6, 'TBps': nbytes[which] / t * 1e-9,
                   'of_copy_rate': ms[1] / t, 'over_fused': t / ms[0]}
            print('  %-8s %-6s %9.4f ms  %8.1f MB needed  %6.2f TB/s  %5.1f %% of the copy rate  (%.2f x the fused time)'
                  % (which, name, t, row['MB'], row['TBps'], 100 * row['of_copy_rate'], row['over_fused']), flush=True)
            print(json.dumps(row), flush=True)


def main():
    args = sys.argv[1:]
    if args and args[0] == '--run':
        sys.path.insert(0, ROOT)
        for i in range(1, len(args), 2):
            one(int(args[i]), int(args[i + 1]))
        return 0
    if args and len(args) != 2:
        sys.exit(__doc__)
    cases = [tuple(int(a) for a in args)] if args else SHAPES
    try:          # one fresh child under a time limit; after a run that hangs or fails nothing more is started
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--run'] + [str(a) for c in cases for a in c], timeout=TIMEOUT_S)
    except subprocess.TimeoutExpired:
        print('no result within %d s' % TIMEOUT_S, flush=True)
        return 1
    return r.returncode


if __name__ == '__main__':
    sys.exit(main())
