"""Rate of the four BatchNormalization passes over an axis that is not the last one (csrc/bn_axis.hip) against the last-axis passes on the same bytes.

The sibling discriminator's sizes: B = 32, L = 1000, C in {128, 256, 512}, BatchNormalization(axis=1): the (outer, P, inner) = (B, L, C) view, one
parameter per position.  The yardstick is the existing last-axis pass (gn_bn_stats, gn_bn_apply, gn_bn_bwd_stats, gn_bn_bwd_apply without mask or
activation) on the (B * L, C) view of the same tensor: it moves the same bytes.  Each pair is timed in the same process, alternating: a sample is
`calls` launches between two device events, and samples of the new and the old pass alternate until each has run for at least --seconds.
Bytes per element come from the shapes: stats 4, apply 8, bwd_stats 8, bwd_apply 12 (the per-parameter vectors are not counted).

    python scripts/bn_axis_microbench.py [--seconds 0.5] [--out profiles/bn_axis_microbench.txt]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BYTES = {'stats': 4, 'apply': 8, 'bwd_stats': 8, 'bwd_apply': 12}


def passes(B, L, C, dev):
    """{pass: (new, old)}: closures over one (B, L, C) tensor pair and per-parameter vectors of the right length for each view"""
    from gennet_amd import ops
    gen = torch.Generator(device=dev).manual_seed(B + L + C)
    x3 = torch.randn((B, L, C), device=dev, generator=gen) * 1.5 + 0.7
    dy3 = torch.randn((B, L, C), device=dev, generator=gen)
    x2, dy2 = x3.view(B * L, C), dy3.view(B * L, C)

    def vectors(n):
        mean = torch.randn(n, device=dev, generator=gen) * 0.1 + 0.7
        inv = torch.rand(n, device=dev, generator=gen) * 0.2 + 0.6
        gamma = torch.rand(n, device=dev, generator=gen) + 0.5
        return mean, inv, gamma, gamma * inv, -mean * gamma * inv, torch.empty(n, device=dev), torch.empty(n, device=dev)
    mP, iP, gP, scP, shP, dgP, dbP = vectors(L)
    mC, iC, gC, scC, shC, dgC, dbC = vectors(C)
    dsP = ops.bn_axis_bwd_stats(dy3, x3, mP, iP)
    dsC = ops.bn_bwd_stats(dy2, None, x2, None, mC, iC, scale=scC, shift=shC)
    nP, nC = B * C, B * L
    return {
        'stats': (lambda: ops.bn_axis_stats(x3), lambda: ops.bn_stats(x2)),
        'apply': (lambda: ops.bn_axis_apply(x3, scP, shP), lambda: ops.bn_apply(x2, scC, shC)),
        'bwd_stats': (lambda: ops.bn_axis_bwd_stats(dy3, x3, mP, iP), lambda: ops.bn_bwd_stats(dy2, None, x2, None, mC, iC, scale=scC, shift=shC)),
        'bwd_apply': (lambda: ops.bn_axis_bwd_apply(dy3, x3, gP, mP, iP, dsP, nP, dsP, dgP, dbP),
                      lambda: ops.bn_bwd_apply(dy2, None, x2, None, gC, mC, iC, dsC, nC, dsC, dgC, dbC, scale=scC, shift=shC)),
    }


def sample(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / calls


def time_pair(new, old, seconds, calls=20):
    for fn in (new, old):                  # warm-up: code objects, the scratch buffer, the allocator's blocks
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    t = {'new': [], 'old': []}
    while min(sum(v) * calls for v in t.values()) < seconds or len(t['new']) < 5:
        t['new'].append(sample(new, calls))
        t['old'].append(sample(old, calls))
    return {k: (float(np.median(v)), float(np.min(v)), len(v)) for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seconds', type=float, default=0.5, help='least timed window per variant')
    ap.add_argument('--B', type=int, default=32)
    ap.add_argument('--L', type=int, default=1000)
    ap.add_argument('--channels', type=int, nargs='+', default=[128, 256, 512])
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from gennet_amd.engine import device
    dev = device()
    lines = ['# scripts/bn_axis_microbench.py on %s: B = %d, L = %d, BatchNormalization(axis=1) as (outer, P, inner) = (B, L, C) against the last-axis passes on (B * L, C)'
             % (torch.cuda.get_device_name(dev), a.B, a.L),
             '# samples of 20 launches between device events, new and old alternating, >= %.2f s per variant; GB/s = bytes from shapes / median time per launch' % a.seconds,
             '%5s %-10s %6s %12s %10s %12s %10s %9s' % ('C', 'pass', 'MB', 'axis us', 'axis GB/s', 'last us', 'last GB/s', 'axis/last')]
    rows = []
    for C in a.channels:
        for name, (new, old) in passes(a.B, a.L, C, dev).items():
            nbytes = BYTES[name] * a.B * a.L * C
            r = time_pair(new, old, a.seconds)
            gb = {k: nbytes / v[0] / 1e9 for k, v in r.items()}
            rows.append({'C': C, 'pass': name, 'bytes': nbytes, 'axis_us': r['new'][0] * 1e6, 'axis_gbs': gb['new'], 'last_us': r['old'][0] * 1e6, 'last_gbs': gb['old'],
                         'samples': r['new'][2]})
            lines.append('%5d %-10s %6.1f %12.2f %10.1f %12.2f %10.1f %9.3f' % (C, name, nbytes / 1e6, r['new'][0] * 1e6, gb['new'], r['old'][0] * 1e6, gb['old'],
                                                                               r['new'][0] / r['old'][0]))
    lines.append(json.dumps({'bench': 'bn_axis', 'B': a.B, 'L': a.L, 'rows': rows}))
    text = '\n'.join(lines)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
