"""Rate of the pooling passes (csrc/pooling.hip) against existing passes that move the same bytes.

The sizes of scripts/bn_axis_microbench.py: B = 32, L = 1000, C in {128, 256, 512}, the tensor (B, L, C) = (B, L, 1, C).  Pairs (new | yardstick):
  max_fwd, max_bwd   the generic windowed maximum at pool (2,1), strides (2,1), 'valid' | gn_maxpool_h2_fwd / _bwd on the same tensor
  gavg_fwd           the global average over L | the fixed-order column sum over the same bytes: the bias gradient of the (B * L, C) view
  gavg_bwd           the global average's gradient, a pure store of the tensor | gn_bn_apply (the plain stream-through pass: 8 bytes per
                     element) on as many rows of C floats as move the same bytes
  avg_fwd, avg_bwd   the windowed average and its gradient at (2,1)/(2,1)/'valid' | gn_bn_apply, likewise
Each pair is timed in the same process, alternating: a sample is `calls` launches between two device events, and samples of the new pass and
the yardstick alternate until each has run for at least --seconds.  Bytes come from the shapes (each operand read once, the result written
once; the per-channel vectors are not counted).  The gate of DESIGN 8h is new / yardstick >= 0.97 in bytes per second at the largest C.

    python scripts/pool_microbench.py [--seconds 0.5] [--out profiles/pool_microbench.txt]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GATE = 0.97


def passes(B, L, C, dev):
    """{pass: (new, new bytes, yardstick, yardstick bytes)}: closures over one (B, L, C) tensor"""
    from gennet_amd import ops
    gen = torch.Generator(device=dev).manual_seed(B + L + C)
    x = torch.randn((B, L, 1, C), device=dev, generator=gen)
    x3, x2 = x.view(B, L, C), x.view(B * L, C)
    n = 4 * B * L * C                                            # bytes of the tensor
    half = torch.randn((B, L // 2, 1, C), device=dev, generator=gen)      # a gradient of the pooled shape
    g2 = torch.randn((B, C), device=dev, generator=gen)
    scale, shift = torch.rand(C, device=dev, generator=gen) + 0.5, torch.randn(C, device=dev, generator=gen)
    db = torch.empty(C, device=dev)
    p, s = (2, 1), (2, 1)

    def stream(nbytes):
        """gn_bn_apply over the rows of x2 that move about nbytes (8 per element), and the bytes it does move"""
        rows = min(B * L, max(1, nbytes // (8 * C)))
        xs = x2[:rows]
        return (lambda: ops.bn_apply(xs, scale, shift)), 8 * rows * C

    return {
        'max_fwd': (lambda: ops.pool2d_fwd('max', x, p, s, 'valid'), n + n // 2, lambda: ops.maxpool_h2_fwd(x), n + n // 2),
        'max_bwd': (lambda: ops.pool2d_bwd('max', half, x, x.shape, p, s, 'valid'), 2 * n + n // 2, lambda: ops.maxpool_h2_bwd(half, x), 2 * n + n // 2),
        'gavg_fwd': (lambda: ops.global_pool_fwd('avg', x3), n, lambda: ops.bias_grad(x2, db), n),
        'gavg_bwd': (lambda: ops.global_pool_bwd('avg', g2, None, None, x3.shape), n) + stream(n),
        'avg_fwd': (lambda: ops.pool2d_fwd('avg', x, p, s, 'valid'), n + n // 2) + stream(n + n // 2),
        'avg_bwd': (lambda: ops.pool2d_bwd('avg', half, None, x.shape, p, s, 'valid'), n + n // 2) + stream(n + n // 2),
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
    lines = ['# scripts/pool_microbench.py on %s: B = %d, L = %d, the pooling passes on (B, L, 1, C) against existing passes that move the same bytes'
             % (torch.cuda.get_device_name(dev), a.B, a.L),
             '# samples of 20 launches between device events, new and yardstick alternating, >= %.2f s per variant; GB/s = bytes from shapes / median time per launch' % a.seconds,
             '# new/old = ratio of the two GB/s; the gate: >= %.2f at C = %d' % (GATE, max(a.channels)),
             '%5s %-9s %7s %10s %10s %7s %10s %10s %8s' % ('C', 'pass', 'new MB', 'new us', 'new GB/s', 'old MB', 'old us', 'old GB/s', 'new/old')]
    rows = []
    for C in a.channels:
        for name, (new, new_bytes, old, old_bytes) in passes(a.B, a.L, C, dev).items():
            r = time_pair(new, old, a.seconds)
            gb_new, gb_old = new_bytes / r['new'][0] / 1e9, old_bytes / r['old'][0] / 1e9
            rows.append({'C': C, 'pass': name, 'new_bytes': new_bytes, 'new_us': r['new'][0] * 1e6, 'new_gbs': gb_new, 'old_bytes': old_bytes,
                         'old_us': r['old'][0] * 1e6, 'old_gbs': gb_old, 'ratio': gb_new / gb_old, 'samples': r['new'][2]})
            lines.append('%5d %-9s %7.1f %10.2f %10.1f %7.1f %10.2f %10.1f %8.3f%s' % (C, name, new_bytes / 1e6, r['new'][0] * 1e6, gb_new, old_bytes / 1e6,
                                                                                      r['old'][0] * 1e6, gb_old, gb_new / gb_old,
                                                                                      '  < gate' if C == max(a.channels) and gb_new / gb_old < GATE else ''))
    lines.append(json.dumps({'bench': 'pool', 'B': a.B, 'L': a.L, 'gate': GATE, 'rows': rows}))
    text = '\n'.join(lines)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
