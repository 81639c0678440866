"""The any-channel convolution kernels (csrc/conv_anyc.hip) against what a user can do without them: zero-pad the channels to the
next multiples of 4 with torch, run the strict kernels on the padded shape, slice the result back to a contiguous tensor.

Shapes: d_model's tap-folded layer (4 -> 50 channels, 4 taps, 50 -> 35 rows) at batch 512 and 20 000, and three sizes where a launch is not
overhead.  Per shape and direction (forward, data gradient, weight gradient), `--warmup` untimed rounds, then `--reps` rounds in which the three
variants run one after the other (so drift hits all alike), each call between its own pair of device events:
  anyc      the _any entry point on the ragged shape
  composed  pad (activations; the weights are padded once, outside) + strict kernel on the padded shape + slice to a contiguous result
  padded    the strict kernel on the padded shape alone: what giving up float4 / LDS-DMA staging costs
Conv math 'fp32', so the strict launches are the direct (or small-channel) family.  One JSON line per shape: median [min, max] in
microseconds, and anyc / composed of the medians."""
import argparse
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [
    # name, B, L, Cin, Cout, k, stride, padding
    ('d_model folded conv, batch 512', 512, 50, 4, 50, 4, 1, 'valid'),
    ('d_model folded conv, batch 20000', 20000, 50, 4, 50, 4, 1, 'valid'),
    ('50 -> 100, k 5', 32, 2048, 50, 100, 5, 1, 'same'),
    ('100 -> 50, k 5', 32, 2048, 100, 50, 5, 1, 'same'),
    ('130 -> 258, k 5, stride 2', 32, 2048, 130, 258, 5, 2, 'same'),
]


def library_label():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    try:
        head = subprocess.run(['git', '-C', root, 'rev-parse', '--short', 'HEAD'], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True).stdout.strip()
        dirty = subprocess.run(['git', '-C', root, 'status', '--porcelain', '--', 'gennet_amd', 'include'], stdout=subprocess.PIPE,
                               stderr=subprocess.DEVNULL, text=True).stdout.strip()
    except OSError:
        head, dirty = '', ''
    return (head + (' + uncommitted changes' if dirty else '')) if head else 'no git metadata beside the library'


def rounds(variants, warmup, reps):
    """{name: [ms per call]}: the variants one after the other per round, each call between its own events"""
    import torch
    for _ in range(warmup):
        for _, fn in variants:
            fn()
    torch.cuda.synchronize()
    ev = {name: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)] for name, _ in variants}
    for r in range(reps):
        for name, fn in variants:
            ev[name][r][0].record()
            fn()
            ev[name][r][1].record()
    torch.cuda.synchronize()
    return {name: [a.elapsed_time(b) for a, b in pairs] for name, pairs in ev.items()}


def stats(ms):
    import numpy as np
    us = np.asarray(ms) * 1e3
    return [round(float(np.median(us)), 1), round(float(us.min()), 1), round(float(us.max()), 1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--only', default='', help='run the shapes whose name contains this text (a profiler run of one shape)')
    ap.add_argument('--label', default='', help='what to call the library in the output (default: the git commit beside it)')
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F
    from gennet_amd import _lib, ops
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    ops.set_conv_math('fp32')
    print(json.dumps({'library': os.path.relpath(_lib.LIB_PATH, os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), 'commit': args.label or library_label(), 'conv_math': 'fp32', 'warmup': args.warmup, 'reps': args.reps,
                      'columns': 'median [min, max] us'}), flush=True)
    up4 = lambda c: -(-c // 4) * 4                                                     # noqa: E731
    for name, B, L, Cin, Cout, k, s, padding in [c for c in SHAPES if args.only in c[0]]:
        assert ops.conv_needs_any(Cin, Cout)
        Lout, pl = ops.conv_geometry(L, k, s, padding)
        ci, co = up4(Cin) - Cin, up4(Cout) - Cout
        x = torch.randn(B, L, Cin, device=dev); dy = torch.randn(B, Lout, Cout, device=dev)
        w = torch.randn(k, Cin, Cout, device=dev) * 0.05; b = torch.randn(Cout, device=dev)
        wt = ops.conv1d_transpose_w(w)
        wp = F.pad(w, (0, co, 0, ci)).contiguous(); bp = F.pad(b, (0, co)).contiguous(); wtp = ops.conv1d_transpose_w(wp)
        xp = F.pad(x, (0, ci)).contiguous(); dyp = F.pad(dy, (0, co)).contiguous()
        pad_x = (lambda: F.pad(x, (0, ci))) if ci else (lambda: x)
        pad_dy = (lambda: F.pad(dy, (0, co))) if co else (lambda: dy)
        cut = lambda t, n: t[..., :n].contiguous() if t.shape[-1] != n else t           # noqa: E731
        directions = {
            'fwd': [('anyc', lambda: ops.conv1d_fwd(x, w, b, s, pl, Lout, 'relu', any_channels=True)),
                    ('composed', lambda: cut(ops.conv1d_fwd(pad_x(), wp, bp, s, pl, Lout, 'relu'), Cout)),
                    ('padded', lambda: ops.conv1d_fwd(xp, wp, bp, s, pl, Lout, 'relu'))],
            'dgrad': [('anyc', lambda: ops.conv1d_dgrad(dy, wt, L, s, pl, any_channels=True)),
                      ('composed', lambda: cut(ops.conv1d_dgrad(pad_dy(), wtp, L, s, pl), Cin)),
                      ('padded', lambda: ops.conv1d_dgrad(dyp, wtp, L, s, pl))],
            'wgrad': [('anyc', lambda: ops.conv1d_wgrad(x, dy, k, s, pl, any_channels=True)),
                      ('composed', lambda: (lambda dw, db: (dw[:, :Cin, :Cout].contiguous(), db[:Cout].contiguous()))(*ops.conv1d_wgrad(pad_x(), pad_dy(), k, s, pl))),
                      ('padded', lambda: ops.conv1d_wgrad(xp, dyp, k, s, pl))],
        }
        out = {'shape': name, 'B': B, 'L': L, 'Cin': Cin, 'Cout': Cout, 'k': k, 'stride': s, 'padding': padding, 'padded_to': [up4(Cin), up4(Cout)],
               'GFLOP': round(2.0 * B * Lout * k * Cin * Cout / 1e9, 3)}
        for d, variants in directions.items():
            t = rounds(variants, args.warmup, args.reps)
            row = {n: stats(v) for n, v in t.items()}
            row['anyc_over_composed'] = round(row['anyc'][0] / row['composed'][0], 3)
            row['anyc_over_padded'] = round(row['anyc'][0] / row['padded'][0], 3)
            out[d] = row
        print(json.dumps(out), flush=True)
        del x, dy, xp, dyp
    return 0


if __name__ == '__main__':
    sys.exit(main())
