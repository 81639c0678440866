"""The two softmax passes (csrc/softmax.hip) in each of their regimes, as achieved HBM bytes / s.

Every tensor holds 2^27 floats (512 MiB, twice the 256 MiB last-level cache), so a pass reads from and writes to HBM.  Timed with HIP events around
`--reps` calls after `--warmup` calls, `--rounds` times; the median round is reported with the lowest and the highest.  Bytes are counted from
shapes: forward 8 per element where a row fits the lanes that own it and 12 where it is read twice, backward 12 and 20.  A device-to-device copy
of the same tensor (8 bytes per element) is timed in the same run, between the regimes, as the rate to hold them against.  One JSON line per shape."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N = 1 << 27
# (regime, P, inner, row fits); outer = N / (P * inner)
SHAPES = [('rows W=4', 4, 1, True), ('rows W=16', 16, 1, True), ('rows W=64', 64, 1, True), ('rows NJ=16', 1024, 1, True), ('block', 4096, 1, True),
          ('stream', 65536, 1, False), ('split', 32, 8, True), ('split', 512, 8, False), ('axis float4', 8, 256, True), ('axis float4', 128, 256, False)]


def timed(fn, warmup, reps):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def spread(ts, nbytes):
    return {'ms': round(statistics.median(ts), 4), 'TB/s': round(nbytes / statistics.median(ts) * 1e-9, 3),
            'TB/s range': [round(nbytes / max(ts) * 1e-9, 3), round(nbytes / min(ts) * 1e-9, 3)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=3)
    args = ap.parse_args()
    import torch
    from gennet_amd import ops
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    x = torch.randn(N, device=dev)
    dy = torch.randn(N, device=dev)
    y, dx = torch.empty_like(x), torch.empty_like(x)
    for regime, P, inner, fits in SHAPES:
        view = (N // (P * inner), P, inner)
        fwd, bwd, copy = [], [], []
        for _ in range(args.rounds):
            copy.append(timed(lambda: dx.copy_(x), args.warmup, args.reps))
            fwd.append(timed(lambda: ops.softmax_fwd(x, view, out=y), args.warmup, args.reps))
            bwd.append(timed(lambda: ops.softmax_bwd(dy, y, view, out=dx), args.warmup, args.reps))
        print(json.dumps({'regime': regime, 'view': view, 'forward': spread(fwd, (8 if fits else 12) * N), 'backward': spread(bwd, (12 if fits else 20) * N),
                          'copy': spread(copy, 8 * N)}), flush=True)


if __name__ == '__main__':
    main()
