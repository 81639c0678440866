"""The one-block loss kernel (gn_mse_loss, csrc/elementwise.hip) against the streaming loss pass (gn_loss_pass, csrc/loss.hip) for
mean_squared_error at 2^10 .. 2^22 elements: where the engine should switch from the first to the second (ops.LOSS_PASS_MIN_ELEMENTS).

Both are called through the C ABI on preallocated buffers, so what lies between the device events is the launches alone: `--warmup` calls of
each, then `--reps` timed calls of each, the two variants alternating call by call, every call between its own pair of events.  Reported per
size: median and minimum of the old kernel and of the pass (one call = the partial kernel + the one-block finish), the ratio of the medians,
and the pass's HBM rate (12 bytes per element: p, y read, dp written) against the project's streaming yard-stick, 0.7 of the measured
6.29 TB/s copy rate.  The last lines time the evaluation form (dp = NULL, 8 bytes per element) and two other kinds at the largest size.
Prints a table, then one JSON line."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_TBS = 6.29
YARDSTICK = 0.7 * HBM_TBS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--min-log2', type=int, default=10)
    ap.add_argument('--max-log2', type=int, default=22)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--reps', type=int, default=20)
    args = ap.parse_args()
    import numpy as np
    import torch
    from gennet_amd import _lib, ops
    if not torch.cuda.is_available():
        raise SystemExit('loss_bench: no GPU (a timing needs the device)')
    dev = torch.device('cuda:0')
    stream = torch.cuda.current_stream().cuda_stream
    nmax = 1 << args.max_log2
    p = torch.rand(nmax, device=dev)
    y = torch.rand(nmax, device=dev)
    dp = torch.empty(nmax, device=dev)
    out = torch.empty(2, device=dev)
    cols = 256

    def old(n):
        _lib.call('gn_mse_loss', p.data_ptr(), y.data_ptr(), dp.data_ptr(), out.data_ptr(), n, n, stream)

    def new(n, kind='mean_squared_error', grad=True):
        rows = n // cols
        ws = ops.workspace(_lib.size('gn_loss_pass_workspace', rows, cols), dev)
        _lib.call('gn_loss_pass', ops.LOSS_KINDS[kind], p.data_ptr(), y.data_ptr(), dp.data_ptr() if grad else None, out.data_ptr(), rows, cols, float(rows),
                  ws.data_ptr(), ws.numel(), stream)

    def timed(fns, n):
        """Alternating, each call between its own events: {name: [ms, ...]}."""
        for _ in range(args.warmup):
            for _, fn in fns:
                fn(n)
        torch.cuda.synchronize()
        ev = dict((name, []) for name, _ in fns)
        for _ in range(args.reps):
            for name, fn in fns:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn(n)
                b.record()
                ev[name].append((a, b))
        torch.cuda.synchronize()
        return dict((name, np.array([a.elapsed_time(b) for a, b in v]) * 1e3) for name, v in ev.items())     # microseconds

    rows_out = []
    print('# mean_squared_error, %d warm-up + %d timed calls per variant and size, alternating; microseconds between device events' % (args.warmup, args.reps))
    print('%10s %12s %12s %12s %12s %9s %10s %8s' % ('elements', 'old median', 'old min', 'pass median', 'pass min', 'old/pass', 'pass TB/s', 'of %.2f' % YARDSTICK))
    for lg in range(args.min_log2, args.max_log2 + 1):
        n = 1 << lg
        t = timed([('old', old), ('pass', new)], n)
        mo, mp = float(np.median(t['old'])), float(np.median(t['pass']))
        tbs = 12.0 * n / (mp * 1e-6) / 1e12
        rows_out.append({'elements': n, 'old_us_median': mo, 'old_us_min': float(t['old'].min()), 'pass_us_median': mp, 'pass_us_min': float(t['pass'].min()),
                         'pass_tb_s': tbs})
        print('%10d %12.2f %12.2f %12.2f %12.2f %9.2f %10.3f %8.3f' % (n, mo, t['old'].min(), mp, t['pass'].min(), mo / mp, tbs, tbs / YARDSTICK))
    cross = next((r['elements'] for r in rows_out if r['pass_us_median'] < r['old_us_median']), None)
    print('# first size at which the pass is faster: %s' % cross)
    extra = {}
    for name, kind, grad, bpe in (('mse, dp = NULL', 'mean_squared_error', False, 8), ('logcosh', 'logcosh', True, 12),
                                  ('binary_crossentropy', 'binary_crossentropy', True, 12), ('cosine_proximity', 'cosine_proximity', True, 20)):
        t = timed([(name, lambda n, kind=kind, grad=grad: new(n, kind, grad))], nmax)[name]
        m = float(np.median(t))
        extra[name] = {'us_median': m, 'tb_s': bpe * nmax / (m * 1e-6) / 1e12}
        print('# %-22s at %d elements: median %.2f us, %d bytes per element, %.3f TB/s' % (name, nmax, m, bpe, extra[name]['tb_s']))
    print(json.dumps({'bench': 'loss', 'crossover_elements': cross, 'threshold': ops.LOSS_PASS_MIN_ELEMENTS, 'sizes': rows_out, 'extra': extra}))


if __name__ == '__main__':
    main()
