"""The one-block loss kernel (gn_mse_loss, loss_kernel in csrc/loss.hip) against the streaming loss pass (gn_loss_pass, the same file) for
mean_squared_error at 2^10 .. 2^22 elements: where the engine should switch from the first to the second (ops.LOSS_PASS_MIN_ELEMENTS).

Both are called through the C ABI on preallocated buffers, so what lies between the device events is the launches alone: `--warmup` calls of
each, then `--reps` timed calls of each, the two variants alternating call by call, every call between its own pair of events.  Reported per
size: median and minimum of the old kernel and of the pass (one call = the partial kernel + the one-block finish), the ratio of the medians,
and the pass's HBM rate (12 bytes per element: p, y read, dp written) against the project's streaming yard-stick, 0.7 of the measured
6.29 TB/s copy rate.  The last lines time the evaluation form (dp = NULL, 8 bytes per element) and two other kinds at the largest size.

Then the weighted pass (gn_loss_pass_weighted) beside the unweighted one, under the same protocol: at `--weighted-log2`
element counts (default 2^15 and 2^22), cols = 1 and cols = 1024, mean_squared_error and binary_crossentropy, with and without dp, four
variants alternating call by call -- the unweighted pass twice (the distance of its two medians is the run-to-run spread), the weighted pass
on a precomputed count, and the count kernel alone.  The yard-stick of the weighted pass is the unweighted one scaled by the bytes it moves,
(12 + 4 / cols) / 12 with dp and (8 + 4 / cols) / 8 without.
Prints the tables, then one JSON line."""
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
    ap.add_argument('--weighted-log2', default='15,22', help='element counts (log2, comma-separated) of the weighted comparison')
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
    out = torch.empty(3, device=dev)
    wt = torch.rand(nmax, device=dev) + 0.5
    wt[::4] = 0.0                                    # a quarter of the rows masked, as a padded batch
    cnt = torch.empty(1, dtype=torch.float64, device=dev)
    cols = 256

    def old(n):
        _lib.call('gn_mse_loss', p.data_ptr(), y.data_ptr(), dp.data_ptr(), out.data_ptr(), n, n, stream)

    def new(n, kind='mean_squared_error', grad=True):
        rows = n // cols
        ws = ops.workspace(_lib.size('gn_loss_pass_workspace', rows, cols), dev)
        _lib.call('gn_loss_pass', ops.LOSS_KINDS[kind], p.data_ptr(), y.data_ptr(), dp.data_ptr() if grad else None, out.data_ptr(), rows, cols, float(rows),
                  ws.data_ptr(), ws.numel(), stream)

    def shaped(n, c, kind, grad):
        rows = n // c
        ws = ops.workspace(max(_lib.size('gn_loss_pass_weighted_workspace', rows, c), _lib.size('gn_weight_count_workspace', rows)), dev)
        k, d = ops.LOSS_KINDS[kind], dp.data_ptr() if grad else None

        def plain(_):
            _lib.call('gn_loss_pass', k, p.data_ptr(), y.data_ptr(), d, out.data_ptr(), rows, c, float(rows), ws.data_ptr(), ws.numel(), stream)

        def weighted(_):
            _lib.call('gn_loss_pass_weighted', k, p.data_ptr(), y.data_ptr(), wt.data_ptr(), cnt.data_ptr(), d, out.data_ptr(), rows, c, ws.data_ptr(), ws.numel(),
                      stream)

        def count(_):
            _lib.call('gn_weight_count', wt.data_ptr(), rows, cnt.data_ptr(), ws.data_ptr(), ws.numel(), stream)
        return plain, weighted, count

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
    weighted = []
    print('# weighted pass against the unweighted one: medians in microseconds; pass A / B: the same unweighted call twice in the alternation')
    print('%10s %6s %-20s %4s %9s %9s %10s %9s %9s %9s' % ('elements', 'cols', 'kind', 'dp', 'pass A', 'pass B', 'weighted', 'count', 'w / pass', 'yardstick'))
    for lg in [int(v) for v in args.weighted_log2.split(',') if v]:
        n = 1 << lg
        if n > nmax:
            continue
        for c in (1, 1024):
            for kind in ('mean_squared_error', 'binary_crossentropy'):
                for grad in (True, False):
                    plain, wfn, cfn = shaped(n, c, kind, grad)
                    cfn(n)                           # the count the weighted pass reads
                    t = timed([('a', plain), ('w', wfn), ('b', plain), ('c', cfn)], n)
                    med = dict((k, float(np.median(v))) for k, v in t.items())
                    base = 0.5 * (med['a'] + med['b'])
                    yard = ((12.0 if grad else 8.0) + 4.0 / c) / (12.0 if grad else 8.0)
                    weighted.append({'elements': n, 'cols': c, 'kind': kind, 'dp': grad, 'pass_a_us': med['a'], 'pass_b_us': med['b'], 'weighted_us': med['w'],
                                     'count_us': med['c'], 'ratio': med['w'] / base, 'byte_ratio': yard})
                    print('%10d %6d %-20s %4s %9.2f %9.2f %10.2f %9.2f %9.3f %9.3f' % (n, c, kind, 'yes' if grad else 'no', med['a'], med['b'], med['w'], med['c'],
                                                                                 med['w'] / base, yard))
    print(json.dumps({'bench': 'loss', 'crossover_elements': cross, 'threshold': ops.LOSS_PASS_MIN_ELEMENTS, 'sizes': rows_out, 'extra': extra,
                      'weighted': weighted}))


if __name__ == '__main__':
    main()
