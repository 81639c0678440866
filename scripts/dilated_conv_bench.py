"""Conv1D(64, 5, padding='causal', dilation_rate=d) beside the undilated 'same' layer of the same shape, which runs the same kernels.

Input (B, L, 64) = (64, 2048, 64) by default, d in 1, 2, 16.  Timed with HIP events around `--reps` calls after `--warmup` calls, `--rounds` times, the
dilated layer and the plain one alternating within a round; the median round is reported, with the lowest and the highest:
  layer    forward + backward (data, weight and bias gradient) of the layer outside a model
  passes   the four passes of csrc/dilate.hip the dilated layer adds, alone, on its tensors: split x, merge y, split dy, merge dx (d = 1: the
           merge of y and the split of dy are not run), each as HBM bytes / s -- the floats read inside the input plus the floats written, from
           shapes -- and as a fraction of the measured 6.29 TB/s copy rate
One JSON line per d."""
import argparse
import json
import os
import statistics
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_TBS = 6.29


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


def spread(ts):
    return {'median': round(statistics.median(ts), 4), 'min': round(min(ts), 4), 'max': round(max(ts), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--length', type=int, default=2048)
    ap.add_argument('--channels', type=int, default=64)
    ap.add_argument('--dilations', default='1,2,16')
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=5)
    args = ap.parse_args()
    import torch
    from gennet_amd import ops, layers as Ly
    from gennet_amd.engine import RunContext
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    ops.set_conv_math()
    B, L, C, k = args.batch, args.length, args.channels, 5
    x = torch.randn(B, L, C, device=dev)
    dy = torch.randn(B, L, C, device=dev)
    node = types.SimpleNamespace(index=0, fused_act=None, fused_drop=None, fold_up=None, infer_bn=None, lazy_bn=-1, fuse_prev=-1)

    def make(**kw):
        layer = Ly.Conv1D(C, k, **kw)
        layer.build((L, C))
        layer.kernel.grad = torch.zeros(layer.kernel.shape, device=dev)
        layer.bias.grad = torch.zeros(layer.bias.shape, device=dev)

        def step():
            ctx = RunContext(True)
            layer.forward(ctx, node, x)
            layer.backward(ctx, node, dy, True, True)
        return step

    plain = make(padding='same')
    for d in [int(v) for v in args.dilations.split(',')]:
        dilated = make(padding='causal', dilation_rate=d)
        pl = (k - 1) * d
        M = max(-(-(L + pl) // d), k)
        Lrun = M - k + 1
        xs, ys = torch.empty(B * d, M, C, device=dev), torch.randn(B * d, Lrun, C, device=dev)
        dxs = torch.randn(B * d, M, C, device=dev)
        out_y, out_x, dys = torch.empty(B, L, C, device=dev), torch.empty(B, L, C, device=dev), torch.empty(B * d, Lrun, C, device=dev)
        n = B * L * C
        passes = [('split_x', lambda: ops.dilate_split(x, d, pl, M, out=xs), 4 * (n + xs.numel())),
                  ('merge_dx', lambda: ops.dilate_merge(dxs, B, d, pl, L, out=out_x), 8 * n)]
        if d > 1:
            passes += [('merge_y', lambda: ops.dilate_merge(ys, B, d, 0, L, out=out_y), 8 * n),
                       ('split_dy', lambda: ops.dilate_split(dy, d, 0, Lrun, out=dys), 4 * (n + dys.numel()))]
        t = {'dilated': [], 'plain': []}
        tp = dict((name, []) for name, _, _ in passes)
        for _ in range(args.rounds):
            t['dilated'].append(timed(dilated, args.warmup, args.reps))
            t['plain'].append(timed(plain, args.warmup, args.reps))
            for name, fn, _ in passes:
                tp[name].append(timed(fn, args.warmup, args.reps))
        row = {'layer': "Conv1D(%d, %d, padding='causal', dilation_rate=%d)" % (C, k, d), 'in': [B, L, C], 'phase_batch': [B * d, M, C],
               'conv_math': ops.default_conv_math(), 'fwd_bwd_ms': {'dilated': spread(t['dilated']), "plain 'same'": spread(t['plain'])},
               'dilated_over_plain': round(statistics.median(t['dilated']) / statistics.median(t['plain']), 3), 'passes': {}}
        total = 0.0
        for name, _, nbytes in passes:
            ms = statistics.median(tp[name])
            total += ms
            tbs = nbytes / (ms * 1e-3) / 1e12
            row['passes'][name] = {'ms': spread(tp[name]), 'bytes': nbytes, 'TB_per_s': round(tbs, 3), 'fraction_of_copy_rate': round(tbs / HBM_TBS, 3)}
        row['passes_ms_total'] = round(total, 4)
        print(json.dumps(row), flush=True)
    return 0


if __name__ == '__main__':
    sys.exit(main())
