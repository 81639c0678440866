"""Optimizer update passes at the generator's trained-parameter count: every rule of gennet_amd/csrc/optim.hip (and the default Adam pass),
with and without clipnorm, stepped through engine.Optimizer on one flat segment.

Run it under `rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python3 scripts/optimizer_sweep.py`, in a run of its own; then
`python3 scripts/optimizer_sweep.py --stats <dir>/.../kernel_stats.csv` turns the kernel times into bytes / s: HBM bytes the pass must move
(bytes per weight x n, below) over the average kernel time, against the achievable 6.3 TB/s (MI355X_MICROARCH.md).  The event-timed step rates
the run itself prints include the host work of a step and are a cross-check only."""
import argparse
import csv
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

RULES = ['sgd', 'rmsprop', 'adagrad', 'adadelta', 'adamax', 'adam', 'amsgrad']
RULE_ID = {r: k for k, r in enumerate(RULES)}            # gn_optim_rule
# HBM bytes per weight per step: read p, g and the state once, write p and the state once (fp32)
BYTES = {'sgd': 20, 'rmsprop': 20, 'adagrad': 20, 'adadelta': 28, 'adamax': 28, 'adam': 28, 'amsgrad': 36}
CLIP_BYTES = 4                                           # clipnorm: one more read of g (the sum-of-squares pass)
ACHIEVABLE_TBS = 6.3


def make(rule, clip, lr=1e-4):
    from gennet_amd import engine
    kw = {'clipnorm': 1.0} if clip else {}
    if rule == 'amsgrad':
        return engine.Adam(lr, amsgrad=True, **kw)
    if rule == 'adam':
        return engine.Adam(lr, decay=1e-6 if not clip else 0.0, **kw)       # decay: the fused rule pass, not the default Adam pass
    return {'sgd': engine.SGD, 'rmsprop': engine.RMSprop, 'adagrad': engine.Adagrad, 'adadelta': engine.Adadelta, 'adamax': engine.Adamax}[rule](lr, **kw)


def run(args):
    import numpy as np
    import torch
    from gennet_amd import bbh, engine
    n = args.n or sum(p.size for p in bbh.generator_model(args.n_pix).trainable_weights)
    engine.device()
    rng = np.random.RandomState(0)
    p = engine.Param('w', (0.05 * rng.randn(n)).astype(np.float32))
    engine.group_params([p])
    p.grad.copy_(engine.to_device((1e-3 * rng.randn(n)).astype(np.float32)))
    configs = [(r, c) for r in RULES for c in (False, True)] + [('adam_default', False)]
    out = []
    for rule, clip in configs:
        opt = engine.Adam(1e-4, beta_1=0.5) if rule == 'adam_default' else make(rule, clip)
        opt.bind([p])
        for _ in range(args.warmup):
            opt.step()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(args.reps):
            opt.step()
        b.record()
        b.synchronize()
        ms = a.elapsed_time(b) / args.reps
        nbytes = (BYTES['adam' if rule == 'adam_default' else rule] + (CLIP_BYTES if clip else 0)) * n
        rec = {'rule': rule, 'clipnorm': clip, 'n': n, 'event_ms_per_step': round(ms, 4), 'event_TBps': round(nbytes / ms / 1e9, 3)}
        out.append(rec)
        print(json.dumps(rec), flush=True)
        opt.state = None
    return out


def from_stats(path, n):
    """Average kernel time of each pass from rocprofv3's kernel_stats.csv -> achieved bytes / s."""
    avg = {}
    for row in csv.DictReader(open(path)):
        name = row['Name']
        m = re.search(r'optim_kernel<(\d+)>', name)
        key = RULES[int(m.group(1))] if m else ('sumsq' if 'optim_sumsq_kernel' in name else 'finalize' if 'optim_clip_factor_kernel' in name
                                                 else 'adam_default' if 'adam_kernel' in name else None)
        if key:
            avg[key] = (float(row['AverageNs']), int(row['Calls']))
    lines = ['# n = %d weights (the generator\'s trained parameters); bytes per weight x n over the rocprofv3 average kernel time; achievable %.1f TB/s'
             % (n, ACHIEVABLE_TBS), '%-14s %6s %10s %9s %7s %8s' % ('pass', 'B/wt', 'avg us', 'TB/s', 'of 6.3', 'launches')]
    res = {}
    for key in RULES + ['adam_default']:
        if key not in avg:
            continue
        ns, calls = avg[key]
        b = BYTES['adam' if key == 'adam_default' else key] * n
        res[key] = {'bytes_per_weight': b // n, 'avg_us': ns / 1e3, 'TBps': b / ns / 1e3}
        lines.append('%-14s %6d %10.1f %9.3f %7.3f %8d' % (key, b // n, ns / 1e3, b / ns / 1e3, b / ns / 1e3 / ACHIEVABLE_TBS, calls))
    if 'sumsq' in avg and 'finalize' in avg:
        s_ns, f_ns = avg['sumsq'][0], avg['finalize'][0]
        lines.append('%-14s %6d %10.1f %9.3f %7.3f %8d' % ('sumsq (clip)', CLIP_BYTES, s_ns / 1e3, CLIP_BYTES * n / s_ns / 1e3,
                                                           CLIP_BYTES * n / s_ns / 1e3 / ACHIEVABLE_TBS, avg['sumsq'][1]))
        lines.append('%-14s %6s %10.1f' % ('clip finalize', '-', f_ns / 1e3))
        for key in RULES:
            if key in avg:
                ns = avg[key][0] + s_ns + f_ns
                b = (BYTES[key] + CLIP_BYTES) * n
                lines.append('%-14s %6d %10.1f %9.3f %7.3f' % (key + '+clip', BYTES[key] + CLIP_BYTES, ns / 1e3, b / ns / 1e3, b / ns / 1e3 / ACHIEVABLE_TBS))
    print('\n'.join(lines))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n-pix', type=int, default=2048, help='generator size whose trained-parameter count is n')
    ap.add_argument('--n', type=int, default=0, help='override the weight count')
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--stats', default=None, help="rocprofv3 kernel_stats.csv of a sweep run: print the bandwidth table")
    args = ap.parse_args()
    if args.stats:
        from gennet_amd import bbh
        from_stats(args.stats, args.n or sum(p.size for p in bbh.generator_model(args.n_pix).trainable_weights))
    else:
        run(args)


if __name__ == '__main__':
    main()
