"""Noise-layer passes (gennet_amd/csrc/noise_layers.hip) at the discriminator's first activation at the benchmark's GAN batch:
512 x 1024 x 2 x 256 fp32 (1 GiB).  Each pass is timed with HIP events around `--reps` launches after `--warmup` launches and reported as time,
HBM bytes / s (8 bytes per element: one read, one write) and the fraction of the measured 6.29 TB/s copy rate.  The same run times the
two-pass composition the fused GaussianNoise forward replaces: gn_fill_normal into a scratch tensor (4 bytes per element), then an add pass
(gn_axpy, 12 bytes per element).  Prints one JSON line per pass and a summary line; exits non-zero if the fused forward is not faster."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_TBS = 6.29


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', default='512,1024,2,256')
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reps', type=int, default=10)
    args = ap.parse_args()
    import numpy as np
    import torch
    from gennet_amd import ops
    from gennet_amd.layers import AlphaDropout, GaussianDropout
    dev = torch.device('cuda:0')
    shape = tuple(int(v) for v in args.shape.split(','))
    n = int(np.prod(shape))
    x = ops.fill_normal(shape, 0.0, 1.0, 1, 0, dev)
    y = torch.empty_like(x)
    t = torch.empty_like(x)
    gd, ad = GaussianDropout(0.4), AlphaDropout(0.4)
    seed = 7

    def fused_noise(k):
        ops.gaussian_noise(x, 0.1, seed, k * n // 4, out=y)

    def two_pass(k):
        ops.axpy(ops.fill_normal(shape, 0.0, 0.1, seed, k * n // 4, dev), x, 1.0)

    def fill_only(k):
        ops.fill_normal(shape, 0.0, 0.1, seed, k * n // 4, dev)

    def add_only(k):
        ops.axpy(t, x, 1.0)

    passes = [
        ('gaussian_noise_fwd', fused_noise, 8),
        ('gaussian_dropout_apply', lambda k: ops.gaussian_dropout(x, gd.sd, seed, k * n // 4, out=y), 8),
        ('alpha_dropout_fwd', lambda k: ops.alpha_dropout_fwd(x, ad.rate, ad.a, ad.b, ad.alpha_p, seed, k * n // 4, out=y), 8),
        ('alpha_dropout_bwd', lambda k: ops.alpha_dropout_bwd(x, ad.rate, ad.a, seed, k * n // 4, out=y), 8),
        ('fill_normal', fill_only, 4),
        ('axpy_add', add_only, 12),
        ('fill_normal+add (two passes)', two_pass, 16),
    ]
    res = {}
    for name, fn, bpe in passes:
        for k in range(args.warmup):
            fn(k)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for k in range(args.reps):
            fn(args.warmup + k)
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1) / args.reps
        bps = bpe * n / (ms * 1e-3)
        res[name] = ms
        print(json.dumps({'pass': name, 'elements': n, 'ms': round(ms, 4), 'bytes_per_element': bpe, 'TB_per_s': round(bps / 1e12, 3),
                          'fraction_of_hbm': round(bps / (HBM_TBS * 1e12), 3),
                          'elements_per_s': round(n / (ms * 1e-3) / 1e9, 2)}), flush=True)
    fused, composed = res['gaussian_noise_fwd'], res['fill_normal+add (two passes)']
    print(json.dumps({'summary': 'gaussian_noise_fwd vs fill_normal + add', 'fused_ms': round(fused, 4), 'two_pass_ms': round(composed, 4),
                      'speedup': round(composed / fused, 3)}), flush=True)
    return 0 if fused < composed else 1


if __name__ == '__main__':
    sys.exit(main())
