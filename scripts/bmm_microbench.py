#!/usr/bin/env python
"""Time the six batched products of attention over (batch, L, M, C) -- q . k^T, a . v and their four gradient products -- through gn_bmm (the fp32
matrix-core kernel of csrc/bmm.hip), through gn_bmm_valu (the batched 16 x 16 VALU tile, the form capi.hip's dense_any uses) and through
torch.bmm in fp32, in one process per shape: 5 warm-up launches, then the median of 15 samples of 5 launches each between two device events.
Prints us per launch, TFLOP/s (2 * batch * L * M * C over the time), the share of the 157.3 TFLOP/s fp32 MFMA peak and the ratio to torch.bmm,
and the largest difference between the three results at the timed size.  Each shape runs in a child process under a time limit.
  python scripts/bmm_microbench.py                   # (64, 1024, 1024, 64) and (16, 2048, 2048, 128)
  python scripts/bmm_microbench.py batch L M C       # one shape"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(64, 1024, 1024, 64), (16, 2048, 2048, 128)]
PEAK_TFLOPS = 157.3
WARMUP, SAMPLES, LAUNCHES, TIMEOUT_S = 5, 15, 5, 240


def products(batch, L, M, C):
    """(name, a shape, b shape, trans_a, trans_b): the output is (batch, rows of A, columns of B)"""
    q, k, a, v = (batch, L, C), (batch, M, C), (batch, L, M), (batch, M, C)
    return [('scores = q . k^T', q, k, False, True), ('ctx = a . v', a, v, False, False),
            ('dq = dscores . k', a, k, False, False), ('dk = dscores^T . q', a, q, True, False),
            ('da = dctx . v^T', q, v, False, True), ('dv = a^T . dctx', a, q, True, False)]


def one(batch, L, M, C):
    import torch
    sys.path.insert(0, ROOT)
    from gennet_amd import ops
    from gennet_amd.engine import device
    dev = device()

    def median_us(fn):
        for _ in range(WARMUP):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(SAMPLES):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(LAUNCHES):
                fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3 / LAUNCHES)
        return sorted(ts)[len(ts) // 2]

    flop = 2.0 * batch * L * M * C
    print('shape (batch %d, L %d, M %d, C %d): %.1f GFLOP a product' % (batch, L, M, C, flop / 1e9))
    print('%-20s %9s %7s %6s %8s | %9s %7s | %9s %7s | %9s' % ('product', 'mfma us', 'TF', 'peak', 'x torch', 'valu us', 'TF', 'torch us', 'TF', 'max diff'))
    rows = []
    for i, (name, sa, sb, ta, tb) in enumerate(products(batch, L, M, C)):
        a = ops.fill_uniform(sa, -1.0, 1.0, 10 + i, 0, dev)
        b = ops.fill_uniform(sb, -1.0, 1.0, 20 + i, 0, dev)
        out = torch.empty((batch, sa[2] if ta else sa[1], sb[1] if tb else sb[2]), device=dev)
        at, bt = (a.transpose(1, 2) if ta else a), (b.transpose(1, 2) if tb else b)
        ref = torch.empty_like(out)
        t_mfma = median_us(lambda: ops.bmm(a, b, ta, tb, out=out))
        c_mfma = out.clone()
        t_valu = median_us(lambda: ops.bmm(a, b, ta, tb, out=out, valu=True))
        c_valu = out.clone()
        t_torch = median_us(lambda: torch.bmm(at, bt, out=ref))
        diff = max(float((c_mfma - c_valu).abs().max()), float((c_mfma - ref).abs().max()))
        tf = [flop / (t * 1e-6) / 1e12 for t in (t_mfma, t_valu, t_torch)]
        print('%-20s %9.1f %7.1f %5.0f%% %8.2f | %9.1f %7.1f | %9.1f %7.1f | %9.2g'
              % (name, t_mfma, tf[0], 100 * tf[0] / PEAK_TFLOPS, t_torch / t_mfma, t_valu, tf[1], t_torch, tf[2], diff), flush=True)
        rows.append({'product': name, 'mfma_us': t_mfma, 'valu_us': t_valu, 'torch_us': t_torch, 'mfma_tflops': tf[0], 'valu_tflops': tf[1],
                     'torch_tflops': tf[2], 'max_diff': diff})
    print(json.dumps({'shape': [batch, L, M, C], 'rows': rows}), flush=True)


def main():
    if len(sys.argv) == 6 and sys.argv[1] == '--one':
        return one(*[int(v) for v in sys.argv[2:]])
    shapes = [tuple(int(v) for v in sys.argv[1:])] if len(sys.argv) == 5 else SHAPES
    for s in shapes:
        try:          # a fresh child per shape under a time limit; after a run that hangs or fails nothing more is started
            r = subprocess.run([sys.executable, os.path.abspath(__file__), '--one'] + [str(v) for v in s], timeout=TIMEOUT_S)
        except subprocess.TimeoutExpired:
            print('shape %r: no result within %d s' % (s, TIMEOUT_S), flush=True)
            return 1
        if r.returncode:
            print('shape %r: exit status %d' % (s, r.returncode), flush=True)
            return r.returncode
    return 0


if __name__ == '__main__':
    sys.exit(main())
