#!/usr/bin/env python
"""Time keras layers.LSTM's arithmetic at (B, T, Cin, u) -- forward in the inference phase (zx = X W through gn_bmm, then gn_lstm_fwd) and a
training forward + backward (gn_lstm_fwd storing gates, c and hprev; gn_lstm_bwd; dW, dU as the layer forms them, dX through gn_bmm; db) -- and torch.nn.LSTM in fp32
at the same shape on the same GPU (forward under no_grad, and forward + backward with gradients for the input and the weights) as the outside
yardstick.  One process per shape: 3 warm-up runs, then the median of 11 samples of one run each between two device events.  Prints ms per
run, us per time step, the ratio to torch, and the largest difference between the two forward results on the same weights (sigmoid gates, the
form torch implements).  Each shape runs in a child process under a time limit; ours is timed and printed before torch's is started.
  python scripts/lstm_microbench.py                 # (8, 1024, 64, 64), (64, 256, 64, 128), (512, 128, 128, 256)
  python scripts/lstm_microbench.py B T Cin u       # one shape"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(8, 1024, 64, 64), (64, 256, 64, 128), (512, 128, 128, 256)]
WARMUP, SAMPLES, TIMEOUT_S = 3, 11, 240


def one(B, T, Cin, u):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from gennet_amd import ops
    from gennet_amd.engine import device
    from gennet_amd.recurrent import rows_product
    dev = device()

    def median_ms(fn):
        for _ in range(WARMUP):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(SAMPLES):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return sorted(ts)[len(ts) // 2]

    rng = np.random.RandomState(0)
    x = torch.tensor(rng.randn(B, T, Cin).astype(np.float32), device=dev)
    W = torch.tensor((rng.randn(Cin, 4 * u) / np.sqrt(Cin)).astype(np.float32), device=dev)
    U = torch.tensor((rng.randn(u, 4 * u) / np.sqrt(u)).astype(np.float32), device=dev)
    b = torch.tensor((0.1 * rng.randn(4 * u)).astype(np.float32), device=dev)
    dy = torch.tensor(rng.randn(B, T, u).astype(np.float32), device=dev)
    dW, dU, db = torch.empty_like(W), torch.empty_like(U), torch.empty_like(b)
    acts = dict(activation='tanh', recurrent_activation='sigmoid')

    def fwd(training=False):
        zx = ops.bmm(x.view(1, B * T, Cin), W.view(1, Cin, 4 * u)).view(B, T, 4 * u)
        return ops.lstm_fwd(zx, U, b, None, None, training=training, **acts)

    def fwd_bwd():
        h, gates, c, hprev = fwd(True)
        dz, _, _ = ops.lstm_bwd(dy, gates, c, U, None, **acts)
        dz2 = dz.view(B * T, 4 * u)
        rows_product(x.view(B * T, Cin), dz2, dW)
        rows_product(hprev.view(B * T, u), dz2, dU)
        ops.bias_grad(dz2, db)
        return ops.bmm(dz2.view(1, B * T, 4 * u), W.view(1, Cin, 4 * u), trans_b=True)

    print('shape (B %d, T %d, Cin %d, u %d)' % (B, T, Cin, u), flush=True)
    t_f, t_fb = median_ms(fwd), median_ms(fwd_bwd)
    h_ours = fwd()[0]
    row = {'shape': [B, T, Cin, u], 'fwd_ms': t_f, 'fwd_bwd_ms': t_fb}
    print('  gennet_amd   forward %9.3f ms (%7.2f us a step)   forward + backward %9.3f ms (%7.2f us a step)'
          % (t_f, 1e3 * t_f / T, t_fb, 1e3 * t_fb / T), flush=True)

    m = torch.nn.LSTM(Cin, u, batch_first=True).to(dev)
    with torch.no_grad():
        m.weight_ih_l0.copy_(W.t())
        m.weight_hh_l0.copy_(U.t())
        m.bias_ih_l0.copy_(b)
        m.bias_hh_l0.zero_()
    xg = x.clone().requires_grad_(True)

    def t_fwd():
        with torch.no_grad():
            return m(x)[0]

    def t_fwd_bwd():
        m.zero_grad(set_to_none=True)
        xg.grad = None
        m(xg)[0].backward(dy)

    tt_f, tt_fb = median_ms(t_fwd), median_ms(t_fwd_bwd)
    diff = float((t_fwd() - h_ours).abs().max())
    row.update(torch_fwd_ms=tt_f, torch_fwd_bwd_ms=tt_fb, max_diff=diff)
    print('  torch.nn.LSTM forward %9.3f ms (%7.2f us a step)   forward + backward %9.3f ms (%7.2f us a step)'
          % (tt_f, 1e3 * tt_f / T, tt_fb, 1e3 * tt_fb / T))
    print('  torch / gennet_amd: forward %.2f, forward + backward %.2f;  largest |h - h_torch| %.3g' % (tt_f / t_f, tt_fb / t_fb, diff))
    print(json.dumps(row), flush=True)


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
