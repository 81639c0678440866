#!/usr/bin/env python
"""Time keras layers.LSTM's arithmetic at (B, T, Cin, u) -- forward in the inference phase (zx = X W through gn_bmm, then gn_lstm_fwd) and a
training forward + backward (gn_lstm_fwd storing gates, c and hprev; gn_lstm_bwd; dW, dU as the layer forms them, dX through gn_bmm; db) -- and torch.nn.LSTM in fp32
at the same shape on the same GPU (forward under no_grad, and forward + backward with gradients for the input and the weights) as the outside
yardstick.  --cell gru times keras layers.GRU the same way (gn_gru_fwd / gn_gru_bwd, dU as the layer forms it; --reset-after for that form) against
torch.nn.GRU; its forward results are compared under --reset-after alone, the form torch implements.  One process per shape: 3 warm-up runs, then the median of 11 samples of one run each between two device events.  Prints ms per
run, us per time step, the ratio to torch, and the largest difference between the two forward results on the same weights (sigmoid gates, the
form torch implements).  Each shape runs in a child process under a time limit; ours is timed and printed before torch's is started.
  python scripts/lstm_microbench.py                 # (8, 1024, 64, 64), (64, 256, 64, 128), (512, 128, 128, 256)
  python scripts/lstm_microbench.py B T Cin u       # one shape
  python scripts/lstm_microbench.py --cell gru [--reset-after] [B T Cin u]"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(8, 1024, 64, 64), (64, 256, 64, 128), (512, 128, 128, 256)]
WARMUP, SAMPLES, TIMEOUT_S = 3, 11, 240


def one(B, T, Cin, u, cell='lstm', reset_after=False):
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

    G = 4 if cell == 'lstm' else 3                 # gate column blocks
    rng = np.random.RandomState(0)
    x = torch.tensor(rng.randn(B, T, Cin).astype(np.float32), device=dev)
    W = torch.tensor((rng.randn(Cin, G * u) / np.sqrt(Cin)).astype(np.float32), device=dev)
    U = torch.tensor((rng.randn(u, G * u) / np.sqrt(u)).astype(np.float32), device=dev)
    b = torch.tensor((0.1 * rng.randn(G * u)).astype(np.float32), device=dev)
    dy = torch.tensor(rng.randn(B, T, u).astype(np.float32), device=dev)
    dW, dU, db = torch.empty_like(W), torch.empty_like(U), torch.empty_like(b)
    acts = dict(activation='tanh', recurrent_activation='sigmoid')

    def fwd(training=False):
        zx = ops.bmm(x.view(1, B * T, Cin), W.view(1, Cin, 4 * u)).view(B, T, 4 * u)
        return ops.lstm_fwd(zx, U, b, None, None, training=training, **acts)

    rb = torch.tensor((0.1 * rng.randn(3 * u)).astype(np.float32), device=dev) if reset_after else None
    drb = torch.empty(3 * u, dtype=torch.float32, device=dev)

    def gru_fwd(training=False):
        zx = ops.bmm(x.view(1, B * T, Cin), W.view(1, Cin, 3 * u)).view(B, T, 3 * u)
        return ops.gru_fwd(zx, U, b, rb, None, reset_after=reset_after, training=training, **acts)

    def gru_fwd_bwd():                             # layers.GRU.backward
        h, gates, hprev, aux = gru_fwd(True)
        dz, dzr, _ = ops.gru_bwd(dy, gates, hprev, aux, U, reset_after=reset_after, **acts)
        dz2 = dz.view(B * T, 3 * u)
        rows_product(x.view(B * T, Cin), dz2, dW)
        ops.bias_grad(dz2, db)
        if reset_after:
            dzr2 = dzr.view(B * T, 3 * u)
            rows_product(hprev.view(B * T, u), dzr2, dU)
            ops.bias_grad(dzr2, drb)
        else:
            dz_zr, dz_h = ops.concat_bwd(dz2, [(B * T, 2 * u), (B * T, u)], 1)
            dU_zr, dU_h = dz.new_empty((u, 2 * u)), dz.new_empty((u, u))
            rows_product(hprev.view(B * T, u), dz_zr, dU_zr)
            rows_product(aux.view(B * T, u), dz_h, dU_h)
            ops.concat_fwd([dU_zr, dU_h], 1, out=dU)
        return ops.bmm(dz2.view(1, B * T, 3 * u), W.view(1, Cin, 3 * u), trans_b=True)

    def fwd_bwd():
        h, gates, c, hprev = fwd(True)
        dz, _, _ = ops.lstm_bwd(dy, gates, c, U, None, **acts)
        dz2 = dz.view(B * T, 4 * u)
        rows_product(x.view(B * T, Cin), dz2, dW)
        rows_product(hprev.view(B * T, u), dz2, dU)
        ops.bias_grad(dz2, db)
        return ops.bmm(dz2.view(1, B * T, 4 * u), W.view(1, Cin, 4 * u), trans_b=True)

    if cell == 'gru':
        fwd, fwd_bwd = gru_fwd, gru_fwd_bwd
    print('%s%s shape (B %d, T %d, Cin %d, u %d)' % (cell, ' reset_after' if reset_after else '', B, T, Cin, u), flush=True)
    t_f, t_fb = median_ms(fwd), median_ms(fwd_bwd)
    h_ours = fwd()[0]
    row = {'cell': cell, 'reset_after': bool(reset_after), 'shape': [B, T, Cin, u], 'fwd_ms': t_f, 'fwd_bwd_ms': t_fb}
    print('  gennet_amd   forward %9.3f ms (%7.2f us a step)   forward + backward %9.3f ms (%7.2f us a step)'
          % (t_f, 1e3 * t_f / T, t_fb, 1e3 * t_fb / T), flush=True)

    m = (torch.nn.LSTM if cell == 'lstm' else torch.nn.GRU)(Cin, u, batch_first=True).to(dev)
    perm = torch.arange(G * u, device=dev)
    if cell == 'gru':                              # torch's gate order is r, z, n
        perm = torch.cat([perm[u:2 * u], perm[:u], perm[2 * u:]])
    with torch.no_grad():
        m.weight_ih_l0.copy_(W[:, perm].t())
        m.weight_hh_l0.copy_(U[:, perm].t())
        m.bias_ih_l0.copy_(b[perm])
        if rb is None:
            m.bias_hh_l0.zero_()
        else:
            m.bias_hh_l0.copy_(rb[perm])
    xg = x.clone().requires_grad_(True)

    def t_fwd():
        with torch.no_grad():
            return m(x)[0]

    def t_fwd_bwd():
        m.zero_grad(set_to_none=True)
        xg.grad = None
        m(xg)[0].backward(dy)

    tt_f, tt_fb = median_ms(t_fwd), median_ms(t_fwd_bwd)
    diff = float((t_fwd() - h_ours).abs().max()) if cell == 'lstm' or reset_after else float('nan')      # torch.nn.GRU is the reset_after form
    row.update(torch_fwd_ms=tt_f, torch_fwd_bwd_ms=tt_fb, max_diff=diff)
    print('  torch.nn.%s  forward %9.3f ms (%7.2f us a step)   forward + backward %9.3f ms (%7.2f us a step)'
          % (cell.upper(), tt_f, 1e3 * tt_f / T, tt_fb, 1e3 * tt_fb / T))
    print('  torch / gennet_amd: forward %.2f, forward + backward %.2f;  largest |h - h_torch| %.3g' % (tt_f / t_f, tt_fb / t_fb, diff))
    print(json.dumps(row), flush=True)


def main():
    import argparse
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--cell', choices=('lstm', 'gru'), default='lstm')
    ap.add_argument('--reset-after', action='store_true', help='the reset_after form of the GRU cell')
    ap.add_argument('--one', action='store_true', help='time the one shape in this process (what the parent starts per shape)')
    ap.add_argument('shape', nargs='*', type=int, metavar='B T Cin u')
    a = ap.parse_args()
    if len(a.shape) not in (0, 4) or (a.one and not a.shape) or (a.reset_after and a.cell != 'gru'):
        ap.error('a shape is the four numbers B T Cin u; --reset-after goes with --cell gru')
    if a.one:
        return one(*a.shape, cell=a.cell, reset_after=a.reset_after)
    flags = ['--cell', a.cell] + (['--reset-after'] if a.reset_after else [])
    for s in [tuple(a.shape)] if a.shape else SHAPES:
        try:          # a fresh child per shape under a time limit; after a run that hangs or fails nothing more is started
            r = subprocess.run([sys.executable, os.path.abspath(__file__), '--one'] + flags + [str(v) for v in s], timeout=TIMEOUT_S)
        except subprocess.TimeoutExpired:
            print('shape %r: no result within %d s' % (s, TIMEOUT_S), flush=True)
            return 1
        if r.returncode:
            print('shape %r: exit status %d' % (s, r.returncode), flush=True)
            return r.returncode
    return 0


if __name__ == '__main__':
    sys.exit(main())
