#!/usr/bin/env python
"""Time keras layers.SeparableConv1D's arithmetic at (B, L, Cin, k, dm, filters), padding 'same', stride 1, relu:
  * the three depthwise kernels of csrc/depthwise.hip one by one: the bytes the algorithm needs (every operand once: x + w + y, dy + w + dx,
    x + dy + dw, computed from the shape) over the kernel's time, beside the rate of a device-to-device copy that moves the same number of bytes
    (half read, half written), timed in the same process -- the streaming rate the card gives that byte count;
  * the whole layer as gennet_amd/separable.py runs it, forward (inference phase) and forward + backward (all three weight gradients and dx);
  * fp32 torch on the same card: F.conv1d(groups=Cin) then a 1 x 1 F.conv1d, in torch's own channels-first layout, no transposes in the window;
  * this project's dense Conv1D(filters, k) of the same (Cin, filters, k), as layers.Conv1D launches it (tap-folded past 5 taps).
One process per shape: 3 warm-up runs, then the median of 11 samples of one run each between two device events.  Each shape runs in a child
process under a time limit; every figure is printed as soon as it is measured, and one JSON line a shape at the end.
  python scripts/sepconv_microbench.py                          # (64, 2048, 64, 16, 1, 128), (16, 8192, 256, 5, 1, 256), (256, 2048, 8, 16, 2, 64)
  python scripts/sepconv_microbench.py B L Cin k dm filters     # one shape"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(64, 2048, 64, 16, 1, 128), (16, 8192, 256, 5, 1, 256), (256, 2048, 8, 16, 2, 64)]
WARMUP, SAMPLES, TIMEOUT_S = 3, 11, 240


def median_ms(fn):
    import torch
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


def kernel_bytes(B, L, Lout, C, k, dm):
    """bytes each depthwise kernel needs: every operand once"""
    x, y, w = B * L * C, B * Lout * C * dm, k * C * dm
    return {'fwd': 4 * (x + w + y), 'dgrad': 4 * (y + w + x), 'wgrad': 4 * (x + y + w)}


def one(B, L, Cin, k, dm, filters):
    import numpy as np
    import torch
    import torch.nn.functional as F
    sys.path.insert(0, ROOT)
    from gennet_amd import layers as Ly, ops
    from gennet_amd.engine import device
    from gennet_amd.recurrent import rows_product
    dev = device()
    rng = np.random.RandomState(0)
    t = lambda a: torch.tensor(np.asarray(a, np.float32), device=dev)          # noqa: E731
    Cm, rows = Cin * dm, B * L
    x, dy = t(rng.randn(B, L, Cin)), t(rng.randn(B, L, filters))
    w, P, b = t(rng.randn(k, Cin, dm) / np.sqrt(k)), t(rng.randn(1, Cm, filters) / np.sqrt(Cm)), t(0.1 * rng.randn(filters))
    dt0 = t(rng.randn(B, L, Cm))
    dw, dP, db = torch.empty_like(w), torch.empty_like(P), torch.empty_like(b)
    row = {'shape': [B, L, Cin, k, dm, filters]}
    print('separable shape (B %d, L %d, Cin %d, k %d, dm %d, filters %d)' % (B, L, Cin, k, dm, filters), flush=True)

    # the three kernels against a copy of the same byte count
    nbytes = kernel_bytes(B, L, L, Cin, k, dm)
    runs = {'fwd': lambda: ops.dwconv1d_fwd(x, w, 1, 'same'), 'dgrad': lambda: ops.dwconv1d_dgrad(dt0, w, L, 1, 'same'),
            'wgrad': lambda: ops.dwconv1d_wgrad(x, dt0, k, 1, 'same', dw=dw)}
    for name in ('fwd', 'dgrad', 'wgrad'):
        ms = median_ms(runs[name])
        src = torch.empty(nbytes[name] // 8, dtype=torch.float32, device=dev).normal_()
        dst = torch.empty_like(src)
        copy_ms = median_ms(lambda: dst.copy_(src))
        row.update({name + '_ms': ms, name + '_bytes': nbytes[name], name + '_TBps': nbytes[name] / ms * 1e-9, name + '_copy_TBps': nbytes[name] / copy_ms * 1e-9})
        print('  dwconv1d_%-5s %9.3f ms  %7.1f MB needed  %6.2f TB/s;  a copy of the same bytes %9.3f ms  %6.2f TB/s  (kernel / copy %.2f)'
              % (name, ms, nbytes[name] * 1e-6, row[name + '_TBps'], copy_ms, row[name + '_copy_TBps'], ms / copy_ms), flush=True)
        del src, dst

    # the layer as gennet_amd/separable.py runs it
    def fwd(training=False):
        tt = ops.dwconv1d_fwd(x, w, 1, 'same')
        y = ops.bmm(tt.view(1, rows, Cm), P.view(1, Cm, filters)).view(B, L, filters)
        return tt, ops.bias_act_dropout(y, b, 'relu', 0.0)

    def fwd_bwd():
        tt, y = fwd(True)
        g = ops.act_bwd(dy.clone(), y, 'relu', 0.0, inplace=True).view(rows, filters)
        rows_product(tt.view(rows, Cm), g, dP.view(Cm, filters))
        ops.bias_grad(g, db)
        dtt = ops.bmm(g.view(1, rows, filters), P.view(1, Cm, filters), trans_b=True).view(B, L, Cm)
        ops.dwconv1d_wgrad(x, dtt, k, 1, 'same', dw=dw)
        return ops.dwconv1d_dgrad(dtt, w, L, 1, 'same')

    t_f, t_fb = median_ms(fwd), median_ms(fwd_bwd)
    pw_ms = median_ms(lambda: ops.bmm(dt0.view(1, rows, Cm), P.view(1, Cm, filters)))
    row.update(layer_fwd_ms=t_f, layer_fwd_bwd_ms=t_fb, pointwise_fwd_ms=pw_ms, pointwise_TFLOPs=2.0 * rows * Cm * filters / pw_ms * 1e-9)
    print('  gennet_amd layer   forward %9.3f ms   forward + backward %9.3f ms   (the pointwise product alone %9.3f ms, %.1f TFLOP/s)'
          % (t_f, t_fb, pw_ms, row['pointwise_TFLOPs']), flush=True)
    y_ours = fwd()[1]

    # torch, channels first
    xc = x.permute(0, 2, 1).contiguous()
    dyc = dy.permute(0, 2, 1).contiguous()
    wc = w.permute(1, 2, 0).reshape(Cm, 1, k).contiguous().requires_grad_(True)
    pc = P.permute(2, 1, 0).contiguous().requires_grad_(True)
    bc = b.clone().requires_grad_(True)
    xg = xc.clone().requires_grad_(True)

    def t_layer(inp):
        return torch.relu(F.conv1d(F.conv1d(inp, wc, padding='same', groups=Cin), pc, bc))

    def t_fwd():
        with torch.no_grad():
            return t_layer(xc)

    def t_fwd_bwd():
        for v in (wc, pc, bc, xg):
            v.grad = None
        t_layer(xg).backward(dyc)

    tt_f, tt_fb = median_ms(t_fwd), median_ms(t_fwd_bwd)
    diff = float((t_fwd().permute(0, 2, 1) - y_ours).abs().max())
    row.update(torch_fwd_ms=tt_f, torch_fwd_bwd_ms=tt_fb, max_diff=diff)
    print('  torch fp32         forward %9.3f ms   forward + backward %9.3f ms' % (tt_f, tt_fb))
    print('  torch / gennet_amd: forward %.2f, forward + backward %.2f;  largest |y - y_torch| %.3g' % (tt_f / t_f, tt_fb / t_fb, diff), flush=True)

    # this project's dense Conv1D(filters, k) on the same input, as layers.Conv1D launches it
    conv = Ly.Conv1D(filters, k, padding='same', activation='relu')
    conv._ensure_built((L, Cin))
    run = Ly._ConvRun(conv, Cin, False, L)
    cw, cb = conv.kernel.data, conv.bias.data
    cdw, cdb = torch.empty_like(cw), torch.empty_like(cb)
    launch = lambda *c: ops.conv1d_fwd(*c, 'relu', 0.0, any_channels=run.any_channels)          # noqa: E731

    def c_fwd():
        return Ly._kconv_fwd(x, cw, cb, run.stride, run.pl, run.Lout, launch)

    def c_fwd_bwd():
        y, xf, wf = c_fwd()
        g = ops.act_bwd(dy.clone(), y, 'relu', 0.0, inplace=True)
        Ly._kconv_wgrad(xf, g, run.k, run.stride, run.pl, cdw, cdb, any_channels=run.any_channels, folded=True)
        return Ly._kconv_dgrad(g, wf, run.k, run.L, run.stride, run.pl, None, run.any_channels, folded=True)

    c_f, c_fb = median_ms(c_fwd), median_ms(c_fwd_bwd)
    row.update(dense_fwd_ms=c_f, dense_fwd_bwd_ms=c_fb)
    print('  dense Conv1D       forward %9.3f ms   forward + backward %9.3f ms;  dense / separable: forward %.2f, forward + backward %.2f'
          % (c_f, c_fb, c_f / t_f, c_fb / t_fb))
    print(json.dumps(row), flush=True)


def main():
    import argparse
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--one', action='store_true', help='time the one shape in this process (what the parent starts per shape)')
    ap.add_argument('shape', nargs='*', type=int, metavar='B L Cin k dm filters')
    a = ap.parse_args()
    if len(a.shape) not in (0, 6) or (a.one and not a.shape):
        ap.error('a shape is the six numbers B L Cin k dm filters')
    if a.one:
        return one(*a.shape)
    for s in [tuple(a.shape)] if a.shape else SHAPES:
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
