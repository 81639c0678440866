"""Conv2DTranspose (gennet_amd.layers.Conv2DTranspose) against the Conv1D launches of its adjoint shape, which run the same kernels.

Layers: the four Conv2DTranspose layers of the reference's g_model.hdf5 at batch 512, and a BBH-sized stride-2 layer,
Conv2DTranspose(512, (1, 5), strides=(1, 2), padding='same') on (B, 1, 1024, 1024), whose adjoint is the PE net's last Conv1D(1024, 5,
strides=2).  Per layer and direction, timed with HIP events around `--reps` calls after `--warmup` calls:
  fwd    the layer's forward (adjoint data gradient + the bias / activation pass of csrc/conv_transpose.hip)  vs  gn_conv1d_dgrad alone
  dgrad  the layer's data gradient                                                                            vs  gn_conv1d_fwd (no bias)
  wgrad  the layer's weight + bias gradient                                                                   vs  gn_conv1d_wgrad
and the bias / activation pass by itself as HBM bytes / s (8 bytes per element: one read, one write) and the fraction of the measured
6.29 TB/s copy rate.  One JSON line per layer; the last line checks the forward against "data gradient + one pass at 0.7 of HBM"."""
import argparse
import json
import os
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=512, help="g_model layers' batch")
    ap.add_argument('--bbh-batch', type=int, default=32, help="the BBH-sized layer's batch")
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--only', default='', help='run the layers whose name contains this text (a profiler run of one layer)')
    args = ap.parse_args()
    import torch
    from gennet_amd import ops, layers as L
    from gennet_amd.engine import RunContext
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    cases = [('g_model conv2d_transpose_1', args.batch, 1, 1, 1, 128, 4, 1, 'valid'),
             ('g_model conv2d_transpose_2', args.batch, 1, 4, 128, 64, 8, 1, 'valid'),
             ('g_model conv2d_transpose_3', args.batch, 1, 11, 64, 32, 16, 1, 'valid'),
             ('g_model conv2d_transpose_4', args.batch, 1, 26, 32, 16, 32, 1, 'valid'),
             ('BBH Conv2DTranspose(512, (1,5), (1,2), same)', args.bbh_batch, 1, 1024, 1024, 512, 5, 2, 'same')]
    ok = True
    for name, B, H, W, Cin, Fl, kw, s, padding in [c for c in cases if args.only in c[0]]:
        layer = L.Conv2DTranspose(Fl, (1, kw), strides=(1, s), padding=padding, activation='relu')
        layer.build((H, W, Cin))
        layer.kernel.grad = torch.zeros(layer.kernel.shape, device=dev)
        layer.bias.grad = torch.zeros(layer.bias.shape, device=dev)
        Wout = layer.out_length(W)
        _, pl = ops.conv_geometry(Wout, kw, s, padding)
        x = torch.randn(B, H, W, Cin, device=dev)
        dy = torch.randn(B, H, Wout, Fl, device=dev)
        node = types.SimpleNamespace(index=0, fused_act=None, fused_drop=None)
        wadj = layer.kernel.data.view(kw, Fl, Cin)
        x3, dy3 = x.view(B * H, W, Cin), dy.view(B * H, Wout, Fl)

        def fwd():
            ctx = RunContext(True)
            layer.forward(ctx, node, x)

        ctx0 = RunContext(True)
        layer.forward(ctx0, node, x)
        saved = [ctx0.tape[0]]

        def layer_dx():
            ctx = RunContext(True); ctx.tape[0] = saved[0]
            layer.backward(ctx, node, dy, True, False)

        def layer_dw():
            ctx = RunContext(True); ctx.tape[0] = saved[0]
            layer.backward(ctx, node, dy, False, True)

        if kw > 5:
            w2 = ops.conv1d_tapfold_w(wadj); wt2 = ops.conv1d_transpose_w(w2); h = ops.tap_groups(kw)[1]
            adj_dgrad = lambda: ops.conv1d_tapunfold_dx(ops.conv1d_dgrad(x3, wt2, Wout + pl, s, 0), Wout, kw, pl)         # noqa: E731
            adj_fwd = lambda: ops.conv1d_fwd(ops.conv1d_tapfold_x(dy3, kw, pl), w2, None, s, 0, W)                       # noqa: E731
            adj_wgrad = lambda: ops.conv1d_wgrad(ops.conv1d_tapfold_x(dy3, kw, pl), x3, h, s, 0, want_db=False)                         # noqa: E731
        else:
            wt = ops.conv1d_transpose_w(wadj)
            adj_dgrad = lambda: ops.conv1d_dgrad(x3, wt, Wout, s, pl)                                                     # noqa: E731
            adj_fwd = lambda: ops.conv1d_fwd(dy3, wadj, None, s, pl, W)                                                   # noqa: E731
            adj_wgrad = lambda: ops.conv1d_wgrad(dy3, x3, kw, s, pl, want_db=False)                                                      # noqa: E731
        y = adj_dgrad()
        bias_pass = lambda: ops.bias_act_dropout(y, layer.bias.data, 'relu')                                              # noqa: E731
        t = {k: timed(f, args.warmup, args.reps) for k, f in (('fwd', fwd), ('dgrad', layer_dx), ('wgrad', layer_dw), ('adj_dgrad', adj_dgrad),
                                                               ('adj_fwd', adj_fwd), ('adj_wgrad', adj_wgrad), ('bias_pass', bias_pass))}
        n = y.numel()
        bias_tbs = 8 * n / (t['bias_pass'] * 1e-3) / 1e12
        budget = t['adj_dgrad'] + 8 * n / (0.7 * HBM_TBS * 1e12) * 1e3
        ok = ok and t['fwd'] <= budget * 1.03
        print(json.dumps({'layer': name, 'in': [B, H, W, Cin], 'out': [B, H, Wout, Fl], 'ms': {k: round(v, 4) for k, v in t.items()},
                          'bias_pass_TB_per_s': round(bias_tbs, 3), 'bias_pass_fraction_of_hbm': round(bias_tbs / HBM_TBS, 3),
                          'fwd_budget_ms': round(budget, 4), 'fwd_within_budget': t['fwd'] <= budget * 1.03}), flush=True)
    print(json.dumps({'summary': 'forward <= adjoint data gradient + one output pass at 0.7 of HBM (3 % timing spread)', 'ok': ok}), flush=True)
    return 0


if __name__ == '__main__':
    sys.exit(main())
