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
  python scripts/lstm_microbench.py --cell gru [--reset-after] [B T Cin u]
--bidirectional times keras layers.Bidirectional's arithmetic (merge_mode 'concat', sequences) the same way, for either cell and both GRU forms:
  (a) the pair launch (gn_lstm_pair_fwd / _bwd, gn_gru_pair_fwd / _bwd: both directions as one grid, written straight into the merged layout);
  (b) the two single-direction entry points one after the other on the same operands -- the same bits, which is checked -- WITHOUT the reverse
      and concatenate passes a layer built on them would add, so (a) / (b) is the launch against the two launches and nothing else;
  (c) torch.nn.LSTM / torch.nn.GRU(bidirectional=True) in fp32.
The products around the recurrence (two input projections, the weight gradients a direction, dX) are the same calls in (a) and (b).
  python scripts/lstm_microbench.py --bidirectional [--cell gru [--reset-after]] [B T Cin u]
--cell rnn times keras layers.SimpleRNN (gn_rnn_fwd / gn_rnn_bwd; with --bidirectional gn_rnn_pair_fwd / _bwd against two single launches) against
fp32 torch.nn.RNN and, in the same process on the same x, against this project's GRU with reset_after=True, the one-product form of the same
scheme with three gate blocks:
  python scripts/lstm_microbench.py --cell rnn [--bidirectional] [B T Cin u]"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(8, 1024, 64, 64), (64, 256, 64, 128), (512, 128, 128, 256)]
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


def one_bidirectional(B, T, Cin, u, cell='lstm', reset_after=False):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from gennet_amd import ops
    from gennet_amd.engine import device
    from gennet_amd.recurrent import rows_product
    dev = device()
    G = 4 if cell == 'lstm' else 3
    rng = np.random.RandomState(0)
    t = lambda a: torch.tensor(a.astype(np.float32), device=dev)          # noqa: E731
    x = t(rng.randn(B, T, Cin))
    W = [t(rng.randn(Cin, G * u) / np.sqrt(Cin)) for _ in range(2)]
    U = [t(rng.randn(u, G * u) / np.sqrt(u)) for _ in range(2)]
    b = [t(0.1 * rng.randn(G * u)) for _ in range(2)]
    rb = [t(0.1 * rng.randn(G * u)) for _ in range(2)] if reset_after else None
    dy = t(rng.randn(B, T, 2 * u))
    dy_single = [dy[..., :u].contiguous(), dy[..., u:].flip(1).contiguous()]          # (b)'s gradients in processing order, formed outside the timing
    dW, dU, db, drb = ([torch.empty_like(v) for v in vs] for vs in (W, U, b, b))
    acts = dict(activation='tanh', recurrent_activation='sigmoid')

    def project():
        return [ops.bmm(x.view(1, B * T, Cin), W[d].view(1, Cin, G * u)).view(B, T, G * u) for d in range(2)]

    def weight_grads(d, hprev, last, dz, dzr):              # a direction's share of layers.LSTM.backward / layers.GRU.backward
        dz2 = dz.view(B * T, G * u)
        rows_product(x.view(B * T, Cin), dz2, dW[d])
        ops.bias_grad(dz2, db[d])
        if cell == 'lstm':
            rows_product(hprev.view(B * T, u), dz2, dU[d])
        elif reset_after:
            dzr2 = dzr.view(B * T, 3 * u)
            rows_product(hprev.view(B * T, u), dzr2, dU[d])
            ops.bias_grad(dzr2, drb[d])
        else:
            dz_zr, dz_h = ops.concat_bwd(dz2, [(B * T, 2 * u), (B * T, u)], 1)
            dU_zr, dU_h = dz.new_empty((u, 2 * u)), dz.new_empty((u, u))
            rows_product(hprev.view(B * T, u), dz_zr, dU_zr)
            rows_product(last.view(B * T, u), dz_h, dU_h)
            ops.concat_fwd([dU_zr, dU_h], 1, out=dU[d])
        return ops.bmm(dz2.view(1, B * T, G * u), W[d].view(1, Cin, G * u), trans_b=True)

    def pair(training=False):                               # (a)
        if cell == 'lstm':
            y, _, gates, last, hprev = ops.lstm_pair_fwd(project(), U, b, training=training, **acts)
        else:
            y, _, gates, hprev, last = ops.gru_pair_fwd(project(), U, b, rb, reset_after=reset_after, training=training, **acts)
        return y, gates, hprev, last

    def pair_fwd_bwd():
        y, gates, hprev, last = pair(True)
        if cell == 'lstm':
            dz, dzr = ops.lstm_pair_bwd(dy, gates, last, U, **acts), None
        else:
            dz, dzr = ops.gru_pair_bwd(dy, gates, hprev, last, U, reset_after=reset_after, **acts)
        dx = [weight_grads(d, hprev[d], last[d], dz[d], dzr[d] if dzr else None) for d in range(2)]
        return ops.merge_fwd('add', dx), dz

    def two(training=False):                                # (b)
        zx, out = project(), []
        for d in range(2):
            if cell == 'lstm':
                h, gates, last, hprev = ops.lstm_fwd(zx[d], U[d], b[d], None, None, reverse=bool(d), training=training, **acts)
            else:
                h, gates, hprev, last = ops.gru_fwd(zx[d], U[d], b[d], rb[d] if rb else None, None, reset_after=reset_after, reverse=bool(d),
                                                    training=training, **acts)
            out.append((h, gates, hprev, last))
        return out

    def two_fwd_bwd():
        dx, dzs = [], []
        for d, (h, gates, hprev, last) in enumerate(two(True)):
            if cell == 'lstm':
                dz, dzr = ops.lstm_bwd(dy_single[d], gates, last, U[d], None, reverse=bool(d), **acts)[0], None
            else:
                dz, dzr, _ = ops.gru_bwd(dy_single[d], gates, hprev, last, U[d], reset_after=reset_after, reverse=bool(d), **acts)
            dx.append(weight_grads(d, hprev, last, dz, dzr))
            dzs.append(dz)
        return ops.merge_fwd('add', dx), dzs

    what = 'bidirectional %s%s' % (cell, ' reset_after' if reset_after else '')
    print('%s shape (B %d, T %d, Cin %d, u %d)' % (what, B, T, Cin, u), flush=True)
    a_f, a_fb = median_ms(pair), median_ms(pair_fwd_bwd)
    b_f, b_fb = median_ms(two), median_ms(two_fwd_bwd)
    y = pair()[0]
    hf, hb = (r[0] for r in two())
    (dxa, dza), (dxb, dzb) = pair_fwd_bwd(), two_fwd_bwd()
    equal = bool(torch.equal(y[..., :u], hf) and torch.equal(y[..., u:], hb.flip(1)) and torch.equal(dxa, dxb)
                 and all(torch.equal(p, q) for p, q in zip(dza, dzb)))
    row = {'bidirectional': True, 'cell': cell, 'reset_after': bool(reset_after), 'shape': [B, T, Cin, u], 'pair_fwd_ms': a_f, 'pair_fwd_bwd_ms': a_fb,
           'two_fwd_ms': b_f, 'two_fwd_bwd_ms': b_fb, 'equal_bits': equal}
    print('  (a) pair launch      forward %9.3f ms   forward + backward %9.3f ms' % (a_f, a_fb))
    print('  (b) two launches     forward %9.3f ms   forward + backward %9.3f ms' % (b_f, b_fb))
    print('  (a) / (b): forward %.3f, forward + backward %.3f;  the same bits: %s' % (a_f / b_f, a_fb / b_fb, equal), flush=True)

    m = (torch.nn.LSTM if cell == 'lstm' else torch.nn.GRU)(Cin, u, batch_first=True, bidirectional=True).to(dev)
    perm = torch.arange(G * u, device=dev)
    if cell == 'gru':                              # torch's gate order is r, z, n
        perm = torch.cat([perm[u:2 * u], perm[:u], perm[2 * u:]])
    with torch.no_grad():
        for d, suffix in enumerate(('', '_reverse')):
            getattr(m, 'weight_ih_l0' + suffix).copy_(W[d][:, perm].t())
            getattr(m, 'weight_hh_l0' + suffix).copy_(U[d][:, perm].t())
            getattr(m, 'bias_ih_l0' + suffix).copy_(b[d][perm])
            if rb is None:
                getattr(m, 'bias_hh_l0' + suffix).zero_()
            else:
                getattr(m, 'bias_hh_l0' + suffix).copy_(rb[d][perm])
    xg = x.clone().requires_grad_(True)

    def t_fwd():
        with torch.no_grad():
            return m(x)[0]

    def t_fwd_bwd():
        m.zero_grad(set_to_none=True)
        xg.grad = None
        m(xg)[0].backward(dy)

    c_f, c_fb = median_ms(t_fwd), median_ms(t_fwd_bwd)
    diff = float((t_fwd() - y).abs().max()) if cell == 'lstm' or reset_after else float('nan')      # torch.nn.GRU is the reset_after form
    row.update(torch_fwd_ms=c_f, torch_fwd_bwd_ms=c_fb, max_diff=diff)
    print('  (c) torch.nn.%s   forward %9.3f ms   forward + backward %9.3f ms' % (cell.upper(), c_f, c_fb))
    print('  (c) / (a): forward %.2f, forward + backward %.2f;  largest |y - y_torch| %.3g' % (c_f / a_f, c_fb / a_fb, diff))
    print(json.dumps(row), flush=True)


def one_rnn(B, T, Cin, u, bidirectional=False):
    """keras layers.SimpleRNN, one direction or Bidirectional (concat, sequences), beside torch.nn.RNN and this project's GRU (reset_after=True)"""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from gennet_amd import ops
    from gennet_amd.engine import device
    from gennet_amd.recurrent import rows_product
    dev = device()
    nd = 2 if bidirectional else 1
    rng = np.random.RandomState(0)
    t = lambda a: torch.tensor(a.astype(np.float32), device=dev)          # noqa: E731
    x = t(rng.randn(B, T, Cin))
    W = [t(rng.randn(Cin, u) / np.sqrt(Cin)) for _ in range(nd)]
    U = [t(rng.randn(u, u) / np.sqrt(u)) for _ in range(nd)]
    b = [t(0.1 * rng.randn(u)) for _ in range(nd)]
    dy = t(rng.randn(B, T, nd * u))
    dy_single = [dy[..., :u].contiguous()] + ([dy[..., u:].flip(1).contiguous()] if bidirectional else [])
    dW, dU, db = ([torch.empty_like(v) for v in vs] for vs in (W, U, b))
    # the GRU beside it: the same x, three gate blocks
    Wg = [t(rng.randn(Cin, 3 * u) / np.sqrt(Cin)) for _ in range(nd)]
    Ug = [t(rng.randn(u, 3 * u) / np.sqrt(u)) for _ in range(nd)]
    bg, rbg = ([t(0.1 * rng.randn(3 * u)) for _ in range(nd)] for _ in range(2))
    dWg, dUg, dbg, drbg = ([torch.empty_like(v) for v in vs] for vs in (Wg, Ug, bg, rbg))
    gacts = dict(activation='tanh', recurrent_activation='sigmoid', reset_after=True)

    def project(Ws, G):
        return [ops.bmm(x.view(1, B * T, Cin), w.view(1, Cin, G * u)).view(B, T, G * u) for w in Ws]

    def rnn_grads(d, hprev, dz):                             # a direction's share of layers.SimpleRNN.backward
        dz2 = dz.view(B * T, u)
        rows_product(x.view(B * T, Cin), dz2, dW[d])
        rows_product(hprev.view(B * T, u), dz2, dU[d])
        ops.bias_grad(dz2, db[d])
        return ops.bmm(dz2.view(1, B * T, u), W[d].view(1, Cin, u), trans_b=True)

    def gru_grads(d, hprev, dz, dzr):                        # a direction's share of layers.GRU.backward under reset_after
        dz2, dzr2 = dz.view(B * T, 3 * u), dzr.view(B * T, 3 * u)
        rows_product(x.view(B * T, Cin), dz2, dWg[d])
        ops.bias_grad(dz2, dbg[d])
        rows_product(hprev.view(B * T, u), dzr2, dUg[d])
        ops.bias_grad(dzr2, drbg[d])
        return ops.bmm(dz2.view(1, B * T, 3 * u), Wg[d].view(1, Cin, 3 * u), trans_b=True)

    def fwd(training=False):                                 # one launch: the single entry point, or the pair
        zx = project(W, 1)
        if bidirectional:
            y, _, hs, hprev = ops.rnn_pair_fwd(zx, U, b, training=training)
            return y, hs, hprev
        h, hs, hprev = ops.rnn_fwd(zx[0], U[0], b[0], None, training=training)
        return h, [hs], [hprev]

    def fwd_bwd():
        y, hs, hprev = fwd(True)
        dz = ops.rnn_pair_bwd(dy, hs, U) if bidirectional else [ops.rnn_bwd(dy, hs[0], U[0])[0]]
        dx = [rnn_grads(d, hprev[d], dz[d]) for d in range(nd)]
        return (ops.merge_fwd('add', dx) if bidirectional else dx[0]), dz

    def two(training=False):                                 # --bidirectional: the two single launches on the same operands
        zx = project(W, 1)
        return [ops.rnn_fwd(zx[d], U[d], b[d], None, reverse=bool(d), training=training) for d in range(2)]

    def two_fwd_bwd():
        dx, dzs = [], []
        for d, (h, hs, hprev) in enumerate(two(True)):
            dz = ops.rnn_bwd(dy_single[d], hs, U[d], reverse=bool(d))[0]
            dx.append(rnn_grads(d, hprev, dz))
            dzs.append(dz)
        return ops.merge_fwd('add', dx), dzs

    def gru_fwd(training=False):
        zx = project(Wg, 3)
        if bidirectional:
            y, _, gates, hprev, aux = ops.gru_pair_fwd(zx, Ug, bg, rbg, training=training, **gacts)
            return y, gates, hprev, aux
        h, gates, hprev, aux = ops.gru_fwd(zx[0], Ug[0], bg[0], rbg[0], None, training=training, **gacts)
        return h, [gates], [hprev], [aux]

    def gru_fwd_bwd():
        y, gates, hprev, aux = gru_fwd(True)
        if bidirectional:
            dz, dzr = ops.gru_pair_bwd(dy, gates, hprev, aux, Ug, **gacts)
        else:
            dz, dzr, _ = ops.gru_bwd(dy, gates[0], hprev[0], aux[0], Ug[0], **gacts)
            dz, dzr = [dz], [dzr]
        dx = [gru_grads(d, hprev[d], dz[d], dzr[d]) for d in range(nd)]
        return ops.merge_fwd('add', dx) if bidirectional else dx[0]

    what = 'bidirectional rnn' if bidirectional else 'rnn'
    print('%s shape (B %d, T %d, Cin %d, u %d)' % (what, B, T, Cin, u), flush=True)
    t_f, t_fb = median_ms(fwd), median_ms(fwd_bwd)
    row = {'cell': 'rnn', 'bidirectional': bool(bidirectional), 'shape': [B, T, Cin, u], 'fwd_ms': t_f, 'fwd_bwd_ms': t_fb}
    print('  gennet_amd SimpleRNN   forward %9.3f ms (%7.2f us a step)   forward + backward %9.3f ms (%7.2f us a step)'
          % (t_f, 1e3 * t_f / T, t_fb, 1e3 * t_fb / T), flush=True)
    y_ours = fwd()[0]
    if bidirectional:
        b_f, b_fb = median_ms(two), median_ms(two_fwd_bwd)
        hf, hb = (r[0] for r in two())
        (dxa, dza), (dxb, dzb) = fwd_bwd(), two_fwd_bwd()
        equal = bool(torch.equal(y_ours[..., :u], hf) and torch.equal(y_ours[..., u:], hb.flip(1)) and torch.equal(dxa, dxb)
                     and all(torch.equal(p, q) for p, q in zip(dza, dzb)))
        row.update(two_fwd_ms=b_f, two_fwd_bwd_ms=b_fb, equal_bits=equal)
        print('  two single launches    forward %9.3f ms   forward + backward %9.3f ms' % (b_f, b_fb))
        print('  pair / two: forward %.3f, forward + backward %.3f;  the same bits: %s' % (t_f / b_f, t_fb / b_fb, equal), flush=True)
    g_f, g_fb = median_ms(gru_fwd), median_ms(gru_fwd_bwd)
    row.update(gru_fwd_ms=g_f, gru_fwd_bwd_ms=g_fb)
    print('  gennet_amd GRU (ra=1)  forward %9.3f ms (%7.2f us a step)   forward + backward %9.3f ms (%7.2f us a step)'
          % (g_f, 1e3 * g_f / T, g_fb, 1e3 * g_fb / T))
    print('  SimpleRNN / GRU: forward %.3f, forward + backward %.3f' % (t_f / g_f, t_fb / g_fb), flush=True)

    m = torch.nn.RNN(Cin, u, nonlinearity='tanh', batch_first=True, bidirectional=bool(bidirectional)).to(dev)
    with torch.no_grad():
        for d, suffix in enumerate(('', '_reverse')[:nd]):
            getattr(m, 'weight_ih_l0' + suffix).copy_(W[d].t())
            getattr(m, 'weight_hh_l0' + suffix).copy_(U[d].t())
            getattr(m, 'bias_ih_l0' + suffix).copy_(b[d])
            getattr(m, 'bias_hh_l0' + suffix).zero_()
    xg = x.clone().requires_grad_(True)

    def t_fwd():
        with torch.no_grad():
            return m(x)[0]

    def t_fwd_bwd():
        m.zero_grad(set_to_none=True)
        xg.grad = None
        m(xg)[0].backward(dy)

    tt_f, tt_fb = median_ms(t_fwd), median_ms(t_fwd_bwd)
    diff = float((t_fwd() - y_ours).abs().max())
    row.update(torch_fwd_ms=tt_f, torch_fwd_bwd_ms=tt_fb, max_diff=diff)
    print('  torch.nn.RNN           forward %9.3f ms (%7.2f us a step)   forward + backward %9.3f ms (%7.2f us a step)'
          % (tt_f, 1e3 * tt_f / T, tt_fb, 1e3 * tt_fb / T))
    print('  torch / gennet_amd: forward %.2f, forward + backward %.2f;  largest |y - y_torch| %.3g' % (tt_f / t_f, tt_fb / t_fb, diff))
    print(json.dumps(row), flush=True)


def one(B, T, Cin, u, cell='lstm', reset_after=False):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from gennet_amd import ops
    from gennet_amd.engine import device
    from gennet_amd.recurrent import rows_product
    dev = device()

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
    ap.add_argument('--cell', choices=('lstm', 'gru', 'rnn'), default='lstm')
    ap.add_argument('--reset-after', action='store_true', help='the reset_after form of the GRU cell')
    ap.add_argument('--bidirectional', action='store_true', help="keras layers.Bidirectional: the pair launch against two single launches and torch")
    ap.add_argument('--one', action='store_true', help='time the one shape in this process (what the parent starts per shape)')
    ap.add_argument('shape', nargs='*', type=int, metavar='B T Cin u')
    a = ap.parse_args()
    if len(a.shape) not in (0, 4) or (a.one and not a.shape) or (a.reset_after and a.cell != 'gru'):
        ap.error('a shape is the four numbers B T Cin u; --reset-after goes with --cell gru')
    if a.one and a.cell == 'rnn':
        return one_rnn(*a.shape, bidirectional=a.bidirectional)
    if a.one:
        return (one_bidirectional if a.bidirectional else one)(*a.shape, cell=a.cell, reset_after=a.reset_after)
    flags = ['--cell', a.cell] + (['--reset-after'] if a.reset_after else []) + (['--bidirectional'] if a.bidirectional else [])
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
