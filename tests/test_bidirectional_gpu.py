"""GPU tests of keras layers.Bidirectional: the pair entry points gn_lstm_pair_fwd / _bwd and gn_gru_pair_fwd / _bwd, which run both
directions as the second dimension of one grid, and the layer at model level.

Section 1, kernel level.  The single-direction entry points are held against the fp64 definitions in tests/test_lstm_gpu.py and
tests/test_gru_gpu.py; here they are the oracle: each direction of a pair launch must have, BIT FOR BIT, what the single entry point gives on the
same operands -- h after re-indexing (direction 1 writes step s at position T-1-s), the stored tensors, dz and dzr.  The pair runs on guarded
buffers (tests/test_lstm_gpu.py's Guarded), in the concatenated layout (one (B, [T,] 2u) buffer, ld = 2u) and in the split one (two buffers,
ld = u).  SHAPES (B, T, u): B over {1, 15, 16, 17, 33} (16 batch rows a block), T over {1, 2, 3, 17}, u on both sides of every geometry edge:
1, 16 | 17 (one tile, two), the LDS | streamed switch of the LSTM backward (80 | 81) and forward (88 | 89) and of both GRU kernels (104 | 105,
derived below from the restated geometry), 130 (two tiles a wave) and 512 (the largest, four tiles a wave); B T <= 600.
Section 2, model level: tests/test_lstm_gpu.py's train_and_compare as it stands (predict 1e-5, loss 1e-6, gradients and weights 1e-4), against
tests/bidirectional_ref.py in torch fp64, three SGD steps."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bidirectional_ref as BR
from test_gru_gpu import geometry as gru_geometry
from test_lstm_gpu import LR, Guarded, dev, geometry as lstm_geometry, same_bits, train_and_compare

pytestmark = pytest.mark.gpu

# (B, T, u)
SHAPES = [(1, 1, 1), (15, 2, 16), (16, 3, 17), (17, 17, 80), (33, 1, 81), (1, 2, 88), (15, 3, 89), (16, 17, 104), (17, 1, 105), (33, 2, 130),
          (1, 3, 512), (33, 17, 16)]
IDS = ['b%d-t%d-u%d' % s for s in SHAPES]
CELLS = [('lstm', False), ('gru', False), ('gru', True)]
CELL_IDS = ['lstm', 'gru-ra0', 'gru-ra1']


@pytest.fixture(autouse=True)
def the_initial_weight_generator_is_left_as_found():
    """Initial weights come from ONE process-wide generator (engine._INIT_RNG), and tests elsewhere build their models from wherever it stands:
    the tests here put it back, so the files that run after this one draw what they drew before it existed."""
    from gennet_amd import engine
    rng = engine._INIT_RNG
    state = rng.get_state()
    yield
    rng.set_state(state)
    engine._INIT_RNG = rng


def test_the_shapes_cover_the_set_and_straddle_the_edges():
    assert set(s[0] for s in SHAPES) == {1, 15, 16, 17, 33} and set(s[1] for s in SHAPES) == {1, 2, 3, 17} and len(SHAPES) == 12
    assert all(s[0] * s[1] <= 600 for s in SHAPES)
    us = set(s[2] for s in SHAPES)
    assert us == {1, 16, 17, 80, 81, 88, 89, 104, 105, 130, 512}
    lg = dict((u, lstm_geometry(u)) for u in range(1, 513))
    gg = dict((u, gru_geometry(u)) for u in range(1, 513))
    assert max(u for u in lg if lg[u][3]) == 80 and max(u for u in lg if lg[u][2]) == 88          # LSTM: backward, forward
    assert max(u for u in gg if gg[u][2]) == 104 and max(u for u in gg if gg[u][3]) == 104        # GRU: forward, backward
    for g in (lg, gg):
        assert [g[u][:2] for u in (1, 16, 17, 130, 512)] == [(1, 1), (1, 1), (1, 2), (2, 5), (4, 8)]


def gates_of(cell):
    return 4 if cell == 'lstm' else 3


def draw(cell, reset_after, B, T, u, seed):
    """zx, U, bias, rbias of both directions and dy for both layouts' positions, fp32"""
    rng = np.random.RandomState(seed)
    G = gates_of(cell)
    f32 = lambda a: np.ascontiguousarray(a, np.float32)          # noqa: E731
    d = dict(zx=[f32(rng.randn(B, T, G * u)) for _ in range(2)], U=[f32(rng.randn(u, G * u) / np.sqrt(u)) for _ in range(2)],
             b=[f32(0.5 * rng.randn(G * u)) for _ in range(2)], rb=[f32(0.5 * rng.randn(G * u)) for _ in range(2)] if reset_after else None,
             dy=[f32(rng.randn(B, T, u)) for _ in range(2)])
    return d


def singles(cell, reset_after, d, reverse0, seq, training=True):
    """the two single-direction entry points, one after the other, on the operands of the pair: per direction h, the stored tensors, dz, dzr as
    the pair must lay them out (h at the pair's positions; the rest at the input time index, as the single kernels do)"""
    from gennet_amd import ops
    t = lambda a: None if a is None else torch.tensor(a, device=dev())          # noqa: E731
    out = []
    T = d['zx'][0].shape[1]
    for k in range(2):
        reverse = bool(reverse0) != bool(k)
        zx, U, b = t(d['zx'][k]), t(d['U'][k]), t(d['b'][k])
        dy_pos = d['dy'][k]                                                 # the gradient at the pair's positions
        dy_proc = dy_pos[:, ::-1] if k else dy_pos                          # ... in the direction's processing order
        dy = t(np.array(dy_proc if seq else dy_pos[:, 0], order='C'))       # seq off: any (B, u) gradient for the last step
        if cell == 'lstm':
            h, gates, c, hprev = ops.lstm_fwd(zx, U, b, None, None, 'tanh', 'hard_sigmoid', reverse=reverse, training=training)
            r = dict(gates=gates, c=c, hprev=hprev)
            if training:
                r['dz'] = ops.lstm_bwd(dy, gates, c, U, None, 'tanh', 'hard_sigmoid', reverse=reverse)[0]
        else:
            rb = t(d['rb'][k]) if reset_after else None
            h, gates, hprev, aux = ops.gru_fwd(zx, U, b, rb, None, 'tanh', 'hard_sigmoid', reset_after=reset_after, reverse=reverse, training=training)
            r = dict(gates=gates, hprev=hprev, aux=aux)
            if training:
                r['dz'], r['dzr'], _ = ops.gru_bwd(dy, gates, hprev, aux, U, 'tanh', 'hard_sigmoid', reset_after=reset_after, reverse=reverse)
        h = h.cpu().numpy()
        r = dict((n, v.cpu().numpy()) for n, v in r.items() if v is not None)
        r['h'] = (h[:, ::-1] if k else h) if seq else h[:, T - 1]
        out.append(r)
    return out


def table(ptrs):
    return (ctypes.c_void_p * 2)(*ptrs)


def pair(cell, reset_after, d, reverse0, seq, concat, pad=37, training=True, backward=True):
    """gn_*_pair_fwd and gn_*_pair_bwd on guarded buffers -> per direction h, the stored tensors, dz, dzr; the guards are checked"""
    from gennet_amd import _lib, ops
    B, T, Gu = d['zx'][0].shape
    G = gates_of(cell)
    u = Gu // G
    lead = (B, T) if seq else (B,)
    ins = dict((n, [Guarded(np.shape(v), v, pad) for v in d[n]]) for n in ('zx', 'U', 'b') + (('rb',) if reset_after else ()))
    dys = [np.ascontiguousarray(v if seq else v[:, 0]) for v in d['dy']]
    if concat:
        hbuf = [Guarded(lead + (2 * u,), None, pad)]
        hp = [hbuf[0].t.data_ptr(), hbuf[0].t.data_ptr() + 4 * u]
        dybuf = [Guarded(lead + (2 * u,), np.concatenate(dys, -1), pad)]
        dyp = [dybuf[0].t.data_ptr(), dybuf[0].t.data_ptr() + 4 * u]
    else:
        hbuf = [Guarded(lead + (u,), None, pad) for _ in range(2)]
        hp = [g.t.data_ptr() for g in hbuf]
        dybuf = [Guarded(lead + (u,), v, pad) for v in dys]
        dyp = [g.t.data_ptr() for g in dybuf]
    ld = 2 * u if concat else u
    names = ('gates', 'c', 'hprev') if cell == 'lstm' else ('gates', 'hprev', 'aux')
    st = dict((n, [Guarded((B, T, Gu if n == 'gates' else u), None, pad) for _ in range(2)]) for n in names)
    grads = dict((n, [Guarded((B, T, Gu), None, pad) for _ in range(2)]) for n in (('dz', 'dzr') if reset_after else ('dz',)))
    P = lambda gs: table([g.t.data_ptr() for g in gs])          # noqa: E731
    s = torch.cuda.current_stream().cuda_stream
    act, ract = ops.LSTM_ACT['tanh'], ops.LSTM_ACT['hard_sigmoid']
    if cell == 'lstm':
        ws = ops.workspace(2 * max(_lib.size('gn_lstm_fwd_workspace', u), _lib.size('gn_lstm_bwd_workspace', u)), dev())
        _lib.call('gn_lstm_pair_fwd', P(ins['zx']), P(ins['U']), P(ins['b']), table(hp), P(st['gates']), P(st['c']), P(st['hprev']), ws.data_ptr(),
                  ws.numel(), B, T, u, ld, act, ract, int(reverse0), int(seq), int(training), s)
    else:
        ws = ops.workspace(2 * max(_lib.size('gn_gru_fwd_workspace', u), _lib.size('gn_gru_bwd_workspace', u)), dev())
        _lib.call('gn_gru_pair_fwd', P(ins['zx']), P(ins['U']), P(ins['b']), P(ins['rb']) if reset_after else None, table(hp), P(st['gates']),
                  P(st['hprev']), P(st['aux']), ws.data_ptr(), ws.numel(), B, T, u, ld, act, ract, int(reset_after), int(reverse0), int(seq),
                  int(training), s)
    what = '%s pair forward' % cell
    if concat:
        both = hbuf[0].check(what + ' h')
        hs = [both[..., :u], both[..., u:]]
    else:
        hs = [g.check(what + ' h') for g in hbuf]
    out = [dict(h=hs[k]) for k in range(2)]
    if not training:
        torch.cuda.synchronize()
        assert all(g.untouched() for gs in st.values() for g in gs), 'the inference phase stored something'
        return out
    for n in names:
        for k in range(2):
            out[k][n] = st[n][k].check('%s %s' % (what, n))
    if not backward:
        return out
    if cell == 'lstm':
        _lib.call('gn_lstm_pair_bwd', table(dyp), P(st['gates']), P(st['c']), P(ins['U']), P(grads['dz']), ws.data_ptr(), ws.numel(), B, T, u, ld, act,
                  ract, int(reverse0), int(seq), s)
    else:
        _lib.call('gn_gru_pair_bwd', table(dyp), P(st['gates']), P(st['hprev']), P(st['aux']), P(ins['U']), P(grads['dz']),
                  P(grads['dzr']) if reset_after else None, ws.data_ptr(), ws.numel(), B, T, u, ld, act, ract, int(reset_after), int(reverse0), int(seq), s)
    for n, gs in grads.items():
        for k in range(2):
            out[k][n] = gs[k].check('%s pair backward %s' % (cell, n))
    return out


@pytest.mark.parametrize('cell,reset_after', CELLS, ids=CELL_IDS)
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_a_pair_launch_equals_two_single_launches_bit_for_bit(shape, cell, reset_after):
    """forward and backward; reverse0 0 and 1; sequences and the last step only; the concatenated layout, where each direction's columns of the one
    buffer must hold exactly that direction's values (and every element is written, the guards are not), and the split layout"""
    B, T, u = shape
    d = draw(cell, reset_after, B, T, u, seed=B * 10000 + T * 1000 + u)
    for n, (reverse0, seq) in enumerate(((False, True), (True, True), (False, False), (True, False))):
        want = singles(cell, reset_after, d, reverse0, seq)
        for concat in (True, False):
            got = pair(cell, reset_after, d, reverse0, seq, concat, pad=37 - ((n + concat) & 1))
            for k in range(2):
                assert set(got[k]) == set(want[k]), (sorted(got[k]), sorted(want[k]))
                for name in want[k]:
                    assert same_bits(got[k][name], want[k][name]), (name, 'direction %d' % k, reverse0, seq, concat,
                                                                    int((got[k][name] != want[k][name]).sum()))
        if B * T * u >= 16:                                                     # a single unit may sit saturated: its dz is all zeros
            assert np.abs(want[0]['dz']).max() > 0 and np.abs(want[1]['dz']).max() > 0
        if T > 1 and seq:
            assert not same_bits(want[1]['h'], want[1]['h'][:, ::-1])           # the flip is no identity here


@pytest.mark.parametrize('cell,reset_after', CELLS, ids=CELL_IDS)
@pytest.mark.parametrize('reverse0,seq,concat', [(False, True, True), (True, False, False)], ids=['seq-concat', 'reversed-last-split'])
@pytest.mark.parametrize('u', [64, 130])
def test_a_sample_of_a_pair_launch_does_not_depend_on_the_batch(u, reverse0, seq, concat, cell, reset_after):
    """rows 0 and 32 of a B = 33 pair launch have the bits of the B = 1 pair launches of those samples, with sequences in the concatenated layout
    and, from reverse0 = 1, for the last step alone in the split one.  u = 64: U in LDS; u = 130: streamed"""
    B, T = 33, 5
    d = draw(cell, reset_after, B, T, u, seed=u)
    whole = pair(cell, reset_after, d, reverse0, seq, concat)
    for row in (0, 32):
        one = dict((n, None if v is None else [a[row:row + 1] if n in ('zx', 'dy') else a for a in v]) for n, v in d.items())
        got = pair(cell, reset_after, one, reverse0, seq, concat, pad=36)
        for k in range(2):
            for name in whole[k]:
                assert same_bits(got[k][name][0], whole[k][name][row]), (name, k, row)


@pytest.mark.parametrize('cell,reset_after', CELLS, ids=CELL_IDS)
def test_the_inference_phase_stores_nothing(cell, reset_after):
    d = draw(cell, reset_after, 3, 4, 5, seed=5)
    for concat in (True, False):
        a = pair(cell, reset_after, d, False, True, concat, training=False)
        b = pair(cell, reset_after, d, False, True, concat, backward=False)
        assert all(same_bits(a[k]['h'], b[k]['h']) for k in range(2))


def test_bad_arguments_are_errors_and_launch_nothing():
    from gennet_amd import _lib, ops
    B, T, u = 2, 3, 5
    s = torch.cuda.current_stream().cuda_stream
    tanh, hard = ops.LSTM_ACT['tanh'], ops.LSTM_ACT['hard_sigmoid']
    ws = ops.workspace(2 * max(_lib.size('gn_lstm_fwd_workspace', 512), _lib.size('gn_lstm_bwd_workspace', 512), _lib.size('gn_gru_fwd_workspace', 512),
                               _lib.size('gn_gru_bwd_workspace', 512)), dev())
    for cell, G in (('lstm', 4), ('gru', 3)):
        one = lambda *shape: np.ones(shape, np.float32)          # noqa: E731
        ins = [[Guarded(sh, one(*sh), 36) for _ in range(2)] for sh in ((B, T, G * u), (u, G * u), (G * u,), (B, T, u))]
        zx, U, b, small = ([g.t.data_ptr() for g in gs] for gs in ins)
        outs = [[Guarded(sh, None, 36) for _ in range(2)] for sh in ((B, T, u), (B, T, G * u), (B, T, u), (B, T, u))]
        h, big, o1, o2 = ([g.t.data_ptr() for g in gs] for gs in outs)
        good = dict(zx=zx, U=U, b=b, rb=b, h=h, gates=big, c=o1, hprev=o1, aux=o2, ws=ws.data_ptr(), ws_bytes=ws.numel(), B=B, T=T, u=u, ld=u, act=tanh,
                    ract=hard, ra=1, dy=small, sgates=zx, sc=small, dz=big, dzr=big)

        def tb(v):
            return None if v is None else table(v)

        def fwd(**kw):
            g = dict(good, **kw)
            if cell == 'lstm':
                _lib.call('gn_lstm_pair_fwd', tb(g['zx']), tb(g['U']), tb(g['b']), tb(g['h']), tb(g['gates']), tb(g['c']), tb(g['hprev']), g['ws'],
                          g['ws_bytes'], g['B'], g['T'], g['u'], g['ld'], g['act'], g['ract'], 0, 1, 1, s)
            else:
                _lib.call('gn_gru_pair_fwd', tb(g['zx']), tb(g['U']), tb(g['b']), tb(g['rb']), tb(g['h']), tb(g['gates']), tb(g['hprev']), tb(g['aux']),
                          g['ws'], g['ws_bytes'], g['B'], g['T'], g['u'], g['ld'], g['act'], g['ract'], g['ra'], 0, 1, 1, s)

        def bwd(**kw):
            g = dict(good, **kw)
            if cell == 'lstm':
                _lib.call('gn_lstm_pair_bwd', tb(g['dy']), tb(g['sgates']), tb(g['sc']), tb(g['U']), tb(g['dz']), g['ws'], g['ws_bytes'], g['B'], g['T'],
                          g['u'], g['ld'], g['act'], g['ract'], 1, 1, s)
            else:
                _lib.call('gn_gru_pair_bwd', tb(g['dy']), tb(g['sgates']), tb(g['sc']), tb(g['sc']), tb(g['U']), tb(g['dz']), tb(g['dzr']), g['ws'],
                          g['ws_bytes'], g['B'], g['T'], g['u'], g['ld'], g['act'], g['ract'], g['ra'], 1, 1, s)

        def refused(text, fn, code=None):
            with pytest.raises(_lib.GennetHipError) as e:
                fn()
            assert '(%d)' % (_lib.GN_EINVAL if code is None else code) in str(e.value) and text in str(e.value), str(e.value)
            torch.cuda.synchronize()
            assert all(o.untouched() for gs in outs for o in gs)

        need = dict(fwd=2 * _lib.size('gn_lstm_fwd_workspace' if cell == 'lstm' else 'gn_gru_fwd_workspace', u),
                    bwd=2 * _lib.size('gn_lstm_bwd_workspace' if cell == 'lstm' else 'gn_gru_bwd_workspace', u))
        for call, query in ((fwd, 'fwd'), (bwd, 'bwd')):
            refused('null table', lambda: call(U=None))                                     # a NULL table
            refused('null pointer in direction 1', lambda: call(U=[U[0], None]))            # a NULL entry
            refused('ld = 4', lambda: call(ld=u - 1))
            refused('bad shape', lambda: call(T=0))
            refused('bad shape', lambda: call(u=0))
            refused('at most 512', lambda: call(u=513))
            refused('unknown activation code 7', lambda: call(act=7))
            refused('unknown recurrent activation code 0', lambda: call(ract=tanh))
            if cell == 'gru':
                refused('reset_after = 2', lambda: call(ra=2))
            refused('workspace too small', lambda: call(ws_bytes=need[query] - 1), _lib.GN_EWORKSPACE)
            call(B=0)                                                                       # nothing to do: no error, no launch
            torch.cuda.synchronize()
            assert all(o.untouched() for gs in outs for o in gs)
        fwd(ws_bytes=need['fwd'])                                                           # twice the single query is enough
        bwd(ws_bytes=need['bwd'])
        torch.cuda.synchronize()
        for gs in outs[:2]:
            for o in gs:
                o.check('%s pair' % cell)


# ---------------------------------------------------------------------------------------------------------------------
# section 2: models against torch fp64 autograd
# ---------------------------------------------------------------------------------------------------------------------
def seed_biases(model, rng):
    """every bias moves off its initial value (both triples of a Bidirectional: its weights 2 and 5)"""
    for l in model.layers:
        ws = l.get_weights()
        for i in ([2, 5] if type(l).__name__ == 'Bidirectional' else [len(ws) - 1] if ws else []):
            ws[i] = (ws[i] + 0.1 * rng.randn(*ws[i].shape)).astype(np.float32)
        if ws:
            l.set_weights(ws)


def bi_ref(P, layer, x):
    inner = layer.layer
    kw = dict(activation=inner.activation, recurrent_activation=inner.recurrent_activation, return_sequences=inner.return_sequences,
              go_backwards=inner.go_backwards)
    cell = type(inner).__name__.lower()
    if cell == 'gru':
        kw['reset_after'] = inner.reset_after
    return BR.torch_forward(cell, x, P[layer.name], layer.merge_mode, **kw)


def sequential(*layers):
    from gennet_amd.engine import Sequential
    model = Sequential()
    for l in layers:
        model.add(l)
    return model


def conv_bi_model():
    """Conv1D(6, 3) -> Bidirectional(LSTM(7, return_sequences=True)) -> Bidirectional(GRU(5), 'sum') -> Dense(2)"""
    from gennet_amd import layers as Ly
    conv = Ly.Conv1D(6, 3, input_shape=(12, 3))
    first = Ly.Bidirectional(Ly.LSTM(7, return_sequences=True))
    second = Ly.Bidirectional(Ly.GRU(5), merge_mode='sum')
    head = Ly.Dense(2)

    def ref(P, x):
        w, b = P[conv.name]
        c = F.conv1d(x.permute(0, 2, 1), w.permute(2, 1, 0)).permute(0, 2, 1) + b
        return bi_ref(P, second, bi_ref(P, first, c)) @ P[head.name][0] + P[head.name][1]
    return sequential(conv, first, second, head), ref


def test_conv_bilstm_bigru_dense_trains_as_torch_fp64():
    model, ref = conv_bi_model()
    rng = np.random.RandomState(41)
    seed_biases(model, rng)
    assert model.output_shape == (None, 2) and [n.out_shape for n in model.nodes] == [(10, 6), (10, 14), (5,), (2,)]
    train_and_compare(model, ref, [rng.randn(5, 12, 3).astype(np.float32)], rng.randn(5, 2).astype(np.float32), what='conv-bilstm-bigru')


def one_layer_model(inner, merge_mode, T=9, Cin=4):
    from gennet_amd import layers as Ly
    bi = Ly.Bidirectional(inner, merge_mode=merge_mode, input_shape=(T, Cin))
    head = Ly.Dense(1)
    seq = inner.return_sequences
    model = sequential(bi, Ly.GlobalAveragePooling1D(), head) if seq else sequential(bi, head)

    def ref(P, x):
        y = bi_ref(P, bi, x)
        return (y.mean(1) if seq else y) @ P[head.name][0] + P[head.name][1]
    return model, ref


# id -> (inner class, its keywords, merge_mode)
MODELS = {
    'mul-lstm-seq': ('LSTM', dict(units=6, return_sequences=True), 'mul'),
    'ave-gru-seq': ('GRU', dict(units=7, return_sequences=True, recurrent_activation='sigmoid'), 'ave'),
    'mul-gru-last': ('GRU', dict(units=6), 'mul'),
    'concat-lstm-last': ('LSTM', dict(units=20), 'concat'),
    'concat-gru-go-backwards-seq': ('GRU', dict(units=8, return_sequences=True, go_backwards=True), 'concat'),
    'sum-lstm-go-backwards-last': ('LSTM', dict(units=6, go_backwards=True), 'sum'),
    'concat-gru-reset-after-seq': ('GRU', dict(units=6, return_sequences=True, reset_after=True), 'concat'),
}


@pytest.mark.parametrize('which', sorted(MODELS))
def test_a_bidirectional_layer_trains_as_torch_fp64(which):
    """the remaining merge modes, concat without sequences, an inner go_backwards=True (the forward copy then walks backwards and the backward
    copy forwards, and position is not input time), reset_after=True"""
    from gennet_amd import layers as Ly
    cls, kw, mode = MODELS[which]
    inner = getattr(Ly, cls)(**kw)
    model, ref = one_layer_model(inner, mode)
    rng = np.random.RandomState(42 + sorted(MODELS).index(which))
    seed_biases(model, rng)
    u = inner.units * (2 if mode == 'concat' else 1)
    assert model.nodes[0].out_shape == ((9, u) if inner.return_sequences else (u,))
    train_and_compare(model, ref, [rng.randn(6, 9, 4).astype(np.float32)], rng.randn(6, 1).astype(np.float32), what=which)


def regularized_model():
    from gennet_amd import layers as Ly, regularizers
    inner = Ly.LSTM(8, return_sequences=True, kernel_regularizer=regularizers.l2(0.01), recurrent_regularizer=regularizers.l1(0.002),
                    bias_regularizer=regularizers.l1_l2(0.003, 0.004))
    return one_layer_model(inner, 'concat', T=10, Cin=3)


def test_the_weight_regularizers_penalty_shows_in_the_loss():
    model, ref = regularized_model()
    rng = np.random.RandomState(51)
    seed_biases(model, rng)
    assert [p.regularizer is not None for p in model.layers[0].weights] == [True] * 6
    pens = train_and_compare(model, ref, [rng.randn(5, 10, 3).astype(np.float32)], rng.randn(5, 1).astype(np.float32), what='regularized')
    assert min(pens) > 0.05          # the loss was held against loss + penalty of BOTH triples: the penalty is no rounding matter


def test_save_and_load_round_trip(tmp_path):
    from gennet_amd.engine import SGD, load_model
    model, _ = conv_bi_model()
    rng = np.random.RandomState(52)
    seed_biases(model, rng)
    x, t = rng.randn(5, 12, 3).astype(np.float32), rng.randn(5, 2).astype(np.float32)
    model.compile(optimizer=SGD(lr=LR), loss='mean_squared_error')
    model.train_on_batch(x, t)
    path = os.path.join(str(tmp_path), 'bi.h5')
    model.save(path)
    again = load_model(path)
    assert [type(n.layer).__name__ for n in again.nodes] == ['Conv1D', 'Bidirectional', 'Bidirectional', 'Dense']
    for a, b in zip(again.layers, model.layers):
        assert a.get_config() == b.get_config() and [p.name for p in a.weights] == [p.name for p in b.weights]
    assert np.array_equal(model.predict(x), again.predict(x))
    a, b = model.train_on_batch(x, t), again.train_on_batch(x, t)
    assert a == b and all(np.array_equal(v, w) for v, w in zip(model.get_weights(), again.get_weights()))


def test_predict_allocates_no_tape():
    from gennet_amd import engine
    model, _ = conv_bi_model()
    x = np.random.RandomState(53).randn(3, 12, 3).astype(np.float32)
    ctx = engine.RunContext(False)
    out = model._forward(model._prep_inputs(x), ctx)
    assert tuple(out[0].shape) == (3, 2) and not any(model.nodes[i].index in ctx.tape for i in (1, 2))
    ctx = engine.RunContext(True)
    model._forward(model._prep_inputs(x), ctx)
    x_kept, hprev, gates, c, h = ctx.tape[model.nodes[1].index]
    assert tuple(x_kept.shape) == (3, 10, 6) and h is None                # the halves are kept under 'mul' alone
    assert [[tuple(v.shape) for v in pair_] for pair_ in (hprev, gates, c)] == [[(3, 10, 7)] * 2, [(3, 10, 28)] * 2, [(3, 10, 7)] * 2]


def test_a_captured_step_replays_bit_identically():
    """the model as a hipGraph (engine.StepGraph): the pointer tables are host arguments read at the call, so the captured launches carry the
    addresses; eager step, capture, three replays against four eager steps of a twin"""
    from gennet_amd import engine
    from gennet_amd.engine import SGD, to_device
    rng = np.random.RandomState(54)
    x, t = to_device(rng.randn(5, 12, 3).astype(np.float32)), to_device(rng.randn(5, 2).astype(np.float32))
    eager, _ = conv_bi_model()
    seed_biases(eager, rng)
    graphed, _ = conv_bi_model()
    graphed.set_weights(eager.get_weights())
    for m in (eager, graphed):
        m.compile(optimizer=SGD(lr=LR, momentum=0.5), loss='mean_squared_error')
    want = []
    for _ in range(4):
        want.append((eager.train_on_batch_device([x], [t]).cpu().numpy().copy(), [w.copy() for w in eager.get_weights()]))
    got = [(graphed.train_on_batch_device([x], [t]).cpu().numpy().copy(), [w.copy() for w in graphed.get_weights()])]
    sg = engine.StepGraph()
    torch.cuda.synchronize()
    sg.capture(lambda: graphed.train_on_batch_device([x], [t]))
    for _ in range(3):
        sg.wait_inputs_consumed()
        stats = sg.replay()
        torch.cuda.synchronize()
        got.append((stats.cpu().numpy().copy(), [w.copy() for w in graphed.get_weights()]))
    for step, ((s0, w0), (s1, w1)) in enumerate(zip(want, got)):
        assert np.array_equal(s0, s1), (step, s0, s1)
        assert all(np.array_equal(v, w) for v, w in zip(w0, w1)), step
    assert not np.array_equal(want[0][0], want[3][0])                      # the steps differ: a replay that did nothing would show
