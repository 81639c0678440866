"""GPU parity of keras layers.SimpleRNN: csrc/rnn.hip through gn_rnn_fwd / gn_rnn_bwd and the pair entry points against the fp64 definition
tests/rnn_ref.py (itself checked against torch.nn.RNN and torch autograd in tests/test_rnn_cpu.py), and the layer at model level, alone and
inside Bidirectional, against torch fp64 autograd on the CPU.  The Guarded buffers, the activation error table and train_and_compare are those
of tests/test_lstm_gpu.py.

Section 1, kernel level.  Inputs sit in NaN-surrounded buffers, outputs in sentinel-filled ones, a view 36 or 37 floats in.  R.SHAPES is LSTM's
covering set of (B, T, Cin) with u moved to the edges of csrc/rnn_geom.h:
  u    {1, 3, 4, 15, 16, 17, 31, 32, 33, 64, 128, 129, 130, 176, 177, 260, 512}: below one MFMA, both sides of one and of two tiles; 128 | 129, one
       tile a wave and two with U in LDS; 176, the last u whose padded U (forward) and U^T (backward) lie in LDS beside the state, and 177, the
       first streamed one -- the geometry's two LDS-or-streamed decisions fall on this one pair; more tiles than waves (130: two a wave; 260:
       three; 512: four on 8 waves, the largest u the entry points take)
  B, T, Cin as in tests/test_lstm_gpu.py.
Section 2, model level: the bounds of tests/test_lstm_gpu.py's train_and_compare as they stand, over three SGD steps."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bidirectional_ref as BR
import rnn_ref as R
from test_lstm_gpu import ACT_ERR, EPS, LR, Guarded, dev, same_bits, seed_biases, torch_params, train_and_compare
from test_gru_gpu import MARGIN

pytestmark = pytest.mark.gpu

SHAPES, IDS = R.SHAPES, R.IDS


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


def test_the_shapes_cover_the_set():
    assert set(s[0] for s in SHAPES) == {1, 2, 15, 16, 17, 33} and set(s[1] for s in SHAPES) == {1, 2, 3, 17}
    assert set(s[2] for s in SHAPES) == {1, 3, 16, 17} and len(SHAPES) == 24
    assert set(s[3] for s in SHAPES) >= {1, 3, 4, 15, 16, 17, 31, 32, 33, 64, 130, 260, 512}          # the tile and wave edges


def geometry(u):
    """csrc/rnn_geom.h, restated: (tiles a wave, waves, U in LDS forward, U^T in LDS backward, workspace bytes forward, backward)"""
    KP, UP = -(-u // 8) * 8, -(-u // 16) * 16
    SU, SUT = UP | 16, UP | 16
    ntiles = UP // 16
    NT = -(-ntiles // 8)
    fwd = 2 * 16 * (KP + 1) * 4 + KP * SU * 4
    bwd = 2 * 16 * (KP + 1) * 4 + KP * SUT * 4
    return NT, -(-ntiles // NT), fwd <= 160 * 1024, bwd <= 160 * 1024, KP * SU * 4, KP * SUT * 4


LDS_EDGES = sorted(set(max(u for u in range(1, 513) if geometry(u)[side]) for side in (2, 3)))          # the last u in LDS: forward, backward


def test_the_shapes_straddle_the_kernel_edges():
    us = set(s[3] for s in SHAPES)
    g = dict((u, geometry(u)) for u in range(1, 513))
    for side in (2, 3):                      # forward, backward: the set holds the last u in LDS and the first streamed one
        last = max(u for u in g if g[u][side])
        assert all(g[u][side] == (u <= last) for u in g) and last in us and last + 1 in us, (side, last)
    assert LDS_EDGES == [176] and g[176][2] and g[176][3] and not g[177][2] and not g[177][3]
    assert [g[u][:2] for u in (1, 16, 17, 64, 128, 129, 130, 176, 177, 260, 512)] == [(1, 1), (1, 1), (1, 2), (1, 4), (1, 8), (2, 5), (2, 5), (2, 6),
                                                                                     (2, 6), (3, 6), (4, 8)]
    from gennet_amd import _lib
    for u in us:
        assert _lib.size('gn_rnn_fwd_workspace', u) == g[u][4] and _lib.size('gn_rnn_bwd_workspace', u) == g[u][5]


def run_kernels(zx, U, b, h0, dy, activation, reverse, pad=37, training=True):
    """gn_rnn_fwd (training phase) and gn_rnn_bwd on guarded buffers -> h (processing order); hs, hprev, dz (input time order); dh0"""
    from gennet_amd import _lib, ops
    B, T, u = zx.shape
    gi = dict((k, None if v is None else Guarded(np.shape(v), v, pad)) for k, v in dict(zx=zx, U=U, b=b, h0=h0, dy=dy).items())
    go = dict((k, Guarded(s, None, pad)) for k, s in dict(h=(B, T, u), hs=(B, T, u), hprev=(B, T, u), dz=(B, T, u), dh0=(B, u)).items())
    p = dict((k, None if v is None else v.t.data_ptr()) for k, v in list(gi.items()) + list(go.items()))
    s = torch.cuda.current_stream().cuda_stream
    act = ops.LSTM_ACT[activation]
    ws = ops.workspace(_lib.size('gn_rnn_fwd_workspace', u), dev())
    _lib.call('gn_rnn_fwd', p['zx'], p['U'], p['b'], p['h0'], p['h'], p['hs'], p['hprev'], ws.data_ptr(), ws.numel(), B, T, u, act, int(reverse),
              int(training), s)
    out = dict(h=go['h'].check('rnn_fwd h'))
    if not training:
        torch.cuda.synchronize()
        assert all(go[k].untouched() for k in ('hs', 'hprev', 'dz', 'dh0'))
        return out
    for k in ('hs', 'hprev'):
        out[k] = go[k].check('rnn_fwd ' + k)
    ws = ops.workspace(_lib.size('gn_rnn_bwd_workspace', u), dev())
    _lib.call('gn_rnn_bwd', p['dy'], p['hs'], p['U'], p['dz'], p['dh0'], ws.data_ptr(), ws.numel(), B, T, u, act, int(reverse), int(np.ndim(dy) == 3), s)
    for k in ('dz', 'dh0'):
        out[k] = go[k].check('rnn_bwd ' + k)
    return out


def reference_at_input_time(k, r):
    """the reference's stored tensors as the kernels index them"""
    t = lambda a: np.ascontiguousarray(R.at_input_time(a, k['go_backwards']))          # noqa: E731
    return dict(h=k['h'], hs=t(k['h']), hprev=t(k['h_prev']), dz=t(r['dz']), dh0=r['dh0'])


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_integer_sequences_are_exact(shape):
    """activation='linear' on R.integer_case's integers, at the shape's own T: every value, product and partial sum of the forward and of the
    backward is an integer below 2^24 (asserted on sums of absolute values; tests/test_rnn_cpu.py asserts it for every shape without a GPU), so
    ANY correct kernel returns the reference's h, hs, hprev, dz and dh0 bit for bit -- and a wrong time index, a wrong lane map, a dropped k
    group, a transposed U, a stale LDS copy or a reversed direction does not.  Both walking directions, dy as a sequence and for the last
    step only, an integer h0."""
    c = R.integer_case(shape)
    assert c['big'] < 2 ** 24, c['big']
    for reverse, dy, k, r in c['cases']:
        want = reference_at_input_time(k, r)
        assert all(np.array_equal(v, np.rint(v)) for v in want.values())
        for pad in (37, 36):
            got = run_kernels(c['zx'], c['U'], c['b'], c['h0'], dy, 'linear', reverse, pad)
            assert set(got) == set(want)
            for name, v in want.items():
                assert same_bits(got[name], v.astype(np.float32)), (name, reverse, dy.ndim, pad, int((got[name] != v).sum()))
    print(shape, 'largest magnitude', c['big'])


def gamma(n):
    """Higham's gamma_n = n e / (1 - n e) for the unit roundoff e = 2^-24"""
    return n * EPS / (1 - n * EPS)


# |act'(y) - act'(y64)| <= GRAD_LIP[act](y64) |y - y64| + 2 e: the derivative through the output value, two roundings on values <= 1
GRAD_LIP = {'tanh': lambda y: 2 * np.abs(y), 'sigmoid': lambda y: np.abs(1 - 2 * y), 'relu': lambda y: 0 * y, 'linear': lambda y: 0 * y}


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_one_step_meets_the_derived_bound(shape):
    """T = 1 with random h0 and dy, against the fp64 evaluation of the same fp32 inputs, e = 2^-24, gamma_n = n e / (1 - n e) (Higham (3.4)).
      pre      (sum_k h U, one fma chain of u terms from +0) + (zx + b): a term passes at most u + 2 roundings,
                   d_pre = gamma_{u+2} (sum_k |h U| + |zx| + |b|)
      h        act(pre), every activation's Lipschitz constant <= 1: d_h = d_pre + ACT_ERR[act](h), the function's own error
               (tests/test_lstm_gpu.py's table); hs must be h's bits and hprev h0's
      dz       (dy + 0) act'(h) with act' through the OUTPUT value, evaluated at the kernel's h: tanh 1 - y y, sigmoid y (1 - y) (two roundings
               on values <= 1), relu and linear exact: d_g = L(y) d_h + 2 e with L = 2 |y|, |1 - 2 y|, 0, 0; relu's derivative jumps at 0, so
               where |pre| <= d_pre the kernel may stand on the other side and d_g = 1.   d_dz = |dy| d_g + e |dz|
      dh0      dz . U^T, one chain of u terms from +0: d_dh0 = (1 + gamma_u) sum_k d_dz |U^T| + gamma_u sum_k |dz U^T|
    Every element of h, dz and dh0 is compared; nothing is added on top."""
    B, _, Cin, u = shape
    rng = np.random.RandomState(7 + B * 1000 + Cin * 10 + u)
    f32 = lambda a: a.astype(np.float32)          # noqa: E731
    zx, U, b = f32(rng.randn(B, 1, u)), f32(rng.randn(u, u) / np.sqrt(u)), f32(0.5 * rng.randn(u))
    h0, dy = f32(rng.rand(B, u) * 2 - 1), f32(rng.randn(B, u))
    A = lambda v: np.abs(np.asarray(v, np.float64))          # noqa: E731
    for n, an in enumerate(R.ACTIVATIONS):
        k = R.recurrence(zx, U, b, h0, an, bool(n & 1))
        r = R.recurrence_backward(k, dy)
        got = run_kernels(zx, U, b, h0, dy, an, bool(n & 1), pad=37 - (n & 1))
        h64, pre64, dz64 = k['h'][:, 0], k['pre'][:, 0], r['dz'][:, 0]
        d_pre = gamma(u + 2) * (A(h0) @ A(U) + A(zx[:, 0]) + A(b))
        d_h = d_pre + ACT_ERR[an](h64)
        d_g = GRAD_LIP[an](h64) * d_h + (2 * EPS if an in ('tanh', 'sigmoid') else 0)
        if an == 'relu':
            d_g = np.where(A(pre64) <= d_pre, 1.0, 0.0)
        d_dz = A(dy) * d_g + EPS * A(dz64)
        d_dh0 = (1 + gamma(u)) * (d_dz @ A(U).T) + gamma(u) * (A(dz64) @ A(U).T)
        for name, ref, bound in (('h', h64, d_h), ('dz', dz64, d_dz), ('dh0', r['dh0'], d_dh0)):
            g = got[name][:, 0] if name != 'dh0' else got[name]
            err = np.abs(g.astype(np.float64) - ref)
            print(shape, an, name, 'worst error / bound %.3g' % (err / (bound + 1e-300)).max())
            assert (err <= bound).all(), (an, name, float((err / (bound + 1e-300)).max()))
        assert same_bits(got['hprev'][:, 0], h0) and same_bits(got['hs'], got['h'])


@pytest.mark.parametrize('activation', R.ACTIVATIONS)
@pytest.mark.parametrize('family', R.FAMILIES)
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_sequences_against_the_fp64_reference(shape, family, activation):
    """zx = X W (gn_bmm), the recurrence and its backward against tests/rnn_ref.py in fp64.  The yardstick is the numpy fp32 restatement of the
    same recurrence, measured against fp64 on the same inputs: the GPU's largest error in h, dz and dh0 may be at most MARGIN = 8 (the project's
    figure in tests/test_gru_gpu.py: the same device functions, the same chain classes) times max(the restatement's, 2^-24 max|ref|).  Four
    activations, two input families (R.draw_family); the seed is R.sequence_case's, chosen from the reference alone (tests/test_rnn_cpu.py
    asserts one exists for every case).  No element is excluded from any comparison."""
    from gennet_amd import ops
    B, T, Cin, u = shape
    n = SHAPES.index(shape)
    case = R.sequence_case(shape, family, activation)
    assert case is not None
    x, W, U, b, dy, k64, k32 = (case[key] for key in ('x', 'W', 'U', 'b', 'dy', 'k64', 'k32'))
    reverse = case['reverse']
    r64, r32 = R.recurrence_backward(k64, dy), R.recurrence_backward(k32, dy.astype(np.float32))
    want = reference_at_input_time(k64, r64)
    rest = reference_at_input_time(k32, r32)
    t = lambda a: torch.tensor(np.array(a, dtype=np.float32, order='C'), device=dev())          # noqa: E731
    zx = ops.bmm(t(x).view(1, B * T, Cin), t(W).view(1, Cin, u)).view(B, T, u).cpu().numpy()
    got = run_kernels(zx, U, b, None, dy, activation, reverse, pad=37 - (n & 1))
    assert same_bits(got['hs'], R.at_input_time(got['h'], reverse))
    worst = {}
    for name in ('h', 'dz', 'dh0'):
        ref = want[name]
        yard = max(float(np.abs(rest[name].astype(np.float64) - ref).max()), EPS * float(np.abs(ref).max()))
        err = float(np.abs(got[name].astype(np.float64) - ref).max())
        worst[name] = err / yard if yard else (0.0 if err == 0 else np.inf)
    print(shape, family, activation, 'seed', case['seed'], 'error / yardstick:', ' '.join('%s %.2f' % kv for kv in sorted(worst.items())))
    assert all(v <= MARGIN for v in worst.values()), worst


@pytest.mark.parametrize('u', [LDS_EDGES[0], LDS_EDGES[0] + 1] + [v for e in LDS_EDGES[1:] for v in (e, e + 1)])
def test_a_sample_does_not_depend_on_the_batch_or_the_launch(u):
    """A sample run alone (B = 1), as row 1 of a batch of 3 and as row 16 of a batch of 17 (the only row of a second tile), forward and backward,
    has the same bits every time; two identical launches return the same bits.  The last u with U in LDS and the first streamed one."""
    T = 5
    rng = np.random.RandomState(u)
    f32 = lambda a: a.astype(np.float32)          # noqa: E731
    zx, U, b = f32(rng.randn(17, T, u)), f32(rng.randn(u, u) / np.sqrt(u)), f32(0.5 * rng.randn(u))
    h0, dy = f32(0.5 * rng.randn(17, u)), f32(rng.randn(17, T, u))
    for reverse in (False, True):
        alone = run_kernels(zx[16:17], U, b, h0[16:17], dy[16:17], 'tanh', reverse, pad=36)
        again = run_kernels(zx[16:17], U, b, h0[16:17], dy[16:17], 'tanh', reverse, pad=36)
        assert all(same_bits(alone[k], again[k]) for k in alone) and np.abs(alone['dz']).max() > 0
        for rows, at in (([0, 16, 5], 1), (list(range(17)), 16)):
            whole = run_kernels(zx[rows], U, b, h0[rows], dy[rows], 'tanh', reverse)
            for k in whole:
                assert same_bits(alone[k][0], whole[k][at]), (k, len(rows), reverse)


def test_the_inference_phase_stores_nothing():
    rng = np.random.RandomState(5)
    zx, U, b = rng.randn(3, 4, 5).astype(np.float32), rng.randn(5, 5).astype(np.float32), np.zeros(5, np.float32)
    a = run_kernels(zx, U, b, None, None, 'tanh', False, training=False)
    assert same_bits(a['h'], run_kernels(zx, U, b, None, rng.randn(3, 5).astype(np.float32), 'tanh', False)['h'])


def table(ptrs):
    return None if ptrs is None else (ctypes.c_void_p * 2)(*ptrs)


def test_bad_arguments_are_errors_and_launch_nothing():
    """the four entry points: every refusal launches nothing and writes nothing"""
    from gennet_amd import _lib, ops
    B, T, u = 2, 3, 5
    one = lambda *s: np.ones(s, np.float32)          # noqa: E731
    ins = dict((n, [Guarded(s, one(*s), 36) for _ in range(2)]) for n, s in dict(zx=(B, T, u), U=(u, u), b=(u,), h0=(B, u), dy=(B, T, u), shs=(B, T, u)).items())
    outs = dict((n, [Guarded(s, None, 36) for _ in range(2)]) for n, s in dict(h=(B, T, u), hs=(B, T, u), hprev=(B, T, u), dz=(B, T, u), dh0=(B, u)).items())
    every = [g for gs in outs.values() for g in gs]
    s = torch.cuda.current_stream().cuda_stream
    ws = ops.workspace(2 * max(_lib.size('gn_rnn_fwd_workspace', 512), _lib.size('gn_rnn_bwd_workspace', 512)), dev())
    tanh, hard = ops.LSTM_ACT['tanh'], ops.LSTM_ACT['hard_sigmoid']
    ptr = dict((n, [g.t.data_ptr() for g in gs]) for n, gs in list(ins.items()) + list(outs.items()))
    good = dict(ptr, ws=ws.data_ptr(), ws_bytes=ws.numel(), B=B, T=T, u=u, ld=u, act=tanh, training=1)
    first = lambda v: None if v is None else v[0]          # noqa: E731

    def fwd(**kw):
        g = dict(good, **kw)
        _lib.call('gn_rnn_fwd', first(g['zx']), first(g['U']), first(g['b']), first(g['h0']), first(g['h']), first(g['hs']), first(g['hprev']), g['ws'],
                  g['ws_bytes'], g['B'], g['T'], g['u'], g['act'], 0, g['training'], s)

    def bwd(**kw):
        g = dict(good, **kw)
        _lib.call('gn_rnn_bwd', first(g['dy']), first(g['shs']), first(g['U']), first(g['dz']), first(g['dh0']), g['ws'], g['ws_bytes'], g['B'], g['T'],
                  g['u'], g['act'], 1, 1, s)

    def pfwd(**kw):
        g = dict(good, **kw)
        _lib.call('gn_rnn_pair_fwd', table(g['zx']), table(g['U']), table(g['b']), table(g['h']), table(g['hs']), table(g['hprev']), g['ws'], g['ws_bytes'],
                  g['B'], g['T'], g['u'], g['ld'], g['act'], 0, 1, g['training'], s)

    def pbwd(**kw):
        g = dict(good, **kw)
        _lib.call('gn_rnn_pair_bwd', table(g['dy']), table(g['shs']), table(g['U']), table(g['dz']), g['ws'], g['ws_bytes'], g['B'], g['T'], g['u'],
                  g['ld'], g['act'], 1, 1, s)

    def refused(text, fn, code=None):
        with pytest.raises(_lib.GennetHipError) as e:
            fn()
        assert '(%d)' % (_lib.GN_EINVAL if code is None else code) in str(e.value) and text in str(e.value), str(e.value)
        assert text in _lib.lib().gn_last_error().decode()
        torch.cuda.synchronize()
        assert all(o.untouched() for o in every)

    for k in ('zx', 'U', 'b', 'h', 'ws', 'hs', 'hprev'):
        refused('null pointer', lambda: fwd(**{k: None}))
        if k != 'ws':
            refused('null table', lambda: pfwd(**{k: None}))
            refused('null pointer in direction 1', lambda: pfwd(**{k: [good[k][0], None]}))
            refused('null pointer in direction 0', lambda: pfwd(**{k: [None, good[k][1]]}))
    for k in ('dy', 'shs', 'U', 'dz', 'ws'):
        refused('null pointer', lambda: bwd(**{k: None}))
        if k != 'ws':
            refused('null table', lambda: pbwd(**{k: None}))
            refused('null pointer in direction 1', lambda: pbwd(**{k: [good[k][0], None]}))
    refused('null table', lambda: pfwd(ws=None))
    refused('null table', lambda: pbwd(ws=None))
    need = dict((c, _lib.size('gn_rnn_fwd_workspace' if c in (fwd, pfwd) else 'gn_rnn_bwd_workspace', u) * (2 if c in (pfwd, pbwd) else 1))
                for c in (fwd, bwd, pfwd, pbwd))
    for call in (fwd, bwd, pfwd, pbwd):
        refused('bad shape', lambda: call(T=0))
        refused('bad shape', lambda: call(u=0))
        refused('bad shape', lambda: call(B=-1))
        refused('at most 512', lambda: call(u=513))
        refused('unknown activation code 7', lambda: call(act=7))
        refused('unknown activation code -1', lambda: call(act=-1))
        refused('unknown activation code 4', lambda: call(act=hard))
        refused('workspace too small', lambda: call(ws_bytes=need[call] - 1), _lib.GN_EWORKSPACE)
        call(B=0)                                              # nothing to do is not an error, and launches nothing (the pointers are not looked at)
    for call in (pfwd, pbwd):
        refused('ld = 4', lambda: call(ld=u - 1))
        refused('ld = 4', lambda: call(ld=u - 1, B=0))
    fwd(B=0, zx=None, h=None, ws=None)
    assert _lib.size('gn_rnn_fwd_workspace', 513) == 0 and _lib.size('gn_rnn_bwd_workspace', 0) == 0
    torch.cuda.synchronize()
    assert all(o.untouched() for o in every)
    fwd(hs=None, hprev=None, training=0, h0=None, ws_bytes=need[fwd])          # the inference phase takes no storage, and no initial state
    bwd(dh0=None, ws_bytes=need[bwd])
    pfwd(hs=None, hprev=None, training=0, ws_bytes=need[pfwd])                 # twice the single query is enough
    pbwd(ws_bytes=need[pbwd])
    torch.cuda.synchronize()
    for n in ('h', 'dz'):
        for o in outs[n]:
            o.check('rnn ' + n)
    assert all(o.untouched() for n in ('hs', 'hprev', 'dh0') for o in outs[n])
    with pytest.raises(ValueError, match='recurrent kernel'):
        ops.rnn_fwd(ins['zx'][0].t, ins['U'][0].t[:, :4].contiguous(), ins['b'][0].t)


# --- the pair launch
PAIR_SHAPES = [(1, 1, 1), (15, 2, 16), (16, 3, 17), (17, 17, 128), (33, 1, 129), (1, 2, 176), (15, 3, 177), (2, 17, 64), (33, 2, 260), (1, 3, 512)]


def pair_draw(B, T, u, seed):
    rng = np.random.RandomState(seed)
    f32 = lambda a: np.ascontiguousarray(a, np.float32)          # noqa: E731
    return dict(zx=[f32(rng.randn(B, T, u)) for _ in range(2)], U=[f32(rng.randn(u, u) / np.sqrt(u)) for _ in range(2)],
                b=[f32(0.5 * rng.randn(u)) for _ in range(2)], dy=[f32(rng.randn(B, T, u)) for _ in range(2)])


def pair_singles(d, reverse0, seq):
    """the two single-direction entry points on the operands of the pair: per direction h at the pair's positions, hs, hprev and dz at the input
    time index"""
    out = []
    T = d['zx'][0].shape[1]
    for k in range(2):
        dy_pos = d['dy'][k]                                                 # the gradient at the pair's positions
        dy = np.array((dy_pos[:, ::-1] if k else dy_pos) if seq else dy_pos[:, 0], order='C')          # a copy: no negative stride is left
        r = run_kernels(d['zx'][k], d['U'][k], d['b'][k], None, dy, 'tanh', bool(reverse0) != bool(k), pad=36)
        r.pop('dh0')
        r['h'] = (r['h'][:, ::-1] if k else r['h']) if seq else r['h'][:, T - 1]
        out.append(r)
    return out


def pair_launch(d, reverse0, seq, concat, pad=37):
    """gn_rnn_pair_fwd and gn_rnn_pair_bwd on guarded buffers -> per direction h, hs, hprev, dz; the guards are checked"""
    from gennet_amd import _lib, ops
    B, T, u = d['zx'][0].shape
    lead = (B, T) if seq else (B,)
    ins = dict((n, [Guarded(np.shape(v), v, pad) for v in d[n]]) for n in ('zx', 'U', 'b'))
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
    st = dict((n, [Guarded((B, T, u), None, pad) for _ in range(2)]) for n in ('hs', 'hprev', 'dz'))
    P = lambda gs: table([g.t.data_ptr() for g in gs])          # noqa: E731
    s = torch.cuda.current_stream().cuda_stream
    act = ops.LSTM_ACT['tanh']
    ws = ops.workspace(2 * max(_lib.size('gn_rnn_fwd_workspace', u), _lib.size('gn_rnn_bwd_workspace', u)), dev())
    _lib.call('gn_rnn_pair_fwd', P(ins['zx']), P(ins['U']), P(ins['b']), table(hp), P(st['hs']), P(st['hprev']), ws.data_ptr(), ws.numel(), B, T, u, ld,
              act, int(reverse0), int(seq), 1, s)
    if concat:
        both = hbuf[0].check('rnn pair forward h')
        hs = [both[..., :u], both[..., u:]]
    else:
        hs = [g.check('rnn pair forward h') for g in hbuf]
    out = [dict(h=hs[k]) for k in range(2)]
    for n in ('hs', 'hprev'):
        for k in range(2):
            out[k][n] = st[n][k].check('rnn pair forward ' + n)
    _lib.call('gn_rnn_pair_bwd', table(dyp), P(st['hs']), P(ins['U']), P(st['dz']), ws.data_ptr(), ws.numel(), B, T, u, ld, act, int(reverse0), int(seq), s)
    for k in range(2):
        out[k]['dz'] = st['dz'][k].check('rnn pair backward dz')
    return out


@pytest.mark.parametrize('shape', PAIR_SHAPES, ids=['b%d-t%d-u%d' % s for s in PAIR_SHAPES])
def test_a_pair_launch_equals_two_single_launches_bit_for_bit(shape):
    """forward and backward; reverse0 0 and 1; seq 0 and 1; ld = 2u into ONE (B, [T,] 2u) buffer, where each direction's columns must hold exactly
    that direction's values (and every element is written, the guards are not), and ld = u into two buffers"""
    B, T, u = shape
    d = pair_draw(B, T, u, seed=B * 10000 + T * 1000 + u)
    for n, (reverse0, seq) in enumerate(((False, True), (True, True), (False, False), (True, False))):
        want = pair_singles(d, reverse0, seq)
        for concat in (True, False):
            got = pair_launch(d, reverse0, seq, concat, pad=37 - ((n + concat) & 1))
            for k in range(2):
                assert set(got[k]) == set(want[k]), (sorted(got[k]), sorted(want[k]))
                for name in want[k]:
                    assert same_bits(got[k][name], want[k][name]), (name, 'direction %d' % k, reverse0, seq, concat,
                                                                    int((got[k][name] != want[k][name]).sum()))
        assert np.abs(want[0]['dz']).max() > 0 and np.abs(want[1]['dz']).max() > 0
        if T > 1 and seq:
            assert not same_bits(want[1]['h'], want[1]['h'][:, ::-1])           # the flip is no identity here


# ---------------------------------------------------------------------------------------------------------------------
# section 2: models against torch fp64 autograd (tests/test_lstm_gpu.py's train_and_compare: the bounds of tests/test_merge_gpu.py, three steps)
# ---------------------------------------------------------------------------------------------------------------------
def rnn_ref(P, layer, x):
    W, U, b = P[layer.name]
    return R.torch_forward(x, W, U, b, None, layer.activation, layer.return_sequences, layer.go_backwards)


def bi_ref(weights, layer, x):
    inner = layer.layer
    y, y_rev = (R.torch_forward(x, *weights[3 * d:3 * d + 3], None, inner.activation, inner.return_sequences, inner.go_backwards != bool(d))
                for d in range(2))
    return BR.merge(y, y_rev, layer.merge_mode, inner.return_sequences, cat=torch.cat)


def sequential(*layers):
    from gennet_amd.engine import Sequential
    model = Sequential()
    for l in layers:
        model.add(l)
    return model


def seed_all_biases(model, rng):
    """every bias moves off its initial value (both triples of a Bidirectional: its weights 2 and 5)"""
    for l in model.layers:
        ws = l.get_weights()
        for i in ([2, 5] if type(l).__name__ == 'Bidirectional' else [len(ws) - 1] if ws else []):
            ws[i] = (ws[i] + 0.1 * rng.randn(*ws[i].shape)).astype(np.float32)
        if ws:
            l.set_weights(ws)


def conv_rnn_model():
    """Conv1D(8, 5, strides=2) -> SimpleRNN(12) -> Dense(2); the SimpleRNN carries the three weight regularizers, an l2 on the recurrent kernel"""
    from gennet_amd import layers as Ly, regularizers
    conv = Ly.Conv1D(8, 5, strides=2, input_shape=(21, 4))
    rnn = Ly.SimpleRNN(12, kernel_regularizer=regularizers.l1(0.002), recurrent_regularizer=regularizers.l2(0.01),
                       bias_regularizer=regularizers.l1_l2(0.003, 0.004))
    head = Ly.Dense(2)

    def ref(P, x):
        w, b = P[conv.name]
        c = F.conv1d(x.permute(0, 2, 1), w.permute(2, 1, 0), stride=2).permute(0, 2, 1) + b
        return rnn_ref(P, rnn, c) @ P[head.name][0] + P[head.name][1]
    return sequential(conv, rnn, head), ref


def test_conv_rnn_dense_trains_as_torch_fp64_and_its_penalty_shows():
    model, ref = conv_rnn_model()
    rng = np.random.RandomState(31)
    seed_biases(model, rng)
    assert model.output_shape == (None, 2) and [n.out_shape for n in model.nodes] == [(9, 8), (12,), (2,)]
    assert [p.shape for p in model.layers[1].weights] == [(8, 12), (12, 12), (12,)]
    pens = train_and_compare(model, ref, [rng.randn(5, 21, 4).astype(np.float32)], rng.randn(5, 2).astype(np.float32), what='conv-rnn')
    assert min(pens) > 0.05                                                 # the loss was held against loss + penalty: the penalty is no rounding matter


def test_stacked_rnn_with_a_reversed_relu_layer_trains_as_torch_fp64():
    """return_sequences=True, then go_backwards=True with relu, binary cross-entropy"""
    from gennet_amd import layers as Ly
    first = Ly.SimpleRNN(8, return_sequences=True, input_shape=(7, 3))
    second = Ly.SimpleRNN(5, go_backwards=True, activation='relu')
    head = Ly.Dense(1, activation='sigmoid')
    model = sequential(first, second, head)
    rng = np.random.RandomState(32)
    seed_biases(model, rng)

    def ref(P, x):
        return torch.sigmoid(rnn_ref(P, second, rnn_ref(P, first, x)) @ P[head.name][0] + P[head.name][1])
    train_and_compare(model, ref, [rng.randn(6, 7, 3).astype(np.float32)], (rng.rand(6, 1) < 0.5).astype(np.float32), loss='binary_crossentropy',
                      what='stacked')


def test_weight_gradients_summed_in_row_parts_train_as_torch_fp64():
    """B T = 16 x 64 = 1024 rows: dW and dU are formed in 4 row parts as one batched product and summed by the fixed-order column reduction
    (recurrent.row_splits / rows_product); the models above take the single product"""
    from gennet_amd import layers as Ly
    from gennet_amd.recurrent import row_splits
    assert [row_splits(16 * 64, c) for c in (3 * 5, 5 * 5)] == [4, 4] and row_splits(5 * 9, 8 * 12) == 1
    rnn, head = Ly.SimpleRNN(5, input_shape=(64, 3)), Ly.Dense(1)
    model = sequential(rnn, head)
    rng = np.random.RandomState(37)
    seed_biases(model, rng)

    def ref(P, x):
        return rnn_ref(P, rnn, x) @ P[head.name][0] + P[head.name][1]
    train_and_compare(model, ref, [rng.randn(16, 64, 3).astype(np.float32)], rng.randn(16, 1).astype(np.float32), what='row parts')


def one_layer_model(inner, merge_mode, T=9, Cin=4):
    from gennet_amd import layers as Ly
    bi = Ly.Bidirectional(inner, merge_mode=merge_mode, input_shape=(T, Cin))
    head = Ly.Dense(1)
    seq = inner.return_sequences
    model = sequential(bi, Ly.GlobalAveragePooling1D(), head) if seq else sequential(bi, head)

    def ref(P, x, frozen=None):
        y = bi_ref(P[bi.name] if frozen is None else frozen, bi, x)
        return (y.mean(1) if seq else y) @ P[head.name][0] + P[head.name][1]
    return model, ref


# id -> (the inner layer's keywords, merge_mode): the four merge modes, return_sequences both ways, the inner go_backwards
BI_MODELS = {
    'concat-seq': (dict(units=7, return_sequences=True), 'concat'),
    'sum-last': (dict(units=6), 'sum'),
    'mul-seq-relu': (dict(units=6, return_sequences=True, activation='relu'), 'mul'),
    'ave-seq-go-backwards': (dict(units=5, return_sequences=True, go_backwards=True), 'ave'),
    'concat-last-go-backwards': (dict(units=20, go_backwards=True, activation='sigmoid'), 'concat'),
    'mul-last': (dict(units=6), 'mul'),
}


@pytest.mark.parametrize('which', sorted(BI_MODELS))
def test_a_bidirectional_simple_rnn_trains_as_torch_fp64(which):
    from gennet_amd import layers as Ly
    kw, mode = BI_MODELS[which]
    inner = Ly.SimpleRNN(**kw)
    model, ref = one_layer_model(inner, mode)
    rng = np.random.RandomState(42 + sorted(BI_MODELS).index(which))
    seed_all_biases(model, rng)
    u = inner.units * (2 if mode == 'concat' else 1)
    assert model.nodes[0].out_shape == ((9, u) if inner.return_sequences else (u,)) and len(model.layers[0].weights) == 6
    train_and_compare(model, ref, [rng.randn(6, 9, 4).astype(np.float32)], rng.randn(6, 1).astype(np.float32), what=which)


def test_a_frozen_first_bidirectional_layer_forms_no_input_gradient(monkeypatch):
    """the wrapper frozen and first: its six weights stay, no dX is formed (recurrent._input_grad is not called), and the head behind it trains
    as torch fp64 steps it: train_and_compare's loss bound, 1e-6 relative, over three steps"""
    from gennet_amd import layers as Ly, recurrent
    from gennet_amd.engine import SGD
    model, ref = one_layer_model(Ly.SimpleRNN(6, return_sequences=True), 'concat')
    bi, head = model.layers[0], model.layers[-1]
    bi.trainable = False
    rng = np.random.RandomState(61)
    seed_all_biases(model, rng)
    before = [w.copy() for w in bi.get_weights()]
    frozen = [torch.tensor(w.astype(np.float64)) for w in before]
    calls = []
    real = recurrent._input_grad
    monkeypatch.setattr(recurrent, '_input_grad', lambda *a, **k: calls.append(1) or real(*a, **k))
    model.compile(optimizer=SGD(lr=LR), loss='mean_squared_error')
    x, t = rng.randn(6, 9, 4).astype(np.float32), rng.randn(6, 1).astype(np.float32)
    P = torch_params([head])
    xt, tt = torch.tensor(x.astype(np.float64)), torch.tensor(t.astype(np.float64))
    losses = []
    for step in range(3):
        for v in P[head.name]:
            v.grad = None
        loss_ref = ((ref(P, xt, frozen) - tt) ** 2).mean()
        loss_ref.backward()
        got = model.train_on_batch(x, t)
        got = got[0] if isinstance(got, (list, tuple)) else got
        assert abs(got - float(loss_ref.detach())) <= 1e-6 * abs(float(loss_ref.detach())), (step, got, float(loss_ref.detach()))
        losses.append(got)
        with torch.no_grad():
            for v in P[head.name]:
                v -= LR * v.grad
    assert len(set(losses)) == 3 and not calls
    assert all(np.array_equal(a, b) for a, b in zip(before, bi.get_weights()))


def test_save_and_load_round_trip(tmp_path):
    """.h5, and JSON + weights: the loaded model predicts the same bits and trains on as the original"""
    from gennet_amd.engine import SGD, load_model, model_from_json
    model, _ = conv_rnn_model()
    rng = np.random.RandomState(34)
    seed_biases(model, rng)
    x, t = rng.randn(5, 21, 4).astype(np.float32), rng.randn(5, 2).astype(np.float32)
    model.compile(optimizer=SGD(lr=LR), loss='mean_squared_error')
    model.train_on_batch(x, t)
    path = os.path.join(str(tmp_path), 'conv_rnn.h5')
    model.save(path)
    again = load_model(path)
    assert [type(n.layer).__name__ for n in again.nodes] == ['Conv1D', 'SimpleRNN', 'Dense']
    rnn = again.layers[1]
    assert [p.name for p in rnn.weights] == ['%s/%s' % (rnn.name, n) for n in ('kernel', 'recurrent_kernel', 'bias')]
    from gennet_amd import h5lite, keras_io
    names = keras_io._decode_list(h5lite.File(path)['model_weights'][rnn.name].attrs.get('weight_names'))
    assert names ==['%s/%s:0' % (rnn.name, n) for n in ('kernel', 'recurrent_kernel', 'bias')]
    assert rnn.get_config() == model.layers[1].get_config() and rnn.recurrent_kernel.regularizer.l2 == np.float32(0.01)
    assert all(np.array_equal(u, v) for u, v in zip(model.get_weights(), again.get_weights()))
    assert np.array_equal(model.predict(x), again.predict(x))
    twin = model_from_json(model.to_json())                                 # JSON + weights
    twin.set_weights(model.get_weights())
    assert np.array_equal(model.predict(x), twin.predict(x))
    a, b = model.train_on_batch(x, t), again.train_on_batch(x, t)
    assert a == b and all(np.array_equal(u, v) for u, v in zip(model.get_weights(), again.get_weights()))


def test_a_bidirectional_model_saves_and_loads(tmp_path):
    from gennet_amd import layers as Ly
    from gennet_amd.engine import load_model, model_from_json
    model, _ = one_layer_model(Ly.SimpleRNN(7, return_sequences=True, go_backwards=True), 'mul')
    rng = np.random.RandomState(35)
    seed_all_biases(model, rng)
    x = rng.randn(4, 9, 4).astype(np.float32)
    path = os.path.join(str(tmp_path), 'bi_rnn.h5')
    model.save(path)
    again = load_model(path)
    assert [type(n.layer).__name__ for n in again.nodes][0] == 'Bidirectional' and type(again.layers[0].layer).__name__ == 'SimpleRNN'
    assert [p.name for p in again.layers[0].weights] == [p.name for p in model.layers[0].weights]
    assert again.layers[0].get_config() == model.layers[0].get_config()
    assert np.array_equal(model.predict(x), again.predict(x))
    twin = model_from_json(model.to_json())
    twin.set_weights(model.get_weights())
    assert np.array_equal(model.predict(x), twin.predict(x))


def test_predict_allocates_no_tape():
    from gennet_amd import engine
    model, _ = conv_rnn_model()
    x = np.random.RandomState(35).randn(3, 21, 4).astype(np.float32)
    ctx = engine.RunContext(False)
    out = model._forward(model._prep_inputs(x), ctx)
    assert tuple(out[0].shape) == (3, 2) and model.nodes[1].index not in ctx.tape
    ctx = engine.RunContext(True)
    model._forward(model._prep_inputs(x), ctx)
    kept = ctx.tape[model.nodes[1].index]
    assert [tuple(v.shape) for v in kept] == [(3, 9, 8), (3, 9, 12), (3, 9, 12)]          # x, hprev, the stored h_t


def captured_step_replays(make, x_shape, t_shape, seed_fn):
    """eager step, capture, three replays against four eager steps of a twin"""
    from gennet_amd import engine
    from gennet_amd.engine import SGD, to_device
    rng = np.random.RandomState(36)
    x, t = to_device(rng.randn(*x_shape).astype(np.float32)), to_device(rng.randn(*t_shape).astype(np.float32))
    eager, _ = make()
    seed_fn(eager, rng)
    graphed, _ = make()
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
        assert all(np.array_equal(u, v) for u, v in zip(w0, w1)), step
    assert not np.array_equal(want[0][0], want[3][0])                      # the steps differ: a replay that did nothing would show


def test_a_captured_step_replays_bit_identically():
    """the Conv1D -> SimpleRNN -> Dense model as a hipGraph (engine.StepGraph)"""
    captured_step_replays(conv_rnn_model, (5, 21, 4), (5, 2), seed_biases)


def test_a_captured_bidirectional_step_replays_bit_identically():
    """the pointer tables of the pair launch are host arguments read at the call, so the captured launches carry the addresses"""
    from gennet_amd import layers as Ly
    captured_step_replays(lambda: one_layer_model(Ly.SimpleRNN(7, return_sequences=True), 'concat'), (5, 9, 4), (5, 1), seed_all_biases)
