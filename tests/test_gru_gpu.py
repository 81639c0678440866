"""GPU parity of keras layers.GRU, both reset_after forms: csrc/gru.hip through gn_gru_fwd / gn_gru_bwd against the fp64 definition tests/gru_ref.py
(itself checked against torch.nn.GRU and torch autograd in tests/test_gru_cpu.py), and the layer at model level against torch fp64 autograd on the
CPU.  The Guarded buffers, the activation error table and train_and_compare are those of tests/test_lstm_gpu.py.

Section 1, kernel level.  Inputs sit in NaN-surrounded buffers, outputs in sentinel-filled ones, a view 36 or 37 floats in.  What a form does not
take is there all the same: without reset_after the recurrent bias is a buffer of NaN and dzr a sentinel-filled one that must stay untouched.
R.SHAPES is LSTM's covering set of (B, T, Cin, u) with u moved to the edges of csrc/gru_geom.h:
  u    {1, 3, 4, 15, 16, 17, 31, 32, 33, 64, 100, 104, 105, 112, 130, 260, 512}: below one MFMA, both sides of one and of two tiles; 104, the last u
       whose padded U (forward) and U^T (backward) lie in LDS beside the state, and 105, the first streamed one -- the geometry's four
       LDS-or-streamed decisions (two kernels, two directions) fall on this one pair; 100 and 112, k extents of 104 and 112 under seven tiles;
       more tiles than waves (130: two a wave; 260: three; 512: four on 8 waves, the largest u the entry points take)
  B, T, Cin as in tests/test_lstm_gpu.py.
Section 2, model level: the bounds of tests/test_merge_gpu.py's train_and_compare as they stand, over three SGD steps."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gru_ref as R
from test_lstm_gpu import ACT_ERR, EPS, LR, Guarded, dev, same_bits, seed_biases, seq_sum_f32, train_and_compare

pytestmark = pytest.mark.gpu

SHAPES, IDS = R.SHAPES, R.IDS
FORMS = pytest.mark.parametrize('reset_after', [False, True], ids=['ra0', 'ra1'])


def test_the_shapes_cover_the_set():
    assert set(s[0] for s in SHAPES) == {1, 2, 15, 16, 17, 33} and set(s[1] for s in SHAPES) == {1, 2, 3, 17}
    assert set(s[2] for s in SHAPES) == {1, 3, 16, 17} and len(SHAPES) == 24
    assert set(s[3] for s in SHAPES) >= {1, 3, 4, 15, 16, 17, 31, 32, 33, 64, 130, 260, 512}          # the tile and wave edges


def geometry(u):
    """csrc/gru_geom.h, restated: (tiles a wave, waves, U in LDS forward, U^T in LDS backward, workspace bytes forward, backward)"""
    KP, UP = -(-u // 8) * 8, -(-u // 16) * 16
    SU, SUT = (3 * UP) | 16, UP | 16
    ntiles = UP // 16
    NT = -(-ntiles // 8)
    fwd = 2 * 16 * (KP + 1) * 4 + KP * SU * 4
    bwd = 16 * (3 * KP + 1) * 4 + 3 * KP * SUT * 4
    return NT, -(-ntiles // NT), fwd <= 160 * 1024, bwd <= 160 * 1024, KP * SU * 4, 3 * KP * SUT * 4


def test_the_shapes_straddle_the_kernel_edges():
    us = set(s[3] for s in SHAPES)
    g = dict((u, geometry(u)) for u in range(1, 513))
    for side in (2, 3):                      # forward, backward: the set holds the last u in LDS and the first streamed one
        last = max(u for u in g if g[u][side])
        assert all(g[u][side] == (u <= last) for u in g) and last in us and last + 1 in us, (side, last)
    assert g[104][2] and g[104][3] and not g[105][2] and not g[105][3]
    assert [g[u][:2] for u in (1, 16, 17, 64, 104, 105, 130, 260, 512)] == [(1, 1), (1, 1), (1, 2), (1, 4), (1, 7), (1, 7), (2, 5), (3, 6), (4, 8)]
    from gennet_amd import _lib
    for u in us:
        assert _lib.size('gn_gru_fwd_workspace', u) == g[u][4] and _lib.size('gn_gru_bwd_workspace', u) == g[u][5]


def run_kernels(zx, U, b, rb, h0, dy, activation, recurrent_activation, reverse, pad=37, training=True):
    """gn_gru_fwd (training phase) and gn_gru_bwd on guarded buffers; reset_after is `rb is not None`.
    -> h (processing order); gates, hprev, aux, dz, dzr (input time order; dzr under reset_after only); dh0"""
    from gennet_amd import _lib, ops
    B, T, u3 = zx.shape
    u = u3 // 3
    ra = rb is not None
    nan_rb = np.full(u3, np.nan, np.float32)                       # not looked at without reset_after
    gi = dict((k, None if v is None else Guarded(np.shape(v), v, pad)) for k, v in dict(zx=zx, U=U, b=b, rb=rb if ra else nan_rb, h0=h0, dy=dy).items())
    go = dict((k, Guarded(s, None, pad)) for k, s in dict(h=(B, T, u), gates=(B, T, u3), hprev=(B, T, u), aux=(B, T, u), dz=(B, T, u3), dzr=(B, T, u3),
                                                         dh0=(B, u)).items())
    p = dict((k, None if v is None else v.t.data_ptr()) for k, v in list(gi.items()) + list(go.items()))
    s = torch.cuda.current_stream().cuda_stream
    act, ract = ops.LSTM_ACT[activation], ops.LSTM_ACT[recurrent_activation]
    ws = ops.workspace(_lib.size('gn_gru_fwd_workspace', u), dev())
    _lib.call('gn_gru_fwd', p['zx'], p['U'], p['b'], p['rb'], p['h0'], p['h'], p['gates'], p['hprev'], p['aux'], ws.data_ptr(), ws.numel(), B, T, u, act,
              ract, int(ra), int(reverse), int(training), s)
    out = dict(h=go['h'].check('gru_fwd h'))
    if not training:
        torch.cuda.synchronize()
        assert all(go[k].untouched() for k in ('gates', 'hprev', 'aux'))
        return out
    for k in ('gates', 'hprev', 'aux'):
        out[k] = go[k].check('gru_fwd ' + k)
    ws = ops.workspace(_lib.size('gn_gru_bwd_workspace', u), dev())
    _lib.call('gn_gru_bwd', p['dy'], p['gates'], p['hprev'], p['aux'], p['U'], p['dz'], p['dzr'], p['dh0'], ws.data_ptr(), ws.numel(), B, T, u, act, ract,
              int(ra), int(reverse), int(np.ndim(dy) == 3), s)
    for k in ('dz', 'dh0') + (('dzr',) if ra else ()):
        out[k] = go[k].check('gru_bwd ' + k)
    if not ra:
        torch.cuda.synchronize()
        assert go['dzr'].untouched()
    return out


def reference_at_input_time(k, r):
    """the reference's stored tensors as the kernels index them"""
    t = lambda a: np.ascontiguousarray(R.at_input_time(a, k['go_backwards']))          # noqa: E731
    want = dict(h=k['h'], gates=t(k['gates']), hprev=t(k['h_prev']), aux=t(k['aux']), dz=t(r['dz']), dh0=r['dh0'])
    if k['reset_after']:
        want['dzr'] = t(r['dzr'])
    return want


@FORMS
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_integer_sequences_are_exact(shape, reset_after):
    """activation='linear', hard_sigmoid z and r saturated by biases of +-8 (exactly 0 or 1, mixed per unit), integer x in [-2, 2], W, U (and rb)
    non-zero in the h block only with entries in {-1, 0, 1} (U_h about 15 % dense), integer h0 and dy, at most 5 steps: every value, product and
    partial sum of the forward and of the backward is an integer below 2^24 (asserted on the sums of absolute values), so ANY correct kernel
    returns the reference's h, gates, hprev, aux, dz, dzr, dh0 bit for bit -- and a swapped gate block, a wrong time index, a wrong lane map, a
    dropped k group, r applied on the wrong side of the product or a reversed direction does not.  Both time directions, dy as a sequence and
    for the last step only.  What this CANNOT reach is the [da_z, da_r] . U^T part of dh_{t-1} and the r block of U: a saturated gate's
    derivative is 0, so da_z = da_r = 0 here; the sequence test covers that path."""
    B, T, Cin, u = shape
    T = min(T, 5)
    rng = np.random.RandomState(B * 1000 + T * 100 + Cin * 10 + u)
    x = rng.randint(-2, 3, (B, T, Cin)).astype(np.float64)
    W, U = np.zeros((Cin, 3 * u)), np.zeros((u, 3 * u))
    W[:, 2 * u:] = rng.randint(-1, 2, (Cin, u))
    U[:, 2 * u:] = rng.randint(-1, 2, (u, u)) * (rng.rand(u, u) < (0.15 if u > 8 else 0.6))
    b = np.zeros(3 * u)
    b[:u], b[u:2 * u], b[2 * u:] = 8.0 * rng.choice([-1, 1], u), 8.0 * rng.choice([-1, 1, 1], u), rng.randint(-1, 2, u)
    rb = None
    if reset_after:
        rb = np.zeros(3 * u)
        rb[2 * u:] = rng.randint(-1, 2, u)
    h0 = rng.randint(-2, 3, (B, u)).astype(np.float64)
    zx = x @ W
    for reverse, seq in ((False, True), (True, True), (True, False)):
        dy = rng.randint(-1, 2, (B, T, u) if seq else (B, u)).astype(np.float64)
        k = R.recurrence(zx, U, b, rb, h0, 'linear', 'hard_sigmoid', reset_after, reverse)
        r = R.recurrence_backward(k, dy)
        want = reference_at_input_time(k, r)
        assert set(np.unique(k['gates'][:, :, :2 * u])) <= {0.0, 1.0}
        aU = np.abs(U)
        grads = np.abs(r['dz']) + (np.abs(r['dzr']) if reset_after else 0)
        big = max(float((np.abs(k['h_prev']) @ aU).max() + (np.abs(k['aux']) @ aU).max() + np.abs(zx).max() + 10),
                  float(2 * (grads @ aU.T).max() + 2 * np.abs(r['dz']).max() + 1), 2 * max(float(np.abs(v).max()) for v in want.values()))
        assert big < 2 ** 24, big
        assert all(np.array_equal(v, np.rint(v)) for v in want.values())
        for pad in (37, 36):
            got = run_kernels(zx, U, b, rb, h0, dy, 'linear', 'hard_sigmoid', reverse, pad)
            assert set(got) == set(want)
            for name, v in want.items():
                assert same_bits(got[name], v.astype(np.float32)), (name, reverse, seq, pad, int((got[name] != v).sum()))
    print(shape, reset_after, 'largest magnitude', big)


ONE_STEP_PAIRS = [('tanh', 'hard_sigmoid'), ('sigmoid', 'sigmoid'), ('relu', 'hard_sigmoid'), ('linear', 'sigmoid')]


@FORMS
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_one_step_meets_the_derived_bound(shape, reset_after):
    """T = 1 with random h0, against the fp64 evaluation of the same fp32 inputs, e = 2^-24, first order (Higham (3.4)), as
    tests/test_lstm_gpu.py's test of this name, whose ACT_ERR table gives each activation's own error e_fn; every activation has a Lipschitz
    constant <= 1, and 1 is used.
      z, r     reset_after=False: pre = chain + (zx + b): a term passes at most units + 2 roundings,
                   d_pre = (units + 2) e (sum_k |h U| + |zx| + |b|);      reset_after=True: pre = (chain + rb) + (zx + b), the same count:
                   d_pre = (units + 2) e (sum_k |h U| + |rb| + |zx| + |b|).        d_gate = d_pre + e_ra
      aux      reset_after=False: r h with one rounding: d_aux = |h| d_r + e |r h|
               reset_after=True:  q = chain + rb: d_aux = (units + 1) e (sum_k |h U_h| + |rb_h|)
      hh       reset_after=False: pre_h = chain over (r h) U_h + (zx_h + b_h): the chain's own roundings and the error of r h ENTERING it,
                   d_pre_h = (units + 2) e (sum_k |r h| |U_h| + |zx_h| + |b_h|) + sum_k d_aux_k |U_h|
               reset_after=True:  pre_h = (zx_h + b_h) + r q with three roundings: d_pre_h = |q| d_r + |r| d_aux + e (|r q| + |zx_h + b_h| + |pre_h|)
               d_hh = d_pre_h + e_act
      h        z h0 + (1 - z) hh, four roundings: d_h = (|h0| + |hh|) d_z + |1 - z| d_hh + e (|z h0| + 2 |(1 - z) hh| + |h|)
    and 1 % on top for the second-order terms.  Every element of gates, aux and h is compared; hprev must be h0's bits."""
    B, _, Cin, u = shape
    rng = np.random.RandomState(7 + B * 1000 + Cin * 10 + u + int(reset_after))
    f32 = lambda a: a.astype(np.float32)          # noqa: E731
    zx, U, b = f32(rng.randn(B, 1, 3 * u)), f32(rng.randn(u, 3 * u) / np.sqrt(u)), f32(0.5 * rng.randn(3 * u))
    rb = f32(0.5 * rng.randn(3 * u)) if reset_after else None
    h0, dy = f32(rng.rand(B, u) * 2 - 1), f32(rng.randn(B, u))
    A = lambda v: np.abs(np.asarray(v, np.float64))          # noqa: E731
    blk = lambda v, q: v[..., q * u:(q + 1) * u]             # noqa: E731
    for n, (an, rn) in enumerate(ONE_STEP_PAIRS):
        k = R.recurrence(zx, U, b, rb, h0, an, rn, reset_after, bool(n & 1))
        got = run_kernels(zx, U, b, rb, h0, dy, an, rn, bool(n & 1), pad=37 - (n & 1))
        g64, aux64, h64, pre64 = k['gates'][:, 0], k['aux'][:, 0], k['h'][:, 0], k['pre'][:, 0]
        z, r, hh = (blk(g64, q) for q in range(3))
        hU = A(h0) @ A(U)                                                             # sum_k |h U|, (B, 3u)
        arb = A(rb) if reset_after else 0 * A(b)
        d_pre = (u + 2) * EPS * (hU + arb + A(zx[:, 0]) + A(b))
        d_z, d_r = (blk(d_pre, q) + ACT_ERR[rn](blk(g64, q)) for q in range(2))
        if reset_after:
            d_aux = (u + 1) * EPS * (blk(hU, 2) + blk(arb, 2))
            a_h = blk(zx[:, 0].astype(np.float64) + b.astype(np.float64), 2)
            d_pre_h = A(aux64) * d_r + A(r) * d_aux + EPS * (A(r * aux64) + A(a_h) + A(blk(pre64, 2)))
        else:
            d_aux = A(h0) * d_r + EPS * A(aux64)
            Uh = A(U[:, 2 * u:])
            d_pre_h = (u + 2) * EPS * (A(aux64) @ Uh + blk(A(zx[:, 0]) + A(b), 2)) + d_aux @ Uh
        d_hh = d_pre_h + ACT_ERR[an](hh)
        d_h = (A(h0) + A(hh)) * d_z + A(1 - z) * d_hh + EPS * (A(z * h0) + 2 * A((1 - z) * hh) + A(h64))
        d_gates = np.concatenate([d_z, d_r, d_hh], 1)
        for name, ref, bound in (('gates', g64, d_gates), ('aux', aux64, d_aux), ('h', h64, d_h)):
            err = np.abs(got[name][:, 0].astype(np.float64) - ref)
            print(shape, reset_after, an, rn, name, 'worst error / bound %.3g' % (err / (1.01 * bound + 1e-300)).max())
            assert (err <= 1.01 * bound).all(), (an, rn, name, float((err / (1.01 * bound + 1e-300)).max()))
        assert same_bits(got['hprev'][:, 0], h0)


def restatement_backward(k32, dy):
    """tests/gru_ref.py in fp32, the sums over B T rows taken row after row"""
    r = R.recurrence_backward(k32, dy.astype(np.float32))
    t = lambda a: np.ascontiguousarray(R.at_input_time(a, k32['go_backwards']))          # noqa: E731
    flat = lambda a: a.reshape(-1, a.shape[-1])                                          # noqa: E731
    u = k32['h'].shape[2]
    dz_t, hp_t, aux_t = t(r['dz']), flat(t(k32['h_prev'])), flat(t(k32['aux']))
    out = dict(dz=dz_t, dh0=r['dh0'], dx=dz_t @ k32['W'].T, dW=seq_sum_f32(flat(k32['x']), flat(dz_t)),
               db=flat(dz_t).astype(np.float64).sum(0).astype(np.float32))
    if k32['reset_after']:
        dzr_t = t(r['dzr'])
        out.update(dzr=dzr_t, dU=seq_sum_f32(hp_t, flat(dzr_t)), drb=flat(dzr_t).astype(np.float64).sum(0).astype(np.float32))
    else:
        out['dU'] = np.concatenate([seq_sum_f32(hp_t, flat(dz_t)[:, :2 * u]), seq_sum_f32(aux_t, flat(dz_t)[:, 2 * u:])], 1)
    return out


MARGIN = 8.0


@FORMS
@pytest.mark.parametrize('family', ['keras', 'saturating'])
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_sequences_against_the_fp64_reference(shape, family, reset_after):
    """The whole layer arithmetic -- zx = X W (gn_bmm), the recurrence, its backward, dW, dU, dX (gn_bmm), db and d rb -- against
    tests/gru_ref.py in fp64.  The yardstick is the numpy fp32 restatement of the same recurrence, measured against fp64 on the same inputs: the
    GPU's largest error per tensor may be at most MARGIN = 8 times max(the restatement's, 2^-24 max|ref|) -- the project's figure for LSTM: the
    same device functions, the same chain classes.  Two input families (R.draw_family); the seed is R.sequence_case's, chosen from the
    reference alone (tests/test_gru_cpu.py asserts one exists for every case).  No element is excluded from any comparison."""
    from gennet_amd import ops
    B, T, Cin, u = shape
    n = SHAPES.index(shape)
    case = R.sequence_case(shape, family, reset_after)
    assert case is not None
    x, W, U, b, rb, dy, k64, k32 = (case[key] for key in ('x', 'W', 'U', 'b', 'rb', 'dy', 'k64', 'k32'))
    an, rn, reverse = case['activation'], case['recurrent_activation'], case['reverse']
    r64, g64 = R.recurrence_backward(k64, dy), R.backward(k64, dy)
    want = dict(reference_at_input_time(k64, r64), dx=g64['dx'], dW=g64['dW'], dU=g64['dU'], db=g64['db'])
    want.pop('hprev')
    if reset_after:
        want['drb'] = g64['drb']
    t_in = lambda a: R.at_input_time(a, reverse)          # noqa: E731
    rest = dict(h=k32['h'], gates=t_in(k32['gates']), aux=t_in(k32['aux']), **restatement_backward(k32, dy))

    t = lambda a: torch.tensor(np.array(a, dtype=np.float32, order='C'), device=dev())          # noqa: E731
    xt, Wt = t(x), t(W)
    zx = ops.bmm(xt.view(1, B * T, Cin), Wt.view(1, Cin, 3 * u)).view(B, T, 3 * u).cpu().numpy()
    got = run_kernels(zx, U, b, rb, None, dy, an, rn, reverse, pad=37 - (n & 1))
    dz = t(got['dz']).view(1, B * T, 3 * u)
    left = lambda name: t(got[name]).view(1, B * T, u)          # noqa: E731
    got['dW'] = ops.bmm(xt.view(1, B * T, Cin), dz, trans_a=True)[0].cpu().numpy()
    if reset_after:
        dzr = t(got['dzr']).view(1, B * T, 3 * u)
        got['dU'] = ops.bmm(left('hprev'), dzr, trans_a=True)[0].cpu().numpy()
        got['drb'] = ops.bias_grad(dzr.view(B * T, 3 * u)).cpu().numpy()
    else:                                                  # the two column blocks of dU, from their two left operands
        cols = lambda lo, hi: t(got['dz'][:, :, lo:hi]).view(1, B * T, hi - lo)          # noqa: E731
        got['dU'] = np.concatenate([ops.bmm(left('hprev'), cols(0, 2 * u), trans_a=True)[0].cpu().numpy(),
                                    ops.bmm(left('aux'), cols(2 * u, 3 * u), trans_a=True)[0].cpu().numpy()], 1)
    got['dx'] = ops.bmm(dz, Wt.view(1, Cin, 3 * u), trans_b=True).view(B, T, Cin).cpu().numpy()
    got['db'] = ops.bias_grad(dz.view(B * T, 3 * u)).cpu().numpy()
    worst = {}
    for name, ref in want.items():
        yard = max(float(np.abs(rest[name].astype(np.float64) - ref).max()), EPS * float(np.abs(ref).max()))
        err = float(np.abs(got[name].astype(np.float64) - ref).max())
        worst[name] = err / yard if yard else (0.0 if err == 0 else np.inf)
    print(shape, family, 'ra%d' % reset_after, an, rn, 'seed', case['seed'], 'error / yardstick:', ' '.join('%s %.2f' % kv for kv in sorted(worst.items())))
    assert all(v <= MARGIN for v in worst.values()), worst


@FORMS
@pytest.mark.parametrize('u', [104, 105])
def test_a_sample_does_not_depend_on_the_batch_or_the_launch(u, reset_after):
    """Rows 0 and 32 of a B = 33 run (the first row of the first tile, the only row of the third), forward and backward, have the bits of the two
    B = 1 runs of those samples; two identical launches return the same bits.  u = 104: U in LDS; u = 105: streamed."""
    B, T = 33, 5
    rng = np.random.RandomState(u)
    f32 = lambda a: a.astype(np.float32)          # noqa: E731
    zx, U, b = f32(rng.randn(B, T, 3 * u)), f32(rng.randn(u, 3 * u) / np.sqrt(u)), f32(0.5 * rng.randn(3 * u))
    rb = f32(0.5 * rng.randn(3 * u)) if reset_after else None
    h0, dy = f32(0.5 * rng.randn(B, u)), f32(rng.randn(B, T, u))
    for reverse in (False, True):
        whole = run_kernels(zx, U, b, rb, h0, dy, 'tanh', 'hard_sigmoid', reverse)
        again = run_kernels(zx, U, b, rb, h0, dy, 'tanh', 'hard_sigmoid', reverse)
        assert all(same_bits(whole[k], again[k]) for k in whole)
        assert np.abs(whole['dz'][:, :, :2 * u]).max() > 0
        for row in (0, 32):
            one = run_kernels(zx[row:row + 1], U, b, rb, h0[row:row + 1], dy[row:row + 1], 'tanh', 'hard_sigmoid', reverse, pad=36)
            for k in whole:
                assert same_bits(one[k][0], whole[k][row]), (k, row, reverse)


@FORMS
def test_the_inference_phase_stores_nothing(reset_after):
    rng = np.random.RandomState(5)
    zx, U, b = rng.randn(3, 4, 15).astype(np.float32), rng.randn(5, 15).astype(np.float32), np.zeros(15, np.float32)
    rb = rng.randn(15).astype(np.float32) if reset_after else None
    a = run_kernels(zx, U, b, rb, None, None, 'tanh', 'sigmoid', False, training=False)
    assert same_bits(a['h'], run_kernels(zx, U, b, rb, None, rng.randn(3, 5).astype(np.float32), 'tanh', 'sigmoid', False)['h'])


@FORMS
def test_bad_arguments_are_errors_and_launch_nothing(reset_after):
    from gennet_amd import _lib, ops
    B, T, u = 2, 3, 5
    ra = int(reset_after)
    one = lambda *s: np.ones(s, np.float32)          # noqa: E731
    zx, U, b, rb, st, dy, gates, hp, aux = (Guarded(s, one(*s), 36) for s in ((B, T, 3 * u), (u, 3 * u), (3 * u,), (3 * u,), (B, u), (B, T, u),
                                                                              (B, T, 3 * u), (B, T, u), (B, T, u)))
    outs = [Guarded(s, None, 36) for s in ((B, T, u), (B, T, 3 * u), (B, T, u), (B, T, u), (B, T, 3 * u), (B, u))]
    h, og, ohp, oaux, odzr, dh0 = outs
    s = torch.cuda.current_stream().cuda_stream
    ws = ops.workspace(max(_lib.size('gn_gru_fwd_workspace', 512), _lib.size('gn_gru_bwd_workspace', 512)), dev())
    tanh, hard = ops.LSTM_ACT['tanh'], ops.LSTM_ACT['hard_sigmoid']
    good = dict(zx=zx.t.data_ptr(), U=U.t.data_ptr(), b=b.t.data_ptr(), rb=rb.t.data_ptr(), h0=st.t.data_ptr(), h=h.t.data_ptr(), gates=og.t.data_ptr(),
                hprev=ohp.t.data_ptr(), aux=oaux.t.data_ptr(), ws=ws.data_ptr(), ws_bytes=ws.numel(), B=B, T=T, u=u, act=tanh, ract=hard, ra=ra,
                training=1, dy=dy.t.data_ptr(), sgates=gates.t.data_ptr(), shp=hp.t.data_ptr(), saux=aux.t.data_ptr(), dz=og.t.data_ptr(),
                dzr=odzr.t.data_ptr(), dh0=dh0.t.data_ptr())

    def fwd(**kw):
        g = dict(good, **kw)
        _lib.call('gn_gru_fwd', g['zx'], g['U'], g['b'], g['rb'], g['h0'], g['h'], g['gates'], g['hprev'], g['aux'], g['ws'], g['ws_bytes'], g['B'], g['T'],
                  g['u'], g['act'], g['ract'], g['ra'], 0, g['training'], s)

    def bwd(**kw):
        g = dict(good, **kw)
        _lib.call('gn_gru_bwd', g['dy'], g['sgates'], g['shp'], g['saux'], g['U'], g['dz'], g['dzr'], g['dh0'], g['ws'], g['ws_bytes'], g['B'], g['T'],
                  g['u'], g['act'], g['ract'], g['ra'], 1, 1, s)

    def refused(text, fn, code=None):
        with pytest.raises(_lib.GennetHipError) as e:
            fn()
        assert '(%d)' % (_lib.GN_EINVAL if code is None else code) in str(e.value) and text in str(e.value), str(e.value)
        assert text in _lib.lib().gn_last_error().decode()
        torch.cuda.synchronize()
        assert all(o.untouched() for o in outs)

    for k in ('zx', 'U', 'b', 'h', 'ws', 'gates', 'hprev', 'aux') + (('rb',) if ra else ()):
        refused('null pointer', lambda: fwd(**{k: None}))
    for k in ('dy', 'sgates', 'shp', 'saux', 'U', 'dz', 'ws') + (('dzr',) if ra else ()):
        refused('null pointer', lambda: bwd(**{k: None}))
    for call in (fwd, bwd):
        refused('bad shape', lambda: call(T=0))
        refused('bad shape', lambda: call(u=0))
        refused('bad shape', lambda: call(B=-1))
        refused('at most 512', lambda: call(u=513))
        refused('unknown activation code 7', lambda: call(act=7))
        refused('unknown activation code 4', lambda: call(act=hard))
        refused('unknown recurrent activation code 0', lambda: call(ract=tanh))
        refused('unknown recurrent activation code -1', lambda: call(ract=-1))
        refused('reset_after = 2', lambda: call(ra=2))
        refused('reset_after = -1', lambda: call(ra=-1))
        refused('workspace too small', lambda: call(ws_bytes=_lib.size('gn_gru_fwd_workspace' if call is fwd else 'gn_gru_bwd_workspace', u) - 1),
                _lib.GN_EWORKSPACE)
        call(B=0)                                              # nothing to do is not an error, and launches nothing (the pointers are not looked at)
    fwd(B=0, zx=None, h=None, ws=None)
    assert _lib.size('gn_gru_fwd_workspace', 513) == 0 and _lib.size('gn_gru_bwd_workspace', 0) == 0
    torch.cuda.synchronize()
    assert all(o.untouched() for o in outs)
    if not ra:                                                 # what belongs to reset_after is not looked at without it
        fwd(rb=None, gates=None, hprev=None, aux=None, training=0, h0=None)
        bwd(dzr=None, dh0=None)
    else:                                                      # the inference phase takes no storage, and no initial state
        fwd(gates=None, hprev=None, aux=None, training=0, h0=None)
        bwd(dh0=None)
    torch.cuda.synchronize()
    h.check('gru_fwd')
    og.check('gru_bwd dz')
    assert ohp.untouched() and oaux.untouched() and dh0.untouched() and odzr.untouched() == (not ra)
    with pytest.raises(ValueError, match='recurrent kernel'):
        ops.gru_fwd(zx.t, U.t[:, :8].contiguous(), b.t)
    with pytest.raises(ValueError, match='reset_after'):
        ops.gru_fwd(zx.t, U.t, b.t, rb.t, reset_after=False)


# ---------------------------------------------------------------------------------------------------------------------
# section 2: models against torch fp64 autograd (tests/test_lstm_gpu.py's train_and_compare: the bounds of tests/test_merge_gpu.py, three steps)
# ---------------------------------------------------------------------------------------------------------------------
def gru_ref(P, layer, x):
    W, U, b = P[layer.name]
    b, rb = (b[0], b[1]) if layer.reset_after else (b, None)
    return R.torch_forward(x, W, U, b, rb, None, layer.activation, layer.recurrent_activation, layer.reset_after, layer.return_sequences,
                           layer.go_backwards)


def conv_gru_model(reset_after):
    """Conv1D(8, 5, strides=2) -> GRU(12) -> Dense(2); the GRU carries the three weight regularizers"""
    from gennet_amd import layers as Ly, regularizers
    from gennet_amd.engine import Sequential
    conv = Ly.Conv1D(8, 5, strides=2, input_shape=(21, 4))
    gru = Ly.GRU(12, kernel_regularizer=regularizers.l2(0.01), recurrent_regularizer=regularizers.l1(0.002), bias_regularizer=regularizers.l1_l2(0.003, 0.004),
                 reset_after=reset_after)
    head = Ly.Dense(2)
    model = Sequential()
    for l in (conv, gru, head):
        model.add(l)

    def ref(P, x):
        w, b = P[conv.name]
        c = F.conv1d(x.permute(0, 2, 1), w.permute(2, 1, 0), stride=2).permute(0, 2, 1) + b
        return gru_ref(P, gru, c) @ P[head.name][0] + P[head.name][1]
    return model, ref


@FORMS
def test_conv_gru_dense_trains_as_torch_fp64_and_its_penalty_shows(reset_after):
    model, ref = conv_gru_model(reset_after)
    rng = np.random.RandomState(31)
    seed_biases(model, rng)
    assert model.output_shape == (None, 2) and [n.out_shape for n in model.nodes] == [(9, 8), (12,), (2,)]
    assert model.layers[1].bias.shape == ((2, 36) if reset_after else (36,))
    pens = train_and_compare(model, ref, [rng.randn(5, 21, 4).astype(np.float32)], rng.randn(5, 2).astype(np.float32), what='conv-gru ra%d' % reset_after)
    assert min(pens) > 0.05                                                 # the loss was held against loss + penalty: the penalty is no rounding matter


@FORMS
def test_stacked_gru_with_a_reversed_relu_layer_trains_as_torch_fp64(reset_after):
    """return_sequences=True, reset_after=True with sigmoid gates, then go_backwards=True with relu (in the form under test), binary cross-entropy"""
    from gennet_amd import layers as Ly
    from gennet_amd.engine import Sequential
    first = Ly.GRU(8, return_sequences=True, reset_after=True, recurrent_activation='sigmoid', input_shape=(7, 3))
    second = Ly.GRU(5, go_backwards=True, activation='relu', reset_after=reset_after)
    head = Ly.Dense(1, activation='sigmoid')
    model = Sequential()
    for l in (first, second, head):
        model.add(l)
    rng = np.random.RandomState(32)
    seed_biases(model, rng)

    def ref(P, x):
        return torch.sigmoid(gru_ref(P, second, gru_ref(P, first, x)) @ P[head.name][0] + P[head.name][1])
    train_and_compare(model, ref, [rng.randn(6, 7, 3).astype(np.float32)], (rng.rand(6, 1) < 0.5).astype(np.float32), loss='binary_crossentropy',
                      what='stacked ra%d' % reset_after)


@FORMS
def test_weight_gradients_summed_in_row_parts_train_as_torch_fp64(reset_after):
    """B T = 16 x 64 = 1024 rows: dW and dU (under reset_after=False each of its two column blocks) are formed in 4 row parts as one batched
    product and summed by the fixed-order column reduction (recurrent.row_splits / rows_product); the models above take the single product"""
    from gennet_amd import layers as Ly
    from gennet_amd.engine import Sequential
    from gennet_amd.recurrent import row_splits
    assert [row_splits(16 * 64, c) for c in (3 * 15, 5 * 15, 5 * 10, 5 * 5)] == [4, 4, 4, 4] and row_splits(5 * 9, 8 * 36) == 1
    gru, head = Ly.GRU(5, input_shape=(64, 3), reset_after=reset_after), Ly.Dense(1)
    model = Sequential()
    model.add(gru)
    model.add(head)
    rng = np.random.RandomState(37)
    seed_biases(model, rng)

    def ref(P, x):
        return gru_ref(P, gru, x) @ P[head.name][0] + P[head.name][1]
    train_and_compare(model, ref, [rng.randn(16, 64, 3).astype(np.float32)], rng.randn(16, 1).astype(np.float32), what='row parts ra%d' % reset_after)


@FORMS
def test_save_and_load_round_trip(tmp_path, reset_after):
    from gennet_amd.engine import SGD, load_model
    model, _ = conv_gru_model(reset_after)
    rng = np.random.RandomState(34)
    seed_biases(model, rng)
    x, t = rng.randn(5, 21, 4).astype(np.float32), rng.randn(5, 2).astype(np.float32)
    model.compile(optimizer=SGD(lr=LR), loss='mean_squared_error')
    model.train_on_batch(x, t)
    path = os.path.join(str(tmp_path), 'conv_gru.h5')
    model.save(path)
    again = load_model(path)
    assert [type(n.layer).__name__ for n in again.nodes] == ['Conv1D', 'GRU', 'Dense']
    gru = again.layers[1]
    assert [p.name for p in gru.weights] == ['%s/%s' % (gru.name, n) for n in ('kernel', 'recurrent_kernel', 'bias')]
    assert gru.bias.shape == ((2, 36) if reset_after else (36,)) and gru.reset_after == reset_after
    assert gru.get_config() == model.layers[1].get_config() and gru.recurrent_kernel.regularizer.l1 == np.float32(0.002)
    assert all(np.array_equal(u, v) for u, v in zip(model.get_weights(), again.get_weights()))
    assert np.array_equal(model.predict(x), again.predict(x))
    a, b = model.train_on_batch(x, t), again.train_on_batch(x, t)
    assert a == b and all(np.array_equal(u, v) for u, v in zip(model.get_weights(), again.get_weights()))


@FORMS
def test_predict_allocates_no_tape(reset_after):
    from gennet_amd import engine
    model, _ = conv_gru_model(reset_after)
    x = np.random.RandomState(35).randn(3, 21, 4).astype(np.float32)
    ctx = engine.RunContext(False)
    out = model._forward(model._prep_inputs(x), ctx)
    assert tuple(out[0].shape) == (3, 2) and model.nodes[1].index not in ctx.tape
    ctx = engine.RunContext(True)
    model._forward(model._prep_inputs(x), ctx)
    kept = ctx.tape[model.nodes[1].index]
    assert [tuple(v.shape) for v in kept] == [(3, 9, 8), (3, 9, 12), (3, 9, 36), (3, 9, 12)]          # x, hprev, the gates, aux


@FORMS
def test_a_captured_step_replays_bit_identically(reset_after):
    """the Conv1D -> GRU -> Dense model as a hipGraph (engine.StepGraph): eager step, capture, three replays against four eager steps of a twin"""
    from gennet_amd import engine
    from gennet_amd.engine import SGD, to_device
    rng = np.random.RandomState(36)
    x, t = to_device(rng.randn(5, 21, 4).astype(np.float32)), to_device(rng.randn(5, 2).astype(np.float32))
    eager, _ = conv_gru_model(reset_after)
    seed_biases(eager, rng)
    graphed, _ = conv_gru_model(reset_after)
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
