"""GPU parity of keras layers.LSTM: csrc/lstm.hip through gn_lstm_fwd / gn_lstm_bwd against the fp64 definition tests/lstm_ref.py (itself checked
against torch.nn.LSTM and torch autograd in tests/test_lstm_cpu.py), and the layer at model level against torch fp64 autograd on the CPU.

Section 1, kernel level.  Inputs sit in NaN-surrounded buffers, outputs in sentinel-filled ones; a view starts 144 bytes in (pad 36: 16-byte
aligned) or 148 bytes in (pad 37: every base pointer moved by one float).  SHAPES is a covering set of (B, T, Cin, u) that straddles the
kernel's own edges (csrc/lstm_geom.h):
  B    {1, 2, 15, 16, 17, 33}: a block carries 16 batch rows -- below a tile, both sides of it, three tiles with one row in the last
  u    {1, 3, 4, 15, 16, 17, 31, 32, 33, 64, 80, 81, 88, 89, 100, 130, 260, 512}: below one MFMA (16 units a wave tile, k in groups of 4 padded to
       a multiple of 8), both sides of one and of two tiles, the last u with U^T in LDS for the backward (80) and the first streamed (81), the
       same for U in the forward (88 | 89), more tiles than waves (130: 9 tiles on 5 waves, two a wave; 260: three a wave; 512: four a wave on
       8 waves, the largest u the entry points take)
  Cin  {1, 3, 16, 17}: the input projection and its gradients are gn_bmm over B T rows (Cin = 1: its matrix-vector kernel)
  T    {1, 2, 3, 17}: one step (no recurrence), both LDS copies of h, an odd count, a longer walk
Section 2, model level: the bounds of tests/test_merge_gpu.py's train_and_compare as they stand, over three SGD steps -- predict 1e-5 of the
largest output, each loss 1e-6 relative, gradients and SGD-updated weights 1e-4 of each tensor's largest entry (gradients no finer than 1e-3 of
the model's largest gradient entry)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lstm_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5
EPS = 2.0 ** -24                  # unit roundoff of fp32


def dev():
    return torch.device('cuda:0')


class Guarded(object):
    """A contiguous view `pad` floats into a larger flat buffer: inputs surrounded by NaN, outputs inside a sentinel-filled buffer."""

    def __init__(self, shape, value=None, pad=37):
        self.n, self.pad = int(np.prod(shape)), pad
        self.buf = torch.full((self.n + 2 * pad,), float('nan') if value is not None else SENTINEL, dtype=torch.float32, device=dev())
        self.t = self.buf[pad:pad + self.n].view(shape)
        if value is not None:
            self.t.copy_(torch.tensor(np.ascontiguousarray(value, np.float32), device=dev()))
        assert self.t.is_contiguous() and self.t.data_ptr() == self.buf.data_ptr() + 4 * pad and (self.t.data_ptr() % 16 == 0) == (pad % 4 == 0)

    def check(self, what):
        """the surroundings untouched, every element of the view written"""
        edges = torch.cat([self.buf[:self.pad], self.buf[self.pad + self.n:]])
        assert bool((edges == SENTINEL).all()), '%s: wrote outside its output' % what
        assert not bool((self.t == SENTINEL).any()), '%s: output elements left unwritten' % what
        assert not bool(torch.isnan(self.t).any()), '%s: NaN (an element outside an input was read)' % what
        return self.t.cpu().numpy()

    def untouched(self):
        return bool((self.buf == SENTINEL).all())


def same_bits(a, b):
    """bit for bit, the sign of a zero aside (x + 0 turns -0 into +0)"""
    a, b = np.ascontiguousarray(a, np.float32) + np.float32(0), np.ascontiguousarray(b, np.float32) + np.float32(0)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# (B, T, Cin, u)
SHAPES = [(1, 1, 1, 1), (2, 2, 3, 3), (15, 3, 16, 4), (16, 17, 17, 15), (17, 1, 1, 16), (33, 2, 3, 17), (1, 3, 16, 31), (2, 17, 17, 32),
          (15, 1, 3, 33), (16, 2, 1, 64), (17, 3, 17, 80), (33, 1, 16, 81), (1, 2, 16, 88), (2, 3, 1, 89), (15, 2, 3, 100), (16, 1, 17, 130),
          (2, 2, 16, 260), (2, 3, 3, 512), (1, 17, 1, 64), (2, 1, 17, 100), (17, 2, 3, 130), (33, 17, 16, 4), (17, 1, 1, 512), (15, 2, 1, 33)]
IDS = ['b%d-t%d-c%d-u%d' % s for s in SHAPES]


def test_the_shapes_cover_the_set():
    assert set(s[0] for s in SHAPES) == {1, 2, 15, 16, 17, 33} and set(s[1] for s in SHAPES) == {1, 2, 3, 17}
    assert set(s[2] for s in SHAPES) == {1, 3, 16, 17}
    assert set(s[3] for s in SHAPES) == {1, 3, 4, 15, 16, 17, 31, 32, 33, 64, 80, 81, 88, 89, 100, 130, 260, 512}
    assert len(SHAPES) == 24


def geometry(u):
    """csrc/lstm_geom.h, restated: (tiles a wave, waves, U in LDS forward, U^T in LDS backward)"""
    KP, UP = -(-u // 8) * 8, -(-u // 16) * 16
    ntiles = UP // 16
    NT = -(-ntiles // 8)
    fwd = 2 * 16 * (KP + 1) * 4 + KP * (4 * UP + 16) * 4
    bwd = 16 * (4 * KP + 1) * 4 + 4 * KP * (UP | 16) * 4
    return NT, -(-ntiles // NT), fwd <= 160 * 1024, bwd <= 160 * 1024


def test_the_shapes_straddle_the_kernel_edges():
    g = dict((u, geometry(u)) for u in set(s[3] for s in SHAPES))
    assert g[80][3] and not g[81][3] and g[88][2] and not g[89][2]
    assert [g[u][:2] for u in (1, 16, 17, 64, 130, 260, 512)] == [(1, 1), (1, 1), (1, 2), (1, 4), (2, 5), (3, 6), (4, 8)]
    from gennet_amd import _lib
    for u in g:
        KP, UP = -(-u // 8) * 8, -(-u // 16) * 16
        assert _lib.size('gn_lstm_fwd_workspace', u) == KP * (4 * UP + 16) * 4 and _lib.size('gn_lstm_bwd_workspace', u) == 4 * KP * (UP | 16) * 4


def run_kernels(zx, U, b, h0, c0, dy, activation, recurrent_activation, reverse, pad=37, training=True):
    """gn_lstm_fwd (training phase) and gn_lstm_bwd on guarded buffers -> h (processing order); gates, c, hprev, dz (input time order); dh0, dc0"""
    from gennet_amd import _lib, ops
    B, T, u4 = zx.shape
    u = u4 // 4
    gi = dict((k, None if v is None else Guarded(np.shape(v), v, pad)) for k, v in dict(zx=zx, U=U, b=b, h0=h0, c0=c0, dy=dy).items())
    go = dict((k, Guarded(s, None, pad)) for k, s in dict(h=(B, T, u), gates=(B, T, u4), c=(B, T, u), hprev=(B, T, u), dz=(B, T, u4), dh0=(B, u),
                                                         dc0=(B, u)).items())
    p = dict((k, None if v is None else v.t.data_ptr()) for k, v in list(gi.items()) + list(go.items()))
    s = torch.cuda.current_stream().cuda_stream
    act, ract = ops.LSTM_ACT[activation], ops.LSTM_ACT[recurrent_activation]
    ws = ops.workspace(_lib.size('gn_lstm_fwd_workspace', u), dev())
    _lib.call('gn_lstm_fwd', p['zx'], p['U'], p['b'], p['h0'], p['c0'], p['h'], p['gates'], p['c'], p['hprev'], ws.data_ptr(), ws.numel(), B, T, u, act,
              ract, int(reverse), int(training), s)
    out = dict(h=go['h'].check('lstm_fwd h'))
    if not training:
        torch.cuda.synchronize()
        assert all(go[k].untouched() for k in ('gates', 'c', 'hprev'))
        return out
    for k in ('gates', 'c', 'hprev'):
        out[k] = go[k].check('lstm_fwd ' + k)
    ws = ops.workspace(_lib.size('gn_lstm_bwd_workspace', u), dev())
    _lib.call('gn_lstm_bwd', p['dy'], p['gates'], p['c'], p['c0'], p['U'], p['dz'], p['dh0'], p['dc0'], ws.data_ptr(), ws.numel(), B, T, u, act, ract,
              int(reverse), int(np.ndim(dy) == 3), s)
    for k in ('dz', 'dh0', 'dc0'):
        out[k] = go[k].check('lstm_bwd ' + k)
    return out


def reference_at_input_time(k, r):
    """the reference's stored tensors as the kernels index them"""
    t = lambda a: np.ascontiguousarray(R.at_input_time(a, k['go_backwards']))          # noqa: E731
    return dict(h=k['h'], gates=t(k['gates']), c=t(k['c']), hprev=t(r['h_prev']), dz=t(r['dz']), dh0=r['dh0'], dc0=r['dc0'])


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_integer_sequences_are_exact(shape):
    """activation='linear', hard_sigmoid gates saturated by biases of +-8 (exactly 0 or 1; i, f and o mixed per unit), integer x in [-2, 2], W and U
    non-zero in the c block only with entries in {-1, 0, 1} (U about 15 % dense), integer h0, c0, dy, at most 5 steps: every value, product and
    partial sum of the forward and of the backward is an integer below 2^24 (asserted on the sums of absolute values), so ANY correct kernel returns
    the reference's h, c, gates, hprev, dz, dh0, dc0 bit for bit -- and a swapped gate block, a wrong time index, a wrong lane map, a dropped k
    group or a reversed direction does not.  Both time directions, dy as a sequence and for the last step only."""
    B, T, Cin, u = shape
    T = min(T, 5)
    rng = np.random.RandomState(B * 1000 + T * 100 + Cin * 10 + u)
    x = rng.randint(-2, 3, (B, T, Cin)).astype(np.float64)
    W, U = np.zeros((Cin, 4 * u)), np.zeros((u, 4 * u))
    W[:, 2 * u:3 * u] = rng.randint(-1, 2, (Cin, u))
    U[:, 2 * u:3 * u] = rng.randint(-1, 2, (u, u)) * (rng.rand(u, u) < (0.15 if u > 8 else 0.6))
    b = np.zeros(4 * u)
    b[:u], b[u:2 * u] = 8.0 * rng.choice([-1, 1], u), 8.0 * rng.choice([-1, 1], u)
    b[2 * u:3 * u], b[3 * u:] = rng.randint(-1, 2, u), 8.0 * rng.choice([-1, 1, 1, 1, 1], u)
    h0, c0 = rng.randint(-1, 2, (B, u)).astype(np.float64), rng.randint(-2, 3, (B, u)).astype(np.float64)
    zx = x @ W
    for reverse, seq in ((False, True), (True, True), (True, False)):
        dy = rng.randint(-1, 2, (B, T, u) if seq else (B, u)).astype(np.float64)
        k = R.recurrence(zx, U, b, h0, c0, 'linear', 'hard_sigmoid', reverse)
        r = R.recurrence_backward(k, dy)
        want = reference_at_input_time(k, r)
        assert set(np.unique(k['gates'][:, :, :2 * u])) <= {0.0, 1.0} and set(np.unique(k['gates'][:, :, 3 * u:])) <= {0.0, 1.0}
        hp = np.abs(r['h_prev'])
        big = max(float((hp @ np.abs(U)).max() + np.abs(zx).max() + 8), float((np.abs(r['dz']) @ np.abs(U.T)).max() + 1),
                  max(float(np.abs(v).max()) for v in want.values()), float(np.abs(k['c']).max() * 2 + np.abs(k['c0']).max()))
        assert big < 2 ** 24, big
        assert all(np.array_equal(v, np.rint(v)) for v in want.values())
        for pad in (37, 36):
            got = run_kernels(zx, U, b, h0, c0, dy, 'linear', 'hard_sigmoid', reverse, pad)
            for name, v in want.items():
                assert same_bits(got[name], v.astype(np.float32)), (name, reverse, seq, pad, int((got[name] != v).sum()))
    print(shape, 'largest magnitude', big)


ACT_ERR = {'tanh': lambda y: 1e-7 + EPS * np.abs(y), 'sigmoid': lambda y: 4 * EPS + 0 * y, 'hard_sigmoid': lambda y: 3 * EPS + 0 * y,
           'relu': lambda y: 0 * y, 'linear': lambda y: 0 * y}
ONE_STEP_PAIRS = [('tanh', 'hard_sigmoid'), ('sigmoid', 'sigmoid'), ('relu', 'hard_sigmoid'), ('linear', 'sigmoid')]


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_one_step_meets_the_derived_bound(shape):
    """T = 1 with random h0, c0, against the fp64 evaluation of the same fp32 inputs, u = 2^-24.
      z        (sum_k h U, one fma chain of `units` terms from +0) + zx + b: a term passes at most units + 2 roundings,
                   |z - z64| <= dz := (units + 2) u (sum_k |h U| + |zx| + |b|)                     (Higham (3.4), first order, as tests/test_dot_gpu.py)
      a gate   y = fn(z): |y - y64| <= L dz + e_fn, L <= 1 the Lipschitz constant of every activation (hard_sigmoid 0.2, sigmoid 0.25, the rest 1; 1
               is used), e_fn the function's own error: gn_tanhf 1e-7 absolute (common.h) plus its last rounding u |y|; the sigmoid
               1 / (1 + expf(-x)) at most 4 u (expf within 2 ulp, the sum and the correctly rounded division one each, on a value <= 1);
               hard_sigmoid 3 u (two roundings on values <= 1, the input error of 0.2f counted as one); relu and linear exact
      c        f c0 + i g with three roundings: |c - c64| <= dc := |c0| df + (|g| + dg) di + |i| dg + 3 u (|f c0| + |i g|)
      h        o act(c): |h - h64| <= dh := |act(c)| do + |o| (dc + e_act(c)) + u |h|
    and 1 % on top for the second-order terms.  Every element of gates, c and h is compared."""
    B, _, Cin, u = shape
    rng = np.random.RandomState(7 + B * 1000 + Cin * 10 + u)
    f32 = lambda a: a.astype(np.float32)          # noqa: E731
    zx, U, b = f32(rng.randn(B, 1, 4 * u)), f32(rng.randn(u, 4 * u) / np.sqrt(u)), f32(0.5 * rng.randn(4 * u))
    h0, c0 = f32(rng.rand(B, u) * 2 - 1), f32(rng.randn(B, u))
    dy = f32(rng.randn(B, u))
    for n, (an, rn) in enumerate(ONE_STEP_PAIRS):
        k = R.recurrence(zx, U, b, h0, c0, an, rn, bool(n & 1))
        got = run_kernels(zx, U, b, h0, c0, dy, an, rn, bool(n & 1), pad=37 - (n & 1))
        dz = (u + 2) * EPS * (np.abs(h0.astype(np.float64)) @ np.abs(U.astype(np.float64)) + np.abs(zx[:, 0]) + np.abs(b))
        g64 = k['gates'][:, 0]
        fn = [rn, rn, an, rn]
        dg = np.concatenate([dz[:, q * u:(q + 1) * u] + ACT_ERR[fn[q]](g64[:, q * u:(q + 1) * u]) for q in range(4)], 1)
        i, f, g, o = (np.abs(g64[:, q * u:(q + 1) * u]) for q in range(4))
        di, df, dgg, do = (dg[:, q * u:(q + 1) * u] for q in range(4))
        c64, h64 = k['c'][:, 0], k['h'][:, 0]
        dc = np.abs(c0) * df + (g + dgg) * di + i * dgg + 3 * EPS * (f * np.abs(c0) + i * g)
        tc = R.act(an, c64)
        dh = np.abs(tc) * do + o * (dc + ACT_ERR[an](tc)) + EPS * np.abs(h64)
        for name, ref, bound in (('gates', g64, dg), ('c', c64, dc), ('h', h64, dh)):
            err = np.abs(got[name][:, 0].astype(np.float64) - ref)
            print(shape, an, rn, name, 'worst error / bound %.3g' % (err / (1.01 * bound + 1e-300)).max())
            assert (err <= 1.01 * bound).all(), (an, rn, name, float((err / (1.01 * bound + 1e-300)).max()))
        assert same_bits(got['hprev'][:, 0], h0)


def seq_sum_f32(a, b):
    """sum_r outer(a[r], b[r]) in fp32, row after row: the order class of the weight-gradient products (one chain over B T rows)"""
    acc = np.zeros((a.shape[1], b.shape[1]), np.float32)
    for r in range(a.shape[0]):
        acc += np.outer(a[r], b[r])
    return acc


def restatement_backward(k32, dy):
    """tests/lstm_ref.py in fp32, the sums over B T rows taken row after row"""
    r = R.recurrence_backward(k32, dy.astype(np.float32))
    dz_t = np.ascontiguousarray(R.at_input_time(r['dz'], k32['go_backwards']))
    hp_t = np.ascontiguousarray(R.at_input_time(r['h_prev'], k32['go_backwards']))
    flat = lambda a: a.reshape(-1, a.shape[-1])          # noqa: E731
    return dict(dz=dz_t, dh0=r['dh0'], dc0=r['dc0'], dx=dz_t @ k32['W'].T, dW=seq_sum_f32(flat(k32['x']), flat(dz_t)),
                dU=seq_sum_f32(flat(hp_t), flat(dz_t)), db=flat(dz_t).astype(np.float64).sum(0).astype(np.float32))


def draw_family(family, rng, B, T, Cin, u):
    from gennet_amd import engine
    from gennet_amd.recurrent import orthogonal_blocks
    if family == 'keras':           # keras' own initialisation: Glorot kernel, orthogonal blocks, ones in the f block
        engine.set_init_seed(int(rng.randint(1 << 30)))
        b = np.zeros(4 * u, np.float32)
        b[u:2 * u] = 1.0
        return rng.randn(B, T, Cin).astype(np.float32), engine.glorot_uniform((Cin, 4 * u)), orthogonal_blocks(u), b
    return ((2 * rng.randn(B, T, Cin)).astype(np.float32), (1.5 * (rng.rand(Cin, 4 * u) * 2 - 1)).astype(np.float32),
            (3 / np.sqrt(u) * (rng.rand(u, 4 * u) * 2 - 1)).astype(np.float32), (rng.rand(4 * u) * 2 - 1).astype(np.float32))


def kink_margin(k):
    """the smallest distance of a pre-activation to a point where an activation's derivative jumps: +-2.5 for a hard_sigmoid gate, 0 for relu
    (z_c and c; exact zeros aside: those are structural, c = f 0 + i relu(negative), and fp32 has them too)"""
    u = k['h'].shape[2]
    m = np.inf
    if k['recurrent_activation'] == 'hard_sigmoid':
        z = np.concatenate([k['z'][:, :, :2 * u], k['z'][:, :, 3 * u:]], 2)
        m = min(m, float(np.abs(np.abs(z) - 2.5).min()))
    if k['activation'] == 'relu':
        for v in (k['z'][:, :, 2 * u:3 * u], k['c']):
            nz = np.abs(v[v != 0])
            m = min(m, float(nz.min()) if nz.size else np.inf)
    return m


FAMILY_PAIRS = {'keras': [(a, r) for a in R.ACTIVATIONS for r in R.RECURRENT_ACTIVATIONS],
                'saturating': [('tanh', 'hard_sigmoid'), ('sigmoid', 'hard_sigmoid'), ('tanh', 'sigmoid'), ('tanh', 'hard_sigmoid')]}
MARGIN = 8.0


@pytest.mark.parametrize('family', ['keras', 'saturating'])
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_sequences_against_the_fp64_reference(shape, family):
    """The whole layer arithmetic -- zx = X W (gn_bmm), the recurrence, its backward, dW, dU, dX (gn_bmm) and db -- against tests/lstm_ref.py in
    fp64.  No closed-form bound holds across T steps; the yardstick is the numpy fp32 restatement of the same recurrence, measured against fp64
    on the same inputs: the GPU's largest error per tensor may be at most MARGIN = 8 times max(the restatement's, 2^-24 max|ref|).  The 8 covers
    the device tanh / sigmoid being a few ulp where numpy's are <= 1 ulp, and another summation order.
    Two input families: keras' own initialisation, and a saturating one (x ~ 2 N(0, 1), W ~ 1.5 U(-1, 1), U ~ (3 / sqrt(u)) U(-1, 1),
    b ~ U(-1, 1)) that exercises the zero-derivative branch of hard_sigmoid.  The seed is chosen from the reference alone, on the CPU: the first
    of 0 .. 31 whose smallest distance to a derivative jump (kink_margin) is at least 64 times the restatement's largest |z32 - z64|; one must
    exist.  No element is excluded from any comparison."""
    from gennet_amd import ops
    B, T, Cin, u = shape
    n = SHAPES.index(shape)
    an, rn = FAMILY_PAIRS[family][n % len(FAMILY_PAIRS[family])]
    reverse, seq = bool(n & 1), bool(n & 2)
    for seed in range(32):
        rng = np.random.RandomState(seed * 100 + n)
        x, W, U, b = draw_family(family, rng, B, T, Cin, u)
        dy = rng.randn(*((B, T, u) if seq else (B, u))).astype(np.float32)
        y64, k64 = R.forward(x, W, U, b, None, None, an, rn, seq, reverse)
        y32, k32 = R.forward(x, W, U, b, None, None, an, rn, seq, reverse, dtype=np.float32)
        zerr = float(np.abs(k32['z'] - k64['z']).max())
        if kink_margin(k64) >= 64 * zerr:
            break
    else:
        raise AssertionError('no seed in 0 .. 31 keeps the pre-activations away from the derivative jumps')
    if family == 'saturating' and rn == 'hard_sigmoid' and B * T * u >= 64:
        zg = np.concatenate([k64['z'][:, :, :2 * u], k64['z'][:, :, 3 * u:]], 2)
        assert (np.abs(zg) > 2.5).mean() > 0.05                                       # the family does saturate
    r64 = R.recurrence_backward(k64, dy)
    g64 = R.backward(k64, dy)
    want = dict(reference_at_input_time(k64, r64), dx=g64['dx'], dW=g64['dW'], dU=g64['dU'], db=g64['db'])
    want.pop('hprev')
    r32 = restatement_backward(k32, dy)
    rest = dict(h=k32['h'], gates=R.at_input_time(k32['gates'], reverse), c=R.at_input_time(k32['c'], reverse), **r32)

    t = lambda a: torch.tensor(np.array(a, dtype=np.float32, order='C'), device=dev())          # noqa: E731
    xt, Wt = t(x), t(W)
    zx = ops.bmm(xt.view(1, B * T, Cin), Wt.view(1, Cin, 4 * u)).view(B, T, 4 * u).cpu().numpy()
    got = run_kernels(zx, U, b, None, None, dy, an, rn, reverse, pad=37 - (n & 1))
    dz = t(got['dz']).view(1, B * T, 4 * u)
    got['dW'] = ops.bmm(xt.view(1, B * T, Cin), dz, trans_a=True)[0].cpu().numpy()
    got['dU'] = ops.bmm(t(got['hprev']).view(1, B * T, u), dz, trans_a=True)[0].cpu().numpy()
    got['dx'] = ops.bmm(dz, Wt.view(1, Cin, 4 * u), trans_b=True).view(B, T, Cin).cpu().numpy()
    got['db'] = ops.bias_grad(dz.view(B * T, 4 * u)).cpu().numpy()
    worst = {}
    for name, ref in want.items():
        yard = max(float(np.abs(rest[name].astype(np.float64) - ref).max()), EPS * float(np.abs(ref).max()))
        err = float(np.abs(got[name].astype(np.float64) - ref).max())
        worst[name] = err / yard if yard else (0.0 if err == 0 else np.inf)
    print(shape, family, an, rn, 'seed', seed, 'error / yardstick:', ' '.join('%s %.2f' % kv for kv in sorted(worst.items())))
    assert all(v <= MARGIN for v in worst.values()), worst


@pytest.mark.parametrize('u', [64, 100])
def test_a_sample_does_not_depend_on_the_batch_or_the_launch(u):
    """Rows 0 and 32 of a B = 33 run (the first row of the first tile, the only row of the third), forward and backward, have the bits of the two
    B = 1 runs of those samples; two identical launches return the same bits.  u = 64: U in LDS; u = 100: streamed."""
    B, T = 33, 5
    rng = np.random.RandomState(u)
    f32 = lambda a: a.astype(np.float32)          # noqa: E731
    zx, U, b = f32(rng.randn(B, T, 4 * u)), f32(rng.randn(u, 4 * u) / np.sqrt(u)), f32(0.5 * rng.randn(4 * u))
    h0, c0, dy = f32(0.5 * rng.randn(B, u)), f32(0.5 * rng.randn(B, u)), f32(rng.randn(B, T, u))
    for reverse in (False, True):
        whole = run_kernels(zx, U, b, h0, c0, dy, 'tanh', 'hard_sigmoid', reverse)
        again = run_kernels(zx, U, b, h0, c0, dy, 'tanh', 'hard_sigmoid', reverse)
        assert all(same_bits(whole[k], again[k]) for k in whole)
        assert np.abs(whole['dz']).max() > 0
        for row in (0, 32):
            one = run_kernels(zx[row:row + 1], U, b, h0[row:row + 1], c0[row:row + 1], dy[row:row + 1], 'tanh', 'hard_sigmoid', reverse, pad=36)
            for k in whole:
                assert same_bits(one[k][0], whole[k][row]), (k, row, reverse)


def test_the_inference_phase_stores_nothing():
    rng = np.random.RandomState(5)
    zx, U, b = rng.randn(3, 4, 20).astype(np.float32), rng.randn(5, 20).astype(np.float32), np.zeros(20, np.float32)
    a = run_kernels(zx, U, b, None, None, None, 'tanh', 'sigmoid', False, training=False)
    assert same_bits(a['h'], run_kernels(zx, U, b, None, None, rng.randn(3, 5).astype(np.float32), 'tanh', 'sigmoid', False)['h'])


def test_bad_arguments_are_errors_and_launch_nothing():
    from gennet_amd import _lib, ops
    B, T, u = 2, 3, 5
    one = lambda *s: np.ones(s, np.float32)          # noqa: E731
    zx, U, b, st, dy, gates, c = (Guarded(s, one(*s), 36) for s in ((B, T, 4 * u), (u, 4 * u), (4 * u,), (B, u), (B, T, u), (B, T, 4 * u), (B, T, u)))
    outs = [Guarded(s, None, 36) for s in ((B, T, u), (B, T, 4 * u), (B, T, u), (B, T, u), (B, u), (B, u))]
    h, og, oc, ohp, dh0, dc0 = outs
    s = torch.cuda.current_stream().cuda_stream
    ws = ops.workspace(max(_lib.size('gn_lstm_fwd_workspace', 512), _lib.size('gn_lstm_bwd_workspace', 512)), dev())
    tanh, hard = ops.LSTM_ACT['tanh'], ops.LSTM_ACT['hard_sigmoid']
    good = dict(zx=zx.t.data_ptr(), U=U.t.data_ptr(), b=b.t.data_ptr(), h0=st.t.data_ptr(), c0=st.t.data_ptr(), h=h.t.data_ptr(), gates=og.t.data_ptr(),
                c=oc.t.data_ptr(), hprev=ohp.t.data_ptr(), ws=ws.data_ptr(), ws_bytes=ws.numel(), B=B, T=T, u=u, act=tanh, ract=hard, training=1,
                dy=dy.t.data_ptr(), sgates=gates.t.data_ptr(), sc=c.t.data_ptr(), dz=og.t.data_ptr(), dh0=dh0.t.data_ptr(), dc0=dc0.t.data_ptr())

    def fwd(**kw):
        g = dict(good, **kw)
        _lib.call('gn_lstm_fwd', g['zx'], g['U'], g['b'], g['h0'], g['c0'], g['h'], g['gates'], g['c'], g['hprev'], g['ws'], g['ws_bytes'], g['B'], g['T'],
                  g['u'], g['act'], g['ract'], 0, g['training'], s)

    def bwd(**kw):
        g = dict(good, **kw)
        _lib.call('gn_lstm_bwd', g['dy'], g['sgates'], g['sc'], g['c0'], g['U'], g['dz'], g['dh0'], g['dc0'], g['ws'], g['ws_bytes'], g['B'], g['T'], g['u'],
                  g['act'], g['ract'], 1, 1, s)

    def refused(text, fn, code=None):
        with pytest.raises(_lib.GennetHipError) as e:
            fn()
        assert '(%d)' % (_lib.GN_EINVAL if code is None else code) in str(e.value) and text in str(e.value), str(e.value)
        assert text in _lib.lib().gn_last_error().decode()
        torch.cuda.synchronize()
        assert all(o.untouched() for o in outs)

    for k in ('zx', 'U', 'b', 'h', 'ws', 'gates', 'c', 'hprev'):
        refused('null pointer', lambda: fwd(**{k: None}))
    for k in ('dy', 'sgates', 'sc', 'U', 'dz', 'ws'):
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
        refused('workspace too small', lambda: call(ws_bytes=_lib.size('gn_lstm_fwd_workspace' if call is fwd else 'gn_lstm_bwd_workspace', u) - 1),
                _lib.GN_EWORKSPACE)
        call(B=0)                                              # nothing to do is not an error, and launches nothing (the pointers are not looked at)
    fwd(B=0, zx=None, h=None, ws=None)
    assert _lib.size('gn_lstm_fwd_workspace', 513) == 0 and _lib.size('gn_lstm_bwd_workspace', 0) == 0
    torch.cuda.synchronize()
    assert all(o.untouched() for o in outs)
    fwd(gates=None, c=None, hprev=None, training=0, h0=None, c0=None)          # the inference phase takes no storage, and no initial state
    bwd(dh0=None, dc0=None, c0=None)
    torch.cuda.synchronize()
    h.check('lstm_fwd')
    og.check('lstm_bwd dz')
    assert oc.untouched() and ohp.untouched() and dh0.untouched() and dc0.untouched()
    with pytest.raises(ValueError, match='recurrent kernel'):
        ops.lstm_fwd(zx.t, U.t[:, :8].contiguous(), b.t)


# ---------------------------------------------------------------------------------------------------------------------
# section 2: models against torch fp64 autograd (the logic and bounds of tests/test_merge_gpu.py's train_and_compare, over three steps)
# ---------------------------------------------------------------------------------------------------------------------
LR = 0.05


def rel(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-30)


def seed_biases(model, rng):
    for l in model.layers:
        ws = l.get_weights()
        if ws:
            l.set_weights(ws[:-1] + [(ws[-1] + 0.1 * rng.randn(*ws[-1].shape)).astype(np.float32)])


def torch_params(layers):
    return dict((l.name, [torch.tensor(w.astype(np.float64), requires_grad=True) for w in l.get_weights()]) for l in layers if l.weights)


def penalty_of(layers, P):
    """sum over the regularized weights of l1 sum|w| + l2 sum w^2, on the torch parameters"""
    total = 0.0
    for l in layers:
        for p, w in zip(l.weights, P[l.name]):
            if p.regularizer is not None:
                total = total + p.regularizer.l1 * w.abs().sum() + p.regularizer.l2 * (w * w).sum()
    return total


def train_and_compare(model, ref_forward, xs, t, loss='mean_squared_error', steps=3, what=''):
    """predict, then `steps` SGD train_on_batch steps, against torch fp64 stepping the same way; -> the penalties of the steps"""
    from gennet_amd.engine import SGD
    model.compile(optimizer=SGD(lr=LR), loss=loss)
    layers = [l for l in model.layers if l.weights]
    P = torch_params(layers)
    xt = [torch.tensor(x.astype(np.float64)) for x in xs]
    tt = torch.tensor(t.astype(np.float64))
    feed = xs if len(xs) > 1 else xs[0]
    y = model.predict(feed, batch_size=len(t))
    with torch.no_grad():
        y_ref = ref_forward(P, *xt).numpy()
    print(what, 'predict err %.3g' % rel(y, y_ref))
    assert rel(y, y_ref) < 1e-5
    losses, penalties = [], []
    for step in range(steps):
        for ts in P.values():
            for v in ts:
                v.grad = None
        out = ref_forward(P, *xt)
        pen = penalty_of(layers, P)
        loss_ref = (((out - tt) ** 2).mean() if loss == 'mean_squared_error' else F.binary_cross_entropy(out, tt)) + pen
        loss_ref.backward()
        res = model.train_on_batch(feed, t)
        res = res if isinstance(res, (list, tuple)) else [res]
        pen = float(pen.detach()) if torch.is_tensor(pen) else float(pen)
        print(what, 'step', step, 'loss', res[0], float(loss_ref.detach()), 'penalty', pen)
        assert abs(res[0] - float(loss_ref.detach())) <= 1e-6 * abs(float(loss_ref.detach()))
        losses.append(float(loss_ref.detach()))
        penalties.append(pen)
        g_floor = 1e-3 * max(float(v.grad.abs().max()) for ts in P.values() for v in ts)
        for l in layers:
            for p, ref in zip(l.params, P[l.name]):
                g_ref = ref.grad.numpy()
                gerr = np.abs(p.grad.detach().cpu().numpy().reshape(g_ref.shape) - g_ref).max() / max(np.abs(g_ref).max(), g_floor)
                with torch.no_grad():
                    ref -= LR * ref.grad
                w_ref = ref.detach().numpy()
                werr = np.abs(p.numpy().astype(np.float64) - w_ref).max() / max(np.abs(w_ref).max(), 1e-3)
                print(what, step, l.name, p.name, 'grad err %.3g weight err %.3g' % (gerr, werr))
                assert gerr < 1e-4 and werr < 1e-4, (step, l.name, p.name, gerr, werr)
    assert len(set(losses)) == steps                                       # the steps differ
    return penalties


def lstm_ref(P, layer, x):
    W, U, b = P[layer.name]
    return R.torch_forward(x, W, U, b, None, None, layer.activation, layer.recurrent_activation, layer.return_sequences, layer.go_backwards)


def conv_lstm_model():
    """Conv1D(8, 5, strides=2) -> LSTM(12) -> Dense(2); the LSTM carries the three weight regularizers"""
    from gennet_amd import layers as Ly, regularizers
    from gennet_amd.engine import Sequential
    conv = Ly.Conv1D(8, 5, strides=2, input_shape=(21, 4))
    lstm = Ly.LSTM(12, kernel_regularizer=regularizers.l2(0.01), recurrent_regularizer=regularizers.l1(0.002), bias_regularizer=regularizers.l1_l2(0.003, 0.004))
    head = Ly.Dense(2)
    model = Sequential()
    for l in (conv, lstm, head):
        model.add(l)

    def ref(P, x):
        w, b = P[conv.name]
        c = F.conv1d(x.permute(0, 2, 1), w.permute(2, 1, 0), stride=2).permute(0, 2, 1) + b
        return lstm_ref(P, lstm, c) @ P[head.name][0] + P[head.name][1]
    return model, ref


def test_conv_lstm_dense_trains_as_torch_fp64_and_its_penalty_shows():
    model, ref = conv_lstm_model()
    rng = np.random.RandomState(31)
    seed_biases(model, rng)
    assert model.output_shape == (None, 2) and [n.out_shape for n in model.nodes] == [(9, 8), (12,), (2,)]
    pens = train_and_compare(model, ref, [rng.randn(5, 21, 4).astype(np.float32)], rng.randn(5, 2).astype(np.float32), what='conv-lstm')
    assert min(pens) > 0.05                                                 # entry 0 was held against loss + penalty: the penalty is no rounding matter


def test_stacked_lstm_with_a_reversed_sigmoid_gated_layer_trains_as_torch_fp64():
    from gennet_amd import layers as Ly
    from gennet_amd.engine import Sequential
    first = Ly.LSTM(8, return_sequences=True, input_shape=(7, 3))
    second = Ly.LSTM(5, go_backwards=True, recurrent_activation='sigmoid')
    head = Ly.Dense(1, activation='sigmoid')
    model = Sequential()
    for l in (first, second, head):
        model.add(l)
    rng = np.random.RandomState(32)
    seed_biases(model, rng)

    def ref(P, x):
        return torch.sigmoid(lstm_ref(P, second, lstm_ref(P, first, x)) @ P[head.name][0] + P[head.name][1])
    train_and_compare(model, ref, [rng.randn(6, 7, 3).astype(np.float32)], (rng.rand(6, 1) < 0.5).astype(np.float32), loss='binary_crossentropy',
                      what='stacked')


def test_lstm_feeding_self_attention_trains_as_torch_fp64():
    """LSTM(6, return_sequences=True) as queries, keys and values of the Dot / Softmax attention of DESIGN 8n: three edges leave the layer"""
    from gennet_amd import layers as Ly
    from gennet_amd.engine import Input, Model
    x = Input((9, 4))
    lstm, head = Ly.LSTM(6, return_sequences=True), Ly.Dense(1)
    h = lstm(x)
    ctx = Ly.Dot((2, 1))([Ly.Softmax(-1)(Ly.Dot((2, 2))([h, h])), h])
    model = Model(inputs=x, outputs=head(Ly.GlobalAveragePooling1D()(ctx)))
    rng = np.random.RandomState(33)
    seed_biases(model, rng)

    def ref(P, x):
        h = lstm_ref(P, lstm, x)
        a = torch.softmax(torch.matmul(h, h.transpose(1, 2)), dim=-1)
        return torch.matmul(a, h).mean(1) @ P[head.name][0] + P[head.name][1]
    train_and_compare(model, ref, [rng.randn(4, 9, 4).astype(np.float32)], rng.randn(4, 1).astype(np.float32), what='lstm-attention')


def test_weight_gradients_summed_in_row_parts_train_as_torch_fp64():
    """B T = 16 x 64 = 1024 rows: dW and dU are formed in 4 row parts as one batched product and summed by the fixed-order column reduction
    (recurrent.row_splits / rows_product); the models above have too few rows and take the single product"""
    from gennet_amd import layers as Ly
    from gennet_amd.engine import Sequential
    from gennet_amd.recurrent import row_splits
    assert row_splits(16 * 64, 3 * 20) == 4 and row_splits(16 * 64, 5 * 20) == 4 and row_splits(5 * 9, 8 * 48) == 1
    lstm, head = Ly.LSTM(5, input_shape=(64, 3)), Ly.Dense(1)
    model = Sequential()
    model.add(lstm)
    model.add(head)
    rng = np.random.RandomState(37)
    seed_biases(model, rng)

    def ref(P, x):
        return lstm_ref(P, lstm, x) @ P[head.name][0] + P[head.name][1]
    train_and_compare(model, ref, [rng.randn(16, 64, 3).astype(np.float32)], rng.randn(16, 1).astype(np.float32), what='row parts')


def test_save_and_load_round_trip(tmp_path):
    from gennet_amd.engine import SGD, load_model
    model, _ = conv_lstm_model()
    rng = np.random.RandomState(34)
    seed_biases(model, rng)
    x, t = rng.randn(5, 21, 4).astype(np.float32), rng.randn(5, 2).astype(np.float32)
    model.compile(optimizer=SGD(lr=LR), loss='mean_squared_error')
    model.train_on_batch(x, t)
    path = os.path.join(str(tmp_path), 'conv_lstm.h5')
    model.save(path)
    again = load_model(path)
    assert [type(n.layer).__name__ for n in again.nodes] == ['Conv1D', 'LSTM', 'Dense']
    lstm = again.layers[1]
    assert [p.name for p in lstm.weights] == ['%s/%s' % (lstm.name, n) for n in ('kernel', 'recurrent_kernel', 'bias')]
    assert lstm.get_config() == model.layers[1].get_config() and lstm.recurrent_kernel.regularizer.l1 == np.float32(0.002)
    assert np.array_equal(model.predict(x), again.predict(x))
    a, b = model.train_on_batch(x, t), again.train_on_batch(x, t)
    assert a == b and all(np.array_equal(u, v) for u, v in zip(model.get_weights(), again.get_weights()))


def test_predict_allocates_no_tape():
    from gennet_amd import engine
    model, _ = conv_lstm_model()
    x = np.random.RandomState(35).randn(3, 21, 4).astype(np.float32)
    ctx = engine.RunContext(False)
    out = model._forward(model._prep_inputs(x), ctx)
    assert tuple(out[0].shape) == (3, 2) and model.nodes[1].index not in ctx.tape
    ctx = engine.RunContext(True)
    model._forward(model._prep_inputs(x), ctx)
    kept = ctx.tape[model.nodes[1].index]
    assert [tuple(v.shape) for v in kept] == [(3, 9, 8), (3, 9, 12), (3, 9, 48), (3, 9, 12)]          # x, hprev, the gates, c


def test_a_captured_step_replays_bit_identically():
    """the Conv1D -> LSTM -> Dense model as a hipGraph (engine.StepGraph): eager step, capture, three replays against four eager steps of a twin"""
    from gennet_amd import engine
    from gennet_amd.engine import SGD, to_device
    rng = np.random.RandomState(36)
    x, t = to_device(rng.randn(5, 21, 4).astype(np.float32)), to_device(rng.randn(5, 2).astype(np.float32))
    eager, _ = conv_lstm_model()
    seed_biases(eager, rng)
    graphed, _ = conv_lstm_model()
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
