"""GPU parity of the pooling layers (csrc/pooling.hip through ops.pool2d_*, ops.global_pool_*, and the eight layers of gennet_amd.layers)
against the numpy definition tests/pool_ref.py (itself checked against torch autograd in tests/test_pooling_cpu.py).

Windowed kernels.  A thread owns one unit (4 floats when C % 4 == 0 and every pointer is 16-byte aligned, else 1 float) of y (forward) or dx
(backward); the grid is capped at 2048 blocks of 256 (524288 units) and a thread past it steps its (b, h, w, c) position digit by digit.
Every case runs both modes, forward and backward, in views that start 148 bytes into a buffer (not 16-byte aligned: the scalar kernels) and,
where C % 4 == 0, also 144 bytes in (the float4 kernels).  Which case crosses which seam:
    C = 1, 3, 6 scalar only; C = 4, 260 both paths            W = 1: the 1-D layers; W > 1: windows over both axes
    (3,9,1,3,(3,1),(2,1),'same')     overlap (a cell under two windows), total pad 2
    (3,10,1,4,(3,1),(2,1),'same')    total pad 1: the odd cell at the end
    (3,11,1,6,(2,1),(3,1),'valid')   gaps: every third row under no window, zero gradient
    (3,9,2,4,(2,1),(2,1),'valid')    a dropped last row; the case of gn_maxpool_h2_*: equal to it bit for bit (also at C = 3)
    (3,2,1,1,(3,1),(3,1),'same')     H < pool: one clipped window
    (3,5,4,4,(5,4),(5,4),'valid')    the pool is the whole extent
    (3,7,6,260,(3,2),(2,1),'same')   65 float4 per cell, pads on both axes, overlap along both
    (3,44,64,260,(3,3),(1,1),'same') 549120 float4 units of y and of dx: 24832 threads take a second trip, and the grid's stride
                                     (63 units, 1 column, 38 rows, 2 samples) carries in every digit
    (3,12,15,1030,(2,2),(1,1),'same') 556200 scalar units: the same seam of the scalar kernels
Bounds (pool_ref in fp64 on the fp32 inputs): the maximum and, without overlap, its gradient are comparisons and copies: bit-identical to the
reference cast to fp32; its gradient with overlap k 2^-24 max|dy|, k the covering windows; the average ph pw 2^-24 max|x| (max|x| taken per
sample, so that the sample of huge values does not widen the bound of the others), its gradient k 2^-24 max|dy|.
Inputs: zeros from a 0.4-rate mask and an all-zero sample (exact ties), the first window of sample 0 all -inf, the last sample near -3e38
(the maximum) or -3e38 / (ph pw) (the average, whose fp32 window sum the issue prescribes and which must stay finite to be comparable).

Global kernels.  Block = (column block of min(C / VEC, 256) units, chunk of P, sample); 256 / units row lanes, two rows per lane and trip.
    (2,1,1) P = 1    (3,5,4) one float4 column, 256 row lanes, 5 rows    (2,7,3) scalar    (1,33,260) 65 units x 3 row lanes, 61 lanes idle
    (4,1000,6) and (2,3000,260): few (sample, column) blocks, so P is split into 6 and 250 chunks and global_final_kernel combines the
    partials; asserted through the workspace size    (1,9,1028) and (1,5,258): a second column block with one unit in it
Model level: torch fp64 autograd on the CPU, with the bounds of tests/test_bn_axis_gpu.py's model tests."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pool_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5
EPS = 2.0 ** -24


def dev():
    return torch.device('cuda:0')


class Guarded(object):
    """A contiguous view `pad` floats into a larger flat buffer: inputs surrounded by NaN, outputs inside a sentinel-filled buffer.
    pad = 37: the view starts 148 bytes in (no 16-byte boundary); pad = 36: 144 bytes (aligned)."""

    def __init__(self, shape, value=None, pad=37):
        self.n, self.pad = int(np.prod(shape)), pad
        self.buf = torch.full((self.n + 2 * pad,), float('nan') if value is not None else SENTINEL, dtype=torch.float32, device=dev())
        self.t = self.buf[pad:pad + self.n].view(shape)
        if value is not None:
            self.t.copy_(torch.tensor(np.asarray(value, np.float32), device=dev()))
        assert self.t.is_contiguous() and self.t.data_ptr() == self.buf.data_ptr() + 4 * pad and (self.t.data_ptr() % 16 == 0) == (pad % 4 == 0)

    def refill(self):
        self.buf.fill_(SENTINEL)

    def check(self, what):
        """the surroundings untouched, every element of the view written"""
        edges = torch.cat([self.buf[:self.pad], self.buf[self.pad + self.n:]])
        assert bool((edges == SENTINEL).all()), '%s: wrote outside its output' % what
        assert not bool((self.t == SENTINEL).any()), '%s: output elements left unwritten' % what
        assert not bool(torch.isnan(self.t).any()), '%s: NaN (an element outside an input was read)' % what
        return self.t.cpu().numpy()


def twice(run, out, what):
    """run() into `out` twice: the checked result, bit-identical on the second run"""
    run()
    a = out.check(what).copy()
    out.refill()
    run()
    assert np.array_equal(out.check(what + ' (second run)'), a), '%s: two runs differ' % what
    return a


# B, H, W, C, pool, strides, padding   (the module docstring says what each is for)
CASES = [(3, 9, 1, 3, (3, 1), (2, 1), 'same'),
         (3, 10, 1, 4, (3, 1), (2, 1), 'same'),
         (3, 11, 1, 6, (2, 1), (3, 1), 'valid'),
         (3, 9, 2, 4, (2, 1), (2, 1), 'valid'),
         (3, 9, 2, 3, (2, 1), (2, 1), 'valid'),
         (3, 2, 1, 1, (3, 1), (3, 1), 'same'),
         (3, 5, 4, 4, (5, 4), (5, 4), 'valid'),
         (3, 7, 6, 260, (3, 2), (2, 1), 'same'),
         (3, 8, 1, 1, (2, 1), (2, 1), 'valid'),
         (3, 44, 64, 260, (3, 3), (1, 1), 'same'),
         (3, 12, 15, 1030, (2, 2), (1, 1), 'same')]


def windowed_input(rng, shape, pool, strides, padding, mode):
    B, H, W, C = shape
    x = rng.randn(*shape).astype(np.float32) * (rng.rand(*shape) >= 0.4)
    x[0] = 0.0
    pt, pl = R.pool_geometry(H, pool[0], strides[0], padding)[1], R.pool_geometry(W, pool[1], strides[1], padding)[1]
    x[0, :max(pool[0] - pt, 1), :max(pool[1] - pl, 1), :] = -np.inf          # the in-bounds cells of window (0, 0)
    big = 3e38 if mode == 'max' else 3e38 / (pool[0] * pool[1])
    x[B - 1] = -big * (1.0 - 0.05 * rng.rand(H, W, C))
    return x.astype(np.float32)


@pytest.mark.parametrize('mode', ['max', 'avg'])
@pytest.mark.parametrize('case', CASES, ids=['-'.join(str(v) for v in c).replace(' ', '') for c in CASES])
def test_windowed_passes_against_the_reference(case, mode):
    from gennet_amd import ops
    B, H, W, C, pool, strides, padding = case
    rng = np.random.RandomState(H * 1000 + W * 10 + C)
    x = windowed_input(rng, (B, H, W, C), pool, strides, padding, mode)
    y_ref = R.pool2d_fwd(mode, x, pool, strides, padding)
    dy = rng.randn(*y_ref.shape).astype(np.float32) * (rng.rand(*y_ref.shape) >= 0.2)
    dx_ref = R.pool2d_bwd(mode, dy, x, pool, strides, padding)
    k = R.covering_windows(x.shape, pool, strides, padding)
    gaps = padding == 'valid' and (strides[0] > pool[0] or (H - pool[0]) % strides[0])
    if gaps:
        assert (dx_ref[1].reshape(H, -1) == 0).all(1).any()                  # a row under no window
    finite = np.isfinite(y_ref)
    x_max = np.maximum(np.where(np.isfinite(x), np.abs(x), 0.0).reshape(B, -1).max(1), 1e-30).reshape(B, 1, 1, 1).astype(np.float64)
    for pad in ((37, 36) if C % 4 == 0 else (37,)):
        what = '%s %r pad %d' % (mode, case, pad)
        xg, dyg = Guarded(x.shape, x, pad), Guarded(dy.shape, dy, pad)
        yg, dxg = Guarded(y_ref.shape, None, pad), Guarded(x.shape, None, pad)
        y = twice(lambda: ops.pool2d_fwd(mode, xg.t, pool, strides, padding, out=yg.t), yg, what + ' forward')
        dx = twice(lambda: ops.pool2d_bwd(mode, dyg.t, xg.t if mode == 'max' else None, x.shape, pool, strides, padding, out=dxg.t), dxg, what + ' backward')
        assert np.array_equal(np.isfinite(y), finite) and np.array_equal(y[~finite], y_ref[~finite].astype(np.float32))
        if mode == 'max':
            assert np.array_equal(y, y_ref.astype(np.float32)), what
            err, bound = np.abs(dx - dx_ref).max(), (0.0 if k == 1 else k * EPS * np.abs(dy).max())
        else:
            e = np.where(finite, np.abs(np.where(finite, y, 0.0) - np.where(finite, y_ref, 0.0)), 0.0)
            rel = (e / (pool[0] * pool[1] * EPS * x_max)).max()
            print('%s: forward error / bound %.3g' % (what, rel))
            assert rel <= 1.0, (what, rel)
            err, bound = np.abs(dx - dx_ref).max(), k * EPS * np.abs(dy).max()
        print('%s: backward max err %.3g, bound %.3g (%d covering windows)' % (what, err, bound, k))
        assert err <= bound, (what, err, bound)
        if mode == 'max' and pool == (2, 1) and strides == (2, 1) and padding == 'valid':
            assert torch.equal(yg.t, ops.maxpool_h2_fwd(xg.t)) and torch.equal(dxg.t, ops.maxpool_h2_bwd(dyg.t, xg.t)), what


GLOBAL_SHAPES = [(2, 1, 1), (3, 5, 4), (2, 7, 3), (1, 33, 260), (4, 1000, 6), (2, 3000, 260), (1, 9, 1028), (1, 5, 258)]
WORKSPACE = {(3, 5, 4): 48, (4, 1000, 6): 96 + 6 * 24 * 8, (2, 3000, 260): 2080 + 250 * 520 * 8}      # dy / n_ties per (b, c), 16-byte padded, + the chunks' partials


@pytest.mark.parametrize('B,P,C', GLOBAL_SHAPES)
def test_global_passes_against_the_reference(B, P, C):
    from gennet_amd import _lib, ops
    if (B, P, C) in WORKSPACE:
        assert _lib.size('gn_global_pool_workspace', B, P, C) == WORKSPACE[(B, P, C)]
    rng = np.random.RandomState(B * 10000 + P * 10 + C)
    x = rng.randn(B, P, C).astype(np.float32) * 1.5 + 0.7
    # ties of the maximum per (b, c): c % 3 == 0 one, == 1 two (where P >= 2), == 2 all P positions equal
    top = x.max(1) + 1.0
    for c in range(C):
        if c % 3 == 1 and P >= 2:
            x[:, [0, P - 1], c] = top[:, None, c]
        elif c % 3 == 2:
            x[:, :, c] = top[:, None, c]
    n_ties = (x == x.max(1, keepdims=True)).sum(1)
    assert set(np.unique(n_ties)) <= {1, 2, P} and (C < 3 or P < 3 or len(np.unique(n_ties)) == 3)
    dy = rng.randn(B, C).astype(np.float32)
    for pad in ((37, 36) if C % 4 == 0 else (37,)):
        xg, dyg = Guarded(x.shape, x, pad), Guarded(dy.shape, dy, pad)
        for mode in ('avg', 'max'):
            what = 'global %s (%d,%d,%d) pad %d' % (mode, B, P, C, pad)
            yg, dxg = Guarded((B, C), None, pad), Guarded(x.shape, None, pad)
            y = twice(lambda: ops.global_pool_fwd(mode, xg.t, out=yg.t), yg, what + ' forward')
            y_ref = R.global_fwd(mode, x)
            dx_ref = R.global_bwd(mode, dy, x)
            if mode == 'avg':
                err = np.abs(y - y_ref).max()
                print('%s: forward err %.3g, bound %.3g' % (what, err, 2 * EPS * np.abs(x).max()))
                assert err <= 2 * EPS * np.abs(x).max(), what
                dx = twice(lambda: ops.global_pool_bwd(mode, dyg.t, None, None, x.shape, out=dxg.t), dxg, what + ' backward')
            else:
                assert np.array_equal(y, y_ref.astype(np.float32)), what
                dx = twice(lambda: ops.global_pool_bwd(mode, dyg.t, xg.t, yg.t, x.shape, out=dxg.t), dxg, what + ' backward')
                assert np.array_equal(dx != 0, (dx_ref != 0))
            rel = (np.abs(dx - dx_ref) / np.maximum(np.abs(dx_ref), 1e-30)).max()
            print('%s: backward error %.3g roundings' % (what, rel / EPS))
            assert rel <= EPS, (what, rel)                                   # one rounding of dy / P or dy / n_ties


def raises_and_writes_nothing(out, call):
    from gennet_amd import _lib
    with pytest.raises(_lib.GennetHipError):
        call()
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()), 'a refused call wrote its output'


def test_refusals_are_errors_and_launch_nothing():
    from gennet_amd import _lib, ops
    s = torch.cuda.current_stream().cuda_stream
    B, H, W, C = 2, 6, 4, 4
    x = torch.ones((B, H, W, C), device=dev()); xp = x.data_ptr()
    y = torch.full((B, 3, 2, C), SENTINEL, device=dev()); yp = y.data_ptr()
    dx = torch.full((B, H, W, C), SENTINEL, device=dev()); dxp = dx.data_ptr()
    ok = dict(mode=0, B=B, H=H, W=W, C=C, ph=2, pw=2, sh=2, sw=2, pt=0, pl=0, Ho=3, Wo=2)

    def fwd(xq=xp, yq=yp, **kw):
        a = dict(ok, **kw)
        _lib.call('gn_pool2d_fwd', a['mode'], xq, yq, a['B'], a['H'], a['W'], a['C'], a['ph'], a['pw'], a['sh'], a['sw'], a['pt'], a['pl'], a['Ho'], a['Wo'], s)

    def bwd(dyq=yp, xq=xp, dxq=dxp, **kw):
        a = dict(ok, **kw)
        _lib.call('gn_pool2d_bwd', a['mode'], dyq, xq, dxq, a['B'], a['H'], a['W'], a['C'], a['ph'], a['pw'], a['sh'], a['sw'], a['pt'], a['pl'], a['Ho'], a['Wo'], s)

    bad = [dict(mode=2), dict(mode=-1), dict(C=0), dict(H=0), dict(W=0), dict(ph=0), dict(pw=-1), dict(sh=0), dict(sw=0), dict(B=-1),
           dict(pt=2), dict(pl=2), dict(pt=-1), dict(Ho=0), dict(Wo=0),
           dict(Ho=4),                 # window 3 starts at row 6 of 6: no in-bounds cell
           dict(Wo=3)]
    for kw in bad:
        raises_and_writes_nothing(y, lambda: fwd(**kw))
        raises_and_writes_nothing(dx, lambda: bwd(**kw))
    raises_and_writes_nothing(y, lambda: fwd(xq=None))
    raises_and_writes_nothing(y, lambda: fwd(yq=None))
    raises_and_writes_nothing(dx, lambda: bwd(dyq=None))
    raises_and_writes_nothing(dx, lambda: bwd(dxq=None))
    raises_and_writes_nothing(dx, lambda: bwd(xq=None))                     # the maximum needs x ...
    fwd(B=0); bwd(B=0)                                                     # B = 0: GN_OK, nothing launched
    torch.cuda.synchronize()
    assert bool((y == SENTINEL).all()) and bool((dx == SENTINEL).all())
    y.fill_(2.0)
    bwd(mode=1, xq=None)                                                   # ... the average does not
    assert torch.equal(dx, torch.full_like(dx, 0.5))
    fwd()
    assert torch.equal(y, torch.ones_like(y))
    # global
    P = 5
    x3 = torch.ones((B, P, C), device=dev()); yg = torch.full((B, C), SENTINEL, device=dev()); dx3 = torch.full((B, P, C), SENTINEL, device=dev())
    nb = _lib.size('gn_global_pool_workspace', B, P, C)
    assert nb == 32 and _lib.size('gn_global_pool_workspace', B, 0, C) == 0
    ws = torch.zeros(nb, dtype=torch.uint8, device=dev())

    def gfwd(mode=0, xq=x3.data_ptr(), yq=yg.data_ptr(), wq=ws.data_ptr(), n=nb, B=B, P=P, C=C):
        _lib.call('gn_global_pool_fwd', mode, xq, yq, wq, n, B, P, C, s)

    def gbwd(mode=0, dyq=yg.data_ptr(), xq=x3.data_ptr(), yq=yg.data_ptr(), dxq=dx3.data_ptr(), wq=ws.data_ptr(), n=nb, B=B, P=P, C=C):
        _lib.call('gn_global_pool_bwd', mode, dyq, xq, yq, dxq, wq, n, B, P, C, s)

    for kw in (dict(mode=2), dict(P=0), dict(C=0), dict(B=-1), dict(wq=None), dict(n=nb - 1), dict(wq=ws.data_ptr() + 4, n=nb)):
        raises_and_writes_nothing(yg, lambda: gfwd(**kw))
        raises_and_writes_nothing(dx3, lambda: gbwd(**kw))
    raises_and_writes_nothing(yg, lambda: gfwd(xq=None))
    raises_and_writes_nothing(yg, lambda: gfwd(yq=None))
    raises_and_writes_nothing(dx3, lambda: gbwd(dxq=None))
    raises_and_writes_nothing(dx3, lambda: gbwd(dyq=None))
    raises_and_writes_nothing(dx3, lambda: gbwd(xq=None))
    raises_and_writes_nothing(dx3, lambda: gbwd(yq=None))
    gfwd(B=0); gbwd(B=0)
    torch.cuda.synchronize()
    assert bool((yg == SENTINEL).all()) and bool((dx3 == SENTINEL).all()) and int(ws.sum()) == 0
    gfwd(mode=1)
    assert torch.equal(yg, torch.ones_like(yg))
    gbwd(mode=1, xq=None, yq=None)
    assert torch.equal(dx3, torch.full_like(dx3, float(np.float32(1.0) / np.float32(5.0))))
    assert ops.POOL_MODES == {'max': 0, 'avg': 1}


# ---- model level ----------------------------------------------------------------------------------------------------------------------
def _disc(pool):
    return ((40,), [('reshape', (-1, 1)), ('conv', 8, 8, 'tanh'), ('leaky', 0.2), ('bn', 1), ('conv', 16, 8, 'tanh'), ('leaky', 0.2), (pool,),
                    ('dense', 2, 'sigmoid')])


NETS = {
    'a_sibling_discriminator': _disc('gap1d'),
    'b_windowed_1d': ((40,), [('reshape', (-1, 1)), ('conv', 8, 5, 'tanh'), ('pool1d', 'max', 2, None, 'valid'), ('conv', 6, 3, 'tanh'),
                              ('pool1d', 'avg', 3, 2, 'same'), ('flatten',), ('dense', 2, None)]),
    'c_transpose_gap2d': ((40,), [('reshape', (-1, 1, 1)), ('convT', 8, 4, 'relu'), ('bn', -1), ('gap2d',), ('dense', 3, None)]),
    'd_conv2d_maxpool2d': ((40,), [('reshape', (20, 2, 1)), ('conv2d', 8, 5, 'tanh'), ('leaky', 0.2), ('pool2d', 'max', (2, 2), None, 'valid'), ('flatten',),
                                   ('dense', 3, None)]),
    'e_global_max': _disc('gmp1d'),
}


def _build(spec, in_shape):
    from gennet_amd import layers as Ly
    from gennet_amd.engine import Sequential
    ls = []
    for i, s in enumerate(spec):
        kw = {'input_shape': in_shape} if i == 0 else {}
        if s[0] == 'reshape':
            ls.append(Ly.Reshape(s[1], **kw))
        elif s[0] == 'conv':
            ls.append(Ly.Conv1D(s[1], s[2], padding='valid', activation=s[3], **kw))
        elif s[0] == 'convT':
            ls.append(Ly.Conv2DTranspose(s[1], (1, s[2]), activation=s[3], **kw))
        elif s[0] == 'conv2d':
            ls.append(Ly.Conv2D(s[1], (s[2], 5), strides=(1, 1), padding='same', activation=s[3], **kw))
        elif s[0] == 'leaky':
            ls.append(Ly.LeakyReLU(s[1], **kw))
        elif s[0] == 'bn':
            ls.append(Ly.BatchNormalization(axis=s[1], **kw))
        elif s[0] == 'pool1d':
            ls.append((Ly.MaxPooling1D if s[1] == 'max' else Ly.AveragePooling1D)(s[2], strides=s[3], padding=s[4], **kw))
        elif s[0] == 'pool2d':
            ls.append((Ly.MaxPooling2D if s[1] == 'max' else Ly.AveragePooling2D)(s[2], strides=s[3], padding=s[4], **kw))
        elif s[0] in ('gap1d', 'gmp1d', 'gap2d'):
            ls.append({'gap1d': Ly.GlobalAveragePooling1D, 'gmp1d': Ly.GlobalMaxPooling1D, 'gap2d': Ly.GlobalAveragePooling2D}[s[0]](**kw))
        elif s[0] == 'flatten':
            ls.append(Ly.Flatten(**kw))
        elif s[0] == 'dense':
            ls.append(Ly.Dense(s[1], activation=s[2], **kw))
    return Sequential(ls), ls


def _act(h, kind):
    return {None: lambda v: v, 'tanh': torch.tanh, 'relu': torch.relu, 'sigmoid': torch.sigmoid}[kind](h)


def _torch_pool(mode, h, pool, strides, padding):
    """(B, H, W, C): -inf pads by TensorFlow's rule and a valid max_pool2d; a sum-pool of h over a sum-pool of ones (tests/test_pooling_cpu.py)"""
    B, H, W, C = h.shape
    (Ho, pt), (Wo, pl) = R.pool_geometry(H, pool[0], strides[0], padding), R.pool_geometry(W, pool[1], strides[1], padding)
    pb, pr = max((Ho - 1) * strides[0] + pool[0] - H - pt, 0), max((Wo - 1) * strides[1] + pool[1] - W - pl, 0)
    hc = h.permute(0, 3, 1, 2)
    if mode == 'max':
        y = F.max_pool2d(F.pad(hc, (pl, pr, pt, pb), value=float('-inf')), pool, strides)
    else:
        def sum_pool(t):
            return F.avg_pool2d(F.pad(t, (pl, pr, pt, pb)), pool, strides) * (pool[0] * pool[1])
        y = sum_pool(hc) / sum_pool(torch.ones_like(hc))
    return y.permute(0, 2, 3, 1)


def _ref_forward(spec, P, x, training, moving):
    """torch fp64, channels last, the batch in front (the pattern of tests/test_bn_axis_gpu.py)"""
    h = x
    for i, s in enumerate(spec):
        if s[0] == 'reshape':
            h = h.reshape((h.shape[0],) + tuple(s[1]))
        elif s[0] == 'conv':
            h = _act(F.conv1d(h.permute(0, 2, 1), P[i][0].permute(2, 1, 0)).permute(0, 2, 1) + P[i][1], s[3])
        elif s[0] == 'convT':              # keras kernel (1, kw, filters, Cin), 'valid', stride 1
            kw, W = P[i][0].shape[1], h.shape[2]
            hp = F.pad(h, (0, 0, kw - 1, kw - 1))
            h = _act(sum(hp[:, :, kw - 1 - j:kw - 1 - j + W + kw - 1, :] @ P[i][0][0, j].T for j in range(kw)) + P[i][1], s[3])
        elif s[0] == 'conv2d':             # kernel (kh, kw, Cin, Cout), strides (1, 1), 'same': pads (k - 1) // 2 in front, the rest behind
            kh, kw = P[i][0].shape[:2]
            hp = F.pad(h.permute(0, 3, 1, 2), ((kw - 1) // 2, kw - 1 - (kw - 1) // 2, (kh - 1) // 2, kh - 1 - (kh - 1) // 2))
            h = _act(F.conv2d(hp, P[i][0].permute(3, 2, 0, 1)).permute(0, 2, 3, 1) + P[i][1], s[3])
        elif s[0] == 'leaky':
            h = torch.where(h > 0, h, float(np.float32(s[1])) * h)
        elif s[0] == 'bn':
            ax = s[1] % h.dim()
            dims = tuple(d for d in range(h.dim()) if d != ax)
            shape = [1] * h.dim(); shape[ax] = h.shape[ax]
            if training:
                mean = h.mean(dim=dims); var = ((h - mean.reshape(shape)) ** 2).mean(dim=dims)
            else:
                mean, var = moving[i]
            h = (h - mean.reshape(shape)) / torch.sqrt(var.reshape(shape) + 1e-3) * P[i][0].reshape(shape) + P[i][1].reshape(shape)
        elif s[0] == 'pool1d':
            h = _torch_pool(s[1], h.unsqueeze(2), (s[2], 1), (s[3] or s[2], 1), s[4]).squeeze(2)
        elif s[0] == 'pool2d':
            h = _torch_pool(s[1], h, s[2], s[3] or s[2], s[4])
        elif s[0] in ('gap1d', 'gap2d'):
            h = h.reshape(h.shape[0], -1, h.shape[-1]).mean(1)
        elif s[0] == 'gmp1d':
            h = h.amax(1)
        elif s[0] == 'flatten':
            h = h.reshape(h.shape[0], -1)
        elif s[0] == 'dense':
            h = _act(h @ P[i][0] + P[i][1], s[2])
    return h


def rel(a, ref):
    a = np.asarray(a, np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-30)


WEIGHTED = ('conv', 'convT', 'conv2d', 'dense', 'bn')


def _seeded(net):
    """the model with seeded biases, BatchNormalization parameters and moving statistics (the zero / one initial values would hide them)"""
    in_shape, spec = NETS[net]
    rng = np.random.RandomState(len(net))
    model, ls = _build(spec, in_shape)
    for l, s in zip(ls, spec):
        ws = l.get_weights()
        if s[0] in ('conv', 'convT', 'conv2d', 'dense'):
            l.set_weights([ws[0], rng.randn(*ws[1].shape).astype(np.float32) * 0.1])
        elif s[0] == 'bn':
            C = ws[0].shape[0]
            l.set_weights([1 + 0.2 * rng.randn(C), 0.2 * rng.randn(C), 0.3 * rng.randn(C), 0.5 + rng.rand(C)])
    return model, ls, spec, in_shape, rng


@pytest.mark.parametrize('net', sorted(NETS))
def test_stacks_with_pooling_layers_train_and_predict(net):
    from gennet_amd.engine import SGD
    B, lr = 6, 0.05
    model, ls, spec, in_shape, rng = _seeded(net)
    model.compile(optimizer=SGD(lr=lr), loss='mean_squared_error')
    x = rng.randn(B, *in_shape).astype(np.float32)
    t = rng.randn(B, *model.output_shape[1:]).astype(np.float32)

    def params():
        return ({i: [torch.tensor(w.astype(np.float64), requires_grad=True) for w in l.get_weights()[:2]] for i, (l, s) in enumerate(zip(ls, spec)) if s[0] in WEIGHTED},
                {i: [torch.tensor(w.astype(np.float64)) for w in l.get_weights()[2:]] for i, (l, s) in enumerate(zip(ls, spec)) if s[0] == 'bn'})
    P, moving = params()
    xt, tt = torch.tensor(x.astype(np.float64)), torch.tensor(t.astype(np.float64))
    y = model.predict(x, batch_size=B)
    with torch.no_grad():
        y_ref = _ref_forward(spec, P, xt, False, moving).numpy()
    print(net, 'predict err', rel(y, y_ref))
    assert rel(y, y_ref) < 1e-5
    loss_ref = ((_ref_forward(spec, P, xt, True, moving) - tt) ** 2).mean()
    loss_ref.backward()
    res = model.train_on_batch(x, t)
    print(net, 'loss', res[0], float(loss_ref.detach()))
    assert abs(res[0] - float(loss_ref.detach())) <= 1e-6 * abs(float(loss_ref.detach()))
    # a gradient is measured against its own largest entry, but no finer than 1e-3 of the model's largest gradient entry (a bias in front of a
    # BatchNormalization holds rounding noise only)
    g_floor = 1e-3 * max(float(v.grad.abs().max()) for ts in P.values() for v in ts)
    for i, (l, s) in enumerate(zip(ls, spec)):
        if i not in P:
            continue
        for p, ref in zip(l.params, P[i]):
            g_ref = ref.grad.numpy()
            gr = p.grad.detach().cpu().numpy().reshape(g_ref.shape)
            gerr = np.abs(gr - g_ref).max() / max(np.abs(g_ref).max(), g_floor)
            w_ref = (ref.detach() - lr * ref.grad).numpy()
            werr = np.abs(p.numpy().astype(np.float64) - w_ref).max() / max(np.abs(w_ref).max(), 1e-3)
            print(net, l.name, p.name, 'grad err %.3g weight err %.3g' % (gerr, werr))
            assert gerr < 1e-4 and werr < 1e-4, (l.name, p.name, gerr, werr)
    P2, moving2 = params()
    y2 = model.predict(x, batch_size=B)
    with torch.no_grad():
        y2_ref = _ref_forward(spec, P2, xt, False, moving2).numpy()
    print(net, 'predict after the step: err', rel(y2, y2_ref))
    assert rel(y2, y2_ref) < 1e-5


@pytest.mark.parametrize('net', ['a_sibling_discriminator', 'b_windowed_1d'])
def test_captured_steps_and_save_load_equal_the_eager_run_bit_for_bit(net, tmp_path):
    """the pattern of tests/test_d_model_gpu.py: the layers make no host sync, so a captured step replays; load_model rebuilds them from their configs"""
    from gennet_amd import layers as Ly
    from gennet_amd.engine import Adam, StepGraph, device
    from gennet_amd.keras.models import load_model
    B = 6
    model, ls, spec, in_shape, rng = _seeded(net)
    model.compile(optimizer=Adam(lr=0.004, beta_1=0.5), loss='mean_squared_error')
    start = str(tmp_path / 'start.h5')
    model.save(start)
    xh = rng.randn(B, *in_shape).astype(np.float32)
    th = rng.rand(B, *model.output_shape[1:]).astype(np.float32)
    x = torch.tensor(xh, device=device()); t = torch.tensor(th, device=device())
    eager, graphed = load_model(start), load_model(start)
    assert [type(l) for l in eager.layers] == [type(l) for l in ls] and any(isinstance(l, (Ly._Pooling, Ly._GlobalPooling)) for l in eager.layers)
    la = [eager.train_result(eager.train_on_batch_device([x], [t]), B) for _ in range(4)]
    graphed.train_on_batch_device([x], [t])          # one eager step first: binds the parameter groups and scratch buffers the graph will hold
    sg = StepGraph()
    torch.cuda.synchronize()
    sg.capture(lambda: graphed.train_on_batch_device([x], [t]))
    lb = []
    for i in range(3):
        if i:
            sg.wait_inputs_consumed()
        lb.append(graphed.train_result(sg.replay(), B))
    assert la[1:] == lb
    for a, b in zip(eager.get_weights(), graphed.get_weights()):
        assert np.array_equal(a, b)
    path = str(tmp_path / 'resumed.h5')
    eager.save(path)
    resumed = load_model(path)
    l5 = eager.train_on_batch(xh, th)
    assert resumed.train_on_batch(xh, th) == l5
    for a, b in zip(eager.get_weights(), resumed.get_weights()):
        assert np.array_equal(a, b)
