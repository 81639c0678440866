"""GPU parity of keras layers.SeparableConv1D: csrc/depthwise.hip through gn_dwconv1d_fwd / _dgrad / _wgrad against the fp64 definition
tests/sepconv_ref.py (itself checked against torch and torch autograd in tests/test_sepconv_cpu.py), and the layer at model level against torch
fp64 autograd on the CPU.

Section 1, kernel level.  Inputs sit in NaN-surrounded buffers, outputs in sentinel-filled ones; a view starts 144 bytes in (pad 36: 16-byte
aligned, the vector path where the channel count allows it) or 148 bytes in (pad 37: every base pointer moved by one float, the scalar path of
the same kernels).  sepconv_ref.SHAPES is a covering set of (B, L, C, k, stride, dilation, dm, padding) drawn from
  C   {1, 3, 4, 5, 8, 67, 260}: either side of the 4-float vector; 260 scalar channel lanes are more than the 256 a block of the weight gradient spans
  L   {1, 2, 7, 33, 130, 257}    k  {1, 2, 3, 5, 16, 40}: one sweep of 8 taps, two, five    stride {1, 2, 3}    dilation {1, 2, 5}    dm {1, 2, 3}
  B   {1, 3, 17}                 both paddings; Lout = 1; a window longer than the sequence (k = 40 'same' on 7 rows)
that straddles the kernels' own edges (csrc/depthwise_geom.h, test_the_shapes_straddle_the_kernel_edges).
The bounds are derived, none is measured: with u = 2^-24 and gamma_n = n u / (1 - n u),
  y   one fmaf chain of at most k terms:                       |y^ - y|   <= gamma_k sum_t |x w|
  dx  one fmaf chain of at most k dm terms:                    |dx^ - dx| <= gamma_{k dm} sum |dy w|
  (the vector forms of dm == 2 keep these orders)
  dw  a thread's fmaf chain holds at most rpp terms (the rows of its part), everything behind it is fp64 and one rounding to fp32 (u), so
      |dw^ - dw| <= gamma_{rpp + 2} sum |x dy| (the fp64 sums add less than 2^-40 of that).
Section 2, model level: the logic and the bounds of tests/test_lstm_gpu.py's train_and_compare, as they stand."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sepconv_ref as R
from test_lstm_gpu import EPS, LR, Guarded, dev, same_bits, seed_biases, torch_params, train_and_compare

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES, IDS = R.SHAPES, R.IDS


def gamma(n):
    return n * EPS / (1 - n * EPS)


def geom_constants():
    text = open(os.path.join(ROOT, 'gennet_amd', 'csrc', 'depthwise_geom.h')).read()
    return dict((k, int(eval(v.replace('(size_t)', '')))) for k, v in re.findall(r'constexpr \w+ (DW_\w+) = ([^;]+);', text))


def wgrad_parts(rows, n, K):
    """csrc/depthwise_geom.h's dw_wgrad_parts, restated: (parts, rows a part)"""
    p = max(min(-(-rows // K['DW_WG_MIN_ROWS']), K['DW_WG_MAX_PARTS'], K['DW_WG_WS_CAP'] // (8 * n)), 1)
    rpp = -(-rows // p)
    return -(-rows // rpp), rpp


def fwd_items(B, Lout, nvec, K):
    """csrc/depthwise_geom.h's dw_fwd_row_lanes and dw_fwd_items, restated: (items, row lanes RS)"""
    R4 = K['DW_ROWS']
    RS = max(1, min(K['DW_WAVE'] // nvec, -(-Lout // R4)))
    return B * -(-Lout // (R4 * RS)) * RS * nvec, RS


def lout_of(shape):
    B, L, C, k, s, d, dm, padding = shape
    return R.geometry(L, k, s, padding, d)[0]


def test_the_shapes_cover_the_set():
    S = SHAPES
    assert set(s[0] for s in S) == {1, 3, 17} and set(s[1] for s in S) == {1, 2, 7, 33, 130, 257} and set(s[2] for s in S) == {1, 3, 4, 5, 8, 67, 260}
    assert set(s[3] for s in S) == {1, 2, 3, 5, 16, 40} and set(s[4] for s in S) == {1, 2, 3} and set(s[5] for s in S) == {1, 2, 5}
    assert set(s[6] for s in S) == {1, 2, 3} and set(s[7] for s in S) == {'same', 'valid'} and len(S) == len(set(S)) == 24
    assert any(lout_of(s) == 1 for s in S) and any((s[3] - 1) * s[5] + 1 > s[1] for s in S) and (17, 7, 4, 40, 1, 1, 1, 'same') in S
    assert all(lout_of(s) >= 1 for s in S)


def test_the_shapes_straddle_the_kernel_edges():
    """every shape runs at pad 36 (vector path where C dm % 4 == 0, data gradient C % 4 == 0) and at pad 37 (scalar path), so both V count.
    Below, at and above every edge that the value set can reach; k = 8 (one full sweep of the weight gradient) and exactly 256 channel lanes are
    not in it, so those two edges are held from below and above (k = 16 and 40 are at a multiple of the sweep)."""
    from gennet_amd import _lib
    K = geom_constants()
    assert (K['DW_BLOCK'], K['DW_VEC'], K['DW_ROWS'], K['DW_WAVE'], K['DW_WG_TAPS'], K['DW_WG_MIN_ROWS']) == (256, 4, 4, 64, 8, 64)
    louts = [lout_of(s) for s in SHAPES]
    R4 = K['DW_ROWS']
    assert any(l < R4 for l in louts) and R4 in louts and any(l > R4 and l % R4 for l in louts) and any(l > R4 and l % R4 == 0 for l in louts)
    # both paths, and the vector path under dm == 1 (16-byte loads of x) and dm > 1 (scalar loads of x beside 16-byte stores)
    assert any(s[2] * s[6] % 4 for s in SHAPES) and any(s[2] % 4 == 0 and s[6] == 1 for s in SHAPES) and any(s[2] * s[6] % 4 == 0 and s[6] > 1 for s in SHAPES)
    fwd_rs = [fwd_items(B, lo, C * dm // V, K) + (lo, C * dm // V) for (B, L, C, k, s, d, dm, p), lo in zip(SHAPES, louts) for V in (1, 4) if C * dm % V == 0]
    fwd = [f[0] for f in fwd_rs]
    # the forward's row lanes: one (64 channel groups or more), several as the wave allows, several as few as the rows allow, a wave of one
    # channel group; and a last row group with rows beyond Lout
    assert any(rs == 1 and n >= 64 for _, rs, lo, n in fwd_rs) and any(rs > 1 and rs == 64 // n for _, rs, lo, n in fwd_rs)
    assert any(1 < rs < 64 // n for _, rs, lo, n in fwd_rs) and any(n == 1 and rs > 1 for _, rs, lo, n in fwd_rs)
    assert any(lo % (R4 * rs) for _, rs, lo, n in fwd_rs) and any(lo % (R4 * rs) == 0 for _, rs, lo, n in fwd_rs)
    dgr = [B * L * C // V for (B, L, C, k, s, d, dm, p) in SHAPES for V in (1, 4) if C % V == 0]
    cap = K['DW_GRID_CAP'] * K['DW_BLOCK']
    for items in (fwd, dgr):      # less than a block, a part-filled last block, more items than the capped grid has threads (the grid-stride loop turns)
        assert any(i < K['DW_BLOCK'] for i in items) and any(i > K['DW_BLOCK'] and i % K['DW_BLOCK'] for i in items) and any(i > cap for i in items)
    lanes = [C * dm // V for (B, L, C, k, s, d, dm, p) in SHAPES for V in (1, 4) if C * dm % V == 0]
    assert any(n == 1 for n in lanes) and any(256 % n for n in lanes if n < 256) and any(n > 256 for n in lanes)
    assert any(s[3] < K['DW_WG_TAPS'] for s in SHAPES) and any(s[3] == 2 * K['DW_WG_TAPS'] for s in SHAPES) and any(s[3] == 5 * K['DW_WG_TAPS'] for s in SHAPES)
    rows = [s[0] * lo for s, lo in zip(SHAPES, louts)]
    M = K['DW_WG_MIN_ROWS']
    assert any(r < M for r in rows) and M in rows and any(r > M for r in rows)
    parts = [wgrad_parts(r, s[3] * s[2] * s[6], K) for s, r in zip(SHAPES, rows)]
    assert any(p == 1 for p, _ in parts) and any(p == 2 for p, _ in parts) and any(p > 8 for p, _ in parts)
    assert any(r % rpp for (p, rpp), r in zip(parts, rows) if p > 1)                             # a short last part
    for s, lo, (p, rpp) in zip(SHAPES, louts, parts):
        assert _lib.size('gn_dwconv1d_wgrad_workspace', s[0], lo, s[2], s[3], s[6]) == p * s[3] * s[2] * s[6] * 8


# ---------------------------------------------------------------------------------------------------------------------
# section 1: the three kernels
# ---------------------------------------------------------------------------------------------------------------------
class GuardedBytes(object):
    """`n` bytes, 64 bytes into a sentinel-filled byte buffer: the exact-size workspace"""

    def __init__(self, n):
        self.n = n
        self.buf = torch.full((n + 128,), 0xA5, dtype=torch.uint8, device=dev())
        assert (self.buf.data_ptr() + 64) % 8 == 0

    def ptr(self):
        return self.buf.data_ptr() + 64

    def edges_untouched(self):
        return bool((self.buf[:64] == 0xA5).all()) and bool((self.buf[64 + self.n:] == 0xA5).all())

    def untouched(self):
        return bool((self.buf == 0xA5).all())


def run_kernels(shape, x, w, dy, pad=37, which=('fwd', 'dgrad', 'wgrad')):
    """the three entry points on guarded buffers, the weight gradient on a workspace of exactly the stated size"""
    from gennet_amd import _lib
    B, L, C, k, s, d, dm, padding = shape
    Lout, pl, _ = R.geometry(L, k, s, padding, d)
    gx, gw, gdy = Guarded(x.shape, x, pad), Guarded(w.shape, w, pad), Guarded(dy.shape, dy, pad)
    st = torch.cuda.current_stream().cuda_stream
    out = {}
    if 'fwd' in which:
        y = Guarded((B, Lout, C * dm), None, pad)
        _lib.call('gn_dwconv1d_fwd', gx.t.data_ptr(), gw.t.data_ptr(), y.t.data_ptr(), B, L, C, k, dm, s, d, pl, Lout, st)
        out['y'] = y.check('dwconv1d_fwd')
    if 'dgrad' in which:
        dx = Guarded((B, L, C), None, pad)
        _lib.call('gn_dwconv1d_dgrad', gdy.t.data_ptr(), gw.t.data_ptr(), dx.t.data_ptr(), B, L, C, k, dm, s, d, pl, Lout, st)
        out['dx'] = dx.check('dwconv1d_dgrad')
    if 'wgrad' in which:
        dw = Guarded((k, C, dm), None, pad)
        nb = _lib.size('gn_dwconv1d_wgrad_workspace', B, Lout, C, k, dm)
        ws = GuardedBytes(nb)
        with pytest.raises(_lib.GennetHipError) as e:
            _lib.call('gn_dwconv1d_wgrad', gx.t.data_ptr(), gdy.t.data_ptr(), dw.t.data_ptr(), ws.ptr(), nb - 1, B, L, C, k, dm, s, d, pl, Lout, st)
        assert '(%d)' % _lib.GN_EWORKSPACE in str(e.value) and 'workspace too small' in str(e.value)
        torch.cuda.synchronize()
        assert dw.untouched() and ws.untouched()
        _lib.call('gn_dwconv1d_wgrad', gx.t.data_ptr(), gdy.t.data_ptr(), dw.t.data_ptr(), ws.ptr(), nb, B, L, C, k, dm, s, d, pl, Lout, st)
        out['dw'] = dw.check('dwconv1d_wgrad')
        assert ws.edges_untouched(), 'dwconv1d_wgrad wrote outside its workspace'
    return out


@pytest.mark.parametrize('pad', [36, 37], ids=['aligned', 'shifted'])
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_integer_data_is_exact(shape, pad):
    """x and dy integers in [-4, 4], w in [-2, 2]: every partial sum of every order is an integer below 2^24 (asserted first), so each of the three
    results equals the fp64 reference bit for bit -- a wrong tap, pad, stride phase or channel order cannot hide"""
    B, L, C, k, s, d, dm, padding = shape
    rng = np.random.RandomState(1000 + SHAPES.index(shape))
    Lout = lout_of(shape)
    x = rng.randint(-4, 5, size=(B, L, C)).astype(np.float64)
    w = rng.randint(-2, 3, size=(k, C, dm)).astype(np.float64)
    dy = rng.randint(-4, 5, size=(B, Lout, C * dm)).astype(np.float64)
    geo = (s, padding, d)
    assert max(R.dw_fwd(np.abs(x), np.abs(w), *geo).max(), R.dw_dgrad(np.abs(dy), np.abs(w), L, *geo).max(),
               R.dw_wgrad(np.abs(x), np.abs(dy), k, *geo).max()) < 2 ** 24
    got = run_kernels(shape, x, w, dy, pad)
    assert same_bits(got['y'], R.dw_fwd(x, w, *geo))
    assert same_bits(got['dx'], R.dw_dgrad(dy, w, L, *geo))
    assert same_bits(got['dw'], R.dw_wgrad(x, dy, k, *geo))


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_real_data_meets_the_derived_bounds(shape):
    B, L, C, k, s, d, dm, padding = shape
    rng = np.random.RandomState(2000 + SHAPES.index(shape))
    Lout = lout_of(shape)
    x, w, dy = (rng.randn(*sh).astype(np.float32) for sh in ((B, L, C), (k, C, dm), (B, Lout, C * dm)))
    geo = (s, padding, d)
    got = run_kernels(shape, x, w, dy, 36 if SHAPES.index(shape) % 2 else 37)
    _, rpp = wgrad_parts(B * Lout, k * C * dm, geom_constants())
    for name, ref, mag, terms in (
            ('y', R.dw_fwd(x, w, *geo), R.dw_fwd(np.abs(x), np.abs(w), *geo), k),
            ('dx', R.dw_dgrad(dy, w, L, *geo), R.dw_dgrad(np.abs(dy), np.abs(w), L, *geo), R.dgrad_terms(L, k, s, padding, d, dm)),
            ('dw', R.dw_wgrad(x, dy, k, *geo), R.dw_wgrad(np.abs(x), np.abs(dy), k, *geo), rpp + 2)):
        err = np.abs(got[name].astype(np.float64) - ref)
        bound = gamma(terms) * mag
        worst = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
        print(name, 'terms', terms, 'largest error / bound %.3g' % worst)
        assert bool((err <= bound).all()), (name, worst)
    assert R.dgrad_terms(L, k, s, padding, d, dm) <= k * dm


def test_a_sample_does_not_depend_on_the_batch_or_the_launch():
    """sample 0 alone and as the first of 3 and of 17: y and dx bit for bit; dw bit-identical over two runs (B = 17: several row parts)"""
    rng = np.random.RandomState(7)
    for C, k, s, d, dm, padding in ((8, 5, 1, 2, 1, 'same'), (5, 4, 2, 1, 3, 'same')):
        L = 33
        Lout = R.geometry(L, k, s, padding, d)[0]
        w = rng.randn(k, C, dm).astype(np.float32)
        x, dy = rng.randn(17, L, C).astype(np.float32), rng.randn(17, Lout, C * dm).astype(np.float32)
        runs = [run_kernels((B, L, C, k, s, d, dm, padding), x[:B], w, dy[:B], 36) for B in (1, 3, 17, 17)]
        for r in runs[1:]:
            assert same_bits(r['y'][:1], runs[0]['y']) and same_bits(r['dx'][:1], runs[0]['dx'])
        assert same_bits(runs[2]['dw'], runs[3]['dw']) and same_bits(runs[2]['y'], runs[3]['y'])
        assert not same_bits(runs[1]['dw'], runs[2]['dw'])


def test_bad_arguments_are_errors_and_launch_nothing():
    from gennet_amd import _lib, ops
    B, L, C, k, dm, Lout = 2, 9, 4, 3, 2, 7
    one = lambda *s: np.ones(s, np.float32)          # noqa: E731
    x, w, dy = (Guarded(s, one(*s), 36) for s in ((B, L, C), (k, C, dm), (B, Lout, C * dm)))
    outs = [Guarded(s, None, 36) for s in ((B, Lout, C * dm), (B, L, C), (k, C, dm))]
    y, dx, dw = outs
    st = torch.cuda.current_stream().cuda_stream
    ws = ops.workspace(_lib.size('gn_dwconv1d_wgrad_workspace', B, Lout, C, k, dm) + 64, dev())
    good = dict(x=x.t.data_ptr(), w=w.t.data_ptr(), dy=dy.t.data_ptr(), y=y.t.data_ptr(), dx=dx.t.data_ptr(), dw=dw.t.data_ptr(), ws=ws.data_ptr(),
                ws_bytes=ws.numel(), B=B, L=L, C=C, k=k, dm=dm, stride=1, dilation=1, pad_left=0, Lout=Lout)

    def fwd(**kw):
        g = dict(good, **kw)
        _lib.call('gn_dwconv1d_fwd', g['x'], g['w'], g['y'], g['B'], g['L'], g['C'], g['k'], g['dm'], g['stride'], g['dilation'], g['pad_left'], g['Lout'], st)

    def dgrad(**kw):
        g = dict(good, **kw)
        _lib.call('gn_dwconv1d_dgrad', g['dy'], g['w'], g['dx'], g['B'], g['L'], g['C'], g['k'], g['dm'], g['stride'], g['dilation'], g['pad_left'], g['Lout'],
                  st)

    def wgrad(**kw):
        g = dict(good, **kw)
        _lib.call('gn_dwconv1d_wgrad', g['x'], g['dy'], g['dw'], g['ws'], g['ws_bytes'], g['B'], g['L'], g['C'], g['k'], g['dm'], g['stride'], g['dilation'],
                  g['pad_left'], g['Lout'], st)

    def refused(text, fn, code=None):
        with pytest.raises(_lib.GennetHipError) as e:
            fn()
        assert '(%d)' % (_lib.GN_EINVAL if code is None else code) in str(e.value) and text in str(e.value), str(e.value)
        assert text in _lib.lib().gn_last_error().decode()
        torch.cuda.synchronize()
        assert all(o.untouched() for o in outs)

    for call, ptrs in ((fwd, ('x', 'w', 'y')), (dgrad, ('dy', 'w', 'dx')), (wgrad, ('x', 'dy', 'dw', 'ws'))):
        for p in ptrs:
            refused('null pointer', lambda: call(**{p: None}))
        for n in ('L', 'C', 'k', 'dm', 'Lout'):
            refused('bad shape', lambda: call(**{n: 0}))
        refused('bad shape', lambda: call(B=-1))
        for kw in (dict(stride=0), dict(dilation=0), dict(pad_left=-1)):
            refused('bad geometry', lambda: call(**kw))
        refused('does not fit', lambda: call(C=1 << 20, k=1 << 10, dm=2))
        refused('2^62', lambda: call(B=1 << 30, L=(1 << 31) - 1, Lout=(1 << 31) - 1, C=16, k=1, dm=1))
        call(B=0)                                               # nothing to do is not an error and launches nothing
        call(B=0, x=None, w=None, dy=None, y=None, dx=None, dw=None, ws=None)
    refused('workspace too small', lambda: wgrad(ws_bytes=_lib.size('gn_dwconv1d_wgrad_workspace', B, Lout, C, k, dm) - 1), _lib.GN_EWORKSPACE)
    refused('8-byte aligned', lambda: wgrad(ws=ws.data_ptr() + 4))
    torch.cuda.synchronize()
    assert all(o.untouched() for o in outs)
    fwd(), dgrad(), wgrad()
    y.check('dwconv1d_fwd'), dx.check('dwconv1d_dgrad'), dw.check('dwconv1d_wgrad')
    with pytest.raises(ValueError, match='depthwise kernel'):
        ops.dwconv1d_fwd(x.t, w.t[:, :3].contiguous())
    with pytest.raises(ValueError, match='rows'):
        ops.dwconv1d_dgrad(dy.t, w.t, L + 1)
    with pytest.raises(ValueError, match='rows'):
        ops.dwconv1d_fwd(x.t[:, :2].contiguous(), w.t)


def test_the_ops_wrappers_take_the_geometry_from_conv_geometry():
    """ops.dwconv1d_* on an even window with stride 2 under 'same' (pad 1 left, 2 right on 10 rows with 5 taps of dilation 1 ... by TF's rule)"""
    from gennet_amd import ops
    from gennet_amd.engine import to_device
    rng = np.random.RandomState(8)
    B, L, C, k, s, dm = 3, 10, 5, 4, 2, 3
    x, w = rng.randint(-4, 5, size=(B, L, C)).astype(np.float32), rng.randint(-2, 3, size=(k, C, dm)).astype(np.float32)
    dy = rng.randint(-4, 5, size=(B, 5, C * dm)).astype(np.float32)
    xd, wd, dyd = to_device(x), to_device(w), to_device(dy)
    assert same_bits(ops.dwconv1d_fwd(xd, wd, s, 'same').cpu().numpy(), R.dw_fwd(x, w, s, 'same'))
    assert same_bits(ops.dwconv1d_dgrad(dyd, wd, L, s, 'same').cpu().numpy(), R.dw_dgrad(dy, w, L, s, 'same'))
    into = torch.empty((k, C, dm), dtype=torch.float32, device=dev())
    assert ops.dwconv1d_wgrad(xd, dyd, k, s, 'same', dw=into) is into and same_bits(into.cpu().numpy(), R.dw_wgrad(x, dy, k, s, 'same'))


# ---------------------------------------------------------------------------------------------------------------------
# section 2: models against torch fp64 autograd (tests/test_lstm_gpu.py's train_and_compare and its bounds)
# ---------------------------------------------------------------------------------------------------------------------
def sep_ref(P, layer, x):
    dwk, pwk, b = P[layer.name]
    return R.torch_forward(x, dwk, pwk, b, layer.stride, layer.padding, layer.dilation, layer.activation[0])


def model_a():
    """SeparableConv1D(16, 5, 'same', dm 2, relu, l2 | l1) -> MaxPooling1D -> SeparableConv1D(8, 3, strides 2) -> Flatten -> Dense(2)"""
    from gennet_amd import layers as Ly, regularizers
    from gennet_amd.engine import Sequential
    first = Ly.SeparableConv1D(16, 5, padding='same', depth_multiplier=2, activation='relu', depthwise_regularizer=regularizers.l2(0.01),
                               pointwise_regularizer=regularizers.l1(0.002), input_shape=(22, 4))
    second, head = Ly.SeparableConv1D(8, 3, strides=2), Ly.Dense(2)
    model = Sequential()
    for l in (first, Ly.MaxPooling1D(2), second, Ly.Flatten(), head):
        model.add(l)

    def ref(P, x):
        h = sep_ref(P, first, x)
        h = F.max_pool1d(h.permute(0, 2, 1), 2).permute(0, 2, 1)
        h = sep_ref(P, second, h)
        return h.reshape(h.shape[0], -1) @ P[head.name][0] + P[head.name][1]
    return model, ref


def test_two_separable_layers_train_as_torch_fp64_and_the_penalty_shows():
    model, ref = model_a()
    rng = np.random.RandomState(41)
    seed_biases(model, rng)
    assert model.output_shape == (None, 2) and [n.out_shape for n in model.nodes] == [(22, 16), (11, 16), (5, 8), (40,), (2,)]
    pens = train_and_compare(model, ref, [rng.randn(6, 22, 4).astype(np.float32)], rng.randn(6, 2).astype(np.float32), what='sep-pool-sep')
    assert min(pens) > 0.01                                                  # the loss was held against loss + penalty: the penalty is no rounding matter


def test_a_residual_dilated_block_trains_as_torch_fp64():
    """Conv1D(8, 1) -> Add([., SeparableConv1D(8, 3, dilation_rate=2, 'same', tanh)]) -> GlobalAveragePooling1D -> Dense(1): two edges leave the
    Conv1D, and the separable layer's input gradient is added to the skip's"""
    from gennet_amd import layers as Ly
    from gennet_amd.engine import Input, Model
    x = Input((19, 3))
    conv, sep, head = Ly.Conv1D(8, 1), Ly.SeparableConv1D(8, 3, dilation_rate=2, padding='same', activation='tanh'), Ly.Dense(1)
    h = conv(x)
    model = Model(inputs=x, outputs=head(Ly.GlobalAveragePooling1D()(Ly.Add()([h, sep(h)]))))
    rng = np.random.RandomState(42)
    seed_biases(model, rng)

    def ref(P, x):
        h = x @ P[conv.name][0][0] + P[conv.name][1]
        return (h + sep_ref(P, sep, h)).mean(1) @ P[head.name][0] + P[head.name][1]
    train_and_compare(model, ref, [rng.randn(5, 19, 3).astype(np.float32)], rng.randn(5, 1).astype(np.float32), what='residual')


def test_odd_everything_with_a_softmax_trains_as_torch_fp64():
    """3 input channels, SeparableConv1D(5, 2, depth_multiplier=3) 'valid' with activation='softmax': 9 depthwise channels, no count a multiple of 4"""
    from gennet_amd import layers as Ly
    from gennet_amd.engine import Sequential
    sep, head = Ly.SeparableConv1D(5, 2, depth_multiplier=3, activation='softmax', input_shape=(7, 3)), Ly.Dense(3)
    model = Sequential()
    for l in (sep, Ly.Flatten(), head):
        model.add(l)
    rng = np.random.RandomState(43)
    seed_biases(model, rng)

    def ref(P, x):
        h = sep_ref(P, sep, x)
        return h.reshape(h.shape[0], -1) @ P[head.name][0] + P[head.name][1]
    train_and_compare(model, ref, [rng.randn(7, 7, 3).astype(np.float32)], rng.randn(7, 3).astype(np.float32), what='odd-softmax')


def test_a_frozen_layer_passes_the_input_gradient_and_a_first_layer_forms_none(monkeypatch):
    """frozen in the middle: the layers in front train as torch's do (the input gradient passes) and its own weights stay; as the first layer no
    dx is formed (ops.dwconv1d_dgrad is not called)"""
    from gennet_amd import layers as Ly, ops
    from gennet_amd.engine import Sequential
    front, sep, head = Ly.Conv1D(4, 3, input_shape=(15, 2)), Ly.SeparableConv1D(6, 3, depth_multiplier=2, padding='same', activation='sigmoid'), Ly.Dense(1)
    sep.trainable = False
    model = Sequential()
    for l in (front, sep, Ly.Flatten(), head):
        model.add(l)
    rng = np.random.RandomState(44)
    seed_biases(model, rng)
    before = [w.copy() for w in sep.get_weights()]

    def ref(P, x):
        w, b = P[front.name]
        h = F.conv1d(x.permute(0, 2, 1), w.permute(2, 1, 0)).permute(0, 2, 1) + b
        h = R.torch_forward(h, *[torch.tensor(v.astype(np.float64)) for v in before], 1, 'same', 1, 'sigmoid')
        return h.reshape(h.shape[0], -1) @ P[head.name][0] + P[head.name][1]
    calls = []
    real = ops.dwconv1d_dgrad
    monkeypatch.setattr(ops, 'dwconv1d_dgrad', lambda *a, **k: calls.append(1) or real(*a, **k))
    # train_and_compare's steps and bounds over the two layers that train (it walks every layer that has weights, the frozen one included)
    from gennet_amd.engine import SGD
    model.compile(optimizer=SGD(lr=LR), loss='mean_squared_error')
    x, t = rng.randn(4, 15, 2).astype(np.float32), rng.randn(4, 1).astype(np.float32)
    P = torch_params([front, head])
    xt, tt = torch.tensor(x.astype(np.float64)), torch.tensor(t.astype(np.float64))
    for step in range(3):
        for ts in P.values():
            for v in ts:
                v.grad = None
        loss_ref = ((ref(P, xt) - tt) ** 2).mean()
        loss_ref.backward()
        res = model.train_on_batch(x, t)
        res = res[0] if isinstance(res, (list, tuple)) else res
        assert abs(res -float(loss_ref.detach())) <= 1e-6 * abs(float(loss_ref.detach()))
        g_floor = 1e-3 * max(float(v.grad.abs().max()) for ts in P.values() for v in ts)
        for l in (front, head):
            for p, r in zip(l.params, P[l.name]):
                g_ref = r.grad.numpy()
                gerr = np.abs(p.grad.detach().cpu().numpy().reshape(g_ref.shape) - g_ref).max() / max(np.abs(g_ref).max(), g_floor)
                with torch.no_grad():
                    r -= LR * r.grad
                werr = np.abs(p.numpy().astype(np.float64) - r.detach().numpy()).max() / max(np.abs(r.detach().numpy()).max(), 1e-3)
                print('frozen', step, p.name, 'grad err %.3g weight err %.3g' % (gerr, werr))
                assert gerr < 1e-4 and werr < 1e-4, (step, p.name, gerr, werr)
        assert float(P[front.name][0].grad.abs().max()) > 0
    assert all(np.array_equal(a, b) for a, b in zip(before, sep.get_weights())) and len(calls) == 3
    del calls[:]
    model, ref = model_a()
    seed_biases(model, rng)
    train_and_compare(model, ref, [rng.randn(3, 22, 4).astype(np.float32)], rng.randn(3, 2).astype(np.float32), what='first layer')
    assert len(calls) == 3                                                   # the second layer's three steps; the first layer forms no dx


def test_save_and_load_round_trip(tmp_path):
    from gennet_amd import h5lite, keras_io
    from gennet_amd.engine import SGD, load_model
    model, _ = model_a()
    rng = np.random.RandomState(45)
    seed_biases(model, rng)
    x, t = rng.randn(5, 22, 4).astype(np.float32), rng.randn(5, 2).astype(np.float32)
    model.compile(optimizer=SGD(lr=LR), loss='mean_squared_error')
    model.train_on_batch(x, t)
    path = os.path.join(str(tmp_path), 'sep.h5')
    model.save(path)
    again = load_model(path)
    assert [type(n.layer).__name__ for n in again.nodes] == ['SeparableConv1D', 'MaxPooling1D', 'SeparableConv1D', 'Flatten', 'Dense']
    sep = again.layers[0]
    assert [p.name for p in sep.weights] == ['%s/%s' % (sep.name, n) for n in ('depthwise_kernel', 'pointwise_kernel', 'bias')]
    g = h5lite.File(path)['model_weights'][sep.name]
    assert keras_io._decode_list(g.attrs.get('weight_names')) == [
        '%s/%s:0' % (sep.name, n) for n in ('depthwise_kernel', 'pointwise_kernel', 'bias')]
    assert sep.get_config() == model.layers[0].get_config() and sep.depthwise_kernel.regularizer.l2 == np.float32(0.01)
    assert np.array_equal(model.predict(x), again.predict(x))
    a, b = model.train_on_batch(x, t), again.train_on_batch(x, t)
    assert a == b and all(np.array_equal(u, v) for u, v in zip(model.get_weights(), again.get_weights()))


def test_predict_allocates_no_tape():
    from gennet_amd import engine
    model, _ = model_a()
    x = np.random.RandomState(46).randn(3, 22, 4).astype(np.float32)
    ctx = engine.RunContext(False)
    out = model._forward(model._prep_inputs(x), ctx)
    assert tuple(out[0].shape) == (3, 2) and model.nodes[0].index not in ctx.tape and model.nodes[2].index not in ctx.tape
    ctx = engine.RunContext(True)
    model._forward(model._prep_inputs(x), ctx)
    kept = ctx.tape[model.nodes[0].index]
    assert [tuple(v.shape) for v in kept] == [(3, 22, 4), (3, 22, 8), (3, 22, 16)]           # x, t, y (relu)
    kept = ctx.tape[model.nodes[2].index]
    assert [None if v is None else tuple(v.shape) for v in kept] == [(3, 11, 16), (3, 5, 16), None]          # linear: y is not kept


def test_a_captured_step_replays_bit_identically():
    """model (a) as a hipGraph (engine.StepGraph): eager step, capture, three replays against four eager steps of a twin"""
    from gennet_amd import engine
    from gennet_amd.engine import SGD, to_device
    rng = np.random.RandomState(47)
    x, t = to_device(rng.randn(5, 22, 4).astype(np.float32)), to_device(rng.randn(5, 2).astype(np.float32))
    eager, _ = model_a()
    seed_biases(eager, rng)
    graphed, _ = model_a()
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
