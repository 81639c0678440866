"""GPU parity of the small-channel convolution kernels (gennet_amd/csrc/small_conv.hip: at most 4 channels on one side, all three
directions), at the shapes where their code changes path.  Every call is asserted to have reached its kernel through the launch counters
11 .. 17 (conv_family.SMALL_KINDS) and to have launched nothing else that is counted.

Checks of every case (check_layer):
  real data     randn inputs against oracle.keras_ref.conv1d_fwd / conv1d_bwd in fp64 on the float32 inputs: 2e-5 of the largest oracle
                magnitude for outputs and data gradients, 5e-5 for weight / bias gradients (the bounds of test_kernels_gpu.py)
  integer data  the same shape with small integers in x, w, b, dy (every partial sum below 2^24 in whatever order it is formed: asserted in
                int_data), epilogue linear, ReLU or leaky 0.25: BIT-IDENTICAL to the int64 numpy result, so a row, tap, channel or chunk
                mix-up shows exactly
  guards        y, dx and dw live inside a larger buffer pre-filled with one NaN bit pattern: the words around them come back unchanged, every
                element inside comes back finite (so every row of a strided data gradient was written)

Which case reaches which seam.  C = the LARGE side, NQ = C / 4 float4 columns, NQc = min(NQ, 256), RL = 256 / NQc row lanes per block
(threads with rl >= RL idle), column blocks = ceil(NQ / 256):
    C 4     NQ 1,   RL 256                C 8     NQ 2,  RL 128                 C 12    NQ 3,  RL 85: 1 idle thread
    C 20    NQ 5,   RL 51: 1 idle         C 100   NQ 25, RL 10: 6 idle          C 512   NQ 128, RL 2
    C 1024  NQ 256, RL 1, one full block  C 1028  NQ 257: forward: a second column trip of ONE thread; weight gradient: a second column block

Forward, small Cin (kind 11, conv_smallcin_kernel<CIN>; MT = min(16 RL, 256) rows per block, the input window through LDS)
    Cin 1..4 x k 1..5, L 9, 'same' and 'valid'; L 1 with k 5 'same' (one row, four of five taps outside)
    Cout 4 (MT 256), 100 (MT 160, the only tile that is no power of two), 512 (MT 32), 1028 (MT 16): Lout = MT - 1, MT, MT + 1
    Cout 12, 20, 1024 (MT 256, 256, 16): Lout = MT + 1
    stride 2 'same' with L even and odd; Cin 4, stride 2, k 5, Lout 257: the largest input window the LDS array holds ((2 * 255 + 5) * 4
    floats) and one row of a second tile; stride 3 halves MT to 128 (Lout 129); all six activations; with and without a bias
    gn_conv1d_fwd_dropout: Cin 1..4 x Cout 8, 12, 1028 x rate 0, 0.4 with a mask that has zeros, against dropout(act(conv)); masked
    elements are exactly zero; on integers the kept ones are the one fp32 product y * (1 / (1 - rate))
Forward, small Cout (kind 12, conv_smallcout_kernel<COUT>: one wave per output row, lanes across Cin in float4 steps, 256 channels a trip)
    Cout 1..4 x Cin 8, 252 (lane 63 idle), 256 (exactly one trip), 260 (a second trip of one lane), 516 (a third trip of one lane)
    B Lout = 1, 4, 5 rows (one wave of a block, one full block, a second block of one wave); stride 1 and 2; k 1, 3, 5
    Cin 4 is NOT a small-Cout launch: Cin <= 4 selects the small-Cin kernel whatever Cout is (capi.hip select_conv), so 4 -> 4 is kind 11
    (asserted) and 4 -> 1..3 is refused by the strict entry; 8 is the narrowest Cin this kernel sees
    the gate of the row-run kernel from outside: Cout 1 / Cin 256 with k 3, with k 5 at stride 2, and with Cin 252 stay on kind 12
Row-run kernel (kind 13, conv_cout1_rows_kernel<5, 16>: Cout 1, Cin >= 256, 5 contiguous taps, unit strides; a wave per run of 16 rows)
    Cin 256, 260 (second trip of one lane), 516, 1024 (four full trips) x Lout 1, 15, 16, 17, 33 (below one run, one short, exact, one row
    of a second run, one row of a third); B 1, 3, 5 at Lout 17: 2, 6, 10 runs (no multiple of the 4 waves of a block, exactly 1.5 and 2.5
    blocks); 'same' and 'valid'; bias with tanh
Data gradients (forward-form launches on the transposed kernel; a strided one is one launch per phase)
    layers with Cout 1..4: small-Cin form (kind 11), offsets descending; layers with Cin 1..4: small-Cout form (kind 12)
    stride 1 (k 5, k 3); stride 2 with k 5 and k 4; stride 3 with k 5; each with L odd and even, 'same' and 'valid' (the 'valid' ones leave
    rows of dx no output row reads: they must come back zero, not unwritten)
    the layer 1 -> 256, k 5, stride 1: Cout' 1 / Cin' 256 with DESCENDING taps stays on kind 12
Weight gradient, small Cin (kind 14, wgrad_smallcin_tab_kernel<CS>: x through a 128-row LDS table, dy rows 4 at a time)
    CS 1..4 x Cout 4, 12, 100, 1028; k 1, 3, 5; strides 1, 2, 3; B 3 x Lout 43 = 129 rows: Cout 4, 12: one chunk = a full 128-row tile and a
    ragged tile of one row; Cout 100: 2 chunks of 65 rows that straddle the batch ends, 10 row lanes x 4-row unroll = 40 rows a trip, the
    second trip ragged; Cout 1028: 17 chunks of 8 rows, the last of one row (the unroll's tail)
Weight gradient, small Cout, stride > 1 (kind 15, wgrad_small_kernel<CS, false>)
    CS 1..4 x Cin 8, 12, 100, 1028 x strides 2, 3 (Cin 4 cannot be reached: Cin <= 4 makes Cin the small side, kind 14 -- asserted)
Weight gradient, small Cout, stride 1 (kind 16, wgrad_smallcout_s1_kernel<CS>: chunks of INPUT rows, dy through the LDS table)
    CS 1..4 x Cin 8, 100, 1028; 'valid' (Lin > M: table rows whose taps fall outside [0, M) are zero) and 'same'; k 1, 3, 5
    the in_stride == 1 gate from both sides: one shape at stride 1 (kind 16) and stride 2 (kind 15)
The reduce (sum_partials: one level up to 64 chunks, level 1 folds chunk k into slab k % 32 above that: kind 17)
    chunks = min(1024 / column blocks, ceil(rows / 8 RL)).  Large side 1024: rows 8, 512, 513, 800, 8200 -> 1, 64 (largest single level),
    65 (smallest two-level: group 0 folds three slabs, the others two), 100 (no multiple of 32), 1024 (the cap); large side 1028, 4100 rows
    -> 512 (the cap with two column blocks).  The restated count is checked against gn_conv1d_wgrad_workspace.  Kind 17 exactly when
    chunks > 64; two runs bit-identical; the 65-chunk case also through kinds 15 and 16.
Exact-size workspace: one case per weight-gradient kernel through the C ABI with exactly gn_conv1d_wgrad_workspace bytes inside a guard.

Worst measured error / bound per test on the MI355X (every run prints them, `pytest -s`) is in each test's docstring, over all its cases:
between 0.000 and 0.027 of the bound everywhere -- the chains here have at most 5 x 1028 terms, or 8200 rows in 1024 fixed-order chunks.
"""
import zlib

import numpy as np
import pytest
import torch

import conv_family as CF
from oracle import keras_ref as K

pytestmark = pytest.mark.gpu

RTOL, RTOL_W = 2e-5, 5e-5
ACTS = [('linear', 0.0), ('relu', 0.0), ('relu_max', 1.0), ('leaky', 0.2), ('tanh', 0.0), ('sigmoid', 0.0)]
INT_ACTS = [('linear', 0.0), ('relu', 0.0), ('leaky', 0.25)]
SENTINEL = 0x7FC0A5A5          # a quiet NaN with a payload: guard words are compared as integers, the inside must come back finite
GUARD = 1024                   # words on each side (a multiple of 4: the kernels store float4)


def dev():
    return torch.device('cuda:0')


def g(a, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=dev())


def f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


class Guarded:
    """A float32 tensor of `shape` inside a buffer of SENTINEL words."""

    def __init__(self, shape):
        self.n = int(np.prod(shape))
        self.buf = torch.full((self.n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=dev())
        self.t = self.buf[GUARD:GUARD + self.n].view(torch.float32).view(*shape)

    def check(self, what):
        assert bool((self.buf[:GUARD] == SENTINEL).all()) and bool((self.buf[GUARD + self.n:] == SENTINEL).all()), '%s: written outside the tensor' % what
        assert bool(torch.isfinite(self.t).all()), '%s: %d elements not written' % (what, int((~torch.isfinite(self.t)).sum()))
        return self.t


class Worst:
    """The worst error / bound of one test, per checked quantity."""

    def __init__(self):
        self.ratio = {}

    def close(self, what, t, ref, tol, case):
        a = t.detach().cpu().numpy().astype(np.float64)
        ref = np.asarray(ref, np.float64)
        assert a.shape == ref.shape, (what, case, a.shape, ref.shape)
        scale = max(np.abs(ref).max(), 1e-30)
        r = np.abs(a - ref).max() / (tol * scale)
        if r > self.ratio.get(what, -1.0):
            self.ratio[what] = r
        assert r <= 1.0, '%s %s: max err %.3e of scale %.3e = %.3f of the %.0e bound' % (what, case, r * tol * scale, scale, r, tol)


@pytest.fixture
def worst(request):
    w = Worst()
    yield w
    print('\n%s: worst error / bound  %s' % (request.node.name, '  '.join('%s %.3f' % kv for kv in sorted(w.ratio.items()))))


def exact(what, t, ref, case):
    a = t.detach().cpu().numpy().astype(np.float64)
    ref = np.asarray(ref, np.float64)
    assert a.shape == ref.shape, (what, case, a.shape, ref.shape)
    bad = np.argwhere(a != ref)
    assert len(bad) == 0, '%s %s: %d of %d elements differ from the integer result, first at %s: %r, expected %r' % (
        what, case, len(bad), a.size, tuple(bad[0]), a[tuple(bad[0])], ref[tuple(bad[0])])


def _rng(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)


def real_data(B, L, Cin, Cout, k, Lout, key):
    rng = _rng('real', key)
    return (f32(rng.randn(B, L, Cin)), f32(rng.randn(k, Cin, Cout) / np.sqrt(k * Cin)), f32(rng.randn(Cout)), f32(rng.randn(B, Lout, Cout)))


def int_data(B, L, Cin, Cout, k, Lout, key):
    """int64 x, w, b, dy with every partial sum of every direction below 2^24 in absolute value, whatever the order of summation: fp32 is exact."""
    rng = _rng('int', key)
    x = rng.randint(-3, 4, (B, L, Cin)).astype(np.int64)
    w = rng.randint(-3, 4, (k, Cin, Cout)).astype(np.int64)
    b = rng.randint(-4, 5, (Cout,)).astype(np.int64)
    dy = rng.randint(-2, 3, (B, Lout, Cout)).astype(np.int64)
    ax, aw, ab, ady = (int(np.abs(v).max()) for v in (x, w, b, dy))
    assert k * Cin * ax * aw + ab < 2 ** 24                 # forward
    assert k * Cout * ady * aw < 2 ** 24                    # data gradient
    assert B * Lout * max(ax, 1) * ady < 2 ** 24            # weight and bias gradient
    return x, w, b, dy


# ---------------------------------------------------------------------------------------------- the C ABI into guarded buffers
def fwd_call(xd, wd, bd, s, pl, Lout, act, p, mask=None, rate=0.0):
    from gennet_amd import _lib, ops
    B, L, Cin = xd.shape
    k, _, Cout = wd.shape
    y = Guarded((B, Lout, Cout))
    if mask is None:
        _lib.call('gn_conv1d_fwd', ops._p(xd), ops._p(wd), ops._p(bd), ops._p(y.t), B, L, Cin, Cout, k, s, pl, Lout, ops.ACT[act], float(p), ops._stream())
    else:
        _lib.call('gn_conv1d_fwd_dropout', ops._p(xd), ops._p(wd), ops._p(bd), ops._p(mask), ops._p(y.t), B, L, Cin, Cout, k, s, pl, Lout, ops.ACT[act],
                  float(p), float(rate), ops._stream())
    return y


def dgrad_call(dyd, wt, L, s, pl):
    from gennet_amd import _lib, ops
    B, Lout, Cout = dyd.shape
    k, _, Cin = wt.shape
    dx = Guarded((B, L, Cin))
    _lib.call('gn_conv1d_dgrad', ops._p(dyd), ops._p(wt), ops._p(dx.t), B, L, Cin, Cout, k, s, pl, Lout, ops._stream())
    return dx


def wgrad_call(xd, dyd, k, s, pl):
    from gennet_amd import ops
    dw = Guarded((k, xd.shape[2], dyd.shape[2]))
    _, db = ops.conv1d_wgrad(xd, dyd, k, s, pl, dw=dw.t)
    return dw, db


def counted(want, fn, case):
    out, got = CF.small_launches(fn)
    assert got == want, '%s: launches %s expected, got %s' % (case, want, got)
    return out


def chunks_of(rows, CL):
    """wgrad_small_chunks restated (checked against gn_conv1d_wgrad_workspace in wgrad_kinds)."""
    NQ = CL // 4
    NQc = min(NQ, 256)
    RL, gx = 256 // NQc, -(-NQ // NQc)
    return max(1, min(-(-1024 // gx), -(-rows // (RL * 8))))


def wgrad_kinds(kind, B, L, Cin, Cout, k, s, Lout):
    """{kind: 1} and the level-1 reduce when the launch has more than 64 chunks; the chunk count cross-checked against the advertised workspace
    (the partial slabs, or the bias gradient's column-reduction partials where those are larger)."""
    from gennet_amd import _lib
    chunks = chunks_of(B * Lout, Cout if Cin <= 4 else Cin)
    slabs = chunks * k * Cin * Cout * 4
    assert _lib.size('gn_conv1d_wgrad_workspace', B, L, Cin, Cout, k, s, Lout) - 256 == max(slabs, _lib.size('gn_bias_grad_workspace', B * Lout, Cout) - 256)
    return ({kind: 1, 17: 1} if chunks > 64 else {kind: 1}), chunks


def check_layer(worst, B, L, Cin, Cout, k, s, padding, fwd=None, dgrad=None, wgrad=None, acts=(('linear', 0.0),), bias=True, no_bias_too=False):
    """The directions whose expected launches ({kind: count}) are given, on real and on integer data, into guarded buffers.  wgrad names the
    weight-gradient kernel's kind; the reduce's kind 17 is added from the chunk count."""
    from gennet_amd import ops
    Lout, pl = ops.conv_geometry(L, k, s, padding)
    case = (B, L, Cin, Cout, k, s, padding)
    assert Lout >= 1, case
    if wgrad is not None:
        wgrad, _ = wgrad_kinds(wgrad, B, L, Cin, Cout, k, s, Lout)
    for ints in (False, True):
        x, w, b, dy = (int_data if ints else real_data)(B, L, Cin, Cout, k, Lout, case)
        if not bias:
            b = None
        tag = '%s %s' % (case, 'int' if ints else 'real')
        xd, wd, dyd = g(x), g(w), g(dy)
        bd = None if b is None else g(b)
        if fwd is not None:
            z = K.conv1d_fwd(x, w, b, s, padding)
            assert z.shape == (B, Lout, Cout), (tag, z.shape)
            for act, p in ([INT_ACTS[zlib.crc32(repr(case).encode()) % 3]] if ints else acts):
                y = counted(fwd, lambda: fwd_call(xd, wd, bd, s, pl, Lout, act, p), tag).check('y ' + tag)
                ref = K.act_fwd(z.astype(np.float64), act, p)
                exact('y', y, ref, tag) if ints else worst.close('y', y, ref, RTOL, tag + ' ' + act)
            if no_bias_too and b is not None:
                y = counted(fwd, lambda: fwd_call(xd, wd, None, s, pl, Lout, 'linear', 0.0), tag).check('y ' + tag)
                ref = K.conv1d_fwd(x, w, None, s, padding)
                exact('y', y, ref, tag) if ints else worst.close('y', y, ref, RTOL, tag + ' no bias')
        if dgrad is None and wgrad is None:
            continue
        dx_ref, dw_ref, db_ref = K.conv1d_bwd(x, w, dy, s, padding)
        if dgrad is not None:
            wt = ops.conv1d_transpose_w(wd)
            dx = counted(dgrad, lambda: dgrad_call(dyd, wt, L, s, pl), tag).check('dx ' + tag)
            exact('dx', dx, dx_ref, tag) if ints else worst.close('dx', dx, dx_ref, RTOL, tag)
        if wgrad is not None:
            dwg, db = counted(wgrad, lambda: wgrad_call(xd, dyd, k, s, pl), tag)
            dw = dwg.check('dw ' + tag)
            if ints:
                exact('dw', dw, dw_ref, tag); exact('db', db, db_ref, tag)
            else:
                worst.close('dw', dw, dw_ref, RTOL_W, tag); worst.close('db', db, db_ref, RTOL_W, tag)


def L_for(Lout, k, s, padding):
    """An input length whose conv has Lout rows."""
    return s * Lout if padding == 'same' else s * (Lout - 1) + k


# ---------------------------------------------------------------------------------------------- forward, small Cin (kind 11)
def test_smallcin_forward_every_cin_and_tap_count(worst):
    """conv_smallcin_kernel<1..4> with 1..5 taps, 'same' and 'valid', and a one-row input whose taps are mostly outside.
    Worst error / bound on the MI355X: y 0.010."""
    for Cin in (1, 2, 3, 4):
        for k in (1, 2, 3, 4, 5):
            for padding in ('same', 'valid'):
                check_layer(worst, 2, 9, Cin, 8, k, 1, padding, fwd={11: 1})
        check_layer(worst, 2, 1, Cin, 8, 5, 1, 'same', fwd={11: 1})


def _mt(Cout):
    NQc = min(Cout // 4, 256)
    return min(16 * (256 // NQc), 256)


@pytest.mark.parametrize("Cout,louts", [(4, (255, 256, 257)), (12, (257,)), (20, (257,)), (100, (159, 160, 161)), (512, (31, 32, 33)), (1024, (17,)),
                                        (1028, (15, 16, 17))])
def test_smallcin_forward_row_tiles_and_uneven_columns(worst, Cout, louts):
    """Lout one short of, at and one past the MT rows of a block, for every column decomposition (idle threads, RL 1, a second column trip).
    Worst error / bound on the MI355X: y 0.012."""
    assert _mt(Cout) in (louts[0] - 1, louts[0] + 1) and (len(louts) == 1 or louts[1] == _mt(Cout))
    for i, Lout in enumerate(louts):
        Cin = 1 + (Cout // 4 + i) % 4
        check_layer(worst, 2, Lout, Cin, Cout, 5, 1, 'same', fwd={11: 1}, no_bias_too=(i == 0))


def test_smallcin_forward_strides_activations_bias(worst):
    """Stride 2 'same' at even and odd L with all six epilogues, with and without a bias; the largest LDS input window (Cin 4, stride 2,
    5 taps, 256 rows) with one row of a second tile; stride 3, where the window halves the rows per block to 128.
    Worst error / bound on the MI355X: y 0.010."""
    for L in (50, 51):
        check_layer(worst, 2, L, 2, 12, 5, 2, 'same', fwd={11: 1}, acts=ACTS, no_bias_too=True)
        check_layer(worst, 2, L, 3, 100, 4, 2, 'valid', fwd={11: 1}, acts=ACTS[:2], bias=False)
    check_layer(worst, 2, 513, 4, 4, 5, 2, 'same', fwd={11: 1})
    check_layer(worst, 2, 515, 4, 4, 5, 2, 'valid', fwd={11: 1})
    check_layer(worst, 2, 387, 4, 4, 5, 3, 'same', fwd={11: 1})
    check_layer(worst, 2, 385, 1, 1028, 5, 3, 'same', fwd={11: 1})


@pytest.mark.parametrize("Cout", [8, 12, 1028])
def test_smallcin_forward_dropout_epilogue(worst, Cout):
    """gn_conv1d_fwd_dropout on the small-Cin kernel against dropout(act(conv)) of the oracle, the mask given: dropped elements exactly zero;
    on integers the kept ones are the single fp32 product y * (1 / (1 - rate)).
    Worst error / bound on the MI355X: y 0.021."""
    from gennet_amd import ops
    B, L, k, s = 2, 19, 5, 1
    Lout, pl = ops.conv_geometry(L, k, s, 'same')
    for Cin in (1, 2, 3, 4):
        for rate in (0.0, 0.4):
            case = ('dropout', Cin, Cout, rate)
            mask = (_rng(case).rand(B, Lout, Cout) >= 0.4).astype(np.uint8)
            assert 0 < mask.sum() < mask.size
            md = g(mask, torch.uint8)
            for ints, (act, p) in ((False, ('leaky', 0.2)), (False, ('tanh', 0.0)), (True, ('leaky', 0.25)), (True, ('linear', 0.0))):
                x, w, b, _ = (int_data if ints else real_data)(B, L, Cin, Cout, k, Lout, case)
                xd, wd, bd = g(x), g(w), g(b)
                y = counted({11: 1}, lambda: fwd_call(xd, wd, bd, s, pl, Lout, act, p, md, rate), case).check('y %s' % (case,))
                a = K.act_fwd(K.conv1d_fwd(x, w, b, s, 'same').astype(np.float64), act, p)
                assert bool((y[md == 0] == 0).all()), case
                if ints:
                    keep = np.float32(1.0) / (np.float32(1.0) - np.float32(rate))
                    exact('y', y, (a.astype(np.float32) * keep) * mask, case)
                else:
                    worst.close('y', y, K.dropout_fwd(a, mask, rate), RTOL, '%s %s' % (case, act))
            # the plain entry on the same inputs is the same conv: with a mask of ones at rate 0 the two are bit-identical
            ones = torch.ones((B, Lout, Cout), dtype=torch.uint8, device=dev())
            assert torch.equal(fwd_call(xd, wd, bd, s, pl, Lout, 'linear', 0.0, ones, 0.0).t, fwd_call(xd, wd, bd, s, pl, Lout, 'linear', 0.0).t), case


# ---------------------------------------------------------------------------------------------- forward, small Cout (kinds 12 and 13)
def _smallcout_kind(Cin, Cout, k, s):
    """The gate of conv_smallcout_dispatch: the row-run kernel takes Cout 1 / Cin >= 256 / 5 contiguous taps / unit strides."""
    return 13 if (Cout == 1 and Cin >= 256 and k == 5 and s == 1) else 12


@pytest.mark.parametrize("Cout", [1, 2, 3, 4])
def test_smallcout_forward_channel_trips_rows_strides_taps(worst, Cout):
    """conv_smallcout_kernel<COUT> over the channel trips (an idle lane, exactly one trip, one lane of a second and of a third), 1, 4 and 5
    output rows, strides 1 and 2, 1, 3 and 5 taps; which rows go with which (stride, taps, padding) rotates with Cin and Cout so that every
    value meets every Cin.  Worst error / bound on the MI355X: y 0.027."""
    rows = [(1, 1), (2, 2), (1, 5), (5, 1)]                                  # (B, Lout): 1, 4, 5, 5 rows
    geo = [(1, 1, 'valid'), (3, 1, 'same'), (5, 2, 'valid'), (3, 2, 'same'), (5, 1, 'same'), (1, 2, 'valid'), (5, 2, 'same'), (3, 1, 'valid'), (5, 1, 'valid')]
    seen = set()
    for i, Cin in enumerate((8, 252, 256, 260, 516)):
        for j in range(len(geo)):
            k, s, padding = geo[j]
            B, Lout = rows[(i + j + Cout) % len(rows)]
            kind = _smallcout_kind(Cin, Cout, k, s)
            seen.add(kind)
            check_layer(worst, B, L_for(Lout, k, s, padding), Cin, Cout, k, s, padding, fwd={kind: 1}, acts=(('leaky', 0.2),), no_bias_too=(j == 0))
    assert seen == ({12, 13} if Cout == 1 else {12})


def test_smallcout_gates(worst):
    """Both sides of every gate around conv_smallcout_kernel: Cin <= 4 is a small-Cin launch whatever Cout is; the row-run kernel takes
    Cout 1 / Cin >= 256 / k 5 / stride 1 only.  Worst error / bound on the MI355X: y 0.010, dx 0.009, dw 0.003, db 0.000."""
    check_layer(worst, 2, 9, 4, 4, 5, 1, 'same', fwd={11: 1}, dgrad={11: 1}, wgrad=14)       # 4 -> 4: the small-Cin kernels in every direction
    check_layer(worst, 2, 9, 8, 4, 5, 1, 'same', fwd={12: 1})
    check_layer(worst, 2, 20, 256, 1, 5, 1, 'same', fwd={13: 1})
    check_layer(worst, 2, 20, 252, 1, 5, 1, 'same', fwd={12: 1})                              # Cin below 256
    check_layer(worst, 2, 20, 256, 1, 3, 1, 'same', fwd={12: 1})                              # 3 taps
    check_layer(worst, 2, 20, 256, 1, 5, 2, 'same', fwd={12: 1})                              # stride 2
    check_layer(worst, 2, 20, 256, 2, 5, 1, 'same', fwd={12: 1})                              # Cout 2
    check_layer(worst, 2, 20, 1, 256, 5, 1, 'same', dgrad={12: 1})                            # the data gradient of 1 -> 256: descending taps


@pytest.mark.parametrize("Cin", [256, 260, 516, 1024])
def test_cout1_row_run_kernel(worst, Cin):
    """conv_cout1_rows_kernel at every run boundary and channel trip, with run counts that fill no whole block, bias and tanh.
    Worst error / bound on the MI355X: y 0.021."""
    acts = (('tanh', 0.0), ('linear', 0.0))
    for i, Lout in enumerate((1, 15, 16, 17, 33)):
        padding = ('same', 'valid')[(i + Cin // 4) % 2]
        check_layer(worst, 2, L_for(Lout, 5, 1, padding), Cin, 1, 5, 1, padding, fwd={13: 1}, acts=acts, no_bias_too=(i == 3))
    for B in (1, 3, 5):
        for padding in ('same', 'valid'):
            check_layer(worst, B, L_for(17, 5, 1, padding), Cin, 1, 5, 1, padding, fwd={13: 1}, acts=acts)


# ---------------------------------------------------------------------------------------------- data gradients
DGRAD_GEO = [(5, 1), (3, 1), (5, 2), (4, 2), (5, 3)]           # (k, stride)


@pytest.mark.parametrize("c", [1, 2, 3, 4])
def test_data_gradient_small_cin_form(worst, c):
    """Layers with Cout = c: the data gradient is a small-Cin launch (kind 11) per phase on the transposed kernel, offsets descending.
    Worst error / bound on the MI355X: dx 0.008."""
    for i, (k, s) in enumerate(DGRAD_GEO):
        CL = (12, 8, 100, 1028, 20)[(i + c) % 5]
        for L in (21, 22):
            for padding in ('same', 'valid'):
                check_layer(worst, 2, L, CL, c, k, s, padding, dgrad={11: s})


@pytest.mark.parametrize("c", [1, 2, 3, 4])
def test_data_gradient_small_cout_form(worst, c):
    """Layers with Cin = c: the data gradient is a small-Cout launch (kind 12) per phase; never the row-run kernel (descending taps).
    Worst error / bound on the MI355X: dx 0.009."""
    for i, (k, s) in enumerate(DGRAD_GEO):
        CL = (260, 8, 252, 516, 256)[(i + c) % 5]
        for L in (21, 22):
            for padding in ('same', 'valid'):
                check_layer(worst, 2, L, c, CL, k, s, padding, dgrad={12: s})


# ---------------------------------------------------------------------------------------------- weight gradients
@pytest.mark.parametrize("Cout", [4, 12, 100, 1028])
def test_weight_gradient_small_cin(worst, Cout):
    """wgrad_smallcin_tab_kernel<1..4> over 129 rows in 3 batch elements: a full and a one-row table tile, chunks across batch ends, the
    4-row unroll's tail; strides 1, 2, 3 and 1, 3, 5 taps.  Worst error / bound on the MI355X: dw 0.010, db 0.001."""
    geo = [(5, 1, 'same'), (3, 2, 'valid'), (1, 3, 'same'), (5, 2, 'same'), (3, 1, 'valid'), (5, 3, 'valid'), (1, 1, 'valid'), (3, 3, 'same'), (1, 2, 'same')]
    for CS in (1, 2, 3, 4):
        for j in range(3):
            k, s, padding = geo[(3 * CS + j + Cout // 4) % len(geo)]
            check_layer(worst, 3, L_for(43, k, s, padding), CS, Cout, k, s, padding, wgrad=14)


@pytest.mark.parametrize("Cin", [8, 12, 100, 1028])
def test_weight_gradient_small_cout_strided(worst, Cin):
    """wgrad_small_kernel<1..4, false> at strides 2 and 3.  Worst error / bound on the MI355X: dw 0.010, db 0.001."""
    geo = [(5, 2, 'same'), (5, 3, 'valid'), (3, 2, 'valid'), (4, 2, 'same'), (3, 3, 'same'), (1, 2, 'valid')]
    for CS in (1, 2, 3, 4):
        for j in range(3):
            k, s, padding = geo[(3 * CS + j + Cin // 4) % len(geo)]
            check_layer(worst, 3, L_for(43, k, s, padding), Cin, CS, k, s, padding, wgrad=15)


@pytest.mark.parametrize("Cin", [8, 100, 1028])
def test_weight_gradient_small_cout_unit_stride(worst, Cin):
    """wgrad_smallcout_s1_kernel<1..4>: 'valid' (more input rows than output rows: zero rows in the dy table) and 'same'; the same shape at
    stride 2 is the other kernel.  Worst error / bound on the MI355X: dw 0.007, db 0.001."""
    for CS in (1, 2, 3, 4):
        for k, padding in ((5, 'valid'), (5, 'same'), ((3, 1)[CS % 2], ('valid', 'same')[CS // 2 % 2])):
            check_layer(worst, 3, L_for(43, k, 1, padding), Cin, CS, k, 1, padding, wgrad=16)
        check_layer(worst, 3, 86, Cin, CS, 5, 2, 'same', wgrad=15)


def test_weight_gradient_cin_4_is_the_small_cin_kernel(worst):
    """Cin <= 4 makes Cin the small side whatever Cout is: 4 -> 4 runs the tabled small-Cin kernel at every stride, never kinds 15 / 16.
    Worst error / bound on the MI355X: dw 0.006, db 0.001."""
    for s in (1, 2):
        check_layer(worst, 3, 43 * s, 4, 4, 5, s, 'same', wgrad=14)


REDUCE = [
    # B, Lout, Cin, Cout, chunks, the weight-gradient kernel's kind
    (2, 4, 1, 1024, 1, 14), (2, 256, 2, 1024, 64, 14), (3, 171, 1, 1024, 65, 14), (2, 400, 3, 1024, 100, 14), (2, 4100, 1, 1024, 1024, 14),
    (2, 2050, 1, 1028, 512, 14),
    (2, 256, 1024, 2, 64, 16), (3, 171, 1024, 1, 65, 16), (2, 256, 1024, 3, 64, 15), (3, 171, 1024, 2, 65, 15),
]


@pytest.mark.parametrize("B,Lout,Cin,Cout,chunks,kind", REDUCE)
def test_partial_slab_reduce(worst, B, Lout, Cin, Cout, chunks, kind):
    """sum_partials at 1, 64, 65, 100, 1024 and (two column blocks) 512 chunks: one level up to 64, the level-1 kernel (kind 17) above; the
    chunk count is confirmed by the advertised workspace; exact on integers; two runs bit-identical.
    Worst error / bound on the MI355X: dw 0.007, db 0.001."""
    from gennet_amd import ops
    s = 2 if kind == 15 else 1
    k, padding = (5 if Lout < 1000 else 3), 'same'
    L = L_for(Lout, k, s, padding)
    want, n = wgrad_kinds(kind, B, L, Cin, Cout, k, s, Lout)
    assert n == chunks and (17 in want) == (chunks > 64)
    check_layer(worst, B, L, Cin, Cout, k, s, padding, wgrad=kind)
    x, _, _, dy = real_data(B, L, Cin, Cout, k, Lout, 'twice')
    xd, dyd = g(x), g(dy)
    pl = ops.conv_geometry(L, k, s, padding)[1]
    dw1, db1 = ops.conv1d_wgrad(xd, dyd, k, s, pl)
    dw2, db2 = ops.conv1d_wgrad(xd, dyd, k, s, pl)
    assert torch.equal(dw1, dw2) and torch.equal(db1, db2)


@pytest.mark.parametrize("B,L,Cin,Cout,k,s,padding,kind", [(3, 43, 3, 100, 5, 1, 'same', 14), (3, 86, 100, 3, 5, 2, 'same', 15), (3, 47, 1028, 2, 5, 1, 'valid', 16),
                                                           (3, 171, 1, 1024, 5, 1, 'same', 14)])
def test_weight_gradient_inside_an_exact_size_workspace(B, L, Cin, Cout, k, s, padding, kind):
    """The C ABI with exactly gn_conv1d_wgrad_workspace bytes: nothing is written past them, and the result is the ops call's bit for bit."""
    from gennet_amd import _lib, ops
    Lout, pl = ops.conv_geometry(L, k, s, padding)
    x, _, _, dy = real_data(B, L, Cin, Cout, k, Lout, 'exact-ws')
    xd, dyd = g(x), g(dy)
    want, _ = wgrad_kinds(kind, B, L, Cin, Cout, k, s, Lout)
    nb = _lib.size('gn_conv1d_wgrad_workspace', B, L, Cin, Cout, k, s, Lout)
    guard = 1 << 16
    buf = torch.full((nb + guard,), 0xA5, dtype=torch.uint8, device=dev())
    dw, db = Guarded((k, Cin, Cout)), Guarded((Cout,))
    counted(want, lambda: _lib.call('gn_conv1d_wgrad', ops._p(xd), ops._p(dyd), ops._p(dw.t), ops._p(db.t), ops._p(buf), nb, B, L, Cin, Cout, k, s, pl, Lout,
                                    ops._stream()), (B, L, Cin, Cout))
    torch.cuda.synchronize()
    assert bool((buf[nb:] == 0xA5).all()), 'partial slabs written past the advertised workspace size'
    dw_ops, db_ops = ops.conv1d_wgrad(xd, dyd, k, s, pl)
    assert torch.equal(dw.check('dw'), dw_ops) and torch.equal(db.check('db'), db_ops)
