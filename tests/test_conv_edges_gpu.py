"""The matrix-core convolution families at their buffer and workspace edges: the direct kernels (csrc/conv_mfma.hip, conv_pipe.hip,
wgrad_pipe.hip), the merged and phased stride-2 data gradients, the transform-domain kernels (conv_wino*.hip, wgrad_wino*.hip), the opt-in
split kernels (conv_bf16x3.hip, wgrad_bf16x3.hip) and the Dense layers that run on them.  These kernels stage their operands by LDS-DMA
through buffer descriptors whose byte counts are computed in the kernel, and store through a descriptor of Ly * Cout * 4 bytes that drops the
rows of a ragged last tile: a count that is too large reads or writes past the tensor, which a parity test on torch.empty never sees.

Every call here goes through the C ABI (_lib.call) on views inside larger buffers (GUARD = 1024 words on each side, so every view keeps the
16-byte alignment the kernels are given everywhere else):
  float inputs  x, w, wt, bias, dy, y_prev inside one quiet-NaN bit pattern (NanIn): the NaN words come back unchanged (compared as int32) and
                the inside is bit-identical to what was put in; a stray LOAD brings a NaN into an output
  u8 masks      inside 0xA5 bytes (ByteIn), checked the same way
  outputs       y, dx, dw, db, sums inside a sentinel pattern (Guarded): the sentinel words on both sides come back unchanged, every word inside
                comes back finite (every row was written, the rows of a 'valid' strided data gradient that no output row reads included)
  workspaces    exactly the advertised size followed by 64 KiB of 0xA5 (ExactWs): the guard comes back untouched
  the result    against oracle.keras_ref in fp64 on the float32 inputs at the bounds of the family's own parity test (test_kernels_gpu.py: 2e-5 of
                the largest oracle magnitude for y / dx, 5e-5 for dw / db; test_bf16x3_gpu.py: y, dw 2e-5, the merged stride-2 data gradient 2e-6,
                db 1e-5), bit for bit against the ops wrapper on plain tensors (the guard does not change the kernel's path), and -- direct and
                split kernels, Dense -- BIT-IDENTICAL to the int64 numpy result on small integers (every partial sum below 2^24; integers up to
                128 are exact in one bf16 piece).  The transform-domain kernels multiply by sixths and fifteenths: tolerance only.
Every call is asserted to reach its family through the launch counters (conv_family.run).  Counter kind 0 does not tell the members of the direct
family apart, so conv_member / dgrad_members / wgrad_member restate the selection of conv_mfma_dispatch, launch_conv, conv_pipe_try,
conv_pipe_merged_supported, conv_pipe_run_merged, wgrad_square and wgrad_split_plan, every row names its member, and the test asserts that the
restated rule gives that name; the restated K-split count is cross-checked against gn_conv1d_wgrad_workspace.

Which row reaches which member and seam (TM = rows per block; "last" = rows in the last M tile of every batch element, B >= 2 so that a ragged
tile of element 0 would land in element 1):
Forward (FWD)
    generic square   20 -> 72 and 48 -> 192 (Cout % 128, Cin % 8 nonzero), M 129 / 257 (last 1) and 128 (full).  48 -> 192 at M 129 would be the
                     tall tile and the pipelined kernel (fill(256) == fill(128)), so its one-row tile is taken at M 257
    dma square       1 tap, 16 -> 128, M 129 (last 1): the pipelined kernel needs 2 taps
    dma tall         4 taps, stride 2, 16 -> 64, M 257 (last 1): a strided pipelined launch needs 5 taps
    pipe narrow 256  16 -> 4096, B 4: M 255, 256, 257            pipe narrow 64   16 -> 64, B 2: M 63, 64, 65
    pipe narrow 128  16 -> 4096, B 2: M 129, 255, 256 (blocks_of(4) == blocks_of(2) up to M 128, so 128-row blocks exist for M 129 .. 256
                     only here: last 1, 127 and full)
    pipe tall        8 -> 512, 5 taps, B 4, M 4097: 2080 wave tiles, 17 tiles of 256, last 1
    pipe square      the same with 3 taps: 33 tiles of 128, last 1
    stride 2, pipe   16 -> 64, L 130 and 131, 'same' and 'valid' (de-interleaved slab: the odd half one row shorter at odd spans)
    wino             32 -> 64, TM 128: M 127, 128, 129 and 1, 2, 3
    wino_s2          32 -> 64, TM 128: M 127, 128, 129 (L 254, 256, 258) and L 1, 2, 3
    bf16x3           256 -> 256: the 128-row kernel (M < 192) at M 127, 128, 129 and 1, 2, 3, the 256-row kernel at M 255, 256, 257; stride 2
                     (M >= 192) at M 255, 256, 257
Data gradient (DGRAD; the launch runs Cout -> Cin, M = L rows, or ceil(L / 2) pairs)
    generic square   72 <- 20, L 129     pipe narrow 64   64 <- 16, L 65
    merged 256       4096 <- 16, both phases per wave: L 513, 514 x 'same', 'valid' (odd L: the odd phase one row shorter; even L 'valid': the last row
                     of dx is read by no output row and must be zero); 1024 <- 16, B 8, L 896 just inside merge_below
    merged 128 / 64  one phase per wave: 4096 <- 16, L 259 'same' / 260 'valid'; 128 <- 24, L 131 'same' / 130 'valid'
    phases           1024 <- 16, B 8, L 898 just outside merge_below; 32 <- 64 (Cout' % 64 nonzero) and 4 taps
    wino             64 <- 32, L 127, 128, 129, 1, 2, 3        wino_s2  64 <- 32, TM 256 rows of dx: L 255, 256, 257, 2, 3 and 256 'valid'
    bf16x3           256 <- 256 L 129, 257; merged stride 2: L 511, 512, 513
    fused            gn_conv1d_dgrad_fused (MODE 2 relu, leaky; MODE 3 mask + rate) on direct, wino, merged and wino_s2, y_prev and mask_prev guarded
Weight gradient (WGRAD; db wanted and NULL, always in exactly gn_conv1d_wgrad_workspace bytes)
    reg 64x64        3 taps 16 -> 64; 1 tap 8 -> 8 with B 256, L 1: 256 splits of 256-byte slabs, the largest split count per slab byte, M 1
    reg 32x128       2 taps 64 -> 128; 20 -> 72 stride 2 (ragged channels); 3 taps 64 -> 128 B 3 L 700: splits INSIDE batch elements
    pipe 64x64       64 -> 128 B 3 L 700: splits INSIDE batch elements, ragged last chunk; 64 -> 64 B 256 L 1: 256 whole-element splits of one-row
                     elements with the per-split bias partials behind 20 MB of slabs; B 4 L 20: elements shorter than a chunk; stride 2 B 5 L 333 (whole elements) and B 3 L 1400
                     (inside)
    pipe 32x128      32 -> 128 B 3 L 133
    wino / wino_s2 / bf16x3 (stride 1 and 2): ragged chunks, splits inside elements, 1 .. 3 rows
Also: gn_conv1d_fwd_dropout (MODE 1 mask descriptor) and gn_conv1d_fwd_stats (y, sums, workspace guarded) on direct, wino, wino_s2; gn_dense_fwd /
gn_dense_bwd (dx wanted and NULL) on the matrix-core route; gn_conv1d_fwd_wino, gn_conv1d_fwd_bf16x3 and the conv-math workspaces of modes 2 and
1 at exact size; one byte less than advertised is GN_EWORKSPACE with nothing written.

Worst measured error / bound per test on the MI355X (`pytest -s` prints them) is in each test's docstring.
"""
import contextlib
import zlib

import numpy as np
import pytest
import torch

import conv_family as CF
from oracle import keras_ref as K

pytestmark = pytest.mark.gpu

RTOL, RTOL_W = 2e-5, 5e-5                                              # test_kernels_gpu.py
BF16X3_TOL = {'y': 2e-5, 'dx': 2e-5, 'dx merged': 2e-6, 'dw': 2e-5, 'db': 1e-5}      # test_bf16x3_gpu.py
SENTINEL = 0x7FC0A5A5          # outputs: a quiet NaN with a payload
NANWORD = 0x7FC05A5A           # around inputs: another one
FILL = 0xA5                    # bytes around masks and behind workspaces
GUARD = 1024                   # words on each side (a multiple of 4: every view stays 16-byte aligned)
WS_GUARD = 1 << 16
INT_ACTS = [('linear', 0.0), ('relu', 0.0), ('leaky', 0.25)]
EXACT = ('direct', 'merged', 'phases', 'bf16x3')                       # families whose arithmetic is exact on small integers


def dev():
    return torch.device('cuda:0')


def g(a, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=dev())


def f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def _rng(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)


def _cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------- guarded buffers
class Guarded:
    """An output tensor of `shape` (float32 or float64) inside a buffer of SENTINEL words."""

    def __init__(self, shape, dtype=torch.float32):
        self.words = int(np.prod(shape)) * (2 if dtype == torch.float64 else 1)
        self.buf = torch.full((self.words + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=dev())
        self.t = self.buf[GUARD:GUARD + self.words].view(dtype).view(*shape)

    def check(self, what):
        inside = self.buf[GUARD:GUARD + self.words]
        assert bool((self.buf[:GUARD] == SENTINEL).all()) and bool((self.buf[GUARD + self.words:] == SENTINEL).all()), '%s: written outside the tensor' % what
        assert bool(torch.isfinite(self.t).all()), '%s: %d elements not written, or NaN read from outside an input' % (what, int((~torch.isfinite(self.t)).sum()))
        assert not bool((inside == SENTINEL).any()), '%s: words not written' % what
        return self.t

    def untouched(self):
        return bool((self.buf == SENTINEL).all())


class NanIn:
    """A float32 input (numpy array or device tensor) inside a buffer of NANWORD words."""

    def __init__(self, a):
        a = a.detach().to(dev()) if torch.is_tensor(a) else g(a)
        self.n = a.numel()
        self.buf = torch.full((self.n + 2 * GUARD,), NANWORD, dtype=torch.int32, device=dev())
        self.t = self.buf[GUARD:GUARD + self.n].view(torch.float32).view(*a.shape)
        self.t.copy_(a)
        self.bits = self.buf[GUARD:GUARD + self.n].clone()

    def check(self, what):
        assert bool((self.buf[:GUARD] == NANWORD).all()) and bool((self.buf[GUARD + self.n:] == NANWORD).all()), '%s: the guard of an input was written' % what
        assert torch.equal(self.buf[GUARD:GUARD + self.n], self.bits), '%s: an input was written' % what


class ByteIn:
    """A uint8 keep-mask inside a buffer of FILL bytes (4 * GUARD on each side)."""

    def __init__(self, a):
        a = g(a, torch.uint8)
        self.n, self.g = a.numel(), 4 * GUARD
        self.buf = torch.full((self.n + 2 * self.g,), FILL, dtype=torch.uint8, device=dev())
        self.t = self.buf[self.g:self.g + self.n].view(*a.shape)
        self.t.copy_(a)
        self.bits = self.t.clone()

    def check(self, what):
        assert bool((self.buf[:self.g] == FILL).all()) and bool((self.buf[self.g + self.n:] == FILL).all()), '%s: the guard of a mask was written' % what
        assert torch.equal(self.t, self.bits), '%s: a mask was written' % what


class ExactWs:
    """A workspace of exactly nb bytes, followed by WS_GUARD bytes of FILL."""

    def __init__(self, nb):
        self.nb = int(nb)
        self.buf = torch.full((self.nb + WS_GUARD,), FILL, dtype=torch.uint8, device=dev())

    def check(self, what, used=None):
        """Nothing behind the first `used` bytes (default: all nb) was written."""
        torch.cuda.synchronize()
        assert bool((self.buf[self.nb if used is None else int(used):] == FILL).all()), '%s: written past the advertised workspace size' % what

    def untouched(self):
        return bool((self.buf == FILL).all())


def checked(what, *inputs):
    for i in inputs:
        if i is not None:
            i.check(what)


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


def tol_of(family, what, stride=1):
    if family == 'bf16x3':
        return BF16X3_TOL['dx merged' if (what == 'dx' and stride == 2) else what]
    return RTOL if what in ('y', 'dx') else RTOL_W


@contextlib.contextmanager
def conv_math(math):
    from gennet_amd import ops
    if math == 'bf16x3':
        ops.set_conv_math('bf16x3', workspace_gb=0.25)
        try:
            yield
        finally:
            ops.set_conv_math()
    else:
        with ops.conv_math(math):
            yield


# ---------------------------------------------------------------------------------------------- the selection rule of the direct family, restated
def conv_member(B, M, Lin, Ly, Cin, Cout, ntaps, in_stride, span):
    """conv_mfma_dispatch -> launch_conv -> conv_pipe_try for one forward-form launch of M rows per batch element (Lin input rows, Ly output rows
    per element, `span` = rows the taps cover)."""
    def fill(T):
        return float(M) / (float(_cdiv(M, T)) * T)
    tall = Cout <= 64 or (Cout % 64 == 0 and ntaps >= 4 and fill(256) >= 0.97 * fill(128))
    TN, KC, tile = (64 if tall else 128), (16 if ntaps == 1 else 8), ('tall' if tall else 'square')
    if not (Cout % TN == 0 and Cin % KC == 0 and Lin * Cin * 4 < 2 ** 30):
        return 'generic ' + tile
    if KC == 8 and 2 <= ntaps <= 5 and span <= ntaps and Ly * Cout * 4 < 2 ** 30 and (in_stride == 1 or (in_stride == 2 and ntaps == 5)):
        if Cout % 64 == 0 and B * _cdiv(M, 64) * (Cout // 64) < 2048:
            nwm = 4
            while nwm > 1 and B * _cdiv(M, 64 * nwm) * (Cout // 64) < 256:
                nwm >>= 1
            return 'pipe narrow %d' % (64 * nwm)
        return 'pipe ' + tile
    return 'dma ' + tile


def dgrad_members(B, L, Cin, Cout, k, s, pl, Lout):
    """select_dgrad / dgrad_impl under the fp32 math for the layer Cin -> Cout: the merged member, or one conv_member per output phase."""
    if s == 2 and k == 5 and L >= 2 and Cin > 4 and Cout > 4:
        M = (L + 1) // 2
        if Cout % 8 == 0 and Cin % 64 == 0 and L * Cin * 4 < 2 ** 30 and Lout * Cout * 4 < 2 ** 30 and B * _cdiv(M, 64) * (Cin // 64) * 2 < 2048:
            nwm = 4
            while nwm > 1 and B * _cdiv(M, 64 * nwm) * (Cin // 64) < 256:
                nwm >>= 1
            return ('merged %d %s' % (64 * nwm, 'two-set' if nwm == 4 else 'phase-split'),)
    out = []
    for p in range(min(s, L)):
        taps = [kk for kk in range(k) if (p + pl - kk) % s == 0]
        out.append(conv_member(B, (L - p + s - 1) // s, Lout, L, Cout, Cin, len(taps), 1, len(taps)))
    return tuple(out)


def split_plan(B, M, Cin, Cout, TC, TN):
    """wgrad_split_plan: (splits, K-chunks of 32 rows per split)."""
    cpb, tiles = _cdiv(M, 32), _cdiv(Cin, TC) * _cdiv(Cout, TN)
    s = max(_cdiv(2048, tiles), 1)
    if s <= B or tiles * B >= 256:
        s = min(s, B)
        cps = _cdiv(B, s) * cpb
    else:
        s = _cdiv(512, tiles)
        cps = _cdiv(cpb, min(_cdiv(s, B), max(cpb // 4, 1)))
    return _cdiv(B * cpb, cps), cps


def wgrad_member(B, M, Cin, Cout, ntaps):
    """wgrad_square / launch_wgrad / wgrad_split_plan: (member, splits)."""
    square = Cout <= 64 or (ntaps == 5 and Cin % 64 == 0 and Cout % 64 == 0)
    TC, TN = (64, 64) if square else (32, 128)
    piped = ntaps == 5 and Cin % TC == 0 and Cout % TN == 0
    splits, cps = split_plan(B, M, Cin, Cout, TC, TN)
    how = 'inside' if cps < _cdiv(M, 32) else 'whole'
    return '%s %dx%d %s' % ('pipe' if piped else 'reg', TC, TN, how), splits


# ---------------------------------------------------------------------------------------------- data and oracle of one case
def real_data(B, L, Cin, Cout, k, Lout, key):
    rng = _rng('real', key)
    return (f32(rng.randn(B, L, Cin)), f32(rng.randn(k, Cin, Cout) / np.sqrt(k * Cin)), f32(rng.randn(Cout)), f32(rng.randn(B, Lout, Cout)))


def int_data(B, L, Cin, Cout, k, Lout, key):
    """int64 x, w, b, dy with every partial sum of every direction below 2^24 in absolute value, whatever the order of summation: fp32 is exact
    (and every value is exact in one bf16 piece)."""
    rng = _rng('int', key)
    hi = 4 if k * Cin * 9 + 4 < 2 ** 24 and k * Cout * 6 < 2 ** 24 else 2
    x = rng.randint(-(hi - 1), hi, (B, L, Cin)).astype(np.int64)
    w = rng.randint(-(hi - 1), hi, (k, Cin, Cout)).astype(np.int64)
    b = rng.randint(-4, 5, (Cout,)).astype(np.int64)
    dy = rng.randint(-2, 3, (B, Lout, Cout)).astype(np.int64)
    ax, aw, ab, ady = (int(np.abs(v).max()) for v in (x, w, b, dy))
    assert max(ax, aw, ab, ady) <= 128
    assert k * Cin * ax * aw + ab < 2 ** 24                 # forward
    assert k * Cout * ady * aw < 2 ** 24                    # data gradient
    assert B * Lout * max(ax, 1) * ady < 2 ** 24            # weight and bias gradient
    return x, w, b, dy


class Case:
    """Inputs of one layer shape (real or integer data), on the host, as plain device tensors and inside NaN guards; the oracle's results, each
    computed once.  Shared between the maths of a shape through CF.OneCase."""

    def __init__(self, B, L, Cin, Cout, k, s, padding, ints):
        from gennet_amd import ops
        self.shape = (B, L, Cin, Cout, k, s, padding)
        self.ints = ints
        self.Lout, self.pl = ops.conv_geometry(L, k, s, padding)
        assert self.Lout >= 1, self.shape
        self.x, self.w, self.b, self.dy = (int_data if ints else real_data)(B, L, Cin, Cout, k, self.Lout, self.shape)
        self._dev, self._nan, self._z, self._bwd = {}, {}, None, None
        self.tag = '%s %s' % (self.shape, 'int' if ints else 'real')

    def host(self, name):
        return getattr(self, name)

    def plain(self, name):
        from gennet_amd import ops
        if name not in self._dev:
            self._dev[name] = ops.conv1d_transpose_w(self.plain('w')) if name == 'wt' else g(self.host(name))
        return self._dev[name]

    def nan(self, name):
        if name not in self._nan:
            self._nan[name] = NanIn(self.plain(name))
        return self._nan[name]

    @property
    def z(self):
        if self._z is None:
            self._z = K.conv1d_fwd(self.x, self.w, self.b, self.shape[5], self.shape[6]).astype(np.float64)
            assert self._z.shape == (self.shape[0], self.Lout, self.shape[3])
        return self._z

    @property
    def bwd(self):
        if self._bwd is None:
            self._bwd = K.conv1d_bwd(self.x.astype(np.float64), self.w.astype(np.float64), self.dy.astype(np.float64), self.shape[5], self.shape[6])
        return self._bwd


_REAL, _INT = CF.OneCase(), CF.OneCase()


def case_of(shape, ints=False):
    return (_INT if ints else _REAL).get(tuple(shape), lambda: Case(*shape, ints))


def ids(rows, n=9):
    return ['-'.join(str(v) for v in r[:n]) for r in rows]


# ---------------------------------------------------------------------------------------------- the C ABI into guarded buffers
def c_fwd(c, act, p, mask=None, rate=0.0, bias=True):
    from gennet_amd import _lib, ops
    B, L, Cin, Cout, k, s, _ = c.shape
    x, w, b = c.nan('x'), c.nan('w'), (c.nan('b') if bias else None)
    y = Guarded((B, c.Lout, Cout))
    if mask is None:
        _lib.call('gn_conv1d_fwd', ops._p(x.t), ops._p(w.t), ops._p(b.t if b else None), ops._p(y.t), B, L, Cin, Cout, k, s, c.pl, c.Lout, ops.ACT[act], float(p), ops._stream())
    else:
        _lib.call('gn_conv1d_fwd_dropout', ops._p(x.t), ops._p(w.t), ops._p(b.t if b else None), ops._p(mask.t), ops._p(y.t), B, L, Cin, Cout, k, s, c.pl, c.Lout,
                  ops.ACT[act], float(p), float(rate), ops._stream())
    t = y.check('y ' + c.tag)
    checked('fwd ' + c.tag, x, w, b, mask)
    return t


def c_dgrad(c, prev=None):
    """prev = (NanIn y_prev, act, param, ByteIn mask or None, rate): gn_conv1d_dgrad_fused."""
    from gennet_amd import _lib, ops
    B, L, Cin, Cout, k, s, _ = c.shape
    dy, wt = c.nan('dy'), c.nan('wt')
    dx = Guarded((B, L, Cin))
    if prev is None:
        _lib.call('gn_conv1d_dgrad', ops._p(dy.t), ops._p(wt.t), ops._p(dx.t), B, L, Cin, Cout, k, s, c.pl, c.Lout, ops._stream())
        yp = mk = None
    else:
        yp, act, param, mk, rate = prev
        _lib.call('gn_conv1d_dgrad_fused', ops._p(dy.t), ops._p(wt.t), ops._p(dx.t), B, L, Cin, Cout, k, s, c.pl, c.Lout, ops._p(yp.t), ops._p(mk.t if mk else None),
                  ops.ACT[act], float(param), float(rate), ops._stream())
    t = dx.check('dx ' + c.tag)
    checked('dgrad ' + c.tag, dy, wt, yp, mk)
    return t


def c_wgrad(c, want_db=True):
    """gn_conv1d_wgrad in exactly gn_conv1d_wgrad_workspace bytes: (dw, db or None)."""
    from gennet_amd import _lib, ops
    B, L, Cin, Cout, k, s, _ = c.shape
    x, dy = c.nan('x'), c.nan('dy')
    dw, db = Guarded((k, Cin, Cout)), (Guarded((Cout,)) if want_db else None)
    ws = ExactWs(_lib.size('gn_conv1d_wgrad_workspace', B, L, Cin, Cout, k, s, c.Lout))
    _lib.call('gn_conv1d_wgrad', ops._p(x.t), ops._p(dy.t), ops._p(dw.t), ops._p(db.t if db else None), ops._p(ws.buf), ws.nb, B, L, Cin, Cout, k, s, c.pl, c.Lout,
              ops._stream())
    ws.check('wgrad ' + c.tag)
    checked('wgrad ' + c.tag, x, dy)
    return dw.check('dw ' + c.tag), (db.check('db ' + c.tag) if db else None)


# ---------------------------------------------------------------------------------------------- forward
FWD = [
    # B, L, Cin, Cout, k, stride, padding, math, family, member of the direct family (conv_member)
    (2, 129, 20, 72, 5, 1, 'same', 'fp32', 'direct', 'generic square'),
    (2, 128, 20, 72, 5, 1, 'same', 'fp32', 'direct', 'generic square'),
    (2, 257, 48, 192, 5, 1, 'same', 'fp32', 'direct', 'generic square'),
    (2, 128, 48, 192, 5, 1, 'same', 'fp32', 'direct', 'generic square'),
    (2, 129, 16, 128, 1, 1, 'valid', 'fp32', 'direct', 'dma square'),
    (2, 514, 16, 64, 4, 2, 'same', 'fp32', 'direct', 'dma tall'),
    (4, 255, 16, 4096, 5, 1, 'same', 'fp32', 'direct', 'pipe narrow 256'),
    (4, 256, 16, 4096, 5, 1, 'same', 'fp32', 'direct', 'pipe narrow 256'),
    (4, 257, 16, 4096, 5, 1, 'same', 'fp32', 'direct', 'pipe narrow 256'),
    (2, 129, 16, 4096, 5, 1, 'same', 'fp32', 'direct', 'pipe narrow 128'),
    (2, 255, 16, 4096, 5, 1, 'same', 'fp32', 'direct', 'pipe narrow 128'),
    (2, 256, 16, 4096, 5, 1, 'same', 'fp32', 'direct', 'pipe narrow 128'),
    (2, 63, 16, 64, 5, 1, 'same', 'fp32', 'direct', 'pipe narrow 64'),
    (2, 64, 16, 64, 5, 1, 'same', 'fp32', 'direct', 'pipe narrow 64'),
    (2, 65, 16, 64, 5, 1, 'same', 'fp32', 'direct', 'pipe narrow 64'),
    (4, 4097, 8, 512, 5, 1, 'same', 'fp32', 'direct', 'pipe tall'),
    (4, 4097, 8, 512, 3, 1, 'same', 'fp32', 'direct', 'pipe square'),
    (2, 130, 16, 64, 5, 2, 'same', 'fp32', 'direct', 'pipe narrow 64'),
    (2, 131, 16, 64, 5, 2, 'same', 'fp32', 'direct', 'pipe narrow 64'),
    (2, 130, 16, 64, 5, 2, 'valid', 'fp32', 'direct', 'pipe narrow 64'),
    (2, 131, 16, 64, 5, 2, 'valid', 'fp32', 'direct', 'pipe narrow 64'),
] + [(2, L, 32, 64, 5, 1, 'same', 'wino', 'wino', None) for L in (127, 128, 129, 1, 2, 3)] + [
    (2, L, 32, 64, 5, 2, 'same', 'wino', 'wino_s2', None) for L in (254, 256, 258, 1, 2, 3)] + [
    (2, L, 256, 256, 5, 1, 'same', 'bf16x3', 'bf16x3', None) for L in (127, 128, 129, 255, 256, 257, 1, 2, 3)] + [
    (2, L, 256, 256, 5, 2, 'same', 'bf16x3', 'bf16x3', None) for L in (510, 512, 514)]


def _nonlinear(shape):
    return [('relu', 0.0), ('leaky', 0.2), ('tanh', 0.0)][zlib.crc32(repr(shape).encode()) % 3]


@pytest.mark.parametrize("B,L,Cin,Cout,k,s,padding,math,family,member", FWD, ids=ids(FWD))
def test_forward_inside_guards(worst, B, L, Cin, Cout, k, s, padding, math, family, member):
    """gn_conv1d_fwd with a linear and a non-linear epilogue, with and without a bias, for every member of the direct family and the tile walks
    of wino, wino_s2 and bf16x3.  Worst error / bound on the MI355X: y 0.082 (direct), 0.089 (wino), 0.033 (wino_s2), 0.213 (bf16x3)."""
    from gennet_amd import ops
    shape = (B, L, Cin, Cout, k, s, padding)
    if member is not None:
        Lout = ops.conv_geometry(L, k, s, padding)[0]
        assert conv_member(B, Lout, L, Lout, Cin, Cout, k, s, k) == member, shape
    for ints in ((False, True) if family in EXACT else (False,)):
        c = case_of(shape, ints)
        acts = [INT_ACTS[zlib.crc32(repr(shape).encode()) % 3]] if ints else [('linear', 0.0), _nonlinear(shape)]
        with conv_math(math):
            for i, (act, p) in enumerate(acts):
                bias = ints or i > 0 or L % 2 == 0                            # the linear run of an odd-length case has no bias
                y = CF.run('fwd', family, lambda: c_fwd(c, act, p, bias=bias))
                y_ops = CF.run('fwd', family, lambda: ops.conv1d_fwd(c.plain('x'), c.plain('w'), c.plain('b') if bias else None, s, c.pl, c.Lout, act, p))
                assert torch.equal(y, y_ops), c.tag
                ref = K.act_fwd(c.z if bias else c.z - c.b, act, p)
                exact('y', y, ref, c.tag) if ints else worst.close('y', y, ref, tol_of(family, 'y'), '%s %s' % (c.tag, act))


DROPOUT = [
    (2, 129, 16, 64, 5, 1, 'same', 'fp32', 'direct'), (2, 129, 20, 72, 5, 1, 'same', 'fp32', 'direct'), (2, 131, 16, 64, 5, 2, 'valid', 'fp32', 'direct'),
    (2, 129, 32, 64, 5, 1, 'same', 'fp32', 'direct'), (2, 129, 32, 64, 5, 1, 'same', 'wino', 'wino'),
    (2, 258, 32, 64, 5, 2, 'same', 'fp32', 'direct'), (2, 258, 32, 64, 5, 2, 'same', 'wino', 'wino_s2'),
]


@pytest.mark.parametrize("B,L,Cin,Cout,k,s,padding,math,family", DROPOUT, ids=ids(DROPOUT))
def test_forward_dropout_epilogue_inside_guards(worst, B, L, Cin, Cout, k, s, padding, math, family):
    """gn_conv1d_fwd_dropout (the MODE 1 mask descriptor of ybytes >> 2 bytes; the generic kernel's pointer loads) at rate 0.4 with the mask
    inside a guarded byte buffer: dropped elements exactly zero, the rest against dropout(act(conv)).  Worst error / bound on the MI355X: y 0.084."""
    from gennet_amd import ops
    c = case_of((B, L, Cin, Cout, k, s, padding))
    mask = (_rng('mask', c.shape).rand(B, c.Lout, Cout) >= 0.4).astype(np.uint8)
    assert 0 < mask.sum() < mask.size
    m, md = ByteIn(mask), g(mask, torch.uint8)
    with conv_math(math):
        for act, p in (('leaky', 0.2), ('tanh', 0.0)):
            y = CF.run('fwd', family, lambda: c_fwd(c, act, p, m, 0.4))
            y_ops = CF.run('fwd', family, lambda: ops.conv1d_fwd_dropout(c.plain('x'), c.plain('w'), c.plain('b'), md, s, c.pl, c.Lout, act, p, 0.4))
            assert torch.equal(y, y_ops), c.tag
            assert bool((y[md == 0] == 0).all()), c.tag
            worst.close('y', y, K.dropout_fwd(K.act_fwd(c.z, act, p), mask, 0.4), tol_of(family, 'y'), '%s %s' % (c.tag, act))


STATS = [
    (3, 129, 64, 128, 5, 1, 'same', 'fp32', 'direct'), (3, 129, 64, 128, 5, 1, 'same', 'wino', 'wino'),
    (8, 65, 64, 64, 5, 1, 'same', 'fp32', 'direct'), (8, 65, 64, 64, 5, 1, 'same', 'wino', 'wino'),
    (2, 258, 64, 64, 5, 2, 'same', 'fp32', 'direct'), (2, 258, 64, 64, 5, 2, 'same', 'wino', 'wino_s2'),
    (2, 129, 20, 72, 5, 1, 'valid', 'fp32', 'direct'),
]


@pytest.mark.parametrize("B,L,Cin,Cout,k,s,padding,math,family", STATS, ids=ids(STATS))
def test_forward_with_statistics_inside_guards(worst, B, L, Cin, Cout, k, s, padding, math, family):
    """gn_conv1d_fwd_stats with y, the fp64 sums and an exact-size workspace all guarded: the per-block partials of the 64-row narrow-wave blocks,
    of the transform-domain kernels, and the separate pass behind the generic kernel.  Worst error / bound on the MI355X: y 0.028."""
    from gennet_amd import _lib, ops
    c = case_of((B, L, Cin, Cout, k, s, padding))
    x, w, b = c.nan('x'), c.nan('w'), c.nan('b')
    y, sums = Guarded((B, c.Lout, Cout)), Guarded((2 * Cout,), torch.float64)
    ws = ExactWs(_lib.size('gn_conv1d_fwd_stats_workspace', B, c.Lout, Cout))
    with conv_math(math):
        CF.run('fwd', family, lambda: _lib.call('gn_conv1d_fwd_stats', ops._p(x.t), ops._p(w.t), ops._p(b.t), ops._p(y.t), ops._p(sums.t), ops._p(ws.buf), ws.nb,
                                               B, L, Cin, Cout, k, s, c.pl, c.Lout, ops._stream()))
        y_ops, sums_ops = CF.run('fwd', family, lambda: ops.conv1d_fwd_stats(c.plain('x'), c.plain('w'), c.plain('b'), s, c.pl, c.Lout))
    ws.check('stats ' + c.tag)
    checked('stats ' + c.tag, x, w, b)
    yt, st = y.check('y ' + c.tag), sums.check('sums ' + c.tag)
    assert torch.equal(yt, y_ops) and torch.equal(st, sums_ops), c.tag
    worst.close('y', yt, c.z, tol_of(family, 'y'), c.tag)
    yd = yt.double().reshape(-1, Cout)
    ref = torch.cat([yd.sum(0), (yd * yd).sum(0)]).cpu().numpy()
    assert np.abs(st.cpu().numpy() - ref).max() <= 1e-12 * np.abs(ref).max()          # fp64 sums of the same fp32 values: order only


# ---------------------------------------------------------------------------------------------- data gradient
DGRAD = [
    # B, L, Cin, Cout, k, stride, padding, math, family, members of the direct family (dgrad_members)
    (2, 129, 72, 20, 5, 1, 'same', 'fp32', 'direct', ('generic square',)),
    (2, 65, 64, 16, 5, 1, 'same', 'fp32', 'direct', ('pipe narrow 64',)),
    (2, 513, 4096, 16, 5, 2, 'same', 'fp32', 'merged', ('merged 256 two-set',)),
    (2, 514, 4096, 16, 5, 2, 'same', 'fp32', 'merged', ('merged 256 two-set',)),
    (2, 513, 4096, 16, 5, 2, 'valid', 'fp32', 'merged', ('merged 256 two-set',)),
    (2, 514, 4096, 16, 5, 2, 'valid', 'fp32', 'merged', ('merged 256 two-set',)),
    (2, 259, 4096, 16, 5, 2, 'same', 'fp32', 'merged', ('merged 128 phase-split',)),
    (2, 260, 4096, 16, 5, 2, 'valid', 'fp32', 'merged', ('merged 128 phase-split',)),
    (2, 131, 128, 24, 5, 2, 'same', 'fp32', 'merged', ('merged 64 phase-split',)),
    (2, 130, 128, 24, 5, 2, 'valid', 'fp32', 'merged', ('merged 64 phase-split',)),
    (8, 896, 1024, 16, 5, 2, 'same', 'fp32', 'merged', ('merged 256 two-set',)),                     # CONV_CASES of test_kernels_gpu.py: just inside merge_below ...
    (8, 898, 1024, 16, 5, 2, 'same', 'fp32', 'phases', ('pipe narrow 256', 'pipe narrow 256')),      # ... and just outside
    (2, 77, 32, 64, 5, 2, 'same', 'fp32', 'phases', ('generic tall', 'generic tall')),
    (3, 66, 32, 64, 4, 2, 'same', 'fp32', 'phases', ('generic tall', 'generic tall')),
] + [(2, L, 64, 32, 5, 1, 'same', 'wino', 'wino', None) for L in (127, 128, 129, 1, 2, 3)] + [
    (2, L, 64, 32, 5, 2, 'same', 'wino', 'wino_s2', None) for L in (255, 256, 257, 2, 3)] + [
    (2, 256, 64, 32, 5, 2, 'valid', 'wino', 'wino_s2', None)] + [
    (2, L, 256, 256, 5, 1, 'same', 'bf16x3', 'bf16x3', None) for L in (129, 257)] + [
    (2, L, 256, 256, 5, 2, 'same', 'bf16x3', 'bf16x3', None) for L in (511, 512, 513)]


@pytest.mark.parametrize("B,L,Cin,Cout,k,s,padding,math,family,members", DGRAD, ids=ids(DGRAD))
def test_data_gradient_inside_guards(worst, B, L, Cin, Cout, k, s, padding, math, family, members):
    """gn_conv1d_dgrad: unit stride on direct, wino, bf16x3; stride 2 merged (both block forms, odd and even L, 'same' and 'valid'), in phases,
    on wino_s2 and on the merged bf16x3 form.  Every row of dx comes back finite.
    Worst error / bound on the MI355X: dx 0.029 (direct, merged, phases), 0.036 (wino), 0.013 (wino_s2), 0.054 (bf16x3), 0.545 (bf16x3 merged, at its 2e-6)."""
    from gennet_amd import ops
    shape = (B, L, Cin, Cout, k, s, padding)
    if members is not None:
        Lout, pl = ops.conv_geometry(L, k, s, padding)
        assert dgrad_members(B, L, Cin, Cout, k, s, pl, Lout) == members, shape
    for ints in ((False, True) if family in EXACT else (False,)):
        c = case_of(shape, ints)
        with conv_math(math):
            dx = CF.run('dgrad', family, lambda: c_dgrad(c), s)
            dx_ops = CF.run('dgrad', family, lambda: ops.conv1d_dgrad(c.plain('dy'), c.plain('wt'), L, s, c.pl), s)
        assert torch.equal(dx, dx_ops), c.tag
        exact('dx', dx, c.bwd[0], c.tag) if ints else worst.close('dx', dx, c.bwd[0], tol_of(family, 'dx', s), c.tag)


FUSED = [
    (2, 65, 64, 16, 5, 1, 'same', 'fp32', 'direct'), (2, 129, 64, 32, 5, 1, 'same', 'fp32', 'direct'), (2, 129, 64, 32, 5, 1, 'same', 'wino', 'wino'),
    (2, 131, 128, 24, 5, 2, 'same', 'fp32', 'merged'), (2, 513, 4096, 16, 5, 2, 'same', 'fp32', 'merged'),
    (2, 257, 64, 32, 5, 2, 'same', 'fp32', 'merged'), (2, 257, 64, 32, 5, 2, 'same', 'wino', 'wino_s2'),
]


@pytest.mark.parametrize("B,L,Cin,Cout,k,s,padding,math,family", FUSED, ids=ids(FUSED))
def test_fused_data_gradient_inside_guards(worst, B, L, Cin, Cout, k, s, padding, math, family):
    """gn_conv1d_dgrad_fused with y_prev and mask_prev guarded: MODE 2 through relu and through LeakyReLU, MODE 3 through LeakyReLU and
    Dropout(0.4), on the direct, transform-domain, merged and stride-2 transform-domain kernels.  Worst error / bound on the MI355X: dx 0.026."""
    from gennet_amd import ops
    c = case_of((B, L, Cin, Cout, k, s, padding))
    rng = _rng('fused', c.shape)
    pre = f32(rng.randn(B, L, Cin))
    keep = (rng.rand(B, L, Cin) >= 0.4).astype(np.uint8)
    a, ks = float(np.float32(0.2)), float(np.float32(1.0) / (np.float32(1.0) - np.float32(0.4)))
    slope = np.where(pre > 0, 1.0, a)
    dx_ref = c.bwd[0]
    forms = [(f32(np.maximum(pre, 0.0)), 'relu', 0.0, None, 0.0, dx_ref * (pre > 0)),
             (f32(pre * slope), 'leaky', 0.2, None, 0.0, dx_ref * slope),
             (f32(f32(pre * slope) * keep * ks), 'leaky', 0.2, keep, 0.4, dx_ref * slope * keep * ks)]
    with conv_math(math):
        for y_prev, act, param, mask, rate, ref in forms:
            yp, mk = NanIn(y_prev), (ByteIn(mask) if mask is not None else None)
            dx = CF.run('dgrad', family, lambda: c_dgrad(c, (yp, act, param, mk, rate)), s)
            prev = (g(y_prev), act, param, g(mask, torch.uint8) if mask is not None else None, rate)
            dx_ops = CF.run('dgrad', family, lambda: ops.conv1d_dgrad(c.plain('dy'), c.plain('wt'), L, s, c.pl, prev=prev), s)
            assert torch.equal(dx, dx_ops), c.tag
            if mask is not None:
                assert bool((dx[g(mask, torch.uint8) == 0] == 0).all()), c.tag
            worst.close('dx', dx, ref, tol_of(family, 'dx'), '%s %s %s' % (c.tag, act, 'mask' if mask is not None else ''))


# ---------------------------------------------------------------------------------------------- weight gradient
WGRAD = [
    # B, L, Cin, Cout, k, stride, padding, math, family, member of the direct family (wgrad_member)
    (2, 50, 16, 64, 3, 1, 'same', 'fp32', 'direct', 'reg 64x64 whole'),
    (3, 700, 64, 128, 3, 1, 'same', 'fp32', 'direct', 'reg 32x128 inside'),
    (256, 1, 8, 8, 1, 1, 'valid', 'fp32', 'direct', 'reg 64x64 whole'),
    (2, 45, 64, 128, 2, 1, 'valid', 'fp32', 'direct', 'reg 32x128 whole'),
    (2, 40, 20, 72, 5, 2, 'same', 'fp32', 'direct', 'reg 32x128 whole'),
    (3, 133, 32, 128, 5, 1, 'valid', 'fp32', 'direct', 'pipe 32x128 whole'),
    (256, 1, 64, 64, 5, 1, 'same', 'fp32', 'direct', 'pipe 64x64 whole'),
    (4, 20, 64, 64, 5, 1, 'same', 'fp32', 'direct', 'pipe 64x64 whole'),
    (2, 3, 64, 64, 5, 1, 'same', 'fp32', 'direct', 'pipe 64x64 whole'),
    (2, 3, 64, 64, 5, 1, 'same', 'wino', 'wino', None),
    (2, 1, 64, 64, 5, 1, 'same', 'wino', 'wino', None),
    (3, 133, 64, 128, 5, 1, 'valid', 'fp32', 'direct', 'pipe 64x64 whole'),
    (3, 133, 64, 128, 5, 1, 'valid', 'wino', 'wino', None),
    (3, 700, 64, 128, 5, 1, 'same', 'fp32', 'direct', 'pipe 64x64 inside'),
    (3, 700, 64, 128, 5, 1, 'same', 'wino', 'wino', None),
    (5, 333, 64, 64, 5, 2, 'valid', 'fp32', 'direct', 'pipe 64x64 whole'),
    (5, 333, 64, 64, 5, 2, 'valid', 'wino', 'wino_s2', None),
    (3, 1400, 64, 64, 5, 2, 'valid', 'fp32', 'direct', 'pipe 64x64 inside'),
    (3, 1400, 64, 64, 5, 2, 'valid', 'wino', 'wino_s2', None),
    (2, 150, 64, 128, 5, 2, 'valid', 'wino', 'wino_s2', None),
    (2, 3, 64, 64, 5, 2, 'same', 'wino', 'wino_s2', None),
    (2, 300, 256, 256, 5, 1, 'same', 'bf16x3', 'bf16x3', None),
    (4, 20, 256, 256, 5, 1, 'same', 'bf16x3', 'bf16x3', None),
    (2, 600, 512, 256, 5, 2, 'same', 'bf16x3', 'bf16x3', None),
]


@pytest.mark.parametrize("B,L,Cin,Cout,k,s,padding,math,family,member", WGRAD, ids=ids(WGRAD))
def test_weight_gradient_inside_guards_and_an_exact_size_workspace(worst, B, L, Cin, Cout, k, s, padding, math, family, member):
    """gn_conv1d_wgrad with db wanted and NULL, the partial slabs (and the per-split bias partials behind them) in exactly
    gn_conv1d_wgrad_workspace bytes: register-staged and pipelined direct kernels on both tiles, K-splits of whole batch elements and inside
    them, elements shorter than a chunk, M = 1; wino, wino_s2, bf16x3 at both strides.
    Worst error / bound on the MI355X: dw 0.009, db 0.001 (direct); dw 0.019 (wino), 0.006 (wino_s2); dw 0.018, db 0.005 (bf16x3)."""
    from gennet_amd import _lib, ops
    shape = (B, L, Cin, Cout, k, s, padding)
    if member is not None:
        Lout = ops.conv_geometry(L, k, s, padding)[0]
        got, splits = wgrad_member(B, Lout, Cin, Cout, k)
        assert got == member, (shape, got)
        with conv_math(math):
            nb = _lib.size('gn_conv1d_wgrad_workspace', B, L, Cin, Cout, k, s, Lout)
        assert nb - 256 == max(splits * (k * Cin * Cout * 4 + Cout * 8), _lib.size('gn_bias_grad_workspace', B * Lout, Cout) - 256), (shape, splits)
    for ints in ((False, True) if family in EXACT else (False,)):
        c = case_of(shape, ints)
        with conv_math(math):
            dw, db = CF.run('wgrad', family, lambda: c_wgrad(c))
            dw0, _ = CF.run('wgrad', family, lambda: c_wgrad(c, want_db=False))
            dw_ops, db_ops = CF.run('wgrad', family, lambda: ops.conv1d_wgrad(c.plain('x'), c.plain('dy'), k, s, c.pl))
        assert torch.equal(dw, dw_ops) and torch.equal(db, db_ops) and torch.equal(dw0, dw_ops), c.tag
        if ints:
            exact('dw', dw, c.bwd[1], c.tag); exact('db', db, c.bwd[2], c.tag)
        else:
            worst.close('dw', dw, c.bwd[1], tol_of(family, 'dw'), c.tag); worst.close('db', db, c.bwd[2], tol_of(family, 'db'), c.tag)


# ---------------------------------------------------------------------------------------------- Dense on the matrix-core route
DENSE = [
    # B, in, out, member (conv_member of the 1-tap launch with B = 1, M = the batch)
    (5, 32, 64, 'dma tall'), (129, 64, 128, 'dma square'), (128, 64, 128, 'dma square'), (130, 100, 1024, 'generic square'), (4, 64, 260, 'generic square'),
    (257, 16, 8, 'generic tall'),
]


def _dense_data(B, n_in, n_out, ints):
    rng = _rng('dense', B, n_in, n_out, ints)
    if ints:
        assert n_in * 9 + 4 < 2 ** 24 and n_out * 6 < 2 ** 24 and B * 6 < 2 ** 24
        return (rng.randint(-3, 4, (B, n_in)).astype(np.float64), rng.randint(-3, 4, (n_in, n_out)).astype(np.float64), rng.randint(-4, 5, (n_out,)).astype(np.float64),
                rng.randint(-2, 3, (B, n_out)).astype(np.float64))
    return f32(rng.uniform(-1, 1, (B, n_in))), f32(rng.randn(n_in, n_out) * 0.1), f32(rng.randn(n_out)), f32(rng.randn(B, n_out))


@pytest.mark.parametrize("B,n_in,n_out,member", DENSE, ids=ids(DENSE, 3))
def test_dense_inside_guards_and_an_exact_size_workspace(worst, B, n_in, n_out, member):
    """gn_dense_fwd and gn_dense_bwd (dx wanted and NULL; the transposed kernel, the partial slabs and the bias partials in exactly
    gn_dense_bwd_workspace bytes) on the all-DMA 1-tap kernel (KC 16) and the generic one; exact on integers.
    Worst error / bound on the MI355X: y 0.039, dx 0.104, dw 0.012, db 0.001."""
    from gennet_amd import _lib, ops
    assert n_in % 4 == 0 and n_out % 4 == 0 and n_out > 4
    assert conv_member(1, B, B, B, n_in, n_out, 1, 1, 1) == member
    for ints in (False, True):
        x, w, b, dy = _dense_data(B, n_in, n_out, ints)
        tag = 'dense %s %s' % ((B, n_in, n_out), 'int' if ints else 'real')
        xn, wn, bn, dyn = NanIn(x), NanIn(w), NanIn(b), NanIn(dy)
        act, p = ('relu', 0.0) if ints else ('tanh', 0.0)
        with conv_math('fp32'):
            y = Guarded((B, n_out))
            CF.run('fwd', 'direct', lambda: _lib.call('gn_dense_fwd', ops._p(xn.t), ops._p(wn.t), ops._p(bn.t), ops._p(y.t), B, n_in, n_out, ops.ACT[act], p, ops._stream()))
            checked(tag, xn, wn, bn)
            yt = y.check('y ' + tag)
            assert torch.equal(yt, ops.dense_fwd(g(x), g(w), g(b), act, p)), tag
            ref = K.act_fwd(K.dense_fwd(x, w, b), act, p)
            exact('y', yt, ref, tag) if ints else worst.close('y', yt, ref, RTOL, tag)
            dx_ref, dw_ref, db_ref = K.dense_bwd(x, w, dy)
            dx_ops, dw_ops, db_ops = ops.dense_bwd(g(x), g(w), g(dy), need_dx=True)
            for need_dx in (True, False):
                dx, dw, db = (Guarded((B, n_in)) if need_dx else None), Guarded((n_in, n_out)), Guarded((n_out,))
                ws = ExactWs(_lib.size('gn_dense_bwd_workspace', B, n_in, n_out))
                _lib.call('gn_dense_bwd', ops._p(xn.t), ops._p(wn.t), ops._p(dyn.t), ops._p(dx.t if dx else None), ops._p(dw.t), ops._p(db.t), ops._p(ws.buf), ws.nb,
                          B, n_in, n_out, ops._stream())
                ws.check(tag)
                checked(tag, xn, wn, dyn)
                dwt, dbt = dw.check('dw ' + tag), db.check('db ' + tag)
                assert torch.equal(dwt, dw_ops) and torch.equal(dbt, db_ops), tag
                if need_dx:
                    dxt = dx.check('dx ' + tag)
                    assert torch.equal(dxt, dx_ops), tag
                    exact('dx', dxt, dx_ref, tag) if ints else worst.close('dx', dxt, dx_ref, RTOL, tag)
            if ints:
                exact('dw', dwt, dw_ref, tag); exact('db', dbt, db_ref, tag)
            else:
                worst.close('dw', dwt, dw_ref, RTOL_W, tag); worst.close('db', dbt, db_ref, RTOL_W, tag)


# ---------------------------------------------------------------------------------------------- exact-size workspaces of the direct entry points
@pytest.mark.parametrize("B,L,Cin,Cout", [(2, 129, 32, 64), (2, 3, 8, 64), (3, 300, 64, 128)])
def test_fwd_wino_inside_an_exact_size_workspace(worst, B, L, Cin, Cout):
    """gn_conv1d_fwd_wino: the transformed kernel in exactly gn_conv1d_wino_workspace bytes.  Worst error / bound on the MI355X: y 0.027."""
    from gennet_amd import _lib, ops
    c = case_of((B, L, Cin, Cout, 5, 1, 'same'))
    x, w, b = c.nan('x'), c.nan('w'), c.nan('b')
    y, ws = Guarded((B, L, Cout)), ExactWs(_lib.size('gn_conv1d_wino_workspace', Cin, Cout))
    assert ws.nb == 6 * Cin * Cout * 4
    CF.run('fwd', 'wino', lambda: _lib.call('gn_conv1d_fwd_wino', ops._p(x.t), ops._p(w.t), ops._p(b.t), ops._p(y.t), ops._p(ws.buf), ws.nb, B, L, Cin, Cout, 5, 1, c.pl, L,
                                            ops.ACT['relu'], 0.0, ops._stream()))
    ws.check(c.tag)
    checked(c.tag, x, w, b)
    yt = y.check('y ' + c.tag)
    assert torch.equal(yt, ops.conv1d_fwd_wino(c.plain('x'), c.plain('w'), c.plain('b'), c.pl, L, 'relu')), c.tag
    worst.close('y', yt, K.act_fwd(c.z, 'relu'), RTOL, c.tag)


@pytest.mark.parametrize("B,L,Cin,Cout,k,s,padding", [(2, 300, 64, 128, 5, 1, 'same'), (3, 129, 48, 64, 3, 1, 'same'), (2, 277, 16, 64, 5, 1, 'valid'),
                                                      (2, 514, 32, 64, 5, 2, 'same')])
def test_fwd_bf16x3_inside_an_exact_size_workspace(worst, B, L, Cin, Cout, k, s, padding):
    """gn_conv1d_fwd_bf16x3: the split planes of x (with the zero guard rows 'same' padding reads on both sides) and of w in exactly
    gn_conv1d_bf16x3_workspace bytes, ragged M tiles of the 128-row and the 256-row kernels; exact on integers.
    Worst error / bound on the MI355X: y 0.019."""
    from gennet_amd import _lib, ops
    for ints in (False, True):
        c = case_of((B, L, Cin, Cout, k, s, padding), ints)
        x, w, b = c.nan('x'), c.nan('w'), c.nan('b')
        for act in ('linear', 'relu'):
            y, ws = Guarded((B, c.Lout, Cout)), ExactWs(_lib.size('gn_conv1d_bf16x3_workspace', B, L, Cin, Cout, k))
            CF.run('fwd', 'bf16x3', lambda: _lib.call('gn_conv1d_fwd_bf16x3', ops._p(x.t), ops._p(w.t), ops._p(b.t), ops._p(y.t), ops._p(ws.buf), ws.nb, B, L, Cin, Cout, k, s,
                                                      c.pl, c.Lout, ops.ACT[act], 0.0, 1, ops._stream()))
            ws.check(c.tag)
            checked(c.tag, x, w, b)
            yt = y.check('y ' + c.tag)
            assert torch.equal(yt, ops.conv1d_fwd_bf16x3(c.plain('x'), c.plain('w'), c.plain('b'), s, c.pl, c.Lout, act)), c.tag
            ref = K.act_fwd(c.z, act)
            exact('y', yt, ref, c.tag) if ints else worst.close('y', yt, ref, BF16X3_TOL['y'], '%s %s' % (c.tag, act))


# ---------------------------------------------------------------------------------------------- the conv-math workspace
def test_transform_domain_conv_math_workspace_is_written_up_to_the_transformed_kernel_only(worst):
    """gn_set_conv_math(2, ...) on a buffer of exactly 64 MiB behind which 64 KiB of the pattern follow: a wino forward writes 6 Cin Cout floats,
    a wino_s2 forward 7 Cin Cout, and nothing behind them.  Worst error / bound on the MI355X: y 0.024."""
    from gennet_amd import _lib, ops
    ws = ExactWs(ops.WINO_WS_BYTES)
    try:
        _lib.call('gn_set_conv_math', 2, ops._p(ws.buf), ws.nb)
        for shape, family, slabs in (((2, 129, 32, 64, 5, 1, 'same'), 'wino', 6), ((2, 258, 32, 128, 5, 2, 'same'), 'wino_s2', 7)):
            c = case_of(shape)
            y = CF.run('fwd', family, lambda: c_fwd(c, 'linear', 0.0))
            ws.check(c.tag, slabs * shape[2] * shape[3] * 4)
            worst.close('y', y, c.z, RTOL, c.tag)
            with ops.conv_math('wino'):
                y_ops = ops.conv1d_fwd(c.plain('x'), c.plain('w'), c.plain('b'), shape[5], c.pl, c.Lout)
            _lib.call('gn_set_conv_math', 2, ops._p(ws.buf), ws.nb)
            assert torch.equal(y, y_ops), c.tag
    finally:
        ops.set_conv_math()


def test_split_conv_math_workspace_of_exactly_the_advertised_size(worst):
    """gn_set_conv_math(1, ...) on exactly gn_conv1d_bf16x3_workspace bytes: a forward, a merged stride-2 data gradient (the launch Cout -> Cin
    over Lout rows) and a weight gradient (whose transposed planes, 6 B ceil(M / 32) (40 stride Cin + 32 Cout) + 256 bytes, fit the forward's
    size at this shape) write nothing behind them.  Worst error / bound on the MI355X: y 0.045, dx 0.545, dw 0.015."""
    from gennet_amd import _lib, ops
    try:
        for what, shape in (('fwd', (1, 256, 256, 256, 5, 1, 'same')), ('dgrad', (2, 511, 256, 256, 5, 2, 'same')), ('wgrad', (1, 256, 256, 256, 5, 1, 'same'))):
            B, L, Cin, Cout, k, s, _ = shape
            c = case_of(shape)
            nb = _lib.size('gn_conv1d_bf16x3_workspace', B, c.Lout, Cout, Cin, k) if what == 'dgrad' else _lib.size('gn_conv1d_bf16x3_workspace', B, L, Cin, Cout, k)
            if what == 'wgrad':
                assert 6 * B * _cdiv(c.Lout, 32) * (40 * s * Cin + 32 * Cout) + 256 <= nb
            ws = ExactWs(nb)
            _lib.call('gn_set_conv_math', 1, ops._p(ws.buf), ws.nb)
            if what == 'fwd':
                out = CF.run('fwd', 'bf16x3', lambda: c_fwd(c, 'linear', 0.0))
                worst.close('y', out, c.z, BF16X3_TOL['y'], c.tag)
            elif what == 'dgrad':
                out = CF.run('dgrad', 'bf16x3', lambda: c_dgrad(c), s)
                worst.close('dx', out, c.bwd[0], BF16X3_TOL['dx merged'], c.tag)
            else:
                out = CF.run('wgrad', 'bf16x3', lambda: c_wgrad(c))[0]
                worst.close('dw', out, c.bwd[1], BF16X3_TOL['dw'], c.tag)
            ws.check('%s %s' % (what, c.tag))
            with conv_math('bf16x3'):
                ref = (ops.conv1d_fwd(c.plain('x'), c.plain('w'), c.plain('b'), s, c.pl, c.Lout) if what == 'fwd'
                       else ops.conv1d_dgrad(c.plain('dy'), c.plain('wt'), L, s, c.pl) if what == 'dgrad' else ops.conv1d_wgrad(c.plain('x'), c.plain('dy'), k, s, c.pl)[0])
            assert torch.equal(out, ref), (what, c.tag)
    finally:
        ops.set_conv_math()


# ---------------------------------------------------------------------------------------------- one byte less than advertised
def test_one_byte_less_than_the_advertised_workspace_is_refused_and_nothing_is_written():
    """Every entry point that takes ws_bytes answers GN_EWORKSPACE to one byte less than its size query returns, on the host: no kernel is
    started, the outputs keep their sentinel and the workspace its pattern."""
    from gennet_amd import _lib, ops
    L_ = _lib.lib()
    st = ops._stream()
    B, L, Cin, Cout, k = 2, 64, 64, 64, 5
    c = case_of((B, L, Cin, Cout, k, 1, 'same'))
    x, w, b, dy = c.nan('x'), c.nan('w'), c.nan('b'), c.nan('dy')
    p = ops._p

    def refused(name, size, outs, call):
        ws = ExactWs(size)
        rc = call(ws)
        torch.cuda.synchronize()
        assert rc == _lib.GN_EWORKSPACE, (name, rc, L_.gn_last_error())
        assert ws.untouched() and all(o.untouched() for o in outs), name
        checked(name, x, w, b, dy)

    for math in ('fp32', 'wino'):
        with conv_math(math):
            dw, db = Guarded((k, Cin, Cout)), Guarded((Cout,))
            refused('gn_conv1d_wgrad ' + math, _lib.size('gn_conv1d_wgrad_workspace', B, L, Cin, Cout, k, 1, L), (dw, db),
                    lambda ws: L_.gn_conv1d_wgrad(p(x.t), p(dy.t), p(dw.t), p(db.t), p(ws.buf), ws.nb - 1, B, L, Cin, Cout, k, 1, c.pl, L, st))
            y, sums = Guarded((B, L, Cout)), Guarded((2 * Cout,), torch.float64)
            refused('gn_conv1d_fwd_stats ' + math, _lib.size('gn_conv1d_fwd_stats_workspace', B, L, Cout), (y, sums),
                    lambda ws: L_.gn_conv1d_fwd_stats(p(x.t), p(w.t), p(b.t), p(y.t), p(sums.t), p(ws.buf), ws.nb - 1, B, L, Cin, Cout, k, 1, c.pl, L, st))
    y = Guarded((B, L, Cout))
    refused('gn_conv1d_fwd_wino', _lib.size('gn_conv1d_wino_workspace', Cin, Cout), (y,),
            lambda ws: L_.gn_conv1d_fwd_wino(p(x.t), p(w.t), p(b.t), p(y.t), p(ws.buf), ws.nb - 1, B, L, Cin, Cout, k, 1, c.pl, L, 0, 0.0, st))
    refused('gn_conv1d_fwd_bf16x3', _lib.size('gn_conv1d_bf16x3_workspace', B, L, Cin, Cout, k), (y,),
            lambda ws: L_.gn_conv1d_fwd_bf16x3(p(x.t), p(w.t), p(b.t), p(y.t), p(ws.buf), ws.nb - 1, B, L, Cin, Cout, k, 1, c.pl, L, 0, 0.0, 1, st))
    n_in, n_out = 64, 128
    xd, wd, dyd = NanIn(_rng('d', 0).randn(B, n_in)), NanIn(_rng('d', 1).randn(n_in, n_out)), NanIn(_rng('d', 2).randn(B, n_out))
    dx, dw, db = Guarded((B, n_in)), Guarded((n_in, n_out)), Guarded((n_out,))
    refused('gn_dense_bwd', _lib.size('gn_dense_bwd_workspace', B, n_in, n_out), (dx, dw, db),
            lambda ws: L_.gn_dense_bwd(p(xd.t), p(wd.t), p(dyd.t), p(dx.t), p(dw.t), p(db.t), p(ws.buf), ws.nb - 1, B, n_in, n_out, st))
    checked('gn_dense_bwd', xd, wd, dyd)
