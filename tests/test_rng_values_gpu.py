"""The VALUE of every random draw the device makes, against tests/philox_ref.py (Philox4x32-10 written down from the paper and tied to Random123's
known-answer vectors by tests/test_philox_ref_cpu.py).  The other RNG tests compare the library with itself (counter ranges tile, fused passes
equal fill_normal / dropout_mask, moments); here a wrong round count, a dropped high word of counter or seed, a wrong Weyl constant, a wrong
shift in u01_24, swapped Box-Muller lanes, `>` for `>=` or an ignored stream base changes a compared value.

Which case reaches what (gennet_amd/csrc: common.h, elementwise.hip for the fills and the dropout mask, noise_layers.hip, bn_dropgen.hip,
synth.hip, noise_chain.h, synth_fused.hip)

Element-wise draws (fill_uniform, dropout_mask, fill_normal: one thread per counter = 4 elements, grid capped at 2048 blocks of 256 = 2^19 threads)
    n 1, 3                  one counter, tail stores only           n 4   one full counter (the mask's dword store), no tail
    n 5                     a full counter and a one-element tail   n 4099   16 blocks + 1 thread, three-element tail
    n 2^21 + 5              2^19 + 2 counters: a second grid-stride trip of two threads, the last with a one-element tail
    offset 0                the published vectors' counter          offset 2^33 + 7   c1 = 2 from the first counter on
    offset 2^32 - 2         c1 changes INSIDE the draw: counters 0 and 1 have c1 = 0, from the third on c1 = 1 (n >= 9 reaches it)
    seed 0, 77              k1 = 0 (0: the known-answer key)        seed 0x1234567890   k1 = 0x12        seed 2^64 - 1   both key words all ones
    Every length runs at (seed 0x1234567890, offset 2^32 - 2): high key word, the carry, and at 2^21 + 5 half a million counters with c1 = 1.
    Every (seed, offset) pair runs at n = 4099.
    dropout_mask            aligned pointer (dword stores) and a byte view 1 byte into a buffer (byte stores, guard bytes checked); rates 0.2, 0.4,
                            0 (all kept) and the exact u of the middle element, which `>=` keeps and `>` would drop
    fill_uniform            (-1, 1), (0, 1): (hi - lo) u exact, bit for bit; (20, 35), (0.5, 2): one of the two rounding forms, the same for all
    fill_normal             mean 0 and sd a power of two: the affine step is exact and the error is the draw's own; sd by value and from device memory;
                            one case with mean -2 (its final rounding adds half an ulp of the result)

Edge words under seed 0 (found by a host search, re-derived here from the restatement before they are used; n = 4 at that offset)
    counter 2330056 lane 2    word >> 8 = 0xFFFFFF: u = 1 - 2^-24, where lo + (hi - lo) u rounds to hi for (20, 35) and (0.5, 1)
    counter 7113731 lane 1    u2 at its maximum (the largest angle)
    counter 38471471 lane 0   u1 = 2^-24: the largest radius sqrt(48 ln 2) = 5.768
    counter 14883995 lane 0   u = 0: u1 = 1, radius 0, both values of the pair exactly the mean; dropped by any positive rate, kept by rate 0

Stream base (gn_set_rng_base: the device word a replayed graph adds to every offset)
    (o, b) = (5, 1000)  plain                (2^32 - 3, 9)   o < 2^32 <= o + b: the sum carries into c1 on the device

fp64 draws
    gn_noise_fd (3, 5)      one block, odd Nf: pair 2 straddles the re / im blocks        (2, 257)   a second block holding ONE pair
                (2, 300)    a second block of 44 pairs; all at offset 2^32 - 3 (the carry falls inside series 0) and a seed with a high word
    NoiseSynth(256, 4)      N = 1024, the smallest fused length (Nf = 513), 3 rows, counter 2^32 + 5, seed with a high word
    templates_prior         256 templates of 1024 trials at (seed 7, counter 0) and at (seed 0x5DEECE66D0000007, counter 2^32 + 12345)

Tolerances: measured worst error x at most 4, under the ceiling the draw's arithmetic allows (figures in the tests' docstrings).
"""
import ctypes

import numpy as np
import pytest
import torch

import philox_ref as R

pytestmark = pytest.mark.gpu

LENGTHS = [1, 3, 4, 5, 4099, (1 << 21) + 5]
SEEDS = [0, 77, 0x1234567890, 2 ** 64 - 1]
OFFSETS = [0, 2 ** 32 - 2, 2 ** 33 + 7]
HOME = (0x1234567890, 2 ** 32 - 2)
CASES = [(n,) + HOME for n in LENGTHS] + [(4099, s, o) for s in SEEDS for o in OFFSETS if (s, o) != HOME]

# Random123 known-answer row 1: Philox4x32-10 of counter (0, 0, 0, 0) under key (0, 0)
KAT0 = (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)
# (counter, lane, word >> 8) under seed 0
EDGE_U_MAX, EDGE_U2_MAX, EDGE_RAD_MAX, EDGE_U_ZERO = (2330056, 2, 0xFFFFFF), (7113731, 1, 0xFFFFFF), (38471471, 0, 0xFFFFFF), (14883995, 0, 0)

# Measured on an MI355X over every case of this file (each test prints its figure), then given a margin of under 4x:
#   fp32 Box-Muller (fill_normal by value / from device memory, gaussian_noise, edge words, stream base): worst |err| / sd 5.74e-7 (n = 2^21 + 5;
#     logf / sqrtf / sincosf and the products at |z| up to 5.2: a few ulp of the value).  Issue ceiling 1e-5; a swapped lane or a wrong u1 gives O(1).
#   fp64 Box-Muller (gn_noise_fd, the noise chain): worst |err| 4.44e-16 = half an ulp of a value in [2, 4).  Ceiling 1e-13.
#   prior masses: worst relative error 2.19e-16 (one ulp of exp).  Ceiling 1e-12.
TOL_NORMAL = 2.0e-6      # |device - restatement| / sd
TOL_NORMAL64 = 1.7e-15   # absolute
TOL_MASS = 8.0e-16       # relative


def _dev():
    return torch.device('cuda:0')


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _np(t):
    return t.cpu().numpy()


def _normal_err(got, n, mean, sd, seed, offset):
    """worst |device - restatement| / sd; with mean != 0 the final fp32 rounding of mean + sd z (half an ulp of the result) is taken off first"""
    ref = R.normal(n, mean, sd, seed, offset)
    got = _np(got).astype(np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all()
    err = np.abs(got - ref)
    if mean != 0.0:
        err = np.maximum(err - 2.0 ** -24 * np.abs(ref) * (1 + 2.0 ** -20), 0.0)
    return float(err.max() / sd)


def test_the_device_reproduces_the_published_vector():
    """seed 0, offset 0, n = 4, (0, 1): exactly (word >> 8) / 2^24 of Random123's first known-answer row -- written out here, not computed."""
    from gennet_amd import ops
    got = _np(ops.fill_uniform((4,), 0.0, 1.0, 0, 0, _dev()))
    assert got.tolist() == [(w >> 8) / 2.0 ** 24 for w in KAT0]


@pytest.mark.parametrize('n,seed,offset', CASES)
def test_fill_uniform(n, seed, offset):
    from gennet_amd import ops
    for lo, hi in ((-1.0, 1.0), (0.0, 1.0)):
        sep, fused = R.uniform(n, lo, hi, seed, offset)
        got = _np(ops.fill_uniform((n,), lo, hi, seed, offset, _dev()))
        assert np.array_equal(_bits(got), _bits(sep)) and np.array_equal(_bits(got), _bits(fused)), (lo, hi)
    for lo, hi in ((20.0, 35.0), (0.5, 2.0)):
        sep, fused = R.uniform(n, lo, hi, seed, offset)
        got = _np(ops.fill_uniform((n,), lo, hi, seed, offset, _dev()))
        assert np.array_equal(_bits(got), _bits(sep)) or np.array_equal(_bits(got), _bits(fused)), (lo, hi)
        assert (got >= lo).all() and (got < hi).all()


def _mask_unaligned(n, rate, seed, offset):
    """gn_dropout_mask on a byte view starting 1 byte into a buffer: the kernel's byte-store path.  -> (mask, guard bytes intact)"""
    from gennet_amd import _lib
    buf = torch.full((n + 9,), 0xAA, dtype=torch.uint8, device=_dev())
    view = buf[1:1 + n]
    assert view.data_ptr() % 4 == 1
    _lib.call('gn_dropout_mask', view.data_ptr(), n, ctypes.c_float(rate), seed, offset, _stream())
    b = _np(buf)
    return b[1:1 + n], b[0] == 0xAA and (b[1 + n:] == 0xAA).all()


@pytest.mark.parametrize('n,seed,offset', CASES)
def test_dropout_mask(n, seed, offset):
    from gennet_amd import ops
    k = n // 2
    u_k = float(R.u01_24(R.lane_words(n, seed, offset))[k])              # the rate at which element k sits ON the boundary: u >= rate keeps it
    for rate in (0.2, 0.4, 0.0, u_k):
        ref = R.keep_mask(n, rate, seed, offset)
        got = _np(ops.dropout_mask((n,), rate, seed, offset, _dev()))
        assert got.dtype == np.uint8 and np.array_equal(got, ref), rate
        got1, intact = _mask_unaligned(n, rate, seed, offset)
        assert np.array_equal(got1, ref) and intact, rate
        if rate == 0.0:
            assert got.all()
    assert ref[k] == 1 and got[k] == 1 and got1[k] == 1


@pytest.mark.parametrize('n,seed,offset', CASES)
def test_fill_normal(n, seed, offset):
    """Measured: worst |device - restatement| / sd = 5.74e-7 over all cases (at n = 2^21 + 5; 2.7e-7 .. 3.9e-7 at n = 4099, 1.9e-7 at the edge words);
    TOL_NORMAL = 2.0e-6 is 3.5x that and a fifth of the 1e-5 ceiling."""
    from gennet_amd import ops
    worst = _normal_err(ops.fill_normal((n,), 0.0, 1.0, seed, offset, _dev()), n, 0.0, 1.0, seed, offset)
    sd_dev = torch.tensor([0.125], dtype=torch.float32, device=_dev())
    worst = max(worst, _normal_err(ops.fill_normal((n,), 0.0, ops.DevScalar(sd_dev.data_ptr()), seed, offset, _dev()), n, 0.0, 0.125, seed, offset))
    if n == 4099:
        worst = max(worst, _normal_err(ops.fill_normal((n,), -2.0, 0.5, seed, offset, _dev()), n, -2.0, 0.5, seed, offset))
    print('fill_normal n %d seed %#x offset %#x: worst |err| / sd %.3e' % (n, seed, offset, worst))
    assert worst <= TOL_NORMAL


def test_edge_words():
    from gennet_amd import ops
    for c, lane, top in (EDGE_U_MAX, EDGE_U2_MAX, EDGE_RAD_MAX, EDGE_U_ZERO):
        assert int(R.philox4x32_10(c, 0)[0, lane]) >> 8 == top, (c, lane)
        z = ops.fill_normal((4,), 0.0, 1.0, 0, c, _dev())
        worst = _normal_err(z, 4, 0.0, 1.0, 0, c)
        print('fill_normal at edge counter %d: worst |err| / sd %.3e, values %s' % (c, worst, _np(z).tolist()))
        assert worst <= TOL_NORMAL
        for rate in (0.0, 2.0 ** -24, 0.2):
            assert np.array_equal(_np(ops.dropout_mask((4,), rate, 0, c, _dev())), R.keep_mask(4, rate, 0, c))
    # the largest radius the fp32 Box-Muller can produce, and the pair that is exactly the mean
    c = EDGE_RAD_MAX[0]
    assert np.hypot(*R.normal(2, 0.0, 1.0, 0, c)) == pytest.approx(np.sqrt(48 * np.log(2.0)), rel=1e-14)
    assert np.hypot(*_np(ops.fill_normal((2,), 0.0, 1.0, 0, c, _dev())).astype(np.float64)) == pytest.approx(np.sqrt(48 * np.log(2.0)), rel=1e-6)
    c = EDGE_U_ZERO[0]
    assert _np(ops.fill_normal((4,), 3.0, 0.5, 0, c, _dev()))[:2].tolist() == [3.0, 3.0]
    assert _np(ops.dropout_mask((4,), 2.0 ** -24, 0, c, _dev()))[0] == 0 and _np(ops.dropout_mask((4,), 0.0, 0, c, _dev()))[0] == 1


@pytest.mark.parametrize('lo,hi', [(-1.0, 1.0), (0.0, 1.0), (20.0, 35.0), (0.5, 1.0), (5.0, 95.0)])
def test_uniform_is_half_open_at_the_top(lo, hi):
    """u = 1 - 2^-24: lo + (hi - lo) u rounds to hi itself for (20, 35) and (0.5, 1), with two roundings as with one; the kernel returns the largest
    float below hi there and leaves every smaller value alone (the bit-for-bit cases of test_fill_uniform)."""
    from gennet_amd import ops
    c, lane, top = EDGE_U_MAX
    assert int(R.philox4x32_10(c, 0)[0, lane]) >> 8 == top
    got = _np(ops.fill_uniform((4,), lo, hi, 0, c, _dev()))
    sep, fused = R.uniform(4, lo, hi, 0, c)
    assert (got < hi).all() and (got >= lo).all(), got.tolist()
    assert np.array_equal(_bits(got), _bits(sep)) or np.array_equal(_bits(got), _bits(fused))
    assert got[lane] == got.max()


def test_gaussian_noise_closes_the_chain():
    """The noise layers are tied to fill_normal / dropout_mask bit for bit elsewhere; one direct case shows the chain ends at the restatement."""
    from gennet_amd import ops
    n, seed, offset = 4099, 2 ** 64 - 1, 2 ** 32 - 2
    y = ops.gaussian_noise(torch.zeros(n, device=_dev()), 0.25, seed, offset)
    assert _normal_err(y, n, 0.0, 0.25, seed, offset) <= TOL_NORMAL


@pytest.mark.parametrize('o,b', [(5, 1000), (2 ** 32 - 3, 9)])
def test_stream_base_is_added_to_every_offset(o, b):
    """With gn_set_rng_base(&b) a draw at offset o is the restatement's draw at o + b, in every kernel that draws; after the reset it is o again."""
    from gennet_amd import ops
    n, seed, rate, C = 1003, 0x1234567890, 0.3, 8
    rows = 126
    base = torch.tensor([b], dtype=torch.int64, device=_dev())
    ones = torch.ones(n, device=_dev())
    x2d = torch.ones((rows, C), device=_dev()); sc = torch.ones(C, device=_dev()); sh = torch.zeros(C, device=_dev())
    torch.cuda.synchronize()
    ops.set_rng_base(base.data_ptr())
    try:
        u = ops.fill_uniform((n,), 0.0, 1.0, seed, o, _dev())
        z = ops.fill_normal((n,), 0.0, 1.0, seed, o, _dev())
        m = ops.dropout_mask((n,), rate, seed, o, _dev())
        g = ops.gaussian_noise(torch.zeros(n, device=_dev()), 0.5, seed, o)
        a = ops.alpha_dropout_fwd(ones, rate, 1.0, 0.0, -1.0, seed, o)      # keep ? 1 : -1
        y, bm = ops.bn_apply_dropgen(x2d, sc, sh, 'linear', 0.0, rate, seed, o)
        torch.cuda.synchronize()
    finally:
        ops.set_rng_base(None)                                          # per host thread: it would leak into every later test
    keep = R.keep_mask(n, rate, seed, o + b)
    assert np.array_equal(_bits(_np(u)), _bits(R.uniform(n, 0.0, 1.0, seed, o + b)[0]))
    assert _normal_err(z, n, 0.0, 1.0, seed, o + b) <= TOL_NORMAL and _normal_err(g, n, 0.0, 0.5, seed, o + b) <= TOL_NORMAL
    assert np.array_equal(_np(m), keep)
    assert np.array_equal(_np(a) > 0, keep.astype(bool))
    keep2 = R.keep_mask(rows * C, rate, seed, o + b).reshape(rows, C)
    assert np.array_equal(_np(bm), keep2) and np.array_equal(_np(y) != 0, keep2.astype(bool))
    assert not np.array_equal(keep, R.keep_mask(n, rate, seed, o))      # the case can tell the two apart
    assert np.array_equal(_np(ops.dropout_mask((n,), rate, seed, o, _dev())), R.keep_mask(n, rate, seed, o))
    assert np.array_equal(_bits(_np(ops.fill_uniform((n,), 0.0, 1.0, seed, o, _dev()))), _bits(R.uniform(n, 0.0, 1.0, seed, o)[0]))


@pytest.mark.parametrize('nb,Nf', [(3, 5), (2, 257), (2, 300)])
def test_noise_fd_normals(nb, Nf):
    """gn_noise_fd with amp = 1.  Measured: worst |device - restatement| = 4.44e-16 over the three shapes (1.1e-16 at (3, 5)); TOL_NORMAL64 = 1.7e-15
    is 3.8x that, ceiling 1e-13."""
    from gennet_amd import _lib
    seed, offset = 0xFEDCBA9876543210, 2 ** 32 - 3
    amp = torch.ones(Nf, dtype=torch.float64, device=_dev())
    X = torch.full((nb, Nf, 2), float('nan'), dtype=torch.float64, device=_dev())
    _lib.call('gn_noise_fd', amp.data_ptr(), X.data_ptr(), nb, Nf, seed, offset, _stream())
    got = _np(X)
    ref = R.normals_fd(nb, Nf, seed, offset)
    assert (got[:, 0, :] == 0.0).all()                                  # the DC bin, exactly
    err = max(np.abs(got[:, :, 0] - ref[:, :Nf]).max(), np.abs(got[:, :, 1] - ref[:, Nf:]).max())
    print('gn_noise_fd (%d, %d): worst |err| %.3e' % (nb, Nf, err))
    assert err <= TOL_NORMAL64


def _psd(fs, T_obs):
    from oracle import synth_ref as S
    return S.analytic_psd(fs * T_obs // 2 + 1, 1.0 / T_obs)


def test_noise_chain_normals():
    """NoiseSynth.draw(want_normals=True) at N = 1024.  Measured: worst |device - restatement| = 4.44e-16; TOL_NORMAL64 = 1.7e-15, ceiling 1e-13."""
    from gennet_amd import templates as T
    nb, seed, counter = 3, 0xFEDCBA9876543210, 2 ** 32 + 5
    ns = T.NoiseSynth(256, 4, _psd(256, 4))
    out, normals = ns.draw(nb, seed, counter, want_normals=True)
    ref = R.normals_chain(nb, ns.Nf, seed, counter)
    got = _np(normals)
    assert got.shape == ref.shape == (nb, 2 * 513) and np.isfinite(_np(out)).all()
    err = np.abs(got - ref).max()
    print('noise chain normals: worst |err| %.3e' % err)
    assert err <= TOL_NORMAL64


# (seed, counter): the restatement alone, on the CPU, finds no template of either batch closer than 1e-9 (relative) to an acceptance boundary
PRIOR_CASES = [(7, 0), (0x5DEECE66D0000007, 2 ** 32 + 12345)]


@pytest.mark.parametrize('seed,counter', PRIOR_CASES)
def test_prior_draws(seed, counter):
    """256 templates drawn inside gn_synth_templates_prior against prior(): the accepted trial's masses, index and labels.  A template that comes
    within 1e-9 (relative) of an acceptance boundary may be decided differently by the device's exp / pow and is left out; at most one may be.
    Measured: worst relative mass error 2.19e-16 (both batches); TOL_MASS = 8.0e-16 is 3.7x that, ceiling 1e-12.  Closest approach to a boundary, from
    the restatement alone: 4.41e-6 at (seed 7, counter 0), 2.29e-5 at (seed 0x5DEECE66D0000007, counter 2^32 + 12345): no template is left out."""
    from gennet_amd import templates as T
    nb, fs, T_obs = 256, 256, 4
    syn = T.Synth(fs, T_obs, _psd(fs, T_obs))
    lo, hi = T.convert_beta([0.45, 0.55], fs, T_obs)
    assert hi > lo
    p = R.prior(nb, seed, counter, lo, hi)
    sure = p.margin >= 1e-9
    print('prior seed %#x counter %d: closest approach to a boundary %.3e, templates left out %d' % (seed, counter, p.margin.min(), (~sure).sum()))
    assert (~sure).sum() <= 1 and (p.trial >= 0).all()
    out, labels, ref, mm, idx = syn.templates_prior(nb, seed, counter, lo, hi, want_params=True)
    mm, idx, labels = _np(mm), _np(idx), _np(labels)
    assert np.array_equal(idx[sure], p.idx[sure])
    e1, e2 = np.abs(mm[:, 0] - p.m1) / p.m1, np.abs(mm[:, 1] - p.m2) / p.m2
    print('prior masses: worst relative error m1 %.3e m2 %.3e' % (e1[sure].max(), e2[sure].max()))
    assert e1[sure].max() <= TOL_MASS and e2[sure].max() <= TOL_MASS
    for got, want in ((labels[:, 0], p.mc), (labels[:, 1], p.q)):
        w32 = want.astype(np.float32)
        assert got.dtype == np.float32 and (np.abs(got.astype(np.float64) - w32.astype(np.float64)) <= np.spacing(w32))[sure].all()
    assert np.isfinite(_np(out)).all()
