"""tests/philox_ref.py (the reference of tests/test_rng_values_gpu.py) checked on the CPU: against Random123's published known-answer vectors, a
Philox written a second time on python ints, an all-float64 Box-Muller, a scalar loop over the prior's trials, and exact rational arithmetic for
the singly-rounded uniform.  No GPU."""
import math
from fractions import Fraction

import numpy as np
import pytest

import philox_ref as R

# Random123 (kat_vectors, philox4x32 10): counter words, key words, output words
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def _philox_int(counter, seed):
    """Philox4x32-10 once more, on python ints, one counter at a time (no numpy, no uint64 wrap-around to get wrong)."""
    c = [counter & 0xFFFFFFFF, counter >> 32, 0, 0]
    k = [seed & 0xFFFFFFFF, seed >> 32]
    for r in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return c


@pytest.mark.parametrize('ctr,key,out', KAT)
def test_known_answer_vectors(ctr, key, out):
    assert tuple(int(v) for v in R.philox4x32_10(ctr, key)[0]) == out


def test_counter_and_seed_words():
    """(counter, seed) -> (c0, c1, 0, 0), (k0, k1): the first known-answer row is counter 0 under seed 0; the high words matter; the vectorised
    form equals the python-int one, across the 2^32 carry and at the ends of the uint64 range."""
    assert tuple(int(v) for v in R.philox4x32_10(0, 0)[0]) == KAT[0][2]
    cs = [0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 33 + 7, 2 ** 64 - 1]
    for seed in (0, 77, 0x1234567890, 2 ** 64 - 1):
        got = R.philox4x32_10(cs, seed)
        assert got.shape == (len(cs), 4) and got.dtype == np.uint32
        assert [[int(v) for v in row] for row in got] == [_philox_int(c, seed) for c in cs]
        assert [int(v) for v in R.philox4x32_10(7, seed)[0]] != _philox_int(2 ** 33 + 7, seed)                         # c1 is used
    assert _philox_int(5, 0x1234567890) != _philox_int(5, 0x34567890)                                                  # k1 is used
    run = R.philox4x32_10(R.counters(6, 2 ** 32 - 2), 77)
    assert [[int(v) for v in row] for row in run] == [_philox_int(2 ** 32 - 2 + i, 77) for i in range(6)]
    assert [int(v) for v in R.counters(3, 2 ** 64 - 1)] == [2 ** 64 - 1, 0, 1]
    # nine rounds is another function
    assert not np.array_equal(R.philox4x32_10_words((0, 0, 0, 0), (0, 0), rounds=9), R.philox4x32_10_words((0, 0, 0, 0), (0, 0)))


def test_unit_interval_maps():
    w = np.array([0, 0xFF, 0x100, 0x80000000, 0xFFFFFFFF], np.uint32)
    u = R.u01_24(w)
    assert u.dtype == np.float32 and [Fraction(float(v)) for v in u] == [Fraction(int(x) >> 8, 2 ** 24) for x in w]
    hi = np.array([0, 0, 0x80000000, 0xFFFFFFFF], np.uint32); lo = np.array([0, 0x800, 5, 0xFFFFFFFF], np.uint32)
    v = R.u01_53(hi, lo)
    assert v.dtype == np.float64
    for a, b, got in zip(hi, lo, v):
        x = ((int(a) << 32) | int(b)) >> 11
        assert float(got) == (float(x) + 0.5) * 2.0 ** -53 and 0.0 < got <= 1.0
    assert [Fraction(float(t)) for t in v[:2]] == [Fraction(2 * x + 1, 2 ** 54) for x in (0, 1)]                          # exact below 2^52
    assert v[2] == 0.5 and v[3] == 1.0                                  # from 2^52 on x + 0.5 rounds to even: 2^52 + 0.5 -> 2^52, 2^53 - 0.5 -> 2^53


@pytest.mark.parametrize('lo,hi', [(-1.0, 1.0), (0.0, 1.0), (20.0, 35.0), (0.5, 2.0), (0.5, 1.0), (5.0, 95.0)])
def test_uniform_rounding_forms(lo, hi):
    """The two forms agree bit for bit where (hi - lo) u is exact ((0, 1); (-1, 1): 2u); elsewhere they differ by at most one ulp; the fused one
    is the exact rational value rounded once; neither reaches hi."""
    n, seed, off = 4099, 77, 2 ** 32 - 2
    sep, fused = R.uniform(n, lo, hi, seed, off)
    assert sep.dtype == fused.dtype == np.float32 and sep.shape == fused.shape == (n,)
    if (lo, hi) in ((-1.0, 1.0), (0.0, 1.0)):
        assert np.array_equal(sep.view(np.int32), fused.view(np.int32))
    else:
        assert (np.abs(sep.astype(np.float64) - fused.astype(np.float64)) <= np.spacing(np.minimum(np.abs(sep), np.abs(fused)))).all()
    assert (sep >= lo).all() and (sep < hi).all() and (fused >= lo).all() and (fused < hi).all()
    u = R.u01_24(R.lane_words(n, seed, off))
    d = Fraction(float(np.float32(np.float32(hi) - np.float32(lo))))
    for k in range(0, n, 13):
        exact = Fraction(lo) + d * Fraction(float(u[k]))
        f = float(fused[k])
        nb = [float(np.nextafter(np.float32(f), np.float32(s))) for s in (-np.inf, np.inf)]
        assert all(abs(Fraction(f) - exact) <= abs(Fraction(x) - exact) for x in nb), (k, f)
        assert abs(Fraction(f) - exact) * 2 <= Fraction(float(np.spacing(np.float32(abs(f)))))


def test_uniform_top_of_the_range():
    """u = 1 - 2^-24 (seed 0, counter 2330056, lane 2): lo + (hi - lo) u rounds to hi for (20, 35) and (0.5, 1) in either form; the restatement
    returns the largest float below hi, and leaves every other value alone."""
    c, lane = 2330056, 2
    assert int(R.philox4x32_10(c, 0)[0, lane]) >> 8 == 0xFFFFFF
    for lo, hi in [(-1.0, 1.0), (0.0, 1.0), (20.0, 35.0), (0.5, 1.0), (5.0, 95.0)]:
        for v in R.uniform(4, lo, hi, 0, c):
            assert (v < hi).all() and (v >= lo).all()
            assert v[lane] == np.nextafter(np.float32(hi), np.float32(lo)) or (lo, hi) in ((-1.0, 1.0), (5.0, 95.0))
    u = np.float32(1.0) - np.float32(2.0 ** -24)
    for lo, hi in [(20.0, 35.0), (0.5, 1.0)]:
        assert np.float32(lo) + np.float32(np.float32(hi - lo) * u) == np.float32(hi)                                  # why the clamp exists
        assert np.float32(float(np.float32(hi - lo)) * float(u) + lo) == np.float32(hi)


def test_keep_mask_is_u_ge_rate():
    n, seed, off = 1003, 0x1234567890, 2 ** 33 + 7
    u = R.u01_24(R.lane_words(n, seed, off))
    k = int(np.argsort(u)[n // 5])
    m = R.keep_mask(n, float(u[k]), seed, off)
    assert m.dtype == np.uint8 and m[k] == 1 and m.sum() == (u >= u[k]).sum() == n - n // 5
    assert R.keep_mask(n, 0.0, seed, off).all()


def test_normal_against_an_all_float64_box_muller():
    """The same draw with NOTHING in float32: u2 = k / 2^24 and t = 2 pi u2 in float64.  normal() differs only through its float32 angle
    t32 = fl32(fl32(2 pi) u2):  |t32 - t| <= |fl32(2 pi) - 2 pi| u2 + 2^-24 fl32(2 pi) u2   (constant error + one rounding, half an ulp relative),
    and |d(rad cos t)|, |d(rad sin t)| <= rad |dt|.  So per element |z - z64| <= sd rad u2 (1.75e-7 + 3.75e-7) <= 3.2e-6 sd (rad <= sqrt(48 ln 2))."""
    n, seed, off, mean, sd = 4099, 2 ** 64 - 1, 2 ** 32 - 2, 0.0, 0.5
    z = R.normal(n, mean, sd, seed, off)
    w = R.philox4x32_10(R.counters((n + 3) // 4, off), seed).astype(np.float64).reshape(-1, 2, 2)
    k = np.floor(w / 256.0)
    u1, u2 = 1.0 - k[:, :, 0] / 2.0 ** 24, k[:, :, 1] / 2.0 ** 24
    rad = np.sqrt(-2.0 * np.log(u1))
    z64 = mean + sd * np.stack([rad * np.cos(2.0 * np.pi * u2), rad * np.sin(2.0 * np.pi * u2)], axis=-1).reshape(-1)[:n]
    two_pi32 = float(np.float32(6.283185307179586))
    dt = abs(two_pi32 - 2.0 * np.pi) * u2 + 2.0 ** -24 * two_pi32 * u2
    bound = (sd * np.stack([rad * dt, rad * dt], axis=-1).reshape(-1)[:n]) * (1 + 1e-9) + 1e-15
    err = np.abs(z - z64)
    assert (err <= bound).all(), (err - bound).max()
    assert bound.max() <= 3.2e-6 * sd and err.max() > 1e-9 * sd           # the bound is tight enough to mean something, and the rounding is there
    assert abs(z.mean() - mean) < 5 * sd / np.sqrt(n) and abs(z.std() - sd) < 5 * sd / np.sqrt(2 * n)
    # layout: the odd tail takes the first elements of the last counter
    assert np.array_equal(R.normal(5, mean, sd, seed, off), z[:5])
    assert np.array_equal(R.normal(8, mean, sd, seed, off + 1), z[4:12])


def test_fp64_normal_layouts():
    """normals_fd and normals_chain draw the same pairs and place them differently; both against a scalar loop on python floats."""
    nb, Nf, seed, off = 2, 5, 0x1234567890, 2 ** 32 - 3
    fd, ch = R.normals_fd(nb, Nf, seed, off), R.normals_chain(nb, Nf, seed, off)
    assert fd.shape == ch.shape == (nb, 2 * Nf)
    for b in range(nb):
        for p in range(Nf):
            w = _philox_int(off + b * Nf + p, seed)
            u1 = (float(((w[0] << 32) | w[1]) >> 11) + 0.5) * 2.0 ** -53
            u2 = (float(((w[2] << 32) | w[3]) >> 11) + 0.5) * 2.0 ** -53
            rad = math.sqrt(-2.0 * math.log(u1))
            pair = (rad * math.cos(2.0 * math.pi * u2), rad * math.sin(2.0 * math.pi * u2))
            assert np.allclose([ch[b, p], ch[b, Nf + p]], pair, rtol=0, atol=1e-14)
            for e in range(2):
                v = 2 * p + e
                want = 0.0 if v in (0, Nf) else pair[e]
                assert abs(fd[b, v] - want) <= 1e-14
    assert (fd[:, 0] == 0).all() and (fd[:, Nf] == 0).all()


def test_prior_accepts_the_first_trial_that_obeys_the_rule():
    nb, seed, counter, lo, hi = 8, 0xABCDEF0123, 2 ** 32 + 11, 100, 357
    p = R.prior(nb, seed, counter, lo, hi)
    eta = p.m1 * p.m2 / (p.m1 + p.m2) ** 2
    mc = (p.m1 + p.m2) * eta ** 0.6
    assert ((p.m1 + p.m2 < 100) & (p.m1 > 5) & (p.m2 > 5) & (p.m1 >= p.m2) & (p.m2 / p.m1 >= 0.5) & (mc >= 20) & (mc <= 35)).all()
    assert np.array_equal(mc, p.mc) and np.array_equal(p.m2 / p.m1, p.q) and (p.idx >= lo).all() and (p.idx < hi).all()
    assert (p.trial >= 0).all() and p.trial.max() > 0 and (p.margin > 0).all()
    lmin, lspan = math.log(5.0), math.log(95.0) - math.log(5.0)
    for b in range(nb):                                                 # a scalar loop on python floats: stop at the first accepted trial
        for t in range(1024):
            w = _philox_int(counter + b * 1024 + t, seed)
            x1, x2 = (math.exp(lmin + (w[i] + 0.5) / 2.0 ** 32 * lspan) for i in (0, 1))
            e = x1 * x2 / (x1 + x2) ** 2
            m = (x1 + x2) * e ** 0.6
            if x1 + x2 < 100 and x1 > 5 and x2 > 5 and x1 >= x2 and x2 / x1 >= 0.5 and 20 <= m <= 35:
                break
        assert t == p.trial[b] and p.idx[b] == lo + ((w[2] * (hi - lo)) >> 32)
        assert abs(x1 - p.m1[b]) <= 1e-14 * x1 and abs(x2 - p.m2[b]) <= 1e-14 * x2
    # an empty window gives idx_lo; a rule nothing can satisfy gives the kernel's fallback
    assert (R.prior(3, seed, counter, 40, 40).idx == 40).all()
    none = R.prior(2, seed, counter, lo, hi, m_min=60.0, trials=64)
    assert (none.trial == -1).all() and (none.m1 == 36.0).all() and (none.m2 == 29.0).all() and (none.idx == lo).all()
