"""Host restatement of every random draw the library makes on the device (numpy only, vectorised over counters).

The library draws everything from Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC 2011), counter
words (c0, c1, c2, c3) = (counter low, counter high, 0, 0), key (k0, k1) = (seed low, seed high) (gennet_amd/csrc/common.h).  This file writes the
generator down from the paper -- every word is a uint64 that is masked back to 32 bits -- and then each draw as the header documents it.
tests/test_philox_ref_cpu.py checks THIS file (Random123's known-answer vectors, a pure-python-int Philox, an all-float64 Box-Muller, exact
rational arithmetic for the fused rounding); tests/test_rng_values_gpu.py checks the kernels against it.

Layouts
  uniform / keep_mask / normal    element k: counter offset + k // 4, lane k % 4          (fill_uniform, dropout_mask, fill_normal, noise layers)
  normals_fd                      pair p of series b: counter offset + b Nf + p -> positions (2p, 2p + 1) of [re block | im block]   (gn_noise_fd)
  normals_chain                   bin k of row b: counter + b Nf + k -> (re[k], im[k])                                (gn_noise_whitened)
  prior                           trial t of template b: counter + b trials + t                                   (gn_synth_templates_prior)
"""
import functools
from collections import namedtuple

import numpy as np

M32 = np.uint64(0xFFFFFFFF)
_MUL0, _MUL1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)          # the two round multipliers
_WEYL0, _WEYL1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)        # key schedule: golden ratio and sqrt(3) - 1
_S32 = np.uint64(32)
TWO_PI_F32 = np.float32(6.283185307179586)


def _u64(a):
    """uint64 array (at least 1-d) from python ints (up to 2^64 - 1) or an array."""
    if isinstance(a, np.ndarray):
        return np.atleast_1d(a.astype(np.uint64))
    if isinstance(a, (list, tuple)):
        return np.array([int(v) for v in a], dtype=np.uint64)
    return np.array([int(a)], dtype=np.uint64)


def philox4x32_10_words(ctr, key, rounds=10):
    """The full generator: ctr = four arrays (or ints) of 32-bit words, key = two; returns (n, 4) uint32.
    One round (the paper's S-box on two multiplies):  (hi0, lo0) = M0 * c0, (hi1, lo1) = M1 * c2,
        c' = (hi1 ^ c1 ^ k0,  lo1,  hi0 ^ c3 ^ k1,  lo0);    the key is bumped by the Weyl constants between rounds."""
    c0, c1, c2, c3 = np.broadcast_arrays(*[_u64(c) & M32 for c in ctr])
    k0, k1 = [_u64(k) & M32 for k in key]
    for r in range(rounds):
        if r:
            k0 = (k0 + _WEYL0) & M32
            k1 = (k1 + _WEYL1) & M32
        p0, p1 = _MUL0 * c0, _MUL1 * c2                             # both factors < 2^32: the product fits a uint64
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & M32, (p0 >> _S32) ^ c3 ^ k1, p0 & M32
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1).astype(np.uint32)


def philox4x32_10(counter, seed):
    """(n, 4) uint32.  counter, seed: uint64 arrays or python ints -> words (counter & M32, counter >> 32, 0, 0), key (seed & M32, seed >> 32),
    the library's convention; or a 4-tuple of counter words and a 2-tuple of key words (the published known-answer vectors)."""
    if isinstance(counter, tuple):
        assert len(counter) == 4 and isinstance(seed, tuple) and len(seed) == 2
        return philox4x32_10_words(counter, seed)
    c, s = _u64(counter), _u64(seed)
    return philox4x32_10_words((c & M32, c >> _S32, 0, 0), (s & M32, s >> _S32))


def counters(n, offset):
    """offset + 0 .. offset + n - 1 as uint64 (wrapping at 2^64, like the device's uint64_t)."""
    with np.errstate(over='ignore'):
        return np.uint64(int(offset)) + np.arange(n, dtype=np.uint64)


def u01_24(words):
    """float32 in [0, 1): the top 24 bits over 2^24.  Exact (a 24-bit integer times a power of two)."""
    return (np.asarray(words, np.uint32) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def u01_53(hi, lo):
    """float64 in (0, 1]: (x + 0.5) / 2^53 with x the top 53 bits of hi:lo.  x -> float64 and the scaling are exact; x + 0.5 is ONE correctly
    rounded IEEE addition (inexact from x = 2^52 on), the same operation the device performs."""
    x = ((np.asarray(hi).astype(np.uint64) << _S32) | np.asarray(lo).astype(np.uint64)) >> np.uint64(11)
    return (x.astype(np.float64) + 0.5) * 2.0 ** -53


@functools.lru_cache(maxsize=8)
def _lane_words(n4, seed, offset):
    w = philox4x32_10(counters(n4, offset), seed)
    w.setflags(write=False)
    return w


def lane_words(n, seed, offset):
    """The n words of an element-wise draw: element k = lane k % 4 of counter offset + k // 4.  (Cached: several draws share one stream.)"""
    return _lane_words((int(n) + 3) // 4, int(seed), int(offset)).reshape(-1)[:n]


def _fma_f32(a, b, c):
    """float32(a * b + c) rounded ONCE, for float32 arrays.  a * b is exact in float64 (48 bits); the float64 sum is brought to round-to-odd with
    the error term of TwoSum, after which the rounding to float32 (29 bits narrower) is that of the exact sum (Boldo & Melquiond 2008)."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = np.broadcast_to(c.astype(np.float64), p.shape)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    other = np.nextafter(s, np.where(err > 0, np.inf, -np.inf))
    return np.where((err != 0) & even, other, s).astype(np.float32)


def uniform(n, lo, hi, seed, offset):
    """uniform [lo, hi) in float32: min(lo + (hi - lo) u, largest float below hi).  Returns (separately rounded, fused): hi - lo is rounded to
    float32 in both; then either the product and the sum are rounded one after the other, or the sum is rounded once (a fused multiply-add)."""
    lo, hi = np.float32(lo), np.float32(hi)
    u = u01_24(lane_words(n, seed, offset))
    d = np.float32(hi - lo)
    top = np.nextafter(hi, lo)
    sep = (lo + (d * u).astype(np.float32)).astype(np.float32)
    fused = _fma_f32(np.full(u.shape, d, np.float32), u, np.float32(lo))
    return np.minimum(sep, top), np.minimum(fused, top)


def keep_mask(n, rate, seed, offset):
    """uint8 keep-mask: keep iff u >= float32(rate)."""
    return (u01_24(lane_words(n, seed, offset)) >= np.float32(rate)).astype(np.uint8)


def normal(n, mean, sd, seed, offset):
    """float64 restatement of the fp32 Box-Muller: pair e of a counter uses lanes (2e, 2e + 1); u1 = 1 - u(lane 2e) in (0, 1], u2 = u(lane 2e + 1);
    rad = sqrt(-2 ln u1); (rad cos t, rad sin t) -> elements (2e, 2e + 1), t = float32(2 pi) * u2 ROUNDED TO float32 as on the device (the one step
    whose rounding is visible at the output's scale); everything after it in float64.  Returns mean + sd * z in float64."""
    n4 = (int(n) + 3) // 4
    u = u01_24(lane_words(4 * n4, seed, offset)).reshape(n4, 2, 2)
    u1 = (np.float32(1.0) - u[:, :, 0]).astype(np.float64)           # exact in float32
    t = (TWO_PI_F32 * u[:, :, 1]).astype(np.float32).astype(np.float64)
    rad = np.sqrt(-2.0 * np.log(u1))
    z = np.stack([rad * np.cos(t), rad * np.sin(t)], axis=-1).reshape(-1)[:n]
    return float(np.float32(mean)) + float(np.float32(sd)) * z


def _box_muller_f64(w):
    u1, u2 = u01_53(w[..., 0], w[..., 1]), u01_53(w[..., 2], w[..., 3])
    rad = np.sqrt(-2.0 * np.log(u1))
    t = (2.0 * np.pi) * u2
    return rad * np.cos(t), rad * np.sin(t)


def normals_fd(nb, Nf, seed, offset):
    """(nb, 2 Nf) float64, per series [re block | im block]: pair p of series b (counter offset + b Nf + p) gives positions 2p and 2p + 1 of the
    2 Nf values; bin 0 of either block is zero (gn_noise_fd with amp = 1)."""
    w = philox4x32_10(counters(nb * Nf, offset), seed).reshape(nb, Nf, 4)
    a, b = _box_muller_f64(w)
    out = np.stack([a, b], axis=-1).reshape(nb, 2 * Nf)
    out[:, 0] = 0.0
    out[:, Nf] = 0.0
    return out


def normals_chain(nb, Nf, seed, counter):
    """(nb, 2 Nf) float64, per row [re block | im block]: bin k of row b (counter + b Nf + k) gives (re[k], im[k]); bin 0 is drawn like the
    others (the chain discards it later) -- NoiseSynth.draw(want_normals=True)."""
    w = philox4x32_10(counters(nb * Nf, counter), seed).reshape(nb, Nf, 4)
    a, b = _box_muller_f64(w)
    return np.concatenate([a, b], axis=1)


Prior = namedtuple('Prior', 'trial m1 m2 idx mc q margin')


def prior_trials(nb, seed, counter, m_min=5.0, M_max=100.0, trials=1024):
    """All trials of all templates, (nb, trials) each: x1, x2, mc, q, the acceptance flag, the smallest relative distance of the trial to any of
    the seven acceptance boundaries, and lane 2 (the index word)."""
    w = philox4x32_10(counters(nb * trials, counter), seed).reshape(nb, trials, 4)
    lmin = np.log(m_min)
    lspan = np.log(M_max - m_min) - lmin
    x1 = np.exp(lmin + (w[..., 0].astype(np.float64) + 0.5) * 2.0 ** -32 * lspan)
    x2 = np.exp(lmin + (w[..., 1].astype(np.float64) + 0.5) * 2.0 ** -32 * lspan)
    eta = x1 * x2 / ((x1 + x2) * (x1 + x2))
    mc = (x1 + x2) * eta ** 0.6
    q = x2 / x1
    ok = (x1 + x2 < M_max) & (x1 > m_min) & (x2 > m_min) & (x1 >= x2) & (q >= 0.5) & (mc >= 20.0) & (mc <= 35.0)
    dist = np.min([np.abs(x1 + x2 - M_max) / M_max, np.abs(x1 - m_min) / m_min, np.abs(x2 - m_min) / m_min, np.abs(x1 - x2) / x1,
                   np.abs(q - 0.5) / 0.5, np.abs(mc - 20.0) / 20.0, np.abs(mc - 35.0) / 35.0], axis=0)
    return x1, x2, mc, q, ok, dist, w[..., 2]


def prior(nb, seed, counter, idx_lo, idx_hi, m_min=5.0, M_max=100.0, trials=1024):
    """The in-kernel mass prior (csrc/synth_fused.hip): per template the LOWEST accepted trial of its `trials` counters.  A trial draws two
    log-uniform masses x = exp(ln m_min + (word + 0.5) / 2^32 * (ln(M_max - m_min) - ln m_min)) from lanes 0 and 1 and is accepted iff
        x1 + x2 < M_max,  x1 > m_min,  x2 > m_min,  x1 >= x2,  x2 / x1 >= 0.5,  mc >= 20,  mc <= 35      (mc = (x1 + x2) eta^0.6);
    idx = idx_lo + ((lane 2 * (idx_hi - idx_lo)) >> 32).  No accepted trial: trial = -1 and the kernel's fallback (36, 29, idx_lo).
    margin: the template's closest relative distance to ANY of the seven boundaries over the trials up to and including the accepted one --
    below it, a last-bit difference in exp / pow could decide a trial differently."""
    x1, x2, mc, q, ok, dist, w2 = prior_trials(nb, seed, counter, m_min, M_max, trials)
    hit = ok.any(axis=1)
    t = np.where(hit, ok.argmax(axis=1), trials - 1)
    r = np.arange(nb)
    span = max(int(idx_hi) - int(idx_lo), 0)
    idx = int(idx_lo) + ((w2[r, t].astype(np.uint64) * np.uint64(span)) >> _S32).astype(np.int64)
    m1, m2 = np.where(hit, x1[r, t], 36.0), np.where(hit, x2[r, t], 29.0)
    eta = m1 * m2 / ((m1 + m2) * (m1 + m2))
    margin = np.array([dist[b, :t[b] + 1].min() for b in range(nb)])
    return Prior(np.where(hit, t, -1), m1, m2, np.where(hit, idx, int(idx_lo)).astype(np.int32), (m1 + m2) * eta ** 0.6, m2 / m1, margin)
