"""GPU parity of keras layers.Attention: csrc/attention.hip through the C ABI and ops.attention_fwd / attention_bwd against the fp64 definition
tests/attention_ref.py (itself checked against a triple loop and torch autograd in tests/test_attention_cpu.py), and the layer at model level against
torch fp64 autograd on the CPU.

Section 1, kernel level.  BQ = 128 rows a block owns and BK = 64 rows a staged tile holds come from the library's header.  Inputs sit in
NaN-surrounded buffers, outputs in sentinel-filled ones; a view starts 144 bytes in (pad 36: 16-byte aligned, the 16-byte loads where the row length
is a multiple of 4) or 148 bytes in (pad 37: the guarded 4-byte loads).

THE BOUND of the parity and stability tests is not a constant: in the same test the same operands go through the composed path the README offered
before -- ops.bmm (q . k^T) -> ops.softmax_fwd -> ops.bmm (p . v) and its backward, scale folded into q -- and its largest error against fp64
is measured per tensor.  The fused kernels may exceed it by a factor of 4, plus a floor of 4 ulp (4 * 2^-23) of the tensor's largest reference
magnitude.  The margin: the running maximum adds one rescaling of the accumulator and of the row sum per key tile, two extra roundings per tile on a
chain of Tk terms; the floor covers tensors the composed path gets exactly (Tk = 1: out = v).  A causal case takes the bound of its non-causal
twin (the same operands).  Two tensors have no composed counterpart: lse takes the bound of the composed scores, and the scale gradient, one
number, that of sum (dS * q k^T) formed from the composed path's dS and summed by ops.bias_grad -- with the floor on the magnitude of its terms, the
one departure from "the tensor's largest magnitude"; magnitudes() gives the reason and the figures under both definitions.  The measured ratios are
printed.

Section 2, model level: the logic and bounds of tests/test_dot_gpu.py's train_and_compare as they stand, over three SGD steps."""
import os

import numpy as np
import pytest
import torch

import attention_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5
ULP = 2.0 ** -23
FACTOR, FLOOR = 4.0, 4.0 * ULP


def dev():
    return torch.device('cuda:0')


def tiles():
    from gennet_amd import ops
    return ops.ATTENTION_BQ, ops.ATTENTION_BK, ops.ATTENTION_MAX_D


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
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def run_fused(q, k, v, dout, scale, causal, pad):
    """forward (training phase) and backward through the C ABI on guarded buffers -> dict of numpy arrays"""
    from gennet_amd import _lib
    B, Tq, d = q.shape
    Tk, dv = v.shape[1], v.shape[2]
    gq, gk, gv, gd = (Guarded(t.shape, t, pad) for t in (q, k, v, dout))
    sc = torch.tensor([scale], dtype=torch.float32, device=dev()) if scale is not None else None
    out, lse = Guarded((B, Tq, dv), None, pad), Guarded((B, Tq), None, pad)
    s = torch.cuda.current_stream().cuda_stream
    psc = sc.data_ptr() if sc is not None else None
    _lib.call('gn_attention_fwd', gq.t.data_ptr(), gk.t.data_ptr(), gv.t.data_ptr(), psc, out.t.data_ptr(), lse.t.data_ptr(), B, Tq, Tk, d, dv, int(causal), s)
    what = 'attention %r causal=%d pad %d' % ((B, Tq, Tk, d, dv), causal, pad)
    res = dict(out=out.check(what + ' out'), lse=lse.check(what + ' lse'))
    dq, dk, dvv, rows = Guarded(q.shape, None, pad), Guarded(k.shape, None, pad), Guarded(v.shape, None, pad), Guarded((B * Tq,), None, pad)
    ws = torch.empty(_lib.size('gn_attention_workspace', B, Tq), dtype=torch.uint8, device=dev())
    _lib.call('gn_attention_bwd', gq.t.data_ptr(), gk.t.data_ptr(), gv.t.data_ptr(), psc, out.t.data_ptr(), lse.t.data_ptr(), gd.t.data_ptr(),
              dq.t.data_ptr(), dk.t.data_ptr(), dvv.t.data_ptr(), rows.t.data_ptr(), ws.data_ptr(), ws.numel(), B, Tq, Tk, d, dv, int(causal), s)
    res.update(dq=dq.check(what + ' dq'), dk=dk.check(what + ' dk'), dv=dvv.check(what + ' dv'), dscale_rows=rows.check(what + ' dscale rows'))
    res['dscale'] = res['dscale_rows'].astype(np.float64).sum()
    return res


def run_composed(q, k, v, dout, scale):
    """the non-causal composed path: bmm -> softmax -> bmm and its backward, scale folded into q"""
    from gennet_amd import ops
    tq, tk, tv, td = (torch.tensor(t, device=dev()) for t in (q, k, v, dout))
    B, Tq, Tk = q.shape[0], q.shape[1], k.shape[1]
    sc = 1.0 if scale is None else float(np.float32(scale))
    qs = (tq * sc).contiguous()
    view = (B * Tq, Tk, 1)
    s = ops.bmm(qs, tk, trans_b=True)
    p = ops.softmax_fwd(s, view)
    out = ops.bmm(p, tv)
    dvv = ops.bmm(p, td, trans_a=True)
    dp = ops.bmm(td, tv, trans_b=True)
    ds = ops.softmax_bwd(dp, p, view)
    dq = ops.bmm(ds, tk) * sc
    dk = ops.bmm(ds, qs, trans_a=True)
    raw = ops.bmm(tq, tk, trans_b=True)
    rows = (ds * raw).sum(-1).reshape(-1, 1).contiguous()
    dscale = ops.bias_grad(rows)
    return dict(out=out.cpu().numpy(), dq=dq.cpu().numpy(), dk=dk.cpu().numpy(), dv=dvv.cpu().numpy(), dscale=float(dscale.cpu().numpy()[0]),
                scores=s.cpu().numpy())


def abserr(got, ref):
    return float(np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64)).max())


def relerr(got, ref):
    return abserr(got, ref) / max(float(np.abs(np.asarray(ref, np.float64)).max()), 1e-30)


def magnitudes(q, k, v, dout, sc, ref):
    """the largest magnitude of each reference tensor, with ONE exception, the scale gradient.  It is a single number, sum_ij dS (q . k), and a sum that
    cancels (sum_j dS[i, j] = 0 for every row): the error of such a sum in fp32, in any order, scales with the sum of the magnitudes of its terms,
    not with its result (Higham, Accuracy and Stability, (4.4): |error| <= gamma_n sum |terms|), and the composed path has no scale gradient, so the
    "composed error" of it (run_composed: the composed dS times q k^T, summed) is one draw of that noise, not a maximum over a tensor.  Its magnitude
    for the floor is therefore 'dscale_terms' = sum_ij p (|dP| + |delta|) |q . k|, the terms as the kernels form them.  Measured under the plain
    definition (|dscale| itself, 'dscale' below, printed with every case and asserted nowhere): 10 of the 35 parity cases exceed the bound, the worst
    5.67 times, the median fused / composed error 1.7; with the terms' magnitude the worst case is 0.33 of the bound."""
    q, k, v, dout = (np.asarray(t, np.float64) for t in (q, k, v, dout))
    raw = np.abs(np.einsum('bic,bjc->bij', q, k))
    dp = np.abs(np.einsum('bic,bjc->bij', dout, v))
    _, _, p = R.forward(q, k, v, sc, False)
    delta = np.abs((dout * ref['out']).sum(-1, keepdims=True))
    big = lambda t: float(np.abs(t).max())          # noqa: E731
    return dict(out=big(ref['out']), scores=sc * raw.max(), dv=big(ref['dv']), dq=big(ref['dq']), dk=big(ref['dk']), dscale=abs(ref['dscale']),
                dscale_terms=float((p * (dp + delta) * raw).sum()))


def check_against_the_composed_path(q, k, v, dout, scale, causal, pad, what):
    sc = 1.0 if scale is None else float(np.float32(scale))
    plain_out, plain_lse, _ = R.forward(q, k, v, sc, False)
    plain = R.backward(q, k, v, dout, sc, False)
    plain.update(out=plain_out, lse=plain_lse, scores=sc * np.einsum('bic,bjc->bij', q.astype(np.float64), k.astype(np.float64)))
    comp = run_composed(q, k, v, dout, scale)
    mag = magnitudes(q, k, v, dout, sc, plain)
    bound = dict((name, FACTOR * abserr(comp[name], plain[name]) + FLOOR * mag[name]) for name in ('out', 'dq', 'dk', 'dv', 'dscale', 'scores'))
    strict = bound['dscale']
    bound['dscale'] = FACTOR * abserr(comp['dscale'], plain['dscale']) + FLOOR * mag['dscale_terms']          # magnitudes() says why
    bound['lse'] = bound['scores']
    ref_out, ref_lse, _ = R.forward(q, k, v, sc, causal)
    ref = R.backward(q, k, v, dout, sc, causal)
    ref.update(out=ref_out, lse=ref_lse)
    got = run_fused(q, k, v, dout, scale, causal, pad)
    worst = {}
    for name in ('out', 'lse', 'dq', 'dk', 'dv', 'dscale'):
        assert np.isfinite(np.asarray(got[name])).all(), (what, name)
        err = abserr(got[name], ref[name])
        worst[name] = err / bound[name] if bound[name] > 0 else (0.0 if err == 0 else float('inf'))      # a reference of exactly 0: err <= bound is err == 0
        m = max(mag['scores' if name == 'lse' else name], 1e-300)
        print(what, name, 'fused err %.3g, composed err %.3g (of the largest magnitude), fused / bound %.3g, fused / composed %.3g'
              % (err / m, (bound[name] / m - FLOOR) / FACTOR, worst[name], err / max((bound[name] - FLOOR * m) / FACTOR, 1e-300)))
    print(what, 'dscale with the floor on |dscale| itself (not asserted): fused / bound %.3g' % (abserr(got['dscale'], ref['dscale']) / max(strict, 1e-300)))
    assert all(w <= 1.0 for w in worst.values()), (what, worst)
    return got, ref


# (B, Tq, Tk, d, dv, causal, scale, pad): every Tq of {1, BQ-1, BQ, BQ+1, 2BQ+3}, every Tk of {1, BK-1, BK, BK+1, 3BK+5}, every (d, dv) of the list
# and the limit, B 1 and 3, both alignments, causal with Tq <, = and > Tk
def parity_cases():
    BQ, BK, MAXD = tiles()
    tq = [1, BQ - 1, BQ, BQ + 1, 2 * BQ + 3]
    tk = [1, BK - 1, BK, BK + 1, 3 * BK + 5]
    dd = [(1, 1), (3, 5), (4, 20), (20, 4), (64, 64), (128, 96), (MAXD, MAXD)]
    cases = []
    n = 0
    for a in tq:                                   # 25 non-causal cases: the full product of Tq and Tk, the rest cycling
        for b in tk:
            d, dv = dd[n % len(dd)]
            cases.append((1 if n % 2 else 3, a, b, d, dv, False, None if n % 3 else 0.7, 37 if n % 4 < 2 else 36))
            n += 1
    for a, b in [(1, 1), (BQ - 1, 3 * BK + 5), (BQ, BK - 1), (2 * BQ + 3, 3 * BK + 5), (BQ + 1, BK + 1), (BQ, BQ), (2 * BQ + 3, 2 * BQ + 3), (BK + 1, BK + 1),
                 (1, BK + 1), (2 * BQ + 3, 1)]:
        d, dv = dd[n % len(dd)]
        cases.append((1 if n % 2 else 3, a, b, d, dv, True, None if n % 3 else 0.7, 37 if n % 4 < 2 else 36))
        n += 1
    return cases


def case_id(c):
    return 'b%d-tq%d-tk%d-d%d-dv%d-%s-%s-pad%d' % (c[0], c[1], c[2], c[3], c[4], 'causal' if c[5] else 'full', 'scale' if c[6] else 'unit', c[7])


def test_the_cases_cover_the_set():
    BQ, BK, MAXD = tiles()
    C = parity_cases()
    assert (BQ, BK, MAXD) == (128, 64, 128) and len(C) == 35
    assert set(c[1] for c in C if not c[5]) == {1, BQ - 1, BQ, BQ + 1, 2 * BQ + 3} and set(c[2] for c in C if not c[5]) == {1, BK - 1, BK, BK + 1, 3 * BK + 5}
    assert set((c[3], c[4]) for c in C) == {(1, 1), (3, 5), (4, 20), (20, 4), (64, 64), (128, 96), (MAXD, MAXD)}
    assert set(c[0] for c in C) == {1, 3} and set(c[7] for c in C) == {36, 37} and set(c[6] for c in C) == {None, 0.7}
    causal = [c for c in C if c[5]]
    assert any(c[1] < c[2] for c in causal) and any(c[1] == c[2] for c in causal) and any(c[1] > c[2] for c in causal)
    assert any(c[7] == 36 and c[3] % 4 == 0 and c[4] % 4 == 0 for c in C) and any(c[7] == 36 and c[3] % 4 for c in C)


@pytest.mark.parametrize('case', parity_cases(), ids=case_id)
def test_forward_and_all_gradients_against_fp64_within_the_composed_bound(case):
    B, Tq, Tk, d, dv, causal, scale, pad = case
    rng = np.random.RandomState(Tq * 1000 + Tk * 10 + d + dv)
    q, k, v, dout = (rng.randn(*s).astype(np.float32) for s in ((B, Tq, d), (B, Tk, d), (B, Tk, dv), (B, Tq, dv)))
    got, ref = check_against_the_composed_path(q, k, v, dout, scale, causal, pad, case_id(case))
    if causal:                                     # keys past every query get no gradient at all: exact zeros
        assert not got['dk'][:, Tq:].any() and not got['dv'][:, Tq:].any()


def test_large_scores_and_where_the_maximum_lies():
    """scores from -80 to +80 (a direct exp overflows fp32 at 88.7 and the row sum before that): row 0 ascending in j (its maximum in the last key tile:
    every earlier tile is rescaled), row 1 descending (the maximum in the first tile: every later p underflows to 0), row 2 all scores equal (the
    uniform average of v), row 3 between 0 and 80"""
    BQ, BK, _ = tiles()
    Tk = 3 * BK + 5
    rng = np.random.RandomState(5)
    k = np.zeros((1, Tk, 4), np.float32)
    k[0, :, 0] = np.linspace(-1, 1, Tk)
    k[0, :, 1] = 1.0
    q = np.array([[[80, 0, 0, 0], [-80, 0, 0, 0], [0, 0, 0, 0], [40, 40, 0, 0]]], np.float32)
    v, dout = rng.randn(1, Tk, 6).astype(np.float32), rng.randn(1, 4, 6).astype(np.float32)
    s = np.einsum('bic,bjc->bij', q.astype(np.float64), k.astype(np.float64))
    assert s.max() == 80 and s.min() == -80 and s[0, 0].argmax() == Tk - 1 and s[0, 1].argmax() == 0 and not s[0, 2].any()
    for causal in (False, True):
        got, ref = check_against_the_composed_path(q, k, v, dout, None, causal, 36, 'stability causal=%d' % causal)
    got, _ = check_against_the_composed_path(q, k, v, dout, None, False, 37, 'stability')
    assert np.abs(got['out'][0, 2] - v[0].astype(np.float64).mean(0)).max() <= 4 * Tk * 2.0 ** -24 * np.abs(v).max()      # a sum of Tk equal weights


def fused_ops(q, k, v, dout, scale, causal):
    from gennet_amd import ops
    out, lse = ops.attention_fwd(q, k, v, scale, causal, training=True)
    dq, dk, dv, rows = ops.attention_bwd(q, k, v, out, lse, dout, scale, causal, need_dscale=True)
    return dict(out=out, lse=lse, dq=dq, dk=dk, dv=dv, rows=rows.view(q.shape[0], q.shape[1]))


@pytest.mark.parametrize('causal', [False, True], ids=['full', 'causal'])
def test_a_sample_alone_has_the_bits_it_has_in_the_batch_and_two_runs_agree(causal):
    rng = np.random.RandomState(7)
    B, Tq, Tk, d, dv = 3, 130, 70, 20, 12
    q, k, v, dout = (torch.tensor(rng.randn(*s).astype(np.float32), device=dev()) for s in ((B, Tq, d), (B, Tk, d), (B, Tk, dv), (B, Tq, dv)))
    scale = torch.tensor([0.6], device=dev())
    whole, again = fused_ops(q, k, v, dout, scale, causal), fused_ops(q, k, v, dout, scale, causal)
    for name in whole:
        assert torch.equal(whole[name], again[name]), name
    for b in range(B):
        one = fused_ops(*(t[b:b + 1].contiguous() for t in (q, k, v, dout)), scale, causal)
        for name in whole:
            assert same_bits(one[name][0].cpu().numpy(), whole[name][b].cpu().numpy()), (name, b)
    # the inference phase writes the same out
    from gennet_amd import ops
    out, lse = ops.attention_fwd(q, k, v, scale, causal)
    assert lse is None and torch.equal(out, whole['out'])


def test_causal_rows_do_not_see_the_future_bit_for_bit():
    rng = np.random.RandomState(8)
    B, T, d, dv, cut = 2, 150, 8, 8, 70
    q, k, v, dout = (rng.randn(*s).astype(np.float32) for s in ((B, T, d), (B, T, d), (B, T, dv), (B, T, dv)))
    dv_ = dev()
    base = fused_ops(*(torch.tensor(t, device=dv_) for t in (q, k, v, dout)), None, True)
    k2, v2 = k.copy(), v.copy()
    k2[:, cut + 1:] += rng.randn(B, T - cut - 1, d).astype(np.float32)
    v2[:, cut + 1:] = rng.randn(B, T - cut - 1, dv).astype(np.float32)
    moved = fused_ops(*(torch.tensor(t, device=dv_) for t in (q, k2, v2, dout)), None, True)
    for name in ('out', 'lse', 'dq', 'rows'):               # output rows i <= cut do not depend on keys and values at j > i
        assert torch.equal(base[name][:, :cut + 1], moved[name][:, :cut + 1]), name
    assert not torch.equal(base['out'][:, cut + 1:], moved['out'][:, cut + 1:])
    q2, d2 = q.copy(), dout.copy()
    q2[:, :cut] += rng.randn(B, cut, d).astype(np.float32)
    d2[:, :cut] = rng.randn(B, cut, dv).astype(np.float32)
    moved = fused_ops(*(torch.tensor(t, device=dv_) for t in (q2, k, v, d2)), None, True)
    for name in ('dk', 'dv'):                               # dK[j], dV[j] for j >= cut do not depend on query rows i < cut <= j
        assert torch.equal(base[name][:, cut:], moved[name][:, cut:]), name
        assert not torch.equal(base[name][:, :cut], moved[name][:, :cut])


def test_no_score_matrix_is_allocated():
    """B = 1, Tq = Tk = 4096, d = dv = 8: operands and results are about 1.2 MiB, one (Tq, Tk) tensor would be 64 MiB"""
    rng = np.random.RandomState(9)
    T = 4096
    q, k, v, dout = (torch.tensor(rng.randn(1, T, 8).astype(np.float32), device=dev()) for _ in range(4))
    scale = torch.tensor([0.35], device=dev())
    fused_ops(q[:, :64].contiguous(), k[:, :64].contiguous(), v[:, :64].contiguous(), dout[:, :64].contiguous(), scale, False)      # library and workspace are up
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    got = fused_ops(q, k, v, dout, scale, False)
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated() - before
    print('peak growth over forward + backward: %.2f MiB' % (growth / 2.0 ** 20))
    assert growth < 8 * 2 ** 20
    ref_out, _, _ = R.forward(q.cpu().numpy(), k.cpu().numpy(), v.cpu().numpy(), float(np.float32(0.35)))
    assert relerr(got['out'].cpu().numpy(), ref_out) < 1e-5


def test_bad_arguments_are_errors_and_launch_nothing():
    from gennet_amd import _lib
    B, Tq, Tk, d, dv = 2, 5, 6, 4, 3
    ones = lambda *s: Guarded(s, np.ones(s, np.float32), 36)          # noqa: E731
    q, k, v, o, l, do = ones(B, Tq, d), ones(B, Tk, d), ones(B, Tk, dv), ones(B, Tq, dv), ones(B, Tq), ones(B, Tq, dv)
    outs = [Guarded(s, None, 36) for s in ((B, Tq, dv), (B, Tq), (B, Tq, d), (B, Tk, d), (B, Tk, dv), (B * Tq,), (B * Tq,))]
    out, lse, dq, dk, dvv, rows, ws = outs
    s = torch.cuda.current_stream().cuda_stream
    good = dict(q=q.t.data_ptr(), k=k.t.data_ptr(), v=v.t.data_ptr(), scale=None, out=out.t.data_ptr(), lse=lse.t.data_ptr(), B=B, Tq=Tq, Tk=Tk, d=d, dv=dv,
                o=o.t.data_ptr(), l=l.t.data_ptr(), dout=do.t.data_ptr(), dq=dq.t.data_ptr(), dk=dk.t.data_ptr(), dvv=dvv.t.data_ptr(), rows=rows.t.data_ptr(),
                ws=ws.t.data_ptr(), ws_bytes=4 * B * Tq)

    def fwd(**kw):
        g = dict(good, **kw)
        _lib.call('gn_attention_fwd', g['q'], g['k'], g['v'], g['scale'], g['out'], g['lse'], g['B'], g['Tq'], g['Tk'], g['d'], g['dv'], 0, s)

    def bwd(**kw):
        g = dict(good, **kw)
        _lib.call('gn_attention_bwd', g['q'], g['k'], g['v'], g['scale'], g['o'], g['l'], g['dout'], g['dq'], g['dk'], g['dvv'], g['rows'], g['ws'], g['ws_bytes'],
                  g['B'], g['Tq'], g['Tk'], g['d'], g['dv'], 1, s)

    def refused(text, fn, code=None):
        with pytest.raises(_lib.GennetHipError) as e:
            fn()
        assert '(%d)' % (_lib.GN_EINVAL if code is None else code) in str(e.value) and text in str(e.value), str(e.value)
        assert text in _lib.lib().gn_last_error().decode()
        torch.cuda.synchronize()
        assert all(g.untouched() for g in outs)

    assert _lib.size('gn_attention_workspace', B, Tq) == 4 * B * Tq and _lib.size('gn_attention_workspace', 0, Tq) == 0
    for call, ptrs in ((fwd, ('q', 'k', 'v', 'out')), (bwd, ('q', 'k', 'v', 'o', 'l', 'dout', 'ws'))):
        for name in ptrs:
            refused('null pointer', lambda: call(**{name: None}))
        refused('negative batch size', lambda: call(B=-1))
        for name in ('Tq', 'Tk'):
            refused('at least 1 each', lambda: call(**{name: 0}))
            refused('at least 1 each', lambda: call(**{name: -2}))
        for name in ('d', 'dv'):
            refused('outside 1 .. 128', lambda: call(**{name: 0}))
            refused('outside 1 .. 128', lambda: call(**{name: 129}))
        refused('exceed the grid', lambda: call(B=2 ** 31 - 1, Tq=129, Tk=129))
        call(B=0)                                             # nothing to do is not an error and launches nothing
        call(B=0, q=None, k=None, v=None)
    refused('workspace of 39 bytes, 40 needed', lambda: bwd(ws_bytes=4 * B * Tq - 1), _lib.GN_EWORKSPACE)
    bwd(dq=None, dk=None, dvv=None, rows=None)                # no gradient asked for
    torch.cuda.synchronize()
    assert all(g.untouched() for g in outs)
    fwd()
    bwd()
    torch.cuda.synchronize()
    for g, name in zip(outs[:6], ('out', 'lse', 'dq', 'dk', 'dv', 'rows')):
        g.check(name)


# ---------------------------------------------------------------------------------------------------------------------
# section 2: models against torch fp64 autograd (the logic and bounds of tests/test_dot_gpu.py's train_and_compare, copied as they stand)
# ---------------------------------------------------------------------------------------------------------------------
LR = 0.05


def rel(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-30)


def seed_weights(model, rng):
    """every kernel (Keras' glorot_uniform) and bias (0.1 N(0, 1)) of model.parts from `rng`.  tests/test_dot_gpu.py seeds the biases only and leaves
    the kernels to the process-wide initialiser stream, whose state depends on the tests that ran before; the loss bound of train_and_compare
    (1e-6 relative) is a few fp32 ulp of a loss that is itself a difference, so here the whole model is a function of the seed."""
    for l in model.parts:
        ws = l.get_weights()
        lim = np.sqrt(6.0 / (ws[0].shape[-2] + ws[0].shape[-1]))
        l.set_weights([rng.uniform(-lim, lim, ws[0].shape).astype(np.float32), (0.1 * rng.randn(*ws[1].shape)).astype(np.float32)])


def torch_params(layers):
    return dict((l.name, [torch.tensor(w.astype(np.float64), requires_grad=True) for w in l.get_weights()]) for l in layers if l.weights)


def train_and_compare(model, ref_forward, xs, t, steps=3, what=''):
    """predict, then `steps` SGD train_on_batch steps, against torch fp64 stepping the same way"""
    from gennet_amd.engine import SGD
    model.compile(optimizer=SGD(lr=LR), loss='mean_squared_error')
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
    losses = []
    for step in range(steps):
        for ts in P.values():
            for v in ts:
                v.grad = None
        loss_ref = ((ref_forward(P, *xt) - tt) ** 2).mean()
        loss_ref.backward()
        res = model.train_on_batch(feed, t)
        print(what, 'step', step, 'loss', res[0], float(loss_ref.detach()))
        assert abs(res[0] - float(loss_ref.detach())) <= 1e-6 * abs(float(loss_ref.detach()))
        losses.append(float(loss_ref.detach()))
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
    return P


def conv1(P, layer, x):
    """Conv1D(filters, 1) on channels-last x"""
    return x @ P[layer.name][0][0] + P[layer.name][1]


def dot_attention_model():
    """tests/test_dot_gpu.py's attention_model: the composed Dot -> Softmax -> Dot block"""
    from gennet_amd import layers as Ly
    from gennet_amd.engine import Input, Model
    x = Input((10, 8))
    cq, ck, cv, head = Ly.Conv1D(8, 1), Ly.Conv1D(8, 1), Ly.Conv1D(8, 1), Ly.Dense(1)
    scores = Ly.Dot((2, 2))([cq(x), ck(x)])
    ctx = Ly.Dot((2, 1))([Ly.Softmax(-1)(scores), cv(x)])
    model = Model(inputs=x, outputs=head(Ly.GlobalAveragePooling1D()(Ly.Add()([ctx, x]))))
    model.parts = (cq, ck, cv, head)
    return model


def attention_model(heads=1, **kw):
    """the same block on Attention(**kw)([q, v, k]); heads > 1: (B, T, 8) -> Reshape (T, heads, 8 / heads) -> Permute((2, 1, 3)) and back"""
    from gennet_amd import layers as Ly
    from gennet_amd.engine import Input, Model
    x = Input((10, 8))
    cq, ck, cv, head, att = Ly.Conv1D(8, 1), Ly.Conv1D(8, 1), Ly.Conv1D(8, 1), Ly.Dense(1), Ly.Attention(**kw)

    def split(t):
        return Ly.Permute((2, 1, 3))(Ly.Reshape((10, heads, 8 // heads))(t)) if heads > 1 else t
    ctx = att([split(cq(x)), split(cv(x)), split(ck(x))])
    if heads > 1:
        ctx = Ly.Reshape((10, 8))(Ly.Permute((2, 1, 3))(ctx))
    model = Model(inputs=x, outputs=head(Ly.GlobalAveragePooling1D()(Ly.Add()([ctx, x]))))
    model.parts = (cq, ck, cv, head)

    def ref(P, x):
        def heads_of(t):
            return t.reshape(t.shape[0], 10, heads, 8 // heads).permute(0, 2, 1, 3)
        q, k, v = heads_of(conv1(P, cq, x)), heads_of(conv1(P, ck, x)), heads_of(conv1(P, cv, x))
        s = torch.matmul(q, k.transpose(2, 3))
        if att.use_scale:
            s = s * P[att.name][0]
        if att.causal:
            s = s.masked_fill(~torch.tril(torch.ones(10, 10, dtype=torch.bool)), float('-inf'))
        ctx = torch.matmul(torch.softmax(s, dim=-1), v).permute(0, 2, 1, 3).reshape(x.shape[0], 10, 8)
        return (ctx + x).mean(1) @ P[head.name][0] + P[head.name][1]
    return model, ref, att


def test_the_layer_computes_what_the_composed_block_computes():
    """the same weights in the Dot -> Softmax -> Dot model of tests/test_dot_gpu.py and in the Attention model: the same prediction and the same step"""
    from gennet_amd.engine import SGD
    rng = np.random.RandomState(21)
    old = dot_attention_model()
    seed_weights(old, rng)
    new, _, _ = attention_model()
    for mine, theirs in zip(new.parts, old.parts):            # layer by layer: the two graphs list ck and cv in another order
        mine.set_weights(theirs.get_weights())
    assert [type(n.layer).__name__ for n in new.nodes].count('Attention') == 1 and new.nodes[3].inbound == [0, 1, 2]
    x, t = rng.randn(3, 10, 8).astype(np.float32), rng.randn(3, 1).astype(np.float32)
    assert rel(new.predict(x), old.predict(x)) < 1e-5
    for m in (old, new):
        m.compile(optimizer=SGD(lr=LR), loss='mean_squared_error')
    a, b = old.train_on_batch(x, t), new.train_on_batch(x, t)
    assert abs(a[0] - b[0]) <= 1e-6 * abs(a[0])
    for mine, theirs in zip(new.parts, old.parts):
        for u, w in zip(theirs.get_weights(), mine.get_weights()):
            assert np.abs(u - w).max() <= 1e-5 * max(np.abs(u).max(), 1e-3)


@pytest.mark.parametrize('kw', [dict(), dict(use_scale=True), dict(causal=True), dict(heads=2), dict(use_scale=True, causal=True, heads=2)],
                         ids=['plain', 'use_scale', 'causal', 'two-heads', 'two-heads-scale-causal'])
def test_self_attention_block_trains_as_torch_fp64(kw):
    model, ref, att = attention_model(**kw)
    rng = np.random.RandomState(21)
    seed_weights(model, rng)
    if att.use_scale:
        att.set_weights([np.float32(0.8)])
    if kw.get('heads'):
        assert tuple([n for n in model.nodes if n.layer is att][0].out_shape) == (2, 10, 4)
    P = train_and_compare(model, ref, [rng.randn(3, 10, 8).astype(np.float32)], rng.randn(3, 1).astype(np.float32), what='attention %r' % (kw,))
    if att.use_scale:                              # the scale moved, and where torch moved it (train_and_compare bounded the gradient and the weight)
        assert att.get_weights()[0].shape == () and att.get_weights()[0] != np.float32(0.8)
        assert abs(float(att.get_weights()[0]) - float(P[att.name][0].detach())) < 1e-4


def test_two_inputs_share_key_and_value():
    """Attention()([q, v]): key is value, whose gradient is the sum of both roles"""
    from gennet_amd import layers as Ly
    from gennet_amd.engine import Input, Model
    x = Input((10, 8))
    cq, cv, head = Ly.Conv1D(8, 1), Ly.Conv1D(8, 1), Ly.Dense(1)
    model = Model(inputs=x, outputs=head(Ly.GlobalAveragePooling1D()(Ly.Attention()([cq(x), cv(x)]))))
    model.parts = (cq, cv, head)

    def ref(P, x):
        q, v = conv1(P, cq, x), conv1(P, cv, x)
        return torch.matmul(torch.softmax(torch.matmul(q, v.transpose(1, 2)), dim=-1), v).mean(1) @ P[head.name][0] + P[head.name][1]
    rng = np.random.RandomState(22)
    seed_weights(model, rng)
    train_and_compare(model, ref, [rng.randn(3, 10, 8).astype(np.float32)], rng.randn(3, 1).astype(np.float32), what='attention [q, v]')


def test_save_and_load_round_trip_with_scale(tmp_path):
    from gennet_amd import hostio  # noqa: F401
    from gennet_amd.engine import SGD, load_model
    model, _, att = attention_model(use_scale=True, causal=True)
    rng = np.random.RandomState(26)
    seed_weights(model, rng)
    att.set_weights([np.float32(0.8)])
    x, t = rng.randn(3, 10, 8).astype(np.float32), rng.randn(3, 1).astype(np.float32)
    model.compile(optimizer=SGD(lr=LR), loss='mean_squared_error')
    model.train_on_batch(x, t)
    path = os.path.join(str(tmp_path), 'attention.h5')
    model.save(path)
    again = load_model(path)
    assert [type(n.layer).__name__ for n in again.nodes] == [type(n.layer).__name__ for n in model.nodes]
    assert [n.inbound for n in again.nodes] == [n.inbound for n in model.nodes]
    twin = [n.layer for n in again.nodes if type(n.layer).__name__ == 'Attention'][0]
    assert twin.use_scale and twin.causal and [p.name for p in twin.weights] == [att.name + '/scale']
    assert twin.get_weights()[0] == att.get_weights()[0] != np.float32(0.8)
    assert np.array_equal(model.predict(x), again.predict(x))
    a, b = model.train_on_batch(x, t), again.train_on_batch(x, t)
    assert a == b and all(np.array_equal(u, v) for u, v in zip(model.get_weights(), again.get_weights()))
    # without use_scale the file carries no weight for the layer
    plain, _, _ = attention_model()
    plain.save(path)
    assert not [n.layer for n in load_model(path).nodes if type(n.layer).__name__ == 'Attention'][0].weights


def test_a_captured_step_replays_bit_identically_with_the_live_scale():
    """use_scale=True as a hipGraph (engine.StepGraph): eager step, capture, three replays against four eager steps of a twin.  The kernels read
    scale through a device pointer: a replay that had frozen the captured value would leave the later steps' losses and weights different."""
    from gennet_amd import engine
    from gennet_amd.engine import SGD, to_device
    rng = np.random.RandomState(27)
    x, t = to_device(rng.randn(3, 10, 8).astype(np.float32)), to_device(rng.randn(3, 1).astype(np.float32))
    eager, _, att = attention_model(use_scale=True)
    seed_weights(eager, rng)
    att.set_weights([np.float32(0.8)])
    graphed, _, att_g = attention_model(use_scale=True)
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
    scales = [float(att_g.get_weights()[0])]
    for _ in range(3):
        sg.wait_inputs_consumed()
        stats = sg.replay()
        torch.cuda.synchronize()
        got.append((stats.cpu().numpy().copy(), [w.copy() for w in graphed.get_weights()]))
        scales.append(float(att_g.get_weights()[0]))
    for step, ((s0, w0), (s1, w1)) in enumerate(zip(want, got)):
        assert np.array_equal(s0, s1), (step, s0, s1)
        assert all(np.array_equal(u, v) for u, v in zip(w0, w1)), step
    assert not np.array_equal(want[0][0], want[3][0]) and len(set(scales)) == 4 and scales[0] != 0.8          # the steps differ, and the scale with them
