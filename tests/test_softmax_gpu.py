"""GPU parity of softmax (csrc/softmax.hip through ops.softmax_fwd / softmax_bwd) against the numpy fp64 definition tests/softmax_ref.py
(itself checked against torch in tests/test_softmax_cpu.py), and of the layers at model level against torch fp64 autograd on the CPU.

Section 1, kernel level.  Inputs sit in NaN-surrounded buffers, outputs in sentinel-filled ones; a view starts 144 bytes in (pad 36: 16-byte
aligned, the float4 columns of `axis`) or 148 bytes in (pad 37: scalar).  The regimes and their seams, as csrc/softmax.hip names them
(`path` below restates them), and the shapes on both sides of each:
    inner == 1   rows: W = min(64, pow2ceil(P)) lanes a row, NJ = pow2ceil(ceil(P / 64)) values a lane: P = 1 | 2 | 3, 4 | 5, 8 | 9, 16 | 17,
                 32 | 33, 63, 64 | 65, 128 | 129, 256 | 257, 512 | 513, 1023, 1024 | 1025 (block, LDS) ... 4095, 4096 | 4097 (stream, 3 tiles)
    inner < 16   split, S = 64 / inner lanes a column in chunks of CH = 4 (P <= 4 S) or 16 positions a lane, a column fits while P <= 16 S:
                 inner 3 (S 21): P = 2, 3, 84 | 85, 336 | 337; inner 4, 5: P = 3, 33; inner 15 (S 4): P = 16 | 17, 64 | 65
    inner >= 16  axis: inner 16 | 15 is the small-inner switch; chunks of 16 positions (float4 columns, inner % 4 == 0 and pad 36: 8):
                 inner 16, 20 (float4 at pad 36, scalar at 37), 17 (scalar): P = 1, 8 | 9, 16 | 17, 33
    outer        1 and 3 everywhere.  Grids are capped at 2048 blocks of 256 lanes and stride beyond; the smallest outer with a second trip:
                 rows: 8192 waves, 64 / W rows a wave, U = 8 / NJ row groups a wave and trip (NJ <= 4): a wave's second group starts at
                 8192 * (64 / W) + 1 rows (8193 at P = 33, 131073 at P = 3, NJ = 2: 8193 at P = 65, NJ = 4: 8193 at P = 129), its second trip at
                 8192 * U * (64 / W) + 1 (65537 at P = 33, 1048577 at P = 3, 32769 at P = 65, 16385 at P = 129; NJ = 8: 8193 at P = 257);
                 block and stream 2049 rows (a block a row); split 8193 (a wave an o); axis 2048 * 256 + 1 columns: scalar inner 17 * outer
                 30841 = 524297, float4 inner 16 (4 columns a lane) * outer 131073 = 524292 lanes.
Inputs: seeded normals times 1 and times 30; rows that mix +-3e38 with normals (exact 0 and 1 / k); rows of one repeated value (bit-identical to
float32(1) / float32(P): every exponential is 1, the sum P exactly, one correctly rounded division); rows with one entry 104.5 .. 124.5 above
the rest (expf is +0 below -103.28: exactly 1 and 0); P = 1 (exactly 1, gradient exactly 0).

Forward bound, against softmax_ref in fp64 on the same fp32 inputs, in units of eps = 2^-23 (a rounding is <= eps / 2 relative):
    |y - r| <= (c + |x - m|) eps r + 2^-126,      c = 3 + (ln P + D) / 2 + R (2 + (ln P) / 2)
  numerator   e = expf(fl(x - m)): expf is <= 1 ulp <= eps (HIP's stated accuracy), the subtraction's rounding (eps / 2) |x - m| goes through
              the exponential as a relative error: (1 + |x - m| / 2) eps; the maximum m is exact in any order
  sum         every term carries (1 + t_j / 2) eps, t_j = |x_j - m|, weighted by its share w_j of the sum; sum_j w_j t_j = H(w) - ln s <= ln P
              (H the entropy of w, s >= 1): (1 + (ln P) / 2) eps; a term passes at most D additions: D eps / 2
  quotient    one correctly rounded division: eps / 2;      total 2.5 + (ln P + D) / 2, and 0.5 for the products of these terms
  rescales    a path that cannot hold the row multiplies its running sum by expf(M_old - M_new) at most R times (once per tile or chunk, whatever
              the data): expf eps, the product eps / 2, its addition is in D, its argument's rounding again sums to <= (ln P) / 2 over a row
  D, R        rows: NJ - 1 + log2 W, 0.  block: ceil(P / 256) - 1 + 8 (a lane's chain, the 6 butterfly steps, 2 for the four waves), 0.
              stream: T = ceil(P / 2048) tiles: 7 + (T - 1) + 8, T - 1.  split / axis: Q = ceil(P / (CH S)) chunks (S = 1 for axis; CH above):
              CH - 1 + (Q - 1) + (S - 1), Q - 1.
Backward bound, from the fp32 y the forward kernel wrote and a seeded dy:
    |dx - r| <= c' eps |y| (|dy| + sum_j |dy_j y_j|),      c' = 2 + D' / 2
  each product dy_j y_j eps / 2, the sum D' eps / 2 of sum |dy_j y_j|, the difference and the last product eps / 2 each of |y| (|dy| + sum):
  1.5 + D' / 2, and 0.5 for the products of these terms.  D' = D except stream, where a lane adds its ceil(P / 256) products in one chain:
  ceil(P / 256) - 1 + 8.  The bound has no floor, so it is asserted where fp32 can meet it: on the y of every input kind but the normals
  times 30, whose y holds denormals (a product with one is rounded to a multiple of 2^-149, which no factor of eps |y| covers); those run
  with the forward's floor 2^-126 added, and that is said here and in DESIGN 8k.
In place (y on x, dx on dy) gives the bits of out of place; two runs give identical bits.

Section 2, model level: the bounds of tests/test_bn_axis_gpu.py's model tests -- predict 1e-5 of the largest output, the loss 1e-6 relative,
gradients and SGD-updated weights 1e-4 of each tensor's largest entry (gradients no finer than 1e-3 of the model's largest gradient entry)."""
import math
import os

import numpy as np
import pytest
import torch

import loss_ref
import softmax_models as M
import softmax_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5
EPS = 2.0 ** -23
FLOOR = 2.0 ** -126


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
        """the surroundings untouched, every element of the view written, no NaN (an element outside an input was read)"""
        edges = torch.cat([self.buf[:self.pad], self.buf[self.pad + self.n:]])
        assert bool((edges == SENTINEL).all()), '%s: wrote outside its output' % what
        assert not bool((self.t == SENTINEL).any()), '%s: output elements left unwritten' % what
        assert not bool(torch.isnan(self.t).any()), '%s: NaN' % what
        return self.t.cpu().numpy()

    def edges_nan(self):
        return bool(torch.isnan(torch.cat([self.buf[:self.pad], self.buf[self.pad + self.n:]])).all())

    def untouched(self):
        return bool((self.buf == SENTINEL).all())


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def pow2ceil(n):
    return 1 << max(0, (int(n) - 1).bit_length())


def path(P, inner, aligned):
    """(regime, D, R, D') of csrc/softmax.hip for a shape: the longest chain of additions, the rescales of the running sum, the backward's chain"""
    if inner == 1:
        if P <= 1024:
            W, NJ = min(64, pow2ceil(P)), pow2ceil(-(-P // 64))
            D = NJ - 1 + int(math.log2(W))
            return 'rows', D, 0, D
        if P <= 4096:
            D = -(-P // 256) - 1 + 8
            return 'block', D, 0, D
        T = -(-P // 2048)
        return 'stream', 7 + (T - 1) + 8, T - 1, -(-P // 256) - 1 + 8
    if inner < 16:
        S = 64 // inner
        CH = 4 if P <= 4 * S else 16
    else:
        S, CH = 1, 8 if (inner % 4 == 0 and aligned) else 16
    Q = -(-P // (CH * S))
    D = CH - 1 + (Q - 1) + (S - 1)
    return ('split' if inner < 16 else 'axis4' if CH == 8 else 'axis1'), D, Q - 1, D


def c_forward(P, D, Rs):
    return 3.0 + (math.log(P) + D) / 2.0 + Rs * (2.0 + math.log(P) / 2.0)


def c_backward(Db):
    return 2.0 + Db / 2.0


KINDS = ('n1', 'n30', 'big', 'same', 'peak')


def make_input(kind, rng, outer, P, inner):
    x = rng.randn(outer, P, inner).astype(np.float32)
    if kind == 'n30':
        x = (30.0 * x).astype(np.float32)
    elif kind == 'big':                    # each column: +3e38 at one or two positions, -3e38 at some, normals elsewhere
        hi = rng.randint(0, P, size=(outer, 1, inner))
        pos = np.arange(P).reshape(1, P, 1)
        x[np.broadcast_to(rng.rand(outer, P, inner) < 0.3, x.shape)] = -3e38
        x[np.broadcast_to(pos == (hi + 1) % P, x.shape) & np.broadcast_to(rng.rand(outer, 1, inner) < 0.5, x.shape)] = 3e38
        x[np.broadcast_to(pos == hi, x.shape)] = 3e38
    elif kind == 'same':
        x = np.broadcast_to((0.37 * rng.randn(outer, 1, inner)).astype(np.float32), x.shape).copy()
    elif kind == 'peak':
        hi = rng.randint(0, P, size=(outer, 1, inner))
        top = (x.max(axis=1, keepdims=True) + 104.5 + 20.0 * rng.rand(outer, 1, inner)).astype(np.float32)
        x = np.where(np.arange(P).reshape(1, P, 1) == hi, top, x).astype(np.float32)
    return x


# (outer, P, inner); every shape runs 144 and 148 bytes in
SHAPES = ([(o, P, 1) for P in (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64, 65, 128, 129, 256, 257, 512, 513, 1023, 1024, 1025, 4095, 4096, 4097)
           for o in ((1, 3) if P in (1, 3, 33, 65, 1025, 4097) else (3,))]
          + [(3, P, 3) for P in (2, 3, 84, 85, 336, 337)] + [(3, 16, 15), (3, 17, 15)] + [(1, 337, 3)] + [(3, P, i) for P in (3, 33) for i in (4, 5)] + [(3, 64, 15), (3, 65, 15), (1, 65, 15)]
          + [(3, P, i) for i in (16, 17, 20) for P in (1, 8, 9, 16, 17, 33)] + [(1, 17, 16), (1, 17, 17)])
SECOND_TRIP = [(8193, 33, 1), (131073, 3, 1), (8193, 65, 1), (8193, 129, 1), (65537, 33, 1), (1048577, 3, 1), (32769, 65, 1), (16385, 129, 1),
               (8193, 257, 1), (2049, 1025, 1), (2049, 4097, 1), (8193, 2, 3), (30841, 2, 17), (131073, 2, 16)]
WORST = {'fwd': (0.0, None), 'fwd_ulp': (0.0, None), 'bwd': (0.0, None)}


def run_case(outer, P, inner, pad, kinds):
    from gennet_amd import ops
    view = (outer, P, inner)
    regime, D, Rs, Db = path(P, inner, pad % 4 == 0)
    c, cb = c_forward(P, D, Rs), c_backward(Db)
    rng = np.random.RandomState((outer * 7919 + P * 31 + inner * 7 + pad) % (2 ** 31))
    for kind in kinds:
        x = make_input(kind, rng, outer, P, inner)
        what = '%s %r pad %d %s' % (regime, view, pad, kind)
        gx = Guarded(x.shape, x, pad)
        gy = Guarded(x.shape, None, pad)
        ops.softmax_fwd(gx.t, view, out=gy.t)
        y = gy.check(what)
        r, m, d = R.softmax_fwd(x, view)
        err, bound = np.abs(y.astype(np.float64) - r), (c + np.abs(d)) * EPS * r + FLOOR
        ratio = float((err / bound).max())
        ulps = float((np.where(r > 2.0 ** -100, (err / (EPS * np.maximum(r, 2.0 ** -100))) - np.abs(d), 0.0)).max())
        print('%-44s forward c %.1f err/bound %.3f, (err / (eps r) - |x - m|) max %.2f' % (what, c, ratio, ulps))
        for key, val in (('fwd', ratio), ('fwd_ulp', ulps)):
            if val > WORST[key][0]:
                WORST[key] = (val, what)
        assert (err <= bound).all(), (what, ratio)
        assert np.isfinite(y).all() and (y >= 0).all() and (y <= 1).all()
        if kind == 'same' or P == 1:
            assert same_bits(y, np.full(x.shape, np.float32(1) / np.float32(P), np.float32)), what
        if kind == 'peak' and P > 1:
            assert same_bits(y, (x == x.max(axis=1, keepdims=True)).astype(np.float32)), what
        if kind == 'big':
            k = (x == np.float32(3e38)).sum(axis=1, keepdims=True)
            assert same_bits(y, np.where(x == np.float32(3e38), np.float32(1) / k.astype(np.float32), np.float32(0))), what
        # two runs, and in place
        gy2 = Guarded(x.shape, None, pad)
        ops.softmax_fwd(gx.t, view, out=gy2.t)
        assert same_bits(gy2.check(what), y), what + ': two runs differ'
        gxi = Guarded(x.shape, x, pad)
        assert ops.softmax_fwd(gxi.t, view, inplace=True).data_ptr() == gxi.t.data_ptr()
        assert same_bits(gxi.t.cpu().numpy(), y) and gxi.edges_nan(), what + ': in place differs'
        # backward from the fp32 y the kernel wrote
        dy = rng.randn(*x.shape).astype(np.float32)
        gdy, gdx = Guarded(x.shape, dy, pad), Guarded(x.shape, None, pad)
        ops.softmax_bwd(gdy.t, gy.t, view, out=gdx.t)
        dx = gdx.check(what + ' backward')
        rb, mag = R.softmax_bwd(dy, y, view)
        berr = np.abs(dx.astype(np.float64) - rb)
        bbound = cb * EPS * np.abs(y.astype(np.float64)) * (np.abs(dy.astype(np.float64)) + mag) + (FLOOR if kind == 'n30' else 0.0)
        bratio = float((berr / np.maximum(bbound, 1e-300)).max()) if (bbound > 0).any() else 0.0
        print('%-44s backward c\' %.1f err/bound %.3f' % (what, cb, bratio))
        if bratio > WORST['bwd'][0] and kind != 'n30':
            WORST['bwd'] = (bratio, what)
        assert (berr <= bbound).all(), (what, bratio)
        if P == 1:
            assert same_bits(dx, np.zeros(x.shape, np.float32)), what             # 1 * (dy - dy * 1): +0
        gdx2 = Guarded(x.shape, None, pad)
        ops.softmax_bwd(gdy.t, gy.t, view, out=gdx2.t)
        assert same_bits(gdx2.check(what), dx), what + ': two backward runs differ'
        assert ops.softmax_bwd(gdy.t, gy.t, view, inplace=True).data_ptr() == gdy.t.data_ptr()
        assert same_bits(gdy.t.cpu().numpy(), dx) and gdy.edges_nan(), what + ': backward in place differs'


@pytest.mark.parametrize('pad', [36, 37])
@pytest.mark.parametrize('outer,P,inner', SHAPES, ids=['%dx%dx%d' % s for s in SHAPES])
def test_both_passes_meet_the_derived_bounds_on_each_side_of_every_seam(outer, P, inner, pad):
    run_case(outer, P, inner, pad, KINDS)


@pytest.mark.parametrize('outer,P,inner', SECOND_TRIP, ids=['%dx%dx%d' % s for s in SECOND_TRIP])
def test_a_second_trip_of_the_grid_stride_loop(outer, P, inner):
    """the smallest outer at which one unit of the capped grid takes a second trip (module docstring), 144 bytes in; normals and the exact rows"""
    run_case(outer, P, inner, 36, ('n1', 'same'))


def test_p_equal_one_is_exactly_one_with_an_exactly_zero_gradient():
    from gennet_amd import ops
    rng = np.random.RandomState(5)
    for inner in (1, 3, 16, 17):
        x = (30 * rng.randn(5, 1, inner)).astype(np.float32)
        y = ops.softmax_fwd(torch.tensor(x, device=dev()), (5, 1, inner))
        dx = ops.softmax_bwd(torch.tensor(rng.randn(5, 1, inner).astype(np.float32), device=dev()), y, (5, 1, inner))
        assert bool((y == 1).all()) and bool((dx == 0).all())


def test_the_entry_points_refuse_and_leave_the_output_untouched():
    from gennet_amd import _lib, ops
    L = _lib.lib()
    x = Guarded((4, 6), np.ones((4, 6), np.float32), 36)
    y = Guarded((4, 6), None, 36)
    s = torch.cuda.current_stream().cuda_stream
    for args in ((None, y.t.data_ptr(), 4, 6, 1, s), (x.t.data_ptr(), None, 4, 6, 1, s), (x.t.data_ptr(), y.t.data_ptr(), 0, 6, 1, s),
                 (x.t.data_ptr(), y.t.data_ptr(), 4, 0, 1, s), (x.t.data_ptr(), y.t.data_ptr(), 4, 6, 0, s), (x.t.data_ptr(), y.t.data_ptr(), 4, -6, 1, s),
                 (x.t.data_ptr(), y.t.data_ptr(), 1, 65536, 32768, s)):
        assert L.gn_softmax_fwd(*args) == _lib.GN_EINVAL and L.gn_last_error().decode().startswith('softmax_fwd: '), args
    for args in ((None, x.t.data_ptr(), y.t.data_ptr(), 4, 6, 1, s), (x.t.data_ptr(), None, y.t.data_ptr(), 4, 6, 1, s),
                 (x.t.data_ptr(), x.t.data_ptr(), None, 4, 6, 1, s), (x.t.data_ptr(), x.t.data_ptr(), y.t.data_ptr(), 4, 6, -1, s),
                 (x.t.data_ptr(), x.t.data_ptr(), y.t.data_ptr(), 1, 65536, 32768, s)):
        assert L.gn_softmax_bwd(*args) == _lib.GN_EINVAL and L.gn_last_error().decode().startswith('softmax_bwd: '), args
    torch.cuda.synchronize()
    assert y.untouched()
    with pytest.raises(ValueError, match='does not cover'):
        ops.softmax_fwd(x.t, (4, 5, 1), out=y.t)
    with pytest.raises(ValueError, match='does not cover'):
        ops.softmax_bwd(x.t, x.t, (2, 6, 1), out=y.t)
    assert y.untouched()
    ops.softmax_fwd(x.t, (4, 6, 1), out=y.t)
    assert same_bits(y.check('after the refusals'), np.full((4, 6), np.float32(1) / np.float32(6)))


def test_zz_report_the_largest_errors_seen():
    """no assertion of its own beyond the cases above: prints the maxima that DESIGN 8k records (runs last in this file's kernel section)"""
    print('largest forward err / bound %.3f at %s' % WORST['fwd'])
    print('largest forward err in eps r beyond |x - m|: %.2f at %s' % WORST['fwd_ulp'])
    print('largest backward err / bound %.3f at %s' % WORST['bwd'])
    assert WORST['fwd'][0] <= 1.0 and WORST['bwd'][0] <= 1.0


# ---- section 2: models ----------------------------------------------------------------------------------------------------------------------
LR = 0.05


def seed_weights(model, rng):
    """biases, gammas, betas and moving statistics off their 0 / 1 initial values"""
    for l in model.layers:
        ws = l.get_weights()
        if len(ws) == 2:
            l.set_weights([ws[0], (0.1 * rng.randn(*ws[1].shape)).astype(np.float32)])
        elif len(ws) == 4:
            C = ws[0].shape[0]
            l.set_weights([1 + 0.2 * rng.randn(C), 0.2 * rng.randn(C), 0.1 + 0.05 * rng.randn(C), 0.01 + 0.02 * rng.rand(C)])


def categorical_crossentropy(p, t):
    """keras 2.2.4 losses.categorical_crossentropy on probabilities (TF backend): renormalise, clip to [1e-7, 1 - 1e-7], -sum t log p; the mean"""
    q = p / p.sum(-1, keepdim=True)
    return -(t * torch.log(q.clamp(loss_ref.EPS, loss_ref.ONE_M_EPS))).sum(-1).mean()


def mse(p, t):
    return ((p - t) ** 2).mean()


def rel(a, ref):
    a = np.asarray(a, np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-30)


def weights_of(model):
    trained = [l for l in model.layers if l.weights]
    P = dict((l.name, [torch.tensor(a.astype(np.float64), requires_grad=True) for a in l.get_weights()[:2]]) for l in trained)
    moving = dict((l.name, [torch.tensor(a.astype(np.float64)) for a in l.get_weights()[2:]]) for l in trained if len(l.get_weights()) == 4)
    return trained, P, moving


CASES = {'a': ((32, 4), 6, 'categorical_crossentropy', 2), 'b': ((6,), 8, 'mean_squared_error', 2), 'c': ((16, 4), 4, 'mean_squared_error', 1),
         'd': ((32, 8), 4, 'mean_squared_error', 2), 'e': ((1, 8, 4), 4, 'mean_squared_error', 1), 'f': ((16, 4), 4, 'mean_squared_error', 1),
         'g': ((32, 4), 6, 'mean_squared_error', 2),
         # the other conv forms a layer with activation='softmax' launches: tap-folded, upsample-folded, any-channel, the width-2 Conv2D
         'h': ((16, 4), 4, 'mean_squared_error', 1), 'i': ((8, 4), 4, 'mean_squared_error', 1), 'j': ((16, 5), 4, 'mean_squared_error', 1),
         'k': ((8, 2, 4), 4, 'mean_squared_error', 1)}


@pytest.mark.parametrize('key', sorted(CASES))
def test_the_models_predict_and_train_like_torch_fp64(key):
    from gennet_amd.engine import SGD
    in_shape, B, loss, steps = CASES[key]
    rng = np.random.RandomState(ord(key))
    model, ref = M.MODELS[key]()
    seed_weights(model, rng)
    model.compile(optimizer=SGD(lr=LR), loss=loss, metrics=['categorical_accuracy'] if key == 'a' else None)
    x = rng.randn(B, *in_shape).astype(np.float32)
    out_shape = tuple(model.output_shape[1:])
    if key == 'a':
        t = np.eye(3, dtype=np.float32)[rng.randint(0, 3, B)]
    else:
        t = (rng.rand(B, *out_shape) if key in 'cefghijk' else rng.randn(B, *out_shape)).astype(np.float32)
    xt, tt = torch.tensor(x.astype(np.float64)), torch.tensor(t.astype(np.float64))
    loss_fn = categorical_crossentropy if key == 'a' else mse
    trained, P, moving = weights_of(model)
    y = model.predict(x, batch_size=B)
    with torch.no_grad():
        y_ref = ref(P, xt, False, None, moving).numpy()
    print(key, 'predict err', rel(y, y_ref))
    assert rel(y, y_ref) < 1e-5
    assert np.array_equal(model.predict_on_batch(x), y)
    if key in 'hij':                       # the conv form the layer is meant to reach
        from gennet_amd import layers as Ly
        model._plan()
        node = model.nodes[-1]
        run = Ly._ConvRun(node.layer, in_shape[-1], node.fold_up is not None, 16)
        assert (run.tap_folded, run.up_folded, run.any_channels) == {'h': (True, False, False), 'i': (False, True, False), 'j': (False, False, True)}[key]
    if key in 'aefhijk':                   # the output is the softmax: rows of probabilities
        assert np.abs(y.sum(-1) - 1).max() < 1e-6 and (y > 0).all()
    biggest = 0.0
    for step in range(steps):
        trained, P, moving = weights_of(model)
        masks = {'b_drop': (rng.rand(B, 8) >= M.DROP_RATE).astype(np.uint8)} if key == 'b' else None
        tm = None if masks is None else dict((k, torch.tensor(v.astype(np.float64))) for k, v in masks.items())
        out = ref(P, xt, True, tm, moving)
        loss_t = loss_fn(out, tt)
        loss_t.backward()
        res = np.ravel(model.train_on_batch(x, t, dropout_masks=masks))
        print(key, 'step %d loss %.9g reference %.9g' % (step, res[0], float(loss_t.detach())))
        assert abs(res[0] - float(loss_t.detach())) <= 1e-6 * abs(float(loss_t.detach()))
        if key == 'a':
            assert abs(res[1] - float((out.detach().numpy().argmax(-1) == t.argmax(-1)).mean())) < 1e-6
        g_floor = 1e-3 * max(float(v.grad.abs().max()) for ts in P.values() for v in ts)
        for l in trained:
            for p, got, r_ in zip(l.params, l.get_weights()[:2], P[l.name]):
                g_ref = r_.grad.numpy()
                gerr = np.abs(p.grad.detach().cpu().numpy().reshape(g_ref.shape) - g_ref).max() / max(np.abs(g_ref).max(), g_floor)
                w_ref = (r_.detach() - LR * r_.grad).numpy()
                werr = np.abs(got.astype(np.float64) - w_ref).max() / max(np.abs(w_ref).max(), 1e-3)
                biggest = max(biggest, float(np.abs(g_ref).max()))
                print(key, 'step %d %s grad err %.3g weight err %.3g' % (step, p.name, gerr, werr))
                assert gerr < 1e-4 and werr < 1e-4, (key, step, p.name, gerr, werr)
    assert biggest > 1e-4                  # the gradients are no rounding noise


def test_the_training_surface_runs_on_a_softmax_head():
    """test_on_batch, evaluate, fit, sample_weight and class_weight on model (a): the weights live in the loss pass, the softmax needs nothing new"""
    from gennet_amd.engine import SGD
    rng = np.random.RandomState(21)
    model, ref = M.model_a()
    seed_weights(model, rng)
    model.compile(optimizer=SGD(lr=LR), loss='categorical_crossentropy', metrics=['categorical_accuracy'])
    x = rng.randn(8, 32, 4).astype(np.float32)
    labels = rng.randint(0, 3, 8)
    t = np.eye(3, dtype=np.float32)[labels]
    _, P, _ = weights_of(model)
    with torch.no_grad():
        rows = -(torch.tensor(t.astype(np.float64)) * torch.log(ref(P, torch.tensor(x.astype(np.float64)), False).clamp(loss_ref.EPS, loss_ref.ONE_M_EPS))).sum(-1).numpy()
    plain = np.ravel(model.test_on_batch(x, t))
    assert abs(plain[0] - rows.mean()) <= 1e-6 * rows.mean()
    assert abs(np.ravel(model.evaluate(x, t, batch_size=8))[0] - plain[0]) <= 1e-6 * plain[0]
    w = np.array([2, 0, 1, 1, 3, 0, 1, 2], np.float32)
    weighted = np.ravel(model.test_on_batch(x, t, sample_weight=w))
    assert abs(weighted[0] - (rows * w).sum() / 6) <= 1e-6 * weighted[0]                   # sum w l / #{w != 0}
    cw = {0: 1.0, 1: 2.0, 2: 0.5}
    before = [a.copy() for a in model.get_weights()]
    got = np.ravel(model.train_on_batch(x, t, class_weight=cw))
    twin, _ = M.model_a()
    twin.compile(optimizer=SGD(lr=LR), loss='categorical_crossentropy', metrics=['categorical_accuracy'])
    twin.set_weights(before)
    want = np.ravel(twin.train_on_batch(x, t, sample_weight=np.array([cw[int(k)] for k in labels], np.float32)))
    assert np.array_equal(got, want) and all(np.array_equal(u, v) for u, v in zip(model.get_weights(), twin.get_weights()))
    hist = model.fit(x, t, batch_size=4, epochs=6, shuffle=False)
    assert len(hist['loss']) == 6 and np.isfinite(hist['loss']).all() and hist['loss'][-1] < hist['loss'][0]


def test_the_five_spellings_run_the_same_two_kernels(tmp_path):
    """the layer's own activation, Activation('softmax'), Softmax(-1), a loaded .h5 and a loaded JSON: the same bits forward, the same step"""
    from gennet_amd import layers as L
    from gennet_amd.engine import SGD, Sequential, load_model, model_from_json
    rng = np.random.RandomState(22)
    own = Sequential([L.Dense(5, activation='softmax', input_shape=(7,))])
    act = Sequential([L.Dense(5, input_shape=(7,)), L.Activation('softmax')])
    lay = Sequential([L.Dense(5, input_shape=(7,)), L.Softmax(axis=-1)])
    seed_weights(own, rng)
    path_ = os.path.join(str(tmp_path), 'own.h5')
    own.save(path_)
    models = [own, act, lay, load_model(path_), model_from_json(own.to_json())]
    x, t = rng.randn(6, 7).astype(np.float32), np.eye(5, dtype=np.float32)[rng.randint(0, 5, 6)]
    outs = []
    for m in models:
        m.set_weights(own.get_weights())
        m.compile(optimizer=SGD(lr=LR), loss='categorical_crossentropy')
    for m in models:
        y = m.predict(x, batch_size=6)
        loss = np.ravel(m.train_on_batch(x, t))
        outs.append((y, loss, m.get_weights()))
    for y, loss, ws in outs[1:]:
        assert same_bits(y, outs[0][0]) and np.array_equal(loss, outs[0][1]) and all(same_bits(u, v) for u, v in zip(ws, outs[0][2]))


def test_a_captured_step_with_softmax_replays_bit_identically():
    """model (a) as a hipGraph (engine.StepGraph): an eager step, the capture, three replays, against four eager steps of a twin.  The softmax
    passes take no workspace and no host-side decision depends on data, so there is nothing for the graph to keep alive or to freeze."""
    from gennet_amd import engine
    from gennet_amd.engine import SGD, to_device
    rng = np.random.RandomState(23)
    x = to_device(rng.randn(6, 32, 4).astype(np.float32))
    t = to_device(np.eye(3, dtype=np.float32)[rng.randint(0, 3, 6)])
    eager, _ = M.model_a()
    seed_weights(eager, rng)
    graphed, _ = M.model_a()
    graphed.set_weights(eager.get_weights())
    for m in (eager, graphed):
        m.compile(optimizer=SGD(lr=LR, momentum=0.5), loss='categorical_crossentropy', metrics=['categorical_accuracy'])
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
