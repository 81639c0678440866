"""GPU parity of keras layers.Dot: csrc/bmm.hip through ops.bmm / l2norm_fwd / l2norm_bwd against the fp64 definition tests/dot_ref.py (itself
checked against torch autograd in tests/test_dot_cpu.py), and the layer at model level against torch fp64 autograd on the CPU.

Section 1, kernel level.  Inputs sit in NaN-surrounded buffers, outputs in sentinel-filled ones; a view starts 144 bytes in (pad 36: 16-byte
aligned) or 148 bytes in (pad 37: every base pointer moved by one float, which forces the scalar loads of the matrix-core kernel).
The shapes are a covering set of M, N in {1, 2, 31, 32, 33, 64, 65, 100} and K in {1, 2, 3, 15, 16, 17, 33, 70}, batch 1 and 3, in all four
orientation pairs (a or a^T, b or b^T in memory): every value of each, both sides of the 32-wide wave tile and of the 64-wide block tile, of the
16-wide k chunk, K below one MFMA (1) and odd, row lengths that are multiples of 4 (16-byte loads at pad 36) and not, and M == 1 / N == 1 (the
thin kernel, both its forms).  The 128-wide block tiles are taken only by grids of 1024 blocks and more: LARGE_GRIDS reaches each of them.

Section 2, model level: the bounds of tests/test_merge_gpu.py's train_and_compare as they stand, over three SGD steps -- predict 1e-5 of the
largest output, each loss 1e-6 relative, gradients and SGD-updated weights 1e-4 of each tensor's largest entry (gradients no finer than 1e-3 of
the model's largest gradient entry)."""
import os

import numpy as np
import pytest
import torch

import dot_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5
U = 2.0 ** -24                  # unit roundoff of fp32


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
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# (batch, M, N, K)
SHAPES = [(1, 1, 1, 70), (3, 1, 33, 17), (1, 100, 1, 33), (3, 2, 1, 1), (1, 1, 64, 16), (3, 65, 1, 2),        # thin
          (3, 2, 2, 1), (1, 2, 31, 2), (3, 31, 2, 3), (1, 32, 32, 15), (3, 33, 31, 16), (1, 32, 64, 16), (3, 64, 32, 17), (1, 64, 64, 33),
          (1, 33, 65, 70), (3, 31, 100, 15), (1, 65, 33, 3), (3, 100, 64, 16), (1, 65, 65, 17), (3, 100, 100, 70), (1, 100, 65, 2),
          (1, 64, 100, 16), (3, 65, 2, 33), (1, 2, 100, 1)]
ORIENT = [(False, False), (False, True), (True, False), (True, True)]
IDS = ['b%d-m%d-n%d-k%d' % s for s in SHAPES]


def test_the_shapes_cover_the_set():
    assert set(s[1] for s in SHAPES) == set(s[2] for s in SHAPES) == {1, 2, 31, 32, 33, 64, 65, 100}
    assert set(s[3] for s in SHAPES) == {1, 2, 3, 15, 16, 17, 33, 70} and set(s[0] for s in SHAPES) == {1, 3}


def stored(x, trans):
    """the array as the kernel reads it: (batch, rows, cols), or its transpose in memory under `trans`"""
    return np.ascontiguousarray(x.transpose(0, 2, 1)) if trans else x


def run_bmm(a, b, ta, tb, pad, valu=False):
    from gennet_amd import ops
    ga, gb = Guarded(stored(a, ta).shape, stored(a, ta), pad), Guarded(stored(b, tb).shape, stored(b, tb), pad)
    out = Guarded((a.shape[0], a.shape[1], b.shape[2]), None, pad)
    ops.bmm(ga.t, gb.t, trans_a=ta, trans_b=tb, out=out.t, valu=valu)
    return out.check('bmm %r ta=%d tb=%d pad %d' % (a.shape[:2] + b.shape[2:], ta, tb, pad))


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_integer_products_are_exact(shape):
    """Integers in [-4, 4]: every product and partial sum is an integer below 2^24, so ANY correct kernel returns the int64 product bit for bit,
    and a swapped row / column, a wrong lane map, a dropped or doubled k chunk or a transposed operand does not (a != a^T, b != a)."""
    batch, M, N, K = shape
    rng = np.random.RandomState(M * 1000 + N * 10 + K)
    a, b = rng.randint(-4, 5, (batch, M, K)), rng.randint(-4, 5, (batch, K, N))
    if M > 1 and K > 1 and M == K:
        assert not np.array_equal(a, a.transpose(0, 2, 1))
    want = R.bmm(a, b)
    assert want.dtype == np.int64 and np.abs(want).max() < 2 ** 24
    for ta, tb in ORIENT:
        for pad in (37, 36):
            for valu in (False, True):
                c = run_bmm(a.astype(np.float32), b.astype(np.float32), ta, tb, pad, valu)
                assert same_bits(c, (want + 0).astype(np.float32)), (valu, ta, tb, pad, int((c != want).sum()))


@pytest.mark.parametrize('shape', SHAPES + [(1, 33, 65, 1000), (3, 1, 2, 1000), (1, 65, 1, 1000)], ids=IDS + ['b1-m33-n65-k1000', 'b3-m1-n2-k1000', 'b1-m65-n1-k1000'])
def test_real_products_meet_the_fma_chain_bound(shape):
    """Uniform [-1, 1) data against the fp64 product c64 of the same fp32 operands:  |c - c64| <= K * 2^-24 * sum_k |a b|  per element.
    Derivation: an fp32 fma chain c_k = fl(c_{k-1} + a_k b_k) rounds once per term, c_k = (c_{k-1} + a_k b_k)(1 + d_k), |d_k| <= u = 2^-24, so the
    term a_j b_j reaches the result multiplied by prod_{k >= j} (1 + d_k), at most K factors: |c - c64| <= ((1 + u)^K - 1) sum |a b| = K u sum |a b|
    to first order (Higham, Accuracy and Stability, (3.4); the second-order part K^2 u^2 / 2 < 2e-9 K u at K = 1000 is far inside the slack of a
    worst-case bound).  Any other summation order of the same K terms (the thin kernel's 64 interleaved chains and butterfly) passes each term through
    fewer roundings and meets the same bound.  The matrix-core kernel and the VALU tile are both the k-ordered chain: the same bits."""
    batch, M, N, K = shape
    rng = np.random.RandomState(M * 1000 + N * 10 + K + 1)
    a, b = (rng.rand(batch, M, K) * 2 - 1).astype(np.float32), (rng.rand(batch, K, N) * 2 - 1).astype(np.float32)
    c64 = R.bmm(a, b)
    bound = K * U * R.bmm(np.abs(a), np.abs(b))
    for ta, tb in ORIENT:
        for pad in (37, 36):
            c = run_bmm(a, b, ta, tb, pad)
            err = np.abs(c.astype(np.float64) - c64)
            print(shape, ta, tb, pad, 'worst error / bound %.3g' % (err / bound).max())
            assert (err <= bound).all(), (ta, tb, pad, float((err / bound).max()))
            v = run_bmm(a, b, ta, tb, pad, valu=True)
            assert (np.abs(v.astype(np.float64) - c64) <= bound).all()
            if M > 1 and N > 1:
                assert same_bits(c, v), (ta, tb, pad, int((c != v).sum()))


@pytest.mark.parametrize('kernel', ['mfma', 'thin-rows', 'thin-lanes'])
def test_an_output_does_not_depend_on_the_launch(kernel):
    """Batch entry j computed alone, and rows [37, 42) computed alone (another block tile, another position in it), are the bits of the whole."""
    from gennet_amd import ops
    rng = np.random.RandomState(11)
    batch, M, K, N = 3, 100, 70, 65 if kernel == 'mfma' else 1
    ta = kernel == 'thin-lanes'                       # a stored (batch, K, M): the matrix is contiguous along its rows' index, a lane per output
    a, b = (rng.rand(batch, M, K) * 2 - 1).astype(np.float32), (rng.rand(batch, K, N) * 2 - 1).astype(np.float32)
    ta_t = torch.tensor(stored(a, ta), device=dev())
    tb_t = torch.tensor(b, device=dev())
    whole = ops.bmm(ta_t, tb_t, trans_a=ta).cpu().numpy()
    assert np.abs(whole - R.bmm(a, b)).max() < 1e-4
    for j in range(batch):
        one = ops.bmm(ta_t[j:j + 1].contiguous(), tb_t[j:j + 1].contiguous(), trans_a=ta).cpu().numpy()
        assert same_bits(one[0], whole[j]), (kernel, j)
    m0 = 37
    rows = ta_t[:, :, m0:m0 + 5].contiguous() if ta else ta_t[:, m0:m0 + 5].contiguous()
    part = ops.bmm(rows, tb_t, trans_a=ta).cpu().numpy()
    assert same_bits(part, whole[:, m0:m0 + 5]), kernel
    assert same_bits(whole, ops.bmm(ta_t, tb_t, trans_a=ta).cpu().numpy())          # and two runs give identical bits


# (batch, M, N, K) -> the block tile run_mfma picks: 128 a side needs an extent beyond 64 AND 1024 blocks, so the wide tiles want a large batch
LARGE_GRIDS = [((256, 130, 130, 3), (128, 128)), ((200, 130, 130, 17), (128, 64)), ((512, 130, 33, 2), (128, 64)), ((512, 33, 130, 16), (64, 128)),
               ((100, 130, 130, 3), (64, 64))]


def tile_of(batch, M, N):
    """csrc/bmm.hip run_mfma, restated"""
    bm, bn = (64 if M <= 64 else 128), (64 if N <= 64 else 128)
    blocks = lambda m, n: -(-M // m) * -(-N // n) * batch          # noqa: E731
    if bn == 128 and blocks(bm, bn) < 1024:
        bn = 64
    if bm == 128 and blocks(bm, bn) < 1024:
        bm = 64
    return bm, bn


@pytest.mark.parametrize('shape,tile', LARGE_GRIDS, ids=['b%d-m%d-n%d-k%d' % s for s, _ in LARGE_GRIDS])
def test_every_block_tile_is_exact_and_gives_the_bits_of_the_others(shape, tile):
    """Integer operands through each of the four block tiles (the covering set above has too few blocks for the wide ones: all 64 x 64), bit-identical
    to the int64 product; and on real data a batch entry computed alone -- by the 64 x 64 tile -- has the bits it has in the batch."""
    from gennet_amd import ops
    batch, M, N, K = shape
    assert tile_of(batch, M, N) == tile and tile_of(1, M, N) == (64, 64)
    rng = np.random.RandomState(batch + M + N + K)
    a, b = rng.randint(-4, 5, (batch, M, K)), rng.randint(-4, 5, (batch, K, N))
    want = R.bmm(a, b).astype(np.float32)
    for (ta, tb), pad in zip(ORIENT, (36, 37, 37, 36)):
        assert same_bits(run_bmm(a.astype(np.float32), b.astype(np.float32), ta, tb, pad), want), (ta, tb, pad)
    x, y = (rng.rand(batch, M, K) * 2 - 1).astype(np.float32), (rng.rand(batch, K, N) * 2 - 1).astype(np.float32)
    tx, ty = torch.tensor(x, device=dev()), torch.tensor(y, device=dev())
    whole = ops.bmm(tx, ty)
    for j in (0, batch - 1):
        assert torch.equal(ops.bmm(tx[j:j + 1].contiguous(), ty[j:j + 1].contiguous())[0], whole[j]), j


L2_VIEWS = [(7, 1, 5), (3, 33, 1), (2, 64, 3), (1, 1000, 1)]


@pytest.mark.parametrize('pad', [37, 36])
@pytest.mark.parametrize('view', L2_VIEWS, ids=['x'.join(map(str, v)) for v in L2_VIEWS])
def test_l2norm_passes_meet_their_bounds(view, pad):
    """Against dot_ref in fp64 on the same fp32 inputs, u = 2^-24 (one rounding is <= u relative; division and square root are correctly rounded,
    hipcc's default).  Forward:  |inv - r_inv| <= (P / 2 + 2.5) u r_inv,   |y - r_y| <= (P / 2 + 3.5) u |r_y|
      sum      s = sum_p x^2 by fma: a term passes at most P roundings in any order the kernels use (a lane's chain, then butterfly steps whose
               additions of zeros are exact): P u relative, all terms being non-negative
      inv      the square root halves it and rounds (P / 2 + 1), the division rounds (+ 1); where s < 1e-12 inv is the constant 1e6 (2e-9 from
               1 / sqrt(1e-12f)); y = x * inv rounds once more (+ 1); 0.5 for the products of these terms.  An all-zero vector gives y = +-0 exactly.
    Backward, from the fp32 y and inv the forward kernel wrote and a seeded dy, T = sum_p |dy y|:
      |dx - r| <= (P + 3.5) u inv (|dy| + |y| T)
      t = sum_p dy y by fma: P u T; y t rounds (u |y| T), the difference rounds (u (|dy| + |y| T)), the product with inv rounds (the same):
      inv u (|y| T (P + 3) + 2 |dy|), and 0.5 for the products of these terms.  A clamped vector (inv == 1e6) has dx = inv * dy: one rounding."""
    from gennet_amd import ops
    outer, P, inner = view
    rng = np.random.RandomState(outer * 100 + P + pad)
    x = rng.randn(outer, P, inner).astype(np.float32)
    x[outer - 1, :, inner // 2] = 0.0                                      # one all-zero vector
    dy = rng.randn(outer, P, inner).astype(np.float32)
    gx = Guarded(x.shape, x, pad)
    y, inv = ops.l2norm_fwd(gx.t, view)
    torch.cuda.synchronize()
    y, inv = y.cpu().numpy(), inv.cpu().numpy()
    ry, rinv, rcl = R.l2norm_fwd(x, view)
    assert rcl.sum() == 1 and rcl[outer - 1, inner // 2]
    assert inv.shape == (outer, inner) and (np.abs(inv - rinv) <= (P / 2 + 2.5) * U * rinv).all(), float((np.abs(inv - rinv) / rinv).max() / U)
    assert (np.abs(y - ry) <= (P / 2 + 3.5) * U * np.abs(ry)).all()
    assert (y[outer - 1, :, inner // 2] == 0).all() and inv[outer - 1, inner // 2] == np.float32(1e6)
    print(view, 'forward worst / bound %.3g' % (np.abs(y - ry) / np.maximum((P / 2 + 3.5) * U * np.abs(ry), 1e-300)).max())
    gdy, gy, ginv = Guarded(dy.shape, dy, pad), Guarded(y.shape, y, pad), Guarded(inv.shape, inv, pad)
    out = Guarded(dy.shape, None, pad)
    ops.l2norm_bwd(gdy.t, gy.t, ginv.t, view, out=out.t)
    dx = out.check('l2norm_bwd %r' % (view,))
    cl = inv == np.float32(1e6)
    assert np.array_equal(cl, rcl)
    r = R.l2norm_bwd(dy, y, inv.astype(np.float64), cl, view)
    T = np.abs(dy.astype(np.float64) * y).sum(1, keepdims=True)
    bound = (P + 3.5) * U * inv.astype(np.float64)[:, None, :] * (np.abs(dy) + np.abs(y) * T)
    print(view, 'backward worst / bound %.3g' % (np.abs(dx - r) / bound).max())
    assert (np.abs(dx - r) <= bound).all()
    assert same_bits(dx[outer - 1, :, inner // 2], np.float32(1e6) * dy[outer - 1, :, inner // 2])          # dx = inv * dy


def test_bad_arguments_are_errors_and_launch_nothing():
    from gennet_amd import _lib
    batch, M, N, K = 2, 5, 6, 7
    a = Guarded((batch, M, K), np.ones((batch, M, K), np.float32), 36)
    b = Guarded((batch, K, N), np.ones((batch, K, N), np.float32), 36)
    out = Guarded((batch, M, N), None, 36)
    s = torch.cuda.current_stream().cuda_stream
    pa, pb, pc = a.t.data_ptr(), b.t.data_ptr(), out.t.data_ptr()
    good = dict(a=pa, b=pb, c=pc, batch=batch, M=M, N=N, K=K, a_batch=M * K, a_m=K, a_k=1, b_batch=K * N, b_k=N, b_n=1)

    def call(valu, **kw):
        g = dict(good, **kw)
        _lib.call('gn_bmm_valu' if valu else 'gn_bmm', g['a'], g['b'], g['c'], g['batch'], g['M'], g['N'], g['K'], g['a_batch'], g['a_m'], g['a_k'],
                  g['b_batch'], g['b_k'], g['b_n'], s)

    def refused(text, fn):
        with pytest.raises(_lib.GennetHipError) as e:
            fn()
        assert '(%d)' % _lib.GN_EINVAL in str(e.value) and text in str(e.value), str(e.value)
        assert text in _lib.lib().gn_last_error().decode()
        torch.cuda.synchronize()
        assert out.untouched()

    for valu in (False, True):
        for k in ('a', 'b', 'c'):
            refused('null pointer', lambda: call(valu, **{k: None}))
        for k in ('batch', 'M', 'N'):
            refused('negative size', lambda: call(valu, **{k: -1}))
        refused('K = 0', lambda: call(valu, K=0))
        refused('K = -3', lambda: call(valu, K=-3))
        for k in ('a_batch', 'a_m', 'a_k', 'b_batch', 'b_k', 'b_n'):
            refused('strides must be positive', lambda: call(valu, **{k: 0}))
            refused('strides must be positive', lambda: call(valu, **{k: -good[k]}))
        refused("a's strides", lambda: call(valu, a_m=2, a_k=3))            # neither is 1
        refused("a's strides", lambda: call(valu, a_m=K - 1, a_k=1))        # rows overlap: (m, K - 1) is (m + 1, 0)
        refused("a's strides", lambda: call(valu, a_m=1, a_k=M - 1))
        refused("b's strides", lambda: call(valu, b_k=N - 1, b_n=1))
        refused("b's strides", lambda: call(valu, b_k=1, b_n=K - 1))
        refused('exceed the grid', lambda: call(valu, batch=2 ** 31 - 1, M=129, N=2))          # 2 (valu: 9) row tiles an entry: >= 2^31 blocks
        refused('spans 2^62', lambda: call(valu, batch=2 ** 31 - 1, M=2 ** 20, N=2 ** 20, b_k=2 ** 20))
        # nothing to do is not an error, and launches nothing (the pointers are not looked at)
        for k in ('batch', 'M', 'N'):
            call(valu, **{k: 0})
        call(valu, a=None, b=None, c=None, M=0)
    x = Guarded((4, 6), np.ones((4, 6), np.float32), 36)
    px = x.t.data_ptr()
    refused('null pointer', lambda: _lib.call('gn_l2norm_fwd', None, pc, pc, 4, 6, 1, s))
    refused('null pointer', lambda: _lib.call('gn_l2norm_fwd', px, pc, None, 4, 6, 1, s))
    refused('null pointer', lambda: _lib.call('gn_l2norm_bwd', px, px, None, pc, 4, 6, 1, s))
    refused('null pointer', lambda: _lib.call('gn_l2norm_bwd', px, px, px, None, 4, 6, 1, s))
    refused('bad shape', lambda: _lib.call('gn_l2norm_fwd', px, pc, pc, 4, 0, 1, s))
    refused('bad shape', lambda: _lib.call('gn_l2norm_fwd', px, pc, pc, 4, 6, -1, s))
    refused('bad shape', lambda: _lib.call('gn_l2norm_bwd', px, px, px, pc, 4, 2 ** 16, 2 ** 15, s))
    _lib.call('gn_l2norm_fwd', px, pc, pc, 0, 6, 1, s)
    _lib.call('gn_l2norm_bwd', px, px, px, pc, 0, 6, 1, s)
    torch.cuda.synchronize()
    assert out.untouched()


# ---------------------------------------------------------------------------------------------------------------------
# section 2: models against torch fp64 autograd (the logic and bounds of tests/test_merge_gpu.py's train_and_compare, over several steps)
# ---------------------------------------------------------------------------------------------------------------------
LR = 0.05


def rel(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-30)


def seed_biases(model, rng):
    for l in model.layers:
        ws = l.get_weights()
        if len(ws) == 2:
            l.set_weights([ws[0], (0.1 * rng.randn(*ws[1].shape)).astype(np.float32)])


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


def attention_model():
    from gennet_amd import layers as Ly
    from gennet_amd.engine import Input, Model
    x = Input((10, 8))
    cq, ck, cv, head = Ly.Conv1D(8, 1), Ly.Conv1D(8, 1), Ly.Conv1D(8, 1), Ly.Dense(1)
    scores = Ly.Dot((2, 2))([cq(x), ck(x)])
    ctx = Ly.Dot((2, 1))([Ly.Softmax(-1)(scores), cv(x)])
    model = Model(inputs=x, outputs=head(Ly.GlobalAveragePooling1D()(Ly.Add()([ctx, x]))))

    def ref(P, x):
        q, k, v = conv1(P, cq, x), conv1(P, ck, x), conv1(P, cv, x)
        a = torch.softmax(torch.matmul(q, k.transpose(1, 2)), dim=-1)
        return (torch.matmul(a, v) + x).mean(1) @ P[head.name][0] + P[head.name][1]
    return model, ref


def test_self_attention_block_trains_as_torch_fp64():
    model, ref = attention_model()
    rng = np.random.RandomState(21)
    seed_biases(model, rng)
    assert [type(n.layer).__name__ for n in model.nodes].count('Dot') == 2
    train_and_compare(model, ref, [rng.randn(3, 10, 8).astype(np.float32)], rng.randn(3, 1).astype(np.float32), what='attention')


def test_attention_pooling_trains_as_torch_fp64():
    """weights (B, L) over time times values (B, L, C): a rank-2 by rank-3 product, M == 1 (the thin kernel, forward and both gradients)"""
    from gennet_amd import layers as Ly
    from gennet_amd.engine import Input, Model
    x = Input((10, 8))
    cs, cv, head = Ly.Conv1D(1, 1), Ly.Conv1D(4, 1), Ly.Dense(1)
    w = Ly.Softmax()(Ly.Flatten()(cs(x)))
    model = Model(inputs=x, outputs=head(Ly.Dot((1, 1))([w, cv(x)])))
    assert [n.out_shape for n in model.nodes if type(n.layer).__name__ == 'Dot'] == [(4,)]
    rng = np.random.RandomState(22)
    seed_biases(model, rng)

    def ref(P, x):
        w = torch.softmax(conv1(P, cs, x)[:, :, 0], dim=-1)
        return torch.einsum('bl,blc->bc', w, conv1(P, cv, x)) @ P[head.name][0] + P[head.name][1]
    train_and_compare(model, ref, [rng.randn(3, 10, 8).astype(np.float32)], rng.randn(3, 1).astype(np.float32), what='attention pooling')


def test_cosine_head_trains_as_torch_fp64():
    from gennet_amd import layers as Ly
    from gennet_amd.engine import Input, Model
    x = Input((5,))
    da, db, head = Ly.Dense(8), Ly.Dense(8), Ly.Dense(1)
    model = Model(inputs=x, outputs=head(Ly.Dot(1, normalize=True)([da(x), db(x)])))
    assert [n.out_shape for n in model.nodes if type(n.layer).__name__ == 'Dot'] == [(1,)]
    rng = np.random.RandomState(23)
    seed_biases(model, rng)

    def ref(P, x):
        a, b = x @ P[da.name][0] + P[da.name][1], x @ P[db.name][0] + P[db.name][1]
        a = a / torch.sqrt(torch.clamp((a * a).sum(1, keepdim=True), min=1e-12))
        b = b / torch.sqrt(torch.clamp((b * b).sum(1, keepdim=True), min=1e-12))
        return (a * b).sum(1, keepdim=True) @ P[head.name][0] + P[head.name][1]
    train_and_compare(model, ref, [rng.randn(6, 5).astype(np.float32)], rng.randn(6, 1).astype(np.float32), what='cosine')


def test_gram_matrix_of_one_tensor_on_both_edges():
    """Dot(2)([t, t]): inbound [i, i]; the layer returns two gradients and the engine sums them.  The output is quartic in the conv's weights: with
    unit-variance inputs SGD at LR = 0.05 diverges (the torch fp64 run alone: loss 18 -> 6e3 -> 1e12) and multiplies a last-bit difference by the same
    factors, so the inputs are scaled by 0.3, where the run descends."""
    from gennet_amd import layers as Ly
    from gennet_amd.engine import Input, Model
    x = Input((6, 8))
    c, head = Ly.Conv1D(4, 1), Ly.Dense(1)
    t = c(x)
    model = Model(inputs=x, outputs=head(Ly.Flatten()(Ly.Dot(2)([t, t]))))
    assert [n.inbound for n in model.nodes] == [[-1], [0, 0], [1], [2]] and model.nodes[1].out_shape == (6, 6)
    rng = np.random.RandomState(24)
    seed_biases(model, rng)

    def ref(P, x):
        t = conv1(P, c, x)
        return torch.matmul(t, t.transpose(1, 2)).reshape(x.shape[0], -1) @ P[head.name][0] + P[head.name][1]
    train_and_compare(model, ref, [(0.3 * rng.randn(3, 6, 8)).astype(np.float32)], rng.randn(3, 1).astype(np.float32), what='gram')


def test_a_graph_input_on_either_edge_gets_no_gradient():
    """Dot((2, 1))([h, x2]) and Dot((2, 2))([x1, h]): need_dx is false for the graph input, true for h, whose two gradients are summed.
    Inputs scaled by 0.3 as in the Gram test: with unit-variance inputs SGD at LR = 0.05 diverges on this model too."""
    from gennet_amd import layers as Ly
    from gennet_amd.engine import Input, Model
    x1, x2 = Input((6, 4)), Input((4, 3))
    c, head = Ly.Conv1D(4, 1), Ly.Dense(1)
    h = c(x1)
    d1, d2 = Ly.Dot((2, 1))([h, x2]), Ly.Dot((2, 2))([x1, h])
    model = Model(inputs=[x1, x2], outputs=head(Ly.Flatten()(Ly.Concatenate()([d1, d2]))))
    assert [n.inbound for n in model.nodes[:3]] == [[-1], [0, -2], [-1, 0]] and model.nodes[3].out_shape == (6, 9)
    rng = np.random.RandomState(25)
    seed_biases(model, rng)

    def ref(P, a, b):
        h = conv1(P, c, a)
        j = torch.cat([torch.matmul(h, b), torch.matmul(a, h.transpose(1, 2))], dim=2)
        return j.reshape(a.shape[0], -1) @ P[head.name][0] + P[head.name][1]
    train_and_compare(model, ref, [(0.3 * rng.randn(3, 6, 4)).astype(np.float32), (0.3 * rng.randn(3, 4, 3)).astype(np.float32)], rng.randn(3, 1).astype(np.float32),
                      what='graph inputs')


def test_save_and_load_round_trip(tmp_path):
    from gennet_amd.engine import SGD, load_model
    model, _ = attention_model()
    rng = np.random.RandomState(26)
    seed_biases(model, rng)
    x, t = rng.randn(3, 10, 8).astype(np.float32), rng.randn(3, 1).astype(np.float32)
    model.compile(optimizer=SGD(lr=LR), loss='mean_squared_error')
    model.train_on_batch(x, t)
    path = os.path.join(str(tmp_path), 'attention.h5')
    model.save(path)
    again = load_model(path)
    assert [type(n.layer).__name__ for n in again.nodes] == [type(n.layer).__name__ for n in model.nodes]
    assert [n.inbound for n in again.nodes] == [n.inbound for n in model.nodes]
    dots = [n.layer for n in again.nodes if type(n.layer).__name__ == 'Dot']
    assert [d.axes for d in dots] == [(2, 2), (2, 1)] and not any(d.normalize for d in dots)
    assert np.array_equal(model.predict(x), again.predict(x))
    a, b = model.train_on_batch(x, t), again.train_on_batch(x, t)
    assert a == b and all(np.array_equal(u, v) for u, v in zip(model.get_weights(), again.get_weights()))


def test_a_captured_step_of_the_attention_block_replays_bit_identically():
    """the self-attention model as a hipGraph (engine.StepGraph): eager step, capture, three replays against four eager steps of a twin"""
    from gennet_amd import engine
    from gennet_amd.engine import SGD, to_device
    rng = np.random.RandomState(27)
    x, t = to_device(rng.randn(3, 10, 8).astype(np.float32)), to_device(rng.randn(3, 1).astype(np.float32))
    eager, _ = attention_model()
    seed_biases(eager, rng)
    graphed, _ = attention_model()
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
