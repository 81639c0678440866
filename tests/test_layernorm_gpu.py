"""GPU parity of keras layers.LayerNormalization: csrc/layernorm.hip through the C ABI and ops.layernorm_fwd / layernorm_bwd against the fp64
definition tests/layernorm_ref.py (itself checked against a plain loop and torch autograd in tests/test_layernorm_cpu.py), and the layer at model
level against torch fp64 autograd on the CPU.

Section 1, kernel level.  The regime seams and the grid caps come from the library's header.  Inputs sit in NaN-surrounded buffers, outputs (the
workspace too) in sentinel-filled ones; a view starts 144 bytes in (pad 36: 16-byte aligned, the 16-byte accesses where N % 4 == 0) or 148 bytes
in (pad 37: the guarded 4-byte accesses).

THE BOUND of the parity tests is not a constant.  In the same test the same operands go through fp32 torch.nn.functional.layer_norm and its
autograd on the device, and torch's largest error against fp64 is measured per tensor (y, dx, dgamma, dbeta).  The kernels may exceed the larger
of that error and the rounding floor of the inputs (layernorm_ref.floors: a row at offset mu loses |mu| / sigma ulps in x - mean whatever the
implementation does, and one lucky rounding in torch must not set the bar) by a factor of 4, plus 4 ulp (4 * 2^-23) of the tensor's largest
reference magnitude; the factor covers a different but equally valid summation order.  The rows of every case cycle through the offsets 0, -50,
1000 and 3 * 10^4 and the spreads 1, 0.1, 3 and 10^-3; eps alternates between 10^-3 and 10^-6.  The measured ratios are printed.

Section 2, model level: the logic and bounds of tests/test_attention_gpu.py's train_and_compare as they stand (layernorm_ref.train_and_compare),
over three SGD steps."""
import os

import numpy as np
import pytest
import torch

import layernorm_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5
ULP = 2.0 ** -23
FACTOR, FLOOR = 4.0, 4.0 * ULP
OFFSETS, SPREADS = (0.0, -50.0, 1000.0, 3e4), (1.0, 0.1, 3.0, 1e-3)
MAX_ELEMENTS = 9 << 19           # 4.5 M floats, 18 MB a tensor: the largest parity case


def dev():
    return torch.device('cuda:0')


def seams():
    from gennet_amd import ops
    return ops.LAYERNORM_ROWS_MAX_N, ops.LAYERNORM_BLOCK_MAX_N, ops.LAYERNORM_FWD_GRID_CAP, ops.LAYERNORM_BWD_GRID_CAP, ops.LAYERNORM_BWD_GRID_CAP_WIDE


def geometry(N):
    """(rows a wave holds, rows one trip of a block holds, backward grid cap) for N, restated from csrc/layernorm_geom.h"""
    rows_max, _, _, cap, wide = seams()
    if N > rows_max:
        return 1, 1, wide
    quads = (N + 3) // 4
    W = 1
    while W < 64 and W < quads:
        W *= 2
    NJ = (quads + 63) // 64
    U = 1 if NJ >= 3 else 4 // NJ
    return 64 // W, 4 * (64 // W) * U, cap


class Guarded(object):
    """A contiguous view `pad` floats into a larger flat buffer: inputs surrounded by NaN, outputs inside a sentinel-filled buffer."""

    def __init__(self, shape, value=None, pad=37):
        self.n, self.pad = int(np.prod(shape)), pad
        self.buf = torch.full((self.n + 2 * pad,), float('nan') if value is not None else SENTINEL, dtype=torch.float32, device=dev())
        self.t = self.buf[pad:pad + self.n].view(shape)
        if value is not None:
            self.t.copy_(torch.tensor(np.ascontiguousarray(value, np.float32), device=dev()))
        assert self.t.is_contiguous() and self.t.data_ptr() == self.buf.data_ptr() + 4 * pad and (self.t.data_ptr() % 16 == 0) == (pad % 4 == 0)

    def edges_untouched(self):
        return bool((torch.cat([self.buf[:self.pad], self.buf[self.pad + self.n:]]) == SENTINEL).all())

    def check(self, what):
        """the surroundings untouched, every element of the view written"""
        assert self.edges_untouched(), '%s: wrote outside its output' % what
        assert not bool((self.t == SENTINEL).any()), '%s: output elements left unwritten' % what
        assert not bool(torch.isnan(self.t).any()), '%s: NaN (an element outside an input was read)' % what
        return self.t.cpu().numpy()

    def untouched(self):
        return bool((self.buf == SENTINEL).all())


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def operands(rows, N, seed):
    """x with the offset and the spread of a row cycling through OFFSETS and SPREADS, dy, gamma, beta: float32"""
    rng = np.random.RandomState(seed)
    r = np.arange(rows)
    off = np.array(OFFSETS)[(r + seed) % 4][:, None]
    spread = np.array(SPREADS)[(r // 4 + seed) % 4][:, None]
    x = (off + spread * rng.randn(rows, N)).astype(np.float32)
    return x, rng.randn(rows, N).astype(np.float32), (1.0 + 0.5 * rng.randn(N)).astype(np.float32), rng.randn(N).astype(np.float32)


def run_kernels(x, dy, gamma, beta, eps, pad, want=('dx', 'dgamma', 'dbeta'), training=True):
    """forward and backward through the C ABI on guarded buffers -> dict of numpy arrays (None where a tensor was not asked for)"""
    from gennet_amd import _lib
    rows, N = x.shape
    gx, gd = Guarded(x.shape, x, pad), Guarded(dy.shape, dy, pad)
    gg = Guarded((N,), gamma, pad) if gamma is not None else None
    gb = Guarded((N,), beta, pad) if beta is not None else None
    y, mean, rstd = Guarded((rows, N), None, pad), Guarded((rows,), None, pad), Guarded((rows,), None, pad)
    s = torch.cuda.current_stream().cuda_stream
    ptr = lambda g: g.t.data_ptr() if g is not None else None          # noqa: E731
    what = 'layernorm rows %d N %d pad %d' % (rows, N, pad)
    if not training:                               # the inference phase: mean and rstd NULL, the same y
        _lib.call('gn_layernorm_fwd', ptr(gx), ptr(gg), ptr(gb), ptr(y), None, None, rows, N, eps, s)
        assert mean.untouched() and rstd.untouched()
        infer = y.check(what + ' y (inference)')
        y = Guarded((rows, N), None, pad)
    _lib.call('gn_layernorm_fwd', ptr(gx), ptr(gg), ptr(gb), ptr(y), ptr(mean), ptr(rstd), rows, N, eps, s)
    res = dict(y=y.check(what + ' y'), mean=mean.check(what + ' mean'), rstd=rstd.check(what + ' rstd'))
    if not training:
        assert same_bits(infer, res['y']), what + ': the inference phase writes another y'
    nbytes = _lib.size('gn_layernorm_bwd_workspace', rows, N)
    assert nbytes % 4 == 0
    ws = Guarded((nbytes // 4,), None, pad)
    outs = dict(dx=Guarded((rows, N), None, pad), dgamma=Guarded((N,), None, pad), dbeta=Guarded((N,), None, pad))
    _lib.call('gn_layernorm_bwd', ptr(gd), ptr(gx), ptr(gg), ptr(mean), ptr(rstd), ptr(outs['dx']) if 'dx' in want else None,
              ptr(outs['dgamma']) if 'dgamma' in want else None, ptr(outs['dbeta']) if 'dbeta' in want else None, ptr(ws), nbytes, rows, N, s)
    torch.cuda.synchronize()
    assert ws.edges_untouched(), what + ': wrote outside the workspace'
    if 'dgamma' not in want and 'dbeta' not in want:          # behind the two floats a row of the stream regime
        assert bool((ws.t[2 * rows if N > seams()[1] else 0:] == SENTINEL).all()), what + ': a frozen layer wrote partials'
    for name, g in outs.items():
        if name in want:
            res[name] = g.check(what + ' ' + name)
        else:
            assert g.untouched(), what + ': %s was not asked for' % name
            res[name] = None
    return res


def run_torch(x, dy, gamma, beta, eps):
    """fp32 torch.nn.functional.layer_norm and its autograd on the device"""
    tx = torch.tensor(x, device=dev(), requires_grad=True)
    tg = torch.tensor(gamma, device=dev(), requires_grad=True) if gamma is not None else None
    tb = torch.tensor(beta, device=dev(), requires_grad=True) if beta is not None else None
    ty = torch.nn.functional.layer_norm(tx, (x.shape[1],), tg, tb, eps)
    ty.backward(torch.tensor(dy, device=dev()))
    return dict(y=ty.detach().cpu().numpy(), dx=tx.grad.cpu().numpy(), dgamma=tg.grad.cpu().numpy() if tg is not None else None,
                dbeta=tb.grad.cpu().numpy() if tb is not None else None)


def abserr(got, ref):
    return float(np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64)).max())


WORST = {}


def check_against_torch(x, dy, gamma, beta, eps, pad, what, want=('dx', 'dgamma', 'dbeta'), training=True):
    ref = R.backward(x, dy, gamma, eps)
    ref['y'] = R.forward(x, gamma, beta, eps)[0]
    floors = R.floors(x, dy, gamma, eps)
    theirs = run_torch(x, dy, gamma, beta, eps)
    got = run_kernels(x, dy, gamma, beta, eps, pad, want, training)
    ratios = {}
    for name in ('y',) + tuple(want):
        assert np.isfinite(got[name]).all(), (what, name)
        mag = float(np.abs(ref[name]).max())
        terr = abserr(theirs[name], ref[name]) if theirs[name] is not None else 0.0          # torch has no dgamma without gamma, no dbeta without beta
        bound = FACTOR * max(terr, floors[name]) + FLOOR * mag
        err = abserr(got[name], ref[name])
        ratios[name] = err / bound if bound > 0 else (0.0 if err == 0 else float('inf'))
        WORST[name] = max(WORST.get(name, 0.0), ratios[name])
        print(what, name, 'err %.3g, torch err %.3g, floor %.3g, largest magnitude %.3g, err / bound %.3g' % (err, terr, floors[name], mag, ratios[name]))
    assert all(r <= 1.0 for r in ratios.values()), (what, ratios)
    return got, ref


# (rows, N, pad, variant): every N of the list, the seams and seam + 1 and a streamed N of two chunks and a tail; per N the rows 1, 3, one more than a
# wave holds and one more than one trip of the capped backward grid holds
def parity_cases():
    rows_max, block_max, _, _, _ = seams()
    Ns = [1, 2, 3, 5, 63, 64, 65, 127, 128, 129, 256, 257, rows_max, rows_max + 1, block_max, block_max + 1, 2 * block_max + 5]
    variants = ['full', 'no-gamma', 'no-beta', 'plain', 'inference', 'no-dx', 'frozen', 'dbeta-only']
    cases, n = [], 0
    for N in Ns:
        per_wave, per_trip, cap = geometry(N)
        for rows in (1, 3, per_wave + 1, per_trip * cap + 1):
            assert rows * N <= MAX_ELEMENTS, (rows, N)
            cases.append((rows, N, 36 if len(cases) % 2 else 37, variants[n % len(variants)] if rows < 100 else 'full'))
            n += rows < 100                        # the variants cycle over the small cases; the long ones ask for everything
    return cases


def case_id(c):
    return 'rows%d-n%d-pad%d-%s' % c


VARIANTS = {'full': (True, True, ('dx', 'dgamma', 'dbeta'), True), 'no-gamma': (False, True, ('dx', 'dbeta'), True),
            'no-beta': (True, False, ('dx', 'dgamma'), True), 'plain': (False, False, ('dx',), True), 'inference': (True, True, ('dx', 'dgamma', 'dbeta'), False),
            'no-dx': (True, True, ('dgamma', 'dbeta'), True), 'frozen': (True, True, ('dx',), True), 'dbeta-only': (True, True, ('dx', 'dbeta'), True)}


def test_the_cases_cover_the_set():
    rows_max, block_max, fwd_cap, cap, wide = seams()
    C = parity_cases()
    assert (rows_max, block_max, fwd_cap, cap, wide) == (1024, 4096, 2048, 1024, 512) and len(C) == 17 * 4
    assert {1, 2, 3, 5, 63, 64, 65, 127, 128, 129, rows_max, rows_max + 1, block_max, block_max + 1} < set(c[1] for c in C)
    assert max(c[1] for c in C) > 2 * block_max and set(c[2] for c in C) == {36, 37} and set(c[3] for c in C) == set(VARIANTS)
    for N in set(c[1] for c in C):
        per_wave, per_trip, grid_cap = geometry(N)
        assert set(c[0] for c in C if c[1] == N) == {1, 3, per_wave + 1, per_trip * grid_cap + 1}
    assert geometry(64) == (4, 64, cap) and geometry(1) == (64, 1024, cap) and geometry(1024) == (1, 4, cap) and geometry(1025) == (1, 1, wide)
    assert any(c[2] == 36 and c[1] % 4 == 0 for c in C) and any(c[2] == 36 and c[1] % 4 for c in C) and any(c[2] == 37 and c[1] % 4 == 0 for c in C)
    assert max(c[0] * c[1] for c in C) * 4 <= 18 * 2 ** 20


@pytest.mark.parametrize('case', parity_cases(), ids=case_id)
def test_forward_and_all_gradients_against_fp64_within_the_measured_bound(case):
    rows, N, pad, variant = case
    scale, center, want, training = VARIANTS[variant]
    x, dy, gamma, beta = operands(rows, N, rows + N)
    check_against_torch(x, dy, gamma if scale else None, beta if center else None, 1e-6 if (rows + N) % 2 else 1e-3, pad, case_id(case), want, training)
    print('largest err / bound so far:', ' '.join('%s %.3g' % kv for kv in sorted(WORST.items())))


def run_ops(x, dy, gamma, beta, eps=1e-3):
    from gennet_amd import ops
    N = x.shape[-1]
    y, mean, rstd = ops.layernorm_fwd(x, gamma, beta, N, eps, training=True)
    dx, dgamma, dbeta = ops.layernorm_bwd(dy, x, gamma, mean, rstd, N, True, need_dgamma=gamma is not None, need_dbeta=True)
    return dict(y=y, mean=mean, rstd=rstd, dx=dx, dgamma=dgamma, dbeta=dbeta)


REGIME_NS = [1, 5, 64, 300, 1024, 1025, 4100, 8197]


@pytest.mark.parametrize('N', REGIME_NS)
def test_a_constant_row_gives_beta_bit_for_bit_and_a_finite_dx(N):
    """2.5 k is exact in fp32 for every k <= N, so the sum of a row of 2.5 is exact in any order and the mean is 2.5: x - mean is exactly 0, and
    y = fma(0 * rstd, gamma, beta) = beta.  N = 1 is a constant row whatever its value."""
    rng = np.random.RandomState(N)
    rows = 7
    x = np.full((rows, N), 2.5, np.float32)
    if N == 1:
        x[:, 0] = rng.randn(rows) * 100
    x[3] = rng.randn(N) + 2.5 if N > 1 else x[3]
    _, dy, gamma, beta = operands(rows, N, N)
    for pad in (36, 37):
        got = run_kernels(x, dy, gamma, beta, 1e-3, pad)
        for r in range(rows):
            if N == 1 or r != 3:
                assert same_bits(got['y'][r], beta), (N, pad, r)
        assert np.isfinite(got['dx']).all() and (N == 1 or not same_bits(got['y'][3], beta))
        if N == 1:                                 # xhat is 0: dx = rstd ((g - g) - 0) = 0, dgamma = 0, dbeta = sum dy
            assert not got['dx'].any() and not got['dgamma'].any()


@pytest.mark.parametrize('N', REGIME_NS)
def test_a_row_alone_has_the_bits_it_has_in_the_batch_and_at_either_alignment(N):
    rows = 9
    x, dy, gamma, beta = operands(rows, N, 40 + N)
    whole = run_kernels(x, dy, gamma, beta, 1e-3, 36)
    other = run_kernels(x, dy, gamma, beta, 1e-3, 37)
    for name in ('y', 'mean', 'rstd', 'dx', 'dgamma', 'dbeta'):          # the 4-byte form owns the same columns in the same lanes
        assert same_bits(whole[name], other[name]), (N, name)
    for r in (0, 4, 8):
        one = run_kernels(x[r:r + 1], dy[r:r + 1], gamma, beta, 1e-3, 37 if r == 4 else 36)
        for name in ('y', 'mean', 'rstd', 'dx'):
            assert same_bits(one[name][0], whole[name][r]), (N, r, name)
    dv = dev()
    a = run_ops(*(torch.tensor(t, device=dv) for t in (x, dy, gamma, beta)))
    for name in ('y', 'dx', 'dgamma', 'dbeta'):                           # ops reaches the same kernels
        assert same_bits(a[name].cpu().numpy(), whole[name]), (N, name)


@pytest.mark.parametrize('rows,N', [(140000, 24), (5000, 1000), (1100, 2048), (600, 4100)], ids=lambda v: str(v))
def test_two_runs_of_the_backward_give_identical_weight_gradients(rows, N):
    """more rows than one trip of the capped grid holds: every block sums several rows, the partials of all blocks are summed"""
    dv = dev()
    x, dy, gamma, beta = (torch.tensor(t, device=dv) for t in operands(rows, N, rows))
    a, b = run_ops(x, dy, gamma, beta), run_ops(x, dy, gamma, beta)
    for name in a:
        assert torch.equal(a[name], b[name]), name
    ref = R.backward(x.cpu().numpy(), dy.cpu().numpy(), gamma.cpu().numpy())
    for name in ('dgamma', 'dbeta'):
        err = abserr(a[name].cpu().numpy(), ref[name])
        print(rows, N, name, 'relative to the largest entry: %.3g' % (err / np.abs(ref[name]).max()))


def test_refused_calls_launch_nothing():
    from gennet_amd import _lib
    rows, N = 3, 8
    ones = lambda *s: Guarded(s, np.ones(s, np.float32), 36)          # noqa: E731
    x, dy, gamma, beta, mean_in, rstd_in = ones(rows, N), ones(rows, N), ones(N), ones(N), ones(rows), ones(rows)
    outs = [Guarded(s, None, 36) for s in ((rows, N), (rows,), (rows,), (rows, N), (N,), (N,), (2 * N,))]
    y, mean, rstd, dx, dgamma, dbeta, ws = outs
    s = torch.cuda.current_stream().cuda_stream
    p = lambda g: g.t.data_ptr()          # noqa: E731

    def refused(text, fn, code=None):
        with pytest.raises(_lib.GennetHipError) as e:
            fn()
        assert '(%d)' % (_lib.GN_EINVAL if code is None else code) in str(e.value) and text in str(e.value), str(e.value)
        torch.cuda.synchronize()
        assert all(g.untouched() for g in outs)

    refused('null pointer', lambda: _lib.call('gn_layernorm_fwd', None, p(gamma), p(beta), p(y), p(mean), p(rstd), rows, N, 1e-3, s))
    refused('bad shape', lambda: _lib.call('gn_layernorm_fwd', p(x), p(gamma), p(beta), p(y), p(mean), p(rstd), 0, N, 1e-3, s))
    refused('eps', lambda: _lib.call('gn_layernorm_fwd', p(x), p(gamma), p(beta), p(y), p(mean), p(rstd), rows, N, -1.0, s))
    refused('given together', lambda: _lib.call('gn_layernorm_fwd', p(x), p(gamma), p(beta), p(y), p(mean), None, rows, N, 1e-3, s))
    refused('null pointer', lambda: _lib.call('gn_layernorm_bwd', p(dy), p(x), p(gamma), None, p(rstd_in), p(dx), p(dgamma), p(dbeta), p(ws), 8 * N, rows, N, s))
    refused('dgamma without gamma', lambda: _lib.call('gn_layernorm_bwd', p(dy), p(x), None, p(mean_in), p(rstd_in), p(dx), p(dgamma), p(dbeta), p(ws), 8 * N,
                                                      rows, N, s))
    refused('workspace too small', lambda: _lib.call('gn_layernorm_bwd', p(dy), p(x), p(gamma), p(mean_in), p(rstd_in), p(dx), p(dgamma), p(dbeta), p(ws),
                                                     8 * N - 1, rows, N, s), _lib.GN_EWORKSPACE)
    _lib.call('gn_layernorm_bwd', p(dy), p(x), p(gamma), p(mean_in), p(rstd_in), None, None, None, None, 0, rows, N, s)          # nothing asked for
    torch.cuda.synchronize()
    assert all(g.untouched() for g in outs)
    _lib.call('gn_layernorm_fwd', p(x), p(gamma), p(beta), p(y), p(mean), p(rstd), rows, N, 1e-3, s)
    _lib.call('gn_layernorm_bwd', p(dy), p(x), p(gamma), p(mean), p(rstd), p(dx), p(dgamma), p(dbeta), p(ws), 8 * N, rows, N, s)
    for g, name in zip(outs, ('y', 'mean', 'rstd', 'dx', 'dgamma', 'dbeta', 'workspace')):
        g.check(name)


# ---------------------------------------------------------------------------------------------------------------------
# section 2: models against torch fp64 autograd
# ---------------------------------------------------------------------------------------------------------------------
def seed_weights(model, rng):
    """every kernel (Keras' glorot_uniform) and bias (0.1 N(0, 1)) of model.parts and gamma (1 + 0.2 N(0, 1)) and beta (0.1 N(0, 1)) of model.norms
    from `rng`: the whole model is a function of the seed"""
    for l in model.parts:
        ws = l.get_weights()
        lim = np.sqrt(6.0 / (ws[0].shape[-2] + ws[0].shape[-1]))
        l.set_weights([rng.uniform(-lim, lim, ws[0].shape).astype(np.float32), (0.1 * rng.randn(*ws[1].shape)).astype(np.float32)])
    for l in model.norms:
        l.set_weights([((1.0 if p.name.endswith('gamma') else 0.0) + (0.2 if p.name.endswith('gamma') else 0.1) * rng.randn(*p.shape)).astype(np.float32)
                       for p in l.weights])


def t_norm(P, layer, x):
    """the layer in torch fp64, from its public configuration"""
    ws = list(P.get(layer.name, []))
    shape = tuple(x.shape[a] for a in layer.axis)
    gamma = ws.pop(0).reshape(shape) if layer.scale else None
    beta = ws.pop(0).reshape(shape) if layer.center else None
    return torch.nn.functional.layer_norm(x, shape, gamma, beta, layer.epsilon)


def dense(P, layer, x, act=None):
    y = x @ P[layer.name][0] + P[layer.name][1]
    return torch.relu(y) if act == 'relu' else y


def dense_model(shape=(12,), **kw):
    """Dense -> LayerNormalization -> Dense on (B,) + shape, flattened before the head where the input is a sequence"""
    from gennet_amd import layers as Ly
    from gennet_amd.engine import Input, Model
    x = Input(shape)
    d0, ln, head = Ly.Dense(shape[-1]), Ly.LayerNormalization(**kw), Ly.Dense(3)
    h = ln(d0(x))
    model = Model(inputs=x, outputs=head(Ly.Flatten()(h) if len(shape) > 1 else h))
    model.parts, model.norms = (d0, head), (ln,)

    def ref(P, x):
        h = t_norm(P, ln, dense(P, d0, x))
        return dense(P, head, h.reshape(x.shape[0], -1))
    return model, ref, ln


def encoder_model(heads=1):
    """x -> Attention([x, x]) -> Add -> LayerNormalization -> Dense(relu) -> Dense -> Add -> LayerNormalization -> GlobalAveragePooling1D -> Dense(1)"""
    from gennet_amd import layers as Ly
    from gennet_amd.engine import Input, Model
    T, C = 10, 12
    x = Input((T, C))
    ln1, ln2, f1, f2, head = Ly.LayerNormalization(), Ly.LayerNormalization(epsilon=1e-6), Ly.Dense(16, activation='relu'), Ly.Dense(C), Ly.Dense(1)

    def split(t):
        return Ly.Permute((2, 1, 3))(Ly.Reshape((T, heads, C // heads))(t)) if heads > 1 else t
    q = split(x)
    ctx = Ly.Attention()([q, q])
    if heads > 1:
        ctx = Ly.Reshape((T, C))(Ly.Permute((2, 1, 3))(ctx))
    h1 = ln1(Ly.Add()([x, ctx]))
    h2 = ln2(Ly.Add()([h1, f2(f1(h1))]))
    model = Model(inputs=x, outputs=head(Ly.GlobalAveragePooling1D()(h2)))
    model.parts, model.norms = (f1, f2, head), (ln1, ln2)

    def ref(P, x):
        q = x.reshape(x.shape[0], T, heads, C // heads).permute(0, 2, 1, 3)
        ctx = torch.matmul(torch.softmax(torch.matmul(q, q.transpose(2, 3)), dim=-1), q).permute(0, 2, 1, 3).reshape(x.shape[0], T, C)
        h1 = t_norm(P, ln1, x + ctx)
        h2 = t_norm(P, ln2, h1 + dense(P, f2, dense(P, f1, h1, 'relu')))
        return dense(P, head, h2.mean(1))
    return model, ref


def test_dense_layernorm_dense_trains_as_torch_fp64():
    model, ref, _ = dense_model()
    rng = np.random.RandomState(31)
    seed_weights(model, rng)
    R.train_and_compare(model, ref, [rng.randn(5, 12).astype(np.float32)], rng.randn(5, 3).astype(np.float32), what='dense-ln-dense')


@pytest.mark.parametrize('heads', [1, 2])
def test_the_encoder_block_trains_as_torch_fp64(heads):
    model, ref = encoder_model(heads)
    assert [type(n.layer).__name__ for n in model.nodes].count('LayerNormalization') == 2
    rng = np.random.RandomState(32 + heads)
    seed_weights(model, rng)
    R.train_and_compare(model, ref, [rng.randn(3, 10, 12).astype(np.float32)], rng.randn(3, 1).astype(np.float32), what='encoder block, heads %d' % heads)


@pytest.mark.parametrize('B,kw', [(2, dict(axis=[-2, -1])), (8, dict(center=False)), (8, dict(scale=False)), (8, dict(center=False, scale=False, axis=[1, 2]))],
                         ids=['two-axes', 'no-center', 'no-scale', 'plain-two-axes'])
def test_axes_and_absent_weights_train_as_torch_fp64(B, kw):
    """Dense -> LayerNormalization -> Flatten -> Dense(3) on (B, 5, 8).  The loss bound of train_and_compare, 1e-6 relative, is a few fp32 ulp of a
    loss that is itself a difference: an output error of 2^-24 |y| is 2^-23 |y| / |y - t| of the loss, so the bound asks for residuals that stay a
    good fraction of the outputs over the three steps.  With B = 2 the 40 x 3 head fits both samples in one step (measured with center=False: loss
    1.075 -> 0.027, error 1.005e-6 of it); B = 8 gives the head more samples than a step can fit."""
    model, ref, ln = dense_model((5, 8), **kw)
    rng = np.random.RandomState(34)
    seed_weights(model, rng)
    assert [p.shape for p in ln.weights] == [(5, 8) if 'axis' in kw else (8,)] * (kw.get('center', True) + kw.get('scale', True))
    R.train_and_compare(model, ref, [rng.randn(B, 5, 8).astype(np.float32)], rng.randn(B, 3).astype(np.float32), what='layer norm %r' % (kw,))


def test_a_frozen_layer_keeps_its_weights_and_passes_the_gradient_on():
    model, ref, ln = dense_model()
    rng = np.random.RandomState(35)
    seed_weights(model, rng)
    ln.trainable = False
    before = [w.copy() for w in ln.get_weights()]
    R.train_and_compare(model, ref, [rng.randn(5, 12).astype(np.float32)], rng.randn(5, 3).astype(np.float32), what='frozen layer norm', frozen=(ln,))
    assert all(np.array_equal(a, b) for a, b in zip(before, ln.get_weights())) and before[0].std() > 0          # the Dense in front of it was compared: dx flows


def test_a_gamma_regularizer_enters_entry_0_of_train_on_batch():
    from gennet_amd import regularizers
    model, ref, ln = dense_model(gamma_regularizer=regularizers.l2(0.05), beta_regularizer=regularizers.l1(0.02))
    rng = np.random.RandomState(36)
    seed_weights(model, rng)
    x, t = rng.randn(5, 12).astype(np.float32), rng.randn(5, 3).astype(np.float32)

    def penalty(P):
        return np.float32(0.05).item() * (P[ln.name][0] ** 2).sum() + np.float32(0.02).item() * P[ln.name][1].abs().sum()
    P = R.train_and_compare(model, ref, [x], t, what='regularized layer norm', penalty=penalty)
    with torch.no_grad():                          # the penalty is more than 1 % of the loss: a dropped one cannot pass the loss bound
        data = float(((ref(P, torch.tensor(x.astype(np.float64))) - torch.tensor(t.astype(np.float64))) ** 2).mean())
        assert float(penalty(P)) > 0.01 * (data + float(penalty(P)))


def test_save_and_load_round_trip(tmp_path):
    from gennet_amd import h5lite
    from gennet_amd.engine import SGD, load_model
    model, _, ln = dense_model((5, 8), axis=[-2, -1], epsilon=1e-5)
    rng = np.random.RandomState(37)
    seed_weights(model, rng)
    x, t = rng.randn(2, 5, 8).astype(np.float32), rng.randn(2, 3).astype(np.float32)
    model.compile(optimizer=SGD(lr=R.LR), loss='mean_squared_error')
    model.train_on_batch(x, t)
    path = os.path.join(str(tmp_path), 'layernorm.h5')
    model.save(path)
    f = h5lite.File(path)
    assert [n.decode() for n in f['model_weights'][ln.name].attrs['weight_names'].tolist()] == [ln.name + '/gamma:0', ln.name + '/beta:0']
    assert f['model_weights'][ln.name][ln.name]['gamma:0'].shape == (5, 8)
    again = load_model(path)
    assert [type(n.layer).__name__ for n in again.nodes] == [type(n.layer).__name__ for n in model.nodes]
    twin = [n.layer for n in again.nodes if type(n.layer).__name__ == 'LayerNormalization'][0]
    assert (twin.axis, twin.epsilon, twin.center, twin.scale) == ([1, 2], 1e-5, True, True) and [p.name for p in twin.weights] == [p.name for p in ln.weights]
    assert all(np.array_equal(a, b) for a, b in zip(twin.get_weights(), ln.get_weights()))
    assert np.array_equal(model.predict(x), again.predict(x))
    a, b = model.train_on_batch(x, t), again.train_on_batch(x, t)
    assert a == b and all(np.array_equal(u, v) for u, v in zip(model.get_weights(), again.get_weights()))


def test_a_captured_step_replays_bit_identically():
    """the encoder block as a hipGraph (engine.StepGraph): eager step, capture, three replays against four eager steps of a twin"""
    from gennet_amd import engine
    from gennet_amd.engine import SGD, to_device
    rng = np.random.RandomState(38)
    x, t = to_device(rng.randn(3, 10, 12).astype(np.float32)), to_device(rng.randn(3, 1).astype(np.float32))
    eager, _ = encoder_model(2)
    seed_weights(eager, rng)
    graphed, _ = encoder_model(2)
    graphed.set_weights(eager.get_weights())
    for m in (eager, graphed):
        m.compile(optimizer=SGD(lr=R.LR, momentum=0.5), loss='mean_squared_error')
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
    assert not np.array_equal(want[0][0], want[3][0])          # the steps differ
