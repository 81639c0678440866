"""The any-channel convolutions (csrc/conv_anyc.hip) on the GPU: forward, data gradient, weight gradient and bias gradient of channel
pairs no strict entry point takes, against fp64 numpy; bounds by their effect (NaN around every input, a sentinel around every output);
run-to-run bit identity; the kernel family each call reaches (launch counters 9 and 10); the aligned shapes untouched (the _any entry points
reach the same kernels with the same bits, the strict ones still refuse); and Conv1D layers over such pairs against an fp64 restatement.

Tolerances are the project's: 2e-5 of the largest reference value for conv outputs and gradients, 1e-6 relative for a loss, 1e-4 of the largest
entry (floor 1e-3) for gradients and trained weights of a layer stack, 1e-5 for predict."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

MATHS = ('fp32', 'wino')
KINDS = (0, 1, 2, 5, 6, 7, 8, 9, 10)      # csrc/common.h prof_end: the counted families; 9 / 10: the anyc conv / weight gradient
PAD = 37                                  # floats of NaN / sentinel on each side of a view: odd, so no view starts on a 16-byte boundary
SENTINEL = -12345.5


def dev():
    return torch.device('cuda:0')


def launches(fn):
    from gennet_amd import ops
    was = ops.prof_enabled()
    ops.prof_enable(True)
    try:
        ops.prof_reset()
        out = fn()
        counts = {k: ops.prof_collect(k)['launches'] for k in KINDS}
    finally:
        ops.prof_enable(was)
    return out, {k: v for k, v in counts.items() if v}


def geometry(L, k, s, padding):
    """(output length, left padding) by TensorFlow's rule, stated here so that the references do not take it from the package under test:
    'valid': ceil((L - k + 1) / s), no padding; 'same': ceil(L / s), total padding max((out - 1) s + k - L, 0), the smaller half on the left."""
    if padding == 'valid':
        return (L - k) // s + 1, 0
    out = -(-L // s)
    return out, max((out - 1) * s + k - L, 0) // 2


# ---- fp64 numpy: the definition and its two adjoints ----------------------------------------------------------------------------------
def _padded(x, k, s, pl, Lout):
    B, L, C = x.shape
    n = max(L + pl, s * (Lout - 1) + k)
    xp = np.zeros((B, n, C))
    xp[:, pl:pl + L] = x
    return xp


def ref_fwd(x, w, b, s, pl, Lout, act):
    k = w.shape[0]
    xp = _padded(x, k, s, pl, Lout)
    y = np.zeros((x.shape[0], Lout, w.shape[2])) + b
    for j in range(k):
        y += xp[:, j:j + s * Lout:s][:, :Lout] @ w[j]
    return {'linear': y, 'relu': np.maximum(y, 0), 'tanh': np.tanh(y)}[act]


def ref_dgrad(dy, w, L, s, pl):
    k = w.shape[0]
    B, Lout, _ = dy.shape
    n = max(L + pl, s * (Lout - 1) + k)
    dxp = np.zeros((B, n, w.shape[1]))
    for j in range(k):
        dxp[:, j:j + s * Lout:s][:, :Lout] += dy @ w[j].T
    return dxp[:, pl:pl + L]


def ref_wgrad(x, dy, k, s, pl):
    Lout = dy.shape[1]
    xp = _padded(x, k, s, pl, Lout)
    dw = np.stack([np.einsum('btc,btn->cn', xp[:, j:j + s * Lout:s][:, :Lout], dy) for j in range(k)])
    return dw, dy.sum((0, 1))


def rel(a, ref):
    a = np.asarray(a, np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-30)


# ---- guarded buffers ------------------------------------------------------------------------------------------------------------------
class Guarded(object):
    """A contiguous view into a larger flat buffer: inputs surrounded by NaN, outputs inside a sentinel-filled buffer."""

    def __init__(self, shape, value=None):
        n = int(np.prod(shape))
        self.n = n
        self.buf = torch.full((n + 2 * PAD,), float('nan') if value is not None else SENTINEL, dtype=torch.float32, device=dev())
        self.t = self.buf[PAD:PAD + n].view(shape)
        if value is not None:
            self.t.copy_(torch.tensor(np.asarray(value, np.float32), device=dev()))
        assert self.t.is_contiguous() and self.t.data_ptr() == self.buf.data_ptr() + 4 * PAD

    def refill(self):
        self.buf.fill_(SENTINEL)

    def check(self, what):
        """the surroundings untouched, every element of the view written and finite"""
        edges = torch.cat([self.buf[:PAD], self.buf[PAD + self.n:]])
        assert bool((edges == SENTINEL).all()), '%s: wrote outside its output' % what
        assert bool(torch.isfinite(self.t).all()), '%s: non-finite output (an element outside an input was read)' % what
        assert not bool((self.t == SENTINEL).any()), '%s: output elements left unwritten' % what
        return self.t.cpu().numpy()


CASES = [
    # B, L, Cin, Cout, k, stride, padding
    (3, 50, 4, 50, 4, 1, 'valid'),          # d_model's tap-folded layer
    (2, 40, 1, 1, 3, 1, 'same'),
    (2, 41, 3, 3, 5, 2, 'same'),
    (2, 64, 5, 5, 1, 1, 'valid'),
    (2, 100, 7, 64, 5, 1, 'same'),
    (2, 100, 64, 7, 5, 2, 'same'),
    (2, 37, 6, 10, 3, 2, 'valid'),
    (4, 300, 50, 30, 5, 1, 'same'),
    (1, 700, 50, 100, 2, 1, 'valid'),
    (2, 300, 130, 258, 5, 2, 'same'),       # several N tiles, a ragged last K chunk and a ragged last N tile at once
    (2, 131, 9, 11, 4, 2, 'same'),          # even tap count at stride 2: two 2-tap phases
    (1, 5, 2, 3, 5, 1, 'same'),             # shorter than one tile in every direction
    # the boundary of the small-channel dispatchers: Cin <= 4 goes to the small-Cin kernels whatever Cout is, and they need Cout % 4 == 0
    (2, 50, 4, 3, 3, 1, 'same'),            # forward and weight gradient anyc; the data gradient (3 -> 4) strict
    (2, 50, 4, 1, 4, 1, 'valid'),           # Conv1D(1, 16) on one channel, tap-folded
    (2, 50, 3, 4, 3, 1, 'same'),            # forward and weight gradient strict; the data gradient (4 -> 3) anyc
    (2, 51, 2, 4, 5, 2, 'same'),
]


@pytest.mark.parametrize('math', MATHS)
@pytest.mark.parametrize('B,L,Cin,Cout,k,s,padding', CASES, ids=['-'.join(str(v) for v in c) for c in CASES])
def test_any_channel_pairs_parity_bounds_determinism_and_family(B, L, Cin, Cout, k, s, padding, math):
    from gennet_amd import _lib, ops
    fwd_any, dgrad_any = ops.conv_needs_any(Cin, Cout), ops.conv_needs_any(Cout, Cin)     # the data gradient runs the swapped pair
    assert fwd_any or dgrad_any
    fwd_kinds, wgrad_kinds = ({9: 1}, {10: 1}) if fwd_any else ({}, {})                   # (the small-channel kernels are counted apart: conv_family.SMALL_KINDS)
    rng = np.random.RandomState(B * 1000 + L + Cin * 7 + Cout)
    Lout, pl = geometry(L, k, s, padding)
    assert (Lout, pl) == tuple(ops.conv_geometry(L, k, s, padding))
    x = rng.randn(B, L, Cin).astype(np.float32).astype(np.float64)
    w = (rng.randn(k, Cin, Cout) / np.sqrt(k * Cin)).astype(np.float32).astype(np.float64)
    b = rng.randn(Cout).astype(np.float32).astype(np.float64)
    dy = rng.randn(B, Lout, Cout).astype(np.float32).astype(np.float64)
    X, W, Bi, DY = Guarded(x.shape, x), Guarded(w.shape, w), Guarded(b.shape, b), Guarded(dy.shape, dy)
    WT = Guarded((k, Cout, Cin), np.ascontiguousarray(w.transpose(0, 2, 1)))
    st = ops._stream
    phases = min(s, L)
    with ops.conv_math(math):
        # forward, every activation: raw entry point on guarded views, then the ops wrapper (same bits)
        for act in ('linear', 'relu', 'tanh'):
            Y = Guarded((B, Lout, Cout))
            _, got = launches(lambda: _lib.call('gn_conv1d_fwd_any', X.t.data_ptr(), W.t.data_ptr(), Bi.t.data_ptr(), Y.t.data_ptr(), B, L, Cin, Cout, k, s, pl,
                                               Lout, ops.ACT[act], 0.0, st()))
            assert got == fwd_kinds, got
            y = Y.check('forward ' + act)
            err = rel(y, ref_fwd(x, w, b, s, pl, Lout, act))
            print('fwd %s err %.3g' % (act, err))
            assert err < 2e-5
            y2 = ops.conv1d_fwd(X.t, W.t, Bi.t, s, pl, Lout, act, any_channels=True)
            assert torch.equal(y2, Y.t)
        # no bias
        y0 = ops.conv1d_fwd(X.t, W.t, None, s, pl, Lout, any_channels=True)
        assert rel(y0.cpu().numpy(), ref_fwd(x, w, 0.0, s, pl, Lout, 'linear')) < 2e-5
        # data gradient: one launch at unit stride, one per phase otherwise
        DX = Guarded((B, L, Cin))
        _, got = launches(lambda: _lib.call('gn_conv1d_dgrad_any', DY.t.data_ptr(), WT.t.data_ptr(), DX.t.data_ptr(), B, L, Cin, Cout, k, s, pl, Lout, st()))
        assert got == ({9: phases} if dgrad_any else {}), got
        dx = DX.check('data gradient')
        err = rel(dx, ref_dgrad(dy, w, L, s, pl))
        print('dgrad err %.3g' % err)
        assert err < 2e-5
        dx2 = ops.conv1d_dgrad(DY.t, WT.t, L, s, pl, any_channels=True)
        assert torch.equal(dx2, DX.t)
        assert torch.equal(ops.conv1d_transpose_w(W.t), WT.t)
        # weight and bias gradient
        DW, DB = Guarded((k, Cin, Cout)), Guarded((Cout,))
        (dw_t, db_t), got = launches(lambda: ops.conv1d_wgrad(X.t, DY.t, k, s, pl, DW.t, DB.t, any_channels=True))
        assert got == wgrad_kinds, got
        dw, db = DW.check('weight gradient'), DB.check('bias gradient')
        dw_ref, db_ref = ref_wgrad(x, dy, k, s, pl)
        print('wgrad err %.3g db err %.3g' % (rel(dw, dw_ref), rel(db, db_ref)))
        assert rel(dw, dw_ref) < 2e-5 and rel(db, db_ref) < 2e-5
        DW2, DB2 = Guarded((k, Cin, Cout)), Guarded((Cout,))
        ops.conv1d_wgrad(X.t, DY.t, k, s, pl, DW2.t, DB2.t, any_channels=True)
        assert torch.equal(DW.t, DW2.t) and (Cout <= 4 or torch.equal(DB.t, DB2.t))
        dw3, db3 = ops.conv1d_wgrad(X.t, DY.t, k, s, pl, want_db=False, any_channels=True)
        assert db3 is None and torch.equal(dw3, DW.t)
        # the strict entry points still refuse the pair, in the directions the predicate names, and run the others with the same bits
        for refused, call, same in ((fwd_any, lambda: ops.conv1d_fwd(X.t, W.t, Bi.t, s, pl, Lout, 'tanh'), Y.t),
                                    (dgrad_any, lambda: ops.conv1d_dgrad(DY.t, WT.t, L, s, pl), DX.t),
                                    (fwd_any, lambda: ops.conv1d_wgrad(X.t, DY.t, k, s, pl)[0], DW.t)):
            if refused:
                with pytest.raises(_lib.GennetHipError):
                    call()
            else:
                assert torch.equal(call(), same)
    torch.cuda.synchronize()


ALIGNED = [
    # B, L, Cin, Cout, k, stride, padding, math: at least one shape per existing family under its math
    (2, 96, 1, 64, 5, 1, 'same', 'fp32'), (2, 96, 1, 64, 5, 2, 'same', 'wino'),       # small-Cin
    (2, 64, 256, 1, 5, 1, 'same', 'fp32'), (2, 50, 64, 4, 5, 2, 'same', 'wino'),      # small-Cout
    (2, 50, 16, 64, 3, 1, 'same', 'fp32'), (3, 66, 32, 64, 4, 2, 'same', 'wino'),     # direct; stride 2 in phases
    (2, 70, 64, 64, 5, 1, 'same', 'fp32'), (2, 70, 64, 64, 5, 1, 'same', 'wino'),     # direct | wino in all three directions
    (2, 150, 64, 128, 5, 2, 'valid', 'fp32'),                                        # direct with the merged data gradient
    (2, 150, 64, 128, 5, 2, 'valid', 'wino'),                                        # wino_s2 in all three directions
    (2, 90, 64, 24, 5, 2, 'same', 'wino'),                                           # merged data gradient under wino
]


def test_aligned_shapes_reach_the_same_kernels_with_the_same_bits():
    from gennet_amd import ops
    seen = set()
    for B, L, Cin, Cout, k, s, padding, math in ALIGNED:
        assert not ops.conv_needs_any(Cin, Cout)
        rng = np.random.RandomState(L + Cin + Cout)
        Lout, pl = geometry(L, k, s, padding)
        X = torch.tensor(rng.randn(B, L, Cin).astype(np.float32), device=dev())
        W = torch.tensor((rng.randn(k, Cin, Cout) / np.sqrt(k * Cin)).astype(np.float32), device=dev())
        Bi = torch.tensor(rng.randn(Cout).astype(np.float32), device=dev())
        DY = torch.tensor(rng.randn(B, Lout, Cout).astype(np.float32), device=dev())
        WT = ops.conv1d_transpose_w(W)
        with ops.conv_math(math):
            for name, call in (('fwd', lambda a: (ops.conv1d_fwd(X, W, Bi, s, pl, Lout, 'relu', any_channels=a),)),
                               ('dgrad', lambda a: (ops.conv1d_dgrad(DY, WT, L, s, pl, any_channels=a),)),
                               ('wgrad', lambda a: ops.conv1d_wgrad(X, DY, k, s, pl, any_channels=a))):
                strict, n_strict = launches(lambda: call(False))
                anyc, n_any = launches(lambda: call(True))
                assert n_strict == n_any and 9 not in n_any and 10 not in n_any, (name, B, L, Cin, Cout, k, s, math, n_strict, n_any)
                for p, q in zip(strict, anyc):
                    assert torch.equal(p, q), (name, B, L, Cin, Cout, k, s, math)
                seen |= set(n_any)
    assert seen >= {0, 1, 5, 6, 7, 8}, seen          # the table reached every counted family (the small kernels are counted apart: conv_family.SMALL_KINDS, tests/test_small_conv_gpu.py)


def test_predicate_is_what_the_strict_dispatchers_refuse():
    """ops.conv_needs_any against the dispatchers themselves, not against a formula: every pair up to 13 x 13 on a tiny input, strict forward
    and weight gradient refuse exactly where the predicate says so, the strict data gradient where it says so for the swapped pair."""
    from gennet_amd import _lib, ops

    def refuses(call):
        try:
            call()
        except _lib.GennetHipError:
            return True
        return False

    for Cin in range(1, 14):
        for Cout in range(1, 14):
            x = torch.zeros((1, 8, Cin), device=dev()); w = torch.zeros((3, Cin, Cout), device=dev()); dy = torch.zeros((1, 8, Cout), device=dev())
            wt = ops.conv1d_transpose_w(w)
            assert refuses(lambda: ops.conv1d_fwd(x, w, None, 1, 1, 8)) == ops.conv_needs_any(Cin, Cout), (Cin, Cout)
            assert refuses(lambda: ops.conv1d_wgrad(x, dy, 3, 1, 1)) == ops.conv_needs_any(Cin, Cout), (Cin, Cout)
            assert refuses(lambda: ops.conv1d_dgrad(dy, wt, 8, 1, 1)) == ops.conv_needs_any(Cout, Cin), (Cin, Cout)
            for call in (lambda: ops.conv1d_fwd(x, w, None, 1, 1, 8, any_channels=True), lambda: ops.conv1d_wgrad(x, dy, 3, 1, 1, any_channels=True),
                         lambda: ops.conv1d_dgrad(dy, wt, 8, 1, 1, any_channels=True)):
                assert not refuses(call), (Cin, Cout)
    torch.cuda.synchronize()


@pytest.mark.parametrize('Cin,Cout', [(6, 10), (4, 50), (50, 4)])
def test_strict_entry_points_still_refuse(Cin, Cout):
    from gennet_amd import _lib, ops
    x = torch.zeros((2, 16, Cin), device=dev()); w = torch.zeros((3, Cin, Cout), device=dev()); dy = torch.zeros((2, 16, Cout), device=dev())
    with pytest.raises(_lib.GennetHipError):
        ops.conv1d_fwd(x, w, None, 1, 1, 16)
    with pytest.raises(_lib.GennetHipError):
        ops.conv1d_dgrad(dy, ops.conv1d_transpose_w(w), 16, 1, 1)
    with pytest.raises(_lib.GennetHipError):
        ops.conv1d_wgrad(x, dy, 3, 1, 1)
    # and the workspace query answers for such a pair
    assert _lib.size('gn_conv1d_wgrad_workspace', 2, 16, Cin, Cout, 3, 1, 16) >= 4 * 3 * Cin * Cout


# ---- layer level: a Sequential of Conv1D / LeakyReLU / Activation / Dropout / BatchNormalization / UpSampling1D against torch fp64 autograd ----
def _ref_forward(spec, P, x, masks, training, moving):
    """spec: [(kind, ...)]; P: {index: [tensors]}; x (B, L, C) float64, channels last."""
    h = x
    for i, s in enumerate(spec):
        if s[0] == 'conv':
            _, filters, k, stride, padding = s
            Lout, pl = geometry(h.shape[1], k, stride, padding)
            need = max(h.shape[1] + pl, stride * (Lout - 1) + k)
            hp = F.pad(h.permute(0, 2, 1), (pl, need - h.shape[1] - pl))
            h = F.conv1d(hp, P[i][0].permute(2, 1, 0), stride=stride)[:, :, :Lout].permute(0, 2, 1) + P[i][1]
        elif s[0] == 'leaky':
            h = torch.where(h > 0, h, float(np.float32(s[1])) * h)
        elif s[0] == 'tanh':
            h = torch.tanh(h)
        elif s[0] == 'drop':
            if training:
                h = h * masks[i] / (1.0 - s[1])
        elif s[0] == 'bn':
            if training:
                mean = h.mean(dim=(0, 1)); var = ((h - mean) ** 2).mean(dim=(0, 1))
            else:
                mean, var = moving[i]
            h = (h - mean) / torch.sqrt(var + 1e-3) * P[i][0] + P[i][1]
        elif s[0] == 'up':
            h = h.repeat_interleave(2, dim=1)
    return h


def _build(spec, in_shape):
    from gennet_amd import layers as Ly
    from gennet_amd.engine import Sequential
    ls = []
    for i, s in enumerate(spec):
        kw = {'input_shape': in_shape} if i == 0 else {}
        if s[0] == 'conv':
            ls.append(Ly.Conv1D(s[1], s[2], strides=s[3], padding=s[4], **kw))
        elif s[0] == 'leaky':
            ls.append(Ly.LeakyReLU(s[1], **kw))
        elif s[0] == 'tanh':
            ls.append(Ly.Activation('tanh', **kw))
        elif s[0] == 'drop':
            ls.append(Ly.Dropout(s[1], **kw))
        elif s[0] == 'bn':
            ls.append(Ly.BatchNormalization(**kw))
        elif s[0] == 'up':
            ls.append(Ly.UpSampling1D(2, **kw))
    return Sequential(ls), ls


NETS = {
    'd_model_conv': ((50, 1), [('conv', 50, 16, 1, 'valid'), ('leaky', 0.2)]),
    # one filter over 16 taps on one channel folds to 4 -> 1 (small-Cin refuses it); then 3 -> 4, whose data gradient alone (4 -> 3) is ragged
    'one_filter': ((50, 1), [('conv', 3, 16, 1, 'valid'), ('leaky', 0.2), ('conv', 4, 3, 1, 'same'), ('tanh',), ('conv', 1, 17, 1, 'valid')]),
    # a fused activation, a declined fused Dropout, a declined producer-gradient fusion
    'act_drop_conv': ((64, 50), [('conv', 30, 5, 2, 'same'), ('leaky', 0.2), ('drop', 0.3), ('conv', 12, 3, 1, 'valid')]),
    # BatchNormalization over 30 channels with its fused activation and Dropout, then ragged Cin into aligned filters in front of a BatchNormalization
    'bn_chain': ((80, 8), [('conv', 30, 5, 1, 'valid'), ('bn',), ('tanh',), ('drop', 0.25), ('conv', 32, 5, 2, 'valid'), ('bn',)]),
    # UpSampling1D(2) -> Conv1D(6, 5, 'same') on 5 channels: folded by the planner into a 3-tap conv with 2 * 6 columns, pair (5, 12); the fold
    # needs a layer in front of the upsample (the planner does not fold a graph input), itself a ragged pair with a declined producer gradient
    'upsample': ((40, 3), [('conv', 5, 3, 1, 'same'), ('leaky', 0.2), ('up',), ('conv', 6, 5, 1, 'same')]),
}


@pytest.mark.parametrize('math', MATHS)
@pytest.mark.parametrize('net', sorted(NETS))
def test_conv1d_layers_over_any_channel_pairs_train_and_predict(net, math):
    from gennet_amd import ops
    from gennet_amd.engine import SGD
    in_shape, spec = NETS[net]
    B, lr = 6, 0.05
    rng = np.random.RandomState(len(net))
    model, ls = _build(spec, in_shape)
    # seeded biases, BatchNormalization parameters and moving statistics (the zero / one initial values would hide them)
    for l, s in zip(ls, spec):
        ws = l.get_weights()
        if s[0] == 'conv':
            l.set_weights([ws[0], rng.randn(*ws[1].shape).astype(np.float32) * 0.1])
        elif s[0] == 'bn':
            C = ws[0].shape[0]
            l.set_weights([1 + 0.2 * rng.randn(C), 0.2 * rng.randn(C), 0.3 * rng.randn(C), 0.5 + rng.rand(C)])
    model.compile(optimizer=SGD(lr=lr), loss='mean_squared_error')
    model._plan()
    assert ('up',) not in spec or [n.fold_up is not None for n in model.nodes if n.layer is ls[-1]] == [True]
    x = rng.randn(B, *in_shape).astype(np.float32)
    out_shape = tuple(model.output_shape[1:])
    t = rng.randn(B, *out_shape).astype(np.float32)
    P = {i: [torch.tensor(w.astype(np.float64), requires_grad=True) for w in l.get_weights()[:2]] for i, (l, s) in enumerate(zip(ls, spec)) if s[0] in ('conv', 'bn')}
    moving = {i: [torch.tensor(w.astype(np.float64)) for w in l.get_weights()[2:]] for i, (l, s) in enumerate(zip(ls, spec)) if s[0] == 'bn'}
    # shapes of the dropout inputs, for the injected masks
    masks, masks_named = {}, {}
    shp = (B,) + tuple(in_shape)
    with torch.no_grad():
        h = torch.zeros(shp, dtype=torch.float64)
        for i, s in enumerate(spec):
            if s[0] == 'drop':
                m = (rng.rand(*h.shape) >= s[1])
                masks[i] = torch.tensor(m.astype(np.float64)); masks_named[ls[i].name] = m.astype(np.uint8)
            h = _ref_forward([s], {0: P.get(i)}, h, {0: masks.get(i)}, True, {0: moving.get(i)})
    with ops.conv_math(math):
        (y, counts) = launches(lambda: model.predict(x, batch_size=B))
        with torch.no_grad():
            y_ref = _ref_forward(spec, P, torch.tensor(x.astype(np.float64)), masks, False, moving).numpy()
        print(net, math, 'predict launches', counts, 'err', rel(y, y_ref))
        assert 9 in counts and rel(y, y_ref) < 1e-5
        loss_ref = ((_ref_forward(spec, P, torch.tensor(x.astype(np.float64)), masks, True, moving) - torch.tensor(t.astype(np.float64))) ** 2).mean()
        loss_ref.backward()
        (res, counts) = launches(lambda: model.train_on_batch(x, t, dropout_masks=masks_named))
        print(net, math, 'train launches', counts, 'loss', res[0], float(loss_ref.detach()))
        assert 9 in counts and 10 in counts
        assert abs(res[0] - float(loss_ref.detach())) <= 1e-6 * abs(float(loss_ref.detach()))
        # a conv bias in front of a BatchNormalization has a zero gradient in exact arithmetic (the normalisation removes it) and holds rounding
        # noise only: a gradient is measured against its own largest entry, but no finer than 1e-3 of the model's largest gradient entry (the
        # weight floor of 1e-3, carried over to gradients, which have no unit scale of their own)
        g_floor = 1e-3 * max(float(t.grad.abs().max()) for ts in P.values() for t in ts)
        for i, (l, s) in enumerate(zip(ls, spec)):
            if i not in P:
                continue
            for p, ref in zip(l.params, P[i]):
                g_ref = ref.grad.numpy()
                g = p.grad.detach().cpu().numpy().reshape(g_ref.shape)
                gerr = np.abs(g - g_ref).max() / max(np.abs(g_ref).max(), g_floor)
                w_ref = (ref.detach() - lr * ref.grad).numpy()
                werr = np.abs(p.numpy().astype(np.float64) - w_ref).max() / max(np.abs(w_ref).max(), 1e-3)
                print(net, math, l.name, p.name, 'grad err %.3g weight err %.3g' % (gerr, werr))
                assert gerr < 1e-4 and werr < 1e-4, (l.name, p.name, gerr, werr)
