"""Conv2DTranspose on the GPU against torch CPU fp64 (F.conv_transpose2d with weight W.permute(3, 2, 0, 1), 'same' cropped at TF's left
padding), under each conv math, and the kernel family each direction reaches; the bias / activation / dropout pass of csrc/conv_transpose.hip;
and the column reductions and BatchNormalization over channel counts that are not multiples of 4."""
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_family as CF
from oracle import keras_ref as K

pytestmark = pytest.mark.gpu

RTOL = 2e-5


def g(a, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=torch.device('cuda:0'))


def rel(t, ref):
    a = t.detach().cpu().numpy().astype(np.float64) if isinstance(t, torch.Tensor) else np.asarray(t, np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-30)


_TORCH_ACT = {'linear': lambda v: v, 'relu': torch.relu, 'tanh': torch.tanh, 'sigmoid': torch.sigmoid}


def torch_ref(x, w, b, dy, s, padding, act):
    """fp64 forward and gradients of keras' Conv2DTranspose (channels_last, kernel (1, kw), strides (1, s))."""
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    wt = torch.tensor(w, dtype=torch.float64, requires_grad=True)
    bt = torch.tensor(b, dtype=torch.float64, requires_grad=True)
    W, kw = x.shape[2], w.shape[1]
    Wout = W * s + max(kw - s, 0) if padding == 'valid' else W * s
    full = F.conv_transpose2d(xt.permute(0, 3, 1, 2).contiguous(), wt.permute(3, 2, 0, 1).contiguous(), stride=(1, s), padding=0)
    pl = max((W - 1) * s + kw - Wout, 0) // 2 if padding == 'same' else 0
    y = _TORCH_ACT[act](full[:, :, :, pl:pl + Wout].permute(0, 2, 3, 1) + bt)
    (y * torch.tensor(dy, dtype=torch.float64)).sum().backward()
    return y.detach().numpy(), xt.grad.numpy(), wt.grad.numpy(), bt.grad.numpy()


def run_layer(layer, x, w, b, dy, training=True, node=None):
    from gennet_amd.engine import RunContext
    layer.build(x.shape[1:])
    layer.kernel.assign(w); layer.bias.assign(b)
    layer.kernel.grad = torch.zeros(w.shape, dtype=torch.float32, device='cuda:0')
    layer.bias.grad = torch.zeros(b.shape, dtype=torch.float32, device='cuda:0')
    node = node or types.SimpleNamespace(index=0, fused_act=None, fused_drop=None)
    ctx = RunContext(training)
    y = layer.forward(ctx, node, g(x))
    dx = layer.backward(ctx, node, g(dy), True, True)
    return y, dx, layer.kernel.grad, layer.bias.grad


CASES = [
    # B, H, W, Cin, filters, kw, s, padding, act
    (2, 1, 1, 1, 128, 4, 1, 'valid', 'relu'),       # the reference's g_model.hdf5, layer by layer
    (2, 1, 4, 128, 64, 8, 1, 'valid', 'relu'),
    (2, 1, 11, 64, 32, 16, 1, 'valid', 'relu'),
    (2, 1, 26, 32, 16, 32, 1, 'valid', 'relu'),
    (2, 3, 37, 3, 16, 3, 2, 'same', 'tanh'),
    (1, 3, 100, 32, 64, 5, 2, 'same', 'linear'),
    (2, 1, 257, 128, 256, 4, 2, 'valid', 'sigmoid'),
    (2, 3, 64, 32, 1, 5, 1, 'same', 'tanh'),
    (2, 1, 1000, 16, 16, 1, 1, 'valid', 'linear'),
    (1, 1, 1024, 128, 64, 5, 2, 'same', 'relu'),
    (2, 3, 50, 3, 64, 8, 2, 'valid', 'relu'),
    (2, 1, 300, 32, 256, 16, 2, 'same', 'tanh'),
    (2, 3, 9, 1, 16, 32, 1, 'same', 'linear'),
]
_ORACLE = CF.OneCase()


def _case(B, H, W, Cin, Fl, kw, s, padding, act):
    rng = np.random.RandomState(7 * W + kw + s)
    x = rng.randn(B, H, W, Cin).astype(np.float32)
    lim = np.sqrt(6.0 / ((Fl + Cin) * kw))
    w = rng.uniform(-lim, lim, (1, kw, Fl, Cin)).astype(np.float32)
    b = (rng.randn(Fl) * 0.1).astype(np.float32)
    Wout = W * s + max(kw - s, 0) if padding == 'valid' else W * s
    dy = rng.randn(B, H, Wout, Fl).astype(np.float32)
    return (x, w, b, dy) + torch_ref(x.astype(np.float64), w.astype(np.float64), b.astype(np.float64), dy.astype(np.float64), s, padding, act)


@pytest.mark.parametrize('B,H,W,Cin,Fl,kw,s,padding,act,math', CF.per_math(CASES, 8))
def test_conv2d_transpose_matches_torch_fp64(B, H, W, Cin, Fl, kw, s, padding, act, math):
    from gennet_amd import ops, layers as L
    x, w, b, dy, y_ref, dx_ref, dw_ref, db_ref = _ORACLE.get((B, H, W, Cin, Fl, kw, s, padding, act),
                                                             lambda: _case(B, H, W, Cin, Fl, kw, s, padding, act))
    with ops.conv_math(math):
        layer = L.Conv2DTranspose(Fl, (1, kw), strides=(1, s), padding=padding, activation=act)
        y, dx, dw, db = run_layer(layer, x, w, b, dy)
    assert rel(y, y_ref) < RTOL
    assert rel(dx, dx_ref) < RTOL
    assert rel(dw, dw_ref) < RTOL
    assert rel(db, db_ref) < RTOL


FAMILY_CASES = [
    (2, 1, 64, 64, 128, 5, 1, 'same'),
    (2, 1, 128, 64, 64, 5, 2, 'same'),
    (2, 3, 40, 3, 16, 4, 2, 'valid'),
    (2, 1, 1024, 1024, 512, 5, 2, 'same'),      # the PE net's last Conv1D(1024, 5, strides=2), transposed
    (2, 1, 26, 32, 16, 32, 1, 'valid'),         # g_model's conv2d_transpose_4: the tap fold (7 groups of 5 taps over 16 filters)
    (2, 3, 50, 16, 64, 8, 2, 'same'),           # tap fold, stride 2
]


@pytest.mark.parametrize('B,H,W,Cin,Fl,kw,s,padding,math', CF.per_math(FAMILY_CASES, 8))
def test_each_direction_reaches_the_family_of_the_adjoint_conv1d(B, H, W, Cin, Fl, kw, s, padding, math):
    """forward = the adjoint Conv1D's data gradient, data gradient = its forward, weight gradient = its weight gradient: the same launches."""
    from gennet_amd import ops, layers as L
    from gennet_amd.engine import RunContext
    rng = np.random.RandomState(3)
    layer = L.Conv2DTranspose(Fl, (1, kw), strides=(1, s), padding=padding)
    Wout = layer.out_length(W)
    _, pl = ops.conv_geometry(Wout, kw, s, padding)
    x = g(rng.randn(B, H, W, Cin)); dy = g(rng.randn(B, H, Wout, Fl))
    wadj = g(rng.randn(kw, Fl, Cin) * 0.05)
    with ops.conv_math(math):
        layer.build((H, W, Cin))
        layer.kernel.assign(wadj.cpu().numpy().reshape(1, kw, Fl, Cin))
        layer.kernel.grad = torch.zeros((1, kw, Fl, Cin), device='cuda:0'); layer.bias.grad = torch.zeros((Fl,), device='cuda:0')
        node = types.SimpleNamespace(index=0, fused_act=None, fused_drop=None)
        ctx = RunContext(True)
        _, fwd = CF.launches(lambda: layer.forward(ctx, node, x))
        saved = ctx.tape[0]
        x3, dy3 = x.view(B * H, W, Cin), dy.view(B * H, Wout, Fl)
        # the adjoint Conv1D (kw taps, Fl -> Cin, stride s, pad pl over Wout rows) as Conv1D runs it: past 5 taps, h-tap groups over the folded input
        adj_dgrad = lambda: L._kconv_dgrad(x3, wadj, kw, Wout, s, pl)                   # noqa: E731
        adj_fwd = lambda: L._kconv_fwd(dy3, wadj, None, s, pl, W)                       # noqa: E731
        adj_wgrad = lambda: L._kconv_wgrad(dy3, x3, kw, s, pl, want_db=False)           # noqa: E731
        assert fwd == CF.launches(adj_dgrad)[1]
        # data gradient alone, then weight gradient alone
        _, bwd_dx = CF.launches(lambda: layer.backward(ctx, node, dy, True, False))
        assert bwd_dx == CF.launches(adj_fwd)[1]
        ctx.tape[0] = saved
        _, bwd_dw = CF.launches(lambda: layer.backward(ctx, node, dy, False, True))
        assert bwd_dw == CF.launches(adj_wgrad)[1]


@pytest.mark.parametrize('C', [1, 3, 16, 50, 913])
def test_bias_act_dropout_pass_draws_the_dropout_mask(C):
    """gn_bias_act_dropout: act(y + b), the keep-mask drawn as gn_dropout_mask draws it (same seed / offset, bit for bit), and the given-mask form."""
    from gennet_amd import ops
    rng = np.random.RandomState(C)
    rows = 37
    y0 = rng.randn(rows, C).astype(np.float32); b = rng.randn(C).astype(np.float32)
    rate, seed, off = 0.3, 1234, 40
    y = g(y0)
    mask = torch.empty((rows, C), dtype=torch.uint8, device='cuda:0')
    ops.bias_act_dropout(y, g(b), 'tanh', 0.0, mask, rate, gen=(seed, off))
    want_mask = ops.dropout_mask((rows, C), rate, seed, off, torch.device('cuda:0'))
    assert torch.equal(mask, want_mask)
    m = want_mask.cpu().numpy().astype(np.float64)
    ref = np.tanh(y0.astype(np.float64) + b) * m / (1 - rate)
    assert rel(y, ref) < 1e-6
    y2 = g(y0)
    ops.bias_act_dropout(y2, g(b), 'tanh', 0.0, want_mask, rate)
    assert torch.equal(y2, y)
    y3 = g(y0)
    ops.bias_act_dropout(y3, g(b), 'relu')
    assert rel(y3, np.maximum(y0.astype(np.float64) + b, 0)) < 1e-7


def test_fused_dropout_after_conv2d_transpose_uses_the_dropout_stream():
    from gennet_amd import ops, layers as L
    from gennet_amd.engine import RunContext, device_rng
    rng = np.random.RandomState(5)
    x = rng.randn(2, 3, 20, 8).astype(np.float32)
    layer = L.Conv2DTranspose(2, (1, 4), strides=(1, 2), padding='same', activation='relu')      # 2 filters: the pass's any-C path
    layer.build((3, 20, 8))
    drop = L.Dropout(0.25)
    node = types.SimpleNamespace(index=0, fused_act=None, fused_drop=(0.25, drop))
    seed, off = device_rng().take(0)
    y = layer.forward(RunContext(True), node, g(x))
    want = ops.dropout_mask(tuple(y.shape), 0.25, seed, off, torch.device('cuda:0'))
    plain = layer.forward(RunContext(False), types.SimpleNamespace(index=1, fused_act=None, fused_drop=None), g(x))
    keep = want.bool()
    assert torch.equal(y == 0, ~keep | (plain == 0))
    ref = torch.where(keep, plain.double() / (1 - 0.25), torch.zeros_like(plain.double()))
    assert (y.double() - ref).abs().max().item() <= 1e-6 * ref.abs().max().item()


ANY_C = [1, 2, 3, 5, 50, 913]


@pytest.mark.parametrize('C', ANY_C)
def test_bias_grad_and_bn_stats_over_any_channel_count(C):
    from gennet_amd import ops
    rng = np.random.RandomState(C)
    for rows in (1, 7, 3000):
        x = rng.randn(rows, C).astype(np.float32)
        db = ops.bias_grad(g(x))
        assert rel(db, x.astype(np.float64).sum(0)) < 1e-6
        sums = ops.bn_stats(g(x))
        ref = np.concatenate([x.astype(np.float64).sum(0), (x.astype(np.float64) ** 2).sum(0)])
        assert np.abs(sums.cpu().numpy() - ref).max() <= 1e-9 * max(1.0, np.abs(ref).max())
        if C > 4:          # the fixed-order reduction: bit-identical runs (C <= 4 keeps its atomics path)
            assert torch.equal(db, ops.bias_grad(g(x)))
        assert torch.equal(sums, ops.bn_stats(g(x)))


@pytest.mark.parametrize('C', ANY_C)
@pytest.mark.parametrize('act,rate', [('linear', 0.0), ('relu', 0.0), ('tanh', 0.3)])
def test_batchnorm_over_any_channel_count(C, act, rate):
    """BatchNormalization training forward (fused activation and dropout), backward, moving statistics with zero-debias, and inference,
    against the fp64 oracle; two backward runs bit-identical."""
    from gennet_amd import ops, layers as L
    from gennet_amd.engine import RunContext
    rng = np.random.RandomState(C + 11)
    rows = 300
    x = (rng.randn(rows, C) * 2 + 0.5).astype(np.float32)
    dy = rng.randn(rows, C).astype(np.float32)
    bn = L.BatchNormalization()
    bn.build((C,))
    gam = (1 + 0.1 * rng.randn(C)).astype(np.float32); bet = (0.1 * rng.randn(C)).astype(np.float32)
    bn.gamma.assign(gam); bn.beta.assign(bet)
    bn.gamma.grad = torch.zeros(C, device='cuda:0'); bn.beta.grad = torch.zeros(C, device='cuda:0')
    drop = L.Dropout(rate) if rate else None
    node = types.SimpleNamespace(index=0, fused_act=None if act == 'linear' else (act, 0.0), fused_drop=(rate, drop) if rate else None)
    mask = (rng.rand(rows, C) >= rate).astype(np.uint8)
    ctx = RunContext(True, dropout_masks={drop.name: g(mask, torch.uint8)} if rate else None, site='m')
    y = bn.forward(ctx, node, g(x))
    tape = dict(ctx.tape)
    dx = bn.backward(ctx, node, g(dy), True, True)
    dgam, dbet = bn.gamma.grad.clone(), bn.beta.grad.clone()
    ctx.tape = tape
    dx2 = bn.backward(ctx, node, g(dy), True, True)
    assert torch.equal(dx, dx2) and torch.equal(bn.gamma.grad, dgam)

    x64 = x.astype(np.float64)
    z, cache, mean, var = K.bn_train_fwd(x64, gam.astype(np.float64), bet.astype(np.float64))
    a = K.act_fwd(z, act)
    m = mask.astype(np.float64) if rate else 1.0
    y_ref = a * m / (1 - rate)
    assert rel(y, y_ref) < 2e-5
    dz = K.act_bwd(dy.astype(np.float64) * m / (1 - rate), a, act)
    dx_ref, dg_ref, db_ref = K.bn_train_bwd(dz, cache, gam.astype(np.float64))
    assert rel(dx, dx_ref) < 2e-5 and rel(dgam, dg_ref) < 2e-5 and rel(dbet, db_ref) < 2e-5
    mm, mv, _ = K.bn_moving_update_zero_debias(np.zeros(C), np.ones(C), [np.zeros(C), np.zeros(C), 0], mean, var, rows, 0.99)
    assert rel(bn.moving_mean.data, mm) < 1e-5 and rel(bn.moving_variance.data, mv) < 1e-5
    yi = bn.forward(RunContext(False), types.SimpleNamespace(index=1, fused_act=node.fused_act, fused_drop=None), g(x))
    assert rel(yi, K.act_fwd(K.bn_infer_fwd(x64, gam, bet, mm, mv), act)) < 2e-5


@pytest.mark.parametrize('C', [3, 50])
def test_batchnorm_draws_its_own_dropout_mask_over_any_channel_count(C):
    """No injected mask, C % 4 != 0: the fused Dropout's keep-mask comes from Dropout.make_mask on the layer's stream position (what
    bn_apply_dropgen draws for C % 4 == 0), i.e. ops.dropout_mask at the same seed / offset."""
    from gennet_amd import ops, layers as L
    from gennet_amd.engine import RunContext, device_rng
    rng = np.random.RandomState(C)
    x = g(rng.randn(200, C) + 0.3)
    bn = L.BatchNormalization()
    bn.build((C,))
    drop = L.Dropout(0.4)
    seed, off = device_rng().take(0)
    y = bn.forward(RunContext(True, site='a'), types.SimpleNamespace(index=0, fused_act=None, fused_drop=(0.4, drop)), x)
    want = ops.dropout_mask((200, C), 0.4, seed, off, torch.device('cuda:0')).bool()
    plain = bn.forward(RunContext(True, site='b'), types.SimpleNamespace(index=0, fused_act=None, fused_drop=None), x)
    assert torch.equal(y == 0, ~want | (plain == 0))
    ref = torch.where(want, plain.double() / (1 - 0.4), torch.zeros_like(plain.double()))
    assert (y.double() - ref).abs().max().item() <= 1e-6 * ref.abs().max().item()
