"""GPU parity of BatchNormalization over an axis that is not the last one (csrc/bn_axis.hip through ops.bn_axis_*, layers.BatchNormalization(axis=...)),
and of a layer's own activation followed by an activation layer (Model._plan).

Kernel level.  The tensor is an (outer, P, inner) view, one parameter per p.  The oracle is oracle/keras_ref.py's last-axis BatchNormalization
on np.moveaxis(x, 1, -1).  Bounds are those tests/test_layer_passes_gpu.py::test_column_sums_and_batchnorm_at_uneven_channel_counts applies to
the same quantities of the last-axis kernels (`close` is a copy of its helper): sums 1e-6; saved mean and moving statistics 1e-5; y 2e-5;
dgamma, dbeta, dx 1e-4.  dsums is [dbeta | dgamma] before its cast to fp32 (sums of fp32 xhat terms, not of the inputs), so it carries their 1e-4.
Which shape crosses which seam (block = one p x one chunk of o, 256 lanes over the chunk's outer * inner / VEC units, 4 units per lane and trip):
    (2,3,2)      smallest of everything, scalar loads               (3,5,4)      smallest float4 path: 3 units per block
    (5,7,6)      inner even, no multiple of 4: runs 8-byte aligned  (2,1,8)      P = 1         (1,4,8)   outer = 1
    (4,33,260)   65 float4 per run: 260 units per block, one full 256-lane trip and 4 lanes of a second
    (3,2,1028)   771 float4 units per block: past 3 x 256           (3,2,1030)   3090 scalar units: past 3 x 1024, a lane's second 4-unit trip
    (7,12,1)     inner = 1: every run one float
    (600,3,12)   1800 float4 units per position: the chunk rule (chunks = min(2048 / P, ceil(units / 1024), outer)) gives 2 chunks of 300 rows,
                 so colred_finalize sums more than one partial per position; asserted below through the workspace size

Model level, against torch fp64 autograd on the CPU, in the pattern and with the bounds of
tests/test_conv_anyc_gpu.py::test_conv1d_layers_over_any_channel_pairs_train_and_predict: predict 1e-5, loss 1e-6 relative, gradients and
SGD-updated weights 1e-4 (gradients no finer than 1e-3 of the model's largest gradient entry)."""
import os
import pickle
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import keras_ref as K

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev():
    return torch.device('cuda:0')


def g(a, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=dev())


def f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def host(t):
    return t.detach().cpu().numpy().astype(np.float64) if isinstance(t, torch.Tensor) else np.asarray(t, np.float64)


def close(t, ref, rtol, atol=0.0, what=''):
    a, ref = host(t), np.asarray(ref, np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    scale = max(np.abs(ref).max(), 1e-30)
    err = np.abs(a - ref).max()
    print('%s max err %.3e vs scale %.3e (rel %.3e, bound %.1e)' % (what, err, scale, err / scale, rtol))
    assert err <= rtol * scale + atol, '%s max err %.3e vs scale %.3e (rel %.3e)' % (what, err, scale, err / scale)


def last(a):
    """(outer, P, inner) -> (outer, inner, P): the oracle's layout"""
    return np.moveaxis(host(a), 1, -1)


# (600,3,12): the one with more than one chunk per position (module docstring); were the kernel's chunk length raised, outer has to follow
SHAPES = [(2, 3, 2), (3, 5, 4), (5, 7, 6), (2, 1, 8), (1, 4, 8), (4, 33, 260), (3, 2, 1028), (3, 2, 1030), (7, 12, 1), (600, 3, 12)]


@pytest.mark.parametrize('outer,P,inner', SHAPES)
def test_four_passes_against_the_oracle_on_the_moved_axis(outer, P, inner):
    from gennet_amd import _lib, ops
    rng = np.random.RandomState(outer * 100000 + P * 1000 + inner)
    x = f32(rng.randn(outer, P, inner) * 1.5 + 0.7); dy = f32(rng.randn(outer, P, inner))
    gamma = f32(rng.rand(P) + 0.5); beta = f32(rng.randn(P) * 0.1)
    n = outer * inner
    xg, dyg, gd, bd = g(x), g(dy), g(gamma), g(beta)
    if (outer, P, inner) == (600, 3, 12):
        assert _lib.size('gn_bn_axis_stats_workspace', outer, P, inner) == 2 * (2 * P * 8)           # two chunks of partials
    # statistics: fp64 sums of the fp32 values, bit-identical on a second run
    sums = ops.bn_axis_stats(xg)
    close(sums[:P], x.sum((0, 2)), 1e-6, what='sum x'); close(sums[P:], (x * x).sum((0, 2)), 1e-6, what='sum x^2')
    assert torch.equal(ops.bn_axis_stats(xg), sums)
    y_ref, cache, mean, var = K.bn_train_fwd(last(x), gamma, beta)
    # finalize with P parameters and count = outer * inner: both moving-average forms, two updates each (local_step 1, 2)
    mm0, mv0 = f32(rng.randn(P) * 0.1), f32(rng.rand(P) + 0.5)
    for form in ('ema', 'tf_zero_debias'):
        mm, mv, bm, bv = g(mm0), g(mv0), g(np.zeros(P)), g(np.zeros(P))
        mm_ref, mv_ref, zd_ref = mm0, mv0, [np.zeros(P), np.zeros(P), 0]
        for step in (1, 2):
            if form == 'ema':
                scale, shift, smean, sinv = ops.bn_finalize(sums, n, gd, bd, K.BN_EPS, 0.99, mm, mv)
                mm_ref, mv_ref = K.bn_moving_update(mm_ref, mv_ref, mean, var, n, 0.99)
            else:
                scale, shift, smean, sinv = ops.bn_finalize(sums, n, gd, bd, K.BN_EPS, 0.99, mm, mv, (bm, bv, step))
                mm_ref, mv_ref, zd_ref = K.bn_moving_update_zero_debias(mm_ref, mv_ref, zd_ref, mean, var, n, 0.99)
            close(mm, mm_ref, 1e-5, what='%s moving mean %d' % (form, step)); close(mv, mv_ref, 1e-5, what='%s moving variance %d' % (form, step))
        close(smean, mean, 1e-5, 1e-6, what='saved mean'); close(sinv, cache[1], 1e-5, what='saved invstd')
    y = ops.bn_axis_apply(xg, scale, shift)
    close(last(y), y_ref, 2e-5, what='y')
    # backward
    dx_ref, dg_ref, db_ref = K.bn_train_bwd(last(dy), cache, gamma)
    dsums = ops.bn_axis_bwd_stats(dyg, xg, smean, sinv)
    close(dsums[:P], db_ref, 1e-4, what='dsums dbeta'); close(dsums[P:], dg_ref, 1e-4, what='dsums dgamma')
    assert torch.equal(ops.bn_axis_bwd_stats(dyg, xg, smean, sinv), dsums)
    dgamma = torch.full((P,), 7.0, device=dev()); dbeta = torch.full((P,), 7.0, device=dev())
    dx = ops.bn_axis_bwd_apply(dyg, xg, gd, smean, sinv, dsums, n, dsums, dgamma, dbeta)
    close(dgamma, dg_ref, 1e-4, what='dgamma'); close(dbeta, db_ref, 1e-4, what='dbeta')
    close(last(dx), dx_ref, 1e-4, what='dx')
    assert torch.equal(ops.bn_axis_bwd_apply(dyg, xg, gd, smean, sinv, dsums, n, dsums, dgamma, dbeta), dx)
    # inference phase: the same apply pass with the coefficients of the moving statistics
    sc_i, sh_i = ops.bn_infer_coeffs(gd, bd, mm, mv, K.BN_EPS)
    close(last(ops.bn_axis_apply(xg, sc_i, sh_i)), K.bn_infer_fwd(last(x), gamma, beta, host(mm), host(mv)), 2e-5, what='y inference')


@pytest.mark.parametrize('outer,P', [(7, 12), (257, 12), (3001, 5), (4096, 4)])
def test_inner_one_is_the_last_axis_case_of_the_column_kernels(outer, P):
    """(outer, P, 1) against ops.bn_stats / ops.bn_apply on the (outer, P) view.  Both sums are fp64 sums of the same fp32 terms in another order:
    each differs from the exact sum by at most outer * 2^-53 of the sum of magnitudes, 4.6e-13 at outer = 4096, so 1e-12 of it holds between them.
    The apply pass is the same fmaf per element: bit for bit."""
    from gennet_amd import ops
    rng = np.random.RandomState(outer + P)
    x = f32(rng.randn(outer, P) * 1.5 + 0.7)
    x2 = g(x); x3 = x2.reshape(outer, P, 1)
    a, b = host(ops.bn_axis_stats(x3)), host(ops.bn_stats(x2))
    bound = 1e-12 * np.concatenate([np.abs(x).sum(0), (x * x).sum(0)])
    print('inner = 1 sums: largest difference / bound %.3g' % (np.abs(a - b) / bound).max())
    assert (np.abs(a - b) <= bound).all(), (np.abs(a - b) / bound).max()
    scale, shift = g(rng.rand(P) + 0.5), g(rng.randn(P))
    assert torch.equal(ops.bn_axis_apply(x3, scale, shift).reshape(outer, P), ops.bn_apply(x2, scale, shift, None, 'linear', 0.0))


def test_bad_arguments_are_errors_and_launch_nothing():
    from gennet_amd import _lib, ops
    stream = torch.cuda.current_stream().cuda_stream
    for shape in ((2, 0, 3), (2, 3, 0)):                                   # P = 0, inner = 0
        z = torch.zeros(shape, device=dev()); v = torch.zeros(max(shape[1], 1), device=dev())
        for call in (lambda: ops.bn_axis_stats(z), lambda: ops.bn_axis_apply(z, v, v), lambda: ops.bn_axis_bwd_stats(z, z, v, v)):
            with pytest.raises(_lib.GennetHipError):
                call()
    outer, P, inner = 600, 3, 12
    x = g(np.ones((outer, P, inner)))
    nb = _lib.size('gn_bn_axis_stats_workspace', outer, P, inner)
    ws = torch.zeros(nb, dtype=torch.uint8, device=dev())
    sums = torch.full((2 * P,), -5.0, dtype=torch.float64, device=dev())
    with pytest.raises(_lib.GennetHipError) as e:
        _lib.call('gn_bn_axis_stats', x.data_ptr(), outer, P, inner, sums.data_ptr(), ws.data_ptr(), nb - 1, stream)
    assert 'workspace' in str(e.value)
    with pytest.raises(_lib.GennetHipError):
        _lib.call('gn_bn_axis_bwd_stats', x.data_ptr(), x.data_ptr(), sums.data_ptr(), sums.data_ptr(), sums.data_ptr(), ws.data_ptr(), nb - 1, outer, P, inner, stream)
    torch.cuda.synchronize()
    assert (sums == -5.0).all() and int(ws.sum()) == 0                     # nothing ran
    _lib.call('gn_bn_axis_stats', x.data_ptr(), outer, P, inner, sums.data_ptr(), ws.data_ptr(), nb, stream)
    assert torch.equal(sums, torch.full((2 * P,), float(outer * inner), dtype=torch.float64, device=dev()))


# ---- model level ----------------------------------------------------------------------------------------------------------------------
NETS = {
    # the sibling discriminator with its Flatten tail: BatchNormalization(axis=1) at inner = 6 and 12; the activation-pair rule in values
    'discriminator': ((64,), [('reshape', (-1, 1)), ('conv', 6, 8, 'tanh'), ('leaky', 0.2), ('bn', 1), ('conv', 12, 8, 'tanh'), ('leaky', 0.2), ('bn', 1),
                              ('flatten',), ('dense', 2, 'sigmoid')]),
    # the sibling generator without dilation: inner = 1 (the column kernels on the (outer, P) view), 32, 28
    'generator': ((10,), [('reshape', (-1, 1, 1)), ('bn', 1), ('convT', 8, 4, 'relu'), ('leaky', 0.2), ('bn', 1), ('convT', 4, 4, 'relu'), ('leaky', 0.2),
                          ('bn', 1), ('flatten',), ('dense', 5, None)]),
    # axis=2 of a 4-D tensor: outer spans the batch and H (18 rows), P = 7, inner = 8
    'axis2_4d': ((12,), [('reshape', (3, 4, 1)), ('convT', 8, 4, 'relu'), ('bn', 2), ('convT', 4, 4, None), ('flatten',), ('dense', 5, None)]),
}
BN_VIEWS = {'discriminator': [(1, 57, 6), (1, 50, 12)], 'generator': [(1, 10, 1), (1, 10, 32), (1, 10, 28)], 'axis2_4d': [(3, 7, 8)]}


def _build(spec, in_shape, form):
    from gennet_amd import layers as Ly
    from gennet_amd.engine import Sequential
    ls = []
    for i, s in enumerate(spec):
        kw = {'input_shape': in_shape} if i == 0 else {}
        if s[0] == 'reshape':
            ls.append(Ly.Reshape(s[1], **kw))
        elif s[0] == 'conv':
            ls.append(Ly.Conv1D(s[1], s[2], padding='valid', activation=s[3], **kw))
        elif s[0] == 'convT':
            ls.append(Ly.Conv2DTranspose(s[1], (1, s[2]), activation=s[3], **kw))
        elif s[0] == 'leaky':
            ls.append(Ly.LeakyReLU(s[1], **kw))
        elif s[0] == 'bn':
            ls.append(Ly.BatchNormalization(axis=s[1], moving_average=form, **kw))
        elif s[0] == 'flatten':
            ls.append(Ly.Flatten(**kw))
        elif s[0] == 'dense':
            ls.append(Ly.Dense(s[1], activation=s[2], **kw))
    return Sequential(ls), ls


def _act(h, kind):
    return {None: lambda v: v, 'tanh': torch.tanh, 'relu': torch.relu, 'sigmoid': torch.sigmoid}[kind](h)


def _ref_forward(spec, P, x, training, moving, stats=None):
    """torch fp64, channels last, the batch in front.  stats: receives {index: (batch mean, biased batch variance)} of the BatchNormalization layers."""
    h = x
    for i, s in enumerate(spec):
        if s[0] == 'reshape':
            h = h.reshape((h.shape[0],) + tuple(s[1]))
        elif s[0] == 'conv':
            h = _act(F.conv1d(h.permute(0, 2, 1), P[i][0].permute(2, 1, 0)).permute(0, 2, 1) + P[i][1], s[3])
        elif s[0] == 'convT':              # keras kernel (1, kw, filters, Cin), 'valid', stride 1: y[b, h, v, f] = sum_j sum_c x[b, h, v - j, c] k[0, j, f, c]
            kw, W = P[i][0].shape[1], h.shape[2]
            hp = F.pad(h, (0, 0, kw - 1, kw - 1))
            h = _act(sum(hp[:, :, kw - 1 - j:kw - 1 - j + W + kw - 1, :] @ P[i][0][0, j].T for j in range(kw)) + P[i][1], s[3])
        elif s[0] == 'leaky':
            h = torch.where(h > 0, h, float(np.float32(s[1])) * h)
        elif s[0] == 'bn':
            dims = tuple(d for d in range(h.dim()) if d != s[1])
            shape = [1] * h.dim(); shape[s[1]] = h.shape[s[1]]
            if training:
                mean = h.mean(dim=dims); var = ((h - mean.reshape(shape)) ** 2).mean(dim=dims)
                if stats is not None:
                    stats[i] = (mean.detach().numpy(), var.detach().numpy())
            else:
                mean, var = moving[i]
            h = (h - mean.reshape(shape)) / torch.sqrt(var.reshape(shape) + 1e-3) * P[i][0].reshape(shape) + P[i][1].reshape(shape)
        elif s[0] == 'flatten':
            h = h.reshape(h.shape[0], -1)
        elif s[0] == 'dense':
            h = _act(h @ P[i][0] + P[i][1], s[2])
    return h


def rel(a, ref):
    a = np.asarray(a, np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-30)


@pytest.mark.parametrize('form', ['tf_zero_debias', 'ema'])
@pytest.mark.parametrize('net', sorted(NETS))
def test_sibling_stacks_train_and_predict(net, form):
    from gennet_amd.engine import SGD
    in_shape, spec = NETS[net]
    B, lr = 6, 0.05
    rng = np.random.RandomState(len(net))
    model, ls = _build(spec, in_shape, form)
    weighted = ('conv', 'convT', 'dense', 'bn')
    # seeded biases, BatchNormalization parameters and moving statistics (the zero / one initial values would hide them)
    for l, s in zip(ls, spec):
        ws = l.get_weights()
        if s[0] in ('conv', 'convT', 'dense'):
            l.set_weights([ws[0], rng.randn(*ws[1].shape).astype(np.float32) * 0.1])
        elif s[0] == 'bn':
            C = ws[0].shape[0]
            l.set_weights([1 + 0.2 * rng.randn(C), 0.2 * rng.randn(C), 0.3 * rng.randn(C), 0.5 + rng.rand(C)])
    bns = [l for l, s in zip(ls, spec) if s[0] == 'bn']
    assert [l.view for l in bns] == BN_VIEWS[net] and not any(l.is_batchnorm for l in bns)
    model.compile(optimizer=SGD(lr=lr), loss='mean_squared_error')
    model._plan()
    assert not any(n.absorbed for n in model.nodes) and all(n.fused_act is None for n in model.nodes)      # a layer's own activation keeps the LeakyReLU a node
    x = rng.randn(B, *in_shape).astype(np.float32)
    t = rng.randn(B, *model.output_shape[1:]).astype(np.float32)

    def params():
        return ({i: [torch.tensor(w.astype(np.float64), requires_grad=True) for w in l.get_weights()[:2]] for i, (l, s) in enumerate(zip(ls, spec)) if s[0] in weighted},
                {i: [torch.tensor(w.astype(np.float64)) for w in l.get_weights()[2:]] for i, (l, s) in enumerate(zip(ls, spec)) if s[0] == 'bn'})
    P, moving = params()
    xt, tt = torch.tensor(x.astype(np.float64)), torch.tensor(t.astype(np.float64))
    y = model.predict(x, batch_size=B)
    with torch.no_grad():
        y_ref = _ref_forward(spec, P, xt, False, moving).numpy()
    print(net, form, 'predict err', rel(y, y_ref))
    assert rel(y, y_ref) < 1e-5
    stats = {}
    loss_ref = ((_ref_forward(spec, P, xt, True, moving, stats) - tt) ** 2).mean()
    loss_ref.backward()
    res = model.train_on_batch(x, t)
    print(net, form, 'loss', res[0], float(loss_ref.detach()))
    assert abs(res[0] - float(loss_ref.detach())) <= 1e-6 * abs(float(loss_ref.detach()))
    # a bias in front of a BatchNormalization has a zero gradient in exact arithmetic and holds rounding noise only: a gradient is measured against
    # its own largest entry, but no finer than 1e-3 of the model's largest gradient entry (test_conv_anyc_gpu's floor)
    g_floor = 1e-3 * max(float(v.grad.abs().max()) for ts in P.values() for v in ts)
    for i, (l, s) in enumerate(zip(ls, spec)):
        if i not in P:
            continue
        for p, ref in zip(l.params, P[i]):
            g_ref = ref.grad.numpy()
            gr = p.grad.detach().cpu().numpy().reshape(g_ref.shape)
            gerr = np.abs(gr - g_ref).max() / max(np.abs(g_ref).max(), g_floor)
            w_ref = (ref.detach() - lr * ref.grad).numpy()
            werr = np.abs(p.numpy().astype(np.float64) - w_ref).max() / max(np.abs(w_ref).max(), 1e-3)
            print(net, form, l.name, p.name, 'grad err %.3g weight err %.3g' % (gerr, werr))
            assert gerr < 1e-4 and werr < 1e-4, (l.name, p.name, gerr, werr)
    # moving statistics: the oracle's update with n = outer * inner elements per parameter
    for i, (l, s) in enumerate(zip(ls, spec)):
        if s[0] != 'bn':
            continue
        n = B * l.view[0] * l.view[2]
        mm0, mv0 = (m.numpy() for m in moving[i])
        mean, var = stats[i]
        if form == 'ema':
            mm_ref, mv_ref = K.bn_moving_update(mm0, mv0, mean, var, n, 0.99)
            assert l.zero_debias == {}
        else:
            mm_ref, mv_ref, _ = K.bn_moving_update_zero_debias(mm0, mv0, [np.zeros_like(mm0), np.zeros_like(mm0), 0], mean, var, n, 0.99)
            assert l.zero_debias[model.name][2] == 1 and l.zero_debias[model.name][0].shape == (l.view[1],)
        close(l.moving_mean.numpy(), mm_ref, 1e-5, what='%s moving mean' % l.name); close(l.moving_variance.numpy(), mv_ref, 1e-5, what='%s moving variance' % l.name)
    # predict again: the reference on the model's weights as they are now, its updated moving statistics included -- and not the old ones
    P2, moving2 = params()
    y2 = model.predict(x, batch_size=B)
    with torch.no_grad():
        y2_ref = _ref_forward(spec, P2, xt, False, moving2).numpy()
        y2_old = _ref_forward(spec, P2, xt, False, moving).numpy()
    print(net, form, 'predict after the step: err', rel(y2, y2_ref), 'against the old moving statistics', rel(y2, y2_old))
    assert rel(y2, y2_ref) < 1e-5 and rel(y2, y2_old) > 1e-4            # ten times the parity bound apart: told apart for certain


def test_zero_debias_state_of_a_position_batchnorm_survives_save_and_load(tmp_path):
    from gennet_amd.engine import SGD
    from gennet_amd.keras.models import load_model
    in_shape, spec = NETS['discriminator']
    model, ls = _build(spec, in_shape, None)
    model.compile(optimizer=SGD(lr=0.05), loss='mean_squared_error')
    rng = np.random.RandomState(2)
    for _ in range(2):
        model.train_on_batch(rng.randn(6, 64).astype(np.float32), rng.rand(6, 2).astype(np.float32))
    path = str(tmp_path / 'd.h5')
    model.save(path, True)
    m2 = load_model(path)
    for a, b in zip([l for l in model.layers if hasattr(l, 'zero_debias')], [l for l in m2.layers if hasattr(l, 'zero_debias')]):
        assert b.axis == 1 and b.view == a.view and list(b.zero_debias) == [model.name]
        sa, sb = a.zero_debias[model.name], b.zero_debias[model.name]
        assert sb[2] == 2 and torch.equal(sa[0], sb[0]) and torch.equal(sa[1], sb[1]) and sb[0].shape == (a.view[1],)
    assert all(np.array_equal(u, v) for u, v in zip(model.get_weights(), m2.get_weights()))
    x = rng.randn(6, 64).astype(np.float32)
    assert np.array_equal(model.predict(x, batch_size=6), m2.predict(x, batch_size=6))


# ---- data parallelism -------------------------------------------------------------------------------------------------------------------
WORKER = os.path.join(ROOT, 'tests', 'bn_axis_dp_worker.py')


def free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def launch(out, world):
    """As tests/test_dist.py starts its `gpu` mode: the worker directly for one rank, torch.distributed.run for more."""
    env = dict(os.environ)
    env.pop('RANK', None); env.pop('WORLD_SIZE', None); env.pop('LOCAL_RANK', None)
    if world == 1:
        cmd = [sys.executable, WORKER, out]
    else:
        cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(world), '--master-addr', '127.0.0.1',
               '--master-port', str(free_port()), WORKER, out]
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    return [pickle.load(open('%s.%d' % (out, k), 'rb')) for k in range(world)]


def test_two_ranks_equal_one_rank_with_position_batchnorm(tmp_path):
    """2 ranks x 4 rows against 1 rank x 8 rows: sums and backward sums all-reduced, count x 2.  Losses to test_dist's 1e-5 relative + 1e-7; weights to
    1e-4 of each tensor's largest magnitude; the replicas bit-identical to each other."""
    one = launch(str(tmp_path / 'one'), 1)[0]
    two = launch(str(tmp_path / 'two'), 2)
    for r in two:
        assert len(r['losses']) == 3
        for u, v in zip(r['losses'], one['losses']):
            print('loss', u, v)
            assert abs(u - v) <= 1e-5 * abs(v) + 1e-7, (r['losses'], one['losses'])
        for w, wr in zip(r['weights'], one['weights']):
            err = np.abs(w - wr).max() / np.abs(wr).max()
            print('weight', w.shape, 'err %.3g' % err)
            assert err <= 1e-4, (w.shape, err)
    for w0, w1 in zip(two[0]['weights'], two[1]['weights']):
        assert np.array_equal(w0, w1)
