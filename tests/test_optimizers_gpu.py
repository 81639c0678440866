"""Keras optimizers beyond the default Adam pass on the MI355X (gennet_amd/csrc/optim.hip through engine.Optimizer):
  * the fused update of every rule against the fp64 restatement tests/optim_ref.py: plain and with decay, clipnorm above and below the limit,
    clipvalue, nesterov, amsgrad; lengths 1, 3, 4099, 2^20 + 7; three segments at misaligned starts (the clip norm spans all three); 5 steps;
    two runs bit-identical;
  * the CNN point estimator for 20 steps per optimizer and a GAN iteration series with RMSprop + clipnorm against the network oracles with their
    optimizer replaced by the restatement;
  * captured step graphs bit-identical to the eager loop; save -> load_model -> resume bit-identical to an uninterrupted run; 2 ranks == 1 rank.

Tolerance of the kernel tests: the kernel rounds every operation to fp32 (2^-24 relative, -ffp-contract=off), the restatement is fp64 on the
same fp32 inputs.  A rule has at most ~10 operations per step, each state recursion carries its error forward, so after 5 steps the
difference is below 5 x 10 x 6e-8 = 3e-6 of the operands' magnitude: rtol 1e-5, plus atol 1e-6 of the array's largest magnitude for
elements where p + update cancels (the error is relative to the operands, not to the small result)."""
import os
import pickle
import random
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import optim_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = [1, 3, 4099, 2 ** 20 + 7]
OFFSETS = (0, 1, 3)                        # element offset of each of the three segments' p and g: aligned, then two misaligned starts


def _cases():
    base = {'SGD': dict(lr=0.01, momentum=0.9), 'RMSprop': dict(lr=1e-3), 'Adagrad': dict(lr=0.01), 'Adadelta': dict(), 'Adamax': dict(),
            'Adam': dict(lr=1e-3, beta_1=0.5)}
    out = []
    for cls, kw in base.items():
        out += [(cls, kw, 'plain'), (cls, dict(kw, decay=0.05), 'decay'), (cls, kw, 'clip_above'), (cls, kw, 'clip_below'),
                (cls, dict(kw, clipvalue=0.5), 'clipvalue')]
    out += [('SGD', dict(lr=0.01, momentum=0.9, nesterov=True), 'nesterov'), ('Adam', dict(lr=1e-3, amsgrad=True), 'amsgrad'),
            ('Adamax', dict(lr=2e-3, clipvalue=0.7, decay=0.01), 'clipnorm+clipvalue')]
    return out


class _Group(object):
    """A flat group as engine.ParamGroup lays it out (segment padded to 64 floats, padding zero), placed at an element offset of a larger buffer."""

    def __init__(self, p0, off):
        n = p0.size
        pad = -(-n // 64) * 64
        self.pbuf = torch.zeros(off + pad + 8, dtype=torch.float32, device='cuda')
        self.gbuf = torch.zeros_like(self.pbuf)
        self.data, self.grad = self.pbuf[off:off + pad], self.gbuf[off:off + pad]
        self.data[:n].copy_(torch.from_numpy(p0))


class _P(object):
    def __init__(self, grp, n, k):
        self.group, self.offset, self.size, self.shape, self.name = grp, 0, n, (n,), 'w%d' % k


def _run_device(cls, kw, p0s, grads):
    from gennet_amd import engine
    engine.device()
    opt = engine.OPTIMIZERS[cls](**kw)
    groups = [_Group(p, off) for p, off in zip(p0s, OFFSETS)]
    params = [_P(g, p.size, k) for k, (g, p) in enumerate(zip(groups, p0s))]
    opt.bind(params)
    factors = []
    for gs in grads:
        for grp, g in zip(groups, gs):
            grp.grad[:g.size].copy_(torch.from_numpy(g))
        opt.step()
        if opt._factor is not None:
            factors.append(opt._factor.cpu().numpy()[0])
    torch.cuda.synchronize()
    seg = {id(grp): st for grp, _, _, st in opt.state}                    # engine.segments orders segments by group identity
    states = [seg[id(grp)] for grp in groups]
    n = [p.size for p in p0s]
    return (opt, groups, states, [grp.data[:k].cpu().numpy() for grp, k in zip(groups, n)],
            [[states[k][j][:n[k]].cpu().numpy() for k in range(len(groups))] for j in range(opt._n_slots())], factors)


def _inputs(n, steps, seed):
    rng = np.random.RandomState(seed)
    p0s = [rng.randn(n).astype(np.float32) for _ in OFFSETS]
    grads = [[rng.randn(n).astype(np.float32) for _ in OFFSETS] for _ in range(steps)]
    return p0s, grads


def _close(dev, ref, what):
    ref = np.asarray(ref, np.float64)
    err = np.abs(dev.astype(np.float64) - ref)
    tol = 1e-5 * np.abs(ref) + 1e-6 * max(np.abs(ref).max(), 1e-30)
    assert np.all(err <= tol), (what, float(err.max()), int((err > tol).sum()))


@pytest.mark.parametrize('n', LENGTHS)
@pytest.mark.parametrize('cls,kw,case', _cases(), ids=['%s-%s' % (c[0], c[2]) for c in _cases()])
def test_update_kernel_matches_restatement(cls, kw, case, n):
    steps = 5
    p0s, grads = _inputs(n, steps, 1000 + n)
    kw = dict(kw)
    norm = np.sqrt(3.0 * n)                                                # E|g| over the three segments
    if case == 'clip_above':
        kw['clipnorm'] = 0.5 * norm
    elif case == 'clip_below':
        kw['clipnorm'] = 2.0 * norm + 10.0
    elif case == 'clipnorm+clipvalue':
        kw['clipnorm'] = 0.5 * norm
    opt, groups, states, p_dev, st_dev, factors = _run_device(cls, kw, p0s, grads)
    ref_p = [p.astype(np.float64) for p in p0s]
    ref = R.KerasOpt(cls.lower(), ref_p, **kw)
    for gs in grads:
        ref.step(ref_p, [g.astype(np.float64) for g in gs])
    assert opt.iterations == steps
    for k in range(3):
        _close(p_dev[k], ref_p[k], (cls, case, n, 'p', k))
        for j, st in enumerate(st_dev):
            _close(st[k], ref.state[j][k], (cls, case, n, 'state', j, k))
        # the padding of every segment stays zero under every rule
        assert not groups[k].data[n:].any() and all(not t[n:].any() for t in states[k])
    if 'clipnorm' in kw and n > 3:
        assert all(f < 1 for f in factors) if case != 'clip_below' else all(f == 1 for f in factors), factors


@pytest.mark.parametrize('cls,kw', [('RMSprop', dict(lr=1e-3, clipnorm=100.0)), ('Adam', dict(lr=1e-3, amsgrad=True, clipnorm=100.0, clipvalue=0.5)),
                                    ('SGD', dict(momentum=0.9, nesterov=True, clipnorm=100.0)), ('Adadelta', dict(clipnorm=100.0))])
def test_two_runs_are_bit_identical(cls, kw):
    p0s, grads = _inputs(2 ** 20 + 7, 3, 7)
    a = _run_device(cls, kw, p0s, grads)
    b = _run_device(cls, kw, p0s, grads)
    assert all(f < 1 for f in a[5]) and [f.tobytes() for f in a[5]] == [f.tobytes() for f in b[5]]
    for x, y in zip(a[3], b[3]):
        assert x.tobytes() == y.tobytes()
    for sa, sb in zip(a[4], b[4]):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(sa, sb))


@pytest.mark.parametrize('off', [1, 2])
@pytest.mark.parametrize('cls,kw', [('SGD', dict(momentum=0.9, nesterov=True)), ('RMSprop', {}), ('Adagrad', {}), ('Adadelta', {}), ('Adamax', {}),
                                    ('Adam', dict(amsgrad=True))])
def test_mutually_aligned_misaligned_arrays(cls, kw, off):
    """Every array starting at the same offset off 16 bytes: the float4 body behind a scalar head, and a scalar tail."""
    from gennet_amd import engine, ops
    engine.device()
    opt = engine.OPTIMIZERS[cls](**kw)
    n = 4099
    rng = np.random.RandomState(off)
    p0, g = rng.randn(n).astype(np.float32), rng.randn(n).astype(np.float32)

    def at(a):
        buf = torch.zeros(n + 8, dtype=torch.float32, device='cuda')
        buf[off:off + n].copy_(torch.from_numpy(a))
        return buf[off:off + n]
    p, gd = at(p0), at(g)
    st = [at(np.zeros(n, np.float32)) for _ in range(opt._n_slots())]
    rule = 'amsgrad' if kw.get('amsgrad') else opt.RULE
    h0, h1, eps, nest = opt._hyper()
    lr = opt._next_scalar()
    ops.optim_step(rule, p, gd, st, lr, h0, h1, eps, nest)
    ref_p = [p0.astype(np.float64)]
    ref = R.KerasOpt(cls.lower(), ref_p, **kw)
    ref.step(ref_p, [g.astype(np.float64)])
    _close(p.cpu().numpy(), ref_p[0], (cls, off))
    for j, t in enumerate(st):
        _close(t.cpu().numpy(), ref.state[j][0], (cls, off, j))


def test_default_adam_still_takes_the_original_pass(monkeypatch):
    """Adam without decay / amsgrad / clipping runs gn_adam_step (its numbers are unchanged); any of the three moves it to the fused rule pass."""
    from gennet_amd import engine, ops
    calls = []
    monkeypatch.setattr(ops, 'adam_step', lambda *a: calls.append('adam'))
    monkeypatch.setattr(ops, 'optim_step', lambda *a: calls.append(a[0]))
    for kw, want in ((dict(lr=9e-5, beta_1=0.5), 'adam'), (dict(decay=1e-3), 'adam'), (dict(amsgrad=True), 'amsgrad'), (dict(clipvalue=1.0), 'adam')):
        calls.clear()
        opt = engine.Adam(**kw)
        p0s, grads = _inputs(100, 1, 0)
        groups = [_Group(p, 0) for p in p0s]
        opt.bind([_P(g, 100, k) for k, g in enumerate(groups)])
        opt.step()
        assert calls == [want] * 3
        assert opt._default_pass() == (kw == dict(lr=9e-5, beta_1=0.5))


# --------------------------------------------------------------------------------------------------------------------------------------------
# model level: the network oracles with the restatement as their optimizer
# --------------------------------------------------------------------------------------------------------------------------------------------
PE_CASES = [('SGD', dict(lr=1e-4, momentum=0.9, nesterov=True)), ('RMSprop', dict(lr=1e-4, clipnorm=10.0)), ('Adagrad', dict(lr=1e-3, decay=0.01)),
            ('Adadelta', dict(clipvalue=1.0)), ('Adamax', dict(lr=2e-4)), ('Adam', dict(lr=9e-5, beta_1=0.5, amsgrad=True, decay=0.01))]


@pytest.mark.parametrize('cls,kw', PE_CASES, ids=[c[0] for c in PE_CASES])
def test_pe_20_steps_follow_the_oracle(cls, kw):
    """Tolerances of the existing CNN checks (tests/test_trajectory_gpu.py's many-step form of the PE test): losses 1e-4, weights 1e-3 of the
    tensor's largest element, predictions 1e-4."""
    from gennet_amd import bbh, engine
    from oracle import nets_ref as N
    from test_nets_gpu import assert_decisions_consistent, decisions_for, f32, load_stack_into_layers, rel, round_stack
    n_pix, B, steps = 256, 5, 20
    rng = np.random.RandomState(77)
    ref = N.PENet(n_pix, rng)
    round_stack(ref.mc); round_stack(ref.q)
    ref.mc.params[-1][...] = 25.0; ref.q.params[-1][...] = 0.6
    ref.opt = R.KerasOpt(cls.lower(), ref.mc.params + ref.q.params, **kw)
    model = bbh.signal_pe_model(n_pix)
    n_mc = len([s for s in ref.mc.spec if s[0] in ('dense', 'conv1d')])
    with_params = [l for l in model.layers if l.weights]
    load_stack_into_layers(ref.mc, with_params[:n_mc])
    load_stack_into_layers(ref.q, with_params[n_mc:])
    model.compile(loss='mean_squared_error', optimizer=engine.OPTIMIZERS[cls](**kw), metrics=['accuracy'])
    bank = f32(rng.randn(32, n_pix, 1)); lab_mc = f32(rng.uniform(20, 35, 32)); lab_q = f32(rng.uniform(0.5, 1, 32))
    for step in range(steps):
        rows = rng.choice(32, B, replace=False)
        x = bank[rows]
        cap = {}
        out = model.train_on_batch(x, [lab_mc[rows], lab_q[rows]], capture=cap)
        out_ref = ref.train_on_batch(x, lab_mc[rows], lab_q[rows],
                                     decisions=(decisions_for(ref.mc, with_params[:n_mc], cap), decisions_for(ref.q, with_params[n_mc:], cap)))
        del cap
        assert_decisions_consistent(ref.mc, ref.q)
        for a, b in zip(out[:3], out_ref[:3]):
            assert abs(a - b) <= 1e-4 * abs(b) + 1e-7, (step, out, out_ref)
    assert model.optimizer.iterations == steps and ref.opt.iterations == steps
    ws = [p_.data.cpu().numpy() for l in with_params for p_ in l.params]
    for k, (w, wr) in enumerate(zip(ws, ref.mc.params + ref.q.params)):
        assert np.abs(w - wr).max() <= 1e-3 * np.abs(wr).max(), (k, w.shape, rel(w, wr))
    xs = bank[:8]
    p_ref = ref.predict(xs); p = model.predict(xs)
    assert rel(p[0], p_ref[0]) < 1e-4 and rel(p[1], p_ref[1]) < 1e-4


def test_gan_iterations_with_rmsprop_clipnorm_follow_the_oracle():
    """Two GAN iterations (D step, then G step through the frozen D) with RMSprop + clipnorm on both optimizers; the limit sits below the
    gradient norm, so the clip-norm branch is taken.  Tolerances of test_nets_gpu.py's GAN test with RMSprop's first-step size sqrt(1/(1-rho)) lr."""
    from gennet_amd import bbh, engine
    from test_nets_gpu import _build_gan, assert_decisions_consistent, decisions_for, f32, masks_by_name, rel, stack_masks
    n_pix, B, iters, lr = 64, 4, 2, 1e-4
    rng = np.random.RandomState(3)
    ref, nets, event = _build_gan(n_pix, rng)
    G, D, DG = nets.generator, nets.signal_discriminator, nets.signal_discriminator_on_generator
    kw = dict(lr=lr, clipnorm=0.05)
    DG.optimizer = engine.RMSprop(**kw)                 # replaced before the first step binds any state
    D.optimizer = engine.RMSprop(**kw)
    ref.opt_g = R.KerasOpt('rmsprop', ref.G.params, **kw)
    ref.opt_d = R.KerasOpt('rmsprop', ref.D.params, **kw)
    factors = []
    for it in range(iters):
        z = f32(rng.uniform(-1, 1, (B, 100)))
        fake_ref = ref.generate(z)
        real = f32(rng.randn(B, n_pix)); noise = f32(rng.randn(B, n_pix, 1))
        sX_ref, sy = ref.assemble_d_batch(real, noise, fake_ref)
        d_masks = stack_masks(ref.D, sX_ref, rng)
        cap = {}
        out = D.train_on_batch(sX_ref, sy, dropout_masks=masks_by_name(ref.D, d_masks, D.layers), capture=cap)
        out_ref = ref.d_train_on_batch(sX_ref, sy, d_masks, decisions_for(ref.D, D.layers, cap))
        del cap
        assert_decisions_consistent(ref.D)
        assert abs(out[0] - out_ref[0]) <= 2e-5 * abs(out_ref[0]) and out[1] == pytest.approx(out_ref[1])
        factors.append(D.optimizer._factor.item())
        z2 = f32(rng.uniform(-1, 1, (B, 100)))
        g_masks = stack_masks(ref.G, z2, rng)
        d_masks2 = stack_masks(ref.D, (B, n_pix, 2, 1), rng)
        names = dict(masks_by_name(ref.G, g_masks, G.layers)); names.update(masks_by_name(ref.D, d_masks2, D.layers))
        cap = {}
        out = DG.train_on_batch(z2, [1] * B, dropout_masks=names, capture=cap)
        out_ref = ref.g_train_on_batch(z2, [1] * B, g_masks, d_masks2, decisions_for(ref.D, D.layers, cap))
        del cap
        assert_decisions_consistent(ref.D)
        assert abs(out[0] - out_ref[0]) <= 2e-5 * abs(out_ref[0]) and out[1] == pytest.approx(out_ref[1])
        factors.append(DG.optimizer._factor.item())
    assert min(factors) < 1, factors                                             # the clip-norm branch was taken
    step_budget = iters * lr * np.sqrt(1.0 / (1.0 - 0.9))
    for st, model in ((ref.G, G), (ref.D, D)):
        ws = [p.data.cpu().numpy() for l in model.layers for p in l.params]
        for w, wr in zip(ws, st.params):
            assert np.abs(w - wr).max() <= 2e-4 * np.abs(wr).max() + 0.02 * step_budget
    z3 = f32(rng.uniform(-1, 1, (B, 100)))
    assert rel(G.predict(z3), ref.generate(z3)) < 1e-4


# --------------------------------------------------------------------------------------------------------------------------------------------
# graph capture, resume, data parallelism
# --------------------------------------------------------------------------------------------------------------------------------------------
def _rmsprop_decay_clipnorm():
    from gennet_amd import engine
    return engine.RMSprop(9e-5, decay=1e-3, clipnorm=1.0)


def _sgd_nesterov():
    from gennet_amd import engine
    return engine.SGD(9e-5, momentum=0.9, nesterov=True, clipvalue=0.5)


GRAPH_OPTS = {'rmsprop_decay_clipnorm': _rmsprop_decay_clipnorm, 'sgd_nesterov': _sgd_nesterov}


def _setup(n_pix, seed, factory):
    from gennet_amd import bbh, engine
    engine.set_init_seed(seed); engine.set_device_seed(100 + seed)
    random.seed(seed); np.random.seed(seed)
    rng = np.random.RandomState(seed)
    event = rng.randn(n_pix, 1).astype(np.float32)
    nets = bbh.build_and_compile(event, n_pix, optimizer=factory)
    bank = bbh.DeviceBank(rng.randn(64, n_pix).astype(np.float32), np.stack([rng.uniform(20, 35, 64), rng.uniform(0.5, 1, 64)], 1))
    return nets, bank, engine.to_device(event.reshape(-1))


def _weights(model):
    return [w.copy() for w in model.get_weights()]


@pytest.mark.parametrize('which', sorted(GRAPH_OPTS))
def test_graphed_steps_are_bit_identical_to_the_eager_loop(which):
    from gennet_amd import bbh
    n_pix, B, steps = 256, 8, 6
    fac = GRAPH_OPTS[which]
    nets, bank, ev = _setup(n_pix, 3, fac)
    eager = [bbh.gan_train_step(nets, bank, ev, B) for _ in range(steps)]
    eager_pe = [bbh.pe_train_step(nets.signal_pe, bank, B) for _ in range(steps)]
    w_eager = _weights(nets.generator) + _weights(nets.signal_discriminator) + _weights(nets.signal_pe)
    nets, bank, ev = _setup(n_pix, 3, fac)
    gan, pe = bbh.GraphedGANStep(nets, bank, ev, B), bbh.GraphedPEStep(nets.signal_pe, bank, B)
    graphed = [gan() for _ in range(steps)]
    graphed_pe = [pe() for _ in range(steps)]
    assert gan.sg is not None and pe.sg is not None
    assert graphed == eager and graphed_pe == eager_pe, (graphed, eager)
    w_graph = _weights(nets.generator) + _weights(nets.signal_discriminator) + _weights(nets.signal_pe)
    assert all(np.array_equal(a, b) for a, b in zip(w_eager, w_graph))
    assert nets.signal_discriminator.optimizer.iterations == steps and nets.signal_pe.optimizer.iterations == steps


RESUME = [('SGD', dict(lr=1e-4, momentum=0.9)), ('RMSprop', dict(lr=1e-4)), ('Adagrad', dict(lr=1e-3)), ('Adadelta', {}), ('Adamax', dict(lr=2e-4)),
          ('Adam', dict(lr=1e-4, amsgrad=True, clipnorm=5.0))]


@pytest.mark.parametrize('cls,kw', RESUME, ids=[c[0] for c in RESUME])
def test_save_load_resume_is_bit_identical(tmp_path, cls, kw):
    from gennet_amd import bbh, engine, h5lite
    from gennet_amd.keras.models import load_model
    n_pix, B = 128, 4
    rng = np.random.RandomState(5)
    batches = [(rng.randn(B, n_pix, 1).astype(np.float32), rng.uniform(20, 35, B).astype(np.float32), rng.uniform(0.5, 1, B).astype(np.float32))
               for _ in range(6)]

    def fresh():
        engine.set_init_seed(11); engine.set_device_seed(21)       # same weights, same Philox (dropout) positions
        m = bbh.signal_pe_model(n_pix)
        m.compile(loss='mean_squared_error', optimizer=engine.OPTIMIZERS[cls](**kw), metrics=['accuracy'])
        return m
    a = fresh()
    la = [a.train_on_batch(x, [ym, yq]) for x, ym, yq in batches]
    b = fresh()
    lb = [b.train_on_batch(x, [ym, yq]) for x, ym, yq in batches[:3]]
    path = str(tmp_path / 'pe.h5')
    b.save(path, True)
    og = h5lite.File(path)['optimizer_weights']
    if cls == 'Adam':                                                      # amsgrad: full-shape vhat in the file
        names = [n.decode() for n in og.attrs['weight_names']]
        n = len(b._train_params)
        assert len(names) == 1 + 3 * n and all(og[nm].value.shape == p.shape for nm, p in zip(names[1 + 2 * n:], b._keras_train_order()))
    c = load_model(path)
    assert type(c.optimizer) is type(b.optimizer) and c.optimizer.get_config() == b.optimizer.get_config()
    lc = [c.train_on_batch(x, [ym, yq]) for x, ym, yq in batches[3:]]
    assert lb + lc == la
    assert all(np.array_equal(u, v) for u, v in zip(a.get_weights(), c.get_weights()))
    assert c.optimizer.iterations == (6 if c.optimizer.SAVES_ITERATIONS else 3)    # RMSprop / Adagrad / Adadelta files carry no count (Keras 2.2.4)


def test_rmsprop_clipnorm_two_ranks_equal_one_rank(tmp_path):
    """tests/test_dist.py's pattern with RMSprop + clipnorm: the clip factor, formed from all-reduced gradients, is bitwise equal on both ranks."""
    worker = os.path.join(ROOT, 'tests', 'optim_dp_worker.py')

    def launch(out, world):
        env = dict(os.environ)
        for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK'):
            env.pop(k, None)
        if world == 1:
            cmd = [sys.executable, worker, out]
        else:
            s = socket.socket(); s.bind(('127.0.0.1', 0)); port = s.getsockname()[1]; s.close()
            cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(world), '--master-addr', '127.0.0.1',
                   '--master-port', str(port), worker, out]
        r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-3000:]
        return [pickle.load(open('%s.%d' % (out, k), 'rb')) for k in range(world)]
    one = launch(str(tmp_path / 'one'), 1)[0]
    two = launch(str(tmp_path / 'two'), 2)
    assert all(f < 1 for f in one['factor'])                               # the clip-norm branch is taken
    assert [f.tobytes() for f in two[0]['factor']] == [f.tobytes() for f in two[1]['factor']]
    for r in two:
        for a, b in zip(r['losses'], one['losses']):
            for u, v in zip(a, b):
                assert abs(u - v) <= 1e-5 * abs(v) + 1e-7, (r['losses'], one['losses'])
        assert np.allclose(np.concatenate(r['factor']), np.concatenate(one['factor']), rtol=1e-5)
        for w, wr in zip(r['weights'], one['weights']):
            assert np.abs(w - wr).max() <= 1e-4 * np.abs(wr).max() + 0.02 * 4 * 1e-4 * np.sqrt(10.0)
    for w0, w1 in zip(two[0]['weights'], two[1]['weights']):
        assert np.array_equal(w0, w1)
