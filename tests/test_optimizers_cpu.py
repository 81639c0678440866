"""Keras 2.2.4 optimizers beyond the default Adam (SGD, RMSprop, Adagrad, Adadelta, Adamax; Adam with decay / amsgrad / clipping), CPU only:
the facade classes and their get_config, compile('<name>'), the fp64 restatement tests/optim_ref.py against torch.optim where the update has
the same form (and hand-unrolled sequences where it does not), Keras' clipping order, the training_config round trip of all six classes, and
the optimizer_weights layout pinned on the reference's SGD-compiled g_model.hdf5."""
import gzip
import json
import os

import numpy as np
import pytest
import torch

from gennet_amd import h5lite

import optim_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'keras_h5_golden.json')))
f32 = R.f32

KERAS_KEYS = {'SGD': {'lr', 'momentum', 'decay', 'nesterov'}, 'RMSprop': {'lr', 'rho', 'decay', 'epsilon'}, 'Adagrad': {'lr', 'decay', 'epsilon'},
              'Adadelta': {'lr', 'rho', 'decay', 'epsilon'}, 'Adamax': {'lr', 'beta_1', 'beta_2', 'decay', 'epsilon'},
              'Adam': {'lr', 'beta_1', 'beta_2', 'decay', 'epsilon', 'amsgrad'}}


def test_facade_classes_and_keras_config():
    from gennet_amd.keras.optimizers import SGD, RMSprop, Adagrad, Adadelta, Adamax, Adam, Nadam
    for cls in (SGD, RMSprop, Adagrad, Adadelta, Adamax, Adam):
        o = cls()
        assert set(o.get_config()) == KERAS_KEYS[cls.__name__], cls
        assert o.get_config()['lr'] == f32(R.DEFAULTS[cls.__name__.lower()]['lr'])
    assert SGD(lr=0.004).get_config() == {'lr': 0.004000000189989805, 'momentum': 0.0, 'decay': 0.0, 'nesterov': False}   # g_model.hdf5's record
    c = RMSprop(lr=1e-3, rho=0.9, decay=1e-4, clipnorm=1.0, clipvalue=0.5).get_config()
    assert c == {'lr': f32(1e-3), 'rho': f32(0.9), 'decay': f32(1e-4), 'epsilon': 1e-7, 'clipnorm': 1.0, 'clipvalue': 0.5}
    assert c['rho'] != 0.9 and c['decay'] != 1e-4                         # K.variable: float32-rounded
    assert Adadelta(rho=0.95).get_config()['rho'] == 0.95                 # a python float in Keras 2.2.4's Adadelta
    assert SGD(momentum=0.9, nesterov=True).get_config()['momentum'] == f32(0.9)
    assert Adamax(beta_1=0.8).get_config()['beta_1'] == f32(0.8) and Adamax().get_config()['beta_2'] == f32(0.999)
    assert Adam(amsgrad=True, decay=1e-3).get_config()['amsgrad'] is True
    assert 'clipnorm' not in Adam().get_config() and 'clipvalue' not in Adam().get_config()
    with pytest.raises(TypeError):
        Adam(clip_norm=1.0)                                                  # misspelt: Keras raises, nothing is ignored silently
    with pytest.raises(NotImplementedError):
        Nadam()


@pytest.mark.parametrize('name,cls', [('sgd', 'SGD'), ('rmsprop', 'RMSprop'), ('adagrad', 'Adagrad'), ('adadelta', 'Adadelta'), ('adamax', 'Adamax'),
                                      ('adam', 'Adam'), ('RMSprop', 'RMSprop')])
def test_compile_by_name_gives_keras_defaults(name, cls):
    from gennet_amd import bbh
    m = bbh.signal_pe_model(64)
    m.compile(loss='mean_squared_error', optimizer=name)
    assert type(m.optimizer).__name__ == cls
    want = {k: v for k, v in R.config(cls.lower()).items()}
    got = m.optimizer.get_config()
    assert got == {k: want[k] for k in got}


def _torch_run(opt_cls, kw, p0, grads):
    p = torch.tensor(p0, dtype=torch.float64, requires_grad=True)
    opt = opt_cls([p], **kw)
    for g in grads:
        p.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
    return p.detach().numpy(), opt.state[p]


def _ref_run(kind, p0, grads, **kw):
    p = [np.array(p0, np.float64)]
    o = R.KerasOpt(kind, p, **kw)
    for g in grads:
        o.step(p, [g])
    return p[0], o


def _data(seed=0, n=257, steps=6):
    rng = np.random.RandomState(seed)
    return rng.randn(n), [rng.randn(n) for _ in range(steps)]


@pytest.mark.parametrize('nesterov', [False, True])
def test_sgd_matches_torch(nesterov):
    p0, gs = _data(1)
    lr, mom = f32(0.01), f32(0.9)
    pt, st = _torch_run(torch.optim.SGD, dict(lr=lr, momentum=mom, nesterov=nesterov), p0, gs)
    pr, o = _ref_run('sgd', p0, gs, lr=0.01, momentum=0.9, nesterov=nesterov)
    assert np.allclose(pr, pt, rtol=1e-12, atol=1e-12)
    assert np.allclose(o.state[0][0], -lr * st['momentum_buffer'].numpy(), rtol=1e-12, atol=1e-14)   # Keras' velocity = -lr * torch's buffer
    pr0, _ = _ref_run('sgd', p0, gs, lr=0.01)                                                       # momentum 0: plain p - lr g
    assert np.allclose(pr0, p0 - lr * np.sum(gs, 0), rtol=1e-12, atol=1e-12)


def test_rmsprop_adagrad_adadelta_match_torch():
    p0, gs = _data(2)
    pt, st = _torch_run(torch.optim.RMSprop, dict(lr=f32(1e-3), alpha=f32(0.9), eps=1e-7), p0, gs)
    pr, o = _ref_run('rmsprop', p0, gs, lr=1e-3, rho=0.9)
    assert np.allclose(pr, pt, rtol=1e-12, atol=1e-14) and np.allclose(o.state[0][0], st['square_avg'].numpy(), rtol=1e-12)
    pt, st = _torch_run(torch.optim.Adagrad, dict(lr=f32(0.01), eps=1e-7, initial_accumulator_value=0), p0, gs)
    pr, o = _ref_run('adagrad', p0, gs, lr=0.01)
    assert np.allclose(pr, pt, rtol=1e-12, atol=1e-14) and np.allclose(o.state[0][0], st['sum'].numpy(), rtol=1e-12)
    pt, st = _torch_run(torch.optim.Adadelta, dict(lr=1.0, rho=0.95, eps=1e-7), p0, gs)
    pr, o = _ref_run('adadelta', p0, gs, lr=1.0, rho=0.95)
    assert np.allclose(pr, pt, rtol=1e-12, atol=1e-14)
    assert np.allclose(o.state[0][0], st['square_avg'].numpy(), rtol=1e-12) and np.allclose(o.state[1][0], st['acc_delta'].numpy(), rtol=1e-12)


def test_adamax_and_amsgrad_hand_unrolled():
    """torch places eps differently for these two: three steps unrolled by hand on scalars instead."""
    g = [0.5, -2.0, 0.25]
    b1, b2, lr, eps = f32(0.9), f32(0.999), f32(0.002), 1e-7
    p, m, u = 1.0, 0.0, 0.0
    for t, gt in enumerate(g, 1):
        m = b1 * m + (1 - b1) * gt
        u = max(b2 * u, abs(gt))
        p = p - lr / (1 - b1 ** t) * m / (u + eps)
    pr, o = _ref_run('adamax', np.array([1.0]), [np.array([x]) for x in g])
    assert pr[0] == pytest.approx(p, rel=1e-14) and o.state[1][0][0] == pytest.approx(2.0 * b2, rel=1e-14)   # u after step 3 = max(b2 * 2, 0.25)
    # amsgrad: vhat keeps the largest v; a large gradient first, then small ones, so v falls below vhat
    g = [3.0, 0.01, 0.01]
    b1, b2, lr = f32(0.9), f32(0.999), f32(0.001)
    p, m, v, vh = 1.0, 0.0, 0.0, 0.0
    for t, gt in enumerate(g, 1):
        m = b1 * m + (1 - b1) * gt
        v = b2 * v + (1 - b2) * gt * gt
        vh = max(vh, v)
        p = p - lr * np.sqrt(1 - b2 ** t) / (1 - b1 ** t) * m / (np.sqrt(vh) + eps)
    pr, o = _ref_run('adam', np.array([1.0]), [np.array([x]) for x in g], amsgrad=True)
    assert pr[0] == pytest.approx(p, rel=1e-14) and o.state[2][0][0] == pytest.approx(vh, rel=1e-14) and o.state[2][0][0] > o.state[1][0][0]


def test_decay_uses_the_count_before_the_increment():
    p0, gs = _data(3, 5, 3)
    pr, _ = _ref_run('sgd', p0, gs, lr=0.1, decay=0.5)
    lr, d = f32(0.1), f32(0.5)
    want = p0 - sum(lr / (1 + d * it) * g for it, g in enumerate(gs))
    assert np.allclose(pr, want, rtol=1e-14)


def test_clipping_order_and_both_branches():
    a, b = np.array([3.0, 0.0]), np.array([0.0, 4.0])                      # norm over both weights = 5
    out = R.clip_gradients([a, b], clipnorm=1.0)                            # norm >= clipnorm: scaled to norm 1
    assert np.allclose(out[0], [0.6, 0]) and np.allclose(out[1], [0, 0.8])
    out = R.clip_gradients([a, b], clipnorm=5.0)                            # the boundary is inclusive (norm >= clipnorm) and scales by 1
    assert np.allclose(out[0], a) and np.allclose(out[1], b)
    out = R.clip_gradients([a, b], clipnorm=10.0)                           # below the limit: untouched
    assert np.array_equal(out[0], a) and np.array_equal(out[1], b)
    out = R.clip_gradients([a, b], clipnorm=2.5, clipvalue=1.0)             # clipnorm first (-> [1.5, 0], [0, 2]), then clipvalue
    assert np.allclose(out[0], [1.0, 0]) and np.allclose(out[1], [0, 1.0])
    out = R.clip_gradients([a, b], clipvalue=1.0, clipnorm=100.0)
    assert np.allclose(out[0], [1.0, 0]) and np.allclose(out[1], [0, 1.0])


CASES = [('SGD', dict(lr=0.004, momentum=0.9, nesterov=True, decay=1e-3)), ('RMSprop', dict(lr=1e-4, rho=0.8, clipnorm=1.0)),
         ('Adagrad', dict(epsilon=1e-6, clipvalue=0.5)), ('Adadelta', dict(rho=0.9, decay=0.01)), ('Adamax', dict(beta_1=0.8, clipnorm=2.0, clipvalue=0.1)),
         ('Adam', dict(lr=9e-5, beta_1=0.5, decay=1e-4, amsgrad=True))]


@pytest.mark.parametrize('cls,kw', CASES)
def test_training_config_roundtrip_without_stepping(tmp_path, cls, kw):
    from gennet_amd import bbh, engine
    from gennet_amd.keras.models import load_model
    m = bbh.signal_pe_model(64)
    opt = engine.OPTIMIZERS[cls](**kw)
    m.compile(loss='mean_squared_error', optimizer=opt, metrics=['accuracy'])
    path = str(tmp_path / 'm.h5')
    m.save(path, True)
    f = h5lite.File(path)
    oc = json.loads(f.attrs['training_config'].decode())['optimizer_config']
    assert oc == {'class_name': cls, 'config': opt.get_config()}
    assert 'optimizer_weights' not in f                                      # never stepped: no optimizer state
    m2 = load_model(path)
    assert type(m2.optimizer) is type(opt) and m2.optimizer.get_config() == opt.get_config()
    assert m2.optimizer.clipnorm == kw.get('clipnorm') and m2.optimizer.clipvalue == kw.get('clipvalue')


def _g_model_optimizer_weights():
    """(weight_names, arrays) of optimizer_weights in the reference's g_model.hdf5 (SGD, Keras 2.1.x)."""
    buf = gzip.decompress(open(os.path.join(ROOT, 'tests', 'golden', 'keras_h5', 'g_model.hdf5.gz'), 'rb').read())
    f = h5lite.File(buf)
    og = f['optimizer_weights']
    names = [n.decode() if isinstance(n, bytes) else n for n in og.attrs['weight_names']]
    return f, names, [og[n].value for n in names]


def test_sgd_pin_on_the_reference_g_model():
    from gennet_amd import engine
    f, names, vals = _g_model_optimizer_weights()
    tc = f.attrs['training_config']
    tc = json.loads(tc.decode() if isinstance(tc, bytes) else tc)
    assert tc['optimizer_config'] == {'class_name': 'SGD', 'config': {'decay': 0.0, 'lr': 0.004000000189989805, 'momentum': 0.0, 'nesterov': False}}
    opt = engine.optimizer_from_config(tc['optimizer_config'])
    assert opt.get_config() == tc['optimizer_config']['config']
    shapes = GOLD['g_model.hdf5']['datasets']
    n = len(names) - 1
    assert n == 26
    it, blocks = opt.split_keras_weights(vals, n)                          # by weight_names order: iterations, then one moment per trainable weight
    assert isinstance(it, int) and np.asarray(vals[0]).dtype == np.int64 and np.asarray(vals[0]).shape == ()
    assert len(blocks) == 1 and len(blocks[0]) == 26
    for nm, a in zip(names[1:], blocks[0]):
        assert list(np.shape(a)) == shapes['optimizer_weights/' + nm][0] and shapes['optimizer_weights/' + nm][1] == 'float32'
    assert names[0] == 'SGD/iterations:0' and names[1].startswith('training_1/SGD/')    # the scope prefix is the Keras session's, not fixed
    with pytest.raises(ValueError):
        engine.RMSprop().split_keras_weights(vals, n)                      # another class' layout does not fit


@pytest.mark.parametrize('cls,kw', CASES + [('Adam', {})])
def test_writer_layout_follows_keras(tmp_path, cls, kw, monkeypatch):
    """The writer's optimizer_weights group for a model of our own: names training/<Class>/Variable[_k]:0 in Keras' layout, iterations first
    where Keras saves it (state values come from the restatement: this runs without a device)."""
    from gennet_amd import bbh, engine
    m = bbh.signal_pe_model(64)
    opt = engine.OPTIMIZERS[cls](**kw)
    m.compile(loss='mean_squared_error', optimizer=opt)
    order = m._keras_train_order()
    ref = R.KerasOpt(cls.lower(), [p.numpy() for p in order], **{k: v for k, v in kw.items()})
    ref.iterations = 7
    rng = np.random.RandomState(0)
    for st in ref.state:
        for a in st:
            a[...] = rng.randn(*a.shape)
    monkeypatch.setattr(opt, 'get_keras_weights', lambda params: [np.asarray(a, np.int64) if np.ndim(a) == 0 else np.asarray(a, np.float32)
                                                                  for a in ref.keras_weights(params)])
    opt.state = []                                                          # as if bound
    path = str(tmp_path / 'w.h5')
    m.save(path, True)
    og = h5lite.File(path)['optimizer_weights']
    names = [n.decode() for n in og.attrs['weight_names']]
    lead, blocks = R.LAYOUT[cls.lower()]
    n = len(order)
    assert len(names) == int(lead) + len(blocks) * n
    if lead:
        assert names[0] == '%s/iterations:0' % cls and og[names[0]].value == 7 and og[names[0]].value.dtype == np.int64
    body = names[int(lead):]
    assert body == ['training/%s/Variable%s:0' % (cls, '' if k == 0 else '_%d' % k) for k in range(len(body))]
    vals = [og[nm].value for nm in names]
    it, got = opt.split_keras_weights(vals, n)
    assert it == (7 if lead else None)
    for k, blk in enumerate(got):
        if cls == 'Adam' and k == 2 and not kw.get('amsgrad'):
            assert all(a.shape == (1,) and not a.any() for a in blk)
        else:
            assert all(np.array_equal(a, np.float32(b)) for a, b in zip(blk, ref.state[k]))
