"""The reference's discriminator d_model.hdf5 and the GAN it forms with g_model.hdf5, on the GPU, against the fp64 restatements
(tests/d_model_ref.py, tests/g_model_ref.py): load_model, predict, Adam training of the unfrozen discriminator, GAN = D(G(z)) with D frozen,
the alternating loop with Keras' collect-at-compile trainability, captured training steps and save -> load_model.

d_model's Conv1D(50, 16) on one channel is tap-folded to 4 taps over 4 channels with 50 filters: forward, data gradient (50 -> 4, inside the
GAN) and weight gradient all need the any-channel kernels.  Only committed fixtures are read: the two weights-only files as the
reference ships them, the full-model file in its reduced form (dense_3's kernel zeroed, tests/golden/keras_h5/filled.json)."""
import gzip
import json
import os

import numpy as np
import pytest
import torch

import d_model_ref as R
import g_model_ref as RG

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H5 = os.path.join(ROOT, 'tests', 'golden', 'keras_h5')
GOLD = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'keras_h5_golden.json')))
LR_GAN = float(np.float32(0.004))


def d_file(tmp_path):
    path = str(tmp_path / 'd_model.hdf5')
    with open(path, 'wb') as fh:
        fh.write(gzip.decompress(open(os.path.join(H5, 'd_model.hdf5.gz'), 'rb').read()))
    return path


def weighted(m):
    from gennet_amd import keras_io
    return [l for l in keras_io.top_layers(m) if keras_io.keras_weights(l)]


def weights_of(m):
    from gennet_amd import keras_io
    return {l.name: [p.numpy() for p in keras_io.keras_weights(l)] for l in weighted(m)}


def load_d(tmp_path, trainable, compile_with=None):
    """d_model.hdf5 through load_model, the real weights of best_d_weights.hdf5 in it; trainable=True undoes the frozen state the file records."""
    from gennet_amd.keras.models import load_model
    m = load_model(d_file(tmp_path), compile=False)
    m.load_weights(os.path.join(H5, 'best_d_weights.hdf5'))
    m.trainable = trainable
    for l in m.layers:
        l.trainable = trainable
    if compile_with is not None:
        m.compile(optimizer=compile_with, loss='binary_crossentropy')
    return m


def load_g():
    from gennet_amd.engine import model_from_json
    g = model_from_json(json.dumps(GOLD['g_model.hdf5']['model_config']))
    g.load_weights(os.path.join(H5, 'best_g_weights.hdf5'))
    return g


def adam():
    from gennet_amd.engine import Adam
    return Adam(lr=0.004, beta_1=0.5)           # what the file's training_config records


def rel(a, ref):
    a = np.asarray(a, np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-30)


def assert_weights(m, P, names_of, what):
    """trained weights against the restatement: 1e-4 of the tensor's largest entry, floor 1e-3 (tests/test_g_model_gpu.py)"""
    from gennet_amd import keras_io
    for l in weighted(m):
        for p, n in zip(keras_io.keras_weights(l), names_of(l)):
            if n.startswith('moving'):
                continue
            w_ref = P[(l.name, n)].detach().numpy()
            err = np.abs(p.numpy().astype(np.float64) - w_ref).max() / max(np.abs(w_ref).max(), 1e-3)
            print(what, l.name, n, 'err %.3g' % err)
            assert err < 1e-4, (what, l.name, n, err)


def d_names(l):
    return ['kernel', 'bias']


def g_names(l):
    return ['gamma', 'beta', 'moving_mean', 'moving_variance'] if l.name.startswith('batch') else ['kernel', 'bias']


def one_hot(rng, n):
    t = np.zeros((n, 2), np.float32)
    t[np.arange(n), rng.randint(0, 2, n)] = 1.0
    return t


def test_load_model_and_predict(tmp_path):
    from gennet_amd.keras.models import load_model
    from gennet_amd import keras_io
    m = load_model(d_file(tmp_path))
    assert m.output_shape == (None, 2) and m.loss == 'binary_crossentropy'
    # the reduced file holds zeros for dense_3's kernel (the conv would not reach the output): a seeded one in its place
    rng = np.random.RandomState(0)
    dense_3 = [l for l in weighted(m) if l.name == 'dense_3'][0]
    k3 = keras_io.keras_weights(dense_3)[0]
    assert not k3.numpy().any()
    k3.assign((rng.randn(1750, 50) * 0.03).astype(np.float32))
    x = rng.randn(256, 50).astype(np.float32)
    for stage in ('file', 'best_d_weights'):
        if stage == 'best_d_weights':
            m.load_weights(os.path.join(H5, 'best_d_weights.hdf5'))
        y = m.predict(x, batch_size=256)
        with torch.no_grad():
            ref = R.forward(R.params_from(weights_of(m)), x.astype(np.float64)).numpy()
        print(stage, 'predict err %.3g' % rel(y, ref), 'spread of the outputs', ref.min(), ref.max())
        assert y.shape == (256, 2) and rel(y, ref) < 1e-5
        assert np.array_equal(y, np.concatenate([m.predict(x[:100], batch_size=64), m.predict(x[100:], batch_size=256)]))


def seed_weights(m, seed):
    from gennet_amd import keras_io
    rng = np.random.RandomState(seed)
    for l in weighted(m):
        for p in keras_io.keras_weights(l):
            p.assign((rng.randn(*p.shape) * (0.1 if len(p.shape) == 1 else 1.0 / np.sqrt(np.prod(p.shape[:-1])))).astype(np.float32))


@pytest.mark.parametrize('d_weights', ['best_d_weights', 'seeded'])
def test_five_adam_steps_match_fp64_restatement(tmp_path, d_weights):
    """With the shipped weights the discriminator is collapsed (gradients of ~3e-6 in the conv), and Adam's first steps are then close to
    lr * sign(g): 'seeded' repeats the steps from seeded weights, where the magnitude of the weight gradient counts.
    The discriminator unfrozen and compiled with the file's Adam(lr 0.004, beta_1 0.5) and binary cross-entropy; every step is checked against
    the fp64 step taken from the weights the GPU model holds at that point (the reason tests/test_g_model_gpu.py gives: the sigmoid outputs
    meet keras' clip, the free-running trajectories part); the fp64 Adam moments run along over the five steps."""
    m = load_d(tmp_path, True, adam())
    if d_weights == 'seeded':
        seed_weights(m, 6)
    rng = np.random.RandomState(1)
    x = rng.randn(256, 50).astype(np.float32)
    t = one_hot(rng, 256)
    opt = R.Adam()
    for step in range(5):
        P = R.params_from(weights_of(m))
        ref = R.train_step(P, opt, x.astype(np.float64), t.astype(np.float64))
        loss = m.train_on_batch(x, t)[0]
        print('step', step, 'loss', loss, 'ref', ref)
        assert abs(loss - ref) <= 1e-6 * abs(ref), (step, loss, ref)
        assert_weights(m, P, d_names, 'step %d' % step)


def build_gan(g, d):
    from gennet_amd.engine import Input, Model, SGD
    z = Input(shape=g.input_shapes[0])
    gan = Model(z, d(g(z)))
    gan.compile(optimizer=SGD(lr=0.004), loss='binary_crossentropy')
    return gan


@pytest.mark.parametrize('d_weights', ['best_d_weights', 'seeded'])
def test_gan_steps_train_the_generator_through_the_frozen_discriminator(tmp_path, d_weights):
    """GAN = Model(z, D(G(z))), D frozen, SGD(0.004), targets [0, 1]: the 50 -> 4 data gradient of d_model's folded conv inside a real model.
    The shipped discriminator answers 0.5 to within 1e-7 on every input (its loss sits at ln 2), so the gradient it hands the generator is
    tiny; 'seeded' repeats the steps with seeded discriminator weights, where that gradient moves the generator."""
    from gennet_amd import keras_io
    g, d = load_g(), load_d(tmp_path, False)
    if d_weights == 'seeded':
        seed_weights(d, 5)
    gan = build_gan(g, d)
    d_before = weights_of(d)
    rng = np.random.RandomState(2)
    z = rng.randn(256, 1, 1).astype(np.float32)
    t = np.tile(np.array([[0.0, 1.0]], np.float32), (256, 1))
    for step in range(3):
        PG = RG.params_from(weights_of(g))
        PD = R.params_from(weights_of(d), requires_grad=False)
        ref = R.gan_step(PG, PD, z.astype(np.float64), t.astype(np.float64), LR_GAN)
        loss = gan.train_on_batch(z, t)[0]
        print('step', step, 'loss', loss, 'ref', ref)
        assert abs(loss - ref) <= 1e-6 * abs(ref), (step, loss, ref)
        assert_weights(g, PG, g_names, 'step %d' % step)
    for name, ws in weights_of(d).items():
        for a, b in zip(ws, d_before[name]):
            assert np.array_equal(a, b), name


def test_alternating_loop_with_collect_at_compile_trainability(tmp_path):
    """Three rounds of D.train_on_batch on real rows stacked on G.predict(z), then GAN.train_on_batch: D compiled while trainable, the GAN
    compiled while D is frozen, and both keep what they collected at compile.  Every step re-anchored on the weights the GPU holds."""
    g = load_g()
    d = load_d(tmp_path, True, adam())
    d.trainable = False
    for l in d.layers:
        l.trainable = False
    gan = build_gan(g, d)
    assert len(d._train_params) == 6 and len(gan._train_params) == len([p for l in g.layers for p in l.trainable_params()])
    rng = np.random.RandomState(3)
    opt = R.Adam()
    for rnd in range(3):
        z = rng.randn(128, 1, 1).astype(np.float32)
        real = np.tanh(rng.randn(128, 50)).astype(np.float32)
        fake = g.predict(z, batch_size=128)
        with torch.no_grad():
            fake_ref = RG.forward(RG.params_from(weights_of(g)), z.astype(np.float64), False).numpy()
        assert rel(fake, fake_ref) < 1e-5
        X = np.concatenate([real, fake])
        T = np.concatenate([np.tile(np.array([[0.0, 1.0]], np.float32), (128, 1)), np.tile(np.array([[1.0, 0.0]], np.float32), (128, 1))])
        PD = R.params_from(weights_of(d))
        ref = R.train_step(PD, opt, X.astype(np.float64), T.astype(np.float64))
        loss = d.train_on_batch(X, T)[0]
        print('round', rnd, 'D loss', loss, 'ref', ref)
        assert abs(loss - ref) <= 1e-6 * abs(ref), (rnd, loss, ref)
        assert_weights(d, PD, d_names, 'round %d D' % rnd)
        d_now = weights_of(d)
        PG = RG.params_from(weights_of(g))
        t = np.tile(np.array([[0.0, 1.0]], np.float32), (128, 1))
        ref = R.gan_step(PG, R.params_from(d_now, requires_grad=False), z.astype(np.float64), t.astype(np.float64), LR_GAN)
        loss = gan.train_on_batch(z, t)[0]
        print('round', rnd, 'GAN loss', loss, 'ref', ref)
        assert abs(loss - ref) <= 1e-6 * abs(ref), (rnd, loss, ref)
        assert_weights(g, PG, g_names, 'round %d G' % rnd)
        for name, ws in weights_of(d).items():          # the GAN step leaves the discriminator alone
            for a, b in zip(ws, d_now[name]):
                assert np.array_equal(a, b), name


def test_captured_steps_and_save_load_equal_the_eager_run_bit_for_bit(tmp_path):
    from gennet_amd.engine import StepGraph, device
    from gennet_amd.keras.models import load_model
    rng = np.random.RandomState(4)
    xh = rng.randn(8, 50).astype(np.float32)
    th = one_hot(rng, 8)
    x = torch.tensor(xh, device=device()); t = torch.tensor(th, device=device())
    eager = load_d(tmp_path, True, adam())
    graphed = load_d(tmp_path, True, adam())
    la = [eager.train_result(eager.train_on_batch_device([x], [t]), 8) for _ in range(4)]
    graphed.train_on_batch_device([x], [t])          # one eager step first: binds the parameter groups and scratch buffers the graph will hold
    sg = StepGraph()
    torch.cuda.synchronize()
    sg.capture(lambda: graphed.train_on_batch_device([x], [t]))
    lb = []
    for i in range(3):
        if i:
            sg.wait_inputs_consumed()
        lb.append(graphed.train_result(sg.replay(), 8))
    assert la[1:] == lb
    for (name, ws), (_, vs) in zip(sorted(weights_of(eager).items()), sorted(weights_of(graphed).items())):
        for a, b in zip(ws, vs):
            assert np.array_equal(a, b), name
    # save -> load_model (weights, trainable flags, Adam's iteration count and moments) -> one more step = the uninterrupted run
    path = str(tmp_path / 'd_resumed.h5')
    eager.save(path)
    resumed = load_model(path)
    l5 = eager.train_on_batch(xh, th)
    assert resumed.train_on_batch(xh, th) == l5
    for (name, ws), (_, vs) in zip(sorted(weights_of(eager).items()), sorted(weights_of(resumed).items())):
        for a, b in zip(ws, vs):
            assert np.array_equal(a, b), name
