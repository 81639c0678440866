"""GaussianNoise, GaussianDropout and AlphaDropout on the device (csrc/noise_layers.hip): the draws are fill_normal's and dropout_mask's bit for
bit, the passes match an fp64 restatement, the statistics are Keras', and the layers train like an fp64 torch restatement inside a model, in the
discriminator and the GAN, under graph replay and under a data-parallel row map, taking exactly their counters of the device stream."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ALPHA_P = -1.6732632423543772848170429916717 * 1.0507009873554804934193349852946


def _dev():
    return torch.device('cuda:0')


def _bits(t):
    return t.contiguous().view(torch.int32)


def _alpha_consts(rate):
    a = ((1.0 - rate) * (1.0 + rate * ALPHA_P ** 2)) ** -0.5
    return float(np.float32(a)), float(np.float32(-a * ALPHA_P * rate)), float(np.float32(ALPHA_P))


def _buf(n, fill, lead):
    """n floats starting `lead` floats into a fresh buffer: lead % 4 != 0 gives a pointer that is not 16-byte aligned."""
    b = torch.full((n + lead,), float(fill), device=_dev())
    return b[lead:]


def _call(name, *args):
    from gennet_amd import _lib
    _lib.call(name, *args, torch.cuda.current_stream().cuda_stream)


CASES = [(1, 0, 0, 0), (7, 12345, 1, 0), (4097, 3, 0, 3), ((1 << 16) + 3, 1 << 33, 2, 1), (1 << 20, 77, 0, 0)]


@pytest.mark.parametrize('n,offset,lead_x,lead_y', CASES)
def test_draws_are_fill_normal_and_dropout_mask_bit_for_bit(n, offset, lead_x, lead_y):
    from gennet_amd import ops
    seed = 0x1234567890
    x0, x1 = _buf(n, 0.0, lead_x), _buf(n, 1.0, lead_x)
    y = _buf(n, float('nan'), lead_y)
    _call('gn_gaussian_noise_fwd', x0.data_ptr(), y.data_ptr(), n, ctypes.c_float(0.7), seed, offset)
    assert torch.equal(_bits(y), _bits(ops.fill_normal((n,), 0.0, 0.7, seed, offset, _dev())))
    _call('gn_gaussian_dropout_apply', x1.data_ptr(), y.data_ptr(), n, ctypes.c_float(0.8), seed, offset)
    assert torch.equal(_bits(y), _bits(ops.fill_normal((n,), 1.0, 0.8, seed, offset, _dev())))
    rate = 0.3
    a, b, ap = _alpha_consts(rate)
    xp = _buf(n, 0.0, lead_x)
    xp.copy_(ops.fill_uniform((n,), 0.5, 2.0, 9, 0, _dev()))          # > 0: a x + b > 0 > a alpha_p + b, so the sign is the keep bit
    _call('gn_alpha_dropout_fwd', xp.data_ptr(), y.data_ptr(), n, ctypes.c_float(rate), ctypes.c_float(a), ctypes.c_float(b), ctypes.c_float(ap), seed, offset)
    keep = ops.dropout_mask((n,), rate, seed, offset, _dev()).bool()
    assert torch.equal(y > 0, keep)
    dx = _buf(n, float('nan'), lead_y)
    _call('gn_alpha_dropout_bwd', xp.data_ptr(), dx.data_ptr(), n, ctypes.c_float(rate), ctypes.c_float(a), seed, offset)
    assert torch.equal(dx != 0, keep)
    # in place is allowed
    z = _buf(n, 0.0, lead_x)
    _call('gn_gaussian_noise_fwd', z.data_ptr(), z.data_ptr(), n, ctypes.c_float(0.7), seed, offset)
    assert torch.equal(_bits(z), _bits(ops.fill_normal((n,), 0.0, 0.7, seed, offset, _dev())))


@pytest.mark.parametrize('n,offset,lead_x,lead_y', CASES[1:])
def test_passes_match_fp64_given_the_draw(n, offset, lead_x, lead_y):
    from gennet_amd import ops
    seed, eps = 31, 2.0 ** -23
    x = _buf(n, 0.0, lead_x)
    x.copy_(ops.fill_normal((n,), 0.5, 3.0, 8, 0, _dev()))
    z = ops.fill_normal((n,), 0.0, 1.0, seed, offset, _dev()).double()
    xd = x.double()
    y = _buf(n, 0.0, lead_y)
    # GaussianNoise
    ops.gaussian_noise(x, 0.45, seed, offset, out=y)
    ref = xd + 0.45 * z
    assert ((y.double() - ref).abs() <= 2 * eps * (xd.abs() + (0.45 * z).abs())).all()
    # GaussianDropout, and its backward = the same pass on dy with the forward's counters
    sd = float(np.float32(np.sqrt(0.4 / 0.6)))
    ops.gaussian_dropout(x, sd, seed, offset, out=y)
    m = 1.0 + sd * z
    assert ((y.double() - xd * m).abs() <= 3 * eps * xd.abs() * (1.0 + (sd * z).abs())).all()
    ones = ops.gaussian_dropout(torch.ones(n, device=_dev()), sd, seed, offset)
    assert torch.equal(_bits(y), _bits(x * ones))                      # dy * m with the SAME fp32 m the forward used
    dy = ops.fill_normal((n,), 0.0, 1.0, 123, 0, _dev())
    assert torch.equal(_bits(ops.gaussian_dropout(dy, sd, seed, offset)), _bits(dy * ones))
    # AlphaDropout forward and backward
    rate = 0.2
    a, b, ap = _alpha_consts(rate)
    keep = ops.dropout_mask((n,), rate, seed, offset, _dev()).bool()
    ops.alpha_dropout_fwd(x, rate, a, b, ap, seed, offset, out=y)
    ref = torch.where(keep, a * xd + b, torch.full_like(xd, a * ap + b))
    assert ((y.double() - ref).abs() <= 2 * eps * (abs(a) * xd.abs() + abs(b) + abs(a * ap))).all()
    dx = ops.alpha_dropout_bwd(dy, rate, a, seed, offset)
    ref = torch.where(keep, a * dy.double(), torch.zeros_like(xd))
    assert ((dx.double() - ref).abs() <= eps * (a * dy.double()).abs()).all()


def test_statistics_over_2_pow_24():
    from gennet_amd import ops
    N = 1 << 24
    z = ops.gaussian_noise(torch.zeros(N, device=_dev()), 1.0, 5, 1000, out=None).double()
    mean, var = z.mean().item(), z.var().item()
    assert abs(mean) < 5 / np.sqrt(N) and abs(var - 1.0) < 5 * np.sqrt(2.0 / N), (mean, var)
    rate = 0.4
    a, b, ap = _alpha_consts(rate)
    x = ops.fill_normal((N,), 0.0, 1.0, 6, 0, _dev())
    y = ops.alpha_dropout_fwd(x, rate, a, b, ap, 5, 2000).double()
    kept = (y != float(np.float32(np.float32(a) * np.float32(ap)) + np.float32(b))).double().mean().item()
    assert abs(kept - (1 - rate)) < 5 * np.sqrt(rate * (1 - rate) / N), kept
    m, v = y.mean().item(), y.var().item()                            # self-normalising: N(0, 1) in, mean 0 and variance 1 out
    se_v = ((y - m) ** 2).std().item() / np.sqrt(N)
    assert abs(m) < 5 * np.sqrt(v / N) and abs(v - 1.0) < 5 * se_v, (m, v)


def _small_model(optimizer):
    from gennet_amd.keras.layers import Activation, AlphaDropout, Dense, GaussianDropout, GaussianNoise
    from gennet_amd.keras.models import Sequential
    m = Sequential()
    m.add(Dense(16, input_shape=(12,)))
    m.add(GaussianNoise(0.3))
    m.add(Activation('tanh'))
    m.add(GaussianDropout(0.25))
    m.add(Dense(8))
    m.add(AlphaDropout(0.2))
    m.add(Dense(1))
    m.compile(loss='mean_squared_error', optimizer=optimizer)
    return m


def test_train_step_matches_an_fp64_torch_restatement():
    from gennet_amd import engine, ops
    engine.set_init_seed(21); engine.set_device_seed(17)
    B, lr = 16, 0.1
    m = _small_model(engine.SGD(lr=lr))
    rng = np.random.RandomState(2)
    x = rng.randn(B, 12).astype(np.float32); yt = rng.randn(B).astype(np.float32)
    w = [torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in m.get_weights()]
    s = engine.device_rng()
    seed, off = s.seed, s.offset
    n1 = ops.fill_normal((B, 16), 0.0, 0.3, seed, off, _dev()).cpu().double()
    m2 = ops.fill_normal((B, 16), 1.0, m._top[3].sd, seed, off + B * 16 // 4, _dev()).cpu().double()
    keep = ops.dropout_mask((B, 8), 0.2, seed, off + 2 * B * 16 // 4, _dev()).cpu().bool()
    loss = m.train_on_batch(x, yt)
    assert s.offset == off + (2 * B * 16 + B * 8) // 4
    a, b, ap = _alpha_consts(0.2)
    h = torch.tensor(x, dtype=torch.float64) @ w[0] + w[1]
    h = torch.tanh(h + n1) * m2
    h = h @ w[2] + w[3]
    h = torch.where(keep, a * h + b, torch.full_like(h, a * ap + b))
    out = h @ w[4] + w[5]
    ref = ((out.reshape(-1) - torch.tensor(yt, dtype=torch.float64)) ** 2).mean()
    ref.backward()
    assert abs(loss[0] - ref.item()) <= 1e-5 * abs(ref.item()), (loss, ref.item())
    for got, p in zip(m.get_weights(), w):
        new = (p - lr * p.grad).detach().numpy()
        assert np.abs(got - new).max() <= 1e-5 * np.abs(new).max()


def test_discriminator_input_noise_trains_like_noisy_input():
    from gennet_amd import bbh, engine, ops
    n_pix, B, s = 64, 4, 0.25
    engine.set_init_seed(4); engine.set_device_seed(8)
    d1 = bbh.signal_discriminator_model(n_pix, input_noise=s)
    d0 = bbh.signal_discriminator_model(n_pix)
    d0.set_weights(d1.get_weights())
    for d in (d0, d1):
        d.compile(loss='binary_crossentropy', optimizer=engine.Adam(lr=9e-5, beta_1=0.5), metrics=['accuracy'])
    rng = np.random.RandomState(5)
    x = rng.randn(B, n_pix, 2, 1).astype(np.float32); y = (np.arange(B) < B // 2).astype(np.float32)
    drops = [[l for l in d._top if l.__class__.__name__ == 'Dropout'] for d in (d0, d1)]
    shapes = [(B, n_pix // 2, 2, 256), (B, n_pix // 4, 2, 512)]
    for step in range(3):
        masks = [(rng.uniform(size=sh) >= 0.4).astype(np.uint8) for sh in shapes]
        st = engine.device_rng()
        seed, off = st.seed, st.offset
        l1 = d1.train_on_batch(x, y, dropout_masks=dict((l.name, mk) for l, mk in zip(drops[1], masks)))
        assert st.offset == off + B * n_pix * 2 // 4                  # only the noise layer drew
        xn = engine.to_device(x) + ops.fill_normal(x.shape, 0.0, s, seed, off, _dev())
        l0 = d0.train_on_batch(xn, y, dropout_masks=dict((l.name, mk) for l, mk in zip(drops[0], masks)))
        assert abs(l1[0] - l0[0]) <= 2e-5 * abs(l0[0]), (l1, l0)
    for a, b in zip(d1.get_weights(), d0.get_weights()):
        assert np.abs(a - b).max() <= 2e-5 * max(np.abs(b).max(), 1e-30)
    # the inference phase is the identity and takes nothing
    off = engine.device_rng().offset
    p1, p0 = d1.predict(x), d0.predict(x)
    assert engine.device_rng().offset == off and np.abs(p1 - p0).max() <= 2e-5


@pytest.mark.parametrize('dropout', ['gaussian', 'alpha'])
def test_frozen_discriminator_in_the_gan(dropout):
    from gennet_amd import bbh, engine
    n_pix, B = 128, 4
    engine.set_init_seed(6); engine.set_device_seed(12)
    rng = np.random.RandomState(6)
    event = rng.randn(n_pix, 1).astype(np.float32)
    nets = bbh.build_and_compile(event, n_pix, do_pe=False, d_config={'input_noise': 0.1, 'dropout': dropout})
    kinds = [l.__class__.__name__ for l in nets.signal_discriminator._top]
    assert kinds[0] == 'GaussianNoise' and kinds.count({'gaussian': 'GaussianDropout', 'alpha': 'AlphaDropout'}[dropout]) == 2
    bank = bbh.DeviceBank(rng.randn(32, n_pix).astype(np.float32), np.stack([rng.uniform(20, 35, 32), rng.uniform(0.5, 1, 32)], 1))
    ev = engine.to_device(event.reshape(-1))
    for _ in range(2):
        r = bbh.gan_train_step(nets, bank, ev, B)
        assert all(np.isfinite(r)), r
    wd = nets.signal_discriminator.get_weights(); wg = nets.generator.get_weights()
    off = engine.device_rng().offset
    z = np.random.RandomState(1).uniform(-1, 1, (B, 100)).astype(np.float32)
    sg = nets.signal_discriminator_on_generator.train_on_batch(z, np.ones(B, np.float32))
    assert np.isfinite(sg[0]) and engine.device_rng().offset > off        # D's noise layers are active in the combined step
    assert all(np.array_equal(a, b) for a, b in zip(wd, nets.signal_discriminator.get_weights()))
    assert not all(np.array_equal(a, b) for a, b in zip(wg, nets.generator.get_weights()))


def test_graph_replay_is_bit_identical_to_eager_steps():
    from gennet_amd import engine
    B, steps = 8, 5
    rng = np.random.RandomState(3)
    x = engine.to_device(rng.randn(B, 12).astype(np.float32)); y = engine.to_device(rng.randn(B, 1).astype(np.float32))

    def run(graphed):
        engine.set_init_seed(9); engine.set_device_seed(33)
        m = _small_model(engine.Adam(lr=1e-3))
        out, sg = [], None
        for i in range(steps):
            if not graphed or i == 0:
                out.append(m.train_on_batch_device([x], [y]).cpu().numpy())
                continue
            if sg is None:
                sg = engine.StepGraph()
                torch.cuda.synchronize()
                sg.capture(lambda: m.train_on_batch_device([x], [y]))
            out.append(sg.replay().cpu().numpy())
        return out, m.get_weights(), engine.device_rng().offset

    eager, graph = run(False), run(True)
    assert all(np.array_equal(a, b) for a, b in zip(eager[0], graph[0]))
    assert all(np.array_equal(a, b) for a, b in zip(eager[1], graph[1]))
    assert eager[2] == graph[2]
    assert not np.array_equal(eager[0][1], eager[0][2])                 # the steps drew different noise


class _Node(object):
    index = 0


@pytest.mark.parametrize('row_len', [24, 6])
def test_row_map_gives_every_global_row_its_draw(row_len):
    """bbh.gan_train_step's row map (bbh.py: real rows of the rank, then the mirrored rank's block of the reversed fake half) on one GPU: every
    global row gets what the plain global batch gives it, forward and backward."""
    from gennet_amd import engine, ops
    from gennet_amd.layers import AlphaDropout, GaussianDropout, GaussianNoise
    b, world = 2, 2
    G = 2 * world * b
    x = ops.fill_normal((G, row_len), 0.0, 1.0, 1, 0, _dev()); dy = ops.fill_normal((G, row_len), 0.0, 1.0, 2, 0, _dev())
    for layer in (GaussianNoise(0.5), GaussianDropout(0.3), AlphaDropout(0.3)):
        engine.set_device_seed(9)
        ctx = engine.RunContext(True)
        y = layer.forward(ctx, _Node, x)
        dx = layer.backward(ctx, _Node, dy, True, False)
        end = engine.device_rng().offset
        assert end == (G * row_len + 3) // 4
        for rank in range(world):
            blocks = [(rank * b, b), (world * b + (world - 1 - rank) * b, b)]
            rows = torch.cat([torch.arange(g0, g0 + nr) for g0, nr in blocks]).to(_dev())
            engine.set_device_seed(9)
            ctx = engine.RunContext(True, row_map=(blocks, G))
            yl = layer.forward(ctx, _Node, x[rows].contiguous())
            dxl = layer.backward(ctx, _Node, dy[rows].contiguous(), True, False)
            assert torch.equal(_bits(yl), _bits(y[rows])) and torch.equal(_bits(dxl), _bits(dx[rows]))
            assert engine.device_rng().offset == end
    # a rank that holds only some global rows, one block starting at a pointer that is not 16-byte aligned when row_len = 6
    layer = GaussianDropout(0.3)
    engine.set_device_seed(9)
    y = layer.forward(engine.RunContext(True), _Node, x[:6].contiguous())
    blocks = [(4, 1), (0, 2)]
    rows = torch.tensor([4, 0, 1], device=_dev())
    engine.set_device_seed(9)
    yl = layer.forward(engine.RunContext(True, row_map=(blocks, 6)), _Node, x[:6][rows].contiguous())
    assert torch.equal(_bits(yl), _bits(y[rows]))
    assert engine.device_rng().offset == (6 * row_len + 3) // 4


def test_counter_accounting():
    from gennet_amd import engine
    from gennet_amd.keras.layers import AlphaDropout, Dense, GaussianDropout, GaussianNoise
    from gennet_amd.keras.models import Sequential
    B = 5
    engine.set_device_seed(4)
    m = _small_model(engine.SGD(lr=0.01))
    x = np.random.RandomState(0).randn(B, 12).astype(np.float32); y = np.zeros(B, np.float32)
    s = engine.device_rng()
    off = s.offset
    m.train_on_batch(x, y)
    assert s.offset - off == 2 * -(-B * 16 // 4) + -(-B * 8 // 4)
    off = s.offset
    p = m.predict(x)
    assert s.offset == off and np.isfinite(p).all()
    # identity rates take nothing and change nothing, also in training
    idm = Sequential()
    idm.add(Dense(4, input_shape=(12,)))
    idm.add(GaussianDropout(0.0)); idm.add(AlphaDropout(1.0)); idm.add(GaussianDropout(1.5)); idm.add(AlphaDropout(0.0))
    idm.add(Dense(1))
    idm.compile(loss='mean_squared_error', optimizer=engine.SGD(lr=0.01))
    cap = {}
    off = s.offset
    idm.train_on_batch(x, y, capture=cap)
    assert s.offset == off
    names = [l.name for l in idm._top]
    for a, b in zip(names[1:5], names[2:5]):
        assert torch.equal(cap[a], cap[b])
    assert torch.equal(cap[names[0]], cap[names[4]])
    # GaussianNoise(0) still draws in training (keras: `inputs + K.random_normal(..., stddev=0)`)
    gm = Sequential()
    gm.add(Dense(4, input_shape=(12,))); gm.add(GaussianNoise(0.0)); gm.add(Dense(1))
    gm.compile(loss='mean_squared_error', optimizer=engine.SGD(lr=0.01))
    off = s.offset
    gm.train_on_batch(x, y)
    assert s.offset - off == -(-B * 4 // 4)
