"""The definition of keras.layers.SimpleRNN (keras 2.2.4 layers/recurrent.py, SimpleRNNCell) in numpy: a forward and a hand-written backward
through time.  Run in fp64 it is the reference of tests/test_rnn_cpu.py (checked there against torch.nn.RNN and torch autograd) and
tests/test_rnn_gpu.py; run in fp32 (dtype=np.float32) it is the "restatement" whose own distance to fp64 is the yardstick of the sequence tests.

kernel W (Cin, u), recurrent_kernel U (u, u), bias b (u):
    h_t = act((x_t W + b) + h_{t-1} U)
Everything indexed by the PROCESSING step s: under go_backwards step s reads x[:, T-1-s]; `at_input_time` turns a (B, T, .) array around.
The shape table, the integer case and the seed rule of the GPU tests live here too, so that the CPU suite can hold them to their promises."""
import numpy as np

from lstm_ref import ACTIVATIONS, act, act_grad, at_input_time  # noqa: F401


def recurrence(zx, U, b, h0=None, activation='tanh', go_backwards=False, dtype=np.float64):
    """zx (B, T, u) = X W at the input time index.  -> cache, all (B, T, u) in processing order: h, h_prev, pre (the pre-activation)"""
    zx, U, b = np.asarray(zx, dtype), np.asarray(U, dtype), np.asarray(b, dtype)
    B, T, u = zx.shape[0], zx.shape[1], U.shape[0]
    h = np.zeros((B, u), dtype) if h0 is None else np.asarray(h0, dtype)
    k = dict(h0=h, U=U, b=b, activation=activation, go_backwards=go_backwards, h=np.zeros((B, T, u), dtype), h_prev=np.zeros((B, T, u), dtype),
             pre=np.zeros((B, T, u), dtype))
    for s in range(T):
        pre = h @ U + (zx[:, T - 1 - s if go_backwards else s] + b)
        k['h_prev'][:, s], k['pre'][:, s] = h, pre
        h = act(activation, pre)
        k['h'][:, s] = h
    return k


def recurrence_backward(k, dy):
    """dy (B, T, u) in processing order, or (B, u) for the last step.  -> dz (B, T, u) in processing order; dh0, dU, db"""
    U, an = k['U'], k['activation']
    B, T, u = k['h'].shape
    dt = U.dtype
    dy = np.asarray(dy, dt)
    dh = np.zeros((B, u), dt)
    dz = np.zeros((B, T, u), dt)
    dU = np.zeros_like(U)
    for s in range(T - 1, -1, -1):
        dhv = (dy[:, s] if dy.ndim == 3 else (dy if s == T - 1 else 0)) + dh
        dz[:, s] = dhv * act_grad(an, k['pre'][:, s], k['h'][:, s])
        dh = dz[:, s] @ U.T
        dU += k['h_prev'][:, s].T @ dz[:, s]
    return dict(dz=dz, dh0=dh, dU=dU, db=dz.sum((0, 1)))


def forward(x, W, U, b, h0=None, activation='tanh', return_sequences=False, go_backwards=False, dtype=np.float64):
    """The layer: x (B, T, Cin) -> (y, cache); y (B, T, u) in processing order, or (B, u)"""
    x, W = np.asarray(x, dtype), np.asarray(W, dtype)
    k = recurrence(x @ W, U, b, h0, activation, go_backwards, dtype)
    k.update(x=x, W=W, return_sequences=return_sequences)
    return (k['h'] if return_sequences else k['h'][:, -1]), k


def backward(k, dy):
    """-> dx, dW, dU, db, dh0 for the gradient dy of forward's y"""
    r = recurrence_backward(k, dy)
    dz_t = at_input_time(r['dz'], k['go_backwards'])
    return dict(dx=dz_t @ k['W'].T, dW=np.einsum('btc,btv->cv', k['x'], dz_t), dU=r['dU'], db=r['db'], dh0=r['dh0'])


def torch_forward(x, W, U, b, h0=None, activation='tanh', return_sequences=False, go_backwards=False):
    """The same recurrence on torch tensors (any dtype; autograd runs through it)"""
    import torch
    f = {'tanh': torch.tanh, 'sigmoid': torch.sigmoid, 'relu': torch.relu, 'linear': lambda v: v}[activation]
    B, T, u = x.shape[0], x.shape[1], U.shape[0]
    h = torch.zeros((B, u), dtype=x.dtype) if h0 is None else h0
    zx = x @ W
    hs = []
    for s in range(T):
        h = f((zx[:, T - 1 - s if go_backwards else s] + b) + h @ U)
        hs.append(h)
    return torch.stack(hs, 1) if return_sequences else h


# ---------------------------------------------------------------------------------------------------------------------
# the shape table of tests/test_rnn_gpu.py, the integer case and the seed rule of its sequence test
# ---------------------------------------------------------------------------------------------------------------------
# (B, T, Cin, u): the 24 (B, T, Cin) of tests/test_lstm_gpu.py with u moved to the SimpleRNN geometry's own edges (csrc/rnn_geom.h): U is held in
# LDS up to u = 176 and streamed from 177, in the forward and in the backward alike; 128 | 129: one tile a wave, two (both with U in LDS);
# 130, 260, 512: two, three, four tiles a wave
SHAPES = [(1, 1, 1, 1), (2, 2, 3, 3), (15, 3, 16, 4), (16, 17, 17, 15), (17, 1, 1, 16), (33, 2, 3, 17), (1, 3, 16, 31), (2, 17, 17, 32),
          (15, 1, 3, 33), (16, 2, 1, 64), (17, 3, 17, 176), (33, 1, 16, 177), (1, 2, 16, 176), (2, 3, 1, 177), (15, 2, 3, 129), (16, 1, 17, 130),
          (2, 2, 16, 260), (2, 3, 3, 512), (1, 17, 1, 64), (2, 1, 17, 128), (17, 2, 3, 130), (33, 17, 16, 4), (17, 1, 1, 512), (15, 2, 1, 33)]
IDS = ['b%d-t%d-c%d-u%d' % s for s in SHAPES]


def integer_case(shape):
    """Integer inputs of the exactness test for a shape, activation='linear', all T steps: x in [-2, 2], W and b in {-1, 0, 1}, h0 in [-2, 2].
    A linear recurrence grows as ||U||^T, so U is the sum of d signed permutation matrices (every row and every column has at most d non-zero
    entries, of absolute sum at most d) with d = 3 up to T = 3 and d = 1 above: |h_t| <= c + d |h_{t-1}|, and the backward the same through
    U^T.  -> dict(zx, U, b, h0, cases, big): cases = [(reverse, dy, k, r)] for both walking directions with dy a sequence and the reversed one
    with dy a last row; big bounds every partial sum of the forward and the backward by sums of absolute values."""
    B, T, Cin, u = shape
    rng = np.random.RandomState(B * 1000 + T * 100 + Cin * 10 + u)
    x = rng.randint(-2, 3, (B, T, Cin)).astype(np.float64)
    W = rng.randint(-1, 2, (Cin, u)).astype(np.float64)
    U = np.zeros((u, u))
    for _ in range(3 if T <= 3 else 1):
        U[np.arange(u), rng.permutation(u)] += rng.choice([-1.0, 1.0], u)
    b = rng.randint(-1, 2, u).astype(np.float64)
    h0 = rng.randint(-2, 3, (B, u)).astype(np.float64)
    zx = x @ W
    aU = np.abs(U)
    cases, big = [], 0.0
    for reverse, seq in ((False, True), (True, True), (True, False)):
        dy = rng.randint(-1, 2, (B, T, u) if seq else (B, u)).astype(np.float64)
        k = recurrence(zx, U, b, h0, 'linear', reverse)
        r = recurrence_backward(k, dy)
        big = max(big, float((np.abs(k['h_prev']) @ aU).max() + np.abs(zx).max() + 1), float((np.abs(r['dz']) @ aU.T).max() + 1),
                  2 * float(np.abs(k['h']).max()), 2 * float(np.abs(r['dz']).max()))
        cases.append((reverse, dy, k, r))
    return dict(zx=zx, U=U, b=b, h0=h0, cases=cases, big=big)


FAMILIES = ('keras', 'saturating')


def draw_family(family, rng, B, T, Cin, u):
    """-> x, W, U, b.  'keras': keras' own initialisation, Glorot kernel and an orthogonal recurrent kernel; its zero bias is moved by
    0.1 N(0, 1).  'saturating': x ~ 2 N(0, 1), W ~ 1.5 U(-1, 1), U ~ (3 / sqrt(u)) U(-1, 1), b ~ U(-1, 1)."""
    from gennet_amd import engine
    from gennet_amd.recurrent import orthogonal_blocks
    f32 = lambda a: a.astype(np.float32)          # noqa: E731
    if family == 'keras':
        engine.set_init_seed(int(rng.randint(1 << 30)))
        return f32(rng.randn(B, T, Cin)), engine.glorot_uniform((Cin, u)), orthogonal_blocks(u, 1), f32(0.1 * rng.randn(u))
    return f32(2 * rng.randn(B, T, Cin)), f32(1.5 * (rng.rand(Cin, u) * 2 - 1)), f32(3 / np.sqrt(u) * (rng.rand(u, u) * 2 - 1)), f32(rng.rand(u) * 2 - 1)


def kink_margin(k):
    """the smallest distance of a pre-activation to a point where the activation's derivative jumps: 0 for relu, none for the others"""
    return float(np.abs(k['pre']).min()) if k['activation'] == 'relu' else np.inf


def sequence_case(shape, family, activation):
    """The case of the sequence test for SHAPES[n]: its direction and dy form by n, and the first seed of 0 .. 31 whose smallest distance to a
    derivative jump is at least 64 times the fp32 restatement's largest pre-activation error -- chosen from the reference alone.
    -> dict(seed, reverse, seq, x, W, U, b, dy, k64, k32), or None where no seed does."""
    B, T, Cin, u = shape
    n = SHAPES.index(shape)
    reverse, seq = bool(n & 1), bool(n & 2)
    for seed in range(32):
        rng = np.random.RandomState(seed * 100 + n)
        x, W, U, b = draw_family(family, rng, B, T, Cin, u)
        dy = rng.randn(*((B, T, u) if seq else (B, u))).astype(np.float32)
        _, k64 = forward(x, W, U, b, None, activation, seq, reverse)
        _, k32 = forward(x, W, U, b, None, activation, seq, reverse, dtype=np.float32)
        if kink_margin(k64) >= 64 * float(np.abs(k32['pre'] - k64['pre']).max()):
            return dict(seed=seed, reverse=reverse, seq=seq, x=x, W=W, U=U, b=b, dy=dy, k64=k64, k32=k32)
    return None
