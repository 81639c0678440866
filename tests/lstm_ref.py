"""The definition of keras.layers.LSTM (keras 2.2.4 layers/recurrent.py, LSTMCell) in numpy: a forward and a hand-written backward through time.
Run in fp64 it is the reference of tests/test_lstm_cpu.py (checked there against torch.nn.LSTM and torch autograd) and tests/test_lstm_gpu.py;
run in fp32 (dtype=np.float32) it is the "restatement" whose own distance to fp64 is the yardstick of the sequence tests.

Gate column order i, f, c, o in kernel W (Cin, 4u), recurrent_kernel U (u, 4u), bias b (4u):
    z_t = x_t W + h_{t-1} U + b;  i = ra(z_i), f = ra(z_f), g = act(z_c), o = ra(z_o);  c_t = f c_{t-1} + i g;  h_t = o act(c_t)
Everything indexed by the PROCESSING step s: under go_backwards step s reads x[:, T-1-s]; `at_input_time` turns a (B, T, .) array around."""
import numpy as np

ACTIVATIONS = ('tanh', 'sigmoid', 'relu', 'linear')
RECURRENT_ACTIVATIONS = ('hard_sigmoid', 'sigmoid')


def act(name, x):
    if name == 'tanh':
        return np.tanh(x)
    if name == 'sigmoid':
        e = np.exp(-np.abs(x))                  # no overflow on either side
        return np.where(x >= 0, 1 / (1 + e), e / (1 + e))
    if name == 'relu':
        return np.maximum(x, 0)
    if name == 'hard_sigmoid':
        return np.clip(x.dtype.type(0.2) * x + x.dtype.type(0.5), 0, 1)
    assert name == 'linear', name
    return x


def act_grad(name, x, y):
    """d act / dx at pre-activation x with y = act(x); hard_sigmoid: 0.2 strictly inside (-2.5, 2.5), 0 elsewhere"""
    if name == 'tanh':
        return 1 - y * y
    if name == 'sigmoid':
        return y * (1 - y)
    if name == 'relu':
        return (x > 0).astype(x.dtype)
    if name == 'hard_sigmoid':
        return np.where((x > -2.5) & (x < 2.5), x.dtype.type(0.2), x.dtype.type(0))
    return np.ones_like(x)


def at_input_time(a, go_backwards):
    return a[:, ::-1] if go_backwards else a


def recurrence(zx, U, b, h0=None, c0=None, activation='tanh', recurrent_activation='hard_sigmoid', go_backwards=False, dtype=np.float64):
    """zx (B, T, 4u) = X W at the input time index.  -> cache: h, c (B, T, u), z and gates (B, T, 4u), all in processing order."""
    zx, U, b = np.asarray(zx, dtype), np.asarray(U, dtype), np.asarray(b, dtype)
    B, T, u = zx.shape[0], zx.shape[1], U.shape[0]
    h_prev = np.zeros((B, u), dtype) if h0 is None else np.asarray(h0, dtype)
    c_prev = np.zeros((B, u), dtype) if c0 is None else np.asarray(c0, dtype)
    k = dict(h0=h_prev, c0=c_prev, U=U, b=b, activation=activation, recurrent_activation=recurrent_activation, go_backwards=go_backwards,
             h=np.zeros((B, T, u), dtype), c=np.zeros((B, T, u), dtype), z=np.zeros((B, T, 4 * u), dtype), gates=np.zeros((B, T, 4 * u), dtype))
    for s in range(T):
        z = (h_prev @ U + zx[:, T - 1 - s if go_backwards else s]) + b
        i, f, o = (act(recurrent_activation, z[:, q * u:(q + 1) * u]) for q in (0, 1, 3))
        g = act(activation, z[:, 2 * u:3 * u])
        c_prev = f * c_prev + i * g
        h_prev = o * act(activation, c_prev)
        k['z'][:, s], k['gates'][:, s], k['c'][:, s], k['h'][:, s] = z, np.concatenate([i, f, g, o], 1), c_prev, h_prev
    return k


def recurrence_backward(k, dy):
    """dy (B, T, u) in processing order, or (B, u) for the last step.  -> dz (B, T, 4u) in processing order, dh0, dc0, dU, db"""
    U, an, rn = k['U'], k['activation'], k['recurrent_activation']
    B, T, u = k['h'].shape
    dt = U.dtype
    dy = np.asarray(dy, dt)
    dh, dc = np.zeros((B, u), dt), np.zeros((B, u), dt)
    dz = np.zeros((B, T, 4 * u), dt)
    for s in range(T - 1, -1, -1):
        z, gt = k['z'][:, s], k['gates'][:, s]
        i, f, g, o = (gt[:, q * u:(q + 1) * u] for q in range(4))
        c, c_prev = k['c'][:, s], (k['c'][:, s - 1] if s else k['c0'])
        dhv = (dy[:, s] if dy.ndim == 3 else (dy if s == T - 1 else 0)) + dh
        tc = act(an, c)
        dcv = dc + (dhv * o) * act_grad(an, c, tc)
        dz[:, s] = np.concatenate([(dcv * g) * act_grad(rn, z[:, :u], i), (dcv * c_prev) * act_grad(rn, z[:, u:2 * u], f),
                                   (dcv * i) * act_grad(an, z[:, 2 * u:3 * u], g), (dhv * tc) * act_grad(rn, z[:, 3 * u:], o)], 1)
        dc = dcv * f
        dh = dz[:, s] @ U.T
    h_prev = np.concatenate([k['h0'][:, None], k['h'][:, :-1]], 1)
    return dict(dz=dz, dh0=dh, dc0=dc, dU=np.einsum('bsu,bsv->uv', h_prev, dz), db=dz.sum((0, 1)), h_prev=h_prev)


def forward(x, W, U, b, h0=None, c0=None, activation='tanh', recurrent_activation='hard_sigmoid', return_sequences=False, go_backwards=False,
            dtype=np.float64):
    """The layer: x (B, T, Cin) -> (y, cache); y (B, T, u) in processing order, or (B, u)"""
    x, W = np.asarray(x, dtype), np.asarray(W, dtype)
    k = recurrence(x @ W, U, b, h0, c0, activation, recurrent_activation, go_backwards, dtype)
    k.update(x=x, W=W, return_sequences=return_sequences)
    return (k['h'] if return_sequences else k['h'][:, -1]), k


def backward(k, dy):
    """-> dx, dW, dU, db, dh0, dc0 for the gradient dy of forward's y"""
    r = recurrence_backward(k, dy)
    dz_t = at_input_time(r['dz'], k['go_backwards'])
    return dict(dx=dz_t @ k['W'].T, dW=np.einsum('btc,btv->cv', k['x'], dz_t), dU=r['dU'], db=r['db'], dh0=r['dh0'], dc0=r['dc0'])


def torch_forward(x, W, U, b, h0=None, c0=None, activation='tanh', recurrent_activation='hard_sigmoid', return_sequences=False, go_backwards=False):
    """The same recurrence on torch tensors (any dtype; autograd runs through it)"""
    import torch
    fn = {'tanh': torch.tanh, 'sigmoid': torch.sigmoid, 'relu': torch.relu, 'linear': lambda v: v,
          'hard_sigmoid': lambda v: torch.clamp(0.2 * v + 0.5, 0, 1)}
    a, ra = fn[activation], fn[recurrent_activation]
    B, T, u = x.shape[0], x.shape[1], U.shape[0]
    h = torch.zeros((B, u), dtype=x.dtype) if h0 is None else h0
    c = torch.zeros((B, u), dtype=x.dtype) if c0 is None else c0
    zx = x @ W
    hs = []
    for s in range(T):
        z = h @ U + zx[:, T - 1 - s if go_backwards else s] + b
        i, f, g, o = ra(z[:, :u]), ra(z[:, u:2 * u]), a(z[:, 2 * u:3 * u]), ra(z[:, 3 * u:])
        c = f * c + i * g
        h = o * a(c)
        hs.append(h)
    return torch.stack(hs, 1) if return_sequences else h
