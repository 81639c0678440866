"""The definition of keras.layers.GRU (keras 2.2.4 layers/recurrent.py, GRUCell), both reset_after forms, in numpy: a forward and a hand-written
backward through time.  Run in fp64 it is the reference of tests/test_gru_cpu.py (checked there against torch.nn.GRU and torch autograd) and
tests/test_gru_gpu.py; run in fp32 (dtype=np.float32) it is the "restatement" whose own distance to fp64 is the yardstick of the sequence tests.

Gate column order z, r, h in kernel W (Cin, 3u), recurrent_kernel U (u, 3u), bias b (3u) and, under reset_after, the recurrent bias rb (3u):
    a_t = x_t W + b
    reset_after=False:  m = h_{t-1} U[:, :2u];  z = ra(a_z + m_z), r = ra(a_r + m_r);  hh = act(a_h + (r h_{t-1}) U_h)
    reset_after=True:   m = h_{t-1} U + rb;     z = ra(a_z + m_z), r = ra(a_r + m_r);  q = m_h, hh = act(a_h + r q)
    h_t = z h_{t-1} + (1 - z) hh
Everything indexed by the PROCESSING step s: under go_backwards step s reads x[:, T-1-s]; `at_input_time` turns a (B, T, .) array around.
The shape table and the seed rule of the GPU sequence test live here too, so that the CPU suite can hold them to their promises."""
import numpy as np

from lstm_ref import ACTIVATIONS, RECURRENT_ACTIVATIONS, act, act_grad, at_input_time  # noqa: F401


def recurrence(zx, U, b, rb=None, h0=None, activation='tanh', recurrent_activation='hard_sigmoid', reset_after=False, go_backwards=False,
               dtype=np.float64):
    """zx (B, T, 3u) = X W at the input time index.  -> cache, all in processing order: h, aux, h_prev (B, T, u); pre (the three pre-activations)
    and gates = z, r, hh (B, T, 3u).  aux is r h_{t-1} (reset_after=False) or q (reset_after=True)."""
    zx, U, b = np.asarray(zx, dtype), np.asarray(U, dtype), np.asarray(b, dtype)
    assert (rb is not None) == bool(reset_after)
    rb = None if rb is None else np.asarray(rb, dtype)
    B, T, u = zx.shape[0], zx.shape[1], U.shape[0]
    h = np.zeros((B, u), dtype) if h0 is None else np.asarray(h0, dtype)
    k = dict(h0=h, U=U, b=b, rb=rb, activation=activation, recurrent_activation=recurrent_activation, reset_after=bool(reset_after),
             go_backwards=go_backwards, h=np.zeros((B, T, u), dtype), aux=np.zeros((B, T, u), dtype), h_prev=np.zeros((B, T, u), dtype),
             pre=np.zeros((B, T, 3 * u), dtype), gates=np.zeros((B, T, 3 * u), dtype))
    one = dtype(1)
    for s in range(T):
        a = zx[:, T - 1 - s if go_backwards else s] + b
        if reset_after:
            m = h @ U + rb
            pzr = m[:, :2 * u] + a[:, :2 * u]
        else:
            pzr = h @ U[:, :2 * u] + a[:, :2 * u]
        z, r = act(recurrent_activation, pzr[:, :u]), act(recurrent_activation, pzr[:, u:])
        if reset_after:
            aux = m[:, 2 * u:]
            ph = a[:, 2 * u:] + r * aux
        else:
            aux = r * h
            ph = aux @ U[:, 2 * u:] + a[:, 2 * u:]
        hh = act(activation, ph)
        k['h_prev'][:, s], k['aux'][:, s], k['pre'][:, s], k['gates'][:, s] = h, aux, np.concatenate([pzr, ph], 1), np.concatenate([z, r, hh], 1)
        h = z * h + (one - z) * hh
        k['h'][:, s] = h
    return k


def recurrence_backward(k, dy):
    """dy (B, T, u) in processing order, or (B, u) for the last step.  -> dz = da_z, da_r, da_h and (reset_after) dzr = da_z, da_r, dq, both
    (B, T, 3u) in processing order; dh0, dU, db, drb"""
    U, an, rn, ra = k['U'], k['activation'], k['recurrent_activation'], k['reset_after']
    B, T, u = k['h'].shape
    dt = U.dtype
    one = dt.type(1)
    dy = np.asarray(dy, dt)
    dh = np.zeros((B, u), dt)
    dz, dzr = np.zeros((B, T, 3 * u), dt), np.zeros((B, T, 3 * u), dt)
    dU = np.zeros_like(U)
    for s in range(T - 1, -1, -1):
        pre, gt, hp, aux = k['pre'][:, s], k['gates'][:, s], k['h_prev'][:, s], k['aux'][:, s]
        z, r, hh = (gt[:, q * u:(q + 1) * u] for q in range(3))
        dhv = (dy[:, s] if dy.ndim == 3 else (dy if s == T - 1 else 0)) + dh
        da_z = (dhv * (hp - hh)) * act_grad(rn, pre[:, :u], z)
        da_h = (dhv * (one - z)) * act_grad(an, pre[:, 2 * u:], hh)
        if ra:
            da_r = (da_h * aux) * act_grad(rn, pre[:, u:2 * u], r)
            dzr[:, s] = np.concatenate([da_z, da_r, da_h * r], 1)
            dh = dhv * z + dzr[:, s] @ U.T
            dU += hp.T @ dzr[:, s]
        else:
            drh = da_h @ U[:, 2 * u:].T
            da_r = (drh * hp) * act_grad(rn, pre[:, u:2 * u], r)
            dzr_s = np.concatenate([da_z, da_r], 1)
            dh = (dhv * z + drh * r) + dzr_s @ U[:, :2 * u].T
            dU[:, :2 * u] += hp.T @ dzr_s
            dU[:, 2 * u:] += aux.T @ da_h
        dz[:, s] = np.concatenate([da_z, da_r, da_h], 1)
    return dict(dz=dz, dzr=dzr if ra else None, dh0=dh, dU=dU, db=dz.sum((0, 1)), drb=dzr.sum((0, 1)) if ra else None)


def forward(x, W, U, b, rb=None, h0=None, activation='tanh', recurrent_activation='hard_sigmoid', reset_after=False, return_sequences=False,
            go_backwards=False, dtype=np.float64):
    """The layer: x (B, T, Cin) -> (y, cache); y (B, T, u) in processing order, or (B, u)"""
    x, W = np.asarray(x, dtype), np.asarray(W, dtype)
    k = recurrence(x @ W, U, b, rb, h0, activation, recurrent_activation, reset_after, go_backwards, dtype)
    k.update(x=x, W=W, return_sequences=return_sequences)
    return (k['h'] if return_sequences else k['h'][:, -1]), k


def backward(k, dy):
    """-> dx, dW, dU, db, drb, dh0 for the gradient dy of forward's y"""
    r = recurrence_backward(k, dy)
    dz_t = at_input_time(r['dz'], k['go_backwards'])
    return dict(dx=dz_t @ k['W'].T, dW=np.einsum('btc,btv->cv', k['x'], dz_t), dU=r['dU'], db=r['db'], drb=r['drb'], dh0=r['dh0'])


def torch_forward(x, W, U, b, rb=None, h0=None, activation='tanh', recurrent_activation='hard_sigmoid', reset_after=False, return_sequences=False,
                  go_backwards=False):
    """The same recurrence on torch tensors (any dtype; autograd runs through it)"""
    import torch
    fn = {'tanh': torch.tanh, 'sigmoid': torch.sigmoid, 'relu': torch.relu, 'linear': lambda v: v,
          'hard_sigmoid': lambda v: torch.clamp(0.2 * v + 0.5, 0, 1)}
    f, ra = fn[activation], fn[recurrent_activation]
    B, T, u = x.shape[0], x.shape[1], U.shape[0]
    h = torch.zeros((B, u), dtype=x.dtype) if h0 is None else h0
    zx = x @ W
    hs = []
    for s in range(T):
        a = zx[:, T - 1 - s if go_backwards else s] + b
        if reset_after:
            m = h @ U + rb
            z, r = ra(a[:, :u] + m[:, :u]), ra(a[:, u:2 * u] + m[:, u:2 * u])
            hh = f(a[:, 2 * u:] + r * m[:, 2 * u:])
        else:
            m = h @ U[:, :2 * u]
            z, r = ra(a[:, :u] + m[:, :u]), ra(a[:, u:2 * u] + m[:, u:])
            hh = f(a[:, 2 * u:] + (r * h) @ U[:, 2 * u:])
        h = z * h + (1 - z) * hh
        hs.append(h)
    return torch.stack(hs, 1) if return_sequences else h


# ---------------------------------------------------------------------------------------------------------------------
# the shape table of tests/test_gru_gpu.py and the seed rule of its sequence test
# ---------------------------------------------------------------------------------------------------------------------
# (B, T, Cin, u): the 24 shapes of tests/test_lstm_gpu.py with u moved to the GRU geometry's own edges (csrc/gru_geom.h): U is held in LDS up to
# u = 104 and streamed from 105, in the forward and in the backward alike; 100: KP = 104 beside UP = 112; 112: the first u whose KP is 112
SHAPES = [(1, 1, 1, 1), (2, 2, 3, 3), (15, 3, 16, 4), (16, 17, 17, 15), (17, 1, 1, 16), (33, 2, 3, 17), (1, 3, 16, 31), (2, 17, 17, 32),
          (15, 1, 3, 33), (16, 2, 1, 64), (17, 3, 17, 104), (33, 1, 16, 105), (1, 2, 16, 104), (2, 3, 1, 105), (15, 2, 3, 112), (16, 1, 17, 130),
          (2, 2, 16, 260), (2, 3, 3, 512), (1, 17, 1, 64), (2, 1, 17, 100), (17, 2, 3, 130), (33, 17, 16, 4), (17, 1, 1, 512), (15, 2, 1, 33)]
IDS = ['b%d-t%d-c%d-u%d' % s for s in SHAPES]

FAMILY_PAIRS = {'keras': [(a, r) for a in ACTIVATIONS for r in RECURRENT_ACTIVATIONS],
                'saturating': [('tanh', 'hard_sigmoid'), ('sigmoid', 'hard_sigmoid'), ('tanh', 'sigmoid'), ('tanh', 'hard_sigmoid')]}


def draw_family(family, rng, B, T, Cin, u, reset_after):
    """-> x, W, U, b, rb (None without reset_after).  'keras': keras' own initialisation, Glorot kernel and orthogonal blocks; its zero biases are
    moved by 0.1 N(0, 1) so that the two bias rows of reset_after are told apart.  'saturating': x ~ 2 N(0, 1), W ~ 1.5 U(-1, 1),
    U ~ (3 / sqrt(u)) U(-1, 1), b, rb ~ U(-1, 1)."""
    from gennet_amd import engine
    from gennet_amd.recurrent import orthogonal_blocks
    f32 = lambda a: a.astype(np.float32)          # noqa: E731
    if family == 'keras':
        engine.set_init_seed(int(rng.randint(1 << 30)))
        x, W, U = f32(rng.randn(B, T, Cin)), engine.glorot_uniform((Cin, 3 * u)), orthogonal_blocks(u, 3)
        b, rb = f32(0.1 * rng.randn(3 * u)), f32(0.1 * rng.randn(3 * u))
    else:
        x, W, U = f32(2 * rng.randn(B, T, Cin)), f32(1.5 * (rng.rand(Cin, 3 * u) * 2 - 1)), f32(3 / np.sqrt(u) * (rng.rand(u, 3 * u) * 2 - 1))
        b, rb = f32(rng.rand(3 * u) * 2 - 1), f32(rng.rand(3 * u) * 2 - 1)
    return x, W, U, b, (rb if reset_after else None)


def kink_margin(k):
    """the smallest distance of a pre-activation to a point where an activation's derivative jumps: +-2.5 for a hard_sigmoid z or r, 0 for a relu
    candidate"""
    u = k['h'].shape[2]
    m = np.inf
    if k['recurrent_activation'] == 'hard_sigmoid':
        m = min(m, float(np.abs(np.abs(k['pre'][:, :, :2 * u]) - 2.5).min()))
    if k['activation'] == 'relu':
        m = min(m, float(np.abs(k['pre'][:, :, 2 * u:]).min()))
    return m


def sequence_case(shape, family, reset_after):
    """The case of the sequence test for SHAPES[n]: its activations, direction and dy form by n, and the first seed of 0 .. 31 whose smallest distance
    to a derivative jump is at least 64 times the fp32 restatement's largest pre-activation error -- chosen from the reference alone.
    -> dict(seed, activation, recurrent_activation, reverse, seq, x, W, U, b, rb, dy, k64, k32), or None where no seed does."""
    B, T, Cin, u = shape
    n = SHAPES.index(shape)
    an, rn = FAMILY_PAIRS[family][n % len(FAMILY_PAIRS[family])]
    reverse, seq = bool(n & 1), bool(n & 2)
    for seed in range(32):
        rng = np.random.RandomState(seed * 100 + n)
        x, W, U, b, rb = draw_family(family, rng, B, T, Cin, u, reset_after)
        dy = rng.randn(*((B, T, u) if seq else (B, u))).astype(np.float32)
        _, k64 = forward(x, W, U, b, rb, None, an, rn, reset_after, seq, reverse)
        _, k32 = forward(x, W, U, b, rb, None, an, rn, reset_after, seq, reverse, dtype=np.float32)
        if kink_margin(k64) >= 64 * float(np.abs(k32['pre'] - k64['pre']).max()):
            return dict(seed=seed, activation=an, recurrent_activation=rn, reverse=reverse, seq=seq, x=x, W=W, U=U, b=b, rb=rb, dy=dy, k64=k64, k32=k32)
    return None
