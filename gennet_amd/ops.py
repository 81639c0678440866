"""Thin tensor-level wrappers over the C ABI: torch supplies device memory and the current HIP stream, nothing else.

Every function takes / returns contiguous fp32 CUDA tensors in Keras channels-last layout and launches on
torch's current stream.  No function here computes anything itself.
"""
import ctypes
import functools

import torch

from . import _lib

ACT = _lib.enum_members('GN_ACT_')                              # enum gn_act ...
ACT[None] = ACT['linear']                                       # ... and Keras' activation=None

_ws = {}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _chk(*ts):
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise _lib.GennetHipError('gennet_amd ops need CUDA (HIP) tensors; got a %s tensor -- there is no CPU path' % t.device)
        if not t.is_contiguous():
            raise ValueError('non-contiguous tensor passed to a gennet_amd op')


_ws_on_use = None       # engine.StepGraph.capture installs a callback here: a captured graph keeps the RAW ADDRESS of the scratch buffer it
                        # was handed, so it must also keep the buffer alive after a larger request has replaced it in _ws


def workspace(nbytes, device):
    """Stream-ordered scratch, grown on demand and reused (all ops run on one stream per process)."""
    key = (device.type, device.index)
    buf = _ws.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(int(nbytes * 1.25) + 1024, dtype=torch.uint8, device=device)
        _ws[key] = buf
    if _ws_on_use is not None:
        _ws_on_use(buf)
    return buf


def same_pad(L, k, s):
    """TF 'SAME': out = ceil(L/s); pad_total = max((out-1)*s + k - L, 0); left = total // 2."""
    out = -(-L // s)
    tot = max((out - 1) * s + k - L, 0)
    return out, tot // 2


def conv_geometry(L, k, stride, padding, dilation=1):
    """(Lout, pad_left) of a k-tap conv with taps `dilation` rows apart: the geometry of its effective kernel (k - 1) * dilation + 1.
    'causal' (Keras: pad (k - 1) * dilation rows on the left, then 'valid'): Lout = ceil(L / stride).  Host only."""
    ke = (k - 1) * dilation + 1
    if padding == 'same':
        return same_pad(L, ke, stride)
    if padding == 'valid':
        return (L - ke) // stride + 1, 0
    if padding == 'causal':
        return -(-L // stride), ke - 1
    raise ValueError('padding %r' % (padding,))


def pool_geometry(n, p, s, padding):
    """(n_out, pad_before) of a pooling window p with stride s over n cells, Keras 2.2.4 on TensorFlow.  'valid': (n - p) // s + 1, the cells
    behind the last full window are dropped (n < p: ValueError).  'same': ceil(n / s), the total pad max((n_out - 1) s + p - n, 0) with its
    floor half in front, so the odd cell goes at the end (n < p included: the one window is clipped to the n cells).  Host only."""
    n, p, s = int(n), int(p), int(s)
    if n < 1 or p < 1 or s < 1:
        raise ValueError('pooling %d cells with pool_size %d, strides %d' % (n, p, s))
    if padding == 'same':
        return same_pad(n, p, s)
    if padding == 'valid':
        if n < p:
            raise ValueError("pool_size %d on %d cells with padding 'valid': no full window" % (p, n))
        return (n - p) // s + 1, 0
    raise ValueError('padding %r' % (padding,))


# ---------------------------------------------------------------------------------------------- conv / dense
def conv_needs_any(Cin, Cout):
    """True when the strict forward and weight gradient refuse this channel pair (gn_conv1d_needs_any): only conv1d_fwd / conv1d_wgrad with
    any_channels=True run it, on the `anyc` kernels (csrc/conv_anyc.hip), and no fused variant does.  A data gradient runs the swapped pair:
    conv1d_dgrad of a (Cin, Cout) layer needs any_channels=True when conv_needs_any(Cout, Cin)."""
    return _lib.predicate('gn_conv1d_needs_any', int(Cin), int(Cout))


def conv_layer_needs_any(Cin, Cout):
    """A (Cin, Cout) layer in any of its three directions: the pair, or the swapped pair its data gradient runs (3 -> 4: only the latter)."""
    return conv_needs_any(Cin, Cout) or conv_needs_any(Cout, Cin)


def conv1d_fwd(x, w, b, stride, pad_left, Lout, act='linear', act_param=0.0, any_channels=False):
    """any_channels=True: gn_conv1d_fwd_any -- the same kernels with the same bits wherever the strict entry runs, plus the pairs it refuses."""
    _chk(x, w, b)
    B, L, Cin = x.shape
    k, _, Cout = w.shape
    y = torch.empty((B, Lout, Cout), dtype=torch.float32, device=x.device)
    _lib.call('gn_conv1d_fwd_any' if any_channels else 'gn_conv1d_fwd', _p(x), _p(w), _p(b), _p(y), B, L, Cin, Cout, k, stride, pad_left, Lout, ACT[act], float(act_param), _stream())
    return y


def conv1d_fwd_stats(x, w, b, stride, pad_left, Lout):
    """Linear conv forward + the BatchNorm statistics of its output: (y, sums fp64 (2*Cout,) = [sum y | sum y^2]); the sums come out of
    the conv kernel's epilogue where the pipelined kernel runs, from a separate pass otherwise (same values either way)."""
    _chk(x, w, b)
    B, L, Cin = x.shape
    k, _, Cout = w.shape
    y = torch.empty((B, Lout, Cout), dtype=torch.float32, device=x.device)
    sums = torch.empty((2 * Cout,), dtype=torch.float64, device=x.device)
    nb = _lib.size('gn_conv1d_fwd_stats_workspace', B, Lout, Cout)
    ws = workspace(nb, x.device)
    _lib.call('gn_conv1d_fwd_stats', _p(x), _p(w), _p(b), _p(y), _p(sums), _p(ws), ws.numel(), B, L, Cin, Cout, k, stride, pad_left, Lout, _stream())
    return y, sums


_BF16X3_WS = {}


def conv1d_fwd_bf16x3(x, w, b, stride, pad_left, Lout, act='linear', act_param=0.0, resplit=True):
    """EXPERIMENTAL opt-in: conv1d_fwd on the bf16 matrix cores with 3-way split fp32 operands (csrc/conv_bf16x3.hip)."""
    _chk(x, w, b)
    B, L, Cin = x.shape
    k, _, Cout = w.shape
    n = _lib.size('gn_conv1d_bf16x3_workspace', B, L, Cin, Cout, k)
    key = (x.device, n)
    ws = _BF16X3_WS.get(key)
    if ws is None:
        ws = _BF16X3_WS[key] = torch.empty(n, dtype=torch.uint8, device=x.device)
    y = torch.empty((B, Lout, Cout), dtype=torch.float32, device=x.device)
    _lib.call('gn_conv1d_fwd_bf16x3', _p(x), _p(w), _p(b), _p(y), _p(ws), n, B, L, Cin, Cout, k, stride, pad_left, Lout, ACT[act], float(act_param),
              1 if resplit else 0, _stream())
    return y


def conv1d_fwd_wino(x, w, b, pad_left, Lout, act='linear', act_param=0.0):
    """conv1d_fwd of a unit-stride 5-tap layer through the transform-domain kernel directly (csrc/conv_wino.hip; tests and layer benchmarks)."""
    _chk(x, w, b)
    B, L, Cin = x.shape
    k, _, Cout = w.shape
    n = _lib.size('gn_conv1d_wino_workspace', Cin, Cout)
    ws = workspace(n, x.device)
    y = torch.empty((B, Lout, Cout), dtype=torch.float32, device=x.device)
    _lib.call('gn_conv1d_fwd_wino', _p(x), _p(w), _p(b), _p(y), _p(ws), ws.numel(), B, L, Cin, Cout, k, 1, pad_left, Lout, ACT[act], float(act_param), _stream())
    return y


def conv1d_fwd_dropout(x, w, b, mask, stride, pad_left, Lout, act, act_param, rate):
    """conv + activation + inverted dropout in one epilogue; mask: uint8 keep-mask with the shape of the output."""
    _chk(x, w, b, mask)
    B, L, Cin = x.shape
    k, _, Cout = w.shape
    y = torch.empty((B, Lout, Cout), dtype=torch.float32, device=x.device)
    assert mask.numel() == y.numel()
    _lib.call('gn_conv1d_fwd_dropout', _p(x), _p(w), _p(b), _p(mask), _p(y), B, L, Cin, Cout, k, stride, pad_left, Lout, ACT[act], float(act_param),
              float(rate), _stream())
    return y


def act_dropout_bwd(dy, y, mask, act, act_param, rate, inplace=False):
    _chk(dy, y, mask)
    dx = dy if inplace else torch.empty_like(dy)
    _lib.call('gn_act_dropout_bwd', _p(dy), _p(y), _p(mask), _p(dx), dy.numel(), ACT[act], float(act_param), float(rate), _stream())
    return dx


def conv1d_transpose_w(w):
    _chk(w)
    k, Cin, Cout = w.shape
    wt = torch.empty((k, Cout, Cin), dtype=torch.float32, device=w.device)
    _lib.call('gn_conv1d_transpose_w', _p(w), _p(wt), k, Cin, Cout, _stream())
    return wt


def conv1d_dgrad(dy, wt, L, stride, pad_left, prev=None, any_channels=False):
    """prev = (y_prev, act, act_param, mask_prev, rate): fuse the producer layer's activation/dropout backward into the epilogue.
    any_channels=True: gn_conv1d_dgrad_any (no fused form: prev must be None)."""
    _chk(dy, wt)
    B, Lout, Cout = dy.shape
    k, _, Cin = wt.shape
    if any_channels and prev is not None:
        raise ValueError('conv1d_dgrad(any_channels=True) has no fused producer gradient')
    dx = torch.empty((B, L, Cin), dtype=torch.float32, device=dy.device)
    if prev is None:
        _lib.call('gn_conv1d_dgrad_any' if any_channels else 'gn_conv1d_dgrad', _p(dy), _p(wt), _p(dx), B, L, Cin, Cout, k, stride, pad_left, Lout, _stream())
    else:
        y_prev, act, param, mask, rate = prev
        _chk(y_prev, mask)
        assert y_prev.numel() == dx.numel()
        _lib.call('gn_conv1d_dgrad_fused', _p(dy), _p(wt), _p(dx), B, L, Cin, Cout, k, stride, pad_left, Lout, _p(y_prev), _p(mask), ACT[act], float(param),
                  float(rate), _stream())
    return dx


def can_fuse_dgrad(Cin, Cout):
    return Cin > 4 and Cout > 4 and not conv_needs_any(Cin, Cout)


def conv1d_wgrad(x, dy, k, stride, pad_left, dw=None, db=None, want_db=True, any_channels=False):
    """want_db=False: no bias gradient at all (db stays None; the kernels are handed NULL and skip the column sum of dy).
    any_channels=True: gn_conv1d_wgrad_any."""
    _chk(x, dy, dw, db)
    B, L, Cin = x.shape
    _, Lout, Cout = dy.shape
    if dw is None:
        dw = torch.empty((k, Cin, Cout), dtype=torch.float32, device=x.device)
    if db is None and want_db:
        db = torch.empty((Cout,), dtype=torch.float32, device=x.device)
    nb = _lib.size('gn_conv1d_wgrad_workspace', B, L, Cin, Cout, k, stride, Lout)
    ws = workspace(nb, x.device)
    _lib.call('gn_conv1d_wgrad_any' if any_channels else 'gn_conv1d_wgrad', _p(x), _p(dy), _p(dw), _p(db), _p(ws), ws.numel(), B, L, Cin, Cout, k, stride, pad_left, Lout, _stream())
    return dw, db


def bias_act_dropout(y, b, act='linear', act_param=0.0, mask=None, rate=0.0, gen=None):
    """In place: y = act(y + b) over the last axis, any channel count (csrc/conv_transpose.hip); with mask, inverted dropout after it.
    gen = (seed, offset): the keep-mask is drawn into `mask` in the same pass (gn_dropout_mask's draw); otherwise `mask` is read."""
    _chk(y, b, mask)
    C = y.shape[-1]
    if mask is not None:
        assert mask.numel() == y.numel()
    seed, off = gen if gen is not None else (0, 0)
    _lib.call('gn_bias_act_dropout', _p(y), _p(b), _p(mask), y.numel() // C, C, ACT[act], float(act_param), float(rate), 1 if gen is not None else 0,
              int(seed), int(off), _stream())
    return y


def bias_grad(dy2d, db=None):
    """db[c] = sum over rows of dy2d[row, c] (the bias-gradient reduction of dense_bwd / conv1d_wgrad), any column count."""
    _chk(dy2d, db)
    rows, C = dy2d.shape
    if db is None:
        db = torch.empty((C,), dtype=torch.float32, device=dy2d.device)
    ws = workspace(_lib.size('gn_bias_grad_workspace', rows, C), dy2d.device)
    _lib.call('gn_bias_grad', _p(dy2d), _p(db), _p(ws), ws.numel(), rows, C, _stream())
    return db


def conv2d_w2_fold(w, b):
    _chk(w, b)
    kh, kw, Cin, Cout = w.shape
    assert kw == 5
    wf = torch.empty((kh, 2 * Cin, 2 * Cout), dtype=torch.float32, device=w.device)
    bf = torch.empty((2 * Cout,), dtype=torch.float32, device=w.device)
    _lib.call('gn_conv2d_w2_fold', _p(w), _p(b), _p(wf), _p(bf), kh, Cin, Cout, _stream())
    return wf, bf


def conv2d_w2_unfold_grad(dwf, dbf, Cin, Cout, dw=None, db=None):
    _chk(dwf, dbf, dw, db)
    kh = dwf.shape[0]
    if dw is None:
        dw = torch.empty((kh, 5, Cin, Cout), dtype=torch.float32, device=dwf.device)
    if db is None:
        db = torch.empty((Cout,), dtype=torch.float32, device=dwf.device)
    _lib.call('gn_conv2d_w2_unfold_grad', _p(dwf), _p(dbf), _p(dw), _p(db), kh, Cin, Cout, _stream())
    return dw, db


def maxpool_h2_fwd(x):
    """MaxPooling2D(pool_size=(2,1)) on (B, H, ...): gn_maxpool_h2_fwd."""
    _chk(x)
    B, H = x.shape[0], x.shape[1]
    R = x.numel() // max(B * H, 1)
    y = torch.empty((B, H // 2) + tuple(x.shape[2:]), dtype=torch.float32, device=x.device)
    _lib.call('gn_maxpool_h2_fwd', _p(x), _p(y), B, H, R, _stream())
    return y


def maxpool_h2_bwd(dy, x):
    _chk(dy, x)
    B, H = x.shape[0], x.shape[1]
    R = x.numel() // max(B * H, 1)
    dx = torch.empty_like(x)
    _lib.call('gn_maxpool_h2_bwd', _p(dy), _p(x), _p(dx), B, H, R, _stream())
    return dx


# ---------------------------------------------------------------------------------------------- pooling (csrc/pooling.hip)
POOL_MODES = _lib.enum_members('GN_POOL_')                      # enum gn_pool: {'max': 0, 'avg': 1}


def _pool_args(x_shape, pool, strides, padding):
    """(B, H, W, C) and the geometry gn_pool2d_* take after it: ph, pw, sh, sw, pad_top, pad_left, Ho, Wo"""
    B, H, W, C = (int(v) for v in x_shape)
    (Ho, pt), (Wo, pl) = pool_geometry(H, pool[0], strides[0], padding), pool_geometry(W, pool[1], strides[1], padding)
    return B, H, W, C, int(pool[0]), int(pool[1]), int(strides[0]), int(strides[1]), pt, pl, Ho, Wo


def pool2d_fwd(mode, x, pool, strides, padding, out=None):
    """x (B, H, W, C) -> (B, Ho, Wo, C): the maximum or the average ('max' | 'avg') over pool[0] x pool[1] windows, Keras 2.2.4 on TensorFlow."""
    _chk(x, out)
    B, H, W, C, ph, pw, sh, sw, pt, pl, Ho, Wo = _pool_args(x.shape, pool, strides, padding)
    y = torch.empty((B, Ho, Wo, C), dtype=torch.float32, device=x.device) if out is None else out
    assert tuple(y.shape) == (B, Ho, Wo, C)
    _lib.call('gn_pool2d_fwd', POOL_MODES[mode], _p(x), _p(y), B, H, W, C, ph, pw, sh, sw, pt, pl, Ho, Wo, _stream())
    return y


def pool2d_bwd(mode, dy, x, x_shape, pool, strides, padding, out=None):
    """dx (x_shape) of pool2d_fwd; x may be None for 'avg' (the tape keeps only the shape)."""
    _chk(dy, x, out)
    B, H, W, C, ph, pw, sh, sw, pt, pl, Ho, Wo = _pool_args(x_shape, pool, strides, padding)
    assert tuple(dy.shape) == (B, Ho, Wo, C) and (x is None or tuple(x.shape) == (B, H, W, C))
    dx = torch.empty((B, H, W, C), dtype=torch.float32, device=dy.device) if out is None else out
    _lib.call('gn_pool2d_bwd', POOL_MODES[mode], _p(dy), _p(x), _p(dx), B, H, W, C, ph, pw, sh, sw, pt, pl, Ho, Wo, _stream())
    return dx


def _global_pool_ws(B, P, C, device):
    return workspace(_lib.size('gn_global_pool_workspace', B, P, C), device)           # 16-byte aligned, as every torch allocation is


def global_pool_fwd(mode, x, out=None):
    """x (B, P, C) -> (B, C): the mean or the maximum over P."""
    _chk(x, out)
    B, P, C = (int(v) for v in x.shape)
    y = torch.empty((B, C), dtype=torch.float32, device=x.device) if out is None else out
    ws = _global_pool_ws(B, P, C, x.device)
    _lib.call('gn_global_pool_fwd', POOL_MODES[mode], _p(x), _p(y), _p(ws), ws.numel(), B, P, C, _stream())
    return y


def global_pool_bwd(mode, dy, x, y, x_shape, out=None):
    """dx (x_shape = (B, P, C)); 'avg': dy / P, x and y may be None; 'max': dy / n_ties wherever x equals the maximum y."""
    _chk(dy, x, y, out)
    B, P, C = (int(v) for v in x_shape)
    dx = torch.empty((B, P, C), dtype=torch.float32, device=dy.device) if out is None else out
    ws = _global_pool_ws(B, P, C, dy.device)
    _lib.call('gn_global_pool_bwd', POOL_MODES[mode], _p(dy), _p(x), _p(y), _p(dx), _p(ws), ws.numel(), B, P, C, _stream())
    return dx


@functools.lru_cache(maxsize=None)
def tap_groups(k):
    """(G, h): a k-tap Conv1D (k > 5) runs as G = ceil(k/5) tap groups of h = ceil(k/G) taps; gn_conv1d_tap_groups (csrc/tap_fold.hip) owns the
    rule, asked once per k (a host-only call: nothing is launched)."""
    G, h = ctypes.c_int(), ctypes.c_int()
    _lib.call('gn_conv1d_tap_groups', k, ctypes.byref(G), ctypes.byref(h))
    return G.value, h.value


def conv1d_tapfold_x(x, k, pl):
    """More than 5 taps as h taps over G*Cin channels (csrc/tap_fold.hip): the input with its shifted copies beside it, left padding materialised."""
    _chk(x)
    B, L, Cin = x.shape
    x2 = torch.empty((B, L + pl, tap_groups(k)[0] * Cin), dtype=torch.float32, device=x.device)
    _lib.call('gn_conv1d_tapfold_x', _p(x), _p(x2), B, L, Cin, k, pl, _stream())
    return x2


def conv1d_tapunfold_dx(dx2, L, k, pl):
    _chk(dx2)
    B, L2, C2 = dx2.shape
    G = tap_groups(k)[0]
    assert L2 == L + pl and C2 % G == 0
    dx = torch.empty((B, L, C2 // G), dtype=torch.float32, device=dx2.device)
    _lib.call('gn_conv1d_tapunfold_dx', _p(dx2), _p(dx), B, L, C2 // G, k, pl, _stream())
    return dx


def conv1d_tapfold_w(w):
    _chk(w)
    k, Cin, Cout = w.shape
    G, h = tap_groups(k)
    w2 = torch.empty((h, G * Cin, Cout), dtype=torch.float32, device=w.device)
    _lib.call('gn_conv1d_tapfold_w', _p(w), _p(w2), k, Cin, Cout, _stream())
    return w2


def conv1d_tapunfold_dw(dw2, k, dw=None):
    _chk(dw2, dw)
    h, C2, Cout = dw2.shape
    G, hh = tap_groups(k)
    assert h == hh and C2 % G == 0
    if dw is None:
        dw = torch.empty((k, C2 // G, Cout), dtype=torch.float32, device=dw2.device)
    _lib.call('gn_conv1d_tapunfold_dw', _p(dw2), _p(dw), k, C2 // G, Cout, _stream())
    return dw


def conv1d_up2_fold(w, b, stride):
    """UpSampling1D(2) -> Conv1D(5, 'same', stride) as a 3-tap stride-1 conv on the un-upsampled input (gn_conv1d_up2_fold)."""
    _chk(w, b)
    k, Cin, Cout = w.shape
    assert k == 5 and stride in (1, 2)
    Cf = Cout * (2 if stride == 1 else 1)
    wf = torch.empty((3, Cin, Cf), dtype=torch.float32, device=w.device)
    bf = torch.empty((Cf,), dtype=torch.float32, device=w.device)
    _lib.call('gn_conv1d_up2_fold', _p(w), _p(b), _p(wf), _p(bf), Cin, Cout, stride, _stream())
    return wf, bf


def conv1d_up2_unfold_grad(dwf, dbf, Cout, stride, dw=None, db=None):
    _chk(dwf, dbf, dw, db)
    Cin = dwf.shape[1]
    assert dwf.shape[0] == 3 and dwf.shape[2] == Cout * (2 if stride == 1 else 1)
    if dw is None:
        dw = torch.empty((5, Cin, Cout), dtype=torch.float32, device=dwf.device)
    if db is None:
        db = torch.empty((Cout,), dtype=torch.float32, device=dwf.device)
    _lib.call('gn_conv1d_up2_unfold_grad', _p(dwf), _p(dbf), _p(dw), _p(db), Cin, Cout, stride, _stream())
    return dw, db


def dense_fwd(x, w, b, act='linear', act_param=0.0):
    _chk(x, w, b)
    B, n_in = x.shape
    n_out = w.shape[1]
    y = torch.empty((B, n_out), dtype=torch.float32, device=x.device)
    _lib.call('gn_dense_fwd', _p(x), _p(w), _p(b), _p(y), B, n_in, n_out, ACT[act], float(act_param), _stream())
    return y


def dense_bwd(x, w, dy, need_dx=True, dw=None, db=None, prev=None):
    _chk(x, w, dy, dw, db)
    B, n_in = x.shape
    n_out = w.shape[1]
    dx = torch.empty_like(x) if need_dx else None
    if prev is not None:
        _, act, param, mask, rate = prev
        assert need_dx and n_out <= 4
        if dw is None:
            dw = torch.empty_like(w)
        if db is None:
            db = torch.empty((n_out,), dtype=torch.float32, device=x.device)
        _lib.call('gn_dense_bwd_fused', _p(x), _p(w), _p(dy), _p(dx), _p(dw), _p(db), B, n_in, n_out, _p(mask), ACT[act], float(param), float(rate), _stream())
        return dx, dw, db
    if dw is None:
        dw = torch.empty_like(w)
    if db is None:
        db = torch.empty((n_out,), dtype=torch.float32, device=x.device)
    nb = _lib.size('gn_dense_bwd_workspace', B, n_in, n_out)
    ws = workspace(nb, x.device)
    _lib.call('gn_dense_bwd', _p(x), _p(w), _p(dy), _p(dx), _p(dw), _p(db), _p(ws), ws.numel(), B, n_in, n_out, _stream())
    return dx, dw, db


# ---------------------------------------------------------------------------------------------- elementwise
def act_fwd(x, act, act_param=0.0):
    _chk(x)
    y = torch.empty_like(x)
    _lib.call('gn_act_fwd', _p(x), _p(y), x.numel(), ACT[act], float(act_param), _stream())
    return y


def act_bwd(dy, y, act, act_param=0.0, inplace=False):
    _chk(dy, y)
    dx = dy if inplace else torch.empty_like(dy)
    _lib.call('gn_act_bwd', _p(dy), _p(y), _p(dx), dy.numel(), ACT[act], float(act_param), _stream())
    return dx


# ---------------------------------------------------------------------------------------------- softmax (csrc/softmax.hip)
def _softmax_view(t, view):
    outer, P, inner = (int(v) for v in view)
    if outer < 1 or P < 1 or inner < 1 or outer * P * inner != t.numel():
        raise ValueError('softmax: the (outer, P, inner) view %r does not cover a tensor of %d elements' % ((outer, P, inner), t.numel()))
    if P * inner >= 1 << 31:
        raise ValueError('softmax: P * inner = %d * %d does not fit the int parameters of the kernels (< 2^31)' % (P, inner))
    return outer, P, inner


def softmax_fwd(x, view, out=None, inplace=False):
    """y = softmax of x along the middle axis of its (outer, P, inner) view (element (o, p, i) at (o*P + p)*inner + i); the shape stays x's."""
    _chk(x, out)
    outer, P, inner = _softmax_view(x, view)
    y = x if inplace else torch.empty_like(x) if out is None else out
    _lib.call('gn_softmax_fwd', _p(x), _p(y), outer, P, inner, _stream())
    return y


def softmax_bwd(dy, y, view, out=None, inplace=False):
    """dx = y * (dy - sum_p dy * y) from the stored output y, on the same view"""
    _chk(dy, y, out)
    outer, P, inner = _softmax_view(dy, view)
    assert y.numel() == dy.numel()
    dx = dy if inplace else torch.empty_like(dy) if out is None else out
    _lib.call('gn_softmax_bwd', _p(dy), _p(y), _p(dx), outer, P, inner, _stream())
    return dx


# ---------------------------------------------------------------------------------------------- batched product, l2 normalisation (csrc/bmm.hip)
def bmm(a, b, trans_a=False, trans_b=False, out=None, valu=False):
    """c (batch, M, N) = A . B per batch entry over contiguous 3-D tensors: A = a (batch, M, K), or a^T of a (batch, K, M) under trans_a;
    B = b (batch, K, N), or b^T of b (batch, N, K) under trans_b.  Nothing is transposed in memory: the flags only choose the strides.
    valu=True runs gn_bmm_valu, the 16 x 16 VALU tile (the yardstick of scripts/bmm_microbench.py; the same bits)."""
    _chk(a, b, out)
    if a.dim() != 3 or b.dim() != 3 or a.dtype != torch.float32 or b.dtype != torch.float32 or a.shape[0] != b.shape[0]:
        raise ValueError('bmm: float32 tensors (batch, ., .) of one batch size are expected, got %r and %r' % (tuple(a.shape), tuple(b.shape)))
    batch = a.shape[0]
    K, M = (a.shape[1], a.shape[2]) if trans_a else (a.shape[2], a.shape[1])
    Kb, N = (b.shape[2], b.shape[1]) if trans_b else (b.shape[1], b.shape[2])
    if K != Kb:
        raise ValueError('bmm: the contracted extents differ, %d and %d (a %r%s, b %r%s)'
                         % (K, Kb, tuple(a.shape), '^T' if trans_a else '', tuple(b.shape), '^T' if trans_b else ''))
    c = torch.empty((batch, M, N), dtype=torch.float32, device=a.device) if out is None else out
    assert c.numel() == batch * M * N
    a_m, a_k = (1, M) if trans_a else (K, 1)
    b_k, b_n = (1, K) if trans_b else (N, 1)
    _lib.call('gn_bmm_valu' if valu else 'gn_bmm', _p(a), _p(b), _p(c), batch, M, N, K, M * K, a_m, a_k, K * N, b_k, b_n, _stream())
    return c


def _l2norm_view(t, view):
    outer, P, inner = (int(v) for v in view)
    if outer < 0 or P < 1 or inner < 1 or outer * P * inner != t.numel():
        raise ValueError('l2norm: the (outer, P, inner) view %r does not cover a tensor of %d elements' % ((outer, P, inner), t.numel()))
    return outer, P, inner


def l2norm_fwd(x, view):
    """(y, inv): y = x * inv along the middle axis of the (outer, P, inner) view, inv (outer, inner) = 1 / sqrt(max(sum_p x^2, 1e-12)) (tf.nn.l2_normalize)"""
    _chk(x)
    outer, P, inner = _l2norm_view(x, view)
    y = torch.empty_like(x)
    inv = torch.empty((outer, inner), dtype=torch.float32, device=x.device)
    _lib.call('gn_l2norm_fwd', _p(x), _p(y), _p(inv), outer, P, inner, _stream())
    return y, inv


def l2norm_bwd(dy, y, inv, view, out=None):
    """dx = inv * (dy - y * sum_p dy * y) from the stored y and inv; inv * dy where the sum of squares was clamped"""
    _chk(dy, y, inv, out)
    outer, P, inner = _l2norm_view(dy, view)
    assert y.numel() == dy.numel() and inv.numel() == outer * inner
    dx = torch.empty_like(dy) if out is None else out
    _lib.call('gn_l2norm_bwd', _p(dy), _p(y), _p(inv), _p(dx), outer, P, inner, _stream())
    return dx


# ---------------------------------------------------------------------------------------------- fused attention (csrc/attention.hip)
ATTENTION_BQ, ATTENTION_BK, ATTENTION_MAX_D = (_lib.CONSTS[_k] for _k in ('GN_ATTN_BQ', 'GN_ATTN_BK', 'GN_ATTN_MAX_D'))


def _attention_shape(what, q, k, v, scale):
    _chk(q, k, v, scale)
    if not (q.dim() == k.dim() == v.dim() == 3) or any(t.dtype != torch.float32 for t in (q, k, v)) or q.shape[0] != k.shape[0] or k.shape[:2] != v.shape[:2] \
            or q.shape[2] != k.shape[2]:
        raise ValueError('%s: float32 q (B, Tq, d), k (B, Tk, d), v (B, Tk, dv) are expected, got %r, %r, %r' % (what, tuple(q.shape), tuple(k.shape), tuple(v.shape)))
    if scale is not None and (scale.numel() != 1 or scale.dtype != torch.float32):
        raise ValueError('%s: scale is one float32 on the device, got %r' % (what, tuple(scale.shape)))
    return int(q.shape[0]), int(q.shape[1]), int(k.shape[1]), int(q.shape[2]), int(v.shape[2])


def attention_fwd(q, k, v, scale=None, causal=False, training=False, out=None):
    """-> (out, lse): out (B, Tq, dv) = softmax_j(scale * q . k^T) . v over q (B, Tq, d), k (B, Tk, d), v (B, Tk, dv) in one launch, no (Tq, Tk) tensor
    in memory; under `causal` over j <= i only.  scale: a one-element device tensor (read by the kernel, so a captured step replays with the
    updated weight) or None for 1.  lse (B, Tq) = row maximum + log(row sum) in the training phase, else None."""
    B, Tq, Tk, d, dv = _attention_shape('attention_fwd', q, k, v, scale)
    _chk(out)
    if out is None:
        out = torch.empty((B, Tq, dv), dtype=torch.float32, device=q.device)
    assert out.numel() == B * Tq * dv
    lse = torch.empty((B, Tq), dtype=torch.float32, device=q.device) if training else None
    _lib.call('gn_attention_fwd', _p(q), _p(k), _p(v), _p(scale), _p(out), _p(lse), B, Tq, Tk, d, dv, 1 if causal else 0, _stream())
    return out, lse


def attention_bwd(q, k, v, out, lse, dout, scale=None, causal=False, need=(True, True, True), need_dscale=False):
    """-> (dq, dk, dv, dscale_rows) from the forward's operands, out and lse and the gradient dout (B, Tq, dv): each of dq, dk, dv where `need` asks
    (else None), and with need_dscale the (B * Tq,) row partials of the gradient of scale, sum_j dS[i, j] (q_i . k_j), whose sum (ops.bias_grad over
    the (B * Tq, 1) view) is the gradient.  p is recomputed from lse tile by tile; no atomics."""
    B, Tq, Tk, d, dv = _attention_shape('attention_bwd', q, k, v, scale)
    _chk(out, lse, dout)
    if tuple(out.shape) != (B, Tq, dv) or dout.numel() != out.numel() or lse.numel() != B * Tq:
        raise ValueError('attention_bwd: out, dout (B, Tq, dv) and lse (B, Tq) are expected, got %r, %r, %r' % (tuple(out.shape), tuple(dout.shape), tuple(lse.shape)))
    dq = torch.empty_like(q) if need[0] else None
    dk = torch.empty_like(k) if need[1] else None
    dvv = torch.empty_like(v) if need[2] else None
    rows = torch.empty((B * Tq,), dtype=torch.float32, device=q.device) if need_dscale else None
    nbytes = _lib.size('gn_attention_workspace', B, Tq)
    ws = workspace(nbytes, q.device)
    _lib.call('gn_attention_bwd', _p(q), _p(k), _p(v), _p(scale), _p(out), _p(lse), _p(dout), _p(dq), _p(dk), _p(dvv), _p(rows), _p(ws), ws.numel(), B, Tq,
              Tk, d, dv, 1 if causal else 0, _stream())
    return dq, dk, dvv, rows


# ---------------------------------------------------------------------------------------------- layer normalisation (csrc/layernorm.hip)
LAYERNORM_ROWS_MAX_N, LAYERNORM_BLOCK_MAX_N, LAYERNORM_FWD_GRID_CAP, LAYERNORM_BWD_GRID_CAP, LAYERNORM_BWD_GRID_CAP_WIDE = (
    _lib.CONSTS[_k] for _k in ('GN_LN_ROWS_MAX_N', 'GN_LN_BLOCK_MAX_N', 'GN_LN_FWD_GRID_CAP', 'GN_LN_BWD_GRID_CAP', 'GN_LN_BWD_GRID_CAP_WIDE'))


def _layernorm_rows(what, x, N, *params):
    """rows of the (rows, N) view of x: its trailing axes hold N contiguous floats; every parameter vector has N"""
    if x.dtype != torch.float32 or N < 1 or x.numel() == 0 or x.numel() % N:
        raise ValueError('%s: a non-empty float32 tensor whose trailing axes hold N = %d values is expected, got %r' % (what, N, tuple(x.shape)))
    for p in params:
        if p is not None and (p.dtype != torch.float32 or p.numel() != N):
            raise ValueError('%s: a parameter or its gradient holds %d values, N = %d' % (what, p.numel(), N))
    return x.numel() // N


def layernorm_fwd(x, gamma, beta, N, eps, training=False, out=None):
    """-> (y, mean, rstd): y = (x - mean_r) * rstd_r * gamma + beta over the (rows, N) view of x (rows: every leading axis; N: the product of the
    normalised trailing axes), one launch, biased variance from the centred second pass.  gamma / beta: (N,) device tensors, None for
    scale=False / center=False.  mean and rstd (rows,) in the training phase, else None."""
    _chk(x, gamma, beta, out)
    rows = _layernorm_rows('layernorm_fwd', x, N, gamma, beta)
    y = torch.empty_like(x) if out is None else out
    assert y.numel() == x.numel()
    mean = torch.empty((rows,), dtype=torch.float32, device=x.device) if training else None
    rstd = torch.empty((rows,), dtype=torch.float32, device=x.device) if training else None
    _lib.call('gn_layernorm_fwd', _p(x), _p(gamma), _p(beta), _p(y), _p(mean), _p(rstd), rows, N, eps, _stream())
    return y, mean, rstd


def layernorm_bwd(dy, x, gamma, mean, rstd, N, need_dx=True, dgamma=None, dbeta=None, need_dgamma=False, need_dbeta=False):
    """-> (dx, dgamma, dbeta) from the forward's x, mean and rstd: dx where need_dx (else None); dgamma / dbeta (N,) into the tensors given, or
    into new ones where need_dgamma / need_dbeta, else None -- both None is a frozen layer: one launch, no partials.  One launch over the
    elements plus the fixed-order fp64 sum of the per-block partials; no atomics."""
    _chk(dy, x, gamma, mean, rstd, dgamma, dbeta)
    rows = _layernorm_rows('layernorm_bwd', x, N, gamma, dgamma, dbeta)
    if dy.numel() != x.numel() or dy.dtype != torch.float32 or mean.numel() != rows or rstd.numel() != rows:
        raise ValueError('layernorm_bwd: dy like x and mean, rstd of %d rows are expected, got %r, %r, %r' % (rows, tuple(dy.shape), tuple(mean.shape), tuple(rstd.shape)))
    dx = torch.empty_like(x) if need_dx else None
    if dgamma is None and need_dgamma:
        dgamma = torch.empty((N,), dtype=torch.float32, device=x.device)
    if dbeta is None and need_dbeta:
        dbeta = torch.empty((N,), dtype=torch.float32, device=x.device)
    ws = workspace(_lib.size('gn_layernorm_bwd_workspace', rows, N), x.device)
    _lib.call('gn_layernorm_bwd', _p(dy), _p(x), _p(gamma), _p(mean), _p(rstd), _p(dx), _p(dgamma), _p(dbeta), _p(ws), ws.numel(), rows, N, _stream())
    return dx, dgamma, dbeta


# ---------------------------------------------------------------------------------------------- LSTM recurrence (csrc/lstm.hip)
LSTM_ACT = _lib.enum_members('GN_LSTM_')                        # enum gn_lstm_act: {'tanh': 0, 'sigmoid': 1, 'relu': 2, 'linear': 3, 'hard_sigmoid': 4}


def _lstm_shape(what, zx, U):
    if zx.dim() != 3 or U.dim() != 2 or U.shape[1] != 4 * U.shape[0] or zx.shape[2] != U.shape[1] or zx.dtype != torch.float32 or U.dtype != torch.float32:
        raise ValueError('%s: float32 (B, T, 4u) beside a recurrent kernel (u, 4u) is expected, got %r and %r' % (what, tuple(zx.shape), tuple(U.shape)))
    return int(zx.shape[0]), int(zx.shape[1]), int(U.shape[0])


def lstm_fwd(zx, U, bias, h0=None, c0=None, activation='tanh', recurrent_activation='hard_sigmoid', reverse=False, training=False):
    """The LSTM recurrence over zx (B, T, 4u) = X . W (gate columns i, f, c, o): -> (h, gates, c, hprev).  h (B, T, u) is in processing order
    (under `reverse` step s reads zx[:, T-1-s]); in the training phase gates (B, T, 4u), c (B, T, u) and hprev (B, T, u), the h that entered each
    step, are stored at the input time index for lstm_bwd, else they are None.  h0 / c0 (B, u): None is zeros."""
    _chk(zx, U, bias, h0, c0)
    B, T, u = _lstm_shape('lstm_fwd', zx, U)
    assert bias.numel() == 4 * u and all(t is None or tuple(t.shape) == (B, u) for t in (h0, c0))
    h = torch.empty((B, T, u), dtype=torch.float32, device=zx.device)
    gates = c = hprev = None
    if training:
        gates = torch.empty((B, T, 4 * u), dtype=torch.float32, device=zx.device)
        c, hprev = torch.empty_like(h), torch.empty_like(h)
    ws = workspace(_lib.size('gn_lstm_fwd_workspace', u), zx.device)
    _lib.call('gn_lstm_fwd', _p(zx), _p(U), _p(bias), _p(h0), _p(c0), _p(h), _p(gates), _p(c), _p(hprev), _p(ws), ws.numel(), B, T, u,
              LSTM_ACT[activation], LSTM_ACT[recurrent_activation], int(bool(reverse)), int(bool(training)), _stream())
    return h, gates, c, hprev


def lstm_bwd(dy, gates, c, U, c0=None, activation='tanh', recurrent_activation='hard_sigmoid', reverse=False, want_state_grads=False):
    """Backward through time from the stored gates and c: dy (B, T, u) in processing order, or (B, u) for the last step only.
    -> (dz (B, T, 4u) at the input time index, dh0, dc0); the two state gradients (B, u) only under want_state_grads, else None."""
    _chk(dy, gates, c, U, c0)
    B, T, u = _lstm_shape('lstm_bwd', gates, U)
    if tuple(dy.shape) not in ((B, T, u), (B, u)) or tuple(c.shape) != (B, T, u):
        raise ValueError('lstm_bwd: dy %r and c %r beside gates %r' % (tuple(dy.shape), tuple(c.shape), tuple(gates.shape)))
    dz = torch.empty_like(gates)
    dh0 = dc0 = None
    if want_state_grads:
        dh0, dc0 = (torch.empty((B, u), dtype=torch.float32, device=dy.device) for _ in range(2))
    ws = workspace(_lib.size('gn_lstm_bwd_workspace', u), dy.device)
    _lib.call('gn_lstm_bwd', _p(dy), _p(gates), _p(c), _p(c0), _p(U), _p(dz), _p(dh0), _p(dc0), _p(ws), ws.numel(), B, T, u,
              LSTM_ACT[activation], LSTM_ACT[recurrent_activation], int(bool(reverse)), int(dy.dim() == 3), _stream())
    return dz, dh0, dc0


# ---------------------------------------------------------------------------------------------- GRU recurrence (csrc/gru.hip)
def _gru_shape(what, zx, U):
    if zx.dim() != 3 or U.dim() != 2 or U.shape[1] != 3 * U.shape[0] or zx.shape[2] != U.shape[1] or zx.dtype != torch.float32 or U.dtype != torch.float32:
        raise ValueError('%s: float32 (B, T, 3u) beside a recurrent kernel (u, 3u) is expected, got %r and %r' % (what, tuple(zx.shape), tuple(U.shape)))
    return int(zx.shape[0]), int(zx.shape[1]), int(U.shape[0])


def gru_fwd(zx, U, bias, rbias=None, h0=None, activation='tanh', recurrent_activation='hard_sigmoid', reset_after=False, reverse=False,
            training=False):
    """The GRU recurrence over zx (B, T, 3u) = X . W (gate columns z, r, h): -> (h, gates, hprev, aux).  h (B, T, u) is in processing order
    (under `reverse` step s reads zx[:, T-1-s]); in the training phase gates (B, T, 3u) = z, r, hh, hprev (B, T, u), the h that entered each
    step, and aux (B, T, u) = r h_{t-1} (q under reset_after) are stored at the input time index for gru_bwd, else they are None.
    bias (3u); rbias (3u), the recurrent bias, exactly under reset_after; h0 (B, u): None is zeros."""
    _chk(zx, U, bias, rbias, h0)
    B, T, u = _gru_shape('gru_fwd', zx, U)
    if (rbias is not None) != bool(reset_after):
        raise ValueError('gru_fwd: the recurrent bias goes with reset_after, and only with it')
    assert bias.numel() == 3 * u and (rbias is None or rbias.numel() == 3 * u) and (h0 is None or tuple(h0.shape) == (B, u))
    h = torch.empty((B, T, u), dtype=torch.float32, device=zx.device)
    gates = hprev = aux = None
    if training:
        gates = torch.empty((B, T, 3 * u), dtype=torch.float32, device=zx.device)
        hprev, aux = torch.empty_like(h), torch.empty_like(h)
    ws = workspace(_lib.size('gn_gru_fwd_workspace', u), zx.device)
    _lib.call('gn_gru_fwd', _p(zx), _p(U), _p(bias), _p(rbias), _p(h0), _p(h), _p(gates), _p(hprev), _p(aux), _p(ws), ws.numel(), B, T, u,
              LSTM_ACT[activation], LSTM_ACT[recurrent_activation], int(bool(reset_after)), int(bool(reverse)), int(bool(training)), _stream())
    return h, gates, hprev, aux


def gru_bwd(dy, gates, hprev, aux, U, activation='tanh', recurrent_activation='hard_sigmoid', reset_after=False, reverse=False, want_state_grad=False):
    """Backward through time from what gru_fwd stored: dy (B, T, u) in processing order, or (B, u) for the last step only.
    -> (dz, dzr, dh0): dz (B, T, 3u) = da_z, da_r, da_h at the input time index; dzr (B, T, 3u) = da_z, da_r, dq under reset_after, else None;
    dh0 (B, u) only under want_state_grad, else None."""
    _chk(dy, gates, hprev, aux, U)
    B, T, u = _gru_shape('gru_bwd', gates, U)
    if tuple(dy.shape) not in ((B, T, u), (B, u)) or tuple(hprev.shape) != (B, T, u) or tuple(aux.shape) != (B, T, u):
        raise ValueError('gru_bwd: dy %r, hprev %r and aux %r beside gates %r' % (tuple(dy.shape), tuple(hprev.shape), tuple(aux.shape), tuple(gates.shape)))
    dz = torch.empty_like(gates)
    dzr = torch.empty_like(gates) if reset_after else None
    dh0 = torch.empty((B, u), dtype=torch.float32, device=dy.device) if want_state_grad else None
    ws = workspace(_lib.size('gn_gru_bwd_workspace', u), dy.device)
    _lib.call('gn_gru_bwd', _p(dy), _p(gates), _p(hprev), _p(aux), _p(U), _p(dz), _p(dzr), _p(dh0), _p(ws), ws.numel(), B, T, u,
              LSTM_ACT[activation], LSTM_ACT[recurrent_activation], int(bool(reset_after)), int(bool(reverse)), int(dy.dim() == 3), _stream())
    return dz, dzr, dh0


# ---------------------------------------------------------------------------------------------- SimpleRNN recurrence (csrc/rnn.hip)
def _rnn_shape(what, zx, U):
    if zx.dim() != 3 or U.dim() != 2 or U.shape[1] != U.shape[0] or zx.shape[2] != U.shape[1] or zx.dtype != torch.float32 or U.dtype != torch.float32:
        raise ValueError('%s: float32 (B, T, u) beside a recurrent kernel (u, u) is expected, got %r and %r' % (what, tuple(zx.shape), tuple(U.shape)))
    return int(zx.shape[0]), int(zx.shape[1]), int(U.shape[0])


def rnn_fwd(zx, U, bias, h0=None, activation='tanh', reverse=False, training=False):
    """The SimpleRNN recurrence h_t = act((zx_t + b) + h_{t-1} . U) over zx (B, T, u) = X . W: -> (h, hs, hprev).  h (B, T, u) is in processing
    order (under `reverse` step s reads zx[:, T-1-s]); in the training phase hs (B, T, u) = h_t and hprev (B, T, u), the h that entered each
    step, are stored at the input time index for rnn_bwd and the weight gradients, else they are None.  h0 (B, u): None is zeros."""
    _chk(zx, U, bias, h0)
    B, T, u = _rnn_shape('rnn_fwd', zx, U)
    assert bias.numel() == u and (h0 is None or tuple(h0.shape) == (B, u))
    h = torch.empty((B, T, u), dtype=torch.float32, device=zx.device)
    hs = hprev = None
    if training:
        hs, hprev = torch.empty_like(h), torch.empty_like(h)
    ws = workspace(_lib.size('gn_rnn_fwd_workspace', u), zx.device)
    _lib.call('gn_rnn_fwd', _p(zx), _p(U), _p(bias), _p(h0), _p(h), _p(hs), _p(hprev), _p(ws), ws.numel(), B, T, u, LSTM_ACT[activation],
              int(bool(reverse)), int(bool(training)), _stream())
    return h, hs, hprev


def rnn_bwd(dy, hs, U, activation='tanh', reverse=False, want_state_grad=False):
    """Backward through time from the h_t rnn_fwd stored: dy (B, T, u) in processing order, or (B, u) for the last step only.
    -> (dz (B, T, u) at the input time index, dh0 (B, u) only under want_state_grad, else None)."""
    _chk(dy, hs, U)
    B, T, u = _rnn_shape('rnn_bwd', hs, U)
    if tuple(dy.shape) not in ((B, T, u), (B, u)):
        raise ValueError('rnn_bwd: dy %r beside hs %r' % (tuple(dy.shape), tuple(hs.shape)))
    dz = torch.empty_like(hs)
    dh0 = torch.empty((B, u), dtype=torch.float32, device=dy.device) if want_state_grad else None
    ws = workspace(_lib.size('gn_rnn_bwd_workspace', u), dy.device)
    _lib.call('gn_rnn_bwd', _p(dy), _p(hs), _p(U), _p(dz), _p(dh0), _p(ws), ws.numel(), B, T, u, LSTM_ACT[activation], int(bool(reverse)),
              int(dy.dim() == 3), _stream())
    return dz, dh0


# ------------------------------------------------------------------ a pair of directions in one launch (keras Bidirectional)
def _pair(what, ts):
    ts = list(ts)
    if len(ts) != 2:
        raise ValueError('%s: one tensor a direction is expected, got %d' % (what, len(ts)))
    return ts


def _pair_out(B, T, u, concat, seq, device):
    """(the two h or dy views of a pair launch, ld, the merged buffer or None): concat: ONE (B, [T,] 2u) buffer the directions address at columns 0
    and u with ld = 2u; else two (B, [T,] u) buffers with ld = u."""
    lead = (B, T) if seq else (B,)
    if concat:
        y = torch.empty(lead + (2 * u,), dtype=torch.float32, device=device)
        return [y[..., :u], y[..., u:]], 2 * u, y
    return [torch.empty(lead + (u,), dtype=torch.float32, device=device) for _ in range(2)], u, None


def _pair_dy(what, dy, B, T, u, concat):
    """(the two dy views, ld, dy_seq) of a pair backward.  concat: dy is ONE (B, [T,] 2u) tensor, read at columns 0 and u with ld = 2u; else a
    list of two (B, [T,] u) tensors (which may be one tensor twice), ld = u.  dy_seq: whether dy carries the T axis."""
    if concat:
        if not torch.is_tensor(dy):
            raise ValueError('%s: concat=True takes the one concatenated dy, (B, T, 2u) or (B, 2u), not a list' % what)
        _chk(dy)
        if tuple(dy.shape) not in ((B, T, 2 * u), (B, 2 * u)):
            raise ValueError('%s: the concatenated dy is (B, T, 2u) or (B, 2u), got %r' % (what, tuple(dy.shape)))
        return [dy[..., :u], dy[..., u:]], 2 * u, dy.dim() == 3
    if torch.is_tensor(dy):
        raise ValueError('%s: concat=False takes one dy a direction, a list of two (B, T, u) or (B, u) tensors' % what)
    dy = _pair(what, dy)
    _chk(*dy)
    if tuple(dy[0].shape) not in ((B, T, u), (B, u)) or dy[1].shape != dy[0].shape:
        raise ValueError('%s: each dy is (B, T, u) or (B, u), got %r and %r' % (what, tuple(dy[0].shape), tuple(dy[1].shape)))
    return dy, u, dy[0].dim() == 3


def lstm_pair_fwd(zx, U, bias, activation='tanh', recurrent_activation='hard_sigmoid', reverse0=False, seq=True, concat=True, training=False):
    """Two LSTM directions over zx[d] (B, T, 4u) in ONE launch; direction 0 walks with reverse0, direction 1 with its negation, and direction 1's
    step s lands at position T-1-s.  -> (y, h, gates, c, hprev): concat: y is the (B, [T,] 2u) output both directions wrote and h its two column
    views; else y is None and h two (B, [T,] u) tensors.  gates, c, hprev: lists of two as lstm_fwd stores them, or None outside the training
    phase.  seq False: only the last processed step of each direction."""
    zx, U, bias = _pair('lstm_pair_fwd', zx), _pair('lstm_pair_fwd', U), _pair('lstm_pair_fwd', bias)
    _chk(*(zx + U + bias))
    B, T, u = _lstm_shape('lstm_pair_fwd', zx[0], U[0])
    assert (B, T, u) == _lstm_shape('lstm_pair_fwd', zx[1], U[1]) and all(b.numel() == 4 * u for b in bias)
    dev = zx[0].device
    h, ld, y = _pair_out(B, T, u, concat, seq, dev)
    gates = c = hprev = None
    if training:
        gates = [torch.empty((B, T, 4 * u), dtype=torch.float32, device=dev) for _ in range(2)]
        c, hprev = ([torch.empty((B, T, u), dtype=torch.float32, device=dev) for _ in range(2)] for _ in range(2))
    ws = workspace(2 * _lib.size('gn_lstm_fwd_workspace', u), dev)
    _lib.call('gn_lstm_pair_fwd', _ptr_table(zx), _ptr_table(U), _ptr_table(bias), _ptr_table(h), _ptr_table(gates or [None, None]),
              _ptr_table(c or [None, None]), _ptr_table(hprev or [None, None]), _p(ws), ws.numel(), B, T, u, ld, LSTM_ACT[activation],
              LSTM_ACT[recurrent_activation], int(bool(reverse0)), int(bool(seq)), int(bool(training)), _stream())
    return y, h, gates, c, hprev


def lstm_pair_bwd(dy, gates, c, U, activation='tanh', recurrent_activation='hard_sigmoid', reverse0=False, concat=True):
    """Backward through time of both directions in ONE launch.  concat: dy is the concatenated (B, [T,] 2u) gradient, read through ld = 2u;
    else a list of two (B, [T,] u) tensors (the same tensor twice where the merge hands both directions one gradient).  -> [dz_0, dz_1], each (B, T, 4u) at the
    input time index."""
    gates, c, U = _pair('lstm_pair_bwd', gates), _pair('lstm_pair_bwd', c), _pair('lstm_pair_bwd', U)
    _chk(*(gates + c + U))
    B, T, u = _lstm_shape('lstm_pair_bwd', gates[0], U[0])
    assert (B, T, u) == _lstm_shape('lstm_pair_bwd', gates[1], U[1]) and all(tuple(t.shape) == (B, T, u) for t in c)
    dys, ld, dy_seq = _pair_dy('lstm_pair_bwd', dy, B, T, u, concat)
    dz = [torch.empty_like(g) for g in gates]
    ws = workspace(2 * _lib.size('gn_lstm_bwd_workspace', u), dz[0].device)
    _lib.call('gn_lstm_pair_bwd', _ptr_table(dys), _ptr_table(gates), _ptr_table(c), _ptr_table(U), _ptr_table(dz), _p(ws), ws.numel(), B, T, u, ld,
              LSTM_ACT[activation], LSTM_ACT[recurrent_activation], int(bool(reverse0)), int(dy_seq), _stream())
    return dz


def gru_pair_fwd(zx, U, bias, rbias=None, activation='tanh', recurrent_activation='hard_sigmoid', reset_after=False, reverse0=False, seq=True,
                 concat=True, training=False):
    """lstm_pair_fwd for the GRU: -> (y, h, gates, hprev, aux).  rbias: the two recurrent biases, exactly under reset_after."""
    zx, U, bias = _pair('gru_pair_fwd', zx), _pair('gru_pair_fwd', U), _pair('gru_pair_fwd', bias)
    if (rbias is not None) != bool(reset_after):
        raise ValueError('gru_pair_fwd: the recurrent biases go with reset_after, and only with it')
    rbias = _pair('gru_pair_fwd', rbias) if reset_after else [None, None]
    _chk(*(zx + U + bias + rbias))
    B, T, u = _gru_shape('gru_pair_fwd', zx[0], U[0])
    assert (B, T, u) == _gru_shape('gru_pair_fwd', zx[1], U[1]) and all(b is None or b.numel() == 3 * u for b in bias + rbias)
    dev = zx[0].device
    h, ld, y = _pair_out(B, T, u, concat, seq, dev)
    gates = hprev = aux = None
    if training:
        gates = [torch.empty((B, T, 3 * u), dtype=torch.float32, device=dev) for _ in range(2)]
        hprev, aux = ([torch.empty((B, T, u), dtype=torch.float32, device=dev) for _ in range(2)] for _ in range(2))
    ws = workspace(2 * _lib.size('gn_gru_fwd_workspace', u), dev)
    _lib.call('gn_gru_pair_fwd', _ptr_table(zx), _ptr_table(U), _ptr_table(bias), _ptr_table(rbias), _ptr_table(h), _ptr_table(gates or [None, None]),
              _ptr_table(hprev or [None, None]), _ptr_table(aux or [None, None]), _p(ws), ws.numel(), B, T, u, ld, LSTM_ACT[activation],
              LSTM_ACT[recurrent_activation], int(bool(reset_after)), int(bool(reverse0)), int(bool(seq)), int(bool(training)), _stream())
    return y, h, gates, hprev, aux


def gru_pair_bwd(dy, gates, hprev, aux, U, activation='tanh', recurrent_activation='hard_sigmoid', reset_after=False, reverse0=False, concat=True):
    """lstm_pair_bwd for the GRU: -> ([dz_0, dz_1], [dzr_0, dzr_1] under reset_after, else None), as gru_bwd forms them."""
    gates, hprev, aux, U = (_pair('gru_pair_bwd', t) for t in (gates, hprev, aux, U))
    _chk(*(gates + hprev + aux + U))
    B, T, u = _gru_shape('gru_pair_bwd', gates[0], U[0])
    assert (B, T, u) == _gru_shape('gru_pair_bwd', gates[1], U[1]) and all(tuple(t.shape) == (B, T, u) for t in hprev + aux)
    dys, ld, dy_seq = _pair_dy('gru_pair_bwd', dy, B, T, u, concat)
    dz = [torch.empty_like(g) for g in gates]
    dzr = [torch.empty_like(g) for g in gates] if reset_after else None
    ws = workspace(2 * _lib.size('gn_gru_bwd_workspace', u), dz[0].device)
    _lib.call('gn_gru_pair_bwd', _ptr_table(dys), _ptr_table(gates), _ptr_table(hprev), _ptr_table(aux), _ptr_table(U), _ptr_table(dz),
              _ptr_table(dzr or [None, None]), _p(ws), ws.numel(), B, T, u, ld, LSTM_ACT[activation], LSTM_ACT[recurrent_activation],
              int(bool(reset_after)), int(bool(reverse0)), int(dy_seq), _stream())
    return dz, dzr


def rnn_pair_fwd(zx, U, bias, activation='tanh', reverse0=False, seq=True, concat=True, training=False):
    """lstm_pair_fwd for the SimpleRNN: -> (y, h, hs, hprev), hs and hprev lists of two as rnn_fwd stores them, or None outside the training phase."""
    zx, U, bias = _pair('rnn_pair_fwd', zx), _pair('rnn_pair_fwd', U), _pair('rnn_pair_fwd', bias)
    _chk(*(zx + U + bias))
    B, T, u = _rnn_shape('rnn_pair_fwd', zx[0], U[0])
    assert (B, T, u) == _rnn_shape('rnn_pair_fwd', zx[1], U[1]) and all(b.numel() == u for b in bias)
    dev = zx[0].device
    h, ld, y = _pair_out(B, T, u, concat, seq, dev)
    hs = hprev = None
    if training:
        hs, hprev = ([torch.empty((B, T, u), dtype=torch.float32, device=dev) for _ in range(2)] for _ in range(2))
    ws = workspace(2 * _lib.size('gn_rnn_fwd_workspace', u), dev)
    _lib.call('gn_rnn_pair_fwd', _ptr_table(zx), _ptr_table(U), _ptr_table(bias), _ptr_table(h), _ptr_table(hs or [None, None]),
              _ptr_table(hprev or [None, None]), _p(ws), ws.numel(), B, T, u, ld, LSTM_ACT[activation], int(bool(reverse0)), int(bool(seq)),
              int(bool(training)), _stream())
    return y, h, hs, hprev


def rnn_pair_bwd(dy, hs, U, activation='tanh', reverse0=False, concat=True):
    """lstm_pair_bwd for the SimpleRNN: -> [dz_0, dz_1], each (B, T, u) at the input time index, as rnn_bwd forms them."""
    hs, U = _pair('rnn_pair_bwd', hs), _pair('rnn_pair_bwd', U)
    _chk(*(hs + U))
    B, T, u = _rnn_shape('rnn_pair_bwd', hs[0], U[0])
    assert (B, T, u) == _rnn_shape('rnn_pair_bwd', hs[1], U[1])
    dys, ld, dy_seq = _pair_dy('rnn_pair_bwd', dy, B, T, u, concat)
    dz = [torch.empty_like(t) for t in hs]
    ws = workspace(2 * _lib.size('gn_rnn_bwd_workspace', u), dz[0].device)
    _lib.call('gn_rnn_pair_bwd', _ptr_table(dys), _ptr_table(hs), _ptr_table(U), _ptr_table(dz), _p(ws), ws.numel(), B, T, u, ld, LSTM_ACT[activation],
              int(bool(reverse0)), int(dy_seq), _stream())
    return dz


# ---------------------------------------------------------------------------------------------- depthwise conv (csrc/depthwise.hip)
def _dw_shape(what, t, w, channels):
    """(k, C, dm) of a depthwise kernel w beside a float32 (B, rows, `channels` of them) tensor t"""
    if t.dim() != 3 or w.dim() != 3 or t.dtype != torch.float32 or w.dtype != torch.float32:
        raise ValueError('%s: float32 (B, rows, channels) beside a depthwise kernel (k, C, dm) is expected, got %r %s and %r %s'
                         % (what, tuple(t.shape), t.dtype, tuple(w.shape), w.dtype))
    k, C, dm = (int(v) for v in w.shape)
    if int(t.shape[2]) != (C * dm if channels == 'out' else C):
        raise ValueError('%s: %d channels beside a depthwise kernel %r (%s)' % (what, t.shape[2], (k, C, dm), 'C * dm' if channels == 'out' else 'C'))
    return k, C, dm


def dwconv1d_fwd(x, w, stride=1, padding='valid', dilation=1):
    """y (B, Lout, C dm) of x (B, L, C) under the depthwise kernel w (k, C, dm), output channel c dm + m; geometry: conv_geometry (TF's 'same')."""
    _chk(x, w)
    k, C, dm = _dw_shape('dwconv1d_fwd', x, w, 'in')
    B, L = int(x.shape[0]), int(x.shape[1])
    Lout, pl = conv_geometry(L, k, stride, padding, dilation)
    if Lout < 1:
        raise ValueError('dwconv1d_fwd: %d taps (dilation %d, padding %r) on %d rows: the output would have %d rows' % (k, dilation, padding, L, Lout))
    y = torch.empty((B, Lout, C * dm), dtype=torch.float32, device=x.device)
    _lib.call('gn_dwconv1d_fwd', _p(x), _p(w), _p(y), B, L, C, k, dm, int(stride), int(dilation), pl, Lout, _stream())
    return y


def dwconv1d_dgrad(dy, w, L, stride=1, padding='valid', dilation=1):
    """dx (B, L, C) from dy (B, Lout, C dm): every element gathers its (tap, m) pairs, no atomics."""
    _chk(dy, w)
    k, C, dm = _dw_shape('dwconv1d_dgrad', dy, w, 'out')
    B = int(dy.shape[0])
    Lout, pl = conv_geometry(int(L), k, stride, padding, dilation)
    if int(dy.shape[1]) != Lout:
        raise ValueError('dwconv1d_dgrad: dy has %d rows, the conv of %d rows has %d' % (dy.shape[1], L, Lout))
    dx = torch.empty((B, int(L), C), dtype=torch.float32, device=dy.device)
    _lib.call('gn_dwconv1d_dgrad', _p(dy), _p(w), _p(dx), B, int(L), C, k, dm, int(stride), int(dilation), pl, Lout, _stream())
    return dx


def dwconv1d_wgrad(x, dy, k, stride=1, padding='valid', dilation=1, dw=None):
    """dw (k, C, dm) from x (B, L, C) and dy (B, Lout, C dm): per-block partial sums in ops.workspace, summed in a fixed order; written into `dw`
    where given."""
    _chk(x, dy, dw)
    if x.dim() != 3 or dy.dim() != 3 or x.dtype != torch.float32 or dy.dtype != torch.float32 or x.shape[0] != dy.shape[0] or dy.shape[2] % x.shape[2]:
        raise ValueError('dwconv1d_wgrad: float32 x (B, L, C) beside dy (B, Lout, C dm) is expected, got %r %s and %r %s'
                         % (tuple(x.shape), x.dtype, tuple(dy.shape), dy.dtype))
    B, L, C = (int(v) for v in x.shape)
    k, dm = int(k), int(dy.shape[2]) // C
    Lout, pl = conv_geometry(L, k, stride, padding, dilation)
    if int(dy.shape[1]) != Lout:
        raise ValueError('dwconv1d_wgrad: dy has %d rows, the conv of %d rows has %d' % (dy.shape[1], L, Lout))
    if dw is None:
        dw = torch.empty((k, C, dm), dtype=torch.float32, device=x.device)
    elif dw.numel() != k * C * dm or dw.dtype != torch.float32:
        raise ValueError('dwconv1d_wgrad: dw %r %s is no float32 (k, C, dm) = %r' % (tuple(dw.shape), dw.dtype, (k, C, dm)))
    ws = workspace(_lib.size('gn_dwconv1d_wgrad_workspace', B, Lout, C, k, dm), x.device)
    _lib.call('gn_dwconv1d_wgrad', _p(x), _p(dy), _p(dw), _p(ws), ws.numel(), B, L, C, k, dm, int(stride), int(dilation), pl, Lout, _stream())
    return dw


def dropout_mask(shape, rate, seed, offset, device):
    m = torch.empty(shape, dtype=torch.uint8, device=device)
    _lib.call('gn_dropout_mask', _p(m), m.numel(), float(rate), int(seed), int(offset), _stream())
    return m


def conv_fold_bn(w, b, scale, shift):
    """(k, Cin, Cout) kernel and bias with an inference-phase BatchNormalization folded in: conv(x; w', b') = BN_infer(conv(x; w, b))."""
    _chk(w, b, scale, shift)
    w2 = torch.empty_like(w)
    b2 = torch.empty_like(scale)
    _lib.call('gn_conv_fold_bn', _p(w), _p(b), _p(scale), _p(shift), _p(w2), _p(b2), w.numel() // w.shape[-1], w.shape[-1], _stream())
    return w2, b2


_CONV_MATH_WS = {}             # (device, mode) -> the buffer gn_set_conv_math was handed; kept, so switching modes allocates nothing
_CONV_MATH_CUR = [None]        # the buffer of the current mode (StepGraph.capture keeps it alive: a captured graph holds its address)


def default_conv_math():
    """What the engine sets at start-up: GENNET_CONV_MATH, 'wino' when unset."""
    import os
    return os.environ.get('GENNET_CONV_MATH', 'wino')


def default_conv_ws_gb():
    """The opt-in split's workspace the engine starts with: GENNET_CONV_WS_GB, 7 when unset."""
    import os
    return float(os.environ.get('GENNET_CONV_WS_GB', '7'))


WINO_WS_BYTES = 64 << 20       # the library's limit on a transformed kernel (csrc/capi.hip: wino only where it fits); gn_set_conv_math(2) needs it


def set_conv_math(mode=None, workspace_gb=None, device=None):
    """How the MFMA convolutions compute (process-wide; which launches each mode reaches: csrc/capi.hip, select_conv and the table above it):
    'wino' (the engine's default): transform-domain fp32 on the 5-tap layers the selector admits, the direct kernels elsewhere.
    'fp32': the direct exact-fp32 MFMA kernels everywhere (results bit-identical to a k-ordered fmaf chain).
    'bf16x3': opt-in experiment -- the large launches run on the bf16 matrix cores with 3-way split operands; workspace_gb must hold the split
        operands of the largest such launch.
    No arguments: the mode and workspace the engine started with (default_conv_math, default_conv_ws_gb).  One buffer per (device, mode), reused:
    the 'wino' buffer is never replaced, the 'bf16x3' one only by a larger request."""
    dev = device or torch.device('cuda', torch.cuda.current_device())
    if dev.index is None:
        dev = torch.device(dev.type, torch.cuda.current_device())
    if mode is None:
        mode = default_conv_math()
    if workspace_gb is None:
        workspace_gb = default_conv_ws_gb()
    if mode not in ('fp32', 'wino', 'bf16x3'):
        raise ValueError('conv math %r (wino | fp32 | bf16x3)' % (mode,))
    if mode == 'fp32':
        _lib.call('gn_set_conv_math', 0, None, 0)
        _CONV_MATH_CUR[0] = None
        return
    nbytes = WINO_WS_BYTES if mode == 'wino' else int(workspace_gb * (1 << 30))
    key = (dev.type, dev.index, mode)
    ws = _CONV_MATH_WS.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        _CONV_MATH_WS[key] = ws
    _lib.call('gn_set_conv_math', 2 if mode == 'wino' else 1, _p(ws), nbytes)
    _CONV_MATH_CUR[0] = ws


def conv_math_workspace():
    """The device buffer the current conv math works in (None under 'fp32')."""
    return _CONV_MATH_CUR[0]


import contextlib


@contextlib.contextmanager
def conv_math(mode):
    """`with ops.conv_math('fp32'):` -- the given conv arithmetic for the duration of the block, the process default (default_conv_math) afterwards."""
    set_conv_math(mode)
    try:
        yield
    finally:
        set_conv_math()


def prelu_fwd(x, alpha):
    """x (B, ...), alpha with the shape of one sample."""
    _chk(x, alpha)
    y = torch.empty_like(x)
    _lib.call('gn_prelu_fwd', _p(x), _p(alpha), _p(y), x.shape[0], alpha.numel(), _stream())
    return y


def prelu_bwd(dy, x, alpha, need_dx=True, dalpha=None):
    """-> (dx or None, dalpha); dalpha is written into the given tensor when there is one (the flat gradient buffer)."""
    _chk(dy, x, alpha)
    dx = torch.empty_like(x) if need_dx else None
    if dalpha is None:
        dalpha = torch.empty_like(alpha)
    _lib.call('gn_prelu_bwd', _p(dy), _p(x), _p(alpha), _p(dx), _p(dalpha), x.shape[0], alpha.numel(), _stream())
    return dx, dalpha


def dropout_apply(x, mask, rate):
    _chk(x, mask)
    y = torch.empty_like(x)
    _lib.call('gn_dropout_apply', _p(x), _p(mask), _p(y), x.numel(), float(rate), _stream())
    return y


def upsample2_fwd(x):
    _chk(x)
    B, L, Cc = x.shape
    y = torch.empty((B, 2 * L, Cc), dtype=torch.float32, device=x.device)
    _lib.call('gn_upsample2_fwd', _p(x), _p(y), B, L, Cc, _stream())
    return y


def upsample2_bwd(dy):
    _chk(dy)
    B, L2, Cc = dy.shape
    dx = torch.empty((B, L2 // 2, Cc), dtype=torch.float32, device=dy.device)
    _lib.call('gn_upsample2_bwd', _p(dy), _p(dx), B, L2 // 2, Cc, _stream())
    return dx


def subtract_stack_fwd(x, event):
    _chk(x, event)
    B, n = x.shape[0], x.shape[1]
    img = torch.empty((B, n, 2, 1), dtype=torch.float32, device=x.device)
    _lib.call('gn_subtract_stack_fwd', _p(x), _p(event), _p(img), B, n, _stream())
    return img


def subtract_stack_bwd(dimg):
    _chk(dimg)
    B, n = dimg.shape[0], dimg.shape[1]
    dx = torch.empty((B, n, 1), dtype=torch.float32, device=dimg.device)
    _lib.call('gn_subtract_stack_bwd', _p(dimg), _p(dx), B, n, _stream())
    return dx


def affine_stack_fwd(x, a0, b0, a1, b1):
    """x (B, n, 1) -> img (B, n, 2, 1): [a0*x + b0 | a1*x + b1], b0 / b1 (n,) device vectors or None."""
    _chk(x)
    B, n = x.shape[0], x.shape[1]
    img = torch.empty((B, n, 2, 1), dtype=torch.float32, device=x.device)
    _lib.call('gn_affine_stack_fwd', _p(x), _p(b0), _p(b1), float(a0), float(a1), _p(img), B, n, _stream())
    return img


def affine_stack_bwd(dimg, a0, a1):
    _chk(dimg)
    B, n = dimg.shape[0], dimg.shape[1]
    dx = torch.empty((B, n, 1), dtype=torch.float32, device=dimg.device)
    _lib.call('gn_affine_stack_bwd', _p(dimg), float(a0), float(a1), _p(dx), B, n, _stream())
    return dx


def assemble_d_batch(real, noise, fake, event):
    """[real | fake] discriminator batch (2B, n, 2, 1); fake half reversed like the reference's prepend loop."""
    _chk(real, noise, fake, event)
    B, n = real.shape[0], real.shape[1]
    sX = torch.empty((2 * B, n, 2, 1), dtype=torch.float32, device=real.device)
    _lib.call('gn_assemble_d_batch', _p(real), _p(noise), _p(fake), _p(event), _p(sX), B, n, _stream())
    return sX


def fill_uniform(shape, lo, hi, seed, offset, device):
    t = torch.empty(shape, dtype=torch.float32, device=device)
    _lib.call('gn_fill_uniform', _p(t), t.numel(), float(lo), float(hi), int(seed), int(offset), _stream())
    return t


def fill_normal(shape, mean, std, seed, offset, device):
    t = torch.empty(shape, dtype=torch.float32, device=device)
    if isinstance(std, DevScalar):
        _lib.call('gn_fill_normal_dyn', _p(t), t.numel(), float(mean), std.ptr, int(seed), int(offset), _stream())
    else:
        _lib.call('gn_fill_normal', _p(t), t.numel(), float(mean), float(std), int(seed), int(offset), _stream())
    return t


def _noise_out(x, out):
    _chk(x, out)
    return torch.empty_like(x) if out is None else out


def gaussian_noise(x, stddev, seed, offset, out=None):
    """y = x + stddev * z, z = fill_normal's N(0, 1) draw at (seed, offset) (GaussianNoise)."""
    y = _noise_out(x, out)
    _lib.call('gn_gaussian_noise_fwd', _p(x), _p(y), x.numel(), float(stddev), int(seed), int(offset), _stream())
    return y


def gaussian_dropout(x, sd, seed, offset, out=None):
    """y = x * (1 + sd * z) (GaussianDropout's forward, and its backward with the forward's (seed, offset))."""
    y = _noise_out(x, out)
    _lib.call('gn_gaussian_dropout_apply', _p(x), _p(y), x.numel(), float(sd), int(seed), int(offset), _stream())
    return y


def alpha_dropout_fwd(x, rate, a, b, alpha_p, seed, offset, out=None):
    """y = keep ? a * x + b : a * alpha_p + b, keep = dropout_mask's draw at (seed, offset) (AlphaDropout)."""
    y = _noise_out(x, out)
    _lib.call('gn_alpha_dropout_fwd', _p(x), _p(y), x.numel(), float(rate), float(a), float(b), float(alpha_p), int(seed), int(offset), _stream())
    return y


def alpha_dropout_bwd(dy, rate, a, seed, offset, out=None):
    """dx = keep ? a * dy : 0 with the forward's (seed, offset)."""
    dx = _noise_out(dy, out)
    _lib.call('gn_alpha_dropout_bwd', _p(dy), _p(dx), dy.numel(), float(rate), float(a), int(seed), int(offset), _stream())
    return dx


def gather_rows(src, idx):
    _chk(src, idx)
    rows, width = idx.numel(), src.shape[1]
    out = torch.empty((rows, width), dtype=torch.float32, device=src.device)
    _lib.call('gn_gather_rows', _p(src), _p(idx), _p(out), rows, width, _stream())
    return out


def axpy(y, x, a):
    _chk(y, x)
    _lib.call('gn_axpy', _p(y), _p(x), float(a), y.numel(), _stream())
    return y


# ---------------------------------------------------------------------------------------------- merge layers (csrc/merge.hip)
MERGE_MAX_INPUTS = _lib.CONSTS['GN_MERGE_MAX_INPUTS']
MERGE_MODES = dict((k, v) for k, v in _lib.enum_members('GN_MERGE_').items() if k != 'max_inputs')     # enum gn_merge: {'add': 0, 'sub': 1, ...}


def _ptr_table(ts):
    """The host array of device pointers (None: NULL) the merge entry points read when they are called."""
    return (ctypes.c_void_p * len(ts))(*[_p(t) for t in ts])


def _merge_inputs(what, xs):
    xs = list(xs)
    if not 1 <= len(xs) <= MERGE_MAX_INPUTS:
        raise ValueError('%s: %d inputs, 1 .. %d (GN_MERGE_MAX_INPUTS) are supported' % (what, len(xs), MERGE_MAX_INPUTS))
    _chk(*xs)
    if any(x.shape != xs[0].shape or x.dtype != torch.float32 for x in xs):
        raise ValueError('%s: float32 inputs of one shape are expected, got %s' % (what, [tuple(x.shape) for x in xs]))
    return xs


def merge_fwd(mode, xs, out=None):
    """x0 o x1 o ... left to right ('add' | 'sub' | 'mul' | 'avg' | 'max' | 'min'; 'avg': the sum / k), one pass over equal-shaped tensors."""
    xs = _merge_inputs('merge_fwd', xs)
    _chk(out)
    y = torch.empty_like(xs[0]) if out is None else out
    assert y.shape == xs[0].shape
    _lib.call('gn_merge_fwd', MERGE_MODES[mode], _ptr_table(xs), len(xs), _p(y), y.numel(), _stream())
    return y


def merge_bwd(mode, dy, xs, which, out=None):
    """The gradient of input `which` for 'mul' (dy times the other inputs) and 'max' / 'min' (dy where it is the first input at the extremum)."""
    xs = _merge_inputs('merge_bwd', xs)
    _chk(dy, out)
    dx = torch.empty_like(dy) if out is None else out
    assert dy.shape == xs[0].shape and dx.shape == dy.shape
    _lib.call('gn_merge_bwd', MERGE_MODES[mode], _p(dy), _ptr_table(xs), len(xs), int(which), _p(dx), dy.numel(), _stream())
    return dx


def scale(x, a, out=None):
    """a * x into a new tensor (x is not written: the gradient a merge layer receives is shared between its inputs)."""
    _chk(x, out)
    y = torch.empty_like(x) if out is None else out
    _lib.call('gn_scale', _p(x), float(a), _p(y), x.numel(), _stream())
    return y


def _concat_views(shapes, axis):
    """(outer, [w_i]) of tensors that differ along `axis` only: outer = the product of the dimensions in front, w_i = extent_i * those behind."""
    outer = 1
    for v in shapes[0][:axis]:
        outer *= int(v)
    widths = []
    for s in shapes:
        w = 1
        for v in s[axis:]:
            w *= int(v)
        widths.append(w)
    return outer, widths


def concat_fwd(xs, axis, out=None):
    """torch.cat(xs, axis) in one launch; axis >= 0 counts the batch axis."""
    xs = list(xs)
    _chk(*(xs + [out]))
    shapes = [tuple(x.shape) for x in xs]
    outer, widths = _concat_views(shapes, axis)
    shape = shapes[0][:axis] + (sum(s[axis] for s in shapes),) + shapes[0][axis + 1:]
    y = torch.empty(shape, dtype=torch.float32, device=xs[0].device) if out is None else out
    assert tuple(y.shape) == shape and all(s[:axis] + s[axis + 1:] == shape[:axis] + shape[axis + 1:] for s in shapes)
    _lib.call('gn_concat_fwd', _ptr_table(xs), (ctypes.c_int * len(xs))(*widths), len(xs), _p(y), outer, _stream())
    return y


def concat_bwd(dy, shapes, axis, wanted=None, outs=None):
    """[dx_i or None] of concat_fwd in one launch: the slices of dy along `axis` for the inputs that are `wanted` (default: all)."""
    shapes = [tuple(int(v) for v in s) for s in shapes]
    wanted = [True] * len(shapes) if wanted is None else list(wanted)
    _chk(dy)
    outer, widths = _concat_views(shapes, axis)
    assert dy.numel() == outer * sum(widths)
    if outs is None:
        outs = [torch.empty(s, dtype=torch.float32, device=dy.device) if w else None for s, w in zip(shapes, wanted)]
    _chk(*outs)
    _lib.call('gn_concat_bwd', _p(dy), _ptr_table(outs), (ctypes.c_int * len(shapes))(*widths), len(shapes), outer, _stream())
    return outs


# ---------------------------------------------------------------------------------------------- dilated / causal Conv1D (csrc/dilate.hip)
def dilate_split(x, d, off, M, out=None):
    """x (B, L, C) -> xs (B*d, M, C), the d phases of x behind `off` rows of padding: xs[b*d + p, m] = x[b, m*d + p - off] inside [0, L), +0
    elsewhere; input rows beyond the M rows are dropped.  d = 1: a copy behind `off` zero rows."""
    _chk(x, out)
    B, L, C = (int(v) for v in x.shape)
    d, off, M = int(d), int(off), int(M)
    if d < 1 or M < 1:
        raise ValueError('dilate_split: d %d, M %d must be >= 1' % (d, M))
    xs = torch.empty((B * d, M, C), dtype=torch.float32, device=x.device) if out is None else out
    assert tuple(xs.shape) == (B * d, M, C)
    _lib.call('gn_dilate_split', _p(x), _p(xs), B, L, C, d, off, M, _stream())
    return xs


def dilate_merge(xs, B, d, off, L, out=None):
    """xs (B*d, M, C) -> x (B, L, C), x[b, i] = xs[b*d + (i + off) % d, (i + off) // d]: the adjoint of dilate_split(x, d, off, M)."""
    _chk(xs, out)
    Bd, M, C = (int(v) for v in xs.shape)
    B, d, off, L = int(B), int(d), int(off), int(L)
    if B < 1 or d < 1 or L < 1 or Bd != B * d:
        raise ValueError('dilate_merge: %d phase sequences are not B = %d times d = %d (L = %d)' % (Bd, B, d, L))
    x = torch.empty((B, L, C), dtype=torch.float32, device=xs.device) if out is None else out
    assert tuple(x.shape) == (B, L, C)
    _lib.call('gn_dilate_merge', _p(xs), _p(x), B, L, C, d, off, M, _stream())
    return x


# ---------------------------------------------------------------------------------------------- sequence plumbing (csrc/sequence.hip)
def permute(x, perm, out=None):
    """x.permute(perm).contiguous() for 2 .. 4 axes (perm counts the batch axis, axis 0): a copy, a row copy or a tiled transposition.  The backward
    is the same call with the inverse permutation."""
    _chk(x, out)
    perm = [int(v) for v in perm]
    R = x.dim()
    if len(perm) != R:
        raise ValueError('permute: %d axes for a tensor of %d' % (len(perm), R))
    if sorted(perm) != list(range(R)):
        raise ValueError('permute: %r is no permutation of 0 .. %d' % (perm, R - 1))
    shape = tuple(int(x.shape[p]) for p in perm)
    y = torch.empty(shape, dtype=torch.float32, device=x.device) if out is None else out
    assert tuple(y.shape) == shape
    _lib.call('gn_permute', _p(x), _p(y), (ctypes.c_int * R)(*[int(v) for v in x.shape]), (ctypes.c_int * R)(*perm), R, _stream())
    return y


def repeat_fwd(x, n, out=None):
    """x (B, C) -> (B, n, C), every row n times (keras RepeatVector)."""
    _chk(x, out)
    B, C = (int(v) for v in x.shape)
    n = int(n)
    y = torch.empty((B, n, C), dtype=torch.float32, device=x.device) if out is None else out
    assert tuple(y.shape) == (B, n, C)
    _lib.call('gn_repeat_fwd', _p(x), _p(y), B, n, C, _stream())
    return y


def repeat_bwd(dy, out=None):
    """dy (B, n, C) -> dx (B, C) = the sum over n, accumulated in fp64 in a fixed order (by the shape alone) and rounded once."""
    _chk(dy, out)
    B, n, C = (int(v) for v in dy.shape)
    dx = torch.empty((B, C), dtype=torch.float32, device=dy.device) if out is None else out
    assert tuple(dx.shape) == (B, C)
    nb = _lib.size('gn_repeat_bwd_workspace', B, n, C)
    ws = workspace(nb, dy.device) if nb else None
    _lib.call('gn_repeat_bwd', _p(dy), _p(dx), _p(ws), ws.numel() if nb else 0, B, n, C, _stream())
    return dx


def shift1d(x, offset, Lout, out=None):
    """x (B, Lin, C) -> y (B, Lout, C), y[b, l] = x[b, l - offset] inside [0, Lin), +0 elsewhere: ZeroPadding1D with offset = left and
    Lout = left + Lin + right, Cropping1D with offset = -left and Lout = Lin - left - right; each is the other's backward."""
    _chk(x, out)
    B, Lin, C = (int(v) for v in x.shape)
    offset, Lout = int(offset), int(Lout)
    if Lout < 1:
        raise ValueError('shift1d: Lout %d must be >= 1' % Lout)
    y = torch.empty((B, Lout, C), dtype=torch.float32, device=x.device) if out is None else out
    assert tuple(y.shape) == (B, Lout, C)
    _lib.call('gn_shift1d', _p(x), _p(y), B, Lin, Lout, C, offset, _stream())
    return y


# ---------------------------------------------------------------------------------------------- batch norm
def bn_stats(x2d):
    """x2d: (rows, C) view.  Returns fp64 sums tensor (2*C,): [sum x | sum x^2]."""
    _chk(x2d)
    rows, Cc = x2d.shape
    sums = torch.empty((2 * Cc,), dtype=torch.float64, device=x2d.device)
    nb = _lib.size('gn_bn_stats_workspace', rows, Cc)
    ws = workspace(nb, x2d.device)
    _lib.call('gn_bn_stats', _p(x2d), rows, Cc, _p(sums), _p(ws), ws.numel(), _stream())
    return sums


def bn_finalize(sums, count, gamma, beta, eps, momentum, moving_mean, moving_var, zero_debias=None):
    """zero_debias = (biased_mean, biased_var, local_step): TF's assign_moving_average(zero_debias=True) with local_step the already
    incremented update count; None: the plain exponential average."""
    Cc = gamma.numel()
    dev = gamma.device
    scale, shift, smean, sinv = (torch.empty((Cc,), dtype=torch.float32, device=dev) for _ in range(4))
    if zero_debias is not None:
        bm, bv, step = zero_debias
        if isinstance(step, DevScalar):
            _lib.call('gn_bn_finalize_zero_debias_dyn', _p(sums), float(count), _p(gamma), _p(beta), float(eps), float(momentum), _p(moving_mean), _p(moving_var),
                      _p(bm), _p(bv), step.ptr, _p(scale), _p(shift), _p(smean), _p(sinv), Cc, _stream())
        else:
            _lib.call('gn_bn_finalize_zero_debias', _p(sums), float(count), _p(gamma), _p(beta), float(eps), float(momentum), _p(moving_mean), _p(moving_var),
                      _p(bm), _p(bv), int(step), _p(scale), _p(shift), _p(smean), _p(sinv), Cc, _stream())
    else:
        _lib.call('gn_bn_finalize', _p(sums), float(count), _p(gamma), _p(beta), float(eps), float(momentum), _p(moving_mean), _p(moving_var),
                  _p(scale), _p(shift), _p(smean), _p(sinv), Cc, _stream())
    return scale, shift, smean, sinv


def bn_infer_coeffs(gamma, beta, moving_mean, moving_var, eps):
    Cc = gamma.numel()
    scale, shift = (torch.empty((Cc,), dtype=torch.float32, device=gamma.device) for _ in range(2))
    _lib.call('gn_bn_infer_coeffs', _p(gamma), _p(beta), _p(moving_mean), _p(moving_var), float(eps), _p(scale), _p(shift), Cc, _stream())
    return scale, shift


def bn_apply(x2d, scale, shift, mask=None, act='linear', act_param=0.0, rate=0.0):
    _chk(x2d, mask)
    rows, Cc = x2d.shape
    y = torch.empty_like(x2d)
    _lib.call('gn_bn_apply', _p(x2d), _p(scale), _p(shift), _p(mask), _p(y), rows, Cc, ACT[act], float(act_param), float(rate), _stream())
    return y


def bn_apply_dropgen(x2d, scale, shift, act, act_param, rate, seed, offset):
    """bn_apply + activation + dropout with the keep-mask drawn in the same pass (dropout_mask's stream); -> (y, mask)."""
    _chk(x2d)
    rows, Cc = x2d.shape
    y = torch.empty_like(x2d)
    mask = torch.empty((rows, Cc), dtype=torch.uint8, device=x2d.device)
    _lib.call('gn_bn_apply_dropgen', _p(x2d), _p(scale), _p(shift), _p(mask), _p(y), rows, Cc, ACT[act], float(act_param), float(rate), int(seed), int(offset),
              _stream())
    return y, mask


def bn_bwd_stats(dy2d, y2d, x2d, mask, smean, sinv, act='linear', act_param=0.0, rate=0.0, scale=None, shift=None):
    """scale / shift (the forward's bn_finalize outputs): the activation output is recomputed from x2d and y2d (may be None) is not read."""
    _chk(dy2d, y2d, x2d, mask)
    rows, Cc = x2d.shape
    dsums = torch.empty((2 * Cc,), dtype=torch.float64, device=x2d.device)
    nb = _lib.size('gn_bn_stats_workspace', rows, Cc)
    ws = workspace(nb, x2d.device)
    _lib.call('gn_bn_bwd_stats', _p(dy2d), _p(y2d), _p(x2d), _p(mask), _p(smean), _p(sinv), _p(dsums), _p(ws), ws.numel(), rows, Cc,
              ACT[act], float(act_param), float(rate), _p(scale), _p(shift), _stream())
    return dsums


def bn_bwd_apply(dy2d, y2d, x2d, mask, gamma, smean, sinv, dsums_global, count, dsums_local, dgamma, dbeta, act='linear', act_param=0.0, rate=0.0,
                 scale=None, shift=None):
    rows, Cc = x2d.shape
    dx = torch.empty_like(x2d)
    _lib.call('gn_bn_bwd_apply', _p(dy2d), _p(y2d), _p(x2d), _p(mask), _p(gamma), _p(smean), _p(sinv), _p(dsums_global), float(count),
              _p(dsums_local), _p(dx), _p(dgamma), _p(dbeta), rows, Cc, ACT[act], float(act_param), float(rate), _p(scale), _p(shift), _stream())
    return dx


# the same four passes over an axis that is not the last one: x3d an (outer, P, inner) view, one parameter per p (csrc/bn_axis.hip); no
# activation, no mask.  bn_finalize / bn_infer_coeffs serve them with P parameters and count = outer * inner.
def _axis_ws(x3d):
    outer, P, inner = x3d.shape
    return workspace(_lib.size('gn_bn_axis_stats_workspace', outer, P, inner), x3d.device)


def bn_axis_stats(x3d):
    """-> fp64 sums (2*P,): [sum over (o, i) of x | of x^2]."""
    _chk(x3d)
    outer, P, inner = x3d.shape
    sums = torch.empty((2 * P,), dtype=torch.float64, device=x3d.device)
    ws = _axis_ws(x3d)
    _lib.call('gn_bn_axis_stats', _p(x3d), outer, P, inner, _p(sums), _p(ws), ws.numel(), _stream())
    return sums


def bn_axis_apply(x3d, scale, shift):
    _chk(x3d)
    outer, P, inner = x3d.shape
    y = torch.empty_like(x3d)
    _lib.call('gn_bn_axis_apply', _p(x3d), _p(scale), _p(shift), _p(y), outer, P, inner, _stream())
    return y


def bn_axis_bwd_stats(dy3d, x3d, smean, sinv):
    """-> fp64 dsums (2*P,): [sum dy | sum dy * xhat]."""
    _chk(dy3d, x3d)
    outer, P, inner = x3d.shape
    dsums = torch.empty((2 * P,), dtype=torch.float64, device=x3d.device)
    ws = _axis_ws(x3d)
    _lib.call('gn_bn_axis_bwd_stats', _p(dy3d), _p(x3d), _p(smean), _p(sinv), _p(dsums), _p(ws), ws.numel(), outer, P, inner, _stream())
    return dsums


def bn_axis_bwd_apply(dy3d, x3d, gamma, smean, sinv, dsums_global, count, dsums_local, dgamma, dbeta):
    _chk(dy3d, x3d)
    outer, P, inner = x3d.shape
    dx = torch.empty_like(x3d)
    ws = _axis_ws(x3d)
    _lib.call('gn_bn_axis_bwd_apply', _p(dy3d), _p(x3d), _p(gamma), _p(smean), _p(sinv), _p(dsums_global), float(count), _p(dsums_local), _p(dx),
              _p(dgamma), _p(dbeta), _p(ws), ws.numel(), outer, P, inner, _stream())
    return dx


class ConvGrad1(object):
    """The data gradient of a Conv1D(1 filter, k taps, stride 1), NOT materialised: g (B, Lout, 1) the conv's output gradient, w (k, C, 1)
    its kernel, L the conv's input length.  Consumed by bn_bwd_stats_conv1 / bn_bwd_apply_conv1 (gn_bn_bwd_*_conv1)."""

    def __init__(self, g, w, L, pad_left):
        _chk(g, w)
        self.g, self.w, self.L, self.pad_left = g, w, int(L), int(pad_left)
        self.B, self.Lout = int(g.shape[0]), int(g.shape[1])
        self.k, self.C = int(w.shape[0]), int(w.shape[1])
        self.shape = (self.B, self.L, self.C)


def bn_bwd_stats_conv1(cg, x2d, mask, smean, sinv, act, act_param, rate, scale, shift):
    _chk(x2d, mask)
    rows, Cc = x2d.shape
    assert rows == cg.B * cg.L and Cc == cg.C
    dsums = torch.empty((2 * Cc,), dtype=torch.float64, device=x2d.device)
    ws = workspace(_lib.size('gn_bn_stats_workspace', rows, Cc), x2d.device)
    _lib.call('gn_bn_bwd_stats_conv1', _p(cg.g), _p(cg.w), cg.L, cg.Lout, cg.k, cg.pad_left, _p(x2d), _p(mask), _p(smean), _p(sinv), _p(dsums), _p(ws),
              ws.numel(), rows, Cc, ACT[act], float(act_param), float(rate), _p(scale), _p(shift), _stream())
    return dsums


def bn_bwd_apply_conv1(cg, x2d, mask, gamma, smean, sinv, dsums_global, count, dsums_local, dgamma, dbeta, act, act_param, rate, scale, shift):
    rows, Cc = x2d.shape
    dx = torch.empty_like(x2d)
    _lib.call('gn_bn_bwd_apply_conv1', _p(cg.g), _p(cg.w), cg.L, cg.Lout, cg.k, cg.pad_left, _p(x2d), _p(mask), _p(gamma), _p(smean), _p(sinv),
              _p(dsums_global), float(count), _p(dsums_local), _p(dx), _p(dgamma), _p(dbeta), rows, Cc, ACT[act], float(act_param), float(rate),
              _p(scale), _p(shift), _stream())
    return dx


# ---------------------------------------------------------------------------------------------- loss / optimizer
def loss(kind, p, y, Bglobal=None):
    """kind 'binary_crossentropy' | 'mean_squared_error'. p, y (B,1). Returns (dp, out[2] = [loss share, hit count])."""
    _chk(p, y)
    B = p.shape[0]
    dp = torch.empty_like(p)
    out = torch.empty((2,), dtype=torch.float32, device=p.device)
    fn = {'binary_crossentropy': 'gn_bce_loss', 'mean_squared_error': 'gn_mse_loss'}[kind]
    _lib.call(fn, _p(p), _p(y), _p(dp), _p(out), B, int(Bglobal or B), _stream())
    return dp, out


LOSS_KINDS = _lib.enum_members('GN_LOSS_')                      # enum gn_loss ...
del LOSS_KINDS['kinds']                                         # ... without its count, GN_LOSS_KINDS
LOSS_ALIASES = {'mse': 'mean_squared_error', 'mae': 'mean_absolute_error', 'mape': 'mean_absolute_percentage_error',
                'msle': 'mean_squared_logarithmic_error', 'kld': 'kullback_leibler_divergence', 'cosine': 'cosine_proximity'}
# element count from which the engine sends binary_crossentropy / mean_squared_error to loss_pass instead of the one-block kernel of loss():
# the measured crossover (scripts/loss_bench.py) lies far below; the floor of 131 072 keeps every loss call of the
# benchmark, the scripts and the older tests on the kernel, and the bits, it always had
LOSS_PASS_MIN_ELEMENTS = 131072


def loss_pass(kind, p, y, denom=None, grad=True, dp=None):
    """gn_loss_pass: kind a name of LOSS_KINDS (or its integer); p, y (rows, cols) contiguous, any 4-byte alignment.  Returns (dp, out):
    out[2] = [sum of the per-row terms / denom, #elements with round(p) == y], dp = d out[0] / dp (None with grad=False: only out is
    written).  denom: the global row count (default rows).  dp: a tensor to write the gradient into instead of a new one."""
    _chk(p, y, dp)
    rows, cols = p.shape
    if grad and dp is None:
        dp = torch.empty_like(p)
    out = torch.empty((2,), dtype=torch.float32, device=p.device)
    ws = workspace(_lib.size('gn_loss_pass_workspace', rows, cols), p.device)
    _lib.call('gn_loss_pass', LOSS_KINDS.get(kind, kind), _p(p), _p(y), _p(dp) if grad else None, _p(out), rows, cols, float(rows if denom is None else denom),
              _p(ws), ws.numel(), _stream())
    return (dp if grad else None), out


def weight_count(w, count=None):
    """gn_weight_count: the number of w[r] != 0 of a (rows,) weight vector as a one-element fp64 device tensor (exact; it never visits the
    host).  Data-parallel ranks all-reduce it before loss_pass_weighted reads it.  count: a tensor (or one-element view) to write into."""
    _chk(w, count)
    if count is None:
        count = torch.empty((1,), dtype=torch.float64, device=w.device)
    ws = workspace(_lib.size('gn_weight_count_workspace', w.numel()), w.device)
    _lib.call('gn_weight_count', _p(w), w.numel(), _p(count), _p(ws), ws.numel(), _stream())
    return count


def loss_pass_weighted(kind, p, y, w, count, grad=True, dp=None):
    """gn_loss_pass_weighted: loss_pass with one weight per row (w: (rows,) fp32) and the normaliser `count` read on the device (a one-element
    fp64 tensor: weight_count(w), summed over the ranks).  Returns (dp, out): out[3] = [sum_r w_r term_r / count, #elements with
    round(p) == y, sum_r w_r hits_r / (count cols)], dp = d out[0] / dp (None with grad=False)."""
    _chk(p, y, w, count, dp)
    rows, cols = p.shape
    if w.numel() != rows or w.dtype != torch.float32:
        raise ValueError('loss_pass_weighted: %d float32 weights expected, got %s %s' % (rows, tuple(w.shape), w.dtype))
    if count.numel() != 1 or count.dtype != torch.float64:
        raise ValueError('loss_pass_weighted: count is one float64 value on the device')
    if grad and dp is None:
        dp = torch.empty_like(p)
    out = torch.empty((3,), dtype=torch.float32, device=p.device)
    ws = workspace(_lib.size('gn_loss_pass_weighted_workspace', rows, cols), p.device)
    _lib.call('gn_loss_pass_weighted', LOSS_KINDS.get(kind, kind), _p(p), _p(y), _p(w), _p(count), _p(dp) if grad else None, _p(out), rows, cols,
              _p(ws), ws.numel(), _stream())
    return (dp if grad else None), out


def adam_step(p, g, m, v, lr_t, b1, b2, eps):
    """lr_t: a python float, or (inside a captured step graph) the integer device address of a float the host refreshes before every replay."""
    _chk(p, g, m, v)
    if isinstance(lr_t, DevScalar):
        _lib.call('gn_adam_step_dyn', _p(p), _p(g), _p(m), _p(v), p.numel(), lr_t.ptr, float(b1), float(b2), float(eps), _stream())
    else:
        _lib.call('gn_adam_step', _p(p), _p(g), _p(m), _p(v), p.numel(), float(lr_t), float(b1), float(b2), float(eps), _stream())


OPT_RULES = _lib.enum_members('GN_OPT_')                        # enum gn_optim_rule


def optim_step(rule, p, g, states, lr, h0=0.0, h1=0.0, eps=0.0, nesterov=False, clip_scale=None, clipvalue=0.0):
    """One fused update of the Keras rule `rule` (OPT_RULES) over p with gradient g and the rule's state tensors (engine.Optimizer).
    lr: a python float or a DevScalar (captured step); clip_scale: None or a (1,) fp32 device tensor (optim_clip_factor)."""
    _chk(p, g, *states)
    st = [_p(s) for s in states] + [None] * (3 - len(states))
    dyn = isinstance(lr, DevScalar)
    _lib.call('gn_optim_step', OPT_RULES[rule], _p(p), _p(g), st[0], st[1], st[2], p.numel(), 0.0 if dyn else float(lr), lr.ptr if dyn else None,
              float(h0), float(h1), float(eps), 1 if nesterov else 0, None if clip_scale is None else _p(clip_scale), float(clipvalue), _stream())


def optim_sumsq_slots(n):
    return _lib.size('gn_optim_sumsq_slots', int(n))


def optim_sumsq(g, partials):
    """fp64 partial sums of g^2 into partials[:optim_sumsq_slots(g.numel())]."""
    _chk(g)
    _lib.call('gn_optim_sumsq', _p(g), g.numel(), _p(partials), _stream())


def optim_clip_factor(partials, clipnorm, factor):
    """factor[0] = clipnorm / norm if norm >= clipnorm else 1, norm = sqrt(sum of all partials) (fixed order)."""
    _lib.call('gn_optim_clip_factor', _p(partials), partials.numel(), float(clipnorm), _p(factor), _stream())


# ---------------------------------------------------------------------------------------------- regularizers (csrc/regularizer.hip)
@functools.lru_cache(maxsize=None)
def reg_partials(n):
    """fp64 partials that reg_pass writes for a tensor of n floats (a function of n alone)."""
    return _lib.size('gn_reg_partials', int(n))


def reg_pass(x, g, l1, l2, partials):
    """Penalty and gradient of one regularized tensor in one read of x: partials[:reg_partials(x.numel())] = fp64 block partials of
    l1 sum|x| + l2 sum x^2, and g += l1 sign(x) + 2 l2 x (sign(+-0) = 0) unless g is None (penalty only)."""
    _chk(x, g, partials)
    if partials.dtype != torch.float64 or (g is not None and g.numel() != x.numel()):
        raise ValueError('reg_pass: float64 partials and a gradient of the size of x are expected')
    _lib.call('gn_reg_pass', _p(x), _p(g), x.numel(), float(l1), float(l2), _p(partials), partials.numel(), _stream())


def reg_grad(y, g, l1, l2, inplace=False):
    """g + l1 sign(y) + 2 l2 y (the gradient of an activity penalty, added to the gradient arriving at y), into g itself or a new tensor."""
    _chk(y, g)
    if g.numel() != y.numel():
        raise ValueError('reg_grad: a gradient of %d values for an output of %d' % (g.numel(), y.numel()))
    out = g if inplace else torch.empty_like(g)
    _lib.call('gn_reg_grad', _p(y), _p(g), _p(out), y.numel(), float(l1), float(l2), _stream())
    return out


def reg_finish(partials, out):
    """out[0] (fp32) = the sum of all fp64 partials, in a fixed order, rounded once."""
    _chk(partials, out)
    _lib.call('gn_reg_finish', _p(partials), partials.numel(), _p(out), _stream())


class DevScalar(object):
    """Address of one step-varying scalar in a step graph's parameter block (engine.StepGraph.slot)."""

    def __init__(self, ptr):
        self.ptr = int(ptr)


def set_rng_base(ptr):
    _lib.call('gn_set_rng_base', None if ptr is None else int(ptr))


# ---------------------------------------------------------------------------------------------- profiling hooks
_PROF_ON = False


def prof_enable(on=True):
    global _PROF_ON
    _PROF_ON = bool(on)
    _lib.call('gn_prof_enable', 1 if on else 0)


def prof_enabled():
    return _PROF_ON


def prof_reset():
    _lib.call('gn_prof_reset')


def prof_collect(kind=-1):
    """kind 0: conv_mfma kernels (forward + data gradient), 1: wgrad_mfma_kernel, 2: bf16x3 conv (opt-in), 3: fused synthesiser,
    9: anyc forward-form launches (forward, data gradient, each phase of a strided one), 10: anyc weight gradient,
    11 .. 17: the small-channel kernels of csrc/small_conv.hip, one kind each -- 11: conv_smallcin (Cin <= 4), 12: conv_smallcout (Cout <= 4),
    13: conv_cout1_rows (Cout 1, Cin >= 256, 5 contiguous taps, unit strides), 14: wgrad_smallcin_tab, 15: wgrad_small (small Cout, stride > 1),
    16: wgrad_smallcout_s1 (small Cout, stride 1), 17: level 1 of the two-level partial-slab reduce (more than 64 chunks), -1: all."""
    import ctypes
    out = (ctypes.c_double * 4)()
    _lib.call('gn_prof_collect', int(kind), ctypes.cast(out, ctypes.c_void_p))
    return {'launches': int(out[0]), 'ms': out[1], 'flop': out[2], 'bytes': out[3]}
