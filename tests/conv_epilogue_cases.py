"""The case table of tests/test_conv_epilogue_gpu.py and of its recorder tests/tools/record_conv_epilogue_golden.py: every epilogue form of the
transform-domain conv kernels (csrc/conv_wino.hip, csrc/conv_wino_s2.hip) at the smallest shapes that reach each of their paths, with seeded
numpy inputs, so that the same table run on two builds of the library gives outputs that can be compared byte for byte.

A case is (op, geometry, Cin, Cout, variant) IN THE KERNEL'S TERMS: Cin is the reduction width (the channels of x, or of dy in a data gradient)
and Cout the width of what the epilogue writes (y, or dx).  B = 2 everywhere.
  geometry  s1same (L 133: 67 output pairs, a full 64-pair row tile and a ragged one), s1valid (L 37), s2same (L 261), s2valid (L 70)
  Cout      64, 128: one and two column tiles
  Cin       8, 16, 24, 48, 56: 1, 2, 3, 6, 7 channel chunks.  The selector (csrc/capi.hip) sends a layer to the transform-domain families from
            Cin 32 up, so 48 and 56 carry every op; 8, 16, 24 reach conv_wino_kernel through its direct entry (ops.conv1d_fwd_wino) at unit
            stride, and at stride 2 run as plain forwards on the kernel the selector gives them.
  ops       fwd (linear, relu, leaky, tanh, and sigmoid: the runtime-switch epilogue), fwd_dropout (leaky, sigmoid), fwd_stats (y and the fp64
            sums), dgrad plain / through a relu / a tanh / a LeakyReLU + Dropout producer (epilogue modes 0, 1, 0 + statistics, 0, 2, 2, 3).
"""
import hashlib
import zlib

import numpy as np

B = 2
GEOMETRIES = {'s1same': (1, 'same', 133), 's1valid': (1, 'valid', 37), 's2same': (2, 'same', 261), 's2valid': (2, 'valid', 70)}
COUTS = (64, 128)
CINS = (8, 16, 24, 48, 56)
SELECTOR_MIN_CIN = 32
FWD_ACTS = ('linear', 'relu', 'leaky', 'tanh', 'sigmoid')
DGRAD_PRODUCERS = ('none', 'relu', 'tanh', 'leaky_dropout')
HEAD = 256                       # output values kept per case for diagnostics
RATE = 0.4                       # dropout rate of the fused forms
LEAK = 0.2


def cases():
    """[(op, geometry, Cin, Cout, variant)] in a fixed order."""
    out = []
    for geom, (stride, _, _) in GEOMETRIES.items():
        for cout in COUTS:
            for cin in CINS:
                if cin < SELECTOR_MIN_CIN:
                    if stride == 1:
                        out += [('fwd_wino', geom, cin, cout, act) for act in ('linear', 'relu')]
                    else:
                        out.append(('fwd', geom, cin, cout, 'linear'))
                    continue
                out += [('fwd', geom, cin, cout, act) for act in FWD_ACTS]
                out += [('fwd_dropout', geom, cin, cout, act) for act in ('leaky', 'sigmoid')]
                out.append(('fwd_stats', geom, cin, cout, 'linear'))
                out += [('dgrad', geom, cin, cout, p) for p in DGRAD_PRODUCERS]
    return out


def case_id(case):
    return '-'.join(str(v) for v in case)


def family(case):
    """(direction, family of tests/conv_family.py, stride) the case has to reach."""
    op, geom, cin, _, _ = case
    stride = GEOMETRIES[geom][0]
    direction = 'dgrad' if op == 'dgrad' else 'fwd'
    if op == 'fwd_wino':
        return direction, 'wino', stride
    if cin < SELECTOR_MIN_CIN:
        return direction, 'direct', stride
    return direction, 'wino' if stride == 1 else 'wino_s2', stride


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def inputs(case):
    """The seeded host arrays of a case (a dict; which keys depends on the op)."""
    op, geom, cin, cout, variant = case
    stride, padding, L = GEOMETRIES[geom]
    rng = np.random.RandomState(zlib.crc32(case_id(case).encode()) & 0x7fffffff)
    from gennet_amd import ops
    Lout, pl = ops.conv_geometry(L, 5, stride, padding)
    d = {'stride': stride, 'L': L, 'Lout': Lout, 'pl': pl}
    if op != 'dgrad':
        d['x'] = _f32(rng.randn(B, L, cin))
        d['w'] = _f32(rng.randn(5, cin, cout) * 0.05)
        d['b'] = _f32(rng.randn(cout))
        if op == 'fwd_dropout':
            d['mask'] = (rng.rand(B, Lout, cout) >= RATE).astype(np.uint8)
        return d
    # the layer of this data gradient maps Cout -> Cin channels: dy has Cin channels, dx and the producer's output have Cout
    d['dy'] = _f32(rng.randn(B, Lout, cin))
    d['w'] = _f32(rng.randn(5, cout, cin) * 0.05)
    pre = _f32(rng.randn(B, L, cout))
    if variant == 'relu':
        d['y_prev'] = np.maximum(pre, np.float32(0))
    elif variant == 'tanh':
        d['y_prev'] = np.tanh(pre)
    elif variant == 'leaky_dropout':
        keep = (rng.rand(B, L, cout) >= RATE).astype(np.uint8)
        d['mask'] = keep
        d['y_prev'] = _f32(np.where(pre > 0, pre, np.float32(LEAK) * pre) * keep / np.float32(1.0 - RATE))
    return d


def run(case, d, dev, place=None):
    """Runs the case on the library of this tree: -> the list of output tensors.  place(name, tensor) -> tensor lets a test move an input (a
    misaligned view of y_prev or of the mask); by default every input is a fresh allocation."""
    import torch
    from gennet_amd import ops
    op, geom, cin, cout, variant = case

    def g(name):
        t = torch.tensor(d[name], device=dev)
        return place(name, t) if place else t

    s, L, Lout, pl = d['stride'], d['L'], d['Lout'], d['pl']
    if op == 'fwd':
        return [ops.conv1d_fwd(g('x'), g('w'), g('b'), s, pl, Lout, variant, LEAK)]
    if op == 'fwd_wino':
        return [ops.conv1d_fwd_wino(g('x'), g('w'), g('b'), pl, Lout, variant, LEAK)]
    if op == 'fwd_dropout':
        return [ops.conv1d_fwd_dropout(g('x'), g('w'), g('b'), g('mask'), s, pl, Lout, variant, LEAK, RATE)]
    if op == 'fwd_stats':
        return list(ops.conv1d_fwd_stats(g('x'), g('w'), g('b'), s, pl, Lout))
    wt = ops.conv1d_transpose_w(g('w'))
    prev = None
    if variant in ('relu', 'tanh'):
        prev = (g('y_prev'), variant, 0.0, None, 0.0)
    elif variant == 'leaky_dropout':
        prev = (g('y_prev'), 'leaky', LEAK, g('mask'), RATE)
    return [ops.conv1d_dgrad(g('dy'), wt, L, s, pl, prev=prev)]


def digest(outs):
    """(SHA-256 hex digest of the outputs' bytes in order, the first HEAD values of the first output as float32, zero-padded)."""
    arrs = [o.detach().cpu().numpy() for o in outs]
    h = hashlib.sha256()
    for a in arrs:
        h.update(np.ascontiguousarray(a).tobytes())
    head = np.zeros(HEAD, np.float32)
    flat = arrs[0].reshape(-1)[:HEAD]
    head[:flat.size] = flat
    return h.hexdigest(), head
