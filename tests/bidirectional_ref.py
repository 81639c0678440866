"""keras 2.2.4 layers/wrappers.py Bidirectional, restated in fp64 on tests/lstm_ref.py and tests/gru_ref.py: the forward copy runs the inner layer's
go_backwards, the backward copy its negation; with return_sequences the backward half is flipped along time (K.reverse(y_rev, 1)); then the halves
are merged: 'concat' along the last axis, 'sum', 'mul', 'ave' = (y + y_rev) / 2.  A numpy version, and a torch version autograd runs through."""
import numpy as np

import gru_ref
import lstm_ref

MERGE_MODES = ('concat', 'sum', 'mul', 'ave')


def merge(y, y_rev, merge_mode, return_sequences, cat=None):
    """y, y_rev: the two halves in their processing order, (B, T, u) or (B, u); numpy arrays, or torch tensors with cat=torch.cat"""
    if return_sequences:
        y_rev = y_rev.flip(1) if cat is not None else y_rev[:, ::-1]
    if merge_mode == 'concat':
        return cat([y, y_rev], -1) if cat is not None else np.concatenate([y, y_rev], -1)
    if merge_mode == 'sum':
        return y + y_rev
    if merge_mode == 'mul':
        return y * y_rev
    if merge_mode == 'ave':
        return (y + y_rev) / 2
    raise ValueError(merge_mode)


def _halves(module, cell, x, weights, kw):
    """the two inner forwards: weights = the six arrays in keras' order; kw = the inner layer's keywords with its go_backwards"""
    out = []
    for d in range(2):
        W, U, b = weights[3 * d:3 * d + 3]
        k = dict(kw, go_backwards=bool(kw.get('go_backwards', False)) != bool(d))
        if cell == 'lstm':
            out.append(module(x, W, U, b, None, None, **k))
        elif k.get('reset_after'):
            out.append(module(x, W, U, b[0], b[1], None, **k))
        else:
            out.append(module(x, W, U, b, None, None, **k))
    return out


def forward(cell, x, weights, merge_mode='concat', **kw):
    """numpy fp64: cell 'lstm' | 'gru'; kw: activation, recurrent_activation, return_sequences, go_backwards (and reset_after for 'gru', whose
    bias is then (2, 3u))"""
    ref = lstm_ref if cell == 'lstm' else gru_ref
    (y, _), (y_rev, _) = _halves(ref.forward, cell, np.asarray(x, np.float64), [np.asarray(w, np.float64) for w in weights], kw)
    return merge(y, y_rev, merge_mode, kw.get('return_sequences', False))


def torch_forward(cell, x, weights, merge_mode='concat', **kw):
    """the same on torch tensors (fp64 for the gradients)"""
    import torch
    ref = lstm_ref if cell == 'lstm' else gru_ref
    y, y_rev = _halves(ref.torch_forward, cell, x, weights, kw)
    return merge(y, y_rev, merge_mode, kw.get('return_sequences', False), cat=torch.cat)
