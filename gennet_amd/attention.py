"""keras.layers.Attention (tf.keras 2.x layers/dense_attention.py) on the fused fp32 matrix-core kernels of csrc/attention.hip; DESIGN 8u.

The class is part of the gennet_amd.layers name space (gennet_amd.layers.Attention is this class), as every layer is."""
import numpy as np

from . import ops
from .engine import Layer


class Attention(Layer):
    """keras.layers.Attention(use_scale=False, causal=False): dot-product (Luong) attention, called on [query, value] or [query, value, key]
    (key defaults to value): query (B, .., Tq, d), key (B, .., Tk, d), value (B, .., Tk, dv) of rank 3 or more give
    out (B, .., Tq, dv) = softmax_j(scale * query . key^T) . value; the axes between the batch and the last two are folded into the batch (a view),
    so (B, H, T, d) from Reshape + Permute((2, 1, 3)) is multi-head attention.  use_scale adds the trainable scalar weight `scale` (shape (),
    initial 1); causal=True lets position i attend to positions j <= i only.
    One gn_attention_fwd and one gn_attention_bwd: the (Tq, Tk) scores are never written; the tape keeps q, k, v, out and the (B, Tq) log-sum-exp, in
    the training phase only.  The gradient of `scale` is the fixed-order column reduction (ops.bias_grad) of one partial per query row.
    Refused by name: dropout != 0, a mask= call argument, d or dv above ops.ATTENTION_MAX_D.  DESIGN 8u."""
    is_merge = True

    def __init__(self, use_scale=False, causal=False, dropout=0.0, **kw):
        kw.pop('dtype', None)
        Layer.__init__(self, **kw)
        if dropout:
            raise NotImplementedError('Attention(dropout=%r): dropout of the attention scores is not implemented; only dropout=0' % (dropout,))
        self.use_scale, self.causal = bool(use_scale), bool(causal)
        self.scale = None

    def __call__(self, inputs, mask=None, training=None):
        if mask is not None:
            raise NotImplementedError('%s (Attention): the mask= call argument (padding masks) is not implemented; causal=True is' % self.name)
        if not isinstance(inputs, (list, tuple)):
            raise ValueError('Attention layer must be called on a list of inputs, namely [query, value] or [query, value, key].')
        if len(inputs) < 2 or len(inputs) > 3:
            raise ValueError('Attention layer accepts inputs list of length 2 or 3, namely [query, value] or [query, value, key]. Given length: %d' % len(inputs))
        return Layer.__call__(self, inputs)

    def _geometry(self, input_shape):
        """(lead, Tq, Tk, d, dv) for the shapes without the batch axis [query, value(, key)], with the refusals"""
        if not isinstance(input_shape, (list, tuple)) or not all(isinstance(s, (list, tuple)) for s in input_shape) or not 2 <= len(input_shape) <= 3:
            raise ValueError('Attention layer accepts inputs list of length 2 or 3, namely [query, value] or [query, value, key]. Given length: %s'
                             % (len(input_shape) if isinstance(input_shape, (list, tuple)) else 1))
        qs, vs = tuple(input_shape[0]), tuple(input_shape[1])
        ks = tuple(input_shape[2]) if len(input_shape) == 3 else vs
        shown = [(None,) + tuple(s) for s in input_shape]
        if len(qs) < 2 or len(qs) != len(vs) or len(qs) != len(ks):
            raise ValueError('%s (Attention): query, value and key of one rank, 3 or more (the batch axis counted), are expected, got %r' % (self.name, shown))
        if qs[:-2] != vs[:-2] or qs[:-2] != ks[:-2]:
            raise ValueError('%s (Attention): the axes between the batch and the last two must agree, got %r' % (self.name, shown))
        if qs[-1] != ks[-1]:
            raise ValueError('%s (Attention): Dimensions must be equal, but are %s and %s: the last axis of query %r and of key %r'
                             % (self.name, qs[-1], ks[-1], (None,) + qs, (None,) + ks))
        if ks[-2] != vs[-2]:
            raise ValueError('%s (Attention): key %r and value %r must have the same number of positions Tk' % (self.name, (None,) + ks, (None,) + vs))
        d, dv = int(qs[-1]), int(vs[-1])
        if d > ops.ATTENTION_MAX_D or dv > ops.ATTENTION_MAX_D:
            raise NotImplementedError('%s (Attention): d = %d, dv = %d: the kernels hold up to %d features of a row on chip' % (self.name, d, dv, ops.ATTENTION_MAX_D))
        return tuple(int(e) for e in qs[:-2]), int(qs[-2]), int(ks[-2]), d, dv

    def build(self, input_shape):
        self._geometry(input_shape)
        if self.use_scale and self.scale is None:
            self.scale = self.add_weight('scale', np.ones((), np.float32))
        self.built = True

    def compute_output_shape(self, input_shape):
        lead, Tq, _, _, dv = self._geometry(input_shape)
        return lead + (Tq, dv)

    def forward(self, ctx, node, xs):
        lead, Tq, Tk, d, dv = self._geometry([tuple(x.shape[1:]) for x in xs])
        n = xs[0].shape[0] * int(np.prod(lead)) if lead else xs[0].shape[0]
        q = xs[0].contiguous().view(n, Tq, d)
        v = xs[1].contiguous().view(n, Tk, dv)
        k = xs[2].contiguous().view(n, Tk, d) if len(xs) == 3 else v
        scale = self.scale.data.view(1) if self.use_scale else None
        out, lse = ops.attention_fwd(q, k, v, scale, self.causal, training=ctx.training)
        if ctx.training:
            ctx.tape[node.index] = (q, k, v, out, lse, [tuple(x.shape) for x in xs])
        return out.view((xs[0].shape[0],) + tuple(node.out_shape))

    def backward(self, ctx, node, dy, need_dx, need_dw):
        q, k, v, out, lse, shapes = ctx.tape.pop(node.index)
        two = len(shapes) == 2
        need = (need_dx[0], need_dx[1], need_dx[1]) if two else (need_dx[0], need_dx[2], need_dx[1])          # dq, dk, dv
        need_ds = bool(need_dw and self.use_scale)
        scale = self.scale.data.view(1) if self.use_scale else None
        dq, dk, dv, rows = ops.attention_bwd(q, k, v, out, lse, dy.contiguous().view(out.shape), scale, self.causal, need, need_ds)
        if need_ds:
            ops.bias_grad(rows.view(-1, 1), self.scale.grad.view(1))
        if two:
            dval = ops.axpy(dv, dk, 1.0) if need_dx[1] else None          # key is value: its gradient is the sum of both
            res = [dq, dval]
        else:
            res = [dq, dv, dk]
        return [g.view(s) if g is not None else None for g, s in zip(res, shapes)]
