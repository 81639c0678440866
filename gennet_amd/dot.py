"""keras.layers.Dot and keras.layers.dot (keras 2.2.4 layers/merge.py) on the batched fp32 matrix-core product of csrc/bmm.hip; DESIGN 8n.

The class is part of the gennet_amd.layers name space (gennet_amd.layers.Dot is this class), as every layer is."""
import numpy as np

from . import ops
from .engine import Layer


class Dot(Layer):
    """keras.layers.Dot(axes, normalize=False): the batched product K.batch_dot(x1, x2, axes) of two inputs of rank 2 or 3 (batch axis counted),
    out[b, i, j] = sum_k x1[b, .., k, ..] * x2[b, .., k, ..] with x1's remaining axis i and x2's remaining axis j; a rank-2 input is its rank-3
    view with a trailing extent of 1, which is squeezed from the result, and a result that has only the batch axis gets a trailing 1.
    `axes` counts the batch axis: an int for both inputs (a negative one modulo each input's rank) or a pair.  normalize=True L2-normalises
    each input along its axis first (K.l2_normalize), so the product is a cosine proximity.
    One gn_bmm forward and one per wanted gradient, dx1 = dy . x2^T and dx2 = x1^T . dy, each written in its input's own layout (only the strides
    change: csrc/bmm.hip); with normalize a gn_l2norm pass per input in front and per gradient behind.  The tape keeps the two operands of the
    product (the normalised ones and their inverse norms under normalize), in the training phase only.  The gradients are fresh tensors: dy is
    not written.  DESIGN 8n."""
    is_merge = True

    def __init__(self, axes, normalize=False, **kw):
        Layer.__init__(self, **kw)

        def is_int(v):
            return isinstance(v, (int, np.integer)) and not isinstance(v, bool)
        if is_int(axes):
            self.axes = int(axes)
        elif isinstance(axes, (list, tuple)) and len(axes) == 2 and all(is_int(v) for v in axes):
            self.axes = (int(axes[0]), int(axes[1]))
        else:
            raise ValueError('Dot(axes=%r): an integer or a pair of integers' % (axes,))
        if 0 in (self.axes if isinstance(self.axes, tuple) else (self.axes,)):
            raise ValueError('Dot(axes=%r): axis 0 is the batch axis; a product across the samples of a batch is refused' % (axes,))
        self.normalize = bool(normalize)

    def __call__(self, x):
        if not isinstance(x, (list, tuple)) or len(x) != 2:
            raise ValueError('A `Dot` layer should be called on exactly 2 inputs')
        return Layer.__call__(self, x)

    def _geometry(self, input_shape):
        """((d1, d2), axis) of each input's rank-3 view (without the batch extent; axis 1 or 2 of the view, batch counted) for the shapes without
        the batch axis, with keras' refusals."""
        if not isinstance(input_shape, (list, tuple)) or len(input_shape) != 2 or not all(isinstance(s, (list, tuple)) for s in input_shape):
            raise ValueError('A `Dot` layer should be called on exactly 2 inputs')
        shapes = [tuple(s) for s in input_shape]
        ranks = [len(s) + 1 for s in shapes]
        for s, r in zip(shapes, ranks):
            if r > 3:
                raise NotImplementedError('%s (Dot): an input of rank %d, shape %r: inputs of rank 2 or 3 (the batch axis counted) are multiplied'
                                          % (self.name, r, (None,) + s))
        axes = [self.axes % r for r in ranks] if isinstance(self.axes, int) and self.axes < 0 else \
            [self.axes] * 2 if isinstance(self.axes, int) else list(self.axes)
        for ax, s, r in zip(axes, shapes, ranks):
            if not 1 <= ax < r:
                raise ValueError('%s (Dot): axes=%r on an input of shape %r: its axis must be one of 1 .. %d (0 is the batch axis)'
                                 % (self.name, self.axes, (None,) + s, r - 1))
        if shapes[0][axes[0] - 1] != shapes[1][axes[1] - 1]:
            raise ValueError('%s (Dot): Dimension incompatibility %s != %s. Layer shapes: %r, %r'
                             % (self.name, shapes[0][axes[0] - 1], shapes[1][axes[1] - 1], (None,) + shapes[0], (None,) + shapes[1]))
        return [((int(s[0]), int(s[1]) if len(s) == 2 else 1), ax) for s, ax in zip(shapes, axes)]

    def compute_output_shape(self, input_shape):
        geo = self._geometry(input_shape)
        out = tuple(d[2 - ax] for (d, ax), s in zip(geo, input_shape) if len(s) == 2)      # each rank-3 input's remaining axis
        return out if out else (1,)

    def forward(self, ctx, node, xs):
        (d1, ax1), (d2, ax2) = self._geometry([tuple(x.shape[1:]) for x in xs])
        B = xs[0].shape[0]
        a, b = xs[0].contiguous().view((B,) + d1), xs[1].contiguous().view((B,) + d2)
        inv = None
        if self.normalize:
            va, vb = self._norm_view(B, d1, ax1), self._norm_view(B, d2, ax2)
            (a, ia), (b, ib) = ops.l2norm_fwd(a, va), ops.l2norm_fwd(b, vb)
            inv = (ia, va, ib, vb)
        if ctx.training:
            ctx.tape[node.index] = (a, b, ax1, ax2, inv, tuple(xs[0].shape), tuple(xs[1].shape))
        y = ops.bmm(a, b, trans_a=ax1 == 1, trans_b=ax2 == 2)
        return y.view((B,) + tuple(node.out_shape))

    @staticmethod
    def _norm_view(B, d, ax):
        return (B, d[0], d[1]) if ax == 1 else (B * d[0], d[1], 1)

    def backward(self, ctx, node, dy, need_dx, need_dw):
        a, b, ax1, ax2, inv, s1, s2 = ctx.tape.pop(node.index)
        M, N = a.shape[3 - ax1], b.shape[3 - ax2]
        dy = dy.contiguous().view(a.shape[0], M, N)
        dx1 = dx2 = None
        if need_dx[0]:          # dA = dy . B^T as (M, K), or its transpose B . dy^T as (K, M): whichever x1 is stored as
            dx1 = ops.bmm(dy, b, trans_b=ax2 == 1) if ax1 == 2 else ops.bmm(b, dy, trans_a=ax2 == 2, trans_b=True)
            if inv is not None:
                dx1 = ops.l2norm_bwd(dx1, a, inv[0], inv[1])
            dx1 = dx1.view(s1)
        if need_dx[1]:          # dB = A^T . dy as (K, N), or dy^T . A as (N, K)
            dx2 = ops.bmm(a, dy, trans_a=ax1 == 2) if ax2 == 1 else ops.bmm(dy, a, trans_a=True, trans_b=ax1 == 1)
            if inv is not None:
                dx2 = ops.l2norm_bwd(dx2, b, inv[2], inv[3])
            dx2 = dx2.view(s2)
        return [dx1, dx2]


def dot(inputs, axes, normalize=False, **kw):
    return Dot(axes=axes, normalize=normalize, **kw)(inputs)
