"""keras.layers.TimeDistributed (over Dense), RepeatVector, Permute, Cropping1D and ZeroPadding1D (keras 2.2.4 layers/wrappers.py, core.py and
convolutional.py) on the memory-bound passes of csrc/sequence.hip; DESIGN 8t.

The classes are part of the gennet_amd.layers name space (gennet_amd.layers.Permute is this Permute), as every layer is."""
import numpy as np

from . import ops
from .engine import Layer


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def _pair_arg(what, key, v):
    """(left, right) of keras' int-or-pair argument (conv_utils.normalize_tuple), both >= 0"""
    pair = (v, v) if _is_int(v) else tuple(v) if isinstance(v, (tuple, list)) else None
    if pair is None or len(pair) != 2 or not all(_is_int(p) for p in pair):
        raise ValueError('%s(%s=%r): an integer or a pair of integers' % (what, key, v))
    if min(pair) < 0:
        raise ValueError('%s(%s=%r): must be >= 0' % (what, key, v))
    return int(pair[0]), int(pair[1])


def _sequence_shape(layer, input_shape):
    if len(input_shape) != 2:
        raise ValueError('%s (%s) expects (batch, steps, features), got %r' % (layer.name, type(layer).__name__, (None,) + tuple(input_shape)))
    return int(input_shape[0]), int(input_shape[1])


class TimeDistributed(Layer):
    """keras.layers.TimeDistributed(Dense(...)) on an input of rank 3 or more: the inner Dense on the last axis, which is what the bare Dense
    computes on that input (Dense.per_position), launch for launch and bit for bit.  The wrapper holds the two weights under keras' names,
    <wrapper name>/kernel:0 and /bias:0, with the inner layer's regularizers; `trainable` is the inner layer's flag, as keras' Wrapper has it.
    Any other inner class is refused: folding the batch of a whole layer graph is not implemented."""

    def __init__(self, layer, **kw):
        from .layers import Dense
        if not isinstance(layer, Layer):
            raise ValueError('Please initialize `TimeDistributed` layer with a `Layer` instance. You passed: %r' % (layer,))
        if not isinstance(layer, Dense):
            raise NotImplementedError('TimeDistributed(%s): only TimeDistributed(Dense(...)) is implemented; a wrapper that folds the time axis of '
                                      'any other layer into the batch is not' % type(layer).__name__)
        if layer.built:
            raise ValueError('TimeDistributed(layer=%s): the inner layer is already built; the wrapper owns its weights' % layer.name)
        if kw.pop('weights', None) is not None:
            raise NotImplementedError('TimeDistributed(weights=...): initial weights through the constructor are not implemented; use set_weights')
        self.layer = layer
        trainable = bool(kw.pop('trainable', True)) and bool(layer.trainable)
        Layer.__init__(self, **kw)
        self.trainable = trainable

    @property
    def trainable(self):
        return self.layer.trainable

    @trainable.setter
    def trainable(self, value):
        self.layer.trainable = value

    @property
    def activity_regularizer(self):
        return self.layer.activity_regularizer

    @property
    def units(self):
        return self.layer.units

    def build(self, input_shape):
        if len(input_shape) < 2:
            raise ValueError('%s (TimeDistributed) expects an input of at least 3 dimensions (batch, steps, ...), got %r'
                             % (self.name, (None,) + tuple(input_shape)))
        self.layer.build(tuple(input_shape), owner=self)
        self.layer.built = True

    def compute_output_shape(self, input_shape):
        return self.layer.compute_output_shape(tuple(input_shape))

    def writes_dy(self, node):
        return self.layer.writes_dy(node)

    def forward(self, ctx, node, x):
        return self.layer.forward(ctx, node, x)

    def backward(self, ctx, node, dy, need_dx, need_dw):
        return self.layer.backward(ctx, node, dy, need_dx, need_dw)


class RepeatVector(Layer):
    """keras.layers.RepeatVector(n): (B, C) -> (B, n, C).  The backward sums over n in fp64, in an order fixed by the shape."""

    def __init__(self, n, **kw):
        Layer.__init__(self, **kw)
        if not _is_int(n) or n < 1:
            raise ValueError('RepeatVector(n=%r): a positive integer' % (n,))
        self.n = int(n)

    def compute_output_shape(self, input_shape):
        if len(input_shape) != 1:
            raise ValueError('%s (RepeatVector) expects (batch, features), got %r' % (self.name, (None,) + tuple(input_shape)))
        return (self.n, int(input_shape[0]))

    def forward(self, ctx, node, x):
        return ops.repeat_fwd(x.contiguous(), self.n)

    def backward(self, ctx, node, dy, need_dx, need_dw):
        return ops.repeat_bwd(dy.contiguous().view((dy.shape[0],) + tuple(node.out_shape)))


class Permute(Layer):
    """keras.layers.Permute(dims): dims are 1-based and leave the batch axis where it is; inputs of rank 3 and 4 (batch axis included).  The
    identity permutation moves nothing: the layer then is shape_only, like Reshape."""

    def __init__(self, dims, **kw):
        Layer.__init__(self, **kw)
        if not isinstance(dims, (tuple, list)) or not all(_is_int(d) for d in dims):
            raise ValueError('Permute(dims=%r): a tuple of integers' % (dims,))
        self.dims = tuple(int(d) for d in dims)
        if sorted(self.dims) != list(range(1, len(self.dims) + 1)):
            raise ValueError('Invalid permutation `dims` for Permute Layer: %r. The set of indices in `dims` must be consecutive and start from 1.'
                             % (self.dims,))
        if len(self.dims) not in (2, 3):
            raise NotImplementedError('Permute(dims=%r): inputs of rank 3 and 4 (the batch axis included) are implemented' % (self.dims,))

    @property
    def shape_only(self):
        return self.dims == tuple(range(1, len(self.dims) + 1))

    def compute_output_shape(self, input_shape):
        if len(input_shape) != len(self.dims):
            raise ValueError('%s (Permute(dims=%r)) expects an input of %d dimensions (the batch axis included), got %r'
                             % (self.name, self.dims, len(self.dims) + 1, (None,) + tuple(input_shape)))
        return tuple(int(input_shape[d - 1]) for d in self.dims)

    def forward(self, ctx, node, x):
        if self.shape_only:
            return x
        return ops.permute(x.contiguous(), (0,) + self.dims)

    def backward(self, ctx, node, dy, need_dx, need_dw):
        if self.shape_only:
            return dy
        inverse = [0] * (len(self.dims) + 1)
        for i, d in enumerate(self.dims):
            inverse[d] = i + 1
        return ops.permute(dy.contiguous().view((dy.shape[0],) + tuple(node.out_shape)), inverse)


class ZeroPadding1D(Layer):
    """keras.layers.ZeroPadding1D(padding=1): (B, L, C) -> (B, left + L + right, C), the new rows +0."""

    def __init__(self, padding=1, **kw):
        Layer.__init__(self, **kw)
        self.padding = _pair_arg('ZeroPadding1D', 'padding', padding)

    def compute_output_shape(self, input_shape):
        L, C = _sequence_shape(self, input_shape)
        return (self.padding[0] + L + self.padding[1], C)

    def forward(self, ctx, node, x):
        return ops.shift1d(x.contiguous(), self.padding[0], x.shape[1] + sum(self.padding))

    def backward(self, ctx, node, dy, need_dx, need_dw):
        Lout = node.out_shape[0]
        return ops.shift1d(dy.contiguous().view((dy.shape[0],) + tuple(node.out_shape)), -self.padding[0], Lout - sum(self.padding))


class Cropping1D(Layer):
    """keras.layers.Cropping1D(cropping=(1, 1)): (B, L, C) -> (B, L - left - right, C); the backward pads the gradient with +0."""

    def __init__(self, cropping=(1, 1), **kw):
        Layer.__init__(self, **kw)
        self.cropping = _pair_arg('Cropping1D', 'cropping', cropping)

    def compute_output_shape(self, input_shape):
        L, C = _sequence_shape(self, input_shape)
        if L - sum(self.cropping) < 1:
            raise ValueError('%s (Cropping1D(cropping=%r)) on an input of %d steps: no sample is left' % (self.name, self.cropping, L))
        return (L - sum(self.cropping), C)

    def forward(self, ctx, node, x):
        return ops.shift1d(x.contiguous(), -self.cropping[0], x.shape[1] - sum(self.cropping))

    def backward(self, ctx, node, dy, need_dx, need_dw):
        Lout = node.out_shape[0]
        return ops.shift1d(dy.contiguous().view((dy.shape[0],) + tuple(node.out_shape)), self.cropping[0], Lout + sum(self.cropping))
