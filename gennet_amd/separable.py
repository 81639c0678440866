"""keras.layers.SeparableConv1D (keras 2.2.4 layers/convolutional.py) on the streaming depthwise kernels of csrc/depthwise.hip and the matrix-core
product the library already has for the pointwise half; DESIGN 8r.

The class is part of the gennet_amd.layers name space (gennet_amd.layers.SeparableConv1D is this class), as every layer is.  It is no Conv1D:
keras_io and the planner ask isinstance(layer, Conv1D) for the dense convolution alone."""
import numpy as np

from . import engine, ops, regularizers
from .engine import Layer
from .recurrent import _initializer_is, rows_product


def _layers():
    """gennet_amd.layers, which imports this module at its foot: its activation helpers are looked up when a layer is made, not at import"""
    from . import layers
    return layers


def _one(v, what):
    """the integer of keras' int-or-1-tuple arguments (kernel_size, strides, dilation_rate)"""
    if isinstance(v, (tuple, list)):
        if len(v) != 1:
            raise ValueError('SeparableConv1D(%s=%r): an integer or a tuple / list of 1 integer' % (what, v))
        v = v[0]
    return int(v)


class SeparableConv1D(Layer):
    """keras.layers.SeparableConv1D(filters, kernel_size): (B, L, Cin) -> (B, Lout, filters).  A depthwise conv of every input channel with its own
    depth_multiplier kernels, then a pointwise (1 x 1) conv that mixes the Cin * depth_multiplier channels:
        t[b, l, c dm + m] = sum_j x[b, l s - pad_left + j d, c] * depthwise_kernel[j, c, m]
        y = act(t . pointwise_kernel[0] + bias)
    Weights in keras' order: depthwise_kernel (k, Cin, dm), pointwise_kernel (1, Cin dm, filters), bias (filters).  padding 'valid' or 'same' (TF's
    rule, ops.conv_geometry); strides > 1 and dilation_rate > 1 exclude each other, as in Conv1D.
    Forward: ops.dwconv1d_fwd, then ONE gn_bmm over the B Lout rows with ops.bias_act_dropout's bias / activation pass behind it (any channel
    pair), and the softmax pass where activation='softmax'.
    Backward: the activation gradient in place from the stored output; dP = t^T dy (recurrent.rows_product: fixed order), dbias the bias-gradient
    reduction, dt = dy . P^T one gn_bmm; then ops.dwconv1d_wgrad(x, dt) and, when wanted, ops.dwconv1d_dgrad(dt).  No atomics.
    The tape keeps x, t and (where the activation is not linear) y, in the training phase only.  The planner fuses nothing onto the layer."""

    def __init__(self, filters, kernel_size, strides=1, padding='valid', data_format=None, dilation_rate=1, depth_multiplier=1, activation=None,
                 use_bias=True, depthwise_initializer='glorot_uniform', pointwise_initializer='glorot_uniform', bias_initializer='zeros',
                 depthwise_regularizer=None, pointwise_regularizer=None, bias_regularizer=None, activity_regularizer=None, depthwise_constraint=None,
                 pointwise_constraint=None, bias_constraint=None, **kw):
        if not use_bias:
            raise NotImplementedError('SeparableConv1D(use_bias=False)')
        if data_format not in (None, 'channels_last'):
            raise NotImplementedError('SeparableConv1D(data_format=%r): only channels_last' % (data_format,))
        for key, v in (('depthwise_constraint', depthwise_constraint), ('pointwise_constraint', pointwise_constraint), ('bias_constraint', bias_constraint)):
            if v is not None:
                raise NotImplementedError('SeparableConv1D(%s=...): weight constraints are not implemented' % key)
        for key, v in (('depthwise_initializer', depthwise_initializer), ('pointwise_initializer', pointwise_initializer)):
            if not _initializer_is(v, 'glorot_uniform', ('GlorotUniform', 'VarianceScaling'), mode='fan_avg', distribution='uniform'):
                raise NotImplementedError('SeparableConv1D(%s=%r): only glorot_uniform' % (key, v))
        if not _initializer_is(bias_initializer, 'zeros', ('Zeros',)):
            raise NotImplementedError('SeparableConv1D(bias_initializer=%r): only zeros' % (bias_initializer,))
        if padding == 'causal':
            raise NotImplementedError("SeparableConv1D(padding='causal'): keras 2.2.4 has no causal separable convolution")
        if padding not in ('same', 'valid'):
            raise ValueError("SeparableConv1D(padding=%r): 'valid' or 'same'" % (padding,))
        Layer.__init__(self, **kw)
        self.filters = int(filters)
        self.k, self.stride, self.dilation = _one(kernel_size, 'kernel_size'), _one(strides, 'strides'), _one(dilation_rate, 'dilation_rate')
        self.depth_multiplier = int(depth_multiplier)
        if self.filters < 1 or self.k < 1 or self.stride < 1 or self.dilation < 1:
            raise ValueError('SeparableConv1D(filters=%r, kernel_size=%r, strides=%r, dilation_rate=%r): each at least 1'
                             % (filters, kernel_size, strides, dilation_rate))
        if self.depth_multiplier < 1:
            raise ValueError('SeparableConv1D(depth_multiplier=%r): at least 1' % (depth_multiplier,))
        if self.dilation > 1 and self.stride > 1:
            raise ValueError('SeparableConv1D(strides=%d, dilation_rate=%d): strides > 1 and dilation_rate > 1 exclude each other (as in Keras)'
                             % (self.stride, self.dilation))
        self.padding = padding
        self.activation = _layers()._act_spec(activation, 'SeparableConv1D')
        self.depthwise_regularizer, self.pointwise_regularizer = regularizers.get(depthwise_regularizer), regularizers.get(pointwise_regularizer)
        self.bias_regularizer, self.activity_regularizer = regularizers.get(bias_regularizer), regularizers.get(activity_regularizer)

    def _geometry(self, input_shape):
        if len(input_shape) != 2:
            raise ValueError('%s (SeparableConv1D) expects (batch, steps, channels), got %r' % (self.name, (None,) + tuple(input_shape)))
        L = int(input_shape[0])
        Lout = ops.conv_geometry(L, self.k, self.stride, self.padding, self.dilation)[0]
        if Lout < 1:
            raise ValueError('SeparableConv1D(kernel_size=%d, dilation_rate=%d, padding=%r) on an input of shape %r: the output would have %d rows'
                             % (self.k, self.dilation, self.padding, tuple(input_shape), Lout))
        return Lout

    def build(self, input_shape):
        self._geometry(input_shape)
        Cin, dm = int(input_shape[1]), self.depth_multiplier
        self.depthwise_kernel = self.add_weight('depthwise_kernel', engine.glorot_uniform((self.k, Cin, dm)), regularizer=self.depthwise_regularizer)
        self.pointwise_kernel = self.add_weight('pointwise_kernel', engine.glorot_uniform((1, Cin * dm, self.filters)),
                                                regularizer=self.pointwise_regularizer)
        self.bias = self.add_weight('bias', np.zeros(self.filters, np.float32), regularizer=self.bias_regularizer)

    def compute_output_shape(self, input_shape):
        return (self._geometry(input_shape), self.filters)

    def forward(self, ctx, node, x):
        L_ = _layers()
        x = x.contiguous()
        B = x.shape[0]
        Cm, F = self.pointwise_kernel.shape[1], self.filters
        t = ops.dwconv1d_fwd(x, self.depthwise_kernel.data, self.stride, self.padding, self.dilation)
        rows = B * t.shape[1]
        y = ops.bmm(t.view(1, rows, Cm), self.pointwise_kernel.data.view(1, Cm, F)).view(B, t.shape[1], F)
        a = self.activation
        ka = L_._kernel_act(a)
        ops.bias_act_dropout(y, self.bias.data, ka[0], ka[1])
        if a is L_._SOFTMAX:
            y = L_._channel_softmax(self, y)
        if ctx.training:
            ctx.tape[node.index] = (x, t, y if a[0] != 'linear' else None)
        return y

    def writes_dy(self, node):
        return self.activation[0] != 'linear'

    def backward(self, ctx, node, dy, need_dx, need_dw):
        x, t, y = ctx.tape.pop(node.index)
        B, Lout, Cm = t.shape
        F, rows = self.filters, B * Lout
        dy = _layers()._conv_bwd_epilogue(dy.contiguous().view(B, Lout, F), y, self.activation, None, 0.0, ctx, node)
        dy2 = dy.view(rows, F)
        P = self.pointwise_kernel
        if need_dw:
            rows_product(t.view(rows, Cm), dy2, P.grad.view(Cm, F))
            ops.bias_grad(dy2, self.bias.grad)
        if not (need_dw or need_dx):
            return None
        dt = ops.bmm(dy2.view(1, rows, F), P.data.view(1, Cm, F), trans_b=True).view(B, Lout, Cm)
        if need_dw:
            ops.dwconv1d_wgrad(x, dt, self.k, self.stride, self.padding, self.dilation, dw=self.depthwise_kernel.grad)
        if not need_dx:
            return None
        return ops.dwconv1d_dgrad(dt, self.depthwise_kernel.data, x.shape[1], self.stride, self.padding, self.dilation)
