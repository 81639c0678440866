"""Keras-style layers used by BBH_version/bbhMahoGANy.py, executing on the HIP kernel library (gennet_amd.ops).

Layer list and defaults follow bbhMahoGANy.py:33-40 and SURVEY Appendix B: channels_last, glorot_uniform kernels, zero
biases, BatchNormalization(axis=-1, epsilon=1e-3, gamma=1, beta=0, moving_mean=0, moving_variance=1).
Layers that the reference imports but never places on the hot path are not provided; asking for an unsupported
configuration raises instead of silently running something else.
"""
import collections

import numpy as np
import torch

from . import ops, regularizers
from .engine import Layer, Model, capturing, device, device_rng, glorot_uniform

import os as _os
_NO_DROPGEN = bool(_os.environ.get('GN_NO_DROPGEN'))      # A/B switch: separate dropout-mask kernel instead of drawing it inside bn_apply
_NO_LAZYGRAD = bool(_os.environ.get('GN_NO_LAZYGRAD'))    # A/B switch: materialise the 1-filter conv's data gradient in front of a BatchNormalization
_NO_UPFOLD = bool(_os.environ.get('GN_NO_UPFOLD'))        # A/B switch: materialise UpSampling1D instead of folding it into the conv
_NO_CONVSTATS = bool(_os.environ.get('GN_NO_CONVSTATS'))  # A/B switch: separate BatchNorm statistics pass instead of the conv epilogue

_ACT_NAMES = {'relu': ('relu', 0.0), 'tanh': ('tanh', 0.0), 'sigmoid': ('sigmoid', 0.0), 'linear': ('linear', 0.0), None: ('linear', 0.0)}
# softmax is no entry of ops.ACT: a reduction along an axis, not an epilogue.  A kernel layer with activation='softmax' keeps this spec, launches
# its conv or dense kernel linear (_kernel_act) and runs ops.softmax_fwd over its channels behind it; the planner fuses nothing onto such a layer
# (DESIGN 8k).  A callable of gennet_amd.keras.activations names itself.
_SOFTMAX = ('softmax', 0.0)
_LINEAR = ('linear', 0.0)


def _act_spec(activation, what):
    name = getattr(activation, '__name__', activation) if callable(activation) else activation
    if name == 'softmax':
        return _SOFTMAX
    if name not in _ACT_NAMES:
        raise NotImplementedError('%s(activation=%r): one of relu, tanh, sigmoid, linear, softmax' % (what, activation))
    return _ACT_NAMES[name]


def _activation_name(name):
    def fn(x, *a, **k):
        raise NotImplementedError('gennet_amd.keras.activations.%s is a name for activation=%r; applied to a tensor it has no HIP lowering: use the '
                                  'layer (Activation(%r)%s)' % (name, name, name, ', Softmax(axis)' if name == 'softmax' else ''))
    fn.__name__ = fn.__qualname__ = name
    return fn


ACTIVATIONS = dict((n, _activation_name(n)) for n in ('softmax', 'relu', 'tanh', 'sigmoid', 'linear'))      # gennet_amd.keras.activations


def _kernel_act(a):
    """the epilogue a conv or dense kernel is launched with for the layer activation `a`"""
    return _LINEAR if a is _SOFTMAX else a


def _is_softmax(layer):
    return getattr(layer, 'activation', None) is _SOFTMAX


def _channel_softmax(layer, y):
    """softmax over the channels of a kernel layer's output, in place: the linear tensor is read by nothing else.  In memory the output of every
    conv form (tap-folded, upsample-folded, width-2 Conv2D, Conv2DTranspose, the merged phases) is rows of layer.filters / layer.units floats."""
    P = layer.units if hasattr(layer, 'units') else layer.filters
    return ops.softmax_fwd(y, (y.numel() // P, P, 1), inplace=True)


def _check_init(kernel_initializer):
    if kernel_initializer not in (None, 'glorot_uniform'):
        raise NotImplementedError('kernel_initializer %r (only glorot_uniform is used on the hot path)' % (kernel_initializer,))


def _take_regularizers(layer, kernel, bias, activity):
    """the three regularizer keywords of Dense and the conv layers, through regularizers.get (an L1L2, 'l1' / 'l2' / 'l1_l2', a config dict, None)"""
    layer.kernel_regularizer, layer.bias_regularizer = regularizers.get(kernel), regularizers.get(bias)
    layer.activity_regularizer = regularizers.get(activity)


def _conv_fwd(node, ctx, x, w, b, stride, pl, Lout, act, out_shape_for_mask, any_channels=False, drop_ok=True):
    """conv + activation epilogue, and the one place that decides what becomes of a Dropout the planner fused onto the node: applied in the conv's
    epilogue in the training phase; refused where the layer has none (drop_ok False: a Conv1D with <= 4 filters).  any_channels: the `anyc` kernels
    have no fused Dropout, and none arrives: Conv1D.fusable_drop declined it (Sequential and Model build a layer before they plan it)."""
    if node.fused_drop is not None:
        assert act is not _SOFTMAX, 'a fused Dropout on a softmax layer'
        assert not any_channels, 'a fused Dropout on a channel pair of the any-channel kernels (plan the model after building it)'
        if not drop_ok:
            raise NotImplementedError('Dropout directly after a Conv1D with <= 4 filters')
        if ctx.training and node.fused_drop[0] > 0.0:
            rate, drop_layer = node.fused_drop
            mask = drop_layer.make_mask(ctx, out_shape_for_mask)
            return ops.conv1d_fwd_dropout(x, w, b, mask, stride, pl, Lout, act[0], act[1], rate), mask, rate
    act = _kernel_act(act)
    return ops.conv1d_fwd(x, w, b, stride, pl, Lout, act[0], act[1], any_channels=any_channels), None, 0.0


def _conv_bwd_epilogue(dy, y, act, mask, rate, ctx=None, node=None):
    """gradient through [activation -> dropout] expressed through the layer output, in place, one pass -- unless the consumer's
    data-gradient kernel already applied it in its epilogue (engine backward fusion)."""
    if act is _SOFTMAX:                # the softmax gradient first, from the stored output; what follows is the layer's backward with a linear epilogue
        assert mask is None and node.index not in ctx.pre_applied
        P = node.layer.units if hasattr(node.layer, 'units') else node.layer.filters
        return ops.softmax_bwd(dy, y, (dy.numel() // P, P, 1), inplace=True)
    if ctx is not None and node.index in ctx.pre_applied:
        return dy
    if mask is not None:
        return ops.act_dropout_bwd(dy, y, mask, act[0], act[1], rate, inplace=True)
    if act[0] != 'linear':
        return ops.act_bwd(dy, y, act[0], act[1], inplace=True)
    return dy


def _epilogue_writes_dy(layer, node):
    """Layer.writes_dy of the layers whose backward starts with _conv_bwd_epilogue: it overwrites dy unless the epilogue is linear and has no Dropout."""
    a = node.fused_act or layer.activation
    return a[0] != 'linear' or node.fused_drop is not None


# A k-tap conv, 1 <= k <= 40, in its three directions.  More than 5 taps (`filtsize = 5 # 10 is best`, bbhMahoGANy.py:228) run as G = ceil(k/5) groups
# of h = ceil(k/G) taps over the input with its shifted copies as further channel groups and the left padding materialised (csrc/tap_fold.hip): the
# same <= 5-tap matrix-core kernels on 0 padding, the tap groups accumulating in their K loop; gradients come out folded and are unfolded.  Every
# argument is that of the k-tap conv; folded=True: the caller kept that operand in its folded form, and it is not folded again.
def _kconv_fwd(x, w, b, stride, pl, Lout, launch=ops.conv1d_fwd):
    """-> (launch(x, w, b, stride, pl, Lout) on the operands as they are launched, those x and w)"""
    if w.shape[0] > 5:
        x, w, pl = ops.conv1d_tapfold_x(x, w.shape[0], pl), ops.conv1d_tapfold_w(w), 0
    return launch(x, w, b, stride, pl, Lout), x, w


def _kconv_dgrad(dy, w, k, L, stride, pl, prev=None, any_channels=False, folded=False):
    """prev: the producer's [activation -> dropout] backward in the epilogue (ops.conv1d_dgrad), for <= 5 taps"""
    if k <= 5:
        return ops.conv1d_dgrad(dy, ops.conv1d_transpose_w(w), L, stride, pl, prev, any_channels=any_channels)
    assert prev is None
    w2 = w if folded else ops.conv1d_tapfold_w(w)
    return ops.conv1d_tapunfold_dx(ops.conv1d_dgrad(dy, ops.conv1d_transpose_w(w2), L + pl, stride, 0, None, any_channels=any_channels), L, k, pl)


def _kconv_wgrad(x, dy, k, stride, pl, dw=None, db=None, want_db=True, any_channels=False, folded=False):
    """-> (dw, db), written into the given tensors where given"""
    if k <= 5:
        return ops.conv1d_wgrad(x, dy, k, stride, pl, dw, db, want_db, any_channels)
    x2 = x if folded else ops.conv1d_tapfold_x(x, k, pl)
    dw2, db = ops.conv1d_wgrad(x2, dy, ops.tap_groups(k)[1], stride, 0, None, db, want_db, any_channels)
    return ops.conv1d_tapunfold_dw(dw2, k, dw), db


def _launched_pair(k, Cin, Cout, up_folded=False, stride=1):
    """(Cin, Cout) of the conv that is launched for a k-tap Cin -> Cout layer: the tap fold puts its G tap groups side by side as input channels;
    an UpSampling1D folded into a stride-1 layer makes the two output phases its columns."""
    return Cin * ops.tap_groups(k)[0] if k > 5 else Cin, 2 * Cout if up_folded and stride == 1 else Cout


class _ConvRun(object):
    """The conv a Conv1D launches on (L, Cin) inputs, the UpSampling1D in front folded into it (Model._plan: node.fold_up) or not.  Whatever depends
    on what is launched asks this record: the planner and build() one without L (channels only), the forward one that the backward finds on the tape.
      k, stride, pl, Lout    the layer's own conv or, upsample folded, the 3-tap stride-1 conv on the un-upsampled input (ops.conv1d_up2_fold; for
                             stride 1 its (L, 2 * filters) output is the layer's (2L, filters) output in memory)
      tap_folded             k > 5: launched as tap_groups(k)[1] taps on 0 padding over L + pl rows (_kconv_*), gradients unfolded with (L, pl)
      Cin_run, Cout_run      the launched channel pair; fwd_any: only the `anyc` kernels take it (ops.conv_needs_any); any_channels: it or the data
                             gradient's swapped pair -- then no fusion that rests on a strict fused entry point is made
      phase                  None, or (d, pl, L, Lout) of a dilated or causal layer (Conv1D.phased): the conv above then is the layer's
                             k taps on 0 padding over the d phase sequences of the padded input, a (B*d, M, Cin) batch -- L = M, pl = 0,
                             Lout = (M - k) // stride + 1 -- between ops.dilate_split with these (d, pl) and ops.dilate_merge back to (L, Lout) rows"""
    __slots__ = ('L', 'Cin', 'k', 'stride', 'pl', 'Lout', 'tap_folded', 'up_folded', 'Cin_run', 'Cout_run', 'fwd_any', 'any_channels', 'phase')

    def __init__(self, layer, Cin, up_folded, L=None):
        self.L, self.Cin, self.up_folded, self.tap_folded, self.phase = L, Cin, up_folded, layer.k > 5, None
        self.k, self.stride = (3, 1) if up_folded else (layer.k, layer.stride)
        self.Cin_run, self.Cout_run = _launched_pair(layer.k, Cin, layer.filters, up_folded, layer.stride)
        self.fwd_any = ops.conv_needs_any(self.Cin_run, self.Cout_run)
        self.any_channels = self.fwd_any or ops.conv_needs_any(self.Cout_run, self.Cin_run)
        if L is not None and layer.phased:
            assert not up_folded
            d = layer.dilation
            Lout, pl = ops.conv_geometry(L, layer.k, layer.stride, layer.padding, d)
            pr = (layer.k - 1) * d - pl if layer.padding == 'same' else 0
            M = max(-(-(L + pl + pr) // d), layer.k)
            self.phase, self.L, self.pl, self.Lout = (d, pl, L, Lout), M, 0, (M - layer.k) // layer.stride + 1
            return
        self.Lout, self.pl = (None, None) if L is None else (L, 1) if up_folded else ops.conv_geometry(L, layer.k, layer.stride, layer.padding)


def _transpose_pair_ok(k, filters, Cin):
    """Conv2DTranspose runs the adjoint Conv1D (filters -> Cin, tap-folded past 5 taps) on the strict entry points: both channel counts multiples of
    4, or one side <= 4 and the other a multiple of 4.  (Wider than the library's own rule where both sides are <= 4: DESIGN 8c, known gap.)"""
    a, b = _launched_pair(k, filters, Cin)
    return (a % 4 == 0 and b % 4 == 0) or (a <= 4 and b % 4 == 0) or (b <= 4 and a % 4 == 0)


# tape entry of the conv layers: x, y, mask in the shape of the conv that ran, w its kernel; run: Conv1D's record; pl, in_shape: Conv2D, Conv2DTranspose
_ConvTape = collections.namedtuple('_ConvTape', 'x y act mask rate w run pl in_shape', defaults=(None, None, None, None))


class Dense(Layer):
    """bbhMahoGANy.py:234 (100 -> 256*n_pix/2, MFMA GEMM), :377,:399,:494 (flatten -> 1 heads, streaming dot product).

    On an input of rank 3 or more (batch axis included) the layer acts on the last axis, as in keras: kernel (input_shape[-1], units), output
    input_shape[:-1] + (units,).  It then runs as the one-tap Conv1D it is, on the (B, positions, features) view and on that layer's kernels in
    all three directions: their weight gradients split a long row axis, gn_dense_bwd's do not.  The planner's fusions of the
    (batch, features) layer are switched off for such an instance: each was written against the rank-2 entry points."""

    @property
    def per_position(self):
        """built on an input with axes in front of the features: the layer runs on the (B, positions, features) view"""
        return getattr(self, '_per_position', False)

    @property
    def fusable_act(self):
        return not self.per_position

    @property
    def offers_act_bwd(self):
        return not _is_softmax(self) and not self.per_position

    @property
    def can_absorb_prev_act_bwd(self):
        k = getattr(self, 'kernel', None)          # the fused small-output backward needs an input width that is a multiple of 4
        return self.units <= 4 and (k is None or k.shape[0] % 4 == 0) and not self.per_position

    def __init__(self, units, activation=None, kernel_initializer='glorot_uniform', use_bias=True, kernel_regularizer=None, bias_regularizer=None,
                 activity_regularizer=None, **kw):
        Layer.__init__(self, **kw)
        _check_init(kernel_initializer)
        _take_regularizers(self, kernel_regularizer, bias_regularizer, activity_regularizer)
        if not use_bias:
            raise NotImplementedError('Dense(use_bias=False)')
        self.units = int(units)
        self.activation = _act_spec(activation, 'Dense')

    def build(self, input_shape, owner=None):
        """owner: the wrapper (TimeDistributed) that holds the two weights, under its own name, in this layer's place"""
        if len(input_shape) < 1:
            raise ValueError('Dense expects (batch, ..., features), got a tensor without a feature axis')
        self._per_position = len(input_shape) > 1
        owner = self if owner is None else owner
        self.kernel = owner.add_weight('kernel', glorot_uniform((input_shape[-1], self.units)), regularizer=self.kernel_regularizer)
        self.bias = owner.add_weight('bias', np.zeros(self.units, np.float32), regularizer=self.bias_regularizer)

    def compute_output_shape(self, input_shape):
        return tuple(input_shape[:-1]) + (self.units,)

    def _forward_positions(self, ctx, node, x):
        """Conv1D(units, 1) on the (B, positions, features) view: the kernel (features, units) is that layer's (1, features, units) in memory"""
        a = self.activation
        assert node.fused_act is None and node.fused_drop is None and node.fuse_prev < 0, 'a planner fusion on a per-position Dense'
        ka = _kernel_act(a)
        n_in = self.kernel.shape[0]
        x3 = x.contiguous().view(x.shape[0], -1, n_in)
        any_channels = ops.conv_layer_needs_any(n_in, self.units)
        y = ops.conv1d_fwd(x3, self.kernel.data.view(1, n_in, self.units), self.bias.data, 1, 0, x3.shape[1], ka[0], ka[1], any_channels=any_channels)
        if a is _SOFTMAX:
            y = _channel_softmax(self, y)
        if ctx.training:
            ctx.tape[node.index] = (x3, y, a, any_channels, tuple(x.shape))
        return y.view(tuple(x.shape[:-1]) + (self.units,))

    def _backward_positions(self, ctx, node, dy, need_dx, need_dw):
        x3, y, a, any_channels, x_shape = ctx.tape.pop(node.index)
        n_in = self.kernel.shape[0]
        dy = _conv_bwd_epilogue(dy.contiguous().view(y.shape), y, a, None, 0.0, ctx, node)
        if need_dw:
            ops.conv1d_wgrad(x3, dy, 1, 1, 0, self.kernel.grad.view(1, n_in, self.units), self.bias.grad, any_channels=any_channels)
        if not need_dx:
            return None
        wt = ops.conv1d_transpose_w(self.kernel.data.view(1, n_in, self.units))
        return ops.conv1d_dgrad(dy, wt, x3.shape[1], 1, 0, None, any_channels=any_channels).view(x_shape)

    def forward(self, ctx, node, x):
        if self.per_position:
            return self._forward_positions(ctx, node, x)
        a = node.fused_act or self.activation
        ka = _kernel_act(a)
        y = ops.dense_fwd(x, self.kernel.data, self.bias.data, ka[0], ka[1])
        if a is _SOFTMAX:
            y = _channel_softmax(self, y)
        ctx.tape[node.index] = (x, y, a)
        if ctx.training and ka[0] != 'linear':
            ctx.epi[node.index] = (y, a[0], a[1], None, 0.0)
        return y

    def writes_dy(self, node):
        return _epilogue_writes_dy(self, node)

    def backward(self, ctx, node, dy, need_dx, need_dw, prev=None):
        if self.per_position:
            assert prev is None
            return self._backward_positions(ctx, node, dy, need_dx, need_dw)
        x, y, a = ctx.tape.pop(node.index)
        dy = _conv_bwd_epilogue(dy.contiguous(), y, a, None, 0.0, ctx, node)
        if prev is not None:
            ctx.pre_applied.add(node.fuse_prev)
        if need_dw:
            dx, _, _ = ops.dense_bwd(x, self.kernel.data, dy, need_dx, self.kernel.grad, self.bias.grad, prev=prev)
            return dx
        # frozen layer: data gradient only (scratch weight-gradient buffers are not needed on the small-output path)
        dx, _, _ = ops.dense_bwd(x, self.kernel.data, dy, True, prev=prev)
        return dx


class Conv1D(Layer):
    """bbhMahoGANy.py:250-292, :362-394.

    dilation_rate > 1 or padding='causal' (neither is in the reference): the layer is `phased` -- its own k-tap conv on 0 padding over
    the d phase sequences of the zero-padded input (ops.dilate_split), the phases of the output put back in order (ops.dilate_merge).  Such an
    instance runs on the same kernels as the undilated layer of its channel pair and takes part in none of the planner's cross-layer fusions: the
    phase tensor has rows that are no output and is in another order than the tensors around it."""
    fusable_act = True

    @property
    def phased(self):
        return self.dilation > 1 or self.padding == 'causal'

    @property
    def offers_act_bwd(self):
        return not self.phased and not _is_softmax(self)

    @property
    def can_absorb_prev_act_bwd(self):
        return not self.phased

    @property
    def fusable_drop(self):
        """The planner (Model._plan) asks per instance: a channel pair that only the `anyc` kernels take has no fused Dropout, so the Dropout layer
        runs on its own.  Asked before an UpSampling1D fold is decided, so for every 5-tap 'same' layer neither the unfolded nor the folded pair
        may need them, folded or not in the end: declining costs one pass, fusing wrongly an error.
        A built layer with <= 4 filters declines as well: its Dropout runs as a pass of its own."""
        if self.phased:              # the mask would be in the layer's layout, the conv's epilogue in the phase layout
            return False
        if _is_softmax(self):        # the conv's epilogue runs in front of the softmax pass, the Dropout behind it
            return False
        k = getattr(self, 'kernel', None)
        if k is None:
            return True
        if self.filters <= 4:        # the small-Cout kernels have no Dropout epilogue (gn_conv1d_fwd_dropout needs more than 4 columns)
            return False
        return not any(_ConvRun(self, k.shape[1], up).any_channels for up in ((False, True) if self.can_fold_upsample() else (False,)))

    def __init__(self, filters, kernel_size, strides=1, padding='valid', activation=None, kernel_initializer='glorot_uniform', use_bias=True,
                 dilation_rate=1, kernel_regularizer=None, bias_regularizer=None, activity_regularizer=None, **kw):
        Layer.__init__(self, **kw)
        _check_init(kernel_initializer)
        _take_regularizers(self, kernel_regularizer, bias_regularizer, activity_regularizer)
        if not use_bias:
            raise NotImplementedError('Conv1D(use_bias=False)')
        self.filters = int(filters)
        self.k = int(kernel_size[0] if isinstance(kernel_size, (tuple, list)) else kernel_size)
        self.stride = int(strides[0] if isinstance(strides, (tuple, list)) else strides)
        if isinstance(dilation_rate, (tuple, list)):
            if len(dilation_rate) != 1:
                raise ValueError('Conv1D(dilation_rate=%r): an integer or a tuple / list of 1 integer' % (dilation_rate,))
            dilation_rate = dilation_rate[0]
        self.dilation = int(dilation_rate)
        if self.dilation < 1:
            raise ValueError('Conv1D(dilation_rate=%r): must be >= 1' % (dilation_rate,))
        if self.dilation > 1 and self.stride > 1:
            raise ValueError('Conv1D(strides=%d, dilation_rate=%d): strides > 1 and dilation_rate > 1 exclude each other (as in Keras)'
                             % (self.stride, self.dilation))
        if padding not in ('same', 'valid', 'causal'):
            raise NotImplementedError('padding %r' % (padding,))
        self.padding = padding
        self.activation = _act_spec(activation, 'Conv1D')

    def build(self, input_shape):
        L, Cin = input_shape
        if self.stride < 1 or (Cin > 4 and self.stride > 2):
            raise NotImplementedError('Conv1D(strides=%d) on %d input channels: the matrix-core kernels implement strides 1 and 2 '
                                      '(any stride >= 1 runs for <= 4 input channels)' % (self.stride, Cin))
        if not 1 <= self.k <= 40:
            raise NotImplementedError('Conv1D(kernel_size=%d): 1..40 taps (bbhMahoGANy.py:228 names 5 and 10)' % self.k)
        if self.phased:
            Lout = ops.conv_geometry(L, self.k, self.stride, self.padding, self.dilation)[0]
            if Lout < 1:
                raise ValueError('Conv1D(kernel_size=%d, dilation_rate=%d, padding=%r) on an input of shape %r: the output would have %d rows'
                                 % (self.k, self.dilation, self.padding, tuple(input_shape), Lout))
        if self.stride > 2 and _ConvRun(self, Cin, False).fwd_any:      # (its data gradient's phases have unit input stride)
            raise NotImplementedError('Conv1D(%d filters, strides=%d) on %d input channels: strides above 2 run on the small-Cin kernels only, which '
                                      'need a multiple of 4 filters; the any-channel kernels implement strides 1 and 2'
                                      % (self.filters, self.stride, Cin))
        self.kernel = self.add_weight('kernel', glorot_uniform((self.k, Cin, self.filters)), regularizer=self.kernel_regularizer)
        self.bias = self.add_weight('bias', np.zeros(self.filters, np.float32), regularizer=self.bias_regularizer)

    def compute_output_shape(self, input_shape):
        return (ops.conv_geometry(input_shape[0], self.k, self.stride, self.padding, self.dilation)[0], self.filters)

    @property
    def can_fold_bn(self):
        return self.activation[0] == 'linear' and self.filters % 4 == 0 and self.filters > 4 and not self.phased

    def can_defer_dgrad(self, Cin):
        """1 filter, stride 1: a BatchNormalization producer can form this layer's data gradient inside its own backward passes."""
        return (self.filters == 1 and self.stride == 1 and self.k <= 5 and Cin % 4 == 0 and not self.phased and not _is_softmax(self)
                and not _NO_LAZYGRAD)

    def can_fold_upsample(self):
        """UpSampling1D(2) in front folds into the weights (ops.conv1d_up2_fold): the engine's planner asks."""
        return self.k == 5 and self.padding == 'same' and self.stride in (1, 2) and not self.phased and not _NO_UPFOLD

    def _launch(self, run, x, w, b, launch):
        """`launch` (_kconv_fwd) on the operands of the conv that runs: tap-folded (k > 5), or the kernel with the upsample folded in (k == 5)"""
        if run.up_folded:
            w, b = ops.conv1d_up2_fold(w, b, self.stride)
        return _kconv_fwd(x, w, b, run.stride, run.pl, run.Lout, launch)

    def forward(self, ctx, node, x):
        a = node.fused_act or self.activation
        B = x.shape[0]
        run = _ConvRun(self, x.shape[2], node.fold_up is not None, x.shape[1])
        if run.phase is not None:
            # dilated or causal: the k taps on 0 padding over the phase sequences, bias and activation in that conv's epilogue (elementwise: they
            # commute with the permutation), the output's phases merged back.  d == 1 (causal): the split only pads, the conv's output is y.
            assert node.fused_drop is None and node.infer_bn is None and node.fold_up is None, 'a planner fusion on a dilated or causal Conv1D'
            d, pl, _, Lout = run.phase
            xs = ops.dilate_split(x, d, pl, run.L)
            (ys, _, _), xs, w = self._launch(run, xs, self.kernel.data, self.bias.data, lambda *conv: _conv_fwd(
                node, ctx, *conv, a, None, run.any_channels))
            y = ops.dilate_merge(ys, B, d, 0, Lout) if d > 1 else ys
            if a is _SOFTMAX:          # over the channels of the layer's own rows, the surplus rows of the phase tensor gone
                y = _channel_softmax(self, y)
            ctx.tape[node.index] = _ConvTape(xs, y, a, None, 0.0, w, run)
            return y
        bn_node = None if run.any_channels else node.infer_bn
        if not ctx.training and bn_node is not None and run.Cin > 4:
            # inference phase: the following BatchNormalization (moving statistics) folds into the layer's own kernel, its activation into the
            # epilogue: one kernel, and the pre-BN tensor is never written (generator.predict, bbhMahoGANy.py:1248).  (Asks for the layer's own
            # Cin > 4, the statistics below for the launched one: they differ for a tap-folded layer on <= 4 channels, as they always have.)
            bn = bn_node.layer
            scale, shift = ops.bn_infer_coeffs(bn.gamma.data, bn.beta.data, bn.moving_mean.data, bn.moving_variance.data, bn.epsilon)
            w, b = ops.conv_fold_bn(self.kernel.data, self.bias.data, scale, shift)
            act = bn_node.fused_act or ('linear', 0.0)
            ctx.skip.add(bn_node.index)
            return self._launch(run, x, w, b, lambda *conv: ops.conv1d_fwd(*conv, act[0], act[1]))[0].view(B, -1, self.filters)
        if ctx.training and bn_node is not None and run.Cin_run > 4 and run.Cout_run == self.filters and not _NO_CONVSTATS:
            # training phase, linear conv whose only consumer is a BatchNormalization: its batch statistics come out of the conv kernel's
            # epilogue (no separate pass over the output); the BN node picks them up from ctx.bn_sums.  (Not for the two-phase folded
            # form, whose columns are (phase, channel): that BN layer runs its own statistics pass.)
            (y, sums), x, w = self._launch(run, x, self.kernel.data, self.bias.data, ops.conv1d_fwd_stats)
            ctx.bn_sums[bn_node.index] = sums
            ctx.tape[node.index] = _ConvTape(x, y, a, None, 0.0, w, run)
            return y
        (y, mask, rate), x, w = self._launch(run, x, self.kernel.data, self.bias.data, lambda *conv: _conv_fwd(
            node, ctx, *conv, a, (B, run.Lout, run.Cout_run), run.any_channels, self.filters > 4))
        if a is _SOFTMAX:
            y = _channel_softmax(self, y)
        ctx.tape[node.index] = _ConvTape(x, y, a, mask, rate, w, run)
        y = y.view(B, -1, self.filters)
        if ctx.training and (_kernel_act(a)[0] != 'linear' or mask is not None):
            ctx.epi[node.index] = (y, a[0], a[1], None if mask is None else mask.view(y.shape), rate)
        return y

    def writes_dy(self, node):
        return _epilogue_writes_dy(self, node)

    def backward(self, ctx, node, dy, need_dx, need_dw, prev=None):
        t = ctx.tape.pop(node.index)
        run = t.run
        dy = _conv_bwd_epilogue(dy.contiguous().view(t.y.shape), t.y, t.act, t.mask, t.rate, ctx, node)
        if run.phase is not None:
            # the activation gradient above ran in the layer's own layout; the phases of dy (their surplus rows +0: they add nothing to dw and db)
            # go through the undilated conv's two gradients, and the data gradient's phases merge back behind the pl padding rows
            d, pl, L, _ = run.phase
            dys = ops.dilate_split(dy, d, 0, run.Lout) if d > 1 else dy
            if need_dw:
                _kconv_wgrad(t.x, dys, run.k, run.stride, 0, self.kernel.grad, self.bias.grad, any_channels=run.any_channels, folded=True)
            if not need_dx:
                return None
            dxs = _kconv_dgrad(dys, t.w, run.k, run.L, run.stride, 0, None, run.any_channels, folded=True)
            return ops.dilate_merge(dxs, dy.shape[0], d, pl, L)
        if need_dw:         # t.x, t.w: as the forward launched them, folds included
            if run.up_folded:
                dwf, dbf = _kconv_wgrad(t.x, dy, run.k, run.stride, run.pl, any_channels=run.any_channels)
                ops.conv1d_up2_unfold_grad(dwf, dbf, self.filters, self.stride, self.kernel.grad, self.bias.grad)
            else:
                _kconv_wgrad(t.x, dy, run.k, run.stride, run.pl, self.kernel.grad, self.bias.grad, any_channels=run.any_channels, folded=True)
        if not need_dx:
            return None
        if prev is not None and not run.tap_folded and ops.can_fuse_dgrad(run.Cin_run, run.Cout_run):
            ctx.pre_applied.add(node.fuse_prev)
        else:
            prev = None
        if node.lazy_bn >= 0:
            # 1 filter, stride 1, and the input comes straight from a BatchNormalization: that layer's backward passes form this
            # data gradient on the fly (ops.ConvGrad1); the (B, L, Cin) tensor is neither written here nor read there
            return ops.ConvGrad1(dy, self.kernel.data, run.L, run.pl)
        return _kconv_dgrad(dy, t.w, run.k, run.L, run.stride, run.pl, prev, run.any_channels, folded=True)


class Conv2D(Layer):
    """bbhMahoGANy.py:439,:447: Conv2D(C, (5,5), strides=(2,1), padding='same') on a width-2 image (n, 2, Cin).
    Executed as the exactly equivalent Conv1D over H with (w,c)-interleaved channels; the dead
    width taps kw in {0,4} receive zero gradient, as they do in the reference."""
    fusable_act = True
    can_absorb_prev_act_bwd = True

    @property
    def fusable_drop(self):
        """the launched conv has 2 * filters columns, and the fused Dropout epilogue needs more than 4 (gn_conv1d_fwd_dropout)"""
        return not _is_softmax(self) and self.filters > 2

    @property
    def offers_act_bwd(self):
        return not _is_softmax(self)

    def __init__(self, filters, kernel_size, strides=(1, 1), padding='valid', activation=None, kernel_initializer='glorot_uniform', use_bias=True,
                 kernel_regularizer=None, bias_regularizer=None, activity_regularizer=None, **kw):
        Layer.__init__(self, **kw)
        _check_init(kernel_initializer)
        _take_regularizers(self, kernel_regularizer, bias_regularizer, activity_regularizer)
        self.filters = int(filters)
        self.kh, self.kw = (kernel_size, kernel_size) if isinstance(kernel_size, int) else tuple(kernel_size)
        self.sh, self.sw = (strides, strides) if isinstance(strides, int) else tuple(strides)
        self.padding = padding
        self.activation = _act_spec(activation, 'Conv2D')
        if self.kw != 5 or self.sw != 1 or padding != 'same' or not use_bias:
            raise NotImplementedError('Conv2D is implemented for the hot-path case only: kernel (kh,5), strides (sh,1), padding "same", width-2 input')

    def build(self, input_shape):
        H, W, Cin = input_shape
        if W != 2:
            raise NotImplementedError('Conv2D is implemented for width-2 images (got width %d)' % W)
        if ops.conv_layer_needs_any(2 * Cin, 2 * self.filters):
            # the layer runs as a Conv1D over (w, c)-interleaved rows, 2 * Cin -> 2 * filters, on the strict entry points
            raise NotImplementedError('Conv2D(%d filters) on %d input channels: the width-2 layer runs as a %d -> %d channel Conv1D, and the conv '
                                      'kernels it uses need both counts multiples of 4, or one of them <= 4 and the other a multiple of 4'
                                      % (self.filters, Cin, 2 * Cin, 2 * self.filters))
        self.kernel = self.add_weight('kernel', glorot_uniform((self.kh, self.kw, Cin, self.filters)), regularizer=self.kernel_regularizer)
        self.bias = self.add_weight('bias', np.zeros(self.filters, np.float32), regularizer=self.bias_regularizer)

    def compute_output_shape(self, input_shape):
        return (ops.conv_geometry(input_shape[0], self.kh, self.sh, 'same')[0], 2, self.filters)

    def forward(self, ctx, node, x):
        a = node.fused_act or self.activation
        B, H, W, Cin = x.shape
        Lout, pl = ops.conv_geometry(H, self.kh, self.sh, 'same')
        wf, bf = ops.conv2d_w2_fold(self.kernel.data, self.bias.data)
        xf = x.reshape(B, H, 2 * Cin)
        y, mask, rate = _conv_fwd(node, ctx, xf, wf, bf, self.sh, pl, Lout, a, (B, Lout, 2, self.filters))
        if a is _SOFTMAX:
            y = _channel_softmax(self, y)
        ctx.tape[node.index] = _ConvTape(xf, y, a, mask, rate, wf, pl=pl, in_shape=x.shape)
        if ctx.training and (_kernel_act(a)[0] != 'linear' or mask is not None):
            ctx.epi[node.index] = (y, a[0], a[1], mask, rate)
        return y.reshape(B, Lout, 2, self.filters)

    def writes_dy(self, node):
        return _epilogue_writes_dy(self, node)

    def backward(self, ctx, node, dy, need_dx, need_dw, prev=None):
        t = ctx.tape.pop(node.index)
        Cin = t.in_shape[3]
        dy = _conv_bwd_epilogue(dy.contiguous().reshape(t.y.shape), t.y, t.act, t.mask, t.rate, ctx, node)
        if need_dw:
            dwf, dbf = ops.conv1d_wgrad(t.x, dy, self.kh, self.sh, t.pl)
            ops.conv2d_w2_unfold_grad(dwf, dbf, Cin, self.filters, self.kernel.grad, self.bias.grad)
        if need_dx:
            if prev is not None and ops.can_fuse_dgrad(2 * Cin, 2 * self.filters):
                ctx.pre_applied.add(node.fuse_prev)
            else:
                prev = None
            return ops.conv1d_dgrad(dy, ops.conv1d_transpose_w(t.w), t.x.shape[1], self.sh, t.pl, prev).reshape(t.in_shape)
        return None


def _pair(v, what):
    t = (v, v) if isinstance(v, int) else tuple(int(u) for u in v)
    if len(t) != 2:
        raise ValueError('Conv2DTranspose: %s %r is not a pair' % (what, v))
    return t


class Conv2DTranspose(Layer):
    """keras.layers.Conv2DTranspose (keras 2.2.4, channels_last) with kernel (1, kw) and strides (1, s), s in {1, 2}: the layer of the reference's
    g_model.hdf5 and of 2_model_version/*/noise_gan.py.  Rows are independent, so (B, H, W, Cin) runs as B*H sequences of length W.

    TF's conv2d_transpose is the gradient, with respect to its input, of a conv2d over the output length with the same padding rule, and the
    keras kernel (1, kw, filters, Cin) with kh dropped is exactly this project's Conv1D layout (k, Cin=filters, Cout=Cin) of that adjoint conv.
    So the layer runs on the Conv1D kernel families: forward = the adjoint's data gradient plus the bias / activation / dropout pass of
    csrc/conv_transpose.hip; data gradient = the adjoint's forward; weight gradient = the adjoint's weight gradient with the operands swapped;
    more than 5 taps through the tap fold, as Conv1D does."""
    fusable_act = True

    @property
    def fusable_drop(self):
        return not _is_softmax(self)

    def __init__(self, filters, kernel_size, strides=(1, 1), padding='valid', output_padding=None, data_format=None, dilation_rate=(1, 1),
                 activation=None, use_bias=True, kernel_initializer='glorot_uniform', kernel_regularizer=None, bias_regularizer=None,
                 activity_regularizer=None, **kw):
        Layer.__init__(self, **kw)
        _check_init(kernel_initializer)
        _take_regularizers(self, kernel_regularizer, bias_regularizer, activity_regularizer)
        self.filters = int(filters)
        kh, self.k = _pair(kernel_size, 'kernel_size')
        sh, self.stride = _pair(strides, 'strides')
        supported = ('Conv2DTranspose is implemented for kernel (1, kw) with 1 <= kw <= 40, strides (1, 1) or (1, 2), padding "valid" or "same", '
                     'dilation (1, 1), no output_padding, use_bias=True, channels_last')
        if kh != 1 or sh != 1 or self.stride not in (1, 2) or not 1 <= self.k <= 40:
            raise NotImplementedError('%s (got kernel_size %r, strides %r)' % (supported, kernel_size, strides))
        if _pair(dilation_rate, 'dilation_rate') != (1, 1) or output_padding is not None or not use_bias:
            raise NotImplementedError('%s (got dilation_rate %r, output_padding %r, use_bias %r)' % (supported, dilation_rate, output_padding, use_bias))
        if data_format not in (None, 'channels_last'):
            raise NotImplementedError('%s (got data_format %r)' % (supported, data_format))
        if padding not in ('same', 'valid'):
            raise NotImplementedError('%s (got padding %r)' % (supported, padding))
        if self.k < self.stride:
            raise NotImplementedError('Conv2DTranspose(kernel (1, %d), strides (1, %d)): every stride phase needs a tap (kw >= s)' % (self.k, self.stride))
        self.padding = padding
        self.activation = _act_spec(activation, 'Conv2DTranspose')

    def build(self, input_shape):
        if len(input_shape) != 3:
            raise ValueError('Conv2DTranspose expects (batch, H, W, channels) inputs, got %r' % (tuple(input_shape),))
        if not _transpose_pair_ok(self.k, self.filters, input_shape[2]):
            raise NotImplementedError('Conv2DTranspose(%d filters, kernel (1, %d)) on %d input channels: the conv kernels need both channel counts '
                                      'multiples of 4, or one of them <= 4 and the other a multiple of 4' % (self.filters, self.k, input_shape[2]))
        # keras' layout (1, kw, filters, Cin): glorot limit sqrt(6 / ((filters + Cin) kw)), and .h5 reads / writes are plain copies
        self.kernel = self.add_weight('kernel', glorot_uniform((1, self.k, self.filters, input_shape[2])), regularizer=self.kernel_regularizer)
        self.bias = self.add_weight('bias', np.zeros(self.filters, np.float32), regularizer=self.bias_regularizer)

    def out_length(self, W):
        """keras deconv_length (conv_utils.py) for 'valid' / 'same' without output_padding."""
        return W * self.stride + max(self.k - self.stride, 0) if self.padding == 'valid' else W * self.stride

    def compute_output_shape(self, input_shape):
        return (input_shape[0], self.out_length(input_shape[1]), self.filters)

    def forward(self, ctx, node, x):
        a = node.fused_act or self.activation
        B, H, W, Cin = x.shape
        Wout = self.out_length(W)
        pl = ops.conv_geometry(Wout, self.k, self.stride, self.padding)[1]
        x3 = x.contiguous().view(B * H, W, Cin)
        wadj = self.kernel.data.view(self.k, self.filters, Cin)         # the adjoint Conv1D's kernel (k, Cin=filters, Cout=Cin), no copy
        y = _kconv_dgrad(x3, wadj, self.k, Wout, self.stride, pl)
        mask, rate = None, 0.0
        soft, a = a is _SOFTMAX, _kernel_act(a)            # softmax: the bias pass linear, then the softmax pass over the channels
        if ctx.training and node.fused_drop is not None and node.fused_drop[0] > 0.0:
            rate, drop_layer = node.fused_drop
            if ctx.dropout_masks.get(drop_layer.name) is None and ctx.row_map is None:
                mask = torch.empty(y.shape, dtype=torch.uint8, device=y.device)
                ops.bias_act_dropout(y, self.bias.data, a[0], a[1], mask, rate, gen=device_rng().take(y.numel()))
            else:                          # injected mask, or data parallelism: Dropout's own draw over the layer's (B, H, Wout, filters) shape
                mask = drop_layer.make_mask(ctx, (B, H, Wout, self.filters)).view(y.shape)
                ops.bias_act_dropout(y, self.bias.data, a[0], a[1], mask, rate)
        else:
            ops.bias_act_dropout(y, self.bias.data, a[0], a[1])
        if soft:
            y, a = _channel_softmax(self, y), _SOFTMAX
        ctx.tape[node.index] = _ConvTape(x3, y, a, mask, rate, wadj, pl=pl, in_shape=x.shape)
        y = y.view(B, H, Wout, self.filters)
        if ctx.training and (_kernel_act(a)[0] != 'linear' or mask is not None):
            ctx.epi[node.index] = (y, a[0], a[1], None if mask is None else mask.view(y.shape), rate)
        return y

    def writes_dy(self, node):
        return _epilogue_writes_dy(self, node)

    def backward(self, ctx, node, dy, need_dx, need_dw, prev=None):
        t = ctx.tape.pop(node.index)
        dy = _conv_bwd_epilogue(dy.contiguous().view(t.y.shape), t.y, t.act, t.mask, t.rate, ctx, node)      # (B*H, Wout, filters)
        if need_dw:         # the adjoint's bias: none
            ops.bias_grad(dy.view(-1, self.filters), self.bias.grad)
            _kconv_wgrad(dy, t.x, self.k, self.stride, t.pl, self.kernel.grad.view(t.w.shape), want_db=False)
        if not need_dx:
            return None
        return _kconv_fwd(dy, t.w, None, self.stride, t.pl, t.x.shape[1])[0].view(t.in_shape)


BN_MOVING_AVERAGE = 'tf_zero_debias'       # default form of the moving-statistics update (BatchNormalization docstring)


class BatchNormalization(Layer):
    """bbhMahoGANy.py:235,:251,:260,:268,:276,:284 (momentum=0.99).  Train phase: batch mean / biased variance (fp64
    accumulation), moving statistics updated with keras' n/(n-(1+eps)) variance correction; inference: moving statistics.
    A following Activation and Dropout run in the same pass (one read, one write).  Under data parallelism the
    statistics are all-reduced (SyncBN) so that N ranks x B/N rows reproduce a single-device batch of B.

    axis: keras' axis, counting the batch dimension (1..n-1 or -1..-(n-1) for rank-n inputs).  The last axis (-1 or n-1) is the channel
    BatchNormalization described above.  Any other axis -- BatchNormalization(axis=1) on (B, L, C) in the reference's 2_model_version models: one
    gamma / beta / moving pair per position l, statistics over the batch and the channels -- runs the plain passes of csrc/bn_axis.hip over
    the (outer, P, inner) view with the same finalize, moving-average forms and all-reduce, fuses with nothing, and is no BatchNormalization
    for the planner (is_batchnorm, fusable_act, fusable_drop are per instance).

    moving_average = 'tf_zero_debias' (default) reproduces keras 2.2.4 on its TF 1.12 backend: K.moving_average_update calls
    tf moving_averages.assign_moving_average(x, value, momentum, zero_debias=True), which keeps a zero-initialised `biased` shadow
    accumulator and a `local_step` counter and sets moving = biased / (1 - momentum^local_step): the moving statistics forget their
    0 / 1 initial values at the first update (what generator.predict sees early in training, bbhMahoGANy.py:1248).  TF creates one
    such pair PER CALL SITE of the layer (the generator's layers are called again when the generator is added to another
    Sequential, :517, :537), and only the call site inside the model being trained is updated: the state is therefore kept per
    (layer, training model).  The pairs are not keras weights: real keras never writes them to .h5 files and starts them from zero
    after load_weights; keras_io keeps them in a private section of files written here.
    moving_average = 'ema': the plain exponential average (zero_debias=False; what tf.keras and later keras versions do)."""
    def __init__(self, axis=-1, momentum=0.99, epsilon=1e-3, moving_average=None, beta_regularizer=None, gamma_regularizer=None, **kw):
        Layer.__init__(self, **kw)
        self.beta_regularizer, self.gamma_regularizer = regularizers.get(beta_regularizer), regularizers.get(gamma_regularizer)
        if isinstance(axis, bool) or not isinstance(axis, (int, np.integer)):
            raise NotImplementedError('BatchNormalization(axis=%r): one integer axis' % (axis,))
        self.axis = int(axis)              # keras' axis, counting the batch dimension; written back as given (keras_io)
        self.view = None                   # build: (rows of `outer` per sample, P, inner) of the (outer, P, inner) view, P = the normalised axis
        self.momentum, self.epsilon = float(momentum), float(epsilon)
        self.moving_average = moving_average or BN_MOVING_AVERAGE
        if self.moving_average not in ('tf_zero_debias', 'ema'):
            raise ValueError("BatchNormalization(moving_average=%r): 'tf_zero_debias' or 'ema'" % (moving_average,))
        self.zero_debias = {}              # training-model name -> [biased_mean, biased_var (device fp32), local_step (int)]

    def zero_debias_state(self, site):
        st = self.zero_debias.get(site)
        if st is None:
            C = self.gamma.shape[0]
            st = [torch.zeros(C, dtype=torch.float32, device=device()), torch.zeros(C, dtype=torch.float32, device=device()), 0]
            self.zero_debias[site] = st
        return st

    def build(self, input_shape):
        n = len(input_shape) + 1           # rank with the batch dimension
        if not (1 <= self.axis <= n - 1 or -(n - 1) <= self.axis <= -1):
            raise ValueError('BatchNormalization(axis=%d) on inputs of shape %r: the axis must be one of 1..%d or -1..-%d'
                             % (self.axis, (None,) + tuple(input_shape), n - 1, n - 1))
        k = (self.axis if self.axis > 0 else self.axis + n) - 1
        C = int(input_shape[k])
        self.view = (int(np.prod(input_shape[:k], dtype=np.int64)), C, int(np.prod(input_shape[k + 1:], dtype=np.int64)))
        self._last_axis = k == len(input_shape) - 1
        self.gamma = self.add_weight('gamma', np.ones(C, np.float32), regularizer=self.gamma_regularizer)
        self.beta = self.add_weight('beta', np.zeros(C, np.float32), regularizer=self.beta_regularizer)
        self.moving_mean = self.add_weight('moving_mean', np.zeros(C, np.float32), trainable=False)
        self.moving_variance = self.add_weight('moving_variance', np.ones(C, np.float32), trainable=False)

    @property
    def is_batchnorm(self):
        """A channel (last-axis) BatchNormalization: what the planner and the conv layers fuse with -- activation and Dropout in the apply pass,
        the fold into the producing conv in predict, ctx.bn_sums from its epilogue, the deferred data gradient (lazy_bn).  Over any other axis
        the layer takes part in none of that and runs its plain passes.  (Before build only -1 is known to be the last axis.)"""
        return self._last_axis if self.view is not None else self.axis == -1

    fusable_act = fusable_drop = is_batchnorm

    def _train_coeffs(self, ctx, sums, count):
        """all-reduce of the statistics, finalize and moving-statistics update of the training phase -> (scale, shift, save_mean, save_invstd, count),
        count the number of elements reduced per parameter over all ranks"""
        if ctx.dp is not None:
            ctx.dp.all_reduce_sum(sums)
            count *= ctx.dp.world_size
        zd = None
        if self.moving_average == 'tf_zero_debias':
            st = self.zero_debias_state(ctx.site)
            cap = capturing()
            if cap is None:
                st[2] += 1
                zd = (st[0], st[1], st[2])
            else:                          # captured step graph: local_step advances once per REPLAY and reaches the kernel through device memory

                def next_step(st=st):
                    st[2] += 1
                    return st[2]
                zd = (st[0], st[1], cap.slot('i', next_step))
        return ops.bn_finalize(sums, count, self.gamma.data, self.beta.data, self.epsilon, self.momentum,
                               self.moving_mean.data, self.moving_variance.data, zd) + (count,)

    def _param_grads(self, need_dw):
        if need_dw:
            return self.gamma.grad, self.beta.grad
        return torch.empty_like(self.gamma.data), torch.empty_like(self.beta.data)

    def forward(self, ctx, node, x):
        if not self.is_batchnorm:
            return self._forward_axis(ctx, node, x)
        if node.index in ctx.skip:         # inference phase: already folded into the producing convolution
            return x
        C = x.shape[-1]
        x2 = x.reshape(-1, C)
        act = node.fused_act or ('linear', 0.0)
        if not ctx.training:
            scale, shift = ops.bn_infer_coeffs(self.gamma.data, self.beta.data, self.moving_mean.data, self.moving_variance.data, self.epsilon)
            return ops.bn_apply(x2, scale, shift, None, act[0], act[1]).reshape(x.shape)
        sums = ctx.bn_sums.pop(node.index, None)          # handed over by the producing convolution's epilogue, if it had one
        if sums is None:
            sums = ops.bn_stats(x2)
        scale, shift, smean, sinv, count = self._train_coeffs(ctx, sums, x2.shape[0])
        mask, rate = None, 0.0
        if node.fused_drop is not None and node.fused_drop[0] > 0.0:
            rate, drop_layer = node.fused_drop
            if ctx.dropout_masks.get(drop_layer.name) is None and C % 4 == 0 and not _NO_DROPGEN and (ctx.row_map is None or len(ctx.row_map[0]) == 1):
                # no injected mask: draw it inside the apply pass (same Philox stream as Dropout.make_mask would take; under data parallelism the
                # counters of this rank's rows of the global tensor)
                if ctx.row_map is None:
                    seed, off = device_rng().take(x2.numel())
                else:
                    (g0, nrows), grows = ctx.row_map[0][0], ctx.row_map[1]
                    seed, offs = device_rng().take_rows(x2.numel() // nrows, [(g0, nrows)], grows)
                    off = offs[0]
                y, mask = ops.bn_apply_dropgen(x2, scale, shift, act[0], act[1], rate, seed, off)
                ctx.tape[node.index] = (x2, mask, smean, sinv, count, act, rate, scale, shift)
                return y.reshape(x.shape)
            mask = drop_layer.make_mask(ctx, x2.shape)
        y = ops.bn_apply(x2, scale, shift, mask, act[0], act[1], rate)
        # the backward pass recomputes the activation output from x2 with this scale / shift (bit-identical to y before the
        # dropout scale), so the layer output is not kept for it: 4 of 13 / 17 bytes per element less in its two passes
        ctx.tape[node.index] = (x2, mask, smean, sinv, count, act, rate, scale, shift)
        return y.reshape(x.shape)

    def backward(self, ctx, node, dy, need_dx, need_dw):
        if not self.is_batchnorm:
            return self._backward_axis(ctx, node, dy, need_dw)
        x2, mask, smean, sinv, count, act, rate, scale, shift = ctx.tape.pop(node.index)
        y = None                       # any channel count: the activation output is recomputed from x2 with scale / shift
        lazy = isinstance(dy, ops.ConvGrad1)
        if lazy:
            local = ops.bn_bwd_stats_conv1(dy, x2, mask, smean, sinv, act[0], act[1], rate, scale, shift)
        else:
            dy2 = dy.contiguous().reshape(x2.shape)
            local = ops.bn_bwd_stats(dy2, y, x2, mask, smean, sinv, act[0], act[1], rate, scale, shift)
        glob = local
        if ctx.dp is not None:
            glob = local.clone()
            ctx.dp.all_reduce_sum(glob)
        dgamma, dbeta = self._param_grads(need_dw)
        if lazy:
            dx = ops.bn_bwd_apply_conv1(dy, x2, mask, self.gamma.data, smean, sinv, glob, count, local, dgamma, dbeta, act[0], act[1], rate, scale, shift)
        else:
            dx = ops.bn_bwd_apply(dy2, y, x2, mask, self.gamma.data, smean, sinv, glob, count, local, dgamma, dbeta, act[0], act[1], rate, scale, shift)
        return dx.reshape(dy.shape)

    # -- any axis but the last: the plain sequence statistics -> all-reduce -> finalize -> apply over the (outer, P, inner) view, nothing fused.
    # inner >= 2 runs csrc/bn_axis.hip; inner == 1 is a last-axis layout and runs the column kernels on its (outer, P) view.  By shape alone.
    def _forward_axis(self, ctx, node, x):
        P, inner = self.view[1], self.view[2]
        xv = x.contiguous().reshape((-1, P) if inner == 1 else (-1, P, inner))
        apply_ = ops.bn_apply if inner == 1 else ops.bn_axis_apply
        if not ctx.training:
            scale, shift = ops.bn_infer_coeffs(self.gamma.data, self.beta.data, self.moving_mean.data, self.moving_variance.data, self.epsilon)
            return apply_(xv, scale, shift).reshape(x.shape)
        sums = ops.bn_stats(xv) if inner == 1 else ops.bn_axis_stats(xv)
        scale, shift, smean, sinv, count = self._train_coeffs(ctx, sums, xv.shape[0] * inner)
        # scale / shift: 2 P floats, asked for by the column kernels' backward in place of the layer output (which no pass reads: no activation)
        ctx.tape[node.index] = (xv, smean, sinv, count, scale, shift)
        return apply_(xv, scale, shift).reshape(x.shape)

    def _backward_axis(self, ctx, node, dy, need_dw):
        xv, smean, sinv, count, scale, shift = ctx.tape.pop(node.index)
        dyv = dy.contiguous().reshape(xv.shape)
        if xv.dim() == 2:
            local = ops.bn_bwd_stats(dyv, None, xv, None, smean, sinv, scale=scale, shift=shift)
        else:
            local = ops.bn_axis_bwd_stats(dyv, xv, smean, sinv)
        glob = local
        if ctx.dp is not None:
            glob = local.clone()
            ctx.dp.all_reduce_sum(glob)
        dgamma, dbeta = self._param_grads(need_dw)
        if xv.dim() == 2:
            dx = ops.bn_bwd_apply(dyv, None, xv, None, self.gamma.data, smean, sinv, glob, count, local, dgamma, dbeta, scale=scale, shift=shift)
        else:
            dx = ops.bn_axis_bwd_apply(dyv, xv, self.gamma.data, smean, sinv, glob, count, local, dgamma, dbeta)
        return dx.reshape(dy.shape)


def _softmax_view(layer, axis, input_shape):
    """(rows of `outer` per sample, P, inner) of a softmax over keras' `axis` (the batch axis counted, as BatchNormalization(axis=) counts it) of
    inputs of `input_shape` (without the batch axis), with keras' refusals."""
    n = len(input_shape) + 1
    what = '%s (%s)' % (layer.name, type(layer).__name__)
    if n == 1:
        raise ValueError('%s: Cannot apply softmax to a tensor that is 1D' % what)
    if axis == 0 or axis == -n:
        raise ValueError('%s: softmax over axis %d is the batch axis: it would normalise across the samples of a batch, and under data parallelism '
                         'across ranks; choose one of 1..%d or -1..-%d' % (what, axis, n - 1, n - 1))
    if not (1 <= axis <= n - 1 or -(n - 1) <= axis <= -1):
        raise ValueError('%s: softmax axis %d on inputs of shape %r: the axis must be one of 1..%d or -1..-%d'
                         % (what, axis, (None,) + tuple(input_shape), n - 1, n - 1))
    k = (axis if axis > 0 else axis + n) - 1
    return (int(np.prod(input_shape[:k], dtype=np.int64)), int(input_shape[k]), int(np.prod(input_shape[k + 1:], dtype=np.int64)))


class Softmax(Layer):
    """keras.layers.Softmax(axis=-1) (layers/advanced_activations.py): exp(x - max) / sum exp(x - max) along `axis`, which counts the batch axis;
    the batch axis itself is refused.  Two passes of csrc/softmax.hip on the (outer, P, inner) view, the gradient from the stored output.
    No activation for the planner (act_spec stays None): nothing absorbs it and it absorbs nothing."""

    def __init__(self, axis=-1, **kw):
        Layer.__init__(self, **kw)
        if isinstance(axis, bool) or not isinstance(axis, (int, np.integer)):
            raise ValueError('%s (Softmax): axis=%r is not one integer' % (self.name, axis))
        self.axis = int(axis)
        self.view = None

    def build(self, input_shape):
        self.view = _softmax_view(self, self.axis, input_shape)

    def compute_output_shape(self, input_shape):
        _softmax_view(self, self.axis, input_shape)
        return tuple(input_shape)

    def forward(self, ctx, node, x):
        per, P, inner = self.view
        view = (x.shape[0] * per, P, inner)
        y = ops.softmax_fwd(x.contiguous(), view)
        ctx.tape[node.index] = (y, view)
        return y

    def backward(self, ctx, node, dy, need_dx, need_dw):
        y, view = ctx.tape.pop(node.index)
        return ops.softmax_bwd(dy.contiguous(), y, view)


class Activation(Layer):
    """keras.layers.Activation.  Activation('softmax') is keras' softmax over the last axis: the Softmax layer's two passes under this layer's
    name and config, and like it no activation for the planner."""

    def __init__(self, activation, **kw):
        Layer.__init__(self, **kw)
        spec = _act_spec(activation, 'Activation')
        self.softmax = spec is _SOFTMAX
        self.act_spec = None if self.softmax else spec
        self.view = None

    softmax = False                                        # LeakyReLU, ReLU: element-wise

    def build(self, input_shape):
        if self.softmax:
            self.view = _softmax_view(self, -1, input_shape)

    def compute_output_shape(self, input_shape):
        if self.softmax:
            _softmax_view(self, -1, input_shape)
        return tuple(input_shape)

    forward_softmax, backward_softmax = Softmax.forward, Softmax.backward

    def forward(self, ctx, node, x):
        if self.softmax:
            return self.forward_softmax(ctx, node, x)
        y = x if self.act_spec[0] == 'linear' else ops.act_fwd(x.contiguous(), self.act_spec[0], self.act_spec[1])
        ctx.tape[node.index] = y
        return y

    def backward(self, ctx, node, dy, need_dx, need_dw):
        if self.softmax:
            return self.backward_softmax(ctx, node, dy, need_dx, need_dw)
        y = ctx.tape.pop(node.index)
        if self.act_spec[0] == 'linear':
            return dy
        return ops.act_bwd(dy.contiguous(), y, self.act_spec[0], self.act_spec[1])


class LeakyReLU(Activation):
    def __init__(self, alpha=0.3, **kw):
        Layer.__init__(self, **kw)
        self.alpha = float(np.float32(alpha))       # K.cast_to_floatx(alpha): the reference's Keras files record 0.20000000298023224 for 0.2
        self.act_spec = ('leaky', self.alpha)


class ReLU(Activation):
    """keras.layers.ReLU(max_value=...) (bbhMahoGANy.py:400: ReLU(max_value=1.0))."""

    def __init__(self, max_value=None, negative_slope=0.0, threshold=0.0, **kw):
        Layer.__init__(self, **kw)
        if negative_slope or threshold:
            raise NotImplementedError('ReLU(negative_slope/threshold)')
        self.act_spec = ('relu', 0.0) if max_value is None else ('relu_max', float(max_value))


class PReLU(Layer):
    """keras.layers.PReLU() (bbhMahoGANy.py:39; the act = 'prelu' branches of generator_model, :237-286): one learnable slope per
    feature of a sample (no shared axes), initialised to zero; y = x > 0 ? x : alpha * x."""

    def __init__(self, alpha_initializer='zeros', shared_axes=None, alpha_regularizer=None, **kw):
        Layer.__init__(self, **kw)
        self.alpha_regularizer = regularizers.get(alpha_regularizer)
        if alpha_initializer not in ('zeros', None) and not (isinstance(alpha_initializer, dict) and alpha_initializer.get('class_name') == 'Zeros'):
            raise NotImplementedError('PReLU(alpha_initializer=%r)' % (alpha_initializer,))
        if shared_axes:
            raise NotImplementedError('PReLU(shared_axes=%r)' % (shared_axes,))

    def build(self, input_shape):
        if int(np.prod(input_shape)) % 4:
            raise NotImplementedError('PReLU on %r: the feature count must be a multiple of 4' % (tuple(input_shape),))
        self.alpha = self.add_weight('alpha', np.zeros(tuple(input_shape), np.float32), regularizer=self.alpha_regularizer)

    def forward(self, ctx, node, x):
        x = x.contiguous()
        ctx.tape[node.index] = x
        return ops.prelu_fwd(x, self.alpha.data)

    def backward(self, ctx, node, dy, need_dx, need_dw):
        x = ctx.tape.pop(node.index)
        dx, _ = ops.prelu_bwd(dy.contiguous(), x, self.alpha.data, need_dx or not need_dw, self.alpha.grad if need_dw else None)
        return dx


class ActivityRegularization(Layer):
    """keras.layers.ActivityRegularization(l1=0., l2=0.): the identity, whose output carries the activity regularizer L1L2(l1, l2).  The penalty and
    its gradient term are the engine's (Model._forward / _backward); the layer itself launches nothing.  With both coefficients zero it
    regularizes nothing and no pass runs."""

    def __init__(self, l1=0., l2=0., **kw):
        Layer.__init__(self, **kw)
        reg = regularizers.L1L2(l1=l1, l2=l2)
        self.l1, self.l2 = reg.l1, reg.l2
        self.activity_regularizer = regularizers.active(reg)

    def forward(self, ctx, node, x):
        return x

    def backward(self, ctx, node, dy, need_dx, need_dw):
        return dy


class Dropout(Layer):
    """Inverted dropout, active in the training phase only (which keras applies to the WHOLE graph in train_on_batch,
    including layers of frozen sub-models: bbhMahoGANy.py:1296 keeps D's Dropout(0.4) active during the G step)."""

    def __init__(self, rate, **kw):
        Layer.__init__(self, **kw)
        self.rate = float(rate)
        self.drop_rate = self.rate

    def make_mask(self, ctx, shape):
        inj = ctx.dropout_masks.get(self.name)
        if inj is not None:
            return inj.reshape(shape).contiguous()
        n = int(np.prod(shape))
        if ctx.row_map is None:
            seed, off = device_rng().take(n)
            return ops.dropout_mask(shape, self.rate, seed, off, device())
        # data parallelism: the local rows are blocks of the global batch; every block draws the counters of its global rows
        blocks, grows = ctx.row_map
        if sum(nr for _, nr in blocks) != shape[0]:
            raise ValueError('Dropout: the row map covers %d rows, the tensor has %d' % (sum(nr for _, nr in blocks), shape[0]))
        row_len = n // shape[0]
        seed, offs = device_rng().take_rows(row_len, blocks, grows)
        parts = [ops.dropout_mask((nr,) + tuple(shape[1:]), self.rate, seed, off, device()) for (_, nr), off in zip(blocks, offs)]
        return parts[0] if len(parts) == 1 else torch.cat(parts)

    def forward(self, ctx, node, x):
        if not ctx.training or self.rate == 0.0:
            ctx.tape[node.index] = None
            return x
        mask = self.make_mask(ctx, x.shape)
        ctx.tape[node.index] = mask
        return ops.dropout_apply(x.contiguous(), mask, self.rate)

    def backward(self, ctx, node, dy, need_dx, need_dw):
        mask = ctx.tape.pop(node.index)
        if mask is None:
            return dy
        return ops.dropout_apply(dy.contiguous(), mask, self.rate)


_SELU_ALPHA_P = -1.6732632423543772848170429916717 * 1.0507009873554804934193349852946     # keras' AlphaDropout: -alpha * scale of SELU


def _noise_rate(layer_name, rate):
    rate = float(rate)
    if rate != rate:
        raise ValueError('%s(rate=nan)' % layer_name)
    return rate


class _NoiseLayer(Layer):
    """Keras 2.2.4 layers/noise.py: a training-phase-only layer whose draw is made inside its own kernel (gennet_amd/csrc/noise_layers.hip).
    The forward takes ceil(n / 4) counters of the device stream (under ctx.row_map, those of its global rows, one launch per block, as
    Dropout.make_mask); the tape keeps only (seed, [(local row start, rows, counter offset)]) and the backward regenerates the draw from it.
    Not a Dropout for the planner: drop_rate stays None, so no conv / BatchNormalization epilogue absorbs it."""

    def _active(self):
        return True

    def _run(self, kind, x, seed, offset, out):
        raise NotImplementedError

    def _draws(self, ctx, shape):
        n = int(np.prod(shape))
        if ctx.row_map is None:
            seed, off = device_rng().take(n)
            return seed, [(0, shape[0], off)]
        blocks, grows = ctx.row_map
        if sum(nr for _, nr in blocks) != shape[0]:
            raise ValueError('%s: the row map covers %d rows, the tensor has %d' % (self.name, sum(nr for _, nr in blocks), shape[0]))
        seed, offs = device_rng().take_rows(n // shape[0], blocks, grows)
        parts, r0 = [], 0
        for (_, nr), off in zip(blocks, offs):
            parts.append((r0, nr, off))
            r0 += nr
        return seed, parts

    def _apply(self, kind, x, seed, parts):
        x = x.contiguous()
        y = torch.empty_like(x)
        for r0, nr, off in parts:
            self._run(kind, x[r0:r0 + nr], seed, off, y[r0:r0 + nr])
        return y

    def forward(self, ctx, node, x):
        if not ctx.training or not self._active():
            ctx.tape[node.index] = None
            return x
        seed, parts = self._draws(ctx, x.shape)
        ctx.tape[node.index] = (seed, parts)
        return self._apply('fwd', x, seed, parts)

    def backward(self, ctx, node, dy, need_dx, need_dw):
        t = ctx.tape.pop(node.index)
        if t is None:
            return dy
        return self._apply('bwd', dy, t[0], t[1])


class GaussianNoise(_NoiseLayer):
    """keras.layers.GaussianNoise(stddev): y = x + stddev * z in the training phase (the reference's sibling models put GaussianNoise(1) on the
    discriminator's input).  The gradient is the identity."""

    def __init__(self, stddev, **kw):
        Layer.__init__(self, **kw)
        self.stddev = float(stddev)
        if not (self.stddev >= 0.0 and np.isfinite(self.stddev)):
            raise ValueError('GaussianNoise(stddev=%r): a finite standard deviation >= 0' % (stddev,))

    def _run(self, kind, x, seed, offset, out):
        ops.gaussian_noise(x, self.stddev, seed, offset, out)

    def backward(self, ctx, node, dy, need_dx, need_dw):
        ctx.tape.pop(node.index)
        return dy


class GaussianDropout(_NoiseLayer):
    """keras.layers.GaussianDropout(rate): y = x * m, m ~ N(1, rate / (1 - rate)) in the training phase; dx = dy * m (the same pass with the
    forward's counters).  rate outside (0, 1) is the identity, as in keras."""

    def __init__(self, rate, **kw):
        Layer.__init__(self, **kw)
        self.rate = _noise_rate('GaussianDropout', rate)
        self.sd = float(np.float32(np.sqrt(self.rate / (1.0 - self.rate)))) if self._active() else 0.0

    def _active(self):
        return 0.0 < self.rate < 1.0

    def _run(self, kind, x, seed, offset, out):
        ops.gaussian_dropout(x, self.sd, seed, offset, out)


class AlphaDropout(_NoiseLayer):
    """keras.layers.AlphaDropout(rate): a dropped value becomes SELU's negative saturation alpha_p, then the affine map a * x + b that keeps
    zero mean and unit variance; in the training phase only.  rate outside (0, 1) is the identity, as in keras.  Every draw comes from the
    process's one device stream, so noise_shape and seed are refused rather than ignored."""

    def __init__(self, rate, noise_shape=None, seed=None, **kw):
        Layer.__init__(self, **kw)
        if noise_shape is not None:
            raise NotImplementedError('AlphaDropout(noise_shape=%r): only the full-shape draw is implemented' % (noise_shape,))
        if seed is not None:
            raise NotImplementedError('AlphaDropout(seed=%r): the draws come from the device stream (engine.set_device_seed)' % (seed,))
        self.rate = _noise_rate('AlphaDropout', rate)
        if self._active():
            r, ap = self.rate, _SELU_ALPHA_P
            a = ((1.0 - r) * (1.0 + r * ap ** 2)) ** -0.5
            self.a, self.b, self.alpha_p = float(np.float32(a)), float(np.float32(-a * ap * r)), float(np.float32(ap))

    def _active(self):
        return 0.0 < self.rate < 1.0

    def _run(self, kind, x, seed, offset, out):
        if kind == 'fwd':
            ops.alpha_dropout_fwd(x, self.rate, self.a, self.b, self.alpha_p, seed, offset, out)
        else:
            ops.alpha_dropout_bwd(x, self.rate, self.a, seed, offset, out)


class Reshape(Layer):
    shape_only = True

    def __init__(self, target_shape, **kw):
        Layer.__init__(self, **kw)
        self.target_shape_arg = tuple(int(v) for v in target_shape)      # may hold one -1, as keras allows
        self.target_shape = self.target_shape_arg
        if list(self.target_shape_arg).count(-1) > 1:
            raise ValueError('Reshape: at most one unknown dimension')

    def compute_output_shape(self, input_shape):
        n = int(np.prod(input_shape))
        if -1 in self.target_shape_arg:
            known = -int(np.prod(self.target_shape_arg))
            assert known > 0 and n % known == 0, 'Reshape%r does not fit an input of %d elements' % (self.target_shape_arg, n)
            self.target_shape = tuple(n // known if v == -1 else v for v in self.target_shape_arg)
        assert n == int(np.prod(self.target_shape)), 'Reshape%r does not fit an input of %d elements' % (self.target_shape_arg, n)
        return self.target_shape

    def forward(self, ctx, node, x):
        ctx.tape[node.index] = x.shape
        return x.reshape((x.shape[0],) + self.target_shape)

    def backward(self, ctx, node, dy, need_dx, need_dw):
        return dy.reshape(ctx.tape.pop(node.index))


class Flatten(Layer):
    shape_only = True
    """Row-major flatten of channels-last activations: feature index = t*C + c (keras order, SURVEY Appendix B.7)."""

    def compute_output_shape(self, input_shape):
        return (int(np.prod(input_shape)),)

    def forward(self, ctx, node, x):
        ctx.tape[node.index] = x.shape
        return x.reshape(x.shape[0], -1)

    def backward(self, ctx, node, dy, need_dx, need_dw):
        return dy.reshape(ctx.tape.pop(node.index))


class UpSampling1D(Layer):
    """bbhMahoGANy.py:249,:258.  In front of a 5-tap 'same' Conv1D (both uses in the generator) the planner folds it into that conv's
    weights and this layer never runs; the kernels below serve every other placement."""
    is_upsample2 = True

    def __init__(self, size=2, **kw):
        Layer.__init__(self, **kw)
        if size != 2:
            raise NotImplementedError('UpSampling1D(size=%r)' % (size,))

    def compute_output_shape(self, input_shape):
        return (2 * input_shape[0], input_shape[1])

    def forward(self, ctx, node, x):
        return ops.upsample2_fwd(x.contiguous())

    def backward(self, ctx, node, dy, need_dx, need_dw):
        return ops.upsample2_bwd(dy.contiguous())


def _pool_tuple(v, rank, what):
    t = (int(v),) * rank if isinstance(v, (int, np.integer)) and not isinstance(v, bool) else tuple(int(u) for u in v)
    if len(t) != rank or any(u < 1 for u in t):
        raise ValueError('%s %r: %d positive integer%s' % (what, v, rank, '' if rank == 1 else 's'))
    return t


class _Pooling(Layer):
    """Keras 2.2.4 layers/pooling.py on the passes of csrc/pooling.hip: channels_last, any pool_size, strides (None: the pool size) and
    padding 'valid' | 'same'.  The 1-D layers run as (B, L, 1, C).  An ordinary layer for the planner: it absorbs nothing and nothing absorbs it.
    The tape keeps x for the maximum in the training phase, shapes only for the average."""
    mode, rank = None, 2

    def __init__(self, pool_size=None, strides=None, padding='valid', data_format=None, **kw):
        Layer.__init__(self, **kw)
        name = type(self).__name__
        if pool_size is None:
            pool_size = 2
        if data_format not in (None, 'channels_last'):
            raise NotImplementedError('%s(data_format=%r): channels_last only' % (name, data_format))
        if padding not in ('valid', 'same'):
            raise ValueError("%s(padding=%r): 'valid' or 'same'" % (name, padding))
        self.pool_size = _pool_tuple(pool_size, self.rank, '%s(pool_size)' % name)
        self.strides = self.pool_size if strides is None else _pool_tuple(strides, self.rank, '%s(strides)' % name)
        self.padding = padding
        # the discriminator's `maxpool = True` layers keep their own two kernels (csrc/pool.hip): same kernels, same launches
        self.h2 = self.mode == 'max' and self.rank == 2 and self.pool_size == (2, 1) and self.strides == (2, 1) and padding == 'valid'

    def _pool2(self):
        return (self.pool_size + (1,))[:2], (self.strides + (1,))[:2]

    def compute_output_shape(self, input_shape):
        if len(input_shape) != self.rank + 1:
            raise ValueError('%s expects (batch, %s, channels) inputs, got %r' % (type(self).__name__, 'steps' if self.rank == 1 else 'rows, cols',
                                                                                 (None,) + tuple(input_shape)))
        out =tuple(ops.pool_geometry(n, p, s, self.padding)[0] for n, p, s in zip(input_shape, self.pool_size, self.strides))
        return out + (input_shape[-1],)

    def forward(self, ctx, node, x):
        x = x.contiguous()
        if self.h2:
            if ctx.training:
                ctx.tape[node.index] = x
            return ops.maxpool_h2_fwd(x)
        x4 = x if self.rank == 2 else x.unsqueeze(2)
        if ctx.training:
            ctx.tape[node.index] = (x4 if self.mode == 'max' else None, tuple(x4.shape))
        pool, strides = self._pool2()
        y = ops.pool2d_fwd(self.mode, x4, pool, strides, self.padding)
        return y if self.rank == 2 else y.squeeze(2)

    def backward(self, ctx, node, dy, need_dx, need_dw):
        if self.h2:
            return ops.maxpool_h2_bwd(dy.contiguous(), ctx.tape.pop(node.index))
        x4, shape = ctx.tape.pop(node.index)
        dy = dy.contiguous()
        pool, strides = self._pool2()
        dx = ops.pool2d_bwd(self.mode, dy if self.rank == 2 else dy.unsqueeze(2), x4, shape, pool, strides, self.padding)
        return dx if self.rank == 2 else dx.squeeze(2)


class MaxPooling2D(_Pooling):
    """keras.layers.MaxPooling2D.  bbhMahoGANy.py:444, :453, :462, ... (`maxpool = True`) place MaxPooling2D(pool_size=(2,1)) -- pairs of rows along
    H; strides = pool_size, 'valid' -- which runs the two kernels of csrc/pool.hip; every other configuration runs csrc/pooling.hip.  The
    gradient goes to the first maximum of a window in row-major order, as TensorFlow's."""
    mode = 'max'

    def __init__(self, pool_size=(2, 2), strides=None, padding='valid', data_format=None, **kw):
        _Pooling.__init__(self, pool_size, strides, padding, data_format, **kw)


class AveragePooling2D(_Pooling):
    """keras.layers.AveragePooling2D: under 'same' the divisor is the number of in-bounds cells of the window (TensorFlow excludes the padding)."""
    mode = 'avg'

    def __init__(self, pool_size=(2, 2), strides=None, padding='valid', data_format=None, **kw):
        _Pooling.__init__(self, pool_size, strides, padding, data_format, **kw)


class MaxPooling1D(_Pooling):
    """keras.layers.MaxPooling1D (the Conv1D -> MaxPooling1D(pool_size=2) blocks of the reference's tests/burstMahoGANy.py)."""
    mode, rank = 'max', 1

    def __init__(self, pool_size=2, strides=None, padding='valid', data_format=None, **kw):
        _Pooling.__init__(self, pool_size, strides, padding, data_format, **kw)


class AveragePooling1D(_Pooling):
    mode, rank = 'avg', 1

    def __init__(self, pool_size=2, strides=None, padding='valid', data_format=None, **kw):
        _Pooling.__init__(self, pool_size, strides, padding, data_format, **kw)


class _GlobalPooling(Layer):
    """Keras 2.2.4 Global{Average,Max}Pooling{1D,2D}: (B, L, C) or (B, H, W, C) -> (B, C) over the (B, P, C) view.  The average's gradient is
    dy / P; the maximum is K.max, whose gradient is dy / n_ties at every position equal to the maximum (tf.reduce_max), and the tape keeps x and
    y for it in the training phase."""
    mode, rank = None, 1

    def __init__(self, data_format=None, **kw):
        Layer.__init__(self, **kw)
        if data_format not in (None, 'channels_last'):
            raise NotImplementedError('%s(data_format=%r): channels_last only' % (type(self).__name__, data_format))

    def compute_output_shape(self, input_shape):
        if len(input_shape) != self.rank + 1:
            raise ValueError('%s expects (batch, %s, channels) inputs, got %r' % (type(self).__name__, 'steps' if self.rank == 1 else 'rows, cols',
                                                                                 (None,) + tuple(input_shape)))
        return (input_shape[-1],)

    def forward(self, ctx, node, x):
        x3 = x.contiguous().reshape(x.shape[0], -1, x.shape[-1])
        y = ops.global_pool_fwd(self.mode, x3)
        if ctx.training:
            ctx.tape[node.index] = (x3, y, tuple(x.shape)) if self.mode == 'max' else (None, None, tuple(x.shape))
        return y

    def backward(self, ctx, node, dy, need_dx, need_dw):
        x3, y, shape = ctx.tape.pop(node.index)
        return ops.global_pool_bwd(self.mode, dy.contiguous(), x3, y, (shape[0], int(np.prod(shape[1:-1])), shape[-1])).reshape(shape)


class GlobalAveragePooling1D(_GlobalPooling):
    """the tail of the sibling discriminator (2_model_version/*/subtract_model.py): GlobalAveragePooling1D() -> Dense(2, 'sigmoid')"""
    mode, rank = 'avg', 1


class GlobalAveragePooling2D(_GlobalPooling):
    mode, rank = 'avg', 2


class GlobalMaxPooling1D(_GlobalPooling):
    mode, rank = 'max', 1


class GlobalMaxPooling2D(_GlobalPooling):
    mode, rank = 'max', 2


class MyLayer(Layer):
    """bbhMahoGANy.py:164-188: stack([x, const - x], axis=2): (B, n_pix, 1) -> (B, n_pix, 2, 1), const = measured data h(t)."""

    def __init__(self, const, **kw):
        Layer.__init__(self, **kw)
        self._const_host = np.asarray(const, np.float32).reshape(-1)
        self._const = None

    def get_const(self):
        """the layer's constant as the host array it was given (float32, flat)"""
        return self._const_host.copy()

    @property
    def const(self):
        if self._const is None:
            from .engine import to_device
            self._const = to_device(self._const_host)
        return self._const

    def compute_output_shape(self, input_shape):
        return (input_shape[0], 2, 1)

    def forward(self, ctx, node, x):
        assert x.shape[1] == self.const.numel()
        return ops.subtract_stack_fwd(x.contiguous(), self.const)

    def backward(self, ctx, node, dy, need_dx, need_dw):
        return ops.subtract_stack_bwd(dy.contiguous())


# --------------------------------------------------------------------------------------------------------------
# merge layers (keras layers/merge.py; csrc/merge.hip)
# --------------------------------------------------------------------------------------------------------------
def _merge_shapes(layer, input_shape, but_axis=None):
    """The list of input shapes (no batch axis) of a merge layer, checked: 2 .. GN_MERGE_MAX_INPUTS tensors of one rank and, except along
    `but_axis`, one shape.  Broadcasting between inputs is not provided."""
    name = type(layer).__name__
    if not isinstance(input_shape, (list, tuple)) or not input_shape or not isinstance(input_shape[0], (list, tuple)):
        raise ValueError('A merge layer should be called on a list of at least 2 inputs (%s)' % layer.name)
    shapes = [tuple(s) for s in input_shape]
    if len(shapes) < 2:
        raise ValueError('A merge layer should be called on a list of at least 2 inputs (%s got %d)' % (layer.name, len(shapes)))
    if len(shapes) > ops.MERGE_MAX_INPUTS:
        raise ValueError('%s on %d inputs: at most %d (GN_MERGE_MAX_INPUTS) are joined in one layer' % (name, len(shapes), ops.MERGE_MAX_INPUTS))
    for s in shapes[1:]:
        same = len(s) == len(shapes[0]) and all(a == b for d, (a, b) in enumerate(zip(s, shapes[0])) if d != but_axis)
        if not same:
            raise ValueError('%s: the inputs must have the same shape%s (no broadcasting between inputs), got %r and %r'
                             % (name, '' if but_axis is None else ' except along the concatenation axis', (None,) + shapes[0], (None,) + s))
    return shapes


class _Merge(Layer):
    """Keras 2.2.4 layers/merge.py _Merge on one pass of csrc/merge.hip: the inputs folded left to right in fp32, as keras' _merge_function loops.
    Called on a list of 2 .. 8 tensors of one shape.  The backward returns one gradient per input (None where none is wanted): Add hands its dy to
    every input and Average one scaled tensor to all of them -- Model._backward never writes into a tensor two edges hold.  The tape keeps the
    inputs only where the gradient reads them (Multiply, Maximum, Minimum), in the training phase."""
    is_merge = True
    mode = None

    def compute_output_shape(self, input_shape):
        return _merge_shapes(self, input_shape)[0]

    def forward(self, ctx, node, xs):
        xs = [x.contiguous() for x in xs]
        if ctx.training and self.mode in ('mul', 'max', 'min'):
            ctx.tape[node.index] = xs
        return ops.merge_fwd(self.mode, xs)

    def backward(self, ctx, node, dy, need_dx, need_dw):
        k = len(need_dx)
        dy = dy.contiguous()
        if self.mode in ('mul', 'max', 'min'):
            xs = ctx.tape.pop(node.index)
            return [ops.merge_bwd(self.mode, dy, xs, j) if w else None for j, w in enumerate(need_dx)]
        if self.mode == 'add':
            return [dy if w else None for w in need_dx]
        if self.mode == 'sub':
            return [dy if need_dx[0] else None, ops.scale(dy, -1.0) if need_dx[1] else None]
        g = ops.scale(dy, float(np.float32(1.0) / np.float32(k))) if any(need_dx) else None          # 'avg'
        return [g if w else None for w in need_dx]


class Add(_Merge):
    """keras.layers.Add: x0 + x1 + ... (a residual connection: Add()([block(h), h]))."""
    mode = 'add'


class Subtract(_Merge):
    """keras.layers.Subtract: x0 - x1, exactly two inputs (bbhMahoGANy.py:1268: noise_signal - generated, on the host there)."""
    mode = 'sub'

    def compute_output_shape(self, input_shape):
        if isinstance(input_shape, (list, tuple)) and len(input_shape) != 2:
            raise ValueError('A `Subtract` layer should be called on exactly 2 inputs (%s got %d)' % (self.name, len(input_shape)))
        return _Merge.compute_output_shape(self, input_shape)


class Multiply(_Merge):
    mode = 'mul'


class Average(_Merge):
    """keras.layers.Average: (x0 + x1 + ...) / k, the sum left to right and one division."""
    mode = 'avg'


class Maximum(_Merge):
    """keras.layers.Maximum: K.maximum chained left to right; on a tie the gradient goes to the first input that attains the maximum."""
    mode = 'max'


class Minimum(_Merge):
    mode = 'min'


class Concatenate(Layer):
    """keras.layers.Concatenate(axis=-1): the inputs side by side along `axis`, which counts the batch axis as in keras (axis 0 is refused).
    One gather launch forward, one scatter launch backward (only into the inputs that want a gradient).
    bbhMahoGANy.py:1268-1272 as layers: Concatenate(axis=-1)([g, Subtract()([event, g])])."""
    is_merge = True

    def __init__(self, axis=-1, **kw):
        Layer.__init__(self, **kw)
        if isinstance(axis, bool) or not isinstance(axis, (int, np.integer)):
            raise ValueError('Concatenate(axis=%r): an integer' % (axis,))
        if axis == 0:
            raise ValueError('Concatenate(axis=0): concatenating along the batch axis is refused')
        self.axis = int(axis)

    def _axis(self, rank):
        """The axis of the (batch, ...) tensors of `rank` dimensions, 1 <= axis < rank."""
        ax = self.axis + rank if self.axis < 0 else self.axis
        if not 1 <= ax < rank:
            raise ValueError('Concatenate(axis=%d) on inputs of %d dimensions (the batch axis included): the axis must be one of 1 .. %d or -1 .. %d; '
                             'concatenating along the batch axis is refused' % (self.axis, rank, rank - 1, -(rank - 1)))
        return ax

    def compute_output_shape(self, input_shape):
        if not isinstance(input_shape, (list, tuple)) or not input_shape or not isinstance(input_shape[0], (list, tuple)):
            raise ValueError('A merge layer should be called on a list of at least 2 inputs (%s)' % self.name)
        ax = self._axis(len(input_shape[0]) + 1) - 1
        shapes = _merge_shapes(self, input_shape, ax)
        return shapes[0][:ax] + (sum(s[ax] for s in shapes),) + shapes[0][ax + 1:]

    def forward(self, ctx, node, xs):
        xs = [x.contiguous() for x in xs]
        if ctx.training:
            ctx.tape[node.index] = [tuple(x.shape) for x in xs]
        return ops.concat_fwd(xs, self._axis(xs[0].dim()))

    def backward(self, ctx, node, dy, need_dx, need_dw):
        shapes = ctx.tape.pop(node.index)
        return ops.concat_bwd(dy.contiguous(), shapes, self._axis(len(shapes[0])), need_dx)


def add(inputs, **kw):
    return Add(**kw)(inputs)


def subtract(inputs, **kw):
    return Subtract(**kw)(inputs)


def multiply(inputs, **kw):
    return Multiply(**kw)(inputs)


def average(inputs, **kw):
    return Average(**kw)(inputs)


def maximum(inputs, **kw):
    return Maximum(**kw)(inputs)


def minimum(inputs, **kw):
    return Minimum(**kw)(inputs)


def concatenate(inputs, axis=-1, **kw):
    return Concatenate(axis=axis, **kw)(inputs)


# keras.layers.Dot / dot live in gennet_amd/dot.py and are part of this name space
from .dot import Dot, dot  # noqa: E402,F401

# keras.layers.LSTM, keras.layers.GRU, keras.layers.SimpleRNN and keras.layers.Bidirectional live in gennet_amd/recurrent.py (DESIGN 8o - 8q,
# 8s) and are part of this name space
from .recurrent import GRU, LSTM, Bidirectional, SimpleRNN  # noqa: E402,F401

# keras.layers.SeparableConv1D lives in gennet_amd/separable.py and is part of this name space
from .separable import SeparableConv1D  # noqa: E402,F401

# keras.layers.TimeDistributed, RepeatVector, Permute, Cropping1D and ZeroPadding1D live in gennet_amd/sequence.py and are part of
# this name space
from .sequence import Cropping1D, Permute, RepeatVector, TimeDistributed, ZeroPadding1D  # noqa: E402,F401

# keras.layers.Attention lives in gennet_amd/attention.py and is part of this name space
from .attention import Attention  # noqa: E402,F401

# keras.layers.LayerNormalization lives in gennet_amd/layernorm.py and is part of this name space
from .layernorm import LayerNormalization  # noqa: E402,F401
