"""keras.layers.LayerNormalization (tf.keras 2.x layers/normalization.py) on the one-pass row kernels of csrc/layernorm.hip; DESIGN 8v.

The class is part of the gennet_amd.layers name space (gennet_amd.layers.LayerNormalization is this class), as every layer is."""
import numpy as np

from . import ops, regularizers
from .engine import Layer


def _is_initializer(value, name):
    return value is None or value == name or (isinstance(value, dict) and value.get('class_name') == name.capitalize())


class LayerNormalization(Layer):
    """keras.layers.LayerNormalization(axis=-1, epsilon=1e-3, center=True, scale=True): every sample is normalised over `axis` with its own mean
    and biased variance, y = (x - mean) / sqrt(var + epsilon) * gamma + beta -- the same in both phases, no moving state, nothing that depends on
    the batch or on the data-parallel world size.  axis: an int or a list / tuple of ints, counting the batch axis, negatives allowed; the
    normalised axes must be the trailing block of the input (-1, [-2, -1], [1, 2] on a rank-3 input), ascending.  Weights, in keras' order:
    gamma (ones; absent with scale=False) and beta (zeros; absent with center=False), each of the shape of the normalised axes.
    One gn_layernorm_fwd and one gn_layernorm_bwd on the (rows, N) view; the tape keeps x and the (rows,) mean and rstd, in the training phase
    only.  Fuses with nothing: no BatchNormalization for the planner, no activation or dropout epilogue.
    Refused by name: any other set of axes (NotImplementedError), the batch axis, an axis out of range or given twice (ValueError), an
    initializer other than zeros / ones, a constraint.  DESIGN 8v."""

    def __init__(self, axis=-1, epsilon=1e-3, center=True, scale=True, beta_initializer='zeros', gamma_initializer='ones', beta_regularizer=None,
                 gamma_regularizer=None, beta_constraint=None, gamma_constraint=None, **kw):
        kw.pop('dtype', None)
        Layer.__init__(self, **kw)
        axes = list(axis) if isinstance(axis, (list, tuple)) else [axis]
        if not axes or any(isinstance(a, bool) or not isinstance(a, (int, np.integer)) for a in axes):
            raise TypeError("%s (LayerNormalization): Expected an int or a list/tuple of ints for the argument 'axis', but received: %r" % (self.name, axis))
        self.axis = [int(a) for a in axes] if isinstance(axis, (list, tuple)) else int(axis)      # as given until build; then keras' list
        if not _is_initializer(beta_initializer, 'zeros'):
            raise NotImplementedError('%s (LayerNormalization): beta_initializer %r (only zeros)' % (self.name, beta_initializer))
        if not _is_initializer(gamma_initializer, 'ones'):
            raise NotImplementedError('%s (LayerNormalization): gamma_initializer %r (only ones)' % (self.name, gamma_initializer))
        for key, value in (('beta_constraint', beta_constraint), ('gamma_constraint', gamma_constraint)):
            if value is not None:
                raise NotImplementedError('%s (LayerNormalization): %s=%r: weight constraints are not implemented' % (self.name, key, value))
        self.epsilon, self.center, self.scale = float(epsilon), bool(center), bool(scale)
        if not (self.epsilon >= 0.0 and np.isfinite(self.epsilon)):
            raise ValueError('%s (LayerNormalization): epsilon=%r: a finite value >= 0' % (self.name, epsilon))
        self.beta_regularizer, self.gamma_regularizer = regularizers.get(beta_regularizer), regularizers.get(gamma_regularizer)
        self.gamma = self.beta = None
        self.N = None

    def _axes(self, input_shape):
        """keras' axis list after build (non-negative, the batch axis counted) for an input shape without the batch axis, with the refusals"""
        n = len(input_shape) + 1
        given = self.axis if isinstance(self.axis, list) else [self.axis]
        shown = (None,) + tuple(input_shape)
        for a in given:
            if not -n <= a < n:
                raise ValueError('%s (LayerNormalization): Invalid axis: %d on inputs of shape %r' % (self.name, a, shown))
        axes = [a + n if a < 0 else a for a in given]
        if len(set(axes)) != len(axes):
            raise ValueError('%s (LayerNormalization): Duplicate axis: %r' % (self.name, tuple(given)))
        if 0 in axes:
            raise ValueError('%s (LayerNormalization): axis %r includes the batch axis: it would normalise across the samples of a batch, and under data '
                             'parallelism across ranks' % (self.name, tuple(given)))
        if axes != list(range(n - len(axes), n)):
            raise NotImplementedError('%s (LayerNormalization): axis %r on inputs of shape %r: only the trailing axes, ascending (%r here), are '
                                      'normalised; other sets of axes are not implemented'
                                      % (self.name, tuple(given), shown, [list(range(n - k, n)) for k in range(1, n)]))
        return axes

    def build(self, input_shape):
        axes = self._axes(input_shape)
        shape = tuple(int(input_shape[a - 1]) for a in axes)
        self.axis, self.N = axes, int(np.prod(shape, dtype=np.int64))
        if self.scale and self.gamma is None:
            self.gamma = self.add_weight('gamma', np.ones(shape, np.float32), regularizer=self.gamma_regularizer)
        if self.center and self.beta is None:
            self.beta = self.add_weight('beta', np.zeros(shape, np.float32), regularizer=self.beta_regularizer)
        self.built = True

    def compute_output_shape(self, input_shape):
        self._axes(input_shape)
        return tuple(input_shape)

    def forward(self, ctx, node, x):
        x = x.contiguous()
        y, mean, rstd = ops.layernorm_fwd(x, self.gamma.data if self.scale else None, self.beta.data if self.center else None, self.N, self.epsilon,
                                          training=ctx.training)
        if ctx.training:
            ctx.tape[node.index] = (x, mean, rstd)
        return y

    def backward(self, ctx, node, dy, need_dx, need_dw):
        x, mean, rstd = ctx.tape.pop(node.index)
        dx, _, _ = ops.layernorm_bwd(dy.contiguous(), x, self.gamma.data if self.scale else None, mean, rstd, self.N, need_dx,
                                     dgamma=self.gamma.grad if need_dw and self.scale else None, dbeta=self.beta.grad if need_dw and self.center else None)
        return dx
