"""keras.regularizers of Keras 2.2.4 (keras/regularizers.py): L1L2 and its three short forms, serialize / deserialize / get.

A regularizer here is a pair of coefficients and nothing else: the penalty l1 * sum|t| + l2 * sum t^2 and its gradient are the passes of
csrc/regularizer.hip, run by the engine.  The coefficients are cast to floatx as Keras casts them: what the kernels
take, and what get_config writes, is np.float32(value)."""
import numpy as np


class Regularizer(object):
    """keras.regularizers.Regularizer: the base class.  Only L1L2 has a HIP pass."""

    def __call__(self, x):
        raise NotImplementedError('%s is a pair of coefficients for the *_regularizer keywords of a layer; there is no tensor runtime to call it on'
                                  % type(self).__name__)

    @classmethod
    def from_config(cls, config):
        return cls(**config)


class L1L2(Regularizer):
    """l1 * sum|t| + l2 * sum t^2 over all elements of t (an activity: the batch axis included, no division by the batch size)."""

    def __init__(self, l1=0., l2=0.):
        self.l1 = float(np.float32(l1))            # K.cast_to_floatx
        self.l2 = float(np.float32(l2))
        for k, v in (('l1', self.l1), ('l2', self.l2)):
            if not (v >= 0.0 and np.isfinite(v)):
                raise ValueError('L1L2(%s=%r): a finite coefficient >= 0' % (k, l1 if k == 'l1' else l2))

    def get_config(self):
        return {'l1': self.l1, 'l2': self.l2}

    def __eq__(self, other):
        return isinstance(other, L1L2) and (self.l1, self.l2) == (other.l1, other.l2)

    def __ne__(self, other):
        return not self == other

    __hash__ = None

    def __repr__(self):
        return 'L1L2(l1=%r, l2=%r)' % (self.l1, self.l2)


def l1(l=0.01):
    return L1L2(l1=l)


def l2(l=0.01):
    return L1L2(l2=l)


def l1_l2(l1=0.01, l2=0.01):
    return L1L2(l1=l1, l2=l2)


def serialize(regularizer):
    """keras.utils.serialize_keras_object: {'class_name': 'L1L2', 'config': {'l1': ..., 'l2': ...}}, or None."""
    if regularizer is None:
        return None
    return {'class_name': type(regularizer).__name__, 'config': regularizer.get_config()}


def deserialize(config, custom_objects=None):
    if isinstance(config, dict) and 'class_name' in config:
        if config['class_name'] != 'L1L2':
            raise ValueError('Unknown regularizer: %s (L1L2 is the one Keras 2.2.4 ships and the one with a HIP pass)' % config['class_name'])
        return L1L2.from_config(config.get('config') or {})
    if isinstance(config, str):
        fn = {'l1': l1, 'l2': l2, 'l1_l2': l1_l2}.get(config)
        if fn is None:
            raise ValueError('Unknown regularizer: %s' % config)
        return fn()
    raise ValueError('Could not interpret regularizer identifier: %r' % (config,))


def get(identifier):
    """keras.regularizers.get: None, an L1L2, one of the strings 'l1' / 'l2' / 'l1_l2' (Keras' defaults of 0.01), or a config dict.  Keras
    would call any other callable on the weight tensor; with no tensor runtime to trace it on, that is refused by name."""
    if identifier is None or isinstance(identifier, L1L2):
        return identifier
    if isinstance(identifier, (dict, str)):
        return deserialize(identifier)
    if callable(identifier):
        raise NotImplementedError('regularizer %s: only keras.regularizers.L1L2 (l1, l2, l1_l2) has a HIP pass; a custom callable cannot be lowered'
                                  % getattr(identifier, '__name__', type(identifier).__name__))
    raise ValueError('Could not interpret regularizer identifier: %r' % (identifier,))


def active(regularizer):
    """The regularizer if it has a non-zero coefficient, else None: L1L2() with both zero (ActivityRegularization's defaults) costs no pass."""
    return regularizer if regularizer is not None and (regularizer.l1 > 0.0 or regularizer.l2 > 0.0) else None
