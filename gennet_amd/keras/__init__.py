"""Import-compatible facade for the subset of Keras 2.2.4 that BBH_version/bbhMahoGANy.py imports (bbhMahoGANy.py:32-43, :65):

    from gennet_amd.keras.models import Sequential, Model            # was: from keras.models import ...
    from gennet_amd.keras.layers import Dense, Input, Reshape, Dropout
    from gennet_amd.keras.layers.core import Activation, Flatten
    from gennet_amd.keras.layers.normalization import BatchNormalization
    from gennet_amd.keras.layers.normalization import LayerNormalization   # tf.keras 2.x; also gennet_amd.keras.layers.LayerNormalization
    from gennet_amd.keras.layers.convolutional import UpSampling1D, Conv2D, Conv1D, Conv2DTranspose
    from gennet_amd.keras.layers.convolutional import SeparableConv1D  # also gennet_amd.keras.layers.SeparableConv1D
    from gennet_amd.keras.layers.advanced_activations import LeakyReLU, ReLU, Softmax
    from gennet_amd.keras.activations import softmax, relu, tanh, sigmoid, linear            # names for activation=
    from gennet_amd.keras import regularizers                          # l1, l2, l1_l2, L1L2, get, serialize, deserialize
    from gennet_amd.keras.layers.noise import GaussianNoise, GaussianDropout, AlphaDropout
    from gennet_amd.keras.layers.pooling import MaxPooling1D, AveragePooling1D, GlobalAveragePooling1D, ...   # all eight pooling layers
    from gennet_amd.keras.layers.merge import Add, Subtract, Concatenate, Dot, add, dot, ...                   # all eight merge layers and functions
    from gennet_amd.keras.layers.recurrent import LSTM, GRU, SimpleRNN # also gennet_amd.keras.layers.LSTM, .GRU, .SimpleRNN
    from gennet_amd.keras.layers.wrappers import Bidirectional         # also gennet_amd.keras.layers.Bidirectional: over LSTM, GRU or SimpleRNN
    from gennet_amd.keras.layers.wrappers import TimeDistributed       # over Dense; also gennet_amd.keras.layers.TimeDistributed
    from gennet_amd.keras.layers.core import RepeatVector, Permute     # also gennet_amd.keras.layers.RepeatVector, .Permute
    from gennet_amd.keras.layers.convolutional import Cropping1D, ZeroPadding1D   # also gennet_amd.keras.layers.Cropping1D, .ZeroPadding1D
    from gennet_amd.keras.layers.dense_attention import Attention      # tf.keras 2.x; also gennet_amd.keras.layers.Attention
    from gennet_amd.keras.engine.topology import Layer
    from gennet_amd.keras.optimizers import Adam, SGD, RMSprop, Adagrad, Adadelta, Adamax   # Nadam: placeholder
    from gennet_amd.keras import backend as K
    from gennet_amd.keras.losses import logcosh, mean_absolute_error, mae, ...                # every name and alias of engine.LOSSES
    from gennet_amd.keras.metrics import categorical_accuracy, mae, mse, mape, msle, cosine   # and their long names
Every class executes on the HIP kernel library; see INTEGRATION.md.

The sub-module tree of the import lines is a name space over gennet_amd.engine / gennet_amd.layers and nothing more, so it is built here,
in one table, and registered in sys.modules (importing gennet_amd.keras makes every dotted path above resolvable); only `backend` has code
of its own.  Names the script imports but never instantiates on the BBH path (:33-43) resolve to placeholders whose constructor raises,
instead of silently running something else.
"""
import sys
import types

from .. import engine as _engine
from .. import layers as _layers
from .. import regularizers as _regularizers
from . import backend  # noqa: F401


def _placeholder(name, where):
    def __init__(self, *a, **k):
        raise NotImplementedError('%s is imported by bbhMahoGANy.py (%s) but never used on the BBH hot path; gennet_amd does not '
                                  'provide it' % (name, where))
    return type(name, (object,), {'__init__': __init__, '__doc__': 'placeholder for keras %s (not on the hot path)' % name})


def _unused(where, *names):
    return dict((n, _placeholder(n, 'bbhMahoGANy.py:' + where)) for n in names)


def _pooling_placeholder(name, where):
    """MaxPooling1D, AveragePooling1D, GlobalAveragePooling1D under the names bbhMahoGANy.py imports and never instantiates: the real classes are
    gennet_amd.layers.<Name> (= gennet_amd.keras.layers.pooling.<Name>, and what load_model builds); these import-line names keep refusing."""
    def __init__(self, *a, **k):
        raise NotImplementedError('%s under this name is the import of bbhMahoGANy.py:%s, which the script never instantiates, and it keeps refusing so '
                                  'that a script which starts to use it is noticed; the layer itself is gennet_amd.layers.%s (also '
                                  'gennet_amd.keras.layers.pooling.%s, and what load_model / model_from_json build)' % (name, where, name, name))
    return type(name, (object,), {'__init__': __init__, '__doc__': 'placeholder for the unused import of keras %s; the layer is gennet_amd.layers.%s'
                                                                   % (name, name)})


def _pick(mod, *names):
    return dict((n, getattr(mod, n)) for n in names)


_core = _pick(_layers, 'Activation', 'ActivityRegularization', 'Dense', 'Dropout', 'Flatten', 'Reshape', 'RepeatVector', 'Permute')
_norm = _pick(_layers, 'BatchNormalization', 'LayerNormalization')
_conv = dict(_pick(_layers, 'Conv1D', 'Conv2D', 'Conv2DTranspose', 'SeparableConv1D', 'UpSampling1D', 'MaxPooling2D', 'Cropping1D', 'ZeroPadding1D'),
             **_unused('37-38', 'UpSampling2D'))
_conv.update((n, _pooling_placeholder(n, '37-38')) for n in ('AveragePooling1D', 'MaxPooling1D'))
_pooling = _pick(_layers, 'MaxPooling1D', 'MaxPooling2D', 'AveragePooling1D', 'AveragePooling2D', 'GlobalAveragePooling1D', 'GlobalAveragePooling2D',
                 'GlobalMaxPooling1D', 'GlobalMaxPooling2D')
_act = dict(_pick(_layers, 'LeakyReLU', 'PReLU', 'ReLU', 'Softmax'), **_unused('39', 'ThresholdedReLU'))
_noise = _pick(_layers, 'GaussianNoise', 'GaussianDropout', 'AlphaDropout')
_merge = _pick(_layers, 'Add', 'Subtract', 'Multiply', 'Average', 'Maximum', 'Minimum', 'Concatenate', 'Dot',
               'add', 'subtract', 'multiply', 'average', 'maximum', 'minimum', 'concatenate', 'dot')
_recurrent = _pick(_layers, 'LSTM', 'GRU', 'SimpleRNN')
_wrappers = _pick(_layers, 'Bidirectional', 'TimeDistributed')
_attention = _pick(_layers, 'Attention')
_top = dict(_pick(_engine, 'Input'), **_pick(_layers, 'MyLayer'))
_top['GlobalAveragePooling1D'] = _pooling_placeholder('GlobalAveragePooling1D', '33-34')
_top.update(_pick(_layers, 'AveragePooling2D', 'GlobalAveragePooling2D', 'GlobalMaxPooling1D', 'GlobalMaxPooling2D'))
for _d in (_core, _norm, _conv, _act, _noise, _merge, _recurrent, _wrappers, _attention):
    _top.update((k, v) for k, v in _d.items() if v is _layers.__dict__.get(k))

_TREE = {
    'models': _pick(_engine, 'Model', 'Sequential', 'load_model', 'model_from_json'),
    'optimizers': dict(_pick(_engine, 'Adam', 'SGD', 'RMSprop', 'Adagrad', 'Adadelta', 'Adamax'), **_unused('43', 'Nadam')),
    'activations': dict(_layers.ACTIVATIONS),
    'regularizers': _pick(_regularizers, 'Regularizer', 'L1L2', 'l1', 'l2', 'l1_l2', 'serialize', 'deserialize', 'get'),
    'engine': {},
    'engine.topology': _pick(_engine, 'Layer'),
    'layers': _top,
    'layers.core': _core,
    'layers.normalization': _norm,
    'layers.convolutional': _conv,
    'layers.advanced_activations': _act,
    'layers.noise': _noise,
    'layers.pooling': _pooling,
    'layers.merge': _merge,
    'layers.recurrent': _recurrent,
    'layers.wrappers': _wrappers,
    'layers.dense_attention': _attention,
    'losses': dict((k, v) for k, v in _engine.LOSS_FUNCTIONS.items() if k != 'categorical_accuracy'),
    'metrics': dict((k, v) for k, v in _engine.LOSS_FUNCTIONS.items() if _engine._loss_name(v) in _engine.PASS_METRICS),
}


def _register():
    for dotted in sorted(_TREE):            # parents sort before their children
        m = types.ModuleType(__name__ + '.' + dotted, 'gennet_amd.keras facade: see gennet_amd/keras/__init__.py')
        m.__dict__.update(_TREE[dotted])
        m.__package__ = __name__ + '.' + dotted if any(k.startswith(dotted + '.') for k in _TREE) else (__name__ + '.' + dotted).rpartition('.')[0]
        if m.__package__ == m.__name__:
            m.__path__ = []                 # a package: `from gennet_amd.keras.layers.core import ...` walks through it
        sys.modules[m.__name__] = m
        parent, _, leaf = m.__name__.rpartition('.')
        setattr(sys.modules[parent], leaf, m)


_register()
