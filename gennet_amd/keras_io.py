"""Keras 2.x HDF5 persistence for gennet_amd models: the byte layout `model.save`,
`save_weights`, `load_weights` and `keras.models.load_model` use in bbhMahoGANy.py:1135-1142, :1171-1173, :1372-1375, so
that `.h5` files interchange with real Keras.  HDF5 itself comes from gennet_amd/h5lite.py (h5py is not in the image).

Layout (keras/engine/saving.py of Keras 2.2.4, restated; confirmed on the real Keras files the reference ships under
2_model_version/weight_version/):
  weights file : root attrs layer_names [S], backend, keras_version; one group per layer of `model.layers` with attr
                 weight_names [S] and one dataset per weight named by the weight ('dense_1/kernel:0' -> nested group);
  model file   : root attrs keras_version, backend, model_config (JSON), training_config (JSON);
                 group model_weights (as above); group optimizer_weights (attr weight_names + datasets:
                 the optimizer class' optimizer.weights: [iterations] + one array per trainable weight per state block, e.g.
                 Adam: iterations, m, v, then vhat ((1,)-shaped stubs without amsgrad); SGD: iterations, m; RMSprop: a;
                 engine.Optimizer._layout).
`model.layers` order: Sequential = layers as added (no InputLayer); functional Model = Keras' depth order (Network
._init_graph_network): depth = longest distance to an output, ties by post-order index of a DFS from the outputs.
A nested model is ONE layer whose weights are trainable_weights + non_trainable_weights (Keras' Layer.weights).
"""
import json

import numpy as np

from . import h5lite
from .regularizers import serialize as _reg
from .engine import Adam, Input, Layer, Model, Sequential, optimizer_from_config, to_snake_case  # noqa: F401

KERAS_VERSION = '2.2.4'
BACKEND = 'tensorflow'


# ---------------------------------------------------------------------------------------------------------------------
# model.layers and layer.weights in Keras' order
# ---------------------------------------------------------------------------------------------------------------------
class InputLayer(object):
    """Stand-in for keras.layers.InputLayer in `model.layers` / model_config of functional models (it has no weights)."""

    def __init__(self, sym):
        self.sym = sym
        self.name = sym.name
        self.trainable = False

    weights = ()


def _sym_graph(model):
    """Post-order DFS over the symbolic tensors from the outputs: [(tensor, layer-or-InputLayer)], each layer call once."""
    order, seen = [], set()

    def visit(t):
        if id(t) in seen:
            return
        seen.add(id(t))
        for s in t.inbound:
            visit(s)
        order.append(t)
    for t in model._sym_outputs:
        visit(t)
    return order


def top_layers(model):
    """`model.layers` as Keras orders them."""
    if isinstance(model, Sequential):
        return list(model._top)
    if getattr(model, '_sym_outputs', None) is None:
        return list(model.layers)
    order = _sym_graph(model)                       # nodes_in_decreasing_depth of Keras' build_map
    index = {id(t): i for i, t in enumerate(order)}
    depth = {}
    for t in reversed(order):
        d = depth.setdefault(id(t), 0)
        for s in t.inbound:
            depth[id(s)] = max(depth.get(id(s), 0), d + 1)
    # a layer called once = one node; depth of the layer = depth of its node
    items = sorted(order, key=lambda t: (-depth[id(t)], index[id(t)]))
    return [InputLayer(t) if t.layer is None else t.layer for t in items]


def _tw(layer):
    if isinstance(layer, InputLayer) or not layer.trainable:
        return []
    if isinstance(layer, Model):
        out = []
        for l in top_layers(layer):
            out += _tw(l)
        return out
    return list(layer.params)


def _ntw(layer):
    if isinstance(layer, InputLayer):
        return []
    if isinstance(layer, Model):
        w = []
        for l in top_layers(layer):
            w += _ntw(l)
        if not layer.trainable:
            t = []
            for l in top_layers(layer):
                t += _tw(l)
            return t + w
        return w
    return list(layer.buffers) if layer.trainable else list(layer.params) + list(layer.buffers)


def keras_weights(layer):
    """`layer.weights` of Keras: trainable_weights + non_trainable_weights (differs from per-layer order for nested models)."""
    return _tw(layer) + _ntw(layer)


def _wname(p):
    return p.name + ':0'


# ---------------------------------------------------------------------------------------------------------------------
# weights <-> HDF5 groups
# ---------------------------------------------------------------------------------------------------------------------
def save_weights_to_group(g, layers):
    g.attrs['layer_names'] = np.array([l.name.encode('utf-8') for l in layers], dtype='S') if layers else np.zeros((0,), 'S1')
    g.attrs['backend'] = BACKEND.encode('utf-8')
    g.attrs['keras_version'] = KERAS_VERSION.encode('utf-8')
    for l in layers:
        lg = g.create_group(l.name)
        ws = keras_weights(l)
        names = [_wname(p) for p in ws]
        if len(set(names)) != len(names):
            raise ValueError('layer %s has duplicate weight names' % l.name)
        lg.attrs['weight_names'] = np.array([n.encode('utf-8') for n in names], dtype='S') if names else np.zeros((0,), np.float64)
        for p, n in zip(ws, names):
            lg.create_dataset(n, np.ascontiguousarray(p.numpy(), dtype=np.float32).reshape(p.shape))      # a () weight stays ()


def _decode_list(a):
    if a is None:
        return []
    return [x.decode('utf-8') if isinstance(x, bytes) else str(x) for x in np.asarray(a).ravel().tolist()]


def load_weights_from_group(g, layers):
    """keras.engine.saving.load_weights_from_hdf5_group: match the layers that HAVE weights, in order; check counts and shapes."""
    layer_names = _decode_list(g.attrs.get('layer_names'))
    file_layers = []
    for name in layer_names:
        wn = _decode_list(g[name].attrs.get('weight_names'))
        if wn:
            file_layers.append((name, wn))
    model_layers = [l for l in layers if keras_weights(l)]
    if len(file_layers) != len(model_layers):
        raise ValueError('You are trying to load a weight file containing %d layers into a model with %d layers.' % (len(file_layers), len(model_layers)))
    todo = []
    for (name, wn), l in zip(file_layers, model_layers):
        ws = keras_weights(l)
        if len(wn) != len(ws):
            raise ValueError('Layer %s (in the file: %s) expects %d weight(s), but the saved weights have %d element(s).' % (l.name, name, len(ws), len(wn)))
        for p, n in zip(ws, wn):
            v = g[name][n].value
            if tuple(v.shape) != tuple(p.shape):
                raise ValueError('Layer %s: weight %s has shape %s in the file, %s in the model' % (l.name, n, tuple(v.shape), tuple(p.shape)))
            todo.append((p, v))
    for p, v in todo:        # nothing is assigned unless everything matched
        p.assign(np.asarray(v, np.float32))


# ---------------------------------------------------------------------------------------------------------------------
# layer / model configs (keras get_config / from_config)
# ---------------------------------------------------------------------------------------------------------------------
_GLOROT = {'class_name': 'VarianceScaling', 'config': {'scale': 1.0, 'mode': 'fan_avg', 'distribution': 'uniform', 'seed': None}}
_ZEROS = {'class_name': 'Zeros', 'config': {}}
_ORTHOGONAL = {'class_name': 'Orthogonal', 'config': {'gain': 1.0, 'seed': None}}
_ONES = {'class_name': 'Ones', 'config': {}}
_ACT_OF_SPEC = {'relu': 'relu', 'tanh': 'tanh', 'sigmoid': 'sigmoid', 'linear': 'linear', 'softmax': 'softmax'}


def _kernel_part(layer):
    """the keys Dense and the conv layers share; a regularizer as keras serializes it: {'class_name': 'L1L2', 'config': {'l1', 'l2'}} or None"""
    return {'use_bias': True, 'kernel_initializer': _GLOROT, 'bias_initializer': _ZEROS, 'kernel_regularizer': _reg(layer.kernel_regularizer),
            'bias_regularizer': _reg(layer.bias_regularizer), 'activity_regularizer': _reg(layer.activity_regularizer), 'kernel_constraint': None,
            'bias_constraint': None}


def layer_config(layer):
    from . import layers as L
    cfg = {'name': layer.name, 'trainable': bool(layer.trainable)}
    if layer.input_shape_arg is not None:
        cfg['batch_input_shape'] = [None] + list(layer.input_shape_arg)
        cfg['dtype'] = 'float32'
    if isinstance(layer, L.Dense):
        cfg.update(units=layer.units, activation=_ACT_OF_SPEC[layer.activation[0]], **_kernel_part(layer))
    elif isinstance(layer, L.Conv1D):
        cfg.update(filters=layer.filters, kernel_size=[layer.k], strides=[layer.stride], padding=layer.padding, data_format='channels_last',
                   dilation_rate=[layer.dilation], activation=_ACT_OF_SPEC[layer.activation[0]], **_kernel_part(layer))
    elif isinstance(layer, L.Conv2DTranspose):
        # the keys (and values) keras 2.1.6 wrote for the reference's g_model.hdf5: no dilation_rate / output_padding
        cfg.update(filters=layer.filters, kernel_size=[1, layer.k], strides=[1, layer.stride], padding=layer.padding, data_format='channels_last',
                   activation=_ACT_OF_SPEC[layer.activation[0]], **_kernel_part(layer))
    elif isinstance(layer, L.Conv2D):
        cfg.update(filters=layer.filters, kernel_size=[layer.kh, layer.kw], strides=[layer.sh, layer.sw], padding=layer.padding,
                   data_format='channels_last', dilation_rate=[1, 1], activation=_ACT_OF_SPEC[layer.activation[0]], **_kernel_part(layer))
    elif isinstance(layer, L.BatchNormalization):
        cfg.update(axis=layer.axis, momentum=layer.momentum, epsilon=layer.epsilon, center=True, scale=True, beta_initializer=_ZEROS, gamma_initializer=_ONES,
                   moving_mean_initializer=_ZEROS, moving_variance_initializer=_ONES, beta_regularizer=_reg(layer.beta_regularizer), gamma_regularizer=_reg(layer.gamma_regularizer),
                   beta_constraint=None, gamma_constraint=None)
    elif isinstance(layer, L.LayerNormalization):      # tf.keras 2.x layers/normalization.py: axis is the list of non-negative axes after build
        cfg.update(axis=list(layer.axis) if isinstance(layer.axis, list) else layer.axis, epsilon=layer.epsilon, center=layer.center, scale=layer.scale,
                   beta_initializer=_ZEROS, gamma_initializer=_ONES, beta_regularizer=_reg(layer.beta_regularizer),
                   gamma_regularizer=_reg(layer.gamma_regularizer), beta_constraint=None, gamma_constraint=None)
    elif isinstance(layer, L.PReLU):
        cfg.update(alpha_initializer=_ZEROS, alpha_regularizer=_reg(layer.alpha_regularizer), alpha_constraint=None, shared_axes=None)
    elif isinstance(layer, L.LeakyReLU):
        cfg.update(alpha=layer.act_spec[1])
    elif isinstance(layer, L.ReLU):
        cfg.update(max_value=(layer.act_spec[1] if layer.act_spec[0] == 'relu_max' else None), negative_slope=0.0, threshold=0.0)
    elif isinstance(layer, L.Activation):
        cfg.update(activation='softmax' if layer.softmax else _ACT_OF_SPEC[layer.act_spec[0]])
    elif isinstance(layer, L.Softmax):
        cfg.update(axis=layer.axis)
    elif isinstance(layer, L.ActivityRegularization):
        cfg.update(l1=layer.l1, l2=layer.l2)
    elif isinstance(layer, L.Dropout):
        cfg.update(rate=layer.rate, noise_shape=None, seed=None)
    elif isinstance(layer, L.GaussianNoise):
        cfg.update(stddev=layer.stddev)
    elif isinstance(layer, (L.GaussianDropout, L.AlphaDropout)):
        cfg.update(rate=layer.rate)
    elif isinstance(layer, L.Reshape):
        cfg.update(target_shape=list(getattr(layer, 'target_shape_arg', layer.target_shape)))
    elif isinstance(layer, L.Flatten):
        cfg.update(data_format='channels_last')
    elif isinstance(layer, L.UpSampling1D):
        cfg.update(size=2)
    elif isinstance(layer, L._Pooling):          # keras 2.2.4 layers/pooling.py: lists of length 1 (1-D) or 2 (2-D)
        cfg.update(pool_size=list(layer.pool_size), padding=layer.padding, strides=list(layer.strides), data_format='channels_last')
    elif isinstance(layer, L._GlobalPooling):
        cfg.update(data_format='channels_last')
    elif isinstance(layer, L.Concatenate):       # keras 2.2.4 layers/merge.py: the six element-wise layers write the base config only
        cfg.update(axis=layer.axis)
    elif isinstance(layer, L.Dot):               # axes as keras writes it: the int, or the pair as a list
        cfg.update(axes=layer.axes if isinstance(layer.axes, int) else list(layer.axes), normalize=layer.normalize)
    elif isinstance(layer, L.Attention):         # tf.keras 2.x layers/dense_attention.py: BaseDenseAttention writes causal and dropout, Attention use_scale
        cfg.update(use_scale=layer.use_scale, causal=layer.causal, dropout=0.0)
    elif isinstance(layer, (L.LSTM, L.GRU, L.SimpleRNN)):    # the keys of keras 2.2.4 layers/recurrent.py LSTM / GRU / SimpleRNN.get_config
        cfg.update(return_sequences=layer.return_sequences, return_state=False, go_backwards=layer.go_backwards, stateful=False, unroll=layer.unroll,
                   units=layer.units, activation=layer.activation, use_bias=True,
                   kernel_initializer=_GLOROT, recurrent_initializer=_ORTHOGONAL, bias_initializer=_ZEROS,
                   kernel_regularizer=_reg(layer.kernel_regularizer), recurrent_regularizer=_reg(layer.recurrent_regularizer),
                   bias_regularizer=_reg(layer.bias_regularizer), activity_regularizer=_reg(layer.activity_regularizer), kernel_constraint=None,
                   recurrent_constraint=None, bias_constraint=None, dropout=0.0, recurrent_dropout=0.0)
        if not isinstance(layer, L.SimpleRNN):   # SimpleRNN writes neither
            cfg.update(recurrent_activation=layer.recurrent_activation, implementation=layer.implementation)
        if isinstance(layer, L.LSTM):
            cfg.update(unit_forget_bias=layer.unit_forget_bias)
        elif isinstance(layer, L.GRU):
            cfg.update(reset_after=layer.reset_after)
    elif isinstance(layer, L.SeparableConv1D):   # keras 2.2.4 layers/convolutional.py: _SeparableConv.get_config, rank and the kernel_* keys popped
        cfg.update(filters=layer.filters, kernel_size=[layer.k], strides=[layer.stride], padding=layer.padding, data_format='channels_last',
                   dilation_rate=[layer.dilation], activation=_ACT_OF_SPEC[layer.activation[0]], use_bias=True, bias_initializer=_ZEROS,
                   bias_regularizer=_reg(layer.bias_regularizer), activity_regularizer=_reg(layer.activity_regularizer), bias_constraint=None,
                   depth_multiplier=layer.depth_multiplier, depthwise_initializer=_GLOROT, pointwise_initializer=_GLOROT,
                   depthwise_regularizer=_reg(layer.depthwise_regularizer), pointwise_regularizer=_reg(layer.pointwise_regularizer),
                   depthwise_constraint=None, pointwise_constraint=None)
    elif isinstance(layer, L.Bidirectional):     # keras 2.2.4 layers/wrappers.py: Wrapper.get_config's 'layer' entry and merge_mode
        cfg.update(layer={'class_name': layer.layer.__class__.__name__, 'config': layer_config(layer.layer)}, merge_mode=layer.merge_mode)
    elif isinstance(layer, L.TimeDistributed):   # keras 2.2.4 layers/wrappers.py: Wrapper.get_config, the base config and the 'layer' entry
        cfg.update(layer={'class_name': layer.layer.__class__.__name__, 'config': layer_config(layer.layer)})
    elif isinstance(layer, L.RepeatVector):      # keras 2.2.4 layers/core.py
        cfg.update(n=layer.n)
    elif isinstance(layer, L.Permute):
        cfg.update(dims=list(layer.dims))
    elif isinstance(layer, L.Cropping1D):        # keras 2.2.4 layers/convolutional.py: the pair, as a list in JSON
        cfg.update(cropping=list(layer.cropping))
    elif isinstance(layer, L.ZeroPadding1D):
        cfg.update(padding=list(layer.padding))
    # custom layers (MyLayer, bbhMahoGANy.py:164-188, defines no get_config): base config only, like Keras writes for them
    return cfg


def model_config(model):
    """{'class_name': 'Sequential' | 'Model', 'config': ...} in the Keras 2.2.4 form."""
    def entry(l):
        if isinstance(l, Model):
            return model_config(l)
        return {'class_name': l.__class__.__name__, 'config': layer_config(l)}

    if isinstance(model, Sequential):
        return {'class_name': 'Sequential', 'config': {'name': model.name, 'layers': [entry(l) for l in model._top]}}
    if getattr(model, '_sym_outputs', None) is None:
        raise ValueError('model %s was not built through Sequential.add or Model(inputs=, outputs=)' % model.name)
    order = _sym_graph(model)
    name_of = {id(t): (t.name if t.layer is None else t.layer.name) for t in order}
    layers = []
    for l in top_layers(model):
        if isinstance(l, InputLayer):
            layers.append({'name': l.name, 'class_name': 'InputLayer', 'inbound_nodes': [],
                           'config': {'batch_input_shape': [None] + list(l.sym.shape), 'dtype': 'float32', 'sparse': False, 'name': l.name}})
            continue
        t = [s for s in order if s.layer is l][0]
        e = entry(l)
        e['name'] = l.name
        e['inbound_nodes'] = [[[name_of[id(s)], 0, 0, {}] for s in t.inbound]]
        layers.append(e)
    return {'class_name': 'Model', 'config': {'name': model.name, 'layers': layers,
                                              'input_layers': [[t.name, 0, 0] for t in model._sym_inputs],
                                              'output_layers': [[name_of[id(t)], 0, 0] for t in model._sym_outputs]}}


def _layer_from_config(class_name, cfg, custom_objects):
    from . import layers as L
    custom_objects = custom_objects or {}
    kw = {'name': cfg.get('name'), 'trainable': cfg.get('trainable', True)}
    if cfg.get('batch_input_shape') is not None:
        kw['input_shape'] = tuple(cfg['batch_input_shape'][1:])
    if class_name in custom_objects:
        obj = custom_objects[class_name]
        if isinstance(obj, Layer):
            layer = obj
        else:
            layer = obj(**{k: v for k, v in cfg.items() if k not in ('batch_input_shape', 'dtype')}) if isinstance(obj, type) else obj(cfg)
        if layer.input_shape_arg is None and 'input_shape' in kw:
            layer.input_shape_arg = kw['input_shape']
        return layer

    def init_ok(c):
        if c is None or c == 'glorot_uniform':
            return
        if isinstance(c, dict) and (c.get('class_name') == 'GlorotUniform' or (c.get('class_name') == 'VarianceScaling' and c['config'].get('mode') == 'fan_avg'
                                                                                and c['config'].get('distribution') == 'uniform')):
            return
        raise NotImplementedError('kernel_initializer %r' % (c,))

    def regs(*keys):                       # the layer constructors take the config dicts as they are (regularizers.get)
        return dict((k, cfg.get(k)) for k in keys)
    kregs = regs('kernel_regularizer', 'bias_regularizer', 'activity_regularizer')

    if class_name == 'Dense':
        init_ok(cfg.get('kernel_initializer'))
        return L.Dense(cfg['units'], activation=cfg.get('activation'), use_bias=cfg.get('use_bias', True), **kregs, **kw)
    if class_name == 'Conv1D':
        init_ok(cfg.get('kernel_initializer'))
        return L.Conv1D(cfg['filters'], cfg['kernel_size'], strides=cfg.get('strides', 1), padding=cfg.get('padding', 'valid'), activation=cfg.get('activation'),
                        use_bias=cfg.get('use_bias', True), dilation_rate=cfg.get('dilation_rate', 1), **kregs, **kw)
    if class_name == 'Conv2D':
        init_ok(cfg.get('kernel_initializer'))
        return L.Conv2D(cfg['filters'], tuple(cfg['kernel_size']), strides=tuple(cfg.get('strides', (1, 1))), padding=cfg.get('padding', 'valid'),
                        activation=cfg.get('activation'), use_bias=cfg.get('use_bias', True), **kregs, **kw)
    if class_name == 'Conv2DTranspose':
        init_ok(cfg.get('kernel_initializer'))
        dil = cfg.get('dilation_rate', [1, 1])
        return L.Conv2DTranspose(cfg['filters'], tuple(cfg['kernel_size']), strides=tuple(cfg.get('strides', (1, 1))), padding=cfg.get('padding', 'valid'),
                                 output_padding=cfg.get('output_padding'), data_format=cfg.get('data_format'),
                                 dilation_rate=tuple(dil) if isinstance(dil, (list, tuple)) else dil, activation=cfg.get('activation'),
                                 use_bias=cfg.get('use_bias', True), **kregs, **kw)
    if class_name == 'BatchNormalization':
        return L.BatchNormalization(axis=cfg.get('axis', -1), momentum=cfg.get('momentum', 0.99), epsilon=cfg.get('epsilon', 1e-3),
                                    **regs('beta_regularizer', 'gamma_regularizer'), **kw)
    if class_name == 'LayerNormalization':       # dtype is accepted and ignored; the layer refuses initializers and constraints it does not run, by name
        keys = ('beta_initializer', 'gamma_initializer', 'beta_constraint', 'gamma_constraint')
        return L.LayerNormalization(axis=cfg.get('axis', -1), epsilon=cfg.get('epsilon', 1e-3), center=cfg.get('center', True), scale=cfg.get('scale', True),
                                    **dict((k, cfg[k]) for k in keys if k in cfg), **regs('beta_regularizer', 'gamma_regularizer'), **kw)
    if class_name == 'PReLU':
        return L.PReLU(alpha_initializer=cfg.get('alpha_initializer', 'zeros'), shared_axes=cfg.get('shared_axes'), **regs('alpha_regularizer'), **kw)
    if class_name == 'LeakyReLU':
        return L.LeakyReLU(alpha=cfg.get('alpha', 0.3), **kw)
    if class_name == 'ReLU':
        return L.ReLU(max_value=cfg.get('max_value'), negative_slope=cfg.get('negative_slope', 0.0), threshold=cfg.get('threshold', 0.0), **kw)
    if class_name == 'Activation':
        return L.Activation(cfg['activation'], **kw)
    if class_name == 'Softmax':
        return L.Softmax(axis=cfg.get('axis', -1), **kw)
    if class_name == 'ActivityRegularization':
        return L.ActivityRegularization(l1=cfg.get('l1', 0.), l2=cfg.get('l2', 0.), **kw)
    if class_name == 'Dropout':
        return L.Dropout(cfg['rate'], **kw)
    if class_name == 'GaussianNoise':
        return L.GaussianNoise(cfg['stddev'], **kw)
    if class_name == 'GaussianDropout':
        return L.GaussianDropout(cfg['rate'], **kw)
    if class_name == 'AlphaDropout':
        return L.AlphaDropout(cfg['rate'], noise_shape=cfg.get('noise_shape'), seed=cfg.get('seed'), **kw)
    if class_name == 'Reshape':
        return L.Reshape(tuple(cfg['target_shape']), **kw)
    if class_name == 'Flatten':
        return L.Flatten(**kw)
    if class_name == 'UpSampling1D':
        return L.UpSampling1D(size=cfg.get('size', 2), **kw)
    if class_name in ('MaxPooling2D', 'AveragePooling2D', 'MaxPooling1D', 'AveragePooling1D'):
        # data_format: absent in the 1-D configs of older keras; 'channels_first' is refused by the layer
        return getattr(L, class_name)(pool_size=cfg.get('pool_size'), strides=cfg.get('strides'), padding=cfg.get('padding', 'valid'),
                                      data_format=cfg.get('data_format'), **kw)
    if class_name in ('GlobalAveragePooling1D', 'GlobalAveragePooling2D', 'GlobalMaxPooling1D', 'GlobalMaxPooling2D'):
        return getattr(L, class_name)(data_format=cfg.get('data_format'), **kw)
    if class_name in ('Add', 'Subtract', 'Multiply', 'Average', 'Maximum', 'Minimum'):
        return getattr(L, class_name)(**kw)
    if class_name == 'Concatenate':
        return L.Concatenate(axis=cfg.get('axis', -1), **kw)
    if class_name == 'Dot':
        return L.Dot(axes=cfg['axes'], normalize=cfg.get('normalize', False), **kw)
    if class_name == 'Attention':                # dtype is accepted and ignored; the layer refuses a dropout other than 0 by name
        return L.Attention(use_scale=cfg.get('use_scale', False), causal=cfg.get('causal', False), dropout=cfg.get('dropout', 0.0), **kw)
    if class_name in ('LSTM', 'GRU'):            # the layer itself refuses what it does not run, naming the key
        keys = ('activation', 'recurrent_activation', 'use_bias', 'kernel_initializer', 'recurrent_initializer', 'bias_initializer',
                'unit_forget_bias' if class_name == 'LSTM' else 'reset_after',
                'kernel_regularizer', 'recurrent_regularizer', 'bias_regularizer', 'activity_regularizer', 'kernel_constraint', 'recurrent_constraint',
                'bias_constraint', 'dropout', 'recurrent_dropout', 'implementation', 'return_sequences', 'return_state', 'go_backwards', 'stateful',
                'unroll')
        return getattr(L, class_name)(cfg['units'], **dict((k, cfg[k]) for k in keys if k in cfg), **kw)
    if class_name == 'SimpleRNN':                # as LSTM / GRU, without recurrent_activation and implementation
        keys = ('activation', 'use_bias', 'kernel_initializer', 'recurrent_initializer', 'bias_initializer', 'kernel_regularizer',
                'recurrent_regularizer', 'bias_regularizer', 'activity_regularizer', 'kernel_constraint', 'recurrent_constraint', 'bias_constraint',
                'dropout', 'recurrent_dropout', 'return_sequences', 'return_state', 'go_backwards', 'stateful', 'unroll')
        return L.SimpleRNN(cfg['units'], **dict((k, cfg[k]) for k in keys if k in cfg), **kw)
    if class_name == 'SeparableConv1D':          # the layer itself refuses what it does not run, naming the key
        keys = ('strides', 'padding', 'data_format', 'dilation_rate', 'depth_multiplier', 'activation', 'use_bias', 'depthwise_initializer',
                'pointwise_initializer', 'bias_initializer', 'depthwise_regularizer', 'pointwise_regularizer', 'bias_regularizer',
                'activity_regularizer', 'depthwise_constraint', 'pointwise_constraint', 'bias_constraint')
        return L.SeparableConv1D(cfg['filters'], cfg['kernel_size'], **dict((k, cfg[k]) for k in keys if k in cfg), **kw)
    if class_name == 'Bidirectional':            # the inner layer through the LSTM / GRU / SimpleRNN paths above, with its own name and go_backwards
        inner = cfg['layer']
        if inner['class_name'] not in ('LSTM', 'GRU', 'SimpleRNN'):
            raise ValueError('Bidirectional wraps an LSTM or a GRU, or a SimpleRNN, not %s' % inner['class_name'])
        return L.Bidirectional(_layer_from_config(inner['class_name'], inner['config'], None), merge_mode=cfg.get('merge_mode', 'concat'), **kw)
    if class_name == 'TimeDistributed':          # the inner layer through its own path above; the wrapper refuses what is not a Dense, naming it
        inner = cfg['layer']
        return L.TimeDistributed(_layer_from_config(inner['class_name'], inner['config'], None), **kw)
    if class_name == 'RepeatVector':
        return L.RepeatVector(cfg['n'], **kw)
    if class_name == 'Permute':
        return L.Permute(tuple(cfg['dims']), **kw)
    if class_name == 'Cropping1D':
        c = cfg.get('cropping', (1, 1))
        return L.Cropping1D(cropping=tuple(c) if isinstance(c, list) else c, **kw)
    if class_name == 'ZeroPadding1D':
        p = cfg.get('padding', 1)
        return L.ZeroPadding1D(padding=tuple(p) if isinstance(p, list) else p, **kw)
    raise ValueError('Unknown layer: %s (pass it through custom_objects={%r: ...})' % (class_name, class_name))


def model_from_config(config, custom_objects=None):
    """keras.models.model_from_config for Sequential / functional Model configs of Keras 2.0 - 2.2 (both Sequential forms)."""
    cls, cfg = config['class_name'], config['config']
    if cls == 'Sequential':
        entries = cfg if isinstance(cfg, list) else cfg['layers']
        m = Sequential(name=None if isinstance(cfg, list) else cfg.get('name'))
        for e in entries:
            if e['class_name'] in ('Sequential', 'Model') and e['class_name'] not in (custom_objects or {}):
                m.add(model_from_config(e, custom_objects))
            elif e['class_name'] == 'InputLayer':
                continue
            else:
                m.add(_layer_from_config(e['class_name'], e['config'], custom_objects))
        return m
    if cls == 'Model':
        tensors = {}
        pending = list(cfg['layers'])
        while pending:
            progressed = False
            for e in list(pending):
                if e['class_name'] == 'InputLayer':
                    tensors[e['name']] = Input(shape=tuple(e['config']['batch_input_shape'][1:]), name=e['name'])
                elif len(e['inbound_nodes']) != 1:
                    raise NotImplementedError('layer %s is called %d times; shared layers are not supported' % (e['name'], len(e['inbound_nodes'])))
                elif all(ref[0] in tensors for ref in e['inbound_nodes'][0]):
                    ins = [tensors[ref[0]] for ref in e['inbound_nodes'][0]]
                    layer = model_from_config(e, custom_objects) if e['class_name'] in ('Sequential', 'Model') else _layer_from_config(e['class_name'], e['config'], custom_objects)
                    tensors[e['name']] = layer(ins[0] if len(ins) == 1 else ins)       # several inbound tensors: a merge layer (any other layer refuses the list)
                else:
                    continue
                pending.remove(e)
                progressed = True
            if not progressed:
                raise ValueError('model config has a cycle or a dangling inbound reference: %s' % [e['name'] for e in pending])
        ins = [tensors[r[0]] for r in cfg['input_layers']]
        outs = [tensors[r[0]] for r in cfg['output_layers']]
        return Model(inputs=ins if len(ins) > 1 else ins[0], outputs=outs if len(outs) > 1 else outs[0], name=cfg.get('name'))
    raise ValueError('cannot build a model from class_name %r' % cls)


# ---------------------------------------------------------------------------------------------------------------------
# files
# ---------------------------------------------------------------------------------------------------------------------
def is_hdf5(path):
    with open(path, 'rb') as fh:
        return fh.read(8) == h5lite.SIGNATURE


STATE_GROUP = 'gennet_amd_state'      # private root group (not a keras layer group: keras' loaders only visit attrs['layer_names'])


def _bn_layers(model):
    from .layers import BatchNormalization
    return [l for l in model.layers if isinstance(l, BatchNormalization)]        # over any axis (is_batchnorm: the channel ones only)


def save_private_state(root, model):
    """BatchNormalization's zero-debias shadow variables (layers.BatchNormalization): TF graph variables that keras itself never saves.
    Written to <STATE_GROUP>/<layer>/<training model>/{biased_mean, biased_var, local_step} so that a run resumed from a file written
    HERE continues the same moving averages; a file from real keras has no such group and the state restarts at zero, as in keras."""
    bns = [l for l in _bn_layers(model) if l.zero_debias]
    if not bns:
        return
    g = root.create_group(STATE_GROUP)
    for l in bns:
        lg = g.create_group(l.name)
        for site, (bm, bv, step) in sorted(l.zero_debias.items()):
            sg = lg.create_group(site)
            sg.create_dataset('biased_mean', np.ascontiguousarray(bm.cpu().numpy(), np.float32))
            sg.create_dataset('biased_var', np.ascontiguousarray(bv.cpu().numpy(), np.float32))
            sg.create_dataset('local_step', np.asarray([step], np.int64))


def load_private_state(f, model):
    from .engine import to_device
    for l in _bn_layers(model):
        l.zero_debias = {}                       # keras semantics for files without the private group: shadow variables restart at zero
    if STATE_GROUP not in f:
        return
    g = f[STATE_GROUP]
    for l in _bn_layers(model):
        if l.name not in g:
            continue
        for site, sg in g[l.name].items():
            l.zero_debias[site] = [to_device(sg['biased_mean'].value), to_device(sg['biased_var'].value), int(np.asarray(sg['local_step'].value).reshape(-1)[0])]


def _write(w, path, writer):
    """The tree `w` holds host copies only: with a hostio.BackgroundWriter the serialisation + file write leaves the caller's thread."""
    if writer is None:
        w.save(path)
    else:
        writer.submit(w.save, path)


def save_weights(model, path, writer=None):
    w = h5lite.Writer()
    save_weights_to_group(w.root, top_layers(model))
    save_private_state(w.root, model)
    _write(w, path, writer)


def load_weights(model, path):
    f = h5lite.File(path)
    g = f['model_weights'] if 'layer_names' not in f.attrs and 'model_weights' in f else f
    load_weights_from_group(g, top_layers(model))
    load_private_state(f, model)


def _loss_json(loss):
    if isinstance(loss, (list, tuple)):
        return [_loss_json(l) for l in loss]
    return loss if isinstance(loss, str) else getattr(loss, '__name__', str(loss))


def save_model(model, path, include_optimizer=True, writer=None):
    w = h5lite.Writer()
    w.root.attrs['keras_version'] = KERAS_VERSION.encode('utf-8')
    w.root.attrs['backend'] = BACKEND.encode('utf-8')
    w.root.attrs['model_config'] = json.dumps(model_config(model)).encode('utf-8')
    save_weights_to_group(w.root.create_group('model_weights'), top_layers(model))
    opt = model.optimizer
    if include_optimizer and opt is not None:
        tc = {
            'optimizer_config': {'class_name': type(opt).__name__, 'config': opt.get_config()},
            'loss': _loss_json(model.loss), 'metrics': _loss_json(list(model.metrics or [])), 'sample_weight_mode': None,
            'loss_weights': getattr(model, 'loss_weights', None)}
        if getattr(model, 'weighted_metrics', None):  # only then: every file of a model compiled without them keeps its bytes
            tc['weighted_metrics'] = _loss_json(list(model.weighted_metrics))
        w.root.attrs['training_config'] = json.dumps(tc).encode('utf-8')
        if opt.state is not None and model._train_params:
            # keras: optimizer.weights in model.trainable_weights order -- [iterations] (if the class saves it) + one block per state array;
            # names in the scheme of a first compile, training/<Class>/Variable[_k]:0 (readers go by the weight_names order, never by name)
            og = w.root.create_group('optimizer_weights')
            cls = type(opt).__name__
            vals = opt.get_keras_weights(model._keras_train_order())
            names = []
            if opt.SAVES_ITERATIONS:
                names.append('%s/iterations:0' % cls)
            names += ['training/%s/Variable%s:0' % (cls, '' if k == 0 else '_%d' % k) for k in range(len(vals) - len(names))]
            for n, a in zip(names, vals):
                og.create_dataset(n, a if n.endswith('iterations:0') else np.asarray(a, np.float32))
            og.attrs['weight_names'] = np.array([n.encode('utf-8') for n in names], dtype='S')
    save_private_state(w.root, model)
    _write(w, path, writer)


def load_model(path, custom_objects=None, compile=True):
    f = h5lite.File(path)
    mc = f.attrs.get('model_config')
    if mc is None:
        raise ValueError('No model found in config file.')
    model = model_from_config(json.loads(mc.decode('utf-8') if isinstance(mc, bytes) else mc), custom_objects)
    load_weights_from_group(f['model_weights'], top_layers(model))
    load_private_state(f, model)
    tc = f.attrs.get('training_config')
    if compile and tc is not None:
        tc = json.loads(tc.decode('utf-8') if isinstance(tc, bytes) else tc)
        # any of engine.OPTIMIZERS with its own config, clipnorm / clipvalue included.  RMSprop, Adagrad and Adadelta files carry no iteration
        # count (Keras 2.2.4 does not save it): a resumed run restarts at iterations = 0, and with decay > 0 restarts the decay schedule
        model.compile(loss=tc['loss'], optimizer=optimizer_from_config(tc['optimizer_config']), metrics=tc.get('metrics') or [],
                      loss_weights=tc.get('loss_weights'), **({'weighted_metrics': tc['weighted_metrics']} if tc.get('weighted_metrics') else {}))
        if 'optimizer_weights' in f:
            og = f['optimizer_weights']
            names = _decode_list(og.attrs.get('weight_names'))
            vals = [og[n].value for n in names]
            model._pending_optimizer_weights = vals      # applied when the optimizer state is bound (first device use)
    return model


def load_optimizer_weights(model, path):
    """The optimizer state (optimizer_weights) of the model file `path` into the compiled `model`, whose optimizer must be of the class the file
    records: what keras.models.load_model restores, for a model that is rebuilt and compiled by the caller (scripts/bbh_train.py --old-model).
    Applied at the first device step, or now if the optimizer state is already bound.  A file without optimizer_weights leaves the state alone."""
    f = h5lite.File(path)
    tc = f.attrs.get('training_config')
    if tc is None or 'optimizer_weights' not in f:
        return False
    oc = json.loads(tc.decode('utf-8') if isinstance(tc, bytes) else tc)['optimizer_config']
    if oc['class_name'] != type(model.optimizer).__name__:
        raise ValueError('%s holds %s state; the model is compiled with %s' % (path, oc['class_name'], type(model.optimizer).__name__))
    og = f['optimizer_weights']
    vals = [og[n].value for n in _decode_list(og.attrs.get('weight_names'))]
    if getattr(model, '_bound', False):
        model.optimizer.set_keras_weights(model._keras_train_order(), vals)
    else:
        model._pending_optimizer_weights = vals
    return True
