"""Keras-style model engine over the HIP kernel library: Layer / Input / Sequential / Model, compile(),
train_on_batch(), predict(), fit(), weight persistence.

Mirrors the Keras 2.2.4 surface that BBH_version/bbhMahoGANy.py uses:
  * Sequential().add(layer | model), functional Input(shape) -> Layer(...)(tensor) -> Model(inputs=, outputs=[...], name=)
    (bbhMahoGANy.py:221-295, :357-404, :432-498, :516-518, :536-538)
  * model.trainable / layer.trainable assignment with COLLECT-AT-COMPILE semantics (:797-809, :1104-1115)
  * compile(loss=, optimizer=Adam(lr=, beta_1=), metrics=['accuracy']) (:1101-1119); one optimizer state per compiled model
  * train_on_batch(x, y) -> [loss, *metrics] python floats, keras ordering for multi-output models (:1165, :1292, :1296)
  * every Keras loss name / alias / keras.losses callable, loss_weights=[...], several metrics; test_on_batch, evaluate, predict_on_batch
    (ops.loss_pass); sample_weight=, class_weight=, compile(weighted_metrics=) (ops.loss_pass_weighted; section 8f)
  * keras.regularizers on weights (*_regularizer keywords) and outputs (activity_regularizer, ActivityRegularization): their penalties in
    entry 0 of train_on_batch / test_on_batch / evaluate, their gradient terms before the optimizer's clipping (ops.reg_pass; section 8l)
  * predict(x) -> ndarray | [ndarray] (default batch_size 32) (:1185, :1248, :1343); learning phase 1 in train_on_batch for
    the WHOLE graph, 0 in predict
  * save / save_weights / load_weights / load_model (:1135-1142, :1173, :1373-1375)

Not a tracing compiler: a model is a flat list of nodes executed eagerly, one or two HIP kernels per node, with peephole
fusions decided once per graph (conv+activation epilogue, BN+activation+dropout single pass).  Weights that a compiled
model trains live in ONE flat fp32 buffer (plus one flat gradient buffer), so the optimizer is a single fused kernel
and data-parallel training needs a single all-reduce per step.
"""
import re

import numpy as np
import torch

from . import ops

_DEVICE = None


def device():
    """The HIP device of this process: cuda:LOCAL_RANK (one process per GPU)."""
    global _DEVICE
    if _DEVICE is None:
        import os
        if not torch.cuda.is_available():
            from ._lib import GennetHipError
            raise GennetHipError('gennet_amd needs an AMD GPU (torch.cuda.is_available() is False); there is no CPU execution path')
        idx = int(os.environ.get('LOCAL_RANK', '0')) % max(torch.cuda.device_count(), 1)
        torch.cuda.set_device(idx)
        _DEVICE = torch.device('cuda', idx)
        # conv arithmetic (ops.set_conv_math): transform-domain fp32 for the unit-stride 5-tap layers by default; GENNET_CONV_MATH=fp32 keeps every
        # launch on the direct kernels, =bf16x3 is the opt-in operand-split experiment
        ops.set_conv_math(device=_DEVICE)
    return _DEVICE


def to_device(a, dtype=torch.float32):
    if isinstance(a, torch.Tensor):
        t = a.to(device=device(), dtype=dtype)
    else:
        t = torch.as_tensor(np.ascontiguousarray(np.asarray(a)), dtype=dtype).to(device())
    return t.contiguous()


_INIT_RNG = np.random.RandomState(12345)


def set_init_seed(seed):
    """Seed of the numpy RNG that draws initial weights (glorot_uniform)."""
    global _INIT_RNG
    _INIT_RNG = np.random.RandomState(seed)


def glorot_uniform(shape):
    """keras VarianceScaling(scale=1, mode='fan_avg', distribution='uniform')."""
    if len(shape) == 2:
        fi, fo = shape
    else:
        rec = int(np.prod(shape[:-2]))
        fi, fo = rec * shape[-2], rec * shape[-1]
    lim = np.sqrt(6.0 / (fi + fo))
    return _INIT_RNG.uniform(-lim, lim, size=shape).astype(np.float32)


# --------------------------------------------------------------------------------------------------------------
# parameters and flat groups
# --------------------------------------------------------------------------------------------------------------
class Param(object):
    """A weight tensor.  The initial value stays on the host until the first device access, so graphs can be built,
    planned and inspected (summary, count_params, get_weights) on a machine without a GPU; all arithmetic needs one."""

    def __init__(self, name, value, trainable=True, regularizer=None):
        self.name = name
        self.regularizer = regularizer     # a regularizers.L1L2 or None: its penalty enters the loss of every model that holds the weight
        self.shape = tuple(value.shape)
        self._host = np.ascontiguousarray(value, np.float32).reshape(self.shape)      # ascontiguousarray makes a () value (1,)
        self._data = None
        self.grad = None
        self.trainable = trainable
        self.group = None
        self.offset = 0

    @property
    def data(self):
        if self._data is None:
            self._data = to_device(self._host)
            self._host = None
        return self._data

    @data.setter
    def data(self, t):
        self._data = t
        self._host = None

    def numpy(self):
        return self._host.copy() if self._data is None else self._data.detach().cpu().numpy().copy()

    def assign(self, w):
        w = np.ascontiguousarray(w, np.float32)
        if self.shape == () and w.size == 1:
            w = w.reshape(())
        assert tuple(w.shape) == self.shape, '%s: %s vs %s' % (self.name, w.shape, self.shape)
        if self._data is None:
            self._host = w
        else:
            self._data.copy_(to_device(w))

    @property
    def size(self):
        return int(np.prod(self.shape)) if self.shape else 1


class ParamGroup(object):
    """Contiguous storage for a set of parameters: data, grad; every parameter starts on a 256-byte boundary."""
    ALIGN = 64

    def __init__(self, params):
        off = 0
        for p in params:
            p.offset = off
            off += -(-p.size // self.ALIGN) * self.ALIGN
        self.numel = off
        self.data = torch.zeros(off, dtype=torch.float32, device=device())
        self.grad = torch.zeros(off, dtype=torch.float32, device=device())
        for p in params:
            self.data[p.offset:p.offset + p.size].copy_(p.data.reshape(-1))
            p.data = self.data[p.offset:p.offset + p.size].view(p.shape)
            p.grad = self.grad[p.offset:p.offset + p.size].view(p.shape)
            p.group = self
        self.params = list(params)


def group_params(params):
    fresh = [p for p in params if p.group is None]
    if fresh:
        ParamGroup(fresh)


def segments(params):
    """Maximal runs of adjacent parameters inside their groups: [(group, start, stop)]."""
    spans = sorted(((id(p.group), p.offset, p) for p in params), key=lambda t: (t[0], t[1]))
    segs = []
    for _, off, p in spans:
        end = off + -(-p.size // ParamGroup.ALIGN) * ParamGroup.ALIGN
        if segs and segs[-1][0] is p.group and segs[-1][2] == off:
            segs[-1][2] = end
        else:
            segs.append([p.group, off, end])
    return [tuple(s) for s in segs]


# --------------------------------------------------------------------------------------------------------------
# run context
# --------------------------------------------------------------------------------------------------------------
class PhiloxStream(object):
    """Counter allocator for the device RNG: every consumer takes a disjoint counter range of one (seed) stream."""

    def __init__(self, seed=0):
        self.seed = int(seed)
        self.offset = 0

    def take(self, n_values):
        off = self.offset
        self.offset += (int(n_values) + 3) // 4
        return self.seed, off

    def take_rows(self, row_len, blocks, global_rows):
        """Counter ranges for (a rank's part of) a GLOBAL tensor of global_rows rows of row_len values each, the batch axis leading (SURVEY 8e:
        "latent z and noise likewise" -- N ranks x B / N rows draw exactly what one process draws for B rows, same seed everywhere).
        blocks = [(global_row_start, n_rows), ...]: the global rows this caller holds, in its local row order.  Returns (seed, [counter offset
        of every block]); the stream advances by the counters of the WHOLE global tensor on every rank, whatever part a rank takes.
        One block (0, global_rows) is take(global_rows * row_len)."""
        row_len, global_rows = int(row_len), int(global_rows)
        base = self.offset
        self.offset += (global_rows * row_len + 3) // 4
        offs = []
        for g0, n in blocks:
            if (int(g0) * row_len) % 4:
                raise ValueError('PhiloxStream.take_rows: a block starting at global row %d of %d-value rows does not start on a Philox counter '
                                 '(4 values each)' % (g0, row_len))
            offs.append(base + int(g0) * row_len // 4)
        return self.seed, offs


_RNG = PhiloxStream(0)


# --------------------------------------------------------------------------------------------------------------
# hipGraph capture of a whole train step
# --------------------------------------------------------------------------------------------------------------
_CAPTURE = None


def capturing():
    """The StepGraph being captured, or None."""
    return _CAPTURE


class StepGraph(object):
    """One train step captured as a hipGraph on the launch stream and replayed (the loops of bbhMahoGANy.py at the script's own batch
    size 8 are launch-bound: ~250 launches of a few microseconds each per iteration).  The library never allocates or synchronises, torch's
    allocator serves the step's temporaries from the graph's private pool, so the captured launches are exactly the eager ones.  What changes
    from step to step cannot be a by-value kernel argument (it would be frozen): it lives in ONE small parameter block in device memory
    that the host refreshes (pinned copy, stream-ordered) before every replay --
      * the Philox stream position: every draw inside the graph adds the block's rng base (gn_set_rng_base) = stream position at replay
        - stream position at capture, so a replay draws exactly what the eager step would have drawn at that point of the stream;
      * Adam's lr_t, BatchNormalization's local_step, the CNN loop's noise sigma: slot(fmt, provider) -- the provider runs once per replay,
        advances the host-side state (iteration counters) and returns the value.
    Batch indices and other per-step inputs are static device tensors the caller overwrites before replay()."""
    SLOTS = 64

    def __init__(self):
        import struct
        self._struct = struct
        self.host = torch.zeros(self.SLOTS * 8, dtype=torch.uint8).pin_memory()
        self.hostbuf = self.host.numpy()
        self.dev = torch.zeros(self.SLOTS * 8, dtype=torch.uint8, device=device())
        self.providers = []
        self.graph = None
        self.rng_start = 0
        self.rng_taken = 0
        self.copied = torch.cuda.Event()
        self._copied_once = False
        self.outputs = None
        self.scratch = []                  # every ops.workspace() buffer handed out during capture and the conv-math buffer: the graph holds their addresses

    def slot(self, fmt, provider):
        """Reserve one 8-byte slot holding a scalar of struct format `fmt` ('f', 'i', 'Q'); provider() -> value is called before every replay."""
        i = len(self.providers)
        if i >= self.SLOTS:
            raise RuntimeError('StepGraph: more than %d step-varying scalars' % self.SLOTS)
        self.providers.append((i, fmt, provider))
        return ops.DevScalar(self.dev.data_ptr() + 8 * i)

    def capture(self, fn):
        """Record fn() (kernel launches on the capture stream; nothing executes now).  Host-side counters that fn advances per step are
        advanced by the providers at replay time instead; the Philox stream is rewound to where it stood."""
        global _CAPTURE
        if _CAPTURE is not None:
            raise RuntimeError('StepGraph.capture: already capturing')
        rng = device_rng()
        self.rng_start = rng.offset

        def keep(buf):
            if not any(b is buf for b in self.scratch):
                self.scratch.append(buf)

        def rng_base():
            base = device_rng().offset - self.rng_start
            device_rng().offset += self.rng_taken
            return base
        base = self.slot('Q', rng_base)
        if ops.conv_math_workspace() is not None:
            keep(ops.conv_math_workspace())
        self.graph = torch.cuda.CUDAGraph()
        _CAPTURE = self
        ops.set_rng_base(base.ptr)
        ops._ws_on_use = keep
        prof = ops.prof_enabled()          # the launch-stream HIP events of the profiling hooks must not be recorded into the graph
        if prof:
            ops.prof_enable(False)
        try:
            with torch.cuda.graph(self.graph):
                self.outputs = fn()
        finally:
            ops.set_rng_base(None)
            ops._ws_on_use = None
            _CAPTURE = None
            if prof:
                ops.prof_enable(True)
            self.rng_taken = rng.offset - self.rng_start
            rng.offset = self.rng_start    # also when fn raised: the draws of a failed capture never executed
        return self.outputs

    def wait_inputs_consumed(self):
        """Block until the previous replay's host -> device copies are done, so pinned staging buffers (this block, the caller's batch
        indices) may be overwritten.  The host stays at most one step ahead of the device."""
        if self._copied_once:
            self.copied.synchronize()

    def replay(self):
        """Refresh the parameter block, then launch the graph on the current stream.  The caller has already waited
        (wait_inputs_consumed) before touching its own staging buffers and enqueued their copies on the current stream."""
        for i, fmt, provider in self.providers:
            self._struct.pack_into('<' + fmt, self.hostbuf, 8 * i, provider())
        self.dev.copy_(self.host, non_blocking=True)
        self.copied.record()
        self._copied_once = True
        self.graph.replay()
        return self.outputs


def set_device_seed(seed):
    global _RNG
    _RNG = PhiloxStream(seed)


def device_rng():
    return _RNG


class RunContext(object):
    def __init__(self, training, dp=None, dropout_masks=None, train_params=None, site=None, row_map=None):
        self.training = training
        # which rows of the GLOBAL batch this step's local rows are: [(global_row_start, n_rows), ...] in local order, and the global row count.
        # Every per-row random draw inside the step (dropout masks) takes the counters of its global rows (PhiloxStream.take_rows), so N ranks
        # draw what one process would.  None: the rows are the whole batch.
        self.row_map = row_map
        self.site = site                   # name of the model whose train_on_batch runs (BatchNormalization keeps per-site state)
        self.capture = None                # testing hook: dict that receives {layer name: output tensor} of every executed node
        self.dp = dp
        self.dropout_masks = dropout_masks or {}
        self.train_ids = None if train_params is None else set(id(p) for p in train_params)
        self.tape = {}
        self.epi = {}                      # node index -> (y, act, act_param, mask, rate): epilogue a consumer's dgrad can differentiate
        self.pre_applied = set()           # producers whose activation gradient has already been applied to their dy
        self.skip = set()                  # inference phase: BatchNormalization nodes already folded into the producing conv
        self.bn_sums = {}                  # training phase: BN node index -> fp64 (sum x, sum x^2) produced by the conv epilogue
        self.reg = None                    # train / test step of a regularized model: node index -> its slice of the step's fp64 penalty partials
        self.reg_y = {}                    # training phase: node index -> the output an activity regularizer's gradient term is formed from

    def wants_grad(self, layer):
        if self.train_ids is None:
            return False
        return any(id(p) in self.train_ids for p in layer.trainable_params())


# --------------------------------------------------------------------------------------------------------------
# layers: base class + symbolic tensors
# --------------------------------------------------------------------------------------------------------------
class SymTensor(object):
    def __init__(self, shape, layer=None, inbound=(), name=None):
        self.shape = tuple(shape)          # without the batch axis
        self.layer = layer
        self.inbound = tuple(inbound)
        self.name = name                   # only graph inputs carry a name (keras InputLayer)


_NAME_COUNTS = {}


def to_snake_case(name):
    """keras.engine.base_layer._to_snake_case: Conv1D -> conv1d, BatchNormalization -> batch_normalization,
    LeakyReLU -> leaky_re_lu, UpSampling1D -> up_sampling1d (the names keras writes into .h5 files)."""
    intermediate = re.sub('(.)([A-Z][a-z0-9]+)', r'\1_\2', name)
    insecure = re.sub('([a-z])([A-Z])', r'\1_\2', intermediate).lower()
    return 'private' + insecure if insecure[0] == '_' else insecure


def _unique_name(base):
    _NAME_COUNTS[base] = _NAME_COUNTS.get(base, 0) + 1
    return '%s_%d' % (base, _NAME_COUNTS[base])


def Input(shape=None, name=None, batch_shape=None, dtype=None):
    if shape is None and batch_shape is not None:
        shape = tuple(batch_shape[1:])
    return SymTensor(shape, name=name or _unique_name('input'))


class Layer(object):
    """Base layer.  Subclasses implement build(input_shape), compute_output_shape(input_shape),
    forward(ctx, node, x) and backward(ctx, node, dy, need_dx, need_dw)."""

    def __init__(self, input_shape=None, name=None, trainable=True, **kwargs):
        if name is None:
            name = _unique_name(to_snake_case(self.__class__.__name__))
        self.name = name
        self.trainable = trainable
        self.built = False
        self.input_shape_arg = tuple(input_shape) if input_shape is not None else None
        self.params = []
        self.buffers = []

    # -- keras-style weight bookkeeping
    def add_weight(self, name, value, trainable=True, regularizer=None):
        p = Param('%s/%s' % (self.name, name), value, trainable, regularizer)
        (self.params if trainable else self.buffers).append(p)
        return p

    def trainable_params(self):
        return self.params

    @property
    def trainable_weights(self):
        return list(self.params) if self.trainable else []

    @property
    def non_trainable_weights(self):
        return list(self.buffers) + ([] if self.trainable else list(self.params))

    @property
    def weights(self):
        return list(self.params) + list(self.buffers)

    def get_weights(self):
        return [p.numpy() for p in self.weights]

    def set_weights(self, ws):
        assert len(ws) == len(self.weights), '%s expects %d arrays' % (self.name, len(self.weights))
        for p, w in zip(self.weights, ws):
            p.assign(w)

    def count_params(self):
        return sum(p.size for p in self.weights)

    # -- shape protocol
    def build(self, input_shape):
        self.built = True

    def compute_output_shape(self, input_shape):
        return input_shape

    def get_config(self):
        """keras' layer config, as model.save writes it (keras_io.layer_config)"""
        from . import keras_io
        return keras_io.layer_config(self)

    # A subclass that defines keras' `call(self, x)` (and not this engine's forward/backward) is a USER-DEFINED layer in keras'
    # conventions (bbhMahoGANy.py:164-188): its build / compute_output_shape see shapes WITH the batch axis, and its call is traced
    # once on a symbolic operand and lowered to a HIP kernel (gennet_amd/keras/backend.py).
    def _is_user_layer(self):
        return callable(getattr(type(self), 'call', None)) and type(self).forward is Layer.forward

    def _ensure_built(self, input_shape):
        if not self.built:
            self.build((None,) + tuple(input_shape) if self._is_user_layer() else tuple(input_shape))
            self.built = True

    def _shape_after(self, input_shape):
        """Output shape without the batch axis for an input shape without the batch axis."""
        if self._is_user_layer():
            out = tuple(self.compute_output_shape((None,) + tuple(input_shape)))[1:]
            self._lower(tuple(input_shape), out)
            return out
        return tuple(self.compute_output_shape(tuple(input_shape)))

    def _lower(self, input_shape, out_shape):
        if getattr(self, '_lowered', None) is None or self._lowered_for != input_shape:
            from .keras import backend as K
            self._lowered = K.lower_layer_call(self, input_shape)
            self._lowered_for = input_shape
            if tuple(out_shape) != (input_shape[0], 2, 1):
                raise ValueError('%s.compute_output_shape gives %r; its call produces %r' % (type(self).__name__, (None,) + tuple(out_shape), (None, input_shape[0], 2, 1)))
        return self._lowered

    # -- functional API
    def __call__(self, x):
        if isinstance(x, (list, tuple)):
            # keras layers/merge.py: only a merge layer takes a list; its build / compute_output_shape receive the list of shapes
            if not self.is_merge:
                raise ValueError('%s (%s) takes a single tensor, not a list of %d: only the merge layers (Add, Subtract, Multiply, Average, Maximum, '
                                 'Minimum, Concatenate) join tensors' % (self.name, type(self).__name__, len(x)))
            if len(x) < 2:
                raise ValueError('A merge layer should be called on a list of at least 2 inputs (%s got %d)' % (self.name, len(x)))
            shapes = [tuple(t.shape) for t in x]
            if not self.built:
                self.build(shapes)
                self.built = True
            return SymTensor(tuple(self.compute_output_shape(shapes)), self, tuple(x))
        if self.is_merge:
            raise ValueError('A merge layer should be called on a list of at least 2 inputs (%s got a single tensor)' % self.name)
        self._ensure_built(x.shape)
        return SymTensor(self._shape_after(x.shape), self, (x,))

    # -- execution
    is_merge = False         # joins several inbound tensors (layers._Merge, layers.Concatenate): forward takes the list, backward returns one
    fusable_act = False      # can take an activation epilogue
    fusable_drop = False     # can take a dropout epilogue
    act_spec = None          # (kind, param) if this layer IS an activation
    activity_regularizer = None   # a regularizers.L1L2 on this layer's own output (Dense, the conv layers, ActivityRegularization)
    drop_rate = None         # rate if this layer IS a dropout

    def writes_dy(self, node):
        """Whether backward() overwrites the gradient it is handed (the in-place activation backward of the conv and dense layers).
        Model._backward copies a gradient that another edge still holds before it hands it to such a layer."""
        return False

    def forward(self, ctx, node, x):
        if not self._is_user_layer():
            raise NotImplementedError
        low = self._lower(tuple(x.shape[1:]), tuple(node.out_shape))
        b0, b1 = low.betas()
        return ops.affine_stack_fwd(x.contiguous(), low.a0, b0, low.a1, b1)

    def backward(self, ctx, node, dy, need_dx, need_dw):
        if not self._is_user_layer():
            raise NotImplementedError
        return ops.affine_stack_bwd(dy.contiguous(), self._lowered.a0, self._lowered.a1)


class Node(object):
    __slots__ = ('layer', 'inbound', 'fused_act', 'fused_drop', 'absorbed', 'index', 'out_shape', 'owners', 'fuse_prev', 'infer_bn', 'fold_up', 'lazy_bn')

    def __init__(self, layer, inbound, out_shape, owners=()):
        self.layer = layer
        self.owners = tuple(owners)        # nested models this node was spliced in from (their .trainable also gates it)
        self.inbound = list(inbound)       # indices: >= 0 node, < 0 graph input (-1 - k)
        self.fused_act = None              # (kind, param) applied in this node's epilogue
        self.fused_drop = None             # (rate, dropout layer) applied in this node's epilogue
        self.absorbed = False              # this node's work happens inside its producer
        self.index = -1
        self.out_shape = out_shape
        self.fuse_prev = -1                # producer node whose [activation -> dropout] backward this node's dgrad absorbs
        self.fold_up = None                # the absorbed UpSampling1D node in front whose work is folded into this conv's weights
        self.infer_bn = None               # the BatchNormalization consumer this conv absorbs in the inference phase
        self.lazy_bn = -1                  # BatchNormalization producer that forms this 1-filter conv's data gradient in its own backward


# --------------------------------------------------------------------------------------------------------------
# optimizer
# --------------------------------------------------------------------------------------------------------------
def _f32(x):
    return float(np.float32(x))


class Optimizer(object):
    """Keras 2.2.4 optimizer (keras/optimizers.py), the work every rule shares: the flat segments of the trained weights and the rule's state
    per segment, the step's one varying scalar (eager: by value; inside a captured step graph: a StepGraph slot), Keras' gradient clipping
    over all trained weights of the compiled model (clipnorm, then clipvalue), get_config, and the rule's optimizer_weights layout in .h5 files.
    A subclass names its fused-pass rule (ops.OPT_RULES), its state arrays, its hyper-parameters and its per-step scalar.

    Shared rules: iterations counts steps; decay > 0 gives lr_eff = lr / (1 + decay * iterations) with iterations before this step's
    increment, t = iterations + 1; epsilon=None is 1e-7; what Keras holds as K.variable (lr, decay, momentum, RMSprop's rho, the betas) is
    float32-rounded, the rest stays a python value.  The host computes the step scalar in fp64 and it is rounded once to fp32."""
    RULE = None                            # ops.OPT_RULES key of the fused update
    SLOTS = ()                             # per-weight state arrays, in the order of Keras' optimizer.weights
    SAVES_ITERATIONS = True                # Keras 2.2.4 puts `iterations` first in optimizer.weights (SGD, Adamax, Adam; not RMSprop, Adagrad, Adadelta)
    CONFIG = ()                            # get_config keys after 'lr', Keras' order

    def __init__(self, lr, decay=0.0, clipnorm=None, clipvalue=None, **kwargs):
        if kwargs:                         # keras.optimizers.Optimizer: only clipnorm / clipvalue
            raise TypeError('Unexpected keyword argument passed to optimizer: %s' % sorted(kwargs)[0])
        self.lr, self.decay = _f32(lr), _f32(decay)
        self.clipnorm, self.clipvalue = clipnorm, clipvalue
        self.iterations = 0
        self.state = None                  # [(group, start, stop, [state tensor per slot])]

    # -- what a rule defines
    def _n_slots(self):
        return len(self.SLOTS)

    def _hyper(self):
        """(h0, h1, eps, nesterov) of gn_optim_step."""
        return 0.0, 0.0, 0.0, False

    def _lr_eff(self, it):
        return self.lr / (1.0 + self.decay * it) if self.decay > 0 else self.lr

    def _scalar(self, it):
        """The step's one varying value for the step that starts at iterations = it: lr_eff (lr_t for Adam, Adamax)."""
        return self._lr_eff(it)

    def _layout(self):
        """Keras' optimizer.weights after `iterations`: one block of per-weight arrays per entry, the state slot it holds (None: a (1,) zero stub)."""
        return list(range(self._n_slots()))

    # -- shared work
    def get_config(self):
        cfg = {'lr': self.lr}
        cfg.update((k, getattr(self, k)) for k in self.CONFIG)
        if self.clipnorm is not None:
            cfg['clipnorm'] = self.clipnorm
        if self.clipvalue is not None:
            cfg['clipvalue'] = self.clipvalue
        return cfg

    def bind(self, params):
        self.state = []
        for grp, a, b in segments(params):
            self.state.append((grp, a, b, [torch.zeros(b - a, dtype=torch.float32, device=device()) for _ in range(self._n_slots())]))
        self._partials = self._factor = None
        if self.clipnorm is not None and self.clipnorm > 0:
            # owned here, not taken from ops.workspace: a captured step graph keeps these addresses for its whole life
            self._part_slices, off = [], 0
            for _, a, b, _ in self.state:
                k = ops.optim_sumsq_slots(b - a)
                self._part_slices.append((off, k)); off += k
            self._partials = torch.zeros(off, dtype=torch.float64, device=device())
            self._factor = torch.ones(1, dtype=torch.float32, device=device())

    def _next_scalar(self):
        it = self.iterations
        self.iterations = it + 1
        return self._scalar(it)

    def _clip_scale(self):
        if self._partials is None:
            return None
        for (grp, a, b, _), (o, k) in zip(self.state, self._part_slices):
            ops.optim_sumsq(grp.grad[a:b], self._partials[o:o + k])
        ops.optim_clip_factor(self._partials, self.clipnorm, self._factor)
        return self._factor

    def _update(self, p, g, st, lr, clip):
        h0, h1, eps, nesterov = self._hyper()
        ops.optim_step(self.RULE, p, g, st, lr, h0, h1, eps, nesterov, clip, self.clipvalue if self.clipvalue and self.clipvalue > 0 else 0.0)

    def step(self):
        cap = capturing()
        # inside a captured step graph the iteration count advances once per REPLAY and the scalar reaches the kernel through device memory
        lr = self._next_scalar() if cap is None else cap.slot('f', self._next_scalar)
        clip = self._clip_scale()
        for grp, a, b, st in self.state:
            self._update(grp.data[a:b], grp.grad[a:b], st, lr, clip)

    def _views(self, p):
        for grp, a, b, st in self.state:
            if grp is p.group and a <= p.offset and p.offset + p.size <= b:
                return [t[p.offset - a:p.offset - a + p.size] for t in st]
        raise KeyError('%s is not trained by this optimizer' % p.name)

    def get_keras_weights(self, params):
        """Keras' optimizer.get_weights() for trained weights `params` in model.trainable_weights order (the .h5 optimizer_weights)."""
        out = [np.asarray(self.iterations, np.int64)] if self.SAVES_ITERATIONS else []
        views = [self._views(p) for p in params]
        for k in self._layout():
            out += [np.zeros((1,), np.float32) if k is None else v[k].cpu().numpy().reshape(p.shape) for p, v in zip(params, views)]
        return out

    def split_keras_weights(self, vals, n):
        """(iterations or None, [[n arrays] per block of _layout()]) from optimizer_weights in weight_names order (never by name: the scope
        prefix depends on the Keras session).  Trailing stub blocks may be absent (Keras before amsgrad wrote no vhat)."""
        vals = list(vals)
        it = None
        if self.SAVES_ITERATIONS:
            if not vals or np.asarray(vals[0]).size != 1:
                raise ValueError('%s: optimizer_weights do not start with the iteration count' % type(self).__name__)
            it = int(np.asarray(vals[0]).reshape(-1)[0])
            vals = vals[1:]
        lay = self._layout()
        need = len(lay)
        while need and lay[need - 1] is None:
            need -= 1
        if len(vals) not in (need * n, len(lay) * n):
            raise ValueError('%s: %d optimizer arrays for %d trained weights (layout %s)' % (type(self).__name__, len(vals), n, lay))
        return it, [vals[j * n:(j + 1) * n] for j in range(len(vals) // n if n else 0)]

    def set_keras_weights(self, params, vals):
        it, blocks = self.split_keras_weights(vals, len(params))
        views = [self._views(p) for p in params]
        for k, arrs in zip(self._layout(), blocks):
            if k is None:
                continue
            for p, v, a in zip(params, views, arrs):
                a = np.asarray(a, np.float32)
                if a.size != p.size:
                    raise ValueError('%s: optimizer array of shape %s for %s %s' % (type(self).__name__, a.shape, p.name, p.shape))
                v[k].copy_(to_device(a.reshape(-1)))
        if it is not None:
            self.iterations = it

    def get_state(self):
        return {'iterations': self.iterations, 'slots': [[t.cpu().numpy() for t in st] for _, _, _, st in (self.state or [])],
                'config': self.get_config()}

    def set_state(self, st):
        self.iterations = st['iterations']
        for (_, _, _, ts), arrs in zip(self.state, st['slots']):
            for t, a in zip(ts, arrs):
                t.copy_(to_device(a))


class SGD(Optimizer):
    """keras.optimizers.SGD: v = momentum m - lr_eff g; m = v; p += momentum v - lr_eff g (nesterov) | v.  optimizer.weights: [iterations] + m
    (the reference's g_model.hdf5 was compiled with SGD; 2_model_version/no_weight_code/noise_gan.py:75 trains with SGD(lr=lr))."""
    RULE, SLOTS, CONFIG = 'sgd', ('m',), ('momentum', 'decay', 'nesterov')

    def __init__(self, lr=0.01, momentum=0.0, decay=0.0, nesterov=False, **kwargs):
        Optimizer.__init__(self, lr, decay, **kwargs)
        self.momentum, self.nesterov = _f32(momentum), bool(nesterov)

    def _hyper(self):
        return self.momentum, 0.0, 0.0, self.nesterov


class RMSprop(Optimizer):
    """keras.optimizers.RMSprop: a = rho a + (1 - rho) g^2; p -= lr_eff g / (sqrt(a) + eps).  optimizer.weights: a (no iterations)."""
    RULE, SLOTS, SAVES_ITERATIONS, CONFIG = 'rmsprop', ('a',), False, ('rho', 'decay', 'epsilon')

    def __init__(self, lr=0.001, rho=0.9, epsilon=None, decay=0.0, **kwargs):
        Optimizer.__init__(self, lr, decay, **kwargs)
        self.rho = _f32(rho)
        self.epsilon = 1e-7 if epsilon is None else float(epsilon)

    def _hyper(self):
        return self.rho, 0.0, self.epsilon, False


class Adagrad(Optimizer):
    """keras.optimizers.Adagrad: a += g^2; p -= lr_eff g / (sqrt(a) + eps).  optimizer.weights: a (no iterations)."""
    RULE, SLOTS, SAVES_ITERATIONS, CONFIG = 'adagrad', ('a',), False, ('decay', 'epsilon')

    def __init__(self, lr=0.01, epsilon=None, decay=0.0, **kwargs):
        Optimizer.__init__(self, lr, decay, **kwargs)
        self.epsilon = 1e-7 if epsilon is None else float(epsilon)

    def _hyper(self):
        return 0.0, 0.0, self.epsilon, False


class Adadelta(Optimizer):
    """keras.optimizers.Adadelta: a = rho a + (1 - rho) g^2; u = g sqrt(d + eps) / sqrt(a + eps); p -= lr_eff u; d = rho d + (1 - rho) u^2.
    rho is a python float in Keras 2.2.4 (not a K.variable).  optimizer.weights: a + d (no iterations)."""
    RULE, SLOTS, SAVES_ITERATIONS, CONFIG = 'adadelta', ('a', 'd'), False, ('rho', 'decay', 'epsilon')

    def __init__(self, lr=1.0, rho=0.95, epsilon=None, decay=0.0, **kwargs):
        Optimizer.__init__(self, lr, decay, **kwargs)
        self.rho = float(rho)
        self.epsilon = 1e-7 if epsilon is None else float(epsilon)

    def _hyper(self):
        return self.rho, 0.0, self.epsilon, False


class Adamax(Optimizer):
    """keras.optimizers.Adamax: lr_t = lr_eff / (1 - b1^t); m = b1 m + (1 - b1) g; u = max(b2 u, |g|); p -= lr_t m / (u + eps).
    optimizer.weights: [iterations] + m + u."""
    RULE, SLOTS, CONFIG = 'adamax', ('m', 'u'), ('beta_1', 'beta_2', 'decay', 'epsilon')

    def __init__(self, lr=0.002, beta_1=0.9, beta_2=0.999, epsilon=None, decay=0.0, **kwargs):
        Optimizer.__init__(self, lr, decay, **kwargs)
        self.beta_1, self.beta_2 = _f32(beta_1), _f32(beta_2)
        self.epsilon = 1e-7 if epsilon is None else float(epsilon)

    def _hyper(self):
        return self.beta_1, self.beta_2, self.epsilon, False

    def _scalar(self, it):
        return self._lr_eff(it) / (1.0 - self.beta_1 ** (it + 1))


class Adam(Optimizer):
    """keras.optimizers.Adam: lr_t = lr_eff*sqrt(1-b2^t)/(1-b1^t); p -= lr_t*m/(sqrt(v)+eps); amsgrad: vhat = max(vhat, v)
    replaces v under the root.  optimizer.weights: [iterations] + m + v + vhat ((1,) zero stubs without amsgrad).  Without decay, amsgrad and
    clipping the update is the library's original Adam pass (gn_adam_step), bit for bit."""
    RULE, SLOTS, CONFIG = 'adam', ('m', 'v', 'vhat'), ('beta_1', 'beta_2', 'decay', 'epsilon', 'amsgrad')

    def __init__(self, lr=0.001, beta_1=0.9, beta_2=0.999, epsilon=None, decay=0.0, amsgrad=False, **kwargs):
        # float32 variables in Keras (K.variable): the values that take part -- and that Keras writes into training_config -- are the
        # float32-rounded ones (the reference's own d_model.hdf5 records beta_2 = 0.9990000128746033); epsilon stays a python float
        Optimizer.__init__(self, lr, decay, **kwargs)
        self.beta_1, self.beta_2 = _f32(beta_1), _f32(beta_2)
        self.epsilon = 1e-7 if epsilon is None else float(epsilon)
        self.amsgrad = bool(amsgrad)

    def _n_slots(self):
        return 3 if self.amsgrad else 2

    def _layout(self):
        return [0, 1, 2 if self.amsgrad else None]

    def _hyper(self):
        return self.beta_1, self.beta_2, self.epsilon, False

    def _scalar(self, it):
        t = it + 1
        return self._lr_eff(it) * np.sqrt(1.0 - self.beta_2 ** t) / (1.0 - self.beta_1 ** t)

    def _default_pass(self):
        return not self.amsgrad and not self.decay > 0 and not (self.clipnorm and self.clipnorm > 0) and not (self.clipvalue and self.clipvalue > 0)

    def _update(self, p, g, st, lr, clip):
        if self._default_pass():
            ops.adam_step(p, g, st[0], st[1], lr, self.beta_1, self.beta_2, self.epsilon)
        else:
            ops.optim_step('amsgrad' if self.amsgrad else 'adam', p, g, st, lr, self.beta_1, self.beta_2, self.epsilon, False, clip,
                           self.clipvalue if self.clipvalue and self.clipvalue > 0 else 0.0)


OPTIMIZERS = {'SGD': SGD, 'RMSprop': RMSprop, 'Adagrad': Adagrad, 'Adadelta': Adadelta, 'Adamax': Adamax, 'Adam': Adam}


def optimizer_from_config(oc):
    """keras.optimizers.deserialize of a training_config's optimizer_config {'class_name', 'config'}."""
    cls = OPTIMIZERS.get(oc['class_name'])
    if cls is None:
        raise NotImplementedError('optimizer %s (supported: %s)' % (oc['class_name'], ', '.join(sorted(OPTIMIZERS))))
    return cls(**oc['config'])


def _get_optimizer(opt):
    if isinstance(opt, str):
        cls = {k.lower(): v for k, v in OPTIMIZERS.items()}.get(opt.lower())
        if cls is None:
            raise NotImplementedError('optimizer %r' % opt)
        return cls()
    return opt


LOSSES = tuple(k for k in ops.LOSS_KINDS if k != 'categorical_accuracy')
OLD_KERNEL_LOSSES = ('binary_crossentropy', 'mean_squared_error')      # the one-block kernel of ops.loss, kept below ops.LOSS_PASS_MIN_ELEMENTS
ACC_METRICS = ('accuracy', 'acc', 'binary_accuracy')                   # the hit count round(p) == y that every loss call returns
PASS_METRICS = ('categorical_accuracy', 'mean_absolute_error', 'mean_squared_error', 'mean_absolute_percentage_error',
                'mean_squared_logarithmic_error', 'cosine_proximity')


def _named_fn(name):
    def fn(y_true, y_pred):
        raise NotImplementedError('%s names a HIP loss pass for compile(loss= / metrics=); there is no tensor runtime to call it on' % name)
    fn.__name__ = fn.__qualname__ = name
    fn.__doc__ = 'keras.losses.%s: pass it (or its name) to compile()' % name
    return fn


# keras.losses / keras.metrics of the facade: one callable per kind, its aliases the same object (as in Keras); compile() knows them by identity
LOSS_FUNCTIONS = dict((k, _named_fn(k)) for k in ops.LOSS_KINDS)
LOSS_FUNCTIONS.update((a, LOSS_FUNCTIONS[k]) for a, k in ops.LOSS_ALIASES.items())
_FN_NAMES = dict((id(fn), k) for k, fn in LOSS_FUNCTIONS.items() if k in ops.LOSS_KINDS)


def _loss_name(l):
    """The kind of ops.LOSS_KINDS that a name, an alias or a facade callable stands for; None for anything else."""
    if callable(l):
        return _FN_NAMES.get(id(l))
    k = ops.LOSS_ALIASES.get(l, l) if isinstance(l, str) else None
    return k if k in ops.LOSS_KINDS else None


# --------------------------------------------------------------------------------------------------------------
# models
# --------------------------------------------------------------------------------------------------------------
class Model(Layer):
    """Functional model: Model(inputs=Input(...), outputs=[t1, t2], name=...).  Also the base of Sequential."""

    def __init__(self, inputs=None, outputs=None, name=None, **kwargs):
        Layer.__init__(self, name=name)
        self.nodes = []
        self.input_shapes = []
        self.output_ids = []
        self._planned = False
        self.optimizer = None
        self.loss = None
        self.metrics = []
        self.loss_weights = None
        self._acc, self._metric_kinds = False, []
        self.weighted_metrics = []
        self._wacc, self._wmetric_kinds = False, []
        self._train_params = None
        self.data_parallel = None
        if inputs is not None:
            self._from_symbolic(inputs, outputs)

    # -- graph construction
    def _from_symbolic(self, inputs, outputs):
        ins = list(inputs) if isinstance(inputs, (list, tuple)) else [inputs]
        outs = list(outputs) if isinstance(outputs, (list, tuple)) else [outputs]
        self.input_shapes = [t.shape for t in ins]
        self._sym_inputs, self._sym_outputs = ins, outs        # kept for model_config / keras layer order (keras_io.py)
        index = {}
        for k, t in enumerate(ins):
            index[id(t)] = -1 - k

        def visit(t):
            if id(t) in index:
                return index[id(t)]
            if t.layer is None:
                raise ValueError('graph reaches an Input that is not listed in inputs=')
            inb = [visit(s) for s in t.inbound]
            idx = self._append(t.layer, inb, t.shape)
            index[id(t)] = idx
            return idx

        self.output_ids = [visit(t) for t in outs]
        self.built = True

    def _append(self, layer, inbound, out_shape, owners=()):
        """Append a leaf layer, or splice in a nested model's nodes (weights are shared with the nested model)."""
        if isinstance(layer, Model):
            assert len(layer.input_shapes) == 1 and len(layer.output_ids) == 1 and len(inbound) == 1, 'nested models must be 1-in / 1-out'
            remap = {}
            for n in layer.nodes:
                inb = [inbound[0] if i < 0 else remap[i] for i in n.inbound]
                remap[n.index] = self._append(n.layer, inb, n.out_shape, tuple(owners) + (layer,) + n.owners)
            return remap[layer.output_ids[0]]
        node = Node(layer, inbound, out_shape, owners)
        node.index = len(self.nodes)
        self.nodes.append(node)
        self._planned = False
        return node.index

    @property
    def layers(self):
        seen, out = set(), []
        for n in self.nodes:
            if id(n.layer) not in seen:
                seen.add(id(n.layer))
                out.append(n.layer)
        return out

    @property
    def output_shape(self):
        shapes = [(None,) + tuple(self.nodes[i].out_shape) for i in self.output_ids]
        return shapes[0] if len(shapes) == 1 else shapes

    def compute_output_shape(self, input_shape):
        return self.nodes[self.output_ids[0]].out_shape

    # -- trainability (keras: model.trainable = False freezes; what counts is the value at compile time)
    def trainable_params(self):
        out = []
        for l in self.layers:
            out.extend(l.trainable_params())
        return out

    @property
    def trainable_weights(self):
        if not self.trainable:
            return []
        out = []
        for l in self.layers:
            out.extend(l.trainable_weights)
        return out

    @property
    def non_trainable_weights(self):
        out = []
        for l in self.layers:
            out.extend(l.non_trainable_weights if self.trainable else l.weights)
        return out

    @property
    def weights(self):
        out = []
        for l in self.layers:
            out.extend(l.weights)
        return out

    def get_weights(self):
        return [w for l in self.layers for w in l.get_weights()]

    def set_weights(self, ws):
        ws = list(ws)
        for l in self.layers:
            n = len(l.weights)
            l.set_weights(ws[:n])
            ws = ws[n:]
        assert not ws, 'too many weight arrays'

    # -- planning: consumers, peephole fusions
    def _plan(self):
        for n in self.nodes:
            n.fused_act, n.fused_drop, n.absorbed, n.fuse_prev, n.fold_up, n.infer_bn, n.lazy_bn = None, None, False, -1, None, None, -1
        consumers = {n.index: [] for n in self.nodes}
        for n in self.nodes:
            for i in n.inbound:
                if i >= 0:
                    consumers[i].append(n.index)
        outs = set(self.output_ids)

        def sole_consumer(i):
            if i in outs or len(consumers[i]) != 1:
                return None
            return self.nodes[consumers[i][0]]

        # a node with an activity regularizer: the penalty is taken of the layer's OWN output, so that tensor is materialised as the
        # layer defines it -- no epilogue of a following layer is fused onto it, forward or backward, in either phase
        def areg(node):
            return node.layer.activity_regularizer is not None

        for n in self.nodes:
            if n.absorbed or areg(n):
                continue
            tail = n
            # a layer with a non-linear activation of its own (Dense, Conv1D, Conv2D, Conv2DTranspose(activation=...)) has its epilogue taken: an
            # activation layer behind it runs as its own pass, act2(act1(z)) as keras computes it, and a Dropout behind that one follows it
            own_act = getattr(n.layer, 'activation', None)
            if n.layer.fusable_act and (own_act is None or own_act[0] == 'linear'):
                c = sole_consumer(tail.index)
                if c is not None and c.layer.act_spec is not None:
                    n.fused_act = c.layer.act_spec
                    c.absorbed = True
                    tail = c
            if n.layer.fusable_drop:
                c = sole_consumer(tail.index)
                if c is not None and c.layer.drop_rate is not None:
                    n.fused_drop = (c.layer.drop_rate, c.layer)
                    c.absorbed = True
        # UpSampling1D(2) whose only consumer is a 5-tap 'same' Conv1D: the pair runs as a 3-tap conv on the un-upsampled tensor with
        # folded weights (layers._ConvRun); the upsample node passes its input through and nothing is materialised
        for n in self.nodes:
            if n.absorbed or not getattr(n.layer, 'is_upsample2', False) or len(n.inbound) != 1 or n.inbound[0] < 0:
                continue
            c = sole_consumer(n.index)
            if c is not None and not c.absorbed and not areg(c) and hasattr(c.layer, 'can_fold_upsample') and c.layer.can_fold_upsample():
                c.fold_up = n
                n.absorbed = True
        # inference-phase fusion: a BatchNormalization that is the sole consumer of a linear conv folds into that conv's weights
        # (predict only: the training phase normalises with batch statistics)
        for n in self.nodes:
            if n.absorbed or areg(n) or not getattr(n.layer, 'can_fold_bn', False) or n.fused_act is not None or n.fused_drop is not None:
                continue
            c = sole_consumer(n.index)
            if c is not None and getattr(c.layer, 'is_batchnorm', False):
                n.infer_bn = c
        # backward fusion: node n's data gradient can carry the producer p's activation/dropout derivative in its epilogue when p's
        # output reaches n through shape-only nodes (absorbed activations, Flatten, Reshape) and nothing else consumes it
        for n in self.nodes:
            if n.absorbed or len(n.inbound) != 1 or not getattr(n.layer, 'can_absorb_prev_act_bwd', False):
                continue
            cur, ok = n.inbound[0], True
            while cur >= 0 and (self.nodes[cur].absorbed or getattr(self.nodes[cur].layer, 'shape_only', False)):
                if len(consumers[cur]) != 1 or cur in outs:
                    ok = False
                    break
                cur = self.nodes[cur].inbound[0]
            if (ok and cur >= 0 and len(consumers[cur]) == 1 and cur not in outs and getattr(self.nodes[cur].layer, 'offers_act_bwd', False)
                    and not areg(self.nodes[cur])):
                n.fuse_prev = cur
        # a 1-filter stride-1 Conv1D whose input comes from a BatchNormalization through absorbed nodes only (the generator's output
        # conv): its data gradient is not materialised, the BatchNormalization's backward passes form it on the fly (ops.ConvGrad1)
        for n in self.nodes:
            if n.absorbed or len(n.inbound) != 1 or n.fold_up is not None or not hasattr(n.layer, 'can_defer_dgrad'):
                continue
            cur = n.inbound[0]
            while cur >= 0 and self.nodes[cur].absorbed and len(consumers[cur]) == 1 and cur not in outs:
                cur = self.nodes[cur].inbound[0]
            if cur < 0 or len(consumers[cur]) != 1 or cur in outs or not getattr(self.nodes[cur].layer, 'is_batchnorm', False) or self.nodes[cur].absorbed:
                continue
            shp = self.nodes[cur].out_shape
            if len(shp) == 2 and n.layer.can_defer_dgrad(shp[1]):
                n.lazy_bn = cur
        self._planned = True

    # -- execution
    def _forward(self, inputs, ctx):
        if not self._planned:
            self._plan()
        vals = {}
        for k, x in enumerate(inputs):
            vals[-1 - k] = x
        for n in self.nodes:
            xs = [vals[i] for i in n.inbound]
            if n.absorbed:
                vals[n.index] = xs[0]
                continue
            vals[n.index] = n.layer.forward(ctx, n, xs[0] if len(xs) == 1 else xs)
            if ctx.reg is not None and n.layer.activity_regularizer is not None:
                # the activity penalty of the layer's own output (this rank's rows): block partials into the step's slice; the training phase
                # keeps the output for the gradient term of the backward sweep (predict has no ctx.reg: it never adds a penalty)
                y, r = vals[n.index].contiguous(), n.layer.activity_regularizer
                ops.reg_pass(y, None, r.l1, r.l2, ctx.reg[n.index])
                if ctx.training:
                    ctx.reg_y[n.index] = y
            if ctx.capture is not None:
                ctx.capture[n.layer.name] = vals[n.index]
        return [vals[i] for i in self.output_ids]

    def _backward(self, out_grads, ctx):
        """Reverse sweep.  A layer's backward returns one tensor for its single inbound edge, or (merge layers) a list with one entry per inbound
        edge, None where that edge gets no gradient; a merge layer is told which edges want one (need_dx is then a list of booleans: graph
        inputs do not).  Fan-out gradients are summed into the tensor stored first, in place -- but only while no other edge holds the same
        memory: Add hands one dy to all its inputs, Flatten / Reshape / absorbed nodes pass views on.  `held` counts, per storage, the pending
        entries of `grads` that alias it.  An entry that shares its storage is not accumulated into: the first sum goes out of place
        (ops.merge_fwd 'add', the traffic of the in-place axpy) and the result, owned, takes its place.  A layer that overwrites its dy
        (Layer.writes_dy) gets a copy while another entry still holds that storage."""
        grads, held = {}, {}

        def key(t):                        # ops.ConvGrad1 (a deferred data gradient, never summed: Model._plan) stands for itself
            return t.untyped_storage().data_ptr() if isinstance(t, torch.Tensor) else id(t)

        def put(i, t):
            g = grads.get(i)
            if g is None:
                grads[i] = t
                held[key(t)] = held.get(key(t), 0) + 1
            elif held[key(g)] > 1:
                held[key(g)] -= 1
                grads[i] = g = ops.merge_fwd('add', [g.contiguous(), t.contiguous().view(g.shape)])
                held[key(g)] = held.get(key(g), 0) + 1
            else:
                ops.axpy(g, t, 1.0)

        def take(i):
            g = grads.pop(i, None)
            if g is not None:
                held[key(g)] -= 1
                if not held[key(g)]:
                    del held[key(g)]
            return g

        for i, g in zip(self.output_ids, out_grads):
            put(i, g)
        for n in reversed(self.nodes):
            dy = take(n.index)
            if dy is None:
                continue
            if n.index in ctx.reg_y:
                # activity regularizer: l1 sign(y) + 2 l2 y joins the gradient arriving at the layer's output, in place unless another
                # pending edge still holds that storage
                y, r = ctx.reg_y.pop(n.index), n.layer.activity_regularizer
                dy = ops.reg_grad(y, dy.contiguous().view(y.shape), r.l1, r.l2, inplace=key(dy) not in held)
            if n.absorbed:
                dxs = [dy]
            else:
                wanted = [i >= 0 for i in n.inbound]
                need_dx = any(wanted)
                need_dw = ctx.wants_grad(n.layer)
                if not need_dx and not need_dw:
                    continue
                if key(dy) in held and n.layer.writes_dy(n):
                    dy = ops.scale(dy.contiguous(), 1.0)
                if n.layer.is_merge:
                    dxs = n.layer.backward(ctx, n, dy, wanted, need_dw)
                else:
                    prev = ctx.epi.get(n.fuse_prev) if (n.fuse_prev >= 0 and need_dx) else None
                    dxs = [n.layer.backward(ctx, n, dy, need_dx, need_dw, prev) if prev is not None else n.layer.backward(ctx, n, dy, need_dx, need_dw)]
            for i, dx in zip(n.inbound, dxs):
                if i >= 0 and dx is not None:
                    put(i, dx)

    # Model used as a layer inside another graph is expanded by _append, so forward/backward are never called on it.

    # -- keras training surface
    def compile(self, loss=None, optimizer=None, metrics=None, loss_weights=None, data_parallel=None, weighted_metrics=None, sample_weight_mode=None,
                **kwargs):
        """Collects the trainable weights NOW (keras semantics): later changes of .trainable do not affect this model.
        loss: per output a name or alias of LOSSES, a keras.losses callable of the facade, or a callable squared error (K.lower_loss);
        loss_weights: a list, one weight per output; metrics: any of ACC_METRICS / PASS_METRICS (names, aliases, facade callables);
        weighted_metrics: the same names, reported as sum_r w_r m_r / #{w != 0} under the sample weights of the call (ones without)."""
        if sample_weight_mode is not None:
            raise NotImplementedError('sample_weight_mode=%r: only per-sample weights (None), one weight per row' % (sample_weight_mode,))
        self.loss = loss
        n_out = len(self.output_ids)
        losses = list(loss) if isinstance(loss, (list, tuple)) else [loss] * n_out
        self._loss_scales = []
        for k, l in enumerate(losses):
            scale = 1.0
            name = _loss_name(l)
            if name is not None and name != 'categorical_accuracy':
                losses[k] = name
            elif callable(l):              # e.g. the script's chisquare_Loss (bbhMahoGANy.py:146-162): traced once and lowered
                from .keras import backend as K
                losses[k], scale = K.lower_loss(l)
            else:
                raise NotImplementedError('loss %r: only %s, their aliases %s (or a callable squared-error loss) run on the HIP path'
                                          % (l, LOSSES, tuple(sorted(ops.LOSS_ALIASES))))
            self._loss_scales.append(scale)
        self._losses = losses
        if isinstance(loss_weights, dict):
            raise NotImplementedError('loss_weights as a dict: pass a list, one weight per output')
        if loss_weights is not None and len(loss_weights) != n_out:
            raise ValueError('loss_weights has %d entries for %d outputs' % (len(loss_weights), n_out))
        self.loss_weights = None if loss_weights is None else [float(w) for w in loss_weights]
        self._loss_w = self.loss_weights or [1.0] * n_out
        self.metrics = list(metrics or [])
        self.weighted_metrics = list(weighted_metrics or [])

        def kinds(ms):                                # the hit-count accuracy (one column, however often it is named) / the loss-pass metrics
            acc, out = False, []
            for m in ms:
                name = _loss_name(m)
                if not callable(m) and m in ACC_METRICS:
                    acc = True
                elif name in PASS_METRICS:
                    if name not in out:
                        out.append(name)
                else:
                    raise NotImplementedError('metric %r: only %s and %s (or their aliases)' % (m, ACC_METRICS, PASS_METRICS))
            return acc, out
        self._acc, self._metric_kinds = kinds(self.metrics)
        self._wacc, self._wmetric_kinds = kinds(self.weighted_metrics)
        self.optimizer = _get_optimizer(optimizer)
        params, seen = [], set()
        if self.trainable:
            for n in self.nodes:
                if n.layer.trainable and all(o.trainable for o in n.owners):
                    for p in n.layer.trainable_params():
                        if id(p) not in seen:
                            seen.add(id(p)); params.append(p)
        self._train_params = params
        # regularizers, as keras' Network.losses collects them: every weight of every layer of the model that carries one, spliced-in
        # models and frozen layers included (a frozen weight: penalty only), each weight once; every node whose layer regularizes its output
        self._reg_params, regd = [], set()
        for n in self.nodes:
            for p in n.layer.weights:
                if p.regularizer is not None and id(p) not in regd:
                    regd.add(id(p)); self._reg_params.append((p, id(p) in seen))
        self._reg_nodes = [n for n in self.nodes if n.layer.activity_regularizer is not None]
        self._bound = False                # flat grouping + optimizer state are created at the first device step
        if data_parallel is not None:
            self.data_parallel = data_parallel
        return self

    def _ensure_bound(self):
        if not self._bound:
            group_params(self._train_params)
            self.optimizer.bind(self._train_params)
            self._bound = True
            pend = getattr(self, '_pending_optimizer_weights', None)
            if pend is not None:           # optimizer_weights of a loaded .h5, in the layout of the optimizer's class (Optimizer._layout)
                self._pending_optimizer_weights = None
                try:
                    self.optimizer.set_keras_weights(self._keras_train_order(), pend)
                except ValueError as e:    # keras.models.load_model: warns and goes on without the optimizer state
                    import warnings
                    warnings.warn('optimizer state not loaded: %s' % e)

    def _keras_train_order(self):
        """The compiled trainable weights in keras' model.trainable_weights order (the order of optimizer_weights in .h5 files)."""
        from . import keras_io
        ids = set(id(p) for p in self._train_params)
        order = [p for p in keras_io._tw(self) if id(p) in ids]
        seen = set(id(p) for p in order)
        return order + [p for p in self._train_params if id(p) not in seen]

    @property
    def metrics_names(self):
        names = ['loss']
        n_out = len(self.output_ids)
        if n_out > 1:
            names += ['out%d_loss' % k for k in range(n_out)]
        for k in range(n_out):
            for m in ((['acc'] if self._acc else []) + self._metric_kinds
                      + ['weighted_' + w for w in (['acc'] if self._wacc else []) + self._wmetric_kinds]):
                names.append(m if n_out == 1 else 'out%d_%s' % (k, m))
        return names

    def _prep_inputs(self, x):
        xs = list(x) if isinstance(x, (list, tuple)) else [x]
        assert len(xs) == len(self.input_shapes), 'model expects %d input arrays' % len(self.input_shapes)
        out = []
        for a, shp in zip(xs, self.input_shapes):
            t = to_device(a)
            if tuple(t.shape[1:]) != tuple(shp):
                t = t.reshape((t.shape[0],) + tuple(shp))
            out.append(t)
        return out

    def _prep_targets(self, y, B):
        n_out = len(self.output_ids)
        ys = list(y) if (isinstance(y, (list, tuple)) and n_out > 1) else [y]
        assert len(ys) == n_out, 'model has %d outputs' % n_out
        return [to_device(a).reshape(B, -1) for a in ys]

    def _prep_weights(self, sample_weight, class_weight, y, B):
        """keras' standardize_weights on the host: per output a float32 (B,) array or None (= ones); None when no output is weighted.
        class_weight {class: weight} (single-output models) becomes the sample weights of the rows' classes: argmax of a row of y, or y[:, 0]
        itself when y has one column.  Raises before anything is launched."""
        n_out = len(self.output_ids)
        if isinstance(sample_weight, dict):
            raise NotImplementedError('sample_weight as a dict: pass a list, one entry (or None) per output')
        if class_weight is not None and not isinstance(class_weight, dict):
            raise ValueError('class_weight is a dict {class: weight}')
        if class_weight is not None and n_out != 1:
            raise ValueError('class_weight is supported for models with a single output only (this one has %d)' % n_out)
        if sample_weight is not None:
            if class_weight is not None:
                import warnings
                warnings.warn('both sample_weight and class_weight were given: class_weight is ignored', UserWarning)
            if n_out == 1:
                one = isinstance(sample_weight, (list, tuple)) and len(sample_weight) == 1 and np.ndim(sample_weight[0]) > 0
                sws = [sample_weight[0] if one else sample_weight]
            else:
                if not isinstance(sample_weight, (list, tuple)) or len(sample_weight) != n_out:
                    raise ValueError('sample_weight of a model with %d outputs is a list with one entry (or None) per output' % n_out)
                sws = list(sample_weight)
            out = []
            for k, w in enumerate(sws):
                if w is None:
                    out.append(None)
                    continue
                w = np.asarray(w.detach().cpu().numpy() if isinstance(w, torch.Tensor) else w, dtype=np.float32)
                if w.ndim != 1:
                    raise ValueError('sample_weight of output %d has shape %s: one weight per row, a 1-D array, is expected' % (k, w.shape))
                if w.shape[0] != B:
                    raise ValueError('sample_weight of output %d has %d entries for %d rows' % (k, w.shape[0], B))
                out.append(np.ascontiguousarray(w))
            return out if any(w is not None for w in out) else None
        if class_weight is None:
            return None
        y = np.asarray(y.detach().cpu().numpy() if isinstance(y, torch.Tensor) else y).reshape(B, -1)
        cls = np.argmax(y, axis=1) if y.shape[1] > 1 else y[:, 0]
        table = dict((float(k), float(v)) for k, v in class_weight.items())
        missing = sorted(set(float(c) for c in cls) - set(table))
        if missing:
            raise ValueError('class_weight has no entry for the classes %s that y holds' % missing)
        return [np.array([table[float(c)] for c in cls], dtype=np.float32)]

    def train_on_batch(self, x, y, dropout_masks=None, capture=None, row_map=None, sample_weight=None, class_weight=None):
        """One optimizer step.  Returns [loss, (per-output losses,) (accuracies)] as python floats, keras order.
        sample_weight: one weight per row (a list with one entry or None per output on multi-output models); class_weight: {class: weight},
        single-output models.  The loss is sum_r w_r l_r / #{w != 0} over the GLOBAL batch, as Keras 2.2.4.
        `dropout_masks` ({dropout layer name: uint8 keep mask}) is a testing hook that replaces the Philox draws; `capture` (a dict) is
        another: it receives {layer name: output tensor} of every executed layer (outputs include the fused activation / dropout).
        row_map (data parallelism): ([(global_row_start, n_rows), ...], global_rows) when the local rows are not the rank's contiguous slice
        [rank * B, (rank + 1) * B) of the global batch (the default) -- the discriminator batch of bbh.gan_train_step."""
        xs = self._prep_inputs(x)
        B = xs[0].shape[0]
        sws = self._weights_to_device(self._prep_weights(sample_weight, class_weight, y, B))
        ys = self._prep_targets(y, B)
        stats = self.train_on_batch_device(xs, ys, dropout_masks, capture, row_map, sws)
        return self.train_result(stats, B)

    @staticmethod
    def _weights_to_device(sws):
        return None if sws is None else [None if w is None else to_device(w) for w in sws]

    def train_on_batch_device(self, xs, ys, dropout_masks=None, capture=None, row_map=None, sample_weights=None):
        """train_on_batch on device tensors (inputs as the graph takes them, targets (B, 1)) without the final device -> host read: returns
        the (n_outputs, 2) device tensor [summed loss term, metric hits] that train_result turns into keras' list.  No host synchronisation
        anywhere in it, so the whole step can be captured into a hipGraph (engine.StepGraph).  sample_weights: per output a (B,) device tensor
        or None; their non-zero count stays on the device, so a captured step replays with whatever the tensors hold then."""
        if self.optimizer is None:
            raise RuntimeError('compile() the model before train_on_batch')
        self._ensure_bound()
        B = xs[0].shape[0]
        dp = self.data_parallel
        world = dp.world_size if dp is not None else 1
        masks = {k: to_device(v, torch.uint8) for k, v in (dropout_masks or {}).items()}
        if row_map is None and dp is not None and world > 1:
            row_map = ([(dp.rank * B, B)], B * world)
        ctx = RunContext(True, dp, masks, self._train_params, self.name, row_map)
        ctx.capture = capture
        reg = self._reg_begin(ctx, B)
        outs = self._forward(xs, ctx)
        dps, stats = self._loss_stats(outs, ys, B, world, True, sample_weights)
        for grp, a, b in segments(self._train_params):
            grp.grad[a:b].zero_()
        self._backward(dps, ctx)
        stats = torch.stack(stats)
        if dp is not None:
            for grp, a, b in segments(self._train_params):
                dp.all_reduce_sum(grp.grad[a:b])
            dp.all_reduce_sum(stats)
        if reg is not None:                # after the all-reduce (the gradients are the global mean), before the optimizer's clipping sees them
            stats = self._reg_end(reg, stats, True)
        self.optimizer.step()
        return stats

    # -- regularizers.  A model without any never enters these: reg is None, its launches and its statistics tensor are unchanged.
    def _reg_begin(self, ctx, B):
        """The step's fp64 penalty partials, one slice per regularized weight and then one per activity-regularized node (ctx.reg: the forward
        sweep fills those).  The slice sizes depend on the tensor sizes alone (ops.reg_partials).  None for a model without regularizers."""
        if not self._reg_params and not self._reg_nodes:
            return None
        off, wsl, asl = 0, [], []
        for p, _ in self._reg_params:
            k = ops.reg_partials(p.size)
            wsl.append((off, k)); off += k
        w_end = off
        for n in self._reg_nodes:
            k = ops.reg_partials(B * int(np.prod(n.out_shape)))
            asl.append((n.index, off, k)); off += k
        parts = torch.zeros(off, dtype=torch.float64, device=device())     # zeros: a slice no pass reached would add nothing
        ctx.reg = dict((i, parts[a:a + k]) for i, a, k in asl)
        return parts, wsl, w_end

    def _reg_end(self, reg, stats, train):
        """One pass per regularized weight: its penalty partials and, in a training step, its gradient term l1 sign(w) + 2 l2 w added ONCE to
        the (already all-reduced) gradient of a weight this model trains; a frozen weight, and every weight in the test phase: penalty only.
        The activity partials are this rank's sums: all-reduced beside the statistics.  Then one fixed-order sum of everything, on the device;
        it returns the statistics with one more row, [penalty, 0, ...], which train_result adds to entry 0."""
        parts, wsl, w_end = reg
        dp = self.data_parallel
        if dp is not None and parts.numel() > w_end:
            dp.all_reduce_sum(parts[w_end:])
        for (p, trained), (a, k) in zip(self._reg_params, wsl):
            ops.reg_pass(p.data, p.grad if train and trained else None, p.regularizer.l1, p.regularizer.l2, parts[a:a + k])
        row = torch.zeros((1, stats.shape[1]), dtype=torch.float32, device=stats.device)
        ops.reg_finish(parts, row[0, :1])
        return torch.cat([stats, row])

    def _loss_stats(self, outs, ys, B, world, grad, sws=None):
        """Per output: the loss (with its gradient when `grad`) and the compiled metrics, all on the device.  Returns (gradients, the
        (n_outputs, 2 + #loss-pass metrics) tensor [loss term, hits, metric, ...]; with weighted_metrics compiled the rows go on with
        [weighted hit share, weighted metric, ...]).
        sws: per output a (B,) weight tensor of the LOCAL rows or None (ones).  A weighted output always takes ops.loss_pass_weighted (the
        one-block kernels have no weighted form), normalised by the number of non-zero weights of the GLOBAL batch: every weighted output's
        count is taken first and all of them cross the ranks in ONE all-reduce."""
        dps, stats = [], []
        sws = list(sws) if sws is not None else [None] * len(outs)
        if len(sws) != len(outs):
            raise ValueError('%d sample weight entries for %d outputs' % (len(sws), len(outs)))
        for k, sw in enumerate(sws):
            if sw is not None and (tuple(sw.shape) != (B,) or sw.dtype != torch.float32):
                raise ValueError('sample weights of output %d: a float32 tensor of shape (%d,) is expected, got %s %s' % (k, B, tuple(sw.shape), sw.dtype))
        weighted = [k for k, sw in enumerate(sws) if sw is not None]
        counts = None
        if weighted:
            counts = torch.empty((len(weighted),), dtype=torch.float64, device=outs[0].device)
            for j, k in enumerate(weighted):
                ops.weight_count(sws[k], counts[j:j + 1])
            if self.data_parallel is not None:
                self.data_parallel.all_reduce_sum(counts)
        wcols = self._wacc or bool(self._wmetric_kinds)
        for k, (p, t, kind, scale, w) in enumerate(zip(outs, ys, self._losses, self._loss_scales, self._loss_w)):
            if sws[k] is not None:
                n = p.numel() // B
                p2, t2, cnt = p.reshape(B, n), t.reshape(B, n), counts[weighted.index(k):weighted.index(k) + 1]
                d, o = ops.loss_pass_weighted(kind, p2, t2, sws[k], cnt, grad=grad)
                if grad:
                    if scale * w != 1.0:
                        ops.axpy(d, d.clone(), scale * w - 1.0)
                    dps.append(d.reshape(p.shape))
                cols = [o[:2]] + [ops.loss_pass(m, p2, t2, B * world, grad=False)[1][:1] for m in self._metric_kinds]     # metrics= stay unweighted
                if wcols:
                    cols += [o[2:]] + [ops.loss_pass_weighted(m, p2, t2, sws[k], cnt, grad=False)[1][:1] for m in self._wmetric_kinds]
                stats.append(torch.cat(cols) if len(cols) > 1 else cols[0])
                continue
            # keras: the loss is the mean over the output's columns, then over the global batch.  The two losses of the first kernel keep it
            # while the output is small (the element-wise kernel over all B * n values, normalised by the global element count: the bits every
            # (B, 1) head always had); every other kind, every larger output and every evaluation is one ops.loss_pass over (B, n)
            n = p.numel() // B if B else 1
            p2, t2 = p.reshape(B, n), t.reshape(B, n)
            if grad and kind in OLD_KERNEL_LOSSES and B * n < ops.LOSS_PASS_MIN_ELEMENTS:
                d, o = ops.loss(kind, p.reshape(B * n, 1), t.reshape(B * n, 1), B * world * n)
            else:
                d, o = ops.loss_pass(kind, p2, t2, B * world, grad=grad)
            if grad:
                if scale * w != 1.0:
                    ops.axpy(d, d.clone(), scale * w - 1.0)
                dps.append(d.reshape(p.shape))
            if self._metric_kinds or wcols:
                ms = dict((m, ops.loss_pass(m, p2, t2, B * world, grad=False)[1][:1])
                          for m in self._metric_kinds + [m for m in self._wmetric_kinds if m not in self._metric_kinds])
                cols = [o] + [ms[m] for m in self._metric_kinds]
                if wcols:                  # weights of ones: every weighted metric is the plain one, the hit share hits / (B world n)
                    cols += [o[1:2] * (1.0 / (B * world * n))] + [ms[m] for m in self._wmetric_kinds]
                o = torch.cat(cols)
            stats.append(o)
        return dps, stats

    def test_on_batch(self, x, y, sample_weight=None):
        """keras test_on_batch: the inference-phase forward (as predict) and the compiled loss and metrics of it; no backward, no optimizer step.
        Returns the list train_on_batch returns."""
        xs = self._prep_inputs(x)
        B = xs[0].shape[0]
        sws = self._weights_to_device(self._prep_weights(sample_weight, None, y, B))
        return self.train_result(self.test_on_batch_device(xs, self._prep_targets(y, B), sws), B)

    def test_on_batch_device(self, xs, ys, sample_weights=None):
        """test_on_batch on device tensors without the device -> host read: the statistics tensor of train_on_batch_device."""
        if self.optimizer is None:
            raise RuntimeError('compile() the model before test_on_batch')
        B = xs[0].shape[0]
        dp = self.data_parallel
        world = dp.world_size if dp is not None else 1
        ctx = RunContext(False)
        reg = self._reg_begin(ctx, B)      # keras adds the penalties in the test phase too (never in predict)
        outs = self._forward(xs, ctx)
        stats = torch.stack(self._loss_stats(outs, ys, B, world, False, sample_weights)[1])
        if dp is not None:
            dp.all_reduce_sum(stats)
        if reg is not None:
            stats = self._reg_end(reg, stats, False)
        return stats

    def evaluate(self, x, y, batch_size=32, verbose=0, sample_weight=None):
        """keras evaluate: the mean of test_on_batch over chunks of batch_size rows, each weighted by its row count.  With sample_weight every
        chunk is normalised by its OWN count of non-zero weights (keras' test_loop)."""
        if self.data_parallel is not None:
            raise NotImplementedError('evaluate under data_parallel: call test_on_batch on each rank\'s rows')
        xs = self._prep_inputs(x)
        B = xs[0].shape[0]
        sws = self._weights_to_device(self._prep_weights(sample_weight, None, y, B))
        ys = self._prep_targets(y, B)
        tot = None
        for s in range(0, B, batch_size):
            nb = min(batch_size, B - s)
            sw = None if sws is None else [None if w is None else w[s:s + nb] for w in sws]
            r = np.asarray(self.train_result(self.test_on_batch_device([t[s:s + nb] for t in xs], [t[s:s + nb] for t in ys], sw), nb)) * nb
            tot = r if tot is None else tot + r
        res = [float(v) / B for v in tot]
        if verbose:
            print(' - '.join('%s: %.6f' % (n, v) for n, v in zip(self.metrics_names, res)))
        return res

    def predict_on_batch(self, x):
        """keras predict_on_batch: one inference-phase forward over all rows of x, no chunking."""
        outs = [o.cpu().numpy() for o in self._forward(self._prep_inputs(x), RunContext(False))]
        return outs if len(outs) > 1 else outs[0]

    def train_result(self, stats, B):
        """[loss, (per-output losses,) (accuracies)] as python floats, keras order, from train_on_batch_device's statistics (one device -> host read)."""
        world = self.data_parallel.world_size if self.data_parallel is not None else 1
        st = stats.cpu().numpy().astype(np.float64)
        penalty = 0.0
        if st.shape[0] == len(self.output_ids) + 1:        # a regularized model: the last row holds the sum of all penalties (_reg_end)
            penalty, st = float(st[-1, 0]), st[:-1]
        losses = [float(v) * sc for v, sc in zip(st[:, 0], self._loss_scales)]
        # per-output entries stay unweighted, as keras reports them; the penalties enter entry 0 alone, once
        res = [float(sum(l * w for l, w in zip(losses, self._loss_w))) + penalty]
        if len(losses) > 1:
            res += losses
        cols = [int(np.prod(self.nodes[i].out_shape)) for i in self.output_ids]
        nm = 2 + len(self._metric_kinds)              # then, with weighted_metrics compiled: [weighted hit share, weighted metric, ...]
        for row, n in zip(st, cols):
            if self._acc:
                res.append(float(row[1]) / (B * world * n))
            res += [float(v) for v in row[2:nm]]
            if self._wacc:
                res.append(float(row[nm]))
            res += [float(v) for v in row[nm + 1:]]
        return res

    def predict_device(self, x, batch_size=32):
        """predict() that keeps inputs and outputs in HBM (torch tensors): inference phase, chunks of batch_size."""
        xs = self._prep_inputs(x)
        B = xs[0].shape[0]
        if B == 0:                         # nothing to run: empty outputs of the right shapes (the kernels are never launched)
            outs = [torch.empty((0,) + tuple(self.nodes[i].out_shape), dtype=torch.float32, device=device()) for i in self.output_ids]
            return outs if len(outs) > 1 else outs[0]
        chunks = []
        for s in range(0, B, batch_size):
            ctx = RunContext(False)
            chunks.append(self._forward([t[s:s + batch_size] for t in xs], ctx))
        outs = [torch.cat([c[k] for c in chunks]) if len(chunks) > 1 else chunks[0][k] for k in range(len(self.output_ids))]
        return outs if len(outs) > 1 else outs[0]

    def predict(self, x, batch_size=32, verbose=0):
        out = self.predict_device(x, batch_size)
        if isinstance(out, list):
            return [o.cpu().numpy() for o in out]
        return out.cpu().numpy()

    def fit(self, x, y, batch_size=32, epochs=1, verbose=0, shuffle=True, sample_weight=None, class_weight=None, validation_data=None, **kwargs):
        """Minimal keras fit: epochs of shuffled mini-batches through train_on_batch; returns {'loss': [...]}.  sample_weight / class_weight
        are shuffled with the rows.  validation_data (x, y) or (x, y, sample_weight) is evaluated after every epoch and adds 'val_loss' and
        one 'val_<name>' per compiled metric to the history."""
        x = np.asarray(x)
        n = x.shape[0]
        ys = list(y) if (isinstance(y, (list, tuple)) and len(self.output_ids) > 1) else [y]
        ys = [np.asarray(a) for a in ys]
        sws = self._prep_weights(sample_weight, class_weight, ys[0], n)
        if validation_data is not None and len(validation_data) not in (2, 3):
            raise ValueError('validation_data is (x, y) or (x, y, sample_weight)')
        hist = {'loss': []}
        rng = np.random.RandomState(0)
        for ep in range(epochs):
            order = rng.permutation(n) if shuffle else np.arange(n)
            tot, cnt = 0.0, 0
            for s in range(0, n, batch_size):
                idx = order[s:s + batch_size]
                yy = [a[idx] for a in ys]
                sw = None if sws is None else [None if w is None else w[idx] for w in sws]
                r = self.train_on_batch(x[idx], yy if len(yy) > 1 else yy[0], sample_weight=sw if sw is None or len(sw) > 1 else sw[0])
                tot += r[0] * len(idx); cnt += len(idx)
            hist['loss'].append(tot / max(cnt, 1))
            if validation_data is not None:
                val = self.evaluate(validation_data[0], validation_data[1], batch_size=batch_size,
                                    sample_weight=validation_data[2] if len(validation_data) == 3 else None)
                for name, v in zip(self.metrics_names, val):
                    hist.setdefault('val_' + name, []).append(v)
            if verbose:
                print('Epoch %d/%d - loss: %.6f' % (ep + 1, epochs, hist['loss'][-1])
                      + (' - val_loss: %.6f' % hist['val_loss'][-1] if validation_data is not None else ''))
        return hist

    def summary(self, print_fn=None):
        lines = ['_' * 65, '%-29s%-26s%s' % ('Layer (type)', 'Output Shape', 'Param #'), '=' * 65]
        tot = 0
        for n in self.nodes:
            cnt = n.layer.count_params()
            tot += cnt
            lines.append('%-29s%-26s%d' % ('%s (%s)' % (n.layer.name, n.layer.__class__.__name__), str((None,) + tuple(n.out_shape)), cnt))
        tr = sum(p.size for p in self.trainable_weights)
        lines += ['=' * 65, 'Total params: {:,}'.format(tot), 'Trainable params: {:,}'.format(tr), 'Non-trainable params: {:,}'.format(tot - tr), '_' * 65]
        s = '\n'.join(lines)
        (print_fn or print)(s)

    # -- persistence: Keras' HDF5 layout through gennet_amd/keras_io.py + h5lite.py (bbhMahoGANy.py:1135-1142, :1171-1173, :1372-1375)
    def save_weights(self, filepath, overwrite=True, writer=None):
        """`writer` (a hostio.BackgroundWriter, not a keras argument): the weights are copied to the host now, the file is written by the
        writer's thread."""
        import os
        from . import keras_io
        if os.path.exists(filepath) and not overwrite:
            raise IOError('%s exists' % filepath)
        keras_io.save_weights(self, filepath, writer)

    def load_weights(self, filepath, by_name=False):
        from . import keras_io
        if by_name:
            raise NotImplementedError('load_weights(by_name=True)')
        keras_io.load_weights(self, filepath)      # raises h5lite.H5Error on anything that is not an HDF5 file (never unpickles)

    def save(self, filepath, overwrite=True, include_optimizer=True, writer=None):
        import os
        from . import keras_io
        if os.path.exists(filepath) and not overwrite:
            raise IOError('%s exists' % filepath)
        keras_io.save_model(self, filepath, include_optimizer, writer)

    def get_config(self):
        from . import keras_io
        return keras_io.model_config(self)['config']

    def to_json(self):
        import json
        from . import keras_io
        return json.dumps(keras_io.model_config(self))


class Sequential(Model):
    def __init__(self, layers=None, name=None):
        Model.__init__(self, name=name)
        self._top = []                     # what was add()-ed, nested models unflattened: keras' `model.layers`
        for l in (layers or []):
            self.add(l)

    def add(self, layer):
        if not self.nodes:
            shp = layer.input_shape_arg if not isinstance(layer, Model) else (layer.input_shapes[0] if layer.input_shapes else None)
            if shp is None:
                raise ValueError('the first layer of a Sequential needs input_shape=')
            self.input_shapes = [tuple(shp)]
            prev, prev_shape = -1, tuple(shp)
        else:
            prev = self.output_ids[0]
            prev_shape = self.nodes[prev].out_shape
        if isinstance(layer, Model):
            out_shape = layer.nodes[layer.output_ids[0]].out_shape
        else:
            layer._ensure_built(prev_shape)
            out_shape = layer._shape_after(prev_shape)
        idx = self._append(layer, [prev], out_shape)
        self._top.append(layer)
        self.output_ids = [idx]
        self.built = True
        return self


def load_model(filepath, custom_objects=None, compile=True):
    """keras.models.load_model: rebuilds the model from the file's model_config, loads model_weights, and (compile=True)
    re-creates the optimizer with its iteration count and Adam moments.  Custom layers (the script's MyLayer,
    bbhMahoGANy.py:164-188, needs its constant) come through custom_objects={'MyLayer': layer_instance | class | factory(config)}."""
    from . import keras_io
    return keras_io.load_model(filepath, custom_objects, compile)


def model_from_json(text, custom_objects=None):
    import json
    from . import keras_io
    return keras_io.model_from_config(json.loads(text), custom_objects)
