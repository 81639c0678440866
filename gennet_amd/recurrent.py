"""keras.layers.LSTM, keras.layers.GRU and keras.layers.SimpleRNN (keras 2.2.4 layers/recurrent.py) on the persistent fp32 matrix-core recurrences
of csrc/lstm.hip, csrc/gru.hip and csrc/rnn.hip; DESIGN 8o, 8p, 8s.  keras.layers.Bidirectional (layers/wrappers.py) over any of them: both
directions in one launch; DESIGN 8q.

The classes are part of the gennet_amd.layers name space (gennet_amd.layers.LSTM is this LSTM), as every layer is."""
import numpy as np

from . import engine, ops, regularizers
from .engine import Layer

_ACTIVATIONS = ('tanh', 'sigmoid', 'relu', 'linear')
_RECURRENT_ACTIVATIONS = ('hard_sigmoid', 'sigmoid')
_ABSENT = object()                  # what SimpleRNN hands _init_recurrent for the keys its constructor does not have


def _name_of(v):
    return getattr(v, '__name__', v) if callable(v) else v


def _initializer_is(v, name, class_names, **config):
    """whether `v` (a name, None, or the config dict keras serializes) is the initializer `name`"""
    if v is None or v == name:
        return True
    return isinstance(v, dict) and v.get('class_name') in class_names and all((v.get('config') or {}).get(k, d) == d for k, d in config.items())


def orthogonal_blocks(u, n=4):
    """(u, n u): n orthogonal u x u blocks side by side, each the Q of the QR factorisation of a standard normal draw with the signs fixed so
    that R's diagonal is positive (the draw then is uniform over the orthogonal group); from the generator glorot_uniform draws from."""
    blocks = []
    for _ in range(n):
        q, r = np.linalg.qr(engine._INIT_RNG.normal(0.0, 1.0, size=(u, u)))
        blocks.append(q * np.where(np.diag(r) < 0, -1.0, 1.0)[None, :])
    return np.concatenate(blocks, axis=1).astype(np.float32)


_SPLIT_MIN_ROWS, _SPLIT_MAX, _SPLIT_MAX_BYTES = 256, 64, 64 << 20


def row_splits(rows, cols):
    """In how many equal parts the B T rows of a weight-gradient product are summed: gn_bmm has no split-K, so one (Cin, 4u) or (u, 4u) result
    over all rows is a handful of blocks walking tens of thousands of rows each.  The largest divisor of `rows` that is at most 64, leaves at
    least 256 rows a part and keeps the (parts, cols) partial results inside 64 MiB; 1 where there is none.  By shape alone."""
    best = 1
    for parts in range(2, _SPLIT_MAX + 1):
        if rows % parts == 0 and rows // parts >= _SPLIT_MIN_ROWS and parts * cols * 4 <= _SPLIT_MAX_BYTES:
            best = parts
    return best


def rows_product(a, dz, out):
    """out (K, N) = a^T . dz for a (rows, K), dz (rows, N): one gn_bmm, or row_splits parts as one batched gn_bmm whose partial results are summed
    by the fixed-order fp64 column reduction (ops.bias_grad over the (parts, K N) view).  Deterministic either way."""
    rows, K, N = a.shape[0], a.shape[1], dz.shape[1]
    parts = row_splits(rows, K * N)
    if parts == 1:
        return ops.bmm(a.view(1, rows, K), dz.view(1, rows, N), trans_a=True, out=out.view(1, K, N))
    part = ops.bmm(a.view(parts, rows // parts, K), dz.view(parts, rows // parts, N), trans_a=True)
    return ops.bias_grad(part.view(parts, K * N), out.view(K * N))


def _init_recurrent(layer, what, kw, units, activation, recurrent_activation, use_bias, kernel_initializer, recurrent_initializer, bias_initializer,
                    kernel_regularizer, recurrent_regularizer, bias_regularizer, activity_regularizer, return_sequences, go_backwards,
                    implementation, unroll):
    """What LSTM, GRU and SimpleRNN share of their constructors: the refusals, each naming its key (`what` is the class name), Layer.__init__ over
    the rest of kw, and the attributes the configs write.  SimpleRNN has no recurrent_activation and no implementation: it hands _ABSENT for
    both, and neither is checked or set."""
    for key in ('dropout', 'recurrent_dropout'):
        if float(kw.pop(key, 0.0) or 0.0) != 0.0:
            raise NotImplementedError('%s(%s=...): dropout inside the cell is not implemented; only 0 runs' % (what, key))
    for key in ('stateful', 'return_state'):
        if kw.pop(key, False):
            raise NotImplementedError('%s(%s=True) is not implemented' % (what, key))
    for key in ('kernel_constraint', 'recurrent_constraint', 'bias_constraint'):
        if kw.pop(key, None) is not None:
            raise NotImplementedError('%s(%s=...): weight constraints are not implemented' % (what, key))
    if not use_bias:
        raise NotImplementedError('%s(use_bias=False)' % what)
    act, ract = _name_of(activation), recurrent_activation if recurrent_activation is _ABSENT else _name_of(recurrent_activation)
    act = 'linear' if act is None else act
    if act not in _ACTIVATIONS:
        raise NotImplementedError('%s(activation=%r): one of %s' % (what, activation, ', '.join(_ACTIVATIONS)))
    if ract is not _ABSENT and ract not in _RECURRENT_ACTIVATIONS:
        raise NotImplementedError('%s(recurrent_activation=%r): one of %s' % (what, recurrent_activation, ', '.join(_RECURRENT_ACTIVATIONS)))
    if not _initializer_is(kernel_initializer, 'glorot_uniform', ('GlorotUniform', 'VarianceScaling'), mode='fan_avg', distribution='uniform'):
        raise NotImplementedError('%s(kernel_initializer=%r): only glorot_uniform' % (what, kernel_initializer))
    if not _initializer_is(recurrent_initializer, 'orthogonal', ('Orthogonal',), gain=1.0):
        raise NotImplementedError('%s(recurrent_initializer=%r): only orthogonal' % (what, recurrent_initializer))
    if not _initializer_is(bias_initializer, 'zeros', ('Zeros',)):
        raise NotImplementedError('%s(bias_initializer=%r): only zeros' % (what, bias_initializer))
    if implementation is not _ABSENT and implementation not in (1, 2):
        raise ValueError('%s(implementation=%r): 1 or 2' % (what, implementation))
    Layer.__init__(layer, **kw)
    layer.units = int(units)
    if layer.units < 1:
        raise ValueError('%s(units=%r): at least 1' % (what, units))
    layer.activation = act
    if ract is not _ABSENT:
        layer.recurrent_activation = ract
    layer.kernel_regularizer, layer.recurrent_regularizer = regularizers.get(kernel_regularizer), regularizers.get(recurrent_regularizer)
    layer.bias_regularizer, layer.activity_regularizer = regularizers.get(bias_regularizer), regularizers.get(activity_regularizer)
    layer.return_sequences, layer.go_backwards = bool(return_sequences), bool(go_backwards)
    layer.unroll = bool(unroll)
    if implementation is not _ABSENT:
        layer.implementation = int(implementation)


def _add_triple(owner, cell, prefix, Cin):
    """kernel (Cin, G u), recurrent_kernel (u, G u) and bias of `cell` (an LSTM, a GRU or a SimpleRNN) as Params of `owner` under `prefix`, drawn in
    keras' order from the generator glorot_uniform draws from, each with the cell's regularizer"""
    u, G = cell.units, cell.n_gates
    return (owner.add_weight(prefix + 'kernel', engine.glorot_uniform((Cin, G * u)), regularizer=cell.kernel_regularizer),
            owner.add_weight(prefix + 'recurrent_kernel', orthogonal_blocks(u, G), regularizer=cell.recurrent_regularizer),
            owner.add_weight(prefix + 'bias', cell.initial_bias(), regularizer=cell.bias_regularizer))


def _input_grad(dz, kernel, x_shape):
    """dX = dz . W^T over the B T rows"""
    B, T, Cin = x_shape
    G = dz.shape[2]
    return ops.bmm(dz.view(1, B * T, G), kernel.data.view(1, Cin, G), trans_b=True).view(B, T, Cin)


class GRU(Layer):
    """keras.layers.GRU(units): (B, T, Cin) -> (B, units), or (B, T, units) with return_sequences.  GRUCell of keras 2.2.4, gate columns z, r, h
    in kernel (Cin, 3u), recurrent_kernel (u, 3u) and bias (3u), or (2, 3u) under reset_after (row 0 the input bias b, row 1 the recurrent rb):
        a_t = x_t . W + b
        reset_after=False:  m = h_{t-1} . U[:, :2u];  z = ra(a_z + m_z), r = ra(a_r + m_r);  hh = act(a_h + (r h_{t-1}) . U_h)
        reset_after=True:   m = h_{t-1} . U + rb;     z = ra(a_z + m_z), r = ra(a_r + m_r);  hh = act(a_h + r m_h)
        h_t = z h_{t-1} + (1 - z) hh
    with act one of tanh, sigmoid, relu, linear and ra hard_sigmoid or sigmoid; h_0 = 0.  go_backwards, implementation and unroll as in LSTM.
    Forward: zx = X . W as one gn_bmm over B T rows, then gn_gru_fwd, one launch that walks the T steps with h on chip.
    Backward: gn_gru_bwd walks the steps down and writes dz (B, T, 3u) = da_z, da_r, da_h: dW = X^T dz, dX = dz W^T, db = sum dz.
    reset_after=True: it also writes dzr = da_z, da_r, dq: dU = hprev^T dzr, d rb = sum dzr.  reset_after=False: dU has two column blocks from two
    left operands, dU[:, :2u] = hprev^T dz[:, :2u] and dU[:, 2u:] = (r hprev)^T da_h; dz is cut into its two column blocks (the concatenate
    pass backwards), each block is one rows_product, and the concatenate pass joins them: fixed order, no atomics.  The tape keeps x, hprev, the
    gates and aux (r hprev, or m_h), in the training phase only.  The planner fuses nothing onto the layer, and dy is not written."""

    def __init__(self, units, activation='tanh', recurrent_activation='hard_sigmoid', use_bias=True, kernel_initializer='glorot_uniform',
                 recurrent_initializer='orthogonal', bias_initializer='zeros', kernel_regularizer=None, recurrent_regularizer=None,
                 bias_regularizer=None, activity_regularizer=None, return_sequences=False, go_backwards=False, implementation=1, unroll=False,
                 reset_after=False, **kw):
        _init_recurrent(self, 'GRU', kw, units, activation, recurrent_activation, use_bias, kernel_initializer, recurrent_initializer, bias_initializer,
                        kernel_regularizer, recurrent_regularizer, bias_regularizer, activity_regularizer, return_sequences, go_backwards,
                        implementation, unroll)
        self.reset_after = bool(reset_after)

    def build(self, input_shape):
        if len(input_shape) != 2:
            raise ValueError('%s (GRU) expects (batch, timesteps, features), got %r' % (self.name, (None,) + tuple(input_shape)))
        Cin, u = int(input_shape[1]), self.units
        if u > 512:
            raise NotImplementedError('%s: GRU(units=%d): at most 512 units run (a block carries all units of its samples on chip)' % (self.name, u))
        self.kernel, self.recurrent_kernel, self.bias = _add_triple(self, self, '', Cin)

    n_gates = 3

    def initial_bias(self):
        return np.zeros((2, 3 * self.units) if self.reset_after else (3 * self.units,), np.float32)

    def compute_output_shape(self, input_shape):
        return (int(input_shape[0]), self.units) if self.return_sequences else (self.units,)

    def forward(self, ctx, node, x):
        x = x.contiguous()
        B, T, Cin = x.shape
        u = self.units
        zx = ops.bmm(x.view(1, B * T, Cin), self.kernel.data.view(1, Cin, 3 * u)).view(B, T, 3 * u)
        b2 = self.bias.data.view(-1, 3 * u)
        h, gates, hprev, aux = ops.gru_fwd(zx, self.recurrent_kernel.data, b2[0], b2[1] if self.reset_after else None, None, self.activation,
                                           self.recurrent_activation, reset_after=self.reset_after, reverse=self.go_backwards, training=ctx.training)
        if ctx.training:
            ctx.tape[node.index] = (x, hprev, gates, aux)
        return h if self.return_sequences else h[:, T - 1, :].contiguous()

    def backward(self, ctx, node, dy, need_dx, need_dw):
        x, hprev, gates, aux = ctx.tape.pop(node.index)
        B, T, _ = x.shape
        u = self.units
        dz, dzr, _ = ops.gru_bwd(dy.contiguous().view((B, T, u) if self.return_sequences else (B, u)), gates, hprev, aux, self.recurrent_kernel.data,
                                 self.activation, self.recurrent_activation, reset_after=self.reset_after, reverse=self.go_backwards)
        if need_dw:
            self.weight_grads(x, (hprev, gates, aux), dz, dzr, self.kernel, self.recurrent_kernel, self.bias)
        return _input_grad(dz, self.kernel, x.shape) if need_dx else None

    def weight_grads(self, x, kept, dz, dzr, kernel, recurrent_kernel, bias):
        """the gradients of one direction's three weights from what its recurrence stored (kept = hprev, gates, aux) and its backward wrote"""
        hprev, _, aux = kept
        B, T, Cin = x.shape
        u = self.units
        dz2 = dz.view(B * T, 3 * u)
        rows_product(x.view(B * T, Cin), dz2, kernel.grad)
        db = bias.grad.view(-1, 3 * u)
        ops.bias_grad(dz2, db[0])
        if self.reset_after:
            dzr2 = dzr.view(B * T, 3 * u)
            rows_product(hprev.view(B * T, u), dzr2, recurrent_kernel.grad)
            ops.bias_grad(dzr2, db[1])
        else:
            dzr_zr, dz_h = ops.concat_bwd(dz2, [(B * T, 2 * u), (B * T, u)], 1)
            dU_zr, dU_h = dz.new_empty((u, 2 * u)), dz.new_empty((u, u))
            rows_product(hprev.view(B * T, u), dzr_zr, dU_zr)
            rows_product(aux.view(B * T, u), dz_h, dU_h)
            ops.concat_fwd([dU_zr, dU_h], 1, out=recurrent_kernel.grad)


class LSTM(Layer):
    """keras.layers.LSTM(units): (B, T, Cin) -> (B, units), or (B, T, units) with return_sequences.  LSTMCell of keras 2.2.4, gate columns
    i, f, c, o in kernel (Cin, 4u), recurrent_kernel (u, 4u) and bias (4u):
        z_t = x_t . W + h_{t-1} . U + b;  i = ra(z_i), f = ra(z_f), g = act(z_c), o = ra(z_o);  c_t = f c_{t-1} + i g;  h_t = o act(c_t)
    with act one of tanh, sigmoid, relu, linear and ra hard_sigmoid or sigmoid; h_0 = c_0 = 0.  go_backwards walks the sequence from its last
    sample, and the returned sequence is in processing order, as keras leaves it.  implementation 1 and 2 are one arithmetic here and unroll is a
    hint; both are kept for the config.
    Forward: zx = X . W for all steps as one gn_bmm over B T rows, then gn_lstm_fwd, one launch that walks the T steps with h and c on chip.
    Backward: gn_lstm_bwd walks the steps down and writes dz (B, T, 4u); dW = X^T dz, dU = hprev^T dz and dX = dz W^T are one gn_bmm each over
    B T rows (the two weight gradients in up to 64 row parts summed in fixed order: rows_product) and db the bias-gradient reduction.  The tape
    keeps x, hprev (h shifted by one step: h_{t-1} beside dz_t), the activated gates and c, in the training phase only.  The planner fuses
    nothing onto the layer, and dy is not written."""

    def __init__(self, units, activation='tanh', recurrent_activation='hard_sigmoid', use_bias=True, kernel_initializer='glorot_uniform',
                 recurrent_initializer='orthogonal', bias_initializer='zeros', unit_forget_bias=True, kernel_regularizer=None,
                 recurrent_regularizer=None, bias_regularizer=None, activity_regularizer=None, return_sequences=False, go_backwards=False,
                 implementation=1, unroll=False, **kw):
        _init_recurrent(self, 'LSTM', kw, units, activation, recurrent_activation, use_bias, kernel_initializer, recurrent_initializer, bias_initializer,
                        kernel_regularizer, recurrent_regularizer, bias_regularizer, activity_regularizer, return_sequences, go_backwards,
                        implementation, unroll)
        self.unit_forget_bias = bool(unit_forget_bias)

    def build(self, input_shape):
        if len(input_shape) != 2:
            raise ValueError('%s (LSTM) expects (batch, timesteps, features), got %r' % (self.name, (None,) + tuple(input_shape)))
        Cin, u = int(input_shape[1]), self.units
        if u > 512:
            raise NotImplementedError('%s: LSTM(units=%d): at most 512 units run (a block carries all units of its samples on chip)' % (self.name, u))
        self.kernel, self.recurrent_kernel, self.bias = _add_triple(self, self, '', Cin)

    n_gates = 4

    def initial_bias(self):
        u = self.units
        bias = np.zeros(4 * u, np.float32)
        if self.unit_forget_bias:
            bias[u:2 * u] = 1.0
        return bias

    def compute_output_shape(self, input_shape):
        return (int(input_shape[0]), self.units) if self.return_sequences else (self.units,)

    def forward(self, ctx, node, x):
        x = x.contiguous()
        B, T, Cin = x.shape
        u = self.units
        zx = ops.bmm(x.view(1, B * T, Cin), self.kernel.data.view(1, Cin, 4 * u)).view(B, T, 4 * u)
        h, gates, c, hprev = ops.lstm_fwd(zx, self.recurrent_kernel.data, self.bias.data, None, None, self.activation, self.recurrent_activation,
                                          reverse=self.go_backwards, training=ctx.training)
        if ctx.training:
            ctx.tape[node.index] = (x, hprev, gates, c)
        return h if self.return_sequences else h[:, T - 1, :].contiguous()

    def backward(self, ctx, node, dy, need_dx, need_dw):
        x, hprev, gates, c = ctx.tape.pop(node.index)
        B, T, _ = x.shape
        u = self.units
        dz, _, _ = ops.lstm_bwd(dy.contiguous().view((B, T, u) if self.return_sequences else (B, u)), gates, c, self.recurrent_kernel.data, None,
                                self.activation, self.recurrent_activation, reverse=self.go_backwards)
        if need_dw:
            self.weight_grads(x, (hprev, gates, c), dz, None, self.kernel, self.recurrent_kernel, self.bias)
        return _input_grad(dz, self.kernel, x.shape) if need_dx else None

    def weight_grads(self, x, kept, dz, dzr, kernel, recurrent_kernel, bias):
        """the gradients of one direction's three weights from what its recurrence stored (kept = hprev, gates, c) and its backward wrote"""
        B, T, Cin = x.shape
        dz2 = dz.view(B * T, 4 * self.units)
        rows_product(x.view(B * T, Cin), dz2, kernel.grad)
        rows_product(kept[0].view(B * T, self.units), dz2, recurrent_kernel.grad)
        ops.bias_grad(dz2, bias.grad)


class SimpleRNN(Layer):
    """keras.layers.SimpleRNN(units): (B, T, Cin) -> (B, units), or (B, T, units) with return_sequences.  SimpleRNNCell of keras 2.2.4 with
    kernel (Cin, u), recurrent_kernel (u, u) and bias (u):
        h_t = act(x_t . W + b + h_{t-1} . U)
    with act one of tanh, sigmoid, relu, linear; h_0 = 0.  There is no recurrent activation, no implementation and no reset_after; go_backwards
    and unroll as in LSTM.
    Forward: zx = X . W as one gn_bmm over B T rows, then gn_rnn_fwd, one launch that walks the T steps with h on chip.
    Backward: gn_rnn_bwd walks the steps down and writes dz (B, T, u): dW = X^T dz, dU = hprev^T dz (rows_product), db = sum dz, dX = dz W^T.
    The tape keeps x, hprev and the stored h_t (a tensor of its own, not the layer's output), in the training phase only.  The planner fuses
    nothing onto the layer, and dy is not written."""

    def __init__(self, units, activation='tanh', use_bias=True, kernel_initializer='glorot_uniform', recurrent_initializer='orthogonal',
                 bias_initializer='zeros', kernel_regularizer=None, recurrent_regularizer=None, bias_regularizer=None, activity_regularizer=None,
                 return_sequences=False, go_backwards=False, unroll=False, **kw):
        for key in ('recurrent_activation', 'implementation', 'reset_after', 'unit_forget_bias'):
            if key in kw:
                raise TypeError('SimpleRNN(%s=...): keras.layers.SimpleRNN has no such argument' % key)
        _init_recurrent(self, 'SimpleRNN', kw, units, activation, _ABSENT, use_bias, kernel_initializer, recurrent_initializer, bias_initializer,
                        kernel_regularizer, recurrent_regularizer, bias_regularizer, activity_regularizer, return_sequences, go_backwards,
                        _ABSENT, unroll)

    def build(self, input_shape):
        if len(input_shape) != 2:
            raise ValueError('%s (SimpleRNN) expects (batch, timesteps, features), got %r' % (self.name, (None,) + tuple(input_shape)))
        Cin, u = int(input_shape[1]), self.units
        if u > 512:
            raise NotImplementedError('%s: SimpleRNN(units=%d): at most 512 units run (a block carries all units of its samples on chip)'
                                      % (self.name, u))
        self.kernel, self.recurrent_kernel, self.bias = _add_triple(self, self, '', Cin)

    n_gates = 1

    def initial_bias(self):
        return np.zeros(self.units, np.float32)

    def compute_output_shape(self, input_shape):
        return (int(input_shape[0]), self.units) if self.return_sequences else (self.units,)

    def forward(self, ctx, node, x):
        x = x.contiguous()
        B, T, Cin = x.shape
        u = self.units
        zx = ops.bmm(x.view(1, B * T, Cin), self.kernel.data.view(1, Cin, u)).view(B, T, u)
        h, hs, hprev = ops.rnn_fwd(zx, self.recurrent_kernel.data, self.bias.data, None, self.activation, reverse=self.go_backwards,
                                   training=ctx.training)
        if ctx.training:
            ctx.tape[node.index] = (x, hprev, hs)
        return h if self.return_sequences else h[:, T - 1, :].contiguous()

    def backward(self, ctx, node, dy, need_dx, need_dw):
        x, hprev, hs = ctx.tape.pop(node.index)
        B, T, _ = x.shape
        u = self.units
        dz, _ = ops.rnn_bwd(dy.contiguous().view((B, T, u) if self.return_sequences else (B, u)), hs, self.recurrent_kernel.data, self.activation,
                            reverse=self.go_backwards)
        if need_dw:
            self.weight_grads(x, (hprev, hs, None), dz, None, self.kernel, self.recurrent_kernel, self.bias)
        return _input_grad(dz, self.kernel, x.shape) if need_dx else None

    def weight_grads(self, x, kept, dz, dzr, kernel, recurrent_kernel, bias):
        """the gradients of one direction's three weights from what its recurrence stored (kept = hprev, hs, None) and its backward wrote"""
        B, T, Cin = x.shape
        dz2 = dz.view(B * T, self.units)
        rows_product(x.view(B * T, Cin), dz2, kernel.grad)
        rows_product(kept[0].view(B * T, self.units), dz2, recurrent_kernel.grad)
        ops.bias_grad(dz2, bias.grad)


_MERGE_PASS = {'sum': 'add', 'mul': 'mul', 'ave': 'avg'}          # merge_mode -> the mode of ops.merge_fwd


class Bidirectional(Layer):
    """keras.layers.Bidirectional(layer, merge_mode='concat') (keras 2.2.4 layers/wrappers.py) over an unbuilt LSTM, GRU or SimpleRNN of this module:
    (B, T, Cin) -> (B, [T,] 2u) for 'concat', (B, [T,] u) for 'sum', 'mul' and 'ave'.  The forward copy walks as the inner layer's go_backwards
    says, the backward copy the other way, and with return_sequences the backward copy's sequence is turned round (K.reverse along time)
    before the halves are merged.  Six weights in keras' order: <name>/forward_<inner>/{kernel, recurrent_kernel, bias}, then the same under
    backward_<inner>; each carries the inner layer's regularizer, and the forward triple is drawn first (what a lone inner layer draws).
    Forward: zx_d = X . W_d, two gn_bmm; then ONE pair launch (ops.lstm_pair_fwd / gru_pair_fwd / rnn_pair_fwd: the direction is the grid's second dimension)
    that writes both halves in time-aligned order -- for 'concat' straight into the (B, [T,] 2u) output, so no reverse and no concatenate pass
    exists; for the other modes into two buffers that ops.merge_fwd joins.
    Backward: 'concat' and 'sum' hand dy to the pair launch as it is (read through a row stride), 'ave' one ops.scale by 1/2 shared by both
    directions, 'mul' the two ops.merge_bwd; ONE pair launch; the weight gradients a direction as LSTM.backward / GRU.backward form them
    (weight_grads); dX = dz_f . W_f^T + dz_b . W_b^T, two gn_bmm and one add pass, forward term first.  Fixed order, no atomics.  The tape keeps
    x and both directions' stored tensors (and the two halves under 'mul'), in the training phase only.  The planner fuses nothing onto the
    layer, and dy is not written."""

    def __init__(self, layer, merge_mode='concat', **kw):
        if not isinstance(layer, (LSTM, GRU, SimpleRNN)):
            raise ValueError('Please initialize `Bidirectional` layer with an unbuilt `LSTM`, `GRU` or `SimpleRNN` instance. You passed: %r' % (layer,))
        if layer.built:
            raise ValueError('Bidirectional(layer=%s): the inner layer is already built; the wrapper owns both copies of its weights' % layer.name)
        if merge_mode is None:
            raise NotImplementedError('Bidirectional(merge_mode=None): the two halves as two outputs are not implemented (a layer has one output)')
        if merge_mode not in ('concat', 'sum', 'mul', 'ave'):
            raise ValueError('Invalid merge mode. Merge mode should be one of {"sum", "mul", "ave", "concat"}, got %r' % (merge_mode,))
        if kw.pop('weights', None) is not None:
            raise NotImplementedError('Bidirectional(weights=...): initial weights through the constructor are not implemented; use set_weights')
        if layer.activity_regularizer is not None:
            raise NotImplementedError('Bidirectional(layer=%s(activity_regularizer=...)): an activity regularizer on the inner layer is not '
                                      'implemented' % type(layer).__name__)
        Layer.__init__(self, **kw)
        self.layer, self.merge_mode = layer, merge_mode

    def build(self, input_shape):
        inner = self.layer
        if len(input_shape) != 2:
            raise ValueError('%s (Bidirectional) expects (batch, timesteps, features), got %r' % (self.name, (None,) + tuple(input_shape)))
        if inner.units > 512:
            raise NotImplementedError('%s: %s(units=%d): at most 512 units run (a block carries all units of its samples on chip)'
                                      % (self.name, type(inner).__name__, inner.units))
        Cin = int(input_shape[1])
        self.forward_weights = _add_triple(self, inner, 'forward_%s/' % inner.name, Cin)
        self.backward_weights = _add_triple(self, inner, 'backward_%s/' % inner.name, Cin)

    def compute_output_shape(self, input_shape):
        width = self.layer.units * (2 if self.merge_mode == 'concat' else 1)
        return (int(input_shape[0]), width) if self.layer.return_sequences else (width,)

    def forward(self, ctx, node, x):
        inner = self.layer
        x = x.contiguous()
        B, T, Cin = x.shape
        G = inner.n_gates * inner.units
        triples = (self.forward_weights, self.backward_weights)
        zx = [ops.bmm(x.view(1, B * T, Cin), W.data.view(1, Cin, G)).view(B, T, G) for W, _, _ in triples]
        U = [t[1].data for t in triples]
        kw = dict(activation=inner.activation, reverse0=inner.go_backwards, seq=inner.return_sequences, concat=self.merge_mode == 'concat',
                  training=ctx.training)
        if isinstance(inner, SimpleRNN):
            y, h, gates, hprev = ops.rnn_pair_fwd(zx, U, [t[2].data for t in triples], **kw)                      # gates: the stored h_t
            last = [None, None]
        elif isinstance(inner, LSTM):
            kw['recurrent_activation'] = inner.recurrent_activation
            y, h, gates, last, hprev = ops.lstm_pair_fwd(zx, U, [t[2].data for t in triples], **kw)                 # last: c
        else:
            kw['recurrent_activation'] = inner.recurrent_activation
            b2 = [t[2].data.view(-1, G) for t in triples]
            y, h, gates, hprev, last = ops.gru_pair_fwd(zx, U, [b[0] for b in b2], [b[1] for b in b2] if inner.reset_after else None,
                                                        reset_after=inner.reset_after, **kw)                      # last: aux
        if ctx.training:
            ctx.tape[node.index] = (x, hprev, gates, last, h if self.merge_mode == 'mul' else None)
        return y if self.merge_mode == 'concat' else ops.merge_fwd(_MERGE_PASS[self.merge_mode], h)

    def backward(self, ctx, node, dy, need_dx, need_dw):
        inner = self.layer
        x, hprev, gates, last, h = ctx.tape.pop(node.index)
        dy = dy.contiguous().view((x.shape[0],) + tuple(node.out_shape))
        if self.merge_mode == 'mul':
            dy = [ops.merge_bwd('mul', dy, h, d) for d in range(2)]
        elif self.merge_mode == 'ave':
            dy = [ops.scale(dy, 0.5)] * 2
        elif self.merge_mode == 'sum':
            dy = [dy, dy]
        triples = (self.forward_weights, self.backward_weights)
        U = [t[1].data for t in triples]
        kw = dict(activation=inner.activation, reverse0=inner.go_backwards, concat=self.merge_mode == 'concat')
        if isinstance(inner, SimpleRNN):
            dz, dzr = ops.rnn_pair_bwd(dy, gates, U, **kw), None
        elif isinstance(inner, LSTM):
            dz, dzr = ops.lstm_pair_bwd(dy, gates, last, U, recurrent_activation=inner.recurrent_activation, **kw), None
        else:
            dz, dzr = ops.gru_pair_bwd(dy, gates, hprev, last, U, recurrent_activation=inner.recurrent_activation, reset_after=inner.reset_after, **kw)
        if need_dw:
            for d, (W, Ud, b) in enumerate(triples):
                inner.weight_grads(x, (hprev[d], gates[d], last[d]), dz[d], dzr[d] if dzr else None, W, Ud, b)
        if not need_dx:
            return None
        return ops.merge_fwd('add', [_input_grad(dz[d], triples[d][0], x.shape) for d in range(2)])
