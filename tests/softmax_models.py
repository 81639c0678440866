"""The small graphs of the softmax tests, each with its torch fp64 restatement: tests/test_softmax_cpu.py asserts on how they are planned,
tests/test_softmax_gpu.py trains them against torch autograd.  A builder returns (model, ref); ref(P, x, training, masks, moving) is the
model's output in torch for the weights P = {layer name: [tensors in get_weights() order]}, `masks` the Dropout keep masks by layer name and
`moving` {layer name: (moving mean, moving variance)} for the inference phase of a BatchNormalization."""
import torch
import torch.nn.functional as F

DROP_RATE = 0.3


def conv1d(h, W, b, padding, dilation=1):
    """keras Conv1D, stride 1, kernel (k, Cin, Cout), channels last"""
    total = (W.shape[0] - 1) * dilation
    pl, pr = {'valid': (0, 0), 'same': (total // 2, total - total // 2), 'causal': (total, 0)}[padding]
    return F.conv1d(F.pad(h.permute(0, 2, 1), (pl, pr)), W.permute(2, 1, 0), dilation=dilation).permute(0, 2, 1) + b


def model_a():
    """conv -> tanh -> global average -> Dense(3, activation='softmax'): the classifier head"""
    from gennet_amd import layers as L
    from gennet_amd.engine import Sequential
    m = Sequential([L.Conv1D(8, 5, padding='same', input_shape=(32, 4), name='a_conv'), L.Activation('tanh', name='a_tanh'),
                    L.GlobalAveragePooling1D(name='a_gap'), L.Dense(3, activation='softmax', name='a_head')])

    def ref(P, x, training=True, masks=None, moving=None):
        h = torch.tanh(conv1d(x, P['a_conv'][0], P['a_conv'][1], 'same')).mean(1)
        return torch.softmax(h @ P['a_head'][0] + P['a_head'][1], -1)
    return m, ref


def model_b():
    """Dense -> Activation('softmax') -> Dropout -> Dense: an activation layer that no producer may absorb, a Dropout that runs on its own"""
    from gennet_amd import layers as L
    from gennet_amd.engine import Sequential
    m = Sequential([L.Dense(8, input_shape=(6,), name='b_in'), L.Activation('softmax', name='b_soft'), L.Dropout(DROP_RATE, name='b_drop'),
                    L.Dense(1, name='b_out')])

    def ref(P, x, training=True, masks=None, moving=None):
        h = torch.softmax(x @ P['b_in'][0] + P['b_in'][1], -1)
        if training:
            h = h * masks['b_drop'] / (1.0 - DROP_RATE)
        return h @ P['b_out'][0] + P['b_out'][1]
    return m, ref


def model_c():
    """Conv1D(activation='softmax') -> Conv1D: the consumer's fused data-gradient epilogue would fire"""
    from gennet_amd import layers as L
    from gennet_amd.engine import Sequential
    m = Sequential([L.Conv1D(8, 3, activation='softmax', input_shape=(16, 4), name='c_soft'), L.Conv1D(4, 3, name='c_out')])

    def ref(P, x, training=True, masks=None, moving=None):
        h = torch.softmax(conv1d(x, P['c_soft'][0], P['c_soft'][1], 'valid'), -1)
        return conv1d(h, P['c_out'][0], P['c_out'][1], 'valid')
    return m, ref


def model_d():
    """attention over time: Conv1D(8, 1) -> Softmax(axis=1) weights the conv's own input, inner = 8"""
    from gennet_amd import layers as L
    from gennet_amd.engine import Input, Model
    inp = Input((32, 8), name='d_in')
    w = L.Softmax(axis=1, name='d_soft')(L.Conv1D(8, 1, name='d_score')(inp))
    out = L.Dense(1, name='d_out')(L.GlobalAveragePooling1D(name='d_gap')(L.Multiply(name='d_mul')([w, inp])))
    m = Model(inputs=inp, outputs=out)

    def ref(P, x, training=True, masks=None, moving=None):
        w = torch.softmax(conv1d(x, P['d_score'][0], P['d_score'][1], 'valid'), 1)
        return (w * x).mean(1) @ P['d_out'][0] + P['d_out'][1]
    return m, ref


def model_e():
    """Conv2DTranspose(4, (1, 3), activation='softmax') on (1, 8, 4)"""
    from gennet_amd import layers as L
    from gennet_amd.engine import Sequential
    m = Sequential([L.Conv2DTranspose(4, (1, 3), activation='softmax', input_shape=(1, 8, 4), name='e_soft')])

    def ref(P, x, training=True, masks=None, moving=None):
        k, b = P['e_soft']                 # (1, kw, filters, Cin), 'valid', stride 1: y[b, h, v, f] = sum_j sum_c x[b, h, v - j, c] k[0, j, f, c]
        kw, W = k.shape[1], x.shape[2]
        xp = F.pad(x, (0, 0, kw - 1, kw - 1))
        return torch.softmax(sum(xp[:, :, kw - 1 - j:kw - 1 - j + W + kw - 1, :] @ k[0, j].T for j in range(kw)) + b, -1)
    return m, ref


def model_f():
    """a causal dilated Conv1D with activation='softmax': the softmax runs on the merged phases"""
    from gennet_amd import layers as L
    from gennet_amd.engine import Sequential
    m = Sequential([L.Conv1D(8, 2, dilation_rate=2, padding='causal', activation='softmax', input_shape=(16, 4), name='f_soft')])

    def ref(P, x, training=True, masks=None, moving=None):
        return torch.softmax(conv1d(x, P['f_soft'][0], P['f_soft'][1], 'causal', 2), -1)
    return m, ref


def model_g():
    """Conv1D(activation='softmax') -> BatchNormalization: the inference fold and the conv-epilogue statistics would fire"""
    from gennet_amd import layers as L
    from gennet_amd.engine import Sequential
    m = Sequential([L.Conv1D(8, 5, padding='same', activation='softmax', input_shape=(32, 4), name='g_soft'), L.BatchNormalization(name='g_bn')])

    def ref(P, x, training=True, masks=None, moving=None):
        h = torch.softmax(conv1d(x, P['g_soft'][0], P['g_soft'][1], 'same'), -1)
        mean, var = (h.mean((0, 1)), h.var((0, 1), unbiased=False)) if training else moving['g_bn']
        return (h - mean) / torch.sqrt(var + 1e-3) * P['g_bn'][0] + P['g_bn'][1]
    return m, ref


def model_h():
    """seven taps: the tap-folded launch"""
    from gennet_amd import layers as L
    from gennet_amd.engine import Sequential
    m = Sequential([L.Conv1D(8, 7, padding='same', activation='softmax', input_shape=(16, 4), name='h_soft')])

    def ref(P, x, training=True, masks=None, moving=None):
        return torch.softmax(conv1d(x, P['h_soft'][0], P['h_soft'][1], 'same'), -1)
    return m, ref


def model_i():
    """UpSampling1D folded into the conv: the launch writes (L, 2 * filters) rows, the softmax runs over the layer's (2L, filters) rows"""
    from gennet_amd import layers as L
    from gennet_amd.engine import Sequential
    m = Sequential([L.Conv1D(4, 1, input_shape=(8, 4), name='i_in'), L.UpSampling1D(2, name='i_up'),      # (the fold needs a node in front of the upsample)
                    L.Conv1D(8, 5, padding='same', activation='softmax', name='i_soft')])

    def ref(P, x, training=True, masks=None, moving=None):
        h = conv1d(x, P['i_in'][0], P['i_in'][1], 'valid').repeat_interleave(2, dim=1)
        return torch.softmax(conv1d(h, P['i_soft'][0], P['i_soft'][1], 'same'), -1)
    return m, ref


def model_j():
    """5 -> 3 channels: the any-channel kernels"""
    from gennet_amd import layers as L
    from gennet_amd.engine import Sequential
    m = Sequential([L.Conv1D(3, 3, activation='softmax', input_shape=(16, 5), name='j_soft')])

    def ref(P, x, training=True, masks=None, moving=None):
        return torch.softmax(conv1d(x, P['j_soft'][0], P['j_soft'][1], 'valid'), -1)
    return m, ref


def model_k():
    """the width-2 Conv2D, strides (2, 1), 'same': the launch writes (w, c)-interleaved rows of 2 * filters floats"""
    from gennet_amd import layers as L
    from gennet_amd.engine import Sequential
    m = Sequential([L.Conv2D(4, (5, 5), strides=(2, 1), padding='same', activation='softmax', input_shape=(8, 2, 4), name='k_soft')])

    def ref(P, x, training=True, masks=None, moving=None):
        k, b = P['k_soft']                 # (kh, kw, Cin, Cout); H = 8, stride 2: pads (1, 2); W = 2, stride 1: pads (2, 2)
        h = F.conv2d(F.pad(x.permute(0, 3, 1, 2), (2, 2, 1, 2)), k.permute(3, 2, 0, 1), stride=(2, 1)).permute(0, 2, 3, 1) + b
        return torch.softmax(h, -1)
    return m, ref


MODELS = {'a': model_a, 'b': model_b, 'c': model_c, 'd': model_d, 'e': model_e, 'f': model_f, 'g': model_g,
          'h': model_h, 'i': model_i, 'j': model_j, 'k': model_k}          # h .. k: the other conv forms the layers launch
PLANNED = ('a', 'b', 'c', 'd', 'g')        # the graphs the planner test asserts on; (e) and (f) never take part in a fusion by construction
