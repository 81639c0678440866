"""A seeded generator of small valid layer graphs for the differential test against tests/model_ref.py.

generate(seed) -> spec, a plain printable dict; build(spec) -> the model, its weights seeded.  np.random.RandomState(seed) is the only source of
randomness.  A graph is a trunk of motifs over (L, C) sequences, (H, W, C) images and flat vectors with the legal transitions between them,
optionally a branch-and-merge (two or three branches; the same tensor on two edges; a tensor that feeds both a layer and the merge), a second
output and a nested frozen or trainable sub-model.  B in 3..6, L <= 48, about 12 nodes at most; channel counts from CHANNELS, with (8 -> 64)-type
5-tap pairs often enough that the transform-domain conv kernels are reached.

spec = {'seed', 'B', 'input': shape, 'ops': [op], 'outputs': [tensor id], 'losses': [kind], 'loss_weights': [w] | None, 'notes': [...]}
op   = {'id', 'cls', 'kw', 'in': [tensor ids]}; tensor 0 is the input; a nested model is {'id', 'cls': 'Model', 'name', 'in_shape', 'ops', 'out',
        'trainable', 'in'}, its own tensor 0 its input.  A keyword ending in _regularizer holds [l1, l2].
notes = [[layer name, planner field, 'take' | reason it is declined]]: what the motif that emitted the layers was built to make the planner do,
        checked against Model._plan by tests/test_graph_gen_cpu.py (the generator never reads a planner field).

admit(spec) says whether the fp64 interpreter alone finds the graph well posed (the kink margins and the conditioning); tests/graph_corpus.py
lists the admitted seeds the tests run."""
import numpy as np

CHANNELS = (1, 2, 3, 4, 5, 6, 8, 12, 16, 17, 20, 24)
MARGIN = 1e-5              # ten fp32 roundings: the distance every non-smooth decision keeps from flipping
LR = 0.05
BARS = {'output': 1e-5, 'loss': 1e-6, 'grad': 1e-4, 'weight': 1e-4, 'moving': 1e-4}      # the bars of tests/test_conv_anyc_gpu.py
CAP = 10.0                 # a bound is max(bar, 8 e32), and at most CAP * bar
SMOOTH = ('tanh', 'sigmoid')
KINKED = ('relu', 'leaky', 'relu_max')


class _Gen(object):
    def __init__(self, seed):
        self.rng = np.random.RandomState(seed)
        self.seed = seed
        self.ops, self.notes, self.next_id, self.prefix = [], [], 1, ''
        self.shape = {}            # tensor id -> shape without the batch axis
        self.second = None         # a tensor that became the second output
        self.extra_flat = None     # ... or a flat tensor off the trunk that did

    # ---- draws
    def pick(self, seq):
        return seq[self.rng.randint(len(seq))]

    def chance(self, p):
        return self.rng.rand() < p

    def slot_free(self):
        """the one second output is still to be had (and this is no sub-model: a nested model has one output)"""
        return self.second is None and self.extra_flat is None and not self.prefix

    # ---- emission
    def add(self, cls, ins, shape, **kw):
        i = self.next_id
        self.next_id += 1
        kw['name'] = '%s%s_%d' % (self.prefix, cls.lower(), i)
        self.ops.append({'id': i, 'cls': cls, 'kw': kw, 'in': list(ins)})
        self.shape[i] = tuple(shape)
        return i

    def name(self, t):
        return [o for o in self.ops if o['id'] == t][0]['kw']['name']

    def note(self, t, field, verdict):
        self.notes.append([self.name(t), field, verdict])

    # ---- element-wise followers
    def activation(self, t, kind=None):
        kind = kind or self.pick(SMOOTH + KINKED)
        if kind == 'leaky':
            return self.add('LeakyReLU', [t], self.shape[t], alpha=0.2)
        if kind == 'relu_max':
            return self.add('ReLU', [t], self.shape[t], max_value=1.0)
        return self.add('Activation', [t], self.shape[t], activation=kind)

    def dropout(self, t):
        return self.add('Dropout', [t], self.shape[t], rate=self.pick((0.25, 0.4)))

    def reg(self):
        return self.pick(([0.01, 0.0], [0.0, 0.02], [0.005, 0.01]))

    # ---- Conv1D
    def conv1d(self, t, filters, k, stride=1, padding='same', dilation=1, activation=None, **kw):
        L, C = self.shape[t]
        tot = (k - 1) * dilation
        Lout = (L - tot - 1) // stride + 1 if padding == 'valid' else -(-L // stride)
        assert Lout >= 1
        if activation is not None:
            kw['activation'] = activation
        if dilation != 1:
            kw['dilation_rate'] = dilation
        if self.chance(0.15):
            kw['kernel_regularizer'] = self.reg()
        return self.add('Conv1D', [t], (Lout, filters), filters=filters, kernel_size=k, strides=stride, padding=padding, **kw)

    def fit_k(self, t, k, padding, dilation=1):
        while padding == 'valid' and (k - 1) * dilation + 1 > self.shape[t][0]:
            k -= 1
        return max(k, 1)

    def ragged(self, a, b):
        """a channel pair the strict conv entry points refuse in one of the three directions (csrc/capi.hip needs_any, for both orders)"""
        def strict(ci, co):
            return co % 4 == 0 if ci <= 4 else ci % 4 == 0 if co <= 4 else (ci % 4 == 0 and co % 4 == 0)
        return not (strict(a, b) and strict(b, a))

    def motif_conv(self, t, obstacle=None):
        """Conv1D -> activation -> Dropout, with one thing in the way of the planner's epilogue fusions (or nothing)."""
        L, C = self.shape[t]
        obstacle = obstacle or self.pick(('none', 'none', 'none', 'second consumer', 'model output', 'activity regularizer', 'own activation', 'softmax',
                                          'any_channels pair', 'phased conv', 'wide', 'small filter count'))
        if obstacle == 'model output' and not self.slot_free():
            obstacle = 'none'
        k = self.pick((1, 2, 3, 5, 5, 7, 16))
        padding, stride, dilation, act, kw = self.pick(('same', 'same', 'valid')), self.pick((1, 1, 2)), 1, None, {}
        f = self.pick([c for c in (8, 12, 16, 20, 24) if not self.ragged(C, c)] or [8])
        if obstacle == 'any_channels pair':
            f = self.pick([c for c in CHANNELS if self.ragged(C, c) and c > 4] or [5])
        if obstacle == 'wide':         # an (8 -> 64)-type 5-tap pair, then 64 -> 64: the transform-domain kernels under the default conv math
            t = self.conv1d(t, 64, 5, 1, 'same')
            C, f, k, padding = 64, 64, 5, 'same'
        if obstacle == 'small filter count':      # <= 4 filters over an aligned pair: the small-Cout kernels, which have no Dropout epilogue
            if not [c for c in (1, 2, 3, 4) if not self.ragged(C, c)]:
                t = self.conv1d(t, 8, 3, 1, 'same')
                C = 8
            f = self.pick([c for c in (1, 2, 3, 4) if not self.ragged(C, c)])
            k = min(k, 5)
        if obstacle == 'phased conv':
            padding, dilation, stride = self.pick(('causal', 'same', 'causal')), self.pick((1, 2, 3)), 1
            if padding == 'same' and dilation == 1:
                dilation = 2
            k = min(k, 5)
        if obstacle == 'own activation':
            act = self.pick(('relu', 'tanh', 'sigmoid'))
        if obstacle == 'softmax':
            act = 'softmax'
        if obstacle == 'activity regularizer':
            kw['activity_regularizer'] = self.reg()
        k = self.fit_k(t, k, padding, dilation)
        c = self.conv1d(t, f, k, stride, padding, dilation, act, **kw)
        ragged = self.ragged(C * (-(-k // 5) if k > 5 else 1), f)
        a = self.activation(c)
        d = self.dropout(a)
        out = d
        if obstacle == 'second consumer':
            where = self.pick(('conv', 'act'))
            out = self.add(self.pick(('Add', 'Multiply', 'Average', 'Subtract')), [d, c if where == 'conv' else a], self.shape[d])
            self.note(c, 'fused_act', 'second consumer' if where == 'conv' else 'take')
            self.note(c, 'fused_drop', 'second consumer')
            return out
        if obstacle == 'model output':
            self.second = c
            self.note(c, 'fused_act', 'model output')
            self.note(c, 'fused_drop', 'model output')
            return out
        if obstacle in ('activity regularizer', 'own activation', 'softmax'):
            if obstacle == 'activity regularizer' and self.chance(0.5):      # ... whose output also feeds a merge: the penalty's gradient term on a summed gradient
                out = self.add(self.pick(('Add', 'Average', 'Multiply')), [d, c], self.shape[d])
            self.note(c, 'fused_act', obstacle)
            self.note(c, 'fused_drop', 'softmax' if obstacle == 'softmax' else 'activity regularizer' if obstacle == 'activity regularizer' else 'own activation')
            return out
        self.note(c, 'fused_act', 'take')
        if obstacle == 'phased conv':
            self.note(c, 'fused_drop', 'phased conv')
        elif ragged:
            self.note(c, 'fused_drop', 'any_channels pair')
        elif f <= 4:
            self.note(c, 'fused_drop', 'small filter count')
        else:
            self.note(c, 'fused_drop', 'take')
        return out

    def motif_conv_bn(self, t, obstacle=None):
        """linear Conv1D -> BatchNormalization -> activation -> Dropout: the inference fold, the epilogue statistics, BN's own epilogue"""
        L, C = self.shape[t]
        obstacle = obstacle or self.pick(('none', 'none', 'none', 'second consumer', 'model output', 'activity regularizer', 'own activation', 'softmax',
                                          'any_channels pair', 'phased conv', 'non-last-axis BatchNormalization'))
        if obstacle == 'model output' and not self.slot_free():
            obstacle = 'none'
        k, padding, stride, dilation, act, kw = self.pick((3, 5, 5, 8)), self.pick(('same', 'valid')), self.pick((1, 1, 2)), 1, None, {}
        f = self.pick((8, 12, 16, 24, 64))
        if obstacle == 'any_channels pair':
            f = self.pick((5, 6, 17))
        if obstacle == 'phased conv':
            padding, dilation, stride, k = 'causal', self.pick((1, 2)), 1, 3
        if obstacle in ('own activation', 'softmax'):
            act = 'softmax' if obstacle == 'softmax' else self.pick(('tanh', 'relu'))
        if obstacle == 'activity regularizer':
            kw['activity_regularizer'] = self.reg()
        k = self.fit_k(t, k, padding, dilation)
        c = self.conv1d(t, f, k, stride, padding, dilation, act, **kw)
        axis = self.pick((1, 1, -2)) if obstacle == 'non-last-axis BatchNormalization' else self.pick((-1, 2))
        bkw = {'moving_average': 'ema'} if self.chance(0.3) else {}
        if self.chance(0.2):
            bkw['gamma_regularizer'] = self.reg()
        b = self.add('BatchNormalization', [c], self.shape[c], axis=axis, **bkw)
        a = self.activation(b)
        d = self.dropout(a)
        out = d
        if obstacle == 'second consumer':
            out = self.add(self.pick(('Add', 'Maximum', 'Minimum')), [d, c], self.shape[d])
        if obstacle == 'model output':
            self.second = c
        self.note(c, 'infer_bn', 'take' if obstacle == 'none' else obstacle)
        last = obstacle != 'non-last-axis BatchNormalization'
        self.note(b, 'fused_act', 'take' if last else obstacle)
        self.note(b, 'fused_drop', 'take' if last else obstacle)
        return out

    def motif_upsample(self, t, placement=None):
        """UpSampling1D in front of a conv that folds it, or of one that cannot; with two consumers; as a model output"""
        L, C = self.shape[t]
        placement = placement or self.pick(('fold', 'fold', 'fold', 'consumer cannot fold', 'second consumer', 'model output', 'activity regularizer',
                                            'phased conv'))
        if placement == 'model output' and not self.slot_free():
            placement = 'consumer cannot fold'
        if t == 0:                     # the planner folds no graph input: a layer in front
            t = self.conv1d(0, self.pick((3, 5, 8)), 3, 1, 'same')
            L, C = self.shape[t]
        u = self.add('UpSampling1D', [t], (2 * L, C), size=2)
        f = self.pick((6, 8, 5, 16, 3))
        kw = {}
        if placement == 'consumer cannot fold':
            k, padding = self.pick(((3, 'same'), (3, 'valid'), (5, 'valid'), (2, 'same')))
            c = self.conv1d(u, f, k, 1, padding)
        elif placement == 'phased conv':
            c = self.conv1d(u, f, 5, 1, 'same', 2)
        else:
            if placement == 'activity regularizer':
                kw['activity_regularizer'] = self.reg()
            c = self.conv1d(u, f, 5, self.pick((1, 1, 2)), 'same', **kw)
        out = c
        if placement == 'second consumer':
            c2 = self.conv1d(u, f, 5, self.ops[-1]['kw']['strides'], 'same')
            out = self.add(self.pick(('Add', 'Subtract', 'Maximum')), [c, c2], self.shape[c])
            self.note(c2, 'fold_up', 'second consumer')
        if placement == 'model output':
            self.second = u
        self.note(c, 'fold_up', 'take' if placement == 'fold' else placement)
        return out

    def motif_fuse_prev(self, t, obstacle=None):
        """producer with an activation (and a Dropout) -> a conv that can take the producer's derivative into its data gradient"""
        L, C = self.shape[t]
        obstacle = obstacle or self.pick(('none', 'none', 'none', 'second consumer', 'model output', 'activity regularizer', 'softmax', 'phased conv'))
        if obstacle == 'model output' and not self.slot_free():
            obstacle = 'none'
        f1, f2 = self.pick((8, 16, 12)), self.pick((8, 16, 32))
        if self.ragged(C, f1):
            f1 = 8 if not self.ragged(C, 8) else f1
        kw = {'activity_regularizer': self.reg()} if obstacle == 'activity regularizer' else {}
        act = 'softmax' if obstacle == 'softmax' else self.pick((None, 'tanh', 'relu'))
        p = self.conv1d(t, f1, self.fit_k(t, self.pick((3, 5)), 'same'), self.pick((1, 2)), 'same', 1, act, **kw)
        h = p
        if act is None:
            h = self.activation(h)
        if self.chance(0.5) and obstacle != 'softmax' and not self.ragged(C, f1):      # (a ragged pair's Dropout is a pass of its own: not shape-only)
            h = self.dropout(h)
        if obstacle == 'phased conv':
            c = self.conv1d(h, f2, 3, 1, 'causal', self.pick((1, 2)))
        else:
            c = self.conv1d(h, f2, self.fit_k(h, self.pick((3, 5, 5)), 'same'), self.pick((1, 2)), 'same')
        out = c
        if obstacle == 'second consumer':
            c2 = self.conv1d(h, f2, 1, self.ops[-1]['kw']['strides'], 'same')
            out = self.add('Concatenate', [c, c2], self.shape[c][:1] + (2 * f2,), axis=-1)
            self.note(c2, 'fuse_prev', 'second consumer')
        if obstacle == 'model output':
            self.second = h
        self.note(c, 'fuse_prev', 'take' if obstacle == 'none' else obstacle)
        return out

    def motif_lazy(self, t, obstacle=None):
        """BatchNormalization -> activation -> a 1-filter Conv1D whose data gradient the BatchNormalization's backward forms"""
        L, C = self.shape[t]
        obstacle = obstacle or self.pick(('none', 'none', 'none', 'second consumer', 'model output', 'any_channels pair', 'phased conv',
                                          'non-last-axis BatchNormalization'))
        if obstacle == 'model output' and not self.slot_free():
            obstacle = 'none'
        if obstacle == 'second consumer' and not self.slot_free():
            obstacle = 'none'
        f = self.pick((5, 6, 17)) if obstacle == 'any_channels pair' else self.pick((8, 16, 24))
        p = self.conv1d(t, f, self.fit_k(t, 3, 'same'), 1, 'same')
        b = self.add('BatchNormalization', [p], self.shape[p], axis=1 if obstacle == 'non-last-axis BatchNormalization' else -1)
        h = self.activation(b, self.pick(('tanh', 'leaky', 'relu')))
        if obstacle == 'phased conv':
            c = self.conv1d(h, 1, 3, 1, 'causal')
        else:
            c = self.conv1d(h, 1, self.pick((1, 3, 5)), 1, self.pick(('same', 'valid')) if self.shape[h][0] >= 5 else 'same')
        out = c
        if obstacle == 'second consumer':
            g = self.add('GlobalAveragePooling1D', [h], (f,))
            self.extra_flat = g
        if obstacle == 'model output':
            self.second = h
        self.note(c, 'lazy_bn', 'take' if obstacle == 'none' else obstacle)
        return out

    def motif_misc_seq(self, t):
        L, C = self.shape[t]
        what = self.pick(('pool', 'pool', 'prelu', 'softmax', 'areg', 'branches', 'branches', 'branches'))
        if what == 'pool' and L >= 4:
            cls = self.pick(('MaxPooling1D', 'AveragePooling1D'))
            p, s, padding = self.pick((2, 3)), self.pick((None, 1, 2)), self.pick(('valid', 'same'))
            st = s or p
            Lout = (L - p) // st + 1 if padding == 'valid' else -(-L // st)
            return self.add(cls, [t], (Lout, C), pool_size=p, strides=s, padding=padding)
        if what == 'prelu' and (L * C) % 4 == 0:
            kw = {'alpha_regularizer': self.reg()} if self.chance(0.3) else {}
            return self.add('PReLU', [t], (L, C), **kw)
        if what == 'softmax':
            return self.add('Softmax', [t], (L, C), axis=self.pick((1, 2, -1)))
        if what == 'areg':
            r = self.reg()
            return self.add('ActivityRegularization', [t], (L, C), l1=r[0], l2=r[1])
        return self.branches(t)

    def branches(self, t):
        """two or three branches off one tensor, joined again: a branch is a shape-keeping layer, the tensor itself, or the same branch twice"""
        shp = self.shape[t]
        n = self.pick((2, 2, 3))
        outs = []
        for j in range(n):
            kind = self.pick(('layer', 'layer', 'self', 'twice'))
            if kind == 'self':
                outs.append(t)
            elif kind == 'twice' and outs:
                outs.append(outs[-1])
            elif len(shp) == 2:
                how = self.pick(('conv', 'conv_act', 'act', 'bn'))
                if how == 'act':
                    outs.append(self.activation(t, self.pick(SMOOTH)))
                elif how == 'bn':
                    outs.append(self.add('BatchNormalization', [t], shp, axis=self.pick((-1, 1))))
                else:
                    act = self.pick(('tanh', 'relu', 'sigmoid')) if how == 'conv_act' else None
                    f = shp[1]
                    outs.append(self.conv1d(t, f, self.fit_k(t, self.pick((1, 3, 5)), 'same'), 1, self.pick(('same', 'causal')), 1, act))
            elif len(shp) == 1:
                outs.append(self.add('Dense', [t], shp, units=shp[0], activation=self.pick((None, 'tanh', 'relu'))))
            else:
                outs.append(self.activation(t, self.pick(SMOOTH)))
        cls = self.pick(('Add', 'Subtract', 'Multiply', 'Average', 'Maximum', 'Minimum', 'Concatenate', 'Concatenate'))
        if cls == 'Subtract':
            outs = outs[:2]
        if cls in ('Maximum', 'Minimum'):      # the same tensor twice would be a tie in every element
            uniq = []
            for o in outs:
                if o not in uniq:
                    uniq.append(o)
            outs = uniq if len(uniq) >= 2 else uniq + [self.activation(t, 'tanh')]
        if cls == 'Concatenate':
            axis = self.pick((-1,) + tuple(range(1, len(shp) + 1)))
            ax = axis % (len(shp) + 1) - 1
            out = tuple(sum(self.shape[o][d] for o in outs) if d == ax else shp[d] for d in range(len(shp)))
            return self.add(cls, outs, out, axis=axis)
        return self.add(cls, outs, shp)

    # ---- images
    def motif_img(self, t):
        H, W, C = self.shape[t]
        what = self.pick(('conv2d', 'conv2d', 'convT', 'convT', 'pool', 'bn', 'branches'))
        if what == 'conv2d' and W == 2:
            f = self.pick([c for c in (2, 4, 6, 8, 12, 16) if not self.ragged(2 * C, 2 * c)] or [0])
            if f:
                sh = self.pick((1, 2))
                act = self.pick((None, None, 'tanh', 'relu', 'softmax'))
                kw = {'activation': act} if act else {}
                c = self.add('Conv2D', [t], (-(-H // sh), 2, f), filters=f, kernel_size=[self.pick((1, 3, 5)), 5], strides=[sh, 1], padding='same', **kw)
                if act is None:
                    c = self.activation(c)
                return self.dropout(c) if self.chance(0.6) else c
        if what == 'convT':
            def ok(k, f):
                a, b = f * (-(-k // 5) if k > 5 else 1), C
                return (a % 4 == 0 and b % 4 == 0) or (a <= 4 and b % 4 == 0) or (b <= 4 and a % 4 == 0)
            k, s = self.pick((2, 3, 4, 7)), self.pick((1, 2))
            fs = [f for f in (1, 2, 3, 4, 8, 12, 16) if ok(k, f)]
            if fs and W * s + k <= 48:
                f, padding = self.pick(fs), self.pick(('valid', 'same'))
                Wout = W * s + max(k - s, 0) if padding == 'valid' else W * s
                act = self.pick((None, None, 'tanh', 'softmax'))
                kw = {'activation': act} if act else {}
                c = self.add('Conv2DTranspose', [t], (H, Wout, f), filters=f, kernel_size=[1, k], strides=[1, s], padding=padding, **kw)
                if act is None:
                    c = self.activation(c)
                return self.dropout(c) if self.chance(0.6) else c
        if what == 'pool' and H >= 2:
            cls = self.pick(('MaxPooling2D', 'AveragePooling2D'))
            pool = [2, 1] if self.chance(0.4) else [self.pick((2, 3)) if H >= 3 else 2, self.pick((1, 2)) if W >= 2 else 1]
            padding = self.pick(('valid', 'same'))
            strides = None if self.chance(0.6) else [self.pick((1, 2)), 1]
            st = strides or pool
            out = tuple((n - p) // s + 1 if padding == 'valid' else -(-n // s) for n, p, s in zip((H, W), pool, st))
            return self.add(cls, [t], out + (C,), pool_size=pool, strides=strides, padding=padding)
        if what == 'branches':
            return self.branches(t)
        return self.add('BatchNormalization', [t], (H, W, C), axis=self.pick((-1, 1, 2, 3)))

    def motif_flat(self, t):
        F = self.shape[t][0]
        what = self.pick(('dense', 'dense', 'dense_drop', 'branches', 'prelu', 'bn'))
        if what == 'branches':
            return self.branches(t)
        if what == 'prelu' and F % 4 == 0:
            return self.add('PReLU', [t], (F,))
        if what == 'bn':
            return self.add('BatchNormalization', [t], (F,), axis=-1)
        u = self.pick((3, 5, 8, 12, 16, 17))
        act = self.pick((None, 'tanh', 'relu', 'sigmoid'))
        kw = {'activation': act} if act else {}
        if self.chance(0.2):
            kw['bias_regularizer'] = self.reg()
        if self.chance(0.15):
            kw['activity_regularizer'] = self.reg()
        d = self.add('Dense', [t], (u,), units=u, **kw)
        if act is None and self.chance(0.7):
            d = self.activation(d)
        return self.dropout(d) if what == 'dense_drop' else d

    # ---- transitions
    def to_flat(self, t):
        shp = self.shape[t]
        if len(shp) == 1:
            return t
        n = int(np.prod(shp))
        if len(shp) == 2:
            cls = self.pick(('Flatten', 'GlobalAveragePooling1D', 'GlobalMaxPooling1D')) if n <= 512 else self.pick(('GlobalAveragePooling1D', 'GlobalMaxPooling1D'))
        else:
            cls = self.pick(('Flatten', 'GlobalAveragePooling2D', 'GlobalMaxPooling2D')) if n <= 512 else self.pick(('GlobalAveragePooling2D', 'GlobalMaxPooling2D'))
        if cls.startswith('GlobalMax') and int(np.prod(shp[:-1])) < 2:
            cls = 'Flatten'
        return self.add(cls, [t], (n,) if cls == 'Flatten' else (shp[-1],))

    def to_seq(self, t):
        shp = self.shape[t]
        if len(shp) == 2:
            return t
        if len(shp) == 3:
            return self.add('Reshape', [t], (shp[0], shp[1] * shp[2]), target_shape=[shp[0], shp[1] * shp[2]])
        L, C = self.pick((8, 12, 16)), self.pick((2, 3, 4, 8))
        d = self.add('Dense', [t], (L * C,), units=L * C, activation=self.pick((None, 'tanh')))
        return self.add('Reshape', [d], (L, C), target_shape=[-1, C])

    def to_img(self, t):
        shp = self.shape[t]
        if len(shp) == 3:
            return t
        t = self.to_seq(t)
        L, C = self.shape[t]
        if C == 1 and self.chance(0.8):
            const = np.round(self.rng.randn(L), 3).tolist()
            return self.add('MyLayer', [t], (L, 2, 1), const=const)
        if C % 2 == 0:
            return self.add('Reshape', [t], (L, 2, C // 2), target_shape=[L, 2, C // 2])
        return self.add('Reshape', [t], (L, 1, C), target_shape=[L, 1, C])

    # ---- one trunk
    def trunk(self, t, steps):
        for _ in range(steps):
            if len(self.ops) >= 11:
                break
            shp = self.shape[t]
            if len(shp) == 2:
                if shp[0] < 3:
                    t = self.to_flat(t)
                    continue
                m = self.pick(('conv', 'conv', 'conv_bn', 'conv_bn', 'upsample', 'upsample', 'fuse_prev', 'fuse_prev', 'lazy', 'misc', 'misc', 'img', 'flat'))
                if m == 'upsample' and shp[0] > 24:
                    m = 'conv'
                t = {'conv': self.motif_conv, 'conv_bn': self.motif_conv_bn, 'upsample': self.motif_upsample, 'fuse_prev': self.motif_fuse_prev,
                     'lazy': self.motif_lazy, 'misc': self.motif_misc_seq, 'img': self.to_img, 'flat': self.to_flat}[m](t)
            elif len(shp) == 3:
                m = self.pick(('img', 'img', 'img', 'seq', 'flat'))
                t = {'img': self.motif_img, 'seq': self.to_seq, 'flat': self.to_flat}[m](t)
            else:
                m = self.pick(('flat', 'flat', 'seq'))
                t = {'flat': self.motif_flat, 'seq': self.to_seq}[m](t)
        return t

    def nested(self, t):
        """a sub-model over the current tensor, frozen or trainable, spliced in as one layer"""
        outer = (self.ops, self.shape, self.next_id, self.prefix)
        i = self.next_id
        self.ops, self.shape, self.next_id, self.prefix = [], {0: self.shape[t]}, 1, 'm%d_' % i
        o = self.trunk(0, self.pick((1, 2)))
        if o == 0:
            o = self.activation(0, 'tanh')
        inner_ops, inner_shape = self.ops, self.shape
        self.ops, self.shape, self.next_id, self.prefix = outer
        self.next_id = i + 1
        self.ops.append({'id': i, 'cls': 'Model', 'name': 'sub_%d' % i, 'in_shape': list(inner_shape[0]), 'ops': inner_ops, 'out': o,
                         'trainable': bool(self.chance(0.5)), 'in': [t]})
        self.shape[i] = inner_shape[o]
        return i


def _head(g, t):
    """-> (output tensor, loss): a small Dense head on flat tensors (absorbs a producer's derivative when it has <= 4 units), or the tensor itself"""
    shp = g.shape[t]
    if len(shp) != 1 and g.chance(0.35) and int(np.prod(shp)) <= 256:
        return t, g.pick(('mean_squared_error', 'logcosh'))
    t = g.to_flat(t)
    u = g.pick((1, 2, 3, 4, 4, 6))
    head = g.pick(('linear', 'sigmoid', 'softmax')) if u > 1 else g.pick(('linear', 'sigmoid'))
    kw = {} if head == 'linear' else {'activation': head}
    d = g.add('Dense', [t], (u,), units=u, **kw)
    return d, {'linear': g.pick(('mean_squared_error', 'logcosh')), 'sigmoid': 'binary_crossentropy', 'softmax': 'categorical_crossentropy'}[head]


def generate(seed):
    g = _Gen(seed)
    B = int(g.rng.randint(3, 7))
    kind = g.pick(('seq', 'seq', 'seq', 'seq', 'seq', 'img', 'flat', 'mylayer'))
    if kind == 'mylayer':
        shape = (int(g.pick((8, 12, 16, 24))), 1)
    elif kind == 'seq':
        shape = (int(g.pick((8, 12, 16, 20, 24, 32, 48))), int(g.pick(CHANNELS[:9])))
    elif kind == 'img':
        shape = (int(g.pick((6, 8, 12, 16))), 2, int(g.pick((1, 2, 4))))
    else:
        shape = (int(g.pick((5, 8, 12, 20))),)
    g.shape[0] = shape
    t = 0
    if kind == 'mylayer':              # the measured data h(t) as the layer's constant: stack([x, h - x]) is a width-2 image
        t = g.add('MyLayer', [0], (shape[0], 2, 1), const=np.round(g.rng.randn(shape[0]), 3).tolist())
    t = g.trunk(t, g.pick((1, 2, 2, 3)))
    if g.chance(0.3) and len(g.ops) <= 8:
        t = g.nested(t)
    if t == 0:
        t = g.trunk(0, 1) if len(shape) != 1 else g.motif_flat(0)
    out, loss = _head(g, t)
    outputs, losses = [out], [loss]
    if g.second is not None:
        outputs.append(g.second)
        losses.append('mean_squared_error')
    elif g.extra_flat is not None:
        outputs.append(g.extra_flat)
        losses.append('mean_squared_error')
    weights = [1.0, float(g.pick((0.5, 2.0)))] if len(outputs) == 2 else None
    return {'seed': seed, 'B': B, 'input': list(shape), 'ops': g.ops, 'outputs': outputs, 'losses': losses, 'loss_weights': weights, 'notes': g.notes}


# ---- the model of a spec ----------------------------------------------------------------------------------------------------------------
def _layer(op):
    from gennet_amd import layers as L, regularizers
    kw = dict(op['kw'])
    for k in list(kw):
        if k.endswith('_regularizer'):
            kw[k] = regularizers.L1L2(l1=kw[k][0], l2=kw[k][1])
        elif isinstance(kw[k], list) and k != 'const':
            kw[k] = tuple(kw[k])
    if op['cls'] == 'MyLayer':
        kw['const'] = np.asarray(kw['const'], np.float32)
    if op['cls'] == 'Reshape':
        return L.Reshape(kw.pop('target_shape'), **kw)
    if op['cls'] == 'Activation':
        return L.Activation(kw.pop('activation'), **kw)
    return getattr(L, op['cls'])(**kw)


def _wire(ops, x0):
    from gennet_amd.engine import Input, Model
    t = {0: x0}
    for op in ops:
        ins = [t[i] for i in op['in']]
        if op['cls'] == 'Model':
            xi = Input(tuple(op['in_shape']), name=op['name'] + '_in')
            sub = Model(inputs=xi, outputs=_wire(op['ops'], xi)[op['out']], name=op['name'])
            sub.trainable = op['trainable']
            t[op['id']] = sub(ins[0])
        else:
            l = _layer(op)
            t[op['id']] = l(ins if l.is_merge else ins[0])
    return t


def seed_weights(model, seed):
    """every weight off its initial value, from the seed alone: kernels ~ N(0, 1 / fan_in), biases and betas ~ 0.1 N, gammas 1 + 0.2 N, moving
    means 0.3 N, moving variances in [0.5, 1.5), PReLU slopes 0.25 + 0.1 N"""
    rng = np.random.RandomState(seed + 7919)
    for l in model.layers:
        ws = []
        for p in l.weights:
            kind, shp = p.name.split('/')[-1], p.shape
            if kind == 'kernel':
                fan = int(np.prod(shp[:-1])) if type(l).__name__ != 'Conv2DTranspose' else shp[1] * shp[3]
                w = rng.randn(*shp) / np.sqrt(fan)
            elif kind == 'gamma':
                w = 1.0 + 0.2 * rng.randn(*shp)
            elif kind == 'moving_mean':
                w = 0.3 * rng.randn(*shp)
            elif kind == 'moving_variance':
                w = 0.5 + rng.rand(*shp)
            elif kind == 'alpha':
                w = 0.25 + 0.1 * rng.randn(*shp)
            else:
                w = 0.1 * rng.randn(*shp)
            ws.append(w.astype(np.float32))
        if ws:
            l.set_weights(ws)


def build(spec):
    from gennet_amd.engine import SGD, Input, Model
    x0 = Input(tuple(spec['input']), name='x_%d' % spec['seed'])
    t = _wire(spec['ops'], x0)
    model = Model(inputs=x0, outputs=[t[i] for i in spec['outputs']], name='graph_%d' % spec['seed'])
    seed_weights(model, spec['seed'])
    model.compile(optimizer=SGD(lr=LR), loss=list(spec['losses']), loss_weights=spec['loss_weights'])
    return model


def data(spec, model):
    """(x, targets, dropout keep masks by layer name), from the seed alone"""
    rng = np.random.RandomState(spec['seed'] + 104729)
    B = spec['B']
    x = rng.randn(B, *spec['input']).astype(np.float32)
    targets = []
    for i, kind in zip(model.output_ids, spec['losses']):
        shp = (B,) + tuple(model.nodes[i].out_shape)
        if kind == 'binary_crossentropy':
            t = (rng.rand(*shp) < 0.5).astype(np.float32)
        elif kind == 'categorical_crossentropy':
            t = np.eye(shp[-1], dtype=np.float32)[rng.randint(shp[-1], size=shp[:-1])]
        else:
            t = rng.randn(*shp).astype(np.float32)
        targets.append(t)
    masks = {}
    for n in model.nodes:
        if type(n.layer).__name__ == 'Dropout':
            masks[n.layer.name] = (rng.rand(B, *n.out_shape) >= n.layer.rate).astype(np.uint8)
    return x, targets, masks


# ---- the reference runs and the bounds ------------------------------------------------------------------------------------------------
def rel(a, ref, floor=1e-30):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return float(np.abs(a - ref).max() / max(np.abs(ref).max(), floor)) if ref.size else 0.0


def reference(spec, model, dtype=None):
    """the three runs of the differential test in the interpreter: predict, one SGD step, predict after it (on the reference's own new weights
    and moving statistics) -> (predict, train, predict after)"""
    import torch
    import model_ref
    dtype = dtype or torch.float64
    x, targets, masks = data(spec, model)
    before = model_ref.interpret(model, x, False, dtype=dtype)
    tg = targets if len(targets) > 1 else targets[0]
    train = model_ref.interpret(model, x, True, masks, dtype, targets=tg, lr=LR)
    new = dict(train.new_weights)
    for name, (m, v) in train.moving.items():
        new[name + '/moving_mean'], new[name + '/moving_variance'] = m, v
    after = model_ref.interpret(model, x, False, dtype=dtype, weights=new)
    return before, train, after


def tensors(runs):
    """{(class, name): array} of everything the differential test compares; gradients carry the floor of tests/test_conv_anyc_gpu.py"""
    before, train, after = runs
    out = {}
    for k, o in enumerate(before.outputs):
        out[('output', 'predict %d' % k)] = o
    for k, o in enumerate(after.outputs):
        out[('output', 'predict after the step %d' % k)] = o
    out[('loss', 'loss')] = np.asarray([train.loss])
    for k, l in enumerate(train.losses):
        out[('loss', 'loss of output %d' % k)] = np.asarray([l])
    for name, g in train.grads.items():
        out[('grad', name)] = g
        out[('weight', name)] = train.new_weights[name]
    for name, (m, v) in train.moving.items():
        out[('moving', name + '/moving_mean')], out[('moving', name + '/moving_variance')] = m, v
    return out


def floors(ref):
    """per tensor the floor of the error measure max |a - b| / max(max |b|, floor): 1e-3 of the largest gradient entry for gradients, 1e-3 for
    weights and moving statistics, none otherwise"""
    gmax = max([float(np.abs(v).max()) for (c, _), v in ref.items() if c == 'grad' and v.size] or [0.0])
    return dict((key, 1e-3 * gmax if key[0] == 'grad' else 1e-3 if key[0] in ('weight', 'moving') else 1e-30) for key in ref)


def bounds(ref64, ref32):
    """{key: (bound, e32)}: bound = max(bar, 8 e32) capped at CAP * bar, e32 the float32 interpreter's error against the float64 one"""
    fl = floors(ref64)
    out = {}
    for key, v in ref64.items():
        e32 = rel(ref32[key], v, fl[key])
        bar = BARS[key[0]]
        out[key] = (min(max(bar, 8.0 * e32), CAP * bar), e32)
    return out


def admit(spec, model=None):
    """(admitted, why): the conditions of the corpus, from the interpreter alone.  Kinks: every non-smooth decision of the three runs keeps MARGIN
    from flipping.  Conditioning: 8 e32 stays under the cap of every tensor's bound."""
    import torch
    model = model or build(spec)
    r64 = reference(spec, model)
    for run, what in zip(r64, ('predict', 'train', 'predict after the step')):
        for name, kind, m in run.margins:
            if not m >= MARGIN:
                return False, '%s: %s %s margin %.3g' % (what, name, kind, m)
    t64 = tensors(r64)
    if not all(np.all(np.isfinite(v)) for v in t64.values()):
        return False, 'non-finite reference'
    gmax = max([float(np.abs(v).max()) for (c, _), v in t64.items() if c == 'grad' and v.size] or [0.0])
    if not gmax > 1e-4:
        return False, 'no gradient to speak of (%.3g)' % gmax
    t32 = tensors(reference(spec, model, torch.float32))
    for key, (bound, e32) in bounds(t64, t32).items():
        if 8.0 * e32 > CAP * BARS[key[0]]:
            return False, 'conditioning: %s %s e32 %.3g' % (key[0], key[1], e32)
    return True, ''
