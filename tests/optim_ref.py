"""fp64 restatement of the Keras 2.2.4 optimizers (keras/optimizers.py: SGD, RMSprop, Adagrad, Adadelta, Adamax, Adam with amsgrad) and of
Optimizer.get_gradients' clipping, written from the rules alone (no gennet_amd import).  KerasOpt.step(params, grads) updates a list of numpy
arrays in place: the interface of oracle.nets_ref.AdamState, so a test can put it in place of a network oracle's optimizer.

What Keras holds as K.variable (lr, decay, momentum, RMSprop's rho, beta_1, beta_2) takes part float32-rounded; Adadelta's rho and epsilon
are python floats; epsilon=None is K.epsilon() = 1e-7."""
import numpy as np

K_EPS = 1e-7

DEFAULTS = {
    'sgd': dict(lr=0.01, momentum=0.0, decay=0.0, nesterov=False),
    'rmsprop': dict(lr=0.001, rho=0.9, epsilon=None, decay=0.0),
    'adagrad': dict(lr=0.01, epsilon=None, decay=0.0),
    'adadelta': dict(lr=1.0, rho=0.95, epsilon=None, decay=0.0),
    'adamax': dict(lr=0.002, beta_1=0.9, beta_2=0.999, epsilon=None, decay=0.0),
    'adam': dict(lr=0.001, beta_1=0.9, beta_2=0.999, epsilon=None, decay=0.0, amsgrad=False),
}
F32_HYPER = {'sgd': ('lr', 'momentum', 'decay'), 'rmsprop': ('lr', 'rho', 'decay'), 'adagrad': ('lr', 'decay'), 'adadelta': ('lr', 'decay'),
             'adamax': ('lr', 'beta_1', 'beta_2', 'decay'), 'adam': ('lr', 'beta_1', 'beta_2', 'decay')}
# optimizer.weights of Keras 2.2.4: does `iterations` lead, and the per-weight state blocks in order
LAYOUT = {'sgd': (True, ('m',)), 'rmsprop': (False, ('a',)), 'adagrad': (False, ('a',)), 'adadelta': (False, ('a', 'd')),
          'adamax': (True, ('m', 'u')), 'adam': (True, ('m', 'v', 'vhat'))}


def f32(x):
    return float(np.float32(x))


def config(kind, **kw):
    """The hyper-parameters as they take part (float32 where Keras keeps a K.variable), Keras defaults filled in."""
    unknown = set(kw) - set(DEFAULTS[kind]) - {'clipnorm', 'clipvalue'}
    assert not unknown, unknown
    c = dict(DEFAULTS[kind], **kw)
    for k in F32_HYPER[kind]:
        c[k] = f32(c[k])
    if 'epsilon' in c:
        c['epsilon'] = K_EPS if c['epsilon'] is None else float(c['epsilon'])
    return c


def clip_gradients(grads, clipnorm=None, clipvalue=None):
    """Optimizer.get_gradients: norm over ALL gradients; g * clipnorm / norm when norm >= clipnorm; then clip to +-clipvalue."""
    grads = [np.asarray(g, np.float64) for g in grads]
    if clipnorm is not None and clipnorm > 0:
        norm = np.sqrt(sum(float(np.sum(g * g)) for g in grads))
        if norm >= clipnorm:
            grads = [g * clipnorm / norm for g in grads]
    if clipvalue is not None and clipvalue > 0:
        grads = [np.clip(g, -clipvalue, clipvalue) for g in grads]
    return grads


class KerasOpt(object):
    def __init__(self, kind, params, **kw):
        self.kind = kind
        self.c = config(kind, **kw)
        self.iterations = 0
        n_state = {'sgd': 1, 'rmsprop': 1, 'adagrad': 1, 'adadelta': 2, 'adamax': 2, 'adam': 3 if self.c.get('amsgrad') else 2}[kind]
        self.state = [[np.zeros(np.shape(p), np.float64) for p in params] for _ in range(n_state)]

    @property
    def t(self):
        return self.iterations

    def step(self, params, grads):
        c = self.c
        grads = clip_gradients(grads, c.get('clipnorm'), c.get('clipvalue'))
        it = self.iterations
        t = it + 1
        lr = c['lr'] / (1.0 + c['decay'] * it) if c['decay'] > 0 else c['lr']
        for i, (p, g) in enumerate(zip(params, grads)):
            s = [st[i] for st in self.state]
            if self.kind == 'sgd':
                v = c['momentum'] * s[0] - lr * g
                s[0][...] = v
                new = p + c['momentum'] * v - lr * g if c['nesterov'] else p + v
            elif self.kind in ('rmsprop', 'adagrad'):
                s[0][...] = c['rho'] * s[0] + (1.0 - c['rho']) * g * g if self.kind == 'rmsprop' else s[0] + g * g
                new = p - lr * g / (np.sqrt(s[0]) + c['epsilon'])
            elif self.kind == 'adadelta':
                rho, eps = c['rho'], c['epsilon']
                s[0][...] = rho * s[0] + (1.0 - rho) * g * g
                u = g * np.sqrt(s[1] + eps) / np.sqrt(s[0] + eps)
                new = p - lr * u
                s[1][...] = rho * s[1] + (1.0 - rho) * u * u
            elif self.kind == 'adamax':
                lr_t = lr / (1.0 - c['beta_1'] ** t)
                s[0][...] = c['beta_1'] * s[0] + (1.0 - c['beta_1']) * g
                s[1][...] = np.maximum(c['beta_2'] * s[1], np.abs(g))
                new = p - lr_t * s[0] / (s[1] + c['epsilon'])
            else:
                lr_t = lr * np.sqrt(1.0 - c['beta_2'] ** t) / (1.0 - c['beta_1'] ** t)
                s[0][...] = c['beta_1'] * s[0] + (1.0 - c['beta_1']) * g
                s[1][...] = c['beta_2'] * s[1] + (1.0 - c['beta_2']) * g * g
                den = s[1]
                if c['amsgrad']:
                    s[2][...] = np.maximum(s[2], s[1])
                    den = s[2]
                new = p - lr_t * s[0] / (np.sqrt(den) + c['epsilon'])
            params[i][...] = new
        self.iterations = t

    def keras_weights(self, params):
        """optimizer.get_weights() in Keras 2.2.4's layout (Adam without amsgrad: (1,) zero vhat stubs)."""
        lead, blocks = LAYOUT[self.kind]
        out = [np.asarray(self.iterations, np.int64)] if lead else []
        for k, _ in enumerate(blocks):
            if k < len(self.state):
                out += [a.copy() for a in self.state[k]]
            else:
                out += [np.zeros((1,), np.float32) for _ in params]
        return out
