"""The graph generator, its corpus and the fp64 interpreter, checked without a GPU (the differential test itself: tests/test_graph_gen_gpu.py).

  * the interpreter (tests/model_ref.py) against the hand-written torch restatements the feature tests already hold, at the same weights, to 1e-12;
  * every public layer class is in model_ref.LAYER_TABLE, every interpreted one occurs in at least two corpus graphs;
  * every corpus graph planned (Model._plan): each of the planner's six decisions is taken in at least three graphs and declined at least once for
    each of its reasons, and the fan-out sweep of Model._backward meets its three aliasing cases at least twice each -- the tables are printed;
  * the same seed gives the same spec, every corpus seed is admitted at its first draw, and the shapes the library refuses refuse at build()."""
import collections
import inspect

import numpy as np
import pytest
import torch

import graph_corpus
import graph_gen as G
import model_ref

FIELDS = {'fused_act': lambda n: n.fused_act is not None, 'fused_drop': lambda n: n.fused_drop is not None, 'fold_up': lambda n: n.fold_up is not None,
          'infer_bn': lambda n: n.infer_bn is not None, 'fuse_prev': lambda n: n.fuse_prev >= 0, 'lazy_bn': lambda n: n.lazy_bn >= 0}
# the reasons for which the planner declines each decision (Model._plan and the per-layer attributes it asks)
REASONS = {
    'fused_act': ('second consumer', 'model output', 'activity regularizer', 'own activation', 'softmax', 'non-last-axis BatchNormalization'),
    'fused_drop': ('second consumer', 'model output', 'activity regularizer', 'own activation', 'softmax', 'any_channels pair', 'phased conv',
                   'non-last-axis BatchNormalization', 'small filter count'),
    'fold_up': ('second consumer', 'model output', 'activity regularizer', 'phased conv', 'consumer cannot fold'),
    'infer_bn': ('second consumer', 'model output', 'activity regularizer', 'own activation', 'softmax', 'any_channels pair', 'phased conv',
                 'non-last-axis BatchNormalization'),
    'fuse_prev': ('second consumer', 'model output', 'activity regularizer', 'softmax', 'phased conv'),
    'lazy_bn': ('second consumer', 'model output', 'any_channels pair', 'phased conv', 'non-last-axis BatchNormalization'),
}
SWEEP = ('aliased gradient', 'writes_dy consumer of an aliased gradient', 'activity-regularized node with fan-out')


@pytest.fixture(scope='module')
def corpus():
    """[(seed, spec, model)], every model planned"""
    out = []
    for seed in graph_corpus.SEEDS:
        spec = G.generate(seed)
        model = G.build(spec)
        model._plan()
        out.append((seed, spec, model))
    return out


# ---- the interpreter against the restatements the feature tests hold ------------------------------------------------------------------
def _params(model, grad=True):
    return dict((l.name, [torch.tensor(w.astype(np.float64), requires_grad=grad and k < len(l.params)) for k, w in enumerate(l.get_weights())])
                for l in model.layers if l.weights)


def _agree(model, ref_out, x, masks, what, phases=(False, True)):
    """interpret() against the restatement ref_out(P, x64, training): the outputs in the given phases, then the loss and the gradient of
    every trainable tensor under a mean squared error against a fixed target -- all to 1e-12 in the project's relative measure (a gradient
    against its own largest entry, floored as tests/test_conv_anyc_gpu.py floors it: 1e-3 of the model's largest gradient entry, so that a
    bias in front of a BatchNormalization, whose gradient is rounding noise, is measured against the model's scale)"""
    rng = np.random.RandomState(5)
    x64 = torch.tensor(x.astype(np.float64))
    for training in phases:
        out = ref_out(_params(model), x64, training)
        got = model_ref.interpret(model, x, training, masks)
        assert G.rel(got.outputs[0], out.detach().numpy()) < 1e-12, (what, training)
    t = rng.randn(*got.outputs[0].shape).astype(np.float32)
    model.loss, model.loss_weights = 'mean_squared_error', None
    got = model_ref.interpret(model, x, True, masks, targets=t, lr=0.05)
    P = _params(model)
    out = ref_out(P, x64, True)
    loss = ((out - torch.tensor(t.astype(np.float64))) ** 2).reshape(out.shape[0], -1).mean(1).mean()
    loss.backward()
    assert abs(got.loss - float(loss.detach())) <= 1e-12 * abs(float(loss.detach())), what
    refs = dict((p.name, ref.grad.numpy() if ref.grad is not None else np.zeros(p.shape)) for l in model.layers for p, ref in zip(l.params, P.get(l.name, [])))
    assert sorted(refs) == sorted(got.grads) and refs
    floor = 1e-3 * max(float(np.abs(g).max()) for g in refs.values())
    assert floor > 0
    for name, g_ref in refs.items():
        err = G.rel(got.grads[name], g_ref, floor)
        assert err < 1e-12, (what, name, err)


def test_interpreter_agrees_with_the_softmax_models():
    import softmax_models as S
    for key in sorted(S.MODELS):
        model, ref = S.MODELS[key]()
        G.seed_weights(model, 11)
        rng = np.random.RandomState(3)
        x = rng.randn(4, *model.input_shapes[0]).astype(np.float32)
        masks = dict((n.layer.name, (rng.rand(4, *n.out_shape) >= n.layer.rate).astype(np.uint8)) for n in model.nodes if type(n.layer).__name__ == 'Dropout')
        m64 = dict((k, torch.tensor(v.astype(np.float64))) for k, v in masks.items())

        def out(P, x64, training):
            moving = dict((l.name, (P[l.name][2], P[l.name][3])) for l in model.layers if len(l.weights) == 4)
            return ref(P, x64, training, m64, moving)
        _agree(model, out, x, masks, 'softmax model ' + key)


def _stack_tests(mod, names):
    for net in names:
        in_shape, spec = mod.NETS[net]
        model, ls = mod._build(spec, in_shape)
        G.seed_weights(model, 13)
        rng = np.random.RandomState(7)
        x = rng.randn(5, *in_shape).astype(np.float32)
        masks, m64 = {}, {}
        for i, (l, n) in enumerate(zip(ls, model.nodes)):
            if type(l).__name__ == 'Dropout':
                masks[l.name] = (rng.rand(5, *n.out_shape) >= l.rate).astype(np.uint8)
                m64[i] = torch.tensor(masks[l.name].astype(np.float64))
        yield net, spec, model, ls, x, masks, m64


def test_interpreter_agrees_with_the_any_channel_stacks():
    import test_conv_anyc_gpu as A
    for net, spec, model, ls, x, masks, m64 in _stack_tests(A, sorted(A.NETS)):
        def out(P, x64, training):
            Pi = dict((i, P[l.name][:2]) for i, l in enumerate(ls) if l.weights)
            moving = dict((i, P[l.name][2:]) for i, l in enumerate(ls) if len(l.weights) == 4)
            return A._ref_forward(spec, Pi, x64, m64, training, moving)
        _agree(model, out, x, masks, 'any-channel stack ' + net)


def test_interpreter_agrees_with_the_pooling_stacks():
    import test_pooling_gpu as Q
    for net, spec, model, ls, x, masks, m64 in _stack_tests(Q, sorted(Q.NETS)):
        def out(P, x64, training):
            Pi = dict((i, P[l.name][:2]) for i, l in enumerate(ls) if l.weights)
            moving = dict((i, P[l.name][2:]) for i, l in enumerate(ls) if len(l.weights) == 4)
            return Q._ref_forward(spec, Pi, x64, training, moving)
        _agree(model, out, x, masks, 'pooling stack ' + net)


def test_interpreter_agrees_with_the_residual_and_dilated_stacks():
    import test_dilated_gpu as D
    import test_merge_gpu as M
    model, (d_in, d_mid, d_out) = M.residual_model()
    G.seed_weights(model, 17)
    x = np.random.RandomState(1).randn(6, 5).astype(np.float32)

    def residual(P, x64, training):
        h = torch.tanh(x64 @ P[d_in.name][0] + P[d_in.name][1])
        return ((h @ P[d_mid.name][0] + P[d_mid.name][1]) + h) @ P[d_out.name][0] + P[d_out.name][1]
    _agree(model, residual, x, {}, 'residual block')
    model, blocks, head = D.stack_model()
    G.seed_weights(model, 19)
    rng = np.random.RandomState(2)
    x = rng.randn(4, 32, 16).astype(np.float32)
    masks = dict((drop.name, (rng.rand(4, 32, 16) >= D.RATE).astype(np.uint8)) for _, drop, _ in blocks)
    m64 = dict((k, torch.tensor(v.astype(np.float64))) for k, v in masks.items())
    # (stack_ref is the training phase; the interpreter's inference phase is held by the other stacks)
    _agree(model, lambda P, x64, training: D.stack_ref(P, x64, m64), x, masks, 'dilated causal stack', phases=(True,))


# ---- the layer table --------------------------------------------------------------------------------------------------------------------
def _classes(ops):
    for op in ops:
        if op['cls'] == 'Model':
            for c in _classes(op['ops']):
                yield c
        else:
            yield op['cls']


def test_every_public_layer_class_is_in_the_table_and_interpreted_ones_are_in_the_corpus(corpus):
    from gennet_amd import layers as L
    from gennet_amd.engine import Layer, Model
    public = sorted(name for name, c in vars(L).items() if inspect.isclass(c) and issubclass(c, Layer) and c.__module__ == L.__name__
                    and not name.startswith('_') and not issubclass(c, Model))
    assert sorted(model_ref.LAYER_TABLE) == public
    for name, verdict in model_ref.LAYER_TABLE.items():
        assert verdict == 'interpreted' or (verdict.startswith('excluded: ') and len(verdict) > 30), name
    graphs = collections.Counter()
    for seed, spec, model in corpus:
        for c in set(_classes(spec['ops'])):
            graphs[c] += 1
    nested = [(seed, op['trainable']) for seed, spec, _ in corpus for op in spec['ops'] if op['cls'] == 'Model']
    print('graphs per layer class:', dict(graphs))
    print('nested models (seed, trainable):', nested)
    thin = [c for c in model_ref.INTERPRETED if graphs[c] < 2]
    assert not thin, 'interpreted classes in fewer than two corpus graphs: %s' % thin
    assert sum(1 for _, tr in nested if tr) >= 2 and sum(1 for _, tr in nested if not tr) >= 2
    assert sum(1 for _, spec, _ in corpus if len(spec['outputs']) > 1) >= 2


# ---- the planner ------------------------------------------------------------------------------------------------------------------------
def planner_table(corpus):
    """{(field, 'take' | reason): [seeds]} from the generator's notes, each note checked against the plan"""
    table = collections.defaultdict(list)
    for seed, spec, model in corpus:
        by_name = dict((n.layer.name, n) for n in model.nodes)
        for name, field, verdict in spec['notes']:
            if name not in by_name:
                continue               # a branch that reaches no output is no part of the model
            taken = FIELDS[field](by_name[name])
            assert taken == (verdict == 'take'), 'seed %d: %s.%s is %s, the generator meant %r\n%s' % (seed, name, field, taken, verdict, spec)
            if seed not in table[(field, verdict)]:
                table[(field, verdict)].append(seed)
    return table


def sweep_events(model):
    """Model._backward replayed on storage identities alone: which of the fan-out sweep's cases a training step of `model` meets.  A layer's
    backward returns a fresh tensor, except: Add hands its dy to every input, Average one scaled tensor to all, Subtract its dy to the first;
    absorbed nodes, Flatten, Reshape, ActivityRegularization and a linear Activation pass their dy on."""
    events, grads, held, fresh = collections.Counter(), {}, {}, [0]

    def new():
        fresh[0] += 1
        return fresh[0]

    def put(i, s):
        g = grads.get(i)
        if g is None:
            grads[i] = s
            held[s] = held.get(s, 0) + 1
        elif held[g] > 1:
            events['aliased gradient'] += 1
            held[g] -= 1
            grads[i] = s2 = new()
            held[s2] = 1
        # else: accumulated in place
    puts = collections.Counter()
    for i in model.output_ids:
        put(i, new()); puts[i] += 1
    for n in reversed(model.nodes):
        dy = grads.pop(n.index, None)
        if dy is None:
            continue
        held[dy] -= 1
        if not held[dy]:
            del held[dy]
        if n.layer.activity_regularizer is not None and puts[n.index] > 1:
            events['activity-regularized node with fan-out'] += 1
        kind = type(n.layer).__name__
        if n.absorbed or kind in ('Flatten', 'Reshape', 'ActivityRegularization') or getattr(n.layer, 'act_spec', None) == ('linear', 0.0):
            dxs = [dy] * len(n.inbound)
        else:
            if dy in held and n.layer.writes_dy(n):
                events['writes_dy consumer of an aliased gradient'] += 1
            if kind == 'Add':
                dxs = [dy] * len(n.inbound)
            elif kind == 'Average':
                dxs = [new()] * len(n.inbound)
            elif kind == 'Subtract':
                dxs = [dy, new()]
            else:
                dxs = [new() for _ in n.inbound]
        for i, dx in zip(n.inbound, dxs):
            if i >= 0:
                put(i, dx); puts[i] += 1
    return events


def test_the_corpus_covers_the_planner_and_the_fan_out_sweep(corpus):
    table = planner_table(corpus)
    print('\nplanner decisions over the corpus (seeds):')
    empty = []
    for field in FIELDS:
        for verdict in ('take',) + REASONS[field]:
            seeds = table.get((field, verdict), [])
            print('  %-10s %-34s %2d  %s' % (field, verdict, len(seeds), seeds))
            if len(seeds) < (3 if verdict == 'take' else 1):
                empty.append((field, verdict))
    unknown = [k for k in table if k[1] != 'take' and k[1] not in REASONS[k[0]]]
    assert not unknown, unknown
    sweep = collections.defaultdict(list)
    for seed, spec, model in corpus:
        for ev in sweep_events(model):
            sweep[ev].append(seed)
    print('fan-out sweep:')
    for ev in SWEEP:
        print('  %-44s %2d  %s' % (ev, len(sweep[ev]), sweep[ev]))
        if len(sweep[ev]) < 2:
            empty.append(('sweep', ev))
    assert not empty, 'cells of the coverage table the corpus leaves empty: %s' % empty


def test_the_unfolded_ragged_upsample_is_in_the_corpus_in_its_three_placements(corpus):
    """UpSampling1D on a channel count that is no multiple of 4, run as its own kernel: in front of a consumer that cannot fold it, with two
    consumers, and as a model output"""
    seen = collections.defaultdict(list)
    for seed, spec, model in corpus:
        consumers = collections.Counter(i for n in model.nodes for i in n.inbound)
        for n in model.nodes:
            if type(n.layer).__name__ == 'UpSampling1D' and not n.absorbed and n.out_shape[1] % 4:
                if n.index in model.output_ids:
                    seen['model output'].append(seed)
                elif consumers[n.index] > 1:
                    seen['two consumers'].append(seed)
                else:
                    seen['consumer cannot fold'].append(seed)
    print('unfolded ragged upsample:', dict(seen))
    assert all(seen[k] for k in ('model output', 'two consumers', 'consumer cannot fold')), dict(seen)


def test_the_corpus_runs_a_dropout_behind_every_conv_form(corpus):
    """a Dropout directly behind (an activation layer behind) a Conv2DTranspose, a width-2 Conv2D, one with <= 2 filters, and a Conv1D with
    <= 4 filters: fused into the epilogue or, where the kernel has none, a pass of its own"""
    seen = collections.defaultdict(list)
    for seed, spec, model in corpus:
        consumers = collections.defaultdict(list)
        for n in model.nodes:
            for i in n.inbound:
                if i >= 0:
                    consumers[i].append(n)
        for n in model.nodes:
            kind = type(n.layer).__name__
            if kind not in ('Conv1D', 'Conv2D', 'Conv2DTranspose'):
                continue
            cur = n
            for _ in range(2):
                if len(consumers[cur.index]) != 1:
                    break
                cur = consumers[cur.index][0]
                if type(cur.layer).__name__ == 'Dropout':
                    small = (kind == 'Conv1D' and n.layer.filters <= 4) or (kind == 'Conv2D' and n.layer.filters <= 2)
                    seen[kind + (' (few filters)' if small else '')].append(seed)
                    break
                if getattr(cur.layer, 'act_spec', None) is None:
                    break
    print('Dropout behind:', dict(seen))
    assert all(seen[k] for k in ('Conv1D', 'Conv1D (few filters)', 'Conv2D', 'Conv2D (few filters)', 'Conv2DTranspose')), dict(seen)


# ---- determinism, admission, refusals ---------------------------------------------------------------------------------------------------
def test_the_same_seed_gives_the_same_spec_and_every_corpus_seed_is_admitted(corpus):
    assert len(graph_corpus.SEEDS) == 48 == len(set(graph_corpus.SEEDS))
    for seed, spec, model in corpus:
        assert G.generate(seed) == spec and repr(G.generate(seed)) == repr(spec)
        assert 3 <= spec['B'] <= 6 and len(model.nodes) <= 16
        ok, why = G.admit(spec)
        assert ok, 'seed %d is not admitted: %s' % (seed, why)


def test_a_conv_with_too_few_columns_for_the_dropout_epilogue_declines_it():
    """gn_conv1d_fwd_dropout needs more than 4 output columns: a built Conv1D with <= 4 filters and a width-2 Conv2D with <= 2 filters (2 * filters
    columns) leave the Dropout behind them a pass of its own; one filter more and it is fused"""
    from gennet_amd import layers as L
    from gennet_amd.engine import Sequential
    cases = ((lambda: L.Conv1D(4, 3, input_shape=(16, 8)), False), (lambda: L.Conv1D(1, 5, padding='same', input_shape=(16, 8)), False),
             (lambda: L.Conv1D(8, 3, input_shape=(16, 8)), True), (lambda: L.Conv2D(2, (3, 5), padding='same', input_shape=(8, 2, 2)), False),
             (lambda: L.Conv2D(4, (3, 5), padding='same', input_shape=(8, 2, 2)), True))
    for make, fused in cases:
        for act in (False, True):
            m = Sequential([make()] + ([L.LeakyReLU(0.2)] if act else []) + [L.Dropout(0.3)])
            m._plan()
            conv, last = m.nodes[0], m.nodes[-1]
            assert (conv.fused_drop is not None) == fused and last.absorbed == fused, (type(conv.layer).__name__, conv.layer.filters, act)
            assert (conv.fused_act is not None) == act


def test_shapes_the_library_cannot_run_are_refused_at_build():
    from gennet_amd import layers as L
    from gennet_amd.engine import Input
    for what, make, shape, text in graph_corpus.REFUSED:
        with pytest.raises((NotImplementedError, ValueError), match=text):
            make(L)(Input(shape))
