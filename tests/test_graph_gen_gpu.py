"""Differential test: every graph of tests/graph_corpus.py on the GPU against the fp64 interpreter of tests/model_ref.py, which knows nothing of
the planner -- predict, one SGD train_on_batch with injected dropout masks, predict again: outputs, the loss and every per-output loss, every
trained tensor's gradient, the weights after the step, the BatchNormalization moving statistics.

The error measure is the project's, max |a - b| / max(max |b|, floor); the bound of a tensor is max(bar, 8 e32) capped at 10 bar, with the bars of
tests/test_conv_anyc_gpu.py (1e-5 outputs, 1e-6 loss, 1e-4 gradients, updated weights and moving statistics; gradients with that file's floor of
1e-3 of the largest gradient entry) and e32 the error of the interpreter run in float32 against its float64 run on the same graph -- the
reference's own rounding noise, never the library's.  Admission (graph_gen.admit) keeps 8 e32 under the cap for every corpus graph.

The default conv math; a graph that reaches a transform-domain kernel (graph_corpus.TRANSFORM) runs under ops.conv_math('fp32') as well, where it
must reach none.  The out-of-place sums and copies the real backward sweep makes are counted and held against the replay the CPU coverage
table is built from.  On a mismatch the message names the first node, in graph order, whose captured output leaves the bound, and prints the spec."""
import numpy as np
import pytest
import torch

import conv_family as CF
import graph_corpus
import graph_gen as G

pytestmark = pytest.mark.gpu

TRANSFORM_KINDS = (5, 6, 7, 8)


class SweepCounts(object):
    """what Model._backward's fan-out handling launched during one step: the out-of-place sums of put() (ops.merge_fwd 'add') and the copies
    handed to a layer that overwrites an aliased dy (ops.scale by 1.0), counted inside the sweep only"""

    def __init__(self, model):
        from gennet_amd import ops
        self.out_of_place = self.copies = 0
        self.inside = False
        merge_fwd, scale, backward = ops.merge_fwd, ops.scale, model._backward

        def counted_merge(mode, xs, *a, **k):
            self.out_of_place += int(self.inside and mode == 'add')
            return merge_fwd(mode, xs, *a, **k)

        def counted_scale(t, f, *a, **k):
            self.copies += int(self.inside and f == 1.0)
            return scale(t, f, *a, **k)

        def sweep(*a, **k):
            self.inside = True
            try:
                return backward(*a, **k)
            finally:
                self.inside = False
        self.patches = ((ops, 'merge_fwd', counted_merge), (ops, 'scale', counted_scale), (model, '_backward', sweep))


def run_engine(spec, model, monkeypatch=None, sweep=None):
    if sweep is not None:
        for obj, name, fn in sweep.patches:
            monkeypatch.setattr(obj, name, fn)
    x, targets, masks = G.data(spec, model)
    B = spec['B']
    tg = targets if len(targets) > 1 else targets[0]
    got, cap = {}, {}
    y0 = model.predict(x, batch_size=B)
    res = model.train_on_batch(x, tg, dropout_masks=masks, capture=cap)
    y1 = model.predict(x, batch_size=B)
    for k, o in enumerate(y0 if isinstance(y0, list) else [y0]):
        got[('output', 'predict %d' % k)] = o
    for k, o in enumerate(y1 if isinstance(y1, list) else [y1]):
        got[('output', 'predict after the step %d' % k)] = o
    got[('loss', 'loss')] = np.asarray([res[0]])
    if len(targets) > 1:
        for k in range(len(targets)):
            got[('loss', 'loss of output %d' % k)] = np.asarray([res[1 + k]])
    else:                                  # one output: keras reports no per-output entry; it is the loss without the penalties
        got[('loss', 'loss of output 0')] = None
    for p in model._train_params:
        got[('grad', p.name)] = p.grad.detach().cpu().numpy()
        got[('weight', p.name)] = p.numpy()
    for l in model.layers:
        if type(l).__name__ == 'BatchNormalization':
            got[('moving', l.name + '/moving_mean')], got[('moving', l.name + '/moving_variance')] = l.moving_mean.numpy(), l.moving_variance.numpy()
    return got, dict((k, v.detach().cpu().numpy()) for k, v in cap.items())


def first_bad_node(model, train, captured, bound):
    """the first node in graph order whose captured training-phase output is neither its own reference output nor, where the planner ran a
    follower inside it, that of a node up to three single-consumer steps further on"""
    consumers = dict((n.index, []) for n in model.nodes)
    for n in model.nodes:
        for i in n.inbound:
            if i >= 0:
                consumers[i].append(n)
    for n in model.nodes:
        if n.layer.name not in captured:
            continue
        got, cur, errs = captured[n.layer.name], n, []
        for _ in range(4):
            ref = train.nodes[cur.layer.name]
            if ref.size == got.size:
                errs.append(G.rel(got.reshape(ref.shape), ref))
            if len(consumers[cur.index]) != 1:
                break
            cur = consumers[cur.index][0]
        if not errs or min(errs) > bound:
            return '%s (%s): error %s' % (n.layer.name, type(n.layer).__name__, ' / '.join('%.3g' % e for e in errs))
    return 'none (every captured forward output is within %.3g: the disagreement arises in the backward sweep or the update)' % bound


def compare(seed, spec, model, runs, bnds, ref, got, captured, what):
    fl = G.floors(ref)
    worst, bad, widest = {}, [], {}
    assert sorted(got) == sorted(ref), (sorted(got), sorted(ref))
    for key in sorted(ref):
        if got[key] is None:
            continue
        bound, e32 = bnds[key]
        err = G.rel(np.asarray(got[key], np.float64).reshape(ref[key].shape), ref[key], fl[key])
        if not np.isfinite(err):
            err = np.inf
        if err / bound >= worst.get(key[0], (-1.0,))[0]:
            worst[key[0]] = (err / bound, err, bound, e32)
        widest[key[0]] = max(widest.get(key[0], 0.0), bound)
        if not err <= bound:
            bad.append('%s %s: error %.3g, bound %.3g (e32 %.3g)' % (key[0], key[1], err, bound, e32))
    # per tensor class the tensor closest to its bound: error / bound (error, its bound, the reference's own float32 error), and the widest bound
    print('seed %d %s: %s' % (seed, what, '  '.join('%s %.3f (error %.2e, bound %.2e, e32 %.2e; widest bound %.2e)' % ((c,) + w + (widest[c],))
                                                    for c, w in sorted(worst.items()))))
    if bad:
        node = first_bad_node(model, runs[1], captured, G.CAP * G.BARS['output'])
        raise AssertionError('seed %d (%s): %d tensors leave their bound:\n  %s\nfirst node off: %s\nspec: %r'
                             % (seed, what, len(bad), '\n  '.join(bad), node, spec))


@pytest.mark.parametrize('seed', graph_corpus.SEEDS)
def test_graph_against_the_fp64_interpreter(seed, monkeypatch):
    from gennet_amd import ops
    from test_graph_gen_cpu import sweep_events
    spec = G.generate(seed)
    model = G.build(spec)
    runs = G.reference(spec, model)
    ref = G.tensors(runs)
    bnds = G.bounds(ref, G.tensors(G.reference(spec, model, torch.float32)))
    sweep = SweepCounts(model)
    (got, captured), counts = CF.launches(lambda: run_engine(spec, model, monkeypatch, sweep))
    torch.cuda.synchronize()
    transform = any(counts[k] for k in TRANSFORM_KINDS)
    compare(seed, spec, model, runs, bnds, ref, got, captured, 'default conv math')
    # the fan-out cases the CPU coverage table claims for this graph (a replay of the sweep on storage identities) are the ones the real sweep took
    events = sweep_events(model)
    assert (sweep.out_of_place, sweep.copies) == (events['aliased gradient'], events['writes_dy consumer of an aliased gradient']), \
        'seed %d: the sweep summed out of place %d times and copied %d times; the replay says %s' % (seed, sweep.out_of_place, sweep.copies, dict(events))
    assert transform == (seed in graph_corpus.TRANSFORM), 'seed %d: transform-domain launches %s' % (seed, counts)
    if transform:
        model = G.build(spec)              # the same seeded weights again
        with ops.conv_math('fp32'):
            (got, captured), counts = CF.launches(lambda: run_engine(spec, model))
        torch.cuda.synchronize()
        assert not any(counts[k] for k in TRANSFORM_KINDS) and counts[0], counts      # the same convs on the direct kernels
        compare(seed, spec, model, runs, bnds, ref, got, captured, "conv math 'fp32'")
