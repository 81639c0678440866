"""Keras 2.2.4 layers.Dot without a GPU: the facade, keras' output shapes and refusals, the JSON round trip, what the planner does around a Dot
node, and the fp64 numpy definition tests/dot_ref.py (the reference of tests/test_dot_gpu.py) against torch.matmul autograd in fp64."""
import json

import numpy as np
import pytest
import torch

import dot_ref as R


def test_facade_names_are_the_layer():
    from gennet_amd import keras, layers
    import gennet_amd.keras.layers.merge as merge
    assert keras.layers.Dot is keras.layers.merge.Dot is merge.Dot is layers.Dot
    assert keras.layers.dot is keras.layers.merge.dot is layers.dot
    # the placeholders stay placeholders
    for mod, name in ((keras.layers.convolutional, 'UpSampling2D'), (keras.layers.advanced_activations, 'ThresholdedReLU'), (keras.optimizers, 'Nadam')):
        with pytest.raises(NotImplementedError):
            getattr(mod, name)()


# shapes without the batch axis, axes, keras' output shape without the batch axis
SHAPES = [(((6, 4), (5, 4)), (2, 2), (6, 5)),          # (B,L,C) . (B,M,C) -> (B,L,M)
          (((6, 5), (5, 4)), (2, 1), (6, 4)),          # (B,L,M) . (B,M,C) -> (B,L,C)
          (((6,), (6, 4)), (1, 1), (4,)),              # (B,L) . (B,L,C) -> (B,C)
          (((7,), (7,)), 1, (1,)),                     # (B,n) . (B,n) -> (B,1)
          (((6, 4), (5, 4)), -1, (6, 5)),
          (((7,), (3, 7)), -1, (3,)),                  # -1 modulo each rank: axes (1, 2)
          (((6, 4), (6, 5)), 1, (4, 5)),               # axes=1 on two rank-3 inputs -> (B, C1, C2)
          (((6, 4), (4,)), (2, 1), (6,)),              # (B,L,C) . (B,C) -> (B,L)
          (((6, 4), (4, 6)), [1, 2], (4, 4))]


@pytest.mark.parametrize('shapes,axes,want', SHAPES)
def test_output_shapes_are_keras(shapes, axes, want):
    from gennet_amd import layers as Ly
    from gennet_amd.engine import Input
    a, b = Input(shapes[0]), Input(shapes[1])
    out = Ly.Dot(axes)([a, b])
    assert tuple(out.shape) == want
    assert tuple(Ly.dot([a, b], axes, normalize=True).shape) == want
    assert R.out_shape((3,) + shapes[0], (3,) + shapes[1], axes) == (3,) + want
    rng = np.random.RandomState(0)
    y, _ = R.dot_fwd(rng.randn(3, *shapes[0]), rng.randn(3, *shapes[1]), axes)
    assert y.shape == (3,) + want


def test_refusals():
    from gennet_amd import layers as Ly
    from gennet_amd.engine import Input
    a, b, v, big = Input((6, 4)), Input((5, 4)), Input((4,)), Input((2, 3, 4))
    for bad in ([a], [a, b, b], a):
        with pytest.raises(ValueError, match='A `Dot` layer should be called on exactly 2 inputs'):
            Ly.Dot(2)(bad)
    with pytest.raises(ValueError, match='exactly 2 inputs'):
        Ly.Dot(2).compute_output_shape([(6, 4)] * 3)
    for axes in (0, (0, 1), (1, 0)):
        with pytest.raises(ValueError, match='batch axis'):
            Ly.Dot(axes)
    for axes in (1.0, (1, 2, 2), 'ab', None, (1, 1.5), True):
        with pytest.raises(ValueError, match='an integer or a pair of integers'):
            Ly.Dot(axes)
    for axes in (3, (2, 3), (-1, -1), -3):
        with pytest.raises(ValueError, match='its axis must be one of'):
            Ly.Dot(axes)([a, b])
    with pytest.raises(ValueError, match='its axis must be one of 1 .. 1'):
        Ly.Dot(2)([a, v])
    with pytest.raises(ValueError, match=r'Dimension incompatibility 6 != 5. Layer shapes: \(None, 6, 4\), \(None, 5, 4\)'):
        Ly.Dot(1)([a, b])
    with pytest.raises(ValueError, match='Dimension incompatibility 4 != 5'):
        Ly.Dot((2, 1))([a, b])
    with pytest.raises(NotImplementedError, match='rank 4'):
        Ly.Dot(-1)([big, big])
    with pytest.raises(NotImplementedError, match='rank 4'):
        Ly.Dot((2, 3))([a, big])
    # a Dot is a merge layer for the engine, and no other layer takes its list
    assert Ly.Dot(1).is_merge and not Ly.Dot(1).writes_dy(None)
    with pytest.raises(ValueError, match='takes a single tensor'):
        Ly.Dense(3)([a, b])


def attention_model():
    from gennet_amd import layers as Ly
    from gennet_amd.engine import Input, Model
    x = Input((10, 8))
    q, k, v = Ly.Conv1D(8, 1)(x), Ly.Conv1D(8, 1)(x), Ly.Conv1D(8, 1)(x)
    scores = Ly.Dot((2, 2))([q, k])
    w = Ly.Softmax(-1)(scores)
    ctx = Ly.Dot((2, 1))([w, v])
    h = Ly.Add()([ctx, x])
    return Model(inputs=x, outputs=Ly.Dense(1)(Ly.GlobalAveragePooling1D()(h)))


@pytest.mark.parametrize('axes,normalize', [(2, False), ((2, 1), False), (1, True), (-1, True)])
def test_json_round_trip(axes, normalize):
    from gennet_amd import layers as Ly
    from gennet_amd.engine import Input, Model, model_from_json
    shapes = {2: ((6, 4), (5, 4)), (2, 1): ((6, 5), (5, 4)), 1: ((7,), (7,)), -1: ((7,), (3, 7))}[axes]
    a, b = Input(shapes[0]), Input(shapes[1])
    m = Model(inputs=[a, b], outputs=Ly.Dot(axes, normalize=normalize, name='prod')([a, b]))
    cfg = json.loads(m.to_json())
    entry = [l for l in cfg['config']['layers'] if l['class_name'] == 'Dot'][0]
    assert entry['config'] == {'name': 'prod', 'trainable': True, 'axes': list(axes) if isinstance(axes, tuple) else axes, 'normalize': normalize}
    assert len(entry['inbound_nodes'][0]) == 2
    again = model_from_json(m.to_json())
    d = [n.layer for n in again.nodes if type(n.layer).__name__ == 'Dot'][0]
    assert d.axes == (axes if not isinstance(axes, list) else tuple(axes)) and d.normalize is normalize and d.name == 'prod'
    assert [n.inbound for n in again.nodes] == [n.inbound for n in m.nodes] == [[-1, -2]]
    assert [tuple(n.out_shape) for n in again.nodes] == [tuple(n.out_shape) for n in m.nodes]
    assert json.loads(again.to_json()) == cfg


def test_json_round_trip_of_the_attention_block():
    from gennet_amd.engine import model_from_json
    m = attention_model()
    again = model_from_json(m.to_json())
    assert [type(n.layer).__name__ for n in again.nodes] == [type(n.layer).__name__ for n in m.nodes]
    assert [n.inbound for n in again.nodes] == [n.inbound for n in m.nodes]


def test_planner_around_a_dot_node():
    """No fusion reaches a Dot node or through it: the convs in front keep no epilogue and absorb nothing, Softmax and Add behind run as themselves,
    and the node's own planner fields stay at rest."""
    from gennet_amd import layers as Ly
    from gennet_amd.engine import Input, Model
    m = attention_model()
    m._plan()
    kinds = [type(n.layer).__name__ for n in m.nodes]
    assert kinds == ['Conv1D', 'Conv1D', 'Dot', 'Softmax', 'Conv1D', 'Dot', 'Add', 'GlobalAveragePooling1D', 'Dense']
    assert [n.inbound for n in m.nodes] == [[-1], [-1], [0, 1], [2], [-1], [3, 4], [5, -1], [6], [7]]
    for n in m.nodes:
        assert not n.absorbed and n.fused_act is None and n.fused_drop is None and n.fuse_prev < 0 and n.fold_up is None and n.infer_bn is None \
            and n.lazy_bn < 0, type(n.layer).__name__
    assert m.nodes[2].out_shape == (10, 10) and m.nodes[5].out_shape == (10, 8)
    # an activation and a dropout behind a Dot are not absorbed by it; a conv with an activation in front keeps its own epilogue only
    x = Input((6, 4))
    c = Ly.Conv1D(4, 3, padding='same')(x)
    act = Ly.Activation('tanh')(c)
    d = Ly.Dot(2)([act, act])
    drop = Ly.Dropout(0.1)(Ly.Activation('relu')(d))
    m2 = Model(inputs=x, outputs=Ly.Dense(1)(Ly.Flatten()(drop)))
    m2._plan()
    conv, a0, dot, a1, dr = m2.nodes[:5]
    assert conv.fused_act == ('tanh', 0.0) and a0.absorbed and dot.inbound == [1, 1]
    assert not dot.absorbed and dot.fused_act is None and dot.fused_drop is None and not a1.absorbed and not dr.absorbed
    assert all(n.fuse_prev < 0 for n in m2.nodes[:5])
    assert not dot.layer.writes_dy(dot)


def _torch_dot(x1, x2, axes, normalize):
    """K.batch_dot / K.l2_normalize restated on torch.matmul (rank-3 views, the contracted axis moved last / first)"""
    a1, a2 = R._axes(axes, (x1.dim(), x2.dim()))
    if normalize:
        x1 = x1 / torch.sqrt(torch.clamp((x1 * x1).sum(a1, keepdim=True), min=R.L2_EPS))
        x2 = x2 / torch.sqrt(torch.clamp((x2 * x2).sum(a2, keepdim=True), min=R.L2_EPS))
    u = x1.unsqueeze(2) if x1.dim() == 2 else x1
    v = x2.unsqueeze(2) if x2.dim() == 2 else x2
    u = u.transpose(1, 2) if a1 == 1 else u
    v = v.transpose(1, 2) if a2 == 2 else v
    return torch.matmul(u, v).reshape(R.out_shape(tuple(x1.shape), tuple(x2.shape), axes))


@pytest.mark.parametrize('normalize', [False, True])
@pytest.mark.parametrize('shapes,axes,want', SHAPES)
def test_the_reference_agrees_with_torch_autograd(shapes, axes, want, normalize):
    rng = np.random.RandomState(len(want) + 7 * normalize)
    x1, x2 = rng.randn(3, *shapes[0]), rng.randn(3, *shapes[1])
    if normalize:                                      # one all-zero vector along each input's axis: y = 0 there, the gradient is inv * dy
        a1, a2 = R._axes(axes, (x1.ndim, x2.ndim))
        for x, ax, sample in ((x1, a1, 0), (x2, a2, 1)):
            if x.ndim == 2:
                x[sample] = 0.0
            elif ax == 2:
                x[sample, 0] = 0.0
            else:
                x[sample, :, 0] = 0.0
    t1, t2 = torch.tensor(x1, requires_grad=True), torch.tensor(x2, requires_grad=True)
    out = _torch_dot(t1, t2, axes, normalize)
    dy = rng.randn(*out.shape)
    out.backward(torch.tensor(dy))
    y, cache = R.dot_fwd(x1, x2, axes, normalize)
    d1, d2 = R.dot_bwd(dy, cache)
    assert y.shape == tuple(out.shape)
    assert np.abs(y - out.detach().numpy()).max() <= 1e-12
    assert np.abs(d1 - t1.grad.numpy()).max() <= 1e-12 * max(1.0, np.abs(d1).max()) and np.abs(d2 - t2.grad.numpy()).max() <= 1e-12 * max(1.0, np.abs(d2).max())
    if normalize:
        assert cache[4][1].any() and cache[5][1].any() and not cache[4][1].all()          # clamped vectors are there, and unclamped ones


def test_l2norm_reference_on_a_zero_vector():
    x = np.zeros((2, 5, 3))
    x[1] = np.arange(15).reshape(5, 3) + 1.0
    y, inv, cl = R.l2norm_fwd(x, (2, 5, 3))
    assert cl[0].all() and not cl[1].any() and (y[0] == 0).all() and np.allclose(inv[0], 1e6) and np.allclose((y[1] ** 2).sum(0), 1.0)
    dy = np.ones((2, 5, 3))
    dx = R.l2norm_bwd(dy, y, inv, cl, (2, 5, 3))
    assert np.allclose(dx[0], 1e6)
    assert np.abs((dx[1] * x[1]).sum(0)).max() < 1e-12          # the gradient of a normalised vector is orthogonal to it


def test_bmm_reference_orientations():
    rng = np.random.RandomState(1)
    a, b = rng.randint(-4, 5, (2, 3, 5)), rng.randint(-4, 5, (2, 5, 4))
    want = np.matmul(a, b)
    assert R.bmm(a, b).dtype == np.int64 and np.array_equal(R.bmm(a, b), want)
    assert np.array_equal(R.bmm(a.transpose(0, 2, 1).copy(), b, trans_a=True), want)
    assert np.array_equal(R.bmm(a, b.transpose(0, 2, 1).copy(), trans_b=True), want)
    assert np.array_equal(R.bmm(a.transpose(0, 2, 1).copy(), b.transpose(0, 2, 1).copy(), True, True), want)
