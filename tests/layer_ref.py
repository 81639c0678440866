"""fp64 numpy references of the streaming passes oracle/keras_ref.py does not restate (tests/test_layer_passes_gpu.py checks the HIP
kernels against them, tests/test_layer_ref_cpu.py checks THEM against torch float64 autograd or a plain loop).  dtype-preserving, like the
oracle: the tests run them in float64."""
import numpy as np

from oracle import keras_ref as K


def act_dropout_bwd(dy, y, mask, kind, param, rate):
    """Backward of [activation -> inverted dropout] written through the LAYER output y = mask * act(z) / (1 - rate) (what a layer keeps):
    the activation output is recovered as y (1 - rate) where the element was kept; dz = mask ? dy / (1 - rate) * act'(that) : 0."""
    keep_scale = 1.0 / (1.0 - rate)
    keep = np.asarray(mask) != 0
    return np.where(keep, K.act_bwd(dy * keep_scale, y / keep_scale, kind, param), 0.0)


def affine_stack_fwd(x, a0, b0, a1, b1):
    """x (B, n, 1) -> (B, n, 2, 1): stack([a0 x + b0, a1 x + b1], axis=2); b0 / b1 (n,) vectors along axis 1, or None.
    MyLayer (K.mylayer_fwd) is (1, None, -1, event)."""
    n = x.shape[1]
    c0 = a0 * x + (0.0 if b0 is None else np.reshape(b0, (1, n, 1)))
    c1 = a1 * x + (0.0 if b1 is None else np.reshape(b1, (1, n, 1)))
    return np.stack([c0, c1], axis=2)


def affine_stack_bwd(dimg, a0, a1):
    return a0 * dimg[:, :, 0] + a1 * dimg[:, :, 1]


def assemble_d_batch(real, noise, fake, event):
    """The discriminator batch of one GAN iteration as width-2 images (2B, n, 2, 1): rows 0..B-1 are [real | noise]; then the fake samples
    in REVERSED order (the training loop prepends them one by one), each as [f | event - f].  real, noise, fake (B, n); event (n,)."""
    B, n = real.shape
    ev = np.reshape(event, (1, n))
    f = fake[::-1]
    top = np.stack([real, noise], axis=2)
    bot = np.stack([f, ev - f], axis=2)
    return np.concatenate([top, bot], axis=0).reshape(2 * B, n, 2, 1)
