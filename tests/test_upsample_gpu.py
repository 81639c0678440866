"""UpSampling1D(2) on any channel count (csrc/elementwise.hip: upsample2_fwd_kernel / upsample2_bwd_kernel) against oracle.keras_ref: the
forward bit for bit, the backward to the one rounding of its two-term sum; on a 16-byte aligned base (float4 units when C % 4 == 0) and on a
base one float past it (one-float units for every C); one block with a tail, and more units than one trip of the grid (2048 blocks of 256
lanes) so that the grid-stride loop makes a second, partial trip.  Inputs sit between NaN, outputs inside a sentinel."""
import numpy as np
import pytest
import torch

from oracle import keras_ref as K

pytestmark = pytest.mark.gpu

TRIP = 2048 * 256          # units one trip of the grid covers (common.h stream_grid)
GUARD = 8                  # floats on each side of a view; the view starts `off` floats past a 16-byte boundary
SENTINEL = -12345.5


def dev():
    return torch.device('cuda:0')


def view(n, off, fill):
    """(buffer, its n-float view starting GUARD + off floats in): torch allocations are 256-byte aligned, GUARD is two 16-byte units"""
    buf = torch.full((n + 2 * GUARD + off,), fill, dtype=torch.float32, device=dev())
    v = buf[GUARD + off:GUARD + off + n]
    assert buf.data_ptr() % 16 == 0 and v.data_ptr() % 16 == 4 * off
    return buf, v


def untouched(buf, n, off):
    edges = torch.cat([buf[:GUARD + off], buf[GUARD + off + n:]])
    return bool((edges == SENTINEL).all())


def rows_for(C, off, size):
    if size == 'small':
        return 2, 5
    units = C // 4 if (C % 4 == 0 and off == 0) else C       # per row
    L = -(-(TRIP + 3 * 256 + 77) // (7 * units))              # a full trip, three more blocks and a ragged one
    return 7, L


@pytest.mark.parametrize('size', ['small', 'two_trips'])
@pytest.mark.parametrize('off', [0, 1])
@pytest.mark.parametrize('C', [1, 3, 4, 5, 8, 17])
def test_upsample2_any_channel_count_against_keras_ref(C, off, size):
    from gennet_amd import _lib, ops
    B, L = rows_for(C, off, size)
    if size == 'two_trips':
        assert B * L * (C // 4 if (C % 4 == 0 and off == 0) else C) > TRIP
    rng = np.random.RandomState(C * 10 + off)
    x = rng.randn(B, L, C).astype(np.float32)
    dy = rng.randn(B, 2 * L, C).astype(np.float32)
    n = x.size
    st = ops._stream
    # forward: every output element one input element, bit for bit
    xb, xv = view(n, off, float('nan')); xv.copy_(torch.from_numpy(x.ravel()).to(dev()))
    yb, yv = view(2 * n, off, SENTINEL)
    _lib.call('gn_upsample2_fwd', xv.data_ptr(), yv.data_ptr(), B, L, C, st())
    y = yv.cpu().numpy().reshape(B, 2 * L, C)
    assert untouched(yb, 2 * n, off), 'forward wrote outside its output'
    assert np.array_equal(y, K.upsample1d_fwd(x))
    # backward: a + b rounded once
    db, dv = view(2 * n, off, float('nan')); dv.copy_(torch.from_numpy(dy.ravel()).to(dev()))
    gb, gv = view(n, off, SENTINEL)
    _lib.call('gn_upsample2_bwd', dv.data_ptr(), gv.data_ptr(), B, L, C, st())
    dx = gv.cpu().numpy().reshape(B, L, C).astype(np.float64)
    assert untouched(gb, n, off), 'backward wrote outside its output'
    ref = K.upsample1d_bwd(dy.astype(np.float64))
    assert np.all(np.abs(dx - ref) <= 2.0 ** -24 * np.abs(ref))
    # a mixed pair (input off a 16-byte boundary, output on one) takes the one-float units too
    if off == 1 and size == 'small':
        yb2, yv2 = view(2 * n, 0, SENTINEL)
        _lib.call('gn_upsample2_fwd', xv.data_ptr(), yv2.data_ptr(), B, L, C, st())
        assert untouched(yb2, 2 * n, 0) and np.array_equal(yv2.cpu().numpy().reshape(B, 2 * L, C), K.upsample1d_fwd(x))
    # the wrappers allocate their outputs: same values
    if off == 0:
        assert torch.equal(ops.upsample2_fwd(xv.view(B, L, C)).reshape(-1), yv)
        assert torch.equal(ops.upsample2_bwd(dv.view(B, 2 * L, C)).reshape(-1), gv)
    torch.cuda.synchronize()
