"""The data gradient of a conv with fewer taps than its stride (Conv1D(kernel_size=1, strides=2), the width-2 Conv2D with kernel (1, 5) and
strides (2, 1)): the input rows no tap reaches have a zero gradient.  gn_conv1d_dgrad clears dx and runs the phases that have taps; against the
fp64 definition of tests/test_conv_anyc_gpu.py on guarded buffers, 2e-5 of the largest reference value (that file's bound), exact zeros in the
rows without taps, on every kernel family such a shape reaches: direct, small-Cin (any stride), small-Cout and any-channel."""
import numpy as np
import pytest
import torch

import test_conv_anyc_gpu as A

pytestmark = pytest.mark.gpu

CASES = [
    # B, L, Cin, Cout, k, stride, padding
    (2, 11, 8, 16, 1, 2, 'same'),           # direct
    (3, 24, 2, 16, 1, 2, 'same'),           # the folded Conv2D((1, 5), strides (2, 1)) on one channel: small-Cin
    (2, 13, 2, 8, 2, 3, 'same'),            # small-Cin at stride 3: one phase of three without a tap
    (2, 12, 16, 2, 1, 2, 'valid'),          # small-Cout
    (2, 10, 6, 10, 1, 2, 'valid'),          # any-channel
    (1, 1, 8, 8, 1, 2, 'same'),             # a single row: only phase 0 exists
]


@pytest.mark.parametrize('B,L,Cin,Cout,k,s,padding', CASES, ids=['-'.join(str(v) for v in c) for c in CASES])
def test_data_gradient_with_fewer_taps_than_the_stride(B, L, Cin, Cout, k, s, padding):
    from gennet_amd import _lib, ops
    rng = np.random.RandomState(L * 100 + Cin + Cout)
    Lout, pl = A.geometry(L, k, s, padding)
    w = (rng.randn(k, Cin, Cout) / np.sqrt(k * Cin)).astype(np.float32).astype(np.float64)
    dy = rng.randn(B, Lout, Cout).astype(np.float32).astype(np.float64)
    DY, WT = A.Guarded(dy.shape, dy), A.Guarded((k, Cout, Cin), np.ascontiguousarray(w.transpose(0, 2, 1)))
    DX = A.Guarded((B, L, Cin))
    if ops.conv_needs_any(Cout, Cin):
        _lib.call('gn_conv1d_dgrad_any', DY.t.data_ptr(), WT.t.data_ptr(), DX.t.data_ptr(), B, L, Cin, Cout, k, s, pl, Lout, ops._stream())
    else:
        _lib.call('gn_conv1d_dgrad', DY.t.data_ptr(), WT.t.data_ptr(), DX.t.data_ptr(), B, L, Cin, Cout, k, s, pl, Lout, ops._stream())
    dx = DX.check('data gradient')
    ref = A.ref_dgrad(dy, w, L, s, pl)
    untouched = np.ones(L, bool)
    for j in range(k):
        untouched[[t for t in (s * np.arange(Lout) + j - pl) if 0 <= t < L]] = False
    assert untouched.any() or L == 1
    assert not dx[:, untouched].any() and not ref[:, untouched].any()
    assert A.rel(dx, ref) < 2e-5
    torch.cuda.synchronize()
