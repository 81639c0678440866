"""The epilogues of the transform-domain conv kernels (csrc/conv_wino.hip, csrc/conv_wino_s2.hip) write 16 bytes per lane through LDS
(csrc/conv_epilogue.h: tile16_wide_epilogue) where they wrote one dword: a change that may not move one output bit or one address.

The reference is NOT the code under test: tests/golden/conv_epilogue_parent.npz holds, for every case of tests/conv_epilogue_cases.py, the SHA-256
of the output bytes as the commit before the change computed them (tests/tools/record_conv_epilogue_golden.py, run on a build of that commit; its
hash is in the file).  Every case is recomputed here and must give the same digest -- which also covers the set of addresses written, since the
outputs are whole tensors -- and must reach the kernel family the table names, with the launch counts the parent had.

A base address off the 16-byte grid (gy) or off the 4-byte grid (keep-mask) takes the per-element epilogue: the same bits again.
"""
import os

import numpy as np
import pytest

import conv_epilogue_cases as C
import conv_family as CF

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'conv_epilogue_parent.npz')
CASES = C.cases()


@pytest.fixture(scope='module')
def golden():
    z = np.load(GOLDEN)
    return {'commit': str(z['commit']), 'kinds': [int(k) for k in z['kinds']],
            'cases': {str(i): (str(s), h, [int(n) for n in l]) for i, s, h, l in zip(z['ids'], z['sha256'], z['head'], z['launches'])}}


def test_the_fixture_holds_exactly_the_case_table(golden):
    assert os.path.getsize(GOLDEN) < 256 * 1024
    assert len(golden['commit']) == 40 and int(golden['commit'], 16) >= 0
    assert sorted(golden['cases']) == sorted(C.case_id(c) for c in CASES) and len(golden['cases']) == len(CASES)
    assert tuple(golden['kinds']) == CF.KINDS
    seen = {(c[0], C.family(c)[1]) for c in CASES}
    assert {('fwd', 'wino'), ('fwd', 'wino_s2'), ('dgrad', 'wino'), ('dgrad', 'wino_s2'), ('fwd_wino', 'wino'), ('fwd_dropout', 'wino'),
            ('fwd_dropout', 'wino_s2'), ('fwd_stats', 'wino'), ('fwd_stats', 'wino_s2')} <= seen


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES, ids=C.case_id)
def test_outputs_equal_the_parent_commit_bit_for_bit(case, golden):
    import torch
    from gennet_amd import ops
    sha, head, counts = golden['cases'][C.case_id(case)]
    d = C.inputs(case)
    direction, fam, stride = C.family(case)
    with ops.conv_math('wino'):
        outs = CF.run(direction, fam, lambda: C.run(case, d, torch.device('cuda:0')), stride)          # asserts the family reached
        _, got = CF.launches(lambda: C.run(case, d, torch.device('cuda:0')))
    assert [got[k] for k in CF.KINDS] == counts, 'launches per kind %s, the parent %s launched %s' % (got, golden['commit'][:7], counts)
    got_sha, got_head = C.digest(outs)
    differ = np.flatnonzero(got_head.view(np.uint32) != head.view(np.uint32))
    assert got_sha == sha, 'outputs differ from commit %s; of the first %d values %d differ, first at %s: %s against %s' % (
        golden['commit'][:7], C.HEAD, differ.size, differ[:1], got_head[differ[:4]], head[differ[:4]])


FALLBACK_CASES = [
    # (case, the input moved off the grid, elements of offset): gy one float (4 bytes) off, the keep-mask one byte off
    (('dgrad', 's1same', 56, 128, 'relu'), 'y_prev', 1),                 # conv_wino_kernel, mode 2
    (('dgrad', 's2same', 56, 128, 'leaky_dropout'), 'y_prev', 1),        # conv_wino_s2_kernel KIND 2, mode 3
    (('dgrad', 's2valid', 48, 64, 'leaky_dropout'), 'mask', 1),          # ... the other row offset, the mask off the grid
    (('fwd_dropout', 's1valid', 48, 128, 'leaky'), 'mask', 3),           # conv_wino_kernel, mode 1
    (('fwd_dropout', 's2same', 56, 64, 'sigmoid'), 'mask', 2),           # conv_wino_s2_kernel KIND 1, mode 1, runtime-switch activation
]


@pytest.mark.gpu
@pytest.mark.parametrize('case,moved,offset', FALLBACK_CASES, ids=lambda v: C.case_id(v) if isinstance(v, tuple) else str(v))
def test_a_misaligned_operand_takes_the_per_element_epilogue_with_the_same_bits(case, moved, offset, golden):
    import torch
    from gennet_amd import ops
    assert case in CASES
    dev = torch.device('cuda:0')
    d = C.inputs(case)
    held = []

    def place(name, t):
        if name != moved:
            return t
        buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=dev)              # allocations start on a 512-byte boundary
        view = buf[offset:offset + t.numel()].view(t.shape)
        view.copy_(t)
        assert view.data_ptr() % (16 if t.dtype == torch.float32 else 4) != 0 and view.is_contiguous()
        held.append(buf)
        return view

    direction, fam, stride = C.family(case)
    with ops.conv_math('wino'):
        outs = CF.run(direction, fam, lambda: C.run(case, d, dev, place), stride)
    assert held, 'the operand was not moved'
    assert C.digest(outs)[0] == golden['cases'][C.case_id(case)][0]
