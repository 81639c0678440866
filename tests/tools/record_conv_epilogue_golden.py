"""Records tests/golden/conv_epilogue_parent.npz: the outputs of every case of tests/conv_epilogue_cases.py as the library of THIS tree computes
them on the GPU -- per case the SHA-256 of the output bytes, the first 256 output values (diagnostics) and the launches per counted kernel kind.
tests/test_conv_epilogue_gpu.py recomputes every case and requires equal digests.

    python tests/tools/record_conv_epilogue_golden.py <commit hash of this tree> [out.npz]

The fixture is the yardstick of the 16-byte epilogue of conv_wino_kernel / conv_wino_s2_kernel, which must not change one output bit: it was
recorded from a build of the commit BEFORE that change (its hash is in the file), with this script and the case table copied into a checkout of
it.  Run it again only from a commit whose outputs are the intended ones, never to make a failing comparison pass.
"""
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
OUT = os.path.join(ROOT, 'tests', 'golden', 'conv_epilogue_parent.npz')


def main():
    import torch
    import conv_epilogue_cases as C
    import conv_family as CF
    from gennet_amd import ops
    commit = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else OUT
    dev = torch.device('cuda:0')
    ids, shas, heads, counts = [], [], [], []
    with ops.conv_math('wino'):
        for case in C.cases():
            d = C.inputs(case)
            outs, got = CF.launches(lambda: C.run(case, d, dev))
            direction, fam, stride = C.family(case)
            want = CF.expected(direction, fam, stride)
            if got != want:
                print('NOTE %s: launches %s, the table expects %s (%s)' % (C.case_id(case), got, want, fam))
            sha, head = C.digest(outs)
            ids.append(C.case_id(case)); shas.append(sha); heads.append(head); counts.append([got[k] for k in CF.KINDS])
    np.savez_compressed(out, commit=np.array(commit), ids=np.array(ids), sha256=np.array(shas), head=np.stack(heads),
                        kinds=np.array(CF.KINDS), launches=np.array(counts, np.int32))
    print('%d cases of commit %s -> %s (%d bytes)' % (len(ids), commit, out, os.path.getsize(out)))


if __name__ == '__main__':
    main()
