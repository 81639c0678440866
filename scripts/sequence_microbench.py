#!/usr/bin/env python
"""Time the four passes of csrc/sequence.hip against a device-to-device copy of the same bytes:
  * permute   (B, L, C) -> (B, C, L), the tiled transposition: reads and writes B L C floats;
  * repeat    (B, C) -> (B, n, C) forward and its backward, the fp64 sum over n: B C + B n C floats either way;
  * pad       (B, L, C) -> (B, l + L + r, C), gn_shift1d: B L C floats read, B (l + L + r) C written.
The bytes are those the algorithm needs, every operand once, computed from the shape; the copy moves the same number of bytes (half read, half
written) in the same process.  Every result is first held against torch.  A sample is REPS launches between two device events (one launch of
these shapes lasts microseconds), kernel and copy samples alternate, 3 warm-up samples, then the median of 11; each case runs in a child
process under a time limit, and one JSON line a case is printed at the end.
  python scripts/sequence_microbench.py                 # permute 64 256 128, repeat 64 256 128, pad 64 2048 64 3 3, and the large permute 64 4096 256
  python scripts/sequence_microbench.py permute B L C | repeat B n C | pad B L C left right"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [('permute', 64, 256, 128), ('repeat', 64, 256, 128), ('pad', 64, 2048, 64, 3, 3), ('permute', 64, 4096, 256)]
ARITY = {'permute': 3, 'repeat': 3, 'pad': 5}
WARMUP, SAMPLES, REPS, TIMEOUT_S = 3, 11, 50, 240


def sample_ms(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / REPS


def median_pair_ms(fn, copy):
    """medians of alternating samples of the pass and of the copy"""
    import torch
    for _ in range(WARMUP):
        sample_ms(fn)
        sample_ms(copy)
    torch.cuda.synchronize()
    a, b = [], []
    for _ in range(SAMPLES):
        a.append(sample_ms(fn))
        b.append(sample_ms(copy))
    return sorted(a)[SAMPLES // 2], sorted(b)[SAMPLES // 2]


def one(kind, *s):
    import torch
    import torch.nn.functional as F
    sys.path.insert(0, ROOT)
    from gennet_amd import ops
    from gennet_amd.engine import device
    dev = device()
    g = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *shape: torch.randn(*shape, device=dev, generator=g)          # noqa: E731
    runs = []                # (name, the pass, floats moved)
    if kind == 'permute':
        B, L, C = s
        x, y = rnd(B, L, C), torch.empty((B, C, L), device=dev)
        assert torch.equal(ops.permute(x, (0, 2, 1)), x.permute(0, 2, 1).contiguous())
        runs.append(('permute', lambda: ops.permute(x, (0, 2, 1), out=y), 2 * B * L * C))
    elif kind == 'repeat':
        B, n, C = s
        x, y, dx = rnd(B, C), torch.empty((B, n, C), device=dev), torch.empty((B, C), device=dev)
        dy = rnd(B, n, C)
        assert torch.equal(ops.repeat_fwd(x, n), x[:, None, :].expand(B, n, C).contiguous())
        ref = dy.double().sum(1)
        assert float((ops.repeat_bwd(dy).double() - ref).abs().max()) <= 2.0 ** -23 * float(ref.abs().max())
        runs.append(('repeat_fwd', lambda: ops.repeat_fwd(x, n, out=y), B * C + B * n * C))
        runs.append(('repeat_bwd', lambda: ops.repeat_bwd(dy, out=dx), B * C + B * n * C))
    else:
        B, L, C, left, right = s
        x, y = rnd(B, L, C), torch.empty((B, left + L + right, C), device=dev)
        assert torch.equal(ops.shift1d(x, left, left + L + right), F.pad(x, (0, 0, left, right)))
        runs.append(('pad', lambda: ops.shift1d(x, left, left + L + right, out=y), B * L * C + B * (left + L + right) * C))
    print('%s %s' % (kind, ' '.join(str(v) for v in s)), flush=True)
    for name, fn, floats in runs:
        nbytes = 4 * floats
        src = torch.empty(nbytes // 8, dtype=torch.float32, device=dev).normal_()
        dst = torch.empty_like(src)
        ms, copy_ms = median_pair_ms(fn, lambda: dst.copy_(src))
        row = {'case': [kind] + list(s), 'pass': name, 'ms': ms, 'bytes': nbytes, 'TBps': nbytes / ms * 1e-9, 'copy_ms': copy_ms,
               'copy_TBps': nbytes / copy_ms * 1e-9, 'pass_over_copy': ms / copy_ms}
        print('  %-10s %9.4f ms  %8.2f MB needed  %6.2f TB/s;  a copy of the same bytes %9.4f ms  %6.2f TB/s  (pass / copy %.2f)'
              % (name, ms, nbytes * 1e-6, row['TBps'], copy_ms, row['copy_TBps'], ms / copy_ms), flush=True)
        print(json.dumps(row), flush=True)
        del src, dst


def main():
    args = sys.argv[1:]
    if args and args[0] == '--one':
        return one(args[1], *[int(v) for v in args[2:]])
    if args:
        if args[0] not in ARITY or len(args) != 1 + ARITY[args[0]]:
            sys.exit(__doc__)
        cases = [(args[0],) + tuple(int(v) for v in args[1:])]
    else:
        cases = CASES
    for c in cases:
        try:          # a fresh child per case under a time limit; after a run that hangs or fails nothing more is started
            r = subprocess.run([sys.executable, os.path.abspath(__file__), '--one'] + [str(v) for v in c], timeout=TIMEOUT_S)
        except subprocess.TimeoutExpired:
            print('case %r: no result within %d s' % (c, TIMEOUT_S), flush=True)
            return 1
        if r.returncode:
            print('case %r: exit status %d' % (c, r.returncode), flush=True)
            return r.returncode
    return 0


if __name__ == '__main__':
    sys.exit(main())
