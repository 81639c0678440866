"""Which convolution kernel family a call reached, read from the library's launch counters (ops.prof_*).

Family names are those of the selection table in csrc/capi.hip above select_conv.  Counter kinds (csrc/common.h, prof_end): 0 direct conv
(forward, data gradient), 1 direct weight gradient, 2 bf16x3, 5 / 6 transform-domain F(2,5) conv / weight gradient, 7 / 8 transform-domain
stride-2 conv / weight gradient.  'small' is a call that launched none of these kinds AND at least one of SMALL_KINDS, the kernels of
csrc/small_conv.hip: 11 conv_smallcin, 12 conv_smallcout, 13 conv_cout1_rows, 14 wgrad_smallcin_tab, 15 wgrad_small (small Cout, stride > 1),
16 wgrad_smallcout_s1, 17 level 1 of the two-level partial-slab reduce (small_launches).
The data gradient of a strided layer is 'merged' (both phases in one direct launch), 'phases' (one direct launch per phase) or 'wino_s2'.
"""
MATHS = ('fp32', 'wino')
KINDS = (0, 1, 2, 5, 6, 7, 8)
SMALL_KINDS = (11, 12, 13, 14, 15, 16, 17)

_FAMILIES = {
    'fwd': {'direct': {0: 1}, 'wino': {5: 1}, 'wino_s2': {7: 1}, 'bf16x3': {2: 1}, 'small': {}},
    'dgrad': {'direct': {0: 1}, 'wino': {5: 1}, 'wino_s2': {7: 1}, 'bf16x3': {2: 1}, 'small': {}, 'merged': {0: 1}, 'phases': None},
    'wgrad': {'direct': {1: 1}, 'wino': {6: 1}, 'wino_s2': {8: 1}, 'bf16x3': {2: 1}, 'small': {}},
}


def expected(direction, family, stride=1):
    """{kind: launches} over KINDS that `family` produces for one call in `direction` ('fwd', 'dgrad', 'wgrad') of a layer of `stride`."""
    fams = _FAMILIES[direction]
    assert family in fams, 'no family %r for %s (one of %s)' % (family, direction, sorted(fams))
    if direction == 'dgrad' and family in ('direct', 'merged', 'phases'):
        # a strided data gradient on the direct kernels is merged or in phases, a unit-stride one is one plain launch
        assert (stride == 1) == (family == 'direct'), 'dgrad family %r at stride %d' % (family, stride)
    want = {0: stride} if family == 'phases' else fams[family]
    return {k: want.get(k, 0) for k in KINDS}


def launches(fn):
    """(fn(), {kind: launches} over KINDS): fn runs with profiling on and the counters emptied first; the previous profiling state is restored."""
    return _counted(fn, KINDS, drop_zeros=False)


def small_launches(fn):
    """(fn(), {kind: launches} over SMALL_KINDS and KINDS with the zero counts left out, e.g. {14: 1, 17: 1}), run as in launches()."""
    return _counted(fn, SMALL_KINDS + KINDS, drop_zeros=True)


def _counted(fn, kinds, drop_zeros):
    from gennet_amd import ops
    was = ops.prof_enabled()
    ops.prof_enable(True)
    try:
        ops.prof_reset()
        out = fn()
        counts = {k: ops.prof_collect(k)['launches'] for k in kinds}
    finally:
        ops.prof_enable(was)
    return out, {k: v for k, v in counts.items() if v or not drop_zeros}


def run(direction, family, fn, stride=1):
    """fn() -- one forward, data-gradient or weight-gradient call -- asserted to have reached `family`; returns what fn returned."""
    out, got = _counted(fn, KINDS + SMALL_KINDS, drop_zeros=False)
    small = {k: got.pop(k) for k in SMALL_KINDS}
    want = expected(direction, family, stride)
    assert got == want, '%s: family %r expected (launches %s), got %s' % (direction, family, want, got)
    if family == 'small':
        assert sum(small.values()) >= 1, '%s: family small expected, but no small-channel kernel was launched (%s)' % (direction, small)
    return out


def families(spec):
    """'fwd dgrad wgrad' family names of a case table -> (fwd, dgrad, wgrad)."""
    f = tuple(spec.split())
    assert len(f) == 3, spec
    return f


def per_math(cases, shape_cols):
    """pytest.param of every case under each of MATHS, the maths of one case next to each other (so that OneCase computes its oracle once),
    the math as the last argument.  Ids: the case's shape columns under 'fp32' (the plain id the case has always had), shape-wino under 'wino'."""
    import pytest
    out = []
    for c in cases:
        sid = '-'.join(str(v) for v in c[:shape_cols])
        out += [pytest.param(*c, m, id=sid if m == 'fp32' else '%s-%s' % (sid, m)) for m in MATHS]
    return out


class OneCase:
    """The oracle of the last case asked for: parametrized over the maths, consecutive tests of one case share it (computed once)."""

    def __init__(self):
        self.key, self.val = None, None

    def get(self, key, make):
        if key != self.key:
            self.key, self.val = None, None          # drop the previous case's arrays before the next are made
            self.val = make()
            self.key = key
        return self.val
