"""CPU-only checks of the ctypes binding that gennet_amd/_lib.py derives from include/gennet_hip.h: signatures pinned against a hand-written
table, the reader's refusals, the arity of every call site, the enum codes ops takes from the header, and the tap-group rule the library owns."""
import ast
import os

import pytest

from gennet_amd import _lib, ops
from gennet_amd._lib import f32, f64, i32, i64, sz, u64, vp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# hand-typed, as the binding was before it was derived: every scalar type of the header, the shortest and the longest parameter list
PINNED = {
    'gn_loss_pass': (i32, [i32, vp, vp, vp, vp, i64, i32, f64, vp, sz, vp]),
    'gn_bias_grad': (i32, [vp, vp, vp, sz, sz, i32, vp]),
    'gn_dropout_mask': (i32, [vp, sz, f32, u64, u64, vp]),
    'gn_prof_reset': (i32, []),
    'gn_synth_templates_noise': (i32, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, f64, f64, f64, f64, f64, f64, f64, f64,
                                       u64, u64, i32, i32, f64, f64, u64, u64, vp, vp]),
    'gn_conv1d_wino_workspace': (sz, [i32, i32]),
    'gn_last_error': (_lib.C.c_char_p, []),
}


def test_derived_signatures_equal_the_pinned_ones():
    assert len(PINNED['gn_synth_templates_noise'][1]) == 37
    for name, (restype, argtypes) in PINNED.items():
        assert _lib.DECLS[name][0] is restype, name
        assert _lib.DECLS[name][1] == argtypes, name
    assert (i32, i64, f32, f64, u64, sz, vp) == (_lib.C.c_int, _lib.C.c_longlong, _lib.C.c_float, _lib.C.c_double, _lib.C.c_uint64, _lib.C.c_size_t,
                                                 _lib.C.c_void_p)


def test_loaded_library_carries_the_derived_types():
    L = _lib.lib()
    for name, (restype, argtypes) in _lib.DECLS.items():
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    assert L.gn_version() >= 100 and isinstance(L.gn_last_error(), bytes)


def test_reader_takes_the_headers_forms():
    fns, consts = _lib.read_header('/* int gn_no(int a); */\n#define GN_A (-4) /* why */\n#define GN_GUARD\nenum gn_e { GN_E_X = 0,\n GN_E_Y = 7 };\n'
                                   'size_t gn_a( void ); // int gn_nor(int a);\nint gn_b();\nconst char * gn_c(const float* x,\n    long long rows, const  double s,'
                                   ' uint64_t seed);\n#ifdef __cplusplus\n}\n#endif\n')
    assert fns == {'gn_a': (sz, []), 'gn_b': (i32, []), 'gn_c': (_lib.C.c_char_p, [vp, i64, f64, u64])}
    assert consts == {'GN_A': -4, 'GN_E_X': 0, 'GN_E_Y': 7}


@pytest.mark.parametrize('text', ['int gn_a(short n, void* stream);',                                  # a type the header does not use
                                  'int gn_a(struct gn_cfg cfg, void* stream);',                        # a struct passed by value
                                  'int gn_a(int x)\nint gn_b(int y);',                                 # a declaration without its ;
                                  'int gn_a(int x);\nint gn_b(int y)',                                 # ... at the end of the text
                                  'long gn_a(void);',                                                  # a return type the header does not use
                                  'int gn_a(int);',                                                    # a parameter without a name
                                  'enum gn_e { GN_E_X, GN_E_Y };'])                                    # an enum member without a value
def test_reader_refuses_what_it_does_not_know(text):
    with pytest.raises(_lib.GennetHipError) as e:
        _lib.read_header('int gn_fine(const float* x, size_t n, void* stream);\n' + text)
    assert 'gn_' in str(e.value)                                                                        # the declaration is named


def test_call_size_and_predicate_refuse_the_wrong_kind():
    for through, name in ((_lib.call, 'gn_conv1d_wino_workspace'), (_lib.predicate, 'gn_conv1d_wino_workspace'),      # size_t, not an error code
                          (_lib.size, 'gn_conv1d_needs_any'),                                                          # int, not size_t
                          (_lib.call, 'gn_last_error'), (_lib.size, 'gn_no_such_entry_point')):
        with pytest.raises(_lib.GennetHipError) as e:
            through(name, 8, 64)
        assert name in str(e.value)
    assert _lib.size('gn_conv1d_wino_workspace', 8, 64) > 0 and _lib.predicate('gn_conv1d_needs_any', 8, 64) is False


def _call_sites():
    """(file, enclosing function, kind, name expression, positional arguments) of every _lib.call / _lib.size / _lib.predicate in the tree."""
    files = [os.path.join(ROOT, f) for f in ('bench.py', '__graft_entry__.py')]
    for top in ('gennet_amd', 'scripts', 'tests'):
        for dirpath, _, names in os.walk(os.path.join(ROOT, top)):
            files += [os.path.join(dirpath, n) for n in names if n.endswith('.py')]
    sites = []

    def walk(node, fn, rel):
        if isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef)):
            fn = node.name
        if (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr in ('call', 'size', 'predicate')
                and isinstance(node.func.value, ast.Name) and node.func.value.id == '_lib'):
            sites.append((rel, fn, node.func.attr, node.args[0], node.args[1:], node.lineno))
        for child in ast.iter_child_nodes(node):
            walk(child, fn, rel)

    for path in sorted(files):
        with open(path) as f:
            walk(ast.parse(f.read(), path), None, os.path.relpath(path, ROOT).replace(os.sep, '/'))
    return sites


def _literal_names(expr):
    """The function names a call site can reach: a string constant, or a conditional expression of two; None when it is computed."""
    if isinstance(expr, ast.Constant) and isinstance(expr.value, str):
        return [expr.value]
    if isinstance(expr, ast.IfExp) and all(isinstance(e, ast.Constant) and isinstance(e.value, str) for e in (expr.body, expr.orelse)):
        return [expr.body.value, expr.orelse.value]
    return None


def test_every_call_site_passes_the_declared_number_of_arguments():
    """A call with a missing or an extra argument hands the kernel garbage, and only a GPU run would show it: so every call site whose function name
    can be read off the source is counted against the header here.  The four sites that compute the name or unpack their arguments are pinned
    by file and enclosing function (ops.loss the only one outside tests/); a new one fails this test."""
    kinds = {'call': i32, 'predicate': i32, 'size': sz}
    resolved, unresolved, wrong = 0, [], []
    for rel, fn, kind, expr, args, line in _call_sites():
        names = _literal_names(expr)
        if names is None or any(isinstance(a, ast.Starred) for a in args):
            unresolved.append((rel, fn))
            continue
        resolved += 1
        for name in names:
            restype, argtypes = _lib.DECLS.get(name, (None, None))
            if restype is not kinds[kind] or len(args) != len(argtypes):
                wrong.append('%s:%d %s(%r) passes %d arguments' % (rel, line, kind, name, len(args)))
    assert not wrong, wrong
    wino = ('tests/test_wino_gpu.py', 'test_a_weight_gradient_workspace_too_small_for_its_kernel_is_an_error')       # twice: a literal name, *args
    assert sorted(unresolved) == sorted([('gennet_amd/ops.py', 'loss'), ('tests/test_noise_layers_gpu.py', '_call'), wino, wino]), unresolved
    assert resolved >= 149, resolved


def test_ops_take_the_enum_codes_from_the_header():
    assert ops.ACT == {'linear': 0, None: 0, 'relu': 1, 'relu_max': 2, 'leaky': 3, 'tanh': 4, 'sigmoid': 5}
    assert ops.LOSS_KINDS == {'binary_crossentropy': 0, 'mean_squared_error': 1, 'mean_absolute_error': 2, 'mean_absolute_percentage_error': 3,
                              'mean_squared_logarithmic_error': 4, 'hinge': 5, 'squared_hinge': 6, 'logcosh': 7, 'poisson': 8,
                              'kullback_leibler_divergence': 9, 'categorical_crossentropy': 10, 'cosine_proximity': 11, 'categorical_accuracy': 12}
    assert list(ops.LOSS_KINDS.values()) == list(range(13))                    # engine.LOSSES keeps the enum's order
    assert ops.OPT_RULES == {'sgd': 0, 'rmsprop': 1, 'adagrad': 2, 'adadelta': 3, 'adamax': 4, 'adam': 5, 'amsgrad': 6}
    assert (_lib.GN_OK, _lib.GN_EINVAL, _lib.GN_ELAUNCH, _lib.GN_EWORKSPACE) == (0, -1, -2, -3)


def test_tap_groups_is_the_librarys_rule():
    for k in range(1, 41):
        G = (k + 4) // 5
        assert ops.tap_groups(k) == (G, -(-k // G)), k
    assert ops.tap_groups.cache_info().currsize >= 40
    with pytest.raises(_lib.GennetHipError):
        ops.tap_groups(0)
