"""ctypes binding of libgennet_hip.so, derived from the one declaration of its C ABI: include/gennet_hip.h.

The HIP library is the product path: if it is missing this module raises at import of the first op -- there is
no CPU / eager-PyTorch fallback anywhere in gennet_amd.
"""
import ctypes as C
import os
import re

from . import build

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'lib', 'libgennet_hip.so')

_lib = None

vp, i32, i64, f32, f64, u64, sz = C.c_void_p, C.c_int, C.c_longlong, C.c_float, C.c_double, C.c_uint64, C.c_size_t

_ARG_TYPES = {'int': i32, 'float': f32, 'double': f64, 'size_t': sz, 'uint64_t': u64, 'long long': i64, '*': vp}      # '*': any pointer
_RETURN_TYPES = {'int': i32, 'size_t': sz, 'const char*': C.c_char_p}


class GennetHipError(RuntimeError):
    pass


def read_header(text):
    """({name: (restype, [argtypes])}, {constant: int}) of the text of gennet_hip.h: its `gn_*` declarations as ctypes, its integer
    #defines and its enum members.  A reader for the vocabulary of that header, not a C parser: a type it does not know, or a statement it
    cannot split, raises GennetHipError naming the declaration."""
    text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', text, flags=re.S)
    consts = dict((k, int(v)) for k, v in re.findall(r'^[ \t]*#[ \t]*define[ \t]+(GN_\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$', text, re.M))
    text = re.sub(r'^[ \t]*#.*$', ' ', text, flags=re.M)
    text = re.sub(r'\}\s*$', '', re.sub(r'extern\s+"C"\s*\{', ' ', text))           # the extern "C" { } around the declarations
    fns = {}
    *statements, rest = text.split(';')
    if rest.strip():
        raise GennetHipError('gennet_hip.h: no ; after %r' % ' '.join(rest.split()))
    for s in statements:
        s = ' '.join(s.split())
        enum = re.fullmatch(r'enum \w+ ?\{([^{}]*)\}', s)
        if enum:
            for member in enum.group(1).split(','):
                m = re.fullmatch(r'\s*(GN_\w+) = (-?\d+)\s*', member)
                if not m:
                    raise GennetHipError('gennet_hip.h: enum member %r of %r has no integer value' % (member.strip(), s))
                consts[m.group(1)] = int(m.group(2))
            continue
        decl = re.fullmatch(r'([^()]+?) ?\b(gn_\w+) ?\(([^()]*)\)', s)
        if not decl:
            raise GennetHipError('gennet_hip.h: cannot read the declaration %r' % s)
        ret, name, params = decl.groups()
        ret = re.sub(r' ?\* ?', '*', ret)
        args = []
        for p in ([] if params.strip() in ('', 'void') else params.split(',')):
            base = '*' if '*' in p else ' '.join(w for w in p.split()[:-1] if w != 'const')      # the last word is the parameter's name
            if base not in _ARG_TYPES:
                raise GennetHipError('gennet_hip.h: unknown parameter type %r in %r' % (p.strip(), s))
            args.append(_ARG_TYPES[base])
        if ret not in _RETURN_TYPES:
            raise GennetHipError('gennet_hip.h: unknown return type %r in %r' % (ret, s))
        fns[name] = (_RETURN_TYPES[ret], args)
    return fns, consts


with open(build.HEADER) as _f:
    DECLS, CONSTS = read_header(_f.read())
GN_OK, GN_EINVAL, GN_ELAUNCH, GN_EWORKSPACE = (CONSTS[_k] for _k in ('GN_OK', 'GN_EINVAL', 'GN_ELAUNCH', 'GN_EWORKSPACE'))


def enum_members(prefix):
    """{lower-cased suffix: value} of the header's constants that start with `prefix`, in the header's order."""
    return dict((k[len(prefix):].lower(), v) for k, v in CONSTS.items() if k.startswith(prefix))


def lib():
    """The loaded library.  Raises (loudly) when the .so has not been built: run `python -m gennet_amd.build`."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            try:                            # a fresh checkout on a box that has hipcc: compile the kernels (~30 s), nothing else
                build.build(verbose=False)
            except Exception as e:          # noqa: BLE001
                raise GennetHipError('%s not found and building it failed (%s): run `python -m gennet_amd.build` '
                                     '(hipcc --offload-arch=gfx950); gennet_amd has no CPU fallback' % (LIB_PATH, e))
        # torch ships its own libamdhip64; it must be the HIP runtime of the process (device pointers and streams come from
        # torch), so torch is imported BEFORE this library is dlopen-ed and the library's NEEDED libamdhip64 resolves to the
        # already-loaded copy.  Loading in the other order gives the process two HIP runtimes and launches fail.
        import torch  # noqa: F401
        L = C.CDLL(LIB_PATH)
        for name, (restype, argtypes) in DECLS.items():
            try:
                fn = getattr(L, name)
            except AttributeError:          # reported by call() / size() / predicate() and by tests/test_host_cpu.py
                continue
            fn.argtypes = argtypes
            fn.restype = restype
        _lib = L
    return _lib


def exported_symbols():
    return sorted(DECLS)


def _fn(name, restype):
    """The bound function `name`, which the header must declare as returning `restype`."""
    if DECLS.get(name, (None,))[0] is not restype:
        raise GennetHipError('%s is not declared in %s as returning %s' % (name, os.path.basename(build.HEADER), restype.__name__))
    try:
        return getattr(lib(), name)
    except AttributeError:
        raise GennetHipError('%s is not exported by %s (stale build?)' % (name, LIB_PATH))


def call(name, *args):
    rc = _fn(name, i32)(*args)
    if rc != 0:
        raise GennetHipError('%s failed (%d): %s' % (name, rc, lib().gn_last_error().decode()))


def size(name, *args):
    return int(_fn(name, sz)(*args))


def predicate(name, *args):
    return bool(_fn(name, i32)(*args))
