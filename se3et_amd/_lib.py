"""ctypes binding of libse3et_hip.so (C ABI declared in include/se3et_hip.h).

There is deliberately no fallback: if the library is missing or a kernel reports an error the caller gets a
RuntimeError -- the product never computes a hot-path op on the CPU or through eager PyTorch."""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
# (SE3_LIB: another build of the same library, for A/B runs of two kernel versions on ONE box -- tools/r5/build_ab.sh)
LIB_PATH = os.environ.get('SE3_LIB') or os.path.join(_HERE, 'csrc', 'libse3et_hip.so')
HEADER = os.path.join(os.path.dirname(_HERE), 'include', 'se3et_hip.h')

_SCALARS = {'int': ctypes.c_int, 'int32_t': ctypes.c_int, 'int64_t': ctypes.c_int64, 'float': ctypes.c_float, 'double': ctypes.c_double,
            'size_t': ctypes.c_size_t, 'uint64_t': ctypes.c_uint64, 'unsigned long long': ctypes.c_uint64}


def _ctype(spelling, proto, ret=False):
    """The ctypes type of one return or parameter type as the header spells it (a parameter may carry its name)."""
    words = [w for w in spelling.split() if w != 'const']
    if not re.search(r'[\[\]()]', spelling):
        if '*' in spelling:
            return ctypes.c_char_p if ret and ''.join(words) == 'char*' else ctypes.c_void_p
        if ret and words == ['void']:
            return None
        for scalar in (words, [] if ret else words[:-1]):
            if ' '.join(scalar) in _SCALARS:
                return _SCALARS[' '.join(scalar)]
    raise RuntimeError('%s: no ctypes type for %r (the binding knows pointers, %s)' % (proto, ' '.join(spelling.split()), ', '.join(_SCALARS)))


_ENUMERATOR = r'\b(SE3_\w+)\s*=\s*(-?\d+)\s*(?:,|$)'


def read_named_enums(text):
    """enum name -> {enumerator: value} of every `enum se3_name { SE3_NAME = integer, .. };` of a C header: the option tables that an
    entry adds beside the limits (ops.ICP_LOSSES).  They are kept apart from read_header's flat constants."""
    text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', text, flags=re.S)
    return {name: {k: int(v) for k, v in re.findall(_ENUMERATOR, body)} for name, body in re.findall(r'\benum\s+(se3_\w+)\s*\{([^}]*)\}', text)}


def read_header(text):
    """(signatures, constants) of a C header: name -> (restype, argtypes) of every `ret se3_name(args);`, and its integer `#define SE3_*`s
    together with the enumerators `SE3_NAME = integer,` of its anonymous enums.
    A prototype outside the closed type map of _ctype raises: a symbol is never left to ctypes' default int signature."""
    text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', text, flags=re.S)
    constants = {k: int(v) for k, v in re.findall(r'^[ \t]*#[ \t]*define[ \t]+(SE3_\w+)[ \t]+(-?\d+)[ \t]*$', text, flags=re.M)}
    for body in re.findall(r'\benum\s*\{([^}]*)\}', text):             # (the anonymous enums; a named one is a table of read_named_enums)
        constants.update((k, int(v)) for k, v in re.findall(_ENUMERATOR, body))
    text = re.sub(r'^[ \t]*#.*$', ' ', text, flags=re.M)
    signatures = {}
    for ret, name, params in re.findall(r'([\w\s*]+?)\b(se3_\w+)\s*\(((?:[^()]|\([^()]*\))*)\)\s*;', text):
        params = [] if params.split() in ([], ['void']) else params.split(',')
        signatures[name] = (_ctype(ret, name, ret=True), [_ctype(p, name) for p in params])
    unread = sorted(set(re.findall(r'\b(se3_\w+)\s*\(', text)) - set(signatures))
    if unread:
        raise RuntimeError('cannot read the prototype of %s' % ', '.join(unread))
    return signatures, constants


def _read():
    if not os.path.exists(HEADER):
        raise RuntimeError('%s is missing: it is the declaration of the C ABI that this binding reads' % HEADER)
    with open(HEADER) as f:
        text = f.read()
    return read_header(text) + (read_named_enums(text),)


# name -> (restype, argtypes) of every symbol, the integer limits and enumerators, and the named option enums, that include/se3et_hip.h
# declares: read once per process
SIGNATURES, CONSTANTS, ENUMS = _read()

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError('%s is missing: build it with `python -m se3et_amd.build` '
                               '(there is no CPU / eager fallback for the SE3ET hot path)' % LIB_PATH)
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        _lib = L
    return _lib


def check(status, what):
    if status != 0:
        raise RuntimeError('%s failed (code %d): %s' % (what, status, lib().se3_last_error().decode()))
