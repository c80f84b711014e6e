"""The ctypes lists of ``_lib.ABI`` and ``tfrecord_native.ABI`` held against the prototypes of include/biscuit_hip.h and
include/biscuit_io.h, position by position (tests/test_host.py, tests/test_tfrecord_native.py): every parameter and every return
type as a width class -- 'ptr', 'i32', 'u32', 'i64', 'u64' (``size_t`` too), 'f32', 'f64', 'void'.  A type neither side of this
table knows is a KeyError, not a guess.  Reads the header's text and the dict only: no library, no GPU."""
import ctypes as C
import re

C_TYPES = {'void': 'void', 'int': 'i32', 'int32_t': 'i32', 'unsigned': 'u32', 'unsigned int': 'u32', 'uint32_t': 'u32', 'int64_t': 'i64',
           'uint64_t': 'u64', 'size_t': 'u64', 'float': 'f32', 'double': 'f64', 'bq_stream_t': 'ptr'}
CTYPES = {None: 'void', C.c_void_p: 'ptr', C.c_char_p: 'ptr', C.c_int32: 'i32', C.c_uint32: 'u32', C.c_int64: 'i64', C.c_uint64: 'u64',
          C.c_float: 'f32', C.c_double: 'f64'}
assert C.c_int is C.c_int32 and C.c_size_t is C.c_uint64                # (this platform: what the bindings are written for)

PROTOTYPE = re.compile(r'([A-Za-z_][\w \t*]*?)\s*\b(bq(?:io)?_\w+)\s*\(([^()]*)\)\s*;')


def c_class(decl, named):
    """The class of a C declarator: ``const uint8_t* d_rows`` -> 'ptr', ``size_t`` -> 'u64' (``named``: a parameter, whose last word
    is its name unless the type is all there is, as in ``(void)``)."""
    if '*' in decl:
        return 'ptr'
    words = [w for w in decl.split() if w != 'const']
    if named and len(words) > 1:
        words = words[:-1]
    return C_TYPES[' '.join(words)]


def header_types(text):
    """{name: (class of the return type, [class of every parameter])} of every prototype in a header's text, comments stripped."""
    text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    text = re.sub(r'//[^\n]*', ' ', text)
    out = {}
    for ret, name, params in PROTOTYPE.findall(text):
        args = [c_class(p, True) for p in params.split(',')] if params.strip() else []
        out[name] = (c_class(ret, False), [] if args == ['void'] else args)
    return out


def ctypes_class(t):
    if isinstance(t, type) and issubclass(t, C._Pointer):
        return 'ptr'
    return CTYPES[t]


def abi_types(abi):
    """{name: (class of restype, [class of every argtype])} of an ``ABI`` dict."""
    return {name: (ctypes_class(res), [ctypes_class(a) for a in args]) for name, (res, args) in abi.items()}


def assert_abi_matches_header(abi, header_path):
    want, got = header_types(open(header_path).read()), abi_types(abi)
    assert set(want) == set(got), set(want) ^ set(got)
    for name in sorted(want):
        assert got[name] == want[name], f'{name}: the binding says {got[name]}, the header {want[name]}'
