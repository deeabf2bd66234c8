"""ctypes binding of libcbinfer_hip.so, derived at import from the one declaration of its C ABI: include/cbinfer_hip.h.

Replaces the reference's cffi ABI-mode dlopen at import time (pycbinfer/conv2d_cg.py:40-50,
conv2d_fg.py:13-32).  There is no fallback: if the HIP library has not been built, importing the
package fails, exactly as the reference fails when its CUDA .so files are missing.

What the header declares appears here under the header's names: every function as `C.cbinfer_*`, every
`typedef struct { ... } cbX;` as the ctypes.Structure `X`, every `#define` and enumerator as an int, both verbatim
(`CB_F32`) and without its `CB_` / `CBINFER_` prefix (`F32`, `HNEXT_MAX`).  A new entry point is declared in the header
and nowhere else.
"""
import ctypes
import os
import re

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "libcbinfer_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_PKG), "include", "cbinfer_hip.h")

_SCALARS = {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float, "cbStream_t": ctypes.c_void_p}
_RETURNS = {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float, "void": None, "char*": ctypes.c_char_p}
# the forms the header is written in.  _SCAFFOLD: what it holds besides declarations -- include guard, <stdint.h>, the
# extern "C" bracket, the stream typedef
_SCAFFOLD = re.compile(r'#ifndef\s+(\w+)\s*\n\s*#define\s+\1[ \t]*\n|#include\s*<\w+\.h>|#endif|'
                       r'#ifdef\s+__cplusplus\s*(?:extern\s+"C"\s*\{|\})\s*#endif|typedef\s+void\s*\*\s*cbStream_t\s*;')
_DEFINE = re.compile(r'^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]*(.*?)[ \t]*$', re.M)
_ENUM = re.compile(r'\benum\s*\{([^{}]*)\}\s*;')
_STRUCT = re.compile(r'\btypedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*cb(\w+)\s*;')
_PROTO = re.compile(r'([\w\s*]+?)\b(cbinfer_\w+)\s*\(([^(){};]*)\)\s*;')
_DECL = re.compile(r'(\w+)((?:\s*\*)*)\s*\b(\w+)\s*(?:\[\s*(\w+)\s*\])?')


def parse_header(text):
    """The C ABI a header text declares: (constants {name: int}, structs {X: ctypes.Structure class of cbX},
    functions {name: (restype, parameter names, argtypes, launcher)}).  launcher: the last parameter is the cbStream_t
    the function enqueues on.  Every form is taken out of the text as it is read; whatever is left over, and any type
    or value outside the tables above, raises ValueError with the offending text -- nothing is skipped."""
    consts, structs, funcs = {}, {}, {}

    def bad(what, text):
        return ValueError("cbinfer_hip.h: %s: '%s'" % (what, " ".join(text.split())))

    def declare(text, param):
        """One declarator, 'const float* output[CBINFER_SPLIT_MAX_SEQUENCES]' -> ('output', c_void_p * 8)."""
        m = _DECL.fullmatch(re.sub(r'\bconst\b', ' ', text).strip())
        if m is None:
            raise bad("unreadable declaration", text)
        base, stars, name, dim = m.groups()
        struct = structs.get(base[2:]) if base.startswith("cb") else None
        if stars:       # a pointer: typed for a parameter that points to one of the header's structs, else opaque
            t = ctypes.POINTER(struct) if (param and struct and stars.count('*') == 1) else ctypes.c_void_p
        elif base in _SCALARS:
            t = _SCALARS[base]
        elif struct and not param:
            t = struct
        else:
            raise bad("type outside the binding's table", text)
        if dim is not None:
            if param or not (dim.isdigit() or dim in consts):
                raise bad("unreadable array size", text)
            t = t * (int(dim) if dim.isdigit() else consts[dim])
        return name, t

    def define(m):
        value = re.fullmatch(r'\(\s*(-?\d+)\s*\)|(-?\d+)', m.group(2))
        if value is None:
            raise bad("#define whose value is not an integer literal", m.group(0))
        consts[m.group(1)] = int(value.group(1) or value.group(2))
        return ''

    def enum(m):
        for value, name in enumerate(n.strip() for n in m.group(1).split(',')):
            if not name.isidentifier():
                raise bad("enumerator that is not a plain name", m.group(0))
            consts[name] = value
        return ''

    def struct(m):
        fields = []
        for decl in filter(str.strip, m.group(1).split(';')):
            first, *more = decl.split(',')      # (int C1, C2, relu1, relu2;)
            name, t = declare(first, False)
            if more and ('*' in first or '[' in first) or not all(n.strip().isidentifier() for n in more):
                raise bad("unreadable declaration", decl)
            fields += [(name, t)] + [(n.strip(), t) for n in more]
        structs[m.group(2)] = type(m.group(2), (ctypes.Structure,),
                                   {"_fields_": fields, "__doc__": "cb%s of include/cbinfer_hip.h." % m.group(2)})
        return ''

    def proto(m):
        res = re.sub(r'\bconst\b|\s', '', m.group(1))
        if res not in _RETURNS:
            raise bad("return type outside the binding's table", m.group(0))
        params = m.group(3).strip()
        decls = [declare(p, True) for p in params.split(',')] if params not in ('', 'void') else []
        funcs[m.group(2)] = (_RETURNS[res], tuple(n for n, _ in decls), [t for _, t in decls],
                             re.search(r'\bcbStream_t\s+\w+$', params) is not None)
        return ''

    text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', text, flags=re.S)
    for pattern, take in ((_SCAFFOLD, ''), (_DEFINE, define), (_ENUM, enum), (_STRUCT, struct), (_PROTO, proto)):
        text = pattern.sub(take, text)
    if text.strip():
        raise bad("text that is none of #define, enum, typedef struct or prototype", text.strip()[:200])
    return consts, structs, funcs


def _declarations():
    with open(HEADER_PATH) as f:
        consts, structs, funcs = parse_header(f.read())
    exported = dict(structs)
    for name, value in consts.items():
        for alias in {name, re.sub(r'^(CBINFER|CB)_', '', name)}:
            if alias in exported or alias in globals():
                raise ImportError("cbinfer_amd: cbinfer_hip.h declares '%s' twice (as %s)" % (alias, name))
            exported[alias] = value
    globals().update(exported)
    return funcs


_FUNCTIONS = _declarations()
EXPORTED_SYMBOLS = tuple(_FUNCTIONS)


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "cbinfer_amd: %s not found. Build the HIP kernels first (python -c 'import "
            "__graft_entry__ as g; g.build()' or make -C cbinfer_amd/csrc). There is no CPU or "
            "PyTorch fallback." % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, _, args, _) in _FUNCTIONS.items():
        fn = getattr(lib, name)     # AttributeError if the ABI is incomplete
        fn.restype = res
        fn.argtypes = args
    if lib.cbinfer_abi_version() != ABI_VERSION:      # noqa: F821  (CBINFER_ABI_VERSION of the header)
        raise ImportError("cbinfer_amd: libcbinfer_hip.so ABI version mismatch: the library reports %d, "
                          "include/cbinfer_hip.h declares %d" % (lib.cbinfer_abi_version(), ABI_VERSION))      # noqa: F821
    return lib


class _Fn(object):
    """One entry point of the library.  Calls go straight to the ctypes function; while a `FrameProgram` records
    (cbinfer_amd/program.py) every call is also noted -- function and argument objects -- so that the frame's launch
    sequence can be replayed later without the modules around it."""
    __slots__ = ('raw', '__name__', 'launcher', 'params')

    def __init__(self, raw, name, launcher, params):
        # launcher: the function enqueues work on a stream (its last parameter is the cbStream_t) -- as opposed to the host
        # helpers (sizes, capability queries), which a recorded frame does not need to repeat
        self.raw, self.__name__, self.launcher, self.params = raw, name, launcher, params

    def __call__(self, *args):
        rec = _RECORDING[0]
        if rec is not None and self.launcher:
            rec.append((self, args))
        return self.raw(*args)

    def pack(self, **kw):
        """The positional arguments of a call, in the declared order, from arguments given by the header's parameter
        names.  For the places that BUILD a call plan (several entry points sharing most of their arguments), not for a
        per-frame path.  (A name given twice is Python's own TypeError.)"""
        missing = [n for n in self.params if n not in kw]
        unknown = [n for n in kw if n not in self.params]
        if missing or unknown:
            raise TypeError("%s: %s" % (self.__name__, ", ".join(
                ["missing argument '%s'" % n for n in missing] + ["no parameter named '%s'" % n for n in unknown])))
        return tuple([kw[n] for n in self.params])


_RECORDING = [None]


class _Lib(object):
    def __init__(self, lib):
        self._cdll = lib
        for name, (_, params, _, launcher) in _FUNCTIONS.items():
            setattr(self, name, _Fn(getattr(lib, name), name, launcher, params))


C = _Lib(_load())


class CBinferError(RuntimeError):
    pass


def check(status):
    """Raise on a non-zero launcher status (the reference launchers return void and never check)."""
    if status != 0:
        raise CBinferError("libcbinfer_hip: %s (status %d)" %
                           (C.cbinfer_status_string(status).decode(), status))


def dtype_code(t):
    import torch
    if t.dtype == torch.float32:
        return CB_F32      # noqa: F821
    if t.dtype == torch.float16:
        return CB_F16      # noqa: F821
    raise TypeError("cbinfer_amd supports float32 and float16 tensors, got %s" % t.dtype)


def stream_ptr(t=None):
    import torch
    return torch.cuda.current_stream(t.device if t is not None else None).cuda_stream


def raw_stream(device_index):
    """Raw handle of torch's current stream on a device (the cheap form used on the per-frame fast path)."""
    import torch
    try:
        return torch._C._cuda_getCurrentRawStream(device_index)
    except AttributeError:      # pragma: no cover  (older torch)
        return torch.cuda.current_stream(device_index).cuda_stream


def ptr(t):
    return t.data_ptr() if t is not None else None


def require_device(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise CBinferError(
                "cbinfer_amd runs on HIP devices only: got a CPU tensor. (The reference's pure-torch "
                "CPU twins are restated in oracle/ for testing, they are not part of the product.)")
