"""CPU-only: the ctypes binding (cbinfer_amd/_lib.py) is derived from include/cbinfer_hip.h -- and the C++ compiler, which
reads the same header, is the judge of the derivation: one generated translation unit static_asserts every function's
signature, every struct's layout and every constant's value as ctypes holds them.  No kernel is launched here."""
import ctypes
import os
import subprocess

import pytest
from optest import lib, raw      # noqa: F401  (fixtures)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PRELUDE = r"""
#include <cstddef>
#include "cbinfer_hip.h"
template <class T> struct Kind;      // (no definition: a type outside the five kinds does not compile)
template <> struct Kind<void> { static constexpr char c = 'v'; };
template <> struct Kind<int> { static constexpr char c = 'i'; };
template <> struct Kind<long> { static constexpr char c = 'l'; };
template <> struct Kind<float> { static constexpr char c = 'f'; };
template <class T> struct Kind<T*> { static constexpr char c = 'p'; };
constexpr bool same(const char* a, const char* b) { return *a == *b && (*a == 0 || same(a + 1, b + 1)); }
template <class R, class... A> constexpr bool sig(R (*)(A...), const char* kinds) {
    const char is[] = {Kind<R>::c, Kind<A>::c..., 0};
    return same(is, kinds);
}
"""


def kind(t):
    """void, int, long, float or pointer -- of a ctypes restype / argtype."""
    if t is None:
        return 'v'
    scalars = {ctypes.c_int: 'i', ctypes.c_long: 'l', ctypes.c_float: 'f'}
    if t in scalars:
        return scalars[t]
    assert t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, ctypes._Pointer), t
    return 'p'


def header_of(lib):
    with open(lib.HEADER_PATH) as f:
        return lib.parse_header(f.read())


def unit(lib):
    """The translation unit: what the loaded binding holds, as static_asserts over the header."""
    consts, structs, funcs = header_of(lib)
    out = [PRELUDE]
    assert tuple(funcs) == lib.EXPORTED_SYMBOLS and len(funcs) >= 167
    for name in lib.EXPORTED_SYMBOLS:
        raw = getattr(lib.C, name).raw
        kinds = kind(raw.restype) + "".join(kind(t) for t in raw.argtypes)
        assert len(getattr(lib.C, name).params) == len(raw.argtypes)
        out.append('static_assert(sig(&%s, "%s"), "%s");' % (name, kinds, name))
    assert len(structs) >= 15
    for name in structs:
        cls = getattr(lib, name)
        out.append('static_assert(sizeof(cb%s) == %d, "cb%s");' % (name, ctypes.sizeof(cls), name))
        for field, _ in cls._fields_:
            d = getattr(cls, field)
            out.append('static_assert(offsetof(cb%s, %s) == %d && sizeof(cb%s::%s) == %d, "cb%s.%s");'
                       % (name, field, d.offset, name, field, d.size, name, field))
    assert len(consts) >= 72
    for name in consts:
        value = getattr(lib, name)
        for prefix in ("CBINFER_", "CB_"):
            if name.startswith(prefix):
                assert getattr(lib, name[len(prefix):]) == value, name
                break
        out.append('static_assert(%s == %d, "%s");' % (name, value, name))
    out.append('static_assert(CBINFER_ABI_VERSION == %d, "the bound ABI version");' % lib.ABI_VERSION)
    return "\n".join(out) + "\n"


def compiles(tmp_path, text, fname):
    path = tmp_path / fname
    path.write_text(text)
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(REPO, "include"), str(path)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    return r.returncode == 0, r.stdout


def test_the_compiler_agrees_with_the_derived_binding(lib, tmp_path):
    assert lib.C.cbinfer_abi_version() == lib.ABI_VERSION == lib.CBINFER_ABI_VERSION
    text = unit(lib)
    ok, log = compiles(tmp_path, text, "abi.cpp")
    assert ok, log[-4000:]
    # ... and the unit can fail: one kind altered (cbinfer_mask_words returns long), one offset moved
    for good, wrong in (('sig(&cbinfer_mask_words, "lii")', 'sig(&cbinfer_mask_words, "iii")'),
                        ('sig(&cbinfer_refresh_state, "ippiiifp")', 'sig(&cbinfer_refresh_state, "ippiiiip")'),
                        ('offsetof(cbHalfLayer, next) == 120', 'offsetof(cbHalfLayer, next) == 128')):
        assert text.count(good) == 1, good
        ok, log = compiles(tmp_path, text.replace(good, wrong), "abi_wrong.cpp")
        assert not ok and "static assertion failed" in log, (wrong, log[-2000:])
    assert ctypes.sizeof(lib.HalfLayer) == 200


@pytest.mark.parametrize("text, names", [
    ("int cbinfer_x(const void* p, double v, cbStream_t stream);", "double v"),
    ("double cbinfer_x(int a);", "double cbinfer_x"),
    ("typedef struct {\n    int a;\n    size_t n;\n} cbThing;", "size_t n"),
    ("typedef struct {\n    int* a, b;\n} cbThing;", "int* a, b"),
    ("typedef struct {\n    float v[CB_UNKNOWN];\n} cbThing;", "v[CB_UNKNOWN]"),
    ("#define CB_X (1 << 3)", "(1 << 3)"),
    ("#define CB_X", "CB_X"),
    ("enum { CB_A, CB_B = 4 };", "CB_B = 4"),
    ("int cbinfer_ok(int a);\nint cbinfer_broken(int a, void (*done)(int),\n                   cbStream_t stream);",
     "cbinfer_broken(int a, void (*done)(int)"),
    ("int cbinfer_broken(int a)\nint cbinfer_ok(int a);", "cbinfer_broken(int a)"),
    ("#pragma pack(1)", "#pragma pack(1)"),
])
def test_the_parser_refuses_what_it_cannot_read(lib, text, names):
    with pytest.raises(ValueError) as e:
        lib.parse_header(text)
    assert names in str(e.value), str(e.value)


def test_the_parser_reads_the_forms_the_header_uses(lib):
    consts, structs, funcs = lib.parse_header(
        "/* a comment with int cbinfer_not(int a); in it */\n"
        "#ifndef X_H\n#define X_H\n#include <stdint.h>\ntypedef void* cbStream_t; // the stream\n"
        "#define CB_N 3\n#define CB_NEG (-2)\nenum { CB_E0, CB_E1 };\n"
        "typedef struct {\n    const float* p;\n    int a, b;\n    float t;\n} cbInner;\n"
        "typedef struct cbOuter {\n    uint64_t* out[CB_N];\n    cbInner in[2];\n} cbOuter;\n"
        "const char* cbinfer_text(int status);\nvoid cbinfer_host(const float* const* x, const cbOuter* o,\n"
        "                  cbOuter** oo);\nlong cbinfer_go(void);\nint cbinfer_launch(const cbInner* i, float th, cbStream_t stream);\n"
        "#endif\n")
    assert consts == {"CB_N": 3, "CB_NEG": -2, "CB_E0": 0, "CB_E1": 1}
    inner, outer = structs["Inner"], structs["Outer"]
    assert [f for f, _ in inner._fields_] == ["p", "a", "b", "t"] and ctypes.sizeof(inner) == 24
    assert outer.out.size == 24 and outer.__dict__["in"].offset == 24 and ctypes.sizeof(outer) == 72
    assert funcs["cbinfer_text"] == (ctypes.c_char_p, ("status",), [ctypes.c_int], False)
    assert funcs["cbinfer_host"] == (None, ("x", "o", "oo"), [ctypes.c_void_p, ctypes.POINTER(outer), ctypes.c_void_p], False)
    assert funcs["cbinfer_go"] == (ctypes.c_long, (), [], False)
    assert funcs["cbinfer_launch"] == (ctypes.c_int, ("i", "th", "stream"),
                                       [ctypes.POINTER(inner), ctypes.c_float, ctypes.c_void_p], True)


def test_launchers_are_the_functions_that_end_in_a_stream(lib):
    C = lib.C
    assert C.cbinfer_cbpad_forward.launcher is True
    assert C.cbinfer_pad_out_size.launcher is False      # (no stream parameter; ends in int*)
    assert C.cbinfer_mask_words.launcher is False
    assert C.cbinfer_conv2d_fg_cpu.launcher is False
    assert sum(getattr(C, n).launcher for n in lib.EXPORTED_SYMBOLS) >= 106


def test_pack_orders_named_arguments_as_declared(lib):
    fn = lib.C.cbinfer_pad_out_size      # (const cbPad* p, int H, int W, int* Ho, int* Wo)
    assert fn.params == ("p", "H", "W", "Ho", "Wo")
    assert fn.pack(Wo=5, Ho=4, W=3, H=2, p=1) == (1, 2, 3, 4, 5)
    with pytest.raises(TypeError, match="cbinfer_pad_out_size.*'W'"):
        fn.pack(p=1, H=2, Ho=4, Wo=5)
    with pytest.raises(TypeError, match="cbinfer_pad_out_size.*'width'"):
        fn.pack(p=1, H=2, W=3, Ho=4, Wo=5, width=3)
    with pytest.raises(TypeError, match="'H'"):
        fn.pack(p=1, H=2, W=3, Ho=4, Wo=5, **{"H": 2})


def test_names_are_the_headers(lib):
    assert lib.CB_F32 == lib.F32 == 0
    assert lib.PW_TANH == 9
    assert lib.HNEXT_MAX == 2
    assert lib.SplitSeq._fields_[-1][0] == "reluOut"
    assert lib.CB_ERR_UNSUPPORTED == lib.ERR_UNSUPPORTED == -2 and lib.SPLIT_MAX_SEQUENCES == 8
    assert lib.HalfLayer.next.offset == 120 and lib.SplitTail.output.size == 8 * ctypes.sizeof(ctypes.c_void_p)
