"""The numpy twin and the case tables of the change-based element-wise operators of two maps (DESIGN 5.25;
cb_binary.hip), shared by tests/test_host_binary.py and tests/test_gpu_binary.py.  The twin implements the specification
of include/cbinfer_hip.h: both operands to float32 (exact), ONE float32 operation, explicit comparisons for maximum /
minimum, a gate value rounded to the operand dtype before the product, one rounding to float16."""
import numpy as np
from optest import pack      # noqa: F401  (handed on to the tests)

OPS = ('add', 'sub', 'mul', 'maximum', 'minimum')
GATES = (None, 'sigmoid', 'hardsigmoid')
FORMS = ('map', 'pixel', 'channel', 'scalar', 'halves')      # CB_BIN_MAP ... CB_BIN_HALVES, in the enum's order
# (op, reverse) of every exact function without a gate
EXACT = [('add', False), ('sub', False), ('sub', True), ('mul', False), ('maximum', False), ('minimum', False)]

# [C, H, W]: the word boundary, the padding bits, n C below, beside and above 256, more mask words than workgroups.  All
# C are even or 1 (the halves form doubles them anyway).
SMALL = [(1, 1, 9), (3, 5, 64), (6, 1, 65)]
LARGE = [(300, 5, 130), (2, 2100, 9)]
SHAPES = SMALL + LARGE
STRIDED = (2, 2100, 9)


def b_shape(form, Cn, H, W):
    """The shape of the second operand as the twin and the library take it (None: the upper half of a)."""
    return {'map': (Cn, H, W), 'pixel': (1, H, W), 'channel': (Cn,), 'scalar': (1,), 'halves': None}[form]


def twin(a, b, bForm, op, gate=None, reverse=False):
    """out [C, H, W] of a [C, H, W] ([2C, H, W] in 'halves' form, b None) and b in the shape of b_shape."""
    dt = a.dtype
    assert dt in (np.float32, np.float16) and op in OPS and gate in GATES
    assert (gate is None or op == 'mul') and (not reverse or op == 'sub')
    if bForm == 'halves':
        assert b is None and a.shape[0] % 2 == 0
        a, b = a[:a.shape[0] // 2], a[a.shape[0] // 2:]
    elif bForm == 'channel':
        b = b.reshape(-1, 1, 1)
    elif bForm == 'scalar':
        b = b.reshape(1, 1, 1)
    assert b.dtype == dt
    f32 = np.float32
    af = a.astype(f32)
    bf = np.broadcast_to(b.astype(f32), af.shape)
    with np.errstate(all='ignore'):
        if gate == 'sigmoid':
            g = f32(1) / (f32(1) + np.exp(-bf, dtype=f32))
            bf = g.astype(dt).astype(f32)
        elif gate == 'hardsigmoid':
            t = bf + f32(3)
            t = np.where(t < f32(0), f32(0), np.where(t > f32(6), f32(6), t)).astype(f32)
            bf = (t / f32(6)).astype(dt).astype(f32)
        if op == 'add':
            r = af + bf
        elif op == 'sub':
            r = bf - af if reverse else af - bf
        elif op == 'mul':
            r = af * bf
        elif op == 'maximum':
            r = np.where(af != af, af, np.where(bf != bf, bf, np.where(bf > af, bf, af)))
        else:
            r = np.where(af != af, af, np.where(bf != bf, bf, np.where(bf < af, bf, af)))
        assert r.dtype == f32
        return r.astype(dt)


def same_bits(got, want):
    """Equal bit for bit, NaNs by NaN-ness."""
    assert got.dtype == want.dtype and got.shape == want.shape
    u = np.uint32 if got.dtype == np.float32 else np.uint16
    gn, wn = np.isnan(got), np.isnan(want)
    return bool(np.array_equal(gn, wn) and np.array_equal(got.view(u)[~gn], want.view(u)[~wn]))


def specials(dtype):
    """+-0, +-inf, NaN, float16 subnormals, ties of equal magnitude and ordinary values: every pair meets in pairs()."""
    v = [0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, 2.5, -2.5, 6.0e-8, -6.0e-8, 5.9e-5, 3.0e-5, -3.0e-5, 65504.0,
         -65504.0, 1.0 + 2.0 ** -10, 3.0, -3.0, 0.1, -7.3, 1e-3, 2.9990, -2.9990, 4.5, 1.0e4]
    return np.array(v, dtype=dtype)


def pairs(dtype):
    """(a, b): every special value against every other, as two [n n] vectors."""
    s = specials(dtype)
    a, b = np.meshgrid(s, s, indexing='ij')
    return a.reshape(-1).copy(), b.reshape(-1).copy()


def frame_sets(rng, H, W):
    """(label, pixels operand a changes, pixels operand b changes) of the frames behind the first one (the sets of
    tests/test_gpu_add.py)."""
    Z = np.zeros((H, W), dtype=bool)

    def at(*pixels):
        m = Z.copy()
        for y, x in pixels:
            m[y, x] = True
        return m
    word = Z.copy()
    word[0, :min(W, 64)] = True
    A = rng.random((H, W)) < 0.1
    B = (rng.random((H, W)) < 0.1) & ~A
    A2, B2 = rng.random((H, W)) < 0.2, rng.random((H, W)) < 0.2
    A2[0, 0] = B2[0, 0] = True
    return [("empty", Z, Z), ("single", at((H // 2, W // 2)), Z), ("full word", word, Z),
            ("last column", Z, at((H - 1, W - 1))), ("both corners", at((0, 0)), at((H - 1, W - 1))),
            ("disjoint", A, B), ("overlapping", A2, B2), ("empty again", Z, Z)]
