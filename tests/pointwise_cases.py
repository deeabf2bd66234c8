"""The specification of the change-based element-wise functions (CBPointwise2d, cb_pointwise.hip) as a
numpy float32 twin, and the shapes, mask patterns and values the host and GPU tests share.  The reference has no such
operator, so the twin written here IS the specification:
  rule 1  affine (optional): v = fl(fl(x scale[c]) + shift[c]) -- two float32 operations, never one FMA;
  rule 2  the function `kind` on v, every operation a float32 one in the order written, comparisons instead of
          fmin / fmax (a NaN stays a NaN); the result rounded to the map's dtype once;
  rule 3  only listed pixels are written; the frame's mask is handed on, padding bits never set.
No GPU is needed to import this file."""
import numpy as np
from optest import bits_of, pack      # noqa: F401  (handed on to the tests)

F32 = np.float32
(IDENTITY, RELU, HARDTANH, LEAKY, PRELU, HARDSWISH, HARDSIGMOID, SIGMOID, SILU, TANH) = range(10)
NAMES = ["IDENTITY", "RELU", "HARDTANH", "LEAKY", "PRELU", "HARDSWISH", "HARDSIGMOID", "SIGMOID", "SILU", "TANH"]
# (kind, p0, p1): the kinds whose twin is exact, and the three that call expf / tanhf
EXACT = [(IDENTITY, 0.0, 0.0), (RELU, 0.0, 0.0), (HARDTANH, 0.0, 6.0), (LEAKY, 0.01, 0.0), (PRELU, 0.0, 0.0),
         (HARDSWISH, 0.0, 0.0), (HARDSIGMOID, 0.0, 0.0)]
INEXACT = [(SIGMOID, 0.0, 0.0), (SILU, 0.0, 0.0), (TANH, 0.0, 0.0)]

# [C, H, W]: W in {9, 64, 65, 130} (word boundary, padding bits), H in {1, 5}, C in {1, 3, 5, 300} (n C below, not a
# multiple of, and many times 256); the last has more mask words than the grid takes workgroups (8 per CU, 256 CUs)
SHAPES = [(1, 1, 9), (3, 5, 64), (5, 1, 65), (300, 5, 130), (5, 5, 9), (1, 5, 130), (3, 1, 130), (300, 1, 64),
          (1, 2100, 9)]
FORMS = ["mask", "list", "all"]


def _clamp(t, lo, hi):
    return np.where(t < lo, lo, np.where(t > hi, hi, t))


def twin(x, kind, p0=0.0, p1=0.0, scale=None, shift=None, slope=None):
    """x [C, H, W] float32 or float16 -> act(x scale + shift) in x's dtype; scale, shift, slope float32 [C]."""
    assert x.dtype in (np.float32, np.float16)
    p0, p1 = F32(p0), F32(p1)
    with np.errstate(all='ignore'):
        v = x.astype(F32)
        if scale is not None:
            assert scale.dtype == F32 and shift.dtype == F32
            v = v * scale[:, None, None]      # (rounded to float32 here ...
            v = v + shift[:, None, None]      #  ... and here)
        if kind == RELU:
            v = np.where(v < 0, F32(0), v)
        elif kind == HARDTANH:
            v = _clamp(v, p0, p1)
        elif kind == LEAKY:
            v = np.where(v > 0, v, v * p0)
        elif kind == PRELU:
            assert slope.dtype == F32
            v = np.where(v > 0, v, slope[:, None, None] * v)
        elif kind == HARDSWISH:
            v = v * _clamp(v + F32(3), F32(0), F32(6)) / F32(6)
        elif kind == HARDSIGMOID:
            v = _clamp(v + F32(3), F32(0), F32(6)) / F32(6)
        elif kind == SIGMOID:
            v = F32(1) / (F32(1) + np.exp(-v))
        elif kind == SILU:
            v = v / (F32(1) + np.exp(-v))
        elif kind == TANH:
            v = np.tanh(v)
        else:
            assert kind == IDENTITY
        assert v.dtype == F32
        return v.astype(x.dtype)


def reference64(x, kind):
    """SIGMOID / SILU / TANH of x (no affine) in float64, by the formula of the specification."""
    v = x.astype(np.float64)
    with np.errstate(all='ignore'):
        if kind == SIGMOID:
            return 1.0 / (1.0 + np.exp(-v))
        if kind == SILU:
            return v / (1.0 + np.exp(-v))
        assert kind == TANH
        return np.tanh(v)


def bn_affine(gamma, beta, mean, var, eps):
    """scale = gamma / sqrt(var + eps), shift = beta - mean scale: float64, each rounded once to float32."""
    scale = gamma.astype(np.float64) / np.sqrt(var.astype(np.float64) + eps)
    return scale.astype(F32), (beta.astype(np.float64) - mean.astype(np.float64) * scale).astype(F32)


def per_channel(rng, C):
    """(scale, shift, slope) float32 [C] for the tests: scales of both signs away from 0, slopes of both signs."""
    scale = (rng.uniform(0.5, 2.0, C) * rng.choice([-1.0, 1.0], C)).astype(F32)
    shift = rng.uniform(-3.0, 3.0, C).astype(F32)
    slope = rng.uniform(-0.5, 0.5, C).astype(F32)
    return scale, shift, slope


def specials(dtype):
    s = [0.0, -0.0, 3.0, -3.0, 6.0, -6.0, 65504.0, -65504.0, np.inf, -np.inf, np.nan]
    if dtype == np.float32:
        s += [1e30, -1e30]
    return np.array(s, dtype=dtype)


def values(rng, shape, dtype, span=8.0, special=None):
    """Uniform in [-span, span], a fifth replaced by 1e-3-scale normals, a twentieth by the special values."""
    v = rng.uniform(-span, span, shape)
    small = rng.random(shape) < 0.2
    v[small] = rng.standard_normal(int(small.sum())) * 1e-3
    v = v.astype(dtype)
    sp = specials(dtype) if special is None else special
    pick = rng.random(shape) < 0.05
    v[pick] = rng.choice(sp, int(pick.sum()))
    if v.size >= len(sp):      # (every special value at least once, where the map has the room)
        v.reshape(-1)[rng.choice(v.size, len(sp), replace=False)] = sp
    return v


def patterns(rng, H, W):
    """(label, bool [H, W]) of consecutive frames: full, empty, one bit, the last column, both sides of a word boundary
    (of a row boundary where a row is one word), random 10 %."""
    Z = np.zeros((H, W), dtype=bool)
    one, last, edge = Z.copy(), Z.copy(), Z.copy()
    one[H // 2, W // 2] = True
    last[:, W - 1] = True
    if W > 64:
        edge[0, 63] = edge[0, 64] = True
        edge[H - 1, 63] = edge[H - 1, 64] = True
    else:
        edge[0, W - 1] = edge[H - 1, 0] = True
    return [("full", ~Z), ("empty", Z), ("one bit", one), ("last column", last), ("word boundary", edge),
            ("random", rng.random((H, W)) < 0.1)]


def same_bits(got, want):
    """Integer views equal wherever `want` is not a NaN, NaNs in the same positions."""
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(bits_of(got)[~nan], bits_of(want)[~nan])
