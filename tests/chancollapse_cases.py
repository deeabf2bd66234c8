"""The specification of the change-based reductions that collapse the channel axis (CBChannelReduce2d's ops 'sum', 'mean',
'norm', 'max', 'min', 'argmax', 'argmin'; cb_chancollapse.hip) as a numpy twin, the float64 reference,
the error bounds and the values the host and GPU tests share:
  rule 1  SUM = sum16(x), MEAN = sum16(x) / float32(C), NORM = sqrt(sum16(x_c x_c)), with sum16 EXACTLY that of
          tests/chanreduce_cases.py (16 slices c mod 16, ascending c within a slice from +0, the fixed tree
          p[2i] + p[2i+1]); every operation a float32 one in the order written, never an FMA; one rounding to the map's
          dtype;
  rule 2  ARGMAX / ARGMIN = the smallest index c whose value is maximal / minimal under torch's CPU order: a NaN beats
          every number and the first NaN wins; +0 == -0 is a tie and the first index wins.  int64;
  rule 3  MAX / MIN = the value AT that index (torch.max / torch.min(x, 1).values): -0 where -0 comes first in a +-0
          tie, a NaN where any channel is one;
  rule 4  only listed pixels are written; the frame's mask is handed on, padding bits never set; the label mask of an
          arg launch has a bit where a listed pixel's label moved (or every listed pixel, in all form).
Shapes, mask patterns and forms are those of tests/chanreduce_cases.py.  No GPU is needed to import this file."""
import math

import numpy as np

import chanreduce_cases as cr
from chanreduce_cases import sum16      # (not copied: THE summation order of DESIGN 5.21)

F32 = np.float32
SUM, MEAN, NORM, MAX, MIN, ARGMAX, ARGMIN = range(7)
NAMES = ["SUM", "MEAN", "NORM", "MAX", "MIN", "ARGMAX", "ARGMIN"]
OP_NAMES = ["sum", "mean", "norm", "max", "min", "argmax", "argmin"]
FLOAT_KINDS, EXTREME_KINDS, ARG_KINDS = (SUM, MEAN, NORM), (MAX, MIN), (ARGMAX, ARGMIN)
SHAPES, FORMS = cr.SHAPES, cr.FORMS
patterns, pack, bits_of, same_bits = cr.patterns, cr.pack, cr.bits_of, cr.same_bits


def packed(kinds):
    """The kinds of one call as the library takes them: 4 bits per op, op k in bits 4k .. 4k+3."""
    return sum(k << (4 * i) for i, k in enumerate(kinds))


def twin_arg(x, kind):
    """x [C, ...] -> int64 [...]: rule 2, written out (numpy's own argmax / argmin follow the same rules; the host test
    checks both against torch)."""
    assert kind in (ARGMAX, ARGMIN, MAX, MIN)
    v = x.astype(F32)
    nan = np.isnan(v)
    if kind in (ARGMAX, MAX):
        best = np.where(nan, -np.inf, v).argmax(axis=0)      # (the first of equal values; +0 == -0)
    else:
        best = np.where(nan, np.inf, v).argmin(axis=0)
    return np.where(nan.any(axis=0), nan.argmax(axis=0), best).astype(np.int64)


def twin(x, kind):
    """x [C, ...] float32 or float16 -> the value kind `kind` over axis 0 in x's dtype."""
    assert x.dtype in (np.float32, np.float16) and kind in FLOAT_KINDS + EXTREME_KINDS
    if kind in EXTREME_KINDS:
        return np.take_along_axis(x, twin_arg(x, kind)[None], axis=0)[0]
    with np.errstate(all='ignore'):
        v = x.astype(F32)
        if kind == SUM:
            y = sum16(v)
        elif kind == MEAN:
            y = sum16(v) / F32(x.shape[0])
        else:
            y = np.sqrt(sum16(v * v))
        assert y.dtype == F32
        return y.astype(x.dtype)


def twin_values(x, kinds):
    """[len(kinds), ...]: the state of one call with several value ops."""
    return np.stack([twin(x, k) for k in kinds])


def reference64(x, kind):
    """SUM / MEAN / NORM in float64 (numpy's own sums): the operator's mathematical value on the stored inputs."""
    v = x.astype(np.float64)
    with np.errstate(all='ignore'):
        return v.sum(axis=0) if kind == SUM else v.mean(axis=0) if kind == MEAN else np.sqrt((v * v).sum(axis=0))


def bound(x, kind, ref):
    """The error bound of a result of dtype x.dtype against ref = reference64(x, kind), per pixel.  u = 2^-24 is what one
    correctly rounded float32 operation adds relative to its result; a value passes through ceil(C / 16) additions in
    its slice and four in the tree: K - 1 with K = ceil(C / 16) + 5, as in DESIGN 5.21.  First order, taken twice:
      SUM   2u (K - 1) sum |x_c|: every addition's rounding is at most u times a partial sum, which sum |x_c| bounds;
      MEAN  2u K sum |x_c| / C: the division is one rounding more;
      NORM  2u (K / 2 + 1) |y|: a square's rounding and the K - 1 additions put K u on the sum of squares, RELATIVE,
            because every term is positive; the square root halves it and rounds once more.
    Each plus 2^-126 (a float32 result may be subnormal); float16 plus 2^-11 |ref| + 2^-24 for the one rounding to it."""
    u = 2.0 ** -24
    K = math.ceil(x.shape[0] / 16) + 5
    with np.errstate(all='ignore'):
        a = np.abs(x.astype(np.float64)).sum(axis=0)
        if kind == SUM:
            b = 2 * u * (K - 1) * a
        elif kind == MEAN:
            b = 2 * u * K * a / x.shape[0]
        else:
            b = 2 * u * (K / 2 + 1) * np.abs(ref)
        b = b + 2.0 ** -126
        if x.dtype == np.float16:
            b = b + 2.0 ** -11 * np.abs(ref) + 2.0 ** -24
        return b


values = cr.values      # (the four distributions of the float kinds are those of the channel reductions)


def tie_values(rng, shape, dtype):
    """Values that make ties the rule: drawn from {-2, -1, -0, +0, 1, 2}; the pixels whose flat index is 5 mod 8 --
    one in eight -- hold a NaN in one channel, or in two where C >= 2."""
    Cn = shape[0]
    v = rng.choice(np.array([-2.0, -1.0, -0.0, 0.0, 1.0, 2.0]), size=shape).astype(dtype).reshape(Cn, -1)
    for p in range(5, v.shape[1], 8):
        v[rng.integers(0, Cn, 2), p] = np.nan
    return v.reshape(shape)


def nan_free(x):
    """bool over the pixels of x [C, ...]: no channel is a NaN."""
    return ~np.isnan(x.astype(np.float32)).any(axis=0)


def extreme_in_two_slices(x, kind):
    """bool over the pixels of x [C, n]: the extreme of `kind` is attained in two or more different slices c mod 16."""
    v = x.astype(np.float32)
    at = v == (v.max(axis=0) if kind in (MAX, ARGMAX) else v.min(axis=0))
    slices = np.zeros((16,) + v.shape[1:], dtype=bool)
    for c in range(v.shape[0]):
        slices[c % 16] |= at[c]
    return slices.sum(axis=0) >= 2
