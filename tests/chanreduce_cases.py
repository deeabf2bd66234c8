"""The specification of the change-based per-pixel channel reductions (CBChannelReduce2d, cb_chanreduce.hip, DESIGN.md
5.21) as a numpy float32 twin, the float64 reference, the error bounds, and the shapes and values the host and GPU tests
share.  The reference project has no such operator, so the twin written here IS the specification:
  rule 1  sum16(v): 16 slices, slice s holds the channels c = s mod 16; a slice's partial starts at +0 and adds its
          channels in ascending c; the 16 partials are combined in the fixed tree p[2i] + p[2i+1], four levels.
          max16(v): the same slices and tree with op(a, b) = b > a ? b : a, a slice's partial starting at -inf.
  rule 2  the formulas of twin() below, every operation a float32 one in the order written, never an FMA; the result
          rounded to the map's dtype once;
  rule 3  only listed pixels are written; the frame's mask is handed on, padding bits never set.
The mask patterns are those of tests/pointwise_cases.py.  No GPU is needed to import this file."""
import math

import numpy as np

import pointwise_cases as pc

F32 = np.float32
LAYERNORM, L2NORM, SOFTMAX, LOGSOFTMAX = range(4)
NAMES = ["LAYERNORM", "L2NORM", "SOFTMAX", "LOGSOFTMAX"]
EPS = {LAYERNORM: 1e-6, L2NORM: 1e-12, SOFTMAX: 0.0, LOGSOFTMAX: 0.0}      # the modules' defaults (ConvNeXt's 1e-6)

# [C, H, W]: C below, at and just over the 16 slices and many times over them; W on both sides of a word boundary; the
# last has more mask words than the grid takes workgroups (8 per CU, 256 CUs)
SHAPES = [(1, 1, 9), (3, 5, 64), (16, 5, 9), (17, 1, 65), (40, 1, 130), (300, 5, 130), (5, 2100, 9)]
FORMS = pc.FORMS
patterns, pack, bits_of, same_bits = pc.patterns, pc.pack, pc.bits_of, pc.same_bits


def _tree(p, op):
    assert len(p) == 16
    while len(p) > 1:
        p = [op(p[2 * i], p[2 * i + 1]) for i in range(len(p) // 2)]
    return p[0]


def sum16(v):
    """v float32 [C, ...] -> [...]: written out as loops -- the order IS the specification."""
    assert v.dtype == F32
    parts = [np.zeros(v.shape[1:], dtype=F32) for _ in range(16)]
    for c in range(v.shape[0]):
        parts[c % 16] = parts[c % 16] + v[c]
    out = _tree(parts, lambda a, b: a + b)
    assert out.dtype == F32
    return out


def max16(v):
    assert v.dtype == F32
    op = (lambda a, b: np.where(b > a, b, a))
    parts = [np.full(v.shape[1:], -np.inf, dtype=F32) for _ in range(16)]
    for c in range(v.shape[0]):
        parts[c % 16] = op(parts[c % 16], v[c])
    return _tree(parts, op)


def twin(x, kind, eps=None, gamma=None, beta=None):
    """x [C, H, W] (or [C, n]) float32 or float16 -> the operator `kind` over axis 0 in x's dtype; gamma, beta float32
    [C] (LAYERNORM only, both or neither); eps: the module's value (rounded to float32 here)."""
    assert x.dtype in (np.float32, np.float16)
    eps = F32(EPS[kind] if eps is None else eps)
    Cn = x.shape[0]
    fC = F32(Cn)
    col = (slice(None),) + (None,) * (x.ndim - 1)
    with np.errstate(all='ignore'):
        v = x.astype(F32)
        if kind == LAYERNORM:
            mean = sum16(v) / fC
            d = v - mean
            var = sum16(d * d) / fC
            r = F32(1) / np.sqrt(var + eps)
            y = d * r
            if gamma is not None:
                assert gamma.dtype == F32 and beta.dtype == F32
                y = y * gamma[col]      # (rounded to float32 here ...
                y = y + beta[col]       #  ... and here)
        elif kind == L2NORM:
            t = np.sqrt(sum16(v * v))
            y = v / np.where(t < eps, eps, t)
        else:
            m = max16(v)
            a = v - m
            e = np.exp(a)
            s = sum16(e)
            y = e / s if kind == SOFTMAX else a - np.log(s)
        assert y.dtype == F32
        return y.astype(x.dtype)


def reference64(x, kind, eps=None, gamma=None, beta=None):
    """The same formulas in float64 (numpy's own sums): the operator's mathematical value on the stored inputs."""
    eps = float(F32(EPS[kind] if eps is None else eps))
    col = (slice(None),) + (None,) * (x.ndim - 1)
    with np.errstate(all='ignore'):
        v = x.astype(np.float64)
        if kind == LAYERNORM:
            d = v - v.mean(axis=0)
            y = d / np.sqrt((d * d).mean(axis=0) + eps)
            if gamma is not None:
                y = y * gamma.astype(np.float64)[col] + beta.astype(np.float64)[col]
            return y
        if kind == L2NORM:
            return v / np.maximum(np.sqrt((v * v).sum(axis=0)), eps)
        a = v - v.max(axis=0)
        s = np.exp(a).sum(axis=0)
        return np.exp(a) / s if kind == SOFTMAX else a - np.log(s)


def bound(x, kind, ref, eps=None, gamma=None, beta=None):
    """The error bound of a result of dtype x.dtype against ref = reference64(x, ...), per value.  u = 2^-24 is what one
    correctly rounded float32 operation adds relative to its result; K = ceil(C / 16) + 5 covers the additions a value
    passes through in sum16 (ceil(C / 16) in its slice, four in the tree) and the division by C; first order, taken
    twice.  With M = mean |x_c|, r = 1 / sqrt(var + eps), A = max |a_c|:
      LAYERNORM   2u (K M r (1 + |y|) + (K + 6) |y|): the error of the mean, K u M, moves every d_c and enters y with
                  weight r -- this is the cancellation term -- and the variance once more with weight |y|; the rest is
                  relative to y.  With gamma, beta the two further roundings add u |y gamma| and u |z|, and the error of
                  y is scaled by |gamma|:  |gamma| bound(y) + 2u (|y gamma| + |z|);
      L2NORM      2u (K / 2 + 4) |y|: the square root halves the sum's relative error;
      SOFTMAX     2u (|a_c| + A + 24 + K + 1) |y|: the rounding of a_c = x_c - m is amplified by expf's condition
                  number |a_c| (and up to A in the sum), expf itself at the OpenCL full profile's 3 ulp = 12 u, in e_c and
                  in s (DESIGN 5.16 argues the figure), the sum's K, the division;
      LOGSOFTMAX  2u (|a_c| + A + 12 + K + 12 |log s| + |y|), absolute: a_c's rounding, the sum's relative error
                  (A + 12 + K) through log's derivative 1 / s <= 1 relative, logf at 3 ulp of |log s|, the subtraction.
    Each plus 2^-126 (a float32 result may be subnormal); float16 plus 2^-11 |ref| + 2^-24 for the one rounding to it."""
    eps = float(F32(EPS[kind] if eps is None else eps))
    u = 2.0 ** -24
    col = (slice(None),) + (None,) * (x.ndim - 1)
    with np.errstate(all='ignore'):
        v = x.astype(np.float64)
        K = math.ceil(x.shape[0] / 16) + 5
        if kind == LAYERNORM:
            d = v - v.mean(axis=0)
            r = 1.0 / np.sqrt((d * d).mean(axis=0) + eps)
            y = d * r
            b = 2 * u * (K * np.abs(v).mean(axis=0) * r * (1 + np.abs(y)) + (K + 6) * np.abs(y))
            if gamma is not None:
                g = gamma.astype(np.float64)[col]
                b = np.abs(g) * b + 2 * u * (np.abs(y * g) + np.abs(ref))
        elif kind == L2NORM:
            b = 2 * u * (K / 2 + 4) * np.abs(ref)
        else:
            a = v - v.max(axis=0)
            logs = np.log(np.exp(a).sum(axis=0))
            # (a -inf channel has e_c = 0 without an error: it counts as |a_c| = 0, which only tightens the bound)
            a = np.where(np.isfinite(a), np.abs(a), 0.0)
            A = a.max(axis=0)
            if kind == SOFTMAX:
                b = 2 * u * (a + A + 24 + K + 1) * np.abs(ref)
            else:
                b = 2 * u * (a + A + 12 + K + 12 * np.abs(logs) + np.where(np.isfinite(ref), np.abs(ref), 0.0))
        b = b + 2.0 ** -126
        if x.dtype == np.float16:
            b = b + 2.0 ** -11 * np.abs(ref) + 2.0 ** -24
        return b


def affine(rng, C):
    """(gamma, beta) float32 [C]: gammas of both signs away from 0."""
    gamma = (rng.uniform(0.5, 2.0, C) * rng.choice([-1.0, 1.0], C)).astype(F32)
    return gamma, rng.uniform(-3.0, 3.0, C).astype(F32)


def values(rng, shape, dtype, span=8.0, special=None):
    """pointwise_cases.values with ONE difference: the special values are placed per PIXEL -- about one pixel in eight
    gets one special in one channel (with per-value specials and C = 300 every pixel would hold a NaN) --; every special
    at least once where the map has that many pixels."""
    Cn = shape[0]
    v = rng.uniform(-span, span, shape)
    small = rng.random(shape) < 0.2
    v[small] = rng.standard_normal(int(small.sum())) * 1e-3
    v = v.astype(dtype).reshape(Cn, -1)
    sp = pc.specials(dtype) if special is None else special
    P = v.shape[1]
    pix = np.flatnonzero(rng.random(P) < 0.125)
    v[rng.integers(0, Cn, len(pix)), pix] = rng.choice(sp, len(pix))
    if P >= len(sp):
        pix = rng.choice(P, len(sp), replace=False)
        v[rng.integers(0, Cn, len(sp)), pix] = sp
    return v.reshape(shape)


def finite_pixels(x):
    """bool over the pixels of x [C, ...]: every channel is finite."""
    return np.isfinite(x.astype(np.float32)).all(axis=0)
