"""The numpy twin of the resize section of include/cbinfer_hip.h (cb_resize.hip), its footprint by brute
force, and the shape table the host and GPU tests share.  No torch here.

A resize is described by a plain object with the fields of cbResize -- Ho, Wo, aH, bH, aW, bW, mode, alignCorners -- as
`Resize` below makes it; mode is one of the CB_RESIZE_* numbers."""
import collections
import fractions
import math

import numpy as np

NEAREST, NEAREST_EXACT, BILINEAR, BICUBIC = range(4)      # CB_RESIZE_*
KINDS = {NEAREST: 'nearest', NEAREST_EXACT: 'nearest-exact', BILINEAR: 'bilinear', BICUBIC: 'bicubic'}
# the six modes of the tests: (mode, alignCorners)
MODES = [(NEAREST, 0), (NEAREST_EXACT, 0), (BILINEAR, 0), (BILINEAR, 1), (BICUBIC, 0), (BICUBIC, 1)]
MODE_IDS = ['nearest', 'nearest-exact', 'bilinear', 'bilinear-aligned', 'bicubic', 'bicubic-aligned']

Resize = collections.namedtuple('Resize', 'Ho Wo aH bH aW bW mode alignCorners')

#   C, Hi, Wi -> Ho, Wo
SHAPES = [
    (1, 1, 1, 1, 1),          # smallest map
    (1, 1, 1, 5, 8),          # every tap clamps to one pixel
    (2, 5, 8, 1, 1),          # N == 1 with align_corners
    (3, 5, 13, 13, 31),       # fractional upscale
    (3, 13, 31, 5, 13),       # fractional downscale
    (2, 3, 32, 3, 64),        # exactly one output word
    (2, 4, 22, 7, 66),        # a footprint across the word boundary
    (2, 3, 70, 4, 11),        # one output word reads two input words
    (1, 2, 9, 16, 72),        # x8, the limit
    (1, 16, 130, 2, 17),      # /7.6, lanes spanning three input words
    (1, 1050, 9, 2100, 9),    # more output words than workgroups
]
STRIDED = (1, 1050, 9, 2100, 9)
# scale_factor cases on a (2, 6, 13) map, without recompute_scale_factor
SCALE_SHAPE = (2, 6, 13)
SCALES = [1.5, 0.75, (2.5, 0.5)]


def shape_id(s):
    return "%dx%dx%d-to-%dx%d" % s


def step_of_size(n, N):
    """The reduced step a / b = n / N of a resize to a size."""
    f = fractions.Fraction(n, N)
    return f.numerator, f.denominator


def resize_of_size(Hi, Wi, Ho, Wo, mode, align):
    aH, bH = step_of_size(Hi, Ho)
    aW, bW = step_of_size(Wi, Wo)
    return Resize(Ho, Wo, aH, bH, aW, bW, mode, align)


def resize_of_scale(Hi, Wi, scale, mode, align):
    """torch's rule for a scale_factor without recompute: N = floor(n sf), a / b = 1 / sf exactly."""
    sH, sW = scale if isinstance(scale, tuple) else (scale, scale)
    fH, fW = 1 / fractions.Fraction(sH), 1 / fractions.Fraction(sW)
    return Resize(int(math.floor(Hi * sH)), int(math.floor(Wi * sW)), fH.numerator, fH.denominator, fW.numerator,
                  fW.denominator, mode, align)


# ---------------------------------------------------------------------------------------------------- source rule
def source(kind, align, o, n, N, a, b):
    """(taps, rho, den) of output coordinate o on an axis of n input and N output pixels with the step a / b: the clamped
    input coordinates it reads and the weight fraction t = rho / den -- python integers, the header's rules."""
    if kind == NEAREST:
        return [min(o * a // b, n - 1)], 0, 1
    if kind == NEAREST_EXACT:
        return [min((2 * o + 1) * a // (2 * b), n - 1)], 0, 1
    if not align:
        num, den = (2 * o + 1) * a - b, 2 * b
    else:
        num, den = (o * (n - 1), N - 1) if N > 1 else (0, 1)
    if kind == BILINEAR:
        num = max(num, 0)
        i0 = num // den
        return [min(i0, n - 1), min(i0 + 1, n - 1)], num - i0 * den, den
    i0 = num // den      # (python's // floors)
    return [min(max(i0 - 1 + k, 0), n - 1) for k in range(4)], num - i0 * den, den


def axis_table(kind, align, n, N, a, b):
    """Per output coordinate of an axis: taps [N, T] and (rho, den) [N, 2]."""
    rows = [source(kind, align, o, n, N, a, b) for o in range(N)]
    return (np.array([r[0] for r in rows], dtype=np.int64).reshape(N, -1),
            np.array([[r[1], r[2]] for r in rows], dtype=np.int64).reshape(N, 2))


# ---------------------------------------------------------------------------------------------------- values
def _weights(kind, frac, dt):
    """The weights [N, T] of an axis from its (rho, den), in `dt`: float32 operation by operation as the header writes
    them out, or the same formulas in float64."""
    f = dt
    t = (frac[:, 0].astype(f) / frac[:, 1].astype(f)).astype(f)      # one correctly rounded division
    one = f(1)
    if kind == BILINEAR:
        return np.stack([one - t, t], axis=1)

    def far(s):
        m = f(-0.75) * s
        m = m - f(-3.75)
        m = m * s
        m = m + f(-6)
        m = m * s
        return m - f(-3)

    def near(u):
        m = f(1.25) * u
        m = m - f(2.25)
        m = m * u
        m = m * u
        return m + one
    return np.stack([far(t + one), near(t), near(one - t), far(f(2) - t)], axis=1)


def _combine(w, p):
    """((w0 p0 + w1 p1) + w2 p2) + w3 p3 along the last axis, every product and sum in the arrays' dtype."""
    acc = w[..., 0] * p[..., 0]
    for k in range(1, w.shape[-1]):
        acc = acc + w[..., k] * p[..., k]
    return acc


def twin(x, rs, npdt):
    """The resize `rs` of x [C, Hi, Wi] (float32 or float16).  npdt=np.float32: the kernel's arithmetic operation by
    operation, rounded to x's dtype once -- equal to the device bit for bit; np.float64: the same rules in float64, not
    rounded."""
    C, Hi, Wi = x.shape
    ty, fy = axis_table(rs.mode, rs.alignCorners, Hi, rs.Ho, rs.aH, rs.bH)
    tx, fx = axis_table(rs.mode, rs.alignCorners, Wi, rs.Wo, rs.aW, rs.bW)
    if rs.mode in (NEAREST, NEAREST_EXACT):
        return x[:, ty[:, 0]][:, :, tx[:, 0]].copy()
    wy, wx = _weights(rs.mode, fy, npdt), _weights(rs.mode, fx, npdt)
    xs = x.astype(npdt)
    # p[c, oy, k, ox, j] = x[c, ty[oy, k], tx[ox, j]]
    p = xs[:, ty][:, :, :, tx]
    rows = _combine(wx[None, None, None], p)                      # [C, Ho, T, Wo]: first over x
    out = _combine(wy[None, :, None, :], np.moveaxis(rows, 2, 3))  # [C, Ho, Wo]: then over y
    return out.astype(x.dtype) if npdt is np.float32 else out


def tap_abs_max(x, rs):
    """max |x| over the taps of every output pixel, [Ho, Wo] (over all channels): the scale of the error bar."""
    C, Hi, Wi = x.shape
    ty, _ = axis_table(rs.mode, rs.alignCorners, Hi, rs.Ho, rs.aH, rs.bH)
    tx, _ = axis_table(rs.mode, rs.alignCorners, Wi, rs.Wo, rs.aW, rs.bW)
    a = np.abs(x.astype(np.float64)).max(axis=0)
    return a[ty][:, :, tx].max(axis=(1, 3))


# ---------------------------------------------------------------------------------------------------- footprint
def footprint(changed, rs):
    """The listed output pixels [Ho, Wo] of a bool change map [Hi, Wi], by brute force: (oy, ox) is listed iff any of its
    clamped taps is, zero weights included."""
    Hi, Wi = changed.shape
    out = np.zeros((rs.Ho, rs.Wo), dtype=bool)
    rows = [source(rs.mode, rs.alignCorners, oy, Hi, rs.Ho, rs.aH, rs.bH)[0] for oy in range(rs.Ho)]
    cols = [source(rs.mode, rs.alignCorners, ox, Wi, rs.Wo, rs.aW, rs.bW)[0] for ox in range(rs.Wo)]
    for oy in range(rs.Ho):
        for ox in range(rs.Wo):
            out[oy, ox] = any(changed[y, x] for y in rows[oy] for x in cols[ox])
    return out


def candidates(i, n, N, a, b, align):
    """The candidate output coordinates of input coordinate i, the list kernel's range: ceil(6 q) + 3 coordinates from
    floor((i - 3) q) - 1 on, q = b / a output pixels per input pixel (N / n with align_corners)."""
    qa, qb = (n, N) if align else (a, b)
    first = ((i - 3) * qb) // qa - 1
    count = -((-6 * qb) // qa) + 3
    return range(max(first, 0), min(first + count, N))


def footprint_by_candidates(changed, rs):
    """The same footprint as the list kernel builds it: per changed pixel its candidate rows and columns, each TESTED
    with the source rule.  Equal to footprint() iff the candidate ranges hold every reader."""
    Hi, Wi = changed.shape
    out = np.zeros((rs.Ho, rs.Wo), dtype=bool)
    for y, x in zip(*np.nonzero(changed)):
        oys = [o for o in candidates(y, Hi, rs.Ho, rs.aH, rs.bH, rs.alignCorners)
               if y in source(rs.mode, rs.alignCorners, o, Hi, rs.Ho, rs.aH, rs.bH)[0]]
        oxs = [o for o in candidates(x, Wi, rs.Wo, rs.aW, rs.bW, rs.alignCorners)
               if x in source(rs.mode, rs.alignCorners, o, Wi, rs.Wo, rs.aW, rs.bW)[0]]
        assert not oxs or (oxs[-1] >> 6) - (oxs[0] >> 6) <= 1      # (two words at most)
        for oy in oys:
            out[oy, oxs] = True
    return out
