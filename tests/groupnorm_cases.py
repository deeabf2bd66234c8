"""The specification of the change-based group norm (CBGroupNorm2d, cb_groupnorm.hip) as a numpy twin,
the error bound against float64 math, and the shapes the host and GPU tests share.  The reference project has no such
operator, so the twin written here IS the specification:
  rule 1  level 1: P[k][c][y][tile], float64, the sum of x (k = 0) and of x x (k = 1) over the 64-column segment `tile`
          of row y by the butterfly p_l + p_(l xor m), m = 1 ... 32, columns >= W contributing +0 (segment_partials);
          a frame recomputes exactly the partials of the segments whose listed word is not zero (update_partials);
  rule 2  level 2: a group's partials are contiguous; 1024 lane sums by index mod 1024 in ascending order from +0, then
          the tree s_l += s_(l + off), off = 512 ... 1; mean = S1 / n, var = max(S2 / n - mean mean, 0) (a NaN stays),
          rstd = 1 / sqrt(var + eps), all float64, each rounded once to float32 (statistics);
  rule 3  group g trips iff `all`, or not |mean - heldMean| heldRstd <= threshold, or not |rstd - heldRstd| <=
          threshold heldRstd, in float32 (strictly more; a NaN trips); a tripped group takes both new values, any other
          keeps both bit for bit (rule);
  rule 4  out = (T)(relu(((float(x) - heldMean) heldRstd) gamma[c] + beta[c])), every operation a float32 operation of
          its own (values), written at a listed pixel for every channel and at every other pixel for the channels of the
          tripped groups; every other element keeps its bits;
  rule 5  the frame's mask is the listed pixels, or every pixel in a frame in which a group tripped.
step() takes the frame's statistics AS THE DEVICE WROTE THEM: the device's float64 division and square root need not be
correctly rounded, and a trip decision must not depend on that.  No GPU is needed to import this file."""
import math

import numpy as np

import pointwise_cases as pc

F32, F64 = np.float32, np.float64
# (C, G): GroupNorm(1, C), two groups, an instance norm, and a group of 16 channels -- one whole channel block of launch
# 1 per group, three blocks in all
CASES = [(4, 1), (6, 2), (6, 6), (48, 3)]
# H x W: one, two and three mask words per row, the last word ragged
MAPS = [(5, 7), (9, 70), (3, 130)]
FORMS = pc.FORMS
pack, bits_of, same_bits = pc.pack, pc.bits_of, pc.same_bits
EPS = 1e-5


def segment_partials(a):
    """P [2, C, H, wpr] float64 of a [C, H, W] (float32 or float16): the butterfly over the 64 lanes of every segment."""
    Cn, H, W = a.shape
    wpr = (W + 63) // 64
    x = np.zeros((Cn, H, wpr * 64), dtype=F64)      # (columns >= W: +0)
    x[:, :, :W] = a.astype(F64)
    lanes = np.arange(64)
    with np.errstate(all='ignore'):
        p = np.stack([x, x * x]).reshape(2, Cn, H, wpr, 64)      # (the square of a float32 is exact in float64)
        for m in (1, 2, 4, 8, 16, 32):
            p = p + p[..., lanes ^ m]
    return np.ascontiguousarray(p[..., 0])


def dirty_segments(listed):
    """bool [H, wpr]: the segments whose word of the listed pixels is not zero."""
    H, W = listed.shape
    wpr = (W + 63) // 64
    pad = np.zeros((H, wpr * 64), dtype=bool)
    pad[:, :W] = listed
    return pad.reshape(H, wpr, 64).any(axis=-1)


def update_partials(P, a, listed):
    """The partials after a frame: recomputed in the dirty segments (for every channel), kept bit for bit elsewhere."""
    return np.where(dirty_segments(listed)[None, None], segment_partials(a), P)


def _sum1024(x):
    """The level-2 sum of the float64 items x [N] in the written order."""
    n = len(x)
    rows = -(-n // 1024)
    pad = np.zeros(rows * 1024, dtype=F64)      # (a lane without an item keeps its sum: s + (+0) == s, s is never -0)
    pad[:n] = x
    with np.errstate(all='ignore'):
        s = np.zeros(1024, dtype=F64)
        for r in pad.reshape(rows, 1024):
            s = s + r
        off = 512
        while off >= 1:
            s = s[:off] + s[off:2 * off]
            off //= 2
    return s[0]


def statistics(P, G, H, W, eps=EPS):
    """stats [2, G] float32 -- means, rstds -- of the partials P [2, C, H, wpr]."""
    Cn = P.shape[1]
    Cg = Cn // G
    n = F64(Cg * H * W)
    stats = np.zeros((2, G), dtype=F32)
    with np.errstate(all='ignore'):
        for g in range(G):
            S1 = _sum1024(P[0, g * Cg:(g + 1) * Cg].reshape(-1))
            S2 = _sum1024(P[1, g * Cg:(g + 1) * Cg].reshape(-1))
            mean = S1 / n
            var = S2 / n - mean * mean
            var = F64(0) if var < 0 else var      # (a NaN stays)
            rstd = F64(1) / np.sqrt(var + F64(eps))
            stats[0, g], stats[1, g] = F32(mean), F32(rstd)
    return stats


def statistics_f32(a, G, eps=EPS):
    """The same two levels with every sum, product and quotient in float32: what the float64 level is there to avoid.
    E[x^2] - mean^2 cancels in float32 when the mean is large against the spread."""
    Cn, H, W = a.shape
    wpr = (W + 63) // 64
    x = np.zeros((Cn, H, wpr * 64), dtype=F32)
    x[:, :, :W] = a.astype(F32)
    lanes = np.arange(64)
    p = np.stack([x, x * x]).reshape(2, Cn, H, wpr, 64)
    for m in (1, 2, 4, 8, 16, 32):
        p = p + p[..., lanes ^ m]
    P = p[..., 0]
    Cg = Cn // G
    n = F32(Cg * H * W)
    stats = np.zeros((2, G), dtype=F32)
    for g in range(G):
        S = []
        for k in (0, 1):
            items = P[k, g * Cg:(g + 1) * Cg].reshape(-1)
            pad = np.zeros(-(-len(items) // 1024) * 1024, dtype=F32)
            pad[:len(items)] = items
            s = np.zeros(1024, dtype=F32)
            for r in pad.reshape(-1, 1024):
                s = s + r
            off = 512
            while off >= 1:
                s = s[:off] + s[off:2 * off]
                off //= 2
            S.append(s[0])
        mean = S[0] / n
        var = S[1] / n - mean * mean
        var = F32(0) if var < 0 else var
        stats[0, g], stats[1, g] = mean, F32(1) / np.sqrt(var + F32(eps))
    assert stats.dtype == F32
    return stats


def rule(stats, held, threshold, all):
    """(held after the frame [2, G], tripped bool [G]) in float32."""
    assert stats.dtype == F32 and held.dtype == F32 and stats.shape == held.shape
    th = F32(threshold)
    with np.errstate(all='ignore'):
        dm = np.abs(stats[0] - held[0]) * held[1]
        dr = np.abs(stats[1] - held[1])
        lim = th * held[1]
        assert dm.dtype == F32 and dr.dtype == F32 and lim.dtype == F32
        tripped = np.ones(stats.shape[1], dtype=bool) if all else (~(dm <= th) | ~(dr <= lim))
    return np.where(tripped[None, :], stats, held).astype(F32), tripped


def values(a, held, G, gamma=None, beta=None, relu=False):
    """rule 4 at every element of a [C, H, W]."""
    Cn = a.shape[0]
    grp = np.arange(Cn) // (Cn // G)
    with np.errstate(all='ignore'):
        v = a.astype(F32) - held[0][grp][:, None, None]
        v = v * held[1][grp][:, None, None]
        if gamma is not None:
            assert gamma.dtype == F32
            v = v * gamma[:, None, None]
        if beta is not None:
            assert beta.dtype == F32
            v = v + beta[:, None, None]
        if relu:
            v = np.where(v < 0, F32(0), v)
        assert v.dtype == F32
        return v.astype(a.dtype)


def step(a, statsNow, held, listed, threshold, all, G, gamma=None, beta=None, relu=False, prev=None):
    """One frame given the statistics of the frame (the twin's own, or as the device wrote them).  a [C, H, W]; held
    the pairs before the frame; listed bool [H, W] the operand's changed pixels (every pixel for an operand without
    change information); all: a fresh state.  Returns (held after the frame, tripped bool [G], out at EVERY element,
    mask bool [H, W], written bool [C, H, W]).  With prev -- the state before the frame -- an element that is not written
    keeps prev's value."""
    Cn = a.shape[0]
    new, tripped = rule(statsNow, held, threshold, all)
    listed = np.ones(a.shape[1:], dtype=bool) if all else listed
    written = listed[None, :, :] | np.repeat(tripped, Cn // G)[:, None, None]
    out = values(a, new, G, gamma, beta, relu)
    if prev is not None:
        out = np.where(written, out, prev)
    mask = np.ones_like(listed) if tripped.any() else listed.copy()
    return new, tripped, out, mask, written


def reference64(a, G, eps=EPS, gamma=None, beta=None, relu=False):
    """(v, y, mean, rstd) of the dense operator in float64 on the stored operand: v the result, y the normalised value
    before the affine, mean / rstd per channel [C, 1, 1].  (The tests check it against F.group_norm in float64.)"""
    Cn, H, W = a.shape
    x = a.astype(F64).reshape(G, -1)
    mean = x.mean(axis=1)
    var = ((x - mean[:, None]) ** 2).mean(axis=1)
    rstd = 1.0 / np.sqrt(var + eps)
    grp = np.arange(Cn) // (Cn // G)
    m, r = mean[grp][:, None, None], rstd[grp][:, None, None]
    y = (a.astype(F64) - m) * r
    v = y.copy()
    if gamma is not None:
        v = v * gamma.astype(F64)[:, None, None]
    if beta is not None:
        v = v + beta.astype(F64)[:, None, None]
    if relu:
        v = np.maximum(v, 0.0)
    return v, y, m, r


def bound(a, G, eps=EPS, gamma=None, beta=None, relu=False):
    """The first-order bound of the threshold-0 result against reference64(), per element, built as
    chanscale_cases.excite_bound builds its own.  u = 2^-24 is what one correctly rounded float32 operation adds relative
    to its result, w = 2^-53 the same for float64.
      the float64 sums: a value passes K = 6 + ceil(N / 1024) + 10 additions on its way into S1 or S2 (butterfly, lane
        sum, tree; N the group's partials), each relative to a partial sum that the sum of the magnitudes bounds, and one
        division; so  E(S1 / n) = (K + 1) w mean|x|,  E(S2 / n) = (K + 1) w mean(x^2);
      mean:  E_m = u |mean| + (K + 1) w mean|x|                                   (its rounding to float32, the sums);
      var = S2 / n - mean mean:  E_var = (K + 4) w (mean(x^2) + 2 |mean| mean|x| + mean^2)
      rstd = 1 / sqrt(var + eps): relative  e_r = u + E_var / (2 (var + eps)) + 4 w      (its rounding to float32, the
        variance at the slope of the inverse root, the addition, the root and the division);
      y = fl(fl(x - mean) rstd):  E_y = rstd E_m + |y| (2u + e_r)                  (two of the four value roundings);
      v = fl(fl(y gamma) + beta): E_v = |gamma| E_y + u |y gamma| + u |v|          (the other two; the ReLU is exact
        and 1-Lipschitz, so the bound of v holds behind it);
      the half ulp of T: 2^-11 |v| and half the smallest subnormal, 2^-25, for float16; nothing for float32 (the
        conversion is exact); plus 2^-126 (a float32 result may be subnormal);
    times 1.01 for the second-order terms."""
    u, w = 2.0 ** -24, 2.0 ** -53
    Cn, H, W = a.shape
    Cg = Cn // G
    v, y, m, r = reference64(a, G, eps, gamma, beta, relu=False)
    x = np.abs(a.astype(F64)).reshape(G, -1)
    K = 6 + math.ceil(Cg * H * ((W + 63) // 64) / 1024) + 10
    grp = np.arange(Cn) // Cg
    ax = x.mean(axis=1)[grp][:, None, None]
    ax2 = (x * x).mean(axis=1)[grp][:, None, None]
    Em = u * np.abs(m) + (K + 1) * w * ax
    Evar = (K + 4) * w * (ax2 + 2 * np.abs(m) * ax + m * m)
    er = u + 0.5 * Evar * r * r + 4 * w      # (r r = 1 / (var + eps))
    Ey = r * Em + np.abs(y) * (2 * u + er)
    g = np.abs(gamma.astype(F64))[:, None, None] if gamma is not None else 1.0
    Ev = g * Ey + (u * np.abs(y) * g if gamma is not None else 0.0) + (u * np.abs(v) if beta is not None else 0.0)
    if a.dtype == np.float16:
        Ev = Ev + 2.0 ** -11 * np.abs(v) + 2.0 ** -25
    return 1.01 * (Ev + 2.0 ** -126)


def ulps(a, b):
    """The distance of two float32 arrays in units of the last place (both finite, same sign or zero)."""
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    return np.abs(ia - ib)


def affine(rng, Cn):
    """(gamma, beta) float32 [C]: scales of both signs away from 0."""
    gamma = (rng.uniform(0.5, 2.0, Cn) * rng.choice([-1.0, 1.0], Cn)).astype(F32)
    return gamma, rng.uniform(-1.0, 1.0, Cn).astype(F32)


def frame_script(rng, Cn, G, H, W, dtype, threshold):
    """Five consecutive frames as (label, a [C, H, W], listed bool [H, W]): fresh; a sparse change (a tenth of the
    pixels rewritten with values a hundredth of a standard deviation away); an empty frame; a drift of every group's
    mean by 0.3 threshold standard deviations; a frame in which the LAST group's mean moves by 3 threshold standard
    deviations and no other group's channels change.  The moves are sums over the listed pixels, so that the statistics
    move while most segments stay clean.  The caller asserts the twin's trip sequence: all, none, none, none, the last."""
    Cg = Cn // G
    a = (rng.standard_normal((Cn, H, W)) + rng.uniform(-1, 1, Cn)[:, None, None]).astype(dtype)
    frames = [("fresh", a.copy(), np.zeros((H, W), dtype=bool))]
    std = a.astype(F64).reshape(G, -1).std(axis=1)

    def some_pixels():
        S = rng.random((H, W)) < 0.1
        S[int(rng.integers(H)), int(rng.integers(W))] = True
        return S

    def move(a, S, shift, groups):
        """The mean of each of `groups` moved by about `shift` standard deviations, at the pixels S alone."""
        new = a.copy()
        for g in groups:
            delta = shift * std[g] * (H * W) / S.sum()
            new[g * Cg:(g + 1) * Cg][:, S] = (a[g * Cg:(g + 1) * Cg][:, S].astype(F64) + delta).astype(dtype)
        return new

    S = some_pixels()
    a = a.copy()
    a[:, S] = (a[:, S].astype(F64) + 0.01 * rng.choice([-1.0, 1.0], (Cn, int(S.sum())))).astype(dtype)
    frames.append(("sparse change", a.copy(), S))
    frames.append(("empty", a.copy(), np.zeros((H, W), dtype=bool)))
    S = some_pixels()
    a = move(a, S, 0.3 * threshold, range(G))
    frames.append(("drift", a.copy(), S))
    S = some_pixels()
    a = move(a, S, 3.0 * threshold, [G - 1])
    frames.append(("one group trips", a.copy(), S))
    return frames
