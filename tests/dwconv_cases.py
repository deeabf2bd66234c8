"""Case table of the depthwise stencil (cb_dwconv.hip) and the numpy twin of its per-channel sum.

A case is a geometry, (C, mult) and an OUTPUT map (Ho, Wo); the input map is the smallest that gives it.  `units_of`
restates the launcher's decomposition -- one unit per (mask word, block of 16 output channels), a persistent grid capped
at 8 workgroups per CU -- so that the one case sized to make a workgroup walk several units can be checked for its
regime without a GPU (tests/test_host_dwconv.py).  No expected output is derived from it.

No GPU and no torch in this module.
"""
from collections import namedtuple

import numpy as np
from optest import mask_words      # noqa: F401  (handed on to the tests)

CB_F32, CB_F16 = 0, 1
ARITH = {"F32": CB_F32, "F16": CB_F16}
ACT_NONE, ACT_RELU, ACT_RELU6 = 0, 1, 2

CBLOCK = 16          # CBDW_CB: output channels per unit
CUS = 256            # compute units of an MI355X
GRID_CAP = 8 * CUS   # cbdw_launch: at most 8 workgroups per CU

MAX_K, MAX_S, MAX_D, MAX_P = 7, 4, 8, 64

# geom: ((kH, kW), (sH, sW), (pH, pW), (dH, dW))
GEOMS = {
    "3x3s1p1": ((3, 3), (1, 1), (1, 1), (1, 1)),
    "3x3s2p1": ((3, 3), (2, 2), (1, 1), (1, 1)),
    "5x5s1p2": ((5, 5), (1, 1), (2, 2), (1, 1)),
    "5x5s2p2": ((5, 5), (2, 2), (2, 2), (1, 1)),
    "7x7s1p3": ((7, 7), (1, 1), (3, 3), (1, 1)),
    "3x3d2p2": ((3, 3), (1, 1), (2, 2), (2, 2)),
    "3x3s2d2p2": ((3, 3), (2, 2), (2, 2), (2, 2)),
    "3x3s1p0": ((3, 3), (1, 1), (0, 0), (1, 1)),
    "2x2s2p0": ((2, 2), (2, 2), (0, 0), (1, 1)),
    "4x4s2p1": ((4, 4), (2, 2), (1, 1), (1, 1)),
    "1x1s2p0": ((1, 1), (2, 2), (0, 0), (1, 1)),
    "aniso": ((3, 5), (2, 1), (0, 3), (1, 2)),
    "3x3p3": ((3, 3), (1, 1), (3, 3), (1, 1)),      # a ring of output pixels no tap reaches
}
CMS = [(1, 1), (3, 1), (5, 3), (16, 1), (17, 2), (37, 1)]      # below, at and across the 16-channel block
WOS = [9, 64, 65, 70, 130]
HOS = [1, 5, 13]

Case = namedtuple("Case", "id geom C mult Hi Wi Ho Wo")


def out_size(n, k, s, p, d):
    return (n + 2 * p - d * (k - 1) - 1) // s + 1


def in_size(o, k, s, p, d):
    """The smallest input extent whose output extent is o."""
    return (o - 1) * s + d * (k - 1) + 1 - 2 * p


def propagated_ok(geom):
    k, s, p, d = geom
    return all(d[i] == 1 and 2 * p[i] <= k[i] for i in (0, 1))


def _make(name, C, mult, Ho, Wo):
    k, s, p, d = GEOMS[name]
    Hi, Wi = in_size(Ho, k[0], s[0], p[0], d[0]), in_size(Wo, k[1], s[1], p[1], d[1])
    assert Hi >= 1 and Wi >= 1, (name, Ho, Wo)
    assert (out_size(Hi, k[0], s[0], p[0], d[0]), out_size(Wi, k[1], s[1], p[1], d[1])) == (Ho, Wo)
    return Case("%s-c%dm%d-%dx%d" % (name, C, mult, Ho, Wo), GEOMS[name], C, mult, Hi, Wi, Ho, Wo)


def _table():
    cases, j = [], 0
    for name in GEOMS:
        for _ in range(3):
            C, mult = CMS[j % len(CMS)]
            k, s, p, d = GEOMS[name]
            Ho = HOS[(j // 2) % len(HOS)]
            while in_size(Ho, k[0], s[0], p[0], d[0]) < 1:      # (padding 3: no input map gives fewer than 5 rows)
                Ho = HOS[HOS.index(Ho) + 1]
            cases.append(_make(name, C, mult, Ho, WOS[j % len(WOS)]))
            j += 1
    return cases


CASES = _table()
# more units than the grid takes workgroups: every workgroup walks several units (asserted in test_host_dwconv.py)
WALK = _make("3x3s1p1", 200, 2, 13, 449)
CASES.append(WALK)
CASE_BY_ID = {c.id: c for c in CASES}
assert len(CASE_BY_ID) == len(CASES)


def units_of(c):
    """(units, workgroups) of the stencil launch of a case."""
    units = mask_words(c.Ho, c.Wo) * ((c.C * c.mult + CBLOCK - 1) // CBLOCK)
    return units, min(units, GRID_CAP)


def act_of(v, act):
    """The activation of the header, on float64; a NaN stays a NaN."""
    if act >= ACT_RELU:
        v = np.where(np.isnan(v), v, np.where(v > 0, v, 0.0))
    if act == ACT_RELU6:
        v = np.where(np.isnan(v), v, np.where(v < 6, v, 6.0))
    return v


def twin(x, w, b, geom, mult, act=ACT_NONE):
    """The per-channel sum of the header in float64, in its order: bias (0 without one), then the in-map taps ky outer,
    kx inner.  x [C, Hi, Wi], w [K, 1, kH, kW], b [K] or None -> (out [K, Ho, Wo], mag [K, Ho, Wo] = sum |w||x| + |b|,
    reach [Ho, Wo]: the output pixels with at least one tap inside the input map)."""
    (kH, kW), (sH, sW), (pH, pW), (dH, dW) = geom
    x, w = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64)
    C, Hi, Wi = x.shape
    K = w.shape[0]
    assert K == C * mult and w.shape[1:] == (1, kH, kW)
    Ho, Wo = out_size(Hi, kH, sH, pH, dH), out_size(Wi, kW, sW, pW, dW)
    bias = np.zeros(K) if b is None else np.asarray(b, dtype=np.float64)
    out = np.broadcast_to(bias[:, None, None], (K, Ho, Wo)).copy()
    mag = np.abs(out)
    reach = np.zeros((Ho, Wo), dtype=bool)
    src = x[np.arange(K) // mult]      # [K, Hi, Wi]
    oy, ox = np.arange(Ho), np.arange(Wo)
    for ky in range(kH):
        iy = oy * sH - pH + ky * dH
        oky = (iy >= 0) & (iy < Hi)
        for kx in range(kW):
            ix = ox * sW - pW + kx * dW
            okx = (ix >= 0) & (ix < Wi)
            ok = oky[:, None] & okx[None, :]
            v = src[:, np.clip(iy, 0, Hi - 1)][:, :, np.clip(ix, 0, Wi - 1)]
            wt = w[:, 0, ky, kx][:, None, None]
            out = np.where(ok[None], out + wt * v, out)
            mag = np.where(ok[None], mag + np.abs(wt) * np.abs(v), mag)
            reach |= ok
    return act_of(out, act), mag, reach
