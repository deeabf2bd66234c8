"""Case table of the general-geometry contraction and detection (cb_geomconv.hip) and a classifier of the regime a shape
lands in.

`geom_form` restates the DEVICE formulas at the top of cbg_conv_kernel (KP, CkkP, stages, tilesN, tilesM, base, SK,
items, chunk) and the padding of cbinfer_geom_*.  CBG_GRID is a constant 512, so nothing here depends on the card.  It
is a classifier only: it says which k-split, item schedule and mask scan a case exercises, so that the table can be
checked for coverage without a GPU (tests/test_host_geomconv.py) and so that a change of the heuristics that moves a
case into another regime makes tests/test_gpu_geomconv.py fail loudly.  No expected output is ever derived from it.

No GPU and no torch in this module.
"""
import zlib
from collections import namedtuple

import numpy as np
from optest import mask_words      # noqa: F401  (handed on to the tests)

CB_F32, CB_F16, CB_F32S = 0, 1, 2
ARITH = {"F32": CB_F32, "F16": CB_F16, "F32S": CB_F32S}

GRID = 512           # CBG_GRID
BM = BN = 64         # CBG_BM, CBG_BN
BK = 32              # CBG_BK
SKMAX = 8            # CBG_SKMAX
SCAN = 256           # threads of the mask scan: chunk = ceil(words / 256) words per thread

REGIMES = ("nows", "one_stage", "sk_stages", "sk_cap8", "sk_grid", "full", "multi_item")
MASK_CLASSES = ("<=256", "257..512", ">512")


def out_size(n, k, s, p, d):
    return (n + 2 * p - d * (k - 1) - 1) // s + 1


def geom_form(K, C, kH, kW, N, has_workspace, words):
    """N: the change count the kernel sees; words: mask words of the output map (0 in list mode)."""
    KP = (K + BM - 1) // BM * BM
    Ckk = C * kH * kW
    CkkP = (Ckk + BK - 1) // BK * BK
    stages = CkkP // BK
    tilesN, tilesM = (N + BN - 1) // BN, KP // BM
    base = tilesN * tilesM
    SK = 1
    if has_workspace and 0 < base < GRID:
        SK = max(1, min(GRID // base, SKMAX, stages))
    chunk = (words + SCAN - 1) // SCAN
    return dict(KP=KP, Ckk=Ckk, CkkP=CkkP, stages=stages, tilesN=tilesN, tilesM=tilesM, base=base, SK=SK,
                items=base * SK, chunk=chunk, words=words, scan_threads=-(-words // chunk) if chunk else 0)


def regime_of(f, has_workspace):
    """'nows': no workspace, SK = 1; 'multi_item': base > 512, a workgroup walks several tiles; 'full':
    257 <= base <= 512, SK = 1, one item or none per workgroup; 'one_stage': base <= 256, but one 32-deep stage; 'sk_cap8':
    SK = 8; 'sk_stages': 2 <= SK = stages < 8; 'sk_grid': 2 <= SK = 512 // base, below both other caps."""
    if not has_workspace:
        return "nows"
    if f["base"] > GRID:
        return "multi_item"
    if f["base"] >= 257:
        assert f["SK"] == 1
        return "full"
    if f["stages"] == 1:
        return "one_stage"
    if f["SK"] == SKMAX:
        return "sk_cap8"
    if f["SK"] == f["stages"]:
        return "sk_stages"
    assert f["SK"] == GRID // f["base"] < min(SKMAX, f["stages"])
    return "sk_grid"


def mask_class_of(words):
    if words == 0:
        return None
    return "<=256" if words <= 256 else "257..512" if words <= 512 else ">512"


# -------------------------------------------------------------------------------------------------------------------
# contraction cases
# -------------------------------------------------------------------------------------------------------------------
# geom: ((kH, kW), (sH, sW), (pH, pW), (dH, dW)); Hi x Wi: the INPUT map.
# pixels (on the OUTPUT map): ('rand', N) N distinct pixels; ('all',); ('last',) the one pixel on the last valid bit of
# the last mask word; ('chunks', (i, ...), N) N pixels, all inside the scan chunks i of the mask (the words
# [i * chunk, (i + 1) * chunk)), every other chunk empty.
# count: the change-count class the case claims ('1', '63', '64', '65', 'all', 'sparse' or None).
Case = namedtuple("Case", "id arith source K C geom Hi Wi pixels ws regime mask_class count")

G3 = ((3, 3), (1, 1), (1, 1), (1, 1))            # output map = input map
G1 = ((1, 1), (1, 1), (0, 0), (1, 1))
G3S2 = ((3, 3), (2, 2), (1, 1), (1, 1))
G3D2 = ((3, 3), (1, 1), (2, 2), (2, 2))
G3P0 = ((3, 3), (1, 1), (0, 0), (1, 1))
G4S4 = ((4, 4), (4, 4), (0, 0), (1, 1))
G7S2 = ((7, 7), (2, 2), (3, 3), (1, 1))
G7D8 = ((7, 7), (1, 1), (24, 24), (8, 8))        # the widest reach: 49 taps over 49 x 49 pixels
G3S4D8 = ((3, 3), (4, 4), (8, 8), (8, 8))
G3P3 = ((3, 3), (1, 1), (3, 3), (1, 1))          # a ring of output pixels no tap reaches


def _c(id, arith, source, K, C, geom, Hi, Wi, pixels, ws, regime, mask_class=None, count=None):
    assert (source == "mask") == (mask_class is not None)
    return Case(id, arith, source, K, C, geom, Hi, Wi, pixels, ws, regime, mask_class, count)


CASES = [
    # ---- F32S, list mode: every regime ---------------------------------------------------------------------------
    _c("f32s-list-nows-63", "F32S", "list", 33, 3, G3S2, 21, 131, ("rand", 63), False, "nows", count="63"),
    _c("f32s-list-one-stage-1", "F32S", "list", 1, 3, G3D2, 9, 70, ("rand", 1), True, "one_stage", count="1"),
    # 65 pixels x 2 channel tiles = 4 items, Ckk 72 -> 3 stages: one slice per stage
    _c("f32s-list-sk-stages-65", "F32S", "list", 70, 8, G3P0, 9, 21, ("rand", 65), True, "sk_stages", count="65"),
    _c("f32s-list-sk-cap8-64", "F32S", "list", 64, 16, G4S4, 32, 36, ("rand", 64), True, "sk_cap8", count="64"),
    # Ckk 1568 -> 49 stages over 8 slices: 6, 6, 6, 6, 6, 6, 6, 7
    _c("f32s-list-sk-cap8-49st", "F32S", "list", 64, 32, G7D8, 26, 40, ("rand", 64), True, "sk_cap8", count="64"),
    # base 100 -> 5 slices of 7 stages (Ckk 216): 1, 1, 2, 1, 2
    _c("f32s-list-sk-grid-5of7", "F32S", "list", 64, 24, G3, 80, 80, ("all",), True, "sk_grid", count="all"),
    # base 200 -> 2 slices of 3 stages: 1, 2
    _c("f32s-list-sk-grid-2of3", "F32S", "list", 256, 8, G3S2, 120, 140, ("rand", 3200), True, "sk_grid"),
    _c("f32s-list-full-511", "F32S", "list", 64, 3, G3, 128, 256, ("rand", 511 * 64), True, "full"),
    _c("f32s-list-full-512", "F32S", "list", 64, 3, G3, 128, 256, ("all",), True, "full", count="all"),
    _c("f32s-list-multi", "F32S", "list", 256, 3, G3, 96, 96, ("all",), True, "multi_item", count="all"),
    # ---- F32S, mask mode: every regime, every mask class ---------------------------------------------------------
    # exactly 256 words: chunk 1, every scan thread owns a word
    _c("f32s-mask-nows-256w", "F32S", "mask", 33, 3, G3, 64, 256, ("rand", 63), False, "nows", "<=256", "63"),
    # 400 words, chunk 2: 65 pixels in three of the 200 chunks, empty ones before, between and behind
    _c("f32s-mask-one-stage-400w", "F32S", "mask", 33, 3, G3, 100, 193, ("chunks", (7, 8, 150), 65), True,
       "one_stage", "257..512", "sparse"),
    # 650 words, chunk 3, 217 scan threads (the last owns two words), a workgroup owns two words
    _c("f32s-mask-last-bit-650w", "F32S", "mask", 64, 3, G3, 130, 257, ("last",), True, "one_stage", ">512", "1"),
    _c("f32s-mask-sk-stages-650w", "F32S", "mask", 70, 4, G3, 130, 257, ("chunks", (0, 100, 216), 65), True,
       "sk_stages", ">512", "sparse"),
    _c("f32s-mask-sk-cap8-49st", "F32S", "mask", 64, 32, G7S2, 16, 18, ("rand", 64), True, "sk_cap8", "<=256", "64"),
    _c("f32s-mask-sk-grid-2of3", "F32S", "mask", 64, 8, G3, 100, 193, ("rand", 12800), True, "sk_grid", "257..512"),
    _c("f32s-mask-full-511-650w", "F32S", "mask", 64, 3, G3, 130, 257, ("rand", 511 * 64), True, "full", ">512"),
    _c("f32s-mask-full-512-650w", "F32S", "mask", 64, 3, G3, 130, 257, ("rand", 512 * 64), True, "full", ">512"),
    _c("f32s-mask-multi", "F32S", "mask", 256, 3, G3, 96, 96, ("all",), True, "multi_item", "<=256", "all"),
    # geometry at the limits through the contraction: padding 64 (most listed pixels have no tap inside the map),
    # stride 4 with dilation 8, a ring that is never listed
    _c("f32s-mask-p64", "F32S", "mask", 33, 2, ((3, 3), (1, 1), (64, 64), (1, 1)), 3, 5, ("all",), True,
       "full", "257..512", "all"),
    _c("f32s-list-s4d8", "F32S", "list", 70, 5, G3S4D8, 30, 261, ("rand", 65), False, "nows", count="65"),
    # ---- F32: the exact f32 MFMA ---------------------------------------------------------------------------------
    _c("f32-mask-nows-256w", "F32", "mask", 33, 3, G3, 64, 256, ("rand", 63), False, "nows", "<=256", "63"),
    _c("f32-list-sk-cap8-49st", "F32", "list", 64, 32, G7S2, 16, 18, ("rand", 64), True, "sk_cap8", count="64"),
    _c("f32-mask-sk-grid-2of3", "F32", "mask", 64, 8, G3, 100, 193, ("rand", 12800), True, "sk_grid", "257..512"),
    _c("f32-mask-multi-650w", "F32", "mask", 64, 3, G3, 130, 257, ("all",), True, "multi_item", ">512", "all"),
    _c("f32-list-sk-stages-65", "F32", "list", 70, 8, G3D2, 9, 21, ("rand", 65), True, "sk_stages", count="65"),
    _c("f32-list-one-stage-1", "F32", "list", 1, 3, G3P3, 9, 70, ("rand", 1), True, "one_stage", count="1"),
    # ---- F16 -----------------------------------------------------------------------------------------------------
    _c("f16-list-nows-65", "F16", "list", 33, 5, G3S2, 21, 131, ("rand", 65), False, "nows", count="65"),
    _c("f16-mask-sk-cap8-49st", "F16", "mask", 64, 32, G7S2, 16, 18, ("rand", 64), True, "sk_cap8", "<=256", "64"),
    _c("f16-list-sk-grid-2of3", "F16", "list", 256, 8, G3S2, 120, 140, ("rand", 3200), True, "sk_grid"),
    _c("f16-mask-multi-650w", "F16", "mask", 64, 3, G3, 130, 257, ("all",), True, "multi_item", ">512", "all"),
    _c("f16-mask-one-stage-400w", "F16", "mask", 70, 3, G3, 100, 193, ("chunks", (0, 99, 199), 63), True,
       "one_stage", "257..512", "sparse"),
    _c("f16-list-one-stage-1", "F16", "list", 1, 1, G1, 7, 9, ("rand", 1), True, "one_stage", count="1"),
]
CASE_BY_ID = {c.id: c for c in CASES}
assert len(CASE_BY_ID) == len(CASES)

# one case per F32S regime for the sparse-operand bound
SPARSE_IDS = ["f32s-list-nows-63", "f32s-mask-one-stage-400w", "f32s-list-sk-stages-65", "f32s-list-sk-cap8-49st",
              "f32s-list-sk-grid-5of7", "f32s-list-full-511", "f32s-mask-multi"]
# list mode: a device count below the host count; entries outside the map
DEVICE_COUNT_IDS = ["f32s-list-sk-stages-65", "f32s-list-sk-cap8-64", "f32s-list-nows-63", "f32-list-sk-cap8-49st",
                    "f16-list-nows-65"]
OUT_OF_MAP_IDS = ["f32s-list-sk-stages-65", "f32s-list-nows-63", "f32s-list-sk-grid-2of3", "f32-list-sk-stages-65",
                  "f16-list-nows-65"]

REF_MAC_CAP = 3e8      # multiply-adds of a case's float64 reference (the dense convolution of its whole output map)


def case_out_hw(c):
    (kH, kW), s, p, d = c.geom
    return out_size(c.Hi, kH, s[0], p[0], d[0]), out_size(c.Wi, kW, s[1], p[1], d[1])


def case_words(c):
    return mask_words(*case_out_hw(c)) if c.source == "mask" else 0


def case_pixels(c):
    """The case's listed output pixels: ascending, distinct, int32; the same on every call."""
    rng = np.random.default_rng(zlib.crc32(c.id.encode()))
    Ho, Wo = case_out_hw(c)
    HW = Ho * Wo
    kind = c.pixels[0]
    if kind == "all":
        return np.arange(HW, dtype=np.int32)
    if kind == "last":
        return np.array([HW - 1], dtype=np.int32)
    if kind == "rand":
        return np.sort(rng.choice(HW, c.pixels[1], replace=False)).astype(np.int32)
    assert kind == "chunks"
    wpr = (Wo + 63) // 64
    words = Ho * wpr
    chunk = (words + SCAN - 1) // SCAN
    pool = []
    for i in c.pixels[1]:
        for w in range(i * chunk, min(words, (i + 1) * chunk)):
            y, x0 = divmod(w, wpr)
            pool.extend(y * Wo + x for x in range(x0 * 64, min(Wo, x0 * 64 + 64)))
    return np.sort(rng.choice(np.array(pool), c.pixels[2], replace=False)).astype(np.int32)


def case_form(c, n=None):
    n = len(case_pixels(c)) if n is None else n
    (kH, kW) = c.geom[0]
    return geom_form(c.K, c.C, kH, kW, n, c.ws, case_words(c))


def cell_of(c, f):
    return (c.arith, c.source, regime_of(f, c.ws), mask_class_of(f["words"]))


def reference_macs(c):
    Ho, Wo = case_out_hw(c)
    return Ho * Wo * c.K * c.C * c.geom[0][0] * c.geom[0][1]


# -------------------------------------------------------------------------------------------------------------------
# detection cases
# -------------------------------------------------------------------------------------------------------------------
DET_C = (1, 2, 3, 4, 5, 7, 8, 9, 15, 31, 32, 33, 47, 48, 70)
DET_WI = (1, 63, 64, 65, 130)
DET_MODES = (0, 1, 2)      # updateInputState
# at the limits; run on Hi = 1 with every C of DET_C, every Wi of DET_WI and the three update modes
DET_LIMIT_GEOMS = {
    "7x7d8s1p24": G7D8,                                      # a 64-pixel segment reaches three output words
    "7x7d8p64": ((7, 7), (1, 1), (64, 64), (8, 8)),
    "1x1s4p0": ((1, 1), (4, 4), (0, 0), (1, 1)),            # (DET_WI holds every residue mod 4)
    "3x3s4p1": ((3, 3), (4, 4), (1, 1), (1, 1)),
    "1x1p64": ((1, 1), (1, 1), (64, 64), (1, 1)),
    "3x3p3": G3P3,                                           # unreachable output pixels
    "2x2s2p2": ((2, 2), (2, 2), (2, 2), (1, 1)),            # unreachable output pixels
    "aniso7x1": ((7, 1), (1, 4), (64, 0), (8, 1)),
}
# the geometries of tests/test_gpu_geom.py, one size each: (geom, C, Hi, Wi)
DET_PLAIN = {
    "7x7s2p3": (G7S2, 3, 9, 131),
    "3x3s2p1": (G3S2, 5, 8, 130),
    "1x1s2p0": (((1, 1), (2, 2), (0, 0), (1, 1)), 16, 5, 129),
    "3x3d2p2": (G3D2, 32, 6, 65),
    "3x3d4p4": (((3, 3), (1, 1), (4, 4), (4, 4)), 3, 11, 64),
    "3x3s1p0": (G3P0, 5, 5, 67),
    "3x3s2d2p2": (((3, 3), (2, 2), (2, 2), (2, 2)), 16, 9, 127),
    "4x4s2p1": (((4, 4), (2, 2), (1, 1), (1, 1)), 32, 6, 130),
    "2x2s2p0": (((2, 2), (2, 2), (0, 0), (1, 1)), 3, 6, 129),
    "4x4s4p0": (G4S4, 5, 9, 257),
    "aniso": (((3, 5), (2, 1), (0, 3), (1, 2)), 64, 7, 63),
}


def detect_waves(C):
    """Waves of cbg_detect_kernel's workgroup (cbinfer_change_detection_geom)."""
    return 16 if C >= 32 else 8 if C >= 8 else 4 if C >= 4 else C


def detection_runs(name):
    """(C, Hi, Wi, mode) of one geometry's detection launches: every C x every mode, Wi cycling so that every Wi meets
    every mode."""
    if name in DET_PLAIN:
        _, C, Hi, Wi = DET_PLAIN[name]
        return [(C, Hi, Wi, m) for m in DET_MODES]
    return [(C, 1, DET_WI[(i + m) % len(DET_WI)], m) for i, C in enumerate(DET_C) for m in DET_MODES]
