"""Case table of the transposed-convolution contraction and detection (cb_tconv.hip) and a classifier of what a shape
exercises.

`tconv_form` restates the DEVICE formulas of cbt_conv_kernel and cbt_layout: per phase ph = ry sW + rx the taps, Ckk_ph =
C taps(ph), CkkP_ph (padded to 32), stages = CkkP_ph / 32, tiles = ceil(n_ph / 64) tilesM; base = sum of the tiles; the
k-split SKmax = min(512 / base, 8) with a workspace and base < 512, per phase SK_ph = max(1, min(SKmax, stages_ph));
items = sum tiles_ph SK_ph.  CBT_GRID is a constant 512, so nothing here depends on the card.  It is a classifier only:
`tags_of` says which features a case exercises, so that the table can be checked for coverage without a GPU
(tests/test_host_tconv.py) and so that a change of the heuristics that moves a case makes tests/test_gpu_tconv.py fail
loudly.  No expected output is ever derived from it.

No GPU and no torch in this module.
"""
import zlib
from collections import namedtuple

import numpy as np
from optest import mask_words      # noqa: F401  (handed on to the tests)

CB_F32, CB_F16, CB_F32S = 0, 1, 2
ARITH = {"F32": CB_F32, "F16": CB_F16, "F32S": CB_F32S}

GRID = 512           # CBT_GRID
BM = BN = 64         # CBT_BM, CBT_BN
BK = 32              # CBT_BK
SKMAX = 8            # CBT_SKMAX
SCAN = 256           # threads of the scan: chunk = ceil(words / 256) mask words (or list entries) per thread

MAX_K, MAX_S, MAX_D = 8, 4, 4
REF_MAC_CAP = 3e8    # multiply-adds of a case's float64 reference (the project's cap, tests/geomconv_cases.py)

# geom: ((kH, kW), (sH, sW), (pH, pW), (dH, dW), (opH, opW))
T2 = ((2, 2), (2, 2), (0, 0), (1, 1), (0, 0))              # U-Net
T4 = ((4, 4), (2, 2), (1, 1), (1, 1), (0, 0))              # segmentation / depth decoders, DCGAN
T3 = ((3, 3), (2, 2), (1, 1), (1, 1), (1, 1))              # torchvision-style decoders: 4, 2, 2, 1 taps per phase
T1S2 = ((1, 1), (2, 2), (0, 0), (1, 1), (1, 1))            # three phases of four without a tap
T3D2 = ((3, 3), (2, 2), (2, 2), (2, 2), (1, 1))            # phases without a tap through the dilation
T8S4 = ((8, 8), (4, 4), (2, 2), (1, 1), (0, 0))            # sixteen phases of four taps
T7S4D4 = ((7, 7), (4, 4), (6, 6), (4, 4), (3, 3))          # the widest reach; one phase of sixteen owns all 49 taps
T2S3 = ((2, 2), (3, 3), (0, 0), (1, 1), (2, 2))            # k < s
TANISO = ((3, 5), (4, 1), (0, 3), (1, 2), (3, 0))          # anisotropic, one stride-1 axis
T3S1 = ((3, 3), (1, 1), (1, 1), (1, 1), (0, 0))            # a single phase
DET_GEOMS = {"2x2s2": T2, "4x4s2p1": T4, "3x3s2p1op1": T3, "1x1s2op1": T1S2, "3x3s2d2p2op1": T3D2, "8x8s4p2": T8S4,
             "7x7s4d4p6op3": T7S4D4, "2x2s3op2": T2S3, "aniso": TANISO, "3x3s1p1": T3S1}


def out_size(n, k, s, p, d, op):
    return (n - 1) * s - 2 * p + d * (k - 1) + op + 1


def geom_out_hw(geom, Hi, Wi):
    k, s, p, d, op = geom
    return out_size(Hi, k[0], s[0], p[0], d[0], op[0]), out_size(Wi, k[1], s[1], p[1], d[1], op[1])


def within_limits(geom):
    k, s, p, d, op = geom
    return all(1 <= k[i] <= MAX_K and 1 <= s[i] <= MAX_S and 1 <= d[i] <= MAX_D and 0 <= p[i] <= d[i] * (k[i] - 1) and
               0 <= op[i] < max(s[i], d[i]) for i in (0, 1))


def phase_taps(k, d, s, r):
    """The taps of one axis that belong to phase r (rule 4)."""
    return [i for i in range(k) if (r - i * d) % s == 0]


def phase_tap_counts(geom):
    """taps(ph) for ph = ry sW + rx."""
    k, s, p, d, op = geom
    return [len(phase_taps(k[0], d[0], s[0], ry)) * len(phase_taps(k[1], d[1], s[1], rx))
            for ry in range(s[0]) for rx in range(s[1])]


def phase_of(geom, Wo, pix):
    """Phase index of flat output pixels."""
    k, s, p, d, op = geom
    pix = np.asarray(pix, dtype=np.int64)
    return ((pix // Wo + p[0]) % s[0]) * s[1] + (pix % Wo + p[1]) % s[1]


def tconv_form(K, C, geom, counts, has_workspace, total):
    """counts: listed pixels per phase as the kernel counts them (0 for a phase without a tap); total: mask words of the
    output map in mask mode, list entries in list mode (what the 256 scan threads share)."""
    KP = (K + BM - 1) // BM * BM
    tilesM = KP // BM
    taps = phase_tap_counts(geom)
    assert len(counts) == len(taps)
    ckk = [C * t for t in taps]
    ckkP = [(v + BK - 1) // BK * BK for v in ckk]
    stages = [v // BK for v in ckkP]
    tiles = [((n + BN - 1) // BN) * tilesM if t else 0 for n, t in zip(counts, taps)]
    base = sum(tiles)
    SKmax = 1
    if has_workspace and 0 < base < GRID:
        SKmax = min(GRID // base, SKMAX)
    SK = [max(1, min(SKmax, st)) for st in stages]
    items = sum(t * k for t, k in zip(tiles, SK))
    chunk = (total + SCAN - 1) // SCAN
    return dict(KP=KP, tilesM=tilesM, taps=taps, Ckk=ckk, CkkP=ckkP, stages=stages, tiles=tiles, base=base, SKmax=SKmax,
                SK=SK, items=items, chunk=chunk, counts=list(counts))


def prepared_bytes(K, C, geom, arith):
    """cbt_layout's total: per phase W_ph[KP][CkkP_ph] and 2 CkkP_ph table ints."""
    f = tconv_form(K, C, geom, [0] * len(phase_tap_counts(geom)), False, 0)
    es = 2 if arith == "F16" else 4
    return sum(f["KP"] * v * es + 8 * v for v in f["CkkP"])


TAGS = ("ph1", "ph63", "ph64", "ph65", "b64_then_1", "only_last", "all", "last_bit", "words<=256", "words257..512",
        "words>512", "nows", "one_stage", "sk_phase_cap", "sk8", "multi_item", "tapless", "phases16", "s3")
# what every arithmetic must reach (the issue's list); the rest are extras of the table
REQUIRED = ("ph1", "ph63", "ph64", "ph65", "b64_then_1", "only_last", "all", "last_bit", "words<=256", "words257..512",
            "words>512", "nows", "one_stage", "sk_phase_cap", "sk8", "multi_item")


def tags_of(c, f, px, Ho, Wo):
    """The features case c exercises, from its form f and its listed pixels px."""
    tags = set()
    n, taps, st, SK = f["counts"], f["taps"], f["stages"], f["SK"]
    live = [ph for ph in range(len(n)) if n[ph]]
    for v in (1, 63, 64, 65):
        if v in n:
            tags.add("ph%d" % v)
    # the tile boundary at a phase boundary: a full tile, then the next listed phase holds one pixel
    if any(n[a] == 64 and n[b] == 1 for a, b in zip(live, live[1:])):
        tags.add("b64_then_1")
    last_with_taps = max(ph for ph in range(len(taps)) if taps[ph])
    if live == [last_with_taps] and len([t for t in taps if t]) > 1:
        tags.add("only_last")
    if len(px) == Ho * Wo:
        tags.add("all")
    if len(px) == 1 and px[0] == Ho * Wo - 1 and c.source == "mask":
        tags.add("last_bit")
    if c.source == "mask":
        w = mask_words(Ho, Wo)
        tags.add("words<=256" if w <= 256 else "words257..512" if w <= 512 else "words>512")
    if not c.ws:
        tags.add("nows")
        assert f["SKmax"] == 1
    if any(st[ph] == 1 for ph in live):
        tags.add("one_stage")
    # the k-split of one listed phase is capped by its stage count while another listed phase has more slices
    if any(SK[a] == st[a] < f["SKmax"] and SK[b] > SK[a] for a in live for b in live):
        tags.add("sk_phase_cap")
    if any(SK[ph] == SKMAX for ph in live):
        tags.add("sk8")
    if f["base"] > GRID and len(live) > 1:      # a workgroup walks items of several phases
        assert f["items"] == f["base"]
        first = lambda item: next(ph for ph in range(len(n)) if item < sum(f["tiles"][:ph + 1]))
        if any(first(i) != first(i + GRID) for i in range(f["items"] - GRID)):
            tags.add("multi_item")
    if any(t == 0 for t in taps):
        tags.add("tapless")
    if len(taps) == 16 and all(taps):
        tags.add("phases16")
    if c.geom[1][1] == 3 and Wo > 64:
        tags.add("s3")
    return tags


# -------------------------------------------------------------------------------------------------------------------
# contraction cases, the same shapes for every arithmetic
# -------------------------------------------------------------------------------------------------------------------
# pixels (on the OUTPUT map): a tuple of per-phase counts (distinct random pixels of that phase); ('all',); ('last',) the
# one pixel on the last valid bit of the last mask word.
Case = namedtuple("Case", "id arith source K C geom Hi Wi pixels ws claims")

SHAPES = [
    # id, source, K, C, geom, Hi, Wi, pixels, workspace, claimed tags
    ("counts", "mask", 33, 8, T2, 5, 20, (64, 1, 63, 65), True,
     ("ph1", "ph63", "ph64", "ph65", "b64_then_1", "one_stage", "words<=256")),
    ("counts-list", "list", 1, 5, T4, 6, 22, (65, 64, 1, 63), True, ("ph1", "ph63", "ph64", "ph65", "b64_then_1")),
    ("only-last", "mask", 70, 13, T3, 9, 12, (0, 0, 0, 7), True, ("only_last", "one_stage")),
    ("only-last-list", "list", 64, 3, T2, 7, 9, (0, 0, 0, 5), False, ("only_last", "nows")),
    # Ckk per phase 256, 128, 128, 64: stages 8, 4, 4, 2 and as many slices each
    ("sk8", "mask", 70, 64, T3, 9, 12, (65, 10, 1, 3), True, ("sk8", "sk_phase_cap", "ph1", "ph65")),
    # Ckk per phase 96, 48, 48, 24: stages 3, 2, 2, 1 under SKmax 8
    ("sk-stages-list", "list", 64, 24, T3, 9, 12, (10, 10, 10, 10), True, ("sk_phase_cap", "one_stage")),
    # 4 x 36 pixel tiles x 4 channel tiles = 576 items: workgroup b walks item b of phase 0 and item b + 512 of phase 3
    ("all-multi", "mask", 256, 5, T2, 48, 48, ("all",), True, ("all", "multi_item", "words<=256")),
    ("all-d2-list", "list", 33, 3, T3D2, 7, 40, ("all",), False, ("all", "tapless", "nows")),
    ("last-bit-650w", "mask", 64, 3, T2, 65, 129, ("last",), True, ("last_bit", "words>512", "ph1")),
    ("sparse-400w", "mask", 33, 3, T4, 50, 100, (1, 65, 0, 64), True, ("words257..512", "ph1", "ph64", "ph65")),
    ("s4-16-phases", "mask", 33, 5, T8S4, 6, 20, (1, 0, 5, 2, 0, 7, 3, 1, 64, 0, 2, 2, 9, 1, 0, 4), True,
     ("phases16", "one_stage")),
    ("s3-all", "mask", 33, 7, T2S3, 5, 45, ("all",), True, ("all", "tapless", "s3")),
    ("aniso-all-list", "list", 70, 6, TANISO, 4, 70, ("all",), True, ("all", "tapless")),
    ("widest-all", "mask", 33, 3, T7S4D4, 5, 20, ("all",), True, ("all", "tapless")),
    ("single-phase-list", "list", 33, 5, T3S1, 9, 70, (65,), True, ("ph65",)),
    ("1x1s2-all", "mask", 33, 9, T1S2, 6, 40, ("all",), False, ("all", "tapless", "nows", "one_stage")),
]
CASES = [Case("%s-%s" % (a.lower(), s[0]), a, *s[1:]) for a in ("F32S", "F32", "F16") for s in SHAPES]
CASE_BY_ID = {c.id: c for c in CASES}
assert len(CASE_BY_ID) == len(CASES)

# list mode at the C ABI: a device count below the host count; entries outside the map
DEVICE_COUNT_IDS = ["f32s-counts-list", "f32s-sk-stages-list", "f32-only-last-list", "f16-counts-list"]
OUT_OF_MAP_IDS = ["f32s-counts-list", "f32s-single-phase-list", "f32-sk-stages-list", "f16-only-last-list"]


def case_out_hw(c):
    return geom_out_hw(c.geom, c.Hi, c.Wi)


def case_pixels(c):
    """The case's listed output pixels: ascending, distinct, int32; the same on every call."""
    rng = np.random.default_rng(zlib.crc32(c.id.split("-", 1)[1].encode()))      # (the same for every arithmetic)
    Ho, Wo = case_out_hw(c)
    HW = Ho * Wo
    if c.pixels == ("all",):
        return np.arange(HW, dtype=np.int32)
    if c.pixels == ("last",):
        return np.array([HW - 1], dtype=np.int32)
    ph = phase_of(c.geom, Wo, np.arange(HW))
    taps = phase_tap_counts(c.geom)
    assert len(c.pixels) == len(taps)
    chosen = []
    for i, n in enumerate(c.pixels):
        pool = np.flatnonzero(ph == i)
        assert n == 0 or taps[i], "a phase without a tap lists nothing the kernel counts"
        chosen.append(rng.choice(pool, n, replace=False))
    return np.sort(np.concatenate(chosen)).astype(np.int32)


def counted(c, px):
    """Per phase, the listed pixels the kernel counts: those of a phase with a tap."""
    Ho, Wo = case_out_hw(c)
    taps = phase_tap_counts(c.geom)
    ph = phase_of(c.geom, Wo, px)
    return [int((ph == i).sum()) if taps[i] else 0 for i in range(len(taps))]


def case_form(c, px=None):
    px = case_pixels(c) if px is None else px
    Ho, Wo = case_out_hw(c)
    return tconv_form(c.K, c.C, c.geom, counted(c, px), c.ws, mask_words(Ho, Wo) if c.source == "mask" else len(px))


def case_tags(c):
    px = case_pixels(c)
    Ho, Wo = case_out_hw(c)
    return tags_of(c, case_form(c, px), px, Ho, Wo)


def reference_macs(c):
    return c.C * c.Hi * c.Wi * c.K * c.geom[0][0] * c.geom[0][1]


# -------------------------------------------------------------------------------------------------------------------
# detection cases
# -------------------------------------------------------------------------------------------------------------------
DET_C = (1, 2, 3, 4, 5, 7, 8, 9, 15, 31, 32, 33, 47, 48, 70)      # (tests/geomconv_cases.py)
DET_WI = (1, 63, 64, 65, 130)
DET_HI = (1, 2, 5, 11)
DET_MODES = (0, 1, 2)      # updateInputState


def detection_runs(name):
    """(C, Hi, Wi, mode) of one geometry's detection launches: every C x every mode, Wi and Hi cycling so that every Wi
    meets every mode."""
    return [(C, DET_HI[(i + 2 * m) % len(DET_HI)], DET_WI[(i + m) % len(DET_WI)], m)
            for i, C in enumerate(DET_C) for m in DET_MODES]
