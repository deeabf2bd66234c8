"""Case table of the grouped contraction (cb_groupconv.hip) and a classifier of the form a shape lands in.

`group_form` restates the DEVICE formulas of cbgr_conv_kernel and the padding of cbinfer_groupconv_*: ROWS, KgP, row
tiles per group, CkkgP, stages, tilesN, items, items against the grid of 512 workgroups, and the words per thread of the
mask scan.  CBGR_GRID is a constant, so nothing here depends on the card.  It is a classifier only: it says which row
padding, item schedule and stage count a case exercises, so that the table can be checked for coverage without a GPU
(tests/test_host_groupconv.py) and so that a change of the heuristics that moves a case into another form makes
tests/test_gpu_groupconv.py fail loudly.  No expected output is ever derived from it.

No GPU and no torch in this module.
"""
import zlib
from collections import namedtuple

import numpy as np
from optest import mask_words      # noqa: F401  (handed on to the tests)

CB_F32, CB_F16, CB_F32S = 0, 1, 2
ARITH = {"F32": CB_F32, "F16": CB_F16, "F32S": CB_F32S}

GRID = 512           # CBGR_GRID
BN = 64              # CBGR_BN
BK = 32              # CBGR_BK
SCAN = 256           # threads of the mask scan: chunk = ceil(words / 256) words per thread

ROWS_CLASSES = ("16", "32", "64", ">64")
SCHEDULES = ("one_item_or_none", "multi_item")
STAGE_CLASSES = ("1", ">1")
SOURCES = ("mask", "list")


def out_size(n, k, s, p, d):
    return (n + 2 * p - d * (k - 1) - 1) // s + 1


def rows_of(Kg):
    return 16 if Kg <= 16 else 32 if Kg <= 32 else 64


def prepared_bytes(G, Cg, Kg, kH, kW, elem):
    f = group_form(G, Cg, Kg, kH, kW, 0, 0)
    return G * f["KgP"] * f["CkkgP"] * elem + 8 * f["CkkgP"]


def group_form(G, Cg, Kg, kH, kW, N, words):
    """N: the change count the kernel sees; words: mask words of the output map (0 in list mode)."""
    ROWS = rows_of(Kg)
    KgP = (Kg + ROWS - 1) // ROWS * ROWS
    rowTiles = KgP // ROWS
    Ckkg = Cg * kH * kW
    CkkgP = (Ckkg + BK - 1) // BK * BK
    stages = CkkgP // BK
    tilesN = (N + BN - 1) // BN
    items = tilesN * G * rowTiles
    chunk = (words + SCAN - 1) // SCAN
    return dict(ROWS=ROWS, KgP=KgP, rowTiles=rowTiles, Ckkg=Ckkg, CkkgP=CkkgP, stages=stages, tilesN=tilesN, items=items,
                chunk=chunk, words=words, useful=(Kg / float(KgP)) * (Ckkg / float(CkkgP)))


def rows_class_of(f):
    return ">64" if f["rowTiles"] > 1 else str(f["ROWS"])


def schedule_of(f):
    """'multi_item': more items than workgroups, some workgroup walks several; else one item or none per workgroup."""
    return "multi_item" if f["items"] > GRID else "one_item_or_none"


def stage_class_of(f):
    return "1" if f["stages"] == 1 else ">1"


# -------------------------------------------------------------------------------------------------------------------
# shapes: the smallest at which each mechanism can go wrong
# -------------------------------------------------------------------------------------------------------------------
# geom: ((kH, kW), (sH, sW), (pH, pW), (dH, dW)); Hi x Wi: the INPUT map.
# pixels (on the OUTPUT map): ('rand', N) N distinct pixels; ('all',); ('last',) the one pixel on the last valid bit of
# the last mask word; ('reachable',) every pixel with a tap inside the input map; ('rand+last', N) N distinct pixels, the
# last pixel of the map among them.
Shape = namedtuple("Shape", "G Cg Kg geom Hi Wi pixels rows schedule stages")

G3 = ((3, 3), (1, 1), (1, 1), (1, 1))
G1 = ((1, 1), (1, 1), (0, 0), (1, 1))
G3S2 = ((3, 3), (2, 2), (1, 1), (1, 1))
G3D2 = ((3, 3), (1, 1), (2, 2), (2, 2))
G7D8 = ((7, 7), (1, 1), (24, 24), (8, 8))
G3P3 = ((3, 3), (1, 1), (3, 3), (1, 1))

SHAPES = {
    # 1088 pixels -> 17 tiles x 32 groups = 544 items > 512: a workgroup walks several items; 12 of 16 rows padded;
    # Ckkg 36: the second stage holds 4 real k of 32
    "resnext-narrow": Shape(32, 4, 4, G3, 34, 32, ("all",), "16", "multi_item", ">1"),
    # Wo 66: a 2-bit second word per row; padded rows of group 0 must not land in group 1's planes; Ckkg 27
    "odd-pad": Shape(2, 3, 5, G3S2, 21, 131, ("rand", 63), "16", "one_item_or_none", "1"),
    # the second tile holds one pixel; Ckkg 72 -> 3 stages; dilation taps over the border
    "rows32": Shape(3, 8, 24, G3D2, 9, 70, ("rand", 65), "32", "one_item_or_none", ">1"),
    # KgP 128: two row tiles, the second with 16 real rows; Ckkg 216 -> 7 stages
    "rows64-two-tiles": Shape(2, 24, 80, G3, 12, 20, ("rand", 64), ">64", "one_item_or_none", ">1"),
    # Ckkg 8; full 16 rows
    "shuffle-1x1": Shape(3, 8, 16, G1, 5, 130, ("last",), "16", "one_item_or_none", "1"),
    "depthwise-degenerate": Shape(6, 1, 2, G3, 7, 64, ("all",), "16", "one_item_or_none", "1"),
    # ROWS 64 with 31 padded rows; Ckkg 98 -> 4 stages; most taps outside the map
    "wide-reach": Shape(2, 2, 33, G7D8, 26, 40, ("rand", 64), "64", "one_item_or_none", ">1"),
    # the ring no tap reaches keeps act(bias); Ckkg 36
    "unreachable": Shape(2, 4, 4, G3P3, 6, 10, ("reachable",), "16", "one_item_or_none", ">1"),
    # 650 mask words: 3 words per scan thread, the last scan threads own none
    "mask-650w": Shape(2, 2, 2, G3, 130, 257, ("rand+last", 65), "16", "one_item_or_none", "1"),
}

Case = namedtuple("Case", "id shape arith source")


def _cases():
    plan = {
        "resnext-narrow": (("F32S", "mask"), ("F16", "list"), ("F32", "list")),
        "odd-pad": (("F32S", "list"), ("F16", "mask"), ("F32", "mask")),
        "rows32": (("F32S", "list"), ("F16", "mask"), ("F32", "list")),
        "rows64-two-tiles": (("F32S", "mask"), ("F16", "list"), ("F32", "list")),
        "shuffle-1x1": (("F32S", "mask"), ("F16", "mask")),
        "depthwise-degenerate": (("F32S", "mask"), ("F32", "list")),
        "wide-reach": (("F32S", "list"), ("F16", "mask"), ("F32", "mask")),
        "unreachable": (("F32S", "mask"), ("F16", "list")),
        "mask-650w": (("F32S", "mask"), ("F16", "mask")),
    }
    return [Case("%s-%s-%s" % (name, a.lower(), src), name, a, src) for name, runs in plan.items() for a, src in runs]


CASES = _cases()
CASE_BY_ID = {c.id: c for c in CASES}
assert len(CASE_BY_ID) == len(CASES)

# one case per ROWS for "a pixel does not depend on the list or the form"
INDEPENDENCE_IDS = ["odd-pad-f32s-list", "rows32-f16-mask", "wide-reach-f32-mask", "rows64-two-tiles-f32s-mask"]
# list mode: a device count below the host count; entries outside the map
DEVICE_COUNT_IDS = ["odd-pad-f32s-list", "rows32-f32-list", "rows64-two-tiles-f16-list"]
OUT_OF_MAP_IDS = ["odd-pad-f32s-list", "rows32-f32-list", "rows64-two-tiles-f16-list"]


def shape_out_hw(s):
    (kH, kW), st, p, d = s.geom
    return out_size(s.Hi, kH, st[0], p[0], d[0]), out_size(s.Wi, kW, st[1], p[1], d[1])


def _reached(n_in, n_out, k, s, p, d):
    o = np.arange(n_out)
    hit = np.zeros(n_out, dtype=bool)
    for j in range(k):
        i = o * s - p + j * d
        hit |= (i >= 0) & (i < n_in)
    return hit


def reachable_map(s):
    """bool [Ho, Wo]: the output pixels with a tap inside the input map."""
    (kH, kW), st, p, d = s.geom
    Ho, Wo = shape_out_hw(s)
    return np.outer(_reached(s.Hi, Ho, kH, st[0], p[0], d[0]), _reached(s.Wi, Wo, kW, st[1], p[1], d[1]))


def shape_pixels(name):
    """The shape's listed output pixels: ascending, distinct, int32; the same on every call."""
    s = SHAPES[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    Ho, Wo = shape_out_hw(s)
    HW = Ho * Wo
    kind = s.pixels[0]
    if kind == "all":
        return np.arange(HW, dtype=np.int32)
    if kind == "last":
        return np.array([HW - 1], dtype=np.int32)
    if kind == "reachable":
        return np.flatnonzero(reachable_map(s).reshape(-1)).astype(np.int32)
    if kind == "rand":
        return np.sort(rng.choice(HW, s.pixels[1], replace=False)).astype(np.int32)
    assert kind == "rand+last"
    return np.sort(np.concatenate([rng.choice(HW - 1, s.pixels[1] - 1, replace=False), [HW - 1]])).astype(np.int32)


def case_form(c, n=None):
    s = SHAPES[c.shape]
    n = len(shape_pixels(c.shape)) if n is None else n
    words = mask_words(*shape_out_hw(s)) if c.source == "mask" else 0
    return group_form(s.G, s.Cg, s.Kg, s.geom[0][0], s.geom[0][1], n, words)


def cell_of(c, f):
    """The five coordinates of a case."""
    return (c.arith, rows_class_of(f), c.source, schedule_of(f), stage_class_of(f))


def claimed_cell(c):
    s = SHAPES[c.shape]
    return (c.arith, s.rows, c.source, s.schedule, s.stages)
