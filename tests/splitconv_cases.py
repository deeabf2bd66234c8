"""Case table of the split-state contraction (cb_split.hip) and a classifier of the launch form a shape lands in.

`split_form` restates the HOST selection of cbs_split_conv (arithmetic, tile height, mask words of the launch -> one of
the ten plain instantiations of cbs_conv_kernel) and the DEVICE's
k-split decision at the top of cbs_conv_kernel.  It is a classifier only: it says which instantiation, split and item
schedule a case exercises, so that the table below can be checked for coverage on a machine without a GPU
(tests/test_host_splitconv.py) and so that a change of the heuristics that moves a case into another cell makes
tests/test_gpu_splitconv.py fail loudly.  No expected output is ever derived from it.

No GPU and no torch in this module.
"""
import zlib
from collections import namedtuple

import numpy as np
from optest import mask_words      # noqa: F401  (handed on to the tests)

ASSUMED_CUS = 256        # the CU count the claimed cells of CASES are written for (MI355X)
MAXSEQ = 8               # CBS_MAXSEQ
PRE_BIG, PRE_X3, PRE_SMALL, PRE_MID2, PRE_MID = 1536, 1024, 1280, 2600, 5120      # cb_split_common.h
CHUNKS = 4               # CBS_CHUNKS
SPLIT_ROUNDS = 2         # CbsParams.splitRounds
DEEP = 48                # stages from which a contraction is a sum of CHUNKS partial sums

Instance = namedtuple("Instance", "arith BM cap mask_lds ring per_cu")


def name_of(i):
    return "%s/%d/pre%d/%s/ring%d/%dwg" % (i.arith, i.BM, i.cap, "lds" if i.mask_lds else "mem", i.ring, i.per_cu)


# the ten plain instantiations cbs_split_conv launches, in its order
X3_128_LDS = Instance("x3", 128, PRE_X3, True, 3, 1)
X3_128_MEM = Instance("x3", 128, PRE_BIG, False, 3, 1)
X3_64_ONE = Instance("x3", 64, PRE_SMALL, True, 5, 1)
X3_64_TWO = Instance("x3", 64, PRE_SMALL, False, 3, 2)
X3_64_MID = Instance("x3", 64, PRE_MID, False, 5, 1)
F16_128 = Instance("f16x2", 128, PRE_BIG, True, 4, 1)
F16_64_ONE = Instance("f16x2", 64, PRE_SMALL, True, 8, 1)
F16_64_TWO = Instance("f16x2", 64, PRE_SMALL, True, 4, 2)
F16_64_MID2 = Instance("f16x2", 64, PRE_MID2, False, 4, 2)
F16_64_MID = Instance("f16x2", 64, PRE_MID, False, 3, 2)
INSTANCES = [X3_128_LDS, X3_128_MEM, X3_64_ONE, X3_64_TWO, X3_64_MID,
             F16_128, F16_64_ONE, F16_64_TWO, F16_64_MID2, F16_64_MID]
INSTANCE_BY_NAME = {name_of(i): i for i in INSTANCES}
REGIMES = ["shallow", "deep_whole", "deep_split", "deep_split_tail", "deep_whole_tail", "fg_shallow", "fg_deep"]


def geom(C, kH, kW):
    """pair, kWs, nStages of cbs_geom."""
    G = C // 16
    pair = G == 1
    kWs = (kW + 1) // 2 if pair else kW
    return dict(pair=pair, kWs=kWs, nStages=kH * kWs if pair else kH * kW * (G // 2))


def supported(C, K, kH, kW):
    return (C in (16, 32, 64) and 1 <= K <= 1024 and kH % 2 == 1 and kW % 2 == 1 and 1 <= kH <= 15 and 1 <= kW <= 15
            and geom(C, kH, kW)["nStages"] >= 4)


def tile_height(K):
    return 64 if K <= 64 else 128


def max_mask_words(K):
    return PRE_BIG if tile_height(K) >= 128 else PRE_MID


def slab_capacity(nSeq, H, W, K, cus):
    bm = tile_height(K)
    kp = (K + bm - 1) // bm * bm
    return max(nSeq * ((H * W + bm - 1) // bm) * (kp // bm), 2 * cus)


def workspace_bytes(nSeq, C, H, W, K, kH, kW, cus):
    if not supported(C, K, kH, kW) or geom(C, kH, kW)["nStages"] < DEEP:
        return 0
    bm = tile_height(K)
    return 256 + slab_capacity(nSeq, H, W, K, cus) * bm * bm * 4


def instance_of(arith, BM, nSeq, MW):
    E = nSeq * MW
    if arith == "x3":
        if BM == 128:
            return X3_128_LDS if E <= PRE_X3 else X3_128_MEM
        if nSeq == 1 and MW <= PRE_SMALL:
            return X3_64_ONE
        return X3_64_TWO if E <= PRE_SMALL else X3_64_MID
    assert arith == "f16x2"
    if BM == 128:
        return F16_128
    if nSeq == 1 and MW <= PRE_SMALL:
        return F16_64_ONE
    if E <= PRE_SMALL:
        return F16_64_TWO
    return F16_64_MID2 if E <= PRE_MID2 else F16_64_MID


def split_form(arith, C, K, kH, kW, H, W, nSeq, N_per_seq, cus, force=0, tail=False, accumulate=False):
    """The launch form of cbinfer_split_conv (tail: cbinfer_split_conv_tail, accumulate: the fine-grained frame) for
    nSeq sequences with N_per_seq listed pixels each, on a card with `cus` CUs, no sequence on the exact path."""
    assert supported(C, K, kH, kW) and 1 <= nSeq <= MAXSEQ and len(N_per_seq) == nSeq
    g = geom(C, kH, kW)
    BM = BN = tile_height(K)
    KP = (K + BM - 1) // BM * BM
    MT, MW = KP // BM, mask_words(H, W)
    assert nSeq * MW <= max_mask_words(K) and H * W * W < (1 << 32)
    inst = instance_of(arith, BM, nSeq, MW)
    assert nSeq * MW <= inst.cap
    deep = g["nStages"] >= DEEP
    assert deep or not tail
    grid = inst.per_cu * cus
    tiles = [(n + BN - 1) // BN for n in N_per_seq]
    TP = sum(tiles)
    CH = CHUNKS if deep else 1
    cap = slab_capacity(nSeq, H, W, K, cus)
    SK = 1
    if TP > 0 and CH > 1 and TP * MT * CH <= SPLIT_ROUNDS * grid and TP * MT * CH <= cap:
        SK = CH
    if force > 0 and CH > 1:
        SK = CH if (force >= CH and TP * MT * CH <= cap) else 1
    items = TP * MT * SK
    if not deep:
        regime = "fg_shallow" if accumulate else "shallow"
    elif accumulate:
        regime = "fg_deep"
    else:
        regime = ("deep_split" if SK > 1 else "deep_whole") + ("_tail" if tail else "")
    return dict(pair=g["pair"], kWs=g["kWs"], nStages=g["nStages"], deep=deep, BM=BM, BN=BN, KP=KP, MT=MT, MW=MW,
                instance=inst, grid=grid, TP=TP, tiles=tiles, SK=SK, items=items, multi_item=items > grid,
                slab_cap=cap, regime=regime)


def cell_of(f):
    return (f["instance"].arith, name_of(f["instance"]), f["regime"], "multi_item" if f["multi_item"] else "single")


# -------------------------------------------------------------------------------------------------------------------
# cells without a case
# -------------------------------------------------------------------------------------------------------------------
REFERENCE_BUDGET = 1.0e9      # multiply-adds of a case's float64 reference


def uncovered(cell):
    """Why a cell of INSTANCES x REGIMES x (single, multi_item) has no row in CASES, or None if it must have one.

    No cell is unreachable for the kernel: a deep contraction is split whenever its 4 TP MT chunk items fit two rounds
    of the grid and the slabs, so an unsplit one has TP MT > grid / 2 tiles and may stay single (<= grid) or not, and a
    split one with more than grid items (at most 2 grid) is a multi_item launch too; the mask-word caps are a matter of
    the map's size, not of the regime.  What is listed here is left out for the cost of its reference, or because the
    regime's own code (the second launch, the accumulate epilogue) does not depend on how many items a workgroup walks."""
    _, name, regime, items = cell
    inst = INSTANCE_BY_NAME[name]
    if regime.endswith("_tail") and items == "multi_item":
        return "the tail launch walks tiles, not the first launch's items: pinned on single-item launches"
    if regime.startswith("fg_") and items == "multi_item":
        return "the accumulate epilogue is per item: pinned on single-item launches, the item walk on the plain regimes"
    if regime in ("deep_whole", "deep_whole_tail") and inst.BM == 128:
        # unsplit by the kernel's own rule: TP MT > 128, and a 128-row tile has at least 65 real channels
        return ("at least 129 tiles x 128 pixels x 1568 k x 65 channels = 1.7e9 multiply-adds (multi_item: twice that): "
                "beyond the reference budget; the forced runs of the deep_split cases reach the unsplit 128-row form")
    return None


def all_cells():
    return [(i.arith, name_of(i), r, m) for i in INSTANCES for r in REGIMES for m in ("single", "multi_item")]


# -------------------------------------------------------------------------------------------------------------------
# the cases
# -------------------------------------------------------------------------------------------------------------------
# change: the INPUT pixels of the case's own sequence that change by more than the threshold in frame 1, as a tuple of
# rectangles (y0, x0, h, w); the change list is their footprint dilated by the filter.  mode: 'conv' (cbinfer_split_conv),
# 'tail' (cbinfer_split_forward_tail), 'fg' (cbinfer_split_forward_fg: the rectangles bound the sparse delta).
# Sequences of an nSeq > 1 case: 0 the case's own change set, 1 static, 2 changes fully, 3.. the own set again.
# count: the class of the own sequence's list length: '1' = one footprint, 'BN-1', 'BN', 'BN+1', 'all' = every pixel,
# 'some' = a part of the map (the rows and blocks that set a tile count), 'sparse' = the footprint of a sparse delta.
Case = namedtuple("Case", "id arith C K kH kW H W nSeq change mode cell count")

TAIL_C1, TAIL_C2 = 64, 8
FG_TAPS = 1.5            # non-zero delta values per patch of a fine-grained case


def _c(id, inst, regime, items, C, K, filt, H, W, nSeq, change, count=None):
    mode = "fg" if regime.startswith("fg") else ("tail" if regime.endswith("tail") else "conv")
    if count is None:
        count = "sparse" if mode == "fg" else ("all" if change == "all" else "some")
    if change == "all":
        change = ((0, 0, H, W),)
    return Case(id, inst.arith, C, K, filt[0], filt[1], H, W, nSeq, tuple(change), mode,
                (inst.arith, name_of(inst), regime, items), count)


def rows(y0, n, W):
    """n whole rows of the map from y0."""
    return ((y0, 0, n, W),)


def singles(H, W, kH, kW, interior, edges, corners):
    """Single changed pixels whose footprints do not touch: `interior` whole ones (kH kW listed pixels each), `edges`
    on the top row (clipped to (kH + 1) / 2 rows), `corners` of the map's four (clipped both ways)."""
    out = [((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1))[i] + (1, 1) for i in range(corners)]
    x = kW // 2 + kW
    for _ in range(edges):
        out.append((0, x, 1, 1))
        x += kW
    assert x - kW // 2 <= W - kW
    y, x = kH // 2 + kH, kW // 2 + kW
    for _ in range(interior):
        if x + kW // 2 + kW > W - 1:
            y, x = y + kH, kW // 2 + kW
        assert y + kH // 2 + kH <= H - 1
        out.append((y, x, 1, 1))
        x += kW
    return tuple(out)


def fg_support(c):
    """[C, H, W] bool: the non-zero delta values of a fine-grained case -- about FG_TAPS per patch inside the case's
    rectangles.  The same on every call."""
    rng = np.random.default_rng(zlib.crc32(c.id.encode()))
    inside = np.zeros((c.H, c.W), dtype=bool)
    for (y0, x0, h, w) in c.change:
        inside[y0:y0 + h, x0:x0 + w] = True
    s = rng.random((c.C, c.H, c.W)) < FG_TAPS / (c.C * c.kH * c.kW)
    return s & inside[None]


def changed_pixels(c):
    """[H, W] bool: the input pixels of the case's own sequence that change in frame 1."""
    if c.mode == "fg":
        return fg_support(c).any(axis=0)
    m = np.zeros((c.H, c.W), dtype=bool)
    for (y0, x0, h, w) in c.change:
        assert 0 <= y0 and 0 <= x0 and h >= 1 and w >= 1 and y0 + h <= c.H and x0 + w <= c.W, c.id
        m[y0:y0 + h, x0:x0 + w] = True
    return m


def dilate(m, kH, kW):
    """The pixels whose kH x kW window (centred, clipped at the map's edge) holds a set pixel."""
    H, W = m.shape
    ph, pw = kH // 2, kW // 2
    p = np.zeros((H + 2 * ph, W + 2 * pw), dtype=bool)
    for dy in range(kH):
        for dx in range(kW):
            p[dy:dy + H, dx:dx + W] |= m
    return p[ph:ph + H, pw:pw + W]


def own_count(c):
    return int(dilate(changed_pixels(c), c.kH, c.kW).sum())


def seq_kinds(c):
    """What each sequence of the case does in frame 1."""
    return (["own", "static", "full"] + ["own"] * MAXSEQ)[:c.nSeq]


def seq_counts(c):
    n = own_count(c)
    return [{"own": n, "static": 0, "full": c.H * c.W}[k] for k in seq_kinds(c)]


def case_form(c, cus, force=0):
    return split_form(c.arith, c.C, c.K, c.kH, c.kW, c.H, c.W, c.nSeq, seq_counts(c), cus, force,
                      tail=c.mode == "tail", accumulate=c.mode == "fg")


def reference_macs(c):
    """Multiply-adds of the float64 reference of the case's largest frame."""
    per = c.C * c.kH * c.kW * c.K
    if c.mode == "fg":
        return sum(seq_counts(c)) * per
    return c.nSeq * c.H * c.W * per      # frame 0: every pixel of every sequence


CASES = [
    _c("x3128lds-shallow-one", X3_128_LDS, "shallow", "single", 16, 65, (3, 3), 1, 8, 1, "all"),
    _c("x3128lds-shallow-multi", X3_128_LDS, "shallow", "multi_item", 16, 65, (3, 3), 300, 130, 1, rows(3, 257, 130)),
    _c("x3128lds-deepsplit-one", X3_128_LDS, "deep_split", "single", 32, 65, (7, 7), 1, 8, 1, "all"),
    _c("x3128lds-deepsplittail-one", X3_128_LDS, "deep_split_tail", "single", 32, 80, (7, 7), 1, 8, 1, "all"),
    _c("x3128mem-shallow-one", X3_128_MEM, "shallow", "single", 16, 65, (3, 3), 1025, 8, 1, rows(3, 1, 8)),
    _c("x3128mem-shallow-multi", X3_128_MEM, "shallow", "multi_item", 16, 65, (3, 3), 513, 65, 1, "all"),
    _c("x3128mem-deepsplit-one", X3_128_MEM, "deep_split", "single", 32, 65, (7, 7), 1025, 8, 1, rows(3, 1, 8)),
    _c("x364one-shallow-one", X3_64_ONE, "shallow", "single", 16, 1, (3, 3), 1, 8, 1, "all"),
    _c("x364one-shallow-multi", X3_64_ONE, "shallow", "multi_item", 16, 1, (3, 3), 300, 65, 1, rows(3, 257, 65)),
    _c("x364one-deepwhole-one", X3_64_ONE, "deep_whole", "single", 32, 1, (7, 7), 150, 65, 1, rows(3, 129, 65)),
    _c("x364one-deepwhole-multi", X3_64_ONE, "deep_whole", "multi_item", 32, 1, (7, 7), 300, 65, 1, rows(3, 257, 65)),
    _c("x364one-deepsplit-one", X3_64_ONE, "deep_split", "single", 32, 1, (7, 7), 1, 8, 1, "all"),
    _c("x364one-deepsplit-multi", X3_64_ONE, "deep_split", "multi_item", 32, 1, (7, 7), 520, 8, 1, "all"),
    _c("x364one-deepsplittail-one", X3_64_ONE, "deep_split_tail", "single", 32, 16, (7, 7), 1, 8, 1, "all"),
    _c("x364one-deepwholetail-one", X3_64_ONE, "deep_whole_tail", "single", 32, 16, (7, 7), 150, 65, 1, rows(3, 129, 65)),
    _c("x364two-shallow-one", X3_64_TWO, "shallow", "single", 16, 1, (3, 3), 1, 8, 2, "all"),
    _c("x364two-shallow-multi", X3_64_TWO, "shallow", "multi_item", 16, 1, (3, 3), 40, 130, 8, rows(3, 33, 130)),
    _c("x364two-deepwhole-one", X3_64_TWO, "deep_whole", "single", 32, 1, (7, 7), 150, 8, 8, "all"),
    _c("x364two-deepwhole-multi", X3_64_TWO, "deep_whole", "multi_item", 64, 1, (5, 5), 40, 130, 8, rows(3, 33, 130)),
    _c("x364two-deepsplit-one", X3_64_TWO, "deep_split", "single", 32, 1, (7, 7), 1, 8, 2, "all"),
    _c("x364two-deepsplit-multi", X3_64_TWO, "deep_split", "multi_item", 32, 1, (7, 7), 300, 65, 2, rows(3, 129, 65)),
    _c("x364mid-shallow-one", X3_64_MID, "shallow", "single", 16, 1, (3, 3), 1281, 8, 1, rows(3, 1, 8)),
    _c("x364mid-shallow-multi", X3_64_MID, "shallow", "multi_item", 16, 1, (3, 3), 300, 8, 8, "all"),
    _c("x364mid-deepwhole-one", X3_64_MID, "deep_whole", "single", 32, 1, (7, 7), 257, 8, 5, "all"),
    _c("x364mid-deepwhole-multi", X3_64_MID, "deep_whole", "multi_item", 32, 1, (7, 7), 300, 8, 8, "all"),
    _c("x364mid-deepsplit-one", X3_64_MID, "deep_split", "single", 32, 1, (7, 7), 1281, 8, 1, rows(3, 1, 8)),
    _c("x364mid-deepsplit-multi", X3_64_MID, "deep_split", "multi_item", 32, 1, (7, 7), 1281, 8, 1, rows(3, 520, 8)),
    _c("f16128-shallow-one", F16_128, "shallow", "single", 16, 65, (3, 3), 1, 8, 1, "all"),
    _c("f16128-shallow-multi", F16_128, "shallow", "multi_item", 16, 65, (3, 3), 520, 65, 1, "all"),
    _c("f16128-deepsplit-one", F16_128, "deep_split", "single", 32, 65, (7, 7), 1, 8, 1, "all"),
    _c("f16128-deepsplittail-one", F16_128, "deep_split_tail", "single", 32, 80, (7, 7), 1, 8, 1, "all"),
    _c("f1664one-shallow-one", F16_64_ONE, "shallow", "single", 16, 1, (3, 3), 1, 8, 1, "all"),
    _c("f1664one-shallow-multi", F16_64_ONE, "shallow", "multi_item", 16, 1, (3, 3), 300, 65, 1, rows(3, 257, 65)),
    _c("f1664one-deepwhole-one", F16_64_ONE, "deep_whole", "single", 32, 1, (7, 7), 150, 65, 1, rows(3, 129, 65)),
    _c("f1664one-deepwhole-multi", F16_64_ONE, "deep_whole", "multi_item", 32, 1, (7, 7), 300, 65, 1, rows(3, 257, 65)),
    _c("f1664one-deepsplit-one", F16_64_ONE, "deep_split", "single", 32, 1, (7, 7), 1, 8, 1, "all"),
    _c("f1664one-deepsplit-multi", F16_64_ONE, "deep_split", "multi_item", 32, 1, (7, 7), 520, 8, 1, "all"),
    _c("f1664one-deepsplittail-one", F16_64_ONE, "deep_split_tail", "single", 32, 16, (7, 7), 1, 8, 1, "all"),
    _c("f1664one-deepwholetail-one", F16_64_ONE, "deep_whole_tail", "single", 32, 16, (7, 7), 150, 65, 1, rows(3, 129, 65)),
    _c("f1664two-shallow-one", F16_64_TWO, "shallow", "single", 16, 1, (3, 3), 1, 8, 2, "all"),
    _c("f1664two-shallow-multi", F16_64_TWO, "shallow", "multi_item", 16, 1, (3, 3), 40, 130, 8, rows(3, 33, 130)),
    _c("f1664two-deepwhole-one", F16_64_TWO, "deep_whole", "single", 32, 1, (7, 7), 150, 8, 8, "all"),
    _c("f1664two-deepwhole-multi", F16_64_TWO, "deep_whole", "multi_item", 64, 1, (5, 5), 40, 130, 8, rows(3, 33, 130)),
    _c("f1664two-deepsplit-one", F16_64_TWO, "deep_split", "single", 32, 1, (7, 7), 1, 8, 2, "all"),
    _c("f1664two-deepsplit-multi", F16_64_TWO, "deep_split", "multi_item", 32, 1, (7, 7), 300, 65, 2, rows(3, 129, 65)),
    _c("f1664mid2-shallow-one", F16_64_MID2, "shallow", "single", 16, 1, (3, 3), 1281, 8, 1, rows(3, 1, 8)),
    _c("f1664mid2-shallow-multi", F16_64_MID2, "shallow", "multi_item", 16, 1, (3, 3), 129, 65, 5, "all"),
    _c("f1664mid2-deepwhole-one", F16_64_MID2, "deep_whole", "single", 32, 1, (7, 7), 257, 8, 5, "all"),
    _c("f1664mid2-deepwhole-multi", F16_64_MID2, "deep_whole", "multi_item", 32, 1, (7, 7), 81, 65, 8, rows(3, 65, 65)),
    _c("f1664mid2-deepsplit-one", F16_64_MID2, "deep_split", "single", 32, 1, (7, 7), 1281, 8, 1, rows(3, 1, 8)),
    _c("f1664mid2-deepsplit-multi", F16_64_MID2, "deep_split", "multi_item", 32, 1, (7, 7), 81, 65, 8, rows(3, 1, 65)),
    _c("f1664mid-shallow-one", F16_64_MID, "shallow", "single", 16, 1, (3, 3), 2601, 8, 1, rows(3, 1, 8)),
    _c("f1664mid-shallow-multi", F16_64_MID, "shallow", "multi_item", 16, 1, (3, 3), 1301, 65, 1, rows(3, 520, 65)),
    _c("f1664mid-deepsplit-one", F16_64_MID, "deep_split", "single", 32, 1, (7, 7), 2601, 8, 1, rows(3, 1, 8)),
    # (two workgroups per CU: more than 512 chunk items only where the slabs hold them -- a map of 525 tiles)
    _c("f1664mid-deepsplit-multi", F16_64_MID, "deep_split", "multi_item", 32, 1, (7, 7), 4200, 8, 1, rows(3, 1034, 8)),
    _c("f1664mid-deepwhole-one", F16_64_MID, "deep_whole", "single", 32, 1, (7, 7), 2601, 8, 1, "all"),
    # (more chunk items than workgroups on the 128-row tile: 65 tiles x 4 chunks on 256 workgroups, K = 65 real channels)
    _c("x3128lds-deepsplit-multi", X3_128_LDS, "deep_split", "multi_item", 32, 65, (7, 7), 129, 64, 1, "all"),
    _c("x3128mem-deepsplit-multi", X3_128_MEM, "deep_split", "multi_item", 32, 65, (7, 7), 1032, 8, 1, "all"),
    _c("f16128-deepsplit-multi", F16_128, "deep_split", "multi_item", 32, 65, (7, 7), 129, 64, 1, "all"),
    # (525 unsplit tiles on 512 workgroups: 2100 chunk items would be more than two rounds)
    _c("f1664mid-deepwhole-multi", F16_64_MID, "deep_whole", "multi_item", 32, 1, (7, 7), 4200, 8, 1, "all"),
    # ---- two row tiles on a deep contraction (MT = 2: slab and chunk indexing, the reduce launch) ----
    _c("x3128lds-deepsplit-mt2", X3_128_LDS, "deep_split", "single", 32, 130, (7, 7), 20, 33, 1, rows(3, 2, 33)),
    _c("f16128-deepsplit-mt2", F16_128, "deep_split", "single", 32, 130, (7, 7), 20, 33, 1, rows(3, 2, 33)),
    # ---- the base shapes of the window-order and side-refresh tests of test_gpu_split.py (16 channels, 7x7: the pair form
    # with kWs = 4 and a half-dummy tap), so that the pixel-order launch those are compared with bit for bit is pinned.
    # 160x240 runs with K = 16 instead of 64: 64 channels there are 1.9e9 multiply-adds, and K <= 64 is one 64-row tile
    # (KP = 64, MT = 1) on the same instance either way -- K = 64 is pinned on 45x67.
    _c("base-win-45x67-k64", X3_64_ONE, "shallow", "single", 16, 64, (7, 7), 45, 67, 1, ((5, 7, 8, 8), (30, 50, 8, 8))),
    _c("base-win-38x130-k32", X3_64_ONE, "shallow", "single", 16, 32, (7, 7), 38, 130, 1, ((0, 0, 8, 8), (20, 100, 8, 30))),
    _c("base-win-64x64-k16", X3_64_ONE, "shallow", "single", 16, 16, (7, 7), 64, 64, 1, ((28, 30, 8, 8),)),
    _c("base-side-160x240-k16", X3_64_ONE, "shallow", "single", 16, 16, (7, 7), 160, 240, 1,
       ((10, 20, 16, 16), (100, 200, 16, 40), (150, 0, 10, 16))),
    # ---- the tail launch behind every instance of the first launch ----
    _c("x3128mem-deepsplittail-one", X3_128_MEM, "deep_split_tail", "single", 32, 80, (7, 7), 1025, 1, 1, rows(3, 1, 1)),
    _c("x364two-deepsplittail-one", X3_64_TWO, "deep_split_tail", "single", 32, 16, (7, 7), 1, 8, 2, "all"),
    _c("x364two-deepwholetail-one", X3_64_TWO, "deep_whole_tail", "single", 32, 16, (7, 7), 150, 8, 8, "all"),
    _c("x364mid-deepsplittail-one", X3_64_MID, "deep_split_tail", "single", 32, 16, (7, 7), 1281, 8, 1, rows(3, 1, 8)),
    _c("x364mid-deepwholetail-one", X3_64_MID, "deep_whole_tail", "single", 32, 16, (7, 7), 257, 8, 5, "all"),
    _c("f1664two-deepsplittail-one", F16_64_TWO, "deep_split_tail", "single", 32, 16, (7, 7), 1, 8, 2, "all"),
    _c("f1664two-deepwholetail-one", F16_64_TWO, "deep_whole_tail", "single", 32, 16, (7, 7), 150, 8, 8, "all"),
    _c("f1664mid2-deepsplittail-one", F16_64_MID2, "deep_split_tail", "single", 32, 16, (7, 7), 1281, 8, 1, rows(3, 1, 8)),
    _c("f1664mid2-deepwholetail-one", F16_64_MID2, "deep_whole_tail", "single", 32, 16, (7, 7), 257, 8, 5, "all"),
    _c("f1664mid-deepsplittail-one", F16_64_MID, "deep_split_tail", "single", 32, 16, (7, 7), 2601, 8, 1, rows(3, 1, 8)),
    _c("f1664mid-deepwholetail-one", F16_64_MID, "deep_whole_tail", "single", 32, 16, (7, 7), 2601, 8, 1, "all"),
    # ---- fine-grained frames (sparse delta inside the rectangles) on every instance ----
    _c("x364one-fgshallow", X3_64_ONE, "fg_shallow", "single", 16, 40, (3, 3), 37, 65, 1, "all"),
    _c("f1664one-fgshallow", F16_64_ONE, "fg_shallow", "single", 32, 64, (1, 5), 37, 65, 1, "all"),
    _c("x364two-fgshallow", X3_64_TWO, "fg_shallow", "single", 16, 16, (3, 3), 40, 65, 3, "all"),
    _c("f1664two-fgshallow", F16_64_TWO, "fg_shallow", "single", 64, 40, (3, 5), 40, 65, 2, "all"),
    _c("f1664mid2-fgshallow", F16_64_MID2, "fg_shallow", "single", 32, 16, (15, 1), 1288, 8, 1, rows(3, 300, 8)),
    _c("x3128lds-fgshallow", X3_128_LDS, "fg_shallow", "single", 16, 130, (3, 3), 40, 65, 1, "all"),
    _c("f16128-fgshallow", F16_128, "fg_shallow", "single", 64, 65, (3, 5), 40, 65, 1, "all"),
    _c("x364one-fgdeep", X3_64_ONE, "fg_deep", "single", 32, 64, (7, 7), 30, 65, 1, "all"),
    _c("f1664one-fgdeep", F16_64_ONE, "fg_deep", "single", 64, 40, (5, 5), 30, 65, 1, "all"),
    _c("x364two-fgdeep", X3_64_TWO, "fg_deep", "single", 16, 16, (15, 15), 30, 65, 2, "all"),
    _c("f1664two-fgdeep", F16_64_TWO, "fg_deep", "single", 32, 64, (7, 7), 20, 65, 3, "all"),
    _c("f1664mid2-fgdeep", F16_64_MID2, "fg_deep", "single", 32, 16, (7, 7), 1288, 8, 1, rows(3, 300, 8)),
    _c("x3128lds-fgdeep", X3_128_LDS, "fg_deep", "single", 64, 65, (5, 5), 30, 65, 1, "all"),
    _c("f16128-fgdeep", F16_128, "fg_deep", "single", 16, 130, (15, 15), 30, 65, 1, "all"),
    _c("x3128mem-fgshallow", X3_128_MEM, "fg_shallow", "single", 16, 65, (3, 3), 1032, 8, 1, rows(3, 300, 8)),
    _c("x3128mem-fgdeep", X3_128_MEM, "fg_deep", "single", 32, 65, (7, 7), 1032, 8, 1, rows(3, 300, 8)),
    _c("x364mid-fgshallow", X3_64_MID, "fg_shallow", "single", 16, 16, (3, 3), 1288, 8, 1, rows(3, 300, 8)),
    _c("x364mid-fgdeep", X3_64_MID, "fg_deep", "single", 32, 16, (7, 7), 1288, 8, 1, rows(3, 300, 8)),
    _c("f1664mid-fgshallow", F16_64_MID, "fg_shallow", "single", 32, 16, (15, 1), 2608, 8, 1, rows(3, 300, 8)),
    _c("f1664mid-fgdeep", F16_64_MID, "fg_deep", "single", 32, 16, (7, 7), 2608, 8, 1, rows(3, 300, 8)),
    # ---- the edges: K, filters, map widths, H = 1, a map smaller than its filter, counts around the tile width ----
    _c("edge-x3-k16-w63-bnm1", X3_64_ONE, "shallow", "single", 16, 16, (3, 3), 37, 63, 1, singles(37, 63, 3, 3, 7, 0, 0), "BN-1"),
    _c("edge-f16-k40-w64-bn", F16_64_ONE, "shallow", "single", 16, 40, (3, 3), 37, 64, 1, singles(37, 64, 3, 3, 6, 1, 1), "BN"),
    _c("edge-x3-k64-1x5-w65-bnp1", X3_64_ONE, "shallow", "single", 32, 64, (1, 5), 20, 65, 1, singles(20, 65, 1, 5, 13, 0, 0), "BN+1"),
    _c("edge-f16-k1-1x5-one", F16_64_ONE, "shallow", "single", 32, 1, (1, 5), 20, 65, 1, singles(20, 65, 1, 5, 1, 0, 0), "1"),
    _c("edge-x3-k65-3x5-w130-bnm1", X3_128_LDS, "shallow", "single", 64, 65, (3, 5), 33, 130, 1, singles(33, 130, 3, 5, 7, 1, 2), "BN-1"),
    _c("edge-f16-k130-3x5-w130-bn", F16_128, "shallow", "single", 64, 130, (3, 5), 33, 130, 1, singles(33, 130, 3, 5, 6, 2, 3), "BN"),
    _c("edge-x3-k130-3x5-w130-bnp1", X3_128_LDS, "shallow", "single", 64, 130, (3, 5), 33, 130, 1, singles(33, 130, 3, 5, 7, 0, 4), "BN+1"),
    _c("edge-f16-k65-3x5-one", F16_128, "shallow", "single", 64, 65, (3, 5), 33, 130, 1, singles(33, 130, 3, 5, 1, 0, 0), "1"),
    _c("edge-x3-w1", X3_64_ONE, "shallow", "single", 16, 16, (3, 3), 70, 1, 1, "all", "all"),
    _c("edge-f16-h1-w130", F16_64_ONE, "shallow", "single", 32, 40, (1, 5), 1, 130, 1, "all", "all"),
    _c("edge-x3-map-below-filter", X3_64_ONE, "shallow", "single", 16, 64, (7, 7), 5, 4, 1, "all", "all"),
    _c("edge-f16-map-below-filter", F16_64_ONE, "shallow", "single", 16, 64, (7, 7), 5, 4, 1, "all", "all"),
    _c("edge-x3-k1024-multi", X3_128_LDS, "shallow", "multi_item", 16, 1024, (3, 3), 60, 70, 1, "all", "all"),
    _c("edge-f16-k1024-multi", F16_128, "shallow", "multi_item", 16, 1024, (3, 3), 60, 70, 1, "all", "all"),
    _c("edge-x3-15x15-pair-deep", X3_64_ONE, "deep_split", "single", 16, 16, (15, 15), 20, 33, 1, rows(3, 2, 33)),
    _c("edge-f16-15x15-pair-deep", F16_64_ONE, "deep_split", "single", 16, 40, (15, 15), 20, 33, 1, rows(3, 2, 33)),
    _c("edge-x3-15x1", X3_64_ONE, "shallow", "single", 32, 40, (15, 1), 40, 8, 1, rows(3, 1, 8)),
    _c("edge-x3-5x5-c64-just-deep", X3_128_LDS, "deep_split", "single", 64, 65, (5, 5), 33, 64, 1, rows(3, 2, 64)),
    _c("edge-f16-7x7-c32-k64", F16_64_TWO, "deep_split", "single", 32, 64, (7, 7), 21, 65, 3, rows(3, 2, 65)),
    _c("edge-x3-7x7-c32-5seq", X3_64_TWO, "deep_split", "single", 32, 64, (7, 7), 21, 65, 5, rows(3, 2, 65)),
]
CASE_BY_ID = {c.id: c for c in CASES}
assert len(CASE_BY_ID) == len(CASES)
