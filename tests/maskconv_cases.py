"""Case table of the three mask-driven contractions -- the row-segment kernel (cb_rowconv.hip), the patch-staged bf16x3
kernel (cb_blockconv.hip) and the row-pair kernel (cb_rowpair.hip) -- with classifiers of the launch form a shape lands
in and a generator of change masks that lays chosen popcounts over the mask words instead of random blobs.

`row_form`, `row_word_form`, `blk_form`, `blk_unit_form` and `pair_form` restate the HOST geometry (row_geom, blk_geom,
the launchers) and the DEVICE's per-word role assignment.  They are classifiers only: they say which form a case
exercises, so that the table can be checked for coverage without a GPU (tests/test_host_maskconv.py) and so that a change
of the heuristics that moves a case into another cell makes tests/test_gpu_maskconv.py fail loudly.  No expected output
is ever derived from them.

No GPU and no torch in this module.
"""
import zlib
from collections import namedtuple

import numpy as np
from optest import mask_words      # noqa: F401  (handed on to the tests)

ASSUMED_CUS = 256        # the CU count the claimed cells of CASES are written for (MI355X)
MAXSEQ = 8               # CBINFER_SPLIT_MAX_SEQUENCES
ROW_BS = 12              # CB_ROW_BS: k-steps of a weight block of the row-segment kernel
ROW_MAXROWS = 256        # CB_ROW_MAXROWS
PAIR_MAXCAND = 4         # CBP_MAXCAND
PAIR_MAXWORDS = 1 << 20  # CBP_MAXWORDS
REFERENCE_BUDGET = 1.0e9      # multiply-adds of a case's float64 reference


# -------------------------------------------------------------------------------------------------------------------
# classifiers
# -------------------------------------------------------------------------------------------------------------------
def row_plane_stride(kH, kW):
    cs = kH * (64 + kW - 1)
    while cs % 32 != 16:
        cs += 1
    return cs


def row_form(C, K, kH, kW):
    """row_geom + cbinfer_rowconv_supported + the launch of cb_rows_launch.  `supported`, `prepared` (= MCH G 1024) are
    checked against the library's host functions; the library exposes nothing for `halves`, `MCW`, the instance choice,
    the staging passes or the consumers per word: those fields are a restatement of the code that can drift."""
    f = dict(supported=False)
    if C <= 0 or K <= 0 or kH <= 0 or kW <= 0 or kW > 33 or kH > 33 or kH * kW == 1:
        return f
    CP = (C + 3) // 4 * 4
    CS = row_plane_stride(kH, kW)
    S = kH * kW * (CP // 4)
    G = (S + 3) // 4
    NB = S // ROW_BS
    MCH = (K + 15) // 16
    MCW = min(MCH, 2)
    lds = (CP * CS + 4 * MCW * 64 * 4) * 4
    f.update(CP=CP, CS=CS, S=S, G=G, NB=NB, rem=S - ROW_BS * NB, MCH=MCH, MCW=MCW, lds=lds, prepared=MCH * G * 1024)
    if lds > 60 * 1024 or CP * kH > ROW_MAXROWS or MCH * G * 1024 > 512 * 1024:
        return f
    f["supported"] = True
    f["instance"] = "7x7x1" if (kH, kW, CP) == (7, 7, 4) else ("7x7x4" if (kH, kW, CP) == (7, 7, 16) else "rt")
    f["groups"] = (MCH + MCW - 1) // MCW
    f["halves"] = 2 if MCW * S >= 256 else 1
    NW, NTH = 4 * MCW, 256 * MCW
    rows = CP * kH
    sh = 0
    while (1 << sh) < kW - 1:
        sh += 1
    edge = (rows << sh) if kW > 1 else 0             # edge slots: TW = 2^sh >= kW - 1 per patch row
    f.update(NW=NW, NTH=NTH, rows=rows, edge_slots_per_row=(1 << sh) if kW > 1 else 0,
             passes=max(1, -(-rows // (8 * NW)), -(-edge // (2 * NTH))))
    # consumers of a word: the workgroups whose arrival the last one counts
    f["consumers_small"] = f["groups"]                                   # nT <= 2
    f["consumers_big"] = f["groups"] * (2 if f["halves"] == 2 else 1)    # nT > 2
    f["inactive_chunk_wave"] = f["groups"] * MCW > MCH
    return f


def row_word_form(form, popcount):
    """Per pixel half nh of a word with `popcount` set bits: (nTr, nTw, kparts, the k-parts that own no full block)."""
    nT = (popcount + 15) >> 4
    out = {}
    for nh in range(form["halves"]):
        if popcount == 0 or 2 * nh >= nT:
            continue
        nTr = min(2 if form["halves"] == 2 else 4, nT - 2 * nh)
        nTw = 4 if nTr == 3 else nTr
        kparts = 4 // nTw
        empty = [kp for kp in range(kparts) if form["NB"] * kp // kparts == form["NB"] * (kp + 1) // kparts]
        out[nh] = (nTr, nTw, kparts, empty)
    return out


def row_cell(f, mode):
    nb = "NB0" if f["NB"] == 0 else ("NB1-3" if f["NB"] < 4 else "NB4+")
    return ("rows", f["instance"], "h%d" % f["halves"], nb, "rem0" if f["rem"] == 0 else "rem+", mode)


def blk_form(C, K, kH, kW):
    """blk_geom + cbinfer_blockconv_supported (R = 2 rows per unit, MG = 2 channel tiles per workgroup)."""
    f = dict(supported=False)
    if C <= 0 or K <= 0 or kH <= 1 or kW <= 1 or kH > 15 or kW > 16:
        return f
    CH, KXQ = (C + 7) // 8, (kW + 3) // 4
    SPC = kH * KXQ
    MT = (K + 15) // 16
    ZM = (MT + 1) // 2
    PR, PC = 2 + kH - 1, 64 + 4 * KXQ
    lds = max(2 * 3 * PR * PC * 16, 4 * 4 * 2 * 1024)
    f.update(CH=CH, KXQ=KXQ, SPC=SPC, MT=MT, ZM=ZM, PR=PR, PC=PC, lds=lds, prepared=ZM * 2 * CH * SPC * 3 * 64 * 16,
             own=(CH * ((SPC + 1) >> 1), CH * (SPC >> 1)))      # steps of the k-half waves 0 and 1
    if PR * PC > 768:
        return f
    magic = (65536 + PC - 1) // PC
    if any(((q * magic) >> 16) != q // PC for q in range(768)):
        return f
    f["supported"] = lds <= 64 * 1024
    f["starved_ring"] = min(f["own"]) < 4            # a wave owns fewer steps than its weight ring has sets
    f["inactive_tile"] = MT % 2 == 1
    return f


def blk_unit_form(popA, popB):
    nTt = ((popA + 15) >> 4) + ((popB + 15) >> 4)
    return dict(nTt=nTt, odd=nTt % 2 == 1, first_empty=popA == 0, second_empty=popB == 0)


def blk_cell(f, mode):
    return ("blocks", "kxq%d" % f["KXQ"], mode)


def pair_supported(C, K, kH, kW, H, W):
    if C < 1 or C > 4 or K < 1 or K > 16 or kH != kW or kH not in (3, 5, 7) or H < 1 or W < 1:
        return False
    return mask_words(H, W) <= PAIR_MAXWORDS and 16 * H * W * 4 < (1 << 30)


def pair_form(C, K, k, H, W, nSeq, cus, det=False):
    """cbp_launch: the instance, the units, the grid, the highest candidate slot some workgroup uses and whether some
    workgroup's last slot lies beyond the units.  (Nothing of this is exposed by the library: a restatement.)"""
    assert pair_supported(C, K, k, k, H, W) and 1 <= nSeq <= MAXSEQ
    wpr = (W + 63) // 64
    units = ((H + 1) // 2) * wpr
    total = units * nSeq
    if det:
        assert nSeq == 1 and k == 7
        grid = total
    else:
        grid = min(8 * cus, total)
        if grid * PAIR_MAXCAND < total:
            grid = (total + PAIR_MAXCAND - 1) // PAIR_MAXCAND
    top = (total + grid - 1) // grid - 1
    return dict(instance="%dx%d%s" % (k, k, "det" if det else ""), wpr=wpr, units=units, total=total, grid=grid,
                top_slot=top, beyond=grid * (top + 1) > total)


def pair_cell(f, fold):
    return ("pair", f["instance"], fold, "slot%d" % f["top_slot"])


# -------------------------------------------------------------------------------------------------------------------
# word patterns
# -------------------------------------------------------------------------------------------------------------------
POPCOUNTS = (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64)
# (popcount of the pair's first row, of its second row): a word alone, its partner alone, both full, an odd total tile
# count, both nearly empty.  A map's full-width slots take this list in order (from the map's `start`), the last odd row
# first: the 26 full-width slots of the 25 x 130 map hold the first 26 entries, its first 2-pixel slot the (1, 1).
PAIRS = ([(x, 0) for x in POPCOUNTS] + [(0, x) for x in POPCOUNTS] + [(64, 64), (17, 16), (1, 1)])

Map = namedtuple("Map", "H W start full")
MAPS = {
    "base": Map(25, 130, 0, False),      # two full words, a 2-pixel word, an odd last row; W % 4 = 2
    "w63": Map(26, 63, 7, False),        # one word a pixel short of full; W % 4 = 3
    "w65": Map(27, 65, 13, False),       # a 1-pixel second word; W % 4 = 1
    "tiny": Map(2, 3, 0, True),          # smaller than a 7x7 filter, every pixel listed
    "h1": Map(1, 130, 3, False),         # one row: every unit of the two-row kernels lacks its second row
}
Pattern = namedtuple("Pattern", "mask words slots")      # words: (y, tx) -> (popcount, bit 0 forced, top bit forced)


def _slots(H, W):
    """The (yo, tx) units of a map in the order they take their pair of popcounts: full-width words first (the last
    odd row in front), then the narrow ones."""
    wpr = (W + 63) // 64
    full = [tx for tx in range(wpr) if W - 64 * tx >= 64]
    narrow = [tx for tx in range(wpr) if W - 64 * tx < 64]
    rows = list(range((H + 1) // 2))
    if H % 2:
        rows = rows[-1:] + rows[:-1]
    return [(yo, tx) for yo in rows for tx in full] + [(yo, tx) for yo in range((H + 1) // 2) for tx in narrow]


def _word(rng, width, pc, force0, forcetop):
    pc = min(pc, width)
    bits = np.zeros(64, dtype=bool)
    if pc == 0:
        return bits, (0, False, False)
    chosen = []
    if force0:
        chosen.append(0)
    if forcetop and len(chosen) < pc and width - 1 not in chosen:
        chosen.append(width - 1)
    rest = [i for i in range(width) if i not in chosen]
    chosen += list(rng.choice(rest, pc - len(chosen), replace=False)) if pc > len(chosen) else []
    bits[chosen] = True
    return bits, (pc, bool(bits[0]) and force0, bool(bits[width - 1]) and forcetop)


def pattern(m):
    """The change mask of a Map: per slot j the popcounts PAIRS[(start + j) % len], capped by the word's width; bit 0
    forced in the words of the slots j % 3 == 0 and the word's last bit in those of j % 3 == 1 (taps cross the patch's
    left and right edge); the map's bottom-right pixel always listed.  The same on every call."""
    H, W = m.H, m.W
    wpr = (W + 63) // 64
    mask = np.zeros((H, wpr * 64), dtype=bool)
    words, slots = {}, []
    if m.full:
        mask[:, :W] = True
        for y in range(H):
            for tx in range(wpr):
                words[(y, tx)] = (min(64, W - 64 * tx), False, False)
        return Pattern(mask[:, :W].copy(), words, [])
    rng = np.random.default_rng(zlib.crc32(("map %d %d %d" % (H, W, m.start)).encode()))
    for j, (yo, tx) in enumerate(_slots(H, W)):
        width = min(64, W - 64 * tx)
        pa, pb = PAIRS[(m.start + j) % len(PAIRS)]
        spec = [pa, pb]
        for r in range(2):
            y = 2 * yo + r
            if y >= H:
                spec[r] = None
                continue
            last = y == H - 1 and tx == wpr - 1
            pc = max(spec[r], 1) if last else spec[r]
            bits, words[(y, tx)] = _word(rng, width, pc, j % 3 == 0 and not last, j % 3 == 1 or last)
            mask[y, 64 * tx:64 * tx + 64] = bits
            spec[r] = words[(y, tx)][0]
        slots.append((yo, tx, width, spec[0], spec[1]))
    return Pattern(mask[:, :W].copy(), words, slots)


def subset(mask, key):
    """About half of a mask's pixels (whole words dropped, whole words kept, words thinned out): the pixels a
    bit-identity test lists alone."""
    rng = np.random.default_rng(zlib.crc32(("subset " + key).encode()))
    keep = rng.random(mask.shape) < 0.5
    H, W = mask.shape
    for y in range(H):
        for x0 in range(0, W, 64):
            r = rng.random()
            if r < 0.2:
                keep[y, x0:x0 + 64] = True
            elif r < 0.4:
                keep[y, x0:x0 + 64] = False
    return mask & keep


def dilate(m, kH, kW):
    """The pixels whose kH x kW window (anchored at (kH-1)/2, (kW-1)/2, clipped at the map's edge) holds a set pixel."""
    H, W = m.shape
    ph, pw = (kH - 1) // 2, (kW - 1) // 2
    p = np.zeros((H + kH - 1, W + kW - 1), dtype=bool)
    p[ph:ph + H, pw:pw + W] = m
    out = np.zeros((H, W), dtype=bool)
    for dy in range(kH):
        for dx in range(kW):
            out |= p[dy:dy + H, dx:dx + W]
    return out


# -------------------------------------------------------------------------------------------------------------------
# the cases
# -------------------------------------------------------------------------------------------------------------------
# kernel: 'rows', 'blocks', 'pair'.  mode: rows 'plain' | 'batched' | 'acc' (opt relu_out); blocks 'plain' | 'acc' |
# 'sparse' (accumulate mode on a delta with SPARSE_TAPS non-zero values per patch); pair 'plain' | 'fold3' | 'fold2' (the
# next layer's records as bf16 triples / f16 pairs; opt ceil, k2), opt det (the layer's own detection in the launch),
# opt slots (a tall narrow map: H, W of the case instead of a Map; the non-empty units are placed by slot_units).
Case = namedtuple("Case", "id kernel C K kH kW map nSeq mode opt cell")
SPARSE_TAPS = 0.7        # expected non-zero delta values per patch of a sparse case (given one: 1.4)
DET_TH = 0.1
NEXT_TH = 0.07


def _opt(c):
    return dict(c.opt)


def case_map(c):
    o = _opt(c)
    return Map(o["H"], o["W"], 0, False) if "slots" in o else MAPS[c.map]


def case_cell(c, cus):
    m = case_map(c)
    if c.kernel == "rows":
        return row_cell(row_form(c.C, c.K, c.kH, c.kW), c.mode)
    if c.kernel == "blocks":
        return blk_cell(blk_form(c.C, c.K, c.kH, c.kW), c.mode)
    return pair_cell(pair_form(c.C, c.K, c.kH, m.H, m.W, c.nSeq, cus, "det" in _opt(c)), c.mode)


def _case(id, kernel, shape, map, mode="plain", nSeq=1, **opt):
    C, K, kH, kW = shape
    c = Case(id, kernel, C, K, kH, kW, map, nSeq, mode, tuple(sorted(opt.items())), None)
    return c._replace(cell=case_cell(c, ASSUMED_CUS))


ROW_SHAPES = [(3, 16, 7, 7), (16, 64, 7, 7), (16, 16, 7, 7), (4, 16, 3, 3), (2, 9, 5, 5), (8, 16, 2, 3), (4, 8, 3, 4),
              (9, 16, 2, 2), (24, 16, 7, 7), (12, 40, 7, 7), (5, 33, 4, 2), (1, 1, 1, 33), (3, 5, 9, 1), (6, 70, 3, 9),
              (20, 128, 5, 5), (64, 16, 3, 3),
              # beyond the issue's list, for the holes of the cell table and the consumer counts:
              (16, 32, 6, 6),       # halves 2 with rem 0
              (16, 70, 7, 7),       # 7x7x4 with 3 chunk groups and halves 2: 3 and 6 consumers per word
              (5, 12, 3, 7)]        # NB 3: one block per k-part but the last, and a remainder block
BLK_SHAPES = [(1, 1, 2, 2), (8, 16, 3, 3), (16, 64, 7, 7), (17, 40, 5, 5), (24, 33, 3, 9), (9, 70, 2, 13), (8, 32, 9, 4),
              (5, 17, 6, 6), (64, 256, 7, 7)]
BLK_SPARSE = [(8, 16, 3, 3), (16, 64, 7, 7), (17, 40, 5, 5), (24, 33, 3, 9), (9, 70, 2, 13)]
PAIR_SHAPES = [(3, 16, 7), (4, 16, 7), (1, 16, 7), (3, 15, 7), (2, 5, 5), (4, 16, 5), (1, 1, 3), (3, 16, 3)]


def _name(s):
    return "x".join(str(v) for v in s)


CASES = []
for s in ROW_SHAPES:
    CASES.append(_case("rows-%s-base" % _name(s), "rows", s, "base"))
for mp in ("w63", "w65", "tiny", "h1"):
    CASES.append(_case("rows-3x16x7x7-%s" % mp, "rows", (3, 16, 7, 7), mp))
    CASES.append(_case("rows-16x64x7x7-%s" % mp, "rows", (16, 64, 7, 7), mp))
CASES += [
    _case("rows-5x33x4x2-w65", "rows", (5, 33, 4, 2), "w65"),
    _case("rows-1x1x1x33-w63", "rows", (1, 1, 1, 33), "w63"),
    _case("rows-3x16x7x7-batched8", "rows", (3, 16, 7, 7), "w65", "batched", 8),
    _case("rows-16x64x7x7-batched2", "rows", (16, 64, 7, 7), "base", "batched", 2),
    _case("rows-6x70x3x9-batched2", "rows", (6, 70, 3, 9), "w63", "batched", 2),
    _case("rows-16x64x7x7-acc", "rows", (16, 64, 7, 7), "base", "acc", relu_out=False),
    _case("rows-3x16x7x7-acc-relu", "rows", (3, 16, 7, 7), "base", "acc", relu_out=True),
    _case("rows-4x16x3x3-acc-relu", "rows", (4, 16, 3, 3), "w65", "acc", relu_out=True),
    _case("rows-2x9x5x5-acc", "rows", (2, 9, 5, 5), "w63", "acc", relu_out=False),
]
for s in BLK_SHAPES:
    CASES.append(_case("blocks-%s-base" % _name(s), "blocks", s, "base"))
for mp in ("w63", "w65", "tiny", "h1"):
    CASES.append(_case("blocks-16x64x7x7-%s" % mp, "blocks", (16, 64, 7, 7), mp))
CASES += [
    _case("blocks-8x16x3x3-w65", "blocks", (8, 16, 3, 3), "w65"),
    _case("blocks-9x70x2x13-w63", "blocks", (9, 70, 2, 13), "w63"),
    _case("blocks-16x64x7x7-acc", "blocks", (16, 64, 7, 7), "base", "acc", relu_out=True),
    _case("blocks-17x40x5x5-acc", "blocks", (17, 40, 5, 5), "w65", "acc", relu_out=False),
]
for s in BLK_SPARSE:
    CASES.append(_case("blocks-%s-sparse" % _name(s), "blocks", s, "base", "sparse", relu_out=True))
for (C, K, k) in PAIR_SHAPES:
    CASES.append(_case("pair-%dx%dx%d-base" % (C, K, k), "pair", (C, K, k, k), "base"))
for mp in ("w63", "w65", "tiny", "h1"):
    CASES.append(_case("pair-3x16x7-%s" % mp, "pair", (3, 16, 7, 7), mp))
CASES += [
    _case("pair-4x16x7-w65", "pair", (4, 16, 7, 7), "w65"),
    _case("pair-1x16x7-w63", "pair", (1, 16, 7, 7), "w63"),
    _case("pair-2x5x5-w65", "pair", (2, 5, 5, 5), "w65"),
    _case("pair-4x16x5-w63", "pair", (4, 16, 5, 5), "w63"),
    _case("pair-1x1x3-tiny", "pair", (1, 1, 3, 3), "tiny"),
    _case("pair-3x16x3-h1", "pair", (3, 16, 3, 3), "h1"),
    # the next layer's pooled detection folded in: records as bf16 triples (fold3) / f16 pairs (fold2), floor / ceil
    # pooled sizes of the odd maps, the next filter 3 or 7 wide
    _case("pair-3x16x7-fold3-floor-k7", "pair", (3, 16, 7, 7), "base", "fold3", ceil=False, k2=7),
    _case("pair-3x16x7-fold2-ceil-k3", "pair", (3, 16, 7, 7), "base", "fold2", ceil=True, k2=3),
    _case("pair-4x16x5-fold3-ceil-k3", "pair", (4, 16, 5, 5), "w65", "fold3", ceil=True, k2=3),
    _case("pair-4x16x5-fold2-floor-k7", "pair", (4, 16, 5, 5), "base", "fold2", ceil=False, k2=7),
    _case("pair-3x16x3-fold3-floor-k3", "pair", (3, 16, 3, 3), "w63", "fold3", ceil=False, k2=3),
    _case("pair-1x16x3-fold2-ceil-k7", "pair", (1, 16, 3, 3), "w65", "fold2", ceil=True, k2=7),
    # the layer's own detection in the launch (7x7, one sequence, one unit per workgroup)
    _case("pair-3x16x7-det", "pair", (3, 16, 7, 7), "base", "plain", det=True),
    _case("pair-4x16x7-det-w65", "pair", (4, 16, 7, 7), "w65", "plain", det=True),
    _case("pair-1x9x7-det-w63", "pair", (1, 9, 7, 7), "w63", "plain", det=True),
    _case("pair-3x16x7-det-tiny", "pair", (3, 16, 7, 7), "tiny", "plain", det=True),
    _case("pair-3x16x7-det-fold3", "pair", (3, 16, 7, 7), "base", "fold3", det=True, ceil=False, k2=7),
    _case("pair-3x16x7-det-fold2", "pair", (3, 16, 7, 7), "w65", "fold2", det=True, ceil=True, k2=3),
    # candidate slots beyond the first (256 CUs: grid 2048; a workgroup takes a second unit beyond 2048 units)
    _case("pair-3x16x7-slots01", "pair", (3, 16, 7, 7), None, "plain", 8, slots=True, H=600, W=40),
    _case("pair-3x16x7-slots02", "pair", (3, 16, 7, 7), None, "plain", 8, slots=True, H=1200, W=8),
    _case("pair-3x16x7-slots03", "pair", (3, 16, 7, 7), None, "plain", 8, slots=True, H=1900, W=8),
    _case("pair-3x16x7-slots03-oneseq", "pair", (3, 16, 7, 7), None, "plain", 1, slots=True, H=16500, W=8),
    _case("pair-3x16x7-slots03-fold3", "pair", (3, 16, 7, 7), None, "fold3", 8, slots=True, H=1900, W=8, ceil=False,
          k2=7),
    _case("pair-2x5x5-slots01", "pair", (2, 5, 5, 5), None, "plain", 8, slots=True, H=600, W=40),
    _case("pair-3x16x3-slots03", "pair", (3, 16, 3, 3), None, "plain", 8, slots=True, H=1900, W=8),
]
CASE_BY_ID = {c.id: c for c in CASES}
assert len(CASE_BY_ID) == len(CASES)


def slot_units(c, cus=ASSUMED_CUS):
    """The non-empty units of a slot case as {global unit index: (popA, popB)}: workgroup 5 with a unit in EVERY slot,
    workgroups 100 and 101 with an empty slot 0 and a unit in the last slot (101: in slot 1 as well), workgroup 777 with
    units in the slots 1 and top, the last workgroup, the neighbours 6 and 7 in slot 0, and the last unit of all."""
    m = case_map(c)
    f = pair_form(c.C, c.K, c.kH, m.H, m.W, c.nSeq, cus)
    g, T, total = f["grid"], f["top_slot"], f["total"]
    want = [(5, s) for s in range(T + 1)] + [(100, T), (101, 1), (101, T), (777, 1), (777, T), (g - 1, 0), (g - 1, T - 1),
                                             (6, 0), (7, 0)]
    units = {}
    for j, (b, s) in enumerate(want):
        u = b + s * g
        if 0 <= s and u < total and u not in units:
            units[u] = PAIRS[(3 * j + 1) % len(PAIRS)]
    units.setdefault(total - 1, (17, 16))
    return units


def slot_masks(c, cus=ASSUMED_CUS):
    """[sequence] -> [H, W] bool of a slot case."""
    m = case_map(c)
    f = pair_form(c.C, c.K, c.kH, m.H, m.W, c.nSeq, cus)
    rng = np.random.default_rng(zlib.crc32(c.id.encode()))
    masks = np.zeros((c.nSeq, m.H, f["wpr"] * 64), dtype=bool)
    for j, (u, (pa, pb)) in enumerate(sorted(slot_units(c, cus).items())):
        q, ul = divmod(u, f["units"])
        yo, tx = divmod(ul, f["wpr"])
        width = min(64, m.W - 64 * tx)
        for r, pc in enumerate((pa, pb)):
            if 2 * yo + r < m.H:
                masks[q, 2 * yo + r, 64 * tx:64 * tx + 64] = _word(rng, width, pc, j % 3 == 0, j % 3 == 1)[0]
    return [masks[q, :, :m.W].copy() for q in range(c.nSeq)]


def sparse_support(c):
    """[C, H, W] bool: the non-zero delta values of a sparse case, about SPARSE_TAPS per patch."""
    m = case_map(c)
    rng = np.random.default_rng(zlib.crc32(c.id.encode()))
    return rng.random((c.C, m.H, m.W)) < SPARSE_TAPS / (c.C * c.kH * c.kW)


def det_changed(c):
    """[H, W] bool: the input pixels of an own-detection case that change by more than the threshold: isolated pixels,
    a block, the map's corners."""
    m = case_map(c)
    rng = np.random.default_rng(zlib.crc32(c.id.encode()))
    ch = rng.random((m.H, m.W)) < 0.004
    if m.H > 12:
        ch[5:9, m.W // 2 - 10:m.W // 2 + 12] = True
    ch[0, 0] = ch[m.H - 1, m.W - 1] = True
    return ch


def case_masks(c):
    """[sequence] -> [H, W] bool: the listed pixels of a case."""
    o, m = _opt(c), case_map(c)
    if "slots" in o:
        return slot_masks(c)
    if "det" in o:
        return [dilate(det_changed(c), c.kH, c.kW)]
    if c.mode == "sparse":
        return [dilate(sparse_support(c).any(axis=0), c.kH, c.kW)]
    base = pattern(m).mask
    # sequences of a batched case: the map, nothing, every pixel, then shifted copies of the map
    out = []
    for q in range(c.nSeq):
        out.append(base if q == 0 else (np.zeros_like(base) if q == 1 and c.nSeq > 2 else
                                        (np.ones_like(base) if q == 2 else np.roll(base, q, axis=0))))
    return out


def reference_macs(c):
    return sum(int(m.sum()) for m in case_masks(c)) * c.C * c.kH * c.kW * c.K


# -------------------------------------------------------------------------------------------------------------------
# cells
# -------------------------------------------------------------------------------------------------------------------
ROW_FORMS = [("7x7x1", "h1", "NB4+", "rem+"), ("7x7x4", "h1", "NB4+", "rem+"), ("7x7x4", "h2", "NB4+", "rem+"),
             ("rt", "h1", "NB0", "rem+"), ("rt", "h1", "NB1-3", "rem0"), ("rt", "h1", "NB1-3", "rem+"),
             ("rt", "h1", "NB4+", "rem0"), ("rt", "h1", "NB4+", "rem+"), ("rt", "h2", "NB4+", "rem0"),
             ("rt", "h2", "NB4+", "rem+")]


def all_cells():
    """The reachable cells.  Row-segment: 7x7 over 4 padded channels has S = 49 (NB 4, rem 1) and never 256 MFMA steps
    per word; over 16 it has S = 196 (NB 16, rem 4) and shares a word between two workgroups exactly with two chunks; a
    run-time shape with NB = 0 has S = rem > 0, and halves == 2 needs MCW S >= 256, i.e. NB >= 10.  Row pair: the
    own-detection instance has one candidate unit per workgroup."""
    cells = [("rows",) + f + (m,) for f in ROW_FORMS for m in ("plain", "batched", "acc")]
    cells += [("blocks", "kxq%d" % q, m) for q in (1, 2, 3, 4) for m in ("plain", "acc", "sparse")]
    cells += [("pair", "%dx%d" % (k, k), fold, "slot%d" % s) for k in (3, 5, 7) for fold in ("plain", "fold3", "fold2")
              for s in range(PAIR_MAXCAND)]
    cells += [("pair", "7x7det", fold, "slot0") for fold in ("plain", "fold3", "fold2")]
    return cells


def uncovered(cell):
    """Why a reachable cell has no row in CASES, or None if it must have one."""
    if cell[0] == "rows":
        form, mode = cell[1:5], cell[5]
        if mode == "batched" and form not in (("7x7x1", "h1", "NB4+", "rem+"), ("7x7x4", "h2", "NB4+", "rem+"),
                                              ("rt", "h1", "NB4+", "rem+")):
            return ("the batched launch differs only in front of the word's load (blockIdx.y -> a sequence's tensors): "
                    "pinned on one shape per instance, the k-loop forms on the plain cells")
        if mode == "acc" and form not in (("7x7x1", "h1", "NB4+", "rem+"), ("7x7x4", "h2", "NB4+", "rem+"),
                                          ("rt", "h1", "NB0", "rem+"), ("rt", "h1", "NB1-3", "rem+")):
            return ("the accumulate epilogue is per output element behind the k-parts' sum: pinned on both 7x7 "
                    "instances and two run-time shapes, the k-loop forms on the plain cells")
        return None
    if cell[0] == "blocks":
        if cell[2] == "acc" and cell[1] not in ("kxq2",):
            return ("a dense accumulate case differs from the sparse ones, which run the accumulate epilogue at every "
                    "KXQ, only in the operands' density -- pinned at every KXQ by the plain cases")
        return None
    _, inst, fold, slot = cell
    if slot == "slot0" or (inst, fold) == ("7x7", "plain") or (inst, fold, slot) == ("7x7", "fold3", "slot3"):
        return None
    if (inst, fold, slot) in (("5x5", "plain", "slot1"), ("3x3", "plain", "slot3")):
        return None
    return ("the candidate-unit loop with its barriers and waits is one body for every instance and fold: slots 1..3 are "
            "pinned on the 7x7 instance (plain at every depth, with the fold at the deepest) and once each on 5x5 and "
            "3x3, whose patches and k-loops differ; what the instances and folds differ in is pinned at slot 0")
