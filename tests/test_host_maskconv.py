"""The case table of the mask-driven contractions (tests/maskconv_cases.py), checked without a GPU: every case lands in
the cell it claims on a 256-CU card, every pattern map has the popcounts, edge bits and row pairs it claims, every
reachable cell is claimed or listed with the reason it has no case, the slot cases place their units where they say, and
the classifiers' thresholds are the library's wherever it exposes a host function."""
import numpy as np
import pytest

import maskconv_cases as mc
from maskconv_cases import CASES, ASSUMED_CUS, MAPS, POPCOUNTS

IDS = [c.id for c in CASES]


@pytest.fixture(scope="module")
def C_():
    from cbinfer_amd import _lib
    return _lib.C


def word_popcounts(mask):
    """{(y, tx): popcount} and the packed words of a [H, W] bool mask -- from its bits, not from the generator's notes."""
    H, W = mask.shape
    wpr = (W + 63) // 64
    b = np.zeros((H, wpr * 64), dtype=np.uint8)
    b[:, :W] = mask
    words = np.packbits(b, axis=1, bitorder="little").view(np.uint64).reshape(H, wpr)
    return {(y, tx): int(b[y, 64 * tx:64 * tx + 64].sum()) for y in range(H) for tx in range(wpr)}, words


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_case_lands_in_its_claimed_cell(case):
    assert mc.case_cell(case, ASSUMED_CUS) == case.cell
    assert case.cell in mc.all_cells()
    m = mc.case_map(case)
    if case.kernel == "rows":
        assert mc.row_form(case.C, case.K, case.kH, case.kW)["supported"]
    elif case.kernel == "blocks":
        assert mc.blk_form(case.C, case.K, case.kH, case.kW)["supported"]
    else:
        assert mc.pair_supported(case.C, case.K, case.kH, case.kW, m.H, m.W)
    masks = mc.case_masks(case)
    assert len(masks) == case.nSeq and all(k.shape == (m.H, m.W) for k in masks)
    assert any(k.any() for k in masks)
    assert mc.reference_macs(case) <= mc.REFERENCE_BUDGET, mc.reference_macs(case)


@pytest.mark.parametrize("name", sorted(MAPS))
def test_pattern_map_has_what_it_claims(name):
    m = MAPS[name]
    p = mc.pattern(m)
    assert p.mask.shape == (m.H, m.W)
    assert np.array_equal(p.mask, mc.pattern(m).mask)                   # the same on every call
    assert p.mask[m.H - 1, m.W - 1]                                     # the bottom-right pixel is listed
    pops, words = word_popcounts(p.mask)
    assert {k: v[0] for k, v in p.words.items()} == pops
    for (y, tx), (pc, bit0, top) in p.words.items():
        width = min(64, m.W - 64 * tx)
        if bit0:
            assert (int(words[y, tx]) >> 0) & 1
        if top:
            assert (int(words[y, tx]) >> (width - 1)) & 1
    if m.full:
        assert p.mask.all()
        return
    # bit 0 and the word's last bit are each forced in some words (with a neighbour word or the map's edge beside them)
    assert any(b0 for (_, b0, _) in p.words.values()) or len(p.slots) < 3
    assert any(top for (_, _, top) in p.words.values())
    for (yo, tx, width, pa, pb) in p.slots:
        assert pops[(2 * yo, tx)] == pa and (pb is None) == (2 * yo + 1 >= m.H)
        if pb is not None:
            assert pops[(2 * yo + 1, tx)] == pb


def test_base_map_holds_every_popcount_class_and_row_pair():
    """25 x 130: every popcount of the list in a full-width word, alone in its pair as first and as second row (the
    first two as the odd last row's words), the pairs (64, 64), (17, 16) and (1, 1), a 2-pixel word, an odd last row."""
    m = MAPS["base"]
    assert (m.H, m.W) == (25, 130) and m.W % 4 == 2
    p = mc.pattern(m)
    full = [(pa, pb) for (_, _, width, pa, pb) in p.slots if width == 64]
    assert {pa for (pa, pb) in full if not pb} == set(POPCOUNTS)
    assert {pb for (pa, pb) in full if pa == 0} == set(POPCOUNTS)
    assert (64, 64) in full and (17, 16) in full
    assert sum(1 for (_, pb) in full if pb is None) == 2
    assert (1, 1) in [(pa, pb) for (_, _, width, pa, pb) in p.slots if width == 2]
    odd = [mc.blk_unit_form(pa, pb or 0) for (pa, pb) in full]
    assert any(u["odd"] for u in odd) and any(not u["odd"] for u in odd)
    assert any(u["first_empty"] for u in odd) and any(u["second_empty"] for u in odd)
    assert {u["nTt"] for u in odd} >= {1, 2, 3, 4, 8}
    # the row-segment kernel's per-word forms on these popcounts: 1..4 tiles, 3 rounded up to 4, k-parts 4 / 2 / 1
    f1, f2 = mc.row_form(3, 16, 7, 7), mc.row_form(16, 64, 7, 7)
    got1 = {mc.row_word_form(f1, pc)[0][:3] for pc in POPCOUNTS}
    assert got1 == {(1, 1, 4), (2, 2, 2), (3, 4, 1), (4, 4, 1)}
    got2 = {(nh,) + v[:3] for pc in POPCOUNTS for nh, v in mc.row_word_form(f2, pc).items()}
    assert got2 == {(0, 1, 1, 4), (0, 2, 2, 2), (1, 1, 1, 4), (1, 2, 2, 2)}
    assert mc.row_word_form(mc.row_form(2, 9, 5, 5), 1)[0][3] == [0, 2]          # NB 2 over four k-parts
    assert mc.row_word_form(mc.row_form(4, 16, 3, 3), 64)[0][3] == [0]           # NB 0: the remainder block is all


def test_maps_cover_the_named_widths():
    assert (MAPS["w63"].W, MAPS["w65"].W) == (63, 65)
    assert {MAPS[n].W % 4 for n in ("base", "w63", "w65")} == {1, 2, 3}
    assert (MAPS["tiny"].H, MAPS["tiny"].W) == (2, 3) and MAPS["h1"].H == 1
    for kernel, shapes in (("rows", [(3, 16, 7, 7)]), ("blocks", [(16, 64, 7, 7)]), ("pair", [(3, 16, 7, 7)])):
        for s in shapes:
            got = {c.map for c in CASES if c.kernel == kernel and (c.C, c.K, c.kH, c.kW) == s and c.mode == "plain"}
            assert set(MAPS) <= got, (kernel, s, got)
    # the 16-byte load that ends past the tensor: W % 4 != 0 with the bottom-right pixel listed, for every C
    for C in (1, 2, 3, 4):
        assert any(c.kernel == "pair" and c.C == C and c.map in ("base", "w63", "w65") for c in CASES), C


def test_every_cell_is_claimed_or_accounted_for(capsys):
    claimed = {}
    for c in CASES:
        claimed.setdefault(c.cell, []).append(c.id)
    lines = []
    for cell in mc.all_cells():
        why = mc.uncovered(cell)
        assert (why is None) == (cell in claimed), (cell, why, claimed.get(cell))
        lines.append("%-58s %s" % (" ".join(cell), ", ".join(claimed[cell]) if why is None else "NO CASE: " + why))
    assert set(claimed) <= set(mc.all_cells())
    with capsys.disabled():
        print("\nmask-driven contractions: cells and their cases\n" + "\n".join(lines))


def test_named_forms_are_in_the_table():
    rows = {(c.C, c.K, c.kH, c.kW): mc.row_form(c.C, c.K, c.kH, c.kW) for c in CASES if c.kernel == "rows"}
    want = {(3, 16, 7, 7): dict(instance="7x7x1", NB=4, rem=1),
            (16, 64, 7, 7): dict(instance="7x7x4", MCW=2, groups=2, halves=2, passes=2),
            (16, 16, 7, 7): dict(instance="7x7x4", MCW=1, passes=4),
            (4, 16, 3, 3): dict(NB=0, rem=9), (2, 9, 5, 5): dict(NB=2, rem=1, MCH=1, CP=4),
            (8, 16, 2, 3): dict(rem=0), (4, 8, 3, 4): dict(rem=0), (9, 16, 2, 2): dict(rem=0),
            (24, 16, 7, 7): dict(halves=2, groups=1, MCW=1, passes=6),
            (12, 40, 7, 7): dict(MCH=3, groups=2, halves=2, inactive_chunk_wave=True),
            (5, 33, 4, 2): dict(edge_slots_per_row=1), (1, 1, 1, 33): dict(edge_slots_per_row=32),
            (3, 5, 9, 1): dict(edge_slots_per_row=0), (6, 70, 3, 9): dict(groups=3), (20, 128, 5, 5): dict(groups=4),
            (64, 16, 3, 3): dict(lds=57344, passes=6), (16, 32, 6, 6): dict(halves=2, rem=0),
            (16, 70, 7, 7): dict(consumers_small=3, consumers_big=6)}
    for s, w in want.items():
        for k, v in w.items():
            assert rows[s][k] == v, (s, k, rows[s][k], v)
    assert {2, 3, 6} <= {f[k] for f in rows.values() for k in ("consumers_small", "consumers_big")}
    blks = {(c.C, c.K, c.kH, c.kW): mc.blk_form(c.C, c.K, c.kH, c.kW) for c in CASES if c.kernel == "blocks"}
    want = {(1, 1, 2, 2): dict(SPC=2, own=(1, 1), starved_ring=True), (8, 16, 3, 3): dict(SPC=3, own=(2, 1)),
            (16, 64, 7, 7): dict(CH=2, KXQ=2, SPC=14, MT=4), (17, 40, 5, 5): dict(CH=3, MT=3, ZM=2, inactive_tile=True),
            (24, 33, 3, 9): dict(KXQ=3), (9, 70, 2, 13): dict(KXQ=4), (8, 32, 9, 4): dict(lds=65280, PR=10, PC=68),
            (5, 17, 6, 6): dict(SPC=12), (64, 256, 7, 7): dict(CH=8)}
    for s, w in want.items():
        for k, v in w.items():
            assert blks[s][k] == v, (s, k, blks[s][k], v)
    assert sum(1 for c in CASES if c.kernel == "blocks" and c.mode == "sparse") >= 3
    assert {c.nSeq for c in CASES if c.mode == "batched"} == {2, 8}
    acc = [dict(c.opt)["relu_out"] for c in CASES if c.kernel == "rows" and c.mode == "acc"]
    assert True in acc and False in acc
    pairs = [c for c in CASES if c.kernel == "pair"]
    assert {(c.C, c.K, c.kH) for c in pairs} >= set(mc.PAIR_SHAPES)
    folds = [(c.mode, dict(c.opt)["ceil"], dict(c.opt)["k2"]) for c in pairs if c.mode != "plain"]
    assert {f[0] for f in folds} == {"fold3", "fold2"} and {f[1] for f in folds} == {True, False}
    assert {f[2] for f in folds} == {3, 7}
    dets = [c for c in pairs if "det" in dict(c.opt)]
    assert {c.mode for c in dets} >= {"plain", "fold3"} and all(c.kH == 7 and c.nSeq == 1 for c in dets)


SLOT_IDS = [c.id for c in CASES if "slots" in dict(c.opt)]


@pytest.mark.parametrize("cid", SLOT_IDS)
def test_slot_case_places_its_units(cid):
    """On 256 CUs: the slots the case claims are in use, some workgroup has two non-empty units in different slots and
    another one an empty slot 0 with a non-empty later slot."""
    c = mc.CASE_BY_ID[cid]
    m = mc.case_map(c)
    f = mc.pair_form(c.C, c.K, c.kH, m.H, m.W, c.nSeq, ASSUMED_CUS)
    assert f["total"] > 8 * ASSUMED_CUS and f["top_slot"] >= 1
    nonempty = {}
    for q, mask in enumerate(mc.case_masks(c)):
        pops, _ = word_popcounts(mask)
        for (y, tx), pc in pops.items():
            if pc:
                u = q * f["units"] + (y // 2) * f["wpr"] + tx
                nonempty.setdefault(u % f["grid"], set()).add(u // f["grid"])
    assert set(sum((sorted(s) for s in nonempty.values()), [])) == set(range(f["top_slot"] + 1))
    assert any(len(s) >= 2 for s in nonempty.values())
    assert any(0 not in s for s in nonempty.values())
    assert len(nonempty) <= 16                       # a few pixels: the float64 reference stays tiny


def test_slot_cases_are_the_issues():
    g = lambda cid: mc.pair_form(3, 16, 7, *mc.case_map(mc.CASE_BY_ID[cid])[:2], mc.CASE_BY_ID[cid].nSeq, ASSUMED_CUS)
    f = g("pair-3x16x7-slots01")
    assert (f["total"], f["grid"], f["top_slot"]) == (2400, 2048, 1)
    f = g("pair-3x16x7-slots03")
    assert (f["total"], f["grid"], f["top_slot"]) == (7600, 2048, 3)
    f = g("pair-3x16x7-slots03-oneseq")
    assert (f["total"], f["grid"], f["top_slot"], f["beyond"]) == (8250, 2063, 3, True)
    assert any(c.mode == "fold3" and "slots" in dict(c.opt) for c in CASES)
    # the largest single-sequence map of the older tests stays in slot 0
    assert mc.pair_form(3, 16, 7, 320, 480, 1, ASSUMED_CUS)["top_slot"] == 0
    assert mc.pair_form(3, 16, 7, 600, 40, 8, 64)["grid"] == 600          # the classifier follows the CU count


def test_thresholds_are_the_librarys(C_):
    Ks = (1, 16, 17, 64, 70, 256, 1024)
    for C in range(1, 71):
        for K in Ks:
            for kH in range(1, 17):
                for kW in range(1, 17):
                    f = mc.row_form(C, K, kH, kW)
                    assert bool(C_.cbinfer_rowconv_supported(C, K, kH, kW)) == f["supported"], (C, K, kH, kW)
                    if f["supported"]:
                        assert C_.cbinfer_rowconv_prepared_bytes(C, K, kH, kW) == f["prepared"] == \
                            f["MCH"] * f["G"] * 1024
                    b = mc.blk_form(C, K, kH, kW)
                    assert bool(C_.cbinfer_blockconv_supported(C, K, kH, kW)) == b["supported"], (C, K, kH, kW)
                    if b["supported"]:
                        assert C_.cbinfer_blockconv_prepared_bytes(C, K, kH, kW) == b["prepared"], (C, K, kH, kW)
    # the boundaries of each limit
    for (C, K, kH, kW) in ((1, 1, 1, 33), (1, 1, 1, 34), (1, 1, 33, 2), (1, 1, 34, 2), (1, 1, 1, 1), (0, 1, 3, 3),
                           (1, 0, 3, 3), (64, 16, 3, 3), (64, 16, 4, 3), (65, 16, 3, 3), (68, 16, 3, 3), (36, 16, 7, 7),
                           (32, 16, 7, 7), (28, 16, 7, 7), (16, 160, 7, 7), (16, 176, 7, 7), (4, 1024, 7, 7),
                           (4, 2048, 7, 7), (8, 16, 33, 1), (12, 16, 21, 3), (12, 16, 22, 3)):
        assert bool(C_.cbinfer_rowconv_supported(C, K, kH, kW)) == mc.row_form(C, K, kH, kW)["supported"], (C, K, kH, kW)
    for (C, K, kH, kW) in ((8, 32, 9, 4), (8, 32, 10, 4), (8, 32, 9, 5), (8, 32, 15, 16), (8, 32, 16, 3), (8, 32, 3, 17),
                           (8, 32, 1, 3), (8, 32, 3, 1), (8, 32, 2, 2), (8, 32, 8, 8), (8, 32, 7, 16), (8, 32, 6, 16)):
        assert bool(C_.cbinfer_blockconv_supported(C, K, kH, kW)) == mc.blk_form(C, K, kH, kW)["supported"], (C, K, kH, kW)
    for (H, W) in ((1, 1), (1, 130), (25, 130), (26, 63), (27, 65), (2, 3), (600, 40), (16500, 8), (37, 64), (1, 64)):
        assert C_.cbinfer_mask_words(H, W) == mc.mask_words(H, W), (H, W)
    for C in range(0, 6):
        for K in (0, 1, 15, 16, 17):
            for kH in range(1, 9):
                for kW in (kH, kH + 2):
                    for (H, W) in ((1, 1), (25, 130), (0, 4), (4, 0), (16500, 8), (16384, 4096), (16385, 4096),
                                   (8192, 2047), (8192, 2048)):
                        assert bool(C_.cbinfer_rowpairs_supported(C, K, kH, kW, H, W)) == \
                            mc.pair_supported(C, K, kH, kW, H, W), (C, K, kH, kW, H, W)
