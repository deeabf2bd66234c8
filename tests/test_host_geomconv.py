"""The case table of the general-geometry contraction (tests/geomconv_cases.py), checked without a GPU: every case
lands in the cell it claims, every required cell of the arithmetic x source x regime x mask-class table is claimed,
every case lists at least one pixel, and the float64 reference of every case stays cheap."""
import numpy as np
import pytest

import geomconv_cases as gc
from geomconv_cases import CASES, CASE_BY_ID, case_form, case_out_hw, case_pixels, case_words, cell_of, geom_form

IDS = [c.id for c in CASES]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_case_lands_in_its_claimed_cell(case):
    f = case_form(case)
    assert cell_of(case, f) == (case.arith, case.source, case.regime, case.mask_class), f
    # the k-split never outgrows the slabs (one per workgroup) or the tickets (one per tile)
    if f["SK"] > 1:
        assert f["items"] <= gc.GRID and f["base"] <= gc.GRID // 2
    # the library's limits
    (kH, kW), s, p, d = case.geom
    assert max(kH, kW) <= 7 and max(s) <= 4 and max(d) <= 8 and max(p) <= 64
    assert case.K in (1, 33, 64, 70, 256)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_case_pixels_and_count_class(case):
    px = case_pixels(case)
    Ho, Wo = case_out_hw(case)
    assert len(px) >= 1
    assert px.dtype == np.int32 and np.all(np.diff(px) > 0) and px[0] >= 0 and px[-1] < Ho * Wo
    assert np.array_equal(px, case_pixels(case))
    want = {"1": 1, "63": 63, "64": 64, "65": 65, "all": Ho * Wo}
    if case.count in want:
        assert len(px) == want[case.count]
    if case.pixels[0] == "last":      # the last valid bit of the last word
        wpr = (Wo + 63) // 64
        assert case_words(case) == Ho * wpr and px[0] == (Ho - 1) * Wo + (wpr - 1) * 64 + (Wo - 1) % 64
    if case.count == "sparse":
        f = case_form(case)
        assert f["chunk"] >= 2
        wpr = (Wo + 63) // 64
        word = (px // Wo) * wpr + (px % Wo) // 64
        used = sorted(set((word // f["chunk"]).tolist()))
        assert used == sorted(case.pixels[1])
        # empty chunks before and behind a populated one
        assert any(u - 1 not in used and u + 1 not in used and 0 < u < f["scan_threads"] - 1 for u in used)


def test_reference_work_stays_small():
    """The float64 reference of a case is one dense convolution of its output map (and one of the absolute values):
    at most 3e8 multiply-adds each."""
    for c in CASES:
        assert gc.reference_macs(c) <= gc.REF_MAC_CAP, (c.id, gc.reference_macs(c))


def test_every_required_cell_is_claimed():
    cells = {(c.arith, c.source, c.regime) for c in CASES}
    for source in ("mask", "list"):
        for regime in gc.REGIMES:
            assert ("F32S", source, regime) in cells, (source, regime)
    for arith in ("F32", "F16"):
        mine = [c for c in CASES if c.arith == arith]
        assert {"nows", "sk_grid", "multi_item"} <= {c.regime for c in mine}, arith
        assert any(c.regime == "sk_cap8" and case_form(c)["stages"] % 8 for c in mine), arith
    for arith in ("F32S", "F32", "F16"):
        assert {c.mask_class for c in CASES if c.arith == arith and c.source == "mask"} == set(gc.MASK_CLASSES), arith
    forms = {c.id: case_form(c) for c in CASES}
    # sk_cap8 with whole and with uneven slices; sk_grid with stages % SK != 0
    cap8 = [forms[c.id]["stages"] for c in CASES if c.regime == "sk_cap8"]
    assert any(s % 8 == 0 for s in cap8) and 49 in cap8
    assert any(forms[c.id]["stages"] % forms[c.id]["SK"] for c in CASES if c.regime == "sk_grid")
    # 'full' at base 511 and 512
    assert {511, 512} <= {forms[c.id]["base"] for c in CASES if c.regime == "full"}
    # the masks: exactly 256 words; chunk 2; chunk 3 with a word count that is no multiple of it
    words = {case_words(c) for c in CASES if c.source == "mask"}
    assert {256, 400, 650} <= words
    f = forms["f32s-mask-sk-stages-650w"]
    assert (f["chunk"], f["scan_threads"], f["words"] % f["chunk"]) == (3, 217, 2)
    assert forms["f32s-mask-one-stage-400w"]["chunk"] == 2 and forms["f32s-mask-nows-256w"]["chunk"] == 1
    # change counts and output channels
    assert {"1", "63", "64", "65", "all", "sparse"} <= {c.count for c in CASES}
    assert {c.K for c in CASES} == {1, 33, 64, 70, 256}
    assert any(c.pixels[0] == "last" for c in CASES)
    for ids in (gc.SPARSE_IDS, gc.DEVICE_COUNT_IDS, gc.OUT_OF_MAP_IDS):
        assert all(i in CASE_BY_ID for i in ids)
    assert sorted(CASE_BY_ID[i].regime for i in gc.SPARSE_IDS) == sorted(gc.REGIMES)
    assert all(CASE_BY_ID[i].arith == "F32S" for i in gc.SPARSE_IDS)
    for i in gc.DEVICE_COUNT_IDS + gc.OUT_OF_MAP_IDS:
        assert CASE_BY_ID[i].source == "list"
    for i in gc.OUT_OF_MAP_IDS:       # room for the foreign entries within numChanges <= Ho Wo
        Ho, Wo = case_out_hw(CASE_BY_ID[i])
        assert len(case_pixels(CASE_BY_ID[i])) + 40 <= Ho * Wo


def test_the_shapes_the_table_was_written_for():
    f = geom_form(64, 16, 3, 3, 6400, True, 0)
    assert (f["Ckk"], f["base"], f["SK"], f["stages"]) == (144, 100, 5, 5)
    f = geom_form(256, 8, 3, 3, 3200, True, 0)
    assert (f["base"], f["SK"], f["stages"]) == (200, 2, 3)
    f = geom_form(64, 32, 7, 7, 64, True, 0)
    assert (f["Ckk"], f["stages"], f["SK"]) == (1568, 49, 8)
    f = geom_form(70, 8, 3, 3, 65, True, 0)
    assert (f["KP"], f["base"], f["SK"]) == (128, 4, 3)
    f = geom_form(256, 3, 3, 3, 96 * 96, True, 0)
    assert (f["items"], f["SK"]) == (576, 1)
    assert geom_form(64, 3, 3, 3, 511 * 64, True, 0)["SK"] == geom_form(64, 3, 3, 3, 512 * 64, True, 0)["SK"] == 1
    assert geom_form(64, 8, 3, 3, 256 * 64, True, 0)["SK"] == 2 and geom_form(64, 8, 3, 3, 257 * 64, True, 0)["SK"] == 1
    assert geom_form(64, 8, 3, 3, 64, False, 0)["SK"] == 1
    assert gc.mask_words(100, 193) == 400 and gc.mask_words(130, 257) == 650 and gc.mask_words(64, 256) == 256


def test_detection_cases():
    assert {gc.detect_waves(C) for C in gc.DET_C} == {1, 2, 3, 4, 8, 16}
    # the pairwise loop's tail at C = G + 1 and 2 G - 1, and C > 32 that is no multiple of 16
    for G in (4, 8):
        assert {C for C in gc.DET_C if gc.detect_waves(C) == G} >= {G, G + 1, 2 * G - 1}, G
    # (16 waves start at C = 32: one pair per wave, then a tail on wave 0 alone / on all waves but the last)
    assert {C for C in gc.DET_C if gc.detect_waves(C) == 16} >= {32, 2 * 16 + 1, 3 * 16 - 1, 48}
    assert {5, 7, 9, 15, 31, 33, 47, 70} <= set(gc.DET_C)
    assert {w % 4 for w in gc.DET_WI} == {0, 1, 2, 3}
    for name in gc.DET_LIMIT_GEOMS:
        runs = gc.detection_runs(name)
        assert {(C, m) for C, _, _, m in runs} == {(C, m) for C in gc.DET_C for m in gc.DET_MODES}
        assert {(W, m) for _, _, W, m in runs} == {(W, m) for W in gc.DET_WI for m in gc.DET_MODES}
        assert all(H == 1 for _, H, _, _ in runs)
        (kH, kW), s, p, d = gc.DET_LIMIT_GEOMS[name]
        for _, H, W, _ in runs:
            assert gc.out_size(H, kH, s[0], p[0], d[0]) >= 1 and gc.out_size(W, kW, s[1], p[1], d[1]) >= 1
            assert H + 2 * p[0] - d[0] * (kH - 1) - 1 >= 0 and W + 2 * p[1] - d[1] * (kW - 1) - 1 >= 0
    # 7 taps at dilation 8, stride 1: one 64-pixel input segment reaches three output mask words
    (kH, kW), s, p, d = gc.DET_LIMIT_GEOMS["7x7d8s1p24"]
    x0 = 64
    lo, hi = x0 + p[1] - (kW - 1) * d[1], x0 + 63 + p[1]
    assert (hi >> 6) - (lo >> 6) + 1 == 3 and gc.out_size(130, kW, s[1], p[1], d[1]) == 130
    assert len(gc.DET_PLAIN) == 11
