"""The case table of the split-state contraction (tests/splitconv_cases.py), checked without a GPU: every case lands in
the cell it claims on a 256-CU card, every cell of the instance x regime x items table is claimed or listed with the
reason it has no case, the oracle's change list of every case has the claimed length, and the classifier's thresholds
are the library's (its host functions need no GPU)."""
import numpy as np
import pytest

import splitconv_cases as sc
from splitconv_cases import CASES, ASSUMED_CUS, case_form, cell_of

IDS = [c.id for c in CASES]


@pytest.fixture(scope="module")
def C_():
    from cbinfer_amd import _lib
    return _lib.C


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_case_lands_in_its_claimed_cell(case):
    f = case_form(case, ASSUMED_CUS)
    assert cell_of(f) == case.cell, f
    assert f["items"] == f["TP"] * f["MT"] * f["SK"] and f["multi_item"] == (f["items"] > f["grid"])
    if f["SK"] > 1:      # a split never outgrows the slabs or two rounds of the grid
        assert f["items"] <= f["slab_cap"] and f["items"] <= 2 * f["grid"]
    assert sc.reference_macs(case) <= sc.REFERENCE_BUDGET, sc.reference_macs(case)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_case_oracle_list_has_its_count_class(case, oracle):
    """The oracle's own detection + dilation of the case's change set gives the list length the classifier was fed."""
    rng = np.random.default_rng(1)
    x0 = rng.standard_normal((1, case.C, case.H, case.W)).astype(np.float32)
    x1 = x0.copy()
    x1[0, :, sc.changed_pixels(case)] += 1.0
    cm = oracle.changeDetection(x1, x0.copy(), (case.kH, case.kW), 0.5)
    idx = oracle.changeIndexesExtr(cm)
    assert len(idx) == sc.own_count(case)
    assert np.array_equal(cm.astype(bool), sc.dilate(sc.changed_pixels(case), case.kH, case.kW))
    f = case_form(case, ASSUMED_CUS)
    want = {"1": case.kH * case.kW, "BN-1": f["BN"] - 1, "BN": f["BN"], "BN+1": f["BN"] + 1, "all": case.H * case.W}
    if case.count == "some":
        assert 0 < len(idx) < case.H * case.W
    elif case.count == "sparse":
        assert case.mode == "fg" and 0 < len(idx) <= case.H * case.W
    else:
        assert case.count in want and len(idx) == want[case.count]


def test_every_cell_is_claimed_or_accounted_for(capsys):
    claimed = {}
    for c in CASES:
        claimed.setdefault(c.cell, []).append(c.id)
    lines = []
    for cell in sc.all_cells():
        why = sc.uncovered(cell)
        assert (why is None) == (cell in claimed), (cell, why, claimed.get(cell))
        lines.append("%-40s %-16s %-10s %s" % (cell[1], cell[2], cell[3],
                                                 ", ".join(claimed[cell]) if why is None else "NO CASE: " + why))
    assert set(claimed) <= set(sc.all_cells())
    with capsys.disabled():
        print("\nsplit-state contraction: cells and their cases\n" + "\n".join(lines))


def test_named_edges_are_in_the_table():
    for arith in ("x3", "f16x2"):
        mine = [c for c in CASES if c.arith == arith]
        assert {1, 16, 40, 64, 65, 130, 1024} <= {c.K for c in mine}, arith
    assert {1, 2, 3, 5, 8} <= {c.nSeq for c in CASES}
    for bn in (64, 128):
        got = {c.count for c in CASES if sc.tile_height(c.K) == bn}
        assert {"1", "BN-1", "BN", "BN+1"} <= got, (bn, got)
    both = {(c.C, c.kH, c.kW) for c in CASES}
    assert {(16, 3, 3), (32, 1, 5), (64, 3, 5), (64, 5, 5), (32, 7, 7), (16, 15, 15), (32, 15, 1)} <= both
    assert {1, 63, 64, 65, 130} <= {c.W for c in CASES}
    assert any(c.H == 1 for c in CASES) and any(c.H < c.kH and c.W < c.kW for c in CASES)
    g = sc.geom(16, 3, 3)
    assert (g["pair"], g["kWs"], g["nStages"]) == (True, 2, 6)
    assert sc.geom(64, 5, 5)["nStages"] == 50 and sc.geom(32, 7, 7)["nStages"] == 49
    g = sc.geom(16, 15, 15)
    assert (g["pair"], g["kWs"], g["nStages"]) == (True, 8, 120)
    f = sc.split_form("x3", 16, 1024, 3, 3, 60, 70, 1, [4200], ASSUMED_CUS)
    assert (f["TP"], f["MT"], f["items"], f["grid"], f["multi_item"]) == (33, 8, 264, 256, True)


def test_thresholds_are_the_librarys(C_):
    assert C_.cbinfer_split_max_sequences() == sc.MAXSEQ
    for K in (1, 16, 40, 64, 65, 130, 256, 1024):
        assert C_.cbinfer_split_max_mask_words(K) == sc.max_mask_words(K), K
    for H, W in ((1, 1), (1, 130), (70, 1), (37, 63), (37, 64), (37, 65), (270, 8), (2601, 8), (33, 130)):
        assert C_.cbinfer_mask_words(H, W) == sc.mask_words(H, W), (H, W)
    for C in (8, 16, 32, 48, 64, 128):
        for K in (0, 1, 64, 65, 1024, 1025):
            for kH, kW in ((1, 1), (1, 3), (1, 5), (3, 3), (3, 5), (5, 5), (7, 7), (15, 1), (15, 15), (2, 3), (17, 3)):
                ok = bool(C_.cbinfer_split_supported(C, K, kH, kW))
                assert ok == bool(sc.supported(C, K, kH, kW)), (C, K, kH, kW)
                if not ok:
                    continue
                for nSeq, H, W in ((1, 5, 4), (1, 60, 70), (3, 21, 65), (8, 150, 8), (1, 2601, 8), (1, 4200, 8)):
                    assert C_.cbinfer_split_workspace_bytes(nSeq, C, H, W, K, kH, kW) == \
                        sc.workspace_bytes(nSeq, C, H, W, K, kH, kW, ASSUMED_CUS), (nSeq, C, H, W, K, kH, kW)


def test_classifier_follows_the_cu_count():
    big = sc.split_form("x3", 32, 64, 7, 7, 150, 65, 1, [100 * 64], 256)
    small = sc.split_form("x3", 32, 64, 7, 7, 150, 65, 1, [100 * 64], 64)
    assert big["SK"] == 4 and small["SK"] == 1 and small["multi_item"]
    assert sc.split_form("x3", 32, 64, 7, 7, 150, 65, 1, [100 * 64], 256, force=1)["SK"] == 1
    # a forced split is refused beyond the slabs the workspace holds
    assert sc.split_form("x3", 32, 64, 7, 7, 150, 65, 1, [128 * 64], 256, force=4)["SK"] == 4
    assert sc.split_form("x3", 32, 64, 7, 7, 150, 65, 1, [129 * 64], 256, force=4)["SK"] == 1
