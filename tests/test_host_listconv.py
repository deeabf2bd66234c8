"""The case table of the list contraction (tests/listconv_cases.py), checked without a GPU: every case lands in the
cell it claims on a 256-CU card, every required cell of the form x regime table is claimed, and the reference of
every case stays cheap."""
import numpy as np
import pytest

import listconv_cases as lc
from listconv_cases import CASES, ASSUMED_CUS, case_form, case_pixels, cell_of, list_form

IDS = [c.id for c in CASES]
TAIL = 37        # garbage entries behind the list in the device-count launches of test_gpu_listconv.py


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_case_lands_in_its_claimed_cell(case):
    f = case_form(case, ASSUMED_CUS)
    assert cell_of(case.dtype, f, case.ws) == case.cell, f
    assert f["kernel"] == ("f16" if case.dtype == "F16" else "f32")
    # ... also when the launch is sized for a longer list than the device count admits
    n = len(case_pixels(case))
    assert cell_of(case.dtype, case_form(case, ASSUMED_CUS, n, n + TAIL), case.ws) == case.cell
    # split-K never outgrows the slabs (one per workgroup) or the ticket words in front of the arrival counters
    if f["SK"] > 1:
        assert f["items"] <= f["grid"] and f["T"] <= 640


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_case_count_class_and_pixels(case):
    f = case_form(case, ASSUMED_CUS)
    px = case_pixels(case)
    HW = case.H * case.W
    assert px.dtype == np.int32 and len(np.unique(px)) == len(px) and px.min() >= 0 and px.max() < HW
    assert np.array_equal(px, case_pixels(case))
    want = {"1": 1, "BN-1": f["BN"] - 1, "BN": f["BN"], "BN+1": f["BN"] + 1, "all": HW}
    if case.count is not None:
        assert len(px) == want[case.count]
    y0, y1, x0, x1 = lc.interior_box(case)
    ys, xs = np.divmod(px, case.W)
    inner = (ys >= y0) & (ys < y1) & (xs >= x0) & (xs < x1)
    ring = (ys == 0) | (ys == case.H - 1) | (xs == 0) | (xs == case.W - 1)
    kind = case.pixels[0]
    if kind == "interior":
        assert inner.all()
        # the fast gather also wants slices without padded k: whole stages (f32) / whole stage pairs (fp16)
        assert f["Ckk"] % (128 if case.dtype == "F16" else 32) == 0
    elif kind == "border":
        assert ring.all() and not inner.any()
        assert {0, case.W - 1, HW - case.W, HW - 1} <= set(px.tolist())        # the four corners
    elif kind == "mixed":
        for w0 in range(0, len(px), 64):
            assert inner[w0:w0 + 64].any() and ring[w0:w0 + 64].any()


def test_reference_work_stays_small():
    for c in CASES:
        assert lc.reference_macs(c) <= 3e8, (c.id, lc.reference_macs(c))


def _claimed(pred):
    return [c for c in CASES if pred(c)]


def test_every_required_cell_is_claimed():
    cells = {c.cell for c in CASES}
    forms = {"F32": ["narrow", "64x64"], "F32S": ["narrow", "64x64", "128x128", "256x64"], "F16": ["narrow", "64x64"]}
    for arith, fs in forms.items():
        for form in fs:
            mine = {(r, i) for (a, f, r, i) in cells if a == arith and f == form}
            regimes = {r for r, _ in mine}
            assert "nows" in regimes, (arith, form)                        # SK = 1 for want of a workspace
            assert "ws_shallow" in regimes, (arith, form)                  # SK = 1 with one: P below the threshold
            if arith == "F32S" and form in ("128x128", "256x64"):
                assert "seam" in regimes, (arith, form)                    # summed by the second launch
            else:
                assert "lastwg" in regimes, (arith, form)                  # summed by the last workgroup
            assert any(i == "multi_item" for _, i in mine), (arith, form)  # a workgroup walks several items
    assert any(r == "seam>8" for (_, _, r, _) in cells)
    # the shapes the issue names
    f = list_form("F32S", 130, 6, 3, 3, 63, False, False, "scatter", ASSUMED_CUS)
    assert (f["KP"], f["form"], f["MT"], f["xmap"]) == (192, "64x64", 3, False)
    f = list_form("F32S", 384, 8, 7, 7, 130, True, False, "scatter", ASSUMED_CUS)
    assert (f["form"], f["MT"], f["xmap"], f["seam"]) == ("128x128", 3, False, True)
    f = list_form("F32", 16, 8, 7, 7, 129, True, False, "scatter", ASSUMED_CUS)
    assert (f["Ckk"], f["CkkP"], f["P"], f["SK"], f["seam"]) == (392, 416, 4, 3, False)
    f = list_form("F16", 16, 19, 7, 7, 129, True, False, "scatter", ASSUMED_CUS)
    assert (f["Ckk"], f["CkkP"], f["P"], f["SK"]) == (931, 1024, 8, 3)
    f = list_form("F32", 256, 4, 3, 3, 96 * 96, True, False, "scatter", ASSUMED_CUS)
    assert (f["T"], f["grid"], f["multi_item"]) == (576, 512, True)
    f = list_form("F32", 64, 48, 7, 7, 40, True, False, "scatter", ASSUMED_CUS)
    assert f["SK"] == 8
    f = list_form("F32S", 256, 81, 7, 7, 100, True, False, "scatter", ASSUMED_CUS)
    assert (f["SK"], f["grid"], f["seam"]) == (32, 256, True)
    for arith in forms:
        assert _claimed(lambda c: c.dtype == arith and c.K == 130) or arith == "F32"
    # three row tiles (no XCD-aware order) on both wide forms, the XCD-aware order elsewhere
    for form in ("64x64", "128x128", "256x64"):
        assert any(case_form(c, ASSUMED_CUS)["MT"] == 3 and not case_form(c, ASSUMED_CUS)["xmap"]
                   for c in CASES if c.cell[1] == form and c.dtype == "F32S"), form
    assert any(case_form(c, ASSUMED_CUS)["xmap"] and case_form(c, ASSUMED_CUS)["MT"] > 1 for c in CASES)


def test_change_counts_and_geometry_are_covered():
    for kernel in ("f32", "f16"):
        mine = [c for c in CASES if (c.dtype == "F16") == (kernel == "f16")]
        assert {"1", "BN-1", "BN", "BN+1", "all"} <= {c.count for c in mine}, kernel
        assert {"interior", "border", "mixed"} <= {c.pixels[0] for c in mine}, kernel
        filters = {(c.kH, c.kW) for c in mine}
        assert {(1, 1), (3, 5), (7, 7), (2, 7)} <= filters, kernel
        assert {1, 63, 64, 65, 130} <= {c.W for c in mine}, kernel
        assert any(c.H == 1 for c in mine), kernel
    assert any(c.dtype == "F16" and c.C % 2 and c.W % 2 for c in CASES)


def test_classifier_follows_the_cu_count():
    # the same shape on a smaller card: fewer slices, or none
    big = list_form("F32S", 256, 81, 7, 7, 100, True, False, "scatter", 256)
    small = list_form("F32S", 256, 81, 7, 7, 100, True, False, "scatter", 16)
    assert big["SK"] == 32 and small["SK"] == 8 and small["grid"] == 16
    # the mask forms always launch the whole grid, and the 1024-thread forms one workgroup per CU
    f = list_form("F32S", 128, 3, 3, 3, 5, False, True, "scatter", 256, n_host=33 * 65)
    assert f["grid"] == 256 and f["NT"] == 1024
    f = list_form("F32", 64, 3, 3, 3, 5, False, True, "scatter", 256, n_host=33 * 65)
    assert f["grid"] == 512
    f = list_form("F32", 64, 3, 3, 3, 5, False, False, "scatter", 256)
    assert f["grid"] == 1
