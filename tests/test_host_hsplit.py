"""The case table of the fp16 layers on the split-state machinery (tests/hsplit_cases.py), checked without a GPU: every
case lands in the cell it claims on a 256-CU card, every cell of the instance x regime x items table is claimed or listed
with the reason it has no case, no case's float64 reference exceeds the budget, the cases' data changes exactly the
listed pixels under the oracle's half predicate, the classifier's sizes are the library's (its host functions need no
GPU) -- and the per-element bar of tests/test_gpu_hsplit.py has teeth on every case's own data without being too tight:
the float64 result rounded once to f16 and an f32 left-to-right sum of the exact products rounded once both pass it, a
reference without one 64-channel stage of one tap, one without the bias and one whose first padded channel repeats the
last real one each violate it."""
import numpy as np
import pytest

import hsplit_cases as hc
from hsplit_cases import CASES, ASSUMED_CUS, case_form, cell_of

IDS = [c.id for c in CASES]


@pytest.fixture(scope="module")
def C_():
    from cbinfer_amd import _lib
    return _lib.C


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_case_lands_in_its_claimed_cell(case):
    f = case_form(case, ASSUMED_CUS)
    assert f["status"] == hc.OK and cell_of(f) == case.cell, f
    assert f["multi_item"] == (f["items"] > f["grid"]) and f["ranges"][-1][1] == f["items"]
    if f["SK"] > 1:      # a split never outgrows the slabs or two rounds of the grid
        assert f["items"] <= f["slab_cap"] and f["items"] <= 2 * f["grid"]
        for tu, ch in zip(f["tiles"], f["chunks"]):      # at least four stages per chunk, no chunk empty
            b = hc.chunk_bounds(f["nStages"], ch)
            assert tu == 0 or min(np.diff(b)) >= 4, (tu, ch, b)
    assert hc.reference_macs(case) <= hc.REFERENCE_BUDGET, hc.reference_macs(case)
    # frame 0 (every pixel) is a launch the library takes too
    f0 = case_form(case, ASSUMED_CUS, [case.H * case.W] * len(case.Ks))
    assert f0["status"] == hc.OK and f0["instance"] == f["instance"]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_case_data_changes_the_listed_pixels(case, oracle):
    """The oracle's half detection of frame 1 against frame 0 finds the case's change set and nothing else, its
    dilation is the list the classifier was fed, and the list has the length class the case claims."""
    f = case_form(case, ASSUMED_CUS)
    for q in range(len(case.Ks)):
        x0, x1, x2 = hc.make_frames(case, q)
        raw = oracle.changeDetection_half(x1, x0.copy(), (1, 1), hc.TH)
        assert np.array_equal(raw.astype(bool), hc.changed_pixels(case, q)), (case.id, q)
        cm = oracle.changePropagation(raw, (case.kH, case.kW))
        assert np.array_equal(cm.astype(bool), hc.listed_pixels(case, q)), (case.id, q)
        assert not oracle.changeDetection_half(x2, x1.copy(), (1, 1), hc.TH).any()
    n = hc.layer_counts(case)[0]
    want = {"1": case.kH * case.kW, "BN-1": f["BN"] - 1, "BN": f["BN"], "BN+1": f["BN"] + 1, "all": case.H * case.W}
    if case.count == "some":
        assert 0 < n < case.H * case.W
    else:
        assert n == want[case.count], (n, case.count)


def test_every_cell_is_claimed_or_accounted_for(capsys):
    claimed = {}
    for c in CASES:
        claimed.setdefault(c.cell, []).append(c.id)
    lines = []
    for cell in hc.all_cells():
        why = hc.uncovered(cell)
        assert (why is None) == (cell in claimed), (cell, why, claimed.get(cell))
        lines.append("%-28s %-13s %-10s %s" % (cell[0], cell[1], cell[2],
                                               ", ".join(claimed[cell]) if why is None else "NO CASE: " + why))
    assert set(claimed) <= set(hc.all_cells())
    with capsys.disabled():
        print("\nfp16 split-state layers: cells and their cases\n" + "\n".join(lines))


def test_named_edges_are_in_the_table():
    assert {64, 100, 185} <= {c.C for c in CASES}
    k64 = {K for c in CASES for K in c.Ks if case_form(c, ASSUMED_CUS)["BM"] == 64}
    k128 = {K for c in CASES for K in c.Ks if case_form(c, ASSUMED_CUS)["BM"] == 128}
    assert {38, 19} <= k64 and any(K % 32 for K in k128), (k64, k128)
    stages = {(c.C, c.kH, c.kW): case_form(c, ASSUMED_CUS)["nStages"] for c in CASES}
    assert stages[(64, 1, 1)] == 1 and stages[(128, 1, 1)] == 2 and 48 in stages.values()
    assert any(c.kW == 1 and c.kH > 1 for c in CASES)
    for bn in (64, 128):
        got = {c.count for c in CASES if case_form(c, ASSUMED_CUS)["BN"] == bn}
        assert {"1", "BN-1", "BN", "BN+1", "all"} <= got, (bn, got)
    # a stage count its chunk count does not divide: the last chunk differs
    assert hc.chunk_bounds(49, 8) == [0, 6, 12, 18, 24, 30, 36, 42, 49]
    assert hc.chunk_bounds(48, 8) == list(range(0, 49, 6)) and hc.chunk_bounds(1, 1) == [0, 1]
    # the step from 8 to 16 chunks: 63 and 65 stages, and one layer of 147 stages on 32 and on 34 tiles
    by = {c.id: case_form(c, ASSUMED_CUS) for c in CASES}
    assert (by["h64lds-split8-63stages"]["nStages"], by["h64lds-split8-63stages"]["chunks"]) == (63, [8])
    assert (by["h64lds-split16-65stages"]["nStages"], by["h64lds-split16-65stages"]["chunks"]) == (65, [16])
    assert (by["h64lds-split16-c185-32tiles"]["tiles"], by["h64lds-split16-c185-32tiles"]["chunks"]) == ([32], [16])
    assert (by["h64lds-split8-c185-34tiles"]["tiles"], by["h64lds-split8-c185-34tiles"]["chunks"]) == ([34], [8])
    # the group rows: unequal chunk counts and item ranges beside an empty layer; a demoted 128-row layer
    f = by["group-unequal-chunks"]
    assert f["chunks"] == [8, 16] and f["ranges"] == [(0, 264), (264, 264)] and f["SK"] == 16
    f = by["h64lds-shallow-demoted-k130"]
    assert f["demoted"] and (f["BM"], f["KP"], f["MT"]) == (64, 256, 4)
    kinds = set()
    for c in CASES:
        kinds |= set(c.opts)
    assert {"next", "pooled", "prodmask", "upstream", "sample0"} <= kinds
    nn = [hc.n_next(c) for c in CASES if "next" in c.opts]
    assert [1, 2] in nn and any(by[c.id]["reduce_launch"] and by[c.id]["SK"] > 1 for c in CASES if "next" in c.opts)


def test_refusals():
    ok = hc.hsplit_form(64, (38, 19), 3, 3, 9, 17, [1, 1], 256)
    assert ok["status"] == hc.OK and ok["KP"] == 64
    assert hc.hsplit_form(64, (64, 65), 3, 3, 9, 17, [1, 1], 256)["status"] == hc.UNSUPPORTED      # tile height
    assert hc.hsplit_form(64, (65, 129), 3, 3, 9, 17, [1, 1], 256)["status"] == hc.UNSUPPORTED     # padded K
    assert hc.hsplit_form(64, (38,), 3, 3, 9, 17, [1], 256, n_next=[1])["status"] == hc.UNSUPPORTED
    assert hc.hsplit_form(64, (64,), 3, 3, 9, 17, [1], 256, n_next=[2])["status"] == hc.OK
    assert hc.hsplit_form(64, (38,), 7, 7, 9, 17, [1], 256, workspace=False)["status"] == hc.BADARG
    assert hc.hsplit_form(64, (38,), 3, 3, 9, 17, [1], 256, workspace=False)["status"] == hc.OK
    assert hc.hsplit_form(64, (38,), 3, 3, 5121, 8, [1], 256)["status"] == hc.UNSUPPORTED          # mask words of a layer
    assert hc.hsplit_form(64, (38, 38), 3, 3, 2561, 8, [1, 1], 256)["status"] == hc.UNSUPPORTED    # ... of the launch
    assert hc.hsplit_form(64, (38, 38), 3, 3, 2560, 8, [1, 1], 256)["instance"] == hc.H64_MEM
    assert hc.hsplit_form(48, (38,), 3, 3, 9, 17, [1], 256)["status"] == hc.UNSUPPORTED


def test_classifier_follows_the_cu_count():
    # 128 -> 128 channels on 184 x 327: 265 full 128-row tiles -- four per CU on 64 CUs, not on 256
    assert hc.hsplit_form(128, (128,), 3, 3, 184, 327, [100], 256)["BM"] == 64
    assert hc.hsplit_form(128, (128,), 3, 3, 184, 327, [100], 64)["BM"] == 128
    big = hc.hsplit_form(185, (38,), 7, 7, 40, 65, [20 * 64], 256)
    small = hc.hsplit_form(185, (38,), 7, 7, 40, 65, [20 * 64], 64)
    assert big["chunks"] == [16] and small["chunks"] == [4] and small["SK"] == 4


def test_sizes_are_the_librarys(C_):
    assert C_.cbinfer_hsplit_max_mask_words(64) == hc.PRE_MID and C_.cbinfer_hsplit_max_mask_words(65) == hc.PRE_MID
    for C in (32, 63, 64, 65, 100, 128, 185, 512, 1024, 1025):
        for K in (0, 1, 19, 38, 64, 65, 100, 130, 1000, 1024, 1025):
            for kH, kW in ((1, 1), (1, 3), (3, 1), (3, 3), (5, 13), (7, 7), (7, 9), (15, 15), (2, 3), (17, 3)):
                ok = bool(C_.cbinfer_hsplit_supported(C, K, kH, kW))
                assert ok == bool(hc.supported(C, K, kH, kW)), (C, K, kH, kW)
                if not ok:
                    continue
                assert C_.cbinfer_hsplit_prepared_bytes(C, K, kH, kW) == hc.prepared_bytes(C, K, kH, kW), (C, K, kH, kW)
                for H, W in ((9, 17), (1, 1), (20, 65), (129, 64), (1537, 1), (4128, 8)):
                    a = (C, H, W, kH, kW)
                    assert C_.cbinfer_hsplit_state_bytes(*a) == hc.state_bytes(*a), a
                    assert C_.cbinfer_hsplit_workspace_bytes(C, H, W, K, kH, kW) == \
                        hc.workspace_bytes(C, H, W, K, kH, kW, ASSUMED_CUS), (a, K)
                    for nL in (0, 1, 2, 3):
                        assert C_.cbinfer_hsplit_group_workspace_bytes(nL, C, H, W, K, kH, kW) == \
                            hc.group_workspace_bytes(nL, C, H, W, K, kH, kW, ASSUMED_CUS), (nL, a, K)
    for c in CASES:
        K, ws = c.Ks[0], hc.group_workspace_bytes(len(c.Ks), c.C, c.H, c.W, c.Ks[0], c.kH, c.kW, ASSUMED_CUS)
        assert C_.cbinfer_hsplit_group_workspace_bytes(len(c.Ks), c.C, c.H, c.W, K, c.kH, c.kW) == ws, c.id
        f = case_form(c, ASSUMED_CUS)
        assert (ws > 0) == f["deep"] and (not f["deep"] or ws == 256 + f["slab_cap"] * 4 * tile_area(K)), c.id
        assert C_.cbinfer_mask_words(c.H, c.W) == f["MW"], c.id


def tile_area(K):
    return hc.tile_height(K) ** 2


# ---------------------------------------------------------------------------------------------------------------------
# the bar on the cases' own data
# ---------------------------------------------------------------------------------------------------------------------
def test_the_bar_never_exceeds_its_ceiling():
    for c in CASES:
        A = hc.bar_A(c.C, c.kH, c.kW)
        assert 0 < A <= hc.a_ceiling(c.C, c.kH, c.kW), c.id
    # a 16-chunk layer beside one that changes everywhere: the launch runs unsplit, the layer alone split
    g = hc.CASE_BY_ID["group-split16-beside-whole"]
    f = case_form(g, ASSUMED_CUS)
    alone = hc.hsplit_form(g.C, g.Ks[:1], g.kH, g.kW, g.H, g.W, hc.layer_counts(g)[:1], ASSUMED_CUS)
    assert (f["SK"], f["chunks"], alone["SK"], alone["chunks"]) == (1, [16, 8], 16, [16])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_bar_has_teeth_and_is_not_too_tight(case):
    """At the listed pixels of frame 1 (the state of a copy-mode layer is the frame), per layer that lists any."""
    C, kH, kW = case.C, case.kH, case.kW
    A = hc.bar_A(C, kH, kW)
    pad_ch = hc.cpad(C) != C
    for q, K in enumerate(case.Ks):
        idx = np.flatnonzero(hc.listed_pixels(case, q).reshape(-1))
        if not len(idx):
            continue
        w, b = hc.make_weights(case, q)
        state = hc.make_frames(case, q)[1]
        P = C * kH * kW
        wm = w.reshape(K, P).astype(np.float32)
        w64, b64 = wm.astype(np.float64), b.astype(np.float64)
        stage = np.zeros((C, kH, kW), dtype=bool)      # one 64-channel stage of one tap: the centre tap's first
        stage[:64, kH // 2, kW // 2] = True
        stage = stage.reshape(-1)
        last = np.zeros((C, kH, kW), dtype=bool)       # the last real channel, every tap
        last[C - 1] = True
        last = last.reshape(-1)
        found = dict(stage=False, bias=False, pad=False)
        step = max(1, int(3e7 // (K * P)))
        for i in range(0, len(idx), step):
            X = hc.patches(state, idx[i:i + step], kH, kW)
            X64 = X.astype(np.float64)
            want = X64 @ w64.T + b64
            mag = np.abs(X64) @ np.abs(w64).T + np.abs(b64)
            lim = hc.bar(want, mag, A)
            # the reference alone stays within the bar: rounded once ...
            assert np.all(np.abs(want.astype(np.float16).astype(np.float64) - want) <= lim), (case.id, q)
            # ... and summed left to right in f32 (the products of f16 values are exact in f32), rounded once
            prod = X[:, None, :] * wm[None, :, :]
            assert np.array_equal(prod.astype(np.float64), X64[:, None, :] * w64[None, :, :])
            acc = np.add.accumulate(prod, axis=2, dtype=np.float32)[:, :, -1] + b.astype(np.float32)
            assert np.all(np.abs(acc.astype(np.float16).astype(np.float64) - want) <= lim), (case.id, q)
            # three wrong references
            found["stage"] |= bool(np.any(np.abs(X64[:, stage] @ w64[:, stage].T) > lim))
            found["bias"] |= bool(np.any(np.abs(b64)[None, :] > lim))
            if pad_ch:
                found["pad"] |= bool(np.any(np.abs(X64[:, last] @ w64[:, last].T) > lim))
        assert found["stage"], "%s layer %d: a dropped stage passes the bar" % (case.id, q)
        assert found["bias"], "%s layer %d: a dropped bias passes the bar" % (case.id, q)
        assert found["pad"] == pad_ch, "%s layer %d: a live padded channel passes the bar" % (case.id, q)
