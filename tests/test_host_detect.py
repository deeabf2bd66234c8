"""The rules and the case table of tests/detect_cases.py, checked without a GPU: every case lands in the cell it claims,
every cell of dtype x form x channel class x update mode is claimed or listed with the reason it cannot be reached, the
named edges are in the table, every case's data has the teeth it is built for, the palette's verdicts are the ones the
contract states in words -- and every rule agrees with the CPU oracle on every case's own data wherever the oracle has
the op: changeDetection, changeDetection_half, changePropagation, changeIndexesExtr, maxPool2d[_half], poolChangeIndexes,
changeDetectionFG, updateOutputFG.  This is where the reference of tests/test_gpu_detect.py is tested alone."""
import numpy as np
import pytest

import detect_cases as dc
from detect_cases import CASES, F16, F32

IDS = [c.id for c in CASES]


def test_every_case_lands_in_its_claimed_cell():
    for c in CASES:
        assert dc.channel_class(c.C) == c.cls and c.C in dc.CHANNELS[c.cls], c.id
        assert dc.unreachable(dc.cell_of(c)) is None, c.id
    assert len(set(IDS)) == len(IDS)


def test_every_cell_is_claimed_or_accounted_for(capsys):
    claimed = {}
    for c in CASES:
        claimed.setdefault(dc.cell_of(c), []).append(c.C)
    lines = []
    for cell in dc.all_cells():
        why = dc.unreachable(cell)
        assert (why is None) == (cell in claimed), (cell, why)
        if why is None:      # every channel count of the class, in every cell
            assert sorted(claimed[cell]) == sorted(dc.CHANNELS[cell[2]]), cell
        lines.append("%-4s %-13s %-5s mode %d  %s" % (cell + (("C = %s" % sorted(claimed[cell])) if why is None
                                                              else "NO CASE: " + why,)))
    assert set(claimed) <= set(dc.all_cells())
    with capsys.disabled():
        print("\nchange detection: cells and their cases (%d cases)\n%s" % (len(CASES), "\n".join(lines)))


def test_constants_are_the_librarys():
    from cbinfer_amd import _lib
    assert _lib.C.cbinfer_split_max_sequences() == dc.MAXSEQ == _lib.SPLIT_MAX_SEQUENCES
    assert (_lib.CB_OK, _lib.CB_ERR_BADARG, _lib.CB_ERR_UNSUPPORTED) == (dc.OK, dc.BADARG, dc.UNSUPPORTED)
    assert (_lib.CB_F32, _lib.CB_F16) == (dc.CODE[F32], dc.CODE[F16])
    for H, W in dc.SIZES:
        assert _lib.C.cbinfer_mask_words(H, W) == dc.pack(np.zeros((H, W), dtype=bool)).size


def test_classifier_on_the_named_channel_counts():
    """The control flow the issue names, per channel count."""
    for C in range(1, 300):      # the classes partition the channel counts
        k = dc.channel_class(C)
        assert k == ("deep" if C > 64 else "few" if C < 4 else "quad" if C % 4 == 0 else "rem"), C
    for C in (1, 2, 3):
        p = dc.paths(C)
        assert p["G"] == 1 and p["keep"] and p["waves"] == [(0, "value", C)]
    assert {dc.paths(C)["G"] for C in dc.CHANNELS["quad"]} == {1, 2, 3, 4, 15, 16}      # 3 and 15 waves included
    for C in dc.CHANNELS["quad"]:
        p = dc.paths(C)
        assert p["keep"] and p["iters"] == [1] and not p["rem_waves"]
    for C in dc.CHANNELS["rem"]:      # the remainder runs on waves 0 .. C - 4 G - 1 only
        p = dc.paths(C)
        assert not p["keep"] and p["iters"] == [1] and p["G"] < 16
        assert p["rem_waves"] == list(range(min(C - 4 * p["G"], p["G"])))      # (one wave: it takes all of them)
        assert sum(w[2] for w in p["waves"]) == C - 4 * p["G"]
    deep = {C: dc.paths(C) for C in dc.CHANNELS["deep"]}
    assert {i for p in deep.values() for i in p["iters"]} == {1, 2, 3, 4}
    assert deep[128]["iters"] == [2] and deep[192]["iters"] == [3] and deep[256]["iters"] == [4]
    assert not deep[128]["rem_waves"] and not deep[192]["rem_waves"] and not deep[256]["rem_waves"]
    assert deep[65]["rem_waves"] == [0] and deep[70]["rem_waves"] == list(range(6)) and deep[129]["rem_waves"] == [0]
    assert deep[127]["iters"] == [1, 2] and deep[127]["waves"][15] == (1, "rem", 3)      # waves of unequal depth
    assert deep[185]["iters"] == [2, 3] and deep[185]["waves"][9] == (2, "rem", 3)
    assert all(not p["keep"] for p in deep.values())


def test_named_edges_are_in_the_table():
    by_form = {}
    for c in CASES:
        by_form.setdefault(c.form, []).append(c)
    assert set(by_form) == set(dc.FORMS)
    for form, cs in by_form.items():
        assert {(c.kH, c.kW) for c in cs} == set(dc.FILTERS), form
        # (a one-column map has no room for the palette: the bit-mask form leaves it to the others)
        assert {c.W for c in cs} == {63, 64, 65, 130} | ({1} if form != "bits" else set()) and {c.H for c in cs} == {1, 5}, form
        for dtype in (F32, F16):
            if form == "batched" and dtype == F16:
                continue
            want = set(dc.THRESHOLDS[dtype][:2] if form == "bits" else dc.THRESHOLDS[dtype])
            assert {c.th for c in cs if c.dtype == dtype} == want, (form, dtype)
    # the byte-map form with more waves than dilated rows: the waves beyond 2 kHH + 1 store nothing
    assert any(dc.detect_groups(c.C) > 2 * (c.kH // 2) + 1 for c in by_form["map"])
    assert any(c.kH // 2 > c.H for c in by_form["map"]) and any(c.kW // 2 == 63 and c.W == 130 for c in by_form["bits"])
    # pooled: every geometry with and without the producer mask, per dtype; both sequence counts, per mode
    for dtype in (F32, F16):
        got = {c.variant for c in by_form["bits_pooled"] if c.dtype == dtype}
        assert got == {g + p for g in dc.GEOMETRIES for p in ("", "+prod")}, (dtype, got)
        assert {c.variant for c in by_form["frame_pooled"] if c.dtype == dtype} == set(dc.GEOMETRIES)
    for mode in dc.MODES:
        for cls in dc.CHANNELS:
            assert {c.variant for c in by_form["batched"] if c.mode == mode and c.cls == cls} == {"2", str(dc.MAXSEQ)}
    # every (dtype, channel count, update mode): a bit-mask case at a positive threshold with every channel's pixel and
    # the whole palette
    for dtype in (F32, F16):
        for cls, Cs in dc.CHANNELS.items():
            for C in Cs:
                for mode in dc.MODES:
                    c = [c for c in by_form["bits"] if (c.dtype, c.C, c.mode) == (dtype, C, mode)]
                    assert len(c) == 1 and c[0].th > 0 and c[0].H * c[0].W >= C + dc.PALETTE_ROOM
    assert all(len(dc.palette(d, t, p)) <= dc.PALETTE_ROOM for d in (F32, F16) for t in dc.THRESHOLDS[d]
               for p in (False, True))
    assert {t for t in dc.THRESHOLDS[F16] if np.float16(np.float32(t)) > np.float32(t)} == {0.3}      # th16 rounds up
    assert {t for t in dc.THRESHOLDS[F16] if np.float16(np.float32(t)) < np.float32(t)} == {0.1}      # ... and down


def test_the_palette_says_what_the_contract_says():
    """The verdicts of the rules on the deciding pairs, against the verdicts stated in words -- and the two mistakes no
    random test notices change them: a comparison in the wrong precision, a threshold that is not th16."""
    for dtype in (F32, F16):
        for th in sorted(set(dc.THRESHOLDS[dtype])):
            names = set()
            for name, s, v, verdict, every in dc.palette(dtype, th):
                got = bool(dc.changed_values(np.array([v]), np.array([s]), th)[0])
                assert got == verdict, (dtype, th, name)
                names.add(name)
            if th > 0:
                assert {"exact-th", "ulp-above", "nan-in", "nan-state", "inf-inf", "inf-finite", "zero-signs"} <= names
            if th > 0 and dtype == F16:
                assert {"ulp-below", "quarter-above-rounds-onto-th", "tie-above", "tie-below"} <= names
            if th == 0:
                assert "subnormal" in names
            if th < 0:
                assert {"equal", "nan-all"} <= names
    pal = {e[0]: e for e in dc.palette(F32, 0.3)}
    _, s, v, _, _ = pal["rounds-onto-th"]      # float64 arithmetic would call it changed
    assert float(s) - float(v) > float(np.float32(0.3)) and np.float32(s - v) == np.float32(0.3)
    pal = {e[0]: e for e in dc.palette(F16, 0.3)}
    _, s, v, _, _ = pal["quarter-above-rounds-onto-th"]      # so would a comparison of the f32 difference with th16
    assert np.float32(s) - np.float32(v) > np.float32(np.float16(np.float32(0.3)))
    _, s, v, _, _ = pal["exact-th"]      # and a comparison with the f32 threshold calls th16 itself changed
    assert np.float32(s) - np.float32(v) > np.float32(0.3)
    assert pal["tie-above"][3] is True and {e[0]: e for e in dc.palette(F16, 0.1)}["tie-above"][3] is False


def _oracle_detection(oracle, x, state, filt, th, update):
    st = state[None].copy()      # (the oracle refreshes in place)
    fn = oracle.changeDetection_half if x.dtype == np.float16 else oracle.changeDetection
    with np.errstate(invalid="ignore", over="ignore"):      # (NaN and infinite differences are part of the data)
        cm = fn(np.ascontiguousarray(x[None]), st, filt, th, updateInputState=update)
    return cm.astype(bool), st[0]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_rules_and_data_of_a_case(case, oracle):
    pooled = case.form.endswith("pooled")
    for q in range(int(case.variant) if case.form == "batched" else 1):
        d = dc.make(case, q)
        state, th = d["state"], case.th
        x = dc.compared(case, d)
        raw, mask, after = dc.expect(case, d)
        # --- the rules against the oracle: the raw map (1x1 support), the dilated map, the feedback refresh
        o_raw, _ = _oracle_detection(oracle, x, state, (1, 1), th, False)
        skipped = ~dc.evaluated(case, d)      # (a segment under zero producer words is not evaluated)
        assert np.array_equal(o_raw & ~skipped, raw) and (th < 0 or not (o_raw & skipped).any())
        o_mask, o_state = _oracle_detection(oracle, x, state, (case.kH, case.kW), th, case.mode == 1)
        assert np.array_equal(o_mask, mask) or (th < 0 and skipped.any())
        assert np.array_equal(oracle.changePropagation(raw.astype(np.int8), (case.kH, case.kW)).astype(bool), mask)
        assert np.array_equal(oracle.changeIndexesExtr(mask.astype(np.int8)), np.flatnonzero(mask))
        if case.mode < 2:
            assert np.array_equal(dc.bits(o_state), dc.bits(after))
        else:
            assert np.array_equal(dc.bits(after), dc.bits(x))
        if pooled:      # the windows hold what the data says, by the oracle's pool over every input pixel
            pH, pW = dc.pooled_size(case)
            assert (case.H, case.W) in ((pH // 2, pW // 2), ((pH + 1) // 2, (pW + 1) // 2))
            every = np.arange(pH * pW, dtype=np.int32)
            got = np.zeros((1,) + d["inp"].shape, dtype=d["inp"].dtype)
            if case.dtype == F16:
                oracle.maxPool2d_half(d["pre"][None], got, every)
            else:
                oracle.maxPool2d(d["pre"][None], got, every)
            pooled_x = dc.pool2(d["pre"], case.H, case.W)
            assert np.array_equal(dc.bits(got[0]), dc.bits(pooled_x)) and np.array_equal(dc.bits(pooled_x), dc.bits(d["inp"]))
            assert not np.isnan(d["pre"]).any()
            if d["prod"] is not None:
                t = dc.touched_segments(d["prod"], pH, pW, case.H, case.W)
                assert t.any() and (t.size == 1 or not t.all())
                if t.size > 1:      # a decoy: a difference under zero producer words that mask or state would show
                    blind = dc.changed(pooled_x, state, th)
                    assert (blind != raw).any() or (dc.bits(dc.update_state(state, pooled_x, blind, 1)) != dc.bits(after)).any()
        # --- the teeth
        ch = dc.changed_values(x, state, th)
        if th >= 0 and d["prod"] is None:
            assert len(d["solo"]) == case.C
            for c, y, px in d["solo"]:      # channel c alone decides its pixel
                assert ch[c, y, px] and ch[:, y, px].sum() == 1, (c, y, px)
                if th > 0 and case.C > 1:      # ... and every other channel differs below the threshold
                    others = np.delete(np.arange(case.C), c)
                    assert (dc.bits(x)[others, y, px] != dc.bits(state)[others, y, px]).all(), (c, y, px)
        for name, y, px, verdict in d["planted"]:
            if d["prod"] is None:
                assert raw[y, px] == verdict, name
        if th > 0:
            quiet = ~raw
            if case.H * case.W > case.C + dc.PALETTE_ROOM:      # sub-threshold drift mode 1 must NOT copy
                assert (dc.bits(x)[:, quiet] != dc.bits(state)[:, quiet]).any()
        if case.form == "bits":
            assert len(d["planted"]) == len(dc.palette(case.dtype, th)) and len(d["solo"]) == case.C
            assert raw.any() and not raw.all()


def test_every_window_position_decides_somewhere():
    """Pooled forms: the value that exceeds the threshold sits in each of the four window positions, and in the windows
    the last row / column clips to two and to one position."""
    for dtype in (F32, F16):
        got = set()
        for c in CASES:
            if c.form.endswith("pooled") and c.dtype == dtype and c.th >= 0:
                got |= set(dc.make(c)["positions"])
        assert {((j, i), 4) for j in (0, 1) for i in (0, 1)} <= got, got
        assert {n for _, n in got} == {1, 2, 4}, got


# ---------------------------------------------------------------------------------------------------------------------
# the other kernels' rules
# ---------------------------------------------------------------------------------------------------------------------
def test_compaction_rule_and_masks(oracle):
    words = {name: dc.pack(dc.compact_mask(H, W, "full")).size for name, H, W in dc.COMPACT_MASKS}
    assert [words[n] for n in ("1w", "63w", "64w", "65w", "130w")] == [1, 63, 64, 65, 130]
    assert words["1920w"] > 1856 and words["3968w"] > 3904      # one and two rounds of the eight-deep prefix loop
    for name, H, W in dc.COMPACT_MASKS:
        for content in dc.COMPACT_CONTENTS:
            m = dc.compact_mask(H, W, content)
            assert np.array_equal(oracle.changeIndexesExtr(m.astype(np.int8)), np.flatnonzero(m)), (name, content)
            back = dc.unpack_mask(dc.pack(m), H, W)
            assert np.array_equal(back[:, :W], m) and not back[:, W:].any()
    assert dc.compact_mask(2, 4150, "last-bit").sum() == 1


@pytest.mark.parametrize("filt", dc.FILTERS)
def test_dilation_rule(oracle, filt):
    for H, W in dc.SIZES:
        raw = np.random.default_rng(H * W).random((H, W)) < 0.05
        raw[H - 1, W - 1] = True
        assert np.array_equal(oracle.changePropagation(raw.astype(np.int8), filt).astype(bool),
                              dc.dilate(raw, filt[0] // 2, filt[1] // 2)), (H, W)


@pytest.mark.parametrize("shape", dc.POOL_SHAPES)
def test_pool_rules(oracle, shape):
    C, iH, iW, ceil = shape
    for dtype in (F32, F16):
        d = dc.pool_data(C, iH, iW, ceil, dtype)
        assert d["n_dev"] < len(d["entries"])
        windows = {((p // iW) // 2, (p % iW) // 2) for p in d["entries"]}
        assert len(windows) < len(d["entries"]) or iH * iW == 1      # several listed pixels per window
        for n in (len(d["entries"]), d["n_dev"]):
            want = dc.max_pool_rule(d["inp"], d["out0"], d["entries"][:n], d["oH"], d["oW"])
            got = d["out0"][None].copy()
            if dtype == F16:
                oracle.maxPool2d_half(d["inp"][None], got, d["entries"][:n])
            else:
                oracle.maxPool2d(d["inp"][None], got, d["entries"][:n])
            assert np.array_equal(dc.bits(got[0]), dc.bits(want))
            if n and n < len(d["entries"]) and iH * iW > 100:      # the outputs no listed window covers keep their pre-fill
                assert (dc.bits(want) == dc.bits(d["out0"])).any() and (dc.bits(want) != dc.bits(d["out0"])).any()
        m = dc.pool_indexes_rule(d["entries"], iW, d["oH"], d["oW"])
        assert np.array_equal(oracle.poolChangeIndexes(d["entries"], (iH, iW), (d["oH"], d["oW"])), np.flatnonzero(m))
        if not ceil and (iH & 1 or iW & 1) and iH > 1:      # entries in the skipped last row / column
            assert any((p // iW) // 2 >= d["oH"] or (p % iW) // 2 >= d["oW"] for p in d["entries"])


def test_per_value_detection_rule(oracle):
    inp, prev, planted = dc.fg_data()
    delta, pred, new = dc.fg_rule(inp, prev, dc.FG_TH, 1)
    diffs, cm = oracle.changeDetectionFG(inp, prev, dc.FG_TH)
    assert np.array_equal(cm.astype(bool), pred) and np.array_equal(dc.bits(diffs), dc.bits(delta))
    for name, i, verdict in planted:
        assert pred[i] == verdict, name
    assert pred.any() and not pred.all() and ((delta == 0) & (inp != prev)).any()
    differs = ~(inp == prev)      # d != 0: a NaN difference counts
    assert np.array_equal(dc.bits(new)[differs], dc.bits(inp)[differs]) and np.array_equal(new[~differs], prev[~differs])
    assert np.array_equal(dc.bits(dc.fg_rule(inp, prev, dc.FG_TH, 0)[2]), dc.bits(prev))


@pytest.mark.parametrize("shape", dc.UPDATE_FG_SHAPES)
def test_scatter_rule_and_its_bar(oracle, shape):
    """The oracle's f32 scatter (one fixed order) lies within the derived bar of the float64 rule; a dropped tap does not."""
    diffs, weight, out0, coords = dc.update_fg_data(*shape)
    want, mag, n = dc.update_fg_rule(diffs, weight, out0, coords)
    bar = dc.update_fg_bar(out0, mag, n)
    got = out0[None].copy()
    oracle.updateOutputFG(diffs, weight, got, coords)
    assert (np.abs(got[0] - want) <= bar).all()
    assert n.max() >= 3 or shape[2] * shape[3] == 1
    w2 = weight.copy()
    w2[:, :, shape[4] // 2, shape[5] // 2] = 0
    assert (np.abs(dc.update_fg_rule(diffs, w2, out0, coords)[0] - want) > bar).any()
    tiny = np.finfo(np.float32).tiny
    assert min(np.abs(diffs).min(), np.abs(weight).min(), np.abs(out0).min()) > 1e6 * tiny
