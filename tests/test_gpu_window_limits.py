"""-m gpu tests of the launch forms of the five window operators of CBBinary2d that their own files leave out: (A) the
grid-stride leg of every persistent loop (correlate, aggregate, deform, attend, attend with partition=) on a map of more
units than the grid has workgroups; (B) the column tile counts NT = 1, 3, 5, 9 of correlate and aggregate -- the NTMAX = 9
kernels, odd NT, taps at +-64 -- on a map of three mask words per row; (C) attention at its channel limits (dv, d > 64) and
over the cell shapes of the partitioned mode; (D) scale= (0, negative, a peaked softmax) and the position bias forms.  The
references, bars and judging functions are those of the operators' own files; a test walks its cases itself, every
assertion names its case."""
import numpy as np
import pytest
import torch

import aggregate_cases as ac
import attend_cases as tc
import correlation_cases as cc
import deform_cases as dc
import winattend_cases as wc
import test_gpu_attend as sliding
import test_gpu_winattend as windowed
from optest import (bits_of, dev, gpu_lib as lib, gpu_pkg as pkg, host_words, npdtype, operand, operand_args,  # noqa: F401
                    pack, raw)
from test_gpu_aggregate import Frame as AggrFrame
from test_gpu_correlation import Frame as CorrFrame, operands as corr_operands
from test_gpu_deform import Layer as DeformLayer

pytestmark = pytest.mark.gpu
DTYPES = ["f32", "f16"]
CONTRACT_GRID = 512      # the workgroups of the deformable convolution's contraction (CBG_GRID), 64 listed pixels a tile


# --------------------------------------------------------------------------------------------- A. the grid-stride leg
def tall_map():
    """(cap, (H, 16)): a map of cap + 5 rows of one mask word each, cap = 8 workgroups per CU being the most a walk's grid
    has (cb_walk_grid) -- the last five rows are walked in a second lap."""
    cap = 8 * torch.cuda.get_device_properties(0).multi_processor_count
    return cap, (cap + 5, 16)


def share(err, bar):
    assert not err[bar == 0].any()
    return float((err / np.where(bar == 0, 1.0, bar)).max())


def check_strided_frame(case, listed, SA, SB, cap, got, full, planted, mcopy, clean):
    """What every change-based frame here must show: both laps have listed rows and idle ones between them, under half
    the map is listed, the listed pixels equal the fresh every-pixel evaluation bit for bit, the others keep the planted
    bits, the handed-on mask is the numpy footprint and the working masks are zero."""
    rows = np.flatnonzero(listed.any(1))
    assert (rows < cap).any() and (rows >= cap).any() and len(rows) < listed.shape[0] // 4, case
    assert SA[:cap].any() and SA[cap:].any() and SB[:cap].any() and SB[cap:].any(), case
    assert listed.mean() < 0.5, case
    assert np.array_equal(host_words(mcopy), pack(listed)) and clean, case
    sel = torch.from_numpy(listed).cuda()
    assert torch.equal(raw(got)[:, sel], raw(full)[:, sel]), case
    assert bool((got[:, ~sel] == planted).all()), case


@pytest.mark.parametrize("arith", DTYPES)
@pytest.mark.parametrize("op", ["correlate", "aggregate"])
def test_correlate_and_aggregate_stride_over_the_grid(lib, op, arith):
    """C = 5 under displacement (1, 2) on the tall map, more words than the grid has workgroups: the every-pixel frame
    within the operator's bound of float64, then a change-based frame on the same state with both operands as lists
    with a device count (the clearing launch behind b's list included)."""
    (cap, size), (_, step, window) = tall_map(), cc.STRIDE_WINDOW
    assert lib.C.cbinfer_mask_words(*size) > cap
    rng = np.random.default_rng(53)

    def draw():
        return corr_operands(rng, (5,) + size, arith) if op == "correlate" else ac.operands(rng, 5, 1, window, size,
                                                                                             npdtype(arith))

    def fresh_state(tdt):
        return (CorrFrame(lib, (5,) + size, window, step, True, tdt) if op == "correlate" else
                AggrFrame(lib, (5,) + size, window, step, 1, tdt))
    a, b = draw()
    state = fresh_state(dev(a).dtype).run(dev(a), dev(b))
    assert np.array_equal(host_words(state.mcopy), pack(np.ones(size, dtype=bool))) and state.clean()
    if op == "correlate":
        ref, weight = cc.reference(a, b, window, step, True)
        bar = cc.bound(a, ref, weight)
    else:
        ref, S = ac.reference(a, b, window, step, 1)
        bar = ac.bound(b, ref, S, window)
    worst = share(np.abs(state.out.double().cpu().numpy() - ref), bar)
    print("share of the bound, strided %s %s %s: %.4f" % (op, size, arith, worst))
    assert worst <= 1.0
    SA, SB = cc.strided_changes(*size, cap)
    fresh = draw()
    a[:, SA], b[:, SB] = fresh[0][:, SA], fresh[1][:, SB]
    listed = cc.footprint(SA, SB, window, step)
    state.out.fill_(-55.0)
    state.run(dev(a), dev(b), operand_args("list", SA, 0, True), operand_args("list", SB, 0, True))
    full = fresh_state(state.out.dtype).run(dev(a), dev(b))
    check_strided_frame((op, arith), listed, SA, SB, cap, state.out, full.out, -55.0, state.mcopy, state.clean())


@pytest.mark.parametrize("arith", DTYPES)
def test_deform_strides_over_both_grids(lib, arith):
    """The 1x1 filter of (C, Go, K) = (8, 1, 8) on the tall map: more words than the footprint launch has workgroups, and
    more 64-pixel tiles in the every-pixel frame than the contraction's grid; then a change-based frame of two lists."""
    cap, size = tall_map()
    case = ("1x1", (8, 1, 8), "planes", False, False, arith, arith, ("list", "list"))
    assert lib.C.cbinfer_mask_words(*size) > cap and -(-size[0] * size[1] // 64) > CONTRACT_GRID
    L = DeformLayer(lib, case, np.random.default_rng(41), size)
    rng = np.random.default_rng(59)
    x = (rng.standard_normal((8,) + size) * 2).astype(L.npdt)
    fld = dc.field(rng, L.geom, 1, L.mod, L.fdt, *size)
    assert L.run(x, fld) == 0
    ref, bar, _ = L.reference(x, fld, None)
    assert np.array_equal(host_words(L.mcopy), pack(np.ones(size, dtype=bool)))
    assert int(L.bits.ne(0).sum()) == 0 and int(L.inBits.ne(0).sum()) == 0
    worst = float((np.abs(L.out.double().cpu().numpy() - ref) / bar).max())
    print("share of the bound, strided deform %s %s: %.4f" % (size, arith, worst))
    assert worst <= 1.0
    SX, SF = cc.strided_changes(*size, cap)
    x[:, SX] = (rng.standard_normal((8,) + size) * 2).astype(L.npdt)[:, SX]
    fld[:, SF] = dc.field(rng, L.geom, 1, L.mod, L.fdt, *size)[:, SF]
    listed = L.reference(x, fld, SX)[2] | SF
    L.out.fill_(-55.0)
    assert L.run(x, fld, operand_args("list", SX, 0, True), operand_args("list", SF, 0, True)) == 0
    full = DeformLayer(lib, case, np.random.default_rng(41), size)
    assert full.run(x, fld) == 0
    clean = int(L.bits.ne(0).sum()) == 0 and int(L.inBits.ne(0).sum()) == 0
    check_strided_frame(("deform", arith), listed, SX, SF, cap, L.out, full.out, -55.0, L.mcopy, clean)


@pytest.mark.parametrize("arith", DTYPES)
@pytest.mark.parametrize("mode", ["sliding", "partition"])
def test_attention_strides_over_the_grid(pkg, mode, arith):
    """d = dv = 5 on the tall map.  Sliding mode, (5, 5, 1) under displacement (1, 2): more words than workgroups.
    Partitioned, three heads under partition (4, 8), shift (1, 3): more words than the footprint launch has workgroups AND
    more (cell, head) units than the frame launch has -- idle units in front of its barrier, kv's working mask cleared by
    head 0's units.  The every-pixel frame within the bound, then a change-based frame of two lists with a device count."""
    cap, size = tall_map()
    assert size[0] * ((size[1] + 63) // 64) > cap
    rng = np.random.default_rng(61)
    if mode == "sliding":
        (displacement, step, window), (Cn, Cv, heads) = cc.STRIDE_WINDOW, (5, 5, 1)
        q, kv, bias = tc.operands(rng, Cn, Cv, heads, window, size, npdtype(arith))

        def fresh_module():
            return sliding.module(pkg, displacement, step, heads, 'mask', bias)
        handed_on = sliding.handed_on
    else:
        part, shift, (Cn, Cv, heads) = (4, 8), (1, 3), (15, 15, 3)
        assert len(wc.cells(part, shift, size)) * heads > cap
        q, kv, bias = wc.operands(rng, Cn, Cv, heads, part, size, npdtype(arith))

        def fresh_module():
            return windowed.module(pkg, part, shift, heads, bias)
        handed_on = windowed.handed_on
    state = fresh_module()
    out = state(dev(q)[None], dev(kv)[None])[1][0].double().cpu().numpy()
    assert np.array_equal(handed_on(state)[0], pack(np.ones(size, dtype=bool))) and handed_on(state)[1]
    if mode == "sliding":
        ref = tc.reference(q, kv, bias, window, step, heads, 'mask', tc.default_scale(Cn, heads))
        bar = tc.bound(ref, window, arith == "f16")
    else:
        ref = wc.reference(q, kv, bias, part, shift, heads, wc.default_scale(Cn, heads))
        bar = wc.bound(ref, arith == "f16")
    worst = share(np.abs(out - ref['out']), bar)
    print("share of the bound, strided attention %s %s %s: %.4f" % (mode, size, arith, worst))
    assert worst <= 1.0
    SQ, SKV = cc.strided_changes(*size, cap)
    fresh = (tc.operands(rng, Cn, Cv, heads, window, size, npdtype(arith)) if mode == "sliding" else
             wc.operands(rng, Cn, Cv, heads, part, size, npdtype(arith)))
    q[:, SQ], kv[:, SKV] = fresh[0][:, SQ], fresh[1][:, SKV]
    listed = cc.footprint(SQ, SKV, window, step) if mode == "sliding" else wc.footprint(SQ, SKV, part, shift)
    state.outputState.fill_(-55.0)
    got = state(operand("list", dev(q)[None], SQ, 0, True), operand("list", dev(kv)[None], SKV, 0, True))[1][0]
    full = fresh_module()(dev(q)[None], dev(kv)[None])[1][0]
    clean = handed_on(state)[1] and not bool(state._binWork['kvBits'].any())
    check_strided_frame((mode, arith), listed, SQ, SKV, cap, got, full, -55.0, state._binWork['copy'], clean)


# ------------------------------------------------------------- B. the column tile counts of correlate and aggregate
LIMIT_RUNS = ([(w, i, cc.LIMIT_MAP) for w, i in zip(cc.LIMIT_WINDOWS, cc.LIMIT_WINDOW_IDS)] +
              [(w, i, cc.MAPS[0]) for w, i in list(zip(cc.LIMIT_WINDOWS, cc.LIMIT_WINDOW_IDS))[2:]])
LIMIT_RUN_IDS = ["%s-%dx%d" % ((i,) + size) for _, i, size in LIMIT_RUNS]


@pytest.mark.parametrize("arith", DTYPES)
@pytest.mark.parametrize("entry,name,size", LIMIT_RUNS, ids=LIMIT_RUN_IDS)
def test_correlate_values_over_the_tile_counts(lib, entry, name, size, arith):
    """correlation_cases.LIMIT_WINDOWS (NT = 1, 3, 5, 9) on 5x150, the two of the NTMAX = 9 kernel on 7x70 as well: every
    pixel listed, C in {5, 67}, normalised and as the plain sum, within test_gpu_correlation.py's bar."""
    displacement, step, window = entry
    for Cn in cc.CHANNELS:
        a, b = corr_operands(np.random.default_rng(17), (Cn,) + size, arith)
        for normalize in (True, False):
            f = CorrFrame(lib, a.shape, window, step, normalize, dev(a).dtype).run(dev(a), dev(b))
            assert np.array_equal(host_words(f.mcopy), pack(np.ones(size, dtype=bool))) and f.clean()
            ref, weight = cc.reference(a, b, window, step, normalize)
            worst = share(np.abs(f.out.double().cpu().numpy() - ref), cc.bound(a, ref, weight))
            print("share of the bound %s NT=%d %s C=%d %s %s: %.4f"
                  % (name, cc.column_tiles(window), size, Cn, normalize, arith, worst))
            assert worst <= 1.0, (Cn, normalize)


@pytest.mark.parametrize("arith", DTYPES)
@pytest.mark.parametrize("entry,name,size", LIMIT_RUNS, ids=LIMIT_RUN_IDS)
def test_aggregate_values_over_the_tile_counts(lib, entry, name, size, arith):
    """The same windows and maps over aggregate_cases.LIMIT_CHANNELS_GROUPS (float16: the zero tile that pads the K axis
    at every one of these NT), within test_gpu_aggregate.py's bar, +0 where every tap is outside the map."""
    displacement, step, window = entry
    for Cn, G in ac.LIMIT_CHANNELS_GROUPS:
        w, v = ac.operands(np.random.default_rng(17), Cn, G, window, size, npdtype(arith))
        f = AggrFrame(lib, v.shape, window, step, G, dev(v).dtype).run(dev(w), dev(v))
        assert np.array_equal(host_words(f.mcopy), pack(np.ones(size, dtype=bool))) and f.clean()
        ref, S = ac.reference(w, v, window, step, G)
        err, bar = np.abs(f.out.double().cpu().numpy() - ref), ac.bound(v, ref, S, window)
        assert not raw(f.out).cpu().numpy()[S == 0].any()
        worst = float((err / np.where(S == 0, 1.0, bar)).max())
        print("share of the bound %s NT=%d %s C=%d G=%d %s: %.4f"
              % (name, cc.column_tiles(window), size, Cn, G, arith, worst))
        assert worst <= 1.0, (Cn, G)


@pytest.mark.parametrize("arith", DTYPES)
@pytest.mark.parametrize("entry,name,size", LIMIT_RUNS, ids=LIMIT_RUN_IDS)
@pytest.mark.parametrize("op", ["correlate", "aggregate"])
def test_change_based_frames_over_the_tile_counts(lib, op, entry, name, size, arith):
    """correlation_cases.frames on the same windows and maps (every frame lists under half the map: frames asserts it),
    C = 67 for correlate and (C, G) = (40, 5) for aggregate: the listed pixels equal a fresh every-pixel evaluation bit for
    bit, the others keep the planted bits, the handed-on mask is the numpy footprint -- taps at +-64 shift b's mask by a
    whole word --, both working masks are zero."""
    displacement, step, window = entry
    rng = np.random.default_rng(29)

    def draw():
        return corr_operands(rng, (67,) + size, arith) if op == "correlate" else ac.operands(rng, 40, 5, window, size,
                                                                                              npdtype(arith))

    def fresh_state(tdt):
        return (CorrFrame(lib, (67,) + size, window, step, True, tdt) if op == "correlate" else
                AggrFrame(lib, (40,) + size, window, step, 5, tdt))
    a, b = draw()
    state = fresh_state(dev(a).dtype)
    for label, form, count, SA, SB in cc.frames(window, step, *size):
        fresh = draw()
        a[:, SA], b[:, SB] = fresh[0][:, SA], fresh[1][:, SB]
        listed = cc.footprint(SA, SB, window, step)
        state.out.fill_(-55.0)
        state.run(dev(a), dev(b), operand_args(form, SA, 0, count), operand_args(form, SB, 0, count))
        full = fresh_state(state.out.dtype).run(dev(a), dev(b))
        assert np.array_equal(host_words(state.mcopy), pack(listed)) and state.clean(), label
        sel = torch.from_numpy(listed).cuda()
        assert torch.equal(raw(state.out)[:, sel], raw(full.out)[:, sel]), label
        assert bool((state.out[:, ~sel] == -55.0).all()), label


# ------------------------------------------------------------------------- C. attention at its channel and cell limits
def test_sliding_attention_values_at_the_channel_limits(pkg):
    """attend_cases.LIMIT_SHAPES -- the second block of v (dv > 64: its own staging, barriers and accumulators), the second
    chunk of k (d > 64), both with tails and full at d = dv = 128 -- under r4 and a window of three column tiles, which
    float16 pads: both borders and dtypes on 7x70, within test_gpu_attend.py's bar."""
    for displacement, step, _ in tc.LIMIT_WINDOWS:
        for arith in DTYPES:
            for border in tc.BORDERS:
                for shape in tc.LIMIT_SHAPES:
                    sliding.judged(pkg, shape, displacement, step, (7, 70), arith, border)


def test_sliding_attention_frames_with_a_second_block_of_v(pkg):
    """test_gpu_attend.py's frame test at (C, Cv, heads) = (8, 80, 1) under attend_cases.LIMIT_WINDOWS: listed pixels equal
    a fresh every-pixel evaluation bit for bit, the others keep the planted bits, the mask is the numpy footprint."""
    for (displacement, step, window), arith in ((w, a) for w in tc.LIMIT_WINDOWS for a in DTYPES):
        (Cn, Cv, heads), size = (8, 80, 1), (7, 70)
        rng = np.random.default_rng(29)
        q, kv, bias = tc.operands(rng, Cn, Cv, heads, window, size, npdtype(arith))
        state = sliding.module(pkg, displacement, step, heads, 'mask', bias)
        state(dev(q)[None], dev(kv)[None])      # (the first frame writes the whole state)
        for label, form, count, SQ, SKV in tc.frames(window, step):
            fresh = tc.operands(rng, Cn, Cv, heads, window, size, npdtype(arith))
            q[:, SQ], kv[:, SKV] = fresh[0][:, SQ], fresh[1][:, SKV]
            listed = tc.footprint(SQ, SKV, window, step)
            state.outputState.fill_(-55.0)      # (planted: a frame may write its footprint and nothing else)
            got = state(operand(form, dev(q)[None], SQ, 0, count), operand(form, dev(kv)[None], SKV, 0, count))[1][0]
            full = sliding.module(pkg, displacement, step, heads, 'mask', bias)(dev(q)[None], dev(kv)[None])[1][0]
            case = (displacement, step, arith, label)
            assert np.array_equal(sliding.handed_on(state)[0], pack(listed)) and sliding.handed_on(state)[1], case
            sel = torch.from_numpy(listed).cuda()
            assert torch.equal(raw(got)[:, sel], raw(full)[:, sel]), case
            assert bool((got[:, ~sel] == -55.0).all()), case


@pytest.mark.parametrize("arith", DTYPES)
@pytest.mark.parametrize("part", wc.LIMIT_PARTITIONS, ids=str)
def test_window_attention_values_over_the_cell_shapes(pkg, part, arith):
    """winattend_cases.LIMIT_PARTITIONS -- every token tile count and padding that PARTITIONS leaves out, one token, one
    row segment across a mask-word boundary, the 31-wide and the 31-high bias table -- over their shifts, the maps of
    test_gpu_winattend.py and one with whole 16-row cells, on two shapes (a bias on the first), within that file's bar; a
    cell of one token hands v on bit for bit (l = p = 1: the arithmetic is exact in both dtypes)."""
    for shift in wc.shifts_within(part):
        for size in wc.LIMIT_MAPS:
            for shape in wc.LIMIT_SHAPES:
                bits, (_, kv), _ = windowed.judged(pkg, shape, part, shift, size, arith)
                if part == (1, 1):
                    assert shift == (0, 0) and np.array_equal(bits, bits_of(kv[shape[0]:])), (size, shape)


# --------------------------------------------------------------------------- D. scale= and the range of the softmax
def test_sliding_attention_scale_and_the_range_of_the_softmax(pkg):
    """scale=: 0 (out is the mean of the values that take part: over the in-map taps under 'mask', over all T under
    'zero'), negative, and attend_cases.PEAKED, where R >= 100 on the float64 reference -- weights that are zero in float32,
    a running maximum that moves by tens between displacement rows -- while the float32 bound still stays below 2^-10 A
    (judged asserts that); then a bias on one head, and a bias handed over as [heads, Dy, Dx]."""
    size, (_, step, window) = (7, 70), tc.WINDOWS[0]
    for arith in DTYPES:
        for border in tc.BORDERS:
            for shape in ((5, 5, 1), (8, 80, 1)):
                _, ref = sliding.judged(pkg, shape, 4, step, size, arith, border, scale=0.0)
                kv = tc.operands(np.random.default_rng(17), *shape, window, size, npdtype(arith))[1]
                mean = tc.uniform_mean(kv, shape[0], window, step, border)
                assert np.abs(ref['out'] - mean).max() <= 1e-12 * np.abs(mean).max(), (shape, border, arith)
            for shape in ((5, 5, 1), (32, 48, 2)):
                sliding.judged(pkg, shape, 4, step, size, arith, border, scale=-(shape[0] // shape[2]) ** -0.5)
            shape, scale = tc.PEAKED
            _, ref = sliding.judged(pkg, shape, 4, step, size, arith, border, scale=scale)
            assert ref['R'].max() >= 100, (border, arith, ref['R'].max())
            sliding.judged(pkg, (5, 5, 1), 4, step, size, arith, border, bias=True)
            sliding.judged(pkg, (32, 48, 2), 4, step, size, arith, border, bias='planes')


@pytest.mark.parametrize("arith", DTYPES)
def test_window_attention_scale_and_the_range_of_the_softmax(pkg, arith):
    """scale=: 0 (out is the mean of the cell's values), negative, and winattend_cases.PEAKED, where R >= 100 on the float64
    reference while the float32 bound still stays below 2^-10 A (judged asserts that); then a bias on one head, and a
    bias handed over flattened."""
    size, part, shift = (16, 24), (7, 7), (3, 3)
    for shape in ((5, 5, 1), (64, 64, 1)):
        _, (_, kv), ref = windowed.judged(pkg, shape, part, shift, size, arith, scale=0.0)
        v, mean = kv[shape[0]:].astype(np.float64), np.zeros_like(ref['out'])
        for (y0, y1), (x0, x1) in wc.cells(part, shift, size):
            mean[:, y0:y1, x0:x1] = v[:, y0:y1, x0:x1].mean(axis=(1, 2), keepdims=True)
        assert np.abs(ref['out'] - mean).max() <= 1e-12 * np.abs(mean).max(), shape
    for shape in ((5, 5, 1), (32, 48, 2)):
        windowed.judged(pkg, shape, part, shift, size, arith, scale=-(shape[0] // shape[2]) ** -0.5)
    shape, part, scale = wc.PEAKED
    for size in wc.MAPS:
        ref = windowed.judged(pkg, shape, part, shift, size, arith, scale=scale)[2]
        assert ref['R'].max() >= 100, (size, ref['R'].max())
    windowed.judged(pkg, (5, 5, 1), part, shift, (16, 24), arith, bias=True)
    windowed.judged(pkg, (32, 48, 2), part, shift, (16, 24), arith, bias='flat')
