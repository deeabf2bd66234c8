"""-m gpu tests of CBBinary2d('attend', partition=) (cb_winattend.hip) against tests/winattend_cases.py's float64
reference and bound.  A test walks its cases itself; every assertion names its case.  DESIGN 5.37 has the worst share."""
import copy

import numpy as np
import pytest
import torch

import winattend_cases as wc
from test_gpu_attend import Wired as Sliding
from optest import (bits_of, dev, gpu_lib as lib, gpu_pkg as pkg, host_words, npdtype, operand, pack, raw,  # noqa: F401
                    share_of)

pytestmark = pytest.mark.gpu
DTYPES = ["f32", "f16"]


def module(pkg, part, shift, heads, bias, scale=None):
    m = pkg.CBBinary2d('attend', partition=part, shift=shift, heads=heads, scale=scale,
                       positionBias=None if bias is None else torch.from_numpy(bias)).cuda()
    m.propChangeIndexes = True
    return m


def handed_on(m):
    return host_words(m._binWork['copy']), not bool(m._binWork['bits'].any())


def judged(pkg, shape, part, shift, size, arith, other=None, scale=None, bias=None):
    """One every-pixel frame against float64 (and `other`, a second float64 formulation) within the bound, which in
    float32 stays below 2^-10 A on the reference alone: (the output's bits, operands, reference).  scale: the module's
    scale= (the reference takes it as the float32 the library is handed), default d ** -0.5; bias: as
    winattend_cases.operands takes it."""
    (Cn, Cv, heads), case = shape, (part, shift, size, shape, arith, scale, bias)
    q, kv, bias = wc.operands(np.random.default_rng(17), Cn, Cv, heads, part, size, npdtype(arith), bias=bias)
    m = module(pkg, part, shift, heads, bias, scale)
    got = m(dev(q)[None], dev(kv)[None])[1][0]
    out = got.double().cpu().numpy()
    assert np.array_equal(handed_on(m)[0], pack(np.ones(size, dtype=bool))) and handed_on(m)[1], case
    scale = wc.default_scale(Cn, heads) if scale is None else float(np.float32(scale))
    ref = wc.reference(q, kv, bias, part, shift, heads, scale)
    assert (wc.bound(ref, False) < 2.0 ** -10 * ref['A']).all(), case
    bar = wc.bound(ref, arith == "f16")
    for want in (ref['out'],) + (() if other is None else (other(q, kv, bias, part, shift, heads, scale),)):
        share = float((np.abs(out - want) / bar).max())
        print("share of the bound", *case, "%.4f" % share)
        assert share <= 1.0, case
    return bits_of(got.cpu().numpy()), (q, kv), ref


@pytest.mark.parametrize("arith", DTYPES)
@pytest.mark.parametrize("part", wc.PARTITIONS, ids=str)
def test_values_against_float64(pkg, part, arith):
    """Every pixel listed, shifts x maps x winattend_cases.SHAPES (a bias on the multi-head ones): within the bound of
    float64, all ones handed on, working masks zero."""
    for shift in wc.shifts(part):
        for size in wc.MAPS:
            for shape in wc.SHAPES:
                judged(pkg, shape, part, shift, size, arith)


@pytest.mark.parametrize("arith", DTYPES)
@pytest.mark.parametrize("part,size", [((7, 7), (14, 21)), ((8, 8), (16, 24))], ids=str)
def test_it_is_swins_shifted_window_attention(pkg, part, size, arith):
    """roll -> window partition -> scores + table bias -> region mask -> softmax -> reverse, in torch float64."""
    judged(pkg, (32, 48, 2), part, (part[0] // 2, part[1] // 2), size, arith, other=wc.swin)


def frames(size):
    """(label, changed pixels of q, of kv) on the 16 x 24 map under partition 7, shift 3: the cells' rows are 0..2, 3..9,
    10..15, their columns 0..2, 3..9, 10..16, 17..23."""
    def at(*pixels):
        S = np.zeros(size, dtype=bool)
        for p in pixels:
            S[p] = True
        return S
    return [("one q pixel", at((5, 5)), at()), ("kv in an interior cell", at(), at((5, 12))),
            ("kv in a clipped corner cell", at(), at((0, 0))), ("two cells of one mask word", at(), at((4, 4), (4, 18))),
            ("nothing", at(), at()), ("everything", ~at(), ~at())]


@pytest.mark.parametrize("form,count", [("mask", False), ("list", False), ("list", True), ("all", False)])
@pytest.mark.parametrize("arith", DTYPES)
def test_change_based_frames_are_the_dense_result(pkg, arith, form, count):
    """Listed pixels equal a fresh every-pixel evaluation bit for bit, the others keep the planted bits, the handed-on
    mask is the numpy footprint (bare operands list every pixel)."""
    (Cn, Cv, heads), size, part, shift = (32, 48, 2), (16, 24), (7, 7), (3, 3)
    rng = np.random.default_rng(29)
    q, kv, bias = wc.operands(rng, Cn, Cv, heads, part, size, npdtype(arith))
    state = module(pkg, part, shift, heads, bias)
    state(dev(q)[None], dev(kv)[None])      # (the first frame writes the whole state)
    for label, SQ, SKV in frames(size):
        fresh = wc.operands(rng, Cn, Cv, heads, part, size, npdtype(arith))
        q[:, SQ], kv[:, SKV] = fresh[0][:, SQ], fresh[1][:, SKV]
        listed = wc.footprint(SQ, SKV, part, shift)
        assert label == "everything" or listed.sum() < listed.size / 2, label
        assert label != "one q pixel" or listed.sum() == 1
        listed = listed | (form == "all")
        state.outputState.fill_(-55.0)      # (planted: a frame may write its footprint and nothing else)
        got = state(operand(form, dev(q)[None], SQ, 0, count), operand(form, dev(kv)[None], SKV, 0, count))[1][0]
        full = module(pkg, part, shift, heads, bias)(dev(q)[None], dev(kv)[None])[1][0]
        assert np.array_equal(handed_on(state)[0], pack(listed)) and handed_on(state)[1], label
        sel = torch.from_numpy(listed).cuda()
        assert torch.equal(raw(got)[:, sel], raw(full)[:, sel]), label
        assert bool((got[:, ~sel] == -55.0).all()), label


class Wired(Sliding):
    """test_gpu_attend.py's block -- conv 3x3 -> q 1x1 and ONE kv 1x1 -> attention -> 1x1 conv -- shifted Swin-type."""

    def __init__(self, pkg, tdt):
        super(Wired, self).__init__(pkg, tdt)
        self.att = pkg.CBBinary2d('attend', partition=(4, 7), shift=(2, 3), heads=2)
        self.att.propChangeIndexes, self.att.cloneOutput = True, False


@pytest.mark.parametrize("tdt", [torch.float32, torch.float16], ids=DTYPES)
def test_hand_wired_block_eager_and_recorded(pkg, lib, tdt):
    """Six frames of a moving block, the last three as a FrameProgram: the output equals the tail fed the float64
    attention of the operands the module received (test_gpu_attend.py's tolerance); one call of the program."""
    net = Wired(pkg, tdt)
    bare, seen = copy.deepcopy(net.tail), {}
    net.att.register_forward_pre_hook(lambda m, args: seen.update(q=args[0][1], kv=args[1][1]))
    rng, prog = np.random.default_rng(31), None
    base = rng.random((1, 3, 12, 66)) * 2 - 1
    with torch.no_grad():
        for t in range(6):
            if t:
                y0, x0 = int(rng.integers(0, 10)), int(rng.integers(0, 60))
                base[:, :, y0:y0 + 2, x0:x0 + 3] = rng.random((1, 3, 2, 3)) * 2 - 1
            if t == 3:
                prog = pkg.FrameProgram(net)
            y = (prog or net)(torch.from_numpy(base).to(tdt).cuda())
            q, kv = (seen[k][0].cpu().numpy() for k in ('q', 'kv'))
            dense = wc.reference(q, kv, None, (4, 7), (2, 3), 2, wc.default_scale(6, 2))['out']
            want = bare(torch.from_numpy(dense[None]).to(tdt).cuda()).float()
            tol = 1e-4 if tdt == torch.float32 else 2 * 2.0 ** -10 * max(1.0, float(want.abs().max()))
            assert float((y.float() - want).abs().max()) <= tol, t
            share = share_of(net.att._binWork['copy'], 12, 66)
            assert share == 1.0 if t == 0 else 0.0 < share < 1.0, (t, share)
    assert [fn for fn, _ in prog.calls].count(lib.C.cbinfer_cbwinattend_forward.raw) == 1
