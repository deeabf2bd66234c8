"""-m gpu tests of CBBinary2d('attend') (cb_attend.hip) against tests/attend_cases.py's float64 reference and bound.  A
test walks its cases itself (the whole file takes a few seconds); every assertion names its case."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn

import attend_cases as ac
from optest import dev, gpu_lib as lib, gpu_pkg as pkg, host_words, npdtype, operand, pack, raw, share_of  # noqa: F401

pytestmark = pytest.mark.gpu


def module(pkg, displacement, step, heads, border, bias, scale=None):
    m = pkg.CBBinary2d('attend', displacement=displacement, step=step, heads=heads, border=border, scale=scale,
                       positionBias=None if bias is None else torch.from_numpy(bias)).cuda()
    m.propChangeIndexes = True
    return m


def handed_on(m):
    return host_words(m._binWork['copy']), not bool(m._binWork['bits'].any())


def judged(pkg, shape, displacement, step, size, arith, border, scale=None, bias=None):
    """One every-pixel frame against float64 within the bound, which in float32 stays below 2^-10 A: (output, reference).
    scale: the module's scale= (the reference takes it as the float32 the library is handed), default d ** -0.5; bias: as
    attend_cases.operands takes it."""
    (Cn, Cv, heads), case = shape, (displacement, step, size, shape, border, arith, scale, bias)
    m = module(pkg, displacement, step, heads, border, None)
    q, kv, bias = ac.operands(np.random.default_rng(17), Cn, Cv, heads, m.window, size, npdtype(arith), bias=bias)
    m = module(pkg, displacement, step, heads, border, bias, scale)
    out = m(dev(q)[None], dev(kv)[None])[1][0]
    assert np.array_equal(handed_on(m)[0], pack(np.ones(size, dtype=bool))) and handed_on(m)[1], case
    ref = ac.reference(q, kv, bias, m.window, step, heads, border,
                       ac.default_scale(Cn, heads) if scale is None else float(np.float32(scale)))
    assert ((ac.bound(ref, m.window, False) < 2.0 ** -10 * ref['A']) | (ref['A'] == 0)).all(), case
    err, bar = np.abs(out.double().cpu().numpy() - ref['out']), ac.bound(ref, m.window, arith == "f16")
    assert not err[bar == 0].any(), case
    share = float((err / np.where(bar == 0, 1.0, bar)).max())
    print("share of the bound", *case, "%.4f" % share)
    assert share <= 1.0, case
    return out, ref


DTYPES = ["f32", "f16"]


def test_values_against_float64(pkg):
    """Every pixel listed: windows x maps x dtypes x borders x attend_cases.SHAPES (a bias on the multi-head ones), then
    windows of one and three column tiles (the four span 2 or 4; float16 pads both to a pair): within the bound of float64,
    all ones handed on, working masks zero; DESIGN 5.36 has the worst printed share."""
    for displacement, step, _ in ac.WINDOWS:
        for size in ac.MAPS:
            for arith in DTYPES:
                for border in ac.BORDERS:
                    for shape in ac.SHAPES:
                        judged(pkg, shape, displacement, step, size, arith, border)
    for displacement in (((-1, 1), (0, 0)), ((-1, 1), (-12, 12))):
        for arith in DTYPES:
            for border in ac.BORDERS:
                judged(pkg, (32, 48, 2), displacement, 1, (7, 70), arith, border)


def test_a_pixel_without_a_tap(pkg):
    """Window ((0, 0), (-3, -1)) on 3x16: column 0 has no in-map tap -- +0 bit for bit under 'mask', within the bound
    of the reference (+0 as well: a uniform softmax over zero values) under 'zero'."""
    for arith in DTYPES:
        for border in ac.BORDERS:
            for shape in ((5, 5, 1), (32, 48, 2)):
                out, ref = judged(pkg, shape, ((0, 0), (-3, -1)), 1, (3, 16), arith, border)
                assert not ref['A'][:, :, 0].any() and (border == 'zero' or not raw(out)[:, :, 0].any()), (arith, shape)


def test_change_based_frames_are_the_dense_result(pkg):
    """correlation_cases.frames (a := q, b := kv; each lists under half the map) per window and dtype: listed pixels equal
    a fresh every-pixel evaluation bit for bit, the others keep the planted bits, the mask is the numpy footprint."""
    for (displacement, step, window), arith in ((w, a) for w in ac.WINDOWS for a in DTYPES):
        (Cn, Cv, heads), size = (32, 48, 2), (7, 70)
        rng = np.random.default_rng(29)
        q, kv, bias = ac.operands(rng, Cn, Cv, heads, window, size, npdtype(arith))
        state = module(pkg, displacement, step, heads, 'mask', bias)
        state(dev(q)[None], dev(kv)[None])      # (the first frame writes the whole state)
        for label, form, count, SQ, SKV in ac.frames(window, step):
            fresh = ac.operands(rng, Cn, Cv, heads, window, size, npdtype(arith))
            q[:, SQ], kv[:, SKV] = fresh[0][:, SQ], fresh[1][:, SKV]
            listed = ac.footprint(SQ, SKV, window, step)
            state.outputState.fill_(-55.0)      # (planted: a frame may write its footprint and nothing else)
            got = state(operand(form, dev(q)[None], SQ, 0, count), operand(form, dev(kv)[None], SKV, 0, count))[1][0]
            full = module(pkg, displacement, step, heads, 'mask', bias)(dev(q)[None], dev(kv)[None])[1][0]
            case = (displacement, step, arith, label)
            assert np.array_equal(handed_on(state)[0], pack(listed)) and handed_on(state)[1], case
            sel = torch.from_numpy(listed).cuda()
            assert torch.equal(raw(got)[:, sel], raw(full)[:, sel]), case
            assert bool((got[:, ~sel] == -55.0).all()), case


class Wired(nn.Module):
    """A NAT-type block by hand: conv 3x3 -> q 1x1 and ONE kv 1x1 (6 -> 12) -> attend, 15 taps, 2 heads -> 1x1 conv."""

    def __init__(self, pkg, tdt):
        super(Wired, self).__init__()
        torch.manual_seed(5)
        convs = nn.Sequential(nn.Conv2d(3, 6, 3, padding=1), nn.Conv2d(6, 6, 1), nn.Conv2d(6, 12, 1), nn.Conv2d(6, 4, 1))
        self.conv, self.q, self.kv, self.tail = pkg.convert(convs.eval().cuda().to(tdt), threshold=0.0)
        self.att = pkg.CBBinary2d('attend', displacement=(1, 2), heads=2)
        for m in (self.conv, self.q, self.kv, self.att):
            m.propChangeIndexes = True
        self.att.cloneOutput = False
        for m in (self.conv, self.q, self.kv, self.tail):
            m.exactF32 = tdt == torch.float32

    def forward(self, x):
        feat = self.conv(x)
        return self.tail(self.att(self.q(feat), self.kv(feat)))


def test_hand_wired_block_eager_and_recorded(pkg, lib):
    """Six frames of a moving block, the last three as a FrameProgram, in both dtypes: the output equals the tail fed the
    float64 attention of the operands the module received (test_gpu_aggregate.py's tolerance); one call of the program."""
    for tdt in (torch.float32, torch.float16):
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
                dense = ac.reference(q, kv, None, net.att.window, 1, 2, 'mask', ac.default_scale(6, 2))['out']
                want = bare(torch.from_numpy(dense[None]).to(tdt).cuda()).float()
                tol = 1e-4 if tdt == torch.float32 else 2 * 2.0 ** -10 * max(1.0, float(want.abs().max()))
                assert float((y.float() - want).abs().max()) <= tol, t
                share = share_of(net.att._binWork['copy'], 12, 66)
                assert share == 1.0 if t == 0 else 0.0 < share < 1.0, (t, share)
        assert [fn for fn, _ in prog.calls].count(lib.C.cbinfer_cbattend_forward.raw) == 1
