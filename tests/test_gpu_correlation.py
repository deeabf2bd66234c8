"""-m gpu tests of the correlation layer (CBBinary2d('correlate'), cb_corr.hip) against the float64
reference of tests/correlation_cases.py on the same operand values; the bar is DESIGN 5.33's derived bound."""
import copy
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn

import correlation_cases as cc
from optest import (dev, gpu_lib as lib, gpu_pkg as pkg, host_words, npdtype, operand_args, pack,  # noqa: F401
                    raw, stream)

pytestmark = pytest.mark.gpu


class Frame(object):
    """One state of cbinfer_cbcorrelation_forward with its masks."""

    def __init__(self, lib, shape, window, step, normalize, dtype, fill=77.0):
        (self.Cn, self.H, self.W), self.lib = shape, lib
        self.corr = ctypes.pointer(lib.Corr(*window[:4], step, int(normalize)))
        assert lib.C.cbinfer_correlation_supported(self.corr, *shape) == 1
        self.out = torch.full((window[4] * window[5], self.H, self.W), fill, dtype=dtype, device="cuda")
        words = lib.C.cbinfer_mask_words(self.H, self.W)
        self.bBits, self.bits = (torch.zeros(words, dtype=torch.int64, device="cuda") for _ in range(2))
        self.mcopy = torch.full((words,), -1, dtype=torch.int64, device="cuda")

    def run(self, a, b, fa=(None, None, 0, None), fb=(None, None, 0, None)):
        ptr, self.keep = self.lib.ptr, (a, b, fa, fb)
        st = self.lib.C.cbinfer_cbcorrelation_forward(
            ptr(a), ptr(b), ptr(self.out), ptr(fa[0]), ptr(fa[1]), fa[2], ptr(fa[3]), ptr(fb[0]), ptr(fb[1]), fb[2],
            ptr(fb[3]), ptr(self.bBits), ptr(self.bits), ptr(self.mcopy), self.Cn, self.H, self.W, self.corr,
            self.lib.dtype_code(a), stream())
        assert st == 0
        return self

    def clean(self):
        return int(self.bits.ne(0).sum()) == 0 and int(self.bBits.ne(0).sum()) == 0


def operands(rng, shape, arith):
    return [(rng.standard_normal(shape) * 2).astype(npdtype(arith)) for _ in range(2)]


@pytest.mark.parametrize("arith", ["f32", "f16"])
@pytest.mark.parametrize("size", cc.MAPS, ids=["7x70", "3x16"])
@pytest.mark.parametrize("displacement,step,window", cc.WINDOWS, ids=cc.WINDOW_IDS)
def test_values_against_float64(lib, displacement, step, window, size, arith):
    """Every pixel listed, C in {5, 67}, normalised and as the plain sum: within (C + 2) 2^-24 sum_c |a_c b_c| s of
    float64 (float16: plus the result's own rounding); -s prints the share of the bound, DESIGN 5.33 has the worst."""
    for Cn in cc.CHANNELS:
        a, b = operands(np.random.default_rng(17), (Cn,) + size, arith)
        for normalize in (True, False):
            f = Frame(lib, a.shape, window, step, normalize, dev(a).dtype).run(dev(a), dev(b))
            assert np.array_equal(host_words(f.mcopy), pack(np.ones(size, dtype=bool))) and f.clean()
            ref, weight = cc.reference(a, b, window, step, normalize)
            err, bar = np.abs(f.out.double().cpu().numpy() - ref), cc.bound(a, ref, weight)
            assert not err[bar == 0].any()      # (every tap outside the map: exactly zero)
            share = float((err / np.where(bar == 0, 1.0, bar)).max())
            print("share of the bound %r step %d %s C=%d %s %s: %.4f"
                  % (displacement, step, size, Cn, normalize, arith, share))
            assert share <= 1.0, (Cn, normalize)


@pytest.mark.parametrize("arith", ["f32", "f16"])
@pytest.mark.parametrize("displacement,step,window", cc.WINDOWS, ids=cc.WINDOW_IDS)
def test_change_based_frames_are_the_dense_result(lib, displacement, step, window, arith):
    """The frames of correlation_cases.frames, each listing less than half the map: the listed pixels equal a fresh
    every-pixel evaluation bit for bit, the others keep the bits planted there, the mask handed on is the numpy
    footprint exactly, and both working masks are zero afterwards."""
    shape = (67, 7, 70)
    rng = np.random.default_rng(29)
    a, b = operands(rng, shape, arith)
    state = Frame(lib, shape, window, step, True, dev(a).dtype)
    for label, form, count, SA, SB in cc.frames(window, step):
        fresh = operands(rng, shape, arith)
        a[:, SA], b[:, SB] = fresh[0][:, SA], fresh[1][:, SB]
        listed = cc.footprint(SA, SB, window, step)
        state.out.fill_(-55.0)      # (planted: a frame may write its footprint and nothing else)
        state.run(dev(a), dev(b), operand_args(form, SA, 0, count), operand_args(form, SB, 0, count))
        full = Frame(lib, shape, window, step, True, state.out.dtype).run(dev(a), dev(b))
        assert np.array_equal(host_words(state.mcopy), pack(listed)) and state.clean(), label
        sel = torch.from_numpy(listed).cuda()
        assert torch.equal(raw(state.out)[:, sel], raw(full.out)[:, sel]), label
        assert bool((state.out[:, ~sel] == -55.0).all()), label


class Wired(nn.Module):
    """conv (3x3, 3 -> 6) -> CBResize2d(flow from a 2-channel head) -> correlate(features, warped) -> 1x1 conv."""

    def __init__(self, pkg, tdt):
        super(Wired, self).__init__()
        torch.manual_seed(5)
        convs = nn.Sequential(nn.Conv2d(3, 6, 3, padding=1), nn.Conv2d(3, 2, 3, padding=1), nn.Conv2d(15, 4, 1))
        cb = pkg.convert(convs.eval().cuda().to(tdt), threshold=0.0)
        self.conv, self.head, self.tail = cb[0], cb[1], cb[2]
        self.warp = pkg.CBResize2d(mode='bilinear', padding_mode='border', align_corners=False).cuda()
        self.corr = pkg.CBBinary2d('correlate', displacement=(1, 2))
        for m in (self.conv, self.head, self.warp, self.corr):
            m.propChangeIndexes = True
        self.warp.cloneOutput = self.corr.cloneOutput = False
        for m in (self.conv, self.head, self.tail):
            m.exactF32 = tdt == torch.float32

    def forward(self, x):
        feat = self.conv(x)
        return self.tail(self.corr(feat, self.warp(feat, flow=self.head(x))))


@pytest.mark.parametrize("tdt", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_hand_wired_chain_eager_and_recorded(pkg, lib, tdt):
    """Six frames of a moving-block sequence, the last three as a FrameProgram: the output equals the same network with
    the dense formula in the middle within the convolution tests' tolerance, and the operator lists a part of the map."""
    net = Wired(pkg, tdt)
    bare, seen = copy.deepcopy(net.tail), {}
    net.corr.register_forward_pre_hook(lambda m, args: seen.update(a=args[0][1], b=args[1][1]))
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
            ab = [seen[k][0].cpu().numpy() for k in 'ab']
            dense, _ = cc.reference(ab[0], ab[1], net.corr.window, 1, True)
            want = bare(torch.from_numpy(dense[None]).to(tdt).cuda()).float()
            tol = 1e-4 if tdt == torch.float32 else 2 * 2.0 ** -10 * max(1.0, float(want.abs().max()))
            assert float((y.float() - want).abs().max()) <= tol, t
            share = float(np.unpackbits(host_words(net.corr._binWork['copy']).view(np.uint8)).sum()) / (12 * 66)
            assert share == 1.0 if t == 0 else 0.0 < share < 1.0, (t, share)
    assert [fn for fn, _ in prog.calls].count(lib.C.cbinfer_cbcorrelation_forward.raw) == 1
