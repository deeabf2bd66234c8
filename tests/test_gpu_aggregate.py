"""-m gpu tests of the per-pixel kernel application (CBBinary2d('aggregate'), cb_aggr.hip) against the
float64 reference of tests/aggregate_cases.py on the same operand values; the bar is DESIGN 5.34's derived bound."""
import copy
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn

import aggregate_cases as ac
from optest import (dev, gpu_lib as lib, gpu_pkg as pkg, host_words, npdtype, operand_args, pack,  # noqa: F401
                    raw, share_of, stream)

pytestmark = pytest.mark.gpu


class Frame(object):
    """One state of cbinfer_cbaggregate_forward with its masks."""

    def __init__(self, lib, shape, window, step, groups, dtype, fill=77.0):
        (self.Cn, self.H, self.W), self.lib = shape, lib
        self.aggr = ctypes.pointer(lib.Aggr(*window[:4], step, groups))
        assert lib.C.cbinfer_aggregate_supported(self.aggr, *shape) == 1
        self.out = torch.full(shape, fill, dtype=dtype, device="cuda")
        words = lib.C.cbinfer_mask_words(self.H, self.W)
        self.vBits, self.bits = (torch.zeros(words, dtype=torch.int64, device="cuda") for _ in range(2))
        self.mcopy = torch.full((words,), -1, dtype=torch.int64, device="cuda")

    def run(self, w, v, fw=(None, None, 0, None), fv=(None, None, 0, None)):
        ptr, self.keep = self.lib.ptr, (w, v, fw, fv)
        st = self.lib.C.cbinfer_cbaggregate_forward(
            ptr(w), ptr(v), ptr(self.out), ptr(fw[0]), ptr(fw[1]), fw[2], ptr(fw[3]), ptr(fv[0]), ptr(fv[1]), fv[2],
            ptr(fv[3]), ptr(self.vBits), ptr(self.bits), ptr(self.mcopy), self.Cn, self.H, self.W, self.aggr,
            self.lib.dtype_code(w), stream())
        assert st == 0
        return self

    def clean(self):
        return int(self.bits.ne(0).sum()) == 0 and int(self.vBits.ne(0).sum()) == 0


@pytest.mark.parametrize("arith", ["f32", "f16"])
@pytest.mark.parametrize("size", ac.MAPS, ids=["7x70", "3x16"])
@pytest.mark.parametrize("displacement,step,window", ac.WINDOWS, ids=ac.WINDOW_IDS)
def test_values_against_float64(lib, displacement, step, window, size, arith):
    """Every pixel listed, (C, G) over aggregate_cases.CHANNELS_GROUPS: within (T + 1) 2^-24 S of float64 (float16: plus
    the result's own rounding), exactly zero where every tap is outside the map; -s prints the share of the bound,
    DESIGN 5.34 has the worst."""
    for Cn, G in ac.CHANNELS_GROUPS:
        w, v = ac.operands(np.random.default_rng(17), Cn, G, window, size, npdtype(arith))
        f = Frame(lib, v.shape, window, step, G, dev(v).dtype).run(dev(w), dev(v))
        assert np.array_equal(host_words(f.mcopy), pack(np.ones(size, dtype=bool))) and f.clean()
        ref, S = ac.reference(w, v, window, step, G)
        got = f.out.double().cpu().numpy()
        err, bar = np.abs(got - ref), ac.bound(v, ref, S, window)
        assert not raw(f.out).cpu().numpy()[S == 0].any()      # (every tap outside the map: +0)
        share = float((err / np.where(S == 0, 1.0, bar)).max())
        print("share of the bound %r step %d %s C=%d G=%d %s: %.4f" % (displacement, step, size, Cn, G, arith, share))
        assert share <= 1.0, (Cn, G)


@pytest.mark.parametrize("arith", ["f32", "f16"])
@pytest.mark.parametrize("displacement,step,window", ac.WINDOWS, ids=ac.WINDOW_IDS)
def test_change_based_frames_are_the_dense_result(lib, displacement, step, window, arith):
    """The frames of correlation_cases.frames with a := w, b := v, each listing less than half the map: the listed pixels
    equal a fresh every-pixel evaluation bit for bit, the others keep the bits planted there, the mask handed on is the
    numpy footprint exactly, and both working masks are zero afterwards."""
    (Cn, G), size = (40, 5), (7, 70)
    rng = np.random.default_rng(29)
    w, v = ac.operands(rng, Cn, G, window, size, npdtype(arith))
    state = Frame(lib, v.shape, window, step, G, dev(v).dtype)
    for label, form, count, SW, SV in ac.frames(window, step):
        fresh = ac.operands(rng, Cn, G, window, size, npdtype(arith))
        w[:, SW], v[:, SV] = fresh[0][:, SW], fresh[1][:, SV]
        listed = ac.footprint(SW, SV, window, step)
        state.out.fill_(-55.0)      # (planted: a frame may write its footprint and nothing else)
        state.run(dev(w), dev(v), operand_args(form, SW, 0, count), operand_args(form, SV, 0, count))
        full = Frame(lib, v.shape, window, step, G, state.out.dtype).run(dev(w), dev(v))
        assert np.array_equal(host_words(state.mcopy), pack(listed)) and state.clean(), label
        sel = torch.from_numpy(listed).cuda()
        assert torch.equal(raw(state.out)[:, sel], raw(full.out)[:, sel]), label
        assert bool((state.out[:, ~sel] == -55.0).all()), label


class Wired(nn.Module):
    """Local attention by hand: conv (3x3, 3 -> 6) -> {q, k, v} 1x1 convs -> correlate(q, k) -> softmax over the 15
    displacements -> aggregate(weights, v) -> 1x1 conv."""

    def __init__(self, pkg, tdt):
        super(Wired, self).__init__()
        torch.manual_seed(5)
        convs = nn.Sequential(nn.Conv2d(3, 6, 3, padding=1), *(nn.Conv2d(6, 6, 1) for _ in range(3)), nn.Conv2d(6, 4, 1))
        cb = pkg.convert(convs.eval().cuda().to(tdt), threshold=0.0)
        self.conv, self.q, self.k, self.v, self.tail = cb
        self.corr = pkg.CBBinary2d('correlate', displacement=(1, 2))
        self.soft = pkg.CBChannelReduce2d(nn.Softmax(dim=1))
        self.aggr = pkg.CBBinary2d('aggregate', displacement=(1, 2))
        for m in (self.conv, self.q, self.k, self.v, self.corr, self.soft, self.aggr):
            m.propChangeIndexes = True
        self.corr.cloneOutput = self.soft.cloneOutput = self.aggr.cloneOutput = False
        for m in (self.conv, self.q, self.k, self.v, self.tail):
            m.exactF32 = tdt == torch.float32

    def forward(self, x):
        feat = self.conv(x)
        return self.tail(self.aggr(self.soft(self.corr(self.q(feat), self.k(feat))), self.v(feat)))


@pytest.mark.parametrize("tdt", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_hand_wired_chain_eager_and_recorded(pkg, lib, tdt):
    """Six frames of a moving-block sequence, the last three as a FrameProgram: the output equals the same tail fed the
    dense float64 aggregate of the operands the module received, within the convolution tests' tolerance; the operator
    lists a part of the map and is one call of the program."""
    net = Wired(pkg, tdt)
    bare, seen = copy.deepcopy(net.tail), {}
    net.aggr.register_forward_pre_hook(lambda m, args: seen.update(w=args[0][1], v=args[1][1]))
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
            wv = [seen[k][0].cpu().numpy() for k in 'wv']
            dense, _ = ac.reference(wv[0], wv[1], net.aggr.window, 1, 1)
            want = bare(torch.from_numpy(dense[None]).to(tdt).cuda()).float()
            tol = 1e-4 if tdt == torch.float32 else 2 * 2.0 ** -10 * max(1.0, float(want.abs().max()))
            assert float((y.float() - want).abs().max()) <= tol, t
            share = share_of(net.aggr._binWork['copy'], 12, 66)
            assert share == 1.0 if t == 0 else 0.0 < share < 1.0, (t, share)
    assert [fn for fn, _ in prog.calls].count(lib.C.cbinfer_cbaggregate_forward.raw) == 1
