"""-m gpu tests of CBBinary2d('deform') (cb_deform.hip) against tests/deform_cases.py; the bar is DESIGN 5.35's bound."""
import copy
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn

import deform_cases as dc
from optest import (bits_of, chain_frames, dev, free_pixel, gpu_lib as lib, gpu_pkg as pkg, host_words,  # noqa: F401
                    npdtype, operand_args, pack, raw, share_of, stream)

pytestmark = pytest.mark.gpu


class Layer(object):      # one state of cbinfer_cbdeform_forward with its prepared weights, masks and workspace
    def __init__(self, lib, case, rng, inSize=(dc.HI, dc.WI)):
        gname, (Cn, Go, K), mod, bias, relu, arith, farith, _ = case
        self.lib, self.geom, self.dims, self.mod, self.relu = lib, dc.GEOMS[gname], (Cn, Go, K), mod, relu
        self.npdt, self.fdt, self.inSize, self.f16 = npdtype(arith), npdtype(farith), inSize, arith == "f16"
        self.size = dc.out_size(self.geom, *inSize)
        self.W = rng.standard_normal((K, Cn) + self.geom[:2]).astype(self.npdt)
        self.bias = rng.standard_normal(K).astype(self.npdt) if bias else None
        self.dtype, fcode = (lib.CB_F16 if a == "f16" else lib.CB_F32 for a in (arith, farith))
        self.d = ctypes.pointer(lib.Deform(lib.Geom(*self.geom), Go, [None, "planes", "sigmoid"].index(mod), fcode, int(relu)))
        nbytes = lib.C.cbinfer_deform_prepared_weights_bytes(K, Cn, self.d, self.dtype)
        self.wp, self.dW, self.dB = torch.zeros(nbytes, dtype=torch.uint8, device="cuda"), dev(self.W), dev(self.bias)
        assert lib.C.cbinfer_deform_prep_weights(lib.ptr(self.dW), lib.ptr(self.wp), K, Cn, self.d, self.dtype, stream()) == 0
        self.out = torch.full((K,) + self.size, 77.0, dtype=self.dW.dtype, device="cuda")
        words = [lib.C.cbinfer_mask_words(*inSize), lib.C.cbinfer_mask_words(*self.size)]
        self.inBits, self.bits = (torch.zeros(n, dtype=torch.int64, device="cuda") for n in words)
        self.mcopy = torch.full((words[1],), -1, dtype=torch.int64, device="cuda")
        self.ws = torch.zeros(lib.C.cbinfer_geom_workspace_bytes(), dtype=torch.uint8, device="cuda")

    def run(self, x, fld, fx=(None, None, 0, None), ff=(None, None, 0, None)):
        ptr, (Cn, _, K) = self.lib.ptr, self.dims
        self.keep = (dev(x), dev(fld), fx, ff)
        return self.lib.C.cbinfer_cbdeform_forward(
            ptr(self.keep[0]), ptr(self.keep[1]), ptr(self.wp), ptr(self.dB), ptr(self.out), ptr(fx[0]), ptr(fx[1]), fx[2],
            ptr(fx[3]), ptr(ff[0]), ptr(ff[1]), ff[2], ptr(ff[3]), ptr(self.inBits), ptr(self.bits), ptr(self.mcopy),
            ptr(self.ws), Cn, *self.inSize, K, self.d, self.dtype, stream())

    def reference(self, x, fld, xChanged):
        ref, S, hit = dc.reference(x, fld, self.W, self.bias, self.geom, self.dims[1], self.mod, self.relu, xChanged)
        return ref, dc.bound(ref, S, self.W, self.dims[0], self.geom[0] * self.geom[1], self.mod, self.f16), hit

def change_sets(geom):
    # (label, x's changed pixels on the input map, the field's on the output map) of the four frames
    kH, kW, sH, sW, pH, pW, dH, dW = geom
    Ho, Wo = dc.out_size(geom)
    sx, sf = (np.zeros((4, dc.HI, dc.WI), dtype=bool), np.zeros((4, Ho, Wo), dtype=bool))
    sx[0, 1:8, 5:60] = sf[0, :2] = True
    sx[1, 3:5, 20:26] = True      # ... and the last tap of ZERO_PIXEL, whose multiplier is exactly 0
    sx[1, dc.ZERO_PIXEL[0] * sH - pH + (kH - 1) * dH, dc.ZERO_PIXEL[1] * sW - pW + (kW - 1) * dW] = True
    sf[2, Ho - 2:, :20] = True
    return list(zip(("both, three tiles and a tail", "x alone", "the field alone", "nothing"), sx, sf))


@pytest.mark.parametrize("case", dc.CASES, ids=["-".join(map(str, c[:1] + c[1] + c[2:7] + c[7])) for c in dc.CASES])
def test_frames_against_float64(lib, case):
    """Four frames through the C ABI: the status, maskCopy == the expected footprint, unlisted pixels keep their bits, both
    working masks zero, and the listed pixels within the derived bound (-s prints the worst share)."""
    rng = np.random.default_rng(41)
    L = Layer(lib, case, rng)
    (Cn, Go, _), forms = L.dims, case[7]
    x = (rng.standard_normal((Cn, dc.HI, dc.WI)) * 2).astype(L.npdt)
    fld = dc.field(rng, L.geom, Go, L.mod, L.fdt)
    before, worst = L.out.cpu().numpy(), 0.0
    for t, (label, SX, SF) in enumerate(change_sets(L.geom)):
        x[:, SX] = (rng.standard_normal((Cn, dc.HI, dc.WI)) * 2).astype(L.npdt)[:, SX]
        fld[:, SF] = dc.field(rng, L.geom, Go, L.mod, L.fdt)[:, SF]
        ref, bar, hit = L.reference(x, fld, SX)
        listed = np.ones(L.size, dtype=bool) if "all" in forms else hit | SF
        assert L.run(x, fld, operand_args(forms[0], SX, free_pixel(SX), bool(t % 2)),
                     operand_args(forms[1], SF, free_pixel(SF), bool(t % 2))) == 0, label
        got = L.out.cpu().numpy()
        assert np.array_equal(host_words(L.mcopy), pack(listed)), label
        assert np.array_equal(bits_of(got)[:, ~listed], bits_of(before)[:, ~listed]), label
        assert int(L.bits.ne(0).sum()) == 0 and int(L.inBits.ne(0).sum()) == 0, label
        assert (t != 0 or listed.sum() > 128) and (t != 1 or listed[dc.ZERO_PIXEL]) and (t != 3 or "all" in forms or
                                                                                         not listed.any()), label
        err = np.abs(got.astype(np.float64) - ref)[:, listed]
        worst = max(worst, float((err / bar[:, listed]).max()) if err.size else 0.0)
        assert np.all(err <= bar[:, listed]), (label, worst)
        before = got
    print("share of the bound %s: %.4f" % ("-".join(map(str, case[:3])), worst))


def test_bits_do_not_depend_on_the_operand_forms(lib):
    """The same frame through (mask, mask) and (list, list): the same bits at every listed pixel."""
    outs = []
    for forms in (("mask", "mask"), ("list", "list")):
        rng = np.random.default_rng(43)
        L = Layer(lib, dc.CASES[1], rng)
        x = (rng.standard_normal((L.dims[0], dc.HI, dc.WI)) * 2).astype(L.npdt)
        fld = dc.field(rng, L.geom, L.dims[1], L.mod, L.fdt)
        _, SX, SF = change_sets(L.geom)[0]
        assert L.run(x, fld, operand_args(forms[0], SX), operand_args(forms[1], SF)) == 0
        outs.append((L.out.cpu().numpy(), host_words(L.mcopy)))
    assert np.array_equal(outs[0][1], outs[1][1]) and outs[0][1].any()
    assert np.array_equal(bits_of(outs[0][0]), bits_of(outs[1][0]))


class Align(nn.Module):      # an mmcv-type DCNv2 block by hand: two CBConv2d (features, the 3 T-plane field), the operator
    def __init__(self, pkg, tdt):
        super(Align, self).__init__()
        torch.manual_seed(7)
        convs = nn.Sequential(nn.Conv2d(8, 8, 3, padding=1), nn.Conv2d(8, 27, 3, padding=1)).eval().cuda().to(tdt)
        self.feat, self.offs = pkg.convert(convs, threshold=0.0)
        self.W, self.b = torch.randn(8, 8, 3, 3).cuda().to(tdt), torch.randn(8).cuda().to(tdt)
        self.dcn = pkg.CBBinary2d('deform', weight=self.W, bias=self.b, padding=1, modulation='sigmoid')
        self.feat.propChangeIndexes = self.offs.propChangeIndexes = True
        self.dcn.cloneOutput = False

    def forward(self, x):
        return self.dcn(self.feat(x), self.offs(x))


@pytest.mark.parametrize("arith", ["f32", "f16"])
def test_hand_wired_block_eager_and_recorded(pkg, arith):
    """Four frames: within the bound of float64 on the activations the module received, a listed share below 1 after
    frame 0, and a FrameProgram replay equal to the eager frames bit for bit."""
    net = Align(pkg, torch.float16 if arith == "f16" else torch.float32)
    twin, seen, prog = copy.deepcopy(net), {}, None
    net.dcn.register_forward_pre_hook(lambda m, args: seen.update(x=args[0][1], f=args[1][1]))
    with torch.no_grad():
        for t, frame in enumerate(chain_frames(np.random.default_rng(47), 4, npdtype(arith))):
            y = net(frame).clone()
            x, f = (seen[k][0].cpu().numpy() for k in 'xf')
            W, b = net.W.cpu().numpy(), net.b.cpu().numpy()
            ref, S, _ = dc.reference(x, f, W, b, dc.GEOMS["3x3"], 1, "sigmoid")
            err = np.abs(y[0].double().cpu().numpy() - ref)
            assert np.all(err <= dc.bound(ref, S, W, 8, 9, "sigmoid", arith == "f16")), t
            share = share_of(net.dcn._binWork['copy'], 20, 70)
            assert share == 1.0 if t == 0 else share < 1.0, (t, share)
            if t == 2:
                prog = pkg.FrameProgram(twin)
            assert torch.equal(raw((prog or twin)(frame)), raw(y)), t
