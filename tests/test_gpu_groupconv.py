"""-m gpu: the change-based grouped convolution (cb_groupconv.hip, cbinfer_amd/groupconv.py) -- through the
raw C ABI on every case of tests/groupconv_cases.py, then the module, then a ResNeXt-type block.

References (nothing expected comes from the code under test): the values are a float64 CPU
torch.nn.functional.conv2d(..., groups=G) of the tensor the gather reads (never a device convolution); the change rule
is the pinned oracle's with a 1x1 filter and the footprint the twin's tap loop (tests/test_gpu_geom.py, imported).

Bounds, per element, with mag = conv(|x|, |w|, groups=G) + |bias| in float64 and Ckkg = Cg kH kW:
  F32S  |err| <= 64 * 2^-24 * mag
  F32   |err| <= Ckkg * 2^-24 * mag
  F16   |err| <= 2^-11 |ref| + Ckkg * 2^-23 * mag + 2^-24, and 2 fp16 ulp of the layer's largest output.
Operands span many binades (every input channel times exp(U(-6, 3))).  Every unlisted output element must keep its
bits; a guard plane in front of and behind the output must stay untouched."""
import copy
import ctypes
import functools
import zlib

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import groupconv_cases as gc
from groupconv_cases import ARITH, CASE_BY_ID, CASES, SHAPES
from test_gpu_dwconv import Spy
from test_gpu_geom import GEOMS, Twin, footprint, frames_for, out_size
from test_gpu_geomconv import Masks
from test_gpu_listconv import half_tol
from optest import bits_of, dev, gpu_lib as lib, npdtype, pkg, raw, stream, tdtype      # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

FILL = 77.0
TH = 0.05
WORST = {}       # arithmetic -> worst err / mag seen (printed; a measurement, not a bar)


def bound_of(arith, Ckkg, want, mag):
    if arith == "F32S":
        return 64 * 2.0 ** -24 * mag
    if arith == "F32":
        return Ckkg * 2.0 ** -24 * mag
    return 2.0 ** -11 * abs(want) + Ckkg * 2.0 ** -23 * mag + 2.0 ** -24


class Data(object):
    """A shape's tensors on the device in one arithmetic's element type, its prepared weights and its float64 reference
    at EVERY output pixel (without the bias).  Made once per (shape, arithmetic) and never changed."""

    def __init__(self, lib, name, arith):
        s = self.s = SHAPES[name]
        self.name, self.arith = name, arith
        (kH, kW), st, p, d = s.geom
        self.C, self.K, self.Ckkg = s.G * s.Cg, s.G * s.Kg, s.Cg * kH * kW
        rng = np.random.default_rng(zlib.crc32((name + arith).encode()) + 1)
        t = npdtype(arith)
        x = rng.standard_normal((1, self.C, s.Hi, s.Wi)) * np.exp(rng.uniform(-6, 3, (1, self.C, 1, 1)))
        w = rng.standard_normal((self.K, s.Cg, kH, kW)) / np.sqrt(self.Ckkg)
        b = rng.standard_normal(self.K)
        x, w, b = x.astype(t), w.astype(t), b.astype(t)
        x64, w64 = torch.from_numpy(x.astype(np.float64)), torch.from_numpy(w.astype(np.float64))
        kw = dict(stride=st, padding=p, dilation=d, groups=s.G)
        ref, mag = F.conv2d(x64, w64, None, **kw)[0], F.conv2d(x64.abs(), w64.abs(), None, **kw)[0]
        self.Ho, self.Wo = gc.shape_out_hw(s)
        assert tuple(ref.shape) == (self.K, self.Ho, self.Wo)
        self.HW = self.Ho * self.Wo
        self.ref, self.mag = ref.reshape(self.K, -1).cuda(), mag.reshape(self.K, -1).cuda()
        self.b64 = torch.from_numpy(b.astype(np.float64)).cuda()[:, None]
        self.x, self.bias, wd = dev(x), dev(b), dev(w)
        self.g = lib.Geom(kH, kW, st[0], st[1], p[0], p[1], d[0], d[1])
        gp, code = ctypes.byref(self.g), ARITH[arith]
        nbytes = lib.C.cbinfer_groupconv_prepared_weights_bytes(self.K, self.C, s.G, gp, code)
        assert nbytes == gc.prepared_bytes(s.G, s.Cg, s.Kg, kH, kW, 2 if arith == "F16" else 4)
        self.wp = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        lib.check(lib.C.cbinfer_groupconv_prep_weights(wd.data_ptr(), self.wp.data_ptr(), self.K, self.C, s.G, s.Hi, s.Wi,
                                                       gp, code, stream()))
        torch.cuda.synchronize()
        self.px = gc.shape_pixels(name)

    def buffers(self, lib):
        """Frame masks, list and count of the output map, and an output with a guard plane in front and behind."""
        C, dt = lib.C, tdtype(self.arith)
        B = dict(bits=torch.zeros(C.cbinfer_frame_mask_bytes(self.Ho, self.Wo) // 8, dtype=torch.int64, device="cuda"),
                 idx=torch.full((self.HW,), -1, dtype=torch.int32, device="cuda"),
                 count=torch.full((1,), -1, dtype=torch.int32, device="cuda"))
        B['buf'] = torch.full(((self.K + 2) * self.HW,), FILL, dtype=dt, device="cuda")
        B['out'] = B['buf'][self.HW:(self.K + 1) * self.HW]
        return B


@functools.lru_cache(maxsize=None)
def _data(lib, name, arith):
    return Data(lib, name, arith)


def launch(lib, d, B, lst=None, n=0, count=None, bias=True, relu=0):
    """cbinfer_conv_changed_grouped in list mode (lst given) or mask mode."""
    s = d.s
    p = lambda t: t.data_ptr() if t is not None else None
    mask = lst is None
    st = lib.C.cbinfer_conv_changed_grouped(
        d.x.data_ptr(), p(lst), n, p(count), p(B['bits']) if mask else None, p(B['idx']) if mask else None,
        p(B['count']) if mask else None, d.wp.data_ptr(), d.bias.data_ptr() if bias else None, B['out'].data_ptr(),
        d.C, s.Hi, s.Wi, d.K, s.G, ctypes.byref(d.g), relu, ARITH[d.arith], stream())
    torch.cuda.synchronize()
    return st


def check_values(d, B, px, bias, relu, what):
    """The listed pixels within the arithmetic's bound, per element; every other element of the output and both guard
    planes still FILL.  Prints the figures before it asserts."""
    K, HW = d.K, d.HW
    px_t = dev(np.asarray(px, dtype=np.int64))
    out = B['out'].view(K, HW)
    want, mag = d.ref[:, px_t], d.mag[:, px_t]
    if bias:
        want, mag = want + d.b64, mag + d.b64.abs()
    if relu:
        want = want.clamp(min=0)
    err = (out[:, px_t].double() - want).abs()
    bound = bound_of(d.arith, d.Ckkg, want, mag)
    if err.numel():
        nz = mag > 0
        rel = float((err[nz] / mag[nz]).max()) if bool(nz.any()) else 0.0
        WORST[d.arith] = max(WORST.get(d.arith, 0.0), rel)
        line = "%s: max |err| %.3g, max err / mag %.3g = %.2f * 2^-24 (worst so far for %s: %.2f * 2^-24)" % (
            what, float(err.max()), rel, rel * 2.0 ** 24, d.arith, WORST[d.arith] * 2.0 ** 24)
        print(line)
        assert bool((err <= bound).all()), line + "; worst err / bound %.3g" % float((err / (bound + 1e-300)).max())
        if d.arith == "F16":
            tol = half_tol(np.array([float(want.abs().max())]))
            assert float(err.max()) <= tol, line + "; 2 fp16 ulp of the largest output: %.3g" % tol
    rest = B['buf'].clone()
    rest[HW:(K + 1) * HW].view(K, HW)[:, px_t] = FILL
    assert bool((rest == FILL).all()), "%s: a value outside the list changed" % what


def run_mask_frames(lib, d, B, frames, bias):
    """Consecutive frames on one frame-mask buffer, the mask written as the detection would (into the mask the parity
    selects, which the protocol keeps clean): list and order, count, mask copy, the other mask, parity and arrival
    counter after each launch, then the values."""
    M = Masks(lib, B['bits'], d.Ho, d.Wo)
    for name, px, relu in frames:
        what = "%s-%s %s bias=%d relu=%d" % (d.name, d.arith, name, bias, relu)
        par = M.ctl()[0]
        assert par in (0, 1) and int(M.mask(par).ne(0).sum()) == 0, what
        listed = np.zeros(d.HW, dtype=bool)
        listed[px] = True
        packed = M.packed(listed)
        M.mask(par).copy_(packed)
        B['buf'].fill_(FILL)
        B['idx'].fill_(-1)
        B['count'].fill_(-1)
        assert launch(lib, d, B, bias=bias, relu=relu) == 0, what
        n = len(px)
        assert B['count'].tolist() == [n], what
        assert torch.equal(B['idx'][:n], dev(np.asarray(px, dtype=np.int32))), what + ": the list"
        assert bool((B['idx'][n:] == -1).all()), what + ": the list past the count"
        assert torch.equal(M.mask(par), packed), what + ": the frame's mask"
        assert torch.equal(M.copy(), packed), what + ": the mask copy"
        assert int(M.mask(par ^ 1).ne(0).sum()) == 0, what + ": the other mask"
        assert M.ctl() == [par ^ 1, 0], what + ": parity / arrival counter"
        check_values(d, B, px, bias, relu, what)      # (this frame's mask is zeroed by the NEXT launch: checked there)


# ---------------------------------------------------------------------------------------------------------------------
# a. the contraction through the raw C ABI: one test per table case
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c.id for c in CASES])
def test_contraction_cases(lib, cid):
    c = CASE_BY_ID[cid]
    f = gc.case_form(c)
    assert gc.cell_of(c, f) == gc.claimed_cell(c), (cid, gc.cell_of(c, f), f)      # the form the table claims
    print("cell %s: %s" % (gc.cell_of(c, f), {k: f[k] for k in ("ROWS", "KgP", "rowTiles", "stages", "tilesN", "items",
                                                                  "chunk")}))
    d = _data(lib, c.shape, c.arith)
    N = len(d.px)
    B = d.buffers(lib)
    if c.source == "mask":
        allpx = np.arange(d.HW, dtype=np.int32)
        none = np.zeros(0, dtype=np.int32)
        # consecutive frames: the case's pixels, nothing changed (writes nothing, count 0, parity flipped), everything
        run_mask_frames(lib, d, B, [("frame 1", d.px, 0), ("nothing changed", none, 1), ("everything changed", allpx, 1)],
                        True)
        run_mask_frames(lib, d, B, [("frame 4", d.px, 1)], False)
        return
    lst = dev(d.px)
    count = dev(np.array([N], dtype=np.int32))
    for bias, relu, cnt in ((True, 0, None), (True, 1, count), (False, 0, count), (False, 1, None)):
        what = "%s bias=%d relu=%d %s count" % (cid, bias, relu, "host" if cnt is None else "device")
        B['buf'].fill_(FILL)
        assert launch(lib, d, B, lst, N, cnt, bias=bias, relu=relu) == 0, what
        check_values(d, B, d.px, bias, relu, what)


def test_unreachable_ring_is_never_listed_by_the_frame(lib, oracle):
    """cbinfer_cbgroupconv2d_forward on the shape with a ring no tap reaches, from a +inf state: the frame lists exactly
    the reachable pixels, the ring keeps what the caller put there."""
    d = _data(lib, "unreachable", "F32S")
    s = d.s
    B = d.buffers(lib)
    state = torch.full((1, d.C, s.Hi, s.Wi), float('inf'), dtype=torch.float32, device="cuda")
    lib.check(lib.C.cbinfer_cbgroupconv2d_forward(
        d.x.data_ptr(), state.data_ptr(), B['out'].data_ptr(), B['bits'].data_ptr(), B['idx'].data_ptr(),
        B['count'].data_ptr(), d.wp.data_ptr(), d.bias.data_ptr(), d.C, s.Hi, s.Wi, d.K, s.G, ctypes.byref(d.g), TH, 1, 1,
        1, ARITH["F32S"], stream()))
    torch.cuda.synchronize()
    n = int(B['count'].item())
    assert 0 < n == len(d.px) < d.HW and np.array_equal(B['idx'][:n].cpu().numpy(), d.px)
    assert torch.equal(state, d.x)
    check_values(d, B, d.px, True, 1, "unreachable, whole frame")


# ---------------------------------------------------------------------------------------------------------------------
# b. list mode at the C ABI: the device count, entries outside the map
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", gc.DEVICE_COUNT_IDS)
def test_list_device_count_below_the_host_count(lib, cid):
    """The kernel takes min(device count, numChanges) entries: the pixels behind the device count keep their bits;
    a device count beyond numChanges does not reach past it; a negative one lists nothing."""
    c = CASE_BY_ID[cid]
    d = _data(lib, c.shape, c.arith)
    N = len(d.px)
    B = d.buffers(lib)
    lst = dev(d.px)
    for n_dev, n_host in ((1, N), (N - 1, N), (N + 1000, N - 1), (-5, N)):
        what = "%s device count %d, host count %d" % (cid, n_dev, n_host)
        B['buf'].fill_(FILL)
        count = dev(np.array([n_dev], dtype=np.int32))
        assert launch(lib, d, B, lst, n_host, count, relu=1) == 0, what
        check_values(d, B, d.px[:max(0, min(n_dev, n_host))], True, 1, what)


@pytest.mark.parametrize("cid", gc.OUT_OF_MAP_IDS)
def test_list_entries_outside_the_map_are_dropped(lib, cid):
    """Entries < 0 and >= Ho Wo, shuffled among the case's pixels: nothing is written through them -- neither into the
    output nor into the plane in front of it or behind it --, the others are computed as ever."""
    c = CASE_BY_ID[cid]
    d = _data(lib, c.shape, c.arith)
    N, HW = len(d.px), d.HW
    rng = np.random.default_rng(9)
    low = np.concatenate([[-1, -HW, -HW - 1, -2 ** 31], -rng.integers(1, 3 * HW, 16)])
    high = np.concatenate([[HW, HW + 1, 2 * HW - 1, 2 ** 31 - 1], HW + rng.integers(0, 3 * HW, 16)])
    full = np.concatenate([d.px, low, high]).astype(np.int32)
    full = full[rng.permutation(len(full))]
    assert len(full) == N + 40 <= HW
    B = d.buffers(lib)
    what = cid + " with entries outside the map"
    assert launch(lib, d, B, dev(full), len(full)) == 0
    check_values(d, B, d.px, True, 0, what)


# ---------------------------------------------------------------------------------------------------------------------
# c. a pixel's bits depend on the input, the weights and the arithmetic only
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", gc.INDEPENDENCE_IDS)
def test_a_pixel_does_not_depend_on_the_list_or_the_form(lib, cid):
    """The same pixel listed alone, in a full tile, in a list whose order puts it into another tile slot (and another
    tile), and in mask mode: its K values are the same bits in all four."""
    c = CASE_BY_ID[cid]
    d = _data(lib, c.shape, c.arith)
    B = d.buffers(lib)
    HW = d.HW
    rng = np.random.default_rng(31)
    target = int(d.px[len(d.px) // 2])
    others = np.array([q for q in rng.permutation(HW) if q != target][:99], dtype=np.int32)
    settings = {
        "alone": np.array([target], dtype=np.int32),
        "full tile, slot 0": np.concatenate([[target], others[:63]]).astype(np.int32),
        "slot 37 of the second tile": np.concatenate([others[:64 + 37], [target], others[64 + 37:]]).astype(np.int32),
    }
    got = {}
    for name, lst in settings.items():
        B['buf'].fill_(FILL)
        assert launch(lib, d, B, dev(lst), len(lst), relu=0) == 0, name
        got[name] = raw(B['out'].view(d.K, HW)[:, target].clone())
        check_values(d, B, np.sort(lst), True, 0, "%s %s" % (cid, name))
    M = Masks(lib, B['bits'], d.Ho, d.Wo)
    listed = np.zeros(HW, dtype=bool)
    listed[np.concatenate([[target], others[:80]])] = True
    M.mask(M.ctl()[0]).copy_(M.packed(listed))
    B['buf'].fill_(FILL)
    assert launch(lib, d, B) == 0
    got["mask mode"] = raw(B['out'].view(d.K, HW)[:, target].clone())
    first = got.pop("alone")
    for name, bits in got.items():
        assert torch.equal(bits, first), (cid, name)


# ---------------------------------------------------------------------------------------------------------------------
# d. the module against a teacher-forced twin
# ---------------------------------------------------------------------------------------------------------------------
class GroupTwin(Twin):
    """tests/test_gpu_geom.py's twin -- the oracle's detection over all channels, the tap-loop footprint -- with the
    float64 grouped convolution for the values; also the magnitude the bounds scale with."""

    def __init__(self, oracle, weight, bias, geom, th, feedback, relu, groups):
        super(GroupTwin, self).__init__(oracle, weight, bias, geom, th, feedback, relu)
        self.groups = groups

    def step(self, x):
        if self.state is None:
            self.state = np.full_like(x, np.inf)
        det = self.oracle.changeDetection if x.dtype == np.float32 else self.oracle.changeDetection_half
        changed = det(np.ascontiguousarray(x), self.state, (1, 1), self.th, updateInputState=self.feedback)
        if not self.feedback:
            self.state[...] = x
        (kH, kW), s, p, d = self.geom
        Hi, Wi = x.shape[-2:]
        Ho, Wo = out_size(Hi, kH, s[0], p[0], d[0]), out_size(Wi, kW, s[1], p[1], d[1])
        listed = footprint(np.asarray(changed).reshape(Hi, Wi) != 0, self.geom, Ho, Wo)
        s64 = torch.from_numpy(self.state.astype(np.float64))
        kw = dict(stride=s, padding=p, dilation=d, groups=self.groups)
        ref = F.conv2d(s64, self.w, self.b, **kw)[0]
        self.mag = F.conv2d(s64.abs(), self.w.abs(), self.b.abs() if self.b is not None else None, **kw)[0].numpy()
        if self.relu:
            ref = torch.relu(ref)
        return np.flatnonzero(listed.reshape(-1)).astype(np.int32), listed, ref.numpy()


MODULE_GEOMS = ["3x3s1p1", "3x3s2p1", "3x3d2p2", "1x1"]
MODES = {"copyInput": (False, True), "feedbackLoop": (True, False), "neither": (False, False)}


def module_geom(name):
    return ((3, 3), (1, 1), (1, 1), (1, 1)) if name == "3x3s1p1" else \
        ((1, 1), (1, 1), (0, 0), (1, 1)) if name == "1x1" else GEOMS[name]


def make_grouped(geom, C, K, G, bias, dtype, seed=3):
    torch.manual_seed(seed)
    k, s, p, d = geom
    return nn.Conv2d(C, K, k, stride=s, padding=p, dilation=d, groups=G, bias=bias).cuda().to(dtype)


def list_of(m):
    """The frame's ascending list as the module's kernel wrote it."""
    work = m.__dict__['_work']
    return work['idx'][:int(work['count'].item())].cpu().numpy()


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("dtype", ["F32", "F16"])
@pytest.mark.parametrize("name", MODULE_GEOMS)
def test_module_tracks_the_twin(pkg, lib, oracle, name, dtype, mode):
    """C=16, K=24, G=4 on a 24x70 map over 6 frames: the list and prevInput equal the twin's bit for bit, listed outputs
    are within the arithmetic's bound of the float64 grouped convolution of the twin's state, unlisted ones keep their
    bits; the mask handed on is the list's."""
    geom = module_geom(name)
    Cin, K, G, Hi, Wi = 16, 24, 4, 24, 70
    arith = "F16" if dtype == "F16" else "F32S"
    feedback, copy_input = MODES[mode]
    conv = make_grouped(geom, Cin, K, G, name != "3x3s2p1", tdtype(dtype))
    m = pkg.CBGroupedConv2d(conv, TH)
    m.feedbackLoop, m.copyInput, m.withReLU, m.propChangeIndexes = feedback, copy_input, name != "3x3d2p2", True
    twin = GroupTwin(oracle, conv.weight, conv.bias, geom, TH, feedback, m.withReLU, G)
    Ckkg = Cin // G * geom[0][0] * geom[0][1]
    rng = np.random.default_rng(50 + MODULE_GEOMS.index(name))
    prev = None
    with torch.no_grad():
        for t, x in enumerate(frames_for(rng, Cin, Hi, Wi, 6, npdtype(dtype))):
            tag = (name, dtype, mode, t)
            tup = m(dev(x))
            assert tup[0] == 'changeIndexes'
            y = tup[1]
            idx, listed, ref = twin.step(x)
            Ho, Wo = listed.shape
            assert tuple(y.shape) == (1, K, Ho, Wo), tag
            assert np.array_equal(list_of(m), idx), tag
            assert t > 0 or idx.size == Ho * Wo, tag
            assert t == 0 or idx.size < Ho * Wo, tag
            assert tup[2].size == (Ho, Wo) and np.array_equal(tup[2].tensor().cpu().numpy(), idx), tag
            assert np.array_equal(bits_of(m.prevInput.cpu().numpy()), bits_of(twin.state)), tag
            out = y.cpu().numpy()[0]
            err = np.abs(out.astype(np.float64) - ref)
            bound = bound_of(arith, Ckkg, ref, twin.mag)
            assert np.all(err[:, listed] <= bound[:, listed]), tag + (float((err / bound)[:, listed].max()),)
            if arith == "F16" and idx.size:
                assert err[:, listed].max() <= half_tol(ref), tag
            if prev is not None:
                assert np.array_equal(bits_of(out)[:, ~listed], bits_of(prev)[:, ~listed]), tag
            prev = out.copy()


@pytest.mark.parametrize("dtype", ["F32", "F16"])
def test_threshold_zero_clear_memory_and_a_new_resolution(pkg, lib, dtype):
    """Threshold 0: after every frame the state is the dense layer of the frame, within the bound, at every pixel -- also
    after clearMemory and at another resolution in the middle of the sequence.  A ('changeIndexes', tensor, indexes)
    input is taken for its tensor."""
    geom = GEOMS["3x3s2p1"]
    Cin, K, G = 12, 20, 2
    arith = "F16" if dtype == "F16" else "F32S"
    conv = make_grouped(geom, Cin, K, G, True, tdtype(dtype), seed=8)
    m = pkg.CBGroupedConv2d(conv, 0.0)
    m.withReLU = True
    w64, b64 = conv.weight.detach().cpu().double(), conv.bias.detach().cpu().double()
    kw = dict(stride=geom[1], padding=geom[2], dilation=geom[3], groups=G)
    rng = np.random.default_rng(77)
    sizes = [(13, 70), (13, 70), (13, 70), (9, 131), (9, 131), (13, 70)]
    x = None
    with torch.no_grad():
        for t, (Hi, Wi) in enumerate(sizes):
            if x is None or x.shape[-2:] != (Hi, Wi):
                x = (rng.random((1, Cin, Hi, Wi)) * 0.9).astype(npdtype(dtype))
            else:
                x = x.copy()
                x[:, :, 2:6, 5:12] = (rng.random((1, Cin, 4, 7)) * 0.9).astype(npdtype(dtype))
            if t == 2:
                pkg.clearMemory(m)
                assert m.prevOutput.numel() == 0 and m.__dict__['_work'] is None
            inp = dev(x) if t % 2 else ('changeIndexes', dev(x), torch.zeros(3, dtype=torch.int32, device="cuda"))
            y = m(inp)
            n = list_of(m).size
            Ho, Wo = y.shape[-2:]
            assert n == Ho * Wo if t in (0, 2, 3, 5) else 0 < n < Ho * Wo, (dtype, t, n)
            x64 = torch.from_numpy(x.astype(np.float64))
            ref = torch.relu(F.conv2d(x64, w64, b64, **kw))[0].numpy()
            mag = F.conv2d(x64.abs(), w64.abs(), b64.abs(), **kw)[0].numpy()
            err = np.abs(y.cpu().numpy()[0].astype(np.float64) - ref)
            assert np.all(err <= bound_of(arith, Cin // G * 9, ref, mag)), (dtype, t, err.max())


def test_exact_f32_switches_the_arithmetic(pkg, lib, oracle):
    """exactF32: the prepared weights and the launch are CB_F32's, and the layer is within the f32 chain's bound."""
    geom = GEOMS["3x3d2p2"]
    Cin, K, G, Hi, Wi = 16, 24, 4, 11, 70
    conv = make_grouped(geom, Cin, K, G, True, torch.float32)
    m = pkg.CBGroupedConv2d(conv, TH)
    twin = GroupTwin(oracle, conv.weight, conv.bias, geom, TH, False, False, G)
    spy = Spy(lib.C)
    from cbinfer_amd import groupconv
    rng = np.random.default_rng(12)
    real = groupconv.C
    try:
        groupconv.C = spy
        with torch.no_grad():
            for t, x in enumerate(frames_for(rng, Cin, Hi, Wi, 3, np.float32)):
                m.exactF32 = t != 1
                want = lib.CB_F32 if m.exactF32 else lib.CB_F32S
                xd = dev(x)
                assert m._arith(xd) == want
                y = m(xd)
                assert m.__dict__['_wprep'][0][-1] == want
                idx, listed, ref = twin.step(x)
                assert np.array_equal(list_of(m), idx), t
                err = np.abs(y.cpu().numpy()[0].astype(np.float64) - ref)
                factor = Cin // G * 9 if m.exactF32 else 64
                assert np.all(err[:, listed] <= factor * 2.0 ** -24 * twin.mag[:, listed]), (t, err[:, listed].max())
    finally:
        groupconv.C = real
    assert spy.calls == {'cbinfer_groupconv_prep_weights': 3, 'cbinfer_cbgroupconv2d_forward': 3}, spy.calls


class ArgSpy(object):
    """Notes the launching library calls a module makes, with their arguments."""

    def __init__(self, real):
        self.__dict__['real'], self.__dict__['log'] = real, []

    def __getattr__(self, name):
        fn = getattr(self.real, name)
        if not getattr(fn, 'launcher', False):
            return fn

        def noted(*a):
            self.log.append((name, a))
            return fn(*a)
        return noted


def test_hand_wired_consumers_take_the_changes(pkg, lib):
    """propChangeIndexes: a 1x1 CBConv2d and a CBAdd2d wired by hand take the layer's MaskChangeIndexes on the OUTPUT map
    -- from the library calls they make, neither runs a detection of its own nor makes a list (the grouped contraction
    left it) -- and equal their dense selves."""
    from cbinfer_amd import conv2d, residual
    from cbinfer_amd.conv2d_cg import MaskChangeIndexes
    geom = GEOMS["3x3s2p1"]
    Cin, K, G, Hi, Wi = 8, 16, 4, 20, 70
    conv = make_grouped(geom, Cin, K, G, True, torch.float32)
    m = pkg.CBGroupedConv2d(conv, TH)
    m.propChangeIndexes = True
    torch.manual_seed(5)
    head = pkg.CBConv2d(nn.Conv2d(K, 8, 1).cuda(), 123.0)
    head.exactF32 = True
    add = pkg.CBAdd2d()
    rng = np.random.default_rng(3)
    spies = {mod: ArgSpy(lib.C) for mod in (conv2d, residual)}
    real = {mod: mod.C for mod in spies}
    w64, b64 = head.weight.detach().cpu().double(), head.bias.detach().cpu().double()
    frames = frames_for(rng, Cin, Hi, Wi, 4, np.float32)
    Ho, Wo = out_size(Hi, 3, 2, 1, 1), out_size(Wi, 3, 2, 1, 1)
    zero = torch.zeros(1, K, Ho, Wo, device="cuda")
    none = torch.zeros(0, dtype=torch.int32, device="cuda")
    counts = []
    try:
        for mod, spy in spies.items():
            mod.C = spy
        with torch.no_grad():
            for t, x in enumerate(frames):
                tup = m(dev(x))
                assert isinstance(tup[2], MaskChangeIndexes) and tup[2].size == (Ho, Wo) and tup[2]._made
                counts.append(list_of(m).size)
                y1 = head(tup)
                y2 = add(tup, ('changeIndexes', zero, none))
                torch.cuda.synchronize()
                state = m.prevOutput
                ref = F.conv2d(state.cpu().double(), w64, b64)
                mag = F.conv2d(state.cpu().double().abs(), w64.abs(), b64.abs())
                assert bool(((y1.cpu().double() - ref).abs() <= (K + 1) * 2.0 ** -24 * mag).all()), t
                assert torch.equal(y2, state), t
    finally:
        for mod in spies:
            mod.C = real[mod]
    assert counts[0] == Ho * Wo and all(n < Ho * Wo for n in counts[1:]), counts
    for mod, spy in spies.items():
        print(mod.__name__, [n for n, _ in spy.log])
        for name, args in spy.log:
            assert not any(word in name for word in ("detect", "compact", "indexes_extr")), name
            if name == 'cbinfer_cbconv2d_forward':      # (frame masks: none; haveIndexes: 1)
                assert args[3] is None and args[19] == 1, args
    assert [n for n, _ in spies[residual].log] == ['cbinfer_cbadd_forward'] * len(frames)
    # the sum took a list or a mask from both operands on every frame but the one that allocated its state
    for _, a in spies[residual].log[1:]:
        assert (a[3] is not None) != (a[4] is not None) and a[8] is not None, a
    assert [n for n, _ in spies[conv2d].log if 'prep' not in n] == ['cbinfer_cbconv2d_forward'] * len(frames)


# ---------------------------------------------------------------------------------------------------------------------
# e. a ResNeXt-type block: 1x1 + ReLU -> grouped 3x3 + ReLU -> 1x1, a 1x1 shortcut, the sum
# ---------------------------------------------------------------------------------------------------------------------
def make_block(pkg, stride, threshold, cloneOutput):
    torch.manual_seed(70 + stride)
    body = nn.Sequential(nn.Conv2d(16, 32, 1), nn.ReLU(), nn.Conv2d(32, 32, 3, stride, 1, groups=8), nn.ReLU(),
                         nn.Conv2d(32, 64, 1)).eval().cuda()
    shortcut = nn.Sequential(nn.Conv2d(16, 64, 1, stride)).eval().cuda()
    cb = pkg.convert(body, threshold=threshold, generalGeometry=True, grouped=True)
    sc = pkg.convert(shortcut, threshold=threshold, generalGeometry=True, grouped=True)
    reduce_, grouped, expand = list(cb)
    assert type(grouped) is pkg.CBGroupedConv2d and grouped.withReLU and reduce_.withReLU
    net = nn.Sequential(pkg.CBResidual(cb, sc, relu=True))
    assert pkg.linkGrouped(net) is net
    assert grouped.propChangeIndexes and expand.propChangeIndexes and sc[0].propChangeIndexes
    for mod in (reduce_, grouped, expand, sc[0], net[0].add):
        mod.cloneOutput = cloneOutput
    reduce_.exactF32 = expand.exactF32 = sc[0].exactF32 = True
    # (module, float64 ReLU?, bound factor: the f32 chain's Ckk + 1 with exactF32, 64 for the bf16 triples)
    layers = [(reduce_, True, 16 + 1), (grouped, True, 64), (expand, False, 32 + 1)]
    return net, layers, sc[0]


def dense_block(x, layers, sc):
    """The float64 dense block and the summed bound of its change-based twin: per layer the error it inherits, |w| * E,
    plus its own factor * 2^-24 * mag with mag taken on |input| + E; the sum adds both operands' errors and one
    rounding."""
    def conv(m, a, w, b):
        return F.conv2d(a, w, b, stride=tuple(m.stride), padding=tuple(m.padding), dilation=tuple(m.dilation),
                        groups=m.groups)
    x = x.detach().cpu().double()

    def run(chain):
        a, E = x, torch.zeros_like(x)
        for m, relu, factor in chain:
            w, b = m.weight.detach().cpu().double(), m.bias.detach().cpu().double()
            ref = conv(m, a, w, b)
            E = conv(m, E, w.abs(), None) + factor * 2.0 ** -24 * conv(m, a.abs() + E, w.abs(), b.abs())
            a = torch.relu(ref) if relu else ref
        return a, E
    a, Ea = run(layers)
    b, Eb = run([(sc, False, 16 + 1)])
    ref = torch.relu(a + b)
    return ref, Ea + Eb + 2.0 ** -24 * ((a + b).abs() + Ea + Eb)


@pytest.mark.parametrize("stride", [1, 2])
def test_resnext_block_against_float64(pkg, lib, stride):
    """Converted with generalGeometry=True, grouped=True, linked, thresholds 0: every pixel of every frame of a 20x70 map
    within the summed bound of the float64 dense block."""
    net, layers, sc = make_block(pkg, stride, 0.0, True)
    rng = np.random.default_rng(5)
    with torch.no_grad():
        for t, x in enumerate(frames_for(rng, 16, 20, 70, 5, np.float32)):
            y = net(dev(x))
            torch.cuda.synchronize()
            ref, E = dense_block(torch.from_numpy(x), layers, sc)
            err = (y.cpu().double() - ref).abs()
            print("stride %d frame %d: max err / bound %.3g" % (stride, t, float((err / E).max())))
            assert tuple(y.shape) == tuple(ref.shape) and bool((err <= E).all()), (stride, t, float((err / E).max()))


def test_resnext_block_lists_fewer_pixels_on_steady_frames(pkg, lib):
    """At the bench's threshold the grouped layer recomputes fewer than all pixels once the sequence is steady."""
    th = TH      # (0.05: the default of bench.py's --threshold)
    net, layers, _ = make_block(pkg, 1, th, True)
    grouped = layers[1][0]
    rng = np.random.default_rng(6)
    counts = []
    with torch.no_grad():
        for x in frames_for(rng, 16, 20, 70, 5, np.float32, th=th):
            net(dev(x))
            counts.append(list_of(grouped).size)
    print("threshold %g: listed pixels per frame %s of %d" % (th, counts, 20 * 70))
    assert counts[0] == 20 * 70 and all(0 < n < 20 * 70 for n in counts[1:]), counts


def test_resnext_block_records_as_a_launch_program(pkg, lib):
    """With cloneOutput=False the block is library calls only: FrameProgram records it, its calls hold the grouped frame
    once; three replayed frames equal the eager network in outputs and states bit for bit."""
    net, _, _ = make_block(pkg, 1, TH, False)
    rng = np.random.default_rng(6)
    frames = [dev(f) for f in frames_for(rng, 16, 20, 70, 7, np.float32)]
    with torch.no_grad():
        for f in frames[:4]:
            net(f)
        eager = copy.deepcopy(net)
        prog = pkg.FrameProgram(net)
        for t, f in enumerate(frames[4:]):
            yp, ye = prog(f), eager(f)
            assert torch.equal(raw(yp), raw(ye)), t
            for ta, tb in zip(pkg.getStateTensors(net), pkg.getStateTensors(eager)):
                assert torch.equal(ta, tb), t
        raws = [fn for fn, _ in prog.calls]
        assert raws.count(lib.C.cbinfer_cbgroupconv2d_forward.raw) == 1
        assert lib.C.cbinfer_cbadd_forward.raw in raws
        assert len(pkg.getStateTensors(net)) == 2 * 4 + 1      # three convs of the body, the shortcut's, the sum


def test_worst_figures_are_reported():
    """The worst err / mag of each arithmetic over the tests above (DESIGN 5.18 records them): measurements, not bars."""
    for arith, rel in sorted(WORST.items()):
        print("worst err / mag, %s: %.3g = %.2f * 2^-24" % (arith, rel, rel * 2.0 ** 24))
