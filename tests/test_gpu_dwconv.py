"""-m gpu: the change-based depthwise convolution (cb_dwconv.hip) through the raw C ABI --
cbinfer_dwconv_changed in both of its forms, one case per shape of tests/dwconv_cases.py and dtype -- and through
CBDepthwiseConv2d: its own detection (cbinfer_cbdwconv2d_forward), propagated changes
(cbinfer_cbdwconv2d_forward_propagated), a separable chain and a MobileNetV2-type block recorded as a launch program.

References (nothing expected comes from the code under test): the values are a float64 CPU F.conv2d(..., groups=C) of
the map the stencil reads (never the device's convolution: DESIGN 5.10); the change rule is the pinned oracle's
changeDetection / changeDetection_half with a 1x1 filter, the footprint test_gpu_geom.footprint.

Bounds, per element, with mag = sum|w||x| + |bias| in float64 and n = kH kW + 1, the depth of the f32 FMA chain:
  F32  |err| <= n * 2^-24 * mag
  F16  |err| <= 2^-11 |ref| + n * 2^-23 * mag + 2^-24
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

import dwconv_cases as dc
from dwconv_cases import ARITH, CASE_BY_ID, CASES, GEOMS
from test_gpu_geom import footprint, frames_for
from test_gpu_geomconv import Masks
from test_gpu_listconv import pack_mask
from test_host_dwconv import cgeom, conv64
from optest import bits_of, dev, gpu_lib as lib, npdtype, pkg, raw, stream, tdtype      # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

FILL = 77.0
TH = 0.05
WORST = {}       # dtype -> worst err / mag seen (printed; a measurement, not a bar)


def bound_of(dtype, n, want, mag):
    if dtype == "F32":
        return n * 2.0 ** -24 * mag
    return 2.0 ** -11 * abs(want) + n * 2.0 ** -23 * mag + 2.0 ** -24


def act64(v, act):
    """The activation on a float64 torch tensor; a NaN stays a NaN (clamp keeps it)."""
    if act == dc.ACT_RELU:
        return v.clamp(min=0)
    if act == dc.ACT_RELU6:
        return v.clamp(min=0, max=6)
    return v


def reach_of(geom, Hi, Wi):
    return dc.twin(np.zeros((1, Hi, Wi)), np.zeros((1, 1) + geom[0]), None, geom, 1)[2]


class Data(object):
    """A case's tensors on the device and its float64 reference at EVERY output pixel (without the bias)."""

    def __init__(self, lib, c, dtype):
        self.c, self.dtype = c, dtype
        k = c.geom[0]
        self.K, self.n = c.C * c.mult, k[0] * k[1] + 1
        rng = np.random.default_rng(zlib.crc32((c.id + dtype).encode()))
        t = npdtype(dtype)
        x = rng.standard_normal((1, c.C, c.Hi, c.Wi)) * np.exp(rng.uniform(-6, 3, (1, c.C, 1, 1)))
        w = rng.standard_normal((self.K, 1, k[0], k[1])) / np.sqrt(k[0] * k[1])
        b = rng.standard_normal(self.K)
        x, w, b = x.astype(t), w.astype(t), b.astype(t)
        xt, wt = torch.from_numpy(x), torch.from_numpy(w)
        ref, mag = conv64(xt, wt, None, c.geom, c.C)[0], conv64(xt.abs(), wt.abs(), None, c.geom, c.C)[0]
        assert tuple(ref.shape) == (self.K, c.Ho, c.Wo)
        self.HW = c.Ho * c.Wo
        self.ref, self.mag = ref.reshape(self.K, -1).cuda(), mag.reshape(self.K, -1).cuda()
        self.b64 = torch.from_numpy(b.astype(np.float64)).cuda()[:, None]
        self.x, self.w, self.bias = dev(x), dev(w), dev(b)
        self.g = cgeom(lib, c.geom)
        self.reach = reach_of(c.geom, c.Hi, c.Wi).reshape(-1)
        self.wpr = (c.Wo + 63) // 64

    def buffers(self, lib):
        c = self.c
        words = lib.C.cbinfer_mask_words(c.Ho, c.Wo)
        B = dict(fm=torch.zeros(lib.C.cbinfer_frame_mask_bytes(c.Ho, c.Wo) // 8, dtype=torch.int64, device="cuda"),
                 bits=torch.zeros(words, dtype=torch.int64, device="cuda"),
                 copy=torch.full((words,), 0x5a5a, dtype=torch.int64, device="cuda"))
        B['buf'] = torch.full(((self.K + 2) * self.HW,), FILL, dtype=tdtype(self.dtype), device="cuda")
        B['out'] = B['buf'][self.HW:(self.K + 1) * self.HW]
        return B

    def patterns(self):
        """(name, listed [Ho, Wo]) of the mask patterns of the issue; those a map is too small for are left out."""
        c = self.c
        rng = np.random.default_rng(zlib.crc32(c.id.encode()) + 5)
        Z = np.zeros((c.Ho, c.Wo), dtype=bool)
        corners = Z.copy()
        corners[[0, 0, -1, -1], [0, -1, 0, -1]] = True
        out = [("random", rng.random(Z.shape) < 0.1), ("empty", Z), ("full", ~Z), ("corners", corners)]
        if c.Wo > 64:
            seam = Z.copy()
            seam[c.Ho // 2, 63] = seam[c.Ho // 2, 64] = True
            out.append(("bit 63 and bit 0", seam))
        if c.Wo % 64:
            last = Z.copy()
            last[:, 64 * (self.wpr - 1):] = True
            out.append(("partial last word", last))
        return out


@functools.lru_cache(maxsize=None)
def _data(lib, cid, dtype):
    return Data(lib, CASE_BY_ID[cid], dtype)


def launch(lib, d, B, form, listed, bias=True, act=0, what=""):
    """One frame of cbinfer_dwconv_changed in the form "frame" (frame masks) or "bits" (bits / maskCopy), the mask
    written as a detection or a footprint launch would; the protocol's state is asserted before and after."""
    c = d.c
    packed = dev(pack_mask(np.asarray(listed, dtype=bool).reshape(c.Ho, c.Wo), d.wpr))
    bp = d.bias.data_ptr() if bias else None
    args = (c.C, c.mult, c.Hi, c.Wi, ctypes.byref(d.g), act, ARITH[d.dtype], stream())
    if form == "frame":
        M = Masks(lib, B['fm'], c.Ho, c.Wo)
        par = M.ctl()[0]
        assert par in (0, 1) and int(M.mask(par).ne(0).sum()) == 0, what
        M.mask(par).copy_(packed)
        st = lib.C.cbinfer_dwconv_changed(d.x.data_ptr(), d.w.data_ptr(), bp, B['out'].data_ptr(), B['fm'].data_ptr(),
                                          None, None, *args)
        torch.cuda.synchronize()
        assert st == 0, what
        assert torch.equal(M.mask(par), packed), what + ": the frame's mask"
        assert torch.equal(M.copy(), packed), what + ": the mask copy"
        assert int(M.mask(par ^ 1).ne(0).sum()) == 0, what + ": the other mask"
        assert M.ctl() == [par ^ 1, 0], what + ": parity / arrival counter"
    else:
        assert int(B['bits'].ne(0).sum()) == 0, what
        B['bits'].copy_(packed)
        st = lib.C.cbinfer_dwconv_changed(d.x.data_ptr(), d.w.data_ptr(), bp, B['out'].data_ptr(), None,
                                          B['bits'].data_ptr(), B['copy'].data_ptr(), *args)
        torch.cuda.synchronize()
        assert st == 0, what
        assert int(B['bits'].ne(0).sum()) == 0, what + ": the working mask"
        assert torch.equal(B['copy'], packed), what + ": the mask copy (bits of the row padding included)"


def check_values(d, B, listed, bias, act, what):
    """The listed pixels a tap reaches within the bound, per element; every other element of the output and both guard
    planes still FILL.  Prints the figures before it asserts."""
    K, HW = d.K, d.HW
    px = np.flatnonzero(np.asarray(listed).reshape(-1) & d.reach)
    px_t = dev(px.astype(np.int64))
    out = B['out'].view(K, HW)
    want, mag = d.ref[:, px_t], d.mag[:, px_t]
    if bias:
        want, mag = want + d.b64, mag + d.b64.abs()
    want = act64(want, act)
    err = (out[:, px_t].double() - want).abs()
    bound = bound_of(d.dtype, d.n, want, mag)
    if err.numel():
        nz = mag > 0
        rel = float((err[nz] / mag[nz]).max()) if bool(nz.any()) else 0.0
        WORST[d.dtype] = max(WORST.get(d.dtype, 0.0), rel)
        line = "%s: %d pixels, max |err| %.3g, max err / mag %.3g = %.2f * 2^-24 (worst so far for %s: %.2f * 2^-24)" % (
            what, len(px), float(err.max()), rel, rel * 2.0 ** 24, d.dtype, WORST[d.dtype] * 2.0 ** 24)
        print(line)
        assert bool((err <= bound).all()), line + "; worst err / bound %.3g" % float((err / (bound + 1e-300)).max())
    rest = B['buf'].clone()
    rest[HW:(K + 1) * HW].view(K, HW)[:, px_t] = FILL
    assert bool((rest == FILL).all()), "%s: a value outside the list (or a pixel no tap reaches) changed" % what


# ---------------------------------------------------------------------------------------------------------------------
# a. the stencil: every shape of the table, both dtypes, both forms
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["frame", "bits"])
@pytest.mark.parametrize("dtype", ["F32", "F16"])
@pytest.mark.parametrize("cid", [c.id for c in CASES])
def test_stencil_cases(lib, cid, dtype, form):
    """Consecutive frames on one set of mask buffers, one per mask pattern (at least four): the protocol's state after
    each launch, then the values.  Bias and activation alternate over the frames."""
    d = _data(lib, cid, dtype)
    B = d.buffers(lib)
    if d.c is dc.WALK:
        units, groups = dc.units_of(d.c)
        assert units > groups == 8 * torch.cuda.get_device_properties(0).multi_processor_count, (units, groups)
    pats = d.patterns()
    assert len(pats) >= 4
    for i, (name, listed) in enumerate(pats):
        bias, act = i % 3 != 1, i % 3
        what = "%s %s %s frame %d (%s) bias=%d act=%d" % (cid, dtype, form, i, name, bias, act)
        B['buf'].fill_(FILL)
        launch(lib, d, B, form, listed, bias, act, what)
        check_values(d, B, listed, bias, act, what)


@pytest.mark.parametrize("dtype", ["F32", "F16"])
@pytest.mark.parametrize("cid", [c.id for c in CASES])
def test_a_pixel_does_not_depend_on_the_list_or_the_form(lib, cid, dtype):
    """The values at the pixels of a sparse mask equal, bit for bit, the same pixels of a full-mask run and of the other
    form; two runs give the same bits."""
    d = _data(lib, cid, dtype)
    c = d.c
    sparse = d.patterns()[0][1]
    sel = dev(np.flatnonzero(sparse.reshape(-1) & d.reach).astype(np.int64))
    runs = {}
    for name, form, listed in (("full frame", "frame", np.ones_like(sparse)), ("sparse frame", "frame", sparse),
                               ("sparse bits", "bits", sparse), ("sparse bits again", "bits", sparse),
                               ("full bits", "bits", np.ones_like(sparse))):
        B = d.buffers(lib)
        launch(lib, d, B, form, listed, True, dc.ACT_RELU6, "%s %s %s" % (cid, dtype, name))
        runs[name] = raw(B['buf']).clone()
    at = lambda name: runs[name][d.HW:(d.K + 1) * d.HW].view(d.K, d.HW)[:, sel]
    assert sel.numel() > 0 or c.Ho * c.Wo < 20
    for name in ("sparse frame", "sparse bits", "full bits"):
        assert torch.equal(at("full frame"), at(name)), (cid, dtype, name)
    assert torch.equal(runs["sparse bits"], runs["sparse bits again"]) and torch.equal(runs["full frame"], runs["full bits"])
    assert torch.equal(runs["sparse frame"], runs["sparse bits"])


@pytest.mark.parametrize("form", ["frame", "bits"])
@pytest.mark.parametrize("dtype", ["F32", "F16"])
def test_activation_bias_nan_and_unreachable_pixels(lib, dtype, form):
    """act 0 / 1 / 2 on values straddling 0 and 6, with a NaN input, with and without bias, on the geometry with a ring
    of output pixels no tap reaches: listed with all the others, they are never written."""
    geom = GEOMS["3x3p3"]
    C, mult, Hi, Wi = 3, 2, 6, 66
    K, t = C * mult, npdtype(dtype)
    rng = np.random.default_rng(11)
    x = (rng.standard_normal((1, C, Hi, Wi)) * 6).astype(t)
    x[0, 1, 2, 5] = np.nan
    w = (rng.standard_normal((K, 1, 3, 3)) / 2).astype(t)
    b = rng.standard_normal(K).astype(t)
    Ho, Wo = Hi + 4, Wi + 4
    reach = reach_of(geom, Hi, Wi)
    assert reach.shape == (Ho, Wo) and 0 < reach.sum() < reach.size
    g = cgeom(lib, geom)
    xd, wd, bd = dev(x), dev(w), dev(b)
    words = lib.C.cbinfer_mask_words(Ho, Wo)
    full = dev(pack_mask(np.ones((Ho, Wo), dtype=bool), 2))
    fm = torch.zeros(lib.C.cbinfer_frame_mask_bytes(Ho, Wo) // 8, dtype=torch.int64, device="cuda")
    bits, cp = torch.zeros(words, dtype=torch.int64, device="cuda"), torch.zeros(words, dtype=torch.int64, device="cuda")
    for act in (dc.ACT_NONE, dc.ACT_RELU, dc.ACT_RELU6):
        for bias in (b, None):
            out = torch.full((K, Ho, Wo), FILL, dtype=tdtype(dtype), device="cuda")
            if form == "frame":
                par = Masks(lib, fm, Ho, Wo).ctl()[0]
                fm[par * words:(par + 1) * words].copy_(full)
            else:
                bits.copy_(full)
            st = lib.C.cbinfer_dwconv_changed(
                xd.data_ptr(), wd.data_ptr(), bd.data_ptr() if bias is not None else None, out.data_ptr(),
                fm.data_ptr() if form == "frame" else None, bits.data_ptr() if form == "bits" else None,
                cp.data_ptr() if form == "bits" else None, C, mult, Hi, Wi, ctypes.byref(g), act, ARITH[dtype], stream())
            torch.cuda.synchronize()
            assert st == 0
            want, mag, _ = dc.twin(x[0], w, bias, geom, mult, act)
            got = out.cpu().numpy().astype(np.float64)
            tag = (dtype, form, act, bias is not None)
            assert np.all(got[:, ~reach] == FILL), tag
            nan = np.isnan(want)
            assert nan.sum() == 9 * mult and np.array_equal(np.isnan(got), nan), tag      # (a NaN stays a NaN)
            ok = reach[None] & ~nan
            err = np.abs(got - want)[ok]
            assert np.all(err <= bound_of(dtype, 10, want[ok], mag[ok])), tag
            v = want[ok]
            assert (v < 0).any() == (act == dc.ACT_NONE) and (v > 6).any() == (act != dc.ACT_RELU6), tag
            if act:
                assert (got[ok] >= 0).all() and (got[ok] == 0).any(), tag
            if act == dc.ACT_RELU6:
                assert (got[ok] <= 6).all() and (got[ok] == 6).any(), tag


# ---------------------------------------------------------------------------------------------------------------------
# b. the module with its own detection
# ---------------------------------------------------------------------------------------------------------------------
class Twin(object):
    """The change rule (the pinned oracle, 1x1 filter), the exact footprint and the state the stencil reads."""

    def __init__(self, oracle, geom, th, feedback):
        self.oracle, self.geom, self.th, self.feedback = oracle, geom, th, feedback
        self.state = None

    def step(self, x):
        if self.state is None:
            self.state = np.full_like(x, np.inf)
        det = self.oracle.changeDetection if x.dtype == np.float32 else self.oracle.changeDetection_half
        changed = det(np.ascontiguousarray(x), self.state, (1, 1), self.th, updateInputState=self.feedback)
        if not self.feedback:
            self.state[...] = x
        Hi, Wi = x.shape[-2:]
        k, s, p, d = self.geom
        Ho, Wo = dc.out_size(Hi, k[0], s[0], p[0], d[0]), dc.out_size(Wi, k[1], s[1], p[1], d[1])
        return footprint(np.asarray(changed).reshape(Hi, Wi) != 0, self.geom, Ho, Wo)


def make_dw(geom, C, mult, bias, dtype):
    k, s, p, d = geom
    torch.manual_seed(C * 100 + mult)
    return nn.Conv2d(C, C * mult, k, s, p, d, groups=C, bias=bias).cuda().to(dtype)


def dense64(m, src, act):
    """(reference, mag) in float64 of the module's layer on the map `src` (a torch tensor [1, C, Hi, Wi])."""
    geom = (m.kernel_size, m.stride, m.padding, m.dilation)
    ref = act64(conv64(src, m.weight, m.bias, geom, m.in_channels), act)[0].numpy()
    mag = conv64(src.abs(), m.weight.abs(), m.bias.abs() if m.bias is not None else None, geom, m.in_channels)[0].numpy()
    return ref, mag


def check_frame(m, y, prev, listed, src, dtype, reach, tag, everywhere=False):
    """y [1, K, Ho, Wo] of the module against the float64 layer on `src`: the listed pixels (every reachable pixel with
    everywhere=True) within the bound, the unlisted ones bit for bit `prev`, the unreachable ones act(bias)."""
    act = m._act()
    ref, mag = dense64(m, src, act)
    out = y[0].cpu().numpy()
    k = m.kernel_size
    sel = reach if everywhere else (listed & reach)
    err = np.abs(out.astype(np.float64) - ref)
    bound = bound_of(dtype, k[0] * k[1] + 1, ref, mag)
    if sel.any():
        rel = float((err / (mag + 1e-300))[:, sel].max())
        WORST[dtype] = max(WORST.get(dtype, 0.0), rel)
        print("%s: %d pixels, max err / mag %.2f * 2^-24" % (tag, int(sel.sum()), rel * 2.0 ** 24))
    assert np.all(err[:, sel] <= bound[:, sel]), (tag, float((err / (bound + 1e-300))[:, sel].max()))
    if prev is not None:
        assert np.array_equal(bits_of(out)[:, ~listed], bits_of(prev)[:, ~listed]), tag
    else:
        assert listed[reach].all(), tag
    if (~reach).any():
        fill = np.zeros(out.shape[0]) if m.bias is None else dc.act_of(m.bias.detach().cpu().double().numpy(), act)
        assert np.array_equal(out[:, ~reach].astype(np.float64), np.broadcast_to(fill[:, None], out[:, ~reach].shape)), tag
    return out


MODULE_GEOMS = ["3x3s1p1", "3x3s2p1", "5x5s2p2", "3x3d2p2", "aniso", "3x3p3", "7x7s1p3", "2x2s2p0"]


@pytest.mark.parametrize("mode", ["copy", "feedback", "nocopy"])
@pytest.mark.parametrize("dtype", ["F32", "F16"])
def test_module_tracks_the_twin(pkg, lib, oracle, dtype, mode):
    """Six teacher-forced frames per geometry: the mask handed on and the list made from it are the twin's, prevInput is
    the twin's state bit for bit, listed pixels within the bound of the float64 layer on that state, unlisted ones keep
    their bits, unreachable ones hold act(bias).  Activation and bias alternate over the geometries."""
    from cbinfer_amd.conv2d_cg import MaskChangeIndexes
    for gi, name in enumerate(MODULE_GEOMS):
        geom = GEOMS[name]
        C, mult, Hi, Wi = (5, 3, 9, 40) if gi % 2 else (17, 2, 7, 70)
        m = pkg.CBDepthwiseConv2d(make_dw(geom, C, mult, gi % 3 != 2, tdtype(dtype)), TH)
        m.feedbackLoop, m.copyInput, m.propChangeIndexes = mode == "feedback", mode != "nocopy", True
        m.withReLU, m.reluCap = gi % 3 != 0, 6.0 if gi % 3 == 2 else None
        twin = Twin(oracle, geom, TH, mode == "feedback")
        rng = np.random.default_rng(200 + gi)
        reach = reach_of(geom, Hi, Wi)
        Ho, Wo = reach.shape
        prev, counts = None, []
        with torch.no_grad():
            for t, x in enumerate(frames_for(rng, C, Hi, Wi, 6, npdtype(dtype))):
                tag = (name, dtype, mode, t)
                kind, y, ix = m(dev(x))
                torch.cuda.synchronize()
                listed = twin.step(x)
                assert kind == 'changeIndexes' and isinstance(ix, MaskChangeIndexes) and ix.size == (Ho, Wo), tag
                assert tuple(y.shape) == (1, C * mult, Ho, Wo), tag
                assert np.array_equal(ix._mask.cpu().numpy(), pack_mask(listed, (Wo + 63) // 64)), tag
                assert np.array_equal(ix.tensor().cpu().numpy(), np.flatnonzero(listed.reshape(-1))), tag
                assert np.array_equal(bits_of(m.prevInput.cpu().numpy()), bits_of(twin.state)), tag
                prev = check_frame(m, y, prev, listed, torch.from_numpy(twin.state), dtype, reach, tag)
                counts.append(int(listed.sum()))
        assert counts[0] == int(reach.sum()) and 0 < min(counts[1:]) and max(counts[1:]) < counts[0], (name, counts)


@pytest.mark.parametrize("dtype", ["F32", "F16"])
def test_threshold_zero_clear_memory_and_a_new_resolution(pkg, lib, oracle, dtype):
    """With threshold 0 every input pixel that differs is listed, so EVERY pixel is within the bound of the float64
    layer on the frame itself; clearMemory makes the next frame dense again; a new resolution reallocates the state."""
    geom = GEOMS["5x5s1p2"]
    C, mult, Hi, Wi = 6, 2, 9, 70
    m = pkg.CBDepthwiseConv2d(make_dw(geom, C, mult, True, tdtype(dtype)), 0.0)
    m.propChangeIndexes, m.withReLU = True, True
    twin = Twin(oracle, geom, 0.0, False)
    rng = np.random.default_rng(9)
    base = (rng.random((1, C, Hi, Wi)) * 0.9).astype(npdtype(dtype))
    frames = []
    for t in range(6):      # one moved block per frame, nothing else differs
        base = base.copy()
        y0, x0 = int(rng.integers(0, Hi - 3)), int(rng.integers(0, Wi - 8))
        base[:, :, y0:y0 + 3, x0:x0 + 8] = rng.random((1, C, 3, 8)).astype(npdtype(dtype))
        frames.append(base)
    reach = reach_of(geom, Hi, Wi)
    prev, counts = None, []
    with torch.no_grad():
        for t, x in enumerate(frames):
            if t == 3:
                m.clearMemory()
                twin.state, prev = None, None
                assert m.prevOutput.numel() == 0 and m.prevInput.numel() == 0 and m.__dict__['_work'] is None
            _, y, ix = m(dev(x))
            torch.cuda.synchronize()
            listed = twin.step(x)
            assert np.array_equal(ix.tensor().cpu().numpy(), np.flatnonzero(listed.reshape(-1))), t
            prev = check_frame(m, y, prev, listed, torch.from_numpy(x), dtype, reach, ("th0", dtype, t), everywhere=True)
            counts.append(int(listed.sum()))
        assert counts[0] == counts[3] == reach.size and 0 < max(counts[1:3] + counts[4:]) < reach.size // 4, counts
        x2 = frames_for(rng, C, 5, 33, 1, npdtype(dtype))[0]
        _, y, ix = m(dev(x2))
        assert tuple(y.shape) == (1, C * mult, 5, 33) and ix.tensor().numel() == 5 * 33
        assert tuple(m.prevInput.shape) == (1, C, 5, 33)
        check_frame(m, y, None, np.ones((5, 33), dtype=bool), torch.from_numpy(x2), dtype, np.ones((5, 33), dtype=bool),
                    ("new resolution", dtype), everywhere=True)


# ---------------------------------------------------------------------------------------------------------------------
# c. propagated changes
# ---------------------------------------------------------------------------------------------------------------------
def block_frames(rng, C, H, W, n, t):
    """n frames [1, C, H, W] in dtype t; a frame differs from the one before in two moved blocks only.  -> (frames,
    changed maps [H, W]; the first all True)."""
    base = (rng.random((1, C, H, W)) * 0.9).astype(t)
    frames, changed = [], []
    for i in range(n):
        new = base.copy()
        if i:
            for _ in range(2):
                y0, x0 = int(rng.integers(0, H)), int(rng.integers(0, W))
                blk = new[:, :, y0:y0 + 4, x0:x0 + 7]
                blk[...] = (rng.random(blk.shape) * 0.9).astype(t)
        changed.append((new != base).any(axis=(0, 1)) if i else np.ones((H, W), dtype=bool))
        frames.append(new)
        base = new
    return frames, changed


class Spy(object):
    """Counts the library calls a module makes (the library object's attributes are read-only function pointers)."""

    def __init__(self, real):
        self.__dict__['real'], self.__dict__['calls'] = real, {}

    def __getattr__(self, name):
        fn = getattr(self.real, name)
        if not getattr(fn, 'launcher', False):
            return fn

        def counted(*a):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*a)
        return counted


@pytest.mark.parametrize("producer", ["list", "count", "mask", "add"])
@pytest.mark.parametrize("dtype", ["F32", "F16"])
def test_propagated_changes_from_a_list_and_from_a_mask(pkg, lib, dtype, producer):
    """The layer fed a producer's changes -- an exact int32 list, a ChangeIndexes with a device-side count, a
    MaskChangeIndexes (its mask, the list is never made) and a real mask-form producer, CBAdd2d: the mask handed on is
    the pool footprint of the changes (everything on the first frame), EVERY pixel is within the bound of the float64
    layer on the frame itself, unlisted pixels keep their bits, no input state is kept."""
    from cbinfer_amd.conv2d_cg import ChangeIndexes, MaskChangeIndexes
    for gi, name in enumerate(["3x3s1p1", "5x5s2p2", "4x4s2p1", "3x3s1p0", "1x1s2p0"]):
        geom = GEOMS[name]
        C, mult, Hi, Wi = (5, 3, 12, 70) if gi % 2 else (17, 1, 9, 131)
        m = pkg.CBDepthwiseConv2d(make_dw(geom, C, mult, gi != 1, tdtype(dtype)), 123.0)      # (the threshold is not used)
        m.propagatedChanges, m.propChangeIndexes, m.withReLU = True, True, gi % 2 == 0
        add = pkg.CBAdd2d()
        add.propChangeIndexes = True
        rng = np.random.default_rng(300 + gi)
        frames, changed = block_frames(rng, C, Hi, Wi, 5, npdtype(dtype))
        frames.append(frames[-1].copy())      # an idle frame
        changed.append(np.zeros((Hi, Wi), dtype=bool))
        reach = reach_of(geom, Hi, Wi)
        Ho, Wo = reach.shape
        zero = torch.zeros(1, C, Hi, Wi, dtype=tdtype(dtype), device="cuda")
        none = torch.zeros(0, dtype=torch.int32, device="cuda")
        prev = None
        with torch.no_grad():
            for t, (x, ch) in enumerate(zip(frames, changed)):
                tag = (name, dtype, producer, t)
                xd = dev(x)
                lst = np.flatnonzero(ch.reshape(-1)).astype(np.int32)
                if producer == "list":
                    inp = ('changeIndexes', xd, dev(lst))
                elif producer == "count":
                    buf = dev(np.concatenate([lst, np.full(7, 3, dtype=np.int32)]))      # (entries behind the count)
                    inp = ('changeIndexes', xd, ChangeIndexes(buf, dev(np.array([len(lst)], dtype=np.int32)), (Hi, Wi)))
                elif producer == "mask":
                    inp = ('changeIndexes', xd, MaskChangeIndexes(dev(pack_mask(ch, (Wi + 63) // 64)), (Hi, Wi), None, None))
                else:
                    inp = add(('changeIndexes', xd, dev(lst)), ('changeIndexes', zero, none))
                    assert isinstance(inp[2], MaskChangeIndexes) and torch.equal(raw(inp[1]), raw(xd)), tag
                kind, y, ix = m(inp)
                torch.cuda.synchronize()
                listed = footprint(ch, geom, Ho, Wo) if t else reach.copy()
                assert isinstance(ix, MaskChangeIndexes) and ix.size == (Ho, Wo), tag
                assert np.array_equal(ix._mask.cpu().numpy(), pack_mask(listed, (Wo + 63) // 64)), tag
                assert m.prevInput.numel() == 0 and int(m._work['bits'].ne(0).sum()) == 0, tag
                if producer in ("mask", "add"):
                    assert not inp[2]._made, tag
                prev = check_frame(m, y, prev, listed, torch.from_numpy(x), dtype, reach, tag, everywhere=True)
        # a bare tensor carries no change information: every pixel is listed
        with torch.no_grad():
            _, y, ix = m(dev(frames[2]))
        assert ix.tensor().numel() == Ho * Wo
        check_frame(m, y, None, reach | True, torch.from_numpy(frames[2]), dtype, reach, (name, "bare"), everywhere=True)


def test_propagated_refusals(pkg, lib):
    from cbinfer_amd.conv2d_cg import ChangeIndexes
    m = pkg.CBDepthwiseConv2d(make_dw(GEOMS["3x3s1p1"], 4, 1, True, torch.float32), 0.1)
    m.propagatedChanges = True
    x = torch.zeros(1, 4, 8, 10, device="cuda")
    idx, cnt = torch.zeros(80, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    with pytest.raises(lib.CBinferError, match="address a 9x10 map, this layer's input map is 8x10"):
        m(('changeIndexes', x, ChangeIndexes(idx, cnt, (9, 10))))
    with pytest.raises(lib.CBinferError, match="must be an int32 tensor or a ChangeIndexes"):
        m(('changeIndexes', x, [1, 2]))
    with pytest.raises(lib.CBinferError, match="contiguous int32 tensor"):
        m(('changeIndexes', x, idx.long()))
    for name in ("3x3d2p2", "3x3p3", "aniso"):
        m = pkg.CBDepthwiseConv2d(make_dw(GEOMS[name], 4, 1, True, torch.float32), 0.1)
        m.propagatedChanges = True
        with pytest.raises(lib.CBinferError, match="propagatedChanges needs dilation 1 and padding <= kernel_size / 2"):
            m(('changeIndexes', torch.zeros(1, 4, 12, 12, device="cuda"), idx))


def dense_chain(x, layers, dtype):
    """The float64 dense network and the composed bound of its change-based twin: per layer (module, activation, n) the
    error the layer inherits, |w| * E, plus its own, the bound of the dtype with mag taken on |input| + E."""
    a, E = x.detach().cpu().double(), None
    for m, act, n in layers:
        w, b = m.weight.detach().cpu().double(), m.bias.detach().cpu().double() if m.bias is not None else None
        kw = dict(stride=tuple(m.stride), padding=tuple(m.padding), dilation=tuple(m.dilation), groups=m.groups)
        E = torch.zeros_like(a) if E is None else E
        ref = act64(F.conv2d(a, w, b, **kw), act)
        mag = F.conv2d(a.abs() + E, w.abs(), b.abs() if b is not None else None, **kw)
        inherited = F.conv2d(E, w.abs(), None, **kw)
        if dtype == "F32":
            E = inherited + n * 2.0 ** -24 * mag
        else:
            own = n * 2.0 ** -23 * mag + 2.0 ** -24
            E = inherited + own + 2.0 ** -11 * (ref.abs() + inherited + own)
        a = ref
    return a, E


def separable_net(pkg, dtype, mult):
    torch.manual_seed(41)
    src = nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), nn.ReLU(), nn.Conv2d(8, 8 * mult, 3, padding=1, groups=8),
                        nn.ReLU6(), nn.Conv2d(8 * mult, 4, 1)).eval().cuda().to(tdtype(dtype))
    with torch.no_grad():
        src[2].weight.mul_(3.0)      # (values on both sides of the cap)
    net = pkg.linkDepthwise(pkg.convert(src, threshold=0.0, depthwise=True))
    conv, dw, head = list(net)
    assert type(dw) is pkg.CBDepthwiseConv2d and dw.propagatedChanges and dw.propChangeIndexes and conv.propChangeIndexes
    assert conv.withReLU and dw.withReLU and dw.reluCap == 6.0 and dw.threshold == 0.0 and head.threshold == 0.0
    conv.exactF32 = head.exactF32 = True
    return net, [(conv, dc.ACT_RELU, 3 * 9 + 1), (dw, dc.ACT_RELU6, 9 + 1), (head, dc.ACT_NONE, 8 * mult + 1)]


@pytest.mark.parametrize("dtype", ["F32", "F16"])
def test_separable_chain_runs_no_detection_in_the_depthwise_layer(pkg, lib, dtype, monkeypatch):
    """CBConv2d -> (ReLU) -> CBDepthwiseConv2d (ReLU6) -> 1x1 CBConv2d after linkDepthwise, every threshold 0, frames
    that differ in blocks only: every frame within the composed bound of the float64 dense network at EVERY pixel; the
    depthwise layer makes one library call per frame, the propagated one, and keeps no input state; its own clearMemory
    in mid-sequence still gives the dense result."""
    import cbinfer_amd.dwconv as dwmod
    net, layers = separable_net(pkg, dtype, 2)
    dw = net[1]
    spy = Spy(lib.C)
    monkeypatch.setattr(dwmod, 'C', spy)
    rng = np.random.default_rng(17)
    frames, changed = block_frames(rng, 3, 20, 70, 7, npdtype(dtype))
    share = []
    hook = dw.register_forward_hook(lambda mod, args, res: share.append(res[2].tensor().numel() / (20 * 70)))
    with torch.no_grad():
        for t, x in enumerate(frames):
            if t == 4:
                dw.clearMemory()
            y = net(dev(x))
            torch.cuda.synchronize()
            ref, E = dense_chain(torch.from_numpy(x), layers, dtype)
            err = (y.cpu().double() - ref).abs()
            print("frame %d: %.1f %% listed, max err / bound %.3g" % (t, 100 * share[-1], float((err / E).max())))
            assert bool((err <= E).all()), (dtype, t, float((err / E).max()))
            assert dw.prevInput.numel() == 0
    hook.remove()
    assert spy.calls == {'cbinfer_cbdwconv2d_forward_propagated': len(frames)}, spy.calls
    assert share[0] == share[4] == 1.0 and 0 < min(share[1:4] + share[5:]) and max(share[1:4] + share[5:]) < 0.5, share


def test_consumers_take_the_mask_the_layer_hands_on(pkg, lib):
    """CBAdd2d, CBConcat2d, CBUpsample2d and the general pools behind a CBDepthwiseConv2d with propChangeIndexes: their
    states equal the torch operator on the layer's state bit for bit, on every frame."""
    geom = GEOMS["3x3s1p1"]
    C, Hi, Wi = 6, 10, 70
    m = pkg.CBDepthwiseConv2d(make_dw(geom, C, 1, True, torch.float32), 0.0)
    m.propChangeIndexes = True
    add, cat = pkg.CBAdd2d(relu=True), pkg.CBConcat2d()
    up = pkg.CBUpsample2d(nn.Upsample(scale_factor=2, mode='nearest'))
    pmax = pkg.CBPoolMax2d(nn.MaxPool2d(3, 2, 1), generalGeometry=True)
    pavg = pkg.CBPoolAvg2d(nn.AvgPool2d(2, 2))
    rng = np.random.default_rng(23)
    frames, _ = block_frames(rng, C, Hi, Wi, 4, np.float32)
    with torch.no_grad():
        for t, x in enumerate(frames):
            y = m(dev(x) - 0.4)
            s = m.prevOutput
            assert torch.equal(raw(add(y, y)), raw(torch.relu(s + s))), t
            assert torch.equal(raw(cat([y, y])), raw(torch.cat([s, s], 1))), t
            assert torch.equal(raw(up(y)), raw(F.interpolate(s, scale_factor=2, mode='nearest'))), t
            assert torch.equal(raw(pmax(y)), raw(F.max_pool2d(s, 3, 2, 1))), t
            assert torch.allclose(pavg(y), F.avg_pool2d(s, 2, 2), rtol=0, atol=1e-6), t
            assert not y[2]._made, t      # (nobody asked for the list)


# ---------------------------------------------------------------------------------------------------------------------
# d. a MobileNetV2-type block: 1x1 expand + ReLU -> 3x3 depthwise + ReLU6 -> 1x1 project, recorded and against float64
# ---------------------------------------------------------------------------------------------------------------------
def make_block(pkg, stride, cloneOutput):
    torch.manual_seed(77)
    body = nn.Sequential(nn.Conv2d(8, 32, 1), nn.ReLU(), nn.Conv2d(32, 32, 3, stride, 1, groups=32), nn.ReLU6(),
                         nn.Conv2d(32, 8, 1)).eval().cuda()
    with torch.no_grad():
        body[2].weight.mul_(4.0)
    cb = pkg.convert(body, threshold=0.0, depthwise=True)
    expand, dw, project = list(cb)
    for m in (expand, dw, project):
        m.cloneOutput = cloneOutput
    expand.exactF32 = project.exactF32 = True
    layers = [(expand, dc.ACT_RELU, 9), (dw, dc.ACT_RELU6, 10), (project, dc.ACT_NONE, 33)]
    if stride == 1:
        net = nn.Sequential(pkg.CBResidual(cb, relu=False))
        net[0].add.cloneOutput = cloneOutput
    else:
        net = cb
    pkg.linkDepthwise(net)
    assert type(dw) is pkg.CBDepthwiseConv2d and dw.reluCap == 6.0 and dw.propagatedChanges and dw.propChangeIndexes
    assert expand.propChangeIndexes
    return net, layers


@pytest.mark.parametrize("stride", [1, 2])
def test_mobilenet_block_against_float64(pkg, lib, stride):
    """Converted with depthwise=True, linked, thresholds 0: every pixel of every frame within the composed bound of the
    float64 dense block (stride 1: inside a CBResidual, the sum one more rounding; stride 2: without)."""
    net, layers = make_block(pkg, stride, True)
    rng = np.random.default_rng(5)
    frames, _ = block_frames(rng, 8, 18, 70, 5, np.float32)
    with torch.no_grad():
        for t, x in enumerate(frames):
            y = net(dev(x))
            torch.cuda.synchronize()
            ref, E = dense_chain(torch.from_numpy(x), layers, "F32")
            if stride == 1:
                ref = ref + torch.from_numpy(x).double()
                E = E + 2.0 ** -24 * (ref.abs() + E)
            err = (y.cpu().double() - ref).abs()
            print("stride %d frame %d: max err / bound %.3g" % (stride, t, float((err / E).max())))
            assert tuple(y.shape) == tuple(ref.shape) and bool((err <= E).all()), (stride, t, float((err / E).max()))
    dw = layers[1][0]
    assert dw.prevInput.numel() == 0


def test_mobilenet_block_records_as_a_launch_program(pkg, lib):
    """With cloneOutput=False the block is library calls only: FrameProgram records it, its calls hold the propagated
    entry point once per frame and no own-detection frame of the depthwise layer; three replayed frames equal the eager
    network in outputs and states bit for bit."""
    net, _ = make_block(pkg, 1, False)
    rng = np.random.default_rng(6)
    frames, _ = block_frames(rng, 8, 18, 70, 7, np.float32)
    frames = [dev(f) for f in frames]
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
        assert raws.count(lib.C.cbinfer_cbdwconv2d_forward_propagated.raw) == 1
        assert lib.C.cbinfer_cbdwconv2d_forward.raw not in raws and lib.C.cbinfer_cbadd_forward.raw in raws
        assert len(pkg.getStateTensors(net)) == 2 * 3 + 1      # two convs and the depthwise layer, the sum


def test_worst_figures_are_reported():
    """The worst err / mag of each dtype over the tests above: measurements, not bars."""
    for dtype, rel in sorted(WORST.items()):
        print("worst err / mag, %s: %.3g = %.2f * 2^-24" % (dtype, rel, rel * 2.0 ** 24))
