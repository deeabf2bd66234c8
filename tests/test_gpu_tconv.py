"""-m gpu: the change-based transposed convolution (cb_tconv.hip) through the raw C ABI --
cbinfer_tconv_prep_weights, cbinfer_change_detection_tconv, cbinfer_conv_changed_tconv -- one case per shape of
tests/tconv_cases.py and arithmetic, and through CBConvTranspose2d (cbinfer_cbconvtranspose2d_forward).

References (nothing expected comes from the code under test): the change rule is the pinned oracle's changeDetection /
changeDetection_half with a 1x1 filter, the footprint the twin's tap loop (tests/test_host_tconv.py), the values a float64
CPU transposed convolution of the map the gather reads (never the device's convolution: DESIGN 5.10).

Bounds, per element, with mag = sum|a||b| + |bias| in float64 and n = C kH kW (tests/test_gpu_geomconv.py):
  F32S  |err| <= 64 * 2^-24 * mag
  F32   |err| <= n * 2^-24 * mag
  F16   |err| <= 2^-11 |ref| + n * 2^-23 * mag + 2^-24, and 2 fp16 ulp of the layer's largest output
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

import tconv_cases as tc
from tconv_cases import ARITH, CASE_BY_ID, CASES, case_form, case_out_hw, case_pixels, case_tags
from test_gpu_geom import footprint as geom_footprint, frames_for
from test_gpu_geomconv import Masks, detection_frame
from test_gpu_listconv import half_tol, pack_mask
from test_host_tconv import tgeom, twin_footprint, twin_reachable
from optest import bits_of, dev, gpu_lib as lib, npdtype, pkg, raw, stream, tdtype      # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

FILL = 77.0
TH = 0.05
WORST = {}       # arithmetic -> worst err / mag seen (printed; a measurement, not a bar)


def tconv64(x, w, b, geom):
    """float64 CPU transposed convolution of torch tensors (pinned against the numpy twin in tests/test_host_tconv.py)."""
    k, s, p, d, op = geom
    return F.conv_transpose2d(x.detach().cpu().double(), w.detach().cpu().double(),
                              b.detach().cpu().double() if b is not None else None, stride=s, padding=p,
                              output_padding=op, dilation=d)


def bound_of(arith, n, want, mag):
    if arith == "F32S":
        return 64 * 2.0 ** -24 * mag
    if arith == "F32":
        return n * 2.0 ** -24 * mag
    return 2.0 ** -11 * abs(want) + n * 2.0 ** -23 * mag + 2.0 ** -24


def frame_buffers(lib, Ho, Wo):
    return torch.zeros(lib.C.cbinfer_frame_mask_bytes(Ho, Wo) // 8, dtype=torch.int64, device="cuda")


def workspace(lib):
    return torch.zeros(lib.C.cbinfer_tconv_workspace_bytes(), dtype=torch.uint8, device="cuda")


class Data(object):
    """A case's tensors on the device, its prepared weights and its float64 reference at EVERY output pixel."""

    def __init__(self, lib, c):
        self.c = c
        k, s, p, d, op = c.geom
        self.n = c.C * k[0] * k[1]
        rng = np.random.default_rng(zlib.crc32(c.id.encode()) + 1)
        t = npdtype(c.arith)
        x = rng.standard_normal((1, c.C, c.Hi, c.Wi)) * np.exp(rng.uniform(-6, 3, (1, c.C, 1, 1)))
        w = rng.standard_normal((c.C, c.K, k[0], k[1])) / np.sqrt(self.n)
        b = rng.standard_normal(c.K)
        x, w, b = x.astype(t), w.astype(t), b.astype(t)
        xt, wt = torch.from_numpy(x), torch.from_numpy(w)
        ref, mag = tconv64(xt, wt, None, c.geom)[0], tconv64(xt.abs(), wt.abs(), None, c.geom)[0]
        self.Ho, self.Wo = case_out_hw(c)
        assert tuple(ref.shape) == (c.K, self.Ho, self.Wo)
        self.HW = self.Ho * self.Wo
        self.ref, self.mag = ref.reshape(c.K, -1).cuda(), mag.reshape(c.K, -1).cuda()      # without the bias
        self.b64 = torch.from_numpy(b.astype(np.float64)).cuda()[:, None]
        self.x, self.bias, wd = dev(x), dev(b), dev(w)
        self.g = tgeom(lib, c.geom)
        gp, code = ctypes.byref(self.g), ARITH[c.arith]
        nbytes = lib.C.cbinfer_tconv_prepared_weights_bytes(c.K, c.C, gp, code)
        assert nbytes == tc.prepared_bytes(c.K, c.C, c.geom, c.arith)
        # (a guard behind the prepared weights: the preparation writes its bytes and no more)
        self.wbuf = torch.full((nbytes + 256,), 0x5a, dtype=torch.uint8, device="cuda")
        self.wp = self.wbuf[:nbytes]
        lib.check(lib.C.cbinfer_tconv_prep_weights(wd.data_ptr(), self.wp.data_ptr(), c.K, c.C, c.Hi, c.Wi, gp, code,
                                                   stream()))
        torch.cuda.synchronize()
        assert bool((self.wbuf[nbytes:] == 0x5a).all())
        self.px = case_pixels(c)
        taps = np.asarray(tc.phase_tap_counts(c.geom))
        self.has_tap = taps[tc.phase_of(c.geom, self.Wo, np.arange(self.HW))] > 0

    def written(self, px):
        """The listed pixels the library writes: those of a phase with a tap."""
        px = np.asarray(px)
        return px[self.has_tap[px]] if len(px) else px

    def buffers(self, lib):
        c = self.c
        B = dict(bits=frame_buffers(lib, self.Ho, self.Wo), ws=workspace(lib) if c.ws else None)
        B['buf'] = torch.full(((c.K + 2) * self.HW,), FILL, dtype=tdtype(c.arith), device="cuda")
        B['out'] = B['buf'][self.HW:(c.K + 1) * self.HW]
        return B


@functools.lru_cache(maxsize=None)
def _data(lib, cid):
    return Data(lib, CASE_BY_ID[cid])


def launch(lib, d, B, lst=None, n=0, count=None, bias=True, relu=0):
    """cbinfer_conv_changed_tconv in list mode (lst given) or mask mode."""
    c = d.c
    p = lambda t: t.data_ptr() if t is not None else None
    st = lib.C.cbinfer_conv_changed_tconv(
        d.x.data_ptr(), p(lst), n, p(count), p(B['bits']) if lst is None else None, d.wp.data_ptr(),
        d.bias.data_ptr() if bias else None, B['out'].data_ptr(), c.C, c.Hi, c.Wi, c.K, ctypes.byref(d.g), relu,
        p(B['ws']), ARITH[c.arith], stream())
    torch.cuda.synchronize()
    return st


def check_values(d, B, px, bias, relu, what):
    """The written pixels within the arithmetic's bound, per element; every other element of the output and both guard
    planes still FILL.  Prints the figures before it asserts."""
    c = d.c
    K, HW = c.K, d.HW
    px_t = dev(np.asarray(px, dtype=np.int64))
    out = B['out'].view(K, HW)
    want, mag = d.ref[:, px_t], d.mag[:, px_t]
    if bias:
        want, mag = want + d.b64, mag + d.b64.abs()
    if relu:
        want = want.clamp(min=0)
    err = (out[:, px_t].double() - want).abs()
    bound = bound_of(c.arith, d.n, want, mag)
    if err.numel():
        nz = mag > 0
        rel = float((err[nz] / mag[nz]).max()) if bool(nz.any()) else 0.0
        WORST[c.arith] = max(WORST.get(c.arith, 0.0), rel)
        line = "%s: max |err| %.3g, max err / mag %.3g = %.2f * 2^-24 (worst so far for %s: %.2f * 2^-24)" % (
            what, float(err.max()), rel, rel * 2.0 ** 24, c.arith, WORST[c.arith] * 2.0 ** 24)
        print(line)
        assert bool((err <= bound).all()), line + "; worst err / bound %.3g" % float((err / (bound + 1e-300)).max())
        if c.arith == "F16":
            tol = half_tol(np.array([float(want.abs().max())]))
            assert float(err.max()) <= tol, line + "; 2 fp16 ulp of the largest output: %.3g" % tol
    rest = B['buf'].clone()
    rest[HW:(K + 1) * HW].view(K, HW)[:, px_t] = FILL
    assert bool((rest == FILL).all()), "%s: a value outside the list changed" % what


def assert_tickets_zero(B, what):
    if B['ws'] is not None:
        assert int(B['ws'][-2048:].ne(0).sum().item()) == 0, what + ": k-split tickets"


# ---------------------------------------------------------------------------------------------------------------------
# a. the contraction: every shape of the table, every arithmetic
# ---------------------------------------------------------------------------------------------------------------------
def run_mask_case(lib, d, B, frames, bias):
    """Consecutive frames on one frame-mask buffer, the mask written as the detection would (into the mask the parity
    selects, which the protocol keeps clean): mask copy, the other mask, parity, arrival counter and tickets after each
    launch, then the values."""
    c = d.c
    M = Masks(lib, B['bits'], d.Ho, d.Wo)
    for name, px, relu in frames:
        what = "%s %s bias=%d relu=%d" % (c.id, name, bias, relu)
        par = M.ctl()[0]
        assert par in (0, 1) and int(M.mask(par).ne(0).sum()) == 0, what
        listed = np.zeros(d.HW, dtype=bool)
        listed[px] = True
        packed = M.packed(listed)
        M.mask(par).copy_(packed)
        B['buf'].fill_(FILL)
        assert launch(lib, d, B, bias=bias, relu=relu) == 0, what
        assert torch.equal(M.mask(par), packed), what + ": the frame's mask"
        assert torch.equal(M.copy(), packed), what + ": the mask copy"
        assert int(M.mask(par ^ 1).ne(0).sum()) == 0, what + ": the other mask"
        assert M.ctl() == [par ^ 1, 0], what + ": parity / arrival counter"
        assert_tickets_zero(B, what)
        check_values(d, B, d.written(px), bias, relu, what)      # (this frame's mask is zeroed by the NEXT launch)


@pytest.mark.parametrize("cid", [c.id for c in CASES])
def test_contraction_cases(lib, cid):
    c = CASE_BY_ID[cid]
    tags, f = case_tags(c), case_form(c)
    assert set(c.claims) <= tags, (cid, sorted(tags), f)
    print("case %s: %s %s" % (cid, sorted(tags), {k: f[k] for k in ("counts", "stages", "tiles", "base", "SK", "items")}))
    d = _data(lib, cid)
    N = len(d.px)
    B = d.buffers(lib)
    if c.source == "mask":
        allpx = np.arange(d.HW, dtype=np.int32)
        none = np.zeros(0, dtype=np.int32)
        # three consecutive frames: the case's pixels, nothing changed, everything changed
        run_mask_case(lib, d, B, [("frame 1", d.px, 0), ("nothing changed", none, 1), ("everything changed", allpx, 1)],
                      True)
        run_mask_case(lib, d, B, [("frame 4", d.px, 1), ("frame 5", d.px, 0)], False)
        return
    lst = dev(d.px)
    count = dev(np.array([N], dtype=np.int32))
    for bias, relu, cnt in ((True, 0, None), (True, 1, count), (False, 0, count), (False, 1, None)):
        what = "%s bias=%d relu=%d %s count" % (cid, bias, relu, "host" if cnt is None else "device")
        B['buf'].fill_(FILL)
        assert launch(lib, d, B, lst, N, cnt, bias=bias, relu=relu) == 0, what
        assert_tickets_zero(B, what)
        check_values(d, B, d.written(d.px), bias, relu, what)


# ---------------------------------------------------------------------------------------------------------------------
# b. list mode at the C ABI: the device count, entries outside the map
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", tc.DEVICE_COUNT_IDS)
def test_list_device_count_below_the_host_count(lib, cid):
    """The kernel takes min(device count, numChanges) entries: the pixels behind the device count keep their bits;
    a device count beyond numChanges does not reach past it; a negative one lists nothing."""
    d = _data(lib, cid)
    N = len(d.px)
    B = d.buffers(lib)
    lst = dev(d.px)
    for n_dev, n_host in ((1, N), (N - 2, N), (N - 1, N), (N + 1000, N - 1), (-5, N)):
        what = "%s device count %d, host count %d" % (cid, n_dev, n_host)
        B['buf'].fill_(FILL)
        count = dev(np.array([n_dev], dtype=np.int32))
        assert launch(lib, d, B, lst, n_host, count, relu=1) == 0, what
        assert_tickets_zero(B, what)
        check_values(d, B, d.written(d.px[:max(0, min(n_dev, n_host))]), True, 1, what)


@pytest.mark.parametrize("cid", tc.OUT_OF_MAP_IDS)
def test_list_entries_outside_the_map_are_dropped(lib, cid):
    """Entries < 0 and >= Ho Wo, shuffled among the case's pixels (the kernel buckets by phase, so the order is free):
    nothing is written through them -- neither into the output nor into the plane in front of it or behind it --, the
    others are computed as ever."""
    d = _data(lib, cid)
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
    assert_tickets_zero(B, what)
    check_values(d, B, d.written(d.px), True, 0, what)


# ---------------------------------------------------------------------------------------------------------------------
# c. the detection: channel split, widths, update modes, every geometry family
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["F32", "F16"])
@pytest.mark.parametrize("name", list(tc.DET_GEOMS))
def test_detection(lib, oracle, name, dtype):
    """cbinfer_change_detection_tconv alone: the state is bit for bit the twin's, the mask of the output map -- read from
    the frame mask before any contraction consumes it -- bit for bit the twin's footprint (so nothing is set beyond Wo in a
    row's last word, and nothing at a pixel no tap reaches), the other mask, the control words and the mask copy
    untouched.  Every seventh launch of a geometry runs on a +inf state (every pixel changed)."""
    geom = tc.DET_GEOMS[name]
    t, code = npdtype(dtype), ARITH[dtype]
    det = oracle.changeDetection if dtype == "F32" else oracle.changeDetection_half
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    g = tgeom(lib, geom)
    for i, (Cin, Hi, Wi, mode) in enumerate(tc.detection_runs(name)):
        tag = (name, dtype, Cin, Hi, Wi, mode)
        Ho, Wo = tc.geom_out_hw(geom, Hi, Wi)
        bits = frame_buffers(lib, Ho, Wo)
        M = Masks(lib, bits, Ho, Wo)
        base = (rng.random((1, Cin, Hi, Wi)) * 0.9).astype(t)
        x = detection_frame(rng, base, TH)
        fresh = i % 7 == 0      # a +inf state: every pixel changed
        state = np.full_like(base, np.inf) if fresh else base.copy()
        sd, xd = dev(state), dev(x)
        lib.check(lib.C.cbinfer_change_detection_tconv(xd.data_ptr(), sd.data_ptr(), bits.data_ptr(), Cin, Hi, Wi,
                                                       ctypes.byref(g), TH, mode, code, stream()))
        torch.cuda.synchronize()
        changed = np.asarray(det(np.ascontiguousarray(x), state, (1, 1), TH, updateInputState=mode == 1))
        if mode == 2:
            state[...] = x
        changed = changed.reshape(Hi, Wi) != 0
        listed = twin_footprint(changed, geom, Ho, Wo)
        if name == "3x3s1p1":      # a single phase: the footprint of the flipped filter's ordinary geometry (5.10)
            assert np.array_equal(listed, geom_footprint(changed, ((3, 3), (1, 1), (1, 1), (1, 1)), Ho, Wo))
        assert changed.all() if fresh else not changed.all() or Hi * Wi < 10, tag
        assert np.array_equal(bits_of(sd.cpu().numpy()), bits_of(state)), tag
        got = M.mask(0).cpu().numpy().view(np.uint64).reshape(Ho, M.wpr)
        want = pack_mask(listed, M.wpr).view(np.uint64).reshape(Ho, M.wpr)
        assert np.array_equal(got, want), tag + (int(listed.sum()),)
        if fresh:
            assert np.array_equal(listed, twin_reachable(geom, Hi, Wi))
        assert int(bits[M.words:].ne(0).sum()) == 0, tag      # mask 1, {parity, counter}, copy


# ---------------------------------------------------------------------------------------------------------------------
# d. the module: sequences against the twin
# ---------------------------------------------------------------------------------------------------------------------
class Twin(object):
    """Rules 1 and 2 on the CPU: the oracle's change rule, the refresh of the mode, the twin's footprint."""

    def __init__(self, oracle, geom, th, feedback):
        self.oracle, self.geom, self.th, self.feedback, self.state = oracle, geom, th, feedback, None

    def step(self, x):
        """x: numpy [1, C, Hi, Wi] in the layer's dtype -> the listed output map (bool)"""
        if self.state is None:
            self.state = np.full_like(x, np.inf)
        det = self.oracle.changeDetection if x.dtype == np.float32 else self.oracle.changeDetection_half
        changed = det(np.ascontiguousarray(x), self.state, (1, 1), self.th, updateInputState=self.feedback)
        if not self.feedback:
            self.state[...] = x
        return twin_footprint(np.asarray(changed).reshape(x.shape[-2:]) != 0, self.geom)


def make_tconv(geom, Cin, K, bias, dtype):
    k, s, p, d, op = geom
    torch.manual_seed(zlib.crc32(repr((geom, Cin, K)).encode()))
    return nn.ConvTranspose2d(Cin, K, k, s, p, op, 1, bias, d).cuda().to(dtype)


def sequence(rng, Cin, Hi, Wi, npd):
    """Six frames: block-wise changes (about a tenth of the blocks), the fourth repeats the third (an idle frame)."""
    fr = frames_for(rng, Cin, Hi, Wi, 5, npd)
    return fr[:3] + [fr[2].copy()] + fr[3:]


def check_frame(m, y, prev, listed, geom, arith, reach, tag):
    """The listed pixels against the float64 transposed convolution of the device's own prevInput, the others bit for
    bit what they were; pixels no tap reaches hold relu(bias)."""
    out = y.detach().cpu().numpy()[0]
    src = m.prevInput.detach()
    k = geom[0]
    n = m.in_channels * k[0] * k[1]
    ref = tconv64(src, m.weight, m.bias, geom)[0].numpy()
    mag = tconv64(src.abs(), m.weight.abs(), m.bias.abs() if m.bias is not None else None, geom)[0].numpy()
    if m.withReLU:
        ref = np.maximum(ref, 0)
    err = np.abs(out.astype(np.float64) - ref)
    bound = bound_of(arith, n, ref, mag)
    print("%s: %d listed, max err / bound %.3g" % (tag, int(listed.sum()),
                                                   float((err / (bound + 1e-300))[:, listed].max()) if listed.any() else 0.0))
    assert np.all(err[:, listed] <= bound[:, listed]), tag
    if arith == "F16" and listed.any():
        assert err[:, listed].max() <= half_tol(ref), tag
    if prev is not None:
        assert np.array_equal(bits_of(out)[:, ~listed], bits_of(prev)[:, ~listed]), tag
    if not reach.all():
        b = m.bias.detach().cpu().numpy() if m.bias is not None else np.zeros(m.out_channels, dtype=out.dtype)
        fill = np.maximum(b, 0) if m.withReLU else b
        assert np.array_equal(bits_of(out[:, ~reach]), bits_of(np.broadcast_to(fill[:, None], out[:, ~reach].shape))), tag
    return out


MODULE_GEOMS = ["2x2s2", "4x4s2p1", "3x3s2p1op1", "1x1s2op1", "2x2s3op2", "aniso"]


@pytest.mark.parametrize("mode", ["feedback", "copy", "nocopy"])
@pytest.mark.parametrize("dtype", ["F32S", "F16"])
def test_module_tracks_the_twin(pkg, lib, oracle, dtype, mode):
    """Six-frame sequences per geometry (one idle frame): the mask handed on, the list made from it and prevInput equal
    the twin's bit for bit; listed pixels within the bound, unlisted ones keep their bits, unreachable ones hold
    relu(bias) on every frame.  withReLU and a bias-free layer alternate over the geometries."""
    from cbinfer_amd.conv2d_cg import MaskChangeIndexes
    for gi, name in enumerate(MODULE_GEOMS):
        geom = tc.DET_GEOMS[name]
        Cin, K, Hi, Wi = (5, 33, 9, 40) if gi % 2 else (16, 70, 7, 33)
        m = pkg.CBConvTranspose2d(make_tconv(geom, Cin, K, gi % 3 != 2, tdtype(dtype)), TH)
        m.feedbackLoop, m.copyInput, m.withReLU, m.propChangeIndexes = mode == "feedback", mode != "nocopy", gi % 2 == 0, True
        twin = Twin(oracle, geom, TH, mode == "feedback")
        rng = np.random.default_rng(100 + gi)
        reach = twin_reachable(geom, Hi, Wi)
        Ho, Wo = reach.shape
        prev, counts = None, []
        with torch.no_grad():
            for t, x in enumerate(sequence(rng, Cin, Hi, Wi, npdtype(dtype))):
                tag = (name, dtype, mode, t)
                kind, y, ix = m(dev(x))
                torch.cuda.synchronize()
                listed = twin.step(x)
                assert kind == 'changeIndexes' and isinstance(ix, MaskChangeIndexes) and ix.size == (Ho, Wo), tag
                assert tuple(y.shape) == (1, K, Ho, Wo), tag
                wpr = (Wo + 63) // 64
                assert np.array_equal(ix._mask.cpu().numpy(), pack_mask(listed, wpr)), tag
                assert np.array_equal(ix.tensor().cpu().numpy(), np.flatnonzero(listed.reshape(-1))), tag
                assert np.array_equal(bits_of(m.prevInput.cpu().numpy()), bits_of(twin.state)), tag
                prev = check_frame(m, y, prev, listed, geom, dtype, reach, tag)
                counts.append(int(listed.sum()))
        assert counts[0] == int(reach.sum()) and counts[3] == 0 and 0 < min(counts[1:3] + counts[4:]), (name, counts)
        assert max(counts[1:]) < counts[0], (name, counts)
        assert m._arith(dev(x)) == ARITH[dtype]


def test_exact_f32_threshold_change_and_clear_memory(pkg, lib, oracle):
    """exactF32 reaches the f32 MFMA (prepared weights and launches are CB_F32's, the f32 chain's bound holds); a
    threshold raised in the middle of a sequence lists fewer pixels, as the twin says; clearMemory makes the next frame
    dense again; a new resolution reallocates the state."""
    geom = tc.T4
    Cin, K, Hi, Wi = 13, 33, 9, 40
    m = pkg.CBConvTranspose2d(make_tconv(geom, Cin, K, True, torch.float32), TH)
    m.exactF32, m.propChangeIndexes, m.feedbackLoop = True, True, True
    twin = Twin(oracle, geom, TH, True)
    rng = np.random.default_rng(7)
    frames = sequence(rng, Cin, Hi, Wi, np.float32)
    reach = twin_reachable(geom, Hi, Wi)
    prev, counts = None, []
    with torch.no_grad():
        for t, x in enumerate(frames):
            if t == 2:
                m.threshold = twin.th = 0.6      # (most of a moved block's pixels stay below it)
            if t == 4:
                m.clearMemory()
                twin.state, prev = None, None
                assert m.prevOutput.numel() == 0 and m._work is None
            _, y, ix = m(dev(x))
            torch.cuda.synchronize()
            listed = twin.step(x)
            assert m._wprep[0][-1] == lib.CB_F32
            assert np.array_equal(ix.tensor().cpu().numpy(), np.flatnonzero(listed.reshape(-1))), t
            assert np.array_equal(bits_of(m.prevInput.cpu().numpy()), bits_of(twin.state)), t
            prev = check_frame(m, y, prev, listed, geom, "F32", reach, ("exactF32", t))
            counts.append(int(listed.sum()))
        assert counts[0] == counts[4] == reach.size and 0 < counts[1] < reach.size and counts[3] == 0, counts
        assert 0 < counts[5] < reach.size
        x2 = frames_for(rng, Cin, 5, 70, 1, np.float32)[0]
        _, y, ix = m(dev(x2))
        assert tuple(y.shape) == (1, K, 10, 140) and ix.tensor().numel() == 1400
        assert tuple(m.prevInput.shape) == (1, Cin, 5, 70)


def test_change_mask_feeds_a_concat_with_a_skip(pkg, lib, oracle):
    """propChangeIndexes into a CBConcat2d together with a skip connection in list form: the mask the layer hands on is
    the twin's, the concat copies the layer's channels at exactly those pixels (its state equals torch.cat of the two
    dense maps bit for bit) and hands on the union."""
    geom = tc.T2
    Cin, K, Hi, Wi = 8, 6, 12, 20
    m = pkg.CBConvTranspose2d(make_tconv(geom, Cin, K, True, torch.float32), TH)
    m.propChangeIndexes = True
    cat = pkg.CBConcat2d()
    cat.propChangeIndexes = True
    twin = Twin(oracle, geom, TH, False)
    rng = np.random.default_rng(3)
    skips = [rng.random((1, 4, 2 * Hi, 2 * Wi)).astype(np.float32)]
    for t in range(1, 6):      # one moved block per frame; the fifth frame repeats the fourth
        s = skips[-1].copy()
        if t != 4:
            y0, x0 = int(rng.integers(0, 2 * Hi - 4)), int(rng.integers(0, 2 * Wi - 6))
            s[:, :, y0:y0 + 4, x0:x0 + 6] += 1.0
        skips.append(s)
    wpr = 1
    with torch.no_grad():
        for t, x in enumerate(sequence(rng, Cin, Hi, Wi, np.float32)):
            skip = dev(skips[t])
            moved = np.ones((2 * Hi, 2 * Wi), dtype=bool) if t == 0 else (skips[t] != skips[t - 1]).any(axis=(0, 1))
            up = m(dev(x))
            listed = twin.step(x)
            assert np.array_equal(up[2]._mask.cpu().numpy(), pack_mask(listed, wpr)), t
            kind, z, ix = cat([up, ('changeIndexes', skip, dev(np.flatnonzero(moved.reshape(-1)).astype(np.int32)))])
            torch.cuda.synchronize()
            assert torch.equal(z.view(torch.int32), torch.cat([m.prevOutput, skip], 1).view(torch.int32)), t
            want = listed | moved if t else np.ones_like(moved)      # (a new concat state is written completely)
            assert np.array_equal(ix._mask.cpu().numpy(), pack_mask(want, wpr)), t


# ---------------------------------------------------------------------------------------------------------------------
# e. a decoder stage: conv -> transposed conv -> concat(skip) -> conv, recorded and against the dense layer
# ---------------------------------------------------------------------------------------------------------------------
class Stage(nn.Module):
    """conv1 (24x40, the skip) -> 2x2 pool -> conv2 (12x20) -> ConvTranspose2d 2x2 s2 -> concat with the skip -> 1x1 head.
    kind 'cb': the transposed convolution and the concat change-based; 'dense': the same converted layers with the
    transposed layer left to torch (F.conv_transpose2d, torch.cat)."""

    def __init__(self, body, cat, head, kind):
        super(Stage, self).__init__()
        self.body, self.cat, self.head, self.kind = body, cat, head, kind

    def forward(self, x):
        conv1, pool, conv2, up = list(self.body)
        skip = conv1(x)
        y = conv2(pool(skip))
        if self.kind == 'cb':
            return self.head(self.cat([up(y), skip]))
        u = F.relu(F.conv_transpose2d(y, up.weight, up.bias, stride=2))
        return self.head(torch.cat([u, skip[1]], 1))


def make_stage(pkg, cloneOutput, threshold):
    torch.manual_seed(31)
    src = nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), nn.ReLU(), nn.MaxPool2d(2), nn.Conv2d(8, 16, 3, padding=1), nn.ReLU(),
                        nn.ConvTranspose2d(16, 8, 2, 2), nn.ReLU())
    body = pkg.convert(src.eval().cuda(), threshold=TH)
    pkg.insertCBPooling(body, cloneOutput=cloneOutput)
    pkg.insertCBTransposedConv(body, threshold=threshold, cloneOutput=cloneOutput)
    conv1, pool, conv2, up = list(body)
    assert type(pool) is pkg.CBPoolMax2d and type(up) is pkg.CBConvTranspose2d and up.withReLU
    assert up.threshold == threshold and up.cloneOutput == cloneOutput and conv1.propChangeIndexes
    up.propChangeIndexes = True
    cat = pkg.CBConcat2d()
    cat.cloneOutput = cloneOutput
    head = pkg.convert(nn.Sequential(nn.Conv2d(16, 4, 1)).eval().cuda(), threshold=TH)[0]
    return Stage(body, cat, head, 'cb')


def stage_frames(n, seed):
    """Frames at 24x40 with block-wise changes."""
    rng = np.random.default_rng(seed)
    base = rng.random((1, 3, 24, 40)) * 0.9
    out = []
    for t in range(n):
        base = base.copy()
        for _ in range(2):
            y0, x0 = int(rng.integers(0, 24)), int(rng.integers(0, 40))
            base[:, :, y0:y0 + 5, x0:x0 + 9] = rng.random(base[:, :, y0:y0 + 5, x0:x0 + 9].shape) * 0.9
        out.append(torch.from_numpy(base.astype(np.float32)).cuda())
    return out


def test_decoder_stage_records_as_a_launch_program(pkg, lib):
    """With cloneOutput=False the stage is library calls only: FrameProgram records it, its calls hold the new entry
    point once per frame, replays equal the eager network in outputs and states bit for bit; the copy with the dense
    transposed layer is refused."""
    net = make_stage(pkg, False, TH)
    frames = stage_frames(9, 52)
    with torch.no_grad():
        for f in frames[:4]:
            net(f)
        eager = copy.deepcopy(net)
        dense = copy.deepcopy(net)
        dense.kind = 'dense'
        prog = pkg.FrameProgram(net)
        for t, f in enumerate(frames[4:]):
            yp, ye = prog(f), eager(f)
            assert torch.equal(raw(yp), raw(ye)), t
            for ta, tb in zip(pkg.getStateTensors(net), pkg.getStateTensors(eager)):
                assert torch.equal(ta, tb), t
        raws = [fn for fn, _ in prog.calls]
        assert raws.count(lib.C.cbinfer_cbconvtranspose2d_forward.raw) == 1
        assert lib.C.cbinfer_cbconcat_forward.raw in raws
        assert len(pkg.getStateTensors(net)) == 2 * 3 + 1 + 2 + 1      # three convs, pool, transposed conv, concat
        with pytest.raises(lib.CBinferError, match="CBConvTranspose2d"):
            pkg.FrameProgram(dense).record(frames[-1])


def test_decoder_stage_against_the_dense_transposed_layer(pkg, lib):
    """The stage with the transposed layer at threshold 0 -- every input pixel that differs is listed, so an unlisted
    output pixel reads exactly the inputs it was last computed from -- against the same converted layers with the
    transposed layer left dense: both feed the layer bit-identical maps; the change-based layer's output is within the
    F32S bound of the float64 transposed convolution of that map at EVERY pixel, bit-identical to its previous frame at
    the unlisted ones, and the layer really ran change-based.  (The dense layer's own values are the vendor library's
    and are only reported.)"""
    net = make_stage(pkg, True, 0.0)
    dense = copy.deepcopy(net)
    dense.kind = 'dense'
    up = net.body[3]
    seen = {}
    hooks = [up.register_forward_hook(lambda mod, args, res: seen.update(inp=args[0], res=res))]
    prev, shares = None, []
    with torch.no_grad():
        for t, f in enumerate(stage_frames(6, 51)):
            net(f)
            dense(f)
            torch.cuda.synchronize()
            y = seen['inp'][1] if type(seen['inp']) == tuple else seen['inp']
            yd = dense.body[2].prevOutput
            assert torch.equal(raw(y), raw(yd)), t
            _, u, ix = seen['res']
            listed = np.zeros(24 * 40, dtype=bool)
            listed[ix.tensor().cpu().numpy()] = True
            listed = listed.reshape(24, 40)
            ref = torch.relu(tconv64(yd, up.weight, up.bias, tc.T2))[0].numpy()
            mag = tconv64(yd.abs(), up.weight.abs(), up.bias.abs(), tc.T2)[0].numpy()
            out = u.cpu().numpy()[0]
            err = np.abs(out.astype(np.float64) - ref)
            assert np.all(err <= 64 * 2.0 ** -24 * mag), (t, float((err / (mag + 1e-300)).max()) * 2.0 ** 24)
            if prev is not None:
                assert np.array_equal(bits_of(out)[:, ~listed], bits_of(prev)[:, ~listed]), t
            vendor = F.relu(F.conv_transpose2d(yd, up.weight, up.bias, stride=2))[0].cpu().numpy()
            print("frame %d: %d listed; |vendor - float64| max %.3g, |change-based - float64| max %.3g"
                  % (t, int(listed.sum()), float(np.abs(vendor - ref).max()), float(err.max())))
            prev = out
            shares.append(listed.mean())
    for h in hooks:
        h.remove()
    assert shares[0] == 1.0 and 0.0 < min(shares[1:]) and max(shares[1:]) < 1.0, shares


def test_worst_figures_are_reported():
    """The worst err / mag of each arithmetic over the tests above: measurements, not bars."""
    for arith, rel in sorted(WORST.items()):
        print("worst err / mag, %s: %.3g = %.2f * 2^-24" % (arith, rel, rel * 2.0 ** 24))
