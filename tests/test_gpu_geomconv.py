"""-m gpu: the general-geometry detection and contraction (cb_geomconv.hip) through the raw C ABI --
cbinfer_geom_prep_weights, cbinfer_change_detection_geom, cbinfer_conv_changed_geom, cbinfer_cbconv2d_forward_geom --,
one case per cell of the arithmetic x source x regime x mask-class table of tests/geomconv_cases.py.

References (nothing expected comes from the code under test): the change rule is the pinned oracle's changeDetection /
changeDetection_half with a 1x1 filter, the footprint the twin's tap loop (tests/test_gpu_geom.py), the values a float64
CPU convolution of the map the gather reads (never the device's convolution: DESIGN 5.10).

Bounds, per element, with mag = sum|a||b| + |bias| in float64:
  F32S  |err| <= 64 * 2^-24 * mag                        (the bar of the list contraction and the split-state kernels)
  F32   |err| <= Ckk * 2^-24 * mag                       (the f32 chain's own bound)
  F16   |err| <= 2^-11 |ref| + Ckk * 2^-23 * mag + 2^-24 (exact products, one f32 rounding per accumulated term with a
        factor 2 for the matrix unit's internal rounding, the final rounding to f16, half the smallest subnormal), and
        2 fp16 ulp of the layer's largest output.
Operands span many binades (every input channel times exp(U(-6, 3))).  Every unlisted output element must keep its
bits; a guard plane in front of and behind the output must stay untouched."""
import ctypes
import functools
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import geomconv_cases as gc
from geomconv_cases import ARITH, CASE_BY_ID, CASES, case_form, case_out_hw, case_pixels, cell_of
from test_gpu_geom import GEOMS, Twin, _c_abi_buffers, footprint, frames_for, make_conv, out_size
from test_gpu_listconv import half_tol, pack_mask
from optest import bits_of, dev, gpu_lib as lib, npdtype, stream, tdtype      # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

FILL = 77.0
TH = 0.05
WORST = {}       # arithmetic -> worst err / mag seen (printed; a measurement, not a bar)


class Data(object):
    """A case's tensors on the device, its prepared weights and its float64 reference at EVERY output pixel."""

    def __init__(self, lib, c, taps=None):
        self.c = c
        (kH, kW), s, p, d = c.geom
        self.Ckk = c.C * kH * kW
        rng = np.random.default_rng(zlib.crc32(c.id.encode()) + 1)
        t = npdtype(c.arith)
        x = rng.standard_normal((1, c.C, c.Hi, c.Wi)) * np.exp(rng.uniform(-6, 3, (1, c.C, 1, 1)))
        if taps is not None:      # sparse operand: about `taps` non-zero values per gathered patch
            x = x * (np.random.default_rng(17).random(x.shape) < taps / float(self.Ckk))
        w = rng.standard_normal((c.K, c.C, kH, kW)) / np.sqrt(self.Ckk)
        b = rng.standard_normal(c.K)
        x, w, b = x.astype(t), w.astype(t), b.astype(t)
        x64, w64 = torch.from_numpy(x.astype(np.float64)), torch.from_numpy(w.astype(np.float64))
        ref = F.conv2d(x64, w64, None, stride=s, padding=p, dilation=d)[0]
        mag = F.conv2d(x64.abs(), w64.abs(), None, stride=s, padding=p, dilation=d)[0]
        self.Ho, self.Wo = case_out_hw(c)
        assert tuple(ref.shape) == (c.K, self.Ho, self.Wo)
        self.HW = self.Ho * self.Wo
        self.ref, self.mag = ref.reshape(c.K, -1).cuda(), mag.reshape(c.K, -1).cuda()      # without the bias
        self.b64 = torch.from_numpy(b.astype(np.float64)).cuda()[:, None]
        self.x, self.bias, wd = dev(x), dev(b), dev(w)
        self.g = lib.Geom(kH, kW, s[0], s[1], p[0], p[1], d[0], d[1])
        gp = ctypes.byref(self.g)
        code = ARITH[c.arith]
        self.wp = torch.empty(lib.C.cbinfer_geom_prepared_weights_bytes(c.K, c.C, gp, code), dtype=torch.uint8,
                              device="cuda")
        lib.check(lib.C.cbinfer_geom_prep_weights(wd.data_ptr(), self.wp.data_ptr(), c.K, c.C, c.Hi, c.Wi, gp, code,
                                                  stream()))
        torch.cuda.synchronize()
        self.px = case_pixels(c)

    def buffers(self, lib):
        """The C ABI buffers of tests/test_gpu_geom.py plus an output with a guard plane in front and behind."""
        c = self.c
        g, Ho, Wo, B = _c_abi_buffers(lib, lib.C, c.geom, c.C, c.K, c.Hi, c.Wi, tdtype(c.arith))
        assert (Ho, Wo) == (self.Ho, self.Wo)
        B['buf'] = torch.full(((c.K + 2) * self.HW,), FILL, dtype=tdtype(c.arith), device="cuda")
        B['out'] = B['buf'][self.HW:(c.K + 1) * self.HW]
        if not c.ws:
            B['ws'] = None
        return B


@functools.lru_cache(maxsize=None)
def _data(lib, cid):
    return Data(lib, CASE_BY_ID[cid])


def launch(lib, d, B, lst=None, n=0, count=None, bias=True, relu=0):
    """cbinfer_conv_changed_geom in list mode (lst given) or mask mode."""
    c = d.c
    p = lambda t: t.data_ptr() if t is not None else None
    mask = lst is None
    st = lib.C.cbinfer_conv_changed_geom(
        d.x.data_ptr(), p(lst), n, p(count), p(B['bits']) if mask else None, p(B['idx']) if mask else None,
        p(B['count']) if mask else None, d.wp.data_ptr(), d.bias.data_ptr() if bias else None, B['out'].data_ptr(),
        c.C, c.Hi, c.Wi, c.K, ctypes.byref(d.g), relu, p(B['ws']), ARITH[c.arith], stream())
    torch.cuda.synchronize()
    return st


def check_values(d, B, px, bias, relu, what):
    """The listed pixels within the arithmetic's bound, per element; every other element of the output and both guard
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
    if c.arith == "F32S":
        bound = 64 * 2.0 ** -24 * mag
    elif c.arith == "F32":
        bound = d.Ckk * 2.0 ** -24 * mag
    else:
        bound = 2.0 ** -11 * want.abs() + d.Ckk * 2.0 ** -23 * mag + 2.0 ** -24
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


def assert_claimed_cell(c, n=None):
    f = case_form(c, n)
    got = cell_of(c, f)
    assert got == (c.arith, c.source, c.regime, c.mask_class), (c.id, got, f)
    return f


class Masks(object):
    """Views of a frame mask buffer: [mask 0][mask 1]{parity, arrival counter}[copy of the frame's mask]."""

    def __init__(self, lib, bits, Ho, Wo):
        C = lib.C
        self.bits, self.Ho, self.Wo = bits, Ho, Wo
        self.words, self.wpr = C.cbinfer_mask_words(Ho, Wo), C.cbinfer_mask_words_per_row(Wo)
        self.copy_at = C.cbinfer_frame_mask_copy_offset(Ho, Wo) // 8
        assert self.words == Ho * self.wpr == gc.mask_words(Ho, Wo)
        assert bits.numel() == self.copy_at + self.words and self.copy_at == 2 * self.words + 2

    def ctl(self):
        return self.bits[2 * self.words:2 * self.words + 1].view(torch.int32).tolist()

    def mask(self, which):
        return self.bits[which * self.words:(which + 1) * self.words]

    def copy(self):
        return self.bits[self.copy_at:self.copy_at + self.words]

    def packed(self, listed):
        return dev(pack_mask(np.asarray(listed, dtype=bool).reshape(self.Ho, self.Wo), self.wpr))


# ---------------------------------------------------------------------------------------------------------------------
# a. the contraction: every cell of the table
# ---------------------------------------------------------------------------------------------------------------------
def run_mask_case(lib, d, B, frames, bias):
    """Consecutive frames on one frame-mask buffer, the mask written as the detection would (into the mask the parity
    selects, which the protocol keeps clean): list and order, count, mask copy, the other mask, parity, arrival
    counter and tickets after each launch, then the values."""
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
        assert_tickets_zero(B, what)
        check_values(d, B, px, bias, relu, what)      # (this frame's mask is zeroed by the NEXT launch: checked there)


@pytest.mark.parametrize("cid", [c.id for c in CASES])
def test_contraction_cells(lib, cid):
    c = CASE_BY_ID[cid]
    f = assert_claimed_cell(c)
    d = _data(lib, cid)
    N = len(d.px)
    print("cell %s: %s" % (cell_of(c, f), {k: f[k] for k in ("stages", "tilesN", "tilesM", "base", "SK", "items",
                                                              "chunk")}))
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
        check_values(d, B, d.px, bias, relu, what)


@pytest.mark.parametrize("cid", gc.SPARSE_IDS)
def test_f32s_low_terms_on_sparse_operands(lib, cid):
    """The F32S bound on an input with about one non-zero value per gathered patch, no bias.  In a deep dense sum a
    dropped lo x hi product of the bf16 triples (2^-17 of ONE product) hides behind sum|a||b| of hundreds of terms; here
    the sum is that one product, at every k position in turn.  Where no tap is non-zero the output is exactly zero."""
    c = CASE_BY_ID[cid]
    assert c.arith == "F32S"
    assert_claimed_cell(c)
    d = Data(lib, c, taps=1.5)
    hit = float((d.mag[:, dev(d.px.astype(np.int64))] > 0).double().mean())
    print("%s: %.0f %% of the listed outputs see a non-zero tap" % (cid, 100 * hit))
    assert 0.15 < hit < 0.95
    B = d.buffers(lib)
    if c.source == "mask":
        run_mask_case(lib, d, B, [("sparse operand", d.px, 0)], False)
    else:
        assert launch(lib, d, B, dev(d.px), len(d.px), bias=False) == 0
        assert_tickets_zero(B, cid)
        check_values(d, B, d.px, False, 0, cid + " sparse operand")


# ---------------------------------------------------------------------------------------------------------------------
# b. list mode at the C ABI: the device count, entries outside the map
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", gc.DEVICE_COUNT_IDS)
def test_list_device_count_below_the_host_count(lib, cid):
    """The kernel takes min(device count, numChanges) entries: the pixels behind the device count keep their bits;
    a device count beyond numChanges does not reach past it; a negative one lists nothing."""
    c = CASE_BY_ID[cid]
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
        check_values(d, B, d.px[:max(0, min(n_dev, n_host))], True, 1, what)


@pytest.mark.parametrize("cid", gc.OUT_OF_MAP_IDS)
def test_list_entries_outside_the_map_are_dropped(lib, cid):
    """Entries < 0 and >= Ho Wo, shuffled among the case's pixels: nothing is written through them -- neither into the
    output nor into the plane in front of it or behind it --, the others are computed as ever."""
    c = CASE_BY_ID[cid]
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
    check_values(d, B, d.px, True, 0, what)


@pytest.mark.parametrize("arith", ["F32S", "F32", "F16"])
def test_padded_k_taps_stay_outside_a_tall_map(lib, arith):
    """The k-depth is padded to 32 with taps that must lie outside every map.  Their table entry used to be
    dy = -32768, dx = 0: for a base pixel (oy sH, ox sW) at row 32768 or beyond of a taller map that is a pixel INSIDE the
    map, read and multiplied by the zero weight -- NaN where it holds an inf.  1x1, padding (1, 0), one channel, 33000 x 1:
    output row oy reads input row oy - 1, its base pixel (oy, 0) is no tap.  Listed: rows whose base pixel holds +inf, below
    and beyond row 32768, all inside the input map; every one must come out as w x[oy - 1] + b."""
    Hi, Wi, geom = 33000, 1, ((1, 1), (1, 1), (1, 0), (1, 1))
    rng = np.random.default_rng(2)
    t = npdtype(arith)
    x = rng.standard_normal((1, 1, Hi, Wi)).astype(t)
    rows = np.array([5, 100, 32766, 32768, 32770, 32900, 32999], dtype=np.int32)
    x[0, 0, rows, 0] = np.inf
    w, b = np.array([[[[0.75]]]], dtype=t), np.array([0.5], dtype=t)
    g, Ho, Wo, B = _c_abi_buffers(lib, lib.C, geom, 1, 1, Hi, Wi, tdtype(arith))
    assert (Ho, Wo) == (Hi + 2, 1)
    gp, code = ctypes.byref(g), ARITH[arith]
    wp = torch.empty(lib.C.cbinfer_geom_prepared_weights_bytes(1, 1, gp, code), dtype=torch.uint8, device="cuda")
    wd, bd, xd, lst = dev(w), dev(b), dev(x), dev(rows)
    lib.check(lib.C.cbinfer_geom_prep_weights(wd.data_ptr(), wp.data_ptr(), 1, 1, Hi, Wi, gp, code, stream()))
    lib.check(lib.C.cbinfer_conv_changed_geom(xd.data_ptr(), lst.data_ptr(), len(rows), None, None, None, None,
                                              wp.data_ptr(), bd.data_ptr(), B['out'].data_ptr(), 1, Hi, Wi, 1, gp, 0,
                                              B['ws'].data_ptr(), code, stream()))
    torch.cuda.synchronize()
    got = B['out'].cpu().numpy().reshape(-1).astype(np.float64)
    xs = x[0, 0, rows - 1, 0].astype(np.float64)
    assert np.isfinite(xs).all()
    want, mag = 0.75 * xs + 0.5, 0.75 * np.abs(xs) + 0.5
    err = np.abs(got[rows] - want)
    print("%s: outputs %s, wanted %s" % (arith, got[rows], want))
    assert np.all(err <= (2.0 ** -10 if arith == "F16" else 64 * 2.0 ** -24) * mag), (arith, got[rows], want)
    rest = got.copy()
    rest[rows] = 7.0
    assert np.all(rest == 7.0)


# ---------------------------------------------------------------------------------------------------------------------
# c. the detection: channel split, widths, update modes, geometries at the limits
# ---------------------------------------------------------------------------------------------------------------------
def detection_frame(rng, base, th):
    """A frame against the state `base`: about a tenth of the pixels moved by 1.5 th on one channel (changed), as many
    by 0.4 th (not changed), the rest equal."""
    _, C, Hi, Wi = base.shape
    x = base.astype(np.float64)
    n = max(1, Hi * Wi // 10)
    for amount in (1.5 * th, 0.4 * th):
        ys, xs, cs = rng.integers(0, Hi, n), rng.integers(0, Wi, n), rng.integers(0, C, n)
        x[0, cs, ys, xs] = base[0, cs, ys, xs].astype(np.float64) + amount * rng.choice([-1.0, 1.0], n)
    return x.astype(base.dtype)


@pytest.mark.parametrize("dtype", ["F32", "F16"])
@pytest.mark.parametrize("name", list(gc.DET_LIMIT_GEOMS) + list(gc.DET_PLAIN))
def test_detection(lib, oracle, name, dtype):
    """cbinfer_change_detection_geom alone: the state is bit for bit the twin's, the mask of the output map -- read from
    the frame mask before any contraction consumes it -- bit for bit the twin's footprint (so nothing is set beyond
    Wo in a row's last word either), the other mask, the control words and the mask copy untouched.  Every seventh
    launch of a geometry runs on a +inf state (every pixel changed)."""
    geom = gc.DET_LIMIT_GEOMS[name] if name in gc.DET_LIMIT_GEOMS else gc.DET_PLAIN[name][0]
    (kH, kW), s, p, d = geom
    t, code = npdtype(dtype), ARITH[dtype]
    det = oracle.changeDetection if dtype == "F32" else oracle.changeDetection_half
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    for i, (Cin, Hi, Wi, mode) in enumerate(gc.detection_runs(name)):
        tag = (name, dtype, Cin, Hi, Wi, mode)
        g, Ho, Wo, B = _c_abi_buffers(lib, lib.C, geom, Cin, 1, Hi, Wi, tdtype(dtype))
        assert (Ho, Wo) == (out_size(Hi, kH, s[0], p[0], d[0]), out_size(Wi, kW, s[1], p[1], d[1]))
        M = Masks(lib, B['bits'], Ho, Wo)
        base = (rng.random((1, Cin, Hi, Wi)) * 0.9).astype(t)
        x = detection_frame(rng, base, TH)
        fresh = i % 7 == 0      # a +inf state: every pixel changed
        state = np.full_like(base, np.inf) if fresh else base.copy()
        B['state'].copy_(dev(state))
        xd = dev(x)
        lib.check(lib.C.cbinfer_change_detection_geom(xd.data_ptr(), B['state'].data_ptr(), B['bits'].data_ptr(), Cin,
                                                      Hi, Wi, ctypes.byref(g), TH, mode, code, stream()))
        torch.cuda.synchronize()
        changed = np.asarray(det(np.ascontiguousarray(x), state, (1, 1), TH, updateInputState=mode == 1))
        if mode == 2:
            state[...] = x
        listed = footprint(changed.reshape(Hi, Wi) != 0, geom, Ho, Wo)
        assert changed.all() if fresh else not changed.all() or Hi * Wi < 10, tag
        assert np.array_equal(bits_of(B['state'].cpu().numpy()), bits_of(state)), tag
        got = M.mask(0).cpu().numpy().view(np.uint64).reshape(Ho, M.wpr)
        want = pack_mask(listed, M.wpr).view(np.uint64).reshape(Ho, M.wpr)
        assert np.array_equal(got, want), tag + (int(listed.sum()),)
        if Wo % 64:
            assert not (got[:, -1] >> np.uint64(Wo % 64)).any(), tag
        assert int(B['bits'][M.words:].ne(0).sum()) == 0, tag      # mask 1, {parity, counter}, copy


# ---------------------------------------------------------------------------------------------------------------------
# d. detection + contraction in one call; the module's arithmetic switch
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ["F32S", "F32", "F16"])
def test_forward_geom_tracks_the_twin(lib, oracle, arith):
    """cbinfer_cbconv2d_forward_geom (feedback mode, ReLU) over four frames at a geometry with unreachable output pixels
    and a stride: list, state and listed values against the twin, unlisted pixels keep their bits."""
    geom = ((3, 3), (2, 2), (3, 3), (1, 1))
    Cin, K, Hi, Wi = 5, 33, 9, 130
    dt = tdtype(arith)
    conv = make_conv(geom, Cin, K, True, dt)
    g, Ho, Wo, B = _c_abi_buffers(lib, lib.C, geom, Cin, K, Hi, Wi, dt)
    gp, code = ctypes.byref(g), ARITH[arith]
    wp = torch.empty(lib.C.cbinfer_geom_prepared_weights_bytes(K, Cin, gp, code), dtype=torch.uint8, device="cuda")
    lib.check(lib.C.cbinfer_geom_prep_weights(conv.weight.data_ptr(), wp.data_ptr(), K, Cin, Hi, Wi, gp, code,
                                              stream()))
    twin = Twin(oracle, conv.weight, conv.bias, geom, TH, True, True)
    rng = np.random.default_rng(4)
    Ckk = Cin * 9
    for t, x in enumerate(frames_for(rng, Cin, Hi, Wi, 4, npdtype(arith))):
        xd = dev(x)
        before = B['out'].clone()
        lib.check(lib.C.cbinfer_cbconv2d_forward_geom(
            xd.data_ptr(), B['state'].data_ptr(), B['out'].data_ptr(), B['bits'].data_ptr(), B['idx'].data_ptr(),
            B['count'].data_ptr(), wp.data_ptr(), conv.bias.data_ptr(), Cin, Hi, Wi, K, gp, TH, 1, 1, 1, 0, Ho * Wo,
            B['ws'].data_ptr(), code, stream()))
        torch.cuda.synchronize()
        idx, listed, ref = twin.step(x)
        n = int(B['count'].item())
        assert np.array_equal(B['idx'][:n].cpu().numpy(), idx), (arith, t)
        assert t > 0 or 0 < n < Ho * Wo
        assert np.array_equal(bits_of(B['state'].cpu().numpy()), bits_of(twin.state)), (arith, t)
        out = B['out'].cpu().numpy()[0]
        mag = F.conv2d(torch.from_numpy(np.abs(twin.state.astype(np.float64))), conv.weight.detach().cpu().double().abs(),
                       conv.bias.detach().cpu().double().abs(), stride=geom[1], padding=geom[2])[0].numpy()
        err = np.abs(out.astype(np.float64) - ref)[:, listed]
        if arith == "F16":
            bound = 2.0 ** -11 * np.abs(ref) + Ckk * 2.0 ** -23 * mag + 2.0 ** -24
        else:
            bound = (64 if arith == "F32S" else Ckk) * 2.0 ** -24 * mag
        assert np.all(err <= bound[:, listed]), (arith, t, err.max())
        assert np.array_equal(bits_of(out)[:, ~listed], bits_of(before.cpu().numpy()[0])[:, ~listed]), (arith, t)
        assert int(B['ws'][-2048:].ne(0).sum().item()) == 0


@pytest.mark.parametrize("name", ["3x3s2p1", "3x3d2p2"])
def test_exact_f32_switch_reaches_the_general_geometry_path(lib, oracle, name):
    """CBConv2d(..., generalGeometry=True) with exactF32=True on a strided and a dilated layer: the prepared weights and
    the launches are CB_F32's, the layer tracks the twin within the f32 chain's bound (Ckk * 2^-24 * mag per element)
    and the bar of tests/test_gpu_geom.py."""
    import pycbinfer
    geom = GEOMS[name]
    Cin, K, Hi, Wi = 16, 70, 11, 131
    conv = make_conv(geom, Cin, K, True, torch.float32)
    m = pycbinfer.CBConv2d(conv, TH, generalGeometry=True)
    m.exactF32 = True
    m.withReLU = True
    twin = Twin(oracle, conv.weight, conv.bias, geom, TH, False, True)
    rng = np.random.default_rng(12)
    w64, b64 = conv.weight.detach().cpu().double().abs(), conv.bias.detach().cpu().double().abs()
    with torch.no_grad():
        for t, x in enumerate(frames_for(rng, Cin, Hi, Wi, 3, np.float32)):
            xd = dev(x)
            assert m._path(xd, Hi, Wi) == 'geom' and m._arith(xd) == lib.CB_F32
            y = m(xd)
            assert m._wprep[0][0] == 'geom' and m._wprep[0][-1] == lib.CB_F32
            idx, listed, ref = twin.step(x)
            assert np.array_equal(m.lastChangeIndexes().tensor().cpu().numpy(), idx), (name, t)
            mag = F.conv2d(torch.from_numpy(np.abs(twin.state.astype(np.float64))), w64, b64, stride=geom[1],
                           padding=geom[2], dilation=geom[3])[0].numpy()
            err = np.abs(y.cpu().numpy()[0].astype(np.float64) - ref)
            assert np.all(err[:, listed] <= Cin * 9 * 2.0 ** -24 * mag[:, listed]), (name, t, err[:, listed].max())
            assert err[:, listed].max() <= 1e-4, (name, t)      # unit-scale data: the absolute bar applies


def test_worst_figures_are_reported():
    """The worst err / mag of each arithmetic over the tests above (DESIGN 6 records them): measurements, not bars."""
    for arith, rel in sorted(WORST.items()):
        print("worst err / mag, %s: %.3g = %.2f * 2^-24" % (arith, rel, rel * 2.0 ** 24))
