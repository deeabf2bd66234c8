"""-m gpu: the list contraction (cb_conv.hip) through the raw C ABI, one case per cell of the form x regime table of
tests/listconv_cases.py, against double-precision math: oracle.genXMatrix patches at the listed pixels times the
weights in float64, plus the bias.  Every listed pixel and every output channel is compared.

Bars: F32 / F32S |err| <= 1e-4; F32S additionally err <= 64 * 2^-24 * sum|a||b| per element (only this bound sees a
dropped low bf16 term) -- on a bias-free launch exactly that, with a bias the bias is one more term of the sum;
accumulate forms 1e-4 * max(1, max|want|); F16: 2 fp16 ulp of the largest |output| (half_tol of test_gpu_ops.py).
"""
import functools
import zlib

import numpy as np
import pytest
import torch

from listconv_cases import (ACCUMULATE_IDS, ARITH, CASE_BY_ID, CASES, CLEAR_BITS_IDS, OUT_OF_MAP_IDS, case_form,
                            case_pixels, cell_of, list_form)
from optest import dev, np_dtype, stream

pytestmark = pytest.mark.gpu

FP32_TOL = 1e-4
HALF_ULPS = 2.0
CB_OK, CB_ERR_BADARG, CB_ERR_UNSUPPORTED = 0, -1, -2
FILL = 77.0
TAIL = 37            # garbage entries behind the list in the device-count launches
SEAM_INFO = 1020     # {SK, tiles, N} left in the workspace header by a launch whose slices meet in a second one


def half_tol(ref):
    m = float(np.abs(np.asarray(ref, dtype=np.float64)).max())
    return HALF_ULPS * 2.0 ** (np.floor(np.log2(max(m, 2.0 ** -14))) - 10)


@pytest.fixture(scope="module")
def lib():
    from cbinfer_amd._lib import C
    assert torch.cuda.is_available()
    return C


def cus():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def make_tensors(seed, dtype, K, C, kH, kW, H, W):
    """Inputs N(0,1) (F32S: every channel times exp(U(-6, 3))), weights N(0,1)/sqrt(Ckk), bias N(0,1), in the
    arithmetic's storage type."""
    rng = np.random.default_rng(seed)
    inp = rng.standard_normal((1, C, H, W))
    if dtype == "F32S":
        inp = inp * np.exp(rng.uniform(-6, 3, (1, C, 1, 1)))
    w = rng.standard_normal((K, C, kH, kW)) / np.sqrt(C * kH * kW)
    b = rng.standard_normal(K)
    t = np_dtype(dtype)
    return inp.astype(t), w.astype(t), b.astype(t)


def reference(oracle, inp, w, px, filt):
    """[K, N] float64: the patches at px times the weights (no bias), and sum|a||b| of the same products."""
    K = w.shape[0]
    X = oracle.genXMatrix(inp.astype(np.float32), px, filt).astype(np.float64)
    Wm = w.reshape(K, -1).astype(np.float64)
    return (X @ Wm.T).T.copy(), (np.abs(X) @ np.abs(Wm).T).T.copy()


def prep_weights(lib, w, H, W, dtype):
    K, C, kH, kW = w.shape
    code = ARITH[dtype]
    wp = torch.empty(lib.cbinfer_prepared_weights_bytes(K, C, kH, kW, code), dtype=torch.uint8, device="cuda")
    wd = dev(w)
    assert lib.cbinfer_prep_weights(wd.data_ptr(), wp.data_ptr(), K, C, kH, kW, H, W, code, stream()) == CB_OK
    torch.cuda.synchronize()
    return wp


def new_workspace(lib):
    return torch.zeros(lib.cbinfer_conv_workspace_bytes(), dtype=torch.uint8, device="cuda")


def assert_header_at_rest(ws, what):
    """Tickets and arrival counters are back at zero; only the three seam words may hold anything."""
    if ws is None:
        return
    head = ws[:4096].view(torch.int32).clone()
    head[SEAM_INFO:SEAM_INFO + 3] = 0
    nz = torch.nonzero(head).flatten().tolist()
    assert not nz, "%s: workspace header words %s are not at rest" % (what, nz[:8])


def assert_close(got, want, dtype, what, mag=None, scale_tol=False):
    """got, want: [K, N] float64 on the device.  Prints the figure before it asserts."""
    err = (got - want).abs()
    worst = float(err.max()) if err.numel() else 0.0
    if dtype == "F16":
        tol = half_tol(want.cpu().numpy()) if want.numel() else 1.0
    else:
        tol = FP32_TOL * (max(1.0, float(want.abs().max())) if scale_tol and want.numel() else 1.0)
    line = "%s: max |err| %.3g, bar %.3g" % (what, worst, tol)
    if mag is not None and err.numel():
        rel = float((err / (mag + 1e-30)).max())
        line += "; max err / sum|a||b| %.3g of 2^-24, bar 64" % (rel * 2.0 ** 24)
    print(line)
    assert worst <= tol, line
    if mag is not None:
        assert bool((err <= 64 * 2.0 ** -24 * mag + 1e-30).all()), line


def assert_output(out, K, HW, px_t, want, dtype, what, prefill, mag=None, scale_tol=False):
    """Listed pixels within the bar; every other value bit-identical to the prefill (a tensor or a number)."""
    o = out.view(K, HW)
    assert_close(o[:, px_t].double(), want, dtype, what, mag, scale_tol)
    rest = o.clone()
    if torch.is_tensor(prefill):
        exp = prefill.view(K, HW).clone()
        rest[:, px_t] = 0
        exp[:, px_t] = 0
        assert torch.equal(rest, exp), "%s: a value outside the list changed" % what
    else:
        rest[:, px_t] = prefill
        assert bool((rest == prefill).all()), "%s: a value outside the list changed" % what


class Data(object):
    """A case's tensors on the device and its float64 reference; built once and shared by the tests."""

    def __init__(self, lib, oracle, c, taps=None):
        self.c = c
        self.filt = (c.kH, c.kW)
        self.HW = c.H * c.W
        self.px = case_pixels(c)
        inp, w, b = make_tensors(zlib.crc32(c.id.encode()) + 1, c.dtype, c.K, c.C, c.kH, c.kW, c.H, c.W)
        if taps is not None:    # sparse operand: about `taps` non-zero values per patch
            keep = np.random.default_rng(17).random(inp.shape) < taps / float(c.C * c.kH * c.kW)
            inp = inp * keep.astype(inp.dtype)
        y, mag = reference(oracle, inp, w, self.px, self.filt)
        self.y = dev(y)                                                # [K, N] without bias
        self.bias64 = dev(b.astype(np.float64))[:, None]
        self.mag = dev(mag) if c.dtype == "F32S" else None
        self.inp, self.bias = dev(inp), dev(b)
        self.wp = prep_weights(lib, w, c.H, c.W, c.dtype)
        self.px_t = dev(self.px.astype(np.int64))
        self.tdtype = torch.float16 if c.dtype == "F16" else torch.float32


@functools.lru_cache(maxsize=None)
def _data(lib, oracle, cid):
    return Data(lib, oracle, CASE_BY_ID[cid])


def conv_changed(lib, d, out, lst, n, count=None, bias=True, relu=0, accumulate=0, ws=None, clear=None, clear_words=0):
    c = d.c
    st = lib.cbinfer_conv_changed(d.inp.data_ptr(), lst.data_ptr(), n, count.data_ptr() if count is not None else None,
                                  d.wp.data_ptr(), d.bias.data_ptr() if bias else None, out.data_ptr(), c.C, c.H, c.W,
                                  c.K, c.kH, c.kW, relu, accumulate, clear.data_ptr() if clear is not None else None,
                                  clear_words, ws.data_ptr() if ws is not None else None, ARITH[c.dtype], stream())
    torch.cuda.synchronize()
    return st


def assert_claimed_cell(c, n=None, n_host=None):
    f = case_form(c, cus(), n, n_host)
    got = cell_of(c.dtype, f, c.ws)
    assert got == c.cell, ("%s: on a card with %d CUs this shape lands in %s, not in the cell %s it was written for "
                           "(%s)" % (c.id, cus(), got, c.cell, f))
    return f


# ---------------------------------------------------------------------------------------------------------------------
# a. every cell of the table
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c.id for c in CASES])
def test_list_forms(lib, oracle, cid):
    c = CASE_BY_ID[cid]
    f = assert_claimed_cell(c)
    d = _data(lib, oracle, cid)
    N, K, HW = len(d.px), c.K, d.HW
    assert_claimed_cell(c, N, N + TAIL)
    print("cell %s: %s" % (c.cell, {k: f[k] for k in ("MT", "T", "P", "SK", "grid", "items", "xmap", "seam")}))
    ws = new_workspace(lib) if c.ws else None
    lst = dev(d.px)
    garbage = np.full(TAIL, 2 ** 31 - 1, dtype=np.int32)
    garbage[::2] = 3 * HW + 1
    lst_tail = dev(np.concatenate([d.px, garbage]))
    count = dev(np.array([N], dtype=np.int32))
    want_b = d.y + d.bias64
    magb = d.mag + d.bias64.abs() if d.mag is not None else None
    for relu in (0, 1):
        want = want_b.clamp(min=0) if relu else want_b
        for devcount in (False, True):
            for rep in (1, 2):          # the second launch finds the workspace as the first one left it
                out = torch.full((1, K, c.H, c.W), FILL, dtype=d.tdtype, device="cuda")
                if devcount:
                    st = conv_changed(lib, d, out, lst_tail, N + TAIL, count, relu=relu, ws=ws)
                else:
                    st = conv_changed(lib, d, out, lst, N, relu=relu, ws=ws)
                assert st == CB_OK
                what = "%s relu=%d %s launch %d" % (cid, relu, "device count" if devcount else "host count", rep)
                assert_output(out, K, HW, d.px_t, want, c.dtype, what, FILL, magb)
                assert_header_at_rest(ws, what)
                if f["seam"]:           # ties the classifier to the kernel
                    info = ws[:4096].view(torch.int32)[SEAM_INFO:SEAM_INFO + 3].tolist()
                    assert info == [f["SK"], f["T"], N], (what, info, f)
    if c.dtype == "F32S":               # without a bias: the per-element bound exactly as it stands
        out = torch.full((1, K, c.H, c.W), FILL, dtype=d.tdtype, device="cuda")
        assert conv_changed(lib, d, out, lst, N, bias=False, ws=ws) == CB_OK
        assert_output(out, K, HW, d.px_t, d.y, c.dtype, cid + " no bias", FILL, d.mag)


@pytest.mark.parametrize("cid", ["f32s-narrow-split3", "f32s-64-split3", "f32s-64-k130", "f32s-128-seam4",
                                 "f32s-128-shallow", "f32s-256-seam4", "f32s-256-nows"])
def test_f32s_low_terms_on_sparse_operands(lib, oracle, cid):
    """The per-element bound 64 * 2^-24 * sum|a||b| on an input with about one non-zero value per patch (what a
    fine-grained delta looks like).  In a deep dense sum a dropped lo x hi product (2^-17 of ONE product) hides
    behind sum|a||b| of hundreds of terms; here the sum is that one product, at every k position in turn.  An
    honest kernel is off by < 3 * 2^-24 per product plus one rounding per non-zero term; where no tap is
    non-zero the output is exactly zero."""
    c = CASE_BY_ID[cid]
    assert_claimed_cell(c)
    d = Data(lib, oracle, c, taps=1.5)
    N, K = len(d.px), c.K
    terms = float((d.mag > 0).sum()) / d.mag.numel()
    print("%s: %.0f %% of the outputs see a non-zero tap" % (cid, 100 * terms))
    assert 0.3 < terms < 0.95
    ws = new_workspace(lib) if c.ws else None
    out = torch.full((1, K, c.H, c.W), FILL, dtype=d.tdtype, device="cuda")
    assert conv_changed(lib, d, out, dev(d.px), N, bias=False, ws=ws) == CB_OK
    assert_output(out, K, d.HW, d.px_t, d.y, c.dtype, cid + " sparse, no bias", FILL, d.mag)
    assert_header_at_rest(ws, cid)


# ---------------------------------------------------------------------------------------------------------------------
# b. accumulate
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ACCUMULATE_IDS)
def test_list_accumulate(lib, oracle, cid):
    """out0 + conv at the listed pixels: the bias and the ReLU flag handed in must both be ignored."""
    c = CASE_BY_ID[cid]
    f = assert_claimed_cell(c)
    d = _data(lib, oracle, cid)
    N, K, HW = len(d.px), c.K, d.HW
    rng = np.random.default_rng(5)
    out0 = dev(rng.standard_normal((1, K, c.H, c.W)).astype(np_dtype(c.dtype)))
    want = out0.view(K, HW)[:, d.px_t].double() + d.y
    if c.dtype == "F16":
        want = want.half().double()
    ws = new_workspace(lib) if c.ws else None
    lst = dev(d.px)
    for rep in (1, 2):
        out = out0.clone()
        assert conv_changed(lib, d, out, lst, N, relu=1, accumulate=1, ws=ws) == CB_OK
        what = "%s accumulate launch %d" % (cid, rep)
        assert_output(out, K, HW, d.px_t, want, c.dtype, what, out0, scale_tol=True)
        assert_header_at_rest(ws, what)
        if f["seam"]:
            assert ws[:4096].view(torch.int32)[SEAM_INFO:SEAM_INFO + 3].tolist() == [f["SK"], f["T"], N]


# ---------------------------------------------------------------------------------------------------------------------
# c. list entries outside the map
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", OUT_OF_MAP_IDS)
def test_list_out_of_map_entries(lib, oracle, cid):
    """Entries in [HW, 2 HW) -- a propagated list of another resolution -- are dropped: nothing is written through
    them, in the plain epilogue, in the last workgroup's sum and in the second launch."""
    c = CASE_BY_ID[cid]
    d = _data(lib, oracle, cid)
    N, K, HW = len(d.px), c.K, d.HW
    rng = np.random.default_rng(9)
    M = 40
    full = np.concatenate([d.px, HW + rng.choice(HW, M, replace=False).astype(np.int32)])
    order = rng.permutation(N + M)
    full = full[order]
    where = np.empty(N + M, dtype=np.int64)
    where[order] = np.arange(N + M)
    f = list_form(c.dtype, c.K, c.C, c.kH, c.kW, N + M, c.ws, False, "scatter", cus())
    assert (f["SK"] > 1) == (c.cell[2] in ("lastwg", "seam", "seam>8")) and f["form"] == c.cell[1], f
    ws = new_workspace(lib) if c.ws else None
    # (one plane of padding behind the output: a write through an entry of the last plane would land there)
    buf = torch.full(((K + 1) * HW,), FILL, dtype=d.tdtype, device="cuda")
    out = buf[:K * HW]
    assert conv_changed(lib, d, out, dev(full), N + M, ws=ws) == CB_OK
    assert_output(out, K, HW, d.px_t, d.y + d.bias64, c.dtype, cid + " with out-of-map entries", FILL)
    assert int((buf != FILL).sum()) == K * N
    assert_header_at_rest(ws, cid)


# ---------------------------------------------------------------------------------------------------------------------
# d. the change mask the launch zeroes for the next frame
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", CLEAR_BITS_IDS)
def test_list_clear_bits(lib, oracle, cid):
    c = CASE_BY_ID[cid]
    d = _data(lib, oracle, cid)
    N, K, HW = len(d.px), c.K, d.HW
    words, guard = 3001, 11
    bits = torch.full((words + guard,), -1, dtype=torch.int64, device="cuda")
    ws = new_workspace(lib) if c.ws else None
    out = torch.full((1, K, c.H, c.W), FILL, dtype=d.tdtype, device="cuda")
    assert conv_changed(lib, d, out, dev(d.px), N, ws=ws, clear=bits, clear_words=words) == CB_OK
    assert int((bits[:words] != 0).sum()) == 0
    assert bool((bits[words:] == -1).all())
    assert_output(out, K, HW, d.px_t, d.y + d.bias64, c.dtype, cid + " with clearBits", FILL)


# ---------------------------------------------------------------------------------------------------------------------
# e.-g. the launches that compact the frame's change mask themselves
# ---------------------------------------------------------------------------------------------------------------------
def pack_mask(m, wpr):
    """bool [H, W] -> int64 [H * wpr]: bit x % 64 of word row * wpr + x / 64."""
    H, W = m.shape
    p = np.zeros((H, wpr * 64), dtype=np.uint8)
    p[:, :W] = m
    return np.packbits(p.reshape(H, wpr, 64), axis=-1, bitorder="little").view("<u8").reshape(-1).view(np.int64)


class Frame(object):
    """The buffers of one self-compacting layer: [mask 0][mask 1]{parity, done, pad}[copy of the frame's mask]."""

    def __init__(self, lib, H, W):
        self.H, self.W = H, W
        self.words = lib.cbinfer_mask_words(H, W)
        self.wpr = lib.cbinfer_mask_words_per_row(W)
        assert self.words == H * self.wpr
        nbytes = lib.cbinfer_frame_mask_bytes(H, W)
        self.copy_at = lib.cbinfer_frame_mask_copy_offset(H, W) // 8
        assert nbytes == 8 * (self.copy_at + self.words) and self.copy_at == 2 * self.words + 2
        self.buf = torch.zeros(nbytes // 8, dtype=torch.int64, device="cuda")
        self.idx = torch.full((H * W,), -1, dtype=torch.int32, device="cuda")
        self.count = torch.full((1,), 77, dtype=torch.int32, device="cuda")

    def ctl(self):
        return self.buf[2 * self.words:2 * self.words + 1].view(torch.int32).tolist()      # [parity, done]

    def mask(self, which):
        return self.buf[which * self.words:(which + 1) * self.words]

    def copy(self):
        return self.buf[self.copy_at:self.copy_at + self.words]

    def write(self, m):
        """As the detection would: into the mask the parity selects, which the protocol keeps clean."""
        par = self.ctl()[0]
        assert par in (0, 1) and int((self.mask(par) != 0).sum()) == 0
        packed = dev(pack_mask(m, self.wpr))
        self.mask(par).copy_(packed)
        return par, packed

    def check(self, par, packed, m, what):
        n = int(m.sum())
        assert self.count.tolist() == [n], what
        px = np.flatnonzero(m.reshape(-1)).astype(np.int32)
        assert torch.equal(self.idx[:n], dev(px)), what + ": listOut"
        assert bool((self.idx[n:] == -1).all()), what + ": listOut past the count"
        assert int((self.mask(par ^ 1) != 0).sum()) == 0, what + ": the other mask"
        assert torch.equal(self.mask(par), packed), what + ": the frame's mask"
        assert torch.equal(self.copy(), packed), what + ": the mask copy"
        assert self.ctl() == [par ^ 1 if n else par, 0], what + ": parity / done"
        return px


MASK_LAYERS = {
    # id: dtype, form, workspace, K, C, filter, H, W, density of the first frame
    "f32-narrow-w65": ("F32", "narrow", False, 8, 3, (3, 3), 33, 65, 0.05),
    "f32-narrow-585w-ws": ("F32", "narrow", True, 8, 2, (3, 3), 65, 520, 0.05),
    "f32-64-w65-ws": ("F32", "64x64", True, 64, 3, (3, 3), 33, 65, 0.05),
    "f32-64-585w": ("F32", "64x64", False, 40, 2, (3, 3), 65, 520, 0.05),
    "f32s-128-w65-ws": ("F32S", "128x128", True, 128, 3, (3, 3), 33, 65, 0.05),
    "f32s-128-w65-seam": ("F32S", "128x128", True, 128, 8, (7, 7), 33, 65, 0.05),
    "f32s-128-1080w": ("F32S", "128x128", False, 128, 1, (3, 3), 40, 1700, 0.05),
    "f32s-256-1080w-ws": ("F32S", "256x64", True, 256, 1, (3, 3), 40, 1700, 0.05),
    "f32s-256-w65": ("F32S", "256x64", False, 256, 3, (3, 3), 33, 65, 0.05),
    "f16-64-w65-ws": ("F16", "64x64", True, 64, 3, (3, 3), 33, 65, 0.05),
    "f16-64-585w": ("F16", "64x64", False, 64, 3, (3, 3), 65, 521, 0.05),
    "f32-narrow-4096w-ws": ("F32", "narrow", True, 8, 1, (3, 3), 64, 4096, 0.004),
}


class MaskLayer(object):
    """Tensors and the float64 reference at EVERY pixel of a layer driven from its frame mask."""

    def __init__(self, lib, oracle, lid, bias=True):
        (self.dtype, self.form, self.has_ws, self.K, self.C, self.filt, self.H, self.W, self.frac) = MASK_LAYERS[lid]
        K, C, H, W = self.K, self.C, self.H, self.W
        self.HW = H * W
        f = list_form(self.dtype, K, C, self.filt[0], self.filt[1], 1, self.has_ws, True, "scatter", cus(), self.HW)
        assert f["form"] == self.form, f
        self.NT = f["NT"]
        inp, w, b = make_tensors(zlib.crc32(lid.encode()) + 1, self.dtype, K, C, self.filt[0], self.filt[1], H, W)
        y, mag = reference(oracle, inp, w, np.arange(self.HW, dtype=np.int32), self.filt)
        self.y, self.bias64 = dev(y), dev(b.astype(np.float64))[:, None]
        self.mag = dev(mag) if self.dtype == "F32S" else None
        self.inp, self.bias = dev(inp), dev(b)
        self.wp = prep_weights(lib, w, H, W, self.dtype)
        self.tdtype = torch.float16 if self.dtype == "F16" else torch.float32

    def form_at(self, n):
        return list_form(self.dtype, self.K, self.C, self.filt[0], self.filt[1], n, self.has_ws, True, "scatter",
                         cus(), self.HW)


@functools.lru_cache(maxsize=None)
def _layer(lib, oracle, lid):
    return MaskLayer(lib, oracle, lid)


def conv_from_mask(lib, L, fr, out, ws, relu=0, upstream=None):
    args = (L.inp.data_ptr(), fr.buf.data_ptr(), fr.idx.data_ptr(), fr.count.data_ptr(), L.wp.data_ptr(),
            L.bias.data_ptr(), out.data_ptr(), L.C, L.H, L.W, L.K, L.filt[0], L.filt[1], relu,
            ws.data_ptr() if ws is not None else None, ARITH[L.dtype], stream())
    if upstream is None:
        st = lib.cbinfer_conv_changed_from_mask(*args)
    else:
        st = lib.cbinfer_conv_changed_from_mask_after(upstream.data_ptr(), *args)
    torch.cuda.synchronize()
    return st


def three_frames(H, W, frac, seed):
    rng = np.random.default_rng(seed)
    return [("random", rng.random((H, W)) < frac), ("empty", np.zeros((H, W), dtype=bool)),
            ("full", np.ones((H, W), dtype=bool))]


@pytest.mark.parametrize("lid", list(MASK_LAYERS))
def test_from_mask_protocol(lib, oracle, lid):
    """Three consecutive frames on one frame-mask buffer: a random mask, an empty one, a full one."""
    L = _layer(lib, oracle, lid)
    fr = Frame(lib, L.H, L.W)
    if "585w" in lid or "1080w" in lid:
        assert L.NT < fr.words <= 2 * L.NT          # a thread owns two words of the prefix scan
    if "4096w" in lid:
        assert fr.words == lib.cbinfer_frame_mask_max_words() == 4096
    if "w65" in lid:
        assert fr.wpr == 2
    ws = new_workspace(lib) if L.has_ws else None
    magb = L.mag + L.bias64.abs() if L.mag is not None else None
    regimes = []
    for relu, (name, m) in zip((0, 1, 1), three_frames(L.H, L.W, L.frac, 3)):
        what = "%s frame '%s'" % (lid, name)
        par, packed = fr.write(m)
        fr.idx.fill_(-1)
        fr.count.fill_(77)
        out = torch.full((1, L.K, L.H, L.W), FILL, dtype=L.tdtype, device="cuda")
        assert conv_from_mask(lib, L, fr, out, ws, relu=relu) == CB_OK
        px = fr.check(par, packed, m, what)
        px_t = dev(px.astype(np.int64))
        want = L.y[:, px_t] + L.bias64
        assert_output(out, L.K, L.HW, px_t, want.clamp(min=0) if relu else want, L.dtype, what, FILL,
                      magb[:, px_t] if magb is not None else None)
        assert_header_at_rest(ws, what)
        f = L.form_at(len(px))
        regimes.append((name, len(px), f["SK"], f["items"] > f["grid"]))
        if f["seam"] and len(px):
            assert ws[:4096].view(torch.int32)[SEAM_INFO:SEAM_INFO + 3].tolist() == [f["SK"], f["T"], len(px)]
    print("%s: (frame, n, SK, multi_item) %s" % (lid, regimes))
    if lid == "f32s-128-w65-seam":
        assert regimes[0][2] > 1 and regimes[2][2] > 1


def test_from_mask_refuses_4097_words(lib):
    H, W, K, C = 4097, 1, 8, 1
    assert lib.cbinfer_mask_words(H, W) == 4097
    buf = torch.zeros(lib.cbinfer_frame_mask_bytes(H, W) // 8, dtype=torch.int64, device="cuda")
    buf[:H] = 1
    before = buf.clone()
    idx = torch.full((H * W,), -1, dtype=torch.int32, device="cuda")
    count = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    inp = torch.ones(1, C, H, W, device="cuda")
    out = torch.full((1, K, H, W), FILL, device="cuda")
    wp = prep_weights(lib, np.ones((K, C, 3, 3), dtype=np.float32), H, W, "F32")
    for code in (0, 2, 1):
        st = lib.cbinfer_conv_changed_from_mask(inp.data_ptr(), buf.data_ptr(), idx.data_ptr(), count.data_ptr(),
                                                wp.data_ptr(), None, out.data_ptr(), C, H, W, K, 3, 3, 0, None, code,
                                                stream())
        torch.cuda.synchronize()
        assert st == CB_ERR_UNSUPPORTED
    assert torch.equal(buf, before) and count.tolist() == [77] and bool((out == FILL).all())
    assert bool((idx == -1).all())


@pytest.mark.parametrize("lid", ["f32-64-w65-ws", "f32s-128-w65-seam", "f16-64-w65-ws"])
def test_from_mask_after_idle(lib, oracle, lid):
    """An upstream count of zero: the frame does not exist for this layer.  Any other count: the plain entry point."""
    L = _layer(lib, oracle, lid)
    m = three_frames(L.H, L.W, L.frac, 4)[0][1]
    fr = Frame(lib, L.H, L.W)
    fr.write(m)
    ws = new_workspace(lib)
    out = torch.full((1, L.K, L.H, L.W), FILL, dtype=L.tdtype, device="cuda")
    snap = [t.clone() for t in (fr.buf, fr.idx, out, ws[:4096])]
    up = dev(np.array([0], dtype=np.int32))
    assert conv_from_mask(lib, L, fr, out, ws, upstream=up) == CB_OK
    assert fr.count.tolist() == [0]
    for a, b in zip(snap, (fr.buf, fr.idx, out, ws[:4096])):
        assert torch.equal(a, b)
    # upstream count 5: bit for bit what the plain entry point does from the same state
    up.fill_(5)
    fr2 = Frame(lib, L.H, L.W)
    fr2.write(m)
    ws2 = new_workspace(lib)
    out2 = out.clone()
    assert conv_from_mask(lib, L, fr, out, ws, relu=1, upstream=up) == CB_OK
    assert conv_from_mask(lib, L, fr2, out2, ws2, relu=1) == CB_OK
    assert fr.count.tolist() == [int(m.sum())]
    for a, b in ((fr.buf, fr2.buf), (fr.idx, fr2.idx), (fr.count, fr2.count), (out, out2), (ws[:4096], ws2[:4096])):
        assert torch.equal(a, b)
    assert_header_at_rest(ws, lid)


@pytest.mark.parametrize("lid", ["f32-64-w65-ws", "f32s-128-w65-seam", "f16-64-w65-ws"])
def test_from_mask_after_idle_empties_the_mask_copy(lib, oracle, lid):
    """The frame before left its mask in the copy behind the two masks.  An upstream count of zero goes out as a count of
    zero AND an empty copy -- the copy is what a module behind the layer is handed as THIS frame's change mask -- and
    touches nothing else: masks, control words, list, output, workspace."""
    L = _layer(lib, oracle, lid)
    m = three_frames(L.H, L.W, L.frac, 4)[0][1]
    fr = Frame(lib, L.H, L.W)
    fr.copy().copy_(dev(pack_mask(m, fr.wpr)))
    assert int((fr.copy() != 0).sum()) > 0
    ws = new_workspace(lib)
    out = torch.full((1, L.K, L.H, L.W), FILL, dtype=L.tdtype, device="cuda")
    snap = [t.clone() for t in (fr.buf[:fr.copy_at], fr.idx, out, ws[:4096])]
    assert conv_from_mask(lib, L, fr, out, ws, upstream=dev(np.array([0], dtype=np.int32))) == CB_OK
    assert fr.count.tolist() == [0] and int((fr.copy() != 0).sum()) == 0
    for a, b in zip(snap, (fr.buf[:fr.copy_at], fr.idx, out, ws[:4096])):
        assert torch.equal(a, b)


@pytest.mark.parametrize("lid,dtype,K", [("f32-64-acc", "F32", 64), ("f32s-128-acc-seam", "F32S", 128),
                                         ("f32s-256-acc-seam", "F32S", 256)])
def test_accumulate_from_mask(lib, oracle, lid, dtype, K):
    """out += conv(W, delta) at the masked pixels, relu(out) kept in a second plane set; same protocol."""
    C, filt, H, W = 8, (7, 7), 33, 65
    HW = H * W
    delta, w, _ = make_tensors(zlib.crc32(lid.encode()), dtype, K, C, 7, 7, H, W)
    y, _ = reference(oracle, delta, w, np.arange(HW, dtype=np.int32), filt)
    y = dev(y)
    wp = prep_weights(lib, w, H, W, dtype)
    delta_t = dev(delta)
    out0 = dev(np.random.default_rng(6).standard_normal((1, K, H, W)).astype(np.float32))
    fr = Frame(lib, H, W)
    ws = new_workspace(lib)
    for name, m in three_frames(H, W, 0.05, 8):
        what = "%s frame '%s'" % (lid, name)
        par, packed = fr.write(m)
        fr.idx.fill_(-1)
        fr.count.fill_(77)
        out = out0.clone()
        relu_out = torch.full((1, K, H, W), FILL, device="cuda")
        st = lib.cbinfer_conv_accumulate_from_mask(delta_t.data_ptr(), fr.buf.data_ptr(), fr.idx.data_ptr(),
                                                   fr.count.data_ptr(), wp.data_ptr(), out.data_ptr(),
                                                   relu_out.data_ptr(), C, H, W, K, 7, 7, ws.data_ptr(), ARITH[dtype],
                                                   stream())
        torch.cuda.synchronize()
        assert st == CB_OK
        px = fr.check(par, packed, m, what)
        px_t = dev(px.astype(np.int64))
        want = out0.view(K, HW)[:, px_t].double() + y[:, px_t]
        assert_output(out, K, HW, px_t, want, dtype, what, out0, scale_tol=True)
        ro = relu_out.view(K, HW)
        assert torch.equal(ro[:, px_t], out.view(K, HW)[:, px_t].clamp(min=0)), what + ": reluOut"
        rest = ro.clone()
        rest[:, px_t] = FILL
        assert bool((rest == FILL).all()), what + ": reluOut outside the mask"
        assert_header_at_rest(ws, what)
        f = list_form(dtype, K, C, 7, 7, len(px), True, True, "accumulate", cus(), HW)
        print("%s: n %d SK %d seam %s" % (what, len(px), f["SK"], f["seam"]))
        if len(px):
            assert f["SK"] > 1 and f["seam"] == (dtype == "F32S")
        if f["seam"] and len(px):
            assert ws[:4096].view(torch.int32)[SEAM_INFO:SEAM_INFO + 3].tolist() == [f["SK"], f["T"], len(px)]


# ---------------------------------------------------------------------------------------------------------------------
# h. what the entry points refuse
# ---------------------------------------------------------------------------------------------------------------------
def test_list_argument_contract(lib, oracle):
    d = _data(lib, oracle, "f32s-128-n1")
    c = d.c
    N = 16
    # the bf16x3 arithmetic has no matrix mode
    X = torch.ones(N, c.C * 9, device="cuda")
    Y = torch.full((N, c.K), FILL, device="cuda")
    st = lib.cbinfer_matrix_mult(X.data_ptr(), d.wp.data_ptr(), None, Y.data_ptr(), N, None, c.C * 9, c.K, 0,
                                 ARITH["F32S"], stream())
    torch.cuda.synchronize()
    assert st in (CB_ERR_UNSUPPORTED, CB_ERR_BADARG) and bool((Y == FILL).all())
    # fp16 has no fine-grained frame: no accumulate form behind a frame mask
    fr = Frame(lib, c.H, c.W)
    fr.write(np.ones((c.H, c.W), dtype=bool))
    before = fr.buf.clone()
    out = torch.full((1, c.K, c.H, c.W), FILL, device="cuda")
    st = lib.cbinfer_conv_accumulate_from_mask(d.inp.data_ptr(), fr.buf.data_ptr(), fr.idx.data_ptr(),
                                               fr.count.data_ptr(), d.wp.data_ptr(), out.data_ptr(), None, c.C, c.H,
                                               c.W, c.K, 3, 3, None, ARITH["F16"], stream())
    torch.cuda.synchronize()
    assert st == CB_ERR_BADARG
    assert torch.equal(fr.buf, before) and fr.count.tolist() == [77] and bool((out == FILL).all())
    # an empty list is no work and no error
    ws = new_workspace(lib)
    lst = dev(np.zeros(4, dtype=np.int32))
    bits = torch.full((8,), -1, dtype=torch.int64, device="cuda")
    for acc in (0, 1):
        assert conv_changed(lib, d, out, lst, 0, relu=1, accumulate=acc, ws=ws, clear=bits, clear_words=8) == CB_OK
    assert bool((out == FILL).all()) and int(ws.view(torch.int32).abs().sum()) == 0
    # ... also when only the device count says so
    count = dev(np.array([0], dtype=np.int32))
    assert conv_changed(lib, d, out, lst, 4, count, relu=1, ws=ws) == CB_OK
    assert bool((out == FILL).all())
    assert_header_at_rest(ws, "device count 0")
    # null pointers and unknown arithmetic codes
    assert lib.cbinfer_conv_changed(None, lst.data_ptr(), 4, None, d.wp.data_ptr(), None, out.data_ptr(), c.C, c.H,
                                    c.W, c.K, 3, 3, 0, 0, None, 0, None, 0, stream()) == CB_ERR_BADARG
    assert lib.cbinfer_conv_changed(d.inp.data_ptr(), lst.data_ptr(), 4, None, d.wp.data_ptr(), None, out.data_ptr(),
                                    c.C, c.H, c.W, c.K, 3, 3, 0, 0, None, 0, None, 7, stream()) == CB_ERR_BADARG
