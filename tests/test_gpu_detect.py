"""-m gpu tests of the front half of a frame against the rules of tests/detect_cases.py (validated on the CPU by
tests/test_host_detect.py), bit for bit:

  * cb_detect_kernel<T, BITS, POOL> over the cell table dtype x form x channel class x update mode -- byte map, bit mask,
    frame masks of either parity, the `_after` form, the batched form, the pooled forms --, on data where every channel
    decides a pixel alone and a palette of ties, roundings, NaN, infinities, signed zeros and subnormals decides one each;
  * cb_compact_kernel / cb_bytes_to_bits_kernel, cb_propagate_kernel, cb_maxpool_kernel, cb_pool_indexes_kernel,
    cb_dilate_indexes_kernel, cb_detect_fg_kernel, cb_detect_fg_frame_kernel; cb_update_fg_kernel against float64
    within a derived bar (the order of its atomics is unspecified);
  * the refusals: a refused call leaves every buffer as it was.

Every buffer a launch writes carries a guard behind its last element.  Where the reference's own kernels were built
(oracle/_ref) the byte-map cases are also compared with them -- in addition, never instead."""
import ctypes
import zlib

import numpy as np
import pytest
import torch

import detect_cases as dc
import refgpu
from detect_cases import CASES, F16, F32
from optest import gpu_lib as lib, raw      # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

IDS = [c.id for c in CASES]
GUARD = 64


def dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a).cuda()


def host(t):
    return t.cpu().numpy()


class Guarded(object):
    """A device copy of an array with GUARD sentinel elements behind it."""

    def __init__(self, a, sentinel=93):
        a = np.ascontiguousarray(a)
        if a.dtype == np.uint64:
            a = a.view(np.int64)
        self.n, self.shape = a.size, a.shape
        self.sentinel = np.full(GUARD, sentinel, dtype=a.dtype)
        self.t = torch.from_numpy(np.concatenate([a.reshape(-1), self.sentinel])).cuda()

    def ptr(self):
        return self.t.data_ptr()

    def get(self):
        a = host(self.t)
        assert np.array_equal(a[self.n:].view(np.uint8), self.sentinel.view(np.uint8)), "written behind the buffer's end"
        return a[:self.n].reshape(self.shape)


def ptrs(tensors):
    return (ctypes.c_void_p * len(tensors))(*tensors)


class Frame(object):
    """A frame mask buffer: two masks with bits set beforehand, the control words with the given parity, noise behind."""

    def __init__(self, lib, H, W, parity, key):
        rng = np.random.default_rng(zlib.crc32(repr(key).encode()))
        self.H, self.W, self.parity = H, W, parity
        self.nw = int(lib.C.cbinfer_mask_words(H, W))
        total = int(lib.C.cbinfer_frame_mask_bytes(H, W)) // 8
        assert total >= 2 * self.nw + 2
        self.before = rng.integers(0, 2 ** 62, total).astype(np.int64)
        self.pre = [rng.random((H, W)) < 0.04 for _ in range(2)]
        for k in (0, 1):
            self.before[k * self.nw:(k + 1) * self.nw] = dc.pack(self.pre[k]).view(np.int64)
        self.before[2 * self.nw:2 * self.nw + 1].view(np.int32)[:] = (parity, 0)
        self.g = Guarded(self.before)

    def check(self, want, tag):
        """The selected mask: the bits set before and the dilated changes, nothing beyond W; every other word as it was."""
        after = self.g.get()
        k = self.parity
        sel = dc.unpack_mask(after[k * self.nw:(k + 1) * self.nw], self.H, self.W)
        assert np.array_equal(sel[:, :self.W], self.pre[k] | want), tag
        assert not sel[:, self.W:].any(), tag
        rest = np.ones(after.size, dtype=bool)
        rest[k * self.nw:(k + 1) * self.nw] = False
        assert np.array_equal(after[rest], self.before[rest]), tag

    def untouched(self, tag):
        assert np.array_equal(self.g.get(), self.before), tag


def filt_half(case):
    return case.kH // 2, case.kW // 2


def launch_bits(lib, case, x, state, words, mode=None):
    kHH, kWH = filt_half(case)
    lib.check(lib.C.cbinfer_change_detection_bits(x.data_ptr(), state.ptr(), words.ptr(), case.W, case.H, case.C, kHH, kWH,
                                                  case.th, case.mode if mode is None else mode, dc.CODE[case.dtype], None))


def check_words(words, want, H, W, tag):
    got = dc.unpack_mask(words, H, W)
    assert np.array_equal(got[:, :W], want), tag
    assert not got[:, W:].any(), tag


def check_state(state, want, tag):
    assert np.array_equal(dc.bits(state.get()), dc.bits(want)), tag


# ---------------------------------------------------------------------------------------------------------------------
# cb_detect_kernel: the cell table
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_detection_case(lib, case):
    C_ = lib.C
    H, W, C, th, mode = case.H, case.W, case.C, case.th, case.mode
    kHH, kWH = filt_half(case)
    code = dc.CODE[case.dtype]
    nw = int(C_.cbinfer_mask_words(H, W))
    nSeq = int(case.variant) if case.form == "batched" else 1
    data = [dc.make(case, q) for q in range(nSeq)]
    want = [dc.expect(case, d) for d in data]      # (raw, dilated mask, state afterwards)
    d, (raw, mask, after) = data[0], want[0]
    state = Guarded(d["state"])

    if case.form == "map":
        x = dev(d["inp"])
        cmap = Guarded(np.full((H, W), 7, dtype=np.int8))
        lib.check(C_.cbinfer_change_detection(x.data_ptr(), state.ptr(), cmap.ptr(), W, H, C, kHH, kWH, th, mode, code, None))
        assert np.array_equal(cmap.get(), mask.astype(np.int8))
        check_state(state, after, "state")
        if refgpu.available() and case.dtype == F32 and mode < 2:      # the reference's own kernel, in addition
            prev = dev(d["state"])
            ref = refgpu.changeDetection(x, prev, (case.kH, case.kW), th, update=bool(mode))
            assert np.array_equal(host(ref), mask.astype(np.int8)), "reference kernel vs rule: mask"
            assert np.array_equal(dc.bits(host(prev)), dc.bits(after)), "reference kernel vs rule: state"

    elif case.form == "bits":
        x = dev(d["inp"])
        words = Guarded(np.zeros(nw, dtype=np.uint64))
        launch_bits(lib, case, x, state, words)
        check_words(words.get(), mask, H, W, "mask")
        check_state(state, after, "state")

    elif case.form in ("frame0", "frame1"):
        x = dev(d["inp"])
        fr = Frame(lib, H, W, int(case.form[-1]), case.id)
        lib.check(C_.cbinfer_change_detection_frame(x.data_ptr(), state.ptr(), fr.g.ptr(), W, H, C, kHH, kWH, th, mode, code,
                                                    None))
        fr.check(mask, "frame")
        check_state(state, after, "state")

    elif case.form == "after":
        x = dev(d["inp"])
        # upstream count 0: the launch is over at once -- state and both masks untouched although the input differs
        assert (dc.bits(d["inp"]) != dc.bits(d["state"])).any()
        fr = Frame(lib, H, W, C & 1, case.id)
        count = dev(np.array([0], dtype=np.int32))
        lib.check(C_.cbinfer_change_detection_frame_after(count.data_ptr(), x.data_ptr(), state.ptr(), fr.g.ptr(), W, H, C, kHH,
                                                          kWH, th, mode, code, None))
        fr.untouched("count 0")
        check_state(state, d["state"], "count 0")
        # a non-zero count, and no count at all: the plain result
        for tag, cnt in (("count 5", dev(np.array([5], dtype=np.int32))), ("no count", None)):
            fr, state = Frame(lib, H, W, (C & 1) ^ (cnt is None), (case.id, tag)), Guarded(d["state"])
            lib.check(C_.cbinfer_change_detection_frame_after(cnt.data_ptr() if cnt is not None else None, x.data_ptr(),
                                                              state.ptr(), fr.g.ptr(), W, H, C, kHH, kWH, th, mode, code, None))
            fr.check(mask, tag)
            check_state(state, after, tag)

    elif case.form == "batched":
        xs = [dev(dq["inp"]) for dq in data]
        states = [Guarded(dq["state"]) for dq in data]
        words = [Guarded(np.zeros(nw, dtype=np.uint64)) for _ in data]
        lib.check(C_.cbinfer_change_detection_bits_batched(ptrs([t.data_ptr() for t in xs]), ptrs([s.ptr() for s in states]),
                                                           ptrs([w.ptr() for w in words]), nSeq, W, H, C, kHH, kWH, th, mode,
                                                           None))
        assert nSeq in (2, C_.cbinfer_split_max_sequences())
        for q in range(nSeq):      # each sequence: its own data, against the rule and against a launch of its own
            check_words(words[q].get(), want[q][1], H, W, q)
            check_state(states[q], want[q][2], q)
            s1, w1 = Guarded(data[q]["state"]), Guarded(np.zeros(nw, dtype=np.uint64))
            launch_bits(lib, case, xs[q], s1, w1)
            assert np.array_equal(w1.get(), words[q].get()) and np.array_equal(dc.bits(s1.get()), dc.bits(states[q].get())), q
        assert len({zlib.crc32(dq["inp"].tobytes()) for dq in data}) == nSeq

    else:      # the pooled forms
        pH, pW = dc.pooled_size(case)
        pre = dev(d["pre"])
        if case.form == "bits_pooled":
            prod = dev(d["prod"]) if d["prod"] is not None else None
            words = Guarded(np.zeros(nw, dtype=np.uint64))
            lib.check(C_.cbinfer_change_detection_bits_pooled(pre.data_ptr(), pH, pW, prod.data_ptr() if prod is not None else None,
                                                              state.ptr(), words.ptr(), W, H, C, kHH, kWH, th, code, None))
            check_words(words.get(), mask, H, W, "mask")
        else:
            fr = Frame(lib, H, W, C & 1, case.id)
            lib.check(C_.cbinfer_change_detection_frame_pooled(pre.data_ptr(), pH, pW, state.ptr(), fr.g.ptr(), W, H, C, kHH, kWH,
                                                               th, code, None))
            fr.check(mask, "frame")
        check_state(state, after, "state")


# ---------------------------------------------------------------------------------------------------------------------
# the per-value frame detection over the channel classes
# ---------------------------------------------------------------------------------------------------------------------
FG_CASES = [c for c in CASES if c.form == "bits" and c.dtype == F32 and c.mode < 2]


@pytest.mark.parametrize("case", FG_CASES, ids=[c.id for c in FG_CASES])
def test_per_value_frame_detection(lib, case):
    """cbinfer_change_detection_fg_frame (either parity) and _fg_bits on the bit-mask cases' data (every channel decides a
    pixel, the palette): delta for EVERY value, prev refreshed where the difference is not zero (refresh = the case's mode),
    the pixels with a changed value dilated into the mask."""
    C_ = lib.C
    H, W, C, th, refresh = case.H, case.W, case.C, case.th, case.mode
    kHH, kWH = filt_half(case)
    d = dc.make(case)
    delta, pred, new = dc.fg_rule(d["inp"], d["state"], th, refresh)
    mask = dc.dilate(pred.any(axis=0), kHH, kWH)
    assert np.array_equal(pred.any(axis=0), dc.changed(d["inp"], d["state"], th))
    x = dev(d["inp"])
    nw = int(C_.cbinfer_mask_words(H, W))
    for form in ("frame0", "frame1", "bits"):
        prev, dl = Guarded(d["state"]), Guarded(np.full((C, H, W), 7, dtype=np.float32))
        if form == "bits":
            words = Guarded(np.zeros(nw, dtype=np.uint64))
            lib.check(C_.cbinfer_change_detection_fg_bits(x.data_ptr(), prev.ptr(), dl.ptr(), words.ptr(), W, H, C, kHH, kWH, th,
                                                          refresh, None))
            check_words(words.get(), mask, H, W, form)
        else:
            fr = Frame(lib, H, W, int(form[-1]), (case.id, form))
            lib.check(C_.cbinfer_change_detection_fg_frame(x.data_ptr(), prev.ptr(), dl.ptr(), fr.g.ptr(), W, H, C, kHH, kWH, th,
                                                           refresh, None))
            fr.check(mask, form)
        assert np.array_equal(dc.bits(dl.get()), dc.bits(delta)), form
        assert np.array_equal(dc.bits(prev.get()), dc.bits(new)), form


def test_per_value_detection(lib):
    C_ = lib.C
    inp, prev, planted = dc.fg_data()
    delta, pred, _ = dc.fg_rule(inp, prev, dc.FG_TH, 0)
    fill = np.random.default_rng(5).standard_normal(dc.FG_NUMVALS).astype(np.float32)
    x, p = dev(inp), Guarded(prev)
    for zero in (0, 1):
        diffs, cmap = Guarded(fill), Guarded(np.full(dc.FG_NUMVALS, 7, dtype=np.int8))
        lib.check(C_.cbinfer_change_detection_fg(x.data_ptr(), p.ptr(), diffs.ptr(), cmap.ptr(), dc.FG_NUMVALS, dc.FG_TH, zero,
                                                 None))
        assert np.array_equal(cmap.get(), pred.astype(np.int8)), zero
        want = delta if zero else np.where(pred, delta, fill)      # zeroUnchanged = 0 keeps the pre-fill elsewhere
        assert np.array_equal(dc.bits(diffs.get()), dc.bits(want)), zero
    assert np.array_equal(dc.bits(p.get()), dc.bits(prev))


@pytest.mark.parametrize("shape", dc.UPDATE_FG_SHAPES)
def test_per_value_scatter_against_float64(lib, shape):
    """cbinfer_update_output_fg (int64 coordinates) and _fg_list (int32, a device count below the capacity): per element
    within (n + 2) 2^-24 (|out0| + sum |w||d|) of float64 -- see detect_cases.update_fg_bar."""
    C_ = lib.C
    K, C, H, W, kH, kW = shape
    diffs, weight, out0, coords = dc.update_fg_data(*shape)
    dd, wd = dev(diffs), dev(weight)
    want, mag, n = dc.update_fg_rule(diffs, weight, out0, coords)
    out, c64, c32 = Guarded(out0), dev(coords), dev(coords.astype(np.int32))
    lib.check(C_.cbinfer_update_output_fg(dd.data_ptr(), wd.data_ptr(), out.ptr(), c64.data_ptr(), K, C, H, W, kH, kW,
                                          len(coords), None))
    err = np.abs(out.get().astype(np.float64) - want)
    assert (err <= dc.update_fg_bar(out0, mag, n)).all(), (err / dc.update_fg_bar(out0, mag, n)).max()
    nd = max(len(coords) - 2, 0)      # the list form stops at the device count
    want, mag, n = dc.update_fg_rule(diffs, weight, out0, coords[:nd])
    out, cnt = Guarded(out0), dev(np.array([nd], dtype=np.int32))
    lib.check(C_.cbinfer_update_output_fg_list(dd.data_ptr(), wd.data_ptr(), out.ptr(), c32.data_ptr(), len(coords),
                                               cnt.data_ptr(), K, C, H, W, kH, kW, None))
    got = out.get()
    assert (np.abs(got.astype(np.float64) - want) <= dc.update_fg_bar(out0, mag, n)).all()
    assert np.array_equal(dc.bits(got)[n == 0], dc.bits(out0)[n == 0])      # no contribution: not a bit moves


# ---------------------------------------------------------------------------------------------------------------------
# compaction, dilation of a byte map
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("content", dc.COMPACT_CONTENTS)
@pytest.mark.parametrize("name,H,W", dc.COMPACT_MASKS)
def test_compaction_of_a_bit_mask(lib, name, H, W, content):
    C_ = lib.C
    m = dc.compact_mask(H, W, content)
    want = np.flatnonzero(m).astype(np.int32)
    words = dc.pack(m)
    bits = dev(words)
    for extras in (False, True):      # with and without the byte map and the cleared other mask
        idx, cnt = Guarded(np.full(H * W, -7, dtype=np.int32)), Guarded(np.array([-1], dtype=np.int32))
        other = Guarded(np.full(words.size, 0x55, dtype=np.uint64))
        cmap = Guarded(np.full((H, W), 7, dtype=np.int8))
        lib.check(C_.cbinfer_compact_bits(bits.data_ptr(), W, H, idx.ptr(), cnt.ptr(), other.ptr() if extras else None,
                                          cmap.ptr() if extras else None, None))
        got = idx.get()
        assert int(cnt.get()[0]) == want.size, (name, extras)
        assert np.array_equal(got[:want.size], want) and (got[want.size:] == -7).all(), (name, extras)
        assert np.array_equal(cmap.get(), m.astype(np.int8) if extras else np.full((H, W), 7, dtype=np.int8))
        assert (other.get() == (0 if extras else 0x55)).all()
    assert np.array_equal(host(bits).view(np.uint64), words)      # the mask itself is read only


@pytest.mark.parametrize("numel", dc.FLAT_NUMELS)
def test_compaction_of_a_byte_map(lib, numel):
    C_ = lib.C
    rng = np.random.default_rng(numel)
    for content in ("empty", "full", "last", "random"):
        m = np.zeros(numel, dtype=np.int8)
        if content == "full":
            m[:] = 1
        elif content == "last":
            m[-1] = -3      # (any non-zero byte counts)
        elif content == "random":
            m = rng.choice(np.array([0, 0, 0, 1, -3], dtype=np.int8), numel)
        want = np.flatnonzero(m).astype(np.int32)
        idx, cnt = Guarded(np.full(numel, -7, dtype=np.int32)), Guarded(np.array([-1], dtype=np.int32))
        scratch = Guarded(np.full((numel + 63) // 64, 0x55, dtype=np.uint64))
        md = dev(m)
        lib.check(C_.cbinfer_change_indexes_extr(md.data_ptr(), numel, scratch.ptr(), idx.ptr(), cnt.ptr(), None))
        got = idx.get()
        assert int(cnt.get()[0]) == want.size, content
        assert np.array_equal(got[:want.size], want) and (got[want.size:] == -7).all(), content
        scratch.get()


@pytest.mark.parametrize("filt", dc.FILTERS)
def test_dilation_of_a_byte_map(lib, filt):
    C_ = lib.C
    for H, W in dc.SIZES:
        raw = np.random.default_rng(H * W).random((H, W)) < 0.05
        raw[H - 1, W - 1] = True
        out, rd = Guarded(np.full((H, W), 7, dtype=np.int8)), dev(raw.astype(np.int8) * 5)      # (any non-zero byte counts)
        lib.check(C_.cbinfer_change_propagation(rd.data_ptr(), out.ptr(), W, H, filt[0] // 2, filt[1] // 2, None))
        assert np.array_equal(out.get(), dc.dilate(raw, filt[0] // 2, filt[1] // 2).astype(np.int8)), (H, W)


# ---------------------------------------------------------------------------------------------------------------------
# the pool and index ops
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, F16])
@pytest.mark.parametrize("shape", dc.POOL_SHAPES)
def test_max_pool_and_indexes_through_the_pool(lib, shape, dtype):
    C_ = lib.C
    C, iH, iW, ceil = shape
    d = dc.pool_data(C, iH, iW, ceil, dtype)
    oH, oW, entries = d["oH"], d["oW"], d["entries"]
    x, lst = dev(d["inp"]), dev(entries)
    nw = int(C_.cbinfer_mask_words(oH, oW))
    for count in (None, d["n_dev"]):      # the host count alone; a device count below it
        n = len(entries) if count is None else count
        cnt = dev(np.array([count], dtype=np.int32)) if count is not None else None
        cp = cnt.data_ptr() if cnt is not None else None
        out = Guarded(d["out0"])
        lib.check(C_.cbinfer_max_pool2d(x.data_ptr(), out.ptr(), lst.data_ptr(), len(entries), cp, C, iH, iW, oH, oW,
                                        dc.CODE[dtype], None))
        want = dc.max_pool_rule(d["inp"], d["out0"], entries[:n], oH, oW)      # (untouched outputs keep the pre-fill)
        assert np.array_equal(dc.bits(out.get()), dc.bits(want)), count
        words = Guarded(np.zeros(nw, dtype=np.uint64))
        lib.check(C_.cbinfer_pool_change_indexes(lst.data_ptr(), len(entries), cp, iW, oH, oW, words.ptr(), None))
        check_words(words.get(), dc.pool_indexes_rule(entries[:n], iW, oH, oW), oH, oW, count)


@pytest.mark.parametrize("filt", dc.FILTERS)
def test_dilation_of_an_index_list(lib, filt):
    """cbinfer_dilate_change_indexes: kWH up to 63 over W = 130; entries outside the map are dropped (the pool kernels do
    not take such entries: their lists above hold in-map pixels only)."""
    C_ = lib.C
    kHH, kWH = filt[0] // 2, filt[1] // 2
    for H, W in ((5, 130), (1, 63), (5, 1), (5, 64)):
        rng = np.random.default_rng(H * W + kWH)
        inside = np.flatnonzero(rng.random(H * W) < 0.05).tolist() + [0, H * W - 1, W - 1]
        entries = np.array(inside + [-1, H * W, H * W + 5, 2 ** 31 - 1, -2 ** 31], dtype=np.int32)
        rng.shuffle(entries)
        ed = dev(entries)
        for count in (None, len(entries) - 3):
            n = len(entries) if count is None else count
            cnt = dev(np.array([count], dtype=np.int32)) if count is not None else None
            words = Guarded(np.zeros(int(C_.cbinfer_mask_words(H, W)), dtype=np.uint64))
            lib.check(C_.cbinfer_dilate_change_indexes(ed.data_ptr(), len(entries), cnt.data_ptr() if cnt is not None else None,
                                                       H, W, kHH, kWH, words.ptr(), None))
            check_words(words.get(), dc.dilate_indexes_rule(entries[:n].tolist(), H, W, kHH, kWH), H, W, (H, W, count))


# ---------------------------------------------------------------------------------------------------------------------
# the refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refused_calls_leave_every_buffer_unchanged(lib):
    """kWHalf = 64, H = 65536, H nSeq > 65535, a dtype of 2 and a null pointer, at every detection entry point: the status
    the header names, and not a byte of any buffer moved."""
    C_ = lib.C
    W, H, C, pH, pW = 5, 3, 2, 6, 10
    rng = np.random.default_rng(1)
    bufs = {}

    def buf(name, n):
        bufs[name] = (rng.integers(1, 100, n).astype(np.int32), None)
        bufs[name] = (bufs[name][0], dev(bufs[name][0]))
        return bufs[name][1].data_ptr()

    x, state, out = buf("x", C * pH * pW), buf("state", C * H * W), buf("out", 64)
    delta, prod, count = buf("delta", C * H * W), buf("prod", 64), buf("count", 1)
    tables = {k: ptrs([v, v]) for k, v in (("inputs", x), ("states", state), ("bitsOut", out))}
    common = dict(W=W, H=H, C=C, kHHalf=1, kWHalf=1, threshold=0.1, stream=None)
    calls = {
        "cbinfer_change_detection": dict(common, input=x, state=state, changeMap=out, updateInputState=1, dtype=0),
        "cbinfer_change_detection_bits": dict(common, input=x, state=state, bitsOut=out, updateInputState=1, dtype=0),
        "cbinfer_change_detection_frame": dict(common, input=x, state=state, frameMasks=out, updateInputState=1, dtype=0),
        "cbinfer_change_detection_frame_after": dict(common, upstreamCount=count, input=x, state=state, frameMasks=out,
                                                     updateInputState=1, dtype=0),
        "cbinfer_change_detection_bits_pooled": dict(common, prePool=x, pH=pH, pW=pW, producerMask=prod, state=state,
                                                     bitsOut=out, dtype=0),
        "cbinfer_change_detection_frame_pooled": dict(common, prePool=x, pH=pH, pW=pW, state=state, frameMasks=out, dtype=0),
        "cbinfer_change_detection_bits_batched": dict(common, nSeq=2, updateInputState=1, **tables),
        "cbinfer_change_detection_fg_frame": dict(common, input=x, prevInput=state, delta=delta, frameMasks=out,
                                                  refreshState=1),
        "cbinfer_change_detection_fg_bits": dict(common, input=x, prevInput=state, delta=delta, bits=out, refreshState=1),
    }
    optional = {"producerMask", "upstreamCount", "stream"}
    tried = 0
    for name, kw in calls.items():
        fn = getattr(C_, name)
        bad = [(dict(kw, kWHalf=64), dc.UNSUPPORTED)]
        big = dict(kw, H=65536, pH=131072) if "pH" in kw else dict(kw, H=65536)
        bad.append((big, dc.UNSUPPORTED))
        if "nSeq" in kw:
            bad.append((dict(kw, H=32768), dc.UNSUPPORTED))      # H nSeq = 65536
            bad.append((dict(kw, states=ptrs([state, None])), dc.BADARG))      # a null entry of a table
            bad.append((dict(kw, nSeq=C_.cbinfer_split_max_sequences() + 1), dc.BADARG))
        if "dtype" in kw:
            bad.append((dict(kw, dtype=2), dc.BADARG))
        for p in kw:
            if p not in optional and isinstance(kw[p], (int, ctypes.Array)) and p not in common and p not in \
                    ("pH", "pW", "nSeq", "dtype", "updateInputState", "refreshState"):
                bad.append((dict(kw, **{p: None}), dc.BADARG))
        for args, status in bad:
            assert fn(*fn.pack(**args)) == status, (name, {k: v for k, v in args.items() if kw[k] is not v})
            tried += 1
    torch.cuda.synchronize()
    for name, (before, t) in bufs.items():
        assert np.array_equal(host(t), before), name
    assert tried >= 9 * 3 + 6
    # the same calls, unperturbed, are taken
    for name, kw in calls.items():
        fn = getattr(C_, name)
        assert fn(*fn.pack(**kw)) == dc.OK, name
    torch.cuda.synchronize()
