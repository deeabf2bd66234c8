"""-m gpu tests of change-based peak suppression and peak lists (cb_peaks.hip) against the numpy twin of
tests/peaks_cases.py, which restates the rule of include/cbinfer_hip.h: through the C ABI every case x form x dtype as
consecutive frames, and through CBPoolMax2d(suppress=...) inside converted networks.  Everything is compared bit for
bit; there is no tolerance anywhere in this file."""
import copy
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import peaks_cases as pc
from peaks_cases import DTYPES, FORMS, SHAPES, WINDOW_IDS, WINDOWS
from optest import (dev, dev_words, free_pixel, host_words, lib, operand_args,      # noqa: F401  (fixtures)
                    gpu_pkg as pkg, raw, stream)

pytestmark = pytest.mark.gpu

# a state no result has: NaNs (a suppressed map holds none)
FILL = {"f32": 0x7fc12345, "f16": 0x7e55}


@pytest.fixture(scope="module")
def walks():
    """The frames of every (shape, value set, dtype, window) and the twin's (out, keep) of each: computed once, shared
    by the forms, never written."""
    cache = {}

    def get(shape, kind, dtype, window):
        key = (shape, kind, dtype, window)
        if key not in cache:
            fr = pc.frames(shape, kind, dtype, window)
            cache[key] = (fr, [pc.twin(x, window) for _, _, x in fr])
        return cache[key]
    return get


def peaks_struct(lib, window):
    kH, kW, cross, floor = WINDOWS[window]
    return lib.Peaks(kH, kW, cross, int(floor is not None), floor or 0.0)


class State(object):
    """The caller-owned buffers of one map through the C ABI: the state full of FILL, peakBits zero, the working mask
    zero, the mask copy and the list buffers full of stale values."""

    def __init__(self, lib, shape, dtype, window):
        self.lib, self.shape, self.dtype, self.window = lib, shape, dtype, window
        Cn, H, W = shape
        self.words = lib.C.cbinfer_mask_words(H, W)
        out = np.empty(shape, dtype=pc.np_dtype(dtype))
        pc.bits_of(out)[...] = FILL[dtype]
        self.hostOut = out
        self.out = dev(out)
        self.peakBits = torch.zeros(Cn * self.words, dtype=torch.int64, device="cuda")
        self.bits = torch.zeros(self.words, dtype=torch.int64, device="cuda")
        self.copy = torch.full((self.words,), -1, dtype=torch.int64, device="cuda")
        self.pk = np.zeros(shape, dtype=bool)
        n = Cn * H * W
        self.work = torch.full((Cn * H + 1,), -5, dtype=torch.int32, device="cuda")
        self.entries = torch.full((n, 3), -7, dtype=torch.int32, device="cuda")
        self.scores = torch.zeros(n, dtype=self.out.dtype, device="cuda")
        self.count = torch.full((1,), -9, dtype=torch.int32, device="cuda")
        self.start = torch.full((Cn + 1,), -9, dtype=torch.int32, device="cuda")
        self.p = peaks_struct(lib, window)

    def frame(self, form, t, S, x):
        lib, ptr = self.lib, self.lib.ptr
        Cn, H, W = self.shape
        L = pc.listed(S, self.window, form)
        # (every other frame: a device count in front of junk -- a pixel outside the footprint L, where there is one)
        mask, lst, cap, cnt = operand_args(form, S, free_pixel(L, middle=True) or 0, bool(t % 2))
        self.x = dev(x)
        self.entries.fill_(-7)
        code = lib.CB_F32 if self.dtype == "f32" else lib.CB_F16
        lib.check(lib.C.cbinfer_cbpeaks_forward(ptr(self.x), ptr(self.out), ptr(self.peakBits), ptr(mask), ptr(lst), cap,
                                                ptr(cnt), ptr(self.bits), ptr(self.copy), Cn, H, W, ctypes.byref(self.p),
                                                code, stream()))
        lib.check(lib.C.cbinfer_peaks_list(ptr(self.x), ptr(self.peakBits), ptr(self.work), ptr(self.entries),
                                           ptr(self.scores), self.entries.size(0), ptr(self.count), ptr(self.start), Cn, H,
                                           W, code, stream()))
        torch.cuda.synchronize()
        return L

    def check(self, L, x, want, where):
        wantOut, k = want
        got = self.out.cpu().numpy()
        assert np.array_equal(pc.bits_of(got[:, L]), pc.bits_of(wantOut[:, L])), (where, "listed pixels")
        assert np.array_equal(pc.bits_of(got[:, ~L]), pc.bits_of(self.hostOut[:, ~L])), (where, "unlisted pixels")
        self.hostOut = got
        assert np.array_equal(host_words(self.copy), pc.pack(L)), (where, "mask copy")
        assert not self.bits.any().item(), (where, "working mask")
        self.pk[:, L] = k[:, L]
        assert np.array_equal(host_words(self.peakBits), pc.peak_bits(self.pk)), (where, "peakBits")
        entries, scores, count, start = pc.peak_list(x, self.pk)
        assert int(self.count.item()) == count and np.array_equal(self.start.cpu().numpy(), start), (where, "count")
        assert np.array_equal(self.entries[:count].cpu().numpy(), entries), (where, "entries")
        assert np.array_equal(pc.bits_of(self.scores[:count].cpu().numpy()), pc.bits_of(scores)), (where, "scores")
        assert bool((self.entries[count:] == -7).all().item()), (where, "beyond the list")


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("window", WINDOW_IDS)
def test_frames_through_the_c_abi(lib, walks, window, dtype, form):
    """Every shape and value set as consecutive frames: at the listed pixels the state has the twin's bits, unlisted
    pixels keep theirs (FILL until they are first listed), maskCopy is the footprint, the working mask zero, peakBits
    the twin's in every word, entries, scores, count and channelStart the twin's.  All three forms are held against the
    same twin, so a pixel's bits depend neither on the other listed pixels nor on the form."""
    for shape in SHAPES:
        for kind in pc.value_sets(dtype):
            fr, twins = walks(shape, kind, dtype, window)
            st = State(lib, shape, dtype, window)
            for t, ((label, S, x), want) in enumerate(zip(fr, twins)):
                L = st.frame(form, t, S, x)
                st.check(L, x, want, (shape, kind, label))


@pytest.mark.parametrize("dtype", DTYPES)
def test_list_capacity_overflow(lib, walks, dtype):
    """N = count - 1 and N = 0: the first N entries in order, nothing beyond them, count and channelStart true."""
    for shape, window in (((5, 5, 70), "w3"), ((19, 12, 64), "cross"), ((1, 1, 1), "w7")):
        fr, twins = walks(shape, "quantised", dtype, window)
        label, S, x = fr[5]
        st = State(lib, shape, dtype, window)
        st.frame("all", 0, S, x)
        entries, scores, count, start = pc.peak_list(x, twins[5][1])
        assert count >= 1
        Cn, H, W = shape
        code = lib.CB_F32 if dtype == "f32" else lib.CB_F16
        for N in (count - 1, 0):
            ent = torch.full((count + 2, 3), -7, dtype=torch.int32, device="cuda")
            sc = torch.full((count + 2,), 7.0, dtype=st.out.dtype, device="cuda")
            cnt = torch.full((1,), -9, dtype=torch.int32, device="cuda")
            start_d = torch.full((Cn + 1,), -9, dtype=torch.int32, device="cuda")
            lib.check(lib.C.cbinfer_peaks_list(lib.ptr(st.x), lib.ptr(st.peakBits), lib.ptr(st.work),
                                               lib.ptr(ent) if N else None, lib.ptr(sc) if N else None, N, lib.ptr(cnt),
                                               lib.ptr(start_d), Cn, H, W, code, stream()))
            torch.cuda.synchronize()
            assert int(cnt.item()) == count and np.array_equal(start_d.cpu().numpy(), start), (shape, N)
            assert np.array_equal(ent[:N].cpu().numpy(), entries[:N]), (shape, N)
            assert np.array_equal(pc.bits_of(sc[:N].cpu().numpy()), pc.bits_of(scores[:N])), (shape, N)
            assert bool((ent[N:] == -7).all().item()) and bool((sc[N:] == 7.0).all().item()), (shape, N)


def test_stale_padding_bits_in_peak_bits_are_cleared(lib):
    """peakBits full of ones before an every-pixel frame: the row-padding bits are zero afterwards."""
    shape = (5, 5, 70)
    (label, S, x), = pc.frames(shape, "random", "f32", "w3")[5:6]
    st = State(lib, shape, "f32", "w3")
    st.peakBits.fill_(-1)
    L = st.frame("all", 0, S, x)
    st.check(L, x, pc.twin(x, "w3"), "stale peakBits")


# ------------------------------------------------------------------------------------------------ the module
class SimpleNMS(nn.Module):
    """What a keypoint head writes: the map where it equals its own max pool and reaches the floor."""

    def __init__(self, k, floor):
        super(SimpleNMS, self).__init__()
        self.k, self.floor = k, floor

    def forward(self, x):
        keep = (F.max_pool2d(x, self.k, 1, self.k // 2) == x) & (x >= self.floor)
        return torch.where(keep, x, torch.zeros_like(x))


H0, W0, CAP = 12, 70, 4096


def passes_net(pkg, tdt):
    """conv -> CBPointwise2d(sigmoid) -> CBPoolMax2d(suppress='window', 5x5, floor 0.4), put there by the passes."""
    torch.manual_seed(23)
    src = nn.Sequential(nn.Conv2d(3, 6, 3, padding=1), nn.Sigmoid(), SimpleNMS(5, 0.4))
    net = pkg.insertCBPointwise(pkg.convert(src.eval().cuda().to(tdt), threshold=0.0), transcendental=True)
    pkg.insertCBPooling(net, cloneOutput=False, generalGeometry=True,
                        nmsTypes={SimpleNMS: dict(kernel_size=5, suppress='window', floor=0.4, peakList=CAP)})
    assert [type(m).__name__ for m in net] == ['CBConv2d', 'CBPointwise2d', 'CBPoolMax2d']
    assert net[0].propChangeIndexes and net[1].propChangeIndexes and net[2].suppress == 'window'
    net[1].cloneOutput = False
    return net, dict(kernel_size=5, suppress='window', floor=0.4)


def resize_net(pkg, tdt):
    """conv -> CBResize2d -> CBPoolMax2d(suppress='cross', floor 0.1), the pose pipeline's end, wired by hand."""
    torch.manual_seed(29)
    net = pkg.convert(nn.Sequential(nn.Conv2d(3, 5, 3, padding=1)).eval().cuda().to(tdt), threshold=0.0)
    net[0].propChangeIndexes = True
    resize = pkg.CBResize2d(size=(2 * H0 + 1, 2 * W0 - 9), mode='bilinear', align_corners=False)
    resize.propChangeIndexes, resize.cloneOutput = True, False
    nmsm = pkg.CBPoolMax2d(nn.MaxPool2d(3, 1, 1), generalGeometry=True, suppress='cross', floor=0.1, peakList=CAP)
    nmsm.cloneOutput = False
    net.add_module('1', resize)
    net.add_module('2', nmsm)
    return net, dict(kernel_size=3, suppress='cross', floor=0.1)


NETS = {"passes": passes_net, "resize": resize_net}


def moving_frames(rng, n, tdt):
    """n frames [1, 3, H0, W0]; a frame differs from the one before in two moved blocks only."""
    base = rng.random((1, 3, H0, W0)) * 2 - 1
    frames = []
    for i in range(n):
        base = base.copy()
        if i:
            for _ in range(2):
                y0, x0 = int(rng.integers(0, H0)), int(rng.integers(0, W0))
                blk = base[:, :, y0:y0 + 2, x0:x0 + 3]
                blk[...] = rng.random(blk.shape) * 2 - 1
        frames.append(torch.from_numpy(base).to(tdt).cuda())
    return frames


def same_state_and_list(a, b):
    """State tensors equal; count and channelStart equal; entries and scores equal up to the count (what lies beyond it
    is whatever earlier frames left there)."""
    for ta, tb in zip(a.getStateTensors(), b.getStateTensors()):
        if not torch.equal(ta, tb):
            return False
    (ea, sa, ca, fa), (eb, sb, cb, fb) = a.peakList(), b.peakList()
    n = int(ca.item())
    return bool(torch.equal(ca, cb) and torch.equal(fa, fb) and torch.equal(ea[:n], eb[:n]) and
                torch.equal(raw(sa[:n]), raw(sb[:n])))


def unpack(words, H, W):
    b = np.unpackbits(host_words(words).view(np.uint8), bitorder='little').reshape(H, -1)
    assert not b[:, W:].any()
    return b[:, :W].astype(bool)


def check_against_the_rule(pkg, m, x, kw, t):
    """State, peakBits and list of the module `m` after a frame whose operand was x: the twin's of x alone, and the
    formula in dense torch operators."""
    from cbinfer_amd.pool import suppression_formula
    xs = x[0].cpu().numpy()
    k = pc.keep(xs, m.kernel_size[0], m.kernel_size[1], int(kw['suppress'] == 'cross'), kw['floor'])
    assert np.array_equal(pc.bits_of(m.outputState[0].cpu().numpy()), pc.bits_of(pc.suppressed(xs, k))), t
    dense = suppression_formula(x.cpu().float(), kw['kernel_size'], kw['suppress'], kw['floor']).to(x.dtype)
    assert torch.equal(raw(m.outputState.cpu()), raw(dense)), t
    assert np.array_equal(host_words(m.peakBits), pc.peak_bits(k)), t
    entries, scores, count, start = pc.peak_list(xs, k)
    e, s, c, st = m.peakList()
    assert int(c.item()) == count and 1 <= count <= CAP and np.array_equal(st.cpu().numpy(), start), t
    assert np.array_equal(e[:count].cpu().numpy(), entries), t
    assert np.array_equal(pc.bits_of(s[:count].cpu().numpy()), pc.bits_of(scores)), t
    host = m.peaksToHost()
    assert len(host) == xs.shape[0] and sum(len(h) for h in host) == count
    assert [(px, py) for px, py, _ in host[-1]] == [(int(r[2]), int(r[1])) for r in entries[start[-2]:]]
    return k


@pytest.mark.parametrize("tdt", (torch.float32, torch.float16), ids=DTYPES)
@pytest.mark.parametrize("which", list(NETS))
def test_networks_over_eight_frames(pkg, lib, which, tdt):
    """Both networks over 8 frames of a moving input, stepped module by module: after every frame state, peakBits and
    list are those of a copy of the module that recomputes every pixel (its memory cleared before the frame), which are
    the twin's and the dense formula's of the module's operand; the mask handed on is the footprint of the mask handed
    in; frames after the first list fewer pixels than the map has.  In the middle the state tensors are carried into a
    fresh module, which goes on as the first; clearMemory makes the next frame list every pixel."""
    net, kw = NETS[which](pkg, tdt)
    net[2].propChangeIndexes = True
    full = copy.deepcopy(net[2])
    frames = moving_frames(np.random.default_rng(5), 8, tdt)
    kH, kW = net[2].kernel_size
    partial = 0
    with torch.no_grad():
        for t, f in enumerate(frames):
            mid = net[0](f)
            if which == "passes":
                mid = net[1](mid)
            tag, x, ix = mid
            Hm, Wm = x.shape[-2:]
            S = unpack(ix._mask, Hm, Wm)
            if t == 4:      # the state carried into a fresh module
                fresh = copy.deepcopy(full)
                fresh.clearMemory()
                fresh.outputState, fresh.peakBits = [s.clone() for s in net[2].getStateTensors()]
                net._modules['2'] = fresh
            if t == 6:
                net[2].clearMemory()
                assert [s.numel() for s in net[2].getStateTensors()] == [0, 0]
            tag2, y, iy = net[2](mid)
            assert tag2 == 'changeIndexes' and y is net[2].outputState and iy.size == (Hm, Wm)
            L = unpack(iy._mask, Hm, Wm)
            want = np.ones((Hm, Wm), dtype=bool) if t in (0, 6) else pc.footprint(S, kH, kW)
            assert np.array_equal(L, want), t
            partial += int(0 < L.sum() < L.size)
            assert not net[2].__dict__['_poolWork']['bits'].any().item()
            check_against_the_rule(pkg, net[2], x, kw, t)
            full.clearMemory()
            full(mid)
            assert same_state_and_list(net[2], full), t
    assert partial >= 5


@pytest.mark.parametrize("which", list(NETS))
def test_frame_program_replays_state_and_list(pkg, lib, which):
    """cloneOutput=False recorded and replayed by a FrameProgram: outputs, states and the list buffers -- which keep
    their addresses -- equal the eager network's after every replayed frame."""
    net, kw = NETS[which](pkg, torch.float32)
    frames = moving_frames(np.random.default_rng(9), 7, torch.float32)
    with torch.no_grad():
        for f in frames[:3]:
            net(f)
        eager = copy.deepcopy(net)
        before = [t.data_ptr() for t in net[2].peakList()]
        prog = pkg.FrameProgram(net)
        for t, f in enumerate(frames[3:]):
            yp, ye = prog(f), eager(f)
            assert torch.equal(raw(yp), raw(ye)), t
            for a, b in zip(pkg.getStateTensors(net), pkg.getStateTensors(eager)):
                assert torch.equal(a, b), t
            assert same_state_and_list(net[2], eager[2]), t
            assert [p.data_ptr() for p in net[2].peakList()] == before
        raws = [fn for fn, _ in prog.calls]
        assert raws.count(lib.C.cbinfer_cbpeaks_forward.raw) == 1 and raws.count(lib.C.cbinfer_peaks_list.raw) == 1
        x = net[1].outputState
        check_against_the_rule(pkg, net[2], x, kw, "replayed")


@pytest.mark.parametrize("dtype", DTYPES)
def test_module_operand_forms(pkg, lib, dtype):
    """A bare tensor lists every pixel; a list (an int32 tensor, a ChangeIndexes with a device count) and a mask walk
    to the same bits; cloneOutput=True hands out a private copy; too many peaks for the list raise in peaksToHost."""
    from cbinfer_amd.conv2d_cg import MaskChangeIndexes
    shape, window = (5, 5, 70), "w3x7"
    kH, kW, cross, floor = WINDOWS[window]
    fr = pc.frames(shape, "quantised", dtype, window)
    for form in ("tensor", "list", "mask"):
        m = pkg.CBPoolMax2d(nn.MaxPool2d((kH, kW), 1, (kH // 2, kW // 2)), generalGeometry=True, suppress='window',
                            floor=floor, peakList=3).cuda()
        m.propChangeIndexes = True
        for t, (label, S, x) in enumerate(fr):
            xd = dev(x)[None]
            idx = torch.from_numpy(np.flatnonzero(S.reshape(-1)).astype(np.int32)).cuda()
            if t == 0:
                given = xd
            elif form == "tensor":
                given = ('changeIndexes', xd, idx)
            else:
                buf = torch.zeros(S.size, dtype=torch.int32, device="cuda")
                buf[:idx.numel()] = idx
                cnt = torch.tensor([idx.numel()], dtype=torch.int32, device="cuda")
                given = ('changeIndexes', xd, pkg.ChangeIndexes(buf, cnt, size=S.shape) if form == "list" else
                         MaskChangeIndexes(dev_words(pc.pack(S)), S.shape, buf, cnt))
            tag, y, iy = m(given)
            out, k = pc.twin(x, window)
            assert y is not m.outputState and torch.equal(raw(y), raw(m.outputState))
            assert np.array_equal(pc.bits_of(y[0].cpu().numpy()), pc.bits_of(out)), (form, label)
            assert np.array_equal(host_words(m.peakBits), pc.peak_bits(k)), (form, label)
            L = np.ones(S.shape, dtype=bool) if t == 0 else pc.footprint(S, kH, kW)
            assert np.array_equal(host_words(iy._mask), pc.pack(L)), (form, label)
            assert iy.tensor().cpu().tolist() == np.flatnonzero(L).tolist()
            entries, scores, count, start = pc.peak_list(x, k)
            e, s, c, st = m.peakList()
            assert int(c.item()) == count > 3 and np.array_equal(e.cpu().numpy(), entries[:3])
            assert np.array_equal(st.cpu().numpy(), start)
        with pytest.raises(lib.CBinferError, match=r"the frame has \d+ peaks, the list holds peakList=3"):
            m.peaksToHost()
    with pytest.raises(lib.CBinferError, match="address a 4x4 map, this pool's input map is 5x70"):
        m(('changeIndexes', xd, pkg.ChangeIndexes(torch.zeros(16, dtype=torch.int32, device="cuda"),
                                                  torch.zeros(1, dtype=torch.int32, device="cuda"), size=(4, 4))))
