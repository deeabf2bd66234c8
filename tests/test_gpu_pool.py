"""-m gpu tests of change-based pooling for any window (CBPoolMax2d(m, generalGeometry=True), CBPoolAvg2d;
cb_pool2d.hip) against a twin written here in numpy / CPU torch.  The reference pools 2x2/stride 2 only, so the twin IS
the specification:
  rule 1  the output size: torch's rule, written out in out_axis() and checked against the shapes torch returns;
  rule 2  the listed output pixels: (oy, ox) iff its window clipped to the input map holds a changed pixel -- written
          twice (tap loop, and max_pool2d(changed) > 0) and asserted equal;
  rule 3  the values: CPU torch's F.max_pool2d / F.avg_pool2d of the same input, BIT FOR BIT at the listed pixels (fp32
          and fp16: the average is an f32 sum in row-major window order, one IEEE division, one rounding); every other
          output pixel keeps its bits.
There is no tolerance anywhere in this file."""
import copy
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F
from optest import (bits_of, dev_words, host_words, lib, npdtype, pack, gpu_pkg as pkg,      # noqa: F401  (fixtures)
                    stream)

pytestmark = pytest.mark.gpu

TH = 0.05

# (window, stride, padding, ceil_mode)
WINDOWS = {
    "3x3s2p1": ((3, 3), (2, 2), (1, 1), False),
    "3x3s2p0ceil": ((3, 3), (2, 2), (0, 0), True),
    "2x2s2p1ceil": ((2, 2), (2, 2), (1, 1), True),
    "2x2s3p0": ((2, 2), (3, 3), (0, 0), False),
    "3x3s3p0": ((3, 3), (3, 3), (0, 0), False),
    "1x1s2p0": ((1, 1), (2, 2), (0, 0), False),
    "7x7s1p3": ((7, 7), (1, 1), (3, 3), False),
    "5x5s1p2": ((5, 5), (1, 1), (2, 2), False),
    "4x4s2p1": ((4, 4), (2, 2), (1, 1), False),
    "aniso": ((3, 2), (2, 1), (1, 0), False),
    "2x2s2p0": ((2, 2), (2, 2), (0, 0), False),
}
STRIDED = ("2x2s2p0", (4200, 9))      # 2100 output mask words, more than workgroups: the grid-stride leg of the kernel
NAMES = list(WINDOWS)
OPS = ["max", "avg_pad", "avg_nopad"]


# ------------------------------------------------------------------------------------------------ the twin
def out_axis(n, k, s, p, ceil):
    """Rule 1."""
    assert n + 2 * p >= k
    o = (-(-(n + 2 * p - k) // s) if ceil else (n + 2 * p - k) // s) + 1
    if ceil and (o - 1) * s >= n + p:
        o -= 1
    return o


def in_size_for(target, k, s, p, ceil):
    """Smallest input size whose output size is `target`."""
    n = max(1, k - 2 * p)
    while out_axis(n, k, s, p, ceil) < target:
        n += 1
    assert out_axis(n, k, s, p, ceil) == target
    return n


def out_hw(win, Hi, Wi):
    (kH, kW), (sH, sW), (pH, pW), ceil = win
    return out_axis(Hi, kH, sH, pH, ceil), out_axis(Wi, kW, sW, pW, ceil)


def footprint(changed, win):
    """Rule 2, both forms; they must agree (the second also checks rule 1 against torch)."""
    (kH, kW), (sH, sW), (pH, pW), ceil = win
    Hi, Wi = changed.shape
    Ho, Wo = out_hw(win, Hi, Wi)
    listed = np.zeros((Ho, Wo), dtype=bool)
    oy, ox = np.arange(Ho), np.arange(Wo)
    for ky in range(kH):
        iy = oy * sH - pH + ky
        oky = (iy >= 0) & (iy < Hi)
        for kx in range(kW):
            ix = ox * sW - pW + kx
            okx = (ix >= 0) & (ix < Wi)
            sub = changed[np.clip(iy, 0, Hi - 1)][:, np.clip(ix, 0, Wi - 1)].astype(bool)
            listed |= sub & oky[:, None] & okx[None, :]
    other = F.max_pool2d(torch.from_numpy(changed.astype(np.float32))[None, None], (kH, kW), (sH, sW), (pH, pW),
                         ceil_mode=ceil)[0, 0].numpy() > 0
    assert other.shape == listed.shape and np.array_equal(listed, other)
    return listed


def cpu_pool(x, win, op):
    """Rule 3: x a CPU tensor [1, C, Hi, Wi] in the layer's dtype."""
    k, s, p, ceil = win
    if op == "max":
        return F.max_pool2d(x, k, s, p, ceil_mode=ceil)
    return F.avg_pool2d(x, k, s, p, ceil_mode=ceil, count_include_pad=(op == "avg_pad"))


def pool_struct(lib, win, op="max"):
    (kH, kW), (sH, sW), (pH, pW), ceil = win
    code = {"max": lib.POOL_MAX, "avg_pad": lib.POOL_AVG_PAD, "avg_nopad": lib.POOL_AVG_NOPAD}[op]
    return lib.Pool(kH, kW, sH, sW, pH, pW, int(ceil), code)


# ------------------------------------------------------------------------------------------------ launch 1
@pytest.mark.parametrize("name", NAMES)
def test_footprint_list_and_mask_form(lib, name):
    """cbinfer_pool_footprint in both forms against the numpy footprint: the mask bit-exact, the compacted list
    ascending; Wo = 64, 65 and 129 (word boundaries), Ho = 5."""
    C, ptr, check = lib.C, lib.ptr, lib.check
    win = WINDOWS[name]
    (kH, kW), (sH, sW), (pH, pW), ceil = win
    g = ctypes.byref(pool_struct(lib, win))
    rng = np.random.default_rng(7)
    for WoT in (64, 65, 129):
        Hi, Wi = in_size_for(5, kH, sH, pH, ceil), in_size_for(WoT, kW, sW, pW, ceil)
        Ho, Wo = out_hw(win, Hi, Wi)
        assert (Ho, Wo) == (5, WoT)
        ho, wo = ctypes.c_int(), ctypes.c_int()
        assert C.cbinfer_pool_out_size(Hi, Wi, g, ctypes.byref(ho), ctypes.byref(wo)) == 0
        assert (ho.value, wo.value) == (Ho, Wo)
        words = C.cbinfer_mask_words(Ho, Wo)
        sets = {"empty": np.zeros((Hi, Wi), dtype=bool), "all": np.ones((Hi, Wi), dtype=bool),
                "random": rng.random((Hi, Wi)) < 0.1}
        singles = [("corner", y, x) for y in (0, Hi - 1) for x in (0, Wi - 1)]
        # input columns whose windows straddle output columns 63 / 64
        singles += [("straddle", Hi // 2, x) for x in range(max(63 * sW - pW, 0), min(64 * sW - pW + kW, Wi))]
        gaps = [x for x in range(Wi) if (x + pW) % sW >= kW]
        if gaps:      # (s > k: a pixel between two windows)
            singles.append(("gap", Hi // 2, gaps[len(gaps) // 2]))
        assert bool(gaps) == (sW > kW)
        for kind, y, x in singles:
            m = np.zeros((Hi, Wi), dtype=bool)
            m[y, x] = True
            sets["%s(%d,%d)" % (kind, y, x)] = m
        for label, changed in sets.items():
            listed = footprint(changed, win)
            if label.startswith("gap"):
                assert not listed.any()
            want = pack(listed)
            idx = np.flatnonzero(changed.reshape(-1)).astype(np.int32)
            if label == "random":      # out-of-map entries are dropped
                idx = np.concatenate([idx[:5], np.array([Hi * Wi, -1, Hi * Wi + 77], dtype=np.int32), idx[5:]])
            n = len(idx)
            # every other set through a device-side count, behind which the buffer holds entries that must not be read
            useCount = label == "random" or label.startswith("corner")
            buf = torch.from_numpy(np.concatenate([idx, np.full(9, (Hi // 2) * Wi + Wi // 2, dtype=np.int32)])).cuda()
            count = torch.tensor([n], dtype=torch.int32, device="cuda") if useCount else None
            bits = torch.zeros(words, dtype=torch.int64, device="cuda")
            check(C.cbinfer_pool_footprint(ptr(buf), buf.numel() if useCount else n, ptr(count), None, Hi, Wi, g,
                                           ptr(bits), stream()))
            assert np.array_equal(host_words(bits), want), (name, WoT, label, "list form")
            out = torch.full((Ho * Wo,), -1, dtype=torch.int32, device="cuda")
            cnt = torch.full((1,), -1, dtype=torch.int32, device="cuda")
            check(C.cbinfer_compact_bits(ptr(bits), Wo, Ho, ptr(out), ptr(cnt), None, None, stream()))
            got = out[:int(cnt.item())].cpu().numpy()
            assert np.array_equal(got, np.flatnonzero(listed.reshape(-1))), (name, WoT, label, "compacted list")
            bits2 = torch.zeros(words, dtype=torch.int64, device="cuda")
            check(C.cbinfer_pool_footprint(None, 0, None, ptr(dev_words(pack(changed))), Hi, Wi, g, ptr(bits2),
                                           stream()))
            assert np.array_equal(host_words(bits2), want), (name, WoT, label, "mask form")
    # exactly one of list and mask; windows beyond the limits: a status, nothing launched
    assert C.cbinfer_pool_footprint(None, 0, None, None, Hi, Wi, g, ptr(bits), stream()) == -1
    assert C.cbinfer_pool_footprint(ptr(buf), 1, None, ptr(bits2), Hi, Wi, g, ptr(bits), stream()) == -1
    bad = pool_struct(lib, ((9, 3), (1, 1), (1, 1), False))
    assert C.cbinfer_pool_footprint(ptr(buf), 1, None, None, Hi, Wi, ctypes.byref(bad), ptr(bits), stream()) == -2
    torch.cuda.synchronize()
    assert np.array_equal(host_words(bits), want)


# ------------------------------------------------------------------------------------------------ launch 2
MARK = {np.dtype(np.float32): 0x4B3C614E, np.dtype(np.float16): 0x5BCD}


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("name", NAMES)
def test_values_through_the_c_abi(lib, name, op):
    """cbinfer_cbpool2d_forward: listed pixels bit-identical to CPU torch, every other pixel keeps the marker, the
    working mask is zero after the call and the mask copy holds the frame's mask."""
    C, ptr, check = lib.C, lib.ptr, lib.check
    win = WINDOWS[name]
    (kH, kW), (sH, sW), (pH, pW), ceil = win
    g = ctypes.byref(pool_struct(lib, win, op))
    rng = np.random.default_rng(13)
    combos = [(1, np.float32, "list"), (5, np.float32, "mask"), (67, np.float32, "list"),
              (1, np.float16, "mask"), (5, np.float16, "list"), (67, np.float16, "mask")]
    for Cn, npdtype, form in combos:
        maps = [(11, 9) if name == "2x2s2p1ceil" else (13, 17)]      # (a 9-wide axis: the drop rule of ceil mode)
        if Cn == 5:      # more than one mask word per row, more than one workgroup
            maps.append((in_size_for(3, kH, sH, pH, ceil), in_size_for(66, kW, sW, pW, ceil)))
        if Cn == 1 and name == STRIDED[0]:
            maps.append(STRIDED[1])
        for Hi, Wi in maps:
            Ho, Wo = out_hw(win, Hi, Wi)
            if (Hi, Wi) == STRIDED[1]:
                assert C.cbinfer_mask_words(Ho, Wo) > 8 * torch.cuda.get_device_properties(0).multi_processor_count
            x = rng.standard_normal((1, Cn, Hi, Wi))
            if Cn == 5 and npdtype == np.float32:
                x = -np.abs(x) - 0.25      # negative values only: the zero padding must not win
            x = x.astype(npdtype)
            xt = torch.from_numpy(x)
            ref = bits_of(cpu_pool(xt, win, op).numpy()[0])
            assert ref.shape == (Cn, Ho, Wo)
            xd = xt.cuda()
            words = C.cbinfer_mask_words(Ho, Wo)
            bits = torch.zeros(words, dtype=torch.int64, device="cuda")
            mcopy = torch.full((words,), -1, dtype=torch.int64, device="cuda")
            out = torch.empty(1, Cn, Ho, Wo, dtype=xd.dtype, device="cuda")
            mark = MARK[np.dtype(npdtype)]
            for changed in (rng.random((Hi, Wi)) < 0.1, np.ones((Hi, Wi), dtype=bool), np.zeros((Hi, Wi), dtype=bool)):
                out.view(torch.int32 if npdtype == np.float32 else torch.int16).fill_(mark)
                listed = footprint(changed, win)
                idx = torch.from_numpy(np.flatnonzero(changed.reshape(-1)).astype(np.int32)).cuda()
                if form == "list":
                    lst, cap, msk = (idx if idx.numel() else out.new_zeros(1, dtype=torch.int32)), idx.numel(), None
                else:
                    lst, cap, msk = None, 0, dev_words(pack(changed))
                check(C.cbinfer_cbpool2d_forward(ptr(xd), ptr(out), ptr(lst), cap, None, ptr(msk), ptr(bits), ptr(mcopy),
                                                 Cn, Hi, Wi, g, lib.dtype_code(xd), stream()))
                got = bits_of(out.cpu().numpy()[0])
                where = (name, op, Cn, npdtype.__name__, form, Hi, Wi, int(changed.sum()))
                assert np.array_equal(got[:, listed], ref[:, listed]), where
                assert (got[:, ~listed] == mark).all(), where
                assert int(bits.ne(0).sum().item()) == 0, where
                assert np.array_equal(host_words(mcopy), pack(listed)), where
    # bad arguments: a status, nothing launched (the output keeps its bits)
    before = out.clone()
    st = stream()
    one = torch.zeros(1, dtype=torch.int32, device="cuda")

    def call(lst=one, msk=None, copyTo=mcopy, H=Hi, dt=lib.CB_F16, gg=g):
        return C.cbinfer_cbpool2d_forward(ptr(xd), ptr(out), ptr(lst), 0, None, ptr(msk), ptr(bits), ptr(copyTo), Cn,
                                          H, Wi, gg, dt, st)
    assert call(lst=None) == -1 and call(msk=bits) == -1      # exactly one of list and mask
    assert call(copyTo=bits) == -1 and call(dt=lib.CB_F32S) == -1
    if kH - 2 * pH > 1:
        assert call(H=kH - 2 * pH - 1) == -1      # a map smaller than the window
    bad = pool_struct(lib, ((3, 3), (9, 1), (1, 1), False), op)
    assert call(gg=ctypes.byref(bad)) == -2
    assert C.cbinfer_pool_changed(ptr(xd), ptr(out), ptr(bits), ptr(mcopy), Cn, Hi, Wi, ctypes.byref(bad), lib.CB_F16,
                                  st) == -2
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), before.view(torch.int16))


# ------------------------------------------------------------------------------------------------ the modules
def walk_frames(rng, C, Hi, Wi, npdtype):
    """Eight frames in [0, 1): moved blocks, an idle frame (the very same values) and one that changes everything."""
    base = rng.random((1, C, Hi, Wi)) * 0.9
    out = []
    for t in range(8):
        if t == 3:
            pass                                            # idle
        elif t == 5:
            base = (base + 0.45) % 0.9                      # everything: every value moves by 0.45
        elif t:
            base = base.copy()
            for _ in range(int(rng.integers(1, 4))):
                y0, x0 = int(rng.integers(0, Hi)), int(rng.integers(0, Wi))
                hh, ww = int(rng.integers(1, 6)), int(rng.integers(1, 9))
                base[:, :, y0:y0 + hh, x0:x0 + ww] = rng.random(base[:, :, y0:y0 + hh, x0:x0 + ww].shape) * 0.9
        out.append(base.astype(npdtype))
    return out


def make_producer(pkg, kind, dtype):
    torch.manual_seed(17)
    if kind == "geom":
        conv = nn.Conv2d(3, 8, 7, stride=2, padding=3, bias=False).cuda().to(dtype)
        m = pkg.CBConv2d(conv, TH, generalGeometry=True)
        size = (45, 139)
    else:
        conv = nn.Conv2d(3, 8, 3, padding=1).cuda().to(dtype)
        m = pkg.CBConv2d(conv, TH)
        m.syncIndexes = kind == "sync"
        size = (23, 70)
    m.propChangeIndexes = True
    return m, size


POOLS = [("max", lambda: nn.MaxPool2d(3, 2, 1), ((3, 3), (2, 2), (1, 1), False)),
         ("max", lambda: nn.MaxPool2d(3, 2, ceil_mode=True), ((3, 3), (2, 2), (0, 0), True)),
         ("avg_pad", lambda: nn.AvgPool2d(2), ((2, 2), (2, 2), (0, 0), False)),
         ("avg_nopad", lambda: nn.AvgPool2d(3, 2, 1, count_include_pad=False), ((3, 3), (2, 2), (1, 1), False))]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("kind", ["mask", "geom", "sync"])
def test_module_walk(pkg, lib, kind, dtype):
    """Behind a mask-driven unit layer (MaskChangeIndexes), a general-geometry 7x7/s2 layer (its list lives on its own
    output map) and a syncIndexes layer (exact tensors): after every frame outputState is the CPU pool of the producer's
    whole prevOutput, bit for bit, and the list handed on is the footprint of the producer's list."""
    from cbinfer_amd.conv2d_cg import ChangeIndexes, MaskChangeIndexes
    npdtype = np.float32 if dtype == torch.float32 else np.float16
    for op, make, win in POOLS:
        prod, (Hin, Win) = make_producer(pkg, kind, dtype)
        pool = pkg.CBPoolAvg2d(make()) if op != "max" else pkg.CBPoolMax2d(make(), generalGeometry=True)
        pool.propChangeIndexes = True
        pool.downsampleIndexes = True      # (ignored: the list handed on lives on the output map anyway)
        rng = np.random.default_rng(29)
        sawMaskForm = False
        with torch.no_grad():
            for t, x in enumerate(walk_frames(rng, 3, Hin, Win, npdtype)):
                tag, y, ix = prod(torch.from_numpy(x).cuda())
                Hi, Wi = y.shape[-2:]
                assert (Hi, Wi) == (23, 70)
                if kind == "sync":
                    assert isinstance(ix, torch.Tensor)
                else:
                    assert isinstance(ix, ChangeIndexes) and ix.size == (Hi, Wi)
                if kind == "mask" and dtype == torch.float32:
                    assert isinstance(ix, MaskChangeIndexes) and not ix._made
                    sawMaskForm = True
                tag2, z, pix = pool((tag, y, ix))
                if sawMaskForm:
                    assert not ix._made      # the producer's list was never materialised
                Ho, Wo = out_hw(win, Hi, Wi)
                ref = cpu_pool(prod.prevOutput.cpu(), win, op)
                assert tuple(pool.outputState.shape) == (1, 8, Ho, Wo) == tuple(ref.shape)
                assert np.array_equal(bits_of(pool.outputState.cpu().numpy()), bits_of(ref.numpy())), (kind, op, t)
                assert z is not pool.outputState and torch.equal(z, pool.outputState)
                lst = (ix if kind == "sync" else ix.tensor()).cpu().numpy()
                changed = np.zeros(Hi * Wi, dtype=bool)
                changed[lst] = True
                if t in (0, 5):
                    assert changed.all()
                if t == 3:
                    assert not changed.any()
                listed = footprint(changed.reshape(Hi, Wi), win)
                assert isinstance(pix, MaskChangeIndexes) and pix.size == (Ho, Wo) and tag2 == 'changeIndexes'
                assert np.array_equal(pix.tensor().cpu().numpy(), np.flatnonzero(listed.reshape(-1))), (kind, op, t)
        # a list that addresses another map is refused
        wrong = ChangeIndexes(torch.zeros(4, dtype=torch.int32, device="cuda"),
                              torch.zeros(1, dtype=torch.int32, device="cuda"), (Hi + 1, Wi))
        with pytest.raises(lib.CBinferError, match="%dx%d map.*%dx%d" % (Hi + 1, Wi, Hi, Wi)):
            pool(('changeIndexes', y, wrong))
        pool.cloneOutput = False
        out = pool(('changeIndexes', y, torch.zeros(0, dtype=torch.int32, device="cuda")))[1]
        assert out is pool.outputState and out._cbinfer_inplace_state
        pool.clearMemory()
        assert pool.outputState.numel() == 0 and pool._poolWork is None


def front_end():
    torch.manual_seed(5)
    return nn.Sequential(nn.Conv2d(3, 16, 7, stride=2, padding=3, bias=False), nn.ReLU(), nn.MaxPool2d(3, 2, 1),
                         nn.Conv2d(16, 16, 3, padding=1), nn.AvgPool2d(2), nn.Conv2d(16, 8, 1)).eval().cuda()


def net_frames(n, seed):
    rng = np.random.default_rng(seed)
    base = rng.random((1, 3, 97, 131)) * 0.9
    out = []
    for t in range(n):
        base = base.copy()
        for _ in range(3):
            y0, x0 = int(rng.integers(0, 97)), int(rng.integers(0, 131))
            base[:, :, y0:y0 + 9, x0:x0 + 14] = rng.random(base[:, :, y0:y0 + 9, x0:x0 + 14].shape) * 0.9
        out.append(torch.from_numpy(base.astype(np.float32)).cuda())
    return out


def test_front_end_records_as_a_launch_program(pkg):
    """conv 7x7/s2 + ReLU -> MaxPool2d(3, 2, 1) -> conv 3x3 -> AvgPool2d(2) -> conv 1x1 at 97x131, every pool
    change-based with cloneOutput=False: FrameProgram records the frame (no torch operator is left in it), the recorded
    program and one CUDAGraph replay equal the eager network bit for bit, outputs and all state tensors."""
    net = pkg.convert(front_end(), threshold=TH, generalGeometry=True)
    pkg.insertCBPooling(net, cloneOutput=False, generalGeometry=True)
    kinds = [type(m).__name__ for m in net.children()]
    assert kinds == ['CBConv2d', 'CBPoolMax2d', 'CBConv2d', 'CBPoolAvg2d', 'CBConv2d'], kinds
    pkg.fuseDetectionIntoProducer(pkg.fusePoolingIntoDetection(net))
    assert not any(m.lazy for m in net.children() if type(m) is not pkg.CBConv2d)
    dense = front_end()
    frames = net_frames(3, 41)
    with torch.no_grad():
        for f in frames:
            y = net(f)
        assert tuple(y.shape) == tuple(dense(frames[-1]).shape) == (1, 8, 12, 16)
        eager = copy.deepcopy(net)
        more = net_frames(6, 42)
        prog = pkg.FrameProgram(net)
        for f in more[:4]:
            yp, ye = prog(f), eager(f)
            assert torch.equal(yp, ye)
            for ta, tb in zip(pkg.getStateTensors(net), pkg.getStateTensors(eager)):
                assert torch.equal(ta, tb)
        assert len(pkg.getStateTensors(net)) == 8
        # one CUDAGraph replay == eager (warm-up on a side stream, capture, new frame into the static input, replay)
        eg = copy.deepcopy(eager)
        gr = copy.deepcopy(eager)
        sin = more[4].clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            gr(sin)
        torch.cuda.current_stream().wait_stream(side)
        eg(more[4])
        g2 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g2, stream=side):
            out = gr(sin)
        sin.copy_(more[5])
        g2.replay()
        ye = eg(more[5])
        torch.cuda.synchronize()
        assert torch.equal(out, ye)
        for ta, tb in zip(pkg.getStateTensors(gr), pkg.getStateTensors(eg)):
            assert torch.equal(ta, tb)
