"""-m gpu tests of the general-geometry CBConv2d (stride, dilation, free zero padding, even filter sizes, no bias;
cb_geomconv.hip) against a twin written here in numpy / CPU torch.  The reference has no such layer, so the twin IS the
specification ("General geometry"):
  rule 1 / 3  per-pixel change on the INPUT map and the state refresh: the pinned oracle's changeDetection /
              changeDetection_half with filtSize=(1, 1) (no dilation), updateInputState as the layer's mode;
  rule 2      the change list on the OUTPUT map: output (oy, ox) iff one of its taps is a changed input pixel -- written
              twice (tap loop, and conv2d(changed, ones) > 0) and asserted equal;
  rule 4      torch.nn.functional.conv2d in float64 on the twin's state, compared at the listed pixels; every other
              output pixel must keep its bits.  An output pixel no tap reaches (padding beyond the dilated filter's
              reach) is never listed, so the C entry points never write it: the caller initialises it -- CBConv2d with
              the bias (after the ReLU), its dense value.
The twin is teacher-forced: it and the module see the same frames.  Bars: fp32 1e-4 absolute, fp16
4 * 2^-10 * max(1, |ref|max) -- those of tests/test_gpu_modules.py::test_fuzz_shapes_track_dense; inputs in [0, 1),
torch's default initialisation."""
import copy
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F
from optest import bits_of, dev, npdtype, gpu_pkg as pkg      # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

FP32_TOL = 1e-4
TH = 0.05

# (kernel, stride, padding, dilation), each a pair
GEOMS = {
    "7x7s2p3": ((7, 7), (2, 2), (3, 3), (1, 1)),
    "3x3s2p1": ((3, 3), (2, 2), (1, 1), (1, 1)),
    "1x1s2p0": ((1, 1), (2, 2), (0, 0), (1, 1)),
    "3x3d2p2": ((3, 3), (1, 1), (2, 2), (2, 2)),
    "3x3d4p4": ((3, 3), (1, 1), (4, 4), (4, 4)),
    "3x3s1p0": ((3, 3), (1, 1), (0, 0), (1, 1)),
    "3x3s2d2p2": ((3, 3), (2, 2), (2, 2), (2, 2)),
    "4x4s2p1": ((4, 4), (2, 2), (1, 1), (1, 1)),
    "2x2s2p0": ((2, 2), (2, 2), (0, 0), (1, 1)),
    "4x4s4p0": ((4, 4), (4, 4), (0, 0), (1, 1)),
    "aniso": ((3, 5), (2, 1), (0, 3), (1, 2)),
    # padding beyond the dilated filter's reach: the outer output pixels have no tap inside the input map
    "3x3p3": ((3, 3), (1, 1), (3, 3), (1, 1)),
    "2x2s2p2": ((2, 2), (2, 2), (2, 2), (1, 1)),
    "1x1p64": ((1, 1), (1, 1), (64, 64), (1, 1)),
}
NAMES = list(GEOMS)
RING = ("3x3p3", "2x2s2p2", "1x1p64")      # geometries with unreachable output pixels
DTYPES = [torch.float32, torch.float16]


def out_size(n, k, s, p, d):
    return (n + 2 * p - d * (k - 1) - 1) // s + 1


def in_size_for(target, k, s, p, d):
    """Smallest input size whose output size is `target`."""
    n = 1
    while n + 2 * p - d * (k - 1) - 1 < 0 or out_size(n, k, s, p, d) < target:
        n += 1
    assert out_size(n, k, s, p, d) == target
    return n


def sizes_for(name, geom, Ho, Wo):
    """Input size of a test map: the smallest with the output size asked for; '1x1p64' (Wo = Wi + 128) on a 1..3-pixel
    map instead."""
    (kH, kW), s, p, d = geom
    if name == "1x1p64":
        return 1 + Ho % 3, 1 + Wo % 3
    return in_size_for(Ho, kH, s[0], p[0], d[0]), in_size_for(Wo, kW, s[1], p[1], d[1])


def reachable(geom, Hi, Wi, Ho, Wo):
    """The output pixels with a tap inside the input map: all of them unless p > d (k-1) on an axis."""
    return footprint(np.ones((Hi, Wi), dtype=bool), geom, Ho, Wo)


def footprint(changed, geom, Ho, Wo):
    """Rule 2, both forms: the tap loop and conv2d(changedMap, ones) > 0; they must agree."""
    (kH, kW), (sH, sW), (pH, pW), (dH, dW) = geom
    Hi, Wi = changed.shape
    listed = np.zeros((Ho, Wo), dtype=bool)
    oy, ox = np.arange(Ho), np.arange(Wo)
    for ky in range(kH):
        iy = oy * sH - pH + ky * dH
        oky = (iy >= 0) & (iy < Hi)
        for kx in range(kW):
            ix = ox * sW - pW + kx * dW
            okx = (ix >= 0) & (ix < Wi)
            sub = changed[np.clip(iy, 0, Hi - 1)][:, np.clip(ix, 0, Wi - 1)].astype(bool)
            listed |= sub & oky[:, None] & okx[None, :]
    other = F.conv2d(torch.from_numpy(changed.astype(np.float32))[None, None], torch.ones(1, 1, kH, kW),
                     stride=(sH, sW), padding=(pH, pW), dilation=(dH, dW))[0, 0].numpy() > 0
    assert np.array_equal(listed, other)
    return listed


class Twin(object):
    def __init__(self, oracle, weight, bias, geom, th, feedback, relu):
        self.oracle, self.geom, self.th, self.feedback, self.relu = oracle, geom, th, feedback, relu
        self.w = weight.detach().cpu().double()
        self.b = bias.detach().cpu().double() if bias is not None else None
        self.state = None

    def step(self, x):
        """x: numpy [1, C, Hi, Wi] in the layer's dtype -> (ascending list, listed map, dense float64 reference)"""
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
        ref = F.conv2d(torch.from_numpy(self.state.astype(np.float64)), self.w, self.b, stride=s, padding=p,
                       dilation=d)[0]
        if self.relu:
            ref = torch.relu(ref)
        return np.flatnonzero(listed.reshape(-1)).astype(np.int32), listed, ref.numpy()


def frames_for(rng, C, Hi, Wi, n, npdtype, th=TH):
    """n frames in [0, 1): a few moved blocks per frame plus fresh noise well below the threshold (any two frames' noise
    differs by at most th / 2, so noise alone never lists a pixel, in feedback mode either)."""
    base = rng.random((1, C, Hi, Wi)) * 0.9
    out = []
    for t in range(n):
        if t:
            base = base.copy()
            for _ in range(int(rng.integers(1, 4))):
                y0, x0 = int(rng.integers(0, Hi)), int(rng.integers(0, Wi))
                hh, ww = int(rng.integers(1, 6)), int(rng.integers(1, 9))
                base[:, :, y0:y0 + hh, x0:x0 + ww] = rng.random(base[:, :, y0:y0 + hh, x0:x0 + ww].shape) * 0.9
        noise = (rng.random(base.shape) - 0.5) * (th / 2)
        out.append(np.clip(base + noise, 0.0, 0.999).astype(npdtype))
    return out


def make_conv(geom, C, K, bias, dtype):
    k, s, p, d = geom
    return nn.Conv2d(C, K, k, stride=s, padding=p, dilation=d, bias=bias).cuda().to(dtype)


def dense_f64(conv, x):
    """conv(x) in float64 on the CPU.  (Not conv(x) on the device: the vendor library's fp16 convolution of the
    stride-2 dilation-2 layer was measured 0.66-0.81 away from this reference, this project's kernel 5e-4.)"""
    b = conv.bias.detach().cpu().double() if conv.bias is not None else None
    return F.conv2d(x.detach().cpu().double(), conv.weight.detach().cpu().double(), b, stride=conv.stride,
                    padding=conv.padding, dilation=conv.dilation)


def bound_for(dtype, ref):
    return FP32_TOL if dtype == torch.float32 else 4 * 2.0 ** -10 * max(1.0, float(np.abs(ref).max()))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16"])
@pytest.mark.parametrize("name", NAMES)
def test_geometries_track_the_twin(pkg, oracle, name, dtype):
    """Every geometry, feedbackLoop / withReLU / bias each both ways, Wo of 63, 64 and 65, K on and off the 32-row tile:
    over 5 frames with a threshold above zero the change list and prevInput equal the twin's bit for bit, listed
    output pixels are within the bar, unlisted ones keep the previous frame's bits."""
    geom = GEOMS[name]
    (kH, kW), s, p, d = geom
    gi = NAMES.index(name)
    rng = np.random.default_rng(100 + gi)
    npdtype = np.float32 if dtype == torch.float32 else np.float16
    for c in range(8):
        feedback, relu, bias = bool(c & 1), bool(c & 2), bool(c & 4)
        Wo = (63, 64, 65)[(c + gi) % 3]
        K = (32, 33, 64, 70)[(c + gi) % 4]
        Cin = (3, 16, 5, 32)[c % 4]
        Hi, Wi = sizes_for(name, geom, 5 + c, Wo)
        Hi += c % s[0]
        Ho, Wo = out_size(Hi, kH, s[0], p[0], d[0]), out_size(Wi, kW, s[1], p[1], d[1])
        conv = make_conv(geom, Cin, K, bias, dtype)
        m = pkg.CBConv2d(conv, TH, generalGeometry=True)
        m.feedbackLoop, m.withReLU = feedback, relu
        twin = Twin(oracle, conv.weight, conv.bias, geom, TH, feedback, relu)
        prev = None
        with torch.no_grad():
            for t, x in enumerate(frames_for(rng, Cin, Hi, Wi, 5, npdtype)):
                y = m(torch.from_numpy(x).cuda())
                idx, listed, ref = twin.step(x)
                tag = (name, str(dtype), c, t)
                assert tuple(y.shape) == (1, K, Ho, Wo), tag
                got = m.lastChangeIndexes().tensor().cpu().numpy()
                assert np.array_equal(got, idx), tag
                if name in RING:      # the first frame lists every pixel a tap reaches, and those are not all
                    assert t > 0 or Ho * Wo > idx.size == int(reachable(geom, Hi, Wi, Ho, Wo).sum()), tag
                else:
                    assert t > 0 or idx.size == Ho * Wo, tag
                assert np.array_equal(bits_of(m.prevInput.cpu().numpy()), bits_of(twin.state)), tag
                out = y.cpu().numpy()[0]
                if idx.size:
                    err = np.abs(out.astype(np.float64)[:, listed] - ref[:, listed]).max()
                    assert err <= bound_for(dtype, ref), tag + (err,)
                if prev is not None:
                    assert np.array_equal(bits_of(out)[:, ~listed], bits_of(prev)[:, ~listed]), tag
                elif name in RING:    # never written: the dense value there is the bias and nothing else
                    assert np.array_equal(out[:, ~listed], ref[:, ~listed].astype(npdtype)), tag
                prev = out.copy()


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16"])
@pytest.mark.parametrize("name", NAMES + ["wide"])
def test_threshold_zero_equals_dense(pkg, name, dtype):
    """With threshold 0 the layer equals conv(x) densely after every frame.  'wide': 256 output channels at 161 x 241,
    where the list fills more tiles than the grid has workgroups (no k-split, several tiles per workgroup).  The
    geometries of RING (output pixels without a tap inside the map, whose dense value is the bias) run with and
    without bias, with and without ReLU."""
    rng = np.random.default_rng(7)
    if name == "wide":
        geom, Cin, K, Hi, Wi = GEOMS["3x3s2p1"], 3, 256, 161, 241
    else:
        geom = GEOMS[name]
        gi = NAMES.index(name)
        Cin, K = (3, 16, 5, 32)[gi % 4], (32, 33, 64, 70)[gi % 4]
        Hi, Wi = sizes_for(name, geom, 9, (63, 64, 65)[gi % 3])
    if name in RING:
        combos = [(b, r) for b in (True, False) for r in (False, True)]
    else:
        combos = [(name != "7x7s2p3", NAMES.index(name) % 2 == 0 if name != "wide" else True)]
    for bias, relu in combos:
        conv = make_conv(geom, Cin, K, bias, dtype)
        m = pkg.CBConv2d(conv, 0.0, generalGeometry=True)
        m.withReLU = relu
        m.feedbackLoop = name in ("3x3d2p2", "4x4s4p0", "wide")
        x = torch.rand(1, Cin, Hi, Wi, device="cuda").to(dtype)
        with torch.no_grad():
            for t in range(4):
                if t:
                    x = x.clone()
                    for _ in range(3):
                        y0, x0 = int(rng.integers(0, Hi)), int(rng.integers(0, Wi))
                        x[:, :, y0:y0 + 4, x0:x0 + 7] = torch.rand_like(x[:, :, y0:y0 + 4, x0:x0 + 7])
                y = m(x.clone())
                ref = dense_f64(conv, x)
                if m.withReLU:
                    ref = torch.relu(ref)
                err = (y.cpu().double() - ref).abs().max().item()
                assert err <= bound_for(dtype, ref.numpy()), (name, bias, relu, t, err)


def test_beyond_the_limits_is_a_cbinfer_error(pkg):
    from cbinfer_amd._lib import CBinferError
    for conv in (nn.Conv2d(3, 8, 16, stride=16), nn.Conv2d(3, 8, 3, dilation=9), nn.Conv2d(3, 8, 3, stride=5)):
        with pytest.raises(CBinferError):
            pkg.CBConv2d(conv.cuda(), TH, generalGeometry=True)
    m = pkg.CBConv2d(nn.Conv2d(3, 8, 3, stride=2).cuda(), TH, generalGeometry=True)
    m.finegrained = True
    with pytest.raises(CBinferError):
        m(torch.rand(1, 3, 9, 9, device="cuda"))
    # propagated indexes address the input map: refused where the output map differs
    m = pkg.CBConv2d(nn.Conv2d(3, 8, 3, stride=2).cuda(), TH, generalGeometry=True)
    with pytest.raises(CBinferError):
        m(('changeIndexes', torch.rand(1, 3, 9, 9, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16"])
def test_unit_geometry_is_untouched_by_the_flag(pkg, dtype):
    """A unit-geometry layer built with generalGeometry=True is bit-identical, lists and outputs, to one built without."""
    rng = np.random.default_rng(3)
    conv = nn.Conv2d(16, 40, 3, padding=1).cuda().to(dtype)
    a, b = pkg.CBConv2d(conv, TH), pkg.CBConv2d(conv, TH, generalGeometry=True)
    assert not b._geom
    npdtype = np.float32 if dtype == torch.float32 else np.float16
    with torch.no_grad():
        for x in frames_for(rng, 16, 21, 70, 5, npdtype):
            xa = torch.from_numpy(x).cuda()
            ya, yb = a(xa.clone()), b(xa.clone())
            assert torch.equal(ya, yb)
            assert torch.equal(a.lastChangeIndexes().tensor(), b.lastChangeIndexes().tensor())
            assert a._path(xa, 21, 70) == b._path(xa, 21, 70) != 'geom'


def test_same_size_dilated_layer_takes_propagated_indexes_and_hands_its_own_on(pkg):
    """Output map == input map (dilated, stride 1, 'same' padding): propagated indexes mean what they mean today; and the
    layer's own list feeds a 1x1 CBConv2d unchanged."""
    conv = nn.Conv2d(8, 16, 3, padding=2, dilation=2).cuda()
    m = pkg.CBConv2d(conv, TH, generalGeometry=True)
    x = torch.rand(1, 8, 12, 70, device="cuda")
    idx = torch.tensor([3, 77, 500], dtype=torch.int32, device="cuda")
    with torch.no_grad():
        y = m(('changeIndexes', x, idx)).clone()
        ref = dense_f64(conv, x).float().cuda()
    H, W = 12, 70
    mask = torch.zeros(H * W, dtype=torch.bool, device="cuda")
    mask[idx.long()] = True
    mask = mask.view(H, W)
    assert (y[0][:, mask] - ref[0][:, mask]).abs().max().item() <= FP32_TOL
    assert torch.isinf(y[0][:, ~mask]).all()
    head = pkg.CBConv2d(conv, TH, generalGeometry=True)
    head.propChangeIndexes = True
    one = nn.Conv2d(16, 4, 1).cuda()
    tail = pkg.CBConv2d(one, TH)
    with torch.no_grad():
        for t in range(3):
            if t:
                x = x.clone()
                x[:, :, 3:6, 10 * t:10 * t + 5] += 0.3
            out = tail(head(x))
            ref = dense_f64(one, dense_f64(conv, x)).float().cuda()
            assert (out - ref).abs().max().item() <= 2 * FP32_TOL


def _c_abi_buffers(lib, C, geom, Cin, K, Hi, Wi, dtype):
    (kH, kW), s, p, d = geom
    g = lib.Geom(kH, kW, s[0], s[1], p[0], p[1], d[0], d[1])
    Ho, Wo = ctypes.c_int(), ctypes.c_int()
    assert C.cbinfer_geom_out_size(Hi, Wi, ctypes.byref(g), ctypes.byref(Ho), ctypes.byref(Wo)) == 0
    Ho, Wo = Ho.value, Wo.value
    dev = "cuda"
    return g, Ho, Wo, dict(
        state=torch.full((1, Cin, Hi, Wi), float('inf'), dtype=dtype, device=dev),
        out=torch.full((1, K, Ho, Wo), 7.0, dtype=dtype, device=dev),
        bits=torch.zeros(C.cbinfer_frame_mask_bytes(Ho, Wo) // 8, dtype=torch.int64, device=dev),
        idx=torch.full((Ho * Wo,), -1, dtype=torch.int32, device=dev),
        count=torch.full((1,), -1, dtype=torch.int32, device=dev),
        ws=torch.zeros(C.cbinfer_geom_workspace_bytes(), dtype=torch.uint8, device=dev))


@pytest.mark.parametrize("name", ["3x3s2p1", "aniso"])
def test_c_abi_detection_and_contraction(pkg, oracle, name):
    """cbinfer_change_detection_geom + cbinfer_conv_changed_geom called directly, against the twin; then a frame in
    which nothing changes: count 0, output untouched, both masks clean."""
    from cbinfer_amd import _lib
    C, ptr, check = _lib.C, _lib.ptr, _lib.check
    geom = GEOMS[name]
    Cin, K, Hi, Wi = 5, 33, 14, 131
    rng = np.random.default_rng(11)
    conv = make_conv(geom, Cin, K, True, torch.float32)
    g, Ho, Wo, B = _c_abi_buffers(_lib, C, geom, Cin, K, Hi, Wi, torch.float32)
    gp = ctypes.byref(g)
    wp = torch.empty(C.cbinfer_geom_prepared_weights_bytes(K, Cin, gp, _lib.CB_F32S), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    check(C.cbinfer_geom_prep_weights(ptr(conv.weight.detach()), ptr(wp), K, Cin, Hi, Wi, gp, _lib.CB_F32S, st))
    twin = Twin(oracle, conv.weight, conv.bias, geom, TH, True, False)
    words = C.cbinfer_mask_words(Ho, Wo)
    frames = frames_for(rng, Cin, Hi, Wi, 3, np.float32)
    for t, x in enumerate(frames + [frames[-1]]):
        xd = torch.from_numpy(x).cuda()
        before = B['out'].clone()
        check(C.cbinfer_change_detection_geom(ptr(xd), ptr(B['state']), ptr(B['bits']), Cin, Hi, Wi, gp, TH, 1,
                                              _lib.CB_F32, st))
        check(C.cbinfer_conv_changed_geom(ptr(B['state']), None, 0, None, ptr(B['bits']), ptr(B['idx']), ptr(B['count']),
                                          ptr(wp), ptr(conv.bias.detach()), ptr(B['out']), Cin, Hi, Wi, K, gp, 0,
                                          ptr(B['ws']), _lib.CB_F32S, st))
        torch.cuda.synchronize()
        idx, listed, ref = twin.step(x)
        n = int(B['count'].item())
        assert np.array_equal(B['idx'][:n].cpu().numpy(), idx), (name, t)
        assert np.array_equal(bits_of(B['state'].cpu().numpy()), bits_of(twin.state))
        out = B['out'].cpu().numpy()[0]
        if n:
            assert np.abs(out.astype(np.float64)[:, listed] - ref[:, listed]).max() <= FP32_TOL
        assert np.array_equal(bits_of(out)[:, ~listed], bits_of(before.cpu().numpy()[0])[:, ~listed])
        if t == len(frames):      # the repeated frame: an empty change list
            assert n == 0 and torch.equal(B['out'], before)
            assert int(B['bits'][:2 * words].ne(0).sum().item()) == 0
        assert int(B['ws'][-2048:].ne(0).sum().item()) == 0      # the k-split arrival counters are left zero
    # list mode with an empty list: nothing launched, output untouched
    before = B['out'].clone()
    check(C.cbinfer_conv_changed_geom(ptr(B['state']), ptr(B['idx']), 0, None, None, None, None, ptr(wp), None,
                                      ptr(B['out']), Cin, Hi, Wi, K, gp, 0, ptr(B['ws']), _lib.CB_F32S, st))
    torch.cuda.synchronize()
    assert torch.equal(B['out'], before)
    # out-of-range geometry: a status, no launch
    bad = _lib.Geom(16, 16, 16, 16, 0, 0, 1, 1)
    assert C.cbinfer_change_detection_geom(ptr(xd), ptr(B['state']), ptr(B['bits']), Cin, Hi, Wi, ctypes.byref(bad), TH,
                                           1, _lib.CB_F32, st) == -2


def mixed_net():
    torch.manual_seed(5)
    return nn.Sequential(
        nn.Conv2d(3, 16, 7, stride=2, padding=3, bias=False), nn.ReLU(),
        nn.Conv2d(16, 16, 3, padding=1), nn.MaxPool2d(2, 2),
        nn.Conv2d(16, 32, 3, stride=2, padding=1), nn.ReLU(),
        nn.Conv2d(32, 32, 3, padding=2, dilation=2), nn.ReLU(),
        nn.Conv2d(32, 8, 1)).eval().cuda()


def converted_mixed(pkg):
    net = pkg.convert(mixed_net(), threshold=TH, generalGeometry=True)
    pkg.insertCBPooling(net, cloneOutput=False)
    pkg.propChangeIndexesOf1x1(net)
    return net


def fuse(pkg, net):
    pkg.fusePoolingIntoDetection(net)
    pkg.fuseDetectionIntoProducer(net)
    pkg.fuseTail1x1(net)
    return net


def mixed_frames(n, seed=21):
    rng = np.random.default_rng(seed)
    return [torch.from_numpy(f).cuda() for f in frames_for(rng, 3, 97, 131, n, np.float32)]


def test_mixed_network_fused_equals_unfused_and_replays(pkg):
    from cbinfer_amd._lib import CBinferError
    plain = converted_mixed(pkg)
    kinds = [type(m).__name__ for m in plain.children()]
    assert kinds == ['CBConv2d', 'CBConv2d', 'CBPoolMax2d', 'CBConv2d', 'CBConv2d', 'CBConv2d'], kinds
    convs = [m for m in plain.children() if type(m) is pkg.CBConv2d]
    assert [bool(m._geom) for m in convs] == [True, False, True, True, False]
    assert convs[0].withReLU and convs[3].propChangeIndexes and convs[1].propChangeIndexes
    fused = fuse(pkg, copy.deepcopy(plain))
    pool = [m for m in fused.children() if type(m) is pkg.CBPoolMax2d][0]
    assert not pool.lazy      # (a general-geometry consumer: the pool keeps pooling itself)
    assert '_fusedConsumers' not in convs[0].__dict__
    dense = mixed_net()
    frames = mixed_frames(6)
    with torch.no_grad():
        for t, f in enumerate(frames):
            ya, yb = plain(f), fused(f)
            assert (ya - yb).abs().max().item() <= FP32_TOL, t
            for ma, mb in zip(convs, [m for m in fused.children() if type(m) is pkg.CBConv2d]):
                assert torch.equal(ma.lastChangeIndexes().tensor(), mb.lastChangeIndexes().tensor()), t
        # threshold-bounded drift against the dense network is not asserted; the layers are (tests above)
        assert tuple(ya.shape) == tuple(dense(frames[-1]).shape)
        # recorded launch program == eager
        eager = copy.deepcopy(fused)
        more = mixed_frames(4, seed=22)
        prog = pkg.FrameProgram(fused)
        for f in more:
            yp, ye = prog(f), eager(f)
            assert torch.equal(yp, ye)
        for ta, tb in zip(pkg.getStateTensors(fused), pkg.getStateTensors(eager)):
            assert torch.equal(ta, tb)
    # one CUDAGraph replay == eager (warm-up on a side stream, capture, new frame into the static input, replay)
    with torch.no_grad():
        eg = copy.deepcopy(eager)
        gr = copy.deepcopy(eager)
        sin = more[2].clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            gr(sin)
        torch.cuda.current_stream().wait_stream(side)
        eg(more[2])
        g2 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g2, stream=side):
            out = gr(sin)
        sin.copy_(more[3])
        g2.replay()
        ye = eg(more[3])
        torch.cuda.synchronize()
        assert torch.equal(out, ye)
    with pytest.raises(CBinferError, match="general-geometry"):
        pkg.SequenceBatch(fused, 2)
    with pytest.raises(CBinferError, match="general-geometry"):
        pkg.BranchGroup([fused])


def test_two_runs_give_the_same_bits(pkg):
    outs = []
    for run in range(2):
        torch.manual_seed(9)
        conv = nn.Conv2d(64, 96, 3, padding=2, dilation=2).cuda()
        m = pkg.CBConv2d(conv, TH, generalGeometry=True)
        net = converted_mixed(pkg)
        rng = np.random.default_rng(33)
        got = []
        with torch.no_grad():
            for x in frames_for(rng, 64, 40, 60, 5, np.float32):
                got.append(m(torch.from_numpy(x).cuda()).clone())
            for f in mixed_frames(4):
                got.append(net(f).clone())
        outs.append(got)
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_change_map_stats_and_state_helpers(pkg):
    conv = nn.Conv2d(3, 8, 3, stride=2, padding=1, bias=False).cuda()
    m = pkg.CBConv2d(conv, TH, generalGeometry=True)
    m.saveChangeMap = m.gatherComputationStats = True
    x = torch.rand(1, 3, 21, 131, device="cuda")
    with torch.no_grad():
        m(x)
        x2 = x.clone()
        x2[:, :, 4:6, 10:13] += 0.4
        m(x2)
    Ho, Wo = 11, 66
    cm = m.changeMap.cpu().numpy()
    assert cm.shape == (Ho, Wo)
    idx = m.lastChangeIndexes().tensor().cpu().numpy()
    assert np.array_equal(np.flatnonzero(cm.reshape(-1)), idx) and 0 < idx.size < Ho * Wo
    assert int(m.compStats['totalInputValues']) == Ho * Wo * 3 * 8 * 9 * 2
    assert [tuple(t.shape) for t in m.getStateTensors()] == [(1, 3, 21, 131), (1, 8, Ho, Wo)]
    m.clearMemory()
    assert m.prevInput.numel() == 0 and m.lastChangeIndexes() is None
