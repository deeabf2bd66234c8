"""CPU-only tests of the change-based decoder operators: the numpy twin of the upsampling rules against
torch (nearest, bit for bit) and against the same rules in float64 (bilinear), the settings CBUpsample2d takes and
refuses, what insertCBUpsampling does to a network, the argument checks of the C entry points, exports, pickling and the
refusals.  No kernel is launched here."""
import copy
import ctypes
import pickle

import numpy as np
import pytest
import torch
import torch.nn as nn
from optest import lib, pkg      # noqa: F401  (fixtures)


# ------------------------------------------------------------------------------------------------ the twin
MODES = [("nearest", False), ("bilinear", False), ("bilinear", True)]


def twin_axis(n, s, mode, align):
    """Per output coordinate o < n s: the two source coordinates and the weight of the second as rho / den, in integers."""
    N = n * s
    o = np.arange(N, dtype=np.int64)
    if mode == "nearest":
        i0 = o // s
        return i0, i0, np.zeros(N, dtype=np.int64), 1
    if not align:
        num, den = np.maximum(2 * o + 1 - s, 0), 2 * s
    elif N > 1:
        num, den = o * (n - 1), N - 1
    else:
        num, den = np.zeros(N, dtype=np.int64), 1
    i0 = num // den
    return i0, np.minimum(i0 + 1, n - 1), num - i0 * den, den


def twin_upsample(x, sH, sW, mode, align, ftype):
    """x [C, Hi, Wi] -> [C, Hi sH, Wi sW] evaluated in `ftype` (nearest: a copy)."""
    y0, y1, ry, dy = twin_axis(x.shape[1], sH, mode, align)
    x0, x1, rx, dx = twin_axis(x.shape[2], sW, mode, align)
    if mode == "nearest":
        return x[:, y0][:, :, x0]
    one = ftype(1)
    ly = (ry.astype(ftype) / ftype(dy))[None, :, None]
    lx = (rx.astype(ftype) / ftype(dx))[None, None, :]
    v = x.astype(ftype)
    a, b, c, d = v[:, y0][:, :, x0], v[:, y0][:, :, x1], v[:, y1][:, :, x0], v[:, y1][:, :, x1]
    return (one - ly) * ((one - lx) * a + lx * b) + ly * ((one - lx) * c + lx * d)


def twin_corner_max(x, sH, sW, mode, align):
    """max(|a|, |b|, |c|, |d|) per output value, float64."""
    y0, y1, _, _ = twin_axis(x.shape[1], sH, mode, align)
    x0, x1, _, _ = twin_axis(x.shape[2], sW, mode, align)
    v = np.abs(x.astype(np.float64))
    return np.maximum(np.maximum(v[:, y0][:, :, x0], v[:, y0][:, :, x1]), np.maximum(v[:, y1][:, :, x0], v[:, y1][:, :, x1]))


def twin_footprint(m, sH, sW, mode, align):
    """The listed output pixels for the bool input mask m [Hi, Wi]: any source pixel listed."""
    y0, y1, _, _ = twin_axis(m.shape[0], sH, mode, align)
    x0, x1, _, _ = twin_axis(m.shape[1], sW, mode, align)
    return m[y0][:, x0] | m[y0][:, x1] | m[y1][:, x0] | m[y1][:, x1]


MAPS = [(1, 1), (3, 70), (5, 129)]
SCALES = [(sH, sW) for sH in range(1, 9) for sW in (1, 2, 3, 5, 8)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_nearest_twin_is_torch_bit_for_bit(dtype):
    rng = np.random.default_rng(1)
    for Hi, Wi in MAPS:
        x = torch.from_numpy(rng.standard_normal((1, 2, Hi, Wi)) * 10).to(dtype)
        for sH, sW in SCALES:
            want = nn.Upsample(scale_factor=(sH, sW), mode="nearest")(x)[0].numpy()
            got = twin_upsample(x[0].numpy(), sH, sW, "nearest", False, None)
            assert got.shape == want.shape == (2, Hi * sH, Wi * sW)
            assert np.array_equal(np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(want).view(np.uint8)), \
                (Hi, Wi, sH, sW)


@pytest.mark.parametrize("align", [False, True])
def test_bilinear_twin_in_float32_is_within_the_bars_of_float64(align):
    """fp32: |out - r| <= 8 2^-24 max(|a|,|b|,|c|,|d|) (weights, products and sums carry one rounding each); fp16: the f32
    value rounded once more, <= 2^-11 |r| + 2^-25 + 9 2^-24 max.  Also: the end points of align_corners=True and the weights
    of a x2 align_corners=False row are what the definition says."""
    rng = np.random.default_rng(2)
    worst = {np.float32: 0.0, np.float16: 0.0}
    for Hi, Wi in MAPS:
        for npdt in (np.float32, np.float16):
            x = (rng.standard_normal((2, Hi, Wi)) * 10).astype(npdt)
            for sH, sW in SCALES:
                r = twin_upsample(x, sH, sW, "bilinear", align, np.float64)
                got = twin_upsample(x, sH, sW, "bilinear", align, np.float32)
                assert got.dtype == np.float32
                mx = twin_corner_max(x, sH, sW, "bilinear", align)
                if npdt == np.float32:
                    err, bar = np.abs(got.astype(np.float64) - r), 8 * 2.0 ** -24 * mx
                else:
                    err = np.abs(got.astype(np.float16).astype(np.float64) - r)
                    bar = 2.0 ** -11 * np.abs(r) + 2.0 ** -25 + 9 * 2.0 ** -24 * mx
                assert (err <= bar).all(), (Hi, Wi, sH, sW, npdt)
                worst[npdt] = max(worst[npdt], float((err / np.where(bar > 0, bar, 1)).max()))
                if align and Hi > 1 and Wi > 1:      # the corners map onto the corners
                    assert np.array_equal(r[:, [0, -1]][:, :, [0, -1]], x.astype(np.float64)[:, [0, -1]][:, :, [0, -1]])
    print("bilinear twin, float32 against float64, worst share of the bar: fp32 %.3f (of 8 units: %.2f), fp16 %.4f"
          % (worst[np.float32], 8 * worst[np.float32], worst[np.float16]))
    if not align:
        i0, i1, rho, den = twin_axis(4, 2, "bilinear", False)
        assert list(i0) == [0, 0, 0, 1, 1, 2, 2, 3] and list(i1) == [1, 1, 1, 2, 2, 3, 3, 3]
        assert list(rho) == [0, 1, 3, 1, 3, 1, 3, 1] and den == 4


def test_footprint_twin():
    m = np.zeros((3, 5), dtype=bool)
    m[1, 2] = True
    f = twin_footprint(m, 2, 3, "nearest", False)
    want = np.zeros((6, 15), dtype=bool)
    want[2:4, 6:9] = True
    assert np.array_equal(f, want)
    # bilinear: every output pixel one of whose four corners is the pixel, zero weights included
    for align in (False, True):
        f = twin_footprint(m, 2, 3, "bilinear", align)
        y0, y1, _, _ = twin_axis(3, 2, "bilinear", align)
        x0, x1, _, _ = twin_axis(5, 3, "bilinear", align)
        rows = [o for o in range(6) if 1 in (y0[o], y1[o])]
        cols = [o for o in range(15) if 2 in (x0[o], x1[o])]
        want = np.zeros((6, 15), dtype=bool)
        want[np.ix_(rows, cols)] = True
        assert np.array_equal(f, want) and f.sum() > 6
    assert twin_footprint(np.ones((1, 1), dtype=bool), 8, 8, "bilinear", True).all()


# ------------------------------------------------------------------------------------------------ the constructor
def test_constructor_takes_and_refuses(pkg, lib):
    U = pkg.CBUpsample2d
    for m, want in ((nn.Upsample(scale_factor=2), ((2, 2), 'nearest', False)),
                    (nn.Upsample(scale_factor=3.0, mode='bilinear'), ((3, 3), 'bilinear', False)),
                    (nn.Upsample(scale_factor=(1, 8), mode='bilinear', align_corners=True), ((1, 8), 'bilinear', True)),
                    (nn.Upsample(scale_factor=(2.0, 5), mode='nearest'), ((2, 5), 'nearest', False)),
                    (nn.Upsample(scale_factor=(4, 1.0)), ((4, 1), 'nearest', False)),
                    (nn.Upsample(scale_factor=2, mode='bilinear', recompute_scale_factor=False), ((2, 2), 'bilinear', False)),
                    (nn.UpsamplingNearest2d(scale_factor=2), ((2, 2), 'nearest', False)),
                    (nn.UpsamplingBilinear2d(scale_factor=4), ((4, 4), 'bilinear', True))):
        cb = U(m)
        assert (cb.scale_factor, cb.mode, cb.align_corners) == want, m
        assert not cb.propChangeIndexes and cb.cloneOutput and cb.outputState.numel() == 0
        assert 'scale_factor=%s' % (want[0],) in repr(cb) and want[1] in repr(cb)
        assert lib.C.cbinfer_upsample_supported(cb._struct()) == 1
    for m, what in ((nn.Upsample(size=(8, 8)), "size="),
                    (nn.UpsamplingNearest2d(size=7), "size="),
                    (nn.Upsample(scale_factor=1.5), "scale_factor=1.5"),
                    (nn.Upsample(scale_factor=(2, 2.5)), "scale_factor="),
                    (nn.Upsample(scale_factor=9), "scale_factor=9"),
                    (nn.Upsample(scale_factor=(2, 16)), "scale_factor="),
                    (nn.Upsample(scale_factor=0.5), "scale_factor=0.5"),
                    (nn.Upsample(scale_factor=(2, 2, 2)), "scale_factor="),
                    (nn.Upsample(scale_factor=2, mode='bicubic'), "mode='bicubic'"),
                    (nn.Upsample(scale_factor=2, mode='nearest-exact'), "mode='nearest-exact'"),
                    (nn.Upsample(scale_factor=2, mode='area'), "mode='area'"),
                    (nn.Upsample(scale_factor=2, mode='bilinear', recompute_scale_factor=True), "recompute_scale_factor"),
                    (nn.Conv2d(3, 3, 1), "nn.Upsample")):
        with pytest.raises(lib.CBinferError, match=what):
            U(m)


# ------------------------------------------------------------------------------------------------ insertCBUpsampling
def test_insert_upsampling_structure_and_flags(pkg):
    torch.manual_seed(1)
    seq = nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), nn.ReLU(), nn.Upsample(scale_factor=2),
                        nn.Conv2d(8, 8, 3, padding=1), nn.ReLU(), nn.Upsample(scale_factor=16),
                        nn.Conv2d(8, 4, 1), nn.Upsample(size=(9, 9)), nn.Tanh(), nn.Upsample(scale_factor=2)).eval()
    net = pkg.convert(seq, threshold=0.05)
    assert list(net._modules) == ['0', '2', '3', '5', '6', '7', '8', '9']
    net[2].copyInput = False
    assert pkg.insertCBUpsampling(net, cloneOutput=False) is net
    assert [type(m).__name__ for m in net] == ['CBConv2d', 'CBUpsample2d', 'CBConv2d', 'Upsample', 'CBConv2d', 'Upsample',
                                               'Tanh', 'Upsample']
    up = net[1]
    assert (up.scale_factor, up.mode, up.cloneOutput, up.propChangeIndexes) == ((2, 2), 'nearest', False, False)
    assert net[0].propChangeIndexes and net[2].copyInput is True
    # beyond the limits, a size=, or behind a module that produces no change list: left dense, flags untouched
    assert not net[2].propChangeIndexes and not net[4].propChangeIndexes
    # behind a CBResidual (its .add hands on), another CBUpsample2d, and pools
    body = pkg.convert(nn.Sequential(nn.Conv2d(8, 8, 3, padding=1), nn.ReLU(), nn.Conv2d(8, 8, 3, padding=1)).eval(),
                       threshold=0.05)
    tail = pkg.convert(nn.Sequential(nn.Conv2d(8, 4, 3, padding=1)).eval(), threshold=0.05)[0]
    tail.copyInput, tail.feedbackLoop = False, True
    net = nn.Sequential()
    net.add_module('block', pkg.CBResidual(body))
    net.add_module('up1', nn.Upsample(scale_factor=2, mode='bilinear'))
    net.add_module('up2', nn.UpsamplingBilinear2d(scale_factor=(2, 2)))
    net.add_module('head', tail)
    pkg.insertCBUpsampling(net)
    assert type(net.up1) is pkg.CBUpsample2d and type(net.up2) is pkg.CBUpsample2d
    assert net.block.add.propChangeIndexes and net.up1.propChangeIndexes and not net.up2.propChangeIndexes
    assert net.up1.cloneOutput and net.up2.cloneOutput and (net.up1.align_corners, net.up2.align_corners) == (False, True)
    assert net.head.copyInput is False      # (feedback mode: the layer keeps no reference to its input)
    for general in (False, True):
        net = pkg.convert(nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), nn.MaxPool2d(2), nn.Upsample(scale_factor=2),
                                        nn.AvgPool2d(3, 2, 1), nn.Upsample(scale_factor=2)).eval(), threshold=0.05)
        pkg.insertCBPooling(net, generalGeometry=general)
        pkg.insertCBUpsampling(net)
        assert type(net[1]) is pkg.CBPoolMax2d and type(net[2]) is pkg.CBUpsample2d and net[1].propChangeIndexes
        assert net[1].downsampleIndexes      # (the list of the 2x2 pool's input addresses another map)
        # (an average pool that was not converted produces no change list)
        assert type(net[4]) is (pkg.CBUpsample2d if general and type(net[3]) is pkg.CBPoolAvg2d else nn.Upsample)


# ------------------------------------------------------------------------------------------------ the C ABI
def test_c_entry_points_check_their_arguments(lib):
    """Bad arguments return CB_ERR_BADARG (-1) before anything is launched (the device pointers here are never
    followed)."""
    C = lib.C
    assert C.cbinfer_abi_version() == 11
    X, O, BITS, COPY, M, L, N2 = (0x10000 * i for i in range(1, 8))

    def up_struct(sH=2, sW=3, mode=lib.UPSAMPLE_BILINEAR, ac=0):
        return ctypes.pointer(lib.Upsample(sH, sW, mode, ac))

    for good in (up_struct(), up_struct(1, 8, lib.UPSAMPLE_NEAREST, 0), up_struct(8, 1, lib.UPSAMPLE_BILINEAR, 1)):
        assert C.cbinfer_upsample_supported(good) == 1
    badStructs = (up_struct(sH=0), up_struct(sW=9), up_struct(sH=-1), up_struct(mode=2), up_struct(mode=-1), up_struct(ac=2))
    for bad in badStructs:
        assert C.cbinfer_upsample_supported(bad) == 0
    assert C.cbinfer_upsample_supported(None) == 0

    def ups(x=X, o=O, mask=None, lst=None, cap=0, count=None, bits=BITS, cp=COPY, Cn=3, Hi=4, Wi=5, up=up_struct(),
            dt=lib.CB_F32):
        return C.cbinfer_cbupsample_forward(x, o, mask, lst, cap, count, bits, cp, Cn, Hi, Wi, up, dt, None)

    for bad in (dict(x=None), dict(o=None), dict(bits=None), dict(cp=None), dict(cp=BITS), dict(up=None), dict(Cn=0),
                dict(Hi=0), dict(Wi=-1), dict(dt=lib.CB_F32S), dict(dt=7), dict(lst=L, cap=-1), dict(mask=M, lst=L),
                dict(count=N2), dict(mask=BITS), dict(mask=COPY), dict(Hi=1 << 15, Wi=1 << 14), dict(Cn=1 << 25),
                dict(Hi=1 << 16, Wi=1 << 15, up=up_struct(1, 1, lib.UPSAMPLE_NEAREST))):
        assert ups(**bad) == -1, bad
    for bad in badStructs:
        assert ups(up=bad) == -1

    def cat(srcs=(X, O), chans=(3, 2), n=None, o=N2, masks=(None, None), lists=(None, None), caps=(0, 0),
            counts=(None, None), bits=BITS, cp=COPY, H=4, W=5, dt=lib.CB_F16):
        k = len(srcs) if srcs is not None else 2
        vp = lambda vals: (ctypes.c_void_p * len(vals))(*vals) if vals is not None else None      # noqa: E731
        ip = lambda vals: (ctypes.c_int32 * len(vals))(*vals) if vals is not None else None      # noqa: E731
        return C.cbinfer_cbconcat_forward(vp(srcs), ip(chans), k if n is None else n, o, vp(masks), vp(lists), ip(caps),
                                          vp(counts), bits, cp, H, W, dt, None)

    words = 4      # (H = 4 rows of one word)
    for bad in (dict(srcs=(X, None)), dict(srcs=(None, O)), dict(srcs=None), dict(chans=None), dict(o=None),
                dict(bits=None), dict(cp=None), dict(cp=BITS), dict(cp=BITS + 8 * (2 * words - 1)), dict(chans=(3, 0)),
                dict(chans=(-1, 2)), dict(H=0), dict(W=0), dict(dt=lib.CB_F32S), dict(dt=-1), dict(n=1), dict(n=5),
                dict(srcs=(X,), chans=(3,), masks=(None,), lists=(None,), caps=(0,), counts=(None,)),
                dict(lists=(L, None), caps=(-1, 0)), dict(caps=(0, -1)), dict(masks=(M, None), lists=(L, None)),
                dict(masks=(None, M), lists=(None, L)), dict(counts=(N2, None)), dict(counts=(None, N2)),
                dict(masks=(COPY, None)), dict(masks=(None, BITS)), dict(masks=(None, BITS + 8 * words)),
                dict(H=1 << 16, W=1 << 15), dict(chans=(1 << 24, 1 << 24))):
        assert cat(**bad) == -1, bad


# ------------------------------------------------------------------------------------------------ module hygiene
def test_exports_state_helpers_and_pickling(pkg, lib):
    assert all(n in pkg.__all__ for n in ('CBUpsample2d', 'CBConcat2d', 'insertCBUpsampling'))
    assert pkg.CBUpsample2d is pkg.decoder.CBUpsample2d and pkg.CBConcat2d is pkg.decoder.CBConcat2d
    assert {'cbinfer_upsample_supported', 'cbinfer_cbupsample_forward', 'cbinfer_cbconcat_forward'} <= set(
        lib.EXPORTED_SYMBOLS)
    assert pkg.ChannelConcat is not pkg.CBConcat2d      # (the dense concat stays what it is)
    up = pkg.CBUpsample2d(nn.Upsample(scale_factor=(2, 3), mode='bilinear', align_corners=True))
    cat = pkg.CBConcat2d()
    up.propChangeIndexes, up.cloneOutput = True, False
    cat.propChangeIndexes = True
    net = nn.Sequential(up)
    net.add_module('cat', cat)
    up.outputState, cat.outputState = torch.ones(1, 2, 4, 6), torch.ones(1, 5, 4, 6)
    up._struct()
    up.__dict__['_work'] = {'key': None}
    cat.__dict__['_work'] = {'key': None}
    cat.__dict__['_channels'] = (2, 3)
    states = pkg.getStateTensors(net)
    assert any(t is up.outputState for t in states) and any(t is cat.outputState for t in states)
    for clone in (pickle.loads(pickle.dumps(net)), copy.deepcopy(net)):
        u, c = clone[0], clone.cat
        assert type(u) is pkg.CBUpsample2d and type(c) is pkg.CBConcat2d
        assert (u.scale_factor, u.mode, u.align_corners, u.propChangeIndexes, u.cloneOutput) == ((2, 3), 'bilinear', True,
                                                                                                 True, False)
        assert (c.propChangeIndexes, c.cloneOutput, c._channels) == (True, True, (2, 3))
        assert u._work is None and c._work is None and u._upC is None
        assert torch.equal(u.outputState, up.outputState) and torch.equal(c.outputState, cat.outputState)
        assert repr(u) == repr(up) and repr(c) == repr(cat) and lib.C.cbinfer_upsample_supported(u._struct()) == 1
    pkg.clearMemory(net)
    assert up.outputState.numel() == 0 and cat.outputState.numel() == 0
    assert up._work is None and cat._work is None and cat._channels is None


def test_forward_refusals_without_a_device(pkg, lib):
    up, cat = pkg.CBUpsample2d(nn.Upsample(scale_factor=2)), pkg.CBConcat2d()
    x = torch.zeros(1, 4, 5, 6)
    Err = lib.CBinferError
    for inp, what in ((torch.zeros(2, 4, 5, 6), r"\[1, C, H, W\]"), (torch.zeros(4, 5, 6), r"\[1, C, H, W\]"),
                      (('changeIndexes', x), "tuple"), (None, "must be a tensor"), (x.double(), "float32 and float16"),
                      (x, "HIP devices only")):
        with pytest.raises(Err, match=what):
            up(inp)
    for ops, what in (([x], "2..4 operands"), ([x] * 5, "2..4 operands"), (x, "LIST of operands"),
                      (('changeIndexes', x, None), "LIST of operands"),
                      ([x, torch.zeros(1, 4, 5, 7)], "operands differ"), ([x, torch.zeros(1, 2, 6, 6)], "operands differ"),
                      ([x, x.half()], "operands differ"), ([x, torch.zeros(2, 4, 5, 6)], r"\[1, C, H, W\]"),
                      ([x, ('changeIndexes', x)], "tuple"), ([x, None], "must be a tensor"),
                      ([x, x], "HIP devices only")):
        with pytest.raises(Err, match=what):
            cat(ops)


def test_batch_and_branch_refusals_name_the_layer(pkg, lib):
    for kind, mod in (("CBUpsample2d", pkg.CBUpsample2d(nn.Upsample(scale_factor=2))), ("CBConcat2d", pkg.CBConcat2d())):
        net = nn.Sequential()
        net.add_module('stem', pkg.convert(nn.Sequential(nn.Conv2d(3, 8, 3, padding=1)).eval(), threshold=0.05)[0])
        net.add_module('dec', mod)
        with pytest.raises(lib.CBinferError, match=r"SequenceBatch: layer 'dec' is %s \(" % kind):
            pkg.SequenceBatch(net, 2)
        with pytest.raises(lib.CBinferError, match=r"BranchGroup: layer '0.dec' is %s \(" % kind):
            pkg.BranchGroup([net])
