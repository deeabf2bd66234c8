"""CPU: the change-based depthwise convolution without a device (cb_dwconv.hip, cbinfer_amd/dwconv.py) --
the numpy twin of the per-channel sum against float64 torch on every case of tests/dwconv_cases.py, the coverage of the
case table, the argument checks of the four C entry points (nothing is launched), what CBDepthwiseConv2d takes and
refuses, convert(..., depthwise=True), linkDepthwise, the refusals of SequenceBatch / BranchGroup, pickling and the state
helpers."""
import ctypes
import inspect
import pickle

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import dwconv_cases as dc
from dwconv_cases import CASES, GEOMS
from optest import lib, pkg      # noqa: F401  (fixtures)


def cgeom(lib, geom):
    k, s, p, d = geom
    return lib.Geom(k[0], k[1], s[0], s[1], p[0], p[1], d[0], d[1])


def conv64(x, w, b, geom, C):
    """float64 CPU depthwise convolution of torch tensors: THE value reference."""
    k, s, p, d = geom
    return F.conv2d(x.detach().cpu().double(), w.detach().cpu().double(),
                    b.detach().cpu().double() if b is not None else None, stride=s, padding=p, dilation=d, groups=C)


# ------------------------------------------------------------------------------------------------ twin and case table
@pytest.mark.parametrize("cid", [c.id for c in CASES])
def test_twin_is_torch_in_float64(cid):
    c = dc.CASE_BY_ID[cid]
    rng = np.random.default_rng(len(cid))
    k = c.geom[0]
    x = rng.standard_normal((c.C, c.Hi, c.Wi))
    w = rng.standard_normal((c.C * c.mult, 1, k[0], k[1]))
    b = rng.standard_normal(c.C * c.mult)
    for bias in (b, None):
        out, mag, reach = dc.twin(x, w, bias, c.geom, c.mult)
        tb = torch.from_numpy(bias) if bias is not None else None
        ref = conv64(torch.from_numpy(x)[None], torch.from_numpy(w), tb, c.geom, c.C)[0].numpy()
        assert out.shape == ref.shape == (c.C * c.mult, c.Ho, c.Wo)
        assert np.abs(out - ref).max() <= 1e-12 * max(1.0, np.abs(mag).max())
        absref = conv64(torch.from_numpy(np.abs(x))[None], torch.from_numpy(np.abs(w)),
                        tb.abs() if tb is not None else None, c.geom, c.C)[0].numpy()
        assert np.abs(mag - absref).max() <= 1e-12 * max(1.0, absref.max())
        ones = F.conv2d(torch.ones(1, 1, c.Hi, c.Wi), torch.ones(1, 1, *k), stride=c.geom[1], padding=c.geom[2],
                        dilation=c.geom[3])[0, 0].numpy() > 0
        assert np.array_equal(reach, ones)
    for act in (dc.ACT_RELU, dc.ACT_RELU6):
        out, _, _ = dc.twin(x * 8, w, b, c.geom, c.mult, act)
        ref = conv64(torch.from_numpy(x * 8)[None], torch.from_numpy(w), torch.from_numpy(b), c.geom, c.C)[0]
        ref = torch.relu(ref) if act == dc.ACT_RELU else F.relu6(ref)
        assert np.abs(out - ref.numpy()).max() <= 1e-10


def test_the_table_covers_what_it_must(lib):
    plain = [c for c in CASES if c is not dc.WALK]
    assert len(CASES) <= 60
    for name, geom in GEOMS.items():
        mine = [c for c in plain if c.geom == geom]
        assert len({(c.C, c.mult, c.Ho, c.Wo) for c in mine}) >= 2, name
        assert lib.C.cbinfer_dwconv_supported(1, 1, ctypes.byref(cgeom(lib, geom))) == 1, name
    assert {(c.C, c.mult) for c in plain} == set(dc.CMS)
    assert {c.Wo for c in plain} == set(dc.WOS) and {c.Ho for c in plain} == set(dc.HOS)
    # below, at and across the 16-channel block; a ring of unreachable pixels; a partial and a full last word
    ks = {c.C * c.mult for c in plain}
    assert min(ks) < dc.CBLOCK and dc.CBLOCK in ks and any(k > dc.CBLOCK and k % dc.CBLOCK for k in ks)
    _, _, reach = dc.twin(np.zeros((1, 5, 5)), np.zeros((1, 1, 3, 3)), None, GEOMS["3x3p3"], 1)
    assert reach.shape == (9, 9) and not reach[0].any() and not reach[:, -1].any() and reach[1:-1, 1:-1].all()
    for c in plain:
        units, groups = dc.units_of(c)
        assert units == groups, c.id      # (one unit per workgroup)
        Ho, Wo = ctypes.c_int(), ctypes.c_int()
        assert lib.C.cbinfer_geom_out_size(c.Hi, c.Wi, ctypes.byref(cgeom(lib, c.geom)), ctypes.byref(Ho),
                                           ctypes.byref(Wo)) == 0
        assert (Ho.value, Wo.value) == (c.Ho, c.Wo), c.id
    units, groups = dc.units_of(dc.WALK)
    assert groups == dc.GRID_CAP and units > groups and units % groups, (units, groups)      # several units, unevenly


# ------------------------------------------------------------------------------------------------ the C entry points
BAD_GEOMS = {      # CB_ERR_UNSUPPORTED (-2)
    "k8": ((8, 3), (1, 1), (1, 1), (1, 1)), "s5": ((3, 3), (1, 5), (1, 1), (1, 1)),
    "d9": ((3, 3), (1, 1), (1, 1), (9, 1)), "p65": ((3, 3), (1, 1), (1, 65), (1, 1)),
}
NONSENSE_GEOMS = {      # CB_ERR_BADARG (-1)
    "k0": ((0, 3), (1, 1), (0, 0), (1, 1)), "s0": ((3, 3), (1, 0), (1, 1), (1, 1)),
    "d0": ((3, 3), (1, 1), (1, 1), (0, 1)), "p-1": ((3, 3), (1, 1), (-1, 1), (1, 1)),
}


def test_supported_and_the_refusals(lib):
    C = lib.C
    good = ctypes.byref(cgeom(lib, GEOMS["3x3s1p1"]))
    assert C.cbinfer_dwconv_supported(32, 1, good) == 1 and C.cbinfer_dwconv_supported(3, 4, good) == 1
    assert C.cbinfer_dwconv_supported(0, 1, good) == 0 and C.cbinfer_dwconv_supported(3, 0, good) == 0
    assert C.cbinfer_dwconv_supported(3, 1, None) == 0
    assert C.cbinfer_dwconv_supported(1 << 20, 1 << 10, good) == 0
    for name, geom in list(BAD_GEOMS.items()) + list(NONSENSE_GEOMS.items()):
        assert C.cbinfer_dwconv_supported(3, 1, ctypes.byref(cgeom(lib, geom))) == 0, name
    widest = ((7, 7), (4, 4), (64, 64), (8, 8))
    assert C.cbinfer_dwconv_supported(3, 1, ctypes.byref(cgeom(lib, widest))) == 1


def test_c_entry_points_check_their_arguments(lib):
    """CB_ERR_BADARG (-1) or CB_ERR_UNSUPPORTED (-2) before anything is launched (the device pointers here are never
    followed)."""
    C = lib.C
    assert C.cbinfer_abi_version() == 11
    assert {'cbinfer_dwconv_supported', 'cbinfer_dwconv_changed', 'cbinfer_cbdwconv2d_forward',
            'cbinfer_cbdwconv2d_forward_propagated'} <= set(lib.EXPORTED_SYMBOLS)
    X, S, O, FM, BITS, COPY, W, B, L, CNT, IM = (0x10000 * i for i in range(1, 12))
    gp = ctypes.byref(cgeom(lib, GEOMS["3x3s1p1"]))

    def changed(x=X, w=W, out=O, fm=FM, bits=None, copy=None, Cin=4, mult=2, Hi=5, Wi=6, g=gp, act=0, dt=lib.CB_F32):
        return C.cbinfer_dwconv_changed(x, w, B, out, fm, bits, copy, Cin, mult, Hi, Wi, g, act, dt, None)

    def fwd(x=X, s=S, out=O, fm=FM, w=W, Cin=4, mult=2, Hi=5, Wi=6, g=gp, act=0, dt=lib.CB_F32):
        return C.cbinfer_cbdwconv2d_forward(x, s, out, fm, w, B, Cin, mult, Hi, Wi, g, 0.1, 1, 1, act, dt, None)

    def prop(x=X, out=O, lst=L, cap=4, cnt=None, im=None, every=0, bits=BITS, copy=COPY, w=W, Cin=4, mult=2, Hi=5, Wi=6,
             g=gp, act=0, dt=lib.CB_F32):
        return C.cbinfer_cbdwconv2d_forward_propagated(x, out, lst, cap, cnt, im, every, bits, copy, w, B, Cin, mult, Hi,
                                                       Wi, g, act, dt, None)

    calls = {"changed": changed, "fwd": fwd, "prop": prop}
    null = {"changed": ("x", "w", "out", "g"), "fwd": ("x", "s", "out", "fm", "w", "g"),
            "prop": ("x", "out", "bits", "copy", "w", "g")}
    for name, fn in calls.items():
        for arg in null[name]:
            assert fn(**{arg: None}) == -1, (name, arg)
        for arg in ("Cin", "mult", "Hi", "Wi"):
            for v in (0, -3):
                assert fn(**{arg: v}) == -1, (name, arg, v)
        for dt in (lib.CB_F32S, 3, -1):      # (no bf16-triple arithmetic: f32 FMAs on exact operands)
            assert fn(dt=dt) == -1, (name, dt)
        for act in (3, -1):
            assert fn(act=act) == -1, (name, act)
        assert fn(Hi=2, Wi=2, g=ctypes.byref(cgeom(lib, GEOMS["3x3s1p0"]))) == -1, name      # (smaller than the filter)
        # beyond an int32: 64 C mult (bad argument); K Ho Wo and C Hi Wi 4 (the guards of cbinfer_conv_changed_geom)
        assert fn(Cin=1 << 20, mult=1 << 6) == -1, name
        assert fn(Cin=4, mult=1 << 16, Hi=128, Wi=128) == -2, name
        assert fn(Cin=1 << 16, mult=1, Hi=64, Wi=64) == -2, name
        for gname, geom in BAD_GEOMS.items():
            assert fn(g=ctypes.byref(cgeom(lib, geom))) == -2, (name, gname)
        for gname, geom in NONSENSE_GEOMS.items():
            assert fn(g=ctypes.byref(cgeom(lib, geom))) == -1, (name, gname)
    # the stencil: exactly one form -- neither, both, half of the second, bits == maskCopy
    assert changed(fm=None) == -1 and changed(bits=BITS, copy=COPY) == -1 and changed(fm=None, bits=BITS) == -1
    assert changed(fm=None, copy=COPY) == -1 and changed(fm=None, bits=BITS, copy=BITS) == -1
    # propagated: exactly one of list and mask (unless every pixel is listed), a count only with a list, a capacity >= 0,
    # the input mask none of the layer's own, bits != maskCopy
    assert prop(lst=None) == -1 and prop(im=IM) == -1 and prop(lst=None, im=IM, cnt=CNT) == -1
    assert prop(cap=-1) == -1 and prop(copy=BITS) == -1
    assert prop(lst=None, im=BITS) == -1 and prop(lst=None, im=COPY) == -1
    # ... and only where the filter's footprint is a pool window's: dilation 1, p <= k / 2
    for name in GEOMS:
        g = ctypes.byref(cgeom(lib, GEOMS[name]))
        if not dc.propagated_ok(GEOMS[name]):
            assert prop(Hi=16, Wi=16, g=g) == -2 and prop(Hi=16, Wi=16, g=g, lst=None, every=1) == -2, name
    assert {n for n in GEOMS if not dc.propagated_ok(GEOMS[n])} == {"3x3d2p2", "3x3s2d2p2", "aniso", "3x3p3"}
    # the whole frame with its own detection: one grid row per input row (cbinfer_change_detection_geom)
    assert fwd(Cin=1, mult=1, Hi=65536, Wi=3) == -2


# ------------------------------------------------------------------------------------------------ the module
def dw(C=8, mult=1, k=3, s=1, p=1, d=1, **kw):
    return nn.Conv2d(C, C * mult, k, s, p, d, groups=C, **kw)


def test_constructor_takes_and_refuses(pkg, lib):
    D = pkg.CBDepthwiseConv2d
    for name, (k, s, p, d) in GEOMS.items():
        m = D(nn.Conv2d(6, 12, k, s, p, d, groups=6, bias=name != "aniso"), 0.05)
        assert (m.kernel_size, m.stride, m.padding, m.dilation) == (k, s, p, d), name
        assert m.weight.shape == (12, 1) + k and (m.bias is None) == (name == "aniso")
    src = dw(5, 3)
    m = D(src, 0.1)
    assert m.weight is src.weight and m.bias is src.bias and m.threshold == 0.1
    assert (m.feedbackLoop, m.copyInput, m.withReLU, m.reluCap, m.propChangeIndexes, m.cloneOutput,
            m.propagatedChanges) == (False, True, False, None, False, True, False)
    assert D(dw(4, 1, 3, 1, 'same'), 0.1).padding == (1, 1) and D(dw(4, 1, 3, 2, 'valid'), 0.1).padding == (0, 0)
    assert D(dw(4, 1, 3, 1, 'same', 2), 0.1).padding == (2, 2)
    assert D(dw(1, 1), 0.1).in_channels == 1      # (groups == in_channels == 1 is a depthwise layer too)
    refused = [
        (nn.Conv2d(8, 8, 3, groups=1), "groups=1 with in_channels=8"),
        (nn.Conv2d(8, 8, 3, groups=2), "groups=2 with in_channels=8"),
        (nn.ConvTranspose2d(8, 8, 3, groups=8), "only plain nn.Conv2d"),
        (nn.Linear(3, 3), "only plain nn.Conv2d"),
        (dw(8, padding_mode='reflect'), "padding_mode='reflect'"),
        (dw(8, 1, 4, 1, 'same'), "padding='same' with kernel_size"),
        (dw(8, 1, (8, 3)), "kernel_size=\\(8, 3\\)"),
        (dw(8, 1, 3, (1, 5)), "stride=\\(1, 5\\)"),
        (dw(8, 1, 3, 1, 1, (9, 1)), "dilation=\\(9, 1\\)"),
        (dw(8, 1, 3, 1, (1, 65)), "padding=\\(1, 65\\)"),
    ]
    for mod, word in refused:
        with pytest.raises(lib.CBinferError, match="CBDepthwiseConv2d: .*%s" % word):
            D(mod, 0.1)
    # the refusals of CBConv2d are what they were
    with pytest.raises(AssertionError):
        pkg.CBConv2d(dw(8), 0.1)
    with pytest.raises(lib.CBinferError, match="grouped and depthwise convolutions are not supported"):
        pkg.CBConv2d(dw(8), 0.1, generalGeometry=True)
    m = D(dw(4), 0.1)
    m.withReLU, m.reluCap = True, 5.0
    with pytest.raises(lib.CBinferError, match="reluCap=5.0"):
        m._act()


def separable():
    return nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), nn.ReLU(), dw(8), nn.ReLU6(), nn.Conv2d(8, 16, 1), nn.ReLU6(),
                         nn.Sequential(dw(16, 2, 3, 2), nn.ReLU(), nn.Dropout(), nn.Conv2d(32, 8, 1)), dw(8, 1, 3, 1, 2, 2))


def test_convert_default_is_unchanged(pkg, lib):
    with pytest.raises(AssertionError):
        pkg.convert(separable())
    with pytest.raises(lib.CBinferError, match="grouped and depthwise convolutions are not supported \\(groups=8\\)"):
        pkg.convert(separable(), generalGeometry=True)
    grouped = nn.Sequential(nn.Conv2d(8, 8, 3, padding=1, groups=2))
    for kw in ({}, {'depthwise': True}):
        with pytest.raises(AssertionError):
            pkg.convert(grouped, **kw)
        with pytest.raises(lib.CBinferError, match="groups=2"):
            pkg.convert(grouped, generalGeometry=True, **kw)
    for fn in (pkg.convert, pkg.convertRecur, pkg.subsitute):
        assert inspect.signature(fn).parameters['depthwise'].default is False
    # without a depthwise layer the keyword changes nothing
    plain = nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), nn.ReLU(), nn.Conv2d(8, 4, 1))
    assert repr(pkg.convert(plain)) == repr(pkg.convert(plain, depthwise=True))


def test_convert_depthwise_structure_names_and_relus(pkg, lib):
    src = separable()
    net = pkg.convert(src, threshold=0.07, generalGeometry=True, depthwise=True)
    assert list(net._modules) == ['0', '2', '4', '5', '6', '7']
    c0, d2, c4, r5, inner, d7 = list(net)
    assert type(c0) is pkg.CBConv2d and c0.withReLU
    assert type(d2) is pkg.CBDepthwiseConv2d and d2.withReLU and d2.reluCap == 6.0 and d2.threshold == 0.07
    assert d2.weight is src[2].weight and d2.bias is src[2].bias
    # an nn.ReLU6 behind a CBConv2d stays the dense module it is
    assert type(c4) is pkg.CBConv2d and not c4.withReLU and type(r5) is nn.ReLU6 and r5 is src[5]
    assert list(inner._modules) == ['0', '3']
    assert type(inner[0]) is pkg.CBDepthwiseConv2d and inner[0].withReLU and inner[0].reluCap is None
    assert inner[0].stride == (2, 2) and inner[0].out_channels == 32 and type(inner[1]) is pkg.CBConv2d
    assert type(d7) is pkg.CBDepthwiseConv2d and not d7.withReLU and d7.dilation == (2, 2)
    # without generalGeometry the stride-1 / padding-k/2 network converts as well
    net2 = pkg.convert(nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), dw(8), nn.ReLU()), depthwise=True)
    assert [type(m).__name__ for m in net2] == ["CBConv2d", "CBDepthwiseConv2d"] and net2[1].withReLU


def test_link_depthwise_flags(pkg):
    net = pkg.convert(separable(), generalGeometry=True, depthwise=True)
    assert pkg.linkDepthwise(net) is net
    c0, d2, c4, r5, inner, d7 = list(net)
    assert d2.propagatedChanges and c0.propChangeIndexes      # behind a CBConv2d
    assert d2.propChangeIndexes                               # in front of a 1x1 / stride-1 / padding-0 CBConv2d
    assert not c4.propChangeIndexes
    assert not inner[0].propagatedChanges and inner[0].propChangeIndexes      # first of its container: detects for itself
    assert not d7.propagatedChanges and not d7.propChangeIndexes              # behind a container; dilation 2
    # dilation 2 behind a producer: outside the propagated limits, nothing is switched on
    net = pkg.convert(nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), dw(8, 1, 3, 1, 2, 2), nn.Conv2d(8, 8, 3, padding=1)),
                      depthwise=True, generalGeometry=True)
    pkg.linkDepthwise(net)
    assert not net[1].propagatedChanges and not net[0].propChangeIndexes and not net[1].propChangeIndexes
    # behind another depthwise layer, a transposed convolution, a residual sum
    chain = nn.Sequential(nn.Conv2d(4, 4, 3, padding=1), nn.ConvTranspose2d(4, 4, 2, 2), dw(4), dw(4, 1, 5, 2, 2))
    net = pkg.insertCBTransposedConv(pkg.convert(chain, depthwise=True))
    pkg.linkDepthwise(net)
    assert [type(m).__name__ for m in net] == ["CBConv2d", "CBConvTranspose2d", "CBDepthwiseConv2d", "CBDepthwiseConv2d"]
    assert net[1].propChangeIndexes and net[2].propagatedChanges and net[2].propChangeIndexes and net[3].propagatedChanges
    res = nn.Sequential(pkg.CBResidual(pkg.convert(nn.Sequential(nn.Conv2d(4, 4, 3, padding=1)))),
                        pkg.CBDepthwiseConv2d(dw(4), 0.1))
    pkg.linkDepthwise(res)
    assert res[0].add.propChangeIndexes and res[1].propagatedChanges
    # the new class is a producer for the decoder insertions
    dec = pkg.convert(nn.Sequential(dw(4), nn.Upsample(scale_factor=2), dw(4), nn.ConvTranspose2d(4, 4, 2, 2)),
                      depthwise=True)
    pkg.insertCBTransposedConv(pkg.insertCBUpsampling(dec))
    assert [type(m).__name__ for m in dec] == ["CBDepthwiseConv2d", "CBUpsample2d", "CBDepthwiseConv2d",
                                               "CBConvTranspose2d"]
    assert dec[0].propChangeIndexes


def test_exports_state_helpers_and_pickling(pkg, lib):
    assert all(n in pkg.__all__ for n in ('CBDepthwiseConv2d', 'linkDepthwise'))
    import pycbinfer.dwconv
    assert pkg.CBDepthwiseConv2d is pkg.dwconv.CBDepthwiseConv2d is pycbinfer.dwconv.CBDepthwiseConv2d
    m = pkg.CBDepthwiseConv2d(dw(3, 2, 5, 2, 2), 0.05)
    m.withReLU, m.reluCap, m.propChangeIndexes, m.propagatedChanges = True, 6.0, True, True
    m._struct()
    m.prevOutput = torch.ones(1, 6, 4, 4)
    m2 = pickle.loads(pickle.dumps(m))
    assert m2.__dict__['_geomC'] is None and m2.__dict__['_work'] is None
    assert (m2.kernel_size, m2.stride, m2.padding, m2.dilation) == ((5, 5), (2, 2), (2, 2), (1, 1))
    assert m2.withReLU and m2.reluCap == 6.0 and m2.propChangeIndexes and m2.propagatedChanges and m2.threshold == 0.05
    assert torch.equal(m2.prevOutput, m.prevOutput) and torch.equal(m2.weight, m.weight)
    assert m2._struct().contents.kH == 5 and m2._act() == lib.ACT_RELU6
    net = nn.Sequential(m, nn.Sequential(pkg.CBDepthwiseConv2d(dw(6), 0.1)))
    states = pkg.getStateTensors(net)
    assert len(states) == 4 and states[1] is m.prevOutput
    pkg.clearMemory(net)
    assert all(t.numel() == 0 for t in pkg.getStateTensors(net)) and m.__dict__['_work'] is None
    r = repr(m)
    assert "CBDepthwiseConv2d" in r and "withReLU=True" in r and "reluCap=6.0" in r and "propagated=True" in r


def test_forward_refusals_without_a_device(pkg, lib):
    m = pkg.CBDepthwiseConv2d(dw(4), 0.05)
    with pytest.raises(lib.CBinferError, match="not \\('changeIndexes', tensor, indexes\\)"):
        m(('indexes', torch.zeros(1, 4, 4, 4)))
    with pytest.raises(lib.CBinferError, match="must be a tensor"):
        m([1, 2])
    with pytest.raises(lib.CBinferError, match="must be a \\[1, 4, H, W\\] tensor"):
        m(torch.zeros(1, 3, 4, 4))
    with pytest.raises(lib.CBinferError, match="HIP devices only"):
        m(torch.zeros(1, 4, 4, 4))


def test_batch_and_branch_refusals_name_the_layer(pkg, lib):
    net = pkg.convert(nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), nn.ReLU()))
    net.add_module('dw', pkg.CBDepthwiseConv2d(dw(8), 0.05))
    with pytest.raises(lib.CBinferError, match=r"SequenceBatch: layer 'dw' is CBDepthwiseConv2d \("):
        pkg.SequenceBatch(net, 2)
    with pytest.raises(lib.CBinferError, match=r"BranchGroup: layer '0.dw' is CBDepthwiseConv2d \("):
        pkg.BranchGroup([net])
    from cbinfer_amd import program
    assert "CBDepthwiseConv2d" in inspect.getsource(program.FrameProgram) or "CBDepthwiseConv2d" in program.__doc__
