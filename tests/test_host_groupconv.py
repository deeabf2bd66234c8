"""CPU: the change-based grouped convolution without a device (cb_groupconv.hip, cbinfer_amd/groupconv.py)
-- cbinfer_groupconv_supported on both sides of every limit, the prepared-bytes formula, the argument checks of the three
launching entry points (nothing is launched), what CBGroupedConv2d takes and refuses, convert(..., grouped=True),
mergeReLURecur, linkGrouped, the refusals of SequenceBatch / BranchGroup, pickling, the coverage of the case table of
tests/groupconv_cases.py, and the resources of the kernel instances read from the code-object metadata."""
import ctypes
import inspect
import os
import pickle
import re
import subprocess

import pytest
import torch
import torch.nn as nn

import groupconv_cases as gc
from groupconv_cases import CASES, SHAPES
from optest import lib, pkg      # noqa: F401  (fixtures)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "cbinfer_amd", "csrc")


def cgeom(lib, geom):
    k, s, p, d = geom
    return lib.Geom(k[0], k[1], s[0], s[1], p[0], p[1], d[0], d[1])


G3 = ((3, 3), (1, 1), (1, 1), (1, 1))
BAD_GEOMS = {      # CB_ERR_UNSUPPORTED (-2): one step beyond each limit
    "k8": ((8, 3), (1, 1), (1, 1), (1, 1)), "s5": ((3, 3), (1, 5), (1, 1), (1, 1)),
    "d9": ((3, 3), (1, 1), (1, 1), (9, 1)), "p65": ((3, 3), (1, 1), (1, 65), (1, 1)),
}
AT_LIMIT_GEOMS = {      # ... and at it
    "k7": ((7, 3), (1, 1), (1, 1), (1, 1)), "s4": ((3, 3), (1, 4), (1, 1), (1, 1)),
    "d8": ((3, 3), (1, 1), (1, 1), (8, 1)), "p64": ((3, 3), (1, 1), (1, 64), (1, 1)),
    "widest": ((7, 7), (4, 4), (64, 64), (8, 8)),
}
NONSENSE_GEOMS = {      # CB_ERR_BADARG (-1)
    "k0": ((0, 3), (1, 1), (0, 0), (1, 1)), "s0": ((3, 3), (1, 0), (1, 1), (1, 1)),
    "d0": ((3, 3), (1, 1), (1, 1), (0, 1)), "p-1": ((3, 3), (1, 1), (-1, 1), (1, 1)),
}


# ------------------------------------------------------------------------------------------------ the C entry points
def test_supported_on_both_sides_of_every_limit(lib):
    C = lib.C
    good = ctypes.byref(cgeom(lib, G3))
    sup = C.cbinfer_groupconv_supported
    assert sup(128, 128, 32, good) == 1 and sup(6, 10, 2, good) == 1
    assert sup(8, 16, 8, good) == 1      # (depthwise: accepted, not the fast path)
    assert sup(8, 8, 1, good) == 0 and sup(8, 8, 2, good) == 1      # groups >= 2
    assert sup(8, 8, 0, good) == 0 and sup(8, 8, -2, good) == 0
    assert sup(9, 8, 2, good) == 0 and sup(8, 9, 2, good) == 0 and sup(9, 9, 3, good) == 1      # divisibility
    assert sup(8, 4, 8, good) == 0      # (K < groups does not divide)
    assert sup(0, 8, 2, good) == 0 and sup(8, 0, 2, good) == 0 and sup(8, 8, 2, None) == 0
    for name, geom in list(BAD_GEOMS.items()) + list(NONSENSE_GEOMS.items()):
        assert sup(8, 8, 2, ctypes.byref(cgeom(lib, geom))) == 0, name
    for name, geom in AT_LIMIT_GEOMS.items():
        assert sup(8, 8, 2, ctypes.byref(cgeom(lib, geom))) == 1, name


@pytest.mark.parametrize("Kg, rows, KgP", [(1, 16, 16), (16, 16, 16), (17, 32, 32), (32, 32, 32), (33, 64, 64),
                                           (64, 64, 64), (65, 64, 128), (80, 64, 128), (129, 64, 192)])
def test_prepared_bytes_formula_at_each_rows(lib, Kg, rows, KgP):
    """G KgP CkkgP elemSize + 8 CkkgP, KgP = Kg rounded up to ROWS, CkkgP = Cg kH kW rounded up to 32; 0 if rejected."""
    nbytes = lib.C.cbinfer_groupconv_prepared_weights_bytes
    assert gc.rows_of(Kg) == rows
    for G, Cg, geom in ((2, 3, G3), (32, 4, G3), (3, 8, ((1, 1), (1, 1), (0, 0), (1, 1))), (2, 2, AT_LIMIT_GEOMS["widest"])):
        (kH, kW) = geom[0]
        gp = ctypes.byref(cgeom(lib, geom))
        CkkgP = (Cg * kH * kW + 31) // 32 * 32
        for dt, elem in ((lib.CB_F32, 4), (lib.CB_F32S, 4), (lib.CB_F16, 2)):
            want = G * KgP * CkkgP * elem + 8 * CkkgP
            assert nbytes(G * Kg, G * Cg, G, gp, dt) == want == gc.prepared_bytes(G, Cg, Kg, kH, kW, elem), (G, Cg, dt)
    good = ctypes.byref(cgeom(lib, G3))
    assert nbytes(8, 8, 1, good, lib.CB_F32) == 0 and nbytes(9, 8, 2, good, lib.CB_F32) == 0
    assert nbytes(8, 8, 2, ctypes.byref(cgeom(lib, BAD_GEOMS["k8"])), lib.CB_F32) == 0
    assert nbytes(8, 8, 2, None, lib.CB_F32) == 0


def test_c_entry_points_check_their_arguments(lib):
    """CB_ERR_BADARG (-1) or CB_ERR_UNSUPPORTED (-2) before anything is launched (the device pointers here are never
    followed)."""
    C = lib.C
    assert C.cbinfer_abi_version() == 11
    names = {'cbinfer_groupconv_supported', 'cbinfer_groupconv_prepared_weights_bytes', 'cbinfer_groupconv_prep_weights',
             'cbinfer_conv_changed_grouped', 'cbinfer_cbgroupconv2d_forward'}
    assert names <= set(lib.EXPORTED_SYMBOLS)
    # the launching ones go through the recording wrappers, the host helpers do not
    assert {n for n in names if getattr(C, n).launcher} == {'cbinfer_groupconv_prep_weights',
                                                            'cbinfer_conv_changed_grouped',
                                                            'cbinfer_cbgroupconv2d_forward'}
    X, S, O, FM, W, WP, B, L, IDX, CNT = (0x10000 * i for i in range(1, 11))
    gp = ctypes.byref(cgeom(lib, G3))

    def prep(w=W, wp=WP, K=8, Cin=4, G=2, Hi=5, Wi=6, g=gp, dt=lib.CB_F32):
        return C.cbinfer_groupconv_prep_weights(w, wp, K, Cin, G, Hi, Wi, g, dt, None)

    def changed(x=X, lst=None, n=0, cnt=None, fm=FM, idx=IDX, count=CNT, wp=WP, out=O, Cin=4, Hi=5, Wi=6, K=8, G=2, g=gp,
                dt=lib.CB_F32):
        return C.cbinfer_conv_changed_grouped(x, lst, n, cnt, fm, idx, count, wp, B, out, Cin, Hi, Wi, K, G, g, 1, dt, None)

    def fwd(x=X, s=S, out=O, fm=FM, idx=IDX, count=CNT, wp=WP, Cin=4, Hi=5, Wi=6, K=8, G=2, g=gp, dt=lib.CB_F32):
        return C.cbinfer_cbgroupconv2d_forward(x, s, out, fm, idx, count, wp, B, Cin, Hi, Wi, K, G, g, 0.1, 1, 1, 1, dt,
                                               None)

    calls = {"prep": prep, "changed": changed, "fwd": fwd}
    null = {"prep": ("w", "wp", "g"), "changed": ("x", "wp", "out", "g"),
            "fwd": ("x", "s", "out", "fm", "idx", "count", "wp", "g")}
    for name, fn in calls.items():
        for arg in null[name]:
            assert fn(**{arg: None}) == -1, (name, arg)
        for arg in ("Cin", "K", "G", "Hi", "Wi"):
            for v in (0, -3):
                assert fn(**{arg: v}) == -1, (name, arg, v)
        for dt in (3, -1):
            assert fn(dt=dt) == -1, (name, dt)
        assert fn(Hi=2, Wi=2, g=ctypes.byref(cgeom(lib, ((3, 3), (1, 1), (0, 0), (1, 1))))) == -1, name   # (filter too large)
        # groups: 1, or no divisor of C or of K
        assert fn(G=1) == -2 and fn(Cin=5) == -2 and fn(K=9) == -2 and fn(Cin=4, K=8, G=3) == -2, name
        for gname, geom in BAD_GEOMS.items():
            assert fn(g=ctypes.byref(cgeom(lib, geom))) == -2, (name, gname)
        for gname, geom in NONSENSE_GEOMS.items():
            assert fn(g=ctypes.byref(cgeom(lib, geom))) == -1, (name, gname)
        # the tap table's group-relative byte offsets are ints: Cg Hi Wi elemSize < 2^31, on both sides
        assert fn(Cin=2 * 2048, K=2, Hi=512, Wi=512) == -2, name             # 2^29 elements x 4 bytes
        assert fn(Cin=2 * 4096, K=2, Hi=512, Wi=512, dt=lib.CB_F16) == -2, name
        assert fn(Hi=1 << 15, Wi=1 << 15, Cin=2, K=2, dt=lib.CB_F16) == -2, name      # Hi Wi >= 2^30
        # Ho Wo >= 2^31
        assert fn(Cin=2, K=2, Hi=1, Wi=(1 << 24), g=ctypes.byref(cgeom(lib, ((1, 1), (1, 1), (64, 0), (1, 1))))) == -1, name
    assert prep(Cin=2 * 2047, K=2, Hi=512, Wi=512, w=None) == -1      # (just inside: judged by its other arguments)
    # the contraction: exactly one list source
    assert changed(lst=L, n=3) == -1 and changed(idx=None) == -1 and changed(count=None) == -1
    assert changed(fm=None) == -1 and changed(fm=None, lst=L, n=-1) == -1 and changed(fm=None, lst=L, n=5 * 6 + 1) == -1
    assert changed(fm=None, lst=L, n=0) == 0      # (an empty host list: nothing to do, nothing launched)
    # the whole frame: one grid row per input row (cbinfer_change_detection_geom)
    assert fwd(Cin=2, K=2, Hi=65536, Wi=3) == -2


# ------------------------------------------------------------------------------------------------ the module
def grp(C=8, K=8, G=2, k=3, s=1, p=1, d=1, **kw):
    return nn.Conv2d(C, K, k, s, p, d, groups=G, **kw)


def test_constructor_takes_and_refuses(pkg, lib):
    D = pkg.CBGroupedConv2d
    for name, (k, s, p, d) in AT_LIMIT_GEOMS.items():
        m = D(nn.Conv2d(6, 12, k, s, p, d, groups=3, bias=name != "k7"), 0.05)
        assert (m.kernel_size, m.stride, m.padding, m.dilation) == (k, s, p, d), name
        assert m.weight.shape == (12, 2) + k and (m.bias is None) == (name == "k7")
    src = grp(6, 10, 2)
    m = D(src, 0.1)
    assert m.weight is src.weight and m.bias is src.bias and m.threshold == 0.1 and m.groups == 2
    assert (m.feedbackLoop, m.copyInput, m.withReLU, m.exactF32, m.propChangeIndexes, m.cloneOutput) == (
        False, True, False, False, False, True)
    assert D(grp(4, 4, 2, 3, 1, 'same'), 0.1).padding == (1, 1) and D(grp(4, 4, 2, 3, 2, 'valid'), 0.1).padding == (0, 0)
    assert D(grp(8, 16, 8), 0.1).groups == 8      # (depthwise: taken)
    refused = [
        (nn.Conv2d(8, 8, 3, groups=1), "groups=1 is not a grouped convolution: use CBConv2d"),
        (nn.ConvTranspose2d(8, 8, 3, groups=2), "only plain nn.Conv2d"),
        (nn.Linear(3, 3), "only plain nn.Conv2d"),
        (grp(padding_mode='reflect'), "padding_mode='reflect'"),
        (grp(8, 8, 2, 4, 1, 'same'), "padding='same' with kernel_size"),
        (grp(8, 8, 2, (8, 3)), "kernel_size=\\(8, 3\\)"),
        (grp(8, 8, 2, 3, (1, 5)), "stride=\\(1, 5\\)"),
        (grp(8, 8, 2, 3, 1, 1, (9, 1)), "dilation=\\(9, 1\\)"),
        (grp(8, 8, 2, 3, 1, (1, 65)), "padding=\\(1, 65\\)"),
    ]
    for mod, word in refused:
        with pytest.raises(lib.CBinferError, match="CBGroupedConv2d: .*%s" % word):
            D(mod, 0.1)
    # what CBConv2d and CBDepthwiseConv2d accept is what it was
    with pytest.raises(AssertionError):
        pkg.CBConv2d(grp(), 0.1)
    with pytest.raises(lib.CBinferError, match="grouped and depthwise convolutions are not supported"):
        pkg.CBConv2d(grp(), 0.1, generalGeometry=True)
    with pytest.raises(lib.CBinferError, match="groups=2 with in_channels=8"):
        pkg.CBDepthwiseConv2d(grp(), 0.1)


def resnext():
    return nn.Sequential(nn.Conv2d(8, 16, 1), nn.ReLU(), grp(16, 16, 4), nn.ReLU(), nn.Conv2d(16, 32, 1),
                         nn.Sequential(grp(32, 32, 8, 3, 2), nn.ReLU6(), nn.Dropout(), nn.Conv2d(32, 8, 3, padding=1)),
                         nn.Conv2d(8, 8, 3, padding=1, groups=8), nn.ReLU())


def test_convert_default_still_refuses(pkg, lib):
    for kw in ({}, {'depthwise': True}):
        with pytest.raises(AssertionError):
            pkg.convert(resnext(), **kw)
        with pytest.raises(lib.CBinferError, match="grouped and depthwise convolutions are not supported \\(groups=4\\)"):
            pkg.convert(resnext(), generalGeometry=True, **kw)
    for fn in (pkg.convert, pkg.convertRecur, pkg.subsitute):
        assert inspect.signature(fn).parameters['grouped'].default is False
    plain = nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), nn.ReLU(), nn.Conv2d(8, 4, 1))
    assert repr(pkg.convert(plain)) == repr(pkg.convert(plain, grouped=True))


def test_convert_grouped_structure_names_and_relus(pkg):
    src = resnext()
    net = pkg.convert(src, threshold=0.07, generalGeometry=True, grouped=True)
    assert list(net._modules) == ['0', '2', '4', '5', '6']
    c0, g2, c4, inner, g6 = list(net)
    assert type(c0) is pkg.CBConv2d and c0.withReLU
    assert type(g2) is pkg.CBGroupedConv2d and g2.withReLU and g2.threshold == 0.07 and g2.groups == 4
    assert g2.weight is src[2].weight and g2.bias is src[2].bias
    assert type(c4) is pkg.CBConv2d and not c4.withReLU
    # an nn.ReLU6 behind a CBGroupedConv2d stays the dense module it is
    assert list(inner._modules) == ['0', '1', '3']
    assert type(inner[0]) is pkg.CBGroupedConv2d and not inner[0].withReLU and inner[0].stride == (2, 2)
    assert type(inner[1]) is nn.ReLU6 and inner[1] is src[5][1] and type(inner[2]) is pkg.CBConv2d
    # without depthwise=True the depthwise layer is a grouped one as well ...
    assert type(g6) is pkg.CBGroupedConv2d and g6.groups == 8 and g6.withReLU
    # ... with it, it goes to CBDepthwiseConv2d
    net = pkg.convert(resnext(), generalGeometry=True, grouped=True, depthwise=True)
    assert [type(m).__name__ for m in net] == ["CBConv2d", "CBGroupedConv2d", "CBConv2d", "Sequential",
                                               "CBDepthwiseConv2d"]
    # without generalGeometry a stride-1 / padding-k/2 network converts too
    net2 = pkg.convert(nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), grp(), nn.ReLU()), grouped=True)
    assert [type(m).__name__ for m in net2] == ["CBConv2d", "CBGroupedConv2d"] and net2[1].withReLU


def test_merge_relu_recur(pkg):
    G = pkg.CBGroupedConv2d
    seq = nn.Sequential(G(grp(), 0.1), nn.ReLU(), nn.Sequential(G(grp(), 0.1), nn.ReLU6()), G(grp(), 0.1), nn.ReLU6(),
                        G(grp(), 0.1))
    out = pkg.mergeReLURecur(seq)
    assert [type(m).__name__ for m in out] == ["CBGroupedConv2d", "Sequential", "CBGroupedConv2d", "ReLU6",
                                               "CBGroupedConv2d"]
    assert out[0].withReLU and not out[2].withReLU and not out[4].withReLU
    assert [type(m).__name__ for m in out[1]] == ["CBGroupedConv2d", "ReLU6"] and not out[1][0].withReLU


def test_link_grouped_flags(pkg):
    net = pkg.convert(resnext(), generalGeometry=True, grouped=True)
    for m in net.modules():
        if type(m) is pkg.CBConv2d:
            m.copyInput = False
    assert pkg.linkGrouped(net) is net
    c0, g2, c4, inner, g6 = list(net)
    assert g2.propChangeIndexes and not c4.copyInput         # in front of a 1x1 / stride-1 / padding-0 CBConv2d
    assert not c0.propChangeIndexes                          # (the grouped layer detects for itself)
    assert not inner[0].propChangeIndexes                    # an nn.ReLU6 stands between
    assert not inner[2].copyInput                            # (not DIRECTLY behind the grouped layer)
    assert not g6.propChangeIndexes
    # a 3x3 CBConv2d directly behind: its own input copy, unless it runs in feedback mode; a strided 1x1 is no 1x1 consumer
    for feedback in (False, True):
        net = pkg.convert(nn.Sequential(grp(), nn.Conv2d(8, 8, 3, padding=1), grp(), nn.Conv2d(8, 8, 1, stride=2)),
                          generalGeometry=True, grouped=True)
        for m in (net[1], net[3]):
            m.copyInput, m.feedbackLoop = False, feedback
        pkg.linkGrouped(net)
        assert not net[0].propChangeIndexes and not net[2].propChangeIndexes
        assert net[1].copyInput == (not feedback) and net[3].copyInput == (not feedback)
    # the passes written before the module have not taken it as a producer (every pass's whole set: test_host_chain.py)
    from cbinfer_amd import chain
    assert not any(pkg.CBGroupedConv2d in chain.producers(name) for name in (
        'linkDepthwise', 'insertCBPointwise', 'insertCBTransposedConv', 'insertCBUpsampling', 'insertCBPooling',
        'insertCBPooling(generalGeometry=True)'))


def test_exports_state_helpers_and_pickling(pkg, lib):
    assert all(n in pkg.__all__ for n in ('CBGroupedConv2d', 'linkGrouped'))
    import pycbinfer.groupconv
    assert pkg.CBGroupedConv2d is pkg.groupconv.CBGroupedConv2d is pycbinfer.groupconv.CBGroupedConv2d
    m = pkg.CBGroupedConv2d(grp(6, 12, 3, 5, 2, 2), 0.05)
    m.withReLU, m.propChangeIndexes, m.exactF32, m.feedbackLoop = True, True, True, True
    m._struct()
    m.__dict__['_wprep'] = ("key", torch.zeros(3))
    m.prevOutput = torch.ones(1, 12, 4, 4)
    m2 = pickle.loads(pickle.dumps(m))
    assert m2.__dict__['_geomC'] is None and m2.__dict__['_work'] is None and m2.__dict__['_wprep'] is None
    assert m.__dict__['_wprep'] is not None
    m.invalidateWeights()
    assert m.__dict__['_wprep'] is None
    assert (m2.kernel_size, m2.stride, m2.padding, m2.dilation, m2.groups) == ((5, 5), (2, 2), (2, 2), (1, 1), 3)
    assert m2.withReLU and m2.propChangeIndexes and m2.exactF32 and m2.feedbackLoop and m2.threshold == 0.05
    assert torch.equal(m2.prevOutput, m.prevOutput) and torch.equal(m2.weight, m.weight)
    assert m2._struct().contents.kH == 5
    net = nn.Sequential(m, nn.Sequential(pkg.CBGroupedConv2d(grp(12, 12, 4), 0.1)))
    states = pkg.getStateTensors(net)
    assert len(states) == 4 and states[1] is m.prevOutput
    pkg.clearMemory(net)
    assert all(t.numel() == 0 for t in pkg.getStateTensors(net)) and m.__dict__['_work'] is None
    r = repr(m)
    assert "CBGroupedConv2d" in r and "groups=3" in r and "withReLU=True" in r and "propChgIdxs=True" in r


def test_forward_refusals_without_a_device(pkg, lib):
    m = pkg.CBGroupedConv2d(grp(4, 4, 2), 0.05)
    with pytest.raises(lib.CBinferError, match="CBGroupedConv2d: .*not \\('changeIndexes', tensor, indexes\\)"):
        m(('indexes', torch.zeros(1, 4, 4, 4)))
    with pytest.raises(lib.CBinferError, match="CBGroupedConv2d: .*must be a tensor"):
        m([1, 2])
    with pytest.raises(lib.CBinferError, match="CBGroupedConv2d: .*must be a \\[1, 4, H, W\\] tensor"):
        m(torch.zeros(1, 3, 4, 4))
    with pytest.raises(lib.CBinferError, match="CBGroupedConv2d: .*must be a \\[1, 4, H, W\\] tensor"):
        m(torch.zeros(2, 4, 4, 4))
    with pytest.raises(lib.CBinferError, match="HIP devices only"):
        m(torch.zeros(1, 4, 4, 4))


def test_batch_and_branch_refusals_name_the_layer(pkg, lib):
    net = pkg.convert(nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), nn.ReLU()))
    net.add_module('gc', pkg.CBGroupedConv2d(grp(), 0.05))
    with pytest.raises(lib.CBinferError, match=r"SequenceBatch: layer 'gc' is CBGroupedConv2d \(.*a change-based grouped "
                                               r"convolution.*ResNeXt-type networks"):
        pkg.SequenceBatch(net, 2)
    with pytest.raises(lib.CBinferError, match=r"BranchGroup: layer '0.gc' is CBGroupedConv2d \(.*a change-based grouped "
                                               r"convolution"):
        pkg.BranchGroup([net])
    from cbinfer_amd import program
    assert "CBGroupedConv2d" in program.__doc__


# ------------------------------------------------------------------------------------------------ the case table
def test_the_table_covers_what_it_must(lib):
    cells = set()
    for c in CASES:
        f = gc.case_form(c)
        assert gc.cell_of(c, f) == gc.claimed_cell(c), (c.id, gc.cell_of(c, f), f)
        cells.add(gc.cell_of(c, f))
        s = SHAPES[c.shape]
        gp = ctypes.byref(cgeom(lib, s.geom))
        assert lib.C.cbinfer_groupconv_supported(s.G * s.Cg, s.G * s.Kg, s.G, gp) == 1, c.id
        Ho, Wo = ctypes.c_int(), ctypes.c_int()
        assert lib.C.cbinfer_geom_out_size(s.Hi, s.Wi, gp, ctypes.byref(Ho), ctypes.byref(Wo)) == 0
        assert (Ho.value, Wo.value) == gc.shape_out_hw(s), c.id
        px = gc.shape_pixels(c.shape)
        assert len(px) and np_sorted_distinct(px) and 0 <= px[0] and px[-1] < Ho.value * Wo.value, c.id
    assert len(CASES) <= 30
    assert {(a, r) for a, r, _, _, _ in cells} == {(a, r) for a in gc.ARITH for r in gc.ROWS_CLASSES}
    assert {(r, s) for _, r, s, _, _ in cells} == {(r, s) for r in gc.ROWS_CLASSES for s in gc.SOURCES}
    assert {s for _, _, s, sched, _ in cells if sched == "multi_item"} == set(gc.SOURCES)
    assert {st for _, _, _, _, st in cells} == set(gc.STAGE_CLASSES)
    for ids in (gc.INDEPENDENCE_IDS, gc.DEVICE_COUNT_IDS, gc.OUT_OF_MAP_IDS):
        assert all(i in gc.CASE_BY_ID for i in ids)
    assert {gc.claimed_cell(gc.CASE_BY_ID[i])[1] for i in gc.INDEPENDENCE_IDS} == set(gc.ROWS_CLASSES)
    assert all(gc.CASE_BY_ID[i].source == "list" for i in gc.DEVICE_COUNT_IDS + gc.OUT_OF_MAP_IDS)
    # what the table says about its shapes
    f = gc.case_form(gc.CASE_BY_ID["resnext-narrow-f32s-mask"])
    assert (f["tilesN"], f["items"], f["stages"], f["Ckkg"], f["KgP"]) == (17, 544, 2, 36, 16)
    f = gc.case_form(gc.CASE_BY_ID["rows64-two-tiles-f32s-mask"])
    assert (f["KgP"], f["rowTiles"], f["stages"]) == (128, 2, 7)
    f = gc.case_form(gc.CASE_BY_ID["wide-reach-f32s-list"])
    assert (f["ROWS"], f["KgP"], f["stages"]) == (64, 64, 4)
    f = gc.case_form(gc.CASE_BY_ID["mask-650w-f32s-mask"])
    assert f["words"] == 650 and f["chunk"] == 3
    assert gc.shape_out_hw(SHAPES["odd-pad"]) == (11, 66)
    reach = gc.reachable_map(SHAPES["unreachable"])
    assert reach.shape == (10, 14) and not reach[0].any() and not reach[:, -1].any() and reach[1:-1, 1:-1].all()
    assert gc.shape_pixels("shuffle-1x1").tolist() == [5 * 130 - 1]


def np_sorted_distinct(px):
    return bool((px[1:] > px[:-1]).all())


# ------------------------------------------------------------------------------------------------ the generated code
def _metadata(text):
    """{kernel name: {field: value}} from the code object metadata of a listing (as tools/kernel_regs.py reads it)."""
    meta = text[text.index("amdhsa.kernels:"):]
    out = {}
    for blk in meta.split("  - .agpr_count:")[1:]:
        f = dict(re.findall(r"\.(\w+):\s+(\S+)", blk))
        out[f["name"]] = f
    return out


def test_kernel_instances_use_no_scratch_and_fit_the_lds(tmp_path):
    """cb_groupconv.hip compiled to gfx950 assembly: every kernel instance -- 3 arithmetics x 3 ROWS of the contraction,
    2 of the weight preparation -- has no scratch and no spilled register, and at most 64 KB of static LDS.  Only the
    code-object metadata is read.  The register counts are printed as a record, not judged."""
    out = os.path.join(str(tmp_path), "cb_groupconv.s")
    subprocess.check_call(["hipcc", "-O3", "--offload-arch=gfx950", "-std=c++17", "-fopenmp", "--cuda-device-only", "-S",
                           "-I", CSRC, os.path.join(CSRC, "cb_groupconv.hip"), "-o", out], stderr=subprocess.DEVNULL)
    with open(out) as f:
        meta = _metadata(f.read())
    conv = {k: v for k, v in meta.items() if "cbgr_conv_kernel" in k}
    prep = {k: v for k, v in meta.items() if "cbgr_prep_kernel" in k}
    assert len(conv) == 9 and len(prep) == 2 and len(meta) == 11, sorted(meta)
    for name, f in sorted(meta.items()):
        print("%s: vgpr %s agpr %s sgpr %s lds %s scratch %s" % (name, f["vgpr_count"], f.get("agpr_count", "0"),
                                                                  f["sgpr_count"], f["group_segment_fixed_size"],
                                                                  f["private_segment_fixed_size"]))
        assert int(f["private_segment_fixed_size"]) == 0, name
        assert int(f["vgpr_spill_count"]) == 0 and int(f.get("sgpr_spill_count", 0)) == 0, name
        assert int(f["group_segment_fixed_size"]) <= 64 * 1024, name
