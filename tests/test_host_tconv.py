"""CPU-only tests of the change-based transposed convolution: the numpy twin of the semantics against
F.conv_transpose2d in float64, output sizes and the taps per phase against brute force, the case table of
tests/tconv_cases.py against its classifier, the argument checks of the C entry points, the settings CBConvTranspose2d
takes and refuses, what insertCBTransposedConv does to a network, exports, pickling and the refusals.  No kernel is
launched here."""
import copy
import ctypes
import pickle

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import tconv_cases as tc
from tconv_cases import CASES, case_form, case_out_hw, case_pixels, case_tags
from optest import lib, pkg      # noqa: F401  (fixtures)


# ------------------------------------------------------------------------------------------------ the twin
def twin_axis(No, Ni, k, s, p, d):
    """Per tap i of one axis: (output coordinates o with n = o + p - i d divisible by s and n / s inside the input,
    their input coordinates n / s)."""
    o = np.arange(No)
    out = []
    for i in range(k):
        n = o + p - i * d
        ok = (n >= 0) & (n % s == 0) & (n // s < Ni)
        out.append((o[ok], n[ok] // s))
    return out


def twin_tconv(x, w, b, geom, relu=False):
    """Rule 3 in float64: x [C, Hi, Wi], w [C, K, kH, kW] (torch's layout), b [K] or None -> [K, Ho, Wo]."""
    k, s, p, d, op = geom
    x, w = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64)
    Cin, Hi, Wi = x.shape
    Ho, Wo = tc.geom_out_hw(geom, Hi, Wi)
    out = np.zeros((w.shape[1], Ho, Wo))
    rows, cols = twin_axis(Ho, Hi, k[0], s[0], p[0], d[0]), twin_axis(Wo, Wi, k[1], s[1], p[1], d[1])
    for ky, (oy, iy) in enumerate(rows):
        for kx, (ox, ix) in enumerate(cols):
            if len(oy) and len(ox):
                out[:, oy[:, None], ox[None, :]] += np.einsum("ck,cyx->kyx", w[:, :, ky, kx], x[:, iy][:, :, ix])
    if b is not None:
        out += np.asarray(b, dtype=np.float64)[:, None, None]
    return np.maximum(out, 0) if relu else out


def twin_footprint(changed, geom, Ho=None, Wo=None):
    """Rule 2: the output pixels that read a changed input pixel through some tap (the exact footprint)."""
    k, s, p, d, op = geom
    Hi, Wi = changed.shape
    if Ho is None:
        Ho, Wo = tc.geom_out_hw(geom, Hi, Wi)
    listed = np.zeros((Ho, Wo), dtype=bool)
    rows, cols = twin_axis(Ho, Hi, k[0], s[0], p[0], d[0]), twin_axis(Wo, Wi, k[1], s[1], p[1], d[1])
    for oy, iy in rows:
        for ox, ix in cols:
            if len(oy) and len(ox):
                listed[oy[:, None], ox[None, :]] |= changed[iy][:, ix].astype(bool)
    return listed


def twin_reachable(geom, Hi, Wi):
    return twin_footprint(np.ones((Hi, Wi), dtype=bool), geom)


def torch_tconv64(x, w, b, geom):
    k, s, p, d, op = geom
    bb = torch.from_numpy(np.asarray(b, dtype=np.float64)) if b is not None else None
    return F.conv_transpose2d(torch.from_numpy(np.asarray(x, dtype=np.float64))[None],
                              torch.from_numpy(np.asarray(w, dtype=np.float64)), bb, stride=s, padding=p,
                              output_padding=op, dilation=d)[0].numpy()


GEOMS = dict(tc.DET_GEOMS)
GEOMS.update({
    "8x8s4d4p28op3": ((8, 8), (4, 4), (28, 28), (4, 4), (3, 3)),      # every limit at once, the padding limit too
    "5x3s3d2": ((5, 3), (3, 2), (4, 1), (2, 3), (2, 2)),
    "1x1s1": ((1, 1), (1, 1), (0, 0), (1, 1), (0, 0)),
    "2x8s1x4": ((2, 8), (1, 4), (1, 7), (4, 1), (3, 3)),
})


@pytest.mark.parametrize("name", sorted(GEOMS))
def test_twin_is_torch_in_float64(name):
    geom = GEOMS[name]
    assert tc.within_limits(geom)
    rng = np.random.default_rng(sorted(GEOMS).index(name))
    sizes = [hw for hw in ((1, 1), (2, 5), (9, 8), (8, 11)) if min(tc.geom_out_hw(geom, *hw)) >= 1]
    assert len(sizes) >= 2
    for Hi, Wi in sizes:
        x, w, b = rng.standard_normal((3, Hi, Wi)), rng.standard_normal((3, 4, geom[0][0], geom[0][1])), rng.standard_normal(4)
        want = torch_tconv64(x, w, b, geom)
        got = twin_tconv(x, w, b, geom)
        assert got.shape == want.shape == (4,) + tc.geom_out_hw(geom, Hi, Wi)
        assert np.abs(got - want).max() <= 1e-13 * max(1.0, np.abs(want).max()), name
        assert np.array_equal(twin_tconv(x, w, None, geom, relu=True), np.maximum(twin_tconv(x, w, None, geom), 0))
        # the footprint: where the transposed convolution of a changed map with a filter of ones is non-zero
        changed = rng.random((Hi, Wi)) < 0.2
        ones = np.ones((1, 1) + geom[0])
        assert np.array_equal(twin_footprint(changed, geom), torch_tconv64(changed[None].astype(float), ones, None, geom)[0] > 0)


@pytest.mark.parametrize("name", sorted(GEOMS))
def test_taps_per_phase_against_brute_force(name):
    """Rule 4: an output coordinate o reads tap i iff o + p - i d is divisible by s; that set depends on (o + p) mod s
    alone and is phase_taps.  The reachable pixels are those whose taps land inside the map."""
    k, s, p, d, op = GEOMS[name]
    for ax in (0, 1):
        No = tc.out_size(9, k[ax], s[ax], p[ax], d[ax], op[ax])
        for o in range(No):
            brute = [i for i in range(k[ax]) if (o + p[ax] - i * d[ax]) % s[ax] == 0]
            assert brute == tc.phase_taps(k[ax], d[ax], s[ax], (o + p[ax]) % s[ax]), (name, ax, o)
    taps = tc.phase_tap_counts(GEOMS[name])
    assert sum(taps) == k[0] * k[1] and len(taps) == s[0] * s[1]
    Ho, Wo = tc.geom_out_hw(GEOMS[name], 9, 8)
    reach = twin_reachable(GEOMS[name], 9, 8).reshape(-1)
    ph = tc.phase_of(GEOMS[name], Wo, np.arange(Ho * Wo))
    assert not reach[np.asarray(taps)[ph] == 0].any()      # a pixel of a phase without a tap is out of reach


def test_phases_without_a_tap():
    assert tc.phase_tap_counts(tc.T1S2) == [1, 0, 0, 0]
    assert tc.phase_tap_counts(tc.T3D2) == [9, 0, 0, 0]
    assert tc.phase_tap_counts(tc.T2S3) == [1, 1, 0, 1, 1, 0, 0, 0, 0]
    assert tc.phase_tap_counts(tc.T3) == [4, 2, 2, 1] and tc.phase_tap_counts(tc.T4) == [4] * 4
    assert tc.phase_tap_counts(tc.T7S4D4) == [49] + [0] * 15 and tc.phase_tap_counts(tc.T8S4) == [4] * 16
    assert tc.phase_tap_counts(tc.TANISO) == [5, 5, 5, 0]
    # rows and columns added by the output padding may be out of reach
    reach = twin_reachable(tc.T1S2, 3, 3)
    assert reach.shape == (6, 6) and not reach[5].any() and not reach[:, 5].any() and reach[4, 4]


# ------------------------------------------------------------------------------------------------ the C ABI, host side
def tgeom(lib, geom):
    k, s, p, d, op = geom
    return lib.TGeom(k[0], k[1], s[0], s[1], p[0], p[1], d[0], d[1], op[0], op[1])


@pytest.mark.parametrize("name", sorted(GEOMS))
def test_out_size_and_prepared_bytes_are_the_classifiers(lib, name):
    geom = GEOMS[name]
    g = tgeom(lib, geom)
    Ho, Wo = ctypes.c_int(), ctypes.c_int()
    for Hi, Wi in ((1, 1), (5, 70), (11, 130)):
        st = lib.C.cbinfer_tconv_out_size(Hi, Wi, ctypes.byref(g), ctypes.byref(Ho), ctypes.byref(Wo))
        if min(tc.geom_out_hw(geom, Hi, Wi)) < 1:      # (the padding eats the whole output of a map this small)
            assert st == -1
            continue
        assert st == 0
        assert (Ho.value, Wo.value) == tc.geom_out_hw(geom, Hi, Wi)
        x = torch.zeros(1, 1, Hi, Wi, dtype=torch.float64)
        k, s, p, d, op = geom
        assert tuple(F.conv_transpose2d(x, torch.zeros(1, 1, *k, dtype=torch.float64), None, s, p, op, 1, d).shape[2:]) == \
            (Ho.value, Wo.value)
    for K, Cin in ((1, 1), (33, 5), (70, 64), (256, 13)):
        for arith, code in tc.ARITH.items():
            assert lib.C.cbinfer_tconv_prepared_weights_bytes(K, Cin, ctypes.byref(g), code) == \
                tc.prepared_bytes(K, Cin, geom, arith), (name, K, Cin, arith)


BAD_GEOMS = {      # beyond the limits: CB_ERR_UNSUPPORTED (-2)
    "k9": ((9, 3), (2, 2), (1, 1), (1, 1), (0, 0)), "kW9": ((3, 9), (2, 2), (1, 1), (1, 1), (0, 0)),
    "s5": ((3, 3), (5, 2), (1, 1), (1, 1), (0, 0)), "sW5": ((3, 3), (2, 5), (1, 1), (1, 1), (0, 0)),
    "d5": ((3, 3), (2, 2), (1, 1), (5, 1), (0, 0)), "dW5": ((3, 3), (2, 2), (1, 1), (1, 5), (0, 0)),
    "p>d(k-1)": ((3, 3), (2, 2), (3, 1), (1, 1), (0, 0)), "pW>d(k-1)": ((3, 3), (2, 2), (1, 3), (1, 1), (0, 0)),
    "op=s": ((3, 3), (2, 2), (1, 1), (1, 1), (2, 0)), "opW=max(s,d)": ((3, 3), (2, 2), (1, 1), (1, 3), (0, 3)),
}
NONSENSE_GEOMS = {      # CB_ERR_BADARG (-1)
    "k0": ((0, 3), (2, 2), (0, 0), (1, 1), (0, 0)), "s0": ((3, 3), (2, 0), (1, 1), (1, 1), (0, 0)),
    "d0": ((3, 3), (2, 2), (1, 1), (0, 1), (0, 0)), "p-1": ((3, 3), (2, 2), (-1, 1), (1, 1), (0, 0)),
    "op-1": ((3, 3), (2, 2), (1, 1), (1, 1), (0, -1)),
}


def test_c_entry_points_check_their_arguments(lib):
    """CB_ERR_BADARG (-1) or CB_ERR_UNSUPPORTED (-2) before anything is launched (the device pointers here are never
    followed)."""
    C = lib.C
    assert C.cbinfer_abi_version() == 11
    assert {'cbinfer_tconv_out_size', 'cbinfer_tconv_prepared_weights_bytes', 'cbinfer_tconv_prep_weights',
            'cbinfer_tconv_workspace_bytes', 'cbinfer_change_detection_tconv', 'cbinfer_conv_changed_tconv',
            'cbinfer_cbconvtranspose2d_forward'} <= set(lib.EXPORTED_SYMBOLS)
    assert C.cbinfer_tconv_workspace_bytes() == 512 * 64 * 64 * 4 + 2048
    X, S, O, BITS, WP, B, L, WS, W = (0x10000 * i for i in range(1, 10))
    good = tgeom(lib, tc.T3)
    gp = ctypes.byref(good)

    def prep(w=W, wp=WP, K=8, Cin=4, Hi=5, Wi=6, g=gp, dt=lib.CB_F32S):
        return C.cbinfer_tconv_prep_weights(w, wp, K, Cin, Hi, Wi, g, dt, None)

    def detect(x=X, s=S, bits=BITS, Cin=4, Hi=5, Wi=6, g=gp, upd=1, dt=lib.CB_F32):
        return C.cbinfer_change_detection_tconv(x, s, bits, Cin, Hi, Wi, g, 0.1, upd, dt, None)

    def conv(x=X, lst=None, n=0, cnt=None, bits=BITS, wp=WP, out=O, Cin=4, Hi=5, Wi=6, K=8, g=gp, dt=lib.CB_F32S):
        return C.cbinfer_conv_changed_tconv(x, lst, n, cnt, bits, wp, B, out, Cin, Hi, Wi, K, g, 0, WS, dt, None)

    def fwd(x=X, s=S, out=O, bits=BITS, wp=WP, Cin=4, Hi=5, Wi=6, K=8, g=gp, dt=lib.CB_F32S):
        return C.cbinfer_cbconvtranspose2d_forward(x, s, out, bits, wp, B, Cin, Hi, Wi, K, g, 0.1, 1, 1, 0, WS, dt, None)

    calls = {"prep": prep, "detect": detect, "conv": conv, "fwd": fwd}
    null = {"prep": ("w", "wp", "g"), "detect": ("x", "s", "bits", "g"), "conv": ("x", "wp", "out", "g"),
            "fwd": ("x", "s", "out", "bits", "wp", "g")}
    for name, fn in calls.items():
        for arg in null[name]:
            assert fn(**{arg: None}) == -1, (name, arg)
        for arg in ("Cin", "Hi", "Wi") + (() if name == "detect" else ("K",)):
            for v in (0, -3):
                assert fn(**{arg: v}) == -1, (name, arg, v)
        for dt in (3, -1) + ((lib.CB_F32S,) if name == "detect" else ()):      # (the detection has no arithmetic)
            assert fn(dt=dt) == -1, (name, dt)
        # beyond an int32: Ho Wo (2 x 40000 by 2 x 40000), C Hi Wi, K Ho Wo
        assert fn(Hi=40000, Wi=40000, Cin=1) == -1, name
        assert fn(Cin=1 << 20, Hi=64, Wi=64) == -1, name
        if name != "detect":
            assert fn(K=1 << 20, Hi=32, Wi=32) == -1, name
        for gname, geom in BAD_GEOMS.items():
            assert fn(g=ctypes.byref(tgeom(lib, geom))) == -2, (name, gname)
        for gname, geom in NONSENSE_GEOMS.items():
            assert fn(g=ctypes.byref(tgeom(lib, geom))) == -1, (name, gname)
    assert detect(upd=3) == -1 and detect(upd=-1) == -1
    # the contraction: neither a mask nor a list; both; a negative capacity or one beyond the map; a count with a mask
    assert conv(bits=None) == -1 and conv(lst=L, n=4) == -1 and conv(bits=BITS, cnt=L) == -1
    assert conv(bits=None, lst=L, n=-1) == -1 and conv(bits=None, lst=L, n=10 * 12 + 1) == -1
    assert conv(bits=None, lst=L, n=0) == 0      # an empty list: nothing to do, nothing launched
    # the size helpers
    Ho, Wo = ctypes.c_int(7), ctypes.c_int(7)
    assert C.cbinfer_tconv_out_size(5, 6, None, ctypes.byref(Ho), ctypes.byref(Wo)) == -1
    assert C.cbinfer_tconv_out_size(0, 6, gp, ctypes.byref(Ho), ctypes.byref(Wo)) == -1
    assert C.cbinfer_tconv_out_size(5, 6, gp, None, ctypes.byref(Wo)) == -1
    assert C.cbinfer_tconv_out_size(5, 6, ctypes.byref(tgeom(lib, BAD_GEOMS["k9"])), ctypes.byref(Ho), ctypes.byref(Wo)) == -2
    assert (Ho.value, Wo.value) == (7, 7)
    for geom in list(BAD_GEOMS.values()) + list(NONSENSE_GEOMS.values()):
        assert C.cbinfer_tconv_prepared_weights_bytes(8, 4, ctypes.byref(tgeom(lib, geom)), lib.CB_F32) == 0
    assert C.cbinfer_tconv_prepared_weights_bytes(8, 4, None, lib.CB_F32) == 0
    assert C.cbinfer_tconv_prepared_weights_bytes(0, 4, gp, lib.CB_F32) == 0
    assert C.cbinfer_tconv_prepared_weights_bytes(8, 4, gp, 5) == 0


# ------------------------------------------------------------------------------------------------ the case table
IDS = [c.id for c in CASES]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_case_reaches_what_it_claims(case):
    px = case_pixels(case)
    Ho, Wo = case_out_hw(case)
    assert len(px) >= 1 and px.dtype == np.int32 and np.all(np.diff(px) > 0) and px[0] >= 0 and px[-1] < Ho * Wo
    assert np.array_equal(px, case_pixels(case))
    f = case_form(case, px)
    tags = case_tags(case)
    assert set(case.claims) <= tags, (case.id, sorted(tags), f)
    assert tags <= set(tc.TAGS)
    # the stage count of a tile is CkkP_ph / 32 -- no stage is spent on another phase's taps
    for ph, t in enumerate(f["taps"]):
        assert f["CkkP"][ph] == -(-case.C * t // 32) * 32 and f["stages"][ph] * 32 == f["CkkP"][ph]
        assert (f["tiles"][ph] == 0) == (t == 0 or f["counts"][ph] == 0)
    assert sum(f["stages"]) * 32 < case.C * case.geom[0][0] * case.geom[0][1] + 32 * len(f["taps"])
    # the k-split never outgrows the slabs (one per workgroup) or the tickets (one per tile)
    if f["SKmax"] > 1:
        assert f["items"] <= tc.GRID and f["base"] < tc.GRID
    assert tc.within_limits(case.geom) and case.K in (1, 33, 64, 70, 256)
    assert tc.reference_macs(case) <= tc.REF_MAC_CAP
    if isinstance(case.pixels[0], int):
        assert f["counts"] == list(case.pixels)
    if case.pixels == ("last",):
        wpr = (Wo + 63) // 64
        assert px[0] == (Ho - 1) * Wo + (wpr - 1) * 64 + (Wo - 1) % 64


def test_every_required_feature_is_reached_by_every_arithmetic():
    for arith in ("F32S", "F32", "F16"):
        mine = [c for c in CASES if c.arith == arith]
        claimed = set().union(*[set(c.claims) for c in mine])
        assert set(tc.REQUIRED) <= claimed, (arith, sorted(set(tc.REQUIRED) - claimed))
        assert {"mask", "list"} == {c.source for c in mine}
        assert {c.K for c in mine} == {1, 33, 64, 70, 256}
        assert any(c.C % 8 for c in mine) and any(c.C == 8 and c.geom == tc.T2 for c in mine)
    for ids in (tc.DEVICE_COUNT_IDS, tc.OUT_OF_MAP_IDS):
        assert all(tc.CASE_BY_ID[i].source == "list" for i in ids)
        assert {tc.CASE_BY_ID[i].arith for i in ids} == {"F32S", "F32", "F16"}
    for i in tc.OUT_OF_MAP_IDS:       # room for the foreign entries within numChanges <= Ho Wo
        Ho, Wo = case_out_hw(tc.CASE_BY_ID[i])
        assert len(case_pixels(tc.CASE_BY_ID[i])) + 40 <= Ho * Wo


def test_the_shapes_the_table_was_written_for():
    f = tc.tconv_form(70, 64, tc.T3, [65, 10, 1, 3], True, 18)
    assert (f["stages"], f["SK"], f["base"], f["items"]) == ([8, 4, 4, 2], [8, 4, 4, 2], 10, 52)
    f = tc.tconv_form(64, 24, tc.T3, [10, 10, 10, 10], True, 40)
    assert (f["stages"], f["SK"], f["SKmax"]) == ([3, 2, 2, 1], [3, 2, 2, 1], 8)
    f = tc.tconv_form(256, 5, tc.T2, [2304] * 4, True, 192)
    assert (f["base"], f["items"], f["SK"]) == (576, 576, [1] * 4)
    f = tc.tconv_form(33, 8, tc.T2, [64, 1, 63, 65], True, 10)
    assert (f["Ckk"], f["stages"], f["tiles"]) == ([8] * 4, [1] * 4, [1, 1, 1, 2])
    assert tc.tconv_form(33, 8, tc.T2, [64, 1, 63, 65], False, 10)["SKmax"] == 1
    # a transposed layer on the general-geometry kernel would spend C kH kW / 32 stages per tile: 4x as many at stride 2
    assert sum(tc.tconv_form(64, 128, tc.T4, [1] * 4, True, 1)["stages"]) == 128 * 16 // 32
    assert tc.mask_words(130, 258) == 650 and tc.mask_words(100, 200) == 400
    # the widest reach: a 64-pixel input segment at s = 4, k = 7, d = 4 reaches six output words
    k, s, p, d, op = tc.T7S4D4
    lo, hi = 64 * s[1] - p[1], (64 + 63) * s[1] - p[1] + (k[1] - 1) * d[1]
    assert (hi >> 6) - (lo >> 6) + 1 == 6
    runs = tc.detection_runs("2x2s2")
    assert {(C, m) for C, _, _, m in runs} == {(C, m) for C in tc.DET_C for m in tc.DET_MODES}
    assert {(W, m) for _, _, W, m in runs} == {(W, m) for W in tc.DET_WI for m in tc.DET_MODES}
    assert max(H for _, H, _, _ in runs) == 11 and set(tc.DET_GEOMS) >= {"7x7s4d4p6op3", "3x3s1p1", "aniso"}


# ------------------------------------------------------------------------------------------------ the constructor
def test_constructor_takes_and_refuses(pkg, lib):
    T = pkg.CBConvTranspose2d
    for name, geom in GEOMS.items():
        k, s, p, d, op = geom
        src = nn.ConvTranspose2d(3, 5, k, s, p, op, 1, name != "aniso", d)
        m = T(src, 0.05)
        assert (m.kernel_size, m.stride, m.padding, m.dilation, m.output_padding) == geom, name
        assert m.weight is src.weight and m.bias is src.bias and m.threshold == 0.05
        assert (m.in_channels, m.out_channels) == (3, 5)
        assert (m.withReLU, m.propChangeIndexes, m.copyInput, m.feedbackLoop, m.exactF32, m.cloneOutput) == \
            (False, False, True, False, False, True)
    refusals = (
        (nn.ConvTranspose2d(4, 4, 9, 2, 1), "kernel_size"), (nn.ConvTranspose2d(4, 4, (3, 9), 2, 1), "kernel_size"),
        (nn.ConvTranspose2d(4, 4, 3, 5, 1), "stride"), (nn.ConvTranspose2d(4, 4, 3, (1, 8), 1), "stride"),
        (nn.ConvTranspose2d(4, 4, 3, 2, 1, dilation=5), "dilation"),
        (nn.ConvTranspose2d(4, 4, 3, 2, 3), "padding"), (nn.ConvTranspose2d(4, 4, (3, 1), 2, (0, 1)), "padding"),
        (nn.ConvTranspose2d(4, 4, 3, 2, 1, groups=2), "groups"), (nn.ConvTranspose2d(4, 4, 3, 2, 1, groups=4), "groups"),
        (nn.Conv2d(4, 4, 3), "nn.ConvTranspose2d"), (nn.ConvTranspose1d(4, 4, 3), "nn.ConvTranspose2d"),
    )
    for src, word in refusals:
        with pytest.raises(lib.CBinferError, match="CBConvTranspose2d: .*%s" % word):
            T(src, 0.05)
    # torch's own rule for output_padding, restated (a module that broke it by hand)
    src = nn.ConvTranspose2d(4, 4, 3, 2, 1)
    src.output_padding = (2, 0)
    with pytest.raises(lib.CBinferError, match="CBConvTranspose2d: output_padding"):
        T(src, 0.05)
    # CBConv2d still says what it said
    with pytest.raises(lib.CBinferError, match="no transposed convolution"):
        pkg.CBConv2d(nn.ConvTranspose2d(4, 4, 3), 0.05, generalGeometry=True)


# ------------------------------------------------------------------------------------------------ insertCBTransposedConv
def test_insert_transposed_conv_structure_and_flags(pkg):
    torch.manual_seed(1)
    seq = nn.Sequential(
        nn.Conv2d(3, 8, 3, padding=1), nn.ReLU(), nn.ConvTranspose2d(8, 8, 2, 2), nn.ReLU(),      # -> 0 (ReLU merged), 1
        nn.Conv2d(8, 8, 3, padding=1), nn.ReLU(), nn.ConvTranspose2d(8, 8, 16, 8, 4),            # beyond the limits
        nn.Conv2d(8, 4, 1), nn.ConvTranspose2d(4, 4, 4, 2, 1), nn.ConvTranspose2d(4, 4, 3, 2, 1, 1), nn.Tanh(),
        nn.ConvTranspose2d(4, 2, 2, 2)).eval()                                                   # behind a torch operator
    net = pkg.convert(seq, threshold=0.05)
    names = [type(m).__name__ for m in net]
    assert names.count("ConvTranspose2d") == 5      # convert() itself is unchanged
    dense = [m for m in net if type(m) is nn.ConvTranspose2d]
    out = pkg.insertCBTransposedConv(net, threshold=0.2, cloneOutput=False)
    assert out is net
    kinds = [type(m).__name__ for m in net]
    assert kinds == ["CBConv2d", "CBConvTranspose2d", "CBConv2d", "ConvTranspose2d", "CBConv2d", "CBConvTranspose2d",
                     "CBConvTranspose2d", "Tanh", "ConvTranspose2d"], kinds
    first, chained, last = net[1], net[5], net[6]
    assert first.withReLU and first.threshold == 0.2 and not first.cloneOutput and first.weight is dense[0].weight
    assert net[2].copyInput and not net[2].feedbackLoop      # the consumer of the first keeps its own input copy
    assert not chained.withReLU and not last.withReLU and last.output_padding == (1, 1)
    assert net[3] is dense[1] and net[8] is dense[4]
    assert not net[0].propChangeIndexes      # the layer runs its own detection: nothing is switched on at the producer
    # defaults; a feedback consumer keeps its flag; nothing happens outside an nn.Sequential's direct pairs
    seq2 = pkg.convert(nn.Sequential(nn.Conv2d(3, 4, 3, padding=1), nn.ConvTranspose2d(4, 4, 2, 2),
                                     nn.Conv2d(4, 4, 3, padding=1)).eval(), threshold=0.05)
    seq2[2].feedbackLoop, seq2[2].copyInput = True, False
    pkg.insertCBTransposedConv(seq2)
    assert type(seq2[1]) is pkg.CBConvTranspose2d and seq2[1].threshold == 1e-1 and seq2[1].cloneOutput
    assert seq2[2].feedbackLoop and not seq2[2].copyInput
    lone = nn.Sequential(nn.ConvTranspose2d(3, 4, 2, 2), nn.ReLU())
    pkg.insertCBTransposedConv(lone)
    assert type(lone[0]) is nn.ConvTranspose2d and len(lone) == 2
    # behind the other producers of insertCBUpsampling's list, a CBUpsample2d included
    up = pkg.convert(nn.Sequential(nn.Conv2d(3, 4, 3, padding=1), nn.Upsample(scale_factor=2),
                                   nn.ConvTranspose2d(4, 4, 4, 2, 1)).eval(), threshold=0.05)
    pkg.insertCBTransposedConv(pkg.insertCBUpsampling(up))
    assert [type(m).__name__ for m in up] == ["CBConv2d", "CBUpsample2d", "CBConvTranspose2d"]


# ------------------------------------------------------------------------------------------------ module hygiene
def test_exports_state_helpers_and_pickling(pkg, lib):
    assert all(n in pkg.__all__ for n in ('CBConvTranspose2d', 'insertCBTransposedConv'))
    assert pkg.CBConvTranspose2d is pkg.tconv.CBConvTranspose2d
    import pycbinfer.tconv
    assert pycbinfer.tconv.insertCBTransposedConv is pkg.insertCBTransposedConv
    m = pkg.CBConvTranspose2d(nn.ConvTranspose2d(3, 5, 4, 2, 1), 0.05)
    net = nn.Sequential(m)
    assert [t.numel() for t in pkg.getStateTensors(net)] == [0, 0]
    assert set(dict(m.named_buffers())) == {'prevInput', 'prevOutput'}
    m._struct()
    m.__dict__['_work'] = {'key': None}
    m.withReLU = True
    for clone in (pickle.loads(pickle.dumps(m)), copy.deepcopy(m)):
        assert clone._work is None and clone._wprep is None and clone._geomC is None
        assert clone.withReLU and clone.kernel_size == (4, 4) and clone.threshold == 0.05
        assert torch.equal(clone.weight, m.weight)
        assert clone._struct().contents.sH == 2 and clone._struct().contents.kW == 4
    pkg.clearMemory(net)
    assert m._work is None and m.prevInput.numel() == 0 and m.prevOutput.numel() == 0
    assert "CBConvTranspose2d" in repr(m) and "withReLU=True" in repr(m)


def test_forward_refusals_without_a_device(pkg, lib):
    m = pkg.CBConvTranspose2d(nn.ConvTranspose2d(4, 5, 2, 2), 0.05)
    Err = lib.CBinferError
    for inp, what in ((torch.zeros(2, 4, 5, 6), r"\[1, 4, H, W\]"), (torch.zeros(4, 5, 6), r"\[1, 4, H, W\]"),
                      (torch.zeros(1, 3, 5, 6), r"\[1, 4, H, W\]"), (torch.zeros(1, 4, 5, 6), "HIP devices only"),
                      (('indexes', torch.zeros(1, 4, 5, 6), None), "not \\('changeIndexes'"),
                      ([torch.zeros(1, 4, 5, 6)], "must be a tensor")):
        with pytest.raises(Err, match=what):
            m(inp)


def test_batch_and_branch_refusals_name_the_layer(pkg, lib):
    net = nn.Sequential()
    net.add_module('stem', pkg.convert(nn.Sequential(nn.Conv2d(3, 8, 3, padding=1)).eval(), threshold=0.05)[0])
    net.add_module('up', pkg.CBConvTranspose2d(nn.ConvTranspose2d(8, 4, 2, 2), 0.05))
    with pytest.raises(lib.CBinferError, match=r"SequenceBatch: layer 'up' is CBConvTranspose2d \("):
        pkg.SequenceBatch(net, 2)
    with pytest.raises(lib.CBinferError, match=r"BranchGroup: layer '0.up' is CBConvTranspose2d \("):
        pkg.BranchGroup([net])
    import cbinfer_amd.program as program
    import inspect
    assert "CBConvTranspose2d" in inspect.getsource(program.FrameProgram)
