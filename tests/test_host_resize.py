"""Host tests of the change-based resize (CBResize2d, insertCBResize; cb_resize.hip): the numpy twin of
the header's rules (tests/resize_cases.py) against float64 and against torch's CPU operators, the footprint as the list
kernel builds it against brute force, the constructor, the limits, the entry point's argument checks and the passes."""
import copy
import ctypes
import inspect
import pickle

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import resize_cases as rc
from optest import dev, lib, pkg      # noqa: F401  (fixtures)

U24 = 2.0 ** -24      # the largest relative error of one f32 rounding
# Sums of the absolute rounding errors of an axis' weights, in units of U24, from one rounding per operation:
#   bilinear: t carries U24 t, 1 - t that and U24 (1 - t) of its own: 2 at most.
#   bicubic:  far(s), s = t + 1 or 2 - t in [1, 2] with an error of 3: the chain A s (|.| <= 1.5), + 3.75 (<= 3), s
#             (<= 6), - 6 (<= 3), s (<= 3.1), + 3 carries 3.75, 6.75, 28.5, 31.5, 75.1 and 75.2 at most;
#             near(u), u = t or 1 - t in [0, 1] with an error of 2: 1.25 u, - 2.25, u, u, + 1 carries 3.75, 6, 11.52,
#             14.56 and 15.56 at most.  Two of each: 2 (75.2 + 15.56) < 184.
E_WEIGHTS = {rc.BILINEAR: 2.0, rc.BICUBIC: 184.0}
S_WEIGHTS = {rc.BILINEAR: 1.0, rc.BICUBIC: 1.375}      # the sum of an axis' absolute weights, at most (t = 1/2)
TERMS = {rc.BILINEAR: 2, rc.BICUBIC: 4}


def f32_bar_units(mode):
    """|twin_f32 - float64 rules| <= units U24 max|tap| before the rounding to the dtype: with E the weights' error sum,
    S the sum of the absolute weights and T the terms of a sum (a product and at most T - 1 additions round each term
    T times at most), a row errs by M (E + T S U24), the output by S of that, E times a row (<= S M) and T S S U24 M of
    its own: M U24 (2 S E + 2 T S S).  bilinear: 2 2 + 2 2 = 8, the bar of DESIGN 5.13; bicubic: 2 1.375 184 + 8
    1.375^2 = 521.2, taken as 540 for the second-order terms."""
    S, E, T = S_WEIGHTS[mode], E_WEIGHTS[mode], TERMS[mode]
    units = 2 * S * E + 2 * T * S * S
    return 8.0 if mode == rc.BILINEAR else max(540.0, units)


def all_cases(mode, align):
    """The table's sizes and the three scale_factor cases as (C, Hi, Wi, cbResize-like)."""
    for Cn, Hi, Wi, Ho, Wo in rc.SHAPES:
        yield Cn, Hi, Wi, rc.resize_of_size(Hi, Wi, Ho, Wo, mode, align)
    for sf in rc.SCALES:
        yield rc.SCALE_SHAPE + (rc.resize_of_scale(rc.SCALE_SHAPE[1], rc.SCALE_SHAPE[2], sf, mode, align),)


def torch_resize(x, rs, size=None, scale=None):
    kw = dict(mode=rc.KINDS[rs.mode])
    if rs.mode in (rc.BILINEAR, rc.BICUBIC):
        kw['align_corners'] = bool(rs.alignCorners)
    if scale is not None:
        return F.interpolate(x, scale_factor=scale, **kw)
    return F.interpolate(x, size=(rs.Ho, rs.Wo), **kw)


# ------------------------------------------------------------------------------------------------ the twin
@pytest.mark.parametrize("mode,align", [m for m in rc.MODES if m[0] >= rc.BILINEAR], ids=rc.MODE_IDS[2:])
def test_f32_twin_is_within_the_bar_of_the_float64_rules(mode, align):
    """fp32: |twin - r| <= units 2^-24 max|tap| with units = 8 (bilinear) and 540 (bicubic), derived in f32_bar_units from
    one rounding per operation times the sums of the absolute weights ((1.375)^2 for bicubic); fp16: one more correct
    rounding, 2^-11 |r| + 2^-25 + (units + 1) 2^-24 max|tap|.  r: the same rules in float64."""
    units = f32_bar_units(mode)
    assert units == (8.0 if mode == rc.BILINEAR else 540.0)
    rng = np.random.default_rng(3)
    worst = 0.0
    for Cn, Hi, Wi, rs in all_cases(mode, align):
        xs = rng.standard_normal((Cn, Hi, Wi)) * 10
        for npdt in (np.float32, np.float16):
            x = xs.astype(npdt)
            got = rc.twin(x, rs, np.float32)
            assert got.dtype == npdt and got.shape == (Cn, rs.Ho, rs.Wo)
            r = rc.twin(x, rs, np.float64)
            mx = rc.tap_abs_max(x, rs)[None]
            bar = units * U24 * mx
            if npdt is np.float16:
                bar = 2.0 ** -11 * np.abs(r) + 2.0 ** -25 + (units + 1) * U24 * mx
            err = np.abs(got.astype(np.float64) - r)
            worst = max(worst, float((err / np.where(bar > 0, bar, 1)).max()))
            assert (err <= bar).all(), (rs, npdt)
    print("%s: worst share of the bar %.4f" % (rc.KINDS[mode], worst))


def test_bicubic_weights_sum_to_one_and_at_most_1_375_in_absolute_value():
    frac = np.array([[r, 4096] for r in range(4096)], dtype=np.int64)
    w = rc._weights(rc.BICUBIC, frac, np.float64)
    assert np.abs(w.sum(axis=1) - 1).max() < 1e-12
    assert np.abs(w).sum(axis=1).max() == 1.375 and np.abs(w).sum(axis=1).argmax() == 2048
    w32 = rc._weights(rc.BICUBIC, frac, np.float32)
    assert w32.dtype == np.float32 and np.abs(w32.astype(np.float64) - w).sum(axis=1).max() <= 184 * U24


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_nearest_kinds_of_the_twin_are_torch_bit_for_bit(dtype):
    """Every size of the table and the three scales: the twin's copies equal F.interpolate on the CPU bit for bit
    (nearest-exact for the sizes; torch derives its index from a float scale, which these sizes do not trip)."""
    rng = np.random.default_rng(5)
    for mode in (rc.NEAREST, rc.NEAREST_EXACT):
        for Cn, Hi, Wi, Ho, Wo in rc.SHAPES:
            x = torch.from_numpy(rng.standard_normal((1, Cn, Hi, Wi))).to(dtype)
            rs = rc.resize_of_size(Hi, Wi, Ho, Wo, mode, 0)
            assert np.array_equal(rc.twin(x[0].numpy(), rs, np.float32), torch_resize(x, rs)[0].numpy()), rs
    for sf in rc.SCALES + [0.5, 2.5]:
        Cn, Hi, Wi = rc.SCALE_SHAPE
        x = torch.from_numpy(rng.standard_normal((1, Cn, Hi, Wi))).to(dtype)
        rs = rc.resize_of_scale(Hi, Wi, sf, rc.NEAREST, 0)
        want = torch_resize(x, rs, scale=sf)
        assert tuple(want.shape[2:]) == (rs.Ho, rs.Wo)
        assert np.array_equal(rc.twin(x[0].numpy(), rs, np.float32), want[0].numpy()), rs


def test_nearest_indexes_are_torchs():
    """The integer rules give torch's indexes for further extent pairs, both kinds, both directions."""
    pairs = [(5, 13), (3, 9), (6, 17), (11, 70), (1, 5)]
    pairs = pairs + [(b, a) for a, b in pairs] + [(12, 20), (33, 65), (22, 66), (32, 64), (9, 72), (130, 17)]
    for n, N in pairs:
        ramp = torch.arange(n, dtype=torch.float32).reshape(1, 1, 1, n)
        a, b = rc.step_of_size(n, N)
        for mode in (rc.NEAREST, rc.NEAREST_EXACT):
            mine = [rc.source(mode, 0, o, n, N, a, b)[0][0] for o in range(N)]
            theirs = F.interpolate(ramp, size=(1, N), mode=rc.KINDS[mode])[0, 0, 0].to(torch.int64).tolist()
            assert mine == theirs, (n, N, rc.KINDS[mode])


@pytest.mark.parametrize("mode,align", [m for m in rc.MODES if m[0] >= rc.BILINEAR], ids=rc.MODE_IDS[2:])
def test_linear_and_cubic_rules_are_torchs(mode, align):
    """A check of the RULE (half-pixel centres, border clamp, A = -0.75) against F.interpolate on the CPU: within
    1e-4 max|x|.  torch derives the coordinate from a float scale; the drift measured with extents <= 70 was 1.2e-5 for
    N(0, 1) inputs, a wrong rule gives 1e-2 and more."""
    rng = np.random.default_rng(9)
    worst = 0.0
    for Cn, Hi, Wi, rs in all_cases(mode, align):
        x = torch.from_numpy(rng.standard_normal((1, Cn, Hi, Wi)).astype(np.float32))
        scaled = (rs.aH * rs.Ho, rs.aW * rs.Wo) != (rs.bH * Hi, rs.bW * Wi)
        if scaled:
            sf = (rs.bH / rs.aH, rs.bW / rs.aW)
            want = torch_resize(x, rs, scale=sf)
        else:
            want = torch_resize(x, rs)
        got = rc.twin(x[0].numpy(), rs, np.float32)
        assert got.shape == tuple(want.shape[1:])
        dev = float(np.abs(got - want[0].numpy()).max()) / float(x.abs().max())
        worst = max(worst, dev)
        assert dev <= 1e-4, (rs, dev)
    print("%s align=%d: worst deviation from torch %.2e max|x|" % (rc.KINDS[mode], align, worst))


@pytest.mark.parametrize("mode,align", rc.MODES, ids=rc.MODE_IDS)
def test_candidate_ranges_hold_every_reader(mode, align):
    """The footprint as the list kernel builds it -- candidate rows and columns, each tested -- equals brute force over
    every output pixel's taps: on the table (the tall map cut to 40 rows) with single pixels, corners and a random
    half, and per axis for EVERY input coordinate of every extent pair n <= 24, n / 8 <= N <= 8 n."""
    rng = np.random.default_rng(11)
    for Cn, Hi, Wi, rs in all_cases(mode, align):
        if Hi > 100:
            Hi, rs = 20, rc.resize_of_size(20, Wi, 40, rs.Wo, mode, align)
        frames = [np.zeros((Hi, Wi), dtype=bool) for _ in range(4)]
        frames[0][Hi // 2, Wi // 2] = frames[1][0, 0] = frames[2][Hi - 1, Wi - 1] = True
        frames.append(rng.random((Hi, Wi)) < 0.5)
        for changed in frames:
            want = rc.footprint(changed, rs)
            assert np.array_equal(rc.footprint_by_candidates(changed, rs), want), rs
            if not changed.any():
                assert not want.any()
        assert rc.footprint(np.ones((Hi, Wi), dtype=bool), rs).all()
    for n in range(1, 25):
        for N in range((n + 7) // 8, 8 * n + 1):
            a, b = rc.step_of_size(n, N)
            readers = [set() for _ in range(n)]
            for o in range(N):
                for i in rc.source(mode, align, o, n, N, a, b)[0]:
                    assert 0 <= i < n
                    readers[i].add(o)
            for i in range(n):
                cand = rc.candidates(i, n, N, a, b, align)
                assert readers[i] <= set(cand), (n, N, i)
                assert len(cand) <= 51


def test_candidate_ranges_hold_for_scale_factors():
    """... and with the step 1 / scale_factor and N = floor(n scale_factor), where a / b is not n / N."""
    for sf in (1.5, 0.75, 2.5, 0.5, 1.25, 7.5, 0.125, 8.0, 3.0):
        for n in range(1, 40):
            N = int(np.floor(n * sf))
            if N < 1:
                continue
            rs = rc.resize_of_scale(n, n, sf, rc.BICUBIC, 0)
            for mode, align in rc.MODES:
                for i in range(n):
                    cand = set(rc.candidates(i, n, N, rs.aH, rs.bH, align))
                    for o in range(N):
                        if i in rc.source(mode, align, o, n, N, rs.aH, rs.bH)[0]:
                            assert o in cand, (sf, n, mode, align, i, o)


def test_downscaling_skips_input_pixels_and_they_list_nothing():
    rs = rc.resize_of_size(16, 130, 2, 17, rc.NEAREST, 0)
    read = np.zeros((16, 130), dtype=bool)
    for oy in range(2):
        for ox in range(17):
            read[rc.source(rc.NEAREST, 0, oy, 16, 2, rs.aH, rs.bH)[0][0], rc.source(rc.NEAREST, 0, ox, 130, 17, rs.aW, rs.bW)[0][0]] = True
    assert read.sum() == 34
    y, x = np.argwhere(~read)[5]
    changed = np.zeros((16, 130), dtype=bool)
    changed[y, x] = True
    assert not rc.footprint(changed, rs).any() and not rc.footprint_by_candidates(changed, rs).any()


# ------------------------------------------------------------------------------------------------ the constructor
def test_constructor_takes_and_refuses(pkg, lib):
    R = pkg.CBResize2d
    for m, want in ((nn.Upsample(size=(8, 9)), ((8, 9), None, 'nearest', False)),
                    (nn.Upsample(size=7, mode='bicubic', align_corners=True), ((7, 7), None, 'bicubic', True)),
                    (nn.Upsample(scale_factor=1.5, mode='bilinear'), (None, (1.5, 1.5), 'bilinear', False)),
                    (nn.Upsample(scale_factor=(2, 0.5), mode='nearest-exact'), (None, (2.0, 0.5), 'nearest-exact', False)),
                    (nn.UpsamplingNearest2d(scale_factor=2), (None, (2.0, 2.0), 'nearest', False)),
                    (nn.UpsamplingBilinear2d(size=(5, 6)), ((5, 6), None, 'bilinear', True))):
        cb = R(m)
        assert (cb.size, cb.scale_factor, cb.mode, cb.align_corners) == want, m
        assert not cb.propChangeIndexes and cb.cloneOutput and cb.outputState.numel() == 0
        assert 'mode=%s' % want[2] in repr(cb)
    cb = R(size=(480, 640), mode='bilinear', align_corners=False)
    assert cb.geometry(60, 80) == (480, 640, 1, 8, 1, 8)
    assert cb.geometry(60, 80, size=(90, 100)) == (90, 100, 2, 3, 4, 5)
    assert R(scale_factor=1.5).geometry(5, 13) == (7, 19, 2, 3, 2, 3)
    assert R(scale_factor=1.5, recompute_scale_factor=True).geometry(5, 13) == (7, 19, 5, 7, 13, 19)
    assert R(scale_factor=(2.5, 0.5)).geometry(6, 13) == (15, 6, 2, 5, 2, 1)
    assert R(scale_factor=8).geometry(2, 9) == (16, 72, 1, 8, 1, 8)

    class MyUpsample(nn.Upsample):
        pass
    Err = lib.CBinferError
    for make, what in ((lambda: R(MyUpsample(scale_factor=2)), "not a subclass"),
                       (lambda: R(nn.Conv2d(3, 3, 1)), "nn.Upsample"),
                       (lambda: R(size=4, antialias=True), "antialias=True"),
                       (lambda: R(nn.Upsample(scale_factor=2, mode='area')), "mode='area'"),
                       (lambda: R(size=4, mode='trilinear'), "mode='trilinear'"),
                       (lambda: R(size=4, mode='nearest', align_corners=False), "align_corners=False"),
                       (lambda: R(size=4, mode='nearest-exact', align_corners=True), "align_corners=True"),
                       (lambda: R(scale_factor=9), "scale_factor=9"),
                       (lambda: R(scale_factor=(2, 0.1)), "scale_factor="),
                       (lambda: R(scale_factor=0.3), "exact rational"),
                       (lambda: R(scale_factor=(2, 2, 2)), "scale_factor="),
                       (lambda: R(size=(4, 0)), "size="),
                       (lambda: R(size=4, scale_factor=2), "only one of"),
                       (lambda: R(nn.Upsample(size=4), size=5), "not both"),
                       (lambda: R().geometry(4, 4), "neither size nor scale_factor"),
                       (lambda: R(size=(33, 8)).geometry(4, 4), "ratio beyond 8"),
                       (lambda: R(size=(4, 1)).geometry(4, 9), "ratio beyond 8"),
                       (lambda: R(scale_factor=0.125).geometry(7, 8), "no output pixel"),
                       (lambda: R(size=(4999, 8)).geometry(9973, 8), "beyond 4096")):
        with pytest.raises(Err, match=what):
            make()
    assert R(scale_factor=0.3, recompute_scale_factor=True).geometry(10, 20) == (3, 6, 10, 3, 10, 3)


def test_forward_refusals_without_a_device(pkg, lib):
    rs = pkg.CBResize2d(size=(7, 9), mode='bicubic')
    x = torch.zeros(1, 4, 5, 6)
    for inp, what in ((torch.zeros(2, 4, 5, 6), "batch 1"), (torch.zeros(4, 5, 6), r"\[1, C, H, W\]"),
                      (('changeIndexes', x), "tuple"), (None, "must be a tensor"), (x.double(), "float32 and float16"),
                      (x.to(torch.bfloat16), "float32 and float16"), (x, "HIP devices only")):
        with pytest.raises(lib.CBinferError, match=what):
            rs(inp)
    with pytest.raises(lib.CBinferError, match="HIP devices only"):
        rs(x, size=(5, 5))


# ------------------------------------------------------------------------------------------------ the C ABI
def rs_struct(lib, Ho=6, Wo=10, aH=2, bH=3, aW=1, bW=2, mode=None, ac=0):
    return ctypes.pointer(lib.Resize(Ho, Wo, aH, bH, aW, bW, lib.RESIZE_BILINEAR if mode is None else mode, ac))


def test_resize_supported_over_the_limits(lib):
    sup = lib.C.cbinfer_resize_supported
    assert (lib.RESIZE_NEAREST, lib.RESIZE_NEAREST_EXACT, lib.RESIZE_BILINEAR, lib.RESIZE_BICUBIC) == (0, 1, 2, 3)
    assert (lib.RESIZE_NEAREST, lib.RESIZE_NEAREST_EXACT, lib.RESIZE_BILINEAR, lib.RESIZE_BICUBIC) == (
        rc.NEAREST, rc.NEAREST_EXACT, rc.BILINEAR, rc.BICUBIC)
    assert ctypes.sizeof(lib.Resize) == 32
    good = [(rs_struct(lib), 4, 5), (rs_struct(lib, mode=lib.RESIZE_BICUBIC, ac=1), 4, 5),
            (rs_struct(lib, mode=lib.RESIZE_NEAREST), 4, 5), (rs_struct(lib, mode=lib.RESIZE_NEAREST_EXACT), 4, 5),
            (rs_struct(lib, 16, 72, 1, 8, 1, 8), 2, 9), (rs_struct(lib, 2, 9, 8, 1, 8, 1), 16, 72),
            (rs_struct(lib, 1, 1, 5, 1, 8, 1), 5, 8), (rs_struct(lib, 5, 8, 1, 5, 1, 8), 1, 1),
            (rs_struct(lib, 4095, 4096, 4096, 4095, 4095, 4096), 4096, 4095),
            (rs_struct(lib, 32767, 32767, 1, 1, 1, 1), 32767, 32767),
            # with align_corners the step is not read: any step within the limits
            (rs_struct(lib, 6, 10, 8, 1, 1, 8, ac=1), 4, 5),
            # a scale_factor's step: N = floor(n sf) may fall short of n b / a
            (rs_struct(lib, 7, 19, 2, 3, 2, 3), 5, 13)]
    for rs, Hi, Wi in good:
        assert sup(rs, Hi, Wi) == 1, (tuple(getattr(rs.contents, f) for f, _ in lib.Resize._fields_), Hi, Wi)
    bad = [(None, 4, 5), (rs_struct(lib, mode=4), 4, 5), (rs_struct(lib, mode=-1), 4, 5), (rs_struct(lib, ac=2), 4, 5),
           (rs_struct(lib, ac=-1), 4, 5), (rs_struct(lib, mode=lib.RESIZE_NEAREST, ac=1), 4, 5),
           (rs_struct(lib, mode=lib.RESIZE_NEAREST_EXACT, ac=1), 4, 5),
           (rs_struct(lib, aH=0), 4, 5), (rs_struct(lib, bW=0), 4, 5), (rs_struct(lib, aW=-1), 4, 5),
           (rs_struct(lib, Ho=0), 4, 5), (rs_struct(lib, Wo=-3), 4, 5), (rs_struct(lib), 0, 5), (rs_struct(lib), 4, 0),
           (rs_struct(lib, 18, 72, 1, 9, 1, 8), 2, 9),            # a / b < 1/8
           (rs_struct(lib, 2, 9, 8, 1, 9, 1), 16, 81),            # a / b > 8
           (rs_struct(lib, 17, 72, 1, 8, 1, 8), 2, 9),            # N > 8 n
           (rs_struct(lib, 2, 9, 8, 1, 8, 1), 17, 72),            # N < n / 8
           (rs_struct(lib, 17, 72, 1, 8, 1, 8, ac=1), 2, 9),      # ... with align_corners as well
           (rs_struct(lib, 4097, 4096, 4096, 4097, 1, 1), 4096, 4096),      # b > 4096
           (rs_struct(lib, 4096, 4097, 1, 1, 4097, 4096), 4096, 4096),      # a > 4096
           (rs_struct(lib, 32768, 8, 1, 1, 1, 1), 32768, 8),      # an extent of 2^15
           (rs_struct(lib, 8, 32768, 1, 1, 1, 2), 8, 16384),
           (rs_struct(lib, 7, 10, 2, 3, 1, 2), 4, 5),             # N a > n b: the output reaches beyond the input
           (rs_struct(lib, 6, 11, 2, 3, 1, 2), 4, 5)]
    for rs, Hi, Wi in bad:
        assert sup(rs, Hi, Wi) == 0, (rs and tuple(getattr(rs.contents, f) for f, _ in lib.Resize._fields_), Hi, Wi)


def test_entry_point_checks_its_arguments(lib):
    """Bad arguments return CB_ERR_BADARG (-1) before anything is launched (the device pointers here are never
    followed)."""
    C = lib.C
    assert C.cbinfer_abi_version() == 11
    X, O, BITS, COPY, M, L, N2 = (0x10000 * i for i in range(1, 8))

    def go(x=X, o=O, mask=None, lst=None, cap=0, count=None, bits=BITS, cp=COPY, Cn=3, Hi=4, Wi=5, rs=rs_struct(lib),
           dt=lib.CB_F32):
        return C.cbinfer_cbresize_forward(x, o, mask, lst, cap, count, bits, cp, Cn, Hi, Wi, rs, dt, None)

    for bad in (dict(x=None), dict(o=None), dict(bits=None), dict(cp=None), dict(cp=BITS), dict(rs=None), dict(Cn=0),
                dict(Hi=0), dict(Wi=-1), dict(dt=lib.CB_F32S), dict(dt=7), dict(lst=L, cap=-1), dict(mask=M, lst=L),
                dict(count=N2), dict(mask=BITS), dict(mask=COPY), dict(Cn=1 << 25), dict(Hi=3), dict(Wi=4),
                dict(Hi=1 << 15, rs=rs_struct(lib, 1 << 15, 10, 1, 1, 1, 2)),
                dict(rs=rs_struct(lib, mode=9)), dict(rs=rs_struct(lib, mode=lib.RESIZE_NEAREST, ac=1)),
                dict(rs=rs_struct(lib, aH=0)), dict(rs=rs_struct(lib, 40, 10, 1, 10, 1, 2))):
        assert go(**bad) == -1, bad


# ------------------------------------------------------------------------------------------------ the passes
def fcn_head(pkg, up):
    torch.manual_seed(2)
    seq = nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), nn.ReLU(), up, nn.Conv2d(8, 4, 1)).eval()
    return pkg.convert(seq, threshold=0.05)


def test_insert_resize_on_heads_stacks_and_what_it_leaves(pkg, lib):
    from cbinfer_amd import chain
    matrix = [chain.producers(name) for name in chain.PASSES]
    # an FCN-type head: conv -> Upsample(size=) -> conv1x1
    net = fcn_head(pkg, nn.Upsample(size=(20, 33), mode='bilinear', align_corners=False))
    assert [type(m).__name__ for m in net] == ['CBConv2d', 'Upsample', 'CBConv2d']
    assert pkg.insertCBResize(net, cloneOutput=False) is net
    assert [type(m).__name__ for m in net] == ['CBConv2d', 'CBResize2d', 'CBConv2d']
    rs = net[1]
    assert (rs.size, rs.mode, rs.align_corners, rs.cloneOutput) == ((20, 33), 'bilinear', False, False)
    assert net[0].propChangeIndexes and rs.propChangeIndexes      # (a 1x1 layer reads exactly the pixels it is handed)
    # an FPN-type stack: the resizes behind one another, then a 3x3 layer that needs its own input copy
    torch.manual_seed(3)
    seq = nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), nn.Upsample(scale_factor=1.5, mode='nearest'),
                        nn.Upsample(size=(9, 9), mode='bicubic'), nn.Conv2d(8, 8, 3, padding=1), nn.Tanh(),
                        nn.Upsample(size=(9, 9)), nn.Conv2d(8, 8, 1), nn.Upsample(scale_factor=16),
                        nn.Conv2d(8, 8, 1), nn.Upsample(scale_factor=2, mode='area')).eval()
    net = pkg.convert(seq, threshold=0.05)
    net[3].copyInput = False
    pkg.insertCBResize(net)
    assert [type(m).__name__ for m in net] == ['CBConv2d', 'CBResize2d', 'CBResize2d', 'CBConv2d', 'Tanh', 'Upsample',
                                               'CBConv2d', 'Upsample', 'CBConv2d', 'Upsample']
    assert net[0].propChangeIndexes and net[1].propChangeIndexes is True and not net[2].propChangeIndexes
    assert net[1].cloneOutput and net[3].copyInput is True
    # behind a non-producer (Tanh), beyond the limits (x16) or a mode the module refuses: dense, flags untouched
    assert not net[3].propChangeIndexes and not net[6].propChangeIndexes and not net[8].propChangeIndexes
    # after insertCBUpsampling only what that pass left is taken
    torch.manual_seed(4)
    seq = nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), nn.Upsample(scale_factor=2, mode='bilinear'),
                        nn.Upsample(scale_factor=1.5, mode='bilinear'), nn.Upsample(scale_factor=2)).eval()
    net = pkg.insertCBResize(pkg.insertCBUpsampling(pkg.convert(seq, threshold=0.05)))
    assert [type(m).__name__ for m in net] == ['CBConv2d', 'CBUpsample2d', 'CBResize2d', 'CBResize2d']
    assert net[1].propChangeIndexes and net[2].propChangeIndexes
    # alone it takes the integer scales too
    net = pkg.insertCBResize(pkg.convert(copy.deepcopy(seq), threshold=0.05))
    assert [type(m).__name__ for m in net] == ['CBConv2d', 'CBResize2d', 'CBResize2d', 'CBResize2d']
    # behind a grouped convolution and a channel reduction
    torch.manual_seed(5)
    seq = nn.Sequential(nn.Conv2d(4, 8, 3, padding=1, groups=2), nn.Upsample(size=(7, 7)), nn.Softmax2d(),
                        nn.Upsample(size=(9, 9), mode='bicubic')).eval()
    net = pkg.convert(seq, threshold=0.05, grouped=True)
    pkg.insertCBResize(net)
    pkg.insertCBChannelOps(net)      # (the module is a producer for the softmax behind it)
    pkg.insertCBResize(net)
    assert [type(m).__name__ for m in net] == ['CBGroupedConv2d', 'CBResize2d', 'CBChannelReduce2d', 'CBResize2d']
    assert net[0].propChangeIndexes and net[1].propChangeIndexes and net[2].propChangeIndexes
    assert matrix == [chain.producers(name) for name in chain.PASSES]      # (what it holds: test_host_chain.py)


def test_the_other_passes_accept_the_module_as_a_producer(pkg, lib):
    from cbinfer_amd import chain
    R = pkg.CBResize2d
    # every pass but the two poolings (every pass's whole set, in order: test_host_chain.py)
    assert [name for name in chain.PASSES if R not in chain.producers(name)] == [
        'insertCBPooling', 'insertCBPooling(generalGeometry=True)']

    def behind(*mods):
        net = nn.Sequential(R(size=(9, 11), mode='bilinear'))
        for k, m in enumerate(mods):
            net.add_module('m%d' % k, m)
        return net.eval()
    net = pkg.insertCBPointwise(behind(nn.ReLU()))
    assert type(net.m0) is pkg.CBPointwise2d and net[0].propChangeIndexes
    net = pkg.insertCBUpsampling(behind(nn.Upsample(scale_factor=2)))
    assert type(net.m0) is pkg.CBUpsample2d and net[0].propChangeIndexes
    net = pkg.insertCBRearrange(behind(nn.PixelShuffle(2)))
    assert type(net.m0) is pkg.CBPixelShuffle2d and net[0].propChangeIndexes
    net = pkg.insertCBChannelOps(behind(nn.Softmax2d()))
    assert type(net.m0) is pkg.CBChannelReduce2d and net[0].propChangeIndexes
    net = pkg.insertCBTransposedConv(behind(nn.ConvTranspose2d(4, 4, 2, stride=2)), threshold=0.05)
    assert type(net.m0) is pkg.CBConvTranspose2d      # (it runs its own detection: nothing is switched on)
    net = pkg.convert(behind(nn.Conv2d(4, 4, 3, padding=1, groups=4)), threshold=0.05, depthwise=True)
    assert type(net.m0) is pkg.CBDepthwiseConv2d and not net[0].propChangeIndexes
    pkg.linkDepthwise(net)
    assert net[0].propChangeIndexes


# ------------------------------------------------------------------------------------------------ module hygiene
def test_exports_state_helpers_and_pickling(pkg, lib):
    assert all(n in pkg.__all__ for n in ('CBResize2d', 'insertCBResize'))
    assert pkg.CBResize2d is pkg.resize.CBResize2d and pkg.insertCBResize is pkg.resize.insertCBResize
    import pycbinfer.resize as alias
    assert alias.CBResize2d is pkg.CBResize2d
    assert {'cbinfer_resize_supported', 'cbinfer_cbresize_forward'} <= set(lib.EXPORTED_SYMBOLS)
    rs = pkg.CBResize2d(scale_factor=(1.5, 0.75), mode='bicubic', align_corners=True)
    rs.propChangeIndexes, rs.cloneOutput = True, False
    net = nn.Sequential(rs)
    rs.outputState = torch.ones(1, 2, 6, 6)
    rs.__dict__['_work'] = {'key': None}
    rs.__dict__['_rsC'] = rs_struct(lib)
    assert any(t is rs.outputState for t in pkg.getStateTensors(net))
    for clone in (pickle.loads(pickle.dumps(net)), copy.deepcopy(net)):
        r = clone[0]
        assert type(r) is pkg.CBResize2d and r._work is None and r._rsC is None
        assert (r.size, r.scale_factor, r.mode, r.align_corners, r.recompute_scale_factor, r.propChangeIndexes,
                r.cloneOutput) == (None, (1.5, 0.75), 'bicubic', True, False, True, False)
        assert torch.equal(r.outputState, rs.outputState) and repr(r) == repr(rs)
        assert r.geometry(4, 8) == (6, 6, 2, 3, 4, 3)
    pkg.clearMemory(net)
    assert rs.outputState.numel() == 0 and rs._work is None


def test_batch_branch_and_program_refusals_name_the_module(pkg, lib):
    net = fcn_head(pkg, nn.Upsample(size=(20, 33), mode='bilinear'))
    pkg.insertCBResize(net)
    with pytest.raises(lib.CBinferError, match=r"SequenceBatch: layer '2' is CBResize2d \(size=\(20, 33\).*a change-based "
                                               r"resize"):
        pkg.SequenceBatch(net, 2)
    with pytest.raises(lib.CBinferError, match=r"BranchGroup: layer '0.2' is CBResize2d"):
        pkg.BranchGroup([net])
    from cbinfer_amd import batch
    assert [row for row in batch.CHAIN_OPERATORS if pkg.CBResize2d in row[0]] == [
        ((pkg.CBResize2d,), 'a change-based resize', 'dense-prediction')]
    # FrameProgram's refusal of a frame that ran a torch operator names the module and its pass, and keeps what it said
    said = inspect.getsource(pkg.FrameProgram)
    assert "pycbinfer.CBResize2d (insertCBResize)" in said
    assert "pycbinfer.CBChannelReduce2d (insertCBChannelOps)" in said and "CBUpsample2d / CBConcat2d" in said
