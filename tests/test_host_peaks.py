"""CPU-only tests of change-based peak suppression and peak lists (CBPoolMax2d(suppress=...), cb_peaks.hip):
the numpy twin of tests/peaks_cases.py against CPU torch, the conditions its cases must meet, the host-pure C function
and the argument refusals of the C ABI, the constructor and its refusals, the defaults, pickling, and the
insertCBPooling(nmsTypes=...) wiring.  No kernel is launched here."""
import copy
import ctypes
import io
import pickle

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import peaks_cases as pc
from peaks_cases import DTYPES, SHAPES, WINDOW_IDS, WINDOWS
from optest import lib, pkg      # noqa: F401  (fixtures)


@pytest.fixture(autouse=True, scope="module")
def header_block(lib):
    """The twin restates the block of include/cbinfer_hip.h that declares cbPeaks: without it there is no rule to test."""
    assert hasattr(lib, 'Peaks') and 'cbinfer_peaks_list' in lib.EXPORTED_SYMBOLS


# ------------------------------------------------------------------------------------------------ the rule
def torch_formula(v, kH, kW, floor):
    """torch.where((F.max_pool2d(x, k, 1, k // 2) == x) & (x >= floor), x, 0); float16 in float32, which is exact."""
    x = torch.from_numpy(v.astype(np.float32))[None]
    keep = F.max_pool2d(x, (kH, kW), 1, (kH // 2, kW // 2)) == x
    if floor is not None:
        keep = keep & (x >= floor)
    return torch.where(keep, x, torch.zeros_like(x))[0].numpy().astype(v.dtype), keep[0].numpy()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("window", [w for w in WINDOW_IDS if not WINDOWS[w][2]])
def test_twin_is_the_torch_formula_bit_for_bit(window, dtype):
    kH, kW, _, floor = WINDOWS[window]
    for shape in SHAPES:
        for kind in pc.value_sets(dtype):
            for fl in (floor, None, 0.0):
                for _, _, x in pc.frames(shape, kind, dtype, window)[:3]:
                    k = pc.keep(x, kH, kW, 0, fl)
                    want, wantKeep = torch_formula(x, kH, kW, fl)
                    assert np.array_equal(k, wantKeep), (shape, kind, fl)
                    assert np.array_equal(pc.bits_of(pc.suppressed(x, k)), pc.bits_of(want)), (shape, kind, fl)


@pytest.mark.parametrize("dtype", DTYPES)
def test_twin_special_values(dtype):
    """A NaN suppresses itself and every pixel that sees it; +0 and -0 are equal and a kept -0 keeps its sign; -inf is
    kept where it is all there is; the floor is compared in float32."""
    dt = pc.np_dtype(dtype)
    v = np.array([[[0.0, -0.0, -1.0, -1.0, np.nan, -1.0, -1.0, -np.inf]]], dtype=dt)
    out, k = pc.twin(v, "w3")
    assert k[0, 0].tolist() == [True, True, False, False, False, False, True, False]
    assert pc.bits_of(out)[0, 0, 1] == pc.bits_of(np.array([-0.0], dtype=dt))[0]
    assert pc.bits_of(out)[0, 0, 4] == 0      # (the NaN itself becomes +0)
    lone = np.full((1, 1, 1), -np.inf, dtype=dt)
    assert pc.keep(lone, 7, 7, 0, None).all() and not pc.keep(lone, 7, 7, 0, -1e30).any()
    assert not pc.keep(np.full((1, 1, 1), np.nan, dtype=dt), 3, 3, 1, None).any()
    assert pc.keep(np.zeros((1, 2, 2), dtype=dt) * -1, 3, 3, 0, 0.0).all()      # (-0 >= 0)
    if dtype == "f16":      # 0.1 is no float16: float16(0.1) = 0.0999755859375 lies BELOW the float32 floor 0.1
        assert not pc.keep(np.full((1, 1, 1), 0.1, dtype=dt), 3, 3, 0, 0.1).any()


def four_comparisons(v, floor):
    """The cross kind at interior pixels, written anew: above or level with the pixel on the left, on the right, above
    and below, and with the floor."""
    f = v.astype(np.float32)
    mid = f[:, 1:-1, 1:-1]
    with np.errstate(invalid="ignore"):
        k = (mid >= f[:, 1:-1, :-2]) & (mid >= f[:, 1:-1, 2:]) & (mid >= f[:, :-2, 1:-1]) & (mid >= f[:, 2:, 1:-1])
        return k & (mid >= np.float32(floor)) if floor is not None else k


@pytest.mark.parametrize("dtype", DTYPES)
def test_cross_is_four_comparisons_at_interior_pixels(dtype):
    for shape in SHAPES[1:]:
        for kind in pc.value_sets(dtype):
            for fl in (0.1, None):
                x = pc.frames(shape, kind, dtype, 'cross')[5][2]
                k = pc.keep(x, 3, 3, 1, fl)
                assert np.array_equal(k[:, 1:-1, 1:-1], four_comparisons(x, fl)), (shape, kind, fl)
                # ... and a superset of the window kind's peaks
                assert not (pc.keep(x, 3, 3, 0, fl) & ~k).any()
    # at the border the in-map neighbours decide: a corner pixel is compared with two of them
    v = np.array([[[5, 1], [1, 0]]], dtype=pc.np_dtype(dtype))
    assert pc.keep(v, 3, 3, 1, None)[0].tolist() == [[True, False], [False, False]]


def test_list_is_argwhere_order_and_bits_are_the_mask_layout():
    for shape in SHAPES:
        x = pc.frames(shape, "quantised", "f32", "w3")[5][2]
        out, k = pc.twin(x, "w3")
        entries, scores, count, start = pc.peak_list(x, k)
        assert np.array_equal(entries, np.argwhere(k).astype(np.int32)) and count == int(k.sum())
        assert np.array_equal(scores, x[k]) and scores.dtype == x.dtype
        assert start.tolist() == [0] + np.cumsum(k.reshape(shape[0], -1).sum(axis=1)).tolist()
        # channel after channel: peakMap[c].nonzero() of torch
        per = [torch.from_numpy(out[c] != 0).nonzero().numpy() for c in range(shape[0])]
        nz = np.concatenate([np.concatenate([np.full((len(p), 1), c), p], axis=1) for c, p in enumerate(per)])
        assert np.array_equal(nz, entries[(x[k] != 0)])
        bits = pc.peak_bits(k)
        wpr = (shape[2] + 63) // 64
        assert bits.dtype == np.uint64 and bits.size == shape[0] * shape[1] * wpr
        for c, y, px in entries[::7].tolist():
            assert (int(bits[(c * shape[1] + y) * wpr + px // 64]) >> (px % 64)) & 1
        assert sum(bin(int(w)).count("1") for w in bits) == count      # (no padding bit)


def test_footprint_is_the_stride_one_pool_footprint():
    rng = np.random.default_rng(3)
    for kH, kW in ((3, 3), (5, 5), (7, 7), (3, 7)):
        S = rng.random((9, 130)) < 0.02
        want = F.max_pool2d(torch.from_numpy(S.astype(np.float32))[None, None], (kH, kW), 1, (kH // 2, kW // 2))[0, 0] > 0
        assert np.array_equal(pc.footprint(S, kH, kW), want.numpy())


@pytest.mark.parametrize("window", WINDOW_IDS)
def test_case_conditions(window):
    """Conditions, not measurements.  In every non-empty frame of the random and the quantised set at least one listed
    pixel is kept and at least one is suppressed; across the frames at least one peak appears and at least one disappears
    at a pixel whose own value did not change; the two neighbour frames end a standing peak whose value stands.  (The
    degenerate 1x1 map has one pixel per channel and no neighbour: it cannot meet them and is left out.)"""
    kH, kW, _, _ = WINDOWS[window]
    for shape in SHAPES[1:]:
        R, Q, P, D = (((slice(None),) + site) for site in pc.sites(shape[1], shape[2], kW // 2))
        for kind in ("random", "quantised"):
            for dtype in DTYPES:
                fr = pc.frames(shape, kind, dtype, window)
                assert [f[0] for f in fr] == ["empty", "one pixel", "corner", "bit 63/64", "full row", "dense",
                                              "neighbour in the row", "neighbour in the row below"]
                appeared = vanished = 0
                before = None
                for label, S, x in fr:
                    _, k = pc.twin(x, window)
                    L = pc.footprint(S, kH, kW)
                    if S.any():
                        assert k[:, L].any() and (~k[:, L]).any(), (shape, kind, dtype, label)
                    if before is not None:
                        assert np.array_equal(k[:, ~L], before[:, ~L])      # (locality: what the footprint rests on)
                        appeared += int((k & ~before)[:, ~S].sum())
                        vanished += int((before & ~k)[:, ~S].sum())
                    if label == "neighbour in the row":      # only Q changes: R stands, P appears
                        assert S.sum() == 1 and S[Q[1:]] and before[R].all() and k[R].all()
                        assert not before[P].any() and k[P].all(), (shape, kind, dtype)
                    if label == "neighbour in the row below":      # only D changes: R goes
                        assert S.sum() == 1 and S[D[1:]] and before[R].all() and not k[R].any(), (shape, kind, dtype)
                    before = k
                assert appeared >= 1 and vanished >= 1, (shape, kind, dtype, appeared, vanished)
    assert pc.sites(5, 70, 3)[:2] == ((0, 63), (0, 64)) and pc.sites(1, 1, 1) is None
    assert [f[0] for f in pc.frames((1, 1, 1), "random", "f32", window)][-1] == "dense"


# ------------------------------------------------------------------------------------------------ the C ABI
def test_peaks_supported_field_by_field(lib):
    C = lib.C

    def ok(kH=3, kW=3, cross=0, hasFloor=0, floor=0.0):
        return C.cbinfer_peaks_supported(ctypes.byref(lib.Peaks(kH, kW, cross, hasFloor, floor)))
    assert C.cbinfer_abi_version() == 11 and lib.ABI_VERSION == 11
    assert [f[0] for f in lib.Peaks._fields_] == ['kH', 'kW', 'cross', 'hasFloor', 'floor']
    assert C.cbinfer_peaks_supported(None) == 0
    for k in range(-1, 11):
        assert ok(kH=k) == ok(kW=k) == int(k in (3, 5, 7)), k
    for kH in (3, 5, 7):
        for kW in (3, 5, 7):
            assert ok(kH=kH, kW=kW) == 1 and ok(kH=kH, kW=kW, cross=1) == int((kH, kW) == (3, 3))
    assert ok(cross=2) == 0 and ok(cross=-1) == 0 and ok(hasFloor=2) == 0 and ok(hasFloor=-1) == 0
    for fl in (float('nan'), float('inf'), float('-inf')):
        assert ok(hasFloor=1, floor=fl) == 0 and ok(hasFloor=0, floor=fl) == 1      # (no floor: the field is not read)
    assert ok(hasFloor=1, floor=-3.5) == 1 and ok(kH=7, kW=3, hasFloor=1, floor=0.1) == 1
    for name in ("cbinfer_peaks_supported", "cbinfer_peaks_changed", "cbinfer_cbpeaks_forward", "cbinfer_peaks_list"):
        assert name in lib.EXPORTED_SYMBOLS
    assert lib.C.cbinfer_peaks_supported.launcher is False and lib.C.cbinfer_peaks_list.launcher is True


def test_c_entry_points_check_their_arguments(lib):
    """Bad arguments return CB_ERR_BADARG (-1) or CB_ERR_UNSUPPORTED (-2) before anything is launched (the pointers
    here are never followed)."""
    C = lib.C
    X, O, PB, M, L, CNT, BITS, COPY, WORK, ENT, SC, START = (0x100000 * i for i in range(1, 13))
    good = lib.Peaks(3, 3, 0, 1, 0.1)

    def fwd(x=X, o=O, pb=PB, mask=None, lst=None, cap=0, cnt=None, bits=BITS, cp=COPY, Cn=3, H=7, W=70, p=good,
            dt=lib.CB_F32):
        return C.cbinfer_cbpeaks_forward(x, o, pb, mask, lst, cap, cnt, bits, cp, Cn, H, W,
                                         ctypes.byref(p) if p is not None else None, dt, None)

    def chg(x=X, o=O, pb=PB, mask=None, every=1, bits=BITS, cp=COPY, Cn=3, H=7, W=70, p=good, dt=lib.CB_F16, **_):
        return C.cbinfer_peaks_changed(x, o, pb, mask, every, bits, cp, Cn, H, W,
                                       ctypes.byref(p) if p is not None else None, dt, None)

    def lst(x=X, pb=PB, work=WORK, ent=ENT, sc=SC, cap=8, count=CNT, start=START, Cn=3, H=7, W=70, dt=lib.CB_F32):
        return C.cbinfer_peaks_list(x, pb, work, ent, sc, cap, count, start, Cn, H, W, dt, None)

    for call in (fwd, chg):
        for bad in (dict(x=None), dict(o=None), dict(pb=None), dict(bits=None), dict(cp=None), dict(p=None), dict(o=X),
                    dict(cp=BITS), dict(mask=BITS), dict(mask=COPY), dict(pb=BITS), dict(pb=COPY), dict(mask=PB),
                    dict(Cn=0), dict(H=0), dict(W=-1), dict(dt=lib.CB_F32S), dict(dt=7)):
            assert call(**bad) == -1, (call.__name__, bad)
        for p in (lib.Peaks(4, 3, 0, 0, 0.0), lib.Peaks(3, 9, 0, 0, 0.0), lib.Peaks(1, 1, 0, 0, 0.0),
                  lib.Peaks(5, 5, 1, 0, 0.0), lib.Peaks(3, 5, 1, 0, 0.0), lib.Peaks(3, 3, 0, 1, float('nan')),
                  lib.Peaks(3, 3, 0, 1, float('inf'))):
            assert call(p=p) == -2, (call.__name__, p.kH, p.kW, p.cross, p.floor)
        for bad in (dict(H=1 << 16, W=1 << 15), dict(Cn=1 << 25)):
            assert call(**bad) == -2, (call.__name__, bad)
    for bad in (dict(mask=M, lst=L, cap=4), dict(cnt=CNT), dict(mask=M, cnt=CNT), dict(lst=L, cap=-1)):
        assert fwd(**bad) == -1, bad
    for bad in (dict(x=None), dict(pb=None), dict(work=None), dict(count=None), dict(start=None), dict(ent=None),
                dict(sc=None), dict(cap=-1), dict(Cn=0), dict(H=0), dict(W=0), dict(dt=9)):
        assert lst(**bad) == -1, bad
    assert lst(Cn=1 << 10, H=1 << 11, W=1 << 10) == -2


# ------------------------------------------------------------------------------------------------ the module
def nms(k=3, **kw):
    return nn.MaxPool2d(k, 1, (k // 2 if isinstance(k, int) else tuple(v // 2 for v in k)), **kw)


def test_constructor_takes_the_documented_modules(pkg):
    for k, kind, floor, N in ((3, 'window', None, 0), (3, 'cross', 0.1, 16), ((3, 7), 'window', 0, 5), (7, 'window', -1.5, 0),
                              ((5, 3), 'window', 0.25, 1)):
        m = pkg.CBPoolMax2d(nms(k), generalGeometry=True, suppress=kind, floor=floor, peakList=N)
        kk = (k, k) if isinstance(k, int) else k
        assert m.suppress == kind and m.kernel_size == kk and m.stride == (1, 1) and m.padding == (kk[0] // 2, kk[1] // 2)
        assert m.floor == (None if floor is None else float(floor)) and m.peakCapacity == N
        assert m._general is True and m._adaptive is False and m.generalGeometry is True
        assert list(m._buffers) == ['outputState', 'partials', 'peakBits'] and m.peakBits.dtype == torch.int64
        assert [t.numel() for t in m.getStateTensors()] == [0, 0] and m.getStateTensors()[1] is m.peakBits
        assert repr(m) == 'CBPoolMax2d (k=%s, suppress=%s, floor=%s, peakList=%d, propChgIdxs=False)' % (
            kk, kind, m.floor, N)


def test_constructor_refusals_by_their_words(pkg, lib):
    P, Err = pkg.CBPoolMax2d, lib.CBinferError
    for m, kw, words in (
            (nms(), dict(suppress='ring'), r"suppress='ring' is not supported, only None, 'window' or 'cross'"),
            (nms(), dict(suppress=True), r"suppress=True is not supported"),
            (nms(), dict(generalGeometry=False, suppress='window'), r"suppress='window' needs generalGeometry=True"),
            (nn.AvgPool2d(3, 1, 1), dict(suppress='window'), r"takes an nn.MaxPool2d \(exactly, not a subclass\), got AvgPool2d"),
            (nn.AdaptiveMaxPool2d(1), dict(suppress='window'), r"takes an nn.MaxPool2d .* got AdaptiveMaxPool2d"),
            (type('MyPool', (nn.MaxPool2d,), {})(3, 1, 1), dict(suppress='window'), r"got MyPool"),
            (nn.MaxPool2d(2, 1, 1), dict(suppress='window'), r"needs kernel_size 3, 5 or 7 per axis, got kernel_size=\(2, 2\)"),
            (nn.MaxPool2d(9, 1, 4), dict(suppress='window'), r"got kernel_size=\(9, 9\)"),
            (nn.MaxPool2d((3, 4), 1, (1, 2)), dict(suppress='window'), r"got kernel_size=\(3, 4\)"),
            (nn.MaxPool2d(3, 2, 1), dict(suppress='window'), r"needs stride=1, got stride=\(2, 2\)"),
            (nn.MaxPool2d(3, padding=1), dict(suppress='window'), r"needs stride=1, got stride=\(3, 3\)"),
            (nn.MaxPool2d(5, 1, 1), dict(suppress='window'), r"needs padding=kernel_size // 2 = \(2, 2\), got padding=\(1, 1\)"),
            (nn.MaxPool2d(3, 1, 0), dict(suppress='cross'), r"got padding=\(0, 0\)"),
            (nn.MaxPool2d(3, 1, 1, dilation=2), dict(suppress='window'), r"needs dilation=1, got dilation=2"),
            (nn.MaxPool2d(3, 1, 1, ceil_mode=True), dict(suppress='window'), r"needs ceil_mode=False"),
            (nn.MaxPool2d(3, 1, 1, return_indices=True), dict(suppress='window'), r"does not take return_indices=True"),
            (nms(5), dict(suppress='cross'), r"suppress='cross' is the 3x3 neighbourhood only, got kernel_size=\(5, 5\)"),
            (nms(), dict(suppress='window', floor=float('nan')), r"floor=nan is not supported, only None or a finite number"),
            (nms(), dict(suppress='window', floor=float('inf')), r"floor=inf is not supported"),
            (nms(), dict(suppress='window', floor='0.1'), r"floor='0.1' is not supported"),
            (nms(), dict(suppress='window', floor=True), r"floor=True is not supported"),
            (nms(), dict(suppress='window', peakList=-1), r"peakList=-1 is not supported, only the capacity"),
            (nms(), dict(suppress='window', peakList=2.5), r"peakList=2.5 is not supported"),
            (nms(), dict(suppress='window', peakList=True), r"peakList=True is not supported"),
            (nms(), dict(floor=0.1), r"floor=0.1 has a meaning with suppress='window' or 'cross' only"),
            (nms(), dict(peakList=8), r"peakList=8 has a meaning with suppress='window' or 'cross' only"),
            (nms(), dict(generalGeometry=False, floor=0.0), r"floor=0.0 has a meaning with suppress=")):
        with pytest.raises(Err, match=words):
            P(m, **dict(dict(generalGeometry=True), **kw))
    for kw, words in ((dict(suppress='window'), r"CBPoolAvg2d: suppress='window' is not supported"),
                      (dict(floor=0.0), r"CBPoolAvg2d: floor=0.0 is not supported"),
                      (dict(peakList=4), r"CBPoolAvg2d: peakList=4 is not supported")):
        with pytest.raises(Err, match=words):
            pkg.CBPoolAvg2d(nn.AvgPool2d(3, 1, 1), **kw)
    m = P(nms(), generalGeometry=True, suppress='window')
    with pytest.raises(Err, match="no peak list is made"):
        m.peakList()
    with pytest.raises(Err, match="the peak list is there after the first frame"):
        P(nms(), generalGeometry=True, suppress='window', peakList=4).peakList()
    with pytest.raises(Err, match="HIP devices only"):
        m(torch.zeros(1, 2, 5, 5))
    with pytest.raises(Err, match=r"must be a \[1, C, H, W\] tensor, got \(2, 2, 5, 5\)"):
        m(torch.zeros(2, 2, 5, 5))
    with pytest.raises(Err, match="float32 and float16 tensors only"):
        m(torch.zeros(1, 2, 5, 5, dtype=torch.float64))
    with pytest.raises(Err, match="change indexes must be an int32 tensor or a ChangeIndexes"):
        m(('changeIndexes', torch.zeros(1, 2, 5, 5), None))


def test_defaults_are_todays_module(pkg, lib):
    """Without the new keywords nothing changes: attributes, buffers, repr and state tensors of the plain pools."""
    for m, rep in ((pkg.CBPoolMax2d(nn.MaxPool2d(3, 1, 1), generalGeometry=True),
                    'CBPoolMax2d (k=(3, 3), s=(1, 1), p=(1, 1), ceil_mode=False, propChgIdxs=False)'),
                   (pkg.CBPoolMax2d(nn.MaxPool2d(2, 2)), 'CBPoolMax2d (k=(2, 2), s=(2, 2), ceil_mode=False, propChgIdxs=False)'),
                   (pkg.CBPoolAvg2d(nn.AvgPool2d(3, 2, 1)),
                    'CBPoolAvg2d (k=(3, 3), s=(2, 2), p=(1, 1), ceil_mode=False, count_include_pad=True, propChgIdxs=False)'),
                   (pkg.CBPoolMax2d(nn.AdaptiveMaxPool2d(1), generalGeometry=True),
                    'CBPoolMax2d (output_size=(1, 1), propChgIdxs=False)')):
        assert repr(m) == rep
        assert m.suppress is None and m.floor is None and m.peakCapacity == 0
        assert list(m._buffers) == ['outputState', 'partials'] and not hasattr(m, 'peakBits')
        assert len(m.getStateTensors()) == (2 if m._adaptive else 1) and m.getStateTensors()[0] is m.outputState
        assert list(m.state_dict()) == ['outputState', 'partials']
        m.clearMemory()
        assert list(m._buffers) == ['outputState', 'partials']
    m = pkg.CBPoolMax2d(nn.MaxPool2d(3, 1, 1), generalGeometry=True)
    assert m._op == lib.POOL_MAX and m._general is True and m.lazy is False and m.downsampleIndexes is False


def test_pickle_round_trip_and_back_fill(pkg):
    m = pkg.CBPoolMax2d(nms((3, 7)), generalGeometry=True, suppress='window', floor=0.25, peakList=9)
    m.propChangeIndexes, m.cloneOutput = True, False
    m.outputState = torch.ones(1, 2, 4, 5)
    m.peakBits = torch.arange(8, dtype=torch.int64)
    m.__dict__['_poolWork'] = dict(key=None)
    buf = io.BytesIO()
    torch.save(m, buf)
    buf.seek(0)
    for q in (torch.load(buf, weights_only=False), pickle.loads(pickle.dumps(m)), copy.deepcopy(m)):
        assert type(q) is pkg.CBPoolMax2d and q.suppress == 'window' and q.floor == 0.25 and q.peakCapacity == 9
        assert q.kernel_size == (3, 7) and q.propChangeIndexes is True and q.cloneOutput is False and repr(q) == repr(m)
        assert torch.equal(q.outputState, m.outputState) and torch.equal(q.peakBits, m.peakBits)
        assert q.__dict__['_poolWork'] is None
        q.clearMemory()
        assert q.outputState.numel() == 0 and q.peakBits.numel() == 0 and q.peakBits.dtype == torch.int64
    # a module pickled before the keywords existed loads as a plain pool
    old = pkg.CBPoolMax2d(nn.MaxPool2d(3, 1, 1), generalGeometry=True)
    state = old.__getstate__()
    for name in ('suppress', 'floor', 'peakCapacity'):
        del state[name]
    back = pkg.CBPoolMax2d.__new__(pkg.CBPoolMax2d)
    back.__setstate__(state)
    assert back.suppress is None and back.floor is None and back.peakCapacity == 0
    assert len(back.getStateTensors()) == 1 and repr(back) == repr(old) and list(back._buffers) == ['outputState', 'partials']
    back.clearMemory()
    assert list(back._buffers) == ['outputState', 'partials']


def test_state_tensors_and_clear_memory_through_the_package(pkg):
    net = nn.Sequential(pkg.CBPoolMax2d(nms(), generalGeometry=True, suppress='cross', floor=0.1),
                        pkg.CBPoolMax2d(nn.MaxPool2d(3, 1, 1), generalGeometry=True))
    a, b = net
    a.outputState, a.peakBits = torch.ones(1, 2, 3, 3), torch.ones(6, dtype=torch.int64)
    b.outputState = torch.ones(1, 2, 3, 3)
    tensors = pkg.getStateTensors(net)
    assert len(tensors) == 3 and tensors[0] is a.outputState and tensors[1] is a.peakBits and tensors[2] is b.outputState
    pkg.clearMemory(net)
    assert [t.numel() for t in pkg.getStateTensors(net)] == [0, 0, 0]


# ------------------------------------------------------------------------------------------------ the pass
class SimpleNMS(nn.Module):
    """What a keypoint head writes: the map where it equals its own 3x3 max pool and reaches the floor."""

    def __init__(self, k=3, floor=0.1):
        super(SimpleNMS, self).__init__()
        self.k, self.floor = k, floor

    def forward(self, x):
        keep = (F.max_pool2d(x, self.k, 1, self.k // 2) == x) & (x >= self.floor)
        return torch.where(keep, x, torch.zeros_like(x))


class CrossNMS(nn.Module):
    def forward(self, x):
        p = F.pad(x, (1, 1, 1, 1), value=float('-inf'))
        keep = (x >= p[..., 1:-1, :-2]) & (x >= p[..., 1:-1, 2:]) & (x >= p[..., :-2, 1:-1]) & (x >= p[..., 2:, 1:-1])
        return torch.where(keep, x, torch.zeros_like(x))


class StrictNMS(SimpleNMS):      # (a tie is no peak here: another operator)
    def forward(self, x):
        best = F.max_pool2d(x, self.k, 1, self.k // 2)
        ties = F.avg_pool2d((x == best).float(), self.k, 1, self.k // 2, count_include_pad=True) * self.k * self.k
        return torch.where((best == x) & (x >= self.floor) & (ties < 1.5), x, torch.zeros_like(x))


def _head(pkg, *tail):
    net = pkg.convert(nn.Sequential(nn.Conv2d(3, 4, 3, padding=1), nn.Sigmoid(), *tail), threshold=0.05)
    return pkg.insertCBPointwise(net)


def test_insert_cb_pooling_nms_types(pkg, lib):
    Err = lib.CBinferError
    kw = dict(kernel_size=3, suppress='window', floor=0.1)
    net = pkg.insertCBPooling(_head(pkg, SimpleNMS(), nn.Conv2d(4, 2, 1)), cloneOutput=False, generalGeometry=True,
                              nmsTypes={SimpleNMS: dict(kw, peakList=32)})
    assert type(net[1]) is pkg.CBPointwise2d and net[1].propChangeIndexes is True
    m = net[2]
    assert type(m) is pkg.CBPoolMax2d and m.suppress == 'window' and m.floor == 0.1 and m.peakCapacity == 32
    assert m.kernel_size == (3, 3) and m.cloneOutput is False and net[3].copyInput is True
    # without nmsTypes, or not behind a producer, the class stays what it is; a subclass is another type
    assert type(pkg.insertCBPooling(_head(pkg, SimpleNMS()), generalGeometry=True)[2]) is SimpleNMS
    net = pkg.insertCBPooling(nn.Sequential(nn.Sigmoid(), SimpleNMS()), generalGeometry=True, nmsTypes={SimpleNMS: kw})
    assert type(net[1]) is SimpleNMS
    net = pkg.insertCBPooling(_head(pkg, StrictNMS()), generalGeometry=True, nmsTypes={SimpleNMS: kw})
    assert type(net[2]) is StrictNMS
    # the ordinary pools beside it are converted as before
    net = pkg.insertCBPooling(_head(pkg, nn.MaxPool2d(3, 2, 1)), generalGeometry=True, nmsTypes={SimpleNMS: kw})
    assert type(net[2]) is pkg.CBPoolMax2d and net[2].suppress is None
    # the cross kind, a 5x5 window
    net = pkg.insertCBPooling(_head(pkg, CrossNMS()), generalGeometry=True,
                              nmsTypes={CrossNMS: dict(kernel_size=3, suppress='cross')})
    assert net[2].suppress == 'cross' and net[2].floor is None
    net = pkg.insertCBPooling(_head(pkg, SimpleNMS(5, 0.3)), generalGeometry=True,
                              nmsTypes={SimpleNMS: dict(kernel_size=5, suppress='window', floor=0.3)})
    assert net[2].kernel_size == (5, 5)
    # a class that computes something else is refused by name: another floor, another window, no floor, ties, cross
    for mod, bad in ((SimpleNMS(), dict(kw, floor=0.2)), (SimpleNMS(), dict(kw, kernel_size=5)),
                     (SimpleNMS(), dict(kernel_size=3, suppress='window')), (StrictNMS(), kw),
                     (SimpleNMS(), dict(kw, suppress='cross')), (nn.Identity(), kw)):
        with pytest.raises(Err, match="%s does not compute peak suppression" % type(mod).__name__):
            pkg.insertCBPooling(_head(pkg, mod), generalGeometry=True, nmsTypes={type(mod): bad})
    with pytest.raises(Err, match="nmsTypes needs generalGeometry=True"):
        pkg.insertCBPooling(_head(pkg, SimpleNMS()), nmsTypes={SimpleNMS: kw})
    for bad in ({SimpleNMS: dict(suppress='window')}, {SimpleNMS: dict(kw, stride=1)}, {SimpleNMS: 3}, {'SimpleNMS': kw}):
        with pytest.raises(Err, match="nmsTypes maps a class to the keywords"):
            pkg.insertCBPooling(_head(pkg, SimpleNMS()), generalGeometry=True, nmsTypes=bad)
    with pytest.raises(Err, match="needs kernel_size 3, 5 or 7"):      # (the constructor's refusal is not swallowed)
        pkg.insertCBPooling(_head(pkg, SimpleNMS()), generalGeometry=True, nmsTypes={SimpleNMS: dict(kw, kernel_size=4)})
    # the table of the producers, the passes and the batched operators are what they were
    from cbinfer_amd import batch, chain
    assert len(chain.PRODUCERS) == 23 and len(chain.PASSES) == 11
    assert pkg.CBPoolMax2d not in batch.CHAIN_OPERATORS
    net = pkg.insertCBPooling(_head(pkg, SimpleNMS(), nn.Conv2d(4, 2, 3, padding=1)), generalGeometry=True,
                              nmsTypes={SimpleNMS: kw})
    with pytest.raises(Err):
        pkg.SequenceBatch(net, 2)
