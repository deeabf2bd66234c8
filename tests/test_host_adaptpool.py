"""CPU-only tests of the change-based adaptive pool (CBPoolAvg2d / CBPoolMax2d on an nn.Adaptive*Pool2d,
cb_adaptpool.hip): the numpy twin of tests/adaptpool_cases.py against CPU torch and float64 math, the
constructors and their refusals, pickling, the state surface, the insertCBPooling wiring, the host-pure C functions and
the argument refusals of the C ABI.  No kernel is launched here."""
import copy
import io
import pickle

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import adaptpool_cases as ac
from adaptpool_cases import CASE_IDS, CASES, DTYPES
from optest import lib, pkg      # noqa: F401  (fixtures)


def torch_pool(x, size, op):
    t = torch.from_numpy(x)[None]
    return (F.adaptive_max_pool2d(t, size) if op == "max" else F.adaptive_avg_pool2d(t, size))[0].numpy()


def case_input(cid, dtype):
    return ac.frames(cid, dtype)[0][0]


# ------------------------------------------------------------------------------------------------ the twin
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cid", CASE_IDS)
def test_twin_max_is_torch_bit_for_bit(cid, dtype):
    x = case_input(cid, dtype)
    size = CASES[cid][3]
    _, out = ac.twin(x, size, "max")
    ref = torch_pool(x, size, "max")
    assert out.dtype == ref.dtype and out.shape == ref.shape
    assert np.array_equal(ac.bits_of(out), ac.bits_of(ref))


@pytest.mark.parametrize("dtype", DTYPES)
def test_twin_max_nan_and_signed_zeros(dtype):
    """A NaN in the window wins; of equal maxima the first in row-major window order: {+0, -0, -0, +0} gives +0 and its
    negation -0, also when the first zero of the window stands in a later row than a zero of the other sign's column."""
    dt = ac.np_dtype(dtype)
    z = np.array([[0.0, -0.0], [-0.0, 0.0]], dtype=dt)
    maps = [z, -z, np.array([[-1.0, -0.0], [0.0, -2.0]], dtype=dt), np.array([[-1.0, 0.0], [-0.0, -2.0]], dtype=dt)]
    # the same four values inside a wider map pooled to 2 x 3 (overlapping windows), the rest below zero
    wide = np.full((5, 70), -3.0, dtype=dt)
    wide[1:3, 22:24] = -z
    maps.append(wide)
    for m, size in zip(maps, ((1, 1),) * 4 + ((2, 3),)):
        x = m[None]
        _, out = ac.twin(x, size, "max")
        assert np.array_equal(ac.bits_of(out), ac.bits_of(torch_pool(x, size, "max"))), (m, size)
    assert np.signbit(ac.twin(z[None], (1, 1), "max")[1]).item() is False
    assert np.signbit(ac.twin(-z[None], (1, 1), "max")[1]).item() is True
    # NaN: wins in its windows, leaves the others torch's bits
    rng = np.random.default_rng(3)
    x = rng.standard_normal((2, 5, 70)).astype(dt)
    x[0, 2, 23] = np.nan      # row 2 lies in both row windows, column 23 in the first two column windows of 70 -> 3
    x[1, 4, 69] = np.nan      # the last pixel: one window
    _, out = ac.twin(x, (2, 3), "max")
    ref = torch_pool(x, (2, 3), "max")
    assert np.array_equal(np.isnan(out), np.isnan(ref)) and np.isnan(out).sum() == 5
    assert np.array_equal(ac.bits_of(out)[~np.isnan(ref)], ac.bits_of(ref)[~np.isnan(ref)])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cid", CASE_IDS)
def test_twin_avg_within_the_derived_bound_of_float64_and_of_torch(cid, dtype):
    """|twin - exact| <= 1.01 (D + 1) 2^-24 mean|x| over the window, D the additions on the longest path of the
    specified order (level 1: strided lane sums and tree; level 2: ascending), + 1 for the division.  fp16 adds the one
    rounding of the result: 2^-11 |result|, or half the spacing of the f16 subnormals (2^-25) where that is more.  The
    same bound holds against torch's own operator (whose order is another one)."""
    x = case_input(cid, dtype)
    Cn, H, W, size = CASES[cid]
    oh, ow = ac.out_size(H, W, size)
    _, out = ac.twin(x, size, "avg")
    ref = torch_pool(x, size, "avg").astype(np.float64)
    x64 = x.astype(np.float64)
    for i in range(oh):
        r0, r1 = ac.lo(i, H, oh), ac.hi(i, H, oh)
        for j in range(ow):
            c0, c1 = ac.lo(j, W, ow), ac.hi(j, W, ow)
            win = x64[:, r0:r1, c0:c1].reshape(Cn, -1)
            exact = win.mean(axis=1)
            D = ac.depth(r1 - r0, c1 - c0, H, W, oh, ow)
            bound = 1.01 * (D + 1) * 2.0 ** -24 * np.abs(win).mean(axis=1)
            if dtype == "f16":
                bound = bound + np.maximum(2.0 ** -11 * np.abs(exact), 2.0 ** -25)
            got = out[:, i, j].astype(np.float64)
            assert np.all(np.abs(got - exact) <= bound), (i, j, np.abs(got - exact).max(), bound.min())
            assert np.all(np.abs(got - ref[:, i, j]) <= bound), (i, j)


def test_twin_avg_is_not_torchs_order_and_depth_counts_the_order():
    """What the header says: the two-level sum is not torch's bits (5 x 70 -> 2 x 3, fp32), and D is computed from the
    window: 24 columns on 32 lanes, 3 rows on 4 lanes: 0 + 5 + 0 + 2."""
    x = case_input("overlap_bit63", "f32")[:3, :, :70].copy()
    _, out = ac.twin(x, (2, 3), "avg")
    assert (ac.bits_of(out) != ac.bits_of(torch_pool(x, (2, 3), "avg"))).sum() > 0
    assert ac.lanes(70, 3) == 32 and ac.lanes(5, 2) == 4 and ac.depth(3, 24, 5, 70, 2, 3) == 7
    assert ac.lanes(70, 1) == 64 and ac.lanes(7, 1) == 8 and ac.depth(7, 70, 7, 70, 1, 1) == 1 + 6 + 0 + 3
    assert ac.lanes(320, 1) == 64 and ac.depth(320, 480, 320, 480, 1, 1) == 7 + 6 + 4 + 6
    assert ac.lanes(5, 5) == 1 and ac.depth(1, 1, 4, 5, 4, 5) == 0


def test_twin_windows_are_torchs_and_a_row_lies_in_one_or_two():
    for N, o in ((7, 1), (5, 2), (13, 6), (9, 7), (4, 4), (70, 3), (130, 3), (200, 1), (64, 2), (1, 1), (31, 30)):
        member = np.zeros((o, N), dtype=bool)
        for i in range(o):
            assert 0 <= ac.lo(i, N, o) < ac.hi(i, N, o) <= N
            member[i, ac.lo(i, N, o):ac.hi(i, N, o)] = True
            assert ac.hi(i, N, o) - ac.lo(i, N, o) <= (N // o if N % o == 0 else N // o + 2)
        # torch's windows: the maximum of a ramp is the window's last element, of the reversed ramp its first
        ramp = torch.arange(N, dtype=torch.float32)[None, None]
        assert F.adaptive_max_pool1d(ramp, o)[0, 0].tolist() == [ac.hi(i, N, o) - 1 for i in range(o)]
        assert F.adaptive_max_pool1d(-ramp, o)[0, 0].tolist() == [-ac.lo(i, N, o) for i in range(o)]
        for y in range(N):
            assert list(ac.rows_of(y, N, o)) == list(np.flatnonzero(member[:, y])) and 1 <= len(ac.rows_of(y, N, o)) <= 2


# ------------------------------------------------------------------------------------------------ the modules
def test_constructors_accept_exactly_the_adaptive_modules(pkg, lib):
    """Fails on the parent commit: CBPoolAvg2d(nn.AdaptiveAvgPool2d(1)) raised 'only nn.AvgPool2d modules are
    converted'."""
    a = pkg.CBPoolAvg2d(nn.AdaptiveAvgPool2d(1))
    m = pkg.CBPoolMax2d(nn.AdaptiveMaxPool2d((None, 3)), generalGeometry=True)
    for mod, size, op in ((a, (1, 1), lib.ADAPT_AVG), (m, (None, 3), lib.ADAPT_MAX)):
        assert mod._adaptive is True and mod._general is True and mod.generalGeometry is True and mod.lazy is False
        assert mod.output_size == size and mod._op == op and 'output_size=%s' % (size,) in repr(mod)
        assert mod.cloneOutput is True and mod.propChangeIndexes is False
        assert [k for k, _ in mod.named_buffers()] == ['outputState', 'partials']
        assert mod.outputState.numel() == 0 and mod.partials.numel() == 0
    assert pkg.CBPoolAvg2d(nn.AdaptiveAvgPool2d((7, None))).output_size == (7, None)
    assert pkg.CBPoolMax2d(nn.AdaptiveMaxPool2d([2, 3]), generalGeometry=True).output_size == (2, 3)
    # the other modules are what they were: no adaptive flag set, the partials empty and not part of the state list
    for mod in (pkg.CBPoolAvg2d(nn.AvgPool2d(2)), pkg.CBPoolMax2d(nn.MaxPool2d(2, 2)),
                pkg.CBPoolMax2d(nn.MaxPool2d(3, 2, 1), generalGeometry=True)):
        assert mod._adaptive is False and mod.partials.numel() == 0 and len(mod.getStateTensors()) == 1
        assert 'output_size' not in repr(mod)


def test_constructor_refusals(pkg, lib):
    Err = lib.CBinferError

    class MyAvg(nn.AdaptiveAvgPool2d):
        pass

    class MyMax(nn.AdaptiveMaxPool2d):
        pass

    for make, what in (
            (lambda: pkg.CBPoolMax2d(nn.AdaptiveMaxPool2d(1, return_indices=True), generalGeometry=True),
             "return_indices=True is not supported"),
            (lambda: pkg.CBPoolMax2d(nn.AdaptiveMaxPool2d(1), generalGeometry=False), "pass generalGeometry=True"),
            (lambda: pkg.CBPoolMax2d(nn.AdaptiveMaxPool2d(1)), "pass generalGeometry=True"),
            (lambda: pkg.CBPoolAvg2d(nn.AdaptiveAvgPool2d(0)), r"output_size=0 is not supported"),
            (lambda: pkg.CBPoolAvg2d(nn.AdaptiveAvgPool2d((1, 2, 3))), r"output_size=\(1, 2, 3\) is not supported"),
            (lambda: pkg.CBPoolAvg2d(nn.AdaptiveAvgPool2d((2.0, 2))), "is not supported"),
            # every other module type: the words they always had -- a subclass is not the type
            (lambda: pkg.CBPoolAvg2d(MyAvg(1)), "^CBPoolAvg2d: only nn.AvgPool2d modules are converted$"),
            (lambda: pkg.CBPoolMax2d(MyMax(1), generalGeometry=True),
             "^CBPoolMax2d: only nn.MaxPool2d modules are converted$"),
            (lambda: pkg.CBPoolAvg2d(nn.AdaptiveMaxPool2d(1)), "^CBPoolAvg2d: only nn.AvgPool2d modules are converted$"),
            (lambda: pkg.CBPoolMax2d(nn.AdaptiveAvgPool2d(1), generalGeometry=True),
             "^CBPoolMax2d: only nn.MaxPool2d modules are converted$"),
            (lambda: pkg.CBPoolAvg2d(nn.MaxPool2d(2)), "^CBPoolAvg2d: only nn.AvgPool2d modules are converted$"),
            (lambda: pkg.CBPoolAvg2d(nn.AvgPool2d(2, divisor_override=3)), "divisor_override=3 is not supported")):
        with pytest.raises(Err, match=what):
            make()
    # at the first frame, naming the map: an output size larger than the map on an axis
    m = pkg.CBPoolAvg2d(nn.AdaptiveAvgPool2d((7, None)))
    assert m._adaptive_out(9, 65) == (7, 65)
    with pytest.raises(Err, match=r"output_size=\(7, 5\) is larger than the 6x5 map"):
        m._adaptive_out(6, 5)
    with pytest.raises(Err, match="HIP devices only"):
        m(('changeIndexes', torch.zeros(1, 2, 9, 9), None))


def test_pickle_round_trip_and_old_pickles(pkg, lib):
    m = pkg.CBPoolMax2d(nn.AdaptiveMaxPool2d((2, None)), generalGeometry=True)
    m.propChangeIndexes = True
    m.cloneOutput = False
    m.outputState = torch.ones(1, 2, 2, 5)
    m.partials = torch.ones(2, 5, 4)
    buf = io.BytesIO()
    torch.save(m, buf)
    buf.seek(0)
    r = torch.load(buf, weights_only=False)
    r2 = pickle.loads(pickle.dumps(m))
    r3 = copy.deepcopy(m)
    for q in (r, r2, r3):
        assert type(q) is pkg.CBPoolMax2d and q._adaptive is True and q._general is True and q.output_size == (2, None)
        assert q.propChangeIndexes is True and q.cloneOutput is False and q._op == lib.ADAPT_MAX
        assert torch.equal(q.outputState, m.outputState) and torch.equal(q.partials, m.partials)
        assert q.__dict__['_poolWork'] is None and repr(q) == repr(m)
    a = pickle.loads(pickle.dumps(pkg.CBPoolAvg2d(nn.AdaptiveAvgPool2d(1))))
    assert a._adaptive is True and a.output_size == (1, 1) and a._op == lib.ADAPT_AVG
    # a module pickled before the adaptive pool existed: no flag, no partials buffer
    old = pkg.CBPoolAvg2d(nn.AvgPool2d(3, 2, 1))
    state = old.__getstate__()
    del state['_adaptive']
    state['_buffers'] = type(state['_buffers'])((k, v) for k, v in state['_buffers'].items() if k != 'partials')
    back = pkg.CBPoolAvg2d.__new__(pkg.CBPoolAvg2d)
    back.__setstate__(state)
    assert back._adaptive is False and back.partials.numel() == 0 and back._general is True
    assert len(back.getStateTensors()) == 1 and 'k=(3, 3)' in repr(back)
    back.clearMemory()
    assert list(back._buffers) == ['outputState', 'partials']


def test_clear_memory_and_state_tensors(pkg):
    net = nn.Sequential(pkg.CBPoolAvg2d(nn.AdaptiveAvgPool2d(1)), pkg.CBPoolAvg2d(nn.AvgPool2d(2)))
    a, b = net[0], net[1]
    a.outputState, a.partials = torch.ones(1, 3, 1, 1), torch.ones(3, 1, 7)
    b.outputState = torch.ones(1, 3, 2, 2)
    a.__dict__['_poolWork'] = dict(key=None)
    tensors = pkg.getStateTensors(net)
    assert len(tensors) == 3 and tensors[0] is a.outputState and tensors[1] is a.partials and tensors[2] is b.outputState
    pkg.clearMemory(net)
    assert a.outputState.numel() == 0 and a.partials.numel() == 0 and b.outputState.numel() == 0
    assert a.__dict__['_poolWork'] is None
    assert [t.numel() for t in pkg.getStateTensors(net)] == [0, 0, 0]


def _head(pkg, pool, tail=None):
    conv = nn.Conv2d(3, 4, 3, padding=1)
    mods = [conv, pool] + ([tail] if tail is not None else [])
    return pkg.convert(nn.Sequential(*mods), threshold=0.05)


def test_insert_cb_pooling_wiring(pkg, lib):
    # the default leaves the module the dense torch operator, with or without generalGeometry
    for kwargs in (dict(), dict(generalGeometry=True), dict(generalGeometry=True, adaptive=False)):
        net = pkg.insertCBPooling(_head(pkg, nn.AdaptiveAvgPool2d(1)), **kwargs)
        assert type(net[1]) is nn.AdaptiveAvgPool2d and net[0].propChangeIndexes is False
    with pytest.raises(lib.CBinferError, match="adaptive=True needs generalGeometry=True"):
        pkg.insertCBPooling(_head(pkg, nn.AdaptiveAvgPool2d(1)), adaptive=True)
    # adaptive=True: both modules behind a CBConv2d, cloneOutput handed on, the consumer rule for a CBConv2d behind
    for pool, cls in ((nn.AdaptiveAvgPool2d(1), pkg.CBPoolAvg2d), (nn.AdaptiveMaxPool2d((2, 3)), pkg.CBPoolMax2d)):
        for clone in (True, False):
            net = pkg.insertCBPooling(_head(pkg, pool, nn.Conv2d(4, 2, 1)), cloneOutput=clone, generalGeometry=True,
                                      adaptive=True)
            assert type(net[1]) is cls and net[1]._adaptive and net[1].cloneOutput is clone
            assert net[0].propChangeIndexes is True and net[2].copyInput is True
    # the same producers as the general pools: behind a CBPointwise2d too, not behind a dense operator
    net = nn.Sequential(pkg.CBPointwise2d(nn.Hardswish()), nn.AdaptiveMaxPool2d(1), nn.Sigmoid(), nn.AdaptiveAvgPool2d(1))
    pkg.insertCBPooling(net, generalGeometry=True, adaptive=True)
    assert type(net[1]) is pkg.CBPoolMax2d and net[0].propChangeIndexes is True and type(net[3]) is nn.AdaptiveAvgPool2d
    # a module the constructor refuses stays dense; the ordinary pools are converted as before
    net = pkg.insertCBPooling(_head(pkg, nn.AdaptiveMaxPool2d(1, return_indices=True)), generalGeometry=True, adaptive=True)
    assert type(net[1]) is nn.AdaptiveMaxPool2d
    net = pkg.insertCBPooling(_head(pkg, nn.AvgPool2d(2)), generalGeometry=True, adaptive=True)
    assert type(net[1]) is pkg.CBPoolAvg2d and net[1]._adaptive is False
    # the other passes treat an adaptive instance as a general pool: never folded, refused by a SequenceBatch
    net = pkg.insertCBPooling(_head(pkg, nn.AdaptiveMaxPool2d(2), nn.Conv2d(4, 2, 3, padding=1)), generalGeometry=True,
                              adaptive=True)
    net[2].feedbackLoop = True
    pkg.fusePoolingIntoDetection(net)
    assert net[1].lazy is False
    with pytest.raises(lib.CBinferError, match="never folded into the next detection"):
        pkg.SequenceBatch(net, 2)


# ------------------------------------------------------------------------------------------------ the C ABI
def test_host_pure_functions(lib):
    C = lib.C
    assert lib.ADAPT_MAX == 0 and lib.ADAPT_AVG == 1 and C.cbinfer_abi_version() == 11
    for Cn, H, W, size in CASES.values():
        oh, ow = ac.out_size(H, W, size)
        assert C.cbinfer_adaptive_pool_supported(H, W, oh, ow) == 1
        assert C.cbinfer_adaptive_pool_partial_elems(Cn, H, W, oh, ow) == Cn * H * ow
        assert C.cbinfer_adaptive_pool_lanes(W, ow) == ac.lanes(W, ow)
    for N in range(1, 140):
        for o in range(1, N + 1):
            assert C.cbinfer_adaptive_pool_lanes(N, o) == ac.lanes(N, o)
    assert C.cbinfer_adaptive_pool_lanes(480, 1) == 64 and C.cbinfer_adaptive_pool_lanes(80, 6) == 16
    assert C.cbinfer_adaptive_pool_lanes(0, 1) == 1 and C.cbinfer_adaptive_pool_lanes(4, 5) == 1
    for H, W, oh, ow in ((0, 5, 1, 1), (5, 0, 1, 1), (5, 5, 0, 1), (5, 5, 1, 0), (5, 5, 6, 1), (5, 5, 1, 6),
                         (8, 5000, 1, 4097), (1 << 16, 1 << 15, 1, 1)):
        assert C.cbinfer_adaptive_pool_supported(H, W, oh, ow) == 0
        assert C.cbinfer_adaptive_pool_partial_elems(3, H, W, oh, ow) == 0
    assert C.cbinfer_adaptive_pool_supported(8, 5000, 8, 4096) == 1
    assert C.cbinfer_adaptive_pool_partial_elems(0, 5, 5, 1, 1) == 0
    assert C.cbinfer_adaptive_pool_partial_elems(1 << 25, 5, 5, 1, 1) == 0            # (64 C beyond an int32)
    assert C.cbinfer_adaptive_pool_partial_elems(1 << 20, 1 << 12, 8, 1, 1) == 0      # (C H ow beyond an int32)


def test_c_entry_points_check_their_arguments(lib):
    """Bad arguments return CB_ERR_BADARG (-1) or CB_ERR_UNSUPPORTED (-2) before anything is launched (the pointers
    here are never followed)."""
    C = lib.C
    X, P, O, M, L, CNT, INB, OUTB, COPY = (0x100000 * i for i in range(1, 10))

    def fwd(x=X, p=P, o=O, mask=None, lst=None, cap=0, cnt=None, inb=INB, outb=OUTB, cp=COPY, Cn=3, H=7, W=70, oh=2, ow=3,
            op=lib.ADAPT_AVG, dt=lib.CB_F32):
        return C.cbinfer_cbadaptivepool2d_forward(x, p, o, mask, lst, cap, cnt, inb, outb, cp, Cn, H, W, oh, ow, op, dt,
                                                  None)

    def part(x=X, p=P, mask=M, inb=None, every=0, outb=OUTB, Cn=3, H=7, W=70, oh=2, ow=3, op=lib.ADAPT_MAX,
             dt=lib.CB_F16):
        return C.cbinfer_adaptive_pool_partials(x, p, mask, inb, every, outb, Cn, H, W, oh, ow, op, dt, None)

    def chg(p=P, o=O, inb=None, outb=OUTB, cp=COPY, Cn=3, H=7, W=70, oh=2, ow=3, op=lib.ADAPT_MAX, dt=lib.CB_F32):
        return C.cbinfer_adaptive_pool_changed(p, o, inb, outb, cp, Cn, H, W, oh, ow, op, dt, None)

    shapes_bad = (dict(Cn=0), dict(H=0), dict(W=-1), dict(oh=0), dict(ow=0), dict(oh=8), dict(ow=71), dict(op=2),
                  dict(op=-1), dict(dt=lib.CB_F32S), dict(dt=7))
    shapes_unsupported = (dict(W=5000, ow=4097), dict(H=1 << 16, W=1 << 15), dict(Cn=1 << 25),
                          dict(Cn=1 << 20, H=1 << 12, oh=1, ow=1))
    for call in (fwd, part, chg):
        for bad in shapes_bad:
            assert call(**bad) == -1, (call.__name__, bad)
        for bad in shapes_unsupported:
            assert call(**bad) == -2, (call.__name__, bad)
    for bad in (dict(x=None), dict(p=None), dict(o=None), dict(outb=None), dict(cp=None), dict(cp=OUTB), dict(o=X),
                dict(p=X), dict(o=P), dict(mask=M, lst=L, cap=4), dict(cnt=CNT), dict(mask=M, cnt=CNT),
                dict(lst=L, cap=-1), dict(lst=L, cap=4, inb=None), dict(lst=L, cap=4, inb=OUTB),
                dict(lst=L, cap=4, inb=COPY), dict(mask=OUTB), dict(mask=COPY), dict(mask=INB)):
        assert fwd(**bad) == -1, bad
    for bad in (dict(x=None), dict(p=None), dict(outb=None), dict(mask=None), dict(mask=OUTB), dict(mask=None, inb=OUTB),
                dict(p=X)):
        assert part(**bad) == -1, bad
    for bad in (dict(p=None), dict(o=None), dict(outb=None), dict(cp=None), dict(cp=OUTB), dict(inb=OUTB),
                dict(inb=COPY), dict(o=P)):
        assert chg(**bad) == -1, bad
