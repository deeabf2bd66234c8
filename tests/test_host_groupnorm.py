"""CPU-only tests of the change-based group norm (CBGroupNorm2d, insertCBGroupNorm; cb_groupnorm.hip):
the numpy twin of tests/groupnorm_cases.py against torch's float64 operators, the argument checks of the C entry points,
the module's refusals, buffers, pickling and wiring.  No kernel is launched here."""
import copy
import ctypes
import pickle

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import groupnorm_cases as gn
from optest import lib, names_of, pkg      # noqa: F401  (fixtures)


def torch64(a, G, gamma, beta, relu, instance=False):
    x = torch.from_numpy(a.astype(np.float64))[None]
    w = torch.from_numpy(gamma.astype(np.float64)) if gamma is not None else None
    b = torch.from_numpy(beta.astype(np.float64)) if beta is not None else None
    y = F.instance_norm(x, weight=w, bias=b, eps=gn.EPS) if instance else F.group_norm(x, G, w, b, gn.EPS)
    return (F.relu(y) if relu else y)[0].numpy()


# ------------------------------------------------------------------------------------------------ the twin
@pytest.mark.parametrize("dtype", [np.float32, np.float16])
def test_twin_at_threshold_zero_is_the_dense_operator_within_the_bound(dtype):
    """threshold = 0, a fresh frame and a frame with a sparse change: the twin's state is within bound() of
    F.group_norm / F.instance_norm in float64 on the stored operand, with and without the affine and the ReLU; the
    float64 reference of groupnorm_cases is torch's own."""
    rng = np.random.default_rng(3)
    worst = 0.0
    for (Cn, G) in gn.CASES:
        for (H, W) in gn.MAPS:
            for aff, relu in ((True, True), (True, False), (False, False)):
                gamma, beta = gn.affine(rng, Cn) if aff else (None, None)
                a = (rng.standard_normal((Cn, H, W)) * 2 + rng.uniform(-3, 3, Cn)[:, None, None]).astype(dtype)
                P = gn.segment_partials(a)
                held, tripped, out, mask, written = gn.step(a, gn.statistics(P, G, H, W), np.zeros((2, G), np.float32),
                                                            None, 0.0, True, G, gamma, beta, relu)
                assert tripped.all() and mask.all() and written.all()
                for t in range(2):
                    if t:
                        S = rng.random((H, W)) < 0.1
                        a = a.copy()
                        a[:, S] = rng.standard_normal((Cn, int(S.sum()))).astype(dtype)
                        P = gn.update_partials(P, a, S)
                        assert np.array_equal(P, gn.segment_partials(a))      # (the dirty segments are all that moved)
                        held, tripped, out, mask, written = gn.step(a, gn.statistics(P, G, H, W), held, S, 0.0, False, G,
                                                                    gamma, beta, relu, prev=out)
                    want = torch64(a, G, gamma, beta, relu, instance=(G == Cn))
                    ref = gn.reference64(a, G, gn.EPS, gamma, beta, relu)[0]
                    assert np.allclose(ref, want, rtol=1e-12, atol=1e-12)
                    err, bound = np.abs(out.astype(np.float64) - want), gn.bound(a, G, gn.EPS, gamma, beta, relu)
                    assert (err <= bound).all(), (Cn, G, H, W, aff, relu, t, float((err / bound).max()))
                    # (the bound says something: three digits of the value in front of the ReLU at the least)
                    assert (bound <= 2e-3 * (1 + np.abs(gn.reference64(a, G, gn.EPS, gamma, beta)[0]))).all()
                    worst = max(worst, float((err / bound).max()))
    print("worst err / bound of the twin against float64: %.3g" % worst)


def test_twin_holds_trips_and_drifts():
    """The rule on numbers that are exact in float32: statistics at held +- threshold hold (the comparison is strict),
    one unit beyond trips; the rstd test is relative; a NaN trips; a drift of 0.375 threshold per frame holds twice and
    trips in the third frame, and a tripped group takes BOTH values."""
    held = np.array([[1.0, -2.0, 3.0, 0.0], [2.0, 0.5, 1.0, 4.0]], np.float32)
    th = 0.25
    # mean: |d| * rstd <= th  <=>  |d| <= th / rstd
    stats = held.copy()
    stats[0] += np.array([0.125, -0.5, 0.25, 0.0625], np.float32)
    new, tripped = gn.rule(stats, held, th, False)
    assert not tripped.any() and gn.same_bits(new, held)
    stats[0, 1] = np.nextafter(np.float32(-2.5), np.float32(-3))
    new, tripped = gn.rule(stats, held, th, False)
    assert list(tripped) == [False, True, False, False] and new[0, 1] == stats[0, 1]
    # rstd: |d| <= th * rstd
    stats = held.copy()
    stats[1] += np.array([0.5, -0.125, 0.25, 1.0], np.float32)
    assert not gn.rule(stats, held, th, False)[1].any()
    stats[1, 3] = np.nextafter(np.float32(5.0), np.float32(6))
    stats[0, 3] = 7.0
    new, tripped = gn.rule(stats, held, th, False)
    assert list(tripped) == [False, False, False, True] and new[0, 3] == 7.0 and new[1, 3] == stats[1, 3]
    stats = held.copy()
    stats[1, 0] = np.nan
    new, tripped = gn.rule(stats, held, th, False)
    assert list(tripped) == [True, False, False, False] and np.isnan(new[1, 0])
    assert gn.rule(held, held, 0.0, False)[1].sum() == 0 and gn.rule(held, held, 0.0, True)[1].all()
    h = held.copy()
    for t, want in ((1, False), (2, False), (3, True)):
        stats = held.copy()
        stats[0] = held[0] + np.float32(0.375 * th * t) / held[1]
        h, tripped = gn.rule(stats, h, th, False)
        assert tripped.all() == want and tripped.any() == want, t
    assert gn.same_bits(h, stats)
    # a frame: nothing listed and nothing tripped writes nothing and hands on an empty mask; a tripped group writes its
    # planes alone and the mask is full
    a = np.arange(4 * 2 * 5, dtype=np.float32).reshape(4, 2, 5)
    none = np.zeros((2, 5), bool)
    held2 = held[:, :2].copy()
    new, tripped, out, mask, written = gn.step(a, held2, held2, none, th, False, 2)
    assert not tripped.any() and not mask.any() and not written.any()
    stats = held2.copy()
    stats[0, 1] = 9.0
    new, tripped, out, mask, written = gn.step(a, stats, held2, none, th, False, 2)
    assert list(tripped) == [False, True] and mask.all() and written[2:].all() and not written[:2].any()


def test_large_mean_needs_the_float64_level():
    """Values 1000 + N(0, 1) in float32: the twin is within bound() of float64 math, the same twin with its statistics
    taken in float32 is not -- E[x^2] - mean^2 cancels there."""
    rng = np.random.default_rng(7)
    for (Cn, G), (H, W) in zip(gn.CASES, gn.MAPS + gn.MAPS[:1]):
        a = (1000.0 + rng.standard_normal((Cn, H, W))).astype(np.float32)
        want = torch64(a, G, None, None, False)
        bound = gn.bound(a, G)
        zero = np.zeros((2, G), np.float32)
        good = gn.step(a, gn.statistics(gn.segment_partials(a), G, H, W), zero, None, 0.0, True, G)[2]
        poor = gn.step(a, gn.statistics_f32(a, G), zero, None, 0.0, True, G)[2]
        assert (np.abs(good - want) <= bound).all(), (Cn, G, H, W)
        assert (np.abs(poor - want) > bound).any(), (Cn, G, H, W)
        print((Cn, G, H, W), "float64 statistics: worst err / bound %.3g, float32 statistics: %.3g"
              % (float((np.abs(good - want) / bound).max()), float((np.abs(poor - want) / bound).max())))


@pytest.mark.parametrize("dtype", [np.float32, np.float16])
def test_frame_script_trips_as_intended(dtype):
    """The five frames the GPU test runs, on the twin alone: every group trips in the fresh frame, none in the next
    three, exactly the last group in the fifth; most segments of the sparse frames stay clean on the wide maps."""
    th = 0.05
    for (Cn, G) in gn.CASES:
        for (H, W) in gn.MAPS:
            rng = np.random.default_rng(100 * Cn + W)
            held, P, seq = np.zeros((2, G), np.float32), None, []
            for t, (label, a, S) in enumerate(gn.frame_script(rng, Cn, G, H, W, dtype, th)):
                P = gn.segment_partials(a) if t == 0 else gn.update_partials(P, a, S)
                held, tripped = gn.rule(gn.statistics(P, G, H, W), held, th, t == 0)
                seq.append(list(np.flatnonzero(tripped)))
            assert seq == [list(range(G)), [], [], [], [G - 1]], (Cn, G, H, W, seq)


# ------------------------------------------------------------------------------------------------ the C entry points
def test_supported_and_bad_arguments(lib):
    C = lib.C
    assert lib.ABI_VERSION == 11
    assert all(C.cbinfer_groupnorm_supported(*a) == 1 for a in [(1, 1), (4096, 1), (4096, 4096), (6, 2), (6, 6), (48, 3)])
    assert all(C.cbinfer_groupnorm_supported(*a) == 0
               for a in [(0, 1), (4097, 1), (6, 4), (6, 0), (6, -1), (6, 12), (-6, 2), (8192, 2)])
    # every refusal comes before the first launch: no device pointer below is ever read; eps is a HOST pointer
    p = [0x1000 * (i + 1) for i in range(12)]
    a, out, gamma, beta, part, stats, held, trip, bits, mcopy, mask, other = p
    eps = (ctypes.c_double * 1)(1e-5)

    def forward(**kw):
        args = dict(a=a, gamma=gamma, beta=beta, outputState=out, partials=part, stats=stats, held=held, tripped=trip,
                    maskA=None, listA=None, capA=0, countA=None, bits=bits, maskCopy=mcopy, C=8, G=2, H=4, W=70, eps=eps,
                    relu=0, threshold=0.1, all=0, dtype=lib.CB_F32, stream=None)
        args.update(kw)
        return C.cbinfer_cbgroupnorm_forward(*C.cbinfer_cbgroupnorm_forward.pack(**args))

    def eps_of(v):
        return (ctypes.c_double * 1)(v)
    for kw in (dict(a=None), dict(outputState=None), dict(partials=None), dict(stats=None), dict(held=None),
               dict(tripped=None), dict(bits=None), dict(maskCopy=None), dict(eps=None), dict(C=0), dict(C=4097, G=1),
               dict(G=0), dict(G=3), dict(G=16), dict(H=0), dict(W=0), dict(dtype=7), dict(relu=2), dict(relu=-1),
               dict(threshold=-0.5), dict(threshold=float('nan')), dict(eps=eps_of(-1e-5)), dict(eps=eps_of(float('nan'))),
               dict(eps=eps_of(float('inf'))), dict(outputState=a), dict(partials=a), dict(partials=out), dict(stats=held),
               dict(stats=out), dict(held=out), dict(tripped=out), dict(maskCopy=bits), dict(maskA=bits), dict(maskA=mcopy),
               dict(maskA=mask, listA=other), dict(countA=mask), dict(listA=mask, capA=-1), dict(H=1 << 16, W=1 << 15)):
        assert forward(**kw) == lib.CB_ERR_BADARG, kw
    assert C.cbinfer_groupnorm_partials(None, part, None, bits, 0, 8, 4, 70, lib.CB_F32, None) == lib.CB_ERR_BADARG
    assert C.cbinfer_groupnorm_partials(a, part, bits, bits, 0, 8, 4, 70, lib.CB_F32, None) == lib.CB_ERR_BADARG
    assert C.cbinfer_groupnorm_partials(a, part, None, bits, 0, 4097, 4, 70, lib.CB_F32, None) == lib.CB_ERR_BADARG
    assert C.cbinfer_groupnorm_stats(part, stats, stats, trip, 8, 2, 4, 70, eps, 0.1, 0, None) == lib.CB_ERR_BADARG
    assert C.cbinfer_groupnorm_stats(part, stats, held, trip, 8, 3, 4, 70, eps, 0.1, 0, None) == lib.CB_ERR_BADARG
    assert C.cbinfer_groupnorm_stats(part, stats, held, trip, 8, 2, 4, 70, None, 0.1, 0, None) == lib.CB_ERR_BADARG
    assert C.cbinfer_groupnorm_changed(a, a, gamma, beta, held, trip, None, 0, bits, mcopy, 8, 2, 4, 70, 0, lib.CB_F32,
                                       None) == lib.CB_ERR_BADARG
    assert C.cbinfer_groupnorm_changed(a, out, None, None, held, trip, None, 0, bits, bits, 8, 2, 4, 70, 0, lib.CB_F32,
                                       None) == lib.CB_ERR_BADARG
    # (all five are launchers but the capability query: a FrameProgram records them)
    assert [getattr(C, 'cbinfer_' + n).launcher for n in ('groupnorm_supported', 'groupnorm_partials', 'groupnorm_stats',
                                                          'groupnorm_changed', 'cbgroupnorm_forward')] == [False] + [True] * 4


# ------------------------------------------------------------------------------------------------ the module
class MyGroupNorm(nn.GroupNorm):
    pass


class MyInstanceNorm(nn.InstanceNorm2d):
    pass


def test_refusals_by_name(pkg, lib):
    Err = lib.CBinferError
    lopsided = nn.GroupNorm(2, 8)
    lopsided.num_groups = 3
    for call, what in (
            (lambda: pkg.CBGroupNorm2d(MyGroupNorm(2, 8), 0.1), r"MyGroupNorm is not supported, only an nn.GroupNorm or an "
                                                                  r"nn.InstanceNorm2d \(exactly those types"),
            (lambda: pkg.CBGroupNorm2d(MyInstanceNorm(8), 0.1), r"MyInstanceNorm is not supported"),
            (lambda: pkg.CBGroupNorm2d(nn.BatchNorm2d(8), 0.1), r"BatchNorm2d is not supported"),
            (lambda: pkg.CBGroupNorm2d(nn.InstanceNorm2d(8, track_running_stats=True), 0.1),
             r"track_running_stats=True normalises with its running statistics in eval mode: that is a per-channel affine"),
            (lambda: pkg.CBGroupNorm2d(lopsided, 0.1), r"3 groups do not divide 8 channels"),
            (lambda: pkg.CBGroupNorm2d(nn.GroupNorm(1, 4100), 0.1), r"4100 channels, the library takes C <= 4096"),
            (lambda: pkg.CBGroupNorm2d(nn.GroupNorm(2, 8), -0.1), r"threshold=-0.1 must be a number >= 0"),
            (lambda: pkg.CBGroupNorm2d(nn.GroupNorm(2, 8), float('nan')), r"threshold=nan must be a number >= 0"),
            (lambda: pkg.CBGroupNorm2d(nn.GroupNorm(2, 8, eps=-1.0), 0.1), r"eps=-1.0 must be a finite number >= 0")):
        with pytest.raises(Err, match=what):
            call()
    m = pkg.CBGroupNorm2d(nn.GroupNorm(2, 8), 0.1)
    x = torch.zeros(1, 8, 4, 6)
    for call, what in (
            (lambda: m(torch.zeros(1, 6, 4, 6)), r"operand a has 6 channels, the norm was made for 8"),
            (lambda: m(torch.zeros(2, 8, 4, 6)), r"operand a must be a \[1, C, H, W\] tensor, got \(2, 8, 4, 6\)"),
            (lambda: m(x.double()), r"float32 and float16 tensors only"),
            (lambda: m(('changeIndexes', x)), r"operand a is a tuple, but not"),
            (lambda: m(x), "HIP devices only")):
        with pytest.raises(Err, match=what):
            call()
    m.threshold = -1.0      # (read again in every frame)
    with pytest.raises(Err, match=r"threshold=-1.0 must be a number >= 0"):
        m(x)


def test_buffers_follow_the_module_and_keep_their_dtypes(pkg):
    src = nn.GroupNorm(2, 6)
    with torch.no_grad():
        src.weight.copy_(torch.arange(6.0) + 1)
        src.bias.copy_(-torch.arange(6.0))
    m = pkg.CBGroupNorm2d(src, 0.05, relu=True)
    with torch.no_grad():
        src.weight.zero_()      # (later edits of the source are not followed)
    assert m.gamma.tolist() == [1, 2, 3, 4, 5, 6] and m.beta[5] == -5 and m.eps == 1e-5
    assert (m.num_channels, m.num_groups, m.relu) == (6, 2, True)
    assert list(m.state_dict()) == ['gamma', 'beta', 'outputState', 'held', 'partials']
    assert m.held.dtype == torch.float32 and m.partials.dtype == torch.float64 and m.held.numel() == 0
    m.held = torch.arange(4.0).reshape(2, 2)
    m.partials = torch.ones(2, 6, 2, 1, dtype=torch.float64)
    m.outputState = torch.ones(1, 6, 2, 2)
    for conv, dt in ((lambda t: t.half(), torch.float16), (lambda t: t.double(), torch.float64),
                     (lambda t: t.to(torch.float16), torch.float16), (lambda t: t.to('meta'), torch.float32)):
        h = conv(copy.deepcopy(m))
        assert h.outputState.dtype == dt
        assert all(getattr(h, n).dtype == torch.float32 for n in ('gamma', 'beta', 'held'))
        assert h.partials.dtype == torch.float64
    h = copy.deepcopy(m).half().float()
    assert torch.equal(h.gamma, m.gamma) and torch.equal(h.held, m.held) and torch.equal(h.partials, m.partials)
    # a half-precision source converts exactly; an instance norm without an affine has no gamma / beta
    m16 = pkg.CBGroupNorm2d(nn.GroupNorm(3, 6).half(), 0.0)
    assert m16.gamma.dtype == torch.float32 and m16.beta.dtype == torch.float32
    inst = pkg.CBGroupNorm2d(nn.InstanceNorm2d(5), 0.0)
    assert inst.gamma is None and inst.beta is None and (inst.num_channels, inst.num_groups) == (5, 5)
    assert list(inst.state_dict()) == ['outputState', 'held', 'partials']
    aff = pkg.CBGroupNorm2d(nn.InstanceNorm2d(5, affine=True, eps=1e-3), 0.0)
    assert aff.gamma.numel() == 5 and aff.eps == 1e-3
    assert repr(m) == ("CBGroupNorm2d (GroupNorm, channels=6, groups=2, eps=1e-05, affine=True, relu=True, threshold=0.05, "
                       "propChgIdxs=False)")


def test_exports_state_helpers_pickle_and_deepcopy(pkg, lib):
    import cbinfer_amd
    import pycbinfer.groupnorm as alias
    from cbinfer_amd import batch, chain
    assert alias is cbinfer_amd.groupnorm and pkg.groupnorm is alias
    for name in ('CBGroupNorm2d', 'insertCBGroupNorm'):
        assert getattr(pkg, name) is getattr(alias, name) is getattr(cbinfer_amd, name)
    assert 'insertCBGroupNorm' in pkg.__all__ and 'CBGroupNorm2d' in pkg.__all__
    # the group norm is a row of each table; no tuple stands beside them
    assert pkg.CBGroupNorm2d in cbinfer_amd._STATEFUL and len(cbinfer_amd._STATEFUL) == 20
    assert not hasattr(cbinfer_amd, '_STATISTIC_STATE') and not hasattr(batch, 'STATISTIC_OPERATORS')
    assert [row for row in batch.CHAIN_OPERATORS if pkg.CBGroupNorm2d in row[0]] == [
        ((pkg.CBGroupNorm2d,), 'a change-based group norm', 'GroupNorm and InstanceNorm')]
    assert len(batch.CHAIN_OPERATORS) == 13
    assert len(chain.PRODUCERS) == 23 and len(chain.PASSES) == 11
    assert [row for row in chain.PRODUCERS if row[0] == 'CBGroupNorm2d'] == [
        ('CBGroupNorm2d', 'groupnorm', chain.ONLY, ())]
    assert not any(pkg.CBGroupNorm2d in chain.producers(p) for p in chain.PASSES)
    assert issubclass(pkg.CBGroupNorm2d, chain.CBStateModule)
    net = nn.Sequential(pkg.CBGroupNorm2d(nn.GroupNorm(2, 4), 0.03, relu=True), pkg.CBGroupNorm2d(nn.InstanceNorm2d(4), 0.0))
    a, b = net[0], net[1]
    a.propChangeIndexes, a.cloneOutput = True, False
    for m in (a, b):
        m.held = torch.arange(2.0 * m.num_groups).reshape(2, -1)
        m.partials = torch.ones(2, 4, 3, 1, dtype=torch.float64)
        m.outputState = torch.ones(1, 4, 3, 5)
        m.__dict__['_gnWork'] = {'key': None, 'tripped': torch.tensor([0, 1] * (m.num_groups // 2), dtype=torch.int32)}
    a._eps_arg()
    assert a.lastTrippedGroups() == [1] and b.lastTrippedGroups() == [1, 3]
    assert pkg.CBGroupNorm2d(nn.GroupNorm(2, 4), 0.0).lastTrippedGroups() == []
    states = pkg.getStateTensors(net)
    assert len(states) == 6
    for m in (a, b):
        assert all(any(t is s for s in states) for t in (m.outputState, m.held, m.partials))
    for clone in (pickle.loads(pickle.dumps(net)), copy.deepcopy(net)):
        ca, cb = clone[0], clone[1]
        assert type(ca) is pkg.CBGroupNorm2d and ca.propChangeIndexes and not ca.cloneOutput and ca.threshold == 0.03
        assert ca._gnWork is None and cb._gnWork is None and ca.__dict__['_epsArg'] is None
        assert torch.equal(ca.held, a.held) and torch.equal(ca.partials, a.partials) and torch.equal(ca.gamma, a.gamma)
        assert torch.equal(cb.outputState, b.outputState) and repr(ca) == repr(a) and cb.gamma is None
    pkg.clearMemory(net)
    for m in (a, b):
        assert m.outputState.numel() == 0 and m.held.numel() == 0 and m.partials.numel() == 0 and m._gnWork is None
        assert m.held.dtype == torch.float32 and m.partials.dtype == torch.float64
    assert a.gamma.numel() == 4      # (the affine is no state)


def test_insert_pass_wiring(pkg, lib):
    torch.manual_seed(1)
    seq = nn.Sequential()
    for name, mod in (('stem', nn.Conv2d(3, 8, 3, padding=1)), ('gn', nn.GroupNorm(2, 8)), ('act', nn.ReLU()),
                      ('mid', nn.Conv2d(8, 8, 1)), ('inorm', nn.InstanceNorm2d(8, affine=True)),
                      ('head', nn.Conv2d(8, 6, 3, padding=1)), ('tail', nn.GroupNorm(1, 6)), ('soft', nn.Softmax2d())):
        seq.add_module(name, mod)
    net = pkg.convert(seq.eval(), threshold=0.05)
    net.head.copyInput = False
    assert pkg.insertCBGroupNorm(net, 0.02, cloneOutput=False) is net
    # names preserved, the ReLU absorbed
    assert list(net._modules) == ['stem', 'gn', 'mid', 'inorm', 'head', 'tail', 'soft']
    assert names_of(net) == ['CBConv2d', 'CBGroupNorm2d', 'CBConv2d', 'CBGroupNorm2d', 'CBConv2d', 'CBGroupNorm2d',
                             'Softmax2d']
    assert net.gn.relu and not net.inorm.relu and not net.tail.relu
    assert (net.gn.num_groups, net.inorm.num_groups, net.tail.num_groups) == (2, 8, 1)
    assert net.inorm.gamma is not None and all(m.threshold == 0.02 for m in (net.gn, net.inorm, net.tail))
    # the producers hand on; the consumer rule: a 1x1 layer takes the changes, a k x k layer copies its input
    assert net.stem.propChangeIndexes and net.mid.propChangeIndexes and net.head.propChangeIndexes
    assert net.gn.propChangeIndexes and not net.inorm.propChangeIndexes and not net.tail.propChangeIndexes
    assert net.head.copyInput is True and not any(m.cloneOutput for m in (net.gn, net.inorm, net.tail))
    # what stays dense: a norm that follows no producer, a subclass, running statistics, beyond the limits -- and the
    # ReLU behind such a norm stays too
    seq = nn.Sequential(nn.GroupNorm(2, 8), nn.Conv2d(8, 8, 3, padding=1), MyGroupNorm(2, 8), nn.ReLU(),
                        nn.Conv2d(8, 8, 1), nn.InstanceNorm2d(8, track_running_stats=True), nn.ReLU(),
                        nn.Conv2d(8, 8, 1), nn.ReLU(), nn.GroupNorm(4, 8), nn.ReLU6()).eval()
    net = pkg.insertCBGroupNorm(pkg.convert(seq, threshold=0.05), 0.02)
    assert names_of(net) == ['GroupNorm', 'CBConv2d', 'MyGroupNorm', 'ReLU', 'CBConv2d', 'InstanceNorm2d', 'ReLU',
                             'CBConv2d', 'CBGroupNorm2d', 'ReLU6']
    # (convert merged the ReLU into the last convolution, so the norm behind it follows a producer; an nn.ReLU6 is no
    #  nn.ReLU and is not absorbed)
    assert not net[1].propChangeIndexes and not net[4].propChangeIndexes and net[7].propChangeIndexes
    assert not net[8].relu and net[8].cloneOutput is True
    # a subclass of nn.ReLU is not absorbed; an nn.Sequential inside a model is walked
    class MyReLU(nn.ReLU):
        pass
    inner = nn.Sequential(nn.Conv2d(3, 4, 3, padding=1), nn.GroupNorm(2, 4), MyReLU()).eval()
    outer = nn.ModuleDict({'body': pkg.convert(inner, threshold=0.0)})
    pkg.insertCBGroupNorm(outer, 0.0)
    assert names_of(outer['body']) == ['CBConv2d', 'CBGroupNorm2d', 'MyReLU'] and not outer['body'][1].relu
    assert outer['body'][1].cloneOutput is True
    with pytest.raises(lib.CBinferError, match=r"threshold=-1 must be a number >= 0"):
        pkg.insertCBGroupNorm(net, -1)


def test_batch_and_branch_group_refuse_by_name(pkg, lib):
    seq = nn.Sequential()
    for name, mod in (('stem', nn.Conv2d(3, 8, 3, padding=1)), ('gn', nn.GroupNorm(2, 8)), ('head', nn.Conv2d(8, 6, 1))):
        seq.add_module(name, mod)
    net = pkg.insertCBGroupNorm(pkg.convert(seq.eval(), threshold=0.0), 0.01)
    with pytest.raises(lib.CBinferError, match=r"SequenceBatch: layer 'gn' is CBGroupNorm2d .*a change-based group norm, "
                                                r"which has no batched kernel: run GroupNorm and InstanceNorm networks"):
        pkg.SequenceBatch(net, 2)
    with pytest.raises(lib.CBinferError, match=r"BranchGroup: layer '0.gn' is CBGroupNorm2d .*a change-based group norm, "
                                                r"which has no grouped launch"):
        pkg.BranchGroup([net])
