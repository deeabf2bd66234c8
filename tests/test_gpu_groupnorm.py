"""-m gpu tests of the change-based group norm (CBGroupNorm2d, insertCBGroupNorm; cb_groupnorm.hip).  The
specification is the numpy twin of tests/groupnorm_cases.py (rules 1-5 there).  The float64 partials are compared bit
for bit; the statistics within one unit of float32 (the device's float64 division and square root need not be correctly
rounded, and a float64 result that is off by a few of ITS units moves the float32 rounding by one unit at the most);
given the statistics the device wrote, `held`, the tripped set, the frame's mask and EVERY element of the state are
compared bit for bit.  At threshold 0 the state is compared with float64 math under groupnorm_cases.bound."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import groupnorm_cases as gn
from optest import (chain_frames, dev, free_pixel, host_words, lib, operand,      # noqa: F401  (fixtures)
                    gpu_pkg as pkg, raw)

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float16]
WORST = {}      # what -> worst figure seen
TH = 0.05       # the threshold of the frame tests
# (C, G, H, W): every case on every map, and one map with more units than launch 1 has workgroups (8 per CU) and more
# partials per group than launch 2 has lanes
SHAPES = [(Cn, G, H, W) for (Cn, G) in gn.CASES for (H, W) in gn.MAPS] + [(4, 2, 2100, 9)]


def tdt_of(dtype):
    return torch.float32 if dtype == np.float32 else torch.float16


def worst(key, value):
    WORST[key] = max(WORST.get(key, 0.0), float(value))


def module_for(pkg, Cn, G, aff, relu, threshold, rng):
    """(module on the device, gamma, beta): an nn.InstanceNorm2d for G == C, else an nn.GroupNorm."""
    src = nn.InstanceNorm2d(Cn, affine=aff, eps=gn.EPS) if G == Cn else nn.GroupNorm(G, Cn, eps=gn.EPS, affine=aff)
    gamma = beta = None
    if aff:
        gamma, beta = gn.affine(rng, Cn)
        with torch.no_grad():
            src.weight.copy_(torch.from_numpy(gamma))
            src.bias.copy_(torch.from_numpy(beta))
    return pkg.CBGroupNorm2d(src, threshold, relu=relu).cuda(), gamma, beta


def poisoned(a, listed, holding):
    """`a` with NaN in every segment that is clean, in the channels of the groups that hold: launch 1 reads no pixel of a
    clean segment, and launch 3 reads an unlisted pixel only in the channels of a tripped group."""
    Cn, H, W = a.shape
    clean = np.repeat(~gn.dirty_segments(listed), 64, axis=1)[:, :W]
    out = a.copy()
    out[holding] = np.where(clean[None], np.nan, a[holding]).astype(a.dtype)
    return out


def check_frame(m, a, P, held, prev, listed, fresh, got, where, G, gamma, beta):
    """Everything a frame leaves, against the twin.  Returns (partials, held, out, tripped)."""
    Cn, H, W = a.shape
    work = m._gnWork
    P = gn.segment_partials(a) if fresh else gn.update_partials(P, a, listed)
    Pdev = m.partials.cpu().numpy()
    assert Pdev.shape == P.shape and np.array_equal(Pdev.view(np.uint64), P.view(np.uint64)), where
    statsTwin, statsDev = gn.statistics(P, G, H, W), work['stats'].cpu().numpy()
    d = gn.ulps(statsDev, statsTwin)
    if d.max() > 0:
        print(where, "statistics: %d of %d differ from the twin, by %d units at the most" % ((d > 0).sum(), d.size, d.max()))
    worst('units of float32 between the device statistics and the twin', d.max())
    assert d.max() <= 1, (where, statsDev, statsTwin)
    new, tripped, out, mask, written = gn.step(a, statsDev, held, listed, m.threshold, fresh, G, gamma, beta, m.relu,
                                               prev=prev)
    assert gn.same_bits(m.held.cpu().numpy(), new), where
    assert np.array_equal(work['tripped'].cpu().numpy(), tripped.astype(np.int32)), where
    assert m.lastTrippedGroups() == list(np.flatnonzero(tripped)), where
    assert np.array_equal(host_words(work['copy']), gn.pack(mask)), where
    assert int(work['bits'].ne(0).sum().item()) == 0, where
    state = m.outputState[0].cpu().numpy()
    bad = ~((gn.bits_of(state) == gn.bits_of(out)) | (np.isnan(state) & np.isnan(out)))
    assert not bad.any(), (where, int(bad.sum()), np.argwhere(bad)[:4], state[bad][:4], out[bad][:4])
    if got is not None:
        assert torch.equal(raw(got), raw(m.outputState)), where
    return P, new, out, tripped


@pytest.mark.parametrize("form", gn.FORMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
def test_frames_equal_the_twin_bit_for_bit(pkg, dtype, form):
    """Every shape, the five frames of groupnorm_cases.frame_script on ONE module: fresh; a sparse change; an empty
    frame; a drift under the threshold; a frame in which exactly the last group trips.  First the TWIN's own trip
    sequence is asserted on the CPU -- all, none, none, none, the last --, so that no case passes by never holding or
    never tripping.  Before every frame the clean segments of the input are overwritten with NaN in the channels of the
    groups that hold: the state shows none of them."""
    for i, (Cn, G, H, W) in enumerate(SHAPES):
        rng = np.random.default_rng(100 * Cn + W)
        frames = gn.frame_script(rng, Cn, G, H, W, dtype, TH)
        # the twin alone, on the CPU
        heldT, PT, seq = np.zeros((2, G), np.float32), None, []
        for t, (label, a, S) in enumerate(frames):
            listed = np.ones((H, W), dtype=bool) if form == "all" else S
            PT = gn.segment_partials(a) if t == 0 else gn.update_partials(PT, a, listed)
            heldT, trippedT = gn.rule(gn.statistics(PT, G, H, W), heldT, TH, t == 0)
            seq.append(list(np.flatnonzero(trippedT)))
        assert seq == [list(range(G)), [], [], [], [G - 1]], (Cn, G, H, W, seq)
        # the device
        aff, relu = [(True, True), (True, False), (False, False), (False, True)][i % 4]
        m, gamma, beta = module_for(pkg, Cn, G, aff, relu, TH, rng)
        m.propChangeIndexes = True
        held, P, prev = np.zeros((2, G), np.float32), None, None
        for t, (label, a, S) in enumerate(frames):
            where = ((Cn, G, H, W), np.dtype(dtype).name, form, label)
            listed = np.ones((H, W), dtype=bool) if form == "all" else S
            holding = np.repeat(~np.isin(np.arange(G), seq[t]), Cn // G)
            x = dev(poisoned(a, listed, holding) if t and form != "all" else a).reshape(1, Cn, H, W)
            out = m(operand(form, x, S, free_pixel(S) or 0, bool(t % 2)))
            assert type(out) is tuple and out[0] == 'changeIndexes' and out[1].dtype == tdt_of(dtype), where
            assert out[2].size == (H, W) and out[2]._mask is m._gnWork['copy'], where
            P, held, prev, tripped = check_frame(m, a, P, held, prev, listed, t == 0, out[1], where, G, gamma, beta)
            assert list(np.flatnonzero(tripped)) == seq[t], where
            assert not np.isnan(prev).any(), where
            n = int(np.unpackbits(host_words(m._gnWork['copy']).view(np.uint8)).sum())
            assert n == (H * W if seq[t] or form == "all" else int(S.sum())), where
        assert m.partials.dtype == torch.float64 and m.held.dtype == torch.float32


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
def test_threshold_zero_against_float64(pkg, dtype):
    """threshold = 0, three frames in mask form -- fresh, two sparse changes --: the state is within
    groupnorm_cases.bound of F.group_norm (+ ReLU) in float64 on the CPU, on the stored operand, at every element."""
    rng = np.random.default_rng(11)
    for i, (Cn, G, H, W) in enumerate(SHAPES):
        aff, relu = [(True, True), (True, False), (False, False), (False, True)][(i + 1) % 4]
        m, gamma, beta = module_for(pkg, Cn, G, aff, relu, 0.0, rng)
        a = (rng.standard_normal((Cn, H, W)) * 2 + rng.uniform(-3, 3, Cn)[:, None, None]).astype(dtype)
        for t in range(3):
            S = rng.random((H, W)) < 0.1
            if t:
                a[:, S] = (rng.standard_normal((Cn, int(S.sum()))) * 2).astype(dtype)
            m(operand("mask", dev(a).reshape(1, Cn, H, W), S, free_pixel(S) or 0, bool(t % 2)))
            want = reference(a, G, gamma, beta, relu)
            got = m.outputState[0].cpu().numpy().astype(np.float64)
            err, bound = np.abs(got - want), gn.bound(a, G, gn.EPS, gamma, beta, relu)
            assert (err <= bound).all(), ((Cn, G, H, W), t, float((err / bound).max()))
            worst(('threshold 0: err / bound', np.dtype(dtype).name), (err / bound).max())
            assert gn.same_bits(m.held.cpu().numpy(), m._gnWork['stats'].cpu().numpy())      # (held IS the statistics)


def reference(a, G, gamma, beta, relu):
    """F.group_norm (+ ReLU) in float64 on the CPU."""
    x = torch.from_numpy(a.astype(np.float64))[None]
    w = torch.from_numpy(gamma.astype(np.float64)) if gamma is not None else None
    b = torch.from_numpy(beta.astype(np.float64)) if beta is not None else None
    y = F.group_norm(x, G, w, b, gn.EPS)
    return (F.relu(y) if relu else y)[0].numpy()


def test_large_mean_holds_the_same_bound(pkg):
    """Values 1000 + N(0, 1) in float32, two frames at threshold 0: the same bound holds.  The twin with its statistics
    taken in float32 breaks it on the same data (shown on the CPU): that is what the float64 level is for."""
    rng = np.random.default_rng(13)
    for (Cn, G, H, W) in SHAPES:
        m, gamma, beta = module_for(pkg, Cn, G, True, False, 0.0, rng)
        a = (1000.0 + rng.standard_normal((Cn, H, W))).astype(np.float32)
        for t in range(2):
            S = rng.random((H, W)) < 0.1
            if t:
                a[:, S] = (1000.0 + rng.standard_normal((Cn, int(S.sum())))).astype(np.float32)
            m(operand("mask", dev(a).reshape(1, Cn, H, W), S, free_pixel(S) or 0, bool(t % 2)))
            want = reference(a, G, gamma, beta, False)
            bound = gn.bound(a, G, gn.EPS, gamma, beta, False)
            err = np.abs(m.outputState[0].cpu().numpy().astype(np.float64) - want)
            assert (err <= bound).all(), ((Cn, G, H, W), t, float((err / bound).max()))
            worst('large mean: err / bound', (err / bound).max())
        poor = gn.step(a, gn.statistics_f32(a, G), np.zeros((2, G), np.float32), None, 0.0, True, G, gamma, beta)[2]
        ratio = float((np.abs(poor - want) / bound).max())
        assert ratio > 1.0, ((Cn, G, H, W), ratio)
        worst('large mean, statistics in float32 (twin, CPU): err / bound', ratio)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
def test_holding_keeps_unlisted_elements_and_stays_within_the_threshold(pkg, dtype):
    """threshold 0.05 and three frames that each move every group's mean by 0.2 threshold standard deviations: no group
    trips; every element at an unlisted pixel keeps its bits; the state is within threshold (1 + |y|) |gamma| plus the
    bound of the dense result of float64 math on the frame's operand."""
    for i, (Cn, G, H, W) in enumerate(SHAPES[:12]):
        rng = np.random.default_rng(17 + i)
        m, gamma, beta = module_for(pkg, Cn, G, True, bool(i % 2), TH, rng)
        Cg = Cn // G
        a = (rng.standard_normal((Cn, H, W)) + rng.uniform(-1, 1, Cn)[:, None, None]).astype(dtype)
        std = a.astype(np.float64).reshape(G, -1).std(axis=1)
        m(dev(a).reshape(1, Cn, H, W))
        assert m.lastTrippedGroups() == list(range(G))
        for t in range(1, 4):
            S = rng.random((H, W)) < 0.1
            S[int(rng.integers(H)), int(rng.integers(W))] = True
            delta = np.repeat(0.2 * TH * std * (H * W) / S.sum(), Cg)
            a[:, S] = (a[:, S].astype(np.float64) + delta[:, None]).astype(dtype)
            before = m.outputState[0].cpu().numpy().copy()
            m(operand("mask", dev(a).reshape(1, Cn, H, W), S, free_pixel(S) or 0, bool(t % 2)))
            where = ((Cn, G, H, W), np.dtype(dtype).name, t)
            assert m.lastTrippedGroups() == [], where
            after = m.outputState[0].cpu().numpy()
            assert np.array_equal(gn.bits_of(after)[:, ~S], gn.bits_of(before)[:, ~S]), where
            assert np.array_equal(host_words(m._gnWork['copy']), gn.pack(S)), where
            want, y, _, _ = gn.reference64(a, G, gn.EPS, gamma, beta, m.relu)
            tol = TH * (1 + np.abs(y)) * np.abs(gamma.astype(np.float64))[:, None, None] + \
                gn.bound(a, G, gn.EPS, gamma, beta, m.relu)
            err = np.abs(after.astype(np.float64) - want)
            assert (err <= tol).all(), (where, float((err / tol).max()))
            worst(('holding: err / (threshold term + bound)', np.dtype(dtype).name), (err / tol).max())


# ------------------------------------------------------------------------------------------------ in a chain
def make_chain(pkg, kind, tdt, threshold, cloneOutput):
    """'gn': 3x3 CBConv2d -> GroupNorm(2, 8) -> ReLU (absorbed) -> 1x1 CBConv2d;  'in': 3x3 CBConv2d -> InstanceNorm2d(8)
    -> 3x3 CBConv2d; 12 x 70 maps, conv thresholds 0.  Returns (net, the dense head on the CPU in float64)."""
    torch.manual_seed(71)
    src = nn.Sequential()
    if kind == 'gn':
        mods = (('stem', nn.Conv2d(4, 8, 3, padding=1)), ('norm', nn.GroupNorm(2, 8)), ('act', nn.ReLU()),
                ('head', nn.Conv2d(8, 6, 1)))
    else:
        mods = (('stem', nn.Conv2d(4, 8, 3, padding=1)), ('norm', nn.InstanceNorm2d(8, affine=True)),
                ('head', nn.Conv2d(8, 6, 3, padding=1)))
    for name, mod in mods:
        src.add_module(name, mod)
    with torch.no_grad():
        src.norm.weight.copy_(torch.linspace(0.5, 2.0, 8) * torch.tensor([1, -1] * 4))
        src.norm.bias.copy_(torch.linspace(-1.0, 1.0, 8))
    src = src.eval().cuda().to(tdt)
    head64 = copy.deepcopy(src.head).cpu().double()
    net = pkg.convert(src, threshold=0.0)
    pkg.insertCBGroupNorm(net, threshold, cloneOutput=cloneOutput)
    assert [type(m).__name__ for m in net] == ['CBConv2d', 'CBGroupNorm2d', 'CBConv2d']
    assert list(net._modules) == ['stem', 'norm', 'head'] and net.norm.relu == (kind == 'gn')
    assert net.stem.propChangeIndexes and net.norm.propChangeIndexes == (kind == 'gn')
    assert net.norm.cloneOutput == cloneOutput and (kind == 'gn' or net.head.copyInput)
    for m in (net.stem, net.head):
        m.cloneOutput = cloneOutput
    if tdt == torch.float32:
        net.stem.exactF32 = net.head.exactF32 = True
    return net, head64


@pytest.mark.parametrize("kind", ["gn", "in"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
def test_chain_at_threshold_zero_is_the_dense_network(pkg, dtype, kind):
    """threshold = 0, five frames of moving blocks.  The norm's state is within groupnorm_cases.bound of F.group_norm
    (+ ReLU) in float64 on the very conv output it was fed; the network's output is within a bound of the dense head in
    float64 on that: the norm's bound entering through |W|, K + 2 float32 roundings of the contraction relative to
    sum |w| |x| (K the taps), and the rounding to the dtype."""
    net, head64 = make_chain(pkg, kind, tdt_of(dtype), 0.0, True)
    norm = net.norm
    gamma, beta = norm.gamma.cpu().numpy(), norm.beta.cpu().numpy()
    u, ut = 2.0 ** -24, (2.0 ** -24 if dtype == np.float32 else 2.0 ** -11)
    Wabs = head64.weight.detach().abs()
    pad = head64.padding
    K = int(head64.weight[0].numel())
    with torch.no_grad():
        for t, f in enumerate(chain_frames(np.random.default_rng(73), 5, dtype, H=12, C=4)):
            y = net(f)
            x = net.stem.prevOutput[0].cpu().numpy()
            want = reference(x, norm.num_groups, gamma, beta, norm.relu)
            bound = gn.bound(x, norm.num_groups, norm.eps, gamma, beta, norm.relu)
            got = norm.outputState[0].cpu().numpy()
            err = np.abs(got.astype(np.float64) - want)
            assert (err <= bound).all(), (t, float((err / bound).max()))
            worst(('chain %s: norm err / bound' % kind, np.dtype(dtype).name), (err / bound).max())
            want_t = torch.from_numpy(want)[None]
            ref = head64(want_t)[0].numpy()
            ybound = (F.conv2d(torch.from_numpy(bound)[None], Wabs, padding=pad)[0].numpy() +
                      (K + 2) * u * (F.conv2d(want_t.abs(), Wabs, padding=pad)[0].numpy() +
                                     head64.bias.detach().abs().numpy()[:, None, None]) +
                      ut * np.abs(ref) + 2.0 ** -24)
            yerr = np.abs(y[0].cpu().numpy().astype(np.float64) - ref)
            assert (yerr <= ybound).all(), (t, float((yerr / ybound).max()))
            worst(('chain %s: output err / bound' % kind, np.dtype(dtype).name), (yerr / ybound).max())


@pytest.mark.parametrize("kind", ["gn", "in"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
def test_chain_records_as_a_launch_program(pkg, lib, dtype, kind):
    """With cloneOutput=False the network is library calls only: FrameProgram records it -- the norm is ONE
    cbinfer_cbgroupnorm_forward --, four replayed frames equal the eager network in outputs and in every state, held and
    partials included, bit for bit."""
    net, _ = make_chain(pkg, kind, tdt_of(dtype), 0.01, False)
    frames = chain_frames(np.random.default_rng(79), 8, dtype, H=12, C=4)
    with torch.no_grad():
        for f in frames[:4]:
            net(f)
        eager = copy.deepcopy(net)
        prog = pkg.FrameProgram(net)
        for t, f in enumerate(frames[4:]):
            yp, ye = prog(f), eager(f)
            assert torch.equal(raw(yp), raw(ye)), t
            sa, sb = pkg.getStateTensors(net), pkg.getStateTensors(eager)
            assert len(sa) == len(sb) == 2 * 2 + 3      # two convs; the state, held and the partials
            for ta, tb in zip(sa, sb):
                assert ta.dtype == tb.dtype and torch.equal(ta, tb), t
        raws = [fn for fn, _ in prog.calls]
        assert raws.count(lib.C.cbinfer_cbgroupnorm_forward.raw) == 1
        assert any(t is net.norm.partials for t in pkg.getStateTensors(net))


def test_batch_and_branch_group_refuse_the_network(pkg, lib):
    net, _ = make_chain(pkg, 'gn', torch.float32, 0.01, True)
    with pytest.raises(lib.CBinferError, match=r"SequenceBatch: layer 'norm' is CBGroupNorm2d .*a change-based group norm"):
        pkg.SequenceBatch(net, 2)
    with pytest.raises(lib.CBinferError, match=r"BranchGroup: layer '0.norm' is CBGroupNorm2d .*a change-based group norm"):
        pkg.BranchGroup([net])


def test_worst_figures_are_reported():
    """The worst figures over the tests above: measurements, not bars (the bars are 1)."""
    for key, rel in sorted(WORST.items(), key=str):
        print("%-72s %.3g" % (key, rel))
    assert WORST
