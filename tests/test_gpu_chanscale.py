"""-m gpu tests of the change-based channel attention scale (CBChannelScale2d, CBSqueezeExcite; cb_chanscale.hip,
DESIGN.md 5.28).  The specification is the numpy twin of tests/chanscale_cases.py (rules 1-4 there).  Given the gate
vector the device wrote, `held`, the tripped words, their count, the frame's mask and EVERY element of the state are
compared bit for bit; the gate vector itself is compared with float64 math under the bounds derived in
chanscale_cases.gate_bound / excite_bound, and bit for bit where no expf is involved."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn

import chanscale_cases as cs
from optest import dev, free_pixel, host_words, lib, operand, gpu_pkg as pkg, raw      # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float16]
WORST = {}      # what -> worst err / bound seen against float64
TH = 0.25       # the threshold of the frame tests: exact in float32, as are the gates built around it


def pixel_patterns(rng, H, W):
    return dict(cs.pc.patterns(rng, H, W))


def frame_script(rng, Cn, H, W):
    """(label, listed bool [H, W], how the frame's vector is made from (held, previous vector)) of consecutive frames.
    The vectors are built for gate=None, where gate == v: numbers that float32 and float16 hold exactly."""
    P = pixel_patterns(rng, H, W)
    Z = P["empty"]
    keep = lambda held, v: v.copy()

    def bump(chans, by):
        def make(held, v):
            v = held.copy()      # (back onto the held values: exactly one set of channels moves)
            v[list(chans)] += np.float32(by)
            return v
        return make
    script = [("fresh", Z, keep), ("nothing", Z, keep)]
    script += [("pixels: " + k, P[k], keep) for k in ("one bit", "last column", "word boundary", "random")]
    for c in sorted(set(c for c in (0, 63, 64, Cn - 1) if c < Cn)):
        script.append(("channel %d" % c, Z, bump([c], 0.5)))
    script.append(("pixels and channels", P["random"], bump(range(0, Cn, 3), -0.5)))
    script.append(("every channel", P["one bit"], bump(range(Cn), 1.0)))
    script.append(("at held + threshold", Z, bump(range(0, Cn, 2), TH)))
    script.append(("at held - threshold", P["last column"], bump(range(Cn), -TH)))
    for k in (1, 2, 3):      # 0.375 TH per frame (0.4 TH is not a float16 number): holds twice, trips in the third
        script.append(("drift %d" % k, Z, bump(range(Cn), 0.375 * TH * k)))
    script.append(("NaN", P["one bit"], bump([Cn // 2], np.nan)))
    script.append(("after the NaN", Z, keep))
    return script


def check_frame(m, a_host, v_host, held, prev, listed, fresh, got, where, gate=None):
    """Everything a frame leaves, against the twin given the device's gate vector.  Returns (held, out, tripped)."""
    work = m._csWork
    gateDev = work['gate'].cpu().numpy()
    new, tripped, out, mask, written = cs.step(a_host, gateDev, held, listed, m.threshold, fresh, prev=prev)
    assert cs.same_bits(m.held.cpu().numpy(), new), where
    assert np.array_equal(host_words(work['tripped']), cs.tripped_words(tripped)), where
    assert m.lastTrippedChannels() == int(tripped.sum()), where
    assert np.array_equal(host_words(work['copy']), cs.pack(mask)), where
    assert int(work['bits'].ne(0).sum().item()) == 0, where
    state = m.outputState[0].cpu().numpy()
    bad = ~((cs.bits_of(state) == cs.bits_of(out)) | (np.isnan(state) & np.isnan(out)))
    assert not bad.any(), (where, int(bad.sum()), np.argwhere(bad)[:4], state[bad][:4], out[bad][:4])
    if got is not None:
        assert torch.equal(raw(got), raw(m.outputState)), where
    return new, out, tripped


@pytest.mark.parametrize("form", cs.FORMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
def test_frames_equal_the_twin_bit_for_bit(pkg, dtype, form):
    """Every shape, the frames of frame_script on ONE module with gate=None (gate == v, so the script places every
    gate exactly): fresh state; nothing changed (state, held keep every bit, empty mask, count 0); pixels only; one
    tripped channel -- 0, 63, 64, C - 1 -- with a full mask and only those planes written; pixels and channels; every
    channel; gates exactly at held +- threshold (not tripped: the comparison is strict); a drift that holds twice and
    trips in the third frame; a NaN.  Before every frame `a` is overwritten at one pixel that is NOT listed: the state
    must show the new value in the tripped channels and the old one in every other."""
    rng = np.random.default_rng(31)
    tdt = torch.float32 if dtype == np.float32 else torch.float16
    for shape in cs.SHAPES:
        Cn, H, W = shape
        m = pkg.CBChannelScale2d(TH, gate=None)
        m.propChangeIndexes = True
        a = cs.pc.values(rng, shape, dtype, span=4.0)
        v = (rng.integers(-8, 9, Cn) * 0.5).astype(dtype)
        held, prev = np.zeros(Cn, np.float32), None
        seen = dict(empty=0, full=0, partial=0, held_written=0)
        for t, (label, S, make) in enumerate(frame_script(rng, Cn, H, W)):
            where = (shape, np.dtype(dtype).name, form, label)
            if t:
                vf = make(held, v.astype(np.float32))
                v = vf.astype(dtype)
                assert np.array_equal(v.astype(np.float32), vf, equal_nan=True), where      # (the dtype holds it exactly)
                fresh_vals = cs.pc.values(rng, shape, dtype, span=4.0)
                a[:, S] = fresh_vals[:, S]
                free = np.flatnonzero(~S.reshape(-1))
                if len(free) and form != "all":      # an operand altered where the list does not say so
                    p = int(free[len(free) // 2])
                    a[:, p // W, p % W] = fresh_vals[:, p // W, p % W]
            listed = np.ones((H, W), dtype=bool) if form == "all" else S
            out = m(operand(form, dev(a).reshape(1, Cn, H, W), S, free_pixel(S) or 0, bool(t % 2)), dev(v).reshape(1, Cn, 1, 1))
            assert type(out) is tuple and out[0] == 'changeIndexes' and out[1].dtype == tdt, where
            assert out[2].size == (H, W) and out[2]._mask is m._csWork['copy'], where
            held, prev, tripped = check_frame(m, a, v, held, prev, listed, t == 0, out[1], where)
            if label == "nothing" or label.startswith("at held") or label in ("drift 1", "drift 2", "after the NaN"):
                assert not tripped.any() or label == "after the NaN", where
            if label in ("every channel", "drift 3", "fresh"):
                assert tripped.all(), where
            if label.startswith("channel "):
                assert list(np.flatnonzero(tripped)) == [int(label.split()[1])], where
            if label == "NaN":
                assert list(np.flatnonzero(tripped)) == [Cn // 2] and np.isnan(prev[Cn // 2]).all(), where
            if label == "after the NaN":      # (a NaN gate differs from itself: it trips in every frame)
                assert list(np.flatnonzero(tripped)) == [Cn // 2], where
            n = int(np.unpackbits(host_words(m._csWork['copy']).view(np.uint8)).sum())
            seen['empty' if n == 0 else 'full' if n == H * W else 'partial'] += 1
        assert seen['full'] >= 6 and (form == "all" or (seen['empty'] >= 4 and (H * W < 3 or seen['partial'] >= 2))), seen


@pytest.mark.parametrize("gate", ['sigmoid', 'hardsigmoid'])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
def test_gates_against_float64_and_frames_with_a_gate(pkg, dtype, gate):
    """The plain form with a gate: the device's gate vector against float64 g(v) under gate_bound (the hard sigmoid is
    the twin's bit for bit), and three frames -- fresh, a small move of every v (below the threshold behind the gate:
    nothing trips), a large move of some -- checked as above in mask form."""
    rng = np.random.default_rng(37)
    for shape in cs.SHAPES:
        Cn, H, W = shape
        m = pkg.CBChannelScale2d(0.02, gate=gate)
        a = cs.pc.values(rng, shape, dtype, span=4.0)
        v0 = rng.uniform(-6, 6, Cn).astype(dtype)
        big = v0.copy()
        big[::2] = -big[::2] + dtype(1.0)
        held, prev = np.zeros(Cn, np.float32), None
        for t, v in enumerate((v0, (v0.astype(np.float32) * 1.001).astype(dtype), big)):
            S = rng.random((H, W)) < 0.1
            a[:, S] = cs.pc.values(rng, shape, dtype, span=4.0)[:, S]
            m(operand("mask", dev(a).reshape(1, Cn, H, W), S, free_pixel(S) or 0, bool(t % 2)), dev(v).reshape(1, Cn, 1, 1))
            where = (shape, np.dtype(dtype).name, gate, t)
            g = m._csWork['gate'].cpu().numpy()
            ref = cs.gate64(v.astype(np.float32), gate)
            err, bound = np.abs(g - ref), cs.gate_bound(ref, gate)
            if gate == 'hardsigmoid':
                assert cs.same_bits(g, cs.gate_fn(v.astype(np.float32), gate)), where
            else:
                assert (err <= bound).all(), (where, float((err / bound).max()))
                WORST[(gate, 'gate')] = max(WORST.get((gate, 'gate'), 0.0), float((err / bound).max()))
            held, prev, tripped = check_frame(m, a, v, held, prev, S, t == 0, None, where, gate)
            assert tripped.all() if t == 0 else (not tripped.any() if t == 1 else tripped.any()), where


@pytest.mark.parametrize("act", cs.ACTS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
def test_fused_excitation_against_the_twin_and_float64(pkg, dtype, act):
    """The excitation in launch 1, gate=None so that the gate vector IS s: C in {3, 65, 300} with R in {1, 16, 17, 40},
    with and without biases, nn.Conv2d and nn.Linear.  With the ReLU no expf is involved: s has the twin's bits, i.e.
    the order of sum16.  Either way s is within excite_bound of float64 on the stored operands.  Two frames through
    check_frame: the state is the product with `held` at every element."""
    rng = np.random.default_rng(41)
    tdt = torch.float32 if dtype == np.float32 else torch.float16
    for (Cn, R) in cs.EXCITE:
        for bias in (True, False):
            W1, b1, W2, b2 = cs.operands(rng, Cn, R, bias)
            if (Cn + R) % 2:
                fc1, fc2 = nn.Linear(Cn, R, bias=bias), nn.Linear(R, Cn, bias=bias)
            else:
                fc1, fc2 = nn.Conv2d(Cn, R, 1, bias=bias), nn.Conv2d(R, Cn, 1, bias=bias)
            with torch.no_grad():
                fc1.weight.copy_(torch.from_numpy(W1).reshape(fc1.weight.shape))
                fc2.weight.copy_(torch.from_numpy(W2).reshape(fc2.weight.shape))
                if bias:
                    fc1.bias.copy_(torch.from_numpy(b1))
                    fc2.bias.copy_(torch.from_numpy(b2))
            m = pkg.CBChannelScale2d(0.05, gate=None, fc1=fc1, fc2=fc2, act=nn.ReLU() if act == 'relu' else nn.SiLU())
            m = m.cuda().to(tdt)
            assert m.w1.dtype == torch.float32 and m.w1.is_cuda
            H, W = 3, 70
            a = cs.pc.values(rng, (Cn, H, W), dtype, span=4.0)
            held, prev = np.zeros(Cn, np.float32), None
            z = rng.uniform(-2, 2, Cn).astype(dtype)
            for t in range(2):
                if t:
                    z = (z.astype(np.float32) + rng.uniform(-0.05, 0.05, Cn).astype(np.float32)).astype(dtype)
                S = rng.random((H, W)) < 0.1
                m(operand("mask", dev(a).reshape(1, Cn, H, W), S, free_pixel(S) or 0, bool(t % 2)), dev(z).reshape(1, Cn, 1, 1))
                where = (Cn, R, bias, np.dtype(dtype).name, act, t)
                s = m._csWork['gate'].cpu().numpy()
                if act == 'relu':
                    assert cs.same_bits(s, cs.excite(z, W1, b1, W2, b2, act)), where
                ref, _, _ = cs.excite64(z, W1, b1, W2, b2, act)
                err, bound = np.abs(s - ref), cs.excite_bound(z, W1, b1, W2, b2, act)
                assert (err <= bound).all(), (where, float((err / bound).max()))
                WORST[(act, 's')] = max(WORST.get((act, 's'), 0.0), float((err / bound).max()))
                held, prev, tripped = check_frame(m, a, z, held, prev, S, t == 0, None, where)


# ------------------------------------------------------------------------------------------------ an SE block in a chain
class SE(nn.Module):
    def __init__(self, C, R):
        super(SE, self).__init__()
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.fc1, self.fc2 = nn.Conv2d(C, R, 1), nn.Conv2d(R, C, 1)
        self.activation, self.scale_activation = nn.ReLU(), nn.Sigmoid()

    def forward(self, x):
        return x * self.scale_activation(self.fc2(self.activation(self.fc1(self.avgpool(x)))))


TV = ('fc1', 'fc2', 'activation', 'scale_activation')


def make_block(pkg, tdt, threshold, cloneOutput):
    """3x3 CBConv2d -> SE block (8 channels, R 2) -> 1x1 CBConv2d on 12 x 70 maps, conv thresholds 0."""
    torch.manual_seed(53)
    src = nn.Sequential()
    for name, mod in (('stem', nn.Conv2d(4, 8, 3, padding=1)), ('se', SE(8, 2)), ('head', nn.Conv2d(8, 6, 1))):
        src.add_module(name, mod)
    src = src.eval().cuda().to(tdt)
    with torch.no_grad():
        src.se.fc2.weight.mul_(4.0)      # (gates away from 1/2)
    dense = copy.deepcopy(src.se)
    net = pkg.convert(src, threshold=0.0)
    pkg.insertCBSqueezeExcite(net, {SE: TV}, threshold, cloneOutput=cloneOutput)
    assert [type(m).__name__ for m in net] == ['CBConv2d', 'CBSqueezeExcite', 'CBConv2d']
    assert net.stem.propChangeIndexes and net.se.propChangeIndexes and net.se.cloneOutput == cloneOutput
    for m in (net.stem, net.head):
        m.cloneOutput = cloneOutput
    if tdt == torch.float32:
        net.stem.exactF32 = net.head.exactF32 = True
    return net, dense


def block_frames(rng, n, npdt, H=12, W=70):
    """n frames [1, 4, H, W]; a frame differs from the one before in two moved blocks only."""
    base = (rng.random((1, 4, H, W)) * 2 - 1).astype(npdt)
    frames = []
    for i in range(n):
        new = base.copy()
        if i:
            for _ in range(2):
                y0, x0 = int(rng.integers(0, H)), int(rng.integers(0, W))
                blk = new[:, :, y0:y0 + 4, x0:x0 + 7]
                blk[...] = (rng.random(blk.shape) * 2 - 1).astype(npdt)
        frames.append(dev(new))
        base = new
    return frames


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
def test_block_at_threshold_zero_is_the_dense_block(pkg, dtype):
    """threshold = 0: the block's state equals x * sigmoid(fc2(relu(fc1(mean(x))))) in float64 on the very conv outputs
    the block was fed, within: the pool's mean (one rounding to the dtype behind a float32 sum), the fused s
    (excite_bound on the pool's stored state), the sigmoid's 14 units with s's error entering at a slope of at most
    1/4, one product and one rounding to the dtype."""
    net, dense = make_block(pkg, torch.float32 if dtype == np.float32 else torch.float16, 0.0, True)
    sc = net.se.scale
    dense32 = dense.float()
    W1, b1, W2, b2 = (t.cpu().numpy() for t in (sc.w1, sc.b1, sc.w2, sc.b2))
    u, ut = 2.0 ** -24, (2.0 ** -24 if dtype == np.float32 else 2.0 ** -11)
    with torch.no_grad():
        for t, f in enumerate(block_frames(np.random.default_rng(59), 5, dtype)):
            net(f)
            x = net.stem.prevOutput[0].cpu().numpy()
            z = net.se.pool.outputState.reshape(-1).cpu().numpy()
            x64 = x.astype(np.float64)
            mean = x64.mean(axis=(1, 2))
            # (the pool: a float32 sum of H W values in some order, a division, one rounding to the dtype)
            pb = (12 * 70 + 2) * u * np.abs(x64).mean(axis=(1, 2)) + ut * np.abs(mean)
            assert (np.abs(z - mean) <= pb).all(), t
            s64, _, _ = cs.excite64(z, W1, b1, W2, b2, 'relu')
            g64 = cs.gate64(s64, 'sigmoid')
            gbound = 14 * u * g64 + 0.25 * cs.excite_bound(z, W1, b1, W2, b2, 'relu')
            g = sc._csWork['gate'].cpu().numpy()
            assert (np.abs(g - g64) <= gbound).all(), t
            assert cs.same_bits(sc.held.cpu().numpy(), g), t      # (threshold 0: held is the gate)
            ref = x64 * g64[:, None, None]
            bound = np.abs(x64) * gbound[:, None, None] + (u + ut) * np.abs(ref) + 2.0 ** -24
            got = sc.outputState[0].cpu().numpy().astype(np.float64)
            assert (np.abs(got - ref) <= bound).all(), (t, float((np.abs(got - ref) / bound).max()))
            WORST[('block', np.dtype(dtype).name)] = max(WORST.get(('block', np.dtype(dtype).name), 0.0),
                                                         float((np.abs(got - ref) / bound).max()))
            # ... and against torch's own dense block -- pool, two 1x1 convolutions, ReLU, sigmoid, product, in float32
            # -- fed the same conv output.  It pools for itself: the pool's error pb enters s through |W2| |W1| and
            # the gate at a slope of at most 1/4; torch's own float32 evaluation is granted the bounds once more.
            want = dense32(torch.from_numpy(x.astype(np.float32)).cuda()[None])[0].cpu().numpy().astype(np.float64)
            gboth = 2 * gbound + 0.25 * (np.abs(W2) @ (np.abs(W1) @ pb)).astype(np.float64)
            tol = np.abs(x64) * gboth[:, None, None] + 2 * (u + ut) * np.abs(ref) + 2.0 ** -24
            assert (np.abs(got - want) <= tol).all(), (t, float((np.abs(got - want) / tol).max()))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
def test_block_holds_its_gates_within_the_threshold(pkg, dtype):
    """threshold = 0.02 over eight frames: |held - gate| <= threshold after every frame, lastTrippedChannels() and the
    state match the twin, the mask handed to the 1x1 layer is the stem's changes unless a channel tripped, and some
    frame trips nothing (that is the point)."""
    net, _ = make_block(pkg, torch.float32 if dtype == np.float32 else torch.float16, 0.02, True)
    sc = net.se.scale
    held, prev, counts, handed = np.zeros(8, np.float32), None, [], {}
    # (the changes the stem hands the block, read as the exact list: synchronises, in a test only)
    net.se.register_forward_pre_hook(lambda mod, args: handed.__setitem__('idx', args[0][2].tensor().cpu().numpy()))
    with torch.no_grad():
        for t, f in enumerate(block_frames(np.random.default_rng(61), 8, dtype)):
            net(f)
            x = net.stem.prevOutput[0].cpu().numpy()
            g = sc._csWork['gate'].cpu().numpy()
            h = sc.held.cpu().numpy()
            assert (np.abs(h - g) <= np.float32(0.02)).all(), t
            n = int(np.unpackbits(host_words(sc._csWork['copy']).view(np.uint8)).sum())
            listed = np.zeros(12 * 70, bool)
            listed[handed['idx']] = True
            listed = listed.reshape(12, 70)
            assert t == 0 or 0 < listed.sum() < 12 * 70, t
            held, prev, tripped = check_frame(sc, x, None, held, prev, listed, t == 0, None, (np.dtype(dtype).name, t))
            counts.append(int(tripped.sum()))
            assert (n == 12 * 70) == bool(tripped.any()), t
    print("tripped channels per frame:", counts)
    # (the gates of this block move by less than the threshold from frame to frame: behind the fresh frame the block
    #  holds them -- that is the point; the tripped paths are test_frames_equal_the_twin_bit_for_bit's)
    assert counts[0] == 8 and min(counts[1:]) == 0, counts


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
def test_block_records_as_a_launch_program(pkg, lib, dtype):
    """With cloneOutput=False the network is library calls only: FrameProgram records it -- the SE block is the pool's
    call and ONE cbinfer_cbchanscale_forward --, four replayed frames equal the eager network in outputs and in every
    state, held included, bit for bit."""
    net, _ = make_block(pkg, torch.float32 if dtype == np.float32 else torch.float16, 0.01, False)
    frames = block_frames(np.random.default_rng(67), 8, dtype)
    with torch.no_grad():
        for f in frames[:4]:
            net(f)
        eager = copy.deepcopy(net)
        prog = pkg.FrameProgram(net)
        for t, f in enumerate(frames[4:]):
            yp, ye = prog(f), eager(f)
            assert torch.equal(raw(yp), raw(ye)), t
            sa, sb = pkg.getStateTensors(net), pkg.getStateTensors(eager)
            assert len(sa) == len(sb) == 2 * 2 + 2 + 2      # two convs, the pool and its partials, the state and held
            for ta, tb in zip(sa, sb):
                assert torch.equal(ta, tb), t
        raws = [fn for fn, _ in prog.calls]
        assert raws.count(lib.C.cbinfer_cbchanscale_forward.raw) == 1
        assert raws.count(lib.C.cbinfer_cbadaptivepool2d_forward.raw) == 1


def test_batch_and_branch_group_refuse_the_network(pkg, lib):
    net, _ = make_block(pkg, torch.float32, 0.01, True)
    with pytest.raises(lib.CBinferError, match=r"SequenceBatch: layer 'se' is CBSqueezeExcite .*channel attention scale"):
        pkg.SequenceBatch(net, 2)
    with pytest.raises(lib.CBinferError, match=r"BranchGroup: layer '0.se' is CBSqueezeExcite .*channel attention scale"):
        pkg.BranchGroup([net])


def test_worst_figures_are_reported():
    """The worst err / bound against float64 over the tests above: measurements, not bars (the bars are 1)."""
    for key, rel in sorted(WORST.items(), key=str):
        print("%-24s worst err / bound = %.3g" % (key, rel))
    assert WORST
