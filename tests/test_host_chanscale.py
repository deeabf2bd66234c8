"""CPU-only tests of the change-based channel attention scale (CBChannelScale2d, CBSqueezeExcite,
insertCBSqueezeExcite; cb_chanscale.hip): the numpy twin of tests/chanscale_cases.py against torch's CPU
operators, the argument checks of the C entry points, the modules' refusals, buffers, pickling and wiring.  No kernel is
launched here."""
import copy
import inspect
import pickle

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import chain_cases
import chanscale_cases as cs
from optest import lib, names_of, pkg      # noqa: F401  (fixtures)


class SE(nn.Module):
    """A squeeze-and-excitation block with torchvision's attribute names."""

    def __init__(self, C, R, act=nn.ReLU, gate=nn.Sigmoid, linear=False, bias=True):
        super(SE, self).__init__()
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.linear = linear
        self.fc1 = nn.Linear(C, R, bias=bias) if linear else nn.Conv2d(C, R, 1, bias=bias)
        self.fc2 = nn.Linear(R, C, bias=bias) if linear else nn.Conv2d(R, C, 1, bias=bias)
        self.activation, self.scale_activation = act(), gate()

    def forward(self, x):
        z = self.avgpool(x)
        if self.linear:
            z = z.flatten(1)
        g = self.scale_activation(self.fc2(self.activation(self.fc1(z))))
        return x * g.reshape(1, -1, 1, 1)


class SubSE(SE):
    pass


class NotSE(SE):
    """The same attributes, another forward: the gate is added."""

    def forward(self, x):
        return x + self.scale_activation(self.fc2(self.activation(self.fc1(self.avgpool(x)))))


TV = ('fc1', 'fc2', 'activation', 'scale_activation')


# ------------------------------------------------------------------------------------------------ the twin
@pytest.mark.parametrize("dtype", [np.float32, np.float16])
def test_twin_at_threshold_zero_is_torchs_product_bit_for_bit(dtype):
    """threshold = 0, gate=None: the frame's state is torch's a * v, every special value against every other, in a
    fresh frame and in a second frame whose vector changed in some channels only."""
    s = cs.pc.specials(dtype)
    k = len(s)
    a = np.tile(s, k).reshape(k, 1, k).copy()      # a[c, 0, p] = s[p]
    v = s.copy()                                   # v[c] = s[c]
    held, tripped, out, mask, written = cs.step(a, v.astype(np.float32), np.zeros(k, np.float32), None, 0.0, True)
    want = (torch.from_numpy(a) * torch.from_numpy(v).reshape(k, 1, 1)).numpy()
    assert cs.same_bits(out, want) and tripped.all() and mask.all() and written.all()
    rng = np.random.default_rng(3)
    a = cs.pc.values(rng, (7, 3, 70), dtype)
    v1, v2 = cs.pc.values(rng, (7,), dtype, special=np.array([0.0, -0.0], dtype)), None
    v2 = v1.copy()
    v2[[1, 5]] = np.array([2.5, -0.75], dtype)
    held, _, out1, _, _ = cs.step(a, v1.astype(np.float32), np.zeros(7, np.float32), None, 0.0, True)
    listed = rng.random((3, 70)) < 0.1
    held, tripped, out2, mask, written = cs.step(a, v2.astype(np.float32), held, listed, 0.0, False, prev=out1)
    assert list(np.flatnonzero(tripped)) == [1, 5] and mask.all()
    assert np.array_equal(written.all(axis=(1, 2)), tripped) and np.array_equal(written[0], listed)
    want = (torch.from_numpy(a) * torch.from_numpy(v2).reshape(7, 1, 1)).numpy()
    assert cs.same_bits(out2, want)


def test_twin_holds_trips_and_drifts():
    """The trip rule on numbers that are exact in float32: a gate at held +- threshold holds (the comparison is
    strict), a drift of 0.375 threshold per frame holds twice and trips in the third frame, held then jumps to the
    current value; a NaN trips; nothing listed and nothing tripped leaves an empty mask."""
    a = np.ones((4, 2, 5), np.float32)
    held = np.array([1.0, 2.0, 3.0, 4.0], np.float32)
    th = 0.25
    none = np.zeros((2, 5), bool)
    g = held + np.array([0.25, -0.25, 0.0, 0.0], np.float32)
    new, tripped, out, mask, written = cs.step(a, g, held, none, th, False)
    assert not tripped.any() and not mask.any() and not written.any() and cs.same_bits(new, held)
    g = held + np.array([0.2500001, 0.0, 0.0, np.nan], np.float32)
    new, tripped, out, mask, written = cs.step(a, g, held, none, th, False)
    assert list(tripped) == [True, False, False, True] and mask.all() and np.isnan(new[3]) and new[0] == g[0]
    assert np.isnan(out[3]).all() and written[0].all() and not written[1].any()
    h = held.copy()
    for t, want in ((1, False), (2, False), (3, True)):
        g = held + np.float32(0.375 * th * t)
        h, tripped, _, _, _ = cs.step(a, g, h, none, th, False)
        assert tripped.all() == want and tripped.any() == want, t
    assert cs.same_bits(h, g)
    assert list(cs.tripped_words(np.arange(130) % 64 == 1)) == [2, 2, 2]      # (channels 1, 65 and 129)
    assert list(cs.tripped_words(np.arange(65) >= 63)) == [1 << 63, 1]


@pytest.mark.parametrize("act", cs.ACTS)
def test_excitation_twin_against_float64_and_torch(act):
    """excite() within excite_bound of the float64 value, which is torch's own float64 fc2(act(fc1(z))); the hard
    sigmoid of the twin is torch's bit for bit, its sigmoid within the 14 units."""
    rng = np.random.default_rng(5)
    for (C, R) in cs.EXCITE:
        for bias in (True, False):
            W1, b1, W2, b2 = cs.operands(rng, C, R, bias)
            z = rng.uniform(-2, 2, C).astype(np.float32)
            s = cs.excite(z, W1, b1, W2, b2, act)
            ref, _, _ = cs.excite64(z, W1, b1, W2, b2, act)
            bound = cs.excite_bound(z, W1, b1, W2, b2, act)
            assert (np.abs(s - ref) <= bound).all(), (C, R, bias, float((np.abs(s - ref) / bound).max()))
            assert (bound <= 2e-3 * (1 + np.abs(ref))).all()      # (the bound says something: three digits at the least)
            fc1, fc2 = nn.Conv2d(C, R, 1, bias=bias).double(), nn.Conv2d(R, C, 1, bias=bias).double()
            with torch.no_grad():
                fc1.weight.copy_(torch.from_numpy(W1.astype(np.float64)).reshape(R, C, 1, 1))
                fc2.weight.copy_(torch.from_numpy(W2.astype(np.float64)).reshape(C, R, 1, 1))
                if bias:
                    fc1.bias.copy_(torch.from_numpy(b1.astype(np.float64)))
                    fc2.bias.copy_(torch.from_numpy(b2.astype(np.float64)))
                fn = F.relu if act == 'relu' else F.silu
                t = fc2(fn(fc1(torch.from_numpy(z.astype(np.float64)).reshape(1, C, 1, 1)))).reshape(C).numpy()
            assert np.allclose(t, ref, rtol=1e-12, atol=1e-12)
    s = np.concatenate([cs.pc.specials(np.float32), rng.uniform(-20, 20, 500).astype(np.float32)])
    assert cs.same_bits(cs.gate_fn(s, 'hardsigmoid'), F.hardsigmoid(torch.from_numpy(s)).numpy())
    ok = np.isfinite(s)
    ref = cs.gate64(s[ok], 'sigmoid')
    assert (np.abs(cs.gate_fn(s[ok], 'sigmoid') - ref) <= cs.gate_bound(ref, 'sigmoid')).all()
    assert cs.same_bits(cs.gate_fn(s, None), s)


# ------------------------------------------------------------------------------------------------ the C entry points
def test_supported_and_bad_arguments(lib):
    C = lib.C
    assert (lib.CS_GATE_NONE, lib.CS_GATE_SIGMOID, lib.CS_GATE_HARDSIGMOID) == (0, 1, 2)
    assert (lib.CS_ACT_NONE, lib.CS_ACT_RELU, lib.CS_ACT_SILU) == (0, 1, 2)
    assert lib.ABI_VERSION == 11
    ok = [(0, 0, 1, 0), (2, 0, 4096, 0), (1, 1, 4096, 1024), (1, 2, 3, 1)]
    bad = [(3, 0, 8, 0), (-1, 0, 8, 0), (1, 0, 4097, 0), (1, 0, 0, 0), (1, 1, 8, 1025), (1, 0, 8, 4), (1, 1, 8, 0),
           (1, 3, 8, 4), (1, 0, 8, -1)]
    assert all(C.cbinfer_chanscale_supported(*a) == 1 for a in ok)
    assert all(C.cbinfer_chanscale_supported(*a) == 0 for a in bad)
    # every refusal comes before the first launch: no pointer below is ever read
    p = [0x1000 * (i + 1) for i in range(12)]
    a, v, out, gate, held, trip, cnt, bits, mcopy, w1, w2, mask = p

    def forward(**kw):
        args = dict(a=a, v=v, w1=None, b1=None, w2=None, b2=None, outputState=out, gate=gate, held=held, tripped=trip,
                    tripCount=cnt, maskA=None, listA=None, capA=0, countA=None, bits=bits, maskCopy=mcopy, C=8, R=0, H=4,
                    W=70, gateFn=1, act=0, threshold=0.1, all=0, dtype=lib.CB_F32, stream=None)
        args.update(kw)
        return C.cbinfer_cbchanscale_forward(*C.cbinfer_cbchanscale_forward.pack(**args))
    for kw in (dict(a=None), dict(v=None), dict(outputState=None), dict(gate=None), dict(held=None), dict(tripped=None),
               dict(tripCount=None), dict(bits=None), dict(maskCopy=None), dict(C=0), dict(C=4097), dict(H=0), dict(W=0),
               dict(R=-1), dict(R=4), dict(R=4, act=1), dict(R=4, act=1, w1=w1), dict(w1=w1, w2=w2), dict(act=1),
               dict(gateFn=3), dict(dtype=7), dict(threshold=-0.5), dict(threshold=float('nan')), dict(outputState=a),
               dict(gate=held), dict(maskCopy=bits), dict(maskA=bits), dict(maskA=mcopy), dict(maskA=mask, listA=mask),
               dict(countA=mask), dict(listA=mask, capA=-1), dict(v=a), dict(v=out), dict(H=1 << 16, W=1 << 15)):
        assert forward(**kw) == lib.CB_ERR_BADARG, kw
    assert C.cbinfer_chanscale_gate(None, None, None, None, None, gate, held, trip, cnt, 8, 0, 1, 0, 0.1, 0, lib.CB_F32,
                                    None) == lib.CB_ERR_BADARG
    assert C.cbinfer_chanscale_changed(a, a, held, trip, cnt, None, 0, bits, mcopy, 8, 4, 70, lib.CB_F32,
                                       None) == lib.CB_ERR_BADARG


# ------------------------------------------------------------------------------------------------ the modules
def test_refusals_by_name(pkg, lib):
    Err = lib.CBinferError
    x, v = torch.zeros(1, 8, 4, 6), torch.zeros(1, 8, 1, 1)
    plain = pkg.CBChannelScale2d(0.1)
    fused = pkg.CBChannelScale2d(0.1, fc1=nn.Conv2d(8, 2, 1), fc2=nn.Conv2d(2, 8, 1), act=nn.ReLU())

    class MyReLU(nn.ReLU):
        pass
    for call, what in (
            (lambda: pkg.CBChannelScale2d(-0.1), r"threshold=-0.1 must be a number >= 0"),
            (lambda: pkg.CBChannelScale2d(float('nan')), r"threshold=nan must be a number >= 0"),
            (lambda: pkg.CBChannelScale2d(0.1, gate='tanh'), r"gate='tanh' is not supported"),
            (lambda: pkg.CBChannelScale2d(0.1, fc1=nn.Conv2d(8, 2, 1)), r"fc1 and fc2 go together"),
            (lambda: pkg.CBChannelScale2d(0.1, act=nn.ReLU()), r"act=ReLU without fc1 / fc2"),
            (lambda: pkg.CBChannelScale2d(0.1, fc1=nn.Conv2d(8, 2, 1), fc2=nn.Conv2d(2, 8, 1)), r"act=NoneType is not"),
            (lambda: pkg.CBChannelScale2d(0.1, fc1=nn.Conv2d(8, 2, 1), fc2=nn.Conv2d(2, 8, 1), act=MyReLU()),
             r"act=MyReLU is not supported, only an nn.ReLU or an nn.SiLU"),
            (lambda: pkg.CBChannelScale2d(0.1, fc1=nn.Conv2d(8, 2, 1), fc2=nn.Conv2d(2, 8, 1), act=nn.Tanh()),
             r"act=Tanh is not supported"),
            (lambda: pkg.CBChannelScale2d(0.1, fc1=nn.Conv2d(8, 2, 3), fc2=nn.Conv2d(2, 8, 1), act=nn.ReLU()),
             r"fc1=Conv2d\(8, 2, kernel_size=\(3, 3\).*is not a plain 1x1 convolution"),
            (lambda: pkg.CBChannelScale2d(0.1, fc1=nn.Conv2d(8, 2, 1), fc2=nn.Conv2d(2, 8, 1, groups=2), act=nn.ReLU()),
             r"fc2=.*is not a plain 1x1 convolution"),
            (lambda: pkg.CBChannelScale2d(0.1, fc1=nn.Bilinear(2, 2, 2), fc2=nn.Conv2d(2, 8, 1), act=nn.ReLU()),
             r"fc1=Bilinear is not supported, only an nn.Conv2d 1x1 or an nn.Linear"),
            (lambda: pkg.CBChannelScale2d(0.1, fc1=nn.Conv2d(8, 2, 1), fc2=nn.Conv2d(3, 8, 1), act=nn.ReLU()),
             r"fc1 maps 8 -> 2 channels and fc2 3 -> 8: they do not chain"),
            (lambda: pkg.CBChannelScale2d(0.1, fc1=nn.Linear(8, 2), fc2=nn.Linear(2, 9), act=nn.SiLU()),
             r"fc1 maps 8 -> 2 channels and fc2 2 -> 9: they do not chain"),
            (lambda: pkg.CBChannelScale2d(0.1, fc1=nn.Linear(4097, 2), fc2=nn.Linear(2, 4097), act=nn.ReLU()),
             r"4097 channels with a hidden width of 2: the library takes C <= 4096 and R <= 1024"),
            (lambda: pkg.CBChannelScale2d(0.1, fc1=nn.Linear(8, 1025), fc2=nn.Linear(1025, 8), act=nn.ReLU()),
             r"8 channels with a hidden width of 1025: the library takes C <= 4096 and R <= 1024"),
            (lambda: plain(torch.zeros(1, 4097, 1, 2), torch.zeros(1, 4097, 1, 1)), r"4097 channels, the library takes C"),
            (lambda: plain(torch.zeros(8, 4, 6), v), r"operand a must be a \[1, C, H, W\] tensor"),
            (lambda: plain(x.double(), v.double()), r"float32 and float16 tensors only"),
            (lambda: plain(x, ('changeIndexes', v, None)),
             r"the vector v is a \[1, C, 1, 1\] channel vector and came with change indexes: a channel vector has no "
             r"pixels, hand it over as a bare tensor"),
            (lambda: fused(x, ('changeIndexes', v, None)), r"the pooled vector z is a \[1, C, 1, 1\] channel vector"),
            (lambda: plain(x, 3.0), r"the vector v must be a tensor, got float"),
            (lambda: plain(x, torch.zeros(1, 7, 1, 1)), r"do not fit: a is \(1, 8, 4, 6\), the vector v is \(1, 7, 1, 1\)"),
            (lambda: plain(x, torch.zeros(8)), r"must be \[1, 8, 1, 1\]"),
            (lambda: plain(x, v.half()), r"the operands differ: a is torch.float32 on cpu, the vector v is torch.float16"),
            (lambda: plain(x, v.to('meta')), r"the operands differ: .* on cpu, the vector v is torch.float32 on meta"),
            (lambda: fused(torch.zeros(1, 6, 4, 6), torch.zeros(1, 6, 1, 1)), r"6 channels, fc1 / fc2 were made for 8"),
            (lambda: plain(('changeIndexes', x), v), r"operand a is a tuple, but not"),
            (lambda: plain(x, v), "HIP devices only"), (lambda: fused(x, v), "HIP devices only")):
        with pytest.raises(Err, match=what):
            call()
    plain.threshold = -1.0      # (a threshold set later -- tuning -- is checked with every frame)
    with pytest.raises(Err, match="threshold=-1.0 must be a number >= 0"):
        plain(x, v)
    for m in (plain, fused):
        assert m.outputState.numel() == 0 and m.held.numel() == 0 and m._csWork is None      # nothing allocated or launched
        assert m.lastTrippedChannels() == 0


def test_weights_are_copied_as_float32_and_stay_so(pkg):
    torch.manual_seed(2)
    fc1, fc2 = nn.Linear(6, 3), nn.Conv2d(3, 6, 1, bias=False)
    m = pkg.CBChannelScale2d(0.05, gate='hardsigmoid', fc1=fc1, fc2=fc2, act=nn.SiLU())
    assert (m.hidden, m.gate, m.actName, m.threshold) == (3, 'hardsigmoid', 'SiLU', 0.05)
    assert m.w1.shape == (3, 6) and m.w2.shape == (6, 3) and m.b1.shape == (3,) and m.b2 is None
    assert torch.equal(m.w1, fc1.weight) and torch.equal(m.w2, fc2.weight.reshape(6, 3)) and m.w1 is not fc1.weight
    with torch.no_grad():
        fc1.weight.zero_()      # (later edits of the source are not followed)
    assert m.w1.abs().sum() > 0
    assert list(m.state_dict()) == ['w1', 'b1', 'w2', 'outputState', 'held']
    m.held = torch.arange(6.0)
    m.outputState = torch.ones(1, 6, 2, 2)
    h = copy.deepcopy(m).half()
    assert h.outputState.dtype == torch.float16
    assert all(getattr(h, n).dtype == torch.float32 for n in ('w1', 'b1', 'w2', 'held'))
    assert torch.equal(h.w1, m.w1) and torch.equal(h.held, m.held)
    # a half-precision source converts exactly
    m16 = pkg.CBChannelScale2d(0.05, fc1=nn.Conv2d(6, 3, 1).half(), fc2=nn.Conv2d(3, 6, 1).half(), act=nn.ReLU())
    assert m16.w1.dtype == torch.float32 and m16.b2.dtype == torch.float32
    assert repr(m) == "CBChannelScale2d (threshold=0.05, gate=hardsigmoid, hidden=3, act=SiLU, propChgIdxs=False)"


def test_exports_state_helpers_pickle_and_deepcopy(pkg, lib):
    import cbinfer_amd
    import pycbinfer.chanscale as alias
    assert alias is cbinfer_amd.chanscale and pkg.chanscale is alias
    for name in ('CBChannelScale2d', 'CBSqueezeExcite', 'insertCBSqueezeExcite'):
        assert getattr(pkg, name) is getattr(alias, name) is getattr(cbinfer_amd, name)
    assert all(n in pkg.__all__ for n in ('CBChannelScale2d', 'CBSqueezeExcite', 'insertCBSqueezeExcite'))
    assert pkg.CBChannelScale2d in cbinfer_amd._STATEFUL and pkg.CBSqueezeExcite not in cbinfer_amd._STATEFUL
    assert not hasattr(cbinfer_amd, '_CHANNEL_STATE')
    se = pkg.CBSqueezeExcite(0.02, nn.Conv2d(4, 2, 1), nn.Conv2d(2, 4, 1), nn.ReLU(), gate='hardsigmoid')
    assert type(se.pool) is pkg.CBPoolAvg2d and se.pool.output_size == (1, 1) and se.pool.cloneOutput is False
    assert type(se.scale) is pkg.CBChannelScale2d and (se.scale.gate, se.scale.hidden, se.threshold) == ('hardsigmoid', 2, 0.02)
    assert not hasattr(pkg.CBSqueezeExcite, 'getStateTensors')      # (a wrapper: its children keep the state)
    se.propChangeIndexes, se.cloneOutput, se.threshold = True, False, 0.03
    assert se.scale.propChangeIndexes is True and se.scale.cloneOutput is False and se.scale.threshold == 0.03
    plain = pkg.CBChannelScale2d(0.1, gate=None)
    net = nn.Sequential(se, plain)
    se.scale.outputState, se.scale.held = torch.ones(1, 4, 2, 2), torch.arange(4.0)
    plain.outputState, plain.held = torch.ones(1, 3, 2, 2), torch.arange(3.0)
    se.pool.outputState = torch.ones(1, 4, 1, 1)
    for m in (se.scale, plain):
        m.__dict__['_csWork'] = {'key': None, 'tripCount': torch.tensor([2], dtype=torch.int32)}
    assert plain.lastTrippedChannels() == 2
    states = pkg.getStateTensors(net)
    assert any(t is se.scale.held for t in states) and any(t is plain.held for t in states)
    assert any(t is se.scale.outputState for t in states) and any(t is se.pool.outputState for t in states)
    for clone in (pickle.loads(pickle.dumps(net)), copy.deepcopy(net)):
        cse, cp = clone[0], clone[1]
        assert type(cse) is pkg.CBSqueezeExcite and type(cp) is pkg.CBChannelScale2d
        assert cse.propChangeIndexes and not cse.cloneOutput and cse.threshold == 0.03 and cp.gate is None
        assert cse.scale._csWork is None and cp._csWork is None
        assert torch.equal(cse.scale.held, se.scale.held) and torch.equal(cse.scale.w1, se.scale.w1)
        assert torch.equal(cp.outputState, plain.outputState) and repr(cse) == repr(se)
    pkg.clearMemory(net)
    for m in (se.scale, plain):
        assert m.outputState.numel() == 0 and m.held.numel() == 0 and m._csWork is None
        assert m.held.dtype == torch.float32
    assert se.pool.outputState.numel() == 0 and se.scale.w1.numel() == 8      # (the weights are no state)


def test_the_chain_tables_are_as_they_were(pkg):
    """The scale and its wiring module are rows of chain.PRODUCERS and producers for no pass yet: chain.PASSES has the
    names that tests/chain_cases.py and tests/test_host_chain.py write out, every pass accepts what it did, and
    insertCBSqueezeExcite walks behind the producers of insertCBGating."""
    from cbinfer_amd import batch, chain
    import test_host_chain
    assert len(chain.PASSES) == len(chain_cases.PASSES) == len(test_host_chain.MATRIX) == 11
    assert list(chain.PASSES) == list(test_host_chain.MATRIX)
    assert len(chain.PRODUCERS) == 23
    assert [row for row in chain.PRODUCERS if 'Scale' in row[0] or 'Squeeze' in row[0]] == [
        ('CBChannelScale2d', 'chanscale', chain.ONLY, ()), ('CBSqueezeExcite', 'chanscale', chain.ONLY, ())]
    for p in chain.PASSES:
        assert pkg.CBChannelScale2d not in chain.producers(p) and pkg.CBSqueezeExcite not in chain.producers(p), p
    assert set(chain_cases.producer_type(c) for c in chain_cases.CASES) <= set(row[0] for row in chain.PRODUCERS)
    assert 'insertCBSqueezeExcite' not in chain.PASSES
    assert "producers('insertCBGating')" in inspect.getsource(pkg.insertCBSqueezeExcite)
    assert [row for row in batch.CHAIN_OPERATORS if {pkg.CBChannelScale2d, pkg.CBSqueezeExcite} & set(row[0])] == [
        ((pkg.CBSqueezeExcite, pkg.CBChannelScale2d), 'a change-based channel attention scale',
         'squeeze-and-excitation')]
    assert not hasattr(batch, 'CHANNEL_OPERATORS')


# ------------------------------------------------------------------------------------------------ wiring
def test_insert_squeeze_excite_wiring_and_what_it_leaves(pkg, lib):
    torch.manual_seed(1)
    seq = nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), SE(8, 2), nn.Conv2d(8, 8, 1), SE(8, 4, nn.SiLU, nn.Hardsigmoid, True),
                        nn.Conv2d(8, 6, 3, padding=1), SE(6, 3, bias=False)).eval()
    net = pkg.convert(seq, threshold=0.05)
    assert names_of(net) == ['CBConv2d', 'SE', 'CBConv2d', 'SE', 'CBConv2d', 'SE']
    net[4].copyInput = False
    want = [copy.deepcopy(net[i]) for i in (1, 3, 5)]
    assert pkg.insertCBSqueezeExcite(net, {SE: TV}, 0.02, cloneOutput=False) is net
    assert names_of(net) == ['CBConv2d', 'CBSqueezeExcite'] * 3 and list(net._modules) == ['0', '1', '2', '3', '4', '5']
    assert net[0].propChangeIndexes and net[2].propChangeIndexes and net[4].propChangeIndexes
    assert net[1].propChangeIndexes and not net[3].propChangeIndexes and not net[5].propChangeIndexes      # (1x1 behind [1])
    assert net[4].copyInput is True and not any(m.cloneOutput for m in (net[1], net[3], net[5]))
    assert all(m.pool.cloneOutput is False and not m.pool.propChangeIndexes for m in (net[1], net[3], net[5]))
    assert [(m.scale.gate, m.scale.actName, m.scale.hidden, m.scale.threshold) for m in (net[1], net[3], net[5])] == [
        ('sigmoid', 'ReLU', 2, 0.02), ('hardsigmoid', 'SiLU', 4, 0.02), ('sigmoid', 'ReLU', 3, 0.02)]
    for cb, src in zip((net[1], net[3], net[5]), want):
        assert torch.equal(cb.scale.w1, src.fc1.weight.reshape(cb.scale.w1.shape))
        assert torch.equal(cb.scale.w2, src.fc2.weight.reshape(cb.scale.w2.shape))
        assert (cb.scale.b1 is None) == (src.fc1.bias is None)
    # a feedback-mode consumer keeps no input reference; the default clones
    net = pkg.convert(nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), SE(8, 2), nn.Conv2d(8, 3, 3, padding=1)).eval(),
                      threshold=0.05)
    net[2].copyInput, net[2].feedbackLoop = False, True
    pkg.insertCBSqueezeExcite(net, {SE: TV}, 0.0)
    assert type(net[1]) is pkg.CBSqueezeExcite and net[1].cloneOutput and net[2].copyInput is False
    # behind the other producers of insertCBGating
    for prod in (pkg.CBPointwise2d(nn.Tanh()), pkg.CBBinary2d('mul', other=2.0), pkg.CBChannelReduce2d(nn.Softmax2d()),
                 pkg.CBAdd2d()):
        net = pkg.insertCBSqueezeExcite(nn.Sequential(prod, SE(8, 2)), {SE: TV}, 0.1)
        assert type(net[1]) is pkg.CBSqueezeExcite and net[0].propChangeIndexes, type(prod).__name__
    # a subclass, a type that is not named, a block behind a non-producer or at the front, a gate or an activation the
    # kernel does not have: dense, flags untouched
    seq = nn.Sequential(SE(3, 2), nn.Conv2d(3, 8, 3, padding=1), SubSE(8, 2), nn.Conv2d(8, 8, 1), nn.Tanh(), SE(8, 2),
                        nn.Conv2d(8, 8, 1), SE(8, 2, gate=nn.Tanh), nn.Conv2d(8, 8, 1), SE(8, 2, act=nn.GELU)).eval()
    net = pkg.convert(seq, threshold=0.05)
    before = names_of(net)
    pkg.insertCBSqueezeExcite(net, {SE: TV}, 0.1)
    assert names_of(net) == before == ['SE', 'CBConv2d', 'SubSE', 'CBConv2d', 'Tanh', 'SE', 'CBConv2d', 'SE', 'CBConv2d',
                                       'SE']
    assert not any(getattr(m, 'propChangeIndexes', False) for m in net)
    net = pkg.convert(nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), SE(8, 2)).eval(), threshold=0.05)
    assert names_of(pkg.insertCBSqueezeExcite(net, {}, 0.1)) == ['CBConv2d', 'SE']


def test_a_class_with_another_forward_is_refused_by_name(pkg, lib):
    net = pkg.convert(nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), NotSE(8, 2)).eval(), threshold=0.05)
    with pytest.raises(lib.CBinferError, match=r"insertCBSqueezeExcite: NotSE does not compute x \* scale_activation\("
                                               r"fc2\(activation\(fc1\(mean\(x\)\)\)\)\)"):
        pkg.insertCBSqueezeExcite(net, {NotSE: TV}, 0.1)
    assert names_of(net) == ['CBConv2d', 'NotSE'] and not net[0].propChangeIndexes
    with pytest.raises(lib.CBinferError, match=r"NotSE has no sub-module 'gate'"):
        pkg.insertCBSqueezeExcite(net, {NotSE: ('fc1', 'fc2', 'activation', 'gate')}, 0.1)
    with pytest.raises(lib.CBinferError, match=r"seTypes maps a class to its four attribute names"):
        pkg.insertCBSqueezeExcite(net, {NotSE: ('fc1', 'fc2')}, 0.1)
    with pytest.raises(lib.CBinferError, match=r"threshold=-1 must be a number >= 0"):
        pkg.insertCBSqueezeExcite(net, {NotSE: TV}, -1)
    # the random tensor of the self-check leaves torch's generator alone
    net = pkg.convert(nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), SE(8, 2)).eval(), threshold=0.05)
    torch.manual_seed(7)
    a = torch.rand(3)
    torch.manual_seed(7)
    assert type(pkg.insertCBSqueezeExcite(net, {SE: TV}, 0.1)[1]) is pkg.CBSqueezeExcite
    assert torch.equal(torch.rand(3), a)


def test_batch_branch_and_program_refusals_name_the_module(pkg, lib):
    net = nn.Sequential()
    net.add_module('stem', pkg.convert(nn.Sequential(nn.Conv2d(3, 8, 3, padding=1)).eval(), threshold=0.05)[0])
    net.add_module('se', pkg.CBSqueezeExcite(0.02, nn.Conv2d(8, 2, 1), nn.Conv2d(2, 8, 1), nn.ReLU()))
    with pytest.raises(lib.CBinferError, match=r"SequenceBatch: layer 'se' is CBSqueezeExcite \(.*a change-based channel "
                                               r"attention scale.*squeeze-and-excitation"):
        pkg.SequenceBatch(net, 2)
    with pytest.raises(lib.CBinferError, match=r"BranchGroup: layer '0.se' is CBSqueezeExcite \(.*channel attention scale"):
        pkg.BranchGroup([net])
    net = nn.Sequential()
    net.add_module('stem', pkg.convert(nn.Sequential(nn.Conv2d(3, 8, 3, padding=1)).eval(), threshold=0.05)[0])
    net.add_module('eca', pkg.CBChannelScale2d(0.02))
    with pytest.raises(lib.CBinferError, match=r"SequenceBatch: layer 'eca' is CBChannelScale2d \(threshold=0.02"):
        pkg.SequenceBatch(net, 2)
    with pytest.raises(lib.CBinferError, match=r"BranchGroup: layer '0.eca' is CBChannelScale2d"):
        pkg.BranchGroup([net])
    import cbinfer_amd.program as program
    assert "pycbinfer.CBSqueezeExcite (insertCBSqueezeExcite)" in inspect.getsource(pkg.FrameProgram)
    assert 'CBSqueezeExcite' in program.__doc__
