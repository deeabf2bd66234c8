"""CPU-only tests of the change-based rearrangements: the numpy twins of tests/rearrange_cases.py against
torch's CPU operators bit for bit and against a brute-force footprint, what the constructors take and refuse, the host
entry points and the argument checks of the C entry point, what insertCBRearrange and the passes behind it do to a
network, exports, pickling and the refusals.  No kernel is launched here."""
import copy
import ctypes
import pickle

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import rearrange_cases as rc
from optest import lib, names_of, pkg      # noqa: F401  (fixtures)


def torch_op(kind, f, x):
    """torch's CPU operator on x [1, C, H, W]."""
    if kind == "shuffle":
        return F.pixel_shuffle(x, f)
    if kind == "unshuffle":
        return F.pixel_unshuffle(x, f)
    return F.channel_shuffle(x, f)


# ------------------------------------------------------------------------------------------------ the twins
@pytest.mark.parametrize("npdt", [np.float32, np.float16], ids=["f32", "f16"])
def test_value_twins_are_torch_bit_for_bit(npdt):
    """Every shape of the three tables; the values hold -0, +-inf and NaNs with payloads and are compared as integers."""
    rng = np.random.default_rng(1)
    for kind, f, shape, row in rc.cases():
        x = rc.special_values(rng, shape, npdt)
        want = torch_op(kind, f, torch.from_numpy(x)[None])[0].numpy()
        got = rc.twin(kind, f, x)
        assert got.shape == want.shape == rc.out_shape(kind, f, shape), (kind, row)
        assert rc.same_bits(got, want), (kind, row)
    # the formulas on a hand-made case each
    x = np.arange(8 * 1 * 2, dtype=np.float32).reshape(8, 1, 2)
    y = rc.twin("shuffle", 2, x)      # out[c, i, 2 x + j] = in[4 c + 2 i + j, 0, x]
    assert y.shape == (2, 2, 4) and list(y[1, 1]) == [x[6, 0, 0], x[7, 0, 0], x[6, 0, 1], x[7, 0, 1]]
    assert rc.same_bits(rc.twin("unshuffle", 2, y), x)
    z = rc.twin("channels", 2, np.arange(6, dtype=np.float32).reshape(6, 1, 1))      # out[2 k + q] = in[3 q + k]
    assert list(z[:, 0, 0]) == [0, 3, 1, 4, 2, 5]


def test_footprint_twins_against_brute_force():
    """An output pixel is listed iff one of the input pixels it reads -- found by rearranging the pixels' own numbers --
    changed."""
    rng = np.random.default_rng(2)
    for kind, f, shape, row in rc.cases():
        Cn, H, W = shape
        ids = np.broadcast_to(np.arange(H * W, dtype=np.int64).reshape(1, H, W), shape)
        reads = rc.twin(kind, f, ids)                     # [Co, Ho, Wo]: the input pixel each output value reads
        masks = [rng.random((H, W)) < p for p in (0.0, 0.05, 0.5, 1.0)]
        one = np.zeros((H, W), dtype=bool)
        one[H - 1, W - 1] = True
        for changed in masks + [one]:
            brute = changed.reshape(-1)[reads].any(0)
            got = rc.footprint(kind, f, changed)
            assert got.dtype == bool and np.array_equal(got, brute), (kind, row)
    m = np.zeros((2, 3), dtype=bool)
    m[1, 2] = True
    want = np.zeros((6, 9), dtype=bool)
    want[3:6, 6:9] = True
    assert np.array_equal(rc.footprint("shuffle", 3, m), want)
    assert np.array_equal(rc.footprint("unshuffle", 3, want), m)
    last = np.zeros((6, 9), dtype=bool)
    last[5, 8] = True      # the last sub-pixel of the last block alone
    assert np.array_equal(rc.footprint("unshuffle", 3, last), m)


# ------------------------------------------------------------------------------------------------ the constructors
class MyShuffle(nn.PixelShuffle):
    pass


class MyChannels(nn.ChannelShuffle):
    pass


def test_constructors_take_and_refuse(pkg, lib):
    P, S, Err = pkg.CBPixelShuffle2d, pkg.CBChannelShuffle2d, lib.CBinferError
    for m, want in ((nn.PixelShuffle(2), (lib.REARRANGE_SHUFFLE, 2, False)),
                    (nn.PixelShuffle(1), (lib.REARRANGE_SHUFFLE, 1, False)),
                    (nn.PixelShuffle(8), (lib.REARRANGE_SHUFFLE, 8, False)),
                    (nn.PixelUnshuffle(3), (lib.REARRANGE_UNSHUFFLE, 3, True)),
                    (nn.PixelUnshuffle(8), (lib.REARRANGE_UNSHUFFLE, 8, True))):
        cb = P(m)
        assert (cb.kind, cb.factor, cb.unshuffle) == want, m
        assert not cb.propChangeIndexes and cb.cloneOutput and cb.outputState.numel() == 0
        assert ('downscale_factor=%d' if want[2] else 'upscale_factor=%d') % want[1] in repr(cb)
        assert lib.C.cbinfer_rearrange_supported(cb._struct()) == 1
    for g in (1, 3, 300):
        cb = S(nn.ChannelShuffle(g))
        assert (cb.kind, cb.factor, cb.groups) == (lib.REARRANGE_CHANNELS, g, g) and 'groups=%d' % g in repr(cb)
        assert not cb.propChangeIndexes and cb.cloneOutput and lib.C.cbinfer_rearrange_supported(cb._struct()) == 1
    for ctor, m, what in ((P, MyShuffle(2), "not a subclass.*MyShuffle"), (P, nn.PixelShuffle(9), "upscale_factor=9"),
                          (P, nn.PixelShuffle(0), "upscale_factor=0"), (P, nn.PixelUnshuffle(9), "downscale_factor=9"),
                          (P, nn.PixelUnshuffle(0), "downscale_factor=0"), (P, nn.PixelShuffle(2.0), "upscale_factor=2.0"),
                          (P, nn.ChannelShuffle(2), "nn.PixelShuffle and nn.PixelUnshuffle"),
                          (P, nn.Upsample(scale_factor=2), "nn.PixelShuffle and nn.PixelUnshuffle"),
                          (S, MyChannels(2), "not a subclass.*MyChannels"), (S, nn.ChannelShuffle(0), "groups=0"),
                          (S, nn.ChannelShuffle(-2), "groups=-2"), (S, nn.PixelShuffle(2), "nn.ChannelShuffle"),
                          (S, nn.Conv2d(3, 3, 1), "nn.ChannelShuffle")):
        with pytest.raises(Err, match=what):
            ctor(m)


# ------------------------------------------------------------------------------------------------ the C ABI
def re_struct(lib, kind, factor):
    return ctypes.pointer(lib.Rearrange(kind, factor))


def test_supported_and_out_shape_over_the_limits(lib):
    C = lib.C
    SH, UN, CH = lib.REARRANGE_SHUFFLE, lib.REARRANGE_UNSHUFFLE, lib.REARRANGE_CHANNELS
    assert (SH, UN, CH) == (rc.SHUFFLE, rc.UNSHUFFLE, rc.CHANNELS) == (0, 1, 2)
    for kind in (SH, UN):
        assert [C.cbinfer_rearrange_supported(re_struct(lib, kind, f)) for f in range(-1, 11)] == \
            [0, 0] + [1] * 8 + [0, 0]
    assert [C.cbinfer_rearrange_supported(re_struct(lib, CH, g)) for g in (-1, 0, 1, 8, 9, 1 << 20)] == [0, 0, 1, 1, 1, 1]
    assert C.cbinfer_rearrange_supported(re_struct(lib, 3, 2)) == 0
    assert C.cbinfer_rearrange_supported(re_struct(lib, -1, 2)) == 0
    assert C.cbinfer_rearrange_supported(None) == 0

    def shape(kind, f, Cn, H, W, r=True):
        co, ho, wo = ctypes.c_int(-7), ctypes.c_int(-7), ctypes.c_int(-7)
        st = C.cbinfer_rearrange_out_shape(re_struct(lib, kind, f) if r else None, Cn, H, W, ctypes.byref(co),
                                           ctypes.byref(ho), ctypes.byref(wo))
        return st, (co.value, ho.value, wo.value)

    untouched = (-7, -7, -7)
    for kindName, f, inShape, row in rc.cases():
        assert shape(rc.KINDS.index(kindName), f, *inShape) == (0, rc.out_shape(kindName, f, inShape)), row
    assert shape(SH, 2, 8, 3, 5) == (0, (2, 6, 10)) and shape(UN, 2, 2, 6, 10) == (0, (8, 3, 5))
    assert shape(CH, 5, 5, 2, 9) == (0, (5, 2, 9))
    # nothing divides: CB_ERR_BADARG (-1); beyond the limits: CB_ERR_UNSUPPORTED (-2); the outputs stay untouched
    for bad in ((SH, 2, 6, 3, 5), (SH, 3, 12, 3, 5), (UN, 2, 2, 5, 10), (UN, 2, 2, 6, 9), (UN, 8, 1, 4, 8), (CH, 4, 6, 2, 2),
                (CH, 7, 6, 2, 2), (SH, 1, 0, 2, 2), (UN, 1, 1, 0, 2), (CH, 1, 1, 2, -1)):
        assert shape(*bad) == (-1, untouched), bad
    for bad in ((SH, 9, 81, 3, 5), (UN, 0, 2, 6, 10), (CH, 0, 6, 2, 2), (5, 2, 8, 4, 4)):
        assert shape(*bad) == (-2, untouched), bad
    assert shape(SH, 2, 8, 3, 5, r=False) == (-1, untouched)
    assert C.cbinfer_rearrange_out_shape(re_struct(lib, SH, 2), 8, 3, 5, None, None, None) == -1


def test_c_entry_point_checks_its_arguments(lib):
    """Bad arguments return CB_ERR_BADARG (-1) before anything is launched (the device pointers here are never
    followed)."""
    C = lib.C
    assert C.cbinfer_abi_version() == 11
    SH, UN, CH = lib.REARRANGE_SHUFFLE, lib.REARRANGE_UNSHUFFLE, lib.REARRANGE_CHANNELS
    X, O, BITS, COPY, M, L, N2 = (0x10000 * i for i in range(1, 8))

    def go(x=X, o=O, mask=None, lst=None, cap=0, count=None, bits=BITS, cp=COPY, Cn=8, H=4, W=6, r=(SH, 2),
           dt=lib.CB_F32):
        return C.cbinfer_cbrearrange_forward(x, o, mask, lst, cap, count, bits, cp, Cn, H, W,
                                             re_struct(lib, *r) if r is not None else None, dt, None)

    for bad in (dict(x=None), dict(o=None), dict(o=X), dict(bits=None), dict(cp=None), dict(cp=BITS), dict(r=None),
                dict(Cn=0), dict(H=0), dict(W=-1), dict(dt=lib.CB_F32S), dict(dt=7), dict(lst=L, cap=-1),
                dict(mask=M, lst=L), dict(count=N2), dict(mask=BITS), dict(mask=COPY),
                # the kind, the factor and what it must divide
                dict(r=(3, 2)), dict(r=(-1, 2)), dict(r=(SH, 0)), dict(r=(SH, 9)), dict(r=(UN, 0)), dict(r=(UN, 9)),
                dict(r=(CH, 0)), dict(r=(CH, -3)), dict(Cn=6), dict(r=(SH, 3)), dict(r=(UN, 4)), dict(r=(UN, 2), H=5),
                dict(r=(UN, 3), H=6, W=8), dict(r=(CH, 3)), dict(r=(CH, 16)),
                # Ho Wo, H W or 64 Co beyond an int32
                dict(Cn=4, H=1 << 15, W=1 << 14), dict(r=(UN, 2), H=1 << 16, W=1 << 15),
                dict(r=(CH, 1), H=1 << 16, W=1 << 15), dict(r=(CH, 1), Cn=1 << 25), dict(r=(SH, 1), Cn=1 << 25),
                dict(r=(UN, 8), Cn=1 << 19, H=8, W=8)):
        assert go(**bad) == -1, bad


# ------------------------------------------------------------------------------------------------ insertCBRearrange
def test_insert_rearrange_on_espcn_type_stacks(pkg):
    torch.manual_seed(1)
    seq = nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), nn.ReLU(), nn.Conv2d(8, 16, 3, padding=1), nn.PixelShuffle(2),
                        nn.Conv2d(4, 3, 3, padding=1)).eval()
    net = pkg.convert(seq, threshold=0.05)
    assert names_of(net) == ['CBConv2d', 'CBConv2d', 'PixelShuffle', 'CBConv2d']
    net[3].copyInput = False
    assert pkg.insertCBRearrange(net, cloneOutput=False) is net
    assert names_of(net) == ['CBConv2d', 'CBConv2d', 'CBPixelShuffle2d', 'CBConv2d']
    assert list(net._modules) == ['0', '2', '3', '4']
    ps = net[2]
    assert (ps.kind, ps.factor, ps.cloneOutput, ps.propChangeIndexes) == (rc.SHUFFLE, 2, False, False)
    assert net[1].propChangeIndexes and not net[0].propChangeIndexes and net[3].copyInput is True
    # a stack ending in a 1x1 layer: the shuffle hands its changes on; a feedback-mode consumer keeps no input reference
    seq = nn.Sequential(nn.Conv2d(3, 18, 3, padding=1), nn.PixelShuffle(3), nn.Conv2d(2, 3, 1)).eval()
    net = pkg.insertCBRearrange(pkg.convert(seq, threshold=0.05))
    assert names_of(net) == ['CBConv2d', 'CBPixelShuffle2d', 'CBConv2d']
    assert net[0].propChangeIndexes and net[1].propChangeIndexes and net[1].cloneOutput and net[1].factor == 3
    net = pkg.convert(nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), nn.PixelShuffle(2), nn.Conv2d(2, 3, 3, padding=1)).eval(),
                      threshold=0.05)
    net[2].copyInput, net[2].feedbackLoop = False, True
    pkg.insertCBRearrange(net)
    assert type(net[1]) is pkg.CBPixelShuffle2d and net[2].copyInput is False and not net[1].propChangeIndexes
    # conv -> pixel shuffle -> activation -> 1x1 (ESPCN's order): insertCBPointwise takes the shuffle as a producer, and
    # so do the other passes; an unshuffle and a second shuffle behind a shuffle are converted too
    seq = nn.Sequential(nn.Conv2d(3, 16, 3, padding=1), nn.PixelShuffle(2), nn.Tanh(), nn.Conv2d(4, 4, 1),
                        nn.PixelUnshuffle(2), nn.PixelShuffle(4), nn.Upsample(scale_factor=2),
                        nn.ConvTranspose2d(1, 2, 2, stride=2)).eval()
    net = pkg.convert(seq, threshold=0.05)
    pkg.insertCBTransposedConv(pkg.insertCBUpsampling(pkg.insertCBPointwise(pkg.insertCBRearrange(net))))
    assert names_of(net) == ['CBConv2d', 'CBPixelShuffle2d', 'CBPointwise2d', 'CBConv2d', 'CBPixelShuffle2d',
                             'CBPixelShuffle2d', 'CBUpsample2d', 'CBConvTranspose2d']
    assert net[1].propChangeIndexes and net[2].propChangeIndexes and net[3].propChangeIndexes
    assert net[4].unshuffle and net[4].propChangeIndexes and not net[5].unshuffle and net[5].propChangeIndexes
    # (insertCBUpsampling and insertCBTransposedConv directly behind a shuffle)
    seq = nn.Sequential(nn.Conv2d(3, 4, 3, padding=1), nn.PixelShuffle(2), nn.ConvTranspose2d(1, 2, 2, stride=2)).eval()
    net = pkg.insertCBTransposedConv(pkg.insertCBRearrange(pkg.convert(seq, threshold=0.05)))
    assert names_of(net) == ['CBConv2d', 'CBPixelShuffle2d', 'CBConvTranspose2d']


def test_insert_rearrange_on_a_shufflenet_type_unit(pkg):
    torch.manual_seed(2)
    seq = nn.Sequential(nn.Conv2d(12, 12, 1, groups=3), nn.ReLU(), nn.ChannelShuffle(3),
                        nn.Conv2d(12, 12, 3, padding=1, groups=12), nn.Conv2d(12, 12, 1, groups=3)).eval()
    net = pkg.convert(seq, threshold=0.05, grouped=True, depthwise=True)
    assert names_of(net) == ['CBGroupedConv2d', 'ChannelShuffle', 'CBDepthwiseConv2d', 'CBGroupedConv2d']
    assert not net[0].propChangeIndexes
    pkg.insertCBRearrange(net)
    assert names_of(net) == ['CBGroupedConv2d', 'CBChannelShuffle2d', 'CBDepthwiseConv2d', 'CBGroupedConv2d']
    assert net[0].propChangeIndexes and not net[1].propChangeIndexes and not net[2].propagatedChanges
    pkg.insertCBPointwise(pkg.linkDepthwise(net))
    assert names_of(net) == ['CBGroupedConv2d', 'CBChannelShuffle2d', 'CBDepthwiseConv2d', 'CBGroupedConv2d']
    assert net[2].propagatedChanges and net[1].propChangeIndexes and net[0].propChangeIndexes
    assert net[1].groups == 3 and net[1].cloneOutput and not net[3].propChangeIndexes


def test_operators_behind_a_non_producer_or_beyond_the_limits_stay_dense(pkg):
    seq = nn.Sequential(nn.PixelUnshuffle(2), nn.Conv2d(12, 81, 3, padding=1), nn.PixelShuffle(9), nn.Conv2d(1, 4, 1),
                        nn.Tanh(), nn.PixelShuffle(2), nn.Conv2d(1, 4, 1), nn.ChannelShuffle(0), MyShuffle(2),
                        nn.Conv2d(1, 4, 1), nn.Sequential(nn.ChannelShuffle(2))).eval()
    net = pkg.convert(seq, threshold=0.05)
    before = names_of(net)
    flags = [getattr(m, 'propChangeIndexes', None) for m in net]
    pkg.insertCBRearrange(net)
    assert names_of(net) == before == ['PixelUnshuffle', 'CBConv2d', 'PixelShuffle', 'CBConv2d', 'Tanh', 'PixelShuffle',
                                       'CBConv2d', 'ChannelShuffle', 'MyShuffle', 'CBConv2d', 'Sequential']
    assert [getattr(m, 'propChangeIndexes', None) for m in net] == flags and not any(f for f in flags)
    assert type(net[10][0]) is nn.ChannelShuffle      # (first in its container: no producer in front)


def test_the_producer_tables(pkg):
    from cbinfer_amd import chain
    # (every pass's whole set, in order: test_host_chain.py)
    shuffles = (pkg.CBPixelShuffle2d, pkg.CBChannelShuffle2d)
    pools = ['insertCBPooling', 'insertCBPooling(generalGeometry=True)']
    assert [name for name in chain.PASSES if not set(shuffles) & set(chain.producers(name))] == pools
    assert all(tuple(t for t in chain.producers(name) if t in shuffles) == shuffles
               for name in chain.PASSES if name not in pools)
    # a grouped convolution: for this pass and the later ones, not for the four before it
    assert [name for name in chain.PASSES if pkg.CBGroupedConv2d in chain.producers(name)] == [
        'insertCBRearrange', 'insertCBChannelOps', 'insertCBPadding', 'insertCBGating', 'insertCBResize']


# ------------------------------------------------------------------------------------------------ module hygiene
def test_exports_state_helpers_and_pickling(pkg, lib):
    import cbinfer_amd
    assert all(n in pkg.__all__ for n in ('CBPixelShuffle2d', 'CBChannelShuffle2d', 'insertCBRearrange'))
    assert pkg.rearrange is cbinfer_amd.rearrange
    import pycbinfer.rearrange as alias
    assert alias is cbinfer_amd.rearrange and pkg.CBPixelShuffle2d is alias.CBPixelShuffle2d
    assert pkg.CBChannelShuffle2d is alias.CBChannelShuffle2d and pkg.insertCBRearrange is alias.insertCBRearrange
    assert {'cbinfer_rearrange_supported', 'cbinfer_rearrange_out_shape', 'cbinfer_cbrearrange_forward'} <= set(
        lib.EXPORTED_SYMBOLS)
    assert lib.C.cbinfer_cbrearrange_forward.launcher and not lib.C.cbinfer_rearrange_out_shape.launcher
    ps, un, cs = (pkg.CBPixelShuffle2d(nn.PixelShuffle(3)), pkg.CBPixelShuffle2d(nn.PixelUnshuffle(2)),
                  pkg.CBChannelShuffle2d(nn.ChannelShuffle(4)))
    ps.propChangeIndexes, ps.cloneOutput = True, False
    cs.propChangeIndexes = True
    net = nn.Sequential(ps, un)
    net.add_module('cs', cs)
    ps.outputState, un.outputState, cs.outputState = torch.ones(1, 2, 6, 9), torch.ones(1, 8, 3, 4), torch.ones(1, 8, 3, 4)
    for m in (ps, un, cs):
        m._struct()
        m.__dict__['_work'] = {'key': None}
    states = pkg.getStateTensors(net)
    assert len(states) == 3 and all(any(t is m.outputState for t in states) for m in (ps, un, cs))
    for clone in (pickle.loads(pickle.dumps(net)), copy.deepcopy(net)):
        p, u, c = clone[0], clone[1], clone.cs
        assert type(p) is pkg.CBPixelShuffle2d and type(u) is pkg.CBPixelShuffle2d and type(c) is pkg.CBChannelShuffle2d
        assert (p.kind, p.factor, p.propChangeIndexes, p.cloneOutput) == (rc.SHUFFLE, 3, True, False)
        assert (u.kind, u.factor, u.propChangeIndexes, u.cloneOutput) == (rc.UNSHUFFLE, 2, False, True)
        assert (c.kind, c.factor, c.propChangeIndexes, c.cloneOutput) == (rc.CHANNELS, 4, True, True)
        for new, old in ((p, ps), (u, un), (c, cs)):
            assert new._work is None and new._reC is None      # transients dropped ...
            assert torch.equal(new.outputState, old.outputState) and repr(new) == repr(old)      # ... state kept
            assert lib.C.cbinfer_rearrange_supported(new._struct()) == 1
            assert (new._struct().contents.kind, new._struct().contents.factor) == (old.kind, old.factor)
    pkg.clearMemory(net)
    for m in (ps, un, cs):
        assert m.outputState.numel() == 0 and m._work is None


def test_forward_refusals_without_a_device(pkg, lib, monkeypatch):
    from cbinfer_amd.conv2d_cg import ChangeIndexes
    Err = lib.CBinferError
    ps, un, cs = (pkg.CBPixelShuffle2d(nn.PixelShuffle(2)), pkg.CBPixelShuffle2d(nn.PixelUnshuffle(2)),
                  pkg.CBChannelShuffle2d(nn.ChannelShuffle(2)))
    x = torch.zeros(1, 4, 6, 8)
    for m, name in ((ps, "CBPixelShuffle2d"), (un, "CBPixelShuffle2d"), (cs, "CBChannelShuffle2d")):
        for inp, what in ((torch.zeros(2, 4, 6, 8), r"\[1, C, H, W\]"), (torch.zeros(4, 6, 8), r"\[1, C, H, W\]"),
                          (torch.zeros(1, 4, 6, 8, dtype=torch.int32), "float32 and float16"),
                          (x.double(), "float32 and float16"), (('changeIndexes', x), "tuple"),
                          (('indexes', x, None), "tuple"), (None, "must be a tensor"), (x, "HIP devices only")):
            with pytest.raises(Err, match=name + ": .*" + what if "HIP" not in what else what):
                m(inp)
    # sizes the factor does not divide: the refusal names the size
    with pytest.raises(Err, match="CBPixelShuffle2d: the input has 6 channels.*= 4 does not divide"):
        ps(torch.zeros(1, 6, 6, 8))
    with pytest.raises(Err, match="CBPixelShuffle2d: the input is a 5x8 map.*= 2 must divide"):
        un(torch.zeros(1, 4, 5, 8))
    with pytest.raises(Err, match="CBPixelShuffle2d: the input is a 6x7 map"):
        un(torch.zeros(1, 4, 6, 7))
    with pytest.raises(Err, match="CBChannelShuffle2d: the input has 5 channels.*groups = 2 does not divide"):
        cs(torch.zeros(1, 5, 6, 8))
    with pytest.raises(Err, match="CBChannelShuffle2d: the input has 2 channels.*groups = 4"):
        pkg.CBChannelShuffle2d(nn.ChannelShuffle(4))(torch.zeros(1, 2, 6, 8))
    # indexes of another map size or type: refused by chain.operand_changes, whose only need of a device is the module's
    # workspace -- the device check is taken out of the way, nothing is launched before the refusal
    import cbinfer_amd.rearrange as mod
    monkeypatch.setattr(mod, 'require_device', lambda *tensors: None)
    wrong = ChangeIndexes(torch.zeros(4, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), (7, 8))
    for m, name in ((ps, "CBPixelShuffle2d"), (un, "CBPixelShuffle2d"), (cs, "CBChannelShuffle2d")):
        with pytest.raises(Err, match=name + ".*7x8 map.*6x8"):
            m(('changeIndexes', x, wrong))
        with pytest.raises(Err, match=name + ".*int32 tensor or a ChangeIndexes"):
            m(('changeIndexes', x, [1, 2]))
        with pytest.raises(Err, match=name + ".*contiguous one-dimensional int32"):
            m(('changeIndexes', x, torch.zeros(3, dtype=torch.int64)))
        assert m.outputState.numel() == 0


def test_batch_and_branch_refusals_name_the_layer(pkg, lib):
    for kind, mod in (("CBPixelShuffle2d", pkg.CBPixelShuffle2d(nn.PixelShuffle(2))),
                      ("CBPixelShuffle2d", pkg.CBPixelShuffle2d(nn.PixelUnshuffle(2))),
                      ("CBChannelShuffle2d", pkg.CBChannelShuffle2d(nn.ChannelShuffle(2)))):
        net = nn.Sequential()
        net.add_module('stem', pkg.convert(nn.Sequential(nn.Conv2d(3, 8, 3, padding=1)).eval(), threshold=0.05)[0])
        net.add_module('re', mod)
        with pytest.raises(lib.CBinferError, match=r"SequenceBatch: layer 're' is %s \(.*a change-based rearrangement.*"
                                                   r"super-resolution and ShuffleNet-type" % kind):
            pkg.SequenceBatch(net, 2)
        with pytest.raises(lib.CBinferError, match=r"BranchGroup: layer '0.re' is %s \(.*a change-based rearrangement"
                                                   % kind):
            pkg.BranchGroup([net])


def test_frame_program_names_the_modules(pkg):
    import cbinfer_amd.program as program
    assert 'CBPixelShuffle2d' in program.__doc__ and 'CBChannelShuffle2d' in program.__doc__
