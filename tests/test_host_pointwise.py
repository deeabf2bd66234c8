"""CPU-only tests of the change-based element-wise functions: the numpy twin of tests/pointwise_cases.py
against torch's CPU operators (bit for bit) and against a float64 batch norm, the argument checks of the C entry points,
the constructor's refusals, insertCBPointwise's structure, the producer lists, pickling and the refusals.  No kernel is
launched here."""
import copy
import pickle

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import pointwise_cases as pc
from optest import lib, pkg      # noqa: F401  (fixtures)


N = 250000


@pytest.mark.parametrize("dtype", [np.float32, np.float16])
def test_twin_equals_torch_cpu_operators_bit_for_bit(dtype):
    """The seven exact kinds on 250 000 values (uniform, 1e-3-scale, +-0, +-3, +-6, +-1e30, +-65504, +-inf, NaN): integer
    views equal wherever the result is not a NaN, NaNs in the same positions.  PReLU with 1 and with C parameters."""
    rng = np.random.default_rng(1)
    Cn = 5
    x = pc.values(rng, (Cn, 100, N // (Cn * 100)), dtype)
    assert np.isnan(x).any() and np.isinf(x).any() and (pc.bits_of(x) == pc.bits_of(np.array([-0.0], dtype))[0]).any()
    t = torch.from_numpy(x)[None]
    slopeC = rng.uniform(-0.5, 0.5, Cn).astype(dtype)      # (a weight in the map's dtype converts to f32 exactly)
    slope1 = slopeC[:1]
    ops = [("ReLU", pc.RELU, {}, lambda: F.relu(t)),
           ("ReLU6", pc.HARDTANH, dict(p0=0.0, p1=6.0), lambda: F.relu6(t)),
           ("Hardtanh", pc.HARDTANH, dict(p0=-1.5, p1=2.25), lambda: F.hardtanh(t, -1.5, 2.25)),
           ("LeakyReLU", pc.LEAKY, dict(p0=0.01), lambda: F.leaky_relu(t, 0.01)),
           ("LeakyReLU 0.2", pc.LEAKY, dict(p0=0.2), lambda: F.leaky_relu(t, 0.2)),
           ("PReLU C", pc.PRELU, dict(slope=slopeC.astype(np.float32)), lambda: F.prelu(t, torch.from_numpy(slopeC))),
           ("PReLU 1", pc.PRELU, dict(slope=np.repeat(slope1, Cn).astype(np.float32)),
            lambda: F.prelu(t, torch.from_numpy(slope1))),
           ("Hardswish", pc.HARDSWISH, {}, lambda: F.hardswish(t)),
           ("Hardsigmoid", pc.HARDSIGMOID, {}, lambda: F.hardsigmoid(t)),
           ("Identity", pc.IDENTITY, {}, lambda: t.clone())]
    for name, kind, kw, op in ops:
        want = op()[0].numpy()
        got = pc.twin(x, kind, **kw)
        assert got.dtype == want.dtype == dtype
        nan = np.isnan(want)
        bad = (np.isnan(got) != nan) | ((pc.bits_of(got) != pc.bits_of(want)) & ~nan)
        assert not bad.any(), (name, int(bad.sum()), x[bad][:5], got[bad][:5], want[bad][:5])


def test_transcendental_twins_are_close_to_float64():
    """SIGMOID / SILU / TANH of the twin (numpy float32) against the float64 formula: a sanity check of the formulas
    with a loose bar of 1e-6 relative -- the bound that binds the KERNEL is derived in tests/test_gpu_pointwise.py."""
    rng = np.random.default_rng(2)
    x = rng.uniform(-20, 20, (3, 40, 50)).astype(np.float32)
    for kind, _, _ in pc.INEXACT:
        got, ref = pc.twin(x, kind).astype(np.float64), pc.reference64(x, kind)
        assert np.all(np.abs(got - ref) <= 1e-6 * np.abs(ref) + 2.0 ** -126), pc.NAMES[kind]


def _bn(Cn, affine, seed, eps=1e-3):
    g = torch.Generator().manual_seed(seed)
    bn = nn.BatchNorm2d(Cn, eps=eps, affine=affine)
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(Cn, generator=g))
        bn.running_var.copy_(torch.rand(Cn, generator=g) * 2 + 0.05)
        if affine:
            bn.weight.copy_(torch.randn(Cn, generator=g))
            bn.bias.copy_(torch.randn(Cn, generator=g))
    return bn.eval()


@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("dtype", [np.float32, np.float16])
def test_affine_of_the_twin_against_a_float64_batch_norm(pkg, dtype, affine):
    """CBPointwise2d's buffers are pc.bn_affine of the module's statistics, bit for bit; the twin's two-rounding affine
    against the eval-mode batch norm evaluated in float64: |err| <= 4 2^-24 (|x scale| + |shift|) -- the four roundings
    (scale, shift, product, sum) give at most 3 to first order, one more covers the higher-order terms --, for fp16 plus
    2^-11 |ref| + 2^-24.  And the two-rounding affine differs from a fused one on these inputs: only then can the GPU
    bit-identity test catch a contracted FMA."""
    rng = np.random.default_rng(3)
    Cn = 7
    bn = _bn(Cn, affine, 4)
    m = pkg.CBPointwise2d(norm=bn)
    gamma = bn.weight.detach().numpy() if affine else np.ones(Cn, dtype=np.float32)
    beta = bn.bias.detach().numpy() if affine else np.zeros(Cn, dtype=np.float32)
    scale, shift = pc.bn_affine(gamma, beta, bn.running_mean.numpy(), bn.running_var.numpy(), bn.eps)
    assert m.scale.dtype == torch.float32 and m.slope is None and m.kind == pc.IDENTITY
    assert np.array_equal(pc.bits_of(m.scale.numpy()), pc.bits_of(scale))
    assert np.array_equal(pc.bits_of(m.shift.numpy()), pc.bits_of(shift))
    x = rng.uniform(-8, 8, (Cn, 30, 40)).astype(dtype)
    got = pc.twin(x, pc.IDENTITY, scale=scale, shift=shift).astype(np.float64)
    with torch.no_grad():
        ref = copy.deepcopy(bn).double()(torch.from_numpy(x.astype(np.float64))[None])[0].numpy()
    x64, s64, h64 = x.astype(np.float64), scale.astype(np.float64)[:, None, None], shift.astype(np.float64)[:, None, None]
    bound = 4 * 2.0 ** -24 * (np.abs(x64 * s64) + np.abs(h64))
    if dtype == np.float16:
        bound = bound + 2.0 ** -11 * np.abs(ref) + 2.0 ** -24
    err = np.abs(got - ref)
    print("affine vs float64 batch norm (%s): max err / bound %.3f" % (np.dtype(dtype).name, float((err / bound).max())))
    assert np.all(err <= bound)
    fused = (x64 * s64 + h64).astype(np.float32)      # (exact in float64: 24 + 24 bits, then one rounding -- an FMA)
    two = pc.twin(x.astype(np.float32), pc.IDENTITY, scale=scale, shift=shift)
    differ = float((pc.bits_of(fused) != pc.bits_of(two)).mean())
    print("two-rounding affine differs from a fused one in %.1f %% of the values" % (100 * differ))
    assert differ > 0.01


def test_c_entry_points_check_their_arguments(lib):
    """Bad arguments return CB_ERR_BADARG (-1) before anything is launched (the pointers here are never followed)."""
    C = lib.C
    assert C.cbinfer_abi_version() == 11
    X, O, BITS, COPY, M, L, S1, S2, S3 = (0x1000 * i for i in range(1, 10))

    def fwd(x=X, o=O, mask=None, lst=None, cap=0, count=None, bits=BITS, cp=COPY, Cn=3, H=4, W=5, kind=pc.RELU, p0=0.0,
            p1=0.0, scale=None, shift=None, slope=None, dt=lib.CB_F32):
        return C.cbinfer_cbpointwise_forward(x, o, mask, lst, cap, count, bits, cp, Cn, H, W, kind, p0, p1, scale, shift,
                                             slope, dt, None)

    def chg(x=X, o=O, mask=None, bits=BITS, cp=COPY, Cn=3, H=4, W=5, kind=pc.HARDTANH, p0=0.0, p1=6.0, scale=None,
            shift=None, slope=None, dt=lib.CB_F16):
        return C.cbinfer_pointwise_changed(x, o, mask, 0, bits, cp, Cn, H, W, kind, p0, p1, scale, shift, slope, dt, None)

    for call in (fwd, chg):
        for bad in (dict(x=None), dict(o=None), dict(o=X), dict(bits=None), dict(cp=None), dict(cp=BITS), dict(mask=BITS),
                    dict(mask=COPY), dict(Cn=0), dict(H=0), dict(W=-1), dict(dt=lib.CB_F32S), dict(dt=7), dict(kind=-1),
                    dict(kind=10), dict(kind=pc.HARDTANH, p0=1.0, p1=0.5), dict(kind=pc.HARDTANH, p0=float('nan'), p1=1.0),
                    dict(kind=pc.PRELU), dict(scale=S1), dict(shift=S2), dict(H=1 << 16, W=1 << 15), dict(Cn=1 << 25)):
            assert call(**bad) == -1, (call.__name__, bad)
    for bad in (dict(lst=L, cap=-1), dict(mask=M, lst=L, cap=1), dict(count=L)):
        assert fwd(**bad) == -1, bad
    sup = C.cbinfer_pointwise_supported
    assert all(sup(k, 0.0, 0.0) == 1 for k in range(10)) and sup(10, 0.0, 0.0) == 0 and sup(-1, 0.0, 0.0) == 0
    assert sup(pc.HARDTANH, -1.0, -1.0) == 1 and sup(pc.HARDTANH, 0.5, 0.25) == 0
    assert sup(pc.LEAKY, 2.0, 1.0) == 1      # (p0 > p1 matters to HARDTANH only)
    assert [getattr(lib, "PW_" + n) for n in pc.NAMES] == list(range(10))


def test_constructor_takes_the_table_and_refuses_the_rest(pkg, lib):
    Err = lib.CBinferError
    table = [(nn.ReLU(inplace=True), pc.RELU, 0.0, 0.0), (nn.ReLU6(), pc.HARDTANH, 0.0, 6.0),
             (nn.Hardtanh(-1.5, 2.25), pc.HARDTANH, -1.5, 2.25), (nn.LeakyReLU(0.2), pc.LEAKY, 0.2, 0.0),
             (nn.PReLU(), pc.PRELU, 0.0, 0.0), (nn.PReLU(4), pc.PRELU, 0.0, 0.0), (nn.Hardswish(), pc.HARDSWISH, 0.0, 0.0),
             (nn.Hardsigmoid(), pc.HARDSIGMOID, 0.0, 0.0), (nn.Sigmoid(), pc.SIGMOID, 0.0, 0.0),
             (nn.SiLU(), pc.SILU, 0.0, 0.0), (nn.Tanh(), pc.TANH, 0.0, 0.0)]
    for act, kind, p0, p1 in table:
        m = pkg.CBPointwise2d(act)
        assert (m.kind, m.p0, m.p1) == (kind, p0, p1) and m.scale is None and m.shift is None, act
        assert not m.propChangeIndexes and m.cloneOutput and m.outputState.numel() == 0
        assert (m.slope is not None) == (kind == pc.PRELU)
    pre = nn.PReLU(4)
    with torch.no_grad():
        pre.weight.copy_(torch.tensor([0.1, -0.2, 0.3, 0.4]))
    m = pkg.CBPointwise2d(act=pre, norm=_bn(4, True, 1))
    assert m.slope.dtype == torch.float32 and torch.equal(m.slope, pre.weight.detach()) and m.scale.numel() == 4
    with torch.no_grad():
        pre.weight.zero_()      # later edits of the source module are not followed
    assert float(m.slope[0]) == float(np.float32(0.1))
    assert set(dict(m.named_buffers())) == {'scale', 'shift', 'slope', 'outputState'}
    # .half() converts the state, the per-channel operands stay float32 bit for bit
    before = m.scale.clone()
    m.half()
    assert m.scale.dtype == torch.float32 and torch.equal(m.scale, before) and m.slope.dtype == torch.float32

    class MyReLU(nn.ReLU):
        pass
    for kw, what in ((dict(), "act=None and norm=None"), (dict(act=MyReLU()), "act=MyReLU is not supported"),
                     (dict(act=nn.GELU()), "act=GELU is not supported"), (dict(act=nn.ELU()), "act=ELU"),
                     (dict(act=nn.Softmax(dim=1)), "act=Softmax"), (dict(act=F.relu), "act=function"),
                     (dict(norm=nn.BatchNorm2d(3)), "training mode"),
                     (dict(norm=nn.BatchNorm2d(3, track_running_stats=False).eval()), "running statistics"),
                     (dict(norm=nn.GroupNorm(1, 3)), "norm=GroupNorm is not supported"),
                     (dict(norm=nn.BatchNorm1d(3).eval()), "norm=BatchNorm1d"),
                     (dict(act=nn.PReLU(3), norm=_bn(4, True, 1)), "act has 3 parameters, norm 4 features")):
        with pytest.raises(Err, match=what):
            pkg.CBPointwise2d(**kw)
    ht = nn.Hardtanh(-1.0, 1.0)
    ht.min_val, ht.max_val = 2.0, 1.0      # (torch's constructor refuses this itself)
    with pytest.raises(Err, match="min_val=2.0 is above max_val=1.0"):
        pkg.CBPointwise2d(ht)
    assert pkg.CBPointwise2d is pkg.pointwise.CBPointwise2d
    assert all(n in pkg.__all__ for n in ('CBPointwise2d', 'insertCBPointwise'))


def test_operand_checks_and_pickle(pkg, lib):
    m = pkg.CBPointwise2d(nn.LeakyReLU(0.1), _bn(4, True, 2))
    m.propChangeIndexes, m.cloneOutput = True, False
    x = torch.zeros(1, 4, 5, 6)
    for inp, what in ((torch.zeros(2, 4, 5, 6), r"\[1, C, H, W\]"), (torch.zeros(4, 5, 6), r"\[1, C, H, W\]"),
                      (('changeIndexes', x), "tuple"), (None, "must be a tensor"), (x.double(), "float32 and float16"),
                      (torch.zeros(1, 3, 5, 6), "the input has 3 channels, scale was made for 4"),
                      (x, "HIP devices only")):
        with pytest.raises(lib.CBinferError, match=what):
            m(inp)
    with pytest.raises(lib.CBinferError, match="the input has 3 channels, slope was made for 4"):
        pkg.CBPointwise2d(nn.PReLU(4))(torch.zeros(1, 3, 5, 6))
    m.__dict__['_pwWork'] = {'key': None}
    c = pickle.loads(pickle.dumps(m))
    assert type(c) is pkg.CBPointwise2d and (c.kind, c.p0, c.propChangeIndexes, c.cloneOutput) == (pc.LEAKY, 0.1, True, False)
    assert c._pwWork is None and c.outputState.numel() == 0 and repr(c) == repr(m) and 'act=LeakyReLU' in repr(c)
    assert torch.equal(c.scale, m.scale) and torch.equal(c.shift, m.shift) and c.slope is None
    # the state helpers reach the module
    m.outputState = torch.ones(1, 4, 3, 3)
    net = nn.Sequential(m)
    assert any(t is m.outputState for t in pkg.getStateTensors(net))
    pkg.clearMemory(net)
    assert m.outputState.numel() == 0 and m._pwWork is None


def _names(seq):
    return [(n, type(m).__name__) for n, m in seq.named_children()]


def test_insert_on_a_mobilenetv3_type_block(pkg, lib):
    """1x1 expand -> BN -> Hardswish -> 3x3 depthwise -> BN -> Hardswish -> 1x1 project (the batch norms behind the
    convolutions folded by foldBatchNorm), then a GELU, a batch norm behind it, a 3x3 head and a Sigmoid."""
    torch.manual_seed(1)
    src = nn.Sequential()
    for name, mod in (('expand', nn.Conv2d(8, 16, 1, bias=False)), ('bn1', _bn(16, True, 1)), ('hs1', nn.Hardswish()),
                      ('dw', nn.Conv2d(16, 16, 3, 1, 1, groups=16)), ('bn2', _bn(16, True, 2)),
                      ('hs2', nn.Hardswish(inplace=True)), ('project', nn.Conv2d(16, 8, 1)), ('gelu', nn.GELU()),
                      ('bn3', _bn(8, True, 3)), ('head', nn.Conv2d(8, 4, 3, padding=1)), ('out', nn.Sigmoid())):
        src.add_module(name, mod)
    src.eval()
    net = pkg.convert(pkg.foldBatchNorm(src), threshold=0.05, generalGeometry=True, depthwise=True)
    assert pkg.insertCBPointwise(net) is net
    assert _names(net) == [('expand', 'CBConv2d'), ('hs1', 'CBPointwise2d'), ('dw', 'CBDepthwiseConv2d'),
                           ('hs2', 'CBPointwise2d'), ('project', 'CBConv2d'), ('gelu', 'GELU'), ('bn3', 'BatchNorm2d'),
                           ('head', 'CBConv2d'), ('out', 'CBPointwise2d')]
    assert net.expand.propChangeIndexes and net.dw.propChangeIndexes and net.head.propChangeIndexes
    assert not net.project.propChangeIndexes      # (the GELU behind it stays dense, and so does the BN behind that)
    assert net.hs1.kind == pc.HARDSWISH and net.hs1.scale is None
    assert net.hs2.kind == pc.HARDSWISH and net.hs2.scale is None
    assert net.out.kind == pc.SIGMOID
    # only the module in front of a 1x1 / stride-1 / padding-0 CBConv2d hands its changes on by itself ...
    assert net.hs2.propChangeIndexes and not net.hs1.propChangeIndexes and not net.out.propChangeIndexes
    # ... linkDepthwise switches the flag on for its own consumer
    assert not net.dw.propagatedChanges
    pkg.linkDepthwise(net)
    assert net.dw.propagatedChanges and net.hs1.propChangeIndexes
    # a second pass finds nothing more to do
    before = _names(net)
    pkg.insertCBPointwise(net)
    assert _names(net) == before


def test_insert_on_a_pre_activation_type_block(pkg, lib):
    """BN -> ReLU -> conv of a pre-activation ResNet inside a CBResidual's body, a BN + PReLU behind the sum, a BN alone
    behind a pool, a LeakyReLU behind a k x k consumer, runs behind dense modules."""
    torch.manual_seed(2)
    body = pkg.convert(nn.Sequential(nn.Conv2d(8, 8, 3, padding=1), nn.ReLU(), nn.Conv2d(8, 8, 3, padding=1)).eval(),
                       threshold=0.05)
    net = nn.Sequential()
    for name, mod in (('stem', nn.Conv2d(3, 8, 3, padding=1)), ('bn0', _bn(8, True, 1)), ('relu0', nn.ReLU()),
                      ('pool', nn.MaxPool2d(3, 2, 1)), ('bnp', _bn(8, False, 2)), ('conv1', nn.Conv2d(8, 8, 3, padding=1)),
                      ('lrelu', nn.LeakyReLU(0.1)), ('conv2', nn.Conv2d(8, 8, 3, padding=1)), ('drop', nn.Identity()),
                      ('tanh', nn.Tanh())):
        net.add_module(name, mod)
    net = pkg.convert(net.eval(), threshold=0.05)
    assert _names(net)[:3] == [('stem', 'CBConv2d'), ('bn0', 'BatchNorm2d'), ('relu0', 'ReLU')]
    pkg.insertCBPooling(net, generalGeometry=True)      # (a pool behind a dense ReLU: stays dense)
    assert type(net.pool) is nn.MaxPool2d
    net.add_module('block', pkg.CBResidual(body, relu=False))
    net.add_module('bnb', _bn(8, True, 3))
    net.add_module('prelu', nn.PReLU(8))
    net.add_module('last', pkg.convert(nn.Sequential(nn.Conv2d(8, 4, 1)).eval(), threshold=0.05)[0])
    pkg.insertCBPointwise(net)
    assert _names(net) == [('stem', 'CBConv2d'), ('bn0', 'CBPointwise2d'), ('pool', 'MaxPool2d'), ('bnp', 'BatchNorm2d'),
                           ('conv1', 'CBConv2d'), ('lrelu', 'CBPointwise2d'), ('conv2', 'CBConv2d'), ('drop', 'Identity'),
                           ('tanh', 'Tanh'), ('block', 'CBResidual'), ('bnb', 'CBPointwise2d'), ('last', 'CBConv2d')]
    assert net.bn0.kind == pc.RELU and net.bn0.scale is not None and net.stem.propChangeIndexes
    assert net.lrelu.kind == pc.LEAKY and net.lrelu.p0 == 0.1 and net.conv1.propChangeIndexes
    assert not net.lrelu.propChangeIndexes      # (conv2 is 3x3: it must run its own detection)
    assert not net.conv2.propChangeIndexes      # (an nn.Identity in between: the Tanh is not directly behind)
    assert net.block.add.propChangeIndexes and net.bnb.kind == pc.PRELU and net.bnb.slope.numel() == 8
    assert net.bnb.propChangeIndexes      # (`last` is a 1x1 / stride-1 / padding-0 CBConv2d)
    assert not net.bn0.propChangeIndexes      # (a dense pool behind it)
    # now the general pools: the pool behind the new module is converted and fed by its mask
    pkg.insertCBPooling(net, generalGeometry=True)
    assert type(net.pool) is pkg.CBPoolMax2d and net.pool._general and net.bn0.propChangeIndexes
    pkg.insertCBPointwise(net)
    assert type(net.bnp) is pkg.CBPointwise2d and net.bnp.kind == pc.IDENTITY and net.pool.propChangeIndexes
    # a batch norm in training mode stops the pass with a sentence, as foldBatchNorm does
    bad = nn.Sequential(pkg.convert(nn.Sequential(nn.Conv2d(3, 4, 1)).eval(), threshold=0.05)[0], nn.BatchNorm2d(4))
    with pytest.raises(lib.CBinferError, match="training mode"):
        pkg.insertCBPointwise(bad)
    # a 2x2 pool of the reference's kind hands on the list of ITS map
    seq = pkg.insertCBPooling(pkg.convert(nn.Sequential(nn.Conv2d(3, 4, 3, padding=1), nn.MaxPool2d(2, 2), nn.SiLU()).eval(),
                                          threshold=0.05))
    pkg.insertCBPointwise(seq)
    assert type(seq[2]) is pkg.CBPointwise2d and seq[1].propChangeIndexes and seq[1].downsampleIndexes


def test_the_class_is_in_the_producer_lists(pkg):
    from cbinfer_amd import chain
    P = pkg.CBPointwise2d
    every = (pkg.CBConv2d, pkg.CBPoolMax2d, pkg.CBPoolAvg2d, pkg.CBAdd2d, pkg.CBResidual, pkg.CBUpsample2d,
             pkg.CBConvTranspose2d, pkg.CBDepthwiseConv2d, P)
    # ONE set for linkDepthwise, insertCBPointwise and insertCBTransposedConv; insertCBUpsampling's is the same but
    # for the transposed convolution; a CBConcat2d is in none (every pass's whole set, in order: test_host_chain.py)
    one = chain.producers('linkDepthwise')
    assert one == chain.producers('insertCBPointwise') == chain.producers('insertCBTransposedConv')
    assert one[:len(every)] == every
    assert chain.producers('insertCBUpsampling') == tuple(t for t in one if t is not pkg.CBConvTranspose2d)
    assert not any(pkg.CBConcat2d in chain.producers(name) for name in chain.PASSES)
    # ... and no module keeps a list of its own that another could extend on import
    for mod in ('decoder', 'tconv', 'dwconv', 'pointwise'):
        assert not [n for n in vars(getattr(__import__('cbinfer_amd.' + mod), mod)) if n.endswith('PRODUCERS')]
    # the passes take it as a producer
    pw = lambda: pkg.CBPointwise2d(nn.SiLU())      # noqa: E731
    seq = pkg.insertCBUpsampling(nn.Sequential(pw(), nn.Upsample(scale_factor=2, mode='nearest')))
    assert type(seq[1]) is pkg.CBUpsample2d and seq[0].propChangeIndexes
    seq = pkg.insertCBTransposedConv(nn.Sequential(pw(), nn.ConvTranspose2d(4, 4, 2, 2).eval()))
    assert type(seq[1]) is pkg.CBConvTranspose2d      # (the layer detects for itself: no flag at the producer)
    dw = pkg.convert(nn.Sequential(nn.Conv2d(4, 4, 3, padding=1, groups=4)).eval(), depthwise=True)[0]
    seq = pkg.linkDepthwise(nn.Sequential(pw(), dw))
    assert dw.propagatedChanges and seq[0].propChangeIndexes
    seq = pkg.insertCBPooling(nn.Sequential(pw(), nn.AvgPool2d(2, 2)), generalGeometry=True)
    assert type(seq[1]) is pkg.CBPoolAvg2d and seq[0].propChangeIndexes
    seq = pkg.insertCBPooling(nn.Sequential(pw(), nn.MaxPool2d(2, 2)))      # (the reference's pool wants a list: as before)
    assert type(seq[1]) is nn.MaxPool2d and not seq[0].propChangeIndexes


def test_batch_and_branch_refusals_name_the_layer(pkg, lib):
    net = pkg.convert(nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), nn.Hardswish()).eval(), threshold=0.05)
    pkg.insertCBPointwise(net)
    with pytest.raises(lib.CBinferError, match=r"SequenceBatch: layer '1' is CBPointwise2d \(act=Hardswish"):
        pkg.SequenceBatch(net, 2)
    with pytest.raises(lib.CBinferError, match=r"BranchGroup: layer '0.1' is CBPointwise2d"):
        pkg.BranchGroup([net])
