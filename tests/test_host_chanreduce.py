"""CPU-only tests of the change-based per-pixel channel reductions: the numpy twin of
tests/chanreduce_cases.py against the float64 formulas under the derived bounds, the float64 formulas against torch's CPU
operators in double, sum16's independence of the other pixels, the argument checks of the C entry points, the
constructor's refusals, insertCBChannelOps' structure, pickling and the refusals.  No kernel is launched here."""
import pickle

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import chanreduce_cases as cc
from optest import lib, pkg      # noqa: F401  (fixtures)


class LayerNorm2d(nn.Module):
    """A channels-first layer norm as ConvNeXt implementations write it: .weight, .bias, .eps (torch has no such class)."""

    def __init__(self, C, eps=1e-6, affine=True):
        super(LayerNorm2d, self).__init__()
        self.weight = nn.Parameter(torch.linspace(0.5, 1.5, C)) if affine else None
        self.bias = nn.Parameter(torch.linspace(-0.3, 0.4, C)) if affine else None
        self.eps, self.C = eps, C

    def forward(self, x):
        return F.layer_norm(x.permute(0, 2, 3, 1), (self.C,), self.weight, self.bias, self.eps).permute(0, 3, 1, 2)


CHANNELS = [1, 2, 3, 15, 16, 17, 40, 300, 1024]
DISTS = [("uniform +-8", lambda rng, s: rng.uniform(-8, 8, s)), ("+-1e-3", lambda rng, s: rng.uniform(-1e-3, 1e-3, s)),
         ("100 +- 0.5", lambda rng, s: 100 + rng.uniform(-0.5, 0.5, s)), ("3 +- 8", lambda rng, s: 3 + rng.uniform(-8, 8, s))]


@pytest.mark.parametrize("dtype", [np.float32, np.float16], ids=["f32", "f16"])
def test_twin_against_float64_under_the_bounds(dtype):
    """The float32 twin against the float64 formula on the stored inputs, every kind (LAYERNORM with and without the
    affine), C below, at and over the 16 slices, four distributions -- 100 +- 0.5 is LayerNorm's cancellation case --
    under chanreduce_cases.bound (derived there).  The bounds are not tuned: a failure is a finding.  The worst
    err / bound per kind is printed."""
    rng = np.random.default_rng(1)
    worst = {}
    for Cn in CHANNELS:
        gamma, beta = cc.affine(rng, Cn)
        for dname, dist in DISTS:
            x = dist(rng, (Cn, 150)).astype(dtype)
            for kind, aff in ((cc.LAYERNORM, False), (cc.LAYERNORM, True), (cc.L2NORM, False), (cc.SOFTMAX, False),
                              (cc.LOGSOFTMAX, False)):
                kw = dict(gamma=gamma, beta=beta) if aff else {}
                got = cc.twin(x, kind, **kw)
                assert got.dtype == dtype
                ref = cc.reference64(x, kind, **kw)
                b = cc.bound(x, kind, ref, **kw)
                err = np.abs(got.astype(np.float64) - ref)
                key = cc.NAMES[kind] + (" affine" if aff else "")
                worst[key] = max(worst.get(key, 0.0), float((err / b).max()))
                assert np.all(err <= b), (key, Cn, dname, float((err / b).max()))
    for key, w in sorted(worst.items()):
        print("%-18s %s worst err / bound = %.3f" % (key, np.dtype(dtype).name, w))


def test_float64_formulas_are_torchs_operators():
    """reference64 against torch's CPU operators in double -- F.layer_norm on the permuted map, F.softmax,
    F.log_softmax, F.normalize -- to 1e-12: this ties the specification to torch's meaning."""
    rng = np.random.default_rng(2)
    for Cn in (1, 3, 17, 40):
        x = rng.uniform(-8, 8, (Cn, 6, 11)).astype(np.float32)
        t = torch.from_numpy(x).double()[None]
        gamma, beta = cc.affine(rng, Cn)
        g, b = torch.from_numpy(gamma).double(), torch.from_numpy(beta).double()
        eps = float(np.float32(1e-6))
        ops = [(cc.LAYERNORM, dict(eps=1e-6), F.layer_norm(t.permute(0, 2, 3, 1), (Cn,), None, None, eps).permute(0, 3, 1, 2)),
               (cc.LAYERNORM, dict(eps=1e-6, gamma=gamma, beta=beta),
                F.layer_norm(t.permute(0, 2, 3, 1), (Cn,), g, b, eps).permute(0, 3, 1, 2)),
               (cc.L2NORM, dict(eps=1e-12), F.normalize(t, p=2.0, dim=1, eps=float(np.float32(1e-12)))),
               (cc.L2NORM, dict(eps=50.0), F.normalize(t, p=2.0, dim=1, eps=50.0)),      # (the clamp is reached)
               (cc.SOFTMAX, {}, F.softmax(t, 1)), (cc.LOGSOFTMAX, {}, F.log_softmax(t, 1))]
        for kind, kw, want in ops:
            ref = cc.reference64(x, kind, **kw)
            assert np.abs(ref - want[0].numpy()).max() <= 1e-12, (cc.NAMES[kind], Cn)


def test_sum16_of_a_pixel_is_independent_of_the_other_pixels():
    """sum16 / max16 of one column alone and inside an array of other pixels: the same bits; and the order matters --
    sum16 is not numpy's pairwise sum on these inputs, so a kernel with another order would be caught."""
    rng = np.random.default_rng(3)
    for Cn in (1, 15, 16, 17, 300):
        v = (rng.uniform(-8, 8, (Cn, 40))).astype(np.float32)
        whole, wholeMax = cc.sum16(v), cc.max16(v)
        for p in (0, 7, 39):
            alone = v[:, p:p + 1].copy()
            assert cc.bits_of(cc.sum16(alone))[0] == cc.bits_of(whole)[p]
            assert cc.bits_of(cc.max16(alone))[0] == cc.bits_of(wholeMax)[p]
        assert np.array_equal(wholeMax, v.max(axis=0))
        assert np.abs(whole.astype(np.float64) - v.astype(np.float64).sum(axis=0)).max() <= 1e-3
    v = rng.uniform(-8, 8, (300, 4000)).astype(np.float32)
    plain = np.zeros(4000, dtype=np.float32)
    for c in range(300):
        plain = plain + v[c]
    assert (cc.bits_of(cc.sum16(v)) != cc.bits_of(plain)).mean() > 0.2
    # an empty slice contributes +0 / -inf: C = 3 leaves 13 of them
    assert cc.sum16(np.array([[1.0], [2.0], [4.0]], dtype=np.float32))[0] == 7.0
    assert cc.max16(np.array([[-5.0], [np.nan], [-7.0]], dtype=np.float32))[0] == -5.0      # (a NaN is never taken)


def test_c_entry_points_check_their_arguments(lib):
    """Bad arguments return CB_ERR_BADARG (-1) before anything is launched (the pointers here are never followed)."""
    C = lib.C
    X, O, BITS, COPY, M, L, G, B = (0x1000 * i for i in range(1, 9))

    def fwd(x=X, o=O, mask=None, lst=None, cap=0, count=None, bits=BITS, cp=COPY, Cn=3, H=4, W=5, kind=cc.SOFTMAX,
            eps=0.0, gamma=None, beta=None, dt=lib.CB_F32):
        return C.cbinfer_cbchanreduce_forward(x, o, mask, lst, cap, count, bits, cp, Cn, H, W, kind, eps, gamma, beta, dt,
                                              None)

    def chg(x=X, o=O, mask=None, bits=BITS, cp=COPY, Cn=3, H=4, W=5, kind=cc.LAYERNORM, eps=1e-6, gamma=None, beta=None,
            dt=lib.CB_F16):
        return C.cbinfer_chanreduce_changed(x, o, mask, 0, bits, cp, Cn, H, W, kind, eps, gamma, beta, dt, None)

    for call in (fwd, chg):
        for bad in (dict(x=None), dict(o=None), dict(o=X), dict(bits=None), dict(cp=None), dict(cp=BITS), dict(mask=BITS),
                    dict(mask=COPY), dict(Cn=0), dict(H=0), dict(W=-1), dict(dt=lib.CB_F32S), dict(dt=7), dict(kind=-1),
                    dict(kind=4), dict(eps=-1e-6), dict(eps=float('nan')), dict(kind=cc.LAYERNORM, gamma=G),
                    dict(kind=cc.LAYERNORM, beta=B), dict(kind=cc.SOFTMAX, gamma=G, beta=B),
                    dict(kind=cc.L2NORM, gamma=G, beta=B), dict(H=1 << 16, W=1 << 15), dict(Cn=1 << 25)):
            assert call(**bad) == -1, (call.__name__, bad)
    for bad in (dict(lst=L, cap=-1), dict(mask=M, lst=L, cap=1), dict(count=L)):
        assert fwd(**bad) == -1, bad
    sup = C.cbinfer_chanreduce_supported
    assert all(sup(k, 1, 0.0) == 1 and sup(k, 2048, 1e-5) == 1 and sup(k, 1 << 20, 1.0) == 1 for k in range(4))
    assert sup(4, 8, 0.0) == 0 and sup(-1, 8, 0.0) == 0 and sup(0, 0, 0.0) == 0
    assert sup(0, 8, -1e-9) == 0 and sup(0, 8, float('nan')) == 0 and sup(0, 8, float('inf')) == 1
    assert [getattr(lib, "CH_" + n) for n in cc.NAMES] == list(range(4))
    assert C.cbinfer_cbchanreduce_forward.launcher and C.cbinfer_chanreduce_changed.launcher
    assert not C.cbinfer_chanreduce_supported.launcher
    assert C.cbinfer_abi_version() == 11


def test_constructor_takes_the_table_and_refuses_the_rest(pkg, lib):
    Err = lib.CBinferError
    table = [(nn.Softmax2d(), cc.SOFTMAX), (nn.Softmax(dim=1), cc.SOFTMAX), (nn.Softmax(dim=-3), cc.SOFTMAX),
             (nn.LogSoftmax(dim=1), cc.LOGSOFTMAX), (nn.LogSoftmax(dim=-3), cc.LOGSOFTMAX)]
    for op, kind in table:
        m = pkg.CBChannelReduce2d(op)
        assert m.kind == kind and m.eps == 0.0 and m.gamma is None and m.beta is None, op
        assert not m.propChangeIndexes and m.cloneOutput and m.outputState.numel() == 0
    m = pkg.CBChannelReduce2d('l2norm')
    assert m.kind == cc.L2NORM and m.eps == float(np.float32(1e-12)) and m.gamma is None
    assert pkg.CBChannelReduce2d('l2norm', eps=1e-6).eps == float(np.float32(1e-6))
    ln = nn.LayerNorm(4, eps=1e-5)
    with torch.no_grad():
        ln.weight.copy_(torch.tensor([0.5, -1.0, 2.0, 1.5]))
        ln.bias.copy_(torch.tensor([0.1, 0.2, -0.3, 0.0]))
    m = pkg.CBChannelReduce2d(ln)
    assert m.kind == cc.LAYERNORM and m.eps == float(np.float32(1e-5)) and m.gamma.dtype == torch.float32
    assert torch.equal(m.gamma, ln.weight.detach()) and torch.equal(m.beta, ln.bias.detach())
    with torch.no_grad():
        ln.weight.zero_()      # later edits of the source module are not followed
    assert float(m.gamma[0]) == 0.5
    assert set(dict(m.named_buffers())) == {'gamma', 'beta', 'outputState'}
    plain = pkg.CBChannelReduce2d(nn.LayerNorm(4, elementwise_affine=False), eps=1e-3)
    assert plain.gamma is None and plain.beta is None and plain.eps == float(np.float32(1e-3))
    own = pkg.CBChannelReduce2d(LayerNorm2d(6), layerNormTypes=(LayerNorm2d,))
    assert own.kind == cc.LAYERNORM and own.gamma.numel() == 6 and own.eps == float(np.float32(1e-6))

    class MySoftmax(nn.Softmax):
        pass

    class MyLayerNorm(nn.LayerNorm):
        pass
    for args, what in (((nn.Softmax(dim=0),), "dim=0"), ((nn.LogSoftmax(dim=2),), "dim=2"), ((nn.Softmax(),), "dim=None"),
                       ((nn.GroupNorm(1, 4),), "op=GroupNorm is not supported"),
                       ((nn.InstanceNorm2d(4),), "op=InstanceNorm2d is not supported"),
                       ((nn.LayerNorm((4, 5, 6)),), r"normalized_shape=\(4, 5, 6\)"),
                       ((MySoftmax(dim=1),), "op=MySoftmax is not supported"),
                       ((MyLayerNorm(4),), "op=MyLayerNorm is not supported"),
                       ((LayerNorm2d(4),), "op=LayerNorm2d is not supported"),
                       ((nn.LayerNorm(4, eps=-1e-5),), "eps=-1e-05"), (('l2norm', -1.0), "eps=-1.0"),
                       (('l2norm', float('nan')), "eps=nan"), ((nn.Softmax2d(), 1e-5), "eps=1e-05 given for op=Softmax2d"),
                       (('l1norm',), "op='l1norm' is not supported"), ((F.softmax,), "op=function is not supported")):
        with pytest.raises(Err, match=what):
            pkg.CBChannelReduce2d(*args)
    assert pkg.CBChannelReduce2d is pkg.chanreduce.CBChannelReduce2d
    assert all(n in pkg.__all__ for n in ('CBChannelReduce2d', 'insertCBChannelOps'))


def test_operand_checks_pickle_and_half(pkg, lib):
    m = pkg.CBChannelReduce2d(LayerNorm2d(4), layerNormTypes=(LayerNorm2d,))
    m.propChangeIndexes, m.cloneOutput = True, False
    x = torch.zeros(1, 4, 5, 6)
    for inp, what in ((torch.zeros(2, 4, 5, 6), r"\[1, C, H, W\]"), (torch.zeros(4, 5, 6), r"\[1, C, H, W\]"),
                      (('changeIndexes', x), "tuple"), (None, "must be a tensor"), (x.double(), "float32 and float16"),
                      (torch.zeros(1, 3, 5, 6), "the input has 3 channels, gamma was made for 4"),
                      (x, "HIP devices only")):
        with pytest.raises(lib.CBinferError, match=what):
            m(inp)
    m.__dict__['_chWork'] = {'key': None}
    c = pickle.loads(pickle.dumps(m))
    assert type(c) is pkg.CBChannelReduce2d and (c.kind, c.eps, c.propChangeIndexes, c.cloneOutput) == (
        cc.LAYERNORM, m.eps, True, False)
    assert c._chWork is None and c.outputState.numel() == 0 and repr(c) == repr(m) and 'op=LayerNorm2d' in repr(c)
    assert torch.equal(c.gamma, m.gamma) and torch.equal(c.beta, m.beta)
    # .half() converts the state, gamma / beta stay float32 bit for bit
    before = m.gamma.clone()
    m.outputState = torch.ones(1, 4, 3, 3)
    m.half()
    assert m.gamma.dtype == torch.float32 and torch.equal(m.gamma, before) and m.beta.dtype == torch.float32
    assert m.outputState.dtype == torch.float16
    # the state helpers reach the module
    net = nn.Sequential(m)
    assert any(t is m.outputState for t in pkg.getStateTensors(net))
    pkg.clearMemory(net)
    assert m.outputState.numel() == 0 and m._chWork is None


def _names(seq):
    return [(n, type(m).__name__) for n, m in seq.named_children()]


def test_insert_on_a_convnext_type_block_and_a_segmentation_head(pkg, lib):
    """1x1 -> 7x7 depthwise -> LayerNorm2d -> 1x1 -> GELU -> LayerNorm2d -> 3x3 head -> Softmax2d, and a head whose
    log-softmax feeds a 3x3 layer."""
    torch.manual_seed(1)
    src = nn.Sequential()
    for name, mod in (('stem', nn.Conv2d(8, 16, 1)), ('dw', nn.Conv2d(16, 16, 7, 1, 3, groups=16)),
                      ('norm', LayerNorm2d(16)), ('pw1', nn.Conv2d(16, 32, 1)), ('gelu', nn.GELU()),
                      ('norm2', LayerNorm2d(32)), ('head', nn.Conv2d(32, 5, 3, padding=1)), ('prob', nn.Softmax2d())):
        src.add_module(name, mod)
    net = pkg.convert(src.eval(), threshold=0.05, depthwise=True)
    # without the user's class named, only the softmax is taken
    assert pkg.insertCBChannelOps(net) is net
    assert _names(net) == [('stem', 'CBConv2d'), ('dw', 'CBDepthwiseConv2d'), ('norm', 'LayerNorm2d'), ('pw1', 'CBConv2d'),
                           ('gelu', 'GELU'), ('norm2', 'LayerNorm2d'), ('head', 'CBConv2d'), ('prob', 'CBChannelReduce2d')]
    assert net.head.propChangeIndexes and not net.dw.propChangeIndexes and net.prob.kind == cc.SOFTMAX
    assert not net.prob.propChangeIndexes
    pkg.insertCBChannelOps(net, layerNormTypes=(LayerNorm2d,))
    assert _names(net)[2] == ('norm', 'CBChannelReduce2d') and _names(net)[5] == ('norm2', 'LayerNorm2d')
    assert net.norm.kind == cc.LAYERNORM and net.norm.gamma.numel() == 16 and net.dw.propChangeIndexes
    assert net.norm.eps == float(np.float32(1e-6))
    assert net.norm.propChangeIndexes      # (pw1 is a 1x1 / stride-1 / padding-0 CBConv2d)
    assert not net.pw1.propChangeIndexes      # (the GELU behind it stays dense, and the norm behind that)
    # a second pass finds nothing more to do
    before = _names(net)
    pkg.insertCBChannelOps(net, layerNormTypes=(LayerNorm2d,))
    assert _names(net) == before
    # linkDepthwise still links the depthwise layer to the layer in front of it
    pkg.linkDepthwise(net)
    assert net.dw.propagatedChanges and net.stem.propChangeIndexes

    seg = nn.Sequential()
    for name, mod in (('c1', nn.Conv2d(8, 6, 3, padding=1)), ('ln', LayerNorm2d(6, affine=False)),
                      ('lsm', nn.LogSoftmax(dim=1)), ('c2', nn.Conv2d(6, 4, 3, padding=1)), ('rows', nn.Softmax(dim=2)),
                      ('c3', nn.Conv2d(4, 4, 1)), ('gn', nn.GroupNorm(1, 4)), ('sm', nn.Softmax(dim=-3))):
        seg.add_module(name, mod)
    seg = pkg.convert(seg.eval(), threshold=0.05)
    seg.c2.copyInput = seg.c3.copyInput = False      # (a user's setting: the layer keeps a reference to its input)
    pkg.insertCBChannelOps(seg, layerNormTypes=[LayerNorm2d])
    assert _names(seg) == [('c1', 'CBConv2d'), ('ln', 'CBChannelReduce2d'), ('lsm', 'CBChannelReduce2d'),
                           ('c2', 'CBConv2d'), ('rows', 'Softmax'), ('c3', 'CBConv2d'), ('gn', 'GroupNorm'),
                           ('sm', 'Softmax')]
    assert seg.c1.propChangeIndexes and seg.ln.gamma is None and seg.ln.kind == cc.LAYERNORM
    assert seg.ln.propChangeIndexes      # (handed on to the module behind it, another CBChannelReduce2d)
    assert seg.lsm.kind == cc.LOGSOFTMAX and not seg.lsm.propChangeIndexes
    assert seg.c2.copyInput      # (a 3x3 layer behind a state that is handed out: it keeps its own input copy)
    assert not seg.c3.copyInput      # (not behind a new module: untouched)
    assert not seg.c2.propChangeIndexes      # (a softmax over the rows is no per-pixel operator: dense)
    assert not seg.c3.propChangeIndexes      # (GroupNorm reduces over the pixels as well; the softmax behind it is behind a dense module)


def test_batch_and_branch_refusals_name_the_layer(pkg, lib):
    net = pkg.convert(nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), nn.Softmax2d()).eval(), threshold=0.05)
    pkg.insertCBChannelOps(net)
    with pytest.raises(lib.CBinferError, match=r"SequenceBatch: layer '1' is CBChannelReduce2d \(op=Softmax2d"):
        pkg.SequenceBatch(net, 2)
    with pytest.raises(lib.CBinferError, match=r"BranchGroup: layer '0.1' is CBChannelReduce2d"):
        pkg.BranchGroup([net])
    # the new module is a producer for these passes and no other (every pass's whole set: test_host_chain.py)
    from cbinfer_amd import chain
    assert [name for name in chain.PASSES if pkg.CBChannelReduce2d in chain.producers(name)] == [
        'insertCBChannelOps', 'insertCBPadding', 'insertCBGating', 'insertCBResize']
