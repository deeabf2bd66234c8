"""CPU-only tests of the change-based reductions that collapse the channel axis: the numpy twin of
tests/chancollapse_cases.py against float64 under the derived bounds and against torch's CPU max / min, the argument
checks of the three C entry points, the constructor's refusals, pickling (also of a module from before these ops),
.half() and insertCBChannelOps(reduceTypes=...).  No kernel is launched here."""
import pickle

import numpy as np
import pytest
import torch
import torch.nn as nn

import chancollapse_cases as cc
import chanreduce_cases as cr
from optest import lib, pkg      # noqa: F401  (fixtures)


class ChannelPool(nn.Module):
    """CBAM's channel pooling, as its implementations write it (torch has no module for it)."""

    def forward(self, x):
        return torch.cat([x.amax(1, keepdim=True), x.mean(1, keepdim=True)], 1)


class ArgMax2d(nn.Module):
    def forward(self, x):
        return torch.argmax(x, 1, keepdim=True)


CHANNELS = [1, 2, 3, 15, 16, 17, 40, 300, 1024]
DISTS = [("uniform +-8", lambda rng, s: rng.uniform(-8, 8, s)), ("+-1e-3", lambda rng, s: rng.uniform(-1e-3, 1e-3, s)),
         ("100 +- 0.5", lambda rng, s: 100 + rng.uniform(-0.5, 0.5, s)), ("3 +- 8", lambda rng, s: 3 + rng.uniform(-8, 8, s))]


@pytest.mark.parametrize("dtype", [np.float32, np.float16], ids=["f32", "f16"])
def test_twin_against_float64_under_the_bounds(dtype):
    """SUM, MEAN and NORM of the float32 twin against the float64 formula on the stored inputs, C from 1 to 1024, the
    four distributions of the channel reductions' test, under chancollapse_cases.bound (derived there); a float16 sum
    beyond the format's range must be the infinity of its sign.  The bounds are not tuned: a failure is a finding.  The worst err / bound
    per kind is printed (DESIGN 5.27 reports it)."""
    rng = np.random.default_rng(1)
    worst = {}
    for Cn in CHANNELS:
        for dname, dist in DISTS:
            x = dist(rng, (Cn, 150)).astype(dtype)
            for kind in cc.FLOAT_KINDS:
                got = cc.twin(x, kind)
                assert got.dtype == dtype and got.shape == (150,)
                ref = cc.reference64(x, kind)
                b = cc.bound(x, kind, ref)
                # (a float16 sum beyond the format's range is an infinity: 1024 channels around 100 reach it)
                fin = np.abs(ref) + b < 65520.0 if dtype == np.float16 else np.isfinite(ref)
                over = np.abs(ref) - b >= 65520.0 if dtype == np.float16 else ~fin
                assert np.array_equal(got[over].astype(np.float64), np.sign(ref[over]) * np.inf)
                assert dtype == np.float16 or fin.all()
                err = np.abs(got.astype(np.float64)[fin] - ref[fin])
                if fin.any():
                    worst[cc.NAMES[kind]] = max(worst.get(cc.NAMES[kind], 0.0), float((err / b[fin]).max()))
                assert np.all(err <= b[fin]), (cc.NAMES[kind], Cn, dname, float((err / b[fin]).max()))
    for key, w in sorted(worst.items()):
        print("%-5s %s worst err / bound = %.3f" % (key, np.dtype(dtype).name, w))


def test_float_kinds_are_torchs_operators_and_sum16s_order():
    """reference64 against torch's CPU operators in double -- sum, mean, linalg.vector_norm over dim 1 -- to 1e-12; and
    the twin's SUM is sum16, not a plain running sum: another order would be caught."""
    rng = np.random.default_rng(2)
    for Cn in (1, 3, 17, 40):
        x = rng.uniform(-8, 8, (Cn, 6, 11)).astype(np.float32)
        t = torch.from_numpy(x).double()[None]
        for kind, want in ((cc.SUM, t.sum(1)), (cc.MEAN, t.mean(1)), (cc.NORM, torch.linalg.vector_norm(t, dim=1))):
            assert np.abs(cc.reference64(x, kind) - want[0].numpy()).max() <= 1e-12, (cc.NAMES[kind], Cn)
    assert cc.sum16 is cr.sum16
    v = rng.uniform(-8, 8, (300, 4000)).astype(np.float32)
    plain = np.zeros(4000, dtype=np.float32)
    for c in range(300):
        plain = plain + v[c]
    assert np.array_equal(cc.bits_of(cc.twin(v, cc.SUM)), cc.bits_of(cr.sum16(v)))
    assert (cc.bits_of(cc.twin(v, cc.SUM)) != cc.bits_of(plain)).mean() > 0.2
    assert np.array_equal(cc.bits_of(cc.twin(v, cc.MEAN)), cc.bits_of(cr.sum16(v) / np.float32(300)))
    assert np.array_equal(cc.bits_of(cc.twin(v, cc.NORM)), cc.bits_of(np.sqrt(cr.sum16(v * v))))
    # float16: the sum is made in float32 and rounded once; beyond the format's range it is the infinity of its sign
    h = np.full((4, 2), 30000.0, dtype=np.float16)
    h[:, 1] = -30000.0
    assert np.array_equal(cc.twin(h, cc.SUM), np.array([np.inf, -np.inf], dtype=np.float16))
    assert np.array_equal(cc.twin(h, cc.MEAN), np.array([30000.0, -30000.0], dtype=np.float16))


@pytest.mark.parametrize("dtype", [np.float32, np.float16], ids=["f32", "f16"])
def test_arg_and_extreme_kinds_are_torchs_on_the_cpu(dtype):
    """The twin's ARGMAX / ARGMIN / MAX / MIN against torch.max / torch.min(x, 1) on the CPU -- indices equal, values
    bit for bit where they are no NaN (signed zeros included) and NaNs in the same places -- and against torch.argmax /
    argmin and numpy's, on tie-heavy values with +0 / -0 mixed and NaN pixels, and on values with infinities."""
    rng = np.random.default_rng(3)
    sawNegZero = sawNan = sawTie = 0
    for Cn in (1, 2, 3, 16, 17, 40, 300):
        for x in (cc.tie_values(rng, (Cn, 4, 50), dtype), cc.values(rng, (Cn, 4, 50), dtype)):
            t = torch.from_numpy(x)[None]
            for argKind, valKind, fn, argFn, npFn in ((cc.ARGMAX, cc.MAX, torch.max, torch.argmax, np.argmax),
                                                      (cc.ARGMIN, cc.MIN, torch.min, torch.argmin, np.argmin)):
                want = fn(t, 1)
                idx, val = cc.twin_arg(x, argKind), cc.twin(x, valKind)
                assert idx.dtype == np.int64 and val.dtype == dtype
                assert np.array_equal(idx, want.indices[0].numpy()), (Cn, cc.NAMES[argKind])
                assert np.array_equal(idx, argFn(t, 1)[0].numpy()) and np.array_equal(idx, npFn(x, axis=0))
                wv = want.values[0].numpy()
                assert cc.same_bits(val, wv), (Cn, cc.NAMES[valKind])
                assert np.array_equal(np.signbit(val[~np.isnan(wv)]), np.signbit(wv[~np.isnan(wv)]))
                sawNegZero += int(((val == 0) & np.signbit(val)).sum())
                sawNan += int(np.isnan(val).sum())
                sawTie += int((cc.extreme_in_two_slices(x.reshape(Cn, -1), argKind)).sum())
    assert sawNegZero and sawNan and sawTie > 1000
    # the rules, one by one
    col = (lambda *v: np.array(v, dtype=dtype)[:, None])
    assert cc.twin_arg(col(1, np.nan, 5, np.nan), cc.ARGMAX)[0] == 1 and cc.twin_arg(col(1, np.nan, -5), cc.ARGMIN)[0] == 1
    assert cc.twin_arg(col(-0.0, 0.0, -0.0), cc.ARGMAX)[0] == 0 and np.signbit(cc.twin(col(-0.0, 0.0), cc.MAX)[0])
    assert cc.twin_arg(col(0.0, -0.0), cc.ARGMIN)[0] == 0 and not np.signbit(cc.twin(col(0.0, -0.0), cc.MIN)[0])
    assert cc.twin_arg(col(-np.inf, -np.inf), cc.ARGMAX)[0] == 0 and cc.twin_arg(col(3, np.inf, np.inf), cc.ARGMAX)[0] == 1
    assert cc.twin_arg(col(2, 7, 7, 2), cc.ARGMAX)[0] == 1 and cc.twin_arg(col(2, 7, 7, 2), cc.ARGMIN)[0] == 0


def test_c_entry_points_check_their_arguments(lib):
    """Bad arguments return CB_ERR_BADARG (-1) before anything is launched (the pointers here are never followed)."""
    C = lib.C
    X, O, BITS, COPY, M, L, LABEL = (0x1000 * i for i in range(1, 8))
    ARG, VAL2 = cc.packed([cc.ARGMAX]), cc.packed([cc.MEAN, cc.MAX])

    def fwd(x=X, o=O, mask=None, lst=None, cap=0, count=None, bits=BITS, cp=COPY, label=None, Cn=3, H=4, W=5, ops=VAL2,
            nOps=2, dt=lib.CB_F32):
        return C.cbinfer_cbchancollapse_forward(x, o, mask, lst, cap, count, bits, cp, label, Cn, H, W, ops, nOps, dt, None)

    def chg(x=X, o=O, mask=None, bits=BITS, cp=COPY, label=None, Cn=3, H=4, W=5, ops=ARG, nOps=1, dt=lib.CB_F16):
        return C.cbinfer_chancollapse_changed(x, o, mask, 0, bits, cp, label, Cn, H, W, ops, nOps, dt, None)

    for call in (fwd, chg):
        for bad in (dict(x=None), dict(o=None), dict(o=X), dict(bits=None), dict(cp=None), dict(cp=BITS), dict(mask=BITS),
                    dict(mask=COPY), dict(Cn=0), dict(H=0), dict(W=-1), dict(dt=lib.CB_F32S), dict(dt=7),
                    dict(nOps=0), dict(nOps=5, ops=cc.packed([0, 1, 2, 3, 4])), dict(nOps=-1), dict(ops=7, nOps=1),
                    dict(ops=15, nOps=1), dict(ops=-1, nOps=1), dict(ops=cc.packed([cc.MEAN, cc.MAX]), nOps=1),
                    dict(ops=cc.packed([cc.ARGMAX, cc.MEAN]), nOps=2), dict(ops=cc.packed([cc.MEAN, cc.ARGMIN]), nOps=2),
                    dict(ops=cc.packed([cc.ARGMAX, cc.ARGMIN]), nOps=2), dict(ops=cc.packed([cc.SUM, 7]), nOps=2),
                    dict(label=LABEL, ops=VAL2, nOps=2), dict(label=LABEL, ops=cc.packed([cc.MAX]), nOps=1),
                    dict(label=BITS, ops=ARG, nOps=1), dict(label=COPY, ops=ARG, nOps=1), dict(label=X, ops=ARG, nOps=1),
                    dict(label=O, ops=ARG, nOps=1), dict(label=M, mask=M, ops=ARG, nOps=1),
                    dict(H=1 << 16, W=1 << 15), dict(Cn=1 << 25)):
            assert call(**bad) == -1, (call.__name__, bad)
    for bad in (dict(lst=L, cap=-1), dict(mask=M, lst=L, cap=1), dict(count=L)):
        assert fwd(**bad) == -1, bad
    sup = C.cbinfer_chancollapse_supported
    assert all(sup(k, 1, 1) == 1 and sup(k, 1, 1 << 20) == 1 for k in range(7))
    assert sup(cc.packed([cc.SUM, cc.MEAN, cc.NORM, cc.MAX]), 4, 8) == 1 and sup(cc.packed([cc.MIN, cc.MIN]), 2, 8) == 1
    assert sup(7, 1, 8) == 0 and sup(0, 0, 8) == 0 and sup(0, 5, 8) == 0 and sup(0, 1, 0) == 0 and sup(0x10, 1, 8) == 0
    assert sup(cc.packed([cc.MEAN, cc.ARGMAX]), 2, 8) == 0 and sup(-1, 4, 8) == 0
    assert [getattr(lib, "CC_" + n) for n in cc.NAMES] == list(range(7))
    assert C.cbinfer_cbchancollapse_forward.launcher and C.cbinfer_chancollapse_changed.launcher
    assert not C.cbinfer_chancollapse_supported.launcher
    # an addition only: the version and the old entry points' refusal of kind 4 are as they were
    assert C.cbinfer_abi_version() == 11 and C.cbinfer_chanreduce_supported(4, 8, 0.0) == 0
    assert {'cbinfer_chancollapse_supported', 'cbinfer_chancollapse_changed', 'cbinfer_cbchancollapse_forward'} <= set(
        lib.EXPORTED_SYMBOLS)


def test_constructor_takes_the_ops_and_refuses_the_rest(pkg, lib):
    Err = lib.CBinferError
    for name, kind in zip(cc.OP_NAMES, range(7)):
        m = pkg.CBChannelReduce2d(name)
        assert m.collapseOps == ((name,), kind) and m.keepdim and not m.labelChanges and m.opName == name
        assert m.kind is None and m.eps == 0.0 and m.gamma is None and m.beta is None
        assert not m.propChangeIndexes and m.cloneOutput and m.outputState.numel() == 0
        assert 'ops=%s,' % name in repr(m)
    m = pkg.CBChannelReduce2d(('mean', 'max'))
    assert m.collapseOps == (('mean', 'max'), cc.packed([cc.MEAN, cc.MAX])) and 'ops=mean,max' in repr(m)
    assert pkg.CBChannelReduce2d(('sum', 'mean', 'norm', 'min')).collapseOps[1] == cc.packed([0, 1, 2, 4])
    assert pkg.CBChannelReduce2d(('norm',)).collapseOps == (('norm',), cc.NORM)
    m = pkg.CBChannelReduce2d('argmin', keepdim=False, labelChanges=True)
    assert not m.keepdim and m.labelChanges and 'labelChanges=True' in repr(m) and 'keepdim=False' in repr(m)
    assert not pkg.CBChannelReduce2d('max', keepdim=False).keepdim
    for args, kw, what in ((('sum', 1e-5), {}, "eps=1e-05 given for op='sum'"),
                           ((('mean', 'max'), 0.0), {}, r"eps=0.0 given for op=\('mean', 'max'\)"),
                           (('argmax',), dict(eps=1e-3), "eps=0.001 given for op='argmax'"),
                           (('mean',), dict(labelChanges=True), "labelChanges=True with op='mean'"),
                           ((('max',),), dict(labelChanges=True), r"labelChanges=True with op=\('max',\)"),
                           (('l2norm',), dict(labelChanges=True), "labelChanges=True with op=l2norm"),
                           ((nn.Softmax2d(),), dict(keepdim=False), "keepdim=False with op=Softmax2d"),
                           ((('mean', 'max'),), dict(keepdim=False), "keepdim=False with the tuple op"),
                           (((),), {}, "has 0 entries"), ((('sum',) * 5,), {}, "has 5 entries"),
                           ((('mean', 'argmax'),), {}, "'argmax' is not one of the value ops"),
                           ((('argmin',),), {}, "'argmin' is not one of the value ops"),
                           ((('mean', 'l2norm'),), {}, "'l2norm' is not one of the value ops"),
                           ((('mean', 3),), {}, "3 is not one of the value ops"),
                           (('l1norm',), {}, "op='l1norm' is not supported, of the strings only 'l2norm'"),
                           (('amax',), {}, "op='amax' is not supported"),
                           ((['mean', 'max'],), {}, "op=list is not supported")):
        with pytest.raises(Err, match=what):
            pkg.CBChannelReduce2d(*args, **kw)
    # the old ops are as they were
    old = pkg.CBChannelReduce2d('l2norm')
    assert old.kind == cr.L2NORM and old.collapseOps is None and old.opName == 'l2norm' and 'kind=l2norm' in repr(old)
    assert pkg.CBChannelReduce2d(nn.Softmax2d()).kind == cr.SOFTMAX


def test_pickle_old_pickles_half_and_operand_checks(pkg, lib):
    m = pkg.CBChannelReduce2d('argmax', labelChanges=True)
    m.propChangeIndexes, m.cloneOutput = True, False
    m.__dict__['_chWork'] = {'key': None}
    c = pickle.loads(pickle.dumps(m))
    assert type(c) is pkg.CBChannelReduce2d and c.collapseOps == m.collapseOps and c.labelChanges and c.keepdim
    assert (c.propChangeIndexes, c.cloneOutput) == (True, False) and c._chWork is None and repr(c) == repr(m)
    # a module pickled before the collapsing ops existed has none of the new attributes: it still prints and runs its
    # own checks (the operand checks come before anything else is read)
    old = pkg.CBChannelReduce2d(nn.Softmax2d())
    for name in ('collapseOps', 'keepdim', 'labelChanges'):
        del old.__dict__[name]
    c = pickle.loads(pickle.dumps(old))
    assert 'collapseOps' not in c.__dict__ and c.kind == cr.SOFTMAX and 'kind=softmax' in repr(c)
    with pytest.raises(lib.CBinferError, match="HIP devices only"):
        c(torch.zeros(1, 4, 5, 6))
    # .half() converts a float state and leaves an int64 label map alone
    m.outputState = torch.arange(12).reshape(1, 1, 3, 4)
    m.half()
    assert m.outputState.dtype == torch.int64 and torch.equal(m.outputState, torch.arange(12).reshape(1, 1, 3, 4))
    v = pkg.CBChannelReduce2d(('mean', 'max'))
    v.outputState = torch.ones(1, 2, 3, 3)
    assert v.half().outputState.dtype == torch.float16
    # the operand checks are the module's
    x = torch.zeros(1, 4, 5, 6)
    for inp, what in ((torch.zeros(2, 4, 5, 6), r"\[1, C, H, W\]"), (('changeIndexes', x), "tuple"),
                      (None, "must be a tensor"), (x.double(), "float32 and float16"), (x.long(), "float32 and float16"),
                      (x, "HIP devices only")):
        with pytest.raises(lib.CBinferError, match=what):
            m(inp)
    net = nn.Sequential(m)
    assert any(t is m.outputState for t in pkg.getStateTensors(net))
    pkg.clearMemory(net)
    assert m.outputState.numel() == 0 and m._chWork is None


def _names(seq):
    return [(n, type(m).__name__) for n, m in seq.named_children()]


def _wiring(net):
    return [(n, type(m).__name__, getattr(m, 'propChangeIndexes', None), getattr(m, 'copyInput', None),
             getattr(m, 'kind', None)) for n, m in net.named_modules()]


def test_insert_takes_the_users_reduce_types(pkg, lib):
    """conv 3x3 -> ChannelPool -> conv 3x3 (2 -> 1) -> Softmax2d -> ... and a head that ends in an ArgMax2d: with
    reduceTypes the user's classes become CBChannelReduce2d with the named op; without the keyword the wiring is what
    it was."""
    def make():
        torch.manual_seed(1)
        src = nn.Sequential()
        for name, mod in (('body', nn.Conv2d(8, 16, 3, padding=1)), ('pool', ChannelPool()),
                          ('gate', nn.Conv2d(2, 1, 3, padding=1)), ('head', nn.Conv2d(1, 5, 1)), ('prob', nn.Softmax2d()),
                          ('label', ArgMax2d())):
            src.add_module(name, mod)
        return pkg.convert(src.eval(), threshold=0.05)

    plain, same = pkg.insertCBChannelOps(make()), pkg.insertCBChannelOps(make(), reduceTypes=None)
    assert _names(plain) == [('body', 'CBConv2d'), ('pool', 'ChannelPool'), ('gate', 'CBConv2d'), ('head', 'CBConv2d'),
                             ('prob', 'CBChannelReduce2d'), ('label', 'ArgMax2d')]
    assert _wiring(plain) == _wiring(same) == _wiring(pkg.insertCBChannelOps(make(), (), {}))
    net = make()
    assert pkg.insertCBChannelOps(net, reduceTypes={ChannelPool: ('max', 'mean'), ArgMax2d: 'argmax'}) is net
    assert _names(net) == [('body', 'CBConv2d'), ('pool', 'CBChannelReduce2d'), ('gate', 'CBConv2d'), ('head', 'CBConv2d'),
                           ('prob', 'CBChannelReduce2d'), ('label', 'CBChannelReduce2d')]
    assert net.pool.collapseOps[0] == ('max', 'mean') and net.label.collapseOps[0] == ('argmax',)
    assert net.body.propChangeIndexes and net.head.propChangeIndexes
    assert net.prob.propChangeIndexes      # (handed on to the module behind it, another CBChannelReduce2d)
    assert not net.pool.propChangeIndexes and net.gate.copyInput      # (a 3x3 layer behind a state that is handed out)
    assert not net.label.propChangeIndexes and net.prob.kind == cr.SOFTMAX

    class MyPool(ChannelPool):
        pass
    sub = make()
    sub.pool = MyPool()      # (exact types, as layerNormTypes has it)
    pkg.insertCBChannelOps(sub, reduceTypes={ChannelPool: ('max', 'mean')})
    assert _names(sub)[1] == ('pool', 'MyPool')
    with pytest.raises(lib.CBinferError, match="'amax' is not one of the value ops"):
        pkg.insertCBChannelOps(make(), reduceTypes={ChannelPool: ('amax', 'mean')})
    # the producer table is as it was
    from cbinfer_amd import chain
    assert [name for name in chain.PASSES if pkg.CBChannelReduce2d in chain.producers(name)] == [
        'insertCBChannelOps', 'insertCBPadding', 'insertCBGating', 'insertCBResize']
