"""CPU-only tests of the change-based element-wise operators of two maps (CBBinary2d, CBGLU2d, CBGated,
insertCBGating; cb_binary.hip): the numpy twin of tests/binary_cases.py against torch's CPU operators
bit for bit, the argument checks of the C entry points, the modules' refusals, buffers, pickling and wiring.  No kernel
is launched here."""
import copy
import inspect
import pickle

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import binary_cases as bc
from optest import lib, names_of, pkg      # noqa: F401  (fixtures)


# ------------------------------------------------------------------------------------------------ the twin
def _by_element(fn):
    """torch.maximum / torch.minimum evaluated by torch's element-wise code.  At a tie of +0 against -0 torch's CPU
    operator has no single answer: the vectorised body of a long tensor returns b (the x86 max / min instruction), the
    element-wise tail -- and any tensor shorter than a vector -- returns a (measured here: 67 float32 pairs give 64
    times b, then 3 times a).  The specification is the element-wise operator, so the reference is taken four elements
    at a time, below every vector width; the operands, every tie among them, are the same."""
    def run(a, b):
        shape = torch.broadcast_shapes(a.shape, b.shape)
        a, b = (t.contiguous().reshape(-1) for t in torch.broadcast_tensors(a, b))
        return torch.cat([fn(x, y) for x, y in zip(a.split(4), b.split(4))]).reshape(shape)
    return run


def _torch_op(op, reverse):
    return {'add': torch.add, 'mul': torch.mul, 'maximum': _by_element(torch.maximum),
            'minimum': _by_element(torch.minimum), 'sub': (lambda a, b: torch.sub(b, a)) if reverse else torch.sub}[op]


@pytest.mark.parametrize("dtype", [np.float32, np.float16])
def test_twin_is_torchs_cpu_operator_bit_for_bit(dtype):
    """torch.add / sub / mul / maximum / minimum and a * F.hardsigmoid(b) on +-0, +-inf, NaN, float16 subnormals and
    ties of equal magnitude, every value against every other, in every operand form by broadcasting.  NaN results are
    compared as NaN-ness, all others by bits."""
    pa, pb = bc.pairs(dtype)
    n = len(pa)
    # form -> (a [C, H, W], b in the twin's shape, b as torch broadcasts it)
    grids = {'map': (pa.reshape(2, 1, n // 2), pb.reshape(2, 1, n // 2), None),
             'halves': (np.concatenate([pa, pb]).reshape(2, 1, n), None, None)}
    s = bc.specials(dtype)
    k = len(s)
    # one-channel map: b[p] against a[c, p] over k channels;  channel vector: b[c] against a[c, p];  scalar: each value
    grids['pixel'] = (np.repeat(s, k).reshape(k, 1, k).copy(), s.reshape(1, 1, k).copy(), None)
    grids['channel'] = (np.tile(s, k).reshape(k, 1, k).copy(), s.copy(), s.reshape(k, 1, 1))
    seen = 0
    for form, (a, b, bt) in grids.items():
        ta = torch.from_numpy(a[:a.shape[0] // 2] if form == 'halves' else a)
        tb = torch.from_numpy(a[a.shape[0] // 2:] if form == 'halves' else (b if bt is None else bt))
        for op, reverse in bc.EXACT:
            want = _torch_op(op, reverse)(ta, tb).numpy()
            got = bc.twin(a, b, form, op, None, reverse)
            assert bc.same_bits(got, want), (form, op, reverse)
            seen += int(np.isnan(want).sum() > 0)
        want = (ta * F.hardsigmoid(tb)).numpy()
        assert bc.same_bits(bc.twin(a, b, form, 'mul', 'hardsigmoid'), want), (form, 'hardsigmoid')
    for v in s:      # scalar form
        a = s.reshape(1, 1, k).copy()
        b = np.array([v], dtype=dtype)
        for op, reverse in bc.EXACT:
            want = _torch_op(op, reverse)(torch.from_numpy(a), torch.from_numpy(b).reshape(1, 1, 1)).numpy()
            assert bc.same_bits(bc.twin(a, b, 'scalar', op, None, reverse), want), ('scalar', op, reverse, v)
        want = (torch.from_numpy(a) * F.hardsigmoid(torch.from_numpy(b).reshape(1, 1, 1))).numpy()
        assert bc.same_bits(bc.twin(a, b, 'scalar', 'mul', 'hardsigmoid'), want), ('scalar', 'hardsigmoid', v)
    assert seen >= 4 * len(bc.EXACT)
    # the rules the header spells out
    z, nz, nan, one = (np.array([[[v]]], dtype=dtype) for v in (0.0, -0.0, np.nan, 1.0))
    assert np.signbit(bc.twin(nz, z, 'map', 'maximum'))[0, 0, 0] and not np.signbit(bc.twin(z, nz, 'map', 'maximum'))[0, 0, 0]
    assert not np.signbit(bc.twin(z, nz, 'map', 'minimum'))[0, 0, 0] and np.signbit(bc.twin(nz, z, 'map', 'minimum'))[0, 0, 0]
    for op in ('maximum', 'minimum'):
        assert np.isnan(bc.twin(nan, one, 'map', op)).all() and np.isnan(bc.twin(one, nan, 'map', op)).all()


def test_twin_sigmoid_gate_rounds_the_gate_first():
    """The gate value is rounded to the operand dtype before the product, as the separate torch operator rounds it."""
    rng = np.random.default_rng(1)
    a = rng.uniform(-20, 20, (3, 4, 5)).astype(np.float16)
    b = rng.uniform(-8, 8, (3, 4, 5)).astype(np.float16)
    got = bc.twin(a, b, 'map', 'mul', 'sigmoid').astype(np.float64)
    g = (1.0 / (1.0 + np.exp(-b.astype(np.float64)))).astype(np.float16).astype(np.float64)
    want = (a.astype(np.float64) * g).astype(np.float16).astype(np.float64)
    assert np.abs(got - want).max() <= 2.0 ** -10 * np.abs(want).max()      # (the float32 exp may move the gate one ulp)


# ------------------------------------------------------------------------------------------------ the C ABI
def test_supported_over_the_whole_grid(lib):
    C = lib.C
    for op in range(-1, 7):
        for gate in range(-1, 5):
            for reverse in (0, 1, 5):
                want = int(0 <= op <= 4 and 0 <= gate <= 2 and (gate == 0 or op == lib.BIN_MUL) and
                           (not reverse or op == lib.BIN_SUB))
                assert C.cbinfer_binary_supported(op, gate, reverse) == want, (op, gate, reverse)
    assert (lib.BIN_ADD, lib.BIN_SUB, lib.BIN_MUL, lib.BIN_MAXIMUM, lib.BIN_MINIMUM) == (0, 1, 2, 3, 4)
    assert (lib.BIN_MAP, lib.BIN_PIXEL, lib.BIN_CHANNEL, lib.BIN_SCALAR, lib.BIN_HALVES) == (0, 1, 2, 3, 4)
    assert C.cbinfer_abi_version() == 11
    assert {'cbinfer_binary_supported', 'cbinfer_binary_changed', 'cbinfer_cbbinary_forward'} <= set(lib.EXPORTED_SYMBOLS)
    header = open(__file__.rsplit('/tests/', 1)[0] + '/include/cbinfer_hip.h').read()
    for name in ('cbinfer_binary_supported', 'cbinfer_binary_changed', 'cbinfer_cbbinary_forward', 'CB_BIN_HALVES',
                 'CB_BIN_GATE_HARDSIGMOID', 'CB_BIN_B_OWN'):
        assert name in header


def test_c_entry_points_check_their_arguments(lib):
    """Bad arguments return CB_ERR_BADARG (-1) before anything is launched (the pointers here are never followed)."""
    C = lib.C
    A, B, O, BITS, COPY, M, L = (0x100000 * i for i in range(1, 8))
    MAP, PIXEL, CHANNEL, SCALAR, HALVES = range(5)
    NONE, OWN = 0, 1

    def fwd(a=A, b=B, o=O, maskA=None, listA=None, capA=0, countA=None, maskB=None, listB=None, capB=0, countB=None,
            form=MAP, chg=OWN, bits=BITS, cp=COPY, Cn=3, H=4, W=5, op=lib.BIN_MUL, gate=0, reverse=0, dt=lib.CB_F32):
        return C.cbinfer_cbbinary_forward(a, b, o, maskA, listA, capA, countA, maskB, listB, capB, countB, form, chg, bits,
                                          cp, Cn, H, W, op, gate, reverse, dt, None)

    def chg(a=A, b=B, o=O, maskA=None, maskB=None, form=MAP, bits=BITS, cp=COPY, Cn=3, H=4, W=5, op=lib.BIN_MUL, gate=0,
            reverse=0, dt=lib.CB_F16):
        return C.cbinfer_binary_changed(a, b, o, maskA, 0, maskB, 0, bits, cp, Cn, H, W, form, op, gate, reverse, dt, None)

    for call in (fwd, chg):
        for bad in (dict(a=None), dict(b=None), dict(o=None), dict(bits=None), dict(cp=None), dict(cp=BITS), dict(Cn=0),
                    dict(H=0), dict(W=-1), dict(dt=lib.CB_F32S), dict(dt=7), dict(H=1 << 16, W=1 << 15),
                    dict(Cn=1 << 25), dict(maskA=COPY), dict(maskA=BITS), dict(maskB=COPY), dict(maskB=BITS),
                    # unknown form / op / gate; a gate or reverse with the wrong op
                    dict(form=-1), dict(form=5), dict(op=-1), dict(op=5), dict(gate=-1), dict(gate=3),
                    dict(op=lib.BIN_ADD, gate=1), dict(op=lib.BIN_SUB, gate=2), dict(op=lib.BIN_MAXIMUM, gate=1),
                    dict(op=lib.BIN_MUL, reverse=1), dict(op=lib.BIN_ADD, reverse=1), dict(op=lib.BIN_MINIMUM, reverse=1),
                    # the halves form derives b itself; the others need it
                    dict(form=HALVES), dict(form=PIXEL, b=None), dict(form=SCALAR, b=None),
                    # out aliasing an operand (in halves form also the derived upper half)
                    dict(o=A), dict(o=B), dict(form=HALVES, b=None, o=A),
                    dict(form=HALVES, b=None, o=A + 3 * 4 * 5 * (4 if call is fwd else 2)),
                    # a mask for an operand that has no pixels of its own
                    dict(form=CHANNEL, maskB=M), dict(form=SCALAR, maskB=M), dict(form=HALVES, b=None, maskB=M)):
            if call is fwd and bad.get('form') == HALVES:
                bad = dict(bad, chg=NONE)
            assert call(**bad) == -1, (call.__name__, bad)
    for bad in (dict(listA=L, capA=-1), dict(listB=L, capB=-1), dict(maskA=M, listA=L), dict(maskB=M, listB=L),
                dict(countA=L), dict(countB=L), dict(chg=-1), dict(chg=2),
                # a mask or a list for b where b cannot have one
                dict(chg=NONE, maskB=M), dict(chg=NONE, listB=L, capB=2), dict(form=PIXEL, chg=NONE, maskB=M),
                dict(form=CHANNEL, listB=L, capB=2), dict(form=SCALAR, chg=NONE, listB=L, capB=2),
                dict(form=HALVES, b=None, chg=NONE, listB=L, capB=2), dict(form=HALVES, b=None, chg=OWN)):
        assert fwd(**bad) == -1, bad


# ------------------------------------------------------------------------------------------------ the modules
def test_constructor_refusals_constants_and_buffers(pkg, lib):
    Err = lib.CBinferError
    B = pkg.CBBinary2d
    for kwargs, what in ((dict(op='div'), "op='div' is not supported"), (dict(op='mul', gate='tanh'), "gate='tanh'"),
                         (dict(op='add', gate='sigmoid'), "a gate goes with 'mul' only"),
                         (dict(op='mul', reverse=True), "reverse with 'sub' only"),
                         (dict(op='mul', other=torch.zeros(2, 3)), r"other has shape \(2, 3\)"),
                         (dict(op='mul', other=torch.zeros(2, 3, 4, 4)), r"other has shape \(2, 3, 4, 4\)"),
                         (dict(op='mul', other=torch.zeros(3, 2, 1)), r"other has shape \(3, 2, 1\)"),
                         (dict(op='mul', other=torch.zeros(3, dtype=torch.int32)), "float32 or float16"),
                         (dict(op='mul', other='gamma'), "got str"), (dict(op='mul', other=True), "got bool")):
        with pytest.raises(Err, match=what):
            B(**kwargs)
    # a constant is copied: later edits of the source are not followed; it follows .half() / .to()
    gamma = nn.Parameter(torch.arange(4, dtype=torch.float32))
    m = B('mul', other=gamma)
    with torch.no_grad():
        gamma.mul_(2.0)
    assert torch.equal(m.other, torch.arange(4, dtype=torch.float32)) and not m.other.requires_grad
    assert list(m.state_dict().keys()) == ['other', 'outputState'] and m.hasOther and m.otherNumber is None
    assert m.half().other.dtype == torch.float16 and m.float().other.dtype == torch.float32
    for shape in ((1, 4, 5, 6), (1, 1, 5, 6), (1, 4, 1, 1), (4, 1, 1), (4,), (1,), (), (1, 1, 1, 1)):
        assert tuple(B('sub', other=torch.zeros(shape), reverse=True).other.shape) == shape
    n = B('mul', other=0.1)
    assert n.other is None and n.otherNumber == 0.1 and n.hasOther and 'number 0.1' in repr(n)
    assert B('maximum', other=3).otherNumber == 3.0
    assert "x * torch.tensor(v, dtype=x.dtype)" in B.__doc__
    # the classification of a constant against the frame
    x = torch.zeros(1, 4, 5, 6)
    for shape, form in (((1, 4, 5, 6), lib.BIN_MAP), ((1, 1, 5, 6), lib.BIN_PIXEL), ((1, 4, 1, 1), lib.BIN_CHANNEL),
                        ((4, 1, 1), lib.BIN_CHANNEL), ((4,), lib.BIN_CHANNEL), ((1,), lib.BIN_SCALAR), ((), lib.BIN_SCALAR)):
        assert B('mul', other=torch.zeros(shape))._constant(x, 4, 5, 6)[1] == form, shape
    for shape in ((1, 3, 5, 6), (3,), (1, 1, 5, 7), (5, 1, 1)):
        with pytest.raises(Err, match=r"`other` has shape .* operand a is \(1, 4, 5, 6\)"):
            B('mul', other=torch.zeros(shape))._constant(x, 4, 5, 6)
    # a buffer of another dtype or device is named with the operand's
    with pytest.raises(Err, match=r"operand a is torch.float16 on cpu, the constant operand `other` torch.float32 on cpu"):
        B('mul', other=torch.zeros(4))(x.half())
    # GLU
    with pytest.raises(Err, match="nn.GLU\\(dim=-1\\) does not gate over the channels"):
        pkg.CBGLU2d(nn.GLU())
    with pytest.raises(Err, match="Sigmoid is not supported, only an nn.GLU"):
        pkg.CBGLU2d(nn.Sigmoid())

    class MyGLU(nn.GLU):
        pass
    with pytest.raises(Err, match="MyGLU is not supported"):
        pkg.CBGLU2d(MyGLU(1))
    assert (pkg.CBGLU2d(nn.GLU(1)).op, pkg.CBGLU2d(nn.GLU(-3)).gate) == ('mul', 'sigmoid')


def test_forward_refusals_name_the_module_and_the_shapes(pkg, lib):
    Err = lib.CBinferError
    x = torch.zeros(1, 4, 5, 6)
    two, const = pkg.CBBinary2d('mul', gate='sigmoid'), pkg.CBBinary2d('mul', other=torch.zeros(4))
    idx = torch.zeros(2, dtype=torch.int32)
    for call, what in ((lambda: two(x), r"forward\(a, b\) takes two operands"),
                       (lambda: const(x, x), r"constant operand `other`: forward\(a\)"),
                       (lambda: two(torch.zeros(2, 4, 5, 6), x), r"operand a must be a \[1, C, H, W\] tensor, got \(2, 4, 5, 6\)"),
                       (lambda: two(x.double(), x.double()), "float32 and float16 tensors only"),
                       (lambda: two(x, torch.zeros(1, 4, 5, 7)), r"a is \(1, 4, 5, 6\), b is \(1, 4, 5, 7\)"),
                       (lambda: two(x, torch.zeros(1, 2, 5, 6)), r"do not fit: a is \(1, 4, 5, 6\), b is \(1, 2, 5, 6\)"),
                       (lambda: two(x, torch.zeros(4)), r"b must be \[1, C, H, W\], \[1, 1, H, W\] or \[1, C, 1, 1\]"),
                       (lambda: two(x, x.half()), "operands differ: a is .*float32.*b is .*float16"),
                       (lambda: two(x, ('changeIndexes', torch.zeros(1, 4, 1, 1), idx)),
                        r"operand b is a \[1, C, 1, 1\] channel vector \(1, 4, 1, 1\) and came with change indexes"),
                       (lambda: two(x, ('changeIndexes', x)), "tuple"), (lambda: two(x, None), "takes two operands"),
                       (lambda: two(x, 'b'), "must be a tensor"),
                       (lambda: two(x, x), "HIP devices only"), (lambda: two(x, x[:, :1]), "HIP devices only"),
                       (lambda: two(x, torch.zeros(1, 4, 1, 1)), "HIP devices only"),
                       (lambda: const(x), "HIP devices only"), (lambda: pkg.CBBinary2d('add', other=2.0)(x), "HIP devices only"),
                       (lambda: pkg.CBGLU2d(nn.GLU(1))(torch.zeros(1, 5, 3, 3)), r"\(1, 5, 3, 3\) has an odd number of channels"),
                       (lambda: pkg.CBGLU2d(nn.GLU(1))(torch.zeros(4, 3, 3)), r"operand x must be a \[1, C, H, W\]"),
                       (lambda: pkg.CBGLU2d(nn.GLU(1))(x), "HIP devices only")):
        with pytest.raises(Err, match=what):
            call()
    for m in (two, const):
        assert m.outputState.numel() == 0 and m._binWork is None      # nothing was allocated, nothing launched


def test_exports_state_helpers_pickle_and_deepcopy(pkg, lib):
    import cbinfer_amd
    assert all(n in pkg.__all__ for n in ('CBBinary2d', 'CBGLU2d', 'CBGated', 'insertCBGating'))
    import pycbinfer.binary as alias
    assert alias is cbinfer_amd.binary and pkg.CBBinary2d is alias.CBBinary2d and pkg.binary is alias
    assert pkg.CBBinary2d in cbinfer_amd._STATEFUL and pkg.CBGLU2d in cbinfer_amd._STATEFUL
    b = pkg.CBBinary2d('sub', other=torch.arange(3.0), reverse=True)
    g = pkg.CBGLU2d(nn.GLU(1))
    b.propChangeIndexes, b.cloneOutput, g.cloneOutput = True, False, False
    gated = pkg.CBGated(nn.Sequential(nn.Tanh()), op='mul', gateFn='hardsigmoid')
    net = nn.Sequential(b, g, gated)
    b.outputState, g.outputState, gated.mul.outputState = torch.ones(1, 3, 2, 2), torch.ones(1, 2, 2, 2), torch.ones(1)
    for m in (b, g, gated.mul):
        m.__dict__['_binWork'] = {'key': None}
    states = pkg.getStateTensors(net)
    assert len(states) == 3 and all(any(t is m.outputState for t in states) for m in (b, g, gated.mul))
    for clone in (pickle.loads(pickle.dumps(net)), copy.deepcopy(net)):
        cb, cg, cm = clone[0], clone[1], clone[2].mul
        assert (type(cb), type(cg), type(cm)) == (pkg.CBBinary2d, pkg.CBGLU2d, pkg.CBBinary2d)
        assert (cb.op, cb.gate, cb.reverse, cb.propChangeIndexes, cb.cloneOutput) == ('sub', None, True, True, False)
        assert (cm.op, cm.gate, cm.reverse) == ('mul', 'hardsigmoid', False) and not cg.cloneOutput
        assert torch.equal(cb.other, torch.arange(3.0)) and cb.other is not b.other
        for new, old in ((cb, b), (cg, g), (cm, gated.mul)):
            assert new._binWork is None and torch.equal(new.outputState, old.outputState) and repr(new) == repr(old)
    pkg.clearMemory(net)
    for m in (b, g, gated.mul):
        assert m.outputState.numel() == 0 and m._binWork is None
    assert torch.equal(b.other, torch.arange(3.0))      # (a constant operand is no state)


# ------------------------------------------------------------------------------------------------ wiring
def test_insert_gating_wiring_and_what_it_leaves(pkg, lib):
    torch.manual_seed(1)
    seq = nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), nn.GLU(1), nn.Conv2d(4, 8, 1), nn.GLU(-3), nn.Conv2d(4, 6, 3, padding=1),
                        nn.GLU(1)).eval()
    net = pkg.convert(seq, threshold=0.05)
    assert names_of(net) == ['CBConv2d', 'GLU', 'CBConv2d', 'GLU', 'CBConv2d', 'GLU']
    net[4].copyInput = False
    assert pkg.insertCBGating(net, cloneOutput=False) is net
    assert names_of(net) == ['CBConv2d', 'CBGLU2d', 'CBConv2d', 'CBGLU2d', 'CBConv2d', 'CBGLU2d']
    assert list(net._modules) == ['0', '1', '2', '3', '4', '5']
    assert net[0].propChangeIndexes and net[2].propChangeIndexes and net[4].propChangeIndexes
    assert net[1].propChangeIndexes and not net[3].propChangeIndexes and not net[5].propChangeIndexes      # (1x1 behind [1])
    assert net[4].copyInput is True and not any(m.cloneOutput for m in (net[1], net[3], net[5]))
    # a feedback-mode consumer keeps no input reference; the default clones
    net = pkg.convert(nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), nn.GLU(1), nn.Conv2d(4, 3, 3, padding=1)).eval(),
                      threshold=0.05)
    net[2].copyInput, net[2].feedbackLoop = False, True
    pkg.insertCBGating(net)
    assert type(net[1]) is pkg.CBGLU2d and net[1].cloneOutput and net[2].copyInput is False
    # behind the other producers, the new ones included
    for prod in (pkg.CBPointwise2d(nn.Tanh()), pkg.CBPad2d(nn.ZeroPad2d(1)), pkg.CBBinary2d('mul', other=2.0),
                 pkg.CBGLU2d(nn.GLU(1)), pkg.CBChannelReduce2d(nn.Softmax2d()), pkg.CBAdd2d()):
        net = pkg.insertCBGating(nn.Sequential(prod, nn.GLU(1)))
        assert type(net[1]) is pkg.CBGLU2d and net[0].propChangeIndexes, type(prod).__name__
    gated = pkg.CBGated(nn.Sequential(nn.Tanh()))
    net = pkg.insertCBGating(nn.Sequential(gated, nn.GLU(1)))
    assert type(net[1]) is pkg.CBGLU2d and gated.mul.propChangeIndexes
    # a GLU over another dim, a subclass, behind a non-producer or at the front: dense, flags untouched

    class MyGLU(nn.GLU):
        pass
    seq = nn.Sequential(nn.GLU(1), nn.Conv2d(4, 8, 3, padding=1), nn.GLU(-1), nn.Conv2d(8, 8, 1), nn.GLU(2), nn.Conv2d(8, 8, 1),
                        MyGLU(1), nn.Conv2d(4, 8, 1), nn.Tanh(), nn.GLU(1)).eval()
    net = pkg.convert(seq, threshold=0.05)
    before = names_of(net)
    pkg.insertCBGating(net)
    assert names_of(net) == before == ['GLU', 'CBConv2d', 'GLU', 'CBConv2d', 'GLU', 'CBConv2d', 'MyGLU', 'CBConv2d', 'Tanh', 'GLU']
    assert not any(getattr(m, 'propChangeIndexes', False) for m in net)


def test_gated_constructor_sets_the_flags(pkg, lib):
    def block(tail=None):
        torch.manual_seed(9)
        body = nn.Sequential(nn.Conv2d(8, 8, 3, padding=1), nn.ReLU(), nn.Conv2d(8, 8, 3, padding=1)).eval()
        if tail is not None:
            body.add_module('tail', tail)
        return pkg.convert(body, threshold=0.05)
    body = block()
    body[0].copyInput = False
    gate = pkg.convert(nn.Sequential(nn.Conv2d(8, 1, 1)).eval(), threshold=0.05)
    gate[0].copyInput, gate[0].feedbackLoop = False, True
    assert not body[1].propChangeIndexes and not gate[0].propChangeIndexes
    g = pkg.CBGated(body, gate)
    assert type(g.body) is nn.Sequential and type(g.gate) is nn.Sequential and g.body is body
    assert type(g.mul) is pkg.CBBinary2d and (g.mul.op, g.mul.gate) == ('mul', 'sigmoid')
    assert not g.mul.propChangeIndexes and g.mul.cloneOutput and not g.mul.hasOther
    assert body[1].propChangeIndexes and not body[0].propChangeIndexes and gate[0].propChangeIndexes
    assert body[0].copyInput is True and gate[0].copyInput is False      # (feedback mode keeps no reference)
    # the last module is not a CBConv2d: nobody could take the list
    body = block(nn.Tanh())
    g = pkg.CBGated(body, op='maximum', gateFn=None)
    assert g.gate is None and (g.mul.op, g.mul.gate) == ('maximum', None)
    assert not any(m.propChangeIndexes for m in body if type(m) is pkg.CBConv2d)
    assert type(pkg.CBGated(body[0]).body) is nn.Sequential and len(pkg.CBGated([body[0], body[1]]).body) == 2
    with pytest.raises(lib.CBinferError, match="a gate goes with 'mul' only"):
        pkg.CBGated(body, op='sub')
    # hand_on_changes reaches the product, as it reaches a CBResidual's sum
    from cbinfer_amd import chain
    chain.hand_on_changes(g)
    assert g.mul.propChangeIndexes


def test_producer_function_and_the_passes_that_use_it(pkg, lib):
    from cbinfer_amd import chain
    new = (pkg.CBBinary2d, pkg.CBGLU2d, pkg.CBGated)
    # producers for every pass but the two poolings, in this order (every pass's whole set: test_host_chain.py)
    pools = ['insertCBPooling', 'insertCBPooling(generalGeometry=True)']
    assert [name for name in chain.PASSES if not set(new) & set(chain.producers(name))] == pools
    assert all(tuple(t for t in chain.producers(name) if t in new) == new for name in chain.PASSES if name not in pools)

    def behind(prod, *mods):
        net = nn.Sequential(prod)
        for k, m in enumerate(mods):
            net.add_module('m%d' % k, m)
        return net.eval()
    for make, flag in ((lambda: pkg.CBBinary2d('mul', other=1.5), lambda p: p.propChangeIndexes),
                       (lambda: pkg.CBGLU2d(nn.GLU(1)), lambda p: p.propChangeIndexes),
                       (lambda: pkg.CBGated(nn.Sequential(nn.Tanh())), lambda p: p.mul.propChangeIndexes)):
        for run, kind in ((lambda p: pkg.insertCBPointwise(behind(p, nn.ReLU())), pkg.CBPointwise2d),
                          (lambda p: pkg.insertCBUpsampling(behind(p, nn.Upsample(scale_factor=2))), pkg.CBUpsample2d),
                          (lambda p: pkg.insertCBResize(behind(p, nn.Upsample(size=(9, 11), mode='bilinear'))), pkg.CBResize2d),
                          (lambda p: pkg.insertCBRearrange(behind(p, nn.PixelShuffle(2))), pkg.CBPixelShuffle2d),
                          (lambda p: pkg.insertCBChannelOps(behind(p, nn.Softmax2d())), pkg.CBChannelReduce2d),
                          (lambda p: pkg.insertCBPadding(behind(p, nn.ZeroPad2d(1))), pkg.CBPad2d),
                          (lambda p: pkg.insertCBGating(behind(p, nn.GLU(1))), pkg.CBGLU2d)):
            prod = make()
            net = run(prod)
            assert type(net.m0) is kind and flag(prod), (type(prod).__name__, kind.__name__)
        prod = make()
        net = pkg.insertCBTransposedConv(behind(prod, nn.ConvTranspose2d(4, 4, 2, stride=2)), threshold=0.05)
        assert type(net.m0) is pkg.CBConvTranspose2d      # (it runs its own detection: nothing is switched on)
        prod = make()
        net = pkg.convert(behind(prod, nn.Conv2d(4, 4, 3, padding=1, groups=4)), threshold=0.05, depthwise=True)
        assert type(net.m0) is pkg.CBDepthwiseConv2d and not flag(prod)
        pkg.linkDepthwise(net)
        assert flag(prod)


def test_batch_branch_and_program_refusals_name_the_module(pkg, lib):
    net = nn.Sequential()
    net.add_module('stem', pkg.convert(nn.Sequential(nn.Conv2d(3, 8, 3, padding=1)).eval(), threshold=0.05)[0])
    net.add_module('glu', pkg.CBGLU2d(nn.GLU(1)))
    with pytest.raises(lib.CBinferError, match=r"SequenceBatch: layer 'glu' is CBGLU2d \(.*a change-based element-wise "
                                               r"operator of two maps.*gated and attention"):
        pkg.SequenceBatch(net, 2)
    with pytest.raises(lib.CBinferError, match=r"BranchGroup: layer '0.glu' is CBGLU2d \(.*element-wise operator of two"):
        pkg.BranchGroup([net])
    net = nn.Sequential()
    net.add_module('stem', pkg.convert(nn.Sequential(nn.Conv2d(3, 8, 3, padding=1)).eval(), threshold=0.05)[0])
    net.add_module('att', pkg.CBGated(nn.Sequential(nn.Tanh())))
    with pytest.raises(lib.CBinferError, match=r"SequenceBatch: layer 'att.mul' is CBBinary2d \(op=mul, gate=sigmoid"):
        pkg.SequenceBatch(net, 2)
    with pytest.raises(lib.CBinferError, match=r"BranchGroup: layer '0.att.mul' is CBBinary2d"):
        pkg.BranchGroup([net])
    from cbinfer_amd import batch
    assert [row for row in batch.CHAIN_OPERATORS if pkg.CBBinary2d in row[0]] == [
        ((pkg.CBBinary2d, pkg.CBGLU2d), 'a change-based element-wise operator of two maps', 'gated and attention')]
    firsts = [row[0] for row in batch.CHAIN_OPERATORS]      # (the row was appended: it stands right behind CBPad2d's)
    assert firsts[firsts.index((pkg.CBBinary2d, pkg.CBGLU2d)) - 1] == (pkg.CBPad2d,)
    import cbinfer_amd.program as program
    said = inspect.getsource(pkg.FrameProgram)
    assert "pycbinfer.CBBinary2d / CBGated / CBGLU2d (insertCBGating)" in said
    assert "pycbinfer.CBPad2d (insertCBPadding) for an explicit padding" in said
    assert 'CBBinary2d' in program.__doc__ and 'CBGLU2d' in program.__doc__
