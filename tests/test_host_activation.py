"""CPU-only tests of the six element-wise kinds of CBPointwise2d(transcendental=True): the float64
formulas of tests/activation_cases.py against torch's CPU operators in double, the argument checks of the C entry
points, the constructor's table and refusals, insertCBPointwise(transcendental=True) on a ConvNeXt-type block and a
monodepth-type run, pickling.  No kernel is launched here."""
import pickle

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import activation_cases as ac
from test_host_chanreduce import LayerNorm2d, _names
from optest import lib, pkg      # noqa: F401  (fixtures)


def test_float64_formulas_are_torchs_operators():
    """reference64 against torch's CPU operators in double -- F.gelu both ways, F.elu, F.celu, F.selu, F.softplus with
    beta and threshold, F.mish -- to 1e-12 relative plus 1e-300: the specification IS the operator.  The formulas hold
    the float32-rounded constants, so torch is given inputs on which that does not show: float32 values, and for the
    kinds with a rounded constant (GELU, GELU_TANH, SELU) the bar holds for the formula with the constants as written
    (rounded=False), and the rounding of the constants moves it by less than a unit of the bound."""
    rng = np.random.default_rng(1)
    x = np.concatenate([rng.uniform(-20, 20, 200000), rng.standard_normal(50000) * 1e-3, [0.0, -0.0, 20.0, -20.0]])
    x = x.astype(np.float32)
    t = torch.from_numpy(x).double()
    alpha13, inv13 = float(np.float32(1.3)), float(np.float32(1.0 / 1.3))
    ops = [(ac.ELU, 1.0, 1.0, F.elu(t, 1.0)), (ac.ELU, 0.5, 1.0, F.elu(t, 0.5)), (ac.ELU, 0.5, 2.0, F.celu(t, 0.5)),
           (ac.SOFTPLUS, 1.0, 20.0, F.softplus(t, 1.0, 20.0)), (ac.SOFTPLUS, 2.0, 5.0, F.softplus(t, 2.0, 5.0)),
           (ac.MISH, 0.0, 0.0, F.mish(t))]
    for kind, p0, p1, want in ops:
        got, want = ac.reference64(x, kind, p0, p1), want.numpy()
        assert np.all(np.abs(got - want) <= 1e-12 * np.abs(want) + 1e-300), ac.case_name(kind, p0, p1)
    # CELU(1.3): the kernel multiplies by float32(1 / alpha), torch divides by alpha -- the same to 2^-25 relative in the
    # argument of expm1, whose condition number is at most 1 here
    got, want = ac.reference64(x, ac.ELU, alpha13, inv13), F.celu(t, alpha13).numpy()
    assert np.all(np.abs(got - want) <= 2.0 ** -24 * np.abs(want) + 1e-300)
    # the three kinds with a float32-rounded constant: exactly torch's operator once the constant is the float64 one
    for kind, want in ((ac.GELU, F.gelu(t)), (ac.GELU_TANH, F.gelu(t, approximate='tanh')), (ac.SELU, F.selu(t))):
        got, want = ac.reference64(x, kind, rounded=False), want.numpy()
        # (GELU's 1 + erf cancels for negative v in torch's double and in ours alike: absolute in |v|)
        assert np.all(np.abs(got - want) <= 1e-12 * np.abs(want) + 1e-15 * np.abs(x) + 1e-300), ac.NAMES[kind]
    # ... and the rounding of the constants moves the formula by less than one unit of the bound
    for kind, want in ((ac.GELU, F.gelu(t)), (ac.GELU_TANH, F.gelu(t, approximate='tanh')), (ac.SELU, F.selu(t))):
        got, want = ac.reference64(x, kind), want.numpy()
        assert np.all(np.abs(got - want) <= 2.0 ** -24 * (np.abs(want) + np.abs(x))), ac.NAMES[kind]


def test_non_finite_inputs_by_the_formula():
    x = np.array([np.inf, -np.inf, np.nan], dtype=np.float32)
    r = {k: ac.reference64(x, k, p0, p1) for k, p0, p1 in ((ac.GELU, 0, 0), (ac.GELU_TANH, 0, 0), (ac.ELU, 0.5, 2.0),
                                                             (ac.SELU, 0, 0), (ac.SOFTPLUS, 2.0, 5.0), (ac.MISH, 0, 0))}
    for k in (ac.GELU, ac.GELU_TANH, ac.MISH):
        assert r[k][0] == np.inf and np.isnan(r[k][1]) and np.isnan(r[k][2]), ac.NAMES[k]
    assert r[ac.ELU][0] == np.inf and r[ac.ELU][1] == -0.5 and np.isnan(r[ac.ELU][2])
    assert r[ac.SELU][0] == np.inf and r[ac.SELU][1] == -float(np.float32(ac.CONSTANTS[4])) and np.isnan(r[ac.SELU][2])
    assert r[ac.SOFTPLUS][0] == np.inf and r[ac.SOFTPLUS][1] == 0.0 and np.isnan(r[ac.SOFTPLUS][2])


def test_torchs_own_float32_operators_have_room_under_the_bounds():
    """Plausibility of the derived bounds: torch's CPU float32 operators, other implementations of the same functions,
    stay well inside them (the bound binds the KERNEL in tests/test_gpu_activation.py)."""
    rng = np.random.default_rng(2)
    x = rng.uniform(-20, 20, 300000).astype(np.float32)
    t = torch.from_numpy(x)
    for kind, p0, p1, got in ((ac.GELU, 0, 0, F.gelu(t)), (ac.GELU_TANH, 0, 0, F.gelu(t, approximate='tanh')),
                              (ac.ELU, 1.0, 1.0, F.elu(t)), (ac.ELU, 0.5, 2.0, F.celu(t, 0.5)), (ac.SELU, 0, 0, F.selu(t)),
                              (ac.SOFTPLUS, 1.0, 20.0, F.softplus(t)), (ac.SOFTPLUS, 2.0, 5.0, F.softplus(t, 2.0, 5.0)),
                              (ac.MISH, 0, 0, F.mish(t))):
        ok, ratio, rel, text = ac.judge(x, got.numpy(), kind, p0, p1)
        print("%-18s torch CPU f32: worst err / bound %.3f" % (ac.case_name(kind, p0, p1), ratio))
        assert ok, (ac.case_name(kind, p0, p1), text)


def test_c_entry_points_take_the_new_kinds_and_refuse_the_gap(lib):
    """cbinfer_pointwise_supported accepts 16..21 and refuses 10..15 and 22, ELU with a non-finite parameter, SOFTPLUS
    with p0 zero or non-finite or p1 a NaN; both entry points return CB_ERR_BADARG (-1) for those with fake pointers,
    before anything is launched."""
    C = lib.C
    assert C.cbinfer_abi_version() == 11
    sup = C.cbinfer_pointwise_supported
    inf, nan = float('inf'), float('nan')
    assert [getattr(lib, "PW_" + ac.NAMES[k]) for k in range(16, 22)] == list(range(16, 22))
    assert all(sup(k, 1.0, 1.0) == 1 for k in range(16, 22))
    assert all(sup(k, 1.0, 1.0) == 0 for k in list(range(10, 16)) + [22, 23, -1])
    refused = [(ac.ELU, inf, 1.0), (ac.ELU, 1.0, inf), (ac.ELU, -inf, 1.0), (ac.ELU, nan, 1.0), (ac.ELU, 1.0, nan),
               (ac.SOFTPLUS, 0.0, 20.0), (ac.SOFTPLUS, -0.0, 20.0), (ac.SOFTPLUS, 1.0, nan), (ac.SOFTPLUS, inf, 20.0),
               (ac.SOFTPLUS, nan, 20.0)]
    for kind, p0, p1 in refused:
        assert sup(kind, p0, p1) == 0, (kind, p0, p1)
    assert sup(ac.ELU, 0.0, 1.0) == 1 and sup(ac.ELU, -1.0, -2.0) == 1      # (alpha = 0 is torch's ELU too)
    assert sup(ac.SOFTPLUS, 2.0, inf) == 1 and sup(ac.SOFTPLUS, -1.0, -inf) == 1
    assert sup(ac.GELU, nan, inf) == 1      # (the parameters matter to ELU and SOFTPLUS only)
    X, O, BITS, COPY = 0x1000, 0x2000, 0x3000, 0x4000
    for kind, p0, p1 in refused + [(k, 1.0, 1.0) for k in (10, 15, 22)]:
        assert C.cbinfer_cbpointwise_forward(X, O, None, None, 0, None, BITS, COPY, 3, 4, 5, kind, p0, p1, None, None,
                                             None, lib.CB_F32, None) == -1, (kind, p0, p1)
        assert C.cbinfer_pointwise_changed(X, O, None, 0, BITS, COPY, 3, 4, 5, kind, p0, p1, None, None, None,
                                           lib.CB_F16, None) == -1, (kind, p0, p1)


def _bn(Cn):
    bn = nn.BatchNorm2d(Cn)
    with torch.no_grad():
        bn.running_var.copy_(torch.linspace(0.5, 2.0, Cn))
    return bn.eval()


def test_constructor_takes_the_new_types_only_with_the_keyword(pkg, lib):
    Err = lib.CBinferError
    inv13 = float(np.float32(1.0 / 1.3))
    table = [(nn.GELU(), ac.GELU, 0.0, 0.0), (nn.GELU(approximate='none'), ac.GELU, 0.0, 0.0),
             (nn.GELU(approximate='tanh'), ac.GELU_TANH, 0.0, 0.0), (nn.ELU(), ac.ELU, 1.0, 1.0),
             (nn.ELU(0.7, inplace=True), ac.ELU, 0.7, 1.0), (nn.CELU(0.5), ac.ELU, 0.5, 2.0),
             (nn.CELU(1.3), ac.ELU, 1.3, inv13), (nn.SELU(inplace=True), ac.SELU, 0.0, 0.0),
             (nn.Softplus(), ac.SOFTPLUS, 1.0, 20.0), (nn.Softplus(2, 5), ac.SOFTPLUS, 2.0, 5.0),
             (nn.Mish(), ac.MISH, 0.0, 0.0)]
    for act, kind, p0, p1 in table:
        m = pkg.CBPointwise2d(act, transcendental=True)
        assert (m.kind, m.p0, m.p1) == (kind, p0, p1) and m.scale is None and m.slope is None, act
        assert not m.propChangeIndexes and m.cloneOutput and m.outputState.numel() == 0
        assert ('act=%s,' % type(act).__name__) in repr(m)
        # without the keyword: refused exactly as before
        for kw in (dict(), dict(transcendental=False)):
            with pytest.raises(Err, match="act=%s is not supported, only an instance of exactly nn.ReLU, .*nn.Tanh$"
                               % type(act).__name__):
                pkg.CBPointwise2d(act, **kw)
    # the old table is there with the keyword as without, and the affine in front works for the new kinds
    assert pkg.CBPointwise2d(nn.Hardswish(), transcendental=True).kind == lib.PW_HARDSWISH
    m = pkg.CBPointwise2d(nn.Mish(), _bn(4), transcendental=True)
    assert m.kind == ac.MISH and m.scale.numel() == 4 and m.shift.dtype == torch.float32
    assert set(dict(m.named_buffers())) == {'scale', 'shift', 'outputState'}

    class MyGELU(nn.GELU):
        pass

    class MyELU(nn.ELU):
        pass
    for act, what in ((MyGELU(), "act=MyGELU is not supported"), (MyELU(), "act=MyELU is not supported"),
                      (nn.Softmax(dim=1), "act=Softmax is not supported"), (nn.Softsign(), "act=Softsign is not supported"),
                      (F.gelu, "act=builtin_function_or_method is not supported"), (nn.LogSigmoid(), "act=LogSigmoid"),
                      (nn.CELU(0.0), "alpha=0 is not supported"), (nn.Softplus(beta=0), "beta=0 is not supported"),
                      (nn.ELU(float('inf')), "parameters inf, 1.0 are not usable"),
                      (nn.Softplus(1.0, float('nan')), "parameters 1.0, nan are not usable")):
        with pytest.raises(Err, match=what):
            pkg.CBPointwise2d(act, transcendental=True)
    g = nn.GELU()
    g.approximate = 'sigmoid'      # (torch's own operator refuses this at the first call)
    with pytest.raises(Err, match="approximate='sigmoid' is not supported, only 'none' and 'tanh'"):
        pkg.CBPointwise2d(g, transcendental=True)
    # the refusal with the keyword names the whole table
    with pytest.raises(Err, match="nn.Tanh, nn.GELU, nn.ELU, nn.CELU, nn.SELU, nn.Softplus, nn.Mish$"):
        pkg.CBPointwise2d(nn.Softsign(), transcendental=True)


def _convnext(pkg):
    torch.manual_seed(1)
    src = nn.Sequential()
    for name, mod in (('stem', nn.Conv2d(8, 16, 1)), ('dw', nn.Conv2d(16, 16, 7, 1, 3, groups=16)),
                      ('norm', LayerNorm2d(16)), ('pw1', nn.Conv2d(16, 32, 1)), ('gelu', nn.GELU()),
                      ('norm2', LayerNorm2d(32)), ('head', nn.Conv2d(32, 5, 3, padding=1)), ('prob', nn.Softmax2d())):
        src.add_module(name, mod)
    return pkg.convert(src.eval(), threshold=0.05, depthwise=True)


def test_insert_on_a_convnext_type_block(pkg, lib):
    """The block of tests/test_host_chanreduce.py, 1x1 -> 7x7 depthwise -> LayerNorm2d -> 1x1 -> GELU -> LayerNorm2d ->
    3x3 head -> Softmax2d: with the keyword no dense torch module is left; without it the GELU stays, and the norm
    behind it."""
    net = _convnext(pkg)
    assert pkg.insertCBPointwise(net, transcendental=True) is net
    pkg.insertCBChannelOps(net, layerNormTypes=(LayerNorm2d,))
    want = [('stem', 'CBConv2d'), ('dw', 'CBDepthwiseConv2d'), ('norm', 'CBChannelReduce2d'), ('pw1', 'CBConv2d'),
            ('gelu', 'CBPointwise2d'), ('norm2', 'CBChannelReduce2d'), ('head', 'CBConv2d'), ('prob', 'CBChannelReduce2d')]
    assert _names(net) == want
    assert not [n for n, m in net.named_children() if type(m).__module__.startswith('torch.')]
    assert net.gelu.kind == ac.GELU and net.gelu.actName == 'GELU' and net.gelu.scale is None
    assert net.pw1.propChangeIndexes      # (the 1x1 producer in front of the GELU hands its changes on)
    # the GELU module hands its mask on exactly where a 1x1 / stride-1 / padding-0 CBConv2d follows: here a norm
    # follows, and insertCBChannelOps has switched the flag on for its own module
    assert net.gelu.propChangeIndexes and net.norm2.kind != ac.GELU
    assert net.norm.propChangeIndexes and net.dw.propChangeIndexes and net.head.propChangeIndexes
    flags = [(n, m.propChangeIndexes) for n, m in net.named_children()]
    pkg.insertCBPointwise(net, transcendental=True)
    pkg.insertCBChannelOps(net, layerNormTypes=(LayerNorm2d,))
    assert _names(net) == want and [(n, m.propChangeIndexes) for n, m in net.named_children()] == flags
    # the pass alone: the flag of the new module depends on what stands behind it
    for behind, flag in ((nn.Conv2d(32, 8, 1), True), (nn.Conv2d(32, 8, 3, padding=1), False),
                         (nn.Conv2d(32, 8, 1, stride=2), False), (nn.Identity(), False)):
        seq = pkg.convert(nn.Sequential(nn.Conv2d(8, 32, 1), nn.GELU(approximate='tanh'), behind).eval(), threshold=0.05,
                          generalGeometry=True)
        pkg.insertCBPointwise(seq, transcendental=True)
        assert type(seq[1]) is pkg.CBPointwise2d and seq[1].kind == ac.GELU_TANH and seq[0].propChangeIndexes
        assert seq[1].propChangeIndexes is flag, behind
    # without the keyword: as before
    for kw in (dict(), dict(transcendental=False)):
        net = _convnext(pkg)
        pkg.insertCBPointwise(net, **kw)
        pkg.insertCBChannelOps(net, layerNormTypes=(LayerNorm2d,))
        assert _names(net)[4:6] == [('gelu', 'GELU'), ('norm2', 'LayerNorm2d')] and not net.pw1.propChangeIndexes


def test_insert_on_a_monodepth_type_run(pkg, lib):
    """conv -> ELU -> ReflectionPad2d -> conv, a decoder step of monodepth2's kind; a batch norm in front of a Mish and
    subclasses next to it."""
    seq = nn.Sequential()
    for name, mod in (('c1', nn.Conv2d(8, 8, 3, padding=1)), ('elu', nn.ELU(inplace=True)), ('pad', nn.ReflectionPad2d(1)),
                      ('c2', nn.Conv2d(8, 4, 3)), ('bn', _bn(4)), ('mish', nn.Mish()), ('c3', nn.Conv2d(4, 4, 1)),
                      ('sp', nn.Softplus(2, 5))):
        seq.add_module(name, mod)
    net = pkg.convert(seq.eval(), threshold=0.05, generalGeometry=True)
    pkg.insertCBPointwise(net, transcendental=True)
    pkg.insertCBPadding(net)
    assert _names(net) == [('c1', 'CBConv2d'), ('elu', 'CBPointwise2d'), ('pad', 'CBPad2d'), ('c2', 'CBConv2d'),
                           ('bn', 'CBPointwise2d'), ('c3', 'CBConv2d'), ('sp', 'CBPointwise2d')]
    assert (net.elu.kind, net.elu.p0, net.elu.p1) == (ac.ELU, 1.0, 1.0) and net.c1.propChangeIndexes
    assert net.elu.propChangeIndexes      # (insertCBPadding's module takes the mask)
    assert net.bn.kind == ac.MISH and net.bn.scale is not None and net.bn.propChangeIndexes and net.c2.propChangeIndexes
    assert (net.sp.kind, net.sp.p0, net.sp.p1) == (ac.SOFTPLUS, 2.0, 5.0) and not net.sp.propChangeIndexes

    class MySELU(nn.SELU):
        pass
    seq = pkg.convert(nn.Sequential(nn.Conv2d(3, 4, 1), MySELU(), nn.Conv2d(4, 4, 1), nn.Softsign()).eval(), threshold=0.05)
    pkg.insertCBPointwise(seq, transcendental=True)
    assert [type(m).__name__ for m in seq] == ['CBConv2d', 'MySELU', 'CBConv2d', 'Softsign']
    assert not seq[0].propChangeIndexes and not seq[2].propChangeIndexes
    # a parameter the kernel refuses stops the pass with the constructor's sentence
    with pytest.raises(lib.CBinferError, match="beta=0 is not supported"):
        pkg.insertCBPointwise(pkg.convert(nn.Sequential(nn.Conv2d(3, 4, 1), nn.Softplus(beta=0)).eval(), threshold=0.05),
                              transcendental=True)


def test_pickle_state_helpers_and_batch_refusals(pkg, lib):
    m = pkg.CBPointwise2d(nn.GELU(approximate='tanh'), _bn(4), transcendental=True)
    m.propChangeIndexes, m.cloneOutput = True, False
    m.__dict__['_pwWork'] = {'key': None}
    c = pickle.loads(pickle.dumps(m))
    assert type(c) is pkg.CBPointwise2d and (c.kind, c.propChangeIndexes, c.cloneOutput) == (ac.GELU_TANH, True, False)
    assert c._pwWork is None and c.outputState.numel() == 0 and repr(c) == repr(m) and 'act=GELU' in repr(c)
    assert torch.equal(c.scale, m.scale) and torch.equal(c.shift, m.shift) and c.slope is None
    m.outputState = torch.ones(1, 4, 3, 3)
    net = nn.Sequential(m)
    assert any(t is m.outputState for t in pkg.getStateTensors(net))
    pkg.clearMemory(net)
    assert m.outputState.numel() == 0 and m._pwWork is None
    with pytest.raises(lib.CBinferError, match="HIP devices only"):
        m(torch.zeros(1, 4, 5, 6))
    net = pkg.insertCBPointwise(pkg.convert(nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), nn.Mish()).eval(), threshold=0.05),
                                transcendental=True)
    with pytest.raises(lib.CBinferError, match=r"SequenceBatch: layer '1' is CBPointwise2d \(act=Mish"):
        pkg.SequenceBatch(net, 2)
    with pytest.raises(lib.CBinferError, match=r"BranchGroup: layer '0.1' is CBPointwise2d"):
        pkg.BranchGroup([net])


def test_the_measuring_tool_uses_the_common_method(monkeypatch):
    """tools/target_activation.py, as tests/test_host_targets.py asks of the *_target.py tools: importing it touches no
    device, and the parts of the measuring method it names are tools/target_common.py's own objects."""
    import importlib
    import os
    import sys
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import target_common as tc

    def touched(*args, **kwargs):
        raise AssertionError("importing target_activation initialises the device")
    monkeypatch.setattr(torch.cuda, "_lazy_init", touched)
    sys.modules.pop("target_activation", None)
    mod = importlib.import_module("target_activation")
    assert callable(mod.main) and mod.rounds is tc.rounds and mod.fmt is tc.fmt
    for attr in ("timed", "rounds", "change_sets", "pack", "fmt", "BATCH", "SETS"):
        if hasattr(mod, attr):
            assert getattr(mod, attr) is getattr(tc, attr), attr
    assert [(name, Cn, H, W, fns) for name, Cn, H, W, _, fns in mod.LAYERS] == [
        ("64 ch", 64, 80, 120, ("GELU", "ELU", "Mish")), ("128 ch", 128, 40, 60, ("GELU",))]
