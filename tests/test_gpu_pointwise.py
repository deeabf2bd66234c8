"""-m gpu tests of the change-based element-wise functions (CBPointwise2d; cb_pointwise.hip).  The
specification is the numpy twin of tests/pointwise_cases.py (rules 1-3 there): the seven kinds without a transcendental
function are compared bit for bit, with and without the affine; SIGMOID / SILU / TANH against float64 math under the
bound derived at test_sigmoid_silu_tanh_against_float64."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import pointwise_cases as pc
from optest import (chain_frames, dev, dev_words, host_words, LayerSpy, lib,      # noqa: F401  (fixtures)
                    operand_args, gpu_pkg as pkg, raw, share_of, stream, walk_frames)

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float16]
WORST = {}      # (kind name, dtype name) -> worst err / |ref| seen against float64
FILL = {np.float32: 0x5BCD5BCD, np.float16: 0x5BCD}


def run_frames(lib, shape, dtype, form, kind, p0, p1, affine, rng, check, span=8.0, special=None):
    """The six mask patterns as consecutive frames through cbinfer_cbpointwise_forward.  Before every frame x gets new
    values at the frame's pixels AND at one pixel outside them; check(x, out at the listed pixels [C, n], where) judges
    the values; unlisted pixels must keep their bits, maskCopy be the frame's mask, the working mask zero: the walk of
    optest.walk_frames, the per-channel parameters drawn in front of it."""
    C, ptr = lib.C, lib.ptr
    Cn, H, W = shape
    scale, shift, slope = pc.per_channel(rng, Cn)
    dscale, dshift, dslope = (dev(v) for v in (scale, shift, slope))
    out = np.empty(shape, dtype=dtype)
    pc.bits_of(out)[...] = FILL[dtype] & (0xFFFFFFFF if dtype == np.float32 else 0xFFFF)

    def call(dx, dout, mask, lst, cap, cnt, bits, mcopy):
        return C.cbinfer_cbpointwise_forward(ptr(dx), ptr(dout), ptr(mask), ptr(lst), cap, ptr(cnt), ptr(bits), ptr(mcopy),
                                             Cn, H, W, kind, p0, p1, ptr(dscale) if affine else None,
                                             ptr(dshift) if affine else None, ptr(dslope) if kind == pc.PRELU else None,
                                             lib.CB_F32 if dtype == np.float32 else lib.CB_F16, stream())

    def judge(x, got, listed, where):
        check(x, got, listed, where, scale if affine else None, shift if affine else None, slope)
    return walk_frames(lib, shape, dtype, form, lambda: pc.patterns(rng, H, W), call, judge, out,
                       lambda: pc.values(rng, shape, dtype, span, special), what=(pc.NAMES[kind], affine))


@pytest.mark.parametrize("form", pc.FORMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
def test_exact_kinds_equal_the_twin_bit_for_bit(lib, dtype, form):
    """Every shape of pointwise_cases.SHAPES, the seven kinds without a transcendental function, with and without the
    affine: at the listed pixels the state has the twin's bits (NaNs in the same positions), -0, +-inf, +-1e30 and
    +-65504 among the values; everything else as run_frames says.  A contracted FMA in the affine would show here (a
    third of the values differ, tests/test_host_pointwise.py)."""
    rng = np.random.default_rng(11)
    saw = 0
    for shape in pc.SHAPES:
        for kind, p0, p1 in pc.EXACT:
            for affine in (False, True):
                def check(x, got, listed, where, scale, shift, slope, kind=kind, p0=p0, p1=p1):
                    want = pc.twin(x, kind, p0, p1, scale, shift, slope)
                    g, w = got[:, listed], want[:, listed]
                    nan = np.isnan(w)
                    bad = (np.isnan(g) != nan) | ((pc.bits_of(g) != pc.bits_of(w)) & ~nan)
                    assert not bad.any(), (where, int(bad.sum()), x[:, listed][bad][:4], g[bad][:4], w[bad][:4])
                saw += run_frames(lib, shape, dtype, form, kind, p0, p1, affine, rng, check)
    assert form == "all" or saw >= 4 * len(pc.SHAPES) * len(pc.EXACT) * 2


@pytest.mark.parametrize("form", pc.FORMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
def test_sigmoid_silu_tanh_against_float64(lib, dtype, form):
    """SIGMOID 1 / (1 + expf(-v)), SILU v / (1 + expf(-v)), TANH tanhf(v) against the same formula in float64:
        |err| <= c 2^-24 |ref| + 2^-126,    for fp16 plus 2^-11 |ref| + 2^-24 (the one rounding to f16; 2^-24 its
    smallest subnormal).  c in units of 2^-24 = half an ulp of a float32 result, i.e. what one correctly rounded
    operation adds.  ROCm ships no table of ulp errors for its device functions under its installation directory
    (neither headers nor documents state one for __ocml_exp_f32 / __ocml_tanh_f32), so the limits are those of the OpenCL
    full profile, which OCML is built to: exp 3 ulp, tanh 5 ulp; taken twice, and an ulp is two units:
        SIGMOID  -v is exact; e = expf(-v): 2 * 3 ulp = 12 units; s = 1 + e: the error of e enters s with weight
                 e / (1 + e) <= 1, plus 1 unit for the addition; 1 / s: plus 1 unit.           c = 12 + 1 + 1 = 14
        SILU     the same with the exact v as the numerator.                                   c = 14
        TANH     tanhf alone: 2 * 5 ulp.                                                       c = 20
    (first order; the products of two such terms are below 2^-40 |ref| and lie inside the doubling.)  Inputs in
    [-20, 20] plus +-inf and NaN, so that the float64 reference is a normal float32 number or exactly 0 / +-1; where the
    reference is not finite (SILU(+inf) = +inf, SILU(-inf) = -inf / inf = NaN, a NaN input) the result must be the same
    infinity or a NaN.  c is not tuned: a failure is a finding.  The worst err / |ref| seen is printed and reported in
    DESIGN 5.16."""
    C14 = {pc.SIGMOID: 14.0, pc.SILU: 14.0, pc.TANH: 20.0}
    rng = np.random.default_rng(13)
    special = np.array([np.inf, -np.inf, np.nan, 20.0, -20.0, 0.0, -0.0], dtype=dtype)
    for shape in pc.SHAPES:
        for kind, p0, p1 in pc.INEXACT:
            def check(x, got, listed, where, scale, shift, slope, kind=kind):
                xs = x[:, listed]
                ref = pc.reference64(xs, kind)
                g = got[:, listed].astype(np.float64)
                fin = np.isfinite(ref)
                assert np.array_equal(np.isnan(g), np.isnan(ref)), where
                assert np.array_equal(g[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)]), where
                err, mag = np.abs(g[fin] - ref[fin]), np.abs(ref[fin])
                bound = C14[kind] * 2.0 ** -24 * mag + 2.0 ** -126
                if x.dtype == np.float16:
                    bound = bound + 2.0 ** -11 * mag + 2.0 ** -24
                big = mag >= 2.0 ** -14      # (relative figures where an f16 result is a normal number too)
                if big.any():
                    key = (pc.NAMES[kind], np.dtype(x.dtype).name)
                    WORST[key] = max(WORST.get(key, 0.0), float((err[big] / mag[big]).max()))
                bad = err > bound
                assert not bad.any(), (where, int(bad.sum()), xs[fin][bad][:4], g[fin][bad][:4], ref[fin][bad][:4],
                                       float((err / bound).max()))
            run_frames(lib, shape, dtype, form, kind, p0, p1, False, rng, check, span=20.0, special=special)
    for (name, dt), rel in sorted(WORST.items()):
        if dt == np.dtype(dtype).name:
            print("%s %s %s: worst err / |ref| = %.3g = %.2f x 2^-24" % (name, dt, form, rel, rel * 2.0 ** 24))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
def test_a_pixel_does_not_depend_on_the_list_the_form_or_the_run(lib, dtype):
    """One pixel's bits -- all ten kinds, with the affine -- listed alone in a mask, in a list among others, in another
    list, with every pixel listed, and all of that a second time: always the same bits."""
    C, ptr = lib.C, lib.ptr
    Cn, H, W = 300, 5, 130
    rng = np.random.default_rng(17)
    x = pc.values(rng, (Cn, H, W), dtype, 8.0, np.array([0.0, -0.0, 3.0, -3.0, 6.0], dtype=dtype))
    scale, shift, slope = pc.per_channel(rng, Cn)
    dx, dscale, dshift, dslope = dev(x), dev(scale), dev(shift), dev(slope)
    py, px = 3, 64
    alone = np.zeros((H, W), dtype=bool)
    alone[py, px] = True
    crowd = rng.random((H, W)) < 0.5
    crowd[py, px] = True
    row = np.zeros((H, W), dtype=bool)
    row[py, :] = True
    words = C.cbinfer_mask_words(H, W)
    for kind, p0, p1 in pc.EXACT + pc.INEXACT:
        seen = []
        for rep in range(2):
            for form, S in (("mask", alone), ("list", crowd), ("list", row), ("mask", row), ("all", alone)):
                dout = torch.zeros((Cn, H, W), dtype=dx.dtype, device="cuda")
                bits = torch.zeros(words, dtype=torch.int64, device="cuda")
                mcopy = torch.zeros(words, dtype=torch.int64, device="cuda")
                mask, lst, cap, cnt = operand_args(form, S, 0, bool(rep % 2))
                st = C.cbinfer_cbpointwise_forward(ptr(dx), ptr(dout), ptr(mask), ptr(lst), cap, ptr(cnt), ptr(bits),
                                                   ptr(mcopy), Cn, H, W, kind, p0, p1, ptr(dscale), ptr(dshift),
                                                   ptr(dslope) if kind == pc.PRELU else None,
                                                   lib.CB_F32 if dtype == np.float32 else lib.CB_F16, stream())
                assert st == 0
                seen.append(pc.bits_of(dout[:, py, px].cpu().numpy()).copy())
        assert all(np.array_equal(s, seen[0]) for s in seen[1:]), pc.NAMES[kind]
        assert len(np.unique(seen[0])) > 1, pc.NAMES[kind]


def test_pointwise_changed_takes_the_mask_as_the_working_mask(lib):
    """cbinfer_pointwise_changed alone: the listed pixels given in `bits` (what a list leaves there), a second set in
    the operand's mask; both are recomputed, the working mask comes back zero and the union is handed on."""
    C, ptr = lib.C, lib.ptr
    Cn, H, W = 3, 4, 70
    rng = np.random.default_rng(5)
    x = pc.values(rng, (Cn, H, W), np.float32)
    A, B = rng.random((H, W)) < 0.2, rng.random((H, W)) < 0.2
    dx, dout = dev(x), torch.zeros((Cn, H, W), device="cuda")
    bits, mask = dev_words(pc.pack(A)), dev_words(pc.pack(B))
    mcopy = torch.zeros(C.cbinfer_mask_words(H, W), dtype=torch.int64, device="cuda")
    assert C.cbinfer_pointwise_changed(ptr(dx), ptr(dout), ptr(mask), 0, ptr(bits), ptr(mcopy), Cn, H, W, pc.HARDSWISH,
                                       0.0, 0.0, None, None, None, lib.CB_F32, stream()) == 0
    got, want = dout.cpu().numpy(), pc.twin(x, pc.HARDSWISH)
    U = A | B
    assert pc.same_bits(got[:, U], want[:, U]) and not pc.bits_of(got)[:, ~U].any()
    assert int(bits.ne(0).sum()) == 0 and np.array_equal(host_words(mcopy), pc.pack(U))
    assert np.array_equal(host_words(mask), pc.pack(B))      # (the operand's mask is read only)


def _bn(Cn, seed):
    g = torch.Generator().manual_seed(seed)
    bn = nn.BatchNorm2d(Cn, eps=1e-3)
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(Cn, generator=g) * 0.3)
        bn.running_var.copy_(torch.rand(Cn, generator=g) * 2 + 0.05)
        bn.weight.copy_(torch.randn(Cn, generator=g))
        bn.bias.copy_(torch.randn(Cn, generator=g))
    return bn.eval()


def module_twin(m, x):
    """The twin of the module `m` on the numpy map x [C, H, W]."""
    np_ = (lambda t: None if t is None else t.detach().cpu().numpy())
    slope = np_(m.slope)
    if slope is not None and slope.size == 1:
        slope = np.repeat(slope, x.shape[0])
    return pc.twin(x, m.kind, m.p0, m.p1, np_(m.scale), np_(m.shift), slope)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
def test_module_forms_flags_and_errors(pkg, lib, dtype):
    """CBPointwise2d: a new state is written completely whatever the list says; a MaskChangeIndexes is taken as its mask
    and its list never made; ChangeIndexes and exact tensors as lists; the flags of CBAdd2d; reallocation on a new
    resolution; clearMemory; a one-parameter PReLU broadcast by the host; the refusals."""
    from cbinfer_amd.conv2d_cg import ChangeIndexes, MaskChangeIndexes
    Cn, H, W = 5, 7, 70
    rng = np.random.default_rng(3)
    tdt = torch.float32 if dtype == np.float32 else torch.float16
    for act, norm in ((nn.Hardtanh(-1.5, 2.25), None), (nn.PReLU(), _bn(Cn, 1)), (None, _bn(Cn, 2)),
                      (nn.PReLU(Cn).to(tdt), None)):
        if act is not None and type(act) is nn.PReLU:
            with torch.no_grad():
                act.weight.copy_(torch.linspace(-0.4, 0.3, act.weight.numel()))
        m = pkg.CBPointwise2d(act, norm).cuda()
        m.propChangeIndexes = True
        x = pc.values(rng, (Cn, H, W), dtype)
        empty = torch.zeros(0, dtype=torch.int32, device="cuda")
        tag, y, ix = m(('changeIndexes', dev(x)[None], empty))      # first frame
        assert tag == 'changeIndexes' and pc.same_bits(m.outputState[0].cpu().numpy(), module_twin(m, x))
        assert y is not m.outputState and torch.equal(raw(y), raw(m.outputState))
        assert isinstance(ix, MaskChangeIndexes) and ix.size == (H, W) and not ix._made
        assert ix.tensor().numel() == H * W
        for t in range(4):
            prev = m.outputState[0].cpu().numpy()
            S = rng.random((H, W)) < 0.1
            if t == 3:
                S[:] = False
            fresh = pc.values(rng, (Cn, H, W), dtype)
            x[:, S] = fresh[:, S]
            if not S[6, 69]:
                x[:, 6, 69] = fresh[:, 6, 69]      # (not listed)
            if t % 2 == 0:
                ind = MaskChangeIndexes(dev_words(pc.pack(S)), (H, W), torch.empty(H * W, dtype=torch.int32, device="cuda"),
                                        torch.zeros(1, dtype=torch.int32, device="cuda"))
            else:
                lb = dev(np.flatnonzero(S.reshape(-1)).astype(np.int32))
                ind = lb if t == 3 else ChangeIndexes(torch.cat([lb, lb.new_full((3,), 6 * W + 69)]),
                                                      torch.tensor([lb.numel()], dtype=torch.int32, device="cuda"), (H, W))
            tag, y, ix = m(('changeIndexes', dev(x)[None], ind))
            if t % 2 == 0:
                assert not ind._made      # the producer's list was never materialised
            got, want = m.outputState[0].cpu().numpy(), module_twin(m, x)
            assert pc.same_bits(got[:, S], want[:, S]), (act, t)
            assert np.array_equal(pc.bits_of(got)[:, ~S], pc.bits_of(prev)[:, ~S]), (act, t)
            assert np.array_equal(host_words(ix._mask), pc.pack(S))
            assert np.array_equal(ix.tensor().cpu().numpy(), np.flatnonzero(S.reshape(-1))), (act, t)
            assert int(m._pwWork['bits'].ne(0).sum()) == 0
        # a bare tensor carries no change information: the dense result; the state itself is handed out, tagged
        m.propChangeIndexes, m.cloneOutput = False, False
        out = m(dev(x)[None])
        assert out is m.outputState and out._cbinfer_inplace_state
        assert pc.same_bits(out[0].cpu().numpy(), module_twin(m, x))
        # a new resolution: the state and the work buffers are made again, the frame is dense whatever the list says
        x2 = pc.values(rng, (Cn, 3, 9), dtype)
        out = m(('changeIndexes', dev(x2)[None], empty))
        assert tuple(out.shape) == (1, Cn, 3, 9) and m._pwWork['key'][:3] == (Cn, 3, 9)
        assert pc.same_bits(out[0].cpu().numpy(), module_twin(m, x2))
        # refusals
        Err = lib.CBinferError
        dx = dev(x2)[None]
        wrong = ChangeIndexes(torch.zeros(4, dtype=torch.int32, device="cuda"),
                              torch.zeros(1, dtype=torch.int32, device="cuda"), (4, 9))
        with pytest.raises(Err, match="4x9 map.*3x9"):
            m(('changeIndexes', dx, wrong))
        with pytest.raises(Err, match="int32"):
            m(('changeIndexes', dx, torch.zeros(3, dtype=torch.int64, device="cuda")))
        with pytest.raises(Err, match="device"):
            m(('changeIndexes', dx, torch.zeros(3, dtype=torch.int32)))
        with pytest.raises(Err, match="int32 tensor or a ChangeIndexes"):
            m(('changeIndexes', dx, [1, 2]))
        if m.scale is not None or (m.slope is not None and m.slope.numel() > 1):
            with pytest.raises(Err, match="the input has 4 channels"):
                m(dx[:, :4].contiguous())
        with pytest.raises(Err, match=r"\[1, C, H, W\]"):
            m(torch.cat([dx, dx]))
        with pytest.raises(Err, match="HIP devices only"):
            m(dx.cpu())
        if m.scale is not None:
            with pytest.raises(Err, match=r"move the module with \.to\(\)"):
                copy.deepcopy(m).cpu()(dx)
        before = m.outputState.clone()
        torch.cuda.synchronize()
        assert torch.equal(raw(m.outputState), raw(before))
        m.clearMemory()
        assert m.outputState.numel() == 0 and m._pwWork is None
        out = m(dx)
        assert pc.same_bits(out[0].cpu().numpy(), module_twin(m, x2))


# ------------------------------------------------------------------------------------------------ a MobileNetV3-type chain
class DenseAct(nn.Module):
    """torch's dense operators in the place of a CBPointwise2d, the producer's changes handed through untouched.  The
    operators are torch's CPU ones, which the twin is pinned to bit for bit (tests/test_host_pointwise.py); the affine is
    two float32 torch operators."""

    def __init__(self, m, fn):
        super(DenseAct, self).__init__()
        self.m, self.fn, self.propChangeIndexes = [m], fn, m.propChangeIndexes

    def forward(self, inp):
        x, ix = (inp[1], inp[2]) if type(inp) == tuple else (inp, None)
        m = self.m[0]
        v = x.detach().cpu()
        if m.scale is not None:
            v = (v.float() * m.scale.cpu().view(1, -1, 1, 1) + m.shift.cpu().view(1, -1, 1, 1))
            y = self.fn(v).to(x.dtype).cuda()
        else:
            y = self.fn(v).cuda()
        return ('changeIndexes', y, ix) if self.propChangeIndexes else y


def make_chain(pkg, tdt):
    """CBConv2d 1x1 -> Hardswish -> 3x3 depthwise -> BN + ReLU6 -> 1x1 CBConv2d, every threshold 0."""
    torch.manual_seed(91)
    src = nn.Sequential()
    for name, mod in (('expand', nn.Conv2d(8, 16, 1)), ('hs', nn.Hardswish()), ('dw', nn.Conv2d(16, 16, 3, 1, 1, groups=16)),
                      ('bn', _bn(16, 7)), ('relu6', nn.ReLU6()), ('project', nn.Conv2d(16, 8, 1))):
        src.add_module(name, mod)
    src = src.eval().cuda().to(tdt)
    with torch.no_grad():
        src.expand.weight.mul_(4.0)      # (values on both sides of -3 and 3)
        src.dw.weight.mul_(3.0)
    net = pkg.convert(src, threshold=0.0, depthwise=True)
    assert [type(m).__name__ for m in net] == ['CBConv2d', 'Hardswish', 'CBDepthwiseConv2d', 'BatchNorm2d', 'ReLU6',
                                               'CBConv2d']
    return net


def link_chain(pkg, net, cloneOutput):
    pkg.linkDepthwise(pkg.insertCBPointwise(net))
    assert [(n, type(m).__name__) for n, m in net.named_children()] == [
        ('expand', 'CBConv2d'), ('hs', 'CBPointwise2d'), ('dw', 'CBDepthwiseConv2d'), ('bn', 'CBPointwise2d'),
        ('project', 'CBConv2d')]
    assert net.expand.propChangeIndexes and net.hs.propChangeIndexes and net.dw.propChangeIndexes
    assert net.bn.propChangeIndexes and net.dw.propagatedChanges and not net.project.propChangeIndexes
    assert net.hs.kind == pc.HARDSWISH and net.bn.kind == pc.HARDTANH and (net.bn.p0, net.bn.p1) == (0.0, 6.0)
    for m in net:
        m.cloneOutput = cloneOutput
    if next(net.parameters()).dtype == torch.float32:
        net.expand.exactF32 = net.project.exactF32 = True
    return net


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
def test_chain_equals_the_chain_with_dense_activations(pkg, lib, dtype, monkeypatch):
    """Six frames: the chain with CBPointwise2d modules against the same chain -- a deep copy made before the first
    frame -- whose activations are torch's dense operators, bit for bit in the output and in every state; every
    CBPointwise2d's state is the dense operator on its own operand.  Behind the first layer nothing detects: the two
    element-wise modules make one cbinfer_cbpointwise_forward call per frame, the depthwise layer one propagated call,
    and no call behind the first layer carries `detect` in its name."""
    import cbinfer_amd.conv2d as convmod
    import cbinfer_amd.conv2d_cg as cgmod
    import cbinfer_amd.dwconv as dwmod
    import cbinfer_amd.pointwise as pwmod
    tdt = torch.float32 if dtype == np.float32 else torch.float16
    net = link_chain(pkg, make_chain(pkg, tdt), True)
    dense = copy.deepcopy(net)
    dense.hs = DenseAct(net.hs, F.hardswish)
    dense.bn = DenseAct(net.bn, F.relu6)
    spy = LayerSpy(lib.C)
    for mod in (convmod, cgmod, dwmod, pwmod):
        monkeypatch.setattr(mod, 'C', spy)
    hooks = []
    for name, m in net.named_children():
        hooks.append(m.register_forward_pre_hook(lambda mod, args, name=name: spy.layer.__setitem__(0, name)))
    frames = chain_frames(np.random.default_rng(19), 6, dtype)
    share = []
    with torch.no_grad():
        for t, f in enumerate(frames):
            y = net(f)
            spy.layer[0] = 'dense'
            yd = dense(f)
            assert tuple(y.shape) == (1, 8, 20, 70) and torch.equal(raw(y), raw(yd)), t
            for name in ('hs', 'bn'):
                state = getattr(net, name).outputState
                src = net.expand.prevOutput if name == 'hs' else net.dw.prevOutput
                ref = module_twin(getattr(net, name), src[0].cpu().numpy())
                assert pc.same_bits(state[0].cpu().numpy(), ref), (name, t)
            assert torch.equal(raw(net.dw.prevOutput), raw(dense.dw.prevOutput)), t
            assert torch.equal(raw(net.project.prevOutput), raw(dense.project.prevOutput)), t
            share.append(share_of(net.bn._pwWork['copy'], 20, 70))
    for h in hooks:
        h.remove()
    print("listed share per frame:", ["%.2f" % s for s in share], {k: v for k, v in spy.calls.items() if k != 'dense'})
    assert share[0] == 1.0 and 0 < min(share[1:]) and max(share[1:]) < 0.5, share
    assert spy.calls['hs'] == {'cbinfer_cbpointwise_forward': 6} and spy.calls['bn'] == {'cbinfer_cbpointwise_forward': 6}
    assert spy.calls['dw'] == {'cbinfer_cbdwconv2d_forward_propagated': 6}
    assert spy.calls['project'] and not any('detect' in n for n in spy.calls['project'])
    assert net.dw.prevInput.numel() == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
def test_chain_records_as_a_launch_program(pkg, lib, dtype):
    """With cloneOutput=False the chain is library calls only: FrameProgram records it, each CBPointwise2d is ONE call
    of the recorded frame, three replayed frames equal the eager network in outputs and states bit for bit."""
    tdt = torch.float32 if dtype == np.float32 else torch.float16
    net = link_chain(pkg, make_chain(pkg, tdt), False)
    frames = chain_frames(np.random.default_rng(23), 7, dtype)
    with torch.no_grad():
        for f in frames[:4]:
            net(f)
        eager = copy.deepcopy(net)
        prog = pkg.FrameProgram(net)
        for t, f in enumerate(frames[4:]):
            yp, ye = prog(f), eager(f)
            assert torch.equal(raw(yp), raw(ye)), t
            for ta, tb in zip(pkg.getStateTensors(net), pkg.getStateTensors(eager)):
                assert torch.equal(ta, tb), t
        raws = [fn for fn, _ in prog.calls]
        assert raws.count(lib.C.cbinfer_cbpointwise_forward.raw) == 2
        assert raws.count(lib.C.cbinfer_cbdwconv2d_forward_propagated.raw) == 1
        assert len(pkg.getStateTensors(net)) == 2 * 2 + 2 + 2      # two convs, the depthwise layer, two pointwise states


def test_chain_with_torch_activations_is_refused_by_frame_program(pkg, lib):
    """What the activations cost without CBPointwise2d: the same converted layers with torch's Hardswish, BatchNorm2d
    and ReLU6 between them cannot be recorded."""
    net = make_chain(pkg, torch.float32)
    for m in net:
        if hasattr(m, 'cloneOutput'):
            m.cloneOutput = False
    frames = chain_frames(np.random.default_rng(29), 4, np.float32)
    with torch.no_grad():
        for f in frames[:3]:
            net(f)
        with pytest.raises(lib.CBinferError, match="torch operators.*CBPointwise2d"):
            pkg.FrameProgram(net).record(frames[3])


def test_worst_figures_are_reported():
    """The worst err / |ref| of SIGMOID / SILU / TANH over the tests above, in units of 2^-24: measurements, not bars
    (the bars are 14, 14 and 20 units, for fp16 plus 2^13 units of the rounding to f16)."""
    for (name, dt), rel in sorted(WORST.items()):
        print("%-8s %-8s worst err / |ref| = %.3g = %.2f x 2^-24" % (name, dt, rel, rel * 2.0 ** 24))
    assert WORST
