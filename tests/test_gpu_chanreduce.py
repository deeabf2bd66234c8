"""-m gpu tests of the change-based per-pixel channel reductions (CBChannelReduce2d; cb_chanreduce.hip).
The specification is the numpy twin of tests/chanreduce_cases.py (rules 1-3 there): LAYERNORM (with and without the
affine) and L2NORM are compared bit for bit; SOFTMAX / LOGSOFTMAX, which call the device's expf / logf, against float64
math under chanreduce_cases.bound."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import chanreduce_cases as cc
from optest import (chain_frames, dev, dev_words, host_words, LayerSpy, lib,      # noqa: F401  (fixtures)
                    operand_args, gpu_pkg as pkg, raw, share_of, stream, walk_frames)

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float16]
WORST = {}      # (kind name, dtype name) -> worst err / bound seen against float64
FILL = {np.float32: 0x5BCD5BCD, np.float16: 0x5BCD}
EXACT = [(cc.LAYERNORM, False), (cc.LAYERNORM, True), (cc.L2NORM, False)]
INEXACT = [(cc.SOFTMAX, False), (cc.LOGSOFTMAX, False)]


class LayerNorm2d(nn.Module):
    """A channels-first layer norm as ConvNeXt implementations write it: .weight, .bias, .eps (torch has no such class)."""

    def __init__(self, C, eps=1e-6):
        super(LayerNorm2d, self).__init__()
        self.weight = nn.Parameter(torch.linspace(0.5, 1.5, C))
        self.bias = nn.Parameter(torch.linspace(-0.3, 0.4, C))
        self.eps, self.C = eps, C

    def forward(self, x):
        return F.layer_norm(x.permute(0, 2, 3, 1), (self.C,), self.weight, self.bias, self.eps).permute(0, 3, 1, 2)


def forward(lib, dx, dout, args, bits, mcopy, kind, eps, dgamma, dbeta):
    """cbinfer_cbchanreduce_forward with the operand `args` = (mask, list, capacity, device count)."""
    Cn, H, W = dx.shape
    mask, lst, cap, cnt = args
    ptr = lib.ptr
    return lib.C.cbinfer_cbchanreduce_forward(ptr(dx), ptr(dout), ptr(mask), ptr(lst), cap, ptr(cnt), ptr(bits), ptr(mcopy),
                                              Cn, H, W, kind, eps, ptr(dgamma), ptr(dbeta),
                                              lib.CB_F32 if dx.dtype == torch.float32 else lib.CB_F16, stream())


def run_frames(lib, shape, dtype, form, kind, affine, rng, check):
    """The six mask patterns as consecutive frames through cbinfer_cbchanreduce_forward.  Before every frame x gets new
    values at the frame's pixels AND at one pixel outside them; check(x, out, listed, where, gamma, beta) judges the
    values at the listed pixels; unlisted pixels must keep their bits, maskCopy be the frame's mask, the working mask
    zero (optest.walk_frames); three quarters of the listed pixels must be finite.  Returns the number of frames with an
    unlisted pixel."""
    Cn, H, W = shape
    gamma, beta = cc.affine(rng, Cn)
    dgamma, dbeta = (dev(gamma), dev(beta)) if affine else (None, None)
    eps = cc.EPS[kind]
    out = np.empty(shape, dtype=dtype)
    cc.bits_of(out)[...] = FILL[dtype]
    n = {'listed': 0, 'finite': 0}

    def call(dx, dout, mask, lst, cap, cnt, bits, mcopy):
        return forward(lib, dx, dout, (mask, lst, cap, cnt), bits, mcopy, kind, eps, dgamma, dbeta)

    def judge(x, got, listed, where):
        check(x, got, listed, where, gamma if affine else None, beta if affine else None)
        n['listed'] += int(listed.sum())
        n['finite'] += int(cc.finite_pixels(x)[listed].sum())
    saw = walk_frames(lib, shape, dtype, form, lambda: cc.patterns(rng, H, W), call, judge, out,
                      lambda: cc.values(rng, shape, dtype), what=(cc.NAMES[kind], affine))
    # (the bit and bound checks must see finite pixels: the special values are placed per pixel)
    assert 4 * n['finite'] >= 3 * n['listed'], (shape, n)
    return saw


def check_twin(kind):
    def check(x, got, listed, where, gamma, beta):
        want = cc.twin(x[:, listed], kind, cc.EPS[kind], gamma, beta)
        g = got[:, listed]
        nan = np.isnan(want)
        bad = (np.isnan(g) != nan) | ((cc.bits_of(g) != cc.bits_of(want)) & ~nan)
        assert not bad.any(), (where, int(bad.sum()), x[:, listed][bad][:4], g[bad][:4], want[bad][:4])
    return check


def check_float64(kind):
    """SOFTMAX / LOGSOFTMAX at the listed pixels against the float64 formula: NaNs exactly where the reference has them
    -- a pixel holding a NaN or +inf is all NaN --, a -inf channel exactly 0 / -inf, every finite reference value under
    chanreduce_cases.bound.  A float16 result beyond the format's range is the infinity of that sign (65520 is where
    rounding to nearest leaves the finite numbers; within the bound of it either is right)."""
    def check(x, got, listed, where, gamma, beta):
        xs = x[:, listed]
        ref = cc.reference64(xs, kind)
        g = got[:, listed].astype(np.float64)
        bnd = cc.bound(xs, kind, ref)
        nan = np.isnan(ref)
        assert np.array_equal(np.isnan(g), nan), where
        poisoned = (np.isnan(xs) | (xs == np.inf)).any(axis=0)
        assert nan[:, poisoned].all() and not nan[:, ~poisoned & ~(xs == -np.inf).all(axis=0)].any(), where
        low = (xs == -np.inf) & ~nan
        assert np.array_equal(g[low], np.full(int(low.sum()), 0.0 if kind == cc.SOFTMAX else -np.inf)), where
        fin = np.isfinite(ref)
        assert np.array_equal(g[~fin & ~nan], ref[~fin & ~nan]), where
        with np.errstate(all='ignore'):
            err = np.abs(g - ref)
            if x.dtype == np.float16:
                sure, maybe = fin & (np.abs(ref) - bnd >= 65520.0), fin & (np.abs(ref) + bnd >= 65520.0)
                assert np.array_equal(g[sure], np.sign(ref[sure]) * np.inf), where
                fin = fin & ~sure & ~(maybe & (g == np.sign(ref) * np.inf))
        bad = fin & ~(err <= bnd)
        if fin.any():
            key = (cc.NAMES[kind], np.dtype(x.dtype).name)
            WORST[key] = max(WORST.get(key, 0.0), float((err[fin] / bnd[fin]).max()))
        assert not bad.any(), (where, int(bad.sum()), g[bad][:4], ref[bad][:4], float((err[fin] / bnd[fin]).max()))
    return check


@pytest.mark.parametrize("form", cc.FORMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
def test_layernorm_and_l2norm_equal_the_twin_bit_for_bit(lib, dtype, form):
    """Every shape of chanreduce_cases.SHAPES; LAYERNORM with and without the affine, and L2NORM: at the listed pixels
    the state has the twin's bits (NaNs in the same positions), -0, +-inf, +-1e30 and +-65504 among the values;
    everything else as run_frames says.  A contracted FMA, another summation order or an approximate division or square
    root would show here."""
    rng = np.random.default_rng(11)
    saw = 0
    for shape in cc.SHAPES:
        for kind, affine in EXACT:
            saw += run_frames(lib, shape, dtype, form, kind, affine, rng, check_twin(kind))
    assert form == "all" or saw >= 4 * len(cc.SHAPES) * len(EXACT)


@pytest.mark.parametrize("form", cc.FORMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
def test_softmax_kinds_against_float64(lib, dtype, form):
    """SOFTMAX and LOGSOFTMAX against the float64 formula under the bounds derived at chanreduce_cases.bound (expf / logf
    at the OpenCL full profile's 3 ulp, taken twice).  The bounds are not tuned: a failure is a finding.  The worst
    err / bound seen is printed and reported in DESIGN 5.21."""
    rng = np.random.default_rng(13)
    for shape in cc.SHAPES:
        for kind, _ in INEXACT:
            run_frames(lib, shape, dtype, form, kind, False, rng, check_float64(kind))
    for (name, dt), w in sorted(WORST.items()):
        if dt == np.dtype(dtype).name:
            print("%s %s %s: worst err / bound = %.3f" % (name, dt, form, w))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
def test_channel_counts_on_both_sides_of_the_kernels_thresholds(lib, dtype):
    """The launch decides by C alone what the LDS holds over the passes: everything up to C = 192, the values of a word
    with at most 16 listed pixels up to C = 768, nothing beyond (cb_chanreduce.hip).  C on both sides of either
    threshold, all kinds, the six patterns (words of 64, of 6 and of one or two listed pixels): the same checks as
    above."""
    rng = np.random.default_rng(23)
    for Cn in (192, 193, 768, 769):
        for kind, affine in EXACT:
            run_frames(lib, (Cn, 2, 70), dtype, "mask", kind, affine, rng, check_twin(kind))
        for kind, _ in INEXACT:
            run_frames(lib, (Cn, 2, 70), dtype, "list", kind, False, rng, check_float64(kind))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
def test_a_pixel_does_not_depend_on_the_list_the_form_or_the_run(lib, dtype):
    """One pixel's bits, all four kinds (LAYERNORM with the affine), C = 300: listed alone (one bit in its word), in a
    list of at most 16 in its word, in a half-full random crowd, in a full row, and with every pixel listed, each twice:
    always the same bits.  This is the test a summation order that depends on the word's popcount fails."""
    Cn, H, W = 300, 5, 130
    rng = np.random.default_rng(17)
    x = cc.values(rng, (Cn, H, W), dtype, 8.0, np.array([0.0, -0.0, 3.0, -3.0, 6.0], dtype=dtype))
    gamma, beta = cc.affine(rng, Cn)
    dx, dgamma, dbeta = dev(x), dev(gamma), dev(beta)
    py, px = 3, 70
    alone = np.zeros((H, W), dtype=bool)
    alone[py, px] = True
    few = alone.copy()
    few[py, 64:128:7] = True
    assert 1 < few[py, 64:128].sum() <= 16
    crowd = rng.random((H, W)) < 0.5
    crowd[py, px] = True
    assert 16 < crowd[py, 64:128].sum() < 64
    row = np.zeros((H, W), dtype=bool)
    row[py, :] = True
    words = lib.C.cbinfer_mask_words(H, W)
    for kind in range(4):
        seen = []
        for rep in range(2):
            for form, S in (("mask", alone), ("list", alone), ("mask", few), ("list", few), ("list", crowd),
                            ("mask", crowd), ("list", row), ("mask", row), ("all", alone)):
                dout = torch.zeros((Cn, H, W), dtype=dx.dtype, device="cuda")
                bits = torch.zeros(words, dtype=torch.int64, device="cuda")
                mcopy = torch.zeros(words, dtype=torch.int64, device="cuda")
                aff = kind == cc.LAYERNORM
                st = forward(lib, dx, dout, operand_args(form, S, 0, bool(rep % 2)), bits, mcopy, kind, cc.EPS[kind],
                             dgamma if aff else None, dbeta if aff else None)
                assert st == 0
                seen.append(cc.bits_of(dout[:, py, px].cpu().numpy()).copy())
        assert all(np.array_equal(s, seen[0]) for s in seen[1:]), cc.NAMES[kind]
        assert len(np.unique(seen[0])) > 1, cc.NAMES[kind]


def test_chanreduce_changed_takes_the_mask_as_the_working_mask(lib):
    """cbinfer_chanreduce_changed alone: the listed pixels given in `bits` (what a list leaves there), a second set in
    the operand's mask; both are recomputed, the working mask comes back zero and the union is handed on."""
    C, ptr = lib.C, lib.ptr
    Cn, H, W = 19, 4, 70
    rng = np.random.default_rng(5)
    x = cc.values(rng, (Cn, H, W), np.float32)
    A, B = rng.random((H, W)) < 0.2, rng.random((H, W)) < 0.2
    gamma, beta = cc.affine(rng, Cn)
    dx, dout, dgamma, dbeta = dev(x), torch.zeros((Cn, H, W), device="cuda"), dev(gamma), dev(beta)
    bits, mask = dev_words(cc.pack(A)), dev_words(cc.pack(B))
    mcopy = torch.zeros(C.cbinfer_mask_words(H, W), dtype=torch.int64, device="cuda")
    assert C.cbinfer_chanreduce_changed(ptr(dx), ptr(dout), ptr(mask), 0, ptr(bits), ptr(mcopy), Cn, H, W, cc.LAYERNORM,
                                        1e-5, ptr(dgamma), ptr(dbeta), lib.CB_F32, stream()) == 0
    got, want = dout.cpu().numpy(), cc.twin(x, cc.LAYERNORM, 1e-5, gamma, beta)
    U = A | B
    assert cc.same_bits(got[:, U], want[:, U]) and not cc.bits_of(got)[:, ~U].any()
    assert int(bits.ne(0).sum()) == 0 and np.array_equal(host_words(mcopy), cc.pack(U))
    assert np.array_equal(host_words(mask), cc.pack(B))      # (the operand's mask is read only)


def module_twin(m, x):
    """The twin of the module `m` on the numpy map x [C, ...]."""
    np_ = (lambda t: None if t is None else t.detach().cpu().numpy())
    return cc.twin(x, m.kind, m.eps, np_(m.gamma), np_(m.beta))


def module_agrees(m, x, got, sel=None):
    """The state `got` of module m on operand x at the pixels `sel`: the twin's bits -- for the softmax kinds within the
    bound of the float64 formula."""
    sel = np.ones(x.shape[1:], dtype=bool) if sel is None else sel
    if m.kind in (cc.SOFTMAX, cc.LOGSOFTMAX):
        check_float64(m.kind)(x, got, sel, (repr(m),), None, None)
        return True
    return cc.same_bits(got[:, sel], module_twin(m, x[:, sel]))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
def test_module_forms_flags_and_errors(pkg, lib, dtype):
    """CBChannelReduce2d: a new state is written completely whatever the list says; a MaskChangeIndexes is taken as its
    mask and its list never made; ChangeIndexes and exact tensors as lists; the flags of CBAdd2d; reallocation on a new
    resolution; clearMemory; the refusals."""
    from cbinfer_amd.conv2d_cg import ChangeIndexes, MaskChangeIndexes
    Cn, H, W = 5, 7, 70
    rng = np.random.default_rng(3)
    for op, kw in ((LayerNorm2d(Cn), dict(layerNormTypes=(LayerNorm2d,))), (nn.LayerNorm(Cn, elementwise_affine=False), {}),
                   ('l2norm', {}), (nn.Softmax2d(), {}), (nn.LogSoftmax(dim=1), {})):
        m = pkg.CBChannelReduce2d(op, **kw).cuda()
        m.propChangeIndexes = True
        x = cc.values(rng, (Cn, H, W), dtype)
        empty = torch.zeros(0, dtype=torch.int32, device="cuda")
        tag, y, ix = m(('changeIndexes', dev(x)[None], empty))      # first frame
        assert tag == 'changeIndexes' and module_agrees(m, x, m.outputState[0].cpu().numpy())
        assert y is not m.outputState and torch.equal(raw(y), raw(m.outputState))
        assert isinstance(ix, MaskChangeIndexes) and ix.size == (H, W) and not ix._made
        assert ix.tensor().numel() == H * W
        for t in range(4):
            prev = m.outputState[0].cpu().numpy()
            S = rng.random((H, W)) < 0.1
            if t == 3:
                S[:] = False
            fresh = cc.values(rng, (Cn, H, W), dtype)
            x[:, S] = fresh[:, S]
            if not S[6, 69]:
                x[:, 6, 69] = fresh[:, 6, 69]      # (not listed)
            if t % 2 == 0:
                ind = MaskChangeIndexes(dev_words(cc.pack(S)), (H, W), torch.empty(H * W, dtype=torch.int32, device="cuda"),
                                        torch.zeros(1, dtype=torch.int32, device="cuda"))
            else:
                lb = dev(np.flatnonzero(S.reshape(-1)).astype(np.int32))
                ind = lb if t == 3 else ChangeIndexes(torch.cat([lb, lb.new_full((3,), 6 * W + 69)]),
                                                      torch.tensor([lb.numel()], dtype=torch.int32, device="cuda"), (H, W))
            tag, y, ix = m(('changeIndexes', dev(x)[None], ind))
            if t % 2 == 0:
                assert not ind._made      # the producer's list was never materialised
            got = m.outputState[0].cpu().numpy()
            assert module_agrees(m, x, got, S), (op, t)
            assert np.array_equal(cc.bits_of(got)[:, ~S], cc.bits_of(prev)[:, ~S]), (op, t)
            assert np.array_equal(host_words(ix._mask), cc.pack(S))
            assert np.array_equal(ix.tensor().cpu().numpy(), np.flatnonzero(S.reshape(-1))), (op, t)
            assert int(m._chWork['bits'].ne(0).sum()) == 0
        # a bare tensor carries no change information: the dense result; the state itself is handed out, tagged
        m.propChangeIndexes, m.cloneOutput = False, False
        out = m(dev(x)[None])
        assert out is m.outputState and out._cbinfer_inplace_state
        assert module_agrees(m, x, out[0].cpu().numpy())
        # a new resolution: the state and the work buffers are made again, the frame is dense whatever the list says
        x2 = cc.values(rng, (Cn, 3, 9), dtype)
        out = m(('changeIndexes', dev(x2)[None], empty))
        assert tuple(out.shape) == (1, Cn, 3, 9) and m._chWork['key'][:3] == (Cn, 3, 9)
        assert module_agrees(m, x2, out[0].cpu().numpy())
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
        if m.gamma is not None:
            with pytest.raises(Err, match="the input has 4 channels"):
                m(dx[:, :4].contiguous())
            with pytest.raises(Err, match=r"move the module with \.to\(\)"):
                copy.deepcopy(m).cpu()(dx)
        with pytest.raises(Err, match=r"\[1, C, H, W\]"):
            m(torch.cat([dx, dx]))
        with pytest.raises(Err, match="HIP devices only"):
            m(dx.cpu())
        before = m.outputState.clone()
        torch.cuda.synchronize()
        assert torch.equal(raw(m.outputState), raw(before))
        m.clearMemory()
        assert m.outputState.numel() == 0 and m._chWork is None
        out = m(dx)
        assert module_agrees(m, x2, out[0].cpu().numpy())


# ------------------------------------------------------------------------------------------------ chains
class DenseTwin(nn.Module):
    """The twin applied densely on the CPU in the place of a CBChannelReduce2d, the producer's changes handed through
    untouched."""

    def __init__(self, m):
        super(DenseTwin, self).__init__()
        self.m, self.propChangeIndexes = [m], m.propChangeIndexes

    def forward(self, inp):
        x, ix = (inp[1], inp[2]) if type(inp) == tuple else (inp, None)
        y = dev(module_twin(self.m[0], x.detach()[0].cpu().numpy()))[None]
        return ('changeIndexes', y, ix) if self.propChangeIndexes else y


def convnext_chain(pkg, tdt, link=True):
    """1x1 CBConv2d 8 -> 16, 7x7 depthwise, channels-first LayerNorm, 1x1 CBConv2d 16 -> 8, every threshold 0."""
    torch.manual_seed(91)
    src = nn.Sequential()
    for name, mod in (('expand', nn.Conv2d(8, 16, 1)), ('dw', nn.Conv2d(16, 16, 7, 1, 3, groups=16)),
                      ('norm', LayerNorm2d(16)), ('project', nn.Conv2d(16, 8, 1))):
        src.add_module(name, mod)
    net = pkg.convert(src.eval().cuda().to(tdt), threshold=0.0, depthwise=True)
    assert [type(m).__name__ for m in net] == ['CBConv2d', 'CBDepthwiseConv2d', 'LayerNorm2d', 'CBConv2d']
    if link:
        pkg.insertCBChannelOps(pkg.linkDepthwise(net), layerNormTypes=(LayerNorm2d,))
        assert [(n, type(m).__name__) for n, m in net.named_children()] == [
            ('expand', 'CBConv2d'), ('dw', 'CBDepthwiseConv2d'), ('norm', 'CBChannelReduce2d'), ('project', 'CBConv2d')]
        assert net.expand.propChangeIndexes and net.dw.propChangeIndexes and net.dw.propagatedChanges
        assert net.norm.propChangeIndexes and not net.project.propChangeIndexes
        assert net.norm.kind == cc.LAYERNORM and net.norm.gamma.dtype == torch.float32
    if tdt == torch.float32:
        net.expand.exactF32 = net.project.exactF32 = True
    return net


def segmentation_chain(pkg, tdt):
    """3x3 CBConv2d 8 -> 5, nn.Softmax2d."""
    torch.manual_seed(93)
    src = nn.Sequential()
    for name, mod in (('head', nn.Conv2d(8, 5, 3, padding=1)), ('prob', nn.Softmax2d())):
        src.add_module(name, mod)
    src = src.eval().cuda().to(tdt)
    with torch.no_grad():
        src.head.weight.mul_(6.0)      # (logits a few units apart)
    net = pkg.insertCBChannelOps(pkg.convert(src, threshold=0.0))
    assert [type(m).__name__ for m in net] == ['CBConv2d', 'CBChannelReduce2d']
    assert net.head.propChangeIndexes and net.prob.kind == cc.SOFTMAX
    if tdt == torch.float32:
        net.head.exactF32 = True
    return net


def set_clone(net, cloneOutput):
    for m in net:
        if hasattr(m, 'cloneOutput'):
            m.cloneOutput = cloneOutput
    return net


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
def test_convnext_chain_equals_the_chain_with_the_dense_twin(pkg, lib, dtype, monkeypatch):
    """Six frames of moving blocks: the chain with a CBChannelReduce2d against a deep copy -- made before the first frame
    -- whose LayerNorm is the twin applied densely on the CPU: bit for bit in the output and in every state.  Each frame
    makes exactly one cbinfer_cbchanreduce_forward call, the depthwise layer one propagated call, and no call behind the
    first layer carries `detect` in its name; after the first frame less than half of the pixels are listed."""
    import cbinfer_amd.chanreduce as chmod
    import cbinfer_amd.conv2d as convmod
    import cbinfer_amd.conv2d_cg as cgmod
    import cbinfer_amd.dwconv as dwmod
    tdt = torch.float32 if dtype == np.float32 else torch.float16
    net = convnext_chain(pkg, tdt)
    dense = copy.deepcopy(net)
    dense.norm = DenseTwin(net.norm)
    spy = LayerSpy(lib.C)
    for mod in (convmod, cgmod, dwmod, chmod):
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
            ref = module_twin(net.norm, net.dw.prevOutput[0].cpu().numpy())
            assert cc.same_bits(net.norm.outputState[0].cpu().numpy(), ref), t
            for name in ('expand', 'dw', 'project'):
                assert torch.equal(raw(getattr(net, name).prevOutput), raw(getattr(dense, name).prevOutput)), (name, t)
            share.append(share_of(net.norm._chWork['copy'], 20, 70))
    for h in hooks:
        h.remove()
    print("listed share per frame:", ["%.2f" % s for s in share], {k: v for k, v in spy.calls.items() if k != 'dense'})
    assert share[0] == 1.0 and 0 < min(share[1:]) and max(share[1:]) < 0.5, share
    assert spy.calls['norm'] == {'cbinfer_cbchanreduce_forward': 6}
    assert spy.calls['dw'] == {'cbinfer_cbdwconv2d_forward_propagated': 6}
    for name in ('dw', 'norm', 'project'):
        assert spy.calls[name] and not any('detect' in n for n in spy.calls[name]), name
    assert net.dw.prevInput.numel() == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
def test_segmentation_head_state_is_the_softmax_of_the_producers_state(pkg, lib, dtype):
    """3x3 CBConv2d -> nn.Softmax2d, six frames: the module's state is within the bound of the float64 softmax of the
    producer's state on every frame, at every pixel."""
    tdt = torch.float32 if dtype == np.float32 else torch.float16
    net = segmentation_chain(pkg, tdt)
    frames = chain_frames(np.random.default_rng(31), 6, dtype)
    share = []
    with torch.no_grad():
        for t, f in enumerate(frames):
            y = net(f)
            assert torch.equal(raw(y), raw(net.prob.outputState))
            logits = net.head.prevOutput[0].cpu().numpy()
            assert module_agrees(net.prob, logits, net.prob.outputState[0].cpu().numpy()), t
            share.append(share_of(net.prob._chWork['copy'], 20, 70))
    assert share[0] == 1.0 and 0 < min(share[1:]) and max(share[1:]) < 0.5, share


@pytest.mark.parametrize("chain", ["convnext", "segmentation"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
def test_chains_record_as_a_launch_program(pkg, lib, dtype, chain):
    """With cloneOutput=False both chains are library calls only: FrameProgram records them, the CBChannelReduce2d is ONE
    call of the recorded frame, three replayed frames equal the eager network in outputs and states bit for bit."""
    tdt = torch.float32 if dtype == np.float32 else torch.float16
    net = set_clone(convnext_chain(pkg, tdt) if chain == "convnext" else segmentation_chain(pkg, tdt), False)
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
        assert raws.count(lib.C.cbinfer_cbchanreduce_forward.raw) == 1
        assert any(t is getattr(net, 'norm' if chain == "convnext" else 'prob').outputState
                   for t in pkg.getStateTensors(net))


def test_chain_with_torchs_layer_norm_is_refused_by_frame_program(pkg, lib):
    """What the LayerNorm costs without CBChannelReduce2d: the same converted layers with the dense channels-first layer
    norm between them cannot be recorded."""
    net = set_clone(convnext_chain(pkg, torch.float32, link=False), False)
    frames = chain_frames(np.random.default_rng(29), 4, np.float32)
    with torch.no_grad():
        for f in frames[:3]:
            net(f)
        with pytest.raises(lib.CBinferError, match="torch operators.*CBChannelReduce2d"):
            pkg.FrameProgram(net).record(frames[3])


def test_worst_figures_are_reported():
    """The worst err / bound of SOFTMAX / LOGSOFTMAX over the tests above: measurements, not bars (the bar is 1)."""
    for (name, dt), w in sorted(WORST.items()):
        print("%-10s %-8s worst err / bound = %.3f" % (name, dt, w))
    assert WORST
