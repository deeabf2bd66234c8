"""-m gpu tests of the six element-wise kinds of CBPointwise2d(transcendental=True) (GELU, GELU_TANH, ELU / CELU, SELU,
SOFTPLUS, MISH; cb_pointwise.hip).  There is no bit-for-bit twin for these kinds: each is held against
the same formula in float64 under the bound DERIVED in tests/activation_cases.py (its docstring has the derivation per
kind); everything else -- unlisted pixels, the masks, the forms, the module, the chain -- is exact."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn

import activation_cases as ac
from optest import (chain_frames, dev, dev_words, host_words, LayerSpy, lib,      # noqa: F401  (fixtures)
                    operand_args, gpu_pkg as pkg, raw, share_of, stream, walk_frames)
from test_gpu_chanreduce import LayerNorm2d, set_clone
from test_gpu_pointwise import FILL

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float16]
WORST = {}      # (case name, dtype name) -> [worst err / bound, worst err / |ref|] seen against float64


def code_of(lib, dtype):
    return lib.CB_F32 if dtype == np.float32 else lib.CB_F16


def note(x, got, kind, p0, p1, where):
    """ac.judge on the listed values, its figures kept for the report."""
    ok, ratio, rel, text = ac.judge(x, got, kind, p0, p1)
    w = WORST.setdefault((ac.case_name(kind, p0, p1), np.dtype(x.dtype).name), [0.0, 0.0])
    w[0], w[1] = max(w[0], ratio), max(w[1], rel if np.isfinite(rel) else 0.0)
    assert ok, (where, text)


def run_frames(lib, shape, dtype, form, kind, p0, p1, rng):
    """The six mask patterns as consecutive frames through cbinfer_cbpointwise_forward, as run_frames of
    tests/test_gpu_pointwise.py: before every frame x gets new values at the frame's pixels AND at one pixel outside
    them; the listed values are judged against the float64 formula, unlisted pixels must keep their bits, maskCopy be
    the frame's mask, the working mask zero (optest.walk_frames)."""
    C, ptr = lib.C, lib.ptr
    Cn, H, W = shape
    special = np.array(ac.SPECIAL, dtype=dtype)
    out = np.empty(shape, dtype=dtype)
    ac.bits_of(out)[...] = FILL[dtype] & (0xFFFFFFFF if dtype == np.float32 else 0xFFFF)

    def call(dx, dout, mask, lst, cap, cnt, bits, mcopy):
        return C.cbinfer_cbpointwise_forward(ptr(dx), ptr(dout), ptr(mask), ptr(lst), cap, ptr(cnt), ptr(bits), ptr(mcopy),
                                             Cn, H, W, kind, p0, p1, None, None, None, code_of(lib, dtype), stream())

    def check(x, got, listed, where):
        note(x[:, listed], got[:, listed], kind, p0, p1, where)
    return walk_frames(lib, shape, dtype, form, lambda: ac.patterns(rng, H, W), call, check, out,
                       lambda: ac.values(rng, shape, dtype, 20.0, special), what=(ac.case_name(kind, p0, p1),))


@pytest.mark.parametrize("form", ac.FORMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
def test_new_kinds_against_float64_under_the_derived_bounds(lib, dtype, form):
    """Every shape of pointwise_cases.SHAPES, the nine kind / parameter sets of activation_cases.CASES, the six mask
    patterns: at the listed pixels the state is within the derived bound of the same formula in float64, in units of
    2^-24 (derivation: the docstring of tests/activation_cases.py and DESIGN 5.30):
        GELU       (33 |v| + 3 |ref|) units      -- erff's 64 units enter as 0.5 |v| 64: 1 + erf(u) cancels for v < 0
        GELU_TANH  (12 |v| + 3 |ref|) units      -- tanhf's 20 units and the argument's 5 enter as 0.5 |v| 22.24
        ELU        14 |ref|   (v > 0: exact)       SELU  13 |ref|   (v > 0: 1)
        SOFTPLUS   21 |ref|, for p0 != 1 plus max(1, |t|) |ref|, t = v p0   (t > p1: exact)
        MISH       41 |ref|
    plus 2^-126; for fp16 plus 2^-11 |ref| + 2^-24.  Inputs in [-20, 20] plus +-inf, NaN and +-0; where the float64
    reference is not finite the result must be the same infinity or a NaN (GELU(-inf) and MISH(-inf) are NaNs,
    ELU(-inf) = -p0 is finite and bound).  The constants are not tuned: a failure is a finding.  Measured on the MI355X
    over all shapes and forms (worst err / bound; worst err / |ref| in units of 2^-24): DESIGN 5.30 has the table."""
    rng = np.random.default_rng(31)
    saw = 0
    for shape in ac.SHAPES:
        for kind, p0, p1 in ac.CASES:
            saw += run_frames(lib, shape, dtype, form, kind, p0, p1, rng)
    assert form == "all" or saw >= 4 * len(ac.SHAPES) * len(ac.CASES)
    for (name, dt), (ratio, rel) in sorted(WORST.items()):
        if dt == np.dtype(dtype).name:
            print("%-16s %s %s: worst err / bound %.3f, worst err / |ref| %.2f x 2^-24" % (name, dt, form, ratio, rel * 2.0 ** 24))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
def test_a_pixel_does_not_depend_on_the_list_the_form_or_the_run(lib, dtype):
    """One pixel's bits -- the six kinds, with the affine -- listed alone in a mask, in a list among others, in another
    list, with every pixel listed, and all of that a second time: always the same bits."""
    C, ptr = lib.C, lib.ptr
    Cn, H, W = 300, 5, 130
    rng = np.random.default_rng(17)
    x = ac.values(rng, (Cn, H, W), dtype, 8.0, np.array([0.0, -0.0, 3.0, -3.0, 6.0], dtype=dtype))
    scale = (rng.uniform(0.5, 2.0, Cn) * rng.choice([-1.0, 1.0], Cn)).astype(np.float32)
    shift = rng.uniform(-3.0, 3.0, Cn).astype(np.float32)
    dx, dscale, dshift = dev(x), dev(scale), dev(shift)
    py, px = 3, 64
    alone = np.zeros((H, W), dtype=bool)
    alone[py, px] = True
    crowd = rng.random((H, W)) < 0.5
    crowd[py, px] = True
    row = np.zeros((H, W), dtype=bool)
    row[py, :] = True
    words = C.cbinfer_mask_words(H, W)
    for kind, p0, p1 in ((ac.GELU, 0.0, 0.0), (ac.GELU_TANH, 0.0, 0.0), (ac.ELU, 0.5, 2.0), (ac.SELU, 0.0, 0.0),
                         (ac.SOFTPLUS, 2.0, 5.0), (ac.MISH, 0.0, 0.0)):
        seen = []
        for rep in range(2):
            for form, S in (("mask", alone), ("list", crowd), ("list", row), ("mask", row), ("all", alone)):
                dout = torch.zeros((Cn, H, W), dtype=dx.dtype, device="cuda")
                bits = torch.zeros(words, dtype=torch.int64, device="cuda")
                mcopy = torch.zeros(words, dtype=torch.int64, device="cuda")
                mask, lst, cap, cnt = operand_args(form, S, 0, bool(rep % 2))
                st = C.cbinfer_cbpointwise_forward(ptr(dx), ptr(dout), ptr(mask), ptr(lst), cap, ptr(cnt), ptr(bits),
                                                   ptr(mcopy), Cn, H, W, kind, p0, p1, ptr(dscale), ptr(dshift), None,
                                                   code_of(lib, dtype), stream())
                assert st == 0
                seen.append(ac.bits_of(dout[:, py, px].cpu().numpy()).copy())
        assert all(np.array_equal(s, seen[0]) for s in seen[1:]), ac.NAMES[kind]
        assert len(np.unique(seen[0])) > 1, ac.NAMES[kind]
        if dtype == np.float32:
            # the affine in front is the two-rounding one of the other kinds: the formula's bound holds on its result
            v = x[:, py, px] * scale + shift
            assert v.dtype == np.float32
            ok, _, _, text = ac.judge(v, seen[0].view(np.float32), kind, p0, p1)
            assert ok, (ac.NAMES[kind], text)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
def test_module_forms_flags_and_reallocation(pkg, lib, dtype):
    """CBPointwise2d(nn.CELU(0.5), transcendental=True): a new state is written completely whatever the list says; a
    MaskChangeIndexes is taken as its mask and its list never made; ChangeIndexes and exact tensors as lists; the flags
    of CBAdd2d; reallocation on a new resolution; clearMemory."""
    from cbinfer_amd.conv2d_cg import ChangeIndexes, MaskChangeIndexes
    Cn, H, W = 5, 7, 70
    rng = np.random.default_rng(3)
    special = np.array(ac.SPECIAL, dtype=dtype)
    m = pkg.CBPointwise2d(nn.CELU(0.5), transcendental=True).cuda()
    assert (m.kind, m.p0, m.p1) == (ac.ELU, 0.5, 2.0)
    m.propChangeIndexes = True
    x = ac.values(rng, (Cn, H, W), dtype, 20.0, special)
    empty = torch.zeros(0, dtype=torch.int32, device="cuda")
    tag, y, ix = m(('changeIndexes', dev(x)[None], empty))      # first frame
    assert tag == 'changeIndexes' and y is not m.outputState and torch.equal(raw(y), raw(m.outputState))
    note(x, m.outputState[0].cpu().numpy(), ac.ELU, 0.5, 2.0, "first frame")
    assert isinstance(ix, MaskChangeIndexes) and ix.size == (H, W) and not ix._made and ix.tensor().numel() == H * W
    for t in range(4):
        prev = m.outputState[0].cpu().numpy()
        S = rng.random((H, W)) < 0.1
        if t == 3:
            S[:] = False
        fresh = ac.values(rng, (Cn, H, W), dtype, 20.0, special)
        x[:, S] = fresh[:, S]
        if not S[6, 69]:
            x[:, 6, 69] = fresh[:, 6, 69]      # (not listed)
        if t % 2 == 0:
            ind = MaskChangeIndexes(dev_words(ac.pack(S)), (H, W), torch.empty(H * W, dtype=torch.int32, device="cuda"),
                                    torch.zeros(1, dtype=torch.int32, device="cuda"))
        else:
            lb = dev(np.flatnonzero(S.reshape(-1)).astype(np.int32))
            ind = lb if t == 3 else ChangeIndexes(torch.cat([lb, lb.new_full((3,), 6 * W + 69)]),
                                                  torch.tensor([lb.numel()], dtype=torch.int32, device="cuda"), (H, W))
        tag, y, ix = m(('changeIndexes', dev(x)[None], ind))
        if t % 2 == 0:
            assert not ind._made      # the producer's list was never materialised
        got = m.outputState[0].cpu().numpy()
        note(x[:, S], got[:, S], ac.ELU, 0.5, 2.0, t)
        assert np.array_equal(ac.bits_of(got)[:, ~S], ac.bits_of(prev)[:, ~S]), t
        assert np.array_equal(host_words(ix._mask), ac.pack(S))
        assert np.array_equal(ix.tensor().cpu().numpy(), np.flatnonzero(S.reshape(-1))), t
        assert int(m._pwWork['bits'].ne(0).sum()) == 0
    # a bare tensor carries no change information: the dense result; the state itself is handed out, tagged
    m.propChangeIndexes, m.cloneOutput = False, False
    out = m(dev(x)[None])
    assert out is m.outputState and out._cbinfer_inplace_state
    note(x, out[0].cpu().numpy(), ac.ELU, 0.5, 2.0, "bare tensor")
    # a new resolution: the state and the work buffers are made again, the frame is dense whatever the list says
    x2 = ac.values(rng, (Cn, 3, 9), dtype, 20.0, special)
    out = m(('changeIndexes', dev(x2)[None], empty))
    assert tuple(out.shape) == (1, Cn, 3, 9) and m._pwWork['key'][:3] == (Cn, 3, 9)
    note(x2, out[0].cpu().numpy(), ac.ELU, 0.5, 2.0, "new resolution")
    m.clearMemory()
    assert m.outputState.numel() == 0 and m._pwWork is None
    out = m(dev(x2)[None])
    note(x2, out[0].cpu().numpy(), ac.ELU, 0.5, 2.0, "after clearMemory")


# ------------------------------------------------------------------------------------------------ a ConvNeXt-type chain
class EveryPixel(nn.Module):
    """In the place of a CBPointwise2d: the same kind recomputed at EVERY pixel through cbinfer_cbpointwise_forward in
    all form into a state of its own, the producer's indexes handed through untouched.  A pixel's bits do not depend on
    the form (tested above), so a chain with this module computes what the chain with the change-based one must."""

    def __init__(self, m, lib):
        super(EveryPixel, self).__init__()
        self.kind, self.p0, self.p1, self.propChangeIndexes, self.lib = m.kind, m.p0, m.p1, m.propChangeIndexes, [lib]
        self.state = None

    def forward(self, inp):
        lib = self.lib[0]
        x, ix = (inp[1], inp[2]) if type(inp) == tuple else (inp, None)
        _, Cn, H, W = x.shape
        if self.state is None:
            words = lib.C.cbinfer_mask_words(H, W)
            self.state = torch.empty_like(x)
            self.bits = torch.zeros(words, dtype=torch.int64, device=x.device)
            self.copy = torch.zeros(words, dtype=torch.int64, device=x.device)
        lib.check(lib.C.cbinfer_cbpointwise_forward(lib.ptr(x), lib.ptr(self.state), None, None, 0, None, lib.ptr(self.bits),
                                                    lib.ptr(self.copy), Cn, H, W, self.kind, self.p0, self.p1, None, None,
                                                    None, lib.dtype_code(x), stream()))
        y = self.state.clone()
        return ('changeIndexes', y, ix) if self.propChangeIndexes else y


def convnext_body(pkg, tdt, transcendental=True):
    """1x1 CBConv2d 8 -> 16, 7x7 depthwise, channels-first LayerNorm, 1x1 16 -> 32, GELU, 1x1 32 -> 8; every threshold 0."""
    torch.manual_seed(91)
    src = nn.Sequential()
    for name, mod in (('stem', nn.Conv2d(8, 16, 1)), ('dw', nn.Conv2d(16, 16, 7, 1, 3, groups=16)), ('norm', LayerNorm2d(16)),
                      ('pw1', nn.Conv2d(16, 32, 1)), ('gelu', nn.GELU()), ('pw2', nn.Conv2d(32, 8, 1))):
        src.add_module(name, mod)
    src = src.eval().cuda().to(tdt)
    with torch.no_grad():
        src.pw1.weight.mul_(4.0)      # (values on both sides of GELU's minimum)
    net = pkg.convert(src, threshold=0.0, depthwise=True)
    pkg.insertCBPointwise(net, transcendental=transcendental)
    pkg.insertCBChannelOps(pkg.linkDepthwise(net), layerNormTypes=(LayerNorm2d,))
    kinds = [type(m).__name__ for m in net]
    assert kinds == ['CBConv2d', 'CBDepthwiseConv2d', 'CBChannelReduce2d', 'CBConv2d',
                     'CBPointwise2d' if transcendental else 'GELU', 'CBConv2d']
    assert net.stem.propChangeIndexes and net.dw.propagatedChanges and net.dw.propChangeIndexes and net.norm.propChangeIndexes
    assert net.pw1.propChangeIndexes is transcendental and not net.pw2.propChangeIndexes
    if transcendental:
        assert net.gelu.kind == ac.GELU and net.gelu.propChangeIndexes
    if tdt == torch.float32:
        net.stem.exactF32 = net.pw1.exactF32 = net.pw2.exactF32 = True
    return net


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
def test_convnext_chain_equals_the_chain_that_recomputes_every_pixel(pkg, lib, dtype, monkeypatch):
    """Six frames of moving blocks: the chain with the GELU as a CBPointwise2d against a deep copy -- made before the
    first frame -- whose GELU is EveryPixel: bit for bit in the output and in every state.  The GELU makes exactly one
    cbinfer_cbpointwise_forward call per frame, the 1x1 layer behind it no call with `detect` in its name; after the
    first frame less than half of the pixels are listed."""
    import cbinfer_amd.chanreduce as chmod
    import cbinfer_amd.conv2d as convmod
    import cbinfer_amd.conv2d_cg as cgmod
    import cbinfer_amd.dwconv as dwmod
    import cbinfer_amd.pointwise as pwmod
    tdt = torch.float32 if dtype == np.float32 else torch.float16
    net = convnext_body(pkg, tdt)
    dense = copy.deepcopy(net)
    dense.gelu = EveryPixel(net.gelu, lib)
    spy = LayerSpy(lib.C)
    for mod in (convmod, cgmod, dwmod, chmod, pwmod):
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
            assert torch.equal(raw(net.gelu.outputState), raw(dense.gelu.state)), t
            note(net.pw1.prevOutput[0].cpu().numpy(), net.gelu.outputState[0].cpu().numpy(), ac.GELU, 0.0, 0.0, ("chain", t))
            for name in ('stem', 'dw', 'pw1', 'pw2'):
                assert torch.equal(raw(getattr(net, name).prevOutput), raw(getattr(dense, name).prevOutput)), (name, t)
            assert torch.equal(raw(net.norm.outputState), raw(dense.norm.outputState)), t
            share.append(share_of(net.gelu._pwWork['copy'], 20, 70))
    for h in hooks:
        h.remove()
    print("listed share per frame:", ["%.2f" % s for s in share], {k: v for k, v in spy.calls.items() if k != 'dense'})
    assert share[0] == 1.0 and 0 < min(share[1:]) and max(share[1:]) < 0.5, share
    assert spy.calls['gelu'] == {'cbinfer_cbpointwise_forward': 6}
    assert spy.calls['pw2'] and not any('detect' in n for n in spy.calls['pw2'])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
def test_convnext_chain_records_as_a_launch_program(pkg, lib, dtype):
    """With cloneOutput=False the chain is library calls only: FrameProgram records it, the GELU is ONE call of the
    recorded frame, three replayed frames equal the eager network in outputs and states bit for bit."""
    tdt = torch.float32 if dtype == np.float32 else torch.float16
    net = set_clone(convnext_body(pkg, tdt), False)
    frames = chain_frames(np.random.default_rng(23), 7, dtype)
    with torch.no_grad():
        for f in frames[:4]:
            net(f)
        eager = copy.deepcopy(net)
        prog = pkg.FrameProgram(net)
        for t, f in enumerate(frames[4:]):
            yp, ye = prog(f), eager(f)
            assert torch.equal(raw(yp), raw(ye)), t
            states = list(zip(pkg.getStateTensors(net), pkg.getStateTensors(eager)))
            assert len(states) >= 6 and all(torch.equal(ta, tb) for ta, tb in states), t
        raws = [fn for fn, _ in prog.calls]
        assert raws.count(lib.C.cbinfer_cbpointwise_forward.raw) == 1


def test_convnext_chain_with_torchs_gelu_is_refused_by_frame_program(pkg, lib):
    """What the one dense activation costs: the same converted layers with torch's nn.GELU between them cannot be
    recorded."""
    net = set_clone(convnext_body(pkg, torch.float32, transcendental=False), False)
    frames = chain_frames(np.random.default_rng(29), 4, np.float32)
    with torch.no_grad():
        for f in frames[:3]:
            net(f)
        with pytest.raises(lib.CBinferError, match="torch operators.*CBPointwise2d"):
            pkg.FrameProgram(net).record(frames[3])


def test_worst_figures_are_reported():
    """The worst err / bound and err / |ref| (in units of 2^-24, where |ref| >= 2^-14) of each kind over the tests
    above: measurements, not bars; DESIGN 5.30 has them."""
    for (name, dt), (ratio, rel) in sorted(WORST.items()):
        print("%-16s %-8s worst err / bound %.3f   worst err / |ref| = %.3g = %.2f x 2^-24" % (name, dt, ratio, rel, rel * 2.0 ** 24))
    assert WORST
