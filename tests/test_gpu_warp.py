"""-m gpu tests of the change-based grid sampling (CBResize2d with a coordinate field; cb_warp.hip)
against F.grid_sample in float64 on the CPU, fed the operand values converted exactly; the bar is DESIGN 5.32's bound."""
import copy
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from optest import gpu_lib as lib, gpu_pkg as pkg, host_words, operand_args, pack, raw, stream  # noqa: F401

pytestmark = pytest.mark.gpu

MODES, PADS = ('nearest', 'bilinear', 'bicubic'), ('zeros', 'border', 'reflection')
DTYPES = [torch.float32, torch.float16]
SHAPE = (5, 9, 70, 7, 130)      # taps straddle the 63 | 64 mask-word boundary, the last output word is cut


def norm(s, n, align):
    return (2 * s / (n - 1) - 1) if align else ((2 * s + 1) / n - 1)


def positions(rng, n, shape, nearest):
    """Source positions of an axis of n pixels: interior points, integer positions (a zero weight) and points up to 2.5
    map sizes outside; for nearest an integer plus at most 0.4."""
    s = rng.uniform(-0.5, n - 0.5, shape)
    far = rng.random(shape) < 0.3
    s[far] = rng.uniform(-2.5 * n, 3.5 * n, shape)[far]
    whole = rng.random(shape) < 0.2
    s[whole] = np.rint(s[whole])
    return np.rint(s) + rng.uniform(-0.4, 0.4, shape) if nearest else s


def field(rng, kind, Hi, Wi, Ho, Wo, align, nearest, cdt):
    """A [1, Ho, Wo, 2] grid (with exact +-1 where that is no rounding tie) or a [1, 2, Ho, Wo] flow."""
    sx, sy = positions(rng, Wi, (Ho, Wo), nearest), positions(rng, Hi, (Ho, Wo), nearest)
    if kind == 'flow':
        d = np.stack([sx - np.arange(Wo)[None, :], sy - np.arange(Ho)[:, None]])
        return torch.from_numpy(d[None]).to(cdt)
    g = np.stack([norm(sx, Wi, align), norm(sy, Hi, align)], axis=-1)
    if align or not nearest:
        g[0, :3] = [[-1, -1], [1, 1], [1, -1]]
    return torch.from_numpy(g[None]).to(cdt)


def reference(x, co, kind, mode, pad, align):
    """(F.grid_sample in float64, the bound of DESIGN 5.32 per output pixel; None for nearest, which is exact)."""
    (Hi, Wi), g = x.shape[2:], co.double().cpu()
    if kind == 'flow':      # source = own pixel + displacement, as a float64 grid
        sx, sy = g[0, 0] + torch.arange(g.size(3))[None, :], g[0, 1] + torch.arange(g.size(2))[:, None]
        g = torch.stack([norm(sx, Wi, align), norm(sy, Hi, align)], dim=-1)[None]
    else:
        sx, sy = (((g[0, ..., k] + 1) / 2 * (n - 1)) if align else (((g[0, ..., k] + 1) * n - 1) / 2)
                  for k, n in ((0, Wi), (1, Hi)))
    want = F.grid_sample(x.double().cpu(), g, mode=mode, padding_mode=pad, align_corners=align)
    if mode == 'nearest':
        for s in (sx, sy):      # no coordinate within 1e-3 px of a rounding tie
            assert float(((s - 0.5) - torch.round(s - 0.5)).abs().min()) >= 1e-3
        return want, None
    u = 2.0 ** -24 * float(x.abs().max())
    reach = torch.clamp(sx.abs(), min=Wi) + torch.clamp(sy.abs(), min=Hi) + 2
    bound = u * (9 + 12 * reach) if mode == 'bilinear' else u * (480 + 16.5 * reach)
    if x.dtype == torch.float16:
        bound = bound + 2.0 ** -11 * want.abs() + 2.0 ** -25
    return want, bound


class Frame(object):
    """One state of cbinfer_cbwarp_forward with its masks."""

    def __init__(self, lib, x, co, kind, mode, pad, align):
        C, self.lib = lib.C, lib
        self.Cn, self.Hi, self.Wi = x.shape[1:]
        self.Ho, self.Wo = co.shape[1:3] if kind == 'grid' else co.shape[2:]
        self.wp = ctypes.pointer(lib.Warp(self.Ho, self.Wo, MODES.index(mode), PADS.index(pad), int(align),
                                          lib.WARP_GRID if kind == 'grid' else lib.WARP_FLOW, lib.dtype_code(co)))
        assert C.cbinfer_warp_supported(self.wp, self.Hi, self.Wi) == 1
        self.out = torch.full((1, self.Cn, self.Ho, self.Wo), 77.0, dtype=x.dtype, device="cuda")
        words = C.cbinfer_mask_words(self.Ho, self.Wo)
        self.inBits = torch.zeros(C.cbinfer_mask_words(self.Hi, self.Wi), dtype=torch.int64, device="cuda")
        self.bits = torch.zeros(words, dtype=torch.int64, device="cuda")
        self.mcopy = torch.full((words,), -1, dtype=torch.int64, device="cuda")

    def run(self, x, co, fx=(None, None, 0, None), fc=(None, None, 0, None)):
        ptr, self.keep = self.lib.ptr, (x, co, fx, fc)
        st = self.lib.C.cbinfer_cbwarp_forward(
            ptr(x), ptr(co), ptr(self.out), ptr(fx[0]), ptr(fx[1]), fx[2], ptr(fx[3]), ptr(fc[0]), ptr(fc[1]), fc[2],
            ptr(fc[3]), ptr(self.inBits), ptr(self.bits), ptr(self.mcopy), self.Cn, self.Hi, self.Wi, self.wp,
            self.lib.dtype_code(x), stream())
        assert st == 0
        return self

    def listed(self):
        bits = np.unpackbits(host_words(self.mcopy).view(np.uint8), bitorder='little')
        return bits.reshape(self.Ho, -1)[:, :self.Wo].astype(bool)

    def clean(self):
        return int(self.bits.ne(0).sum()) == 0 and int(self.inBits.ne(0).sum()) == 0


@pytest.mark.parametrize("kind", ['grid', 'flow'])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
@pytest.mark.parametrize("align", [False, True], ids=["", "aligned"])
@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("mode", MODES)
def test_values_against_float64(lib, mode, pad, align, dtype, kind):
    """Every-pixel form: within the derived bound of float64 (nearest: equal); -s prints the share of the bound, DESIGN
    5.32 has the worst one.  A flow is float16 under a float32 x and the other way round."""
    Cn, Hi, Wi, Ho, Wo = SHAPE
    rng = np.random.default_rng(11)
    x = torch.from_numpy(rng.standard_normal((1, Cn, Hi, Wi)) * 10).to(dtype).cuda()
    cdt = torch.float32 if kind == 'grid' else (torch.float16 if dtype == torch.float32 else torch.float32)
    co = field(rng, kind, Hi, Wi, Ho, Wo, align, mode == 'nearest', cdt).cuda()
    f = Frame(lib, x, co, kind, mode, pad, align).run(x, co)
    assert f.listed().all() and f.clean()
    want, bound = reference(x, co, kind, mode, pad, align)
    got = f.out.double().cpu()
    if bound is None:
        assert torch.equal(got, want)
        return
    share = float(((got - want).abs() / bound).max())
    print("share of the bound %s %s %s %s %s: %.4f" % (mode, pad, align, dtype, kind, share))
    assert share <= 1.0


FRAME_CASES = [(SHAPE, 'grid'), ((1, 9, 70, 1100, 130), 'flow'), ((67, 9, 70, 7, 130), 'flow')]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", FRAME_CASES, ids=["base", "strided", "c67"])
def test_change_based_frames_are_the_dense_result(lib, case, mode):
    """Seven frames behind a first one, the operands in mask form, list form and list form with a device count (unsorted,
    a duplicate, out-of-map entries): the three states are identical bit for bit, equal a fresh every-pixel evaluation,
    keep last frame's bits outside maskCopy, and both working masks are zero."""
    (Cn, Hi, Wi, Ho, Wo), kind = case
    rng = np.random.default_rng(23)
    x = torch.from_numpy(rng.standard_normal((1, Cn, Hi, Wi)) * 10).float().cuda()
    co = field(rng, kind, Hi, Wi, Ho, Wo, False, mode == 'nearest', torch.float32).cuda()
    states = [Frame(lib, x, co, kind, mode, 'border', False).run(x, co) for _ in range(3)]
    if Cn == 1:
        assert states[0].mcopy.numel() > 8 * torch.cuda.get_device_properties(0).multi_processor_count
    none_i, none_o, yy, xx = np.zeros((Hi, Wi), dtype=bool), np.zeros((Ho, Wo), dtype=bool), *np.mgrid[:Hi, :Wi]
    frames = [("single", (yy == 4) & (xx == 63), none_o), ("corner", (yy == 0) & (xx == 0), none_o),
              ("last column", xx == Wi - 1, none_o), ("nothing", none_i, none_o), ("half", xx < Wi // 2, none_o),
              ("coordinates", none_i, rng.random((Ho, Wo)) < 0.05),
              ("both", rng.random((Hi, Wi)) < 0.1, rng.random((Ho, Wo)) < 0.05)]
    for label, SI, SC in frames:
        x, co = x.clone(), co.clone()
        x[0][:, torch.from_numpy(SI).cuda()] += 1.0
        new = field(rng, kind, Hi, Wi, Ho, Wo, False, mode == 'nearest', torch.float32).cuda()
        sel = torch.from_numpy(SC).cuda()
        if kind == 'grid':
            co[0][sel] = new[0][sel]
        else:
            co[0][:, sel] = new[0][:, sel]
        prev = raw(states[0].out).clone()
        for s, (form, count) in zip(states, (("mask", False), ("list", False), ("list", True))):
            s.run(x, co, operand_args(form, SI, 0, count), operand_args(form, SC, 0, count))
            assert s.clean(), (label, form, count)
        full = Frame(lib, x, co, kind, mode, 'border', False).run(x, co)
        listed = torch.from_numpy(states[0].listed()).cuda()
        # (under 'border' the points left of and above the map are clamped onto the corner pixel)
        assert not (label == "nothing" and listed.any()) and not (label == "corner" and int(listed.sum()) <= 4)
        for s in states:
            assert torch.equal(s.mcopy, states[0].mcopy), label
            assert torch.equal(raw(s.out), raw(full.out)), label
            assert torch.equal(raw(s.out)[0][:, ~listed], prev[0][:, ~listed]), label


@pytest.mark.parametrize("form", ["mask", "list"])
@pytest.mark.parametrize("mode,reach", [('nearest', (0, 0)), ('bilinear', (-1, 0)), ('bicubic', (-2, 1))])
def test_the_mask_is_the_footprint_and_no_more(lib, mode, reach, form):
    """Zero flow, where taps are exact: a changed input pixel lists the output pixels reach[0] .. reach[1] from it on
    either axis (bilinear: a zero weight counts; bicubic: the 4x4 block), nothing else, padding bits clear."""
    H, W = 9, 130
    x, flow = torch.randn(1, 3, H, W, device="cuda"), torch.zeros(1, 2, H, W, device="cuda")
    f = Frame(lib, x, flow, 'flow', mode, 'zeros', False).run(x, flow)
    SI = np.zeros((H, W), dtype=bool)
    for p in ((0, 0), (8, 129), (4, 63), (4, 64), (2, 100)):
        SI[p] = True
    want = np.zeros((H, W), dtype=bool)
    for y, xx in zip(*np.nonzero(SI)):
        want[max(y + reach[0], 0):y + reach[1] + 1, max(xx + reach[0], 0):xx + reach[1] + 1] = True
    f.run(x, flow, operand_args(form, SI), (None, f.bits.new_zeros(1, dtype=torch.int32), 0, None))
    assert np.array_equal(host_words(f.mcopy), pack(want)) and f.clean()


# ------------------------------------------------------------------------------------------------ through the modules
class Sampler(nn.Module):
    """A user's module around F.grid_sample with a constant grid; wrong=True: one that computes something else."""

    def __init__(self, grid, wrong=False):
        super(Sampler, self).__init__()
        self.register_buffer('field', grid)
        self.mode, self.padding_mode, self.align_corners, self.wrong = 'bilinear', 'border', False, wrong

    def forward(self, x):
        y = F.grid_sample(x, self.field, mode=self.mode, padding_mode=self.padding_mode, align_corners=self.align_corners)
        return y * 2 if self.wrong else y


def homography(Ho, Wo):
    ys, xs = torch.meshgrid(torch.linspace(-1, 1, Ho), torch.linspace(-1, 1, Wo), indexing='ij')
    w = 1 + 0.2 * xs + 0.1 * ys
    return torch.stack([(0.9 * xs + 0.1 * ys) / w, (0.05 * xs + 1.1 * ys - 0.1) / w], dim=-1)[None]


class Wired(nn.Module):
    """conv (3x3, 3 -> 6) -> CBResize2d -> 1x1 conv; 'flow': a 2-channel flow head's changes are the second operand."""

    def __init__(self, pkg, wiring, tdt):
        super(Wired, self).__init__()
        torch.manual_seed(5)
        self.wiring, Ho, Wo = wiring, 10, 70
        convs = nn.Sequential(nn.Conv2d(3, 6, 3, padding=1), nn.Conv2d(3, 2, 3, padding=1), nn.Conv2d(6, 4, 1))
        kw = dict(mode='bilinear', padding_mode='border', align_corners=False)
        if wiring == 'pass':
            src = nn.Sequential(convs[0], Sampler(homography(Ho, Wo)), convs[2]).eval().cuda().to(tdt)
            net = pkg.insertCBResize(pkg.convert(src, threshold=0.0), cloneOutput=False, gridTypes={Sampler: 'field'})
            self.conv, self.warp, self.tail = net[0], net[1], net[2]
        else:
            cb = pkg.convert(convs.eval().cuda().to(tdt), threshold=0.0)
            self.conv, self.head, self.tail = cb[0], cb[1], cb[2]
            self.warp = (pkg.CBResize2d(grid=homography(Ho, Wo), **kw) if wiring == 'grid' else
                         pkg.CBResize2d(theta=torch.tensor([[0.9, 0.2, 0.1], [-0.1, 1.1, 0.0]]), size=(Ho, Wo), **kw)
                         if wiring == 'theta' else pkg.CBResize2d(**kw)).cuda()
            self.warp.cloneOutput = False
            self.conv.propChangeIndexes = self.head.propChangeIndexes = self.warp.propChangeIndexes = True
        for m in (self.conv, self.tail) + ((self.head,) if wiring == 'flow' else ()):
            m.exactF32 = tdt == torch.float32

    def forward(self, x):
        mid = self.conv(x)
        out = self.warp(mid, flow=self.head(x)) if self.wiring == 'flow' else self.warp(mid)
        return self.tail(out)


@pytest.mark.parametrize("tdt", DTYPES, ids=["f32", "f16"])
@pytest.mark.parametrize("wiring", ['grid', 'theta', 'flow', 'pass'])
def test_through_the_modules_eager_and_recorded(pkg, lib, wiring, tdt):
    """Six frames of a moving-block sequence: the state is within the bar of the float64 operator fed the same layer
    outputs and lists a part of the map, the 1x1 layer behind takes its mask and equals a copy fed the bare tensor;
    frames four to six run as a FrameProgram."""
    net = Wired(pkg, wiring, tdt)
    assert type(net.warp) is pkg.CBResize2d and net.warp.propChangeIndexes
    bare, seen = copy.deepcopy(net.tail), {}
    # (a replayed frame calls no module: it writes the tensors of the recorded one in place)
    net.warp.register_forward_pre_hook(lambda m, args, kw: seen.update(x=args[0][1], flow=kw.get('flow')), with_kwargs=True)
    rng, prog = np.random.default_rng(31), None
    base = rng.random((1, 3, 12, 66)) * 2 - 1
    with torch.no_grad():
        for t in range(6):
            if t:
                y0, x0 = int(rng.integers(0, 10)), int(rng.integers(0, 60))
                base[:, :, y0:y0 + 2, x0:x0 + 3] = rng.random((1, 3, 2, 3)) * 2 - 1
            f = torch.from_numpy(base).to(tdt).cuda()
            if t == 3:
                prog = pkg.FrameProgram(net)
            y, state = (prog or net)(f), net.warp.outputState
            co, kind = (seen['flow'][1], 'flow') if wiring == 'flow' else (net.warp.grid, 'grid')
            want, bound = reference(seen['x'], co, kind, 'bilinear', 'border', False)
            assert bool(((state.double().cpu() - want).abs() <= bound).all()), (wiring, t)
            assert torch.equal(raw(y), raw(bare(state.clone()))), (wiring, t)
            share = float(np.unpackbits(host_words(net.warp._work['copy']).view(np.uint8)).sum()) / state[0, 0].numel()
            assert share == 1.0 if t == 0 else 0.0 < share < 1.0, (wiring, t, share)
    assert [fn for fn, _ in prog.calls].count(lib.C.cbinfer_cbwarp_forward.raw) == 1


def test_a_class_that_does_not_sample_its_grid_is_refused_by_name(pkg, lib):
    src = nn.Sequential(nn.Conv2d(3, 6, 3, padding=1), Sampler(homography(5, 7), wrong=True)).eval().cuda()
    with pytest.raises(lib.CBinferError, match="Sampler does not compute F.grid_sample"):
        pkg.insertCBResize(pkg.convert(src, threshold=0.0), gridTypes={Sampler: 'field'})
