"""-m gpu tests of the change-based resize (CBResize2d; cb_resize.hip).  The reference has no such
operator; the resize section of include/cbinfer_hip.h is the specification and tests/resize_cases.py its numpy twin:
  rule 1  the listed pixels: the output pixels any of whose 1 / 2x2 / 4x4 clamped taps is listed, zero weights included;
          an input without change information lists every pixel; padding bits never set;
  rule 2  the values: listed values equal the f32 twin BIT FOR BIT (fp16: the twin rounded once), whatever the operand's
          form and the other listed pixels; every other value of the state keeps its bits;
  rule 3  the hand-on: the frame's mask in maskCopy, the working mask zero."""
import copy
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import resize_cases as rc
from test_gpu_decoder import SENTINEL, input_frames, list_args, refresh, sel_of
from optest import bits_of, dev_words, host_words, lib, pack, gpu_pkg as pkg, raw, stream      # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float16]
CASES = [s + (None,) for s in rc.SHAPES] + [rc.SCALE_SHAPE + (None, None, sf) for sf in rc.SCALES]


def case_id(c):
    return rc.shape_id(c[:5]) if c[5] is None else "%dx%dx%d-by-%s" % (c[:3] + (c[5],))


def struct_of(lib, rs):
    return ctypes.pointer(lib.Resize(*rs))


def host(t):
    return t[0].cpu().numpy()


# ------------------------------------------------------------------------------------------------ the C ABI
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
@pytest.mark.parametrize("mode", rc.MODES, ids=rc.MODE_IDS)
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_resize_every_form_through_the_c_abi(lib, case, mode, dtype):
    """cbinfer_cbresize_forward: an all-form first frame, then five frames (single, corner, last column, empty, half) each
    run in mask form, in list form and in list form with a device count (unsorted, a duplicate, out-of-map entries) on
    states whose unlisted values were overwritten with a sentinel: maskCopy is the brute-force footprint, the working
    mask is zero, unlisted values keep the sentinel, listed ones equal the f32 twin bit for bit, and the three states
    are identical."""
    C, ptr, check = lib.C, lib.ptr, lib.check
    Cn, Hi, Wi = case[:3]
    if case[5] is None:
        rs = rc.resize_of_size(Hi, Wi, case[3], case[4], *mode)
    else:
        rs = rc.resize_of_scale(Hi, Wi, case[5], *mode)
    Ho, Wo = rs.Ho, rs.Wo
    st = struct_of(lib, rs)
    assert C.cbinfer_resize_supported(st, Hi, Wi) == 1
    words = C.cbinfer_mask_words(Ho, Wo)
    if case[:5] == rc.STRIDED:
        assert words > 8 * torch.cuda.get_device_properties(0).multi_processor_count
    rng = np.random.default_rng(7)
    x = torch.from_numpy(rng.standard_normal((1, Cn, Hi, Wi)) * 10).to(dtype).cuda()
    dt = lib.dtype_code(x)

    def launch(s, mask=None, lst=None, cap=0, count=None):
        check(C.cbinfer_cbresize_forward(ptr(x), ptr(s['out']), ptr(mask), ptr(lst), cap, ptr(count), ptr(s['bits']),
                                         ptr(s['mcopy']), Cn, Hi, Wi, st, dt, stream()))

    states = {}
    want = rc.twin(host(x), rs, np.float32)
    for form in ("mask", "list", "count"):
        s = states[form] = dict(out=torch.empty((1, Cn, Ho, Wo), dtype=dtype, device="cuda"),
                                bits=torch.zeros(words, dtype=torch.int64, device="cuda"),
                                mcopy=torch.full((words,), -1, dtype=torch.int64, device="cuda"))
        raw(s['out']).fill_(SENTINEL)
        launch(s)      # the all form
        assert np.array_equal(host_words(s['mcopy']), pack(np.ones((Ho, Wo), dtype=bool)))
        assert int(s['bits'].ne(0).sum()) == 0
        assert np.array_equal(bits_of(host(s['out'])), bits_of(want)), (rs, dtype, "all")
    for label, SI in input_frames(rng, Hi, Wi):
        refresh(x, SI, rng)
        want = rc.twin(host(x), rs, np.float32)
        listed = rc.footprint(SI, rs)
        sel = sel_of(listed)
        for form, s in states.items():
            where = (rs, dtype, label, form)
            raw(s['out'])[0][:, ~sel] = SENTINEL
            if form == "mask":
                launch(s, mask=dev_words(pack(SI)))
            else:
                lst, cap, count = list_args(SI, useCount=form == "count")
                launch(s, lst=lst, cap=cap, count=count)
            assert np.array_equal(host_words(s['mcopy']), pack(listed)), where
            assert int(s['bits'].ne(0).sum()) == 0, where
            got = bits_of(host(s['out']))
            assert (got[:, ~listed] == SENTINEL).all(), where
            assert np.array_equal(got[:, listed], bits_of(want)[:, listed]), where
        assert torch.equal(raw(states['mask']['out']), raw(states['list']['out']))
        assert torch.equal(raw(states['mask']['out']), raw(states['count']['out']))
    # a list of capacity 0 (any address) is the empty frame
    s = states["list"]
    check(C.cbinfer_cbresize_forward(ptr(x), ptr(s['out']), None, ptr(s['bits']), 0, None, ptr(s['bits']), ptr(s['mcopy']),
                                     Cn, Hi, Wi, st, dt, stream()))
    assert int(s['mcopy'].ne(0).sum()) == 0 and int(s['bits'].ne(0).sum()) == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
def test_integer_scales_against_the_upsample_kernel(lib, dtype):
    """Scales 1..8: nearest equals cbinfer_cbupsample_forward bit for bit.  Bilinear derives the same t from the same
    integers, but that kernel may contract to FMAs: fp32 within the bar of DESIGN 5.13, 8 2^-24 max|tap|, of it; fp16
    compares two values rounded to f16 once each, so two roundings come on top: 2 (2^-11 max(|a|, |b|) + 2^-25) + 8 2^-24
    max|tap|."""
    C, ptr, check = lib.C, lib.ptr, lib.check
    rng = np.random.default_rng(17)
    worst = 0.0
    for Cn, Hi, Wi, sH, sW in ((5, 3, 32, 1, 2), (5, 4, 13, 2, 5), (3, 5, 23, 3, 3), (2, 3, 70, 8, 1), (5, 2, 9, 7, 8),
                               (2, 4, 11, 4, 6)):
        Ho, Wo = Hi * sH, Wi * sW
        x = torch.from_numpy(rng.standard_normal((1, Cn, Hi, Wi)) * 10).to(dtype).cuda()
        words = C.cbinfer_mask_words(Ho, Wo)
        for mode, align in ((rc.NEAREST, 0), (rc.BILINEAR, 0), (rc.BILINEAR, 1)):
            outs = []
            for which in ("resize", "upsample"):
                out = torch.empty((1, Cn, Ho, Wo), dtype=dtype, device="cuda")
                bits = torch.zeros(words, dtype=torch.int64, device="cuda")
                mcopy = torch.zeros(words, dtype=torch.int64, device="cuda")
                if which == "resize":
                    rs = rc.Resize(Ho, Wo, 1, sH, 1, sW, mode, align)
                    check(C.cbinfer_cbresize_forward(ptr(x), ptr(out), None, None, 0, None, ptr(bits), ptr(mcopy), Cn, Hi,
                                                     Wi, struct_of(lib, rs), lib.dtype_code(x), stream()))
                else:
                    up = ctypes.pointer(lib.Upsample(sH, sW, lib.UPSAMPLE_NEAREST if mode == rc.NEAREST else
                                                     lib.UPSAMPLE_BILINEAR, align))
                    check(C.cbinfer_cbupsample_forward(ptr(x), ptr(out), None, None, 0, None, ptr(bits), ptr(mcopy), Cn,
                                                       Hi, Wi, up, lib.dtype_code(x), stream()))
                outs.append(out)
            if mode == rc.NEAREST:
                assert torch.equal(raw(outs[0]), raw(outs[1])), (sH, sW)
                continue
            a, b = (host(o).astype(np.float64) for o in outs)
            mx = rc.tap_abs_max(host(x), rs)[None]
            bar = 8 * 2.0 ** -24 * mx
            if dtype == torch.float16:
                bar = bar + 2 * (2.0 ** -11 * np.maximum(np.abs(a), np.abs(b)) + 2.0 ** -25)
            share = float((np.abs(a - b) / np.where(bar > 0, bar, 1)).max())
            worst = max(worst, share)
            assert (np.abs(a - b) <= bar).all(), (sH, sW, align, share)
    print("bilinear against the integer-scale kernel, %s: worst share of the bar %.4f" % (dtype, worst))


# ------------------------------------------------------------------------------------------------ the module
def test_module_forms_flags_sizes_and_clear_memory(pkg, lib):
    from cbinfer_amd.conv2d_cg import ChangeIndexes, MaskChangeIndexes
    Cn, Hi, Wi = 3, 6, 70
    rng = np.random.default_rng(3)
    for dtype, mode, align, kw in ((torch.float32, 'bicubic', False, dict(size=(9, 100))),
                                   (torch.float16, 'nearest-exact', None, dict(scale_factor=(1.5, 0.5))),
                                   (torch.float32, 'bilinear', True, dict(size=(4, 33)))):
        rsz = pkg.CBResize2d(mode=mode, align_corners=align, **kw)
        rsz.propChangeIndexes = True
        geo = rsz.geometry(Hi, Wi)
        rs = rc.Resize(*(geo + (pkg.resize.MODES[mode], int(bool(align)))))
        Ho, Wo = geo[:2]
        x = torch.from_numpy(rng.standard_normal((1, Cn, Hi, Wi)) * 10).to(dtype).cuda()
        empty = torch.zeros(0, dtype=torch.int32, device="cuda")
        tag, y, ix = rsz(('changeIndexes', x, empty))      # first frame: the state is written completely
        assert tag == 'changeIndexes' and tuple(y.shape) == (1, Cn, Ho, Wo) and y.dtype == dtype
        assert y is not rsz.outputState and torch.equal(raw(y), raw(rsz.outputState))
        assert np.array_equal(bits_of(host(y)), bits_of(rc.twin(host(x), rs, np.float32)))
        assert isinstance(ix, MaskChangeIndexes) and ix.size == (Ho, Wo) and ix.tensor().numel() == Ho * Wo
        for t in range(5):
            prev = host(rsz.outputState).copy()
            SI = rng.random((Hi, Wi)) < 0.1
            if t == 4:
                SI[:] = False
            refresh(x, SI, rng)
            x[0, :, 5, 69] += 1.0      # (not listed in frame 4)
            SI[5, 69] = t != 4
            if t % 3 == 0:
                form = MaskChangeIndexes(dev_words(pack(SI)), (Hi, Wi), torch.empty(Hi * Wi, dtype=torch.int32, device="cuda"),
                                         torch.zeros(1, dtype=torch.int32, device="cuda"))
            else:
                form = torch.from_numpy(np.flatnonzero(SI.reshape(-1)).astype(np.int32)).cuda()
                if t % 3 == 2:      # a device-side count in front of a longer buffer
                    form = ChangeIndexes(torch.cat([form, form.new_full((3,), 0)]),
                                         torch.tensor([form.numel()], dtype=torch.int32, device="cuda"), (Hi, Wi))
            tag, y, ix = rsz(('changeIndexes', x, form))
            if t % 3 == 0:
                assert not form._made      # the producer's list was never materialised
            listed = rc.footprint(SI, rs)
            want, got = rc.twin(host(x), rs, np.float32), host(rsz.outputState)
            assert np.array_equal(bits_of(got)[:, listed], bits_of(want)[:, listed]), (mode, t)
            assert np.array_equal(bits_of(got)[:, ~listed], bits_of(prev)[:, ~listed]), (mode, t)
            assert isinstance(ix, MaskChangeIndexes) and ix.size == (Ho, Wo)
            assert np.array_equal(host_words(ix._mask), pack(listed))
            assert np.array_equal(ix.tensor().cpu().numpy(), np.flatnonzero(listed.reshape(-1))), (mode, t)
            assert int(rsz._work['bits'].ne(0).sum()) == 0
        # a bare tensor carries no change information; cloneOutput=False hands out the tagged state
        rsz.propChangeIndexes, rsz.cloneOutput = False, False
        out = rsz(x)
        assert out is rsz.outputState and out._cbinfer_inplace_state
        assert np.array_equal(bits_of(host(out)), bits_of(rc.twin(host(x), rs, np.float32)))
        # forward(x, size=) overrides the constructor's size for this call: the state is rebuilt, written completely
        # whatever the list says, and the next call without it goes back
        for size in ((7, 75), (6, 70), None, (12, 9)):
            out = rsz(('changeIndexes', x, empty), size=size)
            geo2 = rsz.geometry(Hi, Wi, size)
            rs2 = rc.Resize(*(geo2 + rs[6:]))
            assert tuple(out.shape) == (1, Cn) + geo2[:2] and out is rsz.outputState
            assert np.array_equal(bits_of(host(out)), bits_of(rc.twin(host(x), rs2, np.float32))), (mode, size)
            # the same size again: the state fits, so the (empty) list is believed and an unlisted alteration not picked up
            kept = bits_of(host(out)).copy()
            x[0, :, 0, 0] += 1.0
            again = rsz(('changeIndexes', x, empty), size=size)
            assert again is rsz.outputState and np.array_equal(bits_of(host(again)), kept), (mode, size)
            x[0, :, 0, 0] -= 1.0
        # a restored state (clearMemory) and a new shape are written completely whatever the list says
        rsz.clearMemory()
        assert rsz.outputState.numel() == 0 and rsz._work is None
        out = rsz(('changeIndexes', x, empty))
        assert np.array_equal(bits_of(host(out)), bits_of(rc.twin(host(x), rs, np.float32)))
        x2 = x[:, :2, :4, :33].contiguous()
        out = rsz(('changeIndexes', x2, empty), size=(5, 40))
        rs3 = rc.Resize(*(rsz.geometry(4, 33, (5, 40)) + rs[6:]))
        assert np.array_equal(bits_of(host(out)), bits_of(rc.twin(host(x2), rs3, np.float32)))
        assert rsz._work['key'][:3] == (4, 33, (5, 40))
        # refusals
        Err = lib.CBinferError
        wrong = ChangeIndexes(torch.zeros(4, dtype=torch.int32, device="cuda"),
                              torch.zeros(1, dtype=torch.int32, device="cuda"), (Hi + 1, Wi))
        with pytest.raises(Err, match="%dx%d map.*%dx%d" % (Hi + 1, Wi, Hi, Wi)):
            rsz(('changeIndexes', x, wrong))
        with pytest.raises(Err, match="int32"):
            rsz(('changeIndexes', x, torch.zeros(3, dtype=torch.int64, device="cuda")))
        with pytest.raises(Err, match="ratio beyond 8"):
            rsz(x, size=(49, 70))
        with pytest.raises(Err, match="HIP devices only"):
            rsz(x.cpu())


# ------------------------------------------------------------------------------------------------ networks
NET_MODES = [('nearest', None), ('bilinear', False), ('bicubic', True)]
NET_IDS = ['nearest', 'bilinear', 'bicubic-aligned']


class Stand(nn.Module):
    """In a copy of a network, in place of its CBResize2d: the same module fed the BARE tensor -- every pixel recomputed
    -- or torch's dense F.interpolate; the change indexes handed on are those the network's own module made for the same
    frame, so that the layers behind run in the same form."""

    def __init__(self, inner, kind, lender):
        super(Stand, self).__init__()
        self.inner, self.kind = inner, kind
        self.__dict__['lender'] = lender
        inner.propChangeIndexes = False

    def forward(self, inp, size=None):
        x = inp[1] if type(inp) == tuple else inp
        if self.kind == 'bare':
            y = self.inner(x, size=size)
        else:
            m = self.inner
            kw = dict(size=size) if size is not None else (dict(size=m.size) if m.size else dict(scale_factor=m.scale_factor))
            y = F.interpolate(x, mode=m.mode, align_corners=m.align_corners if m.mode in ('bilinear', 'bicubic') else None,
                              **kw)
        lent = self.lender[0]
        return ('changeIndexes', y, lent[2]) if type(lent) == tuple else y


def lend(module):
    """The last result of `module`, kept in a one-element list."""
    box = [None]
    module.register_forward_hook(lambda mod, args, res: box.__setitem__(0, res))
    return box


def fcn_head(pkg, tdt, mode, cloneOutput):
    """3x3 CBConv2d 3 -> 8 + ReLU, a resize 12x18 -> 20x31, 1x1 CBConv2d 8 -> 4, every threshold 0."""
    torch.manual_seed(41)
    src = nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), nn.ReLU(),
                        nn.Upsample(size=(20, 31), mode=mode[0], align_corners=mode[1]), nn.Conv2d(8, 4, 1))
    net = pkg.insertCBResize(pkg.convert(src.eval().cuda().to(tdt), threshold=0.0), cloneOutput=cloneOutput)
    assert [type(m).__name__ for m in net] == ['CBConv2d', 'CBResize2d', 'CBConv2d']
    assert net[0].propChangeIndexes and net[1].propChangeIndexes and net[1].cloneOutput == cloneOutput
    if tdt == torch.float32:
        net[0].exactF32 = net[2].exactF32 = True
    return net


def with_stand(net, name, kind):
    other = copy.deepcopy(net)
    other._modules[name] = Stand(other._modules[name], kind, lend(net._modules[name]))
    return other


def moving_frames(rng, n, shape, tdt):
    """n frames of `shape`; a frame differs from the one before in two moved blocks only."""
    base = rng.random(shape) * 2 - 1
    frames = []
    for i in range(n):
        base = base.copy()
        if i:
            for _ in range(2):
                y0, x0 = int(rng.integers(0, shape[2])), int(rng.integers(0, shape[3]))
                blk = base[:, :, y0:y0 + 2, x0:x0 + 3]
                blk[...] = rng.random(blk.shape) * 2 - 1
        frames.append(torch.from_numpy(base).to(tdt).cuda())
    return frames


def listed_share(module):
    words = host_words(module._work['copy'])
    return float(np.unpackbits(words.view(np.uint8)).sum()) / float(np.prod(module._work['size']))


@pytest.mark.parametrize("cloneOutput", [True, False], ids=["clone", "inplace"])
@pytest.mark.parametrize("tdt", DTYPES, ids=["f32", "f16"])
@pytest.mark.parametrize("mode", NET_MODES, ids=NET_IDS)
def test_fcn_head_equals_the_modules_fed_bare_tensors(pkg, lib, mode, tdt, cloneOutput):
    """Six frames with local changes: outputs and the resize's state are bit-identical to a copy of the network whose
    CBResize2d is fed the bare tensor (every pixel recomputed); nearest 12 -> 20 also to the copy with torch's dense
    F.interpolate.  After the first frame the module lists a part of the map."""
    net = fcn_head(pkg, tdt, mode, cloneOutput)
    others = [with_stand(net, '2', 'bare')] + ([with_stand(net, '2', 'torch')] if mode[0] == 'nearest' else [])
    shares = []
    with torch.no_grad():
        for t, f in enumerate(moving_frames(np.random.default_rng(51), 6, (1, 3, 12, 18), tdt)):
            y = net(f).clone()
            assert tuple(y.shape) == (1, 4, 20, 31)
            shares.append(listed_share(net[1]))
            for other in others:
                yo = other(f)
                assert torch.equal(raw(y), raw(yo)), (mode, t, other._modules['2'].kind)
                if other._modules['2'].kind == 'bare':
                    assert torch.equal(raw(net[1].outputState), raw(other._modules['2'].inner.outputState)), (mode, t)
    assert shares[0] == 1.0 and 0.0 < min(shares[1:]) and max(shares[1:]) < 1.0, shares


class TopDown(nn.Module):
    """An FPN-type top-down step: lateral 1x1 on the fine map, a 3x3 layer on the coarse one, the coarse result resized
    to the SKIP'S SIZE and added."""

    def __init__(self, pkg, tdt, mode, cloneOutput):
        super(TopDown, self).__init__()
        torch.manual_seed(43)
        convs = pkg.convert(nn.Sequential(nn.Conv2d(8, 8, 1), nn.Conv2d(8, 8, 3, padding=1)).eval().cuda().to(tdt),
                            threshold=0.0)
        self.lateral, self.top = convs[0], convs[1]
        self.resize = pkg.CBResize2d(mode=mode[0], align_corners=mode[1], size=(1, 1))
        self.add = pkg.CBAdd2d()
        for m in (self.lateral, self.top, self.resize):
            m.propChangeIndexes = True
        self.resize.cloneOutput = self.add.cloneOutput = cloneOutput
        if tdt == torch.float32:
            self.lateral.exactF32 = self.top.exactF32 = True

    def forward(self, fine, coarse):
        skip = self.lateral(fine)
        up = self.resize(self.top(coarse), size=skip[1].shape[-2:])
        return self.add(up, skip)


@pytest.mark.parametrize("cloneOutput", [True, False], ids=["clone", "inplace"])
@pytest.mark.parametrize("tdt", DTYPES, ids=["f32", "f16"])
@pytest.mark.parametrize("mode", NET_MODES, ids=NET_IDS)
def test_fpn_top_down_step_equals_the_modules_fed_bare_tensors(pkg, lib, mode, tdt, cloneOutput):
    """CBResize2d to the skip's size (5x40 -> 13x100: a block's footprint spans the rows, not the columns) -> CBAdd2d, six frames with local changes on both maps: bit-identical
    to the copy whose resize is fed bare tensors, nearest 5 -> 13 also to the copy with torch's dense F.interpolate."""
    net = TopDown(pkg, tdt, mode, cloneOutput)
    others = [with_stand(net, 'resize', 'bare')] + ([with_stand(net, 'resize', 'torch')] if mode[0] == 'nearest' else [])
    fine = moving_frames(np.random.default_rng(61), 6, (1, 8, 13, 100), tdt)
    coarse = moving_frames(np.random.default_rng(62), 6, (1, 8, 5, 40), tdt)
    shares = []
    with torch.no_grad():
        for t, (f, c) in enumerate(zip(fine, coarse)):
            y = net(f, c).clone()
            assert tuple(y.shape) == (1, 8, 13, 100) and tuple(net.resize.outputState.shape) == (1, 8, 13, 100)
            shares.append(listed_share(net.resize))
            for other in others:
                assert torch.equal(raw(y), raw(other(f, c))), (mode, t, other.resize.kind)
    assert shares[0] == 1.0 and 0.0 < min(shares[1:]) and max(shares[1:]) < 1.0, shares


@pytest.mark.parametrize("tdt", DTYPES, ids=["f32", "f16"])
def test_fcn_head_records_as_a_launch_program(pkg, lib, tdt):
    """With cloneOutput=False the network is library calls only: FrameProgram records it, cbinfer_cbresize_forward is
    among the recorded calls, replays equal the eager network in outputs and states; the same layers around the dense
    nn.Upsample are refused, and the refusal names the module and its pass."""
    net = fcn_head(pkg, tdt, ('bilinear', False), cloneOutput=False)
    frames = moving_frames(np.random.default_rng(71), 7, (1, 3, 12, 18), tdt)
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
        assert raws.count(lib.C.cbinfer_cbresize_forward.raw) == 1
        assert any(t is net[1].outputState for t in pkg.getStateTensors(net))
        torch.manual_seed(41)
        src = nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), nn.ReLU(), nn.Upsample(size=(20, 31), mode='bilinear'),
                            nn.Conv2d(8, 4, 1))
        dense = pkg.convert(src.eval().cuda().to(tdt), threshold=0.0)
        for f in frames[:3]:
            dense(f)
        with pytest.raises(lib.CBinferError, match=r"torch operators.*CBResize2d \(insertCBResize\)"):
            pkg.FrameProgram(dense).record(frames[3])
