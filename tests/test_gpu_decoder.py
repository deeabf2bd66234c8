"""-m gpu tests of the change-based decoder operators (CBUpsample2d, CBConcat2d; cb_decoder.hip).  The
reference has neither operator, so the numpy twin of tests/test_host_decoder.py IS the specification:
  rule 1  the listed pixels: upsample -- the output pixels one of whose source pixels is listed (nearest: one, bilinear:
          four, zero weights included); concat -- per operand its own pixels, handed on is the union; an operand without
          change information lists every pixel; padding bits never set;
  rule 2  the values: nearest and concat are copies, bit for bit torch's; bilinear is pinned against the twin's rules in
          float64 (fp32: 8 2^-24 max|corner|; fp16: one more rounding); every other value of the state keeps its bits;
  rule 3  the hand-on: the frame's mask in maskCopy, the working masks zero, the list made from the mask ascending."""
import copy
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from test_host_decoder import twin_corner_max, twin_footprint, twin_upsample
from optest import (dev_words, free_pixel, host_words, hostile_list, lib, pack,      # noqa: F401  (fixtures)
                    gpu_pkg as pkg, raw, stream)

pytestmark = pytest.mark.gpu

TH = 0.05
MODES = [("nearest", False), ("bilinear", False), ("bilinear", True)]
#            C, Hi, Wi, sH, sW
UP_SHAPES = [(1, 1, 1, 8, 8), (5, 3, 32, 1, 2), (5, 4, 13, 2, 5), (3, 5, 23, 3, 3), (2, 3, 70, 2, 1), (5, 2, 9, 7, 8),
             (1, 1050, 9, 2, 1)]
UP_STRIDED = (1, 1050, 9, 2, 1)      # more output mask words than workgroups: the grid-stride leg of the word walk
SENTINEL = 0x5BCD


def sel_of(mask):
    return torch.from_numpy(mask).cuda()


def up_struct(lib, sH, sW, mode, align):
    return ctypes.pointer(lib.Upsample(sH, sW, lib.UPSAMPLE_NEAREST if mode == "nearest" else lib.UPSAMPLE_BILINEAR,
                                       int(align)))


def list_args(changed, useCount):
    """(list, capacity, device count) of an int32 change list: unsorted, with a duplicate and entries outside the map;
    with a device count the buffer holds entries behind it that must not be read."""
    return hostile_list(changed, free_pixel(changed) or 0, useCount)


def refresh(t, changed, rng):
    """New values (scaled normals) at the changed pixels of every channel."""
    if changed.any():
        n = int(changed.sum())
        t[0][:, sel_of(changed)] = torch.from_numpy(rng.standard_normal((t.size(1), n)) * 10).to(t.dtype).cuda()


def input_frames(rng, H, W):
    Z = np.zeros((H, W), dtype=bool)

    def at(y, x):
        m = Z.copy()
        m[y, x] = True
        return m
    return [("single", at(H // 2, W // 2)), ("corner", at(0, 0)), ("last column", at(H - 1, W - 1)), ("empty", Z),
            ("half", rng.random((H, W)) < 0.5)]


# ------------------------------------------------------------------------------------------------ upsample, C ABI
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("mode", MODES, ids=["nearest", "bilinear", "bilinear-aligned"])
@pytest.mark.parametrize("shape", UP_SHAPES, ids=lambda s: "%dx%dx%d-x%dx%d" % s)
def test_upsample_every_form_through_the_c_abi(lib, shape, mode, dtype):
    """cbinfer_cbupsample_forward: an all-form first frame, then five frames each run in mask form and in list form (a
    device count on even frames, a host length on odd ones) on states whose unlisted values were overwritten with a
    sentinel: maskCopy is the twin's footprint, the working mask is zero, unlisted values keep the sentinel, listed ones
    equal a dense launch of the same kernel; nearest equals torch's F.interpolate."""
    C, ptr, check = lib.C, lib.ptr, lib.check
    Cn, Hi, Wi, sH, sW = shape
    Ho, Wo = Hi * sH, Wi * sW
    up = up_struct(lib, sH, sW, *mode)
    words = C.cbinfer_mask_words(Ho, Wo)
    if shape == UP_STRIDED:
        assert words > 8 * torch.cuda.get_device_properties(0).multi_processor_count
    rng = np.random.default_rng(7)
    x = torch.from_numpy(rng.standard_normal((1, Cn, Hi, Wi)) * 10).to(dtype).cuda()
    dt = lib.dtype_code(x)

    def launch(out, bits, mcopy, mask=None, lst=None, cap=0, count=None):
        check(C.cbinfer_cbupsample_forward(ptr(x), ptr(out), ptr(mask), ptr(lst), cap, ptr(count), ptr(bits), ptr(mcopy),
                                           Cn, Hi, Wi, up, dt, stream()))

    def dense_now():
        out = torch.empty((1, Cn, Ho, Wo), dtype=dtype, device="cuda")
        raw(out).fill_(SENTINEL)
        bits = torch.zeros(words, dtype=torch.int64, device="cuda")
        mcopy = torch.full((words,), -1, dtype=torch.int64, device="cuda")
        launch(out, bits, mcopy)
        assert np.array_equal(host_words(mcopy), pack(np.ones((Ho, Wo), dtype=bool)))
        assert int(bits.ne(0).sum()) == 0
        if mode[0] == "nearest":
            assert torch.equal(raw(out), raw(F.interpolate(x, scale_factor=(sH, sW), mode="nearest")))
        return out

    states = {}
    for form in ("mask", "list"):
        states[form] = dict(out=dense_now(), bits=torch.zeros(words, dtype=torch.int64, device="cuda"),
                            mcopy=torch.full((words,), -1, dtype=torch.int64, device="cuda"))
    for t, (label, SI) in enumerate(input_frames(rng, Hi, Wi)):
        refresh(x, SI, rng)
        listed = twin_footprint(SI, sH, sW, *mode)
        assert listed.shape == (Ho, Wo)
        sel = sel_of(listed)
        dense = dense_now()
        for form, st in states.items():
            where = (shape, mode, dtype, label, form)
            out, bits, mcopy = st['out'], st['bits'], st['mcopy']
            raw(out)[0][:, ~sel] = SENTINEL
            if form == "mask":
                m = dev_words(pack(SI))
                launch(out, bits, mcopy, mask=m)
            else:
                lst, cap, count = list_args(SI, useCount=t % 2 == 0)
                launch(out, bits, mcopy, lst=lst, cap=cap, count=count)
            assert np.array_equal(host_words(mcopy), pack(listed)), where
            assert int(bits.ne(0).sum()) == 0, where
            assert bool((raw(out)[0][:, ~sel] == SENTINEL).all()), where
            assert torch.equal(raw(out)[0][:, sel], raw(dense)[0][:, sel]), where
    # a list of capacity 0 (any address) is the empty frame
    st = states["list"]
    check(C.cbinfer_cbupsample_forward(ptr(x), ptr(st['out']), None, ptr(st['bits']), 0, None, ptr(st['bits']),
                                       ptr(st['mcopy']), Cn, Hi, Wi, up, dt, stream()))
    assert int(st['mcopy'].ne(0).sum()) == 0 and int(st['bits'].ne(0).sum()) == 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("align", [False, True], ids=["bilinear", "bilinear-aligned"])
@pytest.mark.parametrize("shape", UP_SHAPES, ids=lambda s: "%dx%dx%d-x%dx%d" % s)
def test_bilinear_against_float64(lib, shape, align, dtype):
    """fp32: |out - r| <= 8 2^-24 max(|a|,|b|,|c|,|d|) -- weights, products and sums carry at most one rounding each; fp16:
    <= 2^-11 |r| + 2^-25 + 9 2^-24 max(...) -- one correct rounding of that f32 value, subnormals included.  r: the
    twin's rules evaluated in float64 on the same inputs (scaled normals x 10)."""
    C, ptr, check = lib.C, lib.ptr, lib.check
    Cn, Hi, Wi, sH, sW = shape
    Ho, Wo = Hi * sH, Wi * sW
    rng = np.random.default_rng(13)
    xs = rng.standard_normal((1, Cn, Hi, Wi)) * 10
    if Hi * Wi > 4:
        xs[0, 0, 0, :3] = (3e-6, -2e-7, 6e-8)      # (values whose f16 images are subnormal)
    x = torch.from_numpy(xs).to(dtype).cuda()
    out = torch.empty((1, Cn, Ho, Wo), dtype=dtype, device="cuda")
    words = C.cbinfer_mask_words(Ho, Wo)
    bits = torch.zeros(words, dtype=torch.int64, device="cuda")
    mcopy = torch.zeros(words, dtype=torch.int64, device="cuda")
    check(C.cbinfer_cbupsample_forward(ptr(x), ptr(out), None, None, 0, None, ptr(bits), ptr(mcopy), Cn, Hi, Wi,
                                       up_struct(lib, sH, sW, "bilinear", align), lib.dtype_code(x), stream()))
    xh = x[0].cpu().numpy()
    r = twin_upsample(xh, sH, sW, "bilinear", align, np.float64)
    mx = twin_corner_max(xh, sH, sW, "bilinear", align)
    err = np.abs(out[0].cpu().numpy().astype(np.float64) - r)
    if dtype == torch.float32:
        bar = 8 * 2.0 ** -24 * mx
    else:
        bar = 2.0 ** -11 * np.abs(r) + 2.0 ** -25 + 9 * 2.0 ** -24 * mx
    share = float((err / np.where(bar > 0, bar, 1)).max())
    print("bilinear %s align_corners=%s %s: worst error %.3e, worst share of the bar %.4f"
          % (shape, align, dtype, float(err.max()), share))
    assert (err <= bar).all()


# ------------------------------------------------------------------------------------------------ concat, C ABI
CAT_CHANNELS = [(1, 3), (5, 2, 4), (2, 2, 2, 2)]
CAT_MAPS = [(1, 1), (4, 64), (3, 65), (2, 130)]
FORMS = ["mask", "list", "all"]


def cat_forms(n):
    if n == 2:
        return [(a, b) for a in FORMS for b in FORMS]
    if n == 3:
        return [("mask", "list", "all"), ("list", "mask", "mask"), ("all", "mask", "list")]
    return [("mask", "list", "all", "mask"), ("list", "list", "mask", "mask")]


def cat_frames(rng, n, H, W):
    """Per frame the pixels each operand changes."""
    Z = np.zeros((H, W), dtype=bool)
    one = Z.copy()
    one[H // 2, W // 2] = True
    last = Z.copy()
    last[H - 1, W - 1] = True
    some = rng.random((H, W)) < 0.3
    some[H - 1, 0] = True
    return [("only operand 1", [some if k == 1 else Z for k in range(n)]),
            ("disjoint", [(rng.random((H, W)) < 0.2) & ((np.arange(W)[None, :] + np.arange(H)[:, None]) % n == k)
                          for k in range(n)]),
            ("empty", [Z] * n),
            ("single and last", [one if k == 0 else (last if k == n - 1 else Z) for k in range(n)]),
            ("half", [rng.random((H, W)) < 0.5 for _ in range(n)])]


CAT_STRIDED = (2100, 9)      # more mask words than workgroups: the grid-stride leg of the kernel's loop over the words


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("size", CAT_MAPS, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("chans", CAT_CHANNELS, ids=lambda c: "+".join(map(str, c)))
def test_concat_every_form_through_the_c_abi(lib, chans, size, dtype):
    """cbinfer_cbconcat_forward on two states: one whose unlisted values are overwritten with a sentinel before every
    frame -- operand k's channels are written at operand k's pixels only -- and one left alone, which equals torch.cat
    bit for bit after every frame.  The mask handed on is the union; the working masks are zero."""
    concat_every_form(lib, chans, size, dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_concat_every_form_on_more_words_than_workgroups(lib, dtype):
    """The same on a 2100 x 9 map with the smallest channel split: every workgroup takes several words."""
    words = lib.C.cbinfer_mask_words(*CAT_STRIDED)
    assert words > 8 * torch.cuda.get_device_properties(0).multi_processor_count
    concat_every_form(lib, CAT_CHANNELS[0], CAT_STRIDED, dtype)


def concat_every_form(lib, chans, size, dtype):
    C, ptr, check = lib.C, lib.ptr, lib.check
    H, W = size
    n, total = len(chans), sum(chans)
    first = np.concatenate([[0], np.cumsum(chans)])
    words = C.cbinfer_mask_words(H, W)
    rng = np.random.default_rng(17)
    vp, ip = ctypes.c_void_p * n, ctypes.c_int32 * n

    def launch(srcs, out, bits, mcopy, ops=None):
        ops = ops or [(None, None, 0, None)] * n
        check(C.cbinfer_cbconcat_forward(vp(*[ptr(s) for s in srcs]), ip(*chans), n, ptr(out),
                                         vp(*[ptr(o[0]) for o in ops]), vp(*[ptr(o[1]) for o in ops]),
                                         ip(*[o[2] for o in ops]), vp(*[ptr(o[3]) for o in ops]), ptr(bits), ptr(mcopy),
                                         H, W, lib.dtype_code(out), stream()))

    sawSkipKept = 0
    for forms in cat_forms(n):
        srcs = [torch.from_numpy(rng.standard_normal((1, c, H, W)) * 10).to(dtype).cuda() for c in chans]
        states = []
        for _ in range(2):      # [0]: sentinel state, [1]: the clean one
            out = torch.empty((1, total, H, W), dtype=dtype, device="cuda")
            raw(out).fill_(SENTINEL)
            bits = torch.zeros(n * words, dtype=torch.int64, device="cuda")
            mcopy = torch.full((words,), -1, dtype=torch.int64, device="cuda")
            launch(srcs, out, bits, mcopy)      # the first frame: no change information
            assert torch.equal(raw(out), raw(torch.cat(srcs, 1))), (forms, "first frame")
            assert np.array_equal(host_words(mcopy), pack(np.ones((H, W), dtype=bool)))
            assert int(bits.ne(0).sum()) == 0
            states.append((out, bits, mcopy))
        for t, (label, sets) in enumerate(cat_frames(rng, n, H, W)):
            where = (chans, size, dtype, forms, label)
            for k in range(n):
                refresh(srcs[k], sets[k], rng)
            listed = [np.ones((H, W), dtype=bool) if forms[k] == "all" else sets[k] for k in range(n)]
            union = np.logical_or.reduce(listed)
            keep = []      # (the argument tensors stay alive until the checks have synchronised)
            for which, (out, bits, mcopy) in enumerate(states):
                if which == 0:
                    for k in range(n):
                        raw(out)[0, first[k]:first[k + 1]][:, sel_of(~listed[k])] = SENTINEL
                ops = []
                for k in range(n):
                    if forms[k] == "all":
                        ops.append((None, None, 0, None))
                    elif forms[k] == "mask":
                        ops.append((dev_words(pack(sets[k])), None, 0, None))
                    else:
                        ops.append((None,) + list_args(sets[k], useCount=(t + k) % 2 == 0))
                keep.append(ops)
                launch(srcs, out, bits, mcopy, ops)
                assert np.array_equal(host_words(mcopy), pack(union)), where
                assert int(bits.ne(0).sum()) == 0, where
            ref = torch.cat(srcs, 1)
            tampered, clean = states[0][0], states[1][0]
            assert torch.equal(raw(clean), raw(ref)), where
            for k in range(n):
                sel = sel_of(listed[k])
                part = raw(tampered)[0, first[k]:first[k + 1]]
                assert torch.equal(part[:, sel], raw(ref)[0, first[k]:first[k + 1]][:, sel]), where + (k,)
                assert bool((part[:, ~sel] == SENTINEL).all()), where + (k,)
            if label == "only operand 1" and forms[0] != "all":
                # operand 0 did not change: its channels hold the sentinel at operand 1's pixels
                assert bool((raw(tampered)[0, :first[1]][:, sel_of(sets[1])] == SENTINEL).all()), where
                sawSkipKept += 1
    assert sawSkipKept == sum(forms[0] != "all" for forms in cat_forms(n))


# ------------------------------------------------------------------------------------------------ modules
def test_upsample_module_forms_flags_and_errors(pkg, lib):
    from cbinfer_amd.conv2d_cg import ChangeIndexes, MaskChangeIndexes
    Err = lib.CBinferError
    Cn, Hi, Wi = 5, 6, 70
    rng = np.random.default_rng(3)
    for dtype, (mode, align), scale in ((torch.float32, ("bilinear", False), (2, 3)), (torch.float16, ("nearest", False), 2),
                                        (torch.float32, ("bilinear", True), (3, 1))):
        src = nn.Upsample(scale_factor=scale, mode=mode, align_corners=align if mode == "bilinear" else None)
        up, dense = pkg.CBUpsample2d(src), pkg.CBUpsample2d(src)
        sH, sW = up.scale_factor
        Ho, Wo = Hi * sH, Wi * sW
        up.propChangeIndexes = True
        x = torch.from_numpy(rng.standard_normal((1, Cn, Hi, Wi)) * 10).to(dtype).cuda()
        empty = torch.zeros(0, dtype=torch.int32, device="cuda")
        tag, y, ix = up(('changeIndexes', x, empty))      # first frame: the state is written completely
        assert tag == 'changeIndexes' and tuple(y.shape) == (1, Cn, Ho, Wo) and y.dtype == dtype
        assert torch.equal(raw(y), raw(dense(x))) and y is not up.outputState and torch.equal(raw(y), raw(up.outputState))
        assert isinstance(ix, MaskChangeIndexes) and ix.size == (Ho, Wo) and ix.tensor().numel() == Ho * Wo
        if mode == "nearest":
            assert torch.equal(raw(y), raw(src(x)))
        for t in range(5):
            prev = up.outputState.clone()
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
            tag, y, ix = up(('changeIndexes', x, form))
            if t % 3 == 0:
                assert not form._made      # the producer's list was never materialised
            listed = twin_footprint(SI, sH, sW, mode, align)
            sel = sel_of(listed)
            ref = dense(x)
            assert torch.equal(raw(up.outputState)[0][:, sel], raw(ref)[0][:, sel]), (dtype, mode, t)
            assert torch.equal(raw(up.outputState)[0][:, ~sel], raw(prev)[0][:, ~sel]), (dtype, mode, t)
            assert isinstance(ix, MaskChangeIndexes) and ix.size == (Ho, Wo)
            assert np.array_equal(host_words(ix._mask), pack(listed))
            assert np.array_equal(ix.tensor().cpu().numpy(), np.flatnonzero(listed.reshape(-1))), (dtype, mode, t)
            assert int(up._work['bits'].ne(0).sum()) == 0
        if t == 4:
            assert not torch.equal(raw(up.outputState), raw(dense(x)))      # (the unlisted alteration was not picked up)
        # a bare tensor carries no change information; cloneOutput=False hands out the tagged state
        up.propChangeIndexes, up.cloneOutput = False, False
        out = up(x)
        assert out is up.outputState and out._cbinfer_inplace_state and torch.equal(raw(out), raw(dense(x)))
        # a restored state (clearMemory) and a new shape are written completely whatever the list says
        up.clearMemory()
        assert up.outputState.numel() == 0 and up._work is None
        assert torch.equal(raw(up(('changeIndexes', x, empty))), raw(dense(x)))
        x2 = x[:, :3, :4, :33].contiguous()
        assert torch.equal(raw(up(('changeIndexes', x2, empty))), raw(dense(x2)))
        assert tuple(up.outputState.shape) == (1, 3, 4 * sH, 33 * sW) and up._work['key'][:2] == (4, 33)
        # refusals
        wrong = ChangeIndexes(torch.zeros(4, dtype=torch.int32, device="cuda"),
                              torch.zeros(1, dtype=torch.int32, device="cuda"), (Hi + 1, Wi))
        with pytest.raises(Err, match="%dx%d map.*%dx%d" % (Hi + 1, Wi, Hi, Wi)):
            up(('changeIndexes', x, wrong))
        with pytest.raises(Err, match="int32"):
            up(('changeIndexes', x, torch.zeros(3, dtype=torch.int64, device="cuda")))
        with pytest.raises(Err, match="device"):
            up(('changeIndexes', x, torch.zeros(3, dtype=torch.int32)))
        with pytest.raises(Err, match="int32 tensor or a ChangeIndexes"):
            up(('changeIndexes', x, [1, 2]))
        with pytest.raises(Err, match="HIP devices only"):
            up(x.cpu())


def test_concat_module_forms_flags_and_errors(pkg, lib):
    from cbinfer_amd.conv2d_cg import ChangeIndexes, MaskChangeIndexes
    Err = lib.CBinferError
    H, W, chans = 5, 70, (3, 4, 2)
    rng = np.random.default_rng(4)
    for dtype in (torch.float32, torch.float16):
        cat = pkg.CBConcat2d()
        cat.propChangeIndexes = True
        srcs = [torch.from_numpy(rng.standard_normal((1, c, H, W)) * 10).to(dtype).cuda() for c in chans]
        empty = torch.zeros(0, dtype=torch.int32, device="cuda")
        tag, y, ix = cat([('changeIndexes', s, empty) for s in srcs])      # first frame
        assert tag == 'changeIndexes' and torch.equal(raw(y), raw(torch.cat(srcs, 1))) and y is not cat.outputState
        assert isinstance(ix, MaskChangeIndexes) and ix.size == (H, W) and ix.tensor().numel() == H * W
        for t in range(4):
            prev = cat.outputState.clone()
            sets = [rng.random((H, W)) < 0.1 for _ in chans]
            if t == 3:
                sets = [np.zeros((H, W), dtype=bool)] * 3
            for s, m in zip(srcs, sets):
                refresh(s, m, rng)
            srcs[1][0, :, 4, 69] += 1.0      # (listed by nobody in frame 3)
            if t != 3:
                sets[1][4, 69] = True
            m0 = MaskChangeIndexes(dev_words(pack(sets[0])), (H, W), torch.empty(H * W, dtype=torch.int32, device="cuda"),
                                   torch.zeros(1, dtype=torch.int32, device="cuda"))
            l1 = torch.from_numpy(np.flatnonzero(sets[1].reshape(-1)).astype(np.int32)).cuda()
            l2 = torch.from_numpy(np.flatnonzero(sets[2].reshape(-1)).astype(np.int32)).cuda()
            l2 = ChangeIndexes(torch.cat([l2, l2.new_full((3,), 0)]),
                               torch.tensor([l2.numel()], dtype=torch.int32, device="cuda"), (H, W))
            tag, y, ix = cat([('changeIndexes', srcs[0], m0), ('changeIndexes', srcs[1], l1), ('changeIndexes', srcs[2], l2)])
            assert not m0._made
            ref = torch.cat(srcs, 1)
            c0 = 0
            for c, m in zip(chans, sets):
                sel = sel_of(m)
                assert torch.equal(raw(cat.outputState)[0, c0:c0 + c][:, sel], raw(ref)[0, c0:c0 + c][:, sel]), (dtype, t)
                assert torch.equal(raw(cat.outputState)[0, c0:c0 + c][:, ~sel], raw(prev)[0, c0:c0 + c][:, ~sel]), (dtype, t)
                c0 += c
            union = sets[0] | sets[1] | sets[2]
            assert np.array_equal(host_words(ix._mask), pack(union))
            assert np.array_equal(ix.tensor().cpu().numpy(), np.flatnonzero(union.reshape(-1))), (dtype, t)
            assert int(cat._work['bits'].ne(0).sum()) == 0
        assert not torch.equal(raw(cat.outputState), raw(torch.cat(srcs, 1)))      # (frame 3's unlisted alteration)
        # bare tensors: the dense concat; cloneOutput=False hands out the tagged state
        cat.propChangeIndexes, cat.cloneOutput = False, False
        out = cat([srcs[0], ('changeIndexes', srcs[1], empty), srcs[2]])
        assert out is cat.outputState and out._cbinfer_inplace_state
        assert torch.equal(raw(out)[0, :3], raw(srcs[0])[0]) and torch.equal(raw(out)[0, 7:], raw(srcs[2])[0])
        assert not torch.equal(raw(out)[0, 3:7], raw(srcs[1])[0])      # (operand 1 handed in an empty list)
        assert torch.equal(raw(cat(srcs)), raw(torch.cat(srcs, 1)))
        # another channel split of the same sum, a restored state and a new shape are written completely
        swapped = [srcs[1], srcs[0], srcs[2]]
        assert torch.equal(raw(cat([('changeIndexes', s, empty) for s in swapped])), raw(torch.cat(swapped, 1)))
        cat.clearMemory()
        assert cat.outputState.numel() == 0 and cat._work is None
        assert torch.equal(raw(cat([('changeIndexes', s, empty) for s in srcs])), raw(torch.cat(srcs, 1)))
        two = [s[:, :, :3, :40].contiguous() for s in srcs[:2]]
        assert torch.equal(raw(cat([('changeIndexes', s, empty) for s in two])), raw(torch.cat(two, 1)))
        # refusals
        wrong = ChangeIndexes(torch.zeros(4, dtype=torch.int32, device="cuda"),
                              torch.zeros(1, dtype=torch.int32, device="cuda"), (H, W + 1))
        with pytest.raises(Err, match="operand 1 address a %dx%d map.*%dx%d" % (H, W + 1, H, W)):
            cat([srcs[0], ('changeIndexes', srcs[1], wrong)])
        with pytest.raises(Err, match="int32"):
            cat([('changeIndexes', srcs[0], torch.zeros(3, dtype=torch.int64, device="cuda")), srcs[1]])
        with pytest.raises(Err, match="operands differ"):
            cat([srcs[0], srcs[1][:, :, :, :W - 1]])
        with pytest.raises(Err, match="operands differ"):
            cat([srcs[0], srcs[1].to(torch.float16 if dtype == torch.float32 else torch.float32)])
        with pytest.raises(Err, match="2..4 operands"):
            cat([srcs[0]])
        with pytest.raises(Err, match="HIP devices only"):
            cat([s.cpu() for s in srcs])


# ------------------------------------------------------------------------------------------------ end to end
class Decoder(nn.Module):
    """conv1 -> 2x2 pool -> conv2 -> upsample, concatenated with conv1's output, -> 1x1 head.  kind 'cb': the
    change-based operators fed the producers' tuples; 'bare': the same operators fed bare tensors (all form); 'torch':
    F.interpolate and torch.cat."""

    def __init__(self, body, cat, head, kind, mode):
        super(Decoder, self).__init__()
        self.body, self.cat, self.head, self.kind, self.mode = body, cat, head, kind, mode

    def forward(self, x):
        conv1, pool, conv2, up = list(self.body)
        skip = conv1(x)
        y = conv2(pool(skip))
        if self.kind == 'cb':
            return self.head(self.cat([up(y), skip]))
        if self.kind == 'bare':
            return self.head(self.cat([up(y[1]), skip[1]]))
        kw = dict(mode='bilinear', align_corners=self.mode[1]) if self.mode[0] == 'bilinear' else dict(mode='nearest')
        return self.head(torch.cat([F.interpolate(y[1], scale_factor=2, **kw), skip[1]], 1))


def make_decoder(pkg, mode, cloneOutput):
    torch.manual_seed(31)
    src = nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), nn.ReLU(), nn.MaxPool2d(2), nn.Conv2d(8, 16, 3, padding=1), nn.ReLU(),
                        nn.Upsample(scale_factor=2, mode=mode[0], align_corners=mode[1] if mode[0] == 'bilinear' else None))
    body = pkg.convert(src.eval().cuda(), threshold=TH)
    pkg.insertCBPooling(body, cloneOutput=cloneOutput)
    pkg.insertCBUpsampling(body, cloneOutput=cloneOutput)
    conv1, pool, conv2, up = list(body)
    assert type(pool) is pkg.CBPoolMax2d and type(up) is pkg.CBUpsample2d and (up.mode, up.align_corners) == mode
    assert conv1.propChangeIndexes and conv2.propChangeIndexes and conv2.copyInput and up.cloneOutput == cloneOutput
    up.propChangeIndexes = True
    cat = pkg.CBConcat2d()
    cat.cloneOutput = cloneOutput
    # (the head runs its own change detection on the concatenated map, as it does behind torch.cat)
    head = pkg.convert(nn.Sequential(nn.Conv2d(24, 4, 1)).eval().cuda(), threshold=TH)[0]
    return Decoder(body, cat, head, 'cb', mode)


def variant(net, kind):
    other = copy.deepcopy(net)
    other.kind = kind
    return other


def decoder_frames(n, seed):
    """Frames at 24x40 with block-wise changes."""
    rng = np.random.default_rng(seed)
    base = rng.random((1, 3, 24, 40)) * 0.9
    out = []
    for t in range(n):
        base = base.copy()
        for _ in range(2):
            y0, x0 = int(rng.integers(0, 24)), int(rng.integers(0, 40))
            base[:, :, y0:y0 + 5, x0:x0 + 9] = rng.random(base[:, :, y0:y0 + 5, x0:x0 + 9].shape) * 0.9
        out.append(torch.from_numpy(base.astype(np.float32)).cuda())
    return out


@pytest.mark.parametrize("mode", MODES, ids=["nearest", "bilinear", "bilinear-aligned"])
def test_decoder_network_equals_the_dense_operators(pkg, lib, mode):
    """Eight frames: nearest against the same converted layers joined by F.interpolate and torch.cat; bilinear -- whose
    values are the library's, not torch's -- against the same modules fed bare tensors.  Bit for bit, every frame, and the
    operators really ran change-based (their masks are neither full nor always empty)."""
    from cbinfer_amd.conv2d_cg import MaskChangeIndexes
    net = make_decoder(pkg, mode, cloneOutput=True)
    ref = variant(net, 'torch' if mode[0] == 'nearest' else 'bare')
    net.cat.propChangeIndexes = True
    seen = {}
    hooks = [m.register_forward_hook(lambda mod, args, res, name=name: seen.__setitem__(name, res))
             for name, m in (('up', net.body[3]), ('cat', net.cat))]
    shares = []
    with torch.no_grad():
        for t, f in enumerate(decoder_frames(8, 51)):
            # (the head behind a concat that hands its list on recomputes the listed pixels: feed it the tensor alone)
            net.head, head = nn.Identity(), net.head
            z = net(f)
            net.head = head
            y, want = head(z[1]), ref(f)
            assert tuple(y.shape) == (1, 4, 24, 40) and torch.equal(raw(y), raw(want)), (mode, t)
            assert torch.equal(raw(net.cat.outputState), raw(ref.cat.outputState if ref.kind == 'bare' else
                                                            torch.cat([seen['up'][1], net.body[0].prevOutput], 1)))
            for name, size in (('up', (24, 40)), ('cat', (24, 40))):
                tag, _, ix = seen[name]
                assert tag == 'changeIndexes' and isinstance(ix, MaskChangeIndexes) and ix.size == size
            shares.append(seen['cat'][2].tensor().numel() / (24.0 * 40.0))
    for h in hooks:
        h.remove()
    assert shares[0] == 1.0 and 0.0 < min(shares[1:]) and max(shares[1:]) < 1.0, shares


def test_decoder_network_records_as_a_launch_program(pkg, lib):
    """With cloneOutput=False the network is library calls only: FrameProgram records it, its calls hold both new entry
    points, replays equal the eager network in outputs and states; the torch-operator copy is refused."""
    net = make_decoder(pkg, ("nearest", False), cloneOutput=False)
    frames = decoder_frames(9, 52)
    with torch.no_grad():
        for f in frames[:4]:
            net(f)
        eager, dense = copy.deepcopy(net), variant(net, 'torch')
        prog = pkg.FrameProgram(net)
        for t, f in enumerate(frames[4:]):
            yp, ye, yd = prog(f), eager(f), dense(f)
            assert torch.equal(raw(yp), raw(ye)) and torch.equal(raw(ye), raw(yd)), t
            for ta, tb in zip(pkg.getStateTensors(net), pkg.getStateTensors(eager)):
                assert torch.equal(ta, tb)
        names = [fn.__name__ if hasattr(fn, '__name__') else None for fn, _ in prog.calls]
        raws = [fn for fn, _ in prog.calls]
        assert lib.C.cbinfer_cbupsample_forward.raw in raws and lib.C.cbinfer_cbconcat_forward.raw in raws, names
        assert len(pkg.getStateTensors(net)) == 2 * 3 + 1 + 2
        with pytest.raises(lib.CBinferError, match="torch operators"):
            pkg.FrameProgram(dense).record(frames[-1])
