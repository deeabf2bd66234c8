"""-m gpu tests of the change-based padding (CBPad2d, insertCBPadding, splitConvPadding; cb_pad.hip).
A pad computes nothing, so the specification is torch's dense F.pad bit for bit (the numpy twin of tests/pad_cases.py is
pinned to it in tests/test_host_pad.py):
  rule 1  the listed pixels: an output pixel is listed iff the input pixel it reads is listed -- its own image and its
          reflections, wraps or replicated border run; a constant-mode border pixel reads nothing and is never listed, a
          cropped-off input pixel lists nothing; an input without change information lists every pixel; padding bits
          never set;
  rule 2  the values: at listed pixels torch's operator on the current input, bit for bit; every other value of the
          state keeps its bits;
  rule 3  the hand-on: the frame's mask in maskCopy, the working mask zero, the list made from the mask ascending."""
import copy
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import pad_cases as pc
from rearrange_cases import special_values
from test_gpu_decoder import SENTINEL, input_frames, list_args, refresh, sel_of
from test_gpu_geom import bound_for
from test_gpu_rearrange import net_frames
from optest import dev_words, host_words, lib, pack, gpu_pkg as pkg, raw, stream      # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float16]
VALUE = -3.5      # of the constant-mode cases: a border that is not the zero of a fresh buffer


def torch_pad(mode, pads, x, value=VALUE):
    """torch's dense operator, run on the CPU, for the device tensor x [1, C, H, W]; the result on the device."""
    return F.pad(x.detach().cpu(), pads, mode=mode, value=value if mode == "constant" else 0.0).contiguous().cuda()


# ------------------------------------------------------------------------------------------------ the C ABI
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
@pytest.mark.parametrize("case", pc.CASES, ids=pc.case_id)
def test_every_form_through_the_c_abi(lib, case, dtype):
    """cbinfer_cbpad_forward: an all-form first frame on a sentinel-filled state, then the frames each run in mask form
    and in list form (a device count on even frames, a host length on odd ones) on states whose unlisted values were
    overwritten with a sentinel: maskCopy is the twin's footprint, the working mask is zero, unlisted values keep the
    sentinel, listed ones equal torch's operator on the current input.  A crop case ends with a changed pixel in the
    cropped-off region, which lists nothing."""
    C, ptr, check = lib.C, lib.ptr, lib.check
    mode, pads, (Cn, H, W) = case
    _, Ho, Wo = pc.out_shape(pads, (Cn, H, W))
    p = ctypes.pointer(lib.Pad(pc.MODES.index(mode), *(pads + (VALUE,))))
    words = C.cbinfer_mask_words(Ho, Wo)
    if (Cn, H, W) == pc.STRIDED_SHAPE:      # the grid-stride leg of the word walk
        assert words > 8 * torch.cuda.get_device_properties(0).multi_processor_count
    rng = np.random.default_rng(7)
    npdt = np.float32 if dtype == torch.float32 else np.float16
    x = torch.from_numpy(special_values(rng, (1, Cn, H, W), npdt)).cuda()
    dt = lib.dtype_code(x)

    def launch(out, bits, mcopy, mask=None, lst=None, cap=0, count=None):
        check(C.cbinfer_cbpad_forward(ptr(x), ptr(out), ptr(mask), ptr(lst), cap, ptr(count), ptr(bits), ptr(mcopy),
                                      Cn, H, W, p, dt, stream()))

    def dense_now():
        out = torch.empty((1, Cn, Ho, Wo), dtype=dtype, device="cuda")
        raw(out).fill_(SENTINEL)
        bits = torch.zeros(words, dtype=torch.int64, device="cuda")
        mcopy = torch.full((words,), -1, dtype=torch.int64, device="cuda")
        launch(out, bits, mcopy)
        assert np.array_equal(host_words(mcopy), pack(np.ones((Ho, Wo), dtype=bool))), case
        assert int(bits.ne(0).sum()) == 0
        assert torch.equal(raw(out), raw(torch_pad(mode, pads, x))), case
        return out

    states = {}
    for form in ("mask", "list"):
        states[form] = dict(out=dense_now(), bits=torch.zeros(words, dtype=torch.int64, device="cuda"),
                            mcopy=torch.full((words,), -1, dtype=torch.int64, device="cuda"))
    frames = input_frames(rng, H, W)
    most = np.zeros((H, W), dtype=bool)      # the pixel that reflections read most often
    most[min(1, H - 1), min(1, W - 1)] = True
    frames.append(("read most", most))
    if case in pc.CROPS:
        left, right, top, bottom = pads
        off = np.zeros((H, W), dtype=bool)
        off[0 if top < 0 else H - 1 if bottom < 0 else 0, 0 if left < 0 else W - 1 if right < 0 else 0] = True
        frames.append(("cropped off", off))
    for t, (label, SI) in enumerate(frames):
        refresh(x, SI, rng)
        listed = pc.footprint(mode, pads, SI)
        assert listed.shape == (Ho, Wo)
        if label == "cropped off":
            assert SI.sum() == 1 and not listed.any()
        sel = sel_of(listed)
        want = torch_pad(mode, pads, x)
        for form, st in states.items():
            where = (case, dtype, label, form)
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
            assert torch.equal(raw(out)[0][:, sel], raw(want)[0][:, sel]), where
    # a list of capacity 0 (any address) is the empty frame
    st = states["list"]
    check(C.cbinfer_cbpad_forward(ptr(x), ptr(st['out']), None, ptr(st['bits']), 0, None, ptr(st['bits']),
                                  ptr(st['mcopy']), Cn, H, W, p, dt, stream()))
    assert int(st['mcopy'].ne(0).sum()) == 0 and int(st['bits'].ne(0).sum()) == 0


# ------------------------------------------------------------------------------------------------ the module
#               mode, (left, right, top, bottom), input (C, H, W)
MODULE_CASES = [("constant", (3, 3, 1, 2), (5, 6, 60)),      # Wo = 66
                ("reflect", (2, 5, 2, 1), (3, 6, 62)),       # the right reflection crosses the word boundary
                ("replicate", (2, 64, 0, 1), (3, 5, 70)),    # a 65-bit run across three words
                ("circular", (4, 1, 0, 2), (2, 5, 63))]


def src_module(mode, pads):
    if mode == "constant":
        return nn.ConstantPad2d(pads, VALUE)
    return {"reflect": nn.ReflectionPad2d, "replicate": nn.ReplicationPad2d, "circular": nn.CircularPad2d}[mode](pads)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
@pytest.mark.parametrize("case", MODULE_CASES, ids=lambda c: c[0])
def test_module_forms_flags_and_errors(pkg, lib, case, dtype):
    from cbinfer_amd.conv2d_cg import ChangeIndexes, MaskChangeIndexes
    Err = lib.CBinferError
    mode, pads, (Cn, Hi, Wi) = case
    _, Ho, Wo = pc.out_shape(pads, (Cn, Hi, Wi))
    rng = np.random.default_rng(3)
    m = pkg.CBPad2d(src_module(mode, pads))
    m.propChangeIndexes = True
    x = torch.from_numpy(rng.standard_normal((1, Cn, Hi, Wi)) * 10).to(dtype).cuda()
    empty = torch.zeros(0, dtype=torch.int32, device="cuda")
    tag, y, ix = m(('changeIndexes', x, empty))      # first frame: the state is written completely
    assert tag == 'changeIndexes' and tuple(y.shape) == (1, Cn, Ho, Wo) and y.dtype == dtype
    assert torch.equal(raw(y), raw(torch_pad(mode, pads, x))) and y is not m.outputState
    assert torch.equal(raw(y), raw(m.outputState))
    assert isinstance(ix, MaskChangeIndexes) and ix.size == (Ho, Wo) and ix.tensor().numel() == Ho * Wo
    for t in range(5):
        prev = m.outputState.clone()
        SI = rng.random((Hi, Wi)) < 0.1
        if t == 4:
            SI[:] = False
        refresh(x, SI, rng)
        x[0, :, Hi - 1, Wi - 1] += 1.0      # (not listed in frame 4)
        SI[Hi - 1, Wi - 1] = t != 4
        if t % 3 == 0:
            form = MaskChangeIndexes(dev_words(pack(SI)), (Hi, Wi), torch.empty(Hi * Wi, dtype=torch.int32, device="cuda"),
                                     torch.zeros(1, dtype=torch.int32, device="cuda"))
        else:
            form = torch.from_numpy(np.flatnonzero(SI.reshape(-1)).astype(np.int32)).cuda()
            if t % 3 == 2:      # a device-side count in front of a longer buffer
                form = ChangeIndexes(torch.cat([form, form.new_full((3,), 0)]),
                                     torch.tensor([form.numel()], dtype=torch.int32, device="cuda"), (Hi, Wi))
        tag, y, ix = m(('changeIndexes', x, form))
        if t % 3 == 0:
            assert not form._made      # the producer's list was never materialised
        listed = pc.footprint(mode, pads, SI)
        sel = sel_of(listed)
        ref = torch_pad(mode, pads, x)
        assert torch.equal(raw(m.outputState)[0][:, sel], raw(ref)[0][:, sel]), (case, dtype, t)
        assert torch.equal(raw(m.outputState)[0][:, ~sel], raw(prev)[0][:, ~sel]), (case, dtype, t)
        assert isinstance(ix, MaskChangeIndexes) and ix.size == (Ho, Wo)
        assert np.array_equal(host_words(ix._mask), pack(listed))
        lst = ix.tensor().cpu().numpy()      # made on demand: ascending, the footprint
        assert np.array_equal(lst, np.flatnonzero(listed.reshape(-1))), (case, dtype, t)
        assert int(m._work['bits'].ne(0).sum()) == 0
    assert not torch.equal(raw(m.outputState), raw(torch_pad(mode, pads, x)))      # (frame 4's unlisted alteration)
    # a bare tensor carries no change information; cloneOutput=False hands out the tagged state
    m.propChangeIndexes, m.cloneOutput = False, False
    out = m(x)
    assert out is m.outputState and out._cbinfer_inplace_state and torch.equal(raw(out), raw(torch_pad(mode, pads, x)))
    # a restored state (clearMemory) and a new resolution are written completely whatever the list says
    m.clearMemory()
    assert m.outputState.numel() == 0 and m._work is None
    assert torch.equal(raw(m(('changeIndexes', x, empty))), raw(torch_pad(mode, pads, x)))
    state = m.outputState
    H2, W2 = Hi - 2, Wi - 2
    x2 = x[:, :, :H2, :W2].contiguous()
    assert torch.equal(raw(m(('changeIndexes', x2, empty))), raw(torch_pad(mode, pads, x2)))
    assert m.outputState is not state and tuple(m.outputState.shape) == (1,) + pc.out_shape(pads, (Cn, H2, W2))
    assert m._work['key'][:3] == (Cn, H2, W2)
    # refusals of the operand
    wrong = ChangeIndexes(torch.zeros(4, dtype=torch.int32, device="cuda"),
                          torch.zeros(1, dtype=torch.int32, device="cuda"), (H2 + 1, W2))
    with pytest.raises(Err, match="CBPad2d.*%dx%d map.*%dx%d" % (H2 + 1, W2, H2, W2)):
        m(('changeIndexes', x2, wrong))
    with pytest.raises(Err, match="int32"):
        m(('changeIndexes', x2, torch.zeros(3, dtype=torch.int64, device="cuda")))
    with pytest.raises(Err, match="device"):
        m(('changeIndexes', x2, torch.zeros(3, dtype=torch.int32)))
    with pytest.raises(Err, match="HIP devices only"):
        m(x2.cpu())
    # refusals of the first frame: what depends on the map or on the dtype
    with pytest.raises(Err, match=r"mode='reflect' of a %dx%d map.*below the extent" % (Hi, Wi)):
        pkg.CBPad2d(nn.ReflectionPad2d((0, 0, Hi, 0)))(x)
    with pytest.raises(Err, match=r"mode='circular' of a %dx%d map" % (Hi, Wi)):
        pkg.CBPad2d(nn.CircularPad2d((0, 0, 0, Hi + 1)))(x)
    over = pkg.CBPad2d(padding=1, value=1e6)
    if dtype == torch.float16:
        with pytest.raises(Err, match="value=1000000.0 of a %dx%d float16 map overflows" % (Hi, Wi)):
            over(x)
        assert over.outputState.numel() == 0
    else:
        assert torch.equal(raw(over(x)), raw(torch_pad("constant", (1, 1, 1, 1), x, value=1e6)))


# ------------------------------------------------------------------------------------------------ networks
def listed_share(m):
    """The share of the output map a CBPad2d listed in its last frame."""
    Ho, Wo = m.outputState.shape[2:]
    return float(np.unpackbits(host_words(m._work['copy']).view(np.uint8)).sum()) / (Ho * Wo)


def operand_of(module):
    """The tensor `module` was last fed, kept in a one-element list."""
    box = [None]
    module.register_forward_pre_hook(lambda mod, args: box.__setitem__(0, args[0][1] if type(args[0]) == tuple else args[0]))
    return box


def exact_f32(pkg, net, dtype):
    if dtype == torch.float32:
        for m in net.modules():
            if type(m) is pkg.CBConv2d:
                m.exactF32 = True


def make_monodepth(pkg, dtype, cloneOutput):
    """A monodepth2-type run: conv 3x3 + ReLU -> ReflectionPad2d(1) -> valid conv 3x3 + ReLU -> ZeroPad2d((1, 0, 1, 0)) ->
    conv 1x1, every threshold 0: (the network with the two CBPad2d, the same converted layers with torch's dense pads
    left in place)."""
    torch.manual_seed(41)
    src = nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), nn.ReLU(), nn.ReflectionPad2d(1), nn.Conv2d(8, 8, 3), nn.ReLU(),
                        nn.ZeroPad2d((1, 0, 1, 0)), nn.Conv2d(8, 4, 1)).eval().cuda().to(dtype)
    net = pkg.convert(src, threshold=0.0, generalGeometry=True)
    exact_f32(pkg, net, dtype)
    dense = copy.deepcopy(net)
    pkg.insertCBPadding(net, cloneOutput=cloneOutput)
    assert [type(m).__name__ for m in net] == ['CBConv2d', 'CBPad2d', 'CBConv2d', 'CBPad2d', 'CBConv2d']
    assert [type(m).__name__ for m in dense] == ['CBConv2d', 'ReflectionPad2d', 'CBConv2d', 'ZeroPad2d', 'CBConv2d']
    assert net[0].propChangeIndexes and net[2].propChangeIndexes and net[2].copyInput and net[3].propChangeIndexes
    assert net[1].cloneOutput == cloneOutput and net[3].cloneOutput == cloneOutput
    return net, dense


@pytest.mark.parametrize("cloneOutput", [True, False], ids=["clone", "state"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
def test_monodepth_type_run_equals_the_dense_pads(pkg, lib, dtype, cloneOutput):
    """Six frames, bit for bit in the output and in both pads' states, and the pads really ran change-based: the two 5x9
    blocks dilated by two 3x3 layers cover about a quarter of the map at most, so the listed share stays below 0.6."""
    net, dense = make_monodepth(pkg, dtype, cloneOutput)
    fed = [operand_of(net[1]), operand_of(net[3])]
    shares = []
    with torch.no_grad():
        for t, f in enumerate(net_frames(6, 61, 3, dtype)):
            y, want = net(f), dense(f)
            assert tuple(y.shape) == (1, 4, 25, 41) and torch.equal(raw(y), raw(want)), (dtype, t)
            assert tuple(net[1].outputState.shape) == (1, 8, 26, 42) and tuple(net[3].outputState.shape) == (1, 8, 25, 41)
            assert torch.equal(raw(net[1].outputState), raw(F.pad(fed[0][0], (1, 1, 1, 1), mode='reflect'))), (dtype, t)
            assert torch.equal(raw(net[3].outputState), raw(F.pad(fed[1][0], (1, 0, 1, 0)))), (dtype, t)
            shares.append((listed_share(net[1]), listed_share(net[3])))
    assert shares[0] == (1.0, 1.0), shares
    assert 0.0 < min(min(s) for s in shares[1:]) and max(max(s) for s in shares[1:]) < 0.6, shares


def make_padding_mode_net(pkg, dtype, cloneOutput):
    """conv 3x3 + ReLU -> conv 3x3 padding_mode='replicate' + ReLU -> conv 3x3 padding (1, 2) padding_mode='circular',
    every threshold 0, through splitConvPadding -> convert -> insertCBPadding: (the network with the two CBPad2d, the same
    converted layers with torch's dense pads, the original torch network)."""
    torch.manual_seed(43)
    src = nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), nn.ReLU(), nn.Conv2d(8, 8, 3, padding=1, padding_mode='replicate'),
                        nn.ReLU(), nn.Conv2d(8, 4, 3, padding=(1, 2), padding_mode='circular')).eval().cuda().to(dtype)
    orig = copy.deepcopy(src)
    net = pkg.convert(pkg.splitConvPadding(src), threshold=0.0, generalGeometry=True)
    exact_f32(pkg, net, dtype)
    dense = copy.deepcopy(net)
    pkg.insertCBPadding(net, cloneOutput=cloneOutput)
    assert [type(m).__name__ for m in net] == ['CBConv2d', 'CBPad2d', 'CBConv2d', 'CBPad2d', 'CBConv2d']
    assert [type(m).__name__ for m in dense] == ['CBConv2d', 'ReplicationPad2d', 'CBConv2d', 'CircularPad2d', 'CBConv2d']
    assert (net[1].mode, net[1].padding, net[3].mode, net[3].padding) == ('replicate', (1, 1, 1, 1), 'circular', (2, 2, 1, 1))
    return net, dense, orig


@pytest.mark.parametrize("cloneOutput", [True, False], ids=["clone", "state"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
def test_padding_mode_network_equals_the_dense_pads_and_tracks_torch(pkg, lib, dtype, cloneOutput):
    """Six frames: bit for bit against the same converted layers with torch's dense pads, and against the ORIGINAL unsplit
    torch network (in float64 on the CPU, the reference of tests/test_gpu_geom.py) within that file's bar for a converted
    general-geometry layer at threshold 0 -- fp32 1e-4 absolute, fp16 4 * 2^-10 * max(1, |ref|max)."""
    net, dense, orig = make_padding_mode_net(pkg, dtype, cloneOutput)
    orig = orig.cpu().double()
    shares = []
    with torch.no_grad():
        for t, f in enumerate(net_frames(6, 63, 3, dtype)):
            y, want = net(f), dense(f)
            assert tuple(y.shape) == (1, 4, 24, 42) and torch.equal(raw(y), raw(want)), (dtype, t)
            ref = orig(f.cpu().double())
            err = (y.cpu().double() - ref).abs().max().item()
            print("%s frame %d: |err| %.3g, bar %.3g" % (dtype, t, err, bound_for(dtype, ref.numpy())))
            assert err <= bound_for(dtype, ref.numpy()), (dtype, t, err)
            shares.append((listed_share(net[1]), listed_share(net[3])))
    assert shares[0] == (1.0, 1.0), shares
    assert 0.0 < min(min(s) for s in shares[1:]) and max(max(s) for s in shares[1:]) < 0.6, shares


@pytest.mark.parametrize("cloneOutput", [True, False], ids=["clone", "state"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
def test_reflection_stem_equals_the_dense_operator(pkg, lib, dtype, cloneOutput):
    """A hand-built CBPad2d(nn.ReflectionPad2d(3)) stem in front of a valid 7x7 CBConv2d, fed a bare tensor: every frame
    is written completely and equals the same layer behind torch's operator."""
    torch.manual_seed(47)
    conv = pkg.convert(nn.Sequential(nn.Conv2d(3, 8, 7)).eval().cuda().to(dtype), threshold=0.0, generalGeometry=True)[0]
    conv.copyInput = True
    exact_f32(pkg, conv, dtype)
    stem = pkg.CBPad2d(nn.ReflectionPad2d(3))
    stem.cloneOutput = cloneOutput
    net, dense = nn.Sequential(stem, conv), nn.Sequential(nn.ReflectionPad2d(3), copy.deepcopy(conv))
    with torch.no_grad():
        for t, f in enumerate(net_frames(6, 67, 3, dtype)):
            y, want = net(f), dense(f)
            assert tuple(y.shape) == (1, 8, 24, 40) and torch.equal(raw(y), raw(want)), (dtype, t)
            assert torch.equal(raw(stem.outputState), raw(F.pad(f, (3, 3, 3, 3), mode='reflect')))
            assert listed_share(stem) == 1.0


def test_monodepth_type_run_records_as_a_launch_program(pkg, lib):
    """With cloneOutput=False the network is library calls only: FrameProgram records it, each pad is ONE call of the
    recorded frame, replays equal the eager network and the network with torch's pads in outputs and states; the network
    with torch's pads is refused."""
    net, dense = make_monodepth(pkg, torch.float32, cloneOutput=False)
    frames = net_frames(8, 71, 3, torch.float32)
    with torch.no_grad():
        for f in frames[:4]:
            net(f)
            dense(f)
        eager = copy.deepcopy(net)
        prog = pkg.FrameProgram(net)
        for t, f in enumerate(frames[4:]):
            yp, ye, yd = prog(f), eager(f), dense(f)
            assert torch.equal(raw(yp), raw(ye)) and torch.equal(raw(ye), raw(yd)), t
            for ta, tb in zip(pkg.getStateTensors(net), pkg.getStateTensors(eager)):
                assert torch.equal(ta, tb), t
        raws = [fn for fn, _ in prog.calls]
        assert raws.count(lib.C.cbinfer_cbpad_forward.raw) == 2
        states = pkg.getStateTensors(net)
        assert all(any(t is m.outputState for t in states) for m in (net[1], net[3]))
        assert len(states) == len(pkg.getStateTensors(dense)) + 2
        with pytest.raises(lib.CBinferError, match=r"torch operators.*CBPad2d \(insertCBPadding\)"):
            pkg.FrameProgram(dense).record(frames[-1])
