"""-m gpu tests of the change-based rearrangements (CBPixelShuffle2d, CBChannelShuffle2d; cb_rearrange.hip, DESIGN.md
5.19).  None of the three operators computes anything, so the specification is torch's dense operator bit for bit (the
numpy twins of tests/rearrange_cases.py are pinned to it in tests/test_host_rearrange.py):
  rule 1  the listed pixels: the footprint of the input's changes on the OUTPUT map -- shuffle: the r x r block of every
          changed pixel; unshuffle: the pixels one of whose r x r input pixels changed; channel shuffle: the same
          pixel; an input without change information lists every pixel; padding bits never set;
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

import rearrange_cases as rc
from test_gpu_decoder import SENTINEL, input_frames, list_args, refresh, sel_of
from optest import dev_words, host_words, lib, pack, gpu_pkg as pkg, raw, stream      # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float16]


def torch_op(kind, f, x):
    """torch's dense operator, run on the CPU, for the device tensor x [1, C, H, W]; the result on the device."""
    v = x.detach().cpu()
    if kind == "shuffle":
        y = F.pixel_shuffle(v, f)
    elif kind == "unshuffle":
        y = F.pixel_unshuffle(v, f)
    else:
        y = F.channel_shuffle(v, f)
    return y.contiguous().cuda()


def src_module(kind, f):
    return {"shuffle": nn.PixelShuffle, "unshuffle": nn.PixelUnshuffle, "channels": nn.ChannelShuffle}[kind](f)


# ------------------------------------------------------------------------------------------------ the C ABI
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
@pytest.mark.parametrize("case", rc.cases(), ids=rc.case_id)
def test_every_form_through_the_c_abi(lib, case, dtype):
    """cbinfer_cbrearrange_forward: an all-form first frame on a sentinel-filled state, then the frames each run in mask
    form and in list form (a device count on even frames, a host length on odd ones) on states whose unlisted values were
    overwritten with a sentinel: maskCopy is the twin's footprint, the working mask is zero, unlisted values keep the
    sentinel, listed ones equal torch's operator on the current input."""
    C, ptr, check = lib.C, lib.ptr, lib.check
    kind, f, (Cn, H, W), row = case
    Co, Ho, Wo = rc.out_shape(kind, f, (Cn, H, W))
    r = ctypes.pointer(lib.Rearrange(rc.KINDS.index(kind), f))
    words = C.cbinfer_mask_words(Ho, Wo)
    if row == rc.STRIDED[kind]:      # the grid-stride leg of the word walk
        assert words > 8 * torch.cuda.get_device_properties(0).multi_processor_count
    rng = np.random.default_rng(7)
    npdt = np.float32 if dtype == torch.float32 else np.float16
    x = torch.from_numpy(rc.special_values(rng, (1, Cn, H, W), npdt)).cuda()
    dt = lib.dtype_code(x)

    def launch(out, bits, mcopy, mask=None, lst=None, cap=0, count=None):
        check(C.cbinfer_cbrearrange_forward(ptr(x), ptr(out), ptr(mask), ptr(lst), cap, ptr(count), ptr(bits), ptr(mcopy),
                                            Cn, H, W, r, dt, stream()))

    def dense_now():
        out = torch.empty((1, Co, Ho, Wo), dtype=dtype, device="cuda")
        raw(out).fill_(SENTINEL)
        bits = torch.zeros(words, dtype=torch.int64, device="cuda")
        mcopy = torch.full((words,), -1, dtype=torch.int64, device="cuda")
        launch(out, bits, mcopy)
        assert np.array_equal(host_words(mcopy), pack(np.ones((Ho, Wo), dtype=bool))), case
        assert int(bits.ne(0).sum()) == 0
        assert torch.equal(raw(out), raw(torch_op(kind, f, x))), case
        return out

    states = {}
    for form in ("mask", "list"):
        states[form] = dict(out=dense_now(), bits=torch.zeros(words, dtype=torch.int64, device="cuda"),
                            mcopy=torch.full((words,), -1, dtype=torch.int64, device="cuda"))
    frames = input_frames(rng, H, W)
    if kind == "unshuffle":
        # the only changed pixel is the LAST sub-pixel (r - 1, r - 1) of a block in the last column
        last = np.zeros((H, W), dtype=bool)
        last[(Ho // 2) * f + f - 1, W - 1] = True
        frames.append(("last sub-pixel", last))
    for t, (label, SI) in enumerate(frames):
        refresh(x, SI, rng)
        listed = rc.footprint(kind, f, SI)
        assert listed.shape == (Ho, Wo)
        if label == "last sub-pixel":
            assert listed.sum() == 1 and listed[Ho // 2, Wo - 1]
        sel = sel_of(listed)
        want = torch_op(kind, f, x)
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
    check(C.cbinfer_cbrearrange_forward(ptr(x), ptr(st['out']), None, ptr(st['bits']), 0, None, ptr(st['bits']),
                                        ptr(st['mcopy']), Cn, H, W, r, dt, stream()))
    assert int(st['mcopy'].ne(0).sum()) == 0 and int(st['bits'].ne(0).sum()) == 0


# ------------------------------------------------------------------------------------------------ modules
#               kind, factor, input (C, H, W)
MODULE_CASES = [("shuffle", 3, (18, 6, 22)),       # Wo = 66: blocks across the word boundary
                ("unshuffle", 2, (3, 8, 140)),     # three input words, two output words
                ("channels", 3, (6, 5, 70))]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
@pytest.mark.parametrize("case", MODULE_CASES, ids=lambda c: "%s-%d" % c[:2])
def test_module_forms_flags_and_errors(pkg, lib, case, dtype):
    from cbinfer_amd.conv2d_cg import ChangeIndexes, MaskChangeIndexes
    Err = lib.CBinferError
    kind, f, (Cn, Hi, Wi) = case
    Co, Ho, Wo = rc.out_shape(kind, f, (Cn, Hi, Wi))
    rng = np.random.default_rng(3)
    make = pkg.CBChannelShuffle2d if kind == "channels" else pkg.CBPixelShuffle2d
    m = make(src_module(kind, f))
    m.propChangeIndexes = True
    x = torch.from_numpy(rng.standard_normal((1, Cn, Hi, Wi)) * 10).to(dtype).cuda()
    empty = torch.zeros(0, dtype=torch.int32, device="cuda")
    tag, y, ix = m(('changeIndexes', x, empty))      # first frame: the state is written completely
    assert tag == 'changeIndexes' and tuple(y.shape) == (1, Co, Ho, Wo) and y.dtype == dtype
    assert torch.equal(raw(y), raw(torch_op(kind, f, x))) and y is not m.outputState
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
        listed = rc.footprint(kind, f, SI)
        sel = sel_of(listed)
        ref = torch_op(kind, f, x)
        assert torch.equal(raw(m.outputState)[0][:, sel], raw(ref)[0][:, sel]), (case, dtype, t)
        assert torch.equal(raw(m.outputState)[0][:, ~sel], raw(prev)[0][:, ~sel]), (case, dtype, t)
        assert isinstance(ix, MaskChangeIndexes) and ix.size == (Ho, Wo)
        assert np.array_equal(host_words(ix._mask), pack(listed))
        lst = ix.tensor().cpu().numpy()      # made on demand: ascending, the footprint
        assert np.array_equal(lst, np.flatnonzero(listed.reshape(-1))), (case, dtype, t)
        assert int(m._work['bits'].ne(0).sum()) == 0
    assert not torch.equal(raw(m.outputState), raw(torch_op(kind, f, x)))      # (frame 4's unlisted alteration)
    # a bare tensor carries no change information; cloneOutput=False hands out the tagged state
    m.propChangeIndexes, m.cloneOutput = False, False
    out = m(x)
    assert out is m.outputState and out._cbinfer_inplace_state and torch.equal(raw(out), raw(torch_op(kind, f, x)))
    # a restored state (clearMemory) and a new resolution are written completely whatever the list says
    m.clearMemory()
    assert m.outputState.numel() == 0 and m._work is None
    assert torch.equal(raw(m(('changeIndexes', x, empty))), raw(torch_op(kind, f, x)))
    state = m.outputState
    x2 = x[:, :, :Hi - 2, :Wi - 2 * f].contiguous()
    assert torch.equal(raw(m(('changeIndexes', x2, empty))), raw(torch_op(kind, f, x2)))
    assert m.outputState is not state and tuple(m.outputState.shape) == (1,) + rc.out_shape(kind, f, tuple(x2.shape[1:]))
    assert m._work['key'][:3] == (Cn, Hi - 2, Wi - 2 * f)
    # refusals
    H2, W2 = Hi - 2, Wi - 2 * f
    wrong = ChangeIndexes(torch.zeros(4, dtype=torch.int32, device="cuda"),
                          torch.zeros(1, dtype=torch.int32, device="cuda"), (H2 + 1, W2))
    with pytest.raises(Err, match="%s.*%dx%d map.*%dx%d" % (m.NAME, H2 + 1, W2, H2, W2)):
        m(('changeIndexes', x2, wrong))
    with pytest.raises(Err, match="int32"):
        m(('changeIndexes', x2, torch.zeros(3, dtype=torch.int64, device="cuda")))
    with pytest.raises(Err, match="device"):
        m(('changeIndexes', x2, torch.zeros(3, dtype=torch.int32)))
    with pytest.raises(Err, match="HIP devices only"):
        m(x2.cpu())


# ------------------------------------------------------------------------------------------------ networks
class DenseOp(nn.Module):
    """torch's dense operator (run on the CPU) in the place of a change-based rearrangement, the producer's changes
    handed through untouched where the module hands its own on (a channel shuffle keeps the map, so they still fit)."""

    def __init__(self, m, fn):
        super(DenseOp, self).__init__()
        self.fn, self.propChangeIndexes = fn, m.propChangeIndexes

    def forward(self, inp):
        x, ix = (inp[1], inp[2]) if type(inp) == tuple else (inp, None)
        y = self.fn(x.detach().cpu()).contiguous().cuda()
        return ('changeIndexes', y, ix) if self.propChangeIndexes else y


def net_frames(n, seed, channels, dtype, H=24, W=40):
    """n frames [1, channels, H, W]; a frame differs from the one before in two moved blocks only."""
    rng = np.random.default_rng(seed)
    base = rng.random((1, channels, H, W)) * 0.9
    out = []
    for t in range(n):
        base = base.copy()
        if t:
            for _ in range(2):
                y0, x0 = int(rng.integers(0, H)), int(rng.integers(0, W))
                blk = base[:, :, y0:y0 + 5, x0:x0 + 9]
                blk[...] = rng.random(blk.shape) * 0.9
        out.append(torch.from_numpy(base.astype(np.float32)).to(dtype).cuda())
    return out


def listed_share(m):
    """The share of the output map a rearrangement module listed in its last frame."""
    Ho, Wo = m.outputState.shape[2:]
    return float(np.unpackbits(host_words(m._work['copy']).view(np.uint8)).sum()) / (Ho * Wo)


def make_espcn(pkg, dtype, cloneOutput):
    """conv 3x3 + ReLU -> conv 3x3 to 4 r r channels -> PixelShuffle(2) -> conv 3x3, every threshold 0: (the network
    with the CBPixelShuffle2d, the same converted layers with torch's dense operator left in place)."""
    torch.manual_seed(41)
    src = nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), nn.ReLU(), nn.Conv2d(8, 16, 3, padding=1), nn.PixelShuffle(2),
                        nn.Conv2d(4, 3, 3, padding=1)).eval().cuda().to(dtype)
    net = pkg.convert(src, threshold=0.0)
    if dtype == torch.float32:
        for m in net:
            if type(m) is pkg.CBConv2d:
                m.exactF32 = True
    dense = copy.deepcopy(net)
    pkg.insertCBRearrange(net, cloneOutput=cloneOutput)
    assert [type(m).__name__ for m in net] == ['CBConv2d', 'CBConv2d', 'CBPixelShuffle2d', 'CBConv2d']
    assert [type(m).__name__ for m in dense] == ['CBConv2d', 'CBConv2d', 'PixelShuffle', 'CBConv2d']
    assert net[1].propChangeIndexes and net[3].copyInput and net[2].cloneOutput == cloneOutput
    return net, dense


@pytest.mark.parametrize("cloneOutput", [True, False], ids=["clone", "state"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
def test_espcn_type_network_equals_the_dense_operator(pkg, lib, dtype, cloneOutput):
    """Six frames, bit for bit in the output and in the shuffle's state, and the shuffle really ran change-based."""
    net, dense = make_espcn(pkg, dtype, cloneOutput)
    shares = []
    with torch.no_grad():
        for t, f in enumerate(net_frames(6, 61, 3, dtype)):
            y, want = net(f), dense(f)
            assert tuple(y.shape) == (1, 3, 48, 80) and torch.equal(raw(y), raw(want)), (dtype, t)
            assert torch.equal(raw(net[2].outputState), raw(F.pixel_shuffle(net[1].prevOutput, 2))), (dtype, t)
            shares.append(listed_share(net[2]))
    assert shares[0] == 1.0 and 0.0 < min(shares[1:]) and max(shares[1:]) < 0.6, shares


def make_shuffle_unit(pkg, dtype, cloneOutput):
    """A ShuffleNet-type unit in a CBResidual: grouped 1x1 + ReLU -> ChannelShuffle(3) -> depthwise 3x3 -> grouped 1x1,
    every threshold 0."""
    torch.manual_seed(43)
    src = nn.Sequential(nn.Conv2d(12, 12, 1, groups=3), nn.ReLU(), nn.ChannelShuffle(3),
                        nn.Conv2d(12, 12, 3, padding=1, groups=12), nn.Conv2d(12, 12, 1, groups=3)).eval().cuda().to(dtype)
    body = pkg.convert(src, threshold=0.0, grouped=True, depthwise=True)
    pkg.insertCBPointwise(pkg.linkDepthwise(pkg.insertCBRearrange(body, cloneOutput=cloneOutput)))
    assert [type(m).__name__ for m in body] == ['CBGroupedConv2d', 'CBChannelShuffle2d', 'CBDepthwiseConv2d',
                                                'CBGroupedConv2d']
    assert body[0].propChangeIndexes and body[1].propChangeIndexes and body[2].propagatedChanges
    assert body[1].cloneOutput == cloneOutput
    net = pkg.CBResidual(body, relu=False)
    dense = copy.deepcopy(net)
    dense.body[1] = DenseOp(net.body[1], lambda v: F.channel_shuffle(v, 3))
    return net, dense


@pytest.mark.parametrize("cloneOutput", [True, False], ids=["clone", "state"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
def test_shufflenet_type_unit_equals_the_dense_operator(pkg, lib, dtype, cloneOutput):
    """Six frames: the unit with the CBChannelShuffle2d against a deep copy -- made before the first frame -- whose
    shuffle is torch's dense operator handing the grouped layer's changes through; bit for bit in the output and in
    every layer's state.  The depthwise layer behind the shuffle ran on the shuffle's mask: it keeps no input copy."""
    net, dense = make_shuffle_unit(pkg, dtype, cloneOutput)
    shares = []
    with torch.no_grad():
        for t, f in enumerate(net_frames(6, 63, 12, dtype)):
            y, want = net(f), dense(f)
            assert tuple(y.shape) == (1, 12, 24, 40) and torch.equal(raw(y), raw(want)), (dtype, t)
            assert torch.equal(raw(net.body[1].outputState), raw(F.channel_shuffle(net.body[0].prevOutput, 3))), (dtype, t)
            for k in (0, 2, 3):
                assert torch.equal(raw(net.body[k].prevOutput), raw(dense.body[k].prevOutput)), (dtype, t, k)
            shares.append(listed_share(net.body[1]))
    assert shares[0] == 1.0 and 0.0 < min(shares[1:]) and max(shares[1:]) < 0.6, shares
    assert net.body[2].prevInput.numel() == 0


@pytest.mark.parametrize("cloneOutput", [True, False], ids=["clone", "state"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
def test_unshuffle_stem_equals_the_dense_operator(pkg, lib, dtype, cloneOutput):
    """A PixelUnshuffle(2) stem in front of a CBConv2d, fed a bare tensor: every frame is written completely and equals
    the same layer behind torch's operator."""
    torch.manual_seed(47)
    conv = pkg.convert(nn.Sequential(nn.Conv2d(12, 8, 3, padding=1)).eval().cuda().to(dtype), threshold=0.0)[0]
    conv.copyInput = True
    stem = pkg.CBPixelShuffle2d(nn.PixelUnshuffle(2))
    stem.cloneOutput = cloneOutput
    net, dense = nn.Sequential(stem, conv), nn.Sequential(nn.PixelUnshuffle(2), copy.deepcopy(conv))
    with torch.no_grad():
        for t, f in enumerate(net_frames(6, 67, 3, dtype)):
            y, want = net(f), dense(f)
            assert tuple(y.shape) == (1, 8, 12, 20) and torch.equal(raw(y), raw(want)), (dtype, t)
            assert torch.equal(raw(stem.outputState), raw(F.pixel_unshuffle(f, 2))) and listed_share(stem) == 1.0


def test_espcn_type_network_records_as_a_launch_program(pkg, lib):
    """With cloneOutput=False the network is library calls only: FrameProgram records it, the shuffle is ONE call of the
    recorded frame, replays equal the eager network and the network with torch's operator in outputs and states; the
    network with torch's operator is refused."""
    net, dense = make_espcn(pkg, torch.float32, cloneOutput=False)
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
        assert raws.count(lib.C.cbinfer_cbrearrange_forward.raw) == 1
        assert len(pkg.getStateTensors(net)) == 2 * 3 + 1
        with pytest.raises(lib.CBinferError, match="torch operators.*CBPixelShuffle2d"):
            pkg.FrameProgram(dense).record(frames[-1])
