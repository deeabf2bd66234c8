"""-m gpu tests of the change-based residual add (CBAdd2d, CBResidual; cb_add.hip).  The reference has no
element-wise sum, so the twin written here IS the specification:
  rule 1  the listed pixels: the union of the two operands' changes (an operand without change information lists every
          pixel), padding bits never set;
  rule 2  the values: at listed pixels torch's own relu?(a + b) of the same device tensors (fp32 and fp16); every other
          pixel of the state keeps its bits;
  rule 3  the hand-on: the frame's union mask in maskCopy, the working mask zero, the list made from the mask ascending.
There is no tolerance anywhere in this file."""
import copy
import pickle

import numpy as np
import pytest
import torch
import torch.nn as nn
from optest import (dev_words, host_words, lib, operand_args, pack, gpu_pkg as pkg,      # noqa: F401  (fixtures)
                    raw, stream)

pytestmark = pytest.mark.gpu

TH = 0.05
SHAPES = [(1, 3, 64), (5, 5, 70), (67, 9, 130), (3, 2, 1), (1, 2100, 9)]
STRIDED = (1, 2100, 9)      # more mask words than workgroups: the grid-stride leg of the word walk
FORMS = ["mask", "list", "all"]


def twin(a, b, relu):
    """Rule 2: torch on the same tensors."""
    return torch.relu(a + b) if relu else a + b


def frame_sets(rng, H, W):
    """(label, pixels operand a changes, pixels operand b changes) of the frames behind the first one."""
    Z = np.zeros((H, W), dtype=bool)

    def at(*pixels):
        m = Z.copy()
        for y, x in pixels:
            m[y, x] = True
        return m
    word = Z.copy()
    word[0, :min(W, 64)] = True
    A = rng.random((H, W)) < 0.1
    B = (rng.random((H, W)) < 0.1) & ~A
    A2, B2 = rng.random((H, W)) < 0.2, rng.random((H, W)) < 0.2
    A2[0, 0] = B2[0, 0] = True
    return [("empty", Z, Z), ("single", at((H // 2, W // 2)), Z), ("full word", word, Z),
            ("last column", Z, at((H - 1, W - 1))), ("both corners", at((0, 0)), at((H - 1, W - 1))),
            ("disjoint", A, B), ("overlapping", A2, B2), ("empty again", Z, Z)]


def refresh(t, changed, rng):
    """New values (negative ones among them) at the changed pixels of every channel."""
    if changed.any():
        sel = torch.from_numpy(changed).cuda()
        n = int(changed.sum())
        t[0][:, sel] = torch.from_numpy(rng.standard_normal((t.size(1), n))).to(t.dtype).cuda()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_every_operand_form_through_the_c_abi(lib, shape, dtype):
    """cbinfer_cbadd_forward, relu on and off, all nine pairs of operand forms; after every frame the state equals
    torch's relu?(a + b) at the listed pixels and keeps its bits elsewhere -- also where an operand was altered at a
    pixel in neither list --, the mask handed on is the numpy union, the working mask is zero and the compacted list is
    ascending with the right count."""
    C, ptr, check = lib.C, lib.ptr, lib.check
    Cn, H, W = shape
    words = C.cbinfer_mask_words(H, W)
    assert words == H * ((W + 63) // 64)
    if shape == STRIDED:
        assert words > 8 * torch.cuda.get_device_properties(0).multi_processor_count
    rng = np.random.default_rng(11)
    sawUnlisted = 0
    for relu in (0, 1):
        for fa in FORMS:
            for fb in FORMS:
                a = torch.from_numpy(rng.standard_normal((1, Cn, H, W))).to(dtype).cuda()
                b = torch.from_numpy(rng.standard_normal((1, Cn, H, W))).to(dtype).cuda()
                out = torch.empty_like(a)
                raw(out).fill_(0x5BCD)
                bits = torch.zeros(words, dtype=torch.int64, device="cuda")
                mcopy = torch.full((words,), -1, dtype=torch.int64, device="cuda")
                # the first frame: no change information, the state is written completely
                check(C.cbinfer_cbadd_forward(ptr(a), ptr(b), ptr(out), None, None, 0, None, None, None, 0, None,
                                              ptr(bits), ptr(mcopy), Cn, H, W, relu, lib.dtype_code(a), stream()))
                assert torch.equal(out, twin(a, b, relu)), (fa, fb, relu, "first frame")
                assert np.array_equal(host_words(mcopy), pack(np.ones((H, W), dtype=bool)))
                assert int(bits.ne(0).sum().item()) == 0
                # (two operands, two lists, a first frame without either: this loop stays here -- optest.walk_frames
                # walks one operand -- and takes the operand forms from optest)
                for t, (label, SA, SB) in enumerate(frame_sets(rng, H, W)):
                    where = (shape, dtype, relu, fa, fb, label)
                    prev = out.clone()
                    refresh(a, SA, rng)
                    refresh(b, SB, rng)
                    # an operand altered where NEITHER list says so: a dense sum would pick it up
                    free = np.flatnonzero(~(SA | SB).reshape(-1))
                    if len(free):
                        p = int(free[len(free) // 2])
                        (a if t % 2 else b)[0, :, p // W, p % W] += 3.0
                    listed = np.ones((H, W), dtype=bool) if "all" in (fa, fb) else (SA | SB)
                    ma, la, ca, na = operand_args(fa, SA, 0, use_count=True)
                    mb, lb, cb, nb = operand_args(fb, SB, H * W - 1, use_count=False)
                    check(C.cbinfer_cbadd_forward(ptr(a), ptr(b), ptr(out), ptr(ma), ptr(la), ca, ptr(na), ptr(mb), ptr(lb),
                                                  cb, ptr(nb), ptr(bits), ptr(mcopy), Cn, H, W, relu, lib.dtype_code(a),
                                                  stream()))
                    ref = twin(a, b, relu)
                    sel = torch.from_numpy(listed).cuda()
                    assert torch.equal(out[0][:, sel], ref[0][:, sel]), where
                    assert torch.equal(raw(out)[0][:, ~sel], raw(prev)[0][:, ~sel]), where
                    if len(free) and not listed.all():
                        assert not listed[p // W, p % W]
                        # (with relu both may be zero; counted where the dense sum would have differed)
                        sawUnlisted += int(not torch.equal(ref[0, :, p // W, p % W], prev[0, :, p // W, p % W]))
                    assert np.array_equal(host_words(mcopy), pack(listed)), where
                    assert int(bits.ne(0).sum().item()) == 0, where
                    lst = torch.full((H * W,), -1, dtype=torch.int32, device="cuda")
                    cnt = torch.full((1,), -1, dtype=torch.int32, device="cuda")
                    check(C.cbinfer_compact_bits(ptr(mcopy), W, H, ptr(lst), ptr(cnt), None, None, stream()))
                    n = int(cnt.item())
                    assert n == int(listed.sum()), where
                    assert np.array_equal(lst[:n].cpu().numpy(), np.flatnonzero(listed.reshape(-1))), where
    assert sawUnlisted >= 2 * 4 * 4      # (every pair without an 'all' operand, at least half of its eight frames)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_nan_and_negative_values_through_relu(lib, dtype):
    """relu keeps a NaN a NaN (as torch.relu), zeroes the negative sums and -inf, keeps +inf; without relu they all pass.
    cbinfer_add_changed, the mask-driven launch alone, with the mask given as the working mask."""
    C, ptr, check = lib.C, lib.ptr, lib.check
    Cn, H, W = 3, 4, 70
    rng = np.random.default_rng(5)
    a = torch.from_numpy(rng.standard_normal((1, Cn, H, W))).to(dtype).cuda()
    b = torch.from_numpy(rng.standard_normal((1, Cn, H, W))).to(dtype).cuda()
    a[0, 0, 1, 3], a[0, 1, 1, 3], a[0, 2, 1, 3] = float('nan'), float('inf'), -float('inf')
    a[0, 0, 3, 69], b[0, 0, 3, 69] = float('inf'), -float('inf')      # inf - inf: a NaN made by the sum itself
    a[0, 1, 3, 69], b[0, 1, 3, 69] = -2.0, 0.5
    a[0, 2, 3, 69], b[0, 2, 3, 69] = 65000.0, 65000.0      # (overflows in f16)
    changed = np.zeros((H, W), dtype=bool)
    changed[1, 3] = changed[3, 69] = changed[0, 0] = True
    words = C.cbinfer_mask_words(H, W)
    for relu in (1, 0):
        out = torch.zeros_like(a)
        bits = dev_words(pack(changed))
        mcopy = torch.zeros(words, dtype=torch.int64, device="cuda")
        check(C.cbinfer_add_changed(ptr(a), ptr(b), ptr(out), None, 0, None, 0, ptr(bits), ptr(mcopy), Cn, H, W, relu,
                                    lib.dtype_code(a), stream()))
        ref = twin(a, b, relu)
        sel = torch.from_numpy(changed).cuda()
        got, want = out[0][:, sel], ref[0][:, sel]
        assert int(want.isnan().sum()) == 2 and torch.equal(got.isnan(), want.isnan())
        assert torch.equal(torch.nan_to_num(got, nan=7.0), torch.nan_to_num(want, nan=7.0))
        if relu:
            assert float(got.nan_to_num(nan=0.0).min()) == 0.0 and float(out[0, 1, 3, 69]) == 0.0
            assert float(out[0, 2, 1, 3]) == 0.0 and float(out[0, 1, 1, 3]) == float('inf')
        else:
            assert float(out[0, 1, 3, 69]) == -1.5 and float(out[0, 2, 1, 3]) == -float('inf')
        assert int(raw(out)[0][:, ~sel].ne(0).sum()) == 0
        assert int(bits.ne(0).sum()) == 0 and np.array_equal(host_words(mcopy), pack(changed))


def test_module_forms_flags_and_errors(pkg, lib):
    """CBAdd2d: a new state is written completely whatever the lists say; a MaskChangeIndexes is taken as its mask and
    its list never made; ChangeIndexes and exact tensors as lists; the flags of CBPoolMax2d; the refusals."""
    from cbinfer_amd.conv2d_cg import ChangeIndexes, MaskChangeIndexes
    Cn, H, W = 5, 7, 70
    rng = np.random.default_rng(3)
    for dtype in (torch.float32, torch.float16):
        a = torch.from_numpy(rng.standard_normal((1, Cn, H, W))).to(dtype).cuda()
        b = torch.from_numpy(rng.standard_normal((1, Cn, H, W))).to(dtype).cuda()
        add = pkg.CBAdd2d(relu=True)
        add.propChangeIndexes = True
        empty = torch.zeros(0, dtype=torch.int32, device="cuda")
        tag, y, ix = add(('changeIndexes', a, empty), ('changeIndexes', b, empty))      # first frame
        assert tag == 'changeIndexes' and torch.equal(add.outputState, torch.relu(a + b))
        assert y is not add.outputState and torch.equal(y, add.outputState)
        assert isinstance(ix, MaskChangeIndexes) and ix.size == (H, W) and not ix._made
        assert ix.tensor().numel() == H * W
        for t in range(4):
            prev = add.outputState.clone()
            SA, SB = rng.random((H, W)) < 0.1, rng.random((H, W)) < 0.1
            if t == 3:
                SA[:], SB[:] = False, False
            refresh(a, SA, rng)
            refresh(b, SB, rng)
            a[0, :, 6, 69] += 1.0      # (listed by neither operand in frame 3)
            ma = MaskChangeIndexes(dev_words(pack(SA)), (H, W), torch.empty(H * W, dtype=torch.int32, device="cuda"),
                                   torch.zeros(1, dtype=torch.int32, device="cuda"))
            lb = torch.from_numpy(np.flatnonzero(SB.reshape(-1)).astype(np.int32)).cuda()
            if t % 2:      # a device-side count in front of a longer buffer
                lb = ChangeIndexes(torch.cat([lb, lb.new_full((3,), 6 * W + 69)]),
                                   torch.tensor([lb.numel()], dtype=torch.int32, device="cuda"), (H, W))
            tag, y, ix = add(('changeIndexes', a, ma), ('changeIndexes', b, lb))
            assert not ma._made      # the producer's list was never materialised
            listed = SA | SB
            sel = torch.from_numpy(listed).cuda()
            ref = torch.relu(a + b)
            assert torch.equal(add.outputState[0][:, sel], ref[0][:, sel]), (dtype, t)
            assert torch.equal(raw(add.outputState)[0][:, ~sel], raw(prev)[0][:, ~sel]), (dtype, t)
            assert np.array_equal(host_words(ix._mask), pack(listed))
            assert np.array_equal(ix.tensor().cpu().numpy(), np.flatnonzero(listed.reshape(-1))), (dtype, t)
            assert int(add._addWork['bits'].ne(0).sum()) == 0
        # a bare tensor carries no change information: the dense sum
        add.propChangeIndexes, add.cloneOutput = False, False
        out = add(a, ('changeIndexes', b, empty))
        assert out is add.outputState and out._cbinfer_inplace_state and torch.equal(out, torch.relu(a + b))
        # refusals
        Err = lib.CBinferError
        wrong = ChangeIndexes(torch.zeros(4, dtype=torch.int32, device="cuda"),
                              torch.zeros(1, dtype=torch.int32, device="cuda"), (H + 1, W))
        with pytest.raises(Err, match="%dx%d map.*%dx%d" % (H + 1, W, H, W)):
            add(a, ('changeIndexes', b, wrong))
        with pytest.raises(Err, match="int32"):
            add(('changeIndexes', a, torch.zeros(3, dtype=torch.int64, device="cuda")), b)
        with pytest.raises(Err, match="device"):
            add(('changeIndexes', a, torch.zeros(3, dtype=torch.int32)), b)
        with pytest.raises(Err, match="operands differ"):
            add(a, b[:, :, :, :W - 1])
        with pytest.raises(Err, match="operands differ"):
            add(a, b.to(torch.float16 if dtype == torch.float32 else torch.float32))
        with pytest.raises(Err, match="HIP devices only"):
            add(a.cpu(), b.cpu())
        before = add.outputState.clone()
        torch.cuda.synchronize()
        assert torch.equal(raw(add.outputState), raw(before))
        add.clearMemory()
        assert add.outputState.numel() == 0 and add._addWork is None


# ------------------------------------------------------------------------------------------------ a two-block network
def _conv_bn(ci, co, k, s, p):
    bn = nn.BatchNorm2d(co)
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(co) * 0.1)
        bn.running_var.copy_(torch.rand(co) + 0.5)
        bn.weight.copy_(torch.rand(co) + 0.5)
        bn.bias.copy_(torch.randn(co) * 0.1)
    return [nn.Conv2d(ci, co, k, s, p, bias=False), bn]


def make_net(pkg):
    """8-channel stem + general 3x3/s2/p1 max pool, an identity block 8 -> 8, a downsample block 8 -> 16 (body 3x3/s2/p1,
    shortcut 1x1/s2); every convolution bias-free with a batch norm behind it, folded."""
    torch.manual_seed(23)
    parts = dict(stem=nn.Sequential(*_conv_bn(3, 8, 3, 1, 1), nn.ReLU(), nn.MaxPool2d(3, 2, 1)),
                 body1=nn.Sequential(*_conv_bn(8, 8, 3, 1, 1), nn.ReLU(), *_conv_bn(8, 8, 3, 1, 1)),
                 body2=nn.Sequential(*_conv_bn(8, 16, 3, 2, 1), nn.ReLU(), *_conv_bn(16, 16, 3, 1, 1)),
                 short2=nn.Sequential(*_conv_bn(8, 16, 1, 2, 0)))
    cb = {}
    for name, seq in parts.items():
        seq = pkg.foldBatchNorm(seq.eval().cuda())
        assert not any(type(m) is nn.BatchNorm2d for m in seq)
        cb[name] = pkg.convert(seq, threshold=TH, generalGeometry=True)
    net = nn.Sequential()
    net.add_module('stem', cb['stem'])
    net.add_module('block1', pkg.CBResidual(cb['body1']))
    net.add_module('block2', pkg.CBResidual(cb['body2'], cb['short2']))
    pkg.insertCBPooling(net, cloneOutput=False, generalGeometry=True)
    pool = net.stem[1]
    assert type(pool) is pkg.CBPoolMax2d and pool._general and not pool.cloneOutput and net.stem[0].propChangeIndexes
    pool.propChangeIndexes = True
    net.block1.add.propChangeIndexes = True
    net.block1.add.cloneOutput = net.block2.add.cloneOutput = False
    return net


def net_frames(n, seed):
    """Frames at 64x80 with block-wise changes."""
    rng = np.random.default_rng(seed)
    base = rng.random((1, 3, 64, 80)) * 0.9
    out = []
    for t in range(n):
        base = base.copy()
        for _ in range(3):
            y0, x0 = int(rng.integers(0, 64)), int(rng.integers(0, 80))
            base[:, :, y0:y0 + 9, x0:x0 + 14] = rng.random(base[:, :, y0:y0 + 9, x0:x0 + 14].shape) * 0.9
        out.append(torch.from_numpy(base.astype(np.float32)).cuda())
    return out


def test_two_block_network_records_as_a_launch_program(pkg, lib):
    """Over 6 frames every CBAdd2d.outputState is relu(a + b) of its two operand tensors, bit for bit; FrameProgram
    records the network (with torch's add it refuses), replays equal the eager network in outputs and states; clearMemory
    restarts the sequence with identical outputs; a pickle round trip carries on identically."""
    net = make_net(pkg)
    seen = {}
    hooks = [m.register_forward_pre_hook(lambda mod, args, name=name: seen.__setitem__(name, args))
             for name, m in net.named_modules() if type(m) is pkg.CBAdd2d]
    assert len(hooks) == 2
    frames = net_frames(6, 41)
    firstPass = []
    with torch.no_grad():
        for t, f in enumerate(frames):
            y = net(f)
            assert tuple(y.shape) == (1, 16, 16, 20) and y is net.block2.add.outputState
            for name, (a, b) in seen.items():
                a, b = (x[1] if type(x) == tuple else x for x in (a, b))
                state = net.get_submodule(name).outputState
                assert torch.equal(state, torch.relu(a + b)), (name, t)
            if t:      # behind the first frame the operands carry their changes
                assert type(seen['block1.add'][0]) == tuple and type(seen['block1.add'][1]) == tuple
                assert type(seen['block2.add'][0]) == tuple and type(seen['block2.add'][1]) == tuple
            firstPass.append(y.clone())
        for h in hooks:
            h.remove()
        assert len(pkg.getStateTensors(net)) == 2 * 6 + 1 + 2
        # the frame as a recorded launch program
        eager = copy.deepcopy(net)
        more = net_frames(5, 42)
        prog = pkg.FrameProgram(net)
        for f in more[:4]:
            yp, ye = prog(f), eager(f)
            assert torch.equal(yp, ye)
            for ta, tb in zip(pkg.getStateTensors(net), pkg.getStateTensors(eager)):
                assert torch.equal(ta, tb)
        assert prog.calls is not None and any(fn is lib.C.cbinfer_cbadd_forward.raw for fn, _ in prog.calls)
        # a pickle round trip carries on where the network is
        again = pickle.loads(pickle.dumps(eager))
        assert again.block1.add._addWork is None and torch.equal(again.block2.add.outputState, eager.block2.add.outputState)
        assert torch.equal(again(more[4]), eager(more[4]))
        for ta, tb in zip(pkg.getStateTensors(again), pkg.getStateTensors(eager)):
            assert torch.equal(ta, tb)
        # clearMemory restarts the sequence
        pkg.clearMemory(eager)
        assert eager.block1.add.outputState.numel() == 0
        for f, want in zip(frames, firstPass):
            assert torch.equal(eager(f), want)


def test_torch_add_network_is_refused_by_frame_program(pkg, lib):
    """What the block costs without CBAdd2d: the same layers with torch's add + relu cannot be recorded."""
    net = make_net(pkg)

    class TorchBlock(nn.Module):
        def __init__(self, stem, body):
            super(TorchBlock, self).__init__()
            self.stem, self.body = stem, body

        def forward(self, x):
            x = self.stem(x)[1]
            return torch.relu(self.body(x)[1] + x)
    dense = TorchBlock(net.stem, net.block1.body)
    frames = net_frames(3, 43)
    with torch.no_grad():
        for f in frames:
            dense(f)
        with pytest.raises(lib.CBinferError, match="torch operators"):
            pkg.FrameProgram(dense).record(frames[-1])
