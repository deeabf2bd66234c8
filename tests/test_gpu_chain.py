"""-m gpu: every accepted (pass, producer type) pair of chain.PRODUCERS run on the device (tests/chain_cases.py, DESIGN.md
5.17), over eight 12 x 70 frames: a dense one, three with one or two changed pixels, an idle one, the corner pixel, two
blocks, every pixel.  No tolerance is involved but in (c):
  (a)  the producer's contract -- the pixels at which the tensor it returns differs bitwise from last frame's are a subset
       of the set it hands on; the list is ascending, unique and inside the map, the mask has no padding bit, .size is
       the producer's output map; the idle frame returns the same bits and hands on nothing;
  (b)  the consumer against every pixel -- the pass's operator and its state equal, bit for bit, a twin (a deep copy taken
       before the first frame) fed a clone of the same tensor with EVERY pixel listed; the pools also torch's CPU operator;
  (c)  a consumer with its own detection (insertCBTransposedConv), threshold 0: fed what the producer returned it equals
       the twin fed a clone, and both lie within tests/test_gpu_tconv.py's bound of float64 math;
  (d)  not vacuous -- on the one- and two-pixel frames the operator lists more than nothing and less than half of its map
       (tests/test_host_chain.py has the footprints by numpy dilation), on the idle frame nothing.
Every message carries (pass, producer, op, dtype, cloneOutput, handed, frame).  A second test records each network as a
FrameProgram."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import chain_cases as cc
from test_gpu_pad import operand_of
from test_gpu_tconv import bound_of, tconv64
from optest import host_words, lib, pack, gpu_pkg as pkg, raw      # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

DTYPES = {'f32': torch.float32, 'f16': torch.float16}
HANDED = ('as handed', 'list made first')
_FRAMES = {}


def frames(dtype):
    """The eight frames on the device: made once per dtype, never written."""
    if dtype not in _FRAMES:
        _FRAMES[dtype] = [f.cuda() for f in cc.frames(dtype)]
    return _FRAMES[dtype]


def legs(case, dtype):
    """'list made first' only where the producer hands on a mask whose list is not made."""
    two = cc.hands_of(case.producer, dtype) == 'mask' and case.passName not in cc.OWN_DETECTION
    return HANDED if two else HANDED[:1]


RUNS = [pytest.param(case, dt, clone, handed, id='%s-%s-%s-%s' % (cc.case_id(case), dt, 'clone' if clone else 'state',
                                                                   handed))
        for case in cc.CASES for dt in DTYPES for clone in (True, False) for handed in legs(case, DTYPES[dt])]


def handed_set(ix, size, kind, where):
    """The bool map of the pixels the producer handed on, from the mask words or -- a plain list -- from a clone of it;
    the form is the one chain_cases names for the producer."""
    from cbinfer_amd.conv2d_cg import ChangeIndexes, MaskChangeIndexes
    Ho, Wo = size
    assert isinstance(ix, ChangeIndexes) and ix.size == (Ho, Wo), where
    assert isinstance(ix, MaskChangeIndexes) == (kind != 'list'), (where, type(ix).__name__)
    lst = None
    if isinstance(ix, MaskChangeIndexes):
        assert ix._mask is not None and (kind == 'mask' or ix._made), where
        words = host_words(ix._mask)
        assert words.size == Ho * ((Wo + 63) // 64), where
        bits = np.unpackbits(words.view(np.uint8), bitorder='little').reshape(Ho, -1).astype(bool)
        assert not bits[:, Wo:].any(), where      # (no padding bit)
        listed = bits[:, :Wo]
        assert np.array_equal(words, pack(listed)), where
        if ix._made:
            lst = ix._idx[:int(ix._cnt.item())].cpu().numpy()
            assert np.array_equal(lst, np.flatnonzero(listed.reshape(-1))), where
    else:
        lst = ix.clone().tensor().cpu().numpy()
        listed = np.zeros(Ho * Wo, dtype=bool)
        assert lst.size == 0 or (lst.min() >= 0 and lst.max() < Ho * Wo), where
        listed[lst] = True
        listed = listed.reshape(Ho, Wo)
    if lst is not None:
        assert lst.dtype == np.int32 and bool((np.diff(lst) > 0).all()), where      # (ascending, unique)
    return listed


def own_mask(op):
    """(mask copy, output map) of the operator's last frame; None for the reference's 2x2 pool, which keeps no mask."""
    from cbinfer_amd.chain import CBStateModule
    if isinstance(op, CBStateModule):
        work, state = op.__dict__[op._WORK], op.outputState
    elif hasattr(op, '_poolWork'):
        work, state = op.__dict__['_poolWork'], op.outputState
    else:
        work, state = op.__dict__['_work'], op.prevOutput
    return None if work is None else (work['copy'], tuple(state.shape[2:]))


def share_of(op, handed):
    """The share of its map the operator listed in its last frame, as listed_share() of the operators' own files reads
    it; for an operator without a mask, of the producer's map in the handed-on set."""
    own = own_mask(op)
    if own is None:
        return float(handed.mean())
    return float(np.unpackbits(host_words(own[0]).view(np.uint8)).sum()) / (own[1][0] * own[1][1])


def state_of(m):
    return m.outputState if hasattr(m, 'outputState') else m.prevOutput


def torch_pool(case, x):
    """torch's CPU operator of a pooling case on the device tensor x, or None."""
    x = x.cpu()
    return {'MaxPool2d(2)': lambda: F.max_pool2d(x, 2), 'MaxPool2d(3, 2, 1)': lambda: F.max_pool2d(x, 3, 2, 1),
            'AvgPool2d(2)': lambda: F.avg_pool2d(x, 2)}.get(case.op, lambda: None)()


@pytest.mark.parametrize("case,dt,cloneOutput,handed", RUNS)
def test_every_accepted_pair_on_the_device(pkg, lib, case, dt, cloneOutput, handed):
    from cbinfer_amd.chain import CBStateModule
    from cbinfer_amd.conv2d_cg import MaskChangeIndexes
    dtype = DTYPES[dt]
    net = cc.build(pkg, case, dtype, 'cuda', cloneOutput)
    prod, op = net.seq[1], net.seq[2]
    own = case.passName in cc.OWN_DETECTION
    if own:
        op.threshold = 0.0
    twin = copy.deepcopy(op)
    returned = [None]
    prod.register_forward_hook(lambda mod, args, out: returned.__setitem__(0, out))
    fed = operand_of(op)
    if handed == 'list made first':
        def make_first(mod, args):
            assert isinstance(args[0][2], MaskChangeIndexes) and not args[0][2]._made
            args[0][2].buffer
        op.register_forward_pre_hook(make_first)
    kind = cc.hands_of(case.producer, dtype)
    before, shares = None, {}
    with torch.no_grad():
        for t, f in enumerate(frames(dtype)):
            where = tuple(case) + (dt, cloneOutput, handed, t)
            y = net(f)
            assert torch.is_tensor(y), where
            got = returned[0]
            assert (type(got) == tuple) == (not own), where
            x = (got[1] if type(got) == tuple else got)
            assert fed[0] is x, where
            if hasattr(cc.hand_on_target(prod), 'cloneOutput'):
                assert (x is state_of(cc.hand_on_target(prod))) == (not cloneOutput), where
            x = x.clone()
            size = tuple(x.shape[2:])
            # (a) the producer's contract
            moved = (raw(x) != raw(before)).any(dim=1)[0].cpu().numpy() if t else np.ones(size, dtype=bool)
            listed = None
            if not own:
                listed = handed_set(got[2], size, kind, where)
                assert not (moved & ~listed).any(), (where, "changed outside the handed-on set",
                                                     np.argwhere(moved & ~listed)[:4].tolist())
            if t == cc.IDLE:
                assert not moved.any() and (listed is None or not listed.any()), where
            # (b), (c) the consumer against every pixel
            if isinstance(op, CBStateModule) or own:
                want = twin(x)
            else:
                want = twin(('changeIndexes', x, torch.arange(size[0] * size[1], dtype=torch.int32, device=x.device)))
            assert y.shape == want.shape and torch.equal(raw(y), raw(want)), (where, "output")
            assert torch.equal(raw(state_of(op)), raw(state_of(twin))), (where, "state")
            assert (y is state_of(op)) == (not cloneOutput), where
            dense = torch_pool(case, x)
            if dense is not None:
                assert torch.equal(raw(y.cpu()), raw(dense)), (where, "torch's CPU pool")
            if own:
                g = (op.kernel_size, op.stride, op.padding, op.dilation, op.output_padding)
                ref = tconv64(x, op.weight, op.bias, g)
                mag = tconv64(x.abs(), op.weight.abs(), None, g) + op.bias.detach().cpu().double().abs().view(1, -1, 1, 1)
                n = op.in_channels * g[0][0] * g[0][1]
                err = (y.cpu().double() - ref).abs()
                bound = bound_of('F16' if dtype == torch.float16 else 'F32S', n, ref, mag)
                assert bool((err <= bound).all()), (where, float((err / bound).max()))
            # (d) not vacuous
            shares[t] = share_of(op, listed)
            if t in cc.LOCAL:
                assert 0.0 < shares[t] < 0.5, (where, shares)
            if t == cc.IDLE:
                assert shares[t] == 0.0, (where, shares)
            before = x


# ------------------------------------------------------------------------------------------------ recording
# The cases whose frame legitimately runs torch operators, so that FrameProgram refuses it by its documented message:
# the reference's 2x2 CBPoolMax2d as a producer hands on the OUTPUT-resolution list (downsampleIndexes), which
# conv2d_cg.poolChangeIndexes makes in freshly allocated buffers every frame, as the reference does.
RUNS_TORCH_OPERATORS = {cc.case_id(c): "poolChangeIndexes allocates the output-resolution list every frame"
                        for c in cc.CASES if c.producer == 'CBPoolMax2d 2x2' and c.passName not in cc.OWN_DETECTION}


@pytest.mark.parametrize("case", cc.CASES, ids=cc.case_id)
def test_every_accepted_pair_records_as_a_launch_program(pkg, lib, case):
    """fp32, cloneOutput=False, as handed: after three eager frames FrameProgram records the network, and the remaining
    five frames replayed equal a deep copy of the eager network bit for bit, outputs and every state tensor."""
    net = cc.build(pkg, case, torch.float32, 'cuda', cloneOutput=False)
    fr = frames(torch.float32)
    with torch.no_grad():
        for f in fr[:cc.RECORD_AFTER]:
            net(f)
        prog = pkg.FrameProgram(net)
        if cc.case_id(case) in RUNS_TORCH_OPERATORS:
            with pytest.raises(lib.CBinferError, match=r"ran torch operators a replay would not repeat"):
                prog.record(fr[cc.RECORD_AFTER])
            return
        eager = copy.deepcopy(net)
        for t, f in enumerate(fr[cc.RECORD_AFTER:], cc.RECORD_AFTER):
            where = tuple(case) + (t,)
            yp, ye = prog(f), eager(f)
            assert torch.equal(raw(yp), raw(ye)), (where, "output")
            states, want = pkg.getStateTensors(net), pkg.getStateTensors(eager)
            assert len(states) == len(want) >= 3, where
            for k, (ta, tb) in enumerate(zip(states, want)):
                assert ta.shape == tb.shape and torch.equal(ta, tb), (where, "state tensor %d" % k)
