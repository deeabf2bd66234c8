#!/usr/bin/env python3
"""Target of the change-based element-wise functions (cb_pointwise.hip): fp32 and fp16, 10 % changed pixels per frame in
whole blocks (32x32 frame pixels of a 320x480 frame, i.e. 8 / 8 / 2 pixels at the three layers) --
  64 ch @ 80x120,  144 ch @ 80x120,  256 ch @ 20x30,
for ReLU6, Hardswish, SiLU and BN + ReLU.
Table 1, per layer, function and dtype: cbinfer_cbpointwise_forward with the operand in MASK form (one launch) and in
LIST form (two launches) against the dense torch operator(s) on the same tensor (F.relu6, F.hardswish, F.silu, and
F.batch_norm in eval mode followed by torch.relu).
Table 2, the chain of tests/test_gpu_pointwise.py at 80x120 with 64 -> 144 -> 144 -> 64 channels (1x1 CBConv2d ->
Hardswish -> 3x3 depthwise -> BN + ReLU6 -> 1x1 CBConv2d), frame time of: the chain with CBPointwise2d replayed by
FrameProgram, the same run eagerly, and the same converted layers with torch's dense Hardswish / BatchNorm2d / ReLU6
between them (each layer then runs its own change detection).
The measuring method is tools/target_common.py's.  Prints markdown (profiles/pointwise_target.md).
usage: pointwise_target.py [rounds]"""
import copy
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pycbinfer  # noqa: E402
from cbinfer_amd import _lib  # noqa: E402
from cbinfer_amd._lib import C, check, ptr  # noqa: E402
from target_common import (BATCH, SETS, change_sets, device_sets, dtype_name, fmt, listed_share,  # noqa: E402
                           moving_frames, rounds)

#          name, channels, H, W, block
LAYERS = [("64 ch", 64, 80, 120, 8), ("144 ch", 144, 80, 120, 8), ("256 ch", 256, 20, 30, 2)]


def batch_norm(Cn, seed, dev="cuda"):
    g = torch.Generator().manual_seed(seed)
    bn = nn.BatchNorm2d(Cn, eps=1e-3)
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(Cn, generator=g) * 0.3)
        bn.running_var.copy_(torch.rand(Cn, generator=g) * 2 + 0.05)
        bn.weight.copy_(torch.randn(Cn, generator=g))
        bn.bias.copy_(torch.randn(Cn, generator=g))
    return bn.eval().to(dev)


def functions(Cn, dtype):
    """(name, CBPointwise2d, the dense torch operator(s), tolerance of the sanity comparison in ulps of |ref| + max |ref|)"""
    bn = batch_norm(Cn, 3).to(dtype)
    return [("ReLU6", pycbinfer.CBPointwise2d(nn.ReLU6()), F.relu6, 0),
            ("Hardswish", pycbinfer.CBPointwise2d(nn.Hardswish()), F.hardswish, 2),
            ("SiLU", pycbinfer.CBPointwise2d(nn.SiLU()), F.silu, 16),
            ("BN + ReLU", pycbinfer.CBPointwise2d(nn.ReLU(), bn).cuda(),
             lambda x: torch.relu(F.batch_norm(x, bn.running_mean, bn.running_var, bn.weight, bn.bias, False, 0.0,
                                               bn.eps)), 64)]


def layer(name, Cn, H, W, block, dtype, reps):
    rng = np.random.default_rng(7)
    x = (torch.randn(1, Cn, H, W, device="cuda") * 3).to(dtype)
    sets = change_sets(rng, H, W, block, 0.10)
    masks, lists = device_sets(sets)
    words = C.cbinfer_mask_words(H, W)
    bits = torch.zeros(words, dtype=torch.int64, device="cuda")
    mcopy = torch.zeros(words, dtype=torch.int64, device="cuda")
    out = torch.empty_like(x)
    st = torch.cuda.current_stream().cuda_stream
    dt = _lib.dtype_code(x)
    listed = listed_share(sets)
    for fname, m, dense_op, ulps in functions(Cn, dtype):
        def call(mask, lst, m=m):
            check(C.cbinfer_cbpointwise_forward(ptr(x), ptr(out), ptr(mask), ptr(lst), lst.numel() if lst is not None else 0,
                                                None, ptr(bits), ptr(mcopy), Cn, H, W, m.kind, m.p0, m.p1, ptr(m.scale),
                                                ptr(m.shift), ptr(m.slope), dt, st))

        def dense(i, dense_op=dense_op):
            return dense_op(x)

        def cb_mask(i, call=call):
            call(masks[i % SETS], None)

        def cb_list(i, call=call):
            call(None, lists[i % SETS])

        # results first: with every pixel listed the frame must agree with torch's operator on the device (bit for bit
        # for ReLU6; the device's Hardswish multiplies by a rounded 1/6, SiLU and the batch norm are other formulas)
        call(None, None)
        ref = dense(0).float()
        tol = ulps * (2.0 ** -23 if dtype == torch.float32 else 2.0 ** -10)
        assert bool(((out.float() - ref).abs() <= tol * (ref.abs() + ref.abs().max())).all()), \
            "change-based frame differs from the dense operator (%s)" % fname
        t = rounds([("mask", cb_mask), ("list", cb_list), ("dense", dense)], reps)
        dm = statistics.median(t["dense"]) / statistics.median(t["mask"])
        dl = statistics.median(t["dense"]) / statistics.median(t["list"])
        print("| %s @%dx%d | %s | %s | %.1f %% | %s | %s | %s | %.2fx / %.2fx |"
              % (name, H, W, dtype_name(dtype), fname, listed, fmt(t["mask"]), fmt(t["list"]), fmt(t["dense"]), dm, dl))


def chain(dtype, reps):
    H, W, blk = 80, 120, 8
    rng = np.random.default_rng(11)
    torch.manual_seed(11)
    src = nn.Sequential()
    for name, mod in (('expand', nn.Conv2d(64, 144, 1)), ('hs', nn.Hardswish()),
                      ('dw', nn.Conv2d(144, 144, 3, 1, 1, groups=144)), ('bn', batch_norm(144, 5, "cpu")),
                      ('relu6', nn.ReLU6()), ('project', nn.Conv2d(144, 64, 1))):
        src.add_module(name, mod)
    src = src.eval().cuda().to(dtype)
    sets = change_sets(rng, H, W, blk, 0.05)
    frames = moving_frames(torch.rand(1, 64, H, W, device="cuda").to(dtype), sets, 64, dtype)

    def converted(pointwise):
        net = pycbinfer.convert(copy.deepcopy(src), threshold=0.05, depthwise=True)
        if pointwise:
            pycbinfer.linkDepthwise(pycbinfer.insertCBPointwise(net))
        for m in net:
            if hasattr(m, 'cloneOutput'):
                m.cloneOutput = False
        return net

    netP, netE, netT = converted(True), converted(True), converted(False)
    assert [type(m).__name__ for m in netP] == ['CBConv2d', 'CBPointwise2d', 'CBDepthwiseConv2d', 'CBPointwise2d',
                                                'CBConv2d']
    prog = pycbinfer.FrameProgram(netP)

    def replayed(i):
        return prog(frames[i % SETS])

    def eager(i):
        return netE(frames[i % SETS])

    def torch_acts(i):
        return netT(frames[i % SETS])

    with torch.no_grad():
        for i in range(2 * SETS):      # steady state before the frame is recorded; the same history for all three
            netP(frames[i % SETS])
            eager(i)
            torch_acts(i)
        # results first: replay and eager agree bit for bit; the dense chain within the thresholds' reach
        for i in range(SETS):
            yp, ye, yt = replayed(i), eager(i), torch_acts(i)
            assert torch.equal(yp, ye), "the replayed program differs from the eager chain"
            assert float((ye.float() - yt.float()).abs().max()) < 1.0, "the chain differs from the one with torch activations"
        t = rounds([("replayed", replayed), ("eager", eager), ("torch", torch_acts)], reps)
    changed = listed_share([m | sets[i - 1] for i, m in enumerate(sets)])
    print("| %s | %.1f %% | %s | %s | %s |" % (dtype_name(dtype), changed, fmt(t["replayed"]), fmt(t["eager"]),
                                              fmt(t["torch"])))


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    assert torch.cuda.is_available(), "pointwise_target.py needs a GPU"
    print("# Change-based element-wise functions at 10 % changed pixels\n")
    print("%s, torch %s; times in us per call, median [min..max] over %d interleaved rounds of %d calls\n"
          % (torch.cuda.get_device_name(0), torch.__version__, reps, BATCH))
    print("| layer | dtype | function | changed pixels | cbinfer_cbpointwise_forward, mask form "
          "| cbinfer_cbpointwise_forward, list form | dense torch operator(s) | dense / mask form, dense / list form |")
    print("|---|---|---|---|---|---|---|---|")
    for spec in LAYERS:
        for dtype in (torch.float32, torch.float16):
            layer(*spec, dtype=dtype, reps=reps)
    print("\n## The chain 1x1 64 -> 144, Hardswish, 3x3 depthwise, BN + ReLU6, 1x1 144 -> 64 @80x120, threshold 0.05\n")
    print("| dtype | changed input pixels per frame | CBPointwise2d, replayed by FrameProgram | CBPointwise2d, eager "
          "| torch's dense Hardswish / BatchNorm2d / ReLU6 |")
    print("|---|---|---|---|---|")
    for dtype in (torch.float32, torch.float16):
        chain(dtype, reps)


if __name__ == "__main__":
    main()
