#!/usr/bin/env python3
"""Target of the change-based per-pixel channel reductions (cb_chanreduce.hip): fp32 and fp16, 10 % changed pixels per
frame in whole blocks (32x32 frame pixels of a 320x480 frame, i.e. 8 / 2 pixels at the two resolutions) --
  LayerNorm with affine: 96 ch @ 80x120, 384 ch @ 20x30;   Softmax: 21 ch and 150 ch @ 80x120.
Table 1, per layer, function and dtype: cbinfer_cbchanreduce_forward with the operand in MASK form (one launch) and in
LIST form (two launches) against the dense torch operator on the same tensor (F.layer_norm on the permuted view, the two
permutes included -- its result is a view, as a channels-first LayerNorm module returns it --, and F.softmax over dim 1).
Table 2, a ConvNeXt-type chain at 80x120 with 96 channels (1x1 CBConv2d -> 7x7 depthwise -> channels-first LayerNorm ->
1x1 CBConv2d), frame time of: the chain with CBChannelReduce2d replayed by FrameProgram, the same run eagerly, and the
same converted layers with torch's dense LayerNorm in the middle (the layer behind it then runs its own detection).
The measuring method is tools/target_common.py's.  Prints markdown (profiles/channel_target.md).
usage: channel_target.py [rounds]"""
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

#          name, function, channels, H, W, block
LAYERS = [("96 ch", "LayerNorm", 96, 80, 120, 8), ("384 ch", "LayerNorm", 384, 20, 30, 2),
          ("21 ch", "Softmax", 21, 80, 120, 8), ("150 ch", "Softmax", 150, 80, 120, 8)]


class LayerNorm2d(nn.Module):
    """A channels-first layer norm as ConvNeXt implementations write it (torch has no such class)."""

    def __init__(self, Cn, eps=1e-6):
        super(LayerNorm2d, self).__init__()
        g = torch.Generator().manual_seed(Cn)
        self.weight = nn.Parameter(torch.rand(Cn, generator=g) + 0.5)
        self.bias = nn.Parameter(torch.randn(Cn, generator=g) * 0.3)
        self.eps, self.Cn = eps, Cn

    def forward(self, x):
        return F.layer_norm(x.permute(0, 2, 3, 1), (self.Cn,), self.weight, self.bias, self.eps).permute(0, 3, 1, 2)


def layer(name, fname, Cn, H, W, block, dtype, reps):
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
    if fname == "LayerNorm":
        ln = LayerNorm2d(Cn).cuda().to(dtype)
        m = pycbinfer.CBChannelReduce2d(ln, layerNormTypes=(LayerNorm2d,))
        dense_op, ulps = ln, 64
    else:
        m = pycbinfer.CBChannelReduce2d(nn.Softmax2d())
        dense_op, ulps = (lambda t: F.softmax(t, 1)), 16

    def call(mask, lst):
        check(C.cbinfer_cbchanreduce_forward(ptr(x), ptr(out), ptr(mask), ptr(lst), lst.numel() if lst is not None else 0,
                                             None, ptr(bits), ptr(mcopy), Cn, H, W, m.kind, m.eps, ptr(m.gamma),
                                             ptr(m.beta), dt, st))

    def dense(i):
        return dense_op(x)

    def cb_mask(i):
        call(masks[i % SETS], None)

    def cb_list(i):
        call(None, lists[i % SETS])

    with torch.no_grad():
        # results first: with every pixel listed the frame must agree with torch's operator on the device (another
        # summation order and, in fp16, torch's own intermediate roundings: a loose sanity bar, not the specification's)
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
    H, W, blk, Cn = 80, 120, 8, 96
    rng = np.random.default_rng(11)
    torch.manual_seed(11)
    src = nn.Sequential()
    for name, mod in (('expand', nn.Conv2d(Cn, Cn, 1)), ('dw', nn.Conv2d(Cn, Cn, 7, 1, 3, groups=Cn)),
                      ('norm', LayerNorm2d(Cn)), ('project', nn.Conv2d(Cn, 4 * Cn, 1))):
        src.add_module(name, mod)
    src = src.eval().cuda().to(dtype)
    sets = change_sets(rng, H, W, blk, 0.05)
    frames = moving_frames(torch.rand(1, Cn, H, W, device="cuda").to(dtype), sets, Cn, dtype)

    def converted(channelOps):
        net = pycbinfer.convert(copy.deepcopy(src), threshold=0.05, depthwise=True)
        pycbinfer.linkDepthwise(net)
        if channelOps:
            pycbinfer.insertCBChannelOps(net, layerNormTypes=(LayerNorm2d,))
        for m in net:
            if hasattr(m, 'cloneOutput'):
                m.cloneOutput = False
        return net

    netP, netE, netT = converted(True), converted(True), converted(False)
    assert [type(m).__name__ for m in netP] == ['CBConv2d', 'CBDepthwiseConv2d', 'CBChannelReduce2d', 'CBConv2d']
    assert [type(m).__name__ for m in netT] == ['CBConv2d', 'CBDepthwiseConv2d', 'LayerNorm2d', 'CBConv2d']
    prog = pycbinfer.FrameProgram(netP)

    def replayed(i):
        return prog(frames[i % SETS])

    def eager(i):
        return netE(frames[i % SETS])

    def torch_norm(i):
        return netT(frames[i % SETS])

    with torch.no_grad():
        for i in range(2 * SETS):      # steady state before the frame is recorded; the same history for all three
            netP(frames[i % SETS])
            eager(i)
            torch_norm(i)
        # results first: replay and eager agree bit for bit; the dense chain within the thresholds' reach
        for i in range(SETS):
            yp, ye, yt = replayed(i), eager(i), torch_norm(i)
            assert torch.equal(yp, ye), "the replayed program differs from the eager chain"
            assert float((ye.float() - yt.float()).abs().max()) < 1.0, "the chain differs from the one with torch's LayerNorm"
        t = rounds([("replayed", replayed), ("eager", eager), ("torch", torch_norm)], reps)
    changed = listed_share([m | sets[i - 1] for i, m in enumerate(sets)])
    print("| %s | %.1f %% | %s | %s | %s |" % (dtype_name(dtype), changed, fmt(t["replayed"]), fmt(t["eager"]),
                                              fmt(t["torch"])))


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    assert torch.cuda.is_available(), "channel_target.py needs a GPU"
    print("# Change-based per-pixel channel reductions at 10 % changed pixels\n")
    print("%s, torch %s; times in us per call, median [min..max] over %d interleaved rounds of %d calls\n"
          % (torch.cuda.get_device_name(0), torch.__version__, reps, BATCH))
    print("| layer | dtype | function | changed pixels | cbinfer_cbchanreduce_forward, mask form "
          "| cbinfer_cbchanreduce_forward, list form | dense torch operator | dense / mask form, dense / list form |")
    print("|---|---|---|---|---|---|---|---|")
    for spec in LAYERS:
        for dtype in (torch.float32, torch.float16):
            layer(*spec, dtype=dtype, reps=reps)
    print("\n## The chain 1x1 96 -> 96, 7x7 depthwise, channels-first LayerNorm, 1x1 96 -> 384 @80x120, threshold 0.05\n")
    print("| dtype | changed input pixels per frame | CBChannelReduce2d, replayed by FrameProgram | CBChannelReduce2d, eager "
          "| torch's dense LayerNorm |")
    print("|---|---|---|---|---|")
    for dtype in (torch.float32, torch.float16):
        chain(dtype, reps)


if __name__ == "__main__":
    main()
