#!/usr/bin/env python3
"""Target of the six element-wise kinds of CBPointwise2d(transcendental=True) (cb_pointwise.hip): fp32 and
fp16, 10 % changed pixels per frame in whole blocks (32x32 frame pixels of a 320x480 frame, i.e. 8 / 4 pixels at the
two resolutions) --
  64 ch @ 80x120: GELU, ELU, Mish;   128 ch @ 40x60: GELU (the expand of a ConvNeXt-type block).
Table 1, per layer, function and dtype: cbinfer_cbpointwise_forward with the operand in MASK form (one launch) and in
LIST form (two launches) against the dense torch operator on the same tensor (F.gelu, F.elu, F.mish).
Table 2, the chain of tests/test_gpu_activation.py at 80x120 with 8 -> 16 -> 32 -> 8 channels (1x1 CBConv2d -> 7x7
depthwise -> channels-first LayerNorm -> 1x1 CBConv2d -> GELU -> 1x1 CBConv2d), frame time of: the chain with the GELU as
a CBPointwise2d replayed by FrameProgram, the same run eagerly, and the same converted layers with torch's dense nn.GELU
in it (the layer behind it then runs its own change detection, and the frame cannot be recorded).
The measuring method is tools/target_common.py's.  There is no pass bar.  Prints markdown
(profiles/activation_target.md).  (The file is not called *_target.py: tests/test_host_targets.py pins the list of
those.)
usage: target_activation.py [rounds]"""
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

#          name, channels, H, W, block, functions
LAYERS = [("64 ch", 64, 80, 120, 8, ("GELU", "ELU", "Mish")), ("128 ch", 128, 40, 60, 4, ("GELU",))]
#            name -> (the nn module, the dense torch operator)
FUNCTIONS = {"GELU": (nn.GELU, F.gelu), "ELU": (nn.ELU, F.elu), "Mish": (nn.Mish, F.mish)}


class LayerNorm2d(nn.Module):
    """A channels-first layer norm as ConvNeXt implementations write it."""

    def __init__(self, Cn, eps=1e-6):
        super(LayerNorm2d, self).__init__()
        self.weight, self.bias = nn.Parameter(torch.linspace(0.5, 1.5, Cn)), nn.Parameter(torch.linspace(-0.3, 0.4, Cn))
        self.eps, self.C = eps, Cn

    def forward(self, x):
        return F.layer_norm(x.permute(0, 2, 3, 1), (self.C,), self.weight, self.bias, self.eps).permute(0, 3, 1, 2)


def layer(name, Cn, H, W, block, names, dtype, reps):
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
    for fname in names:
        m = pycbinfer.CBPointwise2d(FUNCTIONS[fname][0](), transcendental=True)
        dense_op = FUNCTIONS[fname][1]

        def call(mask, lst, m=m):
            check(C.cbinfer_cbpointwise_forward(ptr(x), ptr(out), ptr(mask), ptr(lst), lst.numel() if lst is not None else 0,
                                                None, ptr(bits), ptr(mcopy), Cn, H, W, m.kind, m.p0, m.p1, None, None, None,
                                                dt, st))

        def dense(i, dense_op=dense_op):
            return dense_op(x)

        def cb_mask(i, call=call):
            call(masks[i % SETS], None)

        def cb_list(i, call=call):
            call(None, lists[i % SETS])

        # results first: with every pixel listed the frame must agree with torch's operator on the device, which is
        # another implementation of the same function (64 ulps of |ref| + max |ref|: GELU cancels for negative inputs)
        call(None, None)
        ref = dense(0).float()
        tol = 64 * (2.0 ** -23 if dtype == torch.float32 else 2.0 ** -10)
        assert bool(((out.float() - ref).abs() <= tol * (ref.abs() + 1.0)).all()), \
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
    for name, mod in (('stem', nn.Conv2d(8, 16, 1)), ('dw', nn.Conv2d(16, 16, 7, 1, 3, groups=16)), ('norm', LayerNorm2d(16)),
                      ('pw1', nn.Conv2d(16, 32, 1)), ('gelu', nn.GELU()), ('pw2', nn.Conv2d(32, 8, 1))):
        src.add_module(name, mod)
    src = src.eval().cuda().to(dtype)
    sets = change_sets(rng, H, W, blk, 0.05)
    frames = moving_frames(torch.rand(1, 8, H, W, device="cuda").to(dtype), sets, 8, dtype)

    def converted(transcendental):
        net = pycbinfer.convert(copy.deepcopy(src), threshold=0.05, depthwise=True)
        pycbinfer.insertCBPointwise(net, transcendental=transcendental)
        pycbinfer.insertCBChannelOps(pycbinfer.linkDepthwise(net), layerNormTypes=(LayerNorm2d,))
        for m in net:
            if hasattr(m, 'cloneOutput'):
                m.cloneOutput = False
        return net

    netP, netE, netT = converted(True), converted(True), converted(False)
    assert [type(m).__name__ for m in netP] == ['CBConv2d', 'CBDepthwiseConv2d', 'CBChannelReduce2d', 'CBConv2d',
                                                'CBPointwise2d', 'CBConv2d']
    assert type(netT.gelu) is nn.GELU
    prog = pycbinfer.FrameProgram(netP)

    def replayed(i):
        return prog(frames[i % SETS])

    def eager(i):
        return netE(frames[i % SETS])

    def torch_gelu(i):
        return netT(frames[i % SETS])

    with torch.no_grad():
        for i in range(2 * SETS):      # steady state before the frame is recorded; the same history for all three
            netP(frames[i % SETS])
            eager(i)
            torch_gelu(i)
        # results first: replay and eager agree bit for bit; the dense chain within the thresholds' reach
        for i in range(SETS):
            yp, ye, yt = replayed(i), eager(i), torch_gelu(i)
            assert torch.equal(yp, ye), "the replayed program differs from the eager chain"
            assert float((ye.float() - yt.float()).abs().max()) < 1.0, "the chain differs from the one with torch's GELU"
        t = rounds([("replayed", replayed), ("eager", eager), ("torch", torch_gelu)], reps)
    changed = listed_share([m | sets[i - 1] for i, m in enumerate(sets)])
    print("| %s | %.1f %% | %s | %s | %s |" % (dtype_name(dtype), changed, fmt(t["replayed"]), fmt(t["eager"]),
                                              fmt(t["torch"])))


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    assert torch.cuda.is_available(), "target_activation.py needs a GPU"
    print("# Change-based GELU, ELU and Mish at 10 % changed pixels\n")
    print("%s, torch %s; times in us per call, median [min..max] over %d interleaved rounds of %d calls\n"
          % (torch.cuda.get_device_name(0), torch.__version__, reps, BATCH))
    print("| layer | dtype | function | changed pixels | cbinfer_cbpointwise_forward, mask form "
          "| cbinfer_cbpointwise_forward, list form | dense torch operator | dense / mask form, dense / list form |")
    print("|---|---|---|---|---|---|---|---|")
    for spec in LAYERS:
        for dtype in (torch.float32, torch.float16):
            layer(*spec, dtype=dtype, reps=reps)
    print("\n## The chain 1x1 8 -> 16, 7x7 depthwise, LayerNorm, 1x1 16 -> 32, GELU, 1x1 32 -> 8 @80x120, threshold 0.05\n")
    print("| dtype | changed input pixels per frame | GELU as CBPointwise2d, replayed by FrameProgram "
          "| GELU as CBPointwise2d, eager | torch's dense nn.GELU |")
    print("|---|---|---|---|---|")
    for dtype in (torch.float32, torch.float16):
        chain(dtype, reps)


if __name__ == "__main__":
    main()
