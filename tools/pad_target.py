#!/usr/bin/env python3
"""Target of the change-based padding (cb_pad.hip): fp32 and fp16, 10 % changed input pixels per frame in whole 8x8
blocks --
  a monodepth2-type decoder layer   64 ch and 256 ch @96x320, ReflectionPad2d(1),
  a style-transfer stem             3 ch @320x480, ReflectionPad2d(3),
  a restoration layer               64 ch @180x320, ReplicationPad2d(1),
  a TF-ported stride-2 layer        32 ch @160x240, ZeroPad2d((0, 1, 0, 1)).
Table 1, per case and dtype: cbinfer_cbpad_forward with the input in MASK form (one launch) and in LIST form (one more
launch in front) against torch's dense F.pad on the same device tensor.
Table 2, the chain 3x3 conv 64 -> 64 + ReLU -> ReflectionPad2d(1) -> valid 3x3 conv 64 -> 64 @96x320, threshold 0.05,
frame time of: the chain with CBPad2d replayed by FrameProgram, the same run eagerly, and the same converted layers with
torch's dense pad in the middle (the layer behind it then runs its own detection on the padded map).
The measuring method is tools/target_common.py's.  Prints markdown (profiles/pad_target.md).
usage: pad_target.py [rounds]"""
import copy
import ctypes
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

#         name, channels, H, W, mode, (left, right, top, bottom)
CASES = [("monodepth2-type layer", 64, 96, 320, "reflect", (1, 1, 1, 1)),
         ("monodepth2-type layer", 256, 96, 320, "reflect", (1, 1, 1, 1)),
         ("style-transfer stem", 3, 320, 480, "reflect", (3, 3, 3, 3)),
         ("restoration layer", 64, 180, 320, "replicate", (1, 1, 1, 1)),
         ("TF-ported stride-2 layer", 32, 160, 240, "constant", (0, 1, 0, 1))]
MODES = {"constant": _lib.PAD_CONSTANT, "reflect": _lib.PAD_REFLECT, "replicate": _lib.PAD_REPLICATE,
         "circular": _lib.PAD_CIRCULAR}
BLOCK = 8


def case(name, Cn, H, W, mode, pads, tdt, reps):
    rng = np.random.default_rng(7)
    x = torch.randn(1, Cn, H, W, device="cuda").to(tdt)
    sets = change_sets(rng, H, W, BLOCK, 0.10)
    masks, lists = device_sets(sets)
    left, right, top, bottom = pads
    Ho, Wo = H + top + bottom, W + left + right
    p = ctypes.pointer(_lib.Pad(MODES[mode], left, right, top, bottom, 0.0))
    assert C.cbinfer_pad_supported(p, H, W)
    words = C.cbinfer_mask_words(Ho, Wo)
    out = torch.empty(1, Cn, Ho, Wo, device="cuda", dtype=tdt)
    bits = torch.zeros(words, dtype=torch.int64, device="cuda")
    mcopy = torch.zeros(words, dtype=torch.int64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    dt = _lib.dtype_code(x)

    def run(i, form):
        m = masks[i % SETS] if form == "mask" else None
        l = lists[i % SETS] if form == "list" else None
        check(C.cbinfer_cbpad_forward(ptr(x), ptr(out), ptr(m), ptr(l), l.numel() if l is not None else 0, None, ptr(bits),
                                      ptr(mcopy), Cn, H, W, p, dt, st))

    def dense(i):
        return F.pad(x, pads, mode=mode)

    # results first: with every pixel listed the frame is torch's operator bit for bit
    run(0, "all")
    assert torch.equal(out, dense(0)), "the padded map differs from F.pad"
    t = rounds([("mask", lambda i: run(i, "mask")), ("list", lambda i: run(i, "list")), ("dense", dense)], reps)
    med = {k: statistics.median(v) for k, v in t.items()}
    listed = listed_share(sets)
    print("| %s, %d ch @%dx%d %s %s | %s | %.1f %% | %s | %s | %s | %.2fx / %.2fx |"
          % (name, Cn, H, W, mode, pads, dtype_name(tdt), listed, fmt(t["mask"]), fmt(t["list"]), fmt(t["dense"]),
             med["dense"] / med["mask"], med["dense"] / med["list"]))


def chain(tdt, reps):
    H, W, Cn = 96, 320, 64
    rng = np.random.default_rng(11)
    torch.manual_seed(11)
    src = nn.Sequential(nn.Conv2d(Cn, Cn, 3, padding=1), nn.ReLU(), nn.ReflectionPad2d(1), nn.Conv2d(Cn, Cn, 3))
    src = src.eval().cuda().to(tdt)
    sets = change_sets(rng, H, W, BLOCK, 0.05)
    frames = moving_frames(torch.rand(1, Cn, H, W, device="cuda").to(tdt), sets, Cn, tdt)

    def converted(padding):
        net = pycbinfer.convert(copy.deepcopy(src), threshold=0.05, generalGeometry=True)
        if padding:
            pycbinfer.insertCBPadding(net, cloneOutput=False)
        return net

    netP, netE, netT = converted(True), converted(True), converted(False)
    assert [type(m).__name__ for m in netP] == ['CBConv2d', 'CBPad2d', 'CBConv2d']
    assert [type(m).__name__ for m in netT] == ['CBConv2d', 'ReflectionPad2d', 'CBConv2d']
    prog = pycbinfer.FrameProgram(netP)

    def replayed(i):
        return prog(frames[i % SETS])

    def eager(i):
        return netE(frames[i % SETS])

    def torch_pad(i):
        return netT(frames[i % SETS])

    with torch.no_grad():
        for i in range(2 * SETS):      # steady state before the frame is recorded; the same history for all three
            netP(frames[i % SETS])
            eager(i)
            torch_pad(i)
        # results first: replay and eager agree bit for bit; the dense-pad chain within the thresholds' reach
        for i in range(SETS):
            yp, ye, yt = replayed(i), eager(i), torch_pad(i)
            assert torch.equal(yp, ye), "the replayed program differs from the eager chain"
            assert float((ye.float() - yt.float()).abs().max()) < 1.0, "the chain differs from the one with torch's pad"
        t = rounds([("replayed", replayed), ("eager", eager), ("torch", torch_pad)], reps)
    changed = listed_share([m | sets[i - 1] for i, m in enumerate(sets)])
    print("| %s | %.1f %% | %s | %s | %s |" % (dtype_name(tdt), changed, fmt(t["replayed"]), fmt(t["eager"]),
                                              fmt(t["torch"])))


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    assert torch.cuda.is_available(), "pad_target.py needs a GPU"
    print("# Change-based padding at 10 % changed input pixels\n")
    print("%s, torch %s; times in us per call, median [min..max] over %d interleaved rounds of %d calls; the dense operator "
          "is F.pad on the same device tensor\n" % (torch.cuda.get_device_name(0), torch.__version__, reps, BATCH))
    print("| case | dtype | changed input pixels | cbinfer_cbpad_forward, mask form | cbinfer_cbpad_forward, list form "
          "| dense torch operator | dense / mask form, dense / list form |")
    print("|---|---|---|---|---|---|---|")
    for spec in CASES:
        for tdt in (torch.float32, torch.float16):
            case(*spec, tdt=tdt, reps=reps)
            sys.stdout.flush()
    print("\n## The chain 3x3 64 -> 64 + ReLU, ReflectionPad2d(1), valid 3x3 64 -> 64 @96x320, threshold 0.05\n")
    print("| dtype | changed input pixels per frame | CBPad2d, replayed by FrameProgram | CBPad2d, eager "
          "| torch's dense ReflectionPad2d |")
    print("|---|---|---|---|---|")
    for tdt in (torch.float32, torch.float16):
        chain(tdt, reps)
        sys.stdout.flush()


if __name__ == "__main__":
    main()
