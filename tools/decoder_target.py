#!/usr/bin/env python3
"""Target of the change-based decoder operators (cb_decoder.hip): fp32, 10 % changed INPUT pixels per frame in whole
blocks (32x32 frame pixels of a 320x480 frame, i.e. 4 / 2 pixels at the two input resolutions) --
  64 ch @ 80x120 -> 160x240,  128 ch @ 40x60 -> 80x120.
Table 1, per layer: cbinfer_cbupsample_forward (nearest x2, bilinear x2 with align_corners=False) with the input in MASK
form (one launch), against the dense F.interpolate on the same tensor; and cbinfer_cbconcat_forward of two operands of
that many channels at the OUTPUT resolution, both in mask form carrying the upsampled footprint (one launch), against
the dense torch.cat.
Table 2, one decoder stage at 64 ch: upsample x2 (nearest) of a 64-channel 80x120 map -> concat with a 64-channel
160x240 skip -> 1x1 convolution 128 -> 64, frame time of: the three change-based modules replayed by FrameProgram, the
same run eagerly, and the same CBConv2d behind F.interpolate + torch.cat.  Both inputs of the stage arrive with their
change masks, as behind producing layers: a frame differs from the one before in two change sets of 5 % each; the masks
are copied into static mask buffers before every frame, in all three configurations alike.
The measuring method is tools/target_common.py's.  Prints markdown (profiles/decoder_target.md).
usage: decoder_target.py [rounds]"""
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
from cbinfer_amd.conv2d_cg import MaskChangeIndexes  # noqa: E402
from target_common import BATCH, SETS, change_sets, fmt, listed_share, moving_frames, pack, rounds  # noqa: E402

#          name, channels, Hi, Wi, block (input pixels)
LAYERS = [("64 ch", 64, 80, 120, 4), ("128 ch", 128, 40, 60, 2)]


def layer(name, Cn, Hi, Wi, block, reps):
    rng = np.random.default_rng(7)
    Ho, Wo = 2 * Hi, 2 * Wi
    x = torch.randn(1, Cn, Hi, Wi, device="cuda")
    skip = torch.randn(1, Cn, Ho, Wo, device="cuda")
    sets = change_sets(rng, Hi, Wi, block, 0.10)
    inMasks = [torch.from_numpy(pack(m)).cuda() for m in sets]
    outMasks = [torch.from_numpy(pack(np.kron(m, np.ones((2, 2), dtype=bool)))).cuda() for m in sets]
    words = C.cbinfer_mask_words(Ho, Wo)
    st = torch.cuda.current_stream().cuda_stream

    def buffers(n=1):
        return (torch.zeros(n * words, dtype=torch.int64, device="cuda"), torch.zeros(words, dtype=torch.int64, device="cuda"))

    structs = {"nearest": ctypes.pointer(_lib.Upsample(2, 2, _lib.UPSAMPLE_NEAREST, 0)),
               "bilinear": ctypes.pointer(_lib.Upsample(2, 2, _lib.UPSAMPLE_BILINEAR, 0))}
    outs = {k: torch.empty(1, Cn, Ho, Wo, device="cuda") for k in structs}
    work = {k: buffers() for k in structs}

    def cb_up(kind):
        def run(i, mask=True):
            check(C.cbinfer_cbupsample_forward(ptr(x), ptr(outs[kind]), ptr(inMasks[i % SETS]) if mask else None, None, 0,
                                               None, ptr(work[kind][0]), ptr(work[kind][1]), Cn, Hi, Wi, structs[kind],
                                               _lib.CB_F32, st))
        return run

    def dense_up(kind):
        kw = dict(mode="nearest") if kind == "nearest" else dict(mode="bilinear", align_corners=False)
        return lambda i: F.interpolate(x, scale_factor=2, **kw)

    catOut = torch.empty(1, 2 * Cn, Ho, Wo, device="cuda")
    catBits, catCopy = buffers(2)
    srcs = (ctypes.c_void_p * 2)(ptr(outs["nearest"]), ptr(skip))
    chans = (ctypes.c_int32 * 2)(Cn, Cn)
    none = (ctypes.c_void_p * 2)()
    caps = (ctypes.c_int32 * 2)()
    maskArrays = [(ctypes.c_void_p * 2)(ptr(m), ptr(m)) for m in outMasks]

    def cb_cat(i, mask=True):
        check(C.cbinfer_cbconcat_forward(srcs, chans, 2, ptr(catOut), maskArrays[i % SETS] if mask else none, none, caps,
                                         none, ptr(catBits), ptr(catCopy), Ho, Wo, _lib.CB_F32, st))

    def dense_cat(i):
        return torch.cat([outs["nearest"], skip], 1)

    # results first: with every pixel listed nearest and concat must equal torch's operators bit for bit, bilinear within
    # the float32 bar of DESIGN 5.13 (8 2^-24 max |corner| <= 8 2^-24 max |x|)
    cb_up("nearest")(0, mask=False)
    cb_up("bilinear")(0, mask=False)
    cb_cat(0, mask=False)
    assert torch.equal(outs["nearest"], dense_up("nearest")(0)), "nearest differs from F.interpolate"
    assert torch.equal(catOut, dense_cat(0)), "concat differs from torch.cat"
    dev = float((outs["bilinear"].double() - F.interpolate(x.double(), scale_factor=2, mode="bilinear",
                                                           align_corners=False)).abs().max())
    assert dev <= 8 * 2.0 ** -24 * float(x.abs().max()), "bilinear is off the float64 operator by %g" % dev
    t = rounds([("near", cb_up("nearest")), ("dnear", dense_up("nearest")), ("bil", cb_up("bilinear")),
                ("dbil", dense_up("bilinear")), ("cat", cb_cat), ("dcat", dense_cat)], reps)
    listed = listed_share(sets)
    for label, a, b, shape in (("upsample nearest x2", "near", "dnear", "%dx%d -> %dx%d" % (Hi, Wi, Ho, Wo)),
                               ("upsample bilinear x2", "bil", "dbil", "%dx%d -> %dx%d" % (Hi, Wi, Ho, Wo)),
                               ("concat, two operands", "cat", "dcat", "2 x %d ch @%dx%d" % (Cn, Ho, Wo))):
        print("| %s, %s | %s | %.1f %% | %s | %s | %.2fx |"
              % (label, name, shape, listed, fmt(t[a]), fmt(t[b]), statistics.median(t[b]) / statistics.median(t[a])))


class Stage(nn.Module):
    def __init__(self, up, cat, conv, cb):
        super(Stage, self).__init__()
        self.up, self.cat, self.conv, self.cb = up, cat, conv, cb

    def forward(self, pair):
        low, skip = pair
        if self.cb:
            return self.conv(self.cat([self.up(low), skip]))
        return self.conv(torch.cat([F.interpolate(low[1], scale_factor=2, mode="nearest"), skip[1]], 1))


def stage(reps):
    Cn, Hi, Wi, blk = 64, 80, 120, 4
    Ho, Wo = 2 * Hi, 2 * Wi
    rng = np.random.default_rng(11)
    torch.manual_seed(11)
    conv = nn.Sequential(nn.Conv2d(2 * Cn, Cn, 1)).eval().cuda()
    lowSets = change_sets(rng, Hi, Wi, blk, 0.05)
    skipSets = change_sets(rng, Ho, Wo, 2 * blk, 0.05)
    lowBase, skipBase = torch.rand(1, Cn, Hi, Wi, device="cuda"), torch.rand(1, Cn, Ho, Wo, device="cuda")

    def frames_of(base, sets):
        return (moving_frames(base, sets, Cn, torch.float32),
                [torch.from_numpy(pack(m | sets[i - 1])).cuda() for i, m in enumerate(sets)])
    lowFrames, lowMasks = frames_of(lowBase, lowSets)
    skipFrames, skipMasks = frames_of(skipBase, skipSets)

    def incoming(H, W):
        return dict(mask=torch.zeros(C.cbinfer_mask_words(H, W), dtype=torch.int64, device="cuda"), size=(H, W),
                    idx=torch.empty(H * W, dtype=torch.int32, device="cuda"),
                    count=torch.zeros(1, dtype=torch.int32, device="cuda"),
                    frame=torch.empty(1, Cn, H, W, device="cuda"))

    def build(cb):
        up = pycbinfer.CBUpsample2d(nn.Upsample(scale_factor=2, mode="nearest"))
        cat = pycbinfer.CBConcat2d()
        up.propChangeIndexes, up.cloneOutput, cat.cloneOutput = True, False, False
        net = Stage(up, cat, pycbinfer.convert(copy.deepcopy(conv), threshold=0.05)[0], cb)
        ins = (incoming(Hi, Wi), incoming(Ho, Wo))

        def tupled(frame):
            # (the low-resolution frame is the recorded frame: its address is patched; the skip lives in a static buffer)
            lo, sk = ins
            return net((('changeIndexes', frame, MaskChangeIndexes(lo['mask'], lo['size'], lo['idx'], lo['count'])),
                        ('changeIndexes', sk['frame'], MaskChangeIndexes(sk['mask'], sk['size'], sk['idx'], sk['count']))))

        def feed(i):
            ins[0]['mask'].copy_(lowMasks[i % SETS])
            ins[1]['mask'].copy_(skipMasks[i % SETS])
            ins[1]['frame'].copy_(skipFrames[i % SETS])
        return net, tupled, feed

    netP, runP, feedP = build(True)
    netE, runE, feedE = build(True)
    netT, runT, feedT = build(False)
    prog = pycbinfer.FrameProgram(runP)

    def replayed(i):
        feedP(i)
        return prog(lowFrames[i % SETS])

    def eager(i):
        feedE(i)
        return runE(lowFrames[i % SETS])

    def torch_ops(i):
        feedT(i)
        return runT(lowFrames[i % SETS])

    with torch.no_grad():
        for i in range(2 * SETS):      # steady state before the frame is recorded; the same history for all three
            feedP(i)
            runP(lowFrames[i % SETS])
            eager(i)
            torch_ops(i)
        # results first: the three configurations compute the same stage, bit for bit
        for i in range(SETS):
            yp, ye, yt = replayed(i), eager(i), torch_ops(i)
            assert torch.equal(ye, yt), "the change-based stage differs from the layers with torch operators in between"
            assert torch.equal(yp, ye), "the replayed program differs from the eager stage"
        t = rounds([("replayed", replayed), ("eager", eager), ("torch", torch_ops)], reps)
    print("\n## One decoder stage: upsample x2 (nearest) 64 ch @%dx%d -> concat with a 64 ch skip @%dx%d -> 1x1 conv 128 -> 64,"
          " 10 %% changed pixels per frame in both inputs\n" % (Hi, Wi, Ho, Wo))
    print("| configuration | frame time |")
    print("|---|---|")
    print("| CBUpsample2d, CBConcat2d, CBConv2d replayed by FrameProgram | %s |" % fmt(t["replayed"]))
    print("| CBUpsample2d, CBConcat2d, CBConv2d run eagerly | %s |" % fmt(t["eager"]))
    print("| F.interpolate, torch.cat, then the CBConv2d | %s |" % fmt(t["torch"]))
    print("\n(every configuration also copies the two change masks and the skip frame into static buffers per frame)")


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    assert torch.cuda.is_available(), "decoder_target.py needs a GPU"
    print("# Change-based upsampling and concat at 10 % changed pixels (fp32)\n")
    print("%s, torch %s; times in us per call, median [min..max] over %d interleaved rounds of %d calls\n"
          % (torch.cuda.get_device_name(0), torch.__version__, reps, BATCH))
    print("| operator | shape | changed input pixels | change-based, mask form | dense torch operator | dense / change-based |")
    print("|---|---|---|---|---|---|")
    for spec in LAYERS:
        layer(*spec, reps=reps)
    stage(reps)


if __name__ == "__main__":
    main()
