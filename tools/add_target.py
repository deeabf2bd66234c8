#!/usr/bin/env python3
"""Target of the change-based residual add (cb_add.hip): fp32, 10 % changed pixels per frame in whole blocks (32x32 frame
pixels of a 320x480 frame, i.e. 8 / 4 / 2 pixels at the three resolutions) --
  64 ch @ 80x120,  128 ch @ 40x60,  256 ch @ 20x30.
Table 1, per layer: cbinfer_cbadd_forward with both operands in MASK form (one launch) and both in LIST form (three
launches) -- both operands carry the frame's change set --, against the dense torch.relu(a + b) on the same tensors.
Table 2, one 64-channel basic block (two 3x3 layers + add) at 80x120, frame time of: CBResidual replayed by FrameProgram,
CBResidual run eagerly, and the same two CBConv2d layers followed by torch's add + relu.  The block's input arrives with
its change mask, as behind a producing layer: a frame differs from the one before in two change sets of 5 % each, and the
mask (160 words) is copied into the block's static mask buffer before every frame, in all three configurations alike.
The measuring method is tools/target_common.py's.  Prints markdown (profiles/add_target.md).
usage: add_target.py [rounds]"""
import copy
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pycbinfer  # noqa: E402
from cbinfer_amd import _lib  # noqa: E402
from cbinfer_amd._lib import C, check, ptr  # noqa: E402
from cbinfer_amd.conv2d_cg import MaskChangeIndexes  # noqa: E402
from target_common import BATCH, SETS, change_sets, device_sets, fmt, listed_share, moving_frames, pack, rounds  # noqa: E402

#          name, channels, H, W, block
LAYERS = [("64 ch", 64, 80, 120, 8), ("128 ch", 128, 40, 60, 4), ("256 ch", 256, 20, 30, 2)]


def layer(name, Cn, H, W, block, reps):
    rng = np.random.default_rng(7)
    a = torch.randn(1, Cn, H, W, device="cuda")
    b = torch.randn(1, Cn, H, W, device="cuda")
    sets = change_sets(rng, H, W, block, 0.10)
    masks, lists = device_sets(sets)
    words = C.cbinfer_mask_words(H, W)
    bits = torch.zeros(words, dtype=torch.int64, device="cuda")
    mcopy = torch.zeros(words, dtype=torch.int64, device="cuda")
    out = torch.empty_like(a)
    st = torch.cuda.current_stream().cuda_stream

    def dense(i):
        return torch.relu(a + b)

    def cb_mask(i):
        m = masks[i % SETS]
        check(C.cbinfer_cbadd_forward(ptr(a), ptr(b), ptr(out), ptr(m), None, 0, None, ptr(m), None, 0, None, ptr(bits),
                                      ptr(mcopy), Cn, H, W, 1, _lib.CB_F32, st))

    def cb_list(i):
        lst = lists[i % SETS]
        check(C.cbinfer_cbadd_forward(ptr(a), ptr(b), ptr(out), None, ptr(lst), lst.numel(), None, None, ptr(lst),
                                      lst.numel(), None, ptr(bits), ptr(mcopy), Cn, H, W, 1, _lib.CB_F32, st))

    # results first: with every pixel listed the frame must equal torch's operators bit for bit
    check(C.cbinfer_cbadd_forward(ptr(a), ptr(b), ptr(out), None, None, 0, None, None, None, 0, None, ptr(bits), ptr(mcopy),
                                  Cn, H, W, 1, _lib.CB_F32, st))
    assert torch.equal(out, torch.relu(a + b)), "change-based frame differs from the dense operators"
    t = rounds([("mask", cb_mask), ("list", cb_list), ("dense", dense)], reps)
    listed = listed_share(sets)
    dm = statistics.median(t["dense"]) / statistics.median(t["mask"])
    dl = statistics.median(t["dense"]) / statistics.median(t["list"])
    print("| %s @%dx%d | %.1f %% | %s | %s | %s | %.2fx / %.2fx |"
          % (name, H, W, listed, fmt(t["mask"]), fmt(t["list"]), fmt(t["dense"]), dm, dl))


def block(reps):
    Cn, H, W, blk = 64, 80, 120, 8
    rng = np.random.default_rng(11)
    torch.manual_seed(11)
    body = nn.Sequential(nn.Conv2d(Cn, Cn, 3, padding=1), nn.ReLU(), nn.Conv2d(Cn, Cn, 3, padding=1)).eval().cuda()
    sets = change_sets(rng, H, W, blk, 0.05)
    frames = moving_frames(torch.rand(1, Cn, H, W, device="cuda"), sets, Cn, torch.float32)
    masks = [torch.from_numpy(pack(m | sets[i - 1])).cuda() for i, m in enumerate(sets)]
    words = C.cbinfer_mask_words(H, W)

    def incoming():
        return dict(mask=torch.zeros(words, dtype=torch.int64, device="cuda"),
                    idx=torch.empty(H * W, dtype=torch.int32, device="cuda"),
                    count=torch.zeros(1, dtype=torch.int32, device="cuda"))

    def residual():
        res = pycbinfer.CBResidual(pycbinfer.convert(copy.deepcopy(body), threshold=0.05))
        res.add.cloneOutput = False
        return res

    resP, resE, inP, inE, inT = residual(), residual(), incoming(), incoming(), incoming()
    plain = pycbinfer.convert(copy.deepcopy(body), threshold=0.05)

    def tupled(res, buf):
        return lambda f: res(('changeIndexes', f, MaskChangeIndexes(buf['mask'], (H, W), buf['idx'], buf['count'])))

    eagerFn = tupled(resE, inE)
    prog = pycbinfer.FrameProgram(tupled(resP, inP))

    def replayed(i):
        inP['mask'].copy_(masks[i % SETS])
        return prog(frames[i % SETS])

    def eager(i):
        inE['mask'].copy_(masks[i % SETS])
        return eagerFn(frames[i % SETS])

    def torch_add(i):
        inT['mask'].copy_(masks[i % SETS])      # (not used: the same copy as in the other two)
        x = frames[i % SETS]
        return torch.relu(plain(x) + x)

    with torch.no_grad():
        for i in range(2 * SETS):      # steady state before the frame is recorded; the same history for all three
            inP['mask'].copy_(masks[i % SETS])
            tupled(resP, inP)(frames[i % SETS])
            eager(i)
            torch_add(i)
        # results first: the three configurations compute the same block, bit for bit
        for i in range(SETS):
            yp, ye, yt = replayed(i), eager(i), torch_add(i)
            assert torch.equal(ye, yt), "CBResidual differs from the layers with torch's add + relu"
            assert torch.equal(yp, ye), "the replayed program differs from the eager block"
        t = rounds([("replayed", replayed), ("eager", eager), ("torch", torch_add)], reps)
    changed = listed_share([m | sets[i - 1] for i, m in enumerate(sets)])
    print("\n## One basic block: two 3x3 64 -> 64 layers + add + ReLU @%dx%d, %.1f %% changed input pixels per frame\n"
          % (H, W, changed))
    print("| configuration | frame time |")
    print("|---|---|")
    print("| CBResidual replayed by FrameProgram | %s |" % fmt(t["replayed"]))
    print("| CBResidual run eagerly | %s |" % fmt(t["eager"]))
    print("| the two CBConv2d layers, then torch add + relu | %s |" % fmt(t["torch"]))


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    assert torch.cuda.is_available(), "add_target.py needs a GPU"
    print("# Change-based residual add at 10 % changed pixels (fp32)\n")
    print("%s, torch %s; times in us per call, median [min..max] over %d interleaved rounds of %d calls\n"
          % (torch.cuda.get_device_name(0), torch.__version__, reps, BATCH))
    print("| layer | changed pixels | cbinfer_cbadd_forward, mask form | cbinfer_cbadd_forward, list form "
          "| dense torch.relu(a + b) | dense / mask form, dense / list form |")
    print("|---|---|---|---|---|---|")
    for spec in LAYERS:
        layer(*spec, reps=reps)
    block(reps)


if __name__ == "__main__":
    main()
