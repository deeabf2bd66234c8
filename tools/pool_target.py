#!/usr/bin/env python3
"""Target of change-based pooling for any window (cb_pool2d.hip): three layers at 10 % changed input pixels per frame
(whole blocks of 32x32 frame pixels, i.e. 16 / 32 / 4 pixels at the three resolutions), fp32 --
  stem pool    64 ch  160x240  3x3 stride 2 pad 1 max
  ceil pool    16 ch  320x480  3x3 stride 2 ceil_mode max
  transition  256 ch   40x60   2x2 average
Per layer: the frame of cbinfer_cbpool2d_forward (both launches) fed the change LIST and fed the change MASK, torch's
dense F.max_pool2d / F.avg_pool2d on the same tensor, and, for a 2x2/stride-2 window, the existing cbinfer_max_pool2d
launch on the same list (it computes the maximum, not the average: the window is what is compared).
The measuring method is tools/target_common.py's: one warm-up batch per run in front of the rounds.  (This tool used to
warm up with one extra call in front of every timed batch instead; tables recorded that way say so.)
Prints markdown (profiles/pool_target.md).
usage: pool_target.py [rounds]"""
import ctypes
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pycbinfer  # noqa: E402,F401
from cbinfer_amd import _lib  # noqa: E402
from cbinfer_amd._lib import C, check, ptr  # noqa: E402
from target_common import BATCH, SETS, change_sets, device_sets, fmt, listed_share, rounds  # noqa: E402

#          name, channels, H, W, window, stride, padding, ceil, op, block
LAYERS = [("stem pool 64 ch 3x3 s2 p1 max", 64, 160, 240, 3, 2, 1, False, "max", 16),
          ("ceil pool 16 ch 3x3 s2 ceil max", 16, 320, 480, 3, 2, 0, True, "max", 32),
          ("transition 256 ch 2x2 avg", 256, 40, 60, 2, 2, 0, False, "avg", 4)]


def layer(name, Cn, H, W, k, s, p, ceil, op, block, reps):
    rng = np.random.default_rng(7)
    g = _lib.Pool(k, k, s, s, p, p, int(ceil), _lib.POOL_MAX if op == "max" else _lib.POOL_AVG_PAD)
    gp = ctypes.pointer(g)
    ho, wo = ctypes.c_int(), ctypes.c_int()
    check(C.cbinfer_pool_out_size(H, W, gp, ctypes.byref(ho), ctypes.byref(wo)))
    Ho, Wo = ho.value, wo.value
    x = torch.rand(1, Cn, H, W, device="cuda")
    sets = change_sets(rng, H, W, block, 0.10)
    masks, lists = device_sets(sets)
    words = C.cbinfer_mask_words(Ho, Wo)
    bits = torch.zeros(words, dtype=torch.int64, device="cuda")
    copy = torch.zeros(words, dtype=torch.int64, device="cuda")
    out = torch.full((1, Cn, Ho, Wo), float('inf'), device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def dense(i):
        if op == "max":
            return F.max_pool2d(x, k, s, p, ceil_mode=ceil)
        return F.avg_pool2d(x, k, s, p, ceil_mode=ceil)

    def cb_list(i):
        lst = lists[i % SETS]
        check(C.cbinfer_cbpool2d_forward(ptr(x), ptr(out), ptr(lst), lst.numel(), None, None, ptr(bits), ptr(copy), Cn,
                                         H, W, gp, _lib.CB_F32, st))

    def cb_mask(i):
        check(C.cbinfer_cbpool2d_forward(ptr(x), ptr(out), None, 0, None, ptr(masks[i % SETS]), ptr(bits), ptr(copy),
                                         Cn, H, W, gp, _lib.CB_F32, st))

    def old_2x2(i):
        lst = lists[i % SETS]
        check(C.cbinfer_max_pool2d(ptr(x), ptr(out2), ptr(lst), lst.numel(), None, Cn, H, W, Ho, Wo, _lib.CB_F32, st))

    # results first: with every pixel listed the frame must equal torch's CPU operator bit for bit
    every = torch.arange(H * W, dtype=torch.int32, device="cuda")
    check(C.cbinfer_cbpool2d_forward(ptr(x), ptr(out), ptr(every), H * W, None, None, ptr(bits), ptr(copy), Cn, H, W, gp,
                                     _lib.CB_F32, st))
    xc = x.cpu()
    ref = F.max_pool2d(xc, k, s, p, ceil_mode=ceil) if op == "max" else F.avg_pool2d(xc, k, s, p, ceil_mode=ceil)
    assert torch.equal(out.cpu(), ref), "change-based frame differs from the dense operator"
    runs = [("list", cb_list), ("mask", cb_mask), ("dense", dense)]
    if (k, s, p) == (2, 2, 0):
        out2 = torch.full((1, Cn, Ho, Wo), float('inf'), device="cuda")
        runs.append(("old", old_2x2))
    t = rounds(runs, reps)
    listed = listed_share(sets)
    dl = statistics.median(t["dense"]) / statistics.median(t["list"])
    dm = statistics.median(t["dense"]) / statistics.median(t["mask"])
    print("| %s @%dx%d -> %dx%d | %.1f %% | %s | %s | %s | %.2fx / %.2fx | %s |"
          % (name, H, W, Ho, Wo, listed, fmt(t["list"]), fmt(t["mask"]), fmt(t["dense"]), dl, dm,
             fmt(t["old"]) if "old" in t else "-"))


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    assert torch.cuda.is_available(), "pool_target.py needs a GPU"
    print("# Change-based pooling for any window at 10 % changed input pixels (fp32)\n")
    print("%s, torch %s; times in us per call, median [min..max] over %d interleaved rounds of %d calls\n"
          % (torch.cuda.get_device_name(0), torch.__version__, reps, BATCH))
    print("| layer | changed input pixels | cbinfer_cbpool2d_forward, list form | cbinfer_cbpool2d_forward, mask form "
          "| dense torch operator | dense / list form, dense / mask form | cbinfer_max_pool2d (2x2/s2 only) |")
    print("|---|---|---|---|---|---|---|")
    for spec in LAYERS:
        layer(*spec, reps=reps)


if __name__ == "__main__":
    main()
