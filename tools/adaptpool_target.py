#!/usr/bin/env python3
"""Target of the change-based adaptive pool (cb_adaptpool.hip): four layers at 10 % changed input pixels per frame (whole
blocks of pixels), fp32 --
  classifier head  960 ch   15x20  -> 1   avg
  SE squeeze        96 ch   60x80  -> 1   avg
  PSP bin          512 ch   60x80  -> 6   avg
  wide early map    64 ch  320x480 -> 1   avg and max
Per layer: the frame of cbinfer_cbadaptivepool2d_forward fed the change MASK (two launches) and fed the change LIST (three
launches), and torch's dense F.adaptive_avg_pool2d / F.adaptive_max_pool2d on the same tensor.  Before timing, an
every-pixel frame is checked: max against CPU torch bit for bit, avg within 1e-5 relative of it (the summation order is
the library's own).  The measuring method is tools/target_common.py's: one warm-up batch per run in front of the rounds.
(This tool used to warm up with one extra call in front of every timed batch instead; tables recorded that way say so.)
Prints markdown (profiles/adaptive_pool_target.md).
usage: adaptpool_target.py [rounds]"""
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

#          name, channels, H, W, output size, op, block
LAYERS = [("classifier head 960 ch avg", 960, 15, 20, 1, "avg", 2),
          ("SE squeeze 96 ch avg", 96, 60, 80, 1, "avg", 8),
          ("PSP bin 512 ch avg", 512, 60, 80, 6, "avg", 8),
          ("wide early map 64 ch avg", 64, 320, 480, 1, "avg", 32),
          ("wide early map 64 ch max", 64, 320, 480, 1, "max", 32)]


def layer(name, Cn, H, W, o, op, block, reps):
    rng = np.random.default_rng(7)
    code = _lib.ADAPT_MAX if op == "max" else _lib.ADAPT_AVG
    x = torch.rand(1, Cn, H, W, device="cuda")
    sets = change_sets(rng, H, W, block, 0.10)
    masks, lists = device_sets(sets)
    P = torch.empty(C.cbinfer_adaptive_pool_partial_elems(Cn, H, W, o, o), device="cuda")
    inBits = torch.zeros(C.cbinfer_mask_words(H, W), dtype=torch.int64, device="cuda")
    outBits = torch.zeros(C.cbinfer_mask_words(o, o), dtype=torch.int64, device="cuda")
    copy = torch.zeros_like(outBits)
    out = torch.empty((1, Cn, o, o), device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def frame(mask, lst):
        check(C.cbinfer_cbadaptivepool2d_forward(ptr(x), ptr(P), ptr(out), ptr(mask), ptr(lst),
                                                 lst.numel() if lst is not None else 0, None, ptr(inBits), ptr(outBits),
                                                 ptr(copy), Cn, H, W, o, o, code, _lib.CB_F32, st))

    def dense(i):
        return F.adaptive_max_pool2d(x, o) if op == "max" else F.adaptive_avg_pool2d(x, o)

    def cb_list(i):
        frame(None, lists[i % SETS])

    def cb_mask(i):
        frame(masks[i % SETS], None)

    # results first: an every-pixel frame against CPU torch
    frame(None, None)
    xc = x.cpu()
    if op == "max":
        assert torch.equal(out.cpu(), F.adaptive_max_pool2d(xc, o)), "change-based frame differs from the dense operator"
    else:
        assert torch.allclose(out.cpu(), F.adaptive_avg_pool2d(xc, o), rtol=1e-5, atol=0), "average beyond 1e-5"
    t = rounds([("list", cb_list), ("mask", cb_mask), ("dense", dense)], reps)
    # the state after all those frames is still the every-pixel frame's (the input never changed)
    first = out.clone()
    frame(None, None)
    assert torch.equal(out, first)
    listed = listed_share(sets)
    dl = statistics.median(t["dense"]) / statistics.median(t["list"])
    dm = statistics.median(t["dense"]) / statistics.median(t["mask"])
    print("| %s @%dx%d -> %dx%d | %.1f %% | %s | %s | %s | %.2fx / %.2fx |"
          % (name, H, W, o, o, listed, fmt(t["list"]), fmt(t["mask"]), fmt(t["dense"]), dl, dm))


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    assert torch.cuda.is_available(), "adaptpool_target.py needs a GPU"
    print("# Change-based adaptive pooling at 10 % changed input pixels (fp32)\n")
    print("%s, torch %s; times in us per call, median [min..max] over %d interleaved rounds of %d calls\n"
          % (torch.cuda.get_device_name(0), torch.__version__, reps, BATCH))
    print("| layer | changed input pixels | cbinfer_cbadaptivepool2d_forward, list form | "
          "cbinfer_cbadaptivepool2d_forward, mask form | dense torch operator | dense / list form, dense / mask form |")
    print("|---|---|---|---|---|---|")
    for spec in LAYERS:
        layer(*spec, reps=reps)


if __name__ == "__main__":
    main()
