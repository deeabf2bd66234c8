#!/usr/bin/env python3
"""Target of change-based peak suppression and its peak list (CBPoolMax2d(suppress=...), cb_peaks.hip):
fp32 and fp16, 10 % changed pixels per frame in whole 8x8 blocks, on smooth heat-map-like maps --
  19 ch @ 368x368, 3x3 cross, floor 0.1 (the pose detector's heat maps);  80 ch @ 128x128, 3x3 window (a CenterNet-type
  head);  1 ch @ 240x320, 7x7 window (a SuperPoint-type detector).
Table 1, per map and dtype: the calls a frame of the module makes -- cbinfer_cbpeaks_forward with the operand in MASK
form (one launch) and in LIST form (two launches), each alone and followed by cbinfer_peaks_list (three more launches)
-- against torch's dense max_pool2d + compare + where on the same tensor (for the cross kind: four shifted comparisons,
pool.suppression_formula).  Table 2: what the dense path pays on top for the list, torch.nonzero of the suppressed map
with its host sync, against cbinfer_peaks_list alone, which has none.
The measuring method is tools/target_common.py's.  There is no pass bar: the lines where the module loses are printed
like the others.  Prints markdown (profiles/peaks_target.md).  (The file is not called *_target.py:
tests/test_host_targets.py pins the list of those.)
usage: target_peaks.py [rounds]"""
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
from cbinfer_amd.pool import suppression_formula  # noqa: E402
from target_common import BATCH, SETS, change_sets, device_sets, dtype_name, fmt, listed_share, rounds  # noqa: E402

#        name, channels, H, W, window, suppress, floor
MAPS = [("19 ch, 3x3 cross, floor 0.1", 19, 368, 368, 3, 'cross', 0.1),
        ("80 ch, 3x3 window", 80, 128, 128, 3, 'window', None),
        ("1 ch, 7x7 window", 1, 240, 320, 7, 'window', None)]
CAPACITY = 1 << 18


def heat_map(Cn, H, W, dtype):
    """A smooth map in 0 .. 1: noise under two 7x7 box filters, stretched per channel."""
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.rand(1, Cn, H, W, device="cuda", generator=g)
    for _ in range(2):
        x = F.avg_pool2d(x, 7, 1, 3, count_include_pad=False)
    lo, hi = x.amin((2, 3), keepdim=True), x.amax((2, 3), keepdim=True)
    return ((x - lo) / (hi - lo)).to(dtype).contiguous()


def one_map(name, Cn, H, W, k, kind, floor, dtype, reps):
    rng = np.random.default_rng(7)
    x = heat_map(Cn, H, W, dtype)
    sets = change_sets(rng, H, W, 8, 0.10)
    masks, lists = device_sets(sets)
    words = C.cbinfer_mask_words(H, W)
    bits = torch.zeros(words, dtype=torch.int64, device="cuda")
    mcopy = torch.zeros(words, dtype=torch.int64, device="cuda")
    peakBits = torch.zeros(Cn * words, dtype=torch.int64, device="cuda")
    out = torch.empty_like(x)
    work = torch.zeros(Cn * H + 1, dtype=torch.int32, device="cuda")
    entries = torch.zeros((CAPACITY, 3), dtype=torch.int32, device="cuda")
    scores = torch.zeros(CAPACITY, dtype=dtype, device="cuda")
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    start = torch.zeros(Cn + 1, dtype=torch.int32, device="cuda")
    p = _lib.Peaks(k, k, int(kind == 'cross'), int(floor is not None), floor or 0.0)
    st = torch.cuda.current_stream().cuda_stream
    dt = _lib.dtype_code(x)

    def suppress(mask, lst):
        check(C.cbinfer_cbpeaks_forward(ptr(x), ptr(out), ptr(peakBits), ptr(mask), ptr(lst),
                                        lst.numel() if lst is not None else 0, None, ptr(bits), ptr(mcopy), Cn, H, W,
                                        ctypes.byref(p), dt, st))

    def make_list(i=0):
        check(C.cbinfer_peaks_list(ptr(x), ptr(peakBits), ptr(work), ptr(entries), ptr(scores), CAPACITY, ptr(count),
                                   ptr(start), Cn, H, W, dt, st))

    def dense(i=0):
        return suppression_formula(x, k, kind, floor)

    def cb_mask(i):
        suppress(masks[i % SETS], None)

    def cb_list(i):
        suppress(None, lists[i % SETS])

    def cb_mask_peaks(i):
        suppress(masks[i % SETS], None)
        make_list()

    def cb_list_peaks(i):
        suppress(None, lists[i % SETS])
        make_list()

    def dense_nonzero(i, ref=dense()):
        return torch.nonzero(ref[0])      # (waits for the device: the size of the result is not known before)

    # results first: with every pixel listed the frame is the dense formula bit for bit, and the list torch's nonzero
    suppress(None, None)
    make_list()
    ref = dense()
    assert torch.equal(out.view(torch.int32 if dtype == torch.float32 else torch.int16),
                       ref.view(torch.int32 if dtype == torch.float32 else torch.int16)), "frame differs from the formula"
    nz = torch.nonzero(ref[0])
    n = int(count.item())
    held = min(n, CAPACITY)
    assert n == nz.size(0) and torch.equal(entries[:held].long(), nz[:held]), "list differs from torch.nonzero"
    t = rounds([("mask", cb_mask), ("list", cb_list), ("mask+peaks", cb_mask_peaks), ("list+peaks", cb_list_peaks),
                ("dense", dense), ("peaks", make_list), ("nonzero", dense_nonzero)], reps)
    med = {key: statistics.median(v) for key, v in t.items()}
    print("| %s @%dx%d | %s | %.1f %% | %s | %s | %s | %s | %s | %.2fx / %.2fx |"
          % (name, H, W, dtype_name(dtype), listed_share(sets), fmt(t["mask"]), fmt(t["list"]), fmt(t["mask+peaks"]),
             fmt(t["list+peaks"]), fmt(t["dense"]), med["dense"] / med["mask"], med["dense"] / med["list"]))
    return ("| %s @%dx%d | %s | %d | %s | %s | %.2fx |"
            % (name, H, W, dtype_name(dtype), n, fmt(t["peaks"]), fmt(t["nonzero"]), med["nonzero"] / med["peaks"]))


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    assert torch.cuda.is_available(), "target_peaks.py needs a GPU"
    print("# Change-based peak suppression and peak lists at 10 % changed pixels\n")
    print("%s, torch %s; times in us per call, median [min..max] over %d interleaved rounds of %d calls\n"
          % (torch.cuda.get_device_name(0), torch.__version__, reps, BATCH))
    print("| map | dtype | changed pixels | cbinfer_cbpeaks_forward, mask form | list form | mask form + cbinfer_peaks_list "
          "| list form + cbinfer_peaks_list | dense torch formula | dense / mask form, dense / list form |")
    print("|---|---|---|---|---|---|---|---|---|")
    second = []
    with torch.no_grad():
        for spec in MAPS:
            for dtype in (torch.float32, torch.float16):
                second.append(one_map(*spec, dtype=dtype, reps=reps))
    print("\n## The list alone: cbinfer_peaks_list (no host sync) against torch.nonzero of the dense result (with its sync)\n")
    print("| map | dtype | peaks | cbinfer_peaks_list | torch.nonzero | nonzero / peaks_list |")
    print("|---|---|---|---|---|---|")
    print("\n".join(second))


if __name__ == "__main__":
    main()
