#!/usr/bin/env python3
"""Target of change-based pooling for any window (cb_pool2d.hip): three layers at 10 % changed input pixels per frame
(whole blocks of 32x32 frame pixels, i.e. 16 / 32 / 4 pixels at the three resolutions), fp32 --
  stem pool    64 ch  160x240  3x3 stride 2 pad 1 max
  ceil pool    16 ch  320x480  3x3 stride 2 ceil_mode max
  transition  256 ch   40x60   2x2 average
Per layer, interleaved -- REPS rounds of alternating batches of BATCH calls, device events around each batch, median
[min..max] of the per-call time: the frame of cbinfer_cbpool2d_forward (both launches) fed the change LIST and fed the
change MASK, torch's dense F.max_pool2d / F.avg_pool2d on the same tensor, and, for a 2x2/stride-2 window, the existing
cbinfer_max_pool2d launch on the same list (it computes the maximum, not the average: the window is what is compared).
Every call of a batch takes the next of 16 change sets.  Prints markdown (profiles/pool_target.md).
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

#          name, channels, H, W, window, stride, padding, ceil, op, block
LAYERS = [("stem pool 64 ch 3x3 s2 p1 max", 64, 160, 240, 3, 2, 1, False, "max", 16),
          ("ceil pool 16 ch 3x3 s2 ceil max", 16, 320, 480, 3, 2, 0, True, "max", 32),
          ("transition 256 ch 2x2 avg", 256, 40, 60, 2, 2, 0, False, "avg", 4)]
BATCH, SETS = 32, 16


def timed(fn, n):
    """mean device time of fn(i) in us over n back-to-back calls (one warm-up)"""
    fn(0)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(n):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / n


def change_sets(rng, H, W, block):
    """SETS bool maps with 10 % of the block x block tiles set."""
    by, bx = (H + block - 1) // block, (W + block - 1) // block
    out = []
    for _ in range(SETS):
        tiles = np.zeros(by * bx, dtype=bool)
        tiles[rng.choice(by * bx, size=max(1, round(0.10 * by * bx)), replace=False)] = True
        out.append(np.kron(tiles.reshape(by, bx), np.ones((block, block), dtype=bool))[:H, :W])
    return out


def pack(mask):
    H, W = mask.shape
    wpr = (W + 63) // 64
    pad = np.zeros((H, wpr * 64), dtype=bool)
    pad[:, :W] = mask
    return np.packbits(pad.reshape(H, wpr, 64), axis=-1, bitorder='little').reshape(-1).view('<u8').view(np.int64).copy()


def fmt(v):
    return "%.1f [%.1f..%.1f]" % (statistics.median(v), min(v), max(v))


def layer(name, Cn, H, W, k, s, p, ceil, op, block, reps):
    rng = np.random.default_rng(7)
    g = _lib.Pool(k, k, s, s, p, p, int(ceil), _lib.POOL_MAX if op == "max" else _lib.POOL_AVG_PAD)
    gp = ctypes.pointer(g)
    ho, wo = ctypes.c_int(), ctypes.c_int()
    check(C.cbinfer_pool_out_size(H, W, gp, ctypes.byref(ho), ctypes.byref(wo)))
    Ho, Wo = ho.value, wo.value
    x = torch.rand(1, Cn, H, W, device="cuda")
    sets = change_sets(rng, H, W, block)
    lists = [torch.from_numpy(np.flatnonzero(m.reshape(-1)).astype(np.int32)).cuda() for m in sets]
    masks = [torch.from_numpy(pack(m)).cuda() for m in sets]
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
    t = {key: [] for key, _ in runs}
    for _ in range(reps):
        for key, fn in runs:
            t[key].append(timed(fn, BATCH))
    listed = statistics.mean(float(m.mean()) for m in sets) * 100.0
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
