#!/usr/bin/env python3
"""Target of the change-based adaptive pool (cb_adaptpool.hip): four layers at 10 % changed input pixels per frame (whole
blocks of pixels), fp32 --
  classifier head  960 ch   15x20  -> 1   avg
  SE squeeze        96 ch   60x80  -> 1   avg
  PSP bin          512 ch   60x80  -> 6   avg
  wide early map    64 ch  320x480 -> 1   avg and max
Per layer, interleaved -- REPS rounds of alternating batches of BATCH calls, device events around each batch, median
[min..max] of the per-call time: the frame of cbinfer_cbadaptivepool2d_forward fed the change MASK (two launches) and fed
the change LIST (three launches), and torch's dense F.adaptive_avg_pool2d / F.adaptive_max_pool2d on the same tensor.
Every call of a batch takes the next of 16 change sets.  Before timing, an every-pixel frame is checked: max against CPU
torch bit for bit, avg within 1e-5 relative of it (the summation order is the library's own).  Prints markdown
(profiles/adaptive_pool_target.md).
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

#          name, channels, H, W, output size, op, block
LAYERS = [("classifier head 960 ch avg", 960, 15, 20, 1, "avg", 2),
          ("SE squeeze 96 ch avg", 96, 60, 80, 1, "avg", 8),
          ("PSP bin 512 ch avg", 512, 60, 80, 6, "avg", 8),
          ("wide early map 64 ch avg", 64, 320, 480, 1, "avg", 32),
          ("wide early map 64 ch max", 64, 320, 480, 1, "max", 32)]
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


def layer(name, Cn, H, W, o, op, block, reps):
    rng = np.random.default_rng(7)
    code = _lib.ADAPT_MAX if op == "max" else _lib.ADAPT_AVG
    x = torch.rand(1, Cn, H, W, device="cuda")
    sets = change_sets(rng, H, W, block)
    lists = [torch.from_numpy(np.flatnonzero(m.reshape(-1)).astype(np.int32)).cuda() for m in sets]
    masks = [torch.from_numpy(pack(m)).cuda() for m in sets]
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
    runs = [("list", cb_list), ("mask", cb_mask), ("dense", dense)]
    t = {key: [] for key, _ in runs}
    for _ in range(reps):
        for key, fn in runs:
            t[key].append(timed(fn, BATCH))
    # the state after all those frames is still the every-pixel frame's (the input never changed)
    first = out.clone()
    frame(None, None)
    assert torch.equal(out, first)
    listed = statistics.mean(float(m.mean()) for m in sets) * 100.0
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
