#!/usr/bin/env python3
"""Target of the change-based per-pixel kernel application (cb_aggr.hip, cbinfer_cbaggregate_forward): fp32
and fp16, 10 % changed pixels in BOTH operands in whole blocks, mask form and list form --
  KPN 5x5 on 64 ch @ 96x320,  local attention 9x9 on 128 ch @ 64x208 and 196 ch @ 48x160,
  involution 7x7 with groups = C / 16 on 256 ch @ 48x160,  a one-sided stereo-type range on 64 ch @ 96x320 --
against the faster of two dense torch formulations on the same tensors in the same process: unfold + einsum, and the loop
of T shifted products.  Before a row is timed its every-pixel result is checked against the float64 formula within the
bound of DESIGN 5.34.  The measuring method is tools/target_common.py's.  Prints markdown (profiles/aggregate_target.md).
(The file is not called *_target.py: tests/test_host_targets.py pins the list of the tools of that name.)
usage: target_aggregate.py [rounds]"""
import ctypes
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cbinfer_amd import _lib  # noqa: E402
from cbinfer_amd._lib import C, check, ptr  # noqa: E402
from target_common import BATCH, SETS, change_sets, device_sets, dtype_name, fmt, listed_share, rounds  # noqa: E402

#        name, channels, groups, H, W, block, displacement ((y0, y1), (x0, x1))
ROWS = [("KPN 5x5, 64 ch", 64, 1, 96, 320, 8, ((-2, 2), (-2, 2))),
        ("local attention 9x9, 128 ch", 128, 1, 64, 208, 4, ((-4, 4), (-4, 4))),
        ("local attention 9x9, 196 ch", 196, 1, 48, 160, 4, ((-4, 4), (-4, 4))),
        ("involution 7x7, 256 ch", 256, 16, 48, 160, 4, ((-3, 3), (-3, 3))),
        ("stereo range, 64 ch", 64, 1, 96, 320, 8, ((0, 0), (-40, 0)))]


def row(name, Cn, G, H, W, block, disp, dtype, reps):
    rng = np.random.default_rng(7)
    torch.manual_seed(7)
    (y0, y1), (x0, x1) = disp
    taps = [(dy, dx) for dy in range(y0, y1 + 1) for dx in range(x0, x1 + 1)]
    T, Cg = len(taps), Cn // G
    # per-pixel weights as a softmax hands them on: positive, summing to one over the taps of a group
    w = torch.softmax(torch.randn(1, G, T, H, W, device="cuda"), dim=2).view(1, G * T, H, W).to(dtype)
    v = torch.randn(1, Cn, H, W, device="cuda").to(dtype)
    # (left, right, top, bottom) zero padding that every tap's window needs
    pads = (max(0, -x0), max(0, x1), max(0, -y0), max(0, y1))
    aggr = ctypes.pointer(_lib.Aggr(y0, y1, x0, x1, 1, G))
    assert C.cbinfer_aggregate_supported(aggr, Cn, H, W)
    sets = change_sets(rng, H, W, block, 0.10)
    masks, lists = device_sets(sets)
    words = C.cbinfer_mask_words(H, W)
    vbits, bits, mcopy = (torch.zeros(words, dtype=torch.int64, device="cuda") for _ in range(3))
    out = torch.empty(1, Cn, H, W, device="cuda", dtype=dtype)
    st = torch.cuda.current_stream().cuda_stream
    dt = _lib.dtype_code(v)

    def window(vp, dy, dx):
        return vp[:, :, pads[2] + dy:pads[2] + dy + H, pads[0] + dx:pads[0] + dx + W]

    def loop(i, w=w, v=v):
        vp, wg = F.pad(v, pads).view(G, Cg, H + pads[2] + pads[3], W + pads[0] + pads[1]), w.view(G, T, H, W)
        acc = wg[:, 0:1] * window(vp, *taps[0])
        for t in range(1, T):
            acc = acc + wg[:, t:t + 1] * window(vp, *taps[t])
        return acc.view(1, Cn, H, W)

    def unfold(i):
        kh, kw = y1 - y0 + 1, x1 - x0 + 1
        cols = F.unfold(F.pad(v, pads), (kh, kw)).view(G, Cg, T, H, W)
        return torch.einsum('gthw,gcthw->gchw', w.view(G, T, H, W), cols).reshape(1, Cn, H, W)

    def frame(mw, lw, mv, lv):
        check(C.cbinfer_cbaggregate_forward(ptr(w), ptr(v), ptr(out), ptr(mw), ptr(lw),
                                            lw.numel() if lw is not None else 0, None, ptr(mv), ptr(lv),
                                            lv.numel() if lv is not None else 0, None, ptr(vbits), ptr(bits), ptr(mcopy),
                                            Cn, H, W, aggr, dt, st))

    # results first: every pixel listed, against the float64 formula within the bound of DESIGN 5.34
    frame(None, None, None, None)
    wd, vd = w.double().view(G, T, H, W), v.double()
    vp = F.pad(vd, pads).view(G, Cg, H + pads[2] + pads[3], W + pads[0] + pads[1])
    prods = [wd[:, t:t + 1] * window(vp, *taps[t]) for t in range(T)]
    ref, S = sum(prods).view(1, Cn, H, W), sum(p.abs() for p in prods).view(1, Cn, H, W)
    bar = (T + 1) * 2.0 ** -24 * S
    if dtype == torch.float16:
        bar = bar + 2.0 ** -11 * ref.abs() + 2.0 ** -25
    assert bool(((out.double() - ref).abs() <= bar).all()), "kernel application beyond its bound"
    assert torch.allclose(loop(0).double(), ref, atol=2e-2), "dense loop"
    assert torch.allclose(unfold(0).double(), ref, atol=2e-2), "dense unfold"
    t = rounds([("mask", lambda i: frame(masks[i % SETS], None, masks[i % SETS], None)),
                ("list", lambda i: frame(None, lists[i % SETS], None, lists[i % SETS])),
                ("loop", loop), ("unfold", unfold)], reps)
    frame(masks[0], None, masks[0], None)
    listed = float(np.unpackbits(mcopy.cpu().numpy().view(np.uint8)).sum()) / (H * W) * 100.0
    dense = min(statistics.median(t["loop"]), statistics.median(t["unfold"]))
    ratios = [dense / statistics.median(t[k]) for k in ("mask", "list")]
    # (a case where the module loses to the dense operator is written in capitals, as in the other tables)
    verdict = "%.2fx / %.2fx" % tuple(ratios) + (" LOSES" if min(ratios) < 1.0 else "")
    print("| %s @%dx%d | %d taps, G = %d | %s | %.1f %% / %.1f %% | %s | %s | %s | %s | %s |"
          % (name, H, W, T, G, dtype_name(dtype), listed_share(sets), listed, fmt(t["mask"]), fmt(t["list"]),
             fmt(t["loop"]), fmt(t["unfold"]), verdict), flush=True)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    assert torch.cuda.is_available(), "target_aggregate.py needs a GPU"
    print("# Change-based per-pixel kernel application at 10 % changed pixels in both operands\n")
    print("%s, torch %s; times in us per call, median [min..max] over %d interleaved rounds of %d calls; the dense "
          "baseline of a row is the faster of its two torch formulations\n"
          % (torch.cuda.get_device_name(0), torch.__version__, reps, BATCH))
    print("| layer | window | dtype | changed / listed pixels | cbinfer_cbaggregate_forward, mask form | list form | "
          "dense torch, shifted products | dense torch, unfold + einsum | dense / mask form, dense / list form |")
    print("|---|---|---|---|---|---|---|---|---|")
    for name, Cn, G, H, W, block, disp in ROWS:
        for dtype in (torch.float32, torch.float16):
            row(name, Cn, G, H, W, block, disp, dtype, reps)


if __name__ == "__main__":
    main()
