#!/usr/bin/env python3
"""Target of the change-based resize (cb_resize.hip): cbinfer_cbresize_forward with the input in MASK form (one launch)
and in LIST form (one more launch in front), at 10 % and 100 % changed INPUT pixels (whole 4x4 blocks of input pixels),
fp32 and fp16, against torch's dense F.interpolate on the same device tensor --
  a 19-class segmentation head  19 ch @ 60x80   -> 480x640  bilinear,
  an FPN-type top-down step     256 ch @ 30x40  -> 60x80    nearest,
  an HRNet-type fuse downscale  64 ch @ 240x320 -> 120x160  bilinear,
  a super-resolution head       3 ch @ 160x240  -> 640x960  bicubic.
The x2 cases (the FPN step, and the same map with bilinear) are also run through cbinfer_cbupsample_forward, the
integer-scale kernel, on the same input and the same change sets.
The measuring method is tools/target_common.py's.  Prints markdown (profiles/resize_target.md).
`resize_target.py warp` measures the grid sampling instead (cb_warp.hip, cbinfer_cbwarp_forward; profiles/warp_target.md)
at 10 % changed input pixels against torch's dense F.grid_sample on the same tensors --
  a fixed homography       64 ch @ 160x240, bilinear, a constant grid,
  a flow warp              32 ch @ 96x320, bilinear, 10 % of the flow changed too (the dense side also pays the
                           base + permute * scale that turns a flow into a grid),
  a rectification          3 ch @ 320x480, bilinear, a constant grid.
usage: resize_target.py [warp] [rounds]"""
import ctypes
import fractions
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
from target_common import BATCH, SETS, change_sets, device_sets, dtype_name, fmt, listed_share, rounds  # noqa: E402

#         name, channels, Hi, Wi, Ho, Wo, mode, also through the integer-scale kernel
CASES = [("segmentation head", 19, 60, 80, 480, 640, "bilinear", False),
         ("FPN top-down step", 256, 30, 40, 60, 80, "nearest", True),
         ("the same, bilinear", 256, 30, 40, 60, 80, "bilinear", True),
         ("fuse-layer downscale", 64, 240, 320, 120, 160, "bilinear", False),
         ("super-resolution head", 3, 160, 240, 640, 960, "bicubic", False)]
MODES = {"nearest": _lib.RESIZE_NEAREST, "bilinear": _lib.RESIZE_BILINEAR, "bicubic": _lib.RESIZE_BICUBIC}


def case(name, Cn, Hi, Wi, Ho, Wo, mode, integer, tdt, share, reps):
    rng = np.random.default_rng(7)
    x = torch.randn(1, Cn, Hi, Wi, device="cuda").to(tdt)
    sets = change_sets(rng, Hi, Wi, 4, share)
    masks, lists = device_sets(sets)
    words = C.cbinfer_mask_words(Ho, Wo)
    st = torch.cuda.current_stream().cuda_stream
    dt = _lib.dtype_code(x)
    fH, fW = fractions.Fraction(Hi, Ho), fractions.Fraction(Wi, Wo)
    rs = ctypes.pointer(_lib.Resize(Ho, Wo, fH.numerator, fH.denominator, fW.numerator, fW.denominator, MODES[mode], 0))
    assert C.cbinfer_resize_supported(rs, Hi, Wi)
    up = ctypes.pointer(_lib.Upsample(Ho // Hi, Wo // Wi, _lib.UPSAMPLE_NEAREST if mode == "nearest" else
                                      _lib.UPSAMPLE_BILINEAR, 0)) if integer else None
    kw = dict(mode=mode) if mode == "nearest" else dict(mode=mode, align_corners=False)

    def made(entry, struct):
        out = torch.empty(1, Cn, Ho, Wo, device="cuda", dtype=tdt)
        bits = torch.zeros(words, dtype=torch.int64, device="cuda")
        copy = torch.zeros(words, dtype=torch.int64, device="cuda")

        def run(i, form="mask"):
            m = masks[i % SETS] if form == "mask" else None
            l = lists[i % SETS] if form == "list" else None
            check(entry(ptr(x), ptr(out), ptr(m), ptr(l), l.numel() if l is not None else 0, None, ptr(bits), ptr(copy),
                        Cn, Hi, Wi, struct, dt, st))
        return out, run

    out, resize = made(C.cbinfer_cbresize_forward, rs)
    # results first: with every pixel listed, nearest is torch's operator bit for bit, bilinear and bicubic follow it to
    # 1e-4 max|x| in fp32 (torch derives its coordinates from a float scale) and to one fp16 rounding more in fp16
    resize(0, form="all")
    want = F.interpolate(x, size=(Ho, Wo), **kw)
    if mode == "nearest":
        assert torch.equal(out, want), "nearest differs from F.interpolate"
    else:
        dev = float((out.double() - F.interpolate(x.double(), size=(Ho, Wo), **kw)).abs().max())
        bar = (1e-4 if tdt == torch.float32 else 1e-4 + 2.0 ** -10 * 1.9) * float(x.abs().max())
        assert dev <= bar, "%s is off the float64 operator by %g" % (mode, dev)
    runs = [("mask", lambda i: resize(i, "mask")), ("list", lambda i: resize(i, "list")),
            ("dense", lambda i: F.interpolate(x, size=(Ho, Wo), **kw))]
    if integer:
        _, upsample = made(C.cbinfer_cbupsample_forward, up)
        runs += [("umask", lambda i: upsample(i, "mask")), ("ulist", lambda i: upsample(i, "list"))]
    t = rounds(runs, reps)
    med = {k: statistics.median(v) for k, v in t.items()}
    listed = listed_share(sets)
    label = "%s, %d ch @%dx%d -> %dx%d %s" % (name, Cn, Hi, Wi, Ho, Wo, mode)
    dname = dtype_name(tdt)
    for form in ("mask", "list"):
        ukey = "u" + form
        print("| %s | %s | %.0f %% | %s | %s | %s | %.2fx | %s | %s |"
              % (label, dname, listed, form, fmt(t[form]), fmt(t["dense"]), med["dense"] / med[form],
                 fmt(t[ukey]) if integer else "-", "%.2fx" % (med[form] / med[ukey]) if integer else "-"))


#              name, channels, H, W, flow
WARP_CASES = [("fixed homography", 64, 160, 240, False), ("flow warp", 32, 96, 320, True),
              ("rectification", 3, 320, 480, False)]


def warp_case(name, Cn, H, W, flow, tdt, reps):
    rng = np.random.default_rng(7)
    x = torch.randn(1, Cn, H, W, device="cuda").to(tdt)
    ys, xs = torch.meshgrid(torch.linspace(-1, 1, H, device="cuda"), torch.linspace(-1, 1, W, device="cuda"), indexing='ij')
    if flow:      # a smooth flow of a few pixels
        co = torch.stack([3 * torch.sin(3 * ys) + 2 * xs, 2 * torch.cos(2 * xs)])[None].contiguous()
        by, bx = torch.meshgrid((2 * torch.arange(H, device="cuda") + 1) / H - 1,
                                (2 * torch.arange(W, device="cuda") + 1) / W - 1, indexing='ij')
        base = torch.stack([bx, by], dim=-1)[None]      # (the pixel centres, align_corners=False)
        scale = torch.tensor([2.0 / W, 2.0 / H], device="cuda")

        def dense(i):
            return F.grid_sample(x, (base + co.permute(0, 2, 3, 1) * scale).to(tdt), mode='bilinear',
                                 padding_mode='border', align_corners=False)
        align = False
    else:         # a homography (the rectification: a radial term on top)
        w = 1 + 0.15 * xs + 0.1 * ys
        r = 1 + (0.08 * (xs * xs + ys * ys) if name == "rectification" else 0)
        co = torch.stack([(0.95 * xs + 0.05 * ys) * r / w, (0.03 * xs + 1.05 * ys) * r / w], dim=-1)[None].contiguous()
        grid_t = co.to(tdt)

        def dense(i):
            return F.grid_sample(x, grid_t, mode='bilinear', padding_mode='border', align_corners=False)
        align = False
    sets = change_sets(rng, H, W, 4, 0.10)
    masks, lists = device_sets(sets)
    cmasks, clists = device_sets(change_sets(rng, H, W, 4, 0.10)) if flow else (None, None)
    words = C.cbinfer_mask_words(H, W)
    st = torch.cuda.current_stream().cuda_stream
    wp = ctypes.pointer(_lib.Warp(H, W, _lib.WARP_BILINEAR, _lib.WARP_BORDER, int(align),
                                  _lib.WARP_FLOW if flow else _lib.WARP_GRID, _lib.CB_F32))
    assert C.cbinfer_warp_supported(wp, H, W)
    out = torch.empty(1, Cn, H, W, device="cuda", dtype=tdt)
    inb, bits, copy = (torch.zeros(words, dtype=torch.int64, device="cuda") for _ in range(3))
    spare = torch.zeros(1, dtype=torch.int32, device="cuda")

    def run(i, form):
        m = masks[i % SETS] if form == "mask" else None
        l = lists[i % SETS] if form == "list" else None
        if form == "all":
            cm, cl, cn = None, None, 0
        elif not flow:
            cm, cl, cn = None, spare, 0      # a constant grid: the empty list
        else:
            cm = cmasks[i % SETS] if form == "mask" else None
            cl = clists[i % SETS] if form == "list" else None
            cn = cl.numel() if cl is not None else 0
        check(C.cbinfer_cbwarp_forward(ptr(x), ptr(co), ptr(out), ptr(m), ptr(l), l.numel() if l is not None else 0, None,
                                       ptr(cm), ptr(cl), cn, None, ptr(inb), ptr(bits), ptr(copy), Cn, H, W, wp,
                                       _lib.dtype_code(x), st))

    run(0, "all")      # results first, against the float64 operator
    g64 = (base + co.permute(0, 2, 3, 1) * scale).double() if flow else co.double()
    dev = float((out.double() - F.grid_sample(x.double(), g64, mode='bilinear', padding_mode='border',
                                              align_corners=False)).abs().max())
    bar = (1e-4 if tdt == torch.float32 else 1e-4 + 2.0 ** -10 * 1.9) * float(x.abs().max())
    assert dev <= bar, "%s is off the float64 operator by %g" % (name, dev)
    t = rounds([("mask", lambda i: run(i, "mask")), ("list", lambda i: run(i, "list")), ("dense", dense)], reps)
    med = {k: statistics.median(v) for k, v in t.items()}
    for form in ("mask", "list"):
        print("| %s, %d ch @%dx%d bilinear | %s | %.0f %% | %s | %s | %s | %.2fx |"
              % (name, Cn, H, W, dtype_name(tdt), listed_share(sets), form, fmt(t[form]), fmt(t["dense"]),
                 med["dense"] / med[form]))


def warp_main(reps):
    print("# Change-based grid sampling at 10 % changed input pixels\n")
    print("%s, torch %s; times in us per call, median [min..max] over %d interleaved rounds of %d calls; the dense operator "
          "is F.grid_sample on the same device tensors (a flow: with the base + permute * scale in front of it); a ratio "
          "below 1 means the change-based call is slower\n" % (torch.cuda.get_device_name(0), torch.__version__, reps, BATCH))
    print("| case | dtype | changed input pixels | form | cbinfer_cbwarp_forward | dense torch operator | dense / "
          "change-based |")
    print("|---|---|---|---|---|---|---|")
    for spec in WARP_CASES:
        for tdt in (torch.float32, torch.float16):
            warp_case(*spec, tdt=tdt, reps=reps)
            sys.stdout.flush()


def main():
    args = [a for a in sys.argv[1:] if a != "warp"]
    if "warp" in sys.argv[1:]:
        assert torch.cuda.is_available(), "resize_target.py needs a GPU"
        return warp_main(int(args[0]) if args else 15)
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    assert torch.cuda.is_available(), "resize_target.py needs a GPU"
    print("# Change-based resize to a size at 10 % and 100 % changed input pixels\n")
    print("%s, torch %s; times in us per call, median [min..max] over %d interleaved rounds of %d calls; the dense operator "
          "is F.interpolate on the same device tensor, the integer-scale kernel cbinfer_cbupsample_forward on the same "
          "input and change sets\n" % (torch.cuda.get_device_name(0), torch.__version__, reps, BATCH))
    print("| case | dtype | changed input pixels | form | cbinfer_cbresize_forward | dense torch operator | dense / "
          "change-based | integer-scale kernel | resize / integer-scale |")
    print("|---|---|---|---|---|---|---|---|---|")
    for spec in CASES:
        for tdt in (torch.float32, torch.float16):
            for share in (0.10, 1.0):
                case(*spec, tdt=tdt, share=share, reps=reps)
                sys.stdout.flush()


if __name__ == "__main__":
    main()
