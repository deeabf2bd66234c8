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
usage: resize_target.py [rounds]"""
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


def main():
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
