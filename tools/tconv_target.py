#!/usr/bin/env python3
"""Target of the change-based transposed convolution (cb_tconv.hip): fp32 (bf16-triple arithmetic), feedback mode,
threshold 0.05, about 10 % changed INPUT pixels per frame in whole blocks (frame i is a base map with fresh values on
change set i, so it differs from frame i - 1 on two sets of 5 % each) --
  128 -> 64, 2x2 s2 at 80x120 -> 160x240;  128 -> 64, 4x4 s2 p1 at 80x120 -> 160x240;
  256 -> 128, 3x3 s2 p1 op1 at 40x60 -> 80x120.
Per layer:
  frame        cbinfer_cbconvtranspose2d_forward: detection + contraction, two launches;
  dense        F.conv_transpose2d on the same tensor (the vendor library);
  detection    cbinfer_change_detection_tconv alone (state refresh and footprint);
  contraction  cbinfer_conv_changed_tconv alone, fed the frame's ascending list of output pixels (list mode: the kernel
               buckets it by phase itself);
  yardstick    cbg_conv_kernel (cbinfer_conv_changed_geom, list mode) on a stride-1 layer with the SAME filter size on
               C / (sH sW) channels -- the same useful depth C kH kW / (sH sW) = mean C taps(phase) --, the same K, the
               same output map and the same list: what the gather contraction costs without the phase split.
The measuring method is tools/target_common.py's, with two warm-up batches per run; every call of a batch takes the next
of 16 frames.  Prints markdown (profiles/tconv_target.md).
usage: tconv_target.py [rounds]"""
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
from target_common import BATCH, SETS, change_sets, fmt, listed_share, moving_frames, rounds  # noqa: E402

#          name, C, K, (k, s, p, op), Hi, Wi, block (input pixels)
LAYERS = [("128->64 2x2 s2", 128, 64, (2, 2, 0, 0), 80, 120, 4),
          ("128->64 4x4 s2 p1", 128, 64, (4, 2, 1, 0), 80, 120, 4),
          ("256->128 3x3 s2 p1 op1", 256, 128, (3, 2, 1, 1), 40, 60, 2)]
TH = 0.05


def footprint(changed, k, s, p, Ho, Wo):
    """The output pixels that read a changed input pixel: (oy, ox) iff oy + p - ky = s iy for a changed (iy, ix)."""
    listed = np.zeros((Ho, Wo), dtype=bool)
    iy, ix = np.nonzero(changed)
    for ky in range(k):
        for kx in range(k):
            oy, ox = iy * s - p + ky, ix * s - p + kx
            ok = (oy >= 0) & (oy < Ho) & (ox >= 0) & (ox < Wo)
            listed[oy[ok], ox[ok]] = True
    return listed


def layer(name, Cn, K, ksp, Hi, Wi, block, reps):
    k, s, p, op = ksp
    rng = np.random.default_rng(7)
    torch.manual_seed(7)
    st = torch.cuda.current_stream().cuda_stream
    g = ctypes.pointer(_lib.TGeom(k, k, s, s, p, p, 1, 1, op, op))
    ho, wo = ctypes.c_int(), ctypes.c_int()
    check(C.cbinfer_tconv_out_size(Hi, Wi, g, ctypes.byref(ho), ctypes.byref(wo)))
    Ho, Wo = ho.value, wo.value
    w = torch.randn(Cn, K, k, k, device="cuda") / (Cn * k * k / (s * s)) ** 0.5
    b = torch.randn(K, device="cuda")
    sets = change_sets(rng, Hi, Wi, block, 0.05)
    frames = moving_frames(torch.rand(1, Cn, Hi, Wi, device="cuda"), sets, Cn, torch.float32)
    lists = []
    for i, m in enumerate(sets):
        px = np.flatnonzero(footprint(m | sets[i - 1], k, s, p, Ho, Wo).reshape(-1)).astype(np.int32)
        lists.append(torch.from_numpy(px).cuda())
    changed = listed_share([m | sets[i - 1] for i, m in enumerate(sets)])
    listed = statistics.mean(t.numel() for t in lists) / float(Ho * Wo) * 100.0

    arith = _lib.CB_F32S
    wp = torch.empty(C.cbinfer_tconv_prepared_weights_bytes(K, Cn, g, arith), dtype=torch.uint8, device="cuda")
    check(C.cbinfer_tconv_prep_weights(ptr(w), ptr(wp), K, Cn, Hi, Wi, g, arith, st))

    def state():
        return dict(prevIn=torch.full((1, Cn, Hi, Wi), float("inf"), device="cuda"),
                    out=torch.zeros(1, K, Ho, Wo, device="cuda"),
                    bits=torch.zeros(C.cbinfer_frame_mask_bytes(Ho, Wo) // 8, dtype=torch.int64, device="cuda"),
                    ws=torch.zeros(C.cbinfer_tconv_workspace_bytes(), dtype=torch.uint8, device="cuda"))
    A, D, L = state(), state(), state()

    def frame(i):
        check(C.cbinfer_cbconvtranspose2d_forward(ptr(frames[i % SETS]), ptr(A['prevIn']), ptr(A['out']), ptr(A['bits']),
                                                  ptr(wp), ptr(b), Cn, Hi, Wi, K, g, TH, 1, 1, 0, ptr(A['ws']), arith, st))

    def dense(i):
        return F.conv_transpose2d(frames[i % SETS], w, b, stride=s, padding=p, output_padding=op)

    def detection(i):
        # (nobody consumes the mask here: the bits pile up, which costs the detection nothing)
        check(C.cbinfer_change_detection_tconv(ptr(frames[i % SETS]), ptr(D['prevIn']), ptr(D['bits']), Cn, Hi, Wi, g,
                                               TH, 1, _lib.CB_F32, st))

    def contraction(i):
        lst = lists[i % SETS]
        check(C.cbinfer_conv_changed_tconv(ptr(frames[i % SETS]), ptr(lst), lst.numel(), None, None, ptr(wp), ptr(b),
                                           ptr(L['out']), Cn, Hi, Wi, K, g, 0, ptr(L['ws']), arith, st))

    # the yardstick: a stride-1 layer of the same filter size on C / (sH sW) channels over the same output map
    Cy, Hy, Wy = Cn // (s * s), Ho + k - 1, Wo + k - 1
    gy = ctypes.pointer(_lib.Geom(k, k, 1, 1, 0, 0, 1, 1))
    xy = torch.rand(1, Cy, Hy, Wy, device="cuda")
    wy = torch.randn(K, Cy, k, k, device="cuda") / (Cy * k * k) ** 0.5
    wpy = torch.empty(C.cbinfer_geom_prepared_weights_bytes(K, Cy, gy, arith), dtype=torch.uint8, device="cuda")
    check(C.cbinfer_geom_prep_weights(ptr(wy), ptr(wpy), K, Cy, Hy, Wy, gy, arith, st))
    outy = torch.zeros(1, K, Ho, Wo, device="cuda")
    wsy = torch.zeros(C.cbinfer_geom_workspace_bytes(), dtype=torch.uint8, device="cuda")

    def yardstick(i):
        lst = lists[i % SETS]
        check(C.cbinfer_conv_changed_geom(ptr(xy), ptr(lst), lst.numel(), None, None, None, None, ptr(wpy), ptr(b),
                                          ptr(outy), Cy, Hy, Wy, K, gy, 0, ptr(wsy), arith, st))

    # results first: after a frame the layer's state is the dense operator's output within the bf16-triple bar
    # (64 2^-24 sum|a||b|), and so is the list-mode contraction at its listed pixels
    for i in range(SETS + 1):
        frame(i)
    want = F.conv_transpose2d(A['prevIn'].double(), w.double(), b.double(), stride=s, padding=p, output_padding=op)
    mag = F.conv_transpose2d(A['prevIn'].double().abs(), w.double().abs(), b.double().abs(), stride=s, padding=p,
                             output_padding=op)
    err = (A['out'].double() - want).abs()
    assert bool((err <= 64 * 2.0 ** -24 * mag).all()), "the frame is off the float64 operator: %g" % float(err.max())
    contraction(0)
    torch.cuda.synchronize()
    sel = lists[0].long()
    want0 = F.conv_transpose2d(frames[0].double(), w.double(), b.double(), stride=s, padding=p, output_padding=op)
    mag0 = F.conv_transpose2d(frames[0].double().abs(), w.double().abs(), b.double().abs(), stride=s, padding=p,
                              output_padding=op)
    err0 = (L['out'].double() - want0).abs().view(K, -1)[:, sel]
    assert bool((err0 <= 64 * 2.0 ** -24 * mag0.view(K, -1)[:, sel]).all()), "the list-mode contraction is off"

    t = rounds([("frame", frame), ("dense", dense), ("det", detection), ("con", contraction), ("yard", yardstick)], reps,
               warm=2)
    med = {key: statistics.median(v) for key, v in t.items()}
    print("| %s | %dx%d -> %dx%d | %.1f %% / %.1f %% | %s | %s | %.2fx | %s | %s | %s | %.2fx |"
          % (name, Hi, Wi, Ho, Wo, changed, listed, fmt(t["frame"]), fmt(t["dense"]), med["dense"] / med["frame"],
             fmt(t["det"]), fmt(t["con"]), fmt(t["yard"]), med["con"] / med["yard"]))


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    assert torch.cuda.is_available(), "tconv_target.py needs a GPU"
    print("# Change-based transposed convolution at about 10 % changed input pixels (fp32, feedback mode)\n")
    print("%s, torch %s; times in us per call, median [min..max] over %d interleaved rounds of %d calls\n"
          % (torch.cuda.get_device_name(0), torch.__version__, reps, BATCH))
    print("| layer | map | changed input / listed output pixels | frame (2 launches) | F.conv_transpose2d | dense / frame "
          "| detection alone | contraction alone (list mode) | cbg_conv_kernel, same useful depth, K and list "
          "| contraction / yardstick |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    with torch.no_grad():
        for spec in LAYERS:
            layer(*spec, reps=reps)


if __name__ == "__main__":
    main()
