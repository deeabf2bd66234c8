#!/usr/bin/env python3
"""Target of the change-based grouped convolution (cb_groupconv.hip): fp32 (bf16 triples) and fp16, feedback mode, ReLU,
threshold 0.05, about 10 % changed INPUT pixels per frame in whole blocks (frame i is a base map with fresh values on
change set i, so it differs from frame i - 1 on two sets of 5 % each).  The grouped 3x3 layers of ResNeXt-50 32x4d at a
320x480 frame (stages 1, 2 -- strided -- and 4) and a RegNet-type layer of group width 24.  Per layer and dtype:
  detect       cbinfer_change_detection_geom alone (feedback refresh), the frame's first launch;
  contract     cbinfer_conv_changed_grouped alone, fed the frame's list (the second launch without its mask scan);
  frame        cbinfer_cbgroupconv2d_forward: both launches;
  module       CBGroupedConv2d.forward (cloneOutput=False), host work included: device events around the calls;
  dense        F.conv2d(groups=G) on the same tensors (the vendor library), the dense denominator;
  groups=1     the same shape as ONE group through the general-geometry frame (cbinfer_cbconv2d_forward_geom, G times
               the multiply-adds, no row padding): what the grouped form's padding costs against it.
useful / issued: Kg / KgP * Ckkg / CkkgP, the share of the MFMA work that is not padding.
The measuring method is tools/target_common.py's, with two warm-up batches per run; every call of a batch takes the next
of 16 frames.  Prints markdown (profiles/group_target.md).
usage: group_target.py [rounds]"""
import ctypes
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cbinfer_amd  # noqa: E402
from cbinfer_amd import _lib  # noqa: E402
from cbinfer_amd._lib import C, check, ptr  # noqa: E402
from target_common import BATCH, SETS, change_sets, dtype_name, fmt, listed_share, moving_frames, rounds  # noqa: E402

#          name, C, K, G, s, Hi, Wi, block (input pixels)
LAYERS = [("128->128 G=32 3x3", 128, 128, 32, 1, 80, 120, 4),
          ("256->256 G=32 3x3 s2", 256, 256, 32, 2, 80, 120, 4),
          ("240->240 G=10 3x3", 240, 240, 10, 1, 40, 60, 2),
          ("1024->1024 G=32 3x3", 1024, 1024, 32, 1, 20, 30, 2)]
TH = 0.05


def layer(name, Cn, K, G, s, Hi, Wi, block, dtype, reps):
    rng = np.random.default_rng(7)
    torch.manual_seed(7)
    st = torch.cuda.current_stream().cuda_stream
    half = dtype == torch.float16
    code, edt = (_lib.CB_F16, _lib.CB_F16) if half else (_lib.CB_F32S, _lib.CB_F32)
    k, p, d = 3, 1, 1
    g = ctypes.pointer(_lib.Geom(k, k, s, s, p, p, d, d))
    ho, wo = ctypes.c_int(), ctypes.c_int()
    check(C.cbinfer_geom_out_size(Hi, Wi, g, ctypes.byref(ho), ctypes.byref(wo)))
    Ho, Wo = ho.value, wo.value
    Cg, Kg = Cn // G, K // G
    conv = nn.Conv2d(Cn, K, k, s, p, d, groups=G).cuda().to(dtype)
    w, b = conv.weight.detach(), conv.bias.detach()
    w1 = (torch.randn(K, Cn, k, k, device="cuda") / (3.0 * Cn ** 0.5)).to(dtype)      # the same shape as one group
    sets = change_sets(rng, Hi, Wi, block, 0.05)
    frames = moving_frames(torch.rand(1, Cn, Hi, Wi, device="cuda").to(dtype), sets, Cn, dtype)
    one = torch.ones(1, 1, k, k)
    lists = []
    for i, m in enumerate(sets):
        moved = torch.from_numpy((m | sets[i - 1]).astype(np.float32))[None, None]
        listed = (F.conv2d(moved, one, stride=s, padding=p, dilation=d) > 0)[0, 0]
        lists.append(torch.nonzero(listed.reshape(-1)).reshape(-1).int().cuda())
    changed = listed_share([m | sets[i - 1] for i, m in enumerate(sets)])
    listedShare = statistics.mean(float(l.numel()) for l in lists) / (Ho * Wo) * 100.0

    def state():
        return dict(prevIn=torch.full((1, Cn, Hi, Wi), float("inf"), device="cuda", dtype=dtype),
                    out=torch.zeros(1, K, Ho, Wo, device="cuda", dtype=dtype),
                    fm=torch.zeros(C.cbinfer_frame_mask_bytes(Ho, Wo) // 8, dtype=torch.int64, device="cuda"),
                    idx=torch.empty(Ho * Wo, dtype=torch.int32, device="cuda"),
                    count=torch.zeros(1, dtype=torch.int32, device="cuda"))
    A, D, L, O = state(), state(), state(), state()
    wp = torch.empty(C.cbinfer_groupconv_prepared_weights_bytes(K, Cn, G, g, code), dtype=torch.uint8, device="cuda")
    check(C.cbinfer_groupconv_prep_weights(ptr(w.contiguous()), ptr(wp), K, Cn, G, Hi, Wi, g, code, st))
    wp1 = torch.empty(C.cbinfer_geom_prepared_weights_bytes(K, Cn, g, code), dtype=torch.uint8, device="cuda")
    check(C.cbinfer_geom_prep_weights(ptr(w1), ptr(wp1), K, Cn, Hi, Wi, g, code, st))
    ws = torch.zeros(C.cbinfer_geom_workspace_bytes(), dtype=torch.uint8, device="cuda")
    mod = cbinfer_amd.CBGroupedConv2d(conv, TH)
    mod.feedbackLoop, mod.withReLU, mod.cloneOutput = True, True, False

    def frame(i):
        check(C.cbinfer_cbgroupconv2d_forward(ptr(frames[i % SETS]), ptr(A['prevIn']), ptr(A['out']), ptr(A['fm']),
                                              ptr(A['idx']), ptr(A['count']), ptr(wp), ptr(b), Cn, Hi, Wi, K, G, g, TH, 1,
                                              1, 1, code, st))

    def detect(i):      # (its mask is never consumed: bits pile up, which the detection does not look at)
        check(C.cbinfer_change_detection_geom(ptr(frames[i % SETS]), ptr(D['prevIn']), ptr(D['fm']), Cn, Hi, Wi, g, TH, 1,
                                              edt, st))

    def contract(i):
        lst = lists[i % SETS]
        check(C.cbinfer_conv_changed_grouped(ptr(frames[i % SETS]), ptr(lst), lst.numel(), None, None, None, None,
                                             ptr(wp), ptr(b), ptr(L['out']), Cn, Hi, Wi, K, G, g, 1, code, st))

    def module(i):
        mod(frames[i % SETS])

    def dense(i):
        return F.conv2d(frames[i % SETS], w, b, stride=s, padding=p, dilation=d, groups=G)

    def ungrouped(i):
        check(C.cbinfer_cbconv2d_forward_geom(ptr(frames[i % SETS]), ptr(O['prevIn']), ptr(O['out']), ptr(O['fm']),
                                              ptr(O['idx']), ptr(O['count']), ptr(wp1), ptr(b), Cn, Hi, Wi, K, g, TH, 1,
                                              1, 1, 0, Ho * Wo, ptr(ws), code, st))

    # results first: after a pass over the frames the state is the float64 layer's within the kernel's bound
    for i in range(SETS + 1):
        frame(i)
    torch.cuda.synchronize()
    kw = dict(stride=s, padding=p, dilation=d, groups=G)
    src, w64, b64 = A['prevIn'].cpu().double(), w.cpu().double(), b.cpu().double()
    want = F.conv2d(src, w64, b64, **kw).clamp(min=0)
    mag = F.conv2d(src.abs(), w64.abs(), b64.abs(), **kw)
    Ckkg = Cg * k * k
    bound = 2.0 ** -11 * want.abs() + Ckkg * 2.0 ** -23 * mag + 2.0 ** -24 if half else 64 * 2.0 ** -24 * mag
    assert float(((A['out'].cpu().double() - want).abs() / bound).max()) <= 1.0, "the frame is off the float64 layer"

    t = rounds([("detect", detect), ("contract", contract), ("frame", frame), ("module", module), ("dense", dense),
                ("groups=1", ungrouped)], reps, warm=2)
    med = {key: statistics.median(v) for key, v in t.items()}
    rows = 16 if Kg <= 16 else 32 if Kg <= 32 else 64
    KgP, CkkgP = (Kg + rows - 1) // rows * rows, (Ckkg + 31) // 32 * 32
    print("| %s | %dx%d -> %dx%d | %s | %.1f %% / %.1f %% | %d | %.3f | %s | %s | %s | %s | %s | %.2fx | %s | %.2fx |" % (
        name, Hi, Wi, Ho, Wo, dtype_name(dtype), changed, listedShare, rows,
        (Kg / float(KgP)) * (Ckkg / float(CkkgP)), fmt(t["dense"]), fmt(t["detect"]), fmt(t["contract"]), fmt(t["frame"]),
        fmt(t["module"]), med["dense"] / med["frame"], fmt(t["groups=1"]), med["groups=1"] / med["frame"]), flush=True)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    assert torch.cuda.is_available(), "group_target.py needs a GPU"
    print("# Change-based grouped convolution at about 10 % changed input pixels (feedback mode, ReLU)\n")
    print("%s, torch %s; times in us per call, median [min..max] over %d interleaved rounds of %d calls\n"
          % (torch.cuda.get_device_name(0), torch.__version__, reps, BATCH))
    print("| layer | map | dtype | changed input / listed output pixels | ROWS | useful / issued MACs | "
          "F.conv2d(groups=G) | detection | contraction (list form) | frame (2 launches) | module frame | dense / frame | "
          "groups=1 frame (general geometry) | groups=1 / grouped |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    with torch.no_grad():
        for spec in LAYERS:
            for dtype in (torch.float32, torch.float16):
                layer(*spec, dtype=dtype, reps=reps)


if __name__ == "__main__":
    main()
