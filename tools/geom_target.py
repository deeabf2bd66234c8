#!/usr/bin/env python3
"""Target of the general-geometry CBConv2d (cb_geomconv.hip): three layers at about 10 % changed input pixels per frame
(SyntheticVideo; blocks of 32x32 frame pixels, i.e. 32 / 16 / 4 pixels at the three resolutions) --
  stem    3 -> 64   7x7 stride 2 pad 3, no bias   @ 320x480
  down   64 -> 128  3x3 stride 2 pad 1            @ 160x240
  atrous 256 -> 256 3x3 dilation 2 pad 2          @ 40x60
Per layer, fp32 in the default f32-equivalent arithmetic: the kernel times of the frame's two launches (device events
around each library call, mean over the walk), the frame time of the module (host clock around `steps` eager frames ending
in a synchronise), torch.nn.functional.conv2d on the same tensors, and -- interleaved, REPS rounds of alternating
batches -- the contraction alone in list mode against the unit-geometry list kernel (cbinfer_conv_changed) on a layer of
the same Cin kH kW, K and list.  Prints markdown (profiles/geom_conv_target.md).
usage: geom_target.py [steps]"""
import ctypes
import os
import statistics
import sys
import time

import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pycbinfer  # noqa: E402
from cbinfer_amd import _lib, workloads  # noqa: E402
from cbinfer_amd._lib import C, check, ptr  # noqa: E402

LAYERS = [("stem 3->64 7x7 s2 p3 no bias", 3, 64, 7, 2, 3, 1, False, 320, 480, 32),
          ("down 64->128 3x3 s2 p1", 64, 128, 3, 2, 1, 1, True, 160, 240, 16),
          ("atrous 256->256 3x3 d2 p2", 256, 256, 3, 1, 2, 2, True, 40, 60, 4)]
REPS, BATCH = 15, 20


def events():
    return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def timed(fn, n):
    """mean device time of fn() in us over n back-to-back calls (one warm-up)"""
    fn()
    a, b = events()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / n


def layer(name, Cin, K, k, s, p, d, bias, H, W, block, steps):
    torch.manual_seed(1)
    conv = nn.Conv2d(Cin, K, k, stride=s, padding=p, dilation=d, bias=bias).cuda()
    m = pycbinfer.CBConv2d(conv, 0.05, generalGeometry=True)
    m.feedbackLoop = True
    vid = workloads.SyntheticVideo(H=H, W=W, C=Cin, ratio=0.10, block=block, seed=7)
    frames = vid.frames(48)
    st = torch.cuda.current_stream().cuda_stream
    with torch.no_grad():
        for f in frames[:8]:
            m(f)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            m(frames[8 + i % 40])
        torch.cuda.synchronize()
        frame_us = (time.perf_counter() - t0) * 1e6 / steps
        # the two launches on their own, device events around each library call
        g = m._geom_struct()
        work, Ho, Wo = m._work, m.prevOutput.size(-2), m.prevOutput.size(-1)
        wp = m._geom_weights(H, W, _lib.CB_F32S)
        b = ptr(conv.bias.detach()) if bias else None
        det, con, counts = [], [], []
        for i in range(40):
            f = frames[8 + i]
            e0, e1 = events()
            e2 = torch.cuda.Event(enable_timing=True)
            e0.record()
            check(C.cbinfer_change_detection_geom(ptr(f), ptr(m.prevInput), ptr(work['bits']), Cin, H, W, g, 0.05, 1,
                                                  _lib.CB_F32, st))
            e1.record()
            check(C.cbinfer_conv_changed_geom(ptr(m.prevInput), None, 0, None, ptr(work['bits']), ptr(work['idx']),
                                              ptr(work['count']), ptr(wp), b, ptr(m.prevOutput), Cin, H, W, K, g, 0,
                                              ptr(work['conv']), _lib.CB_F32S, st))
            e2.record()
            torch.cuda.synchronize()
            det.append(e0.elapsed_time(e1) * 1e3)
            con.append(e1.elapsed_time(e2) * 1e3)
            counts.append(int(work['count'].item()))
        x = frames[-1]
        dense_us = timed(lambda: F.conv2d(x, conv.weight, conv.bias, stride=s, padding=p, dilation=d), 200)
        # contraction alone, list mode, against the unit-geometry list kernel: same Cin k k, K and list, interleaved
        n = counts[-1]
        idx, cnt = work['idx'].clone(), work['count'].clone()
        unit_in = torch.rand(1, Cin, Ho, Wo, device="cuda")
        unit_out = torch.zeros(1, K, Ho, Wo, device="cuda")
        uw = torch.empty(C.cbinfer_prepared_weights_bytes(K, Cin, k, k, _lib.CB_F32S), dtype=torch.uint8, device="cuda")
        check(C.cbinfer_prep_weights(ptr(conv.weight.detach()), ptr(uw), K, Cin, k, k, Ho, Wo, _lib.CB_F32S, st))
        uws = torch.zeros(C.cbinfer_conv_workspace_bytes(), dtype=torch.uint8, device="cuda")

        def geom_list():
            check(C.cbinfer_conv_changed_geom(ptr(m.prevInput), ptr(idx), Ho * Wo, ptr(cnt), None, None, None, ptr(wp), b,
                                              ptr(m.prevOutput), Cin, H, W, K, g, 0, ptr(work['conv']), _lib.CB_F32S, st))

        def unit_list():
            check(C.cbinfer_conv_changed(ptr(unit_in), ptr(idx), Ho * Wo, ptr(cnt), ptr(uw), b, ptr(unit_out), Cin, Ho,
                                         Wo, K, k, k, 0, 0, None, 0, ptr(uws), _lib.CB_F32S, st))

        ga, ua = [], []
        for _ in range(REPS):
            ga.append(timed(geom_list, BATCH))
            ua.append(timed(unit_list, BATCH))
    med = statistics.median
    gm, um = med(ga), med(ua)
    print("| %s @%dx%d -> %dx%d | %.0f (%.1f %%) | %.1f | %.1f | %.1f | %.1f | %.2fx | %.1f [%.1f..%.1f] | %.1f [%.1f..%.1f] | %.2f |"
          % (name, H, W, Ho, Wo, statistics.mean(counts), 100.0 * statistics.mean(counts) / (Ho * Wo),
             statistics.mean(det), statistics.mean(con), frame_us, dense_us, dense_us / frame_us,
             gm, min(ga), max(ga), um, min(ua), max(ua), gm / um))


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 400
    assert torch.cuda.is_available(), "geom_target.py needs a GPU"
    print("# General-geometry CBConv2d at 10 % changed input pixels (fp32, bf16-triple arithmetic, feedback mode)\n")
    print("%s, torch %s; times in us; [min..max] over %d interleaved rounds of %d launches\n"
          % (torch.cuda.get_device_name(0), torch.__version__, REPS, BATCH))
    print("| layer | listed output pixels | detection launch | contraction launch (mask mode) | frame (module, eager) "
          "| F.conv2d | F.conv2d / frame | contraction, list mode | unit-geometry list kernel, same Cin k k, K, list "
          "| ratio |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for spec in LAYERS:
        layer(*spec, steps=steps)


if __name__ == "__main__":
    main()
