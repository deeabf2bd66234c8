#!/usr/bin/env python3
"""Target of the change-based depthwise convolution (cb_dwconv.hip): fp32 and fp16, feedback mode, threshold 0.05, about
10 % changed INPUT pixels per frame in whole blocks (frame i is a base map with fresh values on change set i, so it
differs from frame i - 1 on two sets of 5 % each).  The depthwise layers of MobileNetV2 at a 320x480 frame, the 7x7
layer of a ConvNeXt-type block and a dilated layer of a DeepLab-type head.  Per layer and dtype:
  own          cbinfer_cbdwconv2d_forward: the layer's own detection (cbinfer_change_detection_geom) + the stencil, two
               launches, feedback mode;
  propagated   cbinfer_cbdwconv2d_forward_propagated fed the producer's change MASK of the frame: footprint, mask move,
               stencil -- three launches, no detection, no input state (not for the dilated layer);
  dense        F.conv2d(groups=C) on the same tensor (the vendor library).
Achieved bytes/s against the ALGORITHMIC bytes of a frame: (input pixels under a tap of a listed output pixel x C +
listed output pixels x K) x element size, plus 2 C Hi Wi x element size for the form with its own detection (input and
state are read once each).
The measuring method is tools/target_common.py's, with two warm-up batches per run; every call of a batch takes the next
of 16 frames.  Prints markdown (profiles/dw_target.md).
usage: dw_target.py [rounds]"""
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
from target_common import BATCH, SETS, change_sets, dtype_name, fmt, listed_share, moving_frames, pack, rounds  # noqa: E402

#          name, C, k, s, p, d, Hi, Wi, block (input pixels)
LAYERS = [("32ch 3x3 s1", 32, 3, 1, 1, 1, 160, 240, 8),
          ("96ch 3x3 s2", 96, 3, 2, 1, 1, 160, 240, 8),
          ("144ch 3x3 s1", 144, 3, 1, 1, 1, 80, 120, 4),
          ("384ch 3x3 s1", 384, 3, 1, 1, 1, 20, 30, 2),
          ("960ch 3x3 s1", 960, 3, 1, 1, 1, 10, 15, 1),
          ("96ch 7x7 s1 p3", 96, 7, 1, 3, 1, 80, 120, 4),
          ("256ch 3x3 d2 p2", 256, 3, 1, 2, 2, 40, 60, 2)]
TH = 0.05


def maps_of(changed, k, s, p, d):
    """(listed output pixels, input pixels under a tap of a listed output pixel) of a changed input map."""
    one = torch.ones(1, 1, k, k)
    listed = F.conv2d(torch.from_numpy(changed.astype(np.float32))[None, None], one, stride=s, padding=p, dilation=d) > 0
    Hi, Wi = changed.shape
    back = F.conv_transpose2d(listed.float(), one, stride=s, padding=p, dilation=d)
    read = torch.zeros(Hi, Wi, dtype=torch.bool)      # (rows and columns behind the last window are never read)
    read[:back.shape[2], :back.shape[3]] = back[0, 0, :Hi, :Wi] > 0
    return listed[0, 0].numpy(), read.numpy()


def layer(name, Cn, k, s, p, d, Hi, Wi, block, dtype, reps):
    rng = np.random.default_rng(7)
    torch.manual_seed(7)
    st = torch.cuda.current_stream().cuda_stream
    code, es = (_lib.CB_F16, 2) if dtype == torch.float16 else (_lib.CB_F32, 4)
    g = ctypes.pointer(_lib.Geom(k, k, s, s, p, p, d, d))
    ho, wo = ctypes.c_int(), ctypes.c_int()
    check(C.cbinfer_geom_out_size(Hi, Wi, g, ctypes.byref(ho), ctypes.byref(wo)))
    Ho, Wo = ho.value, wo.value
    w = (torch.randn(Cn, 1, k, k, device="cuda") / k).to(dtype)
    b = torch.randn(Cn, device="cuda").to(dtype)
    sets = change_sets(rng, Hi, Wi, block, 0.05)
    frames = moving_frames(torch.rand(1, Cn, Hi, Wi, device="cuda").to(dtype), sets, Cn, dtype)
    masks, nbytes = [], []
    for i, m in enumerate(sets):
        moved = m | sets[i - 1]
        masks.append(torch.from_numpy(pack(moved)).cuda())
        listed, read = maps_of(moved, k, s, p, d)
        nbytes.append((int(read.sum()) * Cn + int(listed.sum()) * Cn) * es)
    changed = listed_share([m | sets[i - 1] for i, m in enumerate(sets)])
    listedShare = statistics.mean(float(maps_of(m | sets[i - 1], k, s, p, d)[0].mean()) for i, m in enumerate(sets)) * 100.0
    algo = statistics.mean(nbytes)
    propagated = d == 1 and 2 * p <= k

    words = C.cbinfer_mask_words(Ho, Wo)
    A = dict(prevIn=torch.full((1, Cn, Hi, Wi), float("inf"), device="cuda", dtype=dtype),
             out=torch.zeros(1, Cn, Ho, Wo, device="cuda", dtype=dtype),
             fm=torch.zeros(C.cbinfer_frame_mask_bytes(Ho, Wo) // 8, dtype=torch.int64, device="cuda"))
    P = dict(out=torch.zeros(1, Cn, Ho, Wo, device="cuda", dtype=dtype),
             bits=torch.zeros(words, dtype=torch.int64, device="cuda"),
             copy=torch.zeros(words, dtype=torch.int64, device="cuda"))

    def own(i):
        check(C.cbinfer_cbdwconv2d_forward(ptr(frames[i % SETS]), ptr(A['prevIn']), ptr(A['out']), ptr(A['fm']), ptr(w),
                                           ptr(b), Cn, 1, Hi, Wi, g, TH, 1, 1, _lib.ACT_RELU6, code, st))

    def prop(i, every=0):
        check(C.cbinfer_cbdwconv2d_forward_propagated(ptr(frames[i % SETS]), ptr(P['out']), None, 0, None,
                                                      ptr(masks[i % SETS]), every, ptr(P['bits']), ptr(P['copy']),
                                                      ptr(w), ptr(b), Cn, 1, Hi, Wi, g, _lib.ACT_RELU6, code, st))

    def dense(i):
        return F.conv2d(frames[i % SETS], w, b, stride=s, padding=p, dilation=d, groups=Cn)

    def off(out, src):
        """worst |err| / bound of a state against the float64 layer on the map it was computed from"""
        kw = dict(stride=s, padding=p, dilation=d, groups=Cn)
        want = F.conv2d(src.double(), w.double(), b.double(), **kw).clamp(0, 6)
        mag = F.conv2d(src.double().abs(), w.double().abs(), b.double().abs(), **kw)
        n = k * k + 1
        bound = n * 2.0 ** -24 * mag if es == 4 else 2.0 ** -11 * want.abs() + n * 2.0 ** -23 * mag + 2.0 ** -24
        return float(((out.double() - want).abs() / bound).max())

    # results first: after a pass over the frames the states are the float64 layer's within the kernel's bound
    for i in range(SETS + 1):
        own(i)
    assert off(A['out'], A['prevIn']) <= 1.0, "the frame with its own detection is off the float64 layer"
    runs = [("own", own), ("dense", dense)]
    if propagated:
        prop(0, 1)
        for i in range(1, SETS + 1):
            prop(i)
        assert off(P['out'], frames[0]) <= 1.0, "the propagated frame is off the float64 layer"
        runs.insert(1, ("prop", prop))
    t = rounds(runs, reps, warm=2)
    med = {key: statistics.median(v) for key, v in t.items()}
    detect = 2 * Cn * Hi * Wi * es
    row = "| %s | %dx%d -> %dx%d | %s | %.1f %% / %.1f %% | %s | %s | %.2fx | %.0f |" % (
        name, Hi, Wi, Ho, Wo, dtype_name(dtype), changed, listedShare, fmt(t["dense"]), fmt(t["own"]),
        med["dense"] / med["own"], (algo + detect) / med["own"] * 1e-3)
    if propagated:
        row += " %s | %.2fx | %.0f |" % (fmt(t["prop"]), med["dense"] / med["prop"], algo / med["prop"] * 1e-3)
    else:
        row += " - | - | - |"
    print(row, flush=True)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    assert torch.cuda.is_available(), "dw_target.py needs a GPU"
    print("# Change-based depthwise convolution at about 10 % changed input pixels (feedback mode, ReLU6)\n")
    print("%s, torch %s; times in us per call, median [min..max] over %d interleaved rounds of %d calls; GB/s: the "
          "frame's algorithmic bytes over its median time\n"
          % (torch.cuda.get_device_name(0), torch.__version__, reps, BATCH))
    print("| layer | map | dtype | changed input / listed output pixels | F.conv2d(groups=C) | own detection (2 launches) "
          "| dense / own | own GB/s | propagated (3 launches) | dense / propagated | propagated GB/s |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    with torch.no_grad():
        for spec in LAYERS:
            for dtype in (torch.float32, torch.float16):
                layer(*spec, dtype=dtype, reps=reps)


if __name__ == "__main__":
    main()
