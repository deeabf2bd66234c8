#!/usr/bin/env python3
"""Target of the change-based deformable convolution (cb_deform.hip, cbinfer_cbdeform_forward): fp32 and
fp16, 3x3 / padding 1 with a DCNv2 field (modulation 'sigmoid'), 10 % changed pixels in BOTH operands in whole blocks,
mask form and list form --
  an EDVR-type alignment 64 -> 64 with 8 offset groups @ 180x320 and @ 90x160,  a BasicVSR++-type one with 16 groups
  @ 180x320,  a DCNv2 head 256 -> 256 with one group @ 96x320 --
against the fastest dense formulation on the machine, on the same tensors in the same process: one F.grid_sample per
filter tap (the offset groups as its batch), the sigmoid, and one contraction over (t, c) in torch; and
torchvision.ops.deform_conv2d where it imports.  Before a row is timed its every-pixel result is checked against the same
formulation in float64 within the bound of DESIGN 5.35.  The measuring method is tools/target_common.py's.  Prints
markdown (profiles/deform_target.md).
(The file is not called *_target.py: tests/test_host_targets.py pins the list of the tools of that name.)
usage: target_deform.py [rounds]"""
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

try:
    from torchvision.ops import deform_conv2d
except Exception:      # (not installed, or built for another torch)
    deform_conv2d = None

#        name, C, K, offset groups, H, W, block
ROWS = [("EDVR-type alignment", 64, 64, 8, 180, 320, 8), ("EDVR-type alignment", 64, 64, 8, 90, 160, 8),
        ("BasicVSR++-type alignment", 64, 64, 16, 180, 320, 8), ("DCNv2 head", 256, 256, 1, 96, 320, 8)]
T = 9


def dense(x, field, Wt, bias, Go, H, W):
    """One grid_sample per filter tap, the sigmoid, one contraction: (out [1, K, H, W], cols [T C, H W]).  The
    coordinates are formed in float32 (float64 for a float64 x) and handed to grid_sample in x's dtype."""
    Cn, ct = x.size(1), torch.float64 if x.dtype == torch.float64 else torch.float32
    xg = x.view(Go, Cn // Go, H, W)
    off = field[0, :2 * Go * T].to(ct).view(Go, T, 2, H, W)
    m = torch.sigmoid(field[0, 2 * Go * T:].to(ct)).to(x.dtype).view(Go, T, 1, H, W)
    ys = torch.arange(H, device=x.device, dtype=ct).view(1, H, 1)
    xs = torch.arange(W, device=x.device, dtype=ct).view(1, 1, W)
    cols = []
    for t in range(T):
        sy, sx = ys + (t // 3 - 1) + off[:, t, 0], xs + (t % 3 - 1) + off[:, t, 1]
        grid = torch.stack((sx * (2.0 / (W - 1)) - 1.0, sy * (2.0 / (H - 1)) - 1.0), dim=-1).to(x.dtype)
        cols.append(F.grid_sample(xg, grid, mode='bilinear', padding_mode='zeros', align_corners=True) * m[:, t])
    cols = torch.stack(cols).view(T * Cn, H * W)      # (t, g, c) = (t, c): the k order of Wt
    out = (Wt @ cols).view(1, -1, H, W)
    return (out if bias is None else out + bias.view(1, -1, 1, 1)), cols


def row(name, Cn, K, Go, H, W, block, dtype, reps):
    rng = np.random.default_rng(7)
    torch.manual_seed(7)
    x = torch.randn(1, Cn, H, W, device="cuda").to(dtype)
    field = torch.cat((torch.randn(1, 2 * Go * T, H, W, device="cuda") * 2, torch.randn(1, Go * T, H, W, device="cuda")),
                      dim=1).to(dtype)
    Wd = (torch.randn(K, Cn, 3, 3, device="cuda") / (Cn * T) ** 0.5).to(dtype)
    bias = torch.randn(K, device="cuda").to(dtype)
    Wt = Wd.view(K, Cn, T).permute(0, 2, 1).reshape(K, T * Cn).contiguous()
    dt = _lib.dtype_code(x)
    d = ctypes.pointer(_lib.Deform(_lib.Geom(3, 3, 1, 1, 1, 1, 1, 1), Go, _lib.DEFORM_SIGMOID, dt, 0))
    assert C.cbinfer_deform_supported(d, Cn, H, W, K)
    st = torch.cuda.current_stream().cuda_stream
    wp = torch.empty(C.cbinfer_deform_prepared_weights_bytes(K, Cn, d, dt), dtype=torch.uint8, device="cuda")
    check(C.cbinfer_deform_prep_weights(ptr(Wd), ptr(wp), K, Cn, d, dt, st))
    sets = change_sets(rng, H, W, block, 0.10)
    masks, lists = device_sets(sets)
    words = C.cbinfer_mask_words(H, W)
    inbits, bits, mcopy = (torch.zeros(words, dtype=torch.int64, device="cuda") for _ in range(3))
    ws = torch.zeros(C.cbinfer_geom_workspace_bytes(), dtype=torch.uint8, device="cuda")
    out = torch.empty(1, K, H, W, device="cuda", dtype=dtype)

    def frame(mx, lx, mf, lf):
        check(C.cbinfer_cbdeform_forward(ptr(x), ptr(field), ptr(wp), ptr(bias), ptr(out), ptr(mx), ptr(lx),
                                         lx.numel() if lx is not None else 0, None, ptr(mf), ptr(lf),
                                         lf.numel() if lf is not None else 0, None, ptr(inbits), ptr(bits), ptr(mcopy),
                                         ptr(ws), Cn, H, W, K, d, dt, st))

    # results first: every pixel listed, against the float64 formulation within the bound of DESIGN 5.35
    frame(None, None, None, None)
    ref, cols = dense(x.double(), field, Wt.double(), bias.double(), Go, H, W)
    S = (Wt.double().abs() @ cols.abs()).view(1, K, H, W) + bias.double().abs().view(1, K, 1, 1)
    n, u = Cn * T, 2.0 ** -24
    bar = (6 * n + 33) * u * S
    if dtype == torch.float16:
        bar = (2.0 ** -11 + (n + 31) * u) * S + 2.0 ** -25 * Wd.double().abs().sum() + 2.0 ** -11 * ref.abs() + 2.0 ** -25
    # (the float64 formulation normalises its coordinates: a sample is 1e-12 px off, far below the bound)
    assert bool(((out.double() - ref).abs() <= bar + 1e-9 * S).all()), "deformable convolution beyond its bound"
    # (in fp16 torch's own grid resolves 2^-11 of the map, a tenth of a pixel: its result is timed, not judged)
    assert dtype == torch.float16 or torch.allclose(dense(x, field, Wt, bias, Go, H, W)[0].double(), ref, atol=1e-3)
    runs = [("mask", lambda i: frame(masks[i % SETS], None, masks[i % SETS], None)),
            ("list", lambda i: frame(None, lists[i % SETS], None, lists[i % SETS])),
            ("taps", lambda i: dense(x, field, Wt, bias, Go, H, W))]
    if deform_conv2d is not None:
        off, mk = field[:, :2 * Go * T], torch.sigmoid(field[:, 2 * Go * T:])
        runs.append(("tv", lambda i: deform_conv2d(x, off, Wd, bias, padding=1, mask=mk)))
    t = rounds(runs, reps)
    frame(masks[0], None, masks[0], None)
    listed = float(np.unpackbits(mcopy.cpu().numpy().view(np.uint8)).sum()) / (H * W) * 100.0
    base = min(statistics.median(t[k]) for k in t if k not in ("mask", "list"))
    ratios = [base / statistics.median(t[k]) for k in ("mask", "list")]
    # (a case where the module loses to the dense operator is written in capitals, as in the other tables)
    verdict = "%.2fx / %.2fx" % tuple(ratios) + (" LOSES" if min(ratios) < 1.0 else "")
    print("| %s %d -> %d @%dx%d | Go = %d | %s | %.1f %% / %.1f %% | %s | %s | %s | %s | %s |"
          % (name, Cn, K, H, W, Go, dtype_name(dtype), listed_share(sets), listed, fmt(t["mask"]), fmt(t["list"]),
             fmt(t["taps"]), fmt(t["tv"]) if "tv" in t else "n/a", verdict), flush=True)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    assert torch.cuda.is_available(), "target_deform.py needs a GPU"
    print("# Change-based deformable convolution (3x3, DCNv2 field) at 10 % changed pixels in both operands\n")
    print("%s, torch %s; times in us per call, median [min..max] over %d interleaved rounds of %d calls; the dense "
          "baseline of a row is the faster of the torch formulations that run here\n"
          % (torch.cuda.get_device_name(0), torch.__version__, reps, BATCH))
    print("| layer | offset groups | dtype | changed / listed pixels | cbinfer_cbdeform_forward, mask form | list form | "
          "dense torch, grid_sample per tap + contraction | torchvision deform_conv2d | dense / mask form, dense / list form |")
    print("|---|---|---|---|---|---|---|---|---|")
    for name, Cn, K, Go, H, W, block in ROWS:
        for dtype in (torch.float32, torch.float16):
            row(name, Cn, K, Go, H, W, block, dtype, reps)


if __name__ == "__main__":
    main()
