#!/usr/bin/env python3
"""Target of the change-based partitioned window attention (cb_winattend.hip, cbinfer_cbwinattend_forward):
fp32 and fp16, 10 % changed pixels in BOTH operands in whole 8x8 blocks, mask form and list form, on 80x120 --
  a SwinIR-type layer (8x8, 180 channels, 6 heads), Swin-type layers (7x7, 96 channels / 3 heads and 192 / 6), 12x12 with
  128 channels / 4 heads, each unshifted and shifted by half a window --
against two baselines on the same tensors in the same process:
  (a) dense torch, Swin's formulation: pad to whole windows, roll, window partition, scaled_dot_product_attention with the
      additive region mask (the padding a region of its own), window reverse, roll back, crop;
  (b) the sliding-window mode cbinfer_cbattend_forward at the window of equal tap count (another function: every change
      is smeared over the window's radius).
Before a row is timed the every-pixel result is checked against the float64 reference within the bound of DESIGN 5.37
(tests/winattend_cases.py holds both), and dense torch against the same reference.  The measuring method is
tools/target_common.py's.  Prints markdown (profiles/winattend_target.md).
usage: target_winattend.py [rounds]"""
import ctypes
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
import winattend_cases as wc  # noqa: E402
from cbinfer_amd import _lib  # noqa: E402
from cbinfer_amd._lib import C, check, ptr  # noqa: E402
from target_common import BATCH, SETS, change_sets, device_sets, dtype_name, fmt, listed_share, rounds  # noqa: E402

H, W, BLOCK = 80, 120, 8
#        name, partition, channels (C = Cv), heads
ROWS = [("SwinIR-type", 8, 180, 6), ("Swin-type", 7, 96, 3), ("Swin-type", 7, 192, 6), ("Large-window", 12, 128, 4)]


def row(name, P, Cn, heads, shift, dtype, reps):
    rng = np.random.default_rng(7)
    torch.manual_seed(7)
    d, scale = Cn // heads, wc.default_scale(Cn, heads)
    q = torch.randn(1, Cn, H, W, device="cuda").to(dtype)
    kv = torch.cat([torch.randn(1, Cn, H, W, device="cuda"), 2 * torch.randn(1, Cn, H, W, device="cuda")], 1).to(dtype)
    own = ctypes.pointer(_lib.WinAttend(P, P, shift, shift, heads, 0, scale))
    lo = -(P // 2)      # the sliding window of P x P taps
    slide = ctypes.pointer(_lib.Attend(lo, lo + P - 1, lo, lo + P - 1, 1, heads, _lib.ATTEND_MASK, 0, scale))
    assert C.cbinfer_winattend_supported(own, Cn, Cn, H, W) and C.cbinfer_attend_supported(slide, Cn, Cn, H, W)
    sets = change_sets(rng, H, W, BLOCK, 0.10)
    masks, lists = device_sets(sets)
    words = C.cbinfer_mask_words(H, W)
    kvb, bits, mcopy, kvb2, bits2, mcopy2 = (torch.zeros(words, dtype=torch.int64, device="cuda") for _ in range(6))
    out, outs = (torch.empty(1, Cn, H, W, device="cuda", dtype=dtype) for _ in range(2))
    st, dt = torch.cuda.current_stream().cuda_stream, _lib.dtype_code(q)

    def n(t):
        return t.numel() if t is not None else 0

    def frame(mq, lq, mk, lk):
        check(C.cbinfer_cbwinattend_forward(ptr(q), ptr(kv), None, ptr(out), ptr(mq), ptr(lq), n(lq), None, ptr(mk),
                                            ptr(lk), n(lk), None, ptr(kvb), ptr(bits), ptr(mcopy), Cn, Cn, H, W, own, dt, st))

    def sliding(mq, mk):
        check(C.cbinfer_cbattend_forward(ptr(q), ptr(kv), None, ptr(outs), ptr(mq), None, 0, None, ptr(mk), None, 0, None,
                                         ptr(kvb2), ptr(bits2), ptr(mcopy2), Cn, Cn, H, W, slide, dt, st))

    # dense torch: the padded, rolled map's regions (three bands per axis, the padding a region of its own) as SDPA's mask
    Hp, Wp = -(-H // P) * P, -(-W // P) * P
    nwin = (Hp // P) * (Wp // P)

    def windows(x):      # [1, C, Hp, Wp] -> [windows, heads, tokens, C / heads]
        x = x.reshape(heads, -1, Hp // P, P, Wp // P, P).permute(2, 4, 0, 3, 5, 1)
        return x.reshape(nwin, heads, P * P, -1)
    region = torch.full((1, 1, Hp, Wp), -1.0, device="cuda")
    cells = wc.cells((P, P), (shift, shift), (H, W))
    for i, ((y0, y1), (x0, x1)) in enumerate(cells):
        region[:, :, y0:y1, x0:x1] = i
    region = windows(torch.roll(region, (-shift, -shift), (2, 3)).expand(1, heads, Hp, Wp))[:, :1, :, 0]
    allow = (region[:, :, :, None] == region[:, :, None, :])
    addmask = torch.zeros(allow.shape, device="cuda", dtype=dtype).masked_fill(~allow, float('-inf'))

    def dense(i):
        def cut(x):
            return windows(torch.roll(F.pad(x, (0, Wp - W, 0, Hp - H)), (-shift, -shift), (2, 3)))
        o = F.scaled_dot_product_attention(cut(q), cut(kv[:, :Cn]), cut(kv[:, Cn:]), attn_mask=addmask, scale=scale)
        o = o.reshape(Hp // P, Wp // P, heads, P, P, d).permute(2, 5, 0, 3, 1, 4).reshape(1, Cn, Hp, Wp)
        return torch.roll(o, (shift, shift), (2, 3))[:, :, :H, :W]

    # results first: every pixel listed, against the float64 reference within the bound of DESIGN 5.37
    frame(None, None, None, None)
    ref = wc.reference(q[0].cpu().numpy(), kv[0].cpu().numpy(), None, (P, P), (shift, shift), heads, scale)
    err = np.abs(out[0].double().cpu().numpy() - ref['out'])
    assert (err <= wc.bound(ref, dtype == torch.float16)).all(), "beyond its bound"
    assert np.allclose(dense(0)[0].double().cpu().numpy(), ref['out'], atol=2e-2), "dense torch"
    t = rounds([("mask", lambda i: frame(masks[i % SETS], None, masks[i % SETS], None)),
                ("list", lambda i: frame(None, lists[i % SETS], None, lists[i % SETS])),
                ("slide", lambda i: sliding(masks[i % SETS], masks[i % SETS])),
                ("dense", dense)], reps)
    frame(masks[0], None, masks[0], None)
    listed = float(np.unpackbits(mcopy.cpu().numpy().view(np.uint8)).sum()) / (H * W) * 100.0
    sliding(masks[0], masks[0])
    smeared = float(np.unpackbits(mcopy2.cpu().numpy().view(np.uint8)).sum()) / (H * W) * 100.0
    med = {key: statistics.median(t[key]) for key in t}
    ratios = (med["dense"] / med["mask"], med["dense"] / med["list"], med["slide"] / med["mask"])
    # (a case where the module loses to a baseline is written in capitals, as in the other tables)
    verdict = "%.2fx / %.2fx / %.2fx" % ratios + (" LOSES" if min(ratios) < 1.0 else "")
    print("| %s %dx%d, %d ch, %d heads, shift %d | %s | %.1f %% / %.1f %% / %.1f %% | %s | %s | %s | %s | %s |"
          % (name, P, P, Cn, heads, shift, dtype_name(dtype), listed_share(sets), listed, smeared, fmt(t["mask"]),
             fmt(t["list"]), fmt(t["dense"]), fmt(t["slide"]), verdict), flush=True)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    assert torch.cuda.is_available(), "target_winattend.py needs a GPU"
    print("# Change-based partitioned window attention at 10 % changed pixels in both operands, 80x120\n")
    print("%s, torch %s; times in us per frame, median [min..max] over %d interleaved rounds of %d calls\n"
          % (torch.cuda.get_device_name(0), torch.__version__, reps, BATCH))
    print("| layer | dtype | changed / listed / listed by the sliding window | cbinfer_cbwinattend_forward, mask form | list "
          "form | dense torch (roll, partition, SDPA, reverse) | sliding cbinfer_cbattend_forward, equal taps, mask form | "
          "dense / mask form, dense / list form, sliding / mask form |")
    print("|---|---|---|---|---|---|---|---|")
    for name, P, Cn, heads in ROWS:
        for shift in (0, P // 2):
            for dtype in (torch.float32, torch.float16):
                row(name, P, Cn, heads, shift, dtype, reps)


if __name__ == "__main__":
    main()
