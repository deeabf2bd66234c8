#!/usr/bin/env python3
"""Target of the change-based fused local attention (cb_attend.hip, cbinfer_cbattend_forward): fp32 and
fp16, 10 % changed pixels in BOTH operands in whole blocks, mask form and list form, on 80x120 --
  radius 3 and radius 4 at 64 and 128 channels with 2 and 4 heads,  a 13x13 NAT-type window with d = 32,
  the stereo range ((0, 0), (-40, 0)) --
against two baselines on the same tensors in the same process:
  (a) the hand-wired chain cbinfer_cbcorrelation_forward -> cbinfer_cbchanreduce_forward (softmax) ->
      cbinfer_cbaggregate_forward on the same change lists, where both compute the same function: border 'zero', ONE
      head, scale = 1/C (the module is timed in that setting too, next to the chain);
  (b) dense torch, the loop of shifted products (scores, softmax over the taps, weighted sum), masked as the module's
      default border is.
Before a row is timed the module's every-pixel result is checked against the float64 reference within the bound of
DESIGN 5.36 (tests/attend_cases.py holds both), and the chain against the same reference.  The measuring method is
tools/target_common.py's.  Prints markdown (profiles/attend_target.md).
usage: target_attend.py [rounds]"""
import ctypes
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
import attend_cases as ac  # noqa: E402
from cbinfer_amd import _lib  # noqa: E402
from cbinfer_amd._lib import C, check, ptr  # noqa: E402
from target_common import BATCH, SETS, change_sets, device_sets, dtype_name, fmt, listed_share, rounds  # noqa: E402

H, W, BLOCK = 80, 120, 8
#        name, channels (C = Cv), heads, displacement ((y0, y1), (x0, x1))
ROWS = [("radius %d, %d ch" % (r, c), c, h, ((-r, r), (-r, r))) for r in (3, 4) for c in (64, 128) for h in (2, 4)]
ROWS += [("NAT 13x13, d = 32", 128, 4, ((-6, 6), (-6, 6))), ("stereo range", 64, 2, ((0, 0), (-40, 0)))]


def row(name, Cn, heads, disp, dtype, reps):
    rng = np.random.default_rng(7)
    torch.manual_seed(7)
    (y0, y1), (x0, x1) = disp
    window = (y0, y1, x0, x1, y1 - y0 + 1, x1 - x0 + 1)
    taps = ac.taps(window, 1)
    T, d = len(taps), Cn // heads
    q = torch.randn(1, Cn, H, W, device="cuda").to(dtype)
    kv = torch.cat([torch.randn(1, Cn, H, W, device="cuda"), 2 * torch.randn(1, Cn, H, W, device="cuda")], 1).to(dtype)
    k, v = kv[:, :Cn], kv[:, Cn:]
    pads = (max(0, -x0), max(0, x1), max(0, -y0), max(0, y1))
    scale, scale1 = ac.default_scale(Cn, heads), float(np.float32(1.0) / np.float32(Cn))
    own = ctypes.pointer(_lib.Attend(y0, y1, x0, x1, 1, heads, _lib.ATTEND_MASK, 0, scale))
    one = ctypes.pointer(_lib.Attend(y0, y1, x0, x1, 1, 1, _lib.ATTEND_ZERO, 0, scale1))
    corr, aggr = ctypes.pointer(_lib.Corr(y0, y1, x0, x1, 1, 1)), ctypes.pointer(_lib.Aggr(y0, y1, x0, x1, 1, 1))
    assert C.cbinfer_attend_supported(own, Cn, Cn, H, W) and C.cbinfer_attend_supported(one, Cn, Cn, H, W)
    sets = change_sets(rng, H, W, BLOCK, 0.10)
    masks, lists = device_sets(sets)
    words = C.cbinfer_mask_words(H, W)
    # working masks (zero between frames) and mask copies: the module's, and one set per link of the chain
    kvb, bits, mcopy, b1, w1, c1, w2, c2, b3, w3, c3 = (torch.zeros(words, dtype=torch.int64, device="cuda")
                                                        for _ in range(11))
    out, out1, outc = (torch.empty(1, Cn, H, W, device="cuda", dtype=dtype) for _ in range(3))
    vol, prob = (torch.empty(1, T, H, W, device="cuda", dtype=dtype) for _ in range(2))
    st, dt = torch.cuda.current_stream().cuda_stream, _lib.dtype_code(q)

    def n(t):
        return t.numel() if t is not None else 0

    def frame(att, o, mq, lq, mk, lk):
        check(C.cbinfer_cbattend_forward(ptr(q), ptr(kv), None, ptr(o), ptr(mq), ptr(lq), n(lq), None, ptr(mk), ptr(lk),
                                         n(lk), None, ptr(kvb), ptr(bits), ptr(mcopy), Cn, Cn, H, W, att, dt, st))

    def chain(mq, lq, mk, lk):
        # (every link takes the mask its producer handed on, as the modules wire it)
        every = mq is None and lq is None
        check(C.cbinfer_cbcorrelation_forward(ptr(q), ptr(k), ptr(vol), ptr(mq), ptr(lq), n(lq), None, ptr(mk), ptr(lk),
                                              n(lk), None, ptr(b1), ptr(w1), ptr(c1), Cn, H, W, corr, dt, st))
        check(C.cbinfer_cbchanreduce_forward(ptr(vol), ptr(prob), None if every else ptr(c1), None, 0, None, ptr(w2),
                                             ptr(c2), T, H, W, _lib.CH_SOFTMAX, 0.0, None, None, dt, st))
        check(C.cbinfer_cbaggregate_forward(ptr(prob), ptr(v), ptr(outc), None if every else ptr(c2), None, 0, None,
                                            ptr(mk), ptr(lk), n(lk), None, ptr(b3), ptr(w3), ptr(c3), Cn, H, W, aggr,
                                            dt, st))

    def dense(i):
        # the loop of shifted products per head, a tap outside the map taking no part (the module's default border)
        kp, vp = F.pad(k, pads), F.pad(v, pads)
        inmap = F.pad(torch.ones(1, 1, H, W, device="cuda", dtype=dtype), pads)
        qh = q.view(heads, d, H, W)

        def win(t, dy, dx):
            return t[:, :, pads[2] + dy:pads[2] + dy + H, pads[0] + dx:pads[0] + dx + W]
        s = torch.stack([(qh * win(kp, dy, dx).view(heads, d, H, W)).sum(1) for dy, dx in taps], 1) * scale
        live = torch.cat([win(inmap, dy, dx) for dy, dx in taps], 1)
        p = torch.softmax(s.float().masked_fill(live == 0, float('-inf')), 1).to(dtype)
        acc = p[:, 0:1] * win(vp, *taps[0]).view(heads, d, H, W)
        for t in range(1, T):
            acc = acc + p[:, t:t + 1] * win(vp, *taps[t]).view(heads, d, H, W)
        return acc.view(1, Cn, H, W)

    # results first: every pixel listed, against the float64 reference within the bound of DESIGN 5.36
    f16 = dtype == torch.float16
    qn, kvn = q[0].cpu().numpy(), kv[0].cpu().numpy()
    frame(own, out, None, None, None, None)
    ref = ac.reference(qn, kvn, None, window, 1, heads, 'mask', scale)
    assert (np.abs(out[0].double().cpu().numpy() - ref['out']) <= ac.bound(ref, window, f16)).all(), "beyond its bound"
    assert np.allclose(dense(0)[0].double().cpu().numpy(), ref['out'], atol=2e-2), "dense torch"
    frame(one, out1, None, None, None, None)
    chain(None, None, None, None)
    ref1 = ac.reference(qn, kvn, None, window, 1, 1, 'zero', scale1)
    bar1 = ac.bound(ref1, window, f16)
    assert (np.abs(out1[0].double().cpu().numpy() - ref1['out']) <= bar1).all(), "one head beyond its bound"
    # (the chain rounds the volume and the weights to the dtype on the way: the module's bound and those roundings)
    slack = 2.0 ** -10 * (1.0 + ref1['A']) if f16 else 2.0 ** -20 * (1.0 + ref1['A'])
    assert (np.abs(outc[0].double().cpu().numpy() - ref1['out']) <= bar1 + slack).all(), "chain and module differ"
    t = rounds([("mask", lambda i: frame(own, out, masks[i % SETS], None, masks[i % SETS], None)),
                ("list", lambda i: frame(own, out, None, lists[i % SETS], None, lists[i % SETS])),
                ("one", lambda i: frame(one, out1, masks[i % SETS], None, masks[i % SETS], None)),
                ("chain", lambda i: chain(masks[i % SETS], None, masks[i % SETS], None)),
                ("dense", dense)], reps)
    frame(own, out, masks[0], None, masks[0], None)
    listed = float(np.unpackbits(mcopy.cpu().numpy().view(np.uint8)).sum()) / (H * W) * 100.0
    med = {key: statistics.median(t[key]) for key in t}
    ratios = (med["dense"] / med["mask"], med["dense"] / med["list"], med["chain"] / med["one"])
    # (a case where the module loses to a baseline is written in capitals, as in the other tables)
    verdict = "%.2fx / %.2fx / %.2fx" % ratios + (" LOSES" if min(ratios) < 1.0 else "")
    volume = 2 * T * H * W * (2 if f16 else 4)      # (the correlation volume and the softmax's, both kept as state)
    print("| %s, %d heads | %d taps | %s | %.1f %% / %.1f %% | %s | %s | %s | %s | %s | %d KiB | %s |"
          % (name, heads, T, dtype_name(dtype), listed_share(sets), listed, fmt(t["mask"]), fmt(t["list"]),
             fmt(t["dense"]), fmt(t["one"]), fmt(t["chain"]), volume // 1024, verdict), flush=True)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    assert torch.cuda.is_available(), "target_attend.py needs a GPU"
    print("# Change-based fused local attention at 10 % changed pixels in both operands, 80x120\n")
    print("%s, torch %s; times in us per frame, median [min..max] over %d interleaved rounds of %d calls\n"
          % (torch.cuda.get_device_name(0), torch.__version__, reps, BATCH))
    print("| layer | window | dtype | changed / listed pixels | cbinfer_cbattend_forward, mask form | list form | "
          "dense torch, shifted products | module, one head, border 'zero', scale 1/C, mask form | the chain correlate -> "
          "softmax -> aggregate, mask form | volume state the chain keeps | dense / mask form, dense / list form, "
          "chain / module |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for name, Cn, heads, disp in ROWS:
        for dtype in (torch.float32, torch.float16):
            row(name, Cn, heads, disp, dtype, reps)


if __name__ == "__main__":
    main()
