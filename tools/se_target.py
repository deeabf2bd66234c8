#!/usr/bin/env python3
"""Target of the change-based squeeze-and-excitation block (cb_chanscale.hip behind cb_adaptpool.hip): fp32 and fp16, about
10 % changed pixels per frame in whole blocks, on three blocks --
  MobileNetV3-type   C 96,  R 24, 40x60      EfficientNet-type   C 144, R 6, 80x120      SE-ResNet-type   C 256, R 16, 80x120.
Per block and dtype the frame of library calls -- cbinfer_cbadaptivepool2d_forward (the squeeze: two launches) and
cbinfer_cbchanscale_forward (the fused excitation and the scale: two launches), the operand in MASK form -- at a threshold at
which no channel trips (2: a sigmoid gate cannot move that far) and at one at which every channel that moved trips (0),
against torch's dense block on the same frames in the same process: adaptive_avg_pool2d, two 1x1 convolutions, ReLU,
sigmoid, multiply.  Frame i is a base frame with fresh values on change set i, so it differs from frame i - 1 on two sets
of 5 % each; the mask says so.  The measuring method is tools/target_common.py's; every call of a batch takes the next
of 16 frames.  Prints markdown (profiles/se_target.md).
usage: se_target.py [rounds]"""
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cbinfer_amd import _lib  # noqa: E402
from cbinfer_amd._lib import C, check, ptr  # noqa: E402
from target_common import BATCH, SETS, change_sets, dtype_name, fmt, listed_share, pack, rounds  # noqa: E402

#          name, channels, hidden, H, W, block
BLOCKS = [("MobileNetV3-type", 96, 24, 40, 60, 2), ("EfficientNet-type", 144, 6, 80, 120, 4),
          ("SE-ResNet-type", 256, 16, 80, 120, 4)]


class Block(object):
    """The buffers and the two library calls of one change-based SE block at one threshold."""

    def __init__(self, Cn, R, H, W, dtype, w1, b1, w2, b2, threshold):
        dev = "cuda"
        self.shape, self.R, self.threshold, self.code = (Cn, H, W), R, threshold, _lib.dtype_code(torch.empty(0, dtype=dtype))
        self.w = (w1, b1, w2, b2)
        self.z = torch.empty(1, Cn, 1, 1, dtype=dtype, device=dev)
        self.partials = torch.empty(Cn, 1, H, dtype=torch.float32, device=dev)
        self.out = torch.empty(1, Cn, H, W, dtype=dtype, device=dev)
        self.gate, self.held = (torch.zeros(Cn, dtype=torch.float32, device=dev) for _ in range(2))
        self.tripped = torch.zeros((Cn + 63) // 64, dtype=torch.int64, device=dev)
        self.count = torch.zeros(1, dtype=torch.int32, device=dev)
        words = C.cbinfer_mask_words(H, W)
        self.inBits, self.bits, self.copy = (torch.zeros(words, dtype=torch.int64, device=dev) for _ in range(3))
        self.pbits, self.pcopy = (torch.zeros(1, dtype=torch.int64, device=dev) for _ in range(2))
        self.st = torch.cuda.current_stream().cuda_stream

    def frame(self, x, mask, fresh=False):
        Cn, H, W = self.shape
        m = None if fresh else ptr(mask)
        check(C.cbinfer_cbadaptivepool2d_forward(ptr(x), ptr(self.partials), ptr(self.z), m, None, 0, None, ptr(self.inBits),
                                                 ptr(self.pbits), ptr(self.pcopy), Cn, H, W, 1, 1, _lib.ADAPT_AVG, self.code,
                                                 self.st))
        w1, b1, w2, b2 = self.w
        check(C.cbinfer_cbchanscale_forward(ptr(x), ptr(self.z), ptr(w1), ptr(b1), ptr(w2), ptr(b2), ptr(self.out),
                                            ptr(self.gate), ptr(self.held), ptr(self.tripped), ptr(self.count), m, None, 0,
                                            None, ptr(self.bits), ptr(self.copy), Cn, self.R, H, W, _lib.CS_GATE_SIGMOID,
                                            _lib.CS_ACT_RELU, self.threshold, int(fresh), self.code, self.st))


def block(name, Cn, R, H, W, blk, dtype, reps):
    rng = np.random.default_rng(7)
    torch.manual_seed(7)
    sets = change_sets(rng, H, W, blk, 0.05)
    base = torch.randn(1, Cn, H, W, device="cuda")
    frames, masks = [], []
    for i, m in enumerate(sets):      # frame i differs from frame i - 1 on set i and set i - 1
        f = base.clone()
        f[0][:, torch.from_numpy(m).cuda()] = torch.randn(Cn, int(m.sum()), device="cuda")
        frames.append(f.to(dtype))
        masks.append(torch.from_numpy(pack(m | sets[i - 1])).cuda())
    w1 = torch.randn(R, Cn, device="cuda") / Cn ** 0.5
    w2 = torch.randn(Cn, R, device="cuda") * (2.0 / R ** 0.5)
    b1, b2 = torch.randn(R, device="cuda") * 0.1, torch.randn(Cn, device="cuda") * 0.1
    tw1, tb1, tw2, tb2 = w1.reshape(R, Cn, 1, 1).to(dtype), b1.to(dtype), w2.reshape(Cn, R, 1, 1).to(dtype), b2.to(dtype)
    w1, w2 = tw1.float().reshape(R, Cn).contiguous(), tw2.float().reshape(Cn, R).contiguous()      # (the same values)
    b1, b2 = tb1.float(), tb2.float()

    def dense(i):
        x = frames[i % SETS]
        z = F.adaptive_avg_pool2d(x, 1)
        return x * torch.sigmoid(F.conv2d(torch.relu(F.conv2d(z, tw1, tb1)), tw2, tb2))

    hold, trip = (Block(Cn, R, H, W, dtype, w1, b1, w2, b2, th) for th in (2.0, 0.0))
    for b in (hold, trip):
        b.frame(frames[SETS - 1], None, fresh=True)
    # results first: at threshold 0 every frame is the dense block (within the rounding of the dtype)
    tripped = []
    for i in range(SETS):
        trip.frame(frames[i], masks[i])
        hold.frame(frames[i], masks[i])
        tripped.append(int(trip.count.item()))
        assert int(hold.count.item()) == 0, "a channel tripped at threshold 2"
        want = dense(i)
        tol = 1e-5 if dtype == torch.float32 else 4e-3
        assert torch.allclose(trip.out.float(), want.float(), rtol=tol, atol=tol), "the block differs from the dense one"
    t = rounds([("hold", lambda i: hold.frame(frames[i % SETS], masks[i % SETS])),
                ("trip", lambda i: trip.frame(frames[i % SETS], masks[i % SETS])), ("dense", dense)], reps)
    changed = listed_share([m | sets[i - 1] for i, m in enumerate(sets)])
    med = {k: statistics.median(v) for k, v in t.items()}
    print("| %s C %d R %d @%dx%d | %s | %.1f %% | %s | %s (%.0f of %d tripped) | %s | %.2fx / %.2fx |"
          % (name, Cn, R, H, W, dtype_name(dtype), changed, fmt(t["hold"]), fmt(t["trip"]), statistics.mean(tripped), Cn,
             fmt(t["dense"]), med["dense"] / med["hold"], med["dense"] / med["trip"]))


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    assert torch.cuda.is_available(), "se_target.py needs a GPU"
    print("# Change-based squeeze-and-excitation block at about 10 % changed pixels\n")
    print("%s, torch %s; times in us per frame, median [min..max] over %d interleaved rounds of %d frames\n"
          % (torch.cuda.get_device_name(0), torch.__version__, reps, BATCH))
    print("| block | dtype | changed pixels | pool + scale, no channel trips (threshold 2) | pool + scale, threshold 0 "
          "| dense torch block | dense / no trip, dense / threshold 0 |")
    print("|---|---|---|---|---|---|---|")
    with torch.no_grad():
        for spec in BLOCKS:
            for dtype in (torch.float32, torch.float16):
                block(*spec, dtype=dtype, reps=reps)


if __name__ == "__main__":
    main()
