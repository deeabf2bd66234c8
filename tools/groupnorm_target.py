#!/usr/bin/env python3
"""Target of the change-based group norm (cb_groupnorm.hip): fp32 and fp16, about 10 % changed pixels per frame in whole
blocks, on three norms --
  GroupNorm(32, 256) @80x120 (a detection head)    InstanceNorm2d(64) @96x320 (a monodepth-type decoder)
  GroupNorm(1, 64) @320x480 (a ConvNeXt-type stem: launch 2 is ONE workgroup over 2 x 64 x 320 x 8 partials, 2.6 MB).
Per norm and dtype the frame -- ONE cbinfer_cbgroupnorm_forward with the affine and the ReLU: three launches, four with the
operand in LIST form -- at a threshold at which no group trips (100) and at one at which every group whose statistics moved
trips (0), the operand in mask form and in list form, against torch's dense F.group_norm + relu on the same frames in the
same process.  Frame i is a base frame with fresh values on change set i, so it differs from frame i - 1 on two sets of
5 % each; the mask / the list says so.  The measuring method is tools/target_common.py's; every call of a batch takes the
next of 16 frames.  Prints markdown (profiles/groupnorm_target.md).
usage: groupnorm_target.py [rounds]"""
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
from target_common import BATCH, SETS, change_sets, dtype_name, fmt, listed_share, pack, rounds  # noqa: E402

#        name, channels, groups, H, W, block
NORMS = [("GroupNorm(32, 256)", 256, 32, 80, 120, 4), ("InstanceNorm2d(64)", 64, 64, 96, 320, 4),
         ("GroupNorm(1, 64)", 64, 1, 320, 480, 8)]
EPS = 1e-5


class Norm(object):
    """The buffers and the library call of one change-based group norm at one threshold."""

    def __init__(self, Cn, G, H, W, dtype, gamma, beta, threshold):
        dev = "cuda"
        self.shape, self.G, self.threshold = (Cn, H, W), G, threshold
        self.code = _lib.dtype_code(torch.empty(0, dtype=dtype))
        self.gamma, self.beta = gamma, beta
        self.out = torch.empty(1, Cn, H, W, dtype=dtype, device=dev)
        self.partials = torch.zeros(2, Cn, H, (W + 63) // 64, dtype=torch.float64, device=dev)
        self.stats, self.held = (torch.zeros(2, G, dtype=torch.float32, device=dev) for _ in range(2))
        self.tripped = torch.zeros(G, dtype=torch.int32, device=dev)
        words = C.cbinfer_mask_words(H, W)
        self.bits, self.copy = (torch.zeros(words, dtype=torch.int64, device=dev) for _ in range(2))
        self.eps = (ctypes.c_double * 1)(EPS)
        self.st = torch.cuda.current_stream().cuda_stream

    def frame(self, x, mask=None, lst=None, fresh=False):
        Cn, H, W = self.shape
        check(C.cbinfer_cbgroupnorm_forward(ptr(x), ptr(self.gamma), ptr(self.beta), ptr(self.out), ptr(self.partials),
                                            ptr(self.stats), ptr(self.held), ptr(self.tripped), ptr(mask), ptr(lst),
                                            lst.numel() if lst is not None else 0, None, ptr(self.bits), ptr(self.copy),
                                            Cn, self.G, H, W, self.eps, 1, self.threshold, int(fresh), self.code, self.st))


def norm(name, Cn, G, H, W, blk, dtype, reps):
    rng = np.random.default_rng(7)
    torch.manual_seed(7)
    sets = change_sets(rng, H, W, blk, 0.05)
    base = torch.randn(1, Cn, H, W, device="cuda")
    frames, masks, lists = [], [], []
    for i, m in enumerate(sets):      # frame i differs from frame i - 1 on set i and set i - 1
        f = base.clone()
        f[0][:, torch.from_numpy(m).cuda()] = torch.randn(Cn, int(m.sum()), device="cuda")
        frames.append(f.to(dtype))
        both = m | sets[i - 1]
        masks.append(torch.from_numpy(pack(both)).cuda())
        lists.append(torch.from_numpy(np.flatnonzero(both.reshape(-1)).astype(np.int32)).cuda())
    gamma = torch.rand(Cn, device="cuda") + 0.5
    beta = torch.randn(Cn, device="cuda") * 0.1
    tg, tb = gamma.to(dtype), beta.to(dtype)
    gamma, beta = tg.float(), tb.float()      # (the same values)

    def dense(i):
        return torch.relu(F.group_norm(frames[i % SETS], G, tg, tb, EPS))

    runs = {(th, form): Norm(Cn, G, H, W, dtype, gamma, beta, th) for th in (100.0, 0.0) for form in ("mask", "list")}
    for n in runs.values():
        n.frame(frames[SETS - 1], fresh=True)

    def call(n, form, i):
        if form == "mask":
            n.frame(frames[i % SETS], mask=masks[i % SETS])
        else:
            n.frame(frames[i % SETS], lst=lists[i % SETS])
    # results first: at threshold 0 every frame is the dense operator (within the rounding of the dtype), in both forms;
    # at threshold 100 no group trips
    tripped = []
    for i in range(SETS):
        for (th, form), n in runs.items():
            call(n, form, i)
        tripped.append(int(runs[(0.0, "mask")].tripped.sum().item()))
        assert int(runs[(100.0, "mask")].tripped.sum().item()) == 0, "a group tripped at threshold 100"
        want = dense(i)
        tol = 1e-5 if dtype == torch.float32 else 4e-3
        for form in ("mask", "list"):
            assert torch.allclose(runs[(0.0, form)].out.float(), want.float(), rtol=tol, atol=tol), "differs from dense"
    t = rounds([((th, form), lambda i, n=n, form=form: call(n, form, i)) for (th, form), n in runs.items()] +
               [("dense", dense)], reps)
    changed = listed_share([m | sets[i - 1] for i, m in enumerate(sets)])
    med = {k: statistics.median(v) for k, v in t.items()}
    print("| %s @%dx%d | %s | %.1f %% | %s | %s | %s (%.0f of %d tripped) | %s | %s | %.2fx / %.2fx | %.2fx / %.2fx |"
          % (name, H, W, dtype_name(dtype), changed, fmt(t[(100.0, "mask")]), fmt(t[(100.0, "list")]),
             fmt(t[(0.0, "mask")]), statistics.mean(tripped), G, fmt(t[(0.0, "list")]), fmt(t["dense"]),
             med["dense"] / med[(100.0, "mask")], med["dense"] / med[(100.0, "list")], med["dense"] / med[(0.0, "mask")],
             med["dense"] / med[(0.0, "list")]))


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    assert torch.cuda.is_available(), "groupnorm_target.py needs a GPU"
    print("# Change-based group norm at about 10 % changed pixels\n")
    print("%s, torch %s; times in us per frame, median [min..max] over %d interleaved rounds of %d frames\n"
          % (torch.cuda.get_device_name(0), torch.__version__, reps, BATCH))
    print("| norm (affine, + ReLU) | dtype | changed pixels | no group trips (threshold 100), mask | ... list "
          "| threshold 0, mask | ... list | dense F.group_norm + relu | dense / no trip: mask, list "
          "| dense / threshold 0: mask, list |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    with torch.no_grad():
        for spec in NORMS:
            for dtype in (torch.float32, torch.float16):
                norm(*spec, dtype=dtype, reps=reps)


if __name__ == "__main__":
    main()
