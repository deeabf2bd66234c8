#!/usr/bin/env python3
"""Target of the change-based rearrangements (cb_rearrange.hip): per operator, fp32 and fp16, 10 % and 100 % changed INPUT
pixels per frame in whole blocks --
  pixel shuffle x2     256 ch @160x240 -> 64 ch @320x480   (blocks of 4x4 input pixels),
  pixel unshuffle x2   64 ch @320x480 -> 256 ch @160x240   (blocks of 8x8 input pixels),
  channel shuffle      240 ch, 3 groups @40x60             (blocks of 2x2 pixels).
Three columns: cbinfer_cbrearrange_forward with the input in MASK form (one launch); torch's dense operator on the same
device tensor (made contiguous, as a consumer needs it); and cbinfer_cbupsample_forward, nearest, writing the SAME output
shape from the same footprint (x2 from the low resolution for the shuffle, x1 otherwise) -- the yardstick of a word walk
with the same store traffic.  Nothing gates on these times.
The measuring method is tools/target_common.py's.  Prints markdown (profiles/rearrange_target.md).
usage: rearrange_target.py [rounds]"""
import ctypes
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
from target_common import BATCH, SETS, change_sets, dtype_name, fmt, listed_share, pack, rounds  # noqa: E402

#        name, kind, factor, input (C, H, W), block (input pixels)
CASES = [("pixel shuffle x2", _lib.REARRANGE_SHUFFLE, 2, (256, 160, 240), 4),
         ("pixel unshuffle x2", _lib.REARRANGE_UNSHUFFLE, 2, (64, 320, 480), 8),
         ("channel shuffle, 3 groups", _lib.REARRANGE_CHANNELS, 3, (240, 40, 60), 2)]


def dense_op(kind, f, x):
    if kind == _lib.REARRANGE_SHUFFLE:
        return F.pixel_shuffle(x, f).contiguous()
    if kind == _lib.REARRANGE_UNSHUFFLE:
        return F.pixel_unshuffle(x, f).contiguous()
    return F.channel_shuffle(x, f).contiguous()


def case(name, kind, f, shape, block, dtype, share, reps):
    rng = np.random.default_rng(7)
    Cn, H, W = shape
    co, ho, wo = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    r = ctypes.pointer(_lib.Rearrange(kind, f))
    check(C.cbinfer_rearrange_out_shape(r, Cn, H, W, ctypes.byref(co), ctypes.byref(ho), ctypes.byref(wo)))
    Co, Ho, Wo = co.value, ho.value, wo.value
    x = torch.randn(1, Cn, H, W, device="cuda").to(dtype)
    sets = change_sets(rng, H, W, block, share)
    inMasks = [torch.from_numpy(pack(m)).cuda() for m in sets]
    words = C.cbinfer_mask_words(Ho, Wo)
    st = torch.cuda.current_stream().cuda_stream
    dt = _lib.dtype_code(x)
    out = torch.empty(1, Co, Ho, Wo, device="cuda", dtype=dtype)
    bits, mcopy = (torch.zeros(words, dtype=torch.int64, device="cuda") for _ in range(2))

    def cb(i, mask=True):
        check(C.cbinfer_cbrearrange_forward(ptr(x), ptr(out), ptr(inMasks[i % SETS]) if mask else None, None, 0, None,
                                            ptr(bits), ptr(mcopy), Cn, H, W, r, dt, st))

    def dense(i):
        return dense_op(kind, f, x)

    # the yardstick: nearest upsampling to the same [Co, Ho, Wo] output from the same footprint
    s = f if kind == _lib.REARRANGE_SHUFFLE else 1
    up = ctypes.pointer(_lib.Upsample(s, s, _lib.UPSAMPLE_NEAREST, 0))
    ux = torch.randn(1, Co, Ho // s, Wo // s, device="cuda").to(dtype)
    if kind == _lib.REARRANGE_UNSHUFFLE:
        upMasks = [torch.from_numpy(pack(m.reshape(Ho, f, Wo, f).any((1, 3)))).cuda() for m in sets]
    else:
        upMasks = inMasks
    uout = torch.empty(1, Co, Ho, Wo, device="cuda", dtype=dtype)
    ubits, ucopy = (torch.zeros(words, dtype=torch.int64, device="cuda") for _ in range(2))

    def yard(i):
        check(C.cbinfer_cbupsample_forward(ptr(ux), ptr(uout), ptr(upMasks[i % SETS]), None, 0, None, ptr(ubits), ptr(ucopy),
                                           Co, Ho // s, Wo // s, up, dt, st))

    # results first: with every pixel listed the operator equals torch's bit for bit; in mask form too after a full frame
    cb(0, mask=False)
    assert torch.equal(out, dense(0)), "%s differs from torch's operator" % name
    cb(1)
    assert torch.equal(out, dense(0)), "%s in mask form differs from torch's operator" % name
    yard(1)
    assert torch.equal(ucopy, mcopy), "the yardstick walks another footprint"
    t = rounds([("cb", cb), ("dense", dense), ("yard", yard)], reps)
    listed = listed_share(sets)
    print("| %s | %s | %d ch @%dx%d -> %d ch @%dx%d | %.1f %% | %s | %s | %s | %.2fx |"
          % (name, dtype_name(dtype), Cn, H, W, Co, Ho, Wo, listed, fmt(t["cb"]), fmt(t["dense"]), fmt(t["yard"]),
             statistics.median(t["dense"]) / statistics.median(t["cb"])))


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    assert torch.cuda.is_available(), "rearrange_target.py needs a GPU"
    print("# Change-based pixel shuffle, unshuffle and channel shuffle at 10 % and 100 % changed pixels\n")
    print("%s, torch %s; times in us per call, median [min..max] over %d interleaved rounds of %d calls\n"
          % (torch.cuda.get_device_name(0), torch.__version__, reps, BATCH))
    print("| operator | dtype | shape | changed input pixels | change-based, mask form | dense torch operator | "
          "CBUpsample2d nearest, same output | dense / change-based |")
    print("|---|---|---|---|---|---|---|---|")
    for name, kind, f, shape, block in CASES:
        for dtype in (torch.float32, torch.float16):
            for share in (0.10, 1.0):
                case(name, kind, f, shape, block, dtype, share, reps)


if __name__ == "__main__":
    main()
