#!/usr/bin/env python3
"""Target of the change-based element-wise operators of two maps (cb_binary.hip): fp32 and fp16, 10 % changed pixels per
frame in whole blocks (32x32 frame pixels of a 480x640 / 384x1280 frame, i.e. 8 / 4 / 32 pixels at the resolutions below) --
  64 ch @ 96x320,  256 ch @ 48x160  (second operand a map),
  64 ch @ 96x320 with a one-channel gate map,  3 ch @ 480x640 (a head).
Operators: the gate a * sigmoid(b) (torch: two operators), the layer scale gamma[c] * x (a constant channel vector: only
x's changes count), the difference a - b.  Per row: cbinfer_cbbinary_forward with the operands in MASK form (one launch)
and in LIST form (one launch more per per-frame operand) -- every per-frame operand carries the frame's change set --,
against torch's dense operator(s) on the same tensors.  The measuring method is tools/target_common.py's.  Prints
markdown (profiles/binary_target.md).
usage: binary_target.py [rounds]"""
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cbinfer_amd import _lib  # noqa: E402
from cbinfer_amd._lib import C, check, ptr  # noqa: E402
from target_common import BATCH, SETS, change_sets, device_sets, dtype_name, fmt, listed_share, rounds  # noqa: E402

#          name, channels, H, W, block, second operand of the gate, operators
ROWS = [("64 ch", 64, 96, 320, 8, 'map', ('gate', 'scale', 'sub')),
        ("256 ch", 256, 48, 160, 4, 'map', ('gate', 'scale', 'sub')),
        ("64 ch, one-channel gate", 64, 96, 320, 8, 'pixel', ('gate',)),
        ("3 ch head", 3, 480, 640, 32, 'map', ('gate', 'scale', 'sub'))]
WHAT = {'gate': "a * sigmoid(b)", 'scale': "gamma[c] * x", 'sub': "a - b"}


def row(name, Cn, H, W, block, gateForm, what, dtype, reps):
    rng = np.random.default_rng(7)
    torch.manual_seed(7)
    a = torch.randn(1, Cn, H, W, device="cuda").to(dtype)
    if what == 'scale':
        b, form, chg = torch.randn(1, Cn, 1, 1, device="cuda").to(dtype), _lib.BIN_CHANNEL, _lib.BIN_B_NONE
    elif what == 'gate' and gateForm == 'pixel':
        b, form, chg = torch.randn(1, 1, H, W, device="cuda").to(dtype), _lib.BIN_PIXEL, _lib.BIN_B_OWN
    else:
        b, form, chg = torch.randn(1, Cn, H, W, device="cuda").to(dtype), _lib.BIN_MAP, _lib.BIN_B_OWN
    op = _lib.BIN_SUB if what == 'sub' else _lib.BIN_MUL
    gate = _lib.BIN_GATE_SIGMOID if what == 'gate' else _lib.BIN_GATE_NONE
    own = chg == _lib.BIN_B_OWN
    sets = change_sets(rng, H, W, block, 0.10)
    masks, lists = device_sets(sets)
    words = C.cbinfer_mask_words(H, W)
    bits = torch.zeros(words, dtype=torch.int64, device="cuda")
    mcopy = torch.zeros(words, dtype=torch.int64, device="cuda")
    out = torch.empty_like(a)
    st = torch.cuda.current_stream().cuda_stream
    dt = _lib.dtype_code(a)

    def dense(i):
        if what == 'gate':
            return a * torch.sigmoid(b)
        return b * a if what == 'scale' else a - b

    def frame(ma, la, mb, lb):
        check(C.cbinfer_cbbinary_forward(ptr(a), ptr(b), ptr(out), ptr(ma), ptr(la), la.numel() if la is not None else 0,
                                         None, ptr(mb), ptr(lb), lb.numel() if lb is not None else 0, None, form, chg,
                                         ptr(bits), ptr(mcopy), Cn, H, W, op, gate, 0, dt, st))

    def cb_mask(i):
        m = masks[i % SETS]
        frame(m, None, m if own else None, None)

    def cb_list(i):
        lst = lists[i % SETS]
        frame(None, lst, None, lst if own else None)

    # results first: with every pixel listed the frame must be the dense result -- bit for bit, or within the bound of
    # tests/test_gpu_binary.py for the sigmoid gate
    frame(None, None, None, None)
    if what == 'gate':
        ref = a.double() / (1.0 + torch.exp(-b.double()))
        tol = 15.0 * 2.0 ** -24 + (2.0 * 2.0 ** -11 if dtype == torch.float16 else 0.0)
        assert bool(((out.double() - ref).abs() <= tol * ref.abs() + 2.0 ** -24).all()), "gate beyond its bound"
    else:
        assert torch.equal(out, dense(0)), "change-based frame differs from the dense operator"
    t = rounds([("mask", cb_mask), ("list", cb_list), ("dense", dense)], reps)
    listed = listed_share(sets)
    dm = statistics.median(t["dense"]) / statistics.median(t["mask"])
    dl = statistics.median(t["dense"]) / statistics.median(t["list"])
    print("| %s @%dx%d | %s | %s | %.1f %% | %s | %s | %s | %.2fx / %.2fx |"
          % (name, H, W, WHAT[what], dtype_name(dtype), listed, fmt(t["mask"]), fmt(t["list"]), fmt(t["dense"]), dm, dl))


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    assert torch.cuda.is_available(), "binary_target.py needs a GPU"
    print("# Change-based element-wise operators of two maps at 10 % changed pixels\n")
    print("%s, torch %s; times in us per call, median [min..max] over %d interleaved rounds of %d calls\n"
          % (torch.cuda.get_device_name(0), torch.__version__, reps, BATCH))
    print("| layer | operator | dtype | changed pixels | cbinfer_cbbinary_forward, mask form | cbinfer_cbbinary_forward, "
          "list form | dense torch | dense / mask form, dense / list form |")
    print("|---|---|---|---|---|---|---|---|")
    for name, Cn, H, W, block, gateForm, ops in ROWS:
        for what in ops:
            for dtype in (torch.float32, torch.float16):
                row(name, Cn, H, W, block, gateForm, what, dtype, reps)


if __name__ == "__main__":
    main()
