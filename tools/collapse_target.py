#!/usr/bin/env python3
"""Target of the change-based reductions that collapse the channel axis (cb_chancollapse.hip): fp32 and
fp16, 10 % changed pixels per frame in whole blocks (32x32 frame pixels of a 320x480 frame, i.e. 32 / 8 / 6 / 4 pixels
at the four resolutions) --
  argmax:           21 ch and 150 ch @80x120, 19 ch @320x480     against torch.argmax(x, 1)
  (mean, max):      64 ch @80x120, 256 ch @40x60                 against cat([x.mean(1, True), x.amax(1, True)], 1)
  norm:             128 ch @60x80                                against torch.linalg.vector_norm(x, dim=1)
Per layer and dtype: cbinfer_cbchancollapse_forward with the operand in MASK form (one launch) and in LIST form (two
launches) against the dense torch operator on the same tensor in the same run.  The measuring method is
tools/target_common.py's.  Nothing here is a promise: the table says what came out, the rows where the dense operator
wins included.  Writes markdown (profiles/collapse_target.md).
usage: collapse_target.py [rounds] [output.md]"""
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import pycbinfer  # noqa: E402,F401
from cbinfer_amd import _lib  # noqa: E402
from cbinfer_amd._lib import C, check, ptr  # noqa: E402
from target_common import BATCH, SETS, change_sets, device_sets, dtype_name, fmt, listed_share, rounds  # noqa: E402

#          name, ops, channels, H, W, block
LAYERS = [("21 ch", ("argmax",), 21, 80, 120, 8), ("150 ch", ("argmax",), 150, 80, 120, 8),
          ("19 ch", ("argmax",), 19, 320, 480, 32), ("64 ch", ("mean", "max"), 64, 80, 120, 8),
          ("256 ch", ("mean", "max"), 256, 40, 60, 4), ("128 ch", ("norm",), 128, 60, 80, 6)]
KINDS = dict(sum=_lib.CC_SUM, mean=_lib.CC_MEAN, norm=_lib.CC_NORM, max=_lib.CC_MAX, min=_lib.CC_MIN,
             argmax=_lib.CC_ARGMAX, argmin=_lib.CC_ARGMIN)
DENSE = {("argmax",): ("torch.argmax(x, 1)", lambda x: torch.argmax(x, 1)),
         ("mean", "max"): ("cat([mean, amax], 1)", lambda x: torch.cat([x.mean(1, keepdim=True), x.amax(1, keepdim=True)], 1)),
         ("norm",): ("linalg.vector_norm(x, dim=1)", lambda x: torch.linalg.vector_norm(x, dim=1))}


def layer(name, ops, Cn, H, W, block, dtype, reps):
    rng = np.random.default_rng(7)
    x = (torch.randn(1, Cn, H, W, device="cuda") * 3).to(dtype)
    sets = change_sets(rng, H, W, block, 0.10)
    masks, lists = device_sets(sets)
    words = C.cbinfer_mask_words(H, W)
    bits = torch.zeros(words, dtype=torch.int64, device="cuda")
    mcopy = torch.zeros(words, dtype=torch.int64, device="cuda")
    arg = ops[0] in ("argmax", "argmin")
    out = (torch.empty(1, H, W, dtype=torch.int64, device="cuda") if arg
           else torch.empty(1, len(ops), H, W, dtype=dtype, device="cuda"))
    label = torch.zeros(words, dtype=torch.int64, device="cuda") if arg else None
    st = torch.cuda.current_stream().cuda_stream
    dt = _lib.dtype_code(x)
    packed = sum(KINDS[n] << (4 * k) for k, n in enumerate(ops))
    listed = listed_share(sets)
    dname, dense_op = DENSE[ops]

    def call(mask, lst):
        check(C.cbinfer_cbchancollapse_forward(ptr(x), ptr(out), ptr(mask), ptr(lst), lst.numel() if lst is not None else 0,
                                               None, ptr(bits), ptr(mcopy), ptr(label), Cn, H, W, packed, len(ops), dt, st))

    def dense(i):
        return dense_op(x)

    def cb_mask(i):
        call(masks[i % SETS], None)

    def cb_list(i):
        call(None, lists[i % SETS])

    with torch.no_grad():
        # results first: with every pixel listed the frame must agree with torch's operator on the device -- labels
        # exactly (randn values have no ties), max exactly, mean and norm up to another summation order and, in fp16,
        # torch's own intermediate roundings: a loose sanity bar, not the specification's
        call(None, None)
        ref = dense(0)
        if arg:
            assert torch.equal(out, ref), "change-based labels differ from torch.argmax"
        else:
            got, ref = out.float().reshape(ref.shape), ref.float()
            tol = 64 * (2.0 ** -23 if dtype == torch.float32 else 2.0 ** -10)
            assert bool(((got - ref).abs() <= tol * (ref.abs() + ref.abs().max())).all()), \
                "change-based frame differs from the dense operator (%s)" % dname
        t = rounds([("mask", cb_mask), ("list", cb_list), ("dense", dense)], reps)
    dm = statistics.median(t["dense"]) / statistics.median(t["mask"])
    dl = statistics.median(t["dense"]) / statistics.median(t["list"])
    return ("| %s @%dx%d | %s | %s | %s | %.1f %% | %s | %s | %s | %.2fx / %.2fx |"
            % (name, H, W, dtype_name(dtype), "+".join(ops), dname, listed, fmt(t["mask"]), fmt(t["list"]),
               fmt(t["dense"]), dm, dl))


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(REPO, "profiles", "collapse_target.md")
    assert torch.cuda.is_available(), "collapse_target.py needs a GPU"
    lines = ["# Change-based collapse of the channel axis at 10 % changed pixels\n",
             "%s, torch %s; times in us per call, median [min..max] over %d interleaved rounds of %d calls; the arg rows "
             "include the label-changed mask\n" % (torch.cuda.get_device_name(0), torch.__version__, reps, BATCH),
             "| layer | dtype | ops | dense torch operator | changed pixels | cbinfer_cbchancollapse_forward, mask form "
             "| cbinfer_cbchancollapse_forward, list form | dense | dense / mask form, dense / list form |",
             "|---|---|---|---|---|---|---|---|---|"]
    for spec in LAYERS:
        for dtype in (torch.float32, torch.float16):
            lines.append(layer(*spec, dtype=dtype, reps=reps))
    text = "\n".join(lines) + "\n"
    print(text)
    with open(path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
