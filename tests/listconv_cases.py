"""Case table of the list contraction (cb_conv.hip) and a classifier of the launch form and regime a shape lands in.

`list_form` restates the HOST selection (launch_mfma, launch_f32, launch_f16, cb_conv_grid) and the DEVICE formulas
at the top of cb_mfma_f32_kernel / cb_mfma_f16_kernel.  It is a classifier only: it says which instantiation, split-K
slice count and item schedule a case exercises, so that the table below can be checked for coverage on a machine
without a GPU (tests/test_host_listconv.py) and so that a change of the heuristics that moves a case into another
regime makes tests/test_gpu_listconv.py fail loudly.  No expected output is ever derived from it.

No GPU and no torch in this module.
"""
import math
import struct
import zlib
from collections import namedtuple

import numpy as np

CB_F32, CB_F16, CB_F32S = 0, 1, 2
ARITH = {"F32": CB_F32, "F16": CB_F16, "F32S": CB_F32S}

GRID_PER_CU = 2          # CB_CONV_GRID_PER_CU
SK_TARGET = 2            # CB_SK_TARGET
SKMAX, SKMAX_SEAM = 8, 32
ASSUMED_CUS = 256        # the CU count the claimed cells of CASES are written for (MI355X)


def _f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


def _isqrtf(c, P):
    """(int)sqrtf(c_f32 * (float)P) in float arithmetic."""
    return int(_f32(math.sqrt(_f32(_f32(c) * float(P)))))


def kpad(K):
    return 32 if K <= 32 else (K + 63) // 64 * 64


def ckkpad(Ckk, dtype):
    q = 128 if dtype == "F16" else 32
    return (Ckk + q - 1) // q * q


def list_form(dtype, K, C, kH, kW, N, has_workspace, from_mask, epi, cus, n_host=None):
    """dtype: 'F32' | 'F32S' | 'F16'; N: the change count the kernel sees; epi: 'scatter' | 'accumulate';
    n_host: the capacity the launch was sized for (numChanges; H*W for the mask forms), default N."""
    assert dtype in ARITH and epi in ("scatter", "accumulate")
    n_host = N if n_host is None else n_host
    KP, Ckk = kpad(K), C * kH * kW
    CkkP = ckkpad(Ckk, dtype)
    kernel = "f16" if dtype == "F16" else "f32"
    MS = 1
    if KP <= 32:
        form, WM, WN = "narrow", 1, 4
    elif dtype == "F32S" and KP % 256 == 0:
        form, WM, WN, MS = "256x64", 4, 2, 2
    elif dtype == "F32S" and KP % 128 == 0:
        form, WM, WN, MS = "128x128", 2, 4, 2
    else:
        form, WM, WN = "64x64", 2, 2
    NT = 64 * WM * WN * 2
    BM, BN = 32 * WM * MS, 32 * WN
    # launch_f32: one workgroup per CU for the 1024-thread forms; the kernel's GPC says the same from NT
    GPC = 1 if (kernel == "f32" and NT > 512) else GRID_PER_CU
    seam = bool(has_workspace) and kernel == "f32" and MS == 2     # (both epilogues of the gather form scatter)
    MT = KP // BM
    tiles_cap = -(-n_host // BN) * MT
    grid = 0
    if tiles_cap:
        grid = GPC * cus
        if not has_workspace and tiles_cap < grid and not from_mask:
            grid = tiles_cap
    T = -(-N // BN) * MT
    SK = 1
    if kernel == "f32":
        P = (CkkP + 127) // 128                  # groups of four 32-deep stages, the last one partial
        kcus = grid // GPC
        if has_workspace and T > 0 and P >= 4:
            cap = min(SKMAX_SEAM, P) if seam else min(SKMAX, P, _isqrtf(3.4, P))
            if GPC == 2 and P >= 8 and T * 2 >= kcus:
                SK = max(1, min(cap, SK_TARGET * kcus // T))
            else:
                SK = max(1, min(cap, kcus // T))
        xmap = MT in (1, 2, 4, 8) and grid % 8 == 0
    else:
        P = CkkP // 128                          # pairs of 64-deep stages
        kcus = grid // GRID_PER_CU
        if has_workspace and 0 < T < SK_TARGET * kcus and P >= 8:
            SK = max(1, min(SKMAX, SK_TARGET * kcus // T, _isqrtf(1.7, P)))
        xmap = False
    items = T * SK
    return dict(kernel=kernel, form=form, BM=BM, BN=BN, MT=MT, T=T, P=P, SK=SK, seam=seam, grid=grid, items=items,
                xmap=xmap, multi_item=items > grid, KP=KP, Ckk=Ckk, CkkP=CkkP, NT=NT)


def regime_of(f, has_workspace):
    """'nows': SK = 1 for want of a workspace; 'ws_shallow': a workspace, but the k-depth is below the split
    threshold (P < 4 for f32, P < 8 for fp16); 'ws_full': deep enough, but the list fills the chip on its own;
    'lastwg': 1 < SK <= 8, summed by the last workgroup through slabs and tickets; 'seam': slices summed by the
    second launch; 'seam>8': ... whose batches of eight run more than once."""
    if not has_workspace:
        return "nows"
    if f["SK"] == 1:
        return "ws_shallow" if f["P"] < (4 if f["kernel"] == "f32" else 8) else "ws_full"
    if f["seam"]:
        return "seam>8" if f["SK"] > 8 else "seam"
    return "lastwg"


def cell_of(dtype, f, has_workspace):
    return (dtype, f["form"], regime_of(f, has_workspace), "multi_item" if f["multi_item"] else "single")


# -------------------------------------------------------------------------------------------------------------------
# the cases
# -------------------------------------------------------------------------------------------------------------------
# pixels: ('rand', N) N distinct pixels anywhere; ('all',) every pixel; ('interior', N) only pixels all of whose taps
# lie inside the map (the fast gather, where the slice holds no padded k); ('border',) the outermost ring of the map;
# ('mixed', N) interior and ring pixels alternating, so that every 64-pixel wave holds both.
# count: the change-count class the case claims ('1', 'BN-1', 'BN', 'BN+1', 'all', or None).
Case = namedtuple("Case", "id dtype K C kH kW H W pixels ws cell count")


def _c(id, dtype, K, C, filt, H, W, pixels, ws, form, regime, items="single", count=None):
    return Case(id, dtype, K, C, filt[0], filt[1], H, W, pixels, ws, (dtype, form, regime, items), count)


CASES = [
    # ---- F32: exact f32 MFMA ------------------------------------------------------------------------------------
    _c("f32-narrow-n1", "F32", 7, 5, (3, 5), 23, 41, ("rand", 1), False, "narrow", "nows", count="1"),
    _c("f32-narrow-1x1-w63", "F32", 32, 3, (1, 1), 9, 63, ("rand", 127), True, "narrow", "ws_shallow", count="BN-1"),
    # Ckk 392 -> CkkP 416: 13 stages cut 4/4/5, the last slice ends in padded k
    _c("f32-narrow-split3", "F32", 16, 8, (7, 7), 20, 64, ("rand", 129), True, "narrow", "lastwg", count="BN+1"),
    _c("f32-narrow-multi", "F32", 8, 1, (3, 3), 260, 256, ("all",), False, "narrow", "nows", "multi_item", "all"),
    # T = 130 tiles >= half the CUs and P = 8: the rule that splits towards two workgroups per CU
    _c("f32-narrow-halfgrid", "F32", 8, 19, (7, 7), 130, 130, ("rand", 16640), True, "narrow", "lastwg"),
    _c("f32-64-bn-w65", "F32", 33, 3, (3, 3), 19, 65, ("rand", 64), False, "64x64", "nows", count="BN"),
    _c("f32-64-split3", "F32", 65, 8, (7, 7), 21, 70, ("rand", 65), True, "64x64", "lastwg", count="BN+1"),
    _c("f32-64-split8", "F32", 64, 48, (7, 7), 12, 17, ("rand", 40), True, "64x64", "lastwg"),
    _c("f32-64-multi", "F32", 256, 4, (3, 3), 96, 96, ("all",), True, "64x64", "ws_shallow", "multi_item", "all"),
    _c("f32-64-h1-w130", "F32", 100, 2, (3, 5), 1, 130, ("all",), False, "64x64", "nows", count="all"),
    _c("f32-64-interior", "F32", 64, 32, (3, 3), 30, 40, ("interior", 200), False, "64x64", "nows"),
    _c("f32-64-border", "F32", 40, 5, (7, 7), 16, 24, ("border",), True, "64x64", "ws_shallow"),
    _c("f32-64-mixed", "F32", 64, 32, (3, 3), 30, 40, ("mixed", 128), False, "64x64", "nows"),
    _c("f32-64-w1", "F32", 40, 3, (7, 7), 70, 1, ("all",), False, "64x64", "nows", count="all"),
    _c("f32-narrow-even", "F32", 20, 4, (2, 7), 15, 33, ("rand", 100), True, "narrow", "ws_shallow"),
    _c("f32-64-n1-ws", "F32", 64, 8, (7, 7), 20, 64, ("rand", 1), True, "64x64", "lastwg", count="1"),
    _c("f32-64-bnm1", "F32", 48, 6, (3, 3), 14, 22, ("rand", 63), False, "64x64", "nows", count="BN-1"),
    # ---- F32S: three bf16 terms per operand ------------------------------------------------------------------------
    _c("f32s-narrow-bn", "F32S", 16, 5, (3, 5), 23, 41, ("rand", 128), False, "narrow", "nows", count="BN"),
    _c("f32s-narrow-split3", "F32S", 24, 8, (7, 7), 20, 63, ("rand", 127), True, "narrow", "lastwg", count="BN-1"),
    _c("f32s-narrow-multi", "F32S", 8, 1, (3, 3), 260, 256, ("all",), True, "narrow", "ws_shallow", "multi_item", "all"),
    # K = 130 -> KP 192: three row tiles, no XCD-aware order
    _c("f32s-64-k130", "F32S", 130, 6, (3, 3), 21, 65, ("rand", 63), False, "64x64", "nows", count="BN-1"),
    _c("f32s-64-split3", "F32S", 130, 8, (7, 7), 21, 40, ("rand", 65), True, "64x64", "lastwg", count="BN+1"),
    _c("f32s-64-multi", "F32S", 130, 2, (3, 3), 105, 105, ("all",), True, "64x64", "ws_shallow", "multi_item", "all"),
    _c("f32s-128-n1", "F32S", 128, 3, (3, 3), 17, 40, ("rand", 1), False, "128x128", "nows", count="1"),
    _c("f32s-128-shallow", "F32S", 128, 12, (3, 7), 31, 67, ("rand", 129), True, "128x128", "ws_shallow", count="BN+1"),
    _c("f32s-128-seam4", "F32S", 128, 8, (7, 7), 20, 33, ("rand", 128), True, "128x128", "seam", count="BN"),
    _c("f32s-128-seam9", "F32S", 128, 21, (7, 7), 20, 33, ("rand", 127), True, "128x128", "seam>8", count="BN-1"),
    # K = 384: three row tiles on the 128 x 128 form
    _c("f32s-128-mt3-seam", "F32S", 384, 8, (7, 7), 20, 33, ("rand", 130), True, "128x128", "seam"),
    _c("f32s-128-multi", "F32S", 384, 2, (3, 3), 105, 105, ("all",), True, "128x128", "ws_shallow", "multi_item", "all"),
    _c("f32s-256-nows", "F32S", 256, 5, (3, 5), 23, 41, ("rand", 64), False, "256x64", "nows", count="BN"),
    _c("f32s-256-seam4", "F32S", 512, 8, (7, 7), 20, 33, ("rand", 63), True, "256x64", "seam", count="BN-1"),
    # Ckk 3969 -> 125 stages over 32 slices: the reduce launch's batches of eight run four times
    _c("f32s-256-seam32", "F32S", 256, 81, (7, 7), 12, 13, ("rand", 100), True, "256x64", "seam>8"),
    # Ckk 800 = 25 whole stages, 7 slices, interior pixels only: every slice on the fast gather
    _c("f32s-256-seam7-interior", "F32S", 256, 32, (5, 5), 14, 19, ("interior", 65), True, "256x64", "seam",
       count="BN+1"),
    _c("f32s-256-multi", "F32S", 256, 2, (3, 3), 130, 130, ("all",), False, "256x64", "nows", "multi_item", "all"),
    _c("f32s-256-mt3", "F32S", 768, 2, (3, 3), 9, 33, ("rand", 65), True, "256x64", "ws_shallow", count="BN+1"),
    _c("f32s-128-mixed", "F32S", 128, 32, (3, 3), 30, 40, ("mixed", 256), True, "128x128", "ws_shallow"),
    # ---- F16 ---------------------------------------------------------------------------------------------------------
    _c("f16-narrow-n1", "F16", 20, 3, (3, 3), 11, 35, ("rand", 1), False, "narrow", "nows", count="1"),
    _c("f16-narrow-bn", "F16", 32, 7, (3, 5), 23, 41, ("rand", 128), True, "narrow", "ws_shallow", count="BN"),
    # Ckk 931 -> CkkP 1024, P = 8, SK = 3: stage pairs cut 2/3/3
    _c("f16-narrow-split3", "F16", 16, 19, (7, 7), 20, 33, ("rand", 129), True, "narrow", "lastwg", count="BN+1"),
    _c("f16-narrow-multi", "F16", 8, 3, (3, 3), 260, 257, ("all",), False, "narrow", "nows", "multi_item", "all"),
    _c("f16-narrow-bnm1", "F16", 9, 5, (1, 1), 9, 63, ("rand", 127), False, "narrow", "nows", count="BN-1"),
    _c("f16-64-k130", "F16", 130, 5, (3, 3), 21, 65, ("rand", 63), False, "64x64", "nows", count="BN-1"),
    _c("f16-64-split3", "F16", 130, 19, (7, 7), 21, 41, ("rand", 65), True, "64x64", "lastwg", count="BN+1"),
    _c("f16-64-multi", "F16", 130, 3, (3, 3), 105, 105, ("all",), True, "64x64", "ws_shallow", "multi_item", "all"),
    # Ckk 1152 = 9 whole stage pairs, interior pixels only: split 3/3/3, every slice on the fast gather
    _c("f16-64-interior-split", "F16", 64, 128, (3, 3), 15, 21, ("interior", 200), True, "64x64", "lastwg"),
    _c("f16-64-interior", "F16", 64, 128, (3, 3), 15, 21, ("interior", 64), False, "64x64", "nows", count="BN"),
    _c("f16-64-border", "F16", 48, 9, (7, 7), 16, 25, ("border",), False, "64x64", "nows"),
    _c("f16-64-mixed", "F16", 64, 128, (3, 3), 15, 21, ("mixed", 128), False, "64x64", "nows"),
    _c("f16-64-h1-w130", "F16", 100, 3, (3, 5), 1, 130, ("all",), False, "64x64", "nows", count="all"),
    _c("f16-64-w1", "F16", 40, 3, (7, 7), 70, 1, ("all",), True, "64x64", "ws_shallow", count="all"),
    _c("f16-64-1x1-w64", "F16", 64, 31, (1, 1), 9, 64, ("all",), False, "64x64", "nows", count="all"),
    _c("f16-narrow-even", "F16", 20, 5, (2, 7), 15, 33, ("rand", 100), True, "narrow", "ws_shallow"),
]
CASE_BY_ID = {c.id: c for c in CASES}
assert len(CASE_BY_ID) == len(CASES)

# subsets used by the other GPU tests
ACCUMULATE_IDS = ["f32-64-split3", "f32-64-multi", "f32s-64-k130", "f32s-128-seam9", "f32s-256-seam4",
                  "f16-64-k130", "f16-64-split3", "f16-narrow-bn"]
OUT_OF_MAP_IDS = ["f32-64-split3", "f32-64-bn-w65", "f32s-128-seam4", "f32s-256-seam32", "f16-64-split3",
                  "f16-narrow-bn"]
CLEAR_BITS_IDS = ["f32-64-n1-ws", "f32s-128-seam4", "f16-narrow-split3", "f16-narrow-n1"]


def interior_box(c):
    """[y0, y1) x [x0, x1): the pixels all of whose taps lie inside the map (the test of CB_GATHER_FAST)."""
    ph, pw = (c.kH - 1) // 2, (c.kW - 1) // 2
    return ph, c.H - (c.kH - 1 - ph), pw, c.W - (c.kW - 1 - pw)


def case_pixels(c):
    """The case's change list: ascending, distinct, int32; the same on every call."""
    rng = np.random.default_rng(zlib.crc32(c.id.encode()))
    HW = c.H * c.W
    kind = c.pixels[0]
    if kind == "all":
        return np.arange(HW, dtype=np.int32)
    ys, xs = np.divmod(np.arange(HW), c.W)
    y0, y1, x0, x1 = interior_box(c)
    inner = np.flatnonzero((ys >= y0) & (ys < y1) & (xs >= x0) & (xs < x1))
    ring = np.flatnonzero((ys == 0) | (ys == c.H - 1) | (xs == 0) | (xs == c.W - 1))
    if kind == "rand":
        return np.sort(rng.choice(HW, c.pixels[1], replace=False)).astype(np.int32)
    if kind == "interior":
        return np.sort(rng.choice(inner, c.pixels[1], replace=False)).astype(np.int32)
    if kind == "border":
        return ring.astype(np.int32)
    assert kind == "mixed"
    n = c.pixels[1]
    a = rng.choice(inner, n // 2, replace=False)
    b = rng.choice(ring, n - n // 2, replace=False)
    out = np.empty(n, dtype=np.int32)      # not sorted: alternating, so every wave of 64 slots holds both kinds
    out[0::2], out[1::2] = b, a
    return out


def case_form(c, cus, n=None, n_host=None, epi="scatter"):
    n = len(case_pixels(c)) if n is None else n
    return list_form(c.dtype, c.K, c.C, c.kH, c.kW, n, c.ws, False, epi, cus, n_host)


def reference_macs(c):
    return len(case_pixels(c)) * c.C * c.kH * c.kW * c.K
