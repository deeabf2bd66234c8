"""Case table of the fp16 layers on the split-state machinery (cb_split.hip: cbinfer_hsplit_forward[_group], the four
HALF instantiations of cbs_conv_kernel, cbh_reduce_kernel, cbh_detect_kernel) and a classifier of the launch form a
shape lands in.

`hsplit_form` restates cbh_geom / cbh_supported, the HOST selection of cbinfer_hsplit_forward_group (tile height, the
demotion of a shallow layer to 64-row tiles, the instantiation by the mask words of the launch, the refusals), the
DEVICE's chunk rule at the top of cbs_conv_kernel<..., HALF> (4 -> 8 -> 16 chunks per layer, the split decision, the
layers' item ranges) and the workspace sizes.  It is a classifier only: it says which instantiation, chunk counts and
item schedule a case exercises, so that the table below can be checked for coverage on a machine without a GPU
(tests/test_host_hsplit.py) and so that a change of the heuristics that moves a case into another cell makes
tests/test_gpu_hsplit.py fail loudly.  No expected output is ever derived from it.

The module also holds what the host test and the GPU test must share: the cases' data (weights with per-row scales
exp(U(-4, 2)), inputs exact in f16), the patches of a state in numpy and the per-element bar.

No GPU and no torch in this module.
"""
import zlib
from collections import namedtuple

import numpy as np

from splitconv_cases import dilate, rows, singles
from optest import mask_words      # noqa: F401  (handed on to the tests)

ASSUMED_CUS = 256        # the CU count the claimed cells of CASES are written for (MI355X)
GROUP_MAX, NEXT_MAX = 2, 2                          # CBINFER_HGROUP_MAX, CBINFER_HNEXT_MAX
PRE_BIG, PRE_SMALL, PRE_MID = 1536, 1280, 5120      # cb_split_common.h
SPAD = 4096              # CBS_SPAD
CHUNKS = 4               # CBS_CHUNKS
MAX_CHUNKS = 16          # CbsParams.maxChunks of the fp16 layers
SPLIT_ROUNDS = 2         # CbsParams.splitRounds
DEEP = 48                # stages from which a contraction is a sum of partial sums over fixed stage ranges
OK, BADARG, UNSUPPORTED = 0, -1, -2                 # CB_OK, CB_ERR_BADARG, CB_ERR_UNSUPPORTED

Instance = namedtuple("Instance", "BM cap mask_lds ring per_cu")


def name_of(i):
    return "h/%d/pre%d/%s/ring%d/%dwg" % (i.BM, i.cap, "lds" if i.mask_lds else "mem", i.ring, i.per_cu)


# the four HALF instantiations cbinfer_hsplit_forward_group launches, in its order
H128_LDS = Instance(128, PRE_BIG, True, 4, 1)
H128_MEM = Instance(128, PRE_MID, False, 4, 1)
H64_LDS = Instance(64, PRE_SMALL, True, 4, 2)
H64_MEM = Instance(64, PRE_MID, False, 3, 2)
INSTANCES = [H128_LDS, H128_MEM, H64_LDS, H64_MEM]
INSTANCE_BY_NAME = {name_of(i): i for i in INSTANCES}
REGIMES = ["one_stage", "shallow", "deep_whole", "deep_split4", "deep_split8", "deep_split16"]


def cpad(C):
    return (C + 63) // 64 * 64


def geom(C, H, W, kH, kW):
    """cbh_geom: the padded channel count, the stages (64 channels of one tap each) and the pixel-major copy."""
    Cp = cpad(C)
    padY, padX = kH // 2, kW // 2
    return dict(C=Cp, G=Cp // 64, nStages=kH * kW * (Cp // 64), Wp=W + 2 * padX, Hp=H + 4 * padY + 1, rec=Cp * 2)


def supported(C, K, kH, kW):
    return (64 <= C <= 1024 and 1 <= K <= 1024 and kH % 2 == 1 and kW % 2 == 1 and 1 <= kH <= 15 and 1 <= kW <= 15
            and geom(C, 64, 64, kH, kW)["nStages"] >= 1)


def tile_height(K):      # cbs_bm
    return 64 if K <= 64 else 128


def padded_rows(K):      # cbs_kp
    bm = tile_height(K)
    return (K + bm - 1) // bm * bm


def slab_capacity(nLayers, H, W, K, cus):
    bm = tile_height(K)
    return max(nLayers * ((H * W + bm - 1) // bm) * (padded_rows(K) // bm), 2 * cus)


def state_bytes(C, H, W, kH, kW):
    g = geom(C, H, W, kH, kW)
    return SPAD + g["Hp"] * g["Wp"] * g["rec"]


def prepared_bytes(C, K, kH, kW):
    n = geom(C, 64, 64, kH, kW)["nStages"]
    return (n * (padded_rows(K) // 32) * 4096 + n * 4 + 15) // 16 * 16


def group_workspace_bytes(nLayers, C, H, W, K, kH, kW, cus):
    if not 1 <= nLayers <= GROUP_MAX or not supported(C, K, kH, kW) or geom(C, H, W, kH, kW)["nStages"] < DEEP:
        return 0
    bm = tile_height(K)
    return 256 + slab_capacity(nLayers, H, W, K, cus) * bm * bm * 4


def workspace_bytes(C, H, W, K, kH, kW, cus):
    return group_workspace_bytes(1, C, H, W, K, kH, kW, cus)


def chunk_bounds(nStages, ch):
    """Stage ranges of the ch chunks of a deep fp16 contraction: stage pairs dealt by shifts, the odd last stage in the
    last chunk (chunkBeg of cbs_conv_kernel)."""
    if ch == 1:
        return [0, nStages]
    P2 = nStages >> 1
    return [2 * ((P2 * c) // ch) for c in range(ch)] + [nStages]


def hsplit_form(C, Ks, kH, kW, H, W, N_per_layer, cus, pooled=False, n_next=None, workspace=True):
    """The launch form of cbinfer_hsplit_forward_group for the layers Ks of one geometry with N_per_layer listed pixels
    each on a card with `cus` CUs.  n_next: consumers per layer.  status != OK: the host refuses (nothing else is set).
    The refusals are alike for the classifier only: the library finds the argument errors, the mismatched group and the
    consumer behind K < 64 before anything runs, but the mask words of the LAUNCH (E above the instance's capacity)
    behind its detection launch, which has refreshed the states and set the frame masks by then."""
    Ks, nL = list(Ks), len(Ks)
    n_next = list(n_next) if n_next is not None else [0] * nL
    assert 1 <= nL <= GROUP_MAX and len(N_per_layer) == nL and len(n_next) == nL
    K0 = Ks[0]
    if not supported(C, K0, kH, kW) or H > 65535:
        return dict(status=UNSUPPORTED)
    g = geom(C, H, W, kH, kW)
    KP, BM, MW = padded_rows(K0), tile_height(K0), mask_words(H, W)
    if MW > PRE_MID or g["Hp"] * g["Wp"] * g["rec"] >= 1 << 31 or H * W * W >= 1 << 32:
        return dict(status=UNSUPPORTED)
    deep = g["nStages"] >= DEEP
    if deep and not workspace:
        return dict(status=BADARG)
    for K, nn in zip(Ks, n_next):
        assert 0 <= nn <= NEXT_MAX
        if not supported(C, K, kH, kW) or padded_rows(K) != KP or tile_height(K) != BM:
            return dict(status=UNSUPPORTED)      # (one tile grid for the group)
        if nn > 0 and K < 64:
            return dict(status=UNSUPPORTED)      # (a consumer on this machinery has >= 64 input channels)
    full128 = (H * W + 127) // 128 * (KP // 128)
    demoted = BM == 128 and not deep and full128 < 4 * cus
    if demoted:
        BM = 64
    E = nL * MW
    if BM == 128:
        inst = H128_LDS if E <= PRE_BIG else H128_MEM
    else:
        inst = H64_LDS if E <= PRE_SMALL else H64_MEM
    if E > inst.cap:
        return dict(status=UNSUPPORTED)
    BN, MT, grid = BM, KP // BM, inst.per_cu * cus
    slab_cap, slab_cap1 = slab_capacity(nL, H, W, K0, cus), slab_capacity(1, H, W, K0, cus)
    # ---- the device: chunks per layer, the split decision, the item ranges ----
    CH = CHUNKS if deep else 1
    tiles = [(n + BN - 1) // BN for n in N_per_layer]
    chunks = []
    for tu in tiles:
        c = CH
        if CH > 1:
            while (2 * c <= MAX_CHUNKS and tu * MT * 2 * c <= grid and tu * MT * 2 * c <= slab_cap1
                   and g["nStages"] >= 8 * c):
                c *= 2
        chunks.append(c)
    TP = sum(tiles)
    items_split = sum(tu * MT * c for tu, c in zip(tiles, chunks))
    items_whole = TP * MT
    # (SK in the launch info: the larger of the two slots' counts -- the slot of an absent second layer holds CH)
    SK = 1
    if TP > 0 and CH > 1 and items_split <= SPLIT_ROUNDS * grid and items_split <= slab_cap:
        SK = max(chunks[0], chunks[-1] if nL == GROUP_MAX else CH)
    items = items_split if SK > 1 else items_whole
    ranges, run = [], 0
    for tu, c in zip(tiles, chunks):
        n = tu * MT * (c if SK > 1 else 1)
        ranges.append((run, run + n))
        run += n
    if g["nStages"] <= 2:
        regime = "one_stage"
    elif not deep:
        regime = "shallow"
    elif SK == 1:
        regime = "deep_whole"
    else:      # (the chunk count of the layers that have tiles; an empty layer's is chosen but never walked)
        regime = "deep_split%d" % max(c for tu, c in zip(tiles, chunks) if tu > 0)
    return dict(status=OK, Cp=g["C"], nStages=g["nStages"], deep=deep, demoted=demoted, BM=BM, BN=BN, KP=KP, MT=MT,
                MW=MW, E=E, instance=inst, grid=grid, tiles=tiles, TP=TP, chunks=chunks, SK=SK, items=items,
                ranges=ranges, multi_item=items > grid, slab_cap=slab_cap, slab_cap1=slab_cap1, regime=regime,
                pooled=bool(pooled), reduce_launch=deep and workspace)


def cell_of(f):
    return (name_of(f["instance"]), f["regime"], "multi_item" if f["multi_item"] else "single")


# -------------------------------------------------------------------------------------------------------------------
# cells without a case
# -------------------------------------------------------------------------------------------------------------------
REFERENCE_BUDGET = 2.0e8      # multiply-adds of the float64 reference of one frame of a case


def uncovered(cell):
    """Why a cell of INSTANCES x REGIMES x (single, multi_item) has no row in CASES, or None if it must have one.

    The selection rules reach every cell (256 CUs: a grid of 256 workgroups on 128-row tiles, 512 on 64-row tiles);
    what is listed here costs more than REFERENCE_BUDGET multiply-adds in frame 1, the frame that claims the cell and
    is compared in full, at the cheapest shape that reaches it (frame 0 may be compared at a sample: opts sample0).
    A 128-row tile has 128 pixels; MT = KP / 128 row tiles have at least 128 (MT - 1) + 1 real output channels."""
    name, regime, items = cell
    inst = INSTANCE_BY_NAME[name]
    if inst.BM != 128:
        return None
    if regime in ("one_stage", "shallow"):
        # not demoted: ceil(HW / 128) MT >= 4 x 256 -- a wide K on 16257 pixels or a narrow one on a taller map.
        # More than 256 items are more than 256 / MT pixel tiles: listed pixels x real channels at the least
        #   MT = 1: 32769 x 65 = 2.13e6   MT = 2: 16385 x 129 = 2.11e6   MT = 4: 8193 x 385 = 3.15e6   MT = 8: 4097 x 897 = 3.68e6
        # times the k of the stages: 64 for one stage (1.35e8: within the budget), 192 and more from three (4.05e8)
        if items == "multi_item" and regime == "shallow":
            return ("more than 256 items are at least 16385 listed pixels x 129 channels (two row tiles; 32769 x 65 with "
                    "one, 8193 x 385 with four, 4097 x 897 with eight) x 192 k of three stages = 4.05e8 multiply-adds; "
                    "the multi-item walk of these instances is pinned on one stage")
        return None
    # The cheapest deep contraction on 128-row tiles: K = 65 real channels per row tile, C = 65 (two groups of 64) under
    # a 5x5 filter = 50 stages of 1625 real k; from 64 stages (16 chunks) 3x11 = 66 stages of 2145 k.  The chunk rule
    # on the grid of 256: 4 chunks with more than 32 (pixel tile, row tile) pairs, 8 up to 32, 16 up to 16.
    if regime == "deep_whole":
        # unsplit by the kernel's own rule: 4 TP MT > 2 x 256
        return "at least 129 tiles x 128 pixels x 65 channels x 1625 k = 1.7e9 multiply-adds (multi_item: twice that)"
    if regime == "deep_split4":
        return ("four chunks take more than 32 pairs: 33 tiles = 4097 pixels x 65 channels, or 17 x 2 = 2049 pixels x "
                "129 channels, ... x 1625 k = 4.3e8 multiply-adds at the least")
    if items == "multi_item":
        return ("more than 256 chunk items are two layers of 17 + 16 tiles of 8 chunks (3970 pixels x 65 channels x "
                "1625 k = 4.2e8) or of 9 + 8 tiles of 16 chunks (1922 pixels x 65 x 2145 k = 2.7e8)")
    return None


def all_cells():
    return [(name_of(i), r, m) for i in INSTANCES for r in REGIMES for m in ("single", "multi_item")]


# -------------------------------------------------------------------------------------------------------------------
# the cases
# -------------------------------------------------------------------------------------------------------------------
# Ks: the layers of the launch (two: a group).  change: per layer, the INPUT pixels that change by more than the
# threshold in frame 1, as rectangles (y0, x0, h, w); the change list is their footprint dilated by the filter.
# count: the class of layer 0's list length: '1' = one footprint, 'BN-1', 'BN', 'BN+1', 'all' = every pixel, 'some'.
# opts:  sample0  frame 0 (every pixel) is compared with float64 at a sample of the pixels that fits the budget --
#                 lists, states, masks and every later frame are checked in full
#        next     per layer, the consumers of its output as (kH, kW, threshold)
#        pooled   the detection reads the tensor in front of a 2x2 pool, [C, 2H-1, 2W-1], and a producer mask
#        prodmask the detection is handed a producer mask of the layer's own resolution
#        upstream the launch is handed an upstream count (0: an idle frame)
Case = namedtuple("Case", "id C Ks kH kW H W change cell count opts")


def _c(id, inst, regime, items, C, Ks, filt, H, W, change, count=None, **opts):
    Ks = (Ks,) if isinstance(Ks, int) else tuple(Ks)
    if change == "all" or (change and isinstance(change[0][0], int)):
        change = (change,) + ((),) * (len(Ks) - 1)      # (one set: layer 0's; a second layer's stays empty)
    change = tuple(((0, 0, H, W),) if ch == "all" else tuple(ch) for ch in change)
    assert len(change) == len(Ks)
    if count is None:
        count = "all" if change[0] == ((0, 0, H, W),) else "some"
    return Case(id, C, Ks, filt[0], filt[1], H, W, change, (name_of(inst), regime, items), count, opts)


def px(n, W, y0=0):
    """The first n pixels of the map from row y0 in raster order, as rectangles (a 1x1 filter lists exactly those)."""
    full, rest = divmod(n, W)
    return (((y0, 0, full, W),) if full else ()) + (((y0 + full, 0, 1, rest),) if rest else ())


def changed_pixels(c, layer=0):
    """[H, W] bool: the input pixels of a layer that change in frame 1."""
    m = np.zeros((c.H, c.W), dtype=bool)
    for (y0, x0, h, w) in c.change[layer]:
        assert 0 <= y0 and 0 <= x0 and h >= 1 and w >= 1 and y0 + h <= c.H and x0 + w <= c.W, c.id
        m[y0:y0 + h, x0:x0 + w] = True
    return m


def listed_pixels(c, layer=0):
    return dilate(changed_pixels(c, layer), c.kH, c.kW)


def layer_counts(c):
    return [int(listed_pixels(c, q).sum()) for q in range(len(c.Ks))]


def n_next(c):
    return [len(n) for n in c.opts["next"]] if "next" in c.opts else [0] * len(c.Ks)


def case_form(c, cus, counts=None):
    return hsplit_form(c.C, c.Ks, c.kH, c.kW, c.H, c.W, layer_counts(c) if counts is None else counts, cus,
                       pooled=bool(c.opts.get("pooled")), n_next=n_next(c))


def macs_per_pixel(c):
    return c.C * c.kH * c.kW * sum(c.Ks)


def sample0(c):
    """The pixels of frame 0 (every pixel is listed) that are compared with float64: all of them, or -- opts sample0 --
    the first and the last 128 of the list and a fixed random draw, as many as the budget pays for beside the 256
    pixels of sample0_second."""
    HW = c.H * c.W
    if not c.opts.get("sample0"):
        return np.arange(HW)
    n = int(REFERENCE_BUDGET // macs_per_pixel(c)) - SECOND
    assert 512 <= n < HW, c.id
    rng = np.random.default_rng(zlib.crc32(c.id.encode()) ^ 0x5a)
    pick = np.concatenate([np.arange(128), np.arange(HW - 128, HW), rng.choice(HW, n - 256, replace=False)])
    return np.unique(pick)


SECOND = 256


def sample0_second(c):
    """A second, independent draw of frame 0's pixels of a sample0 case, compared at the layer's 2-ulp bar."""
    rng = np.random.default_rng(zlib.crc32(c.id.encode()) ^ 0xa5a5)
    return np.sort(rng.choice(c.H * c.W, SECOND, replace=False))


def reference_macs(c):
    """Multiply-adds of the float64 reference of the case's costliest frame."""
    per = c.C * c.kH * c.kW
    frame0 = (len(sample0(c)) + (SECOND if c.opts.get("sample0") else 0)) * per * sum(c.Ks)
    frame1 = sum(n * per * K for n, K in zip(layer_counts(c), c.Ks))
    return max(frame0, frame1)


# ---- the cases' data: shared by the host test (teeth of the bar) and the GPU test ----
TH = 0.1


def make_weights(c, layer=0):
    """f16 weights [K, C, kH, kW] with per-output-row scales exp(U(-4, 2)) and an f16 bias."""
    rng = np.random.default_rng(zlib.crc32(("%s/w%d" % (c.id, layer)).encode()))
    K, n = c.Ks[layer], c.C * c.kH * c.kW
    w = (rng.standard_normal((K, c.C, c.kH, c.kW)) / np.sqrt(n) * np.exp(rng.uniform(-4, 2, (K, 1, 1, 1))))
    return w.astype(np.float16), rng.standard_normal(K).astype(np.float16)


def make_frames(c, layer=0):
    """The three frames of a layer, exact in f16: channels scaled by exp(U(-3, 1)) (channel 0: 1); frame 1 = frame 0 with
    new values at the changed pixels (channel 0 moved by more than the threshold for sure) + noise below the threshold
    everywhere else; frame 2 = frame 1."""
    rng = np.random.default_rng(zlib.crc32(("%s/x%d" % (c.id, layer)).encode()))
    C, H, W = c.C, c.H, c.W
    scale = np.exp(rng.uniform(-3, 1, (1, C, 1, 1)))
    scale[0, 0] = 1.0
    x0 = (rng.standard_normal((1, C, H, W)) * scale).astype(np.float16)
    m = changed_pixels(c, layer)
    fresh = (rng.standard_normal((1, C, H, W)) * scale).astype(np.float32)
    fresh[0, 0] = x0[0, 0].astype(np.float32) + np.where(rng.random((H, W)) < 0.5, -1.0, 1.0) * (
        0.5 + np.abs(rng.standard_normal((H, W))))
    noisy = x0.astype(np.float32) + rng.uniform(-0.03, 0.03, x0.shape)
    x1 = np.where(m[None, None], fresh, noisy).astype(np.float16)
    return [x0, x1, x1.copy()]


def patches(state, idx, kH, kW):
    """[N, C kH kW] f32: the zero-padded kH x kW windows of a [1, C, H, W] state around the listed pixels, in the
    filter bank's (channel, ky, kx) order -- the data movement of genXMatrix, in numpy."""
    _, C, H, W = state.shape
    ph, pw = kH // 2, kW // 2
    pad = np.zeros((C, H + 2 * ph, W + 2 * pw), dtype=np.float32)
    pad[:, ph:ph + H, pw:pw + W] = state[0]
    win = np.lib.stride_tricks.sliding_window_view(pad, (kH, kW), axis=(1, 2))      # [C, H, W, kH, kW]
    idx = np.asarray(idx, dtype=np.int64)
    X = win[:, idx // W, idx % W]                                                    # [C, N, kH, kW]
    return np.ascontiguousarray(X.transpose(1, 0, 2, 3)).reshape(idx.size, C * kH * kW)


# ---- the bar ----
# A of the bar.  The observed worst (|err| - rounding terms) / (sum|a||b| + |bias|) of every cell sits far below 2^-20
# (2^-24.3 at the most, MI355X, 2026-10-20: the docstring of tests/test_gpu_hsplit.py), so A is the bar the f32
# split-state forms carry -- below the provable ceiling of every shape these layers take (C >= 64: 66 * 2^-24 and more)
BAR_A = 64 * 2.0 ** -24


def a_ceiling(C, kH, kW):
    """Products of f16 values are exact in f32 and the sum is taken in f32 in some order: n - 1 additions of the n =
    C kH kW products, the bias, and slack for the chunk sums of a deep contraction."""
    return (C * kH * kW + 2) * 2.0 ** -24


def bar_A(C, kH, kW):
    assert BAR_A <= a_ceiling(C, kH, kW)
    return BAR_A


def rounding_terms(want):
    """The single rounding of the result to f16: half an ulp of a normal number, half the subnormal spacing below."""
    return 2.0 ** -11 * np.abs(want) + 2.0 ** -25


def bar(want, mag, A):
    """|got - want| <= 2^-11 |want| + 2^-25 + A (sum|a||b| + |bias|); mag = sum|a||b| + |bias|."""
    return rounding_terms(want) + A * mag


E64 = (3, 3)      # the filter of the tile-width rows (splitconv_cases.singles: footprints of 9, 6 at an edge, 4 in a corner)
BIG = dict(sample0=True)

CASES = [
    # ---- 64-row tiles, mask words in LDS (two workgroups per CU: 512) ----
    _c("h64lds-one-c64-k38-all", H64_LDS, "one_stage", "single", 64, 38, (1, 1), 9, 17, "all"),
    _c("h64lds-one-c64-k38-px1", H64_LDS, "one_stage", "single", 64, 38, (1, 1), 9, 17, ((4, 9, 1, 1),), "1"),
    _c("h64lds-one-c128-k19-bnm1", H64_LDS, "one_stage", "single", 128, 19, (1, 1), 9, 17, px(63, 17, 2), "BN-1"),
    _c("h64lds-one-c100-k64-bn", H64_LDS, "one_stage", "single", 100, 64, (1, 1), 9, 17, px(64, 17, 1), "BN"),
    _c("h64lds-one-multi", H64_LDS, "one_stage", "multi_item", 64, 1, (1, 1), 257, 128, "all"),
    _c("h64lds-shallow-c185-1x1-bnp1", H64_LDS, "shallow", "single", 185, 1, (1, 1), 9, 17, px(65, 17), "BN+1"),
    _c("h64lds-shallow-k38-w63-bnm1", H64_LDS, "shallow", "single", 64, 38, E64, 37, 63, singles(37, 63, 3, 3, 7, 0, 0), "BN-1"),
    _c("h64lds-shallow-k19-w64-bn", H64_LDS, "shallow", "single", 64, 19, E64, 37, 64, singles(37, 64, 3, 3, 6, 1, 1), "BN"),
    _c("h64lds-shallow-k64-1x5-bnp1", H64_LDS, "shallow", "single", 64, 64, (1, 5), 20, 65, singles(20, 65, 1, 5, 13, 0, 0), "BN+1"),
    _c("h64lds-shallow-7x1-one", H64_LDS, "shallow", "single", 64, 19, (7, 1), 22, 17, singles(22, 17, 7, 1, 1, 0, 0), "1"),
    _c("h64lds-shallow-c185-k38", H64_LDS, "shallow", "single", 185, 38, (3, 3), 9, 17, rows(3, 1, 17)),
    _c("h64lds-shallow-c100-k19", H64_LDS, "shallow", "single", 100, 19, (3, 3), 9, 130, ((2, 60, 3, 8),)),
    # (K = 130 pads to 256 rows: a 128-row layer that 20 x 33 pixels demote to 64-row tiles, four of them per pixel tile)
    _c("h64lds-shallow-demoted-k130", H64_LDS, "shallow", "single", 64, 130, (3, 3), 20, 33, rows(3, 2, 33)),
    _c("h64lds-shallow-multi", H64_LDS, "shallow", "multi_item", 64, 1, (3, 3), 257, 128, "all"),
    _c("h64lds-deepwhole-one", H64_LDS, "deep_whole", "single", 64, 1, (7, 7), 129, 64, "all"),
    _c("h64lds-deepwhole-multi", H64_LDS, "deep_whole", "multi_item", 64, 1, (7, 7), 513, 64, "all"),
    _c("h64lds-split8-k38", H64_LDS, "deep_split8", "single", 64, 38, (7, 7), 9, 17, "all"),
    # (48 stages exactly: 1x3 on 1024 channels, eight chunks of 6)
    _c("h64lds-split8-48stages", H64_LDS, "deep_split8", "single", 1024, 19, (1, 3), 9, 17, rows(3, 2, 17)),
    # (four chunks: more than 64 tiles -- 8 x 65 items would be more than the 512 workgroups)
    _c("h64lds-split4-one", H64_LDS, "deep_split4", "single", 64, 3, (7, 7), 129, 64, rows(3, 60, 64)),
    # (129 tiles of four chunks on 512 workgroups, in slabs a map of 516 tiles pays for)
    _c("h64lds-split4-multi", H64_LDS, "deep_split4", "multi_item", 64, 1, (7, 7), 516, 64, rows(3, 123, 64)),
    _c("h64lds-split16-c100-k19", H64_LDS, "deep_split16", "single", 100, 19, (7, 7), 20, 33, rows(3, 2, 33)),
    # (the step from 8 to 16 chunks is taken at c = 8: nStages >= 8 c = 64.  63 and 65 stages are the counts next to it
    #  that a product of an odd filter and C / 64 <= 16 reaches -- 64 itself is none)
    _c("h64lds-split8-63stages", H64_LDS, "deep_split8", "single", 64, 2, (7, 9), 9, 17, "all"),
    _c("h64lds-split16-65stages", H64_LDS, "deep_split16", "single", 64, 2, (5, 13), 9, 17, "all"),
    # (147 stages: 16 chunks up to 32 tiles, 8 from 33 -- the same layer in both)
    _c("h64lds-split16-c185-k38", H64_LDS, "deep_split16", "single", 185, 38, (7, 7), 9, 17, "all"),
    _c("h64lds-split8-c185-34tiles", H64_LDS, "deep_split8", "single", 185, 1, (7, 7), 40, 65, rows(3, 27, 65)),
    _c("h64lds-split16-c185-32tiles", H64_LDS, "deep_split16", "single", 185, 1, (7, 7), 40, 65, rows(3, 25, 65)),
    # (a group of two: 34 + 34 tiles of 8 chunks, 17 + 16 of 16 chunks -- more than 512 items, in the slabs of 2 x 272 and
    #  2 x 264 tiles)
    _c("h64lds-split8-multi", H64_LDS, "deep_split8", "multi_item", 100, (1, 1), (7, 7), 272, 64,
       (rows(3, 28, 64), rows(100, 28, 64))),
    _c("h64lds-split16-multi", H64_LDS, "deep_split16", "multi_item", 65, (1, 1), (5, 13), 264, 64,
       (rows(3, 13, 64), rows(100, 12, 64))),
    # ---- 64-row tiles, mask words in memory (more than 1280 words) ----
    _c("h64mem-one-k19", H64_MEM, "one_stage", "single", 64, 19, (1, 1), 1281, 8, px(63, 8, 5), "BN-1"),
    _c("h64mem-one-multi", H64_MEM, "one_stage", "multi_item", 64, 1, (1, 1), 4100, 8, "all"),
    _c("h64mem-shallow-k19", H64_MEM, "shallow", "single", 64, 19, (3, 3), 1281, 8, rows(3, 6, 8), "BN"),
    _c("h64mem-shallow-multi", H64_MEM, "shallow", "multi_item", 64, 1, (3, 3), 4100, 8, "all"),
    _c("h64mem-deepwhole-one", H64_MEM, "deep_whole", "single", 64, 1, (7, 7), 1281, 8, "all"),
    _c("h64mem-deepwhole-multi", H64_MEM, "deep_whole", "multi_item", 64, 1, (7, 7), 4100, 8, "all"),
    _c("h64mem-split8-one", H64_MEM, "deep_split8", "single", 64, 3, (7, 7), 1281, 8, rows(3, 1, 8)),
    _c("h64mem-split4-one", H64_MEM, "deep_split4", "single", 64, 1, (7, 7), 1281, 8, rows(3, 522, 8)),
    _c("h64mem-split4-multi", H64_MEM, "deep_split4", "multi_item", 64, 1, (7, 7), 4128, 8, rows(3, 1026, 8)),
    _c("h64mem-split16-one", H64_MEM, "deep_split16", "single", 65, 1, (5, 13), 1281, 8, rows(3, 1, 8)),
    _c("h64mem-split8-multi", H64_MEM, "deep_split8", "multi_item", 100, (1, 1), (7, 7), 2176, 8,
       (rows(3, 266, 8), rows(1000, 266, 8))),
    _c("h64mem-split16-multi", H64_MEM, "deep_split16", "multi_item", 65, (1, 1), (5, 13), 2112, 8,
       (rows(3, 132, 8), rows(1000, 124, 8))),
    # ---- 128-row tiles (K > 64), mask words in LDS: shallow ones only where every CU would get four full tiles ----
    _c("h128lds-one-k1000", H128_LDS, "one_stage", "single", 64, 1000, (1, 1), 128, 128, ((5, 0, 1, 127),), "BN-1", **BIG),
    _c("h128lds-shallow-k1000-1x3", H128_LDS, "shallow", "single", 64, 1000, (1, 3), 128, 128, ((5, 0, 1, 127),), "BN", **BIG),
    _c("h128lds-split8-k65", H128_LDS, "deep_split8", "single", 64, 65, (7, 7), 9, 17, "all"),
    _c("h128lds-split8-k130-mt2", H128_LDS, "deep_split8", "single", 64, 130, (7, 7), 9, 17, rows(3, 1, 17)),
    _c("h128lds-split16-c100-k100", H128_LDS, "deep_split16", "single", 100, 100, (7, 7), 9, 17, "all"),
    _c("h128lds-split16-c185-k65", H128_LDS, "deep_split16", "single", 185, 65, (7, 7), 9, 17, "all"),
    _c("h128lds-split8-3x3-bnm1", H128_LDS, "deep_split8", "single", 321, 65, E64, 20, 33, singles(20, 33, 3, 3, 13, 1, 1), "BN-1"),
    _c("h128lds-split8-3x3-bn", H128_LDS, "deep_split8", "single", 321, 65, E64, 20, 33, singles(20, 33, 3, 3, 12, 2, 2), "BN"),
    _c("h128lds-split8-3x3-bnp1", H128_LDS, "deep_split8", "single", 321, 65, E64, 20, 33, singles(20, 33, 3, 3, 13, 2, 0), "BN+1"),
    _c("h128lds-split8-3x3-one", H128_LDS, "deep_split8", "single", 321, 65, E64, 20, 33, singles(20, 33, 3, 3, 1, 0, 0), "1"),
    # (a narrow K stays on 128-row tiles on a taller map: 512 pixel tiles x 2 row tiles; 16385 listed pixels are 258 items)
    _c("h128lds-one-multi-k129", H128_LDS, "one_stage", "multi_item", 64, 129, (1, 1), 1023, 64, px(16385, 64), **BIG),
    # ---- 128-row tiles, mask words in memory (more than 1536 words) ----
    _c("h128mem-one-multi-k65", H128_MEM, "one_stage", "multi_item", 64, 65, (1, 1), 2047, 64, px(32769, 64), **BIG),
    # (66 stages at the fewest real channels: 16 chunks)
    _c("h128mem-split16-c65-w1", H128_MEM, "deep_split16", "single", 65, 65, (3, 11), 1537, 1, rows(3, 1, 1), **BIG),
    _c("h128mem-one-k1000", H128_MEM, "one_stage", "single", 64, 1000, (1, 1), 1537, 11, px(129, 11, 7), "BN+1", **BIG),
    # (a filter whose horizontal half-width is 0 on the 128-row tile)
    _c("h128mem-shallow-k1000-3x1", H128_MEM, "shallow", "single", 64, 1000, (3, 1), 1537, 11, ((9, 4, 1, 1),), "1", **BIG),
    # (a map one pixel wide, 65 channels: one real channel in the second group of 64)
    _c("h128mem-split8-c65-w1", H128_MEM, "deep_split8", "single", 65, 65, (5, 5), 1537, 1, rows(3, 1, 1)),
    # ---- group and chaining rows ----
    # (a) K = 38 and 19 on one padded tile grid, the second layer's change set empty
    _c("group-k38-k19-split16", H64_LDS, "deep_split16", "single", 185, (38, 19), (7, 7), 9, 17, (rows(3, 1, 17), ())),
    # ... and with unequal chunk counts: 33 tiles of 8 chunks beside an empty layer that takes 16
    _c("group-unequal-chunks", H64_LDS, "deep_split8", "single", 65, (3, 2), (5, 13), 40, 65, (rows(3, 28, 65), ())),
    # ... and a layer of 16 chunks beside one that changes everywhere: 96 + 61 x 8 items are more than the slabs hold, the
    # launch runs unsplit, and the first layer folds its sums at the 16 boundaries it has alone (split)
    _c("group-split16-beside-whole", H64_LDS, "deep_whole", "single", 65, (2, 1), (5, 13), 60, 65,
       (rows(3, 1, 65), "all"), "some"),
    _c("group-k38-k19-shallow", H64_LDS, "shallow", "single", 185, (38, 19), (3, 3), 9, 17, (rows(3, 1, 17), ())),
    # (b, c) consumers: one behind the first layer, two with their own filters and thresholds behind the second
    _c("cons-shallow-group", H64_LDS, "shallow", "single", 64, (64, 64), (3, 3), 20, 65,
       (((4, 10, 3, 8),), ((12, 50, 2, 15),)), next=(((1, 1, 0.05),), ((3, 3, 0.05), (7, 1, 0.3)))),
    _c("cons-split16-k100", H128_LDS, "deep_split16", "single", 100, 100, (7, 7), 9, 17, ((4, 8, 1, 1),), "1",
       next=(((3, 3, 0.05), (1, 5, 0.3)),)),
    _c("cons-shallow-k1000", H128_LDS, "shallow", "single", 64, 1000, (1, 3), 128, 128, ((5, 0, 1, 127),), "BN",
       next=(((1, 1, 0.05),),), **BIG),
    # (d, e) pooled detection (odd pool input: the last window of every row and column is clamped) and producer masks
    _c("pooled-prodmask-shallow", H64_LDS, "shallow", "single", 64, 38, (3, 3), 9, 130, ((2, 60, 3, 8),), pooled=True),
    _c("pooled-prodmask-split8", H64_LDS, "deep_split8", "single", 64, 19, (7, 7), 9, 130, ((2, 60, 3, 8),), pooled=True),
    _c("prodmask-shallow", H64_LDS, "shallow", "single", 100, 19, (3, 3), 9, 130, ((2, 60, 3, 8),), prodmask=True),
    _c("prodmask-split16", H64_LDS, "deep_split16", "single", 100, 19, (7, 7), 9, 130, ((4, 60, 1, 8),), prodmask=True),
    # (f) the upstream count: 0 (an idle frame) and not
    _c("upstream-shallow", H64_LDS, "shallow", "single", 64, 19, (3, 3), 9, 17, rows(3, 1, 17), upstream=True),
    _c("upstream-split8", H64_LDS, "deep_split8", "single", 64, 38, (7, 7), 9, 17, rows(3, 1, 17), upstream=True),
]
CASE_BY_ID = {c.id: c for c in CASES}
assert len(CASE_BY_ID) == len(CASES)
