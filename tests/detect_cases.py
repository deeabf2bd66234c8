"""The front half of a frame -- change detection, dilation, compaction, the index / pool / per-value ops -- as rules and
as a case table (tests/test_host_detect.py validates both without a GPU, tests/test_gpu_detect.py runs them on the card).

THE RULES are a few lines of numpy each, bit-level where the contract is:

  changed_values   fp32: fabsf(state - in) > th in float32, strict; fp16: d = half(state - in) rounded ONCE from the exact
                   difference, d > th16 | d < -th16 with th16 = float16(float32(th)).  A NaN difference never changes.
  dilate           by (kHH, kWH), clipped to the map
  update_state     0: kept; 1: every channel of a (pre-dilation) changed pixel takes the input's bits, nothing else moves;
                   2: the state is the input, bit for bit
  pool2 / seen     the compared value of the pooled form: max over the 2x2 window clipped at the border; with a producer
                   mask a (row, word) segment is evaluated only if one of its up to four producer words is non-zero
                   (`evaluated`: a segment that is not reports no change and keeps its state, whatever the threshold)
  fg_rule          d = in - prev; delta = |d| > th ? d : 0; prev <- in where d != 0

THE CLASSIFIER (`paths`, `channel_class`) restates detect_groups and the three loop conditions of cb_detect_kernel.  It
names the cell a case exercises; no expected value comes from it.  A cell is (dtype, form, channel class, update mode).

THE DATA has teeth by construction: for every channel c < C one pixel where channel c ALONE exceeds the threshold (every
other channel of that pixel carries a non-zero sub-threshold difference, which mode 1 must copy there and nowhere else),
and a palette of deciding values -- ties, roundings, NaN, infinities, signed zeros, subnormals --, one per pixel."""
import collections
import zlib

import numpy as np

from optest import pack, raw      # noqa: F401  (handed on to the tests)

F32, F16 = "f32", "f16"
NP = {F32: np.float32, F16: np.float16}
UINT = {np.dtype(np.float32): np.uint32, np.dtype(np.float16): np.uint16}
CODE = {F32: 0, F16: 1}
OK, BADARG, UNSUPPORTED = 0, -1, -2
MAXSEQ = 8      # CBINFER_SPLIT_MAX_SEQUENCES


# ---------------------------------------------------------------------------------------------------------------------
# the rules
# ---------------------------------------------------------------------------------------------------------------------
def bits(a):
    """The values' bit patterns (what 'bit for bit' compares: NaN payloads and the sign of a zero count)."""
    return np.ascontiguousarray(a).view(UINT[a.dtype])


def changed_values(inp, state, th):
    with np.errstate(invalid="ignore", over="ignore"):
        if inp.dtype == np.float32:
            return np.abs(state - inp) > np.float32(th)
        th16 = np.float16(np.float32(th))
        d = (state.astype(np.float64) - inp.astype(np.float64)).astype(np.float16)      # exact, then ONE rounding
        return (d > th16) | (d < -th16)


def changed(inp, state, th):
    """[H, W] bool of [C, H, W] tensors."""
    return changed_values(inp, state, th).any(axis=0)


def dilate(raw, kHH, kWH):
    out = np.zeros(raw.shape, dtype=bool)
    for y, x in zip(*np.nonzero(raw)):
        out[max(0, y - kHH):y + kHH + 1, max(0, x - kWH):x + kWH + 1] = True
    return out


def update_state(state, inp, raw, mode):
    if mode == 0:
        return state.copy()
    if mode == 2:
        return inp.copy()
    out = state.copy()
    out[:, raw] = inp[:, raw]
    return out


def pool2(pre, H, W):
    """[C, pH, pW] -> [C, H, W]: max over the 2x2 / stride-2 window, clipped at the border; rows and columns beyond 2H /
    2W (floor mode, odd size) belong to no window."""
    C, pH, pW = pre.shape
    pad = np.full((C, 2 * H, 2 * W), -np.inf, dtype=pre.dtype)
    hh, ww = min(pH, 2 * H), min(pW, 2 * W)
    pad[:, :hh, :ww] = pre[:, :hh, :ww]
    return pad.reshape(C, H, 2, W, 2).max(axis=(2, 4))


def touched_segments(prod, pH, pW, H, W):
    """[H, words per row] bool: the 64-pixel segments of the pooled map one of whose producer words is non-zero."""
    pwpr, wpr = (pW + 63) // 64, (W + 63) // 64
    p = prod.reshape(pH, pwpr)
    out = np.zeros((H, wpr), dtype=bool)
    for y in range(H):
        for t in range(wpr):
            out[y, t] = p[2 * y:min(2 * y + 2, pH), 2 * t:min(2 * t + 2, pwpr)].any()
    return out


def seen(pooled, state, touched):
    """The pooled frame as a detection with a producer mask may look at it: untouched segments compare as the state."""
    out = state.copy()
    for y, t in zip(*np.nonzero(touched)):
        out[:, y, t * 64:(t + 1) * 64] = pooled[:, y, t * 64:(t + 1) * 64]
    return out


def fg_rule(inp, prev, th, refresh):
    """(delta, per-value change, prev afterwards) of the per-value detection, float32."""
    with np.errstate(invalid="ignore", over="ignore"):
        d = inp - prev
        pred = np.abs(d) > np.float32(th)
        differs = d != 0
    delta = np.where(pred, d, np.float32(0)).astype(np.float32)
    new = prev.copy()
    if refresh:
        new[differs] = inp[differs]
    return delta, pred, new


def unpack_mask(words, H, W):
    """uint64 words -> [H, wpr * 64] bool, the bits beyond W included."""
    wpr = (W + 63) // 64
    w = np.ascontiguousarray(words).view(np.uint64)[:H * wpr]
    return np.unpackbits(w.view(np.uint8), bitorder="little").reshape(H, wpr * 64).astype(bool)


def max_pool_rule(inp, out, entries, oH, oW):
    """cbinfer_max_pool2d: the window of every listed INPUT pixel is recomputed; windows outside the output are skipped."""
    C, iH, iW = inp.shape
    out = out.copy()
    for pos in entries:
        yo, xo = (pos // iW) // 2, (pos % iW) // 2
        if yo < oH and xo < oW:
            out[:, yo, xo] = inp[:, 2 * yo:min(2 * yo + 2, iH), 2 * xo:min(2 * xo + 2, iW)].max(axis=(1, 2))
    return out


def pool_indexes_rule(entries, iW, oH, oW):
    m = np.zeros((oH, oW), dtype=bool)
    for pos in entries:
        yo, xo = (pos // iW) // 2, (pos % iW) // 2
        if yo < oH and xo < oW:
            m[yo, xo] = True
    return m


def dilate_indexes_rule(entries, H, W, kHH, kWH):
    raw = np.zeros((H, W), dtype=bool)
    for pos in entries:
        if 0 <= pos < H * W:      # (an entry outside the map is dropped)
            raw[pos // W, pos % W] = True
    return dilate(raw, kHH, kWH)


def update_fg_rule(diffs, weight, out0, coords):
    """The per-value scatter in float64: (result, sum of |w d| per element, contributions per element)."""
    K, C, kH, kW = weight.shape
    H, W = out0.shape[-2:]
    ph, pw = kH // 2, kW // 2
    out = out0.astype(np.float64).copy()
    mag, n = np.zeros_like(out), np.zeros(out.shape, dtype=np.int64)
    w64, d64 = weight.astype(np.float64), diffs.astype(np.float64).reshape(-1)
    for pos in coords:
        ci, pix = pos // (H * W), pos % (H * W)
        y, x = pix // W, pix % W
        for ky in range(kH):
            for kx in range(kW):
                yy, xx = y - ky + ph, x - kx + pw
                if 0 <= yy < H and 0 <= xx < W:
                    out[:, yy, xx] += w64[:, ci, ky, kx] * d64[pos]
                    mag[:, yy, xx] += np.abs(w64[:, ci, ky, kx] * d64[pos])
                    n[:, yy, xx] += 1
    return out, mag, n


def update_fg_bar(out0, mag, n):
    """The atomics' order is unspecified: n products rounded once each, n additions in any order, every partial sum
    bounded by |out0| + sum |w d| -- (n + 2) 2^-24 of that bound per element covers them with one unit to spare."""
    return (n + 2) * 2.0 ** -24 * (np.abs(out0.astype(np.float64)) + mag)


# ---------------------------------------------------------------------------------------------------------------------
# the classifier of cb_detect_kernel's control flow (a classifier only)
# ---------------------------------------------------------------------------------------------------------------------
def detect_groups(C):
    return min(max(C // 4, 1), 16)


def paths(C):
    """Per wave g of the C-channel launch: (main-loop iterations, 'value' or 'rem', channels handled there)."""
    G = detect_groups(C)
    keep = C <= 4 * G
    waves = []
    for g in range(G):
        c, iters = g, 0
        while c + 3 * G < C:
            c, iters = c + 4 * G, iters + 1
        waves.append((iters, "value" if (keep and c == g) else "rem", len(range(c, C, G))))
    return dict(G=G, keep=keep, waves=waves, iters=sorted({w[0] for w in waves}),
                rem_waves=[g for g, w in enumerate(waves) if w[1] == "rem" and w[2]])


def channel_class(C):
    p = paths(C)
    if p["G"] == 16 and C > 64:
        return "deep"
    if all(w[1] == "value" for w in p["waves"]):
        return "few"
    if p["iters"] == [1] and not p["rem_waves"]:
        return "quad"
    return "rem"


CHANNELS = collections.OrderedDict([
    ("few", (1, 2, 3)),                                   # G = 1, value by value
    ("quad", (4, 8, 12, 16, 60, 64)),                     # C = 4 G: one main iteration, kept registers; 3 and 15 waves
    ("rem", (5, 6, 7, 9, 11, 13, 15, 63)),                # 4 G < C < 4 G + 4: remainder on waves 0 .. C - 4 G - 1
    ("deep", (65, 70, 127, 128, 129, 185, 192, 256)),     # G = 16: one to four iterations, with / without remainder
])
FORMS = ("map", "bits", "frame0", "frame1", "after", "batched", "bits_pooled", "frame_pooled")
MODES = (0, 1, 2)
SIZES = tuple((H, W) for H in (1, 5) for W in (1, 63, 64, 65, 130))
FILTERS = ((1, 1), (7, 7), (3, 127), (129, 1))      # 3x127: kWH = 63, both spill words full; 129x1: kHH far beyond H
THRESHOLDS = {F32: (0.3, 0.3, 0.0, -1.0), F16: (0.3, 0.1, 0.0, -1.0)}      # f16(0.3) rounds up, f16(0.1) down
GEOMETRIES = ("floor-odd", "ceil-odd", "even")
PALETTE_ROOM = 24


def unreachable(cell):
    """Why a cell of dtypes x FORMS x classes x MODES has no case (None: it must have one)."""
    dtype, form, cls, mode = cell
    if form.endswith("pooled") and mode != 1:
        return "the pooled entry points take no update mode: the state is always refreshed at the changed pixels"
    if form == "batched" and dtype == F16:
        return "cbinfer_change_detection_bits_batched is an fp32 entry point"
    return None


def all_cells():
    return [(d, f, k, m) for d in (F32, F16) for f in FORMS for k in CHANNELS for m in MODES]


Case = collections.namedtuple("Case", "id dtype form cls C mode H W kH kW th variant")


def cell_of(case):
    return (case.dtype, case.form, channel_class(case.C), case.mode)


def pooled_size(case):
    g = case.variant.split("+")[0]
    return {"floor-odd": (2 * case.H + 1, 2 * case.W + 1), "ceil-odd": (2 * case.H - 1, 2 * case.W - 1),
            "even": (2 * case.H, 2 * case.W)}[g]


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _build():
    cases = []
    for cell in all_cells():
        if unreachable(cell):
            continue
        dtype, form, cls, mode = cell
        for C in CHANNELS[cls]:
            pick = _rng("case", dtype, form, C, mode)
            # the bit-mask form is the one every (dtype, C, mode) has with room for every channel's pixel AND the palette,
            # at a positive threshold; the other forms draw from all sizes that hold a pixel per channel
            room = C + (PALETTE_ROOM if form == "bits" else 0)
            sizes = [s for s in SIZES if s[0] * s[1] >= room]
            if form != "bits" and C in (1, 3):      # the one-column maps, in every form: 1x1 and 5x1
                sizes = [(1, 1)] if C == 1 else [(5, 1)]
            H, W = sizes[pick.integers(len(sizes))]
            kH, kW = FILTERS[pick.integers(len(FILTERS))]
            ths = THRESHOLDS[dtype][:2] if form == "bits" else THRESHOLDS[dtype]
            th = ths[pick.integers(len(ths))]
            variant = ""
            if form.endswith("pooled"):
                variant = GEOMETRIES[pick.integers(3)]
                if form == "bits_pooled" and pick.integers(2):
                    variant += "+prod"
            elif form == "batched":
                variant = str((2, MAXSEQ)[(CHANNELS[cls].index(C) + mode) % 2])      # both, in every class and mode
            cid = "%s-%s-c%d-m%d-%dx%d-k%dx%d-th%g%s" % (dtype, form, C, mode, H, W, kH, kW, th,
                                                         "-" + variant if variant else "")
            cases.append(Case(cid, dtype, form, cls, C, mode, H, W, kH, kW, th, variant))
    return cases


CASES = _build()
CASE_BY_ID = {c.id: c for c in CASES}


# ---------------------------------------------------------------------------------------------------------------------
# the data
# ---------------------------------------------------------------------------------------------------------------------
def palette(dtype, th, pooled=False):
    """[(name, state value, input value, verdict the issue states or None, every channel?)] -- one deciding pair per
    pixel.  The verdicts are what the contract says in words; the expected values of the tests come from the rules."""
    dt = NP[dtype]
    nan, inf = dt(np.nan), dt(np.inf)
    if dtype == F32:
        nan = np.array([0x7fc12345], dtype=np.uint32).view(np.float32)[0]      # (a payload mode 2 must carry over)
    out = []
    if th > 0:
        t = dt(np.float32(th))
        ulp = np.spacing(t)
        up, down = dt(t + ulp), dt(t - ulp)
        out += [("exact-th", t, 0, False), ("ulp-above", up, 0, True), ("neg-exact-th", -t, 0, False),
                ("neg-ulp-above", -up, 0, True), ("inf-finite", inf, 1, True), ("inf-inf", inf, inf, False),
                ("zero-signs", 0.0, -0.0, False)]
        if dtype == F32:
            # th + 2^-30 is above th in exact arithmetic and rounds ONTO it in f32; th + (half an ulp and a bit) rounds up
            out += [("rounds-onto-th", t, -2.0 ** -30, False), ("rounds-above-th", t, -(float(ulp) / 2 + 2.0 ** -30), True)]
        else:
            odd = bool(int(np.array([t]).view(np.uint16)[0]) & 1)
            out += [("ulp-below", down, 0, False),
                    ("quarter-above-rounds-onto-th", t, -float(ulp) / 4, False),      # exact difference above th16
                    ("quarter-below-next", up, float(ulp) / 4, True),
                    ("tie-above", t, -float(ulp) / 2, odd),      # nearest EVEN: up only from an odd significand
                    ("tie-below", t, float(ulp) / 2, False)]     # ... to th16 - ulp (odd) or onto th16 (even)
        if not pooled:      # (cb_max promises nothing about a NaN in a window)
            out += [("nan-in", 1, nan, False), ("nan-state", nan, 1, False)]
    elif th == 0:
        tiny = 1e-40 if dtype == F32 else 2.0 ** -24      # a subnormal of the format
        out += [("subnormal", tiny, 0, True), ("neg-subnormal", 0, tiny, True), ("zero-signs", 0.0, -0.0, False),
                ("inf-inf", inf, inf, False)]
        if not pooled:
            out += [("nan-in", 1, nan, False)]
    else:
        out += [("equal", 1, 1, True), ("inf-finite", inf, 1, True)]
        if not pooled:
            out += [("nan-all", 1, nan, False, True)]
    return [(e[0], dt(e[1]), dt(e[2]), e[3], len(e) > 4) for e in out]


def make(case, q=0):
    """The data of sequence q of a case: state and input [C, H, W] (for a pooled form: the values the windows hold),
    `solo` [(c, y, x)]: channel c alone decides pixel (y, x), `planted` [(name, y, x, verdict)], and for the pooled forms
    `pre` [C, pH, pW], `prod` (uint64 words or None) and `positions` (the window position that holds each solo value)."""
    C, H, W, th = case.C, case.H, case.W, case.th
    dt = NP[case.dtype]
    rng = _rng("data", case.id, q)
    pooled = case.form.endswith("pooled")
    state = rng.uniform(-2, 2, (C, H, W)).astype(dt)
    if th > 0:
        drift = rng.uniform(-0.4, 0.4, (C, H, W)) * th
        drift[rng.random((C, H, W)) < 0.3] = 0
    elif th == 0:
        drift = np.zeros((C, H, W))
    else:
        drift = rng.uniform(-0.5, 0.5, (C, H, W))
    inp = (state.astype(np.float64) + drift).astype(dt)
    order = rng.permutation(H * W)
    solo, planted = [], []
    if th >= 0 and H * W >= C:
        for c in range(C):
            y, x = divmod(int(order[c]), W)
            if th > 0:      # every other channel: a non-zero difference below the threshold
                d = rng.uniform(0.1, 0.4, C) * th * rng.choice([-1, 1], C)
                inp[:, y, x] = (state[:, y, x].astype(np.float64) + d).astype(dt)
            big = (1.5 + rng.random()) * max(th, 0.05) * (-1 if c & 1 else 1)
            inp[c, y, x] = dt(float(state[c, y, x]) + big)
            solo.append((c, y, x))
    pal = palette(case.dtype, th, pooled)
    first = len(solo)
    if H * W >= first + len(pal):
        for i, (name, s, v, verdict, every) in enumerate(pal):
            y, x = divmod(int(order[first + i]), W)
            inp[:, y, x] = state[:, y, x]
            c = slice(None) if every else (7 * i + 3) % C
            state[c, y, x], inp[c, y, x] = s, v
            planted.append((name, y, x, verdict))
    out = dict(state=state, inp=inp, solo=solo, planted=planted, pre=None, prod=None, positions=[])
    if pooled:
        pH, pW = pooled_size(case)
        pre = np.full((C, pH, pW), 1000.0, dtype=dt)      # (beyond the last window: a decoy no window may read)
        # position k = (c + y + x) mod (positions the border leaves the window) holds the value, the others lie below it
        cc, yy, xx = np.ogrid[:C, :H, :W]
        nj, ni = np.where(2 * yy + 1 < pH, 2, 1), np.where(2 * xx + 1 < pW, 2, 1)
        k = (cc + yy + xx) % (nj * ni)
        with np.errstate(invalid="ignore", over="ignore"):
            low = (inp.astype(np.float64)[None] - 0.5 - rng.random((4, C, H, W))).astype(dt)
        for j in (0, 1):
            for i in (0, 1):
                val = np.where(k == j * ni + i, inp, low[2 * j + i])
                ys, xs = np.flatnonzero(2 * np.arange(H) + j < pH), np.flatnonzero(2 * np.arange(W) + i < pW)
                pre[np.ix_(np.arange(C), 2 * ys + j, 2 * xs + i)] = val[np.ix_(np.arange(C), ys, xs)]
        for c, y, x in solo:
            n = int(nj[0, y, 0] * ni[0, 0, x])
            out["positions"].append((divmod(int(k[c, y, x]), int(ni[0, 0, x])), n))
        out["pre"] = pre
        if case.variant.endswith("+prod"):
            pwpr, wpr = (pW + 63) // 64, (W + 63) // 64
            touch = rng.random((H, wpr)) < 0.5
            touch.flat[0] = True
            if touch.size > 1:
                touch.flat[-1] = False
            for y, t in zip(*np.nonzero(~touch)):      # the decoy: every window value of channel 0 raised by 5
                pre[0, 2 * y:2 * y + 2, 128 * t:128 * t + 2] += dt(5)
                inp[0, y, 64 * t] = dt(float(inp[0, y, 64 * t]) + 5)
            prod = np.zeros((pH, pwpr), dtype=np.uint64)
            for y, t in zip(*np.nonzero(touch)):
                words = [(2 * y + j, 2 * t + i) for j in (0, 1) for i in (0, 1) if 2 * y + j < pH and 2 * t + i < pwpr]
                yy, ww = words[rng.integers(len(words))]
                prod[yy, ww] = np.uint64(1) << np.uint64(rng.integers(min(64, pW - 64 * ww)))
            out["prod"] = prod.reshape(-1)
    return out


def compared(case, d):
    """The [C, H, W] values a case's detection compares with its state."""
    if not case.form.endswith("pooled"):
        return d["inp"]
    pooled = pool2(d["pre"], case.H, case.W)
    if d["prod"] is None:
        return pooled
    pH, pW = pooled_size(case)
    return seen(pooled, d["state"], touched_segments(d["prod"], pH, pW, case.H, case.W))


def evaluated(case, d):
    """[H, W] bool: the pixels a case's detection evaluates at all -- with a producer mask, those of the touched segments
    (a segment that is not evaluated reports no change, whatever the threshold: below zero too)."""
    if d["prod"] is None:
        return np.ones((case.H, case.W), dtype=bool)
    pH, pW = pooled_size(case)
    return np.repeat(touched_segments(d["prod"], pH, pW, case.H, case.W), 64, axis=1)[:, :case.W]


def expect(case, d):
    """(raw change map, dilated mask, state afterwards) by the rules."""
    x = compared(case, d)
    raw = changed(x, d["state"], case.th) & evaluated(case, d)
    return raw, dilate(raw, case.kH // 2, case.kW // 2), update_state(d["state"], x, raw, case.mode)


# ---------------------------------------------------------------------------------------------------------------------
# compaction: the masks
# ---------------------------------------------------------------------------------------------------------------------
# (name, H, W): 1, 63, 64, 65 and 130 words; 65 and 130 leave the last workgroup a partial set of words, the last word of
# 4097 and 4150 columns holds 1 and 54 valid bits; 1920 words: the eight-deep prefix loop runs once for the last
# workgroups, 3968 words (62 x 4096 pixels): twice
COMPACT_MASKS = (("1w", 1, 64), ("1w-partial", 1, 37), ("63w", 1, 63 * 64), ("64w", 1, 4096), ("65w", 1, 4097),
                 ("130w", 2, 4150), ("1920w", 30, 4096), ("3968w", 62, 4096))
COMPACT_CONTENTS = ("empty", "full", "last-bit", "random")
FLAT_NUMELS = (1, 63, 64, 65, 4097, 250001)


def compact_mask(H, W, content):
    m = np.zeros((H, W), dtype=bool)
    if content == "full":
        m[:] = True
    elif content == "last-bit":
        m[H - 1, W - 1] = True
    elif content == "random":
        m = _rng("compact", H, W).random((H, W)) < 0.3
        m[H - 1, W - 1] = True
    return m


# ---------------------------------------------------------------------------------------------------------------------
# the index, pool and per-value ops: shapes and data
# ---------------------------------------------------------------------------------------------------------------------
# (C, iH, iW, ceil): odd sizes in floor mode skip the last row / column, in ceil mode clip the last windows
POOL_SHAPES = ((1, 5, 7, False), (3, 5, 7, True), (3, 6, 8, False), (2, 9, 131, True), (2, 9, 131, False), (2, 1, 1, True))


def pool_data(C, iH, iW, ceil, dtype):
    """Input, pre-filled output, an ascending list with several pixels per window and entries in the last row and column,
    and a device count below the list's length."""
    rng = _rng("pool", C, iH, iW, ceil, dtype)
    dt = NP[dtype]
    oH, oW = ((iH + 1) // 2, (iW + 1) // 2) if ceil else (max(iH // 2, 1), max(iW // 2, 1))
    inp = rng.standard_normal((C, iH, iW)).astype(dt)
    out0 = rng.standard_normal((C, oH, oW)).astype(dt)
    sel = rng.random(iH * iW) < 0.4
    sel[[0, iW - 1, (iH - 1) * iW, iH * iW - 1]] = True
    sel[:min(4, iW)] = True      # (a run of neighbours: both pixels of a window's row are listed)
    entries = np.flatnonzero(sel).astype(np.int32)
    return dict(inp=inp, out0=out0, entries=entries, n_dev=max(len(entries) - 3, 0), oH=oH, oW=oW)


FG_NUMVALS = 1000      # not a multiple of the 256 threads of a workgroup
FG_TH = 0.3


def fg_data():
    rng = _rng("fg")
    prev = rng.uniform(-2, 2, FG_NUMVALS).astype(np.float32)
    inp = (prev + rng.uniform(-0.6, 0.6, FG_NUMVALS)).astype(np.float32)
    planted = []
    for i, (name, s, v, verdict, _) in enumerate(palette(F32, FG_TH)):
        prev[11 * i + 5], inp[11 * i + 5] = v, s      # (d = in - prev here: the pair the other way round)
        planted.append((name, 11 * i + 5, verdict))
    return inp, prev, planted


UPDATE_FG_SHAPES = ((3, 2, 5, 9, 3, 3), (2, 3, 4, 70, 5, 1), (1, 1, 1, 1, 3, 3))      # K, C, H, W, kH, kW


def update_fg_data(K, C, H, W, kH, kW):
    """Normal operands (nothing near an f32 subnormal): diffs, weights, the outputs before, the changed coordinates."""
    rng = _rng("update_fg", K, C, H, W, kH, kW)
    sgn = lambda shape: rng.choice([-1.0, 1.0], shape)
    diffs = (rng.uniform(0.35, 2, (C, H, W)) * sgn((C, H, W))).astype(np.float32)
    weight = (rng.uniform(0.1, 1, (K, C, kH, kW)) * sgn((K, C, kH, kW))).astype(np.float32)
    out0 = (rng.uniform(0.5, 3, (K, H, W)) * sgn((K, H, W))).astype(np.float32)
    sel = rng.random(C * H * W) < 0.4
    sel[[0, C * H * W - 1]] = True
    return diffs, weight, out0, np.flatnonzero(sel).astype(np.int64)
