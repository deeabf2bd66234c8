"""Change-based peak suppression and peak lists (cb_peaks.hip): the numpy twin of the rule in
include/cbinfer_hip.h -- rules 1 to 5, written from the rule, not from the kernel --, the footprint, the bit packing,
the list, and the cases of tests/test_host_peaks.py and tests/test_gpu_peaks.py.

The twin compares every pixel with every neighbour of its neighbourhood, one offset at a time, with numpy's IEEE >=
(a NaN on either side gives False, +0 >= -0 and -0 >= +0 are True); float16 maps are compared in float32, which is
exact.  There is no maximum in it and no pooling: that the rule equals torch's max_pool2d formula is a test."""
import numpy as np
from optest import bits_of, np_dtype, pack      # noqa: F401  (handed on to the tests)

DTYPES = ("f32", "f16")
FORMS = ("all", "mask", "list")

# (C, H, W): the smallest shapes at which each part can go wrong
SHAPES = (
    (1, 1, 1),        # the degenerate map
    (5, 5, 70),       # two words per row, a partial word, more channels than waves
    (3, 9, 130),      # three words
    (19, 12, 64),     # exactly one full word
    (2, 3, 200),      # a short, wide map
)

# id: (kH, kW, cross, floor)
WINDOWS = {
    "w3": (3, 3, 0, None),
    "cross": (3, 3, 1, 0.1),
    "w5": (5, 5, 0, 0.3),
    "w7": (7, 7, 0, None),
    "w3x7": (3, 7, 0, 0.1),
}
WINDOW_IDS = list(WINDOWS)


# ------------------------------------------------------------------------------------------------ the rule
def offsets(kH, kW, cross):
    """Rule 1: the offsets (dy, dx) of the neighbourhood, the centre left out (v >= v holds unless v is a NaN)."""
    if cross:
        assert (kH, kW) == (3, 3)
        return [(-1, 0), (1, 0), (0, -1), (0, 1)]
    return [(dy, dx) for dy in range(-(kH // 2), kH // 2 + 1) for dx in range(-(kW // 2), kW // 2 + 1) if (dy, dx) != (0, 0)]


def keep(v, kH, kW, cross, floor):
    """Rule 2: bool [C, H, W]."""
    _, H, W = v.shape
    f = v.astype(np.float32)
    with np.errstate(invalid="ignore"):
        k = f >= f      # (the centre is a member of its neighbourhood: False for a NaN)
        for dy, dx in offsets(kH, kW, cross):
            # the pixels (y, x) whose neighbour (y + dy, x + dx) lies in the map; every other pixel skips this offset
            y0, y1 = max(0, -dy), min(H, H - dy)
            x0, x1 = max(0, -dx), min(W, W - dx)
            if y0 >= y1 or x0 >= x1:
                continue
            k[:, y0:y1, x0:x1] &= f[:, y0:y1, x0:x1] >= f[:, y0 + dy:y1 + dy, x0 + dx:x1 + dx]
        if floor is not None:
            k &= f >= np.float32(floor)
    return k


def suppressed(v, k):
    """Rule 3: the bits of v where k holds, +0 elsewhere."""
    out = np.zeros_like(v)
    out[k] = v[k]
    return out


def twin(v, window):
    """(out, keep) of the map v [C, H, W] under WINDOWS[window]."""
    kH, kW, cross, floor = WINDOWS[window]
    k = keep(v, kH, kW, cross, floor)
    return suppressed(v, k), k


def peak_bits(k):
    """Rule 4: bool [C, H, W] -> C cbinfer_mask_words(H, W) words, channel after channel."""
    return np.concatenate([pack(k[c]) for c in range(k.shape[0])])


def peak_list(v, k):
    """Rule 5: (entries int32 [n, 3], scores [n] of v's dtype, count, channelStart int32 [C + 1]) -- channel after
    channel, row after row, the columns of a row ascending."""
    Cn, H, _ = v.shape
    entries, scores, start = [], [], [0]
    for c in range(Cn):
        for y in range(H):
            for x in np.flatnonzero(k[c, y]):
                entries.append((c, y, int(x)))
                scores.append(v[c, y, x])
        start.append(len(entries))
    return (np.array(entries, dtype=np.int32).reshape(-1, 3), np.array(scores, dtype=v.dtype), len(entries),
            np.array(start, dtype=np.int32))


def footprint(changed, kH, kW):
    """The pixels whose kH x kW window (stride 1, padding k / 2) holds a changed pixel: bool [H, W]."""
    H, W = changed.shape
    out = np.zeros((H, W), dtype=bool)
    for y, x in zip(*np.nonzero(changed)):
        out[max(0, y - kH // 2):y + kH // 2 + 1, max(0, x - kW // 2):x + kW // 2 + 1] = True
    return out


# ------------------------------------------------------------------------------------------------ values
VALUE_SETS = ("random", "quantised", "special", "f16max")


def value_sets(dtype):
    """f16max holds float16's largest finite magnitudes: it has no float32 form."""
    return VALUE_SETS if dtype == "f16" else VALUE_SETS[:3]


def values(kind, rng, shape, dtype):
    dt = np_dtype(dtype)
    if kind == "random":          # heat-map like: the floors of WINDOWS cut some of them
        return rng.random(shape).astype(dt)
    if kind == "quantised":       # four levels: plateaus and exact ties everywhere
        return (rng.integers(0, 4, shape) / 4.0).astype(dt)
    if kind == "special":
        tiny = np.finfo(dt).smallest_subnormal
        pool = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, tiny, -tiny, 3 * tiny, 0.5, 0.25, -0.5, 1.0], dtype=dt)
        return rng.choice(pool, shape)
    assert kind == "f16max" and dtype == "f16"
    return rng.choice(np.array([65504.0, 65472.0, -65504.0, -65472.0, 65504.0, 0.0], dtype=np.float16), shape)


# what the frames below put on top of a set's values: four heights above every finite value of "random" and "quantised"
TOPS = (2.0, 3.0, 4.0, 5.0)


# ------------------------------------------------------------------------------------------------ frames
def sites(H, W, rW):
    """Where the neighbour frames act, or None where the map has no room: R, the standing peak -- at x = 63 where a row
    has two words --, Q, its neighbour in the row (x = 64), P, the last pixel of the row that still sees Q and does not
    see R, and D, the pixel below R (None in a one-row map)."""
    if W < 2 + rW:
        return None
    xa = min(63, W - 2 - rW)
    return (0, xa), (0, xa + 1), (0, xa + 1 + rW), ((1, xa) if H > 1 else None)


def patterns(H, W, rW):
    """(label, bool [H, W]) of consecutive frames: the six mask patterns -- empty, one pixel, a corner, bit 63 / bit 64,
    a full row, dense -- and then the two frames in which ONLY the neighbour of a standing peak changes: across a word
    boundary (peak at x = 63, changed pixel at x = 64), and across a row."""
    Z = np.zeros((H, W), dtype=bool)
    one, corner, edge, row = Z.copy(), Z.copy(), Z.copy(), Z.copy()
    one[H // 2, W // 2] = True
    corner[H - 1, W - 1] = True
    if W > 64:
        edge[0, 63] = edge[0, 64] = edge[H - 1, 63] = edge[H - 1, 64] = True
    else:
        edge[0, W - 1] = edge[H - 1, 0] = True
    row[H // 2, :] = True
    out = [("empty", Z), ("one pixel", one), ("corner", corner), ("bit 63/64", edge), ("full row", row), ("dense", ~Z)]
    s = sites(H, W, rW)
    if s is not None:
        beside, below = Z.copy(), Z.copy()
        beside[s[1]] = True
        out.append(("neighbour in the row", beside))
        if s[3] is not None:
            below[s[3]] = True
            out.append(("neighbour in the row below", below))
    return out


def frames(shape, kind, dtype, window, seed=0):
    """[(label, changed [H, W], x [C, H, W])]: x of a frame differs from x of the frame before it exactly at the changed
    pixels (all channels; the first frame's predecessor is a map of the set's values).  The sites depend on the window's
    width.  The dense frame leaves R = TOPS[2], Q = TOPS[1] and P = TOPS[0] above everything else: R is a peak, Q is
    suppressed by R, P by Q alone.  The frame after it gives only Q a value of the set: R stays a peak and P BECOMES one
    though its value stands.  The last frame raises only D, below R, to TOPS[3]: R STOPS being a peak though its value
    stands."""
    Cn, H, W = shape
    rW = WINDOWS[window][1] // 2
    rng = np.random.default_rng(seed + 1000 * SHAPES.index(shape) + 10 * VALUE_SETS.index(kind))
    x = values(kind, rng, shape, dtype)
    s = sites(H, W, rW)
    out = []
    for label, S in patterns(H, W, rW):
        fresh = values(kind, rng, shape, dtype)
        x = x.copy()
        x[:, S] = fresh[:, S]
        if label == "dense" and s is not None:
            for site, top in zip(s[:3], (TOPS[2], TOPS[1], TOPS[0])):
                x[(slice(None),) + site] = top
        elif label == "neighbour in the row below":
            x[(slice(None),) + s[3]] = TOPS[3]
        out.append((label, S, x))
    return out


def listed(S, window, form):
    """The pixels a frame with the changed pixels S lists: the footprint, or every pixel."""
    kH, kW, _, _ = WINDOWS[window]
    return np.ones(S.shape, dtype=bool) if form == "all" else footprint(S, kH, kW)
