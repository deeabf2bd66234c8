"""The change-based adaptive pool (cb_adaptpool.hip): the numpy twin of the specification in
include/cbinfer_hip.h and the cases of tests/test_host_adaptpool.py and tests/test_gpu_adaptpool.py.

The twin restates the header: torch's windows, the row-segment partials P[C][ow][H] in f32, both levels the same
reduction (L strided lane sums from +0, then a tree; the maximum keeps the first of equal values), one IEEE division, one
rounding to f16.  numpy's float32 addition and division are correctly rounded and never fused, so the twin's bits are
the specification's."""
import numpy as np
from optest import bits_of, np_dtype, pack      # noqa: F401  (handed on to the tests)

OPS = ("max", "avg")
DTYPES = ("f32", "f16")

# id: (C, H, W, output_size) -- the smallest shapes at which the kernel can still go wrong
CASES = {
    "global_two_words": (3, 7, 70, (1, 1)),       # global; the column window spans two mask words; C below 16
    "overlap_bit63": (17, 5, 130, (2, 3)),        # overlapping windows; a window across bit 63/64; three words per row
    "psp_bin": (5, 13, 129, (6, 6)),              # PSP bin; one pixel in the last word
    "classifier_7x7": (4, 9, 65, (7, 7)),         # windows of 1-2
    "identity": (2, 4, 5, (4, 5)),                # identity windows
    "smallest": (1, 1, 1, (1, 1)),                # the smallest map
    "wide_c_full_word": (70, 3, 64, (1, 2)),      # C above 64; a row of exactly one full word
    "none_axis": (3, 6, 200, (None, 1)),          # None axis; four words per row
}
CASE_IDS = list(CASES)


def lo(i, N, o):
    return (i * N) // o


def hi(i, N, o):
    return -((-(i + 1) * N) // o)


def out_size(H, W, size):
    return tuple(n if v is None else v for v, n in zip(size, (H, W)))


def lanes(N, o):
    """L of the reduction along an axis: the smallest power of two >= the longest window it can have, at most 64."""
    nmax = N // o if N % o == 0 else N // o + 2
    L = 1
    while L < nmax and L < 64:
        L *= 2
    return L


def rows_of(y, H, oh):
    """The one or two row windows that hold input row y."""
    return range((y * oh) // H, -((-(y + 1) * oh) // H))


# ------------------------------------------------------------------------------------------------ level 1
def segment_sum(x, L):
    """x: float32 [..., n], values left to right -> [...]: s_l = +0, s_l += x_k for k = l, l + L, ...; then the tree."""
    n = x.shape[-1]
    M = -(-n // L)
    v = np.zeros(x.shape[:-1] + (M * L,), dtype=np.float32)
    v[..., :n] = x      # (a lane sum is never -0, so adding the +0 of a missing value changes nothing)
    v = v.reshape(x.shape[:-1] + (M, L))
    s = np.zeros(x.shape[:-1] + (L,), dtype=np.float32)
    for m in range(M):
        s = s + v[..., m, :]
    off = L // 2
    while off >= 1:
        s = s[..., :off] + s[..., off:2 * off]
        off //= 2
    assert s.dtype == np.float32
    return s[..., 0]


def segment_max(x):
    """The first of the equal maxima (+0 == -0), a NaN wins: numpy's argmax has both rules."""
    return np.take_along_axis(x, np.argmax(x, axis=-1)[..., None], axis=-1)[..., 0]


def partials(x, ow, op):
    """x: [C, H, W] in either dtype -> P float32 [C, ow, H] (the library's layout)."""
    Cn, H, W = x.shape
    xf = x.astype(np.float32)
    L = lanes(W, ow)
    P = np.empty((Cn, ow, H), dtype=np.float32)
    for j in range(ow):
        seg = xf[:, :, lo(j, W, ow):hi(j, W, ow)]
        P[:, j, :] = segment_max(seg) if op == "max" else segment_sum(seg, L)
    return P


# ------------------------------------------------------------------------------------------------ level 2
def outputs(P, W, oh, dtype, op):
    """P [C, ow, H] -> out [C, oh, ow] in `dtype`: the same reduction over the rows of the window, top to bottom, one
    division, one rounding."""
    Cn, ow, H = P.shape
    L = lanes(H, oh)
    out = np.empty((Cn, oh, ow), dtype=np.float32)
    cols = np.array([hi(j, W, ow) - lo(j, W, ow) for j in range(ow)])
    for i in range(oh):
        r0, r1 = lo(i, H, oh), hi(i, H, oh)
        seg = P[:, :, r0:r1]
        v = segment_max(seg) if op == "max" else segment_sum(seg, L) / ((r1 - r0) * cols).astype(np.float32)[None, :]
        assert v.dtype == np.float32
        out[:, i, :] = v
    return out.astype(np_dtype(dtype))


def twin(x, size, op):
    """(partials, output) of the frame whose input is x [C, H, W]: what the state must be after ANY history."""
    Cn, H, W = x.shape
    oh, ow = out_size(H, W, size)
    P = partials(x, ow, op)
    return P, outputs(P, W, oh, "f32" if x.dtype == np.float32 else "f16", op)


def depth(rows, cols, H, W, oh, ow):
    """D: the additions on the longest path to an output whose window is rows x cols -- per level the additions of the
    longest lane sum behind its first value, and the tree."""
    L1, L2 = lanes(W, ow), lanes(H, oh)
    return (-(-cols // L1) - 1) + (L1.bit_length() - 1) + (-(-rows // L2) - 1) + (L2.bit_length() - 1)


# ------------------------------------------------------------------------------------------------ change sets
def footprint(changed, oh, ow):
    """(listed [oh, ow], dirty [H, ow]): output pixels / row segments whose window holds a changed pixel."""
    H, W = changed.shape
    dirty = np.zeros((H, ow), dtype=bool)
    for j in range(ow):
        dirty[:, j] = changed[:, lo(j, W, ow):hi(j, W, ow)].any(axis=1)
    listed = np.zeros((oh, ow), dtype=bool)
    for i in range(oh):
        listed[i] = dirty[lo(i, H, oh):hi(i, H, oh)].any(axis=0)
    return listed, dirty


def few_pixels(H, W, oh):
    """Frame 2: column 63 and 64, the last column, a row that two windows share (where the map has them)."""
    shared = [y for y in range(H) if len(rows_of(y, H, oh)) == 2]
    ys = shared[0] if shared else H // 2
    changed = np.zeros((H, W), dtype=bool)
    for y, x in ((0, 63), (ys, 64), (H - 1, W - 1), (ys, 0)):
        changed[min(y, H - 1), min(x, W - 1)] = True
    return changed


def walk(H, W, oh):
    """The five change sets of a walk: fresh (None: no state yet), a few pixels, none, every pixel, one pixel."""
    one = np.zeros((H, W), dtype=bool)
    one[H // 2, W // 3] = True
    return [None, few_pixels(H, W, oh), np.zeros((H, W), dtype=bool), np.ones((H, W), dtype=bool), one]


def frames(cid, dtype, seed=0):
    """The five inputs of a walk [C, H, W] in `dtype` and their change sets: frame k differs from frame k - 1 exactly
    at the changed pixels (all channels)."""
    Cn, H, W, size = CASES[cid]
    oh, _ = out_size(H, W, size)
    rng = np.random.default_rng(seed + 17 * CASE_IDS.index(cid))
    sets = walk(H, W, oh)
    xs = [rng.standard_normal((Cn, H, W)).astype(np_dtype(dtype))]
    for changed in sets[1:]:
        x = xs[-1].copy()
        new = rng.standard_normal((Cn, H, W)).astype(np_dtype(dtype))
        # (a new value that happens to equal the old one would still be a listed pixel: nothing depends on it)
        x[:, changed] = new[:, changed]
        xs.append(x)
    return xs, sets

