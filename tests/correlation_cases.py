"""What the tests of the correlation layer share (CBBinary2d('correlate'), cb_corr.hip): the float64
reference by shifted slices, the exact numpy footprint, and the parameter lists."""
import numpy as np

# displacement=, step= and the (y0, y1, x0, x1, Dy, Dx) they resolve to
WINDOWS = [(4, 1, (-4, 4, -4, 4, 9, 9)), ((2, 6), 2, (-2, 2, -6, 6, 3, 7)), (20, 2, (-20, 20, -20, 20, 21, 21)),
           (((0, 0), (-10, 0)), 1, (0, 0, -10, 0, 1, 11))]
WINDOW_IDS = ["r4", "r2x6s2", "r20s2", "stereo10"]
# 7x70: a second mask word of 6 pixels, a 16-group cut by the row end, rows wholly outside for radius 4; 3x16: one exact
# group
MAPS = [(7, 70), (3, 16)]
CHANNELS = [5, 67]      # below one k-step, and a chunk tail
# The column tile counts the four above never reach (they span 8, 12, 40 and 10 columns: NT = 2, 2, 4, 2): NT = 1, 3, 5, 9,
# every odd one and both ends of the NTMAX = 9 kernels; stereo64 and r8x64s8 put taps at +-64, a whole-word shift of the
# footprint.  LIMIT_MAP has three mask words per row (the word before and behind a tap's), a 16-group cut by the row end
# (150 = 2 x 64 + 16 + 6) and taps at +-64 inside the map.
LIMIT_WINDOWS = [(((-2, 2), (0, 0)), 1, (-2, 2, 0, 0, 5, 1)), ((1, 12), 1, (-1, 1, -12, 12, 3, 25)),
                 (((0, 0), (-64, 0)), 1, (0, 0, -64, 0, 1, 65)), (((-8, 8), (-64, 64)), 8, (-8, 8, -64, 64, 3, 17))]
LIMIT_WINDOW_IDS = ["column5", "r1x12", "stereo64", "r8x64s8"]
LIMIT_MAP = (5, 150)
# the window of the grid-stride tests (tests/test_gpu_window_limits.py)
STRIDE_WINDOW = ((1, 2), 1, (-1, 1, -2, 2, 3, 5))


def column_tiles(window):
    """NT of the kernels: the 16-column tiles of b's row that a group of 16 pixels meets."""
    return (16 + window[3] - window[2] + 15) // 16


def taps(window, step):
    y0, y1, x0, x1, Dy, Dx = window
    return [(y0 + i * step, x0 + j * step) for i in range(Dy) for j in range(Dx)]


def shifted(m, dy, dx):
    """s[..., y, x] = m[..., y + dy, x + dx], zero (False) where that lies outside the map."""
    H, W = m.shape[-2:]
    s = np.zeros_like(m)
    ys, xs = slice(max(0, -dy), min(H, H - dy)), slice(max(0, -dx), min(W, W - dx))
    if ys.start < ys.stop and xs.start < xs.stop:
        s[..., ys, xs] = m[..., ys.start + dy:ys.stop + dy, xs.start + dx:xs.stop + dx]
    return s


def reference(a, b, window, step, normalize):
    """(out, bound weight) in float64 of a, b [C, H, W]: out[i Dx + j] = s sum_c a[c] * shifted b[c], and
    s sum_c |a[c] * shifted b[c]|, which the error bound of DESIGN 5.33 multiplies."""
    a, b = a.astype(np.float64), b.astype(np.float64)
    s = 1.0 / a.shape[0] if normalize else 1.0
    prods = [a * shifted(b, dy, dx) for dy, dx in taps(window, step)]
    return np.stack([p.sum(0) for p in prods]) * s, np.stack([np.abs(p).sum(0) for p in prods]) * s


def bound(a, ref, weight):
    """|err| <= (C + 2) 2^-24 sum_c |a_c b_c| s; float16 adds 2^-11 |ref| + 2^-25 for the result's own rounding."""
    bar = (a.shape[0] + 2) * 2.0 ** -24 * weight
    return bar + (2.0 ** -11 * np.abs(ref) + 2.0 ** -25 if a.dtype == np.float16 else 0.0)


def footprint(SA, SB, window, step):
    """Pixel p is listed iff a changed at p or b changed at an in-map p + tap."""
    out = SA.copy()
    for dy, dx in taps(window, step):
        out |= shifted(SB, dy, dx)
    return out


def pixels(H, W, *at):
    m = np.zeros((H, W), dtype=bool)
    for y, xs in at:
        m[y, xs] = True
    return m


def frames(window, step, H=7, W=70):
    """(label, form of both operands, device count, changed pixels of a, of b) of the frames on an H x W map.  The
    listed share of every frame -- by the numpy footprint alone -- stays below one half, so that no frame passes by
    recomputing everything: at radius 20 that takes a single changed pixel of b near a corner."""
    none = pixels(H, W)
    out = [("both, mask form", "mask", False, pixels(H, W, (3, slice(63, 65))), pixels(H, W, (0, 0))),
           ("both, list form", "list", False, pixels(H, W, (H - 1, W - 1)), pixels(H, W, (H - 1, W - 1))),
           ("both, list form with device count", "list", True, pixels(H, W, (1, 5)), pixels(H, W, (0, W - 4))),
           ("a only", "mask", False, pixels(H, W, (2, slice(10, 41))), none),
           ("b only", "list", True, none, pixels(H, W, (H - 2, 33))),
           ("nothing", "list", False, none, none)]
    for label, _, _, SA, SB in out:
        assert footprint(SA, SB, window, step).mean() < 0.5, (label, window)
    return out


def strided_changes(H, W, cap):
    """(changed pixels of a, of b) of the change-based frame on a map of more than `cap` rows of one mask word each, walked
    by `cap` workgroups: both operands change in rows of the first lap and in rows of the second (>= cap), idle words lie
    between them."""
    assert H >= cap + 5 and W >= 13
    return pixels(H, W, (3, 5), (cap + 2, 9)), pixels(H, W, (cap // 2, 2), (cap + 4, 12))
