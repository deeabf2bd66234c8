"""What the tests of the per-pixel kernel application share (CBBinary2d('aggregate'), cb_aggr.hip): the
float64 reference by shifted slices with the weight of its error bound, and the (C, G) list.  Windows, maps, footprint
and frames are the correlation layer's (tests/correlation_cases.py)."""
import numpy as np

from correlation_cases import (LIMIT_MAP, LIMIT_WINDOW_IDS, LIMIT_WINDOWS, MAPS, STRIDE_WINDOW, WINDOW_IDS,  # noqa: F401
                               WINDOWS, column_tiles, footprint, frames, shifted, strided_changes, taps)

# (C, G): below one channel tile, a tile tail, groups narrower than a tile, one channel per group
CHANNELS_GROUPS = [(5, 1), (67, 1), (40, 5), (5, 5)]
# ... under correlation_cases.LIMIT_WINDOWS (float16: the zero tile that pads the K axis at NT = 1, 3, 5 and 9)
LIMIT_CHANNELS_GROUPS = [(5, 1), (67, 1), (40, 5)]


def operands(rng, Cn, G, window, size, npdt):
    """(w [G T, H, W], v [C, H, W]), standard normal x 2 as the correlation tests' operands."""
    T = window[4] * window[5]
    return [(rng.standard_normal((n,) + tuple(size)) * 2).astype(npdt) for n in (G * T, Cn)]


def reference(w, v, window, step, G):
    """(out, S) in float64: out[c] = sum_t w[g(c) T + t] * shifted v[c], and S = sum_t |w * shifted v| over the same taps
    (a tap outside the map is zero in both), which the error bound of DESIGN 5.34 multiplies."""
    w, v = w.astype(np.float64), v.astype(np.float64)
    T = window[4] * window[5]
    wc = np.repeat(w.reshape(G, T, *w.shape[1:]), v.shape[0] // G, axis=0)      # [C, T, H, W]
    out, S = np.zeros_like(v), np.zeros_like(v)
    for t, (dy, dx) in enumerate(taps(window, step)):
        p = wc[:, t] * shifted(v, dy, dx)
        out += p
        S += np.abs(p)
    return out, S


def bound(v, ref, S, window):
    """|err| <= (T + 1) 2^-24 S; float16 adds 2^-11 |ref| + 2^-25 for the result's own rounding."""
    bar = (window[4] * window[5] + 1) * 2.0 ** -24 * S
    return bar + (2.0 ** -11 * np.abs(ref) + 2.0 ** -25 if v.dtype == np.float16 else 0.0)
