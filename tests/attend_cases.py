"""What the tests of the fused local attention share (CBBinary2d('attend'), cb_attend.hip): the float64
reference by shifted slices with its bound's ingredients, the bound, the (C, Cv, heads) list; the rest is correlate's."""
import numpy as np

from correlation_cases import MAPS, WINDOW_IDS, WINDOWS, footprint, frames, shifted, taps  # noqa: F401

# (C, Cv, heads): below one k-step; a chunk tail and a tile tail; two heads with dv = 24; one channel per head
SHAPES = [(5, 5, 1), (67, 40, 1), (32, 48, 2), (6, 6, 6)]
BORDERS = ['mask', 'zero']
U = 2.0 ** -24
# dv = 80: the second block of v with one channel tile; d = 65, dv = 100: both second blocks with tails, over two heads;
# d = dv = 128: the limit, every register of the Q fragment and two full chunks of k
LIMIT_SHAPES = [(8, 80, 1), (130, 200, 2), (128, 128, 1)]
# r4 (NT = 2) and a window of three column tiles, which float16 pads to four
LIMIT_WINDOWS = [(4, 1, (-4, 4, -4, 4, 9, 9)), (((-1, 1), (-12, 12)), 1, (-1, 1, -12, 12, 3, 25))]
# (C, Cv, heads), scale of the peaked softmax: scores of a standard deviation of 8 sqrt 8, so that some weights are zero in
# float32 and the running maximum moves by tens between displacement rows (R >= 100 somewhere on the map)
PEAKED = ((8, 16, 1), 8.0)


def operands(rng, Cn, Cv, heads, window, size, npdt, bias=None):
    """(q, kv, bias [heads, T] or None): q, k standard normal, v standard normal x 2, a bias on the multi-head shapes
    (bias=True: on any shape; bias='planes': handed over as [heads, Dy, Dx])."""
    q = rng.standard_normal((Cn,) + tuple(size)).astype(npdt)
    kv = (rng.standard_normal((Cn + Cv,) + tuple(size)) * np.r_[np.ones(Cn), 2 * np.ones(Cv)][:, None, None]).astype(npdt)
    table = rng.standard_normal((heads, window[4] * window[5])).astype(np.float32) if heads > 1 or bias else None
    return q, kv, table.reshape(heads, window[4], window[5]) if bias == 'planes' else table


def uniform_mean(kv, Cn, window, step, border):
    """What scale = 0 without a bias computes, in float64: the mean of the values at the taps that take part -- under
    'mask' the divisor is the count of in-map taps, under 'zero' all T."""
    v, tp = kv[Cn:].astype(np.float64), taps(window, step)
    total = sum(shifted(v, dy, dx) for dy, dx in tp)
    count = sum(shifted(np.ones(v.shape[1:]), dy, dx) for dy, dx in tp) if border == 'mask' else len(tp)
    return total / np.maximum(count, 1)


def default_scale(Cn, heads):
    """The module's default, d ** -0.5, as the float32 the library is handed."""
    return float(np.float32((Cn // heads) ** -0.5))


def reference(q, kv, bias, window, step, heads, border, scale):
    """The attention in float64 on the operand values, and what bound() multiplies -- a dict of [Cv, H, W] maps (one
    value per head, repeated over its channels): out; A = sum_t p_t |v_t|; V1 = sum_t |v_t| over the taps that take
    part; and of [heads, H, W] maps: Q = max_t scale sum_c |q_c k_c|, R = max_t (max s - s_t), B = max |bias|."""
    q, kv = q.astype(np.float64), kv.astype(np.float64)
    bias = None if bias is None else bias.reshape(heads, -1)      # ([heads, Dy, Dx] is the same table)
    Cn, (H, W) = q.shape[0], q.shape[1:]
    Cv = kv.shape[0] - Cn
    d, dv, tp = Cn // heads, Cv // heads, taps(window, step)
    out, A, V1 = (np.zeros((Cv, H, W)) for _ in range(3))
    Q, R = np.zeros((heads, H, W)), np.zeros((heads, H, W))
    inmap = np.stack([shifted(np.ones((H, W), dtype=bool), dy, dx) for dy, dx in tp])
    part = inmap if border == 'mask' else np.ones_like(inmap)
    for h in range(heads):
        qh, kh, vh = q[h * d:(h + 1) * d], kv[h * d:(h + 1) * d], kv[Cn + h * dv:Cn + (h + 1) * dv]
        s = np.empty((len(tp), H, W))
        for t, (dy, dx) in enumerate(tp):
            p = qh * shifted(kh, dy, dx)
            s[t] = p.sum(0) * scale
            Q[h] = np.maximum(Q[h], np.abs(p).sum(0) * abs(scale))      # (a magnitude: a negative scale has the same)
        if bias is not None:
            s = s + bias[h].astype(np.float64)[:, None, None]
        s = np.where(part, s, -np.inf)
        top = s.max(0)
        top = np.where(np.isfinite(top), top, 0.0)      # (a pixel without a tap: every weight is zero)
        e = np.exp(s - top)
        R[h] = np.where(part, top - np.where(part, s, 0.0), 0.0).max(0)
        w = e / np.where(e.sum(0) > 0, e.sum(0), 1.0)
        for t, (dy, dx) in enumerate(tp):
            vs = shifted(vh, dy, dx)
            out[h * dv:(h + 1) * dv] += w[t] * vs
            A[h * dv:(h + 1) * dv] += w[t] * np.abs(vs)
            V1[h * dv:(h + 1) * dv] += part[t] * np.abs(vs)
    B = np.zeros(heads) if bias is None else np.abs(bias.astype(np.float64)).max(1)
    return dict(out=out, A=A, V1=V1, Q=Q, R=R, B=B[:, None, None] * np.ones((1, H, W)), d=d, dv=dv)


def bound(ref, window, f16):
    """DESIGN 5.36 derives it: delta = (d + 3) u Q + u B per score, eps = 2 delta + u (2 R + 6 + 8 (Dy - 1)) per
    weight, (2 eps + (2 T + 2) u) A for the output; float16 adds 2 x 2^-11 A + 2^-25 V1 for p rounded to f16 and
    2^-11 |out| + 2^-25 for the result's own rounding."""
    rep = ref['dv']
    delta = (ref['d'] + 3) * U * ref['Q'] + U * ref['B']
    eps = np.repeat(2 * delta + U * (2 * ref['R'] + 6 + 8 * (window[4] - 1)), rep, axis=0)
    bar = (2 * eps + (2 * window[4] * window[5] + 2) * U) * ref['A']
    if f16:
        bar = bar + 2 * 2.0 ** -11 * ref['A'] + 2.0 ** -25 * ref['V1'] + 2.0 ** -11 * np.abs(ref['out']) + 2.0 ** -25
    return bar
