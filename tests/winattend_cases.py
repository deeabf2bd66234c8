"""What the tests of the partitioned window attention share (CBBinary2d('attend', partition=), cb_winattend.hip,
DESIGN.md 5.37): the float64 reference by cells with its bound's ingredients, the bound, the numpy footprint, the cases."""
import numpy as np

from attend_cases import U, default_scale  # noqa: F401

PARTITIONS = [(2, 3), (7, 7), (8, 8), (4, 16), (12, 12)]      # below one tile; a tile tail; four tiles; 4 x 16; the limit
MAPS = [(14, 21), (16, 24), (5, 70)]      # divisible by 7; by 8 but not by 7 or 12; shorter than a cell, two mask words
# (C, Cv, heads): below one k-step; d = 30; dv = 24; the limit d = dv = 64; one channel per head
SHAPES = [(5, 5, 1), (60, 60, 2), (32, 48, 2), (64, 64, 1), (6, 6, 6)]


# The cell shapes PARTITIONS leaves out (its token tile counts are NT = 1, 4, 4, 4, 9): one token; one row segment, which
# a shift lays across the mask-word boundary of a 70-wide map; NT = 2 and 3 (float16 pads 3 to 4); NT = 5, 7 and 8 of the
# large variant (float16 pads the odd ones); 144 tokens with a side of 16 -- the 31-wide and the 31-high bias table.
LIMIT_PARTITIONS = [(1, 1), (1, 16), (4, 6), (6, 7), (8, 9), (10, 10), (8, 16), (9, 16), (16, 9)]
LIMIT_MAPS = MAPS + [(33, 20)]      # ... and a map on which a 16-row cell is whole, with a clipped one beside it
LIMIT_SHAPES = [(32, 48, 2), (64, 64, 1)]      # a bias on the first; the limit d = dv = 64
# (C, Cv, heads), partition, scale of the peaked softmax (attend_cases.PEAKED has the reasoning)
PEAKED = ((8, 16, 1), (7, 7), 8.0)


def tiles(part):
    """NT of a whole cell: its 16-token tiles."""
    return (part[0] * part[1] + 15) // 16


def shifts(part):
    return [(0, 0), (part[0] // 2, part[1] // 2), (1, part[1] - 1)]


def shifts_within(part):
    """shifts(part) where a side of one pixel takes no shift: (1, 1) is left with the zero shift only."""
    return sorted({(min(sy, part[0] - 1), min(sx, part[1] - 1)) for sy, sx in shifts(part)})


def spans(n, w, s):
    """The clipped cells of one axis of n pixels: [(lo, hi)], boundaries at s + k w."""
    edges = sorted({0, n} | set(range(s or w, n, w)))
    return list(zip(edges[:-1], edges[1:]))


def cells(part, shift, size):
    return [(ys, xs) for ys in spans(size[0], part[0], shift[0]) for xs in spans(size[1], part[1], shift[1])]


def footprint(SQ, SKV, part, shift):
    """q's changes, and every pixel of a cell in which kv changed."""
    listed = SQ.copy()
    for (y0, y1), (x0, x1) in cells(part, shift, SQ.shape):
        listed[y0:y1, x0:x1] |= SKV[y0:y1, x0:x1].any()
    return listed


def operands(rng, Cn, Cv, heads, part, size, npdt, bias=None):
    """(q, kv, bias [heads, 2 Wy - 1, 2 Wx - 1] or None): q, k standard normal, v standard normal x 2, a bias on the
    multi-head shapes (bias=True: on any shape; bias='flat': handed over as [heads, (2 Wy - 1) (2 Wx - 1)])."""
    q = rng.standard_normal((Cn,) + tuple(size)).astype(npdt)
    kv = (rng.standard_normal((Cn + Cv,) + tuple(size)) * np.r_[np.ones(Cn), 2 * np.ones(Cv)][:, None, None]).astype(npdt)
    table = (rng.standard_normal((heads, 2 * part[0] - 1, 2 * part[1] - 1)).astype(np.float32)
             if heads > 1 or bias else None)
    return q, kv, table.reshape(heads, -1) if bias == 'flat' else table


def reference(q, kv, bias, part, shift, heads, scale):
    """The attention in float64, cell by cell, and what bound() multiplies -- [Cv, H, W] maps: out; A = sum_j p_j |v_j|;
    V1 = sum_j |v_j|; and [heads, H, W] maps: Q = max_j scale sum_c |q_c k_c|, R = max_j (max s - s_j), B = max |bias|,
    N = the tokens of the pixel's cell."""
    q, kv = q.astype(np.float64), kv.astype(np.float64)
    Cn, (H, W), (Wy, Wx) = q.shape[0], q.shape[1:], part
    bias = None if bias is None else bias.reshape(heads, 2 * Wy - 1, 2 * Wx - 1)      # (flattened: the same table)
    Cv = kv.shape[0] - Cn
    d, dv = Cn // heads, Cv // heads
    out, A, V1 = (np.zeros((Cv, H, W)) for _ in range(3))
    Q, R, N = (np.zeros((heads, H, W)) for _ in range(3))
    for (y0, y1), (x0, x1) in cells(part, shift, (H, W)):
        ys, xs = (a.ravel() for a in np.mgrid[y0:y1, x0:x1])
        n, box = len(ys), (slice(y0, y1), slice(x0, x1))
        for h in range(heads):
            qc, kc = (a[(slice(h * d, (h + 1) * d),) + box].reshape(d, n) for a in (q, kv))
            vc = kv[(slice(Cn + h * dv, Cn + (h + 1) * dv),) + box].reshape(dv, n)
            prod = qc[:, :, None] * kc[:, None, :]
            s = prod.sum(0) * scale
            if bias is not None:
                s = s + bias[h].astype(np.float64)[ys[:, None] - ys[None, :] + Wy - 1, xs[:, None] - xs[None, :] + Wx - 1]
            e = np.exp(s - s.max(1, keepdims=True))
            w = e / e.sum(1, keepdims=True)
            put = (slice(h * dv, (h + 1) * dv),) + box
            out[put], A[put] = (vc @ w.T).reshape(dv, y1 - y0, -1), (np.abs(vc) @ w.T).reshape(dv, y1 - y0, -1)
            V1[put] = np.abs(vc).sum(1)[:, None, None]
            # (a magnitude: under a negative scale the score's error is bounded by |scale| sum |q k| as well)
            Q[(h,) + box] = (np.abs(prod).sum(0).max(1) * abs(scale)).reshape(y1 - y0, -1)
            R[(h,) + box] = (s.max(1, keepdims=True) - s).max(1).reshape(y1 - y0, -1)
            N[(h,) + box] = n
    B = np.zeros(heads) if bias is None else np.abs(bias.astype(np.float64)).reshape(heads, -1).max(1)
    return dict(out=out, A=A, V1=V1, Q=Q, R=R, N=N, B=B[:, None, None] * np.ones((1, H, W)), d=d, dv=dv)


def bound(ref, f16):
    """DESIGN 5.37 derives it: delta = (d + 3) u Q + u B per score, eps = 2 delta + u (R + 7) per weight,
    (2 eps + (2 N + 2) u) A for the output; float16 adds DESIGN 5.36's terms: 2 x 2^-11 A + 2^-25 V1 for p rounded to f16
    and 2^-11 |out| + 2^-25 for the result's own rounding."""
    delta = (ref['d'] + 3) * U * ref['Q'] + U * ref['B']
    eps = 2 * delta + U * (ref['R'] + 7)
    bar = np.repeat(2 * eps + (2 * ref['N'] + 2) * U, ref['dv'], axis=0) * ref['A']
    if f16:
        bar = bar + 2 * 2.0 ** -11 * ref['A'] + 2.0 ** -25 * ref['V1'] + 2.0 ** -11 * np.abs(ref['out']) + 2.0 ** -25
    return bar


def swin(q, kv, bias, part, shift, heads, scale):
    """Swin's own formulation in torch float64 on a map divisible by the partition: cyclic shift by (-sy, -sx), window
    partition, scores + table bias, region mask (-inf), softmax, window reverse, shift back."""
    import torch
    (Wy, Wx), (sy, sx), Cn, (H, W) = part, shift, q.shape[0], q.shape[1:]
    nwin, ntok = (H // Wy) * (W // Wx), Wy * Wx

    def windows(x):      # [C, H, W] rolled -> [windows, heads, tokens, C / heads]
        x = torch.roll(torch.from_numpy(x.astype(np.float64)), (-sy, -sx), (1, 2))
        x = x.reshape(heads, -1, H // Wy, Wy, W // Wx, Wx).permute(2, 4, 0, 3, 5, 1)
        return x.reshape(nwin, heads, ntok, -1)
    region = torch.zeros(1, H, W, dtype=torch.float64)
    for i, ys in enumerate((slice(0, -Wy), slice(-Wy, -sy or None), slice(-sy or H, None))):
        for j, xs in enumerate((slice(0, -Wx), slice(-Wx, -sx or None), slice(-sx or W, None))):
            region[:, ys, xs] = 3 * i + j
    region = region.reshape(1, 1, H // Wy, Wy, W // Wx, Wx).permute(2, 4, 0, 3, 5, 1).reshape(nwin, 1, ntok)
    s = windows(q) @ windows(kv[:Cn]).transpose(2, 3) * scale
    if bias is not None:
        cy, cx = (a.ravel() for a in np.mgrid[0:Wy, 0:Wx])
        index = (cy[:, None] - cy[None, :] + Wy - 1) * (2 * Wx - 1) + cx[:, None] - cx[None, :] + Wx - 1
        s = s + torch.from_numpy(bias.astype(np.float64)).reshape(heads, -1)[:, index][None]
    s = s.masked_fill((region[:, :, :, None] != region[:, :, None, :]), float('-inf'))
    o = torch.softmax(s, -1) @ windows(kv[Cn:])
    o = o.reshape(H // Wy, W // Wx, heads, Wy, Wx, -1).permute(2, 5, 0, 3, 1, 4).reshape(-1, H, W)
    return torch.roll(o, (sy, sx), (1, 2)).numpy()
