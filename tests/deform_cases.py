"""The deformable convolution's cases, planted field values, float64 reference with footprint, and bound."""
import numpy as np

# (kH, kW, sH, sW, pH, pW, dH, dW)
GEOMS = {"3x3": (3, 3, 1, 1, 1, 1, 1, 1), "3x3s2": (3, 3, 2, 2, 1, 1, 1, 1), "3x3d2": (3, 3, 1, 1, 2, 2, 2, 2),
         "1x1": (1, 1, 1, 1, 0, 0, 1, 1), "2x3": (2, 3, 1, 1, 0, 0, 1, 1)}
HI, WI = 9, 70      # two mask words per row, a 6-column tail
# (geometry, (C, Go, K), modulation, bias, relu, dtype of x, dtype of the field, (form of x, form of the field))
CASES = [("3x3", (8, 1, 8), None, True, False, "f32", "f32", ("all", "all")),
         ("3x3", (16, 4, 8), "sigmoid", True, False, "f32", "f32", ("mask", "mask")),
         ("3x3s2", (40, 1, 72), "planes", False, True, "f32", "f32", ("list", "mask")),
         ("3x3d2", (12, 3, 8), "sigmoid", True, False, "f32", "f16", ("mask", "list")),
         ("1x1", (8, 1, 8), "planes", False, False, "f32", "f32", ("list", "list")),
         ("2x3", (16, 4, 8), None, True, False, "f32", "f32", ("list", "list")),
         ("3x3", (40, 1, 72), "sigmoid", True, False, "f16", "f16", ("mask", "mask")),
         ("3x3s2", (12, 3, 8), None, False, False, "f16", "f16", ("list", "list")),
         ("3x3d2", (8, 1, 8), "planes", True, True, "f16", "f16", ("mask", "list")),
         ("2x3", (16, 4, 8), "sigmoid", False, False, "f16", "f32", ("list", "mask"))]
ZERO_PIXEL = (2, 3)      # output pixel whose multipliers are exactly 0 and whose offsets are 0


def out_size(g, Hi=HI, Wi=WI):
    return (Hi + 2 * g[4] - g[6] * (g[0] - 1) - 1) // g[2] + 1, (Wi + 2 * g[5] - g[7] * (g[1] - 1) - 1) // g[3] + 1


def bases(geom, Go, Ho, Wo):
    """The integer base coordinates (by, bx), [Go T, Ho, Wo] each, of every (group, tap) plane pair."""
    kH, kW, sH, sW, pH, pW, dH, dW = geom
    t = np.arange(Go * kH * kW) % (kH * kW)
    by = (np.arange(Ho) * sH - pH)[None, :, None] + (t // kW * dH)[:, None, None]
    bx = (np.arange(Wo) * sW - pW)[None, None, :] + (t % kW * dW)[:, None, None]
    return np.broadcast_arrays(by, bx, np.empty((len(t), Ho, Wo)))[:2]


def field(rng, geom, Go, mod, npdt, Hi=HI, Wi=WI):
    """[F, Ho, Wo]: offsets uniform in +-3 px, multipliers in +-2; planted: exact integers that land on the map's last row
    and column, the fringe in (-1, 0), every tap outside, +-1e9, a NaN pair, at ZERO_PIXEL offsets 0 under multipliers 0."""
    Ho, Wo = out_size(geom, Hi, Wi)
    GT = Go * geom[0] * geom[1]
    by, bx = bases(geom, Go, Ho, Wo)
    f = rng.uniform(-3, 3, ((2 if mod is None else 3) * GT, Ho, Wo))
    f[2 * GT:] *= 2.0 / 3
    dy, dx = f[0:2 * GT:2], f[1:2 * GT:2]
    for (y, x), (vy, vx) in {(0, 0): (Hi - 1 - by, Wi - 1 - bx), (0, 1): (-0.5 - by, -0.25 - bx), (0, 2): (-5 - by, 2 - bx),
                             (1, 0): (1e9 + 0 * by, -1e9 + 0 * bx), (1, 1): (np.nan + 0 * by, np.nan + 0 * bx),
                             ZERO_PIXEL: (0 * by, 0 * bx)}.items():
        dy[:, y, x], dx[:, y, x] = vy[:, y, x], vx[:, y, x]
    if mod is not None:
        f[2 * GT:, ZERO_PIXEL[0], ZERO_PIXEL[1]] = 0.0 if mod == "planes" else -np.inf
    with np.errstate(over="ignore"):
        return f.astype(npdt)


def reference(x, fld, W, bias, geom, Go, mod, relu=False, xChanged=None):
    """(out, S, hit) in float64: the coordinates are formed with the specification's ONE f32 addition and clamp -- inputs
    of the sampling --, everything behind them is float64.  S = sum |W| |m| sum |w p| + |bias|, which the bound
    multiplies; hit: the output pixels one of whose counting taps lies in the bool map xChanged."""
    (Cn, Hi, Wi), K, T = x.shape, W.shape[0], geom[0] * geom[1]
    Ho, Wo = fld.shape[1:]
    GT, L = Go * T, np.float32(2.0 ** 20)
    f32 = fld.astype(np.float32)
    s = []
    for base, d in zip(bases(geom, Go, Ho, Wo), (f32[0:2 * GT:2], f32[1:2 * GT:2])):
        with np.errstate(invalid="ignore"):
            v = base.astype(np.float32) + d
            s.append(np.where(v > -L, np.minimum(v, L), -L).astype(np.float64))
    (sy, sx), X = s, x.astype(np.float64)
    m = np.ones((GT, Ho, Wo)) if mod is None else f32[2 * GT:].astype(np.float64)
    if mod == "sigmoid":
        with np.errstate(over="ignore"):
            m = 1.0 / (1.0 + np.exp(-m))
    col, mag, hit = np.zeros((Cn, T, Ho, Wo)), np.zeros((Cn, T, Ho, Wo)), np.zeros((Ho, Wo), dtype=bool)
    fy, fx, Cg = np.floor(sy), np.floor(sx), Cn // Go
    for iy, wy in ((fy, fy + 1 - sy), (fy + 1, sy - fy)):
        for ix, wx in ((fx, fx + 1 - sx), (fx + 1, sx - fx)):
            ok = (iy >= 0) & (iy < Hi) & (ix >= 0) & (ix < Wi)      # the tap counts
            yy, xx = np.clip(iy, 0, Hi - 1).astype(int), np.clip(ix, 0, Wi - 1).astype(int)
            if xChanged is not None:
                hit |= (ok & xChanged[yy, xx]).any(axis=0)
            w = np.where(ok, wy * wx, 0.0)
            for g in range(Go):
                gt, ch = slice(g * T, (g + 1) * T), slice(g * Cg, (g + 1) * Cg)
                term = w[gt] * X[ch][:, yy[gt], xx[gt]]      # [Cg, T, Ho, Wo]
                col[ch] += term
                mag[ch] += np.abs(term)
    mc = np.repeat(m.reshape(Go, T, Ho, Wo), Cg, axis=0)
    W2, b = W.astype(np.float64).reshape(K, Cn, T), (0.0 if bias is None else bias.astype(np.float64)[:, None, None])
    out = np.einsum('kct,ctyx->kyx', W2, col * mc) + b
    S = np.einsum('kct,ctyx->kyx', np.abs(W2), mag * np.abs(mc)) + np.abs(b)
    return (np.maximum(out, 0.0) if relu else out), S, hit


def bound(ref, S, W, Cn, T, mod, f16):
    """DESIGN 5.35's bound, u = 2^-24: sample 7 u, modulation 0 / 1 / 15 u, operand split and dropped products 2 u, 6 C T + 8
    accumulations, bias 1 u; float16: exact products, C T + 8 accumulations, the sample's and the result's own roundings."""
    u, n, M = 2.0 ** -24, Cn * T, {None: 0, "planes": 1, "sigmoid": 15}[mod]
    if not f16:
        return (7 + M + 2 + 6 * n + 8 + 1) * u * S + 2.0 ** -126
    sub = 2.0 ** -25 * np.abs(W.astype(np.float64)).sum(axis=(1, 2, 3))[:, None, None]      # a subnormal f16 sample
    return (2.0 ** -11 + (7 + M + n + 8 + 1) * u) * S + sub + 2.0 ** -11 * np.abs(ref) + 2.0 ** -25
