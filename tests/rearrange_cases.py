"""The numpy twins and shape tables of the change-based rearrangements (cb_rearrange.hip), shared by
tests/test_host_rearrange.py and tests/test_gpu_rearrange.py.  The values come from the index formulas of the C header,
written as index arithmetic -- not the reshape / transpose identity an implementation (or torch) would use:
  shuffle, factor r:      out[c, y r + i, x r + j] = in[c r r + i r + j, y, x]
  unshuffle, factor r:    out[c r r + i r + j, y, x] = in[c, y r + i, x r + j]
  channel shuffle, g:     out[k g + q] = in[q (C / g) + k],  q < g, k < C / g
No torch here."""
import numpy as np

SHUFFLE, UNSHUFFLE, CHANNELS = 0, 1, 2      # CB_REARRANGE_*
KINDS = ("shuffle", "unshuffle", "channels")

# shuffle (Cout, Hi, Wi, r): the input is [Cout r r, Hi, Wi]
SHUFFLE_SHAPES = [(1, 1, 1, 8),
                  (2, 3, 32, 2),       # Wo = 64: exactly one word
                  (1, 4, 22, 3),       # Wo = 66: the block of x = 21 covers bits 63..65
                  (3, 5, 13, 5),       # Wo = 65
                  (2, 2, 10, 7),       # the block of x = 9 covers bits 63..69
                  (5, 3, 9, 1),
                  (1, 1050, 9, 2)]     # 2100 output words: more than the grid takes
SHUFFLE_STRIDED = (1, 1050, 9, 2)
# unshuffle (Cin, Ho, Wo, r): the input is [Cin, Ho r, Wo r]
UNSHUFFLE_SHAPES = [(1, 1, 1, 8),
                    (2, 3, 32, 2),
                    (1, 4, 22, 3),     # output column 21 reads input bits 63..65, across two words
                    (3, 2, 65, 2),     # two output words from three input words; the last lanes have no second word
                    (2, 2, 10, 7),
                    (5, 3, 9, 1),
                    (1, 2100, 9, 2)]
UNSHUFFLE_STRIDED = (1, 2100, 9, 2)
# channel shuffle (C, g, H, W)
CHANNEL_SHAPES = [(1, 1, 1, 1), (6, 2, 3, 64), (6, 3, 5, 65), (12, 4, 1, 130), (300, 3, 4, 9),
                  (5, 5, 2, 9),        # g = C
                  (4, 1, 2, 9),
                  (2, 2, 2100, 9)]
CHANNEL_STRIDED = (2, 2, 2100, 9)


def cases():
    """(kind name, factor, input shape (C, H, W), the table's row) of every case of the three tables."""
    out = []
    for row in SHUFFLE_SHAPES:
        Co, Hi, Wi, r = row
        out.append(("shuffle", r, (Co * r * r, Hi, Wi), row))
    for row in UNSHUFFLE_SHAPES:
        Ci, Ho, Wo, r = row
        out.append(("unshuffle", r, (Ci, Ho * r, Wo * r), row))
    for row in CHANNEL_SHAPES:
        Cn, g, H, W = row
        out.append(("channels", g, (Cn, H, W), row))
    return out


STRIDED = {"shuffle": SHUFFLE_STRIDED, "unshuffle": UNSHUFFLE_STRIDED, "channels": CHANNEL_STRIDED}


def case_id(case):
    return "%s-%s" % (case[0], "x".join(map(str, case[3])))


def out_shape(kind, f, shape):
    Cn, H, W = shape
    if kind == "shuffle":
        assert Cn % (f * f) == 0
        return Cn // (f * f), H * f, W * f
    if kind == "unshuffle":
        assert H % f == 0 and W % f == 0
        return Cn * f * f, H // f, W // f
    assert Cn % f == 0
    return Cn, H, W


def twin(kind, f, x):
    """x [C, H, W] (any dtype: values are copied) -> the rearranged array, by the index formulas."""
    Co, Ho, Wo = out_shape(kind, f, x.shape)
    c = np.arange(Co)[:, None, None]
    oy = np.arange(Ho)[None, :, None]
    ox = np.arange(Wo)[None, None, :]
    if kind == "shuffle":
        return x[c * f * f + (oy % f) * f + ox % f, oy // f, ox // f]
    if kind == "unshuffle":
        rem = c % (f * f)
        return x[c // (f * f), oy * f + rem // f, ox * f + rem % f]
    return x[(c % f) * (Co // f) + c // f, oy, ox]


def footprint(kind, f, changed):
    """The listed output pixels for the bool input map `changed` [H, W]."""
    H, W = changed.shape
    if kind == "shuffle":
        return np.kron(changed, np.ones((f, f), dtype=bool)).astype(bool)
    if kind == "unshuffle":
        return changed.reshape(H // f, f, W // f, f).any((1, 3))
    return changed.copy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def special_values(rng, shape, npdt):
    """Scaled normals with -0, +-inf and NaNs of several payloads sprinkled in (compared as integers)."""
    x = (rng.standard_normal(shape) * 10).astype(npdt)
    it = np.uint32 if npdt == np.float32 else np.uint16
    flat = x.reshape(-1).view(it)
    if npdt == np.float32:
        special = [0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0x7FC12345, 0xFFC00001, 0x7F800001, 0x00000001]
    else:
        special = [0x8000, 0x7C00, 0xFC00, 0x7E00, 0x7E55, 0xFE01, 0x7C01, 0x0001]
    n = flat.size
    for k, v in enumerate(special):
        flat[(k * 7919 + 3) % n] = v
    return x
