"""The numpy twin and the case table of the change-based padding (cb_pad.hip), shared by
tests/test_host_pad.py and tests/test_gpu_pad.py.  The twin is the index formulas of the C header, per axis with n the
input extent, p the leading pad, o the output coordinate and i = o - p:
  constant:   i if 0 <= i < n, otherwise the pixel takes `value` and reads no input
  reflect:    i <- |i|, then i <- 2 (n - 1) - i if i >= n
  replicate:  clamp(i, 0, n - 1)
  circular:   i mod n
No torch here."""
import numpy as np

CONSTANT, REFLECT, REPLICATE, CIRCULAR = 0, 1, 2, 3      # CB_PAD_*
MODES = ("constant", "reflect", "replicate", "circular")

# (mode, (left, right, top, bottom), input (C, H, W)): the smallest shapes at which the kernel can still go wrong
STRIDED_SHAPE = (1, 2100, 5)      # with (2, 2, 1, 1): 2102 output words, more than the grid takes
CASES = [("constant", (0, 0, 0, 0), (1, 1, 1)),             # identity
         ("constant", (64, 64, 64, 64), (1, 1, 1)),         # 129x129 out of one pixel, three words per row
         ("constant", (3, 3, 1, 2), (5, 4, 60)),            # Wo = 66; C = 5: the tail of a channel group
         ("constant", (5, 0, 0, 0), (2, 3, 70)),            # output word 1 reads input columns 59.., across input words
         ("constant", (-1, 2, 2, -1), (3, 4, 6)),           # crop and pad mixed
         ("constant", (-2, -3, -1, -2), (2, 4, 6)),         # pure crop to 1x1
         ("constant", (-64, 0, 0, 0), (1, 2, 130)),         # a whole-word shift
         ("reflect", (3, 3, 3, 3), (2, 4, 4)),              # p = n - 1
         ("reflect", (1, 1, 1, 1), (4, 3, 64)),             # Wo = 66
         ("reflect", (0, 5, 2, 0), (1, 3, 62)),             # the right reflection crosses the word boundary
         ("replicate", (64, 64, 64, 64), (1, 1, 1)),
         ("replicate", (2, 64, 0, 1), (3, 2, 3)),           # a 65-bit run starting off the word boundary
         ("circular", (3, 3, 3, 3), (2, 3, 3)),             # p = n
         ("circular", (4, 1, 0, 2), (1, 5, 63))             # Wo = 68
         ] + [(mode, (2, 2, 1, 1), STRIDED_SHAPE) for mode in MODES]
CROPS = [c for c in CASES if min(c[1]) < 0]


def case_id(case):
    mode, pads, shape = case
    return "%s-%s-%s" % (mode, "_".join(str(p).replace("-", "m") for p in pads), "x".join(map(str, shape)))


def out_shape(pads, shape):
    left, right, top, bottom = pads
    Cn, H, W = shape
    return Cn, H + top + bottom, W + left + right


def source(mode, o, p, n):
    """Source coordinates of the output coordinates `o` (an int array) on an axis of n input pixels with the leading pad
    p; -1 where the pixel reads no input."""
    i = np.asarray(o, dtype=np.int64) - p
    if mode == "constant":
        return np.where((i >= 0) & (i < n), i, -1)
    if mode == "reflect":
        i = np.abs(i)
        return np.where(i >= n, 2 * (n - 1) - i, i)
    if mode == "replicate":
        return np.clip(i, 0, n - 1)
    assert mode == "circular"
    return np.mod(i, n)


def sources(mode, pads, H, W):
    """(sy [Ho], sx [Wo]) of an H x W map."""
    left, right, top, bottom = pads
    sy = source(mode, np.arange(H + top + bottom), top, H)
    sx = source(mode, np.arange(W + left + right), left, W)
    return sy, sx


def twin(mode, pads, x, value=0.0):
    """x [C, H, W] (any dtype: values are copied) -> the padded array; `value` is converted to x's dtype once."""
    Cn, H, W = x.shape
    sy, sx = sources(mode, pads, H, W)
    assert sy.size >= 1 and sx.size >= 1
    reads = (sy >= 0)[:, None] & (sx >= 0)[None, :]
    out = x[:, np.maximum(sy, 0)[:, None], np.maximum(sx, 0)[None, :]].copy()
    if not reads.all():
        with np.errstate(over='ignore'):
            fill = np.float32(value).astype(x.dtype) if x.dtype.kind == 'f' else x.dtype.type(value)
        out[:, ~reads] = fill
    return out


def footprint(mode, pads, changed):
    """The listed output pixels for the bool input map `changed` [H, W]: changed[sy, sx] where the output pixel reads an
    input pixel, False otherwise."""
    H, W = changed.shape
    sy, sx = sources(mode, pads, H, W)
    reads = (sy >= 0)[:, None] & (sx >= 0)[None, :]
    return changed[np.maximum(sy, 0)[:, None], np.maximum(sx, 0)[None, :]] & reads
