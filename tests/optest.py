"""What the operator tests share, written once: the fixtures and conversions, the operand forms of a change-based
operator, the frame walk and the helpers of the network-level tests.  A test module imports what it needs --
    from optest import lib, pkg      # noqa: F401  (fixtures)
(a GPU module takes `gpu_lib as lib` / `gpu_pkg as pkg`, which refuse to run without a device) -- and a *_cases.py
module re-exports pack / bits_of for its callers.  tests/test_host_optest.py keeps second copies from coming back."""
import numpy as np
import pytest
import torch

__all__ = ["lib", "pkg", "gpu_lib", "gpu_pkg", "dev", "dev_words", "host_words", "raw", "bits_of", "stream", "tdtype",
           "npdtype", "np_dtype", "names_of", "mask_words", "pack", "free_pixel", "hostile_list", "operand_args", "operand",
           "walk_frames", "chain_frames", "LayerSpy", "share_of"]


# ------------------------------------------------------------------------------------------ 1. fixtures and conversions
@pytest.fixture(scope="module")
def lib():
    from cbinfer_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def pkg():
    import pycbinfer
    return pycbinfer


@pytest.fixture(scope="module")
def gpu_lib():
    from cbinfer_amd import _lib
    assert torch.cuda.is_available()
    return _lib


@pytest.fixture(scope="module")
def gpu_pkg():
    import pycbinfer
    assert torch.cuda.is_available()
    return pycbinfer


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def dev_words(words):
    return torch.from_numpy(words.view(np.int64)).cuda()


def host_words(t):
    return t.cpu().numpy().view(np.uint64)


def raw(t):
    """The bits of a tensor."""
    return t.view({torch.float32: torch.int32, torch.float16: torch.int16}.get(t.dtype, t.dtype))


def bits_of(a):
    """The integer view of a float array, of any shape and strides (an integer array is its own)."""
    a = np.asarray(a)
    return a.view({np.float32: np.uint32, np.float16: np.uint16}.get(a.dtype.type, a.dtype))


def stream():
    return torch.cuda.current_stream().cuda_stream


def tdtype(arith):
    return torch.float16 if arith in ("F16", "f16") else torch.float32


def npdtype(arith):
    return np.float16 if arith in ("F16", "f16") else np.float32


np_dtype = npdtype


def names_of(net):
    return [type(m).__name__ for m in net]


def mask_words(H, W):
    return H * ((W + 63) // 64)


def pack(mask):
    """A bool [H, W] map as the library's row-padded bit mask (uint64 words)."""
    H, W = mask.shape
    wpr = (W + 63) // 64
    pad = np.zeros((H, wpr * 64), dtype=bool)
    pad[:, :W] = mask
    return np.packbits(pad.reshape(H, wpr, 64), axis=-1, bitorder='little').reshape(-1).view('<u8').copy()


# ------------------------------------------------------------------------------------------------- 2. the operand forms
def free_pixel(listed, middle=False):
    """A pixel outside `listed`, the first or the middle one of them: a caller's junk behind a device count, or the
    pixel it alters without listing it.  None where every pixel is listed."""
    free = np.flatnonzero(~listed.reshape(-1))
    return int(free[len(free) // 2 if middle else 0]) if len(free) else None


def hostile_list(changed, junk=0, use_count=False):
    """(buffer, capacity, device count or None) of the int32 change list of the bool map `changed`: unsorted (reversed),
    with a duplicate and three entries outside the map; with a device count the buffer holds five entries behind it
    (`junk`, the caller's choice of a pixel that is not listed) that must not be read.  The tensors are kept alive by
    the caller."""
    H, W = changed.shape
    idx = np.flatnonzero(changed.reshape(-1)).astype(np.int32)[::-1]
    idx = np.concatenate([idx, idx[:1], np.array([H * W, -1, H * W + 77], dtype=np.int32)])
    if use_count:
        buf = dev(np.concatenate([idx, np.full(5, junk, dtype=np.int32)]))
        return buf, buf.numel(), dev(np.array([len(idx)], dtype=np.int32))
    return dev(idx), len(idx), None


def operand_args(form, changed, junk=0, use_count=False):
    """The ABI's (mask, list, capacity, device count) of one operand in the form 'all' / 'mask' / 'list'."""
    if form == "all":
        return None, None, 0, None
    if form == "mask":
        return dev_words(pack(changed)), None, 0, None
    return (None,) + hostile_list(changed, junk, use_count)


def operand(form, x, listed, junk=0, use_count=False):
    """What a module's forward is handed: the bare tensor ('all'), the tensor with its mask as a MaskChangeIndexes, or
    with the hostile list -- as a ChangeIndexes where it has a device count, else as a plain int32 tensor."""
    from cbinfer_amd.conv2d_cg import ChangeIndexes, MaskChangeIndexes
    H, W = listed.shape
    if form == "all":
        return x
    if form == "mask":
        return ('changeIndexes', x, MaskChangeIndexes(dev_words(pack(listed)), (H, W),
                                                      torch.empty(H * W, dtype=torch.int32, device="cuda"),
                                                      torch.zeros(1, dtype=torch.int32, device="cuda")))
    buf, _, cnt = hostile_list(listed, junk, use_count)
    return ('changeIndexes', x, buf if cnt is None else ChangeIndexes(buf, cnt, (H, W)))


# ---------------------------------------------------------------------------------------------------- 3. the frame walk
def walk_frames(lib, shape, dtype, form, frames, call, check, fill, values, what=()):
    """The frames of one operator with one operand [C, H, W] as consecutive library calls.  values() draws a map of
    `shape`: once for the first x, then once per frame; frames() -- called after the first draw, the order the operators'
    own loops had -- gives the frames' (label, bool [H, W]).  Before every frame x gets new values at the frame's pixels
    AND at one pixel outside them (the middle one of the free pixels, which is also the junk behind the device count
    that every other frame's list has); call(dx, dout, mask, lst, cap, cnt, bits, mcopy) returns the status of the
    operator's library call, check(x, got, listed, where) judges the values.  `fill` is the state before the first
    frame, of the operator's own shape and type.  After every frame: the status is 0, unlisted pixels keep their bits,
    maskCopy is the frame's mask, the working mask zero.  Returns the number of frames that had an unlisted pixel."""
    Cn, H, W = shape
    words = lib.C.cbinfer_mask_words(H, W)
    assert words == mask_words(H, W)
    x = values()
    out = fill
    dout = dev(out)
    bits = torch.zeros(words, dtype=torch.int64, device="cuda")
    mcopy = torch.full((words,), -1, dtype=torch.int64, device="cuda")
    sawUnlisted = 0
    for t, (label, S) in enumerate(frames()):
        where = (shape, np.dtype(dtype).name, form) + tuple(what) + (label,)
        fresh = values()
        x[:, S] = fresh[:, S]
        p = free_pixel(S, middle=True)
        if p is not None:      # an operand altered where the list does not say so: a dense operator would pick it up
            x[:, p // W, p % W] = fresh[:, p // W, p % W]
        listed = np.ones((H, W), dtype=bool) if form == "all" else S
        mask, lst, cap, cnt = operand_args(form, S, p or 0, bool(t % 2))
        st = call(dev(x), dout, mask, lst, cap, cnt, bits, mcopy)
        assert st == 0, where
        got = dout.cpu().numpy()
        check(x, got, listed, where)
        assert np.array_equal(bits_of(got)[..., ~listed], bits_of(out)[..., ~listed]), where
        if p is not None and not listed.all():
            sawUnlisted += 1
        assert np.array_equal(host_words(mcopy), pack(listed)), where
        assert int(bits.ne(0).sum().item()) == 0, where
        out = got
    return sawUnlisted


# ----------------------------------------------------------------------------------------- 4. the network-level helpers
def chain_frames(rng, n, npdt, H=20, W=70, C=8):
    """n frames [1, C, H, W]; a frame differs from the one before in two moved blocks only."""
    base = (rng.random((1, C, H, W)) * 2 - 1).astype(npdt)
    frames = []
    for i in range(n):
        new = base.copy()
        if i:
            for _ in range(2):
                y0, x0 = int(rng.integers(0, H)), int(rng.integers(0, W))
                blk = new[:, :, y0:y0 + 4, x0:x0 + 7]
                blk[...] = (rng.random(blk.shape) * 2 - 1).astype(npdt)
        frames.append(dev(new))
        base = new
    return frames


class LayerSpy(object):
    """Counts the launching library calls made through it (the library object's attributes are read-only function
    pointers): calls[layer][name], where `layer[0]` is what the caller's hooks last put there -- None for a caller that
    does not tell layers apart."""

    def __init__(self, real):
        self.__dict__.update(real=real, calls={}, layer=[None])

    def __getattr__(self, name):
        fn = getattr(self.real, name)
        if not getattr(fn, 'launcher', False):
            return fn

        def counted(*a):
            per = self.calls.setdefault(self.layer[0], {})
            per[name] = per.get(name, 0) + 1
            return fn(*a)
        return counted


def share_of(words, H, W):
    """The share of an [H, W] map whose bits are set in the mask `words` (a device tensor)."""
    return float(np.unpackbits(host_words(words).view(np.uint8)).sum()) / (H * W)
