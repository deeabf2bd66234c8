"""-m gpu test of tests/optest.py's frame walk: a fake operator written in torch passes it in every form, and each of four
broken variants of the fake is caught by one of the walk's own assertions -- what the operators' own loops caught.  The
variants write wrong values to valid places; none does anything a GPU could fault on."""
import numpy as np
import pytest
import torch

from optest import bits_of, dev_words, gpu_lib as lib, pack, walk_frames      # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

SHAPE = (2, 3, 70)
BROKEN = ["dense", "working mask", "stale copy", "behind the count"]


def frames(rng, H, W):
    """Full, empty, one bit, both sides of the word boundary, random 10 % and 30 %: (label, bool [H, W])."""
    Z = np.zeros((H, W), dtype=bool)
    one, edge = Z.copy(), Z.copy()
    one[H // 2, W // 2] = True
    edge[0, 63] = edge[0, 64] = edge[H - 1, 63] = edge[H - 1, 64] = True
    return [("full", ~Z), ("empty", Z), ("one bit", one), ("word boundary", edge), ("random", rng.random((H, W)) < 0.1),
            ("random 30 %", rng.random((H, W)) < 0.3)]


def fake_operator(broken=None):
    """call() of an 'operator' that copies x to the state at the listed pixels, writes the listed set to maskCopy and
    leaves the working mask zero.  broken: 'dense' copies every pixel that differs (so also the altered unlisted one);
    'working mask' leaves a bit set; 'stale copy' writes the frame before's mask to maskCopy; 'behind the count' reads
    the list up to its capacity."""
    last = []

    def call(dx, dout, mask, lst, cap, cnt, bits, mcopy):
        Cn, H, W = dx.shape
        listed = torch.zeros(H * W, dtype=torch.bool, device="cuda")
        if mask is None and lst is None:
            listed[:] = True
        elif mask is not None:
            bit = (mask.view(H, -1, 1) >> torch.arange(64, device="cuda")) & 1
            listed = bit.bool().view(H, -1)[:, :W].reshape(-1)
        else:
            n = cap if cnt is None or broken == "behind the count" else int(cnt.item())
            entries = lst[:n].long()
            listed[entries[(entries >= 0) & (entries < H * W)]] = True
        write = (dx != dout).any(dim=0).view(-1) | listed if broken == "dense" else listed
        dout.view(Cn, -1)[:, write] = dx.view(Cn, -1)[:, write]
        words = pack(listed.view(H, W).cpu().numpy())
        last.append(words)
        mcopy.copy_(dev_words(last[-2] if broken == "stale copy" and len(last) > 1 else words))
        bits.zero_()
        if broken == "working mask":
            bits[-1] = 1
        return 0
    return call


def walk(lib, form, broken=None):
    rng = np.random.default_rng(41)
    seen = []

    def check(x, got, listed, where):
        assert np.array_equal(got[:, listed], x[:, listed]), where
        seen.append(listed.all())
    fill = np.empty(SHAPE, dtype=np.float32)
    bits_of(fill)[...] = 0x5BCD5BCD
    saw = walk_frames(lib, SHAPE, np.float32, form, lambda: frames(rng, *SHAPE[1:]), fake_operator(broken), check, fill,
                      lambda: rng.standard_normal(SHAPE).astype(np.float32))
    assert len(seen) == 6
    return saw


@pytest.mark.parametrize("form", ["all", "mask", "list"])
def test_the_walk_passes_a_correct_operator(lib, form):
    """Six frames in each form; in the forms with change information five of them have an unlisted, altered pixel."""
    assert walk(lib, form) == (0 if form == "all" else 5)


@pytest.mark.parametrize("broken", BROKEN)
def test_the_walk_catches_a_broken_operator(lib, broken):
    """Each variant raises from the walk: the unlisted pixel's bits, the working mask, maskCopy, and -- in list form, on
    a frame whose list has a device count -- the junk entries behind the count, which name the altered unlisted pixel."""
    with pytest.raises(AssertionError):
        walk(lib, "list" if broken == "behind the count" else "mask", broken)
