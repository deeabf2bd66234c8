"""-m gpu: the reduce+tail launch (cbs_reduce_tail_kernel, cb_split.hip) after its loads were gathered into two request
bursts -- the launch info, W2 and b2 at entry; a group's list indices, slab quads and biases together, the
range check of the indices behind the slab requests; the workgroup's first group in a body of its own.  Every output
keeps its bits: pinned against a RECORDING, tests/golden/tail_burst.json (a SHA-256 per output), made by record() below
on the build in front of that change, and against float64 conv1x1 -> [ReLU] -> conv1x1 of the layer's output at 1e-4.

Shapes as tests/test_gpu_tail_waves.py: one frame of a 7x7 split-state layer of 32 input channels, the states at inf so
that every pixel is listed, through cbinfer_split_forward_tail with forceSplit 4 ("split": the slab sums) and 1 ("whole":
the gather path).

  * a workgroup's SECOND group: more than 16 x grid pixels -- the grid is 256 workgroups where ceil(C1/16) x S > 8 waves,
    else 512 (on 256 CUs) -- so the first group runs the body that stages W2 and the second the loop's;
  * nothing changed: the same frame again, N = 0 and SK = 1 in the launch info: layer and tail outputs keep every bit;
  * one group only (1x1, 3x5 and 4x4 maps): all other workgroups find no group;
  * the fine-grained accumulate form at N = 17."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import test_gpu_tail_waves as W
from test_gpu_split import Layer
from optest import dev, gpu_lib as lib      # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

GOLDEN_NAME = "tail_burst.json"
INFO_SK, INFO_N0 = 0, 12      # launch info words: SK, N of sequence 0 (CBS_INFO_TP + CBS_MAXSEQ)


class Big(object):
    """A case of test_gpu_tail_waves' kind on a map of its own."""

    def __init__(self, C0, C1, C2, H, W_, bias=1, relu=1, relu1=1, relu2=0):
        self.C0, self.C1, self.C2, self.H, self.W, self.N = C0, C1, C2, H, W_, H * W_
        self.bias, self.relu, self.relu1, self.relu2 = bias, relu, relu1, relu2
        self.id = "c1_%d-c0_%d-c2_%d-%dx%d-b%dr%d" % (C1, C0, C2, H, W_, bias, relu)


# second group: N > 16 x grid.  (C0, C1) -> waves: (256, 64), (256, 128) 16 -> grid 256; the others 8 or fewer -> 512.
# On a 512-workgroup grid a second group needs more than 8192 pixels, and forceSplit = 4 is honoured only while four
# partial tiles per tile fit the workspace (splits() below): with the 128-row tile and ONE row tile (C0 <= 128) the 91x91
# map still splits -- (128, 16): four waves, S = 4; (128, 128): eight waves, S = 1 -- so the loop's slab burst runs in a
# narrow workgroup too.  With the 64-row tile (C0 <= 64) no map does (more than 128 tiles x 4 > 512): there, and at
# C0 = 256 on 91x91, the second group comes by the gather path with either forceSplit.
SECOND = [Big(256, 64, 8, 65, 64), Big(256, 128, 8, 65, 64, relu1=0), Big(128, 16, 8, 91, 91), Big(128, 128, 8, 91, 91, relu=0),
          Big(32, 16, 8, 91, 91, relu2=1), Big(256, 16, 3, 91, 91, bias=0), Big(32, 64, 8, 91, 91, relu=0)]


def chain_sets(C0, C1):
    """cb_tail_chain_sets (cb_tail_core.h)."""
    groups, R = (C0 + 15) // 16, (C1 + 15) // 16
    live, S = min(groups, 4), 4 if R <= 4 else 2
    while S > 1 and not (live > 4 - 4 // S and (live - 4 // S) * R <= groups):
        S >>= 1
    return S


for _c in SECOND:
    _waves = (_c.C1 + 15) // 16 * chain_sets(_c.C0, _c.C1)
    assert _c.N > 16 * (256 if _waves > 8 else 512), _c.id
assert {(chain_sets(c.C0, c.C1), (c.C1 + 15) // 16) for c in SECOND[:4]} == {(4, 4), (2, 8), (4, 1), (1, 8)}
SMALL = [W.Case(28, 64, 256, 8, 1), W.Case(28, 64, 256, 8, 15), W.Case(28, 64, 256, 8, 16),
         W.Case(1, 16, 32, 8, 1), W.Case(1, 16, 32, 8, 15), W.Case(1, 16, 32, 8, 16)]
SAME = [Big(256, 64, 8, 10, 13), Big(32, 16, 8, 10, 13)]
FG_CASE = W.Case(1, 64, 256, 8, 17)


def digest(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes()).hexdigest()


@pytest.fixture(scope="module")
def recorded(golden_dir):
    with open(os.path.join(golden_dir, GOLDEN_NAME)) as f:
        return json.load(f)


def splits(c):
    """Whether forceSplit = 4 is honoured: four partial tiles per tile within the workspace (cbs_slab_capacity: a tile per
    tile of the map, two per CU at the least).  A map of more than 16 x 512 pixels is beyond it: there the second group
    comes by the gather path with either forceSplit."""
    bm = 64 if c.C0 <= 64 else 128
    tiles = (c.N + bm - 1) // bm * ((c.C0 + bm - 1) // bm)
    return 4 * tiles <= max(tiles, 2 * torch.cuda.get_device_properties(0).multi_processor_count)


def forward(lib, L, tail, c, x, force):
    C_ = lib.C
    L.seqs[0].input, L.seqs[0].producerMask = x.data_ptr(), None
    lib.check(C_.cbinfer_split_forward_tail(L.seqs, 1, 0, 0, 0, L.wp.data_ptr(), L.b.data_ptr(), W.C_IN, c.H, c.W, c.C0,
                                            W.KH, W.KW, W.TH, L.scale, c.relu, L.ws.data_ptr(), force,
                                            ctypes.pointer(tail.st), None))
    torch.cuda.synchronize()
    return L.ws[:64].view(torch.int32).cpu().numpy()


def run_big(lib, c, again=False):
    """{path: digest} of one case through both paths; again: the same frame a second time, which changes nothing."""
    d = W.make_inputs(c)
    tail = W.Tail(lib, c, d)
    assert lib.C.cbinfer_split_tail_supported(W.C_IN, c.C0, W.KH, W.KW, c.C1, c.C2) == 1
    x = dev(d["x"])
    got, layer_out = {}, None
    for path, force in (("split", 4), ("whole", 1)):
        L = Layer(lib, d["w"], d["b"], c.H, c.W, arith="x3")
        if not c.bias:
            L.b = W.NoBias()
        L.out[0].fill_(W.FILL)
        out = tail.fresh_out()
        info = forward(lib, L, tail, c, x, force)
        assert np.array_equal(L.list(0), np.arange(c.N, dtype=np.int32)), (c.id, path)
        assert (info[INFO_SK] > 1) == (path == "split" and splits(c)) and info[INFO_N0] == c.N, (c.id, path, info[:16])
        err = float((tail.float64(L.out[0]) - out.double()).abs().max())
        print("%s %s: SK %d, N %d, tail max |err| %.3g" % (c.id, path, info[INFO_SK], info[INFO_N0], err))
        assert err <= W.FP32_TOL, (c.id, path, err)
        got[path + "/tail"] = digest(out.cpu().numpy())
        got[path + "/layer"] = digest(L.out[0].cpu().numpy())
        if layer_out is None:
            layer_out, tail_out = L.out[0].clone(), out.clone()
        else:
            assert torch.equal(layer_out, L.out[0]) and torch.equal(tail_out, out), (c.id, "whole against split")
        if again:
            info = forward(lib, L, tail, c, x, 0)      # (no forced split: a frame without a change leaves SK = 1)
            assert info[INFO_SK] == 1 and info[INFO_N0] == 0, (c.id, path, info[:16])
            assert int(L.cnt[0].item()) == 0, (c.id, path)
            assert torch.equal(layer_out, L.out[0]) and torch.equal(tail_out, out), (c.id, path, "the unchanged frame")
            got[path + "/again/tail"] = digest(out.cpu().numpy())
            got[path + "/again/layer"] = digest(L.out[0].cpu().numpy())
    return got


def run_small(lib, c):
    return {k: digest(v) for k, v in W.run_case(lib, c).items()}


def run_fg(lib):
    return {k: digest(v) for k, v in W.run_fg_case(lib, FG_CASE).items()}


def record(path):
    """Writes the recording (to be run on the build whose bits are the reference)."""
    from cbinfer_amd import _lib
    rec = {}
    for c in SECOND:
        rec["second/" + c.id] = run_big(_lib, c)
    for c in SAME:
        rec["same/" + c.id] = run_big(_lib, c, again=True)
    for c in SMALL:
        rec["small/" + c.id] = run_small(_lib, c)
    rec["fg/" + FG_CASE.id] = run_fg(_lib)
    with open(path, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
    return rec


@pytest.mark.parametrize("c", SECOND, ids=[c.id for c in SECOND])
def test_second_group_of_a_workgroup(lib, recorded, c):
    assert run_big(lib, c) == recorded["second/" + c.id]


@pytest.mark.parametrize("c", SAME, ids=[c.id for c in SAME])
def test_unchanged_frame_keeps_every_bit(lib, recorded, c):
    assert run_big(lib, c, again=True) == recorded["same/" + c.id]


@pytest.mark.parametrize("c", SMALL, ids=[c.id for c in SMALL])
def test_one_group_in_the_whole_grid(lib, recorded, c):
    assert run_small(lib, c) == recorded["small/" + c.id]


def test_fine_grained_accumulate_form(lib, recorded):
    assert run_fg(lib) == recorded["fg/" + FG_CASE.id]
