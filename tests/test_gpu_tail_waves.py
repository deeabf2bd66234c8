"""-m gpu: the bits of the fused 1x1 tail (cb_tail_core.h: cbs_reduce_tail_kernel of cb_split.hip, cb_tail1x1_kernel of
cb_tail.hip) pinned against a RECORDING, tests/golden/tail_waves.npz, made with the build in front of the change that
deals the first layer's four accumulation chains over waves of their own: every accumulator still receives
the same matrix instructions in the same order from zero, and the accumulators are added in the same association, so
the outputs keep every bit -- for every workgroup shape (R = ceil(C1/16) row blocks x S chain sets), both fragment
loops (up to and beyond 256 input channels), every `parts` of the second layer and its more-outputs-than-threads
branch, full and ragged pixel groups.

Per case one frame of a 7x7 split-state layer of 32 input channels on a map of exactly N pixels (the states start at
inf: every pixel is listed; 7x7 because a 3x3 filter over at most 64 channels is no deep contraction, and
cbinfer_split_forward_tail takes deep ones only), through
    cbinfer_split_forward_tail, forceSplit = 4                           ("split": the slab sums of the launch),
    cbinfer_split_forward_tail, forceSplit = 1                           ("whole": the gather path of the launch),
    cbinfer_tail1x1 on the layer's output                                ("tail1x1"),
and once through the fine-grained accumulate form (cbinfer_split_forward_fg_tail).  The inputs are seeded; the recording
holds the tail outputs only.  Each output is also checked against float64 conv1x1 -> [ReLU] -> conv1x1 of the layer's
output at the 1e-4 of tests/test_gpu_splitconv.py::test_tail_launch_against_float64.

The recording is written by record(path) below (run on the parent build), not by the code under test."""
import ctypes
import itertools
import os
import zlib

import numpy as np
import pytest
import torch

from test_gpu_split import Layer
from optest import dev, gpu_lib as lib      # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

FP32_TOL = 1e-4
TH = 0.1
FILL = 7.25
C_IN, KH, KW = 32, 7, 7
C1S = [4, 16, 17, 48, 64, 65, 128]            # R = 1, 1, 2, 3, 4, 5, 8
C0S = [32, 48, 256, 272]                      # fragment groups 2, 3, 16, 17 (the last: the second fragment loop)
C2S = [1, 8, 21]
MAPS = {1: (1, 1), 15: (3, 5), 16: (4, 4), 17: (1, 17), 130: (10, 13)}
FLAGS = [(1, 1), (0, 0), (1, 0), (0, 1)]      # the layer's (bias, ReLU)


class Case(object):
    def __init__(self, i, C1, C0, C2=None, N=None):
        self.C1, self.C0 = C1, C0
        self.C2 = C2 if C2 is not None else C2S[i % 3]
        self.N = N if N is not None else sorted(MAPS)[i % 5]
        self.H, self.W = MAPS[self.N]
        self.bias, self.relu = FLAGS[i % 4]
        self.relu1, self.relu2 = int(i % 7 != 3), i % 2
        self.id = "c1_%d-c0_%d-c2_%d-n%d-b%dr%d" % (self.C1, self.C0, self.C2, self.N, self.bias, self.relu)


def tail_form(c):
    """(R, parts, leftovers) of the second layer as cb_tail_tile derives them."""
    R, C0P, outs = (c.C1 + 15) // 16, (c.C0 + 15) // 16 * 16, c.C2 * 16
    parts = 1
    while parts < 4 and 2 * parts * outs <= 64 * R and 2 * parts * outs <= C0P * 16 and c.C1 % (2 * parts) == 0:
        parts *= 2
    return R, parts, outs > 64 * R


CASES = [Case(i, C1, C0) for i, (C1, C0) in enumerate(itertools.product(C1S, C0S))]
# (every second-layer form beside the bench's own 256 -> 64 -> 8, and the widest workgroup on the ragged group counts)
CASES += [Case(28, 64, 256, 8, 130), Case(29, 128, 256, 1, 17), Case(30, 128, 272, 21, 15), Case(31, 64, 272, 1, 1),
          Case(32, 16, 256, 1, 16), Case(33, 48, 32, 21, 130)]
CASE_BY_ID = {c.id: c for c in CASES}
assert len(CASE_BY_ID) == len(CASES)
assert {c.C2 for c in CASES} == set(C2S) and {c.N for c in CASES} == set(MAPS)
assert {tail_form(c)[0] for c in CASES} == {1, 2, 3, 4, 5, 8}
assert {tail_form(c)[1] for c in CASES} == {1, 2, 4} and any(tail_form(c)[2] for c in CASES)
FG_CASE = Case(1, 64, 256, 8, 130)            # (bias 0, relu 0: the fine-grained frame has neither)
GOLDEN_NAME = "tail_waves.npz"


@pytest.fixture(scope="module")
def recorded(golden_dir):
    return np.load(os.path.join(golden_dir, GOLDEN_NAME))


class NoBias(object):
    @staticmethod
    def data_ptr():
        return None


def make_inputs(c, tag=""):
    rng = np.random.default_rng(zlib.crc32((c.id + tag).encode()))
    d = {}
    d["w"] = (rng.standard_normal((c.C0, C_IN, KH, KW)) / np.sqrt(C_IN * KH * KW)).astype(np.float32)
    d["b"] = rng.standard_normal(c.C0).astype(np.float32)
    d["x"] = rng.standard_normal((1, C_IN, c.H, c.W)).astype(np.float32)
    d["w1"] = (rng.standard_normal((c.C1, c.C0)) / np.sqrt(c.C0)).astype(np.float32)
    d["b1"] = rng.standard_normal(c.C1).astype(np.float32)
    d["w2"] = (rng.standard_normal((c.C2, c.C1)) / np.sqrt(c.C1)).astype(np.float32)
    d["b2"] = rng.standard_normal(c.C2).astype(np.float32)
    d["x0"] = rng.standard_normal((1, C_IN, c.H, c.W)).astype(np.float32)                  # (fine-grained: old state,
    d["prev"] = rng.standard_normal((1, c.C0, c.H, c.W)).astype(np.float32)                #  old output)
    return d


class Tail(object):
    def __init__(self, lib, c, d, nOut=1):
        C_ = lib.C
        self.c = c
        self.w1, self.b1, self.w2, self.b2 = dev(d["w1"]), dev(d["b1"]), dev(d["w2"]), dev(d["b2"])
        self.w1p = torch.empty(C_.cbinfer_tail1x1_prepared_bytes(c.C1, c.C0) // 4, device="cuda")
        lib.check(C_.cbinfer_tail1x1_prep(self.w1.data_ptr(), self.w1p.data_ptr(), c.C1, c.C0, None))
        self.st = lib.SplitTail()
        self.st.w1Prepared, self.st.b1, self.st.w2, self.st.b2 = (self.w1p.data_ptr(), self.b1.data_ptr(),
                                                                  self.w2.data_ptr(), self.b2.data_ptr())
        self.st.C1, self.st.C2, self.st.relu1, self.st.relu2 = c.C1, c.C2, c.relu1, c.relu2

    def fresh_out(self):
        out = torch.full((1, self.c.C2, self.c.H, self.c.W), FILL, device="cuda")
        self.st.output[0] = out.data_ptr()
        return out

    def float64(self, y):
        """conv1x1 -> [ReLU] -> conv1x1 -> [ReLU] of y [1, C0, H, W] in double."""
        c, f = self.c, torch.nn.functional
        h = f.conv2d(y.double(), self.w1.double().view(c.C1, c.C0, 1, 1), self.b1.double())
        h = torch.relu(h) if c.relu1 else h
        o = f.conv2d(h, self.w2.double().view(c.C2, c.C1, 1, 1), self.b2.double())
        return torch.relu(o) if c.relu2 else o


def run_case(lib, c):
    """{path: tail output [C2, N]} of one case; every path checked against float64 of the layer's own output."""
    C_ = lib.C
    d = make_inputs(c)
    tail = Tail(lib, c, d)
    assert C_.cbinfer_split_tail_supported(C_IN, c.C0, KH, KW, c.C1, c.C2) == 1
    assert C_.cbinfer_tail1x1_supported(c.C0, c.C1, c.C2) == 1
    x = dev(d["x"])
    got, layer_out = {}, None
    for path, force in (("split", 4), ("whole", 1)):
        L = Layer(lib, d["w"], d["b"], c.H, c.W, arith="x3")
        if not c.bias:
            L.b = NoBias()
        L.out[0].fill_(FILL)
        out = tail.fresh_out()
        L.seqs[0].input, L.seqs[0].producerMask = x.data_ptr(), None
        lib.check(C_.cbinfer_split_forward_tail(L.seqs, 1, 0, 0, 0, L.wp.data_ptr(), L.b.data_ptr(), C_IN, c.H, c.W,
                                                c.C0, KH, KW, TH, L.scale, c.relu, L.ws.data_ptr(), force,
                                                ctypes.pointer(tail.st), None))
        torch.cuda.synchronize()
        assert np.array_equal(L.list(0), np.arange(c.N, dtype=np.int32)), (c.id, path)
        SK = int(L.ws[:8].view(torch.int32)[0].item())
        assert (SK > 1) == (path == "split"), (c.id, path, SK)
        err = float((tail.float64(L.out[0]) - out.double()).abs().max())
        print("%s %s: SK %d, tail max |err| %.3g" % (c.id, path, SK, err))
        assert err <= FP32_TOL, (c.id, path, err)
        got[path] = out.cpu().numpy().reshape(c.C2, c.N)
        if layer_out is None:
            layer_out = L.out[0].clone()
        else:
            assert torch.equal(layer_out, L.out[0]), (c.id, "the layer's output: whole against split")
    # the one-launch tail on the same columns, a device-side count below the capacity
    out = torch.full((1, c.C2, c.H, c.W), FILL, device="cuda")
    lst = torch.full((c.N + 3,), c.N + 5, dtype=torch.int32, device="cuda")
    lst[:c.N] = torch.arange(c.N, dtype=torch.int32, device="cuda")
    cnt = torch.tensor([c.N], dtype=torch.int32, device="cuda")
    lib.check(C_.cbinfer_tail1x1(layer_out.data_ptr(), lst.data_ptr(), c.N + 3, cnt.data_ptr(), tail.w1p.data_ptr(),
                                 tail.b1.data_ptr(), tail.w2.data_ptr(), tail.b2.data_ptr(), out.data_ptr(), c.C0, c.C1,
                                 c.C2, c.H, c.W, c.relu1, c.relu2, None))
    torch.cuda.synchronize()
    err = float((tail.float64(layer_out) - out.double()).abs().max())
    print("%s tail1x1: tail max |err| %.3g" % (c.id, err))
    assert err <= FP32_TOL, (c.id, "tail1x1", err)
    got["tail1x1"] = out.cpu().numpy().reshape(c.C2, c.N)
    return got


def run_fg_case(lib, c):
    """The fine-grained accumulate form: out += W delta at every pixel, the relu'd copy kept, the tail on the copy."""
    C_ = lib.C
    d = make_inputs(c, "fg")
    tail = Tail(lib, c, d)
    L = Layer(lib, d["w"], d["b"], c.H, c.W, arith="x3")
    rng = np.random.default_rng(7)
    x1 = (d["x0"] + np.where(rng.random(d["x0"].shape) < 0.5, -1.0, 1.0) * (2 * TH + np.abs(d["x"]))).astype(np.float32)
    L.state[0].copy_(dev(d["x0"]))
    L.rebuild(0)
    L.out[0].copy_(dev(d["prev"]))
    delta = torch.full((1, C_IN, c.H, c.W), FILL, device="cuda")
    relu = torch.relu(L.out[0]).clone()
    L.seqs[0].delta, L.seqs[0].reluOut = delta.data_ptr(), relu.data_ptr()
    xin = dev(x1)
    L.seqs[0].input, L.seqs[0].producerMask = xin.data_ptr(), None
    out = tail.fresh_out()
    lib.check(C_.cbinfer_split_forward_fg_tail(L.seqs, 1, 0, 0, 0, L.wp.data_ptr(), C_IN, c.H, c.W, c.C0, KH, KW, TH,
                                               L.scale, L.ws.data_ptr(), ctypes.pointer(tail.st), None))
    torch.cuda.synchronize()
    assert np.array_equal(L.list(0), np.arange(c.N, dtype=np.int32))
    assert torch.equal(relu, torch.relu(L.out[0]))
    err = float((tail.float64(relu) - out.double()).abs().max())
    print("%s fine-grained: tail max |err| %.3g" % (c.id, err))
    assert err <= FP32_TOL, (c.id, err)
    return {"fg_tail": out.cpu().numpy().reshape(c.C2, c.N), "fg_out": L.out[0].cpu().numpy().reshape(c.C0, c.N)}


def record(path):
    """Writes the recording (to be run on the build whose bits are the reference)."""
    from cbinfer_amd import _lib
    arrays = {}
    for c in CASES:
        for k, v in run_case(_lib, c).items():
            arrays[c.id + "/" + k] = v
    for k, v in run_fg_case(_lib, FG_CASE).items():
        arrays[k] = v
    np.savez(path, **arrays)
    return arrays


@pytest.mark.parametrize("cid", [c.id for c in CASES])
def test_tail_bits_as_recorded(lib, recorded, cid):
    got = run_case(lib, CASE_BY_ID[cid])
    for path in ("split", "whole", "tail1x1"):
        assert np.array_equal(got[path], recorded[cid + "/" + path]), (cid, path)
    # (one body: the launches give each other's bits too)
    assert np.array_equal(got["split"], got["whole"]) and np.array_equal(got["split"], got["tail1x1"]), cid


def test_fine_grained_tail_bits_as_recorded(lib, recorded):
    got = run_fg_case(lib, FG_CASE)
    for k in ("fg_tail", "fg_out"):
        assert np.array_equal(got[k], recorded[k]), k
