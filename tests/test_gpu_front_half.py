"""-m gpu tests of the front half of the frame:

  * the mask scan of cbs_conv_kernel (cb_split.hip) where a thread owns SEVERAL chunks of mask words and the last chunk is
    a partial one -- masks larger than the workgroup, in both tile sizes, pixel order and window order, one sequence and
    two -- against the oracle's state machine (CBConv2d.forward_normal, conv2d.py:178-259): mask copy, change list and
    count, state bit for bit, outputs <= 1e-4;
  * the self-detecting row-pair launch (cbp_rowpair_kernel<7,7,true>, five workgroups per CU) at a map with fewer units
    than CUs and at one with 160 units, against the detection launch + row pairs, bit for bit."""
import ctypes
import math

import numpy as np
import pytest
import torch
from optest import dev, gpu_lib as lib      # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

FP32_TOL = 1e-4


class Layer(object):
    """Buffers of one split-state layer for nSeq sequences + the calls, as CBConv2d._forward_split makes them."""

    def __init__(self, lib, w, b, H, W, arith, nSeq=1, pooled=False):
        C_ = lib.C
        self.lib, self.nSeq, self.H, self.W, self.pooled = lib, nSeq, H, W, pooled
        K, C, kH, kW = w.shape
        self.K, self.C, self.kH, self.kW = K, C, kH, kW
        self.w, self.b = dev(w), dev(b)
        self.x3 = arith == "x3"
        if self.x3:
            self.scale = 0.0
            self.wp = torch.empty(C_.cbinfer_split3_prepared_bytes(C, K, kH, kW), dtype=torch.uint8, device="cuda")
            lib.check(C_.cbinfer_split3_prep_weights(self.w.data_ptr(), self.wp.data_ptr(), K, C, kH, kW, H, W, None))
        else:
            self.scale = 2.0 ** (13 - math.floor(math.log2(float(np.abs(w).max()))))
            self.wp = torch.empty(C_.cbinfer_split_prepared_bytes(C, K, kH, kW), dtype=torch.uint8, device="cuda")
            lib.check(C_.cbinfer_split_prep_weights(self.w.data_ptr(), self.wp.data_ptr(), K, C, kH, kW, H, W, self.scale,
                                                     None))
        words = C_.cbinfer_mask_words(H, W)
        wsb = C_.cbinfer_split_workspace_bytes(nSeq, C, H, W, K, kH, kW)
        self.ws = torch.zeros(wsb, dtype=torch.uint8, device="cuda") if wsb else None
        self.seqs = (lib.SplitSeq * nSeq)()
        self.state, self.S, self.masks, self.out, self.idx, self.cnt, self.copy = [], [], [], [], [], [], []
        self.flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        a = (C, H, W, kH, kW)
        for q in range(nSeq):
            self.state.append(torch.full((1, C, H, W), float("inf"), device="cuda"))
            if self.x3:
                S = torch.empty(C_.cbinfer_split3_state_bytes(*a), dtype=torch.uint8, device="cuda")
                lib.check(C_.cbinfer_split3_state_init(S.data_ptr(), *a, None))
                lib.check(C_.cbinfer_split3_state_rebuild(self.state[q].data_ptr(), S.data_ptr(), *a, None))
            else:
                S = torch.empty(C_.cbinfer_split_state_bytes(*a), dtype=torch.uint8, device="cuda")
                lib.check(C_.cbinfer_split_state_init(S.data_ptr(), *a, None))
                lib.check(C_.cbinfer_split_state_rebuild(self.state[q].data_ptr(), S.data_ptr(), *a, self.flag.data_ptr(),
                                                         None))
            self.S.append(S)
            self.masks.append(torch.zeros(C_.cbinfer_frame_mask_bytes(H, W) // 8, dtype=torch.int64, device="cuda"))
            self.out.append(torch.full((1, K, H, W), float("inf"), device="cuda"))
            self.idx.append(torch.zeros(H * W, dtype=torch.int32, device="cuda"))
            self.cnt.append(torch.full((1,), -1, dtype=torch.int32, device="cuda"))
            self.copy.append(torch.full((words,), -1, dtype=torch.int64, device="cuda"))
            s = self.seqs[q]
            s.state, s.splitState, s.frameMasks = self.state[q].data_ptr(), S.data_ptr(), self.masks[q].data_ptr()
            s.output, s.idxOut, s.countOut = self.out[q].data_ptr(), self.idx[q].data_ptr(), self.cnt[q].data_ptr()
            s.rangeFlag, s.maskCopy = self.flag.data_ptr(), self.copy[q].data_ptr()

    def detect(self, inputs, th):
        for q, x in enumerate(inputs):
            self.seqs[q].input, self.seqs[q].producerMask = x.data_ptr(), None
        pH, pW = (inputs[0].shape[-2], inputs[0].shape[-1]) if self.pooled else (0, 0)
        self.lib.check(self.lib.C.cbinfer_split_detect(self.seqs, self.nSeq, int(self.pooled) | (8 if self.x3 else 0), pH, pW,
                                                       self.C, self.H, self.W, self.kH, self.kW, th, None))

    def conv(self, relu=True):
        self.lib.check(self.lib.C.cbinfer_split_conv(self.seqs, self.nSeq, self.wp.data_ptr(), self.b.data_ptr(), self.C,
                                                     self.H, self.W, self.K, self.kH, self.kW, self.scale, int(relu),
                                                     self.ws.data_ptr() if self.ws is not None else None, 0, None))

    def frame(self, inputs, th, relu=True):
        self.detect(inputs, th)
        self.conv(relu)
        torch.cuda.synchronize()

    def list(self, q=0):
        n = int(self.cnt[q].item())
        assert 0 <= n <= self.H * self.W, n
        return self.idx[q][:n].cpu().numpy()

    def mask_bits(self, q=0):
        words = self.copy[q].cpu().numpy().view(np.uint64)
        wpr = (self.W + 63) // 64
        return np.unpackbits(words.view(np.uint8), bitorder="little").reshape(self.H, wpr * 64)


def walk(rng, C, H, W):
    """A priming frame (every pixel is new to the state), then the three frames of the scan's corner cases: nothing changed;
    one 3x3 block in the map's last rows whose dilated image straddles the boundary of the mask words 0 and 1; every pixel
    changed."""
    x0 = rng.standard_normal((1, C, H, W)).astype(np.float32)
    x2 = x0.copy()
    x2[0, :, H - 3:H, 63:66] += 1.0
    x3 = rng.standard_normal((1, C, H, W)).astype(np.float32)      # (a new frame: some channel of every pixel differs)
    return [x0, x0.copy(), x2, x3]


def check_against_oracle(L, o, q, t, W):
    lst, n = L.list(q), int(L.cnt[q].item())
    assert n == o.lastList.size and np.array_equal(lst, o.lastList), (t, q)
    assert np.array_equal(L.state[q].cpu().numpy(), o.prevInput), (t, q)
    bits = L.mask_bits(q)
    assert np.array_equal(bits[:, :W].astype(np.int8), o.changeMap), (t, q)
    assert not bits[:, W:].any(), (t, q)
    err = np.abs(L.out[q].cpu().numpy() - o.prevOutput).max()
    assert err <= FP32_TOL, (t, q, err)


class Twin(object):
    """The oracle's feedback-mode layer, keeping the last frame's change list."""

    def __init__(self, oracle, w, b, th):
        self.o = oracle.OracleCBConv2d(w, b, th, withReLU=True, feedbackLoop=True, propChangeIndexes=True)

    def forward(self, x):
        self.o.lastList = np.asarray(self.o.forward(x)[2])
        return self.o


# 64x64 tile: a 16 -> 64 layer at 70x260 -- 350 mask words (175 row-pair units) on 256 threads; 128x128 tile: a 64 -> 128
# layer at 130x300 -- 650 words on 512 threads: two chunks per thread, the last threads' chunks partial or empty
CASES = [(16, 64, 7, 70, 260), (64, 128, 3, 130, 300)]


@pytest.fixture(scope="module")
def references(oracle):
    """Per case: weights, the walk and the oracle's results after every frame -- computed once, shared by the tests below
    (state, change map, list, outputs: copies, never written to)."""
    out = {}
    for C, K, k, H, W in CASES:
        rng = np.random.default_rng(C * 1000 + K + H)
        w = (rng.standard_normal((K, C, k, k)) / np.sqrt(C * k * k)).astype(np.float32)
        b = rng.standard_normal(K).astype(np.float32)
        frames = walk(rng, C, H, W)
        tw, snaps = Twin(oracle, w, b, 0.1), []
        for x in frames:
            o = tw.forward(x)
            snap = type("Snap", (), {})()
            snap.lastList, snap.prevInput, snap.changeMap = o.lastList.copy(), o.prevInput.copy(), np.array(o.changeMap)
            snap.prevOutput = o.prevOutput.copy()
            snaps.append(snap)
        assert snaps[1].lastList.size == 0 and snaps[3].lastList.size == H * W
        # (the block's dilated image: rows H - 3 - r .. H - 1, columns 63 - r .. 65 + r -- both sides of a word boundary)
        r = (k - 1) // 2
        assert snaps[2].lastList.size == (3 + r) * (3 + 2 * r) and snaps[2].changeMap[H - 1, 63] and snaps[2].changeMap[H - 1, 64]
        out[(C, K, k, H, W)] = (w, b, frames, snaps)
    return out


@pytest.mark.parametrize("arith", ["x3", "f16x2"])
@pytest.mark.parametrize("case", CASES)
def test_scan_of_a_mask_larger_than_the_workgroup_pixel_order(lib, references, case, arith):
    C, K, k, H, W = case
    w, b, frames, snaps = references[case]
    L = Layer(lib, w, b, H, W, arith)
    for t, (x, o) in enumerate(zip(frames, snaps)):
        L.frame([dev(x)], 0.1)
        check_against_oracle(L, o, 0, t, W)
    assert int(L.flag.item()) == 0


def test_scan_of_a_mask_larger_than_the_workgroup_window_order(lib, references):
    """The 16 -> 64 layer at 70x260 in pooling-window order (cbinfer_split_conv_next) with a 7x7 consumer behind the
    floor-mode 2x2 pool: the producer against the oracle as above, the consumer's state, split copy and frame mask against
    its own pooled detection launch fed the same outputs."""
    case = CASES[0]
    C, K, k, H, W = case
    w, b, frames, snaps = references[case]
    C_ = lib.C
    H2, W2, k2, K2 = H // 2, W // 2, 7, 32
    rng = np.random.default_rng(3)
    w2 = (rng.standard_normal((K2, K, k2, k2)) / np.sqrt(K * k2 * k2)).astype(np.float32)
    b2 = rng.standard_normal(K2).astype(np.float32)
    P = Layer(lib, w, b, H, W, "x3")
    Ca, Cb = Layer(lib, w2, b2, H2, W2, "x3", pooled=True), Layer(lib, w2, b2, H2, W2, "x3", pooled=True)
    nd = lib.NextDetect()
    nd.state, nd.splitState, nd.frameMasks = Cb.state[0].data_ptr(), Cb.S[0].data_ptr(), Cb.masks[0].data_ptr()
    nd.rangeFlag, nd.H, nd.W, nd.kH, nd.kW, nd.threshold, nd.arith = Cb.flag.data_ptr(), H2, W2, k2, k2, 0.05, 1
    assert C_.cbinfer_split_next_supported(C, K, k, k, H, W, ctypes.pointer(nd)) == 1
    for t, (x, o) in enumerate(zip(frames, snaps)):
        P.detect([dev(x)], 0.1)
        lib.check(C_.cbinfer_split_conv_next(P.seqs, 1, P.wp.data_ptr(), P.b.data_ptr(), C, H, W, K, k, k, 0.0, 1, None,
                                             ctypes.pointer(nd), None))
        Ca.detect([P.out[0]], 0.05)
        torch.cuda.synchronize()
        check_against_oracle(P, o, 0, t, W)
        assert torch.equal(Ca.state[0], Cb.state[0]) and torch.equal(Ca.S[0], Cb.S[0]), t
        assert torch.equal(Ca.masks[0], Cb.masks[0]), t
        Ca.masks[0].zero_(), Cb.masks[0].zero_()      # (the consumer's contraction would)


def test_scan_of_two_sequences_in_one_launch(lib, references):
    """Two sequences of the 16 -> 64 case in one launch (700 mask words, the sequence boundary inside a thread's chunk
    range), the second one a frame ahead of the first: each against the oracle's results of its own frame."""
    case = CASES[0]
    C, K, k, H, W = case
    w, b, frames, snaps = references[case]
    L = Layer(lib, w, b, H, W, "x3", nSeq=2)
    order = [(0, 0), (1, 1), (2, 1), (3, 2), (3, 3)]      # (frame of sequence 0, of sequence 1); a repeated frame: no change
    prev = [None, None]
    for t, fr in enumerate(order):
        L.frame([dev(frames[f]) for f in fr], 0.1)
        for q, f in enumerate(fr):
            if f == prev[q]:
                assert int(L.cnt[q].item()) == 0 and not L.mask_bits(q).any(), (t, q)
                assert np.array_equal(L.state[q].cpu().numpy(), snaps[f].prevInput), (t, q)
            else:
                check_against_oracle(L, snaps[f], q, t, W)
            prev[q] = f


def test_two_sequences_through_sequence_batch():
    """Module level: the bench network at 140x520 -- its 16 -> 64 layer is the 70x260 case -- for two sequences through
    pycbinfer.SequenceBatch against each sequence alone through its own copy of the network, bit for bit, outputs and
    every layer state; the three corner frames in a different order per sequence."""
    import bench
    import pycbinfer as pkg
    nets = [bench.build_bench_model()[1] for _ in range(2)]
    batch = pkg.SequenceBatch(bench.build_bench_model()[1], 2)
    rng = np.random.default_rng(21)
    H, W = 140, 520
    x0 = rng.random((1, 3, H, W)).astype(np.float32)
    x2 = x0.copy()
    x2[0, :, H - 3:H, 127:130] += 0.5
    x3 = (x2 + 0.3 + 0.5 * rng.random((1, 3, H, W))).astype(np.float32)
    f = [dev(v) for v in (x0, x2, x3)]
    walks = [[f[0], f[0], f[1], f[2], f[2]], [f[2], f[0], f[0], f[1], f[2]]]

    def states(net):
        out = []
        for m in net.children():
            if type(m) is pkg.CBConv2d:
                out.append((m.prevInput, m.prevOutput))
            elif type(m) is pkg.CBTail1x1:
                out.append((None, m.prevOutput))
        return out

    with torch.no_grad():
        for t in range(5):
            outs = batch([walks[q][t] for q in range(2)])
            for q in range(2):
                y = nets[q](walks[q][t])
                assert torch.equal(outs[q], y), (t, q)
                for (pi, po), (bi, bo) in zip(states(nets[q]), batch.states(q)):
                    assert torch.equal(po, bo), (t, q)
                    if pi is not None:
                        assert torch.equal(pi, bi), (t, q)
    assert not batch.rangeExceeded()


@pytest.mark.parametrize("mode", ["every pixel", "one pixel in the last row"])
@pytest.mark.parametrize("H,W", [(33, 130), (64, 320)])
def test_self_detecting_rowpairs_with_every_unit_resident(lib, H, W, mode):
    """cbinfer_conv_rowpairs_detect + cbinfer_refresh_state against cbinfer_cbconv2d_forward_rowpairs (detection launch + row
    pairs), as tests/test_gpu_rowpair.py::test_rowpairs_with_their_own_detection compares them: outputs, refreshed state, the
    frame's dilated mask and the next layer's state, split copy and frame mask, bit for bit.  33x130: an odd last row, a
    partial last mask word, 51 units -- fewer than CUs; 64x320: 160 units.  Threshold -1: every unit works in every
    frame; threshold 0.05 with ONE changed pixel in the map's last row: the units around it work, all others leave at once."""
    C_ = lib.C
    rng = np.random.default_rng(H * 3 + W)
    C, K, k, k2 = 3, 16, 7, 7
    H2, W2 = H // 2, W // 2
    th = -1.0 if mode == "every pixel" else 0.05
    w = (rng.standard_normal((K, C, k, k)) / np.sqrt(C * k * k)).astype(np.float32)
    b = rng.standard_normal(K).astype(np.float32)
    wp = torch.empty(C_.cbinfer_rowconv_prepared_bytes(C, K, k, k), dtype=torch.uint8, device="cuda")
    lib.check(C_.cbinfer_rowconv_prep_weights(dev(w).data_ptr(), wp.data_ptr(), K, C, k, k, None))
    bd = dev(b)
    words = C_.cbinfer_mask_words(H, W)

    class Side(object):
        def __init__(self):
            self.state = torch.zeros((1, C, H, W), device="cuda")
            self.out = torch.zeros((1, K, H, W), device="cuda")
            self.bits = torch.zeros(words, dtype=torch.int64, device="cuda")
            self.ctl = torch.zeros(words, dtype=torch.int32, device="cuda")
            self.copy = torch.zeros(words, dtype=torch.int64, device="cuda")
            self.state2 = torch.zeros((1, K, H2, W2), device="cuda")
            self.S2 = torch.empty(C_.cbinfer_split3_state_bytes(K, H2, W2, k2, k2), dtype=torch.uint8, device="cuda")
            lib.check(C_.cbinfer_split3_state_init(self.S2.data_ptr(), K, H2, W2, k2, k2, None))
            lib.check(C_.cbinfer_split3_state_rebuild(self.state2.data_ptr(), self.S2.data_ptr(), K, H2, W2, k2, k2, None))
            self.mask2 = torch.zeros(C_.cbinfer_frame_mask_bytes(H2, W2) // 8, dtype=torch.int64, device="cuda")
            self.nd = nd = lib.NextDetect()
            nd.state, nd.splitState, nd.frameMasks = self.state2.data_ptr(), self.S2.data_ptr(), self.mask2.data_ptr()
            nd.rangeFlag, nd.H, nd.W, nd.kH, nd.kW, nd.threshold, nd.arith = None, H2, W2, k2, k2, 0.07, 1

    a, d = Side(), Side()
    x = rng.standard_normal((1, C, H, W)).astype(np.float32)
    counts = []
    for t in range(3):
        x = x.copy()
        if t > 0:
            if mode == "every pixel":
                x += rng.uniform(-0.5, 0.5, x.shape).astype(np.float32)
            else:
                x[0, t % C, H - 1, (W - 2) if t == 1 else 64] += 1.0
        xd = dev(x)
        lib.check(C_.cbinfer_cbconv2d_forward_rowpairs(xd.data_ptr(), a.state.data_ptr(), a.out.data_ptr(),
                                                       a.bits.data_ptr(), a.ctl.data_ptr(), a.copy.data_ptr(),
                                                       wp.data_ptr(), bd.data_ptr(), C, H, W, K, k, k, th, 1,
                                                       ctypes.pointer(a.nd), None))
        lib.check(C_.cbinfer_conv_rowpairs_detect(xd.data_ptr(), d.state.data_ptr(), d.out.data_ptr(), d.copy.data_ptr(),
                                                  wp.data_ptr(), bd.data_ptr(), C, H, W, K, k, k, th, 1,
                                                  ctypes.pointer(d.nd), None))
        lib.check(C_.cbinfer_refresh_state(xd.data_ptr(), d.state.data_ptr(), C, H, W, th, None))
        torch.cuda.synchronize()
        assert torch.equal(a.copy, d.copy), t
        assert torch.equal(a.out, d.out), t
        assert torch.equal(a.state, d.state), t
        assert torch.equal(a.state2, d.state2) and torch.equal(a.S2, d.S2) and torch.equal(a.mask2, d.mask2), t
        bits = np.unpackbits(d.copy.cpu().numpy().view(np.uint8), bitorder="little")
        counts.append(int(bits.sum()))
        a.mask2.zero_(), d.mask2.zero_()
    if mode == "every pixel":
        assert counts == [H * W] * 3, counts
    else:      # the pixel's dilated image, clipped by the map's last row and (frame 1) by its right edge
        assert counts == [H * W, 4 * 5, 4 * 7], counts
