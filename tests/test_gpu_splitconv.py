"""-m gpu: every case of tests/splitconv_cases.py through the C ABI of the split-state kernels (cb_split.hip), pinned
against float64 math: oracle.genXMatrix patches of the oracle's refreshed state times the weights in double, plus the
bias, at every listed pixel and every output channel.  Per frame (0: every pixel, 1: the case's change set + noise below
the threshold, 2: the same input again) the change list, the f32 state and the mask copy equal the oracle's bit for bit,
the listed outputs are within 1e-4 and within 64 * 2^-24 * (sum|a||b| + |bias|) per element, everything else keeps its
bits, and the case ran in the cell it claims on this card (the workspace header of a deep contraction says so too).
Every case runs with bias alone and with ReLU alone.  Deep cases also run with the k-split forced off and on, each pinned
the same way and bit-identical to each other.

Observed worst |err| / (sum|a||b| + |bias|, fine-grained: + |prev|) on an MI355X, 2026-10-19 (printed by
test_zz_report_worst_ratios; the bar is 64 * 2^-24 = 2^-18):
    x3:    shallow 2^-21.8, deep_split 2^-23.1, deep_whole 2^-24.0, deep_split_tail 2^-23.2, deep_whole_tail 2^-23.6,
           forced unsplit / split 2^-23.1, fg_shallow 2^-21.9, fg_deep 2^-22.4
    f16x2: shallow 2^-21.9, deep_split 2^-22.7, deep_whole 2^-23.3, deep_split_tail 2^-23.3, deep_whole_tail 2^-23.0,
           forced unsplit / split 2^-22.8, fg_shallow 2^-21.1, fg_deep 2^-21.3
The sparse tests (test_sparse_operands_fine_grained) have teeth at that bar: a build without the b0 w2 product of the
bf16-triple step failed all six x3 cases the table then held (the 128-row LDS form and the two small 64-row forms,
shallow and deep), a build without the hi lo product of the f16-pair step all eight f16x2 cases (every instance but
the three-stage ring).
"""
import ctypes
import zlib

import numpy as np
import pytest
import torch

import splitconv_cases as sc
from splitconv_cases import CASES, CASE_BY_ID, case_form, cell_of
from test_gpu_split import Layer
from optest import dev, gpu_lib as lib      # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

FP32_TOL = 1e-4
BOUND = 64 * 2.0 ** -24
FILL = 7.25
TH = 0.1
WORST = {}
RAN = set()       # ids of the cases whose test ran to its end

CONV_IDS = [c.id for c in CASES if c.mode == "conv"]
TAIL_IDS = [c.id for c in CASES if c.mode == "tail"]
FG_IDS = [c.id for c in CASES if c.mode == "fg"]
assert len(CONV_IDS) + len(TAIL_IDS) + len(FG_IDS) == len(CASES)


def cus():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def assert_claimed_cell(c):
    f = case_form(c, cus())
    assert cell_of(f) == c.cell, ("%s: on a card with %d CUs this shape lands in %s, not in the cell %s it was written "
                                  "for (%s)" % (c.id, cus(), cell_of(f), c.cell, f))
    return f


class NoBias(object):
    @staticmethod
    def data_ptr():
        return None


def make_weights(rng, c):
    K, C, kH, kW = c.K, c.C, c.kH, c.kW
    w = (rng.standard_normal((K, C, kH, kW)) / np.sqrt(C * kH * kW) *
         np.exp(rng.uniform(-4, 2, (K, 1, 1, 1)))).astype(np.float32)
    return w, rng.standard_normal(K).astype(np.float32)


def make_frames(rng, c):
    """[frame][sequence] inputs: channels scaled by exp(U(-6, 3)); frame 1 = frame 0 with new values at the changed
    pixels (one channel moved by more than the threshold for sure) + noise below the threshold everywhere."""
    C, H, W = c.C, c.H, c.W
    own = sc.changed_pixels(c)
    frames = [[], [], []]
    for kind in sc.seq_kinds(c):
        scale = np.exp(rng.uniform(-6, 3, (1, C, 1, 1)))
        x0 = (rng.standard_normal((1, C, H, W)) * scale).astype(np.float32)
        x0[0, 0, :4] *= 1e-6                         # values deep in the f16 subnormal range of hi AND lo
        m = {"own": own, "static": np.zeros((H, W), bool), "full": np.ones((H, W), bool)}[kind]
        fresh = (rng.standard_normal((1, C, H, W)) * scale).astype(np.float32)
        fresh[0, 0] = x0[0, 0] + np.where(rng.random((H, W)) < 0.5, -1.0, 1.0) * (0.5 + np.abs(rng.standard_normal((H, W))))
        x1 = np.where(m[None, None], fresh, x0 + rng.uniform(-0.03, 0.03, x0.shape)).astype(np.float32)
        frames[0].append(x0), frames[1].append(x1), frames[2].append(x1.copy())
    return frames


def reference(oracle, state, idx, w, chunk=8192):
    """(sum a b, sum |a||b|) in float64 at the listed pixels: [N, K] each."""
    K = w.shape[0]
    wm = w.reshape(K, -1).astype(np.float64)
    y, mag = np.empty((len(idx), K)), np.empty((len(idx), K))
    for i in range(0, len(idx), chunk):
        X = oracle.genXMatrix(state, idx[i:i + chunk], w.shape[2:]).astype(np.float64)
        y[i:i + chunk] = X @ wm.T
        mag[i:i + chunk] = np.abs(X) @ np.abs(wm).T
    return y, mag


def mask_bits(copy, H, W):
    words = copy.cpu().numpy().view(np.uint64)
    wpr = (W + 63) // 64
    return np.unpackbits(words.view(np.uint8), bitorder="little").reshape(H, wpr * 64)[:, :W].astype(np.int8)


def note_worst(c, regime, ratio):
    key = (c.arith, regime)
    WORST[key] = max(WORST.get(key, 0.0), float(ratio))


def check_outputs(c, what, regime, out_t, before, idx, y, mag, b, relu):
    """out_t: the [1,K,H,W] output after the launch, before: its bits in front of it (numpy [K, HW])."""
    K, HW = c.K, c.H * c.W
    now = out_t.cpu().numpy().reshape(K, HW)
    want = y + (b.astype(np.float64)[None, :] if b is not None else 0.0)
    if relu:
        want = np.maximum(want, 0.0)
    bound = mag + (np.abs(b).astype(np.float64)[None, :] if b is not None else 0.0)
    err = np.abs(now[:, idx].T.astype(np.float64) - want)
    ratio = float((err / (bound + 1e-300)).max()) if len(idx) else 0.0
    print("%s: %d listed, max |err| %.3g, worst err / (sum|a||b| + |bias|) %.3g (2^%.1f)" % (
        what, len(idx), err.max() if len(idx) else 0.0, ratio, np.log2(ratio + 1e-300)))
    note_worst(c, regime, ratio)
    assert np.all(np.isfinite(now[:, idx])), what
    assert np.all(err <= FP32_TOL), (what, float(err.max()))
    assert np.all(err <= BOUND * bound + 1e-300), (what, ratio)
    rest = np.ones(HW, bool)
    rest[idx] = False
    assert np.array_equal(now[:, rest].view(np.int32), before[:, rest].view(np.int32)), what + ": a pixel off the list changed"
    return now


def check_header(c, L, f, counts, what):
    if not f["deep"]:
        assert L.ws is None
        return
    info = L.ws[:256].view(torch.int32).cpu().numpy()
    tiles = [(n + f["BN"] - 1) // f["BN"] for n in counts]
    assert info[0] == f["SK"] and info[1] == f["MT"], (what, info[:4], f)
    assert info[4:4 + c.nSeq].tolist() == tiles and info[12:12 + c.nSeq].tolist() == list(counts), (what, info[:20])


def tail_setup(lib, rng, K):
    C_ = lib.C
    C1, C2 = sc.TAIL_C1, sc.TAIL_C2
    w1 = (rng.standard_normal((C1, K)) / np.sqrt(K)).astype(np.float32)
    b1 = rng.standard_normal(C1).astype(np.float32)
    w2 = (rng.standard_normal((C2, C1)) / np.sqrt(C1)).astype(np.float32)
    b2 = rng.standard_normal(C2).astype(np.float32)
    t = dict(w1=dev(w1), b1=dev(b1), w2=dev(w2), b2=dev(b2), C1=C1, C2=C2)
    t["w1p"] = torch.empty(C_.cbinfer_tail1x1_prepared_bytes(C1, K) // 4, device="cuda")
    lib.check(C_.cbinfer_tail1x1_prep(t["w1"].data_ptr(), t["w1p"].data_ptr(), C1, K, None))
    return t


def run_frames(lib, oracle, c, frames, w, b, bias, relu, force, refs, tail=None):
    """The three frames of one configuration; refs: per frame and sequence (idx, state, changeMap, y, mag), computed by
    the first configuration of the case and shared by the others.  Returns the outputs' final bits."""
    C_ = lib.C
    L = Layer(lib, w, b, c.H, c.W, nSeq=c.nSeq, arith=c.arith)
    if not bias:
        L.b = NoBias()
    for q in range(c.nSeq):
        L.out[q].fill_(FILL)
    regime = c.cell[2] if force == 0 else "forced %d" % force
    st, tout = None, None
    if tail is not None:
        assert C_.cbinfer_split_tail_supported(c.C, c.K, c.kH, c.kW, tail["C1"], tail["C2"]) == 1
        tout = [torch.full((1, tail["C2"], c.H, c.W), FILL, device="cuda") for _ in range(c.nSeq)]
        st = lib.SplitTail()
        st.w1Prepared, st.b1, st.w2, st.b2 = (tail["w1p"].data_ptr(), tail["b1"].data_ptr(), tail["w2"].data_ptr(),
                                              tail["b2"].data_ptr())
        st.C1, st.C2, st.relu1, st.relu2 = tail["C1"], tail["C2"], 1, 0
        for q in range(c.nSeq):
            st.output[q] = tout[q].data_ptr()
    for t in range(3):
        what = "%s frame %d bias %d relu %d force %d" % (c.id, t, bias, relu, force)
        before = [L.out[q].cpu().numpy().reshape(c.K, -1).copy() for q in range(c.nSeq)]
        xs = [dev(x) for x in frames[t]]
        if tail is None:
            L.frame(xs, TH, relu=relu, force=force)
        else:
            for q, x in enumerate(xs):
                L.seqs[q].input, L.seqs[q].producerMask = x.data_ptr(), None
            lib.check(C_.cbinfer_split_forward_tail(L.seqs, c.nSeq, 0, 0, 0, L.wp.data_ptr(), L.b.data_ptr(), c.C, c.H,
                                                    c.W, c.K, c.kH, c.kW, TH, L.scale, int(relu), L.ws.data_ptr(), force,
                                                    ctypes.pointer(st), None))
            torch.cuda.synchronize()
        counts = []
        for q in range(c.nSeq):
            idx, state, cmap, y, mag = refs[t][q]
            counts.append(len(idx))
            assert np.array_equal(L.list(q), idx), (what, q)
            assert np.array_equal(L.state[q].cpu().numpy(), state), (what, q)
            assert np.array_equal(mask_bits(L.copy[q], c.H, c.W), cmap), (what, q)
            check_outputs(c, "%s seq %d" % (what, q), regime if t == 1 else "frame %d" % t, L.out[q], before[q], idx, y,
                          mag, b if bias else None, relu)
            if t == 2:
                assert len(idx) == 0
        if t == 1:
            want = sc.seq_counts(c)
            assert counts == want, (what, counts, want)
        f = sc.split_form(c.arith, c.C, c.K, c.kH, c.kW, c.H, c.W, c.nSeq, counts, cus(), force, tail=tail is not None)
        if t == 1 and force == 0:
            assert cell_of(f) == c.cell, (what, cell_of(f))
        if sum(counts):
            check_header(c, L, f, counts, what)
    assert int(L.flag.item()) == 0
    if tail is not None:
        for q in range(c.nSeq):
            y = L.out[q].double()
            dense = torch.nn.functional.conv2d(torch.relu(torch.nn.functional.conv2d(
                y, tail["w1"].double().view(tail["C1"], c.K, 1, 1), tail["b1"].double())),
                tail["w2"].double().view(tail["C2"], tail["C1"], 1, 1), tail["b2"].double())
            te = float((dense - tout[q].double()).abs().max())
            print("%s seq %d: tail max |err| %.3g" % (c.id, q, te))
            assert te <= FP32_TOL, (c.id, q, te)
    return [o.clone() for o in L.out]


def make_refs(oracle, c, frames, w, b):
    os_ = [oracle.OracleCBConv2d(w, b, TH, feedbackLoop=True, propChangeIndexes=True) for _ in range(c.nSeq)]
    refs = []
    for t in range(3):
        row = []
        for q in range(c.nSeq):
            idx = os_[q].forward(frames[t][q])[2].copy()
            state = os_[q].prevInput.copy()
            y, mag = reference(oracle, state, idx, w)
            row.append((idx, state, os_[q].changeMap.copy(), y, mag))
        refs.append(row)
    return refs


def run_case(lib, oracle, cid):
    c = CASE_BY_ID[cid]
    f = assert_claimed_cell(c)
    rng = np.random.default_rng(zlib.crc32(cid.encode()))
    w, b = make_weights(rng, c)
    frames = make_frames(rng, c)
    refs = make_refs(oracle, c, frames, w, b)
    tail = tail_setup(lib, rng, c.K) if c.mode == "tail" else None
    # with and without bias, with and without ReLU: bias alone (no output clamped: every one tells of the arithmetic),
    # ReLU alone
    a = run_frames(lib, oracle, c, frames, w, b, True, False, 0, refs, tail)
    run_frames(lib, oracle, c, frames, w, b, False, True, 0, refs, tail)
    if f["deep"]:
        # the other deep forms, each against float64 -- and bit-identical to the kernel's own choice
        for force in (1, 4):
            o = run_frames(lib, oracle, c, frames, w, b, True, False, force, refs, tail)
            for q in range(c.nSeq):
                assert torch.equal(o[q], a[q]), (cid, force, q)
    RAN.add(cid)


@pytest.mark.parametrize("cid", CONV_IDS)
def test_case_frames_against_float64(lib, oracle, cid):
    run_case(lib, oracle, cid)


@pytest.mark.parametrize("cid", TAIL_IDS)
def test_tail_launch_against_float64(lib, oracle, cid):
    """cbinfer_split_forward_tail: the layer output pinned as every other case, the tail against float64
    conv1x1 -> ReLU -> conv1x1 of that output at 1e-4."""
    run_case(lib, oracle, cid)


@pytest.mark.parametrize("cid", FG_IDS)
def test_sparse_operands_fine_grained(lib, oracle, cid):
    """cbinfer_split_forward_fg on a delta with about 1.5 non-zero values per patch: in a deep dense sum a dropped
    cross term of the bf16 triples or f16 pairs hides behind sum|a||b| of hundreds of products; here the sum is one or
    two products.  The accumulated output against float64 prev + W delta within 64 * 2^-24 * (sum|a||b| + |prev|) -- prev
    spans exp(U(-12, 0)), so that it does not hide the products either --, every pixel off the mask bit-unchanged,
    reluOut = relu(output), the delta tensor, the state, the list and the mask copy exact, the range flag down."""
    c = CASE_BY_ID[cid]
    assert_claimed_cell(c)
    C_ = lib.C
    rng = np.random.default_rng(zlib.crc32(cid.encode()))
    w, b = make_weights(rng, c)
    K, C, H, W = c.K, c.C, c.H, c.W
    L = Layer(lib, w, b, H, W, nSeq=c.nSeq, arith=c.arith)
    sup = sc.fg_support(c)
    x0s, x1s, prevs, deltas, relus = [], [], [], [], []
    for q, kind in enumerate(sc.seq_kinds(c)):
        scale = np.exp(rng.uniform(-6, 3, (1, C, 1, 1)))
        x0 = (rng.standard_normal((1, C, H, W)) * scale).astype(np.float32)
        s = {"own": sup, "static": np.zeros_like(sup), "full": np.ones_like(sup)}[kind][None]
        d = np.where(rng.random(x0.shape) < 0.5, -1.0, 1.0) * (2 * TH + np.abs(rng.standard_normal(x0.shape)) * scale)
        x1 = np.where(s, x0 + d, x0).astype(np.float32)
        prev = (rng.standard_normal((1, K, H, W)) * np.exp(rng.uniform(-12, 0, (1, K, H, W)))).astype(np.float32)
        x0s.append(x0), x1s.append(x1), prevs.append(prev)
        L.state[q].copy_(dev(x0))
        L.out[q].copy_(dev(prev))
        deltas.append(torch.full((1, C, H, W), FILL, device="cuda"))
        relus.append(torch.relu(L.out[q]).clone())
        L.seqs[q].delta, L.seqs[q].reluOut = deltas[q].data_ptr(), relus[q].data_ptr()
    xs = [dev(x) for x in x1s]
    for q in range(c.nSeq):
        L.seqs[q].input, L.seqs[q].producerMask = xs[q].data_ptr(), None
    lib.check(C_.cbinfer_split_forward_fg(L.seqs, c.nSeq, 0, 0, 0, L.wp.data_ptr(), C, H, W, K, c.kH, c.kW, TH, L.scale,
                                          L.ws.data_ptr() if L.ws is not None else None, None))
    torch.cuda.synchronize()
    counts = []
    for q in range(c.nSeq):
        diff = x1s[q] - x0s[q]                       # (f32, as the detection forms it)
        dl = np.where(np.abs(diff) > np.float32(TH), diff, np.float32(0)).astype(np.float32)
        assert np.array_equal(deltas[q].cpu().numpy(), dl), (cid, q)
        assert np.array_equal(L.state[q].cpu().numpy(), x1s[q]), (cid, q)
        mask = sc.dilate((dl[0] != 0).any(axis=0), c.kH, c.kW)
        idx = np.flatnonzero(mask.reshape(-1)).astype(np.int32)
        counts.append(len(idx))
        assert np.array_equal(L.list(q), idx), (cid, q)
        assert np.array_equal(mask_bits(L.copy[q], H, W), mask.astype(np.int8)), (cid, q)
        y, mag = reference(oracle, dl, idx, w)
        pv = prevs[q].reshape(K, -1)
        now = L.out[q].cpu().numpy().reshape(K, -1)
        want = pv[:, idx].T.astype(np.float64) + y
        bound = mag + np.abs(pv[:, idx].T).astype(np.float64)
        err = np.abs(now[:, idx].T.astype(np.float64) - want)
        ratio = float((err / (bound + 1e-300)).max()) if len(idx) else 0.0
        if len(idx) and sc.seq_kinds(c)[q] == "own":
            X = oracle.genXMatrix(dl, idx, (c.kH, c.kW))
            per = (X != 0).sum(axis=1)
            print("%s seq %d: %.2f non-zero values per patch (max %d)" % (cid, q, per.mean(), per.max()))
        print("%s seq %d: %d listed, worst err / (sum|a||b| + |prev|) %.3g (2^%.1f)" % (
            cid, q, len(idx), ratio, np.log2(ratio + 1e-300)))
        note_worst(c, c.cell[2], ratio)
        assert np.all(err <= BOUND * bound + 1e-300), (cid, q, ratio)
        rest = np.ones(H * W, bool)
        rest[idx] = False
        assert np.array_equal(now[:, rest].view(np.int32), pv[:, rest].view(np.int32)), (cid, q)
        assert torch.equal(relus[q], torch.relu(L.out[q])), (cid, q)
    # (a tripped range flag would send an f16-pair sequence down the exact f32 path: nothing of the pair step would run)
    assert int(L.flag.item()) == 0
    assert counts == sc.seq_counts(c), (counts, sc.seq_counts(c))
    f = sc.split_form(c.arith, C, K, c.kH, c.kW, H, W, c.nSeq, counts, cus(), accumulate=True)
    assert cell_of(f) == c.cell
    if sum(counts):
        check_header(c, L, f, counts, cid)
    RAN.add(cid)


def test_zz_report_worst_ratios(capsys):
    """Not a check of the kernels: prints the worst ratio per arithmetic and regime seen by the tests above, and fails
    if a case of the table did not run."""
    with capsys.disabled():
        print("\nworst |err| / bound sum per arithmetic and regime:")
        for (arith, regime), r in sorted(WORST.items()):
            print("  %-6s %-16s %.3g (2^%.1f)" % (arith, regime, r, np.log2(r + 1e-300)))
    missing = [c.id for c in CASES if c.id not in RAN]
    assert not missing, "cases of the table that did not run to their end: %s" % missing
