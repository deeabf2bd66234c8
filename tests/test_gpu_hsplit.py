"""-m gpu: every case of tests/hsplit_cases.py through the C ABI of the fp16 layers on the split-state machinery
(cb_split.hip: cbinfer_hsplit_forward_group -- cbh_detect_kernel, the four HALF instantiations of cbs_conv_kernel,
cbh_reduce_kernel), pinned against float64 math: oracle.genXMatrix patches of the oracle's refreshed f16 state times the
weights in double, plus the bias, at every listed pixel and every output channel.

Per frame (0: every pixel, 1: the case's change set + noise below the threshold, 2: the same input again) and layer the
change list, its length, the mask copy, prevInput and its pixel-major copy equal the oracle's half state machine bit for
bit (changeDetection_half on a 1x1 support, changePropagation; with the feedback loop the changed pixels are refreshed,
without it the whole frame), every listed output meets the per-element bar

    |got - want| <= 2^-11 |want| + 2^-25 + A (sum|a||b| + |bias|)

and the layer's 2-ulp bar of its largest output, every other output keeps its bits, the frame masks (mask and arrival
counters) are zero again, and the case ran in the cell it claims on this card -- by hsplit_cases.hsplit_form at the
card's CU count and, for a deep contraction, by the launch info in the workspace: SK, the row tiles, the tiles and list
lengths per layer, the chunk counts per layer.  Every case runs with and without the feedback loop, each with bias
alone, with ReLU alone and with neither.  Frame 0 of the cases marked sample0 (the shallow 128-row instances take maps
of 16257 pixels and more under a wide K or taller ones under a narrow K; more than 1536 mask words under 66 stages) is
compared with float64 at a sample of the pixels that the reference budget pays for, its whole output is finite, and a
second, independent sample meets the 2-ulp bar; everything else of that frame, and every later frame, in full.  The
single-layer entry cbinfer_hsplit_forward must leave the bits of the group call of one layer.

Group rows: every layer of a two-layer launch is pinned on its own and equals the same layer launched alone bit for bit.
Consumer rows: after the producing launch a copy-mode consumer's state equals the producer's output, its pixel-major
copy follows, its frame mask is the dilation of the oracle's half predicate on (old state, new output) with its own
filter and threshold, and its next call with detect = 0 meets the bar against float64 of that state.  Pooled and
producer-mask rows: segments the producer mask does not cover keep state and mask under a changed decoy pixel.  The
upstream count: 0 leaves everything but countOut (0) and the mask copy (empty) untouched.  A layer split along k and
the same layer unsplit give identical bits: four chunks on both 64-row instances (test_split_and_unsplit_...), eight
and sixteen chunks where a group launch runs unsplit and its layers alone split (frame 0 of group-unequal-chunks,
frame 1 of group-split16-beside-whole).  No 128-row layer is compared that way: an unsplit 128-row launch is beyond
the reference budget (hsplit_cases.uncovered).

A: the provable ceiling is (C kH kW + 2) 2^-24 (products of f16 values are exact in f32; the sum is taken in f32 in some
order).  Observed worst (|err| - rounding terms) / (sum|a||b| + |bias|) on an MI355X (256 CUs), 2026-10-20, printed by
test_zz_report_worst_ratios ("rounding": no element's error exceeded its two rounding terms):
    128-row, mask in LDS:     one_stage 2^-25.2, shallow 2^-26.0, deep_split8 2^-27.1, deep_split16 2^-27.3, frame 0 2^-25.0
    128-row, mask in memory:  one_stage 2^-24.3, shallow rounding, deep_split8 / 16 rounding, frame 0 2^-24.3
    64-row, mask in LDS:      one_stage rounding, shallow 2^-26.5, deep_whole 2^-25.8, deep_split4 2^-27.1,
                              deep_split8 2^-28.2, deep_split16 2^-27.0, frame 0 2^-25.1
    64-row, mask in memory:   one_stage rounding, shallow 2^-25.7, deep_whole 2^-26.7, deep_split4 / 8 / 16 rounding,
                              frame 0 2^-25.6
    consumers' own frames 2^-25.4, producer-mask and pooled rows 2^-27.5, upstream rows 2^-27.8
All of it far below 2^-20, so A = min(ceiling, 64 * 2^-24) = 2^-18 (hsplit_cases.bar_A): the bar the f32 split-state
forms carry; the ceiling alone would be up to 2^-10.9 (C = 185 under 7x7).
"""
import functools
import zlib

import numpy as np
import pytest
import torch

import hsplit_cases as hc
from hsplit_cases import CASES, CASE_BY_ID, TH, cell_of
from test_gpu_detect_edges import pool2
from test_gpu_splitconv import cus, mask_bits, reference
from optest import dev, gpu_lib as lib, raw      # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

FILL = 7.25
WORST = {}
RAN = set()       # ids of the cases whose frames test ran to its end
IDS = [c.id for c in CASES]
# (bias, relu): bias alone (no output clamped: every one tells of the arithmetic), ReLU alone, neither
EPILOGUES = [(True, False), (False, True), (False, False)]


def bits16(a):
    return np.ascontiguousarray(a).view(np.uint16)


class HL(object):
    """The buffers of one fp16 layer [C -> K, kH x kW] on an H x W map, fresh: states at +inf, outputs at FILL."""

    def __init__(self, lib, C, K, kH, kW, H, W, w, b):
        C_ = lib.C
        self.lib, self.C, self.K, self.kH, self.kW, self.H, self.W = lib, C, K, kH, kW, H, W
        self.geo = (C, H, W, kH, kW)
        assert C_.cbinfer_hsplit_supported(C, K, kH, kW) == 1
        self.state = torch.full((1, C, H, W), float("inf"), dtype=torch.float16, device="cuda")
        self.S = self.pixel_state(init_only=True)
        self.MW = C_.cbinfer_mask_words(H, W)
        self.masks = torch.zeros(C_.cbinfer_frame_mask_bytes(H, W) // 8, dtype=torch.int64, device="cuda")
        self.out = torch.full((1, K, H, W), FILL, dtype=torch.float16, device="cuda")
        self.idx = torch.full((H * W,), -1, dtype=torch.int32, device="cuda")
        self.cnt = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        self.copy = torch.full((self.MW,), -1, dtype=torch.int64, device="cuda")
        self.w, self.b = dev(w), dev(b)
        self.wp = torch.empty(C_.cbinfer_hsplit_prepared_bytes(C, K, kH, kW), dtype=torch.uint8, device="cuda")
        lib.check(C_.cbinfer_hsplit_prep_weights(self.w.data_ptr(), self.wp.data_ptr(), K, C, kH, kW, H, W, None))

    def pixel_state(self, init_only=False):
        """A fresh pixel-major copy of the state tensor."""
        C_ = self.lib.C
        S = torch.empty(C_.cbinfer_hsplit_state_bytes(*self.geo), dtype=torch.uint8, device="cuda")
        self.lib.check(C_.cbinfer_hsplit_state_init(S.data_ptr(), *self.geo, None))
        if not init_only:
            self.lib.check(C_.cbinfer_hsplit_state_rebuild(self.state.data_ptr(), S.data_ptr(), *self.geo, None))
        return S

    def list(self):
        return self.idx[:int(self.cnt.item())].cpu().numpy()

    def clean(self, what):
        assert not bool(self.masks.ne(0).any()), what + ": the frame masks (mask, arrival counters) are not zero again"


def workspace_of(lib, nL, C, H, W, K, kH, kW):
    n = lib.C.cbinfer_hsplit_group_workspace_bytes(nL, C, H, W, K, kH, kW)
    return torch.zeros(n, dtype=torch.uint8, device="cuda") if n else None


def workspace(lib, c, nL):
    return workspace_of(lib, nL, c.C, c.H, c.W, c.Ks[0], c.kH, c.kW)


@functools.lru_cache(maxsize=4)
def frames_of(cid, q):
    return hc.make_frames(CASE_BY_ID[cid], q)


def call(lib, c, Ls, ws, fb, bias, relu, inputs=None, pooled=False, prod=None, upstream=None, nexts=None, th=TH,
         geo=None):
    """One cbinfer_hsplit_forward_group call on the layers Ls; inputs None: detect = 0.  Returns the status."""
    arr = (lib.HalfLayer * len(Ls))()
    for q, L in enumerate(Ls):
        a = arr[q]
        a.upstreamCount = upstream.data_ptr() if upstream is not None else None
        a.input = inputs[q].data_ptr() if inputs is not None else None
        a.producerMask = prod[q].data_ptr() if prod is not None else None
        a.state, a.pixelState, a.frameMasks, a.output = (L.state.data_ptr(), L.S.data_ptr(), L.masks.data_ptr(),
                                                        L.out.data_ptr())
        a.idxOut, a.countOut, a.maskCopy = L.idx.data_ptr(), L.cnt.data_ptr(), L.copy.data_ptr()
        a.prepared, a.bias = L.wp.data_ptr(), (L.b.data_ptr() if bias else None)
        a.K, a.threshold, a.relu, a.detect = L.K, th, int(relu), int(inputs is not None)
        ns = nexts[q] if nexts is not None else []
        a.nNext = len(ns)
        for i, n in enumerate(ns):
            a.next[i].state, a.next[i].pixelState, a.next[i].frameMasks = n.state.data_ptr(), n.S.data_ptr(), n.masks.data_ptr()
            a.next[i].kH, a.next[i].kW, a.next[i].threshold = n.kH, n.kW, n.th
    C, H, W, kH, kW = geo if geo is not None else (c.C, c.H, c.W, c.kH, c.kW)
    pH, pW = (inputs[0].shape[-2], inputs[0].shape[-1]) if pooled else (0, 0)
    st = lib.C.cbinfer_hsplit_forward_group(arr, len(Ls), int(pooled), pH, pW, C, H, W, kH, kW, int(fb),
                                            ws.data_ptr() if ws is not None else None, None)
    torch.cuda.synchronize()
    return st


def oracle_walk(oracle, frames, filt, fb, th=TH, state=None):
    """Per frame (list, refreshed state, dilated map) of the oracle's half state machine; frames: what the detection
    may look at."""
    out = []
    for x in frames:
        if state is None:
            state = np.full(x.shape, np.inf, dtype=np.float16)
        with np.errstate(invalid="ignore", over="ignore"):
            raw = oracle.changeDetection_half(x, state, (1, 1), th, updateInputState=bool(fb))
        if not fb:
            state = x.copy()
        cmap = oracle.changePropagation(raw, filt)
        out.append((oracle.changeIndexesExtr(cmap), state.copy(), cmap))
    return out


def with_reference(oracle, walk, w, sel0=None):
    """(idx, state, cmap, sel, y, mag) per frame: the float64 products at idx[sel]."""
    refs = []
    for t, (idx, state, cmap) in enumerate(walk):
        sel = np.arange(len(idx)) if (t > 0 or sel0 is None) else sel0
        y, mag = reference(oracle, state, idx[sel], w)
        refs.append((idx, state, cmap, sel, y, mag))
    return refs


def note_worst(key, ratio):
    WORST[key] = max(WORST.get(key, -1.0), float(ratio))


def check_outputs(key, what, A, L, before, idx, sel, y, mag, b, relu):
    """L.out after the launch against float64 at idx[sel]; before: its bits in front of the launch ([K, HW])."""
    K, HW = L.K, L.H * L.W
    now = L.out.cpu().numpy().reshape(K, HW)
    want = y + (b.astype(np.float64)[None, :] if b is not None else 0.0)
    if relu:
        want = np.maximum(want, 0.0)
    m = mag + (np.abs(b).astype(np.float64)[None, :] if b is not None else 0.0)
    got = now[:, idx[sel]].T.astype(np.float64)
    err = np.abs(got - want)
    ratio = float(((err - hc.rounding_terms(want)) / (m + 1e-300)).max()) if err.size else 0.0
    print("%s: %d of %d listed compared, max |err| %.3g, worst (err - rounding) / (sum|a||b| + |bias|) %.3g" % (
        what, len(sel), len(idx), err.max() if err.size else 0.0, ratio))
    note_worst(key, ratio)
    assert np.all(np.isfinite(got)), what
    assert np.all(err <= hc.bar(want, m, A)), (what, ratio, A)
    # the layer's global bar: two f16 ulps of its largest output
    want16 = want.astype(np.float16).astype(np.float64)
    tol = 2 * 2.0 ** -10 * max(1.0, float(np.abs(want16).max()) if want16.size else 0.0)
    assert np.all(np.abs(got - want16) <= tol), (what, float(np.abs(got - want16).max()), tol)
    rest = np.ones(HW, bool)
    rest[idx] = False
    assert np.array_equal(bits16(now[:, rest]), bits16(before[:, rest])), what + ": a pixel off the list changed"


def check_second(what, L, second, b, relu):
    """Frame 0 of a sample0 case: every output of the layer is finite, and a second, independent sample of the pixels
    meets the layer's 2-ulp bar."""
    sel2, y2 = second
    now = L.out.cpu().numpy().reshape(L.K, -1)
    assert np.all(np.isfinite(now)), what + ": an output is not finite"
    want = y2 + (b.astype(np.float64)[None, :] if b is not None else 0.0)
    if relu:
        want = np.maximum(want, 0.0)
    want16 = want.astype(np.float16).astype(np.float64)
    tol = 2 * 2.0 ** -10 * max(1.0, float(np.abs(want16).max()))
    d = np.abs(now[:, sel2].T.astype(np.float64) - want16)
    assert np.all(d <= tol), (what + ": second sample", float(d.max()), tol)


def check_frame(what, L, idx, state, cmap):
    assert int(L.cnt.item()) == len(idx), (what, int(L.cnt.item()), len(idx))
    assert np.array_equal(L.list(), idx), what + ": change list"
    assert np.array_equal(mask_bits(L.copy, L.H, L.W), cmap), what + ": mask copy"
    assert np.array_equal(bits16(L.state.cpu().numpy()), bits16(state)), what + ": prevInput"


def check_header(what, ws, f, counts):
    """The launch info a deep contraction leaves for its second launch."""
    if not f["deep"]:
        assert ws is None
        return
    info = ws[:256].view(torch.int32).cpu().numpy()
    nL = len(counts)
    assert (info[0], info[1], info[2]) == (f["SK"], f["MT"], nL), (what, info[:4], f)
    assert info[4:4 + nL].tolist() == f["tiles"] and info[12:12 + nL].tolist() == list(counts), (what, info[:16], f)
    assert info[24:24 + nL].tolist() == f["chunks"], (what, info[24:26], f)
    if nL == 1:
        assert info[25] == hc.CHUNKS and info[5] == 0      # (the absent second layer: no tiles, the base chunk count)


def run_config(lib, c, qs, refs, fb, bias, relu, wb, claim, second=None):
    """The three frames of one configuration on the layers qs of the case in ONE launch; returns the layers."""
    Ls = [HL(lib, c.C, c.Ks[q], c.kH, c.kW, c.H, c.W, *wb[q]) for q in qs]
    ws = workspace(lib, c, len(qs))
    A = hc.bar_A(c.C, c.kH, c.kW)
    for t in range(3):
        what = "%s layers %s frame %d fb %d bias %d relu %d" % (c.id, qs, t, fb, bias, relu)
        before = [L.out.cpu().numpy().reshape(L.K, -1).copy() for L in Ls]
        xs = [dev(frames_of(c.id, q)[t]) for q in qs]
        lib.check(call(lib, c, Ls, ws, fb, bias, relu, xs))
        counts = [len(refs[q][t][0]) for q in qs]
        f = hc.hsplit_form(c.C, [c.Ks[q] for q in qs], c.kH, c.kW, c.H, c.W, counts, cus())
        assert f["status"] == hc.OK
        key = cell_of(f)[:2] if t == 1 else (cell_of(f)[0], "frame %d" % t)
        for L, q in zip(Ls, qs):
            idx, state, cmap, sel, y, mag = refs[q][t]
            check_frame("%s layer %d" % (what, q), L, idx, state, cmap)
            check_outputs(key, "%s layer %d" % (what, q), A, L, before[qs.index(q)], idx, sel, y, mag,
                          wb[q][1] if bias else None, relu)
            if t == 0 and second is not None:
                check_second("%s layer %d" % (what, q), L, second[q], wb[q][1] if bias else None, relu)
        for L in Ls:
            L.clean(what)
        check_header(what, ws, f, counts)
        if t == 1 and claim:
            assert counts == hc.layer_counts(c), (what, counts)
            assert cell_of(f) == c.cell, ("%s: on a card with %d CUs this shape lands in %s, not in the cell %s it was "
                                          "written for (%s)" % (c.id, cus(), cell_of(f), c.cell, f))
        if t == 2:
            assert sum(counts) == 0
    for L in Ls:
        assert torch.equal(L.S, L.pixel_state()), "%s: the pixel-major copy is not the state's" % what
    return Ls


def case_refs(oracle, c, fb, wb):
    """Per layer the frames' references, and -- sample0 -- the second sample of frame 0 (every pixel is listed then: a
    pixel's index is its place in the list)."""
    sampled = bool(c.opts.get("sample0"))
    refs, second = [], ([] if sampled else None)
    for q in range(len(c.Ks)):
        walk = oracle_walk(oracle, frames_of(c.id, q), (c.kH, c.kW), fb)
        refs.append(with_reference(oracle, walk, wb[q][0], hc.sample0(c) if sampled else None))
        if sampled:
            sel2 = hc.sample0_second(c)
            assert len(walk[0][0]) == c.H * c.W
            second.append((sel2, reference(oracle, walk[0][1], sel2.astype(np.int32), wb[q][0])[0]))
    return refs, second


@pytest.mark.parametrize("cid", IDS)
def test_case_frames_against_float64(lib, oracle, cid):
    c = CASE_BY_ID[cid]
    f = hc.case_form(c, cus())
    assert f["status"] == hc.OK and cell_of(f) == c.cell, (cid, cus(), cell_of(f), c.cell)
    nL = len(c.Ks)
    wb = [hc.make_weights(c, q) for q in range(nL)]
    for fb in (1, 0):
        refs, second = case_refs(oracle, c, fb, wb)
        for bias, relu in EPILOGUES:
            Ls = run_config(lib, c, list(range(nL)), refs, fb, bias, relu, wb, claim=True, second=second)
            if nL > 1 and bias:
                # every layer of the group launched alone: pinned the same way, and the same bits
                for q in range(nL):
                    alone = run_config(lib, c, [q], refs, fb, bias, relu, wb, claim=False)[0]
                    assert torch.equal(alone.out, Ls[q].out), (cid, fb, q)
                    assert torch.equal(alone.state, Ls[q].state) and torch.equal(alone.S, Ls[q].S), (cid, fb, q)
    RAN.add(cid)


@pytest.mark.parametrize("fb", [1, 0])
@pytest.mark.parametrize("cid", ["h64lds-shallow-c185-k38", "h64lds-split16-c185-k38", "pooled-prodmask-shallow"])
def test_single_layer_entry_equals_the_group_call(lib, cid, fb):
    """cbinfer_hsplit_forward packs its arguments into one cbHalfLayer: the three frames through it leave the bits the
    group call of one layer leaves (pinned above) in every buffer -- with an upstream count, a ReLU, and for the pooled
    row the pool's input and a producer mask."""
    c = CASE_BY_ID[cid]
    pooled = bool(c.opts.get("pooled"))
    w, b = hc.make_weights(c)
    A, B = (HL(lib, c.C, c.Ks[0], c.kH, c.kW, c.H, c.W, w, b) for _ in range(2))
    wsA, wsB = workspace(lib, c, 1), workspace(lib, c, 1)
    up = dev(np.array([3], np.int32))
    rng = np.random.default_rng(7)
    for t, x in enumerate(frames_of(cid, 0)):
        xin = dev(pool_input(rng, x) if pooled else x)
        pH, pW = (xin.shape[-2], xin.shape[-1]) if pooled else (0, 0)
        pm = torch.full((lib.C.cbinfer_mask_words(pH, pW),), -1, dtype=torch.int64, device="cuda") if pooled else None
        lib.check(call(lib, c, [A], wsA, fb, True, True, [xin], pooled=pooled, prod=[pm] if pooled else None, upstream=up))
        lib.check(lib.C.cbinfer_hsplit_forward(
            up.data_ptr(), xin.data_ptr(), int(pooled), pH, pW, pm.data_ptr() if pooled else None, B.state.data_ptr(),
            B.S.data_ptr(), B.masks.data_ptr(), B.out.data_ptr(), B.idx.data_ptr(), B.cnt.data_ptr(), B.copy.data_ptr(),
            B.wp.data_ptr(), B.b.data_ptr(), c.C, c.H, c.W, c.Ks[0], c.kH, c.kW, TH, fb, 1,
            wsB.data_ptr() if wsB is not None else None, None))
        torch.cuda.synchronize()
        for name in ("out", "state", "S", "masks", "idx", "cnt", "copy"):
            assert torch.equal(getattr(A, name), getattr(B, name)), (cid, fb, t, name)
        if wsA is not None:
            assert torch.equal(wsA[:256], wsB[:256]), (cid, fb, t)
        assert int(B.cnt.item()) == [c.H * c.W, hc.layer_counts(c)[0], 0][t], (cid, fb, t)


# ---------------------------------------------------------------------------------------------------------------------
# consumers: their detection in the producing launch, their own call with detect = 0
# ---------------------------------------------------------------------------------------------------------------------
class Consumer(HL):
    """A copy-mode layer [K -> 3, kH x kW] behind a producer of K channels, with its own threshold."""

    def __init__(self, lib, c, K, spec, seed):
        kH, kW, th = spec
        rng = np.random.default_rng(seed)
        w = (rng.standard_normal((3, K, kH, kW)) / np.sqrt(K * kH * kW)).astype(np.float16)
        HL.__init__(self, lib, K, 3, kH, kW, c.H, c.W, w, rng.standard_normal(3).astype(np.float16))
        self.th, self.wnp, self.bnp = th, w, self.b.cpu().numpy()


@pytest.mark.parametrize("fb", [1, 0])
@pytest.mark.parametrize("cid", [c.id for c in CASES if "next" in c.opts])
def test_consumers_ride_in_the_producing_launch(lib, oracle, cid, fb):
    c = CASE_BY_ID[cid]
    nL = len(c.Ks)
    wb = [hc.make_weights(c, q) for q in range(nL)]
    Ls = [HL(lib, c.C, c.Ks[q], c.kH, c.kW, c.H, c.W, *wb[q]) for q in range(nL)]
    plain = [HL(lib, c.C, c.Ks[q], c.kH, c.kW, c.H, c.W, *wb[q]) for q in range(nL)]      # the same layers without consumers
    ws, ws_plain = workspace(lib, c, nL), workspace(lib, c, nL)
    nexts = [[Consumer(lib, c, c.Ks[q], spec, 100 * q + i) for i, spec in enumerate(c.opts["next"][q])] for q in range(nL)]
    for t in range(3):
        what = "%s frame %d fb %d" % (cid, t, fb)
        xs = [dev(frames_of(cid, q)[t]) for q in range(nL)]
        old = [[n.state.cpu().numpy() for n in ns] for ns in nexts]
        lib.check(call(lib, c, Ls, ws, fb, True, True, xs, nexts=nexts))
        lib.check(call(lib, c, plain, ws_plain, fb, True, True, xs))
        counts = [int(L.cnt.item()) for L in Ls]
        f = hc.hsplit_form(c.C, c.Ks, c.kH, c.kW, c.H, c.W, counts, cus(), n_next=hc.n_next(c))
        check_header(what, ws, f, counts)
        if t == 1:
            assert cell_of(f) == c.cell and counts == hc.layer_counts(c), (what, cell_of(f), counts)
        for q, L in enumerate(Ls):
            assert torch.equal(L.out, plain[q].out) and torch.equal(L.idx, plain[q].idx), what
            new = L.out.cpu().numpy()
            for i, n in enumerate(nexts[q]):
                tag = "%s layer %d consumer %d" % (what, q, i)
                assert torch.equal(n.state, L.out), tag + ": the consumer's state is not the producer's output"
                assert torch.equal(n.S, n.pixel_state()), tag + ": pixel-major copy"
                (idx, _, cmap), = oracle_walk(oracle, [new], (n.kH, n.kW), 0, n.th, state=old[q][i].copy())
                got = mask_bits(n.masks[:n.MW], c.H, c.W)
                assert np.array_equal(got, cmap), tag + ": frame mask"
                assert not bool(n.masks[n.MW:].ne(0).any()), tag
                # the consumer's own frame: its contraction alone, on the state the producer wrote
                before = n.out.cpu().numpy().reshape(n.K, -1).copy()
                nws = workspace_of(lib, 1, n.C, c.H, c.W, n.K, n.kH, n.kW)
                lib.check(call(lib, c, [n], nws, 0, True, False, None, th=n.th, geo=n.geo))
                check_frame(tag, n, idx, new, cmap)
                y, mag = reference(oracle, new, idx, n.wnp)
                check_outputs(("consumer", f["regime"] if t == 1 else "frame %d" % t), tag, hc.bar_A(n.C, n.kH, n.kW), n, before, idx,
                              np.arange(len(idx)), y, mag, n.bnp, False)
                n.clean(tag)
        for L in Ls:
            L.clean(what)
        if t > 0:      # something reached the consumers, and not everything
            tot = [len(np.flatnonzero(mask_bits(n.copy, c.H, c.W))) for ns in nexts for n in ns]
            assert all(0 <= v < c.H * c.W for v in tot) and (t == 2 or any(v > 0 for v in tot)), (what, tot)


# ---------------------------------------------------------------------------------------------------------------------
# pooled detection, producer masks
# ---------------------------------------------------------------------------------------------------------------------
def pool_input(rng, x):
    """[1, C, 2H-1, 2W-1] f16 whose 2x2 / stride-2 ceil-mode max pool is x: one pixel of every window holds the value,
    the others less."""
    _, C, H, W = x.shape
    big = np.repeat(np.repeat(x.astype(np.float32), 2, axis=2), 2, axis=3)
    low = big - rng.uniform(0.25, 2.0, big.shape).astype(np.float32)
    keep = np.zeros((2 * H, 2 * W), bool)
    keep[::2, ::2] = True      # (the corner every window has, the clamped last ones too)
    p = np.where(keep[None, None], big, low).astype(np.float16)[:, :, :2 * H - 1, :2 * W - 1]
    assert np.array_equal(bits16(pool2(p)), bits16(x))
    return np.ascontiguousarray(p)


@pytest.mark.parametrize("fb", [1, 0])
@pytest.mark.parametrize("cid", [c.id for c in CASES if c.opts.get("pooled") or c.opts.get("prodmask")])
def test_producer_masks_and_pooled_detection(lib, oracle, cid, fb):
    """Frame 0 without a producer mask, frame 1 with one that covers the change set's segments and not the decoy's,
    frame 2 with an empty one."""
    c = CASE_BY_ID[cid]
    pooled = bool(c.opts.get("pooled"))
    rng = np.random.default_rng(zlib.crc32(cid.encode()))
    w, b = hc.make_weights(c)
    L = HL(lib, c.C, c.Ks[0], c.kH, c.kW, c.H, c.W, w, b)
    ws = workspace(lib, c, 1)
    H, W, wpr = c.H, c.W, (c.W + 63) // 64
    x0, x1, _ = hc.make_frames(c)
    m = hc.changed_pixels(c)
    dy, dx = H - 2, 5                                   # the decoy: a changed pixel in a segment nobody covers
    assert not m[dy, :64].any()
    x1 = x1.copy()
    x1[0, 0, dy, dx] = x0[0, 0, dy, dx] + np.float16(2.0)
    mh, mw = (2 * H - 1, 2 * W - 1) if pooled else (H, W)
    prod = np.zeros((mh, (mw + 63) // 64), dtype=np.uint64)
    for y, x in zip(*np.nonzero(m)):
        yy, xx = (2 * y, 2 * x) if pooled else (y, x)
        prod[yy, xx >> 6] |= np.uint64(1) << np.uint64(xx & 63)
    covered = np.zeros((H, W), bool)
    for y in range(H):
        for tx in range(wpr):
            hit = prod[2 * y:2 * y + 2, 2 * tx:2 * tx + 2].any() if pooled else prod[y, tx] != 0
            covered[y, tx * 64:(tx + 1) * 64] = hit
    assert covered[m].all() and not covered[dy, dx] and not covered.all()
    state = np.full(x0.shape, np.inf, dtype=np.float16)
    A = hc.bar_A(c.C, c.kH, c.kW)
    for t, (x, pm) in enumerate(((x0, None), (x1, prod), (x1, np.zeros_like(prod)))):
        what = "%s frame %d fb %d" % (cid, t, fb)
        seen = x if pm is None else np.where((covered if t == 1 else np.zeros_like(covered))[None, None], x, state)
        (idx, state, cmap), = oracle_walk(oracle, [seen], (c.kH, c.kW), fb, state=state)
        xin = dev(pool_input(rng, x) if pooled else x)
        pmd = [dev(pm.view(np.int64))] if pm is not None else None
        before = L.out.cpu().numpy().reshape(L.K, -1).copy()
        lib.check(call(lib, c, [L], ws, fb, True, False, [xin], pooled=pooled, prod=pmd))
        check_frame(what, L, idx, state, cmap)
        y, mag = reference(oracle, state, idx, w)
        f = hc.hsplit_form(c.C, c.Ks, c.kH, c.kW, H, W, [len(idx)], cus(), pooled=pooled)
        check_outputs(("masked", f["regime"] if t == 1 else "frame %d" % t), what, A, L, before, idx, np.arange(len(idx)), y, mag, b, False)
        check_header(what, ws, f, [len(idx)])
        L.clean(what)
        assert torch.equal(L.S, L.pixel_state()), what
        if t == 1:
            assert cell_of(f) == c.cell and len(idx) == hc.layer_counts(c)[0], (what, cell_of(f), len(idx))
            # the decoy stayed unseen: its state is frame 0's, its pixel is not in the mask
            assert bits16(state[0, 0, dy, dx]) == bits16(x0[0, 0, dy, dx]) and not cmap[dy, dx]
        if t == 2:
            assert len(idx) == 0


# ---------------------------------------------------------------------------------------------------------------------
# the upstream count
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fb", [1, 0])
@pytest.mark.parametrize("cid", [c.id for c in CASES if c.opts.get("upstream")])
def test_upstream_count(lib, oracle, cid, fb):
    """A non-zero count changes nothing; 0 ends the frame at once: countOut 0, the mask copy empty, output, states and
    masks untouched -- whatever the input holds.  The frame after it finds the change."""
    c = CASE_BY_ID[cid]
    w, b = hc.make_weights(c)
    L = HL(lib, c.C, c.Ks[0], c.kH, c.kW, c.H, c.W, w, b)
    ws = workspace(lib, c, 1)
    x0, x1, _ = hc.make_frames(c)
    some, none = dev(np.array([5], np.int32)), dev(np.array([0], np.int32))
    walk = with_reference(oracle, oracle_walk(oracle, [x0, x1], (c.kH, c.kW), fb), w)
    A = hc.bar_A(c.C, c.kH, c.kW)

    def frame(t, x, up):
        what = "%s frame %d fb %d" % (cid, t, fb)
        idx, state, cmap, sel, y, mag = walk[t]
        before = L.out.cpu().numpy().reshape(L.K, -1).copy()
        lib.check(call(lib, c, [L], ws, fb, True, False, [dev(x)], upstream=up))
        check_frame(what, L, idx, state, cmap)
        f = hc.hsplit_form(c.C, c.Ks, c.kH, c.kW, c.H, c.W, [len(idx)], cus())
        check_outputs(("upstream", f["regime"] if t == 1 else "frame %d" % t), what, A, L, before, idx, sel, y, mag, b, False)
        check_header(what, ws, f, [len(idx)])
        L.clean(what)
    frame(0, x0, some)
    keep = [t.clone() for t in (L.out, L.state, L.S, L.masks, L.idx)]
    L.copy.fill_(-1), L.cnt.fill_(-1)
    lib.check(call(lib, c, [L], ws, fb, True, False, [dev(x1)], upstream=none))      # (x1 holds changes: nobody looks)
    assert int(L.cnt.item()) == 0 and not bool(L.copy.ne(0).any())
    for a, k in zip((L.out, L.state, L.S, L.masks, L.idx), keep):
        assert torch.equal(a, k)
    if ws is not None:
        assert int(ws[:4].view(torch.int32).item()) == 1      # (nothing for the second launch)
    frame(1, x1, some)


# ---------------------------------------------------------------------------------------------------------------------
# split and unsplit: the same bits
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["h64lds-split4-one", "h64mem-split4-one"])
def test_split_and_unsplit_give_identical_bits(lib, oracle, cid):
    """The chunk boundaries are the layer's: the case's change set (66 tiles: four chunks each, slabs and the reduce
    launch) and a frame that changes every pixel (unsplit: one workgroup folds its accumulators at the same boundaries)
    leave the same bits at the pixels both list.  Copy mode: both states are the frame."""
    c = CASE_BY_ID[cid]
    w, b = hc.make_weights(c)
    x0, x1, _ = hc.make_frames(c)
    y0 = x0.copy()
    y0[0, 0] += np.float16(4.0)                         # every pixel of x1 is far from this one
    outs = []
    for first, sk in ((x0, 4), (y0, 1)):
        L = HL(lib, c.C, c.Ks[0], c.kH, c.kW, c.H, c.W, w, b)
        ws = workspace(lib, c, 1)
        for x in (first, x1):
            lib.check(call(lib, c, [L], ws, 0, True, True, [dev(x)]))
        info = ws[:256].view(torch.int32).cpu().numpy()
        assert info[0] == sk, (cid, sk, info[:4])
        assert torch.equal(L.state, dev(x1))
        outs.append((L.out.cpu().numpy().reshape(L.K, -1), L.list()))
    (a, ia), (bb, ib) = outs
    assert len(ia) == hc.layer_counts(c)[0] and len(ib) > 128 * 64 and np.isin(ia, ib).all()
    assert np.array_equal(bits16(a[:, ia]), bits16(bb[:, ia]))


# ---------------------------------------------------------------------------------------------------------------------
# argument checks: no kernel runs
# ---------------------------------------------------------------------------------------------------------------------
def test_refused_launches(lib):
    c = CASE_BY_ID["h64lds-one-c64-k38-all"]

    def layers(Ks, kH=3, kW=3):
        return [HL(lib, 64, K, kH, kW, c.H, c.W, np.zeros((K, 64, kH, kW), np.float16), np.zeros(K, np.float16)) for K in Ks]
    x = dev(np.zeros((1, 64, c.H, c.W), np.float16))
    geo = (64, c.H, c.W, 3, 3)
    for Ks in ((64, 65), (65, 129)):      # the tile height, the padded K
        Ls = layers(Ks)
        assert hc.hsplit_form(64, Ks, 3, 3, c.H, c.W, [0, 0], cus())["status"] == hc.UNSUPPORTED
        assert call(lib, c, Ls, None, 1, True, False, [x, x], geo=geo) == hc.UNSUPPORTED
        assert all(int(L.cnt.item()) == -1 and bool(torch.isinf(L.state).all()) for L in Ls)
    L, = layers((38,))
    n = Consumer(lib, c, 64, (3, 3, 0.1), 1)      # (its buffers only: a consumer behind 38 channels is refused)
    assert call(lib, c, [L], None, 1, True, False, [x], nexts=[[n]], geo=geo) == hc.UNSUPPORTED
    L7, = layers((38,), 7, 7)
    assert call(lib, c, [L7], None, 1, True, False, [x], geo=(64, c.H, c.W, 7, 7)) == hc.BADARG
    for q in (L, L7):
        assert int(q.cnt.item()) == -1 and bool(torch.isinf(q.state).all()) and not bool(q.masks.ne(0).any())


def test_zz_report_worst_ratios(capsys):
    """Not a check of the kernels: prints the worst ratio per cell seen by the tests above, and fails if a case of the
    table did not run."""
    with capsys.disabled():
        print("\nworst (|err| - rounding terms) / (sum|a||b| + |bias|) per instance and regime (A = 2^%.1f .. 2^%.1f):" % (
            np.log2(min(hc.bar_A(c.C, c.kH, c.kW) for c in CASES)), np.log2(max(hc.bar_A(c.C, c.kH, c.kW) for c in CASES))))
        for key, r in sorted(WORST.items()):
            print("  %-28s %-14s %.3g (%s)" % (key[0], key[1], r, "2^%.1f" % np.log2(r) if r > 0 else "within the rounding"))
    missing = [c.id for c in CASES if c.id not in RAN]
    assert not missing, "cases of the table that did not run to their end: %s" % missing
