"""-m gpu: every case of tests/maskconv_cases.py through the C ABI of the three mask-driven contractions -- the
row-segment kernel (cb_rowconv.hip), the patch-staged bf16x3 kernel (cb_blockconv.hip) and the row-pair kernel
(cb_rowpair.hip: plain, with the next layer's pooled detection folded in, with its own detection, and on grids whose
workgroups take up to four candidate units) -- pinned against float64 math: oracle.genXMatrix patches of the state times
the weights in double, plus the bias, at every listed pixel and every output channel.

Per case, with bias alone and with ReLU alone: the listed outputs are finite, within 1e-4 and within
64 * 2^-24 * (sum|a||b| + |bias|) per element, every other output keeps the bits of a random pre-fill, the mask copy
equals the mask, the mask and the arrival counters are zero afterwards, a second launch on the emptied mask changes
nothing, and the case ran in the cell it claims on this card.  Accumulate cases: out0 + conv(W, delta) under the same two
bars with |out0| in the bound, reluOut = max(out, 0) of the stored output at the touched pixels and untouched elsewhere.

The operands: state channels scaled by exp(U(-6, 1)), output channels' weights by exp(U(-4, 1)) / sqrt(C kH kW).  With
these sum|a||b| stays below about 26 = 1e-4 / (64 * 2^-24), the magnitude at which the flat bar and the scaled one meet:
beyond it the flat bar would ask more of f32 arithmetic than the project's own bound does.

Bit-identity: a pixel's bits of the block and row-pair kernels do not depend on the rest of the mask (every tile has
accumulators of its own over a fixed step order: a map against a subset of its pixels); a row-pair unit's outputs are the
same whichever candidate slot and sequence index it runs under (a slot case against single-sequence launches of crops of
its content) and whether the launch detects the changes itself or is fed the mask; the row-segment kernel's k-parts meet
in LDS in a fixed order (the same launch twice).

Fold cases: the next layer's detection restated in numpy on the GPU's own outputs -- 2x2 max with the floor / ceil edge
handling, changed = window holds a listed pixel and fabsf(state - pooled) > th in any channel (float32), the changed
pixels take the pooled values in every channel, the frame mask is the changed set dilated by the next filter's support,
the pre-split copy equals a freshly initialised and rebuilt copy of the expected state (byte-exact by construction: the
rebuild writes every record with the split the fold uses, and the states here are finite), the range flag as
cbs_store_part would set it.

Observed worst |err| / (sum|a||b| + |bias| or |out0|) on an MI355X, 2026-10-19 (printed per cell by
test_zz_report_worst_ratios; the bar is 64 * 2^-24 = 2^-18):
    rows:   2^-21.3 (7x7x1 2^-22.0, 7x7x4 2^-22.0, run-time shapes 2^-21.3; accumulate 2^-22.3, batched 2^-21.7)
    blocks: 2^-21.2 (plain 2^-21.2, accumulate 2^-21.2, sparse 2^-21.9)
    pair:   2^-21.5 (plain 2^-22.3, folds 2^-22.2, own detection 2^-21.5, slots 1..3 2^-22.4)
The sparse block cases have teeth at that bar: a build of cb_blockconv.hip without the al * bh product failed all five
of them (worst ratio 2^-17.0 to 2^-17.1, max |err| 1e-6 .. 6e-6) while every dense block case, plain and accumulate,
still passed both bars.  A build of cb_rowconv.hip that skips the remainder block failed every row-segment case with
NB == 0 or rem != 0 on a map tall and wide enough for the last taps to reach a pixel (27 cases), and passed the five
rem == 0 shapes and the 7x7 cases on the 2 x 3 and 1 x 130 maps, where the skipped taps (filter row 6) lie off the map.
"""
import ctypes
import zlib

import numpy as np
import pytest
import torch

import maskconv_cases as mc
from maskconv_cases import CASES, CASE_BY_ID
from optest import dev, gpu_lib as lib, pack      # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

FP32_TOL = 1e-4
BOUND = 64 * 2.0 ** -24
RELU_FILL = -5.0
WORST = {}
RAN = set()       # ids of the cases whose test ran to its end

PLAIN_IDS = [c.id for c in CASES if c.kernel != "pair"]
PAIR_IDS = [c.id for c in CASES if c.kernel == "pair" and not ({"det", "slots"} & set(dict(c.opt)))]
DET_IDS = [c.id for c in CASES if "det" in dict(c.opt)]
SLOT_IDS = [c.id for c in CASES if "slots" in dict(c.opt)]
assert len(PLAIN_IDS) + len(PAIR_IDS) + len(DET_IDS) + len(SLOT_IDS) == len(CASES)


def cus():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def assert_claimed_cell(c):
    got = mc.case_cell(c, cus())
    assert got == c.cell, ("%s: on a card with %d CUs this shape lands in %s, not in the cell %s it was written for"
                           % (c.id, cus(), got, c.cell))


def unpack_mask(words, H, W):
    wpr = (W + 63) // 64
    w = np.ascontiguousarray(words).view(np.uint8)
    return np.unpackbits(w, bitorder="little").reshape(H, wpr * 64)[:, :W].astype(bool)


def make_weights(rng, c):
    K, C, kH, kW = c.K, c.C, c.kH, c.kW
    w = (rng.standard_normal((K, C, kH, kW)) / np.sqrt(C * kH * kW) *
         np.exp(rng.uniform(-4, 1, (K, 1, 1, 1)))).astype(np.float32)
    return w, rng.standard_normal(K).astype(np.float32)


def make_state(rng, C, H, W):
    x = (rng.standard_normal((1, C, H, W)) * np.exp(rng.uniform(-6, 1, (1, C, 1, 1)))).astype(np.float32)
    x[0, 0, :4] *= 1e-6                          # values whose bf16 terms reach far down the exponent range
    return x


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


def check_outputs(c, what, now, before, idx, y, mag, add, relu):
    """now / before: [K, HW] after / in front of the launch; add: what joins the sum ([N, K] or None): the bias or, in
    accumulate mode, the output in front of the launch."""
    want = y + (add if add is not None else 0.0)
    if relu:
        want = np.maximum(want, 0.0)
    bound = mag + (np.abs(add) if add is not None else 0.0)
    err = np.abs(now[:, idx].T.astype(np.float64) - want)
    ratio = float((err / (bound + 1e-300)).max()) if len(idx) else 0.0
    print("%s: %d listed, max |err| %.3g, worst err / bound sum %.3g (2^%.1f)" % (
        what, len(idx), err.max() if len(idx) else 0.0, ratio, np.log2(ratio + 1e-300)))
    key = (c.kernel,) + tuple(c.cell[1:])
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    assert np.all(np.isfinite(now[:, idx])), what
    assert np.all(err <= FP32_TOL), (what, float(err.max()))
    assert np.all(err <= BOUND * bound + 1e-300), (what, ratio)
    rest = np.ones(now.shape[1], bool)
    rest[idx] = False
    assert np.array_equal(now[:, rest].view(np.int32), before[:, rest].view(np.int32)), \
        what + ": a pixel off the mask changed"


class Seq(object):
    """The device buffers of one sequence."""

    def __init__(self, state, mask, out0, relu0=None):
        H, W = mask.shape
        words = H * ((W + 63) // 64)
        self.state, self.out = dev(state), dev(out0)
        self.bits = dev(pack(mask).view(np.int64))
        self.arrive = torch.zeros(words, dtype=torch.int32, device="cuda")
        self.copy = torch.full((words,), -1, dtype=torch.int64, device="cuda")
        self.relu = dev(relu0) if relu0 is not None else None
        self.next = None


class Next(object):
    """The next layer's detection state behind the 2x2 pool of a fold case: f32 state, pre-split copy, frame mask, flag."""

    def __init__(self, lib, planes, H2, W2, k2, state2):
        C_ = lib.C
        self.planes, self.H2, self.W2, self.k2 = planes, H2, W2, k2
        self.state0 = state2
        self.state = dev(state2)
        self.flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.S = self.split_copy(lib, self.state)
        self.mask = torch.zeros(C_.cbinfer_frame_mask_bytes(H2, W2) // 8, dtype=torch.int64, device="cuda")

    def split_copy(self, lib, state):
        C_, K, H2, W2, k2 = lib.C, 16, self.H2, self.W2, self.k2
        if self.planes == 3:
            S = torch.empty(C_.cbinfer_split3_state_bytes(K, H2, W2, k2, k2), dtype=torch.uint8, device="cuda")
            lib.check(C_.cbinfer_split3_state_init(S.data_ptr(), K, H2, W2, k2, k2, None))
            lib.check(C_.cbinfer_split3_state_rebuild(state.data_ptr(), S.data_ptr(), K, H2, W2, k2, k2, None))
        else:
            S = torch.empty(C_.cbinfer_split_state_bytes(K, H2, W2, k2, k2), dtype=torch.uint8, device="cuda")
            lib.check(C_.cbinfer_split_state_init(S.data_ptr(), K, H2, W2, k2, k2, None))
            lib.check(C_.cbinfer_split_state_rebuild(state.data_ptr(), S.data_ptr(), K, H2, W2, k2, k2,
                                                     self.flag.data_ptr(), None))
        return S


def next_size(c):
    o, m = dict(c.opt), mc.case_map(c)
    return ((m.H + 1) // 2, (m.W + 1) // 2) if o["ceil"] else (m.H // 2, m.W // 2)


def pool2(out, H2, W2):
    """2x2 / stride 2 max of [K, H, W] at H2 x W2 pooled pixels; a window cut by the map's edge repeats its last row or
    column (cx1 / r1 of the kernel)."""
    K, H, W = out.shape
    r0, c0 = 2 * np.arange(H2), 2 * np.arange(W2)
    r1, c1 = np.minimum(r0 + 1, H - 1), np.minimum(c0 + 1, W - 1)
    return np.maximum(np.maximum(out[:, r0][:, :, c0], out[:, r0][:, :, c1]),
                      np.maximum(out[:, r1][:, :, c0], out[:, r1][:, :, c1]))


def next_descr(lib, c, nx):
    o = dict(c.opt)
    nd = lib.NextDetect()
    if nx is not None:
        nd.state, nd.splitState, nd.frameMasks = nx.state.data_ptr(), nx.S.data_ptr(), nx.mask.data_ptr()
        nd.rangeFlag = nx.flag.data_ptr()
    nd.H, nd.W = next_size(c)
    nd.kH = nd.kW = o["k2"]
    nd.threshold, nd.arith = mc.NEXT_TH, 1 if c.mode == "fold3" else 0
    return nd


def make_next(lib, rng, c, mask, final_ref):
    """A next-layer state around the pooled EXPECTED outputs: half of the pooled pixels within 0.3 th of them (quiet), half
    up to 3 th off (loud) -- so that listed windows change and do not, and loud windows without a listed pixel stay."""
    o = dict(c.opt)
    H2, W2 = next_size(c)
    pooled = pool2(final_ref, H2, W2)
    amp = np.where(rng.random((1, H2, W2)) < 0.5, 0.3, 3.0) * mc.NEXT_TH
    state2 = (pooled + rng.uniform(-1, 1, pooled.shape) * amp).astype(np.float32)[None]
    return Next(lib, 3 if c.mode == "fold3" else 2, H2, W2, o["k2"], state2)


def check_fold(lib, c, what, s, mask, got):
    """The numpy restatement of the next layer's detection on the GPU's own outputs `got` [K, H, W]."""
    nx = s.next
    H2, W2, k2 = nx.H2, nx.W2, nx.k2
    th = np.float32(mc.NEXT_TH)
    pooled = pool2(got, H2, W2)
    touched = pool2(mask[None].astype(np.float32), H2, W2)[0] > 0
    old = nx.state0[0]
    diff = np.abs(old - pooled)                                  # float32, as fabsf(state - pooled)
    assert diff.dtype == np.float32
    chg = touched & (diff > th).any(axis=0)
    want = np.where(chg[None], pooled, old)
    now = nx.state.cpu().numpy()[0]
    print("%s: fold, %d pooled pixels touched, %d changed, %d loud but untouched" % (
        what, touched.sum(), chg.sum(), (~touched & (diff > th).any(axis=0)).sum()))
    assert np.array_equal(now.view(np.int32), want.view(np.int32)), what + ": the next layer's state"
    words2 = H2 * ((W2 + 63) // 64)
    mw = nx.mask.cpu().numpy()
    assert np.array_equal(unpack_mask(mw[:words2], H2, W2), mc.dilate(chg, k2, k2)), what + ": the next layer's frame mask"
    assert not mw[words2:].any(), what
    over = nx.planes == 2 and bool((np.abs(pooled * np.float32(0.0625)) > np.float32(65504.0))[:, chg].any())
    assert int(nx.flag.item()) == int(over), what
    fresh = nx.split_copy(lib, dev(want[None]))
    assert torch.equal(nx.S, fresh), what + ": the next layer's pre-split copy"
    return int(chg.sum()), int((touched & ~chg).sum())


def vpp(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def prep_weights(lib, c, w):
    C_ = lib.C
    size, fn = ((C_.cbinfer_blockconv_prepared_bytes, C_.cbinfer_blockconv_prep_weights) if c.kernel == "blocks" else
                (C_.cbinfer_rowconv_prepared_bytes, C_.cbinfer_rowconv_prep_weights))
    wq = torch.empty(size(c.C, c.K, c.kH, c.kW), dtype=torch.uint8, device="cuda")
    lib.check(fn(dev(w).data_ptr(), wq.data_ptr(), c.K, c.C, c.kH, c.kW, None))
    return wq


def launch(lib, c, H, W, wq, seqs, bias, relu, batched=False):
    C_ = lib.C
    C, K, kH, kW = c.C, c.K, c.kH, c.kW
    s = seqs[0]
    bp = bias.data_ptr() if bias is not None else None
    if c.kernel == "rows" and c.mode == "acc":
        st = C_.cbinfer_conv_accumulate_rows(s.state.data_ptr(), s.bits.data_ptr(), s.arrive.data_ptr(), s.copy.data_ptr(),
                                             wq.data_ptr(), s.out.data_ptr(), s.relu.data_ptr() if s.relu is not None else None,
                                             C, H, W, K, kH, kW, None)
    elif c.kernel == "rows" and c.mode == "batched":
        st = C_.cbinfer_conv_changed_rows_batched(vpp([q.state for q in seqs]), vpp([q.bits for q in seqs]),
                                                  vpp([q.arrive for q in seqs]), vpp([q.copy for q in seqs]),
                                                  vpp([q.out for q in seqs]), len(seqs), wq.data_ptr(), bp, C, H, W, K, kH,
                                                  kW, int(relu), None)
    elif c.kernel == "rows":
        st = C_.cbinfer_conv_changed_rows(s.state.data_ptr(), s.bits.data_ptr(), s.arrive.data_ptr(), s.copy.data_ptr(),
                                          wq.data_ptr(), bp, s.out.data_ptr(), C, H, W, K, kH, kW, int(relu), None)
    elif c.kernel == "blocks" and c.mode in ("acc", "sparse"):
        st = C_.cbinfer_conv_accumulate_blocks(s.state.data_ptr(), s.bits.data_ptr(), s.arrive.data_ptr(),
                                               s.copy.data_ptr(), wq.data_ptr(), s.out.data_ptr(),
                                               s.relu.data_ptr() if s.relu is not None else None, C, H, W, K, kH, kW, None)
    elif c.kernel == "blocks":
        st = C_.cbinfer_conv_changed_blocks(s.state.data_ptr(), s.bits.data_ptr(), s.arrive.data_ptr(), s.copy.data_ptr(),
                                            wq.data_ptr(), bp, s.out.data_ptr(), C, H, W, K, kH, kW, int(relu), None)
    elif not batched:
        nd = next_descr(lib, c, s.next) if s.next is not None else None
        st = C_.cbinfer_conv_changed_rowpairs(s.state.data_ptr(), s.bits.data_ptr(), s.arrive.data_ptr(), s.copy.data_ptr(),
                                              wq.data_ptr(), bp, s.out.data_ptr(), C, H, W, K, kH, kW, int(relu),
                                              ctypes.pointer(nd) if nd is not None else None, None)
    else:
        tab = (lib.PairSeq * len(seqs))()
        for q, sq in enumerate(seqs):
            tab[q].state, tab[q].output = sq.state.data_ptr(), sq.out.data_ptr()
            tab[q].bits, tab[q].maskCopy = sq.bits.data_ptr(), sq.copy.data_ptr()
            if sq.next is not None:
                tab[q].nextState, tab[q].nextSplitState = sq.next.state.data_ptr(), sq.next.S.data_ptr()
                tab[q].nextFrameMasks, tab[q].nextRangeFlag = sq.next.mask.data_ptr(), sq.next.flag.data_ptr()
        nd = next_descr(lib, c, None) if seqs[0].next is not None else None
        st = C_.cbinfer_conv_changed_rowpairs_batched(tab, len(seqs), wq.data_ptr(), bp, C, H, W, K, kH, kW, int(relu),
                                                      ctypes.pointer(nd) if nd is not None else None, None)
    lib.check(st)
    torch.cuda.synchronize()


class Data(object):
    """The operands of a case and its float64 reference, computed once and shared by its configurations."""

    def __init__(self, oracle, c, rng, masks):
        m = mc.case_map(c)
        self.H, self.W = m.H, m.W
        self.w, self.b = make_weights(rng, c)
        self.acc = c.mode in ("acc", "sparse")
        self.masks = masks
        self.states, self.out0, self.relu0, self.idx, self.ref = [], [], [], [], []
        for q, mask in enumerate(masks):
            x = make_state(rng, c.C, m.H, m.W)
            if c.mode == "sparse":
                x = np.where(mc.sparse_support(c)[None], x, np.float32(0))
            self.states.append(x)
            shape = (1, c.K, m.H, m.W)
            if self.acc:       # (the output in front spans many binades, so that it does not hide the products)
                self.out0.append((rng.standard_normal(shape) * np.exp(rng.uniform(-12, 0, shape))).astype(np.float32))
            else:
                self.out0.append(rng.standard_normal(shape).astype(np.float32))
            self.relu0.append(np.full(shape, RELU_FILL, np.float32) if dict(c.opt).get("relu_out") else None)
            idx = np.flatnonzero(mask.reshape(-1)).astype(np.int32)
            self.idx.append(idx)
            self.ref.append(reference(oracle, x, idx, self.w))

    def final(self, c, q, bias, relu):
        """The expected [K, H, W] outputs of sequence q after the launch (float64 math rounded to f32)."""
        y = self.ref[q][0] + (self.b.astype(np.float64)[None] if bias else 0.0)
        if relu:
            y = np.maximum(y, 0.0)
        f = self.out0[q][0].reshape(c.K, -1).copy()
        f[:, self.idx[q]] = y.T.astype(np.float32)
        return f.reshape(c.K, self.H, self.W)


def run_config(lib, c, d, wq, bias, relu, masks=None, check=True, fold_rng=None, batched=False):
    """One launch of the case with bias or ReLU (accumulate modes: neither) on fresh buffers, with every check of the
    module's docstring; masks: other listed pixels than the case's (a subset: then only the protocol is checked).
    Returns the outputs [sequence] -> numpy [K, HW]."""
    H, W, K = d.H, d.W, c.K
    own = masks is None
    masks = d.masks if own else masks
    seqs = [Seq(d.states[q], masks[q], d.out0[q], d.relu0[q]) for q in range(len(masks))]
    if fold_rng is not None:
        for q, s in enumerate(seqs):
            s.next = make_next(lib, fold_rng, c, masks[q], d.final(c, q, bias, relu))
    bias_t = None
    if not d.acc:
        # (the row-segment and block launchers insist on a bias vector: zeros stand for none; the row pair takes NULL)
        bias_t = dev(d.b) if bias else (None if c.kernel == "pair" else torch.zeros(K, device="cuda"))
    launch(lib, c, H, W, wq, seqs, bias_t, relu, batched)
    outs = []
    changed = quiet = 0
    for q, s in enumerate(seqs):
        what = "%s seq %d bias %d relu %d" % (c.id, q, bias, relu)
        now = s.out.cpu().numpy().reshape(K, -1)
        before = d.out0[q].reshape(K, -1)
        idx = np.flatnonzero(masks[q].reshape(-1)).astype(np.int32)
        if check and own:
            y, mag = d.ref[q]
            add = before[:, idx].T.astype(np.float64) if d.acc else (d.b.astype(np.float64)[None] if bias else None)
            check_outputs(c, what, now, before, idx, y, mag, add, relu)
        else:
            rest = np.ones(H * W, bool)
            rest[idx] = False
            assert np.array_equal(now[:, rest].view(np.int32), before[:, rest].view(np.int32)), what
        assert np.array_equal(s.copy.cpu().numpy(), pack(masks[q]).view(np.int64)), what + ": the mask copy"
        assert int(s.bits.abs().sum().item()) == 0 and int(s.arrive.abs().sum().item()) == 0, what
        if s.relu is not None:
            r = s.relu.cpu().numpy().reshape(K, -1)
            want = np.where(now[:, idx] <= 0, np.float32(0), now[:, idx])      # (max(out, 0); -0 stores +0)
            assert np.array_equal(r[:, idx].view(np.int32), want.view(np.int32)), what
            rest = np.ones(H * W, bool)
            rest[idx] = False
            assert np.all(r[:, rest] == RELU_FILL), what
        if s.next is not None:
            a, b = check_fold(lib, c, what, s, masks[q], now.reshape(K, H, W))
            changed, quiet = changed + a, quiet + b
        outs.append(now)
    if fold_rng is not None and own and check:
        assert changed > 0 and quiet > 0, (c.id, changed, quiet)
    # a second launch on the emptied mask changes nothing
    keep = [(s.next.state.clone(), s.next.S.clone(), s.next.mask.clone()) if s.next is not None else None for s in seqs]
    launch(lib, c, H, W, wq, seqs, bias_t, relu, batched)
    for q, s in enumerate(seqs):
        assert np.array_equal(s.out.cpu().numpy().reshape(K, -1).view(np.int32), outs[q].view(np.int32)), (c.id, q)
        assert int(s.copy.abs().sum().item()) == 0 and int(s.bits.abs().sum().item()) == 0, (c.id, q)
        if keep[q] is not None:
            assert all(torch.equal(a, b) for a, b in zip(keep[q], (s.next.state, s.next.S, s.next.mask))), (c.id, q)
    return outs


def case_rng(c):
    return np.random.default_rng(zlib.crc32(c.id.encode()))


def same_bits(a, b, idx):
    return np.array_equal(a[:, idx].view(np.int32), b[:, idx].view(np.int32))


@pytest.mark.parametrize("cid", PLAIN_IDS)
def test_rows_and_blocks_against_float64(lib, oracle, cid):
    """cbinfer_conv_changed_rows[_batched] / _blocks and cbinfer_conv_accumulate_rows / _blocks.  The sparse block cases
    run on a delta with one or two non-zero values per patch: in a dense sum a dropped cross term of the bf16 triples
    hides behind sum|a||b| of hundreds of products; here the sum is one or two."""
    c = CASE_BY_ID[cid]
    assert_claimed_cell(c)
    rng = case_rng(c)
    d = Data(oracle, c, rng, mc.case_masks(c))
    wq = prep_weights(lib, c, d.w)
    if c.mode == "sparse":
        X = oracle.genXMatrix(d.states[0], d.idx[0], (c.kH, c.kW))
        per = (X != 0).sum(axis=1)
        print("%s: %.2f non-zero values per patch (max %d)" % (cid, per.mean(), per.max()))
        assert per.min() >= 1 and per.mean() <= 2
    configs = [(False, False)] if d.acc else [(True, False), (False, True)]
    first = None
    for bias, relu in configs:
        outs = run_config(lib, c, d, wq, bias, relu)
        first = first if first is not None else outs
    bias, relu = configs[0]
    if c.kernel == "rows":
        again = run_config(lib, c, d, wq, bias, relu)
        for q in range(c.nSeq):
            assert np.array_equal(again[q].view(np.int32), first[q].view(np.int32)), (cid, q)
    else:
        sub = [mc.subset(m, cid) for m in d.masks]
        part = run_config(lib, c, d, wq, bias, relu, masks=sub)
        for q in range(c.nSeq):
            idx = np.flatnonzero(sub[q].reshape(-1))
            assert len(idx) and same_bits(part[q], first[q], idx), (cid, q)
    RAN.add(cid)


@pytest.mark.parametrize("cid", PAIR_IDS)
def test_rowpairs_against_float64(lib, oracle, cid):
    """cbinfer_conv_changed_rowpairs, plain and with the next layer's pooled detection folded in."""
    c = CASE_BY_ID[cid]
    assert_claimed_cell(c)
    rng = case_rng(c)
    d = Data(oracle, c, rng, mc.case_masks(c))
    wq = prep_weights(lib, c, d.w)
    fold = c.mode != "plain"
    first = run_config(lib, c, d, wq, True, False, fold_rng=rng if fold else None)
    run_config(lib, c, d, wq, False, True, fold_rng=rng if fold else None)
    sub = [mc.subset(m, cid) for m in d.masks]
    if sub[0].any():
        part = run_config(lib, c, d, wq, True, False, masks=sub, fold_rng=rng if fold else None)
        idx = np.flatnonzero(sub[0].reshape(-1))
        assert same_bits(part[0], first[0], idx), cid
    RAN.add(cid)


@pytest.mark.parametrize("cid", DET_IDS)
def test_rowpairs_with_their_own_detection_against_float64(lib, oracle, cid):
    """cbinfer_conv_rowpairs_detect: the mask copy is the numpy dilation of any_c |state - frame| > th, the outputs are
    pinned on the REFRESHED values, the state itself is left alone, and everything the launch writes equals, bit for
    bit, what the plain instance writes when it is fed that mask and the refreshed state."""
    c = CASE_BY_ID[cid]
    assert_claimed_cell(c)
    C_ = lib.C
    m = mc.case_map(c)
    H, W, K, C = m.H, m.W, c.K, c.C
    rng = case_rng(c)
    th = np.float32(mc.DET_TH)
    state0 = make_state(rng, C, H, W)
    ch = mc.det_changed(c)
    frame = (state0 + rng.uniform(-0.03, 0.03, state0.shape)).astype(np.float32)
    jump = np.where(rng.random((H, W)) < 0.5, -1.0, 1.0) * (0.5 + np.abs(rng.standard_normal((H, W))))
    cc = rng.integers(0, C, (H, W))
    for ci in range(C):
        frame[0, ci] += np.where(ch & (cc == ci), jump, 0.0).astype(np.float32)
    changed = (np.abs(state0 - frame) > th).any(axis=1)[0]
    assert np.array_equal(changed, ch)
    mask = mc.dilate(changed, c.kH, c.kW)
    assert np.array_equal(mask, mc.case_masks(c)[0])
    refreshed = np.where(changed[None, None], frame, state0).astype(np.float32)
    d = Data(oracle, c, rng, [mask])
    d.states = [refreshed]
    d.ref = [reference(oracle, refreshed, d.idx[0], d.w)]
    wq = prep_weights(lib, c, d.w)
    fold = c.mode != "plain"
    for bias, relu in ((True, False), (False, True)):
        what = "%s bias %d relu %d" % (cid, bias, relu)
        frng = np.random.default_rng(zlib.crc32(what.encode()))
        s = Seq(state0, np.zeros_like(mask), d.out0[0])
        if fold:
            s.next = make_next(lib, frng, c, mask, d.final(c, 0, bias, relu))
        nd = next_descr(lib, c, s.next) if fold else None
        bias_t = dev(d.b) if bias else None
        fd = dev(frame)
        lib.check(C_.cbinfer_conv_rowpairs_detect(fd.data_ptr(), s.state.data_ptr(), s.out.data_ptr(), s.copy.data_ptr(),
                                                  wq.data_ptr(), bias_t.data_ptr() if bias else None, C, H, W, K, c.kH,
                                                  c.kW, float(th), int(relu), ctypes.pointer(nd) if fold else None, None))
        torch.cuda.synchronize()
        now = s.out.cpu().numpy().reshape(K, -1)
        y, mag = d.ref[0]
        check_outputs(c, what, now, d.out0[0].reshape(K, -1), d.idx[0], y, mag,
                      d.b.astype(np.float64)[None] if bias else None, relu)
        assert np.array_equal(s.copy.cpu().numpy(), pack(mask).view(np.int64)), what + ": the mask copy"
        assert np.array_equal(s.state.cpu().numpy(), state0), what + ": the state is refreshed by a later launch"
        if fold:
            a, b = check_fold(lib, c, what, s, mask, now.reshape(K, H, W))
            assert a > 0 and b > 0, (what, a, b)
        # the plain instance fed the same mask and the refreshed state
        p = Seq(refreshed, mask, d.out0[0])
        if fold:
            p.next = make_next(lib, np.random.default_rng(zlib.crc32(what.encode())), c, mask, d.final(c, 0, bias, relu))
        launch(lib, c, H, W, wq, [p], bias_t, relu)
        assert torch.equal(p.out, s.out), what
        if fold:
            assert torch.equal(p.next.state, s.next.state) and torch.equal(p.next.S, s.next.S), what
            assert torch.equal(p.next.mask, s.next.mask) and torch.equal(p.next.flag, s.next.flag), what
    RAN.add(cid)


@pytest.mark.parametrize("cid", SLOT_IDS)
def test_rowpair_candidate_slots_against_float64(lib, oracle, cid):
    """Grids whose workgroups take more than one candidate unit (beyond 8 units per CU), through the batched entry
    point: every non-empty unit pinned against float64 as everywhere, and bit-identical to a single-sequence launch of a
    few rows around it, where it is a slot-0 unit of sequence 0."""
    c = CASE_BY_ID[cid]
    assert_claimed_cell(c)
    m = mc.case_map(c)
    H, W, K = m.H, m.W, c.K
    f = mc.pair_form(c.C, c.K, c.kH, H, W, c.nSeq, cus())
    rng = case_rng(c)
    d = Data(oracle, c, rng, mc.case_masks(c))
    wq = prep_weights(lib, c, d.w)
    fold = c.mode != "plain"
    first = run_config(lib, c, d, wq, True, False, fold_rng=rng if fold else None, batched=True)
    run_config(lib, c, d, wq, False, True, fold_rng=rng if fold else None, batched=True)
    plain = c._replace(mode="plain")
    done = set()
    for u in sorted(mc.slot_units(c, cus())):
        q, ul = divmod(u, f["units"])
        yo = ul // f["wpr"]
        r0, r1 = max(0, 2 * yo - 8), min(H, 2 * yo + 10)
        if (q, r0) in done:
            continue
        done.add((q, r0))
        s = Seq(d.states[q][:, :, r0:r1], d.masks[q][r0:r1], d.out0[q][:, :, r0:r1])
        launch(lib, plain, r1 - r0, W, wq, [s], dev(d.b), False)
        crop = s.out.cpu().numpy()[0]
        rows = slice(2 * yo - r0, min(2 * yo + 2, H) - r0)
        full = first[q].reshape(K, H, W)[:, 2 * yo:min(2 * yo + 2, H)]
        assert d.masks[q][2 * yo:2 * yo + 2].any()
        assert np.array_equal(crop[:, rows].view(np.int32), full.view(np.int32)), (cid, u, q, yo, u // f["grid"])
    assert len(done) >= 4
    RAN.add(cid)


def test_zz_report_worst_ratios(capsys):
    """Not a check of the kernels: prints the worst ratio per kernel and cell seen by the tests above, and fails if a case
    of the table did not run."""
    with capsys.disabled():
        print("\nworst |err| / bound sum per kernel and cell (the bar: 2^-18):")
        for key, r in sorted(WORST.items()):
            print("  %-60s %.3g (2^%.1f)" % (" ".join(key), r, np.log2(r + 1e-300)))
        for kernel in ("rows", "blocks", "pair"):
            rs = [r for k, r in WORST.items() if k[0] == kernel]
            if rs:
                print("  %-60s %.3g (2^%.1f)" % (kernel + " (all cells)", max(rs), np.log2(max(rs) + 1e-300)))
    missing = [c.id for c in CASES if c.id not in RAN]
    assert not missing, "cases of the table that did not run to their end: %s" % missing
