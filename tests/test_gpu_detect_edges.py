"""-m gpu tests of the change detections at the edges of mask words and of the map, where the word dilation they share
(cb_dilate_word / cb_or_dilated_rows, the producer-mask shortcut and the clamped pooled load of cb_common.h) can go wrong
and the random masks of the other tests rarely look: a 5-row map of 64, 65 and 130 columns -- one exact word; a second
word with one valid bit; three words, two valid bits in the last --, a 7x7 filter and one whose horizontal half width
is 0 (the dilation loop runs zero times), ONE pixel changed per frame at the columns 0, 2, 61, 63, 64, 66, W-1 of the
first and the last row.

Every call site of the shared parts, through the library entry point that reaches it: the plain detection (fp32 / fp16,
bit mask / byte map, 3 and 16 channels), the fine-grained frame detection, cbinfer_split_detect (f16 pairs / bf16 triples,
pooled or not), the fp16 group's detection (pooled or not), the row-pair launch's folded detection of the layer behind
the pool and the window-order contraction's.  Each walk starts from a constant state; frame mask and refreshed state are
compared bit for bit with the CPU oracle (changeDetection / changeDetection_half on a 1x1 support, then
changePropagation) after every frame.

The split-state layers take no 1x1 filter (fewer than four k-stages): their zero-width dilation is a 7x1 filter.  The
pooled forms read an odd pool input (2H-1 x 2W-1: the last window of every row and column is clamped) and are handed a
producer mask with a single word set -- a second changed pixel under words that are not set must stay unseen."""
import ctypes

import numpy as np
import pytest
import torch
from optest import dev, gpu_lib as lib, raw      # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

H = 5
WIDTHS = (64, 65, 130)
TH, BASE, SPIKE = 0.1, 0.25, 1.0      # (all exact in f16)


def pixels(W):
    cols = sorted({c for c in (0, 2, 61, 63, 64, 66, W - 1) if c < W})
    return [(y, x) for y in (0, H - 1) for x in cols]


def expect(oracle, inp, state, filt, th=TH):
    """(raw change map, dilated map, refreshed state) of one feedback-mode detection, by the oracle."""
    st = state.copy()
    if inp.dtype == np.float16:
        raw = oracle.changeDetection_half(inp, st, (1, 1), th, updateInputState=True)
    else:
        raw = oracle.changeDetection(inp, st, (1, 1), th, updateInputState=True)
    return raw, oracle.changePropagation(raw, filt), st


def mask_bits(words, Hm, Wm):
    wpr = (Wm + 63) // 64
    w = words.cpu().numpy().view(np.uint64)[:Hm * wpr]
    return np.unpackbits(w.view(np.uint8), bitorder="little").reshape(Hm, wpr * 64)


def check_mask(words, want, Hm, Wm, tag):
    bits = mask_bits(words, Hm, Wm)
    assert np.array_equal(bits[:, :Wm].astype(np.int8), want), tag
    assert not bits[:, Wm:].any(), tag      # (nothing beyond the row's last pixel)


def pool2(x):
    """2x2 / stride-2 max pool, ceil mode (windows clipped at the border)."""
    n, c, h, w = x.shape
    p = np.full((n, c, h + (h & 1), w + (w & 1)), -np.inf, dtype=x.dtype)
    p[:, :, :h, :w] = x
    return p.reshape(n, c, p.shape[2] // 2, 2, p.shape[3] // 2, 2).max(axis=(3, 5))


class PooledWalk(object):
    """The frames of a pooled detection's walk: the pool's input [1,C,2H-1,2W-1], one more pooled pixel raised per frame,
    a decoy raised in the map's middle row under producer-mask words that stay zero, and the producer mask with the one
    word set that covers the raised pixel.  `seen(pooled, state)`: the pooled frame as the detection may look at it --
    segments none of whose 2x2 producer words is set keep the state's values."""

    def __init__(self, C, W, dtype):
        self.C, self.W, self.pH, self.pW = C, W, 2 * H - 1, 2 * W - 1
        self.pwpr = (self.pW + 63) // 64
        self.x = np.full((1, C, self.pH, self.pW), BASE, dtype=dtype)

    def step(self, i, y, x):
        self.x = self.x.copy()
        self.x[0, i % self.C, 2 * y, 2 * x] += SPIKE
        self.x[0, i % self.C, 2 * (H // 2), 2 * x] += SPIKE      # the decoy: pooled row 2, producer rows 4 and 5
        self.prod = np.zeros((self.pH, self.pwpr), dtype=np.uint64)
        self.prod[2 * y, (2 * x) >> 6] = np.uint64(1) << np.uint64((2 * x) & 63)
        return self.x, self.prod

    def seen(self, state):
        pooled = pool2(self.x)
        out = state.copy()
        for y in range(H):
            for tx in range((self.W + 63) // 64):
                if self.prod[2 * y:2 * y + 2, 2 * tx:2 * tx + 2].any():
                    out[..., y, tx * 64:(tx + 1) * 64] = pooled[..., y, tx * 64:(tx + 1) * 64]
        return out


# ---------------------------------------------------------------------------------------------------------------------
# cb_detect.hip
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["bits", "map"])
@pytest.mark.parametrize("C", [3, 16])
@pytest.mark.parametrize("dtype", [np.float32, np.float16])
@pytest.mark.parametrize("filt", [(7, 7), (1, 1)])
@pytest.mark.parametrize("W", WIDTHS)
def test_plain_detection(lib, oracle, W, filt, dtype, C, form):
    C_ = lib.C
    code = 0 if dtype == np.float32 else 1
    x = np.full((1, C, H, W), BASE, dtype=dtype)
    st_o, st_g = x.copy(), dev(x)
    words = torch.zeros(C_.cbinfer_mask_words(H, W), dtype=torch.int64, device="cuda")
    cmap = torch.zeros((H, W), dtype=torch.int8, device="cuda")
    for i, (y, px) in enumerate(pixels(W)):
        x = x.copy()
        x[0, i % C, y, px] += SPIKE
        raw, want, st_o = expect(oracle, x, st_o, filt)
        assert raw.sum() == 1 and raw[y, px]
        xd = dev(x)
        if form == "bits":
            words.zero_()
            lib.check(C_.cbinfer_change_detection_bits(xd.data_ptr(), st_g.data_ptr(), words.data_ptr(), W, H, C,
                                                       filt[0] // 2, filt[1] // 2, TH, 1, code, None))
            check_mask(words, want, H, W, (y, px))
        else:
            lib.check(C_.cbinfer_change_detection(xd.data_ptr(), st_g.data_ptr(), cmap.data_ptr(), W, H, C,
                                                  filt[0] // 2, filt[1] // 2, TH, 1, code, None))
            assert np.array_equal(cmap.cpu().numpy(), want), (y, px)
        assert np.array_equal(st_g.cpu().numpy(), st_o), (y, px)


@pytest.mark.parametrize("C", [3, 16])
@pytest.mark.parametrize("dtype", [np.float32, np.float16])
@pytest.mark.parametrize("filt", [(7, 7), (1, 1)])
@pytest.mark.parametrize("W", WIDTHS)
def test_plain_detection_pooled(lib, oracle, W, filt, dtype, C):
    C_ = lib.C
    code = 0 if dtype == np.float32 else 1
    walk = PooledWalk(C, W, dtype)
    st_o = np.full((1, C, H, W), BASE, dtype=dtype)
    st_g = dev(st_o)
    words = torch.zeros(C_.cbinfer_mask_words(H, W), dtype=torch.int64, device="cuda")
    for i, (y, px) in enumerate(pixels(W)):
        x, prod = walk.step(i, y, px)
        raw, want, st_o = expect(oracle, walk.seen(st_o), st_o, filt)
        assert raw.sum() == 1 and raw[y, px]
        words.zero_()
        xd, prodd = dev(x), dev(prod.view(np.int64))
        lib.check(C_.cbinfer_change_detection_bits_pooled(xd.data_ptr(), walk.pH, walk.pW, prodd.data_ptr(), st_g.data_ptr(),
                                                          words.data_ptr(), W, H, C, filt[0] // 2, filt[1] // 2, TH, code,
                                                          None))
        check_mask(words, want, H, W, (y, px))
        assert np.array_equal(st_g.cpu().numpy(), st_o), (y, px)


@pytest.mark.parametrize("filt", [(7, 7), (1, 1)])
@pytest.mark.parametrize("W", WIDTHS)
def test_fine_grained_frame_detection(lib, oracle, W, filt):
    C_, C = lib.C, 3
    x = np.full((1, C, H, W), BASE, dtype=np.float32)
    st_o, prev = x.copy(), dev(x)
    delta = torch.full((1, C, H, W), 7.0, device="cuda")
    masks = torch.zeros(C_.cbinfer_frame_mask_bytes(H, W) // 8, dtype=torch.int64, device="cuda")
    nw = C_.cbinfer_mask_words(H, W)
    for i, (y, px) in enumerate(pixels(W)):
        x = x.copy()
        x[0, i % C, y, px] += SPIKE
        d = x - st_o
        raw, want, st_o = expect(oracle, x, st_o, filt)
        assert raw.sum() == 1 and raw[y, px]
        masks[:nw].zero_()
        xd = dev(x)
        lib.check(C_.cbinfer_change_detection_fg_frame(xd.data_ptr(), prev.data_ptr(), delta.data_ptr(), masks.data_ptr(),
                                                       W, H, C, filt[0] // 2, filt[1] // 2, TH, 1, None))
        check_mask(masks, want, H, W, (y, px))
        assert np.array_equal(prev.cpu().numpy(), x), (y, px)
        assert np.array_equal(delta.cpu().numpy(), np.where(np.abs(d) > TH, d, 0).astype(np.float32)), (y, px)


# ---------------------------------------------------------------------------------------------------------------------
# cb_split.hip: cbinfer_split_detect, the fp16 group's detection
# ---------------------------------------------------------------------------------------------------------------------
def split_state(lib, state, C, Hs, Ws, kH, kW, x3, flag=None):
    """A fresh split copy (f16 pairs / bf16 triples) of an f32 state tensor."""
    C_ = lib.C
    a = (C, Hs, Ws, kH, kW)
    if x3:
        S = torch.empty(C_.cbinfer_split3_state_bytes(*a), dtype=torch.uint8, device="cuda")
        lib.check(C_.cbinfer_split3_state_init(S.data_ptr(), *a, None))
        lib.check(C_.cbinfer_split3_state_rebuild(state.data_ptr(), S.data_ptr(), *a, None))
    else:
        S = torch.empty(C_.cbinfer_split_state_bytes(*a), dtype=torch.uint8, device="cuda")
        lib.check(C_.cbinfer_split_state_init(S.data_ptr(), *a, None))
        lib.check(C_.cbinfer_split_state_rebuild(state.data_ptr(), S.data_ptr(), *a,
                                                 flag.data_ptr() if flag is not None else None, None))
    return S


@pytest.mark.parametrize("pooled", [False, True])
@pytest.mark.parametrize("x3", [True, False])
@pytest.mark.parametrize("filt", [(7, 7), (7, 1)])
@pytest.mark.parametrize("W", WIDTHS)
def test_split_detect(lib, oracle, W, filt, x3, pooled):
    C_, C = lib.C, 16
    kH, kW = filt
    assert C_.cbinfer_split_supported(C, 1, kH, kW) == 1
    walk = PooledWalk(C, W, np.float32)
    x = np.full((1, C, H, W), BASE, dtype=np.float32)
    st_o = x.copy()
    st_g = dev(st_o)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    S = split_state(lib, st_g, C, H, W, kH, kW, x3, flag)
    masks = torch.zeros(C_.cbinfer_frame_mask_bytes(H, W) // 8, dtype=torch.int64, device="cuda")
    nw = C_.cbinfer_mask_words(H, W)
    seq = (lib.SplitSeq * 1)()
    s = seq[0]
    s.state, s.splitState, s.frameMasks, s.rangeFlag = st_g.data_ptr(), S.data_ptr(), masks.data_ptr(), flag.data_ptr()
    for i, (y, px) in enumerate(pixels(W)):
        if pooled:
            xin, prod = walk.step(i, y, px)
            prodd = dev(prod.view(np.int64))
            s.producerMask = prodd.data_ptr()
            seen = walk.seen(st_o)
        else:
            x = x.copy()
            x[0, i % C, y, px] += SPIKE
            xin, seen, s.producerMask = x, x, None
        raw, want, st_o = expect(oracle, seen, st_o, filt)
        assert raw.sum() == 1 and raw[y, px]
        xd = dev(xin)
        s.input = xd.data_ptr()
        masks[:nw].zero_()      # (the contraction would)
        lib.check(C_.cbinfer_split_detect(seq, 1, int(pooled) | (8 if x3 else 0), walk.pH if pooled else 0,
                                          walk.pW if pooled else 0, C, H, W, kH, kW, TH, None))
        check_mask(masks, want, H, W, (y, px))
        assert np.array_equal(st_g.cpu().numpy(), st_o), (y, px)
    # the split copy took the same pixels: it is the split of the refreshed state
    assert torch.equal(S, split_state(lib, st_g, C, H, W, kH, kW, x3, flag))
    assert int(flag.item()) == 0


@pytest.mark.parametrize("pooled", [False, True])
@pytest.mark.parametrize("filt", [(7, 7), (1, 1)])
@pytest.mark.parametrize("W", WIDTHS)
def test_half_group_detection(lib, oracle, W, filt, pooled):
    """cbinfer_hsplit_forward_group, one 64 -> 64 layer in feedback mode that runs its own detection: the mask copy the
    launch leaves is the frame's dilated mask."""
    C_, C, K = lib.C, 64, 64
    kH, kW = filt
    a = (C, H, W, kH, kW)
    assert C_.cbinfer_hsplit_supported(C, K, kH, kW) == 1
    rng = np.random.default_rng(W)
    wgt = dev((rng.standard_normal((K, C, kH, kW)) / np.sqrt(C * kH * kW)).astype(np.float16))
    bias = dev(rng.standard_normal(K).astype(np.float16))
    wp = torch.empty(C_.cbinfer_hsplit_prepared_bytes(C, K, kH, kW), dtype=torch.uint8, device="cuda")
    lib.check(C_.cbinfer_hsplit_prep_weights(wgt.data_ptr(), wp.data_ptr(), K, C, kH, kW, H, W, None))
    walk = PooledWalk(C, W, np.float16)
    x = np.full((1, C, H, W), BASE, dtype=np.float16)
    st_o = x.copy()
    st_g = dev(st_o)

    def pixel_state():
        S = torch.empty(C_.cbinfer_hsplit_state_bytes(*a), dtype=torch.uint8, device="cuda")
        lib.check(C_.cbinfer_hsplit_state_init(S.data_ptr(), *a, None))
        lib.check(C_.cbinfer_hsplit_state_rebuild(st_g.data_ptr(), S.data_ptr(), *a, None))
        return S
    S = pixel_state()
    nw = C_.cbinfer_mask_words(H, W)
    masks = torch.zeros(C_.cbinfer_frame_mask_bytes(H, W) // 8, dtype=torch.int64, device="cuda")
    copy = torch.full((nw,), -1, dtype=torch.int64, device="cuda")
    out = torch.zeros((1, K, H, W), dtype=torch.float16, device="cuda")
    idx = torch.zeros(H * W, dtype=torch.int32, device="cuda")
    cnt = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    wsb = C_.cbinfer_hsplit_group_workspace_bytes(1, C, H, W, K, kH, kW)
    assert wsb == C_.cbinfer_hsplit_workspace_bytes(C, H, W, K, kH, kW) and (wsb > 0) == (kH * kW >= 48)
    ws = torch.zeros(wsb, dtype=torch.uint8, device="cuda") if wsb else None
    layer = (lib.HalfLayer * 1)()
    L = layer[0]
    L.state, L.pixelState, L.frameMasks, L.output = st_g.data_ptr(), S.data_ptr(), masks.data_ptr(), out.data_ptr()
    L.idxOut, L.countOut, L.maskCopy = idx.data_ptr(), cnt.data_ptr(), copy.data_ptr()
    L.prepared, L.bias = wp.data_ptr(), bias.data_ptr()
    L.K, L.threshold, L.relu, L.detect, L.nNext = K, TH, 0, 1, 0
    for i, (y, px) in enumerate(pixels(W)):
        if pooled:
            xin, prod = walk.step(i, y, px)
            prodd = dev(prod.view(np.int64))
            L.producerMask = prodd.data_ptr()
            seen = walk.seen(st_o)
        else:
            x = x.copy()
            x[0, i % C, y, px] += np.float16(SPIKE)
            xin, seen, L.producerMask = x, x, None
        raw, want, st_o = expect(oracle, seen, st_o, filt)
        assert raw.sum() == 1 and raw[y, px]
        xd = dev(xin)
        L.input = xd.data_ptr()
        lib.check(C_.cbinfer_hsplit_forward_group(layer, 1, int(pooled), walk.pH if pooled else 0, walk.pW if pooled else 0,
                                                  C, H, W, kH, kW, 1, ws.data_ptr() if ws is not None else None, None))
        check_mask(copy, want, H, W, (y, px))
        assert int(cnt.item()) == int(want.sum()), (y, px)
        assert np.array_equal(st_g.cpu().numpy(), st_o), (y, px)
    assert torch.equal(S, pixel_state())


# ---------------------------------------------------------------------------------------------------------------------
# the folded detections of the layer behind the 2x2 pool: row-pair launch, window-order contraction
# ---------------------------------------------------------------------------------------------------------------------
TH2 = 0.05


class Consumer(object):
    """State, split copy (bf16 triples) and frame mask of a 16-channel layer on the 5 x W2 map behind a ceil-mode pool."""

    def __init__(self, lib, W2, filt):
        C_ = lib.C
        self.W2, self.filt = W2, filt
        self.state = torch.full((1, 16, H, W2), float("inf"), device="cuda")
        self.S = split_state(lib, self.state, 16, H, W2, filt[0], filt[1], True)
        self.mask = torch.zeros(C_.cbinfer_frame_mask_bytes(H, W2) // 8, dtype=torch.int64, device="cuda")
        self.nd = nd = lib.NextDetect()
        nd.state, nd.splitState, nd.frameMasks = self.state.data_ptr(), self.S.data_ptr(), self.mask.data_ptr()
        nd.rangeFlag = None
        nd.H, nd.W, nd.kH, nd.kW, nd.threshold, nd.arith = H, W2, filt[0], filt[1], TH2, 1

    def check(self, lib, oracle, out, st_o, tag, pixel=None):
        """After a producer launch that left `out`: mask and state against the oracle's detection on the pooled outputs;
        returns the oracle's refreshed state."""
        raw, want, st_o = expect(oracle, pool2(out.cpu().numpy()), st_o, self.filt, TH2)
        if pixel is not None:
            assert raw.sum() == 1 and raw[pixel], tag
        check_mask(self.mask, want, H, self.W2, tag)
        assert np.array_equal(self.state.cpu().numpy(), st_o), tag
        self.mask.zero_()      # (the consumer's contraction would)
        return st_o


def centre_tap_weights(K, C, kH, kW):
    """Weights whose only non-zero tap is the centre one, positive: an output pixel depends on its own input pixel
    alone, and a raised input raises the output -- ONE pooled pixel of the consumer changes per raised input pixel."""
    rng = np.random.default_rng(K + C)
    w = np.zeros((K, C, kH, kW), dtype=np.float32)
    w[:, :, kH // 2, kW // 2] = rng.uniform(0.5, 1.0, (K, C)).astype(np.float32)
    return w, rng.standard_normal(K).astype(np.float32)


@pytest.mark.parametrize("filt2", [(7, 7), (7, 1)])
@pytest.mark.parametrize("W2", WIDTHS)
def test_rowpair_folded_detection(lib, oracle, W2, filt2):
    C_ = lib.C
    C, K, k, Hp, Wp = 3, 16, 3, 2 * H - 1, 2 * W2 - 1
    w, b = centre_tap_weights(K, C, k, k)
    wp = torch.empty(C_.cbinfer_rowconv_prepared_bytes(C, K, k, k), dtype=torch.uint8, device="cuda")
    lib.check(C_.cbinfer_rowconv_prep_weights(dev(w).data_ptr(), wp.data_ptr(), K, C, k, k, None))
    bd = dev(b)
    words = C_.cbinfer_mask_words(Hp, Wp)
    state = torch.full((1, C, Hp, Wp), float("inf"), device="cuda")
    out = torch.full((1, K, Hp, Wp), float("inf"), device="cuda")
    bits = torch.zeros(words, dtype=torch.int64, device="cuda")
    ctl = torch.zeros(words, dtype=torch.int32, device="cuda")
    copy = torch.zeros(words, dtype=torch.int64, device="cuda")
    cons = Consumer(lib, W2, filt2)
    st_o = cons.state.cpu().numpy()
    x = np.full((1, C, Hp, Wp), BASE, dtype=np.float32)
    for i, pix in enumerate([None] + pixels(W2)):      # (the first frame primes: every pixel is new to both layers)
        if pix is not None:
            x = x.copy()
            x[0, i % C, 2 * pix[0], 2 * pix[1]] += SPIKE
        xd = dev(x)
        lib.check(C_.cbinfer_cbconv2d_forward_rowpairs(xd.data_ptr(), state.data_ptr(), out.data_ptr(), bits.data_ptr(),
                                                       ctl.data_ptr(), copy.data_ptr(), wp.data_ptr(), bd.data_ptr(), C, Hp, Wp,
                                                       K, k, k, TH, 0, ctypes.pointer(cons.nd), None))
        st_o = cons.check(lib, oracle, out, st_o, pix, pix)
    assert torch.equal(cons.S, split_state(lib, cons.state, 16, H, W2, filt2[0], filt2[1], True))


@pytest.mark.parametrize("filt2", [(7, 7), (7, 1)])
@pytest.mark.parametrize("W2", WIDTHS)
def test_window_order_folded_detection(lib, oracle, W2, filt2):
    """cbinfer_split_conv_next: a 16 -> 16 producer (7x1 filter, bf16 triples) in window order on the 9 x (2 W2 - 1) map."""
    from test_gpu_front_half import Layer
    C_ = lib.C
    C, K, kH, kW, Hp, Wp = 16, 16, 7, 1, 2 * H - 1, 2 * W2 - 1
    w, b = centre_tap_weights(K, C, kH, kW)
    P = Layer(lib, w, b, Hp, Wp, "x3")
    cons = Consumer(lib, W2, filt2)
    assert C_.cbinfer_split_next_supported(C, K, kH, kW, Hp, Wp, ctypes.pointer(cons.nd)) == 1
    st_o = cons.state.cpu().numpy()
    x = np.full((1, C, Hp, Wp), BASE, dtype=np.float32)
    for i, pix in enumerate([None] + pixels(W2)):
        if pix is not None:
            x = x.copy()
            x[0, i % C, 2 * pix[0], 2 * pix[1]] += SPIKE
        xd = dev(x)
        P.detect([xd], TH)
        lib.check(C_.cbinfer_split_conv_next(P.seqs, 1, P.wp.data_ptr(), P.b.data_ptr(), C, Hp, Wp, K, kH, kW, 0.0, 0, None,
                                             ctypes.pointer(cons.nd), None))
        torch.cuda.synchronize()
        st_o = cons.check(lib, oracle, P.out[0], st_o, pix, pix)
    assert torch.equal(cons.S, split_state(lib, cons.state, 16, H, W2, filt2[0], filt2[1], True))
