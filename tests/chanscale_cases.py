"""The specification of the change-based channel attention scale (CBChannelScale2d, cb_chanscale.hip) as
a numpy float32 twin, the float64 references, the error bounds, and the shapes the host and GPU tests share.  The
reference project has no such operator, so the twin written here IS the specification:
  rule 1  s = (float)v, or the excitation s = W2 act(W1 z + b1) + b2 with every product and sum a float32 operation of
          its own and the sums in the order of chanreduce_cases.sum16 (excite() below); gate = g(s) in float32;
  rule 2  channel c trips iff `all` or not |gate[c] - held[c]| <= threshold (strictly more; a NaN trips); a tripped
          channel takes held[c] = gate[c], any other keeps held[c] bit for bit;
  rule 3  out[c, p] = (T)(float(a[c, p]) * held[c]) -- one float32 product, one rounding to T -- is written at a listed
          pixel for every channel and at every other pixel for the tripped channels; every other element keeps its bits;
  rule 4  the frame's mask is the listed pixels, or every pixel in a frame in which a channel tripped.
step() takes the frame's gate vector AS THE DEVICE WROTE IT: the device's expf differs from numpy's in the last bits,
and a trip decision must not depend on that.  No GPU is needed to import this file."""
import math

import numpy as np

import chanreduce_cases as cr
import pointwise_cases as pc

F32 = np.float32
GATES = [None, 'sigmoid', 'hardsigmoid']
ACTS = ['relu', 'silu']
# [C, H, W]: C below, at and just over one ballot word (64 channels) and many words; W on both sides of a mask-word
# boundary; the last has more mask words than the grid takes workgroups (8 per CU, 256 CUs)
SHAPES = [(1, 1, 9), (3, 5, 64), (64, 5, 9), (65, 1, 65), (300, 5, 130), (5, 2100, 9)]
# (C, R) of the fused excitation: R below, at and just over the 16 slices of sum16, and several times over them
EXCITE = [(3, 1), (3, 16), (65, 17), (65, 40), (300, 1), (300, 16), (300, 17), (300, 40)]
FORMS = pc.FORMS
pack, bits_of, same_bits = pc.pack, pc.bits_of, pc.same_bits


def _clamp(t, lo, hi):
    return np.where(t < lo, lo, np.where(t > hi, hi, t))


def gate_fn(s, gate):
    """g(s) in float32 by the formulas of the specification (numpy's exp for the sigmoid)."""
    assert s.dtype == F32
    with np.errstate(all='ignore'):
        if gate == 'sigmoid':
            g = F32(1) / (F32(1) + np.exp(-s))
        elif gate == 'hardsigmoid':
            g = _clamp(s + F32(3), F32(0), F32(6)) / F32(6)
        else:
            assert gate is None
            g = s
    assert g.dtype == F32
    return g


def gate64(s, gate):
    """g(s) in float64."""
    s = s.astype(np.float64)
    with np.errstate(all='ignore'):
        if gate == 'sigmoid':
            return 1.0 / (1.0 + np.exp(-s))
        if gate == 'hardsigmoid':
            return np.clip(s + 3.0, 0.0, 6.0) / 6.0
        return s


def _act(h, act):
    with np.errstate(all='ignore'):
        if act == 'relu':
            return np.where(h < 0, F32(0), h)
        assert act == 'silu'
        return h / (F32(1) + np.exp(-h))


def excite(z, W1, b1, W2, b2, act):
    """s [C] float32 of the pooled vector z [C] (float32 or float16): hidden = act(sum16_c(W1[r, c] z[c]) + b1[r]),
    s[c] = sum16_r(W2[c, r] hidden[r]) + b2[c]; W1 [R, C], W2 [C, R], b1 / b2 float32 or None (nothing is added)."""
    assert W1.dtype == F32 and W2.dtype == F32 and W1.shape == W2.shape[::-1]
    with np.errstate(all='ignore'):
        zf = z.astype(F32)
        h = cr.sum16(np.ascontiguousarray((W1 * zf[None, :]).T))        # [C, R] -> [R]
        if b1 is not None:
            assert b1.dtype == F32
            h = h + b1
        hidden = _act(h, act)
        s = cr.sum16(np.ascontiguousarray((W2 * hidden[None, :]).T))    # [R, C] -> [C]
        if b2 is not None:
            assert b2.dtype == F32
            s = s + b2
    assert s.dtype == F32
    return s


def excite64(z, W1, b1, W2, b2, act):
    """(s, h, hidden) in float64 on the stored operands."""
    z, W1, W2 = (t.astype(np.float64) for t in (z, W1, W2))
    h = W1 @ z + (b1.astype(np.float64) if b1 is not None else 0.0)
    with np.errstate(all='ignore'):
        hidden = np.maximum(h, 0.0) if act == 'relu' else h / (1.0 + np.exp(-h))
    s = W2 @ hidden + (b2.astype(np.float64) if b2 is not None else 0.0)
    return s, h, hidden


def excite_bound(z, W1, b1, W2, b2, act):
    """The error bound of the fused s against excite64(), per channel, built as chanreduce_cases.bound builds its own.
    u = 2^-24 is what one correctly rounded float32 operation adds relative to its result; a sum16 of n products spends
    K(n) = ceil(n / 16) + 5 roundings on a value (the product, ceil(n / 16) additions in its slice, four in the tree),
    each relative to a partial sum that the sum of the magnitudes bounds; the bias costs one more, relative to the
    result.  First order, taken twice:
      E(h[r])      = 2u (K(C) sum_c |W1[r, c] z[c]| + |h[r]|)
      E(hidden[r]) = E(h[r]) for the ReLU (exact, 1-Lipschitz);  1.1 E(h[r]) + 14u |hidden[r]| for the SiLU (its slope is
                     at most 1.0999; DESIGN 5.16 has the 14 units of v / (1 + expf(-v)))
      E(s[c])      = sum_r |W2[c, r]| E(hidden[r]) + 2u (K(R) sum_r |W2[c, r] hidden[r]| + |s[c]|)
    plus 2^-126 (a float32 result may be subnormal).  Worst err / bound seen on the MI355X over EXCITE, with and without
    biases, fp32 and fp16 (tests/test_gpu_chanscale.py): 0.085 with the ReLU, 0.087 with the SiLU."""
    u = 2.0 ** -24
    s, h, hidden = excite64(z, W1, b1, W2, b2, act)
    z64, W1a, W2a = z.astype(np.float64), np.abs(W1.astype(np.float64)), np.abs(W2.astype(np.float64))
    K1, K2 = math.ceil(W1.shape[1] / 16) + 5, math.ceil(W1.shape[0] / 16) + 5
    Eh = 2 * u * (K1 * (W1a @ np.abs(z64)) + np.abs(h))
    Ehid = Eh if act == 'relu' else 1.1 * Eh + 14 * u * np.abs(hidden)
    return W2a @ Ehid + 2 * u * (K2 * (W2a @ np.abs(hidden)) + np.abs(s)) + 2.0 ** -126


def gate_bound(ref, gate):
    """The bound of the device's gate against gate64() of the SAME float32 argument: the sigmoid's 14 units of DESIGN
    5.16 (expf at the OpenCL full profile's 3 ulp, taken twice: 12, entering 1 + e with a weight of at most 1, one for
    the addition, one for the division) plus 2^-126; the hard sigmoid and the identity are exact.  Worst err / bound
    seen on the MI355X: 0.127 (1.8 of the 14 units)."""
    if gate == 'sigmoid':
        return 14 * 2.0 ** -24 * np.abs(ref) + 2.0 ** -126
    return np.zeros_like(ref)


def product(a, held):
    """(T)(float(a) * held[c]) at every element of a [C, H, W]."""
    assert held.dtype == F32
    with np.errstate(all='ignore'):
        p = a.astype(F32) * held[:, None, None]
        assert p.dtype == F32
        return p.astype(a.dtype)


def step(a, gateNow, held, listed, threshold, all, prev=None):
    """One frame.  a [C, H, W] (float32 or float16), gateNow the frame's gates as the device wrote them, held the gates
    before the frame (both float32 [C]), listed bool [H, W] the operand's changed pixels (every pixel for an operand
    without change information), all: a fresh state.  Returns (held after the frame, tripped bool [C], out at EVERY
    element, mask bool [H, W], written bool [C, H, W]).  With prev -- the state before the frame -- an element that is
    not written keeps prev's value; without it `out` is the product everywhere, which is the same thing as long as `a`
    changed at listed pixels only."""
    assert gateNow.dtype == F32 and held.dtype == F32 and gateNow.shape == held.shape == (a.shape[0],)
    th = F32(threshold)
    with np.errstate(all='ignore'):
        tripped = np.ones(len(held), dtype=bool) if all else ~(np.abs(gateNow - held) <= th)
    new = np.where(tripped, gateNow, held).astype(F32)
    listed = np.ones(a.shape[1:], dtype=bool) if all else listed
    written = listed[None, :, :] | tripped[:, None, None]
    out = product(a, new)
    if prev is not None:
        out = np.where(written, out, prev)
    mask = np.ones_like(listed) if tripped.any() else listed.copy()
    return new, tripped, out, mask, written


def tripped_words(tripped):
    """The tripped channels as the library's ballot words (uint64, bit c % 64 of word c / 64)."""
    n = (len(tripped) + 63) // 64
    pad = np.zeros(n * 64, dtype=bool)
    pad[:len(tripped)] = tripped
    return np.packbits(pad.reshape(n, 64), axis=-1, bitorder='little').reshape(-1).view('<u8').copy()


def operands(rng, C, R, bias=True):
    """(W1 [R, C], b1, W2 [C, R], b2) float32: weights of both signs scaled so that s stays within a few units."""
    W1 = (rng.standard_normal((R, C)) / math.sqrt(C)).astype(F32)
    W2 = (rng.standard_normal((C, R)) * (2.0 / math.sqrt(R))).astype(F32)
    b1 = rng.uniform(-0.5, 0.5, R).astype(F32) if bias else None
    b2 = rng.uniform(-1.0, 1.0, C).astype(F32) if bias else None
    return W1, b1, W2, b2
