"""Change-based operators of two maps: CBBinary2d, CBGLU2d, CBGated and insertCBGating (cb_binary.hip),
CBBinary2d('correlate'), the correlation layer / cost volume of flow and stereo networks (cb_corr.hip), and
CBBinary2d('aggregate'), the per-pixel kernel application that takes such a volume back to a feature map (cb_aggr.hip,
DESIGN 5.34), and CBBinary2d('deform'), the deformable convolution of a feature map and an offset field (cb_deform.hip,
DESIGN 5.35), and CBBinary2d('attend'), local attention -- scores, softmax and weighted sum -- in one kernel
(cb_attend.hip), with partition= the partitioned window attention of Swin-type blocks (cb_winattend.hip,
DESIGN 5.37).

The reference has no element-wise operator of two maps, and CBAdd2d is the sum alone: a gate `feat * sigmoid(gate)`, a
layer scale `gamma[c] * x`, a residual by difference `x - net(x)`, an element-wise maximum or an nn.GLU over the
channels ends a change-based chain -- the torch operator recomputes the whole map, drops both operands' change lists and
cannot be recorded by a FrameProgram.  Every producer of this package leaves the pixels outside its change list bit for
bit as they were, so op(a, b) can differ from last frame's only at the UNION of the two lists, and a constant operand (a
parameter) never changes: the modules here recompute it there and are the dense result exactly, without a threshold.
"""
import ctypes
import numbers

import torch
import torch.nn as nn

from . import _lib
from ._lib import C, CBinferError, check, ptr, require_device, stream_ptr
from .chain import (EVERY_PIXEL, OPERAND_WORDS, CBStateModule, check_map, form_args, insert_behind_producers,
                    mask_workspace, operand_changes, producers, split_operand)
from .residual import _sequential

_OPS = {'add': _lib.BIN_ADD, 'sub': _lib.BIN_SUB, 'mul': _lib.BIN_MUL, 'maximum': _lib.BIN_MAXIMUM,
        'minimum': _lib.BIN_MINIMUM}
_GATES = {None: _lib.BIN_GATE_NONE, 'sigmoid': _lib.BIN_GATE_SIGMOID, 'hardsigmoid': _lib.BIN_GATE_HARDSIGMOID}
# the correlation layer, the per-pixel kernel application, the deformable convolution and the fused local attention have
# entry points of their own and no CB_BIN_* code (cb_corr.hip, cb_aggr.hip, cb_deform.hip, cb_attend.hip)
CORRELATE, AGGREGATE, DEFORM, ATTEND = 'correlate', 'aggregate', 'deform', 'attend'
_BORDERS = {'mask': _lib.ATTEND_MASK, 'zero': _lib.ATTEND_ZERO}
MAX_ATTEND_SPAN, MAX_HEAD_CHANNELS, MAX_HEADS = 48, 128, 64
MAX_PARTITION, MAX_PARTITION_TOKENS, MAX_PARTITION_HEAD_CHANNELS = 16, 144, 64
_MODULATIONS = {None: _lib.DEFORM_NONE, 'planes': _lib.DEFORM_PLANES, 'sigmoid': _lib.DEFORM_SIGMOID}
_DEFORM_KEYS = ('weight', 'bias', 'stride', 'padding', 'dilation', 'offsetGroups', 'modulation', 'relu')
MAX_DISPLACEMENT, MAX_STEP, MAX_CORR_CHANNELS, MAX_WEIGHT_PLANES = 64, 8, 512, 4096


def correlation_window(displacement, step, what="output channels"):
    """(y0, y1, x0, x1, Dy, Dx) of CBBinary2d('correlate' / 'aggregate', displacement=, step=): displacement an int r
    (both axes -r .. r), a pair (ry, rx) or ((y0, y1), (x0, x1)); CBinferError naming the setting beyond the library's
    limits.  what: the name of the Dy Dx things the window makes in the limit's message."""
    def whole(v):
        return isinstance(v, numbers.Integral) and not isinstance(v, bool)
    d = displacement
    if whole(d):
        d = (d, d)
    ok = isinstance(d, (tuple, list)) and len(d) == 2
    if ok and all(whole(v) for v in d):
        d = ((-d[0], d[0]), (-d[1], d[1]))
    ok = ok and all(isinstance(r, (tuple, list)) and len(r) == 2 and all(whole(v) for v in r) for r in d)
    if not ok:
        raise CBinferError("CBBinary2d: displacement=%r must be an int r, a pair (ry, rx) or ((y0, y1), (x0, x1))"
                           % (displacement,))
    (y0, y1), (x0, x1) = ((int(v) for v in r) for r in d)
    if not whole(step) or not 1 <= step <= MAX_STEP:
        raise CBinferError("CBBinary2d: step=%r must be an int in 1 .. %d" % (step, MAX_STEP))
    if y0 > y1 or x0 > x1 or max(abs(v) for v in (y0, y1, x0, x1)) > MAX_DISPLACEMENT:
        raise CBinferError("CBBinary2d: displacement=%r: every range must be ascending and within -%d .. %d"
                           % (displacement, MAX_DISPLACEMENT, MAX_DISPLACEMENT))
    if (y1 - y0) % step or (x1 - x0) % step:
        raise CBinferError("CBBinary2d: step=%d must divide both range lengths of displacement=%r (%d and %d)"
                           % (step, displacement, y1 - y0, x1 - x0))
    Dy, Dx = (y1 - y0) // step + 1, (x1 - x0) // step + 1
    if Dy * Dx > MAX_CORR_CHANNELS:
        raise CBinferError("CBBinary2d: displacement=%r with step=%d gives %d x %d = %d %s, the limit is %d"
                           % (displacement, step, Dy, Dx, Dy * Dx, what, MAX_CORR_CHANNELS))
    return y0, y1, x0, x1, Dy, Dx


# operand_changes' refusals in these modules' words (which: 'operand a' / 'operand b')
_WORDS = (
    "%(name)s: the change indexes of %(which)s address a %(h)dx%(w)d map, the operands are %(H)dx%(W)d maps",
    OPERAND_WORDS[1],
    "%(name)s: the change indexes of %(which)s must be a contiguous one-dimensional int32 tensor on the operands' device")


class _CBBinaryBase(CBStateModule):
    """What CBBinary2d and CBGLU2d share: the function, the workspace and the library call."""
    _WORK = '_binWork'

    def _set_function(self, name, op, gate, reverse):
        if op not in _OPS:
            raise CBinferError("%s: op=%r is not supported, only one of %s"
                               % (name, op, ", ".join(repr(k) for k in list(_OPS) + [CORRELATE, AGGREGATE, DEFORM, ATTEND])))
        if gate not in _GATES:
            raise CBinferError("%s: gate=%r is not supported, only None, 'sigmoid' or 'hardsigmoid'" % (name, gate))
        self.op, self.gate, self.reverse = op, gate, bool(reverse)
        if not C.cbinfer_binary_supported(_OPS[op], _GATES[gate], int(self.reverse)):
            raise CBinferError("%s: op=%r with gate=%r, reverse=%r: a gate goes with 'mul' only (out = a * g(b)), "
                               "reverse with 'sub' only (out = b - a)" % (name, op, gate, self.reverse))

    def _workspace(self, H, W, dev):
        """Working mask (zero between frames), the frame's mask copy, index buffer and count: once per map size."""
        return self._cached_work((H, W, dev), lambda: mask_workspace(H, W, dev))

    def _frame(self, name, a, ia, b, ib, form, bChanges, nc, H, W):
        """One frame: a [1, nc (2 nc in halves form), H, W], b in `form` (None in halves form), ia / ib the operands'
        change indexes or None."""
        work = self._workspace(H, W, a.device)
        # (a list the producer's kernel already made is taken before its mask: CBAdd2d's rule)
        fa = operand_changes(name, 'operand a', ia, H, W, a.device, work['idx'], words=_WORDS, maskWhenMade=False)
        fb = EVERY_PIXEL
        if bChanges == _lib.BIN_B_OWN and form in (_lib.BIN_MAP, _lib.BIN_PIXEL):
            fb = operand_changes(name, 'operand b', ib, H, W, a.device, work['idx'], words=_WORDS, maskWhenMade=False)
        if self._fresh_state((1, nc, H, W), a):      # (written completely: neither operand's change information is used)
            fa = fb = EVERY_PIXEL
        check(C.cbinfer_cbbinary_forward(ptr(a), ptr(b), ptr(self.outputState), *form_args(fa), *form_args(fb), form,
                                         bChanges, ptr(work['bits']), ptr(work['copy']), nc, H, W, _OPS[self.op],
                                         _GATES[self.gate], int(self.reverse), _lib.dtype_code(a), stream_ptr(a)))
        return self._result(work, H, W)


class CBBinary2d(_CBBinaryBase):
    """out = op(a, b) -- op one of 'add', 'sub' (reverse=True: b - a), 'mul' (gate='sigmoid' / 'hardsigmoid':
    a * g(b)), 'maximum', 'minimum' --, recomputed at the union of the operands' changed pixels (no counterpart in the
    reference; the arithmetic is specified in include/cbinfer_hip.h and is torch's bit for bit but for the sigmoid gate,
    whose bound DESIGN 5.25 has).

    forward(a, b) without `other`, forward(a) with it.  a is [1, C, H, W]; a per-frame b is [1, C, H, W], [1, 1, H, W]
    (one value per pixel, used for every channel) or [1, C, 1, 1] (a per-frame channel vector changes the whole map: every
    pixel is recomputed, and the frame still consists of library calls only).  Each argument is a bare tensor -- no change
    information: every pixel is recomputed -- or the ('changeIndexes', tensor, indexes) tuple of a producer with
    propChangeIndexes, taken as CBAdd2d takes it; a tuple for a [1, C, 1, 1] operand is refused.

    other: a constant second operand, which never changes, so only a's changes count -- a tensor or Parameter of shape
    [1, C, H, W], [1, 1, H, W], [1, C, 1, 1] / [C, 1, 1] / [C], or of one element.  It is COPIED here into the buffer
    `other`, which follows .to() / .half(); later edits of the source are not followed (as CBPointwise2d).  A Python
    number is converted once to the operand's dtype at the first frame: for float16 that is
    x * torch.tensor(v, dtype=x.dtype), which can differ in the last bit from torch's x * v.

    The flags are CBAdd2d's: propChangeIndexes hands on the union as a MaskChangeIndexes; cloneOutput=False hands out the
    state itself, tagged, and the frame is then free of torch operators.

    op='correlate' -- CBBinary2d('correlate', displacement=4, step=1, normalize=True) -- is the correlation layer (cost
    volume) of FlowNet / PWC-Net / DispNet-type networks on the matrix cores (cb_corr.hip): a and b are
    [1, C, H, W] maps of one shape, dtype and device, the state is [1, Dy Dx, H, W],
        out[i Dx + j, y, x] = (1/C) sum_c a[c, y, x] b[c, y + y0 + i step, x + x0 + j step],
    a tap outside the map contributing nothing; normalize=False is the plain sum.  displacement: an int r (both axes
    -r .. r), a pair (ry, rx), or ((y0, y1), (x0, x1)) for one-sided ranges (stereo: ((0, 0), (-40, 0))); step divides
    both range lengths; every |displacement| <= 64, step <= 8, Dy Dx <= 512.  A pixel is recomputed iff a changed there or
    b changed at one of its window's taps -- the handed-on mask is that footprint.  `other`, `gate` and `reverse` do not
    go with it, and displacement / step / normalize go with no other op.  It has no conversion pass: an operator of two
    inputs never stands in an nn.Sequential, it is wired by hand as the per-frame flow of CBResize2d is.

    op='aggregate' -- CBBinary2d('aggregate', displacement=4, step=1, groups=1), forward(w, v) -- is the operator that
    consumes such a volume (cb_aggr.hip): the attn . V half of local attention, the kernel application of
    kernel-prediction networks, CARAFE's reassembly, involution (groups = C / 16) and dynamic filters, on the matrix
    cores.  w is [1, G T, H, W] with T = Dy Dx taps and G = groups dividing C, v [1, C, H, W] of the same H, W, dtype and
    device, the state is [1, C, H, W],
        out[c, y, x] = sum_{i, j} w[g(c) T + i Dx + j, y, x] v[c, y + y0 + i step, x + x0 + j step],   g(c) = c // (C // G),
    a tap outside the map contributing nothing: the plane order of w is correlate's, so correlate -> softmax -> aggregate
    needs nothing in between.  displacement / step as for 'correlate' (T <= 512, G T <= 4096).  A pixel is recomputed iff
    w changed there or v changed at one of its window's taps.  Both operands must hold FINITE values (a 16-pixel group
    multiplies the columns outside a pixel's own window by zero).  `other`, `gate`, `reverse` and `normalize` do not go
    with it, `groups` goes with no other op; it has no conversion pass either.

    op='deform' -- CBBinary2d('deform', weight=W, bias=None, stride=1, padding=0, dilation=1, offsetGroups=1,
    modulation=None, relu=False), forward(x, field) -- is the deformable convolution (DCNv1 / DCNv2:
    torchvision.ops.deform_conv2d, mmcv's ModulatedDeformConv2d) on the matrix cores (cb_deform.hip).  W is
    [K, C, kH, kW] and bias [K] or None, both COPIED into buffers that follow .to() / .half(); x is [1, C, Hi, Wi], the
    state [1, K, Ho, Wo] with the convolution's output size.  field is [1, F, Ho, Wo], float32 or float16 whatever x is:
    first the 2 Go T offset planes (T = kH kW, Go = offsetGroups dividing C; plane 2 (g T + t) is dy, the next one dx for
    tap t = ky kW + kx: torchvision's and mmcv's layout), then by modulation= nothing (None, F = 2 Go T), Go T multiplier
    planes ('planes', F = 3 Go T: torchvision's mask behind the offsets) or the same planes before their sigmoid
    ('sigmoid': mmcv's DCNv2 block, whose conv_offset output is this field as it stands),
        out[k, oy, ox] = bias[k] + sum_{c, t} W[k, c, t] m[g(c) T + t, oy, ox]
                                              S(x[c], oy sH - pH + ky dH + dy, ox sW - pW + kx dW + dx),
    S the bilinear sample in which a tap outside the map contributes nothing.  A pixel is recomputed iff the field changed
    there or x changed at one of its taps that count; the handed-on mask is that footprint on the OUTPUT map.  One weight
    group only; the keywords of the other ops do not go with it and its own go with no other op; it has no conversion
    pass either.

    op='attend' -- CBBinary2d('attend', displacement=4, step=1, heads=1, scale=None, border='mask', positionBias=None),
    forward(q, kv) -- is local / neighbourhood attention (SASA, NAT-type blocks, HaloNet-style heads, local cross-frame
    attention) as ONE kernel on the matrix cores (cb_attend.hip): what correlate -> softmax -> aggregate
    compute, without the volume of heads x T score planes, which stays in a wave's registers.  q is [1, C, H, W]; kv is
    [1, C + Cv, H, W] of the same H, W, dtype and device, its first C channels k and the remaining Cv channels v -- the kv
    projection as ONE convolution and one change list (separately produced k and v go through CBConcat2d); the state is
    [1, Cv, H, W].  heads divides C and Cv, d = C / heads, dv = Cv / heads, head h owns channels h d .. of q and k and
    h dv .. of v and out:
        s[h, t] = scale sum_c q[h d + c, y, x] k[h d + c, y + dy_t, x + dx_t] (+ positionBias[h, t]),
        out[h dv + c, y, x] = sum_t softmax_t(s[h, .]) v[h dv + c, y + dy_t, x + dx_t],
    t = i Dx + j in correlate's tap order.  scale: a float, default d ** -0.5.  positionBias: None or a constant
    [heads, Dy Dx] / [heads, Dy, Dx] tensor (the relative position bias of NAT / Swin-type blocks), COPIED into a float32
    buffer that follows .to() and stays float32 under .half().  border='mask': a tap outside the map takes no part in the
    softmax (a pixel without any tap is +0); border='zero': such a tap has score 0 (plus its bias) and value 0, which is
    what the hand-wired correlate -> softmax -> aggregate chain computes.  displacement / step as for 'correlate' with
    x1 - x0 <= 48; d, dv <= 128; heads <= 64.  A pixel is recomputed iff q changed there or kv changed at one of its
    window's in-map taps.  Both operands must hold FINITE values, as for 'aggregate'.  `other`, `gate`, `reverse`,
    `normalize`, `groups` and the keywords of 'deform' do not go with it, its own go with no other op; it has no
    conversion pass either.

    op='attend' with partition= -- CBBinary2d('attend', partition=(Wy, Wx), shift=(sy, sx), heads=1, scale=None,
    positionBias=None), forward(q, kv) -- is PARTITIONED window attention (Swin, Video-Swin frames, SwinIR-type
    restoration networks, Twins' locally-grouped attention) as one kernel of its own (cb_winattend.hip).
    The operands, heads and scale are those above.  The map is cut into non-overlapping Wy x Wx cells: pixel (y, x) lies
    in cell (floor((y - sy) / Wy), floor((x - sx) / Wx)), so rows y < sy are cell row -1; cells are clipped at the map's
    edge and the tokens of a cell are its in-map pixels.  Every token attends to every token of its own cell:
        s[i, j] = scale sum_c q[h d + c, i] k[h d + c, j] (+ positionBias[h, yi - yj + Wy - 1, xi - xj + Wx - 1]),
        out[h dv + c, i] = sum_j softmax_j(s[i, .]) v[h dv + c, j].
    partition and shift: an int or a pair, 1 <= Wy, Wx <= 16, Wy Wx <= 144, 0 <= sy < Wy, 0 <= sx < Wx (shift defaults
    to 0); d, dv <= 64; heads <= 64.  positionBias: a constant [heads, 2 Wy - 1, 2 Wx - 1] tensor or the same flattened
    -- Swin's relative_position_bias_table.t() as it stands --, kept in float32.  On a map whose sides are multiples of
    Wy and Wx this is exactly Swin's cyclic shift by (-sy, -sx) with its region mask: the three bands per axis of the
    rolled map are the clipped cells.  Two differences: on other map sizes Swin zero-pads and the padding takes part in
    its softmax, here the cells are clipped; and Swin's mask adds -100 where this rule excludes the key exactly.  A pixel
    is recomputed iff q changed there or kv changed at ANY pixel of its cell; a cell without a change costs nothing.
    displacement=, step= and border= do not go with partition=, shift= goes with nothing else.  Out of scope: Swin-V2's
    cosine attention and per-head logit scale, global attention, a conversion pass (INTEGRATION.md has the wiring of a
    Swin block pair)."""

    def __init__(self, op, other=None, gate=None, reverse=False, displacement=None, step=None, normalize=None,
                 groups=None, weight=None, bias=None, stride=None, padding=None, dilation=None, offsetGroups=None,
                 modulation=None, relu=False, heads=None, scale=None, border=None, positionBias=None, partition=None,
                 shift=None):
        super(CBBinary2d, self).__init__()
        if op != ATTEND:
            for key, value in dict(heads=heads, scale=scale, border=border, positionBias=positionBias,
                                   partition=partition, shift=shift).items():
                if value is not None:
                    raise CBinferError("CBBinary2d: %s= is a setting of op='attend', op=%r does not take it" % (key, op))
        window = dict(displacement=displacement, step=step, normalize=normalize)
        own = dict(zip(_DEFORM_KEYS, (weight, bias, stride, padding, dilation, offsetGroups, modulation, relu or None)))
        if op == DEFORM:
            refused = dict(window, other=other, gate=gate, reverse=reverse or None)
            for key, value in refused.items():
                if value is not None:
                    raise CBinferError("CBBinary2d: %s= does not go with op=%r" % (key, op))
            if groups not in (None, 1):
                raise CBinferError("CBBinary2d: groups=%r: op='deform' takes one weight group only (offsetGroups= are the "
                                   "offset field's groups)" % (groups,))
            self.op, self.gate, self.reverse = op, None, False
            self._set_deform(weight, bias, stride, padding, dilation, offsetGroups, modulation, relu)
            self._buffers['outputState'] = self._buffers.pop('outputState')
            self.otherNumber, self.hasOther, self._deformPrep = None, False, None
            return
        for key, value in own.items():
            if value is not None:
                raise CBinferError("CBBinary2d: %s= goes with op='deform' only, not with op=%r" % (key, op))
        if op == ATTEND:
            refused = dict(other=other, gate=gate, reverse=reverse or None, normalize=normalize, groups=groups)
            for key, value in refused.items():
                if value is not None:
                    raise CBinferError("CBBinary2d: %s= does not go with op=%r" % (key, op))
            self.op, self.gate, self.reverse = op, None, False
            if partition is not None:
                for key, value in dict(displacement=displacement, step=step, border=border).items():
                    if value is not None:
                        raise CBinferError("CBBinary2d: %s= does not go with partition= (the cells are the window)" % key)
                self._set_partition(partition, shift, heads, scale, positionBias)
            elif shift is not None:
                raise CBinferError("CBBinary2d: shift= goes with partition= only")
            else:
                self._set_attend(displacement, step, heads, scale, border, positionBias)
            self._buffers['outputState'] = self._buffers.pop('outputState')
            self.otherNumber, self.hasOther = None, False
            return
        if op in (CORRELATE, AGGREGATE):
            refused = (('other', other is not None), ('gate', gate is not None), ('reverse', bool(reverse)),
                       ('groups', groups is not None) if op == CORRELATE else ('normalize', normalize is not None))
            for key, given in refused:
                if given:
                    raise CBinferError("CBBinary2d: %s= does not go with op=%r" % (key, op))
            self.op, self.gate, self.reverse = op, None, False
            self.displacement = 4 if displacement is None else displacement
            self.step = 1 if step is None else step
            if op == CORRELATE:
                self.normalize = True if normalize is None else bool(normalize)
                self.window = correlation_window(self.displacement, self.step)
            else:
                self.groups = 1 if groups is None else groups
                self.window = correlation_window(self.displacement, self.step, "taps")
                taps = self.window[4] * self.window[5]
                if (not isinstance(self.groups, numbers.Integral) or isinstance(self.groups, bool) or
                        not 1 <= self.groups <= MAX_WEIGHT_PLANES // taps):
                    raise CBinferError("CBBinary2d: groups=%r must be an int >= 1 with groups x %d taps within %d weight "
                                       "planes" % (self.groups, taps, MAX_WEIGHT_PLANES))
        else:
            for key, value in window.items():
                if value is not None:
                    raise CBinferError("CBBinary2d: %s= goes with op='correlate' only, not with op=%r (displacement= and "
                                       "step= with op='aggregate' as well)" % (key, op))
            if groups is not None:
                raise CBinferError("CBBinary2d: groups= goes with op='aggregate' only, not with op=%r" % (op,))
            self._set_function('CBBinary2d', op, gate, reverse)
        self.otherNumber = None
        self.hasOther = other is not None
        buf = None
        if isinstance(other, numbers.Real) and not isinstance(other, bool):
            self.otherNumber = float(other)
        elif torch.is_tensor(other):
            t = other.detach()
            ok = (t.numel() == 1 or t.dim() == 1 or (t.dim() == 3 and tuple(t.shape[1:]) == (1, 1)) or
                  (t.dim() == 4 and t.size(0) == 1))
            if not ok or t.numel() == 0:
                raise CBinferError("CBBinary2d: other has shape %s; a constant operand is [1, C, H, W], [1, 1, H, W], "
                                   "[1, C, 1, 1], [C, 1, 1], [C] or one element" % (tuple(t.shape),))
            if t.dtype not in (torch.float32, torch.float16):
                raise CBinferError("CBBinary2d: other must be a float32 or float16 tensor, got %s" % t.dtype)
            buf = t.clone().contiguous()
        elif other is not None:
            raise CBinferError("CBBinary2d: other must be a tensor, a Parameter or a Python number, got %s"
                               % type(other).__name__)
        self.register_buffer('other', buf)
        # (the state behind the constant operand, as state_dict() lists them)
        self._buffers['outputState'] = self._buffers.pop('outputState')

    def _constant(self, a, nc, H, W):
        """(tensor, CB_BIN_* form) of the constant operand for the frame of `a`; a number is converted once per
        workspace (the first frame) and kept with it."""
        if self.otherNumber is not None:
            require_device(a)
            work = self._workspace(H, W, a.device)
            key = (a.dtype, a.device)
            if work.get('numberKey') != key:
                work['number'] = torch.tensor([self.otherNumber], dtype=a.dtype).to(a.device)
                work['numberKey'] = key
            return work['number'], _lib.BIN_SCALAR
        t = self.other
        if t.dtype != a.dtype or t.device != a.device:
            raise CBinferError("CBBinary2d: operand a is %s on %s, the constant operand `other` %s on %s (move the "
                               "module with .to() / .half())" % (a.dtype, a.device, t.dtype, t.device))
        shape = tuple(t.shape)
        if t.numel() == 1:
            return t, _lib.BIN_SCALAR
        if shape == (1, nc, H, W):
            return t, _lib.BIN_MAP
        if shape == (1, 1, H, W):
            return t, _lib.BIN_PIXEL
        if shape in ((1, nc, 1, 1), (nc, 1, 1), (nc,)):
            return t, _lib.BIN_CHANNEL
        raise CBinferError("CBBinary2d: the constant operand `other` has shape %s, operand a is %s"
                           % (shape, tuple(a.shape)))

    def _set_deform(self, weight, bias, stride, padding, dilation, offsetGroups, modulation, relu):
        def whole(n):
            return isinstance(n, numbers.Integral) and not isinstance(n, bool)

        def pair(key, v, default):
            v = default if v is None else v
            v = (v, v) if whole(v) else v
            if not (isinstance(v, (tuple, list)) and len(v) == 2 and all(whole(n) for n in v)):
                raise CBinferError("CBBinary2d: %s=%r must be an int or a pair of ints" % (key, v))
            return int(v[0]), int(v[1])
        if not torch.is_tensor(weight) or weight.dim() != 4 or weight.numel() == 0:
            raise CBinferError("CBBinary2d: op='deform' takes weight=, a [K, C, kH, kW] tensor, got %s"
                               % (tuple(weight.shape) if torch.is_tensor(weight) else type(weight).__name__,))
        if weight.dtype not in (torch.float32, torch.float16):
            raise CBinferError("CBBinary2d: weight must be a float32 or float16 tensor, got %s" % weight.dtype)
        K, Cin, kH, kW = weight.shape
        if bias is not None and (not torch.is_tensor(bias) or tuple(bias.shape) != (K,) or bias.dtype != weight.dtype):
            raise CBinferError("CBBinary2d: bias must be a [%d] tensor of the weight's dtype or None" % K)
        if modulation not in _MODULATIONS:
            raise CBinferError("CBBinary2d: modulation=%r is not supported, only None, 'planes' or 'sigmoid'"
                               % (modulation,))
        Go = 1 if offsetGroups is None else offsetGroups
        if not whole(Go) or not 1 <= Go <= 16:
            raise CBinferError("CBBinary2d: offsetGroups=%r must be an int in 1 .. 16" % (offsetGroups,))
        if Cin % Go:
            raise CBinferError("CBBinary2d: offsetGroups=%d does not divide the %d input channels of weight" % (Go, Cin))
        self.stride, self.padding, self.dilation = (pair('stride', stride, 1), pair('padding', padding, 0),
                                                    pair('dilation', dilation, 1))
        self.offsetGroups, self.modulation, self.relu = int(Go), modulation, bool(relu)
        self.register_buffer('weight', weight.detach().clone().contiguous())
        self.register_buffer('bias', None if bias is None else bias.detach().clone().contiguous())
        if C.cbinfer_deform_prepared_weights_bytes(K, Cin, ctypes.byref(self._deform_struct(_lib.CB_F32)),
                                                   _lib.CB_F32) <= 0:
            raise CBinferError("CBBinary2d: kernel %dx%d stride=%s padding=%s dilation=%s is beyond what the library takes "
                               "(per axis: filter <= 7, stride <= 4, dilation <= 8, padding <= 64)"
                               % (kH, kW, self.stride, self.padding, self.dilation))

    def _deform_struct(self, fieldCode):
        kH, kW = self.weight.shape[2:]
        geom = _lib.Geom(kH, kW, *(self.stride + self.padding + self.dilation))
        return _lib.Deform(geom, self.offsetGroups, _MODULATIONS[self.modulation], fieldCode, int(self.relu))

    def _deform_forward(self, x, field):
        name = 'CBBinary2d'
        if field is None:
            raise CBinferError("CBBinary2d: forward(x, field) takes two operands")
        x, ix = split_operand(name, x, 'operand x')
        check_map(name, x, 'operand x')
        field, ifield = split_operand(name, field, 'the field')
        check_map(name, field, 'the field')
        w = self.weight
        K, Cin, kH, kW = w.shape
        if x.size(1) != Cin:
            raise CBinferError("CBBinary2d: operand x has %d channels, the weight takes %d" % (x.size(1), Cin))
        if w.dtype != x.dtype or w.device != x.device or field.device != x.device:
            raise CBinferError("CBBinary2d: operand x is %s on %s, the weight %s on %s, the field on %s (move the module "
                               "with .to() / .half())" % (x.dtype, x.device, w.dtype, w.device, field.device))
        Hi, Wi = x.size(2), x.size(3)
        planes = (2 if self.modulation is None else 3) * self.offsetGroups * kH * kW
        if field.size(1) != planes:
            raise CBinferError("CBBinary2d: the field has %d channels, offsetGroups=%d x %d x %d taps with modulation=%r "
                               "take %d" % (field.size(1), self.offsetGroups, kH, kW, self.modulation, planes))
        d = self._deform_struct(_lib.dtype_code(field))
        Ho, Wo = ctypes.c_int(), ctypes.c_int()
        if (C.cbinfer_geom_out_size(Hi, Wi, ctypes.byref(d.geom), ctypes.byref(Ho), ctypes.byref(Wo)) != 0 or
                not C.cbinfer_deform_supported(ctypes.byref(d), Cin, Hi, Wi, K)):
            raise CBinferError("CBBinary2d: the deformable convolution of a %s map to %d channels is beyond the "
                               "library's limits" % (tuple(x.shape), K))
        Ho, Wo = Ho.value, Wo.value
        if tuple(field.shape[2:]) != (Ho, Wo):
            raise CBinferError("CBBinary2d: the field is a %dx%d map, the output map of a %dx%d input is %dx%d"
                               % (field.size(2), field.size(3), Hi, Wi, Ho, Wo))
        require_device(x, field)

        def make():
            # (the output's working mask, x's on its own map, the shared split-k workspace with its zero counters)
            return dict(mask_workspace(Ho, Wo, x.device), deform=ctypes.pointer(d),
                        inBits=torch.zeros(C.cbinfer_mask_words(Hi, Wi), dtype=torch.int64, device=x.device),
                        conv=torch.zeros(C.cbinfer_geom_workspace_bytes(), dtype=torch.uint8, device=x.device))
        work = self._cached_work((DEFORM, Cin, Hi, Wi, field.dtype, x.device), make)
        key = (w.data_ptr(), w._version, w.dtype, w.device)
        if self._deformPrep is None or self._deformPrep[0] != key:
            code = _lib.dtype_code(w)
            wp = torch.empty(C.cbinfer_deform_prepared_weights_bytes(K, Cin, work['deform'], code), dtype=torch.uint8,
                             device=w.device)
            check(C.cbinfer_deform_prep_weights(ptr(w), ptr(wp), K, Cin, work['deform'], code, stream_ptr(w)))
            self._deformPrep = (key, wp)
        fx = operand_changes(name, 'operand x', ix, Hi, Wi, x.device, work['idx'], words=_WORDS, maskWhenMade=False)
        ff = operand_changes(name, 'the field', ifield, Ho, Wo, x.device, work['idx'], words=_WORDS, maskWhenMade=False)
        if self._fresh_state((1, K, Ho, Wo), x):      # (written completely: no change information is used)
            fx = ff = EVERY_PIXEL
        check(C.cbinfer_cbdeform_forward(ptr(x), ptr(field), ptr(self._deformPrep[1]), ptr(self.bias),
                                         ptr(self.outputState), *form_args(fx), *form_args(ff), ptr(work['inBits']),
                                         ptr(work['bits']), ptr(work['copy']), ptr(work['conv']), Cin, Hi, Wi, K,
                                         work['deform'], _lib.dtype_code(x), stream_ptr(x)))
        return self._result(work, Ho, Wo)

    def _set_heads(self, heads, scale):
        self.heads = 1 if heads is None else heads
        if (not isinstance(self.heads, numbers.Integral) or isinstance(self.heads, bool) or
                not 1 <= self.heads <= MAX_HEADS):
            raise CBinferError("CBBinary2d: heads=%r must be an int in 1 .. %d" % (heads, MAX_HEADS))
        if scale is not None and (not isinstance(scale, numbers.Real) or isinstance(scale, bool) or
                                  not abs(float(scale)) < float('inf')):
            raise CBinferError("CBBinary2d: scale=%r must be a finite number or None (d ** -0.5)" % (scale,))
        self.scale = None if scale is None else float(scale)

    def _set_partition(self, partition, shift, heads, scale, positionBias):
        def pair(key, v):
            v = (v, v) if isinstance(v, numbers.Integral) and not isinstance(v, bool) else v
            if not (isinstance(v, (tuple, list)) and len(v) == 2 and
                    all(isinstance(n, numbers.Integral) and not isinstance(n, bool) for n in v)):
                raise CBinferError("CBBinary2d: %s=%r must be an int or a pair of ints" % (key, v))
            return int(v[0]), int(v[1])
        Wy, Wx = self.partition = pair('partition', partition)
        if not (1 <= Wy <= MAX_PARTITION and 1 <= Wx <= MAX_PARTITION and Wy * Wx <= MAX_PARTITION_TOKENS):
            raise CBinferError("CBBinary2d: partition=%r: a cell is 1 .. %d pixels a side and %d tokens at most"
                               % (partition, MAX_PARTITION, MAX_PARTITION_TOKENS))
        sy, sx = self.shift = pair('shift', 0 if shift is None else shift)
        if not (0 <= sy < Wy and 0 <= sx < Wx):
            raise CBinferError("CBBinary2d: shift=%r must be within 0 .. partition - 1 = (%d, %d)"
                               % (shift, Wy - 1, Wx - 1))
        self._set_heads(heads, scale)
        buf = None
        if positionBias is not None:
            shapes = ((self.heads, (2 * Wy - 1) * (2 * Wx - 1)), (self.heads, 2 * Wy - 1, 2 * Wx - 1))
            if (not torch.is_tensor(positionBias) or tuple(positionBias.shape) not in shapes or
                    not positionBias.is_floating_point()):
                raise CBinferError("CBBinary2d: positionBias must be a floating-point tensor of shape %s or %s, got %s"
                                   % (shapes + (tuple(positionBias.shape) if torch.is_tensor(positionBias)
                                                else type(positionBias).__name__,)))
            buf = positionBias.detach().float().reshape(shapes[0]).clone().contiguous()
        self.register_buffer('positionBias', buf)

    def _set_attend(self, displacement, step, heads, scale, border, positionBias):
        self.displacement = 4 if displacement is None else displacement
        self.step = 1 if step is None else step
        self.window = correlation_window(self.displacement, self.step, "taps")
        y0, y1, x0, x1, Dy, Dx = self.window
        if x1 - x0 > MAX_ATTEND_SPAN:
            raise CBinferError("CBBinary2d: displacement=%r: op='attend' takes a column range x1 - x0 of %d at most, "
                               "got %d" % (self.displacement, MAX_ATTEND_SPAN, x1 - x0))
        self._set_heads(heads, scale)
        self.border = 'mask' if border is None else border
        if self.border not in _BORDERS:
            raise CBinferError("CBBinary2d: border=%r is not supported, only 'mask' or 'zero'" % (border,))
        buf = None
        if positionBias is not None:
            shapes = ((self.heads, Dy * Dx), (self.heads, Dy, Dx))
            if (not torch.is_tensor(positionBias) or tuple(positionBias.shape) not in shapes or
                    not positionBias.is_floating_point()):
                raise CBinferError("CBBinary2d: positionBias must be a floating-point tensor of shape %s or %s, got %s"
                                   % (shapes + (tuple(positionBias.shape) if torch.is_tensor(positionBias)
                                                else type(positionBias).__name__,)))
            buf = positionBias.detach().float().reshape(self.heads, Dy * Dx).clone().contiguous()
        self.register_buffer('positionBias', buf)

    def _apply(self, fn, *args, **kwargs):
        # (the position bias follows the module's device and stays float32, the kernel's: .half() does not convert it)
        held = self._buffers.get('positionBias')
        super(CBBinary2d, self)._apply(fn, *args, **kwargs)
        if held is not None and self._buffers['positionBias'].dtype != torch.float32:
            self._buffers['positionBias'] = held.to(self._buffers['positionBias'].device)
        return self

    def _attend(self, q, kv):
        name = 'CBBinary2d'
        if kv is None:
            raise CBinferError("CBBinary2d: forward(q, kv) takes two operands")
        q, iq = split_operand(name, q, 'operand q')
        check_map(name, q, 'operand q')
        kv, ikv = split_operand(name, kv, 'operand kv')
        check_map(name, kv, 'operand kv')
        if tuple(kv.shape[2:]) != tuple(q.shape[2:]) or kv.dtype != q.dtype or kv.device != q.device:
            raise CBinferError("CBBinary2d: the operands differ: q is %s %s on %s, kv is %s %s on %s"
                               % (tuple(q.shape), q.dtype, q.device, tuple(kv.shape), kv.dtype, kv.device))
        part = getattr(self, 'partition', None)
        nc, H, W = q.size(1), q.size(2), q.size(3)
        ncv = kv.size(1) - nc
        if ncv < 1:
            raise CBinferError("CBBinary2d: operand kv has %d channels: behind the %d channels of k (operand q's count) "
                               "it holds no channel of v" % (kv.size(1), nc))
        if nc % self.heads or ncv % self.heads:
            raise CBinferError("CBBinary2d: heads=%d does not divide the %d channels of q and k and the %d channels of v"
                               % (self.heads, nc, ncv))
        most = MAX_HEAD_CHANNELS if part is None else MAX_PARTITION_HEAD_CHANNELS
        if max(nc, ncv) // self.heads > most:
            raise CBinferError("CBBinary2d: %d channels of q and %d of v over heads=%d: a head takes %d channels at most"
                               % (nc, ncv, self.heads, most))
        bias = self.positionBias
        if bias is not None and bias.device != q.device:
            raise CBinferError("CBBinary2d: operand q is on %s, positionBias on %s (move the module with .to())"
                               % (q.device, bias.device))
        require_device(q, kv)

        def make():
            scale = (nc // self.heads) ** -0.5 if self.scale is None else self.scale
            if part is None:
                y0, y1, x0, x1, Dy, Dx = self.window
                att = _lib.Attend(y0, y1, x0, x1, self.step, self.heads, _BORDERS[self.border], int(bias is not None),
                                  scale)
                supported = C.cbinfer_attend_supported
            else:
                att = _lib.WinAttend(*(part + self.shift), self.heads, int(bias is not None), scale)
                supported = C.cbinfer_winattend_supported
            if not supported(ctypes.byref(att), nc, ncv, H, W):
                raise CBinferError("CBBinary2d: attending %s to %s is beyond the library's limits"
                                   % (tuple(q.shape), tuple(kv.shape)))
            work = mask_workspace(H, W, q.device, nbits=2)      # (the output's working mask, then kv's)
            return dict(work, attend=ctypes.pointer(att), kvBits=work['bits'][work['copy'].numel():])
        work = self._cached_work((ATTEND, nc, ncv, H, W, q.device), make)
        fq = operand_changes(name, 'operand q', iq, H, W, q.device, work['idx'], words=_WORDS, maskWhenMade=False)
        fkv = operand_changes(name, 'operand kv', ikv, H, W, q.device, work['idx'], words=_WORDS, maskWhenMade=False)
        if self._fresh_state((1, ncv, H, W), q):      # (written completely: no change information is used)
            fq = fkv = EVERY_PIXEL
        forward = C.cbinfer_cbattend_forward if part is None else C.cbinfer_cbwinattend_forward
        check(forward(ptr(q), ptr(kv), ptr(bias), ptr(self.outputState), *form_args(fq), *form_args(fkv),
                      ptr(work['kvBits']), ptr(work['bits']), ptr(work['copy']), nc, ncv, H, W, work['attend'],
                      _lib.dtype_code(q), stream_ptr(q)))
        return self._result(work, H, W)

    def _correlate(self, a, b):
        name = 'CBBinary2d'
        if b is None:
            raise CBinferError("CBBinary2d: forward(a, b) takes two operands")
        a, ia = split_operand(name, a, 'operand a')
        check_map(name, a, 'operand a')
        b, ib = split_operand(name, b, 'operand b')
        if tuple(b.shape) != tuple(a.shape) or b.dtype != a.dtype or b.device != a.device:
            raise CBinferError("CBBinary2d: the operands differ: a is %s %s on %s, b is %s %s on %s"
                               % (tuple(a.shape), a.dtype, a.device, tuple(b.shape), b.dtype, b.device))
        require_device(a, b)
        nc, H, W = a.size(1), a.size(2), a.size(3)
        y0, y1, x0, x1, Dy, Dx = self.window

        def make():
            corr = _lib.Corr(y0, y1, x0, x1, self.step, int(self.normalize))
            if not C.cbinfer_correlation_supported(ctypes.byref(corr), nc, H, W):
                raise CBinferError("CBBinary2d: correlating %s maps is beyond the library's limits" % (tuple(a.shape),))
            work = mask_workspace(H, W, a.device, nbits=2)      # (the output's working mask, then b's)
            return dict(work, corr=ctypes.pointer(corr), bBits=work['bits'][work['copy'].numel():])
        work = self._cached_work((CORRELATE, nc, H, W, a.device), make)
        fa = operand_changes(name, 'operand a', ia, H, W, a.device, work['idx'], words=_WORDS, maskWhenMade=False)
        fb = operand_changes(name, 'operand b', ib, H, W, a.device, work['idx'], words=_WORDS, maskWhenMade=False)
        if self._fresh_state((1, Dy * Dx, H, W), a):      # (written completely: no change information is used)
            fa = fb = EVERY_PIXEL
        check(C.cbinfer_cbcorrelation_forward(ptr(a), ptr(b), ptr(self.outputState), *form_args(fa), *form_args(fb),
                                              ptr(work['bBits']), ptr(work['bits']), ptr(work['copy']), nc, H, W,
                                              work['corr'], _lib.dtype_code(a), stream_ptr(a)))
        return self._result(work, H, W)

    def _aggregate(self, w, v):
        name = 'CBBinary2d'
        if v is None:
            raise CBinferError("CBBinary2d: forward(w, v) takes two operands")
        w, iw = split_operand(name, w, 'operand w')
        check_map(name, w, 'operand w')
        v, iv = split_operand(name, v, 'operand v')
        check_map(name, v, 'operand v')
        if tuple(v.shape[2:]) != tuple(w.shape[2:]) or v.dtype != w.dtype or v.device != w.device:
            raise CBinferError("CBBinary2d: the operands differ: w is %s %s on %s, v is %s %s on %s"
                               % (tuple(w.shape), w.dtype, w.device, tuple(v.shape), v.dtype, v.device))
        y0, y1, x0, x1, Dy, Dx = self.window
        nc, H, W = v.size(1), v.size(2), v.size(3)
        if w.size(1) != self.groups * Dy * Dx:
            raise CBinferError("CBBinary2d: operand w has %d channels, groups=%d x %d x %d taps take %d"
                               % (w.size(1), self.groups, Dy, Dx, self.groups * Dy * Dx))
        if nc % self.groups:
            raise CBinferError("CBBinary2d: groups=%d does not divide the %d channels of operand v" % (self.groups, nc))
        require_device(w, v)

        def make():
            aggr = _lib.Aggr(y0, y1, x0, x1, self.step, self.groups)
            if not C.cbinfer_aggregate_supported(ctypes.byref(aggr), nc, H, W):
                raise CBinferError("CBBinary2d: aggregating %s maps is beyond the library's limits" % (tuple(v.shape),))
            work = mask_workspace(H, W, w.device, nbits=2)      # (the output's working mask, then v's)
            return dict(work, aggr=ctypes.pointer(aggr), vBits=work['bits'][work['copy'].numel():])
        work = self._cached_work((AGGREGATE, nc, H, W, w.device), make)
        fw = operand_changes(name, 'operand w', iw, H, W, w.device, work['idx'], words=_WORDS, maskWhenMade=False)
        fv = operand_changes(name, 'operand v', iv, H, W, w.device, work['idx'], words=_WORDS, maskWhenMade=False)
        if self._fresh_state((1, nc, H, W), v):      # (written completely: no change information is used)
            fw = fv = EVERY_PIXEL
        check(C.cbinfer_cbaggregate_forward(ptr(w), ptr(v), ptr(self.outputState), *form_args(fw), *form_args(fv),
                                            ptr(work['vBits']), ptr(work['bits']), ptr(work['copy']), nc, H, W,
                                            work['aggr'], _lib.dtype_code(w), stream_ptr(w)))
        return self._result(work, H, W)

    def forward(self, a, b=None):
        if self.op == CORRELATE:
            return self._correlate(a, b)
        if self.op == AGGREGATE:
            return self._aggregate(a, b)
        if self.op == DEFORM:
            return self._deform_forward(a, b)
        if self.op == ATTEND:
            return self._attend(a, b)
        if self.hasOther and b is not None:
            raise CBinferError("CBBinary2d: the module has a constant operand `other`: forward(a) takes one argument")
        if not self.hasOther and b is None:
            raise CBinferError("CBBinary2d: forward(a, b) takes two operands (or give the module a constant `other`)")
        a, ia = split_operand('CBBinary2d', a, 'operand a')
        check_map('CBBinary2d', a, 'operand a')
        nc, H, W = a.size(1), a.size(2), a.size(3)
        if self.hasOther:
            t, form = self._constant(a, nc, H, W)
            require_device(a)
            return self._frame('CBBinary2d', a, ia, t, None, form, _lib.BIN_B_NONE, nc, H, W)
        b, ib = split_operand('CBBinary2d', b, 'operand b')
        shape = tuple(b.shape)
        if shape == (1, nc, H, W):
            form = _lib.BIN_MAP
        elif shape == (1, 1, H, W):
            form = _lib.BIN_PIXEL
        elif shape == (1, nc, 1, 1):
            form = _lib.BIN_CHANNEL
        else:
            raise CBinferError("CBBinary2d: the operands do not fit: a is %s, b is %s; b must be [1, C, H, W], "
                               "[1, 1, H, W] or [1, C, 1, 1]" % (tuple(a.shape), shape))
        if b.dtype != a.dtype or b.device != a.device:
            raise CBinferError("CBBinary2d: the operands differ: a is %s %s on %s, b is %s %s on %s"
                               % (tuple(a.shape), a.dtype, a.device, shape, b.dtype, b.device))
        if form == _lib.BIN_CHANNEL and ib is not None:
            raise CBinferError("CBBinary2d: operand b is a [1, C, 1, 1] channel vector %s and came with change indexes: "
                               "a channel vector has no pixels, hand it over as a bare tensor" % (shape,))
        require_device(a, b)
        return self._frame('CBBinary2d', a, ia, b, ib, form, _lib.BIN_B_OWN, nc, H, W)

    def __repr__(self):
        if self.op == CORRELATE:
            return 'CBBinary2d (op=correlate, displacement=%r, step=%d, normalize=%s, propChgIdxs=%s)' % (
                self.displacement, self.step, self.normalize, self.propChangeIndexes)
        if self.op == AGGREGATE:
            return 'CBBinary2d (op=aggregate, displacement=%r, step=%d, groups=%d, propChgIdxs=%s)' % (
                self.displacement, self.step, self.groups, self.propChangeIndexes)
        if self.op == ATTEND and getattr(self, 'partition', None) is not None:
            return ('CBBinary2d (op=attend, partition=%r, shift=%r, heads=%d, scale=%r, positionBias=%s, propChgIdxs=%s)'
                    % (self.partition, self.shift, self.heads, self.scale, self.positionBias is not None,
                       self.propChangeIndexes))
        if self.op == ATTEND:
            return ('CBBinary2d (op=attend, displacement=%r, step=%d, heads=%d, scale=%r, border=%s, positionBias=%s, '
                    'propChgIdxs=%s)' % (self.displacement, self.step, self.heads, self.scale, self.border,
                                         self.positionBias is not None, self.propChangeIndexes))
        if self.op == DEFORM:
            K, Cin, kH, kW = self.weight.shape
            return ('CBBinary2d (op=deform, %d -> %d, kernel=%dx%d, stride=%s, padding=%s, dilation=%s, offsetGroups=%d, '
                    'modulation=%s, bias=%s, relu=%s, propChgIdxs=%s)' % (
                        Cin, K, kH, kW, self.stride, self.padding, self.dilation, self.offsetGroups, self.modulation,
                        self.bias is not None, self.relu, self.propChangeIndexes))
        other = ('number %r' % self.otherNumber if self.otherNumber is not None else
                 tuple(self.other.shape) if self.other is not None else None)
        return 'CBBinary2d (op=%s, gate=%s, reverse=%s, other=%s, propChgIdxs=%s)' % (
            self.op, self.gate, self.reverse, other, self.propChangeIndexes)


class CBGLU2d(_CBBinaryBase):
    """nn.GLU over the channels, out = x[:, :C] * sigmoid(x[:, C:]), recomputed at the operand's changed pixels.

    m: an nn.GLU -- exactly that type -- with dim 1 or -3.  forward(x): a [1, 2C, H, W] tensor or the
    ('changeIndexes', tensor, indexes) tuple of a producer with propChangeIndexes; the state is [1, C, H, W].  Both
    halves are one operand with one change list (the library's halves form).  The flags are CBBinary2d's."""

    def __init__(self, m):
        super(CBGLU2d, self).__init__()
        if type(m) is not nn.GLU:
            raise CBinferError("CBGLU2d: %s is not supported, only an nn.GLU (exactly that type)" % type(m).__name__)
        if m.dim not in (1, -3):
            raise CBinferError("CBGLU2d: nn.GLU(dim=%d) does not gate over the channels of a [1, C, H, W] map "
                               "(dim 1 or -3)" % m.dim)
        self._set_function('CBGLU2d', 'mul', 'sigmoid', False)

    def forward(self, inp):
        x, ix = split_operand('CBGLU2d', inp, 'the input')
        check_map('CBGLU2d', x, 'operand x')
        if x.size(1) % 2:
            raise CBinferError("CBGLU2d: the input %s has an odd number of channels: nn.GLU halves them"
                               % (tuple(x.shape),))
        require_device(x)
        return self._frame('CBGLU2d', x, ix, None, None, _lib.BIN_HALVES, _lib.BIN_B_NONE, x.size(1) // 2, x.size(2),
                           x.size(3))

    def __repr__(self):
        return 'CBGLU2d (propChgIdxs=%s)' % self.propChangeIndexes


class CBGated(nn.Module):
    """out = op(body(x), g(gate(x))), or op(body(x), g(x)) without a gate branch, as one link of a change-based chain:
    the wiring twin of CBResidual (attention gates, gated convolutions, spatial attention with a one-channel gate map).

    `body` and `gate` are CONVERTED nn.Sequential containers.  Both are fed the bare tensor: their first layers run
    their own change detection.  The operator takes the body's result, and the gate branch's or -- without one -- the
    incoming operand with the incoming change list, if there was one.  The constructor switches propChangeIndexes on at
    the last module of body / gate where that is a CBConv2d, and copyInput on at their first layers that are not in
    feedback mode, as CBResidual's does.  The operator is `self.mul`, a CBBinary2d(op, gate=gateFn): set its
    propChangeIndexes / cloneOutput as on a CBAdd2d.  gateFn: 'sigmoid', 'hardsigmoid' or None ('mul' only)."""

    def __init__(self, body, gate=None, op='mul', gateFn='sigmoid'):
        super(CBGated, self).__init__()
        from .conv2d import CBConv2d
        self.body = _sequential(body)
        self.gate = _sequential(gate)
        self.mul = CBBinary2d(op, gate=gateFn)
        for seq in (self.body, self.gate):
            kids = list(seq.children()) if seq is not None else []
            if kids and type(kids[-1]) is CBConv2d:
                kids[-1].propChangeIndexes = True
            if kids and type(kids[0]) is CBConv2d and not kids[0].feedbackLoop:
                kids[0].copyInput = True

    def forward(self, inp):
        src = inp[1] if type(inp) == tuple else inp
        main = self.body(src)
        return self.mul(main, self.gate(src) if self.gate is not None else inp)


def insertCBGating(rootModule, cloneOutput=True):
    """Inside every nn.Sequential of rootModule, an nn.GLU over the channels (exactly that type, dim 1 or -3) that
    directly follows a producer -- chain.producers('insertCBGating') -- becomes a
    CBGLU2d under its name, fed by that producer's changes: propChangeIndexes is switched on at the producer
    (chain.hand_on_changes).  The new module hands its own changes on where it stands directly in front of a 1x1 /
    stride-1 / padding-0 CBConv2d; any other CBConv2d directly behind it needs its own input copy (copyInput) unless it
    runs in feedback mode.  A GLU over another dim, or behind anything else, stays the dense torch operator.  Returns
    rootModule."""
    def convert(glu):
        try:
            return CBGLU2d(glu) if type(glu) is nn.GLU else None
        except CBinferError:
            return None      # (over another dim: stays dense)
    return insert_behind_producers(rootModule, producers('insertCBGating'), convert, cloneOutput=cloneOutput)
