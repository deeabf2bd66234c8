"""Change-based element-wise operators of two maps: CBBinary2d, CBGLU2d, CBGated and insertCBGating (cb_binary.hip,
DESIGN 5.25).

The reference has no element-wise operator of two maps, and CBAdd2d is the sum alone: a gate `feat * sigmoid(gate)`, a
layer scale `gamma[c] * x`, a residual by difference `x - net(x)`, an element-wise maximum or an nn.GLU over the
channels ends a change-based chain -- the torch operator recomputes the whole map, drops both operands' change lists and
cannot be recorded by a FrameProgram.  Every producer of this package leaves the pixels outside its change list bit for
bit as they were, so op(a, b) can differ from last frame's only at the UNION of the two lists, and a constant operand (a
parameter) never changes: the modules here recompute it there and are the dense result exactly, without a threshold.
"""
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
                               % (name, op, ", ".join(repr(k) for k in _OPS)))
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
    state itself, tagged, and the frame is then free of torch operators."""

    def __init__(self, op, other=None, gate=None, reverse=False):
        super(CBBinary2d, self).__init__()
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

    def forward(self, a, b=None):
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
