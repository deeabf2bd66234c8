"""Change-based reductions over the channels of one pixel: CBChannelReduce2d and insertCBChannelOps (cb_chanreduce.hip,
DESIGN 5.21; the kinds that collapse the channel axis: cb_chancollapse.hip).

The reference has no such operator: the channels-first LayerNorm of a ConvNeXt-type block, the nn.Softmax2d /
nn.Softmax(dim=1) / nn.LogSoftmax(dim=1) of a segmentation head and the F.normalize(x, dim=1) of a descriptor head stay
dense torch operators -- they recompute the whole map, drop the producer's change information and cannot be recorded by a
FrameProgram.  None of them is element-wise, but all are PIXEL-wise: the output at a pixel depends on the C values at
that pixel alone.  Every producer of this package leaves the pixels outside its change list bit for bit as they were, so
CBChannelReduce2d recomputes at the producer's changed pixels and is the dense result exactly, without a threshold.
Norms that also reduce over H x W (GroupNorm, InstanceNorm) do not have this property and are not taken.

The same holds for the reductions that COLLAPSE the channel axis: the label map of a segmentation head (the reference's
scene labelling ends every frame with torch.max(y.cpu(), 1)), the channel pooling of a spatial attention
(cat([x.mean(1, keepdim=True), x.amax(1, keepdim=True)], 1)), score and magnitude maps (x.amax(1), x.sum(1),
torch.linalg.vector_norm(x, dim=1)).  They are ops of the same module, named by strings.
"""
import numpy as np
import torch
import torch.nn as nn

from . import _lib
from ._lib import C, CBinferError, check, dtype_code, ptr, require_device, stream_ptr
from .chain import (EVERY_PIXEL, CBStateModule, check_map, form_args, hand_back, insert_behind_producers,
                    mask_workspace, operand_changes, producers, split_operand)

_AFFINE = ('gamma', 'beta')
_SOFTMAX = {nn.Softmax2d: _lib.CH_SOFTMAX, nn.Softmax: _lib.CH_SOFTMAX, nn.LogSoftmax: _lib.CH_LOGSOFTMAX}
KIND_NAMES = ('layernorm', 'l2norm', 'softmax', 'logsoftmax')
# the ops that collapse the channel axis (CB_CC_*): five value kinds, 1 .. 4 of them per module, and two arg kinds
COLLAPSE = {'sum': _lib.CC_SUM, 'mean': _lib.CC_MEAN, 'norm': _lib.CC_NORM, 'max': _lib.CC_MAX, 'min': _lib.CC_MIN,
            'argmax': _lib.CC_ARGMAX, 'argmin': _lib.CC_ARGMIN}
ARG_OPS = ('argmax', 'argmin')


def _collapse_ops(op, eps, keepdim, labelChanges):
    """(names, packed kinds) of a collapsing op -- one of COLLAPSE's strings or a tuple of 1 .. 4 value strings --, or
    None where `op` is none of them; what does not go with them is refused by name."""
    names = (op,) if isinstance(op, str) and op in COLLAPSE else op if isinstance(op, tuple) else None
    if names is None:
        return None
    if not 1 <= len(names) <= 4:
        raise CBinferError("CBChannelReduce2d: op=%r has %d entries, a tuple names 1 to 4 value ops" % (op, len(names)))
    for n in names:
        if not isinstance(n, str) or n not in COLLAPSE or (n in ARG_OPS and isinstance(op, tuple)):
            raise CBinferError("CBChannelReduce2d: op=%r: %r is not one of the value ops 'sum', 'mean', 'norm', 'max', "
                               "'min' a tuple may name ('argmax' / 'argmin' stand alone, as a string)" % (op, n))
    if eps is not None:
        raise CBinferError("CBChannelReduce2d: eps=%r given for op=%r, which has none" % (eps, op))
    if isinstance(op, tuple) and not keepdim:
        raise CBinferError("CBChannelReduce2d: keepdim=False with the tuple op=%r: its ops are the channels of the output"
                           % (op,))
    if labelChanges and names[0] not in ARG_OPS:
        raise CBinferError("CBChannelReduce2d: labelChanges=True with op=%r: only 'argmax' and 'argmin' have labels"
                           % (op,))
    packed = sum(COLLAPSE[n] << (4 * k) for k, n in enumerate(names))
    if not C.cbinfer_chancollapse_supported(packed, len(names), 1):
        raise CBinferError("CBChannelReduce2d: op=%r is not supported by the library (kinds 0x%x, %d ops)"
                           % (op, packed, len(names)))
    return tuple(names), packed


def _f32_vector(t, name):
    """A detached float32 copy [C] of a parameter (an fp16 parameter converts exactly), or None."""
    if t is None:
        return None
    if not torch.is_tensor(t) or t.dim() != 1:
        raise CBinferError("CBChannelReduce2d: op.%s must be a one-dimensional tensor or None" % name)
    return t.detach().float().clone()


def _layer_norm(op, eps):
    """(gamma, beta, eps) of a layer norm over the channel axis: an nn.LayerNorm over (C,), or a channels-first class of
    the user's with .weight, .bias (or None) and .eps."""
    if type(op) is nn.LayerNorm and len(op.normalized_shape) != 1:
        raise CBinferError("CBChannelReduce2d: op=%r normalises over normalized_shape=%s: only a LayerNorm over (C,), "
                           "read as a normalisation over the channel axis, is a per-pixel operator"
                           % (op, tuple(op.normalized_shape)))
    gamma, beta = _f32_vector(getattr(op, 'weight', None), 'weight'), _f32_vector(getattr(op, 'bias', None), 'bias')
    if gamma is None and beta is not None:
        raise CBinferError("CBChannelReduce2d: op=%r has a bias but no weight" % (op,))
    if gamma is not None and beta is None:
        beta = torch.zeros_like(gamma)      # (nn.LayerNorm(bias=False): adding +0 changes no value but a -0)
    if gamma is not None and gamma.numel() != beta.numel():
        raise CBinferError("CBChannelReduce2d: op.weight has %d values, op.bias %d" % (gamma.numel(), beta.numel()))
    return gamma, beta.to(gamma.device) if gamma is not None else None, (op.eps if eps is None else eps)


class CBChannelReduce2d(CBStateModule):
    """A reduction over the channel axis at every pixel, recomputed at the operand's changed pixels (no counterpart in the
    reference).

    op: an nn.Softmax2d; an nn.Softmax or nn.LogSoftmax with dim 1 or -3; an nn.LayerNorm whose normalized_shape is (C,),
    read as a normalisation over the channel axis of the [1, C, H, W] map (it supplies weight, bias and eps;
    elementwise_affine=False: no gamma / beta); or the string 'l2norm' (F.normalize(x, p=2, dim=1, eps), eps 1e-12 by
    default).  The types are taken exactly, not by subclass; layerNormTypes names further -- channels-first --
    layer-norm classes of the user's, exact types with .weight, .bias (or None) and .eps.  eps overrides the operator's.

    The ops that collapse the channel axis are strings: 'sum', 'mean', 'norm' (torch.linalg.vector_norm over
    dim 1), 'max', 'min' (torch.max / torch.min(x, 1).values), or a tuple of 1 .. 4 of these, computed from ONE pass -- the
    state is [1, K, H, W] in the operand's dtype, channel k is op k, ('mean', 'max') is CBAM's channel pooling --; and
    'argmax' / 'argmin' (torch's, bit for bit: the first of equal values, a NaN beats every number), whose state is an
    int64 label map [1, 1, H, W].  keepdim=False (a single op, not a tuple) drops the channel axis: [1, H, W].  They take
    no eps.  sum, mean and norm are the float32 specification of DESIGN 5.27 bit for bit, the other four are torch's
    CPU results bit for bit.  labelChanges=True
    (arg ops only): with propChangeIndexes the module hands on, instead of the frame's mask, the mask of the listed
    pixels whose LABEL differs from last frame's -- a consumer of the label map then sees only those, and the handed-on
    indexes give their list.  No float consumer of this package takes an int64 map: they refuse it by its dtype.
    gamma / beta are copied HERE and kept as float32 buffers (pickled, moved by .to(), kept float32 by .half()): later
    edits of the source module are not followed.  LayerNorm and the L2 norm are the float32 specification of DESIGN 5.21
    bit for bit; the softmax kinds call the device's expf / logf (the bound is there).

    forward(x), propChangeIndexes and cloneOutput are CBPointwise2d's: a bare tensor carries no change information, a
    MaskChangeIndexes is taken as its mask, any other ChangeIndexes or an int32 tensor as a list; the first frame or a new
    shape recomputes every pixel."""

    _WORK = '_chWork'

    def __init__(self, op, eps=None, layerNormTypes=(), keepdim=True, labelChanges=False):
        super(CBChannelReduce2d, self).__init__()
        gamma = beta = None
        self.opName = op if isinstance(op, str) else '+'.join(map(str, op)) if isinstance(op, tuple) else type(op).__name__
        collapse = _collapse_ops(op, eps, keepdim, labelChanges)
        # (read with a default everywhere: a module pickled before these existed has none of them)
        self.collapseOps, self.keepdim, self.labelChanges = collapse, bool(keepdim), bool(labelChanges)
        if collapse is not None:
            self.kind, eps = None, 0.0
        elif not keepdim or labelChanges:
            raise CBinferError("CBChannelReduce2d: %s with op=%s: only the ops that collapse the channel axis take it"
                               % ("keepdim=False" if not keepdim else "labelChanges=True", self.opName))
        elif isinstance(op, str):
            if op != 'l2norm':
                raise CBinferError("CBChannelReduce2d: op=%r is not supported, of the strings only 'l2norm' and the "
                                   "collapsing %s" % (op, ', '.join(repr(n) for n in COLLAPSE)))
            self.kind, eps = _lib.CH_L2NORM, (1e-12 if eps is None else eps)
        elif type(op) in _SOFTMAX:
            dim = 1 if type(op) is nn.Softmax2d else op.dim
            if dim not in (1, -3):
                raise CBinferError("CBChannelReduce2d: op=%r reduces over dim=%r: only dim=1 (or -3), the channel axis "
                                   "of a [1, C, H, W] map, is a per-pixel operator" % (op, dim))
            if eps is not None:
                raise CBinferError("CBChannelReduce2d: eps=%r given for op=%s, which has none" % (eps, self.opName))
            self.kind, eps = _SOFTMAX[type(op)], 0.0
        elif type(op) is nn.LayerNorm or type(op) in tuple(layerNormTypes):
            self.kind = _lib.CH_LAYERNORM
            gamma, beta, eps = _layer_norm(op, eps)
        else:
            raise CBinferError("CBChannelReduce2d: op=%s is not supported, only an instance of exactly nn.Softmax2d, "
                               "nn.Softmax, nn.LogSoftmax, nn.LayerNorm (or one of layerNormTypes), or 'l2norm'"
                               % self.opName)
        try:
            self.eps = float(np.float32(eps))      # (the kernel's value: rounded to f32 once)
        except (TypeError, ValueError):
            raise CBinferError("CBChannelReduce2d: eps=%r is not a number" % (eps,))
        if collapse is None and not C.cbinfer_chanreduce_supported(self.kind, 1, self.eps):
            raise CBinferError("CBChannelReduce2d: eps=%r must be a number >= 0" % (eps,))
        for name, t in zip(_AFFINE, (gamma, beta)):
            self.register_buffer(name, t)
        # (the state behind the per-channel operands, as CBPointwise2d lists them)
        self._buffers['outputState'] = self._buffers.pop('outputState')

    def _apply(self, fn, *args, **kwargs):
        # (.half() / .double() convert every floating-point buffer: gamma / beta stay float32, the kernel's)
        keep = {n: self._buffers[n] for n in _AFFINE if self._buffers.get(n) is not None}
        super(CBChannelReduce2d, self)._apply(fn, *args, **kwargs)
        for n, t in keep.items():
            if self._buffers[n].dtype != torch.float32:
                self._buffers[n] = t.to(self._buffers[n].device)
        return self

    def _workspace(self, nc, H, W, dev):
        """Working mask (zero between frames), the frame's mask copy, index buffer and count: once per map size."""
        return self._cached_work((nc, H, W, dev), lambda: mask_workspace(H, W, dev))

    def _collapse_forward(self, collapse, x, indexes):
        """A frame of a collapsing op: the state has its own shape and, for the arg ops, its own dtype."""
        names, packed = collapse
        nc, H, W = x.size(1), x.size(2), x.size(3)
        require_device(x)
        arg, label = names[0] in ARG_OPS, self.__dict__.get('labelChanges', False)

        def make():      # (the label mask lives with the other masks)
            work = mask_workspace(H, W, x.device)
            if label:
                work['label'] = torch.zeros_like(work['copy'])
            return work
        before = self.__dict__.get(self._WORK)
        work = self._cached_work((nc, H, W, x.device, x.dtype, label), make)
        form = operand_changes('CBChannelReduce2d', 'the input', indexes, H, W, x.device, work['idx'])
        # (keepdim=False is a single op's: the constructor refuses it for a tuple)
        shape = (1, len(names), H, W) if self.__dict__.get('keepdim', True) else (1, H, W)
        dtype = torch.int64 if arg else x.dtype
        state = self.outputState
        if tuple(state.shape) != shape or state.dtype != dtype or state.device != x.device:
            self.outputState = state = torch.empty(shape, dtype=dtype, device=x.device)
            form = EVERY_PIXEL      # (written completely: the operand's change information is not used)
        elif work is not before:
            form = EVERY_PIXEL      # (an operand of another shape or dtype behind a state that happens to fit)
        check(C.cbinfer_cbchancollapse_forward(ptr(x), ptr(state), *form_args(form), ptr(work['bits']),
                                               ptr(work['copy']), ptr(work.get('label')), nc, H, W, packed, len(names),
                                               dtype_code(x), stream_ptr(x)))
        # (labelChanges: the narrower mask is what the consumer is handed)
        return hand_back(self, state, work['label'] if label else work['copy'], (H, W), work)

    def forward(self, inp):
        x, indexes = split_operand('CBChannelReduce2d', inp, 'the input')
        check_map('CBChannelReduce2d', x)
        collapse = self.__dict__.get('collapseOps')
        if collapse is not None:
            return self._collapse_forward(collapse, x, indexes)
        nc, H, W = x.size(1), x.size(2), x.size(3)
        if self.gamma is not None and self.gamma.numel() != nc:
            raise CBinferError("CBChannelReduce2d: the input has %d channels, gamma was made for %d"
                               % (nc, self.gamma.numel()))
        require_device(x)
        if self.gamma is not None and self.gamma.device != x.device:
            raise CBinferError("CBChannelReduce2d: the input is on %s, gamma on %s (move the module with .to())"
                               % (x.device, self.gamma.device))
        work = self._workspace(nc, H, W, x.device)
        form = operand_changes('CBChannelReduce2d', 'the input', indexes, H, W, x.device, work['idx'])
        if self._fresh_state(x.shape, x):      # (written completely: the operand's change information is not used)
            form = EVERY_PIXEL
        check(C.cbinfer_cbchanreduce_forward(ptr(x), ptr(self.outputState), *form_args(form), ptr(work['bits']),
                                             ptr(work['copy']), nc, H, W, self.kind, self.eps, ptr(self.gamma),
                                             ptr(self.beta), dtype_code(x), stream_ptr(x)))
        return self._result(work, H, W)

    def __repr__(self):
        collapse = self.__dict__.get('collapseOps')
        if collapse is not None:
            return 'CBChannelReduce2d (op=%s, ops=%s, keepdim=%s, labelChanges=%s, propChgIdxs=%s)' % (
                self.opName, ','.join(collapse[0]), self.__dict__.get('keepdim', True),
                self.__dict__.get('labelChanges', False), self.propChangeIndexes)
        return 'CBChannelReduce2d (op=%s, kind=%s, eps=%s, affine=%s, propChgIdxs=%s)' % (
            self.opName, KIND_NAMES[self.kind], self.eps, self.gamma is not None, self.propChangeIndexes)


def insertCBChannelOps(rootModule, layerNormTypes=(), reduceTypes=None):
    """Inside every nn.Sequential of rootModule, an nn.Softmax2d, an nn.Softmax / nn.LogSoftmax over dim 1 (or -3), or an
    instance of one of layerNormTypes -- the user's channels-first layer-norm classes, exact types with .weight, .bias (or
    None) and .eps, as ConvNeXt's LayerNorm2d; torch has no such class of its own -- that directly follows a producer
    (chain.producers('insertCBChannelOps'), another CBChannelReduce2d among them) becomes a
    CBChannelReduce2d under the same name, fed by that producer's changes: propChangeIndexes is switched on at the
    producer (chain.hand_on_changes).  The new module hands its own changes on where it stands directly in front of a
    1x1 / stride-1 / padding-0 CBConv2d; any other CBConv2d directly behind it needs its own input copy (copyInput)
    unless it runs in feedback mode, as insertCBRearrange has it.  Anything else -- a softmax over another axis, a module
    behind a dense operator -- stays dense.  linkDepthwise, insertCBPointwise, insertCBUpsampling, insertCBTransposedConv,
    insertCBRearrange and the general pools do not take the new module as a producer (chain.PRODUCERS).

    reduceTypes: a dict from a module class of the user's to a collapsing op of CBChannelReduce2d -- torch has no module
    for x.mean(1, keepdim=True), torch.argmax(x, 1) and their like --, e.g. {ChannelPool: ('max', 'mean'),
    ArgMax2d: 'argmax'}; an instance of exactly such a class (keepdim=True) becomes a CBChannelReduce2d with that op.
    Returns rootModule."""
    layerNormTypes = tuple(layerNormTypes)
    reduceTypes = dict(reduceTypes or {})

    def convert(op):
        if type(op) in reduceTypes:
            return CBChannelReduce2d(reduceTypes[type(op)])      # (what it refuses of the op is raised)
        if type(op) in _SOFTMAX:
            if type(op) is not nn.Softmax2d and op.dim not in (1, -3):
                return None
        elif type(op) not in layerNormTypes:
            return None
        return CBChannelReduce2d(op, layerNormTypes=layerNormTypes)      # (what it refuses of a layer norm is raised)
    return insert_behind_producers(rootModule, producers('insertCBChannelOps'), convert)
