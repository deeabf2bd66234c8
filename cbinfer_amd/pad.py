"""Change-based padding: CBPad2d, insertCBPadding and splitConvPadding (cb_pad.hip).

The reference has no padding operator: an nn.ReflectionPad2d, nn.ReplicationPad2d, nn.ZeroPad2d, nn.ConstantPad2d or
nn.CircularPad2d -- every 3x3 layer of a monodepth2-type depth decoder, the stems and residual blocks of style-transfer
and image-to-image generators, the asymmetric ZeroPad2d((0, 1, 0, 1)) of TF-ported backbones, a U-Net skip cropped with a
negative pad -- ends a change-based chain: torch pads the whole map, drops the producer's change mask and cannot be
recorded by a FrameProgram; an nn.Conv2d with padding_mode 'reflect', 'replicate' or 'circular' is refused by the
convolution modules by name.  A pad computes nothing, and every producer of this package leaves the pixels outside its
change list bit for bit as they were, so the output can differ from last frame's only at the FOOTPRINT of the input's
changes on the output map: the module copies there and is torch's dense result bit for bit, without a threshold.
splitConvPadding turns a padding_mode convolution into what torch itself runs for it -- the pad module and a zero-padding
convolution -- so that convert() and insertCBPadding take both.
"""
import ctypes
import math

import torch
import torch.nn as nn

from . import _lib
from ._lib import C, CBinferError, check, dtype_code, ptr, require_device, stream_ptr
from .chain import (EVERY_PIXEL, CBStateModule, check_map, form_args, insert_behind_producers, mask_workspace,
                    operand_changes, producers, split_operand)

MAX_PAD = 64      # per side, either sign: cbGeom's padding bound
MODES = {'constant': _lib.PAD_CONSTANT, 'reflect': _lib.PAD_REFLECT, 'replicate': _lib.PAD_REPLICATE,
         'circular': _lib.PAD_CIRCULAR}
# the torch modules and the F.pad mode each stands for (ZeroPad2d derives from ConstantPad2d and counts as itself)
PAD_MODULES = {nn.ReflectionPad2d: 'reflect', nn.ReplicationPad2d: 'replicate', nn.ZeroPad2d: 'constant',
               nn.ConstantPad2d: 'constant', nn.CircularPad2d: 'circular'}
_FINITE_MAX = {torch.float16: 65504.0, torch.float32: 3.4028234663852886e38}


def _pads(padding):
    """`padding` (an int or four ints in torch's (left, right, top, bottom) order) as a 4-tuple of ints."""
    def whole(v):
        return isinstance(v, int) and not isinstance(v, bool)
    if whole(padding):
        return (padding,) * 4
    if isinstance(padding, (tuple, list)) and len(padding) in (2, 6) and all(whole(v) for v in padding):
        raise CBinferError("CBPad2d: padding=%r pads %d dimension%s, only 2-d pads (left, right, top, bottom) are supported"
                           % (tuple(padding), len(padding) // 2, '' if len(padding) == 2 else 's'))
    if not (isinstance(padding, (tuple, list)) and len(padding) == 4 and all(whole(v) for v in padding)):
        raise CBinferError("CBPad2d: padding=%r is not supported, only an int or four ints (left, right, top, bottom)"
                           % (padding,))
    return tuple(padding)


class CBPad2d(CBStateModule):
    """F.pad(x, (left, right, top, bottom), mode, value) of a [1, C, H, W] map with every |pad| <= 64, mode 'constant'
    (negative pads crop), 'reflect', 'replicate' or 'circular', copied at the output pixels that read a changed input
    pixel.

    CBPad2d(m) takes an nn.ReflectionPad2d / nn.ReplicationPad2d / nn.ZeroPad2d / nn.ConstantPad2d / nn.CircularPad2d
    (exactly, not a subclass); CBPad2d(padding=..., mode=..., value=...) F.pad's keywords, padding an int or four ints.
    forward(x): a tensor -- no change information, every pixel is written -- or the ('changeIndexes', tensor, indexes)
    tuple of a producer with propChangeIndexes.  A MaskChangeIndexes is taken as its mask (one launch, the list is not
    needed); any other ChangeIndexes, or an exact int32 tensor, as a list (one launch in front).  A constant-mode border
    pixel reads no input: it is written when the state is (the first frame, a new resolution, after clearMemory) and
    keeps its value.  The flags are CBUpsample2d's: propChangeIndexes hands on the frame's footprint as a
    MaskChangeIndexes on the OUTPUT map; cloneOutput=False hands out the state itself, tagged, and the frame is then free
    of torch operators.  What depends on the map -- reflect needs every pad below the extent of its axis, circular not
    above it, the output at least 1x1, a value the frame's dtype holds -- is refused at the first frame."""

    _TRANSIENT = ('_pdC',)

    def __init__(self, m=None, padding=None, mode='constant', value=0.0):
        super(CBPad2d, self).__init__()
        if m is not None:
            if type(m) not in PAD_MODULES:
                raise CBinferError("CBPad2d: only nn.ReflectionPad2d, nn.ReplicationPad2d, nn.ZeroPad2d, nn.ConstantPad2d "
                                   "and nn.CircularPad2d modules are converted (exactly, not a subclass), got %s"
                                   % type(m).__name__)
            if padding is not None or mode != 'constant' or not (isinstance(value, float) and value == 0.0):
                raise CBinferError("CBPad2d: give a module or padding / mode / value, not both")
            padding, mode = m.padding, PAD_MODULES[type(m)]
            value = getattr(m, 'value', 0.0) if mode == 'constant' else 0.0
        if not isinstance(mode, str) or mode not in MODES:
            raise CBinferError("CBPad2d: mode=%r is not supported, only 'constant', 'reflect', 'replicate' and 'circular'"
                               % (mode,))
        if padding is None:
            raise CBinferError("CBPad2d: padding=None is not supported, only an int or four ints (left, right, top, "
                               "bottom)")
        self.padding = _pads(padding)
        if max(abs(v) for v in self.padding) > MAX_PAD:
            raise CBinferError("CBPad2d: padding=%r is beyond what the library takes (-%d..%d per side)"
                               % (self.padding, MAX_PAD, MAX_PAD))
        if mode != 'constant' and min(self.padding) < 0:
            raise CBinferError("CBPad2d: padding=%r with mode=%r is not supported: a negative pad (cropping) is taken in "
                               "mode 'constant' only" % (self.padding, mode))
        if isinstance(value, bool) or not isinstance(value, (int, float)):
            raise CBinferError("CBPad2d: value=%r is not supported, only a float (or an int, taken as one)" % (value,))
        self.mode = mode
        self.value = float(value)
        self.__dict__['_pdC'] = None

    def _struct(self):
        """(pointer to) the module's cbPad; transient, made again after unpickling."""
        if self.__dict__.get('_pdC') is None:
            self.__dict__['_pdC'] = ctypes.pointer(_lib.Pad(MODES[self.mode], *(self.padding + (self.value,))))
        return self.__dict__['_pdC']

    def out_size(self, H, W):
        """(Ho, Wo) of an H x W map; CBinferError naming the map where the padding does not fit it."""
        left, right, top, bottom = self.padding
        said = "CBPad2d: padding=%r with mode=%r of a %dx%d map" % (self.padding, self.mode, H, W)
        if self.mode == 'reflect' and (max(left, right) >= W or max(top, bottom) >= H):
            raise CBinferError("%s: reflection needs every pad below the extent of its axis" % said)
        if self.mode == 'circular' and (max(left, right) > W or max(top, bottom) > H):
            raise CBinferError("%s: circular padding wraps around once at most, no pad may exceed the extent of its axis"
                               % said)
        if H + top + bottom < 1 or W + left + right < 1:
            raise CBinferError("%s leaves no output pixel" % said)
        ho, wo = ctypes.c_int(), ctypes.c_int()
        check(C.cbinfer_pad_out_size(self._struct(), H, W, ctypes.byref(ho), ctypes.byref(wo)))
        return ho.value, wo.value

    def _workspace(self, nc, H, W, dev):
        """Working mask (zero between frames), the frame's mask copy, index buffer and count on the OUTPUT map: once per
        input shape."""
        def make():
            Ho, Wo = self.out_size(H, W)
            return dict(mask_workspace(Ho, Wo, dev), size=(Ho, Wo))
        return self._cached_work((nc, H, W, dev), make)

    def forward(self, inp):
        x, indexes = split_operand('CBPad2d', inp, 'the input')
        check_map('CBPad2d', x, note=' (batch 1)')
        nc, H, W = x.size(1), x.size(2), x.size(3)
        if self.mode == 'constant' and math.isfinite(self.value) and abs(self.value) > _FINITE_MAX[x.dtype]:
            raise CBinferError("CBPad2d: value=%r of a %dx%d %s map overflows the tensor's dtype"
                               % (self.value, H, W, str(x.dtype).replace('torch.', '')))
        require_device(x)
        work = self._workspace(nc, H, W, x.device)
        Ho, Wo = work['size']
        form = operand_changes('CBPad2d', 'the input', indexes, H, W, x.device, work['idx'])
        if self._fresh_state((1, nc, Ho, Wo), x):      # (written completely: the change information is not used)
            form = EVERY_PIXEL
        check(C.cbinfer_cbpad_forward(ptr(x), ptr(self.outputState), *form_args(form), ptr(work['bits']),
                                      ptr(work['copy']), nc, H, W, self._struct(), dtype_code(x), stream_ptr(x)))
        return self._result(work, Ho, Wo)

    def __repr__(self):
        return 'CBPad2d (padding=%s, mode=%s, value=%s, propChgIdxs=%s)' % (self.padding, self.mode, self.value,
                                                                           self.propChangeIndexes)


# ---------------------------------------------------------------------------------------------------- passes
_SPLIT_MODULES = {'reflect': nn.ReflectionPad2d, 'replicate': nn.ReplicationPad2d, 'circular': nn.CircularPad2d}


def _conv_pads(conv):
    """(pH, pW) of an nn.Conv2d whose padding splitConvPadding takes -- ints, or 'same' with an even total per axis --,
    else None."""
    if isinstance(conv.padding, str):
        if conv.padding != 'same':
            return None
        totals = [d * (k - 1) for d, k in zip(conv.dilation, conv.kernel_size)]
        return None if any(t % 2 for t in totals) else tuple(t // 2 for t in totals)
    pads = tuple(conv.padding)
    if len(pads) != 2 or not all(isinstance(v, int) and not isinstance(v, bool) for v in pads):
        return None
    return pads


def splitConvPadding(rootModule):
    """Call before convert(), like foldBatchNorm.  Inside every nn.Sequential of rootModule an nn.Conv2d (exactly) whose
    padding_mode is 'reflect', 'replicate' or 'circular' and whose padding is ints -- or 'same' with an even total per
    axis -- becomes what torch's own forward of such a layer runs: the matching pad module (nn.ReflectionPad2d /
    nn.ReplicationPad2d / nn.CircularPad2d with (pW, pW, pH, pH)) under the new name '<name>_pad', directly in front of
    a NEW nn.Conv2d with padding=0 and padding_mode='zeros' under the old name, which shares the weight and bias
    Parameter objects.  On dense torch the split network equals the original bit for bit, and its state_dict keeps its
    keys; afterwards convert(..., generalGeometry=True) takes the convolution and insertCBPadding the pad.  A layer with
    an odd-total 'same' is left alone (and convert() still refuses it by name).  CBinferError if '<name>_pad' is taken.
    Returns rootModule."""
    for seq in [m for m in rootModule.modules() if type(m) is nn.Sequential]:
        rebuilt = {}
        for name, child in seq._modules.items():
            pads = _conv_pads(child) if type(child) is nn.Conv2d and child.padding_mode in _SPLIT_MODULES else None
            if pads is None:
                rebuilt[name] = child
                continue
            padName = name + '_pad'
            if padName in seq._modules:
                raise CBinferError("splitConvPadding: the pad of layer %r needs the name %r, which another child of its "
                                   "container has" % (name, padName))
            conv = nn.Conv2d(child.in_channels, child.out_channels, child.kernel_size, child.stride, 0, child.dilation,
                             child.groups, child.bias is not None, 'zeros', device='meta')
            conv.weight, conv.bias = child.weight, child.bias      # (the same Parameter objects)
            conv.train(child.training)
            rebuilt[padName] = _SPLIT_MODULES[child.padding_mode]((pads[1], pads[1], pads[0], pads[0]))
            rebuilt[name] = conv
        seq._modules.clear()
        seq._modules.update(rebuilt)
    return rootModule


def insertCBPadding(rootModule, cloneOutput=True):
    """Inside every nn.Sequential of rootModule, an nn.ReflectionPad2d, nn.ReplicationPad2d, nn.ZeroPad2d,
    nn.ConstantPad2d or nn.CircularPad2d within the library's limits that directly follows a producer --
    chain.producers('insertCBPadding'), another CBPad2d among them -- becomes a CBPad2d
    fed by that producer's changes: propChangeIndexes is switched on at the producer (chain.hand_on_changes).  The new
    module hands its own changes on where it stands directly in front of a 1x1 / stride-1 / padding-0 CBConv2d; any other
    CBConv2d directly behind it needs its own input copy (copyInput) unless it runs in feedback mode.  A module beyond the
    limits, or behind anything else -- a pad at the front of a network has no producer; build a CBPad2d stem by hand --,
    stays the dense torch operator; the limits that depend on the map show at the first frame.  Returns rootModule."""
    def convert(m):
        try:
            return CBPad2d(m) if type(m) in PAD_MODULES else None
        except CBinferError:
            return None      # (beyond the limits: stays dense)
    return insert_behind_producers(rootModule, producers('insertCBPadding'), convert, cloneOutput=cloneOutput)
