"""Change-based rearrangements: CBPixelShuffle2d, CBChannelShuffle2d and insertCBRearrange (cb_rearrange.hip).

The reference has none of them: an nn.PixelShuffle -- the upsampler of ESPCN / EDSR-type super-resolution and restoration
networks and of many segmentation and depth heads --, an nn.PixelUnshuffle (space-to-depth) or an nn.ChannelShuffle -- the
middle of a ShuffleNet unit -- ends a change-based chain: torch rearranges the whole map, drops the producer's change mask
and cannot be recorded by a FrameProgram.  None of the three computes anything, and every producer of this package
leaves the pixels outside its change list bit for bit as they were, so the output can differ from last frame's only at
the FOOTPRINT of the input's changes on the output map: the modules copy there and are torch's dense result bit for bit,
without a threshold.
"""
import ctypes

import torch.nn as nn

from . import _lib
from ._lib import C, CBinferError, check, dtype_code, ptr, require_device, stream_ptr
from .chain import (EVERY_PIXEL, CBStateModule, check_map, form_args, insert_behind_producers, mask_workspace,
                    operand_changes, producers, split_operand)

MAX_FACTOR = 8      # of the two pixel shuffles: CBUpsample2d's scale limit


def _int_setting(name, what, v, lo, hi):
    """`v` as an int within lo..hi (hi None: no upper limit); CBinferError naming the setting otherwise."""
    if isinstance(v, bool) or not isinstance(v, int):
        raise CBinferError("%s: %s=%r is not supported, only an int" % (name, what, v))
    if v < lo or (hi is not None and v > hi):
        raise CBinferError("%s: %s=%r is beyond what the library takes (%d..%s)"
                           % (name, what, v, lo, hi if hi is not None else 'the channel count'))
    return v


class _CBRearrange2d(CBStateModule):
    """What the two modules share: the frame.  A subclass sets `kind` (_lib.REARRANGE_*), `factor` and NAME."""

    _TRANSIENT = ('_reC',)
    NAME = None

    def _struct(self):
        """(pointer to) the module's cbRearrange; transient, made again after unpickling."""
        if self.__dict__.get('_reC') is None:
            self.__dict__['_reC'] = ctypes.pointer(_lib.Rearrange(self.kind, self.factor))
        return self.__dict__['_reC']

    def _check_sizes(self, nc, Hi, Wi):
        """CBinferError naming the size of a [1, nc, Hi, Wi] input that the factor does not divide."""
        f = self.factor
        if self.kind == _lib.REARRANGE_SHUFFLE and nc % (f * f):
            raise CBinferError("%s: the input has %d channels, which upscale_factor^2 = %d does not divide"
                               % (self.NAME, nc, f * f))
        if self.kind == _lib.REARRANGE_UNSHUFFLE and (Hi % f or Wi % f):
            raise CBinferError("%s: the input is a %dx%d map, whose height and width downscale_factor = %d must divide"
                               % (self.NAME, Hi, Wi, f))
        if self.kind == _lib.REARRANGE_CHANNELS and nc % f:
            raise CBinferError("%s: the input has %d channels, which groups = %d does not divide" % (self.NAME, nc, f))

    def _out_shape(self, nc, Hi, Wi):
        """(Co, Ho, Wo) of a [1, nc, Hi, Wi] input."""
        self._check_sizes(nc, Hi, Wi)
        co, ho, wo = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        check(C.cbinfer_rearrange_out_shape(self._struct(), nc, Hi, Wi, ctypes.byref(co), ctypes.byref(ho),
                                            ctypes.byref(wo)))
        return co.value, ho.value, wo.value

    def _workspace(self, nc, Hi, Wi, dev):
        """Working mask (zero between frames), the frame's mask copy, index buffer and count on the OUTPUT map: once per
        input shape."""
        def make():
            Co, Ho, Wo = self._out_shape(nc, Hi, Wi)
            return dict(mask_workspace(Ho, Wo, dev), shape=(Co, Ho, Wo))
        return self._cached_work((nc, Hi, Wi, dev), make)

    def forward(self, inp):
        x, indexes = split_operand(self.NAME, inp, 'the input')
        check_map(self.NAME, x)
        nc, Hi, Wi = x.size(1), x.size(2), x.size(3)
        self._check_sizes(nc, Hi, Wi)
        require_device(x)
        work = self._workspace(nc, Hi, Wi, x.device)
        Co, Ho, Wo = work['shape']
        form = operand_changes(self.NAME, 'the input', indexes, Hi, Wi, x.device, work['idx'])
        if self._fresh_state((1, Co, Ho, Wo), x):      # (written completely: the change information is not used)
            form = EVERY_PIXEL
        check(C.cbinfer_cbrearrange_forward(ptr(x), ptr(self.outputState), *form_args(form), ptr(work['bits']),
                                            ptr(work['copy']), nc, Hi, Wi, self._struct(), dtype_code(x), stream_ptr(x)))
        return self._result(work, Ho, Wo)


class CBPixelShuffle2d(_CBRearrange2d):
    """nn.PixelShuffle or nn.PixelUnshuffle with a factor r of 1..8, copied at the output pixels that read a changed
    input pixel: shuffle [1, C r r, H, W] -> [1, C, H r, W r], unshuffle [1, C, H r, W r] -> [1, C r r, H, W].

    forward(x): a tensor -- no change information, every pixel is copied -- or the ('changeIndexes', tensor, indexes)
    tuple of a producer with propChangeIndexes.  A MaskChangeIndexes is taken as its mask (one launch, the list is not
    needed); any other ChangeIndexes, or an exact int32 tensor, as a list (one launch in front).  The flags are
    CBUpsample2d's: propChangeIndexes hands on the frame's footprint as a MaskChangeIndexes on the OUTPUT map;
    cloneOutput=False hands out the state itself, tagged, and the frame is then free of torch operators."""

    NAME = 'CBPixelShuffle2d'

    def __init__(self, m):
        super(CBPixelShuffle2d, self).__init__()
        if type(m) is nn.PixelShuffle:
            self.kind, what, v = _lib.REARRANGE_SHUFFLE, 'upscale_factor', m.upscale_factor
        elif type(m) is nn.PixelUnshuffle:
            self.kind, what, v = _lib.REARRANGE_UNSHUFFLE, 'downscale_factor', m.downscale_factor
        else:
            raise CBinferError("CBPixelShuffle2d: only nn.PixelShuffle and nn.PixelUnshuffle modules (exactly, not a "
                               "subclass) are converted, got %s" % type(m).__name__)
        self.factor = _int_setting(self.NAME, what, v, 1, MAX_FACTOR)
        self.__dict__['_reC'] = None

    @property
    def unshuffle(self):
        return self.kind == _lib.REARRANGE_UNSHUFFLE

    def __repr__(self):
        return 'CBPixelShuffle2d (%s=%d, propChgIdxs=%s)' % ('downscale_factor' if self.unshuffle else 'upscale_factor',
                                                            self.factor, self.propChangeIndexes)


class CBChannelShuffle2d(_CBRearrange2d):
    """nn.ChannelShuffle of g groups on a [1, C, H, W] map, g dividing C: out[k g + q] = in[q (C / g) + k], copied at the
    changed pixels.  forward and the flags are CBPixelShuffle2d's."""

    NAME = 'CBChannelShuffle2d'

    def __init__(self, m):
        super(CBChannelShuffle2d, self).__init__()
        if type(m) is not nn.ChannelShuffle:
            raise CBinferError("CBChannelShuffle2d: only nn.ChannelShuffle modules (exactly, not a subclass) are "
                               "converted, got %s" % type(m).__name__)
        self.kind = _lib.REARRANGE_CHANNELS
        self.factor = _int_setting(self.NAME, 'groups', m.groups, 1, None)
        self.__dict__['_reC'] = None

    @property
    def groups(self):
        return self.factor

    def __repr__(self):
        return 'CBChannelShuffle2d (groups=%d, propChgIdxs=%s)' % (self.factor, self.propChangeIndexes)


def insertCBRearrange(rootModule, cloneOutput=True):
    """Inside every nn.Sequential of rootModule, an nn.PixelShuffle, nn.PixelUnshuffle or nn.ChannelShuffle within the
    library's limits that directly follows a producer -- chain.producers('insertCBRearrange'), another
    CBPixelShuffle2d / CBChannelShuffle2d among them -- becomes the change-based module fed by that producer's changes:
    propChangeIndexes is switched on at the producer (chain.hand_on_changes).  The new module hands its own changes on
    where it stands directly in front of a 1x1 / stride-1 / padding-0 CBConv2d; any other CBConv2d consuming its output
    needs its own input copy (copyInput) unless it runs in feedback mode.  linkDepthwise, insertCBPointwise,
    insertCBUpsampling and insertCBTransposedConv, called afterwards, take the new modules as producers.  A module beyond
    the limits, or behind anything else, stays the dense torch operator.  Returns rootModule."""
    def convert(m):
        try:
            if type(m) in (nn.PixelShuffle, nn.PixelUnshuffle):
                return CBPixelShuffle2d(m)
            if type(m) is nn.ChannelShuffle:
                return CBChannelShuffle2d(m)
        except CBinferError:
            pass      # (beyond the limits: stays dense)
        return None
    return insert_behind_producers(rootModule, producers('insertCBRearrange'), convert, cloneOutput=cloneOutput)
