"""Change-based resize to any size: CBResize2d and insertCBResize (cb_resize.hip).

CBUpsample2d takes an integer scale_factor and nothing else; real decoders resize to a SIZE -- DeepLab / FCN / PSPNet
heads to the image, FPN and HRNet steps to a skip's size (odd extents make the ratio fractional), HRNet's fuse layers and
image pyramids downwards, depth and super-resolution heads with bicubic.  An output pixel reads 1, 2x2 or 4x4 input pixels
at coordinates that are a rational function of its own, and every producer of this package leaves the pixels outside its
change list bit for bit as they were, so the module recomputes at the FOOTPRINT of the input's changes and is the dense
result exactly, without a threshold.

The source coordinates are derived in INTEGERS from the step a / b (include/cbinfer_hip.h, the specification) and the
f32 arithmetic is written out operation by operation: the module equals its numpy twin bit for bit.  torch derives the
coordinates from a float scale, so bilinear and bicubic follow F.interpolate to about 1e-5; the nearest kinds are
bit-identical to torch.
"""
import ctypes
import fractions
import math

import torch
import torch.nn as nn

from . import _lib
from ._lib import C, CBinferError, check, dtype_code, ptr, require_device, stream_ptr
from .chain import (EVERY_PIXEL, CBStateModule, check_map, form_args, insert_behind_producers, mask_workspace,
                    operand_changes, producers, split_operand)

MAX_RATIO = 8          # per axis, either way
MAX_TERM = 4096        # numerator and denominator of the reduced step
MODES = {'nearest': _lib.RESIZE_NEAREST, 'nearest-exact': _lib.RESIZE_NEAREST_EXACT, 'bilinear': _lib.RESIZE_BILINEAR,
         'bicubic': _lib.RESIZE_BICUBIC}
_UPSAMPLERS = (nn.Upsample, nn.UpsamplingNearest2d, nn.UpsamplingBilinear2d)


def _pair(name, v, kind):
    """`v` (a number or a pair of them) as a pair of `kind` (int: a size; float: a scale)."""
    pair = tuple(v) if isinstance(v, (tuple, list, torch.Size)) else (v, v)
    ok = len(pair) == 2 and all(isinstance(e, (int, float)) and not isinstance(e, bool) for e in pair)
    if ok and kind is int:
        ok = all(isinstance(e, int) and e >= 1 for e in pair)
    if ok and kind is float:
        ok = all(math.isfinite(e) and e > 0 for e in pair)
    if not ok:
        raise CBinferError("CBResize2d: %s=%r is not supported, only a positive %s or a pair of them (2-d maps)"
                           % (name, v, 'integer' if kind is int else 'number'))
    return tuple(kind(e) for e in pair)


def axis_step(n, size, scale, recompute):
    """(N, a, b) of one axis of n input pixels as torch defines them: the output extent and the reduced step a / b in
    input pixels per output pixel.  size, or recompute_scale_factor: a / b = n / N; a scale_factor without recompute:
    N = floor(n sf) and a / b = 1 / sf from fractions.Fraction(sf) -- a float is an exact rational."""
    if size is not None:
        N = size
    else:
        N = int(math.floor(float(n) * scale))
        if not recompute:
            step = 1 / fractions.Fraction(scale)
            return N, step.numerator, step.denominator
    step = fractions.Fraction(n, max(N, 1))
    return N, step.numerator, step.denominator


class CBResize2d(CBStateModule):
    """F.interpolate(x, size / scale_factor, mode, align_corners) to any size within a ratio of 8 per axis, up or down:
    mode 'nearest', 'nearest-exact', 'bilinear' or 'bicubic' (align_corners False or True with the last two), recomputed at
    the output pixels that read a changed input pixel.

    CBResize2d(m) takes an nn.Upsample / nn.UpsamplingNearest2d / nn.UpsamplingBilinear2d (exactly, not a subclass);
    CBResize2d(size=..., scale_factor=..., mode=..., align_corners=..., recompute_scale_factor=...) F.interpolate's
    keywords.  forward(x, size=None): x as CBUpsample2d takes it -- a [1, C, Hi, Wi] tensor (every pixel is recomputed) or
    the ('changeIndexes', tensor, indexes) tuple of a producer --; a `size` given here overrides the constructor's for
    this call, as F.interpolate(x, size=skip.shape[-2:]) does.  The state is rebuilt, written completely, when the output
    size changes.  The flags propChangeIndexes and cloneOutput are CBUpsample2d's."""

    _TRANSIENT = ('_rsC',)

    def __init__(self, m=None, size=None, scale_factor=None, mode='nearest', align_corners=None,
                 recompute_scale_factor=None, antialias=False):
        super(CBResize2d, self).__init__()
        Err = CBinferError
        if m is not None:
            if type(m) not in _UPSAMPLERS:
                raise Err("CBResize2d: only nn.Upsample, nn.UpsamplingNearest2d and nn.UpsamplingBilinear2d modules are "
                          "converted (exactly, not a subclass), got %s" % type(m).__name__)
            if size is not None or scale_factor is not None:
                raise Err("CBResize2d: give a module or size / scale_factor, not both")
            size, scale_factor, mode, align_corners = m.size, m.scale_factor, m.mode, m.align_corners
            recompute_scale_factor = getattr(m, 'recompute_scale_factor', None)
        if antialias:
            raise Err("CBResize2d: antialias=%r is not supported" % (antialias,))
        if mode not in MODES:
            raise Err("CBResize2d: mode=%r is not supported, only 'nearest', 'nearest-exact', 'bilinear' and 'bicubic'"
                      % (mode,))
        if mode in ('nearest', 'nearest-exact') and align_corners is not None:
            raise Err("CBResize2d: align_corners=%r has no meaning with mode=%r" % (align_corners, mode))
        if size is not None and scale_factor is not None:
            raise Err("CBResize2d: only one of size=%r and scale_factor=%r may be given" % (size, scale_factor))
        if size is not None and recompute_scale_factor:
            raise Err("CBResize2d: recompute_scale_factor=%r has no meaning with size=%r" % (recompute_scale_factor, size))
        self.size = None if size is None else _pair('size', size, int)
        self.scale_factor = None if scale_factor is None else _pair('scale_factor', scale_factor, float)
        for sf in self.scale_factor or ():
            step = 1 / fractions.Fraction(sf)
            if sf > MAX_RATIO or sf * MAX_RATIO < 1:
                raise Err("CBResize2d: scale_factor=%r is beyond what the library takes (a ratio of 1/%d .. %d per axis)"
                          % (scale_factor, MAX_RATIO, MAX_RATIO))
            if not recompute_scale_factor and max(step.numerator, step.denominator) > MAX_TERM:
                raise Err("CBResize2d: scale_factor=%r is not supported: as an exact rational it is %s, beyond %d in "
                          "numerator or denominator (use size= or recompute_scale_factor=True)"
                          % (scale_factor, fractions.Fraction(sf), MAX_TERM))
        self.mode = mode
        self.align_corners = bool(align_corners)
        self.recompute_scale_factor = bool(recompute_scale_factor)
        self.__dict__['_rsC'] = None

    def geometry(self, Hi, Wi, size=None):
        """(Ho, Wo, aH, bH, aW, bW) for an Hi x Wi input -- `size`: this call's output size --; CBinferError naming the
        setting where the library does not take the resize."""
        size = self.size if size is None else _pair('size', size, int)
        if size is None and self.scale_factor is None:
            raise CBinferError("CBResize2d: neither size nor scale_factor is given")
        per = [axis_step(n, None if size is None else size[k], None if size is not None else self.scale_factor[k],
                         self.recompute_scale_factor) for k, n in enumerate((Hi, Wi))]
        (Ho, aH, bH), (Wo, aW, bW) = per
        said = "size=%r" % (size,) if size is not None else "scale_factor=%r" % (self.scale_factor,)
        if Ho < 1 or Wo < 1:
            raise CBinferError("CBResize2d: %s leaves no output pixel of a %dx%d map" % (said, Hi, Wi))
        if (max(Ho, Hi) > MAX_RATIO * min(Ho, Hi) or max(Wo, Wi) > MAX_RATIO * min(Wo, Wi)):
            raise CBinferError("CBResize2d: %s of a %dx%d map is a ratio beyond %d, which the library does not take"
                               % (said, Hi, Wi, MAX_RATIO))
        if max(aH, bH, aW, bW) > MAX_TERM:
            raise CBinferError("CBResize2d: %s of a %dx%d map is the step %d/%d, %d/%d: beyond %d in numerator or "
                               "denominator" % (said, Hi, Wi, aH, bH, aW, bW, MAX_TERM))
        rs = _lib.Resize(Ho, Wo, aH, bH, aW, bW, MODES[self.mode], int(self.align_corners))
        if not C.cbinfer_resize_supported(ctypes.byref(rs), Hi, Wi):
            raise CBinferError("CBResize2d: %s of a %dx%d map (step %d/%d, %d/%d) is beyond the library's limits"
                               % (said, Hi, Wi, aH, bH, aW, bW))
        return Ho, Wo, aH, bH, aW, bW

    def _workspace(self, Hi, Wi, size, dev):
        """Working mask (zero between frames), the frame's mask copy, index buffer, count and the cbResize: once per map
        and output size."""
        def make():
            geo = self.geometry(Hi, Wi, size)
            rs = _lib.Resize(*(geo + (MODES[self.mode], int(self.align_corners))))
            self.__dict__['_rsC'] = ctypes.pointer(rs)
            return dict(mask_workspace(geo[0], geo[1], dev), size=geo[:2])
        return self._cached_work((Hi, Wi, size, dev), make)

    def forward(self, inp, size=None):
        x, indexes = split_operand('CBResize2d', inp, 'the input')
        check_map('CBResize2d', x, note=' (batch 1)')
        require_device(x)
        nc, Hi, Wi = x.size(1), x.size(2), x.size(3)
        work = self._workspace(Hi, Wi, None if size is None else _pair('size', size, int), x.device)
        Ho, Wo = work['size']
        form = operand_changes('CBResize2d', 'the input', indexes, Hi, Wi, x.device, work['idx'])
        if self._fresh_state((1, nc, Ho, Wo), x):      # (written completely: the change information is not used)
            form = EVERY_PIXEL
        check(C.cbinfer_cbresize_forward(ptr(x), ptr(self.outputState), *form_args(form), ptr(work['bits']),
                                         ptr(work['copy']), nc, Hi, Wi, self.__dict__['_rsC'], dtype_code(x),
                                         stream_ptr(x)))
        return self._result(work, Ho, Wo)

    def __repr__(self):
        return ('CBResize2d (size=%s, scale_factor=%s, mode=%s, align_corners=%s, propChgIdxs=%s)'
                % (self.size, self.scale_factor, self.mode, self.align_corners, self.propChangeIndexes))


def insertCBResize(rootModule, cloneOutput=True):
    """Inside every nn.Sequential of rootModule, an nn.Upsample / nn.UpsamplingNearest2d / nn.UpsamplingBilinear2d that is
    still dense and directly follows a producer -- chain.producers('insertCBResize'), another CBResize2d among them and a
    CBConvTranspose2d not -- becomes a CBResize2d when CBResize2d takes it, fed by that producer's changes:
    propChangeIndexes is switched on at the producer (chain.hand_on_changes).  The new module hands its own changes on
    where it stands directly in front of a 1x1 / stride-1 / padding-0 CBConv2d; any other CBConv2d directly behind it
    needs its own input copy (copyInput) unless it runs in feedback mode.  A module the constructor refuses stays dense;
    the limits that depend on the map (a ratio beyond 8 for a size=) show at the first frame.

    The pass takes integer scales as well, and alone is enough.  Measured at x2 (profiles/resize_target.md): with the
    producer's mask the two kernels are level for nearest and this one is about 20 % faster for bilinear; with a change
    LIST nearest costs about 20 % more here, because the general candidate range tests more rows per entry.  Where that
    matters call insertCBUpsampling FIRST: this pass then takes only what that one left.  Returns rootModule."""
    def convert(up):
        try:
            return CBResize2d(up) if type(up) in _UPSAMPLERS else None
        except CBinferError:
            return None      # (beyond the limits: stays dense)
    return insert_behind_producers(rootModule, producers('insertCBResize'), convert, cloneOutput=cloneOutput)
