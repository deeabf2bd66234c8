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
import copy
import ctypes
import fractions
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from ._lib import C, CBinferError, check, dtype_code, ptr, require_device, stream_ptr
from .chain import (EVERY_PIXEL, CBStateModule, check_map, form_args, insert_behind_producers, mask_workspace,
                    operand_changes, producers, split_operand)

MAX_RATIO = 8          # per axis, either way
MAX_TERM = 4096        # numerator and denominator of the reduced step
MODES = {'nearest': _lib.RESIZE_NEAREST, 'nearest-exact': _lib.RESIZE_NEAREST_EXACT, 'bilinear': _lib.RESIZE_BILINEAR,
         'bicubic': _lib.RESIZE_BICUBIC}
_UPSAMPLERS = (nn.Upsample, nn.UpsamplingNearest2d, nn.UpsamplingBilinear2d)
# grid sampling (cb_warp.hip)
WARP_MODES = {'nearest': _lib.WARP_NEAREST, 'bilinear': _lib.WARP_BILINEAR, 'bicubic': _lib.WARP_BICUBIC}
WARP_PADDINGS = {'zeros': _lib.WARP_ZEROS, 'border': _lib.WARP_BORDER, 'reflection': _lib.WARP_REFLECTION}
MAX_EXTENT = 1 << 15   # every extent of a grid sampling lies below it


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
    size changes.  The flags propChangeIndexes and cloneOutput are CBUpsample2d's.

    GRID SAMPLING (F.grid_sample).  Any of the keywords grid, theta and padding_mode makes the module one
    that samples x through a coordinate field: mode 'nearest', 'bilinear' or 'bicubic', padding_mode 'zeros' (the
    default), 'border' or 'reflection', align_corners either way.  An output pixel is recomputed where its coordinate
    pair changed or one of its taps did.
      grid=G: a constant [1, Ho, Wo, 2] field of normalised (x, y) pairs, float32 or float16, finite.  It is COPIED into
        the persistent buffer `grid`, which follows the module's device but keeps its dtype under .half().
      theta=T, size=(Ho, Wo): the constant grid F.affine_grid(T, (1, 1, Ho, Wo), align_corners) of a [1, 2, 3] or [2, 3]
        matrix, computed once on the CPU in float32.
      neither: forward(x, grid=...) or forward(x, flow=...) hands the field over every frame -- a tensor, or the
        ('changeIndexes', tensor, indexes) tuple of a producer with indexes on the Ho x Wo output map.  grid is
        [1, Ho, Wo, 2], normalised; flow is [1, 2, Ho, Wo], channel 0 = dx and channel 1 = dy in input pixels, the source
        of output pixel (oy, ox) being (ox + dx, oy + dy): what a flow head produces, without the dense
        base + permute * scale in front of F.grid_sample.  The field is float32 or float16 whatever x is."""

    _TRANSIENT = ('_rsC',)

    def __init__(self, m=None, size=None, scale_factor=None, mode='nearest', align_corners=None,
                 recompute_scale_factor=None, antialias=False, grid=None, theta=None, padding_mode=None):
        super(CBResize2d, self).__init__()
        Err = CBinferError
        self.warp = grid is not None or theta is not None or padding_mode is not None
        if self.warp:
            self._init_warp(m, size, scale_factor, mode, align_corners, recompute_scale_factor, antialias, grid, theta,
                            padding_mode)
            return
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

    def _init_warp(self, m, size, scale_factor, mode, align_corners, recompute_scale_factor, antialias, grid, theta,
                   padding_mode):
        Err = CBinferError
        for name, v in (('m', m), ('scale_factor', scale_factor), ('recompute_scale_factor', recompute_scale_factor)):
            if v is not None:
                raise Err("CBResize2d: %s=%r has no meaning with a coordinate field (grid / theta / padding_mode)"
                          % (name, v))
        if antialias:
            raise Err("CBResize2d: antialias=%r is not supported" % (antialias,))
        if mode == 'nearest-exact':
            raise Err("CBResize2d: mode='nearest-exact' is not supported with a coordinate field, only 'nearest', "
                      "'bilinear' and 'bicubic' (F.grid_sample has no such mode)")
        if mode not in WARP_MODES:
            raise Err("CBResize2d: mode=%r is not supported with a coordinate field, only 'nearest', 'bilinear' and "
                      "'bicubic'" % (mode,))
        padding_mode = 'zeros' if padding_mode is None else padding_mode
        if padding_mode not in WARP_PADDINGS:
            raise Err("CBResize2d: padding_mode=%r is not supported, only 'zeros', 'border' and 'reflection'"
                      % (padding_mode,))
        if grid is not None and theta is not None:
            raise Err("CBResize2d: only one of grid and theta may be given")
        if (size is not None) != (theta is not None):
            raise Err("CBResize2d: size=%r goes with theta and only with it (a grid has its own size)" % (size,))
        self.size, self.scale_factor, self.recompute_scale_factor = None, None, False
        self.mode, self.padding_mode, self.align_corners = mode, padding_mode, bool(align_corners)
        if theta is not None:
            Ho, Wo = _pair('size', size, int)
            ok = torch.is_tensor(theta) and tuple(theta.shape) in ((1, 2, 3), (2, 3)) and theta.is_floating_point()
            if not ok:
                raise Err("CBResize2d: theta must be a [1, 2, 3] or [2, 3] floating-point matrix, got %s"
                          % (tuple(theta.shape) if torch.is_tensor(theta) else type(theta).__name__,))
            if max(Ho, Wo) >= MAX_EXTENT:
                raise Err("CBResize2d: size=%r is beyond the library's limits (extents below %d)" % (size, MAX_EXTENT))
            made = F.affine_grid(theta.detach().float().cpu().reshape(1, 2, 3), (1, 1, Ho, Wo),
                                 align_corners=self.align_corners)
            grid = made.to(theta.device)
        if grid is not None:
            ok = (torch.is_tensor(grid) and grid.dim() == 4 and grid.size(0) == 1 and grid.size(3) == 2 and
                  grid.numel() > 0)
            if not ok:
                raise Err("CBResize2d: grid must be a [1, Ho, Wo, 2] tensor (batch 1), got %s"
                          % (tuple(grid.shape) if torch.is_tensor(grid) else type(grid).__name__,))
            if grid.dtype not in (torch.float32, torch.float16):
                raise Err("CBResize2d: grid must be a float32 or float16 tensor, got %s" % grid.dtype)
            if max(grid.size(1), grid.size(2)) >= MAX_EXTENT:
                raise Err("CBResize2d: a %dx%d grid is beyond the library's limits (extents below %d)"
                          % (grid.size(1), grid.size(2), MAX_EXTENT))
            if not bool(torch.isfinite(grid.detach().cpu()).all()):
                raise Err("CBResize2d: grid holds a value that is not finite")
            self.register_buffer('grid', grid.detach().clone().contiguous())
        self.__dict__['_rsC'] = None

    def _apply(self, fn, *args, **kwargs):
        # (the constant grid follows the module's device and keeps its dtype: .half() would cost it 13 bits of position)
        held = self._buffers.pop('grid', None) if self.__dict__.get('warp') else None
        super(CBResize2d, self)._apply(fn, *args, **kwargs)
        if held is not None:
            self._buffers['grid'] = held.to(self.outputState.device)
        return self

    def _warp_forward(self, inp, grid, flow):
        name, Err = 'CBResize2d', CBinferError
        const = self._buffers.get('grid')
        if grid is not None and flow is not None:
            raise Err("CBResize2d: only one of grid= and flow= may be given")
        given = 'grid' if grid is not None else 'flow' if flow is not None else None
        if const is not None and given:
            raise Err("CBResize2d: the module has a constant grid: forward takes no %s=" % given)
        if const is None and not given:
            raise Err("CBResize2d: the module has no constant grid: forward(x, grid=...) or forward(x, flow=...) must "
                      "hand the coordinate field over every frame")
        x, indexes = split_operand(name, inp, 'the input')
        check_map(name, x, note=' (batch 1)')
        if const is not None:
            co, coIdx, kind = const, None, _lib.WARP_GRID
        else:
            co, coIdx = split_operand(name, grid if given == 'grid' else flow, 'the %s' % given)
            kind = _lib.WARP_GRID if given == 'grid' else _lib.WARP_FLOW
        axes = (1, 2, 3) if kind == _lib.WARP_GRID else (2, 3, 1)
        if co.dim() != 4 or co.size(0) != 1 or co.size(axes[2]) != 2 or co.numel() == 0:
            raise Err("CBResize2d: %s must be a %s tensor (batch 1), got %s"
                      % (given or 'grid', '[1, Ho, Wo, 2]' if kind == _lib.WARP_GRID else '[1, 2, Ho, Wo]',
                         tuple(co.shape)))
        if co.dtype not in (torch.float32, torch.float16):
            raise Err("CBResize2d: %s must be a float32 or float16 tensor, got %s" % (given or 'grid', co.dtype))
        require_device(x, co)
        if co.device != x.device:
            raise Err("CBResize2d: the input is on %s, the %s on %s" % (x.device, given or 'constant grid', co.device))
        nc, Hi, Wi, Ho, Wo = x.size(1), x.size(2), x.size(3), co.size(axes[0]), co.size(axes[1])

        def make():
            wp = _lib.Warp(Ho, Wo, WARP_MODES[self.mode], WARP_PADDINGS[self.padding_mode], int(self.align_corners),
                           kind, dtype_code(co))
            if not C.cbinfer_warp_supported(ctypes.byref(wp), Hi, Wi):
                raise Err("CBResize2d: sampling a %dx%d map on a %dx%d field is beyond the library's limits (every "
                          "extent below %d)" % (Hi, Wi, Ho, Wo, MAX_EXTENT))
            return dict(mask_workspace(Ho, Wo, x.device), size=(Ho, Wo), warp=ctypes.pointer(wp),
                        inBits=torch.zeros(C.cbinfer_mask_words(Hi, Wi), dtype=torch.int64, device=x.device))
        work = self._cached_work((Hi, Wi, Ho, Wo, kind, co.dtype, x.device), make)
        fx = operand_changes(name, 'the input', indexes, Hi, Wi, x.device, work['idx'])
        # (a constant grid never changes: the empty list)
        fc = ((None, work['idx'], 0, None) if const is not None else
              operand_changes(name, 'the %s' % given, coIdx, Ho, Wo, x.device, work['idx']))
        if self._fresh_state((1, nc, Ho, Wo), x):      # (written completely: no change information is used)
            fx = fc = EVERY_PIXEL
        check(C.cbinfer_cbwarp_forward(ptr(x), ptr(co), ptr(self.outputState), *form_args(fx), *form_args(fc),
                                       ptr(work['inBits']), ptr(work['bits']), ptr(work['copy']), nc, Hi, Wi,
                                       work['warp'], dtype_code(x), stream_ptr(x)))
        return self._result(work, Ho, Wo)

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

    def forward(self, inp, size=None, grid=None, flow=None):
        if self.__dict__.get('warp'):
            if size is not None:
                raise CBinferError("CBResize2d: size=%r has no meaning in the forward of a module that samples through "
                                   "a coordinate field: the field has its own size" % (size,))
            return self._warp_forward(inp, grid, flow)
        for name, v in (('grid', grid), ('flow', flow)):
            if v is not None:
                raise CBinferError("CBResize2d: %s= needs a module built for a coordinate field (grid=, theta= or "
                                   "padding_mode=); this one is a plain resize" % name)
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
        if self.__dict__.get('warp'):
            const = self._buffers.get('grid')
            return ('CBResize2d (grid=%s, mode=%s, padding_mode=%s, align_corners=%s, propChgIdxs=%s)'
                    % (tuple(const.shape) if const is not None else 'per frame', self.mode, self.padding_mode,
                       self.align_corners, self.propChangeIndexes))
        return ('CBResize2d (size=%s, scale_factor=%s, mode=%s, align_corners=%s, propChgIdxs=%s)'
                % (self.size, self.scale_factor, self.mode, self.align_corners, self.propChangeIndexes))


def computes_grid_sample(m, attr):
    """Whether the module `m` computes F.grid_sample(x, m.<attr>, m.mode, m.padding_mode, m.align_corners), bit for
    bit, on a random CPU tensor: what insertCBResize(gridTypes=...) holds a user's class against."""
    try:
        probe = copy.deepcopy(m).cpu().float()
        grid = getattr(probe, attr)
        x = torch.rand(1, 3, 9, 11, generator=torch.Generator().manual_seed(5)) * 2 - 1
        with torch.no_grad():
            want = F.grid_sample(x, grid, mode=probe.mode, padding_mode=probe.padding_mode,
                                 align_corners=probe.align_corners)
            got = probe(x)
        return torch.is_tensor(got) and got.shape == want.shape and torch.equal(got, want)
    except Exception:
        return False


def insertCBResize(rootModule, cloneOutput=True, gridTypes=None):
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
    matters call insertCBUpsampling FIRST: this pass then takes only what that one left.

    gridTypes: {class: name of its constant-grid attribute}, a class of the user's that computes
    F.grid_sample(x, self.<attribute>, self.mode, self.padding_mode, self.align_corners) -- torch has no module for the
    operator.  A module of EXACTLY such a type behind the same producers becomes CBResize2d(grid=..., mode=...,
    padding_mode=..., align_corners=...).  Before it is converted it is run against that rule on a random CPU tensor: a
    class whose forward is something else, or a module whose configuration the constructor refuses, is refused by name
    (CBinferError), never converted silently and never left dense.  Returns rootModule."""
    gridTypes = dict(gridTypes or {})
    for t, attr in gridTypes.items():
        if not (isinstance(t, type) and isinstance(attr, str)):
            raise CBinferError("insertCBResize: gridTypes maps a class to the name of its constant-grid attribute, got "
                               "%r: %r" % (t, attr))

    def sampling(m):
        attr, said = gridTypes[type(m)], type(m).__name__
        if not computes_grid_sample(m, attr):
            raise CBinferError("insertCBResize: %s does not compute F.grid_sample(x, self.%s, self.mode, "
                               "self.padding_mode, self.align_corners) (checked bit for bit on a random CPU tensor): it "
                               "is not converted" % (said, attr))
        try:
            return CBResize2d(grid=getattr(m, attr), mode=m.mode, padding_mode=m.padding_mode,
                              align_corners=m.align_corners)
        except CBinferError as e:
            raise CBinferError("insertCBResize: %s is not converted: %s" % (said, e))

    def convert(up):
        if type(up) in gridTypes:
            return sampling(up)
        try:
            return CBResize2d(up) if type(up) in _UPSAMPLERS else None
        except CBinferError:
            return None      # (beyond the limits: stays dense)
    return insert_behind_producers(rootModule, producers('insertCBResize'), convert, cloneOutput=cloneOutput)
