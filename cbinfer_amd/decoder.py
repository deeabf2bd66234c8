"""Change-based decoder operators: CBUpsample2d, CBConcat2d and insertCBUpsampling (cb_decoder.hip).

The reference has neither operator: an nn.Upsample or a torch.cat(dim=1) -- what every dense-prediction decoder (FCN and
DeepLab heads, U-Net, the top-down path of an FPN) is built from -- ends a change-based chain: torch recomputes the whole
map at the largest resolutions of the network, drops the producers' change masks and cannot be recorded by a
FrameProgram.  Every producer of this package leaves the pixels outside its change list bit for bit as they were, so the
output of either operator can differ from last frame's only at the FOOTPRINT of the operands' changes: both modules
recompute there and are the dense result exactly, without a threshold.

Bilinear upsampling derives its source coordinates in INTEGERS (include/cbinfer_hip.h); torch derives them from a float
scale and its weights drift by about o 2^-24 along a row, so the bilinear values are pinned against float64 math and are
not bit-identical to F.interpolate.  Nearest is bit-identical to torch.
"""
import ctypes

import torch
import torch.nn as nn

from . import _lib
from ._lib import C, CBinferError, check, dtype_code, ptr, require_device, stream_ptr
from .chain import (EVERY_PIXEL, CBStateModule, check_map, form_args, insert_behind_producers, mask_workspace,
                    operand_changes, producers, split_operand, state_fits)

MAX_SCALE = 8


def _integer_scale(v):
    """An int or an integer-valued float as an int, else None."""
    if isinstance(v, bool):
        return None
    if isinstance(v, int):
        return v
    if isinstance(v, float) and v == int(v):
        return int(v)
    return None


def _check_upsample(m):
    """(sH, sW, mode, align_corners) if the library takes the upsampling module `m`; CBinferError with a sentence naming
    the setting otherwise."""
    Err = CBinferError
    if not isinstance(m, nn.Upsample):
        raise Err("CBUpsample2d: only nn.Upsample, nn.UpsamplingNearest2d and nn.UpsamplingBilinear2d modules are "
                  "converted, got %s" % type(m).__name__)
    if m.size is not None:
        raise Err("CBUpsample2d: size=%r is not supported, only an integer scale_factor" % (m.size,))
    sf = m.scale_factor
    if isinstance(sf, (tuple, list)):
        if len(sf) != 2:
            raise Err("CBUpsample2d: scale_factor=%r is not supported, only a number or a pair (2-d maps)" % (sf,))
        pair = tuple(_integer_scale(v) for v in sf)
    else:
        pair = (_integer_scale(sf),) * 2
    if any(v is None for v in pair):
        raise Err("CBUpsample2d: scale_factor=%r is not supported, only integer scales" % (sf,))
    if any(v < 1 or v > MAX_SCALE for v in pair):
        raise Err("CBUpsample2d: scale_factor=%r is beyond what the library takes (1..%d per axis)" % (sf, MAX_SCALE))
    if m.mode not in ('nearest', 'bilinear'):
        raise Err("CBUpsample2d: mode=%r is not supported, only 'nearest' and 'bilinear'" % (m.mode,))
    if getattr(m, 'recompute_scale_factor', None):
        raise Err("CBUpsample2d: recompute_scale_factor=%r is not supported" % (m.recompute_scale_factor,))
    if m.mode == 'nearest' and m.align_corners is not None:
        raise Err("CBUpsample2d: align_corners=%r has no meaning with mode='nearest'" % (m.align_corners,))
    return pair[0], pair[1], m.mode, bool(m.align_corners)


class CBUpsample2d(CBStateModule):
    """nn.Upsample with an integer scale_factor (1..8 per axis), mode 'nearest' or 'bilinear' (align_corners False or
    True), recomputed at the output pixels that read a changed input pixel.

    forward(x): a [1, C, Hi, Wi] tensor -- no change information, every pixel is recomputed -- or the
    ('changeIndexes', tensor, indexes) tuple of a producer with propChangeIndexes.  A MaskChangeIndexes is taken as its
    mask (one launch, the list is not needed); any other ChangeIndexes, or an exact int32 tensor, as a list (one launch
    in front).  The flags are CBAdd2d's: propChangeIndexes hands on the frame's footprint as a MaskChangeIndexes on the
    OUTPUT map; cloneOutput=False hands out the state itself, tagged, and the frame is then free of torch operators."""

    _TRANSIENT = ('_upC',)

    def __init__(self, m):
        super(CBUpsample2d, self).__init__()
        sH, sW, self.mode, self.align_corners = _check_upsample(m)
        self.scale_factor = (sH, sW)
        self.__dict__['_upC'] = None

    def _struct(self):
        """(pointer to) the module's cbUpsample; transient, made again after unpickling."""
        if self.__dict__.get('_upC') is None:
            mode = _lib.UPSAMPLE_NEAREST if self.mode == 'nearest' else _lib.UPSAMPLE_BILINEAR
            self.__dict__['_upC'] = ctypes.pointer(_lib.Upsample(self.scale_factor[0], self.scale_factor[1], mode,
                                                                 int(self.align_corners)))
        return self.__dict__['_upC']

    def _workspace(self, Hi, Wi, dev):
        """Working mask (zero between frames), the frame's mask copy, index buffer and count: once per map size."""
        Ho, Wo = Hi * self.scale_factor[0], Wi * self.scale_factor[1]
        return self._cached_work((Hi, Wi, dev), lambda: dict(mask_workspace(Ho, Wo, dev), size=(Ho, Wo)))

    def forward(self, inp):
        x, indexes = split_operand('CBUpsample2d', inp, 'the input')
        check_map('CBUpsample2d', x)
        require_device(x)
        nc, Hi, Wi = x.size(1), x.size(2), x.size(3)
        work = self._workspace(Hi, Wi, x.device)
        Ho, Wo = work['size']
        form = operand_changes('CBUpsample2d', 'the input', indexes, Hi, Wi, x.device, work['idx'])
        if self._fresh_state((1, nc, Ho, Wo), x):      # (written completely: the change information is not used)
            form = EVERY_PIXEL
        check(C.cbinfer_cbupsample_forward(ptr(x), ptr(self.outputState), *form_args(form), ptr(work['bits']),
                                           ptr(work['copy']), nc, Hi, Wi, self._struct(), dtype_code(x), stream_ptr(x)))
        return self._result(work, Ho, Wo)

    def __repr__(self):
        return ('CBUpsample2d (scale_factor=%s, mode=%s, align_corners=%s, propChgIdxs=%s)'
                % (self.scale_factor, self.mode, self.align_corners, self.propChangeIndexes))


class CBConcat2d(CBStateModule):
    """torch.cat(operands, dim=1) of 2..4 [1, Ck, H, W] maps: operand k's channels are copied at operand k's changed
    pixels only -- a skip connection that did not change is not touched -- and the union of the operands' changes is
    handed on.

    forward(operands): a list of tensors or ('changeIndexes', tensor, indexes) tuples, each in the forms CBUpsample2d
    takes; the flags are the same.  (pycbinfer.ChannelConcat is the dense concat: it copies every pixel every frame and
    hands nothing on.)"""

    def __init__(self):
        super(CBConcat2d, self).__init__()
        self._channels = None      # (the channel split the state was written with)

    def clearMemory(self):
        super(CBConcat2d, self).clearMemory()
        self.__dict__['_channels'] = None

    def _workspace(self, n, H, W, dev):
        """n working masks (zero between frames), the frame's mask copy, index buffer, count and the host argument
        arrays: once per operand count and map size."""
        return self._cached_work((n, H, W, dev), lambda: dict(
            mask_workspace(H, W, dev, nbits=n),
            srcs=(ctypes.c_void_p * n)(), chans=(ctypes.c_int32 * n)(), masks=(ctypes.c_void_p * n)(),
            lists=(ctypes.c_void_p * n)(), caps=(ctypes.c_int32 * n)(), counts=(ctypes.c_void_p * n)()))

    def forward(self, operands):
        if not isinstance(operands, (list, tuple)) or (type(operands) == tuple and operands[:1] == ('changeIndexes',)):
            raise CBinferError("CBConcat2d: forward takes a LIST of operands (tensors or ('changeIndexes', tensor, "
                               "indexes) tuples), got %s" % type(operands).__name__)
        n = len(operands)
        if not 2 <= n <= 4:
            raise CBinferError("CBConcat2d: 2..4 operands, got %d" % n)
        split = [split_operand('CBConcat2d', x, 'operand %d' % k) for k, x in enumerate(operands)]
        t0 = split[0][0]
        for k, (t, _) in enumerate(split):
            if t.dim() != 4 or t.size(0) != 1:
                raise CBinferError("CBConcat2d: operands must be [1, C, H, W] tensors, operand %d is %s"
                                   % (k, tuple(t.shape)))
            if t.shape[2:] != t0.shape[2:] or t.dtype != t0.dtype or t.device != t0.device:
                raise CBinferError("CBConcat2d: the operands differ: operand 0 is %s %s on %s, operand %d is %s %s on %s"
                                   % (tuple(t0.shape), t0.dtype, t0.device, k, tuple(t.shape), t.dtype, t.device))
        if t0.dtype not in (torch.float32, torch.float16):
            raise CBinferError("CBConcat2d: float32 and float16 tensors only, got %s" % t0.dtype)
        require_device(*[t for t, _ in split])
        H, W = t0.size(2), t0.size(3)
        chans = tuple(t.size(1) for t, _ in split)
        work = self._workspace(n, H, W, t0.device)
        forms = [operand_changes('CBConcat2d', 'operand %d' % k, ix, H, W, t0.device, work['idx'])
                 for k, (_, ix) in enumerate(split)]
        if not state_fits(self.outputState, (1, sum(chans), H, W), t0) or self.__dict__.get('_channels') != chans:
            # a new state is written completely: no operand's change information is used
            self.outputState = torch.empty((1, sum(chans), H, W), dtype=t0.dtype, device=t0.device)
            self.__dict__['_channels'] = chans
            forms = [EVERY_PIXEL] * n
        for k, ((t, _), f) in enumerate(zip(split, forms)):
            work['srcs'][k], work['chans'][k] = t.data_ptr(), chans[k]
            work['masks'][k], work['lists'][k], work['caps'][k], work['counts'][k] = form_args(f)
        check(C.cbinfer_cbconcat_forward(work['srcs'], work['chans'], n, ptr(self.outputState), work['masks'],
                                         work['lists'], work['caps'], work['counts'], ptr(work['bits']),
                                         ptr(work['copy']), H, W, dtype_code(t0), stream_ptr(t0)))
        return self._result(work, H, W)

    def __repr__(self):
        return 'CBConcat2d (propChgIdxs=%s)' % self.propChangeIndexes


_UPSAMPLERS = (nn.Upsample, nn.UpsamplingNearest2d, nn.UpsamplingBilinear2d)


def insertCBUpsampling(rootModule, cloneOutput=True):
    """Inside every nn.Sequential of rootModule, an nn.Upsample / nn.UpsamplingNearest2d / nn.UpsamplingBilinear2d within
    the library's limits that directly follows a producer -- chain.producers('insertCBUpsampling'), another
    CBUpsample2d among them and a CBConvTranspose2d not -- becomes a CBUpsample2d fed by that producer's changes:
    propChangeIndexes is switched on at the producer (chain.hand_on_changes).  The new module hands nothing on: a
    CBConv2d consuming the upsampled map, a 1x1 layer included, needs its own input copy (copyInput) unless it runs in
    feedback mode, as behind a pool of insertCBPooling.  An upsampling beyond the limits stays the dense torch operator.
    Returns rootModule."""
    def convert(up):
        try:
            return CBUpsample2d(up) if type(up) in _UPSAMPLERS else None
        except CBinferError:
            return None      # (beyond the limits: stays dense)
    return insert_behind_producers(rootModule, producers('insertCBUpsampling'), convert, cloneOutput=cloneOutput,
                                   handOn=False)
