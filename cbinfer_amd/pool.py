"""CBPoolMax2d / CBPoolAvg2d: change-based pooling modules on MI355X, and the LazyPool a folded 2x2 pool hands on.

Four forms in one class: the reference's 2x2/stride-2 max pool (pycbinfer/conv2d.py:24-84), any window (cb_pool2d.hip,
DESIGN 5.11), the adaptive / global pool (cb_adaptpool.hip) and, opted into with suppress=, the peak
suppression a keypoint head ends with -- a stride-1 max pool compared with its own input -- and its peak list
(cb_peaks.hip).  The flags, the outputState buffer, the
keyed work buffers and what is left out of a pickle are chain.CBStateModule's, as for every other mask-driven module.
conv2d.py re-exports the three classes: the reference's pickles and this package's older ones name them there.
"""
import ctypes
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from ._lib import C, CBinferError, check, dtype_code, ptr, require_device, stream_ptr
from .chain import (EVERY_PIXEL, PROPAGATED, CBStateModule, check_map, form_args, frame_output, mask_workspace,
                    operand_changes, state_fits)
from .conv2d_cg import MaskChangeIndexes, maxPool2d, poolChangeIndexes


class LazyPool(object):
    """What a CBPoolMax2d with lazy=True hands to the next module instead of a pooled tensor: the pool's
    INPUT and the pooled size.  A feedback-mode CBConv2d folds the pooling into its change detection
    (cbinfer_cbconv2d_forward_pooled) and never needs the pooled map; anything else calls tensor()."""

    def __init__(self, source, outSize, ceil_mode, indexes=None):
        self.source = source
        self.outSize = tuple(outSize)
        self.ceil_mode = ceil_mode
        self.indexes = indexes      # the producer's change indexes of this frame (pre-pool resolution)

    def producerMask(self):
        """The producing layer's change bit mask of this frame, if it ran a mask-driven contraction: the
        consumer's pooled detection then only looks where that layer rewrote something."""
        ix = self.indexes
        if isinstance(ix, MaskChangeIndexes) and ix.size == tuple(self.source.shape[-2:]):
            return ix._mask
        return None

    def tensor(self):
        return F.max_pool2d(self.source, 2, 2, ceil_mode=self.ceil_mode)


def _pool_pair(v, what):
    """An int or a pair of ints of a pooling module as a pair; CBinferError for anything else (a string, a triple)."""
    if isinstance(v, int) and not isinstance(v, bool):
        return (v, v)
    if isinstance(v, (tuple, list)) and len(v) == 2 and all(isinstance(x, int) and not isinstance(x, bool) for x in v):
        return tuple(v)
    raise CBinferError("change-based pooling: %s=%r is not supported, only an int or a pair of ints" % (what, v))


def _check_general_pool(m, kind):
    """(kernel_size, stride, padding, cbPool operation) if the general change-based pool takes `m`, an nn.MaxPool2d
    (kind 'max') or nn.AvgPool2d ('avg'): per axis window <= 8, stride <= 8, padding <= window / 2, dilation 1, no
    return_indices, no divisor_override.  CBinferError with a sentence otherwise."""
    Err = CBinferError
    if kind == 'max':
        name, op = 'CBPoolMax2d', _lib.POOL_MAX
        if not isinstance(m, nn.MaxPool2d):
            raise Err("CBPoolMax2d: only nn.MaxPool2d modules are converted")
        if _pool_pair(m.dilation, 'dilation') != (1, 1):
            raise Err("CBPoolMax2d: dilated max pooling is not supported (dilation=%s)" % (m.dilation,))
        if m.return_indices:
            raise Err("CBPoolMax2d: return_indices=True is not supported (the change-based pool keeps no argmax)")
    else:
        name = 'CBPoolAvg2d'
        if not isinstance(m, nn.AvgPool2d):
            raise Err("CBPoolAvg2d: only nn.AvgPool2d modules are converted")
        if m.divisor_override is not None:
            raise Err("CBPoolAvg2d: divisor_override=%r is not supported" % (m.divisor_override,))
        op = _lib.POOL_AVG_PAD if m.count_include_pad else _lib.POOL_AVG_NOPAD
    k = _pool_pair(m.kernel_size, 'kernel_size')
    s = _pool_pair(m.stride if m.stride is not None else m.kernel_size, 'stride')
    p = _pool_pair(m.padding, 'padding')
    g = _lib.Pool(k[0], k[1], s[0], s[1], p[0], p[1], int(bool(m.ceil_mode)), op)
    if not C.cbinfer_pool_supported(ctypes.byref(g)):
        raise Err("%s: kernel_size=%s stride=%s padding=%s is beyond what the library takes (per axis: window <= 8, "
                  "stride <= 8, padding <= window / 2)" % (name, k, s, p))
    return k, s, p, op


SUPPRESS_KINDS = ('window', 'cross')


def _check_suppress(m, generalGeometry, suppress, floor, peakList):
    """(kernel_size, floor as a float or None, peakList as an int) of CBPoolMax2d(m, suppress=...): m exactly an
    nn.MaxPool2d of stride 1, an odd window of 3, 5 or 7 per axis, padding k // 2, dilation 1, ceil_mode=False and no
    return_indices.  CBinferError that names the argument otherwise."""
    Err = CBinferError
    if suppress not in SUPPRESS_KINDS:
        raise Err("CBPoolMax2d: suppress=%r is not supported, only None, 'window' or 'cross'" % (suppress,))
    if not generalGeometry:
        raise Err("CBPoolMax2d: suppress=%r needs generalGeometry=True (peak suppression is a general-geometry module)"
                  % (suppress,))
    if type(m) is not nn.MaxPool2d:
        raise Err("CBPoolMax2d: suppress=%r takes an nn.MaxPool2d (exactly, not a subclass), got %s"
                  % (suppress, type(m).__name__))
    k = _pool_pair(m.kernel_size, 'kernel_size')
    if not all(v in (3, 5, 7) for v in k):
        raise Err("CBPoolMax2d: suppress=%r needs kernel_size 3, 5 or 7 per axis, got kernel_size=%s" % (suppress, k))
    st = _pool_pair(m.stride if m.stride is not None else m.kernel_size, 'stride')
    if st != (1, 1):
        raise Err("CBPoolMax2d: suppress=%r needs stride=1, got stride=%s" % (suppress, st))
    pd = _pool_pair(m.padding, 'padding')
    if pd != (k[0] // 2, k[1] // 2):
        raise Err("CBPoolMax2d: suppress=%r needs padding=kernel_size // 2 = %s, got padding=%s"
                  % (suppress, (k[0] // 2, k[1] // 2), pd))
    if _pool_pair(m.dilation, 'dilation') != (1, 1):
        raise Err("CBPoolMax2d: suppress=%r needs dilation=1, got dilation=%s" % (suppress, m.dilation))
    if m.ceil_mode:
        raise Err("CBPoolMax2d: suppress=%r needs ceil_mode=False" % (suppress,))
    if m.return_indices:
        raise Err("CBPoolMax2d: suppress=%r does not take return_indices=True" % (suppress,))
    if suppress == 'cross' and k != (3, 3):
        raise Err("CBPoolMax2d: suppress='cross' is the 3x3 neighbourhood only, got kernel_size=%s" % (k,))
    if floor is not None:
        if isinstance(floor, bool) or not isinstance(floor, (int, float)) or not math.isfinite(floor):
            raise Err("CBPoolMax2d: floor=%r is not supported, only None or a finite number" % (floor,))
        floor = float(floor)
    if isinstance(peakList, bool) or not isinstance(peakList, int) or peakList < 0:
        raise Err("CBPoolMax2d: peakList=%r is not supported, only the capacity of the list as an int >= 0" % (peakList,))
    return k, floor, peakList


_ADAPTIVE_POOLS = {'max': nn.AdaptiveMaxPool2d, 'avg': nn.AdaptiveAvgPool2d}


def _check_adaptive_pool(m, kind, generalGeometry):
    """The output_size of the nn.AdaptiveMaxPool2d (kind 'max') or nn.AdaptiveAvgPool2d ('avg') `m` as a pair whose
    entries are an int >= 1 or None (the input's size on that axis).  CBinferError with a sentence otherwise."""
    Err = CBinferError
    name = 'CBPoolMax2d' if kind == 'max' else 'CBPoolAvg2d'
    if not generalGeometry:
        raise Err("%s: an %s runs on the adaptive pool of the general geometry only: pass generalGeometry=True"
                  % (name, type(m).__name__))
    if getattr(m, 'return_indices', False):
        raise Err("%s: return_indices=True is not supported (the change-based pool keeps no argmax)" % name)
    size = m.output_size
    if not isinstance(size, (tuple, list)):
        size = (size, size)
    if len(size) != 2 or not all(v is None or (isinstance(v, int) and not isinstance(v, bool) and v >= 1) for v in size):
        raise Err("%s: output_size=%r is not supported, only an int >= 1, None or a pair of them" % (name, m.output_size))
    return tuple(size)


class CBPoolMax2d(CBStateModule):
    """Change-based max pooling: 2x2/stride-2 (reference: conv2d.py:24-84) and, with generalGeometry=True, any window,
    stride, zero padding and ceil_mode within the library's limits (cb_pool2d.hip) and an
    nn.AdaptiveMaxPool2d of any output size up to the map's, the global pool included (cb_adaptpool.hip).
    cloneOutput (CBStateModule) is the reference's private copy of the state every frame (conv2d.py:73).  forward takes
    the ('changeIndexes', tensor, indexes) tuple of its producer; a bare tensor counts as every pixel listed.

    suppress='window' / 'cross' (with generalGeometry=True; m an nn.MaxPool2d(k, 1, k // 2), k 3, 5 or 7 per axis): peak
    suppression instead of pooling (cb_peaks.hip).  The output [1, C, H, W] keeps a pixel's value where it
    is >= every in-map pixel of its k x k window ('cross': of its four neighbours, 3x3 only) and >= floor, if one is
    given, and is +0 elsewhere: torch.where((F.max_pool2d(x, k, 1, k // 2) == x) & (x >= floor), x, 0) bit for bit.
    Recomputed at the k x k footprint of the operand's changes, which is also the mask handed on.  The state is
    outputState and peakBits (one bit per pixel and channel).  peakList=N > 0: every frame also makes the ordered list of
    the peaks, at most N of them, on the device (peakList(), peaksToHost())."""
    _KIND = 'max'
    _WORK = '_poolWork'          # (device work buffers of the general and the adaptive path)
    _TRANSIENT = ('_poolC',)     # (the ctypes cbPool)

    def __init__(self, m, generalGeometry=False, suppress=None, floor=None, peakList=0):
        super(CBPoolMax2d, self).__init__()
        self.generalGeometry = bool(generalGeometry)
        self.suppress, self.floor, self.peakCapacity = None, None, 0
        if suppress is None and (floor is not None or peakList != 0):
            raise CBinferError("%s: %s has a meaning with suppress='window' or 'cross' only"
                               % (self.__class__.__name__, "floor=%r" % (floor,) if floor is not None
                                  else "peakList=%r" % (peakList,)))
        self._adaptive = suppress is None and type(m) is _ADAPTIVE_POOLS[self._KIND]
        if suppress is not None:
            ks, self.floor, self.peakCapacity = _check_suppress(m, self.generalGeometry, suppress, floor, peakList)
            self.suppress = suppress
            st, pd, self._op = (1, 1), (ks[0] // 2, ks[1] // 2), _lib.POOL_MAX
            self.clearMemory()      # (registers peakBits)
        elif self._adaptive:
            self.output_size = _check_adaptive_pool(m, self._KIND, self.generalGeometry)
            ks, st, pd = None, None, (0, 0)
            self._op = _lib.ADAPT_MAX if self._KIND == 'max' else _lib.ADAPT_AVG
        elif self.generalGeometry:
            ks, st, pd, self._op = _check_general_pool(m, self._KIND)
        else:
            ks = m.kernel_size if isinstance(m.kernel_size, tuple) else (m.kernel_size,) * 2
            st = m.stride if isinstance(m.stride, tuple) else (m.stride,) * 2
            assert ks == (2, 2) and st == (2, 2)
            pd, self._op = (0, 0), _lib.POOL_MAX
        # a window the 2x2 kernel cannot take runs on cb_pool2d.hip; a 2x2/s2/p0 max pool runs as it always did
        # (an adaptive pool runs on cb_adaptpool.hip: never folded, never batched, as every general pool)
        self._general = self._adaptive or (
            self.generalGeometry and (self._KIND != 'max' or (ks, st, pd) != ((2, 2), (2, 2), (0, 0))))
        self.padding = pd
        self._poolC = None
        self.stride = st
        self.kernel_size = ks
        self.ceil_mode = getattr(m, 'ceil_mode', False)
        # True: hand on the list of changed OUTPUT pixels instead of the input-resolution one (conv2d.py:80-83)
        self.downsampleIndexes = False
        # True (fusePoolingIntoDetection): hand the consumer a LazyPool; it pools inside its change detection
        self.lazy = False

    def clearMemory(self):
        super(CBPoolMax2d, self).clearMemory()
        # the row-segment partials of an adaptive pool (f32 [C, ow, H]); empty for every other pool
        if 'partials' not in self._buffers:
            self.register_buffer('partials', torch.zeros(0))
        self.partials = self.partials.new_zeros(0)
        # the peak bits of a suppressing pool (int64 [C mask words]); no other pool has the buffer
        if self.__dict__.get('suppress') is not None:
            if 'peakBits' not in self._buffers:
                self.register_buffer('peakBits', torch.zeros(0, dtype=torch.int64))
            self.peakBits = self.peakBits.new_zeros(0)

    def getStateTensors(self):
        if not hasattr(self, 'outputState'):
            return []
        if self.__dict__.get('suppress') is not None:
            return [self.outputState, self.peakBits]
        return [self.outputState, self.partials] if self.__dict__.get('_adaptive') else [self.outputState]

    def _setDefaultValues(self):
        # back-fill attributes missing in modules pickled by older versions
        for name, val in (('generalGeometry', False), ('_general', False), ('padding', (0, 0)), ('_op', _lib.POOL_MAX),
                          ('_poolC', None), ('_poolWork', None), ('_adaptive', False), ('suppress', None), ('floor', None),
                          ('peakCapacity', 0)):
            if name not in self.__dict__:
                self.__dict__[name] = val
        if 'partials' not in self._buffers:
            self.register_buffer('partials', torch.zeros(0))

    def __setstate__(self, state):
        super(CBPoolMax2d, self).__setstate__(state)
        self._setDefaultValues()

    def _pool_struct(self):
        """(pointer to) the module's cbPool; transient, made again after unpickling."""
        if self.__dict__.get('_poolC') is None:
            k, s_, p_ = self.kernel_size, self.stride, self.padding
            self.__dict__['_poolC'] = ctypes.pointer(_lib.Pool(k[0], k[1], s_[0], s_[1], p_[0], p_[1],
                                                               int(bool(self.ceil_mode)), self._op))
        return self.__dict__['_poolC']

    def _out_hw(self, Hi, Wi):
        Ho, Wo = ctypes.c_int(), ctypes.c_int()
        if C.cbinfer_pool_out_size(Hi, Wi, self._pool_struct(), ctypes.byref(Ho), ctypes.byref(Wo)) != 0:
            raise CBinferError("%s: a %dx%d map is smaller than the window (kernel_size=%s, padding=%s)"
                               % (self.__class__.__name__, Hi, Wi, tuple(self.kernel_size), tuple(self.padding)))
        return Ho.value, Wo.value

    def _adaptive_out(self, Hi, Wi):
        """The output size of an adaptive pool on an Hi x Wi map: None is the map's own size on that axis."""
        oh, ow = (n if v is None else v for v, n in zip(self.output_size, (Hi, Wi)))
        if oh > Hi or ow > Wi:
            raise CBinferError("%s: output_size=%s is larger than the %dx%d map on an axis (an adaptive pool that "
                               "repeats pixels is not converted)" % (self.__class__.__name__, (oh, ow), Hi, Wi))
        if not C.cbinfer_adaptive_pool_supported(Hi, Wi, oh, ow):
            raise CBinferError("%s: a %dx%d map pooled to %s is beyond what the library takes (output width <= 4096)"
                               % (self.__class__.__name__, Hi, Wi, (oh, ow)))
        return oh, ow

    def _frame(self, input, changeIndexes):
        """What a frame on cb_pool2d.hip or cb_adaptpool.hip starts from: (C, Hi, Wi, the work buffers, the form of the
        operand's changes).  The buffers are mask_workspace's on the OUTPUT map, its `size`, and for an adaptive pool
        the working mask of the INPUT map (for a list operand)."""
        nc, Hi, Wi = input.size(-3), input.size(-2), input.size(-1)
        assert input.dim() == 4 and input.size(0) == 1
        dev = input.device

        def make():
            if not self._adaptive:
                size, more = self._out_hw(Hi, Wi), {}
            else:
                size = self._adaptive_out(Hi, Wi)
                more = dict(inBits=torch.zeros(C.cbinfer_mask_words(Hi, Wi), dtype=torch.int64, device=dev))
            return dict(mask_workspace(size[0], size[1], dev), size=size, **more)
        work = self._cached_work((Hi, Wi, dev), make)
        assert not isinstance(changeIndexes, torch.Tensor) or changeIndexes.dim() == 1
        if changeIndexes is None:      # (a pool always stands behind a producer)
            raise CBinferError(PROPAGATED['words'][1] % dict(name=self.__class__.__name__))
        return nc, Hi, Wi, work, operand_changes(self.__class__.__name__, 'pool', changeIndexes, Hi, Wi, dev, work['idx'],
                                                 **PROPAGATED)

    def _forward_general(self, input, changeIndexes):
        """A frame on cb_pool2d.hip: cbinfer_cbpool2d_forward, two launches, no host sync.  The output pixels whose
        window holds a listed input pixel are pooled again; the list handed on lives on the OUTPUT map."""
        nc, Hi, Wi, work, (mask, idx, cap, count) = self._frame(input, changeIndexes)
        Ho, Wo = work['size']
        self._fresh_state((1, nc, Ho, Wo), input, fill=float('inf'))      # (and the frame still goes by the list)
        check(C.cbinfer_cbpool2d_forward(ptr(input), ptr(self.outputState), ptr(idx), cap, ptr(count), ptr(mask),
                                         ptr(work['bits']), ptr(work['copy']), nc, Hi, Wi, self._pool_struct(),
                                         dtype_code(input), stream_ptr(input)))
        # (an input-resolution list means nothing behind such a pool: downsampleIndexes is ignored)
        return self._result(work, Ho, Wo)

    def _forward_adaptive(self, input, changeIndexes):
        """A frame on cb_adaptpool.hip: cbinfer_cbadaptivepool2d_forward, two launches (three for a list), no host sync.
        The row-segment partials that hold a listed input pixel are made again, then the output pixels whose window
        does; the mask handed on lives on the OUTPUT map.  A frame whose state does not fit lists every pixel."""
        nc, Hi, Wi, work, form = self._frame(input, changeIndexes)
        oh, ow = work['size']
        if not (state_fits(self.outputState, (1, nc, oh, ow), input) and
                state_fits(self.partials, (nc, ow, Hi), input, dtype=torch.float32)):
            self.outputState = torch.empty((1, nc, oh, ow), dtype=input.dtype, device=input.device)
            self.partials = torch.empty((nc, ow, Hi), dtype=torch.float32, device=input.device)
            form = EVERY_PIXEL      # (a new state is written completely: the operand's change information is not used)
        check(C.cbinfer_cbadaptivepool2d_forward(ptr(input), ptr(self.partials), ptr(self.outputState), *form_args(form),
                                                 ptr(work['inBits']), ptr(work['bits']), ptr(work['copy']), nc, Hi, Wi,
                                                 oh, ow, self._op, dtype_code(input), stream_ptr(input)))
        return self._result(work, oh, ow)

    def _forward_suppress(self, inp):
        """A frame on cb_peaks.hip: cbinfer_cbpeaks_forward -- one launch, two for a list -- and, with a peak list,
        cbinfer_peaks_list (three more); no host sync.  The pixels of the k x k footprint of the operand's changes are
        judged again; the mask handed on is that footprint.  A frame whose state does not fit lists every pixel."""
        name = self.__class__.__name__
        if torch.is_tensor(inp):
            input, changeIndexes = inp.detach().contiguous(), None
        else:
            assert type(inp) == tuple and inp[0] == 'changeIndexes'
            input, changeIndexes = inp[1].detach().contiguous(), inp[2]
            if changeIndexes is None:
                raise CBinferError(PROPAGATED['words'][1] % dict(name=name))
        check_map(name, input)
        require_device(input)
        nc, H, W = input.size(1), input.size(2), input.size(3)
        dev, N = input.device, self.peakCapacity
        words = C.cbinfer_mask_words(H, W)

        def make():
            more = {}
            if N:
                more = dict(peakEntries=torch.zeros((N, 3), dtype=torch.int32, device=dev),
                            peakScores=torch.zeros(N, dtype=input.dtype, device=dev),
                            peakCount=torch.zeros(1, dtype=torch.int32, device=dev),
                            peakStart=torch.zeros(nc + 1, dtype=torch.int32, device=dev),
                            peakScan=torch.zeros(nc * H + 1, dtype=torch.int32, device=dev))
            k = self.kernel_size
            peaks = _lib.Peaks(k[0], k[1], int(self.suppress == 'cross'), int(self.floor is not None), self.floor or 0.0)
            return dict(mask_workspace(H, W, dev), size=(H, W), peaks=ctypes.pointer(peaks), **more)
        work = self._cached_work((nc, H, W, dev, input.dtype), make)
        form = EVERY_PIXEL
        if changeIndexes is not None:
            form = operand_changes(name, 'pool', changeIndexes, H, W, dev, work['idx'], **PROPAGATED)
        if not (state_fits(self.outputState, (1, nc, H, W), input) and
                state_fits(self.peakBits, (nc * words,), input, dtype=torch.int64)):
            self.outputState = torch.empty((1, nc, H, W), dtype=input.dtype, device=dev)
            self.peakBits = torch.zeros(nc * words, dtype=torch.int64, device=dev)
            form = EVERY_PIXEL      # (a new state is written completely: the operand's change information is not used)
        check(C.cbinfer_cbpeaks_forward(ptr(input), ptr(self.outputState), ptr(self.peakBits), *form_args(form),
                                        ptr(work['bits']), ptr(work['copy']), nc, H, W, work['peaks'],
                                        dtype_code(input), stream_ptr(input)))
        if N:
            check(C.cbinfer_peaks_list(ptr(input), ptr(self.peakBits), ptr(work['peakScan']), ptr(work['peakEntries']),
                                       ptr(work['peakScores']), N, ptr(work['peakCount']), ptr(work['peakStart']), nc, H,
                                       W, dtype_code(input), stream_ptr(input)))
        return self._result(work, H, W)

    def peakList(self):
        """(entries int32 [N, 3] of (c, y, x), scores [N], count [1], channelStart [C + 1]) of the last frame, device
        tensors that keep their addresses from frame to frame; no host sync.  Ascending in (c, y, x); count and
        channelStart are the true numbers, also where the list holds only its first N entries."""
        work = self.__dict__.get(self._WORK)
        if not self.__dict__.get('peakCapacity'):
            raise CBinferError("%s: no peak list is made: construct the module with suppress= and peakList=N > 0"
                               % self.__class__.__name__)
        if work is None or 'peakEntries' not in work:
            raise CBinferError("%s: the peak list is there after the first frame" % self.__class__.__name__)
        return work['peakEntries'], work['peakScores'], work['peakCount'], work['peakStart']

    def peaksToHost(self):
        """The last frame's peaks on the host, one list per channel of (x, y, score) -- what the reference's pose
        detector keeps as all_peaks.  Waits for the device; CBinferError if the frame had more peaks than peakList=N."""
        entries, scores, count, start = (t.cpu() for t in self.peakList())
        n = int(count.item())
        if n > self.peakCapacity:
            raise CBinferError("%s: the frame has %d peaks, the list holds peakList=%d" % (self.__class__.__name__, n,
                                                                                           self.peakCapacity))
        start, entries, scores = start.tolist(), entries.tolist(), scores.tolist()
        return [[(entries[i][2], entries[i][1], scores[i]) for i in range(a, b)] for a, b in zip(start[:-1], start[1:])]

    def forward(self, inp):
        if self.__dict__.get('suppress') is not None:
            return self._forward_suppress(inp)
        if torch.is_tensor(inp):      # (as for every CBStateModule, a bare tensor lists every pixel)
            inp = 'changeIndexes', inp, torch.arange(inp.size(-2) * inp.size(-1), dtype=torch.int32, device=inp.device)
        assert type(inp) == tuple and inp[0] == 'changeIndexes'
        input = inp[1].detach().contiguous()
        changeIndexes = inp[2]
        require_device(input)
        if self.__dict__.get('_adaptive'):
            return self._forward_adaptive(input, changeIndexes)
        if self.__dict__.get('_general'):
            return self._forward_general(input, changeIndexes)
        nc, h, w = input.size(-3), input.size(-2), input.size(-1)
        oh, ow = ((h - 1) // 2 + 1, (w - 1) // 2 + 1) if self.ceil_mode else (h // 2, w // 2)
        if getattr(self, 'lazy', False) and not self.propChangeIndexes:
            return LazyPool(input, (1, nc, oh, ow), self.ceil_mode, changeIndexes)
        exact = isinstance(changeIndexes, torch.Tensor)
        if exact:
            changeIndexes = changeIndexes.detach().contiguous()
            assert changeIndexes.dim() == 1
        if not exact or changeIndexes.numel() != 0:
            self._fresh_state((1, nc, oh, ow), input, fill=float('inf'))
            maxPool2d(input, self.outputState, changeIndexes, self.kernel_size, self.stride)
        output = frame_output(self, self.outputState)
        if not self.propChangeIndexes:
            return output
        if getattr(self, 'downsampleIndexes', False):
            return 'changeIndexes', output, poolChangeIndexes(changeIndexes, (h, w), (output.size(-2), output.size(-1)))
        return 'changeIndexes', output, inp[2]

    def __repr__(self):
        if self.__dict__.get('suppress') is not None:
            return ('%s (k=%s, suppress=%s, floor=%s, peakList=%d, propChgIdxs=%s)' %
                    (self.__class__.__name__, self.kernel_size, self.suppress, self.floor, self.peakCapacity,
                     self.propChangeIndexes))
        if self.__dict__.get('_adaptive'):
            return '%s (output_size=%s, propChgIdxs=%s)' % (self.__class__.__name__, self.output_size,
                                                            self.propChangeIndexes)
        if self.__dict__.get('generalGeometry'):
            return ('%s (k=%s, s=%s, p=%s, ceil_mode=%s, propChgIdxs=%s)' %
                    (self.__class__.__name__, self.kernel_size, self.stride, self.padding, self.ceil_mode,
                     self.propChangeIndexes))
        return ('%s (k=%s, s=%s, ceil_mode=%s, propChgIdxs=%s)' %
                (self.__class__.__name__, self.kernel_size, self.stride, self.ceil_mode,
                 self.propChangeIndexes))


class CBPoolAvg2d(CBPoolMax2d):
    """Change-based average pooling of an nn.AvgPool2d (no counterpart in the reference): any window, stride, zero
    padding, ceil_mode and count_include_pad within the library's limits, 2x2 included (cb_pool2d.hip);
    and of an nn.AdaptiveAvgPool2d of any output size up to the map's (cb_adaptpool.hip).
    The surface is CBPoolMax2d's: propChangeIndexes, cloneOutput, outputState, clearMemory, getStateTensors.  Never
    folded into a consumer's detection (lazy stays False)."""
    _KIND = 'avg'

    def __init__(self, m, suppress=None, floor=None, peakList=0):
        for name, v, given in (('suppress', suppress, suppress is not None), ('floor', floor, floor is not None),
                               ('peakList', peakList, peakList != 0)):
            if given:
                raise CBinferError("CBPoolAvg2d: %s=%r is not supported (peak suppression is CBPoolMax2d's)" % (name, v))
        super(CBPoolAvg2d, self).__init__(m, generalGeometry=True)
        self.count_include_pad = bool(getattr(m, 'count_include_pad', True))

    def __setstate__(self, state):
        super(CBPoolAvg2d, self).__setstate__(state)
        self.__dict__['generalGeometry'] = self.__dict__['_general'] = True

    def __repr__(self):
        if self.__dict__.get('_adaptive'):
            return super(CBPoolAvg2d, self).__repr__()
        return ('%s (k=%s, s=%s, p=%s, ceil_mode=%s, count_include_pad=%s, propChgIdxs=%s)' %
                (self.__class__.__name__, self.kernel_size, self.stride, self.padding, self.ceil_mode,
                 self.count_include_pad, self.propChangeIndexes))


def suppression_formula(x, kernel_size, suppress, floor=None):
    """Peak suppression of a [1, C, H, W] tensor in dense torch operators, the rule of DESIGN 5.31: 'window' as
    torch.where((F.max_pool2d(x, k, 1, k // 2) == x) & (x >= floor), x, 0); 'cross' as four comparisons with the
    neighbours of a map padded with -inf.  What insertCBPooling(nmsTypes=...) holds a user's class against."""
    k = _pool_pair(kernel_size, 'kernel_size')
    if suppress == 'cross':
        p = F.pad(x, (1, 1, 1, 1), value=float('-inf'))
        H, W = x.shape[-2:]
        keep = x == x
        for dy, dx in ((0, 1), (2, 1), (1, 0), (1, 2)):
            keep = keep & (x >= p[..., dy:dy + H, dx:dx + W])
    else:
        keep = F.max_pool2d(x, k, 1, (k[0] // 2, k[1] // 2)) == x
    if floor is not None:
        keep = keep & (x >= floor)
    return torch.where(keep, x, torch.zeros_like(x))


def computes_suppression(m, kernel_size, suppress, floor=None):
    """Whether the user's module `m` computes suppression_formula: both on one small random CPU tensor in float32,
    equal bit for bit.  The tensor holds four levels (plateaus, exact ties) around the floor and three 8 x 8 plateaus
    whose inner pixels are maxima of every window up to 7 x 7: one well below the floor, one a single float32 step
    below it, one exactly at it.  A forward that raises does not."""
    import copy
    ref = copy.deepcopy(m).cpu().float().eval()
    base = torch.tensor(0.0 if floor is None else float(floor), dtype=torch.float32)
    q = torch.randint(0, 4, (1, 3, 24, 24), generator=torch.Generator().manual_seed(7)).float()
    x = base + (q - 1.0) * 0.5
    x[..., 0:8, 0:8] = base - 0.5
    x[..., 16:24, 0:8] = torch.nextafter(base, torch.tensor(float('-inf')))
    x[..., 0:8, 16:24] = base
    with torch.no_grad():
        want = suppression_formula(x, kernel_size, suppress, floor)
        try:
            got = ref(x.clone())
        except Exception:
            return False
    return torch.is_tensor(got) and got.shape == want.shape and got.dtype == want.dtype and \
        torch.equal(got.view(torch.int32), want.view(torch.int32))
