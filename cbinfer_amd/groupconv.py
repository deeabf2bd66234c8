"""Change-based grouped convolution: CBGroupedConv2d and linkGrouped (cb_groupconv.hip).

The reference has no such operator.  A grouped nn.Conv2d (1 < groups < in_channels) -- the 3x3 layer of ResNeXt and
RegNet bottlenecks and of ShuffleNet units, the split layers of AlexNet-type networks -- ends a change-based chain:
CBConv2d refuses groups, torch recomputes the whole map, drops the producer's change mask and cannot be recorded by a
FrameProgram.  The module runs the layer's own change detection on its input (component a1's rule with `threshold`, over
all channels), recomputes exactly the output pixels that read a changed input pixel -- every group at those pixels --
and leaves every other output pixel bit for bit as it was.
"""
import ctypes

import torch
import torch.nn as nn

from . import _lib
from ._lib import C, CBinferError, check, dtype_code, ptr, require_device, stream_ptr
from .chain import hand_back, is_1x1
from .conv2d import CBConv2d, _padding_pair, _same_shape, _switch

MAX_K, MAX_S, MAX_D, MAX_P = 7, 4, 8, 64


def _check_grouped(m):
    """(kernel_size, stride, padding, dilation) as pairs of ints if the library takes the module `m`; CBinferError with
    a sentence naming the setting otherwise."""
    Err = CBinferError
    if not isinstance(m, nn.Conv2d) or m.transposed or tuple(m.output_padding) != (0, 0):
        raise Err("CBGroupedConv2d: only plain nn.Conv2d modules are converted, got %s" % type(m).__name__)
    if m.groups == 1:
        raise Err("CBGroupedConv2d: groups=1 is not a grouped convolution: use CBConv2d")
    if m.padding_mode != 'zeros':
        raise Err("CBGroupedConv2d: padding_mode=%r is not supported, only 'zeros'" % (m.padding_mode,))
    p = _padding_pair(m, 'CBGroupedConv2d')
    k, s, d = (tuple(int(v) for v in t) for t in (m.kernel_size, m.stride, m.dilation))
    for i in (0, 1):
        if k[i] > MAX_K:
            raise Err("CBGroupedConv2d: kernel_size=%s is beyond what the library takes (<= %d per axis)" % (k, MAX_K))
        if s[i] > MAX_S:
            raise Err("CBGroupedConv2d: stride=%s is beyond what the library takes (<= %d per axis)" % (s, MAX_S))
        if d[i] > MAX_D:
            raise Err("CBGroupedConv2d: dilation=%s is beyond what the library takes (<= %d per axis)" % (d, MAX_D))
        if p[i] > MAX_P:
            raise Err("CBGroupedConv2d: padding=%s is beyond what the library takes (<= %d per axis)" % (p, MAX_P))
    g = _lib.Geom(k[0], k[1], s[0], s[1], p[0], p[1], d[0], d[1])
    if not C.cbinfer_groupconv_supported(m.in_channels, m.out_channels, m.groups, ctypes.byref(g)):
        raise Err("CBGroupedConv2d: groups=%d in_channels=%d out_channels=%d kernel_size=%s stride=%s padding=%s "
                  "dilation=%s is beyond what the library takes" % (m.groups, m.in_channels, m.out_channels, k, s, p, d))
    return k, s, p, d


class CBGroupedConv2d(nn.Module):
    """Change-based grouped nn.Conv2d (no counterpart in the reference): groups >= 2 dividing in_channels and
    out_channels; per axis kernel_size <= 7, stride <= 4, dilation <= 8, padding <= 64 (ints, 'valid' or a symmetric
    'same'); with or without bias, batch 1, fp32 or fp16.  groups == in_channels is taken and correct, but
    CBDepthwiseConv2d is the fast path for it.  The parameters are shared with the source module.

    forward(x): a [1, C, Hi, Wi] tensor or the ('changeIndexes', tensor, indexes) tuple of a producer -- the indexes are
    ignored, the layer always runs its own detection on the tensor.  Flags as on CBConv2d: threshold, feedbackLoop,
    copyInput, withReLU, exactF32, propChangeIndexes (hands on the frame's change mask on the OUTPUT map as a
    MaskChangeIndexes); cloneOutput=False hands out prevOutput itself, tagged, and the frame is then free of torch
    operators.  Output pixels no tap reaches (padding > dilation (kernel_size - 1)) hold relu(bias), or 0, from the moment
    the state is allocated and are never written."""

    def __init__(self, m, threshold):
        super(CBGroupedConv2d, self).__init__()
        self.kernel_size, self.stride, self.padding, self.dilation = _check_grouped(m)
        self.groups = m.groups
        self.transposed = False
        self.in_channels = m.in_channels
        self.out_channels = m.out_channels
        self.weight = m.weight      # shared with the source module
        self.bias = m.bias
        self.threshold = threshold
        self.withReLU = False
        self.propChangeIndexes = False
        self.copyInput = True
        self.feedbackLoop = False
        self.exactF32 = False
        self.cloneOutput = True
        self.clearMemory()

    # ---------------------------------------------------------------- state
    def clearMemory(self):
        for name in ('prevInput', 'prevOutput'):
            if name not in self._buffers:
                self.register_buffer(name, self.weight.detach().new_zeros(0))
        self.prevInput = self.weight.detach().new_zeros(0)
        self.prevOutput = self.weight.detach().new_zeros(0)
        for name in ('_work', '_wprep', '_geomC'):      # (transient: device work buffers, ctypes arguments)
            self.__dict__[name] = None

    def getStateTensors(self):
        return [self.prevInput, self.prevOutput]

    def invalidateWeights(self):
        """Forget the cached prepared weights -- after a write through `weight.data`, which bumps neither the Parameter
        object nor its version counter."""
        self.__dict__['_wprep'] = None

    def __getstate__(self):
        d = dict(self.__dict__)
        d.update(_work=None, _wprep=None, _geomC=None)
        return d

    def _struct(self):
        """(pointer to) the layer's cbGeom; transient, made again after unpickling."""
        if self.__dict__.get('_geomC') is None:
            k, s, p, d = self.kernel_size, self.stride, self.padding, self.dilation
            self.__dict__['_geomC'] = ctypes.pointer(_lib.Geom(k[0], k[1], s[0], s[1], p[0], p[1], d[0], d[1]))
        return self.__dict__['_geomC']

    def _out_hw(self, Hi, Wi):
        Ho, Wo = ctypes.c_int(), ctypes.c_int()
        if C.cbinfer_geom_out_size(Hi, Wi, self._struct(), ctypes.byref(Ho), ctypes.byref(Wo)) != 0:
            raise CBinferError("CBGroupedConv2d: a %dx%d map is smaller than the filter's reach (kernel_size=%s, "
                               "dilation=%s, padding=%s)" % (Hi, Wi, self.kernel_size, self.dilation, self.padding))
        return Ho.value, Wo.value

    def _bias_map(self, size, like):
        """The dense value of an output pixel no tap reaches, broadcast over the map: the bias (0 without one), after
        the ReLU when withReLU.  The first frame overwrites every reachable pixel."""
        fill = torch.zeros(size, dtype=like.dtype, device=like.device)
        if self.bias is not None:
            b = self.bias.detach().to(device=like.device, dtype=like.dtype)
            fill += (torch.relu(b) if self.withReLU else b).view(1, -1, 1, 1)
        return fill

    def _state_for(self, input, Ho, Wo):
        """(Re)allocate the state on a new resolution, dtype or device: prevInput +inf -- the first frame of a sequence
        is dense through the same kernels, every input pixel changed."""
        if (not _same_shape(self.prevInput, input.size()) or self.prevInput.dtype != input.dtype or
                self.prevInput.device != input.device):
            self.prevInput = torch.full(input.size(), float('inf'), dtype=input.dtype, device=input.device)
        size = (1, self.out_channels, Ho, Wo)
        if (not _same_shape(self.prevOutput, size) or self.prevOutput.dtype != input.dtype or
                self.prevOutput.device != input.device):
            self.prevOutput = self._bias_map(size, input)

    def _workspace(self, Hi, Wi, dev):
        """Frame masks (zero once), their mask-copy view, index buffer and count of the frame's list: once per map
        size."""
        key = (Hi, Wi, dev)
        work = self.__dict__.get('_work')
        if work is None or work['key'] != key:
            Ho, Wo = self._out_hw(Hi, Wi)
            bits = torch.zeros(C.cbinfer_frame_mask_bytes(Ho, Wo) // 8, dtype=torch.int64, device=dev)
            off = C.cbinfer_frame_mask_copy_offset(Ho, Wo) // 8
            work = self.__dict__['_work'] = dict(
                key=key, size=(Ho, Wo), bits=bits, copy=bits[off:off + C.cbinfer_mask_words(Ho, Wo)],
                idx=torch.empty(Ho * Wo, dtype=torch.int32, device=dev),
                count=torch.zeros(1, dtype=torch.int32, device=dev))
        return work

    def _arith(self, t):
        if dtype_code(t) == _lib.CB_F16:
            return _lib.CB_F16
        return _lib.CB_F32 if (self.exactF32 or _switch('CBINFER_EXACT_F32')) else _lib.CB_F32S

    def _weights(self, Hi, Wi, arith):
        w = self.weight
        key = (w.data_ptr(), w._version, w.dtype, w.device, Hi, Wi, arith)
        wprep = self.__dict__.get('_wprep')
        if wprep is None or wprep[0] != key:
            K, Cin, G, g = self.out_channels, self.in_channels, self.groups, self._struct()
            wp = torch.empty(C.cbinfer_groupconv_prepared_weights_bytes(K, Cin, G, g, arith), dtype=torch.uint8,
                             device=w.device)
            check(C.cbinfer_groupconv_prep_weights(ptr(w.detach().contiguous()), ptr(wp), K, Cin, G, Hi, Wi, g, arith,
                                                   stream_ptr(w)))
            wprep = self.__dict__['_wprep'] = (key, wp)
        return wprep[1]

    # ---------------------------------------------------------------- frame
    def forward(self, inp):
        if type(inp) == tuple:
            if len(inp) != 3 or inp[0] != 'changeIndexes':
                raise CBinferError("CBGroupedConv2d: the input is a tuple, but not ('changeIndexes', tensor, indexes)")
            inp = inp[1]      # (the layer runs its own detection)
        if not torch.is_tensor(inp):
            raise CBinferError("CBGroupedConv2d: the input must be a tensor or the ('changeIndexes', tensor, indexes) "
                               "tuple, got %s" % type(inp).__name__)
        live = bool(getattr(inp, '_cbinfer_inplace_state', False))
        x = inp.detach().contiguous()
        if x.dim() != 4 or x.size(0) != 1 or x.size(1) != self.in_channels:
            raise CBinferError("CBGroupedConv2d: the input must be a [1, %d, H, W] tensor, got %s"
                               % (self.in_channels, tuple(x.shape)))
        require_device(x)
        if x.dtype != self.weight.dtype or x.device != self.weight.device:
            raise CBinferError("CBGroupedConv2d: input (%s on %s) and weights (%s on %s) differ in dtype or device"
                               % (x.dtype, x.device, self.weight.dtype, self.weight.device))
        arith = self._arith(x)
        Cin, K, Hi, Wi = self.in_channels, self.out_channels, x.size(2), x.size(3)
        work = self._workspace(Hi, Wi, x.device)
        Ho, Wo = work['size']
        self._state_for(x, Ho, Wo)
        if not self.prevInput.is_contiguous():
            self.prevInput = self.prevInput.contiguous()
        bias = self.bias.detach() if self.bias is not None else None
        check(C.cbinfer_cbgroupconv2d_forward(
            ptr(x), ptr(self.prevInput), ptr(self.prevOutput), ptr(work['bits']), ptr(work['idx']), ptr(work['count']),
            ptr(self._weights(Hi, Wi, arith)), ptr(bias), Cin, Hi, Wi, K, self.groups, self._struct(),
            float(self.threshold), int(bool(self.feedbackLoop)), int(bool(self.copyInput)), int(bool(self.withReLU)),
            arith, stream_ptr(x)))
        if not self.feedbackLoop and not self.copyInput:
            self.prevInput = x.clone() if live else x
        # (the contraction left the frame's list and count in work['idx'] / work['count']: made)
        return hand_back(self, self.prevOutput, work['copy'], (Ho, Wo), work, made=True)

    def __repr__(self):
        return ('CBGroupedConv2d (%d, %d, groups=%d, k=%s, s=%s, p=%s, d=%s, th=%s, withReLU=%s, propChgIdxs=%s)'
                % (self.in_channels, self.out_channels, self.groups, self.kernel_size, self.stride, self.padding,
                   self.dilation, self.threshold, self.withReLU, self.propChangeIndexes))


def linkGrouped(rootModule):
    """Inside every nn.Sequential of rootModule: a CBGroupedConv2d directly in front of a 1x1 / stride-1 / padding-0
    CBConv2d hands its changes on (propChangeIndexes); any other CBConv2d directly behind a CBGroupedConv2d needs its own
    input copy (copyInput) unless it runs in feedback mode.  Returns rootModule."""
    for seq in [m for m in rootModule.modules() if type(m) == nn.Sequential]:
        kids = list(seq.children())
        for prod, cons in zip(kids[:-1], kids[1:]):
            if type(prod) is not CBGroupedConv2d:
                continue
            if is_1x1(cons):
                prod.propChangeIndexes = True
            elif type(cons) is CBConv2d and not cons.feedbackLoop:
                cons.copyInput = True
    return rootModule
