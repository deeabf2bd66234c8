"""Change-based transposed convolution: CBConvTranspose2d and insertCBTransposedConv (cb_tconv.hip).

The reference has no such operator.  An nn.ConvTranspose2d -- the learned upsampling of U-Net (2x2 / stride 2), of
segmentation and depth decoders and DCGAN-type generators (4x4 / stride 2 / padding 1) and of torchvision-style decoders
(3x3 / stride 2 / padding 1 / output_padding 1) -- ends a change-based chain: torch recomputes the whole map at the
largest resolutions of the network, drops the producer's change mask and cannot be recorded by a FrameProgram.  The
module runs the layer's own change detection on its input (component a1's rule with `threshold`), recomputes exactly the
output pixels that read a changed input pixel and leaves every other output pixel bit for bit as it was.
"""
import ctypes

import torch
import torch.nn as nn

from . import _lib
from ._lib import C, CBinferError, check, dtype_code, ptr, require_device, stream_ptr
from .chain import hand_back, later_producer_types, producer_types
from .conv2d import CBConv2d, _same_shape, _switch

MAX_K, MAX_S, MAX_D = 8, 4, 4


def _check_transposed(m):
    """(kernel_size, stride, padding, dilation, output_padding) as pairs of ints if the library takes the module `m`;
    CBinferError with a sentence naming the setting otherwise."""
    Err = CBinferError
    if not isinstance(m, nn.ConvTranspose2d):
        raise Err("CBConvTranspose2d: only nn.ConvTranspose2d modules are converted, got %s" % type(m).__name__)
    if m.groups != 1:
        raise Err("CBConvTranspose2d: groups=%d is not supported, only groups=1" % m.groups)
    if getattr(m, 'padding_mode', 'zeros') != 'zeros':
        raise Err("CBConvTranspose2d: padding_mode=%r is not supported, only 'zeros'" % (m.padding_mode,))
    k, s, p, d, op = (tuple(int(v) for v in t) for t in (m.kernel_size, m.stride, m.padding, m.dilation,
                                                         m.output_padding))
    for i in (0, 1):
        if k[i] > MAX_K:
            raise Err("CBConvTranspose2d: kernel_size=%s is beyond what the library takes (<= %d per axis)" % (k, MAX_K))
        if s[i] > MAX_S:
            raise Err("CBConvTranspose2d: stride=%s is beyond what the library takes (<= %d per axis)" % (s, MAX_S))
        if d[i] > MAX_D:
            raise Err("CBConvTranspose2d: dilation=%s is beyond what the library takes (<= %d per axis)" % (d, MAX_D))
        if not 0 <= p[i] <= d[i] * (k[i] - 1):
            raise Err("CBConvTranspose2d: padding=%s is beyond what the library takes (0 <= padding <= dilation * "
                      "(kernel_size - 1) per axis, kernel_size=%s dilation=%s)" % (p, k, d))
        if not 0 <= op[i] < max(s[i], d[i]):
            raise Err("CBConvTranspose2d: output_padding=%s must be smaller than max(stride, dilation) per axis "
                      "(stride=%s dilation=%s)" % (op, s, d))
    g = _lib.TGeom(k[0], k[1], s[0], s[1], p[0], p[1], d[0], d[1], op[0], op[1])
    if C.cbinfer_tconv_prepared_weights_bytes(m.out_channels, m.in_channels, ctypes.byref(g), _lib.CB_F32) <= 0:
        raise Err("CBConvTranspose2d: kernel_size=%s stride=%s padding=%s dilation=%s output_padding=%s is beyond what "
                  "the library takes" % (k, s, p, d, op))
    return k, s, p, d, op


class CBConvTranspose2d(nn.Module):
    """Change-based nn.ConvTranspose2d (no counterpart in the reference): per axis kernel_size <= 8, stride <= 4,
    dilation <= 4, 0 <= padding <= dilation (kernel_size - 1), output_padding < max(stride, dilation); groups 1, with or
    without bias, batch 1, fp32 or fp16.  The parameters are shared with the source module.

    forward(x): a [1, C, Hi, Wi] tensor or the ('changeIndexes', tensor, indexes) tuple of a producer -- the indexes are
    ignored, the layer always runs its own detection on the tensor.  Flags as on CBConv2d: threshold, feedbackLoop,
    copyInput, withReLU, exactF32, propChangeIndexes (hands on the frame's change mask on the OUTPUT map as a
    MaskChangeIndexes); cloneOutput=False hands out prevOutput itself, tagged, and the frame is then free of torch
    operators.  Output pixels no tap reaches (a phase without a tap: kernel_size < stride, 1x1 stride 2; rows and columns
    added by output_padding) hold relu(bias), or 0, from the moment the state is allocated and are never written."""

    def __init__(self, m, threshold):
        super(CBConvTranspose2d, self).__init__()
        (self.kernel_size, self.stride, self.padding, self.dilation, self.output_padding) = _check_transposed(m)
        self.groups = m.groups
        self.transposed = True
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
        """(pointer to) the layer's cbTGeom; transient, made again after unpickling."""
        if self.__dict__.get('_geomC') is None:
            k, s, p, d, op = self.kernel_size, self.stride, self.padding, self.dilation, self.output_padding
            self.__dict__['_geomC'] = ctypes.pointer(_lib.TGeom(k[0], k[1], s[0], s[1], p[0], p[1], d[0], d[1],
                                                                op[0], op[1]))
        return self.__dict__['_geomC']

    def _out_hw(self, Hi, Wi):
        Ho, Wo = ctypes.c_int(), ctypes.c_int()
        if C.cbinfer_tconv_out_size(Hi, Wi, self._struct(), ctypes.byref(Ho), ctypes.byref(Wo)) != 0:
            raise CBinferError("CBConvTranspose2d: a %dx%d map has no output (kernel_size=%s stride=%s padding=%s "
                               "dilation=%s output_padding=%s)" % (Hi, Wi, self.kernel_size, self.stride, self.padding,
                                                                   self.dilation, self.output_padding))
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
        """Frame masks (zero once), their mask-copy view, index buffer and count for a consumer that wants the list, the
        split-k workspace: once per map size."""
        key = (Hi, Wi, dev)
        work = self.__dict__.get('_work')
        if work is None or work['key'] != key:
            Ho, Wo = self._out_hw(Hi, Wi)
            bits = torch.zeros(C.cbinfer_frame_mask_bytes(Ho, Wo) // 8, dtype=torch.int64, device=dev)
            off = C.cbinfer_frame_mask_copy_offset(Ho, Wo) // 8
            work = self.__dict__['_work'] = dict(
                key=key, size=(Ho, Wo), bits=bits, copy=bits[off:off + C.cbinfer_mask_words(Ho, Wo)],
                idx=torch.empty(Ho * Wo, dtype=torch.int32, device=dev),
                count=torch.zeros(1, dtype=torch.int32, device=dev),
                conv=torch.zeros(C.cbinfer_tconv_workspace_bytes(), dtype=torch.uint8, device=dev))
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
            Cin, K = w.size(0), w.size(1)
            g = self._struct()
            wp = torch.empty(C.cbinfer_tconv_prepared_weights_bytes(K, Cin, g, arith), dtype=torch.uint8, device=w.device)
            check(C.cbinfer_tconv_prep_weights(ptr(w.detach().contiguous()), ptr(wp), K, Cin, Hi, Wi, g, arith,
                                               stream_ptr(w)))
            wprep = self.__dict__['_wprep'] = (key, wp)
        return wprep[1]

    # ---------------------------------------------------------------- frame
    def forward(self, inp):
        if type(inp) == tuple:
            if len(inp) != 3 or inp[0] != 'changeIndexes':
                raise CBinferError("CBConvTranspose2d: the input is a tuple, but not ('changeIndexes', tensor, indexes)")
            inp = inp[1]      # (the indexes address the input map; the layer runs its own detection)
        if not torch.is_tensor(inp):
            raise CBinferError("CBConvTranspose2d: the input must be a tensor or the ('changeIndexes', tensor, indexes) "
                               "tuple, got %s" % type(inp).__name__)
        live = bool(getattr(inp, '_cbinfer_inplace_state', False))
        x = inp.detach().contiguous()
        if x.dim() != 4 or x.size(0) != 1 or x.size(1) != self.in_channels:
            raise CBinferError("CBConvTranspose2d: the input must be a [1, %d, H, W] tensor, got %s"
                               % (self.in_channels, tuple(x.shape)))
        require_device(x)
        if x.dtype != self.weight.dtype or x.device != self.weight.device:
            raise CBinferError("CBConvTranspose2d: input (%s on %s) and weights (%s on %s) differ in dtype or device"
                               % (x.dtype, x.device, self.weight.dtype, self.weight.device))
        arith = self._arith(x)
        Cin, K, Hi, Wi = self.in_channels, self.out_channels, x.size(2), x.size(3)
        work = self._workspace(Hi, Wi, x.device)
        Ho, Wo = work['size']
        self._state_for(x, Ho, Wo)
        if not self.prevInput.is_contiguous():
            self.prevInput = self.prevInput.contiguous()
        bias = self.bias.detach() if self.bias is not None else None
        check(C.cbinfer_cbconvtranspose2d_forward(
            ptr(x), ptr(self.prevInput), ptr(self.prevOutput), ptr(work['bits']), ptr(self._weights(Hi, Wi, arith)),
            ptr(bias), Cin, Hi, Wi, K, self._struct(), float(self.threshold), int(bool(self.feedbackLoop)),
            int(bool(self.copyInput)), int(bool(self.withReLU)), ptr(work['conv']), arith, stream_ptr(x)))
        if not self.feedbackLoop and not self.copyInput:
            self.prevInput = x.clone() if live else x
        return hand_back(self, self.prevOutput, work['copy'], (Ho, Wo), work)

    def __repr__(self):
        return ('CBConvTranspose2d (%d, %d, k=%s, s=%s, p=%s, d=%s, op=%s, th=%s, withReLU=%s, propChgIdxs=%s)'
                % (self.in_channels, self.out_channels, self.kernel_size, self.stride, self.padding, self.dilation,
                   self.output_padding, self.threshold, self.withReLU, self.propChangeIndexes))


def insertCBTransposedConv(rootModule, threshold=1e-1, cloneOutput=True):
    """Inside every nn.Sequential of rootModule, an nn.ConvTranspose2d within the library's limits that directly follows
    a CBConv2d, CBPoolMax2d, CBPoolAvg2d, CBAdd2d, CBResidual, CBUpsample2d, CBPixelShuffle2d, CBChannelShuffle2d or
    another CBConvTranspose2d becomes a
    CBConvTranspose2d with `threshold` (it runs its own change detection: nothing is switched on at the producer).  An
    nn.ReLU right behind it is absorbed (withReLU).  A CBConv2d consuming the output then needs its own input copy
    (copyInput) unless it runs in feedback mode.  A module beyond the limits stays the dense torch operator.  Returns
    rootModule."""
    for seq in [m for m in rootModule.modules() if type(m) == nn.Sequential]:
        names = list(seq._modules.keys())
        gone = set()
        for pos in range(1, len(names)):
            prod, tc = seq._modules[names[pos - 1]], seq._modules[names[pos]]
            if names[pos - 1] in gone and pos >= 2:
                prod = seq._modules[names[pos - 2]]
            if type(prod) not in producer_types() + later_producer_types() or type(tc) != nn.ConvTranspose2d:
                continue
            try:
                cb = CBConvTranspose2d(tc, threshold)
            except CBinferError:
                continue      # (beyond the limits: stays dense)
            cb.cloneOutput = cloneOutput
            seq._modules[names[pos]] = cb
            nxt = pos + 1
            if nxt < len(names) and type(seq._modules[names[nxt]]) == nn.ReLU:
                cb.withReLU = True
                gone.add(names[nxt])
                nxt += 1
            if nxt < len(names):
                consumer = seq._modules[names[nxt]]
                if type(consumer) == CBConv2d and not consumer.feedbackLoop:
                    consumer.copyInput = True
        for name in gone:
            del seq._modules[name]
    return rootModule
