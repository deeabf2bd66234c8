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
from ._lib import C, CBinferError, check, ptr, stream_ptr
from .chain import hand_back, link_consumer, producers
from .layer import CBContractingLayer, check_limits

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
    limits = [('kernel_size', k, MAX_K), ('stride', s, MAX_S), ('dilation', d, MAX_D)]
    for i in (0, 1):      # (axis by axis: the two range rules of an axis come before the next axis' limits)
        check_limits('CBConvTranspose2d', limits, (i,))
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


class CBConvTranspose2d(CBContractingLayer):
    """Change-based nn.ConvTranspose2d (no counterpart in the reference): per axis kernel_size <= 8, stride <= 4,
    dilation <= 4, 0 <= padding <= dilation (kernel_size - 1), output_padding < max(stride, dilation); groups 1, with or
    without bias, batch 1, fp32 or fp16.  The parameters are shared with the source module.

    forward(x): a [1, C, Hi, Wi] tensor or the ('changeIndexes', tensor, indexes) tuple of a producer -- the indexes are
    ignored, the layer always runs its own detection on the tensor.  Flags as on CBConv2d: threshold, feedbackLoop,
    copyInput, withReLU, exactF32, propChangeIndexes (hands on the frame's change mask on the OUTPUT map as a
    MaskChangeIndexes); cloneOutput=False hands out prevOutput itself, tagged, and the frame is then free of torch
    operators.  Output pixels no tap reaches (a phase without a tap: kernel_size < stride, 1x1 stride 2; rows and columns
    added by output_padding) hold relu(bias), or 0, from the moment the state is allocated and are never written."""
    _GEOM = _lib.TGeom
    _GEOM_FIELDS = ('kernel_size', 'stride', 'padding', 'dilation', 'output_padding')
    _OUT_SIZE = C.cbinfer_tconv_out_size

    def __init__(self, m, threshold):
        super(CBConvTranspose2d, self).__init__(m, threshold, _check_transposed(m))
        self.transposed = True

    def _no_output(self, Hi, Wi):
        return ("CBConvTranspose2d: a %dx%d map has no output (kernel_size=%s stride=%s padding=%s dilation=%s "
                "output_padding=%s)" % (Hi, Wi, self.kernel_size, self.stride, self.padding, self.dilation,
                                        self.output_padding))

    def _prepare(self, w, Hi, Wi, arith):
        Cin, K, g = w.size(0), w.size(1), self._struct()
        wp = torch.empty(C.cbinfer_tconv_prepared_weights_bytes(K, Cin, g, arith), dtype=torch.uint8, device=w.device)
        check(C.cbinfer_tconv_prep_weights(ptr(w), ptr(wp), K, Cin, Hi, Wi, g, arith, stream_ptr(w)))
        return wp

    def _buffers_for(self, Ho, Wo, dev):
        """The base's, and the split-k workspace."""
        return dict(super(CBConvTranspose2d, self)._buffers_for(Ho, Wo, dev),
                    conv=torch.zeros(C.cbinfer_tconv_workspace_bytes(), dtype=torch.uint8, device=dev))

    # ---------------------------------------------------------------- frame
    def forward(self, inp):
        x, _, live = self._operand(inp)      # (the indexes address the input map; the layer runs its own detection)
        arith = self._arith(x)
        Cin, K, Hi, Wi = self.in_channels, self.out_channels, x.size(2), x.size(3)
        work = self._workspace(Hi, Wi, x.device)
        Ho, Wo = work['size']
        self._state_for(x, Ho, Wo)
        bias = self.bias.detach() if self.bias is not None else None
        check(C.cbinfer_cbconvtranspose2d_forward(
            ptr(x), ptr(self.prevInput), ptr(self.prevOutput), ptr(work['bits']), ptr(self._weights(Hi, Wi, arith)),
            ptr(bias), Cin, Hi, Wi, K, self._struct(), float(self.threshold), int(bool(self.feedbackLoop)),
            int(bool(self.copyInput)), int(bool(self.withReLU)), ptr(work['conv']), arith, stream_ptr(x)))
        self._keep_input(x, live)
        return hand_back(self, self.prevOutput, work['copy'], (Ho, Wo), work)

    def __repr__(self):
        return ('CBConvTranspose2d (%d, %d, k=%s, s=%s, p=%s, d=%s, op=%s, th=%s, withReLU=%s, propChgIdxs=%s)'
                % (self.in_channels, self.out_channels, self.kernel_size, self.stride, self.padding, self.dilation,
                   self.output_padding, self.threshold, self.withReLU, self.propChangeIndexes))


def insertCBTransposedConv(rootModule, threshold=1e-1, cloneOutput=True):
    """Inside every nn.Sequential of rootModule, an nn.ConvTranspose2d within the library's limits that directly follows
    a producer -- chain.producers('insertCBTransposedConv'), another CBConvTranspose2d among them -- becomes a
    CBConvTranspose2d with `threshold` (it runs its own change detection: nothing is switched on at the producer).  An
    nn.ReLU right behind it is absorbed (withReLU).  A CBConv2d consuming the output then needs its own input copy
    (copyInput) unless it runs in feedback mode (chain.link_consumer; the layer hands nothing on by itself).  A module
    beyond the limits stays the dense torch operator.  Returns rootModule."""
    for seq in [m for m in rootModule.modules() if type(m) is nn.Sequential]:
        names = list(seq._modules.keys())
        gone = set()
        for pos in range(1, len(names)):
            prod, tc = seq._modules[names[pos - 1]], seq._modules[names[pos]]
            if names[pos - 1] in gone and pos >= 2:
                prod = seq._modules[names[pos - 2]]
            if type(prod) not in producers('insertCBTransposedConv') or type(tc) != nn.ConvTranspose2d:
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
                link_consumer(cb, seq._modules[names[nxt]], handOn=False)
        for name in gone:
            del seq._modules[name]
    return rootModule
