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
from ._lib import C, CBinferError, check, ptr, stream_ptr
from .chain import hand_back, link_consumer
from .conv2d import _padding_pair
from .layer import CBContractingLayer, check_limits

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
    check_limits('CBGroupedConv2d', [('kernel_size', k, MAX_K), ('stride', s, MAX_S), ('dilation', d, MAX_D),
                                     ('padding', p, MAX_P)])
    g = _lib.Geom(k[0], k[1], s[0], s[1], p[0], p[1], d[0], d[1])
    if not C.cbinfer_groupconv_supported(m.in_channels, m.out_channels, m.groups, ctypes.byref(g)):
        raise Err("CBGroupedConv2d: groups=%d in_channels=%d out_channels=%d kernel_size=%s stride=%s padding=%s "
                  "dilation=%s is beyond what the library takes" % (m.groups, m.in_channels, m.out_channels, k, s, p, d))
    return k, s, p, d


class CBGroupedConv2d(CBContractingLayer):
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
        super(CBGroupedConv2d, self).__init__(m, threshold, _check_grouped(m))

    def _prepare(self, w, Hi, Wi, arith):
        K, Cin, G, g = self.out_channels, self.in_channels, self.groups, self._struct()
        wp = torch.empty(C.cbinfer_groupconv_prepared_weights_bytes(K, Cin, G, g, arith), dtype=torch.uint8,
                         device=w.device)
        check(C.cbinfer_groupconv_prep_weights(ptr(w), ptr(wp), K, Cin, G, Hi, Wi, g, arith, stream_ptr(w)))
        return wp

    # ---------------------------------------------------------------- frame
    def forward(self, inp):
        x, _, live = self._operand(inp)      # (the indexes are ignored: the layer runs its own detection)
        arith = self._arith(x)
        Cin, K, Hi, Wi = self.in_channels, self.out_channels, x.size(2), x.size(3)
        work = self._workspace(Hi, Wi, x.device)
        Ho, Wo = work['size']
        self._state_for(x, Ho, Wo)
        bias = self.bias.detach() if self.bias is not None else None
        check(C.cbinfer_cbgroupconv2d_forward(
            ptr(x), ptr(self.prevInput), ptr(self.prevOutput), ptr(work['bits']), ptr(work['idx']), ptr(work['count']),
            ptr(self._weights(Hi, Wi, arith)), ptr(bias), Cin, Hi, Wi, K, self.groups, self._struct(),
            float(self.threshold), int(bool(self.feedbackLoop)), int(bool(self.copyInput)), int(bool(self.withReLU)),
            arith, stream_ptr(x)))
        self._keep_input(x, live)
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
    for seq in [m for m in rootModule.modules() if type(m) is nn.Sequential]:
        kids = list(seq.children())
        for prod, cons in zip(kids[:-1], kids[1:]):
            if type(prod) is CBGroupedConv2d:
                link_consumer(prod, cons)
    return rootModule
