"""Change-based depthwise convolution: CBDepthwiseConv2d and linkDepthwise (cb_dwconv.hip).

The reference has no such operator.  A depthwise nn.Conv2d (groups == in_channels, with a channel multiplier) -- the 3x3
layer of MobileNet / EfficientNet-type blocks, the separable convolutions of Xception / DeepLabv3+, the 7x7 stage of
ConvNeXt-type blocks -- ends a change-based chain: CBConv2d refuses groups, torch recomputes the whole map, drops the
producer's change mask and cannot be recorded by a FrameProgram.  The module either runs the layer's own change
detection on its input (component a1's rule with `threshold`) or, behind a producer that hands on its changes
(propagatedChanges), takes the footprint of the producer's list or mask; it recomputes exactly the listed output pixels
and leaves every other output pixel bit for bit as it was.
"""
import ctypes

import torch.nn as nn

from . import _lib
from ._lib import C, CBinferError, check, dtype_code, ptr, stream_ptr
from .chain import PROPAGATED, hand_back, hand_on_changes, is_1x1, mask_workspace, operand_changes, producers
from .conv2d import _padding_pair
from .layer import CBDetectingLayer, check_limits, frame_masks

MAX_K, MAX_S, MAX_D, MAX_P = 7, 4, 8, 64


def _check_depthwise(m):
    """(kernel_size, stride, padding, dilation) as pairs of ints if the library takes the module `m`; CBinferError with
    a sentence naming the setting otherwise."""
    Err = CBinferError
    if not isinstance(m, nn.Conv2d) or m.transposed or tuple(m.output_padding) != (0, 0):
        raise Err("CBDepthwiseConv2d: only plain nn.Conv2d modules are converted, got %s" % type(m).__name__)
    if m.groups != m.in_channels:
        raise Err("CBDepthwiseConv2d: groups=%d with in_channels=%d is not a depthwise convolution (groups == "
                  "in_channels); general grouped convolutions are not supported" % (m.groups, m.in_channels))
    if m.out_channels % m.in_channels:
        raise Err("CBDepthwiseConv2d: out_channels=%d is not a multiple of in_channels=%d"
                  % (m.out_channels, m.in_channels))
    if m.padding_mode != 'zeros':
        raise Err("CBDepthwiseConv2d: padding_mode=%r is not supported, only 'zeros'" % (m.padding_mode,))
    p = _padding_pair(m, 'CBDepthwiseConv2d')
    k, s, d = (tuple(int(v) for v in t) for t in (m.kernel_size, m.stride, m.dilation))
    check_limits('CBDepthwiseConv2d', [('kernel_size', k, MAX_K), ('stride', s, MAX_S), ('dilation', d, MAX_D),
                                       ('padding', p, MAX_P)])
    g = _lib.Geom(k[0], k[1], s[0], s[1], p[0], p[1], d[0], d[1])
    if not C.cbinfer_dwconv_supported(m.in_channels, m.out_channels // m.in_channels, ctypes.byref(g)):
        raise Err("CBDepthwiseConv2d: kernel_size=%s stride=%s padding=%s dilation=%s is beyond what the library takes"
                  % (k, s, p, d))
    return k, s, p, d


def _propagated_ok(k, p, d):
    """The footprint of a producer's changes is the filter's window: dilation 1 and padding <= kernel_size / 2."""
    return all(d[i] == 1 and 2 * p[i] <= k[i] for i in (0, 1))


class CBDepthwiseConv2d(CBDetectingLayer):
    """Change-based depthwise nn.Conv2d (no counterpart in the reference): groups == in_channels, out_channels a
    multiple of it; per axis kernel_size <= 7, stride <= 4, dilation <= 8, padding <= 64 (ints, 'valid' or a symmetric
    'same'); with or without bias, batch 1, fp32 or fp16.  The parameters are shared with the source module.

    forward(x): a [1, C, Hi, Wi] tensor or the ('changeIndexes', tensor, indexes) tuple of a producer.  Flags:
    threshold, feedbackLoop, copyInput as on CBConv2d; withReLU, and reluCap (None, or 6.0 for ReLU6); propChangeIndexes
    hands on the frame's change mask on the OUTPUT map as a MaskChangeIndexes; cloneOutput=False hands out prevOutput
    itself, tagged, and the frame is then free of torch operators.  propagatedChanges=False: the indexes of a tuple are
    ignored, the layer detects for itself.  propagatedChanges=True (dilation 1, padding <= kernel_size / 2): the output
    pixels whose filter window holds a pixel of the producer's list or mask are recomputed from the input tensor itself;
    no detection runs, prevInput is not kept, `threshold` is not used, and the frame on which prevOutput was
    (re)allocated -- or a bare tensor, which carries no change information -- lists every pixel.  Output pixels no tap
    reaches (padding > dilation (kernel_size - 1)) hold act(bias) from the moment the state is allocated and are never
    written."""

    def __init__(self, m, threshold):
        super(CBDepthwiseConv2d, self).__init__(m, threshold, _check_depthwise(m))
        self.reluCap = None
        self.propagatedChanges = False

    def _act(self):
        if not self.withReLU:
            return _lib.ACT_NONE
        if self.reluCap is None:
            return _lib.ACT_RELU
        if float(self.reluCap) != 6.0:
            raise CBinferError("CBDepthwiseConv2d: reluCap=%r is not supported, only None or 6.0" % (self.reluCap,))
        return _lib.ACT_RELU6

    def _buffers_for(self, Ho, Wo, dev):
        """Frame masks (zero once) and their mask-copy view for the layer's own detection, working mask and mask copy
        for propagated changes, index buffer and count for a consumer that wants the list."""
        frame, frameCopy = frame_masks(Ho, Wo, dev)
        return dict(mask_workspace(Ho, Wo, dev), frame=frame, frameCopy=frameCopy)

    # ---------------------------------------------------------------- frame
    def forward(self, inp):
        x, indexes, live = self._operand(inp)
        Cin, mult, Hi, Wi = self.in_channels, self.out_channels // self.in_channels, x.size(2), x.size(3)
        act, dt = self._act(), dtype_code(x)
        work = self._workspace(Hi, Wi, x.device)
        Ho, Wo = work['size']
        weight = self.weight.detach().contiguous()
        bias = self.bias.detach() if self.bias is not None else None
        if self.propagatedChanges:
            if not _propagated_ok(self.kernel_size, self.padding, self.dilation):
                raise CBinferError("CBDepthwiseConv2d: propagatedChanges needs dilation 1 and padding <= kernel_size / 2 "
                                   "per axis (kernel_size=%s padding=%s dilation=%s): the layer must detect for itself"
                                   % (self.kernel_size, self.padding, self.dilation))
            fresh = self._state_for(x, Ho, Wo, keepInput=False)
            # (checked on every frame, read on all but the first)
            mask, idx, cap, count = operand_changes('CBDepthwiseConv2d', 'layer', indexes, Hi, Wi, x.device, work['idx'],
                                                    **PROPAGATED)
            every = fresh or indexes is None
            if every:
                mask, idx, cap, count = None, None, 0, None
            check(C.cbinfer_cbdwconv2d_forward_propagated(
                ptr(x), ptr(self.prevOutput), ptr(idx), cap, ptr(count), ptr(mask), int(every), ptr(work['bits']),
                ptr(work['copy']), ptr(weight), ptr(bias), Cin, mult, Hi, Wi, self._struct(), act, dt, stream_ptr(x)))
            copy = work['copy']
        else:
            self._state_for(x, Ho, Wo)
            check(C.cbinfer_cbdwconv2d_forward(
                ptr(x), ptr(self.prevInput), ptr(self.prevOutput), ptr(work['frame']), ptr(weight), ptr(bias), Cin, mult,
                Hi, Wi, self._struct(), float(self.threshold), int(bool(self.feedbackLoop)), int(bool(self.copyInput)),
                act, dt, stream_ptr(x)))
            self._keep_input(x, live)
            copy = work['frameCopy']
        return hand_back(self, self.prevOutput, copy, (Ho, Wo), work)

    def __repr__(self):
        return ('CBDepthwiseConv2d (%d, %d, k=%s, s=%s, p=%s, d=%s, th=%s, withReLU=%s, reluCap=%s, propChgIdxs=%s, '
                'propagated=%s)' % (self.in_channels, self.out_channels, self.kernel_size, self.stride, self.padding,
                                    self.dilation, self.threshold, self.withReLU, self.reluCap, self.propChangeIndexes,
                                    self.propagatedChanges))


def linkDepthwise(rootModule):
    """Inside every nn.Sequential of rootModule: a CBDepthwiseConv2d with dilation 1 and padding <= kernel_size / 2 that
    directly follows a producer -- chain.producers('linkDepthwise'), another CBDepthwiseConv2d among them -- takes that
    producer's changes (propagatedChanges on the layer, propChangeIndexes on the producer: chain.hand_on_changes) and
    runs no detection; a CBDepthwiseConv2d directly in front of a 1x1 / stride-1 / padding-0 CBConv2d hands its changes
    on (propChangeIndexes).  Returns rootModule."""
    for seq in [m for m in rootModule.modules() if type(m) is nn.Sequential]:
        kids = list(seq.children())
        for prod, cons in zip(kids[:-1], kids[1:]):
            if (type(cons) is CBDepthwiseConv2d and type(prod) in producers('linkDepthwise') and
                    _propagated_ok(cons.kernel_size, cons.padding, cons.dilation)):
                cons.propagatedChanges = True
                hand_on_changes(prod)
            if type(prod) is CBDepthwiseConv2d and is_1x1(cons):
                prod.propChangeIndexes = True
    return rootModule
