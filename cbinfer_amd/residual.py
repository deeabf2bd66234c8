"""Change-based residual blocks: CBAdd2d, CBResidual and foldBatchNorm (cb_add.hip).

The reference has no element-wise sum: `out = relu(body(x) + x)` of a ResNet-type block ends a change-based chain -- the
torch add recomputes the whole map, drops both operands' change lists and cannot be recorded by a FrameProgram.  Every
producer of this package leaves the pixels outside its change list bit for bit as they were, so the sum can differ from
last frame's only at the UNION of the two lists: CBAdd2d recomputes it there and is the dense result exactly, without a
threshold.  foldBatchNorm removes the nn.BatchNorm2d layers such blocks carry behind their bias-free convolutions, which
convert() would leave as dense torch operators.
"""
import torch
import torch.nn as nn

from ._lib import C, CBinferError, check, dtype_code, ptr, require_device, stream_ptr
from .chain import (EVERY_PIXEL, OPERAND_WORDS, CBStateModule, form_args, mask_workspace, operand_changes,
                    split_operand)
from .conv2d import CBConv2d


# operand_changes' refusals in this module's words (which: 'operand a' / 'operand b')
_ADD_WORDS = (
    "%(name)s: the change indexes of %(which)s address a %(h)dx%(w)d map, the operands are %(H)dx%(W)d maps",
    OPERAND_WORDS[1],
    "%(name)s: the change indexes of %(which)s must be a contiguous one-dimensional int32 tensor on the operands' device")


class CBAdd2d(CBStateModule):
    """out = a + b, with relu=True relu(a + b), recomputed at the union of the operands' changed pixels.

    forward(a, b): each argument a [1, C, H, W] tensor or the ('changeIndexes', tensor, indexes) tuple of a producer with
    propChangeIndexes.  A bare tensor carries no change information: every pixel is recomputed.  A MaskChangeIndexes
    whose list is not made is taken as its mask (the list is never made); any other ChangeIndexes, or an exact int32
    tensor, as a list.  The flags are CBPoolMax2d's: propChangeIndexes hands on the union as a MaskChangeIndexes;
    cloneOutput=False hands out the state itself, tagged, and the frame is then free of torch operators."""
    _WORK = '_addWork'

    def __init__(self, relu=False):
        super(CBAdd2d, self).__init__()
        self.relu = bool(relu)

    def _workspace(self, H, W, dev):
        """Working mask (zero between frames), the frame's mask copy, index buffer and count: once per map size."""
        return self._cached_work((H, W, dev), lambda: mask_workspace(H, W, dev))

    def forward(self, a, b):
        a, ia = split_operand('CBAdd2d', a, 'operand a')
        b, ib = split_operand('CBAdd2d', b, 'operand b')
        if a.dim() != 4 or a.size(0) != 1:
            raise CBinferError("CBAdd2d: operands must be [1, C, H, W] tensors, a is %s" % (tuple(a.shape),))
        if a.shape != b.shape or a.dtype != b.dtype or a.device != b.device:
            raise CBinferError("CBAdd2d: the operands differ: a is %s %s on %s, b is %s %s on %s"
                               % (tuple(a.shape), a.dtype, a.device, tuple(b.shape), b.dtype, b.device))
        require_device(a, b)
        nc, H, W = a.size(1), a.size(2), a.size(3)
        work = self._workspace(H, W, a.device)
        # (a list the producer's kernel already made is taken before its mask)
        fa, fb = (operand_changes('CBAdd2d', 'operand ' + which, ix, H, W, a.device, work['idx'], words=_ADD_WORDS,
                                  maskWhenMade=False) for which, ix in (('a', ia), ('b', ib)))
        if self._fresh_state(a.shape, a):      # (written completely: neither operand's change information is used)
            fa = fb = EVERY_PIXEL
        check(C.cbinfer_cbadd_forward(ptr(a), ptr(b), ptr(self.outputState), *form_args(fa), *form_args(fb),
                                      ptr(work['bits']), ptr(work['copy']), nc, H, W, int(self.relu), dtype_code(a),
                                      stream_ptr(a)))
        return self._result(work, H, W)

    def __repr__(self):
        return 'CBAdd2d (relu=%s, propChgIdxs=%s)' % (self.relu, self.propChangeIndexes)


def _sequential(m):
    if m is None or type(m) is nn.Sequential:
        return m
    return nn.Sequential(*m) if isinstance(m, (list, tuple)) else nn.Sequential(m)


class CBResidual(nn.Module):
    """out = [relu](body(x) + shortcut(x)), or body(x) + x without a shortcut, as one link of a change-based chain.

    `body` and `shortcut` are CONVERTED nn.Sequential containers (pycbinfer.convert; batch norms folded before with
    foldBatchNorm).  Both are fed the bare tensor: their first layers run their own change detection (a 3x3 layer must
    not recompute exactly the propagated pixels).  The sum takes the body's result, and the shortcut's or -- identity --
    the incoming operand with the incoming change list, if there was one.  The constructor switches propChangeIndexes on
    at the last module of body / shortcut where that is a CBConv2d, and copyInput on at their first layers that are not in
    feedback mode (what comes in may be a producer's live state, as behind a pool of insertCBPooling).  The sum is
    `self.add`: set its propChangeIndexes / cloneOutput as on a CBPoolMax2d."""

    def __init__(self, body, shortcut=None, relu=True):
        super(CBResidual, self).__init__()
        self.body = _sequential(body)
        self.shortcut = _sequential(shortcut)
        self.add = CBAdd2d(relu=relu)
        for seq in (self.body, self.shortcut):
            kids = list(seq.children()) if seq is not None else []
            if kids and type(kids[-1]) is CBConv2d:
                kids[-1].propChangeIndexes = True
            if kids and type(kids[0]) is CBConv2d and not kids[0].feedbackLoop:
                kids[0].copyInput = True

    def forward(self, inp):
        src = inp[1] if type(inp) == tuple else inp
        main = self.body(src)
        return self.add(main, self.shortcut(src) if self.shortcut is not None else inp)


def _round_once(x, dtype):
    """The float64 tensor x in `dtype`, rounded ONCE.  torch converts float64 to float16 through float32, two roundings
    that can land on the wrong side of a float16 tie; so the float32 in between is made by rounding to odd (truncate,
    then set the last bit if anything was cut off), after which the second rounding is the correct one."""
    if dtype != torch.float16:
        return x.to(dtype)
    f = x.to(torch.float32)
    bits = f.view(torch.int32)
    bits = torch.where(f.double().abs() > x.abs(), bits - 1, bits)      # (towards zero: the magnitude's bit pattern - 1)
    bits = torch.where(bits.view(torch.float32).double() != x, bits | 1, bits)
    return bits.view(torch.float32).to(torch.float16)


def foldBatchNorm(rootModule):
    """Inside every nn.Sequential of rootModule, an nn.BatchNorm2d directly behind an nn.Conv2d disappears into it: the
    pair becomes a NEW nn.Conv2d with bias under the convolution's name (the source modules' parameters are not
    touched),
        w' = w gamma / sqrt(var + eps)  per output channel,    b' = (b - mean) gamma / sqrt(var + eps) + beta,
    evaluated left to right in float64 and rounded once to the convolution's dtype; gamma = 1, beta = 0 without affine
    parameters, b = 0 without a bias.  The batch norm must be in eval mode and have running statistics, CBinferError
    otherwise.  Call before convert(), which would leave the batch norm a dense torch operator.  Returns rootModule."""
    for seq in [m for m in rootModule.modules() if type(m) is nn.Sequential]:
        names = list(seq._modules.keys())
        for cname, bname in zip(names[:-1], names[1:]):
            conv, bn = seq._modules.get(cname), seq._modules.get(bname)      # (None: folded away just before)
            if type(conv) is not nn.Conv2d or type(bn) is not nn.BatchNorm2d:
                continue
            if bn.training:
                raise CBinferError("foldBatchNorm: batch norm %r is in training mode (call .eval() first): its "
                                   "statistics change with every frame" % bname)
            if bn.running_mean is None or bn.running_var is None:
                raise CBinferError("foldBatchNorm: batch norm %r has no running statistics "
                                   "(track_running_stats=False): it normalises with each frame's own" % bname)
            if bn.num_features != conv.out_channels:
                raise CBinferError("foldBatchNorm: batch norm %r has %d features, convolution %r %d output channels"
                                   % (bname, bn.num_features, cname, conv.out_channels))
            w = conv.weight.detach()
            with torch.no_grad():
                d = torch.sqrt(bn.running_var.detach().double() + bn.eps)
                gamma = bn.weight.detach().double() if bn.weight is not None else torch.ones_like(d)
                beta = bn.bias.detach().double() if bn.bias is not None else torch.zeros_like(d)
                b = conv.bias.detach().double() if conv.bias is not None else torch.zeros_like(d)
                gamma, beta, b, d = (t.to(w.device) for t in (gamma, beta, b, d))
                wf = w.double() * gamma.view(-1, 1, 1, 1) / d.view(-1, 1, 1, 1)
                bf = (b - bn.running_mean.detach().double().to(w.device)) * gamma / d + beta
                folded = nn.Conv2d(conv.in_channels, conv.out_channels, conv.kernel_size, conv.stride, conv.padding,
                                   conv.dilation, conv.groups, True, conv.padding_mode, device=w.device, dtype=w.dtype)
                folded.weight.copy_(_round_once(wf, w.dtype))
                folded.bias.copy_(_round_once(bf, w.dtype))
            folded.train(conv.training)
            seq._modules[cname] = folded
            del seq._modules[bname]
    return rootModule
