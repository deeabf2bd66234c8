"""Change-based activations and per-channel affine: CBPointwise2d and insertCBPointwise (cb_pointwise.hip).

The reference has no element-wise operator of its own: an activation other than the ReLU a CBConv2d absorbs, or an
eval-mode nn.BatchNorm2d that foldBatchNorm cannot fold (BN -> ReLU -> conv, a BN behind a sum or a concat), stays a dense
torch operator -- it recomputes the whole map, drops the producer's change information and cannot be recorded by a
FrameProgram.  Every producer of this package leaves the pixels outside its change list bit for bit as they were, so
f(x) can differ from last frame's only at the producer's changed pixels: CBPointwise2d recomputes it there and is the
dense result exactly, without a threshold.  GELU, ELU / CELU / SELU, Softplus and Mish are taken with transcendental=True
(DESIGN 5.30).
"""
import torch
import torch.nn as nn

from . import _lib
from ._lib import C, CBinferError, check, dtype_code, ptr, require_device, stream_ptr
from .chain import (EVERY_PIXEL, CBStateModule, check_map, form_args, hand_on_changes, is_1x1, mask_workspace,
                    operand_changes, producers, split_operand)

# nn type (exactly, not a subclass) -> (CB_PW_* kind, p0, p1 of the instance)
_ACTIVATIONS = {
    nn.ReLU: lambda m: (_lib.PW_RELU, 0.0, 0.0),
    nn.ReLU6: lambda m: (_lib.PW_HARDTANH, 0.0, 6.0),
    nn.Hardtanh: lambda m: (_lib.PW_HARDTANH, float(m.min_val), float(m.max_val)),
    nn.LeakyReLU: lambda m: (_lib.PW_LEAKY, float(m.negative_slope), 0.0),
    nn.PReLU: lambda m: (_lib.PW_PRELU, 0.0, 0.0),
    nn.Hardswish: lambda m: (_lib.PW_HARDSWISH, 0.0, 0.0),
    nn.Hardsigmoid: lambda m: (_lib.PW_HARDSIGMOID, 0.0, 0.0),
    nn.Sigmoid: lambda m: (_lib.PW_SIGMOID, 0.0, 0.0),
    nn.SiLU: lambda m: (_lib.PW_SILU, 0.0, 0.0),
    nn.Tanh: lambda m: (_lib.PW_TANH, 0.0, 0.0),
}


def _gelu(m):
    if m.approximate not in ('none', 'tanh'):
        raise CBinferError("CBPointwise2d: act=%r: approximate=%r is not supported, only 'none' and 'tanh'"
                           % (m, m.approximate))
    return (_lib.PW_GELU if m.approximate == 'none' else _lib.PW_GELU_TANH), 0.0, 0.0


def _celu(m):
    if float(m.alpha) == 0.0:
        raise CBinferError("CBPointwise2d: act=%r: alpha=0 is not supported (CELU divides by it)" % (m,))
    # (1 / alpha rounded to float32 once, as the kernel takes it)
    return _lib.PW_ELU, float(m.alpha), float(torch.tensor(1.0 / float(m.alpha), dtype=torch.float32))


def _softplus(m):
    if float(m.beta) == 0.0:
        raise CBinferError("CBPointwise2d: act=%r: beta=0 is not supported (Softplus divides by it)" % (m,))
    return _lib.PW_SOFTPLUS, float(m.beta), float(m.threshold)


# the types `transcendental=True` adds: the device's erff / tanhf / expm1f / expf / log1pf, no bit-for-bit twin
_TRANSCENDENTAL = {
    nn.GELU: _gelu,
    nn.ELU: lambda m: (_lib.PW_ELU, float(m.alpha), 1.0),
    nn.CELU: _celu,
    nn.SELU: lambda m: (_lib.PW_SELU, 0.0, 0.0),
    nn.Softplus: _softplus,
    nn.Mish: lambda m: (_lib.PW_MISH, 0.0, 0.0),
}
_PER_CHANNEL = ('scale', 'shift', 'slope')


def _table(transcendental):
    return {**_ACTIVATIONS, **_TRANSCENDENTAL} if transcendental else _ACTIVATIONS


def _bn_affine(norm):
    """(scale, shift) f32 [C] of an eval-mode nn.BatchNorm2d: scale = gamma / sqrt(var + eps), shift = beta - mean scale,
    evaluated in float64, each rounded once; gamma = 1, beta = 0 without affine parameters."""
    if type(norm) is not nn.BatchNorm2d:
        raise CBinferError("CBPointwise2d: norm=%s is not supported, only an nn.BatchNorm2d" % type(norm).__name__)
    if norm.training:
        raise CBinferError("CBPointwise2d: norm is in training mode (call .eval() first): its statistics change with "
                           "every frame")
    if norm.running_mean is None or norm.running_var is None:
        raise CBinferError("CBPointwise2d: norm has no running statistics (track_running_stats=False): it normalises "
                           "with each frame's own")
    with torch.no_grad():
        d = torch.sqrt(norm.running_var.detach().double() + norm.eps)
        gamma = norm.weight.detach().double() if norm.weight is not None else torch.ones_like(d)
        beta = norm.bias.detach().double() if norm.bias is not None else torch.zeros_like(d)
        scale = gamma.to(d.device) / d
        shift = beta.to(d.device) - norm.running_mean.detach().double() * scale
        return scale.float(), shift.float()


class CBPointwise2d(CBStateModule):
    """out = act(norm(x)), recomputed at the operand's changed pixels (no counterpart in the reference).

    act: None or an instance of exactly one of nn.ReLU, nn.ReLU6, nn.Hardtanh, nn.LeakyReLU, nn.PReLU (1 or C
    parameters), nn.Hardswish, nn.Hardsigmoid, nn.Sigmoid, nn.SiLU, nn.Tanh -- not a subclass; `inplace=` is ignored, the
    module writes its own state.  norm: None or an eval-mode nn.BatchNorm2d with running statistics, applied first as
    x scale[c] + shift[c] (two roundings).  At least one of the two.  scale / shift / slope are computed HERE and kept as
    float32 buffers (pickled, moved by .to(), kept float32 by .half()): later edits of the source modules are not
    followed.  The first seven activations are torch's CPU operators bit for bit, fp32 and fp16; Sigmoid, SiLU and Tanh
    call the device's expf / tanhf (DESIGN 5.16 has the bound).  transcendental=True adds exactly nn.GELU (approximate
    'none' or 'tanh'), nn.ELU, nn.CELU (alpha != 0), nn.SELU, nn.Softplus (beta != 0) and nn.Mish, each bounded against
    its formula in float64; without it they are refused as before.

    forward(x): a [1, C, H, W] tensor or the ('changeIndexes', tensor, indexes) tuple of a producer with
    propChangeIndexes.  A bare tensor carries no change information: every pixel is recomputed.  A MaskChangeIndexes
    is taken as its mask, as CBUpsample2d and CBConcat2d take it (its list is never made); any other ChangeIndexes, or an
    exact int32 tensor, as a list.  The flags are CBAdd2d's: propChangeIndexes hands on the frame's mask as a MaskChangeIndexes;
    cloneOutput=False hands out the state itself, tagged, and the frame is then free of torch operators."""

    _WORK = '_pwWork'

    def __init__(self, act=None, norm=None, transcendental=False):
        super(CBPointwise2d, self).__init__()
        if act is None and norm is None:
            raise CBinferError("CBPointwise2d: act=None and norm=None: at least one of the two must be given")
        self.kind, self.p0, self.p1 = _lib.PW_IDENTITY, 0.0, 0.0
        self.actName = None
        scale = shift = slope = None
        if act is not None:
            table = _table(transcendental)
            if type(act) not in table:
                raise CBinferError("CBPointwise2d: act=%s is not supported, only an instance of exactly %s"
                                   % (type(act).__name__, ", ".join("nn." + t.__name__ for t in table)))
            self.kind, self.p0, self.p1 = table[type(act)](act)
            self.actName = type(act).__name__
            if not C.cbinfer_pointwise_supported(self.kind, self.p0, self.p1):
                if self.kind != _lib.PW_HARDTANH:
                    raise CBinferError("CBPointwise2d: act=%r: the parameters %r, %r are not usable"
                                       % (act, self.p0, self.p1))
                raise CBinferError("CBPointwise2d: act=%r: min_val=%r is above max_val=%r" % (act, self.p0, self.p1))
            if self.kind == _lib.PW_PRELU:
                slope = act.weight.detach().float().reshape(-1).clone()      # (an fp16 weight converts exactly)
        if norm is not None:
            scale, shift = _bn_affine(norm)
            if slope is not None and slope.numel() not in (1, scale.numel()):
                raise CBinferError("CBPointwise2d: act has %d parameters, norm %d features"
                                   % (slope.numel(), scale.numel()))
            if slope is not None:
                slope = slope.to(scale.device)
        for name, t in zip(_PER_CHANNEL, (scale, shift, slope)):
            self.register_buffer(name, t)
        # (the state behind the per-channel operands, as state_dict() has always listed them)
        self._buffers['outputState'] = self._buffers.pop('outputState')

    def _apply(self, fn, *args, **kwargs):
        # (.half() / .double() convert every floating-point buffer: the per-channel operands stay float32, the kernel's)
        keep = {n: self._buffers[n] for n in _PER_CHANNEL if self._buffers.get(n) is not None}
        super(CBPointwise2d, self)._apply(fn, *args, **kwargs)
        for n, t in keep.items():
            if self._buffers[n].dtype != torch.float32:
                self._buffers[n] = t.to(self._buffers[n].device)
        return self

    def _workspace(self, nc, H, W, dev):
        """Working mask (zero between frames), the frame's mask copy, index buffer and count, the slope of a
        one-parameter PReLU broadcast over the channels: once per map size."""
        def make():
            slope = self.slope
            if slope is not None and slope.numel() == 1 and nc != 1:
                slope = slope.expand(nc).contiguous()
            return dict(mask_workspace(H, W, dev), slope=slope)
        return self._cached_work((nc, H, W, dev), make)

    def forward(self, inp):
        x, indexes = split_operand('CBPointwise2d', inp, 'the input')
        check_map('CBPointwise2d', x)
        nc, H, W = x.size(1), x.size(2), x.size(3)
        for name in _PER_CHANNEL:
            t = getattr(self, name)
            if t is not None and t.numel() != nc and not (name == 'slope' and t.numel() == 1):
                raise CBinferError("CBPointwise2d: the input has %d channels, %s was made for %d"
                                   % (nc, name, t.numel()))
        require_device(x)
        for name in _PER_CHANNEL:
            t = getattr(self, name)
            if t is not None and t.device != x.device:
                raise CBinferError("CBPointwise2d: the input is on %s, %s on %s (move the module with .to())"
                                   % (x.device, name, t.device))
        work = self._workspace(nc, H, W, x.device)
        form = operand_changes('CBPointwise2d', 'the input', indexes, H, W, x.device, work['idx'])
        if self._fresh_state(x.shape, x):      # (written completely: the operand's change information is not used)
            form = EVERY_PIXEL
        check(C.cbinfer_cbpointwise_forward(ptr(x), ptr(self.outputState), *form_args(form), ptr(work['bits']),
                                            ptr(work['copy']), nc, H, W, self.kind, self.p0, self.p1,
                                            ptr(self.scale), ptr(self.shift), ptr(work['slope']), dtype_code(x),
                                            stream_ptr(x)))
        return self._result(work, H, W)

    def __repr__(self):
        return 'CBPointwise2d (act=%s, p0=%s, p1=%s, norm=%s, propChgIdxs=%s)' % (
            self.actName, self.p0, self.p1, self.scale is not None, self.propChangeIndexes)


def insertCBPointwise(rootModule, transcendental=False):
    """Inside every nn.Sequential of rootModule, a run  [nn.BatchNorm2d] [activation]  (at least one of the two; the
    activations of CBPointwise2d, with transcendental=True those it adds) that directly follows a producer --
    chain.producers('insertCBPointwise'), another CBPointwise2d among them -- becomes ONE CBPointwise2d under the run's first name, fed by that producer's changes:
    propChangeIndexes is switched on at the producer (chain.hand_on_changes).  The new module hands its own changes on
    (propChangeIndexes) only where it stands directly in front of a 1x1 / stride-1 / padding-0 CBConv2d -- a k x k
    CBConv2d that is handed indexes skips its own detection, which would be wrong here;
    linkDepthwise, insertCBUpsampling, insertCBTransposedConv and insertCBPooling(generalGeometry=True), called
    afterwards, switch the flag on for their own consumers.  A run behind anything else, or an activation outside the
    table, stays dense.  A batch norm in training mode or without running statistics raises CBinferError, as
    foldBatchNorm does.  Returns rootModule."""
    for seq in [m for m in rootModule.modules() if type(m) is nn.Sequential]:
        pos = 1
        while pos < len(seq._modules):
            names = list(seq._modules.keys())
            prod, first = seq._modules[names[pos - 1]], seq._modules[names[pos]]
            pos += 1
            if type(prod) not in producers('insertCBPointwise'):
                continue
            norm = first if type(first) is nn.BatchNorm2d else None
            after = seq._modules[names[pos]] if norm is not None and pos < len(names) else first
            act = after if type(after) in _table(transcendental) else None
            if norm is None and act is None:
                continue
            cb = CBPointwise2d(act=act, norm=norm, transcendental=transcendental)
            hand_on_changes(prod)
            seq._modules[names[pos - 1]] = cb
            if norm is not None and act is not None:
                del seq._modules[names[pos]]
            # (pos now names the module behind the run)
            names = list(seq._modules.keys())
            if pos < len(names) and is_1x1(seq._modules[names[pos]]):
                cb.propChangeIndexes = True
    return rootModule
