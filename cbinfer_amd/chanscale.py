"""Change-based channel attention scale: CBChannelScale2d, CBSqueezeExcite and insertCBSqueezeExcite (cb_chanscale.hip,
DESIGN 5.28).

The reference has no squeeze-and-excitation block.  CBPoolAvg2d(nn.AdaptiveAvgPool2d(1)) does the squeeze change-based,
but the excite `x * g(v)` ended the chain: the [1, C, 1, 1] vector v moves a little in every frame of a video, so
CBBinary2d recomputes the whole map behind it and hands on a full mask.  The modules here apply the library's own rule to
the channel vector: a gate that moved by no more than `threshold` is HELD at the value last used, and its channel plane
is recomputed only at the operand's changed pixels; a gate that moved by more TRIPS: it takes the new value and its
whole plane is recomputed.  At threshold = 0 this is the dense result.
"""
import copy

import torch
import torch.nn as nn

from . import _lib
from ._lib import C, CBinferError, check, dtype_code, ptr, require_device, stream_ptr
from .chain import (EVERY_PIXEL, CBStateModule, check_map, form_args, insert_behind_producers, mask_workspace,
                    operand_changes, producers, split_operand)
from .pool import CBPoolAvg2d

MAX_CHANNELS, MAX_HIDDEN = 4096, 1024
_GATES = {None: _lib.CS_GATE_NONE, 'sigmoid': _lib.CS_GATE_SIGMOID, 'hardsigmoid': _lib.CS_GATE_HARDSIGMOID}
_ACTS = {nn.ReLU: _lib.CS_ACT_RELU, nn.SiLU: _lib.CS_ACT_SILU}
# nn type of a gate module (exactly) -> the gate's name
_GATE_MODULES = {nn.Sigmoid: 'sigmoid', nn.Hardsigmoid: 'hardsigmoid', nn.Identity: None}
_F32_BUFFERS = ('w1', 'b1', 'w2', 'b2', 'held')


def _check_threshold(threshold):
    t = float(threshold)
    if not t >= 0.0:      # (also a NaN)
        raise CBinferError("CBChannelScale2d: threshold=%r must be a number >= 0" % (threshold,))
    return t


def _fc_operands(which, fc):
    """(weight f32 [out, in], bias f32 [out] or None) of an nn.Conv2d 1x1 or an nn.Linear (exactly), copied."""
    if type(fc) is nn.Conv2d:
        if (tuple(fc.kernel_size) != (1, 1) or tuple(fc.stride) != (1, 1) or tuple(fc.dilation) != (1, 1) or
                fc.groups != 1 or fc.padding not in ((0, 0), 0, 'valid')):
            raise CBinferError("CBChannelScale2d: %s=%r is not a plain 1x1 convolution (stride 1, no padding, no "
                               "dilation, groups 1)" % (which, fc))
    elif type(fc) is not nn.Linear:
        raise CBinferError("CBChannelScale2d: %s=%s is not supported, only an nn.Conv2d 1x1 or an nn.Linear (exactly "
                           "those types)" % (which, type(fc).__name__))
    w = fc.weight.detach()
    w = w.reshape(w.size(0), w.size(1)).float().clone().contiguous()
    b = fc.bias.detach().float().clone().contiguous() if fc.bias is not None else None
    return w, b


class CBChannelScale2d(CBStateModule):
    """out[c, p] = a[c, p] * held[c], with held[c] the gate g(s[c]) the channel last TRIPPED at (no counterpart in the
    reference; the arithmetic is specified in include/cbinfer_hip.h).

    threshold: a channel trips in a frame when its gate differs from held[c] by strictly more than this (a NaN trips);
    only then held[c] takes the new gate and the whole plane is recomputed.  Every other channel is recomputed at the
    operand's changed pixels alone, with the held gate, so slow drift adds up until it trips.  threshold = 0 gives the
    dense result.  gate: 'sigmoid', 'hardsigmoid' or None (the identity).

    Without fc1 / fc2, forward(a, v) takes any per-frame [1, C, 1, 1] vector v of a's dtype -- also one made by dense
    torch operators: ECA's 1-d convolution, CBAM's shared MLP over two pools.  With fc1 / fc2 -- each an nn.Conv2d 1x1
    or an nn.Linear, exactly, bias optional -- and act, an nn.ReLU or nn.SiLU, exactly, forward(a, z) takes the POOLED
    vector z and the gate launch evaluates s = fc2(act(fc1(z))) itself, in float32 and in the order of sum16: the
    frame of an SE block is then free of torch operators.  The weights are COPIED here into float32 buffers (w1, b1, w2,
    b2), which follow .to() and stay float32 under .half(); later edits of the source modules are not followed.

    a is a [1, C, H, W] tensor (no change information: every pixel is recomputed) or the ('changeIndexes', tensor,
    indexes) tuple of a producer with propChangeIndexes, taken as CBPointwise2d takes it; the vector is a bare tensor.
    C <= 4096, hidden width <= 1024.

    State: outputState and held (float32 [C]), both from getStateTensors(), both dropped by clearMemory().  The flags
    are CBAdd2d's: cloneOutput=False hands out the state itself, tagged; propChangeIndexes hands on the frame's mask as
    a MaskChangeIndexes: the operand's changed pixels -- or EVERY pixel in a frame in which a channel tripped.  A
    per-pixel mask cannot say "channel 7 only": behind a tripped channel the consumer recomputes every pixel.
    lastTrippedChannels(): how many channels tripped in the last frame (synchronises: for tests and for tuning)."""

    _WORK = '_csWork'

    def __init__(self, threshold, gate='sigmoid', fc1=None, fc2=None, act=None):
        super(CBChannelScale2d, self).__init__()
        self.threshold = _check_threshold(threshold)
        if gate not in _GATES:
            raise CBinferError("CBChannelScale2d: gate=%r is not supported, only 'sigmoid', 'hardsigmoid' or None"
                               % (gate,))
        self.gate = gate
        self.actName = None
        w1 = b1 = w2 = b2 = None
        if (fc1 is None) != (fc2 is None):
            raise CBinferError("CBChannelScale2d: fc1 and fc2 go together (both or neither)")
        if fc1 is None:
            if act is not None:
                raise CBinferError("CBChannelScale2d: act=%s without fc1 / fc2: the plain form takes the gate's "
                                   "argument as it is" % type(act).__name__)
            self._act = _lib.CS_ACT_NONE
        else:
            if type(act) not in _ACTS:
                raise CBinferError("CBChannelScale2d: act=%s is not supported, only an nn.ReLU or an nn.SiLU (exactly "
                                   "those types)" % type(act).__name__)
            self._act, self.actName = _ACTS[type(act)], type(act).__name__
            (w1, b1), (w2, b2) = _fc_operands('fc1', fc1), _fc_operands('fc2', fc2)
            if w2.size(1) != w1.size(0) or w2.size(0) != w1.size(1):
                raise CBinferError("CBChannelScale2d: fc1 maps %d -> %d channels and fc2 %d -> %d: they do not chain "
                                   "back to the map's channels" % (w1.size(1), w1.size(0), w2.size(1), w2.size(0)))
            if w1.size(1) > MAX_CHANNELS or w1.size(0) > MAX_HIDDEN:
                raise CBinferError("CBChannelScale2d: %d channels with a hidden width of %d: the library takes C <= %d "
                                   "and R <= %d" % (w1.size(1), w1.size(0), MAX_CHANNELS, MAX_HIDDEN))
            w2, b2 = w2.to(w1.device), (b2.to(w1.device) if b2 is not None else None)
        for name, t in zip(_F32_BUFFERS, (w1, b1, w2, b2)):
            self.register_buffer(name, t)
        # (the states behind the operands, as state_dict() lists them)
        self._buffers['outputState'] = self._buffers.pop('outputState')
        self._buffers['held'] = self._buffers.pop('held')

    @property
    def hidden(self):
        """R, the hidden width of the fused excitation; 0 in the plain form."""
        return self.w1.size(0) if self.w1 is not None else 0

    def clearMemory(self):
        super(CBChannelScale2d, self).clearMemory()
        if 'held' not in self._buffers:
            self.register_buffer('held', torch.zeros(0))
        self.held = torch.zeros(0, dtype=torch.float32, device=self.held.device)

    def getStateTensors(self):
        return [self.outputState, self.held]

    def _apply(self, fn, *args, **kwargs):
        # (.half() / .double() convert every floating-point buffer: the weights and the held gates stay float32, the
        #  kernel's)
        keep = {n: self._buffers[n] for n in _F32_BUFFERS if self._buffers.get(n) is not None}
        super(CBChannelScale2d, self)._apply(fn, *args, **kwargs)
        for n, t in keep.items():
            if self._buffers[n].dtype != torch.float32:
                self._buffers[n] = t.to(self._buffers[n].device)
        return self

    def _workspace(self, nc, H, W, dev):
        """The mask workspace, and the gate launch's outputs: this frame's gates, the tripped words, their count."""
        return self._cached_work((nc, H, W, dev), lambda: dict(
            mask_workspace(H, W, dev), gate=torch.zeros(nc, dtype=torch.float32, device=dev),
            tripped=torch.zeros((nc + 63) // 64, dtype=torch.int64, device=dev),
            tripCount=torch.zeros(1, dtype=torch.int32, device=dev)))

    def lastTrippedChannels(self):
        """The number of channels that tripped in the last frame (0 before the first).  Synchronises."""
        work = self.__dict__.get(self._WORK)
        return int(work['tripCount'].item()) if work is not None else 0

    def forward(self, a, v):
        a, ia = split_operand('CBChannelScale2d', a, 'operand a')
        check_map('CBChannelScale2d', a, 'operand a')
        nc, H, W = a.size(1), a.size(2), a.size(3)
        what = 'the pooled vector z' if self.w1 is not None else 'the vector v'
        if type(v) == tuple:
            raise CBinferError("CBChannelScale2d: %s is a [1, C, 1, 1] channel vector and came with change indexes: a "
                               "channel vector has no pixels, hand it over as a bare tensor" % what)
        if not torch.is_tensor(v):
            raise CBinferError("CBChannelScale2d: %s must be a tensor, got %s" % (what, type(v).__name__))
        if nc > MAX_CHANNELS:
            raise CBinferError("CBChannelScale2d: operand a has %d channels, the library takes C <= %d"
                               % (nc, MAX_CHANNELS))
        if tuple(v.shape) != (1, nc, 1, 1):
            raise CBinferError("CBChannelScale2d: the operands do not fit: a is %s, %s is %s and must be [1, %d, 1, 1]"
                               % (tuple(a.shape), what, tuple(v.shape), nc))
        if v.dtype != a.dtype or v.device != a.device:
            raise CBinferError("CBChannelScale2d: the operands differ: a is %s on %s, %s is %s on %s"
                               % (a.dtype, a.device, what, v.dtype, v.device))
        if self.w1 is not None and self.w1.size(1) != nc:
            raise CBinferError("CBChannelScale2d: operand a has %d channels, fc1 / fc2 were made for %d"
                               % (nc, self.w1.size(1)))
        threshold = _check_threshold(self.threshold)
        v = v.detach().contiguous()
        require_device(a, v)
        for name in _F32_BUFFERS[:4]:
            t = getattr(self, name)
            if t is not None and t.device != a.device:
                raise CBinferError("CBChannelScale2d: operand a is on %s, %s on %s (move the module with .to())"
                                   % (a.device, name, t.device))
        work = self._workspace(nc, H, W, a.device)
        form = operand_changes('CBChannelScale2d', 'operand a', ia, H, W, a.device, work['idx'])
        fresh = self._fresh_state(a.shape, a)
        if fresh or tuple(self.held.shape) != (nc,) or self.held.device != a.device or self.held.dtype != torch.float32:
            # (written completely, with every gate taken as it is: no change information is used)
            self.held = torch.zeros(nc, dtype=torch.float32, device=a.device)
            fresh, form = True, EVERY_PIXEL
        check(C.cbinfer_cbchanscale_forward(ptr(a), ptr(v), ptr(self.w1), ptr(self.b1), ptr(self.w2), ptr(self.b2),
                                            ptr(self.outputState), ptr(work['gate']), ptr(self.held),
                                            ptr(work['tripped']), ptr(work['tripCount']), *form_args(form),
                                            ptr(work['bits']), ptr(work['copy']), nc, self.hidden, H, W,
                                            _GATES[self.gate], self._act, threshold, int(fresh), dtype_code(a),
                                            stream_ptr(a)))
        return self._result(work, H, W)

    def __repr__(self):
        return 'CBChannelScale2d (threshold=%s, gate=%s, hidden=%d, act=%s, propChgIdxs=%s)' % (
            self.threshold, self.gate, self.hidden, self.actName, self.propChangeIndexes)


class CBSqueezeExcite(nn.Module):
    """A squeeze-and-excitation block, x * g(fc2(act(fc1(mean(x))))), as one link of a change-based chain: the wiring
    twin of CBGated.  `pool` is a CBPoolAvg2d(nn.AdaptiveAvgPool2d(1)), `scale` a CBChannelScale2d with the fused
    excitation; forward(inp) hands the same operand, with its change information, to both: scale(inp, pool(inp)).  inp
    is the ('changeIndexes', tensor, indexes) tuple of the producer in front (a pool always stands behind one).  The
    pool hands its state to the scale as it is (cloneOutput=False there): a frame consists of library calls only.
    propChangeIndexes / cloneOutput are the scale's."""

    def __init__(self, threshold, fc1, fc2, act, gate='sigmoid'):
        super(CBSqueezeExcite, self).__init__()
        self.pool = CBPoolAvg2d(nn.AdaptiveAvgPool2d(1))
        self.pool.cloneOutput = False
        self.scale = CBChannelScale2d(threshold, gate=gate, fc1=fc1, fc2=fc2, act=act)

    propChangeIndexes = property(lambda self: self.scale.propChangeIndexes,
                                 lambda self, v: setattr(self.scale, 'propChangeIndexes', v))
    cloneOutput = property(lambda self: self.scale.cloneOutput, lambda self, v: setattr(self.scale, 'cloneOutput', v))
    threshold = property(lambda self: self.scale.threshold, lambda self, v: setattr(self.scale, 'threshold', v))

    def forward(self, inp):
        return self.scale(inp, self.pool(inp))

    def __repr__(self):
        return 'CBSqueezeExcite (%r)' % (self.scale,)


def _follows_the_formula(m, names):
    """Whether the user's module `m` computes x * g(fc2(act(fc1(mean(x))))) with the sub-modules `names` gives: both on
    one small random CPU tensor in float64, equal within 1e-9 relative.  A forward that raises does not."""
    ref = copy.deepcopy(m).cpu().double().eval()
    fc1, fc2, act, gate = (getattr(ref, n) for n in names)
    nc = fc1.weight.size(1)
    x = torch.randn(1, nc, 5, 7, dtype=torch.float64, generator=torch.Generator().manual_seed(nc))
    with torch.no_grad():
        z = x.mean((2, 3), keepdim=True)
        if type(fc1) is nn.Linear:
            g = gate(fc2(act(fc1(z.reshape(1, nc))))).reshape(1, nc, 1, 1)
        else:
            g = gate(fc2(act(fc1(z))))
        want = x * g
        try:
            got = ref(x)
        except Exception:
            return False
    if not torch.is_tensor(got) or got.shape != want.shape:
        return False
    return bool((got - want).abs().max() <= 1e-9 * want.abs().max())


def insertCBSqueezeExcite(rootModule, seTypes, threshold, cloneOutput=True):
    """Inside every nn.Sequential of rootModule, a squeeze-and-excitation module that directly follows a producer --
    chain.producers('insertCBGating') -- becomes a CBSqueezeExcite under its name, fed by that producer's changes
    (chain.insert_behind_producers: propChangeIndexes at the producer, the consumer rule behind the new module).

    seTypes: {class: (fc1, fc2, act, gate)}, the attribute names of the two layers, the activation between them and the
    gate of a class of the user's -- torch has no SE module; torchvision.ops.SqueezeExcitation is
    ('fc1', 'fc2', 'activation', 'scale_activation').  Only a module of EXACTLY such a type is converted, a subclass
    stays dense; so does one whose layers, activation (nn.ReLU, nn.SiLU) or gate (nn.Sigmoid, nn.Hardsigmoid,
    nn.Identity) are beyond CBChannelScale2d.  Before a type's first module is converted, that module and the formula
    x * g(fc2(act(fc1(mean(x))))) are run on one small random CPU tensor in float64: a class whose forward is
    something else is refused by name (CBinferError), never converted silently.  Returns rootModule."""
    threshold = _check_threshold(threshold)
    seTypes = dict(seTypes)
    for t, names in seTypes.items():
        if not (isinstance(t, type) and len(tuple(names)) == 4):
            raise CBinferError("insertCBSqueezeExcite: seTypes maps a class to its four attribute names (fc1, fc2, "
                               "act, gate), got %r: %r" % (t, names))
    checked = set()

    def convert(m):
        if type(m) not in seTypes:
            return None
        names = tuple(seTypes[type(m)])
        missing = [n for n in names if not isinstance(getattr(m, n, None), nn.Module)]
        if missing:
            raise CBinferError("insertCBSqueezeExcite: %s has no sub-module %s" % (type(m).__name__,
                                                                                    ", ".join(map(repr, missing))))
        fc1, fc2, act, gate = (getattr(m, n) for n in names)
        if type(gate) not in _GATE_MODULES:
            return None      # (a gate the kernel does not have: stays dense)
        try:
            cb = CBSqueezeExcite(threshold, fc1, fc2, act, gate=_GATE_MODULES[type(gate)])
        except CBinferError:
            return None      # (beyond the limits: stays dense)
        if type(m) not in checked:
            if not _follows_the_formula(m, names):
                raise CBinferError("insertCBSqueezeExcite: %s does not compute x * %s(%s(%s(%s(mean(x))))) (checked on "
                                   "a random tensor in float64, 1e-9 relative): it is not a squeeze-and-excitation "
                                   "block of that form and is not converted"
                                   % ((type(m).__name__,) + tuple(names[i] for i in (3, 1, 2, 0))))
            checked.add(type(m))
        return cb

    return insert_behind_producers(rootModule, producers('insertCBGating'), convert, cloneOutput=cloneOutput)
