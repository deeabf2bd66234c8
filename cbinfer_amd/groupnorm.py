"""Change-based group norm and instance norm: CBGroupNorm2d and insertCBGroupNorm (cb_groupnorm.hip).

The reference has no norm that reduces over the pixels.  nn.GroupNorm, nn.InstanceNorm2d and GroupNorm(1, C) ended the
change-based chain: a group's (mean, rstd) moves a little in every frame of a video, so the dense operator rewrites the
whole map and the layer behind it finds a map that moved everywhere a little.  The module here keeps a second level of
state -- float64 partial sums over the segments of a row, as the adaptive pools keep theirs -- and applies the library's
own rule to the statistics, as CBChannelScale2d applies it to its gates: a group whose statistics moved by no more than
`threshold` is HELD at the pair it last used and recomputed only at the operand's changed pixels; a group that moved by
more TRIPS: it takes the new pair and its planes are recomputed completely.  At threshold = 0 this is the dense operator.
"""
import ctypes

import torch
import torch.nn as nn

from ._lib import C, CBinferError, check, dtype_code, ptr, require_device, stream_ptr
from .chain import (EVERY_PIXEL, CBStateModule, check_map, form_args, insert_behind_producers, mask_workspace,
                    operand_changes, producers, split_operand, state_fits)

MAX_CHANNELS = 4096
# the buffers that keep their dtype under .half() / .float() / .double(): the kernel's
_KEPT = (('gamma', torch.float32), ('beta', torch.float32), ('held', torch.float32), ('partials', torch.float64))


def _check_threshold(threshold):
    t = float(threshold)
    if not t >= 0.0:      # (also a NaN)
        raise CBinferError("CBGroupNorm2d: threshold=%r must be a number >= 0" % (threshold,))
    return t


def _groups_of(m):
    """(channels, groups) of the norm `m`, refusing by name what is not this operator."""
    if type(m) is nn.GroupNorm:
        nc, groups = int(m.num_channels), int(m.num_groups)
    elif type(m) is nn.InstanceNorm2d:
        if m.track_running_stats:
            raise CBinferError("CBGroupNorm2d: an nn.InstanceNorm2d with track_running_stats=True normalises with its "
                               "running statistics in eval mode: that is a per-channel affine (CBPointwise2d), not this "
                               "operator")
        nc = groups = int(m.num_features)
    else:
        raise CBinferError("CBGroupNorm2d: %s is not supported, only an nn.GroupNorm or an nn.InstanceNorm2d (exactly "
                           "those types, not a subclass)" % type(m).__name__)
    if nc < 1 or groups < 1 or nc % groups != 0:
        raise CBinferError("CBGroupNorm2d: %d groups do not divide %d channels" % (groups, nc))
    if nc > MAX_CHANNELS:
        raise CBinferError("CBGroupNorm2d: %d channels, the library takes C <= %d" % (nc, MAX_CHANNELS))
    eps = float(m.eps)
    if not (eps >= 0.0 and eps != float('inf')):
        raise CBinferError("CBGroupNorm2d: eps=%r must be a finite number >= 0" % (m.eps,))
    return nc, groups, eps


class CBGroupNorm2d(CBStateModule):
    """torch's group norm on a [1, C, H, W] map, out = (a - mean[g]) rstd[g] gamma[c] + beta[c] (optionally followed by
    a ReLU), with (mean[g], rstd[g]) the statistics group g last TRIPPED at (no counterpart in the reference; the
    arithmetic is specified in include/cbinfer_hip.h).

    m: an nn.GroupNorm, or an nn.InstanceNorm2d with track_running_stats=False (G = C, affine or not) -- exactly those
    types, not a subclass; GroupNorm(1, C) is G = 1.  An instance norm with running statistics is refused: in eval mode
    it is a per-channel affine.  weight / bias are COPIED into float32 buffers (gamma, beta; None without an affine),
    which follow .to() and stay float32 under .half(); later edits of `m` are not followed.  C <= 4096.

    threshold: group g trips in a frame when |mean - heldMean| * heldRstd or |rstd - heldRstd| / heldRstd is strictly
    more than this (a NaN trips): the shift of the mean in held standard deviations, and the relative change of rstd.
    Only then the group takes the new pair and its planes are recomputed completely; every other group is recomputed at
    the operand's changed pixels alone, with the held pair, so slow drift adds up until it trips.  To first order the
    normalised value y of a held group is off by at most threshold * (1 + |y|), before gamma.  threshold = 0 gives the
    dense result.  It is read again in every frame.

    forward(a): a is a [1, C, H, W] tensor (no change information: every pixel is recomputed) or the ('changeIndexes',
    tensor, indexes) tuple of a producer with propChangeIndexes, taken as CBPointwise2d takes it.  The statistics are
    float64 sums of float64 partials over 64-column row segments (state `partials`, [2, C, H, ceil(W / 64)]): a frame
    re-sums only the segments that hold a changed pixel and never reads the others.

    State: outputState, held (float32 [2, G]: means, rstds) and partials (float64, whatever the map's dtype), all three
    from getStateTensors(), all dropped by clearMemory(); a state that does not fit the frame makes the frame fresh.
    The flags are CBAdd2d's: cloneOutput=False hands out the state itself, tagged; propChangeIndexes hands on the
    frame's mask as a MaskChangeIndexes: the operand's changed pixels -- or EVERY pixel in a frame in which a group
    tripped (a per-pixel mask cannot name a group).  lastTrippedGroups(): the groups that tripped in the last frame
    (synchronises: for tests and for tuning)."""

    _WORK = '_gnWork'
    _TRANSIENT = ('_epsArg',)

    def __init__(self, m, threshold, relu=False):
        super(CBGroupNorm2d, self).__init__()
        self.threshold = _check_threshold(threshold)
        self.num_channels, self.num_groups, self.eps = _groups_of(m)
        self.relu = bool(relu)
        self.source = type(m).__name__
        weight, bias = getattr(m, 'weight', None), getattr(m, 'bias', None)
        self.register_buffer('gamma', weight.detach().float().clone().contiguous() if weight is not None else None)
        self.register_buffer('beta', bias.detach().float().clone().contiguous() if bias is not None else None)
        # (the states behind the operands, as state_dict() lists them)
        for name in ('outputState', 'held', 'partials'):
            self._buffers[name] = self._buffers.pop(name)
        self.__dict__['_epsArg'] = None

    def clearMemory(self):
        super(CBGroupNorm2d, self).clearMemory()
        for name, dtype in _KEPT[2:]:
            old = self._buffers.get(name)
            if name not in self._buffers:
                self.register_buffer(name, torch.zeros(0))
            setattr(self, name, torch.zeros(0, dtype=dtype, device=old.device if old is not None else None))

    def getStateTensors(self):
        return [self.outputState, self.held, self.partials]

    def _apply(self, fn, *args, **kwargs):
        # (.half() / .float() / .double() convert every floating-point buffer: the affine, the held statistics and the
        #  float64 partials keep the kernel's dtype)
        keep = {n: (self._buffers[n], d) for n, d in _KEPT if self._buffers.get(n) is not None}
        super(CBGroupNorm2d, self)._apply(fn, *args, **kwargs)
        for n, (t, d) in keep.items():
            if self._buffers[n].dtype != d:
                self._buffers[n] = t.to(self._buffers[n].device)
        return self

    def _workspace(self, H, W, dev):
        """The mask workspace, and launch 2's outputs: this frame's statistics and the trip flag of every group."""
        G = self.num_groups
        return self._cached_work((H, W, dev), lambda: dict(
            mask_workspace(H, W, dev), stats=torch.zeros(2, G, dtype=torch.float32, device=dev),
            tripped=torch.zeros(G, dtype=torch.int32, device=dev)))

    def lastTrippedGroups(self):
        """The indexes of the groups that tripped in the last frame (empty before the first).  Synchronises."""
        work = self.__dict__.get(self._WORK)
        return [int(g) for g in work['tripped'].nonzero().flatten().tolist()] if work is not None else []

    def _eps_arg(self):
        arg = self.__dict__.get('_epsArg')
        if arg is None or arg[0] != self.eps:
            arg = self.__dict__['_epsArg'] = (ctypes.c_double * 1)(self.eps)
        return arg

    def forward(self, a):
        a, ia = split_operand('CBGroupNorm2d', a, 'operand a')
        check_map('CBGroupNorm2d', a, 'operand a')
        nc, H, W = a.size(1), a.size(2), a.size(3)
        if nc != self.num_channels:
            raise CBinferError("CBGroupNorm2d: operand a has %d channels, the norm was made for %d"
                               % (nc, self.num_channels))
        if H * W >= 2 ** 31:
            raise CBinferError("CBGroupNorm2d: a %dx%d map is beyond the library's limits (H W within an int32)" % (H, W))
        threshold = _check_threshold(self.threshold)
        require_device(a)
        for name in ('gamma', 'beta'):
            t = getattr(self, name)
            if t is not None and t.device != a.device:
                raise CBinferError("CBGroupNorm2d: operand a is on %s, %s on %s (move the module with .to())"
                                   % (a.device, name, t.device))
        G = self.num_groups
        work = self._workspace(H, W, a.device)
        form = operand_changes('CBGroupNorm2d', 'operand a', ia, H, W, a.device, work['idx'])
        fresh = self._fresh_state(a.shape, a)
        pshape = (2, nc, H, (W + 63) // 64)
        if (fresh or not state_fits(self.held, (2, G), a, torch.float32) or
                not state_fits(self.partials, pshape, a, torch.float64)):
            # (written completely, with every group's statistics taken as they are: no change information is used)
            self.held = torch.zeros(2, G, dtype=torch.float32, device=a.device)
            self.partials = torch.zeros(pshape, dtype=torch.float64, device=a.device)
            fresh, form = True, EVERY_PIXEL
        check(C.cbinfer_cbgroupnorm_forward(ptr(a), ptr(self.gamma), ptr(self.beta), ptr(self.outputState),
                                            ptr(self.partials), ptr(work['stats']), ptr(self.held), ptr(work['tripped']),
                                            *form_args(form), ptr(work['bits']), ptr(work['copy']), nc, G, H, W,
                                            self._eps_arg(), int(self.relu), threshold, int(fresh), dtype_code(a),
                                            stream_ptr(a)))
        return self._result(work, H, W)

    def __repr__(self):
        return 'CBGroupNorm2d (%s, channels=%d, groups=%d, eps=%s, affine=%s, relu=%s, threshold=%s, propChgIdxs=%s)' % (
            self.source, self.num_channels, self.num_groups, self.eps, self.gamma is not None, self.relu, self.threshold,
            self.propChangeIndexes)


def insertCBGroupNorm(rootModule, threshold, cloneOutput=True):
    """Inside every nn.Sequential of rootModule, an nn.GroupNorm or an nn.InstanceNorm2d without running statistics
    (exactly those types) that directly follows a producer -- chain.producers('insertCBChannelOps') -- becomes a
    CBGroupNorm2d under its name, fed by that producer's changes (chain.insert_behind_producers: propChangeIndexes at the
    producer, the consumer rule behind the new module).  An nn.ReLU (exactly) directly behind such a norm is absorbed:
    relu=True, and the ReLU leaves the container.  A module beyond the limits -- more than 4096 channels, an instance
    norm with running statistics -- stays dense, and so does the ReLU behind it.  Returns rootModule."""
    threshold = _check_threshold(threshold)
    prods = producers('insertCBChannelOps')

    def made(m, relu):
        if type(m) not in (nn.GroupNorm, nn.InstanceNorm2d):
            return None
        try:
            return CBGroupNorm2d(m, threshold, relu=relu)
        except CBinferError:
            return None      # (beyond the limits: stays dense)

    # the ReLUs to absorb leave first; the walk below then links the module that stood behind them
    absorbed = set()
    for seq in [m for m in rootModule.modules() if type(m) is nn.Sequential]:
        names = list(seq._modules.keys())
        pos = 1
        while pos < len(names) - 1:
            prod, norm, act = (seq._modules[names[pos + d]] for d in (-1, 0, 1))
            if type(prod) in prods and type(act) is nn.ReLU and made(norm, True) is not None:
                absorbed.add(id(norm))
                del seq._modules[names.pop(pos + 1)]
            pos += 1
    return insert_behind_producers(rootModule, prods, lambda m: made(m, id(m) in absorbed), cloneOutput=cloneOutput)
