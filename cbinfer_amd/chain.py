"""What the change-based operators behind a producer share on the host.

The frame: how an operand and its change information are taken apart (split_operand, check_map, operand_changes), the
form that lists every pixel (EVERY_PIXEL) and how a form is handed to the library (form_args), the ONE test for a state
that no longer fits its frame (state_fits: these modules and the layers of layer.py), the mask workspace and
hand-back of every mask-driven module, and CBStateModule, which CBAdd2d, CBPointwise2d, CBUpsample2d, CBConcat2d, the
shuffles, CBChannelReduce2d, CBResize2d, CBPad2d, CBBinary2d, CBGLU2d, CBChannelScale2d, CBGroupNorm2d and the pools of pool.py
(CBPoolMax2d, CBPoolAvg2d) derive from: the flags, the keyed workspace cache (_cached_work) and the state step
(_fresh_state).

The passes: the ONE table that says which module type counts as a producer for which pass (PRODUCERS, one row per
module type of the package -- every one: the package's `__all__`, its state helpers and the pycbinfer aliases are read
off it --, the exceptions as data) and its accessors (module_types(), producers(passName)), what is switched on at a
producer (hand_on_changes) and at the module behind a new one (link_consumer), and the ONE walk that puts an operator
behind its producers (insert_behind_producers).
"""
import functools
import importlib

import torch
import torch.nn as nn

from ._lib import C, CBinferError, ptr
from .conv2d_cg import ChangeIndexes, MaskChangeIndexes


# ---------------------------------------------------------------------------------------------------- operands
def split_operand(name, x, which):
    """(contiguous tensor, change indexes or None) of an operand: a tensor or ('changeIndexes', tensor, indexes)."""
    if type(x) == tuple:
        if len(x) != 3 or x[0] != 'changeIndexes':
            raise CBinferError("%s: %s is a tuple, but not ('changeIndexes', tensor, indexes)" % (name, which))
        x, indexes = x[1], x[2]
    else:
        indexes = None
    if not torch.is_tensor(x):
        raise CBinferError("%s: %s must be a tensor or the ('changeIndexes', tensor, indexes) tuple, got %s"
                           % (name, which, type(x).__name__))
    return x.detach().contiguous(), indexes


def check_map(name, x, which='the input', note=''):
    """CBinferError in the module's words unless `x` is a [1, C, H, W] map of float32 or float16.  which: how the module
    calls the operand; note: what it adds behind "tensor" (CBResize2d and CBPad2d: ' (batch 1)')."""
    if x.dim() != 4 or x.size(0) != 1:
        raise CBinferError("%s: %s must be a [1, C, H, W] tensor%s, got %s" % (name, which, note, tuple(x.shape)))
    if x.dtype not in (torch.float32, torch.float16):
        raise CBinferError("%s: float32 and float16 tensors only, got %s" % (name, x.dtype))


# The form (mask, list, capacity, device count) of an operand that lists every pixel: what a bare tensor carries, and what
# every operand counts as in a frame that writes a new state
EVERY_PIXEL = (None, None, 0, None)

# The three refusals of operand_changes -- indexes of another map, of another type, a buffer the kernels cannot read --
# as the consumers word them; filled with name, which, the two map sizes and the type's name.
OPERAND_WORDS = (
    "%(name)s: the change indexes of %(which)s address a %(h)dx%(w)d map, the tensor is a %(H)dx%(W)d map",
    "%(name)s: the change indexes of %(which)s must be an int32 tensor or a ChangeIndexes, got %(type)s",
    "%(name)s: the change indexes of %(which)s must be a contiguous one-dimensional int32 tensor on the tensor's device")
# ... and what CBDepthwiseConv2d (which: 'layer') and the general pools ('pool') ask of propagated indexes: their words
# and their rule for a MaskChangeIndexes
PROPAGATED = dict(
    words=("%(name)s: the propagated change indexes address a %(h)dx%(w)d map, this %(which)s's input map is %(H)dx%(W)d",
           "%(name)s: change indexes must be an int32 tensor or a ChangeIndexes",
           "%(name)s: propagated change indexes must be a contiguous int32 tensor on the input's device"),
    maskWhenMade=False, maskNeedsSize=True, contiguous=True)


def operand_changes(name, which, indexes, H, W, dev, spare, words=OPERAND_WORDS, maskWhenMade=True, maskNeedsSize=False,
                    contiguous=False):
    """(mask, list, capacity, device count) of an operand's changes on its H x W map; all None / 0: every pixel is
    listed.  `spare`: any int32 device buffer, which stands for the empty list (an empty tensor has no address).

    When a MaskChangeIndexes is taken as its mask -- one launch less than its list, which is then not needed -- is each
    consumer's own rule and decides what a FrameProgram records: maskWhenMade=False takes the list where the producer's
    kernel already made it; maskNeedsSize additionally asks for a mask that names this very map.  contiguous: an int32
    tensor is made contiguous instead of refused."""
    if indexes is None:
        return EVERY_PIXEL
    said = dict(name=name, which=which, H=H, W=W, type=type(indexes).__name__)
    if isinstance(indexes, ChangeIndexes):
        if indexes.size is not None and tuple(indexes.size) != (H, W):
            raise CBinferError(words[0] % dict(said, h=indexes.size[0], w=indexes.size[1]))
        if (isinstance(indexes, MaskChangeIndexes) and indexes._mask is not None and
                (maskWhenMade or not indexes._made) and (not maskNeedsSize or indexes.size == (H, W))):
            return indexes._mask, None, 0, None
        idx, count = indexes.buffer, indexes.count
    elif torch.is_tensor(indexes):
        idx, count = indexes.detach().contiguous() if contiguous else indexes.detach(), None
    else:
        raise CBinferError(words[1] % said)
    if idx.dtype != torch.int32 or idx.dim() != 1 or not idx.is_contiguous() or idx.device != dev:
        raise CBinferError(words[2] % said)
    cap = idx.numel()
    return None, (idx if cap else spare), cap, count


def form_args(form):
    """The four arguments a library call takes for an operand's form: mask, list, capacity, device count."""
    return ptr(form[0]), ptr(form[1]), form[2], ptr(form[3])


# ---------------------------------------------------------------------------------------------------- state
def state_fits(state, shape, like, dtype=None):
    """Whether the state tensor `state` still serves a frame: it has `shape`, and the dtype and device of `like`.
    dtype: the state's own where it is not the frame's (the f32 partials of an adaptive pool)."""
    return (state is not None and tuple(state.size()) == tuple(shape) and state.dtype == (dtype or like.dtype) and
            state.device == like.device)


def mask_workspace(Ho, Wo, dev, nbits=1):
    """The buffers of a mask-driven module on an Ho x Wo output map: nbits working masks `bits` (zero between frames),
    the frame's mask `copy`, and index buffer and count for a consumer that wants the list."""
    words = C.cbinfer_mask_words(Ho, Wo)
    return dict(bits=torch.zeros(nbits * words, dtype=torch.int64, device=dev),
                copy=torch.zeros(words, dtype=torch.int64, device=dev),
                idx=torch.empty(Ho * Wo, dtype=torch.int32, device=dev),
                count=torch.zeros(1, dtype=torch.int32, device=dev))


def frame_output(module, state):
    """The tensor a frame returns: a private copy of `state` -- or, with cloneOutput=False, the state itself, tagged, so
    that a consumer that keeps a reference (a CBConv2d with copyInput=False) copies it then."""
    if getattr(module, 'cloneOutput', True):
        return state.clone()
    state._cbinfer_inplace_state = True
    return state


def hand_back(module, state, copy, size, work, made=False):
    """What a frame returns: frame_output, and with propChangeIndexes the frame's mask `copy` on the size = (Ho, Wo)
    output map as a MaskChangeIndexes.  made: the frame's kernel already left the list and its count in work['idx'] /
    work['count'] (CBGroupedConv2d), so a consumer that wants the list launches nothing for it."""
    output = frame_output(module, state)
    if module.propChangeIndexes:
        return 'changeIndexes', output, MaskChangeIndexes(copy, size, work['idx'], work['count'], made=made)
    return output


class CBStateModule(nn.Module):
    """A module whose only state is `outputState`: the flags propChangeIndexes / cloneOutput, clearMemory,
    getStateTensors, transient work buffers that are neither state nor pickled and are kept per key (_cached_work), the
    step that keeps or replaces the state at the start of a frame (_fresh_state), and the hand-back (_result)."""
    _WORK = '_work'        # the slot of the work buffers in the instance's __dict__ (tests and old pickles read it)
    _TRANSIENT = ()        # further slots that are made again on demand (ctypes arguments)

    def __init__(self):
        super(CBStateModule, self).__init__()
        self.propChangeIndexes = False
        self.cloneOutput = True
        self.register_buffer('outputState', torch.zeros(0))
        self.clearMemory()

    def clearMemory(self):
        if 'outputState' not in self._buffers:
            self.register_buffer('outputState', torch.zeros(0))
        self.outputState = self.outputState.new_zeros(0)
        self.__dict__[self._WORK] = None

    def getStateTensors(self):
        return [self.outputState]

    def __getstate__(self):
        d = dict(self.__dict__)
        for name in (self._WORK,) + self._TRANSIENT:
            if name in d:
                d[name] = None
        return d

    def _cached_work(self, key, make):
        """The work buffers for `key`: those of the last frame if it had the same key, else dict(make(), key=key), which
        replaces them.  A make() that raises leaves the old ones in place."""
        work = self.__dict__.get(self._WORK)
        if work is None or work['key'] != key:
            work = self.__dict__[self._WORK] = dict(make(), key=key)
        return work

    def _fresh_state(self, shape, like, fill=None):
        """Keep outputState if it still serves a frame of `shape` with the dtype and device of `like`; else allocate it
        and return True: a new state is written completely, so the caller uses no operand's change information
        (EVERY_PIXEL).  fill: the value of a new state whose frame does go by the operand's list (the max pools: +inf)."""
        if state_fits(self.outputState, shape, like):
            return False
        state = torch.empty(tuple(shape), dtype=like.dtype, device=like.device)
        self.outputState = state if fill is None else state.fill_(fill)
        return True

    def _result(self, work, Ho, Wo):
        return hand_back(self, self.outputState, work['copy'], (Ho, Wo), work)


# ---------------------------------------------------------------------------------------------------- producers
_POOLS = ('insertCBPooling', 'insertCBPooling(generalGeometry=True)')
PASSES = ('linkDepthwise', 'insertCBPointwise', 'insertCBTransposedConv', 'insertCBUpsampling', 'insertCBRearrange',
          'insertCBChannelOps', 'insertCBPadding', 'insertCBGating', 'insertCBResize') + _POOLS

# THE table of the producers: one row per module type of the package -- (type, its module, rule, passes) --, which says
# in front of which passes' operator the type (exactly, not a subclass) counts as a producer: one that leaves every pixel
# outside its change list bit for bit as it was and can hand that list on.  BUT: every pass of PASSES but these; ONLY:
# these and no other.  The order of the rows is the order of every set.
BUT, ONLY = 'all passes but', 'only'
PRODUCERS = (
    ('CBConv2d', 'conv2d', BUT, ()),
    # (insertCBPooling is the reference's hand-written rule: behind a CBConv2d, nothing else)
    ('CBPoolMax2d', 'pool', BUT, _POOLS),
    ('CBPoolAvg2d', 'pool', BUT, _POOLS),
    ('CBAdd2d', 'residual', BUT, _POOLS),
    ('CBResidual', 'residual', BUT, _POOLS),
    ('CBUpsample2d', 'decoder', BUT, _POOLS),
    # kept as found: never in front of an upsampling or a resize
    ('CBConvTranspose2d', 'tconv', BUT, _POOLS + ('insertCBUpsampling', 'insertCBResize')),
    ('CBDepthwiseConv2d', 'dwconv', BUT, _POOLS),
    # (the general pools take the mask of CBPointwise2d and CBPad2d)
    ('CBPointwise2d', 'pointwise', BUT, ('insertCBPooling',)),
    ('CBPixelShuffle2d', 'rearrange', BUT, _POOLS),
    ('CBChannelShuffle2d', 'rearrange', BUT, _POOLS),
    ('CBResize2d', 'resize', BUT, _POOLS),
    ('CBPad2d', 'pad', BUT, ('insertCBPooling',)),
    ('CBBinary2d', 'binary', BUT, _POOLS),
    ('CBGLU2d', 'binary', BUT, _POOLS),
    ('CBGated', 'binary', BUT, _POOLS),
    # kept as found: the passes written after it take it, the four before it (linkDepthwise, insertCBPointwise,
    # insertCBTransposedConv, insertCBUpsampling) do not
    ('CBGroupedConv2d', 'groupconv', ONLY, ('insertCBRearrange', 'insertCBChannelOps', 'insertCBResize',
                                            'insertCBPadding', 'insertCBGating')),
    # kept as found: as CBGroupedConv2d, and not for insertCBRearrange
    ('CBChannelReduce2d', 'chanreduce', ONLY, ('insertCBChannelOps', 'insertCBResize', 'insertCBPadding',
                                               'insertCBGating')),
    # a producer for no pass: its forward takes a list of operands and never stands in an nn.Sequential
    ('CBConcat2d', 'decoder', ONLY, ()),
    # a producer for no pass, kept as found (it can hand the list it was given on: propChangeIndexes)
    ('CBTail1x1', 'conv2d', ONLY, ()),
    # producers for no pass, kept as found: the channel attention scale and its wiring module (a wrapper: its pool and
    # its scale keep the state) ...
    ('CBChannelScale2d', 'chanscale', ONLY, ()),
    ('CBSqueezeExcite', 'chanscale', ONLY, ()),
    # ... and the group norm
    ('CBGroupNorm2d', 'groupnorm', ONLY, ()),
)


@functools.lru_cache(maxsize=None)
def module_types():
    """The class of every row of PRODUCERS, in row order.  (Imported here, on first use: their modules import this
    one.)"""
    return tuple(getattr(importlib.import_module('.' + module, __package__), name) for name, module, _, _ in PRODUCERS)


@functools.lru_cache(maxsize=None)
def producers(passName):
    """The module types (exactly, not a subclass) that the pass `passName` of PASSES accepts in front of its module, in
    the order of PRODUCERS."""
    if passName not in PASSES:
        raise CBinferError("chain.producers: %r is no pass of %s" % (passName, PASSES))
    return tuple(t for t, (_, _, rule, passes) in zip(module_types(), PRODUCERS)
                 if (passName in passes) == (rule is ONLY))


def hand_on_changes(prod):
    """Switch the change output of the producer `prod` on for the consumer behind it: propChangeIndexes (a CBResidual's
    at its `.add`, a CBGated's at its `.mul`); a 2x2 CBPoolMax2d of the reference's kind also hands on the
    OUTPUT-resolution list."""
    from .binary import CBGated
    from .pool import CBPoolMax2d
    from .residual import CBResidual
    (prod.add if type(prod) is CBResidual else prod.mul if type(prod) is CBGated else prod).propChangeIndexes = True
    if type(prod) is CBPoolMax2d and not prod.__dict__.get('_general'):
        prod.downsampleIndexes = True      # (the list of the pool's input addresses another map)


def is_1x1(m):
    """A 1x1 / stride-1 / padding-0 CBConv2d: the consumer that reads exactly the pixels it is handed."""
    from .conv2d import CBConv2d
    return (type(m) is CBConv2d and tuple(m.kernel_size) == (1, 1) and tuple(m.stride) == (1, 1) and
            tuple(m.padding) == (0, 0))


def link_consumer(front, consumer, handOn=True):
    """The consumer rule, for the module `consumer` directly behind `front`: a 1x1 / stride-1 / padding-0 CBConv2d takes
    the changes of `front` (propChangeIndexes there); any other CBConv2d (exactly) reads a map that is the state of
    `front` or may be, so it needs its own input copy (copyInput) unless it runs in feedback mode -- a k x k CBConv2d
    that is handed indexes would skip its own detection, which would be wrong.  handOn=False: `front` never hands on,
    a 1x1 layer is a CBConv2d like any other (insertCBUpsampling, insertCBTransposedConv)."""
    from .conv2d import CBConv2d
    if handOn and is_1x1(consumer):
        front.propChangeIndexes = True
    elif type(consumer) is CBConv2d and not consumer.feedbackLoop:
        consumer.copyInput = True


def insert_behind_producers(rootModule, producers, convert, cloneOutput=None, handOn=True):
    """The walk of the passes that put ONE change-based operator behind a producer.  Inside every nn.Sequential (exactly)
    of rootModule, for every module that directly follows one whose exact type is in `producers`: convert(module)
    returns the change-based module to put in its place under its name, or None -- not the pass's operator, or beyond
    the library's limits -- to leave it the dense torch operator.  The producer's change output is switched on
    (hand_on_changes), the new module gets `cloneOutput` unless that is None, and the module behind it the consumer
    rule (link_consumer with handOn).  A new module counts as a producer for the next one where its type is in
    `producers`.  Returns rootModule."""
    for seq in [m for m in rootModule.modules() if type(m) is nn.Sequential]:
        names = list(seq._modules.keys())
        for pos in range(1, len(names)):
            prod = seq._modules[names[pos - 1]]
            cb = convert(seq._modules[names[pos]]) if type(prod) in producers else None
            if cb is None:
                continue
            hand_on_changes(prod)
            if cloneOutput is not None:
                cb.cloneOutput = cloneOutput
            seq._modules[names[pos]] = cb
            if pos + 1 < len(names):
                link_consumer(cb, seq._modules[names[pos + 1]], handOn)
    return rootModule
