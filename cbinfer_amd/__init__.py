"""cbinfer_amd -- CBinfer's change-based convolution hot path, written for AMD MI355X (gfx950).

The public surface is the reference's `pycbinfer` package (pycbinfer/__init__.py): convert(),
clearMemory(), getStateTensors(), propChangeIndexesOf1x1(), tuneThresholdParameters() and the
CBConv2d / CBPoolMax2d modules.  `import pycbinfer` (the alias package at the repository root)
resolves to this package, including the `pycbinfer.conv2d.CBConv2d` class paths that pickled
reference models name.
"""
import torch
import torch.nn as nn

from . import _lib                      # loads libcbinfer_hip.so; raises ImportError if not built
from . import chain
from .conv2d import CBConv2d
from .pool import CBPoolMax2d, computes_suppression
from .pool import CBPoolAvg2d
from .conv2d import CBTail1x1
from .conv2d_cg import ChangeIndexes, ChannelConcat
from .pipeline import FramePipeline
from .batch import SequenceBatch
from .branches import BranchGroup
from .program import FrameProgram
from .residual import CBAdd2d, CBResidual, foldBatchNorm
from .decoder import CBUpsample2d, CBConcat2d, insertCBUpsampling
from .tconv import CBConvTranspose2d, insertCBTransposedConv
from .dwconv import CBDepthwiseConv2d, linkDepthwise
from .pointwise import CBPointwise2d, insertCBPointwise
from .groupconv import CBGroupedConv2d, linkGrouped
from .rearrange import CBPixelShuffle2d, CBChannelShuffle2d, insertCBRearrange
from .chanreduce import CBChannelReduce2d, insertCBChannelOps
from .resize import CBResize2d, insertCBResize
from .pad import CBPad2d, insertCBPadding, splitConvPadding
from .binary import CBBinary2d, CBGLU2d, CBGated, insertCBGating
from .chanscale import CBChannelScale2d, CBSqueezeExcite, insertCBSqueezeExcite
from .groupnorm import CBGroupNorm2d, insertCBGroupNorm

__version__ = "0.1.0"

VERBOSE = False   # the reference prints one line per substituted node; opt-in here


def _log(msg):
    if VERBOSE:
        print(msg)


def _rebuild(container, rule):
    """A new nn.Sequential holding the children of `container` under their old names, each passed
    through rule(child, before, after) -> the module to put in its place, or None to leave it out.
    `before` / `after` are the child's neighbours in the ORIGINAL container (None at the ends)."""
    kids = list(container.named_children())
    out = nn.Sequential()
    for pos, (name, child) in enumerate(kids):
        before = kids[pos - 1][1] if pos > 0 else None
        after = kids[pos + 1][1] if pos + 1 < len(kids) else None
        keep = rule(child, before, after)
        if keep is not None:
            out.add_module(name, keep)
    return out


def subsitute(node, threshold=1e-1, finegrained=False, generalGeometry=False, depthwise=False, grouped=False):
    """(module, replaced?): exactly torch.nn.Conv2d -- not a subclass -- becomes a CBConv2d sharing its
    parameters (reference: __init__.py:10-17; the spelling of the name is the reference's).  generalGeometry=True
    also takes strided, dilated, freely padded and bias-free convolutions (CBConv2d(..., generalGeometry=True)).
    depthwise=True: a depthwise convolution (groups == in_channels > 1) becomes a CBDepthwiseConv2d.  grouped=True: a
    convolution with groups > 1 becomes a CBGroupedConv2d (a depthwise one only where depthwise=True does not take it).
    With the defaults every grouped convolution is refused."""
    if type(node) is not nn.Conv2d:
        return node, False
    if depthwise and node.groups == node.in_channels > 1:
        _log('replacing depthwise conv2d')
        return CBDepthwiseConv2d(node, threshold), True
    if grouped and node.groups > 1:
        _log('replacing grouped conv2d')
        return CBGroupedConv2d(node, threshold), True
    _log('replacing conv2d')
    cb = CBConv2d(node, threshold, generalGeometry=True) if generalGeometry else CBConv2d(node, threshold)
    cb.finegrained = finegrained
    return cb, True


def convertRecur(m, ignoreList=[], threshold=1e-1, finegrained=False, generalGeometry=False, depthwise=False,
                 grouped=False):
    """(converted nn.Sequential, anything changed?) for the children of `m` (reference: __init__.py:20-45):
    names preserved; nn.Dropout and the types of ignoreList dropped; nested nn.Sequential containers
    converted recursively -- as in the reference (:28) WITHOUT handing `finegrained` down; every other
    child goes through subsitute().  If anything changed the ReLUs are merged right away: the reference
    calls convert() on its result at this point (:43-44), a pass that finds nothing left to substitute
    and so amounts to mergeReLURecur()."""
    dropped = tuple(ignoreList) + (nn.Dropout,)
    outcomes = []

    def rule(child, before, after):
        if type(child) is nn.Sequential:
            child, hit = convertRecur(child, ignoreList, threshold, generalGeometry=generalGeometry,
                                      depthwise=depthwise, grouped=grouped)
        elif type(child) in dropped:
            _log('removing node %s' % (type(child),))
            child, hit = None, True
        else:
            child, hit = subsitute(child, threshold=threshold, finegrained=finegrained, generalGeometry=generalGeometry,
                                   depthwise=depthwise, grouped=grouped)
        outcomes.append(hit)
        return child

    mout = _rebuild(m, rule)
    changed = any(outcomes)
    if changed:
        mout = mergeReLURecur(mout)
    return mout, changed


def mergeReLURecur(m):
    """An nn.ReLU right behind a CBConv2d is absorbed into it (withReLU=True) and leaves the container,
    nested nn.Sequential containers included (reference: __init__.py:47-66).  A CBDepthwiseConv2d absorbs an nn.ReLU
    and an nn.ReLU6 (reluCap = 6.0); a CBGroupedConv2d absorbs an nn.ReLU; an nn.ReLU6 behind a CBConv2d or a
    CBGroupedConv2d stays the dense module it is."""
    def rule(child, before, after):
        if type(child) is nn.Sequential:
            return mergeReLURecur(child)
        if type(child) in (CBConv2d, CBGroupedConv2d) and type(after) is nn.ReLU:
            child.withReLU = True
        if type(child) is CBDepthwiseConv2d and type(after) in (nn.ReLU, nn.ReLU6):
            child.withReLU = True
            child.reluCap = 6.0 if type(after) is nn.ReLU6 else None
        if type(child) in (nn.ReLU, nn.ReLU6) and type(before) is CBDepthwiseConv2d:
            _log('merging ReLU layer')
            return None
        if type(child) is nn.ReLU and type(before) in (CBConv2d, CBGroupedConv2d):
            _log('merging ReLU layer')
            return None
        return child
    return _rebuild(m, rule)


def _sequentials(rootModule):
    return [m for m in rootModule.modules() if type(m) == nn.Sequential]


def propChangeIndexesOf1x1(rootModule):
    """Let every CBConv2d that feeds a 1x1 CBConv2d pass its change indexes on, so the 1x1 layer skips
    its own change detection (reference: __init__.py:68-77).

    Deliberate deviation: the reference compares the kernel_size TUPLE with the LIST [1,1] (:73), which
    is never equal, so there this function is a no-op and the applications set the flags by hand
    (sceneLabeling/modelLoader.py:43-44).  Here the comparison is done on values, i.e. the function
    does what its name and the hand-written code say."""
    for seq in _sequentials(rootModule):
        kids = list(seq.children())
        for producer, consumer in zip(kids[:-1], kids[1:]):
            # (a strided or padded 1x1 layer -- general geometry -- does not keep the map: it runs its own detection)
            if (type(producer) == CBConv2d and type(consumer) == CBConv2d and
                    tuple(consumer.kernel_size) == (1, 1) and tuple(consumer.stride) == (1, 1) and
                    tuple(consumer.padding) == (0, 0)):
                _log('enabling propagation of change indexes for 1x1')
                producer.propChangeIndexes = True
    return rootModule


def insertCBPooling(rootModule, cloneOutput=True, generalGeometry=False, adaptive=False, nmsTypes=None):
    """what sceneLabeling/modelLoader.py:62-78 does by hand for experiments 5/6, for any
    converted network: every 2x2/stride-2 nn.MaxPool2d that directly follows a CBConv2d inside an
    nn.Sequential becomes a CBPoolMax2d fed by that layer's change indexes (propChangeIndexes on the
    conv), so only the windows holding a changed pixel are pooled again.  A CBConv2d consuming the pool
    then needs its own input copy (copyInput) unless it runs in feedback mode.  generalGeometry=True: every
    nn.MaxPool2d and nn.AvgPool2d within the library's limits (CBPoolMax2d(m, generalGeometry=True), CBPoolAvg2d) is
    converted, also directly behind a CBPointwise2d or a CBPad2d (the general pools take their mask); a pool beyond them
    stays the dense torch operator.  Both sets are rows of chain.producers().  adaptive=True (with generalGeometry=True
    only): an nn.AdaptiveMaxPool2d / nn.AdaptiveAvgPool2d behind the same producers is converted too -- the global pool of
    a classifier head or a squeeze, the bins of a pyramid; one the modules refuse (return_indices=True) stays dense.

    nmsTypes (with generalGeometry=True only): {class: keywords}, a class of the user's that computes peak suppression --
    torch has no module for it -- and the keywords of the CBPoolMax2d that replaces it, e.g.
    {SimpleNMS: dict(kernel_size=3, suppress='window', floor=0.1)}; peakList=N may be among them.  A module of EXACTLY
    such a type behind the same producers becomes CBPoolMax2d(nn.MaxPool2d(k, 1, k // 2), generalGeometry=True, ...).
    Before a type's first module is converted it is run against the rule in dense torch operators
    (pool.suppression_formula) on a small CPU tensor with plateaus and values below the floor: a class whose forward is
    something else is refused by name (CBinferError), never converted silently.
    Returns rootModule."""
    if adaptive and not generalGeometry:
        raise _lib.CBinferError("insertCBPooling: adaptive=True needs generalGeometry=True (the adaptive pools are "
                                "general-geometry modules)")
    if nmsTypes is not None and not generalGeometry:
        raise _lib.CBinferError("insertCBPooling: nmsTypes needs generalGeometry=True (peak suppression is a "
                                "general-geometry module)")
    nmsTypes = dict(nmsTypes or {})
    for t, kw in nmsTypes.items():
        if not (isinstance(t, type) and isinstance(kw, dict) and {'kernel_size', 'suppress'} <= set(kw) and
                set(kw) <= {'kernel_size', 'suppress', 'floor', 'peakList'}):
            raise _lib.CBinferError("insertCBPooling: nmsTypes maps a class to the keywords kernel_size, suppress and, "
                                    "if wanted, floor and peakList, got %r: %r" % (t, kw))
    checkedNms = set()

    def _suppressing(m):
        kw = dict(nmsTypes[type(m)])
        k = _pair(kw.pop('kernel_size'))
        if not all(isinstance(v, int) and not isinstance(v, bool) for v in k) or len(k) != 2:
            raise _lib.CBinferError("insertCBPooling: nmsTypes[%s]: kernel_size=%r is not an int or a pair of ints"
                                    % (type(m).__name__, k))
        cb = CBPoolMax2d(torch.nn.MaxPool2d(k, 1, (k[0] // 2, k[1] // 2)), generalGeometry=True, **kw)
        if type(m) not in checkedNms:
            if not computes_suppression(m, k, kw['suppress'], kw.get('floor')):
                raise _lib.CBinferError(
                    "insertCBPooling: %s does not compute peak suppression with kernel_size=%s, suppress=%r, floor=%r "
                    "(checked bit for bit on a CPU tensor with plateaus and values below the floor): it is not "
                    "converted" % (type(m).__name__, k, kw['suppress'], kw.get('floor')))
            checkedNms.add(type(m))
        return cb

    def _pair(v):
        return tuple(v) if isinstance(v, (tuple, list)) else (v, v)

    def _converted(pool):
        if type(pool) in nmsTypes:
            return _suppressing(pool)
        if generalGeometry:
            try:
                if type(pool) == torch.nn.MaxPool2d:
                    return CBPoolMax2d(pool, generalGeometry=True)
                if type(pool) == torch.nn.AvgPool2d or (adaptive and type(pool) == torch.nn.AdaptiveAvgPool2d):
                    return CBPoolAvg2d(pool)
                if adaptive and type(pool) == torch.nn.AdaptiveMaxPool2d:
                    return CBPoolMax2d(pool, generalGeometry=True)
            except _lib.CBinferError:
                pass      # (beyond the limits: stays dense)
            return None
        if (type(pool) == torch.nn.MaxPool2d and
                _pair(pool.kernel_size) == (2, 2) and _pair(pool.stride) == (2, 2) and
                _pair(pool.padding) == (0, 0) and _pair(pool.dilation) == (1, 1)):
            return CBPoolMax2d(pool)
        return None

    producers = chain.producers('insertCBPooling(generalGeometry=True)' if generalGeometry else 'insertCBPooling')
    for seq in _sequentials(rootModule):
        names = list(seq._modules.keys())
        for a, b in zip(names[:-1], names[1:]):
            conv, pool = seq._modules[a], seq._modules[b]
            cb = _converted(pool) if type(conv) in producers else None
            if cb is not None:
                _log('change-based pooling after %s' % a)
                conv.propChangeIndexes = True
                cb.cloneOutput = cloneOutput
                seq._modules[b] = cb
                nxt = names.index(b) + 1
                if nxt < len(names) and type(seq._modules[names[nxt]]) == CBConv2d:
                    consumer = seq._modules[names[nxt]]
                    if not consumer.feedbackLoop:
                        consumer.copyInput = True
    return rootModule


def fusePoolingIntoDetection(rootModule, enabled=True):
    """Execution-level fusion (no change of results): a CBPoolMax2d whose consumer inside the same
    nn.Sequential is a feedback-mode CBConv2d stops pooling and lets that layer compute the pooled values
    inside its change detection (CBPoolMax2d.lazy, cbinfer_cbconv2d_forward_pooled) -- one launch less
    per pool and frame.  The pooled map is then not materialised, so the pool must not hand its indexes
    on (propChangeIndexes) and nothing else may read its outputState.  Returns rootModule."""
    for seq in _sequentials(rootModule):
        kids = list(seq.children())
        for pool, consumer in zip(kids[:-1], kids[1:]):
            if type(pool) == CBPoolMax2d:
                # (a feedback-mode layer, or -- round 4 -- a fine-grained one in its in-place form: its split-state frame
                #  takes the pool's input as it is, cbinfer_split_forward_fg; other fine-grained frames pool first)
                # (a general-geometry consumer has no pooled detection: the pool in front of it keeps pooling itself)
                # (a pool of any other window than 2x2/s2/p0 -- cb_pool2d.hip -- is never folded: it pools itself)
                pool.lazy = bool(enabled and type(consumer) == CBConv2d and not pool.propChangeIndexes and
                                 not pool.__dict__.get('_general') and not consumer.__dict__.get('_geom') and
                                 ((consumer.feedbackLoop and not consumer.finegrained) or
                                  (consumer.finegrained and consumer.fgInPlace) or
                                  # (a layer that keeps a copy of its input: the copy-all detection of the split-state
                                  #  kernels takes the pool; where those do not take the layer it pools densely)
                                  (consumer.copyInput and not consumer.feedbackLoop and not consumer.finegrained)))
    return rootModule


def fuseDetectionIntoProducer(rootModule, enabled=True, windowOrder='auto'):
    """Execution-level fusion (no change of results): inside every nn.Sequential a run  CBConv2d (producer) ->
    lazy CBPoolMax2d -> feedback-mode CBConv2d (consumer)  lets the PRODUCER's contraction launch also be the consumer's
    pooled change detection when the producer runs on the row-pair kernel (cb_rowpair.hip: a workgroup owns whole 2x2
    windows) and the consumer on the split-state kernels: one launch less per frame, and the freshly computed outputs
    are compared with the consumer's state while they are still in the workgroup's LDS.  Decided per frame
    (CBConv2d._next_detect): the first frames of a sequence, a frame after the consumer's state was restored or its
    threshold changed run the separate detection.  Call after fusePoolingIntoDetection.  Returns rootModule.

    Round 6: a producer that runs on the split-state kernels itself (<= 64 output channels, a shallow contraction -- the
    16 -> 64 layer of the scene-labeling network) does the same with its contraction in pooling-WINDOW order
    (cbinfer_split_conv_next).  `windowOrder`: True, False (such a producer stays in pixel order, the consumer's detection in
    a launch of its own) or 'auto' (default): the window-order tile holds 16 whole windows -- the unchanged pixels of a
    touched window cost slots -- and its prologue and epilogue are longer, which pays (measured at 160 x 240: 1.7-2.8 us per
    frame from 2 to 35 % recomputed pixels) while its tiles fit ONE round of the grid and costs 2-3 us per round beyond; 'auto'
    decides that when the layer's call plan is made, from the change count of the layer's last frame (CBConv2d._window_fold)."""
    for seq in _sequentials(rootModule):
        kids = list(seq.children())
        for prod, pool, cons in zip(kids[:-2], kids[1:-1], kids[2:]):
            if type(prod) == CBConv2d and type(pool) == CBPoolMax2d and type(cons) == CBConv2d:
                if (enabled and getattr(pool, 'lazy', False) and cons.feedbackLoop and prod.feedbackLoop and
                        not prod.__dict__.get('_geom') and not cons.__dict__.get('_geom')):
                    prod.__dict__['_fusedNext'] = (pool, cons)      # (plain references, not children)
                    prod.__dict__['_winFold'] = windowOrder
                else:
                    prod.__dict__.pop('_fusedNext', None)
        # round 6: a CBConv2d directly behind another one (fp16 layers on the split-state machinery, the consumer in copy
        # mode -- what convert() makes): the producer's contraction launch compares the values it just wrote with the
        # consumer's state, refreshes that state and ORs the consumer's change mask; the consumer runs its contraction
        # alone.  Whether a given frame may do so is decided per frame (CBConv2d._fill_consumers / _detected_upstream).
        for prod, cons in zip(kids[:-1], kids[1:]):
            if type(prod) == CBConv2d and type(cons) == CBConv2d:
                linkConsumers(prod, [cons] if enabled else [])
    return rootModule


def linkConsumers(producer, consumers):
    """Name the CBConv2d layers that consume `producer`'s output tensor directly (same resolution) where the module tree
    does not say so -- e.g. the first layers of the two branches of an OpenPose stage, both fed the feature extractor's
    last output (poseDetection/openPose/PoseModel.py:122-137).  Their change detection then rides in the producer's
    launch whenever that is exact (see fuseDetectionIntoProducer); at most two consumers per producer are folded.  An
    empty list removes the link.  Execution-level only: results do not change."""
    # (a general-geometry layer neither folds a consumer's detection nor has its own folded)
    consumers = [c for c in consumers if type(c) == CBConv2d and not c.__dict__.get('_geom')]
    if consumers and not producer.__dict__.get('_geom'):
        producer.__dict__['_fusedConsumers'] = list(consumers)      # (plain references, not children)
    else:
        producer.__dict__.pop('_fusedConsumers', None)
    return producer


# The module types of chain.PRODUCERS that keep state.  The wrappers (CBResidual, CBGated, CBSqueezeExcite) define no
# getStateTensors: their children are reached as modules of the network.
_STATEFUL = tuple(t for t in chain.module_types() if hasattr(t, 'getStateTensors'))


def _stateful(net):
    return [m for m in net.modules() if type(m) in _STATEFUL]


def clearMemory(net):
    """Drop the frame-to-frame state of every change-based module (reference: __init__.py:79-82)."""
    for m in _stateful(net):
        m.clearMemory()


def getStateTensors(net):
    """Flat list of the state tensors of every change-based module (reference: __init__.py:84-89)."""
    return [t for m in _stateful(net) for t in m.getStateTensors()]


def convert(m, ignoreList=[], threshold=1e-1, generalGeometry=False, depthwise=False, grouped=False):
    """nn.Sequential in -> nn.Sequential out with every Conv2d replaced by a CBConv2d sharing its
    weights, ReLUs merged, Dropout removed (reference: __init__.py:91-94).  generalGeometry=True: strided, dilated,
    freely padded and bias-free convolutions are converted too (the default stops at them with an AssertionError, as
    the reference does).  depthwise=True: depthwise convolutions (groups == in_channels > 1) become CBDepthwiseConv2d
    modules, an nn.ReLU or nn.ReLU6 behind one is absorbed.  grouped=True: convolutions with groups > 1 (depthwise ones
    only where depthwise=True does not take them) become CBGroupedConv2d modules, an nn.ReLU behind one is absorbed.  With
    the defaults grouped convolutions are refused as before."""
    converted, _ = convertRecur(m, ignoreList=ignoreList, threshold=threshold, generalGeometry=generalGeometry,
                                depthwise=depthwise, grouped=grouped)
    return mergeReLURecur(converted)


def setSyncIndexes(net, enabled):
    """Switch every CBConv2d of `net` between the sync-free frame pipeline (False, default) and the
    reference-structured op sequence that blocks on the change count (True)."""
    for m in net.modules():
        if type(m) == CBConv2d:
            m.syncIndexes = bool(enabled)
    return net


def fuseTail1x1(rootModule, enabled=True):
    """Execution-level fusion (results within the fp32 bar of the unfused network): inside every
    nn.Sequential the run  CBConv2d -> nn.Conv2d 1x1 -> nn.ReLU -> nn.Conv2d 1x1  (the dense tail that
    sceneLabeling/modelLoader.py:45-47 keeps for experiments 2-7) becomes  CBConv2d -> CBTail1x1 : the
    two 1x1 layers are evaluated in ONE launch, only at the pixels of the CBConv2d's change list (its
    propChangeIndexes is switched on; a fine-grained head hands on the output pixels its frame touched) -- a
    1x1 layer's output changes only where its input did.  The new
    module takes the first 1x1 layer's name and shares the parameters of both.  enabled=False is a no-op.
    Returns rootModule."""
    if not enabled:
        return rootModule

    def is1x1(m):
        return type(m) is nn.Conv2d and CBTail1x1.accepts(m)

    for seq in _sequentials(rootModule):
        names = list(seq._modules.keys())
        kids = [seq._modules[n] for n in names]
        for i in range(len(kids) - 3):
            head, a, act, b = kids[i:i + 4]
            if (type(head) is CBConv2d and is1x1(a) and type(act) is nn.ReLU and
                    is1x1(b) and a.out_channels == b.in_channels and
                    CBTail1x1.supported(a.in_channels, a.out_channels, b.out_channels) and
                    a.weight.dtype == torch.float32):
                _log('fusing the 1x1 tail behind %s' % names[i])
                head.propChangeIndexes = True
                tail = CBTail1x1(a, b, relu=True)
                seq._modules[names[i + 1]] = tail
                head.__dict__['_fusedTail'] = tail      # (a plain reference, not a child: see CBConv2d._folded_tail)
                del seq._modules[names[i + 2]]
                del seq._modules[names[i + 3]]
                break
    return rootModule


_THRESHOLD_CEILING = 1e30   # a tolerance that is never exceeded must not loop forever (the reference would)


def tuneThresholdParameters(vidSeqReader, evalSequences, numFramesPerSeq, targetGenerator,
                            preprocessor, modelBaseline, modelTest, evaluator, cbModuleList,
                            lossToleranceList, initThreshold=1e-2, thresholdIncrFactor=1.2):
    """Greedy front-to-back per-layer threshold search with the reference's callback protocol
    (reference: __init__.py:98-149).  Modules are visited in list order; a module's threshold climbs
    from initThreshold by thresholdIncrFactor per step for as long as the summed evaluator loss over
    evalSequences stays within the module's tolerance of the loss measured before the module was
    touched, and the last level that did is kept (the reference's "one step back").  As there,
    initThreshold itself is never evaluated.  The loss the next module is judged against is re-measured
    with the kept level."""
    tolerances = lossToleranceList if type(lossToleranceList) is list \
        else [lossToleranceList] * len(cbModuleList)
    assert len(cbModuleList) == len(tolerances)
    device = next(modelTest.parameters()).device

    def sequenceLoss(seqName):
        frames, target = vidSeqReader.getDataFrames(seqName=seqName, numFrames=numFramesPerSeq)
        if target is None:
            target = targetGenerator(frames[-1])
        with torch.no_grad():
            for frame in frames:
                prediction = modelTest(preprocessor(frame).to(device))
        return evaluator(prediction, target)

    def measure():
        clearMemory(modelTest)
        return sum(sequenceLoss(name) for name in evalSequences)

    anchor = measure()
    for pos, (module, tolerance) in enumerate(zip(cbModuleList, tolerances)):
        _log('adjusting threshold for module %d of %d' % (pos + 1, len(cbModuleList)))
        kept = initThreshold
        while kept * thresholdIncrFactor < _THRESHOLD_CEILING:
            module.threshold = kept * thresholdIncrFactor
            loss = measure()
            _log('. (%f < %f + %f)' % (loss, anchor, tolerance))
            if loss - anchor > tolerance:
                break
            kept = module.threshold
        module.threshold = kept
        anchor = measure()


# the CB names are the rows of chain.PRODUCERS; the functions and the other classes are written out
__all__ = [row[0] for row in chain.PRODUCERS] + [
    'foldBatchNorm', 'insertCBUpsampling', 'insertCBTransposedConv', 'linkDepthwise', 'insertCBPointwise',
    'linkGrouped', 'insertCBRearrange', 'insertCBChannelOps', 'insertCBResize', 'insertCBPadding', 'splitConvPadding',
    'insertCBGating', 'insertCBSqueezeExcite', 'insertCBGroupNorm', 'ChangeIndexes', 'ChannelConcat', 'FramePipeline',
    'SequenceBatch', 'BranchGroup', 'FrameProgram', 'convert', 'convertRecur', 'subsitute', 'mergeReLURecur',
    'propChangeIndexesOf1x1', 'insertCBPooling', 'fusePoolingIntoDetection', 'fuseDetectionIntoProducer',
    'linkConsumers', 'fuseTail1x1', 'clearMemory', 'getStateTensors', 'setSyncIndexes', 'tuneThresholdParameters']
