"""Every accepted (pass, producer type) pair of chain.PRODUCERS as a network that runs (tests/test_gpu_chain.py on the
device, tests/test_host_chain.py for the table itself).  Importable without a GPU.

A case is  stem -> producer -> op  on a 12 x 70 map -- W crosses the 64-bit mask word, a x2 producer reaches 140 and the
second word boundary, a /2 producer 35 with padding bits in its only word, H is a multiple of nothing:
  stem      a converted 3x3 nn.Conv2d(3, C, padding=1), threshold 0.05: the source of the changes.  It hands its list on
            to a producer that has no detection of its own; a producer that has one is fed the bare tensor;
  producer  one constructor per row of PRODUCERS (both pool kinds of CBPoolMax2d), 8 channels out;
  op        the torch module the pass converts behind the producer.
BEHIND is written by hand: the host test compares it with the table of the package, so a new row there without a case
here fails by name.  The pass wires the nn.Sequential (stem, producer, op); Chain then calls the three children by hand,
because a producer of two operands cannot stand in nn.Sequential.forward: every flag is the one the pass set."""
import collections

import numpy as np
import torch
import torch.nn as nn

H, W = 12, 70
TH = 0.05
C_OUT = 8      # channels out of every producer

Case = collections.namedtuple('Case', 'passName producer op')


def case_id(c):
    return '%s/%s/%s' % c


def producer_type(c):
    """The module type's name of a case's producer ('CBPoolMax2d 3x3' -> 'CBPoolMax2d')."""
    return c.producer.split()[0]


# ------------------------------------------------------------------------------------------------ footprints
def spread(mask, out_hw, step, first, r):
    """The output pixels (bool [Ho, Wo]) that read a True pixel of `mask`, for an operator whose output pixel o reads,
    per axis, the input pixels within r of first + o * step (step, first: a number or one per axis)."""
    maps = []
    for axis, (n_out, n_in) in enumerate(zip(out_hw, mask.shape)):
        st, fi = (v[axis] if isinstance(v, tuple) else v for v in (step, first))
        centre = fi + np.arange(n_out)[:, None] * st
        maps.append(np.abs(centre - np.arange(n_in)[None, :]) <= r + 1e-9)
    return (maps[0].astype(np.int64) @ mask.astype(np.int64) @ maps[1].astype(np.int64).T) > 0


def same(r):
    """A stride-1 operator that keeps the map and reads a (2r+1) x (2r+1) window."""
    return lambda m: spread(m, m.shape, 1.0, 0.0, r)


def twice(r=0.25):
    """x2 per axis: output pixel o reads input pixel o // 2 (nearest, a 2x2 / stride-2 transposed convolution, a pixel
    shuffle)."""
    return lambda m: spread(m, (2 * m.shape[0], 2 * m.shape[1]), 0.5, -0.25, r)


def pool(k, s, p):
    def reach(m):
        out = tuple((n + 2 * p - k) // s + 1 for n in m.shape)
        return spread(m, out, float(s), (k - 1) / 2.0 - p, (k - 1) / 2.0)
    return reach


def resize(size, r=1.0):
    """A resize to `size` with align_corners=False: 2 x 2 taps (bilinear) around the source coordinate."""
    def reach(m):
        step = tuple(n / float(o) for n, o in zip(m.shape, size))
        return spread(m, size, step, tuple(0.5 * s - 0.5 for s in step), r)
    return reach


def reflect(left, right, top, bottom):
    return lambda m: np.pad(m, ((top, bottom), (left, right)), mode='reflect')


# ------------------------------------------------------------------------------------------------ the producers
def _conv(pkg, put, cin, cout, **kw):
    """A converted 3x3 convolution with padding 1, threshold TH (copyInput as the constructor leaves it: on)."""
    return pkg.convert(nn.Sequential(put(nn.Conv2d(cin, cout, 3, padding=1, **kw))), threshold=TH,
                       depthwise=True, grouped=True)[0]


def _body(pkg, put):
    """Two converted 3x3 layers, the body of a CBResidual or a CBGated."""
    return pkg.convert(nn.Sequential(put(nn.Conv2d(C_OUT, C_OUT, 3, padding=1)),
                                     put(nn.Conv2d(C_OUT, C_OUT, 3, padding=1))), threshold=TH)


Producer = collections.namedtuple('Producer', 'make cin fed two hands reach')
# make(pkg, put): the module; cin: the channels the stem gives it; fed: it has no detection of its own and takes the
# stem's change list; two: forward(a, b), b from a second stem; hands: what it hands on with propChangeIndexes -- 'mask'
# (a MaskChangeIndexes whose list is not made), 'made' (one whose list the frame's kernel made), 'list' (a ChangeIndexes)
# -- a pair: in float32, in float16 (hands_of) --; reach: the footprint of its input's changes on its output map
PRODUCERS = collections.OrderedDict([
    # (fp32 with exactF32 runs the row kernel, which leaves its mask; fp16 the self-compacting list kernel)
    ('CBConv2d', Producer(lambda pkg, put: _conv(pkg, put, C_OUT, C_OUT), 8, False, False, ('mask', 'made'), same(1))),
    ('CBPoolMax2d 2x2', Producer(lambda pkg, put: pkg.CBPoolMax2d(nn.MaxPool2d(2)), 8, True, False, 'list',
                                 pool(2, 2, 0))),
    ('CBPoolMax2d 3x3', Producer(lambda pkg, put: pkg.CBPoolMax2d(nn.MaxPool2d(3, 2, 1), generalGeometry=True), 8, True,
                                 False, 'mask', pool(3, 2, 1))),
    ('CBPoolAvg2d', Producer(lambda pkg, put: pkg.CBPoolAvg2d(nn.AvgPool2d(2)), 8, True, False, 'mask', pool(2, 2, 0))),
    ('CBAdd2d', Producer(lambda pkg, put: pkg.CBAdd2d(), 8, True, True, 'mask', same(0))),
    ('CBResidual', Producer(lambda pkg, put: pkg.CBResidual(_body(pkg, put)), 8, True, False, 'mask', same(2))),
    ('CBUpsample2d', Producer(lambda pkg, put: pkg.CBUpsample2d(nn.Upsample(scale_factor=2)), 8, True, False, 'mask',
                              twice())),
    ('CBConvTranspose2d', Producer(lambda pkg, put: pkg.CBConvTranspose2d(
        put(nn.ConvTranspose2d(C_OUT, C_OUT, 2, stride=2)), TH), 8, False, False, 'mask', twice())),
    ('CBDepthwiseConv2d', Producer(lambda pkg, put: _conv(pkg, put, C_OUT, C_OUT, groups=C_OUT), 8, False, False, 'mask',
                                   same(1))),
    ('CBPointwise2d', Producer(lambda pkg, put: pkg.CBPointwise2d(nn.Tanh()), 8, True, False, 'mask', same(0))),
    ('CBPixelShuffle2d', Producer(lambda pkg, put: pkg.CBPixelShuffle2d(nn.PixelShuffle(2)), 32, True, False, 'mask',
                                  twice())),
    ('CBChannelShuffle2d', Producer(lambda pkg, put: pkg.CBChannelShuffle2d(nn.ChannelShuffle(2)), 8, True, False,
                                    'mask', same(0))),
    ('CBResize2d', Producer(lambda pkg, put: pkg.CBResize2d(size=(9, 53), mode='bilinear'), 8, True, False, 'mask',
                            resize((9, 53)))),
    ('CBPad2d', Producer(lambda pkg, put: pkg.CBPad2d(nn.ReflectionPad2d((1, 2, 1, 0))), 8, True, False, 'mask',
                         reflect(1, 2, 1, 0))),
    ('CBBinary2d', Producer(lambda pkg, put: pkg.CBBinary2d('maximum'), 8, True, True, 'mask', same(0))),
    ('CBGLU2d', Producer(lambda pkg, put: pkg.CBGLU2d(nn.GLU(1)), 16, True, False, 'mask', same(0))),
    ('CBGated', Producer(lambda pkg, put: pkg.CBGated(_body(pkg, put)), 8, True, False, 'mask', same(2))),
    ('CBGroupedConv2d', Producer(lambda pkg, put: _conv(pkg, put, C_OUT, C_OUT, groups=2), 8, False, False, 'made',
                                 same(1))),
    ('CBChannelReduce2d', Producer(lambda pkg, put: pkg.CBChannelReduce2d(nn.Softmax2d()), 8, True, False, 'mask',
                                   same(0))),
])


def hands_of(producer, dtype):
    """The form in which the producer of that name hands its changes on in `dtype`."""
    hands = PRODUCERS[producer].hands
    return hands[dtype == torch.float16] if isinstance(hands, tuple) else hands


# ------------------------------------------------------------------------------------------------ the passes
UP_SIZE = (17, 91)      # of the resize op: within a ratio of 8 of every producer's map, across the word boundary

Op = collections.namedtuple('Op', 'make becomes reach')
# make(pkg, put): what stands behind the producer when the pass runs; becomes: the type's name the pass leaves there
OPS = collections.OrderedDict([
    ('PixelShuffle(2)', Op(lambda pkg, put: nn.PixelShuffle(2), 'CBPixelShuffle2d', twice())),
    ('Softmax2d', Op(lambda pkg, put: nn.Softmax2d(), 'CBChannelReduce2d', same(0))),
    ('Upsample(size, bilinear)', Op(lambda pkg, put: nn.Upsample(size=UP_SIZE, mode='bilinear'), 'CBResize2d',
                                    resize(UP_SIZE))),
    ('ReflectionPad2d(1)', Op(lambda pkg, put: nn.ReflectionPad2d(1), 'CBPad2d', reflect(1, 1, 1, 1))),
    ('GLU(1)', Op(lambda pkg, put: nn.GLU(1), 'CBGLU2d', same(0))),
    ('Upsample(x2)', Op(lambda pkg, put: nn.Upsample(scale_factor=2), 'CBUpsample2d', twice())),
    ('ConvTranspose2d(2, s2)', Op(lambda pkg, put: put(nn.ConvTranspose2d(C_OUT, C_OUT, 2, stride=2)),
                                  'CBConvTranspose2d', twice())),
    ('Tanh', Op(lambda pkg, put: nn.Tanh(), 'CBPointwise2d', same(0))),
    ('depthwise 3x3', Op(lambda pkg, put: _conv(pkg, put, C_OUT, C_OUT, groups=C_OUT), 'CBDepthwiseConv2d', same(1))),
    ('MaxPool2d(2)', Op(lambda pkg, put: nn.MaxPool2d(2), 'CBPoolMax2d', pool(2, 2, 0))),
    ('MaxPool2d(3, 2, 1)', Op(lambda pkg, put: nn.MaxPool2d(3, 2, 1), 'CBPoolMax2d', pool(3, 2, 1))),
    ('AvgPool2d(2)', Op(lambda pkg, put: nn.AvgPool2d(2), 'CBPoolAvg2d', pool(2, 2, 0))),
])

Pass = collections.namedtuple('Pass', 'run takesClone ops')
GENERAL_POOLS = 'insertCBPooling(generalGeometry=True)'
PASSES = collections.OrderedDict([
    ('linkDepthwise', Pass(lambda pkg, net, **kw: pkg.linkDepthwise(net), False, ('depthwise 3x3',))),
    ('insertCBPointwise', Pass(lambda pkg, net, **kw: pkg.insertCBPointwise(net), False, ('Tanh',))),
    ('insertCBTransposedConv', Pass(lambda pkg, net, **kw: pkg.insertCBTransposedConv(net, threshold=TH, **kw), True,
                                    ('ConvTranspose2d(2, s2)',))),
    ('insertCBUpsampling', Pass(lambda pkg, net, **kw: pkg.insertCBUpsampling(net, **kw), True, ('Upsample(x2)',))),
    ('insertCBRearrange', Pass(lambda pkg, net, **kw: pkg.insertCBRearrange(net, **kw), True, ('PixelShuffle(2)',))),
    ('insertCBChannelOps', Pass(lambda pkg, net, **kw: pkg.insertCBChannelOps(net), False, ('Softmax2d',))),
    ('insertCBPadding', Pass(lambda pkg, net, **kw: pkg.insertCBPadding(net, **kw), True, ('ReflectionPad2d(1)',))),
    ('insertCBGating', Pass(lambda pkg, net, **kw: pkg.insertCBGating(net, **kw), True, ('GLU(1)',))),
    ('insertCBResize', Pass(lambda pkg, net, **kw: pkg.insertCBResize(net, **kw), True, ('Upsample(size, bilinear)',))),
    ('insertCBPooling', Pass(lambda pkg, net, **kw: pkg.insertCBPooling(net, **kw), True, ('MaxPool2d(2)',))),
    (GENERAL_POOLS, Pass(lambda pkg, net, **kw: pkg.insertCBPooling(net, generalGeometry=True, **kw), True,
                         ('MaxPool2d(3, 2, 1)', 'AvgPool2d(2)'))),
])
# (the only pass that hands nothing on: its operator runs its own detection)
OWN_DETECTION = ('insertCBTransposedConv',)

_COMMON = ('CBConv2d', 'CBPoolMax2d 2x2', 'CBPoolMax2d 3x3', 'CBPoolAvg2d', 'CBAdd2d', 'CBResidual', 'CBUpsample2d',
           'CBDepthwiseConv2d', 'CBPointwise2d', 'CBPixelShuffle2d', 'CBChannelShuffle2d', 'CBResize2d', 'CBPad2d',
           'CBBinary2d', 'CBGLU2d', 'CBGated')
# pass -> the producers a case runs it behind: every type the pass accepts, both pool kinds of CBPoolMax2d
BEHIND = collections.OrderedDict([
    ('linkDepthwise', _COMMON + ('CBConvTranspose2d',)),
    ('insertCBPointwise', _COMMON + ('CBConvTranspose2d',)),
    ('insertCBTransposedConv', _COMMON + ('CBConvTranspose2d',)),
    ('insertCBUpsampling', _COMMON),
    ('insertCBRearrange', _COMMON + ('CBConvTranspose2d', 'CBGroupedConv2d')),
    ('insertCBChannelOps', _COMMON + ('CBConvTranspose2d', 'CBGroupedConv2d', 'CBChannelReduce2d')),
    ('insertCBPadding', _COMMON + ('CBConvTranspose2d', 'CBGroupedConv2d', 'CBChannelReduce2d')),
    ('insertCBGating', _COMMON + ('CBConvTranspose2d', 'CBGroupedConv2d', 'CBChannelReduce2d')),
    ('insertCBResize', _COMMON + ('CBGroupedConv2d', 'CBChannelReduce2d')),
    ('insertCBPooling', ('CBConv2d',)),
    (GENERAL_POOLS, ('CBConv2d', 'CBPointwise2d', 'CBPad2d')),
])

CASES = [Case(p, producer, op) for p, behind in BEHIND.items() for producer in behind for op in PASSES[p].ops]


def pairs():
    """The (pass, producer type) pairs the cases cover."""
    return set((c.passName, producer_type(c)) for c in CASES)


# ------------------------------------------------------------------------------------------------ the networks
class Chain(nn.Module):
    """stem -> producer -> op: the children of `seq`, which the pass wired, called by hand; a producer of two operands
    takes the result of a second stem as its operand b."""

    def __init__(self, seq, second=None):
        super(Chain, self).__init__()
        self.seq, self.second = seq, second

    def forward(self, frame):
        stem, producer, op = self.seq
        x = stem(frame)
        x = producer(x, self.second(frame)) if self.second is not None else producer(x)
        return op(x)


def hand_on_target(producer):
    """The module of a producer that carries propChangeIndexes and cloneOutput (chain.hand_on_changes)."""
    return getattr(producer, {'CBResidual': 'add', 'CBGated': 'mul'}.get(type(producer).__name__, ''), producer)


def build(pkg, case, dtype=torch.float32, device='cpu', cloneOutput=True):
    """The case's network, wired by its pass: a Chain whose .seq is (stem, producer, the pass's operator).  cloneOutput
    goes to the pass where it takes one, else to the new module, and to the producer in either case; fp32 CBConv2d
    layers run the exact f32 arithmetic."""
    torch.manual_seed(65)

    def put(m):
        return m.eval().to(device=device, dtype=dtype)
    row, run = PRODUCERS[case.producer], PASSES[case.passName]
    stem = _conv(pkg, put, 3, row.cin)
    second = _conv(pkg, put, 3, row.cin) if row.two else None
    for m in (stem, second):
        if m is not None and row.fed:
            m.propChangeIndexes = True
    seq = nn.Sequential(stem, row.make(pkg, put), OPS[case.op].make(pkg, put))
    got = run.run(pkg, seq, **(dict(cloneOutput=cloneOutput) if run.takesClone else {}))
    assert got is seq and len(seq) == 3
    if not run.takesClone:
        seq[2].cloneOutput = cloneOutput
    target = hand_on_target(seq[1])
    if hasattr(target, 'cloneOutput'):
        target.cloneOutput = cloneOutput
    net = Chain(seq, second).to(device)
    if dtype == torch.float32:
        for m in net.modules():
            if type(m) is pkg.CBConv2d:
                m.exactF32 = True
    return net


# ------------------------------------------------------------------------------------------------ the frames
IDLE = 4                        # the frame that is bit-identical to the one before
LOCAL = (1, 2, 3, 5)            # the frames that change one or two pixels
RECORD_AFTER = 3                # the recording test runs this many frames eagerly


def changed():
    """Per frame, the bool [H, W] map of the input pixels that differ from the frame before (frame 0: all)."""
    rng = np.random.default_rng(65)
    maps = [np.zeros((H, W), dtype=bool) for _ in range(8)]
    maps[0][:] = True
    maps[1][6, 35] = True
    maps[2][5, 63] = maps[2][5, 64] = True      # (either side of the word boundary)
    maps[3][H - 1, W - 1] = True
    maps[5][0, 0] = True                        # (the first frame behind the idle one)
    for _ in range(2):                          # (two 5x9 blocks, cut off at the border)
        y0, x0 = int(rng.integers(0, H)), int(rng.integers(0, W))
        maps[6][y0:y0 + 5, x0:x0 + 9] = True
    maps[7][:] = True
    return maps


def frames(dtype):
    """Eight [1, 3, H, W] frames on the CPU.  The values are multiples of 1/256 in [0, 0.4) or [0.5, 0.9), exact in
    float16; a changed pixel moves by exactly 0.5 in every channel, into the other interval."""
    rng = np.random.default_rng(66)
    k = rng.integers(0, 204, (1, 3, H, W))
    base = np.where(k < 102, k, k + 26) / 256.0
    out = []
    for t, sel in enumerate(changed()):
        if t:
            base = base.copy()
            v = base[:, :, sel]
            base[:, :, sel] = np.where(v < 0.45, v + 0.5, v - 0.5)
        out.append(torch.from_numpy(base.astype(np.float32)).to(dtype))
    return out


def footprint(case, sel):
    """An upper bound of the op's listed pixels (bool, on its output map) when the input pixels `sel` changed: the
    stem's 3x3, then the producer's reach, then the op's."""
    return OPS[case.op].reach(PRODUCERS[case.producer].reach(same(1)(sel)))
