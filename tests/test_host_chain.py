"""CPU-only tests of what the change-based operators behind a producer share on the host (cbinfer_amd/chain.py,
DESIGN.md 5.17): the conversion passes against a table of small networks whose wiring was recorded before the walk was
written once, and the helpers of the frame skeleton -- the keyed workspace cache, the state step, the check of an operand
map, the expansion of a form and the consumer rule.  No kernel is launched here."""
import pickle

import pytest
import torch
import torch.nn as nn

import chain_cases as cc
from optest import pkg      # noqa: F401  (fixtures)


@pytest.fixture(scope="module")
def chain():
    from cbinfer_amd import chain
    return chain


@pytest.fixture(scope="module")
def Err():
    from cbinfer_amd import _lib
    return _lib.CBinferError


# ------------------------------------------------------------------------------------------------ the networks
def conv(k=3, feedback=False, **kw):
    """A converted k x k convolution whose copyInput is OFF (the constructor's default is on), so that a pass that
    switches it on shows."""
    import pycbinfer
    m = pycbinfer.convert(nn.Sequential(nn.Conv2d(4, 4, k, padding=k // 2, **kw)).eval(), threshold=0.05,
                          generalGeometry=True, depthwise=True, grouped=True)[0]
    m.copyInput, m.feedbackLoop = False, feedback
    return m


def _producers(pkg):
    """name -> constructor of every kind of module a pass may find in front of its operator: the sixteen types every chain
    pass but the upsamplings accepts, the two further ones most passes add, a pool of each kind, and a dense module."""
    return {
        'CBConv2d': conv,
        'CBPoolMax2d 2x2': lambda: pkg.CBPoolMax2d(nn.MaxPool2d(2)),
        'CBPoolMax2d 3x3': lambda: pkg.CBPoolMax2d(nn.MaxPool2d(3, 2, 1), generalGeometry=True),
        'CBPoolAvg2d': lambda: pkg.CBPoolAvg2d(nn.AvgPool2d(2)),
        'CBAdd2d': lambda: pkg.CBAdd2d(),
        'CBResidual': lambda: pkg.CBResidual(nn.Sequential(conv(), conv())),
        'CBUpsample2d': lambda: pkg.CBUpsample2d(nn.Upsample(scale_factor=2)),
        'CBConvTranspose2d': lambda: pkg.CBConvTranspose2d(nn.ConvTranspose2d(4, 4, 2, stride=2), 0.05),
        'CBDepthwiseConv2d': lambda: conv(groups=4),
        'CBPointwise2d': lambda: pkg.CBPointwise2d(nn.Tanh()),
        'CBPixelShuffle2d': lambda: pkg.CBPixelShuffle2d(nn.PixelShuffle(2)),
        'CBChannelShuffle2d': lambda: pkg.CBChannelShuffle2d(nn.ChannelShuffle(2)),
        'CBResize2d': lambda: pkg.CBResize2d(size=(9, 11)),
        'CBPad2d': lambda: pkg.CBPad2d(nn.ZeroPad2d(1)),
        'CBBinary2d': lambda: pkg.CBBinary2d('mul', other=2.0),
        'CBGLU2d': lambda: pkg.CBGLU2d(nn.GLU(1)),
        'CBGated': lambda: pkg.CBGated(nn.Sequential(conv(), conv())),
        'CBGroupedConv2d': lambda: conv(groups=2),
        'CBChannelReduce2d': lambda: pkg.CBChannelReduce2d(nn.Softmax2d()),
        'dense': lambda: nn.Identity(),
    }


class MySequential(nn.Sequential):
    pass


def _passes(pkg):
    """name -> (the pass, takes cloneOutput?, its operator, an operator it must leave alone: beyond the library's limits
    or not its own)."""
    return {
        'insertCBRearrange': (pkg.insertCBRearrange, True, lambda: nn.PixelShuffle(2), lambda: nn.PixelShuffle(9)),
        'insertCBChannelOps': (pkg.insertCBChannelOps, False, lambda: nn.Softmax2d(), lambda: nn.Softmax(dim=2)),
        'insertCBResize': (pkg.insertCBResize, True, lambda: nn.Upsample(size=(9, 11), mode='bilinear'),
                           lambda: nn.Upsample(scale_factor=16)),
        'insertCBPadding': (pkg.insertCBPadding, True, lambda: nn.ReflectionPad2d(1), lambda: nn.ZeroPad2d(65)),
        'insertCBGating': (pkg.insertCBGating, True, lambda: nn.GLU(1), lambda: nn.GLU(-1)),
        'insertCBUpsampling': (pkg.insertCBUpsampling, True, lambda: nn.Upsample(scale_factor=2),
                               lambda: nn.Upsample(scale_factor=16)),
        'insertCBTransposedConv': (lambda net, **kw: pkg.insertCBTransposedConv(net, threshold=0.05, **kw), True,
                                   lambda: nn.ConvTranspose2d(4, 4, 2, stride=2), lambda: nn.ConvTranspose2d(4, 4, 9)),
        # the passes that do not go through the walk, pinned all the same
        'insertCBPointwise': (pkg.insertCBPointwise, False, lambda: nn.Tanh(), lambda: nn.GELU()),
        'linkDepthwise': (pkg.linkDepthwise, False, lambda: conv(groups=4), lambda: conv(groups=4, dilation=2)),
        'linkGrouped': (pkg.linkGrouped, False, lambda: conv(groups=2), lambda: nn.Identity()),
    }


def networks(pkg, op, beyond):
    """scenario -> constructor of the network, for a pass whose operator `op()` makes and which leaves `beyond()`."""
    S = nn.Sequential
    nets = {'behind ' + kind: (lambda make=make: S(make(), op(), conv())) for kind, make in _producers(pkg).items()}
    nets.update({
        'at position 0': lambda: S(op(), conv()),
        'the last child': lambda: S(conv(), op()),
        'in front of a 1x1': lambda: S(conv(), op(), conv(1)),
        'in front of a strided 1x1': lambda: S(conv(), op(), conv(1, stride=2)),
        'in front of a 3x3 in feedback mode': lambda: S(conv(), op(), conv(feedback=True)),
        'in front of a 1x1 in feedback mode': lambda: S(conv(), op(), conv(1, feedback=True)),
        'in front of a dense module': lambda: S(conv(), op(), nn.Identity()),
        'in front of a grouped convolution': lambda: S(conv(), op(), conv(groups=2)),
        'two in a row': lambda: S(conv(), op(), op(), conv(1)),
        'nested': lambda: S(nn.Identity(), S(conv(), op(), conv(1)), op(), S(S(conv(), op()))),
        'in a subclass of nn.Sequential': lambda: S(MySequential(conv(), op(), conv())),
        'beyond the limits': lambda: S(conv(), beyond(), conv()),
        'a ReLU behind it': lambda: S(conv(), op(), nn.ReLU(), conv()),
        'a ReLU behind it, twice': lambda: S(conv(), op(), nn.ReLU(), op(), nn.ReLU(), conv(1)),
        'a batch norm and an activation behind it': lambda: S(conv(), nn.BatchNorm2d(4).eval(), op(), conv(1)),
    })
    return nets


FLAGS = (('p', 'propChangeIndexes'), ('c', 'cloneOutput'), ('i', 'copyInput'), ('d', 'downsampleIndexes'))


def wiring(net):
    """One line per network: every module's name and type, and the flags it has, the `.add` / `.mul` of the wiring
    modules and the children of nested containers included."""
    said = []
    for name, m in net.named_modules():
        if m is net:
            continue
        flags = ''.join('%s%d' % (short, bool(getattr(m, attr))) for short, attr in FLAGS if hasattr(m, attr))
        said.append('%s:%s%s' % (name, type(m).__name__, '/' + flags if flags else ''))
    return ' '.join(said)


def record(pkg):
    """{pass: {scenario: (wiring with the pass's defaults, wiring with cloneOutput=False or None)}}"""
    table = {}
    for passName, (run, takesClone, op, beyond) in _passes(pkg).items():
        rows = table[passName] = {}
        for scenario, make in networks(pkg, op, beyond).items():
            torch.manual_seed(0)
            net = make()
            assert run(net) is net
            other = None
            if takesClone:
                other = make()
                run(other, cloneOutput=False)
            rows[scenario] = (wiring(net), wiring(other) if other is not None else None)
    return table


# ------------------------------------------------------------------------------------------------ the passes
def test_every_pass_wires_every_network_as_recorded(pkg):
    """WIRING (at the end of this file) was written by record() before the passes shared one walk: child names, types
    and every flag of every module must come out exactly as they did, with the defaults and with cloneOutput=False."""
    got = record(pkg)
    assert sorted(got) == sorted(WIRING)
    for passName, rows in got.items():
        want = WIRING[passName]
        assert sorted(rows) == sorted(want), passName
        for scenario, pair in rows.items():
            assert pair == want[scenario], (passName, scenario)


def test_the_table_shows_what_it_is_there_to_show(pkg):
    """The recorded table itself: every pass converts behind what it accepts and not behind the rest, and the flags the
    consumer rule sets are visible in it."""
    W = WIRING
    assert len(W) == 10 and all(len(rows) == 35 for rows in W.values())
    for passName in ('insertCBRearrange', 'insertCBChannelOps', 'insertCBResize', 'insertCBPadding', 'insertCBGating'):
        rows = W[passName]
        new = rows['behind CBConv2d'][0].split()[1].split(':')[1].split('/')[0]
        assert new.startswith('CB')
        assert rows['in front of a 1x1'][0].split()[1:] == ['1:%s/p1c1' % new, '2:CBConv2d/p0i0']
        assert rows['behind CBConv2d'][0].split()[2] == '2:CBConv2d/p0i1'
        assert rows['in front of a 3x3 in feedback mode'][0].split()[1:] == ['1:%s/p0c1' % new, '2:CBConv2d/p0i0']
        assert new not in rows['behind dense'][0] and new not in rows['at position 0'][0]
        assert new not in rows['beyond the limits'][0] and new not in rows['in a subclass of nn.Sequential'][0]
        assert rows['behind CBPoolMax2d 2x2'][0].startswith('0:CBPoolMax2d/p1c1d1 ')
        assert rows['behind CBPoolMax2d 3x3'][0].startswith('0:CBPoolMax2d/p1c1d0 ')
        assert ' 0.add:CBAdd2d/p1c1 ' in rows['behind CBResidual'][0]
        assert ' 0.mul:CBBinary2d/p1c1 ' in rows['behind CBGated'][0]
        if passName != 'insertCBChannelOps':
            assert rows['in front of a 1x1'][1].split()[1] == '1:%s/p1c0' % new
    # insertCBUpsampling hands nothing on at the new module: a 1x1 consumer copies its input like any other
    assert W['insertCBUpsampling']['in front of a 1x1'][0].split()[1:] == ['1:CBUpsample2d/p0c1', '2:CBConv2d/p0i1']
    assert 'CBUpsample2d' not in W['insertCBUpsampling']['behind CBConvTranspose2d'][0]
    assert 'CBUpsample2d' not in W['insertCBUpsampling']['behind CBGroupedConv2d'][0]
    assert 'CBResize2d' in W['insertCBResize']['behind CBGroupedConv2d'][0]
    assert 'CBPixelShuffle2d' not in W['insertCBRearrange']['behind CBChannelReduce2d'][0]
    # insertCBTransposedConv switches nothing on at the producer and absorbs the ReLU
    assert W['insertCBTransposedConv']['a ReLU behind it'][0] == (
        '0:CBConv2d/p0i0 1:CBConvTranspose2d/p0c1i1 3:CBConv2d/p0i1')


def test_channel_ops_hands_a_refusing_constructor_on(pkg, Err):
    """insertCBChannelOps alone does not catch the constructor's refusal: a layer norm of the user's that has a bias and
    no weight raises, as it always did, and the container is left as it was."""
    class LayerNorm2d(nn.Module):
        def __init__(self):
            super(LayerNorm2d, self).__init__()
            self.weight, self.bias, self.eps = None, nn.Parameter(torch.zeros(4)), 1e-6
    net = nn.Sequential(conv(), LayerNorm2d(), conv())
    with pytest.raises(Err, match="has a bias but no weight"):
        pkg.insertCBChannelOps(net, layerNormTypes=(LayerNorm2d,))
    assert wiring(net) == '0:CBConv2d/p0i0 1:LayerNorm2d 2:CBConv2d/p0i0'


# ------------------------------------------------------------------------------------------------ the consumer rule
def test_consumer_rule_in_its_four_outcomes(pkg, chain):
    def flags(front, cons):
        return front.propChangeIndexes, getattr(cons, 'copyInput', None)
    for handOn, cons, want in ((True, conv(1), (True, False)), (True, conv(3), (False, True)),
                               (True, conv(3, feedback=True), (False, False)), (True, nn.Identity(), (False, None)),
                               (True, conv(1, feedback=True), (True, False)), (True, conv(1, stride=2), (False, True)),
                               (True, conv(groups=2), (False, False)),      # (exactly a CBConv2d, not another layer)
                               # a pass that never hands on: a 1x1 consumer is a CBConv2d like any other
                               (False, conv(1), (False, True)), (False, conv(3), (False, True)),
                               (False, conv(1, feedback=True), (False, False)), (False, nn.Identity(), (False, None))):
        front = pkg.CBPad2d(nn.ZeroPad2d(1))
        assert chain.link_consumer(front, cons, handOn=handOn) is None
        assert flags(front, cons) == want, (handOn, cons)


def test_walk_calls_convert_behind_producers_only_and_returns_the_root(pkg, chain):
    seen = []

    def convert(m):
        seen.append(type(m).__name__)
        return pkg.CBPad2d(nn.ZeroPad2d(1)) if type(m) is nn.ZeroPad2d else None
    net = nn.Sequential(nn.ZeroPad2d(1), conv(), nn.ZeroPad2d(1), nn.ZeroPad2d(2), conv(1), nn.Tanh(), nn.ZeroPad2d(1))
    assert chain.insert_behind_producers(net, (pkg.CBConv2d,), convert) is net
    # (the new CBPad2d is no producer of THIS call; the pad behind the Tanh is never offered)
    assert seen == ['ZeroPad2d', 'Tanh']
    assert wiring(net) == ('0:ZeroPad2d 1:CBConv2d/p1i0 2:CBPad2d/p0c1 3:ZeroPad2d 4:CBConv2d/p0i0 5:Tanh '
                           '6:ZeroPad2d')
    assert list(net._modules) == ['0', '1', '2', '3', '4', '5', '6']


# ------------------------------------------------------------------------------------------------ the frame skeleton
def test_every_pixel_form_and_its_expansion(chain):
    assert chain.EVERY_PIXEL == (None, None, 0, None)
    assert chain.operand_changes('M', 'the input', None, 4, 5, torch.device('cpu'), None) == chain.EVERY_PIXEL
    assert chain.form_args(chain.EVERY_PIXEL) == (None, None, 0, None)
    mask, lst, count = torch.zeros(2, dtype=torch.int64), torch.zeros(6, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    assert chain.form_args((mask, None, 0, None)) == (mask.data_ptr(), None, 0, None)
    assert chain.form_args((None, lst, 6, count)) == (None, lst.data_ptr(), 6, count.data_ptr())


SLOTS = (('CBAdd2d', '_addWork'), ('CBPointwise2d', '_pwWork'), ('CBChannelReduce2d', '_chWork'),
         ('CBBinary2d', '_binWork'), ('CBGLU2d', '_binWork'), ('CBUpsample2d', '_work'), ('CBConcat2d', '_work'),
         ('CBPixelShuffle2d', '_work'), ('CBChannelShuffle2d', '_work'), ('CBResize2d', '_work'), ('CBPad2d', '_work'))


def _module(pkg, name):
    return {'CBAdd2d': lambda: pkg.CBAdd2d(), 'CBConcat2d': lambda: pkg.CBConcat2d(),
            'CBPixelShuffle2d': lambda: pkg.CBPixelShuffle2d(nn.PixelShuffle(2)),
            'CBChannelShuffle2d': lambda: pkg.CBChannelShuffle2d(nn.ChannelShuffle(2))}.get(name, _producers(pkg).get(name))()


@pytest.mark.parametrize("name,slot", SLOTS)
def test_workspace_cache(pkg, name, slot):
    """The same dict for an equal key, a new one for another key, the old one when `make` raises; emptied by
    clearMemory() and dropped by pickling.  `make` stands in for chain.mask_workspace with CPU tensors."""
    m = _module(pkg, name)
    assert m._WORK == slot and m.__dict__[slot] is None
    made = []

    def make():
        made.append(1)
        return dict(bits=torch.zeros(2, dtype=torch.int64), copy=torch.zeros(2, dtype=torch.int64), size=(3, 4))
    key = (3, 4, torch.device('cpu'))
    work = m._cached_work(key, make)
    assert work is m.__dict__[slot] and work['key'] == key and work['size'] == (3, 4) and len(made) == 1
    assert m._cached_work((3, 4, torch.device('cpu')), make) is work and len(made) == 1
    assert getattr(m, slot) is work      # (what the tests and the benchmark read)

    def refuse():
        raise ValueError("no such size")
    with pytest.raises(ValueError, match="no such size"):
        m._cached_work((5, 4, torch.device('cpu')), refuse)
    assert m.__dict__[slot] is work and work['key'] == key
    other = m._cached_work((5, 4, torch.device('cpu')), make)
    assert other is not work and other['key'][0] == 5 and m.__dict__[slot] is other and len(made) == 2
    clone = pickle.loads(pickle.dumps(m))
    assert clone.__dict__[slot] is None and m.__dict__[slot] is other
    m.clearMemory()
    assert m.__dict__[slot] is None
    assert m._cached_work(key, make) is not work and len(made) == 3


def test_resize_keeps_its_workspace_and_its_struct_when_the_geometry_refuses(pkg, Err):
    m = pkg.CBResize2d(size=(9, 11))
    work, struct = {'key': (4, 5, None, torch.device('cpu'))}, object()
    m.__dict__['_work'], m.__dict__['_rsC'] = work, struct
    with pytest.raises(Err, match="is a ratio beyond 8"):
        m._workspace(1, 1, (9, 9), torch.device('cpu'))
    assert m.__dict__['_work'] is work and m.__dict__['_rsC'] is struct
    assert m._workspace(4, 5, None, torch.device('cpu')) is work


def test_state_step_keeps_a_fitting_state_and_says_when_it_made_one(pkg):
    m = pkg.CBPad2d(nn.ZeroPad2d(1))
    x = torch.zeros(1, 3, 4, 5)
    assert m.outputState.numel() == 0
    assert m._fresh_state((1, 3, 6, 7), x) is True
    state = m.outputState
    assert tuple(state.shape) == (1, 3, 6, 7) and state.dtype == x.dtype and state.device == x.device
    assert m._fresh_state((1, 3, 6, 7), x) is False and m.outputState is state
    assert m._fresh_state([1, 3, 6, 7], torch.ones(2, 2)) is False and m.outputState is state
    # another shape, another dtype, another device: each is a new state, with the operand's dtype and device
    assert m._fresh_state((1, 3, 6, 8), x) is True and tuple(m.outputState.shape) == (1, 3, 6, 8)
    assert m._fresh_state((1, 3, 6, 8), x.half()) is True and m.outputState.dtype == torch.float16
    assert m._fresh_state((1, 3, 6, 8), x.half()) is False
    meta = torch.zeros(1, dtype=torch.float16, device='meta')
    assert m._fresh_state((1, 3, 6, 8), meta) is True and m.outputState.device.type == 'meta'
    assert m._fresh_state((1, 3, 6, 8), meta) is False
    assert 'outputState' in m._buffers and m.getStateTensors()[0] is m.outputState
    m.clearMemory()
    assert m.outputState.numel() == 0 and m._fresh_state((1, 3, 6, 8), meta) is True


MAP_WORDS = (('CBPointwise2d', 'the input', ''), ('CBUpsample2d', 'the input', ''), ('CBPixelShuffle2d', 'the input', ''),
             ('CBChannelShuffle2d', 'the input', ''), ('CBChannelReduce2d', 'the input', ''),
             ('CBResize2d', 'the input', ' (batch 1)'), ('CBPad2d', 'the input', ' (batch 1)'),
             ('CBBinary2d', 'operand a', ''), ('CBGLU2d', 'operand x', ''))


@pytest.mark.parametrize("name,which,note", MAP_WORDS)
def test_map_check_raises_each_modules_own_words(pkg, chain, Err, name, which, note):
    """The messages as the modules worded them before the check was written once, byte for byte: through the helper and
    through the module's forward (a 3-D tensor, a batch of 2, a float64 tensor)."""
    m = _module(pkg, name)
    for x in (torch.zeros(4, 6, 6), torch.zeros(2, 4, 6, 6)):
        want = "%s: %s must be a [1, C, H, W] tensor%s, got %s" % (name, which, note, tuple(x.shape))
        for call in (lambda: chain.check_map(name, x, which, note), lambda: m(x)):
            with pytest.raises(Err) as said:
                call()
            assert str(said.value) == want
    x = torch.zeros(1, 4, 6, 6, dtype=torch.float64)
    for call in (lambda: chain.check_map(name, x, which, note), lambda: m(x)):
        with pytest.raises(Err) as said:
            call()
        assert str(said.value) == "%s: float32 and float16 tensors only, got torch.float64" % name
    for dtype in (torch.float32, torch.float16):
        assert chain.check_map(name, torch.zeros(1, 4, 6, 6, dtype=dtype), which, note) is None


def test_add_and_concat_keep_their_own_words(pkg, Err):
    x = torch.zeros(2, 4, 6, 6)
    with pytest.raises(Err) as said:
        pkg.CBAdd2d()(x, x)
    assert str(said.value) == "CBAdd2d: operands must be [1, C, H, W] tensors, a is (2, 4, 6, 6)"
    with pytest.raises(Err) as said:
        pkg.CBConcat2d()([torch.zeros(1, 4, 6, 6), x])
    assert str(said.value) == "CBConcat2d: operands must be [1, C, H, W] tensors, operand 1 is (2, 4, 6, 6)"
    with pytest.raises(Err) as said:
        pkg.CBConcat2d()([torch.zeros(1, 4, 6, 6).double()] * 2)
    assert str(said.value) == "CBConcat2d: float32 and float16 tensors only, got torch.float64"


def test_refusals_keep_their_order(pkg, Err):
    """What a module refuses first on a machine without a GPU: CBPointwise2d, CBChannelReduce2d, the shuffles and CBPad2d
    name the map before the device, CBUpsample2d and CBResize2d the device before anything derived from the map."""
    x = torch.zeros(1, 4, 6, 6)
    bn = nn.BatchNorm2d(3).eval()
    for call, what in ((lambda: pkg.CBPointwise2d(norm=bn)(x), "the input has 4 channels, scale was made for 3"),
                       (lambda: pkg.CBChannelReduce2d(nn.LayerNorm(3))(x), "the input has 4 channels, gamma was made for 3"),
                       (lambda: pkg.CBPixelShuffle2d(nn.PixelShuffle(3))(x), "which upscale_factor\\^2 = 9 does not divide"),
                       (lambda: pkg.CBChannelShuffle2d(nn.ChannelShuffle(3))(x), "which groups = 3 does not divide"),
                       (lambda: pkg.CBPad2d(padding=1, value=1e30)(x.half()), "overflows the tensor's dtype"),
                       (lambda: pkg.CBPad2d(nn.ReflectionPad2d(7))(x), "HIP devices only"),
                       (lambda: pkg.CBUpsample2d(nn.Upsample(scale_factor=2))(x), "HIP devices only"),
                       (lambda: pkg.CBResize2d(size=(600, 6))(x), "HIP devices only"),
                       (lambda: pkg.CBGLU2d(nn.GLU(1))(x[:, :3]), "has an odd number of channels"),
                       (lambda: pkg.CBAdd2d()(x, x.half()), "the operands differ"),
                       (lambda: pkg.CBAdd2d()(x, x), "HIP devices only"),
                       (lambda: pkg.CBConcat2d()([x, x]), "HIP devices only")):
        with pytest.raises(Err, match=what):
            call()


# ------------------------------------------------------------------------------------------------ the GPU cases
def test_every_accepted_pair_has_a_gpu_case(pkg, chain):
    """tests/chain_cases.py, which tests/test_gpu_chain.py runs on the device, covers exactly the (pass, producer type)
    pairs the table accepts: a row added to PRODUCERS, or a pass added to PASSES, without a case there fails here by
    name, and so does a case for a pair the table no longer accepts.  Both kinds of CBPoolMax2d wherever the type is."""
    accepted = {(p, T.__name__) for p in chain.PASSES for T in chain.producers(p)}
    covered = cc.pairs()
    missing, stale = sorted(accepted - covered), sorted(covered - accepted)
    assert not missing, "accepted by chain.PRODUCERS, no case in tests/chain_cases.py: %s" % (missing,)
    assert not stale, "a case in tests/chain_cases.py, not accepted by chain.PRODUCERS: %s" % (stale,)
    assert len(accepted) == 155 and tuple(cc.BEHIND) == tuple(chain.PASSES) == tuple(cc.PASSES)
    for passName, behind in cc.BEHIND.items():
        assert ('CBPoolMax2d 2x2' in behind) == ('CBPoolMax2d 3x3' in behind) == (
            pkg.CBPoolMax2d in chain.producers(passName)), passName
        assert len(set(behind)) == len(behind) and set(behind) <= set(cc.PRODUCERS), passName
    assert len(set(cc.CASES)) == len(cc.CASES) == 155 + 9 + 3      # (+ a second pool kind, + a second general pool)
    assert {cc.producer_type(c) for c in cc.CASES} == {name for name, _, rule, passes in chain.PRODUCERS
                                                       if rule is chain.BUT or passes}


@pytest.mark.parametrize("case", cc.CASES, ids=cc.case_id)
def test_the_pass_wires_every_gpu_case(pkg, chain, case):
    """The pass, run on the case's network, really puts its change-based operator behind the producer and switches the
    producer's change output on where chain.hand_on_changes does -- else the GPU test would compare two dense networks.
    And the condition of that test's listed-share cap: by numpy dilation the footprint of the one- and two-pixel frames
    stays far below half of the operator's map."""
    for cloneOutput in (True, False):
        net = cc.build(pkg, case, cloneOutput=cloneOutput)
        stem, prod, op = net.seq
        assert type(stem) is pkg.CBConv2d and type(prod).__name__ == cc.producer_type(case), case
        assert type(prod) in chain.producers(case.passName), case
        assert type(op).__name__ == cc.OPS[case.op].becomes and type(op).__module__.startswith('cbinfer_amd'), case
        assert op.cloneOutput is cloneOutput, case
        target = cc.hand_on_target(prod)
        assert getattr(target, 'cloneOutput', cloneOutput) is cloneOutput, case
        assert target.propChangeIndexes == (case.passName not in cc.OWN_DETECTION), case
        assert stem.propChangeIndexes == cc.PRODUCERS[case.producer].fed or case.passName == 'linkDepthwise', case
        if case.producer.startswith('CBPoolMax2d'):
            assert bool(prod.__dict__['_general']) == case.producer.endswith('3x3'), case
            assert prod.downsampleIndexes == (case.producer.endswith('2x2') and target.propChangeIndexes), case
        if case.passName == 'linkDepthwise':
            assert op.propagatedChanges, case
        if type(op) is pkg.CBPoolMax2d:
            assert bool(op.__dict__['_general']) == (case.passName == cc.GENERAL_POOLS), case
        assert (net.second is not None) == cc.PRODUCERS[case.producer].two
    maps = cc.changed()
    assert [int(m.sum()) for m in maps[:6]] == [cc.H * cc.W, 1, 2, 1, 0, 1] and maps[7].all() and maps[6].sum() > 9
    for t in cc.LOCAL:
        listed = cc.footprint(case, maps[t])
        assert listed.any() and listed.mean() < 0.5, (case, t, float(listed.mean()))
    assert not cc.footprint(case, maps[cc.IDLE]).any() and cc.footprint(case, maps[0]).all(), case


def test_gpu_frames_are_what_the_cases_say():
    """Eight frames: values in [0, 0.9], exact in float16; a frame differs from the one before at exactly the pixels of
    changed(), by 0.5 in every channel -- ten times the stem's threshold in both dtypes."""
    maps = cc.changed()
    for dtype in (torch.float32, torch.float16):
        fr = cc.frames(dtype)
        assert len(fr) == len(maps) == 8 and all(tuple(f.shape) == (1, 3, cc.H, cc.W) and f.dtype == dtype for f in fr)
        assert all(torch.equal(f.double(), g.double()) for f, g in zip(fr, cc.frames(torch.float32)))
        assert all(0.0 <= float(f.min()) and float(f.max()) <= 0.9 for f in fr)
        for t in range(1, 8):
            moved = (fr[t].double() - fr[t - 1].double()).abs()[0]
            assert bool((moved[:, torch.from_numpy(maps[t])] == 0.5).all()), t
            assert bool((moved[:, torch.from_numpy(~maps[t])] == 0.0).all()), t
        assert torch.equal(fr[cc.IDLE], fr[cc.IDLE - 1])


# ------------------------------------------------------------------------------------------------ recorded
# {pass: {scenario: (wiring(net) after the pass with its defaults, after the pass with cloneOutput=False -- None where
# the pass has no such parameter)}}, written by record() at the commit before the passes shared one walk
WIRING = {
    'insertCBRearrange': {
        'behind CBConv2d': (
            '0:CBConv2d/p1i0 1:CBPixelShuffle2d/p0c1 2:CBConv2d/p0i1',
            '0:CBConv2d/p1i0 1:CBPixelShuffle2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBPoolMax2d 2x2': (
            '0:CBPoolMax2d/p1c1d1 1:CBPixelShuffle2d/p0c1 2:CBConv2d/p0i1',
            '0:CBPoolMax2d/p1c1d1 1:CBPixelShuffle2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBPoolMax2d 3x3': (
            '0:CBPoolMax2d/p1c1d0 1:CBPixelShuffle2d/p0c1 2:CBConv2d/p0i1',
            '0:CBPoolMax2d/p1c1d0 1:CBPixelShuffle2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBPoolAvg2d': (
            '0:CBPoolAvg2d/p1c1d0 1:CBPixelShuffle2d/p0c1 2:CBConv2d/p0i1',
            '0:CBPoolAvg2d/p1c1d0 1:CBPixelShuffle2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBAdd2d': (
            '0:CBAdd2d/p1c1 1:CBPixelShuffle2d/p0c1 2:CBConv2d/p0i1',
            '0:CBAdd2d/p1c1 1:CBPixelShuffle2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBResidual': (
            '0:CBResidual 0.body:Sequential 0.body.0:CBConv2d/p0i1 0.body.1:CBConv2d/p1i0 0.add:CBAdd2d/p1c1 1:CBPixelShuffle2d/p0c1 2:CBConv2d/p0i1',
            '0:CBResidual 0.body:Sequential 0.body.0:CBConv2d/p0i1 0.body.1:CBConv2d/p1i0 0.add:CBAdd2d/p1c1 1:CBPixelShuffle2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBUpsample2d': (
            '0:CBUpsample2d/p1c1 1:CBPixelShuffle2d/p0c1 2:CBConv2d/p0i1',
            '0:CBUpsample2d/p1c1 1:CBPixelShuffle2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBConvTranspose2d': (
            '0:CBConvTranspose2d/p1c1i1 1:CBPixelShuffle2d/p0c1 2:CBConv2d/p0i1',
            '0:CBConvTranspose2d/p1c1i1 1:CBPixelShuffle2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBDepthwiseConv2d': (
            '0:CBDepthwiseConv2d/p1c1i0 1:CBPixelShuffle2d/p0c1 2:CBConv2d/p0i1',
            '0:CBDepthwiseConv2d/p1c1i0 1:CBPixelShuffle2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBPointwise2d': (
            '0:CBPointwise2d/p1c1 1:CBPixelShuffle2d/p0c1 2:CBConv2d/p0i1',
            '0:CBPointwise2d/p1c1 1:CBPixelShuffle2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBPixelShuffle2d': (
            '0:CBPixelShuffle2d/p1c1 1:CBPixelShuffle2d/p0c1 2:CBConv2d/p0i1',
            '0:CBPixelShuffle2d/p1c1 1:CBPixelShuffle2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBChannelShuffle2d': (
            '0:CBChannelShuffle2d/p1c1 1:CBPixelShuffle2d/p0c1 2:CBConv2d/p0i1',
            '0:CBChannelShuffle2d/p1c1 1:CBPixelShuffle2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBResize2d': (
            '0:CBResize2d/p1c1 1:CBPixelShuffle2d/p0c1 2:CBConv2d/p0i1',
            '0:CBResize2d/p1c1 1:CBPixelShuffle2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBPad2d': (
            '0:CBPad2d/p1c1 1:CBPixelShuffle2d/p0c1 2:CBConv2d/p0i1',
            '0:CBPad2d/p1c1 1:CBPixelShuffle2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBBinary2d': (
            '0:CBBinary2d/p1c1 1:CBPixelShuffle2d/p0c1 2:CBConv2d/p0i1',
            '0:CBBinary2d/p1c1 1:CBPixelShuffle2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBGLU2d': (
            '0:CBGLU2d/p1c1 1:CBPixelShuffle2d/p0c1 2:CBConv2d/p0i1',
            '0:CBGLU2d/p1c1 1:CBPixelShuffle2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBGated': (
            '0:CBGated 0.body:Sequential 0.body.0:CBConv2d/p0i1 0.body.1:CBConv2d/p1i0 0.mul:CBBinary2d/p1c1 1:CBPixelShuffle2d/p0c1 2:CBConv2d/p0i1',
            '0:CBGated 0.body:Sequential 0.body.0:CBConv2d/p0i1 0.body.1:CBConv2d/p1i0 0.mul:CBBinary2d/p1c1 1:CBPixelShuffle2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBGroupedConv2d': (
            '0:CBGroupedConv2d/p1c1i0 1:CBPixelShuffle2d/p0c1 2:CBConv2d/p0i1',
            '0:CBGroupedConv2d/p1c1i0 1:CBPixelShuffle2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBChannelReduce2d': (
            '0:CBChannelReduce2d/p0c1 1:PixelShuffle 2:CBConv2d/p0i0',
            '0:CBChannelReduce2d/p0c1 1:PixelShuffle 2:CBConv2d/p0i0'),
        'behind dense': (
            '0:Identity 1:PixelShuffle 2:CBConv2d/p0i0',
            '0:Identity 1:PixelShuffle 2:CBConv2d/p0i0'),
        'at position 0': (
            '0:PixelShuffle 1:CBConv2d/p0i0',
            '0:PixelShuffle 1:CBConv2d/p0i0'),
        'the last child': (
            '0:CBConv2d/p1i0 1:CBPixelShuffle2d/p0c1',
            '0:CBConv2d/p1i0 1:CBPixelShuffle2d/p0c0'),
        'in front of a 1x1': (
            '0:CBConv2d/p1i0 1:CBPixelShuffle2d/p1c1 2:CBConv2d/p0i0',
            '0:CBConv2d/p1i0 1:CBPixelShuffle2d/p1c0 2:CBConv2d/p0i0'),
        'in front of a strided 1x1': (
            '0:CBConv2d/p1i0 1:CBPixelShuffle2d/p0c1 2:CBConv2d/p0i1',
            '0:CBConv2d/p1i0 1:CBPixelShuffle2d/p0c0 2:CBConv2d/p0i1'),
        'in front of a 3x3 in feedback mode': (
            '0:CBConv2d/p1i0 1:CBPixelShuffle2d/p0c1 2:CBConv2d/p0i0',
            '0:CBConv2d/p1i0 1:CBPixelShuffle2d/p0c0 2:CBConv2d/p0i0'),
        'in front of a 1x1 in feedback mode': (
            '0:CBConv2d/p1i0 1:CBPixelShuffle2d/p1c1 2:CBConv2d/p0i0',
            '0:CBConv2d/p1i0 1:CBPixelShuffle2d/p1c0 2:CBConv2d/p0i0'),
        'in front of a dense module': (
            '0:CBConv2d/p1i0 1:CBPixelShuffle2d/p0c1 2:Identity',
            '0:CBConv2d/p1i0 1:CBPixelShuffle2d/p0c0 2:Identity'),
        'in front of a grouped convolution': (
            '0:CBConv2d/p1i0 1:CBPixelShuffle2d/p0c1 2:CBGroupedConv2d/p0c1i0',
            '0:CBConv2d/p1i0 1:CBPixelShuffle2d/p0c0 2:CBGroupedConv2d/p0c1i0'),
        'two in a row': (
            '0:CBConv2d/p1i0 1:CBPixelShuffle2d/p1c1 2:CBPixelShuffle2d/p1c1 3:CBConv2d/p0i0',
            '0:CBConv2d/p1i0 1:CBPixelShuffle2d/p1c0 2:CBPixelShuffle2d/p1c0 3:CBConv2d/p0i0'),
        'nested': (
            '0:Identity 1:Sequential 1.0:CBConv2d/p1i0 1.1:CBPixelShuffle2d/p1c1 1.2:CBConv2d/p0i0 2:PixelShuffle 3:Sequential 3.0:Sequential 3.0.0:CBConv2d/p1i0 3.0.1:CBPixelShuffle2d/p0c1',
            '0:Identity 1:Sequential 1.0:CBConv2d/p1i0 1.1:CBPixelShuffle2d/p1c0 1.2:CBConv2d/p0i0 2:PixelShuffle 3:Sequential 3.0:Sequential 3.0.0:CBConv2d/p1i0 3.0.1:CBPixelShuffle2d/p0c0'),
        'in a subclass of nn.Sequential': (
            '0:MySequential 0.0:CBConv2d/p0i0 0.1:PixelShuffle 0.2:CBConv2d/p0i0',
            '0:MySequential 0.0:CBConv2d/p0i0 0.1:PixelShuffle 0.2:CBConv2d/p0i0'),
        'beyond the limits': (
            '0:CBConv2d/p0i0 1:PixelShuffle 2:CBConv2d/p0i0',
            '0:CBConv2d/p0i0 1:PixelShuffle 2:CBConv2d/p0i0'),
        'a ReLU behind it': (
            '0:CBConv2d/p1i0 1:CBPixelShuffle2d/p0c1 2:ReLU 3:CBConv2d/p0i0',
            '0:CBConv2d/p1i0 1:CBPixelShuffle2d/p0c0 2:ReLU 3:CBConv2d/p0i0'),
        'a ReLU behind it, twice': (
            '0:CBConv2d/p1i0 1:CBPixelShuffle2d/p0c1 2:ReLU 3:PixelShuffle 4:ReLU 5:CBConv2d/p0i0',
            '0:CBConv2d/p1i0 1:CBPixelShuffle2d/p0c0 2:ReLU 3:PixelShuffle 4:ReLU 5:CBConv2d/p0i0'),
        'a batch norm and an activation behind it': (
            '0:CBConv2d/p0i0 1:BatchNorm2d 2:PixelShuffle 3:CBConv2d/p0i0',
            '0:CBConv2d/p0i0 1:BatchNorm2d 2:PixelShuffle 3:CBConv2d/p0i0'),
    },
    'insertCBChannelOps': {
        'behind CBConv2d': (
            '0:CBConv2d/p1i0 1:CBChannelReduce2d/p0c1 2:CBConv2d/p0i1',
            None),
        'behind CBPoolMax2d 2x2': (
            '0:CBPoolMax2d/p1c1d1 1:CBChannelReduce2d/p0c1 2:CBConv2d/p0i1',
            None),
        'behind CBPoolMax2d 3x3': (
            '0:CBPoolMax2d/p1c1d0 1:CBChannelReduce2d/p0c1 2:CBConv2d/p0i1',
            None),
        'behind CBPoolAvg2d': (
            '0:CBPoolAvg2d/p1c1d0 1:CBChannelReduce2d/p0c1 2:CBConv2d/p0i1',
            None),
        'behind CBAdd2d': (
            '0:CBAdd2d/p1c1 1:CBChannelReduce2d/p0c1 2:CBConv2d/p0i1',
            None),
        'behind CBResidual': (
            '0:CBResidual 0.body:Sequential 0.body.0:CBConv2d/p0i1 0.body.1:CBConv2d/p1i0 0.add:CBAdd2d/p1c1 1:CBChannelReduce2d/p0c1 2:CBConv2d/p0i1',
            None),
        'behind CBUpsample2d': (
            '0:CBUpsample2d/p1c1 1:CBChannelReduce2d/p0c1 2:CBConv2d/p0i1',
            None),
        'behind CBConvTranspose2d': (
            '0:CBConvTranspose2d/p1c1i1 1:CBChannelReduce2d/p0c1 2:CBConv2d/p0i1',
            None),
        'behind CBDepthwiseConv2d': (
            '0:CBDepthwiseConv2d/p1c1i0 1:CBChannelReduce2d/p0c1 2:CBConv2d/p0i1',
            None),
        'behind CBPointwise2d': (
            '0:CBPointwise2d/p1c1 1:CBChannelReduce2d/p0c1 2:CBConv2d/p0i1',
            None),
        'behind CBPixelShuffle2d': (
            '0:CBPixelShuffle2d/p1c1 1:CBChannelReduce2d/p0c1 2:CBConv2d/p0i1',
            None),
        'behind CBChannelShuffle2d': (
            '0:CBChannelShuffle2d/p1c1 1:CBChannelReduce2d/p0c1 2:CBConv2d/p0i1',
            None),
        'behind CBResize2d': (
            '0:CBResize2d/p1c1 1:CBChannelReduce2d/p0c1 2:CBConv2d/p0i1',
            None),
        'behind CBPad2d': (
            '0:CBPad2d/p1c1 1:CBChannelReduce2d/p0c1 2:CBConv2d/p0i1',
            None),
        'behind CBBinary2d': (
            '0:CBBinary2d/p1c1 1:CBChannelReduce2d/p0c1 2:CBConv2d/p0i1',
            None),
        'behind CBGLU2d': (
            '0:CBGLU2d/p1c1 1:CBChannelReduce2d/p0c1 2:CBConv2d/p0i1',
            None),
        'behind CBGated': (
            '0:CBGated 0.body:Sequential 0.body.0:CBConv2d/p0i1 0.body.1:CBConv2d/p1i0 0.mul:CBBinary2d/p1c1 1:CBChannelReduce2d/p0c1 2:CBConv2d/p0i1',
            None),
        'behind CBGroupedConv2d': (
            '0:CBGroupedConv2d/p1c1i0 1:CBChannelReduce2d/p0c1 2:CBConv2d/p0i1',
            None),
        'behind CBChannelReduce2d': (
            '0:CBChannelReduce2d/p1c1 1:CBChannelReduce2d/p0c1 2:CBConv2d/p0i1',
            None),
        'behind dense': (
            '0:Identity 1:Softmax2d 2:CBConv2d/p0i0',
            None),
        'at position 0': (
            '0:Softmax2d 1:CBConv2d/p0i0',
            None),
        'the last child': (
            '0:CBConv2d/p1i0 1:CBChannelReduce2d/p0c1',
            None),
        'in front of a 1x1': (
            '0:CBConv2d/p1i0 1:CBChannelReduce2d/p1c1 2:CBConv2d/p0i0',
            None),
        'in front of a strided 1x1': (
            '0:CBConv2d/p1i0 1:CBChannelReduce2d/p0c1 2:CBConv2d/p0i1',
            None),
        'in front of a 3x3 in feedback mode': (
            '0:CBConv2d/p1i0 1:CBChannelReduce2d/p0c1 2:CBConv2d/p0i0',
            None),
        'in front of a 1x1 in feedback mode': (
            '0:CBConv2d/p1i0 1:CBChannelReduce2d/p1c1 2:CBConv2d/p0i0',
            None),
        'in front of a dense module': (
            '0:CBConv2d/p1i0 1:CBChannelReduce2d/p0c1 2:Identity',
            None),
        'in front of a grouped convolution': (
            '0:CBConv2d/p1i0 1:CBChannelReduce2d/p0c1 2:CBGroupedConv2d/p0c1i0',
            None),
        'two in a row': (
            '0:CBConv2d/p1i0 1:CBChannelReduce2d/p1c1 2:CBChannelReduce2d/p1c1 3:CBConv2d/p0i0',
            None),
        'nested': (
            '0:Identity 1:Sequential 1.0:CBConv2d/p1i0 1.1:CBChannelReduce2d/p1c1 1.2:CBConv2d/p0i0 2:Softmax2d 3:Sequential 3.0:Sequential 3.0.0:CBConv2d/p1i0 3.0.1:CBChannelReduce2d/p0c1',
            None),
        'in a subclass of nn.Sequential': (
            '0:MySequential 0.0:CBConv2d/p0i0 0.1:Softmax2d 0.2:CBConv2d/p0i0',
            None),
        'beyond the limits': (
            '0:CBConv2d/p0i0 1:Softmax 2:CBConv2d/p0i0',
            None),
        'a ReLU behind it': (
            '0:CBConv2d/p1i0 1:CBChannelReduce2d/p0c1 2:ReLU 3:CBConv2d/p0i0',
            None),
        'a ReLU behind it, twice': (
            '0:CBConv2d/p1i0 1:CBChannelReduce2d/p0c1 2:ReLU 3:Softmax2d 4:ReLU 5:CBConv2d/p0i0',
            None),
        'a batch norm and an activation behind it': (
            '0:CBConv2d/p0i0 1:BatchNorm2d 2:Softmax2d 3:CBConv2d/p0i0',
            None),
    },
    'insertCBResize': {
        'behind CBConv2d': (
            '0:CBConv2d/p1i0 1:CBResize2d/p0c1 2:CBConv2d/p0i1',
            '0:CBConv2d/p1i0 1:CBResize2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBPoolMax2d 2x2': (
            '0:CBPoolMax2d/p1c1d1 1:CBResize2d/p0c1 2:CBConv2d/p0i1',
            '0:CBPoolMax2d/p1c1d1 1:CBResize2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBPoolMax2d 3x3': (
            '0:CBPoolMax2d/p1c1d0 1:CBResize2d/p0c1 2:CBConv2d/p0i1',
            '0:CBPoolMax2d/p1c1d0 1:CBResize2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBPoolAvg2d': (
            '0:CBPoolAvg2d/p1c1d0 1:CBResize2d/p0c1 2:CBConv2d/p0i1',
            '0:CBPoolAvg2d/p1c1d0 1:CBResize2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBAdd2d': (
            '0:CBAdd2d/p1c1 1:CBResize2d/p0c1 2:CBConv2d/p0i1',
            '0:CBAdd2d/p1c1 1:CBResize2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBResidual': (
            '0:CBResidual 0.body:Sequential 0.body.0:CBConv2d/p0i1 0.body.1:CBConv2d/p1i0 0.add:CBAdd2d/p1c1 1:CBResize2d/p0c1 2:CBConv2d/p0i1',
            '0:CBResidual 0.body:Sequential 0.body.0:CBConv2d/p0i1 0.body.1:CBConv2d/p1i0 0.add:CBAdd2d/p1c1 1:CBResize2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBUpsample2d': (
            '0:CBUpsample2d/p1c1 1:CBResize2d/p0c1 2:CBConv2d/p0i1',
            '0:CBUpsample2d/p1c1 1:CBResize2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBConvTranspose2d': (
            '0:CBConvTranspose2d/p0c1i1 1:Upsample 2:CBConv2d/p0i0',
            '0:CBConvTranspose2d/p0c1i1 1:Upsample 2:CBConv2d/p0i0'),
        'behind CBDepthwiseConv2d': (
            '0:CBDepthwiseConv2d/p1c1i0 1:CBResize2d/p0c1 2:CBConv2d/p0i1',
            '0:CBDepthwiseConv2d/p1c1i0 1:CBResize2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBPointwise2d': (
            '0:CBPointwise2d/p1c1 1:CBResize2d/p0c1 2:CBConv2d/p0i1',
            '0:CBPointwise2d/p1c1 1:CBResize2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBPixelShuffle2d': (
            '0:CBPixelShuffle2d/p1c1 1:CBResize2d/p0c1 2:CBConv2d/p0i1',
            '0:CBPixelShuffle2d/p1c1 1:CBResize2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBChannelShuffle2d': (
            '0:CBChannelShuffle2d/p1c1 1:CBResize2d/p0c1 2:CBConv2d/p0i1',
            '0:CBChannelShuffle2d/p1c1 1:CBResize2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBResize2d': (
            '0:CBResize2d/p1c1 1:CBResize2d/p0c1 2:CBConv2d/p0i1',
            '0:CBResize2d/p1c1 1:CBResize2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBPad2d': (
            '0:CBPad2d/p1c1 1:CBResize2d/p0c1 2:CBConv2d/p0i1',
            '0:CBPad2d/p1c1 1:CBResize2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBBinary2d': (
            '0:CBBinary2d/p1c1 1:CBResize2d/p0c1 2:CBConv2d/p0i1',
            '0:CBBinary2d/p1c1 1:CBResize2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBGLU2d': (
            '0:CBGLU2d/p1c1 1:CBResize2d/p0c1 2:CBConv2d/p0i1',
            '0:CBGLU2d/p1c1 1:CBResize2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBGated': (
            '0:CBGated 0.body:Sequential 0.body.0:CBConv2d/p0i1 0.body.1:CBConv2d/p1i0 0.mul:CBBinary2d/p1c1 1:CBResize2d/p0c1 2:CBConv2d/p0i1',
            '0:CBGated 0.body:Sequential 0.body.0:CBConv2d/p0i1 0.body.1:CBConv2d/p1i0 0.mul:CBBinary2d/p1c1 1:CBResize2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBGroupedConv2d': (
            '0:CBGroupedConv2d/p1c1i0 1:CBResize2d/p0c1 2:CBConv2d/p0i1',
            '0:CBGroupedConv2d/p1c1i0 1:CBResize2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBChannelReduce2d': (
            '0:CBChannelReduce2d/p1c1 1:CBResize2d/p0c1 2:CBConv2d/p0i1',
            '0:CBChannelReduce2d/p1c1 1:CBResize2d/p0c0 2:CBConv2d/p0i1'),
        'behind dense': (
            '0:Identity 1:Upsample 2:CBConv2d/p0i0',
            '0:Identity 1:Upsample 2:CBConv2d/p0i0'),
        'at position 0': (
            '0:Upsample 1:CBConv2d/p0i0',
            '0:Upsample 1:CBConv2d/p0i0'),
        'the last child': (
            '0:CBConv2d/p1i0 1:CBResize2d/p0c1',
            '0:CBConv2d/p1i0 1:CBResize2d/p0c0'),
        'in front of a 1x1': (
            '0:CBConv2d/p1i0 1:CBResize2d/p1c1 2:CBConv2d/p0i0',
            '0:CBConv2d/p1i0 1:CBResize2d/p1c0 2:CBConv2d/p0i0'),
        'in front of a strided 1x1': (
            '0:CBConv2d/p1i0 1:CBResize2d/p0c1 2:CBConv2d/p0i1',
            '0:CBConv2d/p1i0 1:CBResize2d/p0c0 2:CBConv2d/p0i1'),
        'in front of a 3x3 in feedback mode': (
            '0:CBConv2d/p1i0 1:CBResize2d/p0c1 2:CBConv2d/p0i0',
            '0:CBConv2d/p1i0 1:CBResize2d/p0c0 2:CBConv2d/p0i0'),
        'in front of a 1x1 in feedback mode': (
            '0:CBConv2d/p1i0 1:CBResize2d/p1c1 2:CBConv2d/p0i0',
            '0:CBConv2d/p1i0 1:CBResize2d/p1c0 2:CBConv2d/p0i0'),
        'in front of a dense module': (
            '0:CBConv2d/p1i0 1:CBResize2d/p0c1 2:Identity',
            '0:CBConv2d/p1i0 1:CBResize2d/p0c0 2:Identity'),
        'in front of a grouped convolution': (
            '0:CBConv2d/p1i0 1:CBResize2d/p0c1 2:CBGroupedConv2d/p0c1i0',
            '0:CBConv2d/p1i0 1:CBResize2d/p0c0 2:CBGroupedConv2d/p0c1i0'),
        'two in a row': (
            '0:CBConv2d/p1i0 1:CBResize2d/p1c1 2:CBResize2d/p1c1 3:CBConv2d/p0i0',
            '0:CBConv2d/p1i0 1:CBResize2d/p1c0 2:CBResize2d/p1c0 3:CBConv2d/p0i0'),
        'nested': (
            '0:Identity 1:Sequential 1.0:CBConv2d/p1i0 1.1:CBResize2d/p1c1 1.2:CBConv2d/p0i0 2:Upsample 3:Sequential 3.0:Sequential 3.0.0:CBConv2d/p1i0 3.0.1:CBResize2d/p0c1',
            '0:Identity 1:Sequential 1.0:CBConv2d/p1i0 1.1:CBResize2d/p1c0 1.2:CBConv2d/p0i0 2:Upsample 3:Sequential 3.0:Sequential 3.0.0:CBConv2d/p1i0 3.0.1:CBResize2d/p0c0'),
        'in a subclass of nn.Sequential': (
            '0:MySequential 0.0:CBConv2d/p0i0 0.1:Upsample 0.2:CBConv2d/p0i0',
            '0:MySequential 0.0:CBConv2d/p0i0 0.1:Upsample 0.2:CBConv2d/p0i0'),
        'beyond the limits': (
            '0:CBConv2d/p0i0 1:Upsample 2:CBConv2d/p0i0',
            '0:CBConv2d/p0i0 1:Upsample 2:CBConv2d/p0i0'),
        'a ReLU behind it': (
            '0:CBConv2d/p1i0 1:CBResize2d/p0c1 2:ReLU 3:CBConv2d/p0i0',
            '0:CBConv2d/p1i0 1:CBResize2d/p0c0 2:ReLU 3:CBConv2d/p0i0'),
        'a ReLU behind it, twice': (
            '0:CBConv2d/p1i0 1:CBResize2d/p0c1 2:ReLU 3:Upsample 4:ReLU 5:CBConv2d/p0i0',
            '0:CBConv2d/p1i0 1:CBResize2d/p0c0 2:ReLU 3:Upsample 4:ReLU 5:CBConv2d/p0i0'),
        'a batch norm and an activation behind it': (
            '0:CBConv2d/p0i0 1:BatchNorm2d 2:Upsample 3:CBConv2d/p0i0',
            '0:CBConv2d/p0i0 1:BatchNorm2d 2:Upsample 3:CBConv2d/p0i0'),
    },
    'insertCBPadding': {
        'behind CBConv2d': (
            '0:CBConv2d/p1i0 1:CBPad2d/p0c1 2:CBConv2d/p0i1',
            '0:CBConv2d/p1i0 1:CBPad2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBPoolMax2d 2x2': (
            '0:CBPoolMax2d/p1c1d1 1:CBPad2d/p0c1 2:CBConv2d/p0i1',
            '0:CBPoolMax2d/p1c1d1 1:CBPad2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBPoolMax2d 3x3': (
            '0:CBPoolMax2d/p1c1d0 1:CBPad2d/p0c1 2:CBConv2d/p0i1',
            '0:CBPoolMax2d/p1c1d0 1:CBPad2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBPoolAvg2d': (
            '0:CBPoolAvg2d/p1c1d0 1:CBPad2d/p0c1 2:CBConv2d/p0i1',
            '0:CBPoolAvg2d/p1c1d0 1:CBPad2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBAdd2d': (
            '0:CBAdd2d/p1c1 1:CBPad2d/p0c1 2:CBConv2d/p0i1',
            '0:CBAdd2d/p1c1 1:CBPad2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBResidual': (
            '0:CBResidual 0.body:Sequential 0.body.0:CBConv2d/p0i1 0.body.1:CBConv2d/p1i0 0.add:CBAdd2d/p1c1 1:CBPad2d/p0c1 2:CBConv2d/p0i1',
            '0:CBResidual 0.body:Sequential 0.body.0:CBConv2d/p0i1 0.body.1:CBConv2d/p1i0 0.add:CBAdd2d/p1c1 1:CBPad2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBUpsample2d': (
            '0:CBUpsample2d/p1c1 1:CBPad2d/p0c1 2:CBConv2d/p0i1',
            '0:CBUpsample2d/p1c1 1:CBPad2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBConvTranspose2d': (
            '0:CBConvTranspose2d/p1c1i1 1:CBPad2d/p0c1 2:CBConv2d/p0i1',
            '0:CBConvTranspose2d/p1c1i1 1:CBPad2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBDepthwiseConv2d': (
            '0:CBDepthwiseConv2d/p1c1i0 1:CBPad2d/p0c1 2:CBConv2d/p0i1',
            '0:CBDepthwiseConv2d/p1c1i0 1:CBPad2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBPointwise2d': (
            '0:CBPointwise2d/p1c1 1:CBPad2d/p0c1 2:CBConv2d/p0i1',
            '0:CBPointwise2d/p1c1 1:CBPad2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBPixelShuffle2d': (
            '0:CBPixelShuffle2d/p1c1 1:CBPad2d/p0c1 2:CBConv2d/p0i1',
            '0:CBPixelShuffle2d/p1c1 1:CBPad2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBChannelShuffle2d': (
            '0:CBChannelShuffle2d/p1c1 1:CBPad2d/p0c1 2:CBConv2d/p0i1',
            '0:CBChannelShuffle2d/p1c1 1:CBPad2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBResize2d': (
            '0:CBResize2d/p1c1 1:CBPad2d/p0c1 2:CBConv2d/p0i1',
            '0:CBResize2d/p1c1 1:CBPad2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBPad2d': (
            '0:CBPad2d/p1c1 1:CBPad2d/p0c1 2:CBConv2d/p0i1',
            '0:CBPad2d/p1c1 1:CBPad2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBBinary2d': (
            '0:CBBinary2d/p1c1 1:CBPad2d/p0c1 2:CBConv2d/p0i1',
            '0:CBBinary2d/p1c1 1:CBPad2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBGLU2d': (
            '0:CBGLU2d/p1c1 1:CBPad2d/p0c1 2:CBConv2d/p0i1',
            '0:CBGLU2d/p1c1 1:CBPad2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBGated': (
            '0:CBGated 0.body:Sequential 0.body.0:CBConv2d/p0i1 0.body.1:CBConv2d/p1i0 0.mul:CBBinary2d/p1c1 1:CBPad2d/p0c1 2:CBConv2d/p0i1',
            '0:CBGated 0.body:Sequential 0.body.0:CBConv2d/p0i1 0.body.1:CBConv2d/p1i0 0.mul:CBBinary2d/p1c1 1:CBPad2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBGroupedConv2d': (
            '0:CBGroupedConv2d/p1c1i0 1:CBPad2d/p0c1 2:CBConv2d/p0i1',
            '0:CBGroupedConv2d/p1c1i0 1:CBPad2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBChannelReduce2d': (
            '0:CBChannelReduce2d/p1c1 1:CBPad2d/p0c1 2:CBConv2d/p0i1',
            '0:CBChannelReduce2d/p1c1 1:CBPad2d/p0c0 2:CBConv2d/p0i1'),
        'behind dense': (
            '0:Identity 1:ReflectionPad2d 2:CBConv2d/p0i0',
            '0:Identity 1:ReflectionPad2d 2:CBConv2d/p0i0'),
        'at position 0': (
            '0:ReflectionPad2d 1:CBConv2d/p0i0',
            '0:ReflectionPad2d 1:CBConv2d/p0i0'),
        'the last child': (
            '0:CBConv2d/p1i0 1:CBPad2d/p0c1',
            '0:CBConv2d/p1i0 1:CBPad2d/p0c0'),
        'in front of a 1x1': (
            '0:CBConv2d/p1i0 1:CBPad2d/p1c1 2:CBConv2d/p0i0',
            '0:CBConv2d/p1i0 1:CBPad2d/p1c0 2:CBConv2d/p0i0'),
        'in front of a strided 1x1': (
            '0:CBConv2d/p1i0 1:CBPad2d/p0c1 2:CBConv2d/p0i1',
            '0:CBConv2d/p1i0 1:CBPad2d/p0c0 2:CBConv2d/p0i1'),
        'in front of a 3x3 in feedback mode': (
            '0:CBConv2d/p1i0 1:CBPad2d/p0c1 2:CBConv2d/p0i0',
            '0:CBConv2d/p1i0 1:CBPad2d/p0c0 2:CBConv2d/p0i0'),
        'in front of a 1x1 in feedback mode': (
            '0:CBConv2d/p1i0 1:CBPad2d/p1c1 2:CBConv2d/p0i0',
            '0:CBConv2d/p1i0 1:CBPad2d/p1c0 2:CBConv2d/p0i0'),
        'in front of a dense module': (
            '0:CBConv2d/p1i0 1:CBPad2d/p0c1 2:Identity',
            '0:CBConv2d/p1i0 1:CBPad2d/p0c0 2:Identity'),
        'in front of a grouped convolution': (
            '0:CBConv2d/p1i0 1:CBPad2d/p0c1 2:CBGroupedConv2d/p0c1i0',
            '0:CBConv2d/p1i0 1:CBPad2d/p0c0 2:CBGroupedConv2d/p0c1i0'),
        'two in a row': (
            '0:CBConv2d/p1i0 1:CBPad2d/p1c1 2:CBPad2d/p1c1 3:CBConv2d/p0i0',
            '0:CBConv2d/p1i0 1:CBPad2d/p1c0 2:CBPad2d/p1c0 3:CBConv2d/p0i0'),
        'nested': (
            '0:Identity 1:Sequential 1.0:CBConv2d/p1i0 1.1:CBPad2d/p1c1 1.2:CBConv2d/p0i0 2:ReflectionPad2d 3:Sequential 3.0:Sequential 3.0.0:CBConv2d/p1i0 3.0.1:CBPad2d/p0c1',
            '0:Identity 1:Sequential 1.0:CBConv2d/p1i0 1.1:CBPad2d/p1c0 1.2:CBConv2d/p0i0 2:ReflectionPad2d 3:Sequential 3.0:Sequential 3.0.0:CBConv2d/p1i0 3.0.1:CBPad2d/p0c0'),
        'in a subclass of nn.Sequential': (
            '0:MySequential 0.0:CBConv2d/p0i0 0.1:ReflectionPad2d 0.2:CBConv2d/p0i0',
            '0:MySequential 0.0:CBConv2d/p0i0 0.1:ReflectionPad2d 0.2:CBConv2d/p0i0'),
        'beyond the limits': (
            '0:CBConv2d/p0i0 1:ZeroPad2d 2:CBConv2d/p0i0',
            '0:CBConv2d/p0i0 1:ZeroPad2d 2:CBConv2d/p0i0'),
        'a ReLU behind it': (
            '0:CBConv2d/p1i0 1:CBPad2d/p0c1 2:ReLU 3:CBConv2d/p0i0',
            '0:CBConv2d/p1i0 1:CBPad2d/p0c0 2:ReLU 3:CBConv2d/p0i0'),
        'a ReLU behind it, twice': (
            '0:CBConv2d/p1i0 1:CBPad2d/p0c1 2:ReLU 3:ReflectionPad2d 4:ReLU 5:CBConv2d/p0i0',
            '0:CBConv2d/p1i0 1:CBPad2d/p0c0 2:ReLU 3:ReflectionPad2d 4:ReLU 5:CBConv2d/p0i0'),
        'a batch norm and an activation behind it': (
            '0:CBConv2d/p0i0 1:BatchNorm2d 2:ReflectionPad2d 3:CBConv2d/p0i0',
            '0:CBConv2d/p0i0 1:BatchNorm2d 2:ReflectionPad2d 3:CBConv2d/p0i0'),
    },
    'insertCBGating': {
        'behind CBConv2d': (
            '0:CBConv2d/p1i0 1:CBGLU2d/p0c1 2:CBConv2d/p0i1',
            '0:CBConv2d/p1i0 1:CBGLU2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBPoolMax2d 2x2': (
            '0:CBPoolMax2d/p1c1d1 1:CBGLU2d/p0c1 2:CBConv2d/p0i1',
            '0:CBPoolMax2d/p1c1d1 1:CBGLU2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBPoolMax2d 3x3': (
            '0:CBPoolMax2d/p1c1d0 1:CBGLU2d/p0c1 2:CBConv2d/p0i1',
            '0:CBPoolMax2d/p1c1d0 1:CBGLU2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBPoolAvg2d': (
            '0:CBPoolAvg2d/p1c1d0 1:CBGLU2d/p0c1 2:CBConv2d/p0i1',
            '0:CBPoolAvg2d/p1c1d0 1:CBGLU2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBAdd2d': (
            '0:CBAdd2d/p1c1 1:CBGLU2d/p0c1 2:CBConv2d/p0i1',
            '0:CBAdd2d/p1c1 1:CBGLU2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBResidual': (
            '0:CBResidual 0.body:Sequential 0.body.0:CBConv2d/p0i1 0.body.1:CBConv2d/p1i0 0.add:CBAdd2d/p1c1 1:CBGLU2d/p0c1 2:CBConv2d/p0i1',
            '0:CBResidual 0.body:Sequential 0.body.0:CBConv2d/p0i1 0.body.1:CBConv2d/p1i0 0.add:CBAdd2d/p1c1 1:CBGLU2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBUpsample2d': (
            '0:CBUpsample2d/p1c1 1:CBGLU2d/p0c1 2:CBConv2d/p0i1',
            '0:CBUpsample2d/p1c1 1:CBGLU2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBConvTranspose2d': (
            '0:CBConvTranspose2d/p1c1i1 1:CBGLU2d/p0c1 2:CBConv2d/p0i1',
            '0:CBConvTranspose2d/p1c1i1 1:CBGLU2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBDepthwiseConv2d': (
            '0:CBDepthwiseConv2d/p1c1i0 1:CBGLU2d/p0c1 2:CBConv2d/p0i1',
            '0:CBDepthwiseConv2d/p1c1i0 1:CBGLU2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBPointwise2d': (
            '0:CBPointwise2d/p1c1 1:CBGLU2d/p0c1 2:CBConv2d/p0i1',
            '0:CBPointwise2d/p1c1 1:CBGLU2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBPixelShuffle2d': (
            '0:CBPixelShuffle2d/p1c1 1:CBGLU2d/p0c1 2:CBConv2d/p0i1',
            '0:CBPixelShuffle2d/p1c1 1:CBGLU2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBChannelShuffle2d': (
            '0:CBChannelShuffle2d/p1c1 1:CBGLU2d/p0c1 2:CBConv2d/p0i1',
            '0:CBChannelShuffle2d/p1c1 1:CBGLU2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBResize2d': (
            '0:CBResize2d/p1c1 1:CBGLU2d/p0c1 2:CBConv2d/p0i1',
            '0:CBResize2d/p1c1 1:CBGLU2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBPad2d': (
            '0:CBPad2d/p1c1 1:CBGLU2d/p0c1 2:CBConv2d/p0i1',
            '0:CBPad2d/p1c1 1:CBGLU2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBBinary2d': (
            '0:CBBinary2d/p1c1 1:CBGLU2d/p0c1 2:CBConv2d/p0i1',
            '0:CBBinary2d/p1c1 1:CBGLU2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBGLU2d': (
            '0:CBGLU2d/p1c1 1:CBGLU2d/p0c1 2:CBConv2d/p0i1',
            '0:CBGLU2d/p1c1 1:CBGLU2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBGated': (
            '0:CBGated 0.body:Sequential 0.body.0:CBConv2d/p0i1 0.body.1:CBConv2d/p1i0 0.mul:CBBinary2d/p1c1 1:CBGLU2d/p0c1 2:CBConv2d/p0i1',
            '0:CBGated 0.body:Sequential 0.body.0:CBConv2d/p0i1 0.body.1:CBConv2d/p1i0 0.mul:CBBinary2d/p1c1 1:CBGLU2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBGroupedConv2d': (
            '0:CBGroupedConv2d/p1c1i0 1:CBGLU2d/p0c1 2:CBConv2d/p0i1',
            '0:CBGroupedConv2d/p1c1i0 1:CBGLU2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBChannelReduce2d': (
            '0:CBChannelReduce2d/p1c1 1:CBGLU2d/p0c1 2:CBConv2d/p0i1',
            '0:CBChannelReduce2d/p1c1 1:CBGLU2d/p0c0 2:CBConv2d/p0i1'),
        'behind dense': (
            '0:Identity 1:GLU 2:CBConv2d/p0i0',
            '0:Identity 1:GLU 2:CBConv2d/p0i0'),
        'at position 0': (
            '0:GLU 1:CBConv2d/p0i0',
            '0:GLU 1:CBConv2d/p0i0'),
        'the last child': (
            '0:CBConv2d/p1i0 1:CBGLU2d/p0c1',
            '0:CBConv2d/p1i0 1:CBGLU2d/p0c0'),
        'in front of a 1x1': (
            '0:CBConv2d/p1i0 1:CBGLU2d/p1c1 2:CBConv2d/p0i0',
            '0:CBConv2d/p1i0 1:CBGLU2d/p1c0 2:CBConv2d/p0i0'),
        'in front of a strided 1x1': (
            '0:CBConv2d/p1i0 1:CBGLU2d/p0c1 2:CBConv2d/p0i1',
            '0:CBConv2d/p1i0 1:CBGLU2d/p0c0 2:CBConv2d/p0i1'),
        'in front of a 3x3 in feedback mode': (
            '0:CBConv2d/p1i0 1:CBGLU2d/p0c1 2:CBConv2d/p0i0',
            '0:CBConv2d/p1i0 1:CBGLU2d/p0c0 2:CBConv2d/p0i0'),
        'in front of a 1x1 in feedback mode': (
            '0:CBConv2d/p1i0 1:CBGLU2d/p1c1 2:CBConv2d/p0i0',
            '0:CBConv2d/p1i0 1:CBGLU2d/p1c0 2:CBConv2d/p0i0'),
        'in front of a dense module': (
            '0:CBConv2d/p1i0 1:CBGLU2d/p0c1 2:Identity',
            '0:CBConv2d/p1i0 1:CBGLU2d/p0c0 2:Identity'),
        'in front of a grouped convolution': (
            '0:CBConv2d/p1i0 1:CBGLU2d/p0c1 2:CBGroupedConv2d/p0c1i0',
            '0:CBConv2d/p1i0 1:CBGLU2d/p0c0 2:CBGroupedConv2d/p0c1i0'),
        'two in a row': (
            '0:CBConv2d/p1i0 1:CBGLU2d/p1c1 2:CBGLU2d/p1c1 3:CBConv2d/p0i0',
            '0:CBConv2d/p1i0 1:CBGLU2d/p1c0 2:CBGLU2d/p1c0 3:CBConv2d/p0i0'),
        'nested': (
            '0:Identity 1:Sequential 1.0:CBConv2d/p1i0 1.1:CBGLU2d/p1c1 1.2:CBConv2d/p0i0 2:GLU 3:Sequential 3.0:Sequential 3.0.0:CBConv2d/p1i0 3.0.1:CBGLU2d/p0c1',
            '0:Identity 1:Sequential 1.0:CBConv2d/p1i0 1.1:CBGLU2d/p1c0 1.2:CBConv2d/p0i0 2:GLU 3:Sequential 3.0:Sequential 3.0.0:CBConv2d/p1i0 3.0.1:CBGLU2d/p0c0'),
        'in a subclass of nn.Sequential': (
            '0:MySequential 0.0:CBConv2d/p0i0 0.1:GLU 0.2:CBConv2d/p0i0',
            '0:MySequential 0.0:CBConv2d/p0i0 0.1:GLU 0.2:CBConv2d/p0i0'),
        'beyond the limits': (
            '0:CBConv2d/p0i0 1:GLU 2:CBConv2d/p0i0',
            '0:CBConv2d/p0i0 1:GLU 2:CBConv2d/p0i0'),
        'a ReLU behind it': (
            '0:CBConv2d/p1i0 1:CBGLU2d/p0c1 2:ReLU 3:CBConv2d/p0i0',
            '0:CBConv2d/p1i0 1:CBGLU2d/p0c0 2:ReLU 3:CBConv2d/p0i0'),
        'a ReLU behind it, twice': (
            '0:CBConv2d/p1i0 1:CBGLU2d/p0c1 2:ReLU 3:GLU 4:ReLU 5:CBConv2d/p0i0',
            '0:CBConv2d/p1i0 1:CBGLU2d/p0c0 2:ReLU 3:GLU 4:ReLU 5:CBConv2d/p0i0'),
        'a batch norm and an activation behind it': (
            '0:CBConv2d/p0i0 1:BatchNorm2d 2:GLU 3:CBConv2d/p0i0',
            '0:CBConv2d/p0i0 1:BatchNorm2d 2:GLU 3:CBConv2d/p0i0'),
    },
    'insertCBUpsampling': {
        'behind CBConv2d': (
            '0:CBConv2d/p1i0 1:CBUpsample2d/p0c1 2:CBConv2d/p0i1',
            '0:CBConv2d/p1i0 1:CBUpsample2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBPoolMax2d 2x2': (
            '0:CBPoolMax2d/p1c1d1 1:CBUpsample2d/p0c1 2:CBConv2d/p0i1',
            '0:CBPoolMax2d/p1c1d1 1:CBUpsample2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBPoolMax2d 3x3': (
            '0:CBPoolMax2d/p1c1d0 1:CBUpsample2d/p0c1 2:CBConv2d/p0i1',
            '0:CBPoolMax2d/p1c1d0 1:CBUpsample2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBPoolAvg2d': (
            '0:CBPoolAvg2d/p1c1d0 1:CBUpsample2d/p0c1 2:CBConv2d/p0i1',
            '0:CBPoolAvg2d/p1c1d0 1:CBUpsample2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBAdd2d': (
            '0:CBAdd2d/p1c1 1:CBUpsample2d/p0c1 2:CBConv2d/p0i1',
            '0:CBAdd2d/p1c1 1:CBUpsample2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBResidual': (
            '0:CBResidual 0.body:Sequential 0.body.0:CBConv2d/p0i1 0.body.1:CBConv2d/p1i0 0.add:CBAdd2d/p1c1 1:CBUpsample2d/p0c1 2:CBConv2d/p0i1',
            '0:CBResidual 0.body:Sequential 0.body.0:CBConv2d/p0i1 0.body.1:CBConv2d/p1i0 0.add:CBAdd2d/p1c1 1:CBUpsample2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBUpsample2d': (
            '0:CBUpsample2d/p1c1 1:CBUpsample2d/p0c1 2:CBConv2d/p0i1',
            '0:CBUpsample2d/p1c1 1:CBUpsample2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBConvTranspose2d': (
            '0:CBConvTranspose2d/p0c1i1 1:Upsample 2:CBConv2d/p0i0',
            '0:CBConvTranspose2d/p0c1i1 1:Upsample 2:CBConv2d/p0i0'),
        'behind CBDepthwiseConv2d': (
            '0:CBDepthwiseConv2d/p1c1i0 1:CBUpsample2d/p0c1 2:CBConv2d/p0i1',
            '0:CBDepthwiseConv2d/p1c1i0 1:CBUpsample2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBPointwise2d': (
            '0:CBPointwise2d/p1c1 1:CBUpsample2d/p0c1 2:CBConv2d/p0i1',
            '0:CBPointwise2d/p1c1 1:CBUpsample2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBPixelShuffle2d': (
            '0:CBPixelShuffle2d/p1c1 1:CBUpsample2d/p0c1 2:CBConv2d/p0i1',
            '0:CBPixelShuffle2d/p1c1 1:CBUpsample2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBChannelShuffle2d': (
            '0:CBChannelShuffle2d/p1c1 1:CBUpsample2d/p0c1 2:CBConv2d/p0i1',
            '0:CBChannelShuffle2d/p1c1 1:CBUpsample2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBResize2d': (
            '0:CBResize2d/p1c1 1:CBUpsample2d/p0c1 2:CBConv2d/p0i1',
            '0:CBResize2d/p1c1 1:CBUpsample2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBPad2d': (
            '0:CBPad2d/p1c1 1:CBUpsample2d/p0c1 2:CBConv2d/p0i1',
            '0:CBPad2d/p1c1 1:CBUpsample2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBBinary2d': (
            '0:CBBinary2d/p1c1 1:CBUpsample2d/p0c1 2:CBConv2d/p0i1',
            '0:CBBinary2d/p1c1 1:CBUpsample2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBGLU2d': (
            '0:CBGLU2d/p1c1 1:CBUpsample2d/p0c1 2:CBConv2d/p0i1',
            '0:CBGLU2d/p1c1 1:CBUpsample2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBGated': (
            '0:CBGated 0.body:Sequential 0.body.0:CBConv2d/p0i1 0.body.1:CBConv2d/p1i0 0.mul:CBBinary2d/p1c1 1:CBUpsample2d/p0c1 2:CBConv2d/p0i1',
            '0:CBGated 0.body:Sequential 0.body.0:CBConv2d/p0i1 0.body.1:CBConv2d/p1i0 0.mul:CBBinary2d/p1c1 1:CBUpsample2d/p0c0 2:CBConv2d/p0i1'),
        'behind CBGroupedConv2d': (
            '0:CBGroupedConv2d/p0c1i0 1:Upsample 2:CBConv2d/p0i0',
            '0:CBGroupedConv2d/p0c1i0 1:Upsample 2:CBConv2d/p0i0'),
        'behind CBChannelReduce2d': (
            '0:CBChannelReduce2d/p0c1 1:Upsample 2:CBConv2d/p0i0',
            '0:CBChannelReduce2d/p0c1 1:Upsample 2:CBConv2d/p0i0'),
        'behind dense': (
            '0:Identity 1:Upsample 2:CBConv2d/p0i0',
            '0:Identity 1:Upsample 2:CBConv2d/p0i0'),
        'at position 0': (
            '0:Upsample 1:CBConv2d/p0i0',
            '0:Upsample 1:CBConv2d/p0i0'),
        'the last child': (
            '0:CBConv2d/p1i0 1:CBUpsample2d/p0c1',
            '0:CBConv2d/p1i0 1:CBUpsample2d/p0c0'),
        'in front of a 1x1': (
            '0:CBConv2d/p1i0 1:CBUpsample2d/p0c1 2:CBConv2d/p0i1',
            '0:CBConv2d/p1i0 1:CBUpsample2d/p0c0 2:CBConv2d/p0i1'),
        'in front of a strided 1x1': (
            '0:CBConv2d/p1i0 1:CBUpsample2d/p0c1 2:CBConv2d/p0i1',
            '0:CBConv2d/p1i0 1:CBUpsample2d/p0c0 2:CBConv2d/p0i1'),
        'in front of a 3x3 in feedback mode': (
            '0:CBConv2d/p1i0 1:CBUpsample2d/p0c1 2:CBConv2d/p0i0',
            '0:CBConv2d/p1i0 1:CBUpsample2d/p0c0 2:CBConv2d/p0i0'),
        'in front of a 1x1 in feedback mode': (
            '0:CBConv2d/p1i0 1:CBUpsample2d/p0c1 2:CBConv2d/p0i0',
            '0:CBConv2d/p1i0 1:CBUpsample2d/p0c0 2:CBConv2d/p0i0'),
        'in front of a dense module': (
            '0:CBConv2d/p1i0 1:CBUpsample2d/p0c1 2:Identity',
            '0:CBConv2d/p1i0 1:CBUpsample2d/p0c0 2:Identity'),
        'in front of a grouped convolution': (
            '0:CBConv2d/p1i0 1:CBUpsample2d/p0c1 2:CBGroupedConv2d/p0c1i0',
            '0:CBConv2d/p1i0 1:CBUpsample2d/p0c0 2:CBGroupedConv2d/p0c1i0'),
        'two in a row': (
            '0:CBConv2d/p1i0 1:CBUpsample2d/p1c1 2:CBUpsample2d/p0c1 3:CBConv2d/p0i1',
            '0:CBConv2d/p1i0 1:CBUpsample2d/p1c0 2:CBUpsample2d/p0c0 3:CBConv2d/p0i1'),
        'nested': (
            '0:Identity 1:Sequential 1.0:CBConv2d/p1i0 1.1:CBUpsample2d/p0c1 1.2:CBConv2d/p0i1 2:Upsample 3:Sequential 3.0:Sequential 3.0.0:CBConv2d/p1i0 3.0.1:CBUpsample2d/p0c1',
            '0:Identity 1:Sequential 1.0:CBConv2d/p1i0 1.1:CBUpsample2d/p0c0 1.2:CBConv2d/p0i1 2:Upsample 3:Sequential 3.0:Sequential 3.0.0:CBConv2d/p1i0 3.0.1:CBUpsample2d/p0c0'),
        'in a subclass of nn.Sequential': (
            '0:MySequential 0.0:CBConv2d/p0i0 0.1:Upsample 0.2:CBConv2d/p0i0',
            '0:MySequential 0.0:CBConv2d/p0i0 0.1:Upsample 0.2:CBConv2d/p0i0'),
        'beyond the limits': (
            '0:CBConv2d/p0i0 1:Upsample 2:CBConv2d/p0i0',
            '0:CBConv2d/p0i0 1:Upsample 2:CBConv2d/p0i0'),
        'a ReLU behind it': (
            '0:CBConv2d/p1i0 1:CBUpsample2d/p0c1 2:ReLU 3:CBConv2d/p0i0',
            '0:CBConv2d/p1i0 1:CBUpsample2d/p0c0 2:ReLU 3:CBConv2d/p0i0'),
        'a ReLU behind it, twice': (
            '0:CBConv2d/p1i0 1:CBUpsample2d/p0c1 2:ReLU 3:Upsample 4:ReLU 5:CBConv2d/p0i0',
            '0:CBConv2d/p1i0 1:CBUpsample2d/p0c0 2:ReLU 3:Upsample 4:ReLU 5:CBConv2d/p0i0'),
        'a batch norm and an activation behind it': (
            '0:CBConv2d/p0i0 1:BatchNorm2d 2:Upsample 3:CBConv2d/p0i0',
            '0:CBConv2d/p0i0 1:BatchNorm2d 2:Upsample 3:CBConv2d/p0i0'),
    },
    'insertCBTransposedConv': {
        'behind CBConv2d': (
            '0:CBConv2d/p0i0 1:CBConvTranspose2d/p0c1i1 2:CBConv2d/p0i1',
            '0:CBConv2d/p0i0 1:CBConvTranspose2d/p0c0i1 2:CBConv2d/p0i1'),
        'behind CBPoolMax2d 2x2': (
            '0:CBPoolMax2d/p0c1d0 1:CBConvTranspose2d/p0c1i1 2:CBConv2d/p0i1',
            '0:CBPoolMax2d/p0c1d0 1:CBConvTranspose2d/p0c0i1 2:CBConv2d/p0i1'),
        'behind CBPoolMax2d 3x3': (
            '0:CBPoolMax2d/p0c1d0 1:CBConvTranspose2d/p0c1i1 2:CBConv2d/p0i1',
            '0:CBPoolMax2d/p0c1d0 1:CBConvTranspose2d/p0c0i1 2:CBConv2d/p0i1'),
        'behind CBPoolAvg2d': (
            '0:CBPoolAvg2d/p0c1d0 1:CBConvTranspose2d/p0c1i1 2:CBConv2d/p0i1',
            '0:CBPoolAvg2d/p0c1d0 1:CBConvTranspose2d/p0c0i1 2:CBConv2d/p0i1'),
        'behind CBAdd2d': (
            '0:CBAdd2d/p0c1 1:CBConvTranspose2d/p0c1i1 2:CBConv2d/p0i1',
            '0:CBAdd2d/p0c1 1:CBConvTranspose2d/p0c0i1 2:CBConv2d/p0i1'),
        'behind CBResidual': (
            '0:CBResidual 0.body:Sequential 0.body.0:CBConv2d/p0i1 0.body.1:CBConv2d/p1i0 0.add:CBAdd2d/p0c1 1:CBConvTranspose2d/p0c1i1 2:CBConv2d/p0i1',
            '0:CBResidual 0.body:Sequential 0.body.0:CBConv2d/p0i1 0.body.1:CBConv2d/p1i0 0.add:CBAdd2d/p0c1 1:CBConvTranspose2d/p0c0i1 2:CBConv2d/p0i1'),
        'behind CBUpsample2d': (
            '0:CBUpsample2d/p0c1 1:CBConvTranspose2d/p0c1i1 2:CBConv2d/p0i1',
            '0:CBUpsample2d/p0c1 1:CBConvTranspose2d/p0c0i1 2:CBConv2d/p0i1'),
        'behind CBConvTranspose2d': (
            '0:CBConvTranspose2d/p0c1i1 1:CBConvTranspose2d/p0c1i1 2:CBConv2d/p0i1',
            '0:CBConvTranspose2d/p0c1i1 1:CBConvTranspose2d/p0c0i1 2:CBConv2d/p0i1'),
        'behind CBDepthwiseConv2d': (
            '0:CBDepthwiseConv2d/p0c1i0 1:CBConvTranspose2d/p0c1i1 2:CBConv2d/p0i1',
            '0:CBDepthwiseConv2d/p0c1i0 1:CBConvTranspose2d/p0c0i1 2:CBConv2d/p0i1'),
        'behind CBPointwise2d': (
            '0:CBPointwise2d/p0c1 1:CBConvTranspose2d/p0c1i1 2:CBConv2d/p0i1',
            '0:CBPointwise2d/p0c1 1:CBConvTranspose2d/p0c0i1 2:CBConv2d/p0i1'),
        'behind CBPixelShuffle2d': (
            '0:CBPixelShuffle2d/p0c1 1:CBConvTranspose2d/p0c1i1 2:CBConv2d/p0i1',
            '0:CBPixelShuffle2d/p0c1 1:CBConvTranspose2d/p0c0i1 2:CBConv2d/p0i1'),
        'behind CBChannelShuffle2d': (
            '0:CBChannelShuffle2d/p0c1 1:CBConvTranspose2d/p0c1i1 2:CBConv2d/p0i1',
            '0:CBChannelShuffle2d/p0c1 1:CBConvTranspose2d/p0c0i1 2:CBConv2d/p0i1'),
        'behind CBResize2d': (
            '0:CBResize2d/p0c1 1:CBConvTranspose2d/p0c1i1 2:CBConv2d/p0i1',
            '0:CBResize2d/p0c1 1:CBConvTranspose2d/p0c0i1 2:CBConv2d/p0i1'),
        'behind CBPad2d': (
            '0:CBPad2d/p0c1 1:CBConvTranspose2d/p0c1i1 2:CBConv2d/p0i1',
            '0:CBPad2d/p0c1 1:CBConvTranspose2d/p0c0i1 2:CBConv2d/p0i1'),
        'behind CBBinary2d': (
            '0:CBBinary2d/p0c1 1:CBConvTranspose2d/p0c1i1 2:CBConv2d/p0i1',
            '0:CBBinary2d/p0c1 1:CBConvTranspose2d/p0c0i1 2:CBConv2d/p0i1'),
        'behind CBGLU2d': (
            '0:CBGLU2d/p0c1 1:CBConvTranspose2d/p0c1i1 2:CBConv2d/p0i1',
            '0:CBGLU2d/p0c1 1:CBConvTranspose2d/p0c0i1 2:CBConv2d/p0i1'),
        'behind CBGated': (
            '0:CBGated 0.body:Sequential 0.body.0:CBConv2d/p0i1 0.body.1:CBConv2d/p1i0 0.mul:CBBinary2d/p0c1 1:CBConvTranspose2d/p0c1i1 2:CBConv2d/p0i1',
            '0:CBGated 0.body:Sequential 0.body.0:CBConv2d/p0i1 0.body.1:CBConv2d/p1i0 0.mul:CBBinary2d/p0c1 1:CBConvTranspose2d/p0c0i1 2:CBConv2d/p0i1'),
        'behind CBGroupedConv2d': (
            '0:CBGroupedConv2d/p0c1i0 1:ConvTranspose2d 2:CBConv2d/p0i0',
            '0:CBGroupedConv2d/p0c1i0 1:ConvTranspose2d 2:CBConv2d/p0i0'),
        'behind CBChannelReduce2d': (
            '0:CBChannelReduce2d/p0c1 1:ConvTranspose2d 2:CBConv2d/p0i0',
            '0:CBChannelReduce2d/p0c1 1:ConvTranspose2d 2:CBConv2d/p0i0'),
        'behind dense': (
            '0:Identity 1:ConvTranspose2d 2:CBConv2d/p0i0',
            '0:Identity 1:ConvTranspose2d 2:CBConv2d/p0i0'),
        'at position 0': (
            '0:ConvTranspose2d 1:CBConv2d/p0i0',
            '0:ConvTranspose2d 1:CBConv2d/p0i0'),
        'the last child': (
            '0:CBConv2d/p0i0 1:CBConvTranspose2d/p0c1i1',
            '0:CBConv2d/p0i0 1:CBConvTranspose2d/p0c0i1'),
        'in front of a 1x1': (
            '0:CBConv2d/p0i0 1:CBConvTranspose2d/p0c1i1 2:CBConv2d/p0i1',
            '0:CBConv2d/p0i0 1:CBConvTranspose2d/p0c0i1 2:CBConv2d/p0i1'),
        'in front of a strided 1x1': (
            '0:CBConv2d/p0i0 1:CBConvTranspose2d/p0c1i1 2:CBConv2d/p0i1',
            '0:CBConv2d/p0i0 1:CBConvTranspose2d/p0c0i1 2:CBConv2d/p0i1'),
        'in front of a 3x3 in feedback mode': (
            '0:CBConv2d/p0i0 1:CBConvTranspose2d/p0c1i1 2:CBConv2d/p0i0',
            '0:CBConv2d/p0i0 1:CBConvTranspose2d/p0c0i1 2:CBConv2d/p0i0'),
        'in front of a 1x1 in feedback mode': (
            '0:CBConv2d/p0i0 1:CBConvTranspose2d/p0c1i1 2:CBConv2d/p0i0',
            '0:CBConv2d/p0i0 1:CBConvTranspose2d/p0c0i1 2:CBConv2d/p0i0'),
        'in front of a dense module': (
            '0:CBConv2d/p0i0 1:CBConvTranspose2d/p0c1i1 2:Identity',
            '0:CBConv2d/p0i0 1:CBConvTranspose2d/p0c0i1 2:Identity'),
        'in front of a grouped convolution': (
            '0:CBConv2d/p0i0 1:CBConvTranspose2d/p0c1i1 2:CBGroupedConv2d/p0c1i0',
            '0:CBConv2d/p0i0 1:CBConvTranspose2d/p0c0i1 2:CBGroupedConv2d/p0c1i0'),
        'two in a row': (
            '0:CBConv2d/p0i0 1:CBConvTranspose2d/p0c1i1 2:CBConvTranspose2d/p0c1i1 3:CBConv2d/p0i1',
            '0:CBConv2d/p0i0 1:CBConvTranspose2d/p0c0i1 2:CBConvTranspose2d/p0c0i1 3:CBConv2d/p0i1'),
        'nested': (
            '0:Identity 1:Sequential 1.0:CBConv2d/p0i0 1.1:CBConvTranspose2d/p0c1i1 1.2:CBConv2d/p0i1 2:ConvTranspose2d 3:Sequential 3.0:Sequential 3.0.0:CBConv2d/p0i0 3.0.1:CBConvTranspose2d/p0c1i1',
            '0:Identity 1:Sequential 1.0:CBConv2d/p0i0 1.1:CBConvTranspose2d/p0c0i1 1.2:CBConv2d/p0i1 2:ConvTranspose2d 3:Sequential 3.0:Sequential 3.0.0:CBConv2d/p0i0 3.0.1:CBConvTranspose2d/p0c0i1'),
        'in a subclass of nn.Sequential': (
            '0:MySequential 0.0:CBConv2d/p0i0 0.1:ConvTranspose2d 0.2:CBConv2d/p0i0',
            '0:MySequential 0.0:CBConv2d/p0i0 0.1:ConvTranspose2d 0.2:CBConv2d/p0i0'),
        'beyond the limits': (
            '0:CBConv2d/p0i0 1:ConvTranspose2d 2:CBConv2d/p0i0',
            '0:CBConv2d/p0i0 1:ConvTranspose2d 2:CBConv2d/p0i0'),
        'a ReLU behind it': (
            '0:CBConv2d/p0i0 1:CBConvTranspose2d/p0c1i1 3:CBConv2d/p0i1',
            '0:CBConv2d/p0i0 1:CBConvTranspose2d/p0c0i1 3:CBConv2d/p0i1'),
        'a ReLU behind it, twice': (
            '0:CBConv2d/p0i0 1:CBConvTranspose2d/p0c1i1 3:CBConvTranspose2d/p0c1i1 5:CBConv2d/p0i1',
            '0:CBConv2d/p0i0 1:CBConvTranspose2d/p0c0i1 3:CBConvTranspose2d/p0c0i1 5:CBConv2d/p0i1'),
        'a batch norm and an activation behind it': (
            '0:CBConv2d/p0i0 1:BatchNorm2d 2:ConvTranspose2d 3:CBConv2d/p0i0',
            '0:CBConv2d/p0i0 1:BatchNorm2d 2:ConvTranspose2d 3:CBConv2d/p0i0'),
    },
    'insertCBPointwise': {
        'behind CBConv2d': (
            '0:CBConv2d/p1i0 1:CBPointwise2d/p0c1 2:CBConv2d/p0i0',
            None),
        'behind CBPoolMax2d 2x2': (
            '0:CBPoolMax2d/p1c1d1 1:CBPointwise2d/p0c1 2:CBConv2d/p0i0',
            None),
        'behind CBPoolMax2d 3x3': (
            '0:CBPoolMax2d/p1c1d0 1:CBPointwise2d/p0c1 2:CBConv2d/p0i0',
            None),
        'behind CBPoolAvg2d': (
            '0:CBPoolAvg2d/p1c1d0 1:CBPointwise2d/p0c1 2:CBConv2d/p0i0',
            None),
        'behind CBAdd2d': (
            '0:CBAdd2d/p1c1 1:CBPointwise2d/p0c1 2:CBConv2d/p0i0',
            None),
        'behind CBResidual': (
            '0:CBResidual 0.body:Sequential 0.body.0:CBConv2d/p0i1 0.body.1:CBConv2d/p1i0 0.add:CBAdd2d/p1c1 1:CBPointwise2d/p0c1 2:CBConv2d/p0i0',
            None),
        'behind CBUpsample2d': (
            '0:CBUpsample2d/p1c1 1:CBPointwise2d/p0c1 2:CBConv2d/p0i0',
            None),
        'behind CBConvTranspose2d': (
            '0:CBConvTranspose2d/p1c1i1 1:CBPointwise2d/p0c1 2:CBConv2d/p0i0',
            None),
        'behind CBDepthwiseConv2d': (
            '0:CBDepthwiseConv2d/p1c1i0 1:CBPointwise2d/p0c1 2:CBConv2d/p0i0',
            None),
        'behind CBPointwise2d': (
            '0:CBPointwise2d/p1c1 1:CBPointwise2d/p0c1 2:CBConv2d/p0i0',
            None),
        'behind CBPixelShuffle2d': (
            '0:CBPixelShuffle2d/p1c1 1:CBPointwise2d/p0c1 2:CBConv2d/p0i0',
            None),
        'behind CBChannelShuffle2d': (
            '0:CBChannelShuffle2d/p1c1 1:CBPointwise2d/p0c1 2:CBConv2d/p0i0',
            None),
        'behind CBResize2d': (
            '0:CBResize2d/p1c1 1:CBPointwise2d/p0c1 2:CBConv2d/p0i0',
            None),
        'behind CBPad2d': (
            '0:CBPad2d/p1c1 1:CBPointwise2d/p0c1 2:CBConv2d/p0i0',
            None),
        'behind CBBinary2d': (
            '0:CBBinary2d/p1c1 1:CBPointwise2d/p0c1 2:CBConv2d/p0i0',
            None),
        'behind CBGLU2d': (
            '0:CBGLU2d/p1c1 1:CBPointwise2d/p0c1 2:CBConv2d/p0i0',
            None),
        'behind CBGated': (
            '0:CBGated 0.body:Sequential 0.body.0:CBConv2d/p0i1 0.body.1:CBConv2d/p1i0 0.mul:CBBinary2d/p1c1 1:CBPointwise2d/p0c1 2:CBConv2d/p0i0',
            None),
        'behind CBGroupedConv2d': (
            '0:CBGroupedConv2d/p0c1i0 1:Tanh 2:CBConv2d/p0i0',
            None),
        'behind CBChannelReduce2d': (
            '0:CBChannelReduce2d/p0c1 1:Tanh 2:CBConv2d/p0i0',
            None),
        'behind dense': (
            '0:Identity 1:Tanh 2:CBConv2d/p0i0',
            None),
        'at position 0': (
            '0:Tanh 1:CBConv2d/p0i0',
            None),
        'the last child': (
            '0:CBConv2d/p1i0 1:CBPointwise2d/p0c1',
            None),
        'in front of a 1x1': (
            '0:CBConv2d/p1i0 1:CBPointwise2d/p1c1 2:CBConv2d/p0i0',
            None),
        'in front of a strided 1x1': (
            '0:CBConv2d/p1i0 1:CBPointwise2d/p0c1 2:CBConv2d/p0i0',
            None),
        'in front of a 3x3 in feedback mode': (
            '0:CBConv2d/p1i0 1:CBPointwise2d/p0c1 2:CBConv2d/p0i0',
            None),
        'in front of a 1x1 in feedback mode': (
            '0:CBConv2d/p1i0 1:CBPointwise2d/p1c1 2:CBConv2d/p0i0',
            None),
        'in front of a dense module': (
            '0:CBConv2d/p1i0 1:CBPointwise2d/p0c1 2:Identity',
            None),
        'in front of a grouped convolution': (
            '0:CBConv2d/p1i0 1:CBPointwise2d/p0c1 2:CBGroupedConv2d/p0c1i0',
            None),
        'two in a row': (
            '0:CBConv2d/p1i0 1:CBPointwise2d/p1c1 2:CBPointwise2d/p1c1 3:CBConv2d/p0i0',
            None),
        'nested': (
            '0:Identity 1:Sequential 1.0:CBConv2d/p1i0 1.1:CBPointwise2d/p1c1 1.2:CBConv2d/p0i0 2:Tanh 3:Sequential 3.0:Sequential 3.0.0:CBConv2d/p1i0 3.0.1:CBPointwise2d/p0c1',
            None),
        'in a subclass of nn.Sequential': (
            '0:MySequential 0.0:CBConv2d/p0i0 0.1:Tanh 0.2:CBConv2d/p0i0',
            None),
        'beyond the limits': (
            '0:CBConv2d/p0i0 1:GELU 2:CBConv2d/p0i0',
            None),
        'a ReLU behind it': (
            '0:CBConv2d/p1i0 1:CBPointwise2d/p1c1 2:CBPointwise2d/p0c1 3:CBConv2d/p0i0',
            None),
        'a ReLU behind it, twice': (
            '0:CBConv2d/p1i0 1:CBPointwise2d/p1c1 2:CBPointwise2d/p1c1 3:CBPointwise2d/p1c1 4:CBPointwise2d/p1c1 5:CBConv2d/p0i0',
            None),
        'a batch norm and an activation behind it': (
            '0:CBConv2d/p1i0 1:CBPointwise2d/p1c1 3:CBConv2d/p0i0',
            None),
    },
    'linkDepthwise': {
        'behind CBConv2d': (
            '0:CBConv2d/p1i0 1:CBDepthwiseConv2d/p0c1i0 2:CBConv2d/p0i0',
            None),
        'behind CBPoolMax2d 2x2': (
            '0:CBPoolMax2d/p1c1d1 1:CBDepthwiseConv2d/p0c1i0 2:CBConv2d/p0i0',
            None),
        'behind CBPoolMax2d 3x3': (
            '0:CBPoolMax2d/p1c1d0 1:CBDepthwiseConv2d/p0c1i0 2:CBConv2d/p0i0',
            None),
        'behind CBPoolAvg2d': (
            '0:CBPoolAvg2d/p1c1d0 1:CBDepthwiseConv2d/p0c1i0 2:CBConv2d/p0i0',
            None),
        'behind CBAdd2d': (
            '0:CBAdd2d/p1c1 1:CBDepthwiseConv2d/p0c1i0 2:CBConv2d/p0i0',
            None),
        'behind CBResidual': (
            '0:CBResidual 0.body:Sequential 0.body.0:CBConv2d/p0i1 0.body.1:CBConv2d/p1i0 0.add:CBAdd2d/p1c1 1:CBDepthwiseConv2d/p0c1i0 2:CBConv2d/p0i0',
            None),
        'behind CBUpsample2d': (
            '0:CBUpsample2d/p1c1 1:CBDepthwiseConv2d/p0c1i0 2:CBConv2d/p0i0',
            None),
        'behind CBConvTranspose2d': (
            '0:CBConvTranspose2d/p1c1i1 1:CBDepthwiseConv2d/p0c1i0 2:CBConv2d/p0i0',
            None),
        'behind CBDepthwiseConv2d': (
            '0:CBDepthwiseConv2d/p1c1i0 1:CBDepthwiseConv2d/p0c1i0 2:CBConv2d/p0i0',
            None),
        'behind CBPointwise2d': (
            '0:CBPointwise2d/p1c1 1:CBDepthwiseConv2d/p0c1i0 2:CBConv2d/p0i0',
            None),
        'behind CBPixelShuffle2d': (
            '0:CBPixelShuffle2d/p1c1 1:CBDepthwiseConv2d/p0c1i0 2:CBConv2d/p0i0',
            None),
        'behind CBChannelShuffle2d': (
            '0:CBChannelShuffle2d/p1c1 1:CBDepthwiseConv2d/p0c1i0 2:CBConv2d/p0i0',
            None),
        'behind CBResize2d': (
            '0:CBResize2d/p1c1 1:CBDepthwiseConv2d/p0c1i0 2:CBConv2d/p0i0',
            None),
        'behind CBPad2d': (
            '0:CBPad2d/p1c1 1:CBDepthwiseConv2d/p0c1i0 2:CBConv2d/p0i0',
            None),
        'behind CBBinary2d': (
            '0:CBBinary2d/p1c1 1:CBDepthwiseConv2d/p0c1i0 2:CBConv2d/p0i0',
            None),
        'behind CBGLU2d': (
            '0:CBGLU2d/p1c1 1:CBDepthwiseConv2d/p0c1i0 2:CBConv2d/p0i0',
            None),
        'behind CBGated': (
            '0:CBGated 0.body:Sequential 0.body.0:CBConv2d/p0i1 0.body.1:CBConv2d/p1i0 0.mul:CBBinary2d/p1c1 1:CBDepthwiseConv2d/p0c1i0 2:CBConv2d/p0i0',
            None),
        'behind CBGroupedConv2d': (
            '0:CBGroupedConv2d/p0c1i0 1:CBDepthwiseConv2d/p0c1i0 2:CBConv2d/p0i0',
            None),
        'behind CBChannelReduce2d': (
            '0:CBChannelReduce2d/p0c1 1:CBDepthwiseConv2d/p0c1i0 2:CBConv2d/p0i0',
            None),
        'behind dense': (
            '0:Identity 1:CBDepthwiseConv2d/p0c1i0 2:CBConv2d/p0i0',
            None),
        'at position 0': (
            '0:CBDepthwiseConv2d/p0c1i0 1:CBConv2d/p0i0',
            None),
        'the last child': (
            '0:CBConv2d/p1i0 1:CBDepthwiseConv2d/p0c1i0',
            None),
        'in front of a 1x1': (
            '0:CBConv2d/p1i0 1:CBDepthwiseConv2d/p1c1i0 2:CBConv2d/p0i0',
            None),
        'in front of a strided 1x1': (
            '0:CBConv2d/p1i0 1:CBDepthwiseConv2d/p0c1i0 2:CBConv2d/p0i0',
            None),
        'in front of a 3x3 in feedback mode': (
            '0:CBConv2d/p1i0 1:CBDepthwiseConv2d/p0c1i0 2:CBConv2d/p0i0',
            None),
        'in front of a 1x1 in feedback mode': (
            '0:CBConv2d/p1i0 1:CBDepthwiseConv2d/p1c1i0 2:CBConv2d/p0i0',
            None),
        'in front of a dense module': (
            '0:CBConv2d/p1i0 1:CBDepthwiseConv2d/p0c1i0 2:Identity',
            None),
        'in front of a grouped convolution': (
            '0:CBConv2d/p1i0 1:CBDepthwiseConv2d/p0c1i0 2:CBGroupedConv2d/p0c1i0',
            None),
        'two in a row': (
            '0:CBConv2d/p1i0 1:CBDepthwiseConv2d/p1c1i0 2:CBDepthwiseConv2d/p1c1i0 3:CBConv2d/p0i0',
            None),
        'nested': (
            '0:Identity 1:Sequential 1.0:CBConv2d/p1i0 1.1:CBDepthwiseConv2d/p1c1i0 1.2:CBConv2d/p0i0 2:CBDepthwiseConv2d/p0c1i0 3:Sequential 3.0:Sequential 3.0.0:CBConv2d/p1i0 3.0.1:CBDepthwiseConv2d/p0c1i0',
            None),
        'in a subclass of nn.Sequential': (
            '0:MySequential 0.0:CBConv2d/p0i0 0.1:CBDepthwiseConv2d/p0c1i0 0.2:CBConv2d/p0i0',
            None),
        'beyond the limits': (
            '0:CBConv2d/p0i0 1:CBDepthwiseConv2d/p0c1i0 2:CBConv2d/p0i0',
            None),
        'a ReLU behind it': (
            '0:CBConv2d/p1i0 1:CBDepthwiseConv2d/p0c1i0 2:ReLU 3:CBConv2d/p0i0',
            None),
        'a ReLU behind it, twice': (
            '0:CBConv2d/p1i0 1:CBDepthwiseConv2d/p0c1i0 2:ReLU 3:CBDepthwiseConv2d/p0c1i0 4:ReLU 5:CBConv2d/p0i0',
            None),
        'a batch norm and an activation behind it': (
            '0:CBConv2d/p0i0 1:BatchNorm2d 2:CBDepthwiseConv2d/p1c1i0 3:CBConv2d/p0i0',
            None),
    },
    'linkGrouped': {
        'behind CBConv2d': (
            '0:CBConv2d/p0i0 1:CBGroupedConv2d/p0c1i0 2:CBConv2d/p0i1',
            None),
        'behind CBPoolMax2d 2x2': (
            '0:CBPoolMax2d/p0c1d0 1:CBGroupedConv2d/p0c1i0 2:CBConv2d/p0i1',
            None),
        'behind CBPoolMax2d 3x3': (
            '0:CBPoolMax2d/p0c1d0 1:CBGroupedConv2d/p0c1i0 2:CBConv2d/p0i1',
            None),
        'behind CBPoolAvg2d': (
            '0:CBPoolAvg2d/p0c1d0 1:CBGroupedConv2d/p0c1i0 2:CBConv2d/p0i1',
            None),
        'behind CBAdd2d': (
            '0:CBAdd2d/p0c1 1:CBGroupedConv2d/p0c1i0 2:CBConv2d/p0i1',
            None),
        'behind CBResidual': (
            '0:CBResidual 0.body:Sequential 0.body.0:CBConv2d/p0i1 0.body.1:CBConv2d/p1i0 0.add:CBAdd2d/p0c1 1:CBGroupedConv2d/p0c1i0 2:CBConv2d/p0i1',
            None),
        'behind CBUpsample2d': (
            '0:CBUpsample2d/p0c1 1:CBGroupedConv2d/p0c1i0 2:CBConv2d/p0i1',
            None),
        'behind CBConvTranspose2d': (
            '0:CBConvTranspose2d/p0c1i1 1:CBGroupedConv2d/p0c1i0 2:CBConv2d/p0i1',
            None),
        'behind CBDepthwiseConv2d': (
            '0:CBDepthwiseConv2d/p0c1i0 1:CBGroupedConv2d/p0c1i0 2:CBConv2d/p0i1',
            None),
        'behind CBPointwise2d': (
            '0:CBPointwise2d/p0c1 1:CBGroupedConv2d/p0c1i0 2:CBConv2d/p0i1',
            None),
        'behind CBPixelShuffle2d': (
            '0:CBPixelShuffle2d/p0c1 1:CBGroupedConv2d/p0c1i0 2:CBConv2d/p0i1',
            None),
        'behind CBChannelShuffle2d': (
            '0:CBChannelShuffle2d/p0c1 1:CBGroupedConv2d/p0c1i0 2:CBConv2d/p0i1',
            None),
        'behind CBResize2d': (
            '0:CBResize2d/p0c1 1:CBGroupedConv2d/p0c1i0 2:CBConv2d/p0i1',
            None),
        'behind CBPad2d': (
            '0:CBPad2d/p0c1 1:CBGroupedConv2d/p0c1i0 2:CBConv2d/p0i1',
            None),
        'behind CBBinary2d': (
            '0:CBBinary2d/p0c1 1:CBGroupedConv2d/p0c1i0 2:CBConv2d/p0i1',
            None),
        'behind CBGLU2d': (
            '0:CBGLU2d/p0c1 1:CBGroupedConv2d/p0c1i0 2:CBConv2d/p0i1',
            None),
        'behind CBGated': (
            '0:CBGated 0.body:Sequential 0.body.0:CBConv2d/p0i1 0.body.1:CBConv2d/p1i0 0.mul:CBBinary2d/p0c1 1:CBGroupedConv2d/p0c1i0 2:CBConv2d/p0i1',
            None),
        'behind CBGroupedConv2d': (
            '0:CBGroupedConv2d/p0c1i0 1:CBGroupedConv2d/p0c1i0 2:CBConv2d/p0i1',
            None),
        'behind CBChannelReduce2d': (
            '0:CBChannelReduce2d/p0c1 1:CBGroupedConv2d/p0c1i0 2:CBConv2d/p0i1',
            None),
        'behind dense': (
            '0:Identity 1:CBGroupedConv2d/p0c1i0 2:CBConv2d/p0i1',
            None),
        'at position 0': (
            '0:CBGroupedConv2d/p0c1i0 1:CBConv2d/p0i1',
            None),
        'the last child': (
            '0:CBConv2d/p0i0 1:CBGroupedConv2d/p0c1i0',
            None),
        'in front of a 1x1': (
            '0:CBConv2d/p0i0 1:CBGroupedConv2d/p1c1i0 2:CBConv2d/p0i0',
            None),
        'in front of a strided 1x1': (
            '0:CBConv2d/p0i0 1:CBGroupedConv2d/p0c1i0 2:CBConv2d/p0i1',
            None),
        'in front of a 3x3 in feedback mode': (
            '0:CBConv2d/p0i0 1:CBGroupedConv2d/p0c1i0 2:CBConv2d/p0i0',
            None),
        'in front of a 1x1 in feedback mode': (
            '0:CBConv2d/p0i0 1:CBGroupedConv2d/p1c1i0 2:CBConv2d/p0i0',
            None),
        'in front of a dense module': (
            '0:CBConv2d/p0i0 1:CBGroupedConv2d/p0c1i0 2:Identity',
            None),
        'in front of a grouped convolution': (
            '0:CBConv2d/p0i0 1:CBGroupedConv2d/p0c1i0 2:CBGroupedConv2d/p0c1i0',
            None),
        'two in a row': (
            '0:CBConv2d/p0i0 1:CBGroupedConv2d/p0c1i0 2:CBGroupedConv2d/p1c1i0 3:CBConv2d/p0i0',
            None),
        'nested': (
            '0:Identity 1:Sequential 1.0:CBConv2d/p0i0 1.1:CBGroupedConv2d/p1c1i0 1.2:CBConv2d/p0i0 2:CBGroupedConv2d/p0c1i0 3:Sequential 3.0:Sequential 3.0.0:CBConv2d/p0i0 3.0.1:CBGroupedConv2d/p0c1i0',
            None),
        'in a subclass of nn.Sequential': (
            '0:MySequential 0.0:CBConv2d/p0i0 0.1:CBGroupedConv2d/p0c1i0 0.2:CBConv2d/p0i0',
            None),
        'beyond the limits': (
            '0:CBConv2d/p0i0 1:Identity 2:CBConv2d/p0i0',
            None),
        'a ReLU behind it': (
            '0:CBConv2d/p0i0 1:CBGroupedConv2d/p0c1i0 2:ReLU 3:CBConv2d/p0i0',
            None),
        'a ReLU behind it, twice': (
            '0:CBConv2d/p0i0 1:CBGroupedConv2d/p0c1i0 2:ReLU 3:CBGroupedConv2d/p0c1i0 4:ReLU 5:CBConv2d/p0i0',
            None),
        'a batch norm and an activation behind it': (
            '0:CBConv2d/p0i0 1:BatchNorm2d 2:CBGroupedConv2d/p1c1i0 3:CBConv2d/p0i0',
            None),
    },
}


# ------------------------------------------------------------------------------------------------ the producer matrix
# What every pass accepts in front of its module, by name and in order: recorded by running each pass at the commit
# before chain.PRODUCERS was written -- watching the set it handed to the walk or tested its producer against, the types
# it added at the call included; insertCBPooling by offering it every exported type in front of a pool.
B = ['CBConv2d', 'CBPoolMax2d', 'CBPoolAvg2d', 'CBAdd2d', 'CBResidual', 'CBUpsample2d', 'CBConvTranspose2d',
     'CBDepthwiseConv2d', 'CBPointwise2d', 'CBPixelShuffle2d', 'CBChannelShuffle2d', 'CBResize2d', 'CBPad2d',
     'CBBinary2d', 'CBGLU2d', 'CBGated']
B_NO_TRANSPOSED = ['CBConv2d', 'CBPoolMax2d', 'CBPoolAvg2d', 'CBAdd2d', 'CBResidual', 'CBUpsample2d',
                   'CBDepthwiseConv2d', 'CBPointwise2d', 'CBPixelShuffle2d', 'CBChannelShuffle2d', 'CBResize2d',
                   'CBPad2d', 'CBBinary2d', 'CBGLU2d', 'CBGated']
MATRIX = {
    'linkDepthwise': B,
    'insertCBPointwise': B,
    'insertCBTransposedConv': B,
    'insertCBUpsampling': B_NO_TRANSPOSED,
    'insertCBRearrange': B + ['CBGroupedConv2d'],
    'insertCBChannelOps': B + ['CBGroupedConv2d', 'CBChannelReduce2d'],
    'insertCBPadding': B + ['CBGroupedConv2d', 'CBChannelReduce2d'],
    'insertCBGating': B + ['CBGroupedConv2d', 'CBChannelReduce2d'],
    'insertCBResize': B_NO_TRANSPOSED + ['CBGroupedConv2d', 'CBChannelReduce2d'],
    'insertCBPooling': ['CBConv2d'],
    'insertCBPooling(generalGeometry=True)': ['CBConv2d', 'CBPointwise2d', 'CBPad2d'],
}
# the module types that wrap stateful children and keep no state of their own
WRAPPERS = ['CBResidual', 'CBGated', 'CBSqueezeExcite']
# the layers that SequenceBatch takes or refuses by its own rule, not through batch.CHAIN_OPERATORS
BATCH_OWN_RULE = ['CBConv2d', 'CBPoolMax2d', 'CBPoolAvg2d', 'CBTail1x1']


def _module_types():
    """Every nn.Module subclass the package exports under a CB name."""
    import cbinfer_amd
    found = [getattr(cbinfer_amd, n) for n in cbinfer_amd.__all__ if n.startswith('CB')]
    return [t for t in found if isinstance(t, type) and issubclass(t, nn.Module)]


def test_every_pass_accepts_the_producers_recorded(pkg, chain, Err):
    assert list(chain.PASSES) == list(MATRIX) and len(MATRIX) == 11
    for passName, want in MATRIX.items():
        got = chain.producers(passName)
        assert type(got) is tuple and [t.__name__ for t in got] == want, passName
        assert all(t is getattr(pkg, t.__name__) for t in got), passName
    for unknown in ('linkGrouped', 'insertCBPooling(generalGeometry=False)', ''):      # (no set: never all of them)
        with pytest.raises(Err, match="is no pass of"):
            chain.producers(unknown)


def test_producer_table_has_one_row_for_every_module_type(chain):
    import cbinfer_amd
    rows = [row[0] for row in chain.PRODUCERS]
    assert len(set(rows)) == len(rows)
    assert sorted(rows) == sorted(t.__name__ for t in _module_types())      # a row each, and every row exported
    for name, module, rule, passes in chain.PRODUCERS:
        assert getattr(getattr(cbinfer_amd, module), name) is getattr(cbinfer_amd, name)
        assert rule in (chain.BUT, chain.ONLY) and set(passes) <= set(chain.PASSES), name
    # a producer for no pass stands in the table as that
    assert [row[0] for row in chain.PRODUCERS if row[2:] == (chain.ONLY, ())] == [
        'CBConcat2d', 'CBTail1x1', 'CBChannelScale2d', 'CBSqueezeExcite', 'CBGroupNorm2d']
    assert not any(rule == chain.BUT and set(passes) == set(chain.PASSES) for _, _, rule, passes in chain.PRODUCERS)


def test_clear_memory_reaches_every_module_type_with_state():
    import cbinfer_amd
    stateful = [t.__name__ for t in cbinfer_amd._STATEFUL]
    assert len(set(stateful)) == len(stateful)
    for t in _module_types():
        if t.__name__ in WRAPPERS:
            assert not hasattr(t, 'getStateTensors') and t.__name__ not in stateful
        else:
            assert hasattr(t, 'getStateTensors') and hasattr(t, 'clearMemory') and t.__name__ in stateful, t.__name__
    assert set(stateful) <= set(t.__name__ for t in _module_types())
    # the wrappers' own children are reached: what they add is a CBAdd2d / a CBBinary2d
    assert {'CBAdd2d', 'CBBinary2d'} <= set(stateful)


def test_batch_and_branch_group_refuse_every_chain_operator():
    import cbinfer_amd
    from cbinfer_amd import batch
    refused = [t.__name__ for row in batch.CHAIN_OPERATORS for t in row[0]]
    assert len(set(refused)) == len(refused) and not set(refused) & set(BATCH_OWN_RULE)
    # (the wrapper CBSqueezeExcite keeps no state, and is refused under its own name: named_modules() reaches it before
    #  its scale)
    assert sorted(refused + BATCH_OWN_RULE) == sorted([t.__name__ for t in cbinfer_amd._STATEFUL] + ['CBSqueezeExcite'])


def test_batch_refusal_rows_are_the_thirteen_recorded():
    """batch.CHAIN_OPERATORS, row for row: the eleven rows of the table and the two that stood in tables of their own
    beside it (the channel attention scale, the group norm), as they read before the three became one."""
    from cbinfer_amd import batch
    assert [(tuple(t.__name__ for t in types), noun, networks) for types, noun, networks in batch.CHAIN_OPERATORS] == [
        (('CBAdd2d',), 'a change-based sum', 'residual'),
        (('CBUpsample2d', 'CBConcat2d'), 'a change-based decoder operator', 'decoder'),
        (('CBConvTranspose2d',), 'a change-based transposed convolution', 'decoder'),
        (('CBDepthwiseConv2d',), 'a change-based depthwise convolution', 'separable'),
        (('CBPointwise2d',), 'a change-based element-wise function', 'such'),
        (('CBGroupedConv2d',), 'a change-based grouped convolution', 'ResNeXt-type'),
        (('CBPixelShuffle2d', 'CBChannelShuffle2d'), 'a change-based rearrangement',
         'super-resolution and ShuffleNet-type'),
        (('CBChannelReduce2d',), 'a change-based per-pixel channel reduction', 'ConvNeXt-type and segmentation'),
        (('CBResize2d',), 'a change-based resize', 'dense-prediction'),
        (('CBPad2d',), 'a change-based padding', 'reflection-padded and restoration'),
        (('CBBinary2d', 'CBGLU2d'), 'a change-based element-wise operator of two maps', 'gated and attention'),
        (('CBSqueezeExcite', 'CBChannelScale2d'), 'a change-based channel attention scale', 'squeeze-and-excitation'),
        (('CBGroupNorm2d',), 'a change-based group norm', 'GroupNorm and InstanceNorm'),
    ]
    assert type(batch.CHAIN_OPERATORS) is tuple and all(type(row[0]) is tuple for row in batch.CHAIN_OPERATORS)


def test_alias_package_mirrors_the_table(chain):
    import sys
    import cbinfer_amd
    import pycbinfer
    for name, module, _, _ in chain.PRODUCERS:
        assert getattr(pycbinfer, name) is getattr(cbinfer_amd, name)
        assert sys.modules['pycbinfer.' + module] is getattr(pycbinfer, module) is getattr(cbinfer_amd, module)
    for module in ('conv2d_cg', 'conv2d_fg'):
        assert sys.modules['pycbinfer.' + module] is getattr(pycbinfer, module) is getattr(cbinfer_amd, module)
    assert sorted(k for k in sys.modules if k.startswith('pycbinfer.')) == sorted('pycbinfer.' + m for m in (
        'conv2d', 'conv2d_cg', 'conv2d_fg', 'pool', 'residual', 'decoder', 'tconv', 'dwconv', 'pointwise', 'groupconv',
        'rearrange', 'chanreduce', 'resize', 'pad', 'binary', 'chanscale', 'groupnorm'))
    assert pycbinfer.__all__ is cbinfer_amd.__all__
