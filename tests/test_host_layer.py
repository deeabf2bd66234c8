"""CPU: what CBDepthwiseConv2d, CBGroupedConv2d and CBConvTranspose2d share on the host (cbinfer_amd/layer.py, DESIGN
5.20) -- the one base class and what each class has and has not, the bias map, the state (re)allocation, the refusals of
forward, pickling and copying, chain.state_fits and the per-axis limit check.  Pure torch on CPU tensors plus the loaded
library's size functions: nothing is launched."""
import copy
import pickle

import pytest
import torch
import torch.nn as nn

KINDS = ("dw", "grouped", "tconv")
NAMES = dict(dw="CBDepthwiseConv2d", grouped="CBGroupedConv2d", tconv="CBConvTranspose2d")
BIAS = [7.5, -1.25, 0.5, 3.0]      # one element above 6, one below 0; exact in fp16


@pytest.fixture(scope="module")
def pkg():
    import cbinfer_amd
    return cbinfer_amd


def error():
    from cbinfer_amd._lib import CBinferError
    return CBinferError


def source(kind, bias=True):
    """The smallest source module of each class: 4 -> 4 channels, 3x3."""
    if kind == "dw":
        m = nn.Conv2d(4, 4, 3, 1, 1, groups=4, bias=bias)
    elif kind == "grouped":
        m = nn.Conv2d(4, 4, 3, 1, 1, groups=2, bias=bias)
    else:
        m = nn.ConvTranspose2d(4, 4, 3, 2, 1, 1, bias=bias)
    if bias:
        with torch.no_grad():
            m.bias.copy_(torch.tensor(BIAS))
    return m


def layer(pkg, kind, bias=True):
    return getattr(pkg, NAMES[kind])(source(kind, bias), 0.05)


# ------------------------------------------------------------------------------------------------ the base
# the instance attributes of each class at the commit before the base existed (nn.Module's own left out)
COMMON = {'kernel_size', 'stride', 'padding', 'dilation', 'groups', 'transposed', 'in_channels', 'out_channels',
          'threshold', 'withReLU', 'propChangeIndexes', 'copyInput', 'feedbackLoop', 'cloneOutput', '_work', '_geomC'}
ATTRIBUTES = dict(dw=COMMON | {'reluCap', 'propagatedChanges'}, grouped=COMMON | {'exactF32', '_wprep'},
                  tconv=COMMON | {'exactF32', '_wprep', 'output_padding'})


def test_one_base_and_no_borrowed_attributes(pkg):
    import pycbinfer
    from cbinfer_amd import layer as L
    for kind in KINDS:
        cls = getattr(pkg, NAMES[kind])
        assert issubclass(cls, L.CBDetectingLayer) and issubclass(cls, nn.Module)
        assert issubclass(cls, L.CBContractingLayer) == (kind != "dw")
        m = layer(pkg, kind)
        assert type(m) is cls and cls.__module__ == "cbinfer_amd." + dict(dw="dwconv", grouped="groupconv",
                                                                          tconv="tconv")[kind]
        assert set(m.__dict__) - set(nn.Module().__dict__) == ATTRIBUTES[kind], kind
        assert m.transposed == (kind == "tconv")
        assert {n for n, _ in m.named_buffers()} == {'prevInput', 'prevOutput'}
        for name in ('exactF32', 'invalidateWeights', '_arith', '_wprep', '_weights'):
            assert hasattr(m, name) == (kind != "dw"), (kind, name)
        for name in ('reluCap', 'propagatedChanges'):
            assert hasattr(m, name) == (kind == "dw"), (kind, name)
        assert hasattr(m, 'output_padding') == (kind == "tconv")
    for name in ('CBDetectingLayer', 'CBContractingLayer', 'layer'):
        assert name not in pkg.__all__ and name not in pycbinfer.__all__ and not hasattr(pycbinfer, name)


# ------------------------------------------------------------------------------------------------ _bias_map
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("kind", KINDS)
def test_bias_map(pkg, kind, dtype):
    like, size = torch.zeros(1, dtype=dtype), (1, 4, 5, 6)
    b = torch.tensor(BIAS, dtype=dtype).view(1, 4, 1, 1).expand(size)
    none = layer(pkg, kind, bias=False)
    none.withReLU = True
    out = none._bias_map(size, like)
    assert out.dtype == dtype and tuple(out.shape) == size and torch.equal(out, torch.zeros(size, dtype=dtype))
    m = layer(pkg, kind)
    assert torch.equal(m._bias_map(size, like), b)
    m.withReLU = True
    out = m._bias_map(size, like)
    assert out.dtype == dtype and out.is_contiguous() and torch.equal(out, b.clamp(min=0))
    assert out[0, 0, 0, 0] == 7.5 and out[0, 1, 4, 5] == 0
    if kind == "dw":
        m.reluCap = 6.0
        out = m._bias_map(size, like)
        assert torch.equal(out, b.clamp(0, 6))
        assert out[0, 0, 2, 3] == 6 and out[0, 1, 2, 3] == 0 and out[0, 2, 2, 3] == 0.5
        m.reluCap = 5.0
        with pytest.raises(error()) as e:
            m._bias_map(size, like)
        assert str(e.value) == "CBDepthwiseConv2d: reluCap=5.0 is not supported, only None or 6.0"
        m.withReLU = False      # (the cap is read only with the ReLU)
        assert torch.equal(m._bias_map(size, like), b)


# ------------------------------------------------------------------------------------------------ _state_for
def out_size(kind, H, W):
    return (2 * H, 2 * W) if kind == "tconv" else (H, W)


@pytest.mark.parametrize("kind", KINDS)
def test_state_for(pkg, kind):
    m = layer(pkg, kind)
    m.withReLU = True
    x = torch.zeros(1, 4, 5, 6)
    Ho, Wo = m._out_hw(5, 6)
    assert (Ho, Wo) == out_size(kind, 5, 6)
    assert m.prevInput.numel() == 0 and m.prevOutput.numel() == 0
    assert m._state_for(x, Ho, Wo) is True
    pin, pout = m.prevInput, m.prevOutput
    assert pin.shape == x.shape and pin.dtype == x.dtype and bool(torch.isposinf(pin).all())
    assert torch.equal(pout, m._bias_map((1, 4, Ho, Wo), x)) and float(pout[0, 1].max()) == 0.0
    # the same frame shape again: both objects stay
    assert m._state_for(x, Ho, Wo) is False and m.prevInput is pin and m.prevOutput is pout
    # a kept prevInput that is not contiguous is made so, with its values
    m.prevInput = torch.arange(120.).view(1, 4, 6, 5).transpose(2, 3)
    want = m.prevInput.clone()
    assert not m.prevInput.is_contiguous() and m._state_for(x, Ho, Wo) is False
    assert m.prevInput.is_contiguous() and torch.equal(m.prevInput, want) and m.prevOutput is pout
    # another height (and width), another dtype, a cleared memory: both are made again
    for x2 in (torch.zeros(1, 4, 9, 6), torch.zeros(1, 4, 9, 9), torch.zeros(1, 4, 9, 9, dtype=torch.float16)):
        pin, pout = m.prevInput, m.prevOutput
        H2, W2 = m._out_hw(x2.size(2), x2.size(3))
        assert m._state_for(x2, H2, W2) is True
        assert m.prevInput is not pin and m.prevOutput is not pout
        assert m.prevInput.shape == x2.shape and m.prevInput.dtype == x2.dtype
        assert bool(torch.isposinf(m.prevInput).all())
        assert tuple(m.prevOutput.shape) == (1, 4, H2, W2) and m.prevOutput.dtype == x2.dtype
        assert m._state_for(x2, H2, W2) is False
    m.clearMemory()
    assert m.prevInput.numel() == 0 and m.prevOutput.numel() == 0 and m.__dict__['_work'] is None
    assert m._state_for(x, Ho, Wo) is True and m.prevInput.shape == x.shape
    assert tuple(m.prevOutput.shape) == (1, 4, Ho, Wo)


def test_a_map_without_output_is_refused_in_each_class_s_words(pkg):
    cases = [
        (pkg.CBDepthwiseConv2d(nn.Conv2d(4, 4, 3, groups=4), 0.1), (2, 6), (3, 4),
         "CBDepthwiseConv2d: a 2x6 map is smaller than the filter's reach (kernel_size=(3, 3), dilation=(1, 1), "
         "padding=(0, 0))"),
        (pkg.CBGroupedConv2d(nn.Conv2d(4, 4, 3, groups=2, dilation=2, padding=(1, 0)), 0.1), (5, 4), (3, 2),
         "CBGroupedConv2d: a 5x4 map is smaller than the filter's reach (kernel_size=(3, 3), dilation=(2, 2), "
         "padding=(1, 0))"),
        (pkg.CBConvTranspose2d(nn.ConvTranspose2d(4, 4, 3, 1, 2), 0.1), (1, 6), (3, 4),
         "CBConvTranspose2d: a 1x6 map has no output (kernel_size=(3, 3) stride=(1, 1) padding=(2, 2) dilation=(1, 1) "
         "output_padding=(0, 0))"),
    ]
    for m, (Hi, Wi), fits, words in cases:
        with pytest.raises(error()) as e:
            m._out_hw(Hi, Wi)
        assert str(e.value) == words
        assert m._out_hw(5, 6) == fits


def test_state_for_without_the_input(pkg):
    m = layer(pkg, "dw")
    x = torch.zeros(1, 4, 5, 6)
    assert m._state_for(x, 5, 6, keepInput=False) is True and m.prevInput.numel() == 0
    pout = m.prevOutput
    assert m._state_for(x, 5, 6, keepInput=False) is False and m.prevOutput is pout and m.prevInput.numel() == 0
    assert m._state_for(x, 5, 6, keepInput=True) is False and m.prevOutput is pout      # prevInput alone is new
    assert m.prevInput.shape == x.shape and bool(torch.isposinf(m.prevInput).all())
    assert m._state_for(x, 5, 6, keepInput=False) is False and m.prevInput.numel() == 0      # ... and dropped again
    x2 = torch.zeros(1, 4, 9, 9)
    assert m._state_for(x2, 9, 9, keepInput=False) is True and m.prevOutput is not pout
    assert tuple(m.prevOutput.shape) == (1, 4, 9, 9) and m.prevInput.numel() == 0


# ------------------------------------------------------------------------------------------------ forward
REFUSALS = [      # (argument, the sentence with %s for the class name; None: the library's own "HIP devices only")
    (lambda: ('indexes', torch.zeros(1, 3, 5, 6), None),
     "%s: the input is a tuple, but not ('changeIndexes', tensor, indexes)"),
    (lambda: ('changeIndexes', torch.zeros(1, 4, 5, 6)),
     "%s: the input is a tuple, but not ('changeIndexes', tensor, indexes)"),
    (lambda: [1, 2], "%s: the input must be a tensor or the ('changeIndexes', tensor, indexes) tuple, got list"),
    (lambda: ('changeIndexes', None, None),
     "%s: the input must be a tensor or the ('changeIndexes', tensor, indexes) tuple, got NoneType"),
    (lambda: torch.zeros(1, 3, 5, 6), "%s: the input must be a [1, 4, H, W] tensor, got (1, 3, 5, 6)"),
    (lambda: torch.zeros(2, 4, 5, 6), "%s: the input must be a [1, 4, H, W] tensor, got (2, 4, 5, 6)"),
    (lambda: ('changeIndexes', torch.zeros(4, 5, 6), None),
     "%s: the input must be a [1, 4, H, W] tensor, got (4, 5, 6)"),
    (lambda: torch.zeros(1, 4, 5, 6), None),
    (lambda: ('changeIndexes', torch.zeros(1, 4, 5, 6, dtype=torch.float16), None), None),
]


def test_forward_refusals_are_one_sentence(pkg):
    said = {}
    for kind in KINDS:
        m = layer(pkg, kind)
        for make, words in REFUSALS:
            with pytest.raises(error()) as e:
                m(make())
            said.setdefault(kind, []).append(str(e.value))
            if words is None:
                assert str(e.value).startswith("cbinfer_amd runs on HIP devices only: got a CPU tensor.")
            else:
                assert str(e.value) == words % NAMES[kind]
        assert m.prevInput.numel() == 0 and m.prevOutput.numel() == 0 and m.__dict__['_work'] is None
    for kind in KINDS:
        assert [s.replace(NAMES[kind], "X") for s in said[kind]] == [s.replace(NAMES["dw"], "X") for s in said["dw"]]


# ------------------------------------------------------------------------------------------------ pickle, deepcopy
TRANSIENT = dict(dw=('_work', '_geomC'), grouped=('_work', '_wprep', '_geomC'), tconv=('_work', '_wprep', '_geomC'))
GEOMETRY = dict(dw=(3, 3, 1, 1, 1, 1, 1, 1), grouped=(3, 3, 1, 1, 1, 1, 1, 1), tconv=(3, 3, 2, 2, 1, 1, 1, 1, 1, 1))


@pytest.mark.parametrize("how", ["pickle", "deepcopy"])
@pytest.mark.parametrize("kind", KINDS)
def test_round_trip_drops_the_transient_slots(pkg, kind, how):
    m = layer(pkg, kind)
    m.withReLU, m.propChangeIndexes, m.cloneOutput = True, True, False
    m._state_for(torch.zeros(1, 4, 5, 6), *m._out_hw(5, 6))
    m._struct()
    m.__dict__['_work'] = {'key': None}
    if kind != "dw":
        m.__dict__['_wprep'] = ("key", torch.zeros(3))
    assert all(m.__dict__[name] is not None for name in TRANSIENT[kind])
    new = pickle.loads(pickle.dumps(m)) if how == "pickle" else copy.deepcopy(m)
    assert type(new) is type(m) and repr(new) == repr(m)
    assert all(m.__dict__[name] is not None for name in TRANSIENT[kind])      # (the original keeps its own)
    assert {name: new.__dict__[name] for name in TRANSIENT[kind]} == dict.fromkeys(TRANSIENT[kind])
    assert set(new.__dict__) == set(m.__dict__)
    assert new.withReLU and new.propChangeIndexes and not new.cloneOutput and new.threshold == 0.05
    g = new._struct().contents
    assert tuple(getattr(g, f) for f, _ in g._fields_) == GEOMETRY[kind]
    assert type(g).__name__ == ("TGeom" if kind == "tconv" else "Geom") and new._struct() is new.__dict__['_geomC']
    assert list(new.state_dict()) == ['weight', 'bias', 'prevInput', 'prevOutput']
    for key, t in m.state_dict().items():
        assert torch.equal(new.state_dict()[key], t), key
    assert list(layer(pkg, kind, bias=False).state_dict()) == ['weight', 'prevInput', 'prevOutput']
    if kind != "dw":
        m.invalidateWeights()
        assert m.__dict__['_wprep'] is None and m.__dict__['_work'] is not None


# ------------------------------------------------------------------------------------------------ chain.state_fits
def test_state_fits():
    from cbinfer_amd.chain import state_fits
    like = torch.zeros(2, dtype=torch.float16)
    state = torch.zeros(1, 4, 5, 6, dtype=torch.float16)
    assert state_fits(state, (1, 4, 5, 6), like) is True and state_fits(state, torch.Size([1, 4, 5, 6]), like) is True
    assert state_fits(state, [1, 4, 5, 6], state) is True
    for shape in ((1, 4, 6, 5), (1, 4, 5, 7), (4, 5, 6), (1, 4, 30)):
        assert state_fits(state, shape, like) is False, shape
    assert state_fits(state, (1, 4, 5, 6), torch.zeros(2)) is False      # another dtype
    assert state_fits(state.new_zeros(0), (1, 4, 5, 6), like) is False      # an empty state
    assert state_fits(state.new_zeros(0), (0,), like) is True
    assert state_fits(None, (1, 4, 5, 6), like) is False


# ------------------------------------------------------------------------------------------------ the limit check
def conv(kind, k=3, s=1, p=0, d=1):
    if kind == "tconv":
        return nn.ConvTranspose2d(4, 4, k, s, p, 0, 1, True, d)
    return nn.Conv2d(4, 4, k, s, p, d, groups=4 if kind == "dw" else 2)


LIMITS = dict(dw=dict(k=7, s=4, d=8, p=64), grouped=dict(k=7, s=4, d=8, p=64), tconv=dict(k=8, s=4, d=4))
SETTING = dict(k="kernel_size", s="stride", d="dilation", p="padding")


@pytest.mark.parametrize("kind", KINDS)
def test_per_axis_limits(pkg, kind):
    import importlib
    mod = importlib.import_module("cbinfer_amd." + dict(dw="dwconv", grouped="groupconv", tconv="tconv")[kind])
    cls, lim = getattr(pkg, NAMES[kind]), LIMITS[kind]
    assert (mod.MAX_K, mod.MAX_S, mod.MAX_D) == (lim['k'], lim['s'], lim['d'])
    assert getattr(mod, 'MAX_P', None) == lim.get('p')
    for axis in (0, 1):
        for key, limit in lim.items():
            inside = (limit, 1) if axis == 0 else (1, limit)
            beyond = (limit + 1, 1) if axis == 0 else (1, limit + 1)
            m = cls(conv(kind, **{key: inside}), 0.1)
            assert getattr(m, SETTING[key]) == inside
            with pytest.raises(error()) as e:
                cls(conv(kind, **{key: beyond}), 0.1)
            assert str(e.value) == "%s: %s=%s is beyond what the library takes (<= %d per axis)" % (
                NAMES[kind], SETTING[key], beyond, limit)
    # several at once: the first axis with a violation, and on it kernel_size, stride, dilation, padding in this order
    k, s, d = lim['k'] + 1, lim['s'] + 1, lim['d'] + 1
    for kw, first in [(dict(k=(1, k), s=(s, 1)), "stride=(%d, 1)" % s),
                      (dict(k=(k, 1), s=(s, 1)), "kernel_size=(%d, 1)" % k),
                      (dict(s=(1, s), d=(1, d)), "stride=(1, %d)" % s),
                      (dict(k=(1, k), d=(d, 1)), "dilation=(%d, 1)" % d)]:
        with pytest.raises(error()) as e:
            cls(conv(kind, **kw), 0.1)
        assert str(e.value).startswith("%s: %s is beyond" % (NAMES[kind], first)), (kw, str(e.value))
    if kind == "tconv":      # its two range rules of an axis come before the next axis' limits
        with pytest.raises(error(), match=r"^CBConvTranspose2d: padding=\(3, 0\) is beyond what the library "
                                                   r"takes \(0 <= padding <= dilation \* \(kernel_size - 1\) per axis"):
            cls(conv(kind, k=(3, 9), p=(3, 0)), 0.1)
        with pytest.raises(error(), match=r"^CBConvTranspose2d: kernel_size=\(9, 3\) is beyond"):
            cls(conv(kind, k=(9, 3), p=(0, 3)), 0.1)
    else:
        with pytest.raises(error(), match=r"^%s: dilation=\(1, 9\) is beyond" % NAMES[kind]):
            cls(conv(kind, d=(1, 9), p=(1, 65)), 0.1)
        with pytest.raises(error(), match=r"^%s: padding=\(65, 1\) is beyond" % NAMES[kind]):
            cls(conv(kind, d=(1, 9), p=(65, 1)), 0.1)
