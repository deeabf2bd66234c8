"""CPU-only tests of the change-based padding (CBPad2d, insertCBPadding, splitConvPadding; cb_pad.hip):
the numpy twin of tests/pad_cases.py against torch's F.pad on the CPU bit for bit and against a brute-force footprint,
what the constructor takes and refuses, the host entry points and the argument checks of the C entry point, what the two
passes and the passes behind them do to a network, exports, pickling and the refusals.  No kernel is launched here."""
import copy
import ctypes
import inspect
import pickle

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import pad_cases as pc
from rearrange_cases import same_bits, special_values
from optest import lib, names_of, pkg      # noqa: F401  (fixtures)

VALUES = (0.0, -0.0, 0.1, -3.5, float('inf'))


# ------------------------------------------------------------------------------------------------ the twin
@pytest.mark.parametrize("npdt", [np.float32, np.float16], ids=["f32", "f16"])
def test_value_twin_is_torch_bit_for_bit(npdt):
    """Every case of the table (asymmetric pads, reflect p = n - 1, circular p = n, crops); the values hold -0, +-inf
    and NaNs with payloads and are compared as integers; constant mode with every value of VALUES."""
    rng = np.random.default_rng(1)
    for case in pc.CASES:
        mode, pads, shape = case
        x = special_values(rng, shape, npdt)
        for value in VALUES if mode == "constant" else (0.0,):
            want = F.pad(torch.from_numpy(x)[None], pads, mode=mode, value=value)[0].numpy()
            got = pc.twin(mode, pads, x, value)
            assert got.shape == want.shape == pc.out_shape(pads, shape), case
            assert same_bits(got, want), (case, value)
    # the formulas on a hand-made row each: n = 4, p = 3 in front and behind
    o = np.arange(10)
    assert list(pc.source("constant", o, 3, 4)) == [-1, -1, -1, 0, 1, 2, 3, -1, -1, -1]
    assert list(pc.source("reflect", o, 3, 4)) == [3, 2, 1, 0, 1, 2, 3, 2, 1, 0]
    assert list(pc.source("replicate", o, 3, 4)) == [0, 0, 0, 0, 1, 2, 3, 3, 3, 3]
    assert list(pc.source("circular", o, 3, 4)) == [1, 2, 3, 0, 1, 2, 3, 0, 1, 2]
    assert list(pc.source("circular", np.arange(12), 4, 4)) == [0, 1, 2, 3] * 3      # p = n: torch takes it
    assert list(pc.source("constant", np.arange(3), -2, 6)) == [2, 3, 4]             # a crop of 2 in front, 1 behind


def test_the_limits_are_torchs_own_rules(lib):
    """reflect needs pad < n, circular pad <= n: what torch takes cbinfer_pad_supported takes, what torch refuses it
    refuses; torch refuses a value that overflows the dtype as CBPad2d does."""
    x = torch.zeros(1, 1, 3, 4)

    def supported(pads, mode):
        return lib.C.cbinfer_pad_supported(ctypes.pointer(lib.Pad(pc.MODES.index(mode), *(pads + (0.0,)))), 3, 4)

    for pads, mode in (((3, 3, 2, 2), 'reflect'), ((4, 4, 3, 3), 'circular'), ((64, 64, 64, 64), 'replicate')):
        assert tuple(F.pad(x, pads, mode=mode).shape[2:]) == pc.out_shape(pads, (1, 3, 4))[1:]
        assert supported(pads, mode) == 1
    for pads, mode in (((4, 0, 0, 0), 'reflect'), ((0, 0, 0, 3), 'reflect'), ((5, 0, 0, 0), 'circular'),
                       ((0, 0, 4, 0), 'circular')):
        with pytest.raises(RuntimeError):
            F.pad(x, pads, mode=mode)
        assert supported(pads, mode) == 0
    with pytest.raises(RuntimeError, match="overflow"):
        F.pad(x.half(), (1, 1, 1, 1), value=1e6)


def test_footprint_twin_against_brute_force():
    """An output pixel is listed iff the input pixel it reads -- found by padding the pixels' own numbers with the twin,
    -1 where nothing is read -- changed."""
    rng = np.random.default_rng(2)
    for case in pc.CASES:
        mode, pads, (Cn, H, W) = case
        if H > 100:
            H = 7
        ids = np.arange(H * W, dtype=np.int64).reshape(1, H, W)
        reads = pc.twin(mode, pads, ids, value=-1)[0]
        masks = [rng.random((H, W)) < p for p in (0.0, 0.05, 0.5, 1.0)]
        one = np.zeros((H, W), dtype=bool)
        one[min(1, H - 1), min(1, W - 1)] = True
        for changed in masks + [one]:
            flat = np.concatenate([changed.reshape(-1), [False]])      # (index -1: reads nothing)
            got = pc.footprint(mode, pads, changed)
            assert got.dtype == bool and np.array_equal(got, flat[reads]), case
        if mode != "constant":
            assert pc.footprint(mode, pads, np.ones((H, W), dtype=bool)).all()
    m = np.zeros((3, 4), dtype=bool)
    m[1, 1] = True
    want = np.zeros((7, 8), dtype=bool)
    want[[1, 3, 5], 1] = want[[1, 3, 5], 3] = want[[1, 3, 5], 7] = True      # rows 2 + (-1, 1, 3), columns 2 + (-1, 1, 5)
    assert np.array_equal(pc.footprint("reflect", (2, 2, 2, 2), m), want)
    crop = np.zeros((4, 6), dtype=bool)
    crop[0, 0] = True      # cropped off by left = -1
    assert not pc.footprint("constant", (-1, 2, 2, -1), crop).any()


# ------------------------------------------------------------------------------------------------ the constructor
class MyPad(nn.ReflectionPad2d):
    pass


def test_constructor_takes_and_refuses(pkg, lib):
    P, Err = pkg.CBPad2d, lib.CBinferError
    for m, want in ((nn.ReflectionPad2d(1), ((1, 1, 1, 1), 'reflect', 0.0)),
                    (nn.ReflectionPad2d((0, 5, 2, 0)), ((0, 5, 2, 0), 'reflect', 0.0)),
                    (nn.ReplicationPad2d((2, 64, 0, 1)), ((2, 64, 0, 1), 'replicate', 0.0)),
                    (nn.ZeroPad2d((0, 1, 0, 1)), ((0, 1, 0, 1), 'constant', 0.0)),
                    (nn.ZeroPad2d((-1, 2, 2, -1)), ((-1, 2, 2, -1), 'constant', 0.0)),
                    (nn.ConstantPad2d(3, -3.5), ((3, 3, 3, 3), 'constant', -3.5)),
                    (nn.ConstantPad2d((1, 2, 3, 4), 2), ((1, 2, 3, 4), 'constant', 2.0)),
                    (nn.CircularPad2d((4, 1, 0, 2)), ((4, 1, 0, 2), 'circular', 0.0))):
        cb = P(m)
        assert (cb.padding, cb.mode, cb.value) == want, m
        assert type(cb.value) is float and not cb.propChangeIndexes and cb.cloneOutput and cb.outputState.numel() == 0
        assert repr(cb) == 'CBPad2d (padding=%s, mode=%s, value=%s, propChgIdxs=False)' % want
        s = cb._struct().contents
        assert (s.mode, s.left, s.right, s.top, s.bottom, s.value) == (pc.MODES.index(want[1]),) + want[0] + (want[2],)
    cb = P(padding=2, mode='replicate')
    assert (cb.padding, cb.mode, cb.value) == ((2, 2, 2, 2), 'replicate', 0.0)
    cb = P(padding=[1, 0, -3, 64], value=float('inf'))
    assert (cb.padding, cb.mode, cb.value) == ((1, 0, -3, 64), 'constant', float('inf'))
    assert P(padding=(3, 3, 3, 3), mode='reflect').out_size(4, 4) == (10, 10)
    assert P(padding=(4, 4, 3, 3), mode='circular').out_size(3, 4) == (9, 12)
    assert P(padding=(-2, -3, -1, -2)).out_size(4, 6) == (1, 1)
    for make, what in ((lambda: P(MyPad(1)), "not a subclass.*MyPad"),
                       (lambda: P(nn.Conv2d(3, 3, 1)), "nn.ReflectionPad2d.*got Conv2d"),
                       (lambda: P(nn.ReflectionPad1d(1)), "got ReflectionPad1d"),
                       (lambda: P(nn.ZeroPad2d(1), padding=1), "not both"),
                       (lambda: P(nn.ZeroPad2d(1), mode='reflect'), "not both"),
                       (lambda: P(nn.ZeroPad2d(1), value=1.0), "not both"),
                       (lambda: P(), "padding=None"),
                       (lambda: P(padding=(1, 2)), r"padding=\(1, 2\) pads 1 dimension"),
                       (lambda: P(padding=(1, 2, 3, 4, 5, 6)), r"padding=\(1, 2, 3, 4, 5, 6\) pads 3 dimensions"),
                       (lambda: P(padding=(1, 2, 3)), r"padding=\(1, 2, 3\)"),
                       (lambda: P(padding=1.0), "padding=1.0"),
                       (lambda: P(padding=(1, 1, 1.5, 1)), "padding="),
                       (lambda: P(padding=True), "padding=True"),
                       (lambda: P(padding=(1, 1, True, 1)), "padding="),
                       (lambda: P(padding=65), r"padding=\(65, 65, 65, 65\) is beyond"),
                       (lambda: P(padding=(0, 0, -65, 0)), "is beyond"),
                       (lambda: P(nn.ReflectionPad2d(65)), "is beyond"),
                       (lambda: P(padding=(1, -1, 1, 1), mode='reflect'), "negative pad.*'constant' only"),
                       (lambda: P(padding=(1, 1, 1, -2), mode='replicate'), "mode='replicate'.*negative pad"),
                       (lambda: P(padding=(-1, 1, 1, 1), mode='circular'), "negative pad"),
                       (lambda: P(padding=1, mode='zeros'), "mode='zeros'"),
                       (lambda: P(padding=1, mode='symmetric'), "mode='symmetric'"),
                       (lambda: P(padding=1, mode=None), "mode=None"),
                       (lambda: P(padding=1, value='0'), "value='0'"),
                       (lambda: P(padding=1, value=None), "value=None"),
                       (lambda: P(padding=1, value=True), "value=True"),
                       (lambda: P(padding=1, value=torch.zeros(())), "value=tensor"),
                       # what depends on the map names the map
                       (lambda: P(padding=(4, 0, 0, 0), mode='reflect').out_size(9, 4), "reflect.*9x4 map.*below the extent"),
                       (lambda: P(padding=(0, 0, 0, 3), mode='reflect').out_size(3, 9), "3x9 map"),
                       (lambda: P(padding=(0, 5, 0, 0), mode='circular').out_size(9, 4), "circular.*9x4 map.*exceed"),
                       (lambda: P(padding=(0, 0, -2, -2)).out_size(4, 6), "4x6 map leaves no output pixel"),
                       (lambda: P(padding=(-3, -3, 0, 0)).out_size(4, 6), "leaves no output pixel")):
        with pytest.raises(Err, match=what):
            make()


def test_forward_refusals_without_a_device(pkg, lib, monkeypatch):
    from cbinfer_amd.conv2d_cg import ChangeIndexes
    Err = lib.CBinferError
    pad = pkg.CBPad2d(nn.ReflectionPad2d(2))
    x = torch.zeros(1, 4, 6, 8)
    for inp, what in ((torch.zeros(2, 4, 6, 8), "batch 1"), (torch.zeros(4, 6, 8), r"\[1, C, H, W\]"),
                      (torch.zeros(1, 4, 6, 8, dtype=torch.int32), "float32 and float16"), (x.double(), "float32 and float16"),
                      (('changeIndexes', x), "tuple"), (('indexes', x, None), "tuple"), (None, "must be a tensor"),
                      (x, "HIP devices only")):
        with pytest.raises(Err, match=what):
            pad(inp)
    # a finite value the frame's dtype does not hold: refused before the device is asked for, naming the map
    big = pkg.CBPad2d(padding=1, value=1e6)
    with pytest.raises(Err, match=r"value=1000000.0 of a 6x8 float16 map overflows"):
        big(x.half())
    with pytest.raises(Err, match="HIP devices only"):
        big(x)
    with pytest.raises(Err, match="HIP devices only"):
        pkg.CBPad2d(padding=1, value=float('inf'))(x.half())
    with pytest.raises(Err, match="float32 map overflows"):
        pkg.CBPad2d(padding=1, value=1e39)(x)
    # the limits that depend on the map, and indexes of another map size or type (chain.operand_changes): their only need
    # of a device is the module's workspace -- the device check is taken out of the way, nothing is launched
    import cbinfer_amd.pad as mod
    monkeypatch.setattr(mod, 'require_device', lambda *tensors: None)
    with pytest.raises(Err, match="reflect.*2x8 map"):
        pad(torch.zeros(1, 4, 2, 8))
    with pytest.raises(Err, match="circular.*6x8 map"):
        pkg.CBPad2d(nn.CircularPad2d(7))(x)
    with pytest.raises(Err, match="leaves no output pixel"):
        pkg.CBPad2d(nn.ZeroPad2d((-4, -4, 0, 0)))(x)
    wrong = ChangeIndexes(torch.zeros(4, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), (7, 8))
    with pytest.raises(Err, match="CBPad2d.*7x8 map.*6x8"):
        pad(('changeIndexes', x, wrong))
    with pytest.raises(Err, match="CBPad2d.*int32 tensor or a ChangeIndexes"):
        pad(('changeIndexes', x, [1, 2]))
    with pytest.raises(Err, match="CBPad2d.*contiguous one-dimensional int32"):
        pad(('changeIndexes', x, torch.zeros(3, dtype=torch.int64)))
    assert pad.outputState.numel() == 0


# ------------------------------------------------------------------------------------------------ the C ABI
def pd_struct(lib, mode=0, pads=(1, 1, 1, 1), value=0.0):
    return ctypes.pointer(lib.Pad(mode, *(tuple(pads) + (value,))))


def test_supported_and_out_size_over_the_limits(lib):
    C = lib.C
    CO, RF, RP, CI = lib.PAD_CONSTANT, lib.PAD_REFLECT, lib.PAD_REPLICATE, lib.PAD_CIRCULAR
    assert (CO, RF, RP, CI) == (pc.CONSTANT, pc.REFLECT, pc.REPLICATE, pc.CIRCULAR) == (0, 1, 2, 3)
    assert ctypes.sizeof(lib.Pad) == 24
    assert [f for f, _ in lib.Pad._fields_] == ['mode', 'left', 'right', 'top', 'bottom', 'value']

    def size(mode, pads, H, W, p=True):
        ho, wo = ctypes.c_int(-7), ctypes.c_int(-7)
        st = C.cbinfer_pad_out_size(pd_struct(lib, mode, pads) if p else None, H, W, ctypes.byref(ho), ctypes.byref(wo))
        return st, (ho.value, wo.value)

    for case in pc.CASES:
        mode, pads, (Cn, H, W) = case
        k = pc.MODES.index(mode)
        assert C.cbinfer_pad_supported(pd_struct(lib, k, pads), H, W) == 1, case
        assert size(k, pads, H, W) == (0, pc.out_shape(pads, (Cn, H, W))[1:]), case
    good = [(CO, (64, 64, 64, 64), 1, 1), (CO, (-64, -64, -64, -64), 129, 129), (RF, (8, 8, 4, 4), 5, 9),
            (RP, (64, 64, 64, 64), 1, 1), (CI, (9, 9, 5, 5), 5, 9), (CI, (0, 0, 0, 0), 1, 1), (RF, (0, 0, 0, 0), 1, 1),
            (CO, (0, 0, 0, 0), 1 << 20, 1 << 20)]
    for mode, pads, H, W in good:
        assert C.cbinfer_pad_supported(pd_struct(lib, mode, pads), H, W) == 1, (mode, pads, H, W)
    assert C.cbinfer_pad_supported(pd_struct(lib, CO, (1, 1, 1, 1), float('nan')), 4, 4) == 1
    untouched = (-7, -7)
    bad = [(4, (1, 1, 1, 1), 4, 4), (-1, (1, 1, 1, 1), 4, 4),                              # an unknown mode
           (CO, (65, 0, 0, 0), 4, 4), (CO, (0, 0, 0, -65), 200, 200), (RP, (0, 65, 0, 0), 4, 4),      # beyond 64
           (RF, (-1, 1, 1, 1), 4, 4), (RP, (1, 1, -1, 1), 4, 4), (CI, (1, 1, 1, -1), 4, 4),         # a crop outside constant
           (RF, (4, 0, 0, 0), 9, 4), (RF, (0, 4, 0, 0), 9, 4), (RF, (0, 0, 4, 0), 4, 9), (RF, (0, 0, 0, 4), 4, 9),
           (RF, (1, 0, 0, 0), 1, 1),                                                         # reflect: pad >= n
           (CI, (5, 0, 0, 0), 9, 4), (CI, (0, 0, 0, 5), 4, 9),                                # circular: pad > n
           (CO, (-2, -2, 0, 0), 4, 4), (CO, (0, 0, -1, -3), 4, 4), (CO, (-64, -64, 0, 0), 4, 128)]      # no output pixel
    for mode, pads, H, W in bad:
        assert C.cbinfer_pad_supported(pd_struct(lib, mode, pads), H, W) == 0, (mode, pads, H, W)
        assert size(mode, pads, H, W) == (-2, untouched), (mode, pads, H, W)
    assert C.cbinfer_pad_supported(None, 4, 4) == 0
    assert C.cbinfer_pad_supported(pd_struct(lib), 0, 4) == 0 and C.cbinfer_pad_supported(pd_struct(lib), 4, -1) == 0
    assert size(CO, (1, 1, 1, 1), 4, 4, p=False) == (-1, untouched)
    assert size(CO, (1, 1, 1, 1), 0, 4) == (-1, untouched) and size(CO, (1, 1, 1, 1), 4, 0) == (-1, untouched)
    assert C.cbinfer_pad_out_size(pd_struct(lib), 4, 4, None, None) == -1


def test_c_entry_point_checks_its_arguments(lib):
    """Bad arguments return CB_ERR_BADARG (-1) before anything is launched (the device pointers here are never
    followed)."""
    C = lib.C
    assert C.cbinfer_abi_version() == 11
    assert C.cbinfer_cbpad_forward.launcher and not C.cbinfer_pad_out_size.launcher and not C.cbinfer_pad_supported.launcher
    CO, RF, RP, CI = lib.PAD_CONSTANT, lib.PAD_REFLECT, lib.PAD_REPLICATE, lib.PAD_CIRCULAR
    X, O, BITS, COPY, M, L, N2 = (0x10000 * i for i in range(1, 8))

    def go(x=X, o=O, mask=None, lst=None, cap=0, count=None, bits=BITS, cp=COPY, Cn=3, H=4, W=6, p=(RF, (1, 1, 1, 1)),
           dt=lib.CB_F32):
        return C.cbinfer_cbpad_forward(x, o, mask, lst, cap, count, bits, cp, Cn, H, W,
                                       pd_struct(lib, *p) if p is not None else None, dt, None)

    for bad in (dict(x=None), dict(o=None), dict(o=X), dict(bits=None), dict(cp=None), dict(cp=BITS), dict(p=None),
                dict(Cn=0), dict(H=0), dict(W=-1), dict(dt=lib.CB_F32S), dict(dt=7), dict(lst=L, cap=-1),
                dict(mask=M, lst=L), dict(count=N2), dict(mask=BITS), dict(mask=COPY),
                # the mode and the limits
                dict(p=(4, (1, 1, 1, 1))), dict(p=(-1, (1, 1, 1, 1))), dict(p=(CO, (65, 0, 0, 0))),
                dict(p=(CO, (0, 0, 0, -65))), dict(p=(RP, (0, 0, 65, 0))), dict(p=(RF, (-1, 1, 1, 1))),
                dict(p=(RP, (1, 1, 1, -1))), dict(p=(CI, (1, -2, 1, 1))), dict(p=(RF, (6, 0, 0, 0))),
                dict(p=(RF, (0, 0, 0, 4))), dict(p=(CI, (0, 7, 0, 0))), dict(p=(CI, (0, 0, 5, 0))),
                dict(p=(CO, (-3, -3, 0, 0))), dict(p=(CO, (0, 0, -4, 0))),
                # H W, Ho Wo or 64 C beyond an int32
                dict(p=(CO, (0, 0, 0, 0)), H=1 << 16, W=1 << 15), dict(p=(CO, (64, 64, 0, 0)), H=1 << 16, W=(1 << 15) - 128),
                dict(Cn=1 << 25)):
        assert go(**bad) == -1, bad


# ------------------------------------------------------------------------------------------------ splitConvPadding
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("mode", ["reflect", "replicate", "circular"])
def test_split_conv_padding_is_torchs_own_forward(pkg, mode, bias):
    torch.manual_seed(3)
    seq = nn.Sequential()
    seq.add_module('stem', nn.Conv2d(3, 8, 3, padding=(1, 2), padding_mode=mode, bias=bias))
    seq.add_module('act', nn.ReLU())
    seq.add_module('same', nn.Conv2d(8, 8, (3, 5), padding='same', dilation=(2, 1), padding_mode=mode, bias=bias))
    seq.add_module('zeros', nn.Conv2d(8, 4, 3, padding=1, bias=bias))
    seq.add_module('inner', nn.Sequential(nn.Conv2d(4, 4, 3, stride=2, padding=1, padding_mode=mode, bias=bias)))
    seq.eval()
    orig = copy.deepcopy(seq)
    keys = list(seq.state_dict().keys())
    params = {n: p for n, p in seq.named_parameters()}
    zeros = seq.zeros
    rng = torch.get_rng_state()
    assert pkg.splitConvPadding(seq) is seq
    assert torch.equal(rng, torch.get_rng_state())      # (the new layers draw no initial weights)
    assert list(seq._modules) == ['stem_pad', 'stem', 'act', 'same_pad', 'same', 'zeros', 'inner']
    assert list(seq.inner._modules) == ['0_pad', '0']
    padType = {'reflect': nn.ReflectionPad2d, 'replicate': nn.ReplicationPad2d, 'circular': nn.CircularPad2d}[mode]
    assert type(seq.stem_pad) is padType and tuple(seq.stem_pad.padding) == (2, 2, 1, 1)
    assert type(seq.same_pad) is padType and tuple(seq.same_pad.padding) == (2, 2, 2, 2)
    assert type(seq.inner[0]) is padType and tuple(seq.inner[0].padding) == (1, 1, 1, 1)
    for conv, old in ((seq.stem, orig.stem), (seq.same, orig.same), (seq.inner[1], orig.inner[0])):
        assert type(conv) is nn.Conv2d and conv.padding == (0, 0) and conv.padding_mode == 'zeros' and not conv.training
        assert (conv.in_channels, conv.out_channels, conv.kernel_size, conv.stride, conv.dilation, conv.groups) == (
            old.in_channels, old.out_channels, old.kernel_size, old.stride, old.dilation, old.groups)
        assert (conv.bias is None) == (not bias)
    assert seq.zeros is zeros and seq.zeros.padding == (1, 1)
    assert list(seq.state_dict().keys()) == keys
    assert all(p is params[n] for n, p in seq.named_parameters()) and len(params) == len(list(seq.named_parameters()))
    x = torch.randn(1, 3, 9, 11)
    with torch.no_grad():
        assert same_bits(seq(x).numpy(), orig(x).numpy())
    # a second call finds nothing left
    before = list(seq._modules)
    pkg.splitConvPadding(seq)
    assert list(seq._modules) == before


def test_split_conv_padding_leaves_collides_and_feeds_convert(pkg, lib):
    Err = lib.CBinferError
    # an odd-total 'same', a subclass and a conv outside an nn.Sequential are left alone
    class MyConv(nn.Conv2d):
        pass

    class Holder(nn.Module):
        def __init__(self):
            super(Holder, self).__init__()
            self.conv = nn.Conv2d(3, 3, 3, padding=1, padding_mode='reflect')
            self.seq = nn.Sequential(nn.Conv2d(3, 3, 4, padding='same', padding_mode='reflect'),
                                     MyConv(3, 3, 3, padding=1, padding_mode='reflect'),
                                     nn.Conv2d(3, 3, 3, padding='valid', padding_mode='reflect'))
    h = Holder()
    kids = list(h.seq)
    pkg.splitConvPadding(h)
    assert list(h.seq) == kids and h.conv.padding_mode == 'reflect'
    # the name collision names both
    seq = nn.Sequential()
    seq.add_module('c', nn.Conv2d(3, 3, 3, padding=1, padding_mode='replicate'))
    seq.add_module('c_pad', nn.ReLU())
    with pytest.raises(Err, match="splitConvPadding: .*'c'.*'c_pad'"):
        pkg.splitConvPadding(seq)
    assert list(seq._modules) == ['c', 'c_pad'] and seq.c.padding_mode == 'replicate'
    # without the split convert() raises as before; with it the layers convert and the pads join the chain

    def make():
        torch.manual_seed(4)
        return nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), nn.ReLU(), nn.Conv2d(8, 8, 3, padding=1, padding_mode='replicate'),
                             nn.ReLU(), nn.Conv2d(8, 4, 3, padding=(1, 2), padding_mode='circular')).eval()
    with pytest.raises(Err, match="padding_mode='replicate'"):
        pkg.convert(make(), threshold=0.05, generalGeometry=True)
    for make_cb in (lambda m: pkg.CBConv2d(m(1), 0.1, generalGeometry=True), lambda m: pkg.CBDepthwiseConv2d(m(4), 0.1),
                    lambda m: pkg.CBGroupedConv2d(m(2), 0.1)):      # the constructors keep their refusals
        with pytest.raises(Err, match="padding_mode='reflect'"):
            make_cb(lambda groups: nn.Conv2d(4, 4, 3, padding=1, padding_mode='reflect', groups=groups))
    net = pkg.convert(pkg.splitConvPadding(make()), threshold=0.05, generalGeometry=True)
    assert names_of(net) == ['CBConv2d', 'ReplicationPad2d', 'CBConv2d', 'CircularPad2d', 'CBConv2d']
    assert list(net._modules) == ['0', '2_pad', '2', '4_pad', '4']
    assert tuple(net[2].padding) == (0, 0) and net[2].withReLU and tuple(net[4].padding) == (0, 0)
    pkg.insertCBPadding(net)
    assert names_of(net) == ['CBConv2d', 'CBPad2d', 'CBConv2d', 'CBPad2d', 'CBConv2d']
    assert (net[1].mode, net[1].padding, net[3].mode, net[3].padding) == ('replicate', (1, 1, 1, 1), 'circular', (2, 2, 1, 1))
    assert net[0].propChangeIndexes and net[2].propChangeIndexes and net[2].copyInput and net[4].copyInput


# ------------------------------------------------------------------------------------------------ insertCBPadding
def test_insert_padding_wiring_and_what_it_leaves(pkg, lib):
    from cbinfer_amd import chain
    matrix = [chain.producers(name) for name in chain.PASSES]
    # a monodepth2-type run: conv -> ReflectionPad2d -> valid 3x3 conv -> ZeroPad2d -> 1x1 conv
    torch.manual_seed(1)
    seq = nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), nn.ReLU(), nn.ReflectionPad2d(1), nn.Conv2d(8, 8, 3), nn.ReLU(),
                        nn.ZeroPad2d((1, 0, 1, 0)), nn.Conv2d(8, 4, 1)).eval()
    net = pkg.convert(seq, threshold=0.05, generalGeometry=True)
    assert names_of(net) == ['CBConv2d', 'ReflectionPad2d', 'CBConv2d', 'ZeroPad2d', 'CBConv2d']
    net[2].copyInput = False
    assert pkg.insertCBPadding(net, cloneOutput=False) is net
    assert names_of(net) == ['CBConv2d', 'CBPad2d', 'CBConv2d', 'CBPad2d', 'CBConv2d']
    assert list(net._modules) == ['0', '2', '3', '5', '6']
    assert (net[1].mode, net[1].padding, net[1].cloneOutput, net[1].propChangeIndexes) == ('reflect', (1, 1, 1, 1), False, False)
    assert (net[3].mode, net[3].padding, net[3].cloneOutput, net[3].propChangeIndexes) == ('constant', (1, 0, 1, 0), False, True)
    assert net[0].propChangeIndexes and net[2].propChangeIndexes and net[2].copyInput is True and not net[4].propChangeIndexes
    # a feedback-mode consumer keeps no input reference
    net = pkg.convert(nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), nn.ReplicationPad2d(1), nn.Conv2d(8, 3, 3)).eval(),
                      threshold=0.05, generalGeometry=True)
    net[2].copyInput, net[2].feedbackLoop = False, True
    pkg.insertCBPadding(net)
    assert type(net[1]) is pkg.CBPad2d and net[1].cloneOutput and net[2].copyInput is False and not net[1].propChangeIndexes
    # behind a pointwise function, a grouped conv, a resize, a channel reduction and another pad
    torch.manual_seed(2)
    seq = nn.Sequential(nn.Conv2d(4, 8, 3, padding=1, groups=2), nn.CircularPad2d(2), nn.ConstantPad2d((0, 1, 0, 1), 0.5),
                        nn.Tanh(), nn.ReplicationPad2d(1), nn.Upsample(size=(9, 9)), nn.ZeroPad2d((-1, -1, 0, 0)),
                        nn.Softmax2d(), nn.ReflectionPad2d(2)).eval()
    net = pkg.convert(seq, threshold=0.05, grouped=True)
    pkg.insertCBPadding(net)
    assert names_of(net) == ['CBGroupedConv2d', 'CBPad2d', 'CBPad2d', 'Tanh', 'ReplicationPad2d', 'Upsample', 'ZeroPad2d',
                             'Softmax2d', 'ReflectionPad2d']
    assert net[0].propChangeIndexes and net[1].propChangeIndexes and not net[2].propChangeIndexes and net[2].value == 0.5
    pkg.insertCBPointwise(net)
    pkg.insertCBPadding(net)
    pkg.insertCBResize(net)
    pkg.insertCBPadding(net)
    pkg.insertCBChannelOps(net)
    pkg.insertCBPadding(net)
    assert names_of(net) == ['CBGroupedConv2d', 'CBPad2d', 'CBPad2d', 'CBPointwise2d', 'CBPad2d', 'CBResize2d', 'CBPad2d',
                             'CBChannelReduce2d', 'CBPad2d']
    assert all(m.propChangeIndexes for m in list(net)[:-1]) and not net[8].propChangeIndexes
    assert net[6].padding == (-1, -1, 0, 0)
    # behind a non-producer, at the front of a container, beyond the limits or a subclass: dense, flags untouched
    seq = nn.Sequential(nn.ReflectionPad2d(3), nn.Conv2d(3, 8, 7), nn.ZeroPad2d(65), nn.Conv2d(8, 8, 1), nn.Tanh(),
                        nn.ReflectionPad2d(1), nn.Conv2d(8, 8, 1), MyPad(1), nn.Conv2d(8, 8, 1), nn.ReflectionPad1d(1),
                        nn.Sequential(nn.ZeroPad2d(1))).eval()
    net = pkg.convert(seq, threshold=0.05, generalGeometry=True)
    before = names_of(net)
    flags = [getattr(m, 'propChangeIndexes', None) for m in net]
    pkg.insertCBPadding(net)
    assert names_of(net) == before == ['ReflectionPad2d', 'CBConv2d', 'ZeroPad2d', 'CBConv2d', 'Tanh', 'ReflectionPad2d',
                                       'CBConv2d', 'MyPad', 'CBConv2d', 'ReflectionPad1d', 'Sequential']
    assert [getattr(m, 'propChangeIndexes', None) for m in net] == flags and not any(f for f in flags)
    assert type(net[10][0]) is nn.ZeroPad2d
    # the producer matrix is as it was (what it holds: test_host_chain.py)
    assert matrix == [chain.producers(name) for name in chain.PASSES]


def test_the_other_passes_accept_the_module_as_a_producer(pkg, lib):
    from cbinfer_amd import chain
    P = pkg.CBPad2d
    # every pass but the 2x2 pooling of the reference's kind (every pass's whole set, in order: test_host_chain.py)
    assert [name for name in chain.PASSES if P not in chain.producers(name)] == ['insertCBPooling']

    def behind(*mods):
        net = nn.Sequential(P(nn.ReflectionPad2d(1)))
        for k, m in enumerate(mods):
            net.add_module('m%d' % k, m)
        return net.eval()
    net = pkg.insertCBPointwise(behind(nn.ReLU()))
    assert type(net.m0) is pkg.CBPointwise2d and net[0].propChangeIndexes
    net = pkg.insertCBUpsampling(behind(nn.Upsample(scale_factor=2)))
    assert type(net.m0) is pkg.CBUpsample2d and net[0].propChangeIndexes
    net = pkg.insertCBResize(behind(nn.Upsample(size=(9, 11), mode='bilinear')))
    assert type(net.m0) is pkg.CBResize2d and net[0].propChangeIndexes
    net = pkg.insertCBRearrange(behind(nn.PixelShuffle(2)))
    assert type(net.m0) is pkg.CBPixelShuffle2d and net[0].propChangeIndexes
    net = pkg.insertCBChannelOps(behind(nn.Softmax2d()))
    assert type(net.m0) is pkg.CBChannelReduce2d and net[0].propChangeIndexes
    net = pkg.insertCBPadding(behind(nn.ZeroPad2d(1)))
    assert type(net.m0) is P and net[0].propChangeIndexes
    net = pkg.insertCBTransposedConv(behind(nn.ConvTranspose2d(4, 4, 2, stride=2)), threshold=0.05)
    assert type(net.m0) is pkg.CBConvTranspose2d      # (it runs its own detection: nothing is switched on)
    net = pkg.convert(behind(nn.Conv2d(4, 4, 3, padding=1, groups=4)), threshold=0.05, depthwise=True)
    assert type(net.m0) is pkg.CBDepthwiseConv2d and not net[0].propChangeIndexes
    pkg.linkDepthwise(net)
    assert net[0].propChangeIndexes
    # insertCBPooling builds its own set: the general pools take the module's mask, the reference's 2x2 pool does not
    net = pkg.insertCBPooling(behind(nn.MaxPool2d(3, 2, 1)), generalGeometry=True)
    assert type(net.m0) is pkg.CBPoolMax2d and net[0].propChangeIndexes
    net = pkg.insertCBPooling(behind(nn.MaxPool2d(2, 2)))
    assert type(net.m0) is nn.MaxPool2d and not net[0].propChangeIndexes


# ------------------------------------------------------------------------------------------------ module hygiene
def test_exports_state_helpers_and_pickling(pkg, lib):
    import cbinfer_amd
    assert all(n in pkg.__all__ for n in ('CBPad2d', 'insertCBPadding', 'splitConvPadding'))
    assert pkg.pad is cbinfer_amd.pad
    import pycbinfer.pad as alias
    assert alias is cbinfer_amd.pad and pkg.CBPad2d is alias.CBPad2d
    assert pkg.insertCBPadding is alias.insertCBPadding and pkg.splitConvPadding is alias.splitConvPadding
    assert {'cbinfer_pad_supported', 'cbinfer_pad_out_size', 'cbinfer_cbpad_forward'} <= set(lib.EXPORTED_SYMBOLS)
    pd = pkg.CBPad2d(padding=(1, 2, 0, 3), mode='replicate')
    cp = pkg.CBPad2d(nn.ConstantPad2d((-1, 2, 2, -1), -3.5))
    pd.propChangeIndexes, pd.cloneOutput = True, False
    net = nn.Sequential(pd, cp)
    pd.outputState, cp.outputState = torch.ones(1, 2, 6, 9), torch.ones(1, 2, 7, 10)
    for m in (pd, cp):
        m._struct()
        m.__dict__['_work'] = {'key': None}
    states = pkg.getStateTensors(net)
    assert len(states) == 2 and all(any(t is m.outputState for t in states) for m in (pd, cp))
    for clone in (pickle.loads(pickle.dumps(net)), copy.deepcopy(net)):
        a, b = clone[0], clone[1]
        assert type(a) is pkg.CBPad2d and type(b) is pkg.CBPad2d
        assert (a.padding, a.mode, a.value, a.propChangeIndexes, a.cloneOutput) == ((1, 2, 0, 3), 'replicate', 0.0, True, False)
        assert (b.padding, b.mode, b.value, b.propChangeIndexes, b.cloneOutput) == ((-1, 2, 2, -1), 'constant', -3.5, False, True)
        for new, old in ((a, pd), (b, cp)):
            assert new._work is None and new._pdC is None      # transients dropped ...
            assert torch.equal(new.outputState, old.outputState) and repr(new) == repr(old)      # ... state kept
            s, t = new._struct().contents, old._struct().contents
            assert (s.mode, s.left, s.right, s.top, s.bottom, s.value) == (t.mode, t.left, t.right, t.top, t.bottom, t.value)
            assert new.out_size(4, 8) == old.out_size(4, 8)
    pkg.clearMemory(net)
    for m in (pd, cp):
        assert m.outputState.numel() == 0 and m._work is None


def test_batch_branch_and_program_refusals_name_the_module(pkg, lib):
    net = nn.Sequential()
    net.add_module('stem', pkg.convert(nn.Sequential(nn.Conv2d(3, 8, 3, padding=1)).eval(), threshold=0.05)[0])
    net.add_module('pad', pkg.CBPad2d(nn.ReflectionPad2d(1)))
    with pytest.raises(lib.CBinferError, match=r"SequenceBatch: layer 'pad' is CBPad2d \(padding=\(1, 1, 1, 1\), "
                                               r"mode=reflect.*a change-based padding.*reflection-padded and restoration"):
        pkg.SequenceBatch(net, 2)
    with pytest.raises(lib.CBinferError, match=r"BranchGroup: layer '0.pad' is CBPad2d \(.*a change-based padding"):
        pkg.BranchGroup([net])
    from cbinfer_amd import batch
    assert [row for row in batch.CHAIN_OPERATORS if pkg.CBPad2d in row[0]] == [
        ((pkg.CBPad2d,), 'a change-based padding', 'reflection-padded and restoration')]
    # FrameProgram's refusal of a frame that ran a torch operator names the module and its pass, and keeps what it said
    import cbinfer_amd.program as program
    said = inspect.getsource(pkg.FrameProgram)
    assert "pycbinfer.CBPad2d (insertCBPadding) for an explicit padding" in said
    assert "pycbinfer.CBResize2d (insertCBResize)" in said and "CBUpsample2d / CBConcat2d" in said
    assert 'CBPad2d' in program.__doc__
