"""CPU-only tests of change-based pooling for any window: the constructors and their limits, the output
size rule against torch, the conversion helper, the state helpers and pickling.  No kernel is launched here."""
import ctypes
import pickle

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F
from optest import lib, pkg      # noqa: F401  (fixtures)


def test_constructors_and_limits(pkg, lib):
    Err = lib.CBinferError
    with pytest.raises(AssertionError):
        pkg.CBPoolMax2d(nn.MaxPool2d(3, 2, 1))
    m = pkg.CBPoolMax2d(nn.MaxPool2d(3, 2, 1, ceil_mode=True), generalGeometry=True)
    assert m._general and not m.lazy and m.propChangeIndexes is False and m.cloneOutput is True
    r = repr(m)
    for part in ("CBPoolMax2d", "(3, 3)", "(2, 2)", "(1, 1)", "ceil_mode=True"):
        assert part in r, r
    # a 2x2 / stride 2 / no padding max pool runs as it always did, with or without the flag
    assert not pkg.CBPoolMax2d(nn.MaxPool2d(2, 2), generalGeometry=True)._general
    assert pkg.CBPoolMax2d(nn.MaxPool2d(2, 2, 1), generalGeometry=True)._general
    for bad in (nn.MaxPool2d(3, 2, 1, dilation=2), nn.MaxPool2d(3, 2, 1, return_indices=True), nn.MaxPool2d(9),
                nn.MaxPool2d(3, 9), nn.MaxPool2d(3, 2, 2), nn.MaxPool2d((3, 9), 1), nn.AvgPool2d(3, 2, 1)):
        with pytest.raises(Err):
            pkg.CBPoolMax2d(bad, generalGeometry=True)
    a = pkg.CBPoolAvg2d(nn.AvgPool2d((3, 2), (2, 1), (1, 0), count_include_pad=False))
    assert a._general and a._op == lib.POOL_AVG_NOPAD and a.kernel_size == (3, 2) and a.stride == (2, 1)
    assert a.padding == (1, 0) and "count_include_pad=False" in repr(a) and "(1, 0)" in repr(a)
    assert pkg.CBPoolAvg2d(nn.AvgPool2d(2))._op == lib.POOL_AVG_PAD      # 2x2 included
    for bad in (nn.AvgPool2d(2, divisor_override=3), nn.AvgPool2d(9), nn.AvgPool2d(2, 9), nn.AvgPool2d(3, 1, 2),
                nn.MaxPool2d(2)):
        with pytest.raises(Err):
            pkg.CBPoolAvg2d(bad)
    assert pkg.CBPoolAvg2d is pkg.conv2d.CBPoolAvg2d and 'CBPoolAvg2d' in pkg.__all__


def _out(lib, n, m, k, s, p, ceil):
    g = lib.Pool(k[0], k[1], s[0], s[1], p[0], p[1], int(ceil), lib.POOL_MAX)
    ho, wo = ctypes.c_int(-7), ctypes.c_int(-7)
    st = lib.C.cbinfer_pool_out_size(n, m, ctypes.byref(g), ctypes.byref(ho), ctypes.byref(wo))
    return st, ho.value, wo.value


def test_out_size_is_torchs(lib):
    cases = 0
    zeros = {n: torch.zeros(1, 1, n, n) for n in range(1, 41)}
    for k in range(1, 9):
        for s in range(1, 9):
            for p in range(0, k // 2 + 1):
                for ceil in (False, True):
                    for n in range(1, 41):
                        if n + 2 * p < k:
                            assert _out(lib, n, n, (k, k), (s, s), (p, p), ceil) == (-1, -7, -7)
                            continue
                        cases += 1
                        ref = F.max_pool2d(zeros[n], k, s, p, ceil_mode=ceil).shape
                        assert _out(lib, n, n, (k, k), (s, s), (p, p), ceil) == (0, ref[-2], ref[-1]), (n, k, s, p, ceil)
    assert cases == 14560
    # the drop rule of ceil mode
    assert _out(lib, 9, 9, (2, 2), (2, 2), (1, 1), True) == (0, 5, 5)
    assert _out(lib, 8, 8, (1, 1), (2, 2), (0, 0), True) == (0, 4, 4)
    for k, s, p in (((3, 2), (2, 1), (1, 0)), ((2, 7), (3, 2), (1, 3)), ((8, 1), (1, 8), (4, 0))):
        for ceil in (False, True):
            for n, m in ((13, 17), (8, 40), (31, 9)):
                ref = F.max_pool2d(torch.zeros(1, 1, n, m), k, s, p, ceil_mode=ceil).shape
                assert _out(lib, n, m, k, s, p, ceil) == (0, ref[-2], ref[-1]), (n, m, k, s, p, ceil)
                ref = F.avg_pool2d(torch.zeros(1, 1, n, m), k, s, p, ceil_mode=ceil).shape
                assert _out(lib, n, m, k, s, p, ceil)[1:] == (ref[-2], ref[-1])
    # a map smaller than the window on ONE axis, a window beyond the limits: a status
    assert _out(lib, 2, 30, (5, 3), (1, 1), (1, 1), False)[0] == -1
    assert _out(lib, 30, 30, (9, 3), (1, 1), (1, 1), False)[0] == -2
    g = lib.Pool(3, 3, 2, 2, 1, 1, 0, lib.POOL_MAX)
    assert lib.C.cbinfer_pool_supported(ctypes.byref(g)) == 1
    for field, val in (("kH", 9), ("sW", 9), ("pH", 2), ("op", 3), ("kW", 0), ("sH", 0), ("pW", -1), ("ceilMode", 2)):
        g = lib.Pool(3, 3, 2, 2, 1, 1, 0, lib.POOL_MAX)
        setattr(g, field, val)
        assert lib.C.cbinfer_pool_supported(ctypes.byref(g)) == 0, field


def _net():
    torch.manual_seed(3)
    return nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), nn.ReLU(), nn.MaxPool2d(3, 2, 1),
                         nn.Conv2d(8, 8, 3, padding=1), nn.AvgPool2d(2),
                         nn.Conv2d(8, 8, 3, padding=1), nn.MaxPool2d(9, 2, 4),
                         nn.Conv2d(8, 4, 3, padding=1), nn.MaxPool2d(2, 2), nn.Conv2d(4, 4, 1)).eval()


def test_insert_cb_pooling(pkg):
    net = pkg.insertCBPooling(pkg.convert(_net(), threshold=0.05))
    kinds = [type(m).__name__ for m in net.children()]
    assert kinds == ['CBConv2d', 'MaxPool2d', 'CBConv2d', 'AvgPool2d', 'CBConv2d', 'MaxPool2d', 'CBConv2d',
                     'CBPoolMax2d', 'CBConv2d'], kinds
    assert not net[0].propChangeIndexes and not net[2].propChangeIndexes

    net = pkg.insertCBPooling(pkg.convert(_net(), threshold=0.05), cloneOutput=False, generalGeometry=True)
    kids = list(net.children())
    kinds = [type(m).__name__ for m in kids]
    assert kinds == ['CBConv2d', 'CBPoolMax2d', 'CBConv2d', 'CBPoolAvg2d', 'CBConv2d', 'MaxPool2d', 'CBConv2d',
                     'CBPoolMax2d', 'CBConv2d'], kinds
    assert kids[1]._general and kids[3]._general and not kids[7]._general
    assert kids[0].propChangeIndexes and kids[2].propChangeIndexes and kids[6].propChangeIndexes
    assert not kids[4].propChangeIndexes      # (the pool beyond the limits stays dense: nobody wants the list)
    assert not kids[1].cloneOutput and not kids[3].cloneOutput and kids[2].copyInput and kids[4].copyInput
    # the fusions never fold such a pool into a detection; the 2x2 one still is
    for m in kids:
        if type(m) is pkg.CBConv2d:
            m.feedbackLoop = True
    pkg.fuseDetectionIntoProducer(pkg.fusePoolingIntoDetection(net))
    assert not kids[1].lazy and not kids[3].lazy and kids[7].lazy
    assert '_fusedNext' not in kids[0].__dict__ and '_fusedNext' not in kids[2].__dict__
    with pytest.raises(pkg.conv2d_cg.CBinferError, match=r"layer '2' is CBPoolMax2d \(k=\(3, 3\)"):
        pkg.SequenceBatch(net, 2)
    # the state helpers reach a CBPoolAvg2d
    avg = kids[3]
    avg.outputState = torch.ones(1, 8, 3, 3)
    assert any(t is avg.outputState for t in pkg.getStateTensors(net))
    pkg.clearMemory(net)
    assert avg.outputState.numel() == 0 and avg._poolWork is None
    from cbinfer_amd import evalTools
    assert [type(m).__name__ for m in evalTools.getCBpoolLayers(net)] == ['CBPoolMax2d', 'CBPoolAvg2d', 'CBPoolMax2d']


class _AsPickledBefore(object):
    """Pickles `module` as a version without the general path did: the state lacks the new attributes."""
    NEW = ('generalGeometry', '_general', 'padding', '_op', '_poolC', '_poolWork')

    def __init__(self, module):
        self.module = module

    def __reduce__(self):
        state = {k: v for k, v in self.module.__dict__.items() if k not in self.NEW}
        return object.__new__, (type(self.module),), state


def test_pickle_round_trip(pkg, lib):
    mx = pkg.CBPoolMax2d(nn.MaxPool2d(3, 2, 1, ceil_mode=True), generalGeometry=True)
    mx.propChangeIndexes = True
    mx._pool_struct()      # (a ctypes pointer cannot be pickled: it must not travel)
    av = pkg.CBPoolAvg2d(nn.AvgPool2d(2, count_include_pad=False))
    av.cloneOutput = False
    for m in (mx, av):
        c = pickle.loads(pickle.dumps(m))
        assert type(c) is type(m) and repr(c) == repr(m)
        for name in ('kernel_size', 'stride', 'padding', 'ceil_mode', '_op', '_general', 'generalGeometry',
                     'propChangeIndexes', 'cloneOutput'):
            assert getattr(c, name) == getattr(m, name), name
        assert c._poolC is None and c._poolWork is None and c.outputState.numel() == 0
        g = c._pool_struct().contents
        assert (g.kH, g.sH, g.pH, g.ceilMode, g.op) == (m.kernel_size[0], m.stride[0], m.padding[0],
                                                        int(m.ceil_mode), m._op)
    old = pickle.loads(pickle.dumps(_AsPickledBefore(pkg.CBPoolMax2d(nn.MaxPool2d(2, 2, ceil_mode=True)))))
    assert type(old) is pkg.CBPoolMax2d and 'padding' in old.__dict__
    assert (old.generalGeometry, old._general, old.padding, old._op) == (False, False, (0, 0), lib.POOL_MAX)
    assert old.ceil_mode and old.kernel_size == (2, 2) and 'p=' not in repr(old)
