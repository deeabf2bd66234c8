"""CPU-only tests of where the pooling modules live and what they are made of: cbinfer_amd/pool.py, on
chain.CBStateModule, reachable under every class path a pickle may name.  No kernel is launched here."""
import copy
import io
import os
import pickle

import pytest
import torch
import torch.nn as nn
from optest import pkg      # noqa: F401  (fixtures)

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'pool_modules_parent.pkl')
# what test_host_pool.test_pickle_round_trip compares, and the members of the other forms
ATTRS = ('kernel_size', 'stride', 'padding', 'ceil_mode', '_op', '_general', 'generalGeometry', 'propChangeIndexes',
         'cloneOutput', '_adaptive', 'downsampleIndexes', 'lazy')


def _modules(pkg):
    """The five modules of the fixture, as the commit before pool.py pickled them (run there, CPU only):

        mods = _modules(pycbinfer)
        assert type(mods[0]).__module__ == 'cbinfer_amd.conv2d'
        with open('tests/golden/pool_modules_parent.pkl', 'wb') as f:
            pickle.dump(mods, f, protocol=2)
    """
    mods = [pkg.CBPoolMax2d(nn.MaxPool2d(2, 2)),
            pkg.CBPoolMax2d(nn.MaxPool2d(3, 2, 1, ceil_mode=True), generalGeometry=True),
            pkg.CBPoolAvg2d(nn.AvgPool2d(2, count_include_pad=False)),
            pkg.CBPoolAvg2d(nn.AdaptiveAvgPool2d(1)),
            pkg.CBPoolMax2d(nn.AdaptiveMaxPool2d((2, None)), generalGeometry=True)]
    mods[0].propChangeIndexes = mods[0].downsampleIndexes = True
    mods[1].cloneOutput = False
    mods[1]._pool_struct()      # (a ctypes pointer cannot be pickled: it must not travel)
    mods[3].outputState = torch.arange(3.0).view(1, 3, 1, 1)
    mods[3].partials = torch.arange(12.0).view(3, 1, 4)
    return mods


def _assert_same(got, want):
    assert type(got) is type(want) and repr(got) == repr(want)
    for name in ATTRS:
        assert getattr(got, name) == getattr(want, name), name
    assert getattr(got, 'output_size', None) == getattr(want, 'output_size', None)
    assert getattr(got, 'count_include_pad', None) == getattr(want, 'count_include_pad', None)
    assert list(got._buffers) == ['outputState', 'partials']
    for name in got._buffers:
        a, b = getattr(got, name), getattr(want, name)
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), name
    assert got.__dict__['_poolC'] is None and got.__dict__['_poolWork'] is None
    assert len(got.getStateTensors()) == len(want.getStateTensors())


def test_class_paths_are_one_class(pkg):
    import cbinfer_amd
    import cbinfer_amd.conv2d
    import cbinfer_amd.pool
    import pycbinfer.conv2d
    import pycbinfer.pool
    from cbinfer_amd import chain
    from cbinfer_amd.conv2d import LazyPool
    assert pycbinfer.pool is cbinfer_amd.pool and LazyPool is cbinfer_amd.pool.LazyPool
    for name in ('CBPoolMax2d', 'CBPoolAvg2d'):
        cls = getattr(cbinfer_amd.pool, name)
        for where in (cbinfer_amd, cbinfer_amd.conv2d, pkg, pkg.conv2d, pycbinfer.conv2d, pycbinfer.pool):
            assert getattr(where, name) is cls, (where.__name__, name)
        assert cls.__module__ == 'cbinfer_amd.pool' and issubclass(cls, chain.CBStateModule)
        assert (cls._WORK, cls._TRANSIENT) == ('_poolWork', ('_poolC',))
    for m in _modules(pkg):
        assert type(m).__module__ == 'cbinfer_amd.pool'
    # conv2d.py defines no pool any more, and keeps the convolution helper its siblings import
    defined = [n for n, v in vars(cbinfer_amd.conv2d).items() if getattr(v, '__module__', None) == 'cbinfer_amd.conv2d']
    assert '_padding_pair' in defined and not [n for n in defined if 'ool' in n], defined


def test_forward_takes_what_a_state_module_takes(pkg):
    """tests/test_gpu_chain.py feeds every CBStateModule a bare tensor for "every pixel listed" (there against the list
    form, bit for bit): a pool gets as far as the device check with one; anything else is the AssertionError it was."""
    from cbinfer_amd._lib import CBinferError
    for m in _modules(pkg):
        with pytest.raises(CBinferError, match="HIP devices only"):
            m(torch.zeros(1, 2, 6, 6))
        for bad in (None, [torch.zeros(1, 2, 6, 6)], ('indexes', torch.zeros(1, 2, 6, 6), None)):
            with pytest.raises(AssertionError):
                m(bad)


def test_a_pickle_of_the_parent_commit_loads(pkg):
    with open(FIXTURE, 'rb') as f:
        data = f.read()
    assert b'cbinfer_amd.conv2d' in data and b'cbinfer_amd.pool' not in data and len(data) < 8192
    loaded = pickle.loads(data)
    fresh = _modules(pkg)
    assert len(loaded) == len(fresh) == 5
    for got, want in zip(loaded, fresh):
        _assert_same(got, want)
    assert loaded[3].outputState.numel() == 3 and loaded[3].partials.numel() == 12
    g = loaded[1]._pool_struct().contents      # (made again on demand)
    assert (g.kH, g.sH, g.pH, g.ceilMode) == (3, 2, 1, 1)


def test_a_pickle_written_now_round_trips_and_loads_under_the_old_path(pkg):
    mods = _modules(pkg)
    data = pickle.dumps(mods, protocol=2)
    assert b'cbinfer_amd.pool\n' in data and b'cbinfer_amd.conv2d' not in data
    buf = io.BytesIO()
    torch.save(mods, buf)
    buf.seek(0)
    renamed = data.replace(b'cbinfer_amd.pool\n', b'cbinfer_amd.conv2d\n')      # (protocol 2: GLOBAL ends at a newline)
    assert renamed != data
    for back in (pickle.loads(data), torch.load(buf, weights_only=False), copy.deepcopy(mods), pickle.loads(renamed),
                 pickle.loads(pickle.dumps(mods))):
        for got, want in zip(back, mods):
            _assert_same(got, want)


def test_a_workspace_that_cannot_be_made_leaves_the_old_one(pkg):
    """chain.CBStateModule._cached_work: a make() that raises -- here _adaptive_out on a map smaller than output_size --
    does not touch the work buffers of the last frame."""
    from cbinfer_amd._lib import CBinferError
    m = pkg.CBPoolAvg2d(nn.AdaptiveAvgPool2d((7, None)))
    x = torch.zeros(1, 2, 9, 65)
    work = m._frame(x, torch.zeros(0, dtype=torch.int32))[3]
    assert m.__dict__['_poolWork'] is work and work['key'] == (9, 65, x.device) and work['size'] == (7, 65)
    assert work['inBits'].numel() * 64 >= 9 * 65
    assert m._frame(x, torch.zeros(0, dtype=torch.int32))[3] is work      # the same key: the same buffers
    with pytest.raises(CBinferError, match=r"output_size=\(7, 5\) is larger than the 6x5 map"):
        m._frame(torch.zeros(1, 2, 6, 5), torch.zeros(0, dtype=torch.int32))
    assert m.__dict__['_poolWork'] is work
    g = pkg.CBPoolMax2d(nn.MaxPool2d(3, 2), generalGeometry=True)
    work = g.__dict__['_poolWork'] = dict(key=None)      # (a frame's worth, set by hand)
    with pytest.raises(CBinferError, match="a 2x2 map is smaller than the window"):
        g._frame(torch.zeros(1, 2, 2, 2), torch.zeros(0, dtype=torch.int32))
    assert g.__dict__['_poolWork'] is work
    assert g._frame(torch.zeros(1, 2, 9, 8), torch.zeros(0, dtype=torch.int32))[3]['size'] == (4, 3)
    pkg.clearMemory(nn.Sequential(m, g))
    assert m.__dict__['_poolWork'] is None and g.__dict__['_poolWork'] is None
