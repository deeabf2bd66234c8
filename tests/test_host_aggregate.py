"""Host tests of the per-pixel kernel application (CBBinary2d('aggregate'), cb_aggr.hip).  No device is
needed."""
import ctypes

import pytest
import torch

import aggregate_cases as ac
from optest import lib, pkg      # noqa: F401  (fixtures)


@pytest.mark.parametrize("kw,words", [
    (dict(other=2.0), "other= does not go with op='aggregate'"), (dict(gate='sigmoid'), "gate= does not go"),
    (dict(reverse=True), "reverse= does not go"), (dict(normalize=True), "normalize= does not go with op='aggregate'"),
    (dict(displacement=65), "within -64 .. 64"), (dict(displacement=2.5), "displacement="),
    (dict(displacement=5, step=3), "step=3 must divide both range lengths"),
    (dict(displacement=20), "1681 taps, the limit is 512"), (dict(groups=0), "groups=0 must be an int >= 1"),
    (dict(groups=51), "groups x 81 taps within 4096"), (dict(groups=2.0), "groups=2.0"),
    (dict(op='mul', groups=2), "groups= goes with op='aggregate' only, not with op='mul'"),
    (dict(op='correlate', groups=2), "groups= does not go with op='correlate'")])
def test_constructor_refusals(pkg, lib, kw, words):
    with pytest.raises(lib.CBinferError, match=words):
        pkg.CBBinary2d(**dict(dict(op='aggregate'), **kw))


def test_forward_refusals(pkg, lib):
    m, w, v = pkg.CBBinary2d('aggregate', displacement=1, groups=2), torch.zeros(1, 18, 5, 6), torch.zeros(1, 4, 5, 6)
    for a, b, words in ((w, None, "takes two operands"), (w, torch.zeros(1, 4, 5, 7), r"the operands differ: w is \(1, 18"),
                        (w, v.half(), "the operands differ"), (torch.zeros(1, 9, 5, 6), v, "operand w has 9 channels, "
                         "groups=2 x 3 x 3 taps take 18"), (w, torch.zeros(1, 5, 5, 6), "groups=2 does not divide the 5"),
                        (w, ('changeIndexes', v), "not \\('changeIndexes', tensor, indexes\\)"), (w, v, "HIP devices only")):
        with pytest.raises(lib.CBinferError, match=words):
            m(a, b)


@pytest.mark.parametrize("displacement,step,window", ac.WINDOWS, ids=ac.WINDOW_IDS)
def test_displacement_forms(pkg, displacement, step, window):
    m = pkg.CBBinary2d('aggregate', displacement=displacement, step=step, groups=5)
    assert m.window == window and m.groups == 5 and list(m.state_dict()) == ['outputState']
    assert repr(m) == 'CBBinary2d (op=aggregate, displacement=%r, step=%d, groups=5, propChgIdxs=False)' % (displacement, step)
    assert pkg.CBBinary2d('aggregate').window == (-4, 4, -4, 4, 9, 9) and pkg.CBBinary2d('aggregate').groups == 1


def test_existing_ops_keep_repr_and_state_dict(pkg):
    assert repr(pkg.CBBinary2d('mul', gate='sigmoid')) == \
        'CBBinary2d (op=mul, gate=sigmoid, reverse=False, other=None, propChgIdxs=False)'
    assert repr(pkg.CBBinary2d('correlate')) == \
        'CBBinary2d (op=correlate, displacement=4, step=1, normalize=True, propChgIdxs=False)'
    assert list(pkg.CBBinary2d('add', other=torch.zeros(3)).state_dict()) == ['other', 'outputState']
    assert list(pkg.CBBinary2d('correlate').state_dict()) == ['outputState']


def aggr_struct(lib, y0=-4, y1=4, x0=-4, x1=4, step=1, groups=1):
    return ctypes.pointer(lib.Aggr(y0, y1, x0, x1, step, groups))


def test_aggregate_supported_over_its_limits(lib):
    sup = lib.C.cbinfer_aggregate_supported
    for good, Cn in ((aggr_struct(lib), 67), (aggr_struct(lib, 0, 0, -64, 64), 67), (aggr_struct(lib, -64, 64, 0, 0, 8), 67),
                     (aggr_struct(lib, -15, 16, -7, 8, groups=8), 64), (aggr_struct(lib, groups=50), 100),
                     (aggr_struct(lib, -3, 3, -3, 3, groups=16), 256), (aggr_struct(lib, groups=5), 5)):
        assert sup(good, Cn, 7, 70) == 1      # (the fourth: 32 x 16 = 512 taps x 8 groups = 4096 planes)
    assert sup(None, 4, 5, 6) == 0 and lib.ABI_VERSION == 11
    for bad in (aggr_struct(lib, -65), aggr_struct(lib, y1=65), aggr_struct(lib, x0=-65), aggr_struct(lib, x1=65),
                aggr_struct(lib, 1, 0), aggr_struct(lib, x0=2, x1=1), aggr_struct(lib, step=0), aggr_struct(lib, step=9),
                aggr_struct(lib, -5, 5, -5, 5, 3), aggr_struct(lib, -16, 16, -7, 8), aggr_struct(lib, -20, 20, -20, 20),
                aggr_struct(lib, groups=0), aggr_struct(lib, groups=-1), aggr_struct(lib, groups=5),
                aggr_struct(lib, groups=51), aggr_struct(lib, -15, 16, -7, 8, groups=9)):
        assert sup(bad, 459, 5, 6) == 0      # (459 = 9 x 51: only 5 of the group counts does not divide it)
    for Cn, H, W in ((0, 5, 6), (4, 0, 6), (4, 5, 0), (1 << 25, 5, 6), (4, 1 << 16, 1 << 15)):
        assert sup(aggr_struct(lib), Cn, H, W) == 0


def test_entry_point_checks_its_arguments(lib):
    """Bad arguments return CB_ERR_BADARG (-1) before anything is launched (the device pointers are never followed)."""
    A, B, O, BB, BITS, COPY, M, L, N2 = (0x10000 * i for i in range(1, 10))
    assert {'cbinfer_aggregate_supported', 'cbinfer_cbaggregate_forward'} <= set(lib.EXPORTED_SYMBOLS)
    assert lib.C.cbinfer_abi_version() == lib.ABI_VERSION == 11

    def go(w=A, v=B, o=O, wm=None, wl=None, wc=0, wn=None, vm=None, vl=None, vc=0, vn=None, vb=BB, bits=BITS, cp=COPY,
           Cn=4, H=4, W=5, ag=aggr_struct(lib), dt=lib.CB_F32):
        return lib.C.cbinfer_cbaggregate_forward(w, v, o, wm, wl, wc, wn, vm, vl, vc, vn, vb, bits, cp, Cn, H, W, ag, dt,
                                                 None)

    for bad in (dict(w=None), dict(v=None), dict(o=None), dict(o=A), dict(o=B), dict(vb=None), dict(bits=None),
                dict(cp=None), dict(cp=BITS), dict(vb=BITS), dict(vb=COPY), dict(ag=None), dict(Cn=0), dict(H=0), dict(W=0),
                dict(dt=7), dict(Cn=1 << 25), dict(wl=L, wc=-1), dict(vl=L, vc=-1), dict(wm=M, wl=L), dict(vm=M, vl=L),
                dict(wn=N2), dict(vn=N2), dict(wm=BB), dict(wm=BITS), dict(wm=COPY), dict(vm=BB), dict(vm=BITS),
                dict(vm=COPY), dict(ag=aggr_struct(lib, step=9)), dict(ag=aggr_struct(lib, -20, 20, -20, 20)),
                dict(ag=aggr_struct(lib, groups=3)), dict(ag=aggr_struct(lib, groups=64))):
        assert go(**bad) == -1, bad
