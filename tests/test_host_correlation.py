"""Host tests of the correlation layer (CBBinary2d('correlate'), cb_corr.hip).  No device is needed."""
import ctypes

import pytest
import torch

import correlation_cases as cc
from optest import lib, pkg      # noqa: F401  (fixtures)


@pytest.mark.parametrize("kw,words", [
    (dict(other=2.0), "other= does not go with op='correlate'"), (dict(gate='sigmoid'), "gate= does not go"),
    (dict(reverse=True), "reverse= does not go"), (dict(displacement=65), "within -64 .. 64"),
    (dict(displacement=((0, 0), (3, 1))), "ascending"), (dict(displacement=(1, 2, 3)), "displacement="),
    (dict(displacement=2.5), "displacement="), (dict(step=9), "step=9 must be an int in 1 .. 8"),
    (dict(step=0), "step=0"), (dict(displacement=5, step=3), "step=3 must divide both range lengths"),
    (dict(displacement=20), "1681 output channels, the limit is 512")] + [
    (dict(op='mul', **{key: 1}), "%s= goes with op='correlate' only, not with op='mul'" % key)
    for key in ("displacement", "step", "normalize")])
def test_constructor_refusals(pkg, lib, kw, words):
    with pytest.raises(lib.CBinferError, match=words):
        pkg.CBBinary2d(**dict(dict(op='correlate'), **kw))


def test_forward_refusals(pkg, lib):
    m, x = pkg.CBBinary2d('correlate'), torch.zeros(1, 4, 5, 6)
    for b, words in ((None, "takes two operands"), (torch.zeros(1, 4, 5, 7), r"the operands differ: a is \(1, 4, 5, 6\)"),
                     (x.half(), "the operands differ"), (torch.zeros(1, 1, 5, 6), "the operands differ"),
                     (('changeIndexes', x), "not \\('changeIndexes', tensor, indexes\\)"), (x, "HIP devices only")):
        with pytest.raises(lib.CBinferError, match=words):
            m(x, b)
    with pytest.raises(lib.CBinferError, match=r"operand a must be a \[1, C, H, W\] tensor"):
        m(torch.zeros(2, 4, 5, 6), torch.zeros(2, 4, 5, 6))


@pytest.mark.parametrize("displacement,step,window", cc.WINDOWS, ids=cc.WINDOW_IDS)
def test_displacement_forms_and_frame_sets(pkg, displacement, step, window):
    """The three forms resolve to (y0, y1, x0, x1, Dy, Dx); the frames of the GPU test list less than half the map."""
    m = pkg.CBBinary2d('correlate', displacement=displacement, step=step, normalize=False)
    assert m.window == window and len(cc.taps(window, step)) == window[4] * window[5]
    assert len(cc.frames(window, step)) == 6
    assert 'correlate' in repr(m) and list(m.state_dict()) == ['outputState'] and not m.normalize
    assert pkg.CBBinary2d('correlate').window == (-4, 4, -4, 4, 9, 9) and pkg.CBBinary2d('correlate').normalize


def test_existing_ops_keep_repr_and_state_dict(pkg):
    assert repr(pkg.CBBinary2d('mul', gate='sigmoid')) == \
        'CBBinary2d (op=mul, gate=sigmoid, reverse=False, other=None, propChgIdxs=False)'
    assert repr(pkg.CBBinary2d('sub', other=torch.zeros(3), reverse=True)) == \
        'CBBinary2d (op=sub, gate=None, reverse=True, other=(3,), propChgIdxs=False)'
    assert list(pkg.CBBinary2d('add', other=torch.zeros(3)).state_dict()) == ['other', 'outputState']
    assert list(pkg.CBBinary2d('add').state_dict()) == ['outputState']


def corr_struct(lib, y0=-4, y1=4, x0=-4, x1=4, step=1, normalize=1):
    return ctypes.pointer(lib.Corr(y0, y1, x0, x1, step, normalize))


def test_correlation_supported_over_its_limits(lib):
    sup = lib.C.cbinfer_correlation_supported
    for good in (corr_struct(lib), corr_struct(lib, 0, 0, -64, 64), corr_struct(lib, -64, 64, 0, 0, 8, 0),
                 corr_struct(lib, -20, 20, -20, 20, 2), corr_struct(lib, -15, 16, -7, 8)):      # (32 x 16 = 512)
        assert sup(good, 67, 7, 70) == 1
    assert sup(None, 4, 5, 6) == 0 and lib.C.cbinfer_binary_supported(5, 0, 0) == 0 and lib.ABI_VERSION == 11
    for bad in (corr_struct(lib, -65), corr_struct(lib, y1=65), corr_struct(lib, x0=-65), corr_struct(lib, x1=65),
                corr_struct(lib, 1, 0), corr_struct(lib, x0=2, x1=1), corr_struct(lib, step=0), corr_struct(lib, step=9),
                corr_struct(lib, -5, 5, -5, 5, 3), corr_struct(lib, -4, 4, -3, 4, 2), corr_struct(lib, normalize=2),
                corr_struct(lib, -16, 16, -7, 8), corr_struct(lib, -20, 20, -20, 20)):      # (33 x 16, 41 x 41)
        assert sup(bad, 4, 5, 6) == 0
    for Cn, H, W in ((0, 5, 6), (4, 0, 6), (4, 5, 0), (1 << 25, 5, 6), (4, 1 << 16, 1 << 15)):
        assert sup(corr_struct(lib), Cn, H, W) == 0


def test_entry_point_checks_its_arguments(lib):
    """Bad arguments return CB_ERR_BADARG (-1) before anything is launched (the device pointers are never followed)."""
    A, B, O, BB, BITS, COPY, M, L, N2 = (0x10000 * i for i in range(1, 10))
    assert {'cbinfer_correlation_supported', 'cbinfer_cbcorrelation_forward'} <= set(lib.EXPORTED_SYMBOLS)

    def go(a=A, b=B, o=O, am=None, al=None, ac=0, an=None, bm=None, bl=None, bc=0, bn=None, bb=BB, bits=BITS, cp=COPY,
           Cn=3, H=4, W=5, co=corr_struct(lib), dt=lib.CB_F32):
        return lib.C.cbinfer_cbcorrelation_forward(a, b, o, am, al, ac, an, bm, bl, bc, bn, bb, bits, cp, Cn, H, W, co, dt,
                                                   None)

    for bad in (dict(a=None), dict(b=None), dict(o=None), dict(o=A), dict(o=B), dict(bb=None), dict(bits=None),
                dict(cp=None), dict(cp=BITS), dict(bb=BITS), dict(bb=COPY), dict(co=None), dict(Cn=0), dict(H=0), dict(W=0),
                dict(dt=7), dict(Cn=1 << 25), dict(al=L, ac=-1), dict(bl=L, bc=-1), dict(am=M, al=L), dict(bm=M, bl=L),
                dict(an=N2), dict(bn=N2), dict(am=BB), dict(am=BITS), dict(am=COPY), dict(bm=BB), dict(bm=BITS),
                dict(bm=COPY), dict(co=corr_struct(lib, step=9)), dict(co=corr_struct(lib, -20, 20, -20, 20))):
        assert go(**bad) == -1, bad


@pytest.mark.parametrize("displacement,step,window", cc.LIMIT_WINDOWS, ids=cc.LIMIT_WINDOW_IDS)
def test_limit_windows_resolve_to_their_tile_counts(pkg, lib, displacement, step, window):
    """correlation_cases.LIMIT_WINDOWS: what correlation_window() makes of them, the column tile counts NT = 1, 3, 5, 9 --
    the last two in the NTMAX = 9 kernels --, and frames that list under half of 5x150 and, for NT >= 5, of 7x70."""
    assert pkg.CBBinary2d('correlate', displacement=displacement, step=step).window == window
    assert pkg.CBBinary2d('aggregate', displacement=displacement, step=step).window == window
    NT = cc.column_tiles(window)
    assert NT == dict(zip(cc.LIMIT_WINDOW_IDS, (1, 3, 5, 9)))[cc.LIMIT_WINDOW_IDS[cc.LIMIT_WINDOWS.index((displacement, step,
                                                                                                         window))]]
    assert lib.C.cbinfer_correlation_supported(corr_struct(lib, *window[:4], step), 67, *cc.LIMIT_MAP) == 1
    assert len(cc.frames(window, step, *cc.LIMIT_MAP)) == 6 and (NT < 5 or len(cc.frames(window, step, *cc.MAPS[0])) == 6)
    assert [cc.column_tiles(w) for _, _, w in cc.WINDOWS] == [2, 2, 4, 2]


def test_strided_changes_list_under_half_in_both_laps():
    """The change-based frame of the grid-stride tests on a map of cap + 5 rows: rows of both laps, under half listed."""
    cap, (_, step, window) = 2048, cc.STRIDE_WINDOW
    SA, SB = cc.strided_changes(cap + 5, 16, cap)
    listed = cc.footprint(SA, SB, window, step)
    assert SA[:cap].any() and SA[cap:].any() and SB[:cap].any() and SB[cap:].any()
    assert listed[:cap].any() and listed[cap:].any() and listed.mean() < 0.5 and cc.column_tiles(window) == 2
