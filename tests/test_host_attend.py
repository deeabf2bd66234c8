"""Host tests of the fused local attention (CBBinary2d('attend'), cb_attend.hip).  No device is needed."""
import ctypes

import pytest
import torch

from optest import lib, pkg      # noqa: F401  (fixtures)


@pytest.mark.parametrize("kw,words", [
    (dict(other=2.0), "other= does not go with op='attend'"), (dict(gate='sigmoid'), "gate= does not go"),
    (dict(reverse=True), "reverse= does not go"), (dict(normalize=True), "normalize= does not go with op='attend'"),
    (dict(groups=2), "groups= does not go with op='attend'"), (dict(stride=2), "stride= goes with op='deform' only"),
    (dict(weight=torch.zeros(1, 1, 1, 1)), "weight= goes with op='deform' only, not with op='attend'"),
    (dict(displacement=65), "within -64 .. 64"), (dict(displacement=20), "1681 taps, the limit is 512"),
    (dict(displacement=((0, 0), (-49, 0))), "column range x1 - x0 of 48 at most, got 49"),
    (dict(heads=65), "heads=65 must be an int in 1 .. 64"), (dict(scale=float('inf')), "scale=inf must be a finite"),
    (dict(border='reflect'), "border='reflect' is not supported, only 'mask' or 'zero'"),
    (dict(heads=2, positionBias=torch.zeros(2, 80)), r"positionBias must be .* \(2, 81\) or \(2, 9, 9\), got \(2, 80\)"),
    (dict(op='mul', heads=2), "heads= is a setting of op='attend', op='mul' does not take it"),
    (dict(op='correlate', scale=0.5, border='zero'), "scale= is a setting of op='attend', op='correlate'"),
    (dict(op='deform', positionBias=torch.zeros(1, 81)), "positionBias= is a setting of op='attend', op='deform'")])
def test_constructor_refusals(pkg, lib, kw, words):
    with pytest.raises(lib.CBinferError, match=words):
        pkg.CBBinary2d(**dict(dict(op='attend'), **kw))


def test_forward_refusals(pkg, lib):
    m, q, kv = pkg.CBBinary2d('attend', displacement=1, heads=2), torch.zeros(1, 4, 5, 6), torch.zeros(1, 10, 5, 6)
    for a, b, words in ((q, None, "takes two operands"), (q, torch.zeros(1, 10, 5, 7), r"the operands differ: q is \(1, 4"),
                        (q, kv.half(), "the operands differ"), (q, q.clone(), "operand kv has 4 channels: behind the 4 "
                         "channels of k .* no channel of v"), (q, torch.zeros(1, 9, 5, 6), "heads=2 does not divide the 4 "
                         "channels of q and k and the 5 channels of v"), (torch.zeros(1, 5, 5, 6), kv, "heads=2 does not"),
                        (torch.zeros(1, 258, 5, 6), torch.zeros(1, 260, 5, 6), "a head takes 128 channels at most"),
                        (q, ('changeIndexes', kv), "not \\('changeIndexes', tensor, indexes\\)"), (q, kv, "HIP devices only")):
        with pytest.raises(lib.CBinferError, match=words):
            m(a, b)


def test_settings_repr_and_state_dict(pkg):
    m = pkg.CBBinary2d('attend')
    assert (m.window, m.heads, m.scale, m.border, list(m.state_dict())) == ((-4, 4, -4, 4, 9, 9), 1, None, 'mask', ['outputState'])
    bias = torch.arange(30.0).reshape(2, 3, 5)
    m = pkg.CBBinary2d('attend', displacement=(1, 2), heads=2, scale=0.25, border='zero', positionBias=bias.double())
    assert repr(m) == ("CBBinary2d (op=attend, displacement=(1, 2), step=1, heads=2, scale=0.25, border=zero, "
                       "positionBias=True, propChgIdxs=False)")
    bias.zero_()      # (copied, and float32 whatever it was, also under .half())
    assert m.half().positionBias.dtype == torch.float32 and m.positionBias.shape == (2, 15)
    assert float(m.positionBias[1, 14]) == 29.0 and list(m.state_dict()) == ['positionBias', 'outputState']
    assert repr(pkg.CBBinary2d('mul', gate='sigmoid')) == \
        'CBBinary2d (op=mul, gate=sigmoid, reverse=False, other=None, propChgIdxs=False)'
    assert repr(pkg.CBBinary2d('aggregate')) == \
        'CBBinary2d (op=aggregate, displacement=4, step=1, groups=1, propChgIdxs=False)'
    assert list(pkg.CBBinary2d('add', other=torch.zeros(3)).half().state_dict()) == ['other', 'outputState']
    assert list(pkg.CBBinary2d('correlate').state_dict()) == ['outputState']


def att(lib, y0=-4, y1=4, x0=-4, x1=4, step=1, heads=1, border=0, hasBias=0, scale=0.5):
    return ctypes.pointer(lib.Attend(y0, y1, x0, x1, step, heads, border, hasBias, scale))


def test_attend_supported_over_its_limits(lib):
    sup = lib.C.cbinfer_attend_supported
    for good, Cn, Cv in ((att(lib), 67, 40), (att(lib, 0, 0, -48, 0), 128, 128), (att(lib, -64, 64, 0, 0, 8), 5, 5),
                         (att(lib, heads=64, border=1, hasBias=1), 64 * 128, 64), (att(lib, -10, 10, -24, 24, 2, 6), 6, 6)):
        assert sup(good, Cn, Cv, 7, 70) == 1
    assert sup(None, 4, 4, 5, 6) == 0 and lib.ABI_VERSION == 11
    for bad in (att(lib, -65), att(lib, x1=65), att(lib, 1, 0), att(lib, step=0), att(lib, step=9), att(lib, -5, 5, -5, 5, 3),
                att(lib, -20, 20, -20, 20), att(lib, 0, 0, -49, 0), att(lib, heads=0), att(lib, heads=65), att(lib, heads=5),
                att(lib, border=2), att(lib, border=-1), att(lib, hasBias=2), att(lib, scale=float('nan')),
                att(lib, scale=float('inf'))):
        assert sup(bad, 64, 64, 5, 6) == 0
    for Cn, Cv, H, W in ((129, 4, 5, 6), (4, 129, 5, 6), (0, 4, 5, 6), (4, 0, 5, 6), (4, 4, 0, 6), (4, 4, 5, 0),
                         (4, 4, 1 << 16, 1 << 15)):
        assert sup(att(lib), Cn, Cv, H, W) == 0


def test_entry_point_checks_its_arguments(lib):
    """Bad arguments return CB_ERR_BADARG (-1) before anything is launched."""
    Q, KV, O, KB, BITS, COPY, M, L, N2, PB = (0x10000 * i for i in range(1, 11))
    assert {'cbinfer_attend_supported', 'cbinfer_cbattend_forward'} <= set(lib.EXPORTED_SYMBOLS)
    assert lib.C.cbinfer_abi_version() == lib.ABI_VERSION == 11 and (lib.ATTEND_MASK, lib.ATTEND_ZERO) == (0, 1)

    def go(q=Q, kv=KV, pb=None, o=O, qm=None, ql=None, qc=0, qn=None, km=None, kl=None, kc=0, kn=None, kb=KB, bits=BITS,
           cp=COPY, Cn=4, Cv=4, H=4, W=5, at=att(lib), dt=lib.CB_F32):
        return lib.C.cbinfer_cbattend_forward(q, kv, pb, o, qm, ql, qc, qn, km, kl, kc, kn, kb, bits, cp, Cn, Cv, H, W, at,
                                              dt, None)

    for bad in (dict(q=None), dict(kv=None), dict(o=None), dict(o=Q), dict(o=KV), dict(kv=Q), dict(kb=None),
                dict(bits=None), dict(cp=None), dict(cp=BITS), dict(kb=BITS), dict(kb=COPY), dict(at=None), dict(Cn=0),
                dict(Cv=0), dict(H=0), dict(W=0), dict(dt=7), dict(Cn=129), dict(Cv=129), dict(ql=L, qc=-1),
                dict(kl=L, kc=-1), dict(qm=M, ql=L), dict(km=M, kl=L), dict(qn=N2), dict(kn=N2), dict(qm=KB), dict(qm=BITS),
                dict(qm=COPY), dict(km=KB), dict(km=BITS), dict(km=COPY), dict(pb=PB), dict(at=att(lib, hasBias=1)),
                dict(at=att(lib, step=9)), dict(at=att(lib, 0, 0, -49, 0)), dict(at=att(lib, heads=3)),
                dict(at=att(lib, border=2)), dict(at=att(lib, scale=float('nan')))):
        assert go(**bad) == -1, bad


def test_limit_cases_are_what_they_claim(pkg):
    """attend_cases.LIMIT_WINDOWS resolve to two and three column tiles; LIMIT_SHAPES reach the second block of v and the
    second chunk of k; PEAKED has R >= 100 somewhere on the float64 reference while the float32 bound stays below 2^-10 A,
    in both dtypes and under both borders; scale = 0 makes the reference the mean of the values that take part."""
    import numpy as np

    import attend_cases as ac
    from correlation_cases import column_tiles
    for (displacement, step, window), NT in zip(ac.LIMIT_WINDOWS, (2, 3)):
        assert pkg.CBBinary2d('attend', displacement=displacement, step=step).window == window
        assert column_tiles(window) == NT
    assert [(Cn // h > 64, Cv // h > 64) for Cn, Cv, h in ac.LIMIT_SHAPES] == [(False, True), (True, True), (True, True)]
    (Cn, Cv, heads), scale = ac.PEAKED
    window = ac.WINDOWS[0][2]
    for npdt in (np.float32, np.float16):
        q, kv, bias = ac.operands(np.random.default_rng(17), Cn, Cv, heads, window, (7, 70), npdt)
        for border in ac.BORDERS:
            ref = ac.reference(q, kv, bias, window, 1, heads, border, scale)
            assert bias is None and ref['R'].max() >= 100
            assert np.array_equal(ac.reference(q, kv, bias, window, 1, heads, border, -scale)['Q'], ref['Q'])
            assert ((ac.bound(ref, window, False) < 2.0 ** -10 * ref['A']) | (ref['A'] == 0)).all()
            flat = ac.reference(q, kv, None, window, 1, heads, border, 0.0)['out']
            mean = ac.uniform_mean(kv, Cn, window, 1, border)
            assert np.abs(flat - mean).max() <= 1e-12 * np.abs(mean).max()
    table = ac.operands(np.random.default_rng(17), 5, 5, 1, window, (3, 16), np.float32, bias='planes')[2]
    assert table.shape == (1, 9, 9) and ac.operands(np.random.default_rng(17), 5, 5, 1, window, (3, 16), np.float32)[2] is None
