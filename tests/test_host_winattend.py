"""Host tests of the partitioned window attention (CBBinary2d('attend', partition=), cb_winattend.hip).
No device is needed."""
import ctypes

import pytest
import torch

from optest import lib, pkg      # noqa: F401  (fixtures)


@pytest.mark.parametrize("kw,words", [
    (dict(displacement=2), "displacement= does not go with partition="), (dict(step=1), "step= does not go with partition="),
    (dict(border='mask'), "border= does not go with partition="), (dict(partition=None, shift=1), "shift= goes with partition= only"),
    (dict(partition=17), "partition=17: a cell is 1 .. 16 pixels a side and 144 tokens at most"),
    (dict(partition=(12, 13)), "144 tokens at most"), (dict(partition=0), "a cell is 1 .. 16"),
    (dict(partition=(7, 7, 7)), "must be an int or a pair of ints"), (dict(partition=7.0), "must be an int or a pair"),
    (dict(shift=7), r"shift=7 must be within 0 .. partition - 1 = \(6, 6\)"), (dict(shift=(0, -1)), "must be within"),
    (dict(heads=65), "heads=65 must be an int in 1 .. 64"), (dict(scale=float('inf')), "scale=inf must be a finite"),
    (dict(other=2.0), "other= does not go with op='attend'"), (dict(groups=2), "groups= does not go with op='attend'"),
    (dict(heads=2, positionBias=torch.zeros(2, 13, 12)), r"positionBias must be .* \(2, 169\) or \(2, 13, 13\), got \(2, 13, 12\)"),
    (dict(op='mul'), "partition= is a setting of op='attend', op='mul' does not take it"),
    (dict(op='correlate', partition=None, shift=1), "shift= is a setting of op='attend', op='correlate'"),
    (dict(op='aggregate'), "partition= is a setting of op='attend', op='aggregate'")])
def test_constructor_refusals(pkg, lib, kw, words):
    with pytest.raises(lib.CBinferError, match=words):
        pkg.CBBinary2d(**dict(dict(op='attend', partition=7), **kw))


def test_forward_refusals(pkg, lib):
    m, q, kv = pkg.CBBinary2d('attend', partition=4, heads=2), torch.zeros(1, 4, 5, 6), torch.zeros(1, 10, 5, 6)
    for a, b, words in ((q, None, "takes two operands"), (q, kv.half(), "the operands differ"),
                        (q, q.clone(), "no channel of v"), (q, torch.zeros(1, 9, 5, 6), "heads=2 does not divide"),
                        (torch.zeros(1, 130, 5, 6), torch.zeros(1, 132, 5, 6), "a head takes 64 channels at most"),
                        (q, kv, "HIP devices only")):
        with pytest.raises(lib.CBinferError, match=words):
            m(a, b)


def test_settings_repr_and_state_dict_of_both_modes(pkg):
    m = pkg.CBBinary2d('attend', partition=(8, 4), shift=(4, 1), heads=2, scale=0.25, positionBias=torch.arange(210.0).reshape(2, 15, 7))
    assert repr(m) == ("CBBinary2d (op=attend, partition=(8, 4), shift=(4, 1), heads=2, scale=0.25, positionBias=True, "
                       "propChgIdxs=False)")
    assert m.half().positionBias.dtype == torch.float32 and m.positionBias.shape == (2, 105)
    assert list(m.state_dict()) == ['positionBias', 'outputState'] and not hasattr(m, 'window')
    m = pkg.CBBinary2d('attend', partition=7)
    assert (m.partition, m.shift, m.heads, m.scale, list(m.state_dict())) == ((7, 7), (0, 0), 1, None, ['outputState'])
    s = pkg.CBBinary2d('attend', displacement=(1, 2), heads=2)      # (the sliding mode is as it was)
    assert repr(s) == ("CBBinary2d (op=attend, displacement=(1, 2), step=1, heads=2, scale=None, border=mask, "
                       "positionBias=False, propChgIdxs=False)")
    assert list(s.state_dict()) == ['outputState'] and not hasattr(s, 'partition') and not hasattr(s, 'shift')
    assert (s.window, s.border) == ((-1, 1, -2, 2, 3, 5), 'mask')


def win(lib, Wy=7, Wx=7, sy=0, sx=0, heads=1, hasBias=0, scale=0.5):
    return ctypes.pointer(lib.WinAttend(Wy, Wx, sy, sx, heads, hasBias, scale))


def test_winattend_supported_over_its_limits(lib):
    sup = lib.C.cbinfer_winattend_supported
    for good, Cn, Cv in ((win(lib), 60, 40), (win(lib, 12, 12, 11, 11), 64, 64), (win(lib, 1, 1), 5, 5),
                         (win(lib, 16, 9, 15, 8, 64, 1), 64 * 64, 64), (win(lib, 9, 16, heads=6), 6, 12)):
        assert sup(good, Cn, Cv, 7, 70) == 1
    assert sup(None, 4, 4, 5, 6) == 0 and lib.ABI_VERSION == 11
    for bad in (win(lib, 0), win(lib, 7, 0), win(lib, 17, 1), win(lib, 1, 17), win(lib, 12, 13), win(lib, sy=7),
                win(lib, sx=7), win(lib, sy=-1), win(lib, sx=-1), win(lib, heads=0), win(lib, heads=65), win(lib, heads=5),
                win(lib, hasBias=2), win(lib, hasBias=-1), win(lib, scale=float('nan')), win(lib, scale=float('inf'))):
        assert sup(bad, 64, 64, 5, 6) == 0
    for Cn, Cv, H, W in ((65, 4, 5, 6), (4, 65, 5, 6), (0, 4, 5, 6), (4, 0, 5, 6), (4, 4, 0, 6), (4, 4, 5, 0),
                         (4, 4, 1 << 16, 1 << 15)):
        assert sup(win(lib), Cn, Cv, H, W) == 0


def test_entry_point_checks_its_arguments(lib):
    """Bad arguments return CB_ERR_BADARG (-1) before anything is launched."""
    Q, KV, O, KB, BITS, COPY, M, L, N2, PB = (0x10000 * i for i in range(1, 11))
    assert {'cbinfer_winattend_supported', 'cbinfer_cbwinattend_forward'} <= set(lib.EXPORTED_SYMBOLS)
    assert lib.C.cbinfer_abi_version() == lib.ABI_VERSION == 11

    def go(q=Q, kv=KV, pb=None, o=O, qm=None, ql=None, qc=0, qn=None, km=None, kl=None, kc=0, kn=None, kb=KB, bits=BITS,
           cp=COPY, Cn=4, Cv=4, H=4, W=5, at=win(lib), dt=lib.CB_F32):
        return lib.C.cbinfer_cbwinattend_forward(q, kv, pb, o, qm, ql, qc, qn, km, kl, kc, kn, kb, bits, cp, Cn, Cv, H, W,
                                                 at, dt, None)

    for bad in (dict(q=None), dict(kv=None), dict(o=None), dict(o=Q), dict(o=KV), dict(kv=Q), dict(kb=None),
                dict(bits=None), dict(cp=None), dict(cp=BITS), dict(kb=BITS), dict(kb=COPY), dict(at=None), dict(Cn=0),
                dict(Cv=0), dict(H=0), dict(W=0), dict(dt=7), dict(Cn=65), dict(Cv=65), dict(ql=L, qc=-1),
                dict(kl=L, kc=-1), dict(qm=M, ql=L), dict(km=M, kl=L), dict(qn=N2), dict(kn=N2), dict(qm=KB), dict(qm=BITS),
                dict(qm=COPY), dict(km=KB), dict(km=BITS), dict(km=COPY), dict(pb=PB), dict(at=win(lib, hasBias=1)),
                dict(at=win(lib, 17, 1)), dict(at=win(lib, sy=7)), dict(at=win(lib, heads=3)),
                dict(at=win(lib, scale=float('nan')))):
        assert go(**bad) == -1, bad


def test_limit_cases_are_what_they_claim(pkg):
    """winattend_cases.LIMIT_PARTITIONS have the token tile counts 1, 1, 2, 3, 5, 7, 8, 9, 9 and shifts the module takes;
    PEAKED has R >= 100 on the float64 reference of every map while the float32 bound stays below 2^-10 A."""
    import numpy as np

    import winattend_cases as wc
    assert [wc.tiles(p) for p in wc.LIMIT_PARTITIONS] == [1, 1, 2, 3, 5, 7, 8, 9, 9]
    assert sorted({wc.tiles(p) for p in wc.PARTITIONS}) == [1, 4, 9]
    for part in wc.LIMIT_PARTITIONS + wc.PARTITIONS:
        for shift in wc.shifts_within(part):
            assert pkg.CBBinary2d('attend', partition=part, shift=shift).shift == shift
        assert part in ((1, 1), (1, 16)) or wc.shifts_within(part) == sorted(wc.shifts(part))
    assert wc.shifts_within((1, 1)) == [(0, 0)] and wc.shifts_within((1, 16)) == [(0, 0), (0, 8), (0, 15)]
    (Cn, Cv, heads), part, scale = wc.PEAKED
    for npdt in (np.float32, np.float16):
        for size in wc.MAPS:
            q, kv, bias = wc.operands(np.random.default_rng(17), Cn, Cv, heads, part, size, npdt)
            ref = wc.reference(q, kv, bias, part, (3, 3), heads, scale)
            assert ref['R'].max() >= 100 and (wc.bound(ref, False) < 2.0 ** -10 * ref['A']).all()
            assert np.array_equal(wc.reference(q, kv, bias, part, (3, 3), heads, -scale)['Q'], ref['Q'])
    flat = wc.operands(np.random.default_rng(17), 5, 5, 1, (2, 3), (5, 70), np.float32, bias='flat')[2]
    assert flat.shape == (1, 15)
