"""Host tests of the deformable convolution (CBBinary2d('deform'), cb_deform.hip); no device needed."""
import ctypes

import pytest
import torch

from optest import lib, pkg      # noqa: F401  (fixtures)

W8 = torch.zeros(6, 8, 3, 3)


@pytest.mark.parametrize("kw,words", [
    (dict(other=2.0), "other= does not go with op='deform'"), (dict(gate='sigmoid'), "gate= does not go"),
    (dict(reverse=True), "reverse= does not go"), (dict(displacement=2), "displacement= does not go"),
    (dict(groups=2), "groups=2: op='deform' takes one weight group only"), (dict(weight=None), "takes weight="),
    (dict(weight=torch.zeros(6, 8, 3)), "takes weight="), (dict(weight=W8.double()), "float32 or float16"),
    (dict(bias=torch.zeros(5)), r"bias must be a \[6\] tensor"), (dict(modulation='softmax'), "modulation='softmax'"),
    (dict(offsetGroups=3), "offsetGroups=3 does not divide the 8"), (dict(offsetGroups=17), "offsetGroups=17 must be"),
    (dict(stride=(1, 2, 3)), "stride="), (dict(stride=5), "beyond what the library takes"),
    (dict(op='mul', weight=W8), "weight= goes with op='deform' only, not with op='mul'"),
    (dict(op='correlate', weight=None, offsetGroups=2), "offsetGroups= goes with op='deform' only"),
    (dict(op='aggregate', weight=None, modulation='planes'), "modulation= goes with op='deform' only"),
    (dict(op='add', weight=None, relu=True), "relu= goes with op='deform' only")])
def test_constructor_refusals(pkg, lib, kw, words):
    with pytest.raises(lib.CBinferError, match=words):
        pkg.CBBinary2d(**dict(dict(op='deform', weight=W8), **kw))


def test_forward_refusals(pkg, lib):
    m = pkg.CBBinary2d('deform', weight=W8, padding=1, offsetGroups=2, modulation='planes')
    x, f = torch.zeros(1, 8, 5, 6), torch.zeros(1, 54, 5, 6)
    for a, b, words in ((x, None, "takes two operands"), (torch.zeros(1, 4, 5, 6), f, "operand x has 4 channels"),
                        (x, torch.zeros(1, 36, 5, 6), "the field has 36 channels, offsetGroups=2 x 3 x 3 taps with "
                         "modulation='planes' take 54"), (x, torch.zeros(1, 54, 5, 7), "the field is a 5x7 map, the output "
                         "map of a 5x6 input is 5x6"), (x.half(), f, "operand x is torch.float16 on cpu, the weight "
                         "torch.float32"), (x, ('changeIndexes', f), "not \\('changeIndexes', tensor, indexes\\)"),
                        (x, f.half(), "HIP devices only")):      # (a float16 field under a float32 x is taken)
        with pytest.raises(lib.CBinferError, match=words):
            m(a, b)


def test_buffers_repr_and_containers(pkg, lib):
    src = torch.arange(6 * 8 * 9, dtype=torch.float32).reshape(6, 8, 3, 3)
    m = pkg.CBBinary2d('deform', weight=src, bias=torch.ones(6), stride=2, padding=(1, 2), modulation='sigmoid', relu=True)
    src.zero_()      # (copied at construction)
    assert list(m.state_dict()) == ['weight', 'bias', 'outputState'] and m.weight[5, 7, 2, 2] == 431
    twin = pkg.CBBinary2d('deform', weight=W8, bias=torch.zeros(6))
    twin.load_state_dict(m.state_dict())
    assert torch.equal(twin.weight, m.weight) and torch.equal(twin.bias, m.bias)
    assert m.half().weight.dtype == m.bias.dtype == torch.float16
    assert repr(m) == ('CBBinary2d (op=deform, 8 -> 6, kernel=3x3, stride=(2, 2), padding=(1, 2), dilation=(1, 1), '
                       'offsetGroups=1, modulation=sigmoid, bias=True, relu=True, propChgIdxs=False)')
    assert "'deform'" in str(pytest.raises(lib.CBinferError, pkg.CBBinary2d, 'pow').value)
    # the containers that refuse the module name the op through its repr
    with pytest.raises(lib.CBinferError, match="op=deform"):
        pkg.SequenceBatch(torch.nn.Sequential(m), 2)


def deform(lib, k=(3, 3), s=(1, 1), p=(1, 1), d=(1, 1), Go=1, mod=0, fdt=0, relu=0):
    return ctypes.pointer(lib.Deform(lib.Geom(*(k + s + p + d)), Go, mod, lib.CB_F32 if fdt == 0 else fdt, relu))


def test_deform_supported_at_its_limits(lib):
    sup = lib.C.cbinfer_deform_supported
    for good, dims in ((deform(lib), (8, 9, 70, 8)), (deform(lib, (7, 7), (4, 4), (64, 64), (8, 8)), (8, 9, 70, 8)),
                       (deform(lib, Go=16, mod=2, fdt=lib.CB_F16, relu=1), (16, 9, 70, 8)),
                       (deform(lib, (1, 1), p=(0, 0)), (8, 32767, 1, 1)), (deform(lib), (255, 1024, 1024, 2047))):
        assert sup(good, *dims) == 1
    assert sup(None, 8, 9, 70, 8) == 0 and lib.ABI_VERSION == 11
    for bad in (deform(lib, (8, 3)), deform(lib, s=(5, 1)), deform(lib, d=(1, 9)), deform(lib, p=(65, 1)), deform(lib, Go=0),
                deform(lib, Go=17), deform(lib, Go=3), deform(lib, mod=3), deform(lib, mod=-1), deform(lib, fdt=7),
                deform(lib, relu=2), deform(lib, (7, 7), p=(0, 0))):
        assert sup(bad, 16, 5, 70, 8) == 0      # (the last: the filter does not fit the unpadded 5-row map)
    for dims in ((0, 9, 70, 8), (8, 0, 70, 8), (8, 9, 0, 8), (8, 9, 70, 0), (8, 32768, 1, 1), (256, 1024, 1024, 8),
                 (8, 1024, 1024, 2048), (8, 9, 70, 1 << 20)):
        assert sup(deform(lib), *dims) == 0
    nbytes = lib.C.cbinfer_deform_prepared_weights_bytes
    assert nbytes(70, 40, deform(lib), lib.CB_F32) == 128 * 9 * 64 * 4 and nbytes(8, 8, deform(lib), lib.CB_F16) == 64 * 288 * 2


def test_entry_point_checks_its_arguments(lib):
    """Bad arguments return CB_ERR_BADARG (-1) before anything is launched (the device pointers are never followed)."""
    X, F, WP, O, IB, BITS, COPY, WS, M, L, N2 = (0x10000 * i for i in range(1, 12))

    def go(x=X, f=F, wp=WP, b=None, o=O, xm=None, xl=None, xc=0, xn=None, fm=None, fl=None, fc=0, fn=None, ib=IB, bits=BITS,
           cp=COPY, ws=WS, Cn=8, H=9, W=70, K=8, d=deform(lib), dt=lib.CB_F32):
        return lib.C.cbinfer_cbdeform_forward(x, f, wp, b, o, xm, xl, xc, xn, fm, fl, fc, fn, ib, bits, cp, ws, Cn, H, W, K,
                                              d, dt, None)

    for bad in (dict(x=None), dict(f=None), dict(wp=None), dict(o=None), dict(ws=None), dict(o=X), dict(o=F), dict(ib=None),
                dict(bits=None), dict(cp=None), dict(cp=BITS), dict(ib=BITS), dict(ib=COPY), dict(d=None), dict(Cn=0),
                dict(H=0), dict(W=0), dict(K=0), dict(dt=7), dict(xl=L, xc=-1), dict(fl=L, fc=-1), dict(xm=M, xl=L),
                dict(fm=M, fl=L), dict(xn=N2), dict(fn=N2), dict(xm=IB), dict(xm=BITS), dict(xm=COPY), dict(fm=IB),
                dict(fm=BITS), dict(fm=COPY), dict(d=deform(lib, Go=3)), dict(d=deform(lib, mod=3)),
                dict(d=deform(lib, s=(5, 5)))):
        assert go(**bad) == -1, bad
    assert lib.C.cbinfer_deform_prep_weights(X, WP, 8, 8, deform(lib, s=(5, 5)), lib.CB_F32, None) == -1
