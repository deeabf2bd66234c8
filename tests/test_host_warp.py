"""Host tests of the change-based grid sampling (CBResize2d with a coordinate field, insertCBResize(gridTypes=);
cb_warp.hip).  No device is needed."""
import ctypes
import pickle

import pytest
import torch
import torch.nn.functional as F

from optest import lib, pkg      # noqa: F401  (fixtures)

G = torch.zeros(1, 4, 5, 2)
THETA = torch.tensor([[0.9, 0.2, 0.1], [-0.1, 1.1, 0.0]])


@pytest.mark.parametrize("kw,words", [
    (dict(grid=G, mode='nearest-exact'), "nearest-exact"),
    (dict(grid=G, mode='area'), "mode='area'"),
    (dict(grid=G, padding_mode='wrap'), "padding_mode='wrap'"),
    (dict(grid=G, theta=THETA, size=(4, 5)), "only one of grid and theta"),
    (dict(grid=G, size=(4, 5)), "size="), (dict(theta=THETA), "size="),
    (dict(grid=G, scale_factor=2.0), "scale_factor"), (dict(grid=G, antialias=True), "antialias"),
    (dict(grid=torch.zeros(2, 4, 5, 2)), r"\[1, Ho, Wo, 2\]"), (dict(grid=G.double()), "float32 or float16"),
    (dict(grid=torch.full((1, 4, 5, 2), float('nan'))), "not finite"),
    (dict(grid=torch.zeros(1, 1, 1 << 15, 2)), "limits"),
    (dict(theta=torch.zeros(3, 3), size=(4, 5)), "theta"), (dict(theta=THETA, size=(1 << 15, 5)), "limits")])
def test_constructor_refusals(pkg, lib, kw, words):
    with pytest.raises(lib.CBinferError, match=words):
        pkg.CBResize2d(**kw)


def test_forward_refusals_name_the_keyword(pkg, lib):
    x, plain = torch.zeros(1, 3, 6, 7), pkg.CBResize2d(size=(4, 5))
    const, frame = pkg.CBResize2d(grid=G), pkg.CBResize2d(padding_mode='border', mode='bicubic')
    for module, kw, words in ((plain, dict(grid=G), "grid= needs"), (plain, dict(flow=G), "flow= needs"),
                              (const, dict(size=(4, 5)), "size="), (const, dict(grid=G), "takes no grid="),
                              (const, dict(flow=G), "takes no flow="), (frame, dict(), "every frame"),
                              (frame, dict(grid=G, flow=G), "only one of grid= and flow="),
                              (frame, dict(flow=G), r"\[1, 2, Ho, Wo\]"), (frame, dict(grid=G.long()), "float32 or float16"),
                              (frame, dict(grid=G), "HIP devices only")):
        with pytest.raises(lib.CBinferError, match=words):
            module(x, **kw)
    with pytest.raises(lib.CBinferError, match="gridTypes maps a class"):
        pkg.insertCBResize(torch.nn.Sequential(), gridTypes={torch.nn.ReLU: 3})


def test_constant_grid_is_a_persistent_buffer(pkg):
    m = pkg.CBResize2d(grid=G + 0.25, mode='bilinear', padding_mode='reflection', align_corners=True)
    assert (m.mode, m.padding_mode, m.align_corners) == ('bilinear', 'reflection', True)
    assert list(m.state_dict()) == ['outputState', 'grid'] and list(pkg.CBResize2d(size=(3, 3)).state_dict()) == ['outputState']
    again = pickle.loads(pickle.dumps(m))
    assert torch.equal(again.grid, G + 0.25) and again.padding_mode == 'reflection'
    other = pkg.CBResize2d(grid=G)
    other.load_state_dict(m.state_dict())
    assert torch.equal(other.grid, G + 0.25)
    assert m.half().grid.dtype == torch.float32 and m.outputState.dtype == torch.float16      # the grid keeps its bits
    for theta, align in ((THETA, False), (THETA[None].half(), True)):      # theta= is F.affine_grid bit for bit
        m = pkg.CBResize2d(theta=theta, size=(6, 9), mode='bilinear', align_corners=align)
        assert torch.equal(m.grid, F.affine_grid(theta.float().reshape(1, 2, 3), (1, 1, 6, 9), align_corners=align))


def warp_struct(lib, Ho=4, Wo=5, mode=1, pad=0, ac=0, kind=0, cdt=None):
    return ctypes.pointer(lib.Warp(Ho, Wo, mode, pad, ac, kind, lib.CB_F32 if cdt is None else cdt))


def test_warp_supported_over_its_limits(lib):
    sup, top = lib.C.cbinfer_warp_supported, (1 << 15) - 1
    for mode in range(3):
        for pad in range(3):
            assert sup(warp_struct(lib, top, 1, mode, pad, 1, 1, lib.CB_F16), 1, top) == 1
    assert sup(None, 4, 5) == 0
    for bad, Hi, Wi in ((warp_struct(lib, top + 1), 4, 5), (warp_struct(lib, 4, top + 1), 4, 5), (warp_struct(lib), top + 1, 5),
                        (warp_struct(lib), 4, top + 1), (warp_struct(lib, 0), 4, 5), (warp_struct(lib), 4, 0),
                        (warp_struct(lib, mode=3), 4, 5), (warp_struct(lib, mode=-1), 4, 5), (warp_struct(lib, pad=3), 4, 5),
                        (warp_struct(lib, ac=2), 4, 5), (warp_struct(lib, kind=2), 4, 5), (warp_struct(lib, cdt=7), 4, 5)):
        assert sup(bad, Hi, Wi) == 0


def test_entry_point_checks_its_arguments(lib):
    """Bad arguments return CB_ERR_BADARG (-1) before anything is launched (the device pointers are never followed)."""
    X, CO, O, INB, BITS, COPY, M, L, N2 = (0x10000 * i for i in range(1, 10))
    assert {'cbinfer_warp_supported', 'cbinfer_cbwarp_forward'} <= set(lib.EXPORTED_SYMBOLS) and lib.ABI_VERSION == 11

    def go(x=X, co=CO, o=O, xm=None, xl=None, xc=0, xn=None, cm=None, cl=None, cc=0, cn=None, inb=INB, bits=BITS, cp=COPY,
           Cn=3, Hi=4, Wi=5, wp=warp_struct(lib), dt=lib.CB_F32):
        return lib.C.cbinfer_cbwarp_forward(x, co, o, xm, xl, xc, xn, cm, cl, cc, cn, inb, bits, cp, Cn, Hi, Wi, wp, dt, None)

    for bad in (dict(x=None), dict(co=None), dict(o=None), dict(o=X), dict(o=CO), dict(inb=None), dict(bits=None),
                dict(cp=None), dict(cp=BITS), dict(inb=BITS), dict(inb=COPY), dict(wp=None), dict(Cn=0), dict(Hi=0),
                dict(Wi=1 << 15), dict(dt=7), dict(Cn=1 << 25), dict(xl=L, xc=-1), dict(cl=L, cc=-1), dict(xm=M, xl=L),
                dict(cm=M, cl=L), dict(xn=N2), dict(cn=N2), dict(xm=INB), dict(xm=BITS), dict(xm=COPY), dict(cm=INB),
                dict(cm=BITS), dict(cm=COPY), dict(wp=warp_struct(lib, mode=5)), dict(wp=warp_struct(lib, cdt=9))):
        assert go(**bad) == -1, bad
