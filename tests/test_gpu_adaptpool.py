"""-m gpu tests of the change-based adaptive pool (cb_adaptpool.hip) against the numpy twin of
tests/adaptpool_cases.py, which restates the specification of include/cbinfer_hip.h: through the C ABI and through
CBPoolAvg2d / CBPoolMax2d, a five-frame walk per case -- fresh, a few pixels, none, every pixel, one pixel -- after every
frame of which output AND partials are the twin's of that frame alone, bit for bit, the mask copy is the footprint and the
working masks are zero.  There is no tolerance anywhere in this file."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import adaptpool_cases as ac
from adaptpool_cases import CASE_IDS, CASES, DTYPES, OPS
from optest import dev_words, host_words, lib, gpu_pkg as pkg, stream      # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def walks():
    """The frames, change sets and twin results of every (case, dtype, op): computed once, never written."""
    cache = {}

    def get(cid, dtype, op):
        key = (cid, dtype)
        if key not in cache:
            cache[key] = ac.frames(cid, dtype)
        if key + (op,) not in cache:
            cache[key + (op,)] = [ac.twin(x, CASES[cid][3], op) for x in cache[key][0]]
        return cache[key] + (cache[key + (op,)],)
    return get


def op_code(lib, op):
    return lib.ADAPT_MAX if op == "max" else lib.ADAPT_AVG


def dt_code(lib, dtype):
    return lib.CB_F32 if dtype == "f32" else lib.CB_F16


class State(object):
    """The caller-owned buffers of one pool through the C ABI; partials and output start as NaN."""

    def __init__(self, lib, cid, dtype):
        self.lib = lib
        self.C, self.H, self.W, size = CASES[cid]
        self.oh, self.ow = ac.out_size(self.H, self.W, size)
        n = lib.C.cbinfer_adaptive_pool_partial_elems(self.C, self.H, self.W, self.oh, self.ow)
        assert n == self.C * self.H * self.ow
        self.P = torch.full((n,), float('nan'), device="cuda")
        self.out = torch.full((self.C, self.oh, self.ow), float('nan'), device="cuda",
                              dtype=torch.float32 if dtype == "f32" else torch.float16)
        self.inBits = torch.zeros(lib.C.cbinfer_mask_words(self.H, self.W), dtype=torch.int64, device="cuda")
        self.outBits = torch.zeros(lib.C.cbinfer_mask_words(self.oh, self.ow), dtype=torch.int64, device="cuda")
        self.copy = torch.full_like(self.outBits, -1)
        self.dtype = dtype

    def frame(self, x, op, form, changed):
        """form 'bare' (every pixel), 'mask' or 'list' (device-side count below the capacity; the entries behind the
        count name other pixels, which must not be listed)."""
        lib, ptr = self.lib, self.lib.ptr
        xd = torch.from_numpy(x).cuda()
        mask = lst = cnt = None
        cap = 0
        if form == "mask":
            mask = dev_words(ac.pack(changed))
        elif form == "list":
            idx = np.flatnonzero(changed.reshape(-1)).astype(np.int32)
            rest = np.flatnonzero(~changed.reshape(-1)).astype(np.int32)[:5]
            outside = np.array([-7, self.H * self.W], dtype=np.int32)      # (entries outside the map are dropped)
            lst = torch.from_numpy(np.concatenate([idx, outside, rest])).cuda()
            cnt = torch.tensor([idx.size + 2], dtype=torch.int32, device="cuda")
            cap = lst.numel()
        lib.check(lib.C.cbinfer_cbadaptivepool2d_forward(
            ptr(xd), ptr(self.P), ptr(self.out), ptr(mask), ptr(lst), cap, ptr(cnt), ptr(self.inBits), ptr(self.outBits),
            ptr(self.copy), self.C, self.H, self.W, self.oh, self.ow, op_code(lib, op), dt_code(lib, self.dtype),
            stream()))
        torch.cuda.synchronize()

    def check(self, want, listed, what):
        P, out = want
        assert np.array_equal(ac.bits_of(self.P.cpu().numpy().reshape(P.shape)), ac.bits_of(P)), (what, "partials")
        assert np.array_equal(ac.bits_of(self.out.cpu().numpy()), ac.bits_of(out)), (what, "output")
        assert np.array_equal(host_words(self.copy), ac.pack(listed)), (what, "mask copy")
        assert not self.inBits.any().item() and not self.outBits.any().item(), (what, "working masks")


def listed_of(changed, form, shape):
    oh, ow = shape
    if changed is None or form == "bare":
        return np.ones((oh, ow), dtype=bool)
    return ac.footprint(changed, oh, ow)[0]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("cid", CASE_IDS)
def test_walk_through_the_c_abi(lib, walks, cid, op, dtype):
    """Every form of the operand walks the same five frames to the twin's bits, so the forms agree bit for bit too."""
    (xs, sets, want) = walks(cid, dtype, op)
    for form in ("bare", "mask", "list"):
        st = State(lib, cid, dtype)
        for k, (x, changed) in enumerate(zip(xs, sets)):
            st.frame(x, op, "bare" if changed is None else form, changed)
            st.check(want[k], listed_of(changed, form, (st.oh, st.ow)), (form, k))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("cid", CASE_IDS)
def test_the_partials_are_really_used(lib, walks, cid, op, dtype):
    """Frame 2 with a NaN at every input pixel that lies in no (row, column window) segment holding a listed pixel:
    the result is still the twin's of the true frame -- a kernel that recomputes windows from the input cannot pass
    (where the map has a clean segment at all)."""
    (xs, sets, want) = walks(cid, dtype, op)
    changed = sets[1]
    _, H, W, size = CASES[cid]
    oh, ow = ac.out_size(H, W, size)
    _, dirty = ac.footprint(changed, oh, ow)
    safe = np.zeros((H, W), dtype=bool)
    for j in range(ow):
        safe[:, ac.lo(j, W, ow):ac.hi(j, W, ow)] |= dirty[:, j:j + 1]
    poisoned = xs[1].copy()
    poisoned[:, ~safe] = np.nan
    assert not np.isnan(want[1][1].astype(np.float32)).any()
    for form in ("mask", "list"):
        st = State(lib, cid, dtype)
        st.frame(xs[0], op, "bare", None)
        st.frame(poisoned, op, form, changed)
        st.check(want[1], listed_of(changed, form, (oh, ow)), (form, int((~safe).sum())))


def test_max_nan_and_signed_zeros_on_the_device(lib):
    """A NaN wins; {+0, -0, -0, +0} gives +0 and its negation -0: CPU torch's bits."""
    for dtype in DTYPES:
        dt = ac.np_dtype(dtype)
        z = np.array([[0.0, -0.0], [-0.0, 0.0]], dtype=dt)
        wide = np.full((3, 7, 70), -3.0, dtype=dt)
        wide[0, 1:3, 22:24] = z
        wide[1, 1:3, 22:24] = -z
        wide[2, 3, 64] = np.nan
        for size in ((1, 1), (2, 3), (7, 70)):
            P = torch.full((3 * 7 * size[1],), 1.0, device="cuda")
            out = torch.zeros((3,) + size, device="cuda", dtype=torch.float32 if dtype == "f32" else torch.float16)
            bits = [torch.zeros(lib.C.cbinfer_mask_words(*size), dtype=torch.int64, device="cuda") for _ in range(2)]
            xd = torch.from_numpy(wide).cuda()
            lib.check(lib.C.cbinfer_cbadaptivepool2d_forward(
                lib.ptr(xd), lib.ptr(P), lib.ptr(out), None, None, 0, None, None,
                lib.ptr(bits[0]), lib.ptr(bits[1]), 3, 7, 70, size[0], size[1], lib.ADAPT_MAX, dt_code(lib, dtype),
                stream()))
            got = out.cpu().numpy()
            ref = F.adaptive_max_pool2d(torch.from_numpy(wide)[None], size)[0].numpy()
            assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.isnan(got).any()
            ok = ~np.isnan(ref)
            assert np.array_equal(ac.bits_of(got)[ok], ac.bits_of(ref)[ok]), (dtype, size)


# ------------------------------------------------------------------------------------------------ the modules
def make_module(pkg, op, size):
    if op == "max":
        m = pkg.CBPoolMax2d(nn.AdaptiveMaxPool2d(size), generalGeometry=True)
    else:
        m = pkg.CBPoolAvg2d(nn.AdaptiveAvgPool2d(size))
    m.propChangeIndexes = True
    return m.cuda()


def operand(pkg, form, changed, H, W):
    """The producer's change information in the three forms a module is handed."""
    from cbinfer_amd.conv2d_cg import MaskChangeIndexes
    idx = np.flatnonzero(changed.reshape(-1)).astype(np.int32)
    if form == "tensor":
        return torch.from_numpy(idx).cuda()
    buf = torch.full((H * W,), 0, dtype=torch.int32, device="cuda")
    buf[:idx.size] = torch.from_numpy(idx).cuda()
    cnt = torch.tensor([idx.size], dtype=torch.int32, device="cuda")
    if form == "list":      # (a device-side count below the capacity; the entries behind it name pixel 0)
        return pkg.ChangeIndexes(buf, cnt, size=(H, W))
    return MaskChangeIndexes(dev_words(ac.pack(changed)), (H, W), buf, cnt)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("cid", CASE_IDS)
def test_walk_through_the_modules(pkg, walks, cid, op, dtype):
    (xs, sets, want) = walks(cid, dtype, op)
    Cn, H, W, size = CASES[cid]
    oh, ow = ac.out_size(H, W, size)
    for form in ("mask", "list", "tensor"):
        m = make_module(pkg, op, size)
        for k, (x, changed) in enumerate(zip(xs, sets)):
            xd = torch.from_numpy(x).cuda()[None]
            # the fresh frame is handed an EMPTY list: a state that does not fit makes every pixel count as changed
            given = np.zeros((H, W), dtype=bool) if changed is None else changed
            tag, y, ix = m(('changeIndexes', xd, operand(pkg, form, given, H, W)))
            torch.cuda.synchronize()
            P, out = want[k]
            assert tag == 'changeIndexes' and y is not m.outputState and tuple(y.shape) == (1, Cn, oh, ow)
            assert m.partials.dtype == torch.float32 and tuple(m.partials.shape) == (Cn, ow, H)
            assert np.array_equal(ac.bits_of(m.partials.cpu().numpy()), ac.bits_of(P)), (form, k)
            assert np.array_equal(ac.bits_of(m.outputState[0].cpu().numpy()), ac.bits_of(out)), (form, k)
            assert torch.equal(y, m.outputState)
            assert ix.size == (oh, ow)
            assert np.array_equal(host_words(ix._mask), ac.pack(listed_of(changed, form, (oh, ow)))), (form, k)
            work = m.__dict__['_poolWork']
            assert not work['bits'].any().item() and not work['inBits'].any().item(), (form, k)
            # the list a consumer may ask for: the listed output pixels, ascending
            assert ix.tensor().cpu().tolist() == np.flatnonzero(listed_of(changed, form, (oh, ow))).tolist()


def test_module_state_surface_on_the_device(pkg, lib):
    m = make_module(pkg, "avg", (2, None))
    m.cloneOutput = False
    x = torch.randn(1, 3, 5, 9, device="cuda")
    none = torch.zeros(0, dtype=torch.int32, device="cuda")
    tag, y, ix = m(('changeIndexes', x, none))
    assert y is m.outputState and getattr(y, '_cbinfer_inplace_state', False) and tuple(y.shape) == (1, 3, 2, 9)
    assert [tuple(t.shape) for t in m.getStateTensors()] == [(1, 3, 2, 9), (3, 9, 5)]
    first = m.outputState.clone()
    # an empty change set: nothing is written, also not from an input that differs
    m(('changeIndexes', torch.randn_like(x), none))
    assert torch.equal(m.outputState, first)
    # another dtype, another map, a cleared state: fresh frames, equal to the twin of their own input
    for xn in (x.half(), torch.randn(1, 3, 6, 9, device="cuda"), None):
        if xn is None:
            m.clearMemory()
            assert m.partials.numel() == 0 and m.outputState.numel() == 0
            xn = x
        m(('changeIndexes', xn, none))
        _, want = ac.twin(xn[0].cpu().numpy(), (2, None), "avg")
        assert np.array_equal(ac.bits_of(m.outputState[0].cpu().numpy()), ac.bits_of(want))
    # a pool always stands behind a producer; an output larger than the map is refused at the frame, naming the map
    with pytest.raises(lib.CBinferError, match="change indexes must be an int32 tensor or a ChangeIndexes"):
        m(('changeIndexes', x, None))
    with pytest.raises(lib.CBinferError, match=r"output_size=\(7, 7\) is larger than the 5x9 map"):
        make_module(pkg, "max", 7)(('changeIndexes', x, none))
    with pytest.raises(lib.CBinferError, match="address a 4x4 map, this pool's input map is 5x9"):
        m(('changeIndexes', x, pkg.ChangeIndexes(torch.zeros(16, dtype=torch.int32, device="cuda"),
                                                 torch.zeros(1, dtype=torch.int32, device="cuda"), size=(4, 4))))


# ------------------------------------------------------------------------------------------------ a gate in the chain
class Squeeze(nn.Module):
    """y = conv(x); out = y * hardsigmoid(amax(y)): the squeeze of an SE block with a max pool, every step a library
    call."""

    def __init__(self, pkg):
        super(Squeeze, self).__init__()
        torch.manual_seed(11)
        self.conv = pkg.convert(nn.Sequential(nn.Conv2d(3, 6, 3, padding=1)).eval().cuda(), threshold=0.05)[0]
        self.conv.propChangeIndexes = True
        self.pool = pkg.CBPoolMax2d(nn.AdaptiveMaxPool2d(1), generalGeometry=True)
        self.pool.propChangeIndexes = True
        self.act = pkg.CBPointwise2d(nn.Hardsigmoid())
        self.mul = pkg.CBBinary2d('mul')
        self.pool.cloneOutput = self.act.cloneOutput = self.mul.cloneOutput = False

    def forward(self, x):
        y = self.conv(x)
        return self.mul(y, self.act(self.pool(y)))


def gate_frames(n, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(1, 3, 12, 70, generator=g)
    frames = [x.clone()]
    for t in range(1, n):
        x = x.clone()
        y0, x0 = (3 * t) % 8, (17 * t) % 60
        x[:, :, y0:y0 + 4, x0:x0 + 9] = torch.randn(1, 3, 4, 9, generator=g)
        frames.append(x)
    return [f.cuda() for f in frames]


def test_a_gate_in_the_chain(pkg, lib):
    """CBConv2d -> CBPoolMax2d(AdaptiveMaxPool2d(1)) -> CBPointwise2d(Hardsigmoid); the bare [1, C, 1, 1] result gates
    the conv's output in CBBinary2d('mul').  Equal to torch's y * hardsigmoid(amax(y)) on the conv's own output bit for
    bit over three frames; records as a FrameProgram with cloneOutput=False and replays equal to eager."""
    net = Squeeze(pkg)
    frames = gate_frames(6, 5)
    with torch.no_grad():
        for t, f in enumerate(frames[:3]):
            out = net(f)
            y = net.conv.prevOutput.cpu()
            assert tuple(y.shape) == (1, 6, 12, 70) and out is net.mul.outputState
            want = y * F.hardsigmoid(torch.amax(y, dim=(2, 3), keepdim=True))
            assert tuple(net.pool.outputState.shape) == (1, 6, 1, 1)
            assert torch.equal(net.pool.outputState.cpu(), torch.amax(y, dim=(2, 3), keepdim=True)), t
            assert np.array_equal(ac.bits_of(out.cpu().numpy()), ac.bits_of(want.numpy())), t
        eager = copy.deepcopy(net)
        prog = pkg.FrameProgram(net)
        for t, f in enumerate(frames[3:]):
            yp, ye = prog(f), eager(f)
            assert np.array_equal(ac.bits_of(yp.cpu().numpy()), ac.bits_of(ye.cpu().numpy())), t
            for ta, tb in zip(pkg.getStateTensors(net), pkg.getStateTensors(eager)):
                assert torch.equal(ta, tb), t
        raws = [fn for fn, _ in prog.calls]
        assert raws.count(lib.C.cbinfer_cbadaptivepool2d_forward.raw) == 1
