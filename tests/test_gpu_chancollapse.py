"""-m gpu tests of the change-based reductions that collapse the channel axis (CBChannelReduce2d's ops 'sum', 'mean',
'norm', 'max', 'min', 'argmax', 'argmin'; cb_chancollapse.hip).  The specification is the numpy twin of
tests/chancollapse_cases.py (rules 1-4 there): SUM / MEAN / NORM are compared bit for bit with it and against float64
under its bounds; the arg and extreme kinds bit for bit with torch.max / torch.min on the CPU copy."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn

import chancollapse_cases as cc
from optest import (chain_frames, dev, dev_words, host_words, LayerSpy, lib,      # noqa: F401  (fixtures)
                    operand_args, gpu_pkg as pkg, raw, stream, walk_frames)

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float16]
FILL = {np.float32: 0x5BCD5BCD, np.float16: 0x5BCD}
LABEL_FILL = -7
WORST = {}      # (kind name, dtype name) -> worst err / bound seen against float64
ALL_CALLS = [(k,) for k in range(7)] + [(cc.SUM, cc.MEAN, cc.NORM, cc.MAX), (cc.MEAN, cc.MAX), (cc.MIN, cc.MAX)]


def is_arg(kinds):
    return kinds[0] in cc.ARG_KINDS


def forward(lib, dx, dout, args, bits, mcopy, label, kinds):
    """cbinfer_cbchancollapse_forward with the operand `args` = (mask, list, capacity, device count)."""
    Cn, H, W = dx.shape
    mask, lst, cap, cnt = args
    ptr = lib.ptr
    return lib.C.cbinfer_cbchancollapse_forward(ptr(dx), ptr(dout), ptr(mask), ptr(lst), cap, ptr(cnt), ptr(bits),
                                                ptr(mcopy), ptr(label), Cn, H, W, cc.packed(kinds), len(kinds),
                                                lib.CB_F32 if dx.dtype == torch.float32 else lib.CB_F16, stream())


def new_state(kinds, H, W, dtype):
    """A state filled with a pattern no result has: [K, H, W] of dtype, or the int64 label map [H, W]."""
    if is_arg(kinds):
        return np.full((H, W), LABEL_FILL, dtype=np.int64)
    out = np.empty((len(kinds), H, W), dtype=dtype)
    cc.bits_of(out)[...] = FILL[dtype]
    return out


def run_frames(lib, shape, dtype, form, kinds, rng, values, check):
    """The six mask patterns as consecutive frames through cbinfer_cbchancollapse_forward.  Before every frame x gets new
    values at the frame's pixels AND at one pixel outside them; check(x, got, listed, where) judges the values at the
    listed pixels; unlisted pixels must keep their bits, maskCopy be the frame's mask, the working mask zero; an arg
    launch's label mask -- full of stale bits before every launch -- must be listed & (all form | new != old), in every
    word.  The walk is optest.walk_frames; the label mask rides in its call and check.  Returns (frames with an unlisted
    pixel, x at the listed pixels of all frames [C, n])."""
    Cn, H, W = shape
    words = lib.C.cbinfer_mask_words(H, W)
    label = torch.empty(words, dtype=torch.int64, device="cuda") if is_arg(kinds) else None
    prev, seen = [new_state(kinds, H, W, dtype)], []

    def call(dx, dout, mask, lst, cap, cnt, bits, mcopy):
        if label is not None:
            label.fill_(-1)
        return forward(lib, dx, dout, (mask, lst, cap, cnt), bits, mcopy, label, kinds)

    def judge(x, got, listed, where):
        check(x, got, listed, where)
        if label is not None:
            moved = listed & (np.ones((H, W), dtype=bool) if form == "all" else got != prev[0])
            assert np.array_equal(host_words(label), cc.pack(moved)), where
        seen.append(x[:, listed].copy())
        prev[0] = got
    saw = walk_frames(lib, shape, dtype, form, lambda: cc.patterns(rng, H, W), call, judge, prev[0],
                      lambda: values(rng, shape, dtype), what=([cc.NAMES[k] for k in kinds],))
    return saw, np.concatenate(seen, axis=1)


def check_float_kinds(kinds):
    """SUM / MEAN / NORM (and the extremes of a mixed call) at the listed pixels: the twin's bits, NaNs in the same
    places; against float64 under chancollapse_cases.bound where every channel is finite and no float32 intermediate
    overflows; a float16 result beyond the format's range is the infinity of its sign."""
    def check(x, got, listed, where):
        xs = x[:, listed]
        want = cc.twin_values(xs, kinds)
        g = got[:, listed]
        nan = np.isnan(want)
        bad = (np.isnan(g) != nan) | ((cc.bits_of(g) != cc.bits_of(want)) & ~nan)
        assert not bad.any(), (where, int(bad.sum()), g[bad][:4], want[bad][:4])
        tame = np.isfinite(xs.astype(np.float32)).all(axis=0) & (np.abs(xs.astype(np.float32)).max(axis=0) <= 65504.0)
        for k, kind in enumerate(kinds):
            if kind not in cc.FLOAT_KINDS or not tame.any():
                continue
            ref = cc.reference64(xs[:, tame], kind)
            bnd = cc.bound(xs[:, tame], kind, ref)
            gk = g[k][tame].astype(np.float64)
            fin = np.ones(ref.shape, dtype=bool)
            if x.dtype == np.float16:
                sure, fin = np.abs(ref) - bnd >= 65520.0, np.abs(ref) + bnd < 65520.0
                assert np.array_equal(gk[sure], np.sign(ref[sure]) * np.inf), where
            err = np.abs(gk[fin] - ref[fin])
            key = (cc.NAMES[kind], np.dtype(x.dtype).name)
            if fin.any():
                WORST[key] = max(WORST.get(key, 0.0), float((err / bnd[fin]).max()))
            assert np.all(err <= bnd[fin]), (where, key, float((err / bnd[fin]).max()))
    return check


def torch_extreme(xs, kind):
    """torch.max / torch.min(x, 1) on the CPU for xs [C, n]: (values, indices) as numpy."""
    r = (torch.max if kind in (cc.MAX, cc.ARGMAX) else torch.min)(torch.from_numpy(np.ascontiguousarray(xs.T)), 1)
    return r.values.numpy(), r.indices.numpy()


def check_against_torch(kinds):
    """The arg and extreme kinds at the listed pixels: torch's CPU result bit for bit (NaNs in the same places)."""
    def check(x, got, listed, where):
        xs = x[:, listed]
        for k, kind in enumerate(kinds):
            values, indices = torch_extreme(xs, kind)
            if kind in cc.ARG_KINDS:
                assert np.array_equal(got[listed], indices), (where, cc.NAMES[kind])
            else:
                g = got[k][listed]
                assert cc.same_bits(g, values), (where, cc.NAMES[kind], g[:8], values[:8])
    return check


@pytest.mark.parametrize("form", cc.FORMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
def test_sum_mean_norm_equal_the_twin_bit_for_bit(lib, dtype, form):
    """Every shape of chanreduce_cases.SHAPES; SUM, MEAN, NORM alone and the four-op call (SUM, MEAN, NORM, MAX): at the
    listed pixels the state has the twin's bits, -0, +-inf, +-1e30 and +-65504 among the values; under the float64
    bounds; everything else as run_frames says.  A contracted FMA, another summation order, an approximate division or
    square root, or ops of one call that disturb each other would show here."""
    rng = np.random.default_rng(11)
    saw = 0
    calls = [(cc.SUM,), (cc.MEAN,), (cc.NORM,), (cc.SUM, cc.MEAN, cc.NORM, cc.MAX)]
    for shape in cc.SHAPES:
        for kinds in calls:
            saw += run_frames(lib, shape, dtype, form, kinds, rng, cc.values, check_float_kinds(kinds))[0]
    assert form == "all" or saw >= 4 * len(cc.SHAPES) * len(calls)
    for (name, dt), w in sorted(WORST.items()):
        if dt == np.dtype(dtype).name:
            print("%s %s %s: worst err / bound = %.3f" % (name, dt, form, w))


@pytest.mark.parametrize("form", cc.FORMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
def test_arg_and_extreme_kinds_equal_torch_bit_for_bit(lib, dtype, form):
    """ARGMAX, ARGMIN, MAX, MIN and the two-op call (MIN, MAX) on values that make ties the rule -- {-2, .., 2} with +0 and
    -0 mixed, a NaN pixel one in eight --: torch.max / torch.min of the CPU copy bit for bit, indices and values; the
    label mask of the arg kinds as run_frames says.  Each run asserts that its inputs are what they claim: with C >= 16
    at least half of the listed NaN-free pixels attain their extreme in two or more slices, and at least three quarters
    of the listed pixels are NaN-free."""
    rng = np.random.default_rng(13)
    for shape in cc.SHAPES:
        for kinds in ((cc.ARGMAX,), (cc.ARGMIN,), (cc.MAX,), (cc.MIN,), (cc.MIN, cc.MAX)):
            _, xs = run_frames(lib, shape, dtype, form, kinds, rng, cc.tie_values, check_against_torch(kinds))
            clean = cc.nan_free(xs)
            assert 4 * int(clean.sum()) >= 3 * xs.shape[1], (shape, kinds)
            if shape[0] >= 16:
                for kind in kinds:
                    tied = cc.extreme_in_two_slices(xs[:, clean], kind)
                    assert 2 * int(tied.sum()) >= int(clean.sum()), (shape, cc.NAMES[kind], float(tied.mean()))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
def test_arg_kinds_on_values_with_infinities_and_large_numbers(lib, dtype):
    """The arg and extreme kinds once more on chanreduce_cases.values (+-inf, +-65504, +-1e30, NaN, -0 among uniform
    values, where ties are rare), C on both sides of 16, in list form."""
    rng = np.random.default_rng(15)
    for shape in ((3, 5, 64), (40, 1, 130), (300, 5, 130)):
        for kinds in ((cc.ARGMAX,), (cc.ARGMIN,), (cc.MIN, cc.MAX)):
            run_frames(lib, shape, dtype, "list", kinds, rng, cc.values, check_against_torch(kinds))


def test_label_mask_is_empty_where_scores_move_and_labels_stay(lib):
    """Frame 1 writes every label (all form: the label mask is the whole map).  Frame 2 doubles every score -- every
    pixel is listed and every score changes, no label does --: the label mask is zero in every word although it held
    stale bits, maskCopy is the full mask.  Frame 3 moves the label of three pixels: exactly their bits."""
    Cn, H, W = 21, 6, 130
    rng = np.random.default_rng(7)
    x = rng.uniform(-4, 4, (Cn, H, W)).astype(np.float32)
    words = lib.C.cbinfer_mask_words(H, W)
    dout = torch.full((H, W), LABEL_FILL, dtype=torch.int64, device="cuda")
    bits = torch.zeros(words, dtype=torch.int64, device="cuda")
    mcopy = torch.zeros(words, dtype=torch.int64, device="cuda")
    label = torch.full((words,), -1, dtype=torch.int64, device="cuda")
    full = np.ones((H, W), dtype=bool)
    assert forward(lib, dev(x), dout, operand_args("all", full), bits, mcopy, label, (cc.ARGMAX,)) == 0
    assert np.array_equal(host_words(label), cc.pack(full))
    first = dout.cpu().numpy()
    assert np.array_equal(first, x.argmax(axis=0))
    label.fill_(-1)
    assert forward(lib, dev(x * 2), dout, operand_args("mask", full), bits, mcopy, label, (cc.ARGMAX,)) == 0
    assert int(label.ne(0).sum()) == 0 and np.array_equal(host_words(mcopy), cc.pack(full))
    assert np.array_equal(dout.cpu().numpy(), first)
    x2 = x * 2
    movedPixels = [(0, 0), (3, 64), (5, 129)]
    for y, xx in movedPixels:
        x2[(first[y, xx] + 1) % Cn, y, xx] = 100.0
    S = rng.random((H, W)) < 0.3
    for y, xx in movedPixels:
        S[y, xx] = True
    label.fill_(-1)
    assert forward(lib, dev(x2), dout, operand_args("list", S), bits, mcopy, label, (cc.ARGMAX,)) == 0
    want = np.zeros((H, W), dtype=bool)
    for y, xx in movedPixels:
        want[y, xx] = True
    assert np.array_equal(host_words(label), cc.pack(want)) and np.array_equal(host_words(mcopy), cc.pack(S))
    assert np.array_equal(dout.cpu().numpy(), x2.argmax(axis=0))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
def test_a_pixel_does_not_depend_on_the_list_the_form_or_the_run(lib, dtype):
    """One pixel's result, every kind and three multi-op calls, C = 300: listed alone (one bit in its word), in a list
    of at most 16 in its word, in a half-full random crowd, in a full row, and with every pixel listed, each twice: always
    the same bits.  This is the test a summation order that depends on the word's popcount fails."""
    Cn, H, W = 300, 5, 130
    rng = np.random.default_rng(17)
    x = cc.values(rng, (Cn, H, W), dtype, 8.0, np.array([0.0, -0.0, 3.0, -3.0, 6.0], dtype=dtype))
    dx = dev(x)
    py, px = 3, 70
    alone = np.zeros((H, W), dtype=bool)
    alone[py, px] = True
    few = alone.copy()
    few[py, 64:128:7] = True
    assert 1 < few[py, 64:128].sum() <= 16
    crowd = rng.random((H, W)) < 0.5
    crowd[py, px] = True
    assert 16 < crowd[py, 64:128].sum() < 64
    row = np.zeros((H, W), dtype=bool)
    row[py, :] = True
    words = lib.C.cbinfer_mask_words(H, W)
    for kinds in ALL_CALLS:
        seen = []
        for rep in range(2):
            for form, S in (("mask", alone), ("list", alone), ("mask", few), ("list", few), ("list", crowd),
                            ("mask", crowd), ("list", row), ("mask", row), ("all", alone)):
                dout = dev(new_state(kinds, H, W, dtype))
                bits = torch.zeros(words, dtype=torch.int64, device="cuda")
                mcopy = torch.zeros(words, dtype=torch.int64, device="cuda")
                assert forward(lib, dx, dout, operand_args(form, S, 0, bool(rep % 2)), bits, mcopy, None, kinds) == 0
                seen.append(cc.bits_of(dout[..., py, px].cpu().numpy()).copy())
        assert all(np.array_equal(s, seen[0]) for s in seen[1:]), kinds
        want = cc.twin_arg(x[:, py, px:px + 1], kinds[0])[0] if is_arg(kinds) else cc.bits_of(
            cc.twin_values(x[:, py, px:px + 1], kinds)[:, 0])
        assert np.array_equal(seen[0], want), kinds


def test_chancollapse_changed_takes_the_mask_as_the_working_mask(lib):
    """cbinfer_chancollapse_changed alone: the listed pixels given in `bits` (what a list leaves there), a second set in
    the operand's mask; both are recomputed, the working mask comes back zero and the union is handed on."""
    C, ptr = lib.C, lib.ptr
    Cn, H, W = 19, 4, 70
    rng = np.random.default_rng(5)
    x = cc.values(rng, (Cn, H, W), np.float32)
    A, B = rng.random((H, W)) < 0.2, rng.random((H, W)) < 0.2
    dx, dout = dev(x), torch.zeros((2, H, W), device="cuda")
    bits, mask = dev_words(cc.pack(A)), dev_words(cc.pack(B))
    mcopy = torch.zeros(C.cbinfer_mask_words(H, W), dtype=torch.int64, device="cuda")
    kinds = (cc.MEAN, cc.MAX)
    assert C.cbinfer_chancollapse_changed(ptr(dx), ptr(dout), ptr(mask), 0, ptr(bits), ptr(mcopy), None, Cn, H, W,
                                          cc.packed(kinds), 2, lib.CB_F32, stream()) == 0
    got, want = dout.cpu().numpy(), cc.twin_values(x, kinds)
    U = A | B
    assert cc.same_bits(got[:, U], want[:, U]) and not cc.bits_of(got)[:, ~U].any()
    assert int(bits.ne(0).sum()) == 0 and np.array_equal(host_words(mcopy), cc.pack(U))
    assert np.array_equal(host_words(mask), cc.pack(B))      # (the operand's mask is read only)


# ------------------------------------------------------------------------------------------------ the module
def module_twin(m, x):
    """The twin of the collapsing module `m` on the numpy map x [C, H, W]: the state without its batch axis."""
    kinds = [cc.OP_NAMES.index(n) for n in m.collapseOps[0]]
    if is_arg(kinds):
        lab = cc.twin_arg(x, kinds[0])
        return lab[None] if m.keepdim else lab
    vals = cc.twin_values(x, kinds)
    return vals if m.keepdim else vals[0]


def state_equals(state, want):
    got = state[0].cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype)
    return np.array_equal(got, want) if got.dtype == np.int64 else cc.same_bits(got, want)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
def test_module_forms_flags_and_errors(pkg, lib, dtype):
    """CBChannelReduce2d with the collapsing ops: a new state is written completely whatever the list says; a
    MaskChangeIndexes is taken as its mask and its list never made; ChangeIndexes and exact tensors as lists; keepdim;
    the state's shape and dtype; cloneOutput=False hands out the tagged state; labelChanges hands on the narrower mask and
    its list; reallocation on a new resolution; clearMemory; the refusals."""
    from cbinfer_amd.conv2d_cg import ChangeIndexes, MaskChangeIndexes
    Cn, H, W = 21, 7, 70
    rng = np.random.default_rng(3)
    tdt = torch.float32 if dtype == np.float32 else torch.float16
    for op, kw, shape, sdt in (('sum', {}, (1, 1, H, W), tdt), ('norm', dict(keepdim=False), (1, H, W), tdt),
                               (('mean', 'max'), {}, (1, 2, H, W), tdt), (('sum', 'mean', 'norm', 'min'), {}, (1, 4, H, W), tdt),
                               ('argmax', {}, (1, 1, H, W), torch.int64), ('argmin', dict(keepdim=False), (1, H, W), torch.int64),
                               ('argmax', dict(labelChanges=True), (1, 1, H, W), torch.int64)):
        m = pkg.CBChannelReduce2d(op, **kw).cuda()
        m.propChangeIndexes = True
        x = cc.tie_values(rng, (Cn, H, W), dtype)
        empty = torch.zeros(0, dtype=torch.int32, device="cuda")
        tag, y, ix = m(('changeIndexes', dev(x)[None], empty))      # first frame
        assert tag == 'changeIndexes' and tuple(m.outputState.shape) == shape and m.outputState.dtype == sdt
        assert state_equals(m.outputState, module_twin(m, x)), op
        assert y is not m.outputState and torch.equal(raw(y), raw(m.outputState))
        assert isinstance(ix, MaskChangeIndexes) and ix.size == (H, W) and not ix._made
        assert ix.tensor().numel() == H * W      # (also with labelChanges: a first frame moves every label)
        for t in range(4):
            prev = m.outputState[0].cpu().numpy()
            S = rng.random((H, W)) < 0.15
            if t == 3:
                S[:] = False
            fresh = cc.tie_values(rng, (Cn, H, W), dtype)
            x[:, S] = fresh[:, S]
            if not S[6, 69]:
                x[:, 6, 69] = fresh[:, 6, 69]      # (not listed)
            if t % 2 == 0:
                ind = MaskChangeIndexes(dev_words(cc.pack(S)), (H, W), torch.empty(H * W, dtype=torch.int32, device="cuda"),
                                        torch.zeros(1, dtype=torch.int32, device="cuda"))
            else:
                lb = dev(np.flatnonzero(S.reshape(-1)).astype(np.int32))
                ind = lb if t == 3 else ChangeIndexes(torch.cat([lb, lb.new_full((3,), 6 * W + 69)]),
                                                      torch.tensor([lb.numel()], dtype=torch.int32, device="cuda"), (H, W))
            tag, y, ix = m(('changeIndexes', dev(x)[None], ind))
            if t % 2 == 0:
                assert not ind._made      # the producer's list was never materialised
            got = m.outputState[0].cpu().numpy()
            want = module_twin(m, x)
            sel = (Ellipsis, S)
            if got.dtype == np.int64:
                assert np.array_equal(got[sel], want[sel]), (op, t)
            else:
                assert cc.same_bits(got[sel], want[sel]), (op, t)
            assert np.array_equal(cc.bits_of(got)[..., ~S], cc.bits_of(prev)[..., ~S]), (op, t)
            assert np.array_equal(host_words(m._chWork['copy']), cc.pack(S))
            handed = S & (got != prev).reshape(-1, H, W)[0] if m.labelChanges else S
            assert np.array_equal(host_words(ix._mask), cc.pack(handed)), (op, t)
            assert np.array_equal(ix.tensor().cpu().numpy(), np.flatnonzero(handed.reshape(-1))), (op, t)
            if m.labelChanges and t == 0:
                assert 0 < handed.sum() < S.sum()      # (narrower: some listed pixels kept their label)
            assert int(m._chWork['bits'].ne(0).sum()) == 0
        # a bare tensor carries no change information: the dense result; the state itself is handed out, tagged
        m.propChangeIndexes, m.cloneOutput = False, False
        out = m(dev(x)[None])
        assert out is m.outputState and out._cbinfer_inplace_state
        assert state_equals(out, module_twin(m, x))
        # a new resolution: the state and the work buffers are made again, the frame is dense whatever the list says
        x2 = cc.tie_values(rng, (Cn, 3, 9), dtype)
        out = m(('changeIndexes', dev(x2)[None], empty))
        assert tuple(out.shape) == shape[:-2] + (3, 9) and m._chWork['key'][:3] == (Cn, 3, 9)
        assert state_equals(out, module_twin(m, x2))
        # ... and another channel count behind a state that still fits
        x3 = cc.tie_values(rng, (Cn + 2, 3, 9), dtype)
        out = m(('changeIndexes', dev(x3)[None], empty))
        assert state_equals(out, module_twin(m, x3))
        # refusals
        Err = lib.CBinferError
        dx = dev(x3)[None]
        wrong = ChangeIndexes(torch.zeros(4, dtype=torch.int32, device="cuda"),
                              torch.zeros(1, dtype=torch.int32, device="cuda"), (4, 9))
        with pytest.raises(Err, match="4x9 map.*3x9"):
            m(('changeIndexes', dx, wrong))
        with pytest.raises(Err, match="int32"):
            m(('changeIndexes', dx, torch.zeros(3, dtype=torch.int64, device="cuda")))
        with pytest.raises(Err, match="int32 tensor or a ChangeIndexes"):
            m(('changeIndexes', dx, [1, 2]))
        with pytest.raises(Err, match=r"\[1, C, H, W\]"):
            m(torch.cat([dx, dx]))
        with pytest.raises(Err, match="HIP devices only"):
            m(dx.cpu())
        with pytest.raises(Err, match="float32 and float16"):
            m(m.outputState if sdt == torch.int64 and m.keepdim else dx.double())      # (a label map is no operand)
        before = m.outputState.clone()
        torch.cuda.synchronize()
        assert torch.equal(raw(m.outputState), raw(before))
        m.clearMemory()
        assert m.outputState.numel() == 0 and m._chWork is None
        assert state_equals(m(dx), module_twin(m, x3))


# ------------------------------------------------------------------------------------------------ chains
class ArgMax2d(nn.Module):
    def forward(self, x):
        return torch.argmax(x, 1, keepdim=True)


class DenseTwin(nn.Module):
    """The twin applied densely on the CPU in the place of a collapsing CBChannelReduce2d."""

    def __init__(self, m):
        super(DenseTwin, self).__init__()
        self.m = [m]

    def forward(self, inp):
        x = inp[1] if type(inp) == tuple else inp
        return dev(module_twin(self.m[0], x.detach()[0].cpu().numpy()))[None]


def exact(net, tdt):
    if tdt == torch.float32:
        for m in net.modules():
            if type(m).__name__ == 'CBConv2d':
                m.exactF32 = True
    return net


def segmentation_head(pkg, tdt):
    """conv 3x3 8 -> 16, conv 1x1 16 -> 5, argmax over the channels with labelChanges, every threshold 0."""
    torch.manual_seed(95)
    src = nn.Sequential()
    for name, mod in (('feat', nn.Conv2d(8, 16, 3, padding=1)), ('head', nn.Conv2d(16, 5, 1)), ('label', ArgMax2d())):
        src.add_module(name, mod)
    net = pkg.convert(src.eval().cuda().to(tdt), threshold=0.0)
    pkg.insertCBChannelOps(net, reduceTypes={ArgMax2d: 'argmax'})
    assert [type(m).__name__ for m in net] == ['CBConv2d', 'CBConv2d', 'CBChannelReduce2d']
    assert net.head.propChangeIndexes and net.label.collapseOps[0] == ('argmax',)
    net.label.labelChanges = net.label.propChangeIndexes = True
    return exact(net, tdt)


def attention_block(pkg, tdt):
    """CBAM's spatial attention: out = body(x) * sigmoid(conv7x7(cat(mean_c x, max_c x))) as a CBGated whose gate branch
    is CBChannelReduce2d(('mean', 'max')) -> 7x7 convolution 2 -> 1 (general geometry)."""
    torch.manual_seed(97)
    body = pkg.convert(nn.Sequential(nn.Conv2d(8, 8, 3, padding=1)).eval().cuda().to(tdt), threshold=0.0)
    conv = pkg.convert(nn.Sequential(nn.Conv2d(2, 1, 7, padding=3)).eval().cuda().to(tdt), threshold=0.0,
                       generalGeometry=True)[0]
    assert type(conv).__name__ == 'CBConv2d' and conv.copyInput      # (it reads a state that is handed out)
    gate = nn.Sequential(pkg.CBChannelReduce2d(('mean', 'max')), conv)
    net = nn.Sequential()
    net.add_module('att', pkg.CBGated(body, gate))
    return exact(net, tdt)


def set_clone(net, cloneOutput):
    for m in net.modules():
        if hasattr(m, 'cloneOutput'):
            m.cloneOutput = cloneOutput
    return net


def tensor_of(y):
    return y[1] if type(y) == tuple else y


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
def test_segmentation_head_labels_are_the_argmax_of_the_producers_state(pkg, lib, dtype, monkeypatch):
    """conv 3x3 -> conv 1x1 -> CBChannelReduce2d('argmax', labelChanges=True), six frames of moving blocks, against a
    deep copy whose last module is the twin applied densely: the label map equals it and torch.argmax of the producer's
    state on every frame; one cbinfer_cbchancollapse_forward per frame; the handed-on mask is the listed pixels whose
    label moved, a subset of the frame's mask; after the first frame less than half of the pixels are listed."""
    import cbinfer_amd.chanreduce as chmod
    tdt = torch.float32 if dtype == np.float32 else torch.float16
    net = segmentation_head(pkg, tdt)
    dense = copy.deepcopy(net)
    dense.label = DenseTwin(net.label)
    spy = LayerSpy(lib.C)
    monkeypatch.setattr(chmod, 'C', spy)
    share = []
    with torch.no_grad():
        prev = None
        for t, f in enumerate(chain_frames(np.random.default_rng(19), 6, dtype)):
            tag, y, ix = net(f)
            yd = dense(f)
            assert y.dtype == torch.int64 and tuple(y.shape) == (1, 1, 20, 70) and torch.equal(y, yd), t
            scores = net.head.prevOutput
            assert torch.equal(net.label.outputState, torch.argmax(scores.cpu(), 1, keepdim=True).cuda()), t
            assert torch.equal(raw(scores), raw(dense.head.prevOutput)), t
            listed = np.unpackbits(host_words(net.label._chWork['copy']).view(np.uint8), bitorder='little')
            moved = np.unpackbits(host_words(ix._mask).view(np.uint8), bitorder='little')
            assert not (moved & ~listed).any(), t
            now = y[0, 0].cpu().numpy()
            if prev is not None:
                assert np.array_equal(host_words(ix._mask), cc.pack(now != prev)), t
                assert np.array_equal(ix.tensor().cpu().numpy(), np.flatnonzero((now != prev).reshape(-1))), t
            share.append(float(listed.sum()) / (20 * 70))
            prev = now
    assert share[0] == 1.0 and 0 < min(share[1:]) and max(share[1:]) < 0.5, share
    assert spy.calls == {None: {'cbinfer_cbchancollapse_forward': 6}}


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
def test_spatial_attention_equals_the_chain_with_the_dense_twin(pkg, lib, dtype, monkeypatch):
    """CBGated(body, gate = CBChannelReduce2d(('mean', 'max')) -> 7x7 convolution 2 -> 1) over six frames against a deep
    copy whose channel pooling is the twin applied densely: bit for bit in the output and in every state; the pooled map
    is the twin of the block's input; one cbinfer_cbchancollapse_forward per frame."""
    import cbinfer_amd.chanreduce as chmod
    tdt = torch.float32 if dtype == np.float32 else torch.float16
    net = attention_block(pkg, tdt)
    dense = copy.deepcopy(net)
    dense.att.gate._modules['0'] = DenseTwin(net.att.gate[0])
    spy = LayerSpy(lib.C)
    monkeypatch.setattr(chmod, 'C', spy)
    with torch.no_grad():
        for t, f in enumerate(chain_frames(np.random.default_rng(21), 6, dtype)):
            y, yd = tensor_of(net(f)), tensor_of(dense(f))
            assert tuple(y.shape) == (1, 8, 20, 70) and torch.equal(raw(y), raw(yd)), t
            pooled = net.att.gate[0].outputState
            assert tuple(pooled.shape) == (1, 2, 20, 70) and state_equals(pooled, module_twin(net.att.gate[0], f[0].cpu().numpy())), t
            for a, b in ((net.att.gate[1], dense.att.gate[1]), (net.att.body[0], dense.att.body[0])):
                assert torch.equal(raw(a.prevOutput), raw(b.prevOutput)), t
    assert spy.calls == {None: {'cbinfer_cbchancollapse_forward': 6}}


@pytest.mark.parametrize("chain", ["segmentation", "attention"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
def test_chains_record_as_a_launch_program(pkg, lib, dtype, chain):
    """With cloneOutput=False both chains are library calls only: FrameProgram records them, the CBChannelReduce2d is ONE
    cbinfer_cbchancollapse_forward of the recorded frame, three replayed frames equal the eager network in outputs and
    states bit for bit."""
    tdt = torch.float32 if dtype == np.float32 else torch.float16
    net = set_clone(segmentation_head(pkg, tdt) if chain == "segmentation" else attention_block(pkg, tdt), False)
    frames = chain_frames(np.random.default_rng(23), 7, dtype)
    with torch.no_grad():
        for f in frames[:4]:
            net(f)
        eager = copy.deepcopy(net)
        prog = pkg.FrameProgram(net)
        for t, f in enumerate(frames[4:]):
            yp, ye = tensor_of(prog(f)), tensor_of(eager(f))
            assert torch.equal(raw(yp), raw(ye)), t
            for ta, tb in zip(pkg.getStateTensors(net), pkg.getStateTensors(eager)):
                assert torch.equal(ta, tb), t
        raws = [fn for fn, _ in prog.calls]
        assert raws.count(lib.C.cbinfer_cbchancollapse_forward.raw) == 1
        op = net.label if chain == "segmentation" else net.att.gate[0]
        assert any(t is op.outputState for t in pkg.getStateTensors(net))


def test_head_with_torchs_argmax_is_refused_by_frame_program(pkg, lib):
    """What the label map costs without the module: the same converted layers with torch.argmax behind them cannot be
    recorded."""
    torch.manual_seed(95)
    src = nn.Sequential(nn.Conv2d(8, 16, 3, padding=1), nn.Conv2d(16, 5, 1), ArgMax2d())
    net = set_clone(pkg.convert(src.eval().cuda(), threshold=0.0), False)
    frames = chain_frames(np.random.default_rng(29), 4, np.float32)
    with torch.no_grad():
        for f in frames[:3]:
            net(f)
        with pytest.raises(lib.CBinferError, match="torch operators.*argmax"):
            pkg.FrameProgram(net).record(frames[3])


def test_worst_figures_are_reported():
    """The worst err / bound of SUM / MEAN / NORM over the tests above: measurements, not bars (the bar is 1)."""
    for (name, dt), w in sorted(WORST.items()):
        print("%-5s %-8s worst err / bound = %.3f" % (name, dt, w))
    assert WORST
