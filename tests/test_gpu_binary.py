"""-m gpu tests of the change-based element-wise operators of two maps (CBBinary2d, CBGLU2d, CBGated, insertCBGating;
cb_binary.hip).  The reference has no such operator; the numpy twin of tests/binary_cases.py IS the
specification (tests/test_host_binary.py shows it equal to torch's CPU operators bit for bit):
  rule 1  the listed pixels: the union of the two operands' changes (an operand without change information lists every
          pixel, a constant operand none), padding bits never set;
  rule 2  the values: at listed pixels the twin's, bit for bit (NaNs by NaN-ness); the sigmoid gate within the derived
          bound of the float64 formula; every other pixel of the state keeps its bits;
  rule 3  the hand-on: the frame's union mask in maskCopy, the working mask zero, the list made from the mask ascending.
"""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import binary_cases as bc
from test_gpu_rearrange import net_frames
from optest import (bits_of, dev, dev_words, free_pixel, host_words, lib, operand_args,      # noqa: F401  (fixtures)
                    gpu_pkg as pkg, raw, stream)

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float16]
CHANGE_FORMS = ["mask", "list", "all"]
WORST = {}


def values(rng, shape, dtype, span=1.0, special=None, lim=None):
    """Normal values times span, cut to [-lim, lim]; one in sixteen from `special`."""
    v = rng.standard_normal(shape) * span
    v = (v if lim is None else np.clip(v, -lim, lim)).astype(dtype)
    if special is not None and len(special):
        pick = rng.random(shape) < 1.0 / 16
        v[pick] = special[rng.integers(0, len(special), int(pick.sum()))]
    return v


def plans(form, pairs):
    """(a's change form, b's change form or None, bChanges) of one operand form: every pair in `pairs` for a map or a
    one-channel map, plus a constant one; a's forms with a constant and with a per-frame channel vector / scalar; a's
    forms for the halves."""
    aforms = sorted({fa for fa, _ in pairs}, key=CHANGE_FORMS.index)
    if form in ('map', 'pixel'):
        return [(fa, fb, 'own') for fa, fb in pairs] + [(fa, None, 'none') for fa in aforms]
    if form == 'halves':
        return [(fa, None, 'none') for fa in aforms]
    return [(fa, None, chg) for fa in aforms for chg in ('none', 'own')]


NINE = [(fa, fb) for fa in CHANGE_FORMS for fb in CHANGE_FORMS]
THREE = [("mask", "mask"), ("list", "list"), ("all", "all")]
SPECIAL = [0.0, -0.0, np.inf, -np.inf, np.nan, 6.0e-8, -3.0e-5, 3.0, -3.0, 65504.0]


def run_frames(lib, shape, dtype, form, fn, plan, rng, check, span=1.0, special=SPECIAL, bspan=None, bspecial=None,
               lim=None, blim=None):
    """cbinfer_cbbinary_forward over a first frame and the frame sets of tests/test_gpu_add.py.  After every frame:
    check(a, b, out, listed, where) judges the listed pixels; the state keeps its bits elsewhere -- also where an operand
    was altered at a pixel in neither list --; maskCopy is the numpy union, `bits` is zero, the compacted list ascending
    with the right count.  Returns the number of frames in which the dense result would have differed at the altered
    unlisted pixel."""
    C, ptr = lib.C, lib.ptr
    op, gate, reverse = fn
    fa, fb, chg = plan
    Cn, H, W = shape
    Ca = 2 * Cn if form == 'halves' else Cn
    special = np.array(special, dtype=dtype)
    bspecial = special if bspecial is None else np.array(bspecial, dtype=dtype)
    bspan = span if bspan is None else bspan
    bshape = bc.b_shape(form, Cn, H, W)
    bPixels = form in ('map', 'pixel')

    def a_values(n):
        """[Ca, n] values of a; in halves form the upper half is the second operand and takes its range."""
        if form != 'halves':
            return values(rng, (Ca, n), dtype, span, special, lim)
        return np.concatenate([values(rng, (Cn, n), dtype, span, special, lim),
                               values(rng, (Cn, n), dtype, bspan, bspecial, blim)])
    a = a_values(H * W).reshape(Ca, H, W)
    b = None if bshape is None else values(rng, bshape, dtype, bspan, bspecial, blim)
    da, db = dev(a), dev(b)
    dout = torch.empty((Cn, H, W), dtype=da.dtype, device="cuda")
    raw(dout).fill_(0x5BCD)
    words = C.cbinfer_mask_words(H, W)
    bits = torch.zeros(words, dtype=torch.int64, device="cuda")
    mcopy = torch.full((words,), -1, dtype=torch.int64, device="cuda")
    code = (lib.BIN_ADD, lib.BIN_SUB, lib.BIN_MUL, lib.BIN_MAXIMUM, lib.BIN_MINIMUM)[bc.OPS.index(op)]
    gcode = bc.GATES.index(gate)
    fcode = bc.FORMS.index(form)
    ccode = lib.BIN_B_OWN if chg == 'own' else lib.BIN_B_NONE
    dt = lib.CB_F32 if dtype == np.float32 else lib.CB_F16

    def call(argsA, argsB):
        (ma, la, ca, na), (mb, lb, cb, nb) = argsA, argsB
        st = C.cbinfer_cbbinary_forward(ptr(da), ptr(db), ptr(dout), ptr(ma), ptr(la), ca, ptr(na), ptr(mb), ptr(lb), cb,
                                        ptr(nb), fcode, ccode, ptr(bits), ptr(mcopy), Cn, H, W, code, gcode, int(reverse),
                                        dt, stream())
        assert st == 0, (st, shape, form, fn, plan)
    none = (None, None, 0, None)
    everything = np.ones((H, W), dtype=bool)
    # the first frame: no change information, the state is written completely (a constant b contributes nothing)
    call(none, none)
    out = dout.cpu().numpy()
    check(a, b, out, everything, (shape, dtype, form, fn, plan, "first frame"))
    assert np.array_equal(host_words(mcopy), bc.pack(everything))
    assert int(bits.ne(0).sum().item()) == 0
    saw = 0
    # (two operands, two lists, a first frame without either: this loop stays here -- optest.walk_frames walks one
    # operand -- and takes the operand forms from optest)
    for t, (label, SA, SB) in enumerate(bc.frame_sets(rng, H, W)):
        where = (shape, dtype, form, fn, plan, label)
        prev = out
        if SA.any():
            a[:, SA] = a_values(int(SA.sum()))
        ownPixels = chg == 'own' and bPixels
        if ownPixels and SB.any():
            b[:, SB] = values(rng, (b.shape[0], int(SB.sum())), dtype, bspan, bspecial, blim)
        if chg == 'own' and not bPixels:
            b[...] = values(rng, b.shape, dtype, bspan, bspecial, blim)      # a per-frame vector / scalar: every pixel
        union = SA | SB if ownPixels else SA
        # an operand altered where NEITHER list says so: a dense operator would pick it up
        p = free_pixel(union, middle=True)
        if p is not None:
            tgt = b if (ownPixels and t % 2) else a
            v = tgt[:, p // W, p % W]
            with np.errstate(invalid='ignore'):      # (another value of the same range)
                tgt[:, p // W, p % W] = np.where(np.abs(v) < 1, v + dtype(3.0), v * dtype(0.5))
        allB = chg == 'own' and (fb == 'all' or not bPixels)
        listed = everything if (fa == 'all' or allB) else union
        da.copy_(dev(a))
        if db is not None:
            db.copy_(dev(b))
        argsA = operand_args(fa, SA, 0, use_count=True)
        argsB = operand_args(fb, SB, H * W - 1, use_count=False) if ownPixels else none
        call(argsA, argsB)
        out = dout.cpu().numpy()
        check(a, b, out, listed, where)
        assert np.array_equal(bits_of(out)[:, ~listed], bits_of(prev)[:, ~listed]), where
        if p is not None and not listed.all():
            assert not listed[p // W, p % W]
            ref = bc.twin(a, b, form, op, gate, reverse)
            saw += int(not np.array_equal(bits_of(ref)[:, p // W, p % W], bits_of(prev)[:, p // W, p % W]))
        assert np.array_equal(host_words(mcopy), bc.pack(listed)), where
        assert int(bits.ne(0).sum().item()) == 0, where
        lst = torch.full((H * W,), -1, dtype=torch.int32, device="cuda")
        cnt = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        assert C.cbinfer_compact_bits(ptr(mcopy), W, H, ptr(lst), ptr(cnt), None, None, stream()) == 0
        n = int(cnt.item())
        assert n == int(listed.sum()), where
        assert np.array_equal(lst[:n].cpu().numpy(), np.flatnonzero(listed.reshape(-1))), where
    return saw


def exact_check(form, fn):
    op, gate, reverse = fn

    def check(a, b, out, listed, where):
        ref = bc.twin(a, b, form, op, gate, reverse)
        assert bc.same_bits(out[:, listed], ref[:, listed]), where
    return check


def ids_shape(s):
    return "%dx%dx%d" % s


# ------------------------------------------------------------------------------------------------ 1, 2: exact functions
@pytest.mark.parametrize("form", bc.FORMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
@pytest.mark.parametrize("shape", bc.SMALL, ids=ids_shape)
def test_every_exact_op_and_operand_form_through_the_c_abi(lib, shape, dtype, form):
    """Every op (reverse for sub), all nine pairs of change forms for a map and a one-channel map, a's three forms with a
    constant and with a per-frame channel vector / scalar, a's three forms for the halves: the twin bit for bit."""
    if shape == bc.STRIDED:
        assert lib.C.cbinfer_mask_words(shape[1], shape[2]) > 8 * torch.cuda.get_device_properties(0).multi_processor_count
    rng = np.random.default_rng(11)
    saw = 0
    for op, reverse in bc.EXACT:
        fn = (op, None, reverse)
        for plan in plans(form, NINE):
            saw += run_frames(lib, shape, dtype, form, fn, plan, rng, exact_check(form, fn))
    assert saw > 0 or shape[1] * shape[2] < 16


@pytest.mark.parametrize("form", bc.FORMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
@pytest.mark.parametrize("shape", bc.LARGE, ids=ids_shape)
def test_mul_and_sub_at_the_large_shapes(lib, shape, dtype, form):
    """n C above 256 (several rounds of the item loop) and more mask words than workgroups (the grid-stride leg): mul and
    sub in mask / mask, list / list and all forms."""
    if shape == bc.STRIDED:
        assert lib.C.cbinfer_mask_words(shape[1], shape[2]) > 8 * torch.cuda.get_device_properties(0).multi_processor_count
    rng = np.random.default_rng(12)
    saw = 0
    for fn in (('mul', None, False), ('sub', None, False), ('sub', None, True)):
        for plan in plans(form, THREE):
            saw += run_frames(lib, shape, dtype, form, fn, plan, rng, exact_check(form, fn))
    assert saw > 0


@pytest.mark.parametrize("form", ['map', 'pixel', 'halves'])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
@pytest.mark.parametrize("shape", bc.SHAPES, ids=ids_shape)
def test_hardsigmoid_gate_is_the_twin_bit_for_bit(lib, shape, dtype, form):
    """out = a * hardsigmoid(b), the gate rounded to the operand dtype first: gate inputs on both sides of the clamp and
    on its corners."""
    rng = np.random.default_rng(13)
    fn = ('mul', 'hardsigmoid', False)
    for plan in plans(form, NINE if shape in bc.SMALL else THREE):
        run_frames(lib, shape, dtype, form, fn, plan, rng, exact_check(form, fn), span=3.0)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
def test_the_mask_driven_launch_alone(lib, dtype):
    """cbinfer_binary_changed: the kernel ORs the working mask it is given (what an operand in list form left there),
    a's mask and b's mask itself; the twin at the union, the bits of `out` kept elsewhere, the working mask zero
    afterwards.  A one-channel hard-sigmoid gate, a reversed map difference, a maximum with a channel vector."""
    C, ptr = lib.C, lib.ptr
    Cn, H, W = 6, 3, 70
    rng = np.random.default_rng(37)
    inBits, SA, SB = (rng.random((H, W)) < 0.15 for _ in range(3))
    inBits[2, 69] = True
    dt = lib.CB_F32 if dtype == np.float32 else lib.CB_F16
    words = C.cbinfer_mask_words(H, W)
    for form, op, gate, reverse in (('pixel', 'mul', 'hardsigmoid', False), ('map', 'sub', None, True),
                                    ('channel', 'maximum', None, False)):
        a = values(rng, (Cn, H, W), dtype, 3.0, np.array(SPECIAL, dtype=dtype))
        b = values(rng, bc.b_shape(form, Cn, H, W), dtype, 3.0, np.array(SPECIAL, dtype=dtype))
        own = form != 'channel'
        listed = inBits | SA | (SB if own else False)
        da, db = dev(a), dev(b)
        dout = torch.zeros((Cn, H, W), dtype=da.dtype, device="cuda")
        bits, mcopy = dev_words(bc.pack(inBits)), torch.full((words,), -1, dtype=torch.int64, device="cuda")
        ma, mb = dev_words(bc.pack(SA)), dev_words(bc.pack(SB)) if own else None
        code = (lib.BIN_ADD, lib.BIN_SUB, lib.BIN_MUL, lib.BIN_MAXIMUM, lib.BIN_MINIMUM)[bc.OPS.index(op)]
        st = C.cbinfer_binary_changed(ptr(da), ptr(db), ptr(dout), ptr(ma), 0, ptr(mb), 0, ptr(bits), ptr(mcopy), Cn, H, W,
                                      bc.FORMS.index(form), code, bc.GATES.index(gate), int(reverse), dt, stream())
        assert st == 0
        out = dout.cpu().numpy()
        ref = bc.twin(a, b, form, op, gate, reverse)
        assert bc.same_bits(out[:, listed], ref[:, listed]), (form, op)
        assert not bits_of(out)[:, ~listed].any(), (form, op)
        assert int(bits.ne(0).sum().item()) == 0 and np.array_equal(host_words(mcopy), bc.pack(listed)), (form, op)


# ------------------------------------------------------------------------------------------------ 3: the sigmoid gate
def sigmoid_check(a, g, got, where, key):
    """got against a / (1 + exp(-g)) in float64; a, g, got arrays of one shape.  See the docstring of
    test_sigmoid_gate_against_float64 for the bound."""
    with np.errstate(all='ignore'):
        ref = a.astype(np.float64) / (1.0 + np.exp(-g.astype(np.float64)))
    got64 = got.astype(np.float64)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isnan(got64), np.isnan(ref)), where
    assert np.array_equal(got64[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)]), where
    err, mag = np.abs(got64[fin] - ref[fin]), np.abs(ref[fin])
    bound = 15.0 * 2.0 ** -24 * mag + 2.0 ** -126
    if a.dtype == np.float16:
        bound = bound + 2.0 * 2.0 ** -11 * mag + 2.0 ** -24
    big = mag >= 2.0 ** -14      # (relative figures where an f16 result is a normal number too)
    if big.any():
        WORST[key] = max(WORST.get(key, 0.0), float((err[big] / mag[big]).max()))
    bad = err > bound
    assert not bad.any(), (where, int(bad.sum()), a[fin][bad][:4], g[fin][bad][:4], got64[fin][bad][:4], ref[fin][bad][:4],
                           float((err / bound).max()))


def broadcast_b(a, b, form):
    """(a's lower part, b broadcast over it) as arrays of one shape."""
    if form == 'halves':
        return a[:a.shape[0] // 2], a[a.shape[0] // 2:]
    if form == 'channel':
        b = b.reshape(-1, 1, 1)
    elif form == 'scalar':
        b = b.reshape(1, 1, 1)
    return a, np.broadcast_to(b, a.shape)


@pytest.mark.parametrize("form", bc.FORMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
def test_sigmoid_gate_against_float64(lib, dtype, form):
    """out = a * sigmoid(b) against a / (1 + exp(-b)) in float64, every shape, the plans of the large shapes:
        fp32   |err| <= 15 * 2^-24 |ref| + 2^-126
        fp16   plus 2 * 2^-11 |ref| + 2^-24.
    Units of 2^-24 = half an ulp of a float32 result, what one correctly rounded operation adds.  The sigmoid
    1 / (1 + expf(-v)) is CBPointwise2d's, whose 14 units tests/test_gpu_pointwise.py derives (OpenCL full profile: expf 3
    ulp, taken twice, an ulp two units: 12; the addition 1; the division 1); the product adds 1 unit: 15.  In fp16 the
    gate value is rounded to f16 before the product and the product once more: two roundings of 2^-11 each (their
    product, 2^-22 |ref|, lies inside the doubled expf limit), and 2^-24, the smallest f16 subnormal, for a result below
    the normal range.  Gate inputs in [-8, 8] with the ends, so that the f16 gate value is a normal number
    (sigmoid(-8) = 3.4e-4 > 2^-14); a in [-20, 20] plus +-inf and NaN: where the reference is not finite the result must
    be the same infinity or a NaN.  The constants are not tuned: a failure is a finding.  The worst err / |ref| seen is
    printed and reported in DESIGN 5.25."""
    rng = np.random.default_rng(17)
    fn = ('mul', 'sigmoid', False)
    key = (form, np.dtype(dtype).name)

    def check(a, b, out, listed, where):
        al, bl = broadcast_b(a, b, form)
        sigmoid_check(al[:, listed], bl[:, listed], out[:, listed], where, key)
    for shape in bc.SHAPES:
        for plan in plans(form, THREE):
            # (a: normal values times 7 cut to +-20;  b: times 3 cut to +-8, which puts the ends among the values)
            run_frames(lib, shape, dtype, form, fn, plan, rng, check, span=7.0,
                       special=[np.inf, -np.inf, np.nan, 20.0, -20.0, 0.0, -0.0], bspan=3.0, bspecial=[8.0, -8.0, 0.0, -0.0],
                       lim=20.0, blim=8.0)
    if key in WORST:
        print("sigmoid gate %s %s: worst err / |ref| = %.3g = %.2f x 2^-24" % (key + (WORST[key], WORST[key] * 2.0 ** 24)))


# ------------------------------------------------------------------------------------------------ 4: form independence
@pytest.mark.parametrize("form,shape", list(zip(bc.FORMS, [(3, 5, 64), (300, 5, 130), (6, 1, 65), (1, 1, 9), (2, 2100, 9)])),
                         ids=bc.FORMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
def test_the_state_does_not_depend_on_the_change_forms(lib, dtype, form, shape):
    """The same frames with the operands' changes as masks, as lists and as all-with-unchanged-values: the states are
    bit-identical after every frame, for every function, the gates included."""
    C, ptr = lib.C, lib.ptr
    Cn, H, W = shape
    Ca = 2 * Cn if form == 'halves' else Cn
    bshape = bc.b_shape(form, Cn, H, W)
    own = form in ('map', 'pixel')
    words = C.cbinfer_mask_words(H, W)
    dt = lib.CB_F32 if dtype == np.float32 else lib.CB_F16
    for op, gate, reverse in [(o, None, r) for o, r in bc.EXACT] + [('mul', 'sigmoid', False), ('mul', 'hardsigmoid', False)]:
        code = (lib.BIN_ADD, lib.BIN_SUB, lib.BIN_MUL, lib.BIN_MAXIMUM, lib.BIN_MINIMUM)[bc.OPS.index(op)]
        states = []
        for cf in CHANGE_FORMS:
            rng = np.random.default_rng(19)      # (the same frames for every change form)
            a = values(rng, (Ca, H, W), dtype, 3.0, np.array(SPECIAL[:4] + SPECIAL[5:], dtype=dtype))
            b = None if bshape is None else values(rng, bshape, dtype, 3.0)
            da, db = dev(a), dev(b)
            dout = torch.zeros((Cn, H, W), dtype=da.dtype, device="cuda")
            bits = torch.zeros(words, dtype=torch.int64, device="cuda")
            mcopy = torch.zeros(words, dtype=torch.int64, device="cuda")
            seen = []
            none = (None, None, 0, None)
            for t, (label, SA, SB) in enumerate([("first", None, None)] + bc.frame_sets(rng, H, W)):
                if t:
                    if SA.any():
                        a[:, SA] = values(rng, (Ca, int(SA.sum())), dtype, 3.0)
                    if own and SB.any():
                        b[:, SB] = values(rng, (b.shape[0], int(SB.sum())), dtype, 3.0)
                    da.copy_(dev(a))
                    if db is not None:
                        db.copy_(dev(b))
                (ma, la, ca, na) = none if not t else operand_args(cf, SA, 0, use_count=True)
                (mb, lb, cb, nb) = none if not (t and own) else operand_args(cf, SB, H * W - 1, use_count=False)
                st = C.cbinfer_cbbinary_forward(ptr(da), ptr(db), ptr(dout), ptr(ma), ptr(la), ca, ptr(na), ptr(mb), ptr(lb),
                                                cb, ptr(nb), bc.FORMS.index(form), lib.BIN_B_OWN if own else lib.BIN_B_NONE,
                                                ptr(bits), ptr(mcopy), Cn, H, W, code, bc.GATES.index(gate), int(reverse), dt,
                                                stream())
                assert st == 0
                seen.append(raw(dout).clone())
            states.append(seen)
        for cf, seen in zip(CHANGE_FORMS[1:], states[1:]):
            for t, (x, y) in enumerate(zip(states[0], seen)):
                assert torch.equal(x, y), (form, op, gate, reverse, cf, t)


# ------------------------------------------------------------------------------------------------ 5: modules
def same(x, y):
    return torch.equal(raw(x.contiguous()), raw(y.contiguous()))


def refresh(t, changed, rng, span=1.0):
    """New values at the changed pixels of every channel."""
    if changed.any():
        sel = torch.from_numpy(changed).cuda()
        n = int(changed.sum())
        t[0][:, sel] = torch.from_numpy(rng.standard_normal((t.size(1), n)) * span).to(t.dtype).cuda()


def mask_indexes(changed):
    from cbinfer_amd.conv2d_cg import MaskChangeIndexes
    H, W = changed.shape
    return MaskChangeIndexes(dev_words(bc.pack(changed)), (H, W), torch.empty(H * W, dtype=torch.int32, device="cuda"),
                             torch.zeros(1, dtype=torch.int32, device="cuda"))


def list_indexes(changed):
    return torch.from_numpy(np.flatnonzero(changed.reshape(-1)).astype(np.int32)).cuda()


def module_sigmoid_check(state, a, g, where):
    """The module's state against the float64 formula of its device operands (the bound of the sigmoid test)."""
    a, g = torch.broadcast_tensors(a, g)
    sigmoid_check(a.cpu().numpy(), g.cpu().numpy(), state.cpu().numpy(), where, ("module", str(state.dtype)))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_binary_module_two_operands(pkg, lib, dtype):
    """CBBinary2d(a, b) with b a map, a one-channel map and a per-frame channel vector against the dense torch
    expression on the same device tensors over several frames: exact ops by bits, the sigmoid gate by its bound, the
    hard-sigmoid gate against torch's CPU operator (which the twin equals bit for bit; the device operator multiplies by
    a rounded 1 / 6).  The union is handed on as a MaskChangeIndexes; a new state is written completely."""
    Cn, H, W = 6, 7, 70
    rng = np.random.default_rng(23)
    dense = {'add': torch.add, 'sub': torch.sub, 'mul': torch.mul, 'maximum': torch.maximum, 'minimum': torch.minimum}
    fns = [(op, None, r) for op, r in bc.EXACT] + [('mul', 'sigmoid', False), ('mul', 'hardsigmoid', False)]
    for bshape in ((1, Cn, H, W), (1, 1, H, W), (1, Cn, 1, 1)):
        for op, gate, reverse in fns:
            m = pkg.CBBinary2d(op, gate=gate, reverse=reverse)
            m.propChangeIndexes = True
            a = torch.from_numpy(rng.standard_normal((1, Cn, H, W))).to(dtype).cuda()
            b = torch.from_numpy(rng.standard_normal(bshape)).to(dtype).cuda()

            def judge(where):
                if gate == 'sigmoid':
                    return module_sigmoid_check(m.outputState, a, b, where)
                if gate == 'hardsigmoid':
                    want = (a.cpu() * F.hardsigmoid(b.cpu())).cuda()
                else:
                    want = dense[op](b, a) if reverse else dense[op](a, b)
                assert same(m.outputState, want), where
            tag, y, ix = m(a, b)      # first frame: bare tensors
            judge((bshape, op, gate, "first"))
            assert tag == 'changeIndexes' and y is not m.outputState and same(y, m.outputState)
            assert np.array_equal(host_words(ix._mask), bc.pack(np.ones((H, W), dtype=bool)))
            for t in range(4):
                prev = m.outputState.clone()
                SA, SB = rng.random((H, W)) < 0.1, rng.random((H, W)) < 0.1
                if t == 3:
                    SA[:], SB[:] = False, False
                refresh(a, SA, rng)
                if bshape[2] == 1:      # a per-frame channel vector: bare, every pixel
                    b = torch.from_numpy(rng.standard_normal(bshape)).to(dtype).cuda()
                    listed = np.ones((H, W), dtype=bool)
                    argB = b
                else:
                    refresh(b, SB, rng)
                    listed = SA | SB
                    argB = ('changeIndexes', b, list_indexes(SB) if t % 2 else mask_indexes(SB))
                keep = a[0, :, 6, 69].clone()
                a[0, :, 6, 69] += 1.0      # (listed by neither operand in frame 3)
                tag, y, ix = m(('changeIndexes', a, mask_indexes(SA) if t % 2 else list_indexes(SA)), argB)
                sel = torch.from_numpy(listed).cuda()
                if not listed.all():
                    assert torch.equal(raw(m.outputState)[0][:, ~sel], raw(prev)[0][:, ~sel]), (bshape, op, t)
                    if not listed[6, 69]:
                        a[0, :, 6, 69] = keep      # (there the state is the dense result of the value before)
                judge((bshape, op, gate, t))
                assert np.array_equal(host_words(ix._mask), bc.pack(listed)), (bshape, op, t)
                assert np.array_equal(ix.tensor().cpu().numpy(), np.flatnonzero(listed.reshape(-1)))
                assert int(m._binWork['bits'].ne(0).sum()) == 0
    # a state of a new size or dtype is rebuilt and written completely, whatever the lists say
    m = pkg.CBBinary2d('sub')
    m.cloneOutput = False
    empty = torch.zeros(0, dtype=torch.int32, device="cuda")
    for shape, dt in (((1, 4, 5, 9), dtype), ((1, 4, 6, 9), dtype), ((1, 4, 6, 9), torch.float16 if dtype == torch.float32 else torch.float32)):
        a = torch.from_numpy(rng.standard_normal(shape)).to(dt).cuda()
        b = torch.from_numpy(rng.standard_normal(shape)).to(dt).cuda()
        out = m(('changeIndexes', a, empty), ('changeIndexes', b, empty))
        assert out is m.outputState and out._cbinfer_inplace_state and same(out, a - b) and out.dtype == dt
    # clearMemory
    net = nn.Sequential(m)
    pkg.clearMemory(net)
    assert m.outputState.numel() == 0 and m._binWork is None
    assert same(m(a, b), a - b)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_binary_module_constants_of_every_shape(pkg, lib, dtype):
    """CBBinary2d(op, other=...) for every constant shape and a Python number: the dense torch expression on the same
    device tensors, bit for bit; only a's changes count; the buffer follows .to() / .half()."""
    Cn, H, W = 4, 5, 67
    rng = np.random.default_rng(29)
    cases = [('mul', (1, Cn, H, W), False), ('add', (1, 1, H, W), False), ('mul', (1, Cn, 1, 1), False),
             ('sub', (Cn, 1, 1), True), ('maximum', (Cn,), False), ('minimum', (1,), False), ('sub', (), False)]
    dense = {'add': torch.add, 'sub': torch.sub, 'mul': torch.mul, 'maximum': torch.maximum, 'minimum': torch.minimum}
    for op, shape, reverse in cases + [('mul', 0.3, False), ('sub', 1, True)]:
        if isinstance(shape, tuple):
            src = torch.from_numpy(np.asarray(rng.standard_normal(shape))).float()
            m = pkg.CBBinary2d(op, other=src, reverse=reverse).cuda()
            m = m.half() if dtype == torch.float16 else m
            other = src.to(dtype).cuda()
            assert m.other.dtype == dtype and m.other.is_cuda and same(m.other, other)
            if len(shape) in (1, 3) and shape != (1,):
                other = other.reshape(1, Cn, 1, 1)
        else:
            m = pkg.CBBinary2d(op, other=shape, reverse=reverse)
            other = torch.tensor(shape, dtype=dtype).cuda()      # (converted once to the operand's dtype)
        m.propChangeIndexes = True
        a = torch.from_numpy(rng.standard_normal((1, Cn, H, W))).to(dtype).cuda()
        for t in range(4):
            prev = m.outputState.clone() if t else None
            SA = rng.random((H, W)) < 0.15
            refresh(a, SA, rng)
            listed = SA if t else np.ones((H, W), dtype=bool)
            if t:
                keep = a[0, :, 4, 66].clone()
                a[0, :, 4, 66] += 1.0
            tag, y, ix = m(('changeIndexes', a, mask_indexes(SA) if t % 2 else list_indexes(SA)))
            sel = torch.from_numpy(listed).cuda()
            if t:
                assert torch.equal(raw(m.outputState)[0][:, ~sel], raw(prev)[0][:, ~sel]), (op, shape, t)
                if not listed[4, 66]:
                    a[0, :, 4, 66] = keep      # (there the state is the dense result of the value before)
            want = dense[op](other, a) if reverse else dense[op](a, other)
            assert same(m.outputState, want), (op, shape, t)
            assert np.array_equal(host_words(ix._mask), bc.pack(listed)), (op, shape, t)
    # a buffer of another dtype than the operand's is refused with both named
    m = pkg.CBBinary2d('mul', other=torch.ones(Cn)).cuda()
    with pytest.raises(lib.CBinferError, match="operand a is torch.float16 on cuda:0, the constant operand `other` "
                                               "torch.float32 on cuda:0"):
        m(a.half())


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_glu_module_and_its_hand_on(pkg, lib, dtype):
    """CBGLU2d against x[:, :C] / (1 + exp(-x[:, C:])) in float64 by the sigmoid bound (and within two roundings of
    torch's own F.glu on the device), over frames with a's change list; an odd channel count is refused."""
    Cn, H, W = 6, 5, 70
    rng = np.random.default_rng(31)
    m = pkg.CBGLU2d(nn.GLU(1))
    m.propChangeIndexes = True
    x = torch.from_numpy(rng.standard_normal((1, 2 * Cn, H, W)) * 1.5).to(dtype).cuda()
    for t in range(5):
        prev = m.outputState.clone() if t else None
        S = rng.random((H, W)) < 0.1
        refresh(x, S, rng, 1.5)
        listed = S if t else np.ones((H, W), dtype=bool)
        tag, y, ix = m(('changeIndexes', x, mask_indexes(S) if t % 2 else list_indexes(S)))
        assert tuple(m.outputState.shape) == (1, Cn, H, W) and same(y, m.outputState)
        module_sigmoid_check(m.outputState, x[:, :Cn], x[:, Cn:], ("glu", dtype, t))
        if t:
            sel = torch.from_numpy(listed).cuda()
            assert torch.equal(raw(m.outputState)[0][:, ~sel], raw(prev)[0][:, ~sel])
        assert np.array_equal(host_words(ix._mask), bc.pack(listed))
    with pytest.raises(lib.CBinferError, match="odd number of channels"):
        m(x[:, :5])
    net = nn.Sequential(m)
    assert len(pkg.getStateTensors(net)) == 1
    pkg.clearMemory(net)
    assert m.outputState.numel() == 0 and m._binWork is None


# ------------------------------------------------------------------------------------------------ 6: chains
def exact_f32(pkg, net):
    for m in net.modules():
        if type(m) is pkg.CBConv2d:
            m.exactF32 = True


class Scale(nn.Module):
    """torch's dense gamma[c] * x."""

    def __init__(self, gamma):
        super(Scale, self).__init__()
        self.register_buffer('gamma', gamma)

    def forward(self, x):
        return x * self.gamma


def test_layer_scale_hands_the_right_mask_to_a_1x1_layer(pkg, lib):
    """conv 3x3 -> CBBinary2d('mul', other=gamma[c]) -> conv 1x1, every threshold 0, against the same converted layers
    with torch's dense product in place: bit for bit over six frames in the output and the product's state -- the 1x1
    layer, which is handed the module's mask and skips its own detection, recomputes exactly what changed."""
    torch.manual_seed(53)
    src = nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), nn.Identity(), nn.Conv2d(8, 4, 1)).eval().cuda()
    net = pkg.convert(src, threshold=0.0)
    exact_f32(pkg, net)
    gamma = torch.randn(1, 8, 1, 1).cuda()
    dense = copy.deepcopy(net)
    dense._modules['1'] = Scale(gamma)
    net._modules['1'] = pkg.CBBinary2d('mul', other=gamma)
    net[0].propChangeIndexes = net[1].propChangeIndexes = True
    with torch.no_grad():
        for t, f in enumerate(net_frames(6, 61, 3, torch.float32)):
            y, want = net(f), dense(f)
            assert tuple(y.shape) == (1, 4, 24, 40) and same(y, want), t
            share = float(np.unpackbits(host_words(net[1]._binWork['copy']).view(np.uint8)).sum()) / (24 * 40)
            assert share == 1.0 if t == 0 else 0.0 < share < 0.6, (t, share)


def make_glu_chain(pkg):
    """conv 3x3 -> GLU over the channels -> conv 1x1 through convert + insertCBGating."""
    torch.manual_seed(57)
    src = nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), nn.GLU(1), nn.Conv2d(4, 4, 1)).eval().cuda()
    net = pkg.insertCBGating(pkg.convert(src, threshold=0.05), cloneOutput=False)
    assert [type(m).__name__ for m in net] == ['CBConv2d', 'CBGLU2d', 'CBConv2d']
    assert net[0].propChangeIndexes and net[1].propChangeIndexes and not net[1].cloneOutput
    return net


def make_attention(pkg):
    """A conv stem and a CBGated attention block: feat = conv 3x3 (stem), out = body(feat) * sigmoid(gate(feat)) with a
    one-channel gate map."""
    torch.manual_seed(59)
    parts = dict(stem=nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), nn.ReLU()),
                 body=nn.Sequential(nn.Conv2d(8, 8, 3, padding=1)), gate=nn.Sequential(nn.Conv2d(8, 1, 1)))
    cb = {k: pkg.convert(v.eval().cuda(), threshold=0.05) for k, v in parts.items()}
    net = nn.Sequential()
    net.add_module('stem', cb['stem'])
    net.add_module('att', pkg.CBGated(cb['body'], cb['gate']))
    net.att.mul.cloneOutput = False
    return net


@pytest.mark.parametrize("which", ["glu", "attention"])
def test_chains_record_as_a_launch_program(pkg, lib, which):
    """Both chains over frames: the operator's state is the float64 formula of its two operands within the sigmoid
    bound; with cloneOutput=False the network is library calls only, FrameProgram records it, and replays equal the eager
    network bit for bit in outputs and states; SequenceBatch and BranchGroup refuse the network by the layer's name."""
    net = make_glu_chain(pkg) if which == "glu" else make_attention(pkg)
    op = net[1] if which == "glu" else net.att.mul
    seen = []
    hook = op.register_forward_pre_hook(lambda mod, args: seen.append(args))
    frames = net_frames(10, 71, 3, torch.float32)
    with torch.no_grad():
        for t, f in enumerate(frames[:5]):
            y = net(f)
            args = [x[1] if type(x) == tuple else x for x in seen[-1]]
            if which == "glu":
                assert tuple(y.shape) == (1, 4, 24, 40)
                module_sigmoid_check(op.outputState, args[0][:, :4], args[0][:, 4:], (which, t))
            else:
                assert y is op.outputState and tuple(y.shape) == (1, 8, 24, 40) and tuple(args[1].shape) == (1, 1, 24, 40)
                module_sigmoid_check(op.outputState, args[0], args[1], (which, t))
            if t:      # behind the first frame the operands carry their changes
                assert all(type(x) == tuple for x in seen[-1])
        hook.remove()
        eager = copy.deepcopy(net)
        prog = pkg.FrameProgram(net)
        for t, f in enumerate(frames[5:]):
            yp, ye = prog(f), eager(f)
            assert same(yp, ye), (which, t)
            for ta, tb in zip(pkg.getStateTensors(net), pkg.getStateTensors(eager)):
                assert torch.equal(ta, tb), (which, t)
        raws = [fn for fn, _ in prog.calls]
        assert raws.count(lib.C.cbinfer_cbbinary_forward.raw) == 1
        assert any(t is op.outputState for t in pkg.getStateTensors(net))
    name = '1' if which == "glu" else 'att.mul'
    kind = 'CBGLU2d' if which == "glu" else 'CBBinary2d'
    with pytest.raises(lib.CBinferError, match=r"SequenceBatch: layer '%s' is %s \(.*element-wise operator of two maps" % (name, kind)):
        pkg.SequenceBatch(net, 2)
    with pytest.raises(lib.CBinferError, match=r"BranchGroup: layer '0.%s' is %s" % (name, kind)):
        pkg.BranchGroup([net])


def test_torch_gate_network_is_refused_by_frame_program(pkg, lib):
    """What the block costs without the module: the same layers with torch's product and sigmoid cannot be recorded."""
    net = make_attention(pkg)

    class TorchGate(nn.Module):
        def __init__(self, stem, body, gate):
            super(TorchGate, self).__init__()
            self.stem, self.body, self.gate = stem, body, gate

        def forward(self, x):
            x = self.stem(x)
            return self.body(x)[1] * torch.sigmoid(self.gate(x)[1])
    dense = TorchGate(net.stem, net.att.body, net.att.gate)
    frames = net_frames(3, 73, 3, torch.float32)
    with torch.no_grad():
        for f in frames:
            dense(f)
        with pytest.raises(lib.CBinferError, match=r"torch operators.*CBBinary2d / CBGated / CBGLU2d \(insertCBGating\)"):
            pkg.FrameProgram(dense).record(frames[-1])
