"""CPU-only tests of the change-based residual add: foldBatchNorm against the float64 formula, the flags
CBResidual's constructor sets, the argument checks of the C entry points, the refusals and pickling.  No kernel is
launched here."""
import copy
import pickle

import numpy as np
import pytest
import torch
import torch.nn as nn
from optest import lib, npdtype, pkg      # noqa: F401  (fixtures)


def _stats(bn, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(bn.num_features, generator=g))
        bn.running_var.copy_(torch.rand(bn.num_features, generator=g) * 2 + 0.05)
        if bn.affine:
            bn.weight.copy_(torch.randn(bn.num_features, generator=g))
            bn.bias.copy_(torch.randn(bn.num_features, generator=g))
    return bn


@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_fold_parameters_are_the_float64_formula_rounded_once(pkg, dtype, bias, affine):
    """w' = w gamma / sqrt(var + eps), b' = (b - mean) gamma / sqrt(var + eps) + beta, left to right in float64 (numpy
    here), one rounding to the module's dtype (numpy's float64 -> float16 is a single rounding; torch's is two)."""
    torch.manual_seed(3)
    npdtype = np.float32 if dtype == torch.float32 else np.float16
    conv = nn.Conv2d(5, 7, 3, stride=2, padding=1, bias=bias)
    bn = _stats(nn.BatchNorm2d(7, eps=1e-3, affine=affine), 4)
    seq = nn.Sequential(conv, bn, nn.ReLU()).to(dtype).eval()
    kept = {k: v.clone() for k, v in seq.state_dict().items()}
    assert pkg.foldBatchNorm(seq) is seq
    assert list(seq._modules) == ['0', '2'] and type(seq[0]) is nn.Conv2d and seq[0] is not conv
    f = seq[0]
    assert (f.stride, f.padding, f.kernel_size, f.in_channels, f.out_channels) == ((2, 2), (1, 1), (3, 3), 5, 7)
    assert f.weight.dtype == dtype and f.bias is not None and f.bias.dtype == dtype and not f.training
    # the source modules' parameters are not touched
    for k, v in list(conv.state_dict(prefix='0.').items()) + list(bn.state_dict(prefix='1.').items()):
        assert torch.equal(v, kept[k]), k
    d = np.sqrt(bn.running_var.numpy().astype(np.float64) + bn.eps)
    gamma = bn.weight.detach().numpy().astype(np.float64) if affine else np.ones(7)
    beta = bn.bias.detach().numpy().astype(np.float64) if affine else np.zeros(7)
    b = conv.bias.detach().numpy().astype(np.float64) if bias else np.zeros(7)
    w = conv.weight.detach().numpy().astype(np.float64)
    wf = (w * gamma[:, None, None, None] / d[:, None, None, None]).astype(npdtype)
    bf = ((b - bn.running_mean.numpy().astype(np.float64)) * gamma / d + beta).astype(npdtype)
    assert torch.equal(f.weight.detach(), torch.from_numpy(wf))
    assert torch.equal(f.bias.detach(), torch.from_numpy(bf))


def test_round_once_is_a_single_rounding():
    """float64 values that sit just beside a float16 tie: through float32 they round to the wrong neighbour."""
    from cbinfer_amd.residual import _round_once
    x = np.array([1.0 + 2.0 ** -11 + 2.0 ** -30, 1.0 + 2.0 ** -11 - 2.0 ** -30, -(1.0 + 3 * 2.0 ** -11 - 2.0 ** -40),
                  65519.99, 6e-8, -3e-8, 0.0, 1e-30, 70000.0, 0.1], dtype=np.float64)
    got = _round_once(torch.from_numpy(x), torch.float16).numpy()
    with np.errstate(over='ignore'):
        want = x.astype(np.float16)
    assert np.array_equal(got.view(np.uint16), want.view(np.uint16))
    assert not np.array_equal(torch.from_numpy(x).to(torch.float16).numpy().view(np.uint16), want.view(np.uint16))
    assert _round_once(torch.from_numpy(x), torch.float32).dtype == torch.float32


def test_folded_network_in_float64(pkg):
    """conv -> BN -> ReLU -> conv -> BN in float64: the folded network within 1e-10 max|out| (float64 rounding is 2e-16
    times a few hundred terms; the bar leaves three orders of margin)."""
    torch.manual_seed(5)
    net = nn.Sequential(nn.Conv2d(6, 9, 3, padding=1, bias=False), _stats(nn.BatchNorm2d(9), 6), nn.ReLU(),
                        nn.Sequential(nn.Conv2d(9, 4, 3, stride=2, padding=1), _stats(nn.BatchNorm2d(4, affine=False), 7))
                        ).double().eval()
    x = torch.randn(1, 6, 13, 17, dtype=torch.float64)
    with torch.no_grad():
        ref = net(x)
        folded = pkg.foldBatchNorm(copy.deepcopy(net))
        assert [type(m).__name__ for m in folded.modules()] == ['Sequential', 'Conv2d', 'ReLU', 'Sequential', 'Conv2d']
        out = folded(x)
    err, bar = float((out - ref).abs().max()), 1e-10 * float(ref.abs().max())
    print("folded vs conv->BN in float64: max |diff| %.3e, bar %.3e" % (err, bar))
    assert err <= bar


def test_fold_refusals(pkg, lib):
    seq = nn.Sequential(nn.Conv2d(3, 4, 3), nn.BatchNorm2d(4))      # (training mode)
    with pytest.raises(lib.CBinferError, match="training mode"):
        pkg.foldBatchNorm(seq)
    assert [type(m).__name__ for m in seq] == ['Conv2d', 'BatchNorm2d']
    seq = nn.Sequential(nn.Conv2d(3, 4, 3), nn.BatchNorm2d(4, track_running_stats=False)).eval()
    with pytest.raises(lib.CBinferError, match="running statistics"):
        pkg.foldBatchNorm(seq)
    # a batch norm that is not behind a convolution is left alone
    seq = nn.Sequential(nn.BatchNorm2d(3), nn.Conv2d(3, 4, 3), nn.ReLU(), nn.BatchNorm2d(4)).eval()
    assert [type(m).__name__ for m in pkg.foldBatchNorm(seq)] == ['BatchNorm2d', 'Conv2d', 'ReLU', 'BatchNorm2d']


def _block(pkg, tail=None):
    torch.manual_seed(9)
    body = nn.Sequential(nn.Conv2d(8, 8, 3, padding=1), nn.ReLU(), nn.Conv2d(8, 8, 3, padding=1)).eval()
    if tail is not None:
        body.add_module('tail', tail)
    return pkg.convert(body, threshold=0.05)


def test_residual_constructor_sets_the_flags(pkg):
    body = _block(pkg)
    body[0].copyInput = False
    short = pkg.convert(nn.Sequential(nn.Conv2d(8, 8, 1, stride=1, bias=False)).eval(), threshold=0.05,
                        generalGeometry=True)
    short[0].copyInput, short[0].feedbackLoop = False, True
    assert not body[1].propChangeIndexes and not short[0].propChangeIndexes
    res = pkg.CBResidual(body, short)
    assert type(res.body) is nn.Sequential and type(res.shortcut) is nn.Sequential and res.body is body
    assert type(res.add) is pkg.CBAdd2d and res.add.relu and not res.add.propChangeIndexes and res.add.cloneOutput
    assert body[1].propChangeIndexes and not body[0].propChangeIndexes and short[0].propChangeIndexes
    assert body[0].copyInput is True
    assert short[0].copyInput is False      # (feedback mode: the layer keeps no reference to its input)
    # the last module is not a CBConv2d: nobody could take the list
    body = _block(pkg, nn.Tanh())
    res = pkg.CBResidual(body, relu=False)
    assert res.shortcut is None and not res.add.relu and not any(m.propChangeIndexes for m in body if type(m) is pkg.CBConv2d)
    # a bare module and a list are wrapped
    assert type(pkg.CBResidual(body[0]).body) is nn.Sequential
    assert len(pkg.CBResidual([body[0], body[1]]).body) == 2
    # the state helpers reach the sum
    res.add.outputState = torch.ones(1, 8, 3, 3)
    res.add.__dict__['_addWork'] = {'key': None}
    net = nn.Sequential(res)
    assert any(t is res.add.outputState for t in pkg.getStateTensors(net))
    pkg.clearMemory(net)
    assert res.add.outputState.numel() == 0 and res.add._addWork is None
    assert pkg.CBAdd2d is pkg.residual.CBAdd2d and all(n in pkg.__all__ for n in ('CBAdd2d', 'CBResidual', 'foldBatchNorm'))


def test_add_operand_checks_and_pickle(pkg, lib):
    add = pkg.CBAdd2d(relu=True)
    add.propChangeIndexes, add.cloneOutput = True, False
    x = torch.zeros(1, 4, 5, 6)
    for a, b, what in ((x, torch.zeros(1, 4, 5, 7), "operands differ"), (x, x.half(), "operands differ"),
                       (torch.zeros(2, 4, 5, 6), torch.zeros(2, 4, 5, 6), r"\[1, C, H, W\]"),
                       (x, ('changeIndexes', x), "tuple"), (x, None, "must be a tensor"),
                       (x, x, "HIP devices only")):
        with pytest.raises(lib.CBinferError, match=what):
            add(a, b)
    add.__dict__['_addWork'] = {'key': None}
    c = pickle.loads(pickle.dumps(add))
    assert type(c) is pkg.CBAdd2d and (c.relu, c.propChangeIndexes, c.cloneOutput) == (True, True, False)
    assert c._addWork is None and c.outputState.numel() == 0 and repr(c) == repr(add)
    assert 'relu=True' in repr(c)


def test_c_entry_points_check_their_arguments(lib):
    """Bad arguments return CB_ERR_BADARG (-1) before anything is launched (the pointers here are never followed)."""
    C = lib.C
    assert C.cbinfer_abi_version() == 11
    A, B, O, BITS, COPY, M, L = (0x1000 * i for i in range(1, 8))

    def fwd(a=A, b=B, o=O, maskA=None, listA=None, capA=0, countA=None, maskB=None, listB=None, capB=0, countB=None,
            bits=BITS, cp=COPY, Cn=3, H=4, W=5, dt=lib.CB_F32):
        return C.cbinfer_cbadd_forward(a, b, o, maskA, listA, capA, countA, maskB, listB, capB, countB, bits, cp, Cn, H, W,
                                       1, dt, None)

    def chg(a=A, b=B, o=O, bits=BITS, cp=COPY, Cn=3, H=4, W=5, dt=lib.CB_F16, maskA=None):
        return C.cbinfer_add_changed(a, b, o, maskA, 0, None, 0, bits, cp, Cn, H, W, 0, dt, None)

    for call in (fwd, chg):
        for bad in (dict(a=None), dict(b=None), dict(o=None), dict(bits=None), dict(cp=None), dict(cp=BITS), dict(Cn=0),
                    dict(H=0), dict(W=-1), dict(dt=lib.CB_F32S), dict(dt=7), dict(H=1 << 16, W=1 << 15),
                    dict(Cn=1 << 25), dict(maskA=COPY), dict(maskA=BITS)):
            assert call(**bad) == -1, (call.__name__, bad)
    for bad in (dict(listA=L, capA=-1), dict(listB=L, capB=-1), dict(maskA=M, listA=L), dict(maskB=M, listB=L),
                dict(countA=L), dict(countB=L)):
        assert fwd(**bad) == -1, bad


def test_batch_and_branch_refusals_name_the_layer(pkg, lib):
    res = pkg.CBResidual(_block(pkg))
    net = nn.Sequential()
    net.add_module('stem', pkg.convert(nn.Sequential(nn.Conv2d(3, 8, 3, padding=1)).eval(), threshold=0.05)[0])
    net.add_module('block1', res)
    with pytest.raises(lib.CBinferError, match=r"SequenceBatch: layer 'block1.add' is CBAdd2d \(relu=True"):
        pkg.SequenceBatch(net, 2)
    with pytest.raises(lib.CBinferError, match=r"BranchGroup: layer '0.block1.add' is CBAdd2d"):
        pkg.BranchGroup([net])
