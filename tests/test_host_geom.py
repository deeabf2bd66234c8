"""Host-side tests of the general-geometry CBConv2d (no GPU): construction and conversion, the library's output-size
helper against torch, pickling, and the generated code of the new kernels (cb_geomconv.hip)."""
import copy
import ctypes
import os
import pickle
import re
import struct
import subprocess
import tempfile

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (kernel, stride, padding, dilation): the geometries tests/test_gpu_geom.py runs
GEOMS = [((7, 7), (2, 2), (3, 3), (1, 1)), ((3, 3), (2, 2), (1, 1), (1, 1)), ((1, 1), (2, 2), (0, 0), (1, 1)),
         ((3, 3), (1, 1), (2, 2), (2, 2)), ((3, 3), (1, 1), (4, 4), (4, 4)), ((3, 3), (1, 1), (0, 0), (1, 1)),
         ((3, 3), (2, 2), (2, 2), (2, 2)), ((4, 4), (2, 2), (1, 1), (1, 1)), ((2, 2), (2, 2), (0, 0), (1, 1)),
         ((4, 4), (4, 4), (0, 0), (1, 1)), ((3, 5), (2, 1), (0, 3), (1, 2))]


def resnet_like():
    return nn.Sequential(
        nn.Sequential(nn.Conv2d(3, 8, 7, stride=2, padding=3, bias=False), nn.ReLU()),          # stem
        nn.Conv2d(8, 16, 3, stride=2, padding=1), nn.ReLU(), nn.Conv2d(8, 16, 1, stride=2),    # down-sampling block
        nn.Dropout(), nn.Conv2d(16, 16, 3, padding=2, dilation=2), nn.ReLU(), nn.Conv2d(16, 4, 1))   # dilated head


def test_constructor_takes_every_geometry_only_with_the_flag():
    import pycbinfer
    for k, s, p, d in GEOMS:
        for bias in (True, False):
            conv = nn.Conv2d(3, 8, k, stride=s, padding=p, dilation=d, bias=bias)
            m = pycbinfer.CBConv2d(conv, 0.1, generalGeometry=True)      # (a TypeError before the feature existed)
            assert m.generalGeometry and m._geom
            assert (m.kernel_size, m.stride, tuple(m.padding), m.dilation) == (k, s, p, d)
            assert m.weight is conv.weight and m.bias is conv.bias
            assert m._path(torch.zeros(1, 3, 40, 40), 40, 40) == 'geom'
            assert m._path(torch.zeros(1, 3, 40, 40), 20, 20, pooled=True) == 'dense'
            with pytest.raises(AssertionError):
                pycbinfer.CBConv2d(conv, 0.1)
    # a unit-geometry module is not moved to the new path by the flag; without a bias it is
    unit = pycbinfer.CBConv2d(nn.Conv2d(3, 8, 3, padding=1), 0.1, generalGeometry=True)
    assert unit.generalGeometry and not unit._geom
    assert pycbinfer.CBConv2d(nn.Conv2d(3, 8, 3, padding=1, bias=False), 0.1, generalGeometry=True)._geom
    assert not pycbinfer.CBConv2d(nn.Conv2d(3, 8, 3, padding=1), 0.1).generalGeometry
    # string padding: 'valid', symmetric 'same'; an asymmetric 'same' is refused with a sentence
    assert tuple(pycbinfer.CBConv2d(nn.Conv2d(3, 8, 3, padding='valid'), 0.1, generalGeometry=True).padding) == (0, 0)
    same = pycbinfer.CBConv2d(nn.Conv2d(3, 8, 3, padding='same', dilation=3), 0.1, generalGeometry=True)
    assert tuple(same.padding) == (3, 3) and same._out_hw(17, 23) == (17, 23)
    from cbinfer_amd._lib import CBinferError
    for bad in (nn.Conv2d(3, 8, 4, padding='same'), nn.Conv2d(3, 8, 16, stride=16), nn.Conv2d(3, 8, 3, stride=5),
                nn.Conv2d(3, 8, 3, dilation=9), nn.Conv2d(4, 8, 3, groups=2), nn.ConvTranspose2d(3, 8, 3),
                nn.Conv2d(3, 8, 3, padding=1, padding_mode='reflect')):
        with pytest.raises(CBinferError):
            pycbinfer.CBConv2d(bad, 0.1, generalGeometry=True)
    fg = pycbinfer.CBConv2d(nn.Conv2d(3, 8, 3, stride=2), 0.1, generalGeometry=True)
    fg.finegrained = True
    with pytest.raises(CBinferError):
        fg._path(torch.zeros(1, 3, 9, 9), 9, 9)


def test_convert_with_general_geometry():
    import pycbinfer
    with pytest.raises(AssertionError):
        pycbinfer.convert(resnet_like())
    cb = pycbinfer.convert(resnet_like(), threshold=0.2, generalGeometry=True)
    assert [n for n, _ in cb.named_children()] == ['0', '1', '3', '5', '7']
    assert [n for n, _ in cb[0].named_children()] == ['0']
    mods = [cb[0][0], cb[1], cb[2], cb[3], cb[4]]
    assert all(type(m) is pycbinfer.CBConv2d and m.threshold == 0.2 for m in mods)
    assert [bool(m._geom) for m in mods] == [True, True, True, True, False]
    assert [m.withReLU for m in mods] == [True, True, False, True, False]
    assert mods[0].bias is None and 'bias=False' in repr(mods[0]) and 'dilation=(2, 2)' in repr(mods[3])
    pycbinfer.propChangeIndexesOf1x1(cb)
    assert mods[3].propChangeIndexes and not mods[1].propChangeIndexes
    # the execution-level options leave such a layer alone
    net = pycbinfer.convert(nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), nn.MaxPool2d(2), nn.Conv2d(8, 8, 3, stride=2),
                                          nn.Conv2d(8, 8, 3, padding=1)), generalGeometry=True)
    pycbinfer.insertCBPooling(net)
    for m in net:
        if type(m) is pycbinfer.CBConv2d:
            m.feedbackLoop = True
    pycbinfer.fuseDetectionIntoProducer(pycbinfer.fusePoolingIntoDetection(net))
    assert type(net[1]) is pycbinfer.CBPoolMax2d and not net[1].lazy
    assert '_fusedNext' not in net[0].__dict__ and '_fusedConsumers' not in net[2].__dict__
    from cbinfer_amd._lib import CBinferError
    with pytest.raises(CBinferError, match="'2'"):
        pycbinfer.SequenceBatch(net, 2)
    with pytest.raises(CBinferError, match="'0.2'"):
        pycbinfer.BranchGroup([net])


def test_geom_out_size_equals_torch():
    from cbinfer_amd import _lib
    C = _lib.C
    checked = invalid = ones = 0
    for H in (1, 2, 5, 7, 8, 16, 31, 33):
        for k in (1, 2, 3, 4, 5, 7):
            for s in (1, 2, 3, 4):
                for p in (0, 1, 3):
                    for d in (1, 2, 4, 8):
                        g = _lib.Geom(k, k, s, s, p, p, d, d)
                        ho, wo = ctypes.c_int(-5), ctypes.c_int(-5)
                        st = C.cbinfer_geom_out_size(H, H + 3, ctypes.byref(g), ctypes.byref(ho), ctypes.byref(wo))
                        try:
                            ref = F.conv2d(torch.zeros(1, 1, H, H + 3), torch.zeros(1, 1, k, k), stride=s, padding=p,
                                           dilation=d).shape[-2:]
                        except RuntimeError:
                            ref = None
                        if ref is None:
                            assert st != 0, (H, k, s, p, d)
                            assert (ho.value, wo.value) == (-5, -5)
                            invalid += 1
                        else:
                            assert st == 0 and (ho.value, wo.value) == tuple(ref), (H, k, s, p, d)
                            ones += ho.value == 1
                        checked += 1
    assert checked > 2000 and invalid > 100 and ones > 100
    # beyond the limits, and nonsense: a status, not a crash
    ho, wo = ctypes.c_int(), ctypes.c_int()
    for bad, status in ((_lib.Geom(16, 16, 16, 16, 0, 0, 1, 1), -2), (_lib.Geom(3, 3, 5, 1, 0, 0, 1, 1), -2),
                        (_lib.Geom(3, 3, 1, 1, 0, 0, 9, 1), -2), (_lib.Geom(3, 3, 1, 1, 65, 0, 1, 1), -2),
                        (_lib.Geom(0, 3, 1, 1, 0, 0, 1, 1), -1), (_lib.Geom(3, 3, 0, 1, 0, 0, 1, 1), -1),
                        (_lib.Geom(3, 3, 1, 1, -1, 0, 1, 1), -1)):
        assert C.cbinfer_geom_out_size(32, 32, ctypes.byref(bad), ctypes.byref(ho), ctypes.byref(wo)) == status
        assert C.cbinfer_geom_prepared_weights_bytes(8, 3, ctypes.byref(bad), 0) == 0
    assert C.cbinfer_geom_out_size(0, 32, ctypes.byref(_lib.Geom(3, 3, 1, 1, 1, 1, 1, 1)), ctypes.byref(ho),
                                   ctypes.byref(wo)) == -1
    # prepared weights: [K to 64][C kH kW to 32] elements + two ints per k
    g = _lib.Geom(7, 7, 2, 2, 3, 3, 1, 1)
    assert C.cbinfer_geom_prepared_weights_bytes(64, 3, ctypes.byref(g), _lib.CB_F32S) == 64 * 160 * 4 + 160 * 8
    assert C.cbinfer_geom_prepared_weights_bytes(65, 3, ctypes.byref(g), _lib.CB_F16) == 128 * 160 * 2 + 160 * 8


def test_pickle_and_deepcopy_keep_the_geometry():
    import pycbinfer
    conv = nn.Conv2d(3, 8, (3, 5), stride=(2, 1), padding=(0, 3), dilation=(1, 2), bias=False)
    m = pycbinfer.CBConv2d(conv, 0.3, generalGeometry=True)
    m._geom_struct()      # (the transient ctypes struct must not travel)
    for twin in (pickle.loads(pickle.dumps(m)), copy.deepcopy(m)):
        assert twin.generalGeometry and twin._geom and twin.bias is None and twin.threshold == 0.3
        assert (twin.kernel_size, twin.stride, tuple(twin.padding), twin.dilation) == ((3, 5), (2, 1), (0, 3), (1, 2))
        assert twin._out_hw(21, 40) == m._out_hw(21, 40) == (10, 38)
        assert sorted(twin.state_dict()) == ['prevInput', 'prevOutput', 'weight']
    # a module pickled before the attribute existed loads as generalGeometry=False
    old = pycbinfer.CBConv2d(nn.Conv2d(3, 8, 3, padding=1), 0.1)
    state = old.__getstate__()
    for name in ('generalGeometry', '_geom', '_geomC'):
        state.pop(name)
    back = pycbinfer.CBConv2d.__new__(pycbinfer.CBConv2d)
    back.__setstate__(state)
    assert back.generalGeometry is False and not back._geom
    assert back._path(torch.zeros(1, 3, 8, 8), 8, 8) != 'geom'


def _gfx950_code_objects(path):
    """The gfx950 code objects bundled in a host shared library (clang offload bundles)."""
    data = open(path, 'rb').read()
    magic, out, at = b'__CLANG_OFFLOAD_BUNDLE__', [], 0
    while True:
        at = data.find(magic, at)
        if at < 0:
            return out
        n, = struct.unpack_from('<Q', data, at + 24)
        off = at + 32
        for _ in range(n):
            o, size, tl = struct.unpack_from('<QQQ', data, off)
            triple = data[off + 24:off + 24 + tl].decode()
            off += 24 + tl
            if 'gfx950' in triple and size:
                out.append(data[at + o:at + o + size])
        at += len(magic)


def test_new_kernels_use_mfma_and_no_scratch():
    """Disassembled from the built library: the contraction kernels of cb_geomconv.hip hold MFMA instructions of their
    arithmetic, no kernel of the file uses scratch memory, and the source names none of the excluded instructions."""
    objdump = "/opt/rocm/llvm/bin/llvm-objdump"
    readelf = "/opt/rocm/llvm/bin/llvm-readelf"
    if not os.path.exists(objdump):
        import shutil
        objdump, readelf = shutil.which("llvm-objdump"), shutil.which("llvm-readelf")
    assert objdump and readelf
    found = {}
    with tempfile.TemporaryDirectory() as tmp:
        for i, blob in enumerate(_gfx950_code_objects(os.path.join(REPO, "cbinfer_amd", "libcbinfer_hip.so"))):
            path = os.path.join(tmp, "co%d.elf" % i)
            open(path, 'wb').write(blob)
            asm = subprocess.run([objdump, "-d", "--no-show-raw-insn", path], capture_output=True, text=True,
                                 check=True).stdout
            if 'cbg_conv_kernel' not in asm:
                continue
            for name, body in re.findall(r"<(\S*cbg_\S*)>:\n(.*?)(?=\n\S*\s*<\S+>:\n|\Z)", asm, re.S):
                found[name] = body
            notes = subprocess.run([readelf, "--notes", path], capture_output=True, text=True, check=True).stdout
            for blk in notes.split(".agpr_count:")[1:]:
                f = dict(re.findall(r"\.(\w+):\s+(\S+)", blk))
                if 'cbg_' in f.get('name', ''):
                    assert f['private_segment_fixed_size'] == '0', f['name']
                    assert f['vgpr_spill_count'] == '0' and f['sgpr_spill_count'] == '0', f['name']
                    found.setdefault('meta', []).append(f['name'])
    kernels = [n for n in found if n != 'meta']
    assert len([n for n in kernels if 'cbg_conv_kernel' in n]) == 3 and len(found.get('meta', ())) == 7, sorted(found)
    want = {'IDF16_Li1E': 'v_mfma_f32_32x32x16_f16', 'IfLi2E': 'v_mfma_f32_32x32x16_bf16', 'IfLi0E': 'v_mfma_f32_32x32x2_f32'}
    for name in kernels:
        assert 'scratch_' not in found[name], name
        for tag, insn in want.items():
            if 'cbg_conv_kernel' + tag in name:
                assert insn in found[name], name
    src = open(os.path.join(REPO, "cbinfer_amd", "csrc", "cb_geomconv.hip")).read().lower()
    for word in ("s_" + "store", "s_buffer_" + "store", "s_scratch_" + "store", "s_" + "atomic", "s_buffer_" + "atomic",
                 "s_dcache_" + "wb", "s_dcache_" + "discard", "getenv"):
        assert word not in src, word


def test_state_of_a_layer_with_unreachable_output_pixels_starts_as_their_dense_value():
    """Padding beyond the dilated filter's reach (p > d (k-1) on an axis): the outer output pixels have no tap inside
    the input map, are never listed and never written.  Their dense value is the bias (after the ReLU), so prevOutput
    is allocated holding it instead of +inf -- bit for bit torch's dense result there --, again after clearMemory(), a
    change of resolution or dtype, with the flags of that moment; every other layer still allocates +inf."""
    import pycbinfer
    torch.manual_seed(3)
    ring = [nn.Conv2d(3, 4, 3, padding=3), nn.Conv2d(3, 4, 2, stride=2, padding=2, bias=False),
            nn.Conv2d(3, 4, 1, padding=64), nn.Conv2d(3, 4, (3, 3), padding=(1, 3)),
            nn.Conv2d(3, 4, 3, stride=2, padding=5, dilation=2)]
    for conv in ring:
        for relu in (False, True):
            m = pycbinfer.CBConv2d(conv, 0.1, generalGeometry=True)
            m.withReLU = relu
            assert m._has_unreached_outputs()
            for size, dtype in (((1, 3, 5, 6), torch.float32), ((1, 3, 7, 4), torch.float32), ((1, 3, 7, 4), torch.float16)):
                x = torch.rand(size)
                m._state_for(size, x.to(dtype))
                with torch.no_grad():
                    dense = conv(x)
                    if relu:
                        dense = F.relu(dense)
                    reach = F.conv2d(torch.ones(1, 1, *size[2:]), torch.ones(1, 1, *conv.kernel_size), stride=conv.stride,
                                     padding=conv.padding, dilation=conv.dilation)[0, 0] > 0
                assert not reach.all() and reach.any()
                assert m.prevOutput.dtype == dtype and tuple(m.prevOutput.shape) == tuple(dense.shape)
                assert torch.isinf(m.prevInput).all()
                assert torch.equal(m.prevOutput[0][:, ~reach], dense[0][:, ~reach].to(dtype))
            # a flag toggled later reaches these pixels when the state is allocated again
            m.withReLU = not relu
            m.clearMemory()
            m._state_for((1, 3, 5, 6), torch.zeros(1, 3, 5, 6))
            want = torch.zeros(4) if conv.bias is None else conv.bias.detach()
            want = F.relu(want) if m.withReLU else want
            assert torch.equal(m.prevOutput, want.view(1, 4, 1, 1).expand(1, 4, *m._out_hw(5, 6)))
            back = pickle.loads(pickle.dumps(m))
            assert torch.equal(back.prevOutput, m.prevOutput) and back._has_unreached_outputs()
    for conv in (nn.Conv2d(3, 4, 3, padding=2, dilation=2), nn.Conv2d(3, 4, 3, stride=2, padding=2),
                 nn.Conv2d(3, 4, 7, stride=2, padding=3, bias=False)):
        m = pycbinfer.CBConv2d(conv, 0.1, generalGeometry=True)
        assert not m._has_unreached_outputs()
        m._state_for((1, 3, 9, 9), torch.zeros(1, 3, 9, 9))
        assert torch.isinf(m.prevOutput).all()
    unit = pycbinfer.CBConv2d(nn.Conv2d(3, 4, 3, padding=1), 0.1)
    assert not unit._has_unreached_outputs()
