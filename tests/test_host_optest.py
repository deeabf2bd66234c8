"""Host tests of tests/optest.py itself: the mask packing and the hostile list, entry by entry, and a scan that keeps second
copies of its helpers out of the other test files."""
import ast
import glob
import os

import numpy as np
import torch

import optest

HERE = os.path.dirname(os.path.abspath(__file__))

# A file that keeps a helper under a name of optest.__all__ because it MEANS something else there.
OTHER_MEANING = {
    ("test_gpu_listconv.py", "lib"): "the fixture hands out the ctypes library object C, not the _lib module",
    ("test_host_layer.py", "pkg"): "the fixture hands out cbinfer_amd, not pycbinfer",
    ("test_gpu_detect.py", "dev"): "uploads uint64 mask words too, as int64",
    ("test_gpu_adaptpool.py", "operand"): "a module's well-formed change information in the forms tensor / list / mask",
    ("test_gpu_pool.py", "walk_frames"): "generates the eight input frames of the pooling networks",
    ("test_gpu_chain.py", "share_of"): "the listed share of an operator of chain.PRODUCERS, by its mask or the handed-on set",
}


def test_pack_against_a_hand_written_map():
    """3 x 70: two words per row; bits 0, 63, 64 and 69 of a row land in bit 0 and 63 of its first word and in bit 0 and 5
    of its second; the 58 padding bits of every second word stay clear."""
    m = np.zeros((3, 70), dtype=bool)
    m[0, 0] = m[0, 63] = True
    m[1, 64] = m[1, 69] = True
    m[2, :] = True
    words = optest.pack(m)
    assert words.dtype == np.uint64 and words.shape == (6,) == (optest.mask_words(3, 70),)
    assert [int(w) for w in words] == [(1 << 63) | 1, 0, 0, (1 << 5) | 1, (1 << 64) - 1, (1 << 6) - 1]
    assert int(optest.bits_of(np.float32(1.0))) == 0x3F800000 and optest.bits_of(np.ones(2, np.float16)).dtype == np.uint16


def test_hostile_list_entry_by_entry(monkeypatch):
    """A 2 x 5 map with pixels 1, 4 and 7 listed: the list is 7, 4, 1 (reversed), 7 again (the duplicate), 10, -1 and 87
    (outside the map); with a device count, five junk entries follow and the count stops in front of them.  (The device
    upload is replaced by the identity: this is the host's part.)"""
    monkeypatch.setattr(optest, "dev", lambda a: torch.from_numpy(np.ascontiguousarray(a)))
    m = np.zeros((2, 5), dtype=bool)
    m.reshape(-1)[[1, 4, 7]] = True
    buf, cap, cnt = optest.hostile_list(m)
    assert buf.dtype == torch.int32 and buf.tolist() == [7, 4, 1, 7, 10, -1, 87] and cap == 7 and cnt is None
    buf, cap, cnt = optest.hostile_list(m, junk=3, use_count=True)
    assert buf.dtype == torch.int32 and buf.tolist() == [7, 4, 1, 7, 10, -1, 87, 3, 3, 3, 3, 3] and cap == 12
    assert cnt.dtype == torch.int32 and cnt.tolist() == [7]
    assert optest.operand_args("list", m, 3, True)[0] is None and optest.operand_args("all", m) == (None, None, 0, None)
    assert optest.free_pixel(m) == 0 and optest.free_pixel(m, middle=True) == 5 and optest.free_pixel(~(m & ~m)) is None


def test_no_other_test_file_defines_what_optest_provides():
    """No file of tests/ but optest.py defines, at top level, a function, class or fixture whose name is in
    optest.__all__; the exceptions are the files of OTHER_MEANING, each with its reason -- and each must still exist."""
    names = set(optest.__all__)
    assert all(hasattr(optest, n) for n in names)
    found, seen = [], set()
    for path in sorted(glob.glob(os.path.join(HERE, "*.py"))):
        base = os.path.basename(path)
        if base == "optest.py":
            continue
        with open(path) as f:
            tree = ast.parse(f.read())
        for node in tree.body:
            if isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef, ast.ClassDef)) and node.name in names:
                (seen.add if (base, node.name) in OTHER_MEANING else found.append)((base, node.name))
    assert not found, found
    assert seen == set(OTHER_MEANING), set(OTHER_MEANING) - seen

