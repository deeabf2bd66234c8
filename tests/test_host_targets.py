"""CPU-only tests of the operator target tools (tools/*_target.py): the input generator and the round order of
tools/target_common.py are pinned, and no tool keeps a private copy of the measuring method.  No kernel is launched and
no tool's main() runs here."""
import ast
import glob
import hashlib
import importlib
import os
import sys

import numpy as np
import pytest

TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
if TOOLS not in sys.path:
    sys.path.insert(0, TOOLS)
import target_common as tc  # noqa: E402

# the tools that measure whole modules by another scheme
OTHER_SCHEME = ("geom_target", "fg_target", "pose_target")
OPERATOR_TOOLS = sorted(name for name in (os.path.basename(p)[:-3] for p in glob.glob(os.path.join(TOOLS, "*_target.py")))
                        if name not in OTHER_SCHEME)
SHARED = ("timed", "rounds", "change_sets", "pack", "fmt", "BATCH", "SETS")


@pytest.mark.parametrize("seed, H, W, block, share, pixels, digest", [
    (7, 96, 320, 8, 0.10, 49152, "a24a86377c1a8157"),
    (7, 80, 120, 8, 0.10, 15360, "ef6a90680125d524"),
    (11, 96, 320, 8, 0.05, 24576, "03c7dd956bf6899e"),
    (7, 40, 60, 4, 0.10, 3840, "0fab6707b4f09efb"),
    (7, 5, 70, 4, 0.10, 586, "ec563d2bae6ff032"),      # a partial block in both axes, two mask words per row
])
def test_change_sets_and_pack_are_the_recorded_tables_inputs(seed, H, W, block, share, pixels, digest):
    """The checksums were taken from the copy every tool carried before the common module existed: the tables under
    profiles/ were recorded on these change sets."""
    sets = tc.change_sets(np.random.default_rng(seed), H, W, block, share)
    assert len(sets) == tc.SETS == 16
    assert all(m.shape == (H, W) and m.dtype == bool for m in sets)
    assert sum(int(m.sum()) for m in sets) == pixels
    words = [tc.pack(m) for m in sets]
    assert all(w.dtype == np.int64 and w.shape == (H * ((W + 63) // 64),) for w in words)
    assert hashlib.sha256(b"".join(w.tobytes() for w in words)).hexdigest()[:16] == digest


def test_pack_sets_bit_x_mod_64_of_word_x_div_64():
    m = np.zeros((5, 70), dtype=bool)
    m[0, 0] = m[1, 63] = m[2, 64] = m[4, 69] = True
    w = tc.pack(m).view(np.uint64).reshape(5, 2)
    want = np.zeros((5, 2), dtype=np.uint64)
    want[0, 0], want[1, 0], want[2, 1], want[4, 1] = 1, 1 << 63, 1, 1 << 5
    assert np.array_equal(w, want)


@pytest.fixture
def recorder(monkeypatch):
    calls = []

    def timed(fn, n):
        calls.append((fn, n))
        return float(len(calls))
    monkeypatch.setattr(tc, "timed", timed)
    return calls


def test_rounds_warms_every_run_once_then_interleaves(recorder):
    t = tc.rounds([("a", "A"), ("b", "B"), ("c", "C")], 3)
    assert "".join(fn for fn, _ in recorder) == "ABC" + "ABC" * 3
    assert all(n == tc.BATCH == 32 for _, n in recorder)
    # the warm-up batches (calls 1 to 3) are not among the times
    assert t == {"a": [4.0, 7.0, 10.0], "b": [5.0, 8.0, 11.0], "c": [6.0, 9.0, 12.0]}


def test_rounds_with_two_warm_ups_warms_a_run_twice_in_a_row(recorder):
    t = tc.rounds([("a", "A"), ("b", "B"), ("c", "C")], 3, warm=2)
    assert "".join(fn for fn, _ in recorder) == "AABBCC" + "ABC" * 3
    assert all(n == tc.BATCH for _, n in recorder)
    assert [len(v) for v in t.values()] == [3, 3, 3] and list(t) == ["a", "b", "c"]


def test_fmt_is_median_min_max():
    assert tc.fmt([3.0, 1.0, 2.0]) == "2.0 [1.0..3.0]"


def test_listed_share_is_the_mean_share_in_percent():
    sets = [np.zeros((4, 4), dtype=bool), np.ones((4, 4), dtype=bool)]
    assert tc.listed_share(sets) == 50.0


def test_the_converted_tools_are_all_there():
    assert OPERATOR_TOOLS == sorted(n + "_target" for n in (
        "adaptpool", "add", "binary", "channel", "collapse", "decoder", "dw", "group", "groupnorm", "pad", "pointwise",
        "pool", "rearrange", "resize", "se", "tconv"))


@pytest.mark.parametrize("name", OPERATOR_TOOLS)
def test_tool_has_no_private_copy_of_the_method(name, monkeypatch):
    """Importing a tool touches no device (its main() asserts that there is one), and whichever part of the method the
    tool names is target_common's own object."""
    import torch

    def touched(*args, **kwargs):
        raise AssertionError("importing %s initialises the device" % name)
    monkeypatch.setattr(torch.cuda, "_lazy_init", touched)
    sys.modules.pop(name, None)
    mod = importlib.import_module(name)
    assert callable(mod.main)
    for attr in SHARED:
        if hasattr(mod, attr):
            assert getattr(mod, attr) is getattr(tc, attr), "%s.%s is a private copy" % (name, attr)
    assert mod.rounds is tc.rounds and mod.fmt is tc.fmt      # every operator tool measures and prints this way
    assert not hasattr(mod, "pack_mask")
    with open(os.path.join(TOOLS, name + ".py")) as f:
        tree = ast.parse(f.read())
    for node in ast.walk(tree):
        if isinstance(node, (ast.Import, ast.ImportFrom)):
            names = [node.module or ""] if isinstance(node, ast.ImportFrom) else [a.name for a in node.names]
            assert not any(n.endswith("_target") for n in names), "%s imports from another tool: %s" % (name, names)
    # (`is` cannot tell a second BATCH = 32 from the first: the tool's own top level may not bind any of the names)
    for node in tree.body:
        bound = set()
        if isinstance(node, (ast.FunctionDef, ast.ClassDef)):
            bound = {node.name}
        elif isinstance(node, ast.Assign):
            bound = {n.id for t in node.targets for n in ast.walk(t) if isinstance(n, ast.Name)}
        assert not bound & set(SHARED), "%s binds %s itself" % (name, sorted(bound & set(SHARED)))
