"""CPU tests of the front half of the frame, on the generated code of cb_rowpair.hip and cb_split.hip (compiled to gfx950
assembly as tools/lint_split_isa.py and tools/lint_vmcnt.py do):

  * the self-detecting row-pair instance is resident five times per CU -- registers, scratch, static LDS --, and the
    instances without detection kept their registers;
  * every cbs_conv_kernel instance scans the change mask in ONE round trip: all mask-word loads of a thread's chunks in
    front of one wait, global loads, and the frame's mask copy stored from the words the scan holds."""
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "cbinfer_amd", "csrc")

LDS_BYTES = 160 * 1024      # per CU (gfx950)
LDS_GRANULE = 1280          # bytes: the allocation granule of the 160 KB LDS (160 KB / 128)
VLOAD = re.compile(r"^(global_load|flat_load|buffer_load|scratch_load)")


def _asm(tmp, name):
    out = os.path.join(str(tmp), name + ".s")
    subprocess.check_call(["hipcc", "-O3", "--offload-arch=gfx950", "-std=c++17", "-fopenmp", "--cuda-device-only", "-S",
                           "-I", CSRC, os.path.join(CSRC, name + ".hip"), "-o", out], stderr=subprocess.DEVNULL)
    with open(out) as f:
        return f.read()


def _metadata(text):
    """{kernel name: {field: value}} from the code object metadata of a listing (as tools/kernel_regs.py reads it)."""
    meta = text[text.index("amdhsa.kernels:"):]
    out = {}
    for blk in meta.split("  - .agpr_count:")[1:]:
        f = dict(re.findall(r"\.(\w+):\s+(\S+)", blk))
        out[f["name"]] = f
    return out


def _bodies(text, prefix):
    """{kernel name: [instruction]} of the kernels whose symbol starts with `prefix` (labels kept, directives dropped)."""
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^(%s\S*):" % prefix, line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is None:
            continue
        ins = line.split(";")[0].strip()
        if ins.startswith(".Lfunc_end"):
            cur = None
            continue
        if not ins or (ins.startswith(".") and not ins.endswith(":")):
            continue
        cur.append(ins)
    return out


@pytest.fixture(scope="module")
def rowpair_asm(tmp_path_factory):
    return _asm(tmp_path_factory.mktemp("isa"), "cb_rowpair")


@pytest.fixture(scope="module")
def split_asm(tmp_path_factory):
    return _asm(tmp_path_factory.mktemp("isa"), "cb_split")


def test_detecting_rowpair_instance_is_resident_five_times_per_cu(rowpair_asm):
    """cbp_rowpair_kernel<7,7,true>: at most 96 registers (five waves per SIMD), no scratch, and five times its static LDS
    -- rounded up to the allocation granule -- within the CU's 160 KB, so that the 1280 units of a 480x320 frame are all
    resident at once.  The instances without detection: their registers as before (107, 107, 104), within +-4."""
    meta = {k: v for k, v in _metadata(rowpair_asm).items() if "cbp_rowpair_kernel" in k}
    assert len(meta) == 4, sorted(meta)
    det = [v for k, v in meta.items() if "ILi7ELi7ELb1E" in k]
    assert len(det) == 1
    det = det[0]
    assert int(det["vgpr_count"]) + int(det.get("agpr_count", 0) or 0) <= 96, det
    assert int(det["private_segment_fixed_size"]) == 0 and int(det["vgpr_spill_count"]) == 0, det
    lds = int(det["group_segment_fixed_size"])
    granules = (lds + LDS_GRANULE - 1) // LDS_GRANULE
    assert 5 * granules * LDS_GRANULE <= LDS_BYTES, lds
    before = {"ILi7ELi7ELb0E": 107, "ILi5ELi5ELb0E": 107, "ILi3ELi3ELb0E": 104}
    for tag, regs in before.items():
        inst = [v for k, v in meta.items() if tag in k]
        assert len(inst) == 1, tag
        assert abs(int(inst[0]["vgpr_count"]) - regs) <= 4, (tag, inst[0]["vgpr_count"])
        assert int(inst[0]["private_segment_fixed_size"]) == 0, tag


def test_mask_scan_is_one_round_trip_in_every_split_instance(split_asm):
    """Every cbs_conv_kernel instance, from its entry to the scan's barrier: the mask words are fetched by global (not
    flat) loads, no `s_waitcnt vmcnt` stands between the first and the last of them, and between the wait behind them and
    the first store of the frame's mask copy there is no vector load -- the copy is written from the scan's registers."""
    bodies = _bodies(split_asm, "_ZN3cbs15cbs_conv_kernel")
    assert len(bodies) == 16, len(bodies)
    for name, body in bodies.items():
        scan = body[:body.index("s_barrier")]
        ops = [i.split()[0] for i in scan]
        assert not any(o.startswith("flat_load") for o in ops), name
        loads = [k for k, o in enumerate(ops) if o == "global_load_dwordx2"]
        assert loads, name
        burst = scan[loads[0]:loads[-1] + 1]
        assert not any(i.startswith("s_waitcnt") and "vmcnt" in i for i in burst), name
        wait = [k for k in range(loads[-1], len(scan)) if scan[k].startswith("s_waitcnt") and "vmcnt" in scan[k]]
        assert wait, name
        store = [k for k in range(wait[0], len(scan)) if ops[k] == "global_store_dwordx2"]
        assert store, name
        assert not any(VLOAD.match(o) for o in ops[wait[0]:store[0]]), name
