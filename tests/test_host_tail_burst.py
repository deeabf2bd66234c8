"""CPU tests of the reduce+tail launch's request bursts (cbs_reduce_tail_kernel of cb_split.hip), on the
generated code of cb_split.hip compiled to gfx950 assembly:

  * from the kernel's first vector-memory load to the end of the first group's request burst (marked in the source by the
    assembly comment `cbs_tail_first_burst_end`) stands ONE `s_waitcnt vmcnt` -- the wait of the entry burst, for the
    launch info -- and no LDS write (W2 / b2 are staged behind the burst); the wait for the list index follows the mark;
  * the launch info is loaded in the entry block and nowhere else: not inside the group loop;
  * registers, scratch and LDS of the six instances are what tools/kernel_regs.py reports: 94 / 95 / 187 VGPRs (the
    parent: 102 / 102 / 194), no scratch, 64 bytes of static LDS (the parent's).

The waits are counted along the control-flow graph of the listing without its back edges (an edge to a block on the
depth-first stack: the first trip through every loop).  The compiler joins the launch's variants (gather path, one / two /
four quads a thread, the first and the later rounds) in blocks that branch on a flag, so the listing has paths no workgroup
takes -- out of one variant's body into the next one's burst.  The count is therefore that of the path with the FEWEST
waits: what every path to the mark holds at the least, the first group's own among them -- the entry's wait, any wait in a
block all paths share, any wait inside the burst's own block.  The last is also asserted by itself: none."""
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "cbinfer_amd", "csrc")

MARK = "cbs_tail_first_burst_end"        # (the later groups' body: NEXT_MARK)
NEXT_MARK = "cbs_tail_next_burst_end"
MAX_WAITS = 1                   # (the entry burst's: the wait for the list index stands behind the last slab request)
VLOAD = re.compile(r"^(global_load|flat_load|buffer_load|scratch_load)")
PREFIX = "_ZN3cbs22cbs_reduce_tail_kernel"
# tools/kernel_regs.py: vgpr (the parent commit's: 194 / 102 / 102), scratch, static LDS (both as the parent's)
FIGURES = {"ILi64ELi64ELi1E": (187, 0, 64), "ILi64ELi64ELi2E": (95, 0, 64), "ILi64ELi64ELi4E": (94, 0, 64),
           "ILi128ELi128ELi1E": (187, 0, 64), "ILi128ELi128ELi2E": (95, 0, 64), "ILi128ELi128ELi4E": (94, 0, 64)}


def _asm(tmp, name):
    out = os.path.join(str(tmp), name + ".s")
    subprocess.check_call(["hipcc", "-O3", "--offload-arch=gfx950", "-std=c++17", "-fopenmp", "--cuda-device-only", "-S",
                           "-I", CSRC, os.path.join(CSRC, name + ".hip"), "-o", out], stderr=subprocess.DEVNULL)
    with open(out) as f:
        return f.read()


def _metadata(text):
    meta = text[text.index("amdhsa.kernels:"):]
    out = {}
    for blk in meta.split("  - .agpr_count:")[1:]:
        f = dict(re.findall(r"\.(\w+):\s+(\S+)", blk))
        f["agpr_count"] = blk.split()[0]
        out[f["name"]] = f
    return out


def _bodies(text, prefix):
    """{kernel: [instruction]}: labels kept, directives and comments dropped, the burst mark kept as the word MARK."""
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^(%s\S*):" % prefix, line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is None:
            continue
        if MARK in line or NEXT_MARK in line:
            cur.append("MARK" if MARK in line else "NEXT_MARK")
            continue
        ins = line.split(";")[0].strip()
        if ins.startswith(".Lfunc_end"):
            cur = None
            continue
        if not ins or (ins.startswith(".") and not ins.endswith(":")):
            continue
        cur.append(ins)
    return out


def _blocks(body):
    """[(label or None, [instruction])] and {label: block index}."""
    blocks, cur = [], (None, [])
    for ins in body:
        if ins.endswith(":"):
            if cur[1] or cur[0]:
                blocks.append(cur)
            cur = (ins[:-1], [])
            continue
        cur[1].append(ins)
        if re.match(r"^(s_branch|s_cbranch_\w+|s_endpgm|s_setpc_b64)\b", ins):
            blocks.append(cur)
            cur = (None, [])
    if cur[1] or cur[0]:
        blocks.append(cur)
    return blocks, {b[0]: i for i, b in enumerate(blocks) if b[0]}


def _succ(blocks, index, i):
    ins = blocks[i][1]
    last = ins[-1] if ins else ""
    if last.startswith("s_endpgm") or last.startswith("s_setpc"):
        return []
    if last.startswith("s_branch"):
        return [index[last.split()[1]]]
    out = [i + 1] if i + 1 < len(blocks) else []
    if last.startswith("s_cbranch"):
        out.append(index[last.split()[1]])
    return out


def _is_wait(ins):
    return ins.startswith("s_waitcnt") and "vmcnt" in ins


def _waits_inside(blocks, index, i, mark):
    """`s_waitcnt vmcnt` between the first vector load of the burst and the mark in block i; the burst's loads are those of
    the mark's block or, where the mark stands alone behind a branch (the first round of a rounds loop), of the blocks
    that branch to it."""
    ins = blocks[i][1]
    head = ins[:ins.index(mark)]
    loads = [k for k, x in enumerate(head) if VLOAD.match(x)]
    if loads:
        return sum(_is_wait(x) for x in head[loads[0]:])
    n = sum(_is_wait(x) for x in head)
    found = None
    for j in range(len(blocks)):
        if j != i and i in _succ(blocks, index, j):
            pj = blocks[j][1]
            lj = [k for k, x in enumerate(pj) if VLOAD.match(x)]
            if lj:
                found = max(found or 0, n + sum(_is_wait(x) for x in pj[lj[0]:]))
    return found


def burst_paths(body):
    """[(waits, LDS writes, waits inside the burst)] per first-group burst mark.  waits / LDS writes: the fewest
    `s_waitcnt vmcnt` / ds_write a path without a back edge holds between the kernel's first vector load and the mark;
    inside the burst: the waits between the first vector load of the mark's own block and the mark."""
    blocks, index = _blocks(body)
    first = next(i for i, b in enumerate(blocks) if any(VLOAD.match(x) for x in b[1]))
    assert first == 0, "the first vector load stands in the entry block"
    # depth-first from the entry: an edge to a block on the stack is a back edge; the rest, in reverse postorder, is a DAG
    state, order, back, stack = {0: 1}, [], set(), [(0, iter(_succ(blocks, index, 0)))]
    while stack:
        i, it = stack[-1]
        j = next(it, None)
        if j is None:
            state[i] = 2
            order.append(i)
            stack.pop()
        elif state.get(j, 0) == 1:
            back.add((i, j))
        elif j not in state:
            state[j] = 1
            stack.append((j, iter(_succ(blocks, index, j))))
    best = {0: (0, 0)}          # at a block's entry
    marks = []
    for i in reversed(order):
        w, d = best[i]
        seen = i != 0
        for x in blocks[i][1]:
            if not seen:
                seen = bool(VLOAD.match(x))
                continue
            if x == "MARK":
                marks.append((w, d, _waits_inside(blocks, index, i, "MARK")))
            w += _is_wait(x)
            d += x.startswith("ds_write")
        for j in _succ(blocks, index, i):
            if (i, j) not in back:
                pw, pd = best.get(j, (w, d))
                best[j] = (min(pw, w), min(pd, d))
    n_marks = sum(x == "MARK" for x in body)
    assert len(marks) == n_marks, "every burst mark is reached (%d of %d)" % (len(marks), n_marks)
    return marks


def info_loads(body):
    """(block index, instruction) of every vector load whose base is the launch-info pointer: the kernel-argument word the
    base of the kernel's FIRST vector load was read from, followed through every scalar load of that word."""
    blocks, _ = _blocks(body)
    flat = [(i, x) for i, b in enumerate(blocks) for x in b[1]]

    def sregs(op):
        m = re.match(r"^s\[(\d+):(\d+)\]$", op)
        if m:
            return set(range(int(m.group(1)), int(m.group(2)) + 1))
        m = re.match(r"^s(\d+)$", op)
        return {int(m.group(1))} if m else set()

    def operands(x):
        return [o.split()[0] for o in x.split(None, 1)[1].split(",") if o.strip()] if " " in x else []      # (modifiers dropped)

    k0 = next(k for k, (_, x) in enumerate(flat) if VLOAD.match(x))
    base = [o for o in operands(flat[k0][1]) if re.match(r"^s\[\d+:\d+\]$", o)]
    assert base, flat[k0][1]
    lo = min(sregs(base[0]))
    off = None
    for _, x in reversed(flat[:k0]):      # the scalar load that filled the pair
        if x.startswith("s_load_dword"):
            ops = operands(x)
            regs = sorted(sregs(ops[0]))
            if lo in regs:
                off = int(ops[2], 0) + 4 * (lo - regs[0])
                break
    assert off is not None, "the first vector load's base comes from the kernel arguments"
    found, holding = [], set()      # holding: the low registers of pairs that hold the info pointer right now
    for i, x in flat:
        ops = operands(x)
        if VLOAD.match(x):
            if any(min(sregs(o)) in holding for o in ops if re.match(r"^s\[\d+:\d+\]$", o)):
                found.append((i, x))
            continue
        if x.startswith("s_load_dword") and ops[1] == "s[0:1]":
            regs = sorted(sregs(ops[0]))
            holding -= set(regs) | {r - 1 for r in regs}
            start = int(ops[2], 0) if re.match(r"^(0x[0-9a-f]+|\d+)$", ops[2]) else None      # (else: a register offset)
            if start is not None and start <= off < start + 4 * len(regs):
                holding.add(regs[0] + (off - start) // 4)
            continue
        if ops and (x.startswith("s_") or x.startswith("v_readlane") or x.startswith("v_readfirstlane")):
            regs = sregs(ops[0])
            holding -= regs | {r - 1 for r in regs}
    return found


@pytest.fixture(scope="module")
def split_asm(tmp_path_factory):
    return _asm(tmp_path_factory.mktemp("isa"), "cb_split")


@pytest.fixture(scope="module")
def tail_bodies(split_asm):
    bodies = _bodies(split_asm, PREFIX)
    assert len(bodies) == 6, sorted(bodies)
    return bodies


def test_first_group_burst_stands_behind_one_wait(tail_bodies):
    for name, body in tail_bodies.items():
        marks = burst_paths(body)
        assert marks, name
        print(name, marks)
        for waits, lds, inside in marks:
            assert waits <= MAX_WAITS, (name, waits)
            assert lds == 0, (name, lds)
            assert inside == 0, (name, inside)
        # the wait for the list index stands BEHIND the mark, in front of the workgroup's first barrier
        blocks, index = _blocks(body)
        for _, ins in blocks:
            if "MARK" in ins:
                rest = ins[ins.index("MARK"):]
                stop = rest.index("s_barrier") if "s_barrier" in rest else len(rest)
                assert any(_is_wait(x) for x in rest[:stop]), name
        # the later groups' body: its burst is not interrupted either
        nxt = [i for i, b in enumerate(blocks) if "NEXT_MARK" in b[1]]
        assert len(nxt) == len(marks), name
        for i in nxt:
            assert _waits_inside(blocks, index, i, "NEXT_MARK") == 0, name


def test_launch_info_is_loaded_at_entry_only(tail_bodies):
    for name, body in tail_bodies.items():
        loads = info_loads(body)
        print(name, loads)
        assert len(loads) == 1 and loads[0][0] == 0, (name, loads)


def test_tail_instances_keep_their_resources(split_asm):
    """Scratch (none) and static LDS as the parent's; the registers the first group's body of its own brought them to
    (94 / 95 / 187 where the parent had 102 / 102 / 194) and no more; a workgroup of the 16-wave instances (S = 2, 4: four
    waves a SIMD) within 128."""
    meta = {k: v for k, v in _metadata(split_asm).items() if k.startswith(PREFIX)}
    assert len(meta) == 6, sorted(meta)
    for name, f in meta.items():
        tag = [t for t in FIGURES if t in name]
        assert len(tag) == 1, name
        vgpr, scratch, lds = FIGURES[tag[0]]
        regs = int(f["vgpr_count"]) + int(f["agpr_count"])
        print(name, "vgpr", regs, "pinned", vgpr)
        assert int(f["private_segment_fixed_size"]) == scratch == 0 and int(f["vgpr_spill_count"]) == 0, name
        assert int(f["group_segment_fixed_size"]) == lds, name
        if "Li1EEE" not in name:
            assert regs <= 128, (name, regs)
        assert regs <= vgpr, (name, regs, vgpr)


def test_launch_info_is_named_once_in_the_source():
    """The kernel's source reads p.info in one place: the entry burst."""
    with open(os.path.join(CSRC, "cb_split.hip")) as f:
        src = f.read()
    body = src[src.index("void cbs_reduce_tail_kernel("):src.index("int cbs_launch_conv(")]
    code = "\n".join(line.split("//")[0] for line in body.splitlines())
    assert len(re.findall(r"\bp\.info\b", code)) == 1
