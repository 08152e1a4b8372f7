"""CPU: the packed form of the settled MISS-tile kernel (k_mcm_miss_packed; fast-math and bit-exact, CHECK off) compiled to gfx950 assembly
the way tests/test_miss_prologue_isa.py does it: no scratch, no spill, at most 64 VGPRs at 8 waves per SIMD, no workgroup barrier — and on the
path a wave takes when the records are current (miss_load_dir == 0) the pixel's state arrives by ONE global_load_dwordx2 and leaves by one
global_store_dwordx2: the 16-byte direction texel (dwordx4) and the 12-byte position texel (dwordx3) are loaded only by the first packed pass
after another kind of pass.  The path is found in the kernel's control-flow graph: with every basic block that holds a dwordx3 / dwordx4 load
taken out, the entry still reaches the record's load, from there the record's store, and from there the end of the program."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# k_mcm_miss_packed<V in {0, VPT_V_FAST = 16}, CHECK = false, LATE>
PLAIN = re.compile(r"^_Z17k_mcm_miss_packedILi(?:0|16)ELb0ELb[01]EE")


@pytest.fixture(scope="module")
def mcm_unit():
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not installed")
    csrc = os.path.join(ROOT, "vpt_amd", "csrc")
    res = subprocess.run(["make", "-C", csrc, "-B", "vpt_mcm.s"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    assert res.returncode == 0, res.stdout.decode()[-2000:]
    return open(os.path.join(csrc, "vpt_mcm.s")).read(), open(os.path.join(csrc, "vpt_mcm.resources.txt")).read()


def plain_kernels(names):
    got = sorted(n for n in names if PLAIN.match(n))
    # fast-math: LATE on and off; bit-exact: LATE on only (vpt_mcm.hip launch_mcm_classes)
    assert len(got) == 3, got
    return got


def kernel_bodies(asm):
    bodies, cur = {}, None
    for line in asm.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = m.group(1); bodies[cur] = []
        elif re.match(r"^\.Lfunc_end\d+:", line):
            cur = None
        elif cur:
            bodies[cur].append(line)
    return bodies


def test_packed_kernels_use_no_scratch_and_at_most_64_vgprs(mcm_unit):
    _, resources = mcm_unit
    usage, cur = {}, None
    for line in resources.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = m.group(1); usage[cur] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and cur:
            usage[cur][m.group(1).strip()] = int(m.group(2))
    for name in plain_kernels(usage):
        u = usage[name]
        assert u.get("ScratchSize", 0) == 0 and u.get("VGPRs Spill", 0) == 0 and u.get("SGPRs Spill", 0) == 0, (name, u)
        assert u.get("VGPRs", 999) <= 64 and u.get("Occupancy", 0) == 8, (name, u)


def test_packed_kernels_have_no_workgroup_barrier(mcm_unit):
    asm, _ = mcm_unit
    bodies = kernel_bodies(asm)
    for name in plain_kernels(bodies):
        body = bodies[name]
        assert any("s_endpgm" in l for l in body), name       # (the body was found whole)
        assert any("ds_write_b64" in l for l in body), name   # the alpha column's pairs are staged by the wave itself
        barriers = [l for l in body if re.search(r"\bs_barrier\b", l)]
        assert not barriers, (name, barriers)


def blocks_of(body):
    """basic blocks of a kernel body: [(label or None, [instructions], [successor labels], falls_through)] in layout order"""
    blocks, label, ins = [], None, []

    def close(falls):
        succ = [m.group(1) for l in ins for m in [re.match(r"\s*s_c?branch\w*\s+(\.LBB\w+)", l)] if m]
        blocks.append((label, list(ins), succ, falls))

    for line in body:
        m = re.match(r"^(\.LBB\w+):", line)
        if m:
            if ins or label is not None or not blocks:
                close(True)
            label, ins = m.group(1), []
            continue
        text = line.split(";")[0].strip()
        if not text or text.startswith("."):
            continue
        ins.append(text)
        if re.match(r"s_cbranch", text):
            close(True); label, ins = None, []
        elif re.match(r"s_branch|s_endpgm|s_setpc", text):
            close(False); label, ins = None, []
    if ins:
        close(False)
    return blocks


def reach(blocks, start, banned):
    """indices of the blocks reachable from block `start` without entering a block of `banned`"""
    index = {b[0]: i for i, b in enumerate(blocks) if b[0] is not None}
    seen, todo = set(), [start]
    while todo:
        i = todo.pop()
        if i in seen or i in banned or i >= len(blocks):
            continue
        seen.add(i)
        _, _, succ, falls = blocks[i]
        todo.extend(index[s] for s in succ if s in index)
        if falls:
            todo.append(i + 1)
    return seen


def test_current_records_travel_as_one_dwordx2_each_way(mcm_unit):
    asm, _ = mcm_unit
    bodies = kernel_bodies(asm)
    for name in plain_kernels(bodies):
        blocks = blocks_of(bodies[name])
        has = lambda i, pat: any(re.match(pat, l) for l in blocks[i][1])
        wide = {i for i in range(len(blocks)) if has(i, r"global_load_dwordx[34]\b")}
        loads = [i for i in range(len(blocks)) if has(i, r"global_load_dwordx2\b")]
        stores = [i for i in range(len(blocks)) if has(i, r"global_store_dwordx2\b")]
        ends = [i for i in range(len(blocks)) if has(i, r"s_endpgm\b")]
        assert wide, name                                       # (the first packed pass after another kind of pass loads the direction texel)
        assert loads and stores and ends, (name, loads, stores)
        assert not any(has(i, r"global_store_dwordx[34]\b") for i in range(len(blocks))), name   # no direction texel is written
        from_entry = reach(blocks, 0, wide)
        ok = False
        for l in loads:
            if l not in from_entry:
                continue
            from_load = reach(blocks, l, wide)
            for s in stores:
                if s in from_load and any(e in reach(blocks, s, wide) for e in ends):
                    ok = True
        assert ok, (name, "no path entry -> dwordx2 load -> dwordx2 store -> end that avoids the dwordx3 / dwordx4 loads")
