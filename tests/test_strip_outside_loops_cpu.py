"""The f64 forward strip outside its k-loops (csrc/strip.hip: strip_kernel, the panel epilogue of phase 1) - read from the gfx950 code of
the BUILT product library, without a GPU, in the manner of tests/test_kstep_valu_cpu.py.

A forward call without the optional outputs (A_out / At_out: the ELBO and the marginals) ends every panel of phase 1 with: the 16 m
values of the thread's rows, 32 stores of A_I into the scratch strip, 64 f64 multiply-adds into the column sums.  Until round 8 that was

    63 basic blocks per panel (one test of A_out and one of At_out per VALUE, each behind its own branch)
    ~15 vector instructions of 64-bit address arithmetic per row (v_mad_u64_u32, v_lshl_add_u64, v_lshlrev_b64, v_mov): ~240 per panel
    the m value of a row loaded, waited for and used row by row BETWEEN the stores: on gfx950 loads and stores share one counter
    (vmcnt) and return in any order among themselves, so each of the 16 waits also waited for the stores issued before it

Asserted here for the product build:

    one basic block holds all 16 loads, all 32 stores and all 64 multiply-adds of the panel (the optional outputs are tested once)
    every load is issued before the first store, and no vmcnt wait stands between the first store and the last
    at most 24 other vector instructions in that block (measured: 20 - 14 halves of 64-bit adds for the store addresses, 4 v_mov_b64,
    2 v_lshl_add_u64; round 7: ~240 per panel).

The f64 SE pre-generation (pregen_mfma) evaluated one 16 x 16 tile after the other: two dependent MFMAs, `s_nop 15` + `s_nop 2` for their
result, four exponentials as four dependent chains (381 vector instructions per 16-row block in four basic blocks).  The pipelined
body issues the NEXT block's eight MFMAs in front of this block's stores, so that nothing waits for an MFMA result:

    no s_nop of 8 or more wait states directly behind an MFMA in a block that evaluates SE exponentials (v_ldexp_f64, no square root)
    one such block holds all 16 exponentials of a 16-row block, and its eight distance MFMAs behind them

The per-loop entry code: the block that sends off a loop's first three tiles (18 global_load_lds_dwordx4) ahead of any MFMA - phase
1's entry; phase 2's opening shares a block with its first MFMAs.  Round 7: 8 vector instructions (3 v_mov_b32, 4 v_readlane_b32 -
scalar-register reloads -, 1 v_readfirstlane_b32); unchanged now.  The accumulators are not zeroed by moves in either listing: the
first MFMAs of a loop take the literal 0 as their C operand (24 such MFMAs in the kernel, round 7 and now), and no run of zeroing v_mov
exists.  The variant that sent the tiles off in front of the epilogue before (measured and rejected:
profiles/round8/b_prologue_hoist_rejected.patch) had five such blocks with up to 8 v_readlane_b32 each and 174 in the kernel.  Asserted:

    every three-tile opening block holds at most 8 vector instructions, of them at most 4 v_readlane_b32 and at most 3 v_mov
    no block of the kernel holds a run of 8 or more v_mov of the literal 0 (the accumulators keep being zeroed through the C operand)
    the kernel's v_readlane_b32 total does not exceed READLANE_TOTAL = 156 (round 7: 143; the pipelined pre-generation reloads more scalars)"""
import os
import re
import subprocess
import tempfile

import pytest

from approxgp import _ffi

LLVM = "/opt/rocm/lib/llvm/bin"
TOOLS = [os.path.join(LLVM, t) for t in ("llvm-objdump", "clang-offload-bundler", "llvm-objcopy")]

READLANE_TOTAL = 156
F64_FORWARD = "strip_kernelIdLi64ELi16ELi256ELi2ELi16ELb0ELb0ELb0E"   # <T, NT, BK, NTHR, MINW, PAD, GRAD, BIGD, SEG>


def _disassembly(lib_path):
    out = []
    with tempfile.TemporaryDirectory() as td:
        fat = os.path.join(td, "fat.bin")
        subprocess.run([TOOLS[2], "--dump-section", f".hip_fatbin={fat}", lib_path, os.path.join(td, "x.so")], check=True)
        blob = open(fat, "rb").read()
        magic = b"__CLANG_OFFLOAD_BUNDLE__"
        starts, off = [], 0
        while True:
            i = blob.find(magic, off)
            if i < 0:
                break
            starts.append(i)
            off = i + 1
        for k, (a, b) in enumerate(zip(starts, starts[1:] + [len(blob)])):
            part, co = os.path.join(td, f"b{k}.bin"), os.path.join(td, f"co{k}.o")
            open(part, "wb").write(blob[a:b])
            r = subprocess.run([TOOLS[1], "--unbundle", "--type=o", f"--input={part}", f"--output={co}",
                                "--targets=hipv4-amdgcn-amd-amdhsa--gfx950"], capture_output=True, text=True)
            if r.returncode == 0 and os.path.exists(co) and os.path.getsize(co) > 0:
                out.append(subprocess.run([TOOLS[0], "-d", co], capture_output=True, text=True, check=True).stdout)
    return out


@pytest.fixture(scope="module")
def forward_blocks():
    """Basic blocks of the f64 forward strip kernel as lists of (mnemonic, operands)."""
    if not os.path.exists(_ffi.LIB_PATH) or "experiments" in os.path.basename(_ffi.LIB_PATH) or not all(os.path.exists(t) for t in TOOLS):
        pytest.skip("needs the built product library and the ROCm llvm tools")
    head = re.compile(r"^([0-9a-f]{16}) <(\S+)>:$")
    ins = re.compile(r"^\s+(\S+)(.*?)//\s*([0-9A-Fa-f]{12}):(.*)$")
    code = []
    for text in _disassembly(_ffi.LIB_PATH):
        start, on = 0, False
        for line in text.splitlines():
            m = head.match(line)
            if m:
                start, on = int(m.group(1), 16), F64_FORWARD in m.group(2)
                continue
            m = ins.match(line) if on else None
            if not m:
                continue
            mnem, ops, addr, tail = m.group(1), m.group(2).strip(), int(m.group(3), 16), m.group(4)
            target = None
            if mnem.startswith("s_cbranch") or mnem == "s_branch":
                t = re.search(r"<\S+\+0x([0-9a-fA-F]+)>", tail)
                assert t, line
                target = start + int(t.group(1), 16)
            code.append((addr, mnem, ops, target))
    assert code, "the f64 forward strip kernel is not in the library"
    leaders = {code[0][0]}
    for i, (addr, mnem, ops, target) in enumerate(code):
        if target is not None or mnem in ("s_endpgm", "s_setpc_b64"):
            if target is not None:
                leaders.add(target)
            if i + 1 < len(code):
                leaders.add(code[i + 1][0])
    blocks, cur = [], []
    for addr, mnem, ops, _ in code:
        if addr in leaders and cur:
            blocks.append(cur)
            cur = []
        cur.append((mnem, ops))
    blocks.append(cur)
    return blocks


def _is_fma64(m):
    return m.startswith("v_fma_f64") or m.startswith("v_fmac_f64")


def test_phase1_epilogue_without_optional_outputs_is_one_block(forward_blocks):
    epi = [b for b in forward_blocks
           if sum(m == "global_store_dwordx2" for m, _ in b) >= 32 and not any(m.startswith("v_mfma") for m, _ in b)]
    for b in epi:
        print("block:", len(b), "instructions,", sum(m == "global_load_dwordx2" for m, _ in b), "loads,",
              sum(m == "global_store_dwordx2" for m, _ in b), "stores,", sum(_is_fma64(m) for m, _ in b), "f64 multiply-adds")
    assert len(epi) == 1, [len(b) for b in epi]           # round 7: no block of the kernel held more than 3 of a panel's 32 stores
    b = epi[0]
    mn = [m for m, _ in b]
    assert mn.count("global_store_dwordx2") == 32 and mn.count("global_load_dwordx2") == 16
    assert sum(_is_fma64(m) for m in mn) == 64
    first_store = mn.index("global_store_dwordx2")
    last_store = len(mn) - 1 - mn[::-1].index("global_store_dwordx2")
    last_load = len(mn) - 1 - mn[::-1].index("global_load_dwordx2")
    assert last_load < first_store, (last_load, first_store)
    waits = [ops for m, ops in b[first_store:last_store] if m == "s_waitcnt" and "vmcnt" in ops]
    assert waits == [], waits                               # round 7: 16 such waits per panel, each behind the stores of the row before
    other = [m for m in mn if m.startswith("v_") and not _is_fma64(m)]
    print("other vector instructions:", len(other), sorted(set(other)))
    assert len(other) <= 24, other                          # measured 20; round 7: ~240 per panel


def test_pregeneration_does_not_wait_for_an_mfma_result(forward_blocks):
    # the SE blocks: exponentials (v_ldexp_f64) and distance MFMAs, and no square root (the Matern bodies of the same kernel, which keep
    # the block-at-a-time form, take sqrt(r2) through v_rsq_f64)
    pre = [b for b in forward_blocks if sum(m.startswith("v_ldexp_f64") for m, _ in b) >= 4 and any(m.startswith("v_mfma_f64") for m, _ in b)
           and not any(m.startswith("v_rsq_f64") or m.startswith("v_sqrt_f64") for m, _ in b)]
    assert pre, "no pre-generation block found"
    for b in pre:
        mn = [m for m, _ in b]
        n_exp, n_mfma = sum(m.startswith("v_ldexp_f64") for m in mn), sum(m.startswith("v_mfma_f64") for m in mn)
        nops = [int(ops, 0) for (m, ops), (pm, _) in zip(b[1:], b[:-1]) if m == "s_nop" and pm.startswith("v_mfma")]
        print(f"pre-generation block: {len(b)} instructions, {n_exp} exponentials, {n_mfma} MFMAs, s_nop behind an MFMA: {nops}")
        assert all(n < 8 for n in nops), ("SE blocks only - the Matern and wide-input bodies keep the block-at-a-time form", nops)   # round 7: s_nop 15 behind every tile's MFMA pair
    # the 8-feature and the 16-feature body: 16 exponentials per block, the next block's MFMAs (2 resp. 4 rounds over 4 tiles) behind the last
    full = [b for b in pre if sum(m.startswith("v_ldexp_f64") for m, _ in b) == 16]
    assert len(full) >= 2, len(full)
    for b in full:
        mn = [m for m, _ in b]
        last_exp = len(mn) - 1 - mn[::-1].index("v_ldexp_f64")
        assert sum(m.startswith("v_mfma_f64") for m in mn[last_exp:]) in (8, 16), mn[last_exp:]


def test_loop_entry_code_stays_small(forward_blocks):
    openings = [b for b in forward_blocks
                if sum(m == "global_load_lds_dwordx4" for m, _ in b) >= 18 and not any(m.startswith("v_mfma") for m, _ in b)]
    assert openings, "no three-tile opening block found"
    for b in openings:
        valu = [m for m, _ in b if m.startswith("v_")]
        print(f"opening block: {len(b)} instructions, {len(valu)} vector: {sorted(valu)}")
        assert len(valu) <= 8, valu
        assert sum(m.startswith("v_readlane") for m in valu) <= 4, valu
        assert sum(m.startswith("v_mov") for m in valu) <= 3, valu
    for b in forward_blocks:
        run = best = 0
        for m, ops in b:
            run = run + 1 if (m.startswith("v_mov_b") and ops.endswith(", 0")) else 0
            best = max(best, run)
        assert best < 8, (best, len(b))
    total = sum(m.startswith("v_readlane") for b in forward_blocks for m, _ in b)
    print("v_readlane_b32 in the kernel:", total)
    assert total <= READLANE_TOTAL, total
