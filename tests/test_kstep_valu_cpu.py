"""The k-steps of the asynchronous loop (csrc/device_common.hpp: TileGemm::rstep, loop_tri_async_w) issue no vector instruction but
their MFMAs - read from the gfx950 code of the BUILT product library, without a GPU.

On gfx950 an f64 MFMA never co-executes with VALU work, so every v_* instruction inside a k-step is time taken from the matrix pipe.
Until round 7 the loop took its LDS buffer index as a run-time value and rebuilt every LDS address of a step with vector adds:

    f64 64-point strips, per 32-MFMA regular step      11  (10 v_add_u32 + 1 v_readfirstlane_b32)
    f64 forward, the eight triangular tail steps       65  per eight steps
    f64 value-and-gradient, the same                   78  per eight steps
    fp32 128-point forward, regular step / tail        18 / 123

Bounds asserted here: a regular-step block 0; a triangular block (fewer MFMAs per step: the zero tiles are skipped) at most one
per step.

What is a block: a basic block of the kernel (leaders: branch targets and the instructions behind branches) that holds an s_barrier
and at least 24 MFMAs.  Behind its last MFMA such a block may run on into the caller's
epilogue (the loop's closing barrier and the address arithmetic of the stores sit in the same basic block as the last step when no
branch separates them): a block is counted up to its last MFMA, and what follows is no k-step."""
import os
import re
import subprocess
import tempfile

import pytest

from approxgp import _ffi

LLVM = "/opt/rocm/lib/llvm/bin"
TOOLS = [os.path.join(LLVM, t) for t in ("llvm-objdump", "clang-offload-bundler", "llvm-objcopy")]

# <T, NT, BK, NTHR, MINW, PAD, GRAD, BIGD, SEG>
F64_FORWARD = "strip_kernelIdLi64ELi16ELi256ELi2ELi16ELb0ELb0ELb0E"
F64_GRAD = "strip_kernelIdLi64ELi16ELi256ELi2ELi16ELb1ELb0ELb0E"
F32_FORWARD = "strip_kernelIfLi128ELi16ELi256ELi2ELi16ELb0ELb0ELb0E"


def _disassembly(lib_path):
    """llvm-objdump -d of every gfx950 code object bundled in the library (unbundled as tests/test_round4_cpu.py does)."""
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
def kernels():
    """name -> list of (address, mnemonic, branch target or None) of every strip kernel of the built product library."""
    if not os.path.exists(_ffi.LIB_PATH) or "experiments" in os.path.basename(_ffi.LIB_PATH) or not all(os.path.exists(t) for t in TOOLS):
        pytest.skip("needs the built product library and the ROCm llvm tools")
    found = {}
    head = re.compile(r"^([0-9a-f]{16}) <(\S+)>:$")
    ins = re.compile(r"^\s+(\S+)(.*?)//\s*([0-9A-Fa-f]{12}):(.*)$")
    for text in _disassembly(_ffi.LIB_PATH):
        name, start, cur = None, 0, None
        for line in text.splitlines():
            m = head.match(line)
            if m:
                start, name = int(m.group(1), 16), m.group(2)
                cur = found.setdefault(name, []) if "strip_kernel" in name else None
                continue
            if cur is None:
                continue
            m = ins.match(line)
            if not m:
                continue
            mnem, addr, tail = m.group(1), int(m.group(3), 16), m.group(4)
            target = None
            if mnem.startswith("s_cbranch") or mnem == "s_branch":
                t = re.search(r"<\S+\+0x([0-9a-fA-F]+)>", tail)
                assert t, line
                target = start + int(t.group(1), 16)
            cur.append((addr, mnem, target))
    return found


def _blocks(code):
    """Basic blocks of a kernel as lists of mnemonics."""
    leaders = {code[0][0]}
    for i, (addr, mnem, target) in enumerate(code):
        if target is not None or mnem in ("s_endpgm", "s_setpc_b64"):
            if target is not None:
                leaders.add(target)
            if i + 1 < len(code):
                leaders.add(code[i + 1][0])
    blocks, cur = [], []
    for addr, mnem, _ in code:
        if addr in leaders and cur:
            blocks.append(cur)
            cur = []
        cur.append(mnem)
    blocks.append(cur)
    return blocks


def _step_blocks(code, mfma, min_mfma):
    """(MFMAs, barriers up to the last MFMA, other v_* up to the last MFMA) of every block with an s_barrier and >= min_mfma MFMAs."""
    out = []
    for b in _blocks(code):
        n = sum(1 for m in b if m.startswith(mfma))
        if n < min_mfma or "s_barrier" not in b:
            continue
        last = max(i for i, m in enumerate(b) if m.startswith(mfma))
        body = b[:last + 1]
        valu = [m for m in body if m.startswith("v_") and not m.startswith("v_mfma_")]
        out.append((n, body.count("s_barrier"), valu))
    return out


def _find(kernels, tag):
    names = [n for n in kernels if tag in n]
    assert len(names) == 1, (tag, names)
    return kernels[names[0]]


def _check(code, mfma, per_step):
    """per_step: MFMAs of a full (regular) step.  Every step but a loop's last ends in one barrier, so a block of regular steps holds
    at least per_step MFMAs per barrier; a block with fewer holds written-out triangular steps (their zero tiles are skipped)."""
    blocks = _step_blocks(code, mfma, 24)
    assert blocks, "no k-step block found"
    for n, bars, valu in blocks:
        print(f"block: {n} MFMAs, {bars} barriers up to the last MFMA, other VALU {valu}")
    regular = [b for b in blocks if b[0] >= per_step * b[1]]
    triangular = [b for b in blocks if b[0] < per_step * b[1]]
    for n, bars, valu in regular:
        assert valu == [], (n, valu)                       # before round 7: 11 per step (fp32: 18)
    for n, bars, valu in triangular:
        assert len(valu) <= bars, (n, bars, valu)          # at most one per step; before round 7: 65 (forward) / 78 (gradient) per eight steps (fp32: 123)
    return regular, triangular


def test_f64_forward_strip_steps_issue_no_valu(kernels):
    regular, triangular = _check(_find(kernels, F64_FORWARD), "v_mfma_f64", 32)
    # phase 1's three-step trip, and the two written-out triangular runs (phase 1's tail: 160 MFMAs, phase 2's head: 90 + 30)
    assert any(n == 96 for n, _, _ in regular)
    assert len(triangular) >= 2


def test_f64_gradient_strip_steps_issue_no_valu(kernels):
    regular, triangular = _check(_find(kernels, F64_GRAD), "v_mfma_f64", 32)
    assert any(n == 96 for n, _, _ in regular)
    assert len(triangular) >= 1


def test_f32_forward_strip_steps_issue_no_valu(kernels):
    regular, triangular = _check(_find(kernels, F32_FORWARD), "v_mfma_f32", 64)
    assert any(n == 192 for n, _, _ in regular)
    assert len(triangular) >= 2
