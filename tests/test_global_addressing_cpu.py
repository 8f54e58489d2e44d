"""The hot kernels address device memory with GLOBAL instructions, not FLAT ones.

uniform_ptr() / uniform_at() (ckks_ntt_core.h) pin a wave-uniform row pointer in an SGPR pair through an empty asm.  An opaque
generic pointer has no address space the compiler knows: every access through it was a flat_* instruction with a 64-bit
per-lane address built by a VALU add, counted on lgkmcnt as well as on vmcnt (so that every LDS wait also waited for the tile
loads in flight).  The helpers now hand the pointer through the asm as an address-space-1 pointer.  Held here, on the gfx950
code objects of the built libckks_hip.so, disassembled by the toolchain's own llvm-objdump: no instruction whose mnemonic
starts with flat_ in the headline kernels of lf_ntt_ws, nor in the rest of the hot set tests/test_abi_cpu.py names."""
import glob
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HEADLINE = ["ntt_pass16_fwd_seq_ws<true>", "ntt_pass16_fwd_seq_ws<false>", "ntt_pass16_fwd_ws<true>", "ntt_pass16_fwd_ws<false>"] + \
           [f"ntt_fwd_cols_ws<{k}>" for k in range(1, 6)]
# the hot set of tests/test_abi_cpu.py::test_hot_kernels_use_no_scratch_memory_and_the_tracked_table_is_current
HOT = re.compile(r"^(ntt_fwd_cols_ws<|ntt_fwd_cols_mixed|ntt_inv_cols_mixed<|ntt_inv_cols_ws<|ntt_inv_cols_digits<|ntt_pass16|"
                 r"ks_ext_cols_mixed<|ks_inner2_kernel<|ks_digits_kernel|ks_moddown|ks_pivots|ew_kernel<|galois_kernel)")
# kernel -> why a FLAT access may stay (an address space that cannot be known: a pointer selected between LDS and global memory).
# Empty: no hot kernel has such a place.
ALLOWED_FLAT = {}


def _objdump():
    import __graft_entry__ as g
    return os.path.join(os.path.dirname(os.path.dirname(g.HIPCC)), "lib", "llvm", "bin", "llvm-objdump")


def _kernel_name(demangled):
    n = re.sub(r"^void ", "", demangled.replace("(anonymous namespace)::", ""))
    depth = 0
    for i, ch in enumerate(n):      # cut the parameter list: the first '(' outside the template arguments
        depth += (ch == "<") - (ch == ">")
        if ch == "(" and depth == 0:
            return n[:i]
    return n


@pytest.fixture(scope="module")
def flat_by_kernel(tmp_path_factory):
    """{kernel: [flat_* instruction lines]} of every hot kernel in the library's gfx950 code objects."""
    import __graft_entry__ as g
    tool = _objdump()
    if not os.path.exists(tool):
        pytest.skip(f"no disassembler at {tool}")
    g.build()
    work = str(tmp_path_factory.mktemp("isa"))
    shutil.copy(g.HIP_LIB, os.path.join(work, "lib.so"))
    subprocess.run([tool, "--offloading", "lib.so"], cwd=work, check=True, capture_output=True)      # one code object per translation unit
    objs = sorted(glob.glob(os.path.join(work, "lib.so.*gfx950")))
    assert objs, os.listdir(work)
    found = {}
    for co in objs:
        def functions(*flag):       # names of the function symbols, in symbol-table order
            text = subprocess.run([tool, "-t", *flag, co], check=True, capture_output=True, text=True).stdout
            rows = [re.match(r"^[0-9a-f]+\s+\S+\s+F\s+\S+\s+[0-9a-f]+\s+(?:\.(?:protected|hidden|internal)\s+)?(.*)$", ln) for ln in text.split("\n")]
            return [m.group(1).strip() for m in rows if m]
        mangled, demangled = functions(), functions("--demangle")
        assert len(mangled) == len(demangled)
        want = {m: _kernel_name(d) for m, d in zip(mangled, demangled) if HOT.match(_kernel_name(d))}      # mangled -> kernel
        if not want:
            continue
        out = subprocess.run([tool, "-d", "--no-show-raw-insn", "--disassemble-symbols=" + ",".join(want), co],
                             check=True, capture_output=True, text=True).stdout
        cur = None
        for ln in out.split("\n"):
            m = re.match(r"^[0-9a-f]+ <(.*)>:$", ln)
            if m:
                cur = want.get(m.group(1))
                if cur is not None:
                    found.setdefault(cur, [])
                continue
            f = ln.split()
            if cur is not None and f and f[0].startswith("flat_"):
                found[cur].append(" ".join(f))
    return found


def test_headline_kernels_hold_no_flat_instruction(flat_by_kernel):
    for k in HEADLINE:
        assert k in flat_by_kernel, (k, sorted(flat_by_kernel)[:10])
        assert not flat_by_kernel[k], (k, len(flat_by_kernel[k]), flat_by_kernel[k][:4])


def test_hot_set_holds_no_flat_instruction(flat_by_kernel):
    assert len(flat_by_kernel) > 60, sorted(flat_by_kernel)
    for need in ("ntt_pass16_fwd_planes", "ntt_pass16_inv_ws", "ntt_inv_cols_ws<5>", "ks_ext_cols_mixed<4>", "ks_inner2_kernel<4, true, true, true>",
                 "ks_digits_kernel", "galois_kernel"):
        assert need in flat_by_kernel, need
    bad = {k: (len(v), v[:3]) for k, v in flat_by_kernel.items() if v and k not in ALLOWED_FLAT}
    assert not bad, bad
    unused = [k for k in ALLOWED_FLAT if not flat_by_kernel.get(k)]
    assert not unused, f"allow-list entries without a FLAT instruction left: {unused}"
