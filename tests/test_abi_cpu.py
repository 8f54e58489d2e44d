"""The C-ABI library loads without a GPU and exports every symbol include/ckks_hip.h declares."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared():
    text = open(os.path.join(ROOT, "include", "ckks_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\bint(?:64_t)?\s+(lf(?:30)?_\w+)\s*\(", text)))


def test_every_declared_symbol_is_exported():
    from liberate_fhe_amd import _native
    names = declared()
    assert len(names) >= 19
    so = ctypes.CDLL(_native.LIB_PATH)
    for n in names:
        assert hasattr(so, n), f"{n} declared in include/ckks_hip.h but not exported"
    assert sorted(_native.EXPORTED) == names, "python binding table out of sync with the header"
    assert _native.lib.lf_abi_version() == 15     # pure host call, no HIP runtime use


def test_python_binding_passes_as_many_arguments_as_the_header_declares():
    """ctypes does not check arity against the library: a signature that drifts from include/ckks_hip.h would shift every
    following argument.  Parameter counts (and pointer / integer kind) of the binding table against the header."""
    from liberate_fhe_amd import _native
    text = open(os.path.join(ROOT, "include", "ckks_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, params in re.findall(r"\bint(?:64_t)?\s+(lf(?:30)?_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S):
        params = [p.strip() for p in params.split(",")] if params.strip() not in ("", "void") else []
        sig = _native._SIGNATURES[name]
        assert len(sig) == len(params), f"{name}: header has {len(params)} parameters, binding {len(sig)}"
        for i, (decl, ct) in enumerate(zip(params, sig)):
            is_ptr = "*" in decl
            bound_ptr = ct is ctypes.c_void_p or (isinstance(ct, type) and issubclass(ct, ctypes._Pointer))
            assert is_ptr == bound_ptr, f"{name} parameter {i} ({decl}): pointer-ness differs from the binding ({ct})"


def test_shim_exposes_the_fifteen_reference_functions():
    from liberate_fhe_amd.ntt import ntt_cuda
    expected = {"mont_mult", "mont_enter", "ntt", "enter_ntt", "intt", "mont_redc", "intt_exit", "intt_exit_reduce",
                "intt_exit_reduce_signed", "reduce_2q", "make_signed", "make_unsigned", "mont_add", "mont_sub",
                "tile_unsigned"}   # reference: src/liberate/ntt/ntt.cpp:421-437
    assert expected == set(ntt_cuda.__all__)
    for n in expected:
        assert callable(getattr(ntt_cuda, n))


def test_product_path_refuses_cpu_tensors():
    """No silent CPU fallback: the shim raises on host tensors."""
    import pytest
    import torch
    from liberate_fhe_amd.ntt import ntt_cuda
    t = torch.zeros((1, 8), dtype=torch.int64)
    with pytest.raises(RuntimeError):
        ntt_cuda.reduce_2q([t], [torch.zeros(1, dtype=torch.int64)])


def test_product_package_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "liberate_fhe_amd")
    for base, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                src = open(os.path.join(base, f)).read()
                assert "import oracle" not in src and "from oracle" not in src and "oracle/" not in src.replace("checker", ""), f


def test_every_include_and_every_source_file_is_part_of_the_library_digest():
    """build() rebuilds (and bench.py drops stamped profiles) when library_digest() changes: every file the library is
    compiled from must be in it — each #include "..." of csrc/ and each .hip / .h file that exists there."""
    import __graft_entry__ as g
    csrc = os.path.join(ROOT, "liberate_fhe_amd", "csrc")
    known = {os.path.realpath(p) for p in g.library_sources()}
    for f in os.listdir(csrc):
        if not f.endswith((".hip", ".h")):
            continue
        path = os.path.join(csrc, f)
        assert os.path.realpath(path) in known, f"{f} exists in csrc/ but is not a library source"
        for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(path).read(), flags=re.M):
            target = os.path.realpath(os.path.join(csrc, inc))
            assert os.path.exists(target), f"{f} includes {inc}: no such file"
            assert target in known, f"{f} includes {inc}, which library_sources() does not list"


def test_no_hip_file_declares_what_another_hip_file_defines():
    """What one .hip file of csrc/ defines and another uses is declared ONCE, in a header both include (csrc/ckks_launch.h, or
    include/ckks_hip.h for the exported entries): no .hip file carries a file-scope prototype or an `extern` declaration of a
    function or variable that another .hip file defines, so a signature cannot drift between a hand-copied prototype and the
    definition it links against."""
    csrc = os.path.join(ROOT, "liberate_fhe_amd", "csrc")
    text = {}
    for f in sorted(os.listdir(csrc)):
        if f.endswith(".hip"):
            src = open(os.path.join(csrc, f)).read()
            src = re.sub(r"/\*.*?\*/", lambda m: "\n" * m.group(0).count("\n"), src, flags=re.S)
            text[f] = re.sub(r"//[^\n]*", "", src)
    assert len(text) >= 7
    proto = re.compile(r"^(?!static\b|typedef\b|using\b|template\b)[A-Za-z_][\w \t]*[\s\*&]+(\w+)\s*\(([^;{}]*)\)\s*;", re.M)
    ext = re.compile(r"^extern\s+(?!\"C\")[^;=(]*?(\w+)\s*(?:\[[^\]]*\])?\s*;", re.M)
    seen = 0
    for f, src in text.items():
        for kind, names in (("prototype", [m.group(1) for m in proto.finditer(src)]), ("extern", ext.findall(src))):
            for name in names:
                seen += 1
                for g, other in text.items():
                    if g == f:
                        continue
                    body = re.search(rf"^[A-Za-z_][\w \t]*[\s\*&]+{name}\s*\([^;{{}}]*\)\s*{{", other, re.M)
                    var = re.search(rf"^(?!extern\b)[A-Za-z_][\w \t]*[\s\*&]+{name}\s*(?:\[[^\]]*\])?\s*(?:=[^;]*)?;", other, re.M)
                    assert not (body if kind == "prototype" else var), f"{f} declares {name} ({kind}), which {g} defines: declare it in a header"
    # the shared declarations exist, in the header both sides include
    header = open(os.path.join(csrc, "ckks_launch.h")).read()
    for name in ("lf_ks_tail_lt", "lf_fp64_digits_ok", "lf_g_intt_digits", "lf_g_ws_extra_stage"):
        assert re.search(rf"\b{name}\b", header), name
        users = [f for f, src in text.items() if re.search(rf"\b{name}\b", src)]
        assert len(users) >= 2, name
        for f in users:
            assert '#include "ckks_launch.h"' in text[f], (f, name)


def test_library_reads_no_environment_variables():
    """A drop-in library's results must not depend on ambient env vars: no getenv anywhere in the C sources."""
    csrc = os.path.join(ROOT, "liberate_fhe_amd", "csrc")
    for f in os.listdir(csrc):
        if f.endswith((".hip", ".h")):
            assert "getenv" not in open(os.path.join(csrc, f)).read(), f


def test_limits_are_exported_and_checked_by_the_engine():
    """lf_limits reports the capacities compiled into the fused kernels; the engine refuses a parameter set
    beyond them at construction (10 special primes: digits of 10 limbs > 8) instead of failing inside a launch."""
    import pytest
    from liberate_fhe_amd import _native
    from liberate_fhe_amd.fhe.backend import HipBackend
    from liberate_fhe_amd.fhe.presets import errors
    assert [_native.lib.lf_limits(i) for i in range(6)] == [8, 8, 250, 8, 24, -1]
    assert HipBackend.limits["special_primes"] == 8

    from liberate_fhe_amd.fhe import ckks_engine
    from tests.oracle_backend import OracleBackend
    ob = OracleBackend()
    ob.limits = HipBackend.limits
    with pytest.raises(errors.KernelLimitExceeded):
        ckks_engine(devices=["cpu"], backend=ob, logN=14, num_special_primes=10, num_scales=10, is_secured=False)


def test_the_advertised_limits_admit_the_edge_parameter_sets():
    """Exactly at the limits: 8 special primes with a digit of 8 limbs pass the engine's check (the kernels are run there by
    tests/test_engine_edges_gpu.py), 9 do not; every parameter set of that file passes."""
    import pytest
    from liberate_fhe_amd.fhe import ckks_engine
    from liberate_fhe_amd.fhe.backend import HipBackend
    from liberate_fhe_amd.fhe.presets import errors
    from tests.helpers import edge_param_sets
    from tests.oracle_backend import OracleBackend
    ob = OracleBackend()
    ob.limits = HipBackend.limits
    for name, params in edge_param_sets().items():
        eng = ckks_engine(devices=["cpu"], backend=ob, **params)
        assert eng.ntt.num_special_primes == params["num_special_primes"], name
    eng = ckks_engine(devices=["cpu"], backend=ob, **edge_param_sets()["sb45_K8"])
    assert max(len(part) for part in eng.ntt.p.p[0][0]) == 8 == HipBackend.limits["digit_limbs"]
    with pytest.raises(errors.KernelLimitExceeded):
        ckks_engine(devices=["cpu"], backend=ob, **dict(edge_param_sets()["sb40_K8"], num_special_primes=9, num_scales=10))


def test_unpickler_refuses_foreign_globals(tmp_path):
    """load() resolves only the container class and the tensor / array reconstructors."""
    import io
    import pickle
    import pytest
    from liberate_fhe_amd.fhe.evaluator import _PortableUnpickler

    class Evil:
        def __reduce__(self):
            return (os.system, ("true",))
    with pytest.raises(pickle.UnpicklingError):
        _PortableUnpickler(io.BytesIO(pickle.dumps(Evil()))).load()
    golden = os.path.join(ROOT, "tests", "golden", "reference_saved_ct.pkl")
    ct = _PortableUnpickler(open(golden, "rb")).load()   # a file the reference wrote still loads
    assert ct.origin == "cipher text"


def test_relaxed_transforms_need_table_and_host_primes():
    """LF_NTT_RELAXED with psi_dp == NULL or q_host == NULL is LF_ERR_ARG — refused from the arguments
    alone, before any device call (so it can be checked without a GPU) — and the Python Consts refuses the same."""
    import ctypes
    import numpy as np
    import pytest
    import torch
    from liberate_fhe_amd._native import lib
    from liberate_fhe_amd.fhe.backend import Consts
    dummy = ctypes.c_void_p(64)          # never dereferenced: every call below fails its argument check
    q = np.array([1099511922689], dtype=np.int64)
    for psi_dp, q_host in ((None, q.ctypes.data), (dummy, None), (None, None)):
        assert lib.lf_ntt(dummy, 1, 1, 13, dummy, psi_dp, q_host, None, 1, dummy, dummy, dummy, dummy, dummy, 0, None) == 10001
        assert lib.lf_intt(dummy, 1, 1, 13, dummy, psi_dp, q_host, dummy, 2, 1, dummy, dummy, dummy, dummy, dummy, 0, None) == 10001
        arr = (ctypes.c_void_p * 1)(64)
        assert lib.lf_rescale_ntt(arr, arr, 1, dummy, 1, 13, dummy, 0, dummy, psi_dp, q_host, None, 1, dummy, dummy, dummy,
                                  dummy, dummy, 0, None) == 10001
    assert lib.lf_intt(dummy, 1, 1, 13, dummy, dummy, q.ctypes.data, dummy, 1, 1, dummy, dummy, dummy, dummy, dummy, 0, None) == 10001
    z = torch.zeros(1, dtype=torch.int64)
    c = Consts.__new__(Consts)
    c._qptr = 0
    with pytest.raises(ValueError):
        c.qptr(relaxed=True)


def test_unpickler_accepts_what_the_reference_load_accepts(tmp_path):
    """Python complex, ndarrays pickled at protocols 2 and 5 inside a container still load."""
    import io
    import pickle
    import numpy as np
    import torch
    from liberate_fhe_amd.fhe.data_struct import data_struct
    from liberate_fhe_amd.fhe.evaluator import _PortableUnpickler
    payload = data_struct(data=[np.arange(6, dtype=np.int64).reshape(2, 3), 1.5 + 2j, torch.arange(4)], include_special=False,
                          ntt_state=False, montgomery_state=False, origin="cipher text", level=0, hash="h", version="v")
    for proto in (2, 4, 5):
        back = _PortableUnpickler(io.BytesIO(pickle.dumps(payload, protocol=proto))).load()
        assert (back.data[0] == payload.data[0]).all() and back.data[1] == 1.5 + 2j and torch.equal(back.data[2], payload.data[2])


def test_lf_tune_is_a_pure_host_call():
    """Launch-shape thresholds: read, set, restore, unknown knob -> -1; no device is touched."""
    from liberate_fhe_amd._native import lib
    assert lib.lf_tune(0, -1) == -1     # the round-3 one-launch knob is gone
    cols = lib.lf_tune(1, -1)
    assert 0 <= cols <= 5
    assert lib.lf_tune(1, 9) == cols and lib.lf_tune(1, -1) == cols      # out of range: ignored
    assert lib.lf_tune(3, -1) == 1 and lib.lf_tune(3, 5) == 1     # digit planes: on by default; out of range: ignored
    assert lib.lf_tune(4, -1) == 1 and lib.lf_tune(4, 7) == 1     # extra column stage of lf_ntt_ws: on; out of range: ignored
    assert lib.lf_tune(5, -1) == 3 and lib.lf_tune(5, 9) == 3     # planes for the sums (bit 0) and the operand stack (bit 1): on
    assert lib.lf_tune(77, 1) == -1


def test_stack_planes_query_follows_the_primes_and_the_knobs():
    """lf_stack_planes (pure host): internal stacks keep fp64-class rows as 6-byte planes at two-pass ring degrees when the rows
    hold primes of BOTH classes and lf_tune's LF_TUNE_DIGIT_PLANES / LF_TUNE_MORE_PLANES (bit 1) say so."""
    import numpy as np
    from liberate_fhe_amd._native import lib
    small, large = (1 << 40) + 12345, (1 << 60) - 93
    mixed = np.array([small, small + 2, large], dtype=np.int64)
    only_small = np.array([small, small + 2], dtype=np.int64)
    only_large = np.array([large], dtype=np.int64)
    q = lambda a: a.ctypes.data
    assert lib.lf_stack_planes(16, 3, q(mixed)) == 1 and lib.lf_stack_planes(13, 3, q(mixed)) == 1
    assert lib.lf_stack_planes(12, 3, q(mixed)) == 0                      # one-pass ring degree: no stack crosses HBM twice
    assert lib.lf_stack_planes(16, 2, q(mixed)) == 0                      # the first two rows only: one class
    assert lib.lf_stack_planes(16, 2, q(only_small)) == 0 and lib.lf_stack_planes(16, 1, q(only_large)) == 0
    assert lib.lf_stack_planes(16, 3, None) == 0
    try:
        lib.lf_tune(5, 1)
        assert lib.lf_stack_planes(16, 3, q(mixed)) == 0
        lib.lf_tune(5, 3)
        lib.lf_tune(3, 0)
        assert lib.lf_stack_planes(16, 3, q(mixed)) == 0
    finally:
        lib.lf_tune(3, 1)
        lib.lf_tune(5, 3)
    assert lib.lf_stack_planes(16, 3, q(mixed)) == 1
    # only where lf_rescale_ntt accepts LF_NTT_PLANES: a column pass of at most 5 stages (logN <= 17)
    assert lib.lf_stack_planes(17, 3, q(mixed)) == 1
    for logN in range(18, lib.lf_limits(4) + 1):
        assert lib.lf_stack_planes(logN, 3, q(mixed)) == 0, logN
    assert lib.lf_stack_planes(lib.lf_limits(4) + 1, 3, q(mixed)) == 0


def test_engine_ops_and_key_switch_refuse_ring_degrees_above_17():
    """The key switch and the engine ops built on it run at 13 <= logN <= 17 (csrc/ckks_common.h KS_LOGN_MAX: the extension
    pass moves words in neighbouring pairs, and cc_mult's stack planes need a column pass of at most 5 stages).  At logN 18 ..
    24 — ring degrees lf_ntt does accept — every such entry returns LF_ERR_ARG from its arguments alone, before anything is
    launched: checked here without a GPU, on pointers that are never dereferenced (a plan with every pointer non-null and
    consistent counts, so that only its logN can fail the check; no call here is one that would pass it)."""
    import ctypes
    import numpy as np
    from liberate_fhe_amd._native import lib, KsPlan
    LF_ERR_ARG = 10001
    assert lib.lf_limits(4) == 24
    dummy = ctypes.c_void_p(64)
    arr = (ctypes.c_void_p * 4)(64, 64, 64, 64)
    q_host = np.array([(1 << 41) - 65535, (1 << 60) - 93, (1 << 60) - 173], dtype=np.int64)
    ell, K = 2, 1
    for logN in (18, 20, 24):
        plan = KsPlan()
        plan.logN, plan.ell, plan.K, plan.nparts, plan.dig_nparts, plan.max_nct = logN, ell, K, 2, 2, 4
        for name, typ in KsPlan._fields_:
            if typ is ctypes.c_void_p:
                setattr(plan, name, 64)
        plan.q_host = q_host.ctypes.data
        assert all(getattr(plan, n) for n, t in KsPlan._fields_ if t is ctypes.c_void_p)
        p = ctypes.byref(plan)
        assert lib.lf_cc_mult_evk(p, arr, arr, dummy, 0, 0, 0, 0, dummy, dummy, None) == LF_ERR_ARG, logN
        assert lib.lf_cc_mult_evk_batch(p, 2, arr, arr, dummy, 0, 0, 0, 0, arr, arr, None) == LF_ERR_ARG, logN
        assert lib.lf_cc_mult_evk_pre(p, arr, arr, 3, None) == LF_ERR_ARG, logN
        assert lib.lf_cc_mult_evk_post(p, dummy, 0, 0, 0, 0, dummy, dummy, 3, None) == LF_ERR_ARG, logN
        assert lib.lf_switch_key(p, dummy, dummy, 0, 0, dummy, 0, 0, 0, 0, dummy, dummy, None) == LF_ERR_ARG, logN
        assert lib.lf_switch_key_batch(p, 2, arr, arr, 0, 0, dummy, 0, 0, 0, 0, arr, arr, None) == LF_ERR_ARG, logN
        assert lib.lf_switch_key_pre(p, dummy, 0, 0, None) == LF_ERR_ARG, logN
        assert lib.lf_switch_key_post(p, dummy, 0, 0, dummy, 0, 0, 0, 0, dummy, dummy, 3, None) == LF_ERR_ARG, logN
        assert lib.lf_ks_plan_fwd(p, dummy, 0, 1, 1, None) == LF_ERR_ARG, logN
        # the key switch's own entries
        rows, qh = ell + K, q_host.ctypes.data
        assert lib.lf_ks_fwd(dummy, 1, rows, logN, dummy, dummy, dummy, dummy, dummy, dummy, qh, dummy, dummy, dummy, dummy,
                             0, None) == LF_ERR_ARG, logN
        assert lib.lf_ks_tail(1, rows, logN, dummy, 0, 0, 0, 0, dummy, dummy, dummy, dummy, dummy, qh, dummy, dummy, dummy,
                              dummy, 0, None) == LF_ERR_ARG, logN
        assert lib.lf_ks_core(dummy, 1, rows, logN, dummy, dummy, dummy, dummy, 0, 0, 0, 0, dummy, dummy, dummy, dummy, dummy,
                              dummy, dummy, qh, dummy, dummy, dummy, dummy, 0, None) == LF_ERR_ARG, logN
        assert lib.lf_ks_core_batch(dummy, 0, 1, 1, rows, logN, dummy, dummy, dummy, dummy, 0, 0, 0, 0, dummy, dummy, dummy,
                                    dummy, dummy, dummy, dummy, qh, dummy, dummy, dummy, dummy, 0, None) == LF_ERR_ARG, logN
        assert lib.lf_relin_fwd(dummy, 0, 1, rows, logN, dummy, dummy, dummy, dummy, dummy, dummy, dummy, qh, dummy, dummy,
                                dummy, dummy, 0, None) == LF_ERR_ARG, logN
        assert lib.lf_relin_tail(1, rows, logN, dummy, 0, 0, 0, 0, dummy, dummy, dummy, dummy, dummy, dummy, dummy, ell,
                                 dummy, qh, dummy, dummy, dummy, dummy, 0, None) == LF_ERR_ARG, logN
        assert lib.lf_relin_core_batch(dummy, 0, 1, 1, rows, logN, dummy, dummy, dummy, dummy, 0, 0, 0, 0, dummy, dummy,
                                       dummy, dummy, dummy, dummy, dummy, dummy, 0, dummy, ell, dummy, qh, dummy, dummy, dummy,
                                       dummy, 0, None) == LF_ERR_ARG, logN


def test_clock_probe_checks_its_arguments_on_the_host():
    """lf_clock_probe (measurement entry): bad arguments are refused before any HIP call."""
    from liberate_fhe_amd._native import lib
    assert lib.lf_clock_probe(None, 4, 1000, 0, None) != 0
    assert lib.lf_clock_probe(8, 0, 1000, 0, None) != 0
    assert lib.lf_clock_probe(8, 4, 0, 0, None) != 0
    assert lib.lf_clock_probe(8, 4096, 1_000_000, 0, None) != 0           # more than ten seconds of spinning


def test_bench_refuses_more_ranks_than_gpus_without_touching_one():
    """`python bench.py --gpus N` with no launcher around it starts its own ranks — after counting the GPUs WITHOUT
    initialising one; on a box with fewer than N it says so and exits 2 (no rank is started, nothing hangs)."""
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LF_BENCH_REHEARSE")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "64", "--steps", "1", "--warmup", "0"],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "GPU(s)" in r.stderr and r.stdout.strip() == ""


def test_hot_kernels_use_no_scratch_memory_and_the_tracked_table_is_current():
    """The design argues from register counts and occupancies: they come from the compiler's own
    kernel-resource-usage remarks of the objects the library is linked from (__graft_entry__.kernel_resources()) and are tracked as
    profiles/r06_kernel_resources.txt.  Held here: no stack object and no spill (scratch = 0 bytes per lane) in the kernels
    every preset's hot path launches — the column passes, the 16-words-per-thread tiled passes, the key switch's extension,
    inner product and digit kernels (a 16-byte struct selected between registers and global memory once put 48 .. 128 bytes per
    lane of ks_inner2_kernel<2 | 4, fold> into scratch; a rolled loop 272 bytes of ntt_inv_cols_digits) — and the occupancies the
    launch shapes were chosen for."""
    import re
    import __graft_entry__ as g
    rows = g.kernel_resources()
    assert len(rows) > 100
    by = {}
    for r in rows:
        by.setdefault(r["kernel"], []).append(r)
    hot = re.compile(r"^(ntt_fwd_cols_ws<|ntt_fwd_cols_mixed|ntt_inv_cols_mixed<|ntt_inv_cols_ws<|ntt_inv_cols_digits<|ntt_pass16|"
                     r"ks_ext_cols_mixed<|ks_inner2_kernel<|ks_digits_kernel|ks_moddown|ks_pivots|ew_kernel<|galois_kernel)")
    seen = [k for k in by if hot.match(k)]
    for need in ("ntt_fwd_cols_ws<5>", "ntt_pass16_fwd_seq_ws<true>", "ntt_pass16_fwd_seq_ws<false>", "ntt_pass16_fwd_planes",
                 "ks_ext_cols_mixed<4>", "ks_inner2_kernel<1, true, true, true>", "ks_inner2_kernel<4, true, true, true>"):
        assert need in by, (need, sorted(seen)[:20])
    bad = {k: [(r["file"], r["scratch"], r["vgpr_spill"]) for r in by[k]] for k in seen if any(r["scratch"] or r["vgpr_spill"] for r in by[k])}   # (SGPR spills go to VGPR lanes, not to memory)
    assert not bad, bad
    # what the launch shapes rest on: 4 tiles of 34 KiB LDS per CU for the tiled passes, 3 waves per SIMD for the five-stage column pass
    for k in seen:
        if k.startswith("ntt_pass16"):
            assert all(r["occupancy"] >= 4 and r["lds"] <= 40960 for r in by[k]), (k, by[k])
    assert all(r["occupancy"] >= 3 for r in by["ntt_fwd_cols_ws<5>"])
    assert all(r["occupancy"] >= 4 for r in by["ks_inner2_kernel<4, true, true, true>"])
    # the only kernels with scratch at all are the 8-words tiled passes (logN <= 12 / in-place logN 17), capped at 80 VGPRs for 6 waves
    allowed = re.compile(r"^(ntt_fwd_pass<|ntt_inv_pass_io<|ntt_inv_pass_mixed<)")
    other = sorted({r["kernel"] for r in rows if r["scratch"] and not allowed.match(r["kernel"])})
    assert not other, other
    assert max(r["scratch"] for r in rows) <= 64
    # the tracked table is the current build's (tools/kernel_resources.py writes it)
    path = os.path.join(ROOT, "profiles", "r06_kernel_resources.txt")
    tracked = {}
    for ln in open(path):
        if ln.startswith("#") or ln.startswith("file "):
            continue
        f = ln.split()
        tracked.setdefault(" ".join(f[1:-7]), set()).add((int(f[-7]), int(f[-3]), int(f[-1])))      # VGPR, scratch, occupancy
    stale = {k: (sorted(tracked.get(k, [])), sorted({(r["vgprs"], r["scratch"], r["occupancy"]) for r in by[k]})) for k in seen
             if len(k) <= 57 and tracked.get(k) != {(r["vgprs"], r["scratch"], r["occupancy"]) for r in by[k]}}
    assert not stale, f"profiles/r06_kernel_resources.txt is stale (python tools/kernel_resources.py r06): {stale}"


def test_stack_planes_class_split_at_two_to_the_41():
    """The library splits the arithmetic classes at SMALL_PRIME_LIMIT = 2^41 exactly where the engine's Python does
    (q >= 2^41: integer class): 2^41 - 65535 is fp64 class, 2^41 + 311297 integer class, on either side of a 60-bit prime."""
    import numpy as np
    from liberate_fhe_amd._native import lib
    from tests.helpers import SMALL_PRIME_LIMIT
    top, bottom, low2, p60 = (1 << 41) - 65535, (1 << 41) + 311297, (1 << 41) - 901119, 1152921504606830593
    q = lambda *v: np.array(v, dtype=np.int64)
    for logN in (13, 14, 16):
        assert lib.lf_stack_planes(logN, 2, q(top, p60).ctypes.data) == 1
        assert lib.lf_stack_planes(logN, 2, q(p60, top).ctypes.data) == 1
        assert lib.lf_stack_planes(logN, 2, q(bottom, p60).ctypes.data) == 0         # both integer class
        assert lib.lf_stack_planes(logN, 2, q(top, low2).ctypes.data) == 0           # both fp64 class
        assert lib.lf_stack_planes(logN, 2, q(top, bottom).ctypes.data) == 1
        assert lib.lf_stack_planes(logN, 2, q(SMALL_PRIME_LIMIT - 1, SMALL_PRIME_LIMIT).ctypes.data) == 1
        assert lib.lf_stack_planes(logN, 2, q(SMALL_PRIME_LIMIT, SMALL_PRIME_LIMIT + 1).ctypes.data) == 0
    assert top < SMALL_PRIME_LIMIT <= bottom and SMALL_PRIME_LIMIT == 1 << 41


def test_edge_primes_sit_at_the_class_edges_and_interleave():
    """tests/helpers.py:pick_edge_primes: NTT primes for the ring, the top of the fp64 class alternating with the bottom of
    the integer class (nothing of either class between them and 2^41), then a ~2^20 prime and a 60-bit one."""
    from liberate_fhe_amd.fhe.context import primes as P
    from tests.helpers import SMALL_PRIME_LIMIT, pick_edge_primes
    for logN in (12, 13, 14, 16, 17):
        M = 2 << logN
        got = pick_edge_primes(logN)
        assert len(set(got)) == len(got) == 6 and all((x - 1) % M == 0 and P.is_prime(x) for x in got)
        assert got[0] == P.next_ntt_prime(SMALL_PRIME_LIMIT - 1, M, up=False)
        assert got[1] == P.next_ntt_prime(SMALL_PRIME_LIMIT + 1, M, up=True)
        assert [x < SMALL_PRIME_LIMIT for x in got[:4]] == [True, False, True, False]
        assert got[2] < got[0] < SMALL_PRIME_LIMIT < got[1] < got[3]
        assert got[4] == P.next_ntt_prime((1 << 20) + 1, M, up=True) < (1 << 23) and (1 << 59) < got[5] < (1 << 60)
    assert pick_edge_primes(13)[0] == pick_edge_primes(14)[0] == (1 << 41) - 65535
