"""cc_matmul (ckks_engine.cc_matmul, lf_cc_matmul: a matrix of ciphertexts times a matrix of ciphertexts, every distinct operand
transformed once) without a GPU: the pure planner, the engine's host logic on the checker backend against cc_dot of every
output's pairs, the refusals, the decryption error with real keys, the C entry's argument checks, the ABI and the new kernel's
resources."""
import ctypes
import os
import re

import numpy as np
import pytest

from liberate_fhe_amd.fhe import encdec
from liberate_fhe_amd.utils import synth
from tests.test_cc_dot_cpu import _fake_plan, lazy_ciphertext, same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LF_ERR_ARG = 10001


def engine_of(logN, num_scales=5):
    from liberate_fhe_amd.fhe import ckks_engine
    from tests.oracle_backend import OracleBackend
    return ckks_engine(devices=["cpu"], backend=OracleBackend(), logN=logN, num_scales=num_scales, num_special_primes=2, is_secured=False)


@pytest.fixture(scope="module", params=[12, 13])
def checker(request):
    return engine_of(request.param)


def definition(eng, A, B, evk):
    """C[i][j] = cc_dot of the pairs (A[i][t], B[t][j]) where neither is None"""
    return [[eng.cc_dot([(A[i][t], B[t][j]) for t in range(len(B)) if A[i][t] is not None and B[t][j] is not None], evk)
             for j in range(len(B[0]))] for i in range(len(A))]


def all_same(got, want):
    return len(got) == len(want) and all(len(g) == len(w) and all(same(x, y) for x, y in zip(g, w)) for g, w in zip(got, want))


# ---- the planner -------------------------------------------------------------------------------------------------------------
def test_limits_are_the_headers():
    from liberate_fhe_amd import _native
    text = open(os.path.join(ROOT, "include", "ckks_hip.h")).read()
    for name, copies in (("LF_CC_MATMUL_MAX_INNER", (encdec.CC_MATMUL_MAX_INNER, _native.LF_CC_MATMUL_MAX_INNER)),
                         ("LF_CC_MATMUL_MAX_OPERANDS", (encdec.CC_MATMUL_MAX_OPERANDS, _native.LF_CC_MATMUL_MAX_OPERANDS))):
        value = int(re.search(rf"#define {name} (\d+)", text).group(1))
        assert all(c == value for c in copies), name
    assert (encdec.CC_MATMUL_MAX_INNER, encdec.CC_MATMUL_MAX_OPERANDS) == (64, 256)


def test_planner_finds_distinct_operands_by_identity():
    a, b, c, d = (object() for _ in range(4))
    A = [[a, b], [c, a]]                                    # a repeats inside A
    m, k, n, calls = encdec.cc_matmul_plan(A, A)
    assert (m, k, n) == (2, 2, 2) and len(calls) == 1
    call = calls[0]
    assert call["rows"] == (0, 2) and [id(x) for x in call["operands"]] == [id(a), id(b), id(c)]
    assert call["ia"] == [0, 1, 2, 0] and call["ib"] == [0, 1, 2, 0]
    # equal but not identical objects are two operands; None maps to -1 and is no operand
    x, y = [1], [1]
    m, k, n, calls = encdec.cc_matmul_plan([[x, None, y]], [[x], [d], [None]])
    assert (m, k, n) == (1, 3, 1) and len(calls[0]["operands"]) == 3
    assert calls[0]["ia"] == [0, -1, 1] and calls[0]["ib"] == [0, 2, -1]
    # any iterables of rows
    m, k, n, calls = encdec.cc_matmul_plan(iter([iter([a, b])]), ((a,), (b,)))
    assert (m, k, n) == (1, 2, 1) and calls[0]["ia"] == [0, 1] and calls[0]["ib"] == [0, 1]


@pytest.mark.parametrize("m,n", [(1, 1), (2, 2), (3, 3), (1, 5), (5, 1), (3, 2), (2, 3), (5, 5), (1, 4), (4, 1), (4, 4), (7, 6)])
@pytest.mark.parametrize("gmax", [1, 2, 4])
def test_tiling_covers_every_output_once(m, n, gmax):
    tiles = encdec.cc_matmul_tiles(m, n, gmax)
    seen = {}
    for i0, j0, R, C in tiles:
        assert R * C in (4, 2, 1) and R * C <= gmax and (R, C) in ((2, 2), (1, 4), (4, 1), (1, 2), (2, 1), (1, 1))
        for i in range(i0, i0 + R):
            for j in range(j0, j0 + C):
                assert 0 <= i < m and 0 <= j < n and (i, j) not in seen
                seen[(i, j)] = (R, C)
    assert len(seen) == m * n


def test_tiling_shapes():
    t = encdec.cc_matmul_tiles
    assert t(1, 1) == [(0, 0, 1, 1)]
    assert t(2, 2) == [(0, 0, 2, 2)]
    assert sorted((R, C) for _, _, R, C in t(3, 3)) == [(1, 1), (1, 2), (2, 1), (2, 2)]        # one shape, all four tile sizes
    assert t(1, 5) == [(0, 0, 1, 4), (0, 4, 1, 1)] and t(5, 1) == [(0, 0, 4, 1), (4, 0, 1, 1)]
    assert t(3, 2) == [(0, 0, 2, 2), (2, 0, 1, 2)]
    assert t(2, 3) == [(0, 0, 2, 2), (0, 2, 2, 1)]
    assert t(2, 2, 2) == [(0, 0, 1, 2), (1, 0, 1, 2)] and t(2, 2, 1) == [(i, j, 1, 1) for i in range(2) for j in range(2)]
    with pytest.raises(ValueError):
        t(0, 1)


def test_planner_splits_by_row_blocks_beyond_the_operand_limit():
    k = 4
    A = [[object() for _ in range(k)] for _ in range(5)]
    B = [[A[0][t]] for t in range(k)]                       # B shares row 0's objects: 20 distinct operands in all
    m, k_, n, calls = encdec.cc_matmul_plan(A, B, max_operands=12)
    assert (m, k_, n) == (5, 4, 1)
    assert [c["rows"] for c in calls] == [(0, 3), (3, 5)]   # 12 operands, then B's 4 + 8
    assert [len(c["operands"]) for c in calls] == [12, 12]
    for c in calls:
        i0, i1 = c["rows"]
        assert len(c["ia"]) == (i1 - i0) * k and len(c["ib"]) == k
        assert [c["operands"][u] for u in c["ia"]] == [x for row in A[i0:i1] for x in row]
        assert [c["operands"][u] for u in c["ib"]] == [row[0] for row in B]
        assert sorted(set(c["ia"]) | set(c["ib"])) == list(range(len(c["operands"])))          # no operand unused
    assert len(encdec.cc_matmul_plan(A, B)[3]) == 1
    # B with one row of A above the limit, or an inner dimension above its own: no native call takes it
    assert encdec.cc_matmul_plan(A, B, max_operands=7)[3] is None
    assert encdec.cc_matmul_plan(A, B, max_inner=3)[3] is None
    wide = [[object() for _ in range(encdec.CC_MATMUL_MAX_INNER + 1)]]
    assert encdec.cc_matmul_plan(wide, [[x] for x in wide[0]])[3] is None


def test_planner_refuses_bad_shapes():
    a = object()
    for A, B in (([], [[a]]), ([[a]], []), ([[]], [[a]]), ([[a]], [[]]),                      # an empty matrix
                 ([[a, a], [a]], [[a], [a]]), ([[a, a]], [[a, a], [a]]),                        # ragged rows
                 ([[a, a]], [[a]]), ([[a]], [[a], [a]]),                                        # mismatched inner dimensions
                 ([[None]], [[a]]), ([[a, None], [None, a]], [[a, None], [a, a]])):             # an output with no term
        with pytest.raises(ValueError):
            encdec.cc_matmul_plan(A, B)


# ---- the engine on the checker backend ------------------------------------------------------------------------------------------
def matrices(eng, level, shape, seed=50):
    m, k, n = shape
    cts = [(lazy_ciphertext if i % 3 == 0 else synth.ciphertext)(eng, seed + i, level) for i in range(m * k + k * n)]
    A = [[cts[i * k + t] for t in range(k)] for i in range(m)]
    B = [[cts[m * k + t * n + j] for j in range(n)] for t in range(k)]
    return A, B


def test_cc_matmul_equals_cc_dot_of_every_output(checker):
    from liberate_fhe_amd.fhe.presets import types
    eng = checker
    evk = synth.key_switch_key(eng, 77)
    for level in (0, 2, eng.num_levels - 2):
        A, B = matrices(eng, level, (1, 1, 1))
        got = eng.cc_matmul(A, B, evk)
        assert all_same(got, definition(eng, A, B, evk)) and same(got[0][0], eng.cc_mult(A[0][0], B[0][0], evk))
        for shape in ((2, 2, 2), (1, 5, 4)):
            A, B = matrices(eng, level, shape)
            got = eng.cc_matmul(A, B, evk)
            assert len(got) == shape[0] and all(len(r) == shape[2] for r in got)
            assert all(c.level == level + 1 and c.origin == types.origins["ct"] and not c.ntt_state and not c.include_special
                       for r in got for c in r)
            assert all_same(got, definition(eng, A, B, evk)), (level, shape)
        A, B = matrices(eng, level, (3, 3, 3))
        A[1][2] = None
        B[0][1] = None
        assert all_same(eng.cc_matmul(A, B, evk), definition(eng, A, B, evk)), level
        A, _ = matrices(eng, level, (2, 2, 2))
        A[1][1] = A[0][0]
        assert all_same(eng.cc_matmul(A, A, evk), definition(eng, A, A, evk)), level
    assert all_same(eng.cc_matmul(iter([iter(A[0])]), ((A[0][0],), (A[1][0],)), evk), definition(eng, [A[0]], [[A[0][0]], [A[1][0]]], evk))


def test_cc_matmul_refusals(checker):
    from liberate_fhe_amd.fhe.presets import errors
    eng = checker
    evk = synth.key_switch_key(eng, 77)
    top = eng.num_levels - 1
    a0, b0, a1, atop = (synth.ciphertext(eng, 60 + i, lvl) for i, lvl in enumerate((0, 0, 1, top)))
    trip = eng.cc_mult(a0, b0, evk, relin=False)
    ntt = eng._new(a0.data, a0.origin, level=0, ntt_state=True)
    special = eng._new(a0.data, a0.origin, level=0, include_special=True)
    for exc, A, B in [(ValueError, [], [[a0]]), (ValueError, [[a0]], [[]]),                                   # an empty matrix
                      (ValueError, [[a0, b0], [a0]], [[a0], [b0]]), (ValueError, [[a0, b0]], [[a0, b0], [a0]]),   # ragged rows
                      (ValueError, [[a0, b0]], [[a0]]), (ValueError, [[a0]], [[a0], [b0]]),                      # inner dimensions
                      (ValueError, [[a0, None]], [[None], [b0]]), (ValueError, [[None]], [[None]]),              # an output with no term
                      (errors.NotMatchType, [[a0, trip]], [[a0], [b0]]), (errors.NotMatchType, [[a0]], [[evk]]),
                      (errors.NotMatchDataStructState, [[a0, b0]], [[a0], [a1]]),                                # one level
                      (errors.NotMatchDataStructState, [[a0], [a1]], [[b0]]),                                    # .. across outputs too
                      (errors.MaximumLevelError, [[atop]], [[atop]]),
                      (errors.NotMatchDataStructState, [[a0]], [[ntt]]), (errors.NotMatchDataStructState, [[special]], [[b0]])]:
        with pytest.raises(exc):
            eng.cc_matmul(A, B, evk)
    assert same(eng.cc_matmul([[a0]], [[b0]], evk)[0][0], eng.cc_mult(a0, b0, evk))      # and the engine still works


def test_real_keys_decrypt_within_twice_the_loop_of_cc_dot():
    """Real keys on the checker engine, 2 x 3 x 2 over fixed random messages in [-1, 1]: every C[i][j] decrypts to the slot-wise
    sum_t a_it b_tj with a maximum error of at most 2 x that of the loop of cc_dot on the same ciphertexts (the margin this
    project uses for such comparisons; here both are one relinearisation per output)."""
    eng = engine_of(13)
    sk = eng.create_secret_key()
    pk, evk = eng.create_public_key(sk), eng.create_evk(sk)
    rng = np.random.default_rng(13)
    ns = eng.num_slots
    ma, mb = rng.uniform(-1, 1, (2, 3, ns)), rng.uniform(-1, 1, (3, 2, ns))
    A = [[eng.encorypt(ma[i, t], pk) for t in range(3)] for i in range(2)]
    B = [[eng.encorypt(mb[t, j], pk) for j in range(2)] for t in range(3)]
    want = np.einsum("its,tjs->ijs", ma, mb)                            # numpy matmul, slot by slot
    got, loop = eng.cc_matmul(A, B, evk), definition(eng, A, B, evk)
    err = lambda C: max(np.abs(eng.decrode(C[i][j], sk) - want[i, j]).max() for i in range(2) for j in range(2))
    e_mm, e_loop = err(got), err(loop)
    print(f"logN 13, 2 x 3 x 2, level 0: max abs error cc_matmul {e_mm:.3e}, loop of cc_dot {e_loop:.3e}, "
          f"largest entry {np.abs(want).max():.2f}")
    assert all(c.level == 1 for r in got for c in r)
    assert e_mm <= 2 * e_loop and e_loop < 1e-5


# ---- the C entry ----------------------------------------------------------------------------------------------------------------
def test_abi():
    from liberate_fhe_amd import _native
    header = open(os.path.join(ROOT, "include", "ckks_hip.h")).read()
    assert re.search(r"\bint64_t lf_cc_matmul_ws_words\(const lf_ks_plan \*plan, int nu\);", header)
    assert re.search(r"\bint lf_cc_matmul\(const lf_ks_plan \*plan, int m, int k, int n, int nu,", header)
    for name in ("lf_cc_matmul", "lf_cc_matmul_ws_words"):
        assert name in _native._SIGNATURES and name in _native.EXPORTED and hasattr(_native.lib, name)
    assert _native.lib.lf_cc_matmul_ws_words.restype is ctypes.c_int64 and _native.lib.lf_cc_matmul.restype is ctypes.c_int
    assert _native.lib.lf_abi_version() == 15                          # additive: the version stays
    from liberate_fhe_amd.fhe import ckks_engine
    from liberate_fhe_amd.fhe.backend import HipBackend
    from liberate_fhe_amd.fhe.ccmatmul import CcMatmulOps
    assert hasattr(HipBackend, "cc_matmul_native") and hasattr(HipBackend, "cc_matmul_ws_words")
    assert issubclass(ckks_engine, CcMatmulOps) and ckks_engine.cc_matmul is CcMatmulOps.cc_matmul


def test_c_entry_refuses_bad_arguments_before_any_launch():
    """lf_cc_matmul returns LF_ERR_ARG from its arguments alone (pointers that are never dereferenced; no call here would pass
    the checks), and lf_cc_matmul_ws_words its value from the shapes."""
    from liberate_fhe_amd._native import KsPlan, lib
    dummy = ctypes.c_void_p(64)

    def ptrs(n, null_at=None):
        arr = (ctypes.c_void_p * max(n, 1))(*([64] * max(n, 1)))
        if null_at is not None:
            arr[null_at] = None
        return arr

    def call(plan, m=2, k=2, n=2, nu=3, ia=(0, 1, 2, 0), ib=(1, 2, 0, -1), ins=None, row0s=None, ksk=dummy, fmt=0, ws=dummy,
             ws_words=1 << 40, out0=None, out1=None, ps=0, cs=0):
        ins = ptrs(2 * nu) if ins is None else ins
        row0s = ptrs(2 * nu) if row0s is None else row0s
        out0 = ptrs(m * n) if out0 is None else out0
        out1 = ptrs(m * n) if out1 is None else out1
        tab = lambda t: None if t is None else (ctypes.c_int64 * max(len(t), 1))(*t)
        return lib.lf_cc_matmul(ctypes.byref(plan) if plan is not None else None, m, k, n, nu, ins, row0s, tab(ia), tab(ib), ksk, ps,
                                cs, 0, fmt, ws, ws_words, out0, out1, None)

    words = lambda plan, nu: lib.lf_cc_matmul_ws_words(ctypes.byref(plan) if plan is not None else None, nu)
    zero = KsPlan()
    assert words(zero, 3) == 0 and words(None, 3) == 0
    assert call(zero) == LF_ERR_ARG and call(None) == LF_ERR_ARG
    for logN in (12, 18):                                              # outside the key switch's ring degrees
        plan = _fake_plan(logN)
        assert words(plan, 3) == 0 and call(plan) == LF_ERR_ARG, logN
    for max_nct in (1, 2, 4):
        plan = _fake_plan(13, max_nct)
        for nu in (1, 3, 256):
            assert words(plan, nu) == (2 * nu + 3 * max_nct) * 2 * (1 << 13)         # the store + a tile's triplets, [ell][N] each
        assert words(plan, 0) == 0 and words(plan, 257) == 0 and words(plan, -1) == 0
        need = words(plan, 3)
        assert call(plan, ws_words=need - 1) == LF_ERR_ARG
        assert call(plan, ws=None) == LF_ERR_ARG
        assert call(plan, ws=ctypes.c_void_p(72)) == LF_ERR_ARG                       # 16-byte aligned
        for bad in (dict(m=0, ia=()), dict(k=0, ia=(), ib=()), dict(n=0, ib=()), dict(m=-1), dict(k=-2), dict(n=-1)):
            assert call(plan, **bad) == LF_ERR_ARG, bad
        assert call(plan, m=1, k=65, n=1, nu=1, ia=(0,) * 65, ib=(0,) * 65) == LF_ERR_ARG   # k above LF_CC_MATMUL_MAX_INNER
        assert call(plan, nu=0) == LF_ERR_ARG and call(plan, nu=257, ins=ptrs(514), row0s=ptrs(514)) == LF_ERR_ARG
        assert call(plan, ia=None) == LF_ERR_ARG and call(plan, ib=None) == LF_ERR_ARG
        assert call(plan, ia=(0, 1, 3, 0)) == LF_ERR_ARG and call(plan, ib=(1, 2, 0, -2)) == LF_ERR_ARG   # an index out of range
        assert call(plan, ia=(0, 1, 1, 0), ib=(1, 0, 0, -1)) == LF_ERR_ARG            # operand 2: no entry uses it
        assert call(plan, ia=(0, -1, 2, 0), ib=(-1, 2, 0, -1)) == LF_ERR_ARG          # output (0, 0) has no term (operand 1 unused too)
        assert call(plan, nu=4, ia=(0, -1, 2, 1), ib=(-1, 2, 0, 3), ins=ptrs(8), row0s=ptrs(8)) == LF_ERR_ARG   # .. every operand used
        for at in range(6):
            assert call(plan, ins=ptrs(6, at)) == LF_ERR_ARG and call(plan, row0s=ptrs(6, at)) == LF_ERR_ARG
        for at in range(4):
            assert call(plan, out0=ptrs(4, at)) == LF_ERR_ARG and call(plan, out1=ptrs(4, at)) == LF_ERR_ARG
        assert call(plan, ksk=None) == LF_ERR_ARG
        assert call(plan, fmt=2) == LF_ERR_ARG
        assert call(plan, fmt=1, ksk=ctypes.c_void_p(72)) == LF_ERR_ARG               # a planes key must be 16-byte aligned
        assert call(plan, fmt=1, ps=1) == LF_ERR_ARG
        a = (ctypes.c_int64 * 4)(0, 1, 2, 0)
        for null_at in (5, 6, 16, 17):                                                # in, row0, out0, out1 themselves
            args = [ctypes.byref(plan), 2, 2, 2, 3, ptrs(6), ptrs(6), a, a, dummy, 0, 0, 0, 0, dummy, 1 << 40, ptrs(4), ptrs(4), None]
            args[null_at] = None
            assert lib.lf_cc_matmul(*args) == LF_ERR_ARG, null_at
        for field in ("rescale_scales", "PR", "x4", "d2", "state", "ext", "sum", "md_ws", "psi_dp", "Ed"):   # what lf_cc_dot refuses
            broken = _fake_plan(13, max_nct)
            setattr(broken, field, None)
            assert words(broken, 3) == 0 and call(broken) == LF_ERR_ARG, field


def test_cc_matmul_kernels_use_no_scratch():
    """matmul_tensor_kernel<R, C> exists for the six tile shapes under its own name, with scratch 0 and no spill, and the
    tracked table lists the instantiations as built."""
    import __graft_entry__ as g
    res = {r["kernel"]: r for r in g.kernel_resources()}
    want = sorted(f"matmul_tensor_kernel<{r}, {c}>" for r, c in ((1, 1), (1, 2), (2, 1), (1, 4), (4, 1), (2, 2)))
    assert sorted(k for k in res if k.startswith("matmul_tensor_kernel<")) == want
    tracked = open(os.path.join(ROOT, "profiles", "r06_kernel_resources.txt")).read()
    for k in want:
        r = res[k]
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, r
        line = next(ln for ln in tracked.splitlines() if ln[18:76].strip() == k)
        f = line.split()
        assert (int(f[-7]), int(f[-3]), int(f[-1])) == (r["vgprs"], r["scratch"], r["occupancy"]), line
