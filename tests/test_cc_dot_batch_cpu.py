"""cc_dot_batch and poly_eval_batch (lf_cc_dot_batch: several dots under one key, the key read once per group) without a GPU: the
engine's host logic on the checker backend against the loops that define the words, the refusals, the C entry's argument checks
and the new inner-product kernel's resources."""
import ctypes
import os

import numpy as np
import pytest

from liberate_fhe_amd.utils import synth
from tests.test_cc_dot_cpu import _fake_plan, pairs_of, same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LF_ERR_ARG = 10001


def engine_of(logN, num_scales=5):
    from liberate_fhe_amd.fhe import ckks_engine
    from tests.oracle_backend import OracleBackend
    return ckks_engine(devices=["cpu"], backend=OracleBackend(), logN=logN, num_scales=num_scales, num_special_primes=2, is_secured=False)


@pytest.fixture(scope="module", params=[12, 13])
def checker(request):
    return engine_of(request.param)


def all_same(got, want):
    return len(got) == len(want) and all(same(g, w) for g, w in zip(got, want))


def test_exports():
    from liberate_fhe_amd import _native
    for name in ("lf_cc_dot_batch", "lf_cc_dot_batch_ws_words"):
        assert name in _native._SIGNATURES and hasattr(_native.lib, name)
    assert _native.lib.lf_cc_dot_batch_ws_words.restype is ctypes.c_int64 and _native.lib.lf_cc_dot_batch.restype is ctypes.c_int
    assert _native.lib.lf_abi_version() == 15                          # additive: the version stays
    from liberate_fhe_amd.fhe.backend import HipBackend
    assert hasattr(HipBackend, "cc_dot_batch_native") and hasattr(HipBackend, "cc_dot_batch_ws_words")


def test_cc_dot_batch_equals_the_loop_of_cc_dot(checker):
    """Dots of unequal pair counts at two levels in one call (grouped by level, results in the caller's order), any iterables."""
    eng = checker
    evk = synth.key_switch_key(eng, 77)
    p0, p2 = pairs_of(eng, 5, 0), pairs_of(eng, 5, 2)
    dots = [p0[:1], p2[:3], p0, p0[2:4], p2[4:], p0[1:3], p2]
    got = eng.cc_dot_batch(dots, evk)
    assert [g.level for g in got] == [1, 3, 1, 1, 3, 1, 3]
    assert all_same(got, [eng.cc_dot(pairs, evk) for pairs in dots])
    assert all_same(eng.cc_dot_batch(iter([iter(p0[:2]), [list(p0[2])]]), evk), [eng.cc_dot(p0[:2], evk), eng.cc_dot([p0[2]], evk)])
    assert eng.cc_dot_batch([], evk) == []


def test_cc_dot_batch_refusals_are_those_of_cc_dot(checker):
    from liberate_fhe_amd.fhe.presets import errors
    eng = checker
    evk = synth.key_switch_key(eng, 77)
    top = eng.num_levels - 1
    a0, b0, a1, atop = (synth.ciphertext(eng, 60 + i, lvl) for i, lvl in enumerate((0, 0, 1, top)))
    trip = eng.cc_mult(a0, b0, evk, relin=False)
    ntt = eng._new(a0.data, a0.origin, level=0, ntt_state=True)
    special = eng._new(a0.data, a0.origin, level=0, include_special=True)
    good = [(a0, b0)]
    for exc, bad in [(ValueError, []), (ValueError, [(a0,)]), (errors.NotMatchType, [(a0, trip)]), (errors.NotMatchType, [(a0, None)]),
                     (errors.NotMatchDataStructState, [(a0, a1)]), (errors.NotMatchDataStructState, [(a0, b0), (a1, a1)]),
                     (errors.MaximumLevelError, [(atop, atop)]), (errors.NotMatchDataStructState, [(a0, ntt)]),
                     (errors.NotMatchDataStructState, [(special, b0)])]:
        for dots in ([bad], [good, bad], [good, good, bad, good]):
            with pytest.raises(exc):
                eng.cc_dot_batch(dots, evk)
    assert all_same(eng.cc_dot_batch([good, [(a1, a1)]], evk), [eng.cc_dot(good, evk), eng.cc_dot([(a1, a1)], evk)])   # levels may differ ACROSS dots


POLYS = (("power", 7, None, None), ("power", 5, None, 8), ("chebyshev", 7, (-3, 5), None), ("chebyshev", 6, None, 2))


@pytest.mark.parametrize("logN", [12, 13])
def test_poly_eval_batch_equals_the_loop_of_poly_eval(logN):
    from liberate_fhe_amd.fhe.presets import errors
    eng = engine_of(logN, 8)
    evk = synth.key_switch_key(eng, 77)
    cts = [synth.ciphertext(eng, 80 + i, 0) for i in range(3)]
    for basis, degree, interval, n1 in POLYS:
        coeffs = np.random.default_rng(degree).uniform(-1, 1, degree + 1)
        got = eng.poly_eval_batch(cts, coeffs, evk, basis=basis, interval=interval, n1=n1)
        want = [eng.poly_eval(ct, coeffs, evk, basis=basis, interval=interval, n1=n1) for ct in cts]
        depth = eng.poly_depth(degree, basis, interval, n1)
        assert all(g.level == depth and not g.ntt_state and not g.include_special for g in got)
        assert all_same(got, want), (basis, degree, interval, n1)
    c3 = [0.5, -1.0, 0.25, 0.125]
    assert all_same(eng.poly_eval_batch(iter(cts[:1]), c3, evk), [eng.poly_eval(cts[0], c3, evk)])
    # refusals, before any work: nothing to evaluate, mixed levels, a wrong type or state, too few levels, poly_eval's own
    up = synth.ciphertext(eng, 90, 1)
    trip = eng.cc_mult(cts[0], cts[1], evk, relin=False)
    with pytest.raises(ValueError):
        eng.poly_eval_batch([], c3, evk)
    with pytest.raises(errors.NotMatchDataStructState):
        eng.poly_eval_batch([cts[0], up], c3, evk)
    with pytest.raises(errors.NotMatchType):
        eng.poly_eval_batch([cts[0], trip], c3, evk)
    with pytest.raises(errors.NotMatchType):
        eng.poly_eval_batch([cts[0], None], c3, evk)
    with pytest.raises(errors.NotMatchDataStructState):
        eng.poly_eval_batch([cts[0], eng._new(cts[0].data, cts[0].origin, level=0, ntt_state=True)], c3, evk)
    with pytest.raises(errors.MaximumLevelError):
        eng.poly_eval_batch([synth.ciphertext(eng, 91, eng.num_levels - 2)] * 2, c3, evk)
    with pytest.raises(ValueError):
        eng.poly_eval_batch(cts, [1.0], evk)
    with pytest.raises(ValueError):
        eng.poly_eval_batch(cts, c3, evk, interval=(-2, 2))


def test_c_entry_refuses_bad_arguments_before_any_launch():
    """lf_cc_dot_batch returns LF_ERR_ARG from its arguments alone (pointers that are never dereferenced; no call here would pass
    the checks): what lf_cc_dot refuses, a dot count that is not 1, 2 or 4 or above the plan's max_nct, pair counts missing or
    below 1, a NULL among the 4 x (sum of pair counts) operand pointers or among the outputs, a workspace missing or smaller than
    lf_cc_dot_batch_ws_words says; and that function's value from the shapes."""
    from liberate_fhe_amd._native import KsPlan, lib
    dummy = ctypes.c_void_p(64)

    def ptrs(n, null_at=None):
        arr = (ctypes.c_void_p * max(n, 1))(*([64] * max(n, 1)))
        if null_at is not None:
            arr[null_at] = None
        return arr

    def call(plan, nps=(2, 1), nd=None, np_arr=True, ins=None, row0s=None, ksk=dummy, fmt=0, ws=dummy, ws_words=1 << 40, out0=None,
             out1=None, ps=0, cs=0):
        nd = len(nps) if nd is None else nd
        total = 4 * sum(max(n, 0) for n in nps)
        arr = (ctypes.c_int64 * max(len(nps), 1))(*nps) if np_arr else None
        ins = ptrs(total) if ins is None else ins
        row0s = ptrs(total) if row0s is None else row0s
        out0 = ptrs(len(nps)) if out0 is None else out0
        out1 = ptrs(len(nps)) if out1 is None else out1
        return lib.lf_cc_dot_batch(ctypes.byref(plan) if plan is not None else None, nd, arr, ins, row0s, ksk, ps, cs, 0, fmt, ws, ws_words,
                                   out0, out1, None)

    words = lambda plan, nd: lib.lf_cc_dot_batch_ws_words(ctypes.byref(plan) if plan is not None else None, nd)
    zero = KsPlan()
    assert words(zero, 2) == 0 and words(None, 2) == 0
    assert call(zero) == LF_ERR_ARG and call(None) == LF_ERR_ARG
    for logN in (12, 18):                                              # outside the key switch's ring degrees
        plan = _fake_plan(logN, 4)
        assert words(plan, 2) == 0 and call(plan) == LF_ERR_ARG, logN
    for max_nct in (1, 2, 4):
        plan = _fake_plan(13, max_nct)
        for nd in (1, 2, 4):
            nps = (3, 1, 9, 2)[:nd]
            if nd > max_nct:                                           # lf_cc_mult_evk_batch's rule
                assert words(plan, nd) == 0 and call(plan, nps) == LF_ERR_ARG, (max_nct, nd)
                continue
            need = words(plan, nd)
            assert need == nd * 3 * 2 * (1 << 13)                      # nd summed triplets [3][ell][N]
            assert call(plan, nps, ws_words=need - 1) == LF_ERR_ARG
            assert call(plan, nps, ws=None) == LF_ERR_ARG
            assert call(plan, nps, np_arr=False) == LF_ERR_ARG
            for at in range(nd):
                for v in (0, -1):
                    bad = list(nps)
                    bad[at] = v
                    assert call(plan, bad) == LF_ERR_ARG
                assert call(plan, nps, out0=ptrs(nd, at)) == LF_ERR_ARG
                assert call(plan, nps, out1=ptrs(nd, at)) == LF_ERR_ARG
            total = 4 * sum(nps)
            for at in (0, total - 1, total // 2, 4 * nps[0] - 1, 4 * nps[0] % total):
                assert call(plan, nps, ins=ptrs(total, at)) == LF_ERR_ARG
                assert call(plan, nps, row0s=ptrs(total, at)) == LF_ERR_ARG
            assert call(plan, nps, ksk=None) == LF_ERR_ARG
            assert call(plan, nps, fmt=2) == LF_ERR_ARG
            assert call(plan, nps, fmt=1, ksk=ctypes.c_void_p(72)) == LF_ERR_ARG   # a planes key must be 16-byte aligned
            assert call(plan, nps, fmt=1, ps=1) == LF_ERR_ARG
            assert call(plan, nps, fmt=1, cs=1) == LF_ERR_ARG
            for which in ("ins", "row0s", "out0", "out1"):
                assert lib.lf_cc_dot_batch(ctypes.byref(plan), nd, (ctypes.c_int64 * nd)(*nps),
                                           *[None if which == w else ptrs(total) for w in ("ins", "row0s")], dummy, 0, 0, 0, 0, dummy, 1 << 40,
                                           *[None if which == w else ptrs(nd) for w in ("out0", "out1")], None) == LF_ERR_ARG, which
            for field in ("rescale_scales", "PR", "x4", "d2", "state", "ext", "sum", "md_ws", "psi_dp", "Ed"):   # what lf_cc_dot refuses
                broken = _fake_plan(13, max_nct)
                setattr(broken, field, None)
                assert words(broken, nd) == 0 and call(broken, nps) == LF_ERR_ARG, field
        for nd in (0, -1, 3, 5, 8):
            assert words(plan, nd) == 0 and call(plan, (1,) * max(nd, 1), nd=nd) == LF_ERR_ARG, nd
    bad = _fake_plan(13)
    bad.max_nct = 0
    assert call(bad, (1,)) == LF_ERR_ARG and words(bad, 1) == 0


def test_batched_dot_kernels_use_no_scratch():
    """ks_dotb_inner_kernel<2 | 4, raw / planes key, raw / planes digits> — the pre-summed fold for several triplets — exists under
    its own name with scratch 0 and no spill, at no less than the occupancy of ks_inner2_kernel<NCT, fold> with the same key
    and digit formats; the tracked table lists the kernels as built."""
    import __graft_entry__ as g
    res = {r["kernel"]: r for r in g.kernel_resources()}
    want = {f"ks_dotb_inner_kernel<{nct}, {pl}, {dpl}>": res[f"ks_inner2_kernel<{nct}, true, {pl}, {dpl}>"]["occupancy"]
            for nct in (2, 4) for pl in ("true", "false") for dpl in ("true", "false")}
    assert sorted(k for k in res if k.startswith("ks_dotb_inner_kernel")) == sorted(want)
    tracked = open(os.path.join(ROOT, "profiles", "r06_kernel_resources.txt")).read()
    for k, floor in want.items():
        r = res[k]
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, r
        assert r["occupancy"] >= floor, (r, floor)
        line = next(ln for ln in tracked.splitlines() if ln[18:76].strip() == k)
        f = line.split()
        assert (int(f[-7]), int(f[-3]), int(f[-1])) == (r["vgprs"], r["scratch"], r["occupancy"]), line
