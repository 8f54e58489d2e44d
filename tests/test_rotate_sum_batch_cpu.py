"""rotate_sum_batch / inner_sum_batch (slot sums over many ciphertexts; lf_rotate_sum_batch, ks_inner_rsumb_kernel) without a GPU:
the engine's host logic on the checker backend — which has no batched entry, so the op IS the loop there — against the loop of
rotate_sum / inner_sum that defines its words; the refusals, raised for the whole list before any backend call; the groupings
and the order of the outputs through a marker backend; the C entry's argument checks and workspace size; the new kernel's
resources.  Every comparison is torch.equal."""
import ctypes
import os
import re

import pytest
import torch

from liberate_fhe_amd.utils import synth
from tests.test_inner_sum_cpu import LT, _Q, keys_for, lazy_ciphertext, words

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LF_ERR_ARG = 10001


def same(a, b):
    return a.level == b.level and a.origin == b.origin and all(torch.equal(x, y) for x, y in zip(words(a), words(b)))


class Counting:
    """A backend wrapper that counts every call that reaches the backend (attribute reads of plain values are not calls)."""

    def __init__(self, inner):
        self._inner, self.calls = inner, 0

    def __getattr__(self, name):
        v = getattr(self._inner, name)
        if not callable(v):
            return v

        def counted(*a, **kw):
            self.calls += 1
            return v(*a, **kw)
        return counted


@pytest.fixture(scope="module")
def checker():
    from liberate_fhe_amd.fhe import ckks_engine
    from tests.oracle_backend import OracleBackend
    eng = ckks_engine(devices=["cpu"], backend=OracleBackend(), **LT)
    return eng, keys_for(eng)


def test_the_checker_backend_has_no_batched_entry(checker):
    eng, _ = checker
    assert not hasattr(eng.backend, "rotate_sum_batch_native")
    assert eng.rsum_batch_sizes == (4, 2)


def test_batch_equals_the_loop_on_the_checker_engine(checker):
    """B = 1, 2, 3, 5 over: keys with and without the self term, the self term alone, a repeated key, step 0, a conjugation key; the
    second ciphertext carries lazy words, the fifth is the first once more."""
    eng, keys = checker
    level = 1
    cts = [synth.ciphertext(eng, 90, level), lazy_ciphertext(eng, 91, level), synth.ciphertext(eng, 92, level),
           synth.ciphertext(eng, 93, level)]
    cts.append(cts[0])
    sets = [([keys[1], keys[2], keys[5]], True), ([keys[1], keys[2], keys[5]], False), ([], True), ([keys[1], keys[5], keys[1]], True),
            ([keys[2], keys[0]], False), ([keys[1], keys["conj"]], True)]
    assert eng.rotate_sum_batch([], [keys[1]]) == [] and eng.rotate_sum_batch([], [], include_self=False) == []
    for ks, with_self in sets:
        want = [eng.rotate_sum(ct, ks, include_self=with_self) for ct in cts]
        for B in (1, 2, 3, 5):
            got = eng.rotate_sum_batch(cts[:B], ks, include_self=with_self)
            assert isinstance(got, list) and len(got) == B
            assert all(same(g, w) for g, w in zip(got, want)), (B, [k.origin for k in ks], with_self)
            if B == 5:
                assert got[0] is not got[4]
    # a tuple of ciphertexts and a tuple of keys serve as well; include_self defaults to True
    got = eng.rotate_sum_batch((cts[1], cts[0]), (keys[1], keys[2], keys[5]))
    want = [eng.rotate_sum(ct, [keys[1], keys[2], keys[5]]) for ct in (cts[1], cts[0])]
    assert all(same(g, w) for g, w in zip(got, want))


def test_mixed_levels_keep_their_places(checker):
    eng, keys = checker
    top = eng.num_levels - 1
    cts = [synth.ciphertext(eng, 20 + i, lvl) for i, lvl in enumerate((0, 2, 0, top, 2))]
    ks = [keys[1], keys[700]]
    got = eng.rotate_sum_batch(cts, ks)
    assert [g.level for g in got] == [0, 2, 0, top, 2]
    assert all(same(g, eng.rotate_sum(ct, ks)) for g, ct in zip(got, cts))


def test_inner_sum_batch_equals_the_loop_of_inner_sum(checker):
    eng, _ = checker
    S = eng.num_slots
    cts = [synth.ciphertext(eng, 17, 1), lazy_ciphertext(eng, 18, 1), synth.ciphertext(eng, 19, 0)]
    for n, stride, radix in ((12, S // 16, 4), (8, -1, 4), (1, 1, 4)):
        steps = eng.inner_sum_steps(n, stride, radix)
        keys = {s: synth.key_switch_key(eng, 70 + i, origin=f"rotation key:{s}") for i, s in enumerate(steps)}
        want = [eng.inner_sum(ct, n, keys, stride=stride, radix=radix) for ct in cts]
        got = eng.inner_sum_batch(cts, n, keys, stride=stride, radix=radix)
        assert len(got) == 3 and all(same(g, w) for g, w in zip(got, want)), (n, stride, radix)
        got = eng.inner_sum_batch(cts[:2], n, list(keys.values())[::-1], stride, radix)      # a list, any order
        assert all(same(g, w) for g, w in zip(got, want))
    assert eng.inner_sum_batch([], 8, {}) == []


def test_refusals_come_before_any_backend_call(checker, monkeypatch):
    from liberate_fhe_amd.fhe.presets import errors
    eng, keys = checker
    ok = [synth.ciphertext(eng, 95 + i, 0) for i in range(3)]
    counting = Counting(eng.backend)
    monkeypatch.setattr(eng, "backend", counting)

    def refused(exc, call, mention=None):
        before = counting.calls
        with pytest.raises(exc) as e:
            call()
        assert counting.calls == before, (exc, counting.calls - before)
        if mention is not None:
            assert mention in str(e.value), str(e.value)

    rs, ins = eng.rotate_sum_batch, eng.inner_sum_batch
    ntt = ok[:2] + [eng._new(ok[2].data, ok[2].origin, level=0, ntt_state=True)]
    special = ok[:2] + [eng._new(ok[2].data, ok[2].origin, level=0, include_special=True)]
    refused(errors.NotMatchType, lambda: rs(ok[:2] + [keys[1]], [keys[1]]))                        # wrong origin, last in the list
    refused(errors.NotMatchType, lambda: rs(ok, [keys[1], synth.key_switch_key(eng, 8)]))          # a key of another kind
    refused(ValueError, lambda: rs(ok, [], include_self=False))                                    # nothing to sum
    refused(NotImplementedError, lambda: rs(ntt, [keys[1]]))                                       # only the last member is bad
    refused(NotImplementedError, lambda: rs(special, [keys[1]]))
    refused(NotImplementedError, lambda: rs(special, [], include_self=True))
    refused(errors.NotMatchType, lambda: ins(ok[:2] + [keys[1]], 2, keys))
    refused(errors.NotMatchType, lambda: ins(ok, 16, [keys[1], keys[2], keys[3]]), mention="4")    # a missing key, named by its step
    refused(errors.NotMatchType, lambda: ins(ok, 2, [keys[1], synth.key_switch_key(eng, 8)]))
    refused(errors.NotMatchType, lambda: ins(ok, 2, [keys[1], keys["conj"]]))                      # looked up by step: no conjugation
    refused(NotImplementedError, lambda: ins(ntt, 2, [keys[1]]))
    refused(NotImplementedError, lambda: ins(special, 2, [keys[1]]))
    refused(ValueError, lambda: ins(ok, 0, keys))
    refused(ValueError, lambda: ins(ok, 2 * eng.num_slots, keys))
    # nothing is refused for an empty list, and nothing is called
    before = counting.calls
    assert rs([], [], include_self=False) == [] and ins([], 0, []) == [] and counting.calls == before


class FakeNative:
    """Marks what the engine sends through the batched entry; everything else is the checker backend's."""
    native_ops = True
    lt_batch_max_cts = 64
    rsum_batch_keys_per_launch = 8

    def __init__(self, inner):
        self._inner, self.batches = inner, []

    def __getattr__(self, name):
        return getattr(self._inner, name)

    def rotate_sum_batch_ws_words(self, plan, nct):
        return 0

    def rotate_sum_batch_native(self, plan, c0s, c1s, exps, keys, first_part, row_off, with_self, outs, ws=None):
        assert len(c0s) == len(c1s) == len(outs) and len(exps) == len(keys)
        self.batches.append(dict(c0=[t.data_ptr() for t in c0s], ell=plan.ell, exps=list(exps), with_self=with_self,
                                 shapes={tuple(o.shape) for o in outs}))
        for j, o in enumerate(outs):
            o.fill_(1000 * len(self.batches) + j)


def marked(eng, monkeypatch):
    fake = FakeNative(eng.backend)
    monkeypatch.setattr(eng, "backend", fake)
    monkeypatch.setattr(eng, "_native_level", lambda lvl: 0)
    monkeypatch.setattr(eng, "_op_plan", lambda lvl, d, nct=1: (type("P", (), {"ell": eng._rows(0, lvl, False), "nct": nct})(), None, 0, 0))
    return fake


def noncontiguous(ct):
    for comp in range(2):
        t = ct.data[comp][0]
        wide = torch.zeros((t.shape[0], 2 * t.shape[1]), dtype=t.dtype)
        wide[:, ::2] = t
        ct.data[comp][0] = wide[:, ::2]
        assert not ct.data[comp][0].is_contiguous()


def test_groupings_through_the_marker_backend(checker, monkeypatch):
    """B = 1 -> no call, 2 -> [2], 3 -> [2], 5 -> [4], 7 -> [6]; the members the groups leave over take rotate_sum and every output
    sits at its input's index."""
    from liberate_fhe_amd.fhe import encdec
    eng, keys = checker
    level = 0
    ks = [keys[1], keys[5], keys["conj"]]
    cts = [synth.ciphertext(eng, 30 + i, level) for i in range(7)]
    want = [eng.rotate_sum(ct, ks, include_self=False) for ct in cts]
    N = eng.ctx.N
    for B, calls in ((1, []), (2, [2]), (3, [2]), (5, [4]), (7, [6])):
        fake = marked(eng, monkeypatch)
        got = eng.rotate_sum_batch(cts[:B], ks, include_self=False)
        monkeypatch.undo()
        assert [len(b["c0"]) for b in fake.batches] == calls, B
        n = sum(calls)
        for b in fake.batches:
            assert b["c0"] == [ct.data[0][0].data_ptr() for ct in cts[:n]] and b["with_self"] is False
            assert b["exps"] == [encdec.galois_exponent(N, 1), encdec.galois_exponent(N, 5), encdec.conjugation_exponent(N)]
            assert b["shapes"] == {(2, b["ell"], N)}
        for j in range(n):
            assert got[j].level == level and int(got[j].data[0][0][0, 0]) == 1000 + j == int(got[j].data[1][0][-1, -1])
        assert all(same(got[j], want[j]) for j in range(n, B)), B


def test_a_noncontiguous_member_takes_the_loop_and_keeps_its_place(checker, monkeypatch):
    eng, keys = checker
    ks = [keys[2]]
    cts = [synth.ciphertext(eng, 30 + i, 0) for i in range(7)]
    for i in (1, 4):
        noncontiguous(cts[i])
    want = [eng.rotate_sum(ct, ks) for ct in cts]
    fake = marked(eng, monkeypatch)
    got = eng.rotate_sum_batch(cts, ks)
    monkeypatch.undo()
    assert [b["c0"] for b in fake.batches] == [[cts[i].data[0][0].data_ptr() for i in (0, 2, 3, 5)]]
    for j, i in enumerate((0, 2, 3, 5)):
        assert int(got[i].data[0][0][0, 0]) == 1000 + j
    assert all(same(got[i], want[i]) for i in (1, 4, 6))
    # a group size left out of rsum_batch_sizes goes to the loop: with (4,) alone three ciphertexts are three single calls
    fake = marked(eng, monkeypatch)
    monkeypatch.setattr(eng, "rsum_batch_sizes", (4,))
    got = eng.rotate_sum_batch([cts[0], cts[2], cts[3]], ks)
    monkeypatch.undo()
    assert fake.batches == [] and all(same(g, want[i]) for g, i in zip(got, (0, 2, 3)))


def test_two_levels_give_one_call_per_level(checker, monkeypatch):
    eng, keys = checker
    levels = (0, 2, 0, 2, 2, 0, 0, 2)
    cts = [synth.ciphertext(eng, 50 + i, lvl) for i, lvl in enumerate(levels)]
    fake = marked(eng, monkeypatch)
    got = eng.rotate_sum_batch(cts, [keys[1]])
    monkeypatch.undo()
    assert len(fake.batches) == 2
    at0, at2 = [i for i, l in enumerate(levels) if l == 0], [i for i, l in enumerate(levels) if l == 2]
    assert fake.batches[0]["c0"] == [cts[i].data[0][0].data_ptr() for i in at0]
    assert fake.batches[1]["c0"] == [cts[i].data[0][0].data_ptr() for i in at2]
    assert fake.batches[0]["ell"] == eng._rows(0, 0, False) and fake.batches[1]["ell"] == eng._rows(0, 2, False)
    for n, idx in enumerate((at0, at2)):
        for j, i in enumerate(idx):
            assert got[i].level == levels[i] and int(got[i].data[0][0][0, 0]) == 1000 * (n + 1) + j


def test_long_lists_split_at_a_multiple_of_four(checker, monkeypatch):
    eng, keys = checker
    top = eng.num_levels - 1                     # (one row: the lightest ciphertexts)
    ct = synth.ciphertext(eng, 3, top)
    cts = [ct] * 71                              # 70 go native (17 x 4 + 2), one is left over
    want = eng.rotate_sum(ct, [keys[1]])
    fake = marked(eng, monkeypatch)
    got = eng.rotate_sum_batch(cts, [keys[1]])
    monkeypatch.undo()
    assert [len(b["c0"]) for b in fake.batches] == [64, 6]
    assert [int(g.data[0][0][0, 0]) for g in got[:70]] == [1000 + j for j in range(64)] + [2000 + j for j in range(6)]
    assert same(got[70], want)


def test_inner_sum_batch_runs_one_batch_per_stage(checker, monkeypatch):
    from liberate_fhe_amd.fhe import encdec
    eng, _ = checker
    steps = eng.inner_sum_steps(12, 1, 4)
    keys = {s: synth.key_switch_key(eng, 70 + i, origin=f"rotation key:{s}") for i, s in enumerate(steps)}
    cts = [synth.ciphertext(eng, 60 + i, 0) for i in range(4)]
    fake = marked(eng, monkeypatch)
    got = eng.inner_sum_batch(cts, 12, keys, radix=4)
    monkeypatch.undo()
    plan = encdec.inner_sum_plan(12, 1, eng.num_slots, 4)
    assert [len(b["c0"]) for b in fake.batches] == [4] * len(plan) and all(b["with_self"] is True for b in fake.batches)
    assert [b["exps"] for b in fake.batches] == [[encdec.galois_exponent(eng.ctx.N, s) for s in st] for _, st in plan]
    assert [int(g.data[0][0][0, 0]) for g in got] == [1000 * len(plan) + j for j in range(4)]


def _fake_plan(logN, x4=True, max_nct=4):
    """The plan tests/test_inner_sum_cpu.py builds for lf_rotate_sum: every pointer a dummy that is never dereferenced."""
    from liberate_fhe_amd._native import KsPlan
    plan = KsPlan()
    plan.logN, plan.ell, plan.K, plan.nparts, plan.dig_nparts, plan.max_nct = logN, 2, 1, 2, 2, max_nct
    for name, typ in KsPlan._fields_:
        if typ is ctypes.c_void_p:
            setattr(plan, name, 64)
    plan.q_host = _Q.ctypes.data
    if not x4:
        plan.x4 = None
    return plan


def test_names_and_constants_of_the_binding():
    from liberate_fhe_amd import _native
    from liberate_fhe_amd.fhe.backend import HipBackend
    assert "lf_rotate_sum_batch" in _native.EXPORTED and "lf_rotate_sum_batch_ws_words" in _native.EXPORTED
    assert _native.lib.lf_rotate_sum_batch.restype is ctypes.c_int
    assert _native.lib.lf_rotate_sum_batch_ws_words.restype is ctypes.c_int64
    header = open(os.path.join(ROOT, "include", "ckks_hip.h")).read()
    assert re.search(r"^int64_t lf_rotate_sum_batch_ws_words\(const lf_ks_plan \*plan, int nct\);", header, re.M)
    assert re.search(r"^int lf_rotate_sum_batch\(const lf_ks_plan \*plan, int nct, const int64_t \*const \*c0,", header, re.M)
    source = open(os.path.join(ROOT, "liberate_fhe_amd", "csrc", "ckks_ks.hip")).read()
    assert int(re.search(r"#define LF_RSB_KEYS (\d+)", source).group(1)) == HipBackend.rsum_batch_keys_per_launch
    assert hasattr(HipBackend, "rotate_sum_batch_native") and hasattr(HipBackend, "rotate_sum_batch_ws_words")
    # the range argument's constants: (keys nparts / 2 + 2 keys + 2) q < 2^52 at LF_FP64_MAX_DIGITS and q < 2^41
    digits = int(re.search(r"#define LF_FP64_MAX_DIGITS (\d+)", header).group(1))
    k = HipBackend.rsum_batch_keys_per_launch
    assert (k * digits // 2 + 2 * k + 2) << 41 < 1 << 52


def test_ws_words_grow_with_the_group_not_with_the_batch():
    from liberate_fhe_amd._native import lib
    ws = lambda plan, nct: lib.lf_rotate_sum_batch_ws_words(ctypes.byref(plan), nct)
    for logN in (12, 18):
        assert ws(_fake_plan(logN, x4=False), 4) == 0                 # a refused plan
    assert lib.lf_rotate_sum_batch_ws_words(None, 4) == 0
    assert ws(_fake_plan(13), 4) == 0                                 # the plan's operand stacks serve
    bare = _fake_plan(13, x4=False)
    per_ct = 2 * 2 << 13                                              # 2 ell N, lf_rotate_sum_ws_words of the same plan
    assert lib.lf_rotate_sum_ws_words(ctypes.byref(bare)) == per_ct
    assert [ws(bare, n) for n in (0, -1, 65)] == [0, 0, 0]            # a refused nct
    assert [ws(bare, n) for n in (1, 2, 3, 4, 5, 7, 64)] == [per_ct * g for g in (1, 2, 2, 4, 4, 4, 4)]
    two = _fake_plan(13, x4=False, max_nct=2)
    assert [ws(two, n) for n in (1, 2, 4, 64)] == [per_ct * g for g in (1, 2, 2, 2)]
    one = _fake_plan(13, x4=False, max_nct=1)
    assert [ws(one, n) for n in (1, 4, 64)] == [per_ct] * 3


def test_c_entry_refuses_bad_arguments_before_any_launch():
    """lf_rotate_sum_batch returns LF_ERR_ARG from its arguments alone (dummy pointers that are never dereferenced; no call here
    would pass the checks): everything lf_rotate_sum refuses, nct < 1 or > LF_LT_BATCH_MAX_CTS, a NULL among the pointer arrays or
    their entries, a workspace that is NULL where words are needed, misaligned or too small."""
    from liberate_fhe_amd._native import LF_LT_BATCH_MAX_CTS, lib
    assert LF_LT_BATCH_MAX_CTS == 64
    dummy = ctypes.c_void_p(64)
    arr = (ctypes.c_void_p * 4)(64, 64, 64, 64)
    many = (ctypes.c_void_p * 65)(*([64] * 65))
    nul = (ctypes.c_void_p * 4)(64, 64, None, 64)

    def call(plan, nct, nr, exps, c0=arr, c1=arr, keys=arr, with_self=0, ws=None, ws_words=0, out0=arr, out1=arr, fmt=0):
        e = (ctypes.c_int64 * max(1, len(exps)))(*exps) if exps is not None else None
        return lib.lf_rotate_sum_batch(ctypes.byref(plan) if plan is not None else None, nct, c0, c1, nr, e, keys, 0, 0, 0, fmt,
                                       with_self, ws, ws_words, out0, out1, None)

    for logN in (12, 18):
        assert call(_fake_plan(logN), 4, 1, [3]) == LF_ERR_ARG, logN
    assert call(None, 4, 1, [3]) == LF_ERR_ARG
    plan = _fake_plan(13)
    N2 = 2 << 13
    # what lf_rotate_sum refuses
    assert call(plan, 4, -1, [3]) == LF_ERR_ARG
    assert call(plan, 4, -1, [3], with_self=1) == LF_ERR_ARG
    assert call(plan, 4, 0, [3]) == LF_ERR_ARG                                 # no key and no self term
    assert call(plan, 4, 1, None) == LF_ERR_ARG
    assert call(plan, 4, 1, [3], keys=None) == LF_ERR_ARG
    assert call(plan, 4, 1, [3], fmt=7) == LF_ERR_ARG
    assert call(plan, 4, 1, [3], fmt=-1) == LF_ERR_ARG
    assert call(plan, 4, 2, [3, 4]) == LF_ERR_ARG                              # even exponent
    assert call(plan, 4, 1, [N2 + 1]) == LF_ERR_ARG                            # >= 2N
    assert call(plan, 4, 1, [0]) == LF_ERR_ARG
    assert call(plan, 4, 1, [-3]) == LF_ERR_ARG
    assert call(plan, 4, 3, [3, 5, 7], keys=nul) == LF_ERR_ARG                 # a NULL key
    odd = (ctypes.c_void_p * 4)(72, 64, 64, 64)
    assert call(plan, 4, 1, [3], keys=odd, fmt=1) == LF_ERR_ARG                # a planes key off its 16-byte alignment
    nopr = _fake_plan(13)
    nopr.PR = None
    assert call(nopr, 4, 1, [3]) == LF_ERR_ARG
    assert call(nopr, 4, 0, [3], with_self=1) == LF_ERR_ARG
    # the batch's own: the count, the pointer arrays and their entries
    assert call(plan, 0, 1, [3]) == LF_ERR_ARG
    assert call(plan, -2, 1, [3]) == LF_ERR_ARG
    assert call(plan, 65, 1, [3], c0=many, c1=many, out0=many, out1=many) == LF_ERR_ARG
    for name in ("c0", "c1", "out0", "out1"):
        assert call(plan, 4, 1, [3], **{name: None}) == LF_ERR_ARG, name
        assert call(plan, 4, 1, [3], **{name: nul}) == LF_ERR_ARG, name
        assert call(plan, 3, 0, [3], with_self=1, **{name: nul}) == LF_ERR_ARG, name    # the last entry of three
    # without operand stacks in the plan: an explicit workspace, 16-byte aligned
    bare = _fake_plan(13, x4=False)
    need = lib.lf_rotate_sum_batch_ws_words(ctypes.byref(bare), 4)
    assert need == 4 * (2 * 2 << 13)
    assert call(bare, 4, 1, [3]) == LF_ERR_ARG
    assert call(bare, 4, 1, [3], ws=dummy, ws_words=need - 1) == LF_ERR_ARG
    assert call(bare, 4, 0, [3], with_self=1, ws=dummy, ws_words=need - 1) == LF_ERR_ARG
    assert call(bare, 4, 1, [3], ws=ctypes.c_void_p(72), ws_words=need) == LF_ERR_ARG
    assert call(bare, 1, 1, [3], ws=dummy, ws_words=lib.lf_rotate_sum_batch_ws_words(ctypes.byref(bare), 1) - 1) == LF_ERR_ARG


def test_batch_kernels_use_no_scratch():
    """Every instantiation of ks_inner_rsumb_kernel (4 and 2 ciphertexts x raw / planes key x raw / planes digits) exists with
    scratch 0 and no spill; the tracked table lists them as built."""
    import __graft_entry__ as g
    res = {r["kernel"]: r for r in g.kernel_resources()}
    by = {k: r for k, r in res.items() if k.startswith("ks_inner_rsumb_kernel<")}
    want = [f"ks_inner_rsumb_kernel<{nct}, {pl}, {dpl}>" for nct in (4, 2) for pl in ("true", "false") for dpl in ("true", "false")]
    assert sorted(by) == sorted(want)
    for k in want:
        assert by[k]["scratch"] == 0 and by[k]["vgpr_spill"] == 0 and by[k]["sgpr_spill"] == 0, by[k]
    tracked = open(os.path.join(ROOT, "profiles", "r06_kernel_resources.txt")).read()
    for k, r in by.items():
        line = next(ln for ln in tracked.splitlines() if ln[18:76].strip() == k)
        f = line.split()
        assert (int(f[-7]), int(f[-3]), int(f[-1])) == (r["vgprs"], r["scratch"], r["occupancy"]), line
