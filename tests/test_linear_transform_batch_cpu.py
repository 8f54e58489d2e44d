"""linear_transform_batch (one transform over many ciphertexts; lf_linear_transform_batch, ks_inner_ltb_kernel) without a GPU: the
engine's host logic on the checker backend — which has no batched entry, so the op IS the loop there — against the loop of
linear_transform that defines its words; the refusals, raised for the whole list before any encoding or backend call; the order
of the outputs when some members take the straggler path; the C entry's argument checks and workspace size; the new kernel's
resources.  Every comparison is torch.equal."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from liberate_fhe_amd.utils import synth
from tests.test_inner_sum_cpu import lazy_ciphertext
from tests.test_linear_transform_cpu import LT, keys_for, words

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = (0, 1, 2, 5, 11, 700)


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
    return eng, keys_for(eng, STEPS)


def test_the_checker_backend_has_no_batched_entry(checker):
    eng, _ = checker
    assert not hasattr(eng.backend, "linear_transform_batch_native")


def test_batch_equals_the_loop_on_the_checker_engine(checker):
    eng, keys = checker
    level = 1
    diags = synth.diagonals(eng, 7, level, (0, 1, 5, 700))
    cts = [lazy_ciphertext(eng, 90, level), synth.ciphertext(eng, 91, level), synth.ciphertext(eng, 92, level)]
    want = [eng.linear_transform(ct, diags, keys) for ct in cts]
    assert eng.linear_transform_batch([], diags, keys) == []
    for B in (1, 3):
        got = eng.linear_transform_batch(cts[:B], diags, keys)
        assert isinstance(got, list) and len(got) == B
        assert all(same(g, w) for g, w in zip(got, want)), B
    # the same object several times; a tuple of ciphertexts and a list of keys serve as well
    got = eng.linear_transform_batch((cts[1], cts[0], cts[1]), diags, [keys[700], keys[5], keys[1]])
    assert same(got[0], want[1]) and same(got[1], want[0]) and same(got[2], want[1])
    assert got[0] is not got[2]


def test_a_mapping_is_encoded_once_at_the_level_of_the_first_ciphertext(checker, monkeypatch):
    """Encoding rounds at random (encode's randround), so two encodings of one mapping differ in their words: the batch encodes
    ONCE, and its outputs are the loop's over that very object."""
    eng, keys = checker
    level = 2
    np.random.seed(5)
    mapping = {0: [0.5, -0.25], 1: eng.example(-1, 1), eng.num_slots + 5: 2.0}
    cts = [synth.ciphertext(eng, 60 + i, level) for i in range(3)]
    made, real = [], eng.encode_diagonals

    def recording(diagonals, lvl, bsgs=None):
        made.append((lvl, real(diagonals, lvl, bsgs)))
        return made[-1][1]
    monkeypatch.setattr(eng, "encode_diagonals", recording)
    got = eng.linear_transform_batch(cts, mapping, keys)
    monkeypatch.undo()
    assert [lvl for lvl, _ in made] == [level] and eng.diagonal_steps(made[0][1]) == [0, 1, 5]
    want = [eng.linear_transform(ct, made[0][1], keys) for ct in cts]
    assert all(same(g, w) for g, w in zip(got, want))


def test_bsgs_diagonals_run_as_the_loop(checker):
    eng, _ = checker
    level, steps = 0, (0, 1, 2, 5, 6, 9)
    diags = synth.diagonals_bsgs(eng, 11, level, steps, 4)
    _, babies, giants = eng.bsgs_steps(diags)
    keys = keys_for(eng, tuple(sorted(set(babies) | set(giants))))
    cts = [synth.ciphertext(eng, 70 + i, level) for i in range(2)]
    want = [eng.linear_transform(ct, diags, keys) for ct in cts]
    got = eng.linear_transform_batch(cts, diags, keys)
    assert all(same(g, w) for g, w in zip(got, want))
    from liberate_fhe_amd.fhe.presets import errors
    missing = {s: k for s, k in keys.items() if s != max(giants)}
    with pytest.raises(errors.NotMatchType) as e:
        eng.linear_transform_batch(cts, diags, missing)
    assert str(max(giants)) in str(e.value)


def test_refusals_come_before_any_encoding_or_backend_call(checker, monkeypatch):
    from liberate_fhe_amd.fhe.presets import errors
    eng, keys = checker
    ok = [synth.ciphertext(eng, 95 + i, 0) for i in range(3)]
    diags = synth.diagonals(eng, 4, 0, (0, 1, 5))
    mapping = {0: [1.0], 1: [0.5, 0.5], 5: [0.25]}
    top = eng.num_levels - 1
    tops = [synth.ciphertext(eng, 99, top)] * 2
    at1 = synth.ciphertext(eng, 98, 1)
    encodes = []
    counting = Counting(eng.backend)
    monkeypatch.setattr(eng, "backend", counting)
    monkeypatch.setattr(eng, "encode_diagonals", lambda *a, **kw: encodes.append(a) or pytest.fail("encode_diagonals was reached"))

    def refused(exc, cts, dg, ks, mention=None):
        before = counting.calls
        with pytest.raises(exc) as e:
            eng.linear_transform_batch(cts, dg, ks)
        assert counting.calls == before and not encodes, (exc, counting.calls - before)
        if mention is not None:
            assert mention in str(e.value), str(e.value)

    for dg in (diags, mapping):
        refused(errors.NotMatchType, ok[:2] + [keys[1]], dg, keys)                       # wrong origin, last in the list
        refused(errors.NotMatchType, ok, dg, [keys[1], synth.key_switch_key(eng, 8)])    # a key of another kind
        refused(NotImplementedError, ok[:2] + [eng._new(ok[2].data, ok[2].origin, level=0, ntt_state=True)], dg, keys)
        refused(NotImplementedError, ok[:2] + [eng._new(ok[2].data, ok[2].origin, level=0, include_special=True)], dg, keys)
        refused(errors.NotMatchType, ok, dg, [keys[1]], mention="step 5")                # a missing key, named by its step
        refused(errors.NotMatchDataStructState, ok[:2] + [at1], dg, keys, mention="ciphertext 2")
    refused(errors.MaximumLevelError, tops, mapping, keys)                               # no level left
    refused(errors.MaximumLevelError, ok[:1] + tops, diags, keys)
    refused(errors.NotMatchDataStructState, [at1] + ok[:2], diags, keys, mention="ciphertext 0")
    refused(errors.NotMatchType, ok, ok[0], keys)                                        # not an encode_diagonals object
    # nothing is refused for an empty list, and nothing is called
    before = counting.calls
    assert eng.linear_transform_batch([], mapping, []) == [] and counting.calls == before


class FakeNative:
    """Marks what the engine sends through the batched entry; everything else is the checker backend's."""
    native_ops = True
    lt_batch_max_cts = 64
    lt_batch_keys_per_launch = 8

    def __init__(self, inner):
        self._inner, self.batches = inner, []

    def __getattr__(self, name):
        return getattr(self._inner, name)

    def linear_transform_batch_ws_words(self, plan, nct):
        return 0

    def linear_transform_batch_native(self, plan, c0s, c1s, exps, keys, first_part, row_off, pt, pt0, scales, round_at, outs, ws=None):
        self.batches.append([t.data_ptr() for t in c0s])
        for j, o in enumerate(outs):
            o.fill_(1000 * len(self.batches) + j)


def test_output_order_follows_input_order_with_stragglers(checker, monkeypatch):
    """Seven ciphertexts, the second and the fifth not contiguous: the five that qualify form a group of 4 for the native entry (a
    marker backend here), the fifth of them and the two stragglers take linear_transform; every output sits at its input's index."""
    eng, keys = checker
    level = 0
    diags = synth.diagonals(eng, 4, level, (0, 1, 5))
    cts = [synth.ciphertext(eng, 30 + i, level) for i in range(7)]
    for i in (1, 4):
        for comp in range(2):
            t = cts[i].data[comp][0]
            wide = torch.zeros((t.shape[0], 2 * t.shape[1]), dtype=t.dtype)
            wide[:, ::2] = t
            cts[i].data[comp][0] = wide[:, ::2]
            assert not cts[i].data[comp][0].is_contiguous()
    want = [eng.linear_transform(ct, diags, keys) for ct in cts]
    fake = FakeNative(eng.backend)
    monkeypatch.setattr(eng, "backend", fake)
    monkeypatch.setattr(eng, "_native_level", lambda lvl: 0)
    monkeypatch.setattr(eng, "_op_plan", lambda lvl, d, nct=1: (type("P", (), {"ell": eng._rows(0, lvl, False)})(), None, 0, 0))
    got = eng.linear_transform_batch(cts, diags, keys)
    monkeypatch.undo()
    assert fake.batches == [[cts[i].data[0][0].data_ptr() for i in (0, 2, 3, 5)]]
    for j, i in enumerate((0, 2, 3, 5)):
        assert got[i].level == level + 1 and int(got[i].data[0][0][0, 0]) == 1000 + j and int(got[i].data[1][0][0, 0]) == 1000 + j
    for i in (1, 4, 6):
        assert same(got[i], want[i]), i
    # a group size left out of lt_batch_sizes goes to the loop: with (4,) alone three ciphertexts are three single calls
    fake.batches.clear()
    monkeypatch.setattr(eng, "backend", fake)
    monkeypatch.setattr(eng, "_native_level", lambda lvl: 0)
    monkeypatch.setattr(eng, "lt_batch_sizes", (4,))
    got = eng.linear_transform_batch([cts[0], cts[2], cts[3]], diags, keys)
    monkeypatch.undo()
    assert fake.batches == [] and all(same(g, want[i]) for g, i in zip(got, (0, 2, 3)))


_Q = np.array([(1 << 41) - 65535, (1 << 60) - 93, (1 << 60) - 173], dtype=np.int64)


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
    assert "lf_linear_transform_batch" in _native.EXPORTED and "lf_linear_transform_batch_ws_words" in _native.EXPORTED
    assert _native.lib.lf_abi_version() == 15
    header = open(os.path.join(ROOT, "include", "ckks_hip.h")).read()
    assert int(re.search(r"#define LF_LT_BATCH_MAX_CTS (\d+)", header).group(1)) == _native.LF_LT_BATCH_MAX_CTS == HipBackend.lt_batch_max_cts
    source = open(os.path.join(ROOT, "liberate_fhe_amd", "csrc", "ckks_ks.hip")).read()
    assert int(re.search(r"#define LF_LTB_KEYS (\d+)", source).group(1)) == HipBackend.lt_batch_keys_per_launch
    assert hasattr(HipBackend, "linear_transform_batch_native")


def test_ws_words_grow_with_the_group_not_with_the_batch():
    from liberate_fhe_amd._native import lib
    ws = lambda plan, nct: lib.lf_linear_transform_batch_ws_words(ctypes.byref(plan), nct)
    for logN in (12, 18):
        assert ws(_fake_plan(logN, x4=False), 4) == 0                 # a refused plan
    assert lib.lf_linear_transform_batch_ws_words(None, 4) == 0
    assert ws(_fake_plan(13), 4) == 0                                 # the plan's operand stacks serve
    bare = _fake_plan(13, x4=False)
    per_ct = 4 * 2 << 13                                              # 4 ell N, lf_linear_transform_ws_words of the same plan
    assert lib.lf_linear_transform_ws_words(ctypes.byref(bare)) == per_ct
    assert [ws(bare, n) for n in (0, -1, 65)] == [0, 0, 0]            # a refused nct
    assert [ws(bare, n) for n in (1, 2, 3, 4, 5, 7, 64)] == [per_ct * g for g in (1, 2, 2, 4, 4, 4, 4)]
    two = _fake_plan(13, x4=False, max_nct=2)
    assert [ws(two, n) for n in (1, 2, 4, 64)] == [per_ct * g for g in (1, 2, 2, 2)]
    one = _fake_plan(13, x4=False, max_nct=1)
    assert [ws(one, n) for n in (1, 4, 64)] == [per_ct] * 3


def test_c_entry_refuses_bad_arguments_before_any_launch():
    """lf_linear_transform_batch returns LF_ERR_ARG from its arguments alone (dummy pointers that are never dereferenced; no call
    here would pass the checks): everything lf_linear_transform refuses, nct < 1 or > LF_LT_BATCH_MAX_CTS, a NULL among the pointer
    arrays or their entries, a workspace that is NULL where words are needed, misaligned or too small."""
    from liberate_fhe_amd._native import LF_LT_BATCH_MAX_CTS, lib
    LF_ERR_ARG = 10001
    dummy = ctypes.c_void_p(64)
    arr = (ctypes.c_void_p * 4)(64, 64, 64, 64)
    many = (ctypes.c_void_p * (LF_LT_BATCH_MAX_CTS + 1))(*([64] * (LF_LT_BATCH_MAX_CTS + 1)))
    nul = (ctypes.c_void_p * 4)(64, 64, None, 64)
    stride = 3 << 13

    def call(plan, nct, nr, exps, c0=arr, c1=arr, keys=arr, pt=dummy, pt0=None, ws=None, ws_words=0, out0=arr, out1=arr, scales=dummy,
             fmt=0, pt_stride=stride):
        e = (ctypes.c_int64 * max(1, len(exps)))(*exps) if exps is not None else None
        return lib.lf_linear_transform_batch(ctypes.byref(plan) if plan is not None else None, nct, c0, c1, nr, e, keys, 0, 0, 0, fmt, pt,
                                             pt_stride, pt0, scales, 0, ws, ws_words, out0, out1, None)

    for logN in (12, 18):
        assert call(_fake_plan(logN), 4, 1, [3]) == LF_ERR_ARG, logN
    assert call(None, 4, 1, [3]) == LF_ERR_ARG
    plan = _fake_plan(13)
    N2 = 2 << 13
    # what lf_linear_transform refuses
    assert call(plan, 4, -1, [3]) == LF_ERR_ARG
    assert call(plan, 4, 0, [3]) == LF_ERR_ARG                                 # no key and no step-0 diagonal
    assert call(plan, 4, 1, None) == LF_ERR_ARG
    assert call(plan, 4, 1, [3], keys=None) == LF_ERR_ARG
    assert call(plan, 4, 1, [3], pt=None) == LF_ERR_ARG
    assert call(plan, 4, 1, [3], pt_stride=stride - 1) == LF_ERR_ARG
    assert call(plan, 4, 1, [3], scales=None) == LF_ERR_ARG
    assert call(plan, 4, 1, [3], fmt=7) == LF_ERR_ARG
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
    one = _fake_plan(13)
    one.ell = 1                                                                # no level left to rescale into
    assert call(one, 4, 1, [3]) == LF_ERR_ARG
    # the batch's own: the count, the pointer arrays and their entries
    assert call(plan, 0, 1, [3]) == LF_ERR_ARG
    assert call(plan, -2, 1, [3]) == LF_ERR_ARG
    assert call(plan, LF_LT_BATCH_MAX_CTS + 1, 1, [3], c0=many, c1=many, out0=many, out1=many) == LF_ERR_ARG
    for name in ("c0", "c1", "out0", "out1"):
        assert call(plan, 4, 1, [3], **{name: None}) == LF_ERR_ARG, name
        assert call(plan, 4, 1, [3], **{name: nul}) == LF_ERR_ARG, name
        assert call(plan, 3, 0, [3], pt0=dummy, **{name: nul}) == LF_ERR_ARG, name      # the last entry of three
    # without operand stacks in the plan: an explicit workspace, 16-byte aligned
    bare = _fake_plan(13, x4=False)
    need = lib.lf_linear_transform_batch_ws_words(ctypes.byref(bare), 4)
    assert need == 4 * (4 * 2 << 13)
    assert call(bare, 4, 1, [3]) == LF_ERR_ARG
    assert call(bare, 4, 1, [3], ws=dummy, ws_words=need - 1) == LF_ERR_ARG
    assert call(bare, 4, 0, [3], pt0=dummy, ws=dummy, ws_words=need - 1) == LF_ERR_ARG
    assert call(bare, 4, 1, [3], ws=ctypes.c_void_p(72), ws_words=need) == LF_ERR_ARG
    assert call(bare, 1, 1, [3], ws=dummy, ws_words=lib.lf_linear_transform_batch_ws_words(ctypes.byref(bare), 1) - 1) == LF_ERR_ARG


def test_batch_kernels_use_no_scratch():
    """Every instantiation of ks_inner_ltb_kernel (4 and 2 ciphertexts x raw / planes key x raw / planes digits, NK = 1 key per
    pass of the digit loop) exists with scratch 0 and no spill, at no fewer waves per SIMD than the flat kernel of four keys; the
    tracked table lists them as built."""
    import __graft_entry__ as g
    res = {r["kernel"]: r for r in g.kernel_resources()}
    by = {k: r for k, r in res.items() if k.startswith("ks_inner_ltb_kernel<")}
    want = [f"ks_inner_ltb_kernel<{nct}, 1, {pl}, {dpl}>" for nct in (4, 2) for pl in ("true", "false") for dpl in ("true", "false")]
    assert sorted(by) == sorted(want)
    for k in want:
        assert by[k]["scratch"] == 0 and by[k]["vgpr_spill"] == 0 and by[k]["sgpr_spill"] == 0, by[k]
        flat = res["ks_inner_lt_kernel<4, " + k.split(", ", 2)[2]]
        assert by[k]["occupancy"] >= flat["occupancy"] >= 3, (by[k], flat)
    tracked = open(os.path.join(ROOT, "profiles", "r06_kernel_resources.txt")).read()
    for k, r in by.items():
        line = next(ln for ln in tracked.splitlines() if ln[18:76].strip() == k)
        f = line.split()
        assert (int(f[-7]), int(f[-3]), int(f[-1])) == (r["vgprs"], r["scratch"], r["occupancy"]), line
