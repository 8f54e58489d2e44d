"""linear_transform_batch over baby-step / giant-step diagonals (lf_linear_transform_bsgs_batch, ks_inner_babyb_kernel) without a
GPU: the exports and their binding, the workspace size, the C entry's argument checks, the new kernel's resources, the engine's
grouping over a marker backend, and the contract on the checker backend (which has no batched entry: the op IS the loop there).
Every comparison is torch.equal."""
import ctypes
import os

import pytest
import torch

from liberate_fhe_amd.utils import synth
from tests.test_linear_transform_batch_cpu import _fake_plan, same
from tests.test_linear_transform_cpu import LT, keys_for

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LF_ERR_ARG = 10001
S_PAIRS = 4   # csrc/ckks_ops.hip: LF_BSGS_S_PAIRS


@pytest.fixture(scope="module")
def checker():
    from liberate_fhe_amd.fhe import ckks_engine
    from tests.oracle_backend import OracleBackend
    return ckks_engine(devices=["cpu"], backend=OracleBackend(), **LT)


def bsgs_keys(eng, diags):
    _, babies, giants = eng.bsgs_steps(diags)
    return keys_for(eng, tuple(sorted(set(babies) | set(giants)))), babies, giants


def test_the_library_exports_the_entry_and_the_binding_declares_it():
    from liberate_fhe_amd import _native
    from liberate_fhe_amd.fhe import ckks_engine
    from liberate_fhe_amd.fhe.backend import HipBackend
    for name in ("lf_linear_transform_bsgs_batch", "lf_linear_transform_bsgs_batch_ws_words"):
        assert name in _native.EXPORTED and getattr(_native.lib, name).argtypes
    assert _native.lib.lf_linear_transform_bsgs_batch_ws_words.restype is ctypes.c_int64
    assert _native.lib.lf_abi_version() == 15
    assert hasattr(HipBackend, "linear_transform_bsgs_batch_native") and hasattr(HipBackend, "linear_transform_bsgs_batch_ws_words")
    header = open(os.path.join(ROOT, "include", "ckks_hip.h")).read()
    assert "int lf_linear_transform_bsgs_batch(" in header and "int64_t lf_linear_transform_bsgs_batch_ws_words(" in header
    # the group sizes of the engine: a subset of (4, 2), largest first
    sizes = ckks_engine.lt_bsgs_batch_sizes
    assert set(sizes) <= {4, 2} and list(sizes) == sorted(sizes, reverse=True)


def test_ws_words_grow_with_the_group_not_with_the_batch():
    from liberate_fhe_amd._native import lib
    ws = lambda plan, nb, nct: lib.lf_linear_transform_bsgs_batch_ws_words(ctypes.byref(plan), nb, nct)
    single = lambda plan, nb: lib.lf_linear_transform_bsgs_ws_words(ctypes.byref(plan), nb)
    plan = _fake_plan(13, x4=False)
    N, ell, K = 1 << 13, plan.ell, plan.K
    pair, poly = 2 * (ell + K) * N, ell * N
    md = lambda count: lib.lf_ks_moddown_ws_words(count, ell, K, N)
    for nb in (0, 3, 63):
        assert ws(plan, nb, 1) == single(plan, nb) > 0
        assert ws(plan, nb, 64) == ws(plan, nb, 5) == ws(plan, nb, 4)
        assert ws(plan, nb, 3) == ws(plan, nb, 2)
        for g in (2, 4):   # per member its pairs, then w, the mod-down's results and the larger mod-down workspace
            assert ws(plan, nb, g) == g * pair * (nb + 1 + S_PAIRS + 1) + g * poly + 2 * g * poly + max(md(g), md(2 * g))
        assert ws(plan, nb, 4) > ws(plan, nb, 2) > ws(plan, nb, 1)
    assert [ws(plan, 64, n) for n in (1, 2, 4)] == [0, 0, 0]              # more baby keys than slots
    assert ws(plan, -1, 4) == 0
    assert [ws(plan, 3, n) for n in (0, -1, 65)] == [0, 0, 0]             # a refused nct
    assert lib.lf_linear_transform_bsgs_batch_ws_words(None, 3, 4) == 0
    for logN in (12, 18):
        assert ws(_fake_plan(logN, x4=False), 3, 4) == 0                  # a refused plan
    two, one = _fake_plan(13, max_nct=2), _fake_plan(13, max_nct=1)       # the plan bounds the group
    assert [ws(two, 3, n) for n in (1, 2, 4, 64)] == [single(two, 3)] + [ws(plan, 3, 2)] * 3
    assert [ws(one, 3, n) for n in (1, 4, 64)] == [single(one, 3)] * 3


def test_c_entry_refuses_bad_arguments_before_any_launch():
    """LF_ERR_ARG from the arguments alone (dummy pointers that are never dereferenced; no call here would pass the checks):
    what lf_linear_transform_bsgs refuses, nct < 1 or > LF_LT_BATCH_MAX_CTS, a NULL among the pointer arrays or their entries,
    a workspace that is NULL, misaligned or too small."""
    from liberate_fhe_amd._native import LF_LT_BATCH_MAX_CTS, lib
    dummy = ctypes.c_void_p(64)
    arr = (ctypes.c_void_p * 4)(64, 64, 64, 64)
    plan = _fake_plan(13)
    N2 = 2 << 13
    i64 = lambda v: (ctypes.c_int64 * max(len(v), 1))(*v)

    def call(nct, pl=plan, bexp=(3, 5), gexp=(0, 9), counts=(2, 1), slots=(0, 2, 1), ws=dummy, short=0, **kw):
        a = dict(c0=arr, c1=arr, out0=arr, out1=arr, bkeys=arr, gkeys=arr, pt=dummy, scales=dummy)
        a.update(kw)
        words = lib.lf_linear_transform_bsgs_batch_ws_words(ctypes.byref(pl), len(bexp), max(1, min(nct, 64))) - short
        return lib.lf_linear_transform_bsgs_batch(ctypes.byref(pl), nct, a["c0"], a["c1"], len(bexp), i64(bexp), a["bkeys"], len(gexp),
                                                  i64(gexp), a["gkeys"], 0, 0, 0, 0, a["pt"], 3 << 13, i64(counts), i64(slots),
                                                  a["scales"], 0, ws, words, a["out0"], a["out1"], None)

    nul = (ctypes.c_void_p * 4)(64, 64, 64, None)
    assert call(0) == call(-1) == call(LF_LT_BATCH_MAX_CTS + 1) == LF_ERR_ARG
    for name in ("c0", "c1", "out0", "out1"):
        assert call(4, **{name: None}) == LF_ERR_ARG, name
        assert call(4, **{name: nul}) == LF_ERR_ARG, name
    assert call(4, ws=None) == LF_ERR_ARG
    assert call(4, ws=ctypes.c_void_p(72)) == LF_ERR_ARG                  # 8 bytes off the alignment
    assert call(4, short=1) == call(2, short=1) == call(1, short=1) == LF_ERR_ARG
    # what the single entry refuses
    assert call(4, bexp=(3, 4)) == LF_ERR_ARG                             # an even exponent
    assert call(4, gexp=(0, N2 + 1)) == LF_ERR_ARG                        # >= 2N
    assert call(4, gexp=(9, 0)) == LF_ERR_ARG                             # a late giant step 0
    assert call(4, slots=(0, 3, 1)) == LF_ERR_ARG                         # a baby slot out of range
    assert call(4, slots=(2, 0, 1)) == LF_ERR_ARG                         # not ascending inside its giant step
    assert call(4, counts=(3, 0)) == LF_ERR_ARG                           # a giant step without diagonals
    assert call(4, bkeys=nul, bexp=(3, 5, 7, 9), slots=(0, 4, 1)) == LF_ERR_ARG   # a NULL key
    assert call(4, pt=None) == call(4, scales=None) == LF_ERR_ARG
    one = _fake_plan(13)
    one.ell = 1                                                           # no level left to rescale into
    assert call(4, pl=one) == LF_ERR_ARG
    assert call(4, pl=_fake_plan(12)) == LF_ERR_ARG


def test_the_group_baby_kernel_uses_no_scratch():
    """Every instantiation of ks_inner_babyb_kernel (4 and 2 ciphertexts x raw / planes key x raw / planes digits) exists with
    scratch 0 and no spill, at no fewer waves per SIMD than the single kernel of four keys; the tracked table lists them as built."""
    import __graft_entry__ as g
    res = {r["kernel"]: r for r in g.kernel_resources()}
    by = {k: r for k, r in res.items() if k.startswith("ks_inner_babyb_kernel<")}
    want = [f"ks_inner_babyb_kernel<{nct}, {pl}, {dpl}>" for nct in (4, 2) for pl in ("true", "false") for dpl in ("true", "false")]
    assert sorted(by) == sorted(want)
    for k in want:
        assert by[k]["scratch"] == 0 and by[k]["vgpr_spill"] == 0 and by[k]["sgpr_spill"] == 0, by[k]
        single = res["ks_inner_baby_kernel<4, " + k.split(", ", 1)[1]]
        assert by[k]["occupancy"] >= single["occupancy"] >= 3, (by[k], single)
    tracked = open(os.path.join(ROOT, "profiles", "r06_kernel_resources.txt")).read()
    for k, r in by.items():
        line = next(ln for ln in tracked.splitlines() if ln[18:76].strip() == k)
        f = line.split()
        assert (int(f[-7]), int(f[-3]), int(f[-1])) == (r["vgprs"], r["scratch"], r["occupancy"]), line


def test_batch_equals_the_loop_on_the_checker_engine(checker, monkeypatch):
    """The contract, on the backend without the entry: a list with a repeated ciphertext gives the loop's words in order, and a
    missing giant-step key is refused, named by its step, before anything is encoded."""
    from liberate_fhe_amd.fhe.presets import errors
    eng = checker
    assert not hasattr(eng.backend, "linear_transform_bsgs_batch_native")
    level = 0
    diags = synth.diagonals_bsgs(eng, 11, level, (0, 1, 2, 5, 6, 9), 4)
    keys, babies, giants = bsgs_keys(eng, diags)
    cts = [synth.ciphertext(eng, 70 + i, level) for i in range(2)]
    want = [eng.linear_transform(ct, diags, keys) for ct in cts]
    got = eng.linear_transform_batch([cts[0], cts[1], cts[0]], diags, keys)
    assert len(got) == 3 and got[0] is not got[2]
    assert all(same(g, w) for g, w in zip(got, want + [want[0]]))
    monkeypatch.setattr(eng, "encode_diagonals", lambda *a, **kw: pytest.fail("encode_diagonals was reached"))
    missing = {s: k for s, k in keys.items() if s != max(giants)}
    with pytest.raises(errors.NotMatchType) as e:
        eng.linear_transform_batch(cts, diags, missing)
    assert f"step {max(giants)}" in str(e.value)


class FakeNative:
    """Marks what the engine sends through the batched baby-step / giant-step entry; everything else is the checker backend's."""
    native_ops = True
    lt_batch_max_cts = 64
    bsgs_max_baby_keys = 63

    def __init__(self, inner):
        self._inner, self.batches, self.args = inner, [], []

    def __getattr__(self, name):
        return getattr(self._inner, name)

    def linear_transform_bsgs_batch_ws_words(self, plan, nb, nct):
        return 0

    def linear_transform_bsgs_batch_native(self, plan, c0s, c1s, bexp, bkeys, gexp, gkeys, first_part, row_off, pack, counts, slots,
                                           scales, round_at, outs, ws):
        self.batches.append([t.data_ptr() for t in c0s])
        self.args.append((list(bexp), list(gexp), list(counts), list(slots), len(bkeys), [k is None for k in gkeys]))
        for j, o in enumerate(outs):
            o.fill_(1000 * len(self.batches) + j)


def strided_inplace(ct):
    for comp in range(2):
        t = ct.data[comp][0]
        wide = torch.zeros((t.shape[0], 2 * t.shape[1]), dtype=t.dtype)
        wide[:, ::2] = t
        ct.data[comp][0] = wide[:, ::2]
        assert not ct.data[comp][0].is_contiguous()


def test_groups_stragglers_and_sizes_over_a_marker_backend(checker, monkeypatch):
    """Seven ciphertexts, the second and the fifth not contiguous: the five that qualify give ONE native call of 4, the fifth of
    them and the two that are not contiguous take linear_transform, every output at its input's index; the call carries what
    the single call carries; a size left out of lt_bsgs_batch_sizes sends its ciphertexts to the loop."""
    from liberate_fhe_amd.fhe import encdec
    eng = checker
    level, n1, steps = 0, 4, (1, 2, 5, 6, 9)
    diags = synth.diagonals_bsgs(eng, 4, level, steps, n1)
    keys, babies, giants = bsgs_keys(eng, diags)
    cts = [synth.ciphertext(eng, 30 + i, level) for i in range(7)]
    for i in (1, 4):
        strided_inplace(cts[i])
    want = [eng.linear_transform(ct, diags, keys) for ct in cts]

    def patched(sizes=None):
        fake = FakeNative(eng.backend)
        monkeypatch.setattr(eng, "backend", fake)
        monkeypatch.setattr(eng, "_native_level", lambda lvl: 0)
        monkeypatch.setattr(eng, "_op_plan", lambda lvl, d, nct=1: (type("P", (), {"ell": eng._rows(0, lvl, False)})(), None, 0, 0))
        if sizes is not None:
            monkeypatch.setattr(eng, "lt_bsgs_batch_sizes", sizes)
        return fake

    fake = patched((4, 2))
    seen_single = []
    monkeypatch.setattr(eng, "linear_transform", lambda ct, dg, ks: seen_single.append(ct) or want[[id(c) for c in cts].index(id(ct))])
    got = eng.linear_transform_batch(cts, diags, keys)
    monkeypatch.undo()
    assert fake.batches == [[cts[i].data[0][0].data_ptr() for i in (0, 2, 3, 5)]]
    assert [id(c) for c in seen_single] == [id(cts[i]) for i in (1, 4, 6)]
    for j, i in enumerate((0, 2, 3, 5)):
        assert got[i].level == level + 1 and int(got[i].data[0][0][0, 0]) == 1000 + j and int(got[i].data[1][0][0, 0]) == 1000 + j
    for i in (1, 4, 6):
        assert got[i] is want[i]
    # baby keys 1 and 2 (slots 1, 2), giant steps 0, 4, 8 with the diagonals (1, 2), (5, 6), (9)
    N = eng.ctx.N
    bexp, gexp, counts, slots, nbk, nokey = fake.args[0]
    assert bexp == [encdec.galois_exponent(N, b) for b in (1, 2)] and nbk == 2
    assert gexp == [0] + [encdec.galois_exponent(N, g) for g in (4, 8)] and nokey == [True, False, False]
    assert counts == [2, 2, 1] and slots == [1, 2, 1, 2, 1]
    # sizes: (4,) alone sends three ciphertexts to the loop, (2,) alone makes one call of two pairs out of five
    for sizes, members, calls in (((4,), (0, 2, 3), []), ((2,), (0, 2, 3, 5, 6), [4]), ((), (0, 2, 3, 5), [])):
        fake = patched(sizes)
        monkeypatch.setattr(eng, "linear_transform", lambda ct, dg, ks: "loop")
        got = eng.linear_transform_batch([cts[i] for i in members], diags, keys)
        monkeypatch.undo()
        assert [len(b) for b in fake.batches] == calls, sizes
        assert [g == "loop" for g in got] == [j >= sum(calls) for j in range(len(members))], sizes
