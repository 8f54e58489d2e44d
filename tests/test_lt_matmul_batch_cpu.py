"""lt_matmul_batch (a matrix of linear transforms times B token vectors of ciphertexts; lf_lt_matmul_batch) without a GPU: the
engine's host logic on the checker backend against the loop of lt_matmul that defines its words, the easy cases, the refusals
(in the middle token, before anything is encoded or run), the C entry's argument checks and the new kernels' resources."""
import ctypes
import os
import re

import pytest
import torch

from liberate_fhe_amd.utils import synth
from tests.test_cc_dot_cpu import lazy_ciphertext, same
from tests.test_linear_transform_bsgs_cpu import _fake_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = (1, 2, 5)
_ENGINES = {}


def checker(logN):
    """(the checker engine at logN, its rotation keys), built once"""
    if logN not in _ENGINES:
        from liberate_fhe_amd.fhe import ckks_engine
        from tests.oracle_backend import OracleBackend
        eng = ckks_engine(devices=["cpu"], backend=OracleBackend(), logN=logN, num_scales=5, num_special_primes=2, is_secured=False)
        _ENGINES[logN] = eng, {s: synth.key_switch_key(eng, 40 + s, origin=f"rotation key:{s}") for s in STEPS}
    return _ENGINES[logN]


def layer_of(eng, shape, level, seed=5):
    """(W, X) of 3 tokens: "1x1"; "2x3" with a None block; "unused": 2 x 2 whose column 1 no output uses; "mixed": encoded and
    mapping blocks, one mapping object twice.  Token 1 carries lazy words, token 2 repeats objects of token 0."""
    D = [synth.diagonals(eng, seed + j, level, st) for j, st in enumerate(((0, 1, 5), (2,), (0,)))]
    mapping = {1: [0.5, -0.25], 0: [1.0, 2.0, -1.0]}
    W = {"1x1": [[D[0]]],
         "2x3": [[D[0], D[1], None], [None, D[2], D[0]]],
         "unused": [[D[0], None], [D[1], None]],
         "mixed": [[mapping, D[1]], [D[2], mapping], [{5: [1.0]}, None]]}[shape]
    k_in = len(W[0])
    pool = [synth.ciphertext(eng, seed + 20 + i, level) for i in range(3)] + [lazy_ciphertext(eng, seed + 30, level)]
    X = [[pool[i % 3] for i in range(k_in)], [pool[3]] + [pool[2]] * (k_in - 1), [pool[(i + 1) % 3] for i in range(k_in)]]
    return W, X


def encoded_matrix(eng, W, X, keys):
    """(lt_matmul_batch(W, X, keys), W with every plain mapping replaced by the object the call encoded for it, those objects in
    the order they were made): tests/test_lt_matmul_cpu.py's helper for the batch, tokens of one level."""
    made, real = [], eng.encode_diagonals
    eng.encode_diagonals = lambda *a, **k: (made.append(real(*a, **k)), made[-1])[1]
    try:
        got = eng.lt_matmul_batch(W, X, keys)
    finally:
        del eng.encode_diagonals
    by_id = {}
    for row in W:
        for b in row:
            if isinstance(b, dict) and id(b) not in by_id and len(by_id) < len(made):
                by_id[id(b)] = made[len(by_id)]                     # (encoded in row-major order, each mapping once)
    return got, [[by_id.get(id(b), b) if isinstance(b, dict) else b for b in row] for row in W], made


@pytest.mark.parametrize("shape", ["1x1", "2x3", "unused", "mixed"])
@pytest.mark.parametrize("logN", [12, 13])
def test_batch_equals_the_loop_on_the_checker_engine(logN, shape):
    """The checker backend has no batch entry: every token takes lt_matmul, and the result is the loop's, as lists and as
    iterators; a mapping block is encoded once per call (per distinct object), not once per token — and since encode draws its
    rounding at random, the loop it is compared with reads the objects the call encoded."""
    eng, keys = checker(logN)
    assert not hasattr(eng.backend, "lt_matmul_batch_native")
    level = 0 if shape != "2x3" else 2
    W, X = layer_of(eng, shape, level)
    got, We, made = encoded_matrix(eng, W, X, keys)
    assert len(made) == (2 if shape == "mixed" else 0)
    want = [eng.lt_matmul(We, cts, keys) for cts in X]
    assert isinstance(got, list) and len(got) == 3 and all(isinstance(g, list) and len(g) == len(W) for g in got)
    assert all(o.level == level + 1 for g in got for o in g)
    assert all(same(a, w) for g, ws in zip(got, want) for a, w in zip(g, ws)), (logN, shape)
    got = eng.lt_matmul_batch(iter([iter(row) for row in We]), (iter(cts) for cts in X), iter(list(keys.values())))
    assert all(same(a, w) for g, ws in zip(got, want) for a, w in zip(g, ws))
    assert set(eng.lt_matmul_steps(W)) <= set(STEPS)                               # (lt_matmul_steps still names the keys)


def test_easy_cases():
    """An empty X is an empty list (the loop checks nothing either); one ciphertext object in every token and position; tokens
    of different levels under a matrix of mappings, each level encoded once."""
    eng, keys = checker(12)
    d0 = synth.diagonals(eng, 3, 0, (0, 1))
    assert eng.lt_matmul_batch([[d0]], [], keys) == [] and eng.lt_matmul_batch([[d0]], iter(()), keys) == []
    assert eng.lt_matmul_batch([], [], keys) == []
    ct = synth.ciphertext(eng, 9, 0)
    got = eng.lt_matmul_batch([[d0, d0]], [[ct, ct]] * 3, keys)
    want = eng.lt_matmul([[d0, d0]], [ct, ct], keys)[0]
    assert len(got) == 3 and all(len(g) == 1 and same(g[0], want) for g in got)
    W = [[{0: [1.0, -2.0], 2: [0.5]}]]
    X = [[synth.ciphertext(eng, 10 + t, lvl)] for t, lvl in enumerate((1, 0, 1))]
    made, real = [], eng.encode_diagonals
    eng.encode_diagonals = lambda *a, **k: (made.append(real(*a, **k)), made[-1])[1]
    try:
        got = eng.lt_matmul_batch(W, X, keys)
    finally:
        del eng.encode_diagonals
    assert sorted(m.level for m in made) == [0, 1]
    assert [g[0].level for g in got] == [2, 1, 2]
    by_level = {m.level: m for m in made}
    assert all(same(g[0], eng.lt_matmul([[by_level[cts[0].level]]], cts, keys)[0]) for g, cts in zip(got, X))


def test_refusals_come_before_anything_is_encoded_or_run(monkeypatch):
    """Each refusal of lt_matmul in the MIDDLE of three tokens is refused for the whole call with the loop's first error, with
    lt_matmul, encode_diagonals, the native hooks, the ntt ops and every allocation patched to record: none is reached."""
    from liberate_fhe_amd.fhe.presets import errors
    eng, keys = checker(12)
    top = eng.num_levels - 1
    c0, c1, ctop = (synth.ciphertext(eng, 60 + i, lvl) for i, lvl in enumerate((0, 1, top)))
    d0, dtop = synth.diagonals(eng, 3, 0, (0, 1, 5)), synth.diagonals(eng, 3, top, (0,))
    bsgs = synth.diagonals_bsgs(eng, 3, 0, (0, 1, 5), 4)
    ntt = eng._new(c0.data, c0.origin, level=0, ntt_state=True)
    special = eng._new(c0.data, c0.origin, level=0, include_special=True)
    mapping = {0: [1.0], 1: [2.0]}
    cases = [
        (ValueError, [[d0]], [c0, c0], keys),                                      # a wrong number of ciphertexts
        (ValueError, [[d0, mapping]], [c0], keys),
        (errors.NotMatchDataStructState, [[d0, mapping]], [c0, c1], keys),         # a level mismatch inside the token
        (errors.NotMatchType, [[d0, mapping]], [c0, c0], [keys[1]]),               # a missing key (step 5)
        (errors.NotMatchType, [[mapping]], [c0], []),
        (errors.NotMatchType, [[mapping]], [d0], keys),                            # diagonals where a ciphertext belongs
        (NotImplementedError, [[bsgs]], [c0], keys),                               # a BSGS block
        (NotImplementedError, [[mapping, bsgs]], [c0, c0], keys),
        (NotImplementedError, [[mapping]], [ntt], keys),                           # an NTT-domain ciphertext
        (NotImplementedError, [[d0, None]], [c0, special], keys),                  # special limbs
        (errors.MaximumLevelError, [[mapping]], [ctop], keys),                     # a token at the last level
    ]
    for exc, W, cts, ks in cases:                                                  # what lt_matmul itself says, before anything is patched
        with pytest.raises(exc):
            eng.lt_matmul(W, cts, ks)
    calls = []

    def boom(name):
        def f(*a, **k):
            calls.append(name)
            raise AssertionError(name + " reached")
        return f

    for name in ("lt_matmul", "linear_transform", "encode_diagonals", "_lt_matmul_encode", "_lt_matmul_native_args", "_lt_matmul_native",
                 "_lt_matmul_steps", "rescale", "clone", "_ws", "_op_plan", "_ks_tables", "_ks_digits_exchanged", "_diag_pack", "_key_pack",
                 "_lt_chat", "_lt_forward", "_lt_inner", "_lt_giant", "_lt_tail"):
        monkeypatch.setattr(eng, name, boom(name))
    for name in ("lt_matmul_native", "lt_matmul_batch_native", "lt_matmul_ws_words", "lt_matmul_batch_ws_words", "galois", "ntt", "intt",
                 "ks_fwd", "ks_tail", "ks_inner", "ks_moddown_ws"):
        monkeypatch.setattr(eng.backend, name, boom(name), raising=False)
    monkeypatch.setattr(eng.backend, "lt_matmul_batch_sizes", (4, 2), raising=False)
    for name in ("enter_ntt", "mont_mult", "mont_add", "mont_enter", "intt_exit_reduce"):
        monkeypatch.setattr(eng.ntt, name, boom(name))
    real_empty, real_zeros = torch.empty, torch.zeros
    monkeypatch.setattr(torch, "empty", lambda *a, **k: (calls.append("empty"), real_empty(*a, **k))[1])
    monkeypatch.setattr(torch, "zeros", lambda *a, **k: (calls.append("zeros"), real_zeros(*a, **k))[1])
    for exc, W, cts, ks in cases:
        good = [c0] * len(W[0])
        with pytest.raises(exc):
            eng.lt_matmul_batch(W, [good, cts, good], ks)
        with pytest.raises(exc):
            eng.lt_matmul_batch(iter(iter(row) for row in W), iter([iter(good), iter(cts), good]), ks)
    with pytest.raises(errors.NotMatchDataStructState):                           # a token beside the level of an encoded block
        eng.lt_matmul_batch([[d0]], [[c0], [c1], [c0]], keys)
    with pytest.raises(errors.MaximumLevelError):                                 # the last level, under an encoded block of it
        eng.lt_matmul_batch([[dtop]], [[ctop], [ctop], [ctop]], keys)
    # the error is the one the loop would have raised first: token 0's operands, then the keys, then token 1's operands
    with pytest.raises(ValueError):
        eng.lt_matmul_batch([[d0]], [[c0], [c0, c0], [ntt]], keys)
    with pytest.raises(NotImplementedError):
        eng.lt_matmul_batch([[d0]], [[c0], [ntt], [c0, c0]], keys)
    with pytest.raises(errors.NotMatchType, match="step 5"):
        eng.lt_matmul_batch([[d0]], [[c0], [ntt], [c0]], [keys[1]])
    with pytest.raises(NotImplementedError):
        eng.lt_matmul_batch([[d0]], [[ntt], [c0], [c0]], [keys[1]])
    with pytest.raises(ValueError):                                                # the matrix before any token
        eng.lt_matmul_batch([[d0], [d0, d0]], [[ntt]], keys)
    assert calls == []
    monkeypatch.undo()
    out = eng.lt_matmul_batch([[d0, None], [None, mapping]], [[c0, c0], [c0, c0]], keys)       # and the engine still works
    assert [[o.level for o in tok] for tok in out] == [[1, 1], [1, 1]]
    assert same(out[1][0], eng.linear_transform(c0, d0, keys))


def test_c_entry_refuses_bad_arguments_before_any_launch():
    """lf_lt_matmul_batch_ws_words: nt (nb_max + 1 + k_out) pairs + the mod-down's buffers and workspace for g = min(nt k_out, 4)
    sums, lf_lt_matmul_ws_words for nt = 1, 0 for a NULL or refused plan, nt outside {1, 2, 4} or above max_nct, k_out above
    LF_LT_MATMUL_MAX_OUTPUTS.  lf_lt_matmul_batch returns LF_ERR_ARG from its arguments alone (dummy pointers that are never
    dereferenced; no call here would pass the checks).  The Python copies of LF_LT_MATMUL_BATCH_MAX_TOKENS are the header's."""
    from liberate_fhe_amd import _native
    from liberate_fhe_amd._native import lib, EXPORTED
    from liberate_fhe_amd.fhe.backend import HipBackend
    LF_ERR_ARG = 10001
    assert "lf_lt_matmul_batch" in EXPORTED and "lf_lt_matmul_batch_ws_words" in EXPORTED
    header = open(os.path.join(ROOT, "include", "ckks_hip.h")).read()
    TMAX = int(re.search(r"#define LF_LT_MATMUL_BATCH_MAX_TOKENS (\d+)", header).group(1))
    OMAX = int(re.search(r"#define LF_LT_MATMUL_MAX_OUTPUTS (\d+)", header).group(1))
    KMAX = int(re.search(r"#define LF_BSGS_MAX_BABY_KEYS (\d+)", header).group(1))
    assert TMAX == _native.LF_LT_MATMUL_BATCH_MAX_TOKENS == HipBackend.lt_matmul_batch_max_tokens == 4
    assert HipBackend.lt_matmul_batch_sizes == (4, 2) and max(HipBackend.lt_matmul_batch_sizes) <= TMAX

    def plan_of(logN, max_nct=4):
        plan = _fake_plan(logN)
        plan.max_nct = max_nct
        return plan

    for logN in (13, 17):
        plan = plan_of(logN)
        N, rows, ell, K = 1 << logN, 3, 2, 1
        for nt in (1, 2, 4):
            for nb in (0, 7, KMAX):
                for k_out in (1, 2, 3, 5, OMAX):
                    g = min(nt * k_out, 4)
                    want = 2 * rows * N * nt * (nb + 1 + k_out) + 2 * g * ell * N + lib.lf_ks_moddown_ws_words(2 * g, ell, K, N)
                    assert lib.lf_lt_matmul_batch_ws_words(ctypes.byref(plan), nb, k_out, nt) == want, (logN, nt, nb, k_out)
                    if nt == 1:
                        assert want == lib.lf_lt_matmul_ws_words(ctypes.byref(plan), nb, k_out)
    plan = plan_of(13)
    for nb, k_out, nt in ((-1, 1, 2), (KMAX + 1, 1, 2), (0, 0, 2), (0, OMAX + 1, 2), (0, OMAX + 1, 1), (1, 1, 0), (1, 1, -1), (1, 1, 3),
                          (1, 1, 5), (1, 1, 8)):
        assert lib.lf_lt_matmul_batch_ws_words(ctypes.byref(plan), nb, k_out, nt) == 0, (nb, k_out, nt)
    assert lib.lf_lt_matmul_batch_ws_words(ctypes.byref(plan_of(13, 2)), 1, 1, 4) == 0              # nt above max_nct
    assert lib.lf_lt_matmul_batch_ws_words(ctypes.byref(plan_of(13, 1)), 1, 1, 2) == 0
    assert lib.lf_lt_matmul_batch_ws_words(ctypes.byref(plan_of(13, 2)), 1, 1, 2) > 0
    for logN in (12, 18):                                                                            # a refused plan
        assert lib.lf_lt_matmul_batch_ws_words(ctypes.byref(plan_of(logN)), 1, 1, 2) == 0
    assert lib.lf_lt_matmul_batch_ws_words(None, 1, 1, 2) == 0

    dummy = ctypes.c_void_p(64)
    stride = 3 << 13

    def i64(values):
        return (ctypes.c_int64 * max(1, len(values)))(*values)

    def ptrs(count, null_at=()):
        arr = (ctypes.c_void_p * max(count, 1))(*([64] * max(count, 1)))
        for at in null_at:
            arr[at] = None
        return arr

    # 2 tokens of 2 inputs x 2 outputs: column 0 has keyed steps (exponents 3, 5), column 1 none; blocks (0,0): slots 0,1,2;
    # (0,1): NULL; (1,0): slot 2; (1,1): slot 0
    def call(plan=plan, nt=2, k_in=2, k_out=2, scales=dummy, ws=dummy, ws_words=1 << 40, fmt=0, **over):
        a = {"ins": ptrs(16), "keys": ptrs(4), "pts": ptrs(4, [1]), "out0": ptrs(8), "out1": ptrs(8), "ncol": i64((2, 0)),
             "exps": i64((3, 5)), "strides": i64((stride, 0, stride, stride)), "counts": i64((3, 0, 1, 1)), "bidx": i64((0, 1, 2, 2, 0))}
        for name, value in over.items():
            assert name in a
            a[name] = value if value is None or isinstance(value, ctypes.Array) else i64(value)
        return lib.lf_lt_matmul_batch(ctypes.byref(plan) if plan is not None else None, nt, k_in, k_out, a["ins"], a["ncol"], a["exps"],
                                      a["keys"], 0, 0, 0, fmt, a["pts"], a["strides"], a["counts"], a["bidx"], scales, 0, ws, ws_words,
                                      a["out0"], a["out1"], None)

    need = lib.lf_lt_matmul_batch_ws_words(ctypes.byref(plan), 2, 2, 2)
    assert need > 0
    assert call(plan=None) == LF_ERR_ARG
    for nt in (0, -1, 3, 5, 8):
        assert call(nt=nt) == LF_ERR_ARG, nt
    assert call(plan=plan_of(13, 1)) == LF_ERR_ARG and call(plan=plan_of(13, 2), nt=4) == LF_ERR_ARG   # nt above max_nct
    for logN in (12, 18):
        assert call(plan=plan_of(logN)) == LF_ERR_ARG
    nopr = plan_of(13)
    nopr.PR = None
    assert call(plan=nopr) == LF_ERR_ARG
    for nt in (1, 2, 4):                                                           # everything lf_lt_matmul refuses, for every nt
        assert call(nt=nt, k_in=0) == LF_ERR_ARG and call(nt=nt, k_out=OMAX + 1) == LF_ERR_ARG
        for name in ("ins", "ncol", "exps", "keys", "pts", "strides", "counts", "bidx", "out0", "out1"):
            assert call(nt=nt, **{name: None}) == LF_ERR_ARG, (nt, name)
        assert call(nt=nt, scales=None) == LF_ERR_ARG and call(nt=nt, fmt=2) == LF_ERR_ARG
        assert call(nt=nt, exps=(4, 5)) == LF_ERR_ARG and call(nt=nt, bidx=(1, 0, 2, 2, 0)) == LF_ERR_ARG
        assert call(nt=nt, pts=ptrs(4, [0, 1])) == LF_ERR_ARG                      # an output with no block
        assert call(nt=nt, ws=None) == LF_ERR_ARG and call(nt=nt, ws=ctypes.c_void_p(72)) == LF_ERR_ARG
        assert call(nt=nt, ws_words=lib.lf_lt_matmul_batch_ws_words(ctypes.byref(plan), 2, 2, nt) - 1) == LF_ERR_ARG
    for at in range(8):                                                            # a NULL among the pointers of either token
        assert call(ins=ptrs(16, [at])) == LF_ERR_ARG, at
    for at in range(4):
        assert call(out0=ptrs(8, [at])) == LF_ERR_ARG and call(out1=ptrs(8, [at])) == LF_ERR_ARG, at
    for at in range(16):
        assert call(nt=4, ins=ptrs(16, [at])) == LF_ERR_ARG, at
    for at in range(8):
        assert call(nt=4, out0=ptrs(8, [at])) == LF_ERR_ARG and call(nt=4, out1=ptrs(8, [at])) == LF_ERR_ARG, at
    # the pointers of an input no block uses are not among the checked ones, for any token (the call is still refused, by its
    # workspace, so nothing is launched)
    unused = dict(pts=ptrs(4, [1, 3]), counts=(3, 0, 1, 0), bidx=(0, 1, 2, 2), ins=ptrs(16, [2, 3, 6, 7]))
    assert call(ws_words=need - 1, **unused) == LF_ERR_ARG


def test_block_productsb_kernels_use_no_scratch():
    """lt_block_productsb_kernel<1 | 2 | 4, 2> exist in ckks_ks.hip under these names with scratch 0 and no spill, at least 4 waves
    per SIMD (streaming kernels, as lt_block_products_kernel), and the tracked table lists them as built; the launch code selects
    exactly these; lt_block_products_kernel<1 | 2 | 4> are still there."""
    import __graft_entry__ as g
    res = {r["kernel"]: r for r in g.kernel_resources()}
    want = [f"lt_block_productsb_kernel<{no}, 2>" for no in (1, 2, 4)]
    assert sorted(k for k in res if k.startswith("lt_block_productsb_kernel")) == sorted(want)
    assert all(f"lt_block_products_kernel<{no}>" in res for no in (1, 2, 4))
    tracked = open(os.path.join(ROOT, "profiles", "r06_kernel_resources.txt")).read()
    for k in want:
        r = res[k]
        assert r["file"] == "ckks_ks.hip" and r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["lds"] == 0, r
        assert r["occupancy"] >= 4, r
        line = next(ln for ln in tracked.splitlines() if ln[18:76].strip() == k)
        f = line.split()
        assert (int(f[-7]), int(f[-3]), int(f[-1])) == (r["vgprs"], r["scratch"], r["occupancy"]), line
