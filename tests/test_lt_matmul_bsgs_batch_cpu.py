"""lt_matmul_bsgs_batch (a matrix of baby-step / giant-step transforms times B token vectors of ciphertexts;
lf_lt_matmul_bsgs_batch) without a GPU: the engine's host logic on the checker backend against the loop of lt_matmul_bsgs that
defines its words, plain mappings, the refusals (in token 0 and in a later token, before anything is encoded or run), two logical
devices, the C entry's argument checks, its workspace query and the backend's names.  The op adds no kernel."""
import ctypes
import os
import re

import pytest
import torch

from liberate_fhe_amd.utils import synth
from tests.test_inner_sum_cpu import lazy_ciphertext
from tests.test_cc_dot_cpu import same
from tests.test_linear_transform_bsgs_cpu import _fake_plan
from tests.test_lt_matmul_bsgs_cpu import LT, N1, LAYOUT, keys_for, layer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def checker():
    from liberate_fhe_amd.fhe import ckks_engine
    from tests.oracle_backend import OracleBackend
    eng = ckks_engine(devices=["cpu"], backend=OracleBackend(), **LT)
    return eng, keys_for(eng)


def tokens(eng, level, B, k_in=3):
    """B token vectors at `level`: token 1 carries lazy words, token 3 IS token 0 (the same objects), token 4 repeats one
    ciphertext object in every position."""
    def tok(t):
        make = lazy_ciphertext if t == 1 else synth.ciphertext
        return [make(eng, 200 + 10 * t + i + 50 * level, level) for i in range(k_in)]
    X = [tok(t) for t in range(min(B, 3))]
    if B > 3:
        X.append(X[0])
    if B > 4:
        X.append([X[2][0]] * k_in)
    return X


@pytest.mark.parametrize("level", [0, 2, "L-2"])
def test_batch_equals_the_loop_on_the_checker_engine(checker, level):
    """The checker backend has no batch entry: every token takes lt_matmul_bsgs and keeps its place.  B = 0, 1, 3, 5 against the
    loop over five tokens computed once; one token is lazy, one repeated; lists and iterators alike."""
    eng, keys = checker
    assert not hasattr(eng.backend, "lt_matmul_bsgs_batch_call") and eng.lt_matmul_bsgs_batch_sizes == (4, 2)
    level = eng.num_levels - 2 if level == "L-2" else level
    W, _ = layer(eng, level)
    X = tokens(eng, level, 5)
    assert X[3] is X[0] and X[4][0] is X[4][1]
    want = [eng.lt_matmul_bsgs(W, cts, keys) for cts in X[:3]]
    want.append(want[0])
    want.append(eng.lt_matmul_bsgs(W, X[4], keys))
    assert eng.lt_matmul_bsgs_batch(W, [], keys) == [] and eng.lt_matmul_bsgs_batch(W, iter(()), keys, n1=N1) == []
    for B in (1, 3, 5):
        got = eng.lt_matmul_bsgs_batch(W, X[:B], keys) if B != 3 else \
            eng.lt_matmul_bsgs_batch(iter([iter(row) for row in W]), (iter(cts) for cts in X[:B]), iter(list(keys.values())), n1=N1)
        assert isinstance(got, list) and len(got) == B and all(isinstance(g, list) and len(g) == len(W) for g in got)
        assert all(o.level == level + 1 for g in got for o in g)
        for t in range(B):
            assert all(same(a, w) for a, w in zip(got[t], want[t])), (level, B, t)


def test_mixed_levels_and_mappings(checker):
    """Tokens at levels (0, 2, 0, 2, 0) under a matrix of {step: vector} mappings keep their order; a mapping is encoded once per
    level and per distinct object, with bsgs=n1; the result is that of the matrix with those very objects in place."""
    eng, keys = checker
    m1 = {5: [0.5, -0.25], 0: [1.0, 2.0, -1.0], 8: [0.125]}
    m2 = {1: [1.0], 12: [0.5]}
    W = [[m1, m2], [None, m1]]
    levels = (0, 2, 0, 2, 0)
    X = [[synth.ciphertext(eng, 300 + 2 * t + i, lvl) for i in range(2)] for t, lvl in enumerate(levels)]
    made, real = [], eng.encode_diagonals
    eng.encode_diagonals = lambda *a, **k: (made.append((real(*a, **k), a, k)), made[-1][0])[1]
    try:
        got = eng.lt_matmul_bsgs_batch(W, X, keys, n1=N1)
    finally:
        del eng.encode_diagonals
    assert [(a[0] is m, a[1], k) for (_, a, k), m in zip(made, (m1, m2, m1, m2))] == \
        [(True, 0, {"bsgs": N1})] * 2 + [(True, 2, {"bsgs": N1})] * 2
    enc = {(a[1], id(a[0])): obj for obj, a, _ in made}
    assert [[o.level for o in g] for g in got] == [[lvl + 1] * 2 for lvl in levels]
    for t, lvl in enumerate(levels):
        e1, e2 = enc[(lvl, id(m1))], enc[(lvl, id(m2))]
        want = eng.lt_matmul_bsgs([[e1, e2], [None, e1]], X[t], keys)
        assert all(same(a, w) for a, w in zip(got[t], want)), t


def test_refusals_come_before_anything_is_computed(checker, monkeypatch):
    """Each refusal of lt_matmul_bsgs, in token 0 and in a later token, is refused for the whole call with the loop's first error,
    with lt_matmul_bsgs, encode_diagonals, the native hooks, the ntt ops and every allocation patched to record: none is reached.
    The engine works afterwards."""
    from liberate_fhe_amd.fhe.presets import errors
    eng, keys = checker
    n = eng.num_slots
    top = eng.num_levels - 1
    c0, c1, ctop = (synth.ciphertext(eng, 60 + i, lvl) for i, lvl in enumerate((0, 1, top)))
    d0, d1 = synth.diagonals_bsgs(eng, 3, 0, (0, 1, 5), 4), synth.diagonals_bsgs(eng, 3, 1, (0, 1), 4)
    d8 = synth.diagonals_bsgs(eng, 3, 0, (0, 1, 9), 8)
    dtop = synth.diagonals_bsgs(eng, 3, top, (0,), 4)
    flat = synth.diagonals(eng, 3, 0, (0, 1, 5))
    ntt = eng._new(c0.data, c0.origin, level=0, ntt_state=True)
    special = eng._new(c0.data, c0.origin, level=0, include_special=True)
    cap_keys, cap_in = eng.lt_matmul_max_column_keys, eng.lt_matmul_max_inputs
    wide = {s: [1.0] for s in range(1, cap_keys + 2)}
    split = [[{s: [1.0] for s in range(1, 40)}], [{s: [1.0] for s in range(30, 70)}]]
    many_keys = {s: k._replace(origin=f"rotation key:{s}") for s, k in zip(range(1, 80), [keys[1]] * 80)}
    calls = []

    def boom(name):
        def f(*a, **k):
            calls.append(name)
            raise AssertionError(name + " reached")
        return f

    for name in ("lt_matmul_bsgs", "linear_transform", "encode_diagonals", "_lt_matmul_encode", "_lt_matmul_native_args",
                 "_lt_matmul_native", "_lt_matmul_steps", "rescale", "clone", "_ws", "_op_plan", "_ks_tables", "_ks_digits_exchanged",
                 "_diag_pack", "_key_pack", "_lt_chat", "_lt_forward", "_lt_inner", "_lt_giant", "_lt_tail"):
        monkeypatch.setattr(eng, name, boom(name))
    for name in ("lt_matmul_bsgs_native", "lt_matmul_bsgs_batch_call", "lt_matmul_bsgs_ws_words", "lt_matmul_bsgs_batch_ws_words",
                 "lt_matmul_native", "galois", "ntt", "intt", "ks_fwd", "ks_tail", "ks_inner", "ks_moddown_ws"):
        monkeypatch.setattr(eng.backend, name, boom(name), raising=False)
    monkeypatch.setattr(eng.backend, "lt_matmul_bsgs_batch_sizes", (4, 2), raising=False)
    for name in ("enter_ntt", "mont_mult", "mont_add", "mont_enter", "intt_exit_reduce"):
        monkeypatch.setattr(eng.ntt, name, boom(name))
    real_empty, real_zeros = torch.empty, torch.zeros
    monkeypatch.setattr(torch, "empty", lambda *a, **k: (calls.append("empty"), real_empty(*a, **k))[1])
    monkeypatch.setattr(torch, "zeros", lambda *a, **k: (calls.append("zeros"), real_zeros(*a, **k))[1])
    # (error, W, the refused token, keys, n1[, a token the loop accepts before it: c0 in every column where none is given]):
    # the cases of tests/test_lt_matmul_bsgs_cpu.py
    cases = [
        (ValueError, [], [c0], keys, None),                                        # W empty
        (ValueError, [[d0]], [], keys, None),                                      # cts empty
        (ValueError, [[]], [], keys, 4),
        (ValueError, [[d0, d0], [d0]], [c0, c0], keys, None),                      # ragged
        (ValueError, [[d0], [d0]], [c0, c0], keys, None),                          # len(W[o]) != len(cts)
        (ValueError, [[d0, d0, d0]], [c0, c0], keys, None),
        (ValueError, [[d0, None], [None, None]], [c0, c0], keys, None),            # a row with no block
        (ValueError, [[d0, d8]], [c0, c0], many_keys, None),                       # blocks of different n1
        (ValueError, [[d0], [d8]], [c0], many_keys, None),
        (ValueError, [[d0]], [c0], keys, 8),                                       # the argument disagrees with the objects
        (ValueError, [[d0, {1: [1.0]}]], [c0, c0], keys, 2),
        (ValueError, [[{0: [1.0]}]], [c0], keys, None),                            # mappings only and no n1
        (ValueError, [[{0: [1.0]}, None], [None, {1: [1.0]}]], [c0, c0], keys, None),
        (ValueError, [[{0: [1.0]}]], [c0], keys, 0),                               # no n1 at all
        (ValueError, [[d0]], [c0], keys, 2.5),
        (ValueError, [[wide]], [c0], many_keys, 128),                              # more keyed baby steps in a column than the cap
        (ValueError, split, [c0], many_keys, 128),
        (ValueError, [[d0] * (cap_in + 1)], [c0] * (cap_in + 1), keys, None),      # k_in above its cap
        (ValueError, [[{}]], [c0], keys, 4),                                       # a mapping without a diagonal
        (ValueError, [[{1: [1.0], 1 + n: [2.0]}]], [c0], keys, 4),                 # the same step twice mod num_slots
        (errors.NotMatchType, [[flat]], [c0], keys, None),                         # a flat-tagged object
        (errors.NotMatchType, [[d0, flat]], [c0, c0], keys, 4),
        (errors.NotMatchType, [[c0]], [c0], keys, None),                           # a ciphertext where diagonals belong
        (errors.NotMatchType, [[d0]], [d0], keys, None),                           # .. and the other way round
        (errors.NotMatchType, [[d0, None]], [c0, None], keys, None),               # (a None ciphertext, even in an unused column)
        (errors.NotMatchType, [[3.5]], [c0], keys, 4),
        (errors.NotMatchType, [[d0]], [c0], [keys[1], keys[4], synth.key_switch_key(eng, 8)], None),   # a key of another kind
        (errors.NotMatchType, [[d0]], [c0], [keys[1]], None),                      # a missing giant key (step 4)
        (errors.NotMatchType, [[d0]], [c0], [keys[4]], None),                      # a missing baby key (step 1)
        (errors.NotMatchType, [[d0]], [c0], {1: keys[1], 5: many_keys[5]}, None),  # the flat form's keys do not serve
        (errors.NotMatchType, [[{0: [1.0], 17: [1.0]}]], [c0], keys, 4),           # .. for a plain mapping (giant step 16)
        (errors.NotMatchDataStructState, [[d1]], [c0], keys, None, [c1]),          # a block of another level
        (errors.NotMatchDataStructState, [[d0, None], [d0, d1]], [c0, c0], keys, None),
        (errors.NotMatchDataStructState, [[d0, d0]], [c0, c1], keys, None),        # ciphertexts of different levels
        (errors.NotMatchDataStructState, [[d0, None]], [c0, c1], keys, None),      # (an unused column is still of the level)
        (errors.MaximumLevelError, [[dtop]], [ctop], keys, None, [ctop]),
        (errors.MaximumLevelError, [[{0: [1.0]}]], [ctop], keys, 4),
        (NotImplementedError, [[d0]], [ntt], keys, None),                          # an NTT-domain ciphertext
        (NotImplementedError, [[d0, None]], [c0, special], keys, None),            # special limbs
    ]
    for exc, W, cts, ks, n1, *rest in cases:
        good = rest[0] if rest else [c0] * (len(W[0]) if W else 1)
        with pytest.raises(exc):                                                   # in token 0
            eng.lt_matmul_bsgs_batch(W, [cts, good, good], ks, n1=n1)
        with pytest.raises(exc):                                                   # in a later token
            eng.lt_matmul_bsgs_batch(W, [good, cts, good], ks, n1=n1)
        with pytest.raises(exc):
            eng.lt_matmul_bsgs_batch(iter(iter(row) for row in W), iter([iter(good), good, iter(cts)]), ks, n1=n1)
    # the error is the one the loop would have raised first: token 0's operands, then the keys, then the other tokens' operands
    with pytest.raises(ValueError):
        eng.lt_matmul_bsgs_batch([[d0]], [[c0], [c0, c0], [ntt]], keys)
    with pytest.raises(NotImplementedError):
        eng.lt_matmul_bsgs_batch([[d0]], [[c0], [ntt], [c0, c0]], keys)
    with pytest.raises(errors.NotMatchType, match="step 4"):
        eng.lt_matmul_bsgs_batch([[d0]], [[c0], [ntt], [c0]], [keys[1]])
    with pytest.raises(NotImplementedError):
        eng.lt_matmul_bsgs_batch([[d0]], [[ntt], [c0], [c0]], [keys[1]])
    with pytest.raises(errors.NotMatchDataStructState):                           # a token beside the level of an encoded block
        eng.lt_matmul_bsgs_batch([[d0]], [[c0], [c1], [c0]], keys)
    with pytest.raises(ValueError):                                                # the matrix before any token
        eng.lt_matmul_bsgs_batch([[d0], [d0, d0]], [[ntt]], keys)
    assert calls == []
    monkeypatch.undo()
    out = eng.lt_matmul_bsgs_batch([[d0, None], [None, {0: [1.0, 0.5]}]], [[c0, c0], [c0, c0]], keys)   # and the engine still works
    assert [[o.level for o in tok] for tok in out] == [[1, 1], [1, 1]]
    assert same(out[1][0], eng.linear_transform(c0, d0, keys)) and same(out[0][0], out[1][0])


def test_two_logical_devices_take_the_loop_and_give_the_single_device_words():
    from liberate_fhe_amd.fhe import ckks_engine
    from tests.oracle_backend import OracleBackend
    from tests.test_pc_dot_gpu import natural_rows
    res = []
    layout = [LAYOUT[1], LAYOUT[5]]
    for ndev in (1, 2):
        eng = ckks_engine(devices=["cpu"] * ndev, backend=OracleBackend(), **LT)
        assert ndev == 1 or eng._native_level(0) is None
        W, _ = layer(eng, 0, layout=layout)
        X = tokens(eng, 0, 2)
        seen, real = [], eng.lt_matmul_bsgs
        eng.lt_matmul_bsgs = lambda *a, **k: (seen.append(a[1]), real(*a, **k))[1]
        try:
            out = eng.lt_matmul_bsgs_batch(W, X, keys_for(eng))
        finally:
            del eng.lt_matmul_bsgs
        assert len(seen) == 2 and seen[0] is not seen[1]                           # the loop, token by token
        assert len(out) == 2 and all(len(tok) == 2 and all(o.level == 1 for o in tok) for tok in out)
        res.append([natural_rows(eng, o) for tok in out for o in tok])
    for a, b in zip(*res):
        for x, y in zip(a, b):
            assert x.shape == y.shape and (x == y).all()


def plan_of(logN, max_nct=4):
    plan = _fake_plan(logN)
    plan.max_nct = max_nct
    return plan


def test_workspace_query():
    """lf_lt_matmul_bsgs_batch_ws_words gives the header's formula, equals lf_lt_matmul_bsgs_ws_words at nt = 1 and is 0 for what
    the entry refuses; the names are exported, the ABI version stays 15, the Python copies of the cap are the header's."""
    from liberate_fhe_amd import _native
    from liberate_fhe_amd._native import lib, EXPORTED, _SIGNATURES
    from liberate_fhe_amd.fhe.backend import HipBackend
    assert "lf_lt_matmul_bsgs_batch" in EXPORTED and "lf_lt_matmul_bsgs_batch_ws_words" in EXPORTED and lib.lf_abi_version() == 15
    assert len(_SIGNATURES["lf_lt_matmul_bsgs_batch"]) == len(_SIGNATURES["lf_lt_matmul_bsgs"]) + 1
    assert len(_SIGNATURES["lf_lt_matmul_bsgs_batch_ws_words"]) == 5
    header = open(os.path.join(ROOT, "include", "ckks_hip.h")).read()
    TMAX = int(re.search(r"#define LF_LT_MATMUL_BSGS_BATCH_MAX_TOKENS (\d+)", header).group(1))
    OMAX = int(re.search(r"#define LF_LT_MATMUL_MAX_OUTPUTS (\d+)", header).group(1))
    KMAX = int(re.search(r"#define LF_BSGS_MAX_BABY_KEYS (\d+)", header).group(1))
    SMAX = int(re.search(r"#define LF_LT_MATMUL_BSGS_MAX_SUMS (\d+)", header).group(1))
    assert TMAX == _native.LF_LT_MATMUL_BSGS_BATCH_MAX_TOKENS == HipBackend.lt_matmul_bsgs_batch_max_tokens == 4
    for logN in (13, 17):
        for max_nct in (1, 2, 4):
            plan = plan_of(logN, max_nct)
            N, rows, ell, K = 1 << logN, 3, 2, 1
            for nt in (1, 2, 4):
                for nb in (0, 7, KMAX):
                    for k_out in (1, 2, 3, 5, OMAX):
                        for sums in (0, 1, 9, SMAX):
                            g4, gw = min(nt * k_out, 4), min(4, max_nct)
                            want = 2 * rows * N * nt * (nb + 1 + k_out + sums) + gw * ell * N + 2 * g4 * ell * N + \
                                max(lib.lf_ks_moddown_ws_words(gw, ell, K, N), lib.lf_ks_moddown_ws_words(2 * g4, ell, K, N))
                            got = lib.lf_lt_matmul_bsgs_batch_ws_words(ctypes.byref(plan), nb, k_out, sums, nt)
                            assert got == (want if nt <= max_nct else 0), (logN, max_nct, nt, nb, k_out, sums)
                            if nt == 1:
                                assert got == lib.lf_lt_matmul_bsgs_ws_words(ctypes.byref(plan), nb, k_out, sums)
    plan = plan_of(13)
    for nb, k_out, sums, nt in ((-1, 1, 0, 2), (KMAX + 1, 1, 0, 2), (0, 0, 0, 2), (0, OMAX + 1, 0, 2), (0, OMAX + 1, 0, 1), (0, 1, -1, 2),
                                (0, 1, SMAX + 1, 2), (0, 1, SMAX + 1, 1), (1, 1, 1, 0), (1, 1, 1, -1), (1, 1, 1, 3), (1, 1, 1, 5), (1, 1, 1, 8)):
        assert lib.lf_lt_matmul_bsgs_batch_ws_words(ctypes.byref(plan), nb, k_out, sums, nt) == 0, (nb, k_out, sums, nt)
    assert lib.lf_lt_matmul_bsgs_batch_ws_words(ctypes.byref(plan_of(13, 2)), 1, 1, 1, 4) == 0          # nt above max_nct
    assert lib.lf_lt_matmul_bsgs_batch_ws_words(ctypes.byref(plan_of(13, 2)), 1, 1, 1, 2) > 0
    for logN in (12, 18):                                                                                # a refused plan
        assert lib.lf_lt_matmul_bsgs_batch_ws_words(ctypes.byref(plan_of(logN)), 1, 1, 1, 2) == 0
    assert lib.lf_lt_matmul_bsgs_batch_ws_words(None, 1, 1, 1, 2) == 0


def test_c_entry_refuses_bad_arguments_before_any_launch():
    """lf_lt_matmul_bsgs_batch returns LF_ERR_ARG from its arguments alone (a plan of dummy pointers that are never dereferenced;
    no call here would pass the checks): nt outside {1, 2, 4} or above max_nct, a NULL among the pointers of any token, what
    lf_lt_matmul_bsgs refuses for every nt, a workspace NULL, misaligned by 8 bytes or one word short."""
    from liberate_fhe_amd._native import lib
    LF_ERR_ARG = 10001
    plan = plan_of(13)
    dummy = ctypes.c_void_p(64)
    stride = 3 << 13

    def i64(values):
        return (ctypes.c_int64 * max(1, len(values)))(*values)

    def ptrs(count, null_at=()):
        arr = (ctypes.c_void_p * max(count, 1))(*([64] * max(count, 1)))
        for at in null_at:
            arr[at] = None
        return arr

    # per token 2 inputs x 2 outputs x 2 giant steps (0 and exponent 5): column 0 has two baby keys (exponents 3, 7), column 1 none.
    # [o][i][j]: (0,0,0) slots 0,1,2; (0,0,1) slot 1; (1,0,1) slot 2; (1,1,0) slot 0; the rest NULL.  Two keyed sums per token.
    NUL = [2, 3, 4, 7]

    def call(plan=plan, nt=2, k_in=2, k_out=2, ng=2, scales=dummy, ws=dummy, ws_words=1 << 40, fmt=0, **over):
        a = {"ins": ptrs(16), "bkeys": ptrs(4), "gkeys": ptrs(4), "pts": ptrs(8, NUL), "out0": ptrs(8), "out1": ptrs(8),
             "ncol": i64((2, 0)), "bexps": i64((3, 7)), "gexps": i64((0, 5)), "strides": i64((stride, stride, 0, 0, 0, stride, stride, 0)),
             "counts": i64((3, 1, 0, 0, 0, 1, 1, 0)), "bidx": i64((0, 1, 2, 1, 2, 0))}
        for name, value in over.items():
            assert name in a
            a[name] = value if value is None or isinstance(value, ctypes.Array) else i64(value)
        return lib.lf_lt_matmul_bsgs_batch(ctypes.byref(plan) if plan is not None else None, nt, k_in, k_out, a["ins"], a["ncol"],
                                           a["bexps"], a["bkeys"], ng, a["gexps"], a["gkeys"], 0, 0, 0, fmt, a["pts"], a["strides"],
                                           a["counts"], a["bidx"], scales, 0, ws, ws_words, a["out0"], a["out1"], None)

    need = {nt: lib.lf_lt_matmul_bsgs_batch_ws_words(ctypes.byref(plan), 2, 2, 2, nt) for nt in (1, 2, 4)}
    assert 0 < need[1] < need[2] < need[4]
    assert call(plan=None) == LF_ERR_ARG
    for nt in (0, -1, 3, 5, 8):
        assert call(nt=nt) == LF_ERR_ARG, nt
    assert call(plan=plan_of(13, 2), nt=4) == LF_ERR_ARG and call(plan=plan_of(13, 1)) == LF_ERR_ARG       # nt above max_nct
    for logN in (12, 18):
        assert call(plan=plan_of(logN)) == LF_ERR_ARG
    nopr = plan_of(13)
    nopr.PR = None
    assert call(plan=nopr) == LF_ERR_ARG
    for nt in (1, 2, 4):                                                           # what lf_lt_matmul_bsgs refuses, for every nt
        assert call(nt=nt, k_in=0) == LF_ERR_ARG and call(nt=nt, k_out=0) == LF_ERR_ARG and call(nt=nt, ng=0) == LF_ERR_ARG
        for name in ("ins", "ncol", "bexps", "bkeys", "gexps", "gkeys", "pts", "strides", "counts", "bidx", "out0", "out1"):
            assert call(nt=nt, **{name: None}) == LF_ERR_ARG, (nt, name)
        assert call(nt=nt, scales=None) == LF_ERR_ARG and call(nt=nt, fmt=2) == LF_ERR_ARG
        assert call(nt=nt, bexps=(4, 7)) == LF_ERR_ARG and call(nt=nt, gexps=(5, 0)) == LF_ERR_ARG
        assert call(nt=nt, gkeys=ptrs(4, [1])) == LF_ERR_ARG                       # a keyed giant step without a key
        assert call(nt=nt, bidx=(1, 0, 2, 1, 2, 0)) == LF_ERR_ARG                  # slots not ascending
        assert call(nt=nt, pts=ptrs(8, NUL + [0, 1])) == LF_ERR_ARG                # an output with no diagonal at all
        assert call(nt=nt, ws=None) == LF_ERR_ARG
        assert call(nt=nt, ws=ctypes.c_void_p(72)) == LF_ERR_ARG                   # misaligned by 8 bytes
        assert call(nt=nt, ws_words=need[nt] - 1) == LF_ERR_ARG                    # one word short (every other argument good)
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
    unused = dict(pts=ptrs(8, NUL + [6]), counts=(3, 1, 0, 0, 0, 1, 0, 0), bidx=(0, 1, 2, 1, 2), ins=ptrs(16, [2, 3, 6, 7]))
    assert call(ws_words=need[2] - 1, **unused) == LF_ERR_ARG


def test_backend_naming():
    """The backend's entry exists under a name that does not end in _native (the *_native methods are a closed list that the fenced
    and the stream-contract suites go through one by one), with the group sizes (4, 2); the checker backend has neither; the op
    adds no kernel, so the tracked resource table is the one of the kernels it launches."""
    from liberate_fhe_amd.fhe.backend import HipBackend
    from tests.helpers import NATIVE_ENTRIES
    from tests.oracle_backend import OracleBackend
    assert callable(HipBackend.lt_matmul_bsgs_batch_call) and callable(HipBackend.lt_matmul_bsgs_batch_ws_words)
    assert HipBackend.lt_matmul_bsgs_batch_sizes == (4, 2)
    mine = [name for name in dir(HipBackend) if name.startswith("lt_matmul_bsgs_batch")]
    assert mine and not any(name.endswith("_native") for name in mine)
    assert {name for name in dir(HipBackend) if name.endswith("_native") and not name.startswith("_")} <= set(NATIVE_ENTRIES)
    assert not hasattr(OracleBackend, "lt_matmul_bsgs_batch_call") and not hasattr(OracleBackend, "lt_matmul_bsgs_batch_sizes")
    import __graft_entry__ as g
    res = {r["kernel"]: r for r in g.kernel_resources()}
    for k in [f"lt_block_productsb_kernel<{no}, 2>" for no in (1, 2, 4)] + \
            [f"{name}<{nct}, {pl}, {dpl}>" for name in ("ks_inner_babyb_kernel", "ks_inner_giantb_kernel") for nct in (2, 4)
             for pl in ("true", "false") for dpl in ("true", "false")]:
        assert res[k]["scratch"] == 0 and res[k]["vgpr_spill"] == 0 and res[k]["sgpr_spill"] == 0, res[k]
