"""pc_matmul_batch (a plaintext matrix times B token vectors of ciphertexts; lf_pc_matmul_batch) without a GPU: the engine's host
logic on the checker backend against the loop of pc_matmul that defines its words, the refusals (before anything runs), the
grouping of the tokens through a marker backend, the C entry's argument checks and the new kernels' resources."""
import ctypes
import os
import re

import pytest
import torch

from liberate_fhe_amd.utils import synth
from tests.test_cc_dot_cpu import same
from tests.test_pc_dot_cpu import message
from tests.test_pc_matmul_cpu import checker, layer_of  # noqa: F401  (checker: the module-scoped engine fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def chunk():
    from liberate_fhe_amd.fhe.backend import HipBackend
    return HipBackend.pc_matmul_chunk


def tokens_of(eng, cts, B, level, seed=70):
    """B token vectors over the layer's ciphertexts and two more: token 0 is the layer's own vector, token t > 0 a rotation of it
    with one fresh ciphertext, the last token (B >= 3) token 0 once more: objects repeat inside a token and across tokens."""
    extra = [synth.ciphertext(eng, seed + i, level) for i in range(2)]
    X = []
    for t in range(B):
        tok = [cts[(i + t) % len(cts)] for i in range(len(cts))]
        if t:
            tok[(t - 1) % len(tok)] = extra[t % 2]
        X.append(tok)
    if B >= 3:
        X[-1] = list(X[0])
    return X


@pytest.mark.parametrize("B", [1, 2, 5])
@pytest.mark.parametrize("shape", ["1x1", "3x2", "CI+1x3"])
def test_batch_equals_the_loop_on_the_checker_engine(checker, shape, B):
    """Holes, an all-None column, repeated objects in and across tokens, with and without a (partly-None) bias; level 0 and, for
    the small shapes, the last legal one.  Lists and iterators."""
    eng = checker
    k_in, k_out = {"1x1": (1, 1), "3x2": (3, 2), "CI+1x3": (chunk() + 1, 3)}[shape]
    for level in ((0,) if k_in > 3 else (0, eng.num_levels - 2)):
        W, cts, bias = layer_of(eng, k_in, k_out, level)
        X = tokens_of(eng, cts, B, level)
        assert k_in < 3 or (bias[0] is None and any(b is not None for b in bias) and all(row[1] is None for row in W) and W[1][0] is None)
        assert B < 3 or (X[-1][0] is X[0][0] and X[1][0] is not X[0][0])
        for b in (None, bias):
            want = [eng.pc_matmul(W, tok, b) for tok in X]
            got = eng.pc_matmul_batch(W, X, b)
            assert isinstance(got, list) and len(got) == B and all(isinstance(g, list) and len(g) == k_out for g in got)
            assert all(o.level == level + 1 for g in got for o in g)
            assert all(same(a, w) for g, ws in zip(got, want) for a, w in zip(g, ws)), (shape, B, level, b is not None)
        got = eng.pc_matmul_batch(iter([iter(row) for row in W]), (iter(tok) for tok in X), iter(bias))
        assert all(same(a, w) for g, ws in zip(got, want) for a, w in zip(g, ws))


def test_an_empty_batch_is_an_empty_list(checker):
    eng = checker
    p0 = eng.encode_plain(message(eng, 1), 0)
    assert eng.pc_matmul_batch([[p0]], []) == [] and eng.pc_matmul_batch([[p0]], iter(())) == []
    assert eng.pc_matmul_batch([], []) == []                   # (the loop checks nothing either)


def test_refusals_come_before_anything_runs(checker, monkeypatch):
    """Every refusal of pc_matmul, in the LAST of three tokens where the tokens can differ (a refusal that lies in W or the bias
    holds for every token): the same exception type as pc_matmul, with pc_matmul, pc_dot, the native hooks, the ntt ops and
    every allocation patched to record — none is reached."""
    from liberate_fhe_amd.fhe.presets import errors
    eng = checker
    top = eng.num_levels - 1
    c0, c1, ctop = (synth.ciphertext(eng, 60 + i, lvl) for i, lvl in enumerate((0, 1, top)))
    m = message(eng, 1)
    p0, p1 = eng.encode_plain(m, 0), eng.encode_plain(m, 1)
    a0, a1, a2 = (eng.encode_plain(m, lvl, "add") for lvl in (0, 1, 2))
    ptop = eng._new(eng.encode_plain(m, top, "add").data, p0.origin, level=top, ntt_state=True, montgomery_state=True)
    ntt = eng._new(c0.data, c0.origin, level=0, ntt_state=True)
    special = eng._new(c0.data, c0.origin, level=0, include_special=True)
    coeff_pt = eng._new(p0.data, p0.origin, level=0, ntt_state=False, montgomery_state=True)
    cases = [
        (ValueError, [], [c0], None),                                             # W empty
        (ValueError, [[p0]], [], None),
        (ValueError, [[p0, p0], [p0]], [c0, c0], None),                           # ragged W
        (ValueError, [[p0], [p0]], [c0, c0], None),                               # a ragged token: len(W[o]) != len(cts)
        (ValueError, [[p0, p0, p0]], [c0, c0], None),
        (ValueError, [[p0, None], [None, None]], [c0, c0], None),                 # a row with no entry
        (errors.NotMatchType, [[a0]], [c0], None),                                # an "add" plaintext in the matrix
        (errors.NotMatchType, [[p0, c0]], [c0, c0], None),                        # a ciphertext where a plaintext belongs
        (errors.NotMatchType, [[p0]], [p0], None),                                # .. and the other way round: a wrong origin
        (errors.NotMatchType, [[p0, None]], [c0, None], None),                    # (a None ciphertext, even in an unused column)
        (errors.NotMatchType, [[p0]], [c0], [p1]),                                # a "mult" plaintext as bias
        (errors.NotMatchType, [[p0]], [c0], [c1]),
        (errors.NotMatchDataStructState, [[coeff_pt]], [c0], None),               # a wrong state of the plaintext
        (errors.NotMatchDataStructState, [[p0]], [ntt], None),                    # an NTT-domain ciphertext
        (errors.NotMatchDataStructState, [[p0]], [special], [a1]),                # special limbs
        (errors.NotMatchDataStructState, [[p0, p0]], [c0, c1], None),             # levels that differ
        (errors.NotMatchDataStructState, [[p0, p1]], [c0, c0], None),
        (errors.NotMatchDataStructState, [[p0], [p1]], [c0], None),
        (errors.NotMatchDataStructState, [[p1]], [c0], None),                     # a level beside W's
        (errors.NotMatchDataStructState, [[p0, None]], [c0, c1], None),           # (an unused column is still of the level)
        (ValueError, [[p0], [p0]], [c0], [a1]),                                   # len(bias) != k_out
        (ValueError, [[p0]], [c0], []),
        (errors.NotMatchDataStructState, [[p0], [p0]], [c0], [None, a0]),         # a bias not at l + 1
        (errors.NotMatchDataStructState, [[p0]], [c0], [a2]),
        (errors.MaximumLevelError, [[ptop]], [ctop], None),
        (errors.MaximumLevelError, [[ptop, None], [ptop, ptop]], [ctop, ctop], None),
    ]
    # what pc_matmul itself says to each case, before anything is patched
    for exc, W, cts, bias in cases:
        with pytest.raises(exc):
            eng.pc_matmul(W, cts, bias)
    calls = []

    def boom(name):
        def f(*a, **k):
            calls.append(name)
            raise AssertionError(name + " reached")
        return f

    for name in ("pc_matmul", "pc_dot", "_pc_matmul_native", "_pc_matmul_batch_native", "rescale", "clone", "_ws"):
        monkeypatch.setattr(eng, name, boom(name))
    for name in ("pc_matmul_native", "pc_matmul_batch_native", "pc_dot_native"):
        monkeypatch.setattr(eng.backend, name, boom(name), raising=False)
    monkeypatch.setattr(eng.backend, "pc_matmul_batch_sizes", (4, 2), raising=False)
    real_empty = torch.empty
    monkeypatch.setattr(torch, "empty", lambda *a, **k: (calls.append("empty"), real_empty(*a, **k))[1])
    for name in ("enter_ntt", "mont_mult", "mont_add", "mont_enter", "intt_exit_reduce", "mont_redc", "reduce_2q"):
        monkeypatch.setattr(eng.ntt, name, boom(name))
    for exc, W, cts, bias in cases:
        good = [ctop if exc is errors.MaximumLevelError else c0] * (len(W[0]) if W else 1)
        with pytest.raises(exc):
            eng.pc_matmul_batch(W, [good, good, cts], bias)
        with pytest.raises(exc):
            eng.pc_matmul_batch(iter(W), iter([good, iter(cts)]), None if bias is None else iter(bias))
    # the error is the one the loop would have raised first
    with pytest.raises(errors.NotMatchType):
        eng.pc_matmul_batch([[p0]], [[c0], [p0], [c0, c0]])
    with pytest.raises(ValueError):
        eng.pc_matmul_batch([[p0]], [[c0], [c0, c0], [p0]])
    assert calls == []
    monkeypatch.undo()
    out = eng.pc_matmul_batch([[p0, None], [p0, p0]], [[c0, c0], [c0, c0]], [None, a1])     # and the engine still works
    assert [[o.level for o in tok] for tok in out] == [[1, 1], [1, 1]]


class FakeNative:
    """Marks what the engine sends through the batched entry; everything else is the checker backend's (which has no native
    pc_matmul or pc_dot: a token that takes pc_matmul runs the composition)."""
    native_ops = True
    pc_matmul_chunk = 16
    pc_matmul_max_outputs = 64
    pc_matmul_batch_sizes = (4, 2)

    def __init__(self, inner):
        self._inner, self.batches = inner, []

    def __getattr__(self, name):
        return getattr(self._inner, name)

    def pc_matmul_batch_ws_words(self, nt, k_in, k_out, rows, logN):
        return 2

    def pc_matmul_batch_native(self, ins, pts, biases, outs, nt, k_in, k_out, rows, logN, *rest):
        assert len(ins) == nt * 2 * k_in and len(pts) == k_out * k_in and len(outs) == nt and all(len(tok) == k_out for tok in outs)
        self.batches.append(dict(nt=nt, k_in=k_in, k_out=k_out, ins=list(ins), pts=list(pts), biases=None if biases is None else list(biases)))
        for t, tok in enumerate(outs):
            for o, pair in enumerate(tok):
                for c in pair:
                    assert tuple(c.shape) == (rows - 1, 1 << logN)
                    c.fill_(10000 * len(self.batches) + 100 * t + o)


def marked(eng, monkeypatch, sizes=(4, 2)):
    """The marker backend under the engine, with the group sizes the backend offers (the engine's own default leaves 4 out)."""
    monkeypatch.setattr(eng, "pc_matmul_batch_sizes", sizes)
    assert not hasattr(eng.backend, "pc_matmul_native") and not hasattr(eng.backend, "pc_dot_native")
    fake = FakeNative(eng.backend)
    monkeypatch.setattr(eng, "backend", fake)
    # the tokens of the checker are host tensors; everything else pc_matmul asks of an operand stays
    monkeypatch.setattr(eng, "_pc_operand_ok", lambda t: t.is_contiguous() and t.dtype == torch.int64 and t.data_ptr() % 16 == 0)
    real = eng._native_level
    # (the native level only where pc_matmul_batch asks: the compositions of the tokens that take pc_matmul are the checker's)
    monkeypatch.setattr(eng, "_native_level", lambda lvl: 0 if fake.asking else real(lvl))
    fake.asking = False
    batch = eng.pc_matmul_batch

    def asking(*a, **k):
        fake.asking = True
        try:
            return batch(*a, **k)
        finally:
            fake.asking = False

    real_mm = eng.pc_matmul

    def loop_call(*a, **k):
        was, fake.asking = fake.asking, False
        fake.loops.append(tuple(id(c) for c in a[1]))
        try:
            return real_mm(*a, **k)
        finally:
            fake.asking = was

    fake.loops = []
    monkeypatch.setattr(eng, "pc_matmul", loop_call)
    return fake, asking


def mark_of(ct):
    return int(ct.data[0][0][0, 0])


def test_groupings_through_the_marker_backend(checker, monkeypatch):
    """7 ready tokens: groups of 4 and 2 and a pc_matmul call for the last; fewer tokens accordingly; every output at its token's
    place; the pointers of a group in [token][input][component] order."""
    eng = checker
    W, cts, bias = layer_of(eng, 3, 2, 0)
    X = [[synth.ciphertext(eng, 100 + 3 * t + i, 0) for i in range(3)] for t in range(7)]
    want = [eng.pc_matmul(W, tok, bias) for tok in X]
    for B, groups, loops in ((1, [], [0]), (2, [2], []), (3, [2], [2]), (4, [4], []), (5, [4], [4]), (6, [4, 2], []), (7, [4, 2], [6])):
        fake, batch = marked(eng, monkeypatch)
        got = batch(W, X[:B], bias)
        monkeypatch.undo()
        assert [b["nt"] for b in fake.batches] == groups and all((b["k_in"], b["k_out"]) == (3, 2) for b in fake.batches), B
        assert fake.loops == [tuple(id(c) for c in X[t]) for t in loops], B
        t0 = 0
        for n, b in enumerate(fake.batches):
            assert b["ins"] == [ct.data[c][0].data_ptr() for tok in X[t0:t0 + b["nt"]] for ct in tok for c in range(2)]
            assert b["pts"] == [None if pt is None else pt.data[0].data_ptr() for row in W for pt in row]
            assert b["biases"] == [None if x is None else x.data[0].data_ptr() for x in bias]
            for t in range(b["nt"]):
                assert [mark_of(o) for o in got[t0 + t]] == [10000 * (n + 1) + 100 * t + o for o in range(2)]
                assert all(o.level == 1 for o in got[t0 + t])
            t0 += b["nt"]
        for t in loops:
            assert all(same(a, w) for a, w in zip(got[t], want[t]))
    # a group size left out of pc_matmul_batch_sizes goes to the loop: with (4,) alone three tokens are three pc_matmul calls
    fake, batch = marked(eng, monkeypatch, (4,))
    got = batch(W, X[:3], bias)
    monkeypatch.undo()
    assert fake.batches == [] and len(fake.loops) == 3 and all(same(a, w) for g, ws in zip(got, want) for a, w in zip(g, ws))
    # the engine's own sizes: pairs only (groups of 4 measured slower) — 7 tokens are 2 + 2 + 2 and a pc_matmul call
    assert type(eng).pc_matmul_batch_sizes == (2,)
    fake, batch = marked(eng, monkeypatch, type(eng).pc_matmul_batch_sizes)
    got = batch(W, X, bias)
    monkeypatch.undo()
    assert [b["nt"] for b in fake.batches] == [2, 2, 2] and fake.loops == [tuple(id(c) for c in X[6])]
    assert [mark_of(got[t][1]) for t in range(6)] == [10000 * (t // 2 + 1) + 100 * (t % 2) + 1 for t in range(6)]
    # .. and a size the backend does not offer is not used
    fake, batch = marked(eng, monkeypatch, (3, 2))
    got = batch(W, X[:3], bias)
    monkeypatch.undo()
    assert [b["nt"] for b in fake.batches] == [2] and len(fake.loops) == 1


def test_a_token_that_is_not_ready_keeps_its_place(checker, monkeypatch):
    """Token 2 of 6 has a non-contiguous component, token 4 one at an odd word offset: the other four are ONE group of 4; the two
    take pc_matmul and sit at their places with pc_matmul's words."""
    eng = checker
    W, cts, bias = layer_of(eng, 3, 2, 0)
    X = [[synth.ciphertext(eng, 100 + 3 * t + i, 0) for i in range(3)] for t in range(6)]
    t = X[2][1].data[0][0]
    wide = torch.zeros((t.shape[0], 2 * t.shape[1]), dtype=t.dtype)
    wide[:, ::2] = t
    X[2][1].data[0][0] = wide[:, ::2]
    t = X[4][2].data[1][0]
    flat = torch.zeros(t.numel() + 2, dtype=t.dtype)
    flat = flat[1:] if flat.data_ptr() % 16 == 0 else flat[2:]
    flat[:t.numel()] = t.reshape(-1)
    X[4][2].data[1][0] = flat[:t.numel()].view(t.shape)
    assert not X[2][1].data[0][0].is_contiguous() and X[4][2].data[1][0].is_contiguous() and X[4][2].data[1][0].data_ptr() % 16 == 8
    want = [eng.pc_matmul(W, tok, bias) for tok in X]
    fake, batch = marked(eng, monkeypatch)
    got = batch(W, X, bias)
    monkeypatch.undo()
    assert [b["nt"] for b in fake.batches] == [4] and fake.loops == [tuple(id(c) for c in X[i]) for i in (2, 4)]
    assert fake.batches[0]["ins"] == [ct.data[c][0].data_ptr() for i in (0, 1, 3, 5) for ct in X[i] for c in range(2)]
    for j, i in enumerate((0, 1, 3, 5)):
        assert [mark_of(o) for o in got[i]] == [10000 + 100 * j, 10000 + 100 * j + 1]
    for i in (2, 4):
        assert all(same(a, w) for a, w in zip(got[i], want[i]))


def test_65_outputs_split_64_and_1_per_group(checker, monkeypatch):
    eng = checker
    pts = [eng.encode_plain(message(eng, 3 + i), 0) for i in range(2)]
    X = [[synth.ciphertext(eng, 130 + t, 0)] for t in range(6)]
    W = [[pts[0]]] * 64 + [[pts[1]]]
    fake, batch = marked(eng, monkeypatch)
    got = batch(W, X)
    monkeypatch.undo()
    assert [(b["nt"], b["k_in"], b["k_out"]) for b in fake.batches] == [(4, 1, 64), (4, 1, 1), (2, 1, 64), (2, 1, 1)] and fake.loops == []
    assert all(b["biases"] is None for b in fake.batches)
    assert fake.batches[1]["pts"] == [pts[1].data[0].data_ptr()] and fake.batches[0]["ins"] == fake.batches[1]["ins"]
    for t0, n in ((0, 1), (4, 3)):
        for t in range(t0, 6 if t0 else 4):
            assert len(got[t]) == 65
            assert [mark_of(o) for o in got[t]] == [10000 * n + 100 * (t - t0) + o for o in range(64)] + [10000 * (n + 1) + 100 * (t - t0)]


def test_c_entry_refuses_bad_arguments_before_any_device_call():
    """lf_pc_matmul_batch returns LF_ERR_ARG from its arguments alone (dummy pointers that are never dereferenced; no call here
    would pass the checks), and lf_pc_matmul_batch_ws_words gives (2 min(k_in, CI) + 2 k_out) nt rows N, 0 for refused shapes."""
    from liberate_fhe_amd import _native
    from liberate_fhe_amd._native import lib, EXPORTED, _SIGNATURES
    from liberate_fhe_amd.fhe.backend import HipBackend
    LF_ERR_ARG = 10001
    assert "lf_pc_matmul_batch" in EXPORTED and "lf_pc_matmul_batch_ws_words" in EXPORTED and lib.lf_abi_version() == 15
    assert len(_SIGNATURES["lf_pc_matmul_batch"]) == len(_SIGNATURES["lf_pc_matmul"]) + 1
    assert _SIGNATURES["lf_pc_matmul_batch"][0] is ctypes.c_int and len(_SIGNATURES["lf_pc_matmul_batch_ws_words"]) == 5
    header = open(os.path.join(ROOT, "include", "ckks_hip.h")).read()
    CI = int(re.search(r"#define LF_PC_MATMUL_CI (\d+)", header).group(1))
    GMAX = int(re.search(r"#define LF_PC_MATMUL_MAX_OUTPUTS (\d+)", header).group(1))
    TMAX = int(re.search(r"#define LF_PC_MATMUL_BATCH_MAX_TOKENS (\d+)", header).group(1))
    assert TMAX == _native.LF_PC_MATMUL_BATCH_MAX_TOKENS == HipBackend.pc_matmul_batch_max_tokens == 4
    assert max(HipBackend.pc_matmul_batch_sizes) <= TMAX and min(HipBackend.pc_matmul_batch_sizes) >= 2
    max_rows = lib.lf_limits(2)
    for nt in range(1, TMAX + 1):
        for logN in (13, 17):
            for rows in (2, 5, max_rows):
                for k_in in (1, 5, CI, CI + 1, 3 * CI):
                    for k_out in (1, 3, 4, 9, GMAX):
                        assert lib.lf_pc_matmul_batch_ws_words(nt, k_in, k_out, rows, logN) == \
                            (2 * min(k_in, CI) + 2 * k_out) * nt * rows * (1 << logN)
    for nt, k_in, k_out, rows, logN in ((0, 1, 1, 3, 13), (-1, 1, 1, 3, 13), (TMAX + 1, 1, 1, 3, 13), (2, 0, 1, 3, 13), (2, -1, 1, 3, 13),
                                        (2, 1, 0, 3, 13), (2, 1, GMAX + 1, 3, 13), (2, 1, 1, 1, 13), (2, 1, 1, 0, 13),
                                        (2, 1, 1, max_rows + 1, 13), (2, 1, 1, 3, 12), (2, 1, 1, 3, 18), (2, 1, 1, 3, 0)):
        assert lib.lf_pc_matmul_batch_ws_words(nt, k_in, k_out, rows, logN) == 0, (nt, k_in, k_out, rows, logN)

    def ptrs(n, null_at=()):
        arr = (ctypes.c_void_p * max(n, 1))(*([64] * max(n, 1)))
        for at in null_at:
            arr[at] = None
        return arr

    names = ("ins", "pts", "bias", "out0", "out1", "psi", "psi_dp", "ipsi", "ipsi_dp", "q_host", "Rs", "Ninv", "one", "zero", "scales",
             "ws", "ql", "qh", "kl", "kh")

    def call(nt=3, k_in=2, k_out=3, rows=3, logN=13, ws_words=1 << 40, **over):
        a = {n: ctypes.c_void_p(64) for n in names}
        tn, ki, ko = max(nt, 1), max(k_in, 1), max(k_out, 1)
        a["ins"], a["pts"], a["bias"], a["out0"], a["out1"] = ptrs(tn * 2 * ki), ptrs(ki * ko), ptrs(ko), ptrs(tn * ko), ptrs(tn * ko)
        a.update(over)
        return lib.lf_pc_matmul_batch(nt, k_in, k_out, a["ins"], a["pts"], a["bias"], a["out0"], a["out1"], rows, logN, a["psi"],
                                      a["psi_dp"], a["ipsi"], a["ipsi_dp"], a["q_host"], a["Rs"], a["Ninv"], a["one"], a["zero"],
                                      a["scales"], 0, a["ws"], ws_words, a["ql"], a["qh"], a["kl"], a["kh"], 0, None)

    for nt in (0, -1, TMAX + 1, 1 << 20):
        assert call(nt=nt) == LF_ERR_ARG, nt
    for k_in in (0, -1):
        assert call(k_in=k_in) == LF_ERR_ARG
    for k_out in (0, -1, GMAX + 1):
        assert call(k_out=k_out) == LF_ERR_ARG
    for rows in (1, 0, -1, max_rows + 1):
        assert call(rows=rows) == LF_ERR_ARG, rows
    for logN in (12, 18, 0):
        assert call(logN=logN) == LF_ERR_ARG, logN
    for n in names:
        if n != "bias":                                                  # (the biases are optional)
            assert call(**{n: None}) == LF_ERR_ARG, n
    for nt in range(1, TMAX + 1):
        for k_in, k_out in ((1, 1), (3, 2), (CI + 1, 5)):
            need = lib.lf_pc_matmul_batch_ws_words(nt, k_in, k_out, 3, 13)
            assert call(nt=nt, k_in=k_in, k_out=k_out, ws_words=need - 1) == LF_ERR_ARG
            for at in (0, nt * 2 * k_in - 1, (nt - 1) * 2 * k_in):           # the first pointer, the last, the last token's first
                assert call(nt=nt, k_in=k_in, k_out=k_out, ins=ptrs(nt * 2 * k_in, [at])) == LF_ERR_ARG
            for at in (0, nt * k_out - 1, (nt - 1) * k_out):
                assert call(nt=nt, k_in=k_in, k_out=k_out, out0=ptrs(nt * k_out, [at])) == LF_ERR_ARG
                assert call(nt=nt, k_in=k_in, k_out=k_out, out1=ptrs(nt * k_out, [at])) == LF_ERR_ARG
            for o in (0, k_out - 1):                                         # an output row whose entries are all NULL
                assert call(nt=nt, k_in=k_in, k_out=k_out, pts=ptrs(k_in * k_out, range(o * k_in, (o + 1) * k_in))) == LF_ERR_ARG
    assert call(ws=ctypes.c_void_p(72)) == LF_ERR_ARG                    # 16-byte aligned
    assert call(ws_words=0) == LF_ERR_ARG
    assert call(ws_words=lib.lf_pc_matmul_ws_words(2, 3, 3, 13)) == LF_ERR_ARG     # one token's workspace for three


def test_the_tile_knob_is_a_tuning_knob():
    """LF_TUNE_PC_MATMUL_TILE: 0 (default: tiles of 2 tokens), 1 and 2 (tiles of 4, for the A/B tool); anything else leaves it."""
    from liberate_fhe_amd._native import lib
    header = open(os.path.join(ROOT, "include", "ckks_hip.h")).read()
    knob = int(re.search(r"#define LF_TUNE_PC_MATMUL_TILE (\d+)", header).group(1))
    assert lib.lf_tune(knob, -1) == 0
    try:
        assert lib.lf_tune(knob, 2) == 0 and lib.lf_tune(knob, 3) == 2 and lib.lf_tune(knob, 1) == 2 and lib.lf_tune(knob, -1) == 1
    finally:
        lib.lf_tune(knob, 0)
    assert lib.lf_tune(knob, -1) == 0


def test_pc_matmulb_kernels_use_no_scratch():
    """Every tile the launch code can select (GO = 1 | 2 | 4 outputs x GT = 2 tokens; GT = 4 under LF_TUNE_PC_MATMUL_TILE) exists
    under its own name with scratch 0 and no spill, the default ones (GT = 2) with at least 4 waves per SIMD, and the tracked table lists it as built; pc_matmul_kernel<1 | 2 | 4> are held to
    their figures, VGPRs 53 / 69 / 85 at 8 / 7 / 5 waves per SIMD (53 / 67 / 83 at the same waves until the three product bodies became
    one: the same instructions to within two, LAB_NOTES has the timings); the launch table selects exactly the three of them."""
    import __graft_entry__ as g
    res = {r["kernel"]: r for r in g.kernel_resources()}
    want = [f"pc_matmulb_kernel<{go}, {gt}>" for go in (1, 2, 4) for gt in (2, 4)]
    assert sorted(k for k in res if k.startswith("pc_matmulb_kernel")) == sorted(want)
    src = open(os.path.join(ROOT, "liberate_fhe_amd", "csrc", "ckks_ks.hip")).read()
    table = src.split("switch ((planes ? 64 : 0) + go * 8 + gt)")[1].split("}")[0]      # (the one dispatch of lf_pc_matmul_products)
    launched = re.findall(r"LF_PCMMB_CASE\((\d), (\d)\)", table)
    assert sorted(f"pc_matmulb_kernel<{go}, {gt}>" for go, gt in launched) == sorted(want)
    one = [f"pc_matmul_kernel<{go}>" for go in re.findall(r"LF_PCMM_CASE\((\d)\)", table)]
    assert sorted(one) == sorted(k for k in res if k.startswith("pc_matmul_kernel")) == [f"pc_matmul_kernel<{go}>" for go in (1, 2, 4)]
    tracked = open(os.path.join(ROOT, "profiles", "r06_kernel_resources.txt")).read()
    for k in want:
        r = res[k]
        assert r["file"] == "ckks_ks.hip" and r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, r
        assert r["occupancy"] >= (4 if k.endswith(", 2>") else 2) and r["lds"] == 0, r
        line = next(ln for ln in tracked.splitlines() if ln[18:76].strip() == k)
        f = line.split()
        assert (int(f[-7]), int(f[-3]), int(f[-1])) == (r["vgprs"], r["scratch"], r["occupancy"]), line
    for k, vgprs, occ in (("pc_matmul_kernel<1>", 53, 8), ("pc_matmul_kernel<2>", 69, 7), ("pc_matmul_kernel<4>", 85, 5)):
        assert (res[k]["vgprs"], res[k]["occupancy"], res[k]["scratch"]) == (vgprs, occ, 0), res[k]
