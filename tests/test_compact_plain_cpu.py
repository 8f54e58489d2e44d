"""Compact plaintexts (ckks_engine.compact_plain / expand_plain; lf_plain_planes, lf_pc_matmul_batch_planes) without a GPU: the
format's sizes and offsets against the primes, the host implementation of the packer and its inverse on edge words, the refusals,
the four product ops on compact plaintexts against the raw ones on the checker backend, persistence, the C entries' argument
checks, what the engine hands the native entry (through a stub) and the new kernels' resources."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from liberate_fhe_amd.utils import synth
from tests.test_cc_dot_cpu import same
from tests.test_pc_dot_cpu import message
from tests.test_pc_matmul_batch_cpu import chunk, tokens_of
from tests.test_pc_matmul_cpu import checker, layer_of  # noqa: F401  (checker: the module-scoped engine fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LF_ERR_ARG = 10001


def primes_of(eng, level):
    return [int(eng.ctx.q[i]) for i in eng.ntt.p.destination_arrays[level][0]]


def edge_words(eng, level, seed=5):
    """A "mult" plaintext whose rows start 0, 1, q - 1, q, 2q - 1 and go on with random lazy words below 2q."""
    like = eng.encode_plain(message(eng, 1), level)
    rng = np.random.default_rng(seed)
    rows = []
    for q in primes_of(eng, level):
        w = rng.integers(0, 2 * q, size=eng.ctx.N, dtype=np.int64)
        w[:5] = [0, 1, q - 1, q, 2 * q - 1]
        rows.append(w)
    return like._replace(data=[torch.from_numpy(np.stack(rows)).to(like.data[0].device)])


def compact_layer(eng, W):
    """W with every distinct plaintext object compacted once (objects that repeat go on repeating)."""
    done = {}
    return [[None if pt is None else done.setdefault(id(pt), eng.compact_plain(pt)) for pt in row] for row in W]


def test_the_class_bound_comes_from_the_library():
    from liberate_fhe_amd import _native
    from liberate_fhe_amd.fhe import backend
    header = open(os.path.join(ROOT, "include", "ckks_hip.h")).read()
    which = int(re.search(r"#define LF_LIMIT_SMALL_PRIME_BITS (\d+)", header).group(1))
    assert which == _native.LF_LIMIT_SMALL_PRIME_BITS and _native.lib.lf_limits(which) == 41
    assert backend.SMALL_PRIME_LIMIT == 1 << 41
    rows = int(re.search(r"#define LF_PLAIN_PLANES_MAX_ROWS (\d+)", header).group(1))
    assert rows == _native.LF_PLAIN_PLANES_MAX_ROWS == backend.HipBackend.plain_planes_max_rows == 64
    src = open(os.path.join(ROOT, "liberate_fhe_amd", "fhe", "plainops.py")).read()
    assert "1 << 41" not in src and "2 ** 41" not in src


def test_size_and_row_offsets_follow_the_primes(checker):
    """(6 n_small + 8 n_int) N bytes; a row starts N / 4 words earlier per fp64-class row before it; at level 0 and at the last legal
    level, where the class mix differs; the engine's offsets, the library's size and the tensor compact_plain returns agree."""
    from liberate_fhe_amd._native import lib
    from liberate_fhe_amd.fhe.backend import SMALL_PRIME_LIMIT
    eng = checker
    N = eng.ctx.N
    mixes = []
    for level in (0, eng.num_levels - 2):
        q = primes_of(eng, level)
        small = [x < SMALL_PRIME_LIMIT for x in q]
        mixes.append((sum(small), len(q) - sum(small)))
        off = eng.plain_planes_offsets(q, N)
        assert off[0] == 0 and len(off) == len(q) + 1
        for r in range(len(q)):
            assert off[r] * 8 == sum(6 * N if s else 8 * N for s in small[:r]) and off[r] * 8 % 16 == 0
        assert off[-1] * 8 == (6 * sum(small) + 8 * (len(q) - sum(small))) * N
        arr = (ctypes.c_int64 * len(q))(*q)
        for r in range(1, len(q) + 1):
            assert lib.lf_plain_planes_words(r, N, arr) == off[r]
        pt = eng.encode_plain(message(eng, 3), level)
        c = eng.compact_plain(pt)
        assert len(c.data) == 1 and c.data[0].dim() == 1 and c.data[0].dtype == torch.int64 and c.data[0].numel() == off[-1]
        assert (c.level, c.hash, c.ntt_state, c.montgomery_state, c.include_special) == (level, pt.hash, True, True, False)
    assert mixes[0][0] >= 1 and mixes[0][1] >= 1 and mixes[0] != mixes[1]          # rows of both classes; another mix at the last level
    assert eng.num_levels - 2 > 0 and len(primes_of(eng, eng.num_levels - 2)) < len(primes_of(eng, 0))


def test_round_trip_on_edge_words(checker):
    """expand_plain(compact_plain(pt)) = pt mod q on every row, for 0, 1, q - 1, q, 2q - 1 and random lazy words; the stored
    fp64-class word is REDC(w) in [0, q] — q itself exactly where w = q — and an integer-class row is stored as it is."""
    from liberate_fhe_amd.fhe.backend import SMALL_PRIME_LIMIT
    from liberate_fhe_amd.fhe.presets import types
    eng = checker
    for level in (0, eng.num_levels - 2):
        pt = edge_words(eng, level)
        q = primes_of(eng, level)
        c = eng.compact_plain(pt)
        assert c.origin == types.origins["pt_mult_planes"]
        back = eng.expand_plain(c)
        assert back.origin == types.origins["pt_mult"] and back.level == level
        qcol = torch.tensor(q, dtype=torch.int64).view(-1, 1)
        assert torch.equal(back.data[0], pt.data[0] % qcol)
        assert eng.expand_plain(pt) is pt
        stored = eng._planes_unpack_rows(c.data[0], q, eng.ctx.N)
        R = eng.ctx.R
        for r, x in enumerate(q):
            w = pt.data[0][r]
            if x >= SMALL_PRIME_LIMIT:
                assert torch.equal(stored[r], w)
                continue
            rinv = pow(R, -1, x)
            want = [x if int(v) == x else int(v) * rinv % x for v in w[:64]]
            assert [int(v) for v in stored[r][:64]] == want
            assert int(stored[r].min()) >= 0 and int(stored[r].max()) <= x
        # the plaintexts encode_plain makes: the same residues back
        pt = eng.encode_plain(message(eng, 4), level)
        assert torch.equal(eng.expand_plain(eng.compact_plain(pt)).data[0], pt.data[0] % qcol)


def test_compact_plain_is_idempotent_and_encode_plain_takes_the_flag(checker, monkeypatch):
    from tests.test_pc_dot_cpu import recording_encode
    eng = checker
    pt = eng.encode_plain(message(eng, 6), 0)
    c = eng.compact_plain(pt)
    assert eng.compact_plain(c) is c
    e = eng.expand_plain(c)                                   # (canonical words: an integer-class row of c keeps its lazy ones)
    assert torch.equal(eng.expand_plain(eng.compact_plain(e)).data[0], e.data[0])
    log, replay = recording_encode(eng, monkeypatch)
    a = eng.encode_plain(message(eng, 7), 1)
    replay(log)
    b = eng.encode_plain(message(eng, 7), 1, compact=True)
    assert b.origin == c.origin and b.level == 1 and torch.equal(b.data[0], eng.compact_plain(a).data[0])


def test_refusals(checker, monkeypatch):
    """A pt_add, compact=True with op="add", compact and raw plaintexts mixed in each of the four ops, a compact operand at another
    level, a compact plaintext in a wrong state, at the top level, where an "add" plaintext belongs: refused with nothing
    computed."""
    from liberate_fhe_amd.fhe.presets import errors
    eng = checker
    m = message(eng, 1)
    top = eng.num_levels - 1
    p0, p1, a0, a1 = eng.encode_plain(m, 0), eng.encode_plain(m, 1), eng.encode_plain(m, 0, "add"), eng.encode_plain(m, 1, "add")
    k0, k1 = eng.compact_plain(p0), eng.compact_plain(p1)
    c0, c1, ctop = (synth.ciphertext(eng, 60 + i, lvl) for i, lvl in enumerate((0, 1, top)))
    ktop = k0._replace(level=top)
    coeff = k0._replace(ntt_state=False)
    calls = []

    def boom(name):
        def f(*a, **k):
            calls.append(name)
            raise AssertionError(name + " reached")
        return f

    with pytest.raises(errors.NotMatchType):
        eng.compact_plain(a0)
    with pytest.raises(errors.NotMatchType):
        eng.compact_plain(c0)
    with pytest.raises(errors.NotMatchType):
        eng.expand_plain(a0)
    with pytest.raises(ValueError):
        eng.encode_plain(m, 0, "add", compact=True)
    for name in ("_pc_matmul_native", "_pc_matmul_batch_native", "_pc_dot_native", "rescale", "clone", "_ws", "expand_plain"):
        monkeypatch.setattr(eng, name, boom(name))
    for name in ("enter_ntt", "mont_mult", "mont_add", "mont_enter", "intt_exit_reduce", "mont_redc", "reduce_2q"):
        monkeypatch.setattr(eng.ntt, name, boom(name))
    real_empty = torch.empty
    monkeypatch.setattr(torch, "empty", lambda *a, **k: (calls.append("empty"), real_empty(*a, **k))[1])
    mixed = [
        lambda: eng.pc_dot([(k0, c0), (p0, c0)]),
        lambda: eng.pc_dot([(p0, c0), (p0, c0), (k0, c0)], a1),
        lambda: eng.pc_matmul([[k0, p0]], [c0, c0]),
        lambda: eng.pc_matmul([[k0, None], [None, p0]], [c0, c0], [a1, None]),
        lambda: eng.pc_matmul_batch([[k0, k0], [p0, k0]], [[c0, c0], [c0, c0]]),
        lambda: eng.pc_matmul_batch([[p0], [k0]], [[c0]] * 3, [None, a1]),
    ]
    for call in mixed:
        with pytest.raises(ValueError, match="compact"):
            call()
    cases = [
        (errors.NotMatchDataStructState, lambda: eng.pc_mult(k0, c1)),                         # levels that differ
        (errors.NotMatchDataStructState, lambda: eng.pc_mult(k1, c0)),
        (errors.NotMatchDataStructState, lambda: eng.pc_dot([(k0, c0), (k1, c0)])),
        (errors.NotMatchDataStructState, lambda: eng.pc_dot([(k0, c0), (k0, c1)])),
        (errors.NotMatchDataStructState, lambda: eng.pc_matmul([[k0, k1]], [c0, c0])),
        (errors.NotMatchDataStructState, lambda: eng.pc_matmul([[k1]], [c0])),
        (errors.NotMatchDataStructState, lambda: eng.pc_matmul_batch([[k0]], [[c0], [c1]])),
        (errors.NotMatchDataStructState, lambda: eng.pc_mult(coeff, c0)),                      # a wrong state
        (errors.NotMatchDataStructState, lambda: eng.pc_dot([(coeff, c0)])),
        (errors.NotMatchDataStructState, lambda: eng.pc_dot([(k0, c0)], a0)),                  # a bias not at l + 1
        (errors.NotMatchType, lambda: eng.pc_dot([(k0, c0)], k1)),                             # a compact plaintext as bias
        (errors.NotMatchType, lambda: eng.pc_matmul([[k0]], [c0], [k1])),
        (errors.NotMatchType, lambda: eng.pc_add(k0, c0)),
        (errors.NotMatchType, lambda: eng.pc_dot([(k0, k0)])),
        (errors.MaximumLevelError, lambda: eng.pc_mult(ktop, ctop)),
        (errors.MaximumLevelError, lambda: eng.pc_dot([(ktop, ctop)])),
        (errors.MaximumLevelError, lambda: eng.pc_matmul([[ktop]], [ctop])),
        (errors.MaximumLevelError, lambda: eng.pc_matmul_batch([[ktop]], [[ctop], [ctop]])),
        (ValueError, lambda: eng.pc_matmul([[k0, None], [None, None]], [c0, c0])),
    ]
    for exc, call in cases:
        with pytest.raises(exc):
            call()
    assert calls == []
    monkeypatch.undo()
    assert eng.pc_mult(k0, c0).level == 1                                                      # and the engine still works


@pytest.mark.parametrize("level", [0, 2])
def test_the_four_ops_on_compact_plaintexts_equal_the_raw_ones(checker, level):
    """Word for word, on the checker backend (where the compact plaintexts are expanded for the call): pc_mult, pc_dot with and
    without bias, pc_matmul and pc_matmul_batch over holes, an all-None column, a partly-None bias, one object that repeats in W
    and across tokens — against the same call on the raw plaintexts and on expand_plain of the compact ones."""
    eng = checker
    assert eng.num_levels - 2 == 2
    for k_in, k_out in ((1, 1), (3, 2)) + (((chunk() + 1, 3),) if level == 0 else ((5, 5),)):
        W, cts, bias = layer_of(eng, k_in, k_out, level)
        K = compact_layer(eng, W)
        E = [[None if pt is None else eng.expand_plain(pt) for pt in row] for row in K]
        assert k_in < 3 or (any(b is None for b in bias) and all(row[1] is None for row in W) and W[1][0] is None)
        flat = [pt for row in K for pt in row if pt is not None]
        assert k_in < 5 or len({id(pt) for pt in flat}) < len(flat)                            # objects repeat in W
        for b in (None, bias):
            want = eng.pc_matmul(W, cts, b)
            for got in (eng.pc_matmul(K, cts, b), eng.pc_matmul(E, cts, b)):
                assert len(got) == k_out and all(same(g, w) for g, w in zip(got, want)), (k_in, k_out, level)
        X = tokens_of(eng, cts, 3, level)
        want = eng.pc_matmul_batch(W, X, bias)
        got = eng.pc_matmul_batch(iter([iter(row) for row in K]), (iter(tok) for tok in X), iter(bias))
        assert all(same(g, w) for gs, ws in zip(got, want) for g, w in zip(gs, ws))
        pairs = [(pt, ct) for pt, ct in zip(W[0], cts) if pt is not None]
        kpairs = [(pt, ct) for pt, ct in zip(K[0], cts) if pt is not None]
        for b in (None, next(x for x in bias if x is not None) if k_in >= 3 else bias[0]):
            assert same(eng.pc_dot(kpairs, b), eng.pc_dot(pairs, b))
        assert same(eng.pc_mult(kpairs[0][0], kpairs[0][1]), eng.pc_mult(*pairs[0]))
    # edge words: w = q is stored as q and expands to 0 — the same residue, the same result
    pt = edge_words(eng, level)
    ct = synth.ciphertext(eng, 9, level)
    assert same(eng.pc_mult(eng.compact_plain(pt), ct), eng.pc_mult(pt, ct))


def test_clone_cpu_cuda_save_load_round_trip(checker, tmp_path):
    """Bitwise, and the loaded object works in pc_dot."""
    eng = checker
    for level in (0, 2):
        pt = edge_words(eng, level, seed=8)
        c = eng.compact_plain(pt)
        ct = synth.ciphertext(eng, 11, level)
        want = eng.pc_dot([(pt, ct)])
        twin = eng.clone(c)
        assert twin.origin == c.origin and twin.data[0].data_ptr() != c.data[0].data_ptr() and torch.equal(twin.data[0], c.data[0])
        host = eng.cpu(c)
        assert host.origin == c.origin and len(host.data) == 1 and host.data[0].device.type == "cpu"
        back = eng.cuda(host)
        assert torch.equal(back.data[0], c.data[0]) and back.level == level
        path = tmp_path / f"compact{level}.pkl"
        eng.save(c, str(path))
        loaded = eng.load(str(path))
        assert loaded.origin == c.origin and loaded.level == level and loaded.hash == c.hash
        assert loaded.data[0].dtype == torch.int64 and torch.equal(loaded.data[0], c.data[0])
        for obj in (twin, back, loaded):
            assert same(eng.pc_dot([(obj, ct)]), want)
        on_host = eng.load(str(path), move_to_gpu=False)
        assert torch.equal(eng.cuda(on_host).data[0], c.data[0])


class Stub:
    """Records what the engine sends through the compact entry; everything else is the checker backend's."""
    native_ops = True
    pc_matmul_chunk = 16
    pc_matmul_max_outputs = 64
    pc_matmul_batch_sizes = (4, 2)
    plain_planes_max_rows = 64

    def __init__(self, inner):
        self._inner, self.calls, self.raw = inner, [], []

    def __getattr__(self, name):
        return getattr(self._inner, name)

    def pc_matmul_batch_planes_ws_words(self, nt, k_in, k_out, rows, logN):
        return 2

    def pc_matmul_batch_ws_words(self, nt, k_in, k_out, rows, logN):
        return 2

    def pc_matmul_batch_native(self, *a):
        self.raw.append(a[4])
        for tok in a[3]:
            for pair in tok:
                for c in pair:
                    c.zero_()

    def pc_matmul_batch_planes_call(self, ins, pts, biases, outs, nt, k_in, k_out, rows, logN, *rest):
        assert len(ins) == nt * 2 * k_in and len(pts) == k_out * k_in and len(outs) == nt and all(len(tok) == k_out for tok in outs)
        self.calls.append(dict(nt=nt, k_in=k_in, k_out=k_out, rows=rows, logN=logN, ins=list(ins), pts=list(pts),
                               biases=None if biases is None else list(biases)))
        for t, tok in enumerate(outs):
            for o, pair in enumerate(tok):
                for c in pair:
                    assert tuple(c.shape) == (rows - 1, 1 << logN)
                    c.fill_(10000 * len(self.calls) + 100 * t + o)


def test_what_the_engine_hands_the_entry(checker, monkeypatch):
    """Through a stub under the engine: pc_mult and pc_dot are nt = 1, k_out = 1; pc_matmul nt = 1; pc_matmul_batch pairs of tokens
    and nt = 1 for the one left over; the pointers are the compact tensors', in [output][input] order, NULL for a hole; the
    ciphertexts' in [token][input][component] order; nothing goes to the raw entry, and raw plaintexts never reach the compact one."""
    eng = checker
    W, cts, bias = layer_of(eng, 3, 2, 0)
    K = compact_layer(eng, W)
    X = tokens_of(eng, cts, 3, 0)
    stub = Stub(eng.backend)
    monkeypatch.setattr(eng, "backend", stub)
    monkeypatch.setattr(eng, "_pc_operand_ok", lambda t: t.is_contiguous() and t.dtype == torch.int64 and t.data_ptr() % 16 == 0)
    monkeypatch.setattr(eng, "_native_level", lambda lvl: 0)
    rows, logN = len(primes_of(eng, 0)), eng.ctx.logN
    ptr = lambda x: None if x is None else x.data[0].data_ptr()
    ins_of = lambda toks: [ct.data[c][0].data_ptr() for tok in toks for ct in tok for c in range(2)]

    out = eng.pc_mult(K[0][0], cts[0])
    assert out.level == 1 and int(out.data[0][0][0, 0]) == 10000
    assert stub.calls[-1] == dict(nt=1, k_in=1, k_out=1, rows=rows, logN=logN, ins=ins_of([[cts[0]]]), pts=[ptr(K[0][0])], biases=None)

    pairs = [(pt, ct) for pt, ct in zip(K[0], cts) if pt is not None]
    b = next(x for x in bias if x is not None)
    eng.pc_dot(pairs, b)
    assert stub.calls[-1] == dict(nt=1, k_in=2, k_out=1, rows=rows, logN=logN, ins=ins_of([[ct for _, ct in pairs]]),
                                  pts=[ptr(pt) for pt, _ in pairs], biases=[ptr(b)])

    n = len(stub.calls)
    got = eng.pc_matmul(K, cts, bias)
    assert len(stub.calls) == n + 1 and [int(o.data[1][0][0, 0]) for o in got] == [10000 * (n + 1), 10000 * (n + 1) + 1]
    assert stub.calls[-1] == dict(nt=1, k_in=3, k_out=2, rows=rows, logN=logN, ins=ins_of([cts]),
                                  pts=[ptr(pt) for row in K for pt in row], biases=[ptr(x) for x in bias])

    n = len(stub.calls)
    got = eng.pc_matmul_batch(K, X, bias)
    assert [(c["nt"], c["k_in"], c["k_out"]) for c in stub.calls[n:]] == [(2, 3, 2), (1, 3, 2)]
    assert stub.calls[n]["ins"] == ins_of(X[:2]) and stub.calls[n + 1]["ins"] == ins_of(X[2:])
    assert all(c["pts"] == [ptr(pt) for row in K for pt in row] and c["biases"] == [ptr(x) for x in bias] for c in stub.calls[n:])
    assert [[int(o.data[0][0][0, 0]) for o in tok] for tok in got] == \
        [[10000 * (n + 1), 10000 * (n + 1) + 1], [10000 * (n + 1) + 100, 10000 * (n + 1) + 101], [10000 * (n + 2), 10000 * (n + 2) + 1]]
    assert stub.raw == []
    # raw plaintexts keep to the raw entry
    n = len(stub.calls)
    eng.pc_matmul_batch(W, X[:2], bias)
    assert stub.raw == [2] and len(stub.calls) == n
    # 65 outputs: 64 + 1 per group of tokens
    n = len(stub.calls)
    eng.pc_matmul_batch([[K[0][0]]] * 65, [[cts[0]], [cts[1]]])
    assert [(c["nt"], c["k_out"]) for c in stub.calls[n:]] == [(2, 64), (2, 1)]


def test_c_entries_refuse_bad_arguments_before_any_device_call():
    """lf_pc_matmul_batch_planes, lf_plain_planes and lf_plain_unplanes return LF_ERR_ARG from their arguments alone (dummy pointers
    that are never dereferenced where a check refuses first; the primes are real host arrays), and the _words queries give 0 for
    what they refuse."""
    from liberate_fhe_amd._native import lib, EXPORTED, _SIGNATURES
    for name in ("lf_pc_matmul_batch_planes", "lf_pc_matmul_batch_planes_ws_words", "lf_plain_planes", "lf_plain_unplanes", "lf_plain_planes_words"):
        assert name in EXPORTED
    assert lib.lf_abi_version() == 15
    assert _SIGNATURES["lf_pc_matmul_batch_planes"] == _SIGNATURES["lf_pc_matmul_batch"]
    header = open(os.path.join(ROOT, "include", "ckks_hip.h")).read()
    CI = int(re.search(r"#define LF_PC_MATMUL_CI (\d+)", header).group(1))
    GMAX = int(re.search(r"#define LF_PC_MATMUL_MAX_OUTPUTS (\d+)", header).group(1))
    TMAX = int(re.search(r"#define LF_PC_MATMUL_BATCH_MAX_TOKENS (\d+)", header).group(1))
    RMAX = int(re.search(r"#define LF_PLAIN_PLANES_MAX_ROWS (\d+)", header).group(1))
    for nt in range(1, TMAX + 1):
        for logN in (13, 17):
            for rows in (2, 5, RMAX):
                for k_in, k_out in ((1, 1), (CI + 1, 3), (3 * CI, GMAX)):
                    assert lib.lf_pc_matmul_batch_planes_ws_words(nt, k_in, k_out, rows, logN) == \
                        lib.lf_pc_matmul_batch_ws_words(nt, k_in, k_out, rows, logN) == (2 * min(k_in, CI) + 2 * k_out) * nt * rows * (1 << logN)
    for nt, k_in, k_out, rows, logN in ((0, 1, 1, 3, 13), (TMAX + 1, 1, 1, 3, 13), (2, 0, 1, 3, 13), (2, 1, 0, 3, 13), (2, 1, GMAX + 1, 3, 13),
                                        (2, 1, 1, 1, 13), (2, 1, 1, RMAX + 1, 13), (2, 1, 1, 3, 12), (2, 1, 1, 3, 18)):
        assert lib.lf_pc_matmul_batch_planes_ws_words(nt, k_in, k_out, rows, logN) == 0, (nt, k_in, k_out, rows, logN)

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
        return lib.lf_pc_matmul_batch_planes(nt, k_in, k_out, a["ins"], a["pts"], a["bias"], a["out0"], a["out1"], rows, logN, a["psi"],
                                             a["psi_dp"], a["ipsi"], a["ipsi_dp"], a["q_host"], a["Rs"], a["Ninv"], a["one"], a["zero"],
                                             a["scales"], 0, a["ws"], ws_words, a["ql"], a["qh"], a["kl"], a["kh"], 0, None)

    for nt in (0, -1, TMAX + 1, 1 << 20):
        assert call(nt=nt) == LF_ERR_ARG, nt
    for k_in in (0, -1):
        assert call(k_in=k_in) == LF_ERR_ARG
    for k_out in (0, -1, GMAX + 1):
        assert call(k_out=k_out) == LF_ERR_ARG
    for rows in (1, 0, -1, RMAX + 1, lib.lf_limits(2)):
        assert call(rows=rows) == LF_ERR_ARG, rows
    for logN in (12, 18, 0):
        assert call(logN=logN) == LF_ERR_ARG, logN
    for n in names:
        if n != "bias":                                                  # (the biases are optional)
            assert call(**{n: None}) == LF_ERR_ARG, n
    for nt in range(1, TMAX + 1):
        for k_in, k_out in ((1, 1), (3, 2), (CI + 1, 5)):
            need = lib.lf_pc_matmul_batch_planes_ws_words(nt, k_in, k_out, 3, 13)
            assert call(nt=nt, k_in=k_in, k_out=k_out, ws_words=need - 1) == LF_ERR_ARG
            for at in (0, nt * 2 * k_in - 1):
                assert call(nt=nt, k_in=k_in, k_out=k_out, ins=ptrs(nt * 2 * k_in, [at])) == LF_ERR_ARG
            for at in (0, nt * k_out - 1):
                assert call(nt=nt, k_in=k_in, k_out=k_out, out0=ptrs(nt * k_out, [at])) == LF_ERR_ARG
                assert call(nt=nt, k_in=k_in, k_out=k_out, out1=ptrs(nt * k_out, [at])) == LF_ERR_ARG
            for o in (0, k_out - 1):                                         # an output row whose entries are all NULL
                assert call(nt=nt, k_in=k_in, k_out=k_out, pts=ptrs(k_in * k_out, range(o * k_in, (o + 1) * k_in))) == LF_ERR_ARG
    assert call(ws=ctypes.c_void_p(72)) == LF_ERR_ARG                    # 16-byte aligned
    assert call(ws_words=0) == LF_ERR_ARG

    # the packer and its inverse
    q = (ctypes.c_int64 * 3)((1 << 40) + 1, (1 << 41) + 1, (1 << 40) + 3)
    for logN in (13, 15, 17):
        N = 1 << logN
        assert lib.lf_plain_planes_words(3, N, q) == 3 * N - 2 * (N // 4) and lib.lf_plain_planes_words(1, N, q) == 3 * N // 4
        assert lib.lf_plain_planes_words(2, N, q) == 3 * N // 4 + N
    for rows, N, qq in ((0, 8192, q), (-1, 8192, q), (RMAX + 1, 8192, q), (3, 4096, q), (3, 1 << 18, q), (3, 8192 + 512, q), (3, 0, q), (3, 8192, None)):
        assert lib.lf_plain_planes_words(rows, N, qq) == 0, (rows, N)
    for fn in (lib.lf_plain_planes, lib.lf_plain_unplanes):
        def pk(src=64, dst=128, rows=3, N=8192, qq=q, ql=64, qh=64, kl=64, kh=64):
            return fn(src, dst, rows, N, qq, ql, qh, kl, kh, 0, None)
        for over in (dict(src=None), dict(dst=None), dict(qq=None), dict(ql=None), dict(qh=None), dict(kl=None), dict(kh=None), dict(dst=64),
                     dict(src=72), dict(dst=136), dict(rows=0), dict(rows=-1), dict(rows=RMAX + 1), dict(N=4096), dict(N=1 << 18),
                     dict(N=8192 + 512)):
            assert pk(**over) == LF_ERR_ARG, over


def test_the_new_kernels_use_no_scratch_and_the_raw_ones_have_not_moved():
    """Every tile the launch code selects for compact plaintexts (GO = 1 | 2 | 4 outputs x GT = 1 | 2 tokens; GT = 4 under
    LF_TUNE_PC_MATMUL_TILE) exists with scratch 0 and no spill, the default ones (GT <= 2) with at least 4 waves per SIMD; so do
    the packer and its inverse; the tracked table lists them as built; pc_matmul_kernel and pc_matmulb_kernel keep the figures
    the table had for them before (pc_matmul_kernel<2 | 4>: 69 / 85 VGPRs since the product bodies became one, 67 / 83 before, the
    waves per SIMD as they were)."""
    import __graft_entry__ as g
    res = {r["kernel"]: r for r in g.kernel_resources()}
    want = [f"pc_planes_matmul_kernel<{go}, {gt}>" for go in (1, 2, 4) for gt in (1, 2, 4)]
    assert sorted(k for k in res if k.startswith("pc_planes_matmul_kernel")) == sorted(want)
    src = open(os.path.join(ROOT, "liberate_fhe_amd", "csrc", "ckks_ks.hip")).read()
    launched = re.findall(r"LF_PCPL_CASE\((\d), (\d)\)", src.split("switch ((planes ? 64 : 0) + go * 8 + gt)")[1].split("}")[0])
    assert sorted(f"pc_planes_matmul_kernel<{go}, {gt}>" for go, gt in launched) == sorted(want)
    tracked = open(os.path.join(ROOT, "profiles", "r06_kernel_resources.txt")).read()
    for k in want + ["plain_planes_kernel", "plain_unplanes_kernel"]:
        r = res[k]
        assert r["file"] == "ckks_ks.hip" and r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["lds"] == 0, r
        assert r["occupancy"] >= (2 if k.endswith(", 4>") else 4), r
        line = next(ln for ln in tracked.splitlines() if ln[18:76].strip() == k)
        f = line.split()
        assert (int(f[-7]), int(f[-3]), int(f[-1])) == (r["vgprs"], r["scratch"], r["occupancy"]), line
    raw = {"pc_matmul_kernel<1>": (53, 8), "pc_matmul_kernel<2>": (69, 7), "pc_matmul_kernel<4>": (85, 5),
           "pc_matmulb_kernel<1, 2>": (84, 5), "pc_matmulb_kernel<2, 2>": (108, 4), "pc_matmulb_kernel<4, 2>": (125, 4),
           "pc_matmulb_kernel<1, 4>": (138, 3), "pc_matmulb_kernel<2, 4>": (164, 3), "pc_matmulb_kernel<4, 4>": (246, 2)}
    for k, (vgprs, occ) in raw.items():
        assert (res[k]["vgprs"], res[k]["occupancy"], res[k]["scratch"]) == (vgprs, occ, 0), res[k]
