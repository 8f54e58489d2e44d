"""pc_matmul (a plaintext matrix times a vector of ciphertexts; lf_pc_matmul) without a GPU: the engine's host logic on the
checker backend against the list of pc_dots and the written-out composition that define its words, the refusals, two logical
devices, the C entry's argument checks and the new kernels' resources."""
import ctypes
import os
import re

import pytest
import torch

from liberate_fhe_amd.utils import synth
from tests.test_cc_dot_cpu import lazy_ciphertext, same
from tests.test_pc_dot_cpu import PC, composition, message

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def checker():
    from liberate_fhe_amd.fhe import ckks_engine
    from tests.oracle_backend import OracleBackend
    return ckks_engine(devices=["cpu"], backend=OracleBackend(), **PC)


def layer_of(eng, k_in, k_out, level, seed=20):
    """(W, cts, bias) over three plaintexts, three ciphertexts (two with lazy words) and two biases, objects repeating on both
    sides; from 3 x 2 on: a hole in every second row, column 1 all None, and a partly-None bias."""
    pts = [eng.encode_plain(message(eng, seed + i), level) for i in range(3)]
    pool = [lazy_ciphertext(eng, seed + 20 + level, level), synth.ciphertext(eng, seed + 21 + level, level),
            lazy_ciphertext(eng, seed + 22 + level, level)]
    adds = [eng.encode_plain(message(eng, seed + 30 + i), level + 1, "add") for i in range(2)]
    cts = [pool[(2 * i) % 3] for i in range(k_in)]                  # ciphertext objects repeat from k_in = 4 on
    W = [[pts[(o + 2 * i) % 3] for i in range(k_in)] for o in range(k_out)]
    bias = [adds[o % 2] for o in range(k_out)]
    if k_in >= 3:
        for o in range(k_out):
            W[o][1] = None                                          # a ciphertext no output uses
            if o % 2:
                W[o][0] = None                                      # a hole in every second row
        bias[0] = None
    return W, cts, bias


def dots_of(eng, W, cts, bias=None):
    """The definition: one pc_dot per row over its non-None entries."""
    bias = [None] * len(W) if bias is None else bias
    return [eng.pc_dot([(pt, ct) for pt, ct in zip(row, cts) if pt is not None], b) for row, b in zip(W, bias)]


@pytest.mark.parametrize("level", [0, 2])
@pytest.mark.parametrize("shape", [(1, 1), (3, 2), (5, 5)])
def test_pc_matmul_equals_the_pc_dots_and_the_composition(checker, level, shape):
    """Level 0 and the last legal one (2 of the 4 levels of this ring), with holes, an all-None column, repeated objects, with
    and without bias, a partly-None bias: the list of pc_dots and the composition written out from the ntt ops, word for word."""
    from liberate_fhe_amd.fhe.presets import types
    eng = checker
    assert eng.num_levels - 2 == 2
    W, cts, bias = layer_of(eng, *shape, level)
    assert shape == (1, 1) or (bias[0] is None and all(row[1] is None for row in W) and W[1][0] is None and W[0][0] is not None)
    for b in (None, bias):
        got = eng.pc_matmul(W, cts, b)
        want = dots_of(eng, W, cts, b)
        assert isinstance(got, list) and len(got) == shape[1]
        for o, (g, w) in enumerate(zip(got, want)):
            assert g.level == level + 1 and g.origin == types.origins["ct"] and not g.ntt_state and not g.include_special
            assert same(g, w), (shape, level, o, b is not None)
            pairs = [(pt, ct) for pt, ct in zip(W[o], cts) if pt is not None]
            assert same(g, composition(eng, pairs, None if b is None else b[o])), (shape, level, o)
    # any iterables; the same plaintext and the same ciphertext everywhere
    pt, ct = next(p for p in W[0] if p is not None), cts[0]
    got = eng.pc_matmul(iter([(pt, pt), iter([pt, None])]), (c for c in (ct, ct)), iter([None, bias[-1]]))
    assert same(got[0], composition(eng, [(pt, ct)] * 2)) and same(got[1], composition(eng, [(pt, ct)], bias[-1]))


def test_refusals_come_before_pc_dot_and_the_backend(checker, monkeypatch):
    """Every refusal is raised with nothing computed: pc_dot, the native call, the ntt ops and every allocation are patched to
    record, and none is reached."""
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
    calls = []

    def boom(name):
        def f(*a, **k):
            calls.append(name)
            raise AssertionError(name + " reached")
        return f

    monkeypatch.setattr(eng, "pc_dot", boom("pc_dot"))
    monkeypatch.setattr(eng, "_pc_matmul_native", boom("_pc_matmul_native"))
    monkeypatch.setattr(eng.backend, "pc_matmul_native", boom("pc_matmul_native"), raising=False)
    monkeypatch.setattr(eng.backend, "pc_dot_native", boom("pc_dot_native"), raising=False)
    real_empty = torch.empty
    monkeypatch.setattr(torch, "empty", lambda *a, **k: (calls.append("empty"), real_empty(*a, **k))[1])
    for name in ("enter_ntt", "mont_mult", "mont_add", "mont_enter", "intt_exit_reduce", "mont_redc", "reduce_2q"):
        monkeypatch.setattr(eng.ntt, name, boom(name))
    for name in ("rescale", "clone", "_ws"):
        monkeypatch.setattr(eng, name, boom(name))
    cases = [
        (ValueError, [], [c0], None),                                             # W empty
        (ValueError, [[p0]], [], None),
        (ValueError, [[p0, p0], [p0]], [c0, c0], None),                           # ragged
        (ValueError, [[p0], [p0]], [c0, c0], None),                               # len(W[o]) != len(cts)
        (ValueError, [[p0, p0, p0]], [c0, c0], None),
        (ValueError, [[p0, None], [None, None]], [c0, c0], None),                 # a row with no entry
        (errors.NotMatchType, [[a0]], [c0], None),                                # an "add" plaintext in the matrix
        (errors.NotMatchType, [[p0, c0]], [c0, c0], None),                        # a ciphertext where a plaintext belongs
        (errors.NotMatchType, [[p0]], [p0], None),                                # .. and the other way round
        (errors.NotMatchType, [[p0, None]], [c0, None], None),                    # (a None ciphertext, even in an unused column)
        (errors.NotMatchType, [[p0]], [c0], [p1]),                                # a "mult" plaintext as bias
        (errors.NotMatchType, [[p0]], [c0], [c1]),
        (errors.NotMatchDataStructState, [[coeff_pt]], [c0], None),               # a wrong state of the plaintext
        (errors.NotMatchDataStructState, [[p0]], [ntt], None),                    # .. of the ciphertext
        (errors.NotMatchDataStructState, [[p0]], [special], [a1]),
        (errors.NotMatchDataStructState, [[p0, p0]], [c0, c1], None),             # levels that differ
        (errors.NotMatchDataStructState, [[p0, p1]], [c0, c0], None),
        (errors.NotMatchDataStructState, [[p0], [p1]], [c0], None),
        (errors.NotMatchDataStructState, [[p1]], [c0], None),
        (errors.NotMatchDataStructState, [[p0, None]], [c0, c1], None),           # (an unused column is still of the level)
        (ValueError, [[p0], [p0]], [c0], [a1]),                                   # len(bias) != k_out
        (ValueError, [[p0]], [c0], []),
        (errors.NotMatchDataStructState, [[p0], [p0]], [c0], [None, a0]),         # a bias not at l + 1
        (errors.NotMatchDataStructState, [[p0]], [c0], [a2]),
        (errors.MaximumLevelError, [[ptop]], [ctop], None),
        (errors.MaximumLevelError, [[ptop, None], [ptop, ptop]], [ctop, ctop], None),
    ]
    for exc, W, cts, bias in cases:
        with pytest.raises(exc):
            eng.pc_matmul(W, cts, bias)
    assert calls == []
    monkeypatch.undo()
    out = eng.pc_matmul([[p0, None], [p0, p0]], [c0, c0], [None, a1])         # and the engine still works
    assert [o.level for o in out] == [1, 1]


def test_two_logical_devices_give_the_single_device_words():
    """Two shards take the composition (no native level); row by row in prime order the words of one device.  The plaintexts
    are carried over in the host form (the polynomial encode returns is random)."""
    from liberate_fhe_amd.fhe import ckks_engine
    from tests.oracle_backend import OracleBackend
    from tests.test_pc_dot_gpu import natural_rows
    one = ckks_engine(devices=["cpu"], backend=OracleBackend(), **PC)
    two = ckks_engine(devices=["cpu"] * 2, backend=OracleBackend(), **PC)
    assert two._native_level(1) is None
    hosts = [one.cpu(one.encode_plain(message(one, 5 + i), 0)) for i in range(3)] + [one.cpu(one.encode_plain(message(one, 9), 1, "add"))]
    res = []
    for eng in (one, two):
        *pts, add = [eng.cuda(h._replace(hash=eng.hash)) for h in hosts]
        cts = [synth.ciphertext(eng, 8 + i, 0) for i in range(3)]
        W = [[pts[0], None, pts[1]], [pts[2], None, pts[0]], [None, None, pts[1]]]
        out = eng.pc_matmul(W, cts, [add, None, add])
        assert len(out) == 3 and all(o.level == 1 for o in out)
        res.append([natural_rows(eng, o) for o in out])
    for a, b in zip(*res):
        for x, y in zip(a, b):
            assert x.shape == y.shape and (x == y).all()


def test_c_entry_refuses_bad_arguments_before_any_device_call():
    """lf_pc_matmul returns LF_ERR_ARG from its arguments alone (dummy pointers that are never dereferenced; no call here would
    pass the checks), and lf_pc_matmul_ws_words gives (2 min(k_in, CI) + 2 k_out) rows N, 0 for the shapes the entry refuses."""
    from liberate_fhe_amd import _native
    from liberate_fhe_amd._native import lib, EXPORTED
    from liberate_fhe_amd.fhe.backend import HipBackend
    LF_ERR_ARG = 10001
    assert "lf_pc_matmul" in EXPORTED and "lf_pc_matmul_ws_words" in EXPORTED and lib.lf_abi_version() == 15
    header = open(os.path.join(ROOT, "include", "ckks_hip.h")).read()
    CI = int(re.search(r"#define LF_PC_MATMUL_CI (\d+)", header).group(1))
    GMAX = int(re.search(r"#define LF_PC_MATMUL_MAX_OUTPUTS (\d+)", header).group(1))
    assert (CI, GMAX) == (_native.LF_PC_MATMUL_CI, _native.LF_PC_MATMUL_MAX_OUTPUTS) == (HipBackend.pc_matmul_chunk, HipBackend.pc_matmul_max_outputs)
    assert 1 <= CI <= 125 and GMAX == 64           # the fp64 bound of a chunk (CI q / 2 + q < 64 q); the issue's 64 outputs
    max_rows = lib.lf_limits(2)
    for logN in (13, 15, 17):
        for rows in (2, 5, max_rows):
            for k_in in (1, 2, 5, CI - 1, CI, CI + 1, 3 * CI):
                for k_out in (1, 2, 3, 4, 5, 9, GMAX):
                    assert lib.lf_pc_matmul_ws_words(k_in, k_out, rows, logN) == (2 * min(k_in, CI) + 2 * k_out) * rows * (1 << logN)
    for k_in, k_out, rows, logN in ((0, 1, 3, 13), (-1, 1, 3, 13), (1, 0, 3, 13), (1, -1, 3, 13), (1, GMAX + 1, 3, 13), (1, 1, 1, 13),
                                    (1, 1, 0, 13), (1, 1, max_rows + 1, 13), (1, 1, 3, 12), (1, 1, 3, 18), (1, 1, 3, 0)):
        assert lib.lf_pc_matmul_ws_words(k_in, k_out, rows, logN) == 0, (k_in, k_out, rows, logN)

    def ptrs(n, null_at=()):
        arr = (ctypes.c_void_p * max(n, 1))(*([64] * max(n, 1)))
        for at in null_at:
            arr[at] = None
        return arr

    names = ("ins", "pts", "bias", "out0", "out1", "psi", "psi_dp", "ipsi", "ipsi_dp", "q_host", "Rs", "Ninv", "one", "zero", "scales",
             "ws", "ql", "qh", "kl", "kh")

    def call(k_in=2, k_out=3, rows=3, logN=13, ws_words=1 << 40, **over):
        a = {n: ctypes.c_void_p(64) for n in names}
        ki, ko = max(k_in, 1), max(k_out, 1)
        a["ins"], a["pts"], a["bias"], a["out0"], a["out1"] = ptrs(2 * ki), ptrs(ki * ko), ptrs(ko), ptrs(ko), ptrs(ko)
        a.update(over)
        return lib.lf_pc_matmul(k_in, k_out, a["ins"], a["pts"], a["bias"], a["out0"], a["out1"], rows, logN, a["psi"], a["psi_dp"],
                                a["ipsi"], a["ipsi_dp"], a["q_host"], a["Rs"], a["Ninv"], a["one"], a["zero"], a["scales"], 0, a["ws"],
                                ws_words, a["ql"], a["qh"], a["kl"], a["kh"], 0, None)

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
    for k_in, k_out in ((1, 1), (3, 2), (CI + 1, 5)):
        need = lib.lf_pc_matmul_ws_words(k_in, k_out, 3, 13)
        assert call(k_in=k_in, k_out=k_out, ws_words=need - 1) == LF_ERR_ARG
        for at in (0, 2 * k_in - 1, k_in):
            assert call(k_in=k_in, k_out=k_out, ins=ptrs(2 * k_in, [at])) == LF_ERR_ARG
        for at in (0, k_out - 1):
            assert call(k_in=k_in, k_out=k_out, out0=ptrs(k_out, [at])) == LF_ERR_ARG
            assert call(k_in=k_in, k_out=k_out, out1=ptrs(k_out, [at])) == LF_ERR_ARG
        for o in (0, k_out - 1):                                         # an output row whose entries are all NULL
            assert call(k_in=k_in, k_out=k_out, pts=ptrs(k_in * k_out, range(o * k_in, (o + 1) * k_in))) == LF_ERR_ARG
    assert call(ws=ctypes.c_void_p(72)) == LF_ERR_ARG                    # 16-byte aligned
    assert call(ws_words=0) == LF_ERR_ARG


def test_pc_matmul_kernels_use_no_scratch():
    """pc_matmul_kernel<1 | 2 | 4> exist under their own names with scratch 0, no spill and at least 4 waves per SIMD (streaming
    kernels); the tracked table lists them as built."""
    import __graft_entry__ as g
    res = {r["kernel"]: r for r in g.kernel_resources()}
    want = [f"pc_matmul_kernel<{n}>" for n in (1, 2, 4)]
    assert sorted(k for k in res if k.startswith("pc_matmul_kernel")) == sorted(want)
    tracked = open(os.path.join(ROOT, "profiles", "r06_kernel_resources.txt")).read()
    for k in want:
        r = res[k]
        assert r["file"] == "ckks_ks.hip" and r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, r
        assert r["occupancy"] >= 4, r
        line = next(ln for ln in tracked.splitlines() if ln[18:76].strip() == k)
        f = line.split()
        assert (int(f[-7]), int(f[-3]), int(f[-1])) == (r["vgprs"], r["scratch"], r["occupancy"]), line
