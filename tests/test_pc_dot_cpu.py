"""Encoded plaintexts (ckks_engine.encode_plain, pc_mult, pc_add, pc_dot; lf_pc_dot: a sum of plaintext-ciphertext products under
one rescale) without a GPU: the engine's host logic on the checker backend against mc_mult / mc_add and against the composition
of public steps that defines pc_dot's words, the refusals, persistence, the decryption error with real keys against the loop of
mc_mults, the C entry's argument checks and the new kernels' resources."""
import ctypes
import os

import numpy as np
import pytest
import torch

from liberate_fhe_amd.utils import synth
from tests.test_cc_dot_cpu import lazy_ciphertext, same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PC = dict(logN=13, num_scales=4, num_special_primes=2, is_secured=False)


@pytest.fixture(scope="module")
def checker():
    from liberate_fhe_amd.fhe import ckks_engine
    from tests.oracle_backend import OracleBackend
    return ckks_engine(devices=["cpu"], backend=OracleBackend(), **PC)


def message(eng, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, eng.num_slots) + 1j * rng.uniform(-1, 1, eng.num_slots)


def recording_encode(eng, monkeypatch):
    """engine.encode records every polynomial it returns; replay(log) makes it hand the recorded ones out again, in order."""
    real = eng.encode
    log = []

    def record(*a, **k):
        out = real(*a, **k)
        log.append([t.clone() for t in out])
        return out

    monkeypatch.setattr(eng, "encode", record)

    def replay(polys):
        it = iter(polys)
        monkeypatch.setattr(eng, "encode", lambda *a, **k: [t.clone() for t in next(it)])

    return log, replay


def composition(eng, pairs, bias=None):
    """The definition of pc_dot's words, written out from the ntt ops and rescale."""
    from liberate_fhe_amd.fhe.presets import types
    l = pairs[0][1].level
    S = None
    for pt, ct in pairs:
        term = []
        for comp in range(2):
            x = [t.clone() for t in ct.data[comp]]
            eng.ntt.enter_ntt(x, l)
            term.append(eng.ntt.mont_mult(pt.data, x, l))
        S = term if S is None else [eng.ntt.mont_add(S[c], term[c], l) for c in range(2)]
    for c in range(2):
        eng.ntt.intt_exit_reduce(S[c], l)
    out = eng.rescale(eng._new(S, types.origins["ct"], level=l))
    if bias is not None:
        c0 = [t.clone() for t in out.data[0]]
        eng.ntt.mont_enter(c0, l + 1)
        c0 = eng.ntt.mont_add(bias.data, c0, l + 1)
        eng.ntt.mont_redc(c0, l + 1)
        eng.ntt.reduce_2q(c0, l + 1)
        out = out._replace(data=[c0, out.data[1]])
    return out


def terms_of(eng, k, level):
    """k pairs over three plaintexts and three ciphertexts (two of them with lazy words); objects repeat on both sides."""
    pts = [eng.encode_plain(message(eng, 20 + i), level) for i in range(3)]
    cts = [lazy_ciphertext(eng, 40 + level, level), synth.ciphertext(eng, 41 + level, level), lazy_ciphertext(eng, 42 + level, level)]
    order = [(0, 0), (1, 1), (0, 2), (2, 0), (1, 0)]       # pt 0 and ct 0 repeat
    return [(pts[p], cts[c]) for p, c in order[:k]]


def test_same_words_as_mc_mult_and_mc_add(checker, monkeypatch):
    """With engine.encode replaying the polynomials it returned for encode_plain, pc_mult(encode_plain(m, l), ct) has mc_mult(m, ct)'s
    words and pc_add(encode_plain(m, l, "add"), ct) has mc_add(m, ct)'s — at level 0 and at the last legal level of each."""
    from liberate_fhe_amd.fhe.presets import types
    eng = checker
    top = eng.num_levels - 1
    for level in (0, top - 1, top):
        m, ct = message(eng, 3 + level), synth.ciphertext(eng, 30 + level, level)
        log, replay = recording_encode(eng, monkeypatch)
        pa = eng.encode_plain(m, level, "add")
        pm = eng.encode_plain(m, level) if level < top else None
        assert pa.origin == types.origins["pt_add"] and pa.level == level and not pa.ntt_state and pa.montgomery_state
        assert len(pa.data) == len(ct.data[0]) and all(p.shape == c.shape for p, c in zip(pa.data, ct.data[0]))
        replay(log)
        assert same(eng.pc_add(pa, ct), eng.mc_add(m, ct)), level
        if pm is not None:
            assert pm.origin == types.origins["pt_mult"] and pm.level == level and pm.ntt_state and pm.montgomery_state
            assert not pm.include_special and all(p.shape == c.shape for p, c in zip(pm.data, ct.data[0]))
            got = eng.pc_mult(pm, ct)
            assert got.level == level + 1 and same(got, eng.mc_mult(m, ct)), level
            assert same(eng.pc_dot([(pm, ct)]), got), level              # one pair without bias: pc_mult's words
        monkeypatch.undo()


@pytest.mark.parametrize("level", [0, 2])
def test_pc_dot_equals_the_composition(checker, level):
    """k = 1, 2, 5, with and without bias, ciphertexts with lazy words, a repeated ciphertext and a repeated plaintext."""
    from liberate_fhe_amd.fhe.presets import types
    eng = checker
    bias = eng.encode_plain(message(eng, 9), level + 1, "add")
    for k in (1, 2, 5):
        pairs = terms_of(eng, k, level)
        for b in (None, bias):
            got = eng.pc_dot(pairs, b)
            assert got.level == level + 1 and got.origin == types.origins["ct"] and not got.ntt_state and not got.include_special
            assert same(got, composition(eng, pairs, b)), (level, k, b is not None)
    pt, ct = terms_of(eng, 1, level)[0]
    assert same(eng.pc_dot([(pt, ct), (pt, ct)]), composition(eng, [(pt, ct)] * 2))
    assert same(eng.pc_dot(iter([[pt, ct]]), bias), eng.pc_add(bias, eng.pc_mult(pt, ct)))   # any iterable, lists as pairs


def test_refusals_come_before_any_backend_call(checker, monkeypatch):
    """Every refusal is raised before the backend is called or a tensor is allocated."""
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
    calls = []
    real_empty = torch.empty
    monkeypatch.setattr(torch, "empty", lambda *a, **k: (calls.append("empty"), real_empty(*a, **k))[1])
    for name in ("enter_ntt", "mont_mult", "mont_add", "mont_enter", "intt_exit_reduce", "mont_redc", "reduce_2q"):
        real = getattr(eng.ntt, name)
        monkeypatch.setattr(eng.ntt, name, lambda *a, _n=name, _r=real, **k: (calls.append(_n), _r(*a, **k))[1])
    for name in ("rescale", "clone", "_ws"):
        real = getattr(eng, name)
        monkeypatch.setattr(eng, name, lambda *a, _n=name, _r=real, **k: (calls.append(_n), _r(*a, **k))[1])
    dot_cases = [
        (ValueError, [], None),
        (ValueError, [(p0,)], None),
        (errors.NotMatchType, [(a0, c0)], None),                       # an "add" plaintext in a product
        (errors.NotMatchType, [(p0, c0), (c0, c0)], None),             # a ciphertext where a plaintext belongs
        (errors.NotMatchType, [(p0, p0)], None),                       # .. and the other way round
        (errors.NotMatchType, [(p0, None)], None),
        (errors.NotMatchType, [(p0, c0)], p1),                         # a "mult" plaintext as bias
        (errors.NotMatchType, [(p0, c0)], c1),
        (errors.NotMatchDataStructState, [(p0, c0), (p1, c1)], None),  # levels that differ
        (errors.NotMatchDataStructState, [(p1, c0)], None),
        (errors.NotMatchDataStructState, [(p0, c0)], a0),              # a bias not at l + 1
        (errors.NotMatchDataStructState, [(p0, c0)], a2),
        (errors.NotMatchDataStructState, [(p0, ntt)], None),
        (errors.NotMatchDataStructState, [(p0, special)], a1),
        (errors.MaximumLevelError, [(ptop, ctop)], None),
    ]
    for exc, pairs, bias in dot_cases:
        with pytest.raises(exc):
            eng.pc_dot(pairs, bias)
    for fn, exc, pt, ct in [
        (eng.pc_mult, errors.NotMatchType, a0, c0), (eng.pc_mult, errors.NotMatchType, c0, c0), (eng.pc_mult, errors.NotMatchType, p0, p0),
        (eng.pc_mult, errors.NotMatchDataStructState, p0, c1), (eng.pc_mult, errors.NotMatchDataStructState, p0, ntt),
        (eng.pc_mult, errors.NotMatchDataStructState, p0, special), (eng.pc_mult, errors.MaximumLevelError, ptop, ctop),
        (eng.pc_add, errors.NotMatchType, p0, c0), (eng.pc_add, errors.NotMatchType, a0, a0),
        (eng.pc_add, errors.NotMatchDataStructState, a1, c0), (eng.pc_add, errors.NotMatchDataStructState, a0, ntt),
    ]:
        with pytest.raises(exc):
            fn(pt, ct)
    assert calls == []
    monkeypatch.undo()
    with pytest.raises(errors.MaximumLevelError):
        eng.encode_plain(m, top)                                          # a "mult" plaintext needs a level to rescale into
    with pytest.raises(ValueError):
        eng.encode_plain(m, 0, "sub")
    assert eng.pc_dot([(p0, c0)], a1).level == 1                          # and the engine still works


def test_persistence(checker, tmp_path):
    """save / load / cpu / cuda / clone treat the encoded plaintexts like any container; pc_dot on the loaded copies gives the
    same words; a file that names a global outside the allow-list is still refused."""
    import pickle
    eng = checker
    pairs = terms_of(eng, 2, 0)
    bias = eng.encode_plain(message(eng, 9), 1, "add")
    want = eng.pc_dot(pairs, bias)
    loaded = []
    for i, obj in enumerate([pairs[0][0], pairs[1][0], bias]):
        path = tmp_path / f"pt{i}.pkl"
        eng.save(obj, str(path))
        back = eng.load(str(path))
        assert back.origin == obj.origin and back.level == obj.level and back.ntt_state == obj.ntt_state
        assert back.montgomery_state == obj.montgomery_state and back.hash == obj.hash
        assert all(torch.equal(a, b) for a, b in zip(back.data, obj.data))
        host = eng.load(str(path), move_to_gpu=False)
        assert all(torch.equal(a, b) for a, b in zip(eng.cuda(host).data, obj.data))
        copy = eng.clone(eng.cuda(eng.cpu(back)))
        assert all(torch.equal(a, b) and a.data_ptr() != b.data_ptr() for a, b in zip(copy.data, obj.data))
        loaded.append(copy)
    assert same(eng.pc_dot([(loaded[0], pairs[0][1]), (loaded[1], pairs[1][1])], loaded[2]), want)
    evil = tmp_path / "evil.pkl"
    evil.write_bytes(pickle.dumps(os.getcwd))
    with pytest.raises(pickle.UnpicklingError):
        eng.load(str(evil))


def test_real_keys_decrypt_within_twice_the_loop_of_mc_mults():
    """Real keys on the checker engine, k = 3 random real vectors with |.| <= 1 against three encrypted ones, and a bias: pc_dot's
    maximum decryption error against float64 is at most 2 x that of the mc_mult / cc_add / mc_add loop on the same inputs (the
    sum takes one rescale rounding instead of three; the factor covers the independent random roundings of the two sets of
    encodings).  Measured on this ring: pc_dot 1.57e-10, the loop 1.65e-10 (both printed)."""
    from liberate_fhe_amd.fhe import ckks_engine
    from tests.oracle_backend import OracleBackend
    eng = ckks_engine(devices=["cpu"], backend=OracleBackend(), **PC)
    sk = eng.create_secret_key()
    pk = eng.create_public_key(sk)
    rng = np.random.default_rng(12)
    n = eng.num_slots
    ws = [rng.uniform(-1, 1, n) for _ in range(3)]
    xs = [rng.uniform(-1, 1, n) for _ in range(3)]
    b = rng.uniform(-1, 1, n)
    cts = [eng.encorypt(x, pk) for x in xs]
    want = sum(w * x for w, x in zip(ws, xs)) + b
    got = eng.pc_dot([(eng.encode_plain(w, 0), ct) for w, ct in zip(ws, cts)], eng.encode_plain(b, 1, "add"))
    assert got.level == 1
    loop = None
    for w, ct in zip(ws, cts):
        p = eng.mc_mult(w, ct)
        loop = p if loop is None else eng.cc_add(loop, p)
    loop = eng.mc_add(b, loop)
    e_dot = np.abs(eng.decrode(got, sk).real - want).max()
    e_loop = np.abs(eng.decrode(loop, sk).real - want).max()
    print(f"logN 13, k = 3 + bias, level 0: max abs error pc_dot {e_dot:.3e}, mc_mult / cc_add / mc_add loop {e_loop:.3e}, "
          f"largest entry {np.abs(want).max():.2f}")
    assert e_dot <= 2 * e_loop and e_loop < 1e-5


def test_c_entry_refuses_bad_arguments_before_any_device_call():
    """lf_pc_dot returns LF_ERR_ARG from its arguments alone (dummy pointers that are never dereferenced; no call here would pass
    the checks), and lf_pc_dot_ws_words gives (2 min(k, 4) + 2) rows N, 0 for the shapes the entry refuses."""
    from liberate_fhe_amd._native import lib, EXPORTED
    LF_ERR_ARG = 10001
    assert "lf_pc_dot" in EXPORTED and "lf_pc_dot_ws_words" in EXPORTED and lib.lf_abi_version() == 15
    max_rows = lib.lf_limits(2)
    for logN in (13, 15, 17):
        for rows in (2, 5, max_rows):
            for k in (1, 2, 3, 4, 5, 9, 16):
                assert lib.lf_pc_dot_ws_words(k, rows, logN) == (2 * min(k, 4) + 2) * rows * (1 << logN), (k, rows, logN)
    for k, rows, logN in ((0, 3, 13), (-1, 3, 13), (1, 1, 13), (1, 0, 13), (1, max_rows + 1, 13), (1, 3, 12), (1, 3, 18), (1, 3, 0)):
        assert lib.lf_pc_dot_ws_words(k, rows, logN) == 0, (k, rows, logN)

    def ptrs(n, null_at=None):
        arr = (ctypes.c_void_p * max(n, 1))(*([64] * max(n, 1)))
        if null_at is not None:
            arr[null_at] = None
        return arr

    names = ("ins", "pts", "bias", "out0", "out1", "psi", "psi_dp", "ipsi", "ipsi_dp", "q_host", "Rs", "Ninv", "one", "zero", "scales",
             "ws", "ql", "qh", "kl", "kh")

    def call(k=2, rows=3, logN=13, ws_words=1 << 40, **over):
        a = {n: ctypes.c_void_p(64) for n in names}
        a["ins"], a["pts"] = ptrs(2 * max(k, 1)), ptrs(max(k, 1))
        a.update(over)
        return lib.lf_pc_dot(k, a["ins"], a["pts"], a["bias"], a["out0"], a["out1"], rows, logN, a["psi"], a["psi_dp"], a["ipsi"],
                             a["ipsi_dp"], a["q_host"], a["Rs"], a["Ninv"], a["one"], a["zero"], a["scales"], 0, a["ws"], ws_words,
                             a["ql"], a["qh"], a["kl"], a["kh"], 0, None)

    for k in (0, -1):
        assert call(k=k) == LF_ERR_ARG
    for rows in (1, 0, -1, max_rows + 1):
        assert call(rows=rows) == LF_ERR_ARG, rows
    for logN in (12, 18, 0):
        assert call(logN=logN) == LF_ERR_ARG, logN
    for n in names:
        if n != "bias":                                                  # (the bias is optional)
            assert call(**{n: None}) == LF_ERR_ARG, n
    for k in (1, 3, 9):
        need = lib.lf_pc_dot_ws_words(k, 3, 13)
        assert call(k=k, ws_words=need - 1) == LF_ERR_ARG
        for at in (0, 2 * k - 1, k):
            assert call(k=k, ins=ptrs(2 * k, at)) == LF_ERR_ARG
        for at in (0, k - 1):
            assert call(k=k, pts=ptrs(k, at)) == LF_ERR_ARG
    assert call(ws=ctypes.c_void_p(72)) == LF_ERR_ARG                    # 16-byte aligned
    assert call(ws_words=0) == LF_ERR_ARG


def test_pc_dot_kernels_use_no_scratch():
    """pc_dot_kernel<1 | 2 | 4> and pc_bias_kernel exist under their own names with scratch 0, no spill and at least 4 waves per
    SIMD (streaming kernels); the tracked table lists them as built."""
    import __graft_entry__ as g
    res = {r["kernel"]: r for r in g.kernel_resources()}
    want = [f"pc_dot_kernel<{n}>" for n in (1, 2, 4)] + ["pc_bias_kernel"]
    assert sorted(k for k in res if k.startswith(("pc_dot_kernel", "pc_bias_kernel"))) == sorted(want)
    tracked = open(os.path.join(ROOT, "profiles", "r06_kernel_resources.txt")).read()
    for k in want:
        r = res[k]
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, r
        assert r["occupancy"] >= 4, r
        line = next(ln for ln in tracked.splitlines() if ln[18:76].strip() == k)
        f = line.split()
        assert (int(f[-7]), int(f[-3]), int(f[-1])) == (r["vgprs"], r["scratch"], r["occupancy"]), line
