"""Compact plaintexts on the GPU: the native packer (lf_plain_planes) and its inverse against the host implementation between
guards; pc_mult, pc_dot, pc_matmul and pc_matmul_batch on compact plaintexts (lf_pc_matmul_batch_planes: pc_planes_matmul_kernel<GO, GT>)
against the raw native calls and the generic composition, word for word, with the backend calls counted; worst-case words against
the checker engine; the large rings; outputs, workspace and the plaintexts themselves between guards; and one decrypted case."""
import inspect

import numpy as np
import pytest
import torch

from tests.helpers import FENCE_FILLS, Fence
from tests.test_pc_dot_gpu import checker_engine, engine, message, params_of, run, same, words
from tests.test_pc_matmul_gpu import chunk, edge_plain, layer_of, pool_of

ENTRIES = ("pc_dot_native", "pc_matmul_native", "pc_matmul_batch_native", "pc_matmul_batch_planes_call")


def primes_of(eng, level):
    return [int(eng.ctx.q[i]) for i in eng.ntt.p.destination_arrays[level][0]]


def edge_words(eng, level, seed=5):
    """A "mult" plaintext whose rows start 0, 1, q - 1, q, 2q - 1 and go on with random lazy words below 2q (also in the last
    columns: the far end of the hi plane)."""
    like = eng.encode_plain(message(eng, 1), level)
    rng = np.random.default_rng(seed)
    rows = []
    for q in primes_of(eng, level):
        w = rng.integers(0, 2 * q, size=eng.ctx.N, dtype=np.int64)
        w[:5] = [0, 1, q - 1, q, 2 * q - 1]
        w[-5:] = [2 * q - 1, q, q - 1, 1, 0]
        rows.append(w)
    return like._replace(data=[torch.from_numpy(np.stack(rows)).to(like.data[0].device)])


def compact_layer(eng, W):
    done = {}
    return [[None if pt is None else done.setdefault(id(pt), eng.compact_plain(pt)) for pt in row] for row in W]


def count_calls(eng, monkeypatch):
    """every call of the four product entries of the backend, in order, as (entry, nt or None)"""
    calls = []
    for name in ENTRIES:
        real = getattr(eng.backend, name)
        at = 4 if "batch" in name else None                   # (the batched entries: nt)
        monkeypatch.setattr(eng.backend, name,
                            lambda *a, _r=real, _n=name, _at=at, **k: (calls.append((_n, None if _at is None else a[_at])), _r(*a, **k))[1],
                            raising=False)
    return calls


def guarded(words_, device, guard=4096):
    buf = torch.full((words_ + 2 * guard,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=device)
    return buf, buf[guard:guard + words_]


def guards_intact(buf, words_, guard=4096):
    return bool((buf[:guard] == 0x5A5A5A5A5A5A5A5A).all()) and bool((buf[guard + words_:] == 0x5A5A5A5A5A5A5A5A).all())


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["logN13", "logN17"])
def test_packer_and_unpacker_equal_the_host_implementation(name):
    """Bitwise, on 0, 1, q - 1, q, 2q - 1 and random lazy words, at level 0 and the last legal one; logN 17 is the largest N: the
    farthest hi plane.  The destination lies between guards."""
    eng = engine(name)
    N = eng.ctx.N
    for level in (0, eng.num_levels - 2):
        pt = edge_words(eng, level)
        q = primes_of(eng, level)
        c = eng._consts(0, level, False)
        n = eng.backend.plain_planes_words(len(q), N, c)
        assert n == eng.plain_planes_offsets(q, N)[-1]
        buf, body = guarded(n, pt.data[0].device)
        eng.backend.plain_planes(pt.data[0], body, c)
        want = eng._planes_host(pt.data[0].cpu(), q)
        assert torch.equal(body.cpu(), want) and guards_intact(buf, n), (name, level)
        assert torch.equal(eng._planes_host(pt.data[0], q).cpu(), want)                      # the torch words on the device
        comp = eng.compact_plain(pt)
        assert comp.data[0].is_cuda and torch.equal(comp.data[0].cpu(), want)
        buf, body = guarded(len(q) * N, pt.data[0].device)
        eng.backend.plain_unplanes(comp.data[0], body.view(len(q), N), c)
        qcol = torch.tensor(q, dtype=torch.int64).view(-1, 1)
        assert torch.equal(body.view(len(q), N).cpu(), pt.data[0].cpu() % qcol) and guards_intact(buf, len(q) * N), (name, level)
        assert torch.equal(eng._unplanes_host(want, q, N), pt.data[0].cpu() % qcol)
        assert torch.equal(eng.expand_plain(comp).data[0].cpu(), pt.data[0].cpu() % qcol)
        # moved and back: the same bytes
        assert torch.equal(eng.cuda(eng.cpu(comp)).data[0], comp.data[0])


@pytest.mark.gpu
@pytest.mark.parametrize("last", [False, True])
@pytest.mark.parametrize("shape", ["1x1", "3x2", "5x5", "CI+1x3"])
def test_the_four_ops_equal_the_raw_native_calls_and_the_composition(shape, last, monkeypatch):
    """logN 13, level 0 and the last legal one (fewer rows: another class mix).  GO = 1, 2 and 4 + 1, a second chunk's read - add -
    write, a None hole, an all-None column, a partly-None bias and no bias; B = 1, 2, 3 tokens: nt = 1, the pair tile, pair +
    single.  Compact = raw native = the generic composition, word for word; the compact calls reach lf_pc_matmul_batch_planes and
    nothing else, the raw ones go where they always went."""
    eng = engine("logN13")
    level = eng.num_levels - 2 if last else 0
    from liberate_fhe_amd.fhe.backend import SMALL_PRIME_LIMIT
    mix = [sorted(q < SMALL_PRIME_LIMIT for q in primes_of(eng, lvl)) for lvl in (0, eng.num_levels - 2)]
    assert mix[0] != mix[1] and all(True in m and False in m for m in mix)               # both classes at both levels, another mix
    k_in, k_out = {"1x1": (1, 1), "3x2": (3, 2), "5x5": (5, 5), "CI+1x3": (chunk() + 1, 3)}[shape]
    W, cts, bias = layer_of(pool_of(eng, level, 50 + level), k_in, k_out)
    K = compact_layer(eng, W)
    X = [[cts[(i + t) % k_in] for i in range(k_in)] for t in range(3)]
    calls = count_calls(eng, monkeypatch)
    P = "pc_matmul_batch_planes_call"
    for b in (None, bias):
        gen = [run(eng, lambda: eng.pc_matmul(W, tok, b), False) for tok in X]                # the composition, per token
        assert calls == []
        raw = eng.pc_matmul(W, X[0], b)
        assert calls == [("pc_matmul_native", None)]
        calls.clear()
        got = eng.pc_matmul(K, X[0], b)
        assert calls == [(P, 1)]
        calls.clear()
        assert len(got) == k_out and all(same(g, r) and same(g, w) for g, r, w in zip(got, raw, gen[0])), (shape, level)
        for B, raw_calls, planes_calls in ((1, [("pc_matmul_native", None)], [(P, 1)]), (2, [("pc_matmul_batch_native", 2)], [(P, 2)]),
                                           (3, [("pc_matmul_batch_native", 2), ("pc_matmul_native", None)], [(P, 2), (P, 1)])):
            raw = eng.pc_matmul_batch(W, X[:B], b)
            assert calls == raw_calls
            calls.clear()
            got = eng.pc_matmul_batch(K, X[:B], b)
            assert calls == planes_calls
            calls.clear()
            assert len(got) == B and all(len(g) == k_out for g in got)
            for t in range(B):
                assert all(same(g, r) and same(g, w) for g, r, w in zip(got[t], raw[t], gen[t])), (shape, level, B, t)
    pairs = [(pt, ct) for pt, ct in zip(W[0], cts) if pt is not None]
    kpairs = [(pt, ct) for pt, ct in zip(K[0], cts) if pt is not None]
    for b in (None, next(x for x in bias if x is not None)):
        raw = eng.pc_dot(pairs, b)
        assert calls == [("pc_dot_native", None)]
        calls.clear()
        got = eng.pc_dot(kpairs, b)
        assert calls == [(P, 1)]
        calls.clear()
        assert same(got, raw) and same(got, run(eng, lambda: eng.pc_dot(pairs, b), False))
    got = eng.pc_mult(kpairs[0][0], kpairs[0][1])
    assert calls == [(P, 1)]
    calls.clear()
    assert same(got, eng.pc_mult(*pairs[0])) and calls == []
    # and on expand_plain of each compact plaintext: the same words
    E = [[None if pt is None else eng.expand_plain(pt) for pt in row] for row in K]
    assert all(same(g, w) for g, w in zip(eng.pc_matmul(E, X[1], bias), gen[1]))


_CHECKER = {}


def checker_dot(level, which, k_in):
    """pc_dot of k_in times (the edge plaintext, the ciphertext of 2q - 1 everywhere) on the checker engine, computed once"""
    from tests.test_cc_dot_gpu import edge_ciphertexts
    key = (level, which, k_in)
    if key not in _CHECKER:
        if "engine" not in _CHECKER:
            _CHECKER["engine"] = checker_engine()
        cpu = _CHECKER["engine"]
        value = (lambda q: q - 1) if which == "q-1" else (lambda q: 2 * q - 1)
        _CHECKER[key] = words(cpu.pc_dot([(edge_plain(cpu, level, value), edge_ciphertexts(cpu, level)["top"])] * k_in))
    return _CHECKER[key]


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["q-1", "2q-1"])
def test_worst_case_words(which):
    """Every ciphertext word 2q - 1, every plaintext word q - 1 resp. 2q - 1; k_in = CI (a full chunk) and 2 CI (the word read back
    on top of one), k_out = 4, B = 2; level 0 and the last legal one.  The compact call against the checker engine on the raw
    plaintexts: every entry of the layer is the same object, so every output of every token is one pc_dot of the checker."""
    from tests.test_cc_dot_gpu import edge_ciphertexts
    from liberate_fhe_amd.fhe.backend import SMALL_PRIME_LIMIT
    CI = chunk()
    gpu = engine("logN13")
    q0 = primes_of(gpu, 0)
    assert any(q < SMALL_PRIME_LIMIT for q in q0) and any(q >= SMALL_PRIME_LIMIT for q in q0)
    value = (lambda q: q - 1) if which == "q-1" else (lambda q: 2 * q - 1)
    for level in (0, gpu.num_levels - 2):
        top = edge_ciphertexts(gpu, level)["top"]
        kpt = gpu.compact_plain(edge_plain(gpu, level, value))
        for k_in in (CI, 2 * CI):
            assert gpu._pc_planes_native(level) is not None
            got = gpu.pc_matmul_batch([[kpt] * k_in] * 4, [[top] * k_in] * 2)
            want = checker_dot(level, which, k_in)
            assert len(got) == 2 and all(len(tok) == 4 for tok in got)
            assert all(torch.equal(words(o)[c], want[c]) for tok in got for o in tok for c in range(2)), (level, k_in)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["silver", "logN17"])
def test_large_rings(name, monkeypatch):
    """2 x 2, B = 2, with a bias, at level 0: compact = raw native, one call of the compact entry."""
    eng = engine(name)
    W, cts, bias = layer_of(pool_of(eng, 0, 31), 2, 2)
    K = compact_layer(eng, W)
    X = [cts, cts[::-1]]
    calls = count_calls(eng, monkeypatch)
    raw = eng.pc_matmul_batch(W, X, bias)
    assert calls == [("pc_matmul_batch_native", 2)]
    calls.clear()
    got = eng.pc_matmul_batch(K, X, bias)
    assert calls == [("pc_matmul_batch_planes_call", 2)]
    assert all(same(g, r) for gs, rs in zip(got, raw) for g, r in zip(gs, rs))
    assert K[0][0].data[0].numel() < W[0][0].data[0].numel()


@pytest.mark.gpu
def test_fenced():
    """A fresh engine with guards around every workspace and output and a hostile fill (every bit set) in the workspace; the compact
    plaintexts themselves between guards.  (CI + 1) x 3 over three tokens (a pair tile, a single, two chunks) with a partly-None
    bias: no guard is touched, every output is written, the plaintexts are unchanged, the words are the unfenced engine's."""
    from liberate_fhe_amd.fhe import ckks_engine
    plain = engine("logN13")
    eng = ckks_engine(devices=["cuda:0"], **params_of("logN13"))
    fence = Fence(eng, FENCE_FILLS["ones"])
    name = "pc_matmul_batch_planes_call"
    real = getattr(eng.backend, name)
    setattr(eng.backend, name, fence._fenced_entry(name, real, inspect.signature(real)))
    k_in, k_out = chunk() + 1, 3
    W, cts, bias = layer_of(pool_of(plain, 0, 77), k_in, k_out)
    X = [[cts[(i + t) % k_in] for i in range(k_in)] for t in range(3)]
    want = plain.pc_matmul_batch(W, X, bias)
    done, fenced = {}, []
    for row in W:
        for pt in row:
            if pt is not None and id(pt) not in done:
                k = plain.compact_plain(pt)
                f = fence.alloc(("compact plaintext", len(fenced)), tuple(k.data[0].shape), None, k.data[0].device)
                f.body.copy_(k.data[0])
                fenced.append((f, k.data[0].clone()))
                done[id(pt)] = k._replace(data=[f.body])
    K = [[None if pt is None else done[id(pt)] for pt in row] for row in W]
    for _ in range(2):                       # (the second call finds the workspace the first one left, refilled)
        fence.refill()
        fence.calls.clear()
        fence.never_written.clear()
        got = eng.pc_matmul_batch(K, X, bias)
        assert fence.calls == [name, name] and fence.never_written == []
        fence.check([f for f, _ in fenced])
        assert all(torch.equal(f.body, kept) for f, kept in fenced)
        assert all(same(g, w) for gs, ws in zip(got, want) for g, w in zip(gs, ws))
    assert any(k[0] == "pc_matmul_batch_ws" for k in fence.scratch)


@pytest.mark.gpu
def test_real_keys_decrypt_within_twice_the_loop_on_silver():
    """silver, real keys, a 4 x 3 layer of random real vectors with |.| <= 1 encoded compact, a bias per output: every output decodes
    to exactly what pc_matmul on the raw plaintexts of the same encodings decodes to, and its maximum error against float64
    W @ x + b is at most 2 x that of the mc_mult / cc_add / mc_add loop on the same inputs in the same run (the bound
    tests/test_pc_matmul_gpu.py holds pc_matmul to).  All errors are printed."""
    eng = engine("silver")
    sk = eng.create_secret_key()
    pk = eng.create_public_key(sk)
    rng = np.random.default_rng(14)
    n = eng.num_slots
    ws = [[rng.uniform(-1, 1, n) for _ in range(4)] for _ in range(3)]
    xs = [rng.uniform(-1, 1, n) for _ in range(4)]
    bs = [rng.uniform(-1, 1, n) for _ in range(3)]
    cts = [eng.encorypt(x, pk) for x in xs]
    W = [[eng.encode_plain(w, 0) for w in row] for row in ws]
    K = [[eng.compact_plain(pt) for pt in row] for row in W]
    bias = [eng.encode_plain(b, 1, "add") for b in bs]
    assert eng._pc_planes_native(0) is not None
    got = eng.pc_matmul(K, cts, bias)
    raw = eng.pc_matmul(W, cts, bias)
    for o in range(3):
        want = sum(w * x for w, x in zip(ws[o], xs)) + bs[o]
        dec = eng.decrode(got[o], sk)
        assert got[o].level == 1 and same(got[o], raw[o]) and np.array_equal(dec, eng.decrode(raw[o], sk))
        loop = None
        for w, ct in zip(ws[o], cts):
            p = eng.mc_mult(w, ct)
            loop = p if loop is None else eng.cc_add(loop, p)
        loop = eng.mc_add(bs[o], loop)
        e_mm = np.abs(dec.real - want).max()
        e_loop = np.abs(eng.decrode(loop, sk).real - want).max()
        print(f"silver, 4 x 3 + bias, level 0, output {o}: max abs error compact pc_matmul {e_mm:.3e}, mc_mult / cc_add / mc_add loop "
              f"{e_loop:.3e}, largest entry {np.abs(want).max():.2f}")
        assert e_mm <= 2 * e_loop and e_loop < 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("k_in", ["2", "CI+1"])
def test_every_tile_of_the_product_body_equals_the_pc_dots(k_in, monkeypatch):
    """The one product body through all its tiles, raw and compact: logN 13, level 0 (rows of both classes), k_out = 7 — output
    groups 4 + 2 + 1, under LF_TUNE_PC_MATMUL_TILE = 2 over four tokens 2 + 2 + 2 + 1 — over k_in = 2 and CI + 1 inputs (a second
    chunk: the read - add - write of S), with holes and a partly-None bias.  Four tokens as ONE native call (tiles 2 + 2; 4 under
    the knob's values 1 and 2) and three as one (2 + 1).  Every output has exactly the words of pc_dot over the row's non-None
    entries on the raw plaintexts, token by token."""
    from liberate_fhe_amd._native import lib
    from liberate_fhe_amd.fhe.backend import SMALL_PRIME_LIMIT
    eng = engine("logN13")
    q0 = primes_of(eng, 0)
    assert any(q < SMALL_PRIME_LIMIT for q in q0) and any(q >= SMALL_PRIME_LIMIT for q in q0)
    k_in, k_out = {"2": 2, "CI+1": chunk() + 1}[k_in], 7
    W, cts, bias = layer_of(pool_of(eng, 0, 61), k_in, k_out)
    assert any(pt is None for row in W for pt in row) and any(b is None for b in bias) and any(b is not None for b in bias)
    K = compact_layer(eng, W)
    X = [[cts[(i + t) % k_in] for i in range(k_in)] for t in range(4)]
    want = [[eng.pc_dot([(pt, ct) for pt, ct in zip(row, tok) if pt is not None], b) for row, b in zip(W, bias)] for tok in X]
    d = eng._pc_planes_native(0)
    assert d is not None
    monkeypatch.setattr(eng, "pc_matmul_batch_sizes", (4, 2))            # (ONE native call of four tokens: what the tile knob acts on)
    calls = count_calls(eng, monkeypatch)
    try:
        for tile in (0, 1, 2):
            lib.lf_tune(6, tile)
            for M, entry, planes in ((W, "pc_matmul_batch_native", False), (K, "pc_matmul_batch_planes_call", True)):
                got = eng.pc_matmul_batch(M, X, bias)
                got3 = eng._pc_matmul_batch_native(M, X[:3], bias, 0, d, planes=planes)
                assert calls == [(entry, 4), (entry, 3)]
                calls.clear()
                for res in (got, got3):
                    assert all(len(tok) == k_out for tok in res)
                    assert all(same(g, w) for gs, ws in zip(res, want) for g, w in zip(gs, ws)), (tile, entry, len(res))
    finally:
        lib.lf_tune(6, 0)
