"""pc_matmul_batch on the GPU: lf_pc_matmul_batch (one native call per group of token vectors: pc_matmulb_kernel<GO, GT> reads
every plaintext word once per tile of tokens) against the loop of pc_matmul on the GPU and the generic composition, word for word; on
worst-case words against the checker engine; under the tuning knobs (every tile of the launch table); with tokens the native
path refuses; and decrypted with real keys against the loop of mc_mults."""
import os

import numpy as np
import pytest
import torch

from liberate_fhe_amd.utils import synth
from tests.test_pc_dot_gpu import checker_engine, engine, message, run, same, words
from tests.test_pc_dot_gpu import lazy  # noqa: F401  (pool_of's lazy ciphertexts)
from tests.test_pc_matmul_gpu import chunk, edge_plain, layer_of, pool_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tokens_of(eng, pool, k_in, B, level, seed=90):
    """B token vectors of k_in ciphertexts over five objects (the pool's three, two of them lazy, and two more): token t holds
    object (2 i + t) % 5 at input i — objects repeat inside a token and across tokens, tokens t and t + 5 are the same vector."""
    five = list(pool[1]) + [synth.ciphertext(eng, seed + i, level) for i in range(2)]
    return [[five[(2 * i + t) % 5] for i in range(k_in)] for t in range(B)]


def count_native_calls(eng, monkeypatch):
    """(calls of lf_pc_matmul_batch as (nt, k_in, k_out) and the input pointers of each, of lf_pc_matmul as (k_in, k_out), of
    lf_pc_dot as k)"""
    mmb, ptrs, mm, dot = [], [], [], []
    be = eng.backend
    real_b, real_mm, real_dot = be.pc_matmul_batch_native, be.pc_matmul_native, be.pc_dot_native
    monkeypatch.setattr(be, "pc_matmul_batch_native",
                        lambda *a, **k: (mmb.append((a[4], a[5], a[6])), ptrs.append(list(a[0])), real_b(*a, **k))[2], raising=False)
    monkeypatch.setattr(be, "pc_matmul_native", lambda *a, **k: (mm.append((a[4], a[5])), real_mm(*a, **k))[1], raising=False)
    monkeypatch.setattr(be, "pc_dot_native", lambda *a, **k: (dot.append(a[4]), real_dot(*a, **k))[1], raising=False)
    return mmb, ptrs, mm, dot


def groups_of(eng, B):
    """The native calls of B ready tokens (the engine's group sizes, largest first) and how many tokens they leave to pc_matmul."""
    g = []
    for k in eng.pc_matmul_batch_sizes:
        g += [k] * ((B - sum(g)) // k)
    return g, B - sum(g)


def batch_against_the_loop(eng, monkeypatch, name, level, shapes, Bs, biases):
    mmb, _, mm, dot = count_native_calls(eng, monkeypatch)
    pool = pool_of(eng, level, 50 + level)
    for k_in, k_out in shapes:
        W, _, bias = layer_of(pool, k_in, k_out)
        X = tokens_of(eng, pool, k_in, max(Bs), level)
        assert X[0][0] is X[1][2 % k_in] or k_in < 3                       # one object in two tokens
        for b in biases(bias):
            # the references once, over all tokens: the loop of native pc_matmuls and the generic composition
            loop = run(eng, lambda: [eng.pc_matmul(W, tok, b) for tok in X], True)
            assert mm == [(k_in, k_out)] * len(X) and mmb == [] and dot == []
            mm.clear()
            gen = run(eng, lambda: eng.pc_matmul_batch(W, X, b), False)
            assert mm == [] and mmb == [] and dot == []
            for B in Bs:
                nat = run(eng, lambda: eng.pc_matmul_batch(W, X[:B], b), True)
                g, left = groups_of(eng, B)
                assert mmb == [(nt, k_in, k_out) for nt in g] and mm == [(k_in, k_out)] * left and dot == [], (name, B, mmb, mm, dot)
                mmb.clear(), mm.clear()
                assert len(nat) == B and all(len(tok) == k_out for tok in nat)
                for t in range(B):
                    for o in range(k_out):
                        assert nat[t][o].level == level + 1 and not nat[t][o].ntt_state and not nat[t][o].include_special
                        assert same(nat[t][o], loop[t][o]) and same(nat[t][o], gen[t][o]), (name, level, k_in, k_out, B, t, o, b is not None)


@pytest.mark.gpu
@pytest.mark.parametrize("sizes", [(4, 2), (2,)])
@pytest.mark.parametrize("level", ["0", "L-2"])
def test_native_call_equals_the_loop_and_the_composition(level, sizes, monkeypatch):
    """logN13, level 0 and the last legal one; B = 2, 3, 4, 7 — with every size the backend offers groups 2, 2 + 1 left over, 4,
    4 + 2 + 1 left over (the 2 + 2 tiles of a 4-token call), with the engine's own sizes 2, 2 + 1, 2 + 2, 2 + 2 + 2 + 1; shapes that take
    GO = 1, 2, 4, groups 4 + 1 and the read - add - write path; holes, an all-None column, lazy and repeated ciphertexts, a
    partly-None bias and no bias: exactly the expected lf_pc_matmul_batch calls, lf_pc_matmul for a left-over token only, the
    words of the loop of native pc_matmuls and of the generic composition."""
    eng = engine("logN13")
    assert type(eng).pc_matmul_batch_sizes == (2,) and eng.backend.pc_matmul_batch_sizes == (4, 2)
    monkeypatch.setattr(eng, "pc_matmul_batch_sizes", sizes)
    lvl = 0 if level == "0" else eng.num_levels - 2
    batch_against_the_loop(eng, monkeypatch, "logN13", lvl, ((1, 1), (3, 2), (5, 5), (chunk() + 1, 3)), (2, 3, 4, 7), lambda bias: (None, bias))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["silver", "logN17"])
def test_native_call_equals_the_loop_on_the_large_rings(name, monkeypatch):
    """B = 4 as ONE native call of four tokens, 5 x 5 with a partly-None bias at level 0."""
    monkeypatch.setattr(engine(name), "pc_matmul_batch_sizes", (4, 2))
    batch_against_the_loop(engine(name), monkeypatch, name, 0, ((5, 5),), (4,), lambda bias: (bias,))


@pytest.mark.gpu
def test_worst_case_words(monkeypatch):
    """Every ciphertext word 2q - 1 on all rows, every plaintext word q - 1 in one run and 2q - 1 in another; k_in = CI (a full
    chunk: every fp64 accumulator at CI q / 2) and 2 CI (the word read back on top of a full chunk), k_out = 4, B = 4 as one
    native call of four tokens (all accumulators of a thread at the bound); a ring with rows of both classes, level 0 and the last legal one.
    Every token and every entry of the layer is the same object, so all sixteen outputs are ONE pc_dot of the checker."""
    from tests.test_cc_dot_gpu import edge_ciphertexts
    CI = chunk()
    gpu, cpu = engine("logN13"), checker_engine()
    monkeypatch.setattr(gpu, "pc_matmul_batch_sizes", (4, 2))
    q0 = [int(gpu.ctx.q[i]) for i in gpu.ntt.p.destination_arrays[0][0]]
    assert any(q < 2 ** 41 for q in q0) and any(q >= 2 ** 41 for q in q0)             # fp64-class and integer-class rows
    for level in (0, gpu.num_levels - 2):
        for value in (lambda q: q - 1, lambda q: 2 * q - 1):
            for k_in in (CI, 2 * CI):
                top, pt = edge_ciphertexts(gpu, level)["top"], edge_plain(gpu, level, value)
                assert gpu._native_level(level + 1) is not None
                got = gpu.pc_matmul_batch([[pt] * k_in] * 4, [[top] * k_in] * 4)
                top, pt = edge_ciphertexts(cpu, level)["top"], edge_plain(cpu, level, value)
                want = words(cpu.pc_dot([(pt, top)] * k_in))
                assert len(got) == 4 and all(len(tok) == 4 for tok in got)
                assert all(torch.equal(a, b) for tok in got for o in tok for a, b in zip(words(o), want)), (level, k_in)


def knob_walk():
    """The body of test_tuning_knobs_change_no_word; it flips process-wide knobs, so it runs in a process of its own.  Knob 6
    (LF_TUNE_PC_MATMUL_TILE) walks the three ways a call of four tokens is covered: every tile of the launch table runs."""
    from liberate_fhe_amd._native import lib
    outs = []
    for name in ("logN13", "silver"):
        eng = engine(name)
        eng.pc_matmul_batch_sizes = (4, 2)                       # (ONE native call of four tokens: what the tile knob acts on)
        pool = pool_of(eng, 0, 12)
        W, _, bias = layer_of(pool, 5, 5)
        X = tokens_of(eng, pool, 5, 4, 0)
        res = [run(eng, lambda: eng.pc_matmul_batch(W, X, bias), False)]
        for planes, more, tile in ((1, 3, 0), (0, 3, 0), (1, 0, 0), (1, 1, 0), (0, 0, 0), (1, 3, 1), (1, 3, 2), (0, 0, 1), (0, 0, 2)):
            lib.lf_tune(3, planes), lib.lf_tune(5, more), lib.lf_tune(6, tile)
            res.append(run(eng, lambda: eng.pc_matmul_batch(W, X, bias), True))
        lib.lf_tune(3, 1), lib.lf_tune(5, 3), lib.lf_tune(6, 0)
        outs.append(res)
    assert all(len(res) == 10 and all(same(a, b) for r in res[1:] for x, y in zip(r, res[0]) for a, b in zip(x, y)) for res in outs)


@pytest.mark.gpu
def test_tuning_knobs_change_no_word():
    """LF_TUNE_DIGIT_PLANES, LF_TUNE_MORE_PLANES (bit 1: the stack planes) and LF_TUNE_PC_MATMUL_TILE on the native call against the
    composition, in a fresh child process (tests/test_cc_dot_gpu.py says why)."""
    import subprocess
    import sys
    code = f"import sys; sys.path.insert(0, {ROOT!r}); from tests.test_pc_matmul_batch_gpu import knob_walk; knob_walk()"
    flags = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable, *flags, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]


@pytest.mark.gpu
def test_a_token_the_native_path_refuses_keeps_its_place(monkeypatch):
    """Token 1 of 3 with a non-contiguous component, with one at an odd word offset (contiguous, not 16-byte aligned), with both:
    the same words; tokens 0 and 2 are ONE native call of two tokens that holds none of token 1's pointers, and token 1 takes
    pc_matmul (whose own native call refuses it too: no lf_pc_matmul, no lf_pc_dot)."""
    eng = engine("logN13")
    mmb, ptrs, mm, dot = count_native_calls(eng, monkeypatch)
    pool = pool_of(eng, 0, 20)
    pts, cts, adds = pool
    W = [[pts[0], pts[1], pts[2]], [pts[1], None, pts[0]], [pts[2], pts[2], None]]
    bias = [adds[0], None, adds[1]]
    X = tokens_of(eng, pool, 3, 3, 0)
    want = eng.pc_matmul_batch(W, X, bias)
    assert mmb == [(2, 3, 3)] and mm == [(3, 3)] and dot == []
    mmb.clear(), mm.clear(), ptrs.clear()
    N = eng.ctx.N

    def strided(t):
        wide = torch.zeros((t.size(0), 2 * N), dtype=torch.int64, device=t.device)
        wide[:, ::2] = t
        return wide[:, ::2]

    def odd(t):
        flat = torch.zeros(t.numel() + 1, dtype=torch.int64, device=t.device)
        flat[1:] = t.reshape(-1)
        return flat[1:].view(t.shape)

    c = X[1][0]
    s = c._replace(data=([strided(c.data[0][0])], [c.data[1][0].clone()]))
    o = c._replace(data=([c.data[0][0].clone()], [odd(c.data[1][0])]))
    so = c._replace(data=(s.data[0], o.data[1]))
    assert not s.data[0][0].is_contiguous() and o.data[1][0].is_contiguous() and o.data[1][0].data_ptr() % 16 == 8
    for bad in (s, o, so):
        tok = [bad] + X[1][1:]
        got = eng.pc_matmul_batch(W, [X[0], tok, X[2]], bias)
        assert mmb == [(2, 3, 3)] and mm == [] and dot == []
        assert ptrs[0] == [ct.data[comp][0].data_ptr() for t in (0, 2) for ct in X[t] for comp in range(2)]
        assert not {bad.data[0][0].data_ptr(), bad.data[1][0].data_ptr()} & set(ptrs[0])
        mmb.clear(), ptrs.clear()
        assert all(same(a, w) for g, ws in zip(got, want) for a, w in zip(g, ws))


@pytest.mark.gpu
def test_real_keys_decrypt_within_twice_the_loop_on_silver(monkeypatch):
    """silver, real keys, B = 2 tokens through a 4 x 3 layer of random real vectors with |.| <= 1 and a bias per output: ONE native
    call; every output decodes to exactly what pc_matmul's output decodes to, and its maximum error against float64 W @ x + b is
    at most 2 x that of the mc_mult / cc_add / mc_add loop on the same inputs in the same run (the bound tests/test_pc_matmul_gpu.py
    holds pc_matmul to).  All errors are printed."""
    eng = engine("silver")
    mmb, _, mm, dot = count_native_calls(eng, monkeypatch)
    sk = eng.create_secret_key()
    pk = eng.create_public_key(sk)
    rng = np.random.default_rng(15)
    n = eng.num_slots
    ws = [[rng.uniform(-1, 1, n) for _ in range(4)] for _ in range(3)]
    xs = [[rng.uniform(-1, 1, n) for _ in range(4)] for _ in range(2)]
    bs = [rng.uniform(-1, 1, n) for _ in range(3)]
    X = [[eng.encorypt(x, pk) for x in tok] for tok in xs]
    W = [[eng.encode_plain(w, 0) for w in row] for row in ws]
    bias = [eng.encode_plain(b, 1, "add") for b in bs]
    assert eng._native_level(1) is not None
    got = eng.pc_matmul_batch(W, X, bias)
    assert mmb == [(2, 4, 3)] and mm == [] and dot == []
    for t in range(2):
        single = eng.pc_matmul(W, X[t], bias)
        for o in range(3):
            want = sum(w * x for w, x in zip(ws[o], xs[t])) + bs[o]
            dec = eng.decrode(got[t][o], sk)
            assert got[t][o].level == 1 and np.array_equal(dec, eng.decrode(single[o], sk))
            loop = None
            for w, ct in zip(ws[o], X[t]):
                p = eng.mc_mult(w, ct)
                loop = p if loop is None else eng.cc_add(loop, p)
            loop = eng.mc_add(bs[o], loop)
            e_mm = np.abs(dec.real - want).max()
            e_loop = np.abs(eng.decrode(loop, sk).real - want).max()
            print(f"silver, 4 x 3 + bias, level 0, token {t}, output {o}: max abs error pc_matmul_batch {e_mm:.3e}, "
                  f"mc_mult / cc_add / mc_add loop {e_loop:.3e}, largest entry {np.abs(want).max():.2f}")
            assert e_mm <= 2 * e_loop and e_loop < 1e-5
