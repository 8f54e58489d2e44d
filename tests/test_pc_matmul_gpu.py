"""pc_matmul on the GPU: lf_pc_matmul (one native call: every ciphertext transformed once, pc_matmul_kernel<4 | 2 | 1> per chunk
of inputs and group of outputs, one inverse transform of all sums, the rescales, pc_bias_kernel) against the composition on the
GPU's generic path and against the list of native pc_dots, on worst-case words against the checker engine, under the tuning
knobs, with operands the native path refuses, past 64 outputs, and decrypted with real keys against the loop of mc_mults."""
import os

import numpy as np
import pytest
import torch

from liberate_fhe_amd.utils import synth
from tests.test_pc_dot_gpu import checker_engine, engine, lazy, message, run, same, words

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def chunk():
    from liberate_fhe_amd.fhe.backend import HipBackend
    return HipBackend.pc_matmul_chunk


def shapes_of(name):
    """(k_in, k_out): the smallest case; GO = 2; GO = 4; output groups 4 + 1 over two transform calls; groups 4 + 4 + 1; one input
    past a chunk (the read - add - write path, groups 2 + 1).  The large rings take the last two kinds only."""
    CI = chunk()
    return ((1, 1), (3, 2), (4, 4), (5, 5), (2, 9), (CI + 1, 3)) if name == "logN13" else ((5, 5), (CI + 1, 3))


def pool_of(eng, level, seed=50):
    """Three plaintexts, three ciphertexts (two of them lazy) of one level and two biases for the level above."""
    pts = [eng.encode_plain(message(eng, seed + i), level) for i in range(3)]
    cts = [synth.ciphertext(eng, seed + i, level) for i in range(3)]
    cts = [lazy(eng, cts[0]), cts[1], lazy(eng, cts[2])]
    return pts, cts, [eng.encode_plain(message(eng, seed + 7 + i), level + 1, "add") for i in range(2)]


def layer_of(pool, k_in, k_out):
    """(W, cts, bias) from the pool, objects repeating on both sides: a hole in every second row, column 1 all None (from three
    inputs on, and only inside one chunk: a longer layer has to cross it), every second bias None."""
    pts, cs, adds = pool
    cts = [cs[i % 3] for i in range(k_in)]
    W = [[pts[(o + 2 * i) % 3] for i in range(k_in)] for o in range(k_out)]
    for o in range(k_out):
        if 3 <= k_in <= chunk():
            W[o][1] = None
        if k_in >= 2 and o % 2:
            W[o][0 if k_in >= 3 else o // 2 % 2] = None
    return W, cts, [adds[o // 2 % 2] if o % 2 == 0 else None for o in range(k_out)]


def dots_of(eng, W, cts, bias):
    return [eng.pc_dot([(pt, ct) for pt, ct in zip(row, cts) if pt is not None], b) for row, b in zip(W, bias)]


def count_native_calls(eng, monkeypatch):
    """(calls of lf_pc_matmul as (k_in, k_out), calls of lf_pc_dot as k)"""
    mm, dot = [], []
    real_mm, real_dot = eng.backend.pc_matmul_native, eng.backend.pc_dot_native
    monkeypatch.setattr(eng.backend, "pc_matmul_native", lambda *a, **k: (mm.append((a[4], a[5])), real_mm(*a, **k))[1], raising=False)
    monkeypatch.setattr(eng.backend, "pc_dot_native", lambda *a, **k: (dot.append(a[4]), real_dot(*a, **k))[1], raising=False)
    return mm, dot


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["logN13", "silver", "logN17"])
def test_native_call_equals_the_composition(name, monkeypatch):
    """Levels 0, a middle one and the last legal one (a single surviving row), every shape of shapes_of, holes, an all-None column,
    repeated and lazy operands, a partly-None bias (without bias too on the small ring): exactly one lf_pc_matmul and no lf_pc_dot
    per pc_matmul; the words of the generic path and of the list of native pc_dots."""
    eng = engine(name)
    mm, dot = count_native_calls(eng, monkeypatch)
    L = eng.num_levels
    for level in sorted({0, (L - 1) // 2, L - 2}):
        pool = pool_of(eng, level, 50 + level)
        for k_in, k_out in shapes_of(name):
            W, cts, bias = layer_of(pool, k_in, k_out)
            for b in ((None, bias) if name == "logN13" else (bias,)):
                n = len(mm)
                nat = run(eng, lambda: eng.pc_matmul(W, cts, b), True)
                assert mm[n:] == [(k_in, k_out)] and dot == []                      # ONE native call
                gen = run(eng, lambda: eng.pc_matmul(W, cts, b), False)
                assert len(mm) == n + 1 and dot == []
                want = run(eng, lambda: dots_of(eng, W, cts, b or [None] * k_out), True)
                assert len(dot) == k_out and len(mm) == n + 1
                dot.clear()
                assert len(nat) == len(gen) == len(want) == k_out
                for o in range(k_out):
                    assert nat[o].level == level + 1 and not nat[o].ntt_state and not nat[o].include_special
                    assert same(nat[o], gen[o]) and same(nat[o], want[o]), (name, level, k_in, k_out, o, b is not None)


def edge_plain(eng, level, value):
    """A "mult" plaintext whose every word is value(q) (Montgomery form, built directly as a tensor)."""
    q = torch.tensor([int(eng.ctx.q[i]) for i in eng.ntt.p.destination_arrays[level][0]], dtype=torch.int64).view(-1, 1)
    like = eng.encode_plain(message(eng, 1), level)
    return like._replace(data=[value(q).expand(-1, eng.ctx.N).contiguous().to(like.data[0].device)])


@pytest.mark.gpu
def test_worst_case_words():
    """Every ciphertext word 2q - 1 on all rows, every plaintext word q - 1 in one run and 2q - 1 in another; k_in = CI (a full
    chunk: the fp64 accumulator at CI q / 2) and k_in = 2 CI (the word read back on top of a full chunk), k_out = 4; a ring with
    rows of both classes, at level 0 and at the last legal one.  Native call against the checker engine: every entry of the
    layer is the same object, so the four outputs are one pc_dot of the checker."""
    from tests.test_cc_dot_gpu import edge_ciphertexts
    CI = chunk()
    gpu, cpu = engine("logN13"), checker_engine()
    q0 = [int(gpu.ctx.q[i]) for i in gpu.ntt.p.destination_arrays[0][0]]
    assert any(q < 2 ** 41 for q in q0) and any(q >= 2 ** 41 for q in q0)             # fp64-class and integer-class rows
    for level in (0, gpu.num_levels - 2):
        for value in (lambda q: q - 1, lambda q: 2 * q - 1):
            for k_in in (CI, 2 * CI):
                res = []
                for eng in (gpu, cpu):
                    top, pt = edge_ciphertexts(eng, level)["top"], edge_plain(eng, level, value)
                    if eng is gpu:
                        assert eng._native_level(level + 1) is not None
                        res.append([words(o) for o in eng.pc_matmul([[pt] * k_in] * 4, [top] * k_in)])
                    else:
                        res.append([words(eng.pc_dot([(pt, top)] * k_in))] * 4)
                assert all(torch.equal(a[c], b[c]) for a, b in zip(*res) for c in range(2)), (level, k_in)


@pytest.mark.gpu
def test_gpu_equals_the_checker():
    """5 x 3 with bias at levels 0 and 2: pc_matmul's words against the checker engine's.  The polynomial encode returns is random
    (its rounding), so the checker's plaintexts are carried over."""
    gpu, cpu = engine("logN13"), checker_engine()
    for level in (0, 2):
        pts_c = [cpu.encode_plain(message(cpu, 30 + i), level) for i in range(3)]
        adds_c = [cpu.encode_plain(message(cpu, 40 + i), level + 1, "add") for i in range(2)]
        cts_c = [synth.ciphertext(cpu, 70 + level + i, level) for i in range(3)]
        up = lambda x: x._replace(data=[t.to("cuda:0") for t in x.data], hash=gpu.hash)
        cts_g = [synth.ciphertext(gpu, 70 + level + i, level) for i in range(3)]
        assert all(torch.equal(a.cpu(), b) for g, c in zip(cts_g, cts_c) for x, y in zip(g.data, c.data) for a, b in zip(x, y))
        Wc, cc, bc = layer_of((pts_c, cts_c, adds_c), 5, 3)
        Wg, cg, bg = layer_of(([up(p) for p in pts_c], cts_g, [up(a) for a in adds_c]), 5, 3)
        got, want = gpu.pc_matmul(Wg, cg, bg), cpu.pc_matmul(Wc, cc, bc)
        assert len(got) == len(want) == 3
        assert all(torch.equal(a, b) for g, w in zip(got, want) for a, b in zip(words(g), words(w))), level


def knob_walk():
    """The body of test_tuning_knobs_change_no_word (the walk of tests/test_pc_dot_gpu.py); it flips process-wide knobs, so it runs
    in a process of its own."""
    from liberate_fhe_amd._native import lib
    outs = []
    for name in ("logN13", "silver"):
        eng = engine(name)
        W, cts, bias = layer_of(pool_of(eng, 0, 12), 5, 5)
        res = []
        for planes, more in ((1, 3), (0, 3), (1, 0), (1, 1), (0, 0)):
            lib.lf_tune(3, planes), lib.lf_tune(5, more)
            for native in (True, False):
                res.append(run(eng, lambda: eng.pc_matmul(W, cts, bias), native))
        outs.append(res)
    assert all(len(res) == 10 and all(same(a, b) for o in res[1:] for a, b in zip(o, res[0])) for res in outs)


@pytest.mark.gpu
def test_tuning_knobs_change_no_word():
    """LF_TUNE_DIGIT_PLANES and LF_TUNE_MORE_PLANES (bit 1: the stack planes), on the native call and on the composition, in a
    fresh child process (tests/test_cc_dot_gpu.py says why)."""
    import subprocess
    import sys
    code = f"import sys; sys.path.insert(0, {ROOT!r}); from tests.test_pc_matmul_gpu import knob_walk; knob_walk()"
    flags = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable, *flags, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]


@pytest.mark.gpu
def test_operands_the_native_path_refuses_take_the_composition(monkeypatch):
    """A non-contiguous ciphertext component and one at an odd word offset (contiguous, not 16-byte aligned), in a column every
    output uses: no native call of either entry, the same words.  A plaintext after cpu() / cuda() is a fresh contiguous, aligned
    device tensor, which the native path takes as pc_dot's does: the same words again."""
    eng = engine("logN13")
    mm, dot = count_native_calls(eng, monkeypatch)
    pts, cts, adds = pool_of(eng, 0, 20)
    W = [[pts[0], pts[1], pts[2]], [pts[1], None, pts[0]], [pts[2], pts[2], None]]
    bias = [adds[0], None, adds[1]]
    want = eng.pc_matmul(W, cts, bias)
    assert mm == [(3, 3)] and dot == []
    N = eng.ctx.N

    def strided(t):
        wide = torch.zeros((t.size(0), 2 * N), dtype=torch.int64, device=t.device)
        wide[:, ::2] = t
        return wide[:, ::2]

    def odd(t):
        flat = torch.zeros(t.numel() + 1, dtype=torch.int64, device=t.device)
        flat[1:] = t.reshape(-1)
        return flat[1:].view(t.shape)

    s = cts[0]._replace(data=([strided(cts[0].data[0][0])], [cts[0].data[1][0]]))
    assert not s.data[0][0].is_contiguous()
    o = cts[0]._replace(data=([cts[0].data[0][0]], [odd(cts[0].data[1][0])]))
    assert o.data[1][0].is_contiguous() and o.data[1][0].data_ptr() % 16 == 8
    so = cts[0]._replace(data=(s.data[0], o.data[1]))
    for c in ([s, cts[1], cts[2]], [o, cts[1], cts[2]], [so, cts[1], cts[2]]):
        got = eng.pc_matmul(W, c, bias)
        assert mm == [(3, 3)] and dot == [] and all(same(g, w) for g, w in zip(got, want))
    back = eng.cuda(eng.cpu(pts[1]))
    assert back.data[0].data_ptr() != pts[1].data[0].data_ptr()
    got = eng.pc_matmul([[back if p is pts[1] else p for p in row] for row in W], cts, bias)
    assert all(same(g, w) for g, w in zip(got, want))


@pytest.mark.gpu
def test_more_outputs_than_one_call_takes(monkeypatch):
    """k_out = 65 over one ciphertext, one shared plaintext object and a second one in the last row: two native calls (64 outputs
    and 1), the words of the loop of pc_dots."""
    eng = engine("logN13")
    mm, dot = count_native_calls(eng, monkeypatch)
    pts, cts, adds = pool_of(eng, 0, 33)
    W = [[pts[0]]] * 64 + [[pts[1]]]
    got = eng.pc_matmul(W, [cts[0]])
    assert mm == [(1, 64), (1, 1)] and dot == []
    shared, last = eng.pc_dot([(pts[0], cts[0])]), eng.pc_dot([(pts[1], cts[0])])
    assert len(got) == 65 and all(same(g, shared) for g in got[:64]) and same(got[64], last) and not same(shared, last)


@pytest.mark.gpu
def test_real_keys_decrypt_within_twice_the_loop_on_silver():
    """silver, real keys, a 4 x 3 layer of random real vectors with |.| <= 1 and a bias per output: every output decodes to
    exactly what the corresponding pc_dot decodes to (the same words), and its maximum error against float64 W @ x + b is at most
    2 x that of the mc_mult / cc_add / mc_add loop on the same inputs in the same run (the bound tests/test_pc_dot_gpu.py holds
    pc_dot to).  All errors are printed."""
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
    bias = [eng.encode_plain(b, 1, "add") for b in bs]
    assert eng._native_level(1) is not None
    got = eng.pc_matmul(W, cts, bias)
    for o in range(3):
        want = sum(w * x for w, x in zip(ws[o], xs)) + bs[o]
        dec = eng.decrode(got[o], sk)
        assert got[o].level == 1 and np.array_equal(dec, eng.decrode(eng.pc_dot(list(zip(W[o], cts)), bias[o]), sk))
        loop = None
        for w, ct in zip(ws[o], cts):
            p = eng.mc_mult(w, ct)
            loop = p if loop is None else eng.cc_add(loop, p)
        loop = eng.mc_add(bs[o], loop)
        e_mm = np.abs(dec.real - want).max()
        e_loop = np.abs(eng.decrode(loop, sk).real - want).max()
        print(f"silver, 4 x 3 + bias, level 0, output {o}: max abs error pc_matmul {e_mm:.3e}, mc_mult / cc_add / mc_add loop {e_loop:.3e}, "
              f"largest entry {np.abs(want).max():.2f}")
        assert e_mm <= 2 * e_loop and e_loop < 1e-5
