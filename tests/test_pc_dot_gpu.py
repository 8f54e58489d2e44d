"""pc_dot on the GPU: lf_pc_dot (one native call: the forward transforms of a chunk of ciphertexts, pc_dot_kernel<4 | 2 | 1>, one
inverse transform, one rescale, pc_bias_kernel) against the composition that defines its words on the GPU's generic path, on
worst-case words against the checker engine, under the tuning knobs, with operands the native path refuses, on two logical
devices, and decrypted with real keys against the loop of mc_mults on the same inputs."""
import os

import numpy as np
import pytest
import torch

from liberate_fhe_amd.utils import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PC = dict(logN=13, num_scales=4, num_special_primes=2, is_secured=False)
KS = (1, 2, 3, 4, 5, 9)        # the templates 1 / 2 / 4, a remainder chunk (2 + 1, 4 + 1), three chunks (4 + 4 + 1)
# (index of the plaintext, of the ciphertext) among three of each: objects repeat on both sides
SLOTS = ((0, 0), (1, 1), (0, 2), (2, 0), (1, 0), (2, 2), (0, 1), (1, 2), (2, 1))


def words(ct):
    return [torch.cat([t.cpu() for t in comp]) for comp in ct.data]


def same(a, b):
    return a.level == b.level and a.origin == b.origin and all(torch.equal(x, y) for x, y in zip(words(a), words(b)))


def params_of(name):
    from liberate_fhe_amd.fhe import presets
    if name == "silver":
        return {k: v for k, v in presets.params[name].items() if k != "devices"}
    if name == "logN17":
        return dict(logN=17, num_scales=3, num_special_primes=2, is_secured=False)     # the five-stage column split
    return PC


_ENGINES = {}


def engine(name):
    """Engines of this file live as long as the process (tests/test_cc_dot_gpu.py: scratch noted by the library is never freed)."""
    from liberate_fhe_amd.fhe import ckks_engine
    if name not in _ENGINES:
        _ENGINES[name] = ckks_engine(devices=["cuda:0"], **params_of(name))
    return _ENGINES[name]


def message(eng, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, eng.num_slots) + 1j * rng.uniform(-1, 1, eng.num_slots)


def lazy(eng, ct):
    """+ q on every third coefficient of c0 and every other one of c1: lazy words below 2q."""
    q = torch.as_tensor(eng._consts(0, ct.level, False).q_host).view(-1, 1).to(ct.data[0][0].device)
    out = []
    for comp, every in ((0, 3), (1, 2)):
        t = ct.data[comp][0].clone()
        t[:, ::every] += q
        out.append([t])
    return ct._replace(data=tuple(out))


def pool_of(eng, level, seed=50):
    """Three plaintexts and three ciphertexts (two of them lazy) of one level, and a bias for the level above."""
    pts = [eng.encode_plain(message(eng, seed + i), level) for i in range(3)]
    cts = [synth.ciphertext(eng, seed + i, level) for i in range(3)]
    cts = [lazy(eng, cts[0]), cts[1], lazy(eng, cts[2])]
    return pts, cts, eng.encode_plain(message(eng, seed + 7), level + 1, "add")


def pairs_of(pts, cts, k):
    return [(pts[i], cts[j]) for i, j in SLOTS[:k]]


def run(eng, fn, native):
    """fn() with the native calls on, or (native_ops off) on the GPU's generic path: the compositions"""
    be = eng.backend
    old = be.native_ops
    be.native_ops = native
    try:
        assert (eng._native_level(0) is not None) == native
        return fn()
    finally:
        be.native_ops = old


def count_native_calls(eng, monkeypatch):
    calls = []
    real = eng.backend.pc_dot_native
    monkeypatch.setattr(eng.backend, "pc_dot_native", lambda *a, **k: (calls.append(a[4]), real(*a, **k))[1], raising=False)
    return calls


def composition(eng, pairs, bias=None):
    """The definition of the op's words, written out (tests/test_pc_dot_cpu.py holds the engine's generic path to it on the checker)."""
    from tests.test_pc_dot_cpu import composition as written_out
    return written_out(eng, pairs, bias)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["logN13", "silver", "logN17"])
def test_native_call_equals_the_composition(name, monkeypatch):
    """Levels 0, a middle one and the last legal one (a single surviving row), every k of KS (fewer on the large rings), with and
    without bias, lazy and repeated operands: exactly one lf_pc_dot call per pc_dot, the words of the generic path."""
    eng = engine(name)
    calls = count_native_calls(eng, monkeypatch)
    L = eng.num_levels
    for level in sorted({0, (L - 1) // 2, L - 2}):
        pts, cts, bias = pool_of(eng, level, 50 + level)
        for k in KS if name == "logN13" else ((1, 5, 9) if level == 0 else (2, 3, 4)):
            pairs = pairs_of(pts, cts, k)
            for b in (None, bias):
                n = len(calls)
                nat = run(eng, lambda: eng.pc_dot(pairs, b), True)
                assert calls[n:] == [k]                                        # ONE native call
                gen = run(eng, lambda: eng.pc_dot(pairs, b), False)
                assert len(calls) == n + 1
                assert nat.level == level + 1 and not nat.ntt_state and not nat.include_special
                assert same(nat, gen), (name, level, k, b is not None)
                if k == 3:   # the generic path IS the composition written out
                    assert same(gen, composition(eng, pairs, b)), (name, level)
        # one pair without bias: pc_mult's words
        assert same(run(eng, lambda: eng.pc_dot([(pts[0], cts[0])]), True), eng.pc_mult(pts[0], cts[0])), (name, level)


def checker_engine():
    from liberate_fhe_amd.fhe import ckks_engine
    from tests.oracle_backend import OracleBackend
    return ckks_engine(devices=["cpu"], backend=OracleBackend(), **PC)


@pytest.mark.gpu
def test_worst_case_words():
    """Every ciphertext word 2q - 1 on all rows, every plaintext word q - 1 (Montgomery form, built directly as tensors), k = 9:
    the largest accumulators of both row classes (two chunks of 4 and one of 1 behind the first write).  Also 0 / 2q - 1 on
    alternating coefficients against a plaintext of 2q - 1 (the lazy bound).  Native call against the checker engine."""
    from tests.test_cc_dot_gpu import edge_ciphertexts
    outs = []
    for eng in (engine("logN13"), checker_engine()):
        res = []
        for level in (0, eng.num_levels - 2):
            e = edge_ciphertexts(eng, level)
            q = torch.tensor([int(eng.ctx.q[i]) for i in eng.ntt.p.destination_arrays[level][0]], dtype=torch.int64).view(-1, 1)
            like = eng.encode_plain(message(eng, 1), level)
            dev = like.data[0].device
            top = like._replace(data=[(q - 1).expand(-1, eng.ctx.N).contiguous().to(dev)])
            lazy_top = like._replace(data=[(2 * q - 1).expand(-1, eng.ctx.N).contiguous().to(dev)])
            q1 = torch.tensor([int(eng.ctx.q[i]) for i in eng.ntt.p.destination_arrays[level + 1][0]], dtype=torch.int64).view(-1, 1)
            bias = eng.encode_plain(message(eng, 2), level + 1, "add")
            bias = bias._replace(data=[(2 * q1 - 1).expand(-1, eng.ctx.N).contiguous().to(dev)])
            for pairs, b in (([(top, e["top"])] * 9, None), ([(top, e["top"])] * 9, bias), ([(lazy_top, e["even"]), (top, e["odd"]), (lazy_top, e["rows"])], bias),
                             ([(top, e["zero"])], bias)):
                if str(dev).startswith("cuda"):
                    assert eng._native_level(level + 1) is not None
                res.append(words(eng.pc_dot(pairs, b)))
        outs.append(res)
    assert len(outs[0]) == len(outs[1]) == 8
    assert all(torch.equal(a[c], b[c]) for a, b in zip(*outs) for c in range(2))


@pytest.mark.gpu
def test_gpu_equals_the_checker():
    """k = 5 with bias (and k = 1 without) on the logN 13 ring: encode_plain's tensors and pc_dot's words against the checker
    engine's.  The polynomial encode returns is random (its rounding), so the checker's plaintexts are carried over."""
    gpu, cpu = engine("logN13"), checker_engine()
    for level in (0, 1):
        pts_c = [cpu.encode_plain(message(cpu, 30 + i), level) for i in range(3)]
        bias_c = cpu.encode_plain(message(cpu, 40), level + 1, "add")
        cts_c = [synth.ciphertext(cpu, 70 + level + i, level) for i in range(3)]
        up = lambda x: x._replace(data=[t.to("cuda:0") for t in x.data], hash=gpu.hash)
        pts_g, bias_g = [up(p) for p in pts_c], up(bias_c)
        cts_g = [synth.ciphertext(gpu, 70 + level + i, level) for i in range(3)]
        assert all(torch.equal(a.cpu(), b) for g, c in zip(cts_g, cts_c) for x, y in zip(g.data, c.data) for a, b in zip(x, y))
        for k, with_bias in ((5, True), (1, False)):
            got = gpu.pc_dot(pairs_of(pts_g, cts_g, k), bias_g if with_bias else None)
            want = cpu.pc_dot(pairs_of(pts_c, cts_c, k), bias_c if with_bias else None)
            assert all(torch.equal(a, b) for a, b in zip(words(got), words(want))), (level, k)


def knob_walk():
    """The body of test_tuning_knobs_change_no_word; it flips process-wide knobs, so it runs in a process of its own."""
    from liberate_fhe_amd._native import lib
    outs = []
    for name in ("logN13", "silver"):
        eng = engine(name)
        pts, cts, bias = pool_of(eng, 0, 12)
        pairs = pairs_of(pts, cts, 5)
        res = []
        for planes, more in ((1, 3), (0, 3), (1, 0), (1, 1), (0, 0)):
            lib.lf_tune(3, planes), lib.lf_tune(5, more)
            for native in (True, False):
                res.append(run(eng, lambda: eng.pc_dot(pairs, bias), native))
        outs.append(res)
    assert all(len(res) == 10 and all(same(o, res[0]) for o in res[1:]) for res in outs)


@pytest.mark.gpu
def test_tuning_knobs_change_no_word():
    """LF_TUNE_DIGIT_PLANES and LF_TUNE_MORE_PLANES (bit 1: the stack planes), on the native call and on the composition, in a
    fresh child process (tests/test_cc_dot_gpu.py says why)."""
    import subprocess
    import sys
    code = f"import sys; sys.path.insert(0, {ROOT!r}); from tests.test_pc_dot_gpu import knob_walk; knob_walk()"
    flags = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable, *flags, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]


@pytest.mark.gpu
def test_operands_the_native_path_refuses_take_the_composition(monkeypatch):
    """A non-contiguous ciphertext component, and one at an odd word offset (contiguous, not 16-byte aligned): no native call, the
    same words (the composition works on clones of the ciphertexts)."""
    eng = engine("logN13")
    calls = count_native_calls(eng, monkeypatch)
    pts, cts, bias = pool_of(eng, 0, 20)
    want = eng.pc_dot(pairs_of(pts, cts, 3), bias)
    assert len(calls) == 1
    N = eng.ctx.N

    def strided(t):
        wide = torch.zeros((t.size(0), 2 * N), dtype=torch.int64, device=t.device)
        wide[:, ::2] = t
        return wide[:, ::2]

    def odd(t):
        flat = torch.zeros(t.numel() + 1, dtype=torch.int64, device=t.device)
        flat[1:] = t.reshape(-1)
        return flat[1:].view(t.shape)

    s = cts[1]._replace(data=([strided(cts[1].data[0][0])], [cts[1].data[1][0]]))
    assert not s.data[0][0].is_contiguous()
    o = cts[2]._replace(data=([cts[2].data[0][0]], [odd(cts[2].data[1][0])]))
    assert o.data[1][0].is_contiguous() and o.data[1][0].data_ptr() % 16 == 8
    for c in ([cts[0], s, cts[2]], [cts[0], cts[1], o], [cts[0], s, o]):
        got = eng.pc_dot(pairs_of(pts, c, 3), bias)
        assert len(calls) == 1 and same(got, want)


def natural_rows(eng, ct):
    """Components as [rows, N] arrays with the rows in the order of the prime chain (tests/test_cc_dot_gpu.py)."""
    dest = eng.ntt.p.destination_arrays[ct.level]
    out = []
    for comp in ct.data:
        rows = {}
        for d, t in enumerate(comp):
            arr = t.cpu().numpy()
            for r, prime in enumerate(dest[d]):
                rows[prime] = arr[r]
        out.append(np.stack([rows[k] for k in sorted(rows)]))
    return out


@pytest.mark.gpu
def test_two_logical_devices_take_the_composition(monkeypatch):
    """Two shards: no native call; row by row in prime order the words of one device (the plaintexts carried over in the host
    form: the polynomial encode returns is random)."""
    from liberate_fhe_amd.fhe import ckks_engine
    one = engine("logN13")
    two = _ENGINES.setdefault("logN13 x 2", ckks_engine(devices=["cuda:0"] * 2, **PC))
    assert one._native_level(1) is not None and two._native_level(1) is None
    hosts = [one.cpu(one.encode_plain(message(one, 5 + i), 0)) for i in range(3)] + [one.cpu(one.encode_plain(message(one, 9), 1, "add"))]
    res = []
    for eng, want_calls in ((one, 1), (two, 0)):
        calls = count_native_calls(eng, monkeypatch)
        *pts, bias = [eng.cuda(h._replace(hash=eng.hash)) for h in hosts]
        cts = [synth.ciphertext(eng, 8 + i, 0) for i in range(3)]
        out = eng.pc_dot(pairs_of(pts, cts, 5), bias)
        assert len(calls) == want_calls and out.level == 1
        res.append(natural_rows(eng, out))
    for x, y in zip(*res):
        assert x.shape == y.shape and (x == y).all()


@pytest.mark.gpu
def test_real_keys_decrypt_within_twice_the_loop_on_silver():
    """silver, real keys, k = 3 random real vectors with |.| <= 1 against three encrypted ones, and a bias: pc_dot's maximum
    decryption error against float64 is at most 2 x that of the mc_mult / cc_add / mc_add loop on the same inputs in the same run
    (one rescale rounding instead of three; the factor covers the independent random roundings of the two sets of encodings).
    Both errors are printed."""
    eng = engine("silver")
    sk = eng.create_secret_key()
    pk = eng.create_public_key(sk)
    rng = np.random.default_rng(12)
    n = eng.num_slots
    ws = [rng.uniform(-1, 1, n) for _ in range(3)]
    xs = [rng.uniform(-1, 1, n) for _ in range(3)]
    b = rng.uniform(-1, 1, n)
    cts = [eng.encorypt(x, pk) for x in xs]
    want = sum(w * x for w, x in zip(ws, xs)) + b
    assert eng._native_level(1) is not None
    got = eng.pc_dot([(eng.encode_plain(w, 0), ct) for w, ct in zip(ws, cts)], eng.encode_plain(b, 1, "add"))
    assert got.level == 1
    loop = None
    for w, ct in zip(ws, cts):
        p = eng.mc_mult(w, ct)
        loop = p if loop is None else eng.cc_add(loop, p)
    loop = eng.mc_add(b, loop)
    e_dot = np.abs(eng.decrode(got, sk).real - want).max()
    e_loop = np.abs(eng.decrode(loop, sk).real - want).max()
    print(f"silver, k = 3 + bias, level 0: max abs error pc_dot {e_dot:.3e}, mc_mult / cc_add / mc_add loop {e_loop:.3e}, "
          f"largest entry {np.abs(want).max():.2f}")
    assert e_dot <= 2 * e_loop and e_loop < 1e-5
