"""weighted_sums / poly_eval on the GPU: lf_weighted_sums (weighted_sums_kernel<4 | 2 | 1>, one native call) against the
composition that defines its words on the GPU's generic path, on worst-case words and at the rounding compare's edge through the
integer entry, against the checker engine, with compact keys, under the tuning knobs, on two logical devices; poly_eval against
the checker engine's words; and both bases decrypted with real keys against float64 evaluation within 8 A e_unit."""
import json
import os

import numpy as np
import pytest
import torch
from numpy.polynomial import chebyshev as C

from liberate_fhe_amd.fhe import encdec
from liberate_fhe_amd.utils import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "engine_digests.json")))
POLY = dict(logN=13, num_scales=8, num_special_primes=2, is_secured=False)
KS = (1, 2, 3, 5, 16)          # one term, the unrolled groups of 4 and their remainders, the cap
GS = (1, 2, 4, 5, 9)           # the templates 1 / 2 / 4, a second launch (4 + 1), two launches of 4 and one of 1


def words(ct):
    return [torch.cat([t.cpu() for t in comp]) for comp in ct.data]


def same(a, b):
    return a.level == b.level and a.origin == b.origin and all(torch.equal(x, y) for x, y in zip(words(a), words(b)))


def all_same(xs, ys):
    return len(xs) == len(ys) and all(same(x, y) for x, y in zip(xs, ys))


def params_of(name):
    from liberate_fhe_amd.fhe import presets
    if name == "silver":
        return {k: v for k, v in presets.params[name].items() if k != "devices"}
    if name == "logN13":
        return POLY
    if name == "logN17":
        return dict(logN=17, num_scales=3, num_special_primes=2, is_secured=False)
    return GOLD[name]["params"]


_KEEP = []


def keep(eng):
    """Engines of this file live as long as the process (tests/test_cc_dot_gpu.py: scratch noted by the library is never freed)."""
    _KEEP.append(eng)
    return eng


_ENGINES = {}


def engine(name):
    from liberate_fhe_amd.fhe import ckks_engine
    if name not in _ENGINES:
        _ENGINES[name] = keep(ckks_engine(devices=["cuda:0"], **params_of(name)))
    return _ENGINES[name]


def lazy(eng, ct):
    """+ q on every third coefficient of c0 and every other one of c1: lazy words below 2q."""
    level = ct.level
    q = torch.as_tensor(eng._consts(0, level, False).q_host).view(-1, 1).to(ct.data[0][0].device)
    out = []
    for comp, every in ((0, 3), (1, 2)):
        t = ct.data[comp][0].clone()
        t[:, ::every] += q
        out.append([t])
    return ct._replace(data=tuple(out))


def pool_of(eng, level, seed=50):
    cts = [synth.ciphertext(eng, seed + i, level) for i in range(3)]
    return [lazy(eng, cts[0]), cts[1], lazy(eng, cts[2])]


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


def sums_composition(eng, cts, weights, consts=None):
    l = cts[0].level
    outs = []
    for g, row in enumerate(weights):
        acc = None
        for ct, w in zip(cts, row):
            s = int(w * eng.scale * np.sqrt(eng.deviations[l + 1]) + 0.5)
            term = eng._scale_rows(ct, eng._row_scalars(s, l, True))
            acc = term if acc is None else eng.cc_add(acc, term)
        out = eng.rescale(acc)
        if consts is not None:
            out = eng.add_scalar(out, consts[g])
        outs.append(out)
    return outs


def count_native_calls(eng, monkeypatch):
    calls = []
    real = eng.backend.weighted_sums_native
    monkeypatch.setattr(eng.backend, "weighted_sums_native", lambda *a, **k: (calls.append(a[3:5]), real(*a, **k))[1], raising=False)
    return calls


@pytest.mark.gpu
def test_native_call_equals_the_composition(monkeypatch):
    """logN 13, levels 0, 1 and L - 2, every k of KS with every G of GS, with and without consts, operand objects repeating;
    k = 17 takes the composition with the same words."""
    eng = engine("logN13")
    calls = count_native_calls(eng, monkeypatch)
    rng = np.random.default_rng(2)
    L = eng.num_levels
    for level in sorted({0, 1, L - 2}):
        pool = pool_of(eng, level, 50 + level)
        for k in KS:
            cts = [pool[i % 3] for i in range(k)]
            for G in GS:
                w = rng.uniform(-2, 2, (G, k))
                w[G // 2, k // 2] = 0.0
                consts = rng.uniform(-3, 3, G) if (k + G) % 2 else None
                n = len(calls)
                nat = run(eng, lambda: eng.weighted_sums(cts, w, consts), True)
                assert calls[n:] == [(k, G)]                                  # ONE native call
                gen = run(eng, lambda: eng.weighted_sums(cts, w, consts), False)
                assert len(calls) == n + 1
                assert len(nat) == G and all(o.level == level + 1 and not o.ntt_state and not o.include_special for o in nat)
                assert all_same(nat, gen), (level, k, G)
                if (k, G) in ((3, 2), (5, 5)):   # the generic path IS the composition written out
                    assert all_same(gen, sums_composition(eng, cts, w, consts)), (level, k, G)
        # one term: mult_scalar's words
        assert same(eng.weighted_sum([pool[0]], [0.625]), eng.mult_scalar(pool[0], 0.625))
        # above the cap: the composition, the same words
        cts = [pool[i % 3] for i in range(17)]
        w, consts = rng.uniform(-1, 1, (2, 17)), rng.uniform(-1, 1, 2)
        n = len(calls)
        got = eng.weighted_sums(cts, w, consts)
        assert len(calls) == n
        assert all_same(got, sums_composition(eng, cts, w, consts)), level
        # non-contiguous operands: the composition
        views = []
        for c in range(2):
            wide = torch.zeros((pool[1].data[c][0].size(0), 2 * eng.ctx.N), dtype=torch.int64, device="cuda:0")
            wide[:, ::2] = pool[1].data[c][0]
            views.append([wide[:, ::2]])
        strided = pool[1]._replace(data=tuple(views))
        assert not strided.data[0][0].is_contiguous() and torch.equal(strided.data[1][0], pool[1].data[1][0])
        got = eng.weighted_sums([pool[0], strided], w[:, :2], consts)
        assert len(calls) == n and all_same(got, eng.weighted_sums([pool[0], pool[1]], w[:, :2], consts))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["silver", "sb45", "sb41", "logN17"])
def test_native_call_equals_the_composition_on_other_rings(name):
    """Mixed prime classes (sb45, sb41), the larger two-pass rings (silver: logN 15, logN 17): one level each, three shapes."""
    eng = engine(name)
    rng = np.random.default_rng(4)
    level = 1 if eng.num_levels > 3 else 0
    pool = pool_of(eng, level, 60)
    for k, G in ((3, 4), (16, 5), (2, 1)) if name != "logN17" else ((3, 4), (5, 1)):
        cts = [pool[i % 3] for i in range(k)]
        w, consts = rng.uniform(-2, 2, (G, k)), rng.uniform(-3, 3, G)
        nat = run(eng, lambda: eng.weighted_sums(cts, w, consts), True)
        gen = run(eng, lambda: eng.weighted_sums(cts, w, consts), False)
        assert all_same(nat, gen), (name, k, G)


def crt_minus_one(eng, level):
    """The integer = q_i - 1 on every row of `level`: the product of its primes, minus one."""
    Q = 1
    for i in eng.ntt.p.destination_arrays[level][0]:
        Q *= int(eng.ctx.q[i])
    return Q - 1


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sb41", "logN13"])
def test_worst_case_words(name):
    """Operands at 2q - 1 and 0 on whole rows and on alternating coefficients (edge_ciphertexts of the cc_dot test), integer
    weights 0, 1, -1 and = q_i - 1 on every row, a const = q_i - 1 on every row; 16 terms of 2q - 1 times q - 1 give the largest
    128-bit sum the kernel can meet.  Native call against the composition, through the integer entry."""
    from tests.test_cc_dot_gpu import edge_ciphertexts
    eng = engine(name)
    for level in (0, eng.num_levels - 2):
        e = edge_ciphertexts(eng, level)
        big, cbig = crt_minus_one(eng, level), crt_minus_one(eng, level + 1)
        cases = [
            ([e["top"]] * 16, [[big] * 16, [1] * 16, [-1] * 16, [0] * 16], [cbig, 0, 1, cbig]),
            ([e["top"], e["zero"], e["rows"], e["even"], e["odd"], e["top|even"]],
             [[big, 1, -1, 0, big, 1], [1, 1, 1, 1, 1, 1], [-1, big, 0, 1, -1, big], [0, 0, 0, 0, 0, 0], [big] * 6], [cbig] * 5),
            ([e["zero"], e["zero"]], [[big, 1]], None),
            ([e["even"], e["odd"]], [[1, 1], [big, big]], [cbig, cbig]),
            ([e["top"]], [[big]], None),
        ]
        for i, (cts, ints, cint) in enumerate(cases):
            nat = run(eng, lambda: eng._weighted_sums_int(cts, ints, cint), True)
            gen = run(eng, lambda: eng._weighted_sums_int(cts, ints, cint), False)
            assert all_same(nat, gen), (name, level, i)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sb41", "logN13"])
def test_the_rounding_compare_at_its_edge(name):
    """Inputs built so that the accumulator's dropped row is q_l / 2 (the last word that rounds down) on one half of the
    coefficients and q_l / 2 + 1 (the first that rounds up) on the other: 3 A - 2 B with A's dropped row solved for in Python
    integers; the composition's accumulator is checked to hold exactly those words, then the native call against it."""
    eng = engine(name)
    for level in (0, 2):
        q0 = int(eng.ctx.q[eng.ntt.p.destination_arrays[level][0][0]])
        round_at = q0 // 2
        N = eng.ctx.N
        A, B = synth.ciphertext(eng, 31, level), synth.ciphertext(eng, 32, level)
        inv3 = pow(3, -1, q0)
        data, targets = [], []
        for comp in range(2):
            target = [round_at + ((j + comp) & 1) for j in range(N)]
            b0 = B.data[comp][0][0].cpu().tolist()
            row0 = [(t + 2 * b) * inv3 % q0 for t, b in zip(target, b0)]
            t = A.data[comp][0].clone()
            t[0] = torch.tensor(row0, dtype=torch.int64)
            data.append([t])
            targets.append(torch.tensor(target, dtype=torch.int64))
        A = A._replace(data=tuple(data))
        ints = [[3, -2], [1, 0], [3, -2]]

        def acc_rows():
            acc = eng.cc_add(eng.mult_int_scalar(A, 3), eng.mult_int_scalar(B, -2))
            return [acc.data[c][0][0].cpu() for c in range(2)]

        got = run(eng, acc_rows, False)
        assert all(torch.equal(g, t) for g, t in zip(got, targets))
        assert {int(v) for v in targets[0]} == {round_at, round_at + 1}
        nat = run(eng, lambda: eng._weighted_sums_int([A, B], ints, [0, 1, 2]), True)
        gen = run(eng, lambda: eng._weighted_sums_int([A, B], ints, [0, 1, 2]), False)
        assert all_same(nat, gen), (name, level)
        # the two halves do round differently: against the same sum with the rounding bit dropped
        down = eng.rescale(eng.cc_add(eng.mult_int_scalar(A, 3), eng.mult_int_scalar(B, -2)), exact_rounding=False)
        diff = (words(nat[0])[0] - words(down)[0]) % torch.tensor([int(eng.ctx.q[i]) for i in eng.ntt.p.destination_arrays[level + 1][0]]).view(-1, 1)
        assert torch.equal(diff[:, 0::2], torch.zeros_like(diff[:, 0::2])) and torch.equal(diff[:, 1::2], torch.ones_like(diff[:, 1::2]))


@pytest.mark.gpu
def test_gpu_equals_the_checker():
    """weighted_sums (native) and poly_eval (power basis degrees 7 and 15, Chebyshev degree 15 on (-4, 4)) against the checker
    engine on the same inputs."""
    from liberate_fhe_amd.fhe import ckks_engine
    from tests.oracle_backend import OracleBackend
    got, want = [], []
    rng = np.random.default_rng(6)
    w, consts = rng.uniform(-2, 2, (5, 3)), rng.uniform(-2, 2, 5)
    c7, c15 = rng.uniform(-1, 1, 8), rng.uniform(-1, 1, 16)
    for eng, out in ((engine("logN13"), got), (ckks_engine(devices=["cpu"], backend=OracleBackend(), **POLY), want)):
        evk = synth.key_switch_key(eng, 77)
        if str(eng.ntt.devices[0]).startswith("cuda"):
            assert eng._native_level(1) is not None
        for level in (0, 2):
            cts = [synth.ciphertext(eng, 70 + level + i, level) for i in range(3)]
            out += [words(o) for o in eng.weighted_sums(cts, w, consts)]
        x = synth.ciphertext(eng, 80, 1)
        out.append(words(eng.poly_eval(x, c7, evk)))
        out.append(words(eng.poly_eval(x, c15, evk)))
        out.append(words(eng.poly_eval(x, c15, evk, basis="chebyshev", interval=(-4, 4))))
    assert len(got) == len(want) == 13
    assert all(torch.equal(a[c], b[c]) for a, b in zip(got, want) for c in range(2))


@pytest.mark.gpu
def test_compact_keys_give_the_same_words():
    from liberate_fhe_amd.fhe import ckks_engine
    eng = keep(ckks_engine(devices=["cuda:0"], **POLY))
    sk = eng.create_secret_key()
    evk = eng.create_evk(sk)
    x = synth.ciphertext(eng, 5, 1)
    coeffs = np.random.default_rng(9).uniform(-1, 1, 8)
    want = eng.poly_eval(x, coeffs, evk)
    assert same(want, run(eng, lambda: eng.poly_eval(x, coeffs, evk), False))
    eng.compact_key(evk)
    assert same(eng.poly_eval(x, coeffs, evk), want)
    assert same(run(eng, lambda: eng.poly_eval(x, coeffs, evk), False), want)


def knob_walk():
    """The body of test_tuning_knobs_change_no_word; it flips process-wide knobs, so it runs in a process of its own."""
    from liberate_fhe_amd._native import lib
    eng = engine("logN13")
    evk = synth.key_switch_key(eng, 77)
    pool = pool_of(eng, 0, 12)
    rng = np.random.default_rng(10)
    w, consts, coeffs = rng.uniform(-2, 2, (5, 3)), rng.uniform(-2, 2, 5), rng.uniform(-1, 1, 8)
    x = synth.ciphertext(eng, 13, 1)
    outs = []
    for planes, more, cols in ((1, 3, 5), (0, 3, 5), (1, 0, 5), (1, 3, 0), (0, 0, 0)):
        lib.lf_tune(3, planes), lib.lf_tune(5, more), lib.lf_tune(1, cols)
        for native in (True, False):
            outs.append(run(eng, lambda: eng.weighted_sums(pool, w, consts) + [eng.poly_eval(x, coeffs, evk)], native))
    assert len(outs) == 10 and all(all_same(o, outs[0]) for o in outs[1:])


@pytest.mark.gpu
def test_tuning_knobs_change_no_word():
    """LF_TUNE_DIGIT_PLANES, LF_TUNE_MORE_PLANES and LF_TUNE_KS_EXT_COLS_MAX, on the native calls and on the compositions, in a
    fresh child process (tests/test_cc_dot_gpu.py says why)."""
    import subprocess
    import sys
    code = f"import sys; sys.path.insert(0, {ROOT!r}); from tests.test_poly_eval_gpu import knob_walk; knob_walk()"
    flags = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable, *flags, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]


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
    """Two shards: no native call; row by row in prime order the words of one device."""
    from liberate_fhe_amd.fhe import ckks_engine
    rng = np.random.default_rng(11)
    w, consts = rng.uniform(-2, 2, (3, 4)), rng.uniform(-2, 2, 3)
    res = []
    for n_dev in (1, 2):
        eng = keep(ckks_engine(devices=["cuda:0"] * n_dev, **POLY))
        assert (eng._native_level(1) is not None) == (n_dev == 1)
        calls = count_native_calls(eng, monkeypatch)
        cts = [synth.ciphertext(eng, 8 + i, 0) for i in range(4)]
        outs = eng.weighted_sums(cts, w, consts)
        assert len(calls) == (1 if n_dev == 1 else 0) and all(o.level == 1 for o in outs)
        res.append([natural_rows(eng, o) for o in outs])
    for a, b in zip(*res):
        for x, y in zip(a, b):
            assert x.shape == y.shape and (x == y).all()


def unit_error(eng, x, pk, sk, evk, level):
    """Decryption error of a ciphertext brought to `level` by the chain of squares on the input x, |x| <= 1."""
    ct, want = eng.encorypt(x, pk), x.copy()
    while ct.level < level:
        ct, want = eng.square(ct, evk), want * want
    return np.abs(eng.decrode(ct, sk).real - want).max()


@pytest.mark.gpu
def test_real_keys_decrypt_within_the_bound_on_silver():
    """silver, real keys.  Power basis, degree 15, random coefficients, messages in [-1, 1]; Chebyshev, degree 31, the
    interpolant of the logistic sigmoid on (-8, 8), messages in (-8, 8).  The error against the float64 evaluation of the same
    series on the DECODED input is at most 8 A e_unit: A the sum of the absolute host coefficients actually multiplied in,
    e_unit the decryption error of the chain of squares brought to the result's level on the same input (scaled into [-1, 1]
    for the sigmoid): each product q_g y^g contributes at most |q_g| err(y^g) + err(q_g) |y^g| <= 2 A_g e_unit, the factor 4
    over that covers the extra level_ups and scalar rescales; a wrong coefficient, level or deviation gives errors many orders
    above.  All four numbers are printed."""
    from liberate_fhe_amd.fhe import ckks_engine, presets
    eng = keep(ckks_engine(**{**presets.params["silver"], "devices": ["cuda:0"]}))
    sk = eng.create_secret_key()
    pk = eng.create_public_key(sk)
    evk = eng.create_evk(sk)
    rng = np.random.default_rng(5)
    n = eng.num_slots
    sigmoid = C.chebinterpolate(lambda t: 1.0 / (1.0 + np.exp(-8.0 * t)), 31)
    cases = [("power", rng.uniform(-1, 1, 16), None, rng.uniform(-1, 1, n)),
             ("chebyshev", sigmoid, (-8, 8), rng.uniform(-8, 8, n))]
    for basis, coeffs, interval, x in cases:
        d = len(coeffs) - 1
        ct = eng.encorypt(x, pk)
        x_dec = eng.decrode(ct, sk).real
        assert eng._native_level(ct.level + 1) is not None
        got = eng.poly_eval(ct, coeffs, evk, basis=basis, interval=interval)
        n1 = encdec.poly_split(d)
        if basis == "chebyshev":
            blocks = encdec.cheb_blocks(coeffs, n1)
            want = C.chebval(x_dec / 8.0, coeffs)
        else:
            blocks = coeffs.reshape(-1, n1)
            want = np.polynomial.polynomial.polyval(x_dec, coeffs)
        A = np.abs(blocks).sum()
        err = np.abs(eng.decrode(got, sk).real - want).max()
        e_unit = unit_error(eng, x if interval is None else x / 8.0, pk, sk, evk, got.level)
        print(f"silver, {basis}, degree {d}, n1 {n1}, level {got.level}: max abs error {err:.3e}, A = {A:.3f}, "
              f"e_unit {e_unit:.3e}, bound {8 * A * e_unit:.3e}")
        assert got.level == eng.poly_depth(d, basis, interval) and err <= 8 * A * e_unit, (basis, err, A, e_unit)
