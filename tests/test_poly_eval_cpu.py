"""weighted_sums / poly_eval (liberate_fhe_amd/fhe/polyeval.py, lf_weighted_sums) without a GPU: the engine's host logic on the
checker backend against the compositions of public ops that define the words, the level schedule, the refusals, the host math
of the Chebyshev split and of poly_split, the C entry's argument checks, the new kernels' resources, and the decryption error
with real keys."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
from numpy.polynomial import chebyshev as C

from liberate_fhe_amd.fhe import encdec
from liberate_fhe_amd.utils import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POLY = dict(logN=13, num_scales=8, num_special_primes=2, is_secured=False)   # 9 levels: degree 15 on an interval needs 6


def words(ct):
    return [torch.cat([t.cpu() for t in comp]) for comp in ct.data]


def same(a, b):
    wa, wb = words(a), words(b)
    return a.level == b.level and a.origin == b.origin and len(wa) == len(wb) and all(torch.equal(x, y) for x, y in zip(wa, wb))


@pytest.fixture(scope="module")
def checker():
    from liberate_fhe_amd.fhe import ckks_engine
    from tests.oracle_backend import OracleBackend
    return ckks_engine(devices=["cpu"], backend=OracleBackend(), **POLY)


@pytest.fixture(scope="module")
def evk(checker):
    return synth.key_switch_key(checker, 77)


def lazy_ciphertext(eng, seed, level):
    """synth ciphertext with lazy words sprinkled in (tests/test_cc_dot_cpu.py)."""
    ct = synth.ciphertext(eng, seed, level)
    for comp, every in ((0, 3), (1, 2)):
        for i, d in enumerate(eng._loc(level)):
            q = torch.as_tensor(eng._consts(d, level, False).q_host).view(-1, 1).to(ct.data[comp][i].device)
            t = ct.data[comp][i].clone()
            t[:, ::every] += q
            ct.data[comp][i] = t
    return ct


def sums_composition(eng, cts, weights, consts=None):
    """The definition of weighted_sums' words, written out."""
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


def tree_powers(eng, x, top, evk, cheb):
    """{b: x^b or T_b(x)} for b <= top by the tree rule, one public op at a time."""
    p = {1: x}
    for b in range(2, top + 1):
        hi = 1 << (b.bit_length() - 1)
        if b == hi:
            sq = eng.square(p[hi // 2], evk)
            p[b] = eng.add_scalar(eng.mult_int_scalar(sq, 2), -1) if cheb else sq
        else:
            prod = eng.auto_cc_mult(p[hi], p[b - hi], evk)
            p[b] = eng.auto_cc_sub(eng.mult_int_scalar(prod, 2), p[abs(hi - (b - hi))]) if cheb else prod
    return p


def up(eng, ct, level):
    return ct if ct.level == level else eng.level_up(ct, level)


def poly_composition(eng, ct, coeffs, evk, basis, interval, n1):
    """The definition of poly_eval's words, written out from public ops (levels taken from the ciphertexts themselves)."""
    coeffs = np.asarray(coeffs, dtype=np.float64)
    cheb = basis == "chebyshev"
    G = -(-coeffs.size // n1)
    if cheb:
        if interval is not None and tuple(interval) != (-1, 1):
            a, b = interval
            ct = eng.add_scalar(eng.mult_scalar(ct, 2.0 / (b - a)), -(a + b) / (b - a))
        blocks, c = [], coeffs
        divisor = np.zeros(n1 + 1)
        divisor[n1] = 1
        for g in range(G):
            if c.size > n1:
                c, rem = C.chebdiv(c, divisor)
            else:
                c, rem = np.zeros(1), c
            blocks.append(np.concatenate([rem, np.zeros(n1 - rem.size)]))
    else:
        blocks = [np.concatenate([coeffs[g * n1:(g + 1) * n1], np.zeros(n1)])[:n1] for g in range(G)]
    p = tree_powers(eng, ct, n1 - 1, evk, cheb)
    Lb = max(p[b].level for b in range(1, n1))
    babies = [up(eng, p[b], Lb) for b in range(1, n1)]
    q = eng.weighted_sums(babies, [blk[1:] for blk in blocks], consts=[blk[0] for blk in blocks])
    if G == 1:
        return q[0]
    y = eng.square(p[n1 // 2], evk)
    if cheb:
        y = eng.add_scalar(eng.mult_int_scalar(y, 2), -1)
    ys = tree_powers(eng, y, G - 1, evk, False)
    Lc = max(ys[G - 1].level, Lb + 1)
    r = eng.cc_dot([(up(eng, q[g], Lc), up(eng, ys[g], Lc)) for g in range(1, G)], evk)
    return eng.cc_add(r, eng.level_up(q[0], Lc + 1))


@pytest.mark.parametrize("level", [0, 3])
def test_weighted_sums_equal_the_composition(checker, level):
    from liberate_fhe_amd.fhe.presets import types
    eng = checker
    rng = np.random.default_rng(3 + level)
    pool = [lazy_ciphertext(eng, 40 + level, level), synth.ciphertext(eng, 41 + level, level), synth.ciphertext(eng, 42 + level, level)]
    for k in (1, 2, 5):
        cts = [pool[i % 3] for i in range(k)]           # objects repeat from k = 5 on
        for G in (1, 3):
            w = rng.uniform(-2, 2, (G, k))
            w[0, k // 2] = 0.0                          # a zero weight is an ordinary term
            for consts in (None, rng.uniform(-3, 3, G)):
                got = eng.weighted_sums(cts, w, consts)
                want = sums_composition(eng, cts, w, consts)
                assert len(got) == G
                for a, b in zip(got, want):
                    assert a.level == level + 1 and a.origin == types.origins["ct"] and not a.ntt_state and not a.include_special
                    assert same(a, b), (level, k, G, consts is None)
                assert same(eng.weighted_sum(cts, w[0], None if consts is None else consts[0]), want[0])
    # one term, no const: mult_scalar's words
    for s in (0.37, -1.5, 1.0):
        assert same(eng.weighted_sums([pool[0]], [[s]])[0], eng.mult_scalar(pool[0], s))
        assert same(eng.weighted_sum([pool[1]], [s]), eng.mult_scalar(pool[1], s))
    # the integer entry: the same words from the integers themselves
    ints = [[5, -7, 0]]
    acc = None
    for ct, s in zip(pool, ints[0]):
        term = eng.mult_int_scalar(ct, s)
        acc = term if acc is None else eng.cc_add(acc, term)
    assert same(eng._weighted_sums_int(pool, ints)[0], eng.rescale(acc))


def test_weighted_sums_refusals(checker, evk):
    from liberate_fhe_amd.fhe.presets import errors
    eng = checker
    a0, b0, a1 = synth.ciphertext(eng, 1, 0), synth.ciphertext(eng, 2, 0), synth.ciphertext(eng, 3, 1)
    top = synth.ciphertext(eng, 4, eng.num_levels - 1)
    trip = eng.cc_mult(a0, b0, evk, relin=False)
    ntt = eng._new(a0.data, a0.origin, level=0, ntt_state=True)
    special = eng._new(a0.data, a0.origin, level=0, include_special=True)
    for exc, cts, w, c in [
        (ValueError, [], [[]], None),
        (errors.NotMatchType, [a0, trip], [[1, 1]], None),
        (errors.NotMatchType, [a0, None], [[1, 1]], None),
        (errors.NotMatchDataStructState, [a0, a1], [[1, 1]], None),
        (errors.NotMatchDataStructState, [a0, ntt], [[1, 1]], None),
        (errors.NotMatchDataStructState, [special, b0], [[1, 1]], None),
        (errors.MaximumLevelError, [top], [[1]], None),
        (ValueError, [a0, b0], [[1, 1, 1]], None),
        (ValueError, [a0, b0], [1, 1], None),
        (ValueError, [a0, b0], [[1, 1]], [1, 2]),
    ]:
        with pytest.raises(exc):
            eng.weighted_sums(cts, w, c)
    with pytest.raises(ValueError):
        eng._weighted_sums_int([a0, b0], [[1]])
    with pytest.raises(ValueError):      # an interval belongs to the Chebyshev basis
        eng.poly_eval(a0, [1.0, 2.0], evk, interval=(-4, 4))


CASES = [("power", 1, None, None), ("power", 3, None, None), ("power", 7, None, None), ("power", 15, None, None),
         ("power", 15, None, 4), ("chebyshev", 7, (-4, 4), None), ("chebyshev", 15, (-4, 4), None), ("chebyshev", 15, (-4, 4), 4),
         ("chebyshev", 7, None, 2)]


@pytest.mark.parametrize("basis,degree,interval,n1", CASES)
def test_poly_eval_equals_its_composition(checker, evk, basis, degree, interval, n1):
    eng = checker
    rng = np.random.default_rng(degree)
    coeffs = rng.uniform(-1, 1, degree + 1)
    ct = synth.ciphertext(eng, 90 + degree, 1)
    got = eng.poly_eval(ct, coeffs, evk, basis=basis, interval=interval, n1=n1)
    split = encdec.poly_split(degree) if n1 is None else n1
    want = poly_composition(eng, ct, coeffs, evk, basis, interval, split)
    assert same(got, want), (basis, degree, n1)
    assert got.level == 1 + eng.poly_depth(degree, basis, interval, n1)
    sched = encdec.poly_schedule(degree, split)
    assert sched["depth"] + (1 if interval else 0) == got.level - 1 and sched["G"] == -(-(degree + 1) // split)


def test_too_few_levels_is_refused_before_any_op(checker, evk, monkeypatch):
    from liberate_fhe_amd.fhe.presets import errors
    eng = checker
    depth = eng.poly_depth(7, "power")
    assert depth == 4 and eng.poly_depth(7, "chebyshev", (-4, 4)) == 5 and eng.poly_depth(1) == 1
    start = eng.num_levels - depth                  # one level short: the result would stand at num_levels
    ct = synth.ciphertext(eng, 5, start)
    calls = []
    for name in ("cc_mult", "cc_mult_batch", "rescale", "level_up", "weighted_sums", "cc_dot", "mult_scalar", "clone"):
        real = getattr(eng, name)
        monkeypatch.setattr(eng, name, lambda *a, _n=name, _r=real, **k: (calls.append(_n), _r(*a, **k))[1])
    with pytest.raises(errors.MaximumLevelError):
        eng.poly_eval(ct, np.ones(8), evk)
    with pytest.raises(errors.MaximumLevelError):
        eng.poly_eval(synth.ciphertext(eng, 5, start - 1), np.ones(8), evk, basis="chebyshev", interval=(-4, 4))
    with pytest.raises(ValueError):
        eng.poly_eval(ct, [1.0], evk)
    with pytest.raises(ValueError):
        eng.poly_eval(ct, np.ones(8), evk, basis="legendre")
    with pytest.raises(ValueError):
        eng.poly_eval(ct, np.ones(8), evk, n1=3)
    with pytest.raises(errors.NotMatchType):
        eng.poly_eval(evk, np.ones(8), evk)
    assert calls == []
    monkeypatch.undo()
    assert eng.poly_eval(synth.ciphertext(eng, 5, start - 1), np.ones(8), evk).level == eng.num_levels - 1


def test_chebyshev_split_reproduces_the_series():
    """sum_g r_g(x) T_n1(x)^g = p(x) in float64, random Chebyshev series up to degree 63, every n1.  The r_g are what the
    evaluation multiplies in, and A = sum |r_g,b| is the scale of its rounding (plain powers of T_n1 are a monomial basis in y:
    for many giant steps the r_g grow far beyond the c_i, A = 9e11 for degree 63 at n1 = 2), so the error is held to 1e-12
    relative to A for every split, and to 1e-12 relative to sum |c_i| for the split poly_split picks, where A stays small."""
    rng = np.random.default_rng(8)
    x = np.linspace(-1, 1, 2001)
    for degree in (1, 2, 5, 7, 15, 16, 31, 40, 63):
        c = rng.uniform(-1, 1, degree + 1)
        want = C.chebval(x, c)
        for n1 in (2, 4, 8, 16, 32, 64):
            blocks = encdec.cheb_blocks(c, n1)
            assert blocks.shape == (-(-(degree + 1) // n1), n1)
            y = C.chebval(x, [0] * n1 + [1])
            got = sum(C.chebval(x, blocks[g]) * y ** g for g in range(blocks.shape[0]))
            err = np.abs(got - want).max()
            assert err <= 1e-12 * np.abs(blocks).sum(), (degree, n1)
            if n1 == encdec.poly_split(degree):
                assert err <= 1e-12 * np.abs(c).sum(), (degree, n1)


def test_poly_split_against_a_brute_force_count():
    """Products counted by walking the evaluation itself (every baby power, y, every further giant power, every pair of the
    closing cc_dot) and levels by simulating the tree; poly_split takes the fewest products, then the smaller depth, then the
    larger n1."""
    def walk(d, n1):
        G = -(-(d + 1) // n1)
        lvl, products = {1: 0}, 0
        for b in range(2, n1):
            hi = 1 << (b.bit_length() - 1)
            lvl[b] = (lvl[hi // 2] if b == hi else max(lvl[hi], lvl[b - hi])) + 1
            products += 1
        Lb = max(lvl[b] for b in range(1, n1))
        if G == 1:
            return products, Lb + 1
        ylvl = {1: lvl[n1 // 2] + 1}
        products += 1
        for g in range(2, G):
            hi = 1 << (g.bit_length() - 1)
            ylvl[g] = (ylvl[hi // 2] if g == hi else max(ylvl[hi], ylvl[g - hi])) + 1
            products += 1
        products += G - 1
        return products, max(ylvl[G - 1], Lb + 1) + 1

    for d in range(1, 64):
        cands = []
        n1 = 2
        while n1 <= 128:
            products, depth = walk(d, n1)
            s = encdec.poly_schedule(d, n1)
            assert (s["products"], s["depth"]) == (products, depth), (d, n1)
            cands.append((products, depth, -n1))
            n1 *= 2
        assert encdec.poly_split(d) == -min(cands)[2], d
    assert [encdec.poly_split(d) for d in (1, 3, 7, 15, 31, 63)] == [2, 2, 4, 8, 8, 16]
    for bad in ((0, 2), (7, 3), (7, 1), (7.5, 4)):
        with pytest.raises(ValueError):
            encdec.poly_schedule(*bad)


def test_c_entry_refuses_bad_arguments_before_any_device_call():
    """lf_weighted_sums returns LF_ERR_ARG from its arguments alone (pointers that are never dereferenced; no call here would
    pass the checks), and the caps of the header are the ones Python mirrors."""
    from liberate_fhe_amd import _native
    from liberate_fhe_amd.fhe.backend import HipBackend
    lib = _native.lib
    LF_ERR_ARG = 10001
    dummy = ctypes.c_void_p(64)

    def ptrs(n, null_at=None):
        arr = (ctypes.c_void_p * max(n, 1))(*([64] * max(n, 1)))
        if null_at is not None:
            arr[null_at] = None
        return arr

    def call(k=3, G=2, rows=2, logN=13, ins=0, row0s=0, outs=0, tab=dummy, consts=None, scales=dummy, mods=(dummy,) * 4):
        ins = ptrs(2 * max(k, 1)) if ins == 0 else ins
        row0s = ptrs(2 * max(k, 1)) if row0s == 0 else row0s
        outs = ptrs(2 * max(G, 1)) if outs == 0 else outs
        return lib.lf_weighted_sums(ins, row0s, outs, k, G, rows, logN, tab, consts, scales, 0, *mods, 0, None)

    assert call(k=0) == LF_ERR_ARG and call(k=-1) == LF_ERR_ARG and call(k=17) == LF_ERR_ARG
    assert call(G=0) == LF_ERR_ARG and call(G=65) == LF_ERR_ARG
    assert call(tab=None) == LF_ERR_ARG and call(scales=None) == LF_ERR_ARG
    assert call(ins=None) == LF_ERR_ARG and call(row0s=None) == LF_ERR_ARG and call(outs=None) == LF_ERR_ARG
    for at in (0, 5):
        assert call(ins=ptrs(6, at)) == LF_ERR_ARG and call(row0s=ptrs(6, at)) == LF_ERR_ARG
    assert call(outs=ptrs(4, 3)) == LF_ERR_ARG
    for i in range(4):
        assert call(mods=tuple(None if j == i else dummy for j in range(4))) == LF_ERR_ARG
    assert call(logN=12) == LF_ERR_ARG and call(logN=18) == LF_ERR_ARG
    assert call(rows=-1) == LF_ERR_ARG and call(rows=lib.lf_limits(2)) == LF_ERR_ARG
    header = open(os.path.join(ROOT, "include", "ckks_hip.h")).read()
    caps = {n: int(v) for n, v in re.findall(r"#define (LF_WSUM_MAX_\w+) (\d+)", header)}
    assert caps == {"LF_WSUM_MAX_TERMS": 16, "LF_WSUM_MAX_OUTPUTS": 64}
    assert (_native.LF_WSUM_MAX_TERMS, _native.LF_WSUM_MAX_OUTPUTS) == (16, 64)
    assert (HipBackend.wsum_max_terms, HipBackend.wsum_max_outputs) == (16, 64)
    assert "lf_weighted_sums" in _native.EXPORTED and lib.lf_abi_version() == 15


def test_weighted_sums_kernels_use_no_scratch():
    """weighted_sums_kernel<1 | 2 | 4>: scratch 0, no spill, at least 4 waves per SIMD, listed in the tracked table as built."""
    import __graft_entry__ as g
    res = {r["kernel"]: r for r in g.kernel_resources()}
    names = [f"weighted_sums_kernel<{n}>" for n in (1, 2, 4)]
    assert sorted(k for k in res if k.startswith("weighted_sums_kernel")) == sorted(names)
    # the tracked table, row by row: file, kernel name (may hold blanks), then VGPR AGPR SGPR LDS scratch v-spill occ
    row = re.compile(r"^(\S+)\s+(.+?)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)$")
    tracked = {}
    for ln in open(os.path.join(ROOT, "profiles", "r06_kernel_resources.txt")):
        m = row.match(ln.rstrip())
        if m and not ln.startswith("#"):
            tracked[m.group(2)] = [int(v) for v in m.groups()[2:]]
    for k in names:
        r = res[k]
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["occupancy"] >= 4, r
        vgpr, _, _, _, scratch, _, occ = tracked[k]
        assert (vgpr, scratch, occ) == (r["vgprs"], r["scratch"], r["occupancy"]), (k, tracked[k])


def unit_error(eng, x, pk, sk, evk, level):
    """Decryption error of a ciphertext brought to `level` by the chain of squares on the input x, |x| <= 1."""
    ct, want = eng.encorypt(x, pk), x.copy()
    while ct.level < level:
        ct, want = eng.square(ct, evk), want * want
    return np.abs(eng.decrode(ct, sk).real - want).max()


def test_real_keys_decrypt_within_the_bound():
    """Real keys on the checker engine, degree 7 in both bases on messages in [-1, 1]: the error against the float64 evaluation of
    the same series on the DECODED input is at most 8 A e_unit, A the sum of the absolute host coefficients actually multiplied
    in, e_unit the decryption error of the chain of squares brought to the result's level on the same input: each product
    q_g y^g contributes at most |q_g| err(y^g) + err(q_g) |y^g| <= 2 A_g e_unit, and the factor 4 over that covers the extra
    level_ups and scalar rescales; a wrong coefficient, level or deviation gives errors many orders above.  Both are printed."""
    from liberate_fhe_amd.fhe import ckks_engine
    from tests.oracle_backend import OracleBackend
    eng = ckks_engine(devices=["cpu"], backend=OracleBackend(), **POLY)
    sk = eng.create_secret_key()
    pk, evk = eng.create_public_key(sk), eng.create_evk(sk)
    rng = np.random.default_rng(21)
    x = rng.uniform(-1, 1, eng.num_slots)
    ct = eng.encorypt(x, pk)
    x_dec = eng.decrode(ct, sk).real
    coeffs = rng.uniform(-1, 1, 8)
    for basis in ("power", "chebyshev"):
        got = eng.poly_eval(ct, coeffs, evk, basis=basis)
        n1 = encdec.poly_split(7)
        blocks = encdec.cheb_blocks(coeffs, n1) if basis == "chebyshev" else coeffs.reshape(-1, n1)
        A = np.abs(blocks).sum()
        want = C.chebval(x_dec, coeffs) if basis == "chebyshev" else np.polynomial.polynomial.polyval(x_dec, coeffs)
        err = np.abs(eng.decrode(got, sk).real - want).max()
        e_unit = unit_error(eng, x, pk, sk, evk, got.level)
        print(f"logN 13, degree 7, {basis}: max abs error {err:.3e}, A = {A:.3f}, e_unit {e_unit:.3e}, bound {8 * A * e_unit:.3e}")
        assert got.level == eng.poly_depth(7, basis) and err <= 8 * A * e_unit, (basis, err, A, e_unit)
