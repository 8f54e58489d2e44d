"""The checker (tests/oracle_backend.OracleBackend, the word-exact reference of tests/test_engine_edges_gpu.py) pinned at
the operands of that file: every coefficient-wise step — rescale, tensor, digits (with and without a Galois map),
extension, inner product, mod-down — against its DEFINITION in Python integers, exact congruences, on the parameter sets
and levels of the GPU file; the range of every output word; and that each operand pattern reaches what it is for.

The steps act coefficient by coefficient, so the rows here are 2^8 words long (the tables of an engine do not depend on N)."""
import warnings

import numpy as np
import pytest
import torch

from tests.helpers import (DIGIT_WORD_BOUND, ENGINE_EDGE_PATTERNS, R, SMALL_PRIME_LIMIT, StepTables, edge_ciphertext, edge_key,
                           edge_param_sets, edge_rows, pre_rescale, pre_rescale_rows, rounder_row0, step_operands, thue_morse)

warnings.filterwarnings("ignore", category=UserWarning)
NS = 1 << 8
SETS = edge_param_sets()
PATTERNS = ("top", "top|0", "half", "mixed", "random")
_ENGINES = {}


def checker(name):
    if name not in _ENGINES:
        from liberate_fhe_amd.fhe import ckks_engine
        from tests.oracle_backend import OracleBackend
        _ENGINES[name] = ckks_engine(devices=["cpu"], backend=OracleBackend(), **SETS[name])
    return _ENGINES[name]


def edge_levels(eng):
    """Level 0, the last level that still has a multiplication, the last level."""
    return (0, eng.num_levels - 2, eng.num_levels - 1)


def ints(a):
    return [[int(v) for v in row] for row in np.asarray(a)]


def crt(residues, moduli):
    x, M = 0, 1
    for r, m in zip(residues, moduli):
        x += M * ((r - x) * pow(M, -1, m) % m)
        M *= m
    return x, M


def test_edge_rows_patterns():
    q = [(1 << 41) - 65535, 1099511922689, 97, 1152921504606830593]
    tm = thue_morse(NS)
    for lazy in (False, True):
        top = [(2 if lazy else 1) * x - 1 for x in q]
        assert all((edge_rows(q, NS, "top", lazy=lazy)[i] == top[i]).all() for i in range(4))
        w = edge_rows(q, NS, "top|0", lazy=lazy)
        assert all((w[i] == np.where(tm == 1, 0, top[i])).all() for i in range(4))
        w = edge_rows(q, NS, "top|1", lazy=lazy)
        assert all((w[i] == np.where(tm == 1, 1, top[i])).all() for i in range(4))
        w = edge_rows(q, NS, "random", 3, lazy=lazy)
        assert all(0 <= w[i].min() and w[i].max() <= top[i] for i in range(4))
    w = edge_rows(q, NS, "half")
    assert all(set(w[i].tolist()) == {q[i] // 2, q[i] // 2 + 1} and w[i][0] == q[i] // 2 for i in range(4))
    m = edge_rows(q, NS, "mixed")
    assert [(m[i] == edge_rows(q[i:i + 1], NS, p)[0]).all() for i, p in enumerate(("top", "top|0", "half", "top|1"))] == [True] * 4
    # a row's words follow its id, not its position (two devices hold the words one device holds)
    assert (edge_rows(q[2:], NS, "mixed", ids=[2, 3]) == m[2:]).all()
    assert (edge_rows(q[2:], NS, "random", 5, ids=[2, 3]) == edge_rows(q, NS, "random", 5)[2:]).all()
    r0 = rounder_row0(q[0], NS)
    at = q[0] // 2
    for lane in (0, 1):
        assert set(r0[lane::2].tolist()) == {0, at - 1, at, at + 1, q[0] - 1}


@pytest.mark.parametrize("name", sorted(SETS))
def test_pre_rescale_round_trip_and_the_negative_word(name):
    """pre_rescale builds the operand of a rescale backwards from the wanted result.  On the checker the round trip is a
    congruence everywhere and word-exact except where a_i - r is negative and the target sits right below q_i: at the target q_i - 1 under a firing
    rounder the signed REDC returns -2, the rounder adds 1 and reduce_2q only ever subtracts, so the reference's rescale
    leaves the word -1 (no uniform input of the 40-bit sets produces a negative word).  rescale_kernel has to return that
    word too, and every consumer has to take it."""
    eng = checker(name)
    be = eng.backend
    seen_negative = False
    for level in (0, eng.num_levels - 2):
        nxt = level + 1
        T = StepTables(eng, nxt)
        q_drop = int(eng.ctx.q[level])
        row0 = rounder_row0(q_drop, NS)
        for pattern in PATTERNS:
            target = edge_rows(T.q_ord, NS, pattern, 7, ids=T.ids_ord)
            src = pre_rescale_rows(T.q_ord, q_drop, target, row0)
            assert ((src >= 0) & (src < np.array(T.q_ord)[:, None])).all()
            out = torch.full((T.ell, NS), -7, dtype=torch.int64)
            be.rescale(torch.from_numpy(src), torch.from_numpy(row0), out, T.ell, eng.rescale_scales[level][0], q_drop // 2, T.c_ord)
            out = out.numpy()
            qv = np.array(T.q_ord)[:, None]
            rho = (row0 > q_drop // 2)[None, :]
            # the definition, in Python integers: (a - r) q_drop^-1 + rho
            for i, q in enumerate(T.q_ord):
                inv = pow(q_drop, -1, q)
                want = [((int(a) - int(r)) * inv + int(h)) % q for a, r, h in zip(src[i], row0, rho[0])]
                assert [int(v) % q for v in out[i]] == want == [int(t) % q for t in target[i]]
            neg = out < 0
            # A negative word: where a_i - r is negative the signed REDC of (a_i - r) * scale lies in (x, x + q_i) with
            # x = (a_i - r) scale / R > -q_drop q_i / R, so a residue within that distance of q_i comes out as residue - q_i;
            # the rounder adds at most 1 and reduce_2q only ever subtracts.  With 40-bit primes x > -2^18 and a uniform
            # input meets such a word with probability 2^-22; the targets q_i - 1 meet it at every large dropped word (-1).
            slack = np.array([(q_drop * q) >> 62 for q in T.q_ord])[:, None] + 1
            assert (out < qv).all() and (out >= -slack).all()
            assert not (neg & ~(src - row0[None, :] < 0)).any() and (out[neg] == (target - qv)[neg]).all()
            if SETS[name]["scale_bits"] == 40:       # the 40-bit sets: only -1, only at target q_i - 1 under a firing rounder
                # (.. or, without the rounder, on a limb so far below the dropped prime that x = (q_i - q_drop) scale / R, the
                # a_i - r of the target q_i - 1, is itself below -1: only the deep set's 31 scale primes spread that far)
                scale = [int(s) for s in eng.rescale_scales[level][0]]
                assert len(scale) == T.ell
                below = np.array([(q - q_drop) * s < -(1 << 62) for q, s in zip(T.q_ord, scale)])[:, None]
                assert not below.any() or name == "sb40_K1_d32"
                assert (out[neg] == -1).all() and not (neg & ~((target == qv - 1) & (rho | below))).any()
            assert (out[~neg] == target[~neg]).all()
            seen_negative |= bool(neg.any())
    assert seen_negative == (SETS[name]["scale_bits"] >= 40)


def test_pre_rescale_follows_the_engine_layout():
    """pre_rescale / pre_rescale_ciphertext on one and on two devices: the checker engine's own rescale of the result is
    the wanted ciphertext (mod q), the dropped limb carries the rounder pattern."""
    from liberate_fhe_amd.fhe import ckks_engine
    from tests.helpers import pre_rescale_ciphertext
    from tests.oracle_backend import OracleBackend
    for n_dev in (1, 2):
        eng = ckks_engine(devices=["cpu"] * n_dev, backend=OracleBackend(), **SETS["sb41_K2"])
        for level in (0, 3):
            ct = pre_rescale_ciphertext(eng, level, "mixed", 5)
            want = edge_ciphertext(eng, level + 1, "mixed", 5)
            got = eng.rescale(ct)
            dest = eng.ntt.p.destination_arrays[level + 1]
            for comp in range(2):
                for i, (g, w) in enumerate(zip(got.data[comp], want.data[comp])):
                    qv = torch.tensor([eng.ctx.q[j] for j in dest[i]])[:, None]
                    assert torch.equal(g % qv, w) and bool((g >= -1).all())


def _digits_definition(T, a, state, tag):
    """Every digit's mixed-radix words y: the integer X = y_0 + m_0 y_1 + m_0 m_1 y_2 + .. is congruent to the digit's
    residues modulo each of its primes, i.e. X = CRT + k prod(m); the reference's lazy REDC leaves y_i in
    (-2^24, m_i + 2^24), so k is 0 or 1 up to that slack; returned: (X per digit and column, largest |y| per digit)."""
    X, top = [], []
    for rows, m in T.order:
        Pd = 1
        for v in m:
            Pd *= v
        cols, big = [], 0
        for j in range(a.shape[1]):
            y = [int(state[r][j]) for r in rows]
            x, L = 0, 1
            for yi, mi in zip(y, m):
                x += L * yi
                L *= mi
            want, _ = crt([int(a[r][j]) for r in rows], m)
            assert (x - want) % Pd == 0, tag
            assert -1 <= (x - want) // Pd <= 1, (tag, (x - want) // Pd)
            assert 0 <= y[0] < m[0] and all(-(1 << 24) < yi < mi + (1 << 24) for yi, mi in zip(y[1:], m[1:])), tag
            big = max(big, max(abs(v) for v in y))
            cols.append(x)
        X.append(cols)
        top.append(big)
    return X, top


@pytest.mark.parametrize("name", sorted(SETS))
def test_checker_steps_equal_their_definitions(name):
    """tensor, digits (plain and under X -> X^5), extension, inner product and mod-down of the checker against Python
    integers, at the three edge levels, every data pattern; keys at 2q - 1 ("top") for the data patterns "top" and "mixed"
    and uniform lazy words for the others (the key pattern only enters the inner product)."""
    eng = checker(name)
    be = eng.backend
    for level in edge_levels(eng):
        T = StepTables(eng, level)
        ell, rows, K = T.ell, T.rows, T.K
        for pattern in PATTERNS:
            kpat = "top" if pattern in ("top", "mixed") else "random"
            tag = f"{name} level {level} {pattern}/{kpat}"
            op = step_operands(T, pattern, kpat, 11 + level, N=NS)
            t = {k: torch.from_numpy(v) for k, v in op.items()}
            # ---- tensor product: d0 = x0 y0 / R, d1 = (x0 y1 + x1 y0) / R, d2 = x1 y1 / R, lazy words ----
            d = torch.full((3, ell, NS), -7, dtype=torch.int64)
            be.tensor(t["x"][0], t["x"][1], t["x"][2], t["x"][3], d[0], d[1], d[2], ell, T.c_ord)
            x = [ints(v) for v in op["x"]]
            for i, q in enumerate(T.q_ord):
                Ri = pow(R, -1, q)
                assert 0 <= int(d[:, i].min()) and int(d[:, i].max()) < 2 * q, tag
                for j in range(NS):
                    x0, x1, y0, y1 = (x[k][i][j] for k in range(4))
                    assert [int(d[k, i, j]) % q for k in range(3)] == [x0 * y0 * Ri % q, (x0 * y1 + x1 * y0) * Ri % q, x1 * y1 * Ri % q], tag
            # ---- digits ----
            st = torch.full((ell, NS), -7, dtype=torch.int64)
            be.ks_digits(t["a"], st, T.n_digits, T.d_desc, T.d_tab, T.c_ord)
            X, top = _digits_definition(T, op["a"], st.numpy(), tag)
            if pattern in ("top", "mixed"):
                # reaches its range: the largest word of every digit lies in the upper half of a residue range.  ("top" is the
                # integer prod(m) - 1, whose words are all m_i - 1 — which the signed REDC leaves as -1 behind the first.)
                # (The 2^43 / 2^44 of the kernel comments leave room no canonical input fills: words AT that bound go
                # through the extension directly, `state_hi` below.)
                for (rws, m), big in zip(T.order, top):
                    assert big >= min(m) // 2, (tag, big, m)
            # under a Galois map: the digits of a(X^5), canonical (make_unsigned + reduce_2q)
            stg = torch.full((ell, NS), -7, dtype=torch.int64)
            be.ks_digits(t["a"], stg, T.n_digits, T.d_desc, T.d_tab, T.c_ord, galois=(pow(5, -1, 2 * NS), T.q2_ord))
            ag = np.empty_like(op["a"])
            n = np.arange(NS)
            pos = (5 * n) % (2 * NS)
            qv = np.array(T.q_ord)[:, None]
            ag[:, pos % NS] = np.where(pos[None, :] >= NS, (qv - op["a"]) % qv, op["a"])
            _digits_definition(T, ag, stg.numpy(), tag + " galois")
            # ---- extension: ext[p][r] = X_p R mod q_r, lazy; also from digit words at the documented bound ----
            for which, state in (("digits", st), ("bound", t["state_hi"])):
                ext = torch.full((T.nparts, rows, NS), -7, dtype=torch.int64)
                be.ks_extend(state, ext, T.nparts, rows, T.e_desc, T.E, T.c_all)
                if which == "bound":
                    Xs = []
                    for rws, m in T.order:
                        L, acc = 1, [0] * NS
                        for r, mi in zip(rws, m):
                            acc = [v + L * int(w) for v, w in zip(acc, op["state_hi"][r])]
                            L *= mi
                        Xs.append(acc)
                else:
                    Xs = X
                for p in range(T.nparts):
                    for r, q in enumerate(T.q_all):
                        row = ext[p, r]
                        if which == "digits":      # (signed words at the bound leave signed lazy words: residues only)
                            assert 0 <= int(row.min()) and int(row.max()) < 2 * q, (tag, which)
                        assert [int(v) % q for v in row] == [v * R % q for v in Xs[p]], (tag, which, p, r)
            # ---- inner product: s_c[r] = sum_p ext[p][r] key[first + p][c][r] / R, lazy ----
            s = torch.full((2, rows, NS), -7, dtype=torch.int64)
            be.ks_inner(t["ext"], t["key"], T.first_part, T.row_off, s[0], s[1], T.nparts, rows, T.c_all)
            for r, q in enumerate(T.q_all):
                Ri = pow(R, -1, q)
                e = [ints(op["ext"][p, r:r + 1])[0] for p in range(T.nparts)]
                for c in range(2):
                    k = [ints(op["key"][T.first_part + p, c, T.row_off + r:T.row_off + r + 1])[0] for p in range(T.nparts)]
                    want = [sum(e[p][j] * k[p][j] for p in range(T.nparts)) * Ri % q for j in range(NS)]
                    assert 0 <= int(s[c, r].min()) and int(s[c, r].max()) < 2 * q, tag
                    assert [int(v) % q for v in s[c, r]] == want, (tag, r, c)
            if pattern == "top":      # the decisive product: a lazy data word 2q - 1 against a lazy key word 2q - 1
                assert all(int(op["ext"][0, r, 0]) == 2 * q - 1 == int(op["key"][T.first_part, 0, T.row_off + r, 0])
                           for r, q in enumerate(T.q_all))
            # ---- mod-down: out = (s - [s]_P) / P (+ addend), canonical; [s]_P = the CRT value of the special rows + k P ----
            specials = T.q_all[ell:]
            Pm = 1
            for v in specials:
                Pm *= v
            for add in (None, t["add"][0]):
                out = torch.full((ell, NS), -7, dtype=torch.int64)
                be.ks_moddown(t["s"][0], out, add, ell, K, T.pir, T.Rs_all, T.c_all)
                for j in range(NS):
                    rep, _ = crt([int(op["s"][0, ell + i, j]) for i in range(K)], specials)
                    fits = []
                    for k in (-1, 0, 1):
                        fits.append(all(int(out[i, j]) == ((int(op["s"][0, i, j]) - rep - k * Pm) * pow(Pm, -1, q)
                                                           + (0 if add is None else int(add[i, j]))) % q
                                        for i, q in enumerate(T.q_ord)))
                    assert any(fits), (tag, j)
            if pattern == "top":      # every pivot of the elimination is q_special - 1: the special rows are the integer P - 1
                rep, _ = crt([int(op["s"][0, ell + i, 0]) for i in range(K)], specials)
                assert rep == Pm - 1
                digits, v = [], rep
                for m in reversed(specials):     # the chain eliminates the last special row first
                    digits.append(v % m)
                    v //= m
                assert digits == [m - 1 for m in reversed(specials)]


def test_state_at_the_documented_bound():
    T = StepTables(checker("sb40_K8"), 0)
    hi = step_operands(T, "top", "top", 0, N=NS)["state_hi"]
    assert int(np.abs(hi[:8]).max()) == DIGIT_WORD_BOUND == (1 << 43) - 1 and all(q < SMALL_PRIME_LIMIT for q in T.q_ord[:8])
    assert int(hi[9].max()) == 2 * T.q_ord[9] - 1 and int(hi[9].min()) == -(2 * T.q_ord[9] - 1)


@pytest.mark.parametrize("name", sorted(SETS))
def test_the_reference_composition_runs_every_listed_set(name):
    """No listed parameter set is dropped: the checker engine runs cc_mult + rotate + rescale on edge operands at each."""
    from tests.helpers import pre_rescale_ciphertext
    eng = checker(name)
    evk, rotk = edge_key(eng, "top", 1), edge_key(eng, "random", 2, origin="rotation key:3")
    a, b = pre_rescale_ciphertext(eng, 0, "mixed", 3), pre_rescale_ciphertext(eng, 0, "top", 4)
    prod = eng.cc_mult(a, b, evk)
    rot = eng.rotate_single(prod, rotk)
    assert prod.level == 1 and rot.level == 1 and eng.rescale(rot).level == 2
    assert any(bool(t.count_nonzero()) for t in prod.data[0])       # not the all-zero product of operands that rescale to 0
