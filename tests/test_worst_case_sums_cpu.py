"""The yardstick of tests/test_worst_case_sums_gpu.py, without a GPU and without the code under test: the operands of that file
(tests/helpers.py: constant_ciphertext, extended_constants, extreme_key) DO meet the conditions its docstring states — every
product of the fp64-class inner sums is +-(q - 1) / 2, the rotation sums pass 64 q, everything stays below 2^52 — computed in
Python integers from the words of the operands; and the checker engine's results on them equal the compositions of public steps
(tests/test_inner_sum_cpu.py, tests/test_linear_transform_cpu.py).  These are conditions on the inputs, not measurements.

Which residue a kernel multiplies (read in the sources):
  * csrc/ckks_ks.hip:138, 154 (ks_ext_pass1): an fp64-class row is extended with the PLAIN table Ed — sum of dp_mulmod_bal(digit
    word, Ed) — transformed, and stored as its canonical residue dp_reduce(.., q): the word x the inner products read is the plain
    residue e R^-1 mod q in [0, q) of the checker's Montgomery-form word e.
  * csrc/ckks_ks.hip:1574 (ks_inner_rsum_kernel; 1046 hoist, 1168 lt, 1377 ltb, 1744 rsumb, 1870 baby, 2319 babyb: the same line):
    acc += dp_mulmod_bal(x, k) with k the Montgomery-form key word as it is stored (below 2q; its canonical residue where the key is
    read from the planes format): the balanced residue of x k = e k R^-1, which is the checker's mont_mult(e, k).  So the model of
    the issue — key word t R e^-1 gives the residue t — holds with no per-row factor.
  * csrc/ckks_ntt_core.h:194 (dp_mulmod_bal): the balanced representative is x k - rint(fl(x k) fl(1 / q)) q.  At t = +-(q - 1) / 2
    the exact quotient is 1 / (2q) > 2^-42 away from a half-integer, and the fp64 quotient's error is about 2^-52 x k / q: with
    extended digits of 40 bits the rint would fall to either side, word by word, and the sums would be pseudo-random after all.
    What is folded into the operands for this: constant_ciphertext keeps component 1 at 1 .. 4, so that x is 1 .. 4 (digits of one
    limb extend to the same small integer on every row), x k < 2^45 is exact and the quotient is off by 2^-50 at most.
    fp64_balanced_product below is that function in IEEE doubles and must give +-(q - 1) / 2 itself."""
import functools
import warnings

import numpy as np
import pytest
import torch

from tests import test_worst_case_sums_gpu as G
from tests.helpers import R, SMALL_PRIME_LIMIT, constant_ciphertext, edge_diagonals, extended_constants, thue_morse
from tests.test_accumulating_ops_edges_cpu import checker, same
from tests.test_inner_sum_cpu import composition as rsum_composition
from tests.test_linear_transform_cpu import composition as lt_composition

warnings.filterwarnings("ignore", category=UserWarning)
D = 0


@functools.lru_cache(maxsize=None)
def setup():
    eng = checker(G.DEEP)
    constants = extended_constants(eng, constant_ciphertext(eng, 0, 0))
    return eng, constants, G.extreme_keys(eng, constants), G.extreme_keys(eng, constants, flip=True)


def fp64_balanced_product(x, k, q):
    """dp_mulmod_bal (csrc/ckks_ntt_core.h:194) for x k < 2^53: hi = x k exactly, lo = 0, quo = rint(hi * fl(1 / q)) in IEEE
    doubles (Python's floats; round() is rint's round-half-even), result hi - quo q, exact"""
    assert 0 <= x * k < 1 << 53
    quo = round(float(x * k) * (1.0 / float(q)))
    return x * k - quo * q


def gathered_constants(eng, ct):
    """[component][ordinary row] the constant word of c^ = P enter_ntt(c) (Montgomery form, below 2q), formed as the compositions
    form it: what the kernels gather (component 0) and add as the self term (both)"""
    level = ct.level
    ell, logN = eng._rows(D, level, False), eng.ctx.logN
    out = []
    for comp in range(2):
        x = torch.empty_like(ct.data[comp][0])
        eng.backend.galois(ct.data[comp][0].contiguous(), x, ell, logN, 1, eng._vec("_2q", D, level, False))
        eng.ntt.enter_ntt([x], level, D, -1)
        eng.ntt.mont_enter_scalar([x], [eng._PR(D, level)], level, D, -1)
        assert bool((x == x[:, :1]).all())
        out.append([int(v) for v in x[:, 0]])
    return out


class Model:
    """Per fp64-class row of `level` and per component and parity of the coefficient index, in Python integers: the products of
    the extreme ciphertext's digits with the key's words, and from them what each kernel holds before its one reduction."""

    def __init__(self, level, flip=False, seed=0):
        eng, constants0, keys, flipped = setup()
        self.eng, self.level = eng, level
        q = eng.ctx.q
        ids0 = list(eng.ntt.p.destination_arrays_with_special[0][D])
        ids = list(eng.ntt.p.destination_arrays_with_special[level][D])
        ell = eng._rows(D, level, False)
        ct = constant_ciphertext(eng, level, seed)
        e = extended_constants(eng, ct)
        gids = eng.parts_alloc[level][D]
        self.nparts = len(e)
        assert self.nparts == len(eng._ks_tables(level)["order"]) == len(gids) and len(ids) - ell == 1
        if seed == 0:          # the rows and parts of a later level are a sub-block of level 0's: one key serves both
            assert all(e[p][r] == constants0[gid][ids0.index(i)] for p, gid in enumerate(gids) for r, i in enumerate(ids))
        key = (flipped if flip else keys)[1]
        chat = gathered_constants(eng, ct)
        par = thue_morse(eng.ctx.N)
        j = [int(np.flatnonzero(par == 0)[1]), int(np.flatnonzero(par == 1)[1])]      # an index of each parity (not index 0)
        par = torch.from_numpy(par)
        self.rows = []
        for r, i in enumerate(ids):
            m = int(q[i])
            if m >= SMALL_PRIME_LIMIT:
                continue
            assert r < ell                                                  # (every fp64-class row is an ordinary one)
            r0 = ids0.index(i)
            prods = [[[], []], [[], []]]                                    # [component][parity] -> one product per part
            for p, gid in enumerate(gids):
                x = e[p][r] * pow(R, -1, m) % m                             # the plain word the kernel reads
                assert 1 <= x <= 4, (level, p, r, x)
                for comp in range(2):
                    words = key.data[gid].data[comp][0][r0]
                    assert bool((words[par == 0] == words[j[0]]).all()) and bool((words[par == 1] == words[j[1]]).all())
                    for h in range(2):
                        k = int(words[j[h]])
                        assert 0 <= k < 2 * m and (k >= m) == bool(r0 % 2)   # the lazy representative on odd rows
                        t = e[p][r] * k * pow(R, -1, m) % m                  # the residue of the checker's mont_mult
                        t = t if t <= m // 2 else t - m
                        for kk in (k, k % m):                               # the stored word and its canonical residue
                            assert fp64_balanced_product(x, kk, m) == t, (level, p, r, comp, h)
                        prods[comp][h].append(t)
            self.rows.append({"q": m, "prods": prods, "chat": [chat[0][r], chat[1][r]]})

    def sums(self, row, keys, gathered=0, self_term=False, start=None):
        """[component][parity]: `keys` keys' products over all parts, `gathered` words of c^0 in component 0, the self term, the
        canonical pair a previous launch left"""
        out = [[0, 0], [0, 0]]
        for comp in range(2):
            for h in range(2):
                v = keys * sum(row["prods"][comp][h])
                if comp == 0:
                    v += gathered * row["chat"][0]
                if self_term:
                    v += row["chat"][comp]
                if start is not None:
                    v += start[comp][h]
                out[comp][h] = v
        return out


@pytest.mark.parametrize("level", G.LEVELS)
def test_every_product_is_at_the_end_of_the_balanced_range(level):
    """+-(q - 1) / 2, exactly, in the integers and in the kernels' fp64 quotient (asserted while the model is built), one sign
    along a whole sum, both signs on every row; under the flipped key the signs trade places; and a ciphertext of other constants
    does NOT see such products under these keys (member 0 of the batches is the extreme one)."""
    nparts = {0: 32, 1: 31}[level]
    for flip in (False, True):
        M = Model(level, flip)
        assert M.nparts == nparts and len(M.rows) == nparts - 1          # (the base prime's row is integer-class)
        for row in M.rows:
            top = (row["q"] - 1) // 2
            for comp in range(2):
                for h in range(2):
                    sign = -1 if (comp + h + flip) % 2 else 1
                    assert row["prods"][comp][h] == [sign * top] * nparts
            assert {p for c in row["prods"] for h in c for p in h} == {top, -top}
            assert row["chat"][0] % row["q"] == row["q"] - 1 and 0 <= row["chat"][0] < 2 * row["q"]       # P c0: the top of its range
    eng, constants, _, _ = setup()
    for seed in (1, 2, 3):
        other = extended_constants(eng, constant_ciphertext(eng, 0, seed))
        assert all(a != b for ra, rb in zip(other, constants) for a, b in zip(ra, rb))
    assert [extended_constants(eng, ct) == constants for ct in G.batch_of(eng, 0)] == [True, False, False, False]
    assert [extended_constants(eng, ct) == constants for ct in G.batch_of(eng, 0, last=True)] == [False, False, False, True]


def test_the_deep_set_is_what_the_gpu_file_says():
    """32 digits of one limb at level 0, 31 at level 1, 33 rows of which 31 are fp64-class; inside LF_FP64_MAX_DIGITS, which no
    engine reaches: the context's prime list runs out first."""
    import os
    import re
    eng = setup()[0]
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ckks_hip.h")).read()
    bound = int(re.search(r"#define LF_FP64_MAX_DIGITS (\d+)", header).group(1))
    ids = eng.ntt.p.destination_arrays_with_special[0][D]
    assert len(ids) == 33 and sum(int(eng.ctx.q[i]) < SMALL_PRIME_LIMIT for i in ids) == 31
    for level in G.LEVELS:
        order = eng._ks_tables(level)["order"]
        assert len(order) == 32 - level <= bound and all(len(rows) == 1 for _, rows, _ in order)
    assert bound == 119


@pytest.mark.parametrize("level", G.LEVELS)
def test_the_accumulators_are_where_the_range_arguments_put_them(level):
    """What each kernel holds before its one reduction, per fp64-class row, for both parities (csrc/ckks_ks.hip: the table above
    lf_fp64_digits_ok)."""
    M = Model(level)
    n = M.nparts
    limit = 1 << 52
    for row in M.rows:
        q = row["q"]
        # ks_inner_rsum_kernel, 4 keys and the self term in one launch: n NR products, NR gathered words, the self term
        acc = M.sums(row, 4, gathered=4, self_term=True)
        assert acc[0][0] > 2 * n * q and acc[1][1] > 2 * n * q - 4 * (n + 1)
        if level == 0:
            assert acc[0][0] > 64 * q and acc[1][1] > 63 * q
        assert acc[0][1] < -(2 * n - 11) * q and acc[1][0] < -(2 * n - 3) * q
        assert all(abs(v) < limit for c in acc for v in c)
        # .. five keys: the launch of 4 leaves canonical words, the launch of 1 starts from them
        left = [[v % q for v in c] for c in M.sums(row, 4, gathered=4, self_term=True)]
        acc = M.sums(row, 1, gathered=1, start=left)
        assert all(abs(v) < limit for c in acc for v in c) and acc[0][0] >= n * (q - 1) // 2
        # ks_inner_rsumb_kernel, 8 keys in one launch: 8 n products, 8 gathered words, the self term
        acc = M.sums(row, 8, gathered=8, self_term=True)
        assert acc[0][0] > (4 * n - 1) * q and acc[1][1] > (4 * n - 1) * q
        if level == 0:
            assert acc[0][0] > 127 * q
        assert all(abs(v) < limit for c in acc for v in c)
        # .. nine keys: the second launch (one key) starts from the canonical pair
        left = [[v % q for v in c] for c in acc]
        assert all(abs(v) < limit for c in M.sums(row, 1, gathered=1, start=left) for v in c)
        # the kernels that reduce with dp_reduce alone: ks_inner_hoist_kernel (nothing joins), ks_inner_baby_kernel /
        # ks_inner_babyb_kernel and the per-key sums of ks_inner_lt_kernel / ks_inner_ltb_kernel before their dp_reduce_bal
        # (one gathered word joins component 0)
        for acc in (M.sums(row, 1), M.sums(row, 1, gathered=1)):
            assert acc[0][0] * 2 >= (n - 2) * q and acc[1][1] * 2 >= (n - 2) * q          # at least (nparts / 2 - 1) q
            assert all(abs(v) < 64 * q for c in acc for v in c)


@pytest.mark.parametrize("level", G.LEVELS)
def test_checker_results_equal_the_compositions_on_these_operands(level):
    """rotate_sum with 4 keys and the self term, with 5 keys and without it, and the flat linear_transform of the GPU file: the
    checker engine's words are those of the compositions of public steps."""
    eng, _, keys, flipped = setup()
    ct = constant_ciphertext(eng, level, 0)
    for ks, with_self in (([keys[s] for s in G.KEY_STEPS[:4]], True), ([keys[s] for s in G.KEY_STEPS[:5]], False),
                          ([flipped[s] for s in G.KEY_STEPS[:4]], True)):
        got = eng.rotate_sum(ct, ks, include_self=with_self)
        assert got.level == level
        same(got, rsum_composition(eng, ct, ks, with_self), f"level {level} rotate_sum {len(ks)} keys self {with_self}")
    diags = edge_diagonals(eng, level, G.FLAT_STEPS, "top", 7 + level)
    got = eng.linear_transform(ct, diags, keys)
    assert got.level == level + 1
    same(got, lt_composition(eng, ct, diags, keys), f"level {level} flat linear_transform")
