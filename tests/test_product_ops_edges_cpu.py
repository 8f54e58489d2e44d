"""The yardstick of tests/test_product_ops_edges_gpu.py, without a GPU: the edge plaintexts hold what their patterns say in the
layout of encode_plain; the checker engine's pc_dot, pc_matmul, pc_matmul_batch, weighted_sums, cc_dot_batch, cc_matmul and
poly_eval, ON THE OPERANDS OF THAT FILE, equal the compositions of public steps that define their words (tests/test_pc_dot_cpu.py,
tests/test_poly_eval_cpu.py, cc_dot of every output's pairs, the loop of pc_matmul); the product with the identity plaintext and
the weighted sum of weight 1 are exactly rescale, on every configuration; and every parameter set, level and shape that file uses
stays inside the ranges the kernels and the C entries document."""
import os
import re
import warnings

import numpy as np
import pytest
import torch

from liberate_fhe_amd.fhe import encdec
from liberate_fhe_amd.fhe.presets import types
from tests import test_product_ops_edges_gpu as G
from tests.helpers import (PLAINTEXT_EDGE_PATTERNS, R, SMALL_PRIME_LIMIT, edge_plaintext, identity_plaintext, pre_rescale_ciphertext,
                           thue_morse)
from tests.test_accumulating_ops_edges_cpu import checker, launch_groups, same
from tests.test_pc_dot_cpu import composition as pc_composition
from tests.test_poly_eval_cpu import poly_composition

warnings.filterwarnings("ignore", category=UserWarning)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PINNED = ["sb40_K1", "sb41_K2"]             # ten digits of one limb; both arithmetic classes row by row
A = G.A


def by_prime(eng, level, pt):
    """prime id -> the [N] words of a plaintext, over every device"""
    out = {}
    dest = eng.ntt.p.destination_arrays[level]
    assert len(pt.data) == len([d for d in range(eng.ntt.num_devices) if d < len(dest)])
    for d, t in enumerate(pt.data):
        assert t.shape == (len(dest[d]), eng.ctx.N) and t.dtype == torch.int64 and t.is_contiguous()
        for r, i in enumerate(dest[d]):
            assert i not in out
            out[i] = t[r].numpy()
    return out


@pytest.mark.parametrize("level", [0, 4])
def test_edge_plaintexts_hold_their_patterns_in_the_layout_of_encode_plain(level):
    eng, two = checker("sb41_K2"), checker("sb41_K2", 2)
    q, N = eng.ctx.q, eng.ctx.N
    ids = eng.ntt.p.destination_arrays[level][0]
    assert {int(q[i]) < SMALL_PRIME_LIMIT for i in ids} == {True, False}
    tm, odd = thue_morse(N), np.arange(N) & 1
    want = {"top": lambda m: np.full(N, 2 * m - 1), "top|0": lambda m: np.where(tm == 1, 0, 2 * m - 1),
            "top|1": lambda m: np.where(tm == 1, 1, 2 * m - 1), "half": lambda m: m // 2 + odd, "q|0": lambda m: np.where(tm == 1, 0, m)}
    rotation = ("top", "top|0", "half", "top|1")
    assert set(PLAINTEXT_EDGE_PATTERNS) == set(want) | {"mixed", "random"}
    message = np.ones(eng.num_slots)
    for kind in ("mult", "add"):
        lvl = level if kind == "mult" else level + 1                    # (the bias of a pc_dot of level-`level` operands)
        ref = eng.encode_plain(message, lvl, kind)
        rows = eng.ntt.p.destination_arrays[lvl][0]
        for pattern in PLAINTEXT_EDGE_PATTERNS:
            pt = edge_plaintext(eng, lvl, pattern, 3, kind)
            assert (pt.origin, pt.level, pt.include_special, pt.ntt_state, pt.montgomery_state, pt.hash, pt.version) == \
                   (ref.origin, ref.level, ref.include_special, ref.ntt_state, ref.montgomery_state, ref.hash, ref.version)
            assert type(pt.data) is type(ref.data) and len(pt.data) == len(ref.data) == 1
            assert pt.data[0].shape == ref.data[0].shape and pt.data[0].dtype == ref.data[0].dtype
            eng._check_plain(pt, kind)                                  # (the engine's own check of an encoded plaintext)
            words = by_prime(eng, lvl, pt)
            assert sorted(words) == sorted(rows)
            for i, w in words.items():
                m = int(q[i])
                assert w.min() >= 0 and w.max() < 2 * m
                if pattern == "random":
                    assert w.max() >= m and len(np.unique(w)) > N // 2                       # lazy words, not a constant
                    other = by_prime(eng, lvl, edge_plaintext(eng, lvl, pattern, 4, kind))[i]
                    assert not (w == other).all()                                             # the seed counts
                else:
                    pat = rotation[i % 4] if pattern == "mixed" else pattern
                    assert (w == want[pat](m)).all(), (kind, pattern, i)
            if pattern == "q|0":
                assert all(set(np.unique(w).tolist()) == {0, int(q[i])} for i, w in words.items())
            # two devices hold the words one device holds, each prime on the device that owns it
            pt2 = edge_plaintext(two, lvl, pattern, 3, kind)
            ref2 = two.encode_plain(message, lvl, kind)
            assert pt2.origin == pt.origin and len(pt2.data) == len(ref2.data) and \
                all(a.shape == b.shape for a, b in zip(pt2.data, ref2.data))
            words2 = by_prime(two, lvl, pt2)
            assert sorted(words2) == sorted(words) and all((words[i] == words2[i]).all() for i in words)
    if level == 0:
        assert len(edge_plaintext(two, 0, "top").data) == 2                                   # (level 0 does live on both devices)
    # the identity: R mod q_i on every word of row i, a "mult" plaintext
    for e in (eng, two):
        one = identity_plaintext(e, level)
        ref = e.encode_plain(message, level)
        assert (one.origin, one.level, one.ntt_state, one.montgomery_state, one.include_special, one.hash) == \
               (ref.origin, ref.level, True, True, False, ref.hash) and one.origin == types.origins["pt_mult"]
        assert all((w == R % int(q[i])).all() for i, w in by_prime(e, level, one).items())


def levels(eng, last):
    return A.levels_of(eng)[last]


@pytest.mark.parametrize("last", [0, 1], ids=G.LEVEL_IDS)
@pytest.mark.parametrize("name", PINNED)
def test_checker_pc_dot_equals_its_composition_on_the_edge_operands(name, last):
    """pc_dot against tests/test_pc_dot_cpu.composition on every case of the GPU file; pc_mult is the composition of one pair."""
    eng = checker(name)
    level = levels(eng, last)
    for what, pairs, bias in G.pc_dot_cases(eng, level):
        got = eng.pc_dot(pairs, bias)
        assert got.level == level + 1
        same(got, pc_composition(eng, pairs, bias), f"{name} level {level} pc_dot {what}")
    for triple in G.TRIPLES:                                            # one pair without bias is pc_mult, and pc_add is the bias step
        mult, add = G.plain_ops(eng, level, triple)
        (ct,), (pt,), _ = G.pc_operands(eng, level, triple)
        same(mult, pc_composition(eng, [(pt, ct)]), f"{name} level {level} pc_mult {'/'.join(triple)}")
        assert add.level == level and torch.equal(add.data[1][0], ct.data[1][0])


@pytest.mark.parametrize("last", [0, 1], ids=G.LEVEL_IDS)
@pytest.mark.parametrize("name", PINNED)
def test_checker_pc_matmul_equals_its_composition_on_the_edge_operands(name, last):
    """pc_matmul — and the GPU file's checker_pc_matmul, which computes a repeated row once — against the composition of every
    row's pairs."""
    eng = checker(name)
    level = levels(eng, last)
    for what, W, cts, bias in G.pc_matmul_cases(eng, level):
        got = G.checker_pc_matmul(eng, W, cts, bias)
        assert len(got) == len(W)
        done = {}
        for o, (row, b) in enumerate(zip(W, bias)):
            key = (tuple(id(pt) for pt in row), id(b))
            if key not in done:
                done[key] = pc_composition(eng, [(pt, ct) for pt, ct in zip(row, cts) if pt is not None], b)
            same(got[o], done[key], f"{name} level {level} pc_matmul {what} output {o}")
        if len(done) > 1 or len(cts) <= G.CI:                           # (the long uniform layer: its rows are one pc_dot)
            for o, (g, w) in enumerate(zip(eng.pc_matmul(W, cts, bias), got)):
                same(g, w, f"{name} level {level} pc_matmul {what} output {o} against the rows computed once")


@pytest.mark.parametrize("last", [0, 1], ids=G.LEVEL_IDS)
@pytest.mark.parametrize("name", PINNED)
def test_checker_pc_matmul_batch_equals_the_loop_of_pc_matmul_on_the_edge_operands(name, last):
    eng = checker(name)
    level = levels(eng, last)
    for what, W, X, bias, _ in G.pc_batch_cases(eng, level):
        got = eng.pc_matmul_batch(W, X, bias)
        assert len(got) == len(X)
        for t, (cts, outs) in enumerate(zip(X, got)):
            for o, (g, w) in enumerate(zip(outs, eng.pc_matmul(W, cts, bias))):
                same(g, w, f"{name} level {level} pc_matmul_batch {what} token {t} output {o}")


def int_sums_composition(eng, cts, ints, consts):
    """tests/test_poly_eval_cpu.sums_composition on the integers themselves, from public ops"""
    outs = []
    for g, row in enumerate(ints):
        acc = None
        for ct, s in zip(cts, row):
            term = eng.mult_int_scalar(ct, s)
            acc = term if acc is None else eng.cc_add(acc, term)
        out = eng.rescale(acc)
        outs.append(out if consts is None else eng._add_int_to_coefficient0(out, consts[g]))
    return outs


@pytest.mark.parametrize("last", [0, 1], ids=G.LEVEL_IDS)
@pytest.mark.parametrize("name", PINNED)
def test_checker_weighted_sums_equal_their_composition_on_the_edge_operands(name, last):
    """.. and, on the first ten coefficients (every phase of the rounder's five values twice), the residues Python integers
    give: sum_t s_t x_t, minus its residue r of the dropped prime, divided by that prime, plus [r > q_drop // 2], plus the const
    at coefficient 0."""
    eng = checker(name)
    level = levels(eng, last)
    ids = eng.ntt.p.destination_arrays[level][0]
    q = [int(eng.ctx.q[i]) for i in ids]
    for what, cts, ints, consts in G.wsum_cases(eng, level):
        got = eng._weighted_sums_int(cts, ints, consts)
        for g, (a, b) in enumerate(zip(got, int_sums_composition(eng, cts, ints, consts))):
            assert a.level == level + 1
            same(a, b, f"{name} level {level} weighted_sums {what} output {g}")
        for g, row in enumerate(ints):
            for comp in range(2):
                for j in range(10):
                    acc = [sum(s * int(ct.data[comp][0][r, j]) for s, ct in zip(row, cts)) % q[r] for r in range(len(q))]
                    rho = int(acc[0] > q[0] // 2)
                    for r in range(1, len(q)):
                        t = (acc[r] - acc[0]) * pow(q[0], -1, q[r]) + rho
                        if consts is not None and comp == 0 and j == 0:
                            t += consts[g]
                        assert (int(got[g].data[comp][0][r - 1, j]) - t) % q[r] == 0, (name, level, what, g, comp, j, r)


@pytest.mark.parametrize("last", [0, 1], ids=G.LEVEL_IDS)
@pytest.mark.parametrize("name", PINNED)
def test_checker_cc_products_equal_cc_dot_of_every_output_on_the_edge_operands(name, last):
    """cc_dot_batch and cc_matmul against cc_dot of each output's pairs (itself held to its composition on these operands by
    tests/test_accumulating_ops_edges_cpu.py); the key cache then holds exactly the two evaluation keys the cases use."""
    cfg, eng = (name, 1), checker(name)
    level = levels(eng, last)
    dots = G.dot_batch_of(eng, level)
    assert [len(d) for d in dots] == list(G.DOT_BATCH)
    seen = set()
    for kpat in G.EVK_PATTERNS:
        evk = A.evk_of(cfg, eng, kpat)
        for j, (g, pairs) in enumerate(zip(eng.cc_dot_batch(dots, evk), dots)):
            assert g.level == level + 1
            same(g, eng.cc_dot(pairs, evk), f"{name} level {level} cc_dot_batch evk {kpat} dot {j}")
    for kpat, what, Am, Bm in G.matmul_cases(eng, level):
        seen.add(kpat)
        evk = A.evk_of(cfg, eng, kpat)
        got = eng.cc_matmul(Am, Bm, evk)
        for i in range(len(Am)):
            for j in range(len(Bm[0])):
                pairs = [(Am[i][t], Bm[t][j]) for t in range(len(Bm)) if Am[i][t] is not None]
                same(got[i][j], eng.cc_dot(pairs, evk), f"{name} level {level} cc_matmul evk {kpat} {what} output ({i}, {j})")
    assert seen == set(G.EVK_PATTERNS)
    assert A._KEYS["cfg"] == cfg and {k for k in A._KEYS if isinstance(k, tuple) and k[0] == id(eng) and k[1] == "evk"} == \
        {(id(eng), "evk", kpat) for kpat in G.EVK_PATTERNS}


@pytest.mark.parametrize("last", [0, 1], ids=["level0", "deepest_level"])
@pytest.mark.parametrize("name", PINNED)
def test_checker_poly_eval_equals_its_composition_on_the_edge_operands(name, last):
    """.. and poly_eval_batch is the loop of poly_eval, under the key of 2q - 1 and on the deepest level under the uniform one too."""
    cfg, eng = (name, 1), checker(name)
    level = G.poly_levels(eng)[last]
    assert level + eng.poly_depth(G.POLY_DEGREE) == (eng.num_levels - 1 if last else 4)
    n1 = encdec.poly_split(G.POLY_DEGREE)
    xs = G.poly_inputs(eng, level)
    for kpat in G.EVK_PATTERNS[:1 + last]:
        evk = A.evk_of(cfg, eng, kpat)
        loop = [eng.poly_eval(x, G.POLY_COEFFS, evk) for x in xs]
        for x, g, pattern in zip(xs, loop, G.POLY_PATTERNS):
            assert g.level == level + 4
            same(g, poly_composition(eng, x, G.POLY_COEFFS, evk, "power", None, n1), f"{name} level {level} poly_eval evk {kpat} {pattern}")
        for i, (b, g) in enumerate(zip(eng.poly_eval_batch(xs, G.POLY_COEFFS, evk), loop)):
            same(b, g, f"{name} level {level} poly_eval_batch evk {kpat} ciphertext {i}")


@pytest.mark.parametrize("last", [0, 1], ids=G.LEVEL_IDS)
@pytest.mark.parametrize("name,n_dev", G.CONFIGS)
def test_the_identity_plaintext_and_the_weight_one_are_rescale(name, n_dev, last):
    """pc_dot([(identity, pre)]) and _weighted_sums_int([pre], [[1]]) have exactly the words of rescale(pre), on one and on two
    devices; pre's dropped limb holds the rounder's five values — 0, round_at - 1, round_at, round_at + 1, q_drop - 1 — on both
    lanes of a 16-byte pair, in both components.  So the rounder cases of the GPU file put those words before the compare
    [row0 > round_at] of lf_pc_dot, lf_pc_matmul, lf_pc_matmul_batch and lf_weighted_sums."""
    eng = checker(name, n_dev)
    level = levels(eng, last)
    p = eng.ntt.p
    owner = p.rescaler_loc[level]
    q_drop = int(eng.ctx.q[p.destination_arrays[level][owner][0]])
    at = q_drop // 2
    ident, pres, _ = G.rounder_operands(eng, level, 2)
    for pre in pres:
        for comp in range(2):
            row0 = pre.data[comp][owner][0].numpy()
            for lane in range(2):
                assert set(row0[lane::2].tolist()) == {0, at - 1, at, at + 1, q_drop - 1}, (name, level, comp, lane)
        want = eng.rescale(pre)
        A.same_ct(eng.pc_dot([(ident, pre)]), want, f"{name} x {n_dev} level {level} pc_dot by the identity")
        A.same_ct(eng._weighted_sums_int([pre], [[1]])[0], want, f"{name} x {n_dev} level {level} the weight 1")
    assert not all(torch.equal(a, b) for x, y in zip(pres[0].data, pres[1].data) for a, b in zip(x, y))   # (the shift counts)


def test_every_case_of_the_gpu_file_stays_inside_the_documented_ranges():
    """A condition on the inputs, not a measurement (tests/test_matrix_ops_edges_cpu.py has the same check for its file): chunks
    against LF_PC_MATMUL_CI, tokens against LF_PC_MATMUL_BATCH_MAX_TOKENS, terms and outputs of the weighted sums against
    LF_WSUM_MAX_TERMS / LF_WSUM_MAX_OUTPUTS, the inner dimension and the operands of cc_matmul against LF_CC_MATMUL_MAX_INNER /
    LF_CC_MATMUL_MAX_OPERANDS, digits against LF_FP64_MAX_DIGITS, and the two fp64 accumulator arguments the cases lean on."""
    header = open(os.path.join(ROOT, "include", "ckks_hip.h")).read()
    cap = {name: int(re.search(rf"#define {name} (\d+)", header).group(1)) for name in
           ("LF_FP64_MAX_DIGITS", "LF_PC_MATMUL_CI", "LF_PC_MATMUL_MAX_OUTPUTS", "LF_PC_MATMUL_BATCH_MAX_TOKENS", "LF_WSUM_MAX_TERMS",
            "LF_WSUM_MAX_OUTPUTS", "LF_CC_MATMUL_MAX_INNER", "LF_CC_MATMUL_MAX_OPERANDS")}
    source = open(os.path.join(ROOT, "liberate_fhe_amd", "csrc", "ckks_ks.hip")).read()
    reduce_every = int(re.search(r"#define LF_MATMUL_REDUCE_EVERY (\d+)", source).group(1))
    engines = [checker(*cfg) for cfg in G.CONFIGS] + [checker("sb40_K7"), checker("sb40_K7", logN=12)]
    assert len(engines) == len(G.CONFIGS) + len(G.ORCHESTRATED)
    digits = set()
    for eng in engines:
        assert max(eng.ctx.q) < 1 << 60                                  # (no set takes weighted_sums' composition for a wide prime)
        for level in set(A.levels_of(eng)) | set(G.poly_levels(eng)):
            assert 0 <= level < eng.num_levels - 1
            nparts = len(eng._ks_tables(level)["order"])
            digits.add(nparts)
            assert nparts / 2 + 4 < 64 and nparts <= cap["LF_FP64_MAX_DIGITS"], (eng.ctx.logN, level, nparts)
        assert G.poly_levels(eng)[1] + eng.poly_depth(G.POLY_DEGREE) == eng.num_levels - 1
    assert max(digits) == 10
    # the pc family: a full chunk and one input past it; fp64-class rows sum CI balanced products and one word inside dp_reduce's 64 q
    assert G.CI == cap["LF_PC_MATMUL_CI"] and cap["LF_PC_MATMUL_CI"] // 2 + 1 < 64
    assert G.PC_MATMUL_SHAPES == ((cap["LF_PC_MATMUL_CI"], 4), (cap["LF_PC_MATMUL_CI"] + 1, 3))
    assert all(k_out <= cap["LF_PC_MATMUL_MAX_OUTPUTS"] for _, k_out in G.PC_MATMUL_SHAPES + (G.PC_MATMUL_HOLES,))
    assert [launch_groups(k_out) for _, k_out in G.PC_MATMUL_SHAPES + (G.PC_MATMUL_HOLES,)] == [[4], [2, 1], [4, 1]]
    assert [launch_groups(k) for k in G.PC_DOT_KS] == [[1], [4], [4, 4, 1]]
    sizes = type(eng).pc_matmul_batch_sizes                             # tokens per native call: the engine groups pairs, 3 = 2 + one left over
    assert sizes == (2,) and max(sizes) <= cap["LF_PC_MATMUL_BATCH_MAX_TOKENS"] and G.PC_BATCH_TOKENS == max(sizes) + 1
    # weighted sums
    assert G.WSUM_K == cap["LF_WSUM_MAX_TERMS"] and G.WSUM_G <= cap["LF_WSUM_MAX_OUTPUTS"] and launch_groups(G.WSUM_G) == [4, 1]
    # the cc products
    assert sum(G.DOT_BATCH) == 21 and len(G.DOT_BATCH) == 7 and max(G.DOT_BATCH) == 9 and launch_groups(9) == [4, 4, 1]
    assert G.MATMUL_REDUCE_EVERY == reduce_every and reduce_every + 1 < 64
    assert G.MATMUL_LONG_INNER == (reduce_every + 1, cap["LF_CC_MATMUL_MAX_INNER"]) == (33, encdec.CC_MATMUL_MAX_INNER)
    assert G.MATMUL_LONG_CFG in G.CONFIGS
    eng = checker(*G.MATMUL_LONG_CFG)
    for kpat, what, Am, Bm in G.matmul_cases(eng, 0):
        m, k, n, calls = encdec.cc_matmul_plan(Am, Bm)
        assert k <= cap["LF_CC_MATMUL_MAX_INNER"] and len(calls) == 1 and len(calls[0]["operands"]) == 3 <= cap["LF_CC_MATMUL_MAX_OPERANDS"]
    top = A.dot_operands(eng, 0)[0][0]
    for K in G.MATMUL_LONG_INNER:
        m, k, n, calls = encdec.cc_matmul_plan([[top] * K] * 2, [[top] * 2] * K)
        assert (m, k, n) == (2, K, 2) and len(calls) == 1 and len(calls[0]["operands"]) == 1
    assert encdec.cc_matmul_plan([[top] * (K + 1)], [[top]] * (K + 1))[3] is None          # one more takes the composition
    # poly_eval: degree 7 is three babies, two blocks and one giant step
    sched = encdec.poly_schedule(G.POLY_DEGREE, encdec.poly_split(G.POLY_DEGREE))
    assert (sched["n1"], sched["G"], sched["baby"], sched["common"], sched["depth"]) == (4, 2, 2, 3, 4)
    assert len(G.POLY_COEFFS) == G.POLY_DEGREE + 1 and len(G.POLY_PATTERNS) == 3
    assert set(G.EVK_PATTERNS) == {"top", "random"} and len(G.TRIPLES) == 5 and {t[1] for t in G.TRIPLES} >= {"half", "q|0", "random"}
