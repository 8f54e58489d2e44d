"""The matrix and slot-sum ops — lt_matmul (lt_block_products_kernel behind the baby sums), lt_matmul_bsgs (ks_inner_giantb_kernel
and the grouped tail) and the single-ciphertext rotate_sum / inner_sum (ks_inner_rsum_kernel) — at worst-case words and on the
edge parameter sets, word for word against the checker engine (tests/oracle_backend.OracleBackend, pinned at these very operands
by tests/test_matrix_ops_edges_cpu.py).

Their own files run them on uniform random words, on parameter sets with 2 to 6 special primes.  Here the ciphertexts, the keys and
the encoded diagonals sit on the bounds the kernels' range arguments rely on (tests/helpers.py: edge_ciphertext, edge_key,
edge_diagonals), on the configurations of tests/test_accumulating_ops_edges_gpu.py, whose engines, key cache, same_ct and
native_calls serve here: ten digits of one limb, 8 special primes on one and two logical devices, both arithmetic classes row by
row, a digit of 8 integer-class limbs, 18-bit primes; at level 0 and at the last level the ops accept; and through the
orchestrated path (native op entries off) at logN 13 and 12.  Which path ran is counted at the backend's native entry: both
leave the checker's words, so a quiet fall-back to the orchestration would otherwise pass.  No tolerance anywhere: every
comparison is torch.equal."""
import warnings

import pytest

from tests import test_accumulating_ops_edges_gpu as A
from tests.helpers import edge_ciphertext, edge_diagonals
from tests.test_lt_matmul_bsgs_cpu import LAYOUT as BSGS_LAYOUT, N1
from tests.test_lt_matmul_gpu import LAYOUT as FLAT_LAYOUT
from tests.test_rotate_sum_batch_gpu import key_sets

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore", category=UserWarning)

CONFIGS, ORCHESTRATED, LEVEL_IDS = A.CONFIGS, A.ORCHESTRATED, A.LEVEL_IDS
# ciphertext pattern, key pattern, diagonal pattern
TRIPLES = (("top", "top", "top"), ("mixed", "top", "mixed"), ("random", "random", "random"))
RSUM_PAIRS = [(c, k) for c in ("top", "mixed") for k in ("top", "random")]      # ciphertext pattern, key pattern
INNER_SUM = (16, 4)                                                             # n, radix: two stages of three keys
INNER_STEPS = (1, 2, 3, 4, 8, 12)


def key_steps():
    """every step any case of this file needs a rotation key for"""
    out = {s for row in FLAT_LAYOUT for st in row if st is not None for s in st}
    for row in BSGS_LAYOUT:
        for st in row:
            if st is not None:
                out |= {s % N1 for s in st} | {s - s % N1 for s in st}
    for steps, _ in key_sets():
        out |= set(steps)
    return sorted((out | set(INNER_STEPS)) - {0})


def keys_of(cfg, eng, pattern):
    return A.keys_of(cfg, eng, pattern, key_steps())


def layer(eng, level, patterns, layout, n1=None):
    """(W, cts) of a layout on edge words: one diagonals object per block, each with its own seed (under "mixed" and "random" no
    two blocks share words), one ciphertext per column"""
    W = [[None if st is None else edge_diagonals(eng, level, st, patterns[2], 40 + 64 * level + 8 * o + i, n1)
          for i, st in enumerate(row)] for o, row in enumerate(layout)]
    cts = [edge_ciphertext(eng, level, patterns[0], 20 + 3 * level + i) for i in range(len(layout[0]))]
    return W, cts


def matmul_op(cfg, eng, level, patterns, layout, n1=None):
    """lt_matmul (n1: lt_matmul_bsgs) of one case on `eng`: the operands depend on the case alone"""
    W, cts = layer(eng, level, patterns, layout, n1)
    keys = keys_of(cfg, eng, patterns[1])
    return eng.lt_matmul(W, cts, keys) if n1 is None else eng.lt_matmul_bsgs(W, cts, keys)


def rsum_op(cfg, eng, level, pair, steps, with_self):
    ct = edge_ciphertext(eng, level, pair[0], 20 + level)
    keys = keys_of(cfg, eng, pair[1])
    return eng.rotate_sum(ct, [keys[s] for s in steps], include_self=with_self)


def inner_sum_op(cfg, eng, level):
    ct = edge_ciphertext(eng, level, "top", 20 + level)
    n, radix = INNER_SUM
    return eng.inner_sum(ct, n, keys_of(cfg, eng, "top"), radix=radix)


def level_of(cfg, last):
    H, C = A.engines(cfg)
    level = A.levels_of(H)[last]
    native = A.native_expected(cfg, H, level)
    assert (H._native_level(level) is not None) == native
    return H, C, level, native


def check_matmul(cfg, last):
    H, C, level, native = level_of(cfg, last)
    for patterns in TRIPLES:
        with A.native_calls(H.backend, "lt_matmul_native") as n:
            got = matmul_op(cfg, H, level, patterns, FLAT_LAYOUT)
        assert n.count == int(native), (cfg, level, patterns, n.count)
        want = matmul_op(cfg, C, level, patterns, FLAT_LAYOUT)
        assert len(got) == len(want) == len(FLAT_LAYOUT)
        for o, (g, w) in enumerate(zip(got, want)):
            assert g.level == level + 1
            A.same_ct(g, w, f"{cfg} level {level} lt_matmul {'/'.join(patterns)} output {o}")
    # 1 x 1: the block products behind the baby sums and the flat kernel leave the same words, on the GPU
    patterns, steps = TRIPLES[0], FLAT_LAYOUT[0][0]
    W, cts = layer(H, level, patterns, [[steps]])
    keys = keys_of(cfg, H, patterns[1])
    with A.native_calls(H.backend, "lt_matmul_native") as n:
        got = H.lt_matmul(W, cts, keys)
    assert n.count == int(native) and len(got) == 1
    with A.native_calls(H.backend, "linear_transform_native") as n:
        flat = H.linear_transform(cts[0], W[0][0], keys)
    assert n.count == int(native)
    A.same_ct(got[0], flat, f"{cfg} level {level} lt_matmul 1 x 1 against linear_transform on the GPU")
    Wc, ctc = layer(C, level, patterns, [[steps]])
    A.same_ct(got[0], C.lt_matmul(Wc, ctc, keys_of(cfg, C, patterns[1]))[0], f"{cfg} level {level} lt_matmul 1 x 1 against the checker")


def check_matmul_bsgs(cfg, last):
    H, C, level, native = level_of(cfg, last)
    assert H.lt_matmul_bsgs_group == 4
    for patterns in TRIPLES:
        with A.native_calls(H.backend, "lt_matmul_bsgs_native") as n:
            got = matmul_op(cfg, H, level, patterns, BSGS_LAYOUT, N1)
        assert n.count == int(native), (cfg, level, patterns, n.count)
        want = matmul_op(cfg, C, level, patterns, BSGS_LAYOUT, N1)
        assert len(got) == len(want) == len(BSGS_LAYOUT)
        for o, (g, w) in enumerate(zip(got, want)):
            assert g.level == level + 1
            A.same_ct(g, w, f"{cfg} level {level} lt_matmul_bsgs {'/'.join(patterns)} output {o}")
        if patterns == TRIPLES[0]:          # the giant steps one output at a time (ks_inner_giant_kernel) against groups of 4
            H.lt_matmul_bsgs_group = 1
            try:
                with A.native_calls(H.backend, "lt_matmul_bsgs_native") as n:
                    single = matmul_op(cfg, H, level, patterns, BSGS_LAYOUT, N1)
            finally:
                del H.lt_matmul_bsgs_group      # (the instance attribute over the class's 4)
            assert n.count == int(native) and H.lt_matmul_bsgs_group == 4
            for o, (g, w) in enumerate(zip(single, want)):
                A.same_ct(g, w, f"{cfg} level {level} lt_matmul_bsgs group 1 output {o}")


def check_rotate_sum(cfg, last):
    H, C, level, native = level_of(cfg, last)
    for pair in RSUM_PAIRS:
        for steps, with_self in key_sets():
            with A.native_calls(H.backend, "rotate_sum_native") as n:
                got = rsum_op(cfg, H, level, pair, steps, with_self)
            assert n.count == int(native), (cfg, level, pair, steps, with_self, n.count)
            want = rsum_op(cfg, C, level, pair, steps, with_self)
            assert got.level == level and not got.ntt_state and not got.include_special
            A.same_ct(got, want, f"{cfg} level {level} rotate_sum {'/'.join(pair)} steps {steps} self {with_self}")


def check_inner_sum(cfg, last):
    H, C, level, native = level_of(cfg, last)
    with A.native_calls(H.backend, "rotate_sum_native") as n:
        got = inner_sum_op(cfg, H, level)
    assert n.count == 2 * int(native), (cfg, level, n.count)           # one call per stage: 16 = 4 x 4
    assert got.level == level
    A.same_ct(got, inner_sum_op(cfg, C, level), f"{cfg} level {level} inner_sum n 16 radix 4")


@pytest.mark.parametrize("last", [0, 1], ids=LEVEL_IDS)
@pytest.mark.parametrize("name,n_dev", CONFIGS)
def test_lt_matmul_on_edge_words_equals_the_checker(name, n_dev, last):
    """lf_lt_matmul (one device) / the orchestration with a digit exchange (two): the 3 x 5 layout of tests/test_lt_matmul_gpu.py
    (key groups 4 + 2 + 1, a step-0-only column, outputs written fresh and outputs added to) under the three pattern triples, on
    every configuration; on "top" also 1 x 1, which must have the words of linear_transform on the GPU."""
    check_matmul((name, n_dev), last)


@pytest.mark.parametrize("last", [0, 1], ids=LEVEL_IDS)
@pytest.mark.parametrize("name,n_dev", CONFIGS)
def test_lt_matmul_bsgs_on_edge_words_equals_the_checker(name, n_dev, last):
    """lf_lt_matmul_bsgs: the 3 x 6 layout of tests/test_lt_matmul_bsgs_cpu.py over n1 = 4 (giant groups 4 + 1, 2 and 1, sums fed
    by one and by two inputs, an output without giant step 0 and one with nothing else) under the three pattern triples; on "top"
    also with lt_matmul_bsgs_group = 1 (the single giant kernel) against the groups of 4."""
    check_matmul_bsgs((name, n_dev), last)


@pytest.mark.parametrize("last", [0, 1], ids=LEVEL_IDS)
@pytest.mark.parametrize("name,n_dev", CONFIGS)
def test_rotate_sum_on_edge_words_equals_the_checker(name, n_dev, last):
    """lf_rotate_sum — the GPU's own ks_inner_rsum_kernel, which rotate_sum_batch's edge test never compares with anything: one
    key; seven with the self term; five without; one more than a batch launch takes; the self term alone; ciphertexts "top" and
    "mixed" under keys at 2q - 1 and uniform ones."""
    check_rotate_sum((name, n_dev), last)


@pytest.mark.parametrize("last", [0, 1], ids=LEVEL_IDS)
@pytest.mark.parametrize("name,n_dev", CONFIGS)
def test_inner_sum_on_edge_words_equals_the_checker(name, n_dev, last):
    """inner_sum(ct, 16, keys, radix=4) from a "top" ciphertext under keys at 2q - 1: two stages of three keys and the self
    term, the second on whatever the first leaves; one native call per stage."""
    check_inner_sum((name, n_dev), last)


@pytest.mark.parametrize("op", ["lt_matmul", "lt_matmul_bsgs", "rotate_sum", "inner_sum"])
@pytest.mark.parametrize("last", [0, 1], ids=LEVEL_IDS)
@pytest.mark.parametrize("cfg", sorted(ORCHESTRATED))
def test_the_same_cases_through_the_orchestrated_path(cfg, last, op):
    """Native op entries off: the engine's step-by-step orchestration of the same operations at logN 13, and at logN 12 where
    the key switch runs unfused.  No native entry may be reached."""
    {"lt_matmul": check_matmul, "lt_matmul_bsgs": check_matmul_bsgs, "rotate_sum": check_rotate_sum,
     "inner_sum": check_inner_sum}[op](cfg, last)
