"""The yardstick of tests/test_matrix_ops_edges_gpu.py, without a GPU: the checker engine's lt_matmul, lt_matmul_bsgs and rotate_sum,
ON THE OPERANDS OF THAT FILE, equal the compositions of public steps that define their words (tests/test_lt_matmul_cpu.py,
tests/test_lt_matmul_bsgs_cpu.py, tests/test_inner_sum_cpu.py); inner_sum is the chain of its plan's rotate_sums; and every
parameter set, level and shape that file uses stays inside the ranges the kernels and the C entries document."""
import os
import re
import warnings

import pytest

from liberate_fhe_amd.fhe import encdec
from tests import test_matrix_ops_edges_gpu as G
from tests.helpers import edge_ciphertext
from tests.test_accumulating_ops_edges_cpu import checker, launch_groups, same
from tests.test_inner_sum_cpu import chain, composition as rsum_composition
from tests.test_lt_matmul_bsgs_cpu import composition as bsgs_composition
from tests.test_lt_matmul_cpu import composition as matmul_composition

warnings.filterwarnings("ignore", category=UserWarning)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PINNED = ["sb40_K1", "sb41_K2"]             # ten digits of one limb; both arithmetic classes row by row


@pytest.mark.parametrize("last", [0, 1], ids=G.LEVEL_IDS)
@pytest.mark.parametrize("name", PINNED)
def test_checker_lt_matmul_equals_its_composition_on_the_edge_operands(name, last):
    cfg, eng = (name, 1), checker(name)
    level = G.A.levels_of(eng)[last]
    for patterns in G.TRIPLES:
        W, cts = G.layer(eng, level, patterns, G.FLAT_LAYOUT)
        got = G.matmul_op(cfg, eng, level, patterns, G.FLAT_LAYOUT)
        want = matmul_composition(eng, W, cts, G.keys_of(cfg, eng, patterns[1]))
        assert len(got) == len(want) == 5
        for o, (g, w) in enumerate(zip(got, want)):
            assert g.level == level + 1
            same(g, w, f"{name} level {level} lt_matmul {'/'.join(patterns)} output {o}")


@pytest.mark.parametrize("last", [0, 1], ids=G.LEVEL_IDS)
@pytest.mark.parametrize("name", PINNED)
def test_checker_lt_matmul_bsgs_equals_its_composition_on_the_edge_operands(name, last):
    cfg, eng = (name, 1), checker(name)
    level = G.A.levels_of(eng)[last]
    for patterns in G.TRIPLES:
        W, cts = G.layer(eng, level, patterns, G.BSGS_LAYOUT, G.N1)
        got = G.matmul_op(cfg, eng, level, patterns, G.BSGS_LAYOUT, G.N1)
        want = bsgs_composition(eng, W, cts, G.keys_of(cfg, eng, patterns[1]), G.N1)
        assert len(got) == len(want) == 6
        for o, (g, w) in enumerate(zip(got, want)):
            assert g.level == level + 1
            same(g, w, f"{name} level {level} lt_matmul_bsgs {'/'.join(patterns)} output {o}")


@pytest.mark.parametrize("last", [0, 1], ids=G.LEVEL_IDS)
@pytest.mark.parametrize("name", PINNED)
def test_checker_rotate_sum_and_inner_sum_equal_their_compositions_on_the_edge_operands(name, last):
    cfg, eng = (name, 1), checker(name)
    level = G.A.levels_of(eng)[last]
    for pair in G.RSUM_PAIRS:
        keys = G.keys_of(cfg, eng, pair[1])
        ct = edge_ciphertext(eng, level, pair[0], 20 + level)
        for steps, with_self in G.key_sets():
            got = G.rsum_op(cfg, eng, level, pair, steps, with_self)
            assert got.level == level
            same(got, rsum_composition(eng, ct, [keys[s] for s in steps], with_self),
                 f"{name} level {level} rotate_sum {'/'.join(pair)} steps {steps} self {with_self}")
    n, radix = G.INNER_SUM
    ct = edge_ciphertext(eng, level, "top", 20 + level)
    same(G.inner_sum_op(cfg, eng, level), chain(eng, ct, n, G.keys_of(cfg, eng, "top"), 1, radix), f"{name} level {level} inner_sum")


def test_every_case_of_the_gpu_file_stays_inside_the_documented_ranges():
    """A condition on the inputs, not a measurement (tests/test_accumulating_ops_edges_cpu.py has the same check for its file):
    digits within LF_FP64_MAX_DIGITS and within nparts / 2 + 4 < 64 (ks_inner_giant(b)_kernel, the tightest of csrc/ckks_ks.hip's
    table); at most 4 keys per launch of the baby kernel and of ks_inner_rsum_kernel; the layouts within LF_LT_MATMUL_MAX_INPUTS /
    LF_LT_MATMUL_MAX_OUTPUTS, LF_BSGS_MAX_BABY_KEYS per column, LF_LT_MATMUL_BSGS_MAX_GIANTS / LF_LT_MATMUL_BSGS_MAX_SUMS."""
    header = open(os.path.join(ROOT, "include", "ckks_hip.h")).read()
    cap = {name: int(re.search(rf"#define {name} (\d+)", header).group(1)) for name in
           ("LF_FP64_MAX_DIGITS", "LF_LT_MATMUL_MAX_INPUTS", "LF_LT_MATMUL_MAX_OUTPUTS", "LF_BSGS_MAX_BABY_KEYS",
            "LF_LT_MATMUL_BSGS_MAX_GIANTS", "LF_LT_MATMUL_BSGS_MAX_SUMS")}
    engines = [checker(*cfg) for cfg in G.CONFIGS] + [checker("sb40_K7"), checker("sb40_K7", logN=12)]
    assert len(engines) == len(G.CONFIGS) + len(G.ORCHESTRATED)
    digits = set()
    for eng in engines:
        for level in G.A.levels_of(eng):
            assert 0 <= level < eng.num_levels - 1
            nparts = len(eng._ks_tables(level)["order"])
            digits.add(nparts)
            assert nparts / 2 + 4 < 64 and nparts <= cap["LF_FP64_MAX_DIGITS"], (eng.ctx.logN, level, nparts)
    assert max(digits) == 10
    slots = 1 << 11                                                     # (logN 12: the fewest slots of any engine here)
    # lt_matmul: the keyed steps of a column are its baby keys
    assert len(G.FLAT_LAYOUT) <= cap["LF_LT_MATMUL_MAX_OUTPUTS"] and len(G.FLAT_LAYOUT[0]) <= cap["LF_LT_MATMUL_MAX_INPUTS"]
    columns = [sorted({s for row in G.FLAT_LAYOUT if row[i] is not None for s in row[i] if s}) for i in range(len(G.FLAT_LAYOUT[0]))]
    assert [launch_groups(len(c)) for c in columns] == [[4, 2, 1], [], [4, 2, 1]]
    assert all(len(c) <= cap["LF_BSGS_MAX_BABY_KEYS"] and max(c, default=0) < slots for c in columns)
    # lt_matmul_bsgs
    assert len(G.BSGS_LAYOUT) <= cap["LF_LT_MATMUL_MAX_OUTPUTS"] and len(G.BSGS_LAYOUT[0]) <= cap["LF_LT_MATMUL_MAX_INPUTS"]
    flat = [s for row in G.BSGS_LAYOUT for st in row if st is not None for s in st]
    _, babies, giants = encdec.bsgs_split(flat, slots, G.N1)
    assert len(giants) <= cap["LF_LT_MATMUL_BSGS_MAX_GIANTS"] and len([b for b in babies if b]) <= cap["LF_BSGS_MAX_BABY_KEYS"]
    keyed_sums = sum(len({s - s % G.N1 for st in row if st is not None for s in st} - {0}) for row in G.BSGS_LAYOUT)
    assert 0 < keyed_sums <= cap["LF_LT_MATMUL_BSGS_MAX_SUMS"] and max(flat) < slots
    needed = set(babies) | set(giants) | {s for c in columns for s in c} | set(G.INNER_STEPS) | {s for st, _ in G.key_sets() for s in st}
    assert sorted(needed - {0}) == G.key_steps()                        # the key cache holds exactly the steps the cases use
    # rotate_sum: at most 4 keys per launch of ks_inner_rsum_kernel, |acc| <= (NR nparts / 2 + 2 NR + 2) q < 2^52 / q
    for steps, with_self in G.key_sets():
        assert (steps or with_self) and all(g <= G.A.LT_GROUP_MAX for g in launch_groups(len(steps))) and all(0 < s < slots for s in steps)
    assert sorted(len(s) for s, _ in G.key_sets()) == [0, 1, 5, 7, 9]
    assert (G.A.LT_GROUP_MAX * max(digits) // 2 + 2 * G.A.LT_GROUP_MAX + 2) << 41 < 1 << 52
    n, radix = G.INNER_SUM
    plan = encdec.inner_sum_plan(n, 1, slots, radix)
    assert [r for r, _ in plan] == [4, 4] and sorted(s for _, st in plan for s in st) == sorted(G.INNER_STEPS)
