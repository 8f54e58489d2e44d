"""The yardstick of tests/test_accumulating_ops_edges_gpu.py, without a GPU: the edge diagonals hold what their patterns say in
the layout of utils.synth.diagonals; the checker engine's linear_transform (flat and baby-step / giant-step) and cc_dot, ON THE
OPERANDS OF THAT FILE, equal the compositions of public steps that define their words (tests/test_linear_transform_cpu.py,
tests/test_linear_transform_bsgs_cpu.py, tests/test_cc_dot_cpu.py); and every parameter set and level that file uses stays
inside the ranges the kernels document."""
import warnings

import numpy as np
import pytest
import torch

from liberate_fhe_amd.fhe import encdec
from liberate_fhe_amd.utils import synth
from tests import test_accumulating_ops_edges_gpu as G
from tests.helpers import SMALL_PRIME_LIMIT, edge_diagonals, edge_param_sets, thue_morse
from tests.test_cc_dot_cpu import composition as dot_composition
from tests.test_linear_transform_bsgs_cpu import bsgs_composition
from tests.test_linear_transform_cpu import composition

warnings.filterwarnings("ignore", category=UserWarning)
SETS = edge_param_sets()
_ENGINES = {}


def checker(name, n_dev=1, **over):
    key = (name, n_dev, tuple(sorted(over.items())))
    if key not in _ENGINES:
        from liberate_fhe_amd.fhe import ckks_engine
        from tests.oracle_backend import OracleBackend
        params = G.LT if name == "LT" else {**SETS[name], **over}
        _ENGINES[key] = ckks_engine(devices=["cpu"] * n_dev, backend=OracleBackend(), **params)
    return _ENGINES[key]


def by_prime(eng, level, j, diags):
    """prime id -> the [N] words of diagonal j, over every device (the special rows are on each device: the same words)"""
    out = {}
    for d, t in enumerate(diags.data[j]):
        for r, i in enumerate(eng.ntt.p.destination_arrays_with_special[level][d]):
            assert i not in out or (out[i] == t[r].numpy()).all()
            out[i] = t[r].numpy()
    return out


@pytest.mark.parametrize("level", [0, 4])
def test_edge_diagonals_hold_their_patterns_in_the_layout_of_synth(level):
    eng, two = checker("sb41_K2"), checker("sb41_K2", 2)
    q, N = eng.ctx.q, eng.ctx.N
    steps = (13, 0, 1, 700)                                            # (given out of order: the pack is ascending)
    ids = eng.ntt.p.destination_arrays_with_special[level][0]
    assert len(ids) == eng._rows(0, level, True) and {int(q[i]) < SMALL_PRIME_LIMIT for i in ids} == {True, False}
    tm, odd = thue_morse(N), np.arange(N) & 1
    want = {"top": lambda m: np.full(N, 2 * m - 1), "top|0": lambda m: np.where(tm == 1, 0, 2 * m - 1),
            "top|1": lambda m: np.where(tm == 1, 1, 2 * m - 1), "half": lambda m: m // 2 + odd}
    rotation = ("top", "top|0", "half", "top|1")
    for n1 in (None, 4):
        ref = synth.diagonals(eng, 3, level, steps) if n1 is None else synth.diagonals_bsgs(eng, 3, level, steps, n1)
        seen = {}
        for pattern in ("top", "top|0", "half", "mixed", "random"):
            dg = edge_diagonals(eng, level, steps, pattern, 3, n1)
            # the layout: tags, flags, shapes, and the pack remembered (the engine finds it without packing again)
            assert (dg.origin, dg.level, dg.include_special, dg.ntt_state, dg.montgomery_state, dg.hash, dg.version) == \
                   (ref.origin, ref.level, ref.include_special, ref.ntt_state, ref.montgomery_state, ref.hash, ref.version)
            assert eng.diagonal_steps(dg) == sorted(steps) and len(dg.data) == len(ref.data) == len(steps)
            assert all(a[0].shape == b[0].shape and a[0].dtype == b[0].dtype and len(a) == len(b) == 1 for a, b in zip(dg.data, ref.data))
            pack = eng._diag_pack(dg)[0]
            assert pack.shape == (len(steps), len(ids), N) and all(dg.data[j][0].data_ptr() == pack[j].data_ptr() for j in range(len(steps)))
            # the words, on ordinary and special rows
            for j in range(len(steps)):
                rows = by_prime(eng, level, j, dg)
                assert sorted(rows) == sorted(ids)
                for i, w in rows.items():
                    m = int(q[i])
                    assert w.min() >= 0 and w.max() < 2 * m
                    if pattern == "random":
                        assert w.max() >= m and len(np.unique(w)) > N // 2                    # lazy words, not a constant
                    else:
                        pat = rotation[(i + j) % 4] if pattern == "mixed" else pattern
                        assert (w == want[pat](m)).all(), (pattern, j, i)
            seen[pattern] = dg
            # two devices hold the words one device holds
            dg2 = edge_diagonals(two, level, steps, pattern, 3, n1)
            assert dg2.origin == dg.origin and all(len(row) == len(two._loc(level, special=True)) for row in dg2.data)
            for j in range(len(steps)):
                a, b = by_prime(eng, level, j, dg), by_prime(two, level, j, dg2)
                assert sorted(a) == sorted(b) and all((a[i] == b[i]).all() for i in a)
        # "mixed" and "random" give every diagonal other words
        for pattern in ("mixed", "random"):
            first = [seen[pattern].data[j][0] for j in range(len(steps))]
            assert all(not torch.equal(first[a], first[b]) for a in range(len(steps)) for b in range(a))


def same(got, want, what):
    assert got.level == want.level and got.origin == want.origin
    for c, (a, b) in enumerate(zip(got.data, want.data)):
        assert torch.equal(a[0], b[0]), f"{what}, component {c}: {int((a[0] != b[0]).sum())} of {b[0].numel()} words differ"


COMPOSED = [t for t in G.TRIPLES if t[0] in ("top", "mixed", "half")]


@pytest.mark.parametrize("last", [0, 1], ids=G.LEVEL_IDS)
@pytest.mark.parametrize("name", ["sb40_K1", "sb41_K2"])
def test_checker_linear_transforms_equal_their_compositions_on_the_edge_operands(name, last):
    """ten digits of one limb, and both arithmetic classes row by row: the checker's flat and baby-step / giant-step transforms on
    the GPU file's ciphertexts, keys and diagonals of the patterns top, mixed and half are the compositions' words."""
    cfg, eng = (name, 1), checker(name)
    level = G.levels_of(eng)[last]
    assert len(COMPOSED) == 3
    for patterns in COMPOSED:
        keys = G.keys_of(cfg, eng, patterns[1])
        ct = G.edge_ciphertext(eng, level, patterns[0], 20 + level)
        for n1, steps in ((None, G.FLAT_STEPS), G.BSGS_FULL):
            diags = edge_diagonals(eng, level, steps, patterns[2], 7 + level, n1)
            got = G.lt_op(cfg, eng, level, patterns, steps, n1)
            want = composition(eng, ct, diags, keys) if n1 is None else bsgs_composition(eng, ct, diags, keys)
            assert got.level == level + 1
            same(got, want, f"{name} level {level} {'/'.join(patterns)} n1 {n1}")


@pytest.mark.parametrize("last", [0, 1], ids=G.LEVEL_IDS)
@pytest.mark.parametrize("name", ["sb40_K1", "sb41_K2"])
def test_checker_cc_dot_equals_its_composition_on_the_edge_operands(name, last):
    cfg, eng = (name, 1), checker(name)
    level = G.levels_of(eng)[last]
    pairs = G.dot_operands(eng, level)
    for kpat, k, slot in [("top", k, 0) for k in G.DOT_KS] + [("top", 5, 1), ("top", 5, 2), ("random", 9, 2), ("random", 1, 0)]:
        assert (kpat, k, slot) in G.dot_cases()
        evk = G.evk_of(cfg, eng, kpat)
        got = eng.cc_dot([pairs[slot]] * k, evk)
        assert got.level == level + 1
        same(got, dot_composition(eng, [pairs[slot]] * k, evk), f"{name} level {level} cc_dot evk {kpat} k {k} pair {slot}")


def launch_groups(n):
    """the keys per launch of lf_ks_tail_lt / lf_ks_tail_rsum / lf_ks_baby_sums (key_group, csrc/ckks_ks.hip): 4 while 4 are left, then
    2, then 1"""
    out = []
    while n:
        g = 4 if n >= 4 else 2 if n >= 2 else 1
        out.append(g)
        n -= g
    return out


def test_every_case_of_the_gpu_file_stays_inside_the_documented_ranges():
    """A condition on the inputs, not a measurement.  csrc/ckks_ks.hip proves the fp64-class sums for
      nparts / 2 + 4 < 64     ("|sums| < (digits / 2 + 4) q, inside dp_reduce's 64 q": ks_inner_giant_kernel, the tightest), and
      at most 4 keys a group  ("|running sums| <= (NR + 2) q, inside dp_reduce's 64 q": ks_inner_lt_kernel, NR <= 4);
    lf_linear_transform_bsgs takes at most 63 baby keys.  A set added to the GPU file that leaves these ranges fails here."""
    import os
    import re
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ckks_hip.h")).read()
    bound = int(re.search(r"#define LF_FP64_MAX_DIGITS (\d+)", header).group(1))
    assert bound / 2 + 4 < 64
    engines = [checker(*cfg) for cfg in G.CONFIGS] + [checker("sb40_K7"), checker("sb40_K7", logN=12), checker("LT")]
    assert len(engines) == len(G.CONFIGS) + len(G.ORCHESTRATED) + 1
    digits = set()
    for eng in engines:
        for level in G.levels_of(eng):
            assert 0 <= level < eng.num_levels - 1
            nparts = len(eng._ks_tables(level)["order"])
            digits.add(nparts)
            assert nparts / 2 + 4 < 64 and nparts <= bound, (eng.ctx.logN, level, nparts)
    assert max(digits) == 10                                            # sb40_K1: the most digits any engine set has
    key_counts = [len([s for s in steps if s]) for _, steps in G.flat_cases()]
    shapes = [(n1, steps) for _, n1, steps in G.bsgs_cases()] + [G.LIMIT_SHAPES[nb] for nb in (62, 63)]
    for n1, steps in shapes:
        _, babies, giants = encdec.bsgs_split(steps, 1 << 11, n1)        # (logN 12: the fewest slots of any engine here)
        nb = len([b for b in babies if b])
        assert nb <= 63 and all(g < (1 << 11) for g in giants)
        key_counts.append(nb)
    for n in key_counts:
        assert all(g <= G.LT_GROUP_MAX for g in launch_groups(n))
    assert G.LT_GROUP_MAX + 2 < 64
    assert sorted(key_counts)[-1] == 63 and 9 in key_counts and 0 in key_counts
    assert max(G.DOT_KS) == 9 and launch_groups(9) == [4, 4, 1]
