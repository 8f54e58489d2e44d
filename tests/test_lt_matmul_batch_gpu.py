"""lt_matmul_batch on the GPU: lf_lt_matmul_batch (one native call per group of 4 or 2 token vectors: one digit launch, one
extension + forward pass and one launch of ks_inner_babyb_kernel per key for the group, lt_block_productsb_kernel per tile of two
tokens) against the loop of lt_matmul that defines its words — at logN 13 over every grouping, shape and key count, against
linear_transform for one input, at the presets, against the checker engine, with compact keys, under the tuning knobs, at
worst-case words (the test of the product kernel's range argument) and once with real keys.  No tolerance anywhere: every
comparison of words is torch.equal."""
import json
import os
import warnings

import numpy as np
import pytest
import torch

from liberate_fhe_amd.utils import synth
from tests.helpers import edge_ciphertext, edge_diagonals, edge_key
from tests.test_inner_sum_cpu import lazy_ciphertext

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore", category=UserWarning)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "engine_digests.json")))
LT = dict(logN=13, num_scales=5, num_special_primes=2, is_secured=False)
NINE = tuple(range(1, 10))
KEY_STEPS = NINE + (700,)
# k_out rows of k_in blocks (steps per block, None: a zero block), by the keyed steps of their columns:
LAYOUTS = {
    "1x1": [[(0, 1, 2, 3, 4)]],                                                    # 4 keyed steps and step 0
    "2x3": [[(1,), (0,), NINE], [(0, 1), (0,), (0, 2, 4, 9)]],                     # 1, 0 (step 0 only: no digits) and 9 keyed steps
    "5x2": [[(0, 1, 2), (0,)], [(3, 4), None], [(1, 4), (0,)], [(0,), (0,)], [(2, 3), (0,)]],   # output groups 4 + 1
    "3x3": [[(0, 1, 5), None, (2,)], [None, None, (0, 2, 700)], [(5,), None, None]],            # None blocks, column 1 unused
}


def words(ct):
    return [torch.cat([t.cpu() for t in comp]) for comp in ct.data]


def same(a, b):
    return a.level == b.level and a.origin == b.origin and all(torch.equal(x, y) for x, y in zip(words(a), words(b)))


def all_same(got, want):
    return len(got) == len(want) and all(len(g) == len(w) and all(same(a, b) for a, b in zip(g, w)) for g, w in zip(got, want))


def keys_of(eng, steps=KEY_STEPS):
    return {s: synth.key_switch_key(eng, 40 + i, origin=f"rotation key:{s}") for i, s in enumerate(steps)}


def matrix(eng, level, layout, seed=7, make=synth.diagonals):
    return [[None if st is None else make(eng, seed + 8 * o + i, level, st) for i, st in enumerate(row)] for o, row in enumerate(layout)]


def tokens(eng, level, k_in, B, seed=90):
    return [[synth.ciphertext(eng, seed + 10 * level + k_in * t + i, level) for i in range(k_in)] for t in range(B)]


def groups(B, sizes=(4, 2)):
    out = []
    while any(k <= B for k in sizes):
        out.append(next(k for k in sizes if k <= B))
        B -= out[-1]
    return out


def strided(eng, ct):
    """the same words behind tensors that are not contiguous"""
    data = []
    for comp in ct.data:
        out = []
        for t in comp:
            wide = torch.zeros((t.shape[0], 2 * t.shape[1]), dtype=t.dtype, device=t.device)
            wide[:, ::2] = t
            out.append(wide[:, ::2])
        data.append(out)
    return eng._new(tuple(data), ct.origin, level=ct.level)


class native_calls:
    """[tokens per lf_lt_matmul_batch call] while the block runs, with groups of 4 and 2 whatever sizes the engine ships"""

    def __init__(self, eng, sizes=(4, 2)):
        self.eng, self.sizes, self.seen = eng, sizes, []

    def __enter__(self):
        real = self.eng.backend.lt_matmul_batch_native

        def spy(plan, toks, *a, **kw):
            self.seen.append(len(toks))
            return real(plan, toks, *a, **kw)
        self.eng.backend.lt_matmul_batch_native = spy
        self.eng.lt_matmul_batch_sizes = self.sizes
        return self.seen

    def __exit__(self, *exc):
        del self.eng.backend.lt_matmul_batch_native
        del self.eng.lt_matmul_batch_sizes


def engine_of(name):
    from liberate_fhe_amd.fhe import ckks_engine, presets
    if name in ("silver", "gold"):
        params = dict(presets.params[name])
        params.pop("devices", None)
    elif name == "logN17":
        params = dict(logN=17, num_scales=3, num_special_primes=2, is_secured=False)
    else:
        params = GOLD[name]["params"]
    return ckks_engine(devices=["cuda:0"], **params)


@pytest.fixture(scope="module")
def lt_engine():
    from liberate_fhe_amd.fhe import ckks_engine
    eng = ckks_engine(devices=["cuda:0"], **LT)
    assert type(eng).lt_matmul_batch_sizes and set(type(eng).lt_matmul_batch_sizes) <= set(eng.backend.lt_matmul_batch_sizes) == {4, 2}
    return eng, keys_of(eng)


@pytest.mark.parametrize("shape", list(LAYOUTS))
@pytest.mark.parametrize("level", [0, 2, 3])
def test_native_batch_equals_the_loop_at_logN_13(lt_engine, level, shape):
    """Levels 0, 2 and L - 2 (one row left); B = 1, 2, 3, 4, 5, 7 token vectors: groups 4 + 2 + a straggler; token 1 carries lazy
    words.  The loop is computed once, over all seven; the spy sees the group sizes of every call."""
    eng, keys = lt_engine
    assert level <= eng.num_levels - 2 and (level != 3 or level == eng.num_levels - 2)
    assert eng._native_level(level) is not None
    layout = LAYOUTS[shape]
    k_in = len(layout[0])
    W = matrix(eng, level, layout)
    X = tokens(eng, level, k_in, 7)
    X[1] = [lazy_ciphertext(eng, 97 + level + i, level) for i in range(k_in)]
    want = [eng.lt_matmul(W, cts, keys) for cts in X]
    assert all(o.level == level + 1 for w in want for o in w)
    with native_calls(eng) as seen:
        for B, calls in ((1, []), (2, [2]), (3, [2]), (4, [4]), (5, [4]), (7, [4, 2])):
            assert groups(B) == calls
            del seen[:]
            got = eng.lt_matmul_batch(W, X[:B], keys)
            assert seen == calls, (B, seen)
            assert all_same(got, want[:B]), (level, shape, B)


def test_one_input_gives_the_words_of_linear_transform(lt_engine):
    """k_in = 1, five tokens (4 + a straggler): output o of token t is linear_transform(X[t][0], W[o][0], keys)."""
    eng, keys = lt_engine
    W = matrix(eng, 1, [[(0, 1, 2, 5, 3)], [(4, 7)], [(0,)]])
    X = tokens(eng, 1, 1, 5)
    with native_calls(eng) as seen:
        got = eng.lt_matmul_batch(W, X, keys)
    assert seen == [4] and len(got) == 5
    for t, (g, cts) in enumerate(zip(got, X)):
        assert len(g) == 3
        for o, out in enumerate(g):
            assert same(out, eng.linear_transform(cts[0], W[o][0], keys)), (t, o)


def test_a_member_that_is_not_contiguous_takes_the_loop_and_keeps_its_place(lt_engine):
    eng, keys = lt_engine
    level, layout = 1, LAYOUTS["3x3"]
    W = matrix(eng, level, layout)
    X = tokens(eng, level, 3, 6)
    want = [eng.lt_matmul(W, cts, keys) for cts in X]
    X[2][2] = strided(eng, X[2][2])
    X[3][1] = strided(eng, X[3][1])                                   # (column 1 is unused: this token still qualifies)
    assert not X[2][2].data[0][0].is_contiguous()
    with native_calls(eng) as seen:
        got = eng.lt_matmul_batch(W, X + [X[0]], keys)               # six that qualify (4 + 2), one that does not, one repeated
    assert seen == [4, 2]
    assert all_same(got, want + [want[0]])


def test_more_outputs_than_one_call_takes(lt_engine):
    """k_out = LF_LT_MATMUL_MAX_OUTPUTS + 1 one-diagonal blocks at level L - 2: two native calls per group (64 + 1 outputs)."""
    eng, keys = lt_engine
    level = eng.num_levels - 2
    k_out = eng.backend.lt_matmul_max_outputs + 1
    assert k_out == 65
    D = [synth.diagonals(eng, 3 + j, level, (j,)) for j in range(3)]
    W = [[D[o % 3], None if o % 4 == 1 else D[(o + 1) % 3]] for o in range(k_out)]
    X = tokens(eng, level, 2, 3)
    want = [eng.lt_matmul(W, cts, keys) for cts in X]
    with native_calls(eng) as seen:
        got = eng.lt_matmul_batch(W, X, keys)
    assert seen == [2, 2]
    assert all(len(g) == k_out for g in got) and all_same(got, want)


@pytest.mark.parametrize("name", ["silver", "sb45", "sb41", "gold", "logN17"])
def test_native_batch_equals_the_loop_at_the_presets(name):
    """2 x 2 blocks of 3 diagonals, B = 3 (a group of 2 and a straggler) and B = 4, at levels 0 and L - 2; sb41 / sb45 run both
    arithmetic classes row by row."""
    eng = engine_of(name)
    keys = keys_of(eng, (1, 2, 3))
    layout = [[(0, 1, 2), (1, 2, 3)], [(0, 2, 3), (0, 1, 3)]]
    for level in sorted({0, eng.num_levels - 2}):
        W = matrix(eng, level, layout, seed=5 + level)
        X = tokens(eng, level, 2, 4, seed=30)
        want = [eng.lt_matmul(W, cts, keys) for cts in X]
        with native_calls(eng) as seen:
            got3 = eng.lt_matmul_batch(W, X[:3], keys)
            got4 = eng.lt_matmul_batch(W, X, keys)
        assert seen == [2, 4]
        assert all_same(got3, want[:3]) and all_same(got4, want), (name, level)
        del W, X, want, got3, got4
    del eng, keys
    torch.cuda.empty_cache()


@pytest.mark.parametrize("params", [LT, dict(LT, logN=12)])
def test_gpu_batch_equals_the_loop_of_the_checker(params):
    """logN 13 (the native call: a group of 2 and a straggler) and logN 12 (the GPU engine itself takes the loop) against the
    checker engine's loop of lt_matmul; B = 3, levels 0 and 2."""
    from liberate_fhe_amd.fhe import ckks_engine
    from tests.oracle_backend import OracleBackend
    got, want = [], []
    H = ckks_engine(devices=["cuda:0"], **params)
    C = ckks_engine(devices=["cpu"], backend=OracleBackend(), **params)
    native = params["logN"] == 13
    assert (H._native_level(0) is not None) == native
    layout = [[(0, 1, 5), None, (2,)], [(1, 2), None, (0, 2, 5)]]
    for eng, out in ((H, got), (C, want)):
        keys = keys_of(eng, (1, 2, 5))
        for level in (0, 2):
            W = matrix(eng, level, layout)
            X = tokens(eng, level, 3, 3, seed=70)
            if eng is H:
                with native_calls(eng) as seen:
                    res = eng.lt_matmul_batch(W, X, keys)
                assert seen == ([2] if native else [])
            else:
                res = [eng.lt_matmul(W, cts, keys) for cts in X]
            out += [words(o) for r in res for o in r]
    assert len(got) == len(want) == 12
    assert all(torch.equal(a[c], b[c]) for a, b in zip(got, want) for c in range(2))


def test_compact_keys_give_the_same_words():
    eng = engine_of("sb41")
    sk = eng.create_secret_key()
    layout = [[(0, 1, 3), (2,)], [None, (0, 1, 2, 3)]]
    keys = [eng.create_rotation_key(sk, d) for d in (1, 2, 3)]
    W = matrix(eng, 1, layout)
    X = tokens(eng, 1, 2, 6)
    want = [eng.lt_matmul(W, cts, keys) for cts in X]
    with native_calls(eng) as seen:
        assert all_same(eng.lt_matmul_batch(W, X, keys), want)
        for k in keys:
            eng.compact_key(k)
        assert all_same(eng.lt_matmul_batch(W, X, keys), want)
    assert seen == [4, 2, 4, 2]


def test_tuning_knobs_change_no_word():
    """LF_TUNE_DIGIT_PLANES (1 / 0), LF_TUNE_MORE_PLANES (3 / 0) and LF_TUNE_KS_EXT_COLS_MAX (column / LDS-tiled extension), in
    the combinations of tests/test_linear_transform_batch_gpu.py: six tokens (4 + 2), 2 x 2 blocks, nine keys in one column."""
    from liberate_fhe_amd._native import lib
    eng = engine_of("sb41")
    keys = keys_of(eng, NINE)
    W = matrix(eng, 0, [[(0,) + NINE, (0, 1)], [(1, 3, 9), (2,)]])
    X = tokens(eng, 0, 2, 6, seed=12)
    want = [eng.lt_matmul(W, cts, keys) for cts in X]
    old = (lib.lf_tune(3, -1), lib.lf_tune(5, -1), lib.lf_tune(1, -1))
    outs = []
    try:
        with native_calls(eng) as seen:
            for planes, more, cols in ((1, 3, 5), (0, 3, 5), (1, 0, 5), (1, 3, 0), (0, 0, 0)):
                lib.lf_tune(3, planes), lib.lf_tune(5, more), lib.lf_tune(1, cols)
                outs.append(eng.lt_matmul_batch(W, X, keys))
    finally:
        lib.lf_tune(3, old[0]), lib.lf_tune(5, old[1]), lib.lf_tune(1, old[2])
    assert seen == [4, 2] * 5
    assert len(outs) == 5 and all(all_same(out, want) for out in outs)


EDGE_CONFIGS = (("sb40_K1", 1), ("sb41_K2", 1), ("sb45_K8", 1))
EDGE_TRIPLES = (("top", "top", "top"), ("mixed", "top", "mixed"))
EDGE_STEPS = tuple(range(1, 9))
# 2 x 2: column 0 has the full set of 9 slots (step 0 and 8 keyed steps) in both of its blocks, so that every accumulator of the
# launch takes 9 terms; column 1 comes second: its launch reads, adds to and writes the sums of column 0 (fresh = 0)
EDGE_LAYOUT = [[(0,) + EDGE_STEPS, (0, 1)], [(0,) + EDGE_STEPS, (1,)]]
_EDGE_KEYS = {}


def edge_keys(cfg, eng, pattern):
    """step -> rotation key of edge words; the keys of ONE configuration are kept, those of the previous one are dropped"""
    if _EDGE_KEYS.get("cfg") != cfg:
        _EDGE_KEYS.clear()
        _EDGE_KEYS["cfg"] = cfg
    key = (id(eng), pattern)
    if key not in _EDGE_KEYS:
        _EDGE_KEYS[key] = {s: edge_key(eng, pattern, 100 + s, origin=f"rotation key:{s}") for s in EDGE_STEPS}
    return _EDGE_KEYS[key]


@pytest.mark.parametrize("last", [False, True])
@pytest.mark.parametrize("patterns", EDGE_TRIPLES)
@pytest.mark.parametrize("cfg", EDGE_CONFIGS)
def test_worst_case_words_against_the_checker_loop(cfg, patterns, last):
    """The range argument beside lt_block_productsb_kernel: pairs below 2q times diagonal words below 2q, every accumulator
    reduced after each of its 9 terms, and the read - add - write of a second input.  Ciphertexts, keys and diagonals on the
    bounds (tests/helpers.py), four tokens (two tiles of one group), at level 0 and at L - 2, word for word against the checker
    engine's loop of lt_matmul."""
    from tests.test_engine_edges_gpu import engines
    H, C = engines(*cfg)
    level = H.num_levels - 2 if last else 0
    res = []
    for eng in (H, C):
        W = [[edge_diagonals(eng, level, st, patterns[2], 40 + 8 * o + i) for i, st in enumerate(row)] for o, row in enumerate(EDGE_LAYOUT)]
        X = [[edge_ciphertext(eng, level, patterns[0], 20 + level + 2 * t + i) for i in range(2)] for t in range(4)]
        keys = edge_keys(cfg, eng, patterns[1])
        if eng is H:
            with native_calls(eng) as seen:
                res.append(eng.lt_matmul_batch(W, X, keys))
            assert seen == [4]
        else:
            res.append([eng.lt_matmul(W, cts, keys) for cts in X])
    assert all_same(*res), (cfg, patterns, level)


def test_block_matrix_times_three_token_vectors_with_real_keys():
    """logN 13 (4096 slots), real keys: a 2 x 2 block matrix of five-diagonal wrapping bands over three token vectors of two fresh
    ciphertexts.  The words are the loop's; the decryption error against the plain block product is printed and held to the bound
    tests/test_lt_matmul_gpu.py holds lt_matmul to for the same construction: at most 2 x the error of the loop of
    linear_transform + cc_add on the same ciphertexts, diagonals and keys."""
    from liberate_fhe_amd.fhe import ckks_engine
    eng = ckks_engine(devices=["cuda:0"], **LT)
    sk = eng.create_secret_key()
    pk = eng.create_public_key(sk)
    n = eng.num_slots
    rng = np.random.default_rng(21)
    steps = (0, 1, 2, n - 2, n - 1)
    D = [[{s: rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n) for s in steps} for _ in range(2)] for _ in range(2)]
    W = [[eng.encode_diagonals(D[o][i], 0) for i in range(2)] for o in range(2)]
    keys = [eng.create_rotation_key(sk, s) for s in eng.lt_matmul_steps(W)]
    assert len(keys) == 4
    ms = [[rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n) for _ in range(2)] for _ in range(3)]
    X = [[eng.encorypt(m, pk) for m in tok] for tok in ms]
    with native_calls(eng) as seen:
        got = eng.lt_matmul_batch(W, X, keys)
    assert seen == [2]
    assert all_same(got, [eng.lt_matmul(W, cts, keys) for cts in X])
    for t, (g, cts, m) in enumerate(zip(got, X, ms)):
        # (M x)[j] = sum_s diag_s[j] x[j - s]: the diagonal times the vector rotated by s (encdec.matrix_diagonals)
        want = [sum(D[o][i][s] * np.roll(m[i], s) for i in range(2) for s in steps) for o in range(2)]
        loop = [eng.cc_add(eng.linear_transform(cts[0], W[o][0], keys), eng.linear_transform(cts[1], W[o][1], keys)) for o in range(2)]
        e_mat = max(np.abs(eng.decrode(a, sk) - w).max() for a, w in zip(g, want))
        e_loop = max(np.abs(eng.decrode(a, sk) - w).max() for a, w in zip(loop, want))
        print(f"logN 13, 2 x 2 blocks of 5 diagonals, token {t}: max abs error lt_matmul_batch {e_mat:.3e}, loop of linear_transform + "
              f"cc_add {e_loop:.3e}, largest entry {max(np.abs(w).max() for w in want):.2f}")
        assert e_mat <= 2 * e_loop, (t, e_mat, e_loop)
