"""linear_transform_batch on the GPU: lf_linear_transform_batch (one native call; groups of 4 and 2 ciphertexts through
ks_inner_ltb_kernel, which loops over the keys of a launch with the group's running sums in registers) against the loop of
linear_transform that defines its words — at logN 13 over every grouping and key count, at the presets, against the checker
engine, with compact keys, under the tuning knobs, at worst-case words (the test of the kernel's range argument) and once with
real keys.  No tolerance anywhere: every comparison is torch.equal."""
import json
import os
import warnings

import numpy as np
import pytest
import torch

from liberate_fhe_amd.fhe import encdec
from liberate_fhe_amd.utils import synth
from tests.helpers import edge_ciphertext, edge_diagonals, edge_key
from tests.test_inner_sum_cpu import lazy_ciphertext

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore", category=UserWarning)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "engine_digests.json")))
LT = dict(logN=13, num_scales=5, num_special_primes=2, is_secured=False)
STEPS = (1, 2, 5, 11, 3, 700, 9)


def keys_per_launch():
    from liberate_fhe_amd.fhe.backend import HipBackend
    return HipBackend.lt_batch_keys_per_launch


def long_steps():
    """lt_batch_keys_per_launch + 1 keyed steps: the second launch re-reads the running pairs"""
    return tuple(range(1, keys_per_launch() + 2))


def words(ct):
    return [torch.cat([t.cpu() for t in comp]) for comp in ct.data]


def same(a, b):
    return a.level == b.level and a.origin == b.origin and all(torch.equal(x, y) for x, y in zip(words(a), words(b)))


def keys_of(eng, steps):
    return {s: synth.key_switch_key(eng, 40 + i, origin=f"rotation key:{s}") for i, s in enumerate(steps)}


def step_sets():
    """1, 2, 4, 5, 7 keys without and with step 0, step 0 alone, and one more key than a launch takes"""
    sets = [tuple(STEPS[:n]) for n in (1, 2, 4, 5, 7)]
    return sets + [(0,) + s for s in sets] + [(0,), long_steps()]


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


def native_calls(eng):
    """[ciphertexts per lf_linear_transform_batch call] while the returned list lives on the backend"""
    seen, real = [], eng.backend.linear_transform_batch_native

    def spy(plan, c0s, *a, **kw):
        seen.append(len(c0s))
        return real(plan, c0s, *a, **kw)
    eng.backend.linear_transform_batch_native = spy
    return seen


@pytest.fixture(scope="module")
def lt_engine():
    from liberate_fhe_amd.fhe import ckks_engine
    eng = ckks_engine(devices=["cuda:0"], **LT)
    return eng, keys_of(eng, tuple(sorted(set(STEPS) | set(long_steps()))))


@pytest.mark.parametrize("level", [0, 2, 3])
def test_native_batch_equals_the_loop_at_logN_13(lt_engine, level):
    """Levels 0, 2 and L - 2 (one row left); B = 1, 2, 3, 4, 5, 7 ciphertexts: groups 4 + 2 + 1 and 2 + 1; the second ciphertext
    carries lazy words; every key set.  The loop is computed once per key set, over all seven."""
    eng, keys = lt_engine
    assert level <= eng.num_levels - 2 and (level != 3 or level == eng.num_levels - 2)
    assert eng._native_level(level) is not None and hasattr(eng.backend, "linear_transform_batch_native")
    cts = [synth.ciphertext(eng, 90 + 10 * level + i, level) for i in range(7)]
    cts[1] = lazy_ciphertext(eng, 97 + level, level)
    seen = native_calls(eng)
    try:
        for steps in step_sets():
            diags = synth.diagonals(eng, 7 + level, level, steps)
            want = [eng.linear_transform(ct, diags, keys) for ct in cts]
            assert all(w.level == level + 1 for w in want)
            for B, calls in ((1, []), (2, [2]), (3, [2]), (4, [4]), (5, [4]), (7, [6])):
                del seen[:]
                got = eng.linear_transform_batch(cts[:B], diags, keys)
                assert seen == calls, (B, seen)
                assert len(got) == B and all(same(g, w) for g, w in zip(got, want)), (level, steps, B)
    finally:
        del eng.backend.linear_transform_batch_native


def test_a_member_that_is_not_contiguous_takes_the_loop_and_keeps_its_place(lt_engine):
    eng, keys = lt_engine
    level = 1
    cts = [synth.ciphertext(eng, 50 + i, level) for i in range(6)]
    diags = synth.diagonals(eng, 3, level, (0,) + STEPS)
    want = [eng.linear_transform(ct, diags, keys) for ct in cts]
    cts[2] = strided(eng, cts[2])
    assert not cts[2].data[0][0].is_contiguous()
    seen = native_calls(eng)
    try:
        got = eng.linear_transform_batch(cts + [cts[0]], diags, keys)      # six that qualify (4 + 2), one straggler, one repeated
    finally:
        del eng.backend.linear_transform_batch_native
    assert seen == [6]
    assert all(same(g, w) for g, w in zip(got, want + [want[0]]))


@pytest.mark.parametrize("name", ["silver", "sb45", "sb41", "gold", "logN17"])
def test_native_batch_equals_the_loop_at_the_presets(name):
    """B = 5 (a group of 4 and a straggler) at levels 0 and L - 2, key sets (0, 1, 2, 5) and seven keys; sb41 / sb45 run both
    arithmetic classes row by row."""
    from liberate_fhe_amd.fhe import ckks_engine, presets
    if name in ("silver", "gold"):
        params = dict(presets.params[name])
        params.pop("devices", None)
    elif name == "logN17":
        params = dict(logN=17, num_scales=3, num_special_primes=2, is_secured=False)
    else:
        params = GOLD[name]["params"]
    eng = ckks_engine(devices=["cuda:0"], **params)
    keys = keys_of(eng, STEPS)
    seen = native_calls(eng)
    for level in sorted({0, eng.num_levels - 2}):
        cts = [synth.ciphertext(eng, 30 + level + i, level) for i in range(5)]
        for steps in ((0, 1, 2, 5), STEPS):
            diags = synth.diagonals(eng, 5 + level, level, steps)
            want = [eng.linear_transform(ct, diags, keys) for ct in cts]
            del seen[:]
            got = eng.linear_transform_batch(cts, diags, keys)
            assert seen == [4]
            assert all(same(g, w) for g, w in zip(got, want)), (name, level, steps)
    del eng, keys, cts, want, got
    torch.cuda.empty_cache()


@pytest.mark.parametrize("params", [LT, dict(LT, logN=12)])
def test_gpu_batch_equals_the_loop_of_the_checker(params):
    """logN 13 (the native call: a group of 2 and a straggler) and logN 12 (the GPU engine itself takes the loop) against the
    checker engine's loop of linear_transform; B = 3, levels 0 and 2."""
    from liberate_fhe_amd.fhe import ckks_engine
    from tests.oracle_backend import OracleBackend
    got, want = [], []
    sets = [(1,), (0, 1, 2), (0, 1, 2, 5, 11, 3, 700)]
    H = ckks_engine(devices=["cuda:0"], **params)
    C = ckks_engine(devices=["cpu"], backend=OracleBackend(), **params)
    assert (H._native_level(0) is not None) == (params["logN"] == 13)
    for eng, out in ((H, got), (C, want)):
        keys = keys_of(eng, STEPS[:6])
        for level in (0, 2):
            cts = [synth.ciphertext(eng, 70 + level + i, level) for i in range(3)]
            for s in sets:
                diags = synth.diagonals(eng, 9, level, s)
                res = eng.linear_transform_batch(cts, diags, keys) if eng is H else [eng.linear_transform(ct, diags, keys) for ct in cts]
                out += [words(r) for r in res]
    assert len(got) == len(want) == 18
    assert all(torch.equal(a[c], b[c]) for a, b in zip(got, want) for c in range(2))


def test_compact_keys_give_the_same_words():
    from liberate_fhe_amd.fhe import ckks_engine
    eng = ckks_engine(devices=["cuda:0"], **GOLD["sb41"]["params"])
    sk = eng.create_secret_key()
    steps = (1, 3, 6, 9, 12)
    keys = [eng.create_rotation_key(sk, d) for d in steps]
    cts = [synth.ciphertext(eng, 5 + i, 1) for i in range(6)]
    diags = synth.diagonals(eng, 6, 1, (0,) + steps)
    want = eng.linear_transform_batch(cts, diags, keys)
    assert all(same(w, eng.linear_transform(ct, diags, keys)) for w, ct in zip(want, cts))
    for k in keys:
        eng.compact_key(k)
    assert all(same(g, w) for g, w in zip(eng.linear_transform_batch(cts, diags, keys), want))


def test_tuning_knobs_change_no_word():
    """LF_TUNE_DIGIT_PLANES (1 / 0), LF_TUNE_MORE_PLANES (3 / 0) and LF_TUNE_KS_EXT_COLS_MAX (column / LDS-tiled extension), in
    the combinations of tests/test_linear_transform_gpu.py: seven ciphertexts (4 + 2 + 1), nine keys (two launches) and step 0."""
    from liberate_fhe_amd._native import lib
    from liberate_fhe_amd.fhe import ckks_engine
    eng = ckks_engine(devices=["cuda:0"], **GOLD["sb41"]["params"])
    steps = (0,) + long_steps()
    keys = keys_of(eng, long_steps())
    cts = [synth.ciphertext(eng, 12 + i, 0) for i in range(7)]
    diags = synth.diagonals(eng, 13, 0, steps)
    want = [eng.linear_transform(ct, diags, keys) for ct in cts]
    old = (lib.lf_tune(3, -1), lib.lf_tune(5, -1), lib.lf_tune(1, -1))
    outs = []
    try:
        for planes, more, cols in ((1, 3, 5), (0, 3, 5), (1, 0, 5), (1, 3, 0), (0, 0, 0)):
            lib.lf_tune(3, planes), lib.lf_tune(5, more), lib.lf_tune(1, cols)
            outs.append(eng.linear_transform_batch(cts, diags, keys))
    finally:
        lib.lf_tune(3, old[0]), lib.lf_tune(5, old[1]), lib.lf_tune(1, old[2])
    assert len(outs) == 5 and all(same(g, w) for out in outs for g, w in zip(out, want))


EDGE_CONFIGS = (("sb40_K1", 1), ("sb41_K2", 1), ("sb45_K8", 1))
EDGE_TRIPLES = (("top", "top", "top"), ("mixed", "top", "mixed"))
_EDGE_KEYS = {}


def edge_keys(cfg, eng, pattern):
    """step -> rotation key of edge words; the keys of ONE configuration are kept, those of the previous one are dropped"""
    if _EDGE_KEYS.get("cfg") != cfg:
        _EDGE_KEYS.clear()
        _EDGE_KEYS["cfg"] = cfg
    key = (id(eng), pattern)
    if key not in _EDGE_KEYS:
        _EDGE_KEYS[key] = {s: edge_key(eng, pattern, 100 + s, origin=f"rotation key:{s}") for s in long_steps()}
    return _EDGE_KEYS[key]


@pytest.mark.parametrize("last", [False, True])
@pytest.mark.parametrize("patterns", EDGE_TRIPLES)
@pytest.mark.parametrize("cfg", EDGE_CONFIGS)
def test_worst_case_words_against_the_checker_loop(cfg, patterns, last):
    """The range argument beside ks_inner_ltb_kernel: the running pairs of a launch take lt_batch_keys_per_launch balanced
    products and a start term unreduced.  Ciphertexts, keys and diagonals on the bounds (tests/helpers.py), four ciphertexts,
    a full launch of keys plus one more (so that a second launch re-reads the pairs) and the step-0 term, at level 0 and at
    L - 2, word for word against the checker engine's loop of linear_transform."""
    from tests.test_engine_edges_gpu import engines
    H, C = engines(*cfg)
    level = H.num_levels - 2 if last else 0
    steps = (0,) + long_steps()
    res = []
    for eng in (H, C):
        cts = [edge_ciphertext(eng, level, patterns[0], 20 + level + i) for i in range(4)]
        diags = edge_diagonals(eng, level, steps, patterns[2], 7 + level)
        keys = edge_keys(cfg, eng, patterns[1])
        if eng is H:
            seen = native_calls(eng)
            try:
                res.append(eng.linear_transform_batch(cts, diags, keys))
            finally:
                del eng.backend.linear_transform_batch_native
            assert seen == [4]
        else:
            res.append([eng.linear_transform(ct, diags, keys) for ct in cts])
    assert all(same(g, w) for g, w in zip(*res)), (cfg, patterns, level)


def test_matrix_times_three_vectors_with_real_keys():
    """logN 13 (4096 slots), real keys: a five-diagonal wrapping band matrix M through matrix_diagonals over three encrypted
    vectors.  The words are the loop's; the decryption error against M @ m_i (the loop's own, since the words are) is printed."""
    from liberate_fhe_amd.fhe import ckks_engine
    eng = ckks_engine(devices=["cuda:0"], **LT)
    sk = eng.create_secret_key()
    pk = eng.create_public_key(sk)
    n = eng.num_slots
    rng = np.random.default_rng(21)
    steps = (0, 1, 2, n - 2, n - 1)
    M = np.zeros((n, n), dtype=np.complex128)
    i = np.arange(n)
    for s in steps:
        M[i, (i - s) % n] = rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)
    diags = eng.encode_diagonals(encdec.matrix_diagonals(M), 0)
    keys = {s: eng.create_rotation_key(sk, s) for s in steps if s}
    np.random.seed(6)
    ms = [eng.example(-1, 1) for _ in range(3)]
    cts = [eng.encorypt(m, pk) for m in ms]
    got = eng.linear_transform_batch(cts, diags, keys)
    want = [eng.linear_transform(ct, diags, keys) for ct in cts]
    assert all(same(g, w) for g, w in zip(got, want))
    for j, (g, m) in enumerate(zip(got, ms)):
        ref = M @ m
        print(f"logN 13 band matrix, vector {j}: linear_transform_batch max abs error {np.abs(eng.decrode(g, sk) - ref).max():.3e}, "
              f"largest entry {np.abs(ref).max():.2f}")
