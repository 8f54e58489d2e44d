"""rotate_sum_batch / inner_sum_batch on the GPU: lf_rotate_sum_batch (one native call; groups of 4 and 2 ciphertexts through
ks_inner_rsumb_kernel, which loops over the keys of a launch with one accumulator pair per ciphertext) against the loop of
rotate_sum that defines its words — at logN 13 over every grouping and key count, at the presets, against the checker engine,
with compact keys, under the tuning knobs, at worst-case words (the test of the kernel's range argument) and once with real keys.
No tolerance anywhere: every comparison is torch.equal."""
import json
import os
import warnings

import numpy as np
import pytest
import torch

from liberate_fhe_amd.utils import synth
from tests.helpers import edge_ciphertext, edge_key
from tests.test_inner_sum_cpu import lazy_ciphertext

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore", category=UserWarning)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "engine_digests.json")))
LT = dict(logN=13, num_scales=5, num_special_primes=2, is_secured=False)
STEPS = (1, 2, 5, 11, 3, 700, 9)


def keys_per_launch():
    from liberate_fhe_amd.fhe.backend import HipBackend
    return HipBackend.rsum_batch_keys_per_launch


def long_steps():
    """rsum_batch_keys_per_launch + 1 steps: the second launch re-reads the pairs the first one left"""
    return tuple(range(1, keys_per_launch() + 2))


def words(ct):
    return [torch.cat([t.cpu() for t in comp]) for comp in ct.data]


def same(a, b):
    return a.level == b.level and a.origin == b.origin and all(torch.equal(x, y) for x, y in zip(words(a), words(b)))


def keys_of(eng, steps):
    return {s: synth.key_switch_key(eng, 40 + i, origin=f"rotation key:{s}") for i, s in enumerate(steps)}


def key_sets():
    """(steps, include_self): one key, seven keys with the self term, five without, one more key than a launch takes, the self
    term alone"""
    return [((1,), False), (STEPS, True), (STEPS[:5], False), (long_steps(), True), ((), True)]


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
    """[ciphertexts per lf_rotate_sum_batch call] while the returned list lives on the backend"""
    seen, real = [], eng.backend.rotate_sum_batch_native

    def spy(plan, c0s, *a, **kw):
        seen.append(len(c0s))
        return real(plan, c0s, *a, **kw)
    eng.backend.rotate_sum_batch_native = spy
    return seen


@pytest.fixture(scope="module")
def lt_engine():
    from liberate_fhe_amd.fhe import ckks_engine
    eng = ckks_engine(devices=["cuda:0"], **LT)
    return eng, keys_of(eng, tuple(sorted(set(STEPS) | set(long_steps()))))


@pytest.mark.parametrize("level", [0, 2, "top"])
def test_native_batch_equals_the_loop_at_logN_13(lt_engine, level):
    """Levels 0, 2 and the top (one row left); B = 1, 2, 3, 4, 5, 7 ciphertexts: groups 4 + 2 + 1 and 2 + 1; the second ciphertext
    carries lazy words; every key set.  The loop is computed once per key set, over all seven."""
    eng, keys = lt_engine
    level = eng.num_levels - 1 if level == "top" else level
    assert eng._native_level(level) is not None and hasattr(eng.backend, "rotate_sum_batch_native")
    cts = [synth.ciphertext(eng, 90 + 10 * level + i, level) for i in range(7)]
    cts[1] = lazy_ciphertext(eng, 97 + level, level)
    seen = native_calls(eng)
    try:
        for steps, with_self in key_sets():
            ks = [keys[s] for s in steps]
            want = [eng.rotate_sum(ct, ks, include_self=with_self) for ct in cts]
            assert all(w.level == level for w in want)
            for B, calls in ((1, []), (2, [2]), (3, [2]), (4, [4]), (5, [4]), (7, [6])):
                del seen[:]
                got = eng.rotate_sum_batch(cts[:B], ks, include_self=with_self)
                assert seen == calls, (B, seen)
                assert len(got) == B and all(same(g, w) for g, w in zip(got, want)), (level, steps, with_self, B)
    finally:
        del eng.backend.rotate_sum_batch_native


def test_a_member_that_is_not_contiguous_takes_the_loop_and_keeps_its_place(lt_engine):
    eng, keys = lt_engine
    level = 1
    cts = [synth.ciphertext(eng, 50 + i, level) for i in range(6)]
    ks = [keys[s] for s in STEPS]
    want = [eng.rotate_sum(ct, ks) for ct in cts]
    cts[2] = strided(eng, cts[2])
    assert not cts[2].data[0][0].is_contiguous()
    seen = native_calls(eng)
    try:
        got = eng.rotate_sum_batch(cts + [cts[0]], ks)      # six that qualify (4 + 2), one straggler, one repeated
    finally:
        del eng.backend.rotate_sum_batch_native
    assert seen == [6]
    assert all(same(g, w) for g, w in zip(got, want + [want[0]]))


def test_mixed_levels_give_one_call_per_level(lt_engine):
    eng, keys = lt_engine
    levels = (0, 2, 0, 2, 0, 0, 2)
    cts = [synth.ciphertext(eng, 60 + i, lvl) for i, lvl in enumerate(levels)]
    ks = [keys[1], keys[700], keys[5]]
    want = [eng.rotate_sum(ct, ks) for ct in cts]
    seen = native_calls(eng)
    try:
        got = eng.rotate_sum_batch(cts, ks)
    finally:
        del eng.backend.rotate_sum_batch_native
    assert seen == [4, 2]
    assert all(same(g, w) for g, w in zip(got, want))


@pytest.mark.parametrize("name", ["sb45", "sb41", "logN17"])
def test_native_batch_equals_the_loop_at_the_presets(name):
    """B = 5 (a group of 4 and a straggler) at level 0 and the top, seven keys with the self term and five without; sb41 / sb45
    run both arithmetic classes row by row, logN 17 with three scales is the five-stage column split that switches spl."""
    from liberate_fhe_amd.fhe import ckks_engine
    if name == "logN17":
        params = dict(logN=17, num_scales=3, num_special_primes=2, is_secured=False)
    else:
        params = GOLD[name]["params"]
    eng = ckks_engine(devices=["cuda:0"], **params)
    keys = keys_of(eng, STEPS)
    seen = native_calls(eng)
    for level in sorted({0, eng.num_levels - 1}):
        cts = [synth.ciphertext(eng, 30 + level + i, level) for i in range(5)]
        for steps, with_self in ((STEPS, True), (STEPS[:5], False)):
            ks = [keys[s] for s in steps]
            want = [eng.rotate_sum(ct, ks, include_self=with_self) for ct in cts]
            del seen[:]
            got = eng.rotate_sum_batch(cts, ks, include_self=with_self)
            assert seen == [4]
            assert all(same(g, w) for g, w in zip(got, want)), (name, level, steps, with_self)
    del eng, keys, cts, want, got
    torch.cuda.empty_cache()


@pytest.mark.parametrize("params", [LT, dict(LT, logN=12)])
def test_gpu_batch_equals_the_loop_of_the_checker(params):
    """logN 13 (the native call: a group of 2 and a straggler) and logN 12 (the GPU engine itself takes the loop) against the
    checker engine's loop of rotate_sum; B = 3, levels 0 and 2."""
    from liberate_fhe_amd.fhe import ckks_engine
    from tests.oracle_backend import OracleBackend
    got, want = [], []
    sets = [((1,), False), ((), True), ((1, 2, 5), True), (STEPS[:6], False)]
    H = ckks_engine(devices=["cuda:0"], **params)
    C = ckks_engine(devices=["cpu"], backend=OracleBackend(), **params)
    assert (H._native_level(0) is not None) == (params["logN"] == 13)
    for eng, out in ((H, got), (C, want)):
        keys = keys_of(eng, STEPS[:6])
        for level in (0, 2):
            cts = [synth.ciphertext(eng, 70 + level + i, level) for i in range(3)]
            for steps, with_self in sets:
                ks = [keys[s] for s in steps]
                res = eng.rotate_sum_batch(cts, ks, include_self=with_self) if eng is H else \
                    [eng.rotate_sum(ct, ks, include_self=with_self) for ct in cts]
                out += [words(r) for r in res]
    assert len(got) == len(want) == 24
    assert all(torch.equal(a[c], b[c]) for a, b in zip(got, want) for c in range(2))


def test_compact_keys_give_the_same_words():
    from liberate_fhe_amd.fhe import ckks_engine
    eng = ckks_engine(devices=["cuda:0"], **GOLD["sb41"]["params"])
    sk = eng.create_secret_key()
    keys = [eng.create_rotation_key(sk, d) for d in (1, 3, 6, 9, 12)]
    cts = [synth.ciphertext(eng, 5 + i, 1) for i in range(6)]
    want = eng.rotate_sum_batch(cts, keys)
    assert all(same(w, eng.rotate_sum(ct, keys)) for w, ct in zip(want, cts))
    for k in keys:
        eng.compact_key(k)
    assert all(same(g, w) for g, w in zip(eng.rotate_sum_batch(cts, keys), want))


def test_tuning_knobs_change_no_word():
    """LF_TUNE_DIGIT_PLANES (1 / 0), LF_TUNE_MORE_PLANES (3 / 0) and LF_TUNE_KS_EXT_COLS_MAX (column / LDS-tiled extension), in
    the combinations of tests/test_inner_sum_gpu.py: seven ciphertexts (4 + 2 + 1), nine keys (two launches) and the self term."""
    from liberate_fhe_amd._native import lib
    from liberate_fhe_amd.fhe import ckks_engine
    eng = ckks_engine(devices=["cuda:0"], **GOLD["sb41"]["params"])
    ks = list(keys_of(eng, long_steps()).values())
    cts = [synth.ciphertext(eng, 12 + i, 0) for i in range(7)]
    want = [eng.rotate_sum(ct, ks) for ct in cts]
    old = (lib.lf_tune(3, -1), lib.lf_tune(5, -1), lib.lf_tune(1, -1))
    outs = []
    try:
        for planes, more, cols in ((1, 3, 5), (0, 3, 5), (1, 0, 5), (1, 3, 0), (0, 0, 0)):
            lib.lf_tune(3, planes), lib.lf_tune(5, more), lib.lf_tune(1, cols)
            outs.append(eng.rotate_sum_batch(cts, ks))
    finally:
        lib.lf_tune(3, old[0]), lib.lf_tune(5, old[1]), lib.lf_tune(1, old[2])
    assert len(outs) == 5 and all(same(g, w) for out in outs for g, w in zip(out, want))


EDGE_CONFIGS = (("sb40_K1", 1), ("sb41_K2", 1), ("sb45_K8", 1))
EDGE_PAIRS = (("top", "top"), ("mixed", "top"))
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
@pytest.mark.parametrize("patterns", EDGE_PAIRS)
@pytest.mark.parametrize("cfg", EDGE_CONFIGS)
def test_worst_case_words_against_the_checker_loop(cfg, patterns, last):
    """The range argument beside ks_inner_rsumb_kernel: an accumulator takes the balanced products of all keys and parts of a
    launch, the gathered words of c^0 and a start word before its one reduction.  Ciphertexts and keys on the bounds
    (tests/helpers.py: patterns `top` and `mixed` for the ciphertexts, keys at the top), four ciphertexts, a full launch of keys
    plus one more (so that a second launch re-reads the pairs) and the self term, at level 0 and at the top, word for word
    against the checker engine's loop of rotate_sum."""
    from tests.test_engine_edges_gpu import engines
    H, C = engines(*cfg)
    level = H.num_levels - 1 if last else 0
    res = []
    for eng in (H, C):
        cts = [edge_ciphertext(eng, level, patterns[0], 20 + level + i) for i in range(4)]
        keys = edge_keys(cfg, eng, patterns[1])
        ks = [keys[s] for s in long_steps()]
        if eng is H:
            seen = native_calls(eng)
            try:
                res.append(eng.rotate_sum_batch(cts, ks, include_self=True))
            finally:
                del eng.backend.rotate_sum_batch_native
            assert seen == [4]
        else:
            res.append([eng.rotate_sum(ct, ks, include_self=True) for ct in cts])
    assert all(same(g, w) for g, w in zip(*res)), (cfg, patterns, level)


def test_inner_sum_batch_with_real_keys():
    """logN 13 (4096 slots), real keys, three ciphertexts: inner_sum_batch at n = 16, radix 4 has the words of the loop of
    inner_sum; the decryption error against sum_j np.roll(m, j) (the loop's own, since the words are) is printed."""
    from liberate_fhe_amd.fhe import ckks_engine
    eng = ckks_engine(devices=["cuda:0"], **LT)
    sk = eng.create_secret_key()
    pk = eng.create_public_key(sk)
    keys = {s: eng.create_rotation_key(sk, s) for s in eng.inner_sum_steps(16, 1, 4)}
    np.random.seed(6)
    ms = [eng.example(-1, 1) for _ in range(3)]
    cts = [eng.encorypt(m, pk) for m in ms]
    seen = native_calls(eng)
    try:
        got = eng.inner_sum_batch(cts, 16, keys, radix=4)
    finally:
        del eng.backend.rotate_sum_batch_native
    assert seen == [2, 2]                                   # two stages of radix 4, a group of two and a straggler each
    want = [eng.inner_sum(ct, 16, keys, radix=4) for ct in cts]
    assert all(same(g, w) for g, w in zip(got, want))
    for j, (g, m) in enumerate(zip(got, ms)):
        ref = sum(np.roll(m, i) for i in range(16))
        print(f"logN 13 inner_sum_batch n=16 radix=4, ciphertext {j}: max abs error {np.abs(eng.decrode(g, sk) - ref).max():.3e}, "
              f"largest entry {np.abs(ref).max():.2f}")
