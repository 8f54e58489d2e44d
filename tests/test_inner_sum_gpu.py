"""Slot sums on the GPU: lf_rotate_sum (one native call, the gathered inner product of all keys into one accumulator pair,
ks_inner_rsum_kernel) against the engine's orchestration of existing steps, against the checker engine, with compact keys, under
the tuning knobs, on two logical devices, and inner_sum / rotate_sum decrypted with real keys against the loops of existing ops."""
import json
import os

import numpy as np
import pytest
import torch

from liberate_fhe_amd.fhe import encdec
from liberate_fhe_amd.utils import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "engine_digests.json")))
LT = dict(logN=13, num_scales=5, num_special_primes=2, is_secured=False)
STEPS = (1, 2, 5, 11, 3, 700, 9)          # seven keys: groups of 4, 2 and 1


def words(ct):
    return [torch.cat([t.cpu() for t in comp]) for comp in ct.data]


def same(a, b):
    return a.level == b.level and all(torch.equal(x, y) for x, y in zip(words(a), words(b)))


def keys_of(eng, steps=STEPS):
    return {s: synth.key_switch_key(eng, 40 + i, origin=f"rotation key:{s}") for i, s in enumerate(steps)}


def run(eng, ct, keys, native, sets):
    be = eng.backend
    old = be.native_ops
    be.native_ops = native
    try:
        assert (eng._native_level(ct.level) is not None) == native
        return [eng.rotate_sum(ct, [keys[s] for s in steps], include_self=with_self) for steps, with_self in sets]
    finally:
        be.native_ops = old


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["silver", "sb45", "sb41", "gold", "logN17"])
def test_native_call_equals_the_orchestrated_steps(name):
    """One key, seven keys (groups of 4, 2 and 1: two hand-overs through the pair) with the self term, five keys without."""
    from liberate_fhe_amd.fhe import ckks_engine, presets
    if name in ("silver", "gold"):
        params = dict(presets.params[name])
        params.pop("devices", None)
    elif name == "logN17":
        params = dict(logN=17, num_scales=3, num_special_primes=2, is_secured=False)    # the five-stage column split
    else:
        params = GOLD[name]["params"]
    eng = ckks_engine(devices=["cuda:0"], **params)
    keys = keys_of(eng)
    sets = [((1,), False), (STEPS, True), (STEPS[:5], False)]
    for level in sorted({0, 1, eng.num_levels - 1}):
        ct = synth.ciphertext(eng, 90 + level, level)
        nat, orc = run(eng, ct, keys, True, sets), run(eng, ct, keys, False, sets)
        for s, a, b in zip(sets, nat, orc):
            assert a.level == level
            assert same(a, b), (level, s)


@pytest.mark.gpu
@pytest.mark.parametrize("params", [LT, dict(logN=12, num_scales=5, num_special_primes=2, is_secured=False)])
def test_gpu_equals_the_checker(params):
    """logN 13 (the native call) and logN 12 (orchestrated only: the unfused steps, index_select) against the checker engine."""
    from liberate_fhe_amd.fhe import ckks_engine
    from tests.oracle_backend import OracleBackend
    got, want = [], []
    sets = [((1,), False), ((), True), ((1, 2), True), ((1, 2, 5, 11, 3), False), (STEPS, True)]
    for eng, out in ((ckks_engine(devices=["cuda:0"], **params), got), (ckks_engine(devices=["cpu"], backend=OracleBackend(), **params), want)):
        keys = keys_of(eng)
        for level in (0, 2):
            ct = synth.ciphertext(eng, 70 + level, level)
            out += [words(eng.rotate_sum(ct, [keys[s] for s in steps], include_self=ws)) for steps, ws in sets]
    assert len(got) == len(want) == 10
    assert all(torch.equal(a[c], b[c]) for a, b in zip(got, want) for c in range(2))


@pytest.mark.gpu
def test_compact_keys_give_the_same_words():
    from liberate_fhe_amd.fhe import ckks_engine
    eng = ckks_engine(devices=["cuda:0"], **GOLD["sb41"]["params"])
    sk = eng.create_secret_key()
    keys = [eng.create_rotation_key(sk, d) for d in (1, 3, 6, 9, 12)]
    ct = synth.ciphertext(eng, 5, 1)
    want = eng.rotate_sum(ct, keys)
    for k in keys:
        eng.compact_key(k)
    assert same(eng.rotate_sum(ct, keys), want)
    eng.backend.native_ops = False
    try:
        assert same(eng.rotate_sum(ct, keys), want)
    finally:
        eng.backend.native_ops = True


@pytest.mark.gpu
def test_tuning_knobs_change_no_word():
    """LF_TUNE_DIGIT_PLANES (1 / 0), LF_TUNE_MORE_PLANES (3 / 0) and LF_TUNE_KS_EXT_COLS_MAX (column / LDS-tiled extension), on the
    native call and on the orchestrated path."""
    from liberate_fhe_amd._native import lib
    from liberate_fhe_amd.fhe import ckks_engine
    eng = ckks_engine(devices=["cuda:0"], **GOLD["sb41"]["params"])
    keys = list(keys_of(eng).values())
    ct = synth.ciphertext(eng, 12, 0)
    old = (lib.lf_tune(3, -1), lib.lf_tune(5, -1), lib.lf_tune(1, -1))
    outs = []
    try:
        for planes, more, cols in ((1, 3, 5), (0, 3, 5), (1, 0, 5), (1, 3, 0), (0, 0, 0)):
            lib.lf_tune(3, planes), lib.lf_tune(5, more), lib.lf_tune(1, cols)
            outs.append(eng.rotate_sum(ct, keys))
            eng.backend.native_ops = False
            try:
                outs.append(eng.rotate_sum(ct, keys))
            finally:
                eng.backend.native_ops = True
    finally:
        lib.lf_tune(3, old[0]), lib.lf_tune(5, old[1]), lib.lf_tune(1, old[2])
    assert len(outs) == 10 and all(same(o, outs[0]) for o in outs[1:])


def natural_rows(eng, ct):
    """Components as [rows, N] arrays with the rows in the order of the prime chain (tests/test_engine_golden.py)."""
    dest = eng.ntt.p.destination_arrays[ct.level]
    out = []
    for comp in ct.data:
        rows = {}
        for d, t in enumerate(comp):
            arr = t.cpu().numpy()
            for r, prime in enumerate(dest[d]):
                rows[prime] = arr[r]
        out.append(np.stack([rows[k] for k in sorted(rows)]))
    return out


@pytest.mark.gpu
def test_gold_on_two_logical_devices_equals_one_device():
    """The orchestrated path with the digit exchange between two shards, row by row in prime order."""
    from liberate_fhe_amd.fhe import ckks_engine, presets
    params = {k: v for k, v in presets.params["gold"].items() if k != "devices"}
    res = []
    for n_dev in (1, 2):
        eng = ckks_engine(devices=["cuda:0"] * n_dev, **params)
        keys = keys_of(eng, STEPS[:3])
        r = eng.rotate_sum(synth.ciphertext(eng, 8, 0), list(keys.values()))
        res.append(natural_rows(eng, r))
        del eng, keys, r
        torch.cuda.empty_cache()
    for x, y in zip(*res):
        assert x.shape == y.shape and (x == y).all()


@pytest.fixture(scope="module")
def silver():
    from liberate_fhe_amd.fhe import ckks_engine, presets
    eng = ckks_engine(**{**presets.params["silver"], "devices": ["cuda:0"]})
    sk = eng.create_secret_key()
    pk = eng.create_public_key(sk)
    evk = eng.create_evk(sk)
    np.random.seed(5)
    m1, m2 = eng.example(-1, 1), eng.example(-1, 1)
    x = eng.cc_mult(eng.encorypt(m1, pk), eng.encorypt(m2, pk), evk)      # shared by the cases, never modified
    return eng, sk, pk, x, m1 * m2


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["n16", "n12_strided", "n8_backwards"])
def test_real_keys_inner_sum_decrypts_no_worse_than_the_loop_of_existing_ops(silver, case):
    """silver, real keys, x = cc_mult(enc(m1), enc(m2)): max |decrode(inner_sum(x, n, stride)) - sum_j np.roll(m1 m2, j stride)| is
    at most 2 x the same quantity of the loop of existing ops on the same input — the log fold rotate_single + cc_add for the powers
    of two, rotate_hoisted + cc_add for n = 12 (both are sums of key-switch noises of the same size; 2 x covers the spread of a
    maximum over 2^14 slots, the margin of the linear-transform tests).  Both errors are printed."""
    eng, sk, pk, x, m = silver
    S = eng.num_slots
    n, stride, radix = {"n16": (16, 1, 4), "n12_strided": (12, S // 16, 4), "n8_backwards": (8, -1, 4)}[case]
    want = sum(np.roll(m, j * stride) for j in range(n))
    steps = eng.inner_sum_steps(n, stride, radix)
    if case == "n12_strided":
        assert [len(st) + 1 for _, st in encdec.inner_sum_plan(n, stride, S, radix)] == [4, 3]
    keys = {s: eng.create_rotation_key(sk, s) for s in steps}
    got = eng.inner_sum(x, n, keys, stride=stride, radix=radix)
    assert got.level == x.level
    err_new = np.abs(eng.decrode(got, sk) - want).max()
    del keys
    if n & (n - 1) == 0:          # the classic fold: log2 n rounds of a rotation and an addition
        loop = x
        for k in range(n.bit_length() - 1):
            rk = eng.create_rotation_key(sk, ((1 << k) * stride) % S)
            loop = eng.cc_add(eng.rotate_single(loop, rk), loop)
    else:                         # no fold for 12: every shifted copy from the hoisted rotations
        rks = [eng.create_rotation_key(sk, (j * stride) % S) for j in range(1, n)]
        loop = x
        for r in eng.rotate_hoisted(x, rks):
            loop = eng.cc_add(loop, r)
    err_loop = np.abs(eng.decrode(loop, sk) - want).max()
    print(f"silver inner_sum n={n} stride={stride} radix={radix}: max abs error {err_new:.3e}, loop of existing ops {err_loop:.3e}, "
          f"largest entry {np.abs(want).max():.2f}")
    assert err_new <= 2 * err_loop, (err_new, err_loop)


@pytest.mark.gpu
def test_real_keys_rotate_sum_with_a_conjugation_key(silver):
    """rotate_sum(ct, [conjk]) decrypts to 2 Re(m) within 2 x the error of cc_add(ct, conjugate(ct, conjk))."""
    eng, sk, pk, _, _ = silver
    conjk = eng.create_conjugation_key(sk)
    np.random.seed(8)
    m = eng.example(-1, 1) + 1j * eng.example(-1, 1)
    ct = eng.encorypt(m, pk)
    want = 2 * m.real
    got = eng.rotate_sum(ct, [conjk])
    assert got.level == ct.level
    err_new = np.abs(eng.decrode(got, sk) - want).max()
    err_loop = np.abs(eng.decrode(eng.cc_add(ct, eng.conjugate(ct, conjk)), sk) - want).max()
    print(f"silver rotate_sum(conjugation key): max abs error {err_new:.3e}, cc_add(ct, conjugate(ct)) {err_loop:.3e}")
    assert err_new <= 2 * err_loop, (err_new, err_loop)


@pytest.mark.gpu
def test_full_width_sum_against_engine_sum():
    """logN 13, real keys: inner_sum over all 4096 slots at radix 4 (six stages of three keys) against engine.sum (twelve fold
    rounds): every slot within 2 x engine.sum's largest error of m.sum()."""
    from liberate_fhe_amd.fhe import ckks_engine
    eng = ckks_engine(devices=["cuda:0"], **LT)
    sk = eng.create_secret_key()
    pk = eng.create_public_key(sk)
    gk = eng.create_galois_key(sk)
    S = eng.num_slots
    keys = {s: eng.create_rotation_key(sk, s) for s in eng.inner_sum_steps(S, 1, 4)}
    assert len(keys) == 18
    np.random.seed(9)
    m = eng.example(-1, 1)
    ct = eng.encorypt(m, pk)
    want = m.sum()
    got = eng.decrode(eng.inner_sum(ct, S, keys, radix=4), sk)
    ref = eng.decrode(eng.sum(ct, gk), sk)
    err_new, err_ref = np.abs(got - want).max(), np.abs(ref - want).max()
    print(f"logN 13 full-width sum: inner_sum max abs error {err_new:.3e}, engine.sum {err_ref:.3e}, sum {want:.3f}")
    assert err_new <= 2 * err_ref, (err_new, err_ref)
