"""Hoisted rotations on the GPU: lf_rotate_hoisted (one native call, the gathered inner product ks_inner_hoist_kernel) against the
engine's orchestration of existing steps, against the checker engine, under the tuning knobs, on two logical devices, and decrypted
with real keys."""
import json
import os

import numpy as np
import pytest
import torch

from liberate_fhe_amd.utils import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "engine_digests.json")))
ROT = dict(logN=13, num_scales=5, num_special_primes=2, is_secured=False)
DELTAS = (1, 2, 5, 11, 3, 700, 1)          # seven keys, one repeated: groups of 4, 2 and 1


def words(ct):
    return [torch.cat([t.cpu() for t in comp]) for comp in ct.data]


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(words(a), words(b)))


def keys_of(eng, deltas=DELTAS):
    return [synth.key_switch_key(eng, 40 + i, origin=f"rotation key:{d}") for i, d in enumerate(deltas)]


def run(eng, ct, keys, native):
    be = eng.backend
    old = be.native_ops
    be.native_ops = native
    try:
        assert (eng._native_level(ct.level) is not None) == native
        return [eng.rotate_hoisted(ct, keys[:n]) for n in (1, 2, 4, 5, 7)]
    finally:
        be.native_ops = old


def check_native_equals_orchestrated(eng, levels):
    keys = keys_of(eng)
    for level in levels:
        ct = synth.ciphertext(eng, 90 + level, level)
        nat, orc = run(eng, ct, keys, True), run(eng, ct, keys, False)
        for a, b in zip(nat, orc):
            assert len(a) == len(b)
            assert all(same(x, y) for x, y in zip(a, b)), level
        # result i of a set is the single-key result of key i
        assert all(same(x, run1[0]) for x, run1 in zip(nat[-1], [eng.rotate_hoisted(ct, [k]) for k in keys]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["silver", "sb45", "sb41", "gold", "logN17"])
def test_native_call_equals_the_orchestrated_steps(name):
    from liberate_fhe_amd.fhe import ckks_engine, presets
    if name in ("silver", "gold"):
        params = dict(presets.params[name])
        params.pop("devices", None)
    elif name == "logN17":
        params = dict(logN=17, num_scales=3, num_special_primes=2, is_secured=False)    # the five-stage column split
    else:
        params = GOLD[name]["params"]
    eng = ckks_engine(devices=["cuda:0"], **params)
    L = eng.num_levels
    check_native_equals_orchestrated(eng, (0, 1, L - 2) if name != "gold" else (0, L - 2))


@pytest.mark.gpu
def test_compact_keys_give_the_same_words():
    from liberate_fhe_amd.fhe import ckks_engine
    eng = ckks_engine(devices=["cuda:0"], **GOLD["sb41"]["params"])
    sk = eng.create_secret_key()
    keys = [eng.create_rotation_key(sk, d) for d in (1, 3, 6, 9, 12)]
    ct = synth.ciphertext(eng, 5, 1)
    want = eng.rotate_hoisted(ct, keys)
    for k in keys:
        eng.compact_key(k)
    assert all(same(a, b) for a, b in zip(eng.rotate_hoisted(ct, keys), want))
    eng.backend.native_ops = False
    try:
        assert all(same(a, b) for a, b in zip(eng.rotate_hoisted(ct, keys), want))
    finally:
        eng.backend.native_ops = True


@pytest.mark.gpu
@pytest.mark.parametrize("params", [ROT, dict(logN=12, num_scales=5, num_special_primes=2, is_secured=False)])
def test_gpu_equals_the_checker(params):
    """logN 13 (the native call) and logN 12 (orchestrated only: the unfused steps, index_select) against the checker engine."""
    from liberate_fhe_amd.fhe import ckks_engine
    from tests.oracle_backend import OracleBackend
    got, want = [], []
    for eng, out in ((ckks_engine(devices=["cuda:0"], **params), got), (ckks_engine(devices=["cpu"], backend=OracleBackend(), **params), want)):
        keys = keys_of(eng, DELTAS[:5])
        for level in (0, 2):
            out += [words(x) for x in eng.rotate_hoisted(synth.ciphertext(eng, 70 + level, level), keys)]
    assert all(torch.equal(a[c], b[c]) for a, b in zip(got, want) for c in range(2))


@pytest.mark.gpu
def test_tuning_knobs_change_no_word():
    """LF_TUNE_DIGIT_PLANES (1 / 0), LF_TUNE_MORE_PLANES (3 / 0) and LF_TUNE_KS_EXT_COLS_MAX (column / LDS-tiled extension)."""
    from liberate_fhe_amd._native import lib
    from liberate_fhe_amd.fhe import ckks_engine
    eng = ckks_engine(devices=["cuda:0"], **GOLD["sb41"]["params"])
    keys = keys_of(eng)
    ct = synth.ciphertext(eng, 12, 0)
    old = (lib.lf_tune(3, -1), lib.lf_tune(5, -1), lib.lf_tune(1, -1))
    outs = []
    try:
        for planes, more, cols in ((1, 3, 5), (0, 3, 5), (1, 0, 5), (1, 3, 0), (0, 0, 0)):
            lib.lf_tune(3, planes), lib.lf_tune(5, more), lib.lf_tune(1, cols)
            outs.append([words(x) for x in eng.rotate_hoisted(ct, keys)])
    finally:
        lib.lf_tune(3, old[0]), lib.lf_tune(5, old[1]), lib.lf_tune(1, old[2])
    assert all(torch.equal(a[c], b[c]) for o in outs[1:] for a, b in zip(o, outs[0]) for c in range(2))


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
        keys = keys_of(eng, DELTAS[:3])
        res.append([natural_rows(eng, x) for x in eng.rotate_hoisted(synth.ciphertext(eng, 8, 0), keys)])
        del eng, keys
        torch.cuda.empty_cache()
    for one, two in zip(*res):
        for x, y in zip(one, two):
            assert x.shape == y.shape and (x == y).all()


@pytest.mark.gpu
def test_real_keys_decrypt_to_the_rotated_product():
    """silver with real keys: the hoisted rotations of prod = cc_mult(m1, m2) decrypt to np.roll(m1 m2, delta) within 2e-7 (the
    bound rotate_single is held to); a step-0 key gives rotate_single's words."""
    from liberate_fhe_amd.fhe import ckks_engine, presets
    eng = ckks_engine(**{**presets.params["silver"], "devices": ["cuda:0"]})
    sk = eng.create_secret_key()
    pk = eng.create_public_key(sk)
    evk = eng.create_evk(sk)
    N = eng.ctx.N
    deltas = (1, 2, 5, 11, N // 8)
    keys = [eng.create_rotation_key(sk, d) for d in deltas]
    np.random.seed(5)
    m1, m2 = eng.example(-1, 1), eng.example(-1, 1)
    prod = eng.cc_mult(eng.encorypt(m1, pk), eng.encorypt(m2, pk), evk)
    for d, r in zip(deltas, eng.rotate_hoisted(prod, keys)):
        assert np.abs(eng.decrode(r, sk) - np.roll(m1 * m2, d)).max() < 2e-7, d
    k0 = eng.create_rotation_key(sk, 0)
    assert same(eng.rotate_hoisted(prod, [k0, keys[0]])[0], eng.rotate_single(prod, k0))
