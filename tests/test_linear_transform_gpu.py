"""Linear transforms on the GPU: lf_linear_transform (one native call, the diagonal-weighted gathered inner product
ks_inner_lt_kernel) against the engine's orchestration of existing steps, against the checker engine, with compact keys, under the
tuning knobs, on two logical devices, and decrypted with real keys against the loop of rotate_hoisted + mc_mult + cc_add."""
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


def step_sets(steps=STEPS):
    """k = 1, 2, 4, 5, 7 keys without and with step 0, and step 0 alone."""
    sets = [tuple(steps[:n]) for n in (1, 2, 4, 5, 7)]
    return sets + [(0,) + s for s in sets] + [(0,)]


def run(eng, ct, keys, native, sets):
    be = eng.backend
    old = be.native_ops
    be.native_ops = native
    try:
        assert (eng._native_level(ct.level) is not None) == native
        return [eng.linear_transform(ct, synth.diagonals(eng, 7, ct.level, s), keys) for s in sets]
    finally:
        be.native_ops = old


def check_native_equals_orchestrated(eng, levels):
    keys = keys_of(eng)
    sets = step_sets()
    for level in levels:
        ct = synth.ciphertext(eng, 90 + level, level)
        nat, orc = run(eng, ct, keys, True, sets), run(eng, ct, keys, False, sets)
        for s, a, b in zip(sets, nat, orc):
            assert a.level == level + 1
            assert same(a, b), (level, s)


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
    check_native_equals_orchestrated(eng, sorted({0, 1, L - 2}))


@pytest.mark.gpu
@pytest.mark.parametrize("params", [LT, dict(logN=12, num_scales=5, num_special_primes=2, is_secured=False)])
def test_gpu_equals_the_checker(params):
    """logN 13 (the native call) and logN 12 (orchestrated only: the unfused steps, index_select) against the checker engine."""
    from liberate_fhe_amd.fhe import ckks_engine
    from tests.oracle_backend import OracleBackend
    got, want = [], []
    sets = [(1,), (0,), (0, 1, 2), (1, 2, 5, 11, 3), (0, 1, 2, 5, 11, 3, 700)]
    for eng, out in ((ckks_engine(devices=["cuda:0"], **params), got), (ckks_engine(devices=["cpu"], backend=OracleBackend(), **params), want)):
        keys = keys_of(eng, STEPS[:6])
        for level in (0, 2):
            ct = synth.ciphertext(eng, 70 + level, level)
            out += [words(eng.linear_transform(ct, synth.diagonals(eng, 9, level, s), keys)) for s in sets]
    assert len(got) == len(want) == 10
    assert all(torch.equal(a[c], b[c]) for a, b in zip(got, want) for c in range(2))


@pytest.mark.gpu
def test_compact_keys_give_the_same_words():
    from liberate_fhe_amd.fhe import ckks_engine
    eng = ckks_engine(devices=["cuda:0"], **GOLD["sb41"]["params"])
    sk = eng.create_secret_key()
    steps = (1, 3, 6, 9, 12)
    keys = [eng.create_rotation_key(sk, d) for d in steps]
    ct = synth.ciphertext(eng, 5, 1)
    diags = synth.diagonals(eng, 6, 1, (0,) + steps)
    want = eng.linear_transform(ct, diags, keys)
    for k in keys:
        eng.compact_key(k)
    assert same(eng.linear_transform(ct, diags, keys), want)
    eng.backend.native_ops = False
    try:
        assert same(eng.linear_transform(ct, diags, keys), want)
    finally:
        eng.backend.native_ops = True


@pytest.mark.gpu
def test_tuning_knobs_change_no_word():
    """LF_TUNE_DIGIT_PLANES (1 / 0), LF_TUNE_MORE_PLANES (3 / 0) and LF_TUNE_KS_EXT_COLS_MAX (column / LDS-tiled extension), on the
    native call and on the orchestrated path."""
    from liberate_fhe_amd._native import lib
    from liberate_fhe_amd.fhe import ckks_engine
    eng = ckks_engine(devices=["cuda:0"], **GOLD["sb41"]["params"])
    keys = keys_of(eng)
    ct = synth.ciphertext(eng, 12, 0)
    diags = synth.diagonals(eng, 13, 0, (0,) + STEPS)
    old = (lib.lf_tune(3, -1), lib.lf_tune(5, -1), lib.lf_tune(1, -1))
    outs = []
    try:
        for planes, more, cols in ((1, 3, 5), (0, 3, 5), (1, 0, 5), (1, 3, 0), (0, 0, 0)):
            lib.lf_tune(3, planes), lib.lf_tune(5, more), lib.lf_tune(1, cols)
            outs.append(eng.linear_transform(ct, diags, keys))
            eng.backend.native_ops = False
            try:
                outs.append(eng.linear_transform(ct, diags, keys))
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
        r = eng.linear_transform(synth.ciphertext(eng, 8, 0), synth.diagonals(eng, 2, 0, (0,) + STEPS[:3]), keys)
        res.append(natural_rows(eng, r))
        del eng, keys, r
        torch.cuda.empty_cache()
    for x, y in zip(*res):
        assert x.shape == y.shape and (x == y).all()


def baseline_loop(eng, ct, diag_by_step, keys_by_step):
    """Existing ops only: rotate_hoisted, mc_mult per diagonal, cc_add (step 0: a plain mc_mult)."""
    steps = [s for s in diag_by_step if s]
    acc = eng.mc_mult(diag_by_step[0], ct) if 0 in diag_by_step else None
    for s, r in zip(steps, eng.rotate_hoisted(ct, [keys_by_step[s] for s in steps])):
        t = eng.mc_mult(diag_by_step[s], r)
        acc = t if acc is None else eng.cc_add(acc, t)
    return acc


@pytest.mark.gpu
def test_real_keys_decrypt_no_worse_than_the_loop_of_existing_ops():
    """silver, real keys, x = cc_mult(enc(m1), enc(m2)), diagonals uniform in [-1, 1] for steps {0, 1, 2, 5, 11, N/8}:
    max |decrode(linear_transform(x)) - sum diag * np.roll(m1 m2, step)| is at most 2 x the same quantity of the loop
    rotate_hoisted + mc_mult + cc_add on the same inputs (both are sums of the same key-switch noises and encode roundings; the
    new op rounds once in the mod-down and the rescale instead of once per diagonal; 2 x covers the spread of a maximum over
    2^14 slots).  Both errors are printed."""
    from liberate_fhe_amd.fhe import ckks_engine, presets
    eng = ckks_engine(**{**presets.params["silver"], "devices": ["cuda:0"]})
    sk = eng.create_secret_key()
    pk = eng.create_public_key(sk)
    evk = eng.create_evk(sk)
    N = eng.ctx.N
    steps = (0, 1, 2, 5, 11, N // 8)
    keys = {s: eng.create_rotation_key(sk, s) for s in steps if s}
    np.random.seed(5)
    m1, m2 = eng.example(-1, 1), eng.example(-1, 1)
    diag = {s: eng.example(-1, 1) for s in steps}
    x = eng.cc_mult(eng.encorypt(m1, pk), eng.encorypt(m2, pk), evk)
    want = sum(diag[s] * np.roll(m1 * m2, s) for s in steps)
    got = eng.linear_transform(x, eng.encode_diagonals(diag, x.level), keys)
    assert got.level == x.level + 1
    err_new = np.abs(eng.decrode(got, sk) - want).max()
    err_loop = np.abs(eng.decrode(baseline_loop(eng, x, diag, keys), sk) - want).max()
    print(f"silver: linear_transform max abs error {err_new:.3e}, loop of existing ops {err_loop:.3e}, largest entry {np.abs(want).max():.2f}")
    assert err_new <= 2 * err_loop, (err_new, err_loop)


@pytest.mark.gpu
def test_matrix_vector_product_with_real_keys():
    """logN 13 (4096 slots), real keys: a five-diagonal wrapping band matrix M (steps 0, 1, 2, n - 2, n - 1) through
    matrix_diagonals; linear_transform decrypts to M @ m with at most 2 x the error of the loop of existing ops."""
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
    dg = encdec.matrix_diagonals(M)
    assert sorted(dg) == sorted(steps)
    keys = {s: eng.create_rotation_key(sk, s) for s in steps if s}
    np.random.seed(6)
    m = eng.example(-1, 1)
    ct = eng.encorypt(m, pk)
    want = M @ m
    err_new = np.abs(eng.decrode(eng.linear_transform(ct, dg, keys), sk) - want).max()
    err_loop = np.abs(eng.decrode(baseline_loop(eng, ct, dg, keys), sk) - want).max()
    print(f"logN 13 band matrix: linear_transform max abs error {err_new:.3e}, loop of existing ops {err_loop:.3e}, largest entry {np.abs(want).max():.2f}")
    assert err_new <= 2 * err_loop, (err_new, err_loop)
