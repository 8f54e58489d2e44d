"""Baby-step / giant-step linear transforms on the GPU: lf_linear_transform_bsgs (one native call: ks_inner_baby_kernel,
lt_diag_products_kernel, ks_inner_giant_kernel between the existing steps) against the engine's orchestration of existing steps,
against the checker engine, with compact keys, under the tuning knobs, on two logical devices, and decrypted with real keys
against the flat linear_transform on the same inputs."""
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
# (n1, steps): 7 baby keys (groups of 4, 2, 1) and 5 giant steps with giant 0 (launches of 4 + 1); 3 baby keys, baby 0 and
# giant 0 absent, one giant step with a single diagonal; n1 = 1 (no baby key at all); one giant step g = 0 (no giant key)
SETS = [
    (8, (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 17, 24, 30, 33)),
    (4, (5, 6, 7, 9, 14)),
    (1, (0, 1, 4)),
    (16, (0, 1, 5, 9)),
]


def words(ct):
    return [torch.cat([t.cpu() for t in comp]) for comp in ct.data]


def same(a, b):
    return a.level == b.level and all(torch.equal(x, y) for x, y in zip(words(a), words(b)))


def key_steps(eng, sets=SETS):
    out = set()
    for n1, steps in sets:
        _, babies, giants = encdec.bsgs_split(steps, eng.num_slots, n1)
        out |= {s for s in babies + giants if s}
    return sorted(out)


def keys_of(eng, steps):
    return {s: synth.key_switch_key(eng, 40 + i, origin=f"rotation key:{s}") for i, s in enumerate(steps)}


def run(eng, ct, keys, native, sets=SETS):
    be = eng.backend
    old = be.native_ops
    be.native_ops = native
    try:
        assert (eng._native_level(ct.level) is not None) == native
        return [eng.linear_transform(ct, synth.diagonals_bsgs(eng, 7, ct.level, steps, n1), keys) for n1, steps in sets]
    finally:
        be.native_ops = old


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
    keys = keys_of(eng, key_steps(eng))
    for level in sorted({0, 1, L - 2}):
        ct = synth.ciphertext(eng, 90 + level, level)
        nat, orc = run(eng, ct, keys, True), run(eng, ct, keys, False)
        for s, a, b in zip(SETS, nat, orc):
            assert a.level == level + 1
            assert same(a, b), (level, s)


@pytest.mark.gpu
@pytest.mark.parametrize("params", [LT, dict(logN=12, num_scales=5, num_special_primes=2, is_secured=False)])
def test_gpu_equals_the_checker(params):
    """logN 13 (the native call) and logN 12 (orchestrated only: the unfused steps, index_select) against the checker engine."""
    from liberate_fhe_amd.fhe import ckks_engine
    from tests.oracle_backend import OracleBackend
    got, want = [], []
    for eng, out in ((ckks_engine(devices=["cuda:0"], **params), got), (ckks_engine(devices=["cpu"], backend=OracleBackend(), **params), want)):
        keys = keys_of(eng, key_steps(eng))
        for level in (0, 2):
            ct = synth.ciphertext(eng, 70 + level, level)
            out += [words(eng.linear_transform(ct, synth.diagonals_bsgs(eng, 9, level, steps, n1), keys)) for n1, steps in SETS]
    assert len(got) == len(want) == 2 * len(SETS)
    assert all(torch.equal(a[c], b[c]) for a, b in zip(got, want) for c in range(2))


@pytest.mark.gpu
def test_one_giant_step_gives_the_flat_words_on_the_gpu():
    """n1 above every step: the BSGS kernels and the flat kernel on the same pack leave the same words."""
    from liberate_fhe_amd.fhe import ckks_engine
    eng = ckks_engine(devices=["cuda:0"], **GOLD["sb41"]["params"])
    steps = (0, 1, 2, 5, 11, 3)
    keys = keys_of(eng, [s for s in steps if s])
    ct = synth.ciphertext(eng, 4, 1)
    flat, bsgs = synth.diagonals(eng, 9, 1, steps), synth.diagonals_bsgs(eng, 9, 1, steps, 16)
    assert same(eng.linear_transform(ct, flat, keys), eng.linear_transform(ct, bsgs, keys))


@pytest.mark.gpu
def test_compact_keys_give_the_same_words():
    from liberate_fhe_amd.fhe import ckks_engine
    eng = ckks_engine(devices=["cuda:0"], **GOLD["sb41"]["params"])
    sk = eng.create_secret_key()
    n1, steps = 4, (0, 1, 3, 6, 9, 12)
    _, babies, giants = encdec.bsgs_split(steps, eng.num_slots, n1)
    keys = [eng.create_rotation_key(sk, d) for d in sorted(set(babies + giants)) if d]
    ct = synth.ciphertext(eng, 5, 1)
    diags = synth.diagonals_bsgs(eng, 6, 1, steps, n1)
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
    n1, steps = SETS[0]
    keys = keys_of(eng, key_steps(eng, SETS[:1]))
    ct = synth.ciphertext(eng, 12, 0)
    diags = synth.diagonals_bsgs(eng, 13, 0, steps, n1)
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
    """The orchestrated path with a digit exchange between two shards per giant step, row by row in prime order."""
    from liberate_fhe_amd.fhe import ckks_engine, presets
    params = {k: v for k, v in presets.params["gold"].items() if k != "devices"}
    n1, steps = 4, (0, 1, 2, 4, 5, 9)
    res = []
    for n_dev in (1, 2):
        eng = ckks_engine(devices=["cuda:0"] * n_dev, **params)
        keys = keys_of(eng, key_steps(eng, [(n1, steps)]))
        r = eng.linear_transform(synth.ciphertext(eng, 8, 0), synth.diagonals_bsgs(eng, 2, 0, steps, n1), keys)
        res.append(natural_rows(eng, r))
        del eng, keys, r
        torch.cuda.empty_cache()
    for x, y in zip(*res):
        assert x.shape == y.shape and (x == y).all()


def both_errors(eng, sk, ct, diag, n1, want):
    """(max error of the BSGS form, of the flat form, keys BSGS, keys flat) on the same ciphertext and diagonals"""
    n1, babies, giants = encdec.bsgs_split(diag, eng.num_slots, n1)
    keys = [eng.create_rotation_key(sk, s) for s in sorted(set(babies + giants)) if s]
    got = eng.linear_transform(ct, eng.encode_diagonals(diag, ct.level, bsgs=n1), keys)
    assert got.level == ct.level + 1
    err_bsgs, nb = np.abs(eng.decrode(got, sk) - want).max(), len(keys)
    del keys, got
    torch.cuda.empty_cache()
    keys = [eng.create_rotation_key(sk, s) for s in sorted({s % eng.num_slots for s in diag}) if s]
    err_flat = np.abs(eng.decrode(eng.linear_transform(ct, eng.encode_diagonals(diag, ct.level), keys), sk) - want).max()
    return err_bsgs, err_flat, nb, len(keys)


@pytest.mark.gpu
def test_real_keys_decrypt_within_twice_the_flat_form_on_silver():
    """silver, real keys, x = cc_mult(enc(m1), enc(m2)), 24 diagonals (steps 0..23) uniform in [-1, 1] over n1 = 4 (3 + 5 keys
    against 23): max |decrode - sum diag * np.roll(m1 m2, step)| is at most 2 x that of the flat linear_transform on the same
    inputs (the BSGS form adds one key-switch noise and one mod-down rounding per giant step, both at the scale of the
    unrescaled product; 2 x covers the spread of a maximum over 2^14 slots).  Both errors are printed."""
    from liberate_fhe_amd.fhe import ckks_engine, presets
    eng = ckks_engine(**{**presets.params["silver"], "devices": ["cuda:0"]})
    sk = eng.create_secret_key()
    pk = eng.create_public_key(sk)
    evk = eng.create_evk(sk)
    np.random.seed(5)
    m1, m2 = eng.example(-1, 1), eng.example(-1, 1)
    diag = {s: eng.example(-1, 1) for s in range(24)}
    x = eng.cc_mult(eng.encorypt(m1, pk), eng.encorypt(m2, pk), evk)
    want = sum(diag[s] * np.roll(m1 * m2, s) for s in diag)
    err_bsgs, err_flat, nb, nf = both_errors(eng, sk, x, diag, 4, want)
    print(f"silver, 24 diagonals, n1 = 4, keys {nb} / {nf}: BSGS max abs error {err_bsgs:.3e}, flat linear_transform {err_flat:.3e}, "
          f"largest entry {np.abs(want).max():.2f}")
    assert (nb, nf) == (8, 23)
    assert err_bsgs <= 2 * err_flat, (err_bsgs, err_flat)


@pytest.mark.gpu
def test_matrix_vector_product_with_real_keys():
    """logN 13 (4096 slots), real keys: a matrix with 64 consecutive wrapping diagonals (steps -32..31) through
    matrix_diagonals, n1 = 8 (7 + 7 keys against 63); decrypts to M @ m with at most 2 x the flat form's error."""
    from liberate_fhe_amd.fhe import ckks_engine
    eng = ckks_engine(devices=["cuda:0"], **LT)
    sk = eng.create_secret_key()
    pk = eng.create_public_key(sk)
    n = eng.num_slots
    rng = np.random.default_rng(21)
    M = np.zeros((n, n), dtype=np.complex128)
    i = np.arange(n)
    for s in range(-32, 32):
        M[i, (i - s) % n] = rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)
    dg = encdec.matrix_diagonals(M)
    assert sorted(dg) == sorted(s % n for s in range(-32, 32)) and encdec.bsgs_split(dg, n)[0] == 8
    np.random.seed(6)
    m = eng.example(-1, 1)
    ct = eng.encorypt(m, pk)
    err_bsgs, err_flat, nb, nf = both_errors(eng, sk, ct, dg, 8, M @ m)
    print(f"logN 13, 64 wrapping diagonals, n1 = 8, keys {nb} / {nf}: BSGS max abs error {err_bsgs:.3e}, flat linear_transform "
          f"{err_flat:.3e}, largest entry {np.abs(M @ m).max():.2f}")
    assert (nb, nf) == (14, 63)
    assert err_bsgs <= 2 * err_flat, (err_bsgs, err_flat)
