"""lt_matmul_bsgs on the GPU: lf_lt_matmul_bsgs (one native call: lf_lt_matmul's input-major phase over the pairs of an output and
a giant step, then per keyed giant step the outputs that have it in groups of 4, 2 or 1 through one mod-down, one digit launch, one
forward pass and ks_inner_giantb_kernel, then the tail per group of outputs) against the engine's orchestration of existing steps,
against the checker engine, the three consequences of the definition, giant groups of 1, compact keys, more keyed sums than one
call takes, and decrypted with real keys against the loop of BSGS linear_transform + cc_add on the same inputs."""
import json
import os

import numpy as np
import pytest
import torch

from liberate_fhe_amd.utils import synth
from tests.test_lt_matmul_bsgs_cpu import LAYOUT, LT, N1, keys_for, layer, matmul_bsgs_errors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "engine_digests.json")))


def words(ct):
    return [torch.cat([t.cpu() for t in comp]) for comp in ct.data]


def same(a, b):
    return a.level == b.level and all(torch.equal(x, y) for x, y in zip(words(a), words(b)))


def run(eng, W, cts, keys, native):
    be = eng.backend
    old = be.native_ops
    be.native_ops = native
    try:
        assert (eng._native_level(cts[0].level) is not None) == native
        return eng.lt_matmul_bsgs(W, cts, keys)
    finally:
        be.native_ops = old


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["silver", "sb45", "sb41", "gold", "logN17"])
def test_native_call_equals_the_orchestrated_steps(name):
    """The reference layout (giant groups of 4 + 1, 2 and 1, tail groups of 4 + 2, a zeroed accumulator, an output without a giant
    phase, a column without keys) at levels 0, 1 and L - 2: word for word."""
    from liberate_fhe_amd.fhe import ckks_engine, presets
    if name in ("silver", "gold"):
        params = dict(presets.params[name])
        params.pop("devices", None)
    elif name == "logN17":
        params = dict(logN=17, num_scales=3, num_special_primes=2, is_secured=False)
    else:
        params = GOLD[name]["params"]                                   # fp64-class and integer-class rows mixed
    eng = ckks_engine(devices=["cuda:0"], **params)
    L = eng.num_levels
    keys = keys_for(eng)
    for level in sorted({0, 1, L - 2}):
        W, cts = layer(eng, level)
        nat, orc = run(eng, W, cts, keys, True), run(eng, W, cts, keys, False)
        assert len(nat) == len(orc) == 6
        for o, (a, b) in enumerate(zip(nat, orc)):
            assert a.level == level + 1
            assert same(a, b), (level, o)
        del W, cts, nat, orc


@pytest.mark.gpu
@pytest.mark.parametrize("params", [LT, dict(logN=12, num_scales=5, num_special_primes=2, is_secured=False)])
def test_gpu_equals_the_checker(params):
    """logN 13 (the native call) and logN 12 (orchestrated only: the unfused steps, index_select) against the checker engine."""
    from liberate_fhe_amd.fhe import ckks_engine
    from tests.oracle_backend import OracleBackend
    got, want = [], []
    for eng, out in ((ckks_engine(devices=["cuda:0"], **params), got), (ckks_engine(devices=["cpu"], backend=OracleBackend(), **params), want)):
        assert (eng._native_level(0) is not None) == (out is got and params["logN"] == 13)
        keys = keys_for(eng)
        for level in (0, 2):
            W, cts = layer(eng, level)
            out += [words(o) for o in eng.lt_matmul_bsgs(W, cts, keys)]
    assert len(got) == len(want) == 12
    assert all(torch.equal(a[c], b[c]) for a, b in zip(got, want) for c in range(2))


@pytest.mark.gpu
def test_the_three_consequences_on_the_gpu():
    """sb41, level 1: one input gives linear_transform's BSGS words; giant step 0 alone gives lt_matmul's on the flat-tagged packs;
    output o is that of row o alone, whatever group its giant steps ran in."""
    from liberate_fhe_amd.fhe import ckks_engine
    eng = ckks_engine(devices=["cuda:0"], **GOLD["sb41"]["params"])
    keys = keys_for(eng)
    ct = synth.ciphertext(eng, 4, 1)
    sets = [LAYOUT[0][0], LAYOUT[1][0], LAYOUT[4][0], (0,), (8, 9)]
    W = [[synth.diagonals_bsgs(eng, 9 + o, 1, st, N1)] for o, st in enumerate(sets)]
    got = eng.lt_matmul_bsgs(W, [ct], keys)
    assert len(got) == len(sets)
    for o, g in enumerate(got):
        assert same(g, eng.linear_transform(ct, W[o][0], keys)), o
    layout = [[(0, 1, 2, 3), (0,), (1, 3)], [None, (0,), (2,)], [(1, 2), None, (0, 3)]]
    Wb, cts = layer(eng, 1, layout=layout)
    Wf = [[None if st is None else synth.diagonals(eng, 7 + 8 * o + i, 1, st) for i, st in enumerate(row)] for o, row in enumerate(layout)]
    assert all(same(a, b) for a, b in zip(eng.lt_matmul_bsgs(Wb, cts, keys), eng.lt_matmul(Wf, cts, keys)))
    W, cts = layer(eng, 1)
    got = eng.lt_matmul_bsgs(W, cts, keys)
    for o in range(6):
        assert same(eng.lt_matmul_bsgs([W[o]], cts, keys)[0], got[o]), o


@pytest.mark.gpu
def test_giant_groups_of_one_give_the_words_of_groups_of_four():
    """lt_matmul_bsgs_group = 1 (the single kernel for every keyed sum) and 2 against 4, on sb41 (both classes of rows)."""
    from liberate_fhe_amd.fhe import ckks_engine
    eng = ckks_engine(devices=["cuda:0"], **GOLD["sb41"]["params"])
    keys = keys_for(eng)
    W, cts = layer(eng, 0)
    assert eng.lt_matmul_bsgs_group == 4
    want = eng.lt_matmul_bsgs(W, cts, keys)
    try:
        for group in (1, 2):
            eng.lt_matmul_bsgs_group = group
            got = eng.lt_matmul_bsgs(W, cts, keys)
            assert all(same(g, w) for g, w in zip(got, want)), group
    finally:
        del eng.lt_matmul_bsgs_group
    assert eng.lt_matmul_bsgs_group == 4


@pytest.mark.gpu
def test_compact_keys_give_the_same_words():
    from liberate_fhe_amd.fhe import ckks_engine
    eng = ckks_engine(devices=["cuda:0"], **GOLD["sb41"]["params"])
    sk = eng.create_secret_key()
    layout = [[(0, 1, 3, 4, 5), (2, 6)], [None, (0, 1, 2, 3, 7)], [(5,), (4,)]]
    keys = [eng.create_rotation_key(sk, d) for d in (1, 2, 3, 4)]
    W, cts = layer(eng, 1, layout=layout)
    want = eng.lt_matmul_bsgs(W, cts, keys)
    for k in keys:
        eng.compact_key(k)
    for native in (True, False):
        got = run(eng, W, cts, keys, native)
        assert all(same(g, w) for g, w in zip(got, want)), native


@pytest.mark.gpu
def test_more_keyed_sums_than_one_call_takes():
    """54 outputs of 5 keyed giant steps each at logN 13 (270 keyed sums, one call takes 256): the engine's split over two native
    calls gives the rows taken one at a time."""
    from liberate_fhe_amd.fhe import ckks_engine
    eng = ckks_engine(devices=["cuda:0"], **LT)
    k_out = 54
    giants = (4, 8, 12, 16, 20)
    assert k_out * len(giants) > eng.backend.lt_matmul_bsgs_max_sums >= (k_out - 3) * len(giants)
    keys = keys_for(eng, (1,) + giants)
    D = [synth.diagonals_bsgs(eng, 3 + j, 0, tuple(g + (j + g // 4) % 2 for g in (0,) + giants), N1) for j in range(2)]
    cts = [synth.ciphertext(eng, 20 + i, 0) for i in range(2)]
    W = [[D[o % 2], None if o % 4 == 1 else D[(o + 1) % 2]] for o in range(k_out)]
    assert len(eng._lt_matmul_bsgs_calls([[None if b is None else eng.diagonal_steps(b) for b in row] for row in W], N1)) == 2
    got = eng.lt_matmul_bsgs(W, cts, keys)
    assert len(got) == k_out
    one = {}
    for o, g in enumerate(got):
        kind = (o % 2, o % 4 == 1)                                        # (the rows repeat: four distinct ones)
        if kind not in one:
            one[kind] = eng.lt_matmul_bsgs([W[o]], cts, keys)[0]
        assert same(g, one[kind]), o


@pytest.mark.gpu
def test_real_keys_decrypt_within_twice_the_loop_on_silver():
    """silver, real keys, fresh ciphertexts, 2 x 2 blocks of 15 diagonals (random 8 x 8 blocks on the diagonal of the slot matrix:
    steps -7 .. 7, n1 = 4, three keyed giant steps): max |decrode - numpy product| over both outputs is at most 2 x that of the loop
    of BSGS linear_transform + cc_add on the same ciphertexts, diagonals and keys, run on the GPU (the project's margin for a
    maximum over the slots between two roundings of one quantity).  Both errors are printed."""
    from liberate_fhe_amd.fhe import ckks_engine, presets
    eng = ckks_engine(**{**presets.params["silver"], "devices": ["cuda:0"]})
    sk = eng.create_secret_key()
    pk = eng.create_public_key(sk)
    rng = np.random.default_rng(12)
    ns = eng.num_slots
    ms = [rng.uniform(-1, 1, ns) + 1j * rng.uniform(-1, 1, ns) for _ in range(2)]
    cts = [eng.encorypt(m, pk) for m in ms]
    e_mat, e_loop, nkeys, giants = matmul_bsgs_errors(eng, sk, cts, ms, rng)
    assert nkeys == 6 and giants == [0, 4, ns - 8, ns - 4]
    print(f"silver, 2 x 2 blocks of 15 diagonals, n1 = 4, 6 keys: max abs error lt_matmul_bsgs {e_mat:.3e}, "
          f"loop of BSGS linear_transform + cc_add {e_loop:.3e}")
    assert e_mat <= 2 * e_loop, (e_mat, e_loop)
