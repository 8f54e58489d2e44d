"""lt_matmul on the GPU: lf_lt_matmul (one native call: the BSGS path's baby sums per input, lt_block_products_kernel per input
and group of outputs, one inverse NTT / mod-down / rescale per group of outputs) against the engine's orchestration of existing
steps, against the checker engine, against linear_transform for one input, with compact keys, past the per-call cap of outputs,
and decrypted with real keys against the loop of linear_transform + cc_add on the same inputs."""
import json
import os

import numpy as np
import pytest
import torch

from liberate_fhe_amd.utils import synth
from tests.test_lt_matmul_cpu import block_diagonals

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "engine_digests.json")))
LT = dict(logN=13, num_scales=5, num_special_primes=2, is_secured=False)
KEY_STEPS = (1, 2, 3, 4, 5, 6, 7)                  # 7 distinct keys (gold: the keys are the memory of this test)
# 3 inputs x 5 outputs (output groups 4 + 1), by column:
#   0: steps 0 .. 7 over its blocks (7 keyed steps: key groups 4 + 2 + 1, and step 0), blocks in outputs 0, 2, 4 (launches 2 + 1);
#   1: step 0 only (no key, no digits, no forward pass), blocks in outputs 0, 1, 2, 4 (a launch of 4);
#   2: disjoint step sets and holes, blocks in outputs 0, 2, 3, 4.
# Output 1's first contributing input is column 1, output 3's column 2: they are written fresh there while others add.
LAYOUT = [
    [(0, 1, 2, 3, 4, 5, 6, 7), (0,), (1, 2)],
    [None, (0,), None],
    [(1, 5), (0,), (3, 4)],
    [None, None, (0, 5)],
    [(0, 2, 3, 4, 6, 7), (0,), (6, 7)],
]


def words(ct):
    return [torch.cat([t.cpu() for t in comp]) for comp in ct.data]


def same(a, b):
    return a.level == b.level and all(torch.equal(x, y) for x, y in zip(words(a), words(b)))


def keys_of(eng, steps=KEY_STEPS):
    return {s: synth.key_switch_key(eng, 40 + i, origin=f"rotation key:{s}") for i, s in enumerate(steps)}


def layer(eng, level, seed=7, layout=LAYOUT):
    """(W, cts) of the layout: one diagonals object per block (its own seed), one ciphertext per column"""
    W = [[None if st is None else synth.diagonals(eng, seed + 8 * o + i, level, st) for i, st in enumerate(row)] for o, row in enumerate(layout)]
    cts = [synth.ciphertext(eng, 90 + 3 * level + i, level) for i in range(len(layout[0]))]
    return W, cts


def run(eng, W, cts, keys, native):
    be = eng.backend
    old = be.native_ops
    be.native_ops = native
    try:
        assert (eng._native_level(cts[0].level) is not None) == native
        return eng.lt_matmul(W, cts, keys)
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
        params = dict(logN=17, num_scales=3, num_special_primes=2, is_secured=False)
    else:
        params = GOLD[name]["params"]                                   # fp64-class and integer-class rows mixed
    eng = ckks_engine(devices=["cuda:0"], **params)
    L = eng.num_levels
    keys = keys_of(eng)
    for level in sorted({0, 1, L - 2}):
        W, cts = layer(eng, level)
        nat, orc = run(eng, W, cts, keys, True), run(eng, W, cts, keys, False)
        assert len(nat) == len(orc) == 5
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
        keys = keys_of(eng)
        for level in (0, 2):
            W, cts = layer(eng, level)
            out += [words(o) for o in eng.lt_matmul(W, cts, keys)]
    assert len(got) == len(want) == 10
    assert all(torch.equal(a[c], b[c]) for a, b in zip(got, want) for c in range(2))


@pytest.mark.gpu
def test_one_input_gives_the_words_of_linear_transform_on_the_gpu():
    """sb41, 1 x 3: the block products behind the baby sums and the flat kernel leave the same words."""
    from liberate_fhe_amd.fhe import ckks_engine
    eng = ckks_engine(devices=["cuda:0"], **GOLD["sb41"]["params"])
    keys = keys_of(eng)
    ct = synth.ciphertext(eng, 4, 1)
    W = [[synth.diagonals(eng, 9 + o, 1, st)] for o, st in enumerate(((0, 1, 2, 5, 3), (4, 7), (0,)))]
    got = eng.lt_matmul(W, [ct], keys)
    assert len(got) == 3
    for o, g in enumerate(got):
        assert same(g, eng.linear_transform(ct, W[o][0], keys)), o


@pytest.mark.gpu
def test_compact_keys_give_the_same_words():
    from liberate_fhe_amd.fhe import ckks_engine
    eng = ckks_engine(devices=["cuda:0"], **GOLD["sb41"]["params"])
    sk = eng.create_secret_key()
    layout = [[(0, 1, 3), (2,)], [None, (0, 1, 2, 3)]]
    keys = [eng.create_rotation_key(sk, d) for d in (1, 2, 3)]
    W, cts = layer(eng, 1, layout=layout)
    want = eng.lt_matmul(W, cts, keys)
    for k in keys:
        eng.compact_key(k)
    for native in (True, False):
        got = run(eng, W, cts, keys, native)
        assert all(same(g, w) for g, w in zip(got, want)), native


@pytest.mark.gpu
def test_more_outputs_than_one_call_takes():
    """k_out = LF_LT_MATMUL_MAX_OUTPUTS + 1 one-diagonal blocks at logN 13: the engine's split over two native calls gives the
    outputs taken one row at a time."""
    from liberate_fhe_amd.fhe import ckks_engine
    eng = ckks_engine(devices=["cuda:0"], **LT)
    k_out = eng.backend.lt_matmul_max_outputs + 1
    assert k_out == 65
    keys = keys_of(eng, (1, 2))
    D = [synth.diagonals(eng, 3 + j, 0, (j,)) for j in range(3)]
    cts = [synth.ciphertext(eng, 20 + i, 0) for i in range(2)]
    W = [[D[o % 3], None if o % 4 == 1 else D[(o + 1) % 3]] for o in range(k_out)]
    got = eng.lt_matmul(W, cts, keys)
    assert len(got) == k_out
    for o, g in enumerate(got):
        assert same(g, eng.lt_matmul([W[o]], cts, keys)[0]), o


@pytest.mark.gpu
def test_real_keys_decrypt_within_twice_the_loop_on_silver():
    """silver, real keys, fresh ciphertexts, 2 x 2 blocks of 7 diagonals (random 4 x 4 blocks on the diagonal of the slot matrix:
    steps -3 .. 3): max |decrode - numpy product| over both outputs is at most 2 x that of the loop of linear_transform + cc_add
    on the same ciphertexts, diagonals and keys, run on the GPU (the project's margin for a maximum over the slots between two
    roundings of the same quantity).  Both errors are printed."""
    from liberate_fhe_amd.fhe import ckks_engine, presets
    eng = ckks_engine(**{**presets.params["silver"], "devices": ["cuda:0"]})
    sk = eng.create_secret_key()
    pk = eng.create_public_key(sk)
    rng = np.random.default_rng(12)
    ns = eng.num_slots
    ms = [rng.uniform(-1, 1, ns) + 1j * rng.uniform(-1, 1, ns) for _ in range(2)]
    cts = [eng.encorypt(m, pk) for m in ms]
    A = [[rng.uniform(-1, 1, (4, 4)) for _ in range(2)] for _ in range(2)]
    W = [[eng.encode_diagonals(block_diagonals(A[o][i], ns), 0) for i in range(2)] for o in range(2)]
    keys = [eng.create_rotation_key(sk, s) for s in eng.lt_matmul_steps(W)]
    assert len(keys) == 6
    want = [sum((A[o][i] @ ms[i].reshape(-1, 4).T).T.reshape(-1) for i in range(2)) for o in range(2)]
    got = eng.lt_matmul(W, cts, keys)
    loop = [eng.cc_add(eng.linear_transform(cts[0], W[o][0], keys), eng.linear_transform(cts[1], W[o][1], keys)) for o in range(2)]
    assert all(g.level == 1 for g in got)
    e_mat = max(np.abs(eng.decrode(g, sk) - w).max() for g, w in zip(got, want))
    e_loop = max(np.abs(eng.decrode(g, sk) - w).max() for g, w in zip(loop, want))
    print(f"silver, 2 x 2 blocks of 7 diagonals, 6 keys: max abs error lt_matmul {e_mat:.3e}, loop of linear_transform + cc_add {e_loop:.3e}, "
          f"largest entry {max(np.abs(w).max() for w in want):.2f}")
    assert e_mat <= 2 * e_loop, (e_mat, e_loop)
