"""linear_transform_batch over baby-step / giant-step diagonals on the GPU: lf_linear_transform_bsgs_batch (one native call;
groups of 4 and 2 ciphertexts share every baby key through ks_inner_babyb_kernel and every giant key through
ks_inner_giantb_kernel) against the loop of linear_transform that defines its words — at logN 13 over every grouping and
every shape of the giant steps, at the presets, with compact keys, under the tuning knobs, at worst-case words against the
checker engine (the test of the kernel's range argument), at the entry's refusals and once with real keys.  No tolerance
anywhere: every comparison is torch.equal."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

from liberate_fhe_amd.fhe import encdec
from liberate_fhe_amd.utils import synth
from tests.helpers import edge_ciphertext, edge_diagonals, edge_key
from tests.test_inner_sum_cpu import lazy_ciphertext
from tests.test_linear_transform_batch_gpu import EDGE_CONFIGS, EDGE_TRIPLES, GOLD, LT, same, strided

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore", category=UserWarning)

LF_ERR_ARG = 10001
# (n1, steps): giant 0 plus two keyed giants, baby 0 present; no giant step 0 (the accumulator is zeroed); giant 0 alone (no
# giant key switch); nb = 0 with one keyed giant; no baby 0 anywhere; six giant steps (two chunks of LF_BSGS_S_PAIRS)
SETS = [
    (4, (0, 1, 2, 5, 6, 9)),
    (4, (5, 6, 9)),
    (4, (1, 2, 3)),
    (4, (8,)),
    (4, (1, 5)),
    (2, tuple(range(11))),
]
EDGE_SET = (4, (0, 1, 2, 3, 5, 6, 9))   # three baby keys and slot 0, giant 0 and two keyed giants


def key_steps(eng, sets):
    out = set()
    for n1, steps in sets:
        _, babies, giants = encdec.bsgs_split(steps, eng.num_slots, n1)
        out |= {s for s in babies + giants if s}
    return sorted(out)


def keys_of(eng, steps):
    return {s: synth.key_switch_key(eng, 40 + i, origin=f"rotation key:{s}") for i, s in enumerate(steps)}


def native_calls(eng):
    """[ciphertexts per lf_linear_transform_bsgs_batch call] while the returned list lives on the backend"""
    seen, real = [], eng.backend.linear_transform_bsgs_batch_native

    def spy(plan, c0s, *a, **kw):
        seen.append(len(c0s))
        return real(plan, c0s, *a, **kw)
    eng.backend.linear_transform_bsgs_batch_native = spy
    return seen


@pytest.fixture(scope="module")
def lt_engine():
    from liberate_fhe_amd.fhe import ckks_engine
    eng = ckks_engine(devices=["cuda:0"], **LT)
    return eng, keys_of(eng, key_steps(eng, SETS))


@pytest.mark.parametrize("level", [0, 2, 3])
def test_native_batch_equals_the_loop_at_logN_13(lt_engine, level):
    """Levels 0, 2 and L - 2 (one row left); B = 1, 2, 3, 4, 5, 7 ciphertexts: groups 4 + 2 + 1 and 2 + 1; the second ciphertext
    carries lazy words; one list holds the same object twice inside one group; every shape of SETS.  The loop is computed once
    per shape, over all seven."""
    eng, keys = lt_engine
    assert level <= eng.num_levels - 2 and (level != 3 or level == eng.num_levels - 2)
    assert eng._native_level(level) is not None and tuple(eng.lt_bsgs_batch_sizes) == (4, 2)
    cts = [synth.ciphertext(eng, 90 + 10 * level + i, level) for i in range(7)]
    cts[1] = lazy_ciphertext(eng, 97 + level, level)
    seen = native_calls(eng)
    try:
        for n1, steps in SETS:
            diags = synth.diagonals_bsgs(eng, 7 + level, level, steps, n1)
            want = [eng.linear_transform(ct, diags, keys) for ct in cts]
            assert all(w.level == level + 1 for w in want)
            for B, calls in ((1, []), (2, [2]), (3, [2]), (4, [4]), (5, [4]), (7, [6])):
                del seen[:]
                got = eng.linear_transform_batch(cts[:B], diags, keys)
                assert seen == calls, (B, seen)
                assert len(got) == B and all(same(g, w) for g, w in zip(got, want)), (level, n1, steps, B)
            del seen[:]
            got = eng.linear_transform_batch([cts[0], cts[2], cts[0], cts[1]], diags, keys)
            assert seen == [4] and got[0] is not got[2]
            assert all(same(g, want[i]) for g, i in zip(got, (0, 2, 0, 1))), (level, n1, steps, "repeated")
    finally:
        del eng.backend.linear_transform_bsgs_batch_native


def test_a_member_that_is_not_contiguous_takes_the_loop_and_keeps_its_place(lt_engine):
    eng, keys = lt_engine
    level = 1
    n1, steps = SETS[0]
    cts = [synth.ciphertext(eng, 50 + i, level) for i in range(6)]
    diags = synth.diagonals_bsgs(eng, 3, level, steps, n1)
    want = [eng.linear_transform(ct, diags, keys) for ct in cts]
    cts[2] = strided(eng, cts[2])
    assert not cts[2].data[0][0].is_contiguous()
    seen = native_calls(eng)
    try:
        got = eng.linear_transform_batch(cts + [cts[0]], diags, keys)      # six that qualify (4 + 2), one that does not, one repeated
    finally:
        del eng.backend.linear_transform_bsgs_batch_native
    assert seen == [6]
    assert all(same(g, w) for g, w in zip(got, want + [want[0]]))


@pytest.mark.parametrize("name", ["silver", "sb45", "sb41", "gold", "logN17"])
def test_native_batch_equals_the_loop_at_the_presets(name):
    """Level 0, B = 6 (a group of 4 and a group of 2), n1 = 2 with steps (0, 1, 2, 3); sb41 / sb45 run both arithmetic classes
    row by row."""
    from liberate_fhe_amd.fhe import ckks_engine, presets
    if name in ("silver", "gold"):
        params = dict(presets.params[name])
        params.pop("devices", None)
    elif name == "logN17":
        params = dict(logN=17, num_scales=3, num_special_primes=2, is_secured=False)
    else:
        params = GOLD[name]["params"]
    eng = ckks_engine(devices=["cuda:0"], **params)
    n1, steps = 2, (0, 1, 2, 3)
    keys = keys_of(eng, key_steps(eng, [(n1, steps)]))
    cts = [synth.ciphertext(eng, 30 + i, 0) for i in range(6)]
    diags = synth.diagonals_bsgs(eng, 5, 0, steps, n1)
    want = [eng.linear_transform(ct, diags, keys) for ct in cts]
    seen = native_calls(eng)
    got = eng.linear_transform_batch(cts, diags, keys)
    assert seen == [6]
    assert all(same(g, w) for g, w in zip(got, want)), name
    del eng, keys, cts, want, got
    torch.cuda.empty_cache()


def test_compact_keys_give_the_same_words():
    from liberate_fhe_amd.fhe import ckks_engine
    eng = ckks_engine(devices=["cuda:0"], **GOLD["sb41"]["params"])
    sk = eng.create_secret_key()
    n1, steps = 4, (0, 1, 3, 6, 9, 12)
    keys = [eng.create_rotation_key(sk, d) for d in key_steps(eng, [(n1, steps)])]
    cts = [synth.ciphertext(eng, 5 + i, 1) for i in range(6)]
    diags = synth.diagonals_bsgs(eng, 6, 1, steps, n1)
    seen = native_calls(eng)
    want = eng.linear_transform_batch(cts, diags, keys)
    assert all(same(w, eng.linear_transform(ct, diags, keys)) for w, ct in zip(want, cts))
    for k in keys:
        eng.compact_key(k)
    assert all(same(g, w) for g, w in zip(eng.linear_transform_batch(cts, diags, keys), want))
    assert seen == [6, 6]


def test_tuning_knobs_change_no_word():
    """LF_TUNE_DIGIT_PLANES (1 / 0), LF_TUNE_MORE_PLANES (3 / 0) and LF_TUNE_KS_EXT_COLS_MAX (column / LDS-tiled extension), in
    the combinations of tests/test_linear_transform_gpu.py: seven ciphertexts (4 + 2 + 1), three baby keys, three giant steps."""
    from liberate_fhe_amd._native import lib
    from liberate_fhe_amd.fhe import ckks_engine
    eng = ckks_engine(devices=["cuda:0"], **GOLD["sb41"]["params"])
    n1, steps = EDGE_SET
    keys = keys_of(eng, key_steps(eng, [EDGE_SET]))
    cts = [synth.ciphertext(eng, 12 + i, 0) for i in range(7)]
    diags = synth.diagonals_bsgs(eng, 13, 0, steps, n1)
    want = [eng.linear_transform(ct, diags, keys) for ct in cts]
    old = (lib.lf_tune(3, -1), lib.lf_tune(5, -1), lib.lf_tune(1, -1))
    outs = []
    seen = native_calls(eng)
    try:
        for planes, more, cols in ((1, 3, 5), (0, 3, 5), (1, 0, 5), (1, 3, 0), (0, 0, 0)):
            lib.lf_tune(3, planes), lib.lf_tune(5, more), lib.lf_tune(1, cols)
            outs.append(eng.linear_transform_batch(cts, diags, keys))
    finally:
        lib.lf_tune(3, old[0]), lib.lf_tune(5, old[1]), lib.lf_tune(1, old[2])
    assert seen == [6] * 5
    assert len(outs) == 5 and all(same(g, w) for out in outs for g, w in zip(out, want))


_EDGE_KEYS = {}


def edge_keys(cfg, eng, pattern):
    """step -> rotation key of edge words; the keys of ONE configuration are kept, those of the previous one are dropped"""
    if _EDGE_KEYS.get("cfg") != cfg:
        _EDGE_KEYS.clear()
        _EDGE_KEYS["cfg"] = cfg
    key = (id(eng), pattern)
    if key not in _EDGE_KEYS:
        _EDGE_KEYS[key] = {s: edge_key(eng, pattern, 100 + s, origin=f"rotation key:{s}") for s in key_steps(eng, [EDGE_SET])}
    return _EDGE_KEYS[key]


@pytest.mark.parametrize("last", [False, True])
@pytest.mark.parametrize("patterns", EDGE_TRIPLES)
@pytest.mark.parametrize("cfg", EDGE_CONFIGS)
def test_worst_case_words_against_the_checker_loop(cfg, patterns, last):
    """The range argument beside ks_inner_babyb_kernel: per ciphertext the digits' balanced products and one word of P c0 below
    2q, reduced once.  Ciphertexts, keys and diagonals on the bounds (tests/helpers.py), a group of four, three baby keys and
    two keyed giant steps, at level 0 and at L - 2, word for word against the checker engine's loop of linear_transform."""
    from tests.test_engine_edges_gpu import engines
    H, C = engines(*cfg)
    level = H.num_levels - 2 if last else 0
    n1, steps = EDGE_SET
    res = []
    for eng in (H, C):
        cts = [edge_ciphertext(eng, level, patterns[0], 20 + level + i) for i in range(4)]
        diags = edge_diagonals(eng, level, steps, patterns[2], 7 + level, n1)
        keys = edge_keys(cfg, eng, patterns[1])
        if eng is H:
            seen = native_calls(eng)
            try:
                res.append(eng.linear_transform_batch(cts, diags, keys))
            finally:
                del eng.backend.linear_transform_bsgs_batch_native
            assert seen == [4]
        else:
            res.append([eng.linear_transform(ct, diags, keys) for ct in cts])
    assert all(same(g, w) for g, w in zip(*res)), (cfg, patterns, level)


class Recording:
    """The library with lf_linear_transform_bsgs_batch replaced by a recorder of its marshalled arguments"""

    def __init__(self, real):
        self._real, self.args = real, None

    def __getattr__(self, name):
        return getattr(self._real, name)

    def lf_linear_transform_bsgs_batch(self, *args):
        self.args = args
        return 0


def test_the_entry_refuses_before_any_launch(lt_engine, monkeypatch):
    """nct 0 and 65, a NULL entry in c1, a workspace one word short and one 8 bytes off the alignment: LF_ERR_ARG, the outputs
    still holding their fill pattern.  The arguments are those the engine marshals for a group of 4; unchanged they give the loop."""
    from liberate_fhe_amd._native import lib
    from liberate_fhe_amd.fhe import backend as backend_module
    eng, keys = lt_engine
    level = 0
    n1, steps = SETS[0]
    cts = [synth.ciphertext(eng, 60 + i, level) for i in range(4)]
    diags = synth.diagonals_bsgs(eng, 8, level, steps, n1)
    want = [eng.linear_transform(ct, diags, keys) for ct in cts]
    rec = Recording(lib)
    monkeypatch.setattr(backend_module, "lib", rec)
    held = eng.linear_transform_batch(cts, diags, keys)                    # (the outputs the recorded pointers belong to)
    monkeypatch.undo()
    a = list(rec.args)
    assert a[1] == 4 and len(a) == 25
    plan, nb, ws_ptr, ws_words = a[0], a[4], a[20], a[21]
    assert ws_words == lib.lf_linear_transform_bsgs_batch_ws_words(plan, nb, 4) and ws_ptr % 16 == 0
    FILL = -0x0123456789ABCDEF

    def refused(**change):
        for h in held:
            for comp in h.data:
                comp[0].fill_(FILL)
        b = list(a)
        for k, v in change.items():
            b[int(k[1:])] = v
        code = lib.lf_linear_transform_bsgs_batch(*b)
        torch.cuda.synchronize()
        assert all(bool((comp[0] == FILL).all()) for h in held for comp in h.data), change
        return code

    c1_nul = (ctypes.c_void_p * 4)(*[a[3][i] for i in range(4)])
    c1_nul[2] = None
    # (a larger workspace for the offset pointer, so that only its alignment is wrong)
    big = torch.empty(ws_words + 2, dtype=torch.int64, device=held[0].data[0][0].device)
    assert big.data_ptr() % 16 == 0
    assert refused(_1=0) == LF_ERR_ARG
    assert refused(_1=65) == LF_ERR_ARG
    assert refused(_3=c1_nul) == LF_ERR_ARG
    assert refused(_21=ws_words - 1) == LF_ERR_ARG
    assert refused(_20=big.data_ptr() + 8) == LF_ERR_ARG
    assert lib.lf_linear_transform_bsgs_batch(*list(a[:20]) + [big.data_ptr()] + list(a[21:])) == 0
    torch.cuda.synchronize()
    assert all(same(h, w) for h, w in zip(held, want))
    assert lib.lf_linear_transform_bsgs_batch(*a) == 0                     # and with the recorded workspace itself
    torch.cuda.synchronize()
    assert all(same(h, w) for h, w in zip(held, want))


def test_band_matrix_times_three_vectors_with_real_keys():
    """logN 13 (4096 slots), real keys: a wrapping band matrix M of 16 diagonals (steps -8 .. 7) through matrix_diagonals, split
    with encdec.bsgs_split at n1 = 4 (3 + 3 keys), over three encrypted vectors (a group of 2 and a straggler).  The words are the
    loop's, so the decryption error against M @ m_i IS the loop's own; it is printed."""
    from liberate_fhe_amd.fhe import ckks_engine
    eng = ckks_engine(devices=["cuda:0"], **LT)
    sk = eng.create_secret_key()
    pk = eng.create_public_key(sk)
    n = eng.num_slots
    rng = np.random.default_rng(21)
    M = np.zeros((n, n), dtype=np.complex128)
    i = np.arange(n)
    for s in range(-8, 8):
        M[i, (i - s) % n] = rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)
    dg = encdec.matrix_diagonals(M)
    n1, babies, giants = encdec.bsgs_split(dg, n, 4)
    assert n1 == 4 and sorted(dg) == sorted(s % n for s in range(-8, 8))
    diags = eng.encode_diagonals(dg, 0, bsgs=n1)
    keys = {s: eng.create_rotation_key(sk, s) for s in sorted(set(babies + giants)) if s}
    assert len(keys) == 6
    np.random.seed(6)
    ms = [eng.example(-1, 1) for _ in range(3)]
    cts = [eng.encorypt(m, pk) for m in ms]
    seen = native_calls(eng)
    got = eng.linear_transform_batch(cts, diags, keys)
    assert seen == [2]
    want = [eng.linear_transform(ct, diags, keys) for ct in cts]
    assert all(same(g, w) for g, w in zip(got, want))
    for j, (g, w, m) in enumerate(zip(got, want, ms)):
        ref = M @ m
        err, err_loop = np.abs(eng.decrode(g, sk) - ref).max(), np.abs(eng.decrode(w, sk) - ref).max()
        print(f"logN 13 band matrix of 16 diagonals, n1 = 4, vector {j}: linear_transform_batch max abs error {err:.3e}, the loop's "
              f"{err_loop:.3e}, largest entry {np.abs(ref).max():.2f}")
        assert err == err_loop
