"""lt_matmul (a matrix of linear transforms times a vector of ciphertexts; lf_lt_matmul) without a GPU: the engine's host logic on
the checker backend against linear_transform (k_in = 1) and against the composition written out from the ntt ops, the refusals,
two logical devices, lt_matmul_steps, the C entry's argument checks, the new kernels' resources and the decryption error with real
keys against the loop of linear_transform + cc_add."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from liberate_fhe_amd.fhe import encdec
from liberate_fhe_amd.utils import synth
from tests.test_cc_dot_cpu import lazy_ciphertext, same
from tests.test_linear_transform_bsgs_cpu import _fake_plan, _real_engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LT = dict(logN=13, num_scales=5, num_special_primes=2, is_secured=False)
n = 1 << 12
# the step sets of the blocks: different sets inside one column, 7 keyed steps in one block, a wrapped one, step 0 alone
SETS = [(0, 1, 5), (1, 2, 3, 4, 6, 7, 9), (700,), (0,)]
ALL_STEPS = sorted({s for st in SETS for s in st if s})


def keys_for(eng, steps):
    return {s: synth.key_switch_key(eng, 40 + i, origin=f"rotation key:{s}") for i, s in enumerate(steps) if s}


@pytest.fixture(scope="module")
def checker():
    from liberate_fhe_amd.fhe import ckks_engine
    from tests.oracle_backend import OracleBackend
    eng = ckks_engine(devices=["cpu"], backend=OracleBackend(), **LT)
    assert eng.num_slots == n
    return eng, keys_for(eng, ALL_STEPS)


def layer_of(eng, k_in, k_out, level, seed=11):
    """(W, cts): blocks drawn from four diagonal objects (SETS) and three ciphertexts (two with lazy words), objects repeating on
    both sides; from k_in = 3 on: a hole in every second row, column 1 all None, and one plain {step: vector} entry."""
    D = [synth.diagonals(eng, seed + j, level, st) for j, st in enumerate(SETS)]
    pool = [lazy_ciphertext(eng, seed + 20 + level, level), synth.ciphertext(eng, seed + 21 + level, level),
            lazy_ciphertext(eng, seed + 22 + level, level)]
    cts = [pool[(2 * i) % 3] for i in range(k_in)]
    if k_in >= 3:
        cts[2] = cts[0]                                             # a repeated ciphertext object
    W = [[D[(o + 3 * i) % 4] for i in range(k_in)] for o in range(k_out)]
    if k_in >= 3:
        for o in range(k_out):
            W[o][1] = None                                          # a ciphertext no output uses
            if o % 2:
                W[o][0] = None                                      # a hole in every second row
        W[0][2] = W[0][0]                                           # a repeated diagonals object inside one row
        W[2][0] = {3: [0.5, -0.25], 0: [1.0, 2.0, -1.0]}            # a plain mapping, encoded by lt_matmul
    return W, cts


def composition(eng, W, cts, keys):
    """The definition of the op's words from the engine's public steps on one device, reading the encoded objects: per used
    input c0, c1 canonical; E = per part pre_extend(c1) -> extend -> exact forward NTT; c^ = P enter_ntt(c) on the ordinary
    rows; per step != 0 of the column t_c = sum over the parts of (E gathered by pi_step) x the key's part, t_0 += c^0 gathered
    on the ordinary rows (step 0: t = c^, zero on the special rows); S^o_c = sum_i sum_step pt_{o,i,step} * t^{i,step}_c;
    intt_exit_reduce, mod-down without addend, the engine's rescale."""
    d, N, logN, level = 0, eng.ctx.N, eng.ctx.logN, cts[0].level
    ell, K = eng._rows(d, level, False), eng.ntt.num_special_primes
    _2q, tabs, start = eng._vec("_2q", d, level, False), eng._ks_tables(level), eng.ntt.starts[level][d]

    def canonical(x):
        y = torch.empty_like(x)
        eng.backend.galois(x.contiguous(), y, ell, logN, 1, _2q)
        return y

    def rotated(ct, step):
        c = [canonical(ct.data[comp][0]) for comp in range(2)]
        chat = []
        for comp in range(2):
            x = c[comp].clone()
            eng.ntt.enter_ntt([x], level, d, -1)
            eng.ntt.mont_enter_scalar([x], [eng._PR(d, level)], level, d, -1)
            chat.append(x)
        if step == 0:
            return [torch.cat([chat[comp], torch.zeros((K, N), dtype=torch.int64)]) for comp in range(2)]
        idx = torch.from_numpy(encdec.ntt_galois_index(logN, encdec.galois_exponent(N, step)))
        t = None
        for part_id in range(len(eng.ntt.p.p[level][d])):
            ext = eng.extend(eng.pre_extend([c[1]], d, level, part_id), d, level, part_id, d)
            eng.ntt.ntt([ext], level, d, -2)
            g = ext[:, idx].contiguous()
            part = keys[step].data[eng.parts_alloc[level][d][part_id]].data
            prod = [eng.ntt.mont_mult([g], [part[comp][0][start:]], level, d, -2)[0] for comp in range(2)]
            t = prod if t is None else [eng.ntt.mont_add([t[comp]], [prod[comp]], level, d, -2)[0] for comp in range(2)]
        folded = eng.ntt.mont_add([t[0][:ell].contiguous()], [chat[0][:, idx].contiguous()], level, d, -1)[0]
        t[0] = torch.cat([folded, t[0][ell:]])
        return t

    cache, outs = {}, []
    for row in W:
        S = [None, None]
        for i, blk in enumerate(row):
            if blk is None:
                continue
            for j, step in enumerate(eng.diagonal_steps(blk)):
                key = (id(cts[i]), step)
                if key not in cache:
                    cache[key] = rotated(cts[i], step)
                for comp in range(2):
                    prod = eng.ntt.mont_mult([blk.data[j][0]], [cache[key][comp]], level, d, -2)[0]
                    S[comp] = prod if S[comp] is None else eng.ntt.mont_add([S[comp]], [prod], level, d, -2)[0]
        s = torch.stack(S).contiguous()
        eng.ntt.intt_exit_reduce([s[0]], level, d, -2)
        eng.ntt.intt_exit_reduce([s[1]], level, d, -2)
        out = torch.empty((2, ell, N), dtype=torch.int64)
        eng.backend.ks_moddown_batch([s[0], s[1]], [out[0], out[1]], [None, None], ell, K, tabs[("pir", d)],
                                     eng._vec("Rs", d, level, True), eng._consts(d, level, True), PiP=None, galois=None)
        outs.append(eng.rescale(eng._new(([out[0]], [out[1]]), cts[0].origin, level=level)))
    return outs


def encoded_matrix(eng, W, cts, keys, monkeypatch):
    """lt_matmul(W, ..) and W with every plain mapping replaced by the object lt_matmul encoded for it (encode draws its rounding
    at random: the composition has to read the very words the op multiplied by)."""
    made = []
    real = eng.encode_diagonals
    monkeypatch.setattr(eng, "encode_diagonals", lambda *a, **k: (made.append(real(*a, **k)), made[-1])[1])
    got = eng.lt_matmul(W, cts, keys)
    monkeypatch.undo()
    by_id = {}
    for row in W:
        for b in row:
            if isinstance(b, dict) and id(b) not in by_id:
                by_id[id(b)] = made[len(by_id)]                     # (encoded in row-major order, each mapping once)
    assert len(by_id) == len(made)
    We = [[by_id[id(b)] if isinstance(b, dict) else b for b in row] for row in W]
    return got, We


@pytest.mark.parametrize("level", [0, 3])
@pytest.mark.parametrize("k_out", [1, 3])
def test_one_input_gives_the_words_of_linear_transform(checker, level, k_out):
    """k_in = 1, shapes 1 x 1 and 1 x 3, level 0 and the last legal one: output o is linear_transform(ct, W[o][0], keys) word for
    word."""
    from liberate_fhe_amd.fhe.presets import types
    eng, keys = checker
    assert eng.num_levels - 2 == 3
    ct = lazy_ciphertext(eng, 70 + level, level)
    W = [[synth.diagonals(eng, 5 + o, level, SETS[o])] for o in range(k_out)]
    got = eng.lt_matmul(W, [ct], keys)
    assert isinstance(got, list) and len(got) == k_out
    for o, g in enumerate(got):
        assert g.level == level + 1 and g.origin == types.origins["ct"] and not g.ntt_state and not g.include_special
        assert same(g, eng.linear_transform(ct, W[o][0], keys)), (level, o)


@pytest.mark.parametrize("level", [0, 3])
@pytest.mark.parametrize("shape", [(2, 2), (3, 5)])
def test_lt_matmul_equals_the_composition(checker, level, shape, monkeypatch):
    """(k_in, k_out) = (2, 2) and (3, 5) against the composition written out from the ntt ops, word for word; (3, 5) has
    different step sets inside one column, a hole in every second row, a column all None, a repeated ciphertext, a repeated
    diagonals object and a plain mapping."""
    eng, keys = checker
    W, cts = layer_of(eng, *shape, level)
    if shape == (3, 5):
        assert all(row[1] is None for row in W) and W[1][0] is None and cts[2] is cts[0] and W[0][2] is W[0][0] and isinstance(W[2][0], dict)
        assert len({tuple(eng.diagonal_steps(row[2])) for row in W}) == 4            # four step sets in column 2
    got, We = encoded_matrix(eng, W, cts, keys, monkeypatch)
    want = composition(eng, We, cts, keys)
    assert len(got) == len(want) == shape[1]
    for o, (g, w) in enumerate(zip(got, want)):
        assert g.level == level + 1 and same(g, w), (shape, level, o)
    # any iterables, a list of keys in any order
    Ws = [[b for b in row] for row in We]
    again = eng.lt_matmul(iter([iter(row) for row in Ws]), (c for c in cts), [keys[s] for s in reversed(sorted(keys))])
    assert all(same(a, b) for a, b in zip(again, got))


def test_several_inputs_round_once_not_once_per_block(checker):
    """For k_in > 1 the words are the op's own: cc_add over separate transforms rounds once per block and differs."""
    eng, keys = checker
    W, cts = layer_of(eng, 2, 2, 0)
    got = eng.lt_matmul(W, cts, keys)
    loop = eng.cc_add(eng.linear_transform(cts[0], W[0][0], keys), eng.linear_transform(cts[1], W[0][1], keys))
    assert got[0].level == loop.level and not same(got[0], loop)


def test_lt_matmul_steps(checker):
    eng, keys = checker
    W, _ = layer_of(eng, 3, 5, 0)
    assert eng.lt_matmul_steps(W) == sorted(set(ALL_STEPS) | {3}) == [1, 2, 3, 4, 5, 6, 7, 9, 700]
    assert eng.lt_matmul_steps([[{0: [1.0]}, None]]) == []
    assert eng.lt_matmul_steps(iter([iter([{-1: [1.0], n + 2: [1.0]}])])) == [2, n - 1]


def test_refusals_come_before_anything_is_computed(checker, monkeypatch):
    """Every refusal is raised with nothing computed, encoded or allocated: the backend, linear_transform, encode_diagonals, the
    ntt ops and every allocation are patched to record, and none is reached.  The engine works afterwards."""
    from liberate_fhe_amd.fhe.presets import errors
    eng, keys = checker
    top = eng.num_levels - 1
    c0, c1, ctop = (synth.ciphertext(eng, 60 + i, lvl) for i, lvl in enumerate((0, 1, top)))
    d0, d1 = synth.diagonals(eng, 3, 0, (0, 1, 5)), synth.diagonals(eng, 3, 1, (0, 1))
    dtop = synth.diagonals(eng, 3, top, (0,))
    bsgs = synth.diagonals_bsgs(eng, 3, 0, (0, 1, 5), 4)
    ntt = eng._new(c0.data, c0.origin, level=0, ntt_state=True)
    special = eng._new(c0.data, c0.origin, level=0, include_special=True)
    cap_keys, cap_in = eng.lt_matmul_max_column_keys, eng.lt_matmul_max_inputs
    assert (cap_keys, cap_in) == (63, 64)
    wide = {s: [1.0] for s in range(1, cap_keys + 2)}                      # 64 keyed steps in one block
    split = [[{s: [1.0] for s in range(1, 40)}], [{s: [1.0] for s in range(30, 70)}]]   # .. and in one column over two blocks
    many_keys = {s: k._replace(origin=f"rotation key:{s}") for s, k in zip(range(1, 80), [keys[1]] * 80)}
    calls = []

    def boom(name):
        def f(*a, **k):
            calls.append(name)
            raise AssertionError(name + " reached")
        return f

    for name in ("linear_transform", "encode_diagonals", "_lt_matmul_encode", "_lt_matmul_native_args", "_lt_matmul_native",
                 "_lt_matmul_steps", "rescale", "clone", "_ws", "_op_plan", "_ks_tables", "_ks_digits_exchanged", "_diag_pack", "_key_pack",
                 "_lt_chat", "_lt_forward", "_lt_inner", "_lt_giant", "_lt_tail"):
        monkeypatch.setattr(eng, name, boom(name))
    for name in ("lt_matmul_native", "lt_matmul_ws_words", "galois", "ntt", "intt", "ks_fwd", "ks_tail", "ks_inner", "ks_moddown_ws"):
        monkeypatch.setattr(eng.backend, name, boom(name), raising=False)
    for name in ("enter_ntt", "mont_mult", "mont_add", "mont_enter", "intt_exit_reduce"):
        monkeypatch.setattr(eng.ntt, name, boom(name))
    real_empty, real_zeros = torch.empty, torch.zeros
    monkeypatch.setattr(torch, "empty", lambda *a, **k: (calls.append("empty"), real_empty(*a, **k))[1])
    monkeypatch.setattr(torch, "zeros", lambda *a, **k: (calls.append("zeros"), real_zeros(*a, **k))[1])
    cases = [
        (ValueError, [], [c0], keys),                                              # W empty
        (ValueError, [[d0]], [], keys),                                            # cts empty
        (ValueError, [[]], [], keys),
        (ValueError, [[d0, d0], [d0]], [c0, c0], keys),                            # ragged
        (ValueError, [[d0], [d0]], [c0, c0], keys),                                # len(W[o]) != len(cts)
        (ValueError, [[d0, d0, d0]], [c0, c0], keys),
        (ValueError, [[d0, None], [None, None]], [c0, c0], keys),                  # a row with no block
        (ValueError, [[wide]], [c0], many_keys),                                   # more keyed steps in a column than the cap
        (ValueError, split, [c0], many_keys),
        (ValueError, [[d0] * (cap_in + 1)], [c0] * (cap_in + 1), keys),            # k_in above its cap
        (ValueError, [[{}]], [c0], keys),                                          # a mapping without a diagonal
        (ValueError, [[{1: [1.0], 1 + n: [2.0]}]], [c0], keys),                    # the same step twice mod num_slots
        (errors.NotMatchType, [[c0]], [c0], keys),                                 # a ciphertext where diagonals belong
        (errors.NotMatchType, [[d0]], [d0], keys),                                 # .. and the other way round
        (errors.NotMatchType, [[d0, None]], [c0, None], keys),                     # (a None ciphertext, even in an unused column)
        (errors.NotMatchType, [[3.5]], [c0], keys),
        (errors.NotMatchType, [[d0]], [c0], [keys[1], keys[5], synth.key_switch_key(eng, 8)]),   # a key of another kind
        (errors.NotMatchType, [[d0]], [c0], [keys[1]]),                            # a missing key (step 5)
        (errors.NotMatchType, [[{0: [1.0], 11: [1.0]}]], [c0], keys),              # .. for a plain mapping (step 11)
        (errors.NotMatchDataStructState, [[d1]], [c0], keys),                      # a block of another level
        (errors.NotMatchDataStructState, [[d0, None], [d0, d1]], [c0, c0], keys),
        (errors.NotMatchDataStructState, [[d0, d0]], [c0, c1], keys),              # ciphertexts of different levels
        (errors.NotMatchDataStructState, [[d0, None]], [c0, c1], keys),            # (an unused column is still of the level)
        (errors.MaximumLevelError, [[dtop]], [ctop], keys),
        (errors.MaximumLevelError, [[{0: [1.0]}]], [ctop], keys),
        (NotImplementedError, [[d0]], [ntt], keys),                                # an NTT-domain ciphertext
        (NotImplementedError, [[d0, None]], [c0, special], keys),                  # special limbs
        (NotImplementedError, [[bsgs]], [c0], keys),                               # giant steps inside a block
        (NotImplementedError, [[d0, bsgs]], [c0, c0], keys),
    ]
    for exc, W, cts, ks in cases:
        with pytest.raises(exc):
            eng.lt_matmul(W, cts, ks)
    with pytest.raises(errors.NotMatchType, match="step 5"):                      # the missing step is named
        eng.lt_matmul([[d0]], [c0], [keys[1]])
    with pytest.raises(NotImplementedError):
        eng.lt_matmul_steps([[bsgs]])
    with pytest.raises(ValueError):
        eng.lt_matmul_steps([[d0], [d0, d0]])
    assert calls == []
    monkeypatch.undo()
    # exactly the cap is legal as far as the checks go (the missing key is the first complaint), and the engine still works
    with pytest.raises(errors.NotMatchType):
        eng.lt_matmul([[{s: [1.0] for s in range(0, cap_keys + 1)}]], [c0], keys)
    out = eng.lt_matmul([[d0, None], [None, {0: [1.0, 0.5]}]], [c0, c0], keys)
    assert [o.level for o in out] == [1, 1]
    assert same(out[0], eng.linear_transform(c0, d0, keys))
    # an input that no output uses is legal: its ciphertext is not read
    poisoned = c0._replace(data=([None], [None]))
    assert same(eng.lt_matmul([[d0, None]], [c0, poisoned], keys)[0], out[0])


def test_two_logical_devices_give_the_single_device_words():
    """Two shards take the orchestrated steps with a digit exchange per input; row by row in prime order the words of one device."""
    from liberate_fhe_amd.fhe import ckks_engine
    from tests.oracle_backend import OracleBackend
    from tests.test_pc_dot_gpu import natural_rows
    res = []
    for ndev in (1, 2):
        eng = ckks_engine(devices=["cpu"] * ndev, backend=OracleBackend(), **LT)
        assert ndev == 1 or eng._native_level(0) is None
        keys = keys_for(eng, ALL_STEPS)
        D = [synth.diagonals(eng, 4 + j, 0, st) for j, st in enumerate(SETS)]
        cts = [synth.ciphertext(eng, 8 + i, 0) for i in range(3)]
        W = [[D[0], None, D[1]], [D[2], None, D[0]], [None, None, D[3]]]
        out = eng.lt_matmul(W, cts, keys)
        assert len(out) == 3 and all(o.level == 1 for o in out)
        res.append([natural_rows(eng, o) for o in out])
    for a, b in zip(*res):
        for x, y in zip(a, b):
            assert x.shape == y.shape and (x == y).all()


def test_c_entry_refuses_bad_arguments_before_any_launch():
    """lf_lt_matmul returns LF_ERR_ARG from its arguments alone (dummy pointers that are never dereferenced; no call here would
    pass the checks), lf_lt_matmul_ws_words gives (nb_max + 1 + k_out) pairs + the mod-down's buffers and workspace for
    g = min(k_out, 4) outputs and 0 for what the entry refuses, and the caps are the header's everywhere."""
    from liberate_fhe_amd import _native
    from liberate_fhe_amd._native import lib, EXPORTED
    from liberate_fhe_amd.fhe.backend import HipBackend
    LF_ERR_ARG = 10001
    assert "lf_lt_matmul" in EXPORTED and "lf_lt_matmul_ws_words" in EXPORTED and lib.lf_abi_version() == 15
    header = open(os.path.join(ROOT, "include", "ckks_hip.h")).read()
    IMAX = int(re.search(r"#define LF_LT_MATMUL_MAX_INPUTS (\d+)", header).group(1))
    OMAX = int(re.search(r"#define LF_LT_MATMUL_MAX_OUTPUTS (\d+)", header).group(1))
    KMAX = int(re.search(r"#define LF_BSGS_MAX_BABY_KEYS (\d+)", header).group(1))
    assert (IMAX, OMAX) == (_native.LF_LT_MATMUL_MAX_INPUTS, _native.LF_LT_MATMUL_MAX_OUTPUTS) == \
        (HipBackend.lt_matmul_max_inputs, HipBackend.lt_matmul_max_outputs) == (64, 64)
    assert KMAX == HipBackend.bsgs_max_baby_keys == 63
    for logN in (13, 15, 17):
        plan = _fake_plan(logN)
        N, rows, ell, K = 1 << logN, 3, 2, 1
        for nb in (0, 1, 7, KMAX):
            for k_out in (1, 2, 3, 4, 5, 9, OMAX):
                g = min(k_out, 4)
                want = 2 * rows * N * (nb + 1 + k_out) + 2 * g * ell * N + lib.lf_ks_moddown_ws_words(2 * g, ell, K, N)
                assert lib.lf_lt_matmul_ws_words(ctypes.byref(plan), nb, k_out) == want, (logN, nb, k_out)
    plan = _fake_plan(13)
    for nb, k_out in ((-1, 1), (KMAX + 1, 1), (0, 0), (0, -1), (0, OMAX + 1)):
        assert lib.lf_lt_matmul_ws_words(ctypes.byref(plan), nb, k_out) == 0, (nb, k_out)
    for logN in (12, 18):
        assert lib.lf_lt_matmul_ws_words(ctypes.byref(_fake_plan(logN)), 1, 1) == 0
    assert lib.lf_lt_matmul_ws_words(None, 1, 1) == 0

    dummy = ctypes.c_void_p(64)
    stride = 3 << 13

    def i64(values):
        return (ctypes.c_int64 * max(1, len(values)))(*values)

    def ptrs(count, null_at=()):
        arr = (ctypes.c_void_p * max(count, 1))(*([64] * max(count, 1)))
        for at in null_at:
            arr[at] = None
        return arr

    # 2 inputs x 2 outputs: column 0 has keyed steps (exponents 3, 5), column 1 none; blocks (0,0): slots 0,1,2; (0,1): NULL;
    # (1,0): slot 2; (1,1): slot 0
    def call(plan=plan, k_in=2, k_out=2, scales=dummy, ws=dummy, ws_words=1 << 40, fmt=0, part_stride=0, **over):
        a = {"ins": ptrs(2 * max(k_in, 1)), "keys": ptrs(4), "pts": ptrs(4, [1]), "out0": ptrs(max(k_out, 1)), "out1": ptrs(max(k_out, 1)),
             "ncol": i64((2, 0)), "exps": i64((3, 5)), "strides": i64((stride, 0, stride, stride)), "counts": i64((3, 0, 1, 1)),
             "bidx": i64((0, 1, 2, 2, 0))}
        for name, value in over.items():
            assert name in a
            a[name] = value if value is None or isinstance(value, ctypes.Array) else i64(value)
        return lib.lf_lt_matmul(ctypes.byref(plan) if plan is not None else None, k_in, k_out, a["ins"], a["ncol"], a["exps"], a["keys"],
                                part_stride, 0, 0, fmt, a["pts"], a["strides"], a["counts"], a["bidx"], scales, 0, ws, ws_words,
                                a["out0"], a["out1"], None)

    N2 = 2 << 13
    need = lib.lf_lt_matmul_ws_words(ctypes.byref(plan), 2, 2)
    assert call(plan=None) == LF_ERR_ARG
    for logN in (12, 18):
        assert call(plan=_fake_plan(logN)) == LF_ERR_ARG, logN
    one = _fake_plan(13)
    one.ell = 1                                                                # no level left to rescale into
    assert call(plan=one) == LF_ERR_ARG
    nopr = _fake_plan(13)
    nopr.PR = None
    assert call(plan=nopr) == LF_ERR_ARG
    for k_in in (0, -1, IMAX + 1):
        assert call(k_in=k_in) == LF_ERR_ARG, k_in
    for k_out in (0, -1, OMAX + 1):
        assert call(k_out=k_out) == LF_ERR_ARG, k_out
    for name in ("ins", "ncol", "exps", "keys", "pts", "strides", "counts", "bidx", "out0", "out1"):
        assert call(**{name: None}) == LF_ERR_ARG, name
    assert call(scales=None) == LF_ERR_ARG
    assert call(fmt=2) == LF_ERR_ARG and call(fmt=-1) == LF_ERR_ARG
    assert call(ncol=(-1, 0)) == LF_ERR_ARG and call(ncol=(KMAX + 1, 0)) == LF_ERR_ARG        # a count out of range
    for at in (0, 1, 2, 3):                                                    # a NULL among the used pointers
        assert call(ins=ptrs(4, [at])) == LF_ERR_ARG, at
    for at in (0, 1):
        assert call(keys=ptrs(4, [at])) == LF_ERR_ARG
        assert call(out0=ptrs(2, [at])) == LF_ERR_ARG and call(out1=ptrs(2, [at])) == LF_ERR_ARG
    for bad in ((4, 5), (3, N2 + 1), (-3, 5), (3, 0)):                         # even, >= 2N, negative, zero exponents
        assert call(exps=bad) == LF_ERR_ARG, bad
    assert call(pts=ptrs(4, [0, 1])) == LF_ERR_ARG                             # an output with no block
    assert call(pts=ptrs(4, [1, 2, 3])) == LF_ERR_ARG
    assert call(counts=(3, 1, 1, 1)) == LF_ERR_ARG                             # a NULL block that claims diagonals
    assert call(counts=(0, 0, 1, 1), bidx=(2, 0)) == LF_ERR_ARG                # a block without diagonals
    assert call(counts=(4, 0, 1, 1), bidx=(0, 1, 2, 2, 2, 0)) == LF_ERR_ARG    # more diagonals than the column has slots
    assert call(strides=(stride - 1, 0, stride, stride)) == LF_ERR_ARG
    assert call(bidx=(0, 1, 3, 2, 0)) == LF_ERR_ARG                            # a slot outside its column's set
    assert call(bidx=(0, 1, 2, 2, 1)) == LF_ERR_ARG                            # (column 1 has slot 0 only)
    assert call(bidx=(-1, 1, 2, 2, 0)) == LF_ERR_ARG
    assert call(bidx=(1, 0, 2, 2, 0)) == LF_ERR_ARG                            # slots not ascending
    assert call(bidx=(0, 1, 1, 2, 0)) == LF_ERR_ARG
    assert call(fmt=1, keys=(ctypes.c_void_p * 4)(72, 64, 64, 64)) == LF_ERR_ARG      # a planes key not 16-byte aligned
    assert call(fmt=1, part_stride=1) == LF_ERR_ARG
    assert call(ws=None) == LF_ERR_ARG
    assert call(ws=ctypes.c_void_p(72)) == LF_ERR_ARG                          # misaligned
    assert call(ws_words=need - 1) == LF_ERR_ARG and call(ws_words=0) == LF_ERR_ARG
    # the pointers of an input no block uses are not among the checked ones: with column 1 unused its NULLs are not what is
    # refused (the call is still refused, by its workspace, so nothing is launched)
    unused = dict(pts=ptrs(4, [1, 3]), counts=(3, 0, 1, 0), bidx=(0, 1, 2, 2), ins=ptrs(4, [2, 3]))
    assert call(ws_words=need - 1, **unused) == LF_ERR_ARG


def test_block_products_kernels_use_no_scratch():
    """lt_block_products_kernel<1 | 2 | 4> exist in ckks_ks.hip under these names with scratch 0, no spill and at least 4 waves per
    SIMD (streaming kernels, as lt_diag_products_kernel); the tracked table lists them as built."""
    import __graft_entry__ as g
    res = {r["kernel"]: r for r in g.kernel_resources()}
    want = [f"lt_block_products_kernel<{no}>" for no in (1, 2, 4)]
    assert sorted(k for k in res if k.startswith("lt_block_products_kernel")) == sorted(want)
    tracked = open(os.path.join(ROOT, "profiles", "r06_kernel_resources.txt")).read()
    for k in want:
        r = res[k]
        assert r["file"] == "ckks_ks.hip" and r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, r
        assert r["occupancy"] >= 4, r
        line = next(ln for ln in tracked.splitlines() if ln[18:76].strip() == k)
        f = line.split()
        assert (int(f[-7]), int(f[-3]), int(f[-1])) == (r["vgprs"], r["scratch"], r["occupancy"]), line


def block_diagonals(A, slots):
    """matrix_diagonals of the slots x slots block-diagonal matrix kron(I, A), built without the matrix: with i = m b + r the entry
    M[i][i - step] lies in block b iff 0 <= r - step < m, and is A[r][r - step] there."""
    A = np.asarray(A)
    m = A.shape[0]
    r = np.arange(slots) % m
    out = {}
    for step in range(-(m - 1), m):
        c = r - step
        ok = (c >= 0) & (c < m)
        out[step % slots] = np.where(ok, A[r, np.clip(c, 0, m - 1)], 0.0)
    return out


def matmul_errors(eng, sk, cts, ms, rng):
    """(max error of lt_matmul, max error of the loop of linear_transform + cc_add, keys) for a 2 x 2 matrix of random
    block-diagonal matrices on the same ciphertexts, encoded diagonals and keys, against the numpy product."""
    A = [[rng.uniform(-1, 1, (4, 4)) for _ in range(2)] for _ in range(2)]
    W = [[eng.encode_diagonals(block_diagonals(A[o][i], eng.num_slots), cts[0].level) for i in range(2)] for o in range(2)]
    keys = [eng.create_rotation_key(sk, s) for s in eng.lt_matmul_steps(W)]
    want = [sum((A[o][i] @ ms[i].reshape(-1, 4).T).T.reshape(-1) for i in range(2)) for o in range(2)]
    got = eng.lt_matmul(W, cts, keys)
    loop = [eng.cc_add(eng.linear_transform(cts[0], W[o][0], keys), eng.linear_transform(cts[1], W[o][1], keys)) for o in range(2)]
    e_mat = max(np.abs(eng.decrode(g, sk) - w).max() for g, w in zip(got, want))
    e_loop = max(np.abs(eng.decrode(g, sk) - w).max() for g, w in zip(loop, want))
    return e_mat, e_loop, len(keys)


def test_decryption_error_with_real_keys_stays_within_twice_the_loop():
    """Real keys on the checker engine, 2 x 2 blocks from matrix_diagonals of random block-diagonal matrices (4 x 4 blocks: 7
    diagonals, steps -3 .. 3), fresh ciphertexts at level 0: decrode against the numpy product, at most 2 x the maximum error of
    the loop of linear_transform + cc_add on the same ciphertexts, diagonals and keys (the project's margin for a maximum over
    2^12 slots between two roundings of the same quantity).  Measured here: lt_matmul 2.472e-10, loop 2.472e-10 (printed): the noise of the inputs dominates both."""
    eng, sk, pk = _real_engine()
    rng = np.random.default_rng(9)
    A = rng.uniform(-1, 1, (4, 4))                                         # the diagonals ARE matrix_diagonals of the block matrix
    dense, direct = encdec.matrix_diagonals(np.kron(np.eye(n // 4), A)), block_diagonals(A, n)
    assert sorted(dense) == sorted(direct) == [0, 1, 2, 3, n - 3, n - 2, n - 1] and all((dense[s] == direct[s]).all() for s in dense)
    ms = [rng.uniform(-4, 4, n) + 1j * rng.uniform(-4, 4, n) for _ in range(2)]
    cts = [eng.encorypt(m, pk) for m in ms]
    e_mat, e_loop, nkeys = matmul_errors(eng, sk, cts, ms, rng)
    print(f"logN 13, 2 x 2 blocks of 7 diagonals, {nkeys} keys, level 0: max error lt_matmul {e_mat:.3e}, loop of linear_transform + cc_add {e_loop:.3e}")
    assert nkeys == 6
    assert e_mat <= 2 * e_loop and e_loop < 1e-6
