"""lt_matmul_bsgs (a matrix of baby-step / giant-step linear transforms times a vector of ciphertexts; lf_lt_matmul_bsgs) without a
GPU: the engine's host logic on the checker backend against the composition written out from the ntt ops, the three consequences
of the definition (one input: linear_transform's BSGS form; giant step 0 alone: lt_matmul on flat-tagged packs; output o depends
on row o only), plain mappings, lt_matmul_bsgs_steps, the refusals, two logical devices, the C entry's argument checks, the new
kernel's resources and the decryption error with real keys against the loop of BSGS linear_transform + cc_add."""
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
from tests.test_lt_matmul_cpu import block_diagonals

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LT = dict(logN=13, num_scales=5, num_special_primes=2, is_secured=False)
n = 1 << 12
N1 = 4
KEY_STEPS = (1, 2, 3, 4, 8, 12)                    # baby keys 1, 2, 3; giant keys 4, 8, 12
# The reference layout, 3 inputs x 6 outputs (the tail runs in groups of 4 + 2), [output][input] -> steps, n1 = 4:
#   giant step 4 in outputs 0 - 4 (giant groups of 4 + 1), giant step 8 in outputs 0 and 2 (a group of 2), giant step 12 in output 4
#   only (the single kernel); output 1 has no giant-step-0 diagonal (its accumulator is zeroed), output 5 giant step 0 only (no
#   giant phase); column 1 uses step 0 only (no key, no digits); S^{0,4}, S^{0,8}, S^{2,4}, S^{4,4} are fed by two inputs,
#   S^{1,4}, S^{3,4}, S^{2,8}, S^{4,12} by a single one; block (1, 0) has holes in its baby steps (b = 0, 1, 3), block (0, 2) in
#   every giant step.
LAYOUT = [
    [(0, 1, 2, 3, 4, 5, 6, 7, 8, 9), (0,), (1, 2, 5, 8, 11)],
    [(4, 5, 7), None, None],
    [(1, 5, 9), (0,), (3, 4)],
    [None, None, (0, 2, 4, 7)],
    [(0, 2, 3, 4, 6, 7, 12, 13, 15), (0,), (6, 7)],
    [(1, 2, 3), (0,), None],
]


def giants_of(row, n1=N1):
    return sorted({s - s % n1 for st in row if st is not None for s in st})


def test_the_layout_is_the_one_the_issue_asks_for():
    assert [giants_of(r) for r in LAYOUT] == [[0, 4, 8], [4], [0, 4, 8], [0, 4], [0, 4, 12], [0]]
    assert all(r[1] in (None, (0,)) for r in LAYOUT)
    fed = {(o, g): sum(any(s - s % N1 == g for s in st) for st in r if st is not None) for o, r in enumerate(LAYOUT) for g in giants_of(r)}
    assert fed[(0, 4)] == 2 and fed[(3, 4)] == 1 and fed[(4, 12)] == 1 and fed[(2, 8)] == 1 and fed[(0, 8)] == 2
    assert sorted({s % N1 for s in LAYOUT[1][0]}) == [0, 1, 3]


def keys_for(eng, steps=KEY_STEPS):
    return {s: synth.key_switch_key(eng, 40 + i, origin=f"rotation key:{s}") for i, s in enumerate(steps) if s}


def layer(eng, level, seed=7, layout=LAYOUT, n1=N1, lazy=False):
    """(W, cts) of the layout: one diagonals_bsgs object per block (its own seed), one ciphertext per column"""
    W = [[None if st is None else synth.diagonals_bsgs(eng, seed + 8 * o + i, level, st, n1) for i, st in enumerate(row)]
         for o, row in enumerate(layout)]
    make = lazy_ciphertext if lazy else synth.ciphertext
    cts = [make(eng, 90 + 3 * level + i, level) for i in range(len(layout[0]))]
    return W, cts


@pytest.fixture(scope="module")
def checker():
    from liberate_fhe_amd.fhe import ckks_engine
    from tests.oracle_backend import OracleBackend
    eng = ckks_engine(devices=["cpu"], backend=OracleBackend(), **LT)
    assert eng.num_slots == n
    return eng, keys_for(eng)


def composition(eng, W, cts, keys, n1):
    """The definition of the op's words from the engine's public steps on one device, reading the encoded objects: per used
    input c0, c1 canonical, E = per part pre_extend(c1) -> extend -> exact forward NTT, c^ = P enter_ntt(c) on the ordinary rows;
    per keyed baby step u^{i,b}_c = sum over the parts of (E gathered by pi_b) x key b's part, u_0 += c^0 gathered on the ordinary
    rows (b = 0: u = c^, zero on the special rows); per output and giant step S^{o,g}_c = sum_i sum_b pt_{o,i,g+b} * u^{i,b}_c, over
    the inputs before anything comes down; g != 0: w = mod-down of intt_exit_reduce(S_1), canonical, E^{o,g} its digits, v_c = sum
    over the parts of (E^{o,g} gathered by pi_g) x key g's part, v_0 += S_0 gathered on all rows; A^o = S^{o,0} + sum v;
    intt_exit_reduce, mod-down without addend, the engine's rescale."""
    d, N, logN, level = 0, eng.ctx.N, eng.ctx.logN, cts[0].level
    ell, K = eng._rows(d, level, False), eng.ntt.num_special_primes
    _2q, tabs, start = eng._vec("_2q", d, level, False), eng._ks_tables(level), eng.ntt.starts[level][d]

    def canonical(x):
        y = torch.empty_like(x)
        eng.backend.galois(x.contiguous(), y, ell, logN, 1, _2q)
        return y

    def digits(c1):
        E = []
        for part_id in range(len(eng.ntt.p.p[level][d])):
            ext = eng.extend(eng.pre_extend([c1], d, level, part_id), d, level, part_id, d)
            eng.ntt.ntt([ext], level, d, -2)
            E.append(ext)
        return E

    def inner(E, idx, key):
        t = None
        for part_id, ext in enumerate(E):
            g = ext[:, idx].contiguous()
            part = key.data[eng.parts_alloc[level][d][part_id]].data
            prod = [eng.ntt.mont_mult([g], [part[c][0][start:]], level, d, -2)[0] for c in range(2)]
            t = prod if t is None else [eng.ntt.mont_add([t[c]], [prod[c]], level, d, -2)[0] for c in range(2)]
        return t

    def index(step):
        return torch.from_numpy(encdec.ntt_galois_index(logN, encdec.galois_exponent(N, step)))

    prepared, u = {}, {}

    def baby(ct, b):
        if (id(ct), b) in u:
            return u[(id(ct), b)]
        if id(ct) not in prepared:
            c = [canonical(ct.data[comp][0]) for comp in range(2)]
            chat = []
            for comp in range(2):
                x = c[comp].clone()
                eng.ntt.enter_ntt([x], level, d, -1)
                eng.ntt.mont_enter_scalar([x], [eng._PR(d, level)], level, d, -1)
                chat.append(x)
            prepared[id(ct)] = (c, chat, {})
        c, chat, lazy = prepared[id(ct)]
        if b == 0:
            t = [torch.cat([chat[comp], torch.zeros((K, N), dtype=torch.int64)]) for comp in range(2)]
        else:
            if "E" not in lazy:
                lazy["E"] = digits(c[1])
            idx = index(b)
            t = inner(lazy["E"], idx, keys[b])
            folded = eng.ntt.mont_add([t[0][:ell].contiguous()], [chat[0][:, idx].contiguous()], level, d, -1)[0]
            t[0] = torch.cat([folded, t[0][ell:]])
        u[(id(ct), b)] = t
        return t

    outs = []
    for row in W:
        A = [None, None]
        for g in sorted({s - s % n1 for blk in row if blk is not None for s in eng.diagonal_steps(blk)}):
            S = [None, None]
            for i, blk in enumerate(row):
                if blk is None:
                    continue
                for j, s in enumerate(eng.diagonal_steps(blk)):
                    if s - s % n1 != g:
                        continue
                    t = baby(cts[i], s % n1)
                    for comp in range(2):
                        prod = eng.ntt.mont_mult([blk.data[j][0]], [t[comp]], level, d, -2)[0]
                        S[comp] = prod if S[comp] is None else eng.ntt.mont_add([S[comp]], [prod], level, d, -2)[0]
            if g:
                s1 = S[1].clone()
                eng.ntt.intt_exit_reduce([s1], level, d, -2)
                w = torch.empty((ell, N), dtype=torch.int64)
                eng.backend.ks_moddown_batch([s1], [w], [None], ell, K, tabs[("pir", d)], eng._vec("Rs", d, level, True),
                                             eng._consts(d, level, True), PiP=None, galois=None)
                idx = index(g)
                v = inner(digits(canonical(w)), idx, keys[g])
                v[0] = eng.ntt.mont_add([v[0]], [S[0][:, idx].contiguous()], level, d, -2)[0]
                S = v
            for comp in range(2):
                A[comp] = S[comp] if A[comp] is None else eng.ntt.mont_add([A[comp]], [S[comp]], level, d, -2)[0]
        s = torch.stack(A).contiguous()
        eng.ntt.intt_exit_reduce([s[0]], level, d, -2)
        eng.ntt.intt_exit_reduce([s[1]], level, d, -2)
        out = torch.empty((2, ell, N), dtype=torch.int64)
        eng.backend.ks_moddown_batch([s[0], s[1]], [out[0], out[1]], [None, None], ell, K, tabs[("pir", d)],
                                     eng._vec("Rs", d, level, True), eng._consts(d, level, True), PiP=None, galois=None)
        outs.append(eng.rescale(eng._new(([out[0]], [out[1]]), cts[0].origin, level=level)))
    return outs


@pytest.fixture(scope="module")
def reference(checker):
    """per level the layout's (W, cts, lt_matmul_bsgs(W, cts, keys)), computed once and only read by the tests that share it"""
    eng, keys = checker
    out = {}
    for level in (0, 2):
        W, cts = layer(eng, level, lazy=True)
        out[level] = (W, cts, eng.lt_matmul_bsgs(W, cts, keys))
    return out


@pytest.mark.parametrize("level", [0, 2])
def test_lt_matmul_bsgs_equals_the_composition(checker, reference, level):
    from liberate_fhe_amd.fhe.presets import types
    eng, keys = checker
    W, cts, got = reference[level]
    want = composition(eng, W, cts, keys, N1)
    assert isinstance(got, list) and len(got) == len(want) == 6
    for o, (g, w) in enumerate(zip(got, want)):
        assert g.level == level + 1 and g.origin == types.origins["ct"] and not g.ntt_state and not g.include_special
        assert same(g, w), (level, o)
    if level == 0:   # any iterables, a list of keys in any order, n1 given and agreeing
        again = eng.lt_matmul_bsgs(iter([iter(row) for row in W]), (c for c in cts), [keys[s] for s in reversed(sorted(keys))], n1=N1)
        assert all(same(a, b) for a, b in zip(again, got))


@pytest.mark.parametrize("level", [0, 2])
def test_one_input_gives_the_words_of_linear_transform(checker, level):
    """Consequence 1: k_in = 1, output o is linear_transform(ct, W[o][0], keys) in its BSGS form, word for word."""
    eng, keys = checker
    ct = lazy_ciphertext(eng, 70 + level, level)
    sets = [LAYOUT[0][0], LAYOUT[1][0], LAYOUT[4][0], (0,), (8, 9)]
    W = [[synth.diagonals_bsgs(eng, 5 + o, level, st, N1)] for o, st in enumerate(sets)]
    got = eng.lt_matmul_bsgs(W, [ct], keys)
    assert len(got) == len(sets)
    for o, g in enumerate(got):
        assert g.level == level + 1 and same(g, eng.linear_transform(ct, W[o][0], keys)), (level, o)


@pytest.mark.parametrize("level", [0, 2])
def test_giant_step_zero_alone_gives_the_words_of_lt_matmul(checker, level):
    """Consequence 2: every step below n1, so the only giant step is 0: output o has the words of lt_matmul on the same packs
    tagged flat (synth.diagonals and synth.diagonals_bsgs give a step the same words for the same seed)."""
    eng, keys = checker
    layout = [[(0, 1, 2, 3), (0,), (1, 3)], [None, (0,), (2,)], [(1, 2), None, (0, 3)]]
    Wb, cts = layer(eng, level, layout=layout, lazy=True)
    Wf = [[None if st is None else synth.diagonals(eng, 7 + 8 * o + i, level, st) for i, st in enumerate(row)] for o, row in enumerate(layout)]
    assert all(torch.equal(x[0], y[0]) for rb, rf in zip(Wb, Wf) for b, f in zip(rb, rf) if b is not None for x, y in zip(b.data, f.data))
    assert eng.lt_matmul_bsgs_steps(Wb) == (N1, [0, 1, 2, 3], [0])
    got, want = eng.lt_matmul_bsgs(Wb, cts, keys), eng.lt_matmul(Wf, cts, keys)
    assert len(got) == len(want) == 3 and all(same(a, b) for a, b in zip(got, want))


def test_an_output_depends_on_its_row_only(checker, reference):
    """Consequence 3: lt_matmul_bsgs(W, ..)[o] equals lt_matmul_bsgs([W[o]], ..)[0] whatever the grouping; and for k_in > 1 with a
    keyed giant step the words are the op's own: cc_add over separate transforms comes down once per block and differs."""
    eng, keys = checker
    W, cts, got = reference[0]
    for o in range(6):
        assert same(eng.lt_matmul_bsgs([W[o]], cts, keys)[0], got[o]), o
    pair = eng.lt_matmul_bsgs([W[3], W[0]], cts, keys)
    assert same(pair[0], got[3]) and same(pair[1], got[0])
    loop = eng.linear_transform(cts[0], W[0][0], keys)
    for i in (1, 2):
        loop = eng.cc_add(loop, eng.linear_transform(cts[i], W[0][i], keys))
    assert loop.level == got[0].level and not same(loop, got[0])


def test_plain_mappings_give_the_result_of_the_objects_encoded_for_them(checker, monkeypatch):
    """A {step: vector} mapping is encoded with bsgs=n1 at the ciphertexts' level, each distinct mapping object once; the result
    is that of the matrix with those objects in the mappings' places (encode draws its rounding at random: the very objects)."""
    eng, keys = checker
    cts = [synth.ciphertext(eng, 31 + i, 1) for i in range(2)]
    m1 = {5: [0.5, -0.25], 0: [1.0, 2.0, -1.0], 8: [0.125]}
    m2 = {n + 1: [1.0], -4084: [0.5]}                                    # steps 1 and 12
    obj = synth.diagonals_bsgs(eng, 3, 1, (0, 4, 6), N1)
    W = [[m1, obj], [m2, m1], [None, m2]]
    made = []
    real = eng.encode_diagonals
    monkeypatch.setattr(eng, "encode_diagonals", lambda *a, **k: (made.append((real(*a, **k), a, k)), made[-1][0])[1])
    got = eng.lt_matmul_bsgs(W, cts, keys)
    monkeypatch.undo()
    assert [(a[0] is m, a[1], k) for (_, a, k), m in zip(made, (m1, m2))] == [(True, 1, {"bsgs": N1})] * 2      # row-major, each once
    e1, e2 = made[0][0], made[1][0]
    assert eng.bsgs_steps(e1) == (N1, [0, 1], [0, 4, 8]) and eng.bsgs_steps(e2) == (N1, [0, 1], [0, 12])
    want = eng.lt_matmul_bsgs([[e1, obj], [e2, e1], [None, e2]], cts, keys)
    assert all(same(a, b) for a, b in zip(got, want))
    # mappings only: n1 comes from the argument
    only = eng.lt_matmul_bsgs([[{0: [1.0], 9: [0.5]}]], cts[:1], keys, n1=N1)
    assert len(only) == 1 and only[0].level == 2


def test_lt_matmul_bsgs_steps(checker):
    """(n1, babies, giants): the unions over all blocks in the sense of bsgs_steps, steps taken mod num_slots, 0 where present.
    0 is the one step that can stand in both lists (b < n1 <= g for any other giant step): it needs no key in either."""
    eng, keys = checker
    W, _ = layer(eng, 0)
    assert eng.lt_matmul_bsgs_steps(W) == (N1, [0, 1, 2, 3], [0, 4, 8, 12])
    assert eng.lt_matmul_bsgs_steps(W, n1=N1) == eng.lt_matmul_bsgs_steps(iter([iter(r) for r in W]))
    assert sorted(s for part in eng.lt_matmul_bsgs_steps(W)[1:] for s in part if s) == sorted(KEY_STEPS)
    union = encdec.bsgs_split([s for row in LAYOUT for st in row if st is not None for s in st], n, N1)
    assert eng.lt_matmul_bsgs_steps(W) == union
    assert eng.lt_matmul_bsgs_steps([[{0: [1.0]}, None]], n1=8) == (8, [0], [0])
    assert eng.lt_matmul_bsgs_steps([[{-1: [1.0], n + 2: [1.0]}], [{9: [1.0]}]], n1=4) == (4, [1, 2, 3], [0, 8, n - 4])
    assert eng.lt_matmul_bsgs_steps([[{4: [1.0], 1: [1.0]}]], n1=4) == (4, [0, 1], [0, 4])       # 0 in both lists
    assert eng.lt_matmul_bsgs_steps([[{7: [1.0], 3: [1.0]}, synth.diagonals_bsgs(eng, 1, 0, (3, 6), 3)]]) == (3, [0, 1], [3, 6])
    # the flat op keeps refusing tagged blocks, in both of its entries
    with pytest.raises(NotImplementedError):
        eng.lt_matmul_steps(W)
    with pytest.raises(NotImplementedError):
        eng.lt_matmul(W, [synth.ciphertext(eng, 1, 0)] * 3, keys)


def test_refusals_come_before_anything_is_computed(checker, monkeypatch):
    """Every refusal is raised with nothing computed, encoded or allocated: the backend, linear_transform, encode_diagonals, the
    ntt ops and every allocation are patched to record, and none is reached.  The engine works afterwards."""
    from liberate_fhe_amd.fhe.presets import errors
    eng, keys = checker
    top = eng.num_levels - 1
    c0, c1, ctop = (synth.ciphertext(eng, 60 + i, lvl) for i, lvl in enumerate((0, 1, top)))
    d0, d1 = synth.diagonals_bsgs(eng, 3, 0, (0, 1, 5), 4), synth.diagonals_bsgs(eng, 3, 1, (0, 1), 4)
    d8 = synth.diagonals_bsgs(eng, 3, 0, (0, 1, 9), 8)
    dtop = synth.diagonals_bsgs(eng, 3, top, (0,), 4)
    flat = synth.diagonals(eng, 3, 0, (0, 1, 5))
    ntt = eng._new(c0.data, c0.origin, level=0, ntt_state=True)
    special = eng._new(c0.data, c0.origin, level=0, include_special=True)
    cap_keys, cap_in = eng.lt_matmul_max_column_keys, eng.lt_matmul_max_inputs
    assert (cap_keys, cap_in) == (63, 64) and eng.lt_matmul_bsgs_group == 4
    wide = {s: [1.0] for s in range(1, cap_keys + 2)}                      # 64 keyed baby steps in one block under n1 = 128
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
    for name in ("lt_matmul_bsgs_native", "lt_matmul_bsgs_ws_words", "lt_matmul_native", "galois", "ntt", "intt", "ks_fwd", "ks_tail",
                 "ks_inner", "ks_moddown_ws"):
        monkeypatch.setattr(eng.backend, name, boom(name), raising=False)
    for name in ("enter_ntt", "mont_mult", "mont_add", "mont_enter", "intt_exit_reduce"):
        monkeypatch.setattr(eng.ntt, name, boom(name))
    real_empty, real_zeros = torch.empty, torch.zeros
    monkeypatch.setattr(torch, "empty", lambda *a, **k: (calls.append("empty"), real_empty(*a, **k))[1])
    monkeypatch.setattr(torch, "zeros", lambda *a, **k: (calls.append("zeros"), real_zeros(*a, **k))[1])
    cases = [
        (ValueError, [], [c0], keys, None),                                        # W empty
        (ValueError, [[d0]], [], keys, None),                                      # cts empty
        (ValueError, [[]], [], keys, 4),
        (ValueError, [[d0, d0], [d0]], [c0, c0], keys, None),                      # ragged
        (ValueError, [[d0], [d0]], [c0, c0], keys, None),                          # len(W[o]) != len(cts)
        (ValueError, [[d0, d0, d0]], [c0, c0], keys, None),
        (ValueError, [[d0, None], [None, None]], [c0, c0], keys, None),            # a row with no block
        (ValueError, [[d0, d8]], [c0, c0], many_keys, None),                       # blocks of different n1
        (ValueError, [[d0], [d8]], [c0], many_keys, None),
        (ValueError, [[d0]], [c0], keys, 8),                                       # the argument disagrees with the objects
        (ValueError, [[d0, {1: [1.0]}]], [c0, c0], keys, 2),
        (ValueError, [[{0: [1.0]}]], [c0], keys, None),                            # mappings only and no n1
        (ValueError, [[{0: [1.0]}, None], [None, {1: [1.0]}]], [c0, c0], keys, None),
        (ValueError, [[{0: [1.0]}]], [c0], keys, 0),                               # no n1 at all
        (ValueError, [[d0]], [c0], keys, 2.5),
        (ValueError, [[wide]], [c0], many_keys, 128),                              # more keyed baby steps in a column than the cap
        (ValueError, split, [c0], many_keys, 128),
        (ValueError, [[d0] * (cap_in + 1)], [c0] * (cap_in + 1), keys, None),      # k_in above its cap
        (ValueError, [[{}]], [c0], keys, 4),                                       # a mapping without a diagonal
        (ValueError, [[{1: [1.0], 1 + n: [2.0]}]], [c0], keys, 4),                 # the same step twice mod num_slots
        (errors.NotMatchType, [[flat]], [c0], keys, None),                         # a flat-tagged object
        (errors.NotMatchType, [[d0, flat]], [c0, c0], keys, 4),
        (errors.NotMatchType, [[c0]], [c0], keys, None),                           # a ciphertext where diagonals belong
        (errors.NotMatchType, [[d0]], [d0], keys, None),                           # .. and the other way round
        (errors.NotMatchType, [[d0, None]], [c0, None], keys, None),               # (a None ciphertext, even in an unused column)
        (errors.NotMatchType, [[3.5]], [c0], keys, 4),
        (errors.NotMatchType, [[d0]], [c0], [keys[1], keys[4], synth.key_switch_key(eng, 8)], None),   # a key of another kind
        (errors.NotMatchType, [[d0]], [c0], [keys[1]], None),                      # a missing giant key (step 4)
        (errors.NotMatchType, [[d0]], [c0], [keys[4]], None),                      # a missing baby key (step 1)
        (errors.NotMatchType, [[d0]], [c0], {1: keys[1], 5: many_keys[5]}, None),  # the flat form's keys do not serve
        (errors.NotMatchType, [[{0: [1.0], 17: [1.0]}]], [c0], keys, 4),           # .. for a plain mapping (giant step 16)
        (errors.NotMatchDataStructState, [[d1]], [c0], keys, None),                # a block of another level
        (errors.NotMatchDataStructState, [[d0, None], [d0, d1]], [c0, c0], keys, None),
        (errors.NotMatchDataStructState, [[d0, d0]], [c0, c1], keys, None),        # ciphertexts of different levels
        (errors.NotMatchDataStructState, [[d0, None]], [c0, c1], keys, None),      # (an unused column is still of the level)
        (errors.MaximumLevelError, [[dtop]], [ctop], keys, None),
        (errors.MaximumLevelError, [[{0: [1.0]}]], [ctop], keys, 4),
        (NotImplementedError, [[d0]], [ntt], keys, None),                          # an NTT-domain ciphertext
        (NotImplementedError, [[d0, None]], [c0, special], keys, None),            # special limbs
    ]
    for exc, W, cts, ks, n1 in cases:
        with pytest.raises(exc):
            eng.lt_matmul_bsgs(W, cts, ks, n1=n1)
    with pytest.raises(errors.NotMatchType, match="step 4"):                      # the missing step is named
        eng.lt_matmul_bsgs([[d0]], [c0], [keys[1]])
    with pytest.raises(errors.NotMatchType, match="diagonals bsgs"):              # what a flat object is refused for
        eng.lt_matmul_bsgs([[flat]], [c0], keys)
    for W, n1 in (([[flat]], None), ([[d0], [d8]], None), ([[{0: [1.0]}]], None), ([[d0]], 8), ([[d0], [d0, d0]], None), ([[wide]], 128)):
        with pytest.raises((ValueError, errors.NotMatchType)):
            eng.lt_matmul_bsgs_steps(W, n1)
    assert calls == []
    monkeypatch.undo()
    # exactly the cap is legal as far as the checks go (the missing key is the first complaint), and the engine still works
    with pytest.raises(errors.NotMatchType):
        eng.lt_matmul_bsgs([[{s: [1.0] for s in range(0, cap_keys + 1)}]], [c0], keys, n1=128)
    out = eng.lt_matmul_bsgs([[d0, None], [None, {0: [1.0, 0.5]}]], [c0, c0], keys)
    assert [o.level for o in out] == [1, 1]
    assert same(out[0], eng.linear_transform(c0, d0, keys))
    # an input that no output uses is legal: its ciphertext is not read
    poisoned = c0._replace(data=([None], [None]))
    assert same(eng.lt_matmul_bsgs([[d0, None]], [c0, poisoned], keys)[0], out[0])


def test_two_logical_devices_give_the_single_device_words():
    """Two shards take the orchestrated steps with a digit exchange per input and per keyed (output, giant step); row by row in
    prime order the words of one device."""
    from liberate_fhe_amd.fhe import ckks_engine
    from tests.oracle_backend import OracleBackend
    from tests.test_pc_dot_gpu import natural_rows
    res = []
    layout = [LAYOUT[0], LAYOUT[1], LAYOUT[5]]
    for ndev in (1, 2):
        eng = ckks_engine(devices=["cpu"] * ndev, backend=OracleBackend(), **LT)
        assert ndev == 1 or eng._native_level(0) is None
        W, cts = layer(eng, 0, layout=layout)
        out = eng.lt_matmul_bsgs(W, cts, keys_for(eng))
        assert len(out) == 3 and all(o.level == 1 for o in out)
        res.append([natural_rows(eng, o) for o in out])
    for a, b in zip(*res):
        for x, y in zip(a, b):
            assert x.shape == y.shape and (x == y).all()


def test_c_entry_refuses_bad_arguments_before_any_launch():
    """lf_lt_matmul_bsgs returns LF_ERR_ARG from its arguments alone (dummy pointers that are never dereferenced; no call here
    would pass the checks); lf_lt_matmul_bsgs_ws_words gives the header's formula and 0 for what the entry refuses; both names are
    exported, the ABI version stays 15 and the caps are the header's everywhere."""
    from liberate_fhe_amd import _native
    from liberate_fhe_amd._native import lib, EXPORTED
    from liberate_fhe_amd.fhe.backend import HipBackend
    LF_ERR_ARG = 10001
    assert "lf_lt_matmul_bsgs" in EXPORTED and "lf_lt_matmul_bsgs_ws_words" in EXPORTED and lib.lf_abi_version() == 15
    header = open(os.path.join(ROOT, "include", "ckks_hip.h")).read()
    OMAX = int(re.search(r"#define LF_LT_MATMUL_MAX_OUTPUTS (\d+)", header).group(1))
    IMAX = int(re.search(r"#define LF_LT_MATMUL_MAX_INPUTS (\d+)", header).group(1))
    KMAX = int(re.search(r"#define LF_BSGS_MAX_BABY_KEYS (\d+)", header).group(1))
    GMAX = int(re.search(r"#define LF_LT_MATMUL_BSGS_MAX_GIANTS (\d+)", header).group(1))
    SMAX = int(re.search(r"#define LF_LT_MATMUL_BSGS_MAX_SUMS (\d+)", header).group(1))
    assert (GMAX, SMAX) == (_native.LF_LT_MATMUL_BSGS_MAX_GIANTS, _native.LF_LT_MATMUL_BSGS_MAX_SUMS) == \
        (HipBackend.lt_matmul_bsgs_max_giants, HipBackend.lt_matmul_bsgs_max_sums) == (64, 256)
    for logN in (13, 15, 17):
        for max_nct in (1, 2, 4):
            plan = _fake_plan(logN)
            plan.max_nct = max_nct
            N, rows, ell, K = 1 << logN, 3, 2, 1
            for nb in (0, 1, 7, KMAX):
                for k_out in (1, 2, 3, 4, 5, OMAX):
                    for sums in (0, 1, 8, SMAX):
                        g4, gw = min(k_out, 4), min(4, max_nct)
                        want = 2 * rows * N * (nb + 1 + k_out + sums) + gw * ell * N + 2 * g4 * ell * N + \
                            max(lib.lf_ks_moddown_ws_words(gw, ell, K, N), lib.lf_ks_moddown_ws_words(2 * g4, ell, K, N))
                        assert lib.lf_lt_matmul_bsgs_ws_words(ctypes.byref(plan), nb, k_out, sums) == want, (logN, max_nct, nb, k_out, sums)
    plan = _fake_plan(13)
    for nb, k_out, sums in ((-1, 1, 0), (KMAX + 1, 1, 0), (0, 0, 0), (0, -1, 0), (0, OMAX + 1, 0), (0, 1, -1), (0, 1, SMAX + 1)):
        assert lib.lf_lt_matmul_bsgs_ws_words(ctypes.byref(plan), nb, k_out, sums) == 0, (nb, k_out, sums)
    for logN in (12, 18):
        assert lib.lf_lt_matmul_bsgs_ws_words(ctypes.byref(_fake_plan(logN)), 1, 1, 1) == 0
    assert lib.lf_lt_matmul_bsgs_ws_words(None, 1, 1, 1) == 0

    dummy = ctypes.c_void_p(64)
    stride = 3 << 13

    def i64(values):
        return (ctypes.c_int64 * max(1, len(values)))(*values)

    def ptrs(count, null_at=()):
        arr = (ctypes.c_void_p * max(count, 1))(*([64] * max(count, 1)))
        for at in null_at:
            arr[at] = None
        return arr

    # 2 inputs x 2 outputs x 2 giant steps (0 and exponent 5): column 0 has two baby keys (exponents 3, 7), column 1 none.
    # [o][i][j]: (0,0,0) slots 0,1,2; (0,0,1) slot 1; (1,0,1) slot 2; (1,1,0) slot 0; the rest NULL.  Two keyed sums.
    NUL = [2, 3, 4, 7]

    def call(plan=plan, k_in=2, k_out=2, ng=2, scales=dummy, ws=dummy, ws_words=1 << 40, fmt=0, part_stride=0, **over):
        a = {"ins": ptrs(2 * max(k_in, 1)), "bkeys": ptrs(4), "gkeys": ptrs(4), "pts": ptrs(8, NUL), "out0": ptrs(max(k_out, 1)),
             "out1": ptrs(max(k_out, 1)), "ncol": i64((2, 0)), "bexps": i64((3, 7)), "gexps": i64((0, 5)),
             "strides": i64((stride, stride, 0, 0, 0, stride, stride, 0)), "counts": i64((3, 1, 0, 0, 0, 1, 1, 0)),
             "bidx": i64((0, 1, 2, 1, 2, 0))}
        for name, value in over.items():
            assert name in a
            a[name] = value if value is None or isinstance(value, ctypes.Array) else i64(value)
        return lib.lf_lt_matmul_bsgs(ctypes.byref(plan) if plan is not None else None, k_in, k_out, a["ins"], a["ncol"], a["bexps"],
                                     a["bkeys"], ng, a["gexps"], a["gkeys"], part_stride, 0, 0, fmt, a["pts"], a["strides"], a["counts"],
                                     a["bidx"], scales, 0, ws, ws_words, a["out0"], a["out1"], None)

    N2 = 2 << 13
    need = lib.lf_lt_matmul_bsgs_ws_words(ctypes.byref(plan), 2, 2, 2)
    assert need > 0 and call(ws_words=need - 1) == LF_ERR_ARG                  # (the one call whose other arguments are all good)
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
    for ng in (0, -1, GMAX + 1):
        assert call(ng=ng) == LF_ERR_ARG, ng
    for name in ("ins", "ncol", "bexps", "bkeys", "gexps", "gkeys", "pts", "strides", "counts", "bidx", "out0", "out1"):
        assert call(**{name: None}) == LF_ERR_ARG, name
    assert call(scales=None) == LF_ERR_ARG
    assert call(fmt=2) == LF_ERR_ARG and call(fmt=-1) == LF_ERR_ARG
    assert call(ncol=(-1, 0)) == LF_ERR_ARG and call(ncol=(KMAX + 1, 0)) == LF_ERR_ARG        # a count out of range
    for at in (0, 1, 2, 3):                                                    # a NULL among the used pointers
        assert call(ins=ptrs(4, [at])) == LF_ERR_ARG, at
    for at in (0, 1):
        assert call(bkeys=ptrs(4, [at])) == LF_ERR_ARG
        assert call(out0=ptrs(2, [at])) == LF_ERR_ARG and call(out1=ptrs(2, [at])) == LF_ERR_ARG
    assert call(gkeys=ptrs(4, [1])) == LF_ERR_ARG                              # a keyed giant step without a key
    for bad in ((4, 7), (3, N2 + 1), (-3, 7), (3, 0)):                         # even, >= 2N, negative, zero baby exponents
        assert call(bexps=bad) == LF_ERR_ARG, bad
    for bad in ((0, 6), (0, N2 + 3), (0, -5), (5, 0), (0, 0)):                 # .. giant exponents; a late or a second giant step 0
        assert call(gexps=bad) == LF_ERR_ARG, bad
    assert call(pts=ptrs(8, NUL + [0, 1])) == LF_ERR_ARG                       # an output with no diagonal at all
    assert call(pts=ptrs(8, NUL + [5, 6])) == LF_ERR_ARG
    assert call(pts=ptrs(8, NUL + [1, 5]), counts=(3, 0, 0, 0, 0, 0, 1, 0), bidx=(0, 1, 2, 0)) == LF_ERR_ARG   # a keyed giant step no output uses
    assert call(pts=ptrs(8, NUL + [1]), counts=(3, 1, 0, 0, 0, 1, 1, 0)) == LF_ERR_ARG       # a NULL pack that claims diagonals
    assert call(counts=(3, 1, 1, 0, 0, 1, 1, 0)) == LF_ERR_ARG
    assert call(counts=(3, 0, 0, 0, 0, 1, 1, 0), bidx=(0, 1, 2, 2, 0)) == LF_ERR_ARG         # a pack without diagonals
    assert call(counts=(4, 1, 0, 0, 0, 1, 1, 0), bidx=(0, 1, 2, 2, 1, 2, 0)) == LF_ERR_ARG   # more diagonals than the column has slots
    assert call(strides=(stride - 1, stride, 0, 0, 0, stride, stride, 0)) == LF_ERR_ARG
    assert call(bidx=(0, 1, 3, 1, 2, 0)) == LF_ERR_ARG                         # a slot outside its column's set
    assert call(bidx=(0, 1, 2, 1, 2, 1)) == LF_ERR_ARG                         # (column 1 has slot 0 only)
    assert call(bidx=(-1, 1, 2, 1, 2, 0)) == LF_ERR_ARG
    assert call(bidx=(1, 0, 2, 1, 2, 0)) == LF_ERR_ARG                         # slots not ascending inside one (o, i, j)
    assert call(bidx=(0, 1, 1, 1, 2, 0)) == LF_ERR_ARG
    assert call(fmt=1, bkeys=(ctypes.c_void_p * 4)(72, 64, 64, 64)) == LF_ERR_ARG      # a planes key not 16-byte aligned
    assert call(fmt=1, gkeys=(ctypes.c_void_p * 4)(64, 72, 64, 64)) == LF_ERR_ARG
    assert call(fmt=1, part_stride=1) == LF_ERR_ARG
    assert call(ws=None) == LF_ERR_ARG
    assert call(ws=ctypes.c_void_p(72)) == LF_ERR_ARG                          # misaligned
    assert call(ws_words=0) == LF_ERR_ARG
    # more keyed sums than one call takes: 64 outputs x 5 keyed giant steps, one input, every (o, j) with one diagonal
    k_out, ng = OMAX, 6
    cnt = k_out * ng
    assert k_out * (ng - 1) > SMAX
    assert call(k_in=1, k_out=k_out, ng=ng, ncol=(0,), gexps=(0, 3, 5, 7, 9, 11), gkeys=ptrs(ng), pts=ptrs(cnt), strides=[stride] * cnt,
                counts=[1] * cnt, bidx=[0] * cnt, out0=ptrs(k_out), out1=ptrs(k_out)) == LF_ERR_ARG
    # the pointers of an input no block uses are not among the checked ones: with column 1 unused its NULLs are not what is
    # refused (the call is still refused, by its workspace, so nothing is launched)
    unused = dict(pts=ptrs(8, NUL + [6]), counts=(3, 1, 0, 0, 0, 1, 0, 0), bidx=(0, 1, 2, 1, 2), ins=ptrs(4, [2, 3]))
    assert call(ws_words=need - 1, **unused) == LF_ERR_ARG


def test_giant_batch_kernels_use_no_scratch():
    """ks_inner_giantb_kernel<2 | 4, raw / planes key, raw / planes digits> exist in ckks_ks.hip under these names with scratch 0
    and no spill.  For four outputs the 16 accumulators, 4 digit pairs and 4 key words had to stay within 128 VGPRs (4 waves per
    SIMD); the compiler reports 72 - 74 for them and 68 - 78 for two outputs, 6 waves per SIMD with a planes key and 7 with a raw
    one, which is what DESIGN.md states and what is held here (ks_inner_baby_kernel<4> has 3); the tracked table lists them as
    built."""
    import __graft_entry__ as g
    res = {r["kernel"]: r for r in g.kernel_resources()}
    fmts = [(pl, dpl) for pl in ("true", "false") for dpl in ("true", "false")]
    want = [f"ks_inner_giantb_kernel<{nct}, {pl}, {dpl}>" for nct in (2, 4) for pl, dpl in fmts]
    assert sorted(k for k in res if k.startswith("ks_inner_giantb_kernel")) == sorted(want)
    tracked = open(os.path.join(ROOT, "profiles", "r06_kernel_resources.txt")).read()
    for k in want:
        r = res[k]
        assert r["file"] == "ckks_ks.hip" and r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, r
        pl, dpl = k[len("ks_inner_giantb_kernel<4, "):-1].split(", ")
        assert r["vgprs"] <= 80 and r["occupancy"] >= (6 if pl == "true" else 7), r
        assert r["occupancy"] >= max(3, res[f"ks_inner_baby_kernel<4, {pl}, {dpl}>"]["occupancy"]), r
        line = next(ln for ln in tracked.splitlines() if ln[18:76].strip() == k)
        f = line.split()
        assert (int(f[-7]), int(f[-3]), int(f[-1])) == (r["vgprs"], r["scratch"], r["occupancy"]), line


def matmul_bsgs_errors(eng, sk, cts, ms, rng, m=8, n1=4):
    """(max error of lt_matmul_bsgs, max error of the loop of BSGS linear_transform + cc_add, keys, giant steps) for a 2 x 2 matrix
    of random block-diagonal matrices (m x m blocks: steps -(m - 1) .. m - 1) on the same ciphertexts, encoded diagonals and keys,
    against the numpy product."""
    A = [[rng.uniform(-1, 1, (m, m)) for _ in range(2)] for _ in range(2)]
    W = [[eng.encode_diagonals(block_diagonals(A[o][i], eng.num_slots), cts[0].level, bsgs=n1) for i in range(2)] for o in range(2)]
    _, babies, giants = eng.lt_matmul_bsgs_steps(W)
    keys = [eng.create_rotation_key(sk, s) for s in sorted(set(babies + giants)) if s]
    want = [sum((A[o][i] @ ms[i].reshape(-1, m).T).T.reshape(-1) for i in range(2)) for o in range(2)]
    got = eng.lt_matmul_bsgs(W, cts, keys)
    loop = [eng.cc_add(eng.linear_transform(cts[0], W[o][0], keys), eng.linear_transform(cts[1], W[o][1], keys)) for o in range(2)]
    e_mat = max(np.abs(eng.decrode(g, sk) - w).max() for g, w in zip(got, want))
    e_loop = max(np.abs(eng.decrode(g, sk) - w).max() for g, w in zip(loop, want))
    return e_mat, e_loop, len(keys), giants


def test_decryption_error_with_real_keys_stays_within_twice_the_loop():
    """Real keys on the checker engine, 2 x 2 blocks from random block-diagonal matrices (8 x 8 blocks: 15 diagonals, steps
    -7 .. 7; n1 = 4: baby keys 1, 2, 3 and the keyed giant steps 4, n - 8, n - 4), fresh ciphertexts at level 0: decrode against
    the numpy product, at most 2 x the maximum error of the loop of BSGS linear_transform + cc_add on the same ciphertexts,
    diagonals and keys (the project's margin for a maximum over 2^12 slots between two roundings of one quantity).  Both errors
    are printed."""
    eng, sk, pk = _real_engine()
    rng = np.random.default_rng(9)
    ms = [rng.uniform(-4, 4, n) + 1j * rng.uniform(-4, 4, n) for _ in range(2)]
    cts = [eng.encorypt(m, pk) for m in ms]
    e_mat, e_loop, nkeys, giants = matmul_bsgs_errors(eng, sk, cts, ms, rng)
    print(f"logN 13, 2 x 2 blocks of 15 diagonals, n1 = 4, {nkeys} keys, level 0: max error lt_matmul_bsgs {e_mat:.3e}, "
          f"loop of BSGS linear_transform + cc_add {e_loop:.3e}")
    assert giants == [0, 4, n - 8, n - 4] and nkeys == 6
    assert e_mat <= 2 * e_loop and e_loop < 1e-6
