"""lt_matmul_bsgs_batch on the GPU: lf_lt_matmul_bsgs_batch (one native call per group of 4 or 2 token vectors: the baby sums of
lf_lt_matmul_batch, lt_block_productsb_kernel per tile of two tokens over the pairs of an output and a giant step, the giant step
of lf_lt_matmul_bsgs in chunks of up to 4 (token, output) members) against the loop of lt_matmul_bsgs that defines its words — at
logN 13 over every grouping on the reference layout, against linear_transform for one input and lt_matmul_batch for giant step 0
alone, over more keyed sums than one call takes, at the presets, against the checker engine, with compact keys, under the tuning
knobs and lt_matmul_bsgs_group, at worst-case words, fenced, on held streams and once with real keys.  No tolerance anywhere:
every comparison of words is torch.equal."""
import inspect
import time
import warnings

import numpy as np
import pytest
import torch

from liberate_fhe_amd.utils import synth
from tests.helpers import FENCE_FILLS, BackendSpy, Fence, edge_ciphertext, edge_diagonals, edge_key, hold, independent_streams, still_held
from tests.test_inner_sum_cpu import lazy_ciphertext
from tests.test_lt_matmul_batch_gpu import all_same, engine_of, groups, same, strided, words
from tests.test_lt_matmul_bsgs_cpu import LAYOUT, LT, N1, giants_of, keys_for

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore", category=UserWarning)

ENTRY = "lt_matmul_bsgs_batch_call"
LF_ERR_ARG = 10001


def matrix(eng, level, layout, seed=7, n1=N1):
    return [[None if st is None else synth.diagonals_bsgs(eng, seed + 8 * o + i, level, st, n1) for i, st in enumerate(row)]
            for o, row in enumerate(layout)]


def tokens(eng, level, k_in, B, seed=90):
    return [[synth.ciphertext(eng, seed + 10 * level + k_in * t + i, level) for i in range(k_in)] for t in range(B)]


class native_calls:
    """[tokens per lf_lt_matmul_bsgs_batch call] while the block runs, with groups of 4 and 2 whatever sizes the engine ships: a
    silent fall-back to the loop shows as a missing entry"""

    def __init__(self, eng, sizes=(4, 2)):
        self.eng, self.sizes, self.seen = eng, sizes, []

    def __enter__(self):
        real = getattr(self.eng.backend, ENTRY)

        def spy(plan, toks, *a, **kw):
            self.seen.append(len(toks))
            return real(plan, toks, *a, **kw)
        setattr(self.eng.backend, ENTRY, spy)
        self.eng.lt_matmul_bsgs_batch_sizes = self.sizes
        return self.seen

    def __exit__(self, *exc):
        delattr(self.eng.backend, ENTRY)
        del self.eng.lt_matmul_bsgs_batch_sizes


@pytest.fixture(scope="module")
def lt_engine():
    from liberate_fhe_amd.fhe import ckks_engine
    eng = ckks_engine(devices=["cuda:0"], **LT)
    assert set(type(eng).lt_matmul_bsgs_batch_sizes) <= set(eng.backend.lt_matmul_bsgs_batch_sizes) == {4, 2}
    return eng, keys_for(eng)


@pytest.mark.parametrize("level", [0, 2, 3])
def test_native_batch_equals_the_loop_at_logN_13(lt_engine, level):
    """The reference layout, 6 x 3, n1 = 4: giant step 4 in five outputs, 8 in two, 12 in one (with two tokens the giant chunks are
    4 + 4 + 2, 4 and 2; with four every chunk is one output's four tokens), an output without giant step 0, one with giant step 0
    only, a column without keys.  Levels 0, 2 and L - 2; B = 1, 2, 3, 4, 5, 7 against the loop computed once; token 1 is lazy."""
    eng, keys = lt_engine
    assert level <= eng.num_levels - 2 and (level != 3 or level == eng.num_levels - 2) and eng._native_level(level) is not None
    per_giant = {g: sum(g in giants_of(r) for r in LAYOUT) for g in (4, 8, 12)}
    assert per_giant == {4: 5, 8: 2, 12: 1} and 0 not in giants_of(LAYOUT[1]) and giants_of(LAYOUT[5]) == [0]
    W = matrix(eng, level, LAYOUT)
    X = tokens(eng, level, 3, 7)
    X[1] = [lazy_ciphertext(eng, 97 + level + i, level) for i in range(3)]
    want = [eng.lt_matmul_bsgs(W, cts, keys) for cts in X]
    assert all(o.level == level + 1 for w in want for o in w)
    with native_calls(eng) as seen:
        for B, calls in ((1, []), (2, [2]), (3, [2]), (4, [4]), (5, [4]), (7, [4, 2])):
            assert groups(B) == calls
            del seen[:]
            got = eng.lt_matmul_bsgs_batch(W, X[:B], keys)
            assert seen == calls, (B, seen)
            assert all_same(got, want[:B]), (level, B)


def test_three_outputs_share_one_keyed_giant_step(lt_engine):
    """B = 2: six members under giant step 4, chunks of 4 + 2, the 4 spanning two outputs."""
    eng, keys = lt_engine
    W = matrix(eng, 1, [[(0, 4, 5)], [(1, 6)], [(4, 7)]])
    X = tokens(eng, 1, 1, 2)
    with native_calls(eng) as seen:
        got = eng.lt_matmul_bsgs_batch(W, X, keys)
    assert seen == [2]
    assert all_same(got, [eng.lt_matmul_bsgs(W, cts, keys) for cts in X])


def test_one_input_gives_the_words_of_linear_transform(lt_engine):
    """k_in = 1, five tokens (4 + a straggler): output o of token t is the BSGS linear_transform(X[t][0], W[o][0], keys)."""
    eng, keys = lt_engine
    W = matrix(eng, 1, [[LAYOUT[0][0]], [LAYOUT[1][0]], [(0,)], [(8, 9)]])
    X = tokens(eng, 1, 1, 5)
    with native_calls(eng) as seen:
        got = eng.lt_matmul_bsgs_batch(W, X, keys)
    assert seen == [4] and len(got) == 5
    for t, (g, cts) in enumerate(zip(got, X)):
        assert len(g) == 4
        for o, out in enumerate(g):
            assert same(out, eng.linear_transform(cts[0], W[o][0], keys)), (t, o)


def test_giant_step_zero_alone_gives_the_words_of_lt_matmul_batch(lt_engine):
    eng, keys = lt_engine
    layout = [[(0, 1, 2, 3), (0,), (1, 3)], [None, (0,), (2,)], [(1, 2), None, (0, 3)]]
    Wb = matrix(eng, 1, layout)
    Wf = [[None if st is None else synth.diagonals(eng, 7 + 8 * o + i, 1, st) for i, st in enumerate(row)] for o, row in enumerate(layout)]
    X = tokens(eng, 1, 3, 6)
    with native_calls(eng) as seen:
        got = eng.lt_matmul_bsgs_batch(Wb, X, keys)
    assert seen == [4, 2]
    assert all_same(got, eng.lt_matmul_batch(Wf, X, keys))


def test_a_member_that_is_not_contiguous_takes_the_loop_and_keeps_its_place(lt_engine):
    eng, keys = lt_engine
    level, layout = 1, [[(0, 1, 5), None, (2, 4)], [None, None, (0, 6, 9)], [(5,), None, None]]       # (column 1 is unused)
    W = matrix(eng, level, layout)
    X = tokens(eng, level, 3, 6)
    want = [eng.lt_matmul_bsgs(W, cts, keys) for cts in X]
    X[2][2] = strided(eng, X[2][2])
    X[3][1] = strided(eng, X[3][1])                                   # (an unused column: this token still qualifies)
    assert not X[2][2].data[0][0].is_contiguous()
    with native_calls(eng) as seen:
        got = eng.lt_matmul_bsgs_batch(W, X + [X[0]], keys)          # six that qualify (4 + 2), one that does not, one repeated
    assert seen == [4, 2]
    assert all_same(got, want + [want[0]])


def test_more_keyed_sums_than_one_call_takes(lt_engine):
    """54 outputs of 5 keyed giant steps each (270 keyed sums per token, one call takes 256), as tests/test_lt_matmul_bsgs_gpu.py
    builds them: B = 2 gives two native calls for the group, and the words are those of the rows taken alone."""
    eng, _ = lt_engine
    k_out, giants = 54, (4, 8, 12, 16, 20)
    assert k_out * len(giants) > eng.backend.lt_matmul_bsgs_max_sums
    keys = keys_for(eng, (1,) + giants)
    D = [synth.diagonals_bsgs(eng, 3 + j, 0, tuple(g + (j + g // 4) % 2 for g in (0,) + giants), N1) for j in range(2)]
    W = [[D[o % 2], None if o % 4 == 1 else D[(o + 1) % 2]] for o in range(k_out)]
    X = tokens(eng, 0, 2, 2, seed=20)
    with native_calls(eng) as seen:
        got = eng.lt_matmul_bsgs_batch(W, X, keys)
    assert seen == [2, 2] and all(len(g) == k_out for g in got)
    for t, cts in enumerate(X):
        one = {}
        for o, g in enumerate(got[t]):
            kind = (o % 2, o % 4 == 1)                                    # (the rows repeat: four distinct ones)
            if kind not in one:
                one[kind] = eng.lt_matmul_bsgs([W[o]], cts, keys)[0]
            assert same(g, one[kind]), (t, o)


@pytest.mark.parametrize("name", ["silver", "sb45", "sb41", "gold", "logN17"])
def test_native_batch_equals_the_loop_at_the_presets(name):
    """2 x 2 blocks with two keyed giant steps, B = 3 (a group of 2 and a straggler) and B = 4, at levels 0 and L - 2; sb41 / sb45
    run both arithmetic classes row by row."""
    eng = engine_of(name)
    keys = keys_for(eng, (1, 2, 3, 4, 8))
    layout = [[(0, 1, 4, 6), (2, 8, 9)], [(5, 7, 11), (0, 3, 4)]]
    for level in sorted({0, eng.num_levels - 2}):
        W = matrix(eng, level, layout, seed=5 + level)
        X = tokens(eng, level, 2, 4, seed=30)
        want = [eng.lt_matmul_bsgs(W, cts, keys) for cts in X]
        with native_calls(eng) as seen:
            got3 = eng.lt_matmul_bsgs_batch(W, X[:3], keys)
            got4 = eng.lt_matmul_bsgs_batch(W, X, keys)
        assert seen == [2, 4]
        assert all_same(got3, want[:3]) and all_same(got4, want), (name, level)
        del W, X, want, got3, got4
    del eng, keys
    torch.cuda.empty_cache()


@pytest.mark.parametrize("params", [LT, dict(LT, logN=12)])
def test_gpu_batch_equals_the_loop_of_the_checker(params):
    """logN 13 (the native call: a group of 2 and a straggler) and logN 12 (the GPU engine itself takes the loop) against the
    checker engine's loop of lt_matmul_bsgs; B = 3, levels 0 and 2."""
    from liberate_fhe_amd.fhe import ckks_engine
    from tests.oracle_backend import OracleBackend
    got, want = [], []
    H = ckks_engine(devices=["cuda:0"], **params)
    C = ckks_engine(devices=["cpu"], backend=OracleBackend(), **params)
    native = params["logN"] == 13
    assert (H._native_level(0) is not None) == native
    layout = [LAYOUT[0], LAYOUT[1]]
    for eng, out in ((H, got), (C, want)):
        keys = keys_for(eng)
        for level in (0, 2):
            W = matrix(eng, level, layout)
            X = tokens(eng, level, 3, 3, seed=70)
            if eng is H:
                with native_calls(eng) as seen:
                    res = eng.lt_matmul_bsgs_batch(W, X, keys)
                assert seen == ([2] if native else [])
            else:
                res = [eng.lt_matmul_bsgs(W, cts, keys) for cts in X]
            out += [words(o) for r in res for o in r]
    assert len(got) == len(want) == 12
    assert all(torch.equal(a[c], b[c]) for a, b in zip(got, want) for c in range(2))


def test_compact_keys_give_the_same_words():
    eng = engine_of("sb41")
    sk = eng.create_secret_key()
    layout = [[(0, 1, 3, 4, 5), (2, 6)], [None, (0, 1, 2, 3, 7)], [(5,), (4,)]]
    keys = [eng.create_rotation_key(sk, d) for d in (1, 2, 3, 4)]
    W = matrix(eng, 1, layout)
    X = tokens(eng, 1, 2, 6)
    want = [eng.lt_matmul_bsgs(W, cts, keys) for cts in X]
    with native_calls(eng) as seen:
        assert all_same(eng.lt_matmul_bsgs_batch(W, X, keys), want)
        for k in keys:
            eng.compact_key(k)
        assert all_same(eng.lt_matmul_bsgs_batch(W, X, keys), want)
    assert seen == [4, 2, 4, 2]


def test_tuning_knobs_and_the_giant_group_change_no_word():
    """LF_TUNE_DIGIT_PLANES (1 / 0), LF_TUNE_MORE_PLANES (3 / 0) and LF_TUNE_KS_EXT_COLS_MAX in the five combinations of
    tests/test_lt_matmul_batch_gpu.py, then lt_matmul_bsgs_group = 1 and 2 on the engine (the loop's knob: the batch asks for a plan
    of 4): six tokens (4 + 2), 2 x 2 blocks."""
    from liberate_fhe_amd._native import lib
    eng = engine_of("sb41")
    keys = keys_for(eng)
    W = matrix(eng, 0, [LAYOUT[0][::2], LAYOUT[2][::2]])
    X = tokens(eng, 0, 2, 6, seed=12)
    want = [eng.lt_matmul_bsgs(W, cts, keys) for cts in X]
    old = (lib.lf_tune(3, -1), lib.lf_tune(5, -1), lib.lf_tune(1, -1))
    outs = []
    try:
        with native_calls(eng) as seen:
            for planes, more, cols in ((1, 3, 5), (0, 3, 5), (1, 0, 5), (1, 3, 0), (0, 0, 0)):
                lib.lf_tune(3, planes), lib.lf_tune(5, more), lib.lf_tune(1, cols)
                outs.append(eng.lt_matmul_bsgs_batch(W, X, keys))
    finally:
        lib.lf_tune(3, old[0]), lib.lf_tune(5, old[1]), lib.lf_tune(1, old[2])
    assert seen == [4, 2] * 5
    assert len(outs) == 5 and all(all_same(out, want) for out in outs)
    try:
        with native_calls(eng) as seen:
            for group in (1, 2):
                eng.lt_matmul_bsgs_group = group
                assert all_same(eng.lt_matmul_bsgs_batch(W, X[:5], keys), want[:5]), group
    finally:
        del eng.lt_matmul_bsgs_group
    assert seen == [4, 4] and eng.lt_matmul_bsgs_group == 4


EDGE_CONFIGS = (("sb40_K1", 1), ("sb41_K2", 1), ("sb45_K8", 1))
EDGE_TRIPLES = (("top", "top", "top"), ("mixed", "top", "mixed"))
# 2 x 2, n1 = 4: column 0 fills all four slots of the giant steps 0 and 4 in both of its blocks, so every accumulator and every keyed
# sum of its launches takes its full count of 4 terms; column 1 comes second: its launches read, add to and write an accumulator
# (giant step 0) and a keyed sum (giant step 4) of column 0
EDGE_LAYOUT = [[tuple(range(8)), (0, 5)], [tuple(range(8)), (1, 4)]]
_EDGE_KEYS = {}


def edge_keys(cfg, eng, pattern):
    """step -> rotation key of edge words; the keys of ONE configuration are kept, those of the previous one are dropped"""
    if _EDGE_KEYS.get("cfg") != cfg:
        _EDGE_KEYS.clear()
        _EDGE_KEYS["cfg"] = cfg
    key = (id(eng), pattern)
    if key not in _EDGE_KEYS:
        _EDGE_KEYS[key] = {s: edge_key(eng, pattern, 100 + s, origin=f"rotation key:{s}") for s in (1, 2, 3, 4)}
    return _EDGE_KEYS[key]


@pytest.mark.parametrize("last", [False, True])
@pytest.mark.parametrize("patterns", EDGE_TRIPLES)
@pytest.mark.parametrize("cfg", EDGE_CONFIGS)
def test_worst_case_words_against_the_checker_loop(cfg, patterns, last):
    """Ciphertexts, keys and diagonals on the bounds (tests/helpers.py), four tokens (two tiles of one group, giant chunks of one
    output's four tokens), at level 0 and at L - 2, word for word against the checker engine's loop of lt_matmul_bsgs."""
    from tests.test_engine_edges_gpu import engines
    H, C = engines(*cfg)
    level = H.num_levels - 2 if last else 0
    res = []
    for eng in (H, C):
        W = [[edge_diagonals(eng, level, st, patterns[2], 40 + 8 * o + i, n1=N1) for i, st in enumerate(row)]
             for o, row in enumerate(EDGE_LAYOUT)]
        X = [[edge_ciphertext(eng, level, patterns[0], 20 + level + 2 * t + i) for i in range(2)] for t in range(4)]
        keys = edge_keys(cfg, eng, patterns[1])
        if eng is H:
            with native_calls(eng) as seen:
                res.append(eng.lt_matmul_bsgs_batch(W, X, keys))
            assert seen == [4]
        else:
            res.append([eng.lt_matmul_bsgs(W, cts, keys) for cts in X])
    assert all_same(*res), (cfg, patterns, level)


FENCED_LAYOUT = [LAYOUT[0], LAYOUT[1], LAYOUT[4]]      # 3 baby keys in column 0; keyed sums 2 + 1 + 2


@pytest.fixture(scope="module")
def fenced_case(lt_engine):
    """(W, X, keys, the plain engine's words for B = 4 and B = 2) of the fenced runs, computed once"""
    eng, keys = lt_engine
    W = matrix(eng, 0, FENCED_LAYOUT)
    X = tokens(eng, 0, 3, 4, seed=40)
    with native_calls(eng) as seen:
        want = {B: [[w for o in tok for w in words(o)] for tok in eng.lt_matmul_bsgs_batch(W, X[:B], keys)] for B in (4, 2)}
    assert seen == [4, 2]
    return W, X, keys, want


@pytest.mark.parametrize("fill", sorted(FENCE_FILLS))
def test_fenced(fenced_case, fill):
    """A fresh engine under tests.helpers.Fence (guards around every scratch tensor, a hostile fill inside), the new backend entry
    wrapped here with the fence's own wrapper: B = 4 and B = 2 give the plain run's words, no guard is touched, no output is left
    unwritten; a workspace one word short or misaligned by one word is refused with every body still holding its fill."""
    from liberate_fhe_amd._native import HipError
    from liberate_fhe_amd.fhe import ckks_engine
    W, X, keys, want = fenced_case
    eng = ckks_engine(devices=["cuda:0"], **LT)
    fence = Fence(eng, FENCE_FILLS[fill])
    real = getattr(eng.backend, ENTRY)
    setattr(eng.backend, ENTRY, fence._fenced_entry(ENTRY, real, inspect.signature(real)))
    eng.lt_matmul_bsgs_batch_sizes = (4, 2)
    for B in (4, 2):
        fence.refill()
        del fence.calls[:], fence.never_written[:]
        got = eng.lt_matmul_bsgs_batch(W, X[:B], keys)
        fence.check()
        assert fence.calls == [ENTRY], (fill, B, fence.calls)
        assert not fence.never_written, (fill, B, fence.never_written)
        got = [[w for o in tok for w in words(o)] for tok in got]
        assert all(torch.equal(a, b) for g, w in zip(got, want[B]) for a, b in zip(g, w)), (fill, B)
    for misalign in (False, True):
        kept = []

        def hook(name, a, misalign=misalign):
            if name != ENTRY:
                return
            ws = a["ws"]
            n = ws.numel()
            sums = sum(len([g for g in giants_of(r) if g]) for r in FENCED_LAYOUT)
            assert sums == 5 and n == eng.backend.lt_matmul_bsgs_batch_ws_words(a["plan"], 3, len(FENCED_LAYOUT), sums, len(a["toks"]))
            key = ("refusal ws", misalign)
            fence.scratch[key] = fence.alloc(key, (n + 2,), None, ws.device)
            body = fence.scratch[key].body
            a["ws"] = body[1:1 + n] if misalign else body[:n - 1]
            assert a["ws"].data_ptr() % 16 == (8 if misalign else 0)
            fence.refill()                                                          # from here on nothing may be written
            bodies = list(fence.last_outputs) + [b for b in fence.scratch.values() if b.body.data_ptr() not in fence.const_ptrs]
            kept.extend((b, b.flat.clone()) for b in bodies)

        fence.ws_hook = hook
        try:
            with pytest.raises(HipError, match=str(LF_ERR_ARG)):
                eng.lt_matmul_bsgs_batch(W, X[:2], keys)
        finally:
            fence.ws_hook = None
        assert kept and len(fence.last_outputs) == 2 * 3
        fence.check(fence.last_outputs)
        assert all(torch.equal(b.flat, c) for b, c in kept), (fill, misalign)
    got = [[w for o in tok for w in words(o)] for tok in eng.lt_matmul_bsgs_batch(W, X[:2], keys)]      # and it still works
    assert all(torch.equal(a, b) for g, w in zip(got, want[2]) for a, b in zip(g, w))


HOLD_MS = 50


def test_the_op_on_another_stream_waits_for_the_lanes_previous_op(lt_engine):
    """The stream contract (tests/test_stream_contract_gpu.py): cc_mult on s1 behind a hold, then lt_matmul_bsgs_batch on s2: it does
    not complete while the hold is on, its s2.wait_stream(s1) precedes its first backend call, and the words are right."""
    eng, keys = lt_engine
    evk = synth.key_switch_key(eng, 77)
    a, b = synth.ciphertext(eng, 50, 0), synth.ciphertext(eng, 51, 0)
    W = matrix(eng, 0, [[(0, 1, 2), (3,)], [(1, 2), (0,)]], n1=2)
    keys = keys_for(eng, (1, 2))
    X = tokens(eng, 0, 2, 3, seed=60)
    s1, s2 = independent_streams("cuda:0")
    with native_calls(eng) as seen:
        want = eng.lt_matmul_bsgs_batch(W, X, keys)                                 # (warms both ops)
    assert seen == [2]
    want_mult = eng.cc_mult(a, b, evk)
    torch.cuda.synchronize()
    # the ordering, with the hold
    t0 = time.perf_counter()
    ev = hold(s1, HOLD_MS)
    with torch.cuda.stream(s1):
        ra = eng.cc_mult(a, b, evk)
    with native_calls(eng) as seen, torch.cuda.stream(s2):
        rb = eng.lt_matmul_bsgs_batch(W, X, keys)
    done = torch.cuda.Event()
    done.record(s2)
    enqueue_ms = 1e3 * (time.perf_counter() - t0)
    while not done.query() and time.perf_counter() - t0 < HOLD_MS / 2e3:
        pass
    finished, held = done.query(), still_held(ev)
    assert held, f"inconclusive: the host took {enqueue_ms:.1f} ms to enqueue, the hold of {HOLD_MS} ms ran out before the check"
    assert not finished, "lt_matmul_bsgs_batch completed while the lane's previous op was held: it did not wait"
    torch.cuda.synchronize()
    assert seen == [2] and same(ra, want_mult) and all_same(rb, want)
    # the wait precedes the first backend call (no timing)
    with torch.cuda.stream(s1):
        eng.cc_mult(a, b, evk)
    with BackendSpy(eng.backend, also=[eng.ntt.ops]) as spy:
        with torch.cuda.stream(s2):
            rb = eng.lt_matmul_bsgs_batch(W, X, keys)
    waits = [i for i, x in enumerate(spy.log) if x == ("wait", s2.cuda_stream, s1.cuda_stream)]
    calls = [i for i, x in enumerate(spy.log) if x[0] == "call"]
    assert waits, f"no s2.wait_stream(s1) at all; log {spy.log[:6]}"
    assert ENTRY in spy.calls() and waits[0] < calls[0], f"{spy.log[calls[0]][1]} ran before the wait; log {spy.log[:waits[0] + 1]}"
    torch.cuda.synchronize()
    assert all_same(rb, want)


@pytest.mark.parametrize("last", [False, True], ids=["level0", "last"])
def test_one_token_through_the_batch_bindings_gives_the_single_bindings_words(last):
    """nt = 1 of the family's one body: ONE token through lt_matmul_batch_native and through lt_matmul_bsgs_batch_call against the
    single bindings lt_matmul_native and lt_matmul_bsgs_native, every word, on a fresh engine under tests.helpers.Fence with every
    bit set in scratch and outputs.  2 x 3: the 2 x 2 matrix with one None block beside an input no block uses; level 0 and the
    last level the ops take (the results still have ell = 2).  The engine's drivers send one token to the single bindings, so the
    batch bindings are reached through _lt_matmul_native here."""
    from liberate_fhe_amd.fhe import ckks_engine
    eng = ckks_engine(devices=["cuda:0"], **LT)
    fence = Fence(eng, FENCE_FILLS["ones"])
    real = getattr(eng.backend, ENTRY)
    setattr(eng.backend, ENTRY, fence._fenced_entry(ENTRY, real, inspect.signature(real)))
    level = eng.num_levels - 2 if last else 0
    d = eng._native_level(level)
    assert d is not None and eng._rows(d, level + 1, False) >= 2 and (not last or level + 2 == eng.num_levels)
    keys = keys_for(eng)
    cts = tokens(eng, level, 3, 1)[0]
    layouts = {"lt_matmul": ([[(0, 1, 3), None, None], [(2,), (0, 1), None]], eng.num_slots),
               "lt_matmul_bsgs": ([[(0, 1, 4, 6), None, None], [(5,), (0, 3, 8), None]], N1)}
    entries = {"lt_matmul": ("lt_matmul_native", "lt_matmul_batch_native"), "lt_matmul_bsgs": ("lt_matmul_bsgs_native", ENTRY)}
    for name, (layout, n1) in layouts.items():
        W = [[None if st is None else synth.diagonals(eng, 7 + 8 * o + i, level, st) if name == "lt_matmul" else
              synth.diagonals_bsgs(eng, 7 + 8 * o + i, level, st, n1) for i, st in enumerate(row)] for o, row in enumerate(layout)]
        steps = [[None if b is None else eng.diagonal_steps(b) for b in row] for row in W]
        got = {}
        for batch in (False, True):
            fence.refill()
            del fence.calls[:], fence.never_written[:]
            out = eng._lt_matmul_native(name, W, steps, n1, [cts], keys, level, d, batch=batch)
            fence.check()
            assert fence.calls == [entries[name][batch]], (name, batch, fence.calls)
            assert not fence.never_written, (name, batch, fence.never_written)
            assert len(out) == 1 and len(out[0]) == 2 and all(o.level == level + 1 for o in out[0])
            got[batch] = [w for o in out[0] for w in words(o)]
        assert all(torch.equal(a, b) for a, b in zip(got[False], got[True])), (name, level)


def test_block_matrix_times_three_token_vectors_with_real_keys():
    """logN 13, real keys: 2 x 2 blocks from random 8 x 8 block-diagonal matrices (15 diagonals, steps -7 .. 7, n1 = 4), three token
    vectors of two fresh ciphertexts.  The words are the loop's; the decryption error against the plain product is printed and held
    to the bound the project holds lt_matmul_bsgs to: at most 2 x the error of the loop of BSGS linear_transform + cc_add on the
    same ciphertexts, diagonals and keys (tests/test_lt_matmul_bsgs_cpu.matmul_bsgs_errors, per token)."""
    from liberate_fhe_amd.fhe import ckks_engine
    from tests.test_lt_matmul_cpu import block_diagonals
    eng = ckks_engine(devices=["cuda:0"], **LT)
    sk = eng.create_secret_key()
    pk = eng.create_public_key(sk)
    n, m = eng.num_slots, 8
    rng = np.random.default_rng(23)
    A = [[rng.uniform(-1, 1, (m, m)) for _ in range(2)] for _ in range(2)]
    W = [[eng.encode_diagonals(block_diagonals(A[o][i], n), 0, bsgs=N1) for i in range(2)] for o in range(2)]
    _, babies, giants = eng.lt_matmul_bsgs_steps(W)
    keys = [eng.create_rotation_key(sk, s) for s in sorted(set(babies + giants)) if s]
    assert giants == [0, 4, n - 8, n - 4] and len(keys) == 6
    ms = [[rng.uniform(-4, 4, n) + 1j * rng.uniform(-4, 4, n) for _ in range(2)] for _ in range(3)]
    X = [[eng.encorypt(v, pk) for v in tok] for tok in ms]
    with native_calls(eng) as seen:
        got = eng.lt_matmul_bsgs_batch(W, X, keys)
    assert seen == [2]
    assert all_same(got, [eng.lt_matmul_bsgs(W, cts, keys) for cts in X])
    for t, (g, cts, mt) in enumerate(zip(got, X, ms)):
        want = [sum((A[o][i] @ mt[i].reshape(-1, m).T).T.reshape(-1) for i in range(2)) for o in range(2)]
        loop = [eng.cc_add(eng.linear_transform(cts[0], W[o][0], keys), eng.linear_transform(cts[1], W[o][1], keys)) for o in range(2)]
        e_mat = max(np.abs(eng.decrode(a, sk) - w).max() for a, w in zip(g, want))
        e_loop = max(np.abs(eng.decrode(a, sk) - w).max() for a, w in zip(loop, want))
        print(f"logN 13, 2 x 2 blocks of 15 diagonals, n1 = 4, token {t}: max abs error lt_matmul_bsgs_batch {e_mat:.3e}, loop of BSGS "
              f"linear_transform + cc_add {e_loop:.3e}")
        assert e_mat <= 2 * e_loop, (t, e_mat, e_loop)
