"""level_sum / level_sum_batch / level_up_batch on the GPU: lf_level_sum (level_sum_kernel<1 | 2 | 4 | 8>, one launch for a group
of sets) against the composition that defines its words, evaluated by the checker engine on copies of the operands; on worst-case
words; at the presets against the GPU's own element-wise chain; level_up and poly_eval through the new glue; the outputs between
guards under hostile fills; and on a second stream behind a held cc_mult.  Every comparison is torch.equal."""
import time
import warnings

import numpy as np
import pytest
import torch

from liberate_fhe_amd.utils import synth
from tests import helpers
from tests.helpers import BackendSpy, Fence, FENCE_FILLS, edge_ciphertext, hold, independent_streams, still_held
from tests.test_fenced_ops_gpu import assert_same, flat_words, mirror

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore", category=UserWarning)

DEV = "cuda:0"
LT = dict(logN=13, num_scales=5, num_special_primes=2, is_secured=False)     # the smallest ring with the native path; both prime classes
POLY = dict(LT, num_scales=8)                                                # 9 levels: a degree-7 Chebyshev series on an interval
BIG, NEG = (1 << 69) + 12345, -((1 << 69) + 54321)                           # 70-bit weights
HOLD_MS = 50
_ENG = {}


def engines(name="LT"):
    """(HIP engine, checker engine) of a parameter set, built once per process and kept"""
    if name not in _ENG:
        from liberate_fhe_amd.fhe import ckks_engine
        from tests.oracle_backend import OracleBackend
        params = POLY if name == "POLY" else LT
        _ENG[name] = (ckks_engine(devices=[DEV], **params), ckks_engine(devices=["cpu"], backend=OracleBackend(), **params))
    return _ENG[name]


def lazy(eng, ct, dev=0):
    """+ q on every third coefficient of c0 and every other one of c1: lazy words below 2q"""
    q = torch.as_tensor(eng._consts(dev, ct.level, False).q_host).view(-1, 1).to(ct.data[0][0].device)
    out = []
    for comp, every in ((0, 3), (1, 2)):
        t = ct.data[comp][0].clone()
        t[:, ::every] += q
        out.append([t])
    return ct._replace(data=tuple(out))


def pools(name="LT"):
    """{level: 3 ciphertexts with lazy words} on the GPU, and the checker's copies of the same objects"""
    key = ("pool", name)
    if key not in _ENG:
        H, _ = engines(name)
        g = {l: [lazy(H, synth.ciphertext(H, 100 + 10 * l + i, l)) for i in range(3)] for l in range(H.num_levels)}
        _ENG[key] = (g, {l: [mirror(ct, "cpu") for ct in cts] for l, cts in g.items()})
    return _ENG[key]


def composition(eng, terms, const=None, level=None):
    """The definition of level_sum's words, written out."""
    L = max(ct.level for ct, _ in terms) if level is None else level
    acc = None
    for ct, s in terms:
        u = ct if ct.level == L else eng.level_up(ct, L)
        v = u if s == 1 else eng.mult_int_scalar(u, s)
        acc = v if acc is None else eng.cc_add(acc, v)
    return acc if const is None else eng.add_scalar(acc, const)


class Spy:
    """counts the sets (as term counts) of every level_sum_call: a silent fall-back to the composition shows"""

    def __init__(self, eng):
        self.eng, self.calls, self.real = eng, [], eng.backend.level_sum_call

    def __enter__(self):
        def spied(sets, outs, rows, logN, c):
            self.calls.append([len(terms) for terms, _, _ in sets])
            return self.real(sets, outs, rows, logN, c)
        self.eng.backend.level_sum_call = spied
        return self

    def __exit__(self, *exc):
        del self.eng.backend.level_sum_call


def spec_cases(num_levels):
    """(terms as (level, index in the pool, weight), const, level): L - l = 1, 3 and up to the last level; k = 1, 2, 3 and the cap;
    every weight class (1, -1, 2, 70 bits of either sign); consts of both signs; levelled and same-level terms mixed; a ciphertext
    twice in a set"""
    top = num_levels - 1
    return [
        ([(0, 0, 1)], None, 1),                                              # level_up, L - l = 1
        ([(0, 1, 1)], None, 3),                                              # L - l = 3
        ([(0, 2, 1)], None, top),                                            # to the last level
        ([(top - 1, 0, -1)], 0.5, top),
        ([(1, 0, 2)], -1.0, None),                                           # the Chebyshev square: nothing levelled
        ([(2, 0, 2), (0, 0, -1)], None, None),                               # the Chebyshev product
        ([(3, 0, 1), (1, 1, 1)], None, None),                                # the closing addition
        ([(top, 0, 1), (top, 1, 1)], 1.5, None),                             # cc_add + add_scalar at the last level
        ([(0, 0, BIG), (1, 0, NEG), (3, 1, 1)], -0.25, None),                # k = 3 over three levels, 70-bit weights
        ([(0, 0, 3), (0, 0, -5), (2, 1, 1)], None, 3),                       # the same ciphertext twice, all levelled
        ([(0, 0, 1), (1, 0, -1), (2, 0, 2), (3, 0, BIG), (0, 1, NEG), (1, 1, 1), (3, 1, -1), (3, 2, 2)], 2.0, None),   # the cap
        ([(l % num_levels, i % 3, (-1) ** i * (i + 1)) for i, l in enumerate(range(8))], -3.0, top),                  # the cap, at the last level
    ]


def build(pool, spec):
    return [(pool[l][i], s) for l, i, s in spec]


def test_native_equals_the_composition_on_the_checker():
    H, C = engines()
    g, c = pools()
    assert H._native_level(0) is not None and H._native_level(H.num_levels - 1) is not None
    for spec, const, level in spec_cases(H.num_levels):
        with Spy(H) as spy:
            got = H.level_sum(build(g, spec), const=const, level=level)
        assert spy.calls == [[len(spec)]], (spec, spy.calls)                   # ONE native call
        want = composition(C, build(c, spec), const, level)
        assert got.level == want.level and not got.ntt_state and not got.include_special
        assert_same(flat_words(got), flat_words(want), f"level_sum {spec} const {const} level {level}")
    # level_up itself: one term of weight 1
    with Spy(H) as spy:
        up = H.level_up(g[1][2], 4)
    assert spy.calls == [[1]]
    assert_same(flat_words(up), flat_words(C.level_up(c[1][2], 4)), "level_up")
    # one term too many for a call: the composition, whose level_ups are single calls
    long_spec = [(i % 2, i % 3, i + 2) for i in range(H.backend.lsum_max_terms + 1)]
    with Spy(H) as spy:
        got = H.level_sum(build(g, long_spec), level=2)
    assert spy.calls == [[1]] * len(long_spec)
    assert_same(flat_words(got), flat_words(composition(C, build(c, long_spec), None, 2)), "nine terms")


@pytest.mark.parametrize("nsets", [1, 2, 3, "cap", "cap+1"])
def test_batches_with_mixed_target_levels(nsets):
    H, C = engines()
    g, c = pools()
    S = H.backend.lsum_max_sets
    n = {"cap": S, "cap+1": S + 1}.get(nsets, nsets)
    specs = [s for s in spec_cases(H.num_levels) if s[2] is None]
    picked = [specs[i % len(specs)] for i in range(n)]                        # target levels 1, 2, 3, top, 3: mixed
    with Spy(H) as spy:
        got = H.level_sum_batch([(build(g, spec), const) for spec, const, _ in picked])
    assert sorted(k for call in spy.calls for k in call) == sorted(len(spec) for spec, _, _ in picked)     # every set went native
    levels = [max(l for l, _, _ in spec) for spec, _, _ in picked]
    assert len(spy.calls) == sum(-(-levels.count(L) // S) for L in set(levels))    # one call per target level and S sets
    want = [composition(C, build(c, spec), const) for spec, const, _ in picked]
    assert [o.level for o in got] == levels
    assert_same(flat_words(got), flat_words(want), f"level_sum_batch of {n}")
    # one target level for all: calls of S sets
    with Spy(H) as spy:
        ups = H.level_up_batch([g[i % 3][i % 2] for i in range(n)], 3)
    assert spy.calls == [[1] * min(S, n - i) for i in range(0, n, S)]
    assert_same(flat_words(ups), flat_words([C.level_up(c[i % 3][i % 2], 3) for i in range(n)]), f"level_up_batch of {n}")


def worst(eng, level, pattern, seed=0):
    """edge_ciphertext with q added to every word: "top" puts every word at 2q - 1, "mixed" alternates rows and coefficients
    between 2q - 1, q, q + 1 and the seam of the balanced representation"""
    ct = edge_ciphertext(eng, level, pattern, seed)
    q = torch.as_tensor(eng._consts(0, level, False).q_host).view(-1, 1).to(ct.data[0][0].device)
    return ct._replace(data=tuple([t + q for t in comp] for comp in ct.data))


@pytest.mark.parametrize("pattern", ["top", "mixed", "top|0"])
def test_worst_case_words_with_the_maximal_term_count(pattern):
    """The range argument next to level_sum_kernel: 8 terms of words at 2q - 1 (the dropped rows included), weights whose
    residues are q - 1 on every row: -1, and the product of the target level's primes minus one."""
    H, C = engines()
    top = H.num_levels - 1
    for L in (2, top):
        Q = 1
        for i in H.ntt.p.destination_arrays[L][0]:
            Q *= H.ctx.q[i]
        levels = [l % (L + 1) for l in range(H.backend.lsum_max_terms)]      # levelled and same-level terms
        weights = [-1 if t % 2 else Q - 1 for t in range(len(levels))]
        g = [worst(H, l, pattern, seed=t) for t, l in enumerate(levels)]
        c = [mirror(ct, "cpu") for ct in g]
        for const in (None, -1.0):
            with Spy(H) as spy:
                got = H.level_sum(list(zip(g, weights)), const=const, level=L)
            assert spy.calls == [[len(levels)]]
            want = composition(C, list(zip(c, weights)), const, L)
            assert_same(flat_words(got), flat_words(want), f"{pattern} level {L} const {const}")


def strided(ct):
    views = []
    for comp in range(2):
        t = ct.data[comp][0]
        wide = torch.zeros((t.size(0), 2 * t.size(1)), dtype=torch.int64, device=t.device)
        wide[:, ::2] = t
        views.append([wide[:, ::2]])
    out = ct._replace(data=tuple(views))
    assert not out.data[0][0].is_contiguous() and torch.equal(out.data[1][0], ct.data[1][0])
    return out


def test_noncontiguous_operands_take_the_composition():
    H, C = engines()
    g, c = pools()
    for spec, const in (([(0, 0, 3), (2, 1, 1)], None), ([(2, 0, 2), (0, 1, -1)], 0.5), ([(1, 0, 1)], None)):
        level = 2
        terms = build(g, spec)
        odd = [(strided(terms[0][0]), terms[0][1])] + terms[1:]
        with Spy(H) as spy:
            got = H.level_sum(odd, const=const, level=level)
        assert all(call == [1] for call in spy.calls), spy.calls               # at most the composition's own level_up
        assert_same(flat_words(got), flat_words(composition(C, build(c, spec), const, level)), f"strided {spec}")
        assert_same(flat_words(got), flat_words(H.level_sum(terms, const=const, level=level)), f"strided against contiguous {spec}")


@pytest.mark.parametrize("preset", ["silver", "gold"])
def test_presets_three_terms_across_two_levels(preset):
    """native against the GPU's own element-wise chain (the switch the measuring tool uses)"""
    from liberate_fhe_amd.fhe import ckks_engine, presets
    H = ckks_engine(devices=[DEV], **{k: v for k, v in presets.params[preset].items() if k != "devices"})
    _ENG[preset] = H                                     # (engines of this file live as long as the process)
    terms = [(lazy(H, synth.ciphertext(H, 7, 0)), BIG), (lazy(H, synth.ciphertext(H, 8, 2)), -1), (synth.ciphertext(H, 9, 0), 1)]
    with Spy(H) as spy:
        got = H.level_sum(terms, const=-0.5)
        up = H.level_up(terms[0][0], 2)
    assert spy.calls == [[3], [1]]
    H.level_sum_native = False
    with Spy(H) as spy:
        want = composition(H, terms, -0.5)
        want_up = H.level_up(terms[0][0], 2)
    assert spy.calls == []
    assert_same(flat_words(got), flat_words(want), preset)
    assert_same(flat_words(up), flat_words(want_up), f"{preset} level_up")


@pytest.mark.parametrize("basis,degree,interval", [("power", 7, None), ("chebyshev", 7, (-4, 4))])
def test_poly_eval_and_its_batch_equal_the_checkers(basis, degree, interval):
    H, C = engines("POLY")
    coeffs = np.random.default_rng(degree).uniform(-1, 1, degree + 1)
    got, want = [], []
    for eng, out in ((H, got), (C, want)):
        evk = synth.key_switch_key(eng, 77)
        cts = [synth.ciphertext(eng, 60 + i, 1) for i in range(2)]
        if eng is H:
            with Spy(H) as spy:
                out.append(eng.poly_eval(cts[0], coeffs, evk, basis=basis, interval=interval))
                out.append(eng.poly_eval_batch(cts, coeffs, evk, basis=basis, interval=interval))
            assert spy.calls, "poly_eval's glue did not reach level_sum_call"
        else:
            out.append(eng.poly_eval(cts[0], coeffs, evk, basis=basis, interval=interval))
            out.append(eng.poly_eval_batch(cts, coeffs, evk, basis=basis, interval=interval))
    assert_same(flat_words(got), flat_words(want), f"poly_eval {basis} {degree}")


def test_outputs_between_guards_under_hostile_fills(monkeypatch):
    from liberate_fhe_amd.fhe import ckks_engine
    H, C = engines()
    g, c = pools()
    monkeypatch.setattr(helpers, "NATIVE_ENTRIES", helpers.NATIVE_ENTRIES + ("level_sum_call",))     # for this fence alone
    F = ckks_engine(devices=[DEV], **LT)
    fence = Fence(F, FENCE_FILLS["ones"])
    picked = [spec_cases(H.num_levels)[i] for i in (2, 5, 8, 10)]
    want = [composition(C, build(c, spec), const, level) for spec, const, level in picked]
    batch_want = [C.level_up(ct, 3) for ct in c[0] + c[1]]
    for fill_name, fill in FENCE_FILLS.items():
        fence.fill = fill
        for (spec, const, level), w in zip(picked, want):
            fence.refill()
            del fence.calls[:], fence.never_written[:]
            got = F.level_sum(build(g, spec), const=const, level=level)
            fence.check()
            assert fence.calls == ["level_sum_call"] and not fence.never_written, (fill_name, spec, fence.calls, fence.never_written)
            assert_same(flat_words(got), flat_words(w), f"fenced {spec} fill {fill_name}")
        del fence.calls[:], fence.never_written[:]
        got = F.level_up_batch(g[0] + g[1], 3)
        fence.check()
        assert fence.calls == ["level_sum_call"] and not fence.never_written
        assert_same(flat_words(got), flat_words(batch_want), f"fenced level_up_batch fill {fill_name}")


def test_level_sum_on_a_second_stream_waits_for_a_held_cc_mult():
    """tests/test_stream_contract_gpu.py, sections A and B, for level_sum: behind cc_mult on s1 it waits before its first backend
    call; with s1 held it has not completed half a hold later; the words are those of the idle run."""
    H, _ = engines()
    g, _ = pools()
    evk = synth.key_switch_key(H, 77)
    a, b = synth.ciphertext(H, 50, 0), synth.ciphertext(H, 51, 0)
    terms = [(g[2][0], 2), (g[0][0], -1)]
    s1, s2 = independent_streams(DEV)
    want = [t.clone() for t in flat_words(H.level_sum(terms, const=-1.0))]
    want_mult = [t.clone() for t in flat_words(H.cc_mult(a, b, evk))]
    torch.cuda.synchronize()
    # B: the wait comes first
    with torch.cuda.stream(s1):
        H.cc_mult(a, b, evk)
    with BackendSpy(H.backend, also=[H.ntt.ops]) as spy:
        with torch.cuda.stream(s2):
            r = H.level_sum(terms, const=-1.0)
    waits = [i for i, x in enumerate(spy.log) if x == ("wait", s2.cuda_stream, s1.cuda_stream)]
    calls = [i for i, x in enumerate(spy.log) if x[0] == "call"]
    assert waits and calls == [i for i in calls if i > waits[0]] and spy.calls() == ["level_sum_call"], spy.log
    torch.cuda.synchronize()
    assert_same(flat_words(r), want, "level_sum behind cc_mult")
    # A: held
    t0 = time.perf_counter()
    ev = hold(s1, HOLD_MS)
    with torch.cuda.stream(s1):
        ra = H.cc_mult(a, b, evk)
    with torch.cuda.stream(s2):
        rb = H.level_sum(terms, const=-1.0)
    done = torch.cuda.Event()
    done.record(s2)
    while not done.query() and time.perf_counter() - t0 < HOLD_MS / 2e3:
        pass
    finished, held = done.query(), still_held(ev)
    assert held, f"inconclusive: the hold of {HOLD_MS} ms ran out {1e3 * (time.perf_counter() - t0):.1f} ms after it began"
    assert not finished, "level_sum completed while cc_mult's stream was held: it did not wait"
    torch.cuda.synchronize()
    assert_same(flat_words(ra), want_mult, "cc_mult (held)")
    assert_same(flat_words(rb), want, "level_sum (behind it)")
