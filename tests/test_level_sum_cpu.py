"""level_sum / level_sum_batch / level_up_batch (liberate_fhe_amd/fhe/levelsum.py, lf_level_sum) without a GPU: the engine's host
logic on the checker backend against the composition of public ops that defines the words and against a big-integer evaluation
of the residues; every refusal; the splitting at the caps and what the engine hands the native entry (through a stub that
evaluates the kernel's arithmetic in Python integers); the C entry's argument checks; poly_eval's glue against its docstring."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from liberate_fhe_amd.fhe import encdec
from liberate_fhe_amd.utils import synth
from tests.test_inner_sum_cpu import lazy_ciphertext
from tests.test_poly_eval_cpu import poly_composition

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LT = dict(logN=13, num_scales=5, num_special_primes=2, is_secured=False)
POLY = dict(logN=13, num_scales=8, num_special_primes=2, is_secured=False)   # 9 levels: degree 15 on an interval needs 6
R = 1 << 62
BIG, NEG = (1 << 69) + 12345, -((1 << 69) + 54321)      # 70-bit weights


def words(ct):
    return [torch.cat([t.cpu() for t in comp]) for comp in ct.data]


def same(a, b):
    wa, wb = words(a), words(b)
    return a.level == b.level and a.origin == b.origin and len(wa) == len(wb) and all(torch.equal(x, y) for x, y in zip(wa, wb))


def composition(eng, terms, const=None, level=None):
    """The definition of level_sum's words, written out."""
    L = max(ct.level for ct, _ in terms) if level is None else level
    acc = None
    for ct, s in terms:
        u = ct if ct.level == L else eng.level_up(ct, L)
        v = u if s == 1 else eng.mult_int_scalar(u, s)
        acc = v if acc is None else eng.cc_add(acc, v)
    return acc if const is None else eng.add_scalar(acc, const)


@pytest.fixture(scope="module")
def checker():
    from liberate_fhe_amd.fhe import ckks_engine
    from tests.oracle_backend import OracleBackend
    return ckks_engine(devices=["cpu"], backend=OracleBackend(), **LT)


@pytest.fixture(scope="module")
def pool(checker):
    """ciphertexts of every level, lazy words in each: pool[level][i]"""
    return {l: [lazy_ciphertext(checker, 100 + 10 * l + i, l) for i in range(3)] for l in range(checker.num_levels)}


def cases(eng, pool):
    top = eng.num_levels - 1
    a0, b0, c0 = pool[0]
    return [
        ([(a0, 1)], None, 1),                                        # level_up itself
        ([(a0, 1)], None, top),                                      # .. to the last level
        ([(a0, 2)], -1.0, None),                                     # the Chebyshev square: no level change
        ([(pool[2][0], 2), (a0, -1)], None, None),                   # the Chebyshev product
        ([(pool[3][0], 1), (pool[1][1], 1)], None, None),            # the closing addition
        ([(a0, 1), (pool[1][0], -1), (pool[2][0], BIG), (pool[3][0], NEG)], 0.75, None),     # a residual sum over three levels
        ([(a0, 3), (a0, -5), (b0, 1)], -2.5, 3),                     # the same ciphertext twice, all levelled
        ([(pool[top][0], 1), (pool[top][1], 1)], None, None),        # nothing levelled, weights 1: cc_add
        ([(pool[top - 1][0], 7), (c0, 1)], 1.0, top),
    ]


def test_level_sum_equals_the_composition(checker, pool):
    from liberate_fhe_amd.fhe.presets import types
    eng = checker
    for terms, const, level in cases(eng, pool):
        got = eng.level_sum(terms, const=const, level=level)
        want = composition(eng, terms, const, level)
        assert got.origin == types.origins["ct"] and not got.ntt_state and not got.include_special
        assert same(got, want), ([(ct.level, s) for ct, s in terms], const, level)
    assert same(eng.level_up(pool[0][0], 2), eng.level_sum([(pool[0][0], 1)], level=2))


def test_batches_equal_the_loops_in_order(checker, pool):
    eng = checker
    sets = [(t, c) for t, c, l in cases(eng, pool) if l is None]
    got = eng.level_sum_batch(sets + sets[:1])
    want = [composition(eng, t, c) for t, c in sets + sets[:1]]
    assert len(got) == len(want) and all(same(a, b) for a, b in zip(got, want))
    top = eng.num_levels - 1
    got = eng.level_sum_batch(iter(sets[:2]), level=top)
    assert all(same(a, composition(eng, t, c, top)) for a, (t, c) in zip(got, sets[:2]))
    cts = [pool[0][0], pool[2][1], pool[0][0], pool[1][2]]
    got = eng.level_up_batch(cts, 3)
    assert len(got) == 4 and all(same(a, eng.level_up(ct, 3)) for a, ct in zip(got, cts))
    assert eng.level_sum_batch([]) == [] and eng.level_up_batch([], 2) == []


def big_integer_sum(eng, terms, const, L):
    """canonical residue of sum_t s_t u_t (+ the add_scalar integer on coefficient 0 of c0) from Python integers: u_t = x_t, or
    delta * y with y = (x - z) / q_l + [z > q_l / 2] (mod q) on the words x of the surviving row and z of the dropped row"""
    q = eng.ctx.q
    primes = list(eng.ntt.p.destination_arrays[L][0])
    out = []
    for comp in range(2):
        acc = [np.zeros(eng.ctx.N, dtype=object) for _ in primes]
        for ct, s in terms:
            l = ct.level
            x = ct.data[comp][0].numpy().astype(object)
            assert list(eng.ntt.p.destination_arrays[l][0][L - l:]) == primes
            for r, i in enumerate(primes):
                if l == L:
                    u = x[r]
                else:
                    ql = q[eng.ntt.p.destination_arrays[l][0][0]]
                    delta = round(eng.scale * (eng.deviations[L] / np.sqrt(eng.deviations[l + 1])))
                    z = x[0]
                    u = ((x[L - l + r] - z) * pow(ql, -1, q[i]) + (z > ql // 2)) * delta
                acc[r] = acc[r] + u * s
        if comp == 0 and const is not None:
            for r in range(len(primes)):
                acc[r][0] += eng._add_scalar_int(const, L)
        out.append(torch.tensor(np.array([[int(v) % q[i] for v in acc[r]] for r, i in enumerate(primes)], dtype=np.int64)))
    return out


def test_words_are_the_residues_of_the_big_integer_sum(checker, pool):
    eng = checker
    terms = [(pool[0][0], 1), (pool[1][0], -1), (pool[3][1], BIG), (pool[0][2], NEG), (pool[3][2], 1)]
    got = eng.level_sum(terms, const=-1.25)
    want = big_integer_sum(eng, terms, -1.25, 3)
    assert got.level == 3 and all(torch.equal(a, b) for a, b in zip(words(got), want))
    got = eng.level_up(pool[1][1], eng.num_levels - 1)
    assert all(torch.equal(a, b) for a, b in zip(words(got), big_integer_sum(eng, [(pool[1][1], 1)], None, eng.num_levels - 1)))


def test_refusals(checker, pool, monkeypatch):
    from liberate_fhe_amd.fhe.presets import errors
    eng = checker
    top = eng.num_levels - 1
    a0, b0, _ = pool[0]
    a2 = pool[2][0]
    evk = synth.key_switch_key(eng, 77)
    trip = eng.cc_mult(a0, b0, evk, relin=False)
    ntt = eng._new(a0.data, a0.origin, level=0, ntt_state=True)
    mont = eng._new(a0.data, a0.origin, level=0, montgomery_state=True)
    special = eng._new(a0.data, a0.origin, level=0, include_special=True)
    calls = []
    for name in ("level_up", "mult_int_scalar", "cc_add", "add_scalar", "rescale", "clone"):
        real = getattr(eng, name)
        monkeypatch.setattr(eng, name, lambda *a, _n=name, _r=real, **k: (calls.append(_n), _r(*a, **k))[1])
    bad = [
        (ValueError, [], None, None),                                  # no term
        (ValueError, [(a0, 1)], None, None),                           # a copy
        (ValueError, [(a0, 1)], 0.5, None),                            # .. add_scalar
        (ValueError, [(a0, 1)], None, 0),
        (ValueError, [(a0, 2), (b0, 0)], None, None),                  # a zero weight
        (ValueError, [(a0, 1), (a2, 1)], None, 1),                     # a term deeper than L
        (ValueError, [(a0, 1), (a2, 1)], None, top + 1),               # L beyond the last level
        (ValueError, [a0, b0], None, None),                            # not pairs
        (errors.NotMatchType, [(a0, 1), (trip, 1)], None, None),
        (errors.NotMatchType, [(a0, 1), (None, 1)], None, None),
        (errors.NotMatchType, [(a0, 1), (evk, 1)], None, None),
        (errors.NotMatchDataStructState, [(a2, 1), (ntt, 1)], None, None),
        (errors.NotMatchDataStructState, [(a2, 1), (mont, 1)], None, None),
        (errors.NotMatchDataStructState, [(a2, 1), (special, 1)], None, None),
        (TypeError, [(a0, 1), (a2, 0.5)], None, None),                 # float weights: weighted_sums is the op with a rescale
    ]
    good = ([(a0, 1), (b0, 2)], None)                                   # (fine at every level there is)
    for exc, terms, const, level in bad:
        with pytest.raises(exc):
            eng.level_sum(terms, const=const, level=level)
        result = None
        with pytest.raises(exc):                                      # a batch is refused as a whole: the bad member sits last
            result = eng.level_sum_batch([good, good, (terms, const)], level=level)
        assert result is None
    for exc, cts, level in [(ValueError, [a0, a2], 2), (ValueError, [a0, pool[3][0]], 2), (ValueError, [a0, b0], top + 1),
                            (errors.NotMatchType, [a0, trip], 2), (errors.NotMatchType, [a0, None], 2),
                            (errors.NotMatchDataStructState, [a0, ntt], 2)]:
        result = None
        with pytest.raises(exc):
            result = eng.level_up_batch(cts, level)
        assert result is None
    with pytest.raises(ValueError):
        eng.level_sum_batch([good, a0])
    assert calls == []


# ---- what the engine hands the native entry -------------------------------------------------------------------------------------
def mm62s(a, b, q, k):
    """csrc/ckks_common.h mm62s on Python integers (object arrays): the representative, not only the residue"""
    x = a * b
    xl = x & (R - 1)
    s = (xl * k) & (R - 1)
    return (x >> 62) + (((s << 2) * q) >> 64) + (xl != 0)


class StubNative:
    """A backend with level_sum_call: everything else is the checker backend's.  The call evaluates level_sum_kernel's arithmetic
    (csrc/ckks_fused.hip) in Python integers on exactly what the engine passed, so the tables, the skipped rows, the rescale
    constants and the rounding thresholds are held to the composition without a GPU; `calls` lists the sets of every call."""
    native_ops = True
    lsum_max_terms = 8
    lsum_max_sets = 8

    def __init__(self, inner, evaluate=True):
        self._inner, self.calls, self.evaluate = inner, [], evaluate

    def __getattr__(self, name):
        return getattr(self._inner, name)

    def level_sum_call(self, sets, outs, rows, logN, c):
        assert 1 <= len(sets) <= self.lsum_max_sets and len(outs) == len(sets)
        self.calls.append([len(terms) for terms, _, _ in sets])
        N = 1 << logN
        qs = [int(v) for v in c.q_host]
        assert len(qs) == rows
        for (terms, tab, cst), pair in zip(sets, outs):
            assert 1 <= len(terms) <= self.lsum_max_terms and tuple(tab.shape) == (len(terms), rows)
            assert all(tuple(o.shape) == (rows, N) and o.is_contiguous() for o in pair) and (cst is None or tuple(cst.shape) == (rows,))
            if not self.evaluate:
                for o in pair:
                    o.fill_(1000 * len(self.calls))
                continue
            for comp in range(2):
                for r, q in enumerate(qs):
                    k, r2inv = (-pow(q, -1, R)) % R, pow(R, -2, q)
                    acc = np.zeros(N, dtype=object)
                    for t, (c0, c1, skip, scales, round_at) in enumerate(terms):
                        x = (c0, c1)[comp]
                        assert x.size(0) == rows + skip and (skip == 0) == (scales is None)
                        w = x[skip + r].numpy().astype(object)
                        if skip:
                            assert scales.numel() == rows + skip - 1
                            z = x[0].numpy().astype(object)
                            w = mm62s(w - z, int(scales[skip - 1 + r]), q, k) + (z > round_at)
                            w = np.where(w < q, w, w - q)
                        w = np.where(w < 0, w + q, w)
                        acc = acc + w * int(tab[t, r])
                    v = acc * r2inv % q
                    if cst is not None and comp == 0:
                        v[0] = (v[0] + int(cst[r])) % q
                    pair[comp][r] = torch.tensor(v.astype(np.int64))


def stubbed(eng, monkeypatch, evaluate=True):
    stub = StubNative(eng.backend, evaluate)
    monkeypatch.setattr(eng, "backend", stub)
    monkeypatch.setattr(eng, "_native_level", lambda lvl: 0)
    return stub


def test_the_native_arguments_give_the_compositions_words(checker, pool, monkeypatch):
    eng = checker
    picked = [cases(eng, pool)[i] for i in (1, 3, 5, 6)]
    want = [composition(eng, t, c, l) for t, c, l in picked]
    up_want = eng.level_up(pool[1][0], 3)
    stub = stubbed(eng, monkeypatch)
    got = [eng.level_sum(t, const=c, level=l) for t, c, l in picked]
    up = eng.level_up(pool[1][0], 3)                    # level_up itself takes the native path: one term, weight 1
    monkeypatch.undo()
    assert stub.calls == [[1], [2], [4], [3], [1]]
    assert all(same(a, b) for a, b in zip(got, want)) and same(up, up_want)


def noncontiguous(ct):
    data = [list(comp) for comp in ct.data]
    for comp in range(2):
        t = data[comp][0]
        wide = torch.zeros((t.shape[0], 2 * t.shape[1]), dtype=t.dtype)
        wide[:, ::2] = t
        data[comp][0] = wide[:, ::2]
        assert not data[comp][0].is_contiguous()
    return ct._replace(data=data)


def test_splitting_at_the_caps(checker, pool, monkeypatch):
    from liberate_fhe_amd import _native
    eng = checker
    a0, a1, a2 = pool[0][0], pool[1][0], pool[2][0]
    long_terms = [((a0, a1)[i % 2], i + 2) for i in range(_native.LF_LSUM_MAX_TERMS + 1)]
    want_long = composition(eng, long_terms, None, 2)
    want_odd = composition(eng, [(a0, 3), (a2, 1)])
    stub = stubbed(eng, monkeypatch)
    # one term too many: the composition (whose level_ups are single native calls), word for word
    got = eng.level_sum(long_terms, level=2)
    assert all(c == [1] for c in stub.calls) and len(stub.calls) == len(long_terms)
    del stub.calls[:]
    stub.evaluate = False                                           # from here on the stub only marks its outputs
    # exactly the cap: one call
    eng.level_sum(long_terms[:-1], level=2)
    assert stub.calls == [[_native.LF_LSUM_MAX_TERMS]]
    del stub.calls[:]
    # a batch longer than the cap: several calls, every output at its set's index; two target levels: one call per level
    S = _native.LF_LSUM_MAX_SETS
    sets = [([(a0, 1), (a1, -1)], None)] * (2 * S + 3)
    outs = eng.level_sum_batch(sets)
    assert stub.calls == [[2] * S, [2] * S, [2] * 3]
    assert [int(o.data[0][0][0, 0]) for o in outs] == [1000] * S + [2000] * S + [3000] * 3 and all(o.level == 1 for o in outs)
    del stub.calls[:]
    mixed = [([(a0, 1)], None), ([(a0, 2), (a2, 1)], 0.5), ([(a1, 1)], None), ([(a1, 5), (a2, -1)], None)]
    outs = eng.level_sum_batch([(t, c) for t, c in mixed[1::2]] + [([(a0, 1), (a1, 1)], None)])
    assert stub.calls == [[2, 2], [2]] and [o.level for o in outs] == [2, 2, 1]
    del stub.calls[:]
    outs = eng.level_up_batch([a0, a1, a0], 2)
    assert stub.calls == [[1, 1, 1]] and all(o.level == 2 for o in outs)
    del stub.calls[:]
    # a non-contiguous operand: that set takes the composition (its level_up of a contiguous copy is a call of one term), the
    # others keep the call
    stub.evaluate = True
    outs = eng.level_sum_batch([([(a0, 3), (a2, 1)], None), ([(noncontiguous(a0), 3), (a2, 1)], None)])
    assert stub.calls == [[1], [2]]
    monkeypatch.undo()
    assert same(got, want_long) and same(outs[0], want_odd) and same(outs[1], want_odd)


def test_a_checker_engine_and_a_large_prime_take_the_composition(checker, pool, monkeypatch):
    eng = checker
    terms = [(pool[0][0], 2), (pool[1][0], -1)]
    want = composition(eng, terms)
    assert eng._level_sum_device(terms, 1) is None                  # no level_sum_call on the checker backend
    stub = stubbed(eng, monkeypatch, evaluate=False)
    assert eng._level_sum_device(terms, 1) == 0
    monkeypatch.setattr(eng, "level_sum_native", False)             # the switch the measuring tool uses
    assert same(eng.level_sum(terms), want) and stub.calls == []
    monkeypatch.setattr(eng, "level_sum_native", True)
    q = list(eng.ctx.q)
    monkeypatch.setattr(eng.ctx, "q", q[:-1] + [q[-1] | (1 << 60)])
    assert eng._level_sum_device(terms, 1) is None


# ---- the ABI side ----------------------------------------------------------------------------------------------------------------
def test_the_entry_is_exported_bound_and_capped_as_the_header_says():
    from liberate_fhe_amd import _native
    from liberate_fhe_amd.fhe.backend import HipBackend
    so = ctypes.CDLL(_native.LIB_PATH)
    assert hasattr(so, "lf_level_sum") and "lf_level_sum" in _native._SIGNATURES and len(_native._SIGNATURES["lf_level_sum"]) == 17
    header = open(os.path.join(ROOT, "include", "ckks_hip.h")).read()
    caps = dict(re.findall(r"#define (LF_LSUM_MAX_\w+) (\d+)", header))
    assert caps == {"LF_LSUM_MAX_TERMS": str(_native.LF_LSUM_MAX_TERMS), "LF_LSUM_MAX_SETS": str(_native.LF_LSUM_MAX_SETS)}
    assert (HipBackend.lsum_max_terms, HipBackend.lsum_max_sets) == (_native.LF_LSUM_MAX_TERMS, _native.LF_LSUM_MAX_SETS)
    assert _native.LF_LSUM_MAX_TERMS >= 8
    assert not HipBackend.level_sum_call.__name__.endswith("_native")
    assert _native.lib.lf_abi_version() == 15


def test_the_entry_refuses_bad_arguments_before_any_device_call():
    """lf_level_sum returns LF_ERR_ARG from its arguments alone: dummy pointers that are never dereferenced (no call here is one
    that would pass the check)."""
    from liberate_fhe_amd import _native
    lib, E = _native.lib, _native.LF_ERR_ARG
    T, S = _native.LF_LSUM_MAX_TERMS, _native.LF_LSUM_MAX_SETS
    d = ctypes.c_void_p(64)

    def call(nsets=1, k=(2,), rows=3, logN=13, ins=None, row0s=None, scales=None, tab=None, outs=None, drop=()):
        n = max(sum(min(max(v, 0), T) for v in k), 1)
        ks = (ctypes.c_int64 * max(len(k), 1))(*k)
        arr = lambda count, given: (ctypes.c_void_p * count)(*([64] * count if given is None else given))
        args = dict(k=ks, ins=arr(2 * n, ins), row0=arr(2 * n, row0s), scales=arr(n, scales), round_at=(ctypes.c_int64 * n)(),
                    tab=arr(max(len(k), 1), tab), consts=None, out=arr(2 * max(len(k), 1), outs), ql=d, qh=d, kl=d, kh=d)
        for name in drop:
            args[name] = None
        return lib.lf_level_sum(nsets, args["k"], args["ins"], args["row0"], args["scales"], args["round_at"], args["tab"],
                                args["consts"], args["out"], rows, logN, args["ql"], args["qh"], args["kl"], args["kh"], 0, None)

    assert call(nsets=0, k=()) == E and call(nsets=S + 1, k=(1,) * (S + 1)) == E and call(nsets=-1) == E      # sets outside the cap
    assert call(k=(0,)) == E and call(k=(T + 1,)) == E and call(nsets=2, k=(1, T + 1)) == E                    # terms outside the cap
    for logN in (12, 18, 24, 0):
        assert call(logN=logN) == E
    assert call(rows=-1) == E and call(rows=lib.lf_limits(2) + 1) == E
    for name in ("k", "ins", "row0", "scales", "round_at", "tab", "out", "ql", "qh", "kl", "kh"):
        assert call(drop=(name,)) == E, name
    assert call(ins=[64, 64, 64, None]) == E and call(ins=[None, 64, 64, 64]) == E
    assert call(tab=[None]) == E and call(outs=[64, None]) == E and call(outs=[None, 64]) == E
    assert call(nsets=2, k=(1, 1), tab=[64, None]) == E
    # a dropped row without its rescale constants, and the reverse; one component's dropped row alone
    assert call(row0s=[64, 64, None, None], scales=[64, 64]) == E
    assert call(row0s=[64, 64, 64, 64], scales=[64, None]) == E
    assert call(row0s=[64, None, 64, 64], scales=[64, 64]) == E
    assert call(row0s=[None, None, None, 64], scales=[None, None]) == E


def test_the_new_kernel_uses_no_scratch_and_is_in_the_tracked_table():
    import __graft_entry__ as g
    rows = [r for r in g.kernel_resources() if r["kernel"].startswith("level_sum_kernel<")]
    assert sorted(r["kernel"] for r in rows) == [f"level_sum_kernel<{k}>" for k in (1, 2, 4, 8)]
    assert all(r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["lds"] == 0 and r["occupancy"] >= 4 for r in rows), rows
    tracked = {}
    for ln in open(os.path.join(ROOT, "profiles", "r06_kernel_resources.txt")):
        f = ln.split()
        if len(f) > 8 and f[1].startswith("level_sum_kernel<"):
            tracked[f[1]] = (int(f[-7]), int(f[-3]), int(f[-1]))
    assert tracked == {r["kernel"]: (r["vgprs"], r["scratch"], r["occupancy"]) for r in rows}


# ---- poly_eval's glue --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def poly_checker():
    from liberate_fhe_amd.fhe import ckks_engine
    from tests.oracle_backend import OracleBackend
    return ckks_engine(devices=["cpu"], backend=OracleBackend(), **POLY)


@pytest.mark.parametrize("basis,degree,interval", [("power", 7, None), ("chebyshev", 15, (-4, 4))])
def test_poly_eval_and_its_batch_equal_the_docstring_composition(poly_checker, basis, degree, interval):
    eng = poly_checker
    evk = synth.key_switch_key(eng, 77)
    coeffs = np.random.default_rng(degree).uniform(-1, 1, degree + 1)
    cts = [synth.ciphertext(eng, 60 + degree + i, 1) for i in range(2)]
    split = encdec.poly_split(degree)
    want = [poly_composition(eng, ct, coeffs, evk, basis, interval, split) for ct in cts]
    seen = []
    real = {n: getattr(eng, n) for n in ("level_sum_batch", "level_up_batch")}
    try:
        for n, f in real.items():
            setattr(eng, n, lambda *a, _n=n, _f=f, **k: (seen.append(_n), _f(*a, **k))[1])
        got = eng.poly_eval(cts[0], coeffs, evk, basis=basis, interval=interval)
        assert "level_sum_batch" in seen and "level_up_batch" in seen       # the glue goes through the new path
        batch = eng.poly_eval_batch(cts, coeffs, evk, basis=basis, interval=interval)
    finally:
        for n in real:
            delattr(eng, n)
    assert same(got, want[0])
    assert len(batch) == 2 and all(same(a, b) for a, b in zip(batch, want))
