"""cc_dot (ckks_engine.cc_dot, lf_cc_dot: a sum of ciphertext products under one relinearisation) without a GPU: the engine's
host logic on the checker backend against the composition of public steps that defines the words, the decryption error with
real keys against the chain of cc_mults, the refusals, the C entry's argument checks and the new kernels' resources."""
import ctypes
import os

import numpy as np
import pytest
import torch

from liberate_fhe_amd.utils import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOT = dict(logN=13, num_scales=5, num_special_primes=2, is_secured=False)   # two-pass ring, two digits


def words(ct):
    return [torch.cat([t.cpu() for t in comp]) for comp in ct.data]


def same(a, b):
    wa, wb = words(a), words(b)
    return a.level == b.level and a.origin == b.origin and len(wa) == len(wb) and all(torch.equal(x, y) for x, y in zip(wa, wb))


def lazy_ciphertext(eng, seed, level):
    """synth ciphertext with lazy words sprinkled in: + q on every other coefficient of c1, on every third of c0."""
    ct = synth.ciphertext(eng, seed, level)
    for comp, every in ((0, 3), (1, 2)):
        for i, d in enumerate(eng._loc(level)):
            q = torch.as_tensor(eng._consts(d, level, False).q_host).view(-1, 1).to(ct.data[comp][i].device)
            t = ct.data[comp][i].clone()
            t[:, ::every] += q
            ct.data[comp][i] = t
    return ct


def composition(eng, pairs, evk, relin=True):
    """The definition of the op's words, written out."""
    t = eng.cc_mult(pairs[0][0], pairs[0][1], evk, relin=False)
    for a, b in pairs[1:]:
        t = eng.cc_add_triplet(t, eng.cc_mult(a, b, evk, relin=False))
    return eng.relinearize(t, evk) if relin else t


def pairs_of(eng, k, level):
    """k pairs over four ciphertexts (two of them lazy): (a, b), (b, a), (a, a), then mixed ones; objects repeat."""
    a, b = lazy_ciphertext(eng, 50 + level, level), synth.ciphertext(eng, 51 + level, level)
    c, d = synth.ciphertext(eng, 52 + level, level), lazy_ciphertext(eng, 53 + level, level)
    return [(a, b), (b, a), (a, a), (c, d), (d, b)][:k]


@pytest.fixture(scope="module")
def checker():
    from liberate_fhe_amd.fhe import ckks_engine
    from tests.oracle_backend import OracleBackend
    return ckks_engine(devices=["cpu"], backend=OracleBackend(), **DOT)


def _evk(eng, seed=77):
    return synth.key_switch_key(eng, seed)


@pytest.mark.parametrize("level", [0, 2])
def test_cc_dot_equals_the_composition(checker, level):
    eng = checker
    evk = _evk(eng)
    from liberate_fhe_amd.fhe.presets import types
    for k in (1, 2, 3, 5):
        pairs = pairs_of(eng, k, level)
        got = eng.cc_dot(pairs, evk)
        want = composition(eng, pairs, evk)
        assert got.level == level + 1 and got.origin == types.origins["ct"] and not got.ntt_state and not got.include_special
        assert same(got, want), (level, k)
        # relin=False: the summed triplet itself; its relinearize is the relin=True result
        trip = eng.cc_dot(pairs, evk, relin=False)
        assert trip.origin == types.origins["ctt"] and trip.level == level + 1 and len(trip.data) == 3
        assert same(trip, composition(eng, pairs, evk, relin=False)), (level, k)
        assert same(eng.relinearize(trip, evk), got), (level, k)
    # one pair: cc_mult's words
    a, b = pairs_of(eng, 1, level)[0]
    assert same(eng.cc_dot([(a, b)], evk), eng.cc_mult(a, b, evk))
    assert same(eng.cc_dot([(a, a)], evk), eng.cc_mult(a, a, evk))
    # any iterable of pairs, lists as pairs
    assert same(eng.cc_dot(iter([[a, b], [b, a]]), evk), composition(eng, [(a, b), (b, a)], evk))


def test_real_keys_decrypt_within_twice_the_chain_of_cc_mults():
    """Real keys on the checker engine, four pairs of fixed random messages in [-1, 1]: cc_dot decrypts to sum m_a m_b with a
    maximum error of at most 2 x that of cc_add over four cc_mults of the same ciphertexts (the margin this project uses for
    such comparisons; the op adds the noise of ONE key switch where the chain adds four)."""
    from liberate_fhe_amd.fhe import ckks_engine
    from tests.oracle_backend import OracleBackend
    eng = ckks_engine(devices=["cpu"], backend=OracleBackend(), **DOT)
    sk = eng.create_secret_key()
    pk, evk = eng.create_public_key(sk), eng.create_evk(sk)
    rng = np.random.default_rng(11)
    n = eng.num_slots
    ms = [(rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)) for _ in range(4)]
    pairs = [(eng.encorypt(ma, pk), eng.encorypt(mb, pk)) for ma, mb in ms]
    want = sum(ma * mb for ma, mb in ms)
    got = eng.cc_dot(pairs, evk)
    assert got.level == 1
    chain = None
    for a, b in pairs:
        p = eng.cc_mult(a, b, evk)
        chain = p if chain is None else eng.cc_add(chain, p)
    e_dot = np.abs(eng.decrode(got, sk) - want).max()
    e_chain = np.abs(eng.decrode(chain, sk) - want).max()
    print(f"logN 13, k = 4, level 0: max abs error cc_dot {e_dot:.3e}, cc_add over four cc_mults {e_chain:.3e}, "
          f"largest entry {np.abs(want).max():.2f}")
    assert e_dot <= 2 * e_chain and e_chain < 1e-5


def test_refusals_come_before_any_work(checker, monkeypatch):
    """An empty list, an operand that is no ciphertext, mixed levels, a level with nothing left, operands in the NTT domain or
    with special rows: refused with cc_mult's error classes before a tensor is allocated or a step is called."""
    from liberate_fhe_amd.fhe.presets import errors
    eng = checker
    evk = _evk(eng)
    top = eng.num_levels - 1
    a0, b0, a1, atop = (synth.ciphertext(eng, 60 + i, lvl) for i, lvl in enumerate((0, 0, 1, top)))
    trip = eng.cc_mult(a0, b0, evk, relin=False)
    ntt = eng._new(a0.data, a0.origin, level=0, ntt_state=True)
    special = eng._new(a0.data, a0.origin, level=0, include_special=True)
    calls = []
    real_empty = torch.empty
    monkeypatch.setattr(torch, "empty", lambda *a, **k: (calls.append("empty"), real_empty(*a, **k))[1])
    for name in ("_ws", "cc_mult", "cc_add_triplet", "relinearize", "_op_plan", "_rescale_operands"):
        real = getattr(eng, name)
        monkeypatch.setattr(eng, name, lambda *a, _n=name, _r=real, **k: (calls.append(_n), _r(*a, **k))[1])
    cases = [
        (ValueError, []),
        (ValueError, [(a0,)]),
        (errors.NotMatchType, [(a0, b0), (a0, trip)]),
        (errors.NotMatchType, [(evk, b0)]),
        (errors.NotMatchType, [(a0, None)]),
        (errors.NotMatchDataStructState, [(a0, b0), (a1, a1)]),
        (errors.NotMatchDataStructState, [(a0, a1)]),
        (errors.MaximumLevelError, [(atop, atop)]),
        (errors.NotMatchDataStructState, [(a0, ntt)]),
        (errors.NotMatchDataStructState, [(special, b0)]),
    ]
    for relin in (True, False):
        for exc, pairs in cases:
            with pytest.raises(exc):
                eng.cc_dot(pairs, evk, relin=relin)
    assert calls == []
    monkeypatch.undo()
    assert eng.cc_dot([(a0, b0)], evk).level == 1                      # and the engine still works


_Q = np.array([(1 << 41) - 65535, (1 << 60) - 93, (1 << 60) - 173], dtype=np.int64)


def _fake_plan(logN, max_nct=1):
    from liberate_fhe_amd._native import KsPlan
    plan = KsPlan()
    plan.logN, plan.ell, plan.K, plan.nparts, plan.dig_nparts, plan.max_nct = logN, 2, 1, 2, 2, max_nct
    for name, typ in KsPlan._fields_:
        if typ is ctypes.c_void_p:
            setattr(plan, name, 64)
    plan.q_host = _Q.ctypes.data
    return plan


def test_c_entry_refuses_bad_arguments_before_any_launch():
    """lf_cc_dot returns LF_ERR_ARG from its arguments alone (pointers that are never dereferenced; no call here would pass the
    checks): what lf_cc_mult_evk refuses, np < 1, a NULL among the 4 np operand pointers, an unknown key format, a workspace
    missing or smaller than lf_cc_dot_ws_words says; and that function's value from the shapes."""
    from liberate_fhe_amd._native import lib
    LF_ERR_ARG = 10001
    dummy = ctypes.c_void_p(64)

    def ptrs(n, null_at=None):
        arr = (ctypes.c_void_p * max(n, 1))(*([64] * max(n, 1)))
        if null_at is not None:
            arr[null_at] = None
        return arr

    def call(plan, np_=2, ins=None, row0s=None, ksk=dummy, fmt=0, ws=dummy, ws_words=1 << 40, out0=dummy, out1=dummy, ps=0, cs=0):
        ins = ptrs(4 * np_) if ins is None else ins
        row0s = ptrs(4 * np_) if row0s is None else row0s
        return lib.lf_cc_dot(ctypes.byref(plan) if plan is not None else None, np_, ins, row0s, ksk, ps, cs, 0, fmt, ws, ws_words,
                             out0, out1, None)

    from liberate_fhe_amd._native import KsPlan
    zero = KsPlan()
    assert lib.lf_cc_dot_ws_words(ctypes.byref(zero)) == 0
    assert lib.lf_cc_dot_ws_words(None) == 0
    assert call(zero) == LF_ERR_ARG
    assert call(None) == LF_ERR_ARG
    for logN in (12, 18):                                              # outside the key switch's ring degrees
        plan = _fake_plan(logN)
        assert lib.lf_cc_dot_ws_words(ctypes.byref(plan)) == 0
        assert call(plan) == LF_ERR_ARG, logN
    for max_nct in (1, 2, 4):
        plan = _fake_plan(13, max_nct)
        need = lib.lf_cc_dot_ws_words(ctypes.byref(plan))
        assert need == 3 * 2 * (1 << 13)                               # the summed triplet [3][ell][N]
        assert call(plan, ws_words=need - 1) == LF_ERR_ARG
        assert call(plan, ws=None) == LF_ERR_ARG
        assert call(plan, np_=0) == LF_ERR_ARG
        assert call(plan, np_=-1) == LF_ERR_ARG
        assert call(plan, ins=None, row0s=None, ksk=None) == LF_ERR_ARG
        assert call(plan, out0=None) == LF_ERR_ARG
        assert call(plan, out1=None) == LF_ERR_ARG
        assert call(plan, fmt=2) == LF_ERR_ARG
        assert call(plan, fmt=1, ksk=ctypes.c_void_p(72)) == LF_ERR_ARG   # a planes key must be 16-byte aligned
        assert call(plan, fmt=1, ps=1) == LF_ERR_ARG
        for np_ in (1, 3, 9):
            for at in (0, 4 * np_ - 1, 2 * np_):
                assert call(plan, np_=np_, ins=ptrs(4 * np_, at)) == LF_ERR_ARG
                assert call(plan, np_=np_, row0s=ptrs(4 * np_, at)) == LF_ERR_ARG
        assert lib.lf_cc_dot(ctypes.byref(plan), 1, None, ptrs(4), dummy, 0, 0, 0, 0, dummy, 1 << 40, dummy, dummy, None) == LF_ERR_ARG
        assert lib.lf_cc_dot(ctypes.byref(plan), 1, ptrs(4), None, dummy, 0, 0, 0, 0, dummy, 1 << 40, dummy, dummy, None) == LF_ERR_ARG
        for field in ("rescale_scales", "PR", "x4", "d2", "state", "ext", "sum", "md_ws", "psi_dp", "Ed"):   # what lf_cc_mult_evk refuses
            broken = _fake_plan(13, max_nct)
            setattr(broken, field, None)
            assert lib.lf_cc_dot_ws_words(ctypes.byref(broken)) == 0, field
            assert call(broken) == LF_ERR_ARG, field
    bad = _fake_plan(13)
    bad.max_nct = 0
    assert call(bad) == LF_ERR_ARG and lib.lf_cc_dot_ws_words(ctypes.byref(bad)) == 0


def test_cc_dot_kernels_use_no_scratch():
    """dot_tensor_kernel<1 | 2 | 4> and the pre-summed fold ks_inner2_presum_kernel<raw / planes key, raw / planes digits> exist
    under their own names with scratch 0 and no spill; the streaming tensor kernel keeps at least 4 waves per SIMD, the new fold
    form the occupancy of ks_inner2_kernel<1, fold> with the same key and digit formats; the tracked table lists them as built."""
    import __graft_entry__ as g
    res = {r["kernel"]: r for r in g.kernel_resources()}
    want = {f"dot_tensor_kernel<{n}>": 4 for n in (1, 2, 4)}
    want.update({f"ks_inner2_presum_kernel<{pl}, {dpl}>": res[f"ks_inner2_kernel<1, true, {pl}, {dpl}>"]["occupancy"]
                 for pl in ("true", "false") for dpl in ("true", "false")})
    new = sorted(k for k in res if k.startswith(("dot_tensor_kernel<", "ks_inner2_presum_kernel<")))
    assert new == sorted(want)
    tracked = open(os.path.join(ROOT, "profiles", "r06_kernel_resources.txt")).read()
    for k, floor in want.items():
        r = res[k]
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, r
        assert r["occupancy"] >= floor, (r, floor)
        line = next(ln for ln in tracked.splitlines() if ln[18:76].strip() == k)
        f = line.split()
        assert (int(f[-7]), int(f[-3]), int(f[-1])) == (r["vgprs"], r["scratch"], r["occupancy"]), line
