"""Slot sums (ckks_engine.rotate_sum / inner_sum / inner_sum_steps, encdec.inner_sum_plan, lf_rotate_sum) without a GPU: the
engine's host logic on the checker backend against the composition of public steps that defines the words, the fold of the
addend against rotate_hoisted, the mixed-radix plan, the refusals, the C entry's argument checks and the new kernel's
resources."""
import ctypes
import itertools
import os

import numpy as np
import pytest
import torch

from liberate_fhe_amd.fhe import encdec
from liberate_fhe_amd.utils import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LT = dict(logN=13, num_scales=5, num_special_primes=2, is_secured=False)   # two-pass ring, two digits
STEPS = (1, 2, 5, 11, 3, 700, 9)


def words(ct):
    return [torch.cat([t.cpu() for t in comp]) for comp in ct.data]


def same(a, b):
    return a.level == b.level and all(torch.equal(x, y) for x, y in zip(words(a), words(b)))


def keys_for(eng, steps=STEPS):
    keys = {s: synth.key_switch_key(eng, 40 + i, origin=f"rotation key:{s}") for i, s in enumerate(steps)}
    keys[0] = synth.key_switch_key(eng, 60, origin="rotation key:0")
    keys["conj"] = synth.key_switch_key(eng, 61, origin="conjugation key")
    return keys


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


def exponent_of(eng, key):
    if key.origin == "conjugation key":
        return encdec.conjugation_exponent(eng.ctx.N)
    return encdec.galois_exponent(eng.ctx.N, int(key.origin.split(":")[-1]))


def composition(eng, ct, keys, include_self):
    """The definition of the op's words from the engine's public steps on one device: c0, c1 canonical; E = per part
    pre_extend(c1) -> extend -> exact forward NTT; c^ = enter_ntt(c) * P on the ordinary rows; per key the parts of E gathered by
    pi_p times the key part, summed, + c^0 gathered on the ordinary rows; the self term c^, zero on the special rows; S_c = the
    sum of all of them; intt_exit_reduce, mod-down without addend.  (tests/test_linear_transform_cpu.py's composition with the
    diagonal product and the rescale removed.)"""
    d, N, logN, level = 0, eng.ctx.N, eng.ctx.logN, ct.level
    ell, K = eng._rows(d, level, False), eng.ntt.num_special_primes
    _2q = eng._vec("_2q", d, level, False)
    c = []
    for comp in range(2):
        x = torch.empty_like(ct.data[comp][0])
        eng.backend.galois(ct.data[comp][0].contiguous(), x, ell, logN, 1, _2q)
        c.append(x)
    E = []
    for part_id in range(len(eng.ntt.p.p[level][d])):
        state = eng.pre_extend([c[1]], d, level, part_id)
        ext = eng.extend(state, d, level, part_id, d)
        eng.ntt.ntt([ext], level, d, -2)
        E.append(ext)
    chat = []
    for comp in range(2):
        x = c[comp].clone()
        eng.ntt.enter_ntt([x], level, d, -1)
        eng.ntt.mont_enter_scalar([x], [eng._PR(d, level)], level, d, -1)
        chat.append(x)
    start = eng.ntt.starts[level][d]
    terms = []
    if include_self:
        terms.append([torch.cat([chat[comp], torch.zeros((K, N), dtype=torch.int64)]) for comp in range(2)])
    for key in keys:
        idx = torch.from_numpy(encdec.ntt_galois_index(logN, exponent_of(eng, key)))
        t = None
        for part_id, ext in enumerate(E):
            g = ext[:, idx].contiguous()
            part = key.data[eng.parts_alloc[level][d][part_id]].data
            prod = [eng.ntt.mont_mult([g], [part[comp][0][start:]], level, d, -2)[0] for comp in range(2)]
            t = prod if t is None else [eng.ntt.mont_add([t[comp]], [prod[comp]], level, d, -2)[0] for comp in range(2)]
        folded = eng.ntt.mont_add([t[0][:ell].contiguous()], [chat[0][:, idx].contiguous()], level, d, -1)[0]
        t[0] = torch.cat([folded, t[0][ell:]])
        terms.append(t)
    S = [None, None]
    for t in terms:
        for comp in range(2):
            S[comp] = t[comp] if S[comp] is None else eng.ntt.mont_add([S[comp]], [t[comp]], level, d, -2)[0]
    s = torch.stack(S).contiguous()
    eng.ntt.intt_exit_reduce([s[0]], level, d, -2)
    eng.ntt.intt_exit_reduce([s[1]], level, d, -2)
    out = torch.empty((2, ell, N), dtype=torch.int64)
    tabs = eng._ks_tables(level)
    eng.backend.ks_moddown_batch([s[0], s[1]], [out[0], out[1]], [None, None], ell, K, tabs[("pir", d)],
                                 eng._vec("Rs", d, level, True), eng._consts(d, level, True), PiP=None, galois=None)
    return eng._new(([out[0]], [out[1]]), ct.origin, level=level)


@pytest.fixture(scope="module")
def checker():
    from liberate_fhe_amd.fhe import ckks_engine
    from tests.oracle_backend import OracleBackend
    eng = ckks_engine(devices=["cpu"], backend=OracleBackend(), **LT)
    return eng, keys_for(eng)


def key_sets(keys):
    """1, 2, 4, 5 and 7 keys; a repeated key; a step-0 key; a conjugation key (alone and among rotations)."""
    sets = [[keys[s] for s in STEPS[:n]] for n in (1, 2, 4, 5, 7)]
    return sets + [[keys[1], keys[5], keys[1]], [keys[0]], [keys[2], keys[0]], [keys["conj"]], [keys[1], keys["conj"], keys[2]]]


@pytest.mark.parametrize("level", [0, 2, "top"])
def test_checker_rotate_sum_equals_the_composition(checker, level):
    eng, keys = checker
    level = eng.num_levels - 1 if level == "top" else level
    ct = lazy_ciphertext(eng, 90 + level, level)
    for ks, with_self in itertools.product(key_sets(keys), (True, False)):
        got = eng.rotate_sum(ct, ks, include_self=with_self)
        want = composition(eng, ct, ks, with_self)
        assert got.level == level and got.origin == ct.origin and not got.ntt_state and not got.include_special
        gw, ww = words(got), words(want)
        assert gw[0].shape == ww[0].shape == words(ct)[0].shape
        assert torch.equal(gw[0], ww[0]) and torch.equal(gw[1], ww[1]), (level, [k.origin for k in ks], with_self)
    # the self term alone
    got, want = eng.rotate_sum(ct, [], include_self=True), composition(eng, ct, [], True)
    assert same(got, want)


@pytest.mark.parametrize("level", [0, 2])
def test_one_key_without_self_is_rotate_hoisted(checker, level):
    """moddown(s) + d = moddown(s + P d): the same residues mod q, row by row.  rotate_sum's words are canonical whatever the
    input (its c0 passes through the mod-down); rotate_hoisted adds c0(X^p) behind the mod-down and its word keeps the lazy
    representative a lazy input word brings along, so on lazy inputs only the residues agree.  On canonical
    inputs the words are equal."""
    eng, keys = checker
    q = torch.as_tensor(eng._consts(0, level, False).q_host).view(-1, 1)
    for make, exact in ((lazy_ciphertext, False), (synth.ciphertext, True)):
        ct = make(eng, 33 + level, level)
        for s in (1, 700, 0):
            a = words(eng.rotate_sum(ct, [keys[s]], include_self=False))
            b = words(eng.rotate_hoisted(ct, [keys[s]])[0])
            for x, y in zip(a, b):
                assert int(x.min()) >= 0 and bool((x < q).all()), (level, s)
                assert torch.equal(x, y % q), (level, s)
                if exact:
                    assert torch.equal(x, y), (level, s)


@pytest.mark.parametrize("radix", [2, 4, 8])
@pytest.mark.parametrize("n", [1, 2, 8, 12, 16, 7, 64, 4096])
def test_inner_sum_plan(n, radix):
    num_slots = 1 << 14
    for stride in (1, -1, 3, num_slots // n):
        if n * abs(stride) > num_slots:
            continue
        plan = encdec.inner_sum_plan(n, stride, num_slots, radix)
        assert int(np.prod([r for r, _ in plan], dtype=np.int64)) == n
        if n == 1:
            assert plan == []
        unit, sums = 1, [0]
        for r, steps in plan:
            assert 2 <= r <= max(radix, 7) and len(steps) == r - 1
            assert tuple(steps) == tuple((j * stride * unit) % num_slots for j in range(1, r))
            sums = [a + j * stride * unit for a in sums for j in range(r)]
            unit *= r
        assert sorted(sums) == sorted(j * stride for j in range(n))          # every j * stride exactly once
        # stages are as large as the radix allows, largest first
        if n in (8, 16, 64, 4096):
            assert [r for r, _ in plan][0] == radix
    if n == 12:
        assert [r for r, _ in encdec.inner_sum_plan(12, 1, num_slots, 4)] == [4, 3]
    if n == 7:
        assert [r for r, _ in encdec.inner_sum_plan(7, 1, num_slots, radix)] == [7]


def test_inner_sum_plan_refusals():
    S = 1 << 12
    for bad in (dict(n=0), dict(n=-4), dict(radix=1), dict(radix=0), dict(n=67), dict(n=2 * 71), dict(n=S + 1),
                dict(n=16, stride=S // 16 + 1), dict(n=16, stride=-(S // 16 + 1)), dict(n=2.5)):
        args = dict(n=8, stride=1, radix=4)
        args.update(bad)
        with pytest.raises(ValueError):
            encdec.inner_sum_plan(args["n"], args["stride"], S, args["radix"])
    assert [r for r, _ in encdec.inner_sum_plan(61, 1, S, 4)] == [61]       # the largest prime stage one hoisted set takes
    assert [r for r, _ in encdec.inner_sum_plan(64, 1, S, 64)] == [64]
    assert encdec.inner_sum_plan(S, 1, S, 4)[-1][1][-1] == 3 * S // 4
    assert encdec.inner_sum_plan(16, -S // 16, S, 4)[0][1] == tuple((-j * (S // 16)) % S for j in (1, 2, 3))


def chain(eng, ct, n, keys, stride, radix):
    for _, steps in encdec.inner_sum_plan(n, stride, eng.num_slots, radix):
        ct = eng.rotate_sum(ct, [keys[s] for s in steps], include_self=True)
    return ct


def test_inner_sum_equals_the_chain_of_its_plan(checker):
    eng, _ = checker
    ct = synth.ciphertext(eng, 17, 1)
    S = eng.num_slots
    for n, stride, radix in ((12, 1, 4), (8, -1, 4), (6, S // 8, 2), (1, 1, 4)):
        steps = eng.inner_sum_steps(n, stride, radix)
        assert steps == sorted({s for _, st in encdec.inner_sum_plan(n, stride, S, radix) for s in st})
        keys = {s: synth.key_switch_key(eng, 70 + i, origin=f"rotation key:{s}") for i, s in enumerate(steps)}
        got = eng.inner_sum(ct, n, keys, stride=stride, radix=radix)
        assert got.level == ct.level and same(got, chain(eng, ct, n, keys, stride, radix)), (n, stride, radix)
        assert same(got, eng.inner_sum(ct, n, list(keys.values())[::-1], stride=stride, radix=radix))     # a list, any order
    assert eng.inner_sum_steps(16) == eng.inner_sum_steps(16, 1, encdec.INNER_SUM_RADIX) == [1, 2, 3, 4, 8, 12]


def test_radix_2_4_8_give_three_word_sets_at_logN_12():
    """logN 12 (the unfused orchestration): n = 8 as 2 * 2 * 2, 4 * 2 and 8 — three different sets of words (each radix sums
    other key-switch noises), each equal to the chain of its own plan."""
    from liberate_fhe_amd.fhe import ckks_engine
    from tests.oracle_backend import OracleBackend
    eng = ckks_engine(devices=["cpu"], backend=OracleBackend(), logN=12, num_scales=5, num_special_primes=2, is_secured=False)
    ct = synth.ciphertext(eng, 4, 0)
    keys = {s: synth.key_switch_key(eng, 80 + s, origin=f"rotation key:{s}") for s in range(1, 8)}
    outs = []
    for radix in (2, 4, 8):
        got = eng.inner_sum(ct, 8, keys, radix=radix)
        assert same(got, chain(eng, ct, 8, keys, 1, radix)), radix
        outs.append(got)
    assert not same(outs[0], outs[1]) and not same(outs[1], outs[2]) and not same(outs[0], outs[2])


def test_refusals(checker):
    from liberate_fhe_amd.fhe.presets import errors
    eng, keys = checker
    ct = synth.ciphertext(eng, 95, 0)
    with pytest.raises(errors.NotMatchType) as e:                  # a missing key, named by its step
        eng.inner_sum(ct, 16, [keys[1], keys[2], keys[3]])
    assert "4" in str(e.value)
    with pytest.raises(errors.NotMatchType):                       # a key of another kind
        eng.inner_sum(ct, 2, [keys[1], synth.key_switch_key(eng, 8)])
    with pytest.raises(errors.NotMatchType):
        eng.rotate_sum(ct, [keys[1], synth.key_switch_key(eng, 8)])
    with pytest.raises(errors.NotMatchType):                       # inner_sum looks keys up by step: no conjugation there
        eng.inner_sum(ct, 2, [keys[1], keys["conj"]])
    with pytest.raises(errors.NotMatchType):                       # not a ciphertext
        eng.rotate_sum(keys[1], [keys[1]])
    with pytest.raises(errors.NotMatchType):
        eng.inner_sum(keys[1], 2, keys)
    for kw in (dict(ntt_state=True), dict(include_special=True)):
        bad = eng._new(ct.data, ct.origin, level=0, **kw)
        with pytest.raises(NotImplementedError):
            eng.rotate_sum(bad, [keys[1]])
        with pytest.raises(NotImplementedError):
            eng.inner_sum(bad, 2, [keys[1]])
    with pytest.raises(ValueError):                                # nothing to sum
        eng.rotate_sum(ct, [], include_self=False)
    with pytest.raises(ValueError):
        eng.inner_sum(ct, 0, keys)
    with pytest.raises(ValueError):
        eng.inner_sum(ct, 2 * eng.num_slots, keys)


_Q = np.array([(1 << 41) - 65535, (1 << 60) - 93, (1 << 60) - 173], dtype=np.int64)


def _fake_plan(logN, x4=True):
    from liberate_fhe_amd._native import KsPlan
    plan = KsPlan()
    plan.logN, plan.ell, plan.K, plan.nparts, plan.dig_nparts, plan.max_nct = logN, 2, 1, 2, 2, 1
    for name, typ in KsPlan._fields_:
        if typ is ctypes.c_void_p:
            setattr(plan, name, 64)
    plan.q_host = _Q.ctypes.data
    if not x4:
        plan.x4 = None
    return plan


def test_c_entry_refuses_bad_arguments_before_any_launch():
    """lf_rotate_sum returns LF_ERR_ARG from its arguments alone (pointers that are never dereferenced; no call here would pass
    the checks): nr < 0, nr == 0 without with_self, a NULL key / output / input / exponent array, an even exponent or one outside
    (0, 2N), a key format out of range, a plan without PR, a workspace smaller than lf_rotate_sum_ws_words says, plans at logN
    12 and 18, a NULL plan."""
    from liberate_fhe_amd._native import lib
    LF_ERR_ARG = 10001
    dummy = ctypes.c_void_p(64)
    arr = (ctypes.c_void_p * 4)(64, 64, 64, 64)

    def call(plan, nr, exps, keys=arr, with_self=0, ws=None, ws_words=0, out0=dummy, out1=dummy, c0=dummy, c1=dummy, fmt=0):
        e = (ctypes.c_int64 * max(1, len(exps)))(*exps) if exps is not None else None
        return lib.lf_rotate_sum(ctypes.byref(plan) if plan is not None else None, c0, c1, nr, e, keys, 0, 0, 0, fmt, with_self,
                                 ws, ws_words, out0, out1, None)

    for logN in (12, 18):
        plan = _fake_plan(logN)
        assert lib.lf_rotate_sum_ws_words(ctypes.byref(plan)) == 0
        assert call(plan, 1, [3]) == LF_ERR_ARG, logN
    assert call(None, 1, [3]) == LF_ERR_ARG
    plan = _fake_plan(13)
    N2 = 2 << 13
    assert lib.lf_rotate_sum_ws_words(ctypes.byref(plan)) == 0               # the plan's operand stack serves
    assert call(plan, -1, [3]) == LF_ERR_ARG
    assert call(plan, -1, [3], with_self=1) == LF_ERR_ARG
    assert call(plan, 0, [3]) == LF_ERR_ARG                                   # no key and no self term
    assert call(plan, 1, None) == LF_ERR_ARG
    assert call(plan, 1, [3], keys=None) == LF_ERR_ARG
    assert call(plan, 1, [3], out0=None) == LF_ERR_ARG
    assert call(plan, 1, [3], out1=None) == LF_ERR_ARG
    assert call(plan, 1, [3], c0=None) == LF_ERR_ARG
    assert call(plan, 1, [3], c1=None) == LF_ERR_ARG
    assert call(plan, 1, [3], fmt=7) == LF_ERR_ARG
    assert call(plan, 2, [3, 4]) == LF_ERR_ARG                                # even exponent
    assert call(plan, 1, [N2 + 1]) == LF_ERR_ARG                              # >= 2N
    assert call(plan, 1, [0]) == LF_ERR_ARG
    assert call(plan, 1, [-3]) == LF_ERR_ARG
    nul = (ctypes.c_void_p * 4)(64, None, 64, 64)
    assert call(plan, 2, [3, 5], keys=nul) == LF_ERR_ARG                      # a NULL key
    odd = (ctypes.c_void_p * 4)(72, 64, 64, 64)
    assert call(plan, 1, [3], keys=odd, fmt=1) == LF_ERR_ARG                  # a planes key off its 16-byte alignment
    nopr = _fake_plan(13)
    nopr.PR = None
    assert call(nopr, 1, [3]) == LF_ERR_ARG
    assert call(nopr, 0, [3], with_self=1) == LF_ERR_ARG
    # without an operand stack in the plan: an explicit workspace of 2 ell N words
    bare = _fake_plan(13, x4=False)
    need = lib.lf_rotate_sum_ws_words(ctypes.byref(bare))
    assert need == 2 * 2 << 13
    assert call(bare, 1, [3]) == LF_ERR_ARG
    assert call(bare, 1, [3], ws=dummy, ws_words=need - 1) == LF_ERR_ARG
    assert call(bare, 0, [3], with_self=1, ws=dummy, ws_words=need - 1) == LF_ERR_ARG


def test_rotate_sum_kernels_use_no_scratch():
    """Every instantiation of ks_inner_rsum_kernel (1, 2, 4 keys x raw / planes key x raw / planes digits, and the keyless one
    of a lone self term) exists with scratch 0, no spill and at least 3 waves per SIMD; the tracked table lists them as built."""
    import __graft_entry__ as g
    by = {r["kernel"]: r for r in g.kernel_resources() if r["kernel"].startswith("ks_inner_rsum_kernel<")}
    want = [f"ks_inner_rsum_kernel<{nr}, {pl}, {dpl}>" for nr in (1, 2, 4) for pl in ("true", "false") for dpl in ("true", "false")]
    want.append("ks_inner_rsum_kernel<0, false, false>")
    assert sorted(by) == sorted(want)
    for k in want:
        assert by[k]["scratch"] == 0 and by[k]["vgpr_spill"] == 0, by[k]
        assert by[k]["occupancy"] >= 3, by[k]
    tracked = open(os.path.join(ROOT, "profiles", "r06_kernel_resources.txt")).read()
    for k, r in by.items():
        line = next(ln for ln in tracked.splitlines() if ln[18:76].strip() == k)
        f = line.split()
        assert (int(f[-7]), int(f[-3]), int(f[-1])) == (r["vgprs"], r["scratch"], r["occupancy"]), line
