"""Baby-step / giant-step linear transforms (encode_diagonals(.., bsgs=n1), ckks_engine.linear_transform on what it returns,
lf_linear_transform_bsgs, encdec.bsgs_split) without a GPU: the split of the steps, the engine's host logic on the checker backend
against the composition of public steps that defines the words, the flat form's words where there is one giant step, the
refusals and round trips, the decryption error against the flat form with real keys, the sharded ranks, the C entry's argument
checks and the new kernels' resources."""
import ctypes
import os
import sys
import tempfile
import warnings

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from liberate_fhe_amd.fhe import encdec
from liberate_fhe_amd.utils import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LT = dict(logN=13, num_scales=5, num_special_primes=2, is_secured=False)   # two-pass ring, two digits
n = 1 << 12                                                                # num_slots at logN 13

# (n1, steps): what each case covers
CASES = [
    (4, (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 700, n - 6, n - 1)),   # baby 0 and giant 0 present, a wrapped step, 3 baby keys
    (4, (1, 2, 5, 7)),                                                # baby 0 absent
    (4, (4, 5, 9, 700)),                                              # giant 0 absent
    (4, (9, 10)),                                                     # one giant step only (g = 8), baby 0 absent
    (1, (0, 1, 5)),                                                   # n1 = 1: every step a giant step, the only baby step 0
    (8, (1, 2, 3, 4, 5, 9)),                                          # 5 baby keys (a group of 4 + 1)
    (8, (0, 1, 2, 3, 4, 5, 6, 7, 8, 17, 18)),                         # 7 baby keys (4 + 2 + 1); giant 8 holds a single diagonal
    (16, (3, n - 1)),                                                 # a wrapped step in giant step n - 16
]
ALL_STEPS = sorted({s for _, steps in CASES for s in steps} | {s for n1, steps in CASES for part in encdec.bsgs_split(steps, n, n1)[1:] for s in part})


def words(ct):
    return [torch.cat([t.cpu() for t in comp]) for comp in ct.data]


def keys_for(eng, steps):
    return {s: synth.key_switch_key(eng, 40 + i, origin=f"rotation key:{s}") for i, s in enumerate(steps) if s}


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


def bsgs_composition(eng, ct, diags, keys):
    """The definition of the op's words from the engine's public steps on one device, reading the encoded object: c0, c1
    canonical; E = per part pre_extend(c1) -> extend -> exact forward NTT; c^ = P enter_ntt(c) on the ordinary rows; per baby step
    b != 0 u^b_c = sum over the parts of (E gathered by pi_b) x key b's part, u^b_0 += c^0 gathered on the ordinary rows (b = 0:
    u^0 = c^, zero on the special rows); per giant step S^g_c = sum_b pt_{g,b} * u^b_c; g != 0: w = mod-down of
    intt_exit_reduce(S^g_1), canonical, E^g its digits, v_c = sum over the parts of (E^g gathered by pi_g) x key g's part,
    v_0 += S^g_0 gathered on all rows; A = S^0 + sum v; intt_exit_reduce, mod-down without addend, the engine's rescale."""
    d, N, logN, level = 0, eng.ctx.N, eng.ctx.logN, ct.level
    ell, K = eng._rows(d, level, False), eng.ntt.num_special_primes
    _2q, tabs, start = eng._vec("_2q", d, level, False), eng._ks_tables(level), eng.ntt.starts[level][d]
    n1, babies, giants = eng.bsgs_steps(diags)

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

    c = [canonical(ct.data[comp][0]) for comp in range(2)]
    E = digits(c[1])
    chat = []
    for comp in range(2):
        x = c[comp].clone()
        eng.ntt.enter_ntt([x], level, d, -1)
        eng.ntt.mont_enter_scalar([x], [eng._PR(d, level)], level, d, -1)
        chat.append(x)
    u = {}
    for b in babies:
        if b == 0:
            u[b] = [torch.cat([chat[comp], torch.zeros((K, N), dtype=torch.int64)]) for comp in range(2)]
        else:
            idx = index(b)
            t = inner(E, idx, keys[b])
            folded = eng.ntt.mont_add([t[0][:ell].contiguous()], [chat[0][:, idx].contiguous()], level, d, -1)[0]
            t[0] = torch.cat([folded, t[0][ell:]])
            u[b] = t
    A = [None, None]
    steps = eng.diagonal_steps(diags)
    for g in giants:
        S = [None, None]
        for j, s in enumerate(steps):
            if s - s % n1 != g:
                continue
            for comp in range(2):
                prod = eng.ntt.mont_mult([diags.data[j][0]], [u[s % n1][comp]], level, d, -2)[0]
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
    return eng.rescale(eng._new(([out[0]], [out[1]]), ct.origin, level=level))


@pytest.fixture(scope="module")
def checker():
    from liberate_fhe_amd.fhe import ckks_engine
    from tests.oracle_backend import OracleBackend
    eng = ckks_engine(devices=["cpu"], backend=OracleBackend(), **LT)
    assert eng.num_slots == n
    return eng, keys_for(eng, ALL_STEPS)


def test_bsgs_split():
    for n1, steps in CASES + [(8, range(64)), (3, (0, 1, 2, 3, 4, 100)), (5, (n + 7, -1))]:
        got_n1, babies, giants = encdec.bsgs_split(steps, n, n1)
        assert got_n1 == n1 and babies == sorted(set(babies)) and giants == sorted(set(giants))
        assert all(0 <= b < n1 for b in babies) and all(g % n1 == 0 and 0 <= g < n for g in giants)
        for s in steps:
            s %= n                                                     # steps are taken mod num_slots
            assert s % n1 in babies and s - s % n1 in giants
        assert {g + b for g in giants for b in babies} >= {s % n for s in steps}
    assert encdec.bsgs_split(range(64), n)[0] == 8                     # 7 + 7 keys; 4 and 16 would need 18
    assert encdec.bsgs_split(range(64), n) == (8, list(range(8)), list(range(0, 64, 8)))
    assert encdec.bsgs_split(range(32), n)[0] == 8                     # 4: 3 + 7, 8: 7 + 3: the tie goes to the larger n1
    assert encdec.bsgs_split([n - 1], n, 4) == (4, [3], [n - 4])       # a wrapped step lands in the giant step num_slots - n1
    assert encdec.bsgs_split([n - 1, 3], n, 16) == (16, [3, 15], [0, n - 16])
    assert encdec.bsgs_split([-1], n, 4) == encdec.bsgs_split([n - 1], n, 4)
    assert encdec.bsgs_split(range(-32, 32), n, 8)[2] == [0, 8, 16, 24, n - 32, n - 24, n - 16, n - 8]
    for bad in (0, -2, 2.5, "4", True):
        with pytest.raises(ValueError):
            encdec.bsgs_split([1], n, bad)
    with pytest.raises(ValueError):
        encdec.bsgs_split([], n)


@pytest.mark.parametrize("level", [0, 2])
def test_checker_bsgs_equals_the_composition(checker, level):
    eng, keys = checker
    ct = lazy_ciphertext(eng, 90 + level, level)
    for n1, steps in CASES:
        diags = synth.diagonals_bsgs(eng, 7 + level, level, steps, n1)
        assert eng.bsgs_steps(diags) == encdec.bsgs_split(steps, n, n1)
        got = eng.linear_transform(ct, diags, keys)
        want = bsgs_composition(eng, ct, diags, keys)
        assert got.level == level + 1 and got.origin == ct.origin and not got.ntt_state and not got.include_special
        gw, ww = words(got), words(want)
        assert gw[0].shape == ww[0].shape
        assert torch.equal(gw[0], ww[0]) and torch.equal(gw[1], ww[1]), (level, n1, steps)
    # a list of keys serves as well as a mapping, in any order
    n1, steps = CASES[1]
    diags = synth.diagonals_bsgs(eng, 3, level, steps, n1)
    _, babies, giants = eng.bsgs_steps(diags)
    a = eng.linear_transform(ct, diags, keys)
    b = eng.linear_transform(ct, diags, [keys[s] for s in reversed(sorted(set(babies + giants))) if s])
    assert all(torch.equal(x, y) for x, y in zip(words(a), words(b)))


@pytest.mark.parametrize("level", [0, 2])
def test_one_giant_step_gives_the_flat_words(checker, level):
    """n1 above every step: one giant step, g = 0, nothing is rolled, and the words are those of the flat op on the same pack
    (diagonals_bsgs seeds a step's words as diagonals does, so the two objects hold the same words)."""
    eng, keys = checker
    ct = lazy_ciphertext(eng, 70 + level, level)
    for steps in ((0, 1, 2, 5, 11), (1, 5), (0,)):
        flat = synth.diagonals(eng, 9, level, steps)
        bsgs = synth.diagonals_bsgs(eng, 9, level, steps, 16)
        assert all(torch.equal(x[0], y[0]) for x, y in zip(flat.data, bsgs.data))
        assert eng.bsgs_steps(bsgs) == (16, sorted(steps), [0])
        a, b = eng.linear_transform(ct, flat, keys), eng.linear_transform(ct, bsgs, keys)
        assert all(torch.equal(x, y) for x, y in zip(words(a), words(b))), (level, steps)


def test_refusals_and_round_trips(checker, tmp_path):
    from liberate_fhe_amd.fhe.presets import errors, types
    eng, keys = checker
    ct = synth.ciphertext(eng, 95, 0)
    diags = synth.diagonals_bsgs(eng, 4, 0, (0, 1, 5, 9), 4)           # babies 0, 1; giants 0, 4, 8
    top = eng.num_levels - 1
    assert eng.bsgs_steps(diags) == (4, [0, 1], [0, 4, 8])
    with pytest.raises(errors.NotMatchType):                           # a missing baby key
        eng.linear_transform(ct, diags, [keys[4], keys[8]])
    with pytest.raises(errors.NotMatchType):                           # a missing giant key
        eng.linear_transform(ct, diags, [keys[1], keys[4]])
    with pytest.raises(errors.NotMatchType):                           # the flat form's keys do not serve (5 and 9 are no steps here)
        eng.linear_transform(ct, diags, [keys[1], keys[5], keys[9]])
    with pytest.raises(errors.NotMatchType):                           # a key of another kind
        eng.linear_transform(ct, diags, [keys[1], keys[4], keys[8], synth.key_switch_key(eng, 8)])
    with pytest.raises(errors.NotMatchType):                           # bsgs_steps of a flat object
        eng.bsgs_steps(synth.diagonals(eng, 4, 0, (0, 1)))
    for bad in (0, 2.5, -1):
        with pytest.raises(ValueError):
            eng.encode_diagonals({0: [1.0]}, 0, bsgs=bad)
    with pytest.raises(errors.NotMatchDataStructState):                # diagonals of another level
        eng.linear_transform(synth.ciphertext(eng, 95, 1), diags, keys)
    with pytest.raises(errors.MaximumLevelError):                      # no level left to rescale into
        eng.linear_transform(synth.ciphertext(eng, 95, top), synth.diagonals_bsgs(eng, 4, top, (0, 1), 4), keys)
    with pytest.raises(errors.MaximumLevelError):
        eng.encode_diagonals({0: [1.0]}, top, bsgs=4)
    with pytest.raises(NotImplementedError):
        eng.linear_transform(eng._new(ct.data, ct.origin, level=0, ntt_state=True), diags, keys)
    with pytest.raises(NotImplementedError):
        eng.linear_transform(eng._new(ct.data, ct.origin, level=0, include_special=True), diags, keys)
    with pytest.raises(ValueError):                                    # the same step twice after reduction mod num_slots
        eng.encode_diagonals({1: [1.0], 1 + n: [2.0]}, 0, bsgs=4)
    # baby 0 in giant 0 alone needs no key at all
    assert eng.linear_transform(ct, synth.diagonals_bsgs(eng, 4, 0, (0,), 4), []).level == 1

    # encode_diagonals(bsgs=): tag, steps, flags, views of one pack in (g, b) order
    np.random.seed(3)
    enc = eng.encode_diagonals({5: eng.example(-1, 1), 0: [0.5, -0.25], n + 700: eng.example(-1, 1)[:100], -1: 2.0, 6: 1.0}, 2, bsgs=4)
    assert enc.origin == f"plain diagonals bsgs:4;0,5,6,700,{n - 1}" and enc.origin.startswith(types.origins["diag_bsgs"])
    assert not enc.origin.startswith(types.origins["diag"])
    assert eng.diagonal_steps(enc) == [0, 5, 6, 700, n - 1] and eng.bsgs_steps(enc) == (4, [0, 1, 2, 3], [0, 4, 700, n - 4])
    assert (enc.level, enc.ntt_state, enc.montgomery_state, enc.include_special) == (2, True, True, True)
    rows = eng._rows(0, 2, True)
    assert all(len(row) == 1 and row[0].shape == (rows, eng.ctx.N) for row in enc.data)
    assert all(enc.data[j][0].data_ptr() == enc.data[0][0].data_ptr() + j * rows * eng.ctx.N * 8 for j in range(5))
    order = [(s - s % 4, s % 4) for s in eng.diagonal_steps(enc)]
    assert order == sorted(order)                                      # (g, b) order: giant step 4 is the slice [1:3]
    # bsgs=None is the flat object, and the flat tag is what it was
    flat = eng.encode_diagonals({1: [1.0], 0: [2.0]}, 2)
    assert flat.origin == "plain diagonals:0,1" and eng.diagonal_steps(flat) == [0, 1]
    # cpu() and save -> load keep the words, the steps and n1; the loaded object (no shared pack any more) transforms alike
    host = eng.cpu(enc)
    path = str(tmp_path / "diags_bsgs.pkl")
    eng.save(enc, path)
    back = eng.load(path)
    for other in (host, back):
        assert other.origin == enc.origin and other.level == enc.level and other.include_special
        assert len(other.data) == len(enc.data) and eng.bsgs_steps(other) == eng.bsgs_steps(enc)
    nat = eng._dest_rows(2, True)[0]
    for j in range(5):
        assert torch.equal(back.data[j][0], enc.data[j][0])
        assert torch.equal(host.data[j][0][nat], enc.data[j][0])
    more = keys_for(eng, (1, 2, 3, 4, 700, n - 4))
    ct2 = synth.ciphertext(eng, 96, 2)
    a, b = eng.linear_transform(ct2, enc, more), eng.linear_transform(ct2, back, more)
    assert all(torch.equal(x, y) for x, y in zip(words(a), words(b)))
    # a plain mapping handed to linear_transform stays flat: it needs the flat keys, not the split ones
    assert eng.linear_transform(ct2, {0: [1.0], 5: [0.5, 0.5]}, keys).level == 3


def _real_engine():
    from liberate_fhe_amd.fhe import ckks_engine
    from tests.oracle_backend import OracleBackend
    eng = ckks_engine(devices=["cpu"], backend=OracleBackend(), **LT)
    sk = eng.create_secret_key()
    pk = eng.create_public_key(sk)
    return eng, sk, pk


def _errors(eng, sk, ct, diag, n1, m):
    """(max error of the BSGS form, max error of the flat form) against numpy on the same ciphertext and diagonals"""
    want = sum(np.asarray(v) * np.roll(m, s) for s, v in diag.items())
    n1, babies, giants = encdec.bsgs_split(diag, eng.num_slots, n1)
    bkeys = [eng.create_rotation_key(sk, s) for s in sorted(set(babies + giants)) if s]
    got = eng.decrode(eng.linear_transform(ct, eng.encode_diagonals(diag, ct.level, bsgs=n1), bkeys), sk)
    del bkeys
    fkeys = [eng.create_rotation_key(sk, s) for s in sorted({s % eng.num_slots for s in diag}) if s]
    flat = eng.decrode(eng.linear_transform(ct, eng.encode_diagonals(diag, ct.level), fkeys), sk)
    return np.abs(got - want).max(), np.abs(flat - want).max(), len(fkeys)


def test_decryption_error_with_real_keys_stays_within_twice_the_flat_form():
    """Real keys on the checker engine: steps 0..11, 700, n - 6, n - 1 over n1 = 4 on a fresh ciphertext, and 64 consecutive
    wrapping steps -32..31 over n1 = 8 with complex diagonals.  The BSGS form adds one key-switch noise and one mod-down rounding
    per giant step, both at the scale of the unrescaled product; a maximum over thousands of slots of sums of the same noises:
    at most 2 x the flat form's maximum error on the same inputs (the margin this project uses for that comparison)."""
    eng, sk, pk = _real_engine()
    rng = np.random.default_rng(5)
    m = rng.uniform(-4, 4, n) + 1j * rng.uniform(-4, 4, n)
    ct = eng.encorypt(m, pk)
    steps = tuple(range(12)) + (700, n - 6, n - 1)
    diag = {s: rng.uniform(-2, 2, n) for s in steps}
    e_bsgs, e_flat, nflat = _errors(eng, sk, ct, diag, 4, m)
    print(f"steps 0..11, 700, n-6, n-1; n1 = 4; level 0: keys flat {nflat} / BSGS 8, max error BSGS {e_bsgs:.3e}, flat {e_flat:.3e}")
    assert e_bsgs <= 2 * e_flat and e_flat < 1e-6
    diag = {s: rng.uniform(-2, 2, n) + 1j * rng.uniform(-2, 2, n) for s in range(-32, 32)}
    assert encdec.bsgs_split(diag, n)[0] == 8
    e_bsgs, e_flat, nflat = _errors(eng, sk, ct, diag, None, m)
    print(f"64 wrapping steps -32..31; n1 = 8; level 0: keys flat {nflat} / BSGS 14, max error BSGS {e_bsgs:.3e}, flat {e_flat:.3e}")
    assert nflat == 63
    assert e_bsgs <= 2 * e_flat and e_flat < 1e-6


GLOO_N1, GLOO_STEPS = 4, (0, 1, 4, 9, 10)


def _gloo_run(eng):
    ct = synth.ciphertext(eng, 3, 0)
    _, babies, giants = encdec.bsgs_split(GLOO_STEPS, eng.num_slots, GLOO_N1)
    return eng.linear_transform(ct, synth.diagonals_bsgs(eng, 5, 0, GLOO_STEPS, GLOO_N1), keys_for(eng, sorted(set(babies + giants))))


def _worker(rank, world, port, outdir):
    warnings.filterwarnings("ignore")
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(1)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from liberate_fhe_amd.fhe import ckks_engine
    from liberate_fhe_amd.fhe.comm import DistComm
    from tests.oracle_backend import OracleBackend
    eng = ckks_engine(devices=["cpu"], backend=OracleBackend(), comm=DistComm(local_device="cpu"), **LT)
    r = _gloo_run(eng)
    for comp in range(2):
        np.save(os.path.join(outdir, f"{comp}.{rank}.npy"), r.data[comp][0].numpy() if r.data[comp] else
                np.zeros((0, eng.ctx.N), dtype=np.int64))
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_ranks_equal_one_process():
    """gloo world 2, one process per rank (the orchestrated path with a digit exchange per giant step and the rescale's row
    exchange): every rank's rows equal the single-process result on two devices."""
    from liberate_fhe_amd.fhe import ckks_engine
    from tests.oracle_backend import OracleBackend
    world = 2
    port = 37600 + (os.getpid() % 2000)
    with tempfile.TemporaryDirectory() as outdir:
        mp.spawn(_worker, args=(world, port, outdir), nprocs=world, join=True)
        got = {(c, r): np.load(os.path.join(outdir, f"{c}.{r}.npy")) for c in range(2) for r in range(world)}
    eng = ckks_engine(devices=["cpu"] * world, backend=OracleBackend(), **LT)
    want = _gloo_run(eng)
    assert want.level == 1
    for c in range(2):
        for r in range(world):
            w = want.data[c][r].numpy() if r < len(want.data[c]) else np.zeros((0, eng.ctx.N), dtype=np.int64)
            assert got[(c, r)].shape == w.shape and (got[(c, r)] == w).all(), (c, r)


_Q = np.array([(1 << 41) - 65535, (1 << 60) - 93, (1 << 60) - 173], dtype=np.int64)


def _fake_plan(logN):
    from liberate_fhe_amd._native import KsPlan
    plan = KsPlan()
    plan.logN, plan.ell, plan.K, plan.nparts, plan.dig_nparts, plan.max_nct = logN, 2, 1, 2, 2, 1
    for name, typ in KsPlan._fields_:
        if typ is ctypes.c_void_p:
            setattr(plan, name, 64)
    plan.q_host = _Q.ctypes.data
    return plan


def test_c_entry_refuses_bad_arguments_before_any_launch():
    """lf_linear_transform_bsgs returns LF_ERR_ARG from its arguments alone (pointers that are never dereferenced; no call here
    would pass the checks): what lf_linear_transform refuses, a baby index out of range or not ascending inside a giant step, a
    giant step without diagonals, a keyed giant step without a key, a workspace smaller than lf_linear_transform_bsgs_ws_words
    says; and that function's value from the shapes."""
    from liberate_fhe_amd._native import lib
    LF_ERR_ARG = 10001
    dummy = ctypes.c_void_p(64)
    arr = (ctypes.c_void_p * 4)(64, 64, 64, 64)
    stride = 3 << 13

    def i64(values):
        return (ctypes.c_int64 * max(1, len(values)))(*values)

    def call(plan, bexps=(3,), gexps=(0, 5), counts=(2, 1), bidx=(0, 1, 1), bkeys=arr, gkeys=arr, pt=dummy, ws=dummy, ws_words=1 << 40,
             out0=dummy, out1=dummy, c0=dummy, scales=dummy, pt_stride=stride, nb=None, ng=None):
        return lib.lf_linear_transform_bsgs(ctypes.byref(plan) if plan is not None else None, c0, dummy,
                                            len(bexps) if nb is None else nb, i64(bexps), bkeys,
                                            len(gexps) if ng is None else ng, i64(gexps), gkeys, 0, 0, 0, 0, pt, pt_stride,
                                            i64(counts), i64(bidx), scales, 0, ws, ws_words, out0, out1, None)

    for logN in (12, 18):
        plan = _fake_plan(logN)
        assert lib.lf_linear_transform_bsgs_ws_words(ctypes.byref(plan), 1) == 0
        assert call(plan) == LF_ERR_ARG, logN
    assert call(None) == LF_ERR_ARG
    plan = _fake_plan(13)
    N, rows, ell, N2 = 1 << 13, 3, 2, 2 << 13
    md1 = lib.lf_ks_moddown_ws_words(1, ell, 1, N)
    for nb in (0, 1, 7):
        # the baby pairs (slot 0: the ciphertext itself), four S pairs, the accumulator pair, w, the one-polynomial mod-down's
        # workspace, the final mod-down's [2][ell][N] result
        assert lib.lf_linear_transform_bsgs_ws_words(ctypes.byref(plan), nb) == 2 * rows * N * (nb + 1 + 4 + 1) + ell * N + md1 + 2 * ell * N
    assert lib.lf_linear_transform_bsgs_ws_words(ctypes.byref(plan), -1) == 0
    assert lib.lf_linear_transform_bsgs_ws_words(ctypes.byref(plan), 64) == 0
    need = lib.lf_linear_transform_bsgs_ws_words(ctypes.byref(plan), 1)
    assert call(plan, ws_words=need - 1) == LF_ERR_ARG                         # a workspace too small
    assert call(plan, ws=None) == LF_ERR_ARG
    assert call(plan, nb=-1) == LF_ERR_ARG
    assert call(plan, nb=64) == LF_ERR_ARG
    assert call(plan, ng=0) == LF_ERR_ARG                                      # no giant step at all
    assert call(plan, bkeys=None) == LF_ERR_ARG
    assert call(plan, gkeys=None) == LF_ERR_ARG
    assert call(plan, pt=None) == LF_ERR_ARG
    assert call(plan, out0=None) == LF_ERR_ARG
    assert call(plan, out1=None) == LF_ERR_ARG
    assert call(plan, c0=None) == LF_ERR_ARG
    assert call(plan, scales=None) == LF_ERR_ARG
    assert call(plan, pt_stride=stride - 1) == LF_ERR_ARG
    assert call(plan, bexps=(4,)) == LF_ERR_ARG                                # even exponent
    assert call(plan, bexps=(N2 + 1,)) == LF_ERR_ARG                           # >= 2N
    assert call(plan, bexps=(-3,)) == LF_ERR_ARG
    assert call(plan, gexps=(0, 6)) == LF_ERR_ARG
    assert call(plan, gexps=(0, N2 + 3)) == LF_ERR_ARG
    nul = (ctypes.c_void_p * 4)(64, None, 64, 64)
    assert call(plan, bexps=(3, 5), bkeys=nul, bidx=(0, 1, 2)) == LF_ERR_ARG   # a NULL baby key
    assert call(plan, gkeys=nul) == LF_ERR_ARG                                 # a NULL key of a keyed giant step
    assert call(plan, bidx=(0, 2, 1)) == LF_ERR_ARG                            # a baby index out of range (slots 0 .. nb)
    assert call(plan, bidx=(0, -1, 1)) == LF_ERR_ARG
    assert call(plan, bidx=(1, 0, 1)) == LF_ERR_ARG                            # not ascending inside a giant step
    assert call(plan, bidx=(1, 1, 1)) == LF_ERR_ARG
    assert call(plan, counts=(3, 0)) == LF_ERR_ARG                             # a giant step without diagonals
    one = _fake_plan(13)
    one.ell = 1                                                                # no level left to rescale into
    assert call(one) == LF_ERR_ARG


def test_the_engines_baby_key_limit_is_the_headers_and_the_entrys():
    """HipBackend.bsgs_max_baby_keys (what ckks_engine._linear_transform_bsgs hands to the native call) equals
    LF_BSGS_MAX_BABY_KEYS of include/ckks_hip.h, and the library accepts exactly that many: lf_linear_transform_bsgs_ws_words
    answers for nb = limit and refuses nb = limit + 1, and so does the entry itself (LF_ERR_ARG from its arguments)."""
    import re
    from liberate_fhe_amd._native import lib
    from liberate_fhe_amd.fhe.backend import HipBackend
    header = open(os.path.join(ROOT, "include", "ckks_hip.h")).read()
    limit = int(re.search(r"#define LF_BSGS_MAX_BABY_KEYS (\d+)", header).group(1))
    assert HipBackend.bsgs_max_baby_keys == limit == 63
    assert "define LF_BSGS_MAX_BABY_KEYS" not in open(os.path.join(ROOT, "liberate_fhe_amd", "csrc", "ckks_ops.hip")).read()
    plan = _fake_plan(13)
    assert lib.lf_linear_transform_bsgs_ws_words(ctypes.byref(plan), limit) > 0
    assert lib.lf_linear_transform_bsgs_ws_words(ctypes.byref(plan), limit + 1) == 0


def test_c_entries_refuse_more_digits_than_the_fp64_bound_before_any_launch():
    """LF_FP64_MAX_DIGITS (include/ckks_hip.h) = 119: the fp64-class inner products add one balanced product (|.| <= q / 2) per
    digit and reduce once, exactly for |x| < 64 q; ks_inner_giant_kernel adds two words below 2q besides, so nparts / 2 + 4 < 64
    is the tightest condition over the kernels and 119 the last digit count that meets it.  With a prime below 2^41 in q_host and
    nparts = 120 every entry that ends in such a kernel returns LF_ERR_ARG from its arguments alone (fake pointers, never
    dereferenced; a call that passed would launch, so acceptance is read from the *_ws_words functions, which launch nothing).
    Rows of the integer class only keep the entries' own limit of 254."""
    from liberate_fhe_amd._native import lib
    import re
    LF_ERR_ARG = 10001
    header = open(os.path.join(ROOT, "include", "ckks_hip.h")).read()
    BOUND = int(re.search(r"#define LF_FP64_MAX_DIGITS (\d+)", header).group(1))
    assert BOUND == max(n for n in range(1, 255) if n / 2 + 4 < 64) == 119      # the header's constant IS the derived one
    dummy = ctypes.c_void_p(64)
    arr = (ctypes.c_void_p * 8)(*[64] * 8)
    exps = (ctypes.c_int64 * 4)(3, 5, 7, 9)
    big = np.array([(1 << 60) - 93, (1 << 60) - 173, (1 << 59) - 55], dtype=np.int64)      # integer class only

    def plan_of(nparts, q):
        plan = _fake_plan(13)
        plan.nparts, plan.dig_nparts, plan.q_host = nparts, nparts, q.ctypes.data
        return plan

    def words(plan):
        ref = ctypes.byref(plan)
        return (lib.lf_linear_transform_bsgs_ws_words(ref, 3), lib.lf_cc_dot_ws_words(ref), lib.lf_rotate_hoisted_ws_words(ref))

    assert all(w > 0 for w in words(plan_of(BOUND, _Q)))                    # 119 digits beside an fp64-class row: accepted
    assert words(plan_of(BOUND + 1, _Q)) == (0, 0, 0)                       # 120: refused
    assert all(w > 0 for w in words(plan_of(254, big)))                     # integer class only: as before
    plan = plan_of(BOUND + 1, _Q)
    ref, S = ctypes.byref(plan), 3 << 13
    calls = {
        "lf_linear_transform_bsgs": lambda: lib.lf_linear_transform_bsgs(ref, dummy, dummy, 1, exps, arr, 2, (ctypes.c_int64 * 2)(0, 5), arr,
                                                                         0, 0, 0, 0, dummy, S, (ctypes.c_int64 * 2)(2, 1),
                                                                         (ctypes.c_int64 * 3)(0, 1, 1), dummy, 0, dummy, 1 << 40, dummy, dummy, None),
        "lf_linear_transform": lambda: lib.lf_linear_transform(ref, dummy, dummy, 2, exps, arr, 0, 0, 0, 0, dummy, S, dummy, dummy, 0, dummy,
                                                               1 << 40, dummy, dummy, None),
        "lf_rotate_hoisted": lambda: lib.lf_rotate_hoisted(ref, dummy, dummy, 2, exps, 1, arr, 0, 0, 0, 0, dummy, 1 << 40, arr, arr, None),
        "lf_cc_dot": lambda: lib.lf_cc_dot(ref, 2, arr, arr, dummy, 0, 0, 0, 0, dummy, 1 << 40, dummy, dummy, None),
        "lf_switch_key": lambda: lib.lf_switch_key(ref, dummy, dummy, 0, 0, dummy, 0, 0, 0, 0, dummy, dummy, None),
        "lf_cc_mult_evk": lambda: lib.lf_cc_mult_evk(ref, arr, arr, dummy, 0, 0, 0, 0, dummy, dummy, None),
        "lf_switch_key_batch": lambda: lib.lf_switch_key_batch(ref, 1, arr, arr, 0, 0, dummy, 0, 0, 0, 0, arr, arr, None),
        "lf_cc_mult_evk_batch": lambda: lib.lf_cc_mult_evk_batch(ref, 1, arr, arr, dummy, 0, 0, 0, 0, arr, arr, None),
        "lf_cc_mult_evk_post": lambda: lib.lf_cc_mult_evk_post(ref, dummy, 0, 0, 0, 0, dummy, dummy, 3, None),
        "lf_switch_key_post": lambda: lib.lf_switch_key_post(ref, dummy, 0, 0, dummy, 0, 0, 0, 0, dummy, dummy, 3, None),
    }
    q = ctypes.c_void_p(_Q.ctypes.data)
    n, rows, logN = BOUND + 1, 3, 13
    calls.update({
        "lf_ks_core_batch": lambda: lib.lf_ks_core_batch(dummy, 0, 1, n, rows, logN, dummy, dummy, dummy, dummy, 0, 0, 0, 0, dummy, dummy, dummy,
                                                         dummy, dummy, dummy, dummy, q, dummy, dummy, dummy, dummy, 0, None),
        "lf_ks_core": lambda: lib.lf_ks_core(dummy, n, rows, logN, dummy, dummy, dummy, dummy, 0, 0, 0, 0, dummy, dummy, dummy, dummy, dummy,
                                             dummy, dummy, q, dummy, dummy, dummy, dummy, 0, None),
        "lf_ks_tail": lambda: lib.lf_ks_tail(n, rows, logN, dummy, 0, 0, 0, 0, dummy, dummy, dummy, dummy, dummy, q, dummy, dummy, dummy, dummy,
                                             0, None),
        "lf_relin_core_batch": lambda: lib.lf_relin_core_batch(dummy, 0, 1, n, rows, logN, dummy, dummy, dummy, dummy, 0, 0, 0, 0, dummy, dummy,
                                                               dummy, dummy, dummy, dummy, dummy, dummy, 0, dummy, 2, dummy, q, dummy, dummy,
                                                               dummy, dummy, 0, None),
        "lf_relin_tail": lambda: lib.lf_relin_tail(n, rows, logN, dummy, 0, 0, 0, 0, dummy, dummy, dummy, dummy, dummy, dummy, dummy, 2, dummy,
                                                   q, dummy, dummy, dummy, dummy, 0, None),
    })
    for name, call in calls.items():
        assert call() == LF_ERR_ARG, name


def test_bsgs_kernels_use_no_scratch():
    """The three new launches exist under their own names (baby: 1, 2, 4 keys x raw / planes key x raw / planes digits; giant:
    raw / planes key x raw / planes digits; diagonal products: 1, 2, 4 giant steps per launch) with scratch 0, no spill, and an
    occupancy no lower than ks_inner_lt_kernel's with the same keys and formats (the streaming one: at least 4 waves per SIMD);
    the tracked table lists them as built."""
    import __graft_entry__ as g
    res = {r["kernel"]: r for r in g.kernel_resources()}
    fmts = [(pl, dpl) for pl in ("true", "false") for dpl in ("true", "false")]
    want = {}
    for pl, dpl in fmts:
        for nr in (1, 2, 4):
            want[f"ks_inner_baby_kernel<{nr}, {pl}, {dpl}>"] = res[f"ks_inner_lt_kernel<{nr}, {pl}, {dpl}>"]["occupancy"]
        want[f"ks_inner_giant_kernel<{pl}, {dpl}>"] = res[f"ks_inner_lt_kernel<1, {pl}, {dpl}>"]["occupancy"]
    for ng in (1, 2, 4):
        want[f"lt_diag_products_kernel<{ng}>"] = 4
    new = sorted(k for k in res if k.startswith(("ks_inner_baby_kernel<", "ks_inner_giant_kernel<", "lt_diag_products_kernel<")))
    assert new == sorted(want)
    tracked = open(os.path.join(ROOT, "profiles", "r06_kernel_resources.txt")).read()
    for k, floor in want.items():
        r = res[k]
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, r
        assert r["occupancy"] >= floor, (r, floor)
        line = next(ln for ln in tracked.splitlines() if ln[18:76].strip() == k)
        f = line.split()
        assert (int(f[-7]), int(f[-3]), int(f[-1])) == (r["vgprs"], r["scratch"], r["occupancy"]), line
