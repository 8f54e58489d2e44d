"""mod_raise, sparse secret keys and the coefficient / slot matrices without a GPU (liberate_fhe_amd/fhe/modraise.py,
encdec.coeff_slot_matrices, lf_mod_raise): the matrices against encode / decode; mod_raise's definition on the checker backend
against Python integers on edge words; the sparse key's weight, reproducibility and the untouched default draw; every refusal;
the C entry's argument checks and the kernel's resources."""
import ctypes
import os

import numpy as np
import pytest
import torch

from liberate_fhe_amd.fhe import encdec
from tests import helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P12 = dict(logN=12, num_scales=5, num_special_primes=2, is_secured=False)
SEED, NONCE = [11, 22, 33, 44, 55, 66, 77, 88], [99, 111]


def make(params=P12):
    from liberate_fhe_amd.fhe import ckks_engine
    from tests.oracle_backend import OracleBackend
    return ckks_engine(devices=["cpu"], backend=OracleBackend(), **params)


@pytest.fixture(scope="module")
def checker():
    return make()


# ---- the matrices ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,norm", [(16, "forward"), (64, "forward"), (64, "backward"), (64, "ortho"), (4096, "forward")])
def test_coeff_slot_matrices_against_encode_and_decode(N, norm):
    n = N // 2
    B, C, E, F = encdec.coeff_slot_matrices(N, norm)
    assert all(M.shape == (n, n) and M.dtype == np.complex128 for M in (B, C, E, F))
    assert encdec.coeff_slot_matrices(N, norm)[0] is B                       # kept per (N, norm)
    rng = np.random.default_rng(N)
    for _ in range(3):
        t = rng.normal(size=N)
        z = encdec.decode(torch.from_numpy(t), norm=norm, return_without_scaling=True)[:n].numpy()
        u = t[:n] + 1j * t[n:]
        assert np.abs(u - (B @ z + C @ z.conj())).max() <= 1e-9 * np.abs(u).max()
        assert np.abs(z - (E @ u + F @ u.conj())).max() <= 1e-9 * np.abs(z).max()
        # .. and encode is the map the first pair inverts
        back = encdec.encode(z, device="cpu", norm=norm, return_without_scaling=True).numpy()
        assert np.abs(back - t).max() <= 1e-9 * np.abs(t).max()
    # generator 3: zeta_k^(N/2) alternates between +i and -i, so neither map is complex-linear
    assert np.abs(C).max() > 0.1 * np.abs(B).max() and np.abs(F).max() > 0.1 * np.abs(E).max()
    assert np.abs(B @ E + C @ F.conj() - np.eye(n)).max() <= 1e-9
    assert np.abs(B @ F + C @ E.conj()).max() <= 1e-9


def test_coeff_slot_matrices_refuse_other_sizes():
    for N in (0, 2, 12, 100):
        with pytest.raises(ValueError):
            encdec.coeff_slot_matrices(N)


# ---- the word definition -----------------------------------------------------------------------------------------------
def base_words(qb):
    """what a base-prime row may hold: the canonical edge values, their lazy forms below 2 q_b, and the negative words a rescale
    leaves (REDC of a negative product: above -q_b / 2)"""
    h = (qb - 1) // 2
    canon = [0, 1, 2, h - 1, h, h + 1, h + 2, qb - 2, qb - 1]
    return canon + [qb + v for v in canon] + [-1, -2, -(h // 2), -h + 1, -h]


def centred(w, qb):
    r = w % qb
    return r - qb if r > (qb - 1) // 2 else r


def with_base_rows(eng, level, seed):
    """an edge ciphertext of `level` whose base-prime rows walk through base_words, c1 one step ahead of c0"""
    ct = helpers.edge_ciphertext(eng, level, "mixed", seed)
    d, row = eng._base_row_at(level)
    vals = base_words(eng.base_prime)
    data = []
    for comp in range(2):
        t = ct.data[comp][d].clone()
        t[row] = torch.tensor([vals[(j + comp + seed) % len(vals)] for j in range(eng.ctx.N)], dtype=torch.int64)
        data.append([t])
    return ct._replace(data=tuple(data))


def expected_rows(eng, ct):
    qb = eng.base_prime
    d, row = eng._base_row_at(ct.level)
    out = []
    for comp in range(2):
        v = [centred(int(w), qb) for w in ct.data[comp][d][row]]
        assert all(abs(x) <= (qb - 1) // 2 for x in v)
        out.append(torch.tensor([[x % eng.ctx.q[i] for x in v] for i in eng.ntt.p.destination_arrays[0][0]], dtype=torch.int64))
    return out


def test_mod_raise_words_against_python_integers(checker):
    from liberate_fhe_amd.fhe.presets import types
    eng = checker
    top = eng.num_levels - 1
    assert not hasattr(eng.backend, "mod_raise_call")                       # the checker takes the torch chain: the definition
    for level in (0, 2, top - 1, top):
        ct = with_base_rows(eng, level, level)
        kept = [t.clone() for comp in ct.data for t in comp]
        got = eng.mod_raise(ct)
        assert got.level == 0 and got.origin == types.origins["ct"]
        assert not got.ntt_state and not got.montgomery_state and not got.include_special
        assert got.hash == ct.hash and got.version == ct.version
        want = expected_rows(eng, ct)
        for comp in range(2):
            assert len(got.data[comp]) == 1 and torch.equal(got.data[comp][0], want[comp]), (level, comp)
        assert all(torch.equal(a, b) for a, b in zip(kept, [t for comp in ct.data for t in comp]))       # the operand is read only
    # only the base row is read
    a = with_base_rows(eng, 1, 5)
    b = a._replace(data=tuple([t.clone()] for (t,) in a.data))
    d, row = eng._base_row_at(1)
    for comp in range(2):
        b.data[comp][0][:row] = 0
    ra, rb = eng.mod_raise(a), eng.mod_raise(b)
    assert all(torch.equal(ra.data[c][0], rb.data[c][0]) for c in range(2))


def test_batch_equals_the_loop_in_order(checker):
    eng = checker
    top = eng.num_levels - 1
    cts = [with_base_rows(eng, l, 10 + i) for i, l in enumerate((0, top, 2, 0, top - 1))]
    cts.append(cts[1])                                                      # the same object twice
    got = eng.mod_raise_batch(iter(cts))
    assert len(got) == len(cts)
    for g, ct in zip(got, cts):
        one = eng.mod_raise(ct)
        assert g.level == 0 and all(torch.equal(g.data[c][0], one.data[c][0]) for c in range(2))
    assert eng.mod_raise_batch([]) == []


def test_refusals(checker):
    from liberate_fhe_amd.fhe.presets import errors, types
    from liberate_fhe_amd.utils import synth
    eng = checker
    good = with_base_rows(eng, 1, 0)
    ntt = good._replace(ntt_state=True)
    mont = good._replace(montgomery_state=True)
    special = good._replace(include_special=True)
    triplet = good._replace(origin=types.origins["ctt"], data=tuple(good.data) + (good.data[0],))
    plain = helpers.edge_plaintext(eng, 1, "top", 0, kind="add")
    for bad, err in ((ntt, errors.NotMatchDataStructState), (mont, errors.NotMatchDataStructState),
                     (special, errors.NotMatchDataStructState), (triplet, errors.NotMatchType), (plain, errors.NotMatchType),
                     (synth.key_switch_key(eng, 3), errors.NotMatchType), (None, errors.NotMatchType), (3, errors.NotMatchType)):
        with pytest.raises(err):
            eng.mod_raise(bad)
        with pytest.raises(err):
            eng.mod_raise_batch([good, bad, good])
        if bad is not None and bad != 3:
            with pytest.raises(err):
                eng.coeffs_to_slots(bad, [], None)
            with pytest.raises(err):
                eng.slots_to_coeffs(bad, [], None)


# ---- several devices, several ranks ------------------------------------------------------------------------------------
def _raise_worker(rank, world, port, outdir):
    import sys
    import warnings
    warnings.filterwarnings("ignore")
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(1)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from liberate_fhe_amd.fhe import ckks_engine
    from liberate_fhe_amd.fhe.comm import DistComm
    from liberate_fhe_amd.utils import synth
    from tests.oracle_backend import OracleBackend
    eng = ckks_engine(devices=["cpu"], backend=OracleBackend(), comm=DistComm(local_device="cpu"), **P12)
    assert eng.local_ids == [rank] and eng._multi
    for level in (0, eng.num_levels - 1):
        up = eng.mod_raise(synth.ciphertext(eng, 40 + level, level))
        for comp, shards in enumerate(up.data):
            assert up.level == 0 and len(shards) == 1
            np.save(os.path.join(outdir, f"{level}.{comp}.{rank}.npy"), shards[0].numpy())
    dist.barrier()
    dist.destroy_process_group()


def test_two_devices_and_two_ranks_take_the_same_words_through_torch():
    """one process driving two devices against the definition, and one process per device (gloo) against that"""
    import tempfile
    import warnings
    import torch.multiprocessing as mp
    from liberate_fhe_amd.fhe import ckks_engine
    from liberate_fhe_amd.utils import synth
    from tests.oracle_backend import OracleBackend
    warnings.filterwarnings("ignore")
    eng = ckks_engine(devices=["cpu"] * 2, backend=OracleBackend(), **P12)
    qb = eng.base_prime
    want = {}
    for level in (0, eng.num_levels - 1):
        ct = synth.ciphertext(eng, 40 + level, level)
        src, row = eng._base_row_at(level)
        up = eng.mod_raise(ct)
        assert up.level == 0 and [len(c) for c in up.data] == [2, 2]
        for comp in range(2):
            v = [centred(int(w), qb) for w in ct.data[comp][eng._loc(level).index(src)][row]]
            for d, t in enumerate(up.data[comp]):
                primes = eng.ntt.p.destination_arrays[0][d]
                assert t.shape == (len(primes), eng.ctx.N)
                assert torch.equal(t, torch.tensor([[x % eng.ctx.q[p] for x in v] for p in primes], dtype=torch.int64)), (level, comp, d)
                want[(level, comp, d)] = t.numpy()
    port = 29500 + (os.getpid() % 2000) + 97
    with tempfile.TemporaryDirectory() as outdir:
        mp.spawn(_raise_worker, args=(2, port, outdir), nprocs=2, join=True)
        for (level, comp, d), t in want.items():
            assert np.array_equal(np.load(os.path.join(outdir, f"{level}.{comp}.{d}.npy")), t), (level, comp, d)


# ---- the sparse key ----------------------------------------------------------------------------------------------------
def key_coefficients(eng, sk):
    """the secret's coefficients as signed integers, from its NTT / Montgomery words"""
    s = sk.data[0].clone()
    eng.ntt.intt_exit_reduce_signed([s], 0, -2 if sk.include_special else -1)
    assert all(torch.equal(s[0], row) for row in s)
    return s[0]


def seeded():
    eng = make()
    eng.rng.refresh(SEED, NONCE)
    return eng


@pytest.mark.parametrize("h", [1, 32, 192, 4096])
def test_sparse_key_has_exactly_h_signed_ones(h):
    from liberate_fhe_amd.fhe.presets import types
    eng = seeded()
    dense = eng.create_secret_key()
    sk = eng.create_secret_key(hamming_weight=h)
    assert (sk.origin, sk.level, sk.include_special, sk.ntt_state, sk.montgomery_state) == \
        (dense.origin, dense.level, dense.include_special, dense.ntt_state, dense.montgomery_state)
    assert sk.origin == types.origins["sk"] and [tuple(t.shape) for t in sk.data] == [tuple(t.shape) for t in dense.data]
    s = key_coefficients(eng, sk)
    assert int((s != 0).sum()) == h and set(s.unique().tolist()) <= {-1, 0, 1}
    if h >= 32:
        assert 0 < int((s == 1).sum()) < h                                  # both signs occur
    short = eng.create_secret_key(include_special=False, hamming_weight=h)
    assert not short.include_special and int((key_coefficients(eng, short) != 0).sum()) == h


def test_sparse_key_is_reproducible_and_follows_the_documented_derivation():
    a, b = seeded(), seeded()
    ka, kb = a.create_secret_key(hamming_weight=32), b.create_secret_key(hamming_weight=32)
    assert all(torch.equal(x, y) for x, y in zip(ka.data, kb.data))
    assert not all(torch.equal(x, y) for x, y in zip(ka.data, a.create_secret_key(hamming_weight=32).data))      # the stream moved on
    # one draw of N words below 2^62 from the repeating channel; rank = w >> 1, sign = bit 0, stable order
    c = seeded()
    w = [int(x) for x in c.rng.randint(amax=1 << 62, shift=0, repeats=1)[0].reshape(-1)]
    order = sorted(range(len(w)), key=lambda j: (w[j] >> 1, j))[:32]
    want = torch.zeros(len(w), dtype=torch.int64)
    for j in order:
        want[j] = 1 - 2 * (w[j] & 1)
    assert torch.equal(key_coefficients(a, ka), want)
    # one draw: the next draw of both engines is the same as after a dense key's single draw
    d = seeded()
    d.create_secret_key()
    b.create_secret_key(hamming_weight=7)
    d.create_secret_key()
    assert torch.equal(b.rng.randint(amax=3, shift=-1, repeats=1)[0], d.rng.randint(amax=3, shift=-1, repeats=1)[0])


def test_default_key_words_and_rng_consumption_are_unchanged():
    before = seeded()
    k0 = before.create_secret_key()
    n0 = before.rng.randint(amax=3, shift=-1, repeats=1)[0]
    third = seeded()
    third.create_secret_key(hamming_weight=32)                             # an unrelated sparse draw on a third engine
    after = seeded()
    k1 = after.create_secret_key(include_special=True, hamming_weight=None)
    n1 = after.rng.randint(amax=3, shift=-1, repeats=1)[0]
    assert all(torch.equal(x, y) for x, y in zip(k0.data, k1.data)) and torch.equal(n0, n1)
    # .. and they are the words of the draw the method has always made
    ref = seeded()
    ternary = [t for t in ref.rng.randint(amax=3, shift=-1, repeats=1) if t is not None]
    sk = ref.ntt.tile_unsigned(ternary, lvl=0, mult_type=-2)
    ref.ntt.enter_ntt(sk, 0, -2)
    assert all(torch.equal(x, y) for x, y in zip(k0.data, sk))


@pytest.mark.parametrize("bad", [0, -1, 4097, 1.5, 32.0, True, "32", [32]])
def test_sparse_key_refuses_other_weights(checker, bad):
    with pytest.raises(ValueError):
        checker.create_secret_key(hamming_weight=bad)


# ---- depths, steps, the one-row matrix ---------------------------------------------------------------------------------
def test_steps_and_depths(checker):
    eng = checker
    n = eng.num_slots
    n1, babies, giants = eng.coeff_slot_steps()
    assert n1 == 64 and babies == list(range(n1)) and giants == list(range(0, n, n1))
    assert eng.coeff_slot_steps(16) == encdec.bsgs_split(range(n), n, 16)
    assert eng.coeffs_to_slots_depth(None) == 1 and eng.slots_to_coeffs_depth(None) == 1
    # the raised ciphertext: scale^2 / q_b is about 2^20, the entries GROW — one level
    assert eng.coeffs_to_slots_depth(eng.base_prime) == 1
    # a divisor far above the level's own scale: the constant goes through a level of its own
    assert eng.coeffs_to_slots_depth(float(eng.scale) ** 3) == 2 and eng.slots_to_coeffs_depth(eng.base_prime) == 2
    for bad in (0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            eng.coeffs_to_slots_depth(bad)
    d = {0: np.ones(n), 3: np.ones(n)}
    e = {1: np.ones(n), 70: np.ones(n)}
    assert eng.linear_transform_conj_steps(d, e, 8) == eng.lt_matmul_bsgs_steps([[d, e]], 8) == (8, [0, 1, 3, 6], [0, 64])
    assert eng.linear_transform_conj_steps(d, None, 2) == (2, [0, 1], [0, 2])
    with pytest.raises(ValueError):
        eng.linear_transform_conj_steps(None, None, 2)


# ---- the native entry --------------------------------------------------------------------------------------------------
def test_abi_and_caps():
    import re
    from liberate_fhe_amd import _native
    from liberate_fhe_amd.fhe.backend import HipBackend
    assert "lf_mod_raise" in _native.EXPORTED and _native.lib.lf_abi_version() == 15
    header = open(os.path.join(ROOT, "include", "ckks_hip.h")).read()
    cap = int(re.search(r"#define LF_MOD_RAISE_MAX_CTS (\d+)", header).group(1))
    assert cap == _native.LF_MOD_RAISE_MAX_CTS == HipBackend.mod_raise_max_cts == 64
    assert len(_native._SIGNATURES["lf_mod_raise"]) == 15


def test_c_entry_refuses_from_its_arguments_alone():
    """dummy pointers that are never dereferenced: no call here is one that would pass the checks"""
    from liberate_fhe_amd import _native
    lib, E, cap = _native.lib, _native.LF_ERR_ARG, _native.LF_MOD_RAISE_MAX_CTS
    d = ctypes.c_void_p(64)

    def call(count=1, rows=3, N=4096, qb=(1 << 60) - 93, arrays=None, drop=(), n_arr=None):
        n = max(count, 1) if n_arr is None else n_arr
        arr = {name: (ctypes.c_void_p * n)(*[64] * n) for name in ("in0", "in1", "out0", "out1")}
        for name, values in (arrays or {}).items():
            arr[name] = (ctypes.c_void_p * len(values))(*values)
        args = dict(arr, mont_one=d, ql=d, qh=d, kl=d, kh=d)
        for name in drop:
            args[name] = None
        return lib.lf_mod_raise(count, args["in0"], args["in1"], args["out0"], args["out1"], rows, N, qb, args["mont_one"],
                                args["ql"], args["qh"], args["kl"], args["kh"], 0, None)

    assert call(count=0) == E and call(count=-3) == E and call(count=cap + 1) == E
    assert call(rows=-1) == E and call(rows=lib.lf_limits(2) + 1) == E
    assert call(N=0) == E and call(N=1) == E and call(N=4097) == E
    assert call(qb=0) == E and call(qb=2) == E and call(qb=1 << 62) == E and call(qb=-5) == E
    for name in ("in0", "in1", "out0", "out1", "mont_one", "ql", "qh", "kl", "kh"):
        assert call(drop=(name,)) == E, name
    for name in ("in0", "in1", "out0", "out1"):
        assert call(count=2, arrays={name: [64, None]}) == E, name          # a NULL entry
        assert call(count=2, arrays={name: [64, 72]}) == E, name            # a misaligned one
        assert call(arrays={name: [8]}) == E, name
    assert call(count=cap, rows=0) == 0                                     # nothing to do is not an error, and launches nothing


def test_kernel_resources_are_tracked():
    import __graft_entry__ as g
    g.build()
    res = {r["kernel"]: r for r in g.kernel_resources()}
    k = res["mod_raise_kernel"]
    assert k["file"] == "ckks_raise.hip" and k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["occupancy"] == 8
    tracked = open(os.path.join(ROOT, "profiles", "r06_kernel_resources.txt")).read()
    line = next(ln for ln in tracked.splitlines() if " mod_raise_kernel " in ln)
    assert line.split()[:2] == ["ckks_raise.hip", "mod_raise_kernel"]
    assert [int(x) for x in line.split()[2:]] == [k["vgprs"], k["agprs"], k["sgprs"], k["lds"], k["scratch"], k["vgpr_spill"], k["occupancy"]]
