"""Hoisted rotations (ckks_engine.rotate_hoisted, lf_rotate_hoisted) without a GPU: the slot permutation pi_p against the oracle,
the engine's host logic on the checker backend against the composition of the public step methods that defines the words, the
sharded ranks, the C entry's argument checks and the new kernel's resources."""
import ctypes
import os
import sys
import tempfile
import warnings

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from oracle import oracle as orc
from liberate_fhe_amd.fhe import encdec
from liberate_fhe_amd.utils import synth
from tests.helpers import Limbs, pick_primes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROT = dict(logN=13, num_scales=5, num_special_primes=2, is_secured=False)   # two-pass ring, two digits


@pytest.mark.parametrize("logN", list(range(4, 14)))
def test_ntt_galois_index_is_the_slot_permutation_of_x_to_the_p(logN):
    """oracle ntt(a(X^p)) == ntt(a) gathered by encdec.ntt_galois_index(logN, p), mod q, on every row."""
    lim = Limbs(logN, pick_primes(logN, 2, 1))
    psi, _ = lim.mont_tables()
    N = lim.N
    x = lim.uniform(11)
    for p in sorted({3, 5, pow(3, 7, 2 * N), 2 * N - 1}):
        a = x.copy()
        ga = np.empty_like(x)
        orc.galois(x, ga, lim.rows, p)
        for y in (a, ga):
            orc.mont_enter(y, lim.Rs, lim.rows, *lim.mont_args())
            orc.ntt(y, psi, lim.rows, logN, lim._2q, *lim.mont_args())
        idx = encdec.ntt_galois_index(logN, p)
        assert sorted(idx.tolist()) == list(range(N))
        for r, q in enumerate(lim.q):
            assert ((ga[r].astype(object) - a[r][idx].astype(object)) % q == 0).all(), (logN, p, r)
    with pytest.raises(ValueError):
        encdec.ntt_galois_index(logN, 2)


def composition(eng, ct, rotk):
    """The definition of a hoisted rotation's words from the engine's public steps on one device: c1 made canonical, per part
    pre_extend -> extend -> exact forward NTT -> gathered by pi_p -> mont_mult with the key part, mont_add over the parts,
    intt_exit_reduce, mod-down with c0(X^p) made canonical (tests/test_engine_golden.py _reference_shaped_switcher + the gather)."""
    d, N, logN, level = 0, eng.ctx.N, eng.ctx.logN, ct.level
    ell, K = eng._rows(d, level, False), eng.ntt.num_special_primes
    p = encdec.galois_exponent(N, int(rotk.origin.split(":")[-1]))
    idx = torch.from_numpy(encdec.ntt_galois_index(logN, p))
    _2q = eng._vec("_2q", d, level, False)
    c1 = torch.empty_like(ct.data[1][0])
    eng.backend.galois(ct.data[1][0].contiguous(), c1, ell, logN, 1, _2q)
    sums = None
    for part_id in range(len(eng.ntt.p.p[level][d])):
        state = eng.pre_extend([c1], d, level, part_id)
        ext = eng.extend(state, d, level, part_id, d)
        eng.ntt.ntt([ext], level, d, -2)
        ext = ext[:, idx].contiguous()
        part = rotk.data[eng.parts_alloc[level][d][part_id]].data
        start = eng.ntt.starts[level][d]
        d0 = eng.ntt.mont_mult([ext], [part[0][0][start:]], level, d, -2)[0]
        d1 = eng.ntt.mont_mult([ext], [part[1][0][start:]], level, d, -2)[0]
        sums = [d0, d1] if sums is None else [eng.ntt.mont_add([sums[0]], [d0], level, d, -2)[0],
                                              eng.ntt.mont_add([sums[1]], [d1], level, d, -2)[0]]
    s = torch.stack(sums).contiguous()
    eng.ntt.intt_exit_reduce([s[0]], level, d, -2)
    eng.ntt.intt_exit_reduce([s[1]], level, d, -2)
    out = torch.empty((2, ell, N), dtype=torch.int64, device=s.device)
    tabs = eng._ks_tables(level)
    eng.backend.ks_moddown_batch([s[0], s[1]], [out[0], out[1]], [ct.data[0][0].contiguous(), None], ell, K, tabs[("pir", d)],
                                 eng._vec("Rs", d, level, True), eng._consts(d, level, True), PiP=None,
                                 galois=(pow(p, -1, 2 * N), _2q))
    return out


def words(ct):
    return [torch.cat([t.cpu() for t in comp]) for comp in ct.data]


def test_checker_rotate_hoisted_equals_the_composition():
    from liberate_fhe_amd.fhe import ckks_engine
    from liberate_fhe_amd.fhe.presets import errors
    from tests.oracle_backend import OracleBackend
    eng = ckks_engine(devices=["cpu"], backend=OracleBackend(), **ROT)
    keys = [synth.key_switch_key(eng, 40 + i, origin=f"rotation key:{delta}") for i, delta in enumerate((1, 2, 5, 11, 700))]
    for level in (0, 2):
        ct = synth.ciphertext(eng, 90 + level, level)
        # lazy words in c1: + q on every other coefficient (the canonical step folds them)
        q = torch.as_tensor(eng._consts(0, level, False).q_host).view(-1, 1)
        c1 = ct.data[1][0].clone()
        c1[:, ::2] += q
        ct.data[1][0] = c1
        want = [composition(eng, ct, k) for k in keys]
        for sel in ([0], [0, 1], [0, 1, 2], [0, 1, 2, 3, 4], [3, 3, 1]):
            got = eng.rotate_hoisted(ct, [keys[i] for i in sel])
            assert len(got) == len(sel)
            for g, i in zip(got, sel):
                assert g.level == level and g.origin == ct.origin and g.montgomery_state == ct.montgomery_state
                w = words(g)
                assert torch.equal(w[0], want[i][0]) and torch.equal(w[1], want[i][1]), (level, sel, i)
        # a step-0 key: rotate_single's words
        k0 = synth.key_switch_key(eng, 49, origin="rotation key:0")
        got, ref = eng.rotate_hoisted(ct, [k0, keys[1]])[0], eng.rotate_single(ct, k0)
        assert all(torch.equal(a, b) for a, b in zip(words(got), words(ref)))
        # and not rotate_single's words for another step (both decrypt alike: tests/test_rotate_hoisted_gpu.py)
        assert not torch.equal(words(eng.rotate_hoisted(ct, [keys[0]])[0])[1], words(eng.rotate_single(ct, keys[0]))[1])
    ct = synth.ciphertext(eng, 95, 0)
    assert eng.rotate_hoisted(ct, []) == []
    with pytest.raises(errors.NotMatchType):
        eng.rotate_hoisted(ct, [synth.key_switch_key(eng, 8)])
    with pytest.raises(errors.NotMatchType):
        eng.rotate_hoisted(keys[0], keys[:1])
    with pytest.raises(NotImplementedError):
        eng.rotate_hoisted(eng._new(ct.data, ct.origin, level=0, ntt_state=True), keys[:1])


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
    eng = ckks_engine(devices=["cpu"], backend=OracleBackend(), comm=DistComm(local_device="cpu"), **ROT)
    ct = synth.ciphertext(eng, 3, 0)
    keys = [synth.key_switch_key(eng, 6 + i, origin=f"rotation key:{delta}") for i, delta in enumerate((1, 4, 9))]
    for j, r in enumerate(eng.rotate_hoisted(ct, keys)):
        for comp in range(2):
            np.save(os.path.join(outdir, f"{j}.{comp}.{rank}.npy"), r.data[comp][0].numpy() if r.data[comp] else
                    np.zeros((0, eng.ctx.N), dtype=np.int64))
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_ranks_equal_one_process():
    """gloo world 2, one process per rank (the orchestrated path with the digit exchange): the shards of every rotation equal
    the single-process result on two devices."""
    from liberate_fhe_amd.fhe import ckks_engine
    from tests.oracle_backend import OracleBackend
    world = 2
    port = 33500 + (os.getpid() % 2000)
    with tempfile.TemporaryDirectory() as outdir:
        mp.spawn(_worker, args=(world, port, outdir), nprocs=world, join=True)
        got = {(j, c, r): np.load(os.path.join(outdir, f"{j}.{c}.{r}.npy")) for j in range(3) for c in range(2) for r in range(world)}
    eng = ckks_engine(devices=["cpu"] * world, backend=OracleBackend(), **ROT)
    ct = synth.ciphertext(eng, 3, 0)
    keys = [synth.key_switch_key(eng, 6 + i, origin=f"rotation key:{delta}") for i, delta in enumerate((1, 4, 9))]
    want = eng.rotate_hoisted(ct, keys)
    for j in range(3):
        for c in range(2):
            for r in range(world):
                assert (got[(j, c, r)] == want[j].data[c][r].numpy()).all(), (j, c, r)


def _fake_plan(logN, max_nct=4):
    from liberate_fhe_amd._native import KsPlan
    plan = KsPlan()
    plan.logN, plan.ell, plan.K, plan.nparts, plan.dig_nparts, plan.max_nct = logN, 2, 1, 2, 2, max_nct
    for name, typ in KsPlan._fields_:
        if typ is ctypes.c_void_p:
            setattr(plan, name, 64)
    plan.q_host = _Q.ctypes.data
    return plan


_Q = np.array([(1 << 41) - 65535, (1 << 60) - 93, (1 << 60) - 173], dtype=np.int64)


def test_c_entry_refuses_bad_arguments_before_any_launch():
    """lf_rotate_hoisted returns LF_ERR_ARG from its arguments alone (pointers that are never dereferenced; no call here would
    pass the checks): nr < 1, a NULL key / output / exponent array, an even exponent or one outside (0, 2N), a workspace
    smaller than lf_rotate_hoisted_ws_words says, plans at logN 12 and 18."""
    from liberate_fhe_amd._native import lib
    LF_ERR_ARG = 10001
    dummy = ctypes.c_void_p(64)
    arr = (ctypes.c_void_p * 4)(64, 64, 64, 64)

    def call(plan, nr, exps, keys=arr, ws=None, ws_words=0, out0=arr, out1=arr):
        e = (ctypes.c_int64 * max(1, len(exps)))(*exps) if exps is not None else None
        return lib.lf_rotate_hoisted(ctypes.byref(plan), dummy, dummy, nr, e, 1, keys, 0, 0, 0, 0, ws, ws_words, out0, out1, None)

    for logN in (12, 18):
        plan = _fake_plan(logN)
        assert lib.lf_rotate_hoisted_ws_words(ctypes.byref(plan)) == 0
        assert call(plan, 1, [3]) == LF_ERR_ARG, logN
    plan = _fake_plan(13)
    N2 = 2 << 13
    # 2 digits, groups of 4 keys: 8 sum polynomials do not fit the 3 spare ext slots of 2 digits -> an explicit workspace
    need = lib.lf_rotate_hoisted_ws_words(ctypes.byref(plan))
    assert need == 2 * 4 * 3 << 13
    assert lib.lf_rotate_hoisted_ws_words(ctypes.byref(_fake_plan(13, 1))) == 2 * 3 << 13
    assert call(plan, 0, [3]) == LF_ERR_ARG
    assert call(plan, 1, None) == LF_ERR_ARG
    assert call(plan, 2, [3, 4], ws=dummy, ws_words=need) == LF_ERR_ARG            # even exponent
    assert call(plan, 1, [N2 + 1], ws=dummy, ws_words=need) == LF_ERR_ARG          # >= 2N
    assert call(plan, 1, [-3], ws=dummy, ws_words=need) == LF_ERR_ARG
    assert call(plan, 1, [3]) == LF_ERR_ARG                                       # no workspace where one is needed
    assert call(plan, 1, [3], ws=dummy, ws_words=need - 1) == LF_ERR_ARG
    nul = (ctypes.c_void_p * 4)(64, None, 64, 64)
    assert call(plan, 2, [3, 5], keys=nul, ws=dummy, ws_words=need) == LF_ERR_ARG  # a NULL key
    assert call(plan, 2, [3, 5], out1=nul, ws=dummy, ws_words=need) == LF_ERR_ARG
    assert lib.lf_rotate_hoisted(ctypes.byref(plan), None, dummy, 1, (ctypes.c_int64 * 1)(3), 1, arr, 0, 0, 0, 0, dummy, need,
                                 arr, arr, None) == LF_ERR_ARG
    assert lib.lf_rotate_hoisted(None, dummy, dummy, 1, (ctypes.c_int64 * 1)(3), 1, arr, 0, 0, 0, 0, dummy, need, arr, arr,
                                 None) == LF_ERR_ARG


def test_hoisted_inner_product_kernels_use_no_scratch():
    """Every instantiation of the new inner product (1, 2, 4 keys x raw / planes key x raw / planes digits) exists with
    scratch 0 and the occupancy its plain 256-thread launch gets from the registers: 8 waves per SIMD for one key, at least 5 for
    two, 3 for four (136 VGPRs: pinning 4 waves spills); and the tracked table lists them as built."""
    import __graft_entry__ as g
    rows = [r for r in g.kernel_resources() if r["kernel"].startswith("ks_inner_hoist_kernel<")]
    by = {r["kernel"]: r for r in rows}
    floor = {1: 8, 2: 5, 4: 3}
    for nr in (1, 2, 4):
        for pl in ("true", "false"):
            for dpl in ("true", "false"):
                k = f"ks_inner_hoist_kernel<{nr}, {pl}, {dpl}>"
                assert k in by, k
                assert by[k]["scratch"] == 0 and by[k]["vgpr_spill"] == 0, by[k]
                assert by[k]["occupancy"] >= floor[nr], by[k]
    tracked = open(os.path.join(ROOT, "profiles", "r06_kernel_resources.txt")).read()
    for k, r in by.items():
        line = next(ln for ln in tracked.splitlines() if ln[18:76].strip() == k)
        f = line.split()
        assert (int(f[-7]), int(f[-3]), int(f[-1])) == (r["vgprs"], r["scratch"], r["occupancy"]), line
