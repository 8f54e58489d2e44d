"""Linear transforms (ckks_engine.linear_transform / encode_diagonals, lf_linear_transform, encdec.matrix_diagonals) without a GPU:
the engine's host logic on the checker backend against the composition of public steps that defines the words, the refusals, the
round trips of the encoded diagonals, the sharded ranks, the C entry's argument checks and the new kernel's resources."""
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
STEPS = (0, 1, 2, 5, 11, 700)


def words(ct):
    return [torch.cat([t.cpu() for t in comp]) for comp in ct.data]


def keys_for(eng, steps=STEPS):
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


def composition(eng, ct, diags, keys):
    """The definition of the op's words from the engine's public steps on one device (the issue's section 2): c0, c1 canonical;
    E = per part pre_extend(c1) -> extend -> exact forward NTT; c^ = enter_ntt(c) * P on the ordinary rows; per key the parts of E
    gathered by pi_p times the key part, summed, + c^0 gathered on the ordinary rows (step 0: c^, zero on the special rows);
    S_c = sum pt * t_c; intt_exit_reduce, mod-down without addend, the engine's rescale."""
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
    S = [None, None]
    for j, step in enumerate(eng.diagonal_steps(diags)):
        if step == 0:
            t = [torch.cat([chat[comp], torch.zeros((K, N), dtype=torch.int64)]) for comp in range(2)]
        else:
            idx = torch.from_numpy(encdec.ntt_galois_index(logN, encdec.galois_exponent(N, step)))
            t = None
            for part_id, ext in enumerate(E):
                g = ext[:, idx].contiguous()
                part = keys[step].data[eng.parts_alloc[level][d][part_id]].data
                prod = [eng.ntt.mont_mult([g], [part[comp][0][start:]], level, d, -2)[0] for comp in range(2)]
                t = prod if t is None else [eng.ntt.mont_add([t[comp]], [prod[comp]], level, d, -2)[0] for comp in range(2)]
            folded = eng.ntt.mont_add([t[0][:ell].contiguous()], [chat[0][:, idx].contiguous()], level, d, -1)[0]
            t[0] = torch.cat([folded, t[0][ell:]])
        for comp in range(2):
            prod = eng.ntt.mont_mult([diags.data[j][0]], [t[comp]], level, d, -2)[0]
            S[comp] = prod if S[comp] is None else eng.ntt.mont_add([S[comp]], [prod], level, d, -2)[0]
    s = torch.stack(S).contiguous()
    eng.ntt.intt_exit_reduce([s[0]], level, d, -2)
    eng.ntt.intt_exit_reduce([s[1]], level, d, -2)
    out = torch.empty((2, ell, N), dtype=torch.int64)
    tabs = eng._ks_tables(level)
    eng.backend.ks_moddown_batch([s[0], s[1]], [out[0], out[1]], [None, None], ell, K, tabs[("pir", d)],
                                 eng._vec("Rs", d, level, True), eng._consts(d, level, True), PiP=None, galois=None)
    return eng.rescale(eng._new(([out[0]], [out[1]]), ct.origin, level=level))


@pytest.fixture(scope="module")
def checker():
    from liberate_fhe_amd.fhe import ckks_engine
    from tests.oracle_backend import OracleBackend
    eng = ckks_engine(devices=["cpu"], backend=OracleBackend(), **LT)
    return eng, keys_for(eng)


@pytest.mark.parametrize("level", [0, 2])
def test_checker_linear_transform_equals_the_composition(checker, level):
    eng, keys = checker
    ct = lazy_ciphertext(eng, 90 + level, level)
    for steps in ((1,), (0,), (0, 1), (1, 2, 5), (0, 1, 2, 5, 11, 700)):
        diags = synth.diagonals(eng, 7 + level, level, steps)
        got = eng.linear_transform(ct, diags, keys)
        want = composition(eng, ct, diags, keys)
        assert got.level == level + 1 and got.origin == ct.origin and not got.ntt_state and not got.include_special
        gw, ww = words(got), words(want)
        assert gw[0].shape == ww[0].shape
        assert torch.equal(gw[0], ww[0]) and torch.equal(gw[1], ww[1]), (level, steps)
    # a list of keys serves as well as a mapping, in any order
    diags = synth.diagonals(eng, 3, level, (1, 5))
    a = eng.linear_transform(ct, diags, keys)
    b = eng.linear_transform(ct, diags, [keys[5], keys[700], keys[1]])
    assert all(torch.equal(x, y) for x, y in zip(words(a), words(b)))


def test_refusals_and_round_trips_of_the_encoded_diagonals(checker, tmp_path):
    from liberate_fhe_amd.fhe.presets import errors
    eng, keys = checker
    ct = synth.ciphertext(eng, 95, 0)
    diags = synth.diagonals(eng, 4, 0, (0, 1, 5))
    top = eng.num_levels - 1
    with pytest.raises(errors.NotMatchType):                       # a missing key
        eng.linear_transform(ct, diags, [keys[1]])
    with pytest.raises(errors.NotMatchType):                       # a key of another kind
        eng.linear_transform(ct, diags, [keys[1], synth.key_switch_key(eng, 8)])
    with pytest.raises(errors.NotMatchType):                       # not a ciphertext
        eng.linear_transform(keys[1], diags, keys)
    with pytest.raises(errors.NotMatchType):                       # not an encode_diagonals object
        eng.linear_transform(ct, ct, keys)
    with pytest.raises(errors.NotMatchDataStructState):            # diagonals of another level
        eng.linear_transform(synth.ciphertext(eng, 95, 1), diags, keys)
    with pytest.raises(errors.MaximumLevelError):                  # no level left to rescale into (rescale's error)
        eng.linear_transform(synth.ciphertext(eng, 95, top), diags, keys)
    with pytest.raises(errors.MaximumLevelError):
        eng.encode_diagonals({0: [1.0]}, top)
    with pytest.raises(NotImplementedError):
        eng.linear_transform(eng._new(ct.data, ct.origin, level=0, ntt_state=True), diags, keys)
    with pytest.raises(NotImplementedError):
        eng.linear_transform(eng._new(ct.data, ct.origin, level=0, include_special=True), diags, keys)
    with pytest.raises(Exception):                                 # longer than num_slots: refused as padding refuses it
        eng.encode_diagonals({1: np.ones(eng.num_slots + 1)}, 0)
    with pytest.raises(ValueError):                                # the same step twice after reduction mod num_slots
        eng.encode_diagonals({1: [1.0], 1 + eng.num_slots: [2.0]}, 0)
    # step 0 alone needs no key at all
    only0 = synth.diagonals(eng, 4, 0, (0,))
    assert eng.linear_transform(ct, only0, []).level == 1

    # encode_diagonals: shapes, flags, the steps in the origin (reduced mod num_slots, ascending), views of one pack
    np.random.seed(3)
    enc = eng.encode_diagonals({5: eng.example(-1, 1), 0: [0.5, -0.25], eng.num_slots + 700: eng.example(-1, 1)[:100], 1: 2.0}, 2)
    assert enc.origin == "plain diagonals:0,1,5,700" and eng.diagonal_steps(enc) == [0, 1, 5, 700]
    assert (enc.level, enc.ntt_state, enc.montgomery_state, enc.include_special) == (2, True, True, True)
    rows = eng._rows(0, 2, True)
    assert all(len(row) == 1 and row[0].shape == (rows, eng.ctx.N) for row in enc.data)
    assert all(enc.data[j][0].data_ptr() == enc.data[0][0].data_ptr() + j * rows * eng.ctx.N * 8 for j in range(4))
    # cpu() and save -> load keep the words and the steps; the loaded object (no shared pack any more) transforms alike
    host = eng.cpu(enc)
    path = str(tmp_path / "diags.pkl")
    eng.save(enc, path)
    back = eng.load(path)
    for other in (host, back):
        assert other.origin == enc.origin and other.level == enc.level and other.include_special
        assert len(other.data) == len(enc.data)
    for j in range(4):
        assert torch.equal(back.data[j][0], enc.data[j][0])
    nat = eng._dest_rows(2, True)[0]
    for j in range(4):
        assert torch.equal(host.data[j][0][nat], enc.data[j][0])
    ct2 = synth.ciphertext(eng, 96, 2)
    a, b = eng.linear_transform(ct2, enc, keys), eng.linear_transform(ct2, back, keys)
    assert all(torch.equal(x, y) for x, y in zip(words(a), words(b)))
    # a plain mapping is encoded on the fly at the ciphertext's level
    assert eng.linear_transform(ct2, {0: [1.0], 1: [0.5, 0.5]}, keys).level == 3


def test_matrix_diagonals():
    rng = np.random.default_rng(11)
    n = 256
    steps = (0, 1, 2, 254, 255)
    M = np.zeros((n, n), dtype=np.complex128)
    i = np.arange(n)
    for s in steps:
        M[i, (i - s) % n] = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    dg = encdec.matrix_diagonals(M)
    assert sorted(dg) == sorted(steps)
    v = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    got = sum(dg[s] * np.roll(v, s) for s in dg)
    want = M @ v
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    with pytest.raises(ValueError):
        encdec.matrix_diagonals(np.zeros((4, 5)))
    with pytest.raises(ValueError):
        encdec.matrix_diagonals(np.zeros(4))


GLOO_STEPS = (0, 1, 4, 9)


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
    ct = synth.ciphertext(eng, 3, 0)
    r = eng.linear_transform(ct, synth.diagonals(eng, 5, 0, GLOO_STEPS), keys_for(eng, GLOO_STEPS))
    for comp in range(2):
        np.save(os.path.join(outdir, f"{comp}.{rank}.npy"), r.data[comp][0].numpy() if r.data[comp] else
                np.zeros((0, eng.ctx.N), dtype=np.int64))
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_ranks_equal_one_process():
    """gloo world 2, one process per rank (the orchestrated path with the digit exchange and the rescale's row exchange): every
    rank's rows equal the single-process result on two devices."""
    from liberate_fhe_amd.fhe import ckks_engine
    from tests.oracle_backend import OracleBackend
    world = 2
    port = 35500 + (os.getpid() % 2000)
    with tempfile.TemporaryDirectory() as outdir:
        mp.spawn(_worker, args=(world, port, outdir), nprocs=world, join=True)
        got = {(c, r): np.load(os.path.join(outdir, f"{c}.{r}.npy")) for c in range(2) for r in range(world)}
    eng = ckks_engine(devices=["cpu"] * world, backend=OracleBackend(), **LT)
    ct = synth.ciphertext(eng, 3, 0)
    want = eng.linear_transform(ct, synth.diagonals(eng, 5, 0, GLOO_STEPS), keys_for(eng, GLOO_STEPS))
    assert want.level == 1
    for c in range(2):
        for r in range(world):
            w = want.data[c][r].numpy() if r < len(want.data[c]) else np.zeros((0, eng.ctx.N), dtype=np.int64)
            assert got[(c, r)].shape == w.shape and (got[(c, r)] == w).all(), (c, r)


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
    """lf_linear_transform returns LF_ERR_ARG from its arguments alone (pointers that are never dereferenced; no call here would
    pass the checks): nr < 0, nr == 0 without pt0, a NULL pt / key / output / exponent array / rescale table, an even exponent or
    one outside (0, 2N), a workspace smaller than lf_linear_transform_ws_words says, a level with one limb, plans at logN 12 and
    18, a NULL plan."""
    from liberate_fhe_amd._native import lib
    LF_ERR_ARG = 10001
    dummy = ctypes.c_void_p(64)
    arr = (ctypes.c_void_p * 4)(64, 64, 64, 64)
    stride = 3 << 13

    def call(plan, nr, exps, keys=arr, pt=dummy, pt0=None, ws=None, ws_words=0, out0=dummy, out1=dummy, c0=dummy, scales=dummy):
        e = (ctypes.c_int64 * max(1, len(exps)))(*exps) if exps is not None else None
        return lib.lf_linear_transform(ctypes.byref(plan) if plan is not None else None, c0, dummy, nr, e, keys, 0, 0, 0, 0, pt, stride,
                                       pt0, scales, 0, ws, ws_words, out0, out1, None)

    for logN in (12, 18):
        plan = _fake_plan(logN)
        assert lib.lf_linear_transform_ws_words(ctypes.byref(plan)) == 0
        assert call(plan, 1, [3]) == LF_ERR_ARG, logN
    assert call(None, 1, [3]) == LF_ERR_ARG
    plan = _fake_plan(13)
    N2 = 2 << 13
    assert lib.lf_linear_transform_ws_words(ctypes.byref(plan)) == 0          # the plan's operand stack serves
    assert call(plan, -1, [3]) == LF_ERR_ARG
    assert call(plan, 0, [3]) == LF_ERR_ARG                                   # no key and no step-0 diagonal
    assert call(plan, 1, None) == LF_ERR_ARG
    assert call(plan, 1, [3], keys=None) == LF_ERR_ARG
    assert call(plan, 1, [3], pt=None) == LF_ERR_ARG
    assert call(plan, 1, [3], out0=None) == LF_ERR_ARG
    assert call(plan, 1, [3], out1=None) == LF_ERR_ARG
    assert call(plan, 1, [3], c0=None) == LF_ERR_ARG
    assert call(plan, 1, [3], scales=None) == LF_ERR_ARG
    assert call(plan, 2, [3, 4]) == LF_ERR_ARG                                # even exponent
    assert call(plan, 1, [N2 + 1]) == LF_ERR_ARG                              # >= 2N
    assert call(plan, 1, [-3]) == LF_ERR_ARG
    nul = (ctypes.c_void_p * 4)(64, None, 64, 64)
    assert call(plan, 2, [3, 5], keys=nul) == LF_ERR_ARG                      # a NULL key
    # without an operand stack in the plan: an explicit workspace of 4 ell N words
    bare = _fake_plan(13, x4=False)
    need = lib.lf_linear_transform_ws_words(ctypes.byref(bare))
    assert need == 4 * 2 << 13
    assert call(bare, 1, [3]) == LF_ERR_ARG
    assert call(bare, 1, [3], ws=dummy, ws_words=need - 1) == LF_ERR_ARG
    assert call(bare, 0, [3], pt0=dummy, ws=dummy, ws_words=need - 1) == LF_ERR_ARG
    one = _fake_plan(13)
    one.ell = 1                                                               # no level left to rescale into
    assert call(one, 1, [3]) == LF_ERR_ARG


def test_linear_transform_kernels_use_no_scratch():
    """Every instantiation of ks_inner_lt_kernel (1, 2, 4 keys x raw / planes key x raw / planes digits, and the keyless one
    of a lone step 0) exists with scratch 0, no spill and at least 3 waves per SIMD; the tracked table lists them as built."""
    import __graft_entry__ as g
    by = {r["kernel"]: r for r in g.kernel_resources() if r["kernel"].startswith("ks_inner_lt_kernel<")}
    want = [f"ks_inner_lt_kernel<{nr}, {pl}, {dpl}>" for nr in (1, 2, 4) for pl in ("true", "false") for dpl in ("true", "false")]
    want.append("ks_inner_lt_kernel<0, false, false>")
    assert sorted(by) == sorted(want)
    for k in want:
        assert by[k]["scratch"] == 0 and by[k]["vgpr_spill"] == 0, by[k]
        assert by[k]["occupancy"] >= 3, by[k]
    tracked = open(os.path.join(ROOT, "profiles", "r06_kernel_resources.txt")).read()
    for k, r in by.items():
        line = next(ln for ln in tracked.splitlines() if ln[18:76].strip() == k)
        f = line.split()
        assert (int(f[-7]), int(f[-3]), int(f[-1])) == (r["vgprs"], r["scratch"], r["occupancy"]), line
