"""Transforms at the ring degrees above the engine's (logN 18 up to lf_limits(LF_LIMIT_LOGN) = 24), against the CPU oracle.

The C ABI and the reference-shaped ntt_cuda shim accept these sizes, but the engine stops at 17, and so did the rest of the
suite.  Above 17 a transform takes a path of its own (csrc/ckks_ntt.hip: ntt_forward / intt_impl): the column pass has
S1 = logN - 12 = 6 .. 12 stages and runs in the generic LDS-tiled strided kernels — forward ntt_fwd_pass_mixed<RLX> (stacks
of both arithmetic classes) or ntt_fwd_pass<DP, RLX> (one class), inverse ntt_inv_pass_mixed<RLX> / ntt_inv_pass_io<DP, RLX>
— with tiles of 2^(12 - S1) columns: 64 at logN 18, 2 at 23, ONE at 24.  The contiguous 12-stage pass is the 16-words-per-thread
one (ckks_ntt_tile16.h).  lf_ntt_ws / lf_intt_ws ignore their workspace, lf_rescale_ntt runs lf_rescale_batch and then a plain
transform.

Every stack holds the edge primes of tests/helpers.py:pick_edge_primes (the top of the fp64 class below 2^41, the bottom of
the integer class above it, a small fp64-class prime — about 2^27 at logN 24, where q = 1 mod 2^25 — and a 60-bit prime),
as a mixed stack, as its fp64-class rows only and as its integer-class rows only.  At 2^24 one row is 128 MiB: stacks stay at
4 rows and 2 polynomials, and each limb set is built once per module."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests.helpers import SMALL_PRIME_LIMIT, Limbs, edge_operand, pick_edge_primes
from tests.test_class_edges_gpu import (LF_NTT_PLAIN, LF_NTT_RELAXED, Setup, _mod_rows, check_relaxed_forward,
                                        check_relaxed_inverse, dev)
from tests.test_ntt_cuda_gpu import signed_inputs

pytestmark = pytest.mark.gpu

LF_LIMIT_LOGN = 4
TOP = 0    # a size of 0 or below: that many below lf_limits(LF_LIMIT_LOGN)
MIXED, DP_ONLY, INT_ONLY = (0, 1, 2, 3), (0, 2), (1, 3)   # rows of pick_edge_primes(logN, 1, 1, 1, 1): fp64, int, fp64, int
STACKS = {"mixed": MIXED, "fp64": DP_ONLY, "int": INT_ONLY}
TAILS = ("intt", "intt_exit", "intt_exit_reduce", "intt_exit_reduce_signed")


def size(spec):
    from liberate_fhe_amd._native import lib
    return spec if spec > 0 else lib.lf_limits(LF_LIMIT_LOGN) + spec


@functools.lru_cache(maxsize=None)
def limbs(logN):
    lim = Limbs(logN, pick_edge_primes(logN, 1, 1, 1, 1))
    assert [q < SMALL_PRIME_LIMIT for q in lim.q] == [True, False, True, False]
    lim.mont_tables()
    lim.psi_plain = lim.ipsi_plain = None    # only mont_tables() reads them: 2 x 512 MiB at logN 24
    return lim


_setups = {}


def setup(logN, rows=MIXED):
    """Setup (test_class_edges_gpu.py) of the rows `rows` of the ring's limb set; one ring's tables on the device at a time."""
    if any(k[0] != logN for k in _setups):
        _setups.clear()
        torch.cuda.empty_cache()
    if (logN, rows) not in _setups:
        lim = limbs(logN)
        _setups[(logN, rows)] = Setup(lim if rows == MIXED else lim.select(rows))
    return _setups[(logN, rows)]


@pytest.fixture(scope="module", autouse=True)
def _release_rings():
    """The tables of 2^24 rings are gigabytes on the host and the device: gone before the next module runs."""
    yield
    _setups.clear()
    limbs.cache_clear()
    torch.cuda.empty_cache()


def sub(x, rows):
    return np.ascontiguousarray(x[:, list(rows)])


def oracle_tails(s, x):
    """The oracle's four inverse chains of every polynomial of x, one after the other (tail t is tail t - 1 plus one step)."""
    from oracle import oracle as orc
    lim = s.lim
    y = np.ascontiguousarray(x).copy()
    for b in range(y.shape[0]):
        orc.intt(y[b], s.ipsi_np, lim.Ninv, lim.rows, lim.logN, lim._2q, *lim.mont_args())
    yield 0, y
    for b in range(y.shape[0]):
        orc.mont_redc(y[b], lim.rows, *lim.mont_args())
    yield 1, y
    for b in range(y.shape[0]):
        orc.reduce_2q(y[b], lim.rows, lim._2q)
    yield 2, y
    for b in range(y.shape[0]):
        orc.make_signed(y[b], lim.rows, lim._2q)
    yield 3, y


def test_transform_limit_is_two_to_the_24():
    """The sizes below follow lf_limits(LF_LIMIT_LOGN); today that is 24 = 2 * NTT_TILE_LOG_MAX, where the column pass of the
    logN 24 transform has ONE column per tile."""
    from liberate_fhe_amd._native import lib
    assert lib.lf_limits(LF_LIMIT_LOGN) == 24 == size(TOP)
    assert [size(s) for s in (18, 20, TOP - 1, TOP)] == [18, 20, 23, 24]


@pytest.mark.parametrize("spec", [18, 20, TOP - 1, TOP], ids=["18", "20", "top-1", "top"])
def test_exact_transforms_above_17(spec):
    """lf_ntt, enter_ntt (Rs), and lf_intt with the four tails on a batch of two (the largest differences in every butterfly:
    2q - 1 and 0 by the Thue-Morse parity; random lazy words): bit-exact against the oracle on the mixed stack (the _mixed pass
    kernels) and on its fp64-class and integer-class rows alone (the per-class kernels), and the round trip is the identity."""
    logN = size(spec)
    s = setup(logN)
    x = np.stack([edge_operand(s.lim, "2q-1|0", 1), edge_operand(s.lim, "lazy", 2 + logN)])
    cases = [(name, rows, setup(logN, rows)) for name, rows in STACKS.items()]
    want = np.stack([s.o_ntt(p) for p in x])
    for name, rows, st in cases:
        assert (st.ntt(sub(x, rows)) == sub(want, rows)).all(), f"ntt, {name} stack"
    want = np.stack([s.o_ntt(p, enter=True) for p in x])
    for name, rows, st in cases:
        assert (st.ntt(sub(x, rows), Rs=st.Rs) == sub(want, rows)).all(), f"enter_ntt, {name} stack"
    del want
    for tail, want in oracle_tails(s, x):
        for name, rows, st in cases:
            assert (st.intt(sub(x, rows), tail) == sub(want, rows)).all(), f"{TAILS[tail]}, {name} stack"
    del want
    xc = s.lim.uniform(3 + logN)[None]
    for name, rows, st in cases:
        f = st.ntt(sub(xc, rows), Rs=st.Rs)
        assert (st.intt(f, 2) == sub(xc, rows)).all(), f"round trip, {name} stack"


@pytest.mark.parametrize("spec", [18, TOP], ids=["18", "top"])
def test_shim_transforms_above_17(spec):
    """The reference-shaped ntt_cuda shim takes logN from the tensor: at logN 18 with the reference's [rows, logN, N/2]
    per-stage tables (all six transform entries against the oracle), at the top size with compact tables."""
    from liberate_fhe_amd.fhe.context.ckks_context import stage_butterfly_indices
    from liberate_fhe_amd.ntt import ntt_cuda as nc
    logN = size(spec)
    s = setup(logN)
    lim = s.lim
    d = lambda v: [dev(v)]
    consts = [d(lim._2q), d(lim.ql), d(lim.qh), d(lim.kl), d(lim.kh)]
    if logN == 18:
        ev, od, tw = stage_butterfly_indices(logN, inverse=False)
        iev, iod, itw = stage_butterfly_indices(logN, inverse=True)
        fwd = (d(ev), d(od), d(np.ascontiguousarray(s.psi_np[:, tw])))
        inv = (d(iev), d(iod), d(np.ascontiguousarray(s.ipsi_np[:, itw])))
    else:
        fwd, inv = ([None], [None], d(s.psi_np)), ([None], [None], d(s.ipsi_np))
    x = lim.uniform(5 + logN, lazy=True)
    t = d(x)
    nc.ntt(t, *fwd, *consts)
    assert (t[0].cpu().numpy() == s.o_ntt(x)).all(), "ntt"
    xc = lim.uniform(6 + logN)
    e = d(xc)
    nc.enter_ntt(e, d(lim.Rs), *fwd, *consts)
    fe = e[0].cpu().numpy()
    assert (fe == s.o_ntt(xc, enter=True)).all(), "enter_ntt"
    for tail, want in oracle_tails(s, fe[None]):
        t = d(fe)
        getattr(nc, TAILS[tail])(t, *inv, d(lim.Ninv), *consts)
        assert (t[0].cpu().numpy() == want[0]).all(), TAILS[tail]
        if tail == 2:
            assert (want[0] == xc).all(), "round trip"


def sprinkled(lim, seed):
    """Lazy words with a few out-of-range ones (negative, 2q, 2q + 1) in a few tiles of either pass — the word N - 1 in the last
    tile — next to tiles without any."""
    x = lim.uniform(seed, lazy=True)
    N = lim.N
    for r, q in enumerate(lim.q):
        x[r, 5] = -(q - 3)
        x[r, N - 1] = 2 * q + 1
        x[r, N // 2 + 4096 * 3 + 7] = 2 * q
        x[r, 4096 + 513 + r] = -1
    return x


@pytest.mark.parametrize("spec", [18, TOP], ids=["18", "top"])
def test_out_of_range_words_above_17(spec):
    """Signed and lazy words, boundary words included (test_ntt_cuda_gpu.py:signed_inputs: every tile holds some), and lazy
    words with a few out-of-range ones: an fp64-class tile of the strided pass that holds one leaves the fp64 form for the signed
    integer routine.  Forward (ntt, enter_ntt) and the four inverse chains, bit-exact against the oracle, on the mixed stack and
    on the fp64-class rows alone."""
    logN = size(spec)
    s = setup(logN)
    x = np.stack([signed_inputs(s.lim, 30 + logN), sprinkled(s.lim, 31 + logN)])
    cases = [(name, rows, setup(logN, rows)) for name, rows in (("mixed", MIXED), ("fp64", DP_ONLY))]
    for enter in (False, True):
        want = np.stack([s.o_ntt(p, enter=enter) for p in x])
        for name, rows, st in cases:
            got = st.ntt(sub(x, rows), Rs=st.Rs if enter else None)
            assert (got == sub(want, rows)).all(), f"{'enter_ntt' if enter else 'ntt'}, {name} stack"
    del want
    for tail, want in oracle_tails(s, x):
        for name, rows, st in cases:
            assert (st.intt(sub(x, rows), tail) == sub(want, rows)).all(), f"{TAILS[tail]}, {name} stack"


@pytest.mark.parametrize("spec", [18, TOP], ids=["18", "top"])
def test_workspace_entries_above_17(spec):
    """lf_ntt_ws / lf_intt_ws ignore the workspace above logN 17: with one they equal lf_ntt / lf_intt and the oracle."""
    logN = size(spec)
    s = setup(logN)
    x = sprinkled(s.lim, 40 + logN)[None]
    want = s.o_ntt(x[0], enter=True)
    assert (s.ntt(x, Rs=s.Rs, ws=True)[0] == want).all(), "enter_ntt through lf_ntt_ws"
    assert (s.ntt(x, Rs=s.Rs)[0] == want).all(), "enter_ntt through lf_ntt"
    for tail, want in oracle_tails(s, x):
        if tail in (0, 3):
            assert (s.intt(x, tail, ws=True) == want).all(), f"{TAILS[tail]} through lf_intt_ws"
            assert (s.intt(x, tail) == want).all(), f"{TAILS[tail]} through lf_intt"


@pytest.mark.parametrize("spec", [18, TOP], ids=["18", "top"])
def test_relaxed_forward_above_17(spec):
    """test_class_edges_gpu.py:test_relaxed_forward_on_signed_lazy_words at the large ring degrees: signed-lazy words at
    +-(2q - 1) and random ones in (-2q, 2q)."""
    logN = size(spec)
    s = setup(logN)
    names = ("2q-1", "lazy")
    check_relaxed_forward(s, np.stack([edge_operand(s.lim, p, 50 + logN, signed=True) for p in names]), names)


@pytest.mark.parametrize("spec", [18, TOP], ids=["18", "top"])
def test_relaxed_inverse_above_17(spec):
    """test_class_edges_gpu.py:test_relaxed_inverse_at_the_documented_input_bound at the large ring degrees, whose column pass
    has up to 12 stages (the 2^46 bound was derived when it had at most 5): words at the bound alternating with 0, random ones."""
    logN = size(spec)
    check_relaxed_inverse(setup(logN), seed=logN, kinds=(1, 2))


def _arr(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


@pytest.mark.parametrize("spec", [18, TOP], ids=["18", "top"])
@pytest.mark.parametrize("flags", [0, 1, 3])
def test_rescale_ntt_above_17(spec, flags):
    """lf_rescale_ntt (lf_rescale_batch, then the transform, above 17) against the oracle's rescale — REDC((in - row0) * scale)
    + [row0 > round_at], reduced — followed by the oracle's enter_ntt: exact (flags 0) word for word, relaxed (1) and
    relaxed + plain (3: fp64-class rows skip Rs) as canonical residues."""
    from liberate_fhe_amd._native import lib, check
    from oracle import oracle as orc
    logN = size(spec)
    s = setup(logN)
    lim = s.lim
    rows, N, count = lim.rows, lim.N, 2
    rng = np.random.default_rng(logN * 10 + flags)
    q_drop = (1 << 41) - 65535
    src = [np.stack([rng.integers(0, int(x), size=N, dtype=np.int64) for x in lim.q]) for _ in range(count)]
    src[0][:, ::5] = s.q_host[:, None] - 1
    row0 = [rng.integers(0, q_drop, size=N, dtype=np.int64) for _ in range(count)]
    row0[1][::3] = q_drop - 1
    scales = np.array([rng.integers(1, int(x)) for x in lim.q], dtype=np.int64)
    round_at = q_drop // 2
    srcs, row0s, dscales = [dev(v) for v in src], [dev(v) for v in row0], dev(scales)
    got = torch.full((count, rows, N), -1, dtype=torch.int64, device="cuda")
    check(lib.lf_rescale_ntt(_arr(srcs), _arr(row0s), count, got.data_ptr(), rows, logN, dscales.data_ptr(), round_at,
                             s.psi.data_ptr(), s.dp, s.q_host.ctypes.data, s.Rs.data_ptr(), flags, s.q2.data_ptr(), *s.cp,
                             0, s.st), "rescale_ntt")
    got = got.cpu().numpy()
    small = s.q_host < SMALL_PRIME_LIMIT
    for i in range(count):
        r = np.ascontiguousarray(src[i] - row0[i][None, :])
        orc.mont_enter(r, scales, rows, *lim.mont_args())
        r += (row0[i] > round_at).astype(np.int64)[None, :]
        orc.reduce_2q(r, rows, lim._2q)
        want = s.o_ntt(r, enter=True)
        if flags == 0:
            assert (got[i] == want).all(), f"polynomial {i}"
            continue
        if flags & LF_NTT_PLAIN:
            want = np.where(small[:, None], s.o_ntt(r), want)
        assert ((got[i] >= 0) & (got[i] < s.q_host[:, None])).all(), f"polynomial {i}: canonical words"
        assert (got[i] == _mod_rows(want, s.q_host)).all(), f"polynomial {i}"


@pytest.mark.parametrize("spec", [18, TOP], ids=["18", "top"])
def test_intt_mul_above_17(spec):
    """lf_intt_mul (the product formed as the tiled inverse pass loads its tiles; LF_NTT_RELAXED | LF_NTT_PLAIN as cc_mult calls
    it) with tails 2 and 3: the oracle's element-wise product — plain on fp64-class rows, REDC62 on the others — followed by the
    oracle's inverse chain (N^-1 plain on the fp64-class rows)."""
    from liberate_fhe_amd._native import lib, check
    from oracle import oracle as orc
    logN = size(spec)
    s = setup(logN)
    lim = s.lim
    rows, N = lim.rows, lim.N
    a = np.stack([lim.uniform(60 + logN), lim.uniform(61 + logN)])
    b = np.stack([lim.uniform(62 + logN), lim.uniform(63 + logN)])
    a[0][:, ::7] = s.q_host[:, None] - 1
    b[0][:, ::3] = s.q_host[:, None] - 1
    small = s.q_host < SMALL_PRIME_LIMIT
    want = np.empty_like(a)
    for p in range(2):
        y_int = np.empty_like(a[p])
        orc.mont_mult(a[p], b[p], y_int, rows, *lim.mont_args())
        be = b[p].copy()
        orc.mont_enter(be, lim.Rs, rows, *lim.mont_args())           # b R: the Montgomery product with a is the plain product
        y_dp = np.empty_like(a[p])
        orc.mont_mult(a[p], be, y_dp, rows, *lim.mont_args())
        z_dp = s.o_intt(y_dp, 2)                                     # N^-1 R^-1 intt(a b)
        orc.mont_enter(z_dp, lim.Rs, rows, *lim.mont_args())        # N^-1 intt(a b): PLAIN
        want[p] = np.where(small[:, None], z_dp % s.q_host[:, None], s.o_intt(y_int, 2))
    da, db = dev(a), dev(b)
    for tail in (2, 3):
        if tail == 3:
            for p in range(2):
                orc.make_signed(want[p], rows, lim._2q)
        dst = torch.full((2, rows, N), -1, dtype=torch.int64, device="cuda")
        check(lib.lf_intt_mul(dst.data_ptr(), da.data_ptr(), rows * N, db.data_ptr(), rows * N, 2, rows, logN, s.ipsi.data_ptr(),
                              s.idp, s.q_host.ctypes.data, s.Ninv.data_ptr(), tail, LF_NTT_RELAXED | LF_NTT_PLAIN, *s.cp, 0, s.st),
              "intt_mul")
        assert (dst.cpu().numpy() == want).all(), f"tail {tail}"


def _primes30_for(logN):
    """30-bit word mode primes of the ring: pick_primes30 where it finds three distinct ones below 2^28, else every NTT prime
    below 2^28 (at logN 24, where q = 1 mod 2^25, that is 5 * 2^25 + 1 alone)."""
    from liberate_fhe_amd.fhe.context import primes as P
    from tests.helpers import pick_primes30
    got = pick_primes30(logN, 2, 1)
    if len(set(got)) == 3 and max(got) < (1 << 28):
        return got
    M = 2 << logN
    return [k * M + 1 for k in range(1, (1 << 28) // M) if P.is_prime(k * M + 1)]


@pytest.mark.parametrize("spec", [18, 20, TOP], ids=["18", "20", "top"])
def test_w30_transforms_above_17(spec):
    """The 30-bit / int32 word mode (lf30_ntt / lf30_intt through the shim): ntt, enter_ntt and the four inverse chains against
    the oracle's int32 build."""
    from liberate_fhe_amd.ntt import ntt_cuda as nc
    from oracle import oracle as orc
    logN = size(spec)
    primes = _primes30_for(logN)
    assert primes and max(primes) < (1 << 28)
    lim = Limbs(logN, primes, bits=30)
    psi, ipsi = lim.mont_tables()
    d = lambda v: [dev(v)]
    consts = [d(lim._2q), d(lim.ql), d(lim.qh), d(lim.kl), d(lim.kh)]
    x = lim.uniform(70 + logN, lazy=True)
    for enter in (False, True):
        want = x.copy()
        if enter:
            orc.mont_enter(want, lim.Rs, lim.rows, *lim.mont_args())
        orc.ntt(want, psi, lim.rows, logN, lim._2q, *lim.mont_args())
        t = d(x)
        if enter:
            nc.enter_ntt(t, d(lim.Rs), [None], [None], d(psi), *consts)
        else:
            nc.ntt(t, [None], [None], d(psi), *consts)
        assert (t[0].cpu().numpy() == want).all(), "enter_ntt" if enter else "ntt"
    want = x.copy()
    orc.intt(want, ipsi, lim.Ninv, lim.rows, logN, lim._2q, *lim.mont_args())
    for tail, name in enumerate(TAILS):
        if tail == 1:
            orc.mont_redc(want, lim.rows, *lim.mont_args())
        elif tail == 2:
            orc.reduce_2q(want, lim.rows, lim._2q)
        elif tail == 3:
            orc.make_signed(want, lim.rows, lim._2q)
        t = d(x)
        getattr(nc, name)(t, [None], [None], d(ipsi), d(lim.Ninv), *consts)
        assert (t[0].cpu().numpy() == want).all(), name
