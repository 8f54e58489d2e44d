"""Kernels at the edges of the two arithmetic classes (csrc/ckks_ntt_core.h: primes below SMALL_PRIME_LIMIT = 2^41 run on
fp64 FMA arithmetic, larger ones on 64-bit integers), against the CPU oracle.

The fp64 class is exact only because of bounds that tighten as q approaches 2^41 (the lazy-REDC fix window, dp_reduce's
|x| < 64 m, the 48-bit planes), so every case here runs on the primes right below and right above 2^41, interleaved row by
row, next to a ~2^20 prime and a 60-bit prime (tests/helpers.py:pick_edge_primes), on operands that reach the bounds
(tests/helpers.py:edge_operand)."""
import ctypes

import numpy as np
import pytest
import torch

from tests.helpers import (EDGE_PATTERNS, SMALL_PRIME_LIMIT, Limbs, edge_operand, pick_edge_primes, redc62, thue_morse)

pytestmark = pytest.mark.gpu

LF_NTT_RELAXED, LF_NTT_PLAIN, LF_NTT_PLANES = 1, 2, 16
LF_TUNE_WS_EXTRA_STAGE = 4
# include/ckks_hip.h: a relaxed inverse transform takes words below 2^46 on fp64-class limbs, lazy words on the others
RELAXED_INV_DP_BOUND = 1 << 46


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


class Setup:
    """Device copies of a limb set's constants and tables, and the calls of the C ABI on them."""

    def __init__(self, lim, psi=None, ipsi=None):
        from liberate_fhe_amd.ntt import twiddles
        self.lim = lim
        m_psi, m_ipsi = lim.mont_tables()
        self.psi_np = m_psi if psi is None else psi
        self.ipsi_np = m_ipsi if ipsi is None else ipsi
        self.c = [dev(v) for v in (lim.ql, lim.qh, lim.kl, lim.kh)]
        self.cp = [t.data_ptr() for t in self.c]
        self.psi, self.ipsi = dev(self.psi_np), dev(self.ipsi_np)
        self.q2, self.Ninv, self.Rs = dev(lim._2q), dev(lim.Ninv), dev(lim.Rs)
        self.st = torch.cuda.current_stream().cuda_stream
        self.dp = twiddles.dp_pointer(self.psi, *self.c, 0, self.st)
        self.idp = twiddles.dp_pointer(self.ipsi, *self.c, 0, self.st)
        self.q_host = np.array(lim.q, dtype=np.int64)

    def ntt(self, x, Rs=None, flags=0, ws=False):
        from liberate_fhe_amd._native import lib, check
        lim = self.lim
        t = dev(x)
        batch = t.size(0)
        rs = 0 if Rs is None else Rs.data_ptr()
        if ws:
            w = torch.full((lib.lf_ntt_ws_words(batch, lim.rows, lim.logN),), -1, dtype=torch.int64, device="cuda")
            check(lib.lf_ntt_ws(t.data_ptr(), w.data_ptr(), batch, lim.rows, lim.logN, self.psi.data_ptr(), self.dp,
                                self.q_host.ctypes.data, rs, flags, *self.cp, 0, self.st), "lf_ntt_ws")
        else:
            check(lib.lf_ntt(t.data_ptr(), batch, lim.rows, lim.logN, self.psi.data_ptr(), self.dp, self.q_host.ctypes.data, rs,
                             flags, self.q2.data_ptr(), *self.cp, 0, self.st), "lf_ntt")
        return t.cpu().numpy()

    def intt(self, x, tail, flags=0, ws=False):
        from liberate_fhe_amd._native import lib, check
        lim = self.lim
        t = dev(x)
        batch = t.size(0)
        if ws:
            w = torch.full((lib.lf_ntt_ws_words(batch, lim.rows, lim.logN),), -1, dtype=torch.int64, device="cuda")
            check(lib.lf_intt_ws(t.data_ptr(), w.data_ptr(), batch, lim.rows, lim.logN, self.ipsi.data_ptr(), self.idp,
                                 self.q_host.ctypes.data, self.Ninv.data_ptr(), tail, flags, *self.cp, 0, self.st), "lf_intt_ws")
        else:
            check(lib.lf_intt(t.data_ptr(), batch, lim.rows, lim.logN, self.ipsi.data_ptr(), self.idp, self.q_host.ctypes.data,
                              self.Ninv.data_ptr(), tail, flags, self.q2.data_ptr(), *self.cp, 0, self.st), "lf_intt")
        return t.cpu().numpy()

    # the oracle, one polynomial [rows, N] at a time
    def o_ntt(self, x, enter=False, Rs=None):
        from oracle import oracle as orc
        lim, y = self.lim, np.ascontiguousarray(x).copy()
        if enter:
            orc.mont_enter(y, lim.Rs if Rs is None else Rs, lim.rows, *lim.mont_args())
        orc.ntt(y, self.psi_np, lim.rows, lim.logN, lim._2q, *lim.mont_args())
        return y

    def o_intt(self, x, tail):
        from oracle import oracle as orc
        lim, y = self.lim, np.ascontiguousarray(x).copy()
        orc.intt(y, self.ipsi_np, lim.Ninv, lim.rows, lim.logN, lim._2q, *lim.mont_args())
        if tail >= 1:
            orc.mont_redc(y, lim.rows, *lim.mont_args())
        if tail >= 2:
            orc.reduce_2q(y, lim.rows, lim._2q)
        if tail >= 3:
            orc.make_signed(y, lim.rows, lim._2q)
        return y


def edge_limbs(logN):
    # logN 16 / 17: a few rows, the oracle side of the large rings is the expensive part
    return Limbs(logN, pick_edge_primes(logN) if logN <= 14 else pick_edge_primes(logN, 1, 1, 1, 1))


def edge_batch(lim, seed, signed=False):
    """[4, rows, N]: the four adversarial patterns as the four polynomials of one batch."""
    return np.stack([edge_operand(lim, p, seed + i, signed=signed) for i, p in enumerate(EDGE_PATTERNS)])


@pytest.mark.parametrize("logN", [12, 13, 14, 16, 17])
def test_exact_transforms_at_the_class_edges(logN):
    """lf_ntt (plain and with Rs = enter_ntt), lf_intt with the tails 0 .. 3, and lf_ntt_ws / lf_intt_ws with
    LF_TUNE_WS_EXTRA_STAGE 1 and 0: bit-exact against the oracle on the adversarial patterns, primes at both sides of 2^41."""
    from liberate_fhe_amd._native import lib
    lim = edge_limbs(logN)
    s = Setup(lim)
    x = edge_batch(lim, 10 + logN)
    assert lim.q[0] < SMALL_PRIME_LIMIT < lim.q[1] and lim.q[0] > SMALL_PRIME_LIMIT - (1 << 22)
    want_f = [s.o_ntt(p) for p in x]
    want_e = [s.o_ntt(p, enter=True) for p in x]
    want_i = [[s.o_intt(p, tail) for p in x] for tail in range(4)]
    forms = [(False, None)] + ([(True, 1), (True, 0)] if 13 <= logN <= 17 else [])
    old = lib.lf_tune(LF_TUNE_WS_EXTRA_STAGE, -1)
    try:
        for ws, extra in forms:
            if extra is not None:
                lib.lf_tune(LF_TUNE_WS_EXTRA_STAGE, extra)
            tag = f"ws={ws} extra={extra}"
            got = s.ntt(x, ws=ws)
            for b, p in enumerate(EDGE_PATTERNS):
                assert (got[b] == want_f[b]).all(), f"ntt {p} {tag}"
            got = s.ntt(x, Rs=s.Rs, ws=ws)
            for b, p in enumerate(EDGE_PATTERNS):
                assert (got[b] == want_e[b]).all(), f"enter_ntt {p} {tag}"
            for tail in range(4):
                got = s.intt(x, tail, ws=ws)
                for b, p in enumerate(EDGE_PATTERNS):
                    assert (got[b] == want_i[tail][b]).all(), f"intt tail {tail} {p} {tag}"
    finally:
        lib.lf_tune(LF_TUNE_WS_EXTRA_STAGE, old)


def _window_operands(q, W, count):
    """Up to `count` words A in [0, 2q) with REDC62(A W) = t0 + q for a canonical t0 in [2^21, 2^22): the lazy words the
    exact fp64 path has to rebuild with dp_lazy_fix near the top of its window (dp_below_fix_limit: t0 < 2^22).  Proven
    here with Python integers.  Such a word needs A W >= t0 2^62 >= 2^83, so one factor must be a lazy representative
    (>= q) and q must be near 2^41."""
    Winv = pow(W, -1, q)
    out = []
    for t0 in range((1 << 22) - 1, (1 << 21) - 1, -1):
        A = t0 * (1 << 62) * Winv % q
        for AA in (A, A + q):
            if AA < 2 * q and redc62(AA * W, q) == t0 + q:
                out.append(AA)
        if len(out) >= count:
            break
    return out


@pytest.mark.parametrize("logN", [13, 14])
def test_lazy_fix_window_known_answer(logN):
    """The reference multiplies by lazy Montgomery constants (its tables come from its own lazy REDC, so any entry may be
    the representative in [q, 2q)).  With q = 2^41 - 65535, the twiddle psi_br[1] (first forward stage) entered as
    psi_br[1] + q and Rs as Rs + q, the operands below make the reference's REDC62 return t0 + q with t0 in [2^21, 2^22)
    (proven on the host) — the top of dp_lazy_fix's window, unreachable when q < 2^40.5 or when both factors are canonical
    (then A W < 2 q^2 < 2^83).  The whole transforms (lf_ntt, lf_ntt_ws, enter_ntt through both) must equal the oracle bit
    for bit."""
    from liberate_fhe_amd._native import lib
    q = (1 << 41) - 65535
    primes = pick_edge_primes(logN, 1, 1, 0, 1)
    assert primes[0] == q
    lim = Limbs(logN, primes)
    N = lim.N
    psi, ipsi = (t.copy() for t in lim.mont_tables())
    assert 0 < psi[0, 1] < q
    psi[0, 1] += q                                          # same residue, the lazy representative
    W = int(psi[0, 1])
    s = Setup(lim, psi=psi, ipsi=ipsi)
    Rs_lazy = lim.Rs.copy()
    Rs_lazy[0] += q
    rs = int(Rs_lazy[0])

    rng = np.random.default_rng(logN)
    x = np.stack([lim.uniform(logN + 1, lazy=True), lim.uniform(logN + 2, lazy=True)])
    # forward: stage 0 multiplies a[j + N/2] by psi_br[1]
    fa = _window_operands(q, W, 64)
    assert len(fa) >= 16
    cols = N // 2 + rng.choice(N // 2, size=len(fa), replace=False)
    x[0, 0, cols] = fa
    x[1, 0, cols[::-1]] = fa
    hits = [redc62(int(a) * W, q) - q for a in x[0, 0, N // 2:]]
    assert sum((1 << 21) <= t < (1 << 22) for t in hits if t >= 0) >= 16
    # enter_ntt: the entry product a[j] * (Rs + q)
    ea = _window_operands(q, rs, 64)
    assert len(ea) >= 16
    y = x.copy()
    ecols = rng.choice(N, size=len(ea), replace=False)
    y[:, 0, ecols] = ea
    assert sum((1 << 21) <= redc62(int(a) * rs, q) - q < (1 << 22) for a in y[0, 0]) >= 16

    want = [s.o_ntt(p) for p in x]
    want_e = [s.o_ntt(p, enter=True, Rs=Rs_lazy) for p in y]
    Rs_dev = dev(Rs_lazy)
    old = lib.lf_tune(LF_TUNE_WS_EXTRA_STAGE, -1)
    try:
        for ws, extra in ((False, None), (True, 1), (True, 0)):
            if extra is not None:
                lib.lf_tune(LF_TUNE_WS_EXTRA_STAGE, extra)
            got = s.ntt(x, ws=ws)
            assert all((got[b] == want[b]).all() for b in range(2)), f"ntt ws={ws} extra={extra}"
            got = s.ntt(y, Rs=Rs_dev, ws=ws)
            assert all((got[b] == want_e[b]).all() for b in range(2)), f"enter_ntt ws={ws} extra={extra}"
    finally:
        lib.lf_tune(LF_TUNE_WS_EXTRA_STAGE, old)


def _mod_rows(x, q_host):
    return np.mod(x, q_host[None, :, None] if x.ndim == 3 else q_host[:, None])


@pytest.mark.parametrize("logN", [12, 13, 14, 16, 17])
def test_relaxed_forward_on_signed_lazy_words(logN):
    """LF_NTT_RELAXED (Rs = NULL) and LF_NTT_RELAXED | LF_NTT_PLAIN with Rs on the reference's signed-lazy words at
    +-(2q - 1): residues equal to the oracle's transform mod q (PLAIN: fp64-class rows skip Rs), as canonical words — lazy
    words below 2q on the integer-class rows of a one-pass (logN 12) transform."""
    lim = edge_limbs(logN)
    check_relaxed_forward(Setup(lim), edge_batch(lim, 40 + logN, signed=True), EDGE_PATTERNS)


def check_relaxed_forward(s, x, names):
    """The body of test_relaxed_forward_on_signed_lazy_words on the operands x [batch, rows, N], polynomial b named names[b]
    (also run at the ring degrees above 17 by tests/test_large_rings_gpu.py)."""
    lim = s.lim
    logN = lim.logN
    canon = _mod_rows(x, s.q_host)
    small = s.q_host < SMALL_PRIME_LIMIT
    # canonical words, except the integer-class rows of a one-pass transform (logN <= 12): lazy words in [0, 2q)
    # (include/ckks_hip.h, LF_NTT_RELAXED)
    limit = np.where(small | (logN > 12), s.q_host, 2 * s.q_host)[None, :, None]
    got = s.ntt(x, flags=LF_NTT_RELAXED)
    assert (got >= 0).all() and (got < limit).all()
    for b, p in enumerate(names):
        assert (_mod_rows(got[b], s.q_host) == _mod_rows(s.o_ntt(canon[b]), s.q_host)).all(), f"relaxed {p}"
    got = s.ntt(x, Rs=s.Rs, flags=LF_NTT_RELAXED | LF_NTT_PLAIN)
    assert (got >= 0).all() and (got < limit).all()
    for b, p in enumerate(names):
        want = np.where(small[:, None], s.o_ntt(canon[b]), s.o_ntt(canon[b], enter=True))
        assert (_mod_rows(got[b], s.q_host) == _mod_rows(want, s.q_host)).all(), f"relaxed | plain {p}"


@pytest.mark.parametrize("logN", [12, 13, 14, 16, 17])
def test_relaxed_inverse_at_the_documented_input_bound(logN):
    """A relaxed inverse transform (tails 2 and 3) on the largest words include/ckks_hip.h promises: 2^46 - 1 on fp64-class
    rows (every word, and alternating with 0 by the Thue-Morse parity), 2q - 1 on integer-class rows: the oracle's chain
    of the residues."""
    check_relaxed_inverse(Setup(edge_limbs(logN)), seed=logN)


def check_relaxed_inverse(s, seed, kinds=(0, 1, 2)):
    """The body of test_relaxed_inverse_at_the_documented_input_bound, on the operands `kinds` of: 0 every word at the bound,
    1 the bound alternating with 0 by the Thue-Morse parity, 2 uniform random words below it (also run at the ring degrees
    above 17 by tests/test_large_rings_gpu.py)."""
    lim = s.lim
    small = s.q_host < SMALL_PRIME_LIMIT
    top = np.where(small, RELAXED_INV_DP_BOUND - 1, 2 * s.q_host - 1)[:, None]
    tm = thue_morse(lim.N)[None, :]
    rng = np.random.default_rng(seed)
    make = (lambda: np.broadcast_to(top, (lim.rows, lim.N)), lambda: np.where(tm == 1, 0, top),
            lambda: np.stack([rng.integers(0, int(t), size=lim.N, dtype=np.int64) for t in top[:, 0]]))
    x = np.stack([make[k]() for k in kinds]).astype(np.int64)
    canon = _mod_rows(x, s.q_host)
    for tail in (2, 3):
        got = s.intt(x, tail, flags=LF_NTT_RELAXED)
        for b in range(x.shape[0]):
            assert (got[b] == s.o_intt(canon[b], tail)).all(), f"tail {tail}, operand {b}"


@pytest.mark.parametrize("logN", [13, 14, 16])
def test_stack_planes_on_interleaved_classes(logN):
    """cc_mult's operand stack in the planes format on a chain whose classes alternate row by row: lf_stack_planes says 1,
    lf_rescale_ntt (RELAXED | PLAIN | PLANES) writes the canonical words of the raw stack as u32 / u16 planes on the
    fp64-class rows (the integer-class rows raw), and lf_intt_mul reading either stack gives the same words — which are the
    oracle's chain of the products (plain products on fp64-class rows, REDC62 products on the others)."""
    from liberate_fhe_amd._native import lib, check
    from oracle import oracle as orc
    lim = edge_limbs(logN)
    s = Setup(lim)
    rows, N, count = lim.rows, lim.N, 4
    assert lib.lf_stack_planes(logN, rows, s.q_host.ctypes.data) == 1
    rng = np.random.default_rng(logN)
    q_drop = int(lim.q[1]) | 1
    srcs = [dev(np.stack([rng.integers(0, int(x), size=N, dtype=np.int64) for x in lim.q])) for _ in range(count)]
    for t in srcs[:2]:                                   # words at the top of their range
        t[:, ::3] = torch.from_numpy(s.q_host - 1).cuda()[:, None]
    row0 = [dev(rng.integers(0, q_drop, size=N, dtype=np.int64)) for _ in range(count)]
    row0[0][::2] = q_drop - 1
    scales = dev(np.array([rng.integers(1, int(x)) for x in lim.q], dtype=np.int64))
    arr = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    small = s.q_host < SMALL_PRIME_LIMIT
    stacks, prods = {}, {}
    for planes in (0, LF_NTT_PLANES):
        flags = LF_NTT_RELAXED | LF_NTT_PLAIN | planes
        st = torch.full((count, rows, N), -1, dtype=torch.int64, device="cuda")
        check(lib.lf_rescale_ntt(arr(srcs), arr(row0), count, st.data_ptr(), rows, logN, scales.data_ptr(), q_drop // 2,
                                 s.psi.data_ptr(), s.dp, s.q_host.ctypes.data, s.Rs.data_ptr(), flags, s.q2.data_ptr(),
                                 *s.cp, 0, s.st), "rescale_ntt")
        dst = torch.full((2, rows, N), -1, dtype=torch.int64, device="cuda")
        # polynomials 0, 2 times 1, 3
        check(lib.lf_intt_mul(dst.data_ptr(), st[0].data_ptr(), 2 * rows * N, st[1].data_ptr(), 2 * rows * N, 2, rows, logN,
                              s.ipsi.data_ptr(), s.idp, s.q_host.ctypes.data, s.Ninv.data_ptr(), 2, flags, *s.cp, 0, s.st),
              "intt_mul")
        stacks[planes], prods[planes] = st.cpu().numpy(), dst.cpu().numpy()
    raw, pl = stacks[0], stacks[LF_NTT_PLANES]
    assert ((raw >= 0) & (raw < s.q_host[None, :, None])).all()
    for r in range(rows):
        if small[r]:
            lo = pl[:, r].view(np.uint32)[:, :N].astype(np.int64)
            hi = pl[:, r].view(np.uint16)[:, 2 * N:3 * N].astype(np.int64)
            assert ((hi << 32) | lo == raw[:, r]).all(), f"planes of row {r}"
        else:
            assert (pl[:, r] == raw[:, r]).all(), f"raw row {r}"
    assert (prods[0] == prods[LF_NTT_PLANES]).all()
    for p in range(2):
        A, B = raw[2 * p].copy(), raw[2 * p + 1].copy()
        y_int = np.empty_like(A)
        orc.mont_mult(A, B, y_int, rows, *lim.mont_args())
        Be = B.copy()
        orc.mont_enter(Be, lim.Rs, rows, *lim.mont_args())          # b R: the Montgomery product with A is the plain product
        y_dp = np.empty_like(A)
        orc.mont_mult(A, Be, y_dp, rows, *lim.mont_args())
        z_dp = s.o_intt(y_dp, 2)                                    # N^-1 R^-1 intt(a b)
        orc.mont_enter(z_dp, lim.Rs, rows, *lim.mont_args())       # N^-1 intt(a b): PLAIN
        want = np.where(small[:, None], z_dp % s.q_host[:, None], s.o_intt(y_int, 2))
        assert (prods[0][p] == want).all(), f"intt_mul {p}"
