"""CKKS encode / decode (fp64 negacyclic FFT) and the Galois exponent of a rotation.

API mirror of the reference's src/liberate/fhe/encdec/encdec.py (`encode`, `decode`, `rotate`,
`conjugate`): same slot order (so plaintexts / ciphertexts are interchangeable with the reference's)
and the same fp64 pipeline, which stays on torch.fft — the reference does the same and SURVEY.md §8(f)
ranks it as a "next" row; it is not part of the integer hot path.

Slot order.  The reference orders slots so that the ring automorphism X -> X^3 rotates the decoded
vector by one.  It derives that order by matching cycles of two permutations (encdec.py:65-121,
199-209): the "circular shift" of both halves of [0, N) and the action i -> 3i + 1 (mod N) of the
automorphism on the odd exponents 2i + 1.  `_slot_permutation` below builds the same map directly:
walk each orbit of i -> 3i+1 starting at the image of its smallest member, and lay the orbit along
the corresponding shift cycle.
"""
from __future__ import annotations

import numpy as np
import torch

_perm_cache = {}
_twist_cache = {}


def _orbits(perm: np.ndarray):
    """Cycles of `perm`, each listed from perm[s] round to s, s = smallest unvisited element."""
    n = len(perm)
    seen = np.zeros(n, dtype=bool)
    out = []
    for s in range(n):
        if seen[s]:
            continue
        cyc = []
        x = int(perm[s])
        while True:
            cyc.append(x)
            seen[x] = True
            if x == s:
                break
            x = int(perm[x])
        out.append(cyc)
    return out


def _slot_permutation(N: int):
    """(pre_perm [N/2], post_perm [N]) as numpy int64 — the reference's `prepost_perms`."""
    half = N // 2
    shift = np.concatenate([np.roll(np.arange(half), 1), np.roll(np.arange(half), -1) + half])
    fold = (3 * np.arange(N) + 1) % N
    a, b = _orbits(shift), _orbits(fold)
    assert [len(c) for c in a] == [len(c) for c in b]
    post = np.zeros(N, dtype=np.int64)
    post[np.concatenate([np.array(c) for c in b])] = np.concatenate([np.array(c) for c in a])
    pre = np.argsort(post)[:half]
    return pre, post


def prepost_perms(N, device="cuda:0"):
    key = (N, str(device))
    if key not in _perm_cache:
        pre, post = _slot_permutation(N)
        _perm_cache[key] = (torch.from_numpy(pre).to(device), torch.from_numpy(post).to(device))
    return _perm_cache[key]


def _twist(N, device, sign):
    key = (N, str(device), sign)
    if key not in _twist_cache:
        ang = sign * 1j * torch.pi * torch.arange(N, device=device, dtype=torch.float64) / N
        _twist_cache[key] = torch.exp(ang)
    return _twist_cache[key]


def generate_twister(N, device="cuda:0"):
    return _twist(N, device, -1)


def generate_skewer(N, device="cuda:0"):
    return _twist(N, device, +1)


def encode(m, rng=None, scale=2 ** 40, deviation=1.0, device="cuda:0", norm="forward",
           return_without_scaling=False):
    """Message (N/2 complex slots) -> N real polynomial coefficients (encdec.py:273-298)."""
    N = len(m) * 2
    pre, _ = prepost_perms(N, device)
    mm = torch.from_numpy(np.array(m * deviation)).to(device)
    spread = torch.zeros((N,), dtype=mm.dtype, device=mm.device)
    spread[pre] = mm
    spread = spread + spread.conj().flip(0)
    coeffs = (torch.fft.fft(spread, norm=norm) * generate_twister(N, device)).real
    if return_without_scaling:
        return coeffs
    return rng.randround(coeffs * np.float64(scale))


def decode(m, scale=2 ** 40, correction=1.0, norm="forward", return_without_scaling=False):
    """N polynomial coefficients -> N complex values, the message in the first N/2 (encdec.py:301-323)."""
    N = len(m)
    device = m.device
    _, post = prepost_perms(N, device)
    vals = torch.fft.ifft(m * generate_skewer(N, device), norm=norm)
    if not return_without_scaling:
        vals = vals / scale * correction
    out = torch.zeros_like(vals)
    out[post] = vals
    return out


def galois_exponent(N: int, delta: int) -> int:
    """p such that rotating the slots by `delta` is X -> X^p: p = 3^(delta mod N) mod 2N (encdec.py:224-229)."""
    return pow(3, delta % N, 2 * N)


def conjugation_exponent(N: int) -> int:
    """Complex conjugation of the slots is X -> X^(2N-1) (encdec.py:249-253)."""
    return 2 * N - 1


_coeff_slot_cache = {}


def coeff_slot_matrices(N: int, norm: str = "forward") -> tuple:
    """(B, C, E, F), complex [n, n] with n = N / 2: the maps between the slots z of a REAL coefficient vector t of length N (what
    decode(t, return_without_scaling=True)[:n] gives) and its coefficients packed two to a slot, u = t[:n] + 1j * t[n:]:
        u = B z + C conj(z),        z = E u + F conj(u).
    Only real-linear: with this slot order (generator 3, galois_exponent) the evaluation points zeta_k satisfy
    zeta_k^(N/2) = +i or -i alternating from slot to slot, so neither map is a complex matrix alone — C and F are not zero.
    In closed form from the transforms encode and decode apply, on all unit vectors at once (host numpy, no engine); kept per
    (N, norm).  Read-only: callers share the cached arrays."""
    key = (int(N), norm)
    hit = _coeff_slot_cache.get(key)
    if hit is not None:
        return hit
    if N < 4 or N & (N - 1):
        raise ValueError(f"coeff_slot_matrices: N must be a power of two >= 4, got {N}")
    n = N // 2
    pre, post = _slot_permutation(N)
    k = np.arange(N)
    # decode on the unit vectors: column k of V is decode(e_k)[:n];  z = V t = V_lo Re(u) + V_hi Im(u)
    vals = np.fft.ifft(np.eye(N) * np.exp(1j * np.pi * k / N)[:, None], axis=0, norm=norm)
    V = np.zeros((N, N), dtype=np.complex128)
    V[post] = vals
    V = V[:n]
    E = (V[:, :n] - 1j * V[:, n:]) / 2
    F = (V[:, :n] + 1j * V[:, n:]) / 2
    del V, vals
    # encode without scaling on the unit vectors: t = W z + conj(W) conj(z) with column k of W = (t(e_k) - i t(i e_k)) / 2, where
    # t(m) = Re(fft(spread(m)) * twister) and spread(e_k) has a one at pre[k] and at N - 1 - pre[k]
    twist = np.exp(-1j * np.pi * k / N)[:, None]
    S = np.zeros((N, n), dtype=np.complex128)
    S[pre, np.arange(n)] = 1.0
    fa = np.fft.fft(S, axis=0, norm=norm) * twist                 # the slot's own term
    fb = np.fft.fft(S[::-1], axis=0, norm=norm) * twist           # its mirrored conjugate
    del S
    t_one = (fa + fb).real
    t_i = (1j * fa - 1j * fb).real
    W = (t_one - 1j * t_i) / 2
    B = W[:n] + 1j * W[n:]
    C = W[:n].conj() + 1j * W[n:].conj()
    out = _coeff_slot_cache[key] = (B, C, E, F)
    for M in out:
        M.setflags(write=False)
    return out


def matrix_diagonals(M) -> dict:
    """The non-zero generalized diagonals of a square matrix, {step: vector} with diag_step[i] = M[i][(i - step) mod n]: the
    convention in which M @ v = sum_step diag_step * np.roll(v, step), i.e. what ckks_engine.linear_transform evaluates."""
    M = np.asarray(M)
    if M.ndim != 2 or M.shape[0] != M.shape[1]:
        raise ValueError(f"matrix_diagonals: a square matrix is required, got shape {M.shape}")
    n = M.shape[0]
    i = np.arange(n)
    out = {}
    for step in range(n):
        dg = M[i, (i - step) % n]
        if np.any(dg != 0):
            out[step] = dg
    return out


def bsgs_split(steps, num_slots: int, n1=None) -> tuple:
    """Baby-step / giant-step split of the rotation steps of a linear transform: every step (taken mod num_slots) is g + b with
    b = step mod n1 and g = step - b.  Returns (n1, babies, giants), both sorted and with 0 where it occurs: a transform over
    `steps` needs one rotation key per non-zero baby step and one per non-zero giant step.  n1=None picks the power of two that
    minimises that number of keys (ties: the larger n1, giant steps being the dearer ones)."""
    reduced = sorted({int(s) % num_slots for s in steps})
    if not reduced:
        raise ValueError("bsgs_split: no step given")

    def split(n):
        return sorted({s % n for s in reduced}), sorted({s - s % n for s in reduced})

    if n1 is None:
        best = None
        n = 1
        while n <= num_slots:
            babies, giants = split(n)
            cost = sum(1 for b in babies if b) + sum(1 for g in giants if g)
            if best is None or cost <= best[0]:
                best = (cost, n)
            n *= 2
        n1 = best[1]
    try:
        ok = int(n1) == n1 and int(n1) >= 1 and not isinstance(n1, bool)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"bsgs_split: n1 must be an integer >= 1, got {n1!r}")
    n1 = int(n1)
    babies, giants = split(n1)
    return n1, babies, giants


# The radix inner_sum uses unless told otherwise: the fastest of {2, 4, 8} at gold, level 0, for n = 64 on one MI355X
# (tools/inner_sum.py; the figures are in DESIGN.md §4.2)
INNER_SUM_RADIX = 4
# the most one stage may be: what lf_linear_transform_bsgs allows one hoisted set (LF_BSGS_MAX_BABY_KEYS keys + the ciphertext)
INNER_SUM_MAX_STAGE = 64


def inner_sum_plan(n: int, stride: int, num_slots: int, radix: int = INNER_SUM_RADIX) -> list:
    """The mixed-radix stages of sum_{j < n} rot(x, j * stride): [(r_t, (steps ..)), ..] with n = r_1 r_2 .. r_m.  Stage t adds
    the r_t copies of its input rotated by j * stride * r_1 .. r_{t-1} (mod num_slots), j = 0 .. r_t - 1; its `steps` are those
    of j >= 1, the ones that need a rotation key.  Every j < n is sum_t j_t r_1 .. r_{t-1} with j_t < r_t exactly once, so the
    chain of the stages is the whole sum.  Factors <= radix are taken greedily, largest first; a prime factor above radix is a
    stage of its own.  n = 1: no stage.  ValueError for n < 1, radix < 2, a stage above INNER_SUM_MAX_STAGE, or
    n * |stride| > num_slots (the sum would wrap onto itself)."""
    try:
        ok = int(n) == n and int(stride) == stride and int(radix) == radix and not isinstance(n, bool)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"inner_sum_plan: integers are required, got n={n!r}, stride={stride!r}, radix={radix!r}")
    n, stride, radix = int(n), int(stride), int(radix)
    if n < 1:
        raise ValueError(f"inner_sum_plan: n >= 1 is required, got {n}")
    if radix < 2:
        raise ValueError(f"inner_sum_plan: radix >= 2 is required, got {radix}")
    if n * abs(stride) > num_slots:
        raise ValueError(f"inner_sum_plan: n * |stride| = {n * abs(stride)} exceeds the {num_slots} slots")
    stages, rest, unit = [], n, stride
    while rest > 1:
        r = next((f for f in range(min(radix, rest), 1, -1) if rest % f == 0), None)
        if r is None:                                   # no factor <= radix: the smallest factor left is a prime above it
            r = next(f for f in range(radix + 1, rest + 1) if rest % f == 0)
        if r > INNER_SUM_MAX_STAGE:
            raise ValueError(f"inner_sum_plan: n = {n} has the prime factor {r}, above the {INNER_SUM_MAX_STAGE} of one stage")
        stages.append((r, tuple((j * unit) % num_slots for j in range(1, r))))
        rest //= r
        unit *= r
    return stages


# include/ckks_hip.h: LF_CC_MATMUL_MAX_INNER / LF_CC_MATMUL_MAX_OPERANDS (tests/test_cc_matmul_cpu.py holds these copies to the header)
CC_MATMUL_MAX_INNER = 64
CC_MATMUL_MAX_OPERANDS = 256


def cc_matmul_tiles(m: int, n: int, gmax: int = 4) -> list:
    """The tiles (i0, j0, R, C) lf_cc_matmul cuts an m x n matrix of outputs into (the native entry applies the same rule): every
    output in exactly one tile, R C in {4, 2, 1} and at most gmax (the plan's max_nct).  2 x 2 where both dimensions allow it and
    a tile may hold 4 outputs; strips of 1 x 4 / 4 x 1, then 1 x 2 / 2 x 1, then 1 x 1 along a vector, down an odd last column
    and along an odd last row."""
    if m < 1 or n < 1 or gmax < 1:
        raise ValueError(f"cc_matmul_tiles: m, n, gmax >= 1 are required, got {m}, {n}, {gmax}")

    def strip(i0, j0, length, along_row):
        s = 0
        while s < length:
            left = length - s
            g = 4 if left >= 4 and gmax >= 4 else 2 if left >= 2 and gmax >= 2 else 1
            tiles.append((i0, j0 + s, 1, g) if along_row else (i0 + s, j0, g, 1))
            s += g

    tiles = []
    if n == 1 and m > 1:
        strip(0, 0, m, False)
    elif m == 1 or gmax < 4:
        for i in range(m):
            strip(i, 0, n, True)
    else:
        m2, n2 = m & ~1, n & ~1
        tiles += [(i, j, 2, 2) for i in range(0, m2, 2) for j in range(0, n2, 2)]
        if n & 1:
            strip(0, n - 1, m, False)
        if m & 1:
            strip(m - 1, 0, n2, True)
    return tiles


def cc_matmul_plan(A, B, max_operands: int = CC_MATMUL_MAX_OPERANDS, max_inner: int = CC_MATMUL_MAX_INNER):
    """The shape and the native calls of C = A B for matrices of ciphertext OBJECTS (rows of entries; None: a zero entry):
    (m, k, n, calls).  calls: None where no native call can take the product (k above max_inner, or B with one row of A holding
    more than max_operands distinct operands); else row blocks of A, each a dict
        rows (i0, i1)      the rows of A, and of C, the call covers
        operands           its DISTINCT operands, by object identity, in order of first use (A's rows, then B)
        ia, ib             flat index tables into `operands`, [i - i0][t] resp. [t][j], -1 for None
    with at most max_operands operands per call: rows are taken greedily, the inner dimension is never split.  Pure: no engine,
    no device.  ValueError for an empty matrix, ragged rows, mismatched inner dimensions and an output with no term."""
    A, B = [list(r) for r in A], [list(r) for r in B]
    if not A or not B or not A[0] or not B[0]:
        raise ValueError("cc_matmul: empty matrix")
    m, k, n = len(A), len(A[0]), len(B[0])
    if any(len(r) != k for r in A) or any(len(r) != n for r in B):
        raise ValueError("cc_matmul: ragged rows")
    if len(B) != k:
        raise ValueError(f"cc_matmul: A has {k} columns, B has {len(B)} rows")
    for i in range(m):
        for j in range(n):
            if not any(A[i][t] is not None and B[t][j] is not None for t in range(k)):
                raise ValueError(f"cc_matmul: output ({i}, {j}) has no term")
    if k > max_inner:
        return m, k, n, None
    b_ids = {id(x) for row in B for x in row if x is not None}
    calls, i0 = [], 0
    while i0 < m:
        seen, i1 = set(b_ids), i0
        while i1 < m:
            more = seen | {id(x) for x in A[i1] if x is not None}
            if len(more) > max_operands:
                break
            seen, i1 = more, i1 + 1
        if i1 == i0:
            return m, k, n, None
        index, operands = {}, []

        def at(x):
            if x is None:
                return -1
            if id(x) not in index:
                index[id(x)] = len(operands)
                operands.append(x)
            return index[id(x)]

        ia = [at(A[i][t]) for i in range(i0, i1) for t in range(k)]
        ib = [at(B[t][j]) for t in range(k) for j in range(n)]
        calls.append({"rows": (i0, i1), "operands": operands, "ia": ia, "ib": ib})
        i0 = i1
    return m, k, n, calls


def _tree_levels(b: int) -> int:
    """Levels above the base at which the b-th power stands when powers are built by the tree rule of ckks_engine.poly_eval
    (a power of two 2^j by j squarings; any other b as top power of two times the rest, one level above the former)."""
    return (b - 1).bit_length()


def poly_schedule(degree: int, n1: int) -> dict:
    """The level schedule of ckks_engine.poly_eval for a polynomial of this degree split at n1 (a power of two >= 2), levels
    counted from the operand's: G = ceil((degree + 1) / n1) baby polynomials; "baby": the deepest baby power (all are brought
    there); "common": the level the baby polynomials (baby + 1) and the giant powers y^g are brought to before cc_dot; "depth":
    levels consumed; "products": ciphertext products (tensor products, the pairs of the final cc_dot included)."""
    try:
        ok = int(degree) == degree and degree >= 1 and int(n1) == n1 and n1 >= 2 and (int(n1) & (int(n1) - 1)) == 0
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"poly_schedule: degree >= 1 and n1 a power of two >= 2 are required, got {degree!r}, {n1!r}")
    degree, n1 = int(degree), int(n1)
    G = -(-(degree + 1) // n1)
    baby = _tree_levels(n1 - 1)
    if G == 1:
        return {"n1": n1, "G": 1, "baby": baby, "common": baby + 1, "depth": baby + 1, "products": n1 - 2}
    common = max(n1.bit_length() - 1 + _tree_levels(G - 1), baby + 1)
    return {"n1": n1, "G": G, "baby": baby, "common": common, "depth": common + 1,
            "products": (n1 - 2) + 1 + (G - 2) + (G - 1)}


def poly_split(degree: int) -> int:
    """The baby-step count n1 (a power of two, 2 <= n1 <= the first power of two above `degree`) ckks_engine.poly_eval uses
    unless told otherwise: the one with the fewest ciphertext products (n1 - 2 baby powers, y = x^n1, G - 2 further giant powers
    and the G - 1 pairs of the closing cc_dot, G = ceil((degree + 1) / n1)); ties go to the smaller depth, then to the larger n1
    (more of the work in the fused baby sums, fewer pairs under the closing relinearisation)."""
    best = None
    n = 2
    while True:
        s = poly_schedule(degree, n)
        key = (s["products"], s["depth"], -n)
        if best is None or key < best[0]:
            best = (key, n)
        if n > degree:
            break
        n *= 2
    return best[1]


def cheb_blocks(coeffs, n1: int) -> np.ndarray:
    """The Chebyshev series p = sum_i coeffs[i] T_i as p = sum_g r_g(x) T_n1(x)^g with every r_g a Chebyshev series of degree
    below n1: row g of the result ([G][n1], G = ceil(len(coeffs) / n1)) holds r_g, from repeated numpy chebdiv by T_n1."""
    from numpy.polynomial import chebyshev as C
    c = np.asarray(coeffs, dtype=np.float64)
    G = -(-c.size // n1)
    divisor = np.zeros(n1 + 1)
    divisor[n1] = 1.0
    out = np.zeros((G, n1))
    for g in range(G):
        if c.size > n1:
            c, rem = C.chebdiv(c, divisor)
        else:
            c, rem = np.zeros(1), c
        out[g, :rem.size] = rem
    return out


def ntt_galois_index(logN: int, p: int) -> np.ndarray:
    """pi_p as an int64 index array: NTT(a(X^p))[k] = NTT(a)[pi_p(k)] for the forward transform's order (index k holds the
    evaluation at psi^(2 brev(k) + 1)), pi_p(k) = brev(((2 brev(k) + 1) p mod 2N - 1) / 2).  A pure permutation (p odd):
    hoisted rotations gather the extended digits of one ciphertext by it, once per rotation (ckks_engine.rotate_hoisted)."""
    N = 1 << logN
    if p % 2 == 0 or not 0 < p < 2 * N:
        raise ValueError(f"ntt_galois_index: the exponent must be odd and in (0, 2N), got {p}")

    def brev(x):
        r = np.zeros_like(x)
        for b in range(logN):
            r |= ((x >> b) & 1) << (logN - 1 - b)
        return r

    t = ((2 * brev(np.arange(N, dtype=np.int64)) + 1) * p) % (2 * N)
    return brev((t - 1) // 2)
