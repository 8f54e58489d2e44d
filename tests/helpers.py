"""Shared test scaffolding: synthetic limb sets for any logN, seeded inputs, oracle-side constants."""
from __future__ import annotations

import hashlib
import json
import os

import numpy as np

from liberate_fhe_amd.fhe.context import primes as P
from liberate_fhe_amd.fhe.context.ckks_context import bit_reverse_indices, _power_table

R = 1 << 62
LB = (1 << 31) - 1


def primitive_root_2N(q, N):
    """Same search as the context's, but not capped at x < N (tiny test rings need larger x)."""
    e = (q - 1) // (2 * N)
    for x in range(2, 1000):
        g = pow(x, e, q)
        if pow(g, N, q) != 1:
            return g
    raise ValueError(q)


def i64(v):
    return np.ascontiguousarray(np.asarray(v, dtype=np.int64))


class Limbs:
    """Montgomery / NTT constants of a list of primes for ring degree 2^logN, as host arrays of the word mode:
    bits = 62 (int64 words, R = 2^62, 31-bit halves) or 30 (the reference's int32 mode: R = 2^30, 15-bit halves)."""

    def __init__(self, logN, q, bits=62):
        self.logN, self.N, self.q = logN, 1 << logN, [int(x) for x in q]
        self.bits, self.R, self.half = bits, 1 << bits, bits // 2
        self.dtype = np.int64 if bits == 62 else np.int32
        N, Rr, lb, h = self.N, self.R, (1 << (bits // 2)) - 1, bits // 2
        arr = lambda v: np.ascontiguousarray(np.asarray(v, dtype=self.dtype))
        self.rows = len(self.q)
        self.k = [(Rr * pow(Rr, -1, qi) - 1) // qi for qi in self.q]
        self.ql, self.qh = arr([x & lb for x in self.q]), arr([x >> h for x in self.q])
        self.kl, self.kh = arr([x & lb for x in self.k]), arr([x >> h for x in self.k])
        self._2q = arr([2 * x for x in self.q])
        self.Rs = arr([Rr * Rr % x for x in self.q])
        self.Ninv = arr([pow(N, -1, x) * Rr % x for x in self.q])
        brev = bit_reverse_indices(logN)
        self.root = [primitive_root_2N(x, N) for x in self.q]
        self.psi_plain = np.stack([_power_table(g, N, x)[brev] for g, x in zip(self.root, self.q)]).astype(self.dtype)
        self.ipsi_plain = np.stack([_power_table(pow(g, -1, x), N, x)[brev] for g, x in zip(self.root, self.q)]).astype(self.dtype)
        self._mont = None

    def mont_tables(self):
        """psi_br / ipsi_br entered into Montgomery form with the ORACLE's mm (as the reference does on device)."""
        if self._mont is None:
            from oracle import oracle as orc
            psi, ipsi = self.psi_plain.copy(), self.ipsi_plain.copy()
            orc.mont_enter(psi, self.Rs, self.rows, self.ql, self.qh, self.kl, self.kh)
            orc.mont_enter(ipsi, self.Rs, self.rows, self.ql, self.qh, self.kl, self.kh)
            self._mont = (psi, ipsi)
        return self._mont

    def select(self, idx):
        """The limb set of the rows `idx` of this one (no table is recomputed: rows are independent)."""
        import copy
        idx = list(idx)
        sub = copy.copy(self)
        sub.q, sub.k, sub.root = ([v[i] for i in idx] for v in (self.q, self.k, self.root))
        sub.rows = len(idx)
        for name in ("ql", "qh", "kl", "kh", "_2q", "Rs", "Ninv", "psi_plain", "ipsi_plain"):
            if getattr(self, name) is not None:
                setattr(sub, name, np.ascontiguousarray(getattr(self, name)[idx]))
        sub._mont = None if self._mont is None else tuple(np.ascontiguousarray(t[idx]) for t in self._mont)
        return sub

    def mont_args(self):
        return self.ql, self.qh, self.kl, self.kh

    def uniform(self, seed, lazy=False):
        rng = np.random.default_rng(seed)
        return np.stack([rng.integers(0, (2 if lazy else 1) * x, size=self.N, dtype=np.int64) for x in self.q]).astype(self.dtype)


def pick_primes30(logN, n_scale=2, n_message=1, scale_bits=24):
    """NTT-friendly primes of the 30-bit word mode: `n_scale` near 2^scale_bits, `n_message` just below 2^28
    (the reference's message_bits = buffer_bit_length - 2, ckks_context.py:222)."""
    M = 2 << logN
    out, q = [], (1 << scale_bits) + 1
    for _ in range(n_scale):
        q = P.next_ntt_prime(q, M, up=True)
        out.append(q)
        q += 2
    q = (1 << 28) - 1
    for _ in range(n_message):
        q = P.next_ntt_prime(q, M, up=False)
        out.append(q)
        q -= 2
    return out


def pick_primes(logN, n40=2, n60=1):
    """A few NTT-friendly primes for ring degree 2^logN: `n40` near 2^40 and `n60` just below 2^60."""
    M = 2 << logN
    out, q = [], (1 << 40) + 1
    for _ in range(n40):
        q = P.next_ntt_prime(q, M, up=True)
        out.append(q)
        q += 2
    q = (1 << 60) - 1
    for _ in range(n60):
        q = P.next_ntt_prime(q, M, up=False)
        out.append(q)
        q -= 2
    return out


SMALL_PRIME_LIMIT = 1 << 41     # csrc/ckks_ntt_core.h: rows whose prime is below it run the fp64 class, the others the integer class


def pick_edge_primes(logN, n_top=2, n_bottom=2, n_small=1, n60=1):
    """NTT-friendly primes (q = 1 mod 2N) at the edges of the two arithmetic classes, interleaved by class row by row:
    the `n_top` largest below 2^41 (top of the fp64 class) alternating with the `n_bottom` smallest above 2^41 (bottom of
    the integer class), then `n_small` fp64-class primes from just above 2^20 and `n60` just below 2^60."""
    M = 2 << logN
    top, q = [], SMALL_PRIME_LIMIT - 1
    for _ in range(n_top):
        q = P.next_ntt_prime(q, M, up=False)
        top.append(q)
        q -= 2
    bottom, q = [], SMALL_PRIME_LIMIT + 1
    for _ in range(n_bottom):
        q = P.next_ntt_prime(q, M, up=True)
        bottom.append(q)
        q += 2
    out = []
    for i in range(max(n_top, n_bottom)):
        out += top[i:i + 1] + bottom[i:i + 1]
    q = (1 << 20) + 1
    for _ in range(n_small):
        q = P.next_ntt_prime(q, M, up=True)
        out.append(q)
        q += 2
    q = (1 << 60) - 1
    for _ in range(n60):
        q = P.next_ntt_prime(q, M, up=False)
        out.append(q)
        q -= 2
    return out


def thue_morse(N):
    """0 / 1 per index: the parity of its number of set bits.  Every butterfly pair (j, j + 2^k with bit k of j clear)
    of every stage holds one index of each parity."""
    j = np.arange(N, dtype=np.int64)
    par = np.zeros(N, dtype=np.int64)
    while j.any():
        par ^= j & 1
        j >>= 1
    return par


EDGE_PATTERNS = ("2q-1", "2q-1|0", "q-1", "lazy")


def edge_operand(lim, pattern, seed=0, signed=False):
    """[rows, N] int64 words that drive the transforms to their proven bounds:
      "2q-1"    every word 2q - 1 (the largest forward and inverse sums);
      "2q-1|0"  2q - 1 and 0 by the Thue-Morse parity of the index (the largest difference in every butterfly);
      "q-1"     every word q - 1;
      "lazy"    uniform random lazy words in [0, 2q).
    signed=True (entries that accept the reference's signed-lazy words): the words of "2q-1" and "2q-1|0" become
    +-(2q - 1) by the Thue-Morse parity, "lazy" uniform in (-2q, 2q)."""
    rng = np.random.default_rng(seed)
    tm = thue_morse(lim.N)
    rows = []
    for q in lim.q:
        top = 2 * q - 1
        if pattern == "2q-1":
            v = np.where(tm == 1, -top, top) if signed else np.full(lim.N, top, dtype=np.int64)
        elif pattern == "2q-1|0":
            v = np.where(tm == 1, -top if signed else 0, top)
        elif pattern == "q-1":
            v = np.full(lim.N, q - 1, dtype=np.int64)
        elif pattern == "lazy":
            v = rng.integers(-top if signed else 0, 2 * q, size=lim.N, dtype=np.int64)
        else:
            raise ValueError(pattern)
        rows.append(v.astype(np.int64))
    return np.stack(rows)


def redc62(x, q):
    """The reference's lazy REDC62 of a non-negative integer x < q 2^62, in Python integers: (x + ((x k) mod R) q) / R
    with k = -q^-1 mod R; the result lies in [0, 2q) and is congruent to x R^-1."""
    k = (R * pow(R, -1, q) - 1) // q
    return (x + ((x * k) % R) * q) >> 62


def sha(arr) -> str:
    return hashlib.sha256(np.ascontiguousarray(arr).tobytes()).hexdigest()


class SeededCsprng:
    """Deterministic stand-in for the engines' Csprng (reference csprng.py:18-323): same method names, shapes and
    value ranges; randomness from numpy's PCG64, so the reference engine in the build container and this package's
    engine on the GPU box draw IDENTICAL tensors from one seed (the reference's own Csprng cannot be seeded).
    `devices`: where the drawn tensors are placed (one entry per logical device)."""

    def __init__(self, N, C, repeats, devices=None, seed=12345, local_ids=None, **_):
        import torch
        self.torch = torch
        self.N, self.C, self.num_repeating_channels = N, list(C), repeats
        self.devices = devices or ["cpu"]
        self.num_devices = len(self.devices)
        self.g = np.random.Generator(np.random.PCG64(seed))

    def _t(self, x, dev=0):
        return self.torch.from_numpy(np.ascontiguousarray(x).astype(np.int64)).to(self.devices[dev])

    def randint(self, amax=3, shift=0, repeats=1):
        # amax scalar -> [repeats, N] shared by every device; amax per-device list of per-row moduli
        # -> [C_dev + repeats, N] with the trailing `repeats` rows identical on every device.
        if not isinstance(amax, (list, tuple)):
            x = self.g.integers(0, amax, size=(max(repeats, 1), self.N)) + shift
            return [self._t(x, d) for d in range(self.num_devices)]
        out = []
        rep_rows = None
        for dev, q in enumerate(amax):
            q = list(q)
            n_rep = repeats
            body = q[: len(q) - n_rep] if n_rep else q
            rows = [self.g.integers(0, qi, size=self.N) + shift for qi in body]
            if n_rep:
                if rep_rows is None:
                    rep_rows = [self.g.integers(0, qi, size=self.N) + shift for qi in q[len(q) - n_rep:]]
                rows += rep_rows
            out.append(self._t(np.stack(rows), dev))
        return out

    def discrete_gaussian(self, non_repeats=0, repeats=1, sigma=3.2):
        x = np.rint(self.g.normal(0.0, 3.2, size=(max(repeats, 1), self.N)))
        return [self._t(x, d) for d in range(self.num_devices)]

    def randround(self, coef):
        dev = coef.device if isinstance(coef, self.torch.Tensor) else "cpu"
        c = coef.cpu().numpy() if isinstance(coef, self.torch.Tensor) else np.asarray(coef)
        fl = np.floor(c)
        r = fl + (self.g.random(c.shape) < (c - fl))
        return self.torch.from_numpy(r.astype(np.int64)).to(dev)


def fingerprint(x):
    """A JSON-able summary of a result that is equal exactly when the results are: ints, floats, strings and None as they are,
    tensors and arrays as shape + SHA-256 of their words (int64 for integer data, float64 / complex128 otherwise), data_struct
    objects as their flags plus their data.  numpy scalars count as the Python numbers they equal."""
    import torch
    if hasattr(x, "origin") and hasattr(x, "data") and hasattr(x, "level"):
        return {"origin": x.origin, "level": int(x.level), "include_special": bool(x.include_special),
                "ntt_state": bool(x.ntt_state), "montgomery_state": bool(x.montgomery_state), "data": fingerprint(x.data)}
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    if isinstance(x, np.ndarray):
        kind = np.int64 if x.dtype.kind in "biu" else (np.complex128 if x.dtype.kind == "c" else np.float64)
        return {"shape": list(x.shape), "sha256": sha(x.astype(kind))}
    if isinstance(x, (list, tuple)):
        return [fingerprint(v) for v in x]
    if isinstance(x, dict):
        return {str(k): fingerprint(v) for k, v in sorted(x.items(), key=lambda kv: str(kv[0]))}
    if isinstance(x, (bool, np.bool_)):
        return bool(x)
    if isinstance(x, (int, np.integer)):
        return int(x)
    if isinstance(x, (float, np.floating)):
        return float(x)
    if x is None or isinstance(x, str):
        return x
    raise TypeError(f"no fingerprint for {type(x).__name__}")


class Recorded:
    """Results the reference produced for one test, recorded by tests/golden/make_golden_reference.py into
    tests/golden/reference_results.json: `check(key, value)` asserts that `value` equals the reference's result under
    `key`.  Made with `record=True` (the generator), it stores the fingerprints instead."""

    PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_results.json")
    _store = None

    def __init__(self, test, record=False):
        if Recorded._store is None:
            Recorded._store = json.load(open(self.PATH)) if os.path.exists(self.PATH) else {}
        self.test, self.record = test, record
        if record:
            Recorded._store[test] = {}
        self.expected = Recorded._store.get(test, {})

    def check(self, key, value):
        got = fingerprint(value)
        text = json.dumps(got, sort_keys=True)
        if len(text) > 200:         # a long fingerprint is kept as its digest
            got = "sha256:" + hashlib.sha256(text.encode()).hexdigest()
        if self.record:
            assert key not in self.expected, f"{self.test}: key {key!r} recorded twice"
            self.expected[key] = got
            return
        assert key in self.expected, f"{self.test}: nothing recorded under {key!r} (run tests/golden/make_golden_reference.py)"
        assert got == self.expected[key], f"{self.test}: {key} differs from the reference's result"

    @classmethod
    def save(cls):
        with open(cls.PATH, "w") as f:
            json.dump(cls._store, f, indent=1, sort_keys=True)
            f.write("\n")
