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


# ---- operands for the fused engine kernels (tests/test_engine_edges_*.py) ------------------------------------------------
ENGINE_EDGE_PATTERNS = ("top", "top|0", "top|1", "half", "mixed", "random")
_MIXED_ROTATION = ("top", "top|0", "half", "top|1")


class _Rows:
    """The two attributes edge_operand reads of a limb set."""

    def __init__(self, q, N):
        self.q, self.N = [int(x) for x in q], N


def edge_rows(q_list, N, pattern, seed=0, lazy=False, ids=None):
    """[len(q_list), N] int64 words that sit on the range bounds of the coefficient-wise engine kernels:
      "top"     every word q - 1 (2q - 1 when lazy);
      "top|0"   top and 0 by the Thue-Morse parity of the index;
      "top|1"   top and 1 by the same parity;
      "half"    q // 2 and q // 2 + 1 alternating: the seam of the balanced representation;
      "mixed"   row i takes one of the four above, rotated by its id, so that the integer the rows represent jointly is
                not a small number (all rows at q_i - 1 are the integer -1);
      "random"  uniform words below q (2q when lazy), seeded per row id.
    `ids`: the identity of each row (its prime index: rotation of "mixed", seed of "random"), default 0, 1, ..; the words of
    a prime then do not depend on which device holds it."""
    q_list = [int(q) for q in q_list]
    ids = list(range(len(q_list))) if ids is None else list(ids)
    tm = thue_morse(N)
    odd = np.arange(N, dtype=np.int64) & 1
    out = np.empty((len(q_list), N), dtype=np.int64)
    for r, (q, i) in enumerate(zip(q_list, ids)):
        pat = _MIXED_ROTATION[i % 4] if pattern == "mixed" else pattern
        one = _Rows([q], N)
        if pat == "top":
            out[r] = edge_operand(one, "2q-1" if lazy else "q-1")[0]
        elif pat == "top|0":
            out[r] = edge_operand(one, "2q-1|0")[0] if lazy else np.where(tm == 1, 0, q - 1)
        elif pat == "top|1":
            out[r] = np.where(tm == 1, 1, (2 * q if lazy else q) - 1)
        elif pat == "half":
            out[r] = q // 2 + odd
        elif pat == "random":
            out[r] = np.random.default_rng([seed, i]).integers(0, (2 if lazy else 1) * q, size=N, dtype=np.int64)
        else:
            raise ValueError(pattern)
    return out


def rounder_row0(q_drop, N, shift=0):
    """[N] words of a dropped limb that hold the five values the rescale rounder [row0 > q_drop // 2] turns on —
    0, round_at - 1, round_at, round_at + 1, q_drop - 1 — one after the other along the coefficient index.  The period is
    odd, so each value falls on both lanes of every 16-byte pair."""
    at = int(q_drop) // 2
    vals = np.array([0, at - 1, at, at + 1, int(q_drop) - 1], dtype=np.int64)
    return vals[(np.arange(N) + shift) % 5]


def _edge_ids(engine):
    return getattr(engine, "local_ids", None) or list(range(engine.ntt.num_devices))


def _edge_ct(engine, data, level):
    from liberate_fhe_amd.utils.synth import _data_struct
    return _data_struct(engine)(data=tuple(data), include_special=False, ntt_state=False, montgomery_state=False,
                                origin="cipher text", level=level, hash=engine.hash, version=engine.version)


def edge_ciphertext(engine, level, pattern, seed=0):
    """utils.synth.ciphertext with the words of edge_rows: component 1 takes the next pattern of the list, so that a
    product never multiplies a row by itself."""
    import torch
    q, N = engine.ctx.q, engine.ctx.N
    dest = engine.ntt.p.destination_arrays[level]
    data = []
    for comp in range(2):
        pat = pattern if comp == 0 or pattern in ("mixed", "random") else \
            ENGINE_EDGE_PATTERNS[(ENGINE_EDGE_PATTERNS.index(pattern) + 1) % 4]
        rows = []
        for d in _edge_ids(engine):
            if d < len(dest):
                ids = [i + comp for i in dest[d]] if pattern == "mixed" else dest[d]
                w = edge_rows([q[i] for i in dest[d]], N, pat, seed * 2 + comp, ids=ids)
                rows.append(torch.from_numpy(w).to(engine.ntt.devices[d]))
        data.append(rows)
    return _edge_ct(engine, data, level)


PLAINTEXT_EDGE_PATTERNS = ENGINE_EDGE_PATTERNS + ("q|0",)


def _edge_pt(engine, data, level, kind):
    from liberate_fhe_amd.fhe.presets import types
    from liberate_fhe_amd.utils.synth import _data_struct
    if kind not in ("mult", "add"):
        raise ValueError(kind)
    assert 0 <= level < engine.num_levels - (kind == "mult"), (level, kind)   # (a "mult" plaintext needs a level to rescale into)
    return _data_struct(engine)(data=list(data), include_special=False, ntt_state=kind == "mult", montgomery_state=True,
                                origin=types.origins["pt_" + kind], level=level, hash=engine.hash, version=engine.version)


def edge_plaintext(engine, level, pattern, seed=0, kind="mult"):
    """engine.encode_plain(.., level, kind) — same origin, flags, hash and version, one [rows, N] tensor per local device alive at
    `level` — with the lazy words of edge_rows(.., lazy=True): "top" is 2q - 1 everywhere, "half" the seam of the balanced
    representation, "mixed" another of the four patterns on every row, "random" uniform below 2q.  One more pattern, "q|0": the
    lazy zero q and 0 by the Thue-Morse parity of the index — the REDC of the Montgomery word q is exactly q, the closed end of
    the interval [0, q] the fp64-class rows of the pc kernels reduce a plaintext word into.  kind="add": the bias of `level`
    (for a pc_dot of level-l operands: level = l + 1).  A word follows its prime's id, not the device that holds it."""
    import torch
    q, N = engine.ctx.q, engine.ctx.N
    dest = engine.ntt.p.destination_arrays[level]
    tm = thue_morse(N)
    data = []
    for d in _edge_ids(engine):
        if d < len(dest):
            if pattern == "q|0":
                w = np.where(tm[None, :] == 1, 0, np.array([int(q[i]) for i in dest[d]], dtype=np.int64).reshape(-1, 1))
            else:
                w = edge_rows([q[i] for i in dest[d]], N, pattern, seed, lazy=True, ids=dest[d])
            data.append(torch.from_numpy(w).to(engine.ntt.devices[d]))
    return _edge_pt(engine, data, level, kind)


def identity_plaintext(engine, level):
    """The "mult" plaintext whose every word of row i is R mod q_i — the Montgomery form of 1 in every coefficient of the NTT
    domain: the product with it leaves a ciphertext's words, so pc_dot([(identity, x)]) has exactly the words of rescale(x) and
    whatever x holds in its dropped limb (pre_rescale_ciphertext: the five values of rounder_row0) reaches the rounder of the
    pc entries."""
    import torch
    q, N = engine.ctx.q, engine.ctx.N
    dest = engine.ntt.p.destination_arrays[level]
    data = []
    for d in _edge_ids(engine):
        if d < len(dest):
            w = np.repeat(np.array([R % int(q[i]) for i in dest[d]], dtype=np.int64)[:, None], N, axis=1)
            data.append(torch.from_numpy(np.ascontiguousarray(w)).to(engine.ntt.devices[d]))
    return _edge_pt(engine, data, level, "mult")


def edge_key(engine, pattern, seed=0, origin="key switch key"):
    """utils.synth.key_switch_key (same layout, _remember_pack called the same way) with the lazy words of
    edge_rows(.., lazy=True): "top" is 2q - 1 everywhere."""
    import torch
    from liberate_fhe_amd.utils.synth import _data_struct
    ds_type = _data_struct(engine)
    q, N, p = engine.ctx.q, engine.ctx.N, engine.ntt.p
    nparts = p.num_partitions + 1
    packs = []
    for d in _edge_ids(engine):
        dest = p.destination_arrays_with_special[0][d]
        pack = np.empty((nparts, 2, len(dest), N), dtype=np.int64)
        for gid in range(nparts):
            for comp in range(2):
                pack[gid, comp] = edge_rows([q[i] for i in dest], N, pattern, seed * 4096 + gid * 2 + comp, lazy=True,
                                            ids=[i + gid + comp for i in dest] if pattern == "mixed" else dest)
        packs.append(torch.from_numpy(pack).to(engine.ntt.devices[d]))
    parts = []
    for gid in range(nparts):
        parts.append(ds_type(data=([pk[gid, 0] for pk in packs], [pk[gid, 1] for pk in packs]), include_special=True,
                             ntt_state=True, montgomery_state=True, origin=f"key switch key part index {gid}",
                             level=0, hash=engine.hash, version=engine.version))
    out = ds_type(data=parts, include_special=True, ntt_state=True, montgomery_state=True, origin=origin,
                  level=0, hash=engine.hash, version=engine.version)
    if hasattr(engine, "_remember_pack"):
        engine._remember_pack(out, packs, own=True)
    return out


def edge_diagonals(engine, level, steps, pattern, seed=0, n1=None):
    """utils.synth.diagonals (n1 given: utils.synth.diagonals_bsgs: steps taken mod num_slots, the baby-step / giant-step
    tag) — same layout, same origin tags, _remember_diag_pack called the same way — with the lazy words of
    edge_rows(.., lazy=True) over the ordinary and the special rows of `level`: "top" is 2q - 1 everywhere.  The row ids are
    shifted by the diagonal's index in the pack ("mixed" then gives every diagonal another rotation of the four patterns,
    "random" another stream); a word follows its prime's id, not the device that holds it."""
    import torch
    from liberate_fhe_amd.utils.synth import _data_struct
    ds_type = _data_struct(engine)
    q, N, p = engine.ctx.q, engine.ctx.N, engine.ntt.p
    steps = sorted(int(s) if n1 is None else int(s) % engine.num_slots for s in steps)
    packs = []
    for d in _edge_ids(engine):
        dest = p.destination_arrays_with_special[level][d]
        pack = np.empty((len(steps), len(dest), N), dtype=np.int64)
        for j in range(len(steps)):
            pack[j] = edge_rows([q[i] for i in dest], N, pattern, seed * 8192 + steps[j], lazy=True, ids=[i + j for i in dest])
        packs.append(torch.from_numpy(pack).to(engine.ntt.devices[d]))
    tag = "plain diagonals:" if n1 is None else f"plain diagonals bsgs:{int(n1)};"
    out = ds_type(data=[[pk[j] for pk in packs] for j in range(len(steps))], include_special=True, ntt_state=True,
                  montgomery_state=True, origin=tag + ",".join(str(s) for s in steps), level=level,
                  hash=engine.hash, version=engine.version)
    if hasattr(engine, "_remember_diag_pack"):
        engine._remember_diag_pack(out, packs, own=True)   # the rows are views of the packs
    return out


# ---- operands that take the fp64-class inner sums to the bound their range arguments name (tests/test_worst_case_sums_*.py) ----
def constant_ciphertext(engine, level, seed=0):
    """A ciphertext of CONSTANT polynomials: coefficient 0 is a non-zero word on every row, every other coefficient is 0.  Its
    transforms are one constant per row, and a Galois rotation leaves it unchanged, so extended_constants() serve every key.
    Component 1 holds the small word 1 + (seed + prime id) % 4: with digits of one limb the plain extended digit IS that word
    on every row, which keeps the fp64 quotient of (digit word x key word) / q away from the rounding seam at the products
    +-(q - 1) / 2 that extreme_key() asks for.  Component 0 holds (q - 1) (P R)^-1: P c0 in Montgomery form, the word the
    kernels gather and add, is then q - 1 mod q — the top of its range."""
    import torch
    q, N, p = engine.ctx.q, engine.ctx.N, engine.ntt.p
    dest = p.destination_arrays[level]
    K = engine.ntt.num_special_primes
    P = 1
    for i in p.destination_arrays_with_special[level][0][-K:]:
        P *= int(q[i])
    data = []
    for comp in range(2):
        rows = []
        for d in _edge_ids(engine):
            if d < len(dest):
                w = np.zeros((len(dest[d]), N), dtype=np.int64)
                for r, i in enumerate(dest[d]):
                    m = int(q[i])
                    w[r, 0] = (m - 1) * pow(P * R, -1, m) % m if comp == 0 else 1 + (seed + i) % 4
                rows.append(torch.from_numpy(w).to(engine.ntt.devices[d]))
        data.append(rows)
    return _edge_ct(engine, data, level)


def extended_constants(engine, ct):
    """[parts][rows] Python integers: the extended digits of a constant_ciphertext in the NTT domain — pre_extend -> extend -> ntt
    of component 1, as tests/test_inner_sum_cpu.composition forms them — which are one constant along the index per (part, row):
    Montgomery-form words below 2q.  One device, a checker engine (the steps run on the CPU)."""
    import torch
    d, level = 0, ct.level
    ell = engine._rows(d, level, False)
    c1 = torch.empty_like(ct.data[1][0])
    engine.backend.galois(ct.data[1][0].contiguous(), c1, ell, engine.ctx.logN, 1, engine._vec("_2q", d, level, False))
    out = []
    for part_id in range(len(engine.ntt.p.p[level][d])):
        ext = engine.extend(engine.pre_extend([c1], d, level, part_id), d, level, part_id, d)
        engine.ntt.ntt([ext], level, d, -2)
        assert bool((ext == ext[:, :1]).all()), ("extended digits of a constant polynomial vary along the index", part_id)
        out.append([int(v) for v in ext[:, 0]])
    return out


def extreme_key(engine, ext_constants, origin="key switch key", flip=False):
    """A key-switch key (edge_key's layout, _remember_pack called the same way) under which EVERY product of the inner sums of
    the ciphertext that ext_constants came from (extended_constants at level 0) sits at the end of the balanced range: the word
    at (part p, component c, row r) is t R e[p, r]^-1 mod q_r, so that mont_mult(e, word) — and the fp64 kernels' plain product
    (e R^-1) x word — has the residue t = +-(q_r - 1) / 2: + where the Thue-Morse parity of the coefficient index is 0 in
    component 0, the opposite sign in component 1, all four swapped by `flip`.  Two values per (part, component, row),
    broadcast along the index; odd rows hold the lazy representative word + q.  One device.  The rows and parts of a later level
    are a sub-block of level 0's, and a rotation leaves a constant polynomial unchanged: the one pack serves every level and
    every step (key._replace(origin=..) shares it, 138 MB at 32 digits, instead of copying it)."""
    import torch
    from liberate_fhe_amd.utils.synth import _data_struct
    ds_type = _data_struct(engine)
    q, N, p = engine.ctx.q, engine.ctx.N, engine.ntt.p
    nparts = p.num_partitions + 1
    assert len(_edge_ids(engine)) == 1 and len(ext_constants) == len(engine.parts_alloc[0][0])
    dest = p.destination_arrays_with_special[0][0]
    tm = torch.from_numpy(thue_morse(N)).bool()
    vals = np.zeros((nparts, 2, len(dest), 2), dtype=np.int64)             # [.., 0]: parity 0, [.., 1]: parity 1
    for part_id, gid in enumerate(engine.parts_alloc[0][0]):
        for r, i in enumerate(dest):
            m = int(q[i])
            for comp in range(2):
                for par in range(2):
                    sign = -1 if (comp + par + int(flip)) % 2 else 1
                    t = sign * ((m - 1) // 2)
                    vals[gid, comp, r, par] = t * R * pow(int(ext_constants[part_id][r]), -1, m) % m + (m if r % 2 else 0)
    v = torch.from_numpy(vals)
    pack = torch.where(tm.view(1, 1, 1, N), v[..., 1:2], v[..., 0:1]).contiguous().to(engine.ntt.devices[0])
    parts = [ds_type(data=([pack[gid, 0]], [pack[gid, 1]]), include_special=True, ntt_state=True, montgomery_state=True,
                     origin=f"key switch key part index {gid}", level=0, hash=engine.hash, version=engine.version)
             for gid in range(nparts)]
    out = ds_type(data=parts, include_special=True, ntt_state=True, montgomery_state=True, origin=origin,
                  level=0, hash=engine.hash, version=engine.version)
    if hasattr(engine, "_remember_pack"):
        engine._remember_pack(out, [pack], own=True)
    return out


def pre_rescale_rows(q_rows, q_drop, target_rows, row0):
    """The words a_i = ((t_i - rho) q_drop + r) mod q_i whose rescale (a_i - r) q_drop^-1 + rho is t_i, with r = row0 the
    dropped limb's words and rho = [r > q_drop // 2]; Python integers."""
    q_drop = int(q_drop)
    r = [int(x) for x in row0]
    rho = [int(x > q_drop // 2) for x in r]
    out = np.empty((len(q_rows), len(r)), dtype=np.int64)
    for i, q in enumerate(q_rows):
        q = int(q)
        out[i] = [((int(t) - h) * q_drop + x) % q for t, h, x in zip(target_rows[i], rho, r)]
    return out


def pre_rescale(engine, level, target_rows, row0):
    """One polynomial of a level-`level` ciphertext — a list of [rows, N] arrays, one per device alive at `level`, in the
    engine's layout — whose rescale to level + 1 leaves the words target_rows[d] ([surviving rows of device d, N]) when the
    dropped limb holds row0 ([N] words below the dropped prime).  A ciphertext of edge words does not survive the rescale
    cc_mult opens with (all limbs at q_i - 1 are the integer -1 and rescale to zero), so the operands of every case that
    goes through a rescale are built backwards with this."""
    q = engine.ctx.q
    dest = engine.ntt.p.destination_arrays[level]
    owner = engine.ntt.p.rescaler_loc[level]
    q_drop = q[dest[owner][0]]
    out = []
    for d in range(len(dest)):
        keep = dest[d][1:] if d == owner else dest[d]
        t = np.asarray(target_rows[d]) if len(keep) else np.empty((0, len(row0)), dtype=np.int64)
        body = pre_rescale_rows([q[i] for i in keep], q_drop, t, row0)
        out.append(np.concatenate([np.asarray(row0, dtype=np.int64)[None, :], body]) if d == owner else body)
    return out


def pre_rescale_ciphertext(engine, level, pattern, seed=0, shift=0):
    """A level-`level` ciphertext whose rescale leaves edge_rows(pattern) at level + 1 (see edge_ciphertext for the second
    component), with rounder_row0 in the dropped limb of both components."""
    import torch
    q, N = engine.ctx.q, engine.ctx.N
    dest = engine.ntt.p.destination_arrays[level]
    owner = engine.ntt.p.rescaler_loc[level]
    q_drop = q[dest[owner][0]]
    data = []
    for comp in range(2):
        # (the words are Python-integer work: the HIP engine and the checker engine of one test share them)
        key = (engine.hash, len(dest), str(dest), level, pattern, seed, shift, comp)
        rows = _PRE_RESCALE_CACHE.get(key)
        if rows is None:
            pat = pattern if comp == 0 or pattern in ("mixed", "random") else \
                ENGINE_EDGE_PATTERNS[(ENGINE_EDGE_PATTERNS.index(pattern) + 1) % 4]
            targets = []
            for d in range(len(dest)):
                keep = dest[d][1:] if d == owner else dest[d]
                ids = [i + comp for i in keep] if pattern == "mixed" else keep
                targets.append(edge_rows([q[i] for i in keep], N, pat, seed * 2 + comp, ids=ids))
            rows = _PRE_RESCALE_CACHE[key] = pre_rescale(engine, level, targets, rounder_row0(q_drop, N, shift + 2 * comp))
        data.append([torch.from_numpy(rows[d].copy()).to(engine.ntt.devices[d]) for d in _edge_ids(engine) if d < len(dest)])
    return _edge_ct(engine, data, level)


_PRE_RESCALE_CACHE = {}


# ---- the engine's step kernels on hand-made operands ------------------------------------------------------------------
def edge_param_sets():
    """name -> engine parameters of tests/test_engine_edges_*.py (the ring is small: the point is arithmetic, not size)."""
    base = dict(logN=13, is_secured=False)
    sets = {f"sb40_K{K}": dict(base, scale_bits=40, num_scales=9, num_special_primes=K) for K in (1, 5, 7, 8)}
    sets.update({f"sb41_K{K}": dict(base, scale_bits=41, num_scales=6, num_special_primes=K) for K in (2, 4)})
    sets["sb45_K4"] = dict(base, scale_bits=45, num_scales=6, num_special_primes=4)
    sets["sb45_K8"] = dict(base, scale_bits=45, num_scales=9, num_special_primes=8)     # 9 scales: a digit of 8 wide limbs
    sets["sb20"] = dict(base, scale_bits=20, num_scales=8, num_special_primes=2)
    # the deep set: 32 digits of one limb at level 0, 33 rows of which 31 are fp64-class (tests/test_worst_case_sums_*.py)
    sets["sb40_K1_d32"] = dict(base, scale_bits=40, num_scales=31, num_special_primes=1)
    return sets


class StepTables:
    """What the backend's step methods take, from an engine's own per-level tables (one device)."""

    def __init__(self, eng, level, d=0):
        self.eng, self.level, self.d = eng, level, d
        self.dev = eng.ntt.devices[d]
        self.N, self.logN, self.K = eng.ctx.N, eng.ctx.logN, eng.ntt.num_special_primes
        self.rows, self.ell = eng._rows(d, level, True), eng._rows(d, level, False)
        self.c_ord, self.c_all = eng._consts(d, level, False), eng._consts(d, level, True)
        tabs = self.tabs = eng._ks_tables(level)
        self.n_digits, self.d_desc, self.d_tab = tabs[("digits", d)]
        self.e_desc, self.E, self.Ed = tabs[("extend", d)]
        self.nparts, self.first_part, self.row_off = len(tabs["order"]), tabs["first_part"], eng.ntt.starts[level][d]
        self.pir, self.pip, self.own = tabs[("pir", d)], tabs[("pip", d)], tabs[("own", d)]
        self.Rs_all, self.Rs_ord = eng._vec("Rs", d, level, True), eng._vec("Rs", d, level, False)
        self.q2_ord = eng._vec("_2q", d, level, False)
        self.psi, self.ipsi = eng._tw(d, level, True), eng._tw(d, level, True, True)
        self.psi_ord, self.ipsi_ord = eng._tw(d, level, False), eng._tw(d, level, False, True)
        self.ninv, self.ninv_ord = eng._vec("Ninv", d, level, True), eng._vec("Ninv", d, level, False)
        ids = eng.ntt.p.destination_arrays_with_special[level][d]
        self.ids_all, self.ids_ord = list(ids), list(ids[:self.ell])
        self.q_all = [int(eng.ctx.q[i]) for i in ids]
        self.q_ord = self.q_all[:self.ell]
        self.order = [(rows, [int(eng.ctx.q[i]) for i in primes]) for _, rows, primes in tabs["order"]]

    def put(self, x):
        import torch
        return torch.from_numpy(np.ascontiguousarray(x)).to(self.dev)

    def new(self, *shape):
        """An output buffer pre-filled with -1 with one guard entry behind the last one along the first dimension (a row of
        a polynomial, a polynomial of a stack): `body` is what the call gets, `guard_ok` is asked afterwards."""
        import torch
        return torch.full((shape[0] + 1,) + tuple(shape[1:]), -1, dtype=torch.int64, device=self.dev)


def body(buf):
    return buf[:-1]


def guard_ok(buf):
    return bool((buf[-1] == -1).all())


DIGIT_WORD_BOUND = (1 << 43) - 1      # csrc/ckks_ks.hip: "signed digit words (|y| < 2^43)" of digits made of fp64-class limbs


def step_operands(T, pattern, key_pattern, seed, N=None):
    """The operands of one case of the step kernels, as host arrays (the HIP side and the checker side get copies):
      a         [ell, N]  canonical coefficient words: the polynomial a key switch decomposes
      x         [4, ell, N] lazy NTT-domain words: the operands of the tensor product (x0, x1, y0, y1)
      state_hi  [ell, N]  digit words AT the bound the extension kernels document: +-(2^43 - 1) by the Thue-Morse parity in
                digits whose limbs are all below 2^41, +-(2q - 1) in the others
      ext       [nparts, rows, N] lazy words: extended digits in the NTT domain, Montgomery form
      key       [parts, 2, rows0, N] lazy key words (key_pattern)
      s         [2, rows, N] canonical words: the sums a mod-down divides by P
      add       [2, ell, N] canonical addends"""
    N = T.N if N is None else N
    op = {"a": edge_rows(T.q_ord, N, pattern, seed, ids=T.ids_ord),
          "x": np.stack([edge_rows(T.q_ord, N, pattern, seed + 1 + i, lazy=True, ids=[j + i for j in T.ids_ord]) for i in range(4)]),
          "ext": np.stack([edge_rows(T.q_all, N, pattern, seed + 10 + p, lazy=True, ids=[j + p for j in T.ids_all])
                           for p in range(T.nparts)]),
          "s": np.stack([edge_rows(T.q_all, N, pattern, seed + 30 + c, ids=[j + c for j in T.ids_all]) for c in range(2)]),
          "add": np.stack([edge_rows(T.q_ord, N, pattern, seed + 40 + c, ids=[j + 1 + c for j in T.ids_ord]) for c in range(2)])}
    q0 = T.eng.ctx.q
    ids0 = T.eng.ntt.p.destination_arrays_with_special[0][T.d]
    nk = T.eng.ntt.p.num_partitions + 1
    op["key"] = np.stack([np.stack([edge_rows([q0[i] for i in ids0], N, key_pattern, seed + 50 + 2 * g + c, lazy=True,
                                              ids=[j + g + c for j in ids0]) for c in range(2)]) for g in range(nk)])
    sign = 1 - 2 * thue_morse(N)
    hi = np.empty((T.ell, N), dtype=np.int64)
    for rows, primes in T.order:
        small = all(m < SMALL_PRIME_LIMIT for m in primes)
        for r, m in zip(rows, primes):
            hi[r] = sign * (DIGIT_WORD_BOUND if small else 2 * m - 1)
    op["state_hi"] = hi
    return op


# ---- fenced scratch and outputs of the native op entries (tests/test_fenced_ops_*.py) ------------------------------------
# every HipBackend method that takes `out` or `outs`: the whole ops behind one native call
NATIVE_ENTRIES = ("switch_key_native", "cc_mult_evk", "switch_key_batch_native", "cc_mult_evk_batch_native", "cc_dot_native",
                  "cc_dot_batch_native", "cc_matmul_native", "weighted_sums_native", "pc_dot_native", "pc_matmul_native",
                  "pc_matmul_batch_native", "rotate_hoisted_native", "linear_transform_native", "linear_transform_batch_native",
                  "rotate_sum_native", "rotate_sum_batch_native", "linear_transform_bsgs_native",
                  "linear_transform_bsgs_batch_native", "lt_matmul_native", "lt_matmul_batch_native", "lt_matmul_bsgs_native")
# the halves of a limb-sharded op around the digit exchange (one process per GPU): the two that take `out` get fenced outputs (out
# may be None: which = 1 writes plan scratch only), the three that take none get the guard check of all scratch on the way out
HALF_ENTRIES = ("cc_mult_pre", "switch_key_pre", "plan_fwd", "cc_mult_post", "switch_key_post")
# the hostile fills of scratch bodies and outputs: every bit set (-1 as a word, a NaN as fp64, 0xFF in every plane byte), the
# largest word, seeded uniform 64-bit words.  Zero — what a fresh process often finds in new pages — is the friendly case.
FENCE_FILLS = {"ones": -1, "max": (1 << 63) - 1, "random": "random"}


class FenceError(AssertionError):
    pass


class _Fenced:
    """guard | body | guard inside one allocation; `flat` is the body's span of words, `body` the view the code under test gets"""
    __slots__ = ("key", "buf", "flat", "body", "salts", "target")

    def __init__(self, key, buf, flat, body, salts, target=None):
        self.key, self.buf, self.flat, self.body, self.salts, self.target = key, buf, flat, body, salts, target


class Fence:
    """Guards around every scratch tensor and every output of an engine's native op entries, and a hostile fill inside them.
    Installed on a FRESH engine (before its first op; the engine and its backend keep the wrappers for good):

      scratch   engine._ws is wrapped: every scratch tensor the engine ever asks for — the plan's state / ext / sum / md_ws / x4 /
                d2 and every op workspace, of every lane — is the middle view(shape) of a larger allocation.  cc_matmul keeps its
                growing workspace outside _ws: backend.cc_matmul_native is handed a fenced one of exactly
                cc_matmul_ws_words(plan, nu) words instead.
      outputs   every method of NATIVE_ENTRIES and HALF_ENTRIES the backend has is wrapped: the tensors of its `out` / `outs` argument (found by
                name in the signature, nested lists walked) are replaced by fenced views of the same shape and strides; after the
                call the guards of the outputs AND of all scratch are checked and the bodies copied into the engine's own tensors.
                `calls` lists the entries that ran, in order.  A half without `out`, or handed out = None, gets the guard check of
                all scratch on the way out.  A half called inside a stream capture is passed through unchecked (a guard check
                reads the device, which a capture forbids).
      guards    `guard` words before and behind each body: one polynomial of level 0's full row count, (ell + K) N words, an even
                count (the body stays 16-byte aligned).  They hold a seeded, position-dependent 64-bit pattern XORed with a salt of
                their own; check() compares them with the kept pattern and raises FenceError naming the buffer's key, the side
                ("before": offset 1 is the word next to the body; "behind": offset 0 is) and the first changed word.
      fill      bodies are pre-filled with `fill` (an int, or "random": seeded uniform 64-bit words); refill() puts it back into
                every scratch body before a case — except the buffers that hold constants across calls: whatever is handed to
                backend.moddown_consts and the md_ws of backend.make_plan (both wrapped to learn them).  The scratch part of those
                keeps what the previous call left.
      ws_hook   None, or f(name, arguments: dict) called after the outputs are fenced and before the entry runs: it may replace
                arguments (tests/test_fenced_ops_gpu.py: a workspace one word short, a misaligned one)."""

    def __init__(self, engine, fill, seed=20240229):
        import inspect

        import torch
        self.torch, self.eng, self.be, self.fill = torch, engine, engine.backend, fill
        assert not engine._workspace and not any(k[0] == "plan" for k in engine._tables if isinstance(k, tuple)), \
            "Fence: the engine has run an op already"
        N = engine.ctx.N
        self.guard = max(engine._rows(d, 0, True) for d in range(engine.ntt.num_devices)) * N
        assert self.guard >= 2 and self.guard % 2 == 0
        self._rng, self._seed = {}, seed     # device -> its generator
        self._pattern = {}            # device -> the [guard] words every guard is a salted copy of
        self._salt = 0
        self.scratch, self.calls, self.const_ptrs, self.ws_hook = {}, [], set(), None
        self.last_outputs, self.never_written = [], []     # of the last call / of every call since the list was emptied
        self._matmul_ws = {}
        real_ws = engine._ws

        def fenced_ws(key, shape, dev_id):
            k = (key, tuple(shape), dev_id, engine._lane)
            if k not in engine._workspace:
                f = self.alloc(k, tuple(shape), None, engine.ntt.devices[dev_id])
                self.scratch[k] = f
                engine._workspace[k] = f.body
            return real_ws(key, shape, dev_id)

        engine._ws = fenced_ws
        for name in ("moddown_consts", "make_plan"):
            if hasattr(self.be, name):
                setattr(self.be, name, self._learn_consts(name, getattr(self.be, name)))
        for name in NATIVE_ENTRIES + HALF_ENTRIES:
            if hasattr(self.be, name):
                real = getattr(self.be, name)
                setattr(self.be, name, self._fenced_entry(name, real, inspect.signature(real)))

    # -- allocation, fill, check ------------------------------------------------------------------------------------------
    def _words(self, n, device):
        """n seeded uniform 64-bit words, drawn on `device`"""
        rng = self._rng.get(str(device))
        if rng is None:
            rng = self._rng[str(device)] = self.torch.Generator(device=device).manual_seed(self._seed)
        return self.torch.randint(-(1 << 63), (1 << 63) - 1, (n,), dtype=self.torch.int64, device=device, generator=rng)

    def pattern(self, device):
        p = self._pattern.get(str(device))
        if p is None:
            p = self._pattern[str(device)] = self._words(self.guard, device)
        return p

    def _put_fill(self, flat):
        if self.fill == "random":
            flat.copy_(self._words(flat.numel(), flat.device))
        else:
            flat.fill_(self.fill)

    def alloc(self, key, shape, strides, device, target=None):
        """a fenced tensor of `shape` (strides None: contiguous), the body pre-filled with the fill"""
        torch, G = self.torch, self.guard
        if strides is None:
            strides, n = [], 1
            for s in reversed(shape):
                strides.insert(0, n)
                n *= s
        span = 0 if any(s == 0 for s in shape) else 1 + sum((s - 1) * st for s, st in zip(shape, strides))
        buf = torch.empty(2 * G + span, dtype=torch.int64, device=device)
        salts = []
        for lo in (0, G + span):
            self._salt += 1
            salt = (self._salt * 0x9E3779B97F4A7C15) & ((1 << 64) - 1)
            salts.append(salt - (1 << 64) if salt >> 63 else salt)
            buf[lo:lo + G] = self.pattern(device) ^ salts[-1]
        flat = buf[G:G + span]
        self._put_fill(flat)
        return _Fenced(key, buf, flat, buf.as_strided(tuple(shape), tuple(strides), G), salts, target)

    def check_one(self, f):
        G, pat = self.guard, self.pattern(f.buf.device)
        for side, lo, salt in (("before", 0, f.salts[0]), ("behind", f.buf.numel() - G, f.salts[1])):
            got = f.buf[lo:lo + G] ^ salt
            if not self.torch.equal(got, pat):
                at = int((got != pat).nonzero()[0])
                off = G - at if side == "before" else at
                raise FenceError(f"{f.key}: the guard {side} the buffer was written, first changed word at offset {off} "
                                 f"({int((got != pat).sum())} of {G} words changed)")

    def check(self, outputs=()):
        """the guards of `outputs` and of every scratch buffer"""
        for f in list(outputs) + list(self.scratch.values()):
            self.check_one(f)

    def refill(self):
        for f in self.scratch.values():
            if f.body.data_ptr() not in self.const_ptrs:
                self._put_fill(f.flat)

    def holds_fill(self, f):
        """whether a body still holds an int fill everywhere (nothing was written: the refusal tests)"""
        assert self.fill != "random"
        return bool((f.flat == self.fill).all())

    def unwritten(self):
        """the keys of the last call's outputs that still hold an int fill in EVERY word: the entry never wrote them (no result
        is -1 or 2^63 - 1 everywhere); [] under the random fill, where the comparison across fills shows it"""
        return [] if self.fill == "random" else [f.key for f in self.last_outputs if self.holds_fill(f)]

    # -- the wrappers -----------------------------------------------------------------------------------------------------
    def _capturing(self):
        cuda = self.torch.cuda
        return bool(cuda.is_available() and hasattr(cuda, "is_current_stream_capturing") and cuda.is_current_stream_capturing())

    def _learn_consts(self, name, real):
        def learning(*args, **kw):
            if name == "moddown_consts":
                self.const_ptrs.add((kw["ws"] if "ws" in kw else args[0]).data_ptr())
            else:
                md = (kw["tensors"] if "tensors" in kw else args[1]).get("md_ws")
                if md is not None:
                    self.const_ptrs.add(md.data_ptr())
            return real(*args, **kw)
        return learning

    def _fence_outputs(self, name, x, path, made):
        """the nested lists / tuples of `x` with every tensor replaced by a fenced view of the same shape and strides"""
        if isinstance(x, self.torch.Tensor):
            f = self.alloc((name, "out") + path, tuple(x.shape), tuple(x.stride()), x.device, target=x)
            made.append(f)
            return f.body
        if isinstance(x, (list, tuple)):
            return type(x)(self._fence_outputs(name, v, path + (i,), made) for i, v in enumerate(x))
        return x

    def _fenced_entry(self, name, real, sig):
        which = [p for p in ("out", "outs") if p in sig.parameters]
        assert len(which) == (0 if name in HALF_ENTRIES[:3] else 1), (name, which)

        def entry(*args, **kw):
            if name in HALF_ENTRIES and self._capturing():
                # a half inside a stream capture (ckks_engine._sharded_segments: plan addresses only, out is None): a guard
                # check reads the device, which a capture forbids; the replays are checked by whoever issued them (check())
                return real(*args, **kw)
            bound = sig.bind(*args, **kw)
            bound.apply_defaults()
            a = bound.arguments
            self.calls.append(name)
            made = []
            if which:
                a[which[0]] = self._fence_outputs(name, a[which[0]], (), made)
            if name == "cc_matmul_native":      # its workspace only grows: a fenced one of exactly the words this call needs
                words = self.be.cc_matmul_ws_words(a["plan"], len(a["ins"]) // 2)
                k = ("cc_matmul_ws", words, str(a["ws"].device))
                if k not in self.scratch:
                    self.scratch[k] = self.alloc(k, (words,), None, a["ws"].device)
                a["ws"] = self.scratch[k].body
            self.last_outputs = made
            if self.ws_hook is not None:
                self.ws_hook(name, a)
            ret = real(*bound.args, **bound.kwargs)
            self.check(made)
            self.never_written += self.unwritten()
            for f in made:
                f.target.copy_(f.body)
            return ret
        return entry


def tensors_of(x, out=None):
    """every tensor reachable from x through lists, tuples, dicts and the `data` of data_struct objects, in order"""
    import torch
    out = [] if out is None else out
    if isinstance(x, torch.Tensor):
        out.append(x)
    elif hasattr(x, "origin") and hasattr(x, "data"):
        tensors_of(x.data, out)
    elif isinstance(x, dict):
        for k in sorted(x, key=str):
            tensors_of(x[k], out)
    elif isinstance(x, (list, tuple)):
        for v in x:
            tensors_of(v, out)
    return out


class Untouched:
    """Clones of every tensor of the operands (ciphertext components, key parts, diagonals, plaintexts) taken before a call;
    check(what) afterwards fails with the operand's name and the first changed word."""

    def __init__(self, **operands):
        self.kept = {}
        for name, x in operands.items():
            self.add(name, x)

    def add(self, name, x):
        seen = {}
        for t in tensors_of(x):
            seen.setdefault((t.data_ptr(), tuple(t.shape), tuple(t.stride())), t)
        self.kept[name] = [(t, t.clone()) for t in seen.values()]

    def check(self, what=""):
        import torch
        for name, pairs in self.kept.items():
            for i, (t, c) in enumerate(pairs):
                if not torch.equal(t, c):
                    bad = (t != c).nonzero()
                    raise AssertionError(f"{what}: operand {name!r} was modified (tensor {i}): {len(bad)} words, first at "
                                         f"{tuple(int(v) for v in bad[0])}")


# ---- held streams (tests/test_stream_contract_gpu.py) -------------------------------------------------------------------------
# The engine's stream contract is about what happens while a stream is BUSY: a test that enqueues ops back to back on idle
# streams passes whenever the kernels happen not to overlap.  hold() makes a stream busy for a known time with the project's own
# one-wave spin kernel (lf_clock_probe: bounded, one wave, 16 bytes of output), so "B waited for A" and "B did not wait for A"
# become two event queries.
_HOLD_OUT, _INDEPENDENT = {}, {}


def hold(stream, ms):
    """Keeps `stream` busy for `ms` milliseconds (ms * 100_000 ticks of the constant 100 MHz counter) from the moment the
    spin kernel starts; returns an event recorded right behind it."""
    import torch

    from liberate_fhe_amd._native import check, lib
    dev = stream.device
    out = _HOLD_OUT.get(dev)
    if out is None:
        out = _HOLD_OUT[dev] = torch.zeros(2, dtype=torch.int64, device=dev)      # (every hold writes the same 16 bytes)
        torch.cuda.synchronize(dev)
    check(lib.lf_clock_probe(out.data_ptr(), 1, int(ms * 100_000), dev.index, stream.cuda_stream), "lf_clock_probe")
    ev = torch.cuda.Event()
    ev.record(stream)
    return ev


def still_held(ev):
    return not ev.query()


def hold_report(stream, ms):
    """One hold of `ms` on `stream`, taken apart, as text for a failure message: how long the enqueue kept the host, when the event
    behind the spin kernel reported completion, and what the kernel itself counted.  A pair of streams on one hardware queue shows
    waits of about `ms`; waits near zero mean the hold did not hold, and these three figures say which way: the enqueue blocked the
    host for the hold (host ms about `ms`); the kernel ran short (ticks below ms x 100 000: the constant counter is not 100 MHz
    here); or the event completed ahead of the kernel (ticks right, event ms far below `ms`)."""
    import time

    import torch
    torch.cuda.synchronize(stream.device)
    t0 = time.perf_counter()
    ev = hold(stream, ms)
    t1 = time.perf_counter()
    first = ev.query()
    while not ev.query() and time.perf_counter() - t1 < 1.0:
        pass
    t2 = time.perf_counter()
    torch.cuda.synchronize(stream.device)
    cycles, ticks = (int(v) for v in _HOLD_OUT[stream.device].tolist())
    return (f"one more hold of {ms} ms taken apart: hold() kept the host {1e3 * (t1 - t0):.3f} ms, its event was "
            f"{'already complete' if first else 'pending'} at the first query and complete {1e3 * (t2 - t0):.3f} ms after the enqueue began, "
            f"the kernel counted {ticks} ticks of the constant counter (asked: {int(ms * 100_000)}) in {cycles} core cycles")


def independent_streams(device, hold_ms=5):
    """Two torch streams of `device` that this process's hardware queues run independently: a trivial kernel on the second
    completes while the first is held.  Streams that share a hardware queue would make every ordering check pass whatever the
    engine does.  At most 8 candidates; AssertionError (never a skip) if no pair is found.  One pair per device and process."""
    import time

    import torch
    device = torch.device(device)
    if device in _INDEPENDENT:
        return _INDEPENDENT[device]
    first = torch.cuda.Stream(device=device)
    probe = torch.zeros(64, dtype=torch.int64, device=device)
    torch.cuda.synchronize(device)
    tried = []
    for _ in range(7):
        second = torch.cuda.Stream(device=device)
        ev = hold(first, hold_ms)
        with torch.cuda.stream(second):
            probe.add_(1)
        done = torch.cuda.Event()
        done.record(second)
        t0 = time.perf_counter()
        while not done.query() and still_held(ev):
            pass
        ok = done.query() and still_held(ev)
        tried.append((second.cuda_stream, ok, round(1e3 * (time.perf_counter() - t0), 2)))
        torch.cuda.synchronize(device)
        if ok:
            _INDEPENDENT[device] = (first, second)
            return first, second
    raise AssertionError(f"independent_streams: no stream of {device} ran while another was held for {hold_ms} ms "
                         f"(stream, ran beside the hold, ms waited): {tried}; the ordering checks cannot tell anything here; "
                         f"{hold_report(first, hold_ms)}")


def zeroed_free_memory(device, nbytes):
    """Allocates and zero-fills about `nbytes` in blocks of mixed sizes and drops them WITHOUT empty_cache: what the next lazily
    built table or key pack gets from the caching allocator is then zeros (best effort), not a stale correct copy left by an
    earlier engine of the same parameters.  Zeros, not the hostile fills of Fence: an index table read before it is built must
    stay in range, so that a defect shows as wrong words and never as a wild access."""
    import torch
    sizes = (512, 4096, 1 << 16, 1 << 20, 1 << 22, 1 << 24)
    blocks, total, i = [], 0, 0
    while total < nbytes:
        n = min(sizes[i % len(sizes)], max(512, nbytes - total))
        blocks.append(torch.zeros(n, dtype=torch.uint8, device=device))
        total += n
        i += 1
    torch.cuda.synchronize(device)
    del blocks
    return total


class BackendSpy:
    """Wraps every method of a backend instance that can launch (its public instance methods) and
    torch.cuda.Stream.wait_stream while the block runs.  `log` is the sequence of
    ("call", name) and ("wait", waiting stream handle, awaited stream handle); `before(name)` — if given — runs ahead of
    every wrapped call (tests hold a stream there).  `also`: further launchers — objects or modules whose public callables
    (those named in `__all__`, where there is one) are wrapped and logged in the same way: the engine's element-wise ops go
    through `engine.ntt.ops`, not through the backend.  Plain torch ops are not seen."""
    def __init__(self, backend, before=None, also=()):
        self.backend, self.before, self.log, self._names, self._wait = backend, before, [], [], None
        self.also, self._also = tuple(also), []

    def launchers(self):
        """the backend's public instance methods (the static ones — the *_ws_words sizes, mark_planes — run on the host)"""
        import inspect
        cls = type(self.backend)
        return [n for n in dir(cls) if not n.startswith("_") and inspect.isfunction(inspect.getattr_static(cls, n))]

    def calls(self):
        return [e[1] for e in self.log if e[0] == "call"]

    def __enter__(self):
        import torch
        for name in self.launchers():
            if name in self.backend.__dict__:         # (already wrapped by someone else: leave it)
                continue
            real = getattr(self.backend, name)

            def spied(*args, _real=real, _name=name, **kw):
                if self.before is not None:
                    self.before(_name)
                self.log.append(("call", _name))
                return _real(*args, **kw)

            setattr(self.backend, name, spied)
            self._names.append(name)
        for obj in self.also:
            for name in getattr(obj, "__all__", None) or [n for n in dir(obj) if not n.startswith("_")]:
                real = getattr(obj, name)
                if not callable(real) or isinstance(real, type):
                    continue

                def spied(*args, _real=real, _name=name, **kw):
                    if self.before is not None:
                        self.before(_name)
                    self.log.append(("call", _name))
                    return _real(*args, **kw)

                setattr(obj, name, spied)
                self._also.append((obj, name, real))
        self._wait = torch.cuda.Stream.wait_stream
        spy = self

        def wait_stream(stream, other):
            spy.log.append(("wait", stream.cuda_stream, other.cuda_stream))
            return spy._wait(stream, other)

        torch.cuda.Stream.wait_stream = wait_stream
        return self

    def __exit__(self, *exc):
        import torch
        torch.cuda.Stream.wait_stream = self._wait
        for name in self._names:
            delattr(self.backend, name)
        for obj, name, real in self._also:
            setattr(obj, name, real)
        self._names, self._also = [], []
