"""mod_raise, linear_transform_conj and the coefficient / slot transforms on the GPU.  Words: lf_mod_raise (mod_raise_kernel, one
launch for a batch) against the int64 definition evaluated by the checker engine on copies of the operands, on edge words of two
parameter sets, between guards under hostile fills, with every refusal.  Meaning: the congruences of a raised ciphertext in Python
integers and the overflow bound of a sparse key; coeffs_to_slots, its round trip and its raised form against float64, beside the
error of a random dense transform of the same shape (the control).  Keys and encoded matrices are built once per process.

The plaintext polynomial P = c0 + c1 s of this engine carries scale^2 (encode's scale, and encrypt's): P = scale^2 deviations[level]
coeffs(m).  A message of |m| <= 1 at the last level is therefore far above q_b, and its residue mod q_b is uniform.  The raised tests
take |m| <= 2^-22, for which |P| <= scale^2 deviations 2^-22 < q_b (1/2 - 2^-5): no fractional part of T / q_b is then within 2^-5
of one half, which the test asserts instead of assuming."""
import warnings

import numpy as np
import pytest
import torch

from liberate_fhe_amd.fhe import encdec
from tests import helpers
from tests.helpers import Fence, FENCE_FILLS, edge_ciphertext
from tests.test_fenced_ops_gpu import assert_same, flat_words, mirror
from tests.test_mod_raise_cpu import centred, expected_rows, key_coefficients, with_base_rows

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore", category=UserWarning)

DEV = "cuda:0"
SETS = {"sb40": dict(logN=12, num_scales=5, num_special_primes=2, is_secured=False),
        "sb45": dict(helpers.edge_param_sets()["sb45_K4"])}                  # 45-bit scale primes: the integer class (word tests only)
H_WEIGHT = 32
_ENG = {}


def engines(name="sb40"):
    """(HIP engine, checker engine) of a parameter set, built once per process and kept"""
    if name not in _ENG:
        from liberate_fhe_amd.fhe import ckks_engine
        from tests.oracle_backend import OracleBackend
        _ENG[name] = (ckks_engine(devices=[DEV], **SETS[name]), ckks_engine(devices=["cpu"], backend=OracleBackend(), **SETS[name]))
    return _ENG[name]


class Spy:
    """the ciphertext count of every mod_raise_call: a silent fall-back to the torch chain shows"""

    def __init__(self, eng):
        self.eng, self.calls, self.real = eng, [], eng.backend.mod_raise_call

    def __enter__(self):
        def spied(base_rows, outs, rows, q_b, mont_one, c):
            self.calls.append(len(base_rows))
            return self.real(base_rows, outs, rows, q_b, mont_one, c)
        self.eng.backend.mod_raise_call = spied
        return self

    def __exit__(self, *exc):
        del self.eng.backend.mod_raise_call


def lazy(eng, ct):
    """+ q on every third coefficient of c0 and every other one of c1: lazy words below 2q"""
    q = torch.as_tensor(eng._consts(0, ct.level, False).q_host).view(-1, 1).to(ct.data[0][0].device)
    out = []
    for comp, every in ((0, 3), (1, 2)):
        t = ct.data[comp][0].clone()
        t[:, ::every] += q
        out.append([t])
    return ct._replace(data=tuple(out))


def levels_of(eng):
    top = eng.num_levels - 1
    return [0, top // 2, top - 1, top]


def operands(name):
    """edge ciphertexts of level 0, a middle level and the last two: (GPU objects, the checker's copies)"""
    key = ("ops", name)
    if key not in _ENG:
        H, _ = engines(name)
        g = []
        for level in levels_of(H):
            for i, pattern in enumerate(("top", "mixed", "random", "half")):
                ct = edge_ciphertext(H, level, pattern, seed=level + i)
                g.append(lazy(H, ct) if i % 2 else ct)
            g.append(mirror(with_base_rows(H, level, level), DEV))           # the edge values of the base row itself
        _ENG[key] = (g, [mirror(ct, "cpu") for ct in g])
    return _ENG[key]


# ---- words -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sb40", "sb45"])
def test_mod_raise_words_equal_the_definition(name):
    from liberate_fhe_amd.fhe.presets import types
    H, C = engines(name)
    g, c = operands(name)
    assert H._mod_raise_device(g[0]) == 0
    for i, (a, b) in enumerate(zip(g, c)):
        with Spy(H) as spy:
            got = H.mod_raise(a)
        assert spy.calls == [1], (i, spy.calls)                               # ONE native call
        want = C.mod_raise(b)
        assert got.level == 0 and got.origin == types.origins["ct"]
        assert not got.ntt_state and not got.montgomery_state and not got.include_special
        assert_same(flat_words(got), flat_words(want), f"{name} mod_raise operand {i} (level {a.level})")
    # the definition itself in Python integers, on the base row's edge values at the last level
    a, b = g[-1], c[-1]
    assert_same(flat_words(H.mod_raise(a)), expected_rows(C, b), f"{name} against Python integers")
    # the torch chain on the GPU (what a sharded engine runs on each device) has the same words
    H.mod_raise_native = False
    try:
        with Spy(H) as spy:
            chain = H.mod_raise(a)
        assert spy.calls == []
    finally:
        H.mod_raise_native = True
    assert_same(flat_words(chain), expected_rows(C, b), f"{name} torch chain")


@pytest.mark.parametrize("name", ["sb40", "sb45"])
@pytest.mark.parametrize("B", [1, 3, 5, 65])
def test_mod_raise_batch_of_mixed_levels(name, B):
    H, C = engines(name)
    g, c = operands(name)
    idx = [(7 * i + B) % len(g) for i in range(B)]                             # levels mixed, objects repeated
    with Spy(H) as spy:
        got = H.mod_raise_batch([g[i] for i in idx])
    cap = H.backend.mod_raise_max_cts
    assert spy.calls == [min(cap, B - i) for i in range(0, B, cap)]            # one launch per 64 ciphertexts
    want = {i: C.mod_raise(c[i]) for i in set(idx)}
    assert [o.level for o in got] == [0] * B
    assert_same(flat_words(got), flat_words([want[i] for i in idx]), f"{name} mod_raise_batch of {B}")
    ptrs = [t.data_ptr() for t in flat_words(got)]
    assert len(set(ptrs)) == len(ptrs)                                         # every output its own tensor


@pytest.mark.parametrize("name", ["sb40", "sb45"])
def test_outputs_between_guards_under_hostile_fills(name, monkeypatch):
    from liberate_fhe_amd.fhe import ckks_engine
    _, C = engines(name)
    g, c = operands(name)
    monkeypatch.setattr(helpers, "NATIVE_ENTRIES", helpers.NATIVE_ENTRIES + ("mod_raise_call",))     # for this fence alone
    F = ckks_engine(devices=[DEV], **SETS[name])
    fence = Fence(F, FENCE_FILLS["ones"])
    picked = [0, 4, len(g) - 6, len(g) - 1]
    want = [C.mod_raise(c[i]) for i in picked]
    for fill_name, fill in FENCE_FILLS.items():
        fence.fill = fill
        for i, w in zip(picked, want):
            del fence.calls[:], fence.never_written[:]
            got = F.mod_raise(g[i])
            fence.check()
            assert fence.calls == ["mod_raise_call"] and not fence.never_written, (fill_name, i, fence.calls, fence.never_written)
            assert_same(flat_words(got), flat_words(w), f"fenced operand {i} fill {fill_name}")
        del fence.calls[:], fence.never_written[:]
        got = F.mod_raise_batch([g[i] for i in picked + picked[:1]])
        fence.check()
        assert fence.calls == ["mod_raise_call"] and not fence.never_written
        assert_same(flat_words(got), flat_words(want + want[:1]), f"fenced batch fill {fill_name}")
    # a refused batch writes nothing and launches nothing
    del fence.calls[:]
    bad = g[0]._replace(ntt_state=True)
    from liberate_fhe_amd.fhe.presets import errors
    with pytest.raises(errors.NotMatchDataStructState):
        F.mod_raise_batch([g[1], bad, g[2]])
    assert fence.calls == []


def test_refusals():
    from liberate_fhe_amd.fhe.presets import errors, types
    H, _ = engines()
    g, _ = operands("sb40")
    good = g[0]
    ntt = good._replace(ntt_state=True)
    special = good._replace(include_special=True)
    triplet = good._replace(origin=types.origins["ctt"], data=tuple(good.data) + (good.data[0],))
    plain = helpers.edge_plaintext(H, 1, "top", 0, kind="add")
    kept = [t.clone() for t in flat_words(good)]
    with Spy(H) as spy:
        for bad, err in ((ntt, errors.NotMatchDataStructState), (special, errors.NotMatchDataStructState),
                         (triplet, errors.NotMatchType), (plain, errors.NotMatchType)):
            with pytest.raises(err):
                H.mod_raise(bad)
            with pytest.raises(err):
                H.mod_raise_batch([good, good, bad])
    assert spy.calls == []
    assert_same(flat_words(good), kept, "operands of a refused batch")


# ---- meaning -----------------------------------------------------------------------------------------------------------
def kron(a, b, bits=96):
    """the product of two polynomials with non-negative integer coefficients, exactly (one big-integer product)"""
    nb = bits // 8
    pack = lambda v: int.from_bytes(b"".join(int(x).to_bytes(nb, "little") for x in v), "little")
    prod = (pack(a) * pack(b)).to_bytes(2 * len(a) * nb, "little")
    return [int.from_bytes(prod[i * nb:(i + 1) * nb], "little") for i in range(2 * len(a))]


def negacyclic(a, s):
    """a * s mod X^N + 1 over Z for integer lists (a of any sign below 2^62, s in {-1, 0, 1})"""
    N = len(a)
    parts = []
    for sign_a, av in ((1, [max(x, 0) for x in a]), (-1, [max(-x, 0) for x in a])):
        for sign_s, sv in ((1, [int(x == 1) for x in s]), (-1, [int(x == -1) for x in s])):
            if any(av) and any(sv):
                parts.append((sign_a * sign_s, kron(av, sv)))
    full = [sum(sg * p[j] for sg, p in parts) for j in range(2 * N)]
    return [full[j] - full[j + N] for j in range(N)]


def world():
    """the engine's keys (a secret of weight 32, public, the rotation keys of coeff_slot_steps, conjugation), made once"""
    if "world" not in _ENG:
        H, _ = engines()
        sk = H.create_secret_key(hamming_weight=H_WEIGHT)
        pk = H.create_public_key(sk)
        n1, babies, giants = H.coeff_slot_steps()
        rotks = {s: H.create_rotation_key(sk, s) for s in sorted(set(babies + giants)) if s}
        _ENG["world"] = dict(H=H, sk=sk, pk=pk, n1=n1, rotks=rotks, conjk=H.create_conjugation_key(sk),
                             s=[int(x) for x in key_coefficients(H, sk).cpu()])
    return _ENG["world"]


def message(seed, bound=1.0):
    rng = np.random.default_rng(seed)
    n = SETS["sb40"]["logN"]
    r = bound * np.sqrt(rng.uniform(0, 1, 1 << (n - 1)))
    return r * np.exp(2j * np.pi * rng.uniform(0, 1, 1 << (n - 1)))              # |m| <= bound


def raised(seed, sk, pk, s):
    """(ciphertext at the last level, its raise, T = lift(c0) + lift(c1) s over Z) of a small message"""
    H, _ = engines()
    top = H.num_levels - 1
    assert H.final_scalar[top] is not None                                      # the last decryptable level
    ct = H.level_up(H.encorypt(message(seed, 2.0 ** -22), pk), top)
    up = H.mod_raise(ct)
    qb = H.base_prime
    _, row = H._base_row_at(top)
    v = [[centred(int(w), qb) for w in ct.data[comp][0][row].cpu()] for comp in range(2)]
    T = [a + b for a, b in zip(v[0], negacyclic(v[1], s))]
    return ct, up, T


def congruences(H, up, T, s):
    for i, p in enumerate(H.ntt.p.destination_arrays[0][0]):
        q = H.ctx.q[p]
        c0 = [int(x) for x in up.data[0][0][i].cpu()]
        c1 = [int(x) for x in up.data[1][0][i].cpu()]
        lhs = [(a + b) % q for a, b in zip(c0, negacyclic(c1, s))]
        assert lhs == [t % q for t in T], f"row {i} (prime {q}): (c0' + c1' s) != T"


def test_raised_pair_decrypts_to_the_lift_and_a_sparse_key_bounds_it():
    w = world()
    H, s = w["H"], w["s"]
    assert sum(1 for x in s if x) == H_WEIGHT
    ct, up, T = raised(11, w["sk"], w["pk"], s)
    congruences(H, up, T, s)
    qb = H.base_prime
    # the bound of ANY key of weight h: |lift(c0)| and each of the h terms of lift(c1) s are at most (q_b - 1) / 2
    assert max(abs(t) for t in T) * 2 <= (H_WEIGHT + 1) * qb
    t = [centred(x, qb) for x in T]
    I = [(x - y) // qb for x, y in zip(T, t)]
    assert all(x - y == i * qb for x, y, i in zip(T, t, I)) and max(abs(i) for i in I) <= (H_WEIGHT + 1) // 2 and any(I)
    # the plaintext mod q_b is the unraised ciphertext's: the message part survives (|P| < q_b / 2 for this message)
    want = H.decrode(ct, w["sk"])
    top = ct.level
    coeffs = np.array(t, dtype=np.float64) / (float(H.scale) ** 2 * float(H.deviations[top]))
    got = encdec.decode(torch.from_numpy(coeffs), norm=H.norm, return_without_scaling=True)[:H.num_slots].numpy()
    assert np.abs(got - want).max() < 2.0 ** -32 and np.abs(want).max() > 2.0 ** -24


def test_raised_pair_under_the_default_dense_key():
    H, _ = engines()
    sk = H.create_secret_key()
    pk = H.create_public_key(sk)
    s = [int(x) for x in key_coefficients(H, sk).cpu()]
    assert sum(1 for x in s if x) > H.ctx.N // 2
    _, up, T = raised(12, sk, pk, s)
    congruences(H, up, T, s)                                                    # only the bound differs
    assert max(abs(t) for t in T) * 2 <= (sum(1 for x in s if x) + 1) * H.base_prime


# ---- linear_transform_conj ---------------------------------------------------------------------------------------------
def test_linear_transform_conj_is_the_composition():
    from liberate_fhe_amd.fhe.presets import errors
    w = world()
    H, rotks, conjk = w["H"], w["rotks"], w["conjk"]
    n = H.num_slots
    rng = np.random.default_rng(5)
    vec = lambda: rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)
    m = message(21)
    ct = H.encorypt(m, w["pk"])
    d = H.encode_diagonals({0: vec(), 1: vec(), 5: vec(), 70: vec()}, 0, bsgs=8)
    e = H.encode_diagonals({2: vec(), 64: vec()}, 0, bsgs=8)
    assert H.linear_transform_conj_steps(d, e) == (8, [0, 1, 2, 5, 6], [0, 64])
    got = H.linear_transform_conj(ct, d, e, rotks, conjk)
    want = H.lt_matmul_bsgs([[d, e]], [ct, H.conjugate(ct, conjk)], rotks)[0]
    assert got.level == 1
    assert_same(flat_words(got), flat_words(want), "linear_transform_conj against the composition")
    assert_same(flat_words(H.linear_transform_conj(ct, d, None, rotks, conjk)), flat_words(H.lt_matmul_bsgs([[d]], [ct], rotks)[0]),
                "diags_conj=None")
    assert_same(flat_words(H.linear_transform_conj(ct, None, e, rotks, conjk)),
                flat_words(H.lt_matmul_bsgs([[None, e]], [ct, H.conjugate(ct, conjk)], rotks)[0]), "diags_z=None")
    # what it decrypts to
    dz = {0: vec(), 3: vec()}
    dc = {1: vec()}
    out = H.decrode(H.linear_transform_conj(ct, dz, dc, rotks, conjk, n1=8), w["sk"])
    ref = sum(v * np.roll(m, s) for s, v in dz.items()) + sum(v * np.roll(m.conj(), s) for s, v in dc.items())
    assert np.abs(out - ref).max() < 1e-6
    # a missing key is named by its step
    fewer = {s: k for s, k in rotks.items() if s != 5}
    with pytest.raises(errors.NotMatchType, match="step 5"):
        H.linear_transform_conj(ct, d, e, fewer, conjk)
    with pytest.raises(ValueError):
        H.linear_transform_conj(ct, None, None, rotks, conjk)


# ---- coefficients <-> slots ----------------------------------------------------------------------------------------------
def control_pair(M1, M2, seed):
    """a random dense pair with the row sums of |entry| of (M1, M2)"""
    rng = np.random.default_rng(seed)
    out = []
    for M in (M1, M2):
        G = rng.normal(size=M.shape) + 1j * rng.normal(size=M.shape)
        out.append(G * (np.abs(M).sum(axis=1) / np.abs(G).sum(axis=1))[:, None])
    return out


def control_error(ct, G1, G2, ideal, seed_tag):
    """max error of lt_matmul_bsgs([[G1, G2]], [ct, conj ct]) against numpy float64 on the ideal input: the same key switches,
    products and one rescale as the transform it stands beside"""
    w = world()
    H = w["H"]
    key = ("control", seed_tag, ct.level)
    if key not in _ENG:
        _ENG[key] = [H.encode_diagonals(encdec.matrix_diagonals(G), ct.level, bsgs=w["n1"]) for G in (G1, G2)]
    out = H.lt_matmul_bsgs([_ENG[key]], [ct, H.conjugate(ct, w["conjk"])], w["rotks"])[0]
    return float(np.abs(H.decrode(out, w["sk"]) - (G1 @ ideal + G2 @ ideal.conj())).max())


def packed_coefficients(H, m, level=0):
    t = encdec.encode(m, device="cpu", norm=H.norm, return_without_scaling=True).numpy()
    return t[:H.num_slots] + 1j * t[H.num_slots:]


def transforms():
    """one run of everything the error tests compare, shared between them"""
    if "transforms" not in _ENG:
        w = world()
        H, sk, rotks, conjk = w["H"], w["sk"], w["rotks"], w["conjk"]
        B, C, E, F = encdec.coeff_slot_matrices(H.ctx.N, H.norm)
        m = message(31)
        ct = H.encorypt(m, w["pk"])
        u = packed_coefficients(H, m)
        c2s = H.coeffs_to_slots(ct, rotks, conjk)
        back = H.slots_to_coeffs(c2s, rotks, conjk)
        r = dict(m=m, u=u, ct=ct, c2s=c2s, back=back)
        r["c2s_err"] = float(np.abs(H.decrode(c2s, sk) - u).max())
        r["back_err"] = float(np.abs(H.decrode(back, sk) - m).max())
        r["ctrl1"] = control_error(ct, *control_pair(B, C, 41), m, "c2s")
        r["ctrl2"] = control_error(c2s, *control_pair(E, F, 42), u, "s2c")
        print(f"\ncoeffs_to_slots max error {r['c2s_err']:.3e} | control {r['ctrl1']:.3e};  round trip {r['back_err']:.3e} | "
              f"controls {r['ctrl1']:.3e} + {r['ctrl2']:.3e}")
        _ENG["transforms"] = r
    return _ENG["transforms"]


def test_coeffs_to_slots_default_divisor():
    H, _ = engines()
    r = transforms()
    assert r["c2s"].level == r["ct"].level + H.coeffs_to_slots_depth(None) == 1
    assert r["c2s_err"] <= 4 * r["ctrl1"], (r["c2s_err"], r["ctrl1"])
    assert r["c2s_err"] < 1e-6 * max(1.0, np.abs(r["u"]).max())                # and it is the coefficients at all


def test_round_trip_is_the_identity_on_messages():
    H, _ = engines()
    r = transforms()
    assert r["back"].level == r["ct"].level + H.coeffs_to_slots_depth(None) + H.slots_to_coeffs_depth(None, 1) == 2
    assert r["back_err"] <= 4 * (r["ctrl1"] + r["ctrl2"]), (r["back_err"], r["ctrl1"], r["ctrl2"])


def test_a_small_constant_takes_a_level_of_its_own():
    """a divisor 64 times the level's own scale: the matrices keep their size, the constant is a scalar multiplication"""
    w = world()
    H = w["H"]
    r = transforms()
    divisor = 64.0 * float(H.scale) ** 2 * float(H.deviations[0])
    assert H.coeffs_to_slots_depth(divisor) == 2
    out = H.coeffs_to_slots(r["ct"], w["rotks"], w["conjk"], divisor=divisor)
    assert out.level == 2
    err = float(np.abs(H.decrode(out, w["sk"]) - r["u"] / 64).max())
    print(f"\ncoeffs_to_slots with a constant of 1/64 (two levels): max error {err:.3e}")
    assert err <= 4 * r["ctrl1"]                                                # (the control's error at full size bounds the scaled one)


def test_coeffs_to_slots_of_a_raised_ciphertext():
    w = world()
    H = w["H"]
    n, qb = H.num_slots, H.base_prime
    _, up, T = raised(13, w["sk"], w["pk"], w["s"])
    assert H.coeffs_to_slots_depth(qb) == 1
    out = H.coeffs_to_slots(up, w["rotks"], w["conjk"], divisor=qb)
    assert out.level == 1
    got = H.decrode(out, w["sk"])
    exact = np.array([t / qb for t in T], dtype=np.float64)                     # (true division of Python integers: correctly rounded)
    want = exact[:n] + 1j * exact[n:]
    err = float(np.abs(got - want).max())
    print(f"\ncoeffs_to_slots(mod_raise(ct), divisor=q_b): max error {err:.3e}, max |I| {int(np.abs(np.rint(exact)).max())}")
    assert err <= 2.0 ** -6
    frac = np.abs(exact - np.floor(exact) - 0.5)
    skipped = frac <= 2.0 ** -5
    assert not skipped.any()                                                    # none near one half for this message
    assert np.array_equal(np.rint(got.real), np.rint(exact[:n])) and np.array_equal(np.rint(got.imag), np.rint(exact[n:]))
    assert np.abs(np.rint(exact)).max() >= 1                                    # the overflow is there to be found
