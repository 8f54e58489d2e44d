"""The fp64-class inner sums AT the bound their range arguments name (csrc/ckks_ks.hip: the table above lf_fp64_digits_ok and the
comments beside the kernels: "nparts balanced products of at most q / 2 each, plus a few words below 2q"), word for word against
the checker engine.

Extended digits are NTT outputs, so on any ordinary operand — the "top" patterns included — the products are pseudo-random and
a sum of n of them sits near sqrt(n / 12) q, nowhere near n q / 2.  Here every product IS +-(q - 1) / 2 with one sign along a
whole sum (tests/helpers.py: constant_ciphertext, extended_constants, extreme_key; tests/test_worst_case_sums_cpu.py proves it
from the operands, in Python integers and in the kernels' own fp64 quotient), on the deep parameter set sb40_K1_d32: 32 digits of
one limb at level 0 (31 at level 1, an odd count), 33 rows, 31 of them fp64-class.  ks_inner_rsum_kernel with 4 keys then holds
about 69 q and ks_inner_rsumb_kernel with 8 keys about 137 q before their one reduction — beyond dp_reduce's 64 q, the
dp_reduce_bal-then-dp_reduce path — and the kernels that reduce with dp_reduce alone hold 16 to 17 q.  The context's prime list
runs out between 61 and 80 digits, so LF_FP64_MAX_DIGITS = 119 itself cannot be reached through an engine; that is not a defect.

Which path ran is counted at the backend's native entry: exactly one call each.  In the batch ops member 0 (and, in a second run,
the last member) is the extreme ciphertext; the others are other constants, one seed each, which see ordinary products under
the keys built for member 0.  In the baby-step / giant-step transform only the baby phase sits at the bound: the giant-step
digits come from a mod-down and cannot be steered, so they are along for the ride.

Out of scope: the relinearisation sums of cc_dot / cc_matmul (their digits come from a tensor product behind a rescale) and the
giant-step kernels (their digits come from a mod-down).  dp_reduce's 64 q is a conservative figure: a kernel that merely skipped
dp_reduce_bal might still pass at 70 q.  What these tests catch is a reduction that is wrong for large or negative sums, and a
start term or gathered word added twice or dropped.  No tolerance anywhere: every comparison is torch.equal."""
import warnings

import pytest

from tests.helpers import constant_ciphertext, edge_diagonals, extended_constants, extreme_key
from tests.test_accumulating_ops_edges_gpu import native_calls, same_ct

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore", category=UserWarning)

DEEP = "sb40_K1_d32"
LEVELS = (0, 1)
KEY_STEPS = tuple(range(1, 10))              # nine: one more than a launch of ks_inner_rsumb_kernel takes
HOIST_STEPS = (1, 2, 3, 5)
FLAT_STEPS = (0, 1, 2, 3, 5)
BSGS = (4, tuple(range(8)))                  # n1, steps: baby keys 1, 2, 3 and the giant key 4
MATMUL_LAYOUT = [[(0, 1, 2, 3)] * 2] * 2
# (keys, self term) of rotate_sum: the second group of five keys re-reads the pair the first left
RSUM_CASES = [(n, w) for n in (1, 4, 5) for w in (True, False)]
_CACHE = {}


def extreme_keys(eng, constants, flip=False):
    """step -> the ONE extreme key pack under the origin of each step of KEY_STEPS (a rotation leaves a constant polynomial
    unchanged, so the pack built from the constants serves every step; _replace shares the tensors, 138 MB, and the engine's
    own copy of them in its key format hangs on the first tensor)"""
    base = extreme_key(eng, constants, origin=f"rotation key:{KEY_STEPS[0]}", flip=flip)
    return {s: base._replace(origin=f"rotation key:{s}") for s in KEY_STEPS}


def setup():
    """(HIP engine, checker engine, their extreme keys, their flipped keys): the constants come from the checker's steps"""
    if "setup" not in _CACHE:
        from tests.test_engine_edges_gpu import engines
        H, C = engines(DEEP, 1)
        constants = extended_constants(C, constant_ciphertext(C, 0, 0))
        _CACHE["setup"] = (H, C, {id(e): extreme_keys(e, constants) for e in (H, C)},
                           {id(e): extreme_keys(e, constants, flip=True) for e in (H, C)})
    return _CACHE["setup"]


def batch_of(eng, level, last=False):
    """four constant ciphertexts, one seed each; the extreme one (seed 0, whose constants the keys were built from) first or last"""
    seeds = (1, 2, 3, 0) if last else (0, 1, 2, 3)
    return [constant_ciphertext(eng, level, s) for s in seeds]


def both(op, entry, what, calls=1):
    """op(engine, keys) on the HIP engine, counted at backend.<entry>, against the checker's"""
    H, C, keys, _ = setup()
    assert H._native_level(0) is not None and H._native_level(1) is not None
    with native_calls(H.backend, entry) as n:
        got = op(H, keys[id(H)])
    assert n.count == calls, (what, n.count)
    want = op(C, keys[id(C)])
    if not isinstance(got, list):
        got, want = [got], [want]
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        same_ct(g, w, f"{DEEP} {what} result {i}")
    return got


@pytest.mark.parametrize("level", LEVELS)
def test_rotate_and_rotate_hoisted(level):
    """lf_switch_key (the fused inner product) and lf_rotate_hoisted with 4 steps (ks_inner_hoist_kernel): nparts / 2 q each"""
    both(lambda e, k: e.rotate_single(constant_ciphertext(e, level, 0), k[1]), "switch_key_native", f"level {level} rotate_single")
    both(lambda e, k: e.rotate_hoisted(constant_ciphertext(e, level, 0), [k[s] for s in HOIST_STEPS]), "rotate_hoisted_native",
         f"level {level} rotate_hoisted")


@pytest.mark.parametrize("level", LEVELS)
def test_rotate_sum(level):
    """lf_rotate_sum (ks_inner_rsum_kernel): 1, 4 and 5 keys with and without the self term — with 4 keys and the self term the
    accumulator of component 0 holds more than 64 q where the products are positive and about -59 q where they are negative;
    and once under the flipped keys, where the signs of the two components trade places."""
    for nk, with_self in RSUM_CASES:
        both(lambda e, k: e.rotate_sum(constant_ciphertext(e, level, 0), [k[s] for s in KEY_STEPS[:nk]], include_self=with_self),
             "rotate_sum_native", f"level {level} rotate_sum {nk} keys self {with_self}")
    H, C, _, flipped = setup()
    with native_calls(H.backend, "rotate_sum_native") as n:
        got = H.rotate_sum(constant_ciphertext(H, level, 0), [flipped[id(H)][s] for s in KEY_STEPS[:4]], include_self=True)
    assert n.count == 1
    same_ct(got, C.rotate_sum(constant_ciphertext(C, level, 0), [flipped[id(C)][s] for s in KEY_STEPS[:4]], include_self=True),
            f"{DEEP} level {level} rotate_sum 4 flipped keys")


@pytest.mark.parametrize("level", LEVELS)
def test_rotate_sum_batch(level):
    """lf_rotate_sum_batch (ks_inner_rsumb_kernel) of 4 ciphertexts with 8 keys (one launch: more than 127 q at level 0) and 9
    (a second launch re-reads the pairs); the extreme ciphertext first, then last.  The checker's side is its loop of
    rotate_sum, which is what the batch is defined as."""
    from tests.test_rotate_sum_batch_gpu import keys_per_launch
    assert keys_per_launch() == 8
    for nk in (8, 9):
        for last in (False, True):
            def op(e, k):
                cts = batch_of(e, level, last)
                ks = [k[s] for s in KEY_STEPS[:nk]]
                return e.rotate_sum_batch(cts, ks) if hasattr(e.backend, "rotate_sum_batch_native") else [e.rotate_sum(ct, ks) for ct in cts]
            got = both(op, "rotate_sum_batch_native", f"level {level} rotate_sum_batch {nk} keys extreme member {'last' if last else 'first'}")
            # the extreme member is where it was put: it alone equals rotate_sum of the extreme ciphertext
            H, _, keys, _ = setup()
            alone = H.rotate_sum(constant_ciphertext(H, level, 0), [keys[id(H)][s] for s in KEY_STEPS[:nk]])
            same_ct(got[3 if last else 0], alone, f"{DEEP} level {level} rotate_sum_batch {nk} keys: the extreme member")


@pytest.mark.parametrize("level", LEVELS)
def test_flat_linear_transform_and_its_batch(level):
    """lf_linear_transform (ks_inner_lt_kernel) and lf_linear_transform_batch of 4 ciphertexts (ks_inner_ltb_kernel) on steps
    (0, 1, 2, 3, 5) under diagonals at 2q - 1: every per-key sum at nparts / 2 q plus the gathered word before its
    dp_reduce_bal."""
    diags = lambda e: edge_diagonals(e, level, FLAT_STEPS, "top", 7 + level)
    both(lambda e, k: e.linear_transform(constant_ciphertext(e, level, 0), diags(e), k), "linear_transform_native",
         f"level {level} linear_transform")
    for last in (False, True):
        def op(e, k):
            cts = batch_of(e, level, last)
            if hasattr(e.backend, "linear_transform_batch_native"):
                return e.linear_transform_batch(cts, diags(e), k)
            return [e.linear_transform(ct, diags(e), k) for ct in cts]
        both(op, "linear_transform_batch_native", f"level {level} linear_transform_batch extreme member {'last' if last else 'first'}")


@pytest.mark.parametrize("level", LEVELS)
def test_bsgs_linear_transform_and_lt_matmul(level):
    """lf_linear_transform_bsgs with n1 = 4 over steps 0 .. 7 (ks_inner_baby_kernel at the bound; the giant-step digits come from
    a mod-down and are along for the ride) and lf_lt_matmul 2 x 2 with steps (0, 1, 2, 3) per block (the baby sums of two
    inputs, the extreme ciphertext and another constant)."""
    n1, steps = BSGS
    both(lambda e, k: e.linear_transform(constant_ciphertext(e, level, 0), edge_diagonals(e, level, steps, "top", 9 + level, n1), k),
         "linear_transform_bsgs_native", f"level {level} bsgs linear_transform")

    def op(e, k):
        W = [[edge_diagonals(e, level, st, "top", 11 + level + 2 * o + i) for i, st in enumerate(row)] for o, row in enumerate(MATMUL_LAYOUT)]
        return e.lt_matmul(W, [constant_ciphertext(e, level, s) for s in (0, 1)], k)
    both(op, "lt_matmul_native", f"level {level} lt_matmul 2 x 2")
