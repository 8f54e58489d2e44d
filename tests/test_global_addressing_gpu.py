"""Every access pattern behind uniform_ptr() / uniform_at() (ckks_ntt_core.h: SGPR row base + 32-bit lane offset, global
instead of FLAT instructions) reached once on small shapes.  The change is addressing only, so the yardstick is word-for-word
equality: lf_ntt_ws / lf_intt_ws against the in-place lf_ntt / lf_intt and against the C oracle, at logN 13 (one tile per block)
and logN 16 (ntt_fwd_cols_ws<5>, ntt_pass16_fwd_ws), with 2 fp64-class limbs + 1 integer-class limb and a batch of 3.  Operands
are lazy words, plus one word >= 2q and one negative word per limb: the column waves that meet them write the third plane and
raise their flag bytes, and the tiles behind reload the slow way — those accesses go through the same helpers.  The 8-tiles-
per-block kernel (32 768 tiles on) is tests/test_fullsize_gpu.py's."""
import numpy as np
import pytest

from tests.helpers import SMALL_PRIME_LIMIT, Limbs, pick_primes
from tests.test_class_edges_gpu import Setup

pytestmark = pytest.mark.gpu

BATCH = 3
_CASES = {}


def case(logN):
    """(limbs, setup, operands [3, rows, N], oracle forward, oracle forward with entry, oracle inverse by tail) — computed once."""
    if logN not in _CASES:
        lim = Limbs(logN, pick_primes(logN, 2, 1))
        assert [q < SMALL_PRIME_LIMIT for q in lim.q] == [True, True, False]
        s = Setup(lim)
        x = np.stack([lim.uniform(500 + 10 * logN + b, lazy=True) for b in range(BATCH)])
        for b in range(BATCH):
            for r, q in enumerate(lim.q):
                x[b, r, 64 * (r + 2 * b) + 1] = 2 * q + b                       # >= 2q: first columns, low tiles
                x[b, r, lim.N - 1 - 64 * (r + b) - 2048 * b] = -1 - b           # negative: last columns, high tiles
        fwd = np.stack([s.o_ntt(p) for p in x])
        ent = np.stack([s.o_ntt(p, enter=True) for p in x])
        inv = {tail: np.stack([s.o_intt(p, tail) for p in x]) for tail in (0, 2)}
        for a in (x, fwd, ent, *inv.values()):
            a.setflags(write=False)
        _CASES[logN] = (lim, s, x, fwd, ent, inv)
    return _CASES[logN]


@pytest.mark.parametrize("logN", [13, 16])
def test_forward_through_the_workspace_equals_in_place_and_oracle(logN):
    lim, s, x, fwd, ent, _ = case(logN)
    for name, Rs, want in (("ntt", None, fwd), ("enter_ntt", s.Rs, ent)):
        through, in_place = s.ntt(x, Rs=Rs, ws=True), s.ntt(x, Rs=Rs)
        assert (through == in_place).all(), f"{name}: workspace against in place, {int((through != in_place).sum())} words differ"
        assert (through == want).all(), f"{name}: workspace against the oracle, {int((through != want).sum())} words differ"


@pytest.mark.parametrize("logN", [13, 16])
def test_inverse_through_the_workspace_equals_in_place_and_oracle(logN):
    lim, s, x, _, _, inv = case(logN)
    for tail, want in inv.items():
        through, in_place = s.intt(x, tail, ws=True), s.intt(x, tail)
        assert (through == in_place).all(), f"tail {tail}: workspace against in place, {int((through != in_place).sum())} words differ"
        assert (through == want).all(), f"tail {tail}: workspace against the oracle, {int((through != want).sum())} words differ"
