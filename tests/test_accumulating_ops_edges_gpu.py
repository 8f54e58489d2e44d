"""The accumulating ops — linear_transform (flat: ks_inner_lt_kernel; baby-step / giant-step: ks_inner_baby_kernel,
lt_diag_products_kernel, ks_inner_giant_kernel) and cc_dot (dot_tensor_kernel, ks_inner2_presum_kernel) — at worst-case words
and at the limits of their C entries, word for word against the checker engine (tests/oracle_backend.OracleBackend, pinned at
these very operands by tests/test_accumulating_ops_edges_cpu.py).

Their own files run them on uniform random words, on parameter sets with 2 to 6 special primes.  Here the ciphertexts, the keys
AND the encoded diagonals sit on the bounds the kernels' range arguments rely on (tests/helpers.py: edge_ciphertext, edge_key,
edge_diagonals, pre_rescale_ciphertext), on the sets that take those arguments furthest: ten digits of one limb (K = 1, the
largest sums of balanced products), 8 special primes on one and two logical devices, both arithmetic classes row by row
(sb41_K2), a digit of 8 integer-class limbs (sb45_K8), 18-bit primes (sb20); at level 0 and at the last level the ops accept.
The baby-step / giant-step entry is also taken to its limit of 63 baby keys (bit 63 of the diagonal products' masks), which no
parameter set reaches by accident.  No tolerance anywhere: every comparison is torch.equal."""
import warnings

import pytest
import torch

from liberate_fhe_amd.fhe import encdec
from liberate_fhe_amd.utils import synth
from tests.helpers import edge_ciphertext, edge_diagonals, edge_key, edge_param_sets, pre_rescale_ciphertext
from tests.test_linear_transform_bsgs_gpu import LT, SETS as BSGS_SHAPES

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore", category=UserWarning)

SETS = edge_param_sets()
# (parameter set, logical devices): two devices take the engine's orchestration with a digit exchange between two shards
CONFIGS = (("sb40_K1", 1), ("sb40_K8", 1), ("sb40_K8", 2), ("sb41_K2", 1), ("sb41_K2", 2), ("sb45_K8", 1), ("sb20", 1))
# the two configurations of the orchestrated path (native op entries off): logN 13, and logN 12 where the key switch runs unfused
ORCHESTRATED = {"sb40_K7": dict(SETS["sb40_K7"]), "sb40_K7_logN12": dict(SETS["sb40_K7"], logN=12)}
# ciphertext pattern, key pattern, diagonal pattern (tests/test_engine_edges_gpu.PAIRS with the diagonals beside the ciphertext)
TRIPLES = (("top", "top", "top"), ("mixed", "top", "mixed"), ("top|0", "random", "top"), ("half", "random", "half"),
           ("random", "random", "random"))
FLAT_STEPS = (0, 1, 2, 3, 5, 8, 13)             # six keys: groups of 4 and 2, plus the step-0 term
# on "top" only: keyless; one key and no step 0; nine keys and no step 0 (groups of 4, 4, 1: later groups re-read the pair)
FLAT_SHAPES = ((0,), (5,), (1, 2, 3, 4, 5, 6, 7, 9, 11))
BSGS_FULL = BSGS_SHAPES[0]                      # 7 baby keys (4 + 2 + 1), 5 giant steps with giant 0 (launches of 4 + 1)
DOT_KS = (1, 2, 5, 9)                           # 9: chunks of 4, 4 and 1
LT_GROUP_MAX = 4                                # keys per launch of the flat and the baby kernel (csrc/ckks_ks.hip: NR)
_ENGINES, _KEYS = {}, {}


def flat_cases():
    """(ciphertext / key / diagonal patterns, steps) of the flat form"""
    return [(t, FLAT_STEPS) for t in TRIPLES] + [(TRIPLES[0], s) for s in FLAT_SHAPES]


def bsgs_cases():
    """(patterns, n1, steps) of the baby-step / giant-step form: one shape under every triple, the others on "top" """
    return [(t,) + tuple(BSGS_FULL) for t in TRIPLES] + [(TRIPLES[0],) + tuple(s) for s in BSGS_SHAPES[1:]]


def dot_cases():
    """(evk pattern, k, slot): slot indexes dot_operands' pairs; the one pair fills all k slots.  Every k with every pair under
    the key of 2q - 1 and under the uniform one."""
    return [(kpat, k, s) for kpat in ("top", "random") for k in DOT_KS for s in range(3)]


def key_steps(num_slots):
    """every step any case above needs a rotation key for"""
    out = {s for _, steps in flat_cases() for s in steps}
    for _, n1, steps in bsgs_cases():
        _, babies, giants = encdec.bsgs_split(steps, num_slots, n1)
        out |= set(babies) | set(giants)
    return sorted(out - {0})


def levels_of(eng):
    """level 0 and the last level at which the engine accepts these ops"""
    return (0, eng.num_levels - 2)


def engines(cfg):
    """(HIP engine, checker engine) of a configuration, built once per process and never freed (see tests/test_cc_dot_gpu.keep).
    cfg = (edge parameter set, logical devices) — the cache of tests/test_engine_edges_gpu.py — or a name of ORCHESTRATED."""
    if isinstance(cfg, tuple):
        from tests.test_engine_edges_gpu import engines as edge_engines
        return edge_engines(*cfg)
    if cfg not in _ENGINES:
        from liberate_fhe_amd.fhe import ckks_engine
        from liberate_fhe_amd.fhe.backend import HipBackend
        from tests.oracle_backend import OracleBackend
        be = HipBackend()
        be.native_ops = False
        H = ckks_engine(devices=["cuda:0"], backend=be, **ORCHESTRATED[cfg])
        assert H._native_level(0) is None
        _ENGINES[cfg] = (H, ckks_engine(devices=["cpu"], backend=OracleBackend(), **ORCHESTRATED[cfg]))
    return _ENGINES[cfg]


def keys_of(cfg, eng, pattern, steps=None):
    """step -> rotation key of edge words for every step of key_steps (or of `steps`: the files that share this cache, e.g.
    tests/test_matrix_ops_edges_gpu.py; a step has the same words under either); the keys of ONE configuration are kept (both
    engines', both patterns'), those of the previous one are dropped."""
    if _KEYS.get("cfg") != cfg:
        _KEYS.clear()
        _KEYS["cfg"] = cfg
    key = (id(eng), pattern) if steps is None else (id(eng), pattern, tuple(sorted(steps)))
    if key not in _KEYS:
        wanted = key_steps(eng.num_slots) if steps is None else key[2]
        _KEYS[key] = {s: edge_key(eng, pattern, 100 + s, origin=f"rotation key:{s}") for s in wanted}
    return _KEYS[key]


def evk_of(cfg, eng, pattern):
    if _KEYS.get("cfg") != cfg:
        _KEYS.clear()
        _KEYS["cfg"] = cfg
    key = (id(eng), "evk", pattern)
    if key not in _KEYS:
        _KEYS[key] = edge_key(eng, pattern, 1)
    return _KEYS[key]


def lt_op(cfg, eng, level, patterns, steps, n1=None):
    """linear_transform (n1: baby-step / giant-step) of one case on `eng`: the operands depend on the case alone"""
    ct = edge_ciphertext(eng, level, patterns[0], 20 + level)
    diags = edge_diagonals(eng, level, steps, patterns[2], 7 + level, n1)
    return eng.linear_transform(ct, diags, keys_of(cfg, eng, patterns[1]))


def dot_operands(eng, level):
    """three pairs of ciphertexts whose rescale IS an edge pattern (pre_rescale_ciphertext, as test_engine_edges_gpu._op_results
    builds them): the square of "top" (the largest products), top x mixed, top|0 x mixed"""
    pa, pb, pc = (pre_rescale_ciphertext(eng, level, p, 30 + level, shift=i) for i, p in enumerate(("top", "mixed", "top|0")))
    return [(pa, pa), (pa, pb), (pc, pb)]


def same_ct(got, want, what):
    """the differing words and the first index, as tests/test_engine_edges_gpu.same reports them"""
    assert got.level == want.level and got.origin == want.origin and len(got.data) == len(want.data), what
    for ci, (gc, wc) in enumerate(zip(got.data, want.data)):
        assert len(gc) == len(wc), what
        for di, (g, w) in enumerate(zip(gc, wc)):
            g, w = g.cpu(), w.cpu()
            assert g.shape == w.shape, f"{what}, component {ci}, device {di}: shape {tuple(g.shape)} != {tuple(w.shape)}"
            if not torch.equal(g, w):
                bad = (g != w).nonzero()
                i = tuple(int(v) for v in bad[0])
                raise AssertionError(f"{what}, component {ci}, device {di}: {len(bad)} of {w.numel()} words differ, "
                                     f"first at {i}: {int(g[i])} != {int(w[i])}")


def native_expected(cfg, eng, level):
    """whether the op's one native call applies at `level`: native op entries on, and every limb of the level on one device
    (two logical devices share the limbs of level 0; at the last levels the few limbs left sit on one of them)"""
    holders = [d for d in eng.ntt.p.destination_arrays[level] if len(d)]
    return isinstance(cfg, tuple) and len(holders) == 1


class native_calls:
    """Counts the calls of a backend's native op entry while the block runs.  Both paths of an op leave the checker's words, so
    only the count shows that the one native call — not a quiet fall-back to the orchestration — is what was compared."""

    def __init__(self, backend, name):
        self.backend, self.name, self.count = backend, name, 0

    def __enter__(self):
        real = getattr(self.backend, self.name)

        def counted(*args, **kw):
            self.count += 1
            return real(*args, **kw)

        setattr(self.backend, self.name, counted)       # (an instance attribute over the class's method)
        return self

    def __exit__(self, *exc):
        delattr(self.backend, self.name)


def check_flat(cfg, last):
    H, C = engines(cfg)
    level = levels_of(H)[last]
    native = native_expected(cfg, H, level)
    assert (H._native_level(level) is not None) == native
    for patterns, steps in flat_cases():
        with native_calls(H.backend, "linear_transform_native") as n:
            got = lt_op(cfg, H, level, patterns, steps)
        assert n.count == int(native), (cfg, level, patterns, steps, n.count)
        want = lt_op(cfg, C, level, patterns, steps)
        assert got.level == level + 1
        same_ct(got, want, f"{cfg} level {level} flat {'/'.join(patterns)} steps {steps}")


def check_bsgs(cfg, last):
    H, C = engines(cfg)
    level = levels_of(H)[last]
    native = native_expected(cfg, H, level)
    assert (H._native_level(level) is not None) == native
    for patterns, n1, steps in bsgs_cases():
        with native_calls(H.backend, "linear_transform_bsgs_native") as n:
            got = lt_op(cfg, H, level, patterns, steps, n1)
        assert n.count == int(native), (cfg, level, patterns, n1, steps, n.count)
        want = lt_op(cfg, C, level, patterns, steps, n1)
        assert got.level == level + 1
        same_ct(got, want, f"{cfg} level {level} bsgs {'/'.join(patterns)} n1 {n1} steps {steps}")


def check_dot(cfg, last):
    H, C = engines(cfg)
    level = levels_of(H)[last]
    native = all(native_expected(cfg, H, lv) for lv in (level, level + 1))      # (lf_cc_dot needs both levels on one device)
    for lv in (level, level + 1):
        assert (H._native_level(lv) is not None) == native_expected(cfg, H, lv)
    ph, pc = dot_operands(H, level), dot_operands(C, level)
    for kpat, k, slot in dot_cases():
        with native_calls(H.backend, "cc_dot_native") as n:
            got = H.cc_dot([ph[slot]] * k, evk_of(cfg, H, kpat))
        assert n.count == int(native), (cfg, level, kpat, k, slot, n.count)
        want = C.cc_dot([pc[slot]] * k, evk_of(cfg, C, kpat))
        assert got.level == level + 1 and not got.ntt_state and not got.include_special
        same_ct(got, want, f"{cfg} level {level} cc_dot evk {kpat} k {k} pair {slot}")


LEVEL_IDS = ["level0", "last_level"]


@pytest.mark.parametrize("last", [0, 1], ids=LEVEL_IDS)
@pytest.mark.parametrize("name,n_dev", CONFIGS)
def test_flat_linear_transform_on_edge_words_equals_the_checker(name, n_dev, last):
    """lf_linear_transform (one device) / the orchestration with a digit exchange (two): seven diagonals under the five
    pattern triples; on "top" also the keyless launch, one key without step 0, nine keys without step 0."""
    check_flat((name, n_dev), last)


@pytest.mark.parametrize("last", [0, 1], ids=LEVEL_IDS)
@pytest.mark.parametrize("name,n_dev", CONFIGS)
def test_bsgs_linear_transform_on_edge_words_equals_the_checker(name, n_dev, last):
    """lf_linear_transform_bsgs: 14 diagonals over n1 = 8 under the five pattern triples; on "top" also baby 0 and giant 0
    absent, n1 = 1 (no baby key), one giant step g = 0 (no giant key)."""
    check_bsgs((name, n_dev), last)


@pytest.mark.parametrize("last", [0, 1], ids=LEVEL_IDS)
@pytest.mark.parametrize("name,n_dev", CONFIGS)
def test_cc_dot_on_edge_words_equals_the_checker(name, n_dev, last):
    """lf_cc_dot: k = 1, 2, 5 and 9 copies of each of three pairs (9 copies of the square of "top": the largest accumulator of
    dot_tensor_kernel and the largest T0, T1 the pre-summed fold meets) under a key of 2q - 1 and a uniform one; the operands'
    dropped limb holds the rescale rounder's five values."""
    check_dot((name, n_dev), last)


@pytest.mark.parametrize("op", ["flat", "bsgs", "cc_dot"])
@pytest.mark.parametrize("last", [0, 1], ids=LEVEL_IDS)
@pytest.mark.parametrize("cfg", sorted(ORCHESTRATED))
def test_the_same_cases_through_the_orchestrated_path(cfg, last, op):
    """Native op entries off (tests/test_engine_edges_gpu.test_whole_ops_through_the_orchestrated_path): the engine's
    step-by-step orchestration of the same operations at logN 13, and at logN 12 where the key switch runs unfused."""
    {"flat": check_flat, "bsgs": check_bsgs, "cc_dot": check_dot}[op](cfg, last)


# ---- lf_linear_transform_bsgs at the limit of its ABI: LF_BSGS_MAX_BABY_KEYS = 63 ------------------------------------------------
LIMIT_SHAPES = {62: (64, tuple(range(63)) + (65,)),       # 62 baby keys: slot 62 the last; giant steps 0 and 64
                63: (64, tuple(range(64)) + (65,)),       # 63 baby keys: slot 63 = bit 63 of the masks, the 64-pair workspace
                64: (128, tuple(range(65)) + (129,))}     # 64 keyed baby steps: past the entry's limit, the engine must fall back


def _limit_engines():
    if "limit" not in _ENGINES:
        from liberate_fhe_amd.fhe import ckks_engine
        from tests.oracle_backend import OracleBackend
        _ENGINES["limit"] = (ckks_engine(devices=["cuda:0"], **LT), ckks_engine(devices=["cpu"], backend=OracleBackend(), **LT))
    return _ENGINES["limit"]


def _limit_keys(eng):
    """uniform keys (utils.synth) for the steps of every LIMIT_SHAPES entry; kept with the engine"""
    key = ("limit keys", id(eng))
    if key not in _ENGINES:
        steps = set()
        for n1, shape in LIMIT_SHAPES.values():
            _, babies, giants = encdec.bsgs_split(shape, eng.num_slots, n1)
            steps |= set(babies) | set(giants)
        _ENGINES[key] = {s: synth.key_switch_key(eng, 40 + s, origin=f"rotation key:{s}") for s in sorted(steps - {0})}
    return _ENGINES[key]


def _limit_op(eng, nb, level=0):
    n1, steps = LIMIT_SHAPES[nb]
    _, babies, giants = encdec.bsgs_split(steps, eng.num_slots, n1)
    assert len([b for b in babies if b]) == nb and giants == [0, n1]
    ct = synth.ciphertext(eng, 90 + nb, level)
    return eng.linear_transform(ct, edge_diagonals(eng, level, steps, "random", 5, n1), _limit_keys(eng))


@pytest.mark.parametrize("nb", sorted(LIMIT_SHAPES))
def test_bsgs_at_the_limit_of_the_entry(nb, monkeypatch):
    """62 and 63 baby keys run through lf_linear_transform_bsgs (groups of 4 .. 4, 2 (, 1) keys; 63 or 64 pairs in the workspace;
    at 63 the last slot is bit 63 of lt_diag_products_kernel's masks), 64 through the engine's orchestration; which path ran is
    counted at backend.linear_transform_bsgs_native.  Every result equals the orchestrated path's on the GPU (native op entries
    off), and at 63 keys the checker engine's.  Uniform words: a slot mask that loses or moves a bit drops or swaps whole
    diagonals, which any words show."""
    H, C = _limit_engines()
    be = H.backend
    calls = []
    real = be.linear_transform_bsgs_native
    monkeypatch.setattr(be, "linear_transform_bsgs_native", lambda *a, **kw: (calls.append(len(a[4])), real(*a, **kw))[1])
    assert H._native_level(0) is not None
    got = _limit_op(H, nb)
    assert calls == ([nb] if nb <= 63 else []), (nb, calls)
    monkeypatch.setattr(be, "native_ops", False)
    assert H._native_level(0) is None
    same_ct(got, _limit_op(H, nb), f"LT level 0 bsgs {nb} baby keys, native call against the orchestrated path")
    assert len(calls) <= 1
    if nb == 63:
        same_ct(got, _limit_op(C, nb), f"LT level 0 bsgs {nb} baby keys against the checker")
