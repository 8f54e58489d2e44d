"""Where the native op entries write: every scratch tensor and every output of every op the engine runs as one native call sits
between guards (tests/helpers.Fence) and starts from a hostile fill — every bit set, 2^63 - 1, uniform 64-bit words, never zero.
The edge-word files take the VALUES to their bounds; this one does the same for the ADDRESSES.  The caching allocator rounds
requests up and carves them out of large blocks, so a kernel that writes one row, one plane or one token's stack past its buffer
lands in a neighbour without a fault, and an entry that adds to a sum it should have written fresh — or reads a scratch word an
earlier launch was meant to write — finds harmless zeros in a fresh process.  Neither shows in a comparison of results alone.

One test per op family, parameter set and level.  It runs the family's case list on the UNFENCED engine of the same parameters
(tests/test_engine_edges_gpu.engines, pinned to the checker on these sets by the edge files), then once per fill on the fenced
engine, and asserts after every case: (i) the guards of every scratch buffer and every output are intact; (ii), (iii) the words are
torch.equal to the unfenced engine's, hence equal across the three fills; no output still holds its fill; the operands —
ciphertext components, key parts, diagonals, plaintexts — are untouched (no op modifies an operand by design: DESIGN.md names
none); the set of native entries the fence saw is the family's (a quiet fall-back to the orchestration fails).  (iv) On sb41_K2
the words are also torch.equal to the checker engine's.  Operands are ordinary uniform lazy words: values are not the point.

Parameter sets, all at logN 13 (the smallest ring of the native entries) on one device: sb40_K1 (ten digits of one limb), sb45_K8
(a digit of 8 limbs, K = 8: the other mod-down form), sb41_K2 (both arithmetic classes row by row: planes beside raw words), LT
(5 scales, K = 2).  Levels: 0 and the last one each op accepts (one row left: the degenerate strides).

Refusals, on sb41_K2 through the same wrappers: each of the sixteen entries with a workspace refuses one word fewer than its own
*_ws_words says, and each entry whose header promises it refuses a misaligned one (LF_ERR_ARG, every fenced body still at its fill:
nothing was launched).  The knob walk (LF_TUNE_DIGIT_PLANES x LF_TUNE_MORE_PLANES) runs in a child process.

The limb-sharded halves (lf_*_pre / lf_*_post, lf_ks_plan_fwd) and their graph-replayed segments run under the same fence in the
ranks of tests/test_sharded_edges_gpu.py (Fence wraps HALF_ENTRIES too: fenced outputs for the post halves, the guard check of all
scratch behind the others; sb41_K2 and sb40_K1, two ranks and a solo rank, the three fills, refill() before every case, between
a capture and its replays included).  Not covered: the in-process engine over two logical devices under the fence, and anything that
crosses xGMI; the NTT workspace and the step kernels have fences of their own."""
import os
import warnings

import numpy as np
import pytest
import torch

from liberate_fhe_amd.fhe.backend import HipBackend
from liberate_fhe_amd.utils import synth
from tests import test_accumulating_ops_edges_gpu as A
from tests.helpers import FENCE_FILLS, Fence, Untouched, edge_param_sets
from tests.test_cc_dot_gpu import SLOTS
from tests.test_lt_matmul_bsgs_cpu import LAYOUT as BSGS_LAYOUT, N1
from tests.test_lt_matmul_gpu import LAYOUT as FLAT_LAYOUT
from tests.test_pc_matmul_gpu import layer_of
from tests.test_product_ops_edges_gpu import CI, DOT_BATCH, PC_DOT_KS, PC_MATMUL_HOLES, PC_MATMUL_SHAPES, WSUM_G, WSUM_K
from tests.test_rotate_sum_batch_gpu import STEPS as RSUM_STEPS, key_sets

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore", category=UserWarning)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SET_NAMES = ("sb40_K1", "sb45_K8", "sb41_K2", "LT")
CHECKED = "sb41_K2"                                 # (iv): the set whose words are also compared with the checker engine
LEVEL_IDS = A.LEVEL_IDS
B = 7                                               # every batched op: groups of 4 and 2 and a straggler
LIMIT_N1, LIMIT_STEPS = A.LIMIT_SHAPES[63]          # 63 baby keys: the largest workspace any entry accepts
LF_ERR_ARG = 10001
_FENCED, _OPS = {}, {}


def params_of(name):
    return dict(A.LT) if name == "LT" else dict(edge_param_sets()[name])


def plain_engines(name):
    """(unfenced HIP engine, checker engine): the caches of the edge files"""
    return A._limit_engines() if name == "LT" else A.engines((name, 1))


def fenced_engine(name):
    """(engine, fence) of a parameter set, built once per process and never freed (see tests/test_cc_dot_gpu.keep)"""
    if name not in _FENCED:
        from liberate_fhe_amd.fhe import ckks_engine
        eng = ckks_engine(devices=["cuda:0"], **params_of(name))
        _FENCED[name] = (eng, Fence(eng, FENCE_FILLS["ones"]))
    return _FENCED[name]


def mirror(x, device):
    """x with every tensor on `device` (the checker engine's copy of an operand: same words, same flags, same hash)"""
    if isinstance(x, torch.Tensor):
        return x.to(device)
    if hasattr(x, "origin") and hasattr(x, "_replace"):
        return x._replace(data=mirror(x.data, device))
    if isinstance(x, dict):
        return {k: mirror(v, device) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return type(x)(mirror(v, device) for v in x)
    return x


class Ops:
    """The operands of a parameter set, made once (by the unfenced engine: the fenced one takes the very same objects) and kept
    with a clone of every tensor (`keep`: inputs untouched).  Ops(eng, src): the checker's copies of src's objects."""

    def __init__(self, eng, src=None):
        self.eng, self.src, self.made, self.keep = eng, src, {}, Untouched()

    def get(self, key, make):
        if key not in self.made:
            self.made[key] = make(self.eng) if self.src is None else mirror(self.src.get(key, make), "cpu")
            self.keep.add(str(key), self.made[key])
        return self.made[key]

    def ct(self, seed, level):
        return self.get(("ct", seed, level), lambda e: synth.ciphertext(e, seed, level))

    def cts(self, n, level, seed=50):
        return [self.ct(seed + i, level) for i in range(n)]

    def evk(self):
        return self.get(("evk",), lambda e: synth.key_switch_key(e, 77))

    def key(self, s):
        return self.get(("rotk", s), lambda e: synth.key_switch_key(e, 100 + s, origin=f"rotation key:{s}"))

    def keys(self, steps):
        return {s: self.key(s) for s in sorted(set(steps)) if s}

    def diags(self, seed, level, steps, n1=None):
        make = (lambda e: synth.diagonals(e, seed, level, steps)) if n1 is None else \
            (lambda e: synth.diagonals_bsgs(e, seed, level, steps, n1))
        return self.get(("diags", seed, level, tuple(steps), n1), make)

    def pt(self, seed, level, kind="mult"):
        def make(e):
            m = np.random.default_rng(seed).uniform(-1, 1, e.num_slots)
            return e.encode_plain(m, level, kind)
        return self.get(("pt", seed, level, kind), make)


def ops_of(name):
    if name not in _OPS:
        H, C = plain_engines(name)
        g = Ops(H)
        _OPS[name] = (g, Ops(C, g))
    return _OPS[name]


def flat_words(res):
    """every tensor of a result (a ciphertext, or nested lists of them), in order"""
    if hasattr(res, "origin"):
        return [t for comp in res.data for t in comp]
    return [t for r in res for t in flat_words(r)]


def assert_same(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        g = g.to(w.device)
        assert g.shape == w.shape, (what, i, tuple(g.shape), tuple(w.shape))
        if not torch.equal(g, w):
            bad = (g != w).nonzero()
            raise AssertionError(f"{what}, tensor {i}: {len(bad)} of {w.numel()} words differ, first at {tuple(int(v) for v in bad[0])}: "
                                 f"{int(g[tuple(bad[0])])} != {int(w[tuple(bad[0])])}")


# ---- the case lists: (label, f(engine, ops) -> result, the native entries the case reaches) ---------------------------------
def lv_rescaling(eng, last):
    """level 0 / the last level of an op that rescales (or multiplies into the next level)"""
    return eng.num_levels - 2 if last else 0


def lv_staying(eng, last):
    """level 0 / the last level of an op whose result stays at the operand's level: one row left"""
    return eng.num_levels - 1 if last else 0


def basic_cases(eng, last, name):
    lm, lr = lv_rescaling(eng, last), lv_staying(eng, last)
    return [("cc_mult", lambda e, o: e.cc_mult(o.ct(50, lm), o.ct(51, lm), o.evk()), {"cc_mult_evk"}),
            ("rotate_single", lambda e, o: e.rotate_single(o.ct(50, lr), o.key(1)), {"switch_key_native"}),
            ("cc_mult_batch", lambda e, o: e.cc_mult_batch([(o.ct(50 + i, lm), o.ct(51 + i, lm)) for i in range(B)], o.evk()),
             {"cc_mult_evk_batch_native", "cc_mult_evk"}),
            ("rotate_single_batch", lambda e, o: e.rotate_single_batch(o.cts(B, lr), o.key(5)),
             {"switch_key_batch_native", "switch_key_native"})]


def flat_cases(eng, last, name):
    lv = lv_rescaling(eng, last)
    out = [(f"linear_transform {steps}", lambda e, o, steps=steps: e.linear_transform(o.ct(50, lv), o.diags(7, lv, steps), o.keys(steps)),
            {"linear_transform_native"}) for steps in (A.FLAT_STEPS,) + A.FLAT_SHAPES]
    return out + [("linear_transform_batch", lambda e, o: e.linear_transform_batch(o.cts(B, lv), o.diags(7, lv, A.FLAT_STEPS), o.keys(A.FLAT_STEPS)),
                   {"linear_transform_batch_native", "linear_transform_native"})]


def bsgs_keys(o, n1, steps):
    from liberate_fhe_amd.fhe import encdec
    _, babies, giants = encdec.bsgs_split(steps, o.eng.num_slots, n1)
    return o.keys(list(babies) + list(giants))


def bsgs_cases(eng, last, name):
    lv = lv_rescaling(eng, last)
    n1, steps = A.BSGS_FULL
    out = [("bsgs", lambda e, o: e.linear_transform(o.ct(50, lv), o.diags(9, lv, steps, n1), bsgs_keys(o, n1, steps)),
            {"linear_transform_bsgs_native"}),
           ("bsgs batch", lambda e, o: e.linear_transform_batch(o.cts(B, lv), o.diags(9, lv, steps, n1), bsgs_keys(o, n1, steps)),
            {"linear_transform_bsgs_batch_native", "linear_transform_bsgs_native"})]
    if name == "LT" and not last:     # (63 keys are generated for one set: the workspace grows with nb, not with the set)
        out.append(("bsgs 63 baby keys", lambda e, o: e.linear_transform(o.ct(50, lv), o.diags(11, lv, LIMIT_STEPS, LIMIT_N1),
                                                                        bsgs_keys(o, LIMIT_N1, LIMIT_STEPS)),
                    {"linear_transform_bsgs_native"}))
    return out


def dot_cases(eng, last, name):
    lv = lv_rescaling(eng, last)
    pairs = lambda o, k, first=0: [(o.ct(50 + SLOTS[(first + i) % 9][0], lv), o.ct(50 + SLOTS[(first + i) % 9][1], lv)) for i in range(k)]
    out = [(f"cc_dot {k}", lambda e, o, k=k: e.cc_dot(pairs(o, k), o.evk()), {"cc_dot_native"}) for k in A.DOT_KS]
    assert len(DOT_BATCH) == B
    return out + [("cc_dot_batch", lambda e, o: e.cc_dot_batch([pairs(o, n, j) for j, n in enumerate(DOT_BATCH)], o.evk()),
                   {"cc_dot_batch_native", "cc_dot_native"})]


def matmul_cases(eng, last, name):
    lv = lv_rescaling(eng, last)

    def small(e, o):
        a, b, c = o.cts(3, lv)
        return e.cc_matmul([[a, b, c], [b, None, a]], [[a, b], [b, c], [c, a]], o.evk())

    def square(e, o):
        x = o.cts(3, lv)
        return e.cc_matmul([[x[(i + t) % 3] for t in range(3)] for i in range(3)], [[x[(2 * t + j) % 3] for j in range(3)] for t in range(3)], o.evk())
    return [("cc_matmul 2 x 3 x 2", small, {"cc_matmul_native"}), ("cc_matmul 3 x 3 x 3", square, {"cc_matmul_native"})]


def pc_pool(o, lv):
    return [o.pt(40 + i, lv) for i in range(3)], o.cts(3, lv), [o.pt(60 + i, lv + 1, "add") for i in range(2)]


def pc_cases(eng, last, name):
    lv = lv_rescaling(eng, last)
    out = []
    for k in PC_DOT_KS:
        for bias in (False, True):
            out.append((f"pc_dot {k} bias {bias}",
                        lambda e, o, k=k, bias=bias: e.pc_dot([(pc_pool(o, lv)[0][i % 3], pc_pool(o, lv)[1][(i + 1) % 3]) for i in range(k)],
                                                              pc_pool(o, lv)[2][0] if bias else None), {"pc_dot_native"}))
    shapes = tuple(PC_MATMUL_SHAPES) + (tuple(PC_MATMUL_HOLES), (1, HipBackend.pc_matmul_max_outputs + 1))
    assert shapes[:2] == ((CI, 4), (CI + 1, 3))
    for k_in, k_out in shapes:
        out.append((f"pc_matmul {k_in} x {k_out}", lambda e, o, k_in=k_in, k_out=k_out: e.pc_matmul(*layer_of(pc_pool(o, lv), k_in, k_out)),
                    {"pc_matmul_native"}))

    def batch(e, o, nt, k_in, k_out):
        W, cts, bias = layer_of(pc_pool(o, lv), k_in, k_out)
        return e.pc_matmul_batch(W, [[cts[(i + t) % len(cts)] for i in range(k_in)] for t in range(nt)], bias)
    out.append(("pc_matmul_batch 3 tokens", lambda e, o: batch(e, o, 3, *PC_MATMUL_SHAPES[1]), {"pc_matmul_batch_native", "pc_matmul_native"}))
    out.append((f"pc_matmul_batch {B} tokens", lambda e, o: batch(e, o, B, 2, 2), {"pc_matmul_batch_native", "pc_matmul_native"}))
    return out


def wsum_cases(eng, last, name):
    lv = lv_rescaling(eng, last)
    if max(eng.ctx.q) >= (1 << 60):         # the engine's own condition for lf_weighted_sums: nothing to fence on such a set
        return []
    rng = np.random.default_rng(3)
    ints = [[int(v) for v in row] for row in rng.integers(-5, 6, size=(WSUM_G, WSUM_K))]
    consts = [int(v) for v in rng.integers(-5, 6, size=WSUM_G)]
    return [("weighted_sums 16 terms 5 outputs",
             lambda e, o: e._weighted_sums_int([o.ct(50 + t % 3, lv) for t in range(WSUM_K)], ints, consts), {"weighted_sums_native"})]


def hoisted_cases(eng, last, name):
    lv = lv_staying(eng, last)
    return [(f"rotate_hoisted {n} keys", lambda e, o, n=n: e.rotate_hoisted(o.ct(50, lv), [o.key(s) for s in range(1, n + 1)]),
             {"rotate_hoisted_native"}) for n in (1, 4, 9)]


def rsum_cases(eng, last, name):
    lv = lv_staying(eng, last)
    out = [(f"rotate_sum {steps} self {with_self}",
            lambda e, o, steps=steps, with_self=with_self: e.rotate_sum(o.ct(50, lv), [o.key(s) for s in steps], include_self=with_self),
            {"rotate_sum_native"}) for steps, with_self in key_sets()]
    inner = (1, 2, 3, 4, 8, 12)
    out.append(("inner_sum 16 = 4 x 4", lambda e, o: e.inner_sum(o.ct(50, lv), 16, o.keys(inner), radix=4), {"rotate_sum_native"}))
    both = {"rotate_sum_batch_native", "rotate_sum_native"}
    out.append(("rotate_sum_batch", lambda e, o: e.rotate_sum_batch(o.cts(B, lv), [o.key(s) for s in RSUM_STEPS]), both))
    out.append(("inner_sum_batch", lambda e, o: e.inner_sum_batch(o.cts(B, lv), 16, o.keys(inner), radix=4), both))
    return out


def layer(o, lv, layout, n1=None):
    """(W, cts, keys) of a layout: one diagonals object per block, one ciphertext per column (tests/test_lt_matmul_gpu.layer)"""
    W = [[None if st is None else o.diags(7 + 8 * r + i, lv, st, n1) for i, st in enumerate(row)] for r, row in enumerate(layout)]
    steps = {s for row in layout for st in row if st is not None for s in st}
    if n1 is not None:
        steps = {s % n1 for s in steps} | {s - s % n1 for s in steps}
    return W, o.cts(len(layout[0]), lv), o.keys(steps)


def ltmm_cases(eng, last, name):
    lv = lv_rescaling(eng, last)
    many = HipBackend.lt_matmul_max_outputs + 1

    def flat(e, o):
        W, cts, keys = layer(o, lv, FLAT_LAYOUT)
        return e.lt_matmul(W, cts, keys)

    def wide(e, o):     # one diagonal per output, one more output than a call takes
        d = o.diags(5, lv, (1,))
        return e.lt_matmul([[d]] * many, [o.ct(50, lv)], o.keys((1,)))

    def batch(e, o):
        W, _, keys = layer(o, lv, FLAT_LAYOUT)
        k_in = len(FLAT_LAYOUT[0])
        return e.lt_matmul_batch(W, [[o.ct(50 + (t + i) % 5, lv) for i in range(k_in)] for t in range(B)], keys)

    def bsgs(e, o):
        W, cts, keys = layer(o, lv, BSGS_LAYOUT, N1)
        return e.lt_matmul_bsgs(W, cts, keys)
    return [("lt_matmul 3 x 5", flat, {"lt_matmul_native"}), (f"lt_matmul 1 x {many}", wide, {"lt_matmul_native"}),
            ("lt_matmul_batch", batch, {"lt_matmul_batch_native", "lt_matmul_native"}),
            ("lt_matmul_bsgs 3 x 6", bsgs, {"lt_matmul_bsgs_native"})]


FAMILIES = {"basic": basic_cases, "flat": flat_cases, "bsgs": bsgs_cases, "cc_dot": dot_cases, "cc_matmul": matmul_cases, "pc": pc_cases,
            "weighted_sums": wsum_cases, "rotate_hoisted": hoisted_cases, "rotate_sum": rsum_cases, "lt_matmul": ltmm_cases}


def run_family(family, name, last):
    F, fence = fenced_engine(name)
    H, C = plain_engines(name)
    G, K = ops_of(name)
    cases = FAMILIES[family](F, last, name)
    for lv in (lv_rescaling(F, last), lv_rescaling(F, last) + 1, lv_staying(F, last)):
        assert F._native_level(lv) is not None and H._native_level(lv) is not None
    want = []
    for label, f, _ in cases:
        want.append(flat_words(f(H, G)))
        G.keep.check(f"{name} {family} {label} on the unfenced engine")
    for fill_name, fill in FENCE_FILLS.items():
        fence.fill = fill
        for (label, f, entries), w in zip(cases, want):
            what = f"{name} {family} level {'last' if last else 0} {label} fill {fill_name}"
            fence.refill()
            del fence.calls[:], fence.never_written[:]
            got = flat_words(f(F, G))
            fence.check()                                                   # (i) (every entry has checked them on its way out too)
            assert set(fence.calls) == entries, (what, sorted(set(fence.calls)))
            assert not fence.never_written, (what, fence.never_written)
            G.keep.check(what)
            assert_same(got, w, what)                                       # (ii), (iii)
    if name == CHECKED:
        for (label, f, _), w in zip(cases, want):
            assert_same([t.cpu() for t in w], flat_words(f(C, K)), f"{name} {family} {label} against the checker")      # (iv)
            K.keep.check(f"{name} {family} {label} on the checker")


@pytest.mark.parametrize("last", [0, 1], ids=LEVEL_IDS)
@pytest.mark.parametrize("name", SET_NAMES)
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_fenced_family(family, name, last):
    """One op family on one parameter set at level 0 / the last level: see the module docstring for what is asserted."""
    run_family(family, name, last)


# ---- refusals ---------------------------------------------------------------------------------------------------------------
# entry -> its *_ws_words value from the arguments the entry was handed
WS_WORDS = {
    "cc_dot_native": lambda be, a: be.cc_dot_ws_words(a["plan"]),
    "cc_dot_batch_native": lambda be, a: be.cc_dot_batch_ws_words(a["plan"], len(a["np_list"])),
    "cc_matmul_native": lambda be, a: be.cc_matmul_ws_words(a["plan"], len(a["ins"]) // 2),
    "pc_dot_native": lambda be, a: be.pc_dot_ws_words(a["k"], a["rows"], a["logN"]),
    "pc_matmul_native": lambda be, a: be.pc_matmul_ws_words(a["k_in"], a["k_out"], a["rows"], a["logN"]),
    "pc_matmul_batch_native": lambda be, a: be.pc_matmul_batch_ws_words(a["nt"], a["k_in"], a["k_out"], a["rows"], a["logN"]),
    "rotate_hoisted_native": lambda be, a: be.rotate_hoisted_ws_words(a["plan"]),
    "linear_transform_native": lambda be, a: be.linear_transform_ws_words(a["plan"]),
    "linear_transform_batch_native": lambda be, a: be.linear_transform_batch_ws_words(a["plan"], len(a["c0s"])),
    "rotate_sum_native": lambda be, a: be.rotate_sum_ws_words(a["plan"]),
    "rotate_sum_batch_native": lambda be, a: be.rotate_sum_batch_ws_words(a["plan"], len(a["c0s"])),
    "linear_transform_bsgs_native": lambda be, a: be.linear_transform_bsgs_ws_words(a["plan"], len(a["baby_keys"])),
    "linear_transform_bsgs_batch_native": lambda be, a: be.linear_transform_bsgs_batch_ws_words(a["plan"], len(a["baby_keys"]), len(a["c0s"])),
    "lt_matmul_native": lambda be, a: be.lt_matmul_ws_words(a["plan"], max(len(c) for c in a["col_keys"]), len(a["blocks"])),
    "lt_matmul_batch_native": lambda be, a: be.lt_matmul_batch_ws_words(a["plan"], max(len(c) for c in a["col_keys"]), len(a["blocks"]), len(a["toks"])),
    "lt_matmul_bsgs_native": None,          # (its keyed_sums argument is the engine's: the words are taken from the tensor it sized)
}
# the entries whose scratch lives in plan->x4 when the plan has one (the engine's always has): their workspace path is reached
# with a copy of the plan without x4
X4_LENDERS = ("linear_transform_native", "linear_transform_batch_native", "rotate_sum_native", "rotate_sum_batch_native")
# include/ckks_hip.h promises LF_ERR_ARG for a misaligned workspace for every entry but lf_rotate_hoisted, whose workspace only
# carries the sums' planes through the tiled inverse pass: 4- and 2-byte plane stores, 8-byte raw words, one column thread per load
ALIGNED = tuple(n for n in WS_WORDS if n != "rotate_hoisted_native")
assert len(WS_WORDS) == 16


def refusal_cases(eng):
    """entry -> f(engine, ops): one small call that reaches it, at the last level that rescales (two digits: fewer than three, so
    lf_rotate_hoisted needs its workspace there)"""
    lv = lv_rescaling(eng, True)
    two = [[(0, 1), (2,)], [(1, 2), (0,)]]
    two_bsgs = [[(0, 1, 2), (3,)], [(1, 2), (0,)]]

    def ltm(e, o, batch=False, n1=None):
        W, cts, keys = layer(o, lv, two if n1 is None else two_bsgs, n1)
        if batch:
            return e.lt_matmul_batch(W, [cts, cts[::-1]], keys)
        return e.lt_matmul(W, cts, keys) if n1 is None else e.lt_matmul_bsgs(W, cts, keys)
    pairs = lambda o: [(o.ct(50, lv), o.ct(51, lv)), (o.ct(51, lv), o.ct(52, lv))]
    steps, bsteps = (0, 1, 2), (0, 1, 2, 3)
    return {
        "cc_dot_native": lambda e, o: e.cc_dot(pairs(o), o.evk()),
        "cc_dot_batch_native": lambda e, o: e.cc_dot_batch([pairs(o), pairs(o)[:1]], o.evk()),
        "cc_matmul_native": lambda e, o: e.cc_matmul([[o.ct(50, lv), o.ct(51, lv)]] * 2, [[o.ct(51, lv)] * 2, [o.ct(52, lv)] * 2], o.evk()),
        "pc_dot_native": lambda e, o: e.pc_dot([(o.pt(40, lv), o.ct(50, lv))]),
        "pc_matmul_native": lambda e, o: e.pc_matmul(*layer_of(pc_pool(o, lv), 2, 2)),
        "pc_matmul_batch_native": lambda e, o: e.pc_matmul_batch(layer_of(pc_pool(o, lv), 2, 2)[0], [o.cts(2, lv), o.cts(2, lv, 51)],
                                                                 layer_of(pc_pool(o, lv), 2, 2)[2]),
        "rotate_hoisted_native": lambda e, o: e.rotate_hoisted(o.ct(50, lv), [o.key(1), o.key(2)]),
        "linear_transform_native": lambda e, o: e.linear_transform(o.ct(50, lv), o.diags(7, lv, steps), o.keys(steps)),
        "linear_transform_batch_native": lambda e, o: e.linear_transform_batch(o.cts(2, lv), o.diags(7, lv, steps), o.keys(steps)),
        "rotate_sum_native": lambda e, o: e.rotate_sum(o.ct(50, lv), [o.key(1), o.key(2)]),
        "rotate_sum_batch_native": lambda e, o: e.rotate_sum_batch(o.cts(2, lv), [o.key(1), o.key(2)]),
        "linear_transform_bsgs_native": lambda e, o: e.linear_transform(o.ct(50, lv), o.diags(9, lv, bsteps, 2), o.keys(bsteps)),
        "linear_transform_bsgs_batch_native": lambda e, o: e.linear_transform_batch(o.cts(2, lv), o.diags(9, lv, bsteps, 2), o.keys(bsteps)),
        "lt_matmul_native": lambda e, o: ltm(e, o),
        "lt_matmul_batch_native": lambda e, o: ltm(e, o, batch=True),
        "lt_matmul_bsgs_native": lambda e, o: ltm(e, o, n1=2),
    }


def refused(entry, misalign):
    """Runs the entry's case with its workspace replaced by a view into a fenced buffer — one word short of what its own *_ws_words
    returns, or that many words from an address 8 bytes off a 16-byte boundary — and asserts LF_ERR_ARG with every fenced output
    and scratch body still at its fill.  Had the entry launched on the short view, its last word would be the guard's first."""
    from liberate_fhe_amd._native import HipError, KsPlan
    F, fence = fenced_engine(CHECKED)
    G, _ = ops_of(CHECKED)
    f = refusal_cases(F)[entry]
    fence.fill = FENCE_FILLS["ones"]
    fence.ws_hook = None
    want = flat_words(f(F, G))                          # the call as it is: packs, plans and tables exist afterwards
    seen = []

    def hook(name, a):
        if name != entry:
            return
        if entry in X4_LENDERS:
            plan = KsPlan.from_buffer_copy(a["plan"])
            plan.x4 = None
            a["plan"] = plan
        ws = a["ws"]
        words = ws.numel() if WS_WORDS[entry] is None else WS_WORDS[entry](fence.be, a)
        assert words > 0 and (ws is None or ws.numel() == words), (entry, words, None if ws is None else ws.numel())
        key = ("refusal ws", entry, misalign)
        if key not in fence.scratch:
            fence.scratch[key] = fence.alloc(key, (words + 2,), None, F.ntt.devices[0])
        body = fence.scratch[key].body
        a["ws"] = body[1:1 + words] if misalign else body[:words - 1]
        assert a["ws"].data_ptr() % 16 == (8 if misalign else 0)
        fence.refill()                                  # from here on nothing may be written
        consts = [(b, b.flat.clone()) for b in fence.scratch.values() if b.body.data_ptr() in fence.const_ptrs]
        seen.append((list(fence.last_outputs), consts))

    fence.ws_hook = hook
    try:
        with pytest.raises(HipError, match=str(LF_ERR_ARG)):
            f(F, G)
    finally:
        fence.ws_hook = None
    assert len(seen) == 1, (entry, len(seen))
    outputs, consts = seen[0]
    fence.check(outputs)
    assert outputs and all(fence.holds_fill(b) for b in outputs), entry
    for b in fence.scratch.values():
        if b.body.data_ptr() not in fence.const_ptrs:
            assert fence.holds_fill(b), (entry, b.key)
    assert all(torch.equal(b.flat, c) for b, c in consts), entry
    G.keep.check(entry)
    assert_same(flat_words(f(F, G)), want, f"{entry} after the refusal")


@pytest.mark.parametrize("entry", sorted(WS_WORDS))
def test_a_workspace_one_word_short_is_refused(entry):
    refused(entry, misalign=False)


@pytest.mark.parametrize("entry", sorted(ALIGNED))
def test_a_misaligned_workspace_is_refused_where_the_header_says_so(entry):
    """Every entry of ALIGNED documents the refusal in include/ckks_hip.h and tests the address before any launch: nothing is
    ever launched on a misaligned workspace here."""
    hdr = open(os.path.join(ROOT, "include", "ckks_hip.h")).read()
    lf = "lf_" + entry.replace("_native", "")
    doc = hdr[:hdr.index(f"\nint {lf}(")].rsplit("\n/*", 1)[1]           # the comment block before the declaration
    assert "aligned" in doc, lf
    refused(entry, misalign=True)


def test_the_fence_sees_a_kernel_that_writes_past_its_output():
    """The fence on the real backend, not a stub: lf_switch_key is handed its fenced output moved up by one row, so the last row of
    component 1 falls into the guard behind it — inside the fence's own allocation (the guard is a whole polynomial) — and the
    entry's way out reports N changed words from offset 0 behind the output."""
    from tests.helpers import FenceError
    F, fence = fenced_engine(CHECKED)
    G, _ = ops_of(CHECKED)
    N = F.ctx.N
    assert fence.guard >= N

    def hook(name, a):
        if name == "switch_key_native":
            out = a["out"]
            a["out"] = out.as_strided(tuple(out.shape), tuple(out.stride()), out.storage_offset() + N)

    fence.fill, fence.ws_hook = FENCE_FILLS["ones"], hook
    try:
        with pytest.raises(FenceError) as e:
            F.rotate_single(G.ct(50, 0), G.key(1))
    finally:
        fence.ws_hook = None
    msg = str(e.value)
    assert msg.startswith("('switch_key_native', 'out')") and "guard behind" in msg and f"at offset 0 ({N} of" in msg, msg
    fence.check()                                                           # the scratch guards are whole
    assert_same(flat_words(F.rotate_single(G.ct(50, 0), G.key(1))), flat_words(plain_engines(CHECKED)[0].rotate_single(G.ct(50, 0), G.key(1))),
                "rotate_single after the moved output")


# ---- the format knobs ------------------------------------------------------------------------------------------------------
def knob_walk():
    """The body of test_the_format_knobs_leave_guards_and_words; it flips process-wide knobs, so it runs in a process of its own."""
    from liberate_fhe_amd._native import lib
    from liberate_fhe_amd.fhe import ckks_engine
    eng = ckks_engine(devices=["cuda:0"], **params_of(CHECKED))
    fence = Fence(eng, FENCE_FILLS["ones"])
    ops = Ops(ckks_engine(devices=["cuda:0"], **params_of(CHECKED)))
    cases = [FAMILIES[family](eng, 0, CHECKED)[-1] for family in sorted(FAMILIES)]
    first = None
    for planes in (1, 0):
        for more in (3, 0):
            lib.lf_tune(3, planes), lib.lf_tune(5, more)
            got = []
            for label, f, entries in cases:
                fence.refill()
                del fence.calls[:], fence.never_written[:]
                got.append(flat_words(f(eng, ops)))
                fence.check()
                assert set(fence.calls) == entries and not fence.never_written, (planes, more, label, fence.calls, fence.never_written)
                ops.keep.check(f"{label} planes {planes} more {more}")
            if first is None:
                first = got
            for (label, _, _), g, w in zip(cases, got, first):
                assert_same(g, w, f"{label} planes {planes} more {more}")


def test_the_format_knobs_leave_guards_and_words():
    """LF_TUNE_DIGIT_PLANES (1 / 0) x LF_TUNE_MORE_PLANES (3 / 0) on sb41_K2 at level 0 under the all-ones fill, the last case of
    every family: the knobs change what is written into the same scratch.  In a fresh child process (see
    tests/test_cc_dot_gpu.test_tuning_knobs_change_no_word)."""
    import subprocess
    import sys
    code = f"import sys; sys.path.insert(0, {ROOT!r}); from tests.test_fenced_ops_gpu import knob_walk; knob_walk()"
    flags = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable, *flags, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
