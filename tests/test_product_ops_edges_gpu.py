"""The product ops added since the two earlier edge files — the encoded-plaintext family pc_mult / pc_add / pc_dot / pc_matmul /
pc_matmul_batch (pc_dot_kernel, pc_matmul_kernel, pc_matmulb_kernel, pc_bias_kernel), weighted_sums and poly_eval(_batch)
(weighted_sums_kernel), cc_dot_batch (ks_dotb_inner_kernel) and cc_matmul (matmul_tensor_kernel) — at worst-case words and on the
edge parameter sets, word for word against the checker engine (tests/oracle_backend.OracleBackend, pinned at these very operands
by tests/test_product_ops_edges_cpu.py).

Their own files compare the native call mostly with the generic path on the same device, which shares the transforms, the rescale,
the digit extension and the mod-down with it, on friendly parameter sets, with plaintexts at two constants.  Here the ciphertexts,
the plaintexts, the biases and the keys sit on the bounds the kernels' range arguments rely on (tests/helpers.py: edge_ciphertext,
edge_plaintext, edge_key, pre_rescale_ciphertext), on the configurations of tests/test_accumulating_ops_edges_gpu.py, whose
engines, key cache, same_ct and native_calls serve here: ten digits of one limb, 8 special primes on one and two logical devices,
both arithmetic classes row by row, a digit of 8 integer-class limbs, 18-bit primes; at level 0 and at the last level the ops
accept; and through the orchestrated path (native op entries off) at logN 13 and 12.  The rescale rounder of the pc entries and of
lf_weighted_sums is driven through its five values by the identity plaintext resp. the weight 1 over a pre_rescale_ciphertext.
Which path ran is counted at the backend's native entries: both leave the checker's words, so a quiet fall-back would otherwise
pass.  No tolerance anywhere: every comparison is torch.equal."""
import contextlib
import warnings

import numpy as np
import pytest
import torch

from liberate_fhe_amd.fhe import encdec
from liberate_fhe_amd.fhe.backend import HipBackend
from tests import test_accumulating_ops_edges_gpu as A
from tests.helpers import edge_ciphertext, edge_plaintext, identity_plaintext, pre_rescale_ciphertext
from tests.test_pc_matmul_gpu import layer_of

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore", category=UserWarning)

CONFIGS, ORCHESTRATED, LEVEL_IDS = A.CONFIGS, A.ORCHESTRATED, A.LEVEL_IDS
# ciphertext pattern, plaintext or key pattern, bias pattern
TRIPLES = (("top", "top", "top"), ("mixed", "top", "mixed"), ("half", "half", "half"), ("top|0", "q|0", "top"),
           ("random", "random", "random"))
DISTINCT = (TRIPLES[1], TRIPLES[4])             # the triples that also run with three distinct objects per side
EVK_PATTERNS = ("top", "random")                # a key of 2q - 1 and a uniform one
PC_DOT_KS = (1, 4, 9)                           # launches of 4, then of 4 + 4 + 1 with the read-back
CI = HipBackend.pc_matmul_chunk                 # inputs per chunk of pc_matmul_kernel (include/ckks_hip.h: LF_PC_MATMUL_CI)
PC_MATMUL_SHAPES = ((CI, 4), (CI + 1, 3))       # a full chunk, the largest fp64 accumulator; read - add - write, output groups 2 + 1
PC_MATMUL_HOLES = (3, 5)                        # tests/test_pc_matmul_gpu.layer_of: holes, an all-None column, groups 4 + 1
PC_BATCH_TOKENS = 3                             # a pair through lf_pc_matmul_batch and one token left over for lf_pc_matmul
WSUM_K, WSUM_G = 16, 5                          # the cap of terms; output launches of 4 + 1
DOT_BATCH = (9, 2, 1, 5, 2, 1, 1)               # pairs per dot: native groups of 4 and 2 dots, the seventh through lf_cc_dot
MATMUL_REDUCE_EVERY = 32                        # csrc/ckks_ks.hip: LF_MATMUL_REDUCE_EVERY (held to the source by the _cpu file)
MATMUL_LONG_CFG = ("sb41_K2", 1)
MATMUL_LONG_INNER = (MATMUL_REDUCE_EVERY + 1, encdec.CC_MATMUL_MAX_INNER)   # across the in-register reduction; the entry's limit
POLY_DEGREE = 7
POLY_COEFFS = np.random.default_rng(7).uniform(-1, 1, POLY_DEGREE + 1)
POLY_PATTERNS = ("mixed", "top", "top|0")       # poly_eval takes the first two, poly_eval_batch all three (a group of 2 and one)
FAMILIES = ("pc_mult_add", "pc_dot", "pc_matmul", "pc_matmul_batch", "weighted_sums", "cc_dot_batch", "cc_matmul", "poly_eval")


class native_args(A.native_calls):
    """A.native_calls that also keeps what `pick` makes of the arguments of every call"""

    def __init__(self, backend, name, pick):
        super().__init__(backend, name)
        self.pick, self.seen = pick, []

    def __enter__(self):
        real = getattr(self.backend, self.name)

        def counted(*args, **kw):
            self.count += 1
            self.seen.append(self.pick(*args, **kw))
            return real(*args, **kw)

        setattr(self.backend, self.name, counted)
        return self


@contextlib.contextmanager
def counting(backend, *names):
    """name -> A.native_calls of several native entries at once"""
    with contextlib.ExitStack() as stack:
        yield {name: stack.enter_context(A.native_calls(backend, name)) for name in names}


def native_at(cfg, H, *levels):
    """whether an op that touches `levels` takes its native entry: every one of them on one device (A.native_expected), which
    the engine's own _native_level must agree with level by level"""
    for lv in levels:
        assert (H._native_level(lv) is not None) == A.native_expected(cfg, H, lv), (cfg, lv)
    return all(A.native_expected(cfg, H, lv) for lv in levels)


def level_of(cfg, last):
    H, C = A.engines(cfg)
    return H, C, A.levels_of(H)[last]


def crt_minus_one(eng, level):
    """The integer that is q_i - 1 on every row of `level`, whichever device holds it: the product of its primes, minus one
    (tests/test_poly_eval_gpu.crt_minus_one over every device)."""
    Q = 1
    for dest in eng.ntt.p.destination_arrays[level]:
        for i in dest:
            Q *= int(eng.ctx.q[i])
    return Q - 1


# ---- the encoded-plaintext family ------------------------------------------------------------------------------------------
def pc_operands(eng, level, triple, n=1):
    """n ciphertexts and n "mult" plaintexts of `level`, n biases of level + 1, of a triple's patterns: each object its own seed"""
    cts = [edge_ciphertext(eng, level, triple[0], 20 + 3 * level + i) for i in range(n)]
    pts = [edge_plaintext(eng, level, triple[1], 40 + 3 * level + i) for i in range(n)]
    adds = [edge_plaintext(eng, level + 1, triple[2], 60 + 3 * level + i, "add") for i in range(n)]
    return cts, pts, adds


def rounder_operands(eng, level, n=1):
    """(identity plaintext, n ciphertexts whose dropped limb holds the rounder's five values, a bias of level + 1)"""
    pres = [pre_rescale_ciphertext(eng, level, "mixed", 30 + level, shift=i) for i in range(n)]
    return identity_plaintext(eng, level), pres, edge_plaintext(eng, level + 1, "mixed", 60 + 3 * level, "add")


def plain_ops(eng, level, triple):
    """[pc_mult, pc_add] of one triple: pc_add takes the bias pattern at the ciphertext's level"""
    (ct,), (pt,), _ = pc_operands(eng, level, triple)
    return [eng.pc_mult(pt, ct), eng.pc_add(edge_plaintext(eng, level, triple[2], 60 + 3 * level, "add"), ct)]


def pc_dot_cases(eng, level):
    """(what, pairs, bias): k = 1, 4, 9 copies of one pair with and without bias under every triple; three distinct objects per
    side under "mixed" and "random"; the rounder case without and with bias"""
    out = []
    for triple in TRIPLES:
        (ct,), (pt,), (b,) = pc_operands(eng, level, triple)
        out += [(f"{'/'.join(triple)} k {k} bias {bias is not None}", [(pt, ct)] * k, bias) for k in PC_DOT_KS for bias in (None, b)]
    for triple in DISTINCT:
        cts, pts, adds = pc_operands(eng, level, triple, 3)
        out.append((f"{'/'.join(triple)} three objects per side", list(zip(pts, cts)), adds[1]))
    ident, (pre,), b = rounder_operands(eng, level)
    return out + [("rounder", [(ident, pre)], None), ("rounder with bias", [(ident, pre)], b)]


def pc_matmul_cases(eng, level):
    """(what, W, cts, bias): the two uniform shapes under every triple, the layout with holes under "mixed" and "random", the
    1 x 2 rounder layer"""
    out = []
    for triple in TRIPLES:
        (ct,), (pt,), (b,) = pc_operands(eng, level, triple)
        out += [(f"{'/'.join(triple)} {k_in} x {k_out}", [[pt] * k_in] * k_out, [ct] * k_in, [b] * k_out) for k_in, k_out in PC_MATMUL_SHAPES]
    for triple in DISTINCT:
        cts, pts, adds = pc_operands(eng, level, triple, 3)
        out.append((f"{'/'.join(triple)} {PC_MATMUL_HOLES} with holes",) + tuple(layer_of((pts, cts, adds[:2]), *PC_MATMUL_HOLES)))
    ident, (pre,), b = rounder_operands(eng, level)
    return out + [("rounder", [[ident], [ident]], [pre], [None, b])]


def pc_batch_cases(eng, level):
    """(what, W, X, bias, (lf_pc_matmul_batch calls, lf_pc_matmul calls) where native): three tokens of the (CI + 1) x 3 layer —
    tokens 0 and 1 differ by a rotation of three ciphertexts, token 2 repeats one object — under "top" and "mixed"; two tokens
    of the rounder layer"""
    k_in, k_out = PC_MATMUL_SHAPES[1]
    out = []
    for triple in TRIPLES[:2]:
        cts, pts, adds = pc_operands(eng, level, triple, 3)
        W = [[pts[(o + i) % 3] for i in range(k_in)] for o in range(k_out)]
        X = [[cts[i % 3] for i in range(k_in)], [cts[(i + 1) % 3] for i in range(k_in)], [cts[0]] * k_in]
        assert len(X) == PC_BATCH_TOKENS
        out.append((f"{'/'.join(triple)} {PC_BATCH_TOKENS} tokens of {k_in} x {k_out}", W, X, [adds[0], None, adds[1]], (1, 1)))
    ident, pres, b = rounder_operands(eng, level, 2)
    return out + [("rounder, two tokens", [[ident], [ident]], [[p] for p in pres], [b, None], (1, 0))]


def checker_pc_matmul(C, W, cts, bias):
    """C.pc_matmul(W, cts, bias) — on the checker the loop of pc_dots over the rows (tests/test_product_ops_edges_cpu.py holds it
    to that on these operands) — with rows of the very same objects computed once"""
    done, out = {}, []
    for row, b in zip(W, bias):
        key = (tuple(id(pt) for pt in row), id(b))
        if key not in done:
            done[key] = C.pc_matmul([row], cts, [b])[0]
        out.append(done[key])
    return out


def check_pc_mult_add(cfg, last):
    H, C, level = level_of(cfg, last)
    for triple in TRIPLES:
        got, want = plain_ops(H, level, triple), plain_ops(C, level, triple)
        assert [g.level for g in got] == [level + 1, level]
        for name, g, w in zip(("pc_mult", "pc_add"), got, want):
            A.same_ct(g, w, f"{cfg} level {level} {name} {'/'.join(triple)}")


def check_pc_dot(cfg, last):
    H, C, level = level_of(cfg, last)
    native = native_at(cfg, H, level, level + 1)
    cases_h, cases_c = pc_dot_cases(H, level), pc_dot_cases(C, level)
    assert len(cases_h) == len(TRIPLES) * len(PC_DOT_KS) * 2 + len(DISTINCT) + 2
    for (what, pairs, bias), (_, pairs_c, bias_c) in zip(cases_h, cases_c):
        with A.native_calls(H.backend, "pc_dot_native") as n:
            got = H.pc_dot(pairs, bias)
        assert n.count == int(native), (cfg, level, what, n.count)
        want = C.pc_dot(pairs_c, bias_c)
        assert got.level == level + 1 and not got.ntt_state and not got.include_special
        A.same_ct(got, want, f"{cfg} level {level} pc_dot {what}")
        if what == "rounder":       # the identity plaintext: exactly the rescale of the operand, on the checker
            A.same_ct(want, C.rescale(pairs_c[0][1]), f"{cfg} level {level} pc_dot by the identity against rescale on the checker")


def check_pc_matmul(cfg, last):
    H, C, level = level_of(cfg, last)
    native = native_at(cfg, H, level, level + 1)
    cases_h, cases_c = pc_matmul_cases(H, level), pc_matmul_cases(C, level)
    assert len(cases_h) == len(TRIPLES) * len(PC_MATMUL_SHAPES) + len(DISTINCT) + 1
    for (what, W, cts, bias), (_, Wc, ctc, bc) in zip(cases_h, cases_c):
        with counting(H.backend, "pc_matmul_native", "pc_dot_native") as n:
            got = H.pc_matmul(W, cts, bias)
        assert (n["pc_matmul_native"].count, n["pc_dot_native"].count) == (int(native), 0), (cfg, level, what)
        want = checker_pc_matmul(C, Wc, ctc, bc)
        assert len(got) == len(want) == len(W)
        for o, (g, w) in enumerate(zip(got, want)):
            assert g.level == level + 1
            A.same_ct(g, w, f"{cfg} level {level} pc_matmul {what} output {o}")


def check_pc_matmul_batch(cfg, last):
    H, C, level = level_of(cfg, last)
    native = native_at(cfg, H, level, level + 1) and 13 <= H.ctx.logN <= 17
    assert tuple(H.pc_matmul_batch_sizes) == (2,)
    for (what, W, X, bias, calls), (_, Wc, Xc, bc, _) in zip(pc_batch_cases(H, level), pc_batch_cases(C, level)):
        with counting(H.backend, "pc_matmul_batch_native", "pc_matmul_native", "pc_dot_native") as n:
            got = H.pc_matmul_batch(W, X, bias)
        seen = (n["pc_matmul_batch_native"].count, n["pc_matmul_native"].count, n["pc_dot_native"].count)
        assert seen == ((calls + (0,)) if native else (0, 0, 0)), (cfg, level, what, seen)
        want = C.pc_matmul_batch(Wc, Xc, bc)
        assert len(got) == len(want) == len(X)
        for t, (gt, wt) in enumerate(zip(got, want)):
            assert len(gt) == len(wt) == len(W)
            for o, (g, w) in enumerate(zip(gt, wt)):
                assert g.level == level + 1
                A.same_ct(g, w, f"{cfg} level {level} pc_matmul_batch {what} token {t} output {o}")


# ---- weighted sums -----------------------------------------------------------------------------------------------------
def wsum_cases(eng, level):
    """(what, cts, integer weights, integer consts): 16 terms over three objects and five outputs — every weight q_i - 1 on every
    row (16 terms of top words: the largest 128-bit sum of weighted_sums_kernel), 1, -1, 0, and q_i - 1 / -1 alternating; consts
    q_i - 1, 0, 1 — under every triple's ciphertext pattern; the weight 1 over one pre_rescale_ciphertext (the rounder)"""
    big, cbig = crt_minus_one(eng, level), crt_minus_one(eng, level + 1)
    ints = [[big] * WSUM_K, [1] * WSUM_K, [-1] * WSUM_K, [0] * WSUM_K, [big if t % 2 == 0 else -1 for t in range(WSUM_K)]]
    consts = [cbig, 0, 1, cbig, cbig]
    assert len(ints) == len(consts) == WSUM_G
    out = []
    for pattern in [t[0] for t in TRIPLES]:
        three = [edge_ciphertext(eng, level, pattern, 20 + 3 * level + i) for i in range(3)]
        out.append((pattern, [three[t % 3] for t in range(WSUM_K)], ints, consts))
    return out + [("rounder", rounder_operands(eng, level)[1], [[1]], None)]


def wsum_native(cfg, H, level):
    """lf_weighted_sums applies where both levels sit on one device and — the engine's own condition — no prime reaches 2^60"""
    return native_at(cfg, H, level, level + 1) and max(H.ctx.q) < (1 << 60)


def check_weighted_sums(cfg, last):
    H, C, level = level_of(cfg, last)
    native = wsum_native(cfg, H, level)
    for (what, cts, ints, consts), (_, ctc, _, _) in zip(wsum_cases(H, level), wsum_cases(C, level)):
        with A.native_calls(H.backend, "weighted_sums_native") as n:
            got = H._weighted_sums_int(cts, ints, consts)
        assert n.count == int(native), (cfg, level, what, n.count)
        want = C._weighted_sums_int(ctc, ints, consts)
        assert len(got) == len(want) == len(ints)
        for g, (a, b) in enumerate(zip(got, want)):
            assert a.level == level + 1 and not a.ntt_state and not a.include_special
            A.same_ct(a, b, f"{cfg} level {level} weighted_sums {what} output {g}")
        if what == "rounder":
            A.same_ct(want[0], C.rescale(ctc[0]), f"{cfg} level {level} the weight 1 against rescale on the checker")


# ---- the cc products ---------------------------------------------------------------------------------------------------
def dot_batch_of(eng, level):
    """seven dots over the three pairs of A.dot_operands, dot j starting at pair j: no two dots alike"""
    pairs = A.dot_operands(eng, level)
    return [[pairs[(j + i) % 3] for i in range(n)] for j, n in enumerate(DOT_BATCH)]


def check_cc_dot_batch(cfg, last):
    H, C, level = level_of(cfg, last)
    native = native_at(cfg, H, level, level + 1)
    assert tuple(H.backend.ks_batch_sizes) == (4, 2)
    dots_h, dots_c = dot_batch_of(H, level), dot_batch_of(C, level)
    for kpat in EVK_PATTERNS:
        with native_args(H.backend, "cc_dot_batch_native", lambda plan, np_list, *a, **kw: list(np_list)) as groups, \
                A.native_calls(H.backend, "cc_dot_native") as single:
            got = H.cc_dot_batch(dots_h, A.evk_of(cfg, H, kpat))
        if native:
            assert sorted(groups.seen, key=len, reverse=True) == [list(DOT_BATCH[:4]), list(DOT_BATCH[4:6])] and single.count == 1, \
                (cfg, level, kpat, groups.seen, single.count)
        else:
            assert groups.count == 0 and single.count == 0, (cfg, level, kpat, groups.count, single.count)
        want = C.cc_dot_batch(dots_c, A.evk_of(cfg, C, kpat))
        assert len(got) == len(want) == len(DOT_BATCH)
        for j, (g, w) in enumerate(zip(got, want)):
            assert g.level == level + 1 and not g.ntt_state and not g.include_special
            A.same_ct(g, w, f"{cfg} level {level} cc_dot_batch evk {kpat} dot {j} of {DOT_BATCH[j]} pairs")


def matmul_cases(eng, level):
    """(evk pattern, what, A, B) over the three distinct ciphertexts of A.dot_operands: 2 x 3 x 2 with a None in A under both keys;
    3 x 3 x 3 (tiles of 2 x 2, 2 x 1, 1 x 2 and 1 x 1 outputs) under the key of 2q - 1"""
    (pa, _), (_, pb), (pc, _) = A.dot_operands(eng, level)
    x = [pa, pb, pc]
    out = [(kpat, "2 x 3 x 2", [[pa, pb, pc], [pb, None, pa]], [[pa, pb], [pb, pc], [pc, pa]]) for kpat in EVK_PATTERNS]
    return out + [("top", "3 x 3 x 3", [[x[(i + t) % 3] for t in range(3)] for i in range(3)],
                   [[x[(2 * t + j) % 3] for j in range(3)] for t in range(3)])]


def check_cc_matmul(cfg, last):
    H, C, level = level_of(cfg, last)
    native = native_at(cfg, H, level, level + 1)
    for (kpat, what, Ah, Bh), (_, _, Ac, Bc) in zip(matmul_cases(H, level), matmul_cases(C, level)):
        with A.native_calls(H.backend, "cc_matmul_native") as n:
            got = H.cc_matmul(Ah, Bh, A.evk_of(cfg, H, kpat))
        assert n.count == int(native), (cfg, level, kpat, what, n.count)
        want = C.cc_matmul(Ac, Bc, A.evk_of(cfg, C, kpat))
        assert len(got) == len(want) == len(Ah)
        for i, (gr, wr) in enumerate(zip(got, want)):
            assert len(gr) == len(wr) == len(Bh[0])
            for j, (g, w) in enumerate(zip(gr, wr)):
                assert g.level == level + 1 and not g.ntt_state and not g.include_special
                A.same_ct(g, w, f"{cfg} level {level} cc_matmul evk {kpat} {what} output ({i}, {j})")
    if cfg != MATMUL_LONG_CFG:
        return
    # 2 x K x 2 of one object whose rescale is "top" everywhere: every output is one cc_dot of K pairs of the checker
    assert native
    top_h, top_c = A.dot_operands(H, level)[0][0], A.dot_operands(C, level)[0][0]
    for K in MATMUL_LONG_INNER:
        with A.native_calls(H.backend, "cc_matmul_native") as n:
            got = H.cc_matmul([[top_h] * K] * 2, [[top_h] * 2] * K, A.evk_of(cfg, H, "top"))
        assert n.count == 1, (cfg, level, K, n.count)
        want = C.cc_dot([(top_c, top_c)] * K, A.evk_of(cfg, C, "top"))
        assert [len(row) for row in got] == [2, 2]
        for i in range(2):
            for j in range(2):
                A.same_ct(got[i][j], want, f"{cfg} level {level} cc_matmul 2 x {K} x 2 output ({i}, {j})")


# ---- poly_eval -----------------------------------------------------------------------------------------------------------
def poly_levels(eng):
    """level 0 and the deepest level at which the engine still accepts the degree"""
    return (0, eng.num_levels - 1 - eng.poly_depth(POLY_DEGREE))


def poly_inputs(eng, level):
    return [pre_rescale_ciphertext(eng, level, p, 30 + level, shift=i) for i, p in enumerate(POLY_PATTERNS)]


def check_poly_eval(cfg, last):
    H, C = A.engines(cfg)
    level = poly_levels(H)[last]
    sched = encdec.poly_schedule(POLY_DEGREE, encdec.poly_split(POLY_DEGREE))
    assert sched["G"] == 2 and level + sched["depth"] == (H.num_levels - 1 if last else sched["depth"])
    Lb, Lc = level + sched["baby"], level + sched["common"]
    sums_native, dot_native = wsum_native(cfg, H, Lb), native_at(cfg, H, Lc, Lc + 1)
    xs_h, xs_c = poly_inputs(H, level), poly_inputs(C, level)
    names = ("weighted_sums_native", "cc_dot_native", "cc_dot_batch_native")
    for kpat in EVK_PATTERNS:
        evk_h, evk_c = A.evk_of(cfg, H, kpat), A.evk_of(cfg, C, kpat)
        want = [C.poly_eval(x, POLY_COEFFS, evk_c) for x in xs_c]
        loop = []
        for x in xs_h:
            with counting(H.backend, *names) as n:
                loop.append(H.poly_eval(x, POLY_COEFFS, evk_h))
            seen = tuple(n[name].count for name in names)
            assert (seen[0] >= 1) == sums_native and (seen[1] >= 1) == dot_native and seen[2] == 0, (cfg, level, kpat, seen)
            assert seen[0] + seen[1] == 0 or sums_native or dot_native
        with counting(H.backend, *names) as n:
            batch = H.poly_eval_batch(xs_h, POLY_COEFFS, evk_h)
        seen = tuple(n[name].count for name in names)
        assert (seen[0] >= 1) == sums_native and (seen[1] >= 1) == dot_native and (seen[2] >= 1) == dot_native, (cfg, level, kpat, seen)
        assert len(batch) == len(loop) == len(want) == len(POLY_PATTERNS)
        for i, (b, g, w) in enumerate(zip(batch, loop, want)):
            assert g.level == level + sched["depth"] and not g.ntt_state and not g.include_special
            if i < 2:
                A.same_ct(g, w, f"{cfg} level {level} poly_eval evk {kpat} from {POLY_PATTERNS[i]}")
            A.same_ct(b, w, f"{cfg} level {level} poly_eval_batch evk {kpat} ciphertext {i} against the checker's poly_eval")
            A.same_ct(b, g, f"{cfg} level {level} poly_eval_batch evk {kpat} ciphertext {i} against the loop on the GPU")


CHECKS = {"pc_mult_add": check_pc_mult_add, "pc_dot": check_pc_dot, "pc_matmul": check_pc_matmul,
          "pc_matmul_batch": check_pc_matmul_batch, "weighted_sums": check_weighted_sums, "cc_dot_batch": check_cc_dot_batch,
          "cc_matmul": check_cc_matmul, "poly_eval": check_poly_eval}
assert tuple(CHECKS) == FAMILIES


@pytest.mark.parametrize("last", [0, 1], ids=LEVEL_IDS)
@pytest.mark.parametrize("name,n_dev", CONFIGS)
def test_pc_mult_and_pc_add_on_edge_words_equal_the_checker(name, n_dev, last):
    """The generic compositions (no entry to count): a ciphertext, a "mult" plaintext and an "add" plaintext of every triple —
    plaintext words at 2q - 1, at the seam of the balanced representation, at the lazy zero q, uniform below 2q."""
    check_pc_mult_add((name, n_dev), last)


@pytest.mark.parametrize("last", [0, 1], ids=LEVEL_IDS)
@pytest.mark.parametrize("name,n_dev", CONFIGS)
def test_pc_dot_on_edge_words_equals_the_checker(name, n_dev, last):
    """lf_pc_dot (pc_dot_kernel<1 | 4>, pc_bias_kernel): k = 1, 4 and 9 copies of one pair, with and without bias, under every
    triple; three distinct objects per side under "mixed" and "random"; and the identity plaintext over an operand whose dropped
    limb holds the rounder's five values, which on the checker is also exactly rescale of that operand.  One native call where
    both levels sit on one device, none otherwise."""
    check_pc_dot((name, n_dev), last)


@pytest.mark.parametrize("last", [0, 1], ids=LEVEL_IDS)
@pytest.mark.parametrize("name,n_dev", CONFIGS)
def test_pc_matmul_on_edge_words_equals_the_checker(name, n_dev, last):
    """lf_pc_matmul (pc_matmul_kernel<4 | 2 | 1>): a full chunk x 4 outputs (the largest fp64 accumulator) and one input past a
    chunk x 3 (the read - add - write path, output groups 2 + 1) of one object per side under every triple; 3 x 5 with holes, an
    all-None column and every second bias None over three objects per side under "mixed" and "random"; the 1 x 2 rounder layer."""
    check_pc_matmul((name, n_dev), last)


@pytest.mark.parametrize("last", [0, 1], ids=LEVEL_IDS)
@pytest.mark.parametrize("name,n_dev", CONFIGS)
def test_pc_matmul_batch_on_edge_words_equals_the_checker(name, n_dev, last):
    """lf_pc_matmul_batch (pc_matmulb_kernel): three tokens of the 17 x 3 layer under "top" and "mixed" — exactly one batched call
    for the pair and one lf_pc_matmul for the token left over — and two tokens of the rounder layer (one batched call)."""
    check_pc_matmul_batch((name, n_dev), last)


@pytest.mark.parametrize("last", [0, 1], ids=LEVEL_IDS)
@pytest.mark.parametrize("name,n_dev", CONFIGS)
def test_weighted_sums_on_edge_words_equal_the_checker(name, n_dev, last):
    """lf_weighted_sums through the integer entry: 16 terms, 5 outputs, weights q_i - 1 / 1 / -1 / 0 on every row, consts q_i - 1 /
    0 / 1, under every ciphertext pattern; the weight 1 over an operand whose dropped limb holds the rounder's five values, which
    on the checker is exactly rescale of that operand.  No edge set holds a prime of 2^60 or more, so the native call is expected
    wherever both levels sit on one device (wsum_native asks the engine's own condition)."""
    check_weighted_sums((name, n_dev), last)


@pytest.mark.parametrize("last", [0, 1], ids=LEVEL_IDS)
@pytest.mark.parametrize("name,n_dev", CONFIGS)
def test_cc_dot_batch_on_edge_words_equals_the_checker(name, n_dev, last):
    """lf_cc_dot_batch (ks_dotb_inner_kernel<4 | 2>): seven dots of 9, 2, 1, 5, 2, 1, 1 pairs whose rescale is an edge pattern,
    under a key of 2q - 1 and a uniform one: native groups of 4 and 2 dots, the seventh through lf_cc_dot."""
    check_cc_dot_batch((name, n_dev), last)


@pytest.mark.parametrize("last", [0, 1], ids=LEVEL_IDS)
@pytest.mark.parametrize("name,n_dev", CONFIGS)
def test_cc_matmul_on_edge_words_equals_the_checker(name, n_dev, last):
    """lf_cc_matmul (matmul_tensor_kernel): 2 x 3 x 2 with a None in A under both keys, 3 x 3 x 3 (all four tile shapes) under the key
    of 2q - 1; on sb41_K2 also 2 x 33 x 2 and 2 x 64 x 2 of one object whose rescale is q - 1 everywhere — across the in-register
    reduction after 32 inner indices and at the entry's limit — against one cc_dot of that many pairs on the checker."""
    check_cc_matmul((name, n_dev), last)


@pytest.mark.parametrize("last", [0, 1], ids=["level0", "deepest_level"])
@pytest.mark.parametrize("name,n_dev", CONFIGS)
def test_poly_eval_on_edge_words_equals_the_checker(name, n_dev, last):
    """poly_eval and poly_eval_batch, power basis, degree 7 (three babies, two blocks, one giant), from operands whose rescale is
    "mixed", "top" and "top|0", under both keys: every result has the checker's poly_eval's words, the batch also those of the
    loop on the GPU.  lf_weighted_sums and lf_cc_dot / lf_cc_dot_batch are reached exactly where the levels they work at sit on
    one device."""
    check_poly_eval((name, n_dev), last)


@pytest.mark.parametrize("op", FAMILIES)
@pytest.mark.parametrize("last", [0, 1], ids=LEVEL_IDS)
@pytest.mark.parametrize("cfg", sorted(ORCHESTRATED))
def test_the_same_cases_through_the_orchestrated_path(cfg, last, op):
    """Native op entries off: the engine's compositions of the same operations at logN 13, and at logN 12 where the key switch
    runs unfused.  No native entry may be reached."""
    CHECKS[op](cfg, last)


def test_the_rounder_case_can_fail():
    """lf_pc_dot handed round_at + 1 (an argument of the backend's Python wrapper: words only): the identity / pre result then
    differs from the checker's exactly on the coefficients whose dropped word is round_at + 1 — one in five along the index, on
    every row of both components — and nowhere else.  The rounder case reads what it claims to read."""
    cfg, level = MATMUL_LONG_CFG, 0
    H, C = A.engines(cfg)
    assert native_at(cfg, H, level, level + 1)
    N = H.ctx.N
    round_at = int(H.ctx.q[H.ntt.p.destination_arrays[level][0][0]]) // 2
    (ident_h, (pre_h,), _), (ident_c, (pre_c,), _) = rounder_operands(H, level), rounder_operands(C, level)
    want = C.pc_dot([(ident_c, pre_c)])
    be, handed = H.backend, []
    real = be.pc_dot_native

    def off_by_one(*args, **kw):
        args = list(args)
        handed.append(args[14])
        args[14] += 1                                   # (round_at: backend.pc_dot_native's 15th argument)
        return real(*args, **kw)

    be.pc_dot_native = off_by_one                       # (an instance attribute over the class's method)
    try:
        got = H.pc_dot([(ident_h, pre_h)])
    finally:
        del be.pc_dot_native
    assert handed == [round_at] and "pc_dot_native" not in vars(be)
    j = torch.arange(N)
    total = 0
    for comp in range(2):
        row0 = pre_c.data[comp][0][0]
        hit = row0 == round_at + 1
        assert torch.equal(hit, (j + 2 * comp) % 5 == 3) and int(hit.sum()) in (N // 5, N // 5 + 1)
        differ = got.data[comp][0].cpu() != want.data[comp][0]
        assert torch.equal(differ, hit.expand_as(differ)), (comp, int(differ.sum()), int(hit.sum()) * differ.size(0))
        total += int(differ.sum())
    print(f"round_at + 1: {total} of {2 * want.data[0][0].numel()} words differ, all on the coefficients whose dropped word is {round_at + 1}")
    A.same_ct(H.pc_dot([(ident_h, pre_h)]), want, "the same case with the entry's own round_at")
