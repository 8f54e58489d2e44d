"""cc_matmul on the GPU: lf_cc_matmul (one native call per product: every distinct operand transformed once into a resident store,
matmul_tensor_kernel<R, C> per tile of outputs, lf_cc_dot_batch's steps behind it) against cc_dot of every output's pairs, bit for
bit: on both prime classes, every tile shape, with zero entries and shared objects, on worst-case words against the generic
path, with compact keys, under the tuning knobs and beyond the operand limit of one call.  Conventions (engines kept alive,
synthetic keys and operands, knob flips in a child process): tests/test_cc_dot_gpu.py."""
import os

import pytest

from liberate_fhe_amd.fhe import encdec
from liberate_fhe_amd.utils import synth
from tests.test_cc_dot_gpu import GOLD, edge_ciphertexts, evk_of, keep, params_of, same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# 1 x 1; 2 x 2; all four tile sizes of a matrix (2 x 2, 2 x 1, 1 x 2, 1 x 1); 1 x 4; 4 x 1; 2 x 2 + 2 x 1 with an inner dimension of 1
SHAPES = ((1, 1, 1), (2, 2, 2), (3, 3, 3), (1, 5, 4), (4, 5, 1), (2, 1, 3))


def pool(eng, level, count, seed=50):
    return [synth.ciphertext(eng, seed + i, level) for i in range(count)]


def matrices(cts, shape):
    """A and B of distinct objects, taken from the head of `cts`"""
    m, k, n = shape
    return ([[cts[i * k + t] for t in range(k)] for i in range(m)],
            [[cts[m * k + t * n + j] for j in range(n)] for t in range(k)])


def pairs_of(A, B, i, j):
    return [(A[i][t], B[t][j]) for t in range(len(B)) if A[i][t] is not None and B[t][j] is not None]


def run(eng, A, B, evk, native, calls=None):
    """cc_matmul through the native call, or (native_ops off) through cc_dot's composition on the GPU's generic path;
    calls: receives the (m, k, n) of every lf_cc_matmul call made"""
    be = eng.backend
    old, real = be.native_ops, be.cc_matmul_native
    be.native_ops = native
    if calls is not None:
        be.cc_matmul_native = lambda plan, m, k, n, *a, **kw: (calls.append((m, k, n)), real(plan, m, k, n, *a, **kw))[1]
    try:
        level = next(x for row in A for x in row if x is not None).level
        assert (eng._native_level(level + 1) is not None) == native and (eng._native_level(level) is not None) == native
        return eng.cc_matmul(A, B, evk)
    finally:
        be.native_ops = old
        if calls is not None:
            del be.cc_matmul_native


def generic_dot(eng, pairs, evk):
    """cc_dot through the composition that defines its words, on the GPU's generic path"""
    be = eng.backend
    old = be.native_ops
    be.native_ops = False
    try:
        return eng.cc_dot(pairs, evk)
    finally:
        be.native_ops = old


def check_product(eng, A, B, evk, level, tag, want=None):
    """One native call; every output cc_dot of its pairs, bit for bit, and an allocation of its own.  want: cc_dot results by the
    tuple of the pairs' identities, shared between products that repeat a dot."""
    want = {} if want is None else want
    m, k, n = len(A), len(B), len(B[0])
    calls = []
    got = run(eng, A, B, evk, True, calls)
    assert calls == [(m, k, n)], (tag, calls)
    assert len(got) == m and all(len(r) == n for r in got)
    for i in range(m):
        for j in range(n):
            pairs = pairs_of(A, B, i, j)
            key = tuple((id(a), id(b)) for a, b in pairs)
            if key not in want:
                want[key] = eng.cc_dot(pairs, evk)
            g = got[i][j]
            assert g.level == level + 1 and not g.ntt_state and not g.include_special
            assert same(g, want[key]), (tag, i, j)
    flat = [g for r in got for g in r]
    stores = [t.untyped_storage().data_ptr() for g in flat for comp in g.data for t in comp]
    assert len({g.data[0][0].untyped_storage().data_ptr() for g in flat}) == len(flat) and len(set(stores)) == len(flat), tag
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sb41", "sb45"])
def test_native_call_equals_cc_dot_of_every_output(name):
    from liberate_fhe_amd.fhe import ckks_engine
    eng = keep(ckks_engine(devices=["cuda:0"], **params_of(name)))
    evk = evk_of(eng)
    for level in sorted({0, 1, eng.num_levels - 2}):
        cts = pool(eng, level, max(m * k + k * n for m, k, n in SHAPES), 50 + level)
        for shape in SHAPES:
            A, B = matrices(cts, shape)
            check_product(eng, A, B, evk, level, (name, level, shape))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["silver", "gold", "logN17"])
def test_larger_rings(name):
    """3 x 3 x 3: the four tile sizes of a matrix in one product"""
    from liberate_fhe_amd.fhe import ckks_engine
    eng = keep(ckks_engine(devices=["cuda:0"], **params_of(name)))
    evk = evk_of(eng)
    for level in sorted({0, eng.num_levels - 2}):
        A, B = matrices(pool(eng, level, 18, 50 + level), (3, 3, 3))
        check_product(eng, A, B, evk, level, (name, level))


@pytest.mark.gpu
def test_zero_entries_and_shared_objects():
    from liberate_fhe_amd.fhe import ckks_engine
    eng = keep(ckks_engine(devices=["cuda:0"], **params_of("sb41")))
    evk = evk_of(eng)
    for level in (0, eng.num_levels - 2):
        cts = pool(eng, level, 18, 80 + level)
        # zero entries that leave outputs of one, two and three terms; a whole zero column of A against a full row of B
        A, B = matrices(cts, (3, 3, 3))
        A[0][1] = A[0][2] = A[2][0] = None
        B[1][1] = B[2][2] = None
        terms = sorted({len(pairs_of(A, B, i, j)) for i in range(3) for j in range(3)})
        assert terms == [1, 2, 3], terms
        check_product(eng, A, B, evk, level, ("holes", level))
        A2 = [[cts[0], None, cts[1]], [cts[2], None, cts[3]]]
        check_product(eng, A2, B, evk, level, ("zero column", level))
        # cc_matmul(A, A), a ciphertext repeated inside A, and B sharing objects with A
        S = [[cts[0], cts[1], cts[0]], [cts[2], cts[0], cts[3]], [cts[1], cts[1], cts[4]]]
        check_product(eng, S, S, evk, level, ("A A", level))
        A3, B3 = matrices(cts, (2, 3, 2))
        B3[0][0], B3[2][1], B3[1][0] = A3[0][0], A3[1][2], A3[0][0]
        check_product(eng, A3, B3, evk, level, ("shared", level))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sb41", "gold"])
def test_worst_case_words(name):
    """The inner dimension LF_CC_MATMUL_MAX_INNER with every operand at 2q - 1, 2 x 2 outputs: the largest accumulators, across the
    reduction in registers, in every lane of every tile; a product mixing operands of zeros, of alternating coefficients and of
    alternating rows.  Under a key of largest words and a synthetic one, the native call against the composition on the generic
    path (computed once per distinct dot)."""
    from liberate_fhe_amd.fhe import ckks_engine
    from tests.helpers import edge_key
    eng = keep(ckks_engine(devices=["cuda:0"], **params_of(name)))
    K = encdec.CC_MATMUL_MAX_INNER
    for evk in (edge_key(eng, "top", 1), evk_of(eng)):
        for level in (0, eng.num_levels - 2):
            e = edge_ciphertexts(eng, level)
            top = e["top"]
            calls = []
            got = run(eng, [[top] * K] * 2, [[top] * 2] * K, evk, True, calls)
            assert calls == [(2, K, 2)]
            want = generic_dot(eng, [(top, top)] * K, evk)
            assert all(same(got[i][j], want) for i in range(2) for j in range(2)), (name, level)
            A = [[e["zero"], e["top"], e["even"], e["rows"]], [e["odd"], e["even"], e["top|even"], e["zero"]]]
            B = [[e["zero"], e["odd"]], [e["rows"], e["top"]], [e["even"], e["odd"]], [e["top"], e["rows"]]]
            calls = []
            got = run(eng, A, B, evk, True, calls)
            assert calls == [(2, 4, 2)]
            for i in range(2):
                for j in range(2):
                    assert same(got[i][j], generic_dot(eng, pairs_of(A, B, i, j), evk)), (name, level, i, j)


@pytest.mark.gpu
def test_compact_keys_give_the_same_words():
    from liberate_fhe_amd.fhe import ckks_engine
    eng = keep(ckks_engine(devices=["cuda:0"], **GOLD["sb41"]["params"]))
    sk = eng.create_secret_key()
    evk = eng.create_evk(sk)
    A, B = matrices(pool(eng, 1, 18, 5), (3, 3, 3))
    want = check_product(eng, A, B, evk, 1, "real key")
    eng.compact_key(evk)
    flat = lambda C: [c for r in C for c in r]
    assert all(same(g, w) for g, w in zip(flat(run(eng, A, B, evk, True)), flat(want)))
    assert all(same(g, w) for g, w in zip(flat(run(eng, A, B, evk, False)), flat(want)))


def knob_walk():
    """The body of test_tuning_knobs_change_no_word; it flips process-wide knobs, so it runs in a process of its own."""
    from liberate_fhe_amd._native import lib
    from liberate_fhe_amd.fhe import ckks_engine
    eng = keep(ckks_engine(devices=["cuda:0"], **GOLD["sb41"]["params"]))
    evk = evk_of(eng)
    A, B = matrices(pool(eng, 0, 18, 12), (3, 3, 3))
    outs = []
    for planes, more, cols in ((1, 3, 5), (0, 3, 5), (1, 0, 5), (1, 3, 0), (0, 0, 0)):
        lib.lf_tune(3, planes), lib.lf_tune(5, more), lib.lf_tune(1, cols)
        calls = []
        outs.append([c for r in run(eng, A, B, evk, True, calls) for c in r])
        assert calls == [(3, 3, 3)]
        outs.append([c for r in run(eng, A, B, evk, False) for c in r])
    assert len(outs) == 10 and all(len(o) == 9 and all(same(x, y) for x, y in zip(o, outs[0])) for o in outs[1:])


@pytest.mark.gpu
def test_tuning_knobs_change_no_word():
    """LF_TUNE_DIGIT_PLANES (1 / 0), LF_TUNE_MORE_PLANES (3 / 0) and LF_TUNE_KS_EXT_COLS_MAX (column / LDS-tiled extension), on the
    native call and on the generic path: the formats of the store the tensor kernel reads and of what runs behind it.  In a fresh
    child process, for the reason tests/test_cc_dot_gpu.py gives."""
    import subprocess
    import sys
    code = f"import sys; sys.path.insert(0, {ROOT!r}); from tests.test_cc_matmul_gpu import knob_walk; knob_walk()"
    flags = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable, *flags, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]


@pytest.mark.gpu
def test_beyond_the_operand_limit_the_rows_split_over_calls():
    """5 x 52 distinct entries in A and a B sharing A's first row: 260 distinct operands, above LF_CC_MATMUL_MAX_OPERANDS — two native
    calls (rows 0 .. 3, then row 4), the words of the rows taken one at a time."""
    from liberate_fhe_amd.fhe import ckks_engine
    eng = keep(ckks_engine(devices=["cuda:0"], **params_of("sb41")))
    evk = evk_of(eng)
    level, k = eng.num_levels - 2, 52
    cts = pool(eng, level, 5 * k, 200)
    A = [cts[i * k:(i + 1) * k] for i in range(5)]
    B = [[A[0][t]] for t in range(k)]
    assert 5 * k > encdec.CC_MATMUL_MAX_OPERANDS
    calls = []
    got = run(eng, A, B, evk, True, calls)
    assert calls == [(4, k, 1), (1, k, 1)]
    for i in range(5):
        calls = []
        row = run(eng, [A[i]], B, evk, True, calls)
        assert calls == [(1, k, 1)] and same(got[i][0], row[0][0]), i
    assert same(got[0][0], eng.cc_dot(pairs_of(A, B, 0, 0), evk))
