"""cc_dot_batch on the GPU: lf_cc_dot_batch (one native call per group of 4 or 2 dots: lf_cc_dot's tensor products per dot, then
ONE inverse transform, digit launch, extension, ks_dotb_inner_kernel<2 | 4> and mod-down for the group) against the loop of cc_dot,
on worst-case words against the composition on the generic path, with compact keys, under the tuning knobs and on two logical
devices.  Conventions (engines kept alive, synthetic keys and operands, knob flips in a child process): tests/test_cc_dot_gpu.py."""
import os

import pytest

from liberate_fhe_amd.utils import synth  # noqa: F401  (the helpers below build their operands with it)
from tests.test_cc_dot_gpu import GOLD, SLOTS, edge_ciphertexts, evk_of, keep, natural_rows, operands, params_of, same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# pair counts per dot: one dot (lf_cc_dot's launches), NCT 2, a leftover single behind a group of 2, NCT 4 with unequal pair
# counts (chunks of 4 + 4 + 1 beside a single pair), groups of 4 + 1 and of 4 + 2 + 1
SHAPES = ((1,), (2, 1), (5, 1, 4), (1, 9, 2, 4), (3, 1, 1, 2, 8), (1, 2, 1, 4, 1, 1, 3))


def dots_of(cts, shape):
    """dot j takes its pairs from SLOTS starting at j: four ciphertexts, (a, a) and (b, a) included, no two dots alike"""
    return [[(cts[a], cts[b]) for a, b in (SLOTS[(j + i) % len(SLOTS)] for i in range(n))] for j, n in enumerate(shape)]


def group_sizes(n):
    """native group sizes of n dots of one level: 4s, then a 2 (a last single dot goes through cc_dot)"""
    return [4] * (n // 4) + ([2] if n % 4 >= 2 else [])


def run_batch(eng, dots, evk, native, calls=None):
    """cc_dot_batch through the native calls, or (native_ops off) through the loop of compositions on the GPU's generic path;
    calls: receives the dot count of every lf_cc_dot_batch call made"""
    be = eng.backend
    old, real = be.native_ops, be.cc_dot_batch_native
    be.native_ops = native
    if calls is not None:
        be.cc_dot_batch_native = lambda plan, np_list, *a, **k: (calls.append(len(np_list)), real(plan, np_list, *a, **k))[1]
    try:
        level = dots[0][0][0].level
        assert (eng._native_level(level + 1) is not None) == native and (eng._native_level(level) is not None) == native
        return eng.cc_dot_batch(dots, evk)
    finally:
        be.native_ops = old
        if calls is not None:
            del be.cc_dot_batch_native


def all_same(got, want):
    return len(got) == len(want) and all(same(g, w) for g, w in zip(got, want))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sb41", "sb45", "silver", "gold", "logN17"])
def test_native_call_equals_the_loop_of_cc_dot(name):
    from liberate_fhe_amd.fhe import ckks_engine
    eng = keep(ckks_engine(devices=["cuda:0"], **params_of(name)))
    evk = evk_of(eng)
    L = eng.num_levels
    for level in sorted({0, 1, L - 2}):
        cts = operands(eng, level, 50 + level)
        loop = {}                                        # cc_dot of a dot, once per distinct list of pairs
        for shape in SHAPES:
            dots = dots_of(cts, shape)
            calls = []
            got = run_batch(eng, dots, evk, True, calls)
            assert sorted(calls, reverse=True) == group_sizes(len(shape)), (name, level, shape, calls)
            assert len(got) == len(shape)
            for j, (pairs, g) in enumerate(zip(dots, got)):
                key = (j % len(SLOTS), len(pairs))
                if key not in loop:
                    loop[key] = eng.cc_dot(pairs, evk)
                assert g.level == level + 1 and not g.ntt_state and not g.include_special
                assert same(g, loop[key]), (name, level, shape, j)
            # one allocation per output: a result kept alive pins no other
            stores = [t.untyped_storage().data_ptr() for g in got for comp in g.data for t in comp]
            assert len({g.data[0][0].untyped_storage().data_ptr() for g in got}) == len(got), (name, level, shape)
            assert len(set(stores)) == len(got)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sb41", "gold"])
def test_worst_case_words(name):
    """Four dots of nine identical pairs of operands at 2q - 1: the largest accumulators in all four lanes of the inner product
    at once; a group mixing dots of zeros, of 2q - 1, of alternating coefficients and of alternating rows; on the small ring
    also operands whose RESCALE is q - 1 everywhere.  Under a key of largest words and a synthetic one, native calls against
    the compositions on the generic path."""
    from liberate_fhe_amd.fhe import ckks_engine
    from tests.helpers import edge_key, pre_rescale_ciphertext
    eng = keep(ckks_engine(devices=["cuda:0"], **params_of(name)))
    for evk in (edge_key(eng, "top", 1), evk_of(eng)):
        for level in (0, eng.num_levels - 2):
            e = edge_ciphertexts(eng, level)
            cases = [[[(e["top"], e["top"])] * 9] * 4,
                     [[(e["zero"], e["zero"])] * 2, [(e["top"], e["top"])] * 5, [(e["even"], e["odd"]), (e["even"], e["even"])],
                      [(e["rows"], e["top"]), (e["top|even"], e["rows"]), (e["rows"], e["rows"])]],
                     [[(e["top"], e["top"])] * 9, [(e["odd"], e["odd"])]]]
            if name == "sb41":   # (built backwards in Python integers: the small ring only)
                pre = [pre_rescale_ciphertext(eng, level, p, 30 + level, shift=i) for i, p in enumerate(("top", "top|0"))]
                cases += [[[(pre[0], pre[0])] * 9] * 4, [[(pre[1], pre[0])] * 9, [(pre[0], e["top"]), (pre[1], pre[1])]]]
            for i, dots in enumerate(cases):
                calls = []
                nat = run_batch(eng, dots, evk, True, calls)
                assert calls == [len(dots)]
                assert all_same(nat, run_batch(eng, dots, evk, False)), (name, level, i)


@pytest.mark.gpu
def test_compact_keys_give_the_same_words():
    from liberate_fhe_amd.fhe import ckks_engine
    eng = keep(ckks_engine(devices=["cuda:0"], **GOLD["sb41"]["params"]))
    sk = eng.create_secret_key()
    evk = eng.create_evk(sk)
    dots = dots_of(operands(eng, 1, 5), (5, 1, 4))
    want = eng.cc_dot_batch(dots, evk)
    assert all_same(want, [eng.cc_dot(pairs, evk) for pairs in dots])
    eng.compact_key(evk)
    assert all_same(eng.cc_dot_batch(dots, evk), want)
    assert all_same(run_batch(eng, dots, evk, False), want)


def knob_walk():
    """The body of test_tuning_knobs_change_no_word; it flips process-wide knobs, so it runs in a process of its own."""
    from liberate_fhe_amd._native import lib
    from liberate_fhe_amd.fhe import ckks_engine
    eng = keep(ckks_engine(devices=["cuda:0"], **GOLD["sb41"]["params"]))
    evk = evk_of(eng)
    dots = dots_of(operands(eng, 0, 12), (9, 1, 2, 4))
    outs = []
    for planes, more, cols in ((1, 3, 5), (0, 3, 5), (1, 0, 5), (1, 3, 0), (0, 0, 0)):
        lib.lf_tune(3, planes), lib.lf_tune(5, more), lib.lf_tune(1, cols)
        calls = []
        outs.append(run_batch(eng, dots, evk, True, calls))
        assert calls == [4]
        outs.append(run_batch(eng, dots, evk, False))
    assert len(outs) == 10 and all(all_same(o, outs[0]) for o in outs[1:])


@pytest.mark.gpu
def test_tuning_knobs_change_no_word():
    """LF_TUNE_DIGIT_PLANES (1 / 0), LF_TUNE_MORE_PLANES (3 / 0) and LF_TUNE_KS_EXT_COLS_MAX (column / LDS-tiled extension), on the
    native call and on the loop of compositions: both key-independent formats the four-triplet kernel reads.  In a fresh child
    process, for the reason tests/test_cc_dot_gpu.py gives."""
    import subprocess
    import sys
    code = f"import sys; sys.path.insert(0, {ROOT!r}); from tests.test_cc_dot_batch_gpu import knob_walk; knob_walk()"
    flags = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable, *flags, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]


@pytest.mark.gpu
def test_gold_on_two_logical_devices_equals_one_device():
    """Two shards take the loop of cc_dot (itself the composition there); row by row in prime order."""
    from liberate_fhe_amd.fhe import ckks_engine
    res = []
    for n_dev in (1, 2):
        eng = keep(ckks_engine(devices=["cuda:0"] * n_dev, **params_of("gold")))
        assert (eng._native_level(1) is not None) == (n_dev == 1)
        evk = evk_of(eng)
        calls = []
        real = eng.backend.cc_dot_batch_native
        eng.backend.cc_dot_batch_native = lambda plan, np_list, *a, **k: (calls.append(len(np_list)), real(plan, np_list, *a, **k))[1]
        rs = eng.cc_dot_batch(dots_of(operands(eng, 0, 8), (3, 2)), evk)
        del eng.backend.cc_dot_batch_native
        assert calls == ([2] if n_dev == 1 else [])
        assert len(rs) == 2 and all(r.level == 1 for r in rs)
        res.append([natural_rows(eng, r) for r in rs])
        del evk, rs
    for one, two in zip(*res):
        for x, y in zip(one, two):
            assert x.shape == y.shape and (x == y).all()
