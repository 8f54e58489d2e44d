"""poly_eval_batch on the GPU: the same polynomial on B ciphertexts — every tree step one cc_mult_batch, the recombination one
cc_dot_batch (lf_cc_dot_batch) — against the loop of poly_eval, bit for bit, in both bases, with and without a recombination, on
the small ring of tests/test_poly_eval_gpu.py and once at gold."""
import numpy as np
import pytest

from liberate_fhe_amd.fhe import encdec
from liberate_fhe_amd.utils import synth
from tests.test_poly_eval_gpu import all_same, engine, keep

# (degree, basis, interval, n1): the default split; G = 1 (no dot); a change of variable; a split below the default (G = 4)
POLYS = ((7, "power", None, None), (5, "power", None, 8), (15, "chebyshev", (-3, 5), None), (12, "chebyshev", None, 4))


def dot_calls(eng, monkeypatch):
    calls = []
    real = eng.backend.cc_dot_batch_native
    monkeypatch.setattr(eng.backend, "cc_dot_batch_native",
                        lambda plan, np_list, *a, **k: (calls.append(list(np_list)), real(plan, np_list, *a, **k))[1], raising=False)
    return calls


def check(eng, evk, level, B, degree, basis, interval, n1, calls, seed):
    cts = [synth.ciphertext(eng, seed + i, level) for i in range(B)]
    coeffs = np.random.default_rng(degree).uniform(-1, 1, degree + 1)
    assert eng._native_level(level) is not None and eng._native_level(level + 1) is not None
    n = len(calls)
    got = eng.poly_eval_batch(cts, coeffs, evk, basis=basis, interval=interval, n1=n1)
    made = list(calls[n:])
    want = [eng.poly_eval(ct, coeffs, evk, basis=basis, interval=interval, n1=n1) for ct in cts]
    assert calls[n:] == made                                 # poly_eval itself never takes the batched entry
    depth = eng.poly_depth(degree, basis, interval, n1)
    for g in got:
        assert g.level == level + depth and not g.ntt_state and not g.include_special and g.origin == want[0].origin
    assert all_same(got, want), (B, degree, basis, interval, n1)
    # the recombinations: B dots of G - 1 pairs in groups of 4 and 2 (a last single one through cc_dot); none for G = 1
    G = encdec.poly_schedule(degree, encdec.poly_split(degree) if n1 is None else n1)["G"]
    sizes = [4] * (B // 4) + ([2] if B % 4 >= 2 else [])
    assert sorted(made, reverse=True) == ([[G - 1] * s for s in sizes] if G > 1 else []), (made, G, B)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 3, 5])
def test_poly_eval_batch_equals_the_loop(B, monkeypatch):
    eng = engine("logN13")
    evk = synth.key_switch_key(eng, 77)
    calls = dot_calls(eng, monkeypatch)
    for degree, basis, interval, n1 in POLYS:
        check(eng, evk, 0, B, degree, basis, interval, n1, calls, 90)
    check(eng, evk, 1, B, 7, "power", None, None, calls, 95)     # and from a level above the first


@pytest.mark.gpu
def test_poly_eval_batch_equals_the_loop_at_gold(monkeypatch):
    from liberate_fhe_amd.fhe import ckks_engine
    from tests.test_cc_dot_gpu import params_of
    eng = keep(ckks_engine(devices=["cuda:0"], **params_of("gold")))
    evk = synth.key_switch_key(eng, 77)
    check(eng, evk, 0, 4, 7, "power", None, None, dot_calls(eng, monkeypatch), 90)
