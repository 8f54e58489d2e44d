"""cc_dot on the GPU: lf_cc_dot (one native call: dot_tensor_kernel per chunk of pairs, ks_inner2_presum_kernel, between the
existing steps) against the composition that defines its words on the GPU's generic path, against cc_mult for one pair, on
worst-case words, against the checker engine, with compact keys, under the tuning knobs, on two logical devices, and decrypted
with real keys against the chain of cc_mults on the same inputs."""
import json
import os

import numpy as np
import pytest
import torch

from liberate_fhe_amd.utils import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "engine_digests.json")))
DOT = dict(logN=13, num_scales=5, num_special_primes=2, is_secured=False)
KS = (1, 2, 3, 4, 5, 8, 9)          # chunks of 4, 2 and 1 pairs; the first chunk's write and the later adds
# (index of the left, of the right operand) among four ciphertexts: objects repeat, (a, a) and (a, b), (b, a) included
SLOTS = ((0, 1), (1, 0), (0, 0), (2, 3), (3, 1), (2, 2), (1, 3), (3, 0), (2, 1))


def words(ct):
    return [torch.cat([t.cpu() for t in comp]) for comp in ct.data]


def same(a, b):
    return a.level == b.level and a.origin == b.origin and all(torch.equal(x, y) for x, y in zip(words(a), words(b)))


def params_of(name):
    from liberate_fhe_amd.fhe import presets
    if name in ("silver", "gold"):
        return {k: v for k, v in presets.params[name].items() if k != "devices"}
    if name == "logN17":
        return dict(logN=17, num_scales=3, num_special_primes=2, is_secured=False)     # the five-stage column split
    return GOLD[name]["params"]


_KEEP = []


def keep(eng):
    """Engines of this file live as long as the process.  The library notes the format (planes / raw) its calls leave in an
    engine's scratch and refuses a later reader of another format once a format knob has been flipped in between (LF_ERR_STATE);
    it cannot know that a buffer was freed.  This file runs before the suite's first knob-flipping test, so scratch freed here
    and recycled by a later test would carry such a note: the scratch is therefore never freed."""
    _KEEP.append(eng)
    return eng


def evk_of(eng, seed=77):
    return synth.key_switch_key(eng, seed)


def operands(eng, level, seed=50):
    return [synth.ciphertext(eng, seed + i, level) for i in range(4)]


def pairs_of(cts, k):
    return [(cts[i], cts[j]) for i, j in SLOTS[:k]]


def composition(eng, pairs, evk):
    t = eng.cc_mult(pairs[0][0], pairs[0][1], evk, relin=False)
    for a, b in pairs[1:]:
        t = eng.cc_add_triplet(t, eng.cc_mult(a, b, evk, relin=False))
    return eng.relinearize(t, evk)


def run(eng, pairs, evk, native):
    """cc_dot through the native call, or (native_ops off) through the composition on the GPU's generic path"""
    be = eng.backend
    old = be.native_ops
    be.native_ops = native
    try:
        level = pairs[0][0].level
        assert (eng._native_level(level + 1) is not None) == native and (eng._native_level(level) is not None) == native
        return eng.cc_dot(pairs, evk)
    finally:
        be.native_ops = old


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["silver", "sb45", "sb41", "gold", "logN17"])
def test_native_call_equals_the_composition(name):
    from liberate_fhe_amd.fhe import ckks_engine
    eng = keep(ckks_engine(devices=["cuda:0"], **params_of(name)))
    evk = evk_of(eng)
    L = eng.num_levels
    for level in sorted({0, 1, L - 2}):
        cts = operands(eng, level, 50 + level)
        for k in KS:
            pairs = pairs_of(cts, k)
            nat, gen = run(eng, pairs, evk, True), run(eng, pairs, evk, False)
            assert nat.level == level + 1 and not nat.ntt_state and not nat.include_special
            assert same(nat, gen), (name, level, k)
            if k == 3:   # the generic path IS the composition written out
                assert same(gen, composition(eng, pairs, evk)), (name, level)
        # one pair: cc_mult's words
        a, b = cts[0], cts[1]
        assert same(eng.cc_dot([(a, b)], evk), eng.cc_mult(a, b, evk)), (name, level)
        assert same(eng.cc_dot([(a, a)], evk), eng.cc_mult(a, a, evk)), (name, level)


def edge_ciphertexts(eng, level):
    """Lazy operands at the bounds: every word 2q - 1; every word 0; whole rows alternating between the two; coefficients
    alternating between the two (and the other way round)."""
    dest = eng.ntt.p.destination_arrays[level][0]
    q = torch.tensor([int(eng.ctx.q[i]) for i in dest], dtype=torch.int64).view(-1, 1)
    N = eng.ctx.N
    top = (2 * q - 1).expand(-1, N).contiguous()
    zero = torch.zeros_like(top)
    rows = top.clone()
    rows[1::2] = 0
    even = top.clone()
    even[:, 1::2] = 0
    odd = top.clone()
    odd[:, 0::2] = 0
    base = synth.ciphertext(eng, 1, level)
    dev = eng.ntt.devices[0]
    mk = lambda c0, c1: base._replace(data=([c0.clone().to(dev)], [c1.clone().to(dev)]))
    return {"top": mk(top, top), "zero": mk(zero, zero), "rows": mk(rows, top), "even": mk(even, odd), "odd": mk(odd, top),
            "top|even": mk(top, even)}


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sb41", "gold"])
def test_worst_case_words(name):
    """Operands at 2q - 1 and 0 on whole rows and on alternating coefficients, and operands whose RESCALE is q - 1 everywhere
    (tests/helpers.pre_rescale_ciphertext: the largest products); k = 9 with the same ciphertext in every slot gives the
    largest accumulator the kernel can meet (two chunks of 4 and one of 1).  Native call against the composition."""
    from liberate_fhe_amd.fhe import ckks_engine
    from tests.helpers import edge_key, pre_rescale_ciphertext
    eng = keep(ckks_engine(devices=["cuda:0"], **params_of(name)))
    for evk in (edge_key(eng, "top", 1), evk_of(eng)):
        for level in (0, eng.num_levels - 2):
            e = edge_ciphertexts(eng, level)
            cases = [[(e["top"], e["top"])] * 9, [(e["even"], e["even"])] * 9, [(e["zero"], e["zero"])] * 2,
                     [(e["top"], e["zero"]), (e["rows"], e["top"]), (e["even"], e["odd"]), (e["top|even"], e["rows"]), (e["odd"], e["odd"])]]
            if name == "sb41":   # (built backwards in Python integers: the small ring only)
                pre = [pre_rescale_ciphertext(eng, level, p, 30 + level, shift=i) for i, p in enumerate(("top", "top|0"))]
                cases += [[(pre[0], pre[0])] * 9, [(pre[1], pre[0])] * 9, [(pre[0], e["top"]), (pre[1], pre[1])]]
            for i, pairs in enumerate(cases):
                assert same(run(eng, pairs, evk, True), run(eng, pairs, evk, False)), (name, level, i)


@pytest.mark.gpu
@pytest.mark.parametrize("params", [DOT, dict(DOT, logN=12)])
def test_gpu_equals_the_checker(params):
    """logN 13 (the native call) and logN 12 (no native path: the composition over the unfused steps) against the checker engine."""
    from liberate_fhe_amd.fhe import ckks_engine
    from tests.oracle_backend import OracleBackend
    got, want = [], []
    for eng, out in ((keep(ckks_engine(devices=["cuda:0"], **params)), got), (ckks_engine(devices=["cpu"], backend=OracleBackend(), **params), want)):
        evk = evk_of(eng)
        if str(eng.ntt.devices[0]).startswith("cuda"):
            assert (eng._native_level(1) is not None) == (params["logN"] >= 13)
        for level in (0, 2):
            cts = operands(eng, level, 70 + level)
            out += [words(eng.cc_dot(pairs_of(cts, k), evk)) for k in (1, 2, 5, 9)]
    assert len(got) == len(want) == 8
    assert all(torch.equal(a[c], b[c]) for a, b in zip(got, want) for c in range(2))


@pytest.mark.gpu
def test_compact_keys_give_the_same_words():
    from liberate_fhe_amd.fhe import ckks_engine
    eng = keep(ckks_engine(devices=["cuda:0"], **GOLD["sb41"]["params"]))
    sk = eng.create_secret_key()
    evk = eng.create_evk(sk)
    pairs = pairs_of(operands(eng, 1, 5), 5)
    want = eng.cc_dot(pairs, evk)
    assert same(want, run(eng, pairs, evk, False))
    eng.compact_key(evk)
    assert same(eng.cc_dot(pairs, evk), want)
    assert same(run(eng, pairs, evk, False), want)


def knob_walk():
    """The body of test_tuning_knobs_change_no_word; it flips process-wide knobs, so it runs in a process of its own."""
    from liberate_fhe_amd._native import lib
    from liberate_fhe_amd.fhe import ckks_engine
    eng = keep(ckks_engine(devices=["cuda:0"], **GOLD["sb41"]["params"]))
    evk = evk_of(eng)
    pairs = pairs_of(operands(eng, 0, 12), 9)
    outs = []
    for planes, more, cols in ((1, 3, 5), (0, 3, 5), (1, 0, 5), (1, 3, 0), (0, 0, 0)):
        lib.lf_tune(3, planes), lib.lf_tune(5, more), lib.lf_tune(1, cols)
        outs.append(run(eng, pairs, evk, True))
        outs.append(run(eng, pairs, evk, False))
    assert len(outs) == 10 and all(same(o, outs[0]) for o in outs[1:])


@pytest.mark.gpu
def test_tuning_knobs_change_no_word():
    """LF_TUNE_DIGIT_PLANES (1 / 0), LF_TUNE_MORE_PLANES (3 / 0) and LF_TUNE_KS_EXT_COLS_MAX (column / LDS-tiled extension), on the
    native call and on the composition.  In a fresh child process: every flip of a format knob ages the library's notes of what
    format earlier calls left in scratch, and this file runs before the others of the suite — a later test whose tensors land on
    recycled memory would be refused with LF_ERR_STATE for a note this one made stale."""
    import subprocess
    import sys
    code = f"import sys; sys.path.insert(0, {ROOT!r}); from tests.test_cc_dot_gpu import knob_walk; knob_walk()"
    flags = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable, *flags, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]


def natural_rows(eng, ct):
    """Components as [rows, N] arrays with the rows in the order of the prime chain (tests/test_engine_golden.py)."""
    dest = eng.ntt.p.destination_arrays[ct.level]
    out = []
    for comp in ct.data:
        rows = {}
        for d, t in enumerate(comp):
            arr = t.cpu().numpy()
            for r, prime in enumerate(dest[d]):
                rows[prime] = arr[r]
        out.append(np.stack([rows[k] for k in sorted(rows)]))
    return out


@pytest.mark.gpu
def test_gold_on_two_logical_devices_equals_one_device():
    """Two shards take the composition (a digit exchange inside its one relinearisation); row by row in prime order."""
    from liberate_fhe_amd.fhe import ckks_engine
    res = []
    for n_dev in (1, 2):
        eng = keep(ckks_engine(devices=["cuda:0"] * n_dev, **params_of("gold")))
        assert (eng._native_level(1) is not None) == (n_dev == 1)
        evk = evk_of(eng)
        r = eng.cc_dot(pairs_of(operands(eng, 0, 8), 5), evk)
        assert r.level == 1
        res.append(natural_rows(eng, r))
        del evk, r
    for x, y in zip(*res):
        assert x.shape == y.shape and (x == y).all()


@pytest.mark.gpu
def test_real_keys_decrypt_within_twice_the_chain_on_silver():
    """silver, real keys, eight pairs of messages uniform in [-1, 1]: max |decrode(cc_dot) - sum m_a m_b| is at most 2 x that of
    cc_add over cc_mult_batch of the same ciphertexts (the op adds the noise of one key switch where the chain adds eight; 2 x
    is the margin this project uses for a maximum over 2^14 slots).  Both errors are printed."""
    from liberate_fhe_amd.fhe import ckks_engine, presets
    eng = keep(ckks_engine(**{**presets.params["silver"], "devices": ["cuda:0"]}))
    sk = eng.create_secret_key()
    pk = eng.create_public_key(sk)
    evk = eng.create_evk(sk)
    np.random.seed(5)
    ms = [(eng.example(-1, 1), eng.example(-1, 1)) for _ in range(8)]
    pairs = [(eng.encorypt(ma, pk), eng.encorypt(mb, pk)) for ma, mb in ms]
    want = sum(ma * mb for ma, mb in ms)
    assert eng._native_level(1) is not None
    got = eng.cc_dot(pairs, evk)
    assert got.level == 1
    chain = None
    for p in eng.cc_mult_batch(pairs, evk):
        chain = p if chain is None else eng.cc_add(chain, p)
    err_dot = np.abs(eng.decrode(got, sk) - want).max()
    err_chain = np.abs(eng.decrode(chain, sk) - want).max()
    print(f"silver, k = 8: cc_dot max abs error {err_dot:.3e}, cc_add over cc_mult_batch {err_chain:.3e}, "
          f"largest entry {np.abs(want).max():.2f}")
    assert err_dot <= 2 * err_chain, (err_dot, err_chain)
