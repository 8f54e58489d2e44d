"""The fused engine kernels (csrc/ckks_fused.hip, ckks_ks.hip, ckks_ops.hip) at worst-case words and at the limits of the
ABI, word for word against the checker (tests/oracle_backend.OracleBackend, pinned at these very operands by
tests/test_engine_edges_cpu.py).

Everywhere else these kernels see uniform random words on the presets' parameter sets.  Here the operands sit on the
bounds their range arguments rely on (tests/helpers.py: edge_rows, step_operands, pre_rescale, rounder_row0) and the
parameter sets go up to what lf_limits advertises: 1, 5, 7 and 8 special primes, digits of 7 and 8 limbs, integer-class
digits of several limbs, both arithmetic classes row by row, 18-bit primes, and the last levels of every chain.

Step tests: every HIP step gets the CHECKER's input of that step (so a wrong word is pinned to the step that made it), writes
into buffers pre-filled with -1 with a guard entry behind them, and must leave the checker's words exactly.
Op tests: the HIP engine against the checker engine on edge ciphertexts and edge keys.  No tolerance anywhere but the
decoded-error line of the real-key case."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

from tests.helpers import (SMALL_PRIME_LIMIT, StepTables, body, edge_ciphertext, edge_key, edge_param_sets, edge_rows, guard_ok,
                           pre_rescale_ciphertext, pre_rescale_rows, rounder_row0, step_operands)

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore", category=UserWarning)

SETS = edge_param_sets()
LARGE = {"logN16_K4": dict(logN=16, scale_bits=40, num_special_primes=4, is_secured=False),
         "logN17_K6": dict(logN=17, scale_bits=40, num_scales=11, num_special_primes=6, is_secured=False)}
LF_NTT_RELAXED, LF_NTT_PLAIN, LF_NTT_PLANES = 1, 2, 16
# data pattern x key pattern.  The key pattern only enters the inner product: "top" keys (2q - 1) meet the two data patterns
# that put the largest and the most unequal words there, the other data patterns run against uniform lazy key words.
PAIRS = (("top", "top"), ("mixed", "top"), ("top|0", "random"), ("half", "random"), ("random", "random"))
_ENGINES = {}


def engines(name, n_dev=1):
    """(HIP engine, checker engine) of a parameter set, built once per process."""
    key = (name, n_dev)
    if key not in _ENGINES:
        from liberate_fhe_amd.fhe import ckks_engine
        from tests.oracle_backend import OracleBackend
        params = {**SETS, **LARGE}[name]
        _ENGINES[key] = (ckks_engine(devices=["cuda:0"] * n_dev, **params),
                         ckks_engine(devices=["cpu"] * n_dev, backend=OracleBackend(), **params))
    return _ENGINES[key]


def edge_levels(eng):
    """Level 0, the last level that still has a multiplication, the last level (ell = 2: a scale limb and the base prime)."""
    return (0, eng.num_levels - 2, eng.num_levels - 1)


def cpu(t):
    return torch.from_numpy(np.ascontiguousarray(t))


def same(got, want, what):
    """`got`: a guarded device buffer; `want`: the checker's tensor."""
    assert guard_ok(got), f"{what}: wrote behind its output"
    g = body(got).cpu()
    if not torch.equal(g, want):
        bad = (g != want).nonzero()
        i = tuple(int(v) for v in bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {want.numel()} words differ, first at {i}: {int(g[i])} != {int(want[i])}")


def mont_enter_rows(be, x, Rs, c):
    """x R mod q (lazy, the checker's mont_enter) of [.., rows, N] host words."""
    from oracle import oracle as orc
    y = np.ascontiguousarray(x).copy()
    flat = y.reshape(-1, y.shape[-2], y.shape[-1])
    for k in range(flat.shape[0]):
        orc.mont_enter(flat[k], Rs.numpy(), flat.shape[1], *be._m(c))
    return y


# ======================================================================================================================
# 3. each step kernel against the checker
# ======================================================================================================================
@pytest.mark.parametrize("name", sorted(SETS))
def test_rescale_kernels_on_the_rounder_values_and_the_negative_word(name):
    """lf_rescale, lf_rescale_batch (1, 4, 8 = LF_BATCH_MAX operand sets) and lf_rescale_ntt (exact; RELAXED; RELAXED | PLAIN;
    | PLANES where lf_stack_planes says 1) on operands built backwards (pre_rescale_rows) so that the result is an edge
    pattern, the dropped limb holding 0, round_at - 1, round_at, round_at + 1, q_drop - 1 in both lanes of every pair.  At the
    target q_i - 1 under a firing rounder the reference leaves the word -1 (tests/test_engine_edges_cpu.py): rescale_kernel
    must too, and the rescale-on-load of lf_rescale_ntt must carry it into the transform as the residue q_i - 1."""
    from liberate_fhe_amd._native import lib, check
    H, C = engines(name)
    hb, cb = H.backend, C.backend
    seen_negative = False
    for level in (0, H.num_levels - 2):
        TH, TC = StepTables(H, level + 1), StepTables(C, level + 1)
        ell, N, logN = TH.ell, TH.N, TH.logN
        q_drop = int(H.ctx.q[level])
        at = q_drop // 2
        pats = ("top", "top|0", "top|1", "half", "mixed", "random", "top", "mixed")
        row0 = [rounder_row0(q_drop, N, shift=k) for k in range(8)]
        src = [pre_rescale_rows(TH.q_ord, q_drop, edge_rows(TH.q_ord, N, p, 70 + k, ids=[i + k for i in TH.ids_ord]), row0[k])
               for k, p in enumerate(pats)]
        want = []
        for k in range(8):
            w = torch.empty((ell, N), dtype=torch.int64)
            cb.rescale(cpu(src[k]), cpu(row0[k]), w, ell, C.rescale_scales[level][0], at, TC.c_ord)
            want.append(w)
        seen_negative |= any(bool((w < 0).any()) for w in want)
        d_src, d_row0 = [TH.put(s) for s in src], [TH.put(r) for r in row0]
        scales = H.rescale_scales[level][0]
        for k in range(8):
            out = TH.new(ell, N)
            hb.rescale(d_src[k], d_row0[k], body(out), ell, scales, at, TH.c_ord)
            same(out, want[k], f"rescale level {level} {pats[k]}")
        for count in (1, 4, 8):
            outs = [TH.new(ell, N) for _ in range(count)]
            hb.rescale_batch(d_src[:count], d_row0[:count], [body(o) for o in outs], ell, scales, at, TH.c_ord)
            for k in range(count):
                same(outs[k], want[k], f"rescale_batch({count}) level {level} {pats[k]}")
        # rescale + forward transform.  Exact form: the checker's words.  RELAXED: their residues, canonical.  RELAXED | PLAIN:
        # fp64-class rows stay in the plain domain (the transform of the rescaled words without the Montgomery entry).
        small = np.array(TH.q_ord) < SMALL_PRIME_LIMIT
        qv = torch.tensor(TH.q_ord)[None, :, None]
        count = 4
        exact = torch.stack(want[:count]).clone()
        cb.ntt(exact, count, ell, logN, TC.psi_ord, TC.Rs_ord, TC.c_ord)
        plain = torch.stack(want[:count]).clone()
        plain = torch.where(plain < 0, plain + qv, plain)                    # the residue of the negative word
        cb.ntt(plain, count, ell, logN, TC.psi_ord, None, TC.c_ord)
        want_plain = torch.where(torch.from_numpy(small)[None, :, None], plain % qv, exact % qv)
        for flags, relaxed, pl, wanted in ((0, False, False, exact), (1, True, False, exact % qv), (3, True, True, want_plain)):
            buf = TH.new(count, ell, N)
            hb.rescale_ntt(d_src[:count], d_row0[:count], body(buf), ell, logN, scales, at, TH.psi_ord, TH.Rs_ord, TH.c_ord,
                           relaxed=relaxed, plain=pl)
            same(buf, wanted, f"rescale_ntt flags {flags} level {level}")
        if lib.lf_stack_planes(logN, ell, TH.c_ord.qptr()) == 1:
            from liberate_fhe_amd.ntt import twiddles
            st = torch.cuda.current_stream().cuda_stream
            buf = TH.new(count, ell, N)
            arr = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
            c = TH.c_ord
            dp = twiddles.dp_pointer(TH.psi_ord, c.ql, c.qh, c.kl, c.kh, 0, st)
            check(lib.lf_rescale_ntt(arr(d_src[:count]), arr(d_row0[:count]), count, buf.data_ptr(), ell, logN, scales.data_ptr(),
                                     at, TH.psi_ord.data_ptr(), dp, c.qptr(), TH.Rs_ord.data_ptr(),
                                     LF_NTT_RELAXED | LF_NTT_PLAIN | LF_NTT_PLANES, c._2q.data_ptr(), *c.mont(), 0, st), "rescale_ntt")
            assert guard_ok(buf)
            pl_words = body(buf).cpu().numpy()
            for r in range(ell):
                if small[r]:
                    lo = pl_words[:, r].view(np.uint32)[:, :N].astype(np.int64)
                    hi = pl_words[:, r].view(np.uint16)[:, 2 * N:3 * N].astype(np.int64)
                    assert ((hi << 32) | lo == want_plain[:, r].numpy()).all(), f"planes of row {r} level {level}"
                else:
                    assert (pl_words[:, r] == want_plain[:, r].numpy()).all(), f"raw row {r} level {level}"
    assert seen_negative == (SETS[name]["scale_bits"] >= 40)       # an fp64-class and (sb41, sb45) an integer-class row


def _step_case(H, C, level, pattern, kpat, seed, slow=False):
    """Every key-switch step at one level on one operand set.  slow (large rings): the unfused extension / inner product and
    the batched cores are left out (the checker's side of them is the expensive part; the small sets run them)."""
    hb, cb = H.backend, C.backend
    TH, TC = StepTables(H, level), StepTables(C, level)
    ell, rows, K, N, logN, nparts = TH.ell, TH.rows, TH.K, TH.N, TH.logN, TH.nparts
    tag = f"level {level} {pattern}/{kpat}"
    op = step_operands(TH, pattern, kpat, seed)
    t = {k: cpu(v) for k, v in op.items()}
    g = {k: TH.put(v) for k, v in op.items()}
    p5 = pow(5, -1, 2 * N)
    small = np.array(TH.q_ord) < SMALL_PRIME_LIMIT

    # ---- tensor product: Montgomery form (lazy words), and the plain-domain form of cc_mult ----
    if not slow:
        want = torch.empty((3, ell, N), dtype=torch.int64)
        cb.tensor(t["x"][0], t["x"][1], t["x"][2], t["x"][3], want[0], want[1], want[2], ell, TC.c_ord)
        got = TH.new(3, ell, N)
        hb.tensor(g["x"][0], g["x"][1], g["x"][2], g["x"][3], got[0], got[1], got[2], ell, TH.c_ord)
        same(got, want, f"tensor {tag}")
        # plain = 1: fp64-class rows hold plain canonical residues and get plain products, canonical; the others as above.
        # The checker's plain product x y: REDC(x * (y R)).
        qv = np.array(TH.q_ord)[None, :, None]
        xp = np.where(small[None, :, None], op["x"] % qv, op["x"])
        xe = mont_enter_rows(cb, xp, TC.Rs_ord, TC.c_ord)
        wp = torch.empty((3, ell, N), dtype=torch.int64)
        cb.tensor(cpu(xp[0]), cpu(xp[1]), cpu(xe[2]), cpu(xe[3]), wp[0], wp[1], wp[2], ell, TC.c_ord)
        want = torch.where(torch.from_numpy(small)[None, :, None], wp % torch.from_numpy(qv), want)
        d_xp = TH.put(xp)
        got = TH.new(3, ell, N)
        hb.tensor(d_xp[0], d_xp[1], d_xp[2], d_xp[3], got[0], got[1], got[2], ell, TH.c_ord, plain=True)
        same(got, want, f"tensor plain {tag}")

    # ---- digits: one polynomial, a batch of three, each also under X -> X^5 (canonical and signed addend form) ----
    srcs_c, srcs_g = [t["a"], t["add"][0], t["add"][1]], [g["a"], g["add"][0], g["add"][1]]
    states = {}
    for gal_name, gal_c, gal_h in (("", None, None), (" galois", (p5, TC.q2_ord), (p5, TH.q2_ord)), (" galois signed", (p5, None), (p5, None))):
        wants = [torch.empty((ell, N), dtype=torch.int64) for _ in range(3)]
        cb.ks_digits_batch(srcs_c, wants, TC.n_digits, TC.d_desc, TC.d_tab, TC.c_ord, galois=gal_c)
        got = TH.new(ell, N)
        hb.ks_digits(g["a"], body(got), TH.n_digits, TH.d_desc, TH.d_tab, TH.c_ord, galois=gal_h)
        same(got, wants[0], f"ks_digits{gal_name} {tag}")
        gots = [TH.new(ell, N) for _ in range(3)]
        hb.ks_digits_batch(srcs_g, [body(x) for x in gots], TH.n_digits, TH.d_desc, TH.d_tab, TH.c_ord, galois=gal_h)
        for k in range(3):
            same(gots[k], wants[k], f"ks_digits_batch{gal_name}[{k}] {tag}")
        states[gal_name] = wants
    st_c = states[""][0]
    st_h = TH.put(st_c.numpy())

    # ---- extension (unfused), from the digits and from digit words at the documented bound; inner product ----
    if not slow:
        for which, sc, sh in (("digits", st_c, st_h), ("bound", t["state_hi"], g["state_hi"])):
            want = torch.empty((nparts, rows, N), dtype=torch.int64)
            cb.ks_extend(sc, want, nparts, rows, TC.e_desc, TC.E, TC.c_all)
            got = TH.new(nparts, rows, N)
            hb.ks_extend(sh, body(got), nparts, rows, TH.e_desc, TH.E, TH.c_all)
            same(got, want, f"ks_extend({which}) {tag}")
        want = torch.empty((2, rows, N), dtype=torch.int64)
        cb.ks_inner(t["ext"], t["key"], TC.first_part, TC.row_off, want[0], want[1], nparts, rows, TC.c_all)
        got = TH.new(2, rows, N)
        hb.ks_inner(g["ext"], g["key"], TH.first_part, TH.row_off, got[0], got[1], nparts, rows, TH.c_all)
        same(got, want, f"ks_inner {tag}")

    # ---- fused core: extension + NTT + inner product + inverse NTT, canonical sums; its two halves; its batches ----
    s_want = None
    if logN >= hb.fused_ks_min_logN:
        core_args_c = (nparts, rows, logN, TC.e_desc, TC.E, TC.Ed, t["key"], TC.first_part, TC.row_off)
        core_args_h = (nparts, rows, logN, TH.e_desc, TH.E, TH.Ed, g["key"], TH.first_part, TH.row_off)
        cases = [("digits", st_c, st_h)] + ([] if slow and pattern != "top" else [("bound", t["state_hi"], g["state_hi"])])
        for which, sc, sh in cases:
            want = torch.empty((2, rows, N), dtype=torch.int64)
            tmp_c = torch.empty((nparts, rows, N), dtype=torch.int64)
            cb.ks_core(sc, *core_args_c, tmp_c, want, TC.psi, TC.ipsi, TC.ninv, TC.c_all)
            if which == "digits":
                s_want = want
            got, tmp = TH.new(2, rows, N), TH.new(nparts, rows, N)
            hb.ks_core(sh, *core_args_h, body(tmp), body(got), TH.psi, TH.ipsi, TH.ninv, TH.c_all)
            same(got, want, f"ks_core({which}) {tag}")
            assert guard_ok(tmp)
            got, tmp = TH.new(2, rows, N), TH.new(nparts, rows, N)
            first = 0
            for count in ([1, nparts - 1] if nparts > 1 else [1]):      # two groups of digits, as they arrive from other devices
                hb.ks_fwd(sh, first, count, rows, logN, TH.e_desc, TH.E, TH.Ed, body(tmp), TH.psi, TH.c_all)
                first += count
            hb.ks_tail(nparts, rows, logN, g["key"], TH.first_part, TH.row_off, body(tmp), body(got), TH.ipsi, TH.ninv, TH.c_all)
            same(got, want, f"ks_fwd + ks_tail({which}) {tag}")
            assert guard_ok(tmp)
        if not slow:
            # batches of 1, 2 and 4 states under one key (NCT 1 / 2 / 4): the digits of a, of the two addends, and the bound words
            pool_c = [st_c, states[""][1], states[""][2], t["state_hi"]]
            for nct in (1, 2, 4):
                sts = torch.stack(pool_c[:nct])
                want = torch.empty((nct, 2, rows, N), dtype=torch.int64)
                cb.ks_core_batch(sts, *core_args_c, torch.empty((nct, nparts, rows, N), dtype=torch.int64), want,
                                 TC.psi, TC.ipsi, TC.ninv, TC.c_all)
                got, tmp = TH.new(nct, 2, rows, N), TH.new(nct, nparts, rows, N)
                hb.ks_core_batch(TH.put(sts.numpy()), *core_args_h, body(tmp), body(got), TH.psi, TH.ipsi, TH.ninv, TH.c_all)
                same(got, want, f"ks_core_batch({nct}) {tag}")
                assert guard_ok(tmp)
        # ---- the fused inner product on hand-made extended digits: x = q - 1 against k = 2q - 1 in every word ("top") ----
        if not slow:
            _inner_on_edge_digits(H, C, TH, TC, op, core_args_h, core_args_c, tag)
        # ---- FOLD (cc_mult's relinearisation inside the inner product): the operand stack at the edge words ----
        if level > 0 and not slow:
            # HIP: fp64-class rows plain canonical residues, the others Montgomery-form words (lf_rescale_ntt RELAXED | PLAIN);
            # the checker: Montgomery form everywhere.  The digits are those of x1 * y1, as the fold requires.
            qv = np.array(TH.q_ord)[None, :, None]
            xh = np.where(small[None, :, None], op["x"] % qv, op["x"])
            xc = np.where(small[None, :, None], mont_enter_rows(cb, xh, TC.Rs_ord, TC.c_ord), xh)
            d2 = torch.empty((1, ell, N), dtype=torch.int64)
            cb.intt_mul(d2, cpu(xc[1]), cpu(xc[3]), 1, ell, logN, TC.ipsi_ord, TC.ninv_ord, TC.c_ord)
            st2 = torch.empty((ell, N), dtype=torch.int64)
            cb.ks_digits(d2[0], st2, TC.n_digits, TC.d_desc, TC.d_tab, TC.c_ord)
            PR_c, PR_h = C._PR(0, level), H._PR(0, level)
            want = torch.empty((2, rows, N), dtype=torch.int64)
            cb.ks_core(st2, *core_args_c, torch.empty((nparts, rows, N), dtype=torch.int64), want, TC.psi, TC.ipsi, TC.ninv, TC.c_all,
                       fold=(cpu(xc), PR_c, TC.own))
            d_x, d_st2 = TH.put(xh), TH.put(st2.numpy())
            got, tmp = TH.new(2, rows, N), TH.new(nparts, rows, N)
            hb.ks_core(d_st2, *core_args_h, body(tmp), body(got), TH.psi, TH.ipsi, TH.ninv, TH.c_all, fold=(d_x, PR_h, TH.own))
            same(got, want, f"ks_core fold {tag}")
            got, tmp = TH.new(2, rows, N), TH.new(nparts, rows, N)
            hb.ks_fwd(d_st2, 0, nparts, rows, logN, TH.e_desc, TH.E, TH.Ed, body(tmp), TH.psi, TH.c_all, own=TH.own)
            hb.ks_tail(nparts, rows, logN, g["key"], TH.first_part, TH.row_off, body(tmp), body(got), TH.ipsi, TH.ninv, TH.c_all,
                       fold=(d_x, PR_h, TH.own))
            same(got, want, f"relin_fwd + relin_tail {tag}")
            for nct in (2, 4):
                got, tmp = TH.new(nct, 2, rows, N), TH.new(nct, nparts, rows, N)
                hb.ks_core_batch(d_st2[None].repeat(nct, 1, 1), *core_args_h, body(tmp), body(got), TH.psi, TH.ipsi, TH.ninv, TH.c_all,
                                 fold=(d_x[None].repeat(nct, 1, 1, 1), PR_h, TH.own))
                same(got, want[None].repeat(nct, 1, 1, 1), f"relin_core_batch({nct}) {tag}")

    # ---- mod-down on the edge sums (and on the core's own output), every form, with / without addend and Galois gather ----
    sums = [(t["s"], g["s"])] + ([] if s_want is None else [(s_want, TH.put(s_want.numpy()))])
    for which, (sc, sh) in enumerate(sums):
        ss_c, ss_h = [sc[0], sc[1], sc[1], sc[0]], [sh[0], sh[1], sh[1], sh[0]]
        adds_c, adds_h = [t["add"][0], None, t["add"][1], t["a"]], [g["add"][0], None, g["add"][1], g["a"]]
        for gal_name, gal_c, gal_h in (("", None, None), (" galois", (p5, TC.q2_ord), (p5, TH.q2_ord)), (" galois signed", (p5, None), (p5, None))):
            wants = [torch.empty((ell, N), dtype=torch.int64) for _ in range(4)]
            cb.ks_moddown_batch(ss_c, wants, adds_c, ell, K, TC.pir, TC.Rs_all, TC.c_all, PiP=None, galois=gal_c)
            what = f"sums {which}{gal_name} {tag}"
            if gal_c is None:
                for k in (0, 1):
                    for pip in (None, TH.pip):
                        got = TH.new(ell, N)
                        hb.ks_moddown(ss_h[k], body(got), adds_h[k], ell, K, TH.pir, TH.Rs_all, TH.c_all, PiP=pip)
                        same(got, wants[k], f"ks_moddown[{k}] PiP {pip is not None} {what}")
            for pip in (None, TH.pip):
                gots = [TH.new(ell, N) for _ in range(4)]
                hb.ks_moddown_batch(ss_h, [body(x) for x in gots], adds_h, ell, K, TH.pir, TH.Rs_all, TH.c_all, PiP=pip, galois=gal_h)
                for k in range(4):
                    same(gots[k], wants[k], f"ks_moddown_batch[{k}] PiP {pip is not None} {what}")
            words = hb.moddown_ws_words(4, ell, K, N)
            ws = torch.full((words + N,), -1, dtype=torch.int64, device=TH.dev)
            gots = [TH.new(ell, N) for _ in range(4)]
            hb.ks_moddown_ws(ss_h, [body(x) for x in gots], adds_h, ell, K, ws[:words], TH.pir, TH.Rs_all, TH.c_all, PiP=TH.pip, galois=gal_h)
            for k in range(4):
                same(gots[k], wants[k], f"ks_moddown_ws[{k}] {what}")
            assert bool((ws[words:] == -1).all()), f"ks_moddown_ws wrote behind its workspace {what}"
            if K <= getattr(hb, "moddown_one_max_K", 0):
                ws = torch.full((words + N,), -1, dtype=torch.int64, device=TH.dev)
                hb.moddown_consts(ws[:words], 4, ell, K, N, TH.pip, TH.c_all)
                gots = [TH.new(ell, N) for _ in range(4)]
                hb.ks_moddown_ws(ss_h, [body(x) for x in gots], adds_h, ell, K, ws[:words], TH.pir, TH.Rs_all, TH.c_all, PiP=TH.pip,
                                 galois=gal_h, one_launch=True)
                for k in range(4):
                    same(gots[k], wants[k], f"ks_moddown_one[{k}] {what}")
                assert bool((ws[words:] == -1).all())

    # ---- Galois map of coefficient rows ----
    for q2_c, q2_h in ((None, None), (TC.q2_ord, TH.q2_ord)):
        wants = [torch.empty((ell, N), dtype=torch.int64) for _ in range(2)]
        cb.galois_batch([t["a"], t["add"][0]], wants, ell, logN, 5, q2_c)
        got = TH.new(ell, N)
        hb.galois(g["a"], body(got), ell, logN, 5, q2_h)
        same(got, wants[0], f"galois {q2_c is not None} {tag}")
        gots = [TH.new(ell, N) for _ in range(2)]
        hb.galois_batch([g["a"], g["add"][0]], [body(x) for x in gots], ell, logN, 5, q2_h)
        for k in range(2):
            same(gots[k], wants[k], f"galois_batch[{k}] {q2_c is not None} {tag}")


def _inner_on_edge_digits(H, C, TH, TC, op, core_args_h, core_args_c, tag):
    """lf_ks_tail (ks_inner2_kernel + the inverse transform) reading extended digits written by hand, in the format lf_ks_fwd
    leaves them in: integer-class rows lazy words, fp64-class rows PLAIN canonical residues — raw words, or (mixed stacks
    under LF_TUNE_DIGIT_PLANES, the default) 32-bit low words in the first half of the row and 16-bit high halves behind
    them.  Random data never puts q - 1 against the lazy key word 2q - 1 (dp_mulmod* is documented for w < q); here every
    word of "top" does.  The checker takes the same residues in Montgomery form."""
    from liberate_fhe_amd._native import lib
    hb, cb = H.backend, C.backend
    rows, N, logN, nparts = TH.rows, TH.N, TH.logN, TH.nparts
    q = np.array(TH.q_all)
    small = q < SMALL_PRIME_LIMIT
    x = np.where(small[None, :, None], op["ext"] % q[None, :, None], op["ext"])
    xc = np.where(small[None, :, None], mont_enter_rows(cb, x, TC.Rs_all, TC.c_all), x)
    want = torch.empty((2, rows, N), dtype=torch.int64)
    cb.ks_tail(*core_args_c[:3], *core_args_c[6:], cpu(xc), want, TC.ipsi, TC.ninv, TC.c_all)
    # (the format follows the process-wide knob as it stands; flipping it here would leave format notes of another setting
    # on memory the allocator recycles, which later calls of this process rightly refuse: LF_ERR_STATE)
    planes = lib.lf_tune(3, -1) == 1 and bool(small.any()) and not bool(small.all())
    words = x.copy()
    if planes:
        for r in np.nonzero(small)[0]:
            row = np.zeros((nparts, N), dtype=np.int64)
            row.view(np.uint32)[:, :N] = (x[:, r] & 0xffffffff).astype(np.uint32)
            row.view(np.uint16)[:, 2 * N:3 * N] = (x[:, r] >> 32).astype(np.uint16)
            words[:, r] = row
    got = TH.new(2, rows, N)
    hb.ks_tail(*core_args_h[:3], *core_args_h[6:], TH.put(words), body(got), TH.ipsi, TH.ninv, TH.c_all)
    same(got, want, f"ks_tail on edge digits (planes {planes}) {tag}")


@pytest.mark.parametrize("name", sorted(SETS))
def test_step_kernels_equal_the_checker_word_for_word(name):
    """tensor, digits (single, batch, Galois), extension, inner product, fused core (whole, in halves, batches of 1 / 2 / 4, with
    FOLD operands, on hand-made extended digits), mod-down (chunked, batch, pivots + closed form, one launch), Galois map:
    level 0 with every pattern pair, the last level with a multiplication and the last level (partial digits; a digit made of
    the base prime alone) with the two "top"-key pairs.  (Three states under one key — a group of 2 and a remainder of 1 — is
    the engine's grouping: cc_mult_batch of 3 pairs and rotate_single_batch of 5 in the op tests below.)"""
    H, C = engines(name)
    levels = edge_levels(H)
    for li, level in enumerate(levels):
        for pi, (pattern, kpat) in enumerate(PAIRS if li == 0 else PAIRS[:2]):
            _step_case(H, C, level, pattern, kpat, 100 + 10 * li + pi)


@pytest.mark.parametrize("name", sorted(LARGE))
def test_step_kernels_on_the_large_rings(name):
    """The column form of the extension at K = 4 (logN 16) and the LDS-tiled ks_ext_pass1 (logN 17, 6 special primes): digits,
    fused core (whole and in halves, from real digits and from words at the bound), mod-down and Galois map on "top" / "top"
    and "mixed" / "top" at level 0, "top" / "top" at the last level.  The checker's side is what takes the time here, so the
    unfused steps and the batches are left to the logN 13 sets (the same kernels, row by row)."""
    H, C = engines(name)
    _step_case(H, C, 0, "top", "top", 300, slow=True)
    _step_case(H, C, 0, "mixed", "top", 301, slow=True)
    _step_case(H, C, H.num_levels - 1, "top", "top", 302, slow=True)


# ======================================================================================================================
# 4. whole ops on edge ciphertexts: HIP engine against checker engine
# ======================================================================================================================
def words(x):
    if isinstance(x, list):
        return [words(v) for v in x]
    return [[t.cpu() for t in comp] for comp in x.data]


def _op_results(eng, levels, hoisted=True):
    """The words of every hot op on edge operands at each level.  Operands that go through a rescale are built backwards
    (pre_rescale_ciphertext): their rescale IS the edge pattern, and their dropped limb holds the five rounder values, so the
    rounders of rescale_kernel (rescale), lf_rescale_ntt (cc_mult without relinearisation, the orchestrated cc_mult) and
    lf_cc_mult_evk* (native cc_mult) all see round_at - 1, round_at, round_at + 1."""
    evk, conjk = edge_key(eng, "top", 1), edge_key(eng, "mixed", 2, origin="conjugation key")
    rotks = [edge_key(eng, "top" if i % 2 == 0 else "random", 3 + i, origin=f"rotation key:{d}") for i, d in enumerate((1, 5, 2, 11, 3))]
    out = {}
    for level in levels:
        res = []
        a, b, c = (edge_ciphertext(eng, level, p, 20 + level) for p in ("top", "mixed", "half"))
        res += [eng.rotate_single(a, rotks[0]), eng.rotate_single(b, rotks[1]), eng.conjugate(a, conjk), eng.conjugate(c, conjk)]
        res += eng.rotate_single_batch([a, b, c, b, a], rotks[0])
        res += [eng.cc_add(a, b), eng.cc_sub(a, b), eng.cc_sub(c, a)]
        if hoisted:
            for n in (1, 2, 4, 5):
                res += eng.rotate_hoisted(b, rotks[:n])
        if level < eng.num_levels - 1:
            pa, pb, pc = (pre_rescale_ciphertext(eng, level, p, 30 + level, shift=i) for i, p in enumerate(("top", "mixed", "top|0")))
            res += [eng.rescale(pa), eng.rescale(pb), eng.rescale(pc)]
            res += [eng.cc_mult(pa, pb, evk), eng.cc_mult(pa, pa, evk), eng.cc_mult(pc, pb, evk)]
            trip = eng.cc_mult(pa, pb, evk, relin=False)
            res += [trip, eng.cc_mult(pc, pa, evk, relin=False)]
            res += eng.cc_mult_batch([(pa, pb), (pb, pc), (pa, pa)], evk)
            res.append(eng.relinearize(eng.cc_mult(pb, pc, evk, relin=False), evk))       # an exact triplet through the public entry
        out[level] = words(res)
    return out


def _compare_ops(H, C, levels, **kw):
    got, want = _op_results(H, levels, **kw), _op_results(C, levels, **kw)
    for level in levels:
        assert len(got[level]) == len(want[level])
        for i, (g, w) in enumerate(zip(got[level], want[level])):
            for ci, (gc, wc) in enumerate(zip(g, w)):
                for di, (gt, wt) in enumerate(zip(gc, wc)):
                    if not torch.equal(gt, wt):
                        n = int((gt != wt).sum())
                        raise AssertionError(f"level {level}, result {i}, component {ci}, device {di}: {n} of {wt.numel()} words differ")


@pytest.mark.parametrize("name,n_dev", [("sb40_K7", 1), ("sb40_K8", 1), ("sb40_K8", 2), ("sb41_K2", 1), ("sb41_K2", 2), ("sb20", 1)])
def test_whole_ops_on_edge_ciphertexts_equal_the_checker_engine(name, n_dev):
    """cc_mult (with and without relinearisation), cc_mult_batch, rescale, rotate_single(_batch), conjugate, rotate_hoisted
    with 1, 2, 4 and 5 keys, relinearize of an exact triplet, cc_add / cc_sub: HIP engine against checker engine, on one and
    (K = 8, sb41) two logical devices, at the three edge levels."""
    H, C = engines(name, n_dev)
    _compare_ops(H, C, edge_levels(H))


def test_whole_ops_silver():
    """The same on the silver preset (logN 15), level 0 and the last level with a multiplication (hoisted rotations, which
    have a file of their own at this size, left out: the checker's side is what takes the time)."""
    from liberate_fhe_amd.fhe import ckks_engine, presets
    from tests.oracle_backend import OracleBackend
    params = {k: v for k, v in presets.params["silver"].items() if k != "devices"}
    H = ckks_engine(devices=["cuda:0"], **params)
    C = ckks_engine(devices=["cpu"], backend=OracleBackend(), **params)
    _compare_ops(H, C, (0, H.num_levels - 2), hoisted=False)


@pytest.mark.parametrize("params", [dict(SETS["sb40_K7"]), dict(SETS["sb40_K7"], logN=12)])
def test_whole_ops_through_the_orchestrated_path(params):
    """Native op entries off (the step-by-step orchestration of the same kernels) at logN 13, and logN 12 where the key
    switch runs unfused (lf_ks_extend, lf_ntt, lf_ks_inner, lf_intt): the checker engine's words."""
    from liberate_fhe_amd.fhe import ckks_engine
    from liberate_fhe_amd.fhe.backend import HipBackend
    from tests.oracle_backend import OracleBackend
    be = HipBackend()
    be.native_ops = False
    H = ckks_engine(devices=["cuda:0"], backend=be, **params)
    C = ckks_engine(devices=["cpu"], backend=OracleBackend(), **params)
    assert H._native_level(0) is None
    _compare_ops(H, C, edge_levels(H))


@pytest.mark.parametrize("K", [7, 8])
def test_real_keys_at_seven_and_eight_special_primes(K):
    """Keys, ciphertexts and noise from the HIP samplers at K = 7 and K = 8; cc_mult + rotate_single on the HIP engine and, on
    the very same tensors, on the checker engine: the words are equal, so the decoded error is the checker's, and the result
    is the rotated product to CKKS accuracy.  Measured on an MI355X (largest slot error against roll(m1 * m2, 3)):
    K = 7: HIP 1.148e-08, checker 1.148e-08; K = 8: HIP 1.031e-08, checker 1.031e-08 — equal, as equal words imply; the
    factor 2 of the last line is never used up."""
    H, C = engines(f"sb40_K{K}")

    def to_cpu(x):
        if isinstance(x, torch.Tensor):
            return x.cpu().clone()
        if hasattr(x, "_replace") and hasattr(x, "data"):
            return x._replace(data=to_cpu(x.data))
        if isinstance(x, tuple):
            return tuple(to_cpu(y) for y in x)
        if isinstance(x, list):
            return [to_cpu(y) for y in x]
        return x

    sk = H.create_secret_key()
    pk, evk, rotk = H.create_public_key(sk), H.create_evk(sk), H.create_rotation_key(sk, 3)
    np.random.seed(K)
    m1, m2 = H.example(-1, 1), H.example(-1, 1)
    c1, c2 = H.encorypt(m1, pk), H.encorypt(m2, pk)
    r_hip = H.rotate_single(H.cc_mult(c1, c2, evk), rotk)
    r_chk = C.rotate_single(C.cc_mult(to_cpu(c1), to_cpu(c2), to_cpu(evk)), to_cpu(rotk))
    for a, b in zip(r_hip.data, r_chk.data):
        assert torch.equal(a[0].cpu(), b[0])
    want = np.roll(m1 * m2, 3)
    err_hip = np.abs(H.decrode(r_hip, sk) - want).max()
    err_chk = np.abs(C.decrode(r_chk, to_cpu(sk)) - want).max()
    print(f"decoded error K = {K}: HIP {err_hip:.3e}, checker {err_chk:.3e}")
    assert err_hip <= 2 * err_chk and err_chk < 1e-6
