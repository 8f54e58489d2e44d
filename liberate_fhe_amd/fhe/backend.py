"""Device arithmetic behind the engine: thin tensor-level wrappers over the C ABI (include/ckks_hip.h).

`HipBackend` is the only backend in the package and it has no fallback — every method launches a HIP
kernel through libckks_hip.so on the tensor's GPU and current torch stream.  The engine takes the
backend as an object so that the multi-rank orchestration (which is backend-agnostic Python) can be
exercised by the CPU test-suite with a checker backend that lives under tests/.
"""
from __future__ import annotations

import ctypes

import torch

from .._native import lib, check, KsPlan, LF_KEY_PLANES, LF_LT_MATMUL_BSGS_MAX_GIANTS, LF_LT_MATMUL_BSGS_MAX_SUMS, LF_LT_BATCH_MAX_CTS, \
    LF_LT_MATMUL_BATCH_MAX_TOKENS, LF_LT_MATMUL_BSGS_BATCH_MAX_TOKENS, LF_LIMIT_SMALL_PRIME_BITS, LF_PLAIN_PLANES_MAX_ROWS
from ..ntt import ntt_cuda, twiddles

# the bound of the fp64 class, from the library (include/ckks_hip.h: LF_LIMIT_SMALL_PRIME_BITS): a row whose prime is below it is
# kept as 6-byte planes where a format has them
SMALL_PRIME_LIMIT = 1 << int(lib.lf_limits(LF_LIMIT_SMALL_PRIME_BITS))

_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)   # the stream handle without a Stream object per call


def _ds(t: torch.Tensor):
    if t.device.type != "cuda":
        raise RuntimeError(f"HipBackend: tensor on {t.device}; device memory required (no CPU fallback)")
    idx = t.device.index if t.device.index is not None else torch.cuda.current_device()
    if _raw_stream is not None:
        return idx, _raw_stream(idx)
    return idx, torch.cuda.current_stream(idx).cuda_stream


def _p(t):
    if t is None:
        return 0
    if t.dtype != torch.int64:
        raise TypeError(f"HipBackend: int64 tensor required, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError("HipBackend: contiguous tensor required (the kernels take a raw pointer and a row pitch of N words)")
    return t.data_ptr()


def _pb(t):
    """Device pointer of a uint8 table (None -> NULL)."""
    if t is None:
        return 0
    if t.dtype != torch.uint8 or not t.is_contiguous():
        raise TypeError("HipBackend: contiguous uint8 tensor required")
    return t.data_ptr()


def _pd(t):
    """Device pointer of a float64 table (None -> NULL)."""
    if t is None:
        return 0
    if t.dtype != torch.float64:
        raise TypeError(f"HipBackend: float64 tensor required, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError("HipBackend: contiguous tensor required")
    return t.data_ptr()


def _parr(tensors):
    """Host array of device pointers (None -> NULL) for the batched entry points."""
    arr = (ctypes.c_void_p * len(tensors))()
    for i, t in enumerate(tensors):
        arr[i] = None if t is None else _p(t)
    return arr


class Consts:
    """Per-row Montgomery constants of a contiguous run of limbs on one device."""
    __slots__ = ("ql", "qh", "kl", "kh", "_2q", "q_host", "_mont", "_qptr")

    def __init__(self, ql, qh, kl, kh, _2q, q_host=None):
        self.ql, self.qh, self.kl, self.kh, self._2q = ql, qh, kl, kh, _2q
        self.q_host = q_host   # numpy int64 copy of the primes (launch-time row classification)
        # the vectors live as long as the object: validated and resolved once, not on every launch
        self._mont = (_p(ql), _p(qh), _p(kl), _p(kh))
        self._qptr = 0 if q_host is None else q_host.ctypes.data

    def qptr(self, relaxed=False):
        if relaxed and not self._qptr:
            raise ValueError("relaxed transforms need the host primes (Consts(q_host=...)): the auxiliary twiddle rows "
                             "are laid out by the size of the prime")
        return self._qptr

    def mont(self):
        return self._mont


class HipBackend:
    name = "hip-gfx950"
    ops = ntt_cuda  # the 15 reference-shaped primitives
    # capacities compiled into the fused kernels (include/ckks_hip.h: lf_limits)
    limits = {"digit_limbs": int(lib.lf_limits(0)), "special_primes": int(lib.lf_limits(1)), "rows": int(lib.lf_limits(2)),
              "batch": int(lib.lf_limits(3)), "logN": int(lib.lf_limits(4))}
    # include/ckks_hip.h: LF_BSGS_MAX_BABY_KEYS (tests/test_linear_transform_bsgs_cpu.py holds this copy to the header and to what
    # lf_linear_transform_bsgs_ws_words accepts)
    bsgs_max_baby_keys = 63

    def warm_twiddles(self, table, c: "Consts"):
        """Build the fp64 twin of a twiddle table on the current stream (otherwise built by its first user)."""
        dev, st = _ds(table)
        twiddles.dp_pointer(table, c.ql, c.qh, c.kl, c.kh, dev, st)

    # ---- NTT family over [batch][rows][N] stacks ------------------------------------------------
    def ntt(self, buf, batch, rows, logN, psi, Rs, c: Consts, relaxed=False, plain=False):
        """relaxed: the caller only needs residues mod q (internal transforms whose consumers reduce).
        plain (with relaxed): fp64-class limbs stay in the plain domain (see LF_NTT_PLAIN)."""
        dev, st = _ds(buf)
        dp = twiddles.dp_pointer(psi, c.ql, c.qh, c.kl, c.kh, dev, st)
        check(lib.lf_ntt(_p(buf), batch, rows, logN, _p(psi), dp, c.qptr(relaxed), _p(Rs), (1 if relaxed else 0) | (2 if relaxed and plain else 0), _p(c._2q),
                         *c.mont(), dev, st), "lf_ntt")

    def rescale_ntt(self, srcs, row0s, buf, rows, logN, scales, round_at, psi, Rs, c: Consts, relaxed=False, plain=False):
        """Rescale len(srcs) polynomials into buf[i] and transform them (cc_mult's opening) in one call."""
        dev, st = _ds(buf)
        dp = twiddles.dp_pointer(psi, c.ql, c.qh, c.kl, c.kh, dev, st)
        check(lib.lf_rescale_ntt(_parr(srcs), _parr(row0s), len(srcs), _p(buf), rows, logN, _p(scales), round_at, _p(psi), dp,
                                 c.qptr(relaxed), _p(Rs), (1 if relaxed else 0) | (2 if relaxed and plain else 0), _p(c._2q),
                                 *c.mont(), dev, st), "lf_rescale_ntt")

    def intt(self, buf, batch, rows, logN, ipsi, Ninv, tail, c: Consts, relaxed=False, plain=False):
        dev, st = _ds(buf)
        dp = twiddles.dp_pointer(ipsi, c.ql, c.qh, c.kl, c.kh, dev, st)
        check(lib.lf_intt(_p(buf), batch, rows, logN, _p(ipsi), dp, c.qptr(relaxed and tail >= 2), _p(Ninv), tail,
                          (3 if plain else 1) if relaxed and tail >= 2 else 0, _p(c._2q), *c.mont(), dev, st), "lf_intt")

    def intt_mul(self, dst, a, b, batch, rows, logN, ipsi, Ninv, c: Consts, a_stride=None, b_stride=None, plain=True):
        """dst[p] = intt(a[p] * b[p]) to canonical coefficients (relaxed, tail 2): the product is formed as the first pass
        loads its tiles.  a, b: first polynomial of each factor; *_stride = words between a factor's polynomials."""
        dev, st = _ds(dst)
        N = dst.size(-1)
        dp = twiddles.dp_pointer(ipsi, c.ql, c.qh, c.kl, c.kh, dev, st)
        check(lib.lf_intt_mul(_p(dst), _p(a), rows * N if a_stride is None else a_stride, _p(b),
                              rows * N if b_stride is None else b_stride, batch, rows, logN, _p(ipsi), dp, c.qptr(True), _p(Ninv), 2,
                              3 if plain else 1, *c.mont(), dev, st), "lf_intt_mul")

    def galois(self, a, dst, rows, logN, p, _2q):
        dev, st = _ds(a)
        check(lib.lf_galois(_p(a), _p(dst), rows, logN, p, _p(_2q), dev, st), "lf_galois")

    def galois_batch(self, srcs, dsts, rows, logN, p, _2q):
        """Several polynomials (the components of a ciphertext) through the same permutation in one launch."""
        dev, st = _ds(dsts[0])
        check(lib.lf_galois_batch(_parr(srcs), _parr(dsts), len(srcs), rows, logN, p, _p(_2q), dev, st), "lf_galois_batch")

    def gather_rows(self, rows, dst):
        """len(rows) <= 8 row tensors [N] -> the consecutive rows of dst [len(rows), N]: one launch."""
        dev, st = _ds(dst)
        check(lib.lf_gather_rows(_parr(rows), _p(dst), len(rows), dst.size(-1), dev, st), "lf_gather_rows")

    # ---- fused engine ops ------------------------------------------------------------------------
    def rescale_batch(self, srcs, row0s, outs, rows, scales, round_at, c: Consts):
        dev, st = _ds(outs[0])
        check(lib.lf_rescale_batch(_parr(srcs), _parr(row0s), _parr(outs), len(srcs), rows, outs[0].size(-1), _p(scales),
                                   round_at, *c.mont(), dev, st), "lf_rescale_batch")

    def ks_moddown_batch(self, ss, outs, addends, ell, K, PiR, Rs, c: Consts, PiP=None, galois=None):
        """galois = (p^-1 mod 2N, _2q or None): the addends are added as addend(X^p), read in gather form."""
        dev, st = _ds(outs[0])
        pinv, g2q = (0, None) if galois is None else galois
        check(lib.lf_ks_moddown_batch(_parr(ss), _parr(outs), _parr(addends), len(ss), ell, K, outs[0].size(-1), _p(PiR),
                                      _pd(PiP), _p(Rs), pinv, _p(g2q), *c.mont(), dev, st),
              "lf_ks_moddown_batch")

    def ks_moddown_ws(self, ss, outs, addends, ell, K, ws, PiR, Rs, c: Consts, PiP=None, galois=None, one_launch=False):
        """ks_moddown_batch with a workspace tensor `ws` (int64, >= moddown_ws_words(..) words): the special-prime
        chain is evaluated once per coefficient by a first launch — or, one_launch (K <= moddown_one_max_K, constants
        already in `ws` through moddown_consts): inside the single mod-down launch."""
        dev, st = _ds(outs[0])
        pinv, g2q = (0, None) if galois is None else galois
        fn, what = (lib.lf_ks_moddown_one, "lf_ks_moddown_one") if one_launch else (lib.lf_ks_moddown_ws, "lf_ks_moddown_ws")
        check(fn(_parr(ss), _parr(outs), _parr(addends), len(ss), ell, K, outs[0].size(-1), _p(ws), ws.numel(), _p(PiR), _pd(PiP),
                 _p(Rs), pinv, _p(g2q), *c.mont(), dev, st), what)

    moddown_one_max_K = 2    # LF_MODDOWN_ONE_MAX_K: up to here the mod-down is ONE launch (pivots eliminated inside it)

    def moddown_consts(self, ws, count, ell, K, N, PiP, c: Consts):
        """Write the level constants of the mod-down's fp64 rows into workspace `ws`, ONCE per workspace (needed by
        ks_moddown_ws(.., one_launch=True); the two-launch form rewrites them on every call)."""
        dev, st = _ds(ws)
        check(lib.lf_ks_moddown_consts(_p(ws), ws.numel(), count, ell, K, N, _pd(PiP), *c.mont(), dev, st), "lf_ks_moddown_consts")

    @staticmethod
    def moddown_ws_words(count, ell, K, N):
        return int(lib.lf_ks_moddown_ws_words(count, ell, K, N))

    def rescale(self, src, row0, out, rows, scales, round_at, c: Consts):
        dev, st = _ds(out)
        check(lib.lf_rescale(_p(src), _p(row0), _p(out), rows, out.size(-1), _p(scales), round_at, *c.mont(), dev, st),
              "lf_rescale")

    def tensor(self, x0, x1, y0, y1, d0, d1, d2, rows, c: Consts, plain=False):
        dev, st = _ds(d0)
        check(lib.lf_tensor(_p(x0), _p(x1), _p(y0), _p(y1), _p(d0), _p(d1), _p(d2), rows, d0.size(-1), 1 if plain else 0,
                            *c.mont(), dev, st),
              "lf_tensor")

    def ks_digits(self, a, state, nparts, desc, tab, c: Consts, galois=None):
        """galois = (p^-1 mod 2N, _2q or None): the digits of a(X^p), read in gather form (no permutation pass)."""
        dev, st = _ds(a)
        if galois is None:
            check(lib.lf_ks_digits(_p(a), _p(state), nparts, _p(desc), _p(tab), a.size(-1), *c.mont(), dev, st), "lf_ks_digits")
        else:
            check(lib.lf_ks_digits_galois(_p(a), _p(state), nparts, _p(desc), _p(tab), a.size(-1), galois[0], _p(galois[1]),
                                          *c.mont(), dev, st), "lf_ks_digits_galois")

    def ks_digits_batch(self, srcs, states, nparts, desc, tab, c: Consts, galois=None):
        """ks_digits of len(srcs) (<= 8) polynomials in one launch."""
        dev, st = _ds(srcs[0])
        pinv, g2q = (0, None) if galois is None else galois
        check(lib.lf_ks_digits_batch(_parr(srcs), _parr(states), len(srcs), nparts, _p(desc), _p(tab), srcs[0].size(-1), pinv,
                                     _p(g2q), *c.mont(), dev, st), "lf_ks_digits_batch")

    def ks_extend(self, state, ext, nparts, rows, desc, E, c: Consts):
        dev, st = _ds(ext)
        check(lib.lf_ks_extend(_p(state), _p(ext), nparts, rows, ext.size(-1), _p(desc), _p(E), *c.mont(), dev, st),
              "lf_ks_extend")

    def ks_inner(self, ext, key, first_part, row_off, s0, s1, nparts, rows, c: Consts):
        """key: packed [parts, 2, rows0, N] tensor of this device."""
        dev, st = _ds(ext)
        N = ext.size(-1)
        part_stride, comp_stride = key.stride(0), key.stride(1)
        base = key.data_ptr() + first_part * part_stride * 8
        check(lib.lf_ks_inner(_p(ext), base, part_stride, comp_stride, row_off, _p(s0), _p(s1), nparts, rows, N,
                              *c.mont(), dev, st), "lf_ks_inner")

    @staticmethod
    def _kfmt(key):
        """Format of a packed key tensor (LF_KEY_RAW unless key_planes() made it)."""
        return getattr(key, "lf_key_format", 0)

    def key_planes(self, src_b, src_a, dst_b, dst_a, c: Consts):
        """The two [rows, N] components of one key part (any lazy words) -> the planes format the fused key-switch entries
        read with key_format = LF_KEY_PLANES (include/ckks_hip.h): fp64-class rows as interleaved 32-bit + 16-bit planes of
        the canonical residues of both components, integer-class rows raw."""
        dev, st = _ds(dst_b)
        check(lib.lf_key_planes(_p(src_b), _p(src_a), _p(dst_b), _p(dst_a), src_b.size(0), src_b.size(1), _p(c.ql), _p(c.qh), dev, st),
              "lf_key_planes")

    @staticmethod
    def mark_planes(t):
        t.lf_key_format = LF_KEY_PLANES
        return t

    fused_ks_min_logN = 13   # lf_ks_core needs a two-pass ring degree
    relin_fold = True        # cc_mult's d0 / d1 folded into the key-switch sums (lf_intt_mul, lf_relin_*)

    def ks_core(self, state, nparts, rows, logN, desc, E, Ed, key, first_part, row_off, tmp, s, psi, ipsi, Ninv,
                c: Consts, fold=None):
        """extend + NTT + key inner product + inverse NTT in three fused launches per arithmetic class.
        fold = (x stack [4, ell, N], PR [ell], own [rows] uint8 or None): cc_mult's d0 / d1 enter the sums in the NTT domain and
        the digits' own limbs come from x1 * y1 instead of an extension (lf_relin_core_batch)."""
        dev, st = _ds(s)
        part_stride, comp_stride = key.stride(0), key.stride(1)
        base = key.data_ptr() + first_part * part_stride * 8
        psi_dp = twiddles.dp_pointer(psi, c.ql, c.qh, c.kl, c.kh, dev, st)
        ipsi_dp = twiddles.dp_pointer(ipsi, c.ql, c.qh, c.kl, c.kh, dev, st)
        if fold is not None:
            x, PR, own = fold
            check(lib.lf_relin_core_batch(_p(state), 0, 1, nparts, rows, logN, _p(desc), _p(E), _pd(Ed), base, part_stride,
                                          comp_stride, row_off, self._kfmt(key), _p(tmp), _p(s), _p(psi), psi_dp, _p(ipsi), ipsi_dp, _p(Ninv),
                                          _p(x), 0, _p(PR), x.size(1), _pb(own), c.qptr(), *c.mont(), dev, st),
                  "lf_relin_core_batch")
            return
        check(lib.lf_ks_core(_p(state), nparts, rows, logN, _p(desc), _p(E), _pd(Ed), base, part_stride, comp_stride,
                             row_off, self._kfmt(key), _p(tmp), _p(s), _p(psi), psi_dp, _p(ipsi), ipsi_dp, _p(Ninv),
                             c.qptr(), *c.mont(), dev, st), "lf_ks_core")

    def ks_fwd(self, state, first, count, rows, logN, desc, E, Ed, tmp, psi, c: Consts, own=None):
        """Extension + forward NTT of digits first .. first + count - 1 into tmp[first:first + count] (lf_ks_fwd; with
        `own`, lf_relin_fwd: the digits' own limbs are left out, see ks_core's fold)."""
        dev, st = _ds(tmp)
        psi_dp = twiddles.dp_pointer(psi, c.ql, c.qh, c.kl, c.kh, dev, st)
        N = tmp.size(-1)
        if own is not None:
            check(lib.lf_relin_fwd(_p(state), first, count, rows, logN, _p(desc), _p(E), _pd(Ed), _p(tmp), _p(psi), psi_dp,
                                   _pb(own), c.qptr(), *c.mont(), dev, st), "lf_relin_fwd")
            return
        check(lib.lf_ks_fwd(_p(state), count, rows, logN, _p(desc) + first * 3 * 8, _p(E), _pd(Ed),
                            _p(tmp) + first * rows * N * 8, _p(psi), psi_dp, c.qptr(), *c.mont(), dev, st), "lf_ks_fwd")

    def ks_tail(self, nparts, rows, logN, key, first_part, row_off, tmp, s, ipsi, Ninv, c: Consts, fold=None):
        """Inner product of all extended digits with the key + inverse NTT (lf_ks_tail; fold: lf_relin_tail, see ks_core)."""
        dev, st = _ds(s)
        part_stride, comp_stride = key.stride(0), key.stride(1)
        base = key.data_ptr() + first_part * part_stride * 8
        ipsi_dp = twiddles.dp_pointer(ipsi, c.ql, c.qh, c.kl, c.kh, dev, st)
        if fold is not None:
            x, PR, own = fold
            check(lib.lf_relin_tail(nparts, rows, logN, base, part_stride, comp_stride, row_off, self._kfmt(key), _p(tmp), _p(s), _p(ipsi), ipsi_dp,
                                    _p(Ninv), _p(x), _p(PR), x.size(1), _pb(own), c.qptr(), *c.mont(), dev, st), "lf_relin_tail")
            return
        check(lib.lf_ks_tail(nparts, rows, logN, base, part_stride, comp_stride, row_off, self._kfmt(key), _p(tmp), _p(s), _p(ipsi), ipsi_dp,
                             _p(Ninv), c.qptr(), *c.mont(), dev, st), "lf_ks_tail")

    # ---- whole ops behind one native call (lf_cc_mult_evk / lf_switch_key over an lf_ks_plan) ------------------------
    native_ops = True

    def make_plan(self, ints, tensors, q_host, psi, ipsi, c: Consts):
        """lf_ks_plan from the engine's per-level pieces.  ints: {field: int}; tensors: {field: tensor or None} (int64 /
        float64 / uint8 device tensors); q_host: numpy int64; psi / ipsi: the twiddle views (their auxiliary tables are
        built here, on the current stream).  Returns (plan, keep-alive list)."""
        plan = KsPlan()
        for k, v in ints.items():
            setattr(plan, k, int(v))
        keep = [q_host, psi, ipsi, c]
        for k, t in tensors.items():
            if t is None:
                setattr(plan, k, None)
                continue
            if not t.is_contiguous():
                raise ValueError(f"plan tensor {k} must be contiguous")
            setattr(plan, k, t.data_ptr())
            keep.append(t)
        dev, st = _ds(psi)
        plan.device = dev
        plan.ql, plan.qh, plan.kl, plan.kh = c.mont()
        plan._2q = _p(c._2q)
        plan.q_host = q_host.ctypes.data
        plan.psi, plan.ipsi = _p(psi), _p(ipsi)
        plan.psi_dp = twiddles.dp_pointer(psi, c.ql, c.qh, c.kl, c.kh, dev, st)
        plan.ipsi_dp = twiddles.dp_pointer(ipsi, c.ql, c.qh, c.kl, c.kh, dev, st)
        # the plan outlives this call (the engine caches it per level): it holds the auxiliary twins its two raw
        # addresses point into, so a rebuilt twin (new table version) can never leave the plan reading freed memory
        keep += [twiddles.twin_of(psi), twiddles.twin_of(ipsi)]
        if plan.K <= self.moddown_one_max_K:   # the ops then run the one-launch mod-down: its level constants, once
            check(lib.lf_ks_moddown_consts(plan.md_ws, plan.md_ws_words, 2 * plan.max_nct, plan.ell, plan.K, 1 << plan.logN, plan.PiP,
                                           *c.mont(), dev, st), "lf_ks_moddown_consts")
            plan.md_consts = 2 * plan.max_nct   # the op entries take the one-launch form for exactly this count
        return plan, keep

    @staticmethod
    def _key_args(key, first_part):
        part_stride, comp_stride = key.stride(0), key.stride(1)
        return key.data_ptr() + first_part * part_stride * 8, part_stride, comp_stride

    def switch_key_batch_native(self, plan, c0s, c1s, pinv, canonical, key, first_part, row_off, out):
        """len(c1s) in (1, 2, 4) == plan.max_nct ciphertexts under one key as ONE native call; out [nct, 2, ell, N]."""
        dev, st = _ds(out)
        base, ps, cs = self._key_args(key, first_part)
        nct = len(c1s)
        check(lib.lf_switch_key_batch(ctypes.byref(plan), nct, _parr(c0s), _parr(c1s), pinv, 1 if canonical else 0, base, ps, cs, row_off,
                                      self._kfmt(key), _parr([out[t][0] for t in range(nct)]), _parr([out[t][1] for t in range(nct)]), st),
              "lf_switch_key_batch")

    def cc_mult_evk_batch_native(self, plan, ins, row0s, key, first_part, row_off, out):
        """ins / row0s: 4 device tensors (or raw pointers) per ciphertext pair; out [nct, 2, ell, N]."""
        dev, st = _ds(out)
        base, ps, cs = self._key_args(key, first_part)
        nct = out.size(0)
        check(lib.lf_cc_mult_evk_batch(ctypes.byref(plan), nct, ins, row0s, base, ps, cs, row_off, self._kfmt(key),
                                       _parr([out[t][0] for t in range(nct)]), _parr([out[t][1] for t in range(nct)]), st),
              "lf_cc_mult_evk_batch")

    # ---- the halves of an op around the digit exchange (one process per GPU) -----------------------------------------
    @staticmethod
    def format_knobs():
        """(LF_TUNE_DIGIT_PLANES, LF_TUNE_MORE_PLANES) as they stand: the knobs that decide the FORMAT of the scratch between
        the halves of an op.  Whatever bakes launches of the halves (a captured graph) is only valid under the pair it was
        made under; two reads of process-wide integers, no launch."""
        return lib.lf_tune(3, -1), lib.lf_tune(5, -1)

    def cc_mult_pre(self, plan, ins, row0s, st, which=3):
        """which: 1 = the launch that reads the operands, 2 = the rest of the half (plan addresses only), 3 = both."""
        check(lib.lf_cc_mult_evk_pre(ctypes.byref(plan), ins, row0s, which, st), "lf_cc_mult_evk_pre")

    def switch_key_pre(self, plan, c1, pinv, canonical):
        dev, st = _ds(c1)
        check(lib.lf_switch_key_pre(ctypes.byref(plan), _p(c1), pinv, 1 if canonical else 0, st), "lf_switch_key_pre")

    def plan_fwd(self, plan, digits, first, count, relin):
        dev, st = _ds(digits)
        check(lib.lf_ks_plan_fwd(ctypes.byref(plan), _p(digits), first, count, 1 if relin else 0, st), "lf_ks_plan_fwd")

    def cc_mult_post(self, plan, key, first_part, row_off, out, which=3):
        """which: 1 = inner product + inverse NTT (plan addresses + the key), 2 = the mod-down into `out`, 3 = both
        (out may be None with which = 1)."""
        dev, st = _ds(key)
        base, ps, cs = self._key_args(key, first_part)
        o0 = out.data_ptr() if out is not None else None
        o1 = out.data_ptr() + out.stride(0) * 8 if out is not None else None
        check(lib.lf_cc_mult_evk_post(ctypes.byref(plan), base, ps, cs, row_off, self._kfmt(key), o0, o1, which, st), "lf_cc_mult_evk_post")

    def switch_key_post(self, plan, c0, pinv, canonical, key, first_part, row_off, out, which=3):
        dev, st = _ds(key)
        base, ps, cs = self._key_args(key, first_part)
        o0 = out.data_ptr() if out is not None else None
        o1 = out.data_ptr() + out.stride(0) * 8 if out is not None else None
        check(lib.lf_switch_key_post(ctypes.byref(plan), _p(c0) if c0 is not None else None, pinv, 1 if canonical else 0, base, ps, cs,
                                     row_off, self._kfmt(key), o0, o1, which, st), "lf_switch_key_post")

    def cc_mult_evk(self, plan, ins, row0s, key, first_part, row_off, out):
        """ins / row0s: ctypes arrays of 4 device pointers; out [2, ell, N]."""
        dev, st = _ds(out)
        part_stride, comp_stride = key.stride(0), key.stride(1)
        base = key.data_ptr() + first_part * part_stride * 8
        plane = out.stride(0) * 8
        check(lib.lf_cc_mult_evk(ctypes.byref(plan), ins, row0s, base, part_stride, comp_stride, row_off, self._kfmt(key), out.data_ptr(),
                                 out.data_ptr() + plane, st), "lf_cc_mult_evk")

    def switch_key_native(self, plan, c0, c1, pinv, canonical, key, first_part, row_off, out):
        dev, st = _ds(out)
        part_stride, comp_stride = key.stride(0), key.stride(1)
        base = key.data_ptr() + first_part * part_stride * 8
        plane = out.stride(0) * 8
        check(lib.lf_switch_key(ctypes.byref(plan), _p(c0), _p(c1), pinv, 1 if canonical else 0, base, part_stride, comp_stride,
                                row_off, self._kfmt(key), out.data_ptr(), out.data_ptr() + plane, st), "lf_switch_key")

    @staticmethod
    def cc_dot_ws_words(plan):
        return int(lib.lf_cc_dot_ws_words(ctypes.byref(plan)))

    def cc_dot_native(self, plan, ins, row0s, key, first_part, row_off, out, ws):
        """sum of len(ins) / 4 ciphertext products under one relinearisation as ONE native call (lf_cc_dot).  ins / row0s:
        ctypes arrays of 4 device pointers per pair, in cc_mult_evk's order; out [2, ell, N]; ws: at least
        cc_dot_ws_words(plan) words (the summed triplet)."""
        dev, st = _ds(out)
        base, ps, cs = self._key_args(key, first_part)
        check(lib.lf_cc_dot(ctypes.byref(plan), len(ins) // 4, ins, row0s, base, ps, cs, row_off, self._kfmt(key), _p(ws),
                            0 if ws is None else ws.numel(), out.data_ptr(), out.data_ptr() + out.stride(0) * 8, st), "lf_cc_dot")

    @staticmethod
    def cc_dot_batch_ws_words(plan, nd):
        return int(lib.lf_cc_dot_batch_ws_words(ctypes.byref(plan), nd))

    def cc_dot_batch_native(self, plan, np_list, ins, row0s, key, first_part, row_off, outs, ws):
        """len(np_list) in (1, 2, 4) <= plan.max_nct dots under one key as ONE native call (lf_cc_dot_batch).  np_list: the pair
        count of each dot; ins / row0s: ctypes arrays of 4 device pointers per pair, in cc_mult_evk's order, dot after dot;
        outs: one [2, ell, N] tensor per dot; ws: at least cc_dot_batch_ws_words(plan, len(np_list)) words (the summed triplets)."""
        dev, st = _ds(outs[0])
        base, ps, cs = self._key_args(key, first_part)
        nd = len(np_list)
        nps = (ctypes.c_int64 * nd)(*np_list)
        check(lib.lf_cc_dot_batch(ctypes.byref(plan), nd, nps, ins, row0s, base, ps, cs, row_off, self._kfmt(key), _p(ws),
                                  0 if ws is None else ws.numel(), _parr([o[0] for o in outs]), _parr([o[1] for o in outs]), st),
              "lf_cc_dot_batch")

    @staticmethod
    def cc_matmul_ws_words(plan, nu):
        return int(lib.lf_cc_matmul_ws_words(ctypes.byref(plan), nu))

    def cc_matmul_native(self, plan, m, k, n, ins, row0s, ia, ib, key, first_part, row_off, outs, ws):
        """An m x k matrix of ciphertexts times a k x n one under one key as ONE native call (lf_cc_matmul).  ins / row0s: ctypes
        arrays of 2 device pointers per DISTINCT operand ([operand][component]: first surviving row, dropped row); ia (m k entries,
        [i][t]) / ib (k n entries, [t][j]): the operand of every entry, -1 for a zero one; outs: m n tensors [2, ell, N], [i][j];
        ws: at least cc_matmul_ws_words(plan, len(ins) // 2) words (the transformed operands and a tile's summed triplets)."""
        dev, st = _ds(outs[0])
        base, ps, cs = self._key_args(key, first_part)
        check(lib.lf_cc_matmul(ctypes.byref(plan), m, k, n, len(ins) // 2, ins, row0s, (ctypes.c_int64 * len(ia))(*ia),
                               (ctypes.c_int64 * len(ib))(*ib), base, ps, cs, row_off, self._kfmt(key), _p(ws),
                               0 if ws is None else ws.numel(), _parr([o[0] for o in outs]), _parr([o[1] for o in outs]), st),
              "lf_cc_matmul")

    # include/ckks_hip.h: LF_WSUM_MAX_TERMS / LF_WSUM_MAX_OUTPUTS (tests/test_poly_eval_cpu.py holds these copies to the header)
    wsum_max_terms = 16
    wsum_max_outputs = 64

    def weighted_sums_native(self, ins, row0s, outs, k, G, rows, logN, tab, consts, scales, round_at, c: Consts):
        """G weighted sums of the same k ciphertexts under one rescale as ONE native call (lf_weighted_sums).  ins / row0s:
        ctypes arrays of 2 k device pointers ([term][component]: first surviving row, dropped row); outs: the 2 G output
        tensors [rows, N] ([output][component]); tab [G, k, rows + 1] and consts [G, rows] (or None) device tables; c: the
        constants of the level the operands are at (rows + 1 entries, the dropped limb first)."""
        dev, st = _ds(outs[0])
        check(lib.lf_weighted_sums(ins, row0s, _parr(outs), k, G, rows, logN, _p(tab), _p(consts), _p(scales), round_at, *c.mont(),
                                   dev, st), "lf_weighted_sums")

    # include/ckks_hip.h: LF_LSUM_MAX_TERMS / LF_LSUM_MAX_SETS (tests/test_level_sum_cpu.py holds these copies to the header)
    lsum_max_terms = 8
    lsum_max_sets = 8

    def level_sum_call(self, sets, outs, rows, logN, c: Consts):
        """len(sets) <= lsum_max_sets sums of ciphertexts brought to ONE level as ONE native call (lf_level_sum).  sets: one
        (terms, tab, const) per sum; terms: up to lsum_max_terms entries (c0, c1, skip, scales, round_at) — the term's two
        component tensors, the rows of them that do not survive at the target level (0: the term stands there) and, for
        skip >= 1, the rescale constants of the term's level (skip - 1 entries ahead of those of the target's rows) and its
        rounding threshold, None and 0 otherwise; tab [len(terms), rows] and const ([rows] or None) device tables.  outs: one pair
        of [rows, N] tensors per set; c: the constants of the target level (rows entries)."""
        dev, st = _ds(outs[0][0])
        N = outs[0][0].size(-1)
        n = sum(len(terms) for terms, _, _ in sets)
        ks = (ctypes.c_int64 * len(sets))(*[len(terms) for terms, _, _ in sets])
        ins, row0s = (ctypes.c_void_p * (2 * n))(), (ctypes.c_void_p * (2 * n))()
        scs, ras = (ctypes.c_void_p * n)(), (ctypes.c_int64 * n)()
        i = 0
        for terms, _, _ in sets:
            for c0, c1, skip, scales, round_at in terms:
                if (skip == 0) != (scales is None) or skip < 0 or c0.size(0) != rows + skip or c1.size(0) != rows + skip:
                    raise ValueError("HipBackend.level_sum_call: a term's rows, skipped rows and rescale constants disagree")
                for comp, t in enumerate((c0, c1)):
                    ptr = _p(t)
                    ins[2 * i + comp] = ptr + skip * N * 8
                    row0s[2 * i + comp] = ptr if skip else None     # the dropped limb is the tensor's first row
                if skip:
                    if scales.numel() != rows + skip - 1:
                        raise ValueError("HipBackend.level_sum_call: rescale constants of another level than the term's")
                    scs[i] = _p(scales) + (skip - 1) * 8
                ras[i] = round_at
                i += 1
        check(lib.lf_level_sum(len(sets), ks, ins, row0s, scs, ras, _parr([tab for _, tab, _ in sets]),
                               _parr([cst for _, _, cst in sets]), _parr([o for pair in outs for o in pair]), rows, logN, *c.mont(),
                               dev, st), "lf_level_sum")

    # include/ckks_hip.h: LF_MOD_RAISE_MAX_CTS (tests/test_mod_raise_cpu.py holds this copy to the header)
    mod_raise_max_cts = 64

    def mod_raise_call(self, base_rows, outs, rows, q_b, mont_one, c: Consts):
        """len(base_rows) <= mod_raise_max_cts ciphertexts raised from their base-prime rows to level 0 as ONE native call
        (lf_mod_raise).  base_rows: one pair of [N] views (the base row of c0, of c1) per ciphertext; outs: one pair of [rows, N]
        tensors per ciphertext; mont_one [rows] = R mod q and c: the constants of level 0 (rows entries)."""
        dev, st = _ds(outs[0][0])
        N = outs[0][0].size(-1)
        for pair in base_rows:
            for t in pair:
                if t.dim() != 1 or t.size(0) != N:
                    raise ValueError("HipBackend.mod_raise_call: a base row is one row of N words")
        for pair in outs:
            for t in pair:
                if tuple(t.shape) != (rows, N):
                    raise ValueError("HipBackend.mod_raise_call: an output is [rows, N]")
        if mont_one.numel() != rows:
            raise ValueError("HipBackend.mod_raise_call: constants of another level than the outputs'")
        check(lib.lf_mod_raise(len(base_rows), _parr([p[0] for p in base_rows]), _parr([p[1] for p in base_rows]),
                               _parr([o[0] for o in outs]), _parr([o[1] for o in outs]), rows, N, int(q_b), _p(mont_one), *c.mont(),
                               dev, st), "lf_mod_raise")

    @staticmethod
    def pc_dot_ws_words(k, rows, logN):
        return int(lib.lf_pc_dot_ws_words(k, rows, logN))

    def pc_dot_native(self, ins, pts, bias, outs, k, rows, logN, psi, ipsi, Rs, Ninv, mont_one, zero_row, scales, round_at, ws, c: Consts):
        """sum of k plaintext-ciphertext products (+ bias) under one rescale as ONE native call (lf_pc_dot).  ins: ctypes array of
        2 k device pointers ([term][component], [rows, N] each, the dropped limb first); pts: ctypes array of k device pointers
        (encode_plain's "mult" tensors); bias: the "add" tensor [rows - 1, N] or None; outs: the two output tensors [rows - 1, N];
        psi .. Ninv, c: tables and constants of the level the operands are at; mont_one [rows] = R mod q, zero_row [N] zeros;
        ws: at least pc_dot_ws_words(k, rows, logN) words."""
        dev, st = _ds(outs[0])
        psi_dp = twiddles.dp_pointer(psi, c.ql, c.qh, c.kl, c.kh, dev, st)
        ipsi_dp = twiddles.dp_pointer(ipsi, c.ql, c.qh, c.kl, c.kh, dev, st)
        check(lib.lf_pc_dot(k, ins, pts, _p(bias), _p(outs[0]), _p(outs[1]), rows, logN, _p(psi), psi_dp, _p(ipsi), ipsi_dp, c.qptr(True),
                            _p(Rs), _p(Ninv), _p(mont_one), _p(zero_row), _p(scales), round_at, _p(ws), ws.numel(), *c.mont(), dev, st),
              "lf_pc_dot")

    @staticmethod
    def _pc_matmul_entry(name, shape, ins, pts, biases, pairs, rows, logN, psi, ipsi, Rs, Ninv, mont_one, zero_row, scales, round_at, ws,
                         c: Consts):
        """lf_pc_matmul, lf_pc_matmul_batch or lf_pc_matmul_batch_planes (`name`): shape = its leading (nt,) k_in, k_out; pairs: the
        output pairs in the entry's order, [token][output]."""
        dev, st = _ds(pairs[0][0])
        psi_dp = twiddles.dp_pointer(psi, c.ql, c.qh, c.kl, c.kh, dev, st)
        ipsi_dp = twiddles.dp_pointer(ipsi, c.ql, c.qh, c.kl, c.kh, dev, st)
        out0, out1 = _parr([o[0] for o in pairs]), _parr([o[1] for o in pairs])
        check(getattr(lib, name)(*shape, ins, pts, biases, out0, out1, rows, logN, _p(psi), psi_dp, _p(ipsi), ipsi_dp, c.qptr(True), _p(Rs),
                                 _p(Ninv), _p(mont_one), _p(zero_row), _p(scales), round_at, _p(ws), ws.numel(), *c.mont(), dev, st), name)

    # include/ckks_hip.h: LF_PC_MATMUL_CI / LF_PC_MATMUL_MAX_OUTPUTS (tests/test_pc_matmul_cpu.py holds these copies to the header)
    pc_matmul_chunk = 16
    pc_matmul_max_outputs = 64

    @staticmethod
    def pc_matmul_ws_words(k_in, k_out, rows, logN):
        return int(lib.lf_pc_matmul_ws_words(k_in, k_out, rows, logN))

    def pc_matmul_native(self, ins, pts, biases, outs, k_in, k_out, rows, logN, psi, ipsi, Rs, Ninv, mont_one, zero_row, scales, round_at,
                         ws, c: Consts):
        """k_out sums of plaintext-ciphertext products over the same k_in ciphertexts (+ biases) as ONE native call (lf_pc_matmul).
        ins: ctypes array of 2 k_in device pointers ([input][component]); pts: ctypes array of k_out k_in device pointers, row-major,
        None for an absent term; biases: None or a ctypes array of k_out pointers (None: no bias); outs: k_out pairs of output
        tensors [rows - 1, N]; the rest as pc_dot_native; ws: at least pc_matmul_ws_words(k_in, k_out, rows, logN) words."""
        self._pc_matmul_entry("lf_pc_matmul", (k_in, k_out), ins, pts, biases, outs, rows, logN, psi, ipsi, Rs, Ninv, mont_one, zero_row,
                              scales, round_at, ws, c)

    # include/ckks_hip.h: LF_PC_MATMUL_BATCH_MAX_TOKENS (tests/test_pc_matmul_batch_cpu.py holds this copy to the header); the
    # group sizes lf_pc_matmul_batch has a tile of tokens for, largest first
    pc_matmul_batch_max_tokens = 4
    pc_matmul_batch_sizes = (4, 2)

    @staticmethod
    def pc_matmul_batch_ws_words(nt, k_in, k_out, rows, logN):
        return int(lib.lf_pc_matmul_batch_ws_words(nt, k_in, k_out, rows, logN))

    def pc_matmul_batch_native(self, ins, pts, biases, outs, nt, k_in, k_out, rows, logN, psi, ipsi, Rs, Ninv, mont_one, zero_row, scales,
                               round_at, ws, c: Consts):
        """pc_matmul_native over nt token vectors that share the matrix as ONE native call (lf_pc_matmul_batch).  ins: ctypes array
        of nt 2 k_in device pointers ([token][input][component]); pts, biases: as pc_matmul_native, shared by the tokens; outs: nt
        lists of k_out pairs of output tensors [rows - 1, N]; ws: at least pc_matmul_batch_ws_words(nt, k_in, k_out, rows, logN) words."""
        self._pc_matmul_entry("lf_pc_matmul_batch", (nt, k_in, k_out), ins, pts, biases, [o for tok in outs for o in tok], rows, logN, psi,
                              ipsi, Rs, Ninv, mont_one, zero_row, scales, round_at, ws, c)

    # include/ckks_hip.h: LF_PLAIN_PLANES_MAX_ROWS (tests/test_compact_plain_cpu.py holds this copy to the header)
    plain_planes_max_rows = LF_PLAIN_PLANES_MAX_ROWS

    @staticmethod
    def plain_planes_words(rows, N, c: Consts):
        """8-byte words of the compact form of a [rows, N] "mult" plaintext (lf_plain_planes_words; 0: a size the format refuses)."""
        return int(lib.lf_plain_planes_words(rows, N, c.qptr(True)))

    def plain_planes(self, src, dst, c: Consts):
        """src [rows, N] (a "mult" plaintext's tensor: Montgomery form, lazy words) -> dst, flat, plain_planes_words words: fp64-class
        rows as 6-byte planes of the plain word, integer-class rows as they are (lf_plain_planes, one launch)."""
        dev, st = _ds(dst)
        check(lib.lf_plain_planes(_p(src), _p(dst), src.size(0), src.size(1), c.qptr(True), *c.mont(), dev, st), "lf_plain_planes")

    def plain_unplanes(self, src, dst, c: Consts):
        """The inverse: dst [rows, N] <- the canonical Montgomery residue of every word of the compact src (lf_plain_unplanes)."""
        dev, st = _ds(dst)
        check(lib.lf_plain_unplanes(_p(src), _p(dst), dst.size(0), dst.size(1), c.qptr(True), *c.mont(), dev, st), "lf_plain_unplanes")

    @staticmethod
    def pc_matmul_batch_planes_ws_words(nt, k_in, k_out, rows, logN):
        return int(lib.lf_pc_matmul_batch_planes_ws_words(nt, k_in, k_out, rows, logN))

    def pc_matmul_batch_planes_call(self, ins, pts, biases, outs, nt, k_in, k_out, rows, logN, psi, ipsi, Rs, Ninv, mont_one, zero_row,
                                    scales, round_at, ws, c: Consts):
        """pc_matmul_batch_native with every plaintext of pts a compact one (plain_planes) as ONE native call
        (lf_pc_matmul_batch_planes); nt = 1 is pc_matmul, nt = 1 and k_out = 1 pc_dot.  ws: at least
        pc_matmul_batch_planes_ws_words(nt, k_in, k_out, rows, logN) words."""
        self._pc_matmul_entry("lf_pc_matmul_batch_planes", (nt, k_in, k_out), ins, pts, biases, [o for tok in outs for o in tok], rows, logN,
                              psi, ipsi, Rs, Ninv, mont_one, zero_row, scales, round_at, ws, c)

    @staticmethod
    def rotate_hoisted_ws_words(plan):
        return int(lib.lf_rotate_hoisted_ws_words(ctypes.byref(plan)))

    def rotate_hoisted_native(self, plan, c0, c1, exponents, keys, first_part, row_off, out, ws=None):
        """One ciphertext under len(keys) rotation keys as ONE native call (lf_rotate_hoisted): the digits of c1 are extended and
        transformed once, rotation i gathers them by pi_{exponents[i]}.  keys: packed key tensors of one format and shape;
        out [n, 2, ell, N]; ws: >= rotate_hoisted_ws_words(plan) words (None when that is 0)."""
        dev, st = _ds(out)
        n = len(keys)
        bases = (ctypes.c_void_p * n)()
        for i, key in enumerate(keys):
            bases[i], ps, cs = self._key_args(key, first_part)
        fmt = {self._kfmt(k) for k in keys}
        if len(fmt) != 1:
            raise ValueError("rotate_hoisted_native: the keys of one call must share one format")
        exps = (ctypes.c_int64 * n)(*exponents)
        check(lib.lf_rotate_hoisted(ctypes.byref(plan), _p(c0), _p(c1), n, exps, 1, bases, ps, cs, row_off, fmt.pop(),
                                    _p(ws), 0 if ws is None else ws.numel(), _parr([out[i][0] for i in range(n)]),
                                    _parr([out[i][1] for i in range(n)]), st), "lf_rotate_hoisted")

    @staticmethod
    def linear_transform_ws_words(plan):
        return int(lib.lf_linear_transform_ws_words(ctypes.byref(plan)))

    def linear_transform_native(self, plan, c0, c1, exponents, keys, first_part, row_off, pt, pt0, scales, round_at, out, ws=None):
        """sum_i pt[i] * rot_i(c0, c1) (+ pt0 * (c0, c1)), mod-down and rescale as ONE native call (lf_linear_transform).
        keys: packed key tensors of one format and shape, exponents their Galois exponents; pt [len(keys), rows, N] the encoded
        diagonals in key order (None without keys), pt0 [rows, N] the step-0 diagonal or None; scales / round_at: the rescale
        constants of the level the ciphertext leaves; out [2, ell - 1, N]."""
        dev, st = _ds(out)
        n = len(keys)
        bases = (ctypes.c_void_p * max(n, 1))()
        ps = cs = 0
        for i, key in enumerate(keys):
            bases[i], ps, cs = self._key_args(key, first_part)
        fmt = {self._kfmt(k) for k in keys}
        if len(fmt) > 1:
            raise ValueError("linear_transform_native: the keys of one call must share one format")
        exps = (ctypes.c_int64 * max(n, 1))(*exponents)
        check(lib.lf_linear_transform(ctypes.byref(plan), _p(c0), _p(c1), n, exps, bases, ps, cs, row_off, fmt.pop() if fmt else 0,
                                      _p(pt), 0 if pt is None else pt.stride(0), _p(pt0), _p(scales), round_at, _p(ws),
                                      0 if ws is None else ws.numel(), out.data_ptr(), out.data_ptr() + out.stride(0) * 8, st),
              "lf_linear_transform")

    # csrc/ckks_ks.hip: LF_LTB_KEYS, the keys one launch of ks_inner_ltb_kernel loops over (tests/test_linear_transform_batch_cpu.py
    # holds this copy to the source); include/ckks_hip.h: LF_LT_BATCH_MAX_CTS through _native.py's copy
    lt_batch_keys_per_launch = 8
    lt_batch_max_cts = LF_LT_BATCH_MAX_CTS

    @staticmethod
    def linear_transform_batch_ws_words(plan, nct):
        return int(lib.lf_linear_transform_batch_ws_words(ctypes.byref(plan), nct))

    def linear_transform_batch_native(self, plan, c0s, c1s, exponents, keys, first_part, row_off, pt, pt0, scales, round_at, outs, ws=None):
        """linear_transform_native for len(c0s) <= lt_batch_max_cts ciphertexts under the same diagonals and keys as ONE native call
        (lf_linear_transform_batch): groups of 4, 2 or 1 ciphertexts (plan.max_nct permitting) share every launch, and the inner
        product reads each key and diagonal word once per group.  c0s / c1s: the components, one tensor each per ciphertext;
        outs: one [2, ell - 1, N] tensor per ciphertext; ws: >= linear_transform_batch_ws_words(plan, len(c0s)) words (None
        when that is 0); the rest as linear_transform_native."""
        dev, st = _ds(outs[0])
        n = len(keys)
        bases = (ctypes.c_void_p * max(n, 1))()
        ps = cs = 0
        for i, key in enumerate(keys):
            bases[i], ps, cs = self._key_args(key, first_part)
        fmt = {self._kfmt(k) for k in keys}
        if len(fmt) > 1:
            raise ValueError("linear_transform_batch_native: the keys of one call must share one format")
        exps = (ctypes.c_int64 * max(n, 1))(*exponents)
        check(lib.lf_linear_transform_batch(ctypes.byref(plan), len(c0s), _parr(c0s), _parr(c1s), n, exps, bases, ps, cs, row_off,
                                            fmt.pop() if fmt else 0, _p(pt), 0 if pt is None else pt.stride(0), _p(pt0), _p(scales),
                                            round_at, _p(ws), 0 if ws is None else ws.numel(), _parr([o[0] for o in outs]),
                                            _parr([o[1] for o in outs]), st), "lf_linear_transform_batch")

    @staticmethod
    def rotate_sum_ws_words(plan):
        return int(lib.lf_rotate_sum_ws_words(ctypes.byref(plan)))

    def rotate_sum_native(self, plan, c0, c1, exponents, keys, first_part, row_off, with_self, out, ws=None):
        """sum_i rot_i(c0, c1) (+ (c0, c1) with with_self) and ONE mod-down as ONE native call (lf_rotate_sum): no rescale, the
        level stays.  keys: packed key tensors of one format and shape, exponents their Galois exponents; out [2, ell, N]."""
        dev, st = _ds(out)
        n = len(keys)
        bases = (ctypes.c_void_p * max(n, 1))()
        ps = cs = 0
        for i, key in enumerate(keys):
            bases[i], ps, cs = self._key_args(key, first_part)
        fmt = {self._kfmt(k) for k in keys}
        if len(fmt) > 1:
            raise ValueError("rotate_sum_native: the keys of one call must share one format")
        exps = (ctypes.c_int64 * max(n, 1))(*exponents)
        check(lib.lf_rotate_sum(ctypes.byref(plan), _p(c0), _p(c1), n, exps, bases, ps, cs, row_off, fmt.pop() if fmt else 0,
                                1 if with_self else 0, _p(ws), 0 if ws is None else ws.numel(), out.data_ptr(),
                                out.data_ptr() + out.stride(0) * 8, st), "lf_rotate_sum")

    # csrc/ckks_ks.hip: LF_RSB_KEYS, the keys one launch of ks_inner_rsumb_kernel loops over (tests/test_rotate_sum_batch_cpu.py
    # holds this copy to the source)
    rsum_batch_keys_per_launch = 8

    @staticmethod
    def rotate_sum_batch_ws_words(plan, nct):
        return int(lib.lf_rotate_sum_batch_ws_words(ctypes.byref(plan), nct))

    def rotate_sum_batch_native(self, plan, c0s, c1s, exponents, keys, first_part, row_off, with_self, outs, ws=None):
        """rotate_sum_native for len(c0s) <= lt_batch_max_cts ciphertexts under the same keys as ONE native call
        (lf_rotate_sum_batch): groups of 4, 2 or 1 ciphertexts (plan.max_nct permitting) share every launch, and the inner product
        reads each key word once per group.  c0s / c1s: the components, one tensor each per ciphertext; outs: one [2, ell, N]
        tensor per ciphertext; ws: >= rotate_sum_batch_ws_words(plan, len(c0s)) words (None when that is 0); the rest as
        rotate_sum_native."""
        dev, st = _ds(outs[0])
        n = len(keys)
        bases = (ctypes.c_void_p * max(n, 1))()
        ps = cs = 0
        for i, key in enumerate(keys):
            bases[i], ps, cs = self._key_args(key, first_part)
        fmt = {self._kfmt(k) for k in keys}
        if len(fmt) > 1:
            raise ValueError("rotate_sum_batch_native: the keys of one call must share one format")
        exps = (ctypes.c_int64 * max(n, 1))(*exponents)
        check(lib.lf_rotate_sum_batch(ctypes.byref(plan), len(c0s), _parr(c0s), _parr(c1s), n, exps, bases, ps, cs, row_off,
                                      fmt.pop() if fmt else 0, 1 if with_self else 0, _p(ws), 0 if ws is None else ws.numel(),
                                      _parr([o[0] for o in outs]), _parr([o[1] for o in outs]), st), "lf_rotate_sum_batch")

    @staticmethod
    def linear_transform_bsgs_ws_words(plan, nb):
        return int(lib.lf_linear_transform_bsgs_ws_words(ctypes.byref(plan), nb))

    def linear_transform_bsgs_native(self, plan, c0, c1, baby_exps, baby_keys, giant_exps, giant_keys, first_part, row_off, pack,
                                     counts, slots, scales, round_at, out, ws):
        """The baby-step / giant-step linear transform as ONE native call (lf_linear_transform_bsgs).  baby_keys / baby_exps: the
        packed keys of the non-zero baby steps and their Galois exponents; giant_keys / giant_exps: per giant step its key and
        exponent (None and 0 for the giant step 0, which comes first); pack [k, rows, N]: the encoded diagonals in (giant, baby)
        order; counts: diagonals per giant step; slots: per diagonal its baby slot (0: the ciphertext, 1 + i: baby key i);
        out [2, ell - 1, N]; ws: at least linear_transform_bsgs_ws_words(plan, len(baby_keys)) words."""
        dev, st = _ds(out)
        nb, ng = len(baby_keys), len(giant_keys)
        keyed = list(baby_keys) + [k for k in giant_keys if k is not None]
        fmt = {self._kfmt(k) for k in keyed}
        if len(fmt) > 1:
            raise ValueError("linear_transform_bsgs_native: the keys of one call must share one format")
        ps = cs = 0
        bb, gb = (ctypes.c_void_p * max(nb, 1))(), (ctypes.c_void_p * max(ng, 1))()
        for i, key in enumerate(baby_keys):
            bb[i], ps, cs = self._key_args(key, first_part)
        for i, key in enumerate(giant_keys):
            if key is not None:
                gb[i], ps, cs = self._key_args(key, first_part)
        i64 = lambda v: (ctypes.c_int64 * max(len(v), 1))(*v)
        check(lib.lf_linear_transform_bsgs(ctypes.byref(plan), _p(c0), _p(c1), nb, i64(baby_exps), bb, ng, i64(giant_exps), gb, ps, cs,
                                           row_off, fmt.pop() if fmt else 0, _p(pack), pack.stride(0), i64(counts), i64(slots),
                                           _p(scales), round_at, _p(ws), ws.numel(), out.data_ptr(),
                                           out.data_ptr() + out.stride(0) * 8, st), "lf_linear_transform_bsgs")

    @staticmethod
    def linear_transform_bsgs_batch_ws_words(plan, nb, nct):
        return int(lib.lf_linear_transform_bsgs_batch_ws_words(ctypes.byref(plan), nb, nct))

    def linear_transform_bsgs_batch_native(self, plan, c0s, c1s, baby_exps, baby_keys, giant_exps, giant_keys, first_part, row_off,
                                           pack, counts, slots, scales, round_at, outs, ws):
        """linear_transform_bsgs_native for len(c0s) <= lt_batch_max_cts ciphertexts under the same diagonals and keys as ONE native
        call (lf_linear_transform_bsgs_batch): groups of 4, 2 or 1 ciphertexts (plan.max_nct permitting) share every launch but the
        diagonal products, and every baby and giant key is read once per group.  c0s / c1s: the components, one tensor each per
        ciphertext; outs: one [2, ell - 1, N] tensor per ciphertext; ws: at least
        linear_transform_bsgs_batch_ws_words(plan, len(baby_keys), len(c0s)) words, 16-byte aligned; the rest as
        linear_transform_bsgs_native."""
        dev, st = _ds(outs[0])
        nb, ng = len(baby_keys), len(giant_keys)
        keyed = list(baby_keys) + [k for k in giant_keys if k is not None]
        fmt = {self._kfmt(k) for k in keyed}
        if len(fmt) > 1:
            raise ValueError("linear_transform_bsgs_batch_native: the keys of one call must share one format")
        ps = cs = 0
        bb, gb = (ctypes.c_void_p * max(nb, 1))(), (ctypes.c_void_p * max(ng, 1))()
        for i, key in enumerate(baby_keys):
            bb[i], ps, cs = self._key_args(key, first_part)
        for i, key in enumerate(giant_keys):
            if key is not None:
                gb[i], ps, cs = self._key_args(key, first_part)
        i64 = lambda v: (ctypes.c_int64 * max(len(v), 1))(*v)
        check(lib.lf_linear_transform_bsgs_batch(ctypes.byref(plan), len(c0s), _parr(c0s), _parr(c1s), nb, i64(baby_exps), bb, ng,
                                                 i64(giant_exps), gb, ps, cs, row_off, fmt.pop() if fmt else 0, _p(pack),
                                                 pack.stride(0), i64(counts), i64(slots), _p(scales), round_at, _p(ws), ws.numel(),
                                                 _parr([o[0] for o in outs]), _parr([o[1] for o in outs]), st),
              "lf_linear_transform_bsgs_batch")

    # include/ckks_hip.h: LF_LT_MATMUL_MAX_INPUTS / LF_LT_MATMUL_MAX_OUTPUTS (tests/test_lt_matmul_cpu.py holds these copies to the
    # header); the keyed steps of a column are bounded by bsgs_max_baby_keys
    lt_matmul_max_inputs = 64
    lt_matmul_max_outputs = 64

    @staticmethod
    def lt_matmul_ws_words(plan, nb_max, k_out):
        return int(lib.lf_lt_matmul_ws_words(ctypes.byref(plan), nb_max, k_out))

    def lt_matmul_native(self, plan, ins, col_exps, col_keys, first_part, row_off, blocks, scales, round_at, outs, ws):
        """A k_out x k_in matrix of diagonal sets times k_in ciphertexts as ONE native call (lf_lt_matmul).  ins: per input the
        pair of tensors (c0, c1), or None for an input no block uses; col_exps / col_keys: per input the Galois exponents and the
        packed keys of its keyed steps, ascending (slot 1 + j of the column; slot 0 is the ciphertext); blocks: k_out rows of
        k_in entries, None or (pack [k, rows, N], slots): the block's encoded diagonals and the column slot of each, ascending;
        outs: k_out tensors [2, ell - 1, N]; ws: at least lt_matmul_ws_words(plan, the longest used column, k_out) words."""
        dev, st = _ds(outs[0])
        cols, _, ps, cs, fmt, blk = self._lt_matmul_marshal("lt_matmul_native", col_exps, col_keys, None, first_part, blocks, len(ins))
        check(lib.lf_lt_matmul(ctypes.byref(plan), len(ins), len(blocks), self._lt_matmul_inputs([ins]), *cols, ps, cs, row_off, fmt, *blk,
                               _p(scales), round_at, _p(ws), ws.numel(), _parr([o[0] for o in outs]), _parr([o[1] for o in outs]), st),
              "lf_lt_matmul")

    @staticmethod
    def _lt_matmul_inputs(toks):
        """The `in` array of the lf_lt_matmul family: [token][input][component], NULL for an input given as None."""
        k_in = len(toks[0])
        inp = (ctypes.c_void_p * (len(toks) * 2 * k_in))()
        for t, ins in enumerate(toks):
            for i, pair in enumerate(ins):
                if pair is not None:
                    inp[2 * (t * k_in + i)], inp[2 * (t * k_in + i) + 1] = pair[0].data_ptr(), pair[1].data_ptr()
        return inp

    def _lt_matmul_marshal(self, name, col_exps, col_keys, giants, first_part, blocks, k_in):
        """((keyed steps per column, their exponents, baby key pointers), (giant steps, their exponents, giant key pointers), part
        stride, component stride, key format, (pack pointers, strides, counts, slots)): the keys and the blocks of the four
        lt_matmul bindings as the C ABI takes them, the tuples in the order of its arguments.  giants: (giant_exps, giant_keys), or
        None for the flat bindings, whose block (pack, slots) is the baby-step / giant-step block (pack, [(0, slots)]) under the one
        giant step 0."""
        flat = giants is None
        giant_exps, giant_keys = ([0], [None]) if flat else giants
        k_out, ng = len(blocks), len(giant_keys)
        babies = [k for col in col_keys for k in col]
        fmt = {self._kfmt(k) for k in babies + [k for k in giant_keys if k is not None]}
        if len(fmt) > 1:
            raise ValueError(f"{name}: the keys of one call must share one format")
        ps = cs = 0
        kb, gb = (ctypes.c_void_p * max(len(babies), 1))(), (ctypes.c_void_p * max(ng, 1))()
        for j, key in enumerate(babies):
            kb[j], ps, cs = self._key_args(key, first_part)
        for j, key in enumerate(giant_keys):
            if key is not None:
                gb[j], ps, cs = self._key_args(key, first_part)
        pts = (ctypes.c_void_p * (k_out * k_in * ng))()
        strides, counts, slots = [0] * (k_out * k_in * ng), [0] * (k_out * k_in * ng), []
        for o, row in enumerate(blocks):
            for i, blk in enumerate(row):
                if blk is None:
                    continue
                pack, per_giant = blk
                for j, part in enumerate([(0, per_giant)] if flat else per_giant):
                    if part is None:
                        continue
                    first, sl = part
                    e = (o * k_in + i) * ng + j
                    pts[e] = pack.data_ptr() + first * pack.stride(0) * 8
                    strides[e], counts[e] = pack.stride(0), len(sl)
                    slots += list(sl)
        i64 = lambda v: (ctypes.c_int64 * max(len(v), 1))(*v)
        return ((i64([len(c) for c in col_keys]), i64([e for c in col_exps for e in c]), kb), (ng, i64(giant_exps), gb), ps, cs,
                (fmt.pop() if fmt else 0), (pts, i64(strides), i64(counts), i64(slots)))


    # include/ckks_hip.h: LF_LT_MATMUL_BATCH_MAX_TOKENS through _native.py's copy (tests/test_lt_matmul_batch_cpu.py holds both to
    # the header); the group sizes lf_lt_matmul_batch takes beside 1
    lt_matmul_batch_max_tokens = LF_LT_MATMUL_BATCH_MAX_TOKENS
    lt_matmul_batch_sizes = (4, 2)

    @staticmethod
    def lt_matmul_batch_ws_words(plan, nb_max, k_out, nt):
        return int(lib.lf_lt_matmul_batch_ws_words(ctypes.byref(plan), nb_max, k_out, nt))

    def lt_matmul_batch_native(self, plan, toks, col_exps, col_keys, first_part, row_off, blocks, scales, round_at, outs, ws):
        """lt_matmul_native for a group of nt = 1, 2 or 4 token vectors under one matrix and one key set as ONE native call
        (lf_lt_matmul_batch; the plan sized for nt).  toks: per token what lt_matmul_native takes as `ins` (an input no block uses
        may be None); outs: per token k_out tensors [2, ell - 1, N]; ws: at least lt_matmul_batch_ws_words(plan, the longest used
        column, k_out, nt) words; everything else as lt_matmul_native."""
        dev, st = _ds(outs[0][0])
        cols, _, ps, cs, fmt, blk = self._lt_matmul_marshal("lt_matmul_batch_native", col_exps, col_keys, None, first_part, blocks, len(toks[0]))
        check(lib.lf_lt_matmul_batch(ctypes.byref(plan), len(toks), len(toks[0]), len(blocks), self._lt_matmul_inputs(toks), *cols, ps, cs,
                                     row_off, fmt, *blk, _p(scales), round_at, _p(ws), ws.numel(), _parr([o[0] for tok in outs for o in tok]),
                                     _parr([o[1] for tok in outs for o in tok]), st),
              "lf_lt_matmul_batch")

    # include/ckks_hip.h: LF_LT_MATMUL_BSGS_MAX_GIANTS / LF_LT_MATMUL_BSGS_MAX_SUMS through _native.py's copies
    # (tests/test_lt_matmul_bsgs_cpu.py holds them to the header): the giant steps and the keyed inner sums of one lf_lt_matmul_bsgs call
    lt_matmul_bsgs_max_giants = LF_LT_MATMUL_BSGS_MAX_GIANTS
    lt_matmul_bsgs_max_sums = LF_LT_MATMUL_BSGS_MAX_SUMS

    @staticmethod
    def lt_matmul_bsgs_ws_words(plan, nb_max, k_out, keyed_sums):
        return int(lib.lf_lt_matmul_bsgs_ws_words(ctypes.byref(plan), nb_max, k_out, keyed_sums))

    def lt_matmul_bsgs_native(self, plan, ins, col_exps, col_keys, giant_exps, giant_keys, first_part, row_off, blocks, scales,
                              round_at, outs, ws):
        """A k_out x k_in matrix of baby-step / giant-step diagonal sets times k_in ciphertexts as ONE native call
        (lf_lt_matmul_bsgs).  ins / col_exps / col_keys: as lt_matmul_native, for the keyed BABY steps of each column; giant_exps /
        giant_keys: per giant step its exponent and packed key (0 and None for the giant step 0, which comes first); blocks: k_out
        rows of k_in entries, None or (pack [k, rows, N], per giant step None or (first, slots)): the block's encoded diagonals
        in (giant, baby) order, per giant step the index of its first diagonal in the pack and the column slot of each,
        ascending; outs: k_out tensors [2, ell - 1, N]; ws: at least lt_matmul_bsgs_ws_words(..) words."""
        dev, st = _ds(outs[0])
        cols, giants, ps, cs, fmt, blk = self._lt_matmul_marshal("lt_matmul_bsgs_native", col_exps, col_keys, (giant_exps, giant_keys),
                                                                 first_part, blocks, len(ins))
        check(lib.lf_lt_matmul_bsgs(ctypes.byref(plan), len(ins), len(blocks), self._lt_matmul_inputs([ins]), *cols, *giants, ps, cs, row_off,
                                    fmt, *blk, _p(scales), round_at, _p(ws), ws.numel(), _parr([o[0] for o in outs]),
                                    _parr([o[1] for o in outs]), st), "lf_lt_matmul_bsgs")

    # include/ckks_hip.h: LF_LT_MATMUL_BSGS_BATCH_MAX_TOKENS through _native.py's copy (tests/test_lt_matmul_bsgs_batch_cpu.py holds
    # both to the header); the group sizes lf_lt_matmul_bsgs_batch takes beside 1
    lt_matmul_bsgs_batch_max_tokens = LF_LT_MATMUL_BSGS_BATCH_MAX_TOKENS
    lt_matmul_bsgs_batch_sizes = (4, 2)

    @staticmethod
    def lt_matmul_bsgs_batch_ws_words(plan, nb_max, k_out, keyed_sums, nt):
        return int(lib.lf_lt_matmul_bsgs_batch_ws_words(ctypes.byref(plan), nb_max, k_out, keyed_sums, nt))

    def lt_matmul_bsgs_batch_call(self, plan, toks, col_exps, col_keys, giant_exps, giant_keys, first_part, row_off, blocks, scales,
                                  round_at, outs, ws):
        """lt_matmul_bsgs_native for a group of nt = 1, 2 or 4 token vectors under one matrix and one key set as ONE native call
        (lf_lt_matmul_bsgs_batch; the plan sized for nt).  toks: per token what lt_matmul_bsgs_native takes as `ins` (an input no
        block uses may be None); outs: per token k_out tensors [2, ell - 1, N]; ws: at least lt_matmul_bsgs_batch_ws_words(plan,
        the longest used column, k_out, the keyed inner sums of one token, nt) words; everything else as lt_matmul_bsgs_native.
        (The name: the engine's *_native entries are a closed list the fenced and the stream-contract suites go through one by one;
        this entry has tests of its own for both.)"""
        dev, st = _ds(outs[0][0])
        cols, giants, ps, cs, fmt, blk = self._lt_matmul_marshal("lt_matmul_bsgs_batch_call", col_exps, col_keys, (giant_exps, giant_keys),
                                                                 first_part, blocks, len(toks[0]))
        check(lib.lf_lt_matmul_bsgs_batch(ctypes.byref(plan), len(toks), len(toks[0]), len(blocks), self._lt_matmul_inputs(toks), *cols,
                                          *giants, ps, cs, row_off, fmt, *blk, _p(scales), round_at, _p(ws), ws.numel(),
                                          _parr([o[0] for tok in outs for o in tok]), _parr([o[1] for tok in outs for o in tok]), st),
              "lf_lt_matmul_bsgs_batch")

    def ks_gather(self, ext, dst, index, rows, logN, c: Consts):
        """dst[p][r][k] = ext[p][r][index[k]] for extended digits as ks_fwd leaves them: fp64-class rows of a mixed stack in the
        planes format (u32 low words at byte 0, u16 high halves at byte 4 N of the row: LF_TUNE_DIGIT_PLANES), other rows raw
        words.  torch gathers, no kernel of its own (the orchestrated form of hoisted rotations; the native op gathers in registers)."""
        q = c.q_host[:rows]
        small = torch.as_tensor(q < SMALL_PRIME_LIMIT)
        planes = logN > 12 and bool(small.any()) and not bool(small.all()) and lib.lf_tune(3, -1) == 1
        if not planes:
            torch.index_select(ext, ext.dim() - 1, index, out=dst)
            return
        N = 1 << logN
        sm = torch.nonzero(small).flatten().to(ext.device)
        bg = torch.nonzero(~small).flatten().to(ext.device)
        dst[:, bg] = ext[:, bg].index_select(2, index)
        e32, d32 = ext.view(torch.int32), dst.view(torch.int32)
        e16, d16 = ext.view(torch.int16), dst.view(torch.int16)
        d32[:, sm, :N] = e32[:, sm, :N].index_select(2, index)
        d16[:, sm, 2 * N:3 * N] = e16[:, sm, 2 * N:3 * N].index_select(2, index)

    ks_batch_sizes = (4, 2)   # ciphertexts per lf_ks_core_batch call (largest first)

    def ks_core_batch(self, states, nparts, rows, logN, desc, E, Ed, key, first_part, row_off, tmp, s, psi, ipsi, Ninv,
                      c: Consts, fold=None):
        """ks_core for len(states) in (2, 4) ciphertexts under one key: states = [nct, state_rows, N] tensor,
        tmp [nct, nparts, rows, N], s [nct, 2, rows, N].  fold = (x [nct, 4, ell, N], PR [ell]), see ks_core."""
        dev, st = _ds(s)
        part_stride, comp_stride = key.stride(0), key.stride(1)
        base = key.data_ptr() + first_part * part_stride * 8
        psi_dp = twiddles.dp_pointer(psi, c.ql, c.qh, c.kl, c.kh, dev, st)
        ipsi_dp = twiddles.dp_pointer(ipsi, c.ql, c.qh, c.kl, c.kh, dev, st)
        if fold is not None:
            x, PR, own = fold
            check(lib.lf_relin_core_batch(_p(states), states.stride(0), states.size(0), nparts, rows, logN, _p(desc), _p(E),
                                          _pd(Ed), base, part_stride, comp_stride, row_off, self._kfmt(key), _p(tmp), _p(s), _p(psi), psi_dp,
                                          _p(ipsi), ipsi_dp, _p(Ninv), _p(x), x.stride(0), _p(PR), x.size(2), _pb(own), c.qptr(),
                                          *c.mont(), dev, st), "lf_relin_core_batch")
            return
        check(lib.lf_ks_core_batch(_p(states), states.stride(0), states.size(0), nparts, rows, logN, _p(desc), _p(E),
                                   _pd(Ed), base, part_stride, comp_stride, row_off, self._kfmt(key), _p(tmp), _p(s), _p(psi), psi_dp,
                                   _p(ipsi), ipsi_dp, _p(Ninv), c.qptr(), *c.mont(), dev, st), "lf_ks_core_batch")

    def ks_moddown(self, s, out, addend, ell, K, PiR, Rs, c: Consts, PiP=None):
        dev, st = _ds(out)
        check(lib.lf_ks_moddown(_p(s), _p(out), _p(addend), ell, K, out.size(-1), _p(PiR),
                                _pd(PiP), _p(Rs), *c.mont(), dev, st), "lf_ks_moddown")
