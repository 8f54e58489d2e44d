"""Encoded plaintexts, mixed into `ckks_engine`: a message vector encoded ONCE (encode_plain) and then multiplied into, added to,
or summed against ciphertexts any number of times (pc_mult, pc_add, pc_dot, pc_matmul, pc_matmul_batch) — per-channel weights, masks, biases,
convolution taps, layers.  The reference only has mc_mult / mc_add, which encode on every call; like the engine's other options beyond it, the words
of these ops are DEFINED as compositions of ops the engine already has (written out in the docstrings), and that composition is
what runs wherever the native call (lf_pc_dot, lf_pc_matmul, lf_pc_matmul_batch) does not apply.  A "mult" plaintext also has a
compact form (compact_plain: fp64-class rows as 6-byte planes, three quarters of the memory at level 0 of the presets), which the
four product ops take wherever they take the raw one (lf_pc_matmul_batch_planes).  DESIGN.md §4.2.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from .backend import SMALL_PRIME_LIMIT
from .evaluator import is_struct
from .presets import errors, types


class PlainOps:
    # =============================================================================================
    # the encoded object
    # =============================================================================================
    def encode_plain(self, m, level: int, op: str = "mult", compact: bool = False):
        """The plaintext mc_mult (op="mult") resp. mc_add (op="add") builds from the message `m` for a ciphertext at `level`, as
        a data_struct of its own (one [rows, N] tensor per local device) that save / load / cpu / cuda / clone treat like any other:
          "mult"  enter_ntt(tile_unsigned(encode(m * sqrt(deviations[level + 1]), 0), level)): NTT domain, Montgomery form;
          "add"   mont_enter_scale(tile_unsigned(encode(m, level), level)): coefficient domain, Montgomery form.
        compact=True ("mult" only): compact_plain of that plaintext."""
        if op not in ("mult", "add"):
            raise ValueError(f"encode_plain: op must be 'mult' or 'add', got {op!r}")
        if compact and op != "mult":
            raise ValueError("encode_plain: only a 'mult' plaintext has a compact form")
        if not 0 <= level < self.num_levels:
            raise errors.MaximumLevelError(level=level, level_max=self.num_levels)
        if op == "mult":
            if level + 1 >= self.num_levels:
                raise errors.MaximumLevelError(level=level, level_max=self.num_levels)
            m = np.array(m) * np.sqrt(self.deviations[level + 1])
            pt = self.ntt.tile_unsigned(self.encode(m, 0), level)
            self.ntt.enter_ntt(pt, level)
            pt = self._new(pt, types.origins["pt_mult"], level=level, ntt_state=True, montgomery_state=True)
            return self.compact_plain(pt) if compact else pt
        pt = self.ntt.tile_unsigned(self.encode(m, level), level)
        self.ntt.mont_enter_scale(pt, level)
        return self._new(pt, types.origins["pt_add"], level=level, montgomery_state=True)

    # =============================================================================================
    # the compact form of a "mult" plaintext ("plain planes", include/ckks_hip.h: lf_plain_planes)
    # =============================================================================================
    # One flat int64 tensor per local device, the rows of pt.data[i] back to back in their order: a row whose prime is below
    # SMALL_PRIME_LIMIT (fp64 class) is 6 N bytes — u32 lo[N], then u16 hi[N] — of v = REDC(w), the plain word in [0, q] the product
    # kernels form from the Montgomery word w on every read; any other row is its 8 N bytes as they are.
    def _plain_primes(self, level, d):
        return [int(self.ctx.q[i]) for i in self.ntt.p.destination_arrays[level][d]]

    @staticmethod
    def plain_planes_offsets(primes, N):
        """Word offset of every row of a compact plaintext over `primes`, and the total behind them: rows + 1 entries."""
        off = [0]
        for q in primes:
            off.append(off[-1] + (3 * N // 4 if q < SMALL_PRIME_LIMIT else N))
        return off

    @staticmethod
    def _mulmod41(a, b, q):
        """a b mod q for a tensor a in [0, q), Python ints b in [0, q) and q < 2^41 per row ([rows, 1] columns): b in three 14-bit
        digits, every intermediate below 2^56."""
        col = lambda v: torch.tensor(v, dtype=torch.int64, device=a.device).view(-1, 1)
        qc = col(q)
        acc = (a * col([x >> 28 for x in b])) % qc
        acc = ((acc << 14) + a * col([(x >> 14) & 0x3fff for x in b])) % qc
        return ((acc << 14) + a * col([x & 0x3fff for x in b])) % qc

    def _planes_pack_rows(self, words, primes):
        """[rows, N] stored words (v on fp64-class rows, w on the others) -> the flat compact tensor: pure byte moves."""
        N = words.size(1)
        off = self.plain_planes_offsets(primes, N)
        flat = torch.empty(off[-1], dtype=torch.int64, device=words.device)
        for r, q in enumerate(primes):
            if q >= SMALL_PRIME_LIMIT:
                flat[off[r]:off[r + 1]] = words[r]
                continue
            halves = words[r].contiguous().view(torch.int16).view(N, 4)          # little-endian: bits 0-15, 16-31, 32-47, 48-63
            flat[off[r]:off[r] + N // 2].view(torch.int16).view(N, 2).copy_(halves[:, 0:2])
            flat[off[r] + N // 2:off[r + 1]].view(torch.int16).copy_(halves[:, 2])
        return flat

    def _planes_unpack_rows(self, flat, primes, N):
        """The inverse of _planes_pack_rows: the stored words as [rows, N]."""
        off = self.plain_planes_offsets(primes, N)
        if flat.dim() != 1 or flat.numel() != off[-1]:
            raise errors.NotMatchDataStructState(origin=types.origins["pt_mult_planes"])
        words = torch.zeros((len(primes), N), dtype=torch.int64, device=flat.device)
        for r, q in enumerate(primes):
            if q >= SMALL_PRIME_LIMIT:
                words[r] = flat[off[r]:off[r + 1]]
                continue
            halves = words[r].view(torch.int16).view(N, 4)
            halves[:, 0:2] = flat[off[r]:off[r] + N // 2].view(torch.int16).view(N, 2)
            halves[:, 2] = flat[off[r] + N // 2:off[r + 1]].view(torch.int16)
        return words

    def _planes_host(self, t, primes):
        """compact_plain's words in torch, on whatever device t is: REDC(w) = w R^-1 mod q as the representative REDC62 returns for a
        lazy w < 2q — the canonical residue, except that w = q gives q itself."""
        small = [r for r, q in enumerate(primes) if q < SMALL_PRIME_LIMIT]
        words = t.clone()
        if small:
            q = [primes[r] for r in small]
            qc = torch.tensor(q, dtype=torch.int64, device=t.device).view(-1, 1)
            w = t[small]
            v = self._mulmod41(w % qc, [pow(self.ctx.R, -1, x) for x in q], q)
            words[small] = torch.where(w == qc, qc, v)
        return self._planes_pack_rows(words, primes)

    def _unplanes_host(self, flat, primes, N):
        words = self._planes_unpack_rows(flat, primes, N)
        qall = torch.tensor(primes, dtype=torch.int64, device=flat.device).view(-1, 1)
        small = [r for r, q in enumerate(primes) if q < SMALL_PRIME_LIMIT]
        out = words % qall
        if small:
            q = [primes[r] for r in small]
            out[small] = self._mulmod41(out[small], [self.ctx.R % x for x in q], q)
        return out

    def _planes_native_ok(self, t, rows):
        return t.is_cuda and hasattr(self.backend, "plain_planes") and 13 <= self.ctx.logN <= 17 and t.dtype == torch.int64 \
            and rows <= self.backend.plain_planes_max_rows and t.is_contiguous() and t.data_ptr() % 16 == 0

    def compact_plain(self, pt):
        """The compact form of a "mult" plaintext: same level, same hash, ONE flat tensor per local device with the fp64-class rows
        as 6-byte planes (8 rows N -> (6 n_small + 8 n_int) N bytes; level 0 of the presets: about three quarters).  pc_mult, pc_dot,
        pc_matmul and pc_matmul_batch take it wherever they take pt; clone, cpu, cuda, save and load treat it like pt.  A compact
        plaintext is returned as it is; anything else than a "mult" plaintext raises NotMatchType.  One native launch per device where
        the tensor is on the GPU (logN 13 .. 17), the same words in torch elsewhere."""
        if is_struct(pt) and pt.origin == types.origins["pt_mult_planes"]:
            return pt
        self._check_plain(pt, "mult")
        self._enter()
        data = []
        for d, t in zip(self._loc(pt.level), pt.data):
            primes = self._plain_primes(pt.level, d)
            if self._planes_native_ok(t, len(primes)):
                c = self._consts(d, pt.level, False)
                flat = torch.empty(self.backend.plain_planes_words(len(primes), self.ctx.N, c), dtype=torch.int64, device=t.device)
                self.backend.plain_planes(t, flat, c)
            else:
                flat = self._planes_host(t, primes)
            data.append(flat)
        return pt._replace(data=data, origin=types.origins["pt_mult_planes"])

    def expand_plain(self, pt):
        """The inverse of compact_plain: a "mult" plaintext that holds the canonical Montgomery residue w mod q of every word the
        compact one was made from (the same residues: every product op gives the same words).  A raw "mult" plaintext is returned
        as it is."""
        self._check_plain(pt, "mult", planes_ok=True)
        if pt.origin == types.origins["pt_mult"]:
            return pt
        self._enter()
        N, data = self.ctx.N, []
        for d, flat in zip(self._loc(pt.level), pt.data):
            primes = self._plain_primes(pt.level, d)
            if flat.dim() == 1 and flat.numel() == self.plain_planes_offsets(primes, N)[-1] and self._planes_native_ok(flat, len(primes)):
                t = torch.empty((len(primes), N), dtype=torch.int64, device=flat.device)
                self.backend.plain_unplanes(flat, t, self._consts(d, pt.level, False))
            else:
                t = self._unplanes_host(flat, primes, N)
            data.append(t)
        return pt._replace(data=data, origin=types.origins["pt_mult"])

    def _move_plain_planes(self, pt, direction):
        """cpu() / cuda() of a compact plaintext: the stored words as rows, moved like any other rows, packed again over the primes
        of where they arrive (the host form: every row of the level, in the order of the prime chain).  Byte moves only."""
        N, lvl = self.ctx.N, pt.level
        dest = self.ntt.p.destination_arrays[lvl]
        chain = [int(self.ctx.q[i]) for i in sorted(i for d in dest for i in d)]
        if direction == "gpu2cpu":
            rows = [self._planes_unpack_rows(t, self._plain_primes(lvl, d), N) for d, t in zip(self._loc(lvl), pt.data)]
            host = self.download_to_cpu(rows, lvl, False)[0]
            return pt._replace(data=[self._planes_pack_rows(host[:len(chain)], chain)])
        host = self._planes_unpack_rows(pt.data[0], chain, N)
        rows = self.upload_to_gpu([host], lvl, False)
        return pt._replace(data=[self._planes_pack_rows(t, self._plain_primes(lvl, d)) for d, t in zip(self._loc(lvl), rows)])

    @staticmethod
    def _plain_kind(pts, op):
        """True where the "mult" plaintexts of a call are all compact, False where none is; a mix is refused."""
        kinds = {pt.origin == types.origins["pt_mult_planes"] for pt in pts}
        if len(kinds) > 1:
            raise ValueError(f"{op}: compact and raw plaintexts in one call (compact_plain or expand_plain them all)")
        return kinds == {True}

    def _expanded(self, pts):
        """{id: expand_plain} of the distinct objects among pts (None skipped)."""
        out = {}
        for pt in pts:
            if pt is not None and id(pt) not in out:
                out[id(pt)] = self.expand_plain(pt)
        return out

    def _pc_native(self, l, entry):
        """The device where the backend's one-call `entry` (pc_dot_native, pc_matmul_native, pc_matmul_batch_native or
        pc_matmul_batch_planes_call) applies at level l -> l + 1, or None: both levels on that ONE device of this process, a
        backend that has the entry, logN 13 .. 17 (below 13 _native_level says None for every backend with native ops), the rows of
        l + 1 those of l in their order behind the dropped limb and, for compact plaintexts, no more rows than their mask has bits."""
        d = self._native_level(l + 1)
        dest = self.ntt.p.destination_arrays
        if d is None or self._native_level(l) != d or not hasattr(self.backend, entry) or not 13 <= self.ctx.logN <= 17 \
                or (entry == "pc_matmul_batch_planes_call" and len(dest[l][d]) > self.backend.plain_planes_max_rows) \
                or list(dest[l][d][1:]) != list(dest[l + 1][d]):
            return None
        return d

    def _pc_planes_native(self, l):
        """The device where lf_pc_matmul_batch_planes applies at level l -> l + 1, or None."""
        return self._pc_native(l, "pc_matmul_batch_planes_call")

    @staticmethod
    def _pc_operand_ok(t):
        """What the native calls ask of an operand's tensor (16-byte loads: a contiguous view at an odd word offset takes the
        composition; so does a tensor moved to the host, which the level cannot see)."""
        return t.is_contiguous() and t.dtype == torch.int64 and t.data_ptr() % 16 == 0 and t.is_cuda

    def _pc_operands_ok(self, cts, plains):
        """_pc_operand_ok of both components of every ciphertext and of every distinct plaintext / bias (None skipped)."""
        return all(self._pc_operand_ok(t) for ct in cts for t in (ct.data[0][0], ct.data[1][0])) \
            and all(self._pc_operand_ok(x.data[0]) for x in {id(x): x for x in plains if x is not None}.values())

    # =============================================================================================
    # checks (all before any launch)
    # =============================================================================================
    @staticmethod
    def _check_plain(pt, kind, planes_ok=False):
        want = types.origins["pt_" + kind]
        if not is_struct(pt) or (pt.origin != want and not (planes_ok and pt.origin == types.origins["pt_mult_planes"])):
            raise errors.NotMatchType(origin=getattr(pt, "origin", type(pt).__name__), to=want)
        if pt.include_special or not pt.montgomery_state or pt.ntt_state != (kind == "mult"):
            raise errors.NotMatchDataStructState(origin=pt.origin)

    @staticmethod
    def _check_plain_operand(ct):
        if not is_struct(ct) or ct.origin != types.origins["ct"]:
            raise errors.NotMatchType(origin=getattr(ct, "origin", type(ct).__name__), to=types.origins["ct"])
        if ct.ntt_state or ct.include_special:
            raise errors.NotMatchDataStructState(origin=ct.origin)

    def _check_plain_pair(self, pt, ct, kind):
        self._check_plain(pt, kind, planes_ok=kind == "mult")
        self._check_plain_operand(ct)
        if pt.level != ct.level:
            raise errors.NotMatchDataStructState(origin=f"{pt.origin} at level {pt.level} beside level {ct.level}")

    # =============================================================================================
    # the ops
    # =============================================================================================
    def pc_mult(self, pt, ct):
        """mc_mult(m, ct) for pt = encode_plain(m, ct.level): mc_mult's body behind its encode, the same words whenever encode
        returns the same polynomial.  A compact pt (compact_plain) goes through pc_dot's one-pair path: the same words."""
        self._enter()
        self._check_plain_pair(pt, ct, "mult")
        l = ct.level
        if l + 1 >= self.num_levels:
            raise errors.MaximumLevelError(level=l, level_max=self.num_levels)
        if pt.origin == types.origins["pt_mult_planes"]:
            return self.pc_dot([(pt, ct)])
        out = self.clone(ct)
        self.ntt.enter_ntt(out.data[0], l)
        self.ntt.enter_ntt(out.data[1], l)
        d0 = self.ntt.mont_mult(pt.data, out.data[0], l)
        d1 = self.ntt.mont_mult(pt.data, out.data[1], l)
        self.ntt.intt_exit_reduce(d0, l)
        self.ntt.intt_exit_reduce(d1, l)
        return self.rescale(out._replace(data=[d0, d1]))

    def pc_add(self, pt, ct):
        """mc_add(m, ct) for pt = encode_plain(m, ct.level, "add"): mc_add's body behind its encode."""
        self._enter()
        self._check_plain_pair(pt, ct, "add")
        l = ct.level
        out = self.clone(ct)
        self.ntt.mont_enter(out.data[0], l)
        d0 = self.ntt.mont_add(pt.data, out.data[0], l)
        self.ntt.mont_redc(d0, l)
        self.ntt.reduce_2q(d0, l)
        return out._replace(data=[d0, out.data[1]])

    def pc_dot(self, pairs, bias=None):
        """sum_i pt_i * ct_i (+ bias) over the pairs (pt_i, ct_i) as ONE ciphertext at level + 1, under one rescale.  Every pt_i an
        encode_plain(.., level) of kind "mult", every ct_i a ciphertext of that level (coefficient domain, no special limbs; the
        same object may repeat on either side), bias an encode_plain(.., level + 1, "add") or None.  The product with a plaintext
        is linear in the ciphertext, so the inverse transforms and the rescale run once, on the sum: one rescale rounding instead
        of len(pairs).  The result has exactly the words of
            S_c = mont_mult(pt_0, enter_ntt(ct_0.c));  S_c = mont_add(S_c, mont_mult(pt_i, enter_ntt(ct_i.c)))  for i >= 1, c = 0, 1
            intt_exit_reduce(S_c);  out = rescale((S_0, S_1));  out = pc_add(bias, out)  if bias is given
        (one pair without bias: pc_mult), which is also what runs where the native call does not apply: several devices or ranks,
        logN outside 13..17, a checker backend, operands that are not contiguous or not 16-byte aligned.  Otherwise ONE native call
        (lf_pc_dot).  The pt_i may all be compact (compact_plain; a mix raises ValueError): the result has exactly the words of the
        call on expand_plain of each — which are those of the call on the plaintexts they were compacted from — through ONE
        lf_pc_matmul_batch_planes call under the same conditions, and through expand_plain and the paths above elsewhere."""
        self._enter()
        pairs = [tuple(p) for p in pairs]
        if not pairs:
            raise ValueError("pc_dot: at least one (plaintext, ciphertext) pair")
        for pair in pairs:
            if len(pair) != 2:
                raise ValueError("pc_dot: pairs of an encoded plaintext and a ciphertext")
            self._check_plain(pair[0], "mult", planes_ok=True)
            self._check_plain_operand(pair[1])
        compact = self._plain_kind([pt for pt, _ in pairs], "pc_dot")
        l = pairs[0][1].level
        for pt, ct in pairs:
            for x in (pt, ct):
                if x.level != l:
                    raise errors.NotMatchDataStructState(origin=f"{x.origin} at level {x.level} beside level {l}")
        if bias is not None:
            self._check_plain(bias, "add")
            if bias.level != l + 1:
                raise errors.NotMatchDataStructState(origin=f"{bias.origin} at level {bias.level} beside level {l + 1}")
        if l + 1 >= self.num_levels:
            raise errors.MaximumLevelError(level=l, level_max=self.num_levels)
        d = self._pc_native(l, "pc_matmul_batch_planes_call" if compact else "pc_dot_native")
        if d is not None and self._pc_operands_ok([ct for _, ct in pairs], [pt for pt, _ in pairs] + [bias]):
            if compact:
                return self._pc_matmul_batch_native([[pt for pt, _ in pairs]], [[ct for _, ct in pairs]], [bias], l, d, planes=True)[0][0]
            return self._pc_dot_native(pairs, bias, l, d)
        if compact:
            raw = self._expanded(pt for pt, _ in pairs)
            return self.pc_dot([(raw[id(pt)], ct) for pt, ct in pairs], bias)
        S = None
        for pt, ct in pairs:
            x = self.clone(ct)
            term = []
            for comp in range(2):
                self.ntt.enter_ntt(x.data[comp], l)
                term.append(self.ntt.mont_mult(pt.data, x.data[comp], l))
            S = term if S is None else [self.ntt.mont_add(S[comp], term[comp], l) for comp in range(2)]
        for comp in range(2):
            self.ntt.intt_exit_reduce(S[comp], l)
        out = self.rescale(self._new(S, types.origins["ct"], level=l))
        return out if bias is None else self.pc_add(bias, out)

    def _pc_matmul_checked(self, W, cts, bias):
        """pc_matmul's checks on materialised lists, in its order: (bias as a list of k_out entries, the level)."""
        k_out, k_in = len(W), len(cts)
        if not W or not cts:
            raise ValueError("pc_matmul: at least one row of plaintexts and one ciphertext")
        for row in W:
            if len(row) != k_in:
                raise ValueError(f"pc_matmul: a row of {len(row)} plaintexts beside {k_in} ciphertexts")
            if all(pt is None for pt in row):
                raise ValueError("pc_matmul: a row without a plaintext")
            for pt in row:
                if pt is not None:
                    self._check_plain(pt, "mult", planes_ok=True)
        self._plain_kind([pt for row in W for pt in row if pt is not None], "pc_matmul")
        for ct in cts:
            self._check_plain_operand(ct)
        l = cts[0].level
        for x in cts + [pt for row in W for pt in row if pt is not None]:
            if x.level != l:
                raise errors.NotMatchDataStructState(origin=f"{x.origin} at level {x.level} beside level {l}")
        if bias is not None:
            if len(bias) != k_out:
                raise ValueError(f"pc_matmul: {len(bias)} biases for {k_out} rows")
            for b in bias:
                if b is not None:
                    self._check_plain(b, "add")
                    if b.level != l + 1:
                        raise errors.NotMatchDataStructState(origin=f"{b.origin} at level {b.level} beside level {l + 1}")
        else:
            bias = [None] * k_out
        if l + 1 >= self.num_levels:
            raise errors.MaximumLevelError(level=l, level_max=self.num_levels)
        return bias, l

    def pc_matmul(self, W, cts, bias=None):
        """A plaintext matrix times a vector of ciphertexts: the list of the k_out ciphertexts sum_i W[o][i] * cts[i] (+ bias[o]) at
        level + 1, one rescale each.  W: k_out rows of k_in entries, each an encode_plain(.., level) of kind "mult" or None (a zero
        weight, skipped; every row needs an entry); cts: k_in ciphertexts of that level (coefficient domain, no special limbs);
        bias: None, or k_out entries, each None or an encode_plain(.., level + 1, "add").  Objects may repeat on either side; a
        ciphertext whose whole column is None is legal and is not touched.  Output o has exactly the words of
            pc_dot([(W[o][i], cts[i]) for i in range(k_in) if W[o][i] is not None], bias[o])
        and that loop is what runs where the native call does not apply (pc_dot's conditions).  Otherwise ONE native call
        (lf_pc_matmul) per 64 outputs: every ciphertext is transformed once, whatever k_out, and every transformed word is read
        once per group of four outputs.  The entries of W may all be compact (compact_plain; a mix raises ValueError): the same
        words as on expand_plain of each, through ONE lf_pc_matmul_batch_planes call per 64 outputs under the same conditions, and
        through expand_plain and the paths above elsewhere."""
        self._enter()
        W = [list(row) for row in W]
        cts = list(cts)
        k_out = len(W)
        bias, l = self._pc_matmul_checked(W, cts, None if bias is None else list(bias))
        planes = next(pt for pt in W[0] if pt is not None).origin == types.origins["pt_mult_planes"]
        d = self._pc_native(l, "pc_matmul_batch_planes_call" if planes else "pc_matmul_native")
        if d is not None and self._pc_operands_ok(cts, [pt for row in W for pt in row] + bias):
            step = self.backend.pc_matmul_max_outputs
            if planes:
                return [out for o0 in range(0, k_out, step)
                        for out in self._pc_matmul_batch_native(W[o0:o0 + step], [cts], bias[o0:o0 + step], l, d, planes=True)[0]]
            return [out for o0 in range(0, k_out, step) for out in self._pc_matmul_native(W[o0:o0 + step], cts, bias[o0:o0 + step], l, d)]
        if planes:
            raw = self._expanded(pt for row in W for pt in row)
            return self.pc_matmul([[None if pt is None else raw[id(pt)] for pt in row] for row in W], cts, bias)
        return [self.pc_dot([(pt, ct) for pt, ct in zip(row, cts) if pt is not None], b) for row, b in zip(W, bias)]

    def _pc_matmul_native(self, W, cts, bias, l, d):
        """One lf_pc_matmul call."""
        return self._pc_matmul_call("pc_matmul_native", W, [cts], bias, l, d)[0]

    # group sizes of pc_matmul_batch's native path, largest first (filtered by backend.pc_matmul_batch_sizes), as rsum_batch_sizes: a
    # size that does not beat the loop is left out here and its tokens take pc_matmul one by one — the words are the same.
    # Groups of 4 are left out: on MI355X they lose to groups of 2 everywhere and to the loop at silver (DESIGN.md §4.2 has the
    # numbers); the backend still takes them (tools/pc_matmul_batch.py --ab measures them).
    pc_matmul_batch_sizes = (2,)

    def pc_matmul_batch(self, W, X, bias=None):
        """pc_matmul of many token vectors under the SAME matrix (a dense layer over the tokens of a sequence or the samples of a
        batch): returns exactly [pc_matmul(W, cts, bias) for cts in X], word for word and in order — B lists of k_out ciphertexts
        at level + 1; an empty X gives [].  W, bias: as pc_matmul takes them; X: B token vectors of k_in ciphertexts each (the same
        object may appear in any number of tokens and positions).  What pc_matmul refuses for any token is refused for the whole
        call before anything is allocated or launched, with the error the loop would have raised first.  Where pc_matmul's native
        call applies to a token and the backend has lf_pc_matmul_batch, the tokens that qualify go, in order, in groups of
        pc_matmul_batch_sizes (pairs) through ONE native call per group and per 64 outputs: a group shares every product launch,
        which reads each plaintext word — the larger stream of pc_matmul's products — once per group instead of once per token.  A token
        that does not qualify (a component that is not contiguous, not 16-byte aligned or on the host), the one the groups leave
        over, and every token on a backend without the entry take pc_matmul and keep their place.  The entries of W may all be
        compact (compact_plain; a mix raises ValueError): the same group sizes and the same left-over rule, every native call
        lf_pc_matmul_batch_planes; where that entry does not apply to W (several devices or ranks, a checker backend, logN outside
        13..17) the plaintexts are expanded once for the call and the paths above run."""
        self._enter()
        X = [list(cts) for cts in X]
        if not X:
            return []
        W = [list(row) for row in W]
        bias = None if bias is None else list(bias)
        k_out = len(W)
        levels = [self._pc_matmul_checked(W, cts, bias)[1] for cts in X]
        l = levels[0]                                   # (every token is at W's level, so all levels are equal)
        bias = [None] * k_out if bias is None else bias
        out = [None] * len(X)
        ready = []
        sizes = [k for k in self.pc_matmul_batch_sizes if k in getattr(self.backend, "pc_matmul_batch_sizes", ())]
        planes = next(pt for pt in W[0] if pt is not None).origin == types.origins["pt_mult_planes"]
        d = self._pc_native(l, "pc_matmul_batch_planes_call" if planes else "pc_matmul_batch_native")
        if planes and d is None:
            raw = self._expanded(pt for row in W for pt in row)
            return self.pc_matmul_batch([[None if pt is None else raw[id(pt)] for pt in row] for row in W], X, bias)
        if sizes and d is not None and self._pc_operands_ok([], [pt for row in W for pt in row] + bias):
            ready = [t for t, cts in enumerate(X) if self._pc_operands_ok(cts, [])]
        step = getattr(self.backend, "pc_matmul_max_outputs", k_out)
        while ready:
            g = next((k for k in sizes if k <= len(ready)), None)
            if g is None:
                break
            group, ready = ready[:g], ready[g:]
            parts = [self._pc_matmul_batch_native(W[o0:o0 + step], [X[t] for t in group], bias[o0:o0 + step], l, d, planes=planes)
                     for o0 in range(0, k_out, step)]
            for j, t in enumerate(group):
                out[t] = [o for part in parts for o in part[j]]
        for t, cts in enumerate(X):
            if out[t] is None:
                out[t] = self.pc_matmul(W, cts, bias)
        return out

    def _pc_matmul_batch_native(self, W, toks, bias, l, d, planes=False):
        """One lf_pc_matmul_batch call, or (planes: every plaintext of W compact) one lf_pc_matmul_batch_planes call, of any nt >= 1."""
        return self._pc_matmul_call("pc_matmul_batch_planes_call" if planes else "pc_matmul_batch_native", W, toks, bias, l, d)

    # backend entry -> (its workspace query, the key its workspace is cached under, whether it takes the number of tokens)
    _pc_matmul_entries = {"pc_matmul_native": ("pc_matmul_ws_words", "pc_matmul_ws", False),
                          "pc_matmul_batch_native": ("pc_matmul_batch_ws_words", "pc_matmul_batch_ws", True),
                          "pc_matmul_batch_planes_call": ("pc_matmul_batch_planes_ws_words", "pc_matmul_batch_ws", True)}

    def _pc_matmul_call(self, entry, W, toks, bias, l, d):
        """ONE call of the backend's `entry` on the matrix W, the token vectors toks (exactly one where the entry takes no number of
        tokens) and the biases: the lists of output ciphertexts, one per token."""
        N, k_out, k_in = self.ctx.N, len(W), len(toks[0])
        ws_words, ws_key, batched = self._pc_matmul_entries[entry]
        nt = (len(toks),) if batched else ()
        rows = len(self.ntt.p.destination_arrays[l][d])          # the dropped limb first
        owner = self.ntt.p.rescaler_loc[l]
        round_at = self.ctx.q[self.ntt.p.destination_arrays[l][owner][0]] // 2
        ins, pts = (ctypes.c_void_p * (len(toks) * 2 * k_in))(), (ctypes.c_void_p * (k_out * k_in))()
        for t, cts in enumerate(toks):
            for i, ct in enumerate(cts):
                for comp in range(2):
                    ins[(t * k_in + i) * 2 + comp] = ct.data[comp][0].data_ptr()
        for o, row in enumerate(W):
            for i, pt in enumerate(row):
                pts[o * k_in + i] = None if pt is None else pt.data[0].data_ptr()
        biases = None
        if any(b is not None for b in bias):
            biases = (ctypes.c_void_p * k_out)()
            for o, b in enumerate(bias):
                biases[o] = None if b is None else b.data[0].data_ptr()
        dev = self.ntt.devices[d]
        ident = self._pc_identity(l, d)
        chunk = min(k_in, self.backend.pc_matmul_chunk)
        ws = self._ws(ws_key, (getattr(self.backend, ws_words)(*nt, chunk, k_out, rows, self.ctx.logN),), d)   # (per device and level: the shape)
        outs = [[[torch.empty((rows - 1, N), dtype=torch.int64, device=dev) for _ in range(2)] for _ in range(k_out)] for _ in toks]
        getattr(self.backend, entry)(ins, pts, biases, outs if batched else outs[0], *nt, k_in, k_out, rows, self.ctx.logN,
                                     self._tw(d, l, False), self._tw(d, l, False, True), self._vec("Rs", d, l, False),
                                     self._vec("Ninv", d, l, False), ident[0], ident[1], self.rescale_scales[l][d], round_at, ws,
                                     self._consts(d, l, False))
        return [[self._new(([o[0]], [o[1]]), types.origins["ct"], level=l + 1) for o in tok] for tok in outs]

    def _pc_identity(self, l, d):
        """The identity the forward transform's rescale step is handed (include/ckks_hip.h: lf_pc_dot): R mod q per row, a row of zeros."""
        key = ("pc_dot_identity", l, d)
        ident = self._tables.get(key)
        if ident is None:
            zero = self._tables.get(("zero_row", d))
            if zero is None:
                zero = self._tables[("zero_row", d)] = torch.zeros(self.ctx.N, dtype=torch.int64, device=self.ntt.devices[d])
            ident = self._tables[key] = (self._row_scalars(1, l, True)[self._loc(l).index(d)], zero)
        return ident

    def _pc_dot_native(self, pairs, bias, l, d):
        N, k = self.ctx.N, len(pairs)
        rows = len(self.ntt.p.destination_arrays[l][d])          # the dropped limb first
        owner = self.ntt.p.rescaler_loc[l]
        round_at = self.ctx.q[self.ntt.p.destination_arrays[l][owner][0]] // 2
        ins, pts = (ctypes.c_void_p * (2 * k))(), (ctypes.c_void_p * k)()
        for t, (pt, ct) in enumerate(pairs):
            pts[t] = pt.data[0].data_ptr()
            for comp in range(2):
                ins[2 * t + comp] = ct.data[comp][0].data_ptr()
        dev = self.ntt.devices[d]
        ident = self._pc_identity(l, d)
        ws = self._ws("pc_dot_ws", (self.backend.pc_dot_ws_words(min(k, 4), rows, self.ctx.logN),), d)   # (per device and level: the shape)
        out = [torch.empty((rows - 1, N), dtype=torch.int64, device=dev) for _ in range(2)]
        self.backend.pc_dot_native(ins, pts, None if bias is None else bias.data[0], out, k, rows, self.ctx.logN,
                                   self._tw(d, l, False), self._tw(d, l, False, True), self._vec("Rs", d, l, False),
                                   self._vec("Ninv", d, l, False), ident[0], ident[1], self.rescale_scales[l][d], round_at, ws,
                                   self._consts(d, l, False))
        return self._new(([out[0]], [out[1]]), types.origins["ct"], level=l + 1)
