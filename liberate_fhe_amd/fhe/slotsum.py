"""rotate_sum and inner_sum, mixed into `ckks_engine`: sums over slots — the step behind a dot product, a row sum, a mean,
pooling, or the replication of one value over a block:

    rotate_sum(ct, keys)      = sum_k rot_k(ct) (+ ct)
    inner_sum(ct, n, stride)  = sum_{j < n} rot(ct, j * stride)

A rotation is a key switch, and everything of a key switch behind the inner product with the key — the inverse NTT and the
mod-down — is linear.  So the key-switch sums of several rotations of ONE ciphertext are added while still in the NTT domain
over Q P and brought down once, and the digits of c1 in front are formed, extended and transformed once (rotate_hoisted's shared
half): per rotation only the gathered inner product with its key remains.  It is linear_transform without the diagonals, and so
without the rescale: the level stays.  inner_sum chains such sums over the mixed-radix stages of n (encdec.inner_sum_plan).
Like the engine's other options beyond the reference, the words are DEFINED as a composition of steps the engine already has
(written out in rotate_sum's docstring), and that composition is what runs wherever the native call (lf_rotate_sum) does not
apply.  rotate_sum_batch / inner_sum_batch are the same sums over a list of ciphertexts under ONE key set, with exactly the
loop's words: groups of ciphertexts share every launch of one native call (lf_rotate_sum_batch), which reads each key word once
per group.  DESIGN.md §4.2.
"""
from __future__ import annotations

import torch

from . import encdec
from .data_struct import data_struct
from .evaluator import is_struct
from .presets import errors, types


class SlotSumOps:
    def rotate_sum(self, ct: data_struct, keys: list, include_self: bool = True) -> data_struct:
        """sum over `keys` of the rotation (or conjugation) of ct under that key, plus ct itself with include_self, as ONE
        ciphertext at ct.level: decrypts to sum_k np.roll(m, step_k) (+ m) (rotate_single's direction).  keys: a list of
        rotation keys — a key may repeat, a step-0 key is legal — and / or conjugation keys: rotate_sum(ct, [conjk]) is
        2 Re(m) in one key switch.  Addition commutes with the mod-down, so the key-switch sums are added in the NTT domain over
        Q P and brought down once.  The words are those of: c0, c1 made canonical; E = per part pre_extend(c1) -> extend -> exact
        forward NTT (rotate_hoisted's shared half); c^ = P * enter_ntt(c) on the ordinary rows; per key t_c = sum over the parts
        of E gathered by pi_p times the key part, t_0 += c^0 gathered by pi_p on the ordinary rows; the self term t_c = c^c, zero
        on the special rows; S_c = sum of the t_c; intt_exit_reduce, mod-down without addend.  No rescale.  One native call
        (lf_rotate_sum) where every limb of the level is on one device of this process; otherwise the same words through the
        engine's steps.  Coefficient-domain ciphertexts without special limbs only."""
        self._enter()
        if ct.origin != types.origins["ct"]:
            raise errors.NotMatchType(origin=ct.origin, to=types.origins["ct"])
        keys = list(keys)
        N, logN = self.ctx.N, self.ctx.logN
        exps = []
        for k in keys:
            origin = k.origin if is_struct(k) else type(k).__name__
            if types.origins["rotk"] in origin:
                exps.append(encdec.galois_exponent(N, int(origin.split(":")[-1])))
            elif origin == types.origins["conjk"]:
                exps.append(encdec.conjugation_exponent(N))
            else:
                raise errors.NotMatchType(origin=origin, to=types.origins["rotk"])
        if not keys and not include_self:
            raise ValueError("rotate_sum: no key and no self term: nothing to sum")
        if ct.ntt_state or ct.include_special:
            raise NotImplementedError("rotate_sum: coefficient-domain ciphertexts without special limbs only")
        level = ct.level

        d = self._native_level(level)
        if d is not None and hasattr(self.backend, "rotate_sum_native") and \
                ct.data[0][0].is_contiguous() and ct.data[1][0].is_contiguous():
            plan, _, first_part, row_off = self._op_plan(level, d)
            i0 = self._loc(0, special=True).index(d)
            words = self.backend.rotate_sum_ws_words(plan)
            ws = self._ws("rsum_ws", (words,), d) if words else None
            out = torch.empty((2, plan.ell, N), dtype=torch.int64, device=self.ntt.devices[d])
            self.backend.rotate_sum_native(plan, ct.data[0][0], ct.data[1][0], exps, [self._key_pack(k)[i0] for k in keys],
                                           first_part, row_off, include_self, out, ws)
            return self._new(([out[0]], [out[1]]), types.origins["ct"], level=level, montgomery_state=ct.montgomery_state)

        # orchestrated: the same words through the engine's steps, as linear_transform composes them without the diagonal
        # products and the rescale.  Digits of c1 and their exchange once, extension + forward NTT once per device, c^ per device on
        # its own rows; per key the gather, the key's inner product (through the fused tail where the key pack is in the planes
        # format: its inverse NTT is undone by an exact forward one — the same residues), mont_add into the one pair; ONE inverse
        # NTT and mod-down per device
        tabs = self._ks_tables(level)
        loc, loc0 = self._loc(level), self._loc(0, special=True)
        K, n = self.ntt.num_special_primes, self.ntt
        nparts = len(tabs["order"])
        fused = logN >= self.backend.fused_ks_min_logN
        gather = getattr(self.backend, "ks_gather", None)
        c1 = [t if t.is_contiguous() else t.contiguous() for t in ct.data[1]]   # (the digit kernels take a raw pointer and a row pitch of N)
        digits = self._ks_digits_exchanged(c1, level, galois=(1, True)) if keys else {}
        c0o, c1o = [], []
        for i, d in enumerate(loc):
            li = self.local_ids.index(d)
            rows, ell = self._rows(d, level, True), self._rows(d, level, False)
            cs, cso = self._consts(d, level, True), self._consts(d, level, False)
            tw, itw, ninv = self._tw(d, level, True), self._tw(d, level, True, True), self._vec("Ninv", d, level, True)
            _2q = [n._2q_prepack[-2][level][0][li]]
            g2q = self._vec("_2q", d, level, False)
            dev = self.ntt.devices[d]
            # c^0, c^1 = P * enter_ntt(canonical c) on the ordinary rows (c^1 serves the self term alone)
            chat = torch.empty((2, ell, N), dtype=torch.int64, device=dev)
            for comp in range(2 if include_self else 1):
                src = ct.data[comp][i] if ct.data[comp][i].is_contiguous() else ct.data[comp][i].contiguous()
                self.backend.galois(src, chat[comp], ell, logN, 1, g2q)
                self.backend.ntt(chat[comp], 1, ell, logN, self._tw(d, level, False), self._vec("Rs", d, level, False), cso)
                n.ops.mont_enter([chat[comp]], [self._PR(d, level)], *[x[li:li + 1] for x in n.mont_prepack[-1][level][0]])
            S = None
            if include_self:
                S = torch.zeros((2, rows, N), dtype=torch.int64, device=dev)
                S[:, :ell] = chat
            if keys:
                desc, E, Ed = tabs[("extend", d)]
                ext = self._ws("ks_ext", (nparts, rows, N), d)
                dig, ready = digits[d]
                for handle, first, count in ready:
                    if handle is not None:
                        handle.wait()
                    if fused:
                        self.backend.ks_fwd(dig, first, count, rows, logN, desc, E, Ed, ext, tw, cs)
                if not fused:
                    self.backend.ks_extend(dig, ext, nparts, rows, desc, E, cs)
                    self.backend.ntt(ext, nparts, rows, logN, tw, None, cs, relaxed=True)
                src = self._ws("ks_ext_hoisted", (nparts, rows, N), d)   # (see rotate_hoisted: `ext` receives each key's gather)
                src.copy_(ext)
                s = self._ws("ks_sum", (2, rows, N), d)
                Rs = self._vec("Rs", d, level, True)
                for key, p in zip(keys, exps):
                    idx = self._galois_index(p, d)
                    if gather is not None:
                        gather(src, ext, idx, rows, logN, cs)
                    else:
                        torch.index_select(src, 2, idx, out=ext)
                    kp = self._key_pack(key)[loc0.index(d)]
                    if fused:
                        self.backend.ks_tail(nparts, rows, logN, kp, tabs["first_part"], self.ntt.starts[level][d], ext, s, itw, ninv, cs)
                        self.backend.ntt(s, 2, rows, logN, tw, Rs, cs)     # back into the NTT domain, Montgomery form
                    else:
                        self.backend.ks_inner(ext, kp, tabs["first_part"], self.ntt.starts[level][d], s[0], s[1], nparts, rows, cs)
                    t = s.clone()
                    t[0, :ell] = n.ops.mont_add([t[0, :ell]], [chat[0].index_select(1, idx)], [_2q[0][:ell]])[0]
                    S = t if S is None else torch.stack([n.ops.mont_add([S[comp]], [t[comp]], _2q)[0] for comp in range(2)])
            s2 = S.contiguous()
            self.backend.intt(s2, 2, rows, logN, itw, ninv, 2, cs)         # intt_exit_reduce: canonical coefficients
            out = torch.empty((2, ell, N), dtype=torch.int64, device=dev)
            ws, one = self._moddown_ws("ks_moddown", 2, ell, K, d, tabs, cs)
            mkw = {"one_launch": True} if one else {}
            self.backend.ks_moddown_ws([s2[0], s2[1]], [out[0], out[1]], [None, None], ell, K, ws, tabs[("pir", d)],
                                       self._vec("Rs", d, level, True), cs, PiP=tabs[("pip", d)], **mkw)
            c0o.append(out[0]); c1o.append(out[1])
        return self._new((c0o, c1o), types.origins["ct"], level=level, montgomery_state=ct.montgomery_state)

    # group sizes of rotate_sum_batch's native path, largest first (a subset of backend.ks_batch_sizes that starts at its
    # largest: lf_rotate_sum_batch itself takes 4, then 2), as lt_batch_sizes: a size that does not beat the loop is left out
    # here and its ciphertexts take rotate_sum one by one — the words are the same (DESIGN.md §4.2 has the numbers)
    rsum_batch_sizes = (4, 2)

    def rotate_sum_batch(self, cts: list, keys: list, include_self: bool = True) -> list:
        """rotate_sum of many ciphertexts under the SAME keys: returns exactly [rotate_sum(ct, keys, include_self) for ct in cts],
        word for word and in order (the words are rotate_sum's own; a ciphertext may appear several times; an empty list gives
        []).  keys: as rotate_sum takes them.  What rotate_sum refuses is refused here for the whole list before anything is
        allocated or launched: a wrong origin, a wrong key type, no key and no self term, an NTT-domain or special-limb
        ciphertext.  Ciphertexts of different levels are legal: they are bucketed by level and every output keeps its place.
        Where rotate_sum's native call applies (every limb of the level on one device of this process, a backend with
        lf_rotate_sum_batch, contiguous operands) groups of rsum_batch_sizes ciphertexts of one level go through ONE native
        call of at most backend.lt_batch_max_cts ciphertexts: a group shares every launch, and its inner product — nearly all
        of the op — reads each key word once per group instead of once per ciphertext, looping over the keys inside the
        kernel (ks_inner_rsumb_kernel) with one accumulator pair per ciphertext.  Ciphertexts that do not qualify, the one left
        over by the groups, and every ciphertext on a backend without the entry take rotate_sum one by one."""
        self._enter()
        cts = list(cts)
        if not cts:
            return []
        for ct in cts:
            if not is_struct(ct) or ct.origin != types.origins["ct"]:
                raise errors.NotMatchType(origin=getattr(ct, "origin", type(ct).__name__), to=types.origins["ct"])
        keys = list(keys)
        N = self.ctx.N
        exps = []
        for k in keys:
            origin = k.origin if is_struct(k) else type(k).__name__
            if types.origins["rotk"] in origin:
                exps.append(encdec.galois_exponent(N, int(origin.split(":")[-1])))
            elif origin == types.origins["conjk"]:
                exps.append(encdec.conjugation_exponent(N))
            else:
                raise errors.NotMatchType(origin=origin, to=types.origins["rotk"])
        if not keys and not include_self:
            raise ValueError("rotate_sum_batch: no key and no self term: nothing to sum")
        for ct in cts:
            if ct.ntt_state or ct.include_special:
                raise NotImplementedError("rotate_sum_batch: coefficient-domain ciphertexts without special limbs only")
        out = [None] * len(cts)
        sizes = [k for k in self.rsum_batch_sizes if k in getattr(self.backend, "ks_batch_sizes", ())]
        by_level = {}
        for i, ct in enumerate(cts):
            by_level.setdefault(ct.level, []).append(i)
        for level, members in by_level.items():
            d = self._native_level(level)
            if d is None or not sizes or not hasattr(self.backend, "rotate_sum_batch_native"):
                continue
            ready = [i for i in members if cts[i].data[0][0].is_contiguous() and cts[i].data[1][0].is_contiguous()]
            native, pos = [], 0
            while True:
                n = next((k for k in sizes if k <= len(ready) - pos), 0)
                if not n:
                    break
                native += ready[pos:pos + n]
                pos += n
            if not native:
                continue
            plan, _, first_part, row_off = self._op_plan(level, d, nct=4)
            i0 = self._loc(0, special=True).index(d)
            kpacks = [self._key_pack(k)[i0] for k in keys]
            cap = self.backend.lt_batch_max_cts - self.backend.lt_batch_max_cts % max(sizes)
            for a in range(0, len(native), cap):
                idx = native[a:a + cap]
                words = self.backend.rotate_sum_batch_ws_words(plan, len(idx))
                ws = self._ws("rsum_batch_ws", (words,), d) if words else None
                outs = [torch.empty((2, plan.ell, N), dtype=torch.int64, device=self.ntt.devices[d]) for _ in idx]
                self.backend.rotate_sum_batch_native(plan, [cts[i].data[0][0] for i in idx], [cts[i].data[1][0] for i in idx], exps,
                                                     kpacks, first_part, row_off, include_self, outs, ws)
                for i, o in zip(idx, outs):
                    out[i] = self._new(([o[0]], [o[1]]), types.origins["ct"], level=level, montgomery_state=cts[i].montgomery_state)
        for i, ct in enumerate(cts):
            if out[i] is None:
                out[i] = self.rotate_sum(ct, keys, include_self)
        return out

    def inner_sum_batch(self, cts: list, n: int, rotks, stride: int = 1, radix: int = encdec.INNER_SUM_RADIX) -> list:
        """inner_sum of many ciphertexts under the SAME keys: returns exactly [inner_sum(ct, n, rotks, stride, radix) for ct in
        cts], word for word and in order.  It validates like inner_sum, for the whole list before anything runs, and then chains
        one rotate_sum_batch(.., include_self=True) per stage of encdec.inner_sum_plan, so every stage reads its keys once per
        group of ciphertexts (inner_sum_steps lists the steps a key is needed for).  An empty list gives []."""
        self._enter()
        cts = list(cts)
        if not cts:
            return []
        for ct in cts:
            if not is_struct(ct) or ct.origin != types.origins["ct"]:
                raise errors.NotMatchType(origin=getattr(ct, "origin", type(ct).__name__), to=types.origins["ct"])
        plan = encdec.inner_sum_plan(n, stride, self.num_slots, radix)
        by_step = {}
        for k in (list(rotks.values()) if isinstance(rotks, dict) else list(rotks)):
            if not is_struct(k) or types.origins["rotk"] not in k.origin:
                raise errors.NotMatchType(origin=getattr(k, "origin", type(k).__name__), to=types.origins["rotk"])
            by_step.setdefault(int(k.origin.split(":")[-1]) % self.num_slots, k)
        for _, steps in plan:
            for s in steps:
                if s not in by_step:
                    raise errors.NotMatchType(origin=f"no key for step {s}", to=types.origins["rotk"] + str(s))
        for ct in cts:
            if ct.ntt_state or ct.include_special:
                raise NotImplementedError("inner_sum_batch: coefficient-domain ciphertexts without special limbs only")
        for _, steps in plan:
            cts = self.rotate_sum_batch(cts, [by_step[s] for s in steps], include_self=True)
        return cts

    def inner_sum_steps(self, n: int, stride: int = 1, radix: int = encdec.INNER_SUM_RADIX) -> list:
        """The sorted distinct steps inner_sum(ct, n, .., stride, radix) needs a rotation key for."""
        return sorted({s for _, steps in encdec.inner_sum_plan(n, stride, self.num_slots, radix) for s in steps})

    def inner_sum(self, ct: data_struct, n: int, rotks, stride: int = 1, radix: int = encdec.INNER_SUM_RADIX) -> data_struct:
        """The sum of n copies of ct rotated by 0, stride, .., (n - 1) stride, at ct.level: slot i of the result holds
        sum_{j < n} m[(i - j stride) mod num_slots], i.e. sum_j np.roll(m, j * stride) (rotate_single's direction).  A negative
        stride sums the other way (the replication of one value over a block).  n = r_1 r_2 .. r_m (encdec.inner_sum_plan): one
        rotate_sum(.., include_self=True) per stage, chained — a radix-r stage adds r shifted copies for r - 1 gathered inner
        products and ONE set of digits, inverse NTT and mod-down; radix=2 is the classic log fold in hoisted words.  rotks: a
        list or mapping of rotation keys, looked up by the step in their origin (inner_sum_steps lists the steps needed)."""
        self._enter()
        if ct.origin != types.origins["ct"]:
            raise errors.NotMatchType(origin=ct.origin, to=types.origins["ct"])
        plan = encdec.inner_sum_plan(n, stride, self.num_slots, radix)
        by_step = {}
        for k in (list(rotks.values()) if isinstance(rotks, dict) else list(rotks)):
            if not is_struct(k) or types.origins["rotk"] not in k.origin:
                raise errors.NotMatchType(origin=getattr(k, "origin", type(k).__name__), to=types.origins["rotk"])
            by_step.setdefault(int(k.origin.split(":")[-1]) % self.num_slots, k)
        for _, steps in plan:
            for s in steps:
                if s not in by_step:
                    raise errors.NotMatchType(origin=f"no key for step {s}", to=types.origins["rotk"] + str(s))
        if ct.ntt_state or ct.include_special:
            raise NotImplementedError("inner_sum: coefficient-domain ciphertexts without special limbs only")
        for _, steps in plan:
            ct = self.rotate_sum(ct, [by_step[s] for s in steps], include_self=True)
        return ct
