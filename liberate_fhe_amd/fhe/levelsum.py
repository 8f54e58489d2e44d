"""level_sum, level_sum_batch and level_up_batch, mixed into `ckks_engine`: sums of ciphertexts that stand at DIFFERENT levels —
a residual connection, a skip addition, the corrections of a Chebyshev recurrence, the closing addition of a polynomial
evaluation — and the glue between the engine's fused products:

    level_sum(terms, const, level)  = sum_t s_t * (ct_t brought to level L) (+ const)
    level_up_batch(cts, L)          = [level_up(ct, L) for ct in cts]

The reference has level_up, mult_int_scalar, cc_add and add_scalar as chains of element-wise launches, each a trip through HBM,
and level_up computes a whole rescale of which only the rows of the target level are kept.  Like the engine's other options
beyond the reference, the words are DEFINED as a composition of those public ops (written out in level_sum's docstring), and that
composition is what runs wherever the native call (lf_level_sum) does not apply.  Natively ONE launch reads every surviving
input word once and writes every output word once, for both components of up to backend.lsum_max_sets sums.  DESIGN.md §4.2.
"""
from __future__ import annotations

import operator

import numpy as np
import torch

from .evaluator import is_struct
from .presets import errors, types


class LevelSumOps:
    # native shapes: every shape measured so far is at least as fast as its composition; a shape that is not
    # would be listed here and take the composition
    level_sum_native = True

    def _level_sum_checked(self, terms, level, what):
        """[(ct, int weight)] and the target level of one set, or the refusal: nothing has run when this raises."""
        terms = list(terms)
        if not terms:
            raise ValueError(f"{what}: at least one term")
        out = []
        for term in terms:
            if not isinstance(term, (tuple, list)) or len(term) != 2:
                raise ValueError(f"{what}: terms are (ciphertext, integer) pairs")
            ct, s = term
            if not is_struct(ct) or ct.origin != types.origins["ct"]:
                raise errors.NotMatchType(origin=getattr(ct, "origin", type(ct).__name__), to=types.origins["ct"])
            if ct.ntt_state or ct.montgomery_state or ct.include_special:
                raise errors.NotMatchDataStructState(origin=ct.origin)
            s = operator.index(s)
            if s == 0:
                raise ValueError(f"{what}: a zero weight (leave the term out)")
            out.append((ct, s))
        L = max(ct.level for ct, _ in out) if level is None else operator.index(level)
        if L >= self.num_levels:
            raise ValueError(f"{what}: level {L} is beyond the last level {self.num_levels - 1}")
        for ct, _ in out:
            if ct.level > L:
                raise ValueError(f"{what}: a term at level {ct.level} is deeper than the target level {L}")
        if len(out) == 1 and out[0][1] == 1 and out[0][0].level == L:
            raise ValueError(f"{what}: one term of weight 1 at the target level is a copy (clone, or add_scalar)")
        return out, L

    def _level_sum_composed(self, terms, const, L):
        acc = None
        for ct, s in terms:
            if ct.level != L and not all(t.is_contiguous() for comp in ct.data for t in comp):
                # (rescale takes a raw pointer and a row pitch of N: a strided operand is copied first — the same words)
                ct = ct._replace(data=[[t.contiguous() for t in comp] for comp in ct.data])
            u = ct if ct.level == L else self.level_up(ct, L)
            v = u if s == 1 else self.mult_int_scalar(u, s)
            acc = v if acc is None else self.cc_add(acc, v)
        return acc if const is None else self.add_scalar(acc, const)

    def _level_sum_device(self, terms, L):
        """The device the native call of this set runs on, or None: the composition."""
        be = self.backend
        if not self.level_sum_native or not hasattr(be, "level_sum_call") or not 13 <= self.ctx.logN <= 17:
            return None
        d = self._native_level(L)
        if d is None or len(terms) > be.lsum_max_terms or max(self.ctx.q) >= (1 << 60):
            return None
        dest = self.ntt.p.destination_arrays
        rows = len(dest[L][d])
        for ct, _ in terms:
            l = ct.level
            # (the dropped limb first and the survivors behind it, in the target level's order; 16-byte loads)
            if self._native_level(l) != d or list(dest[l][d][L - l:]) != list(dest[L][d]) or \
                    (l < L and self.ntt.p.rescaler_loc[l] != d):
                return None
            for comp in range(2):
                if len(ct.data[comp]) != 1:
                    return None
                t = ct.data[comp][0]
                if not (t.is_contiguous() and t.dtype == torch.int64 and t.data_ptr() % 16 == 0 and t.dim() == 2
                        and t.size(0) == rows + L - l and t.size(1) == self.ctx.N):
                    return None
        return d

    def _level_sum_table(self, terms, L, d):
        """[k, rows] device table of s_t R^2 (a term at L) or s_t delta_t R^2 (a levelled one) mod each prime of level L: kept per
        (level, levels and weights of the terms), the least recently used of 256 dropped — a copy from pageable host memory
        blocks the host, and the same few shapes (level_up from l, a Chebyshev correction) come back with every evaluation."""
        cache = self._lsum_tables
        key = (L, d, tuple((ct.level, s) for ct, s in terms))
        hit = cache.get(key)
        if hit is not None:
            cache.move_to_end(key)
            return hit
        q, R2 = self.ctx.q, self.ctx.R * self.ctx.R
        primes = self.ntt.p.destination_arrays[L][d]
        rows = []
        for ct, s in terms:
            f = s * R2
            if ct.level < L:     # level_up's integer
                f *= round(self.scale * (self.deviations[L] / np.sqrt(self.deviations[ct.level + 1])))
            rows.append([f % q[i] for i in primes])
        hit = cache[key] = self._t64(rows, d)
        if len(cache) > 256:
            self._retire([cache.popitem(last=False)[1]], d)
        return hit

    def _level_sum_native(self, group, L, d):
        """One native call for up to backend.lsum_max_sets checked sets [(terms, const)] of target level L on device d."""
        N, q = self.ctx.N, self.ctx.q
        rows = len(self.ntt.p.destination_arrays[L][d])
        dev = self.ntt.devices[d]
        self._same_stream(d)
        sets, outs = [], []
        for terms, const in group:
            entries = []
            for ct, _ in terms:
                l = ct.level
                if l == L:
                    entries.append((ct.data[0][0], ct.data[1][0], 0, None, 0))
                else:
                    round_at = q[self.ntt.p.destination_arrays[l][d][0]] // 2
                    entries.append((ct.data[0][0], ct.data[1][0], L - l, self.rescale_scales[l][d], round_at))
            cst = None if const is None else self._row_scalars(self._add_scalar_int(const, L), L, False)[self._loc(L).index(d)]
            sets.append((entries, self._level_sum_table(terms, L, d), cst))
            # (one allocation per component, as rescale makes them: an output kept alive pins no other)
            outs.append([torch.empty((rows, N), dtype=torch.int64, device=dev) for _ in range(2)])
        self.backend.level_sum_call(sets, outs, rows, self.ctx.logN, self._consts(d, L, False))
        return [self._new(([o[0]], [o[1]]), types.origins["ct"], level=L) for o in outs]

    def level_sum_batch(self, sets, level=None) -> list:
        """[level_sum(terms, const, level) for terms, const in sets], word for word and in order; the sets whose target level
        lives on one device share native calls of up to backend.lsum_max_sets sets of ONE target level each, the others take the
        composition one by one.  The same object may appear any number of times, in one set or across sets.  Refused as a whole,
        before any work, where any member would be."""
        self._enter()
        checked = []
        for entry in list(sets):
            if not isinstance(entry, (tuple, list)) or len(entry) != 2:
                raise ValueError("level_sum_batch: sets are (terms, const) pairs")
            terms, L = self._level_sum_checked(entry[0], level, "level_sum")
            checked.append((terms, entry[1], L))
        out = [None] * len(checked)
        groups = {}
        for i, (terms, const, L) in enumerate(checked):
            d = self._level_sum_device(terms, L)
            if d is None:
                out[i] = self._level_sum_composed(terms, const, L)
            else:
                groups.setdefault((L, d), []).append(i)
        cap = getattr(self.backend, "lsum_max_sets", 1)
        for (L, d), idx in groups.items():
            for i0 in range(0, len(idx), cap):
                part = idx[i0:i0 + cap]
                for i, ct in zip(part, self._level_sum_native([checked[i][:2] for i in part], L, d)):
                    out[i] = ct
        return out

    def level_sum(self, terms, const=None, level=None):
        """sum_t s_t * ct_t (+ const) as ONE ciphertext at level L = `level`, or the deepest level among the terms: terms is a
        list of (ct, s), each ct a coefficient-domain ciphertext without special limbs at a level <= L, each s a non-zero Python
        int of any size (only its residues count); const a number, added as add_scalar adds it.  The words are those of
            u_t = ct_t                      if ct_t.level == L   else level_up(ct_t, L)
            v_t = u_t                       if s_t == 1          else mult_int_scalar(u_t, s_t)
            acc = v_0;  acc = cc_add(acc, v_t)  for t = 1 .. k-1
            out = acc                       if const is None     else add_scalar(acc, const)
        which is also what runs where the native call does not apply: several devices or ranks, logN outside 13..17, a checker
        backend, non-contiguous operands, more than backend.lsum_max_terms terms, a prime of 2^60 or more.  Otherwise ONE native
        call (lf_level_sum).  ValueError for no term, a zero weight, a term deeper than L, an L beyond the last level, and for a
        single term of weight 1 already at L (a copy: clone, or add_scalar); the type and state refusals are level_up's and
        cc_add's; all of them before any work."""
        return self.level_sum_batch([(terms, const)], level)[0]

    def level_up_batch(self, cts, dst_level) -> list:
        """[level_up(ct, dst_level) for ct in cts], word for word and in order: every member shallower than dst_level
        (ValueError otherwise, for the whole list); level_sum_batch of one term of weight 1 each."""
        cts = list(cts)
        for ct in cts:
            if is_struct(ct) and ct.origin == types.origins["ct"] and ct.level >= operator.index(dst_level):
                raise ValueError(f"level_up_batch: a member at level {ct.level} is not shallower than level {dst_level}")
        return self.level_sum_batch([([(ct, 1)], None) for ct in cts], dst_level)

    def _level_up_native(self, ct, dst_level):
        """level_up as one native call (one term of weight 1), or None: the reference's chain."""
        if not (isinstance(dst_level, (int, np.integer)) and ct.level < dst_level < self.num_levels) \
                or ct.ntt_state or ct.montgomery_state or ct.include_special:
            return None
        terms = [(ct, 1)]
        d = self._level_sum_device(terms, int(dst_level))
        if d is None:
            return None
        self._enter()
        return self._level_sum_native([(terms, None)], int(dst_level), d)[0]
