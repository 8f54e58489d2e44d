"""Polynomial evaluation on a ciphertext, mixed into `ckks_engine`: several weighted sums of the same ciphertexts under one
rescale (one native call, lf_weighted_sums, where a level lives on one device) and Paterson-Stockmeyer evaluation in the power
and the Chebyshev basis on top of it, of cc_mult_batch and of cc_dot.  The reference has none of these; like the engine's other
options beyond it, their words are DEFINED as compositions of ops the engine already has (written out in the docstrings), and
that composition is what runs wherever the native call does not apply.  DESIGN.md §4.2.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import encdec
from .evaluator import is_struct
from .presets import errors, types


class PolyOps:
    # =============================================================================================
    # weighted sums under one rescale
    # =============================================================================================
    def _check_sum_operands(self, cts, what):
        if not cts:
            raise ValueError(f"{what}: at least one ciphertext")
        for ct in cts:
            if not is_struct(ct) or ct.origin != types.origins["ct"]:
                raise errors.NotMatchType(origin=getattr(ct, "origin", type(ct).__name__), to=types.origins["ct"])
        l = cts[0].level
        for ct in cts:
            if ct.level != l:
                raise errors.NotMatchDataStructState(origin=f"{ct.origin} at level {ct.level} beside level {l}")
            if ct.ntt_state or ct.include_special:
                raise errors.NotMatchDataStructState(origin=ct.origin)
        if l + 1 >= self.num_levels:
            raise errors.MaximumLevelError(level=l, level_max=self.num_levels)
        return l

    def weighted_sums(self, cts: list, weights, consts=None) -> list:
        """[rescale(sum_t weights[g][t] * cts[t]) + consts[g] for g]: G ciphertexts at level + 1 from k ciphertexts of one level
        (coefficient domain, no special limbs; the same object may repeat) — the baby-step sums of a polynomial evaluation, all
        of them under ONE rescale.  The words of output g are those of
            s_t = int(weights[g][t] * scale * sqrt(deviations[level + 1]) + 0.5)              (mult_scalar's integer)
            acc = _scale_rows(cts[0], _row_scalars(s_0, level, True))
            acc = cc_add(acc, _scale_rows(cts[t], _row_scalars(s_t, level, True)))  for t >= 1
            out = rescale(acc);  out = add_scalar(out, consts[g])  if consts is given
        (zero weights are ordinary terms; one term without a const is mult_scalar), which is also what runs where the native
        call does not apply: several devices or ranks, logN outside 13..17, a checker backend, non-contiguous operands, more than
        backend.wsum_max_terms terms, a prime of 2^60 or more.  Otherwise ONE native call (lf_weighted_sums)."""
        cts = list(cts)
        l = self._check_sum_operands(cts, "weighted_sums")
        w = np.asarray(weights, dtype=np.float64)
        if w.ndim != 2 or w.shape[0] < 1 or w.shape[1] != len(cts):
            raise ValueError(f"weighted_sums: weights must be G x {len(cts)}, got shape {w.shape}")
        if consts is not None:
            consts = np.asarray(consts, dtype=np.float64)
            if consts.shape != (w.shape[0],):
                raise ValueError(f"weighted_sums: consts must hold {w.shape[0]} numbers, got shape {consts.shape}")
        ints = [[int(x * self.scale * np.sqrt(self.deviations[l + 1]) + 0.5) for x in row] for row in w]   # as mult_scalar writes it
        cint = None if consts is None else [self._add_scalar_int(c, l + 1) for c in consts]
        return self._weighted_sums_int(cts, ints, cint)

    def weighted_sum(self, cts: list, weights, const=None):
        """weighted_sums for one row of weights: one ciphertext."""
        return self.weighted_sums(cts, [list(weights)], None if const is None else [const])[0]

    def _weighted_sums_int(self, cts, int_matrix, const_ints=None) -> list:
        """weighted_sums on the Python integers themselves: int_matrix[g][t] multiplies cts[t] (any sign and size: only its
        residues count), const_ints[g] is added to coefficient 0 of c0 after the rescale (the integer add_scalar forms)."""
        self._enter()
        cts = list(cts)
        l = self._check_sum_operands(cts, "weighted_sums")
        k, G = len(cts), len(int_matrix)
        if G < 1 or any(len(row) != k for row in int_matrix) or (const_ints is not None and len(const_ints) != G):
            raise ValueError("weighted_sums: G rows of one integer per ciphertext, and G consts or none")
        int_matrix = [[int(s) for s in row] for row in int_matrix]
        const_ints = None if const_ints is None else [int(c) for c in const_ints]
        d = self._native_level(l + 1)
        be = self.backend
        # (16-byte loads: a contiguous view at an odd word offset takes the composition, as do rows in another order than the
        # dropped limb first and the survivors behind it)
        if d is not None and self._native_level(l) == d and hasattr(be, "weighted_sums_native") and self.ctx.logN <= 17 \
                and k <= be.wsum_max_terms and max(self.ctx.q) < (1 << 60) \
                and list(self.ntt.p.destination_arrays[l][d][1:]) == list(self.ntt.p.destination_arrays[l + 1][d]) \
                and all(t.is_contiguous() and t.dtype == torch.int64 and t.data_ptr() % 16 == 0
                        for ct in cts for t in (ct.data[0][0], ct.data[1][0])):
            return self._weighted_sums_native(cts, int_matrix, const_ints, l, d)
        outs = []
        for g in range(G):
            acc = None
            for ct, s in zip(cts, int_matrix[g]):
                term = self._scale_rows(ct, self._row_scalars(s, l, True))
                acc = term if acc is None else self.cc_add(acc, term)
            out = self.rescale(acc)
            if const_ints is not None:
                out = self._add_int_to_coefficient0(out, const_ints[g])
            outs.append(out)
        return outs

    def _weighted_sums_native(self, cts, int_matrix, const_ints, l, d):
        N, k, G = self.ctx.N, len(cts), len(int_matrix)
        q = self.ctx.q
        primes = self.ntt.p.destination_arrays[l][d]          # the dropped limb first
        rows = len(primes) - 1
        R2 = self.ctx.R * self.ctx.R
        owner = self.ntt.p.rescaler_loc[l]
        round_at = q[self.ntt.p.destination_arrays[l][owner][0]] // 2
        ins, row0s = (ctypes.c_void_p * (2 * k))(), (ctypes.c_void_p * (2 * k))()
        for t, ct in enumerate(cts):
            for comp in range(2):
                ptr = ct.data[comp][0].data_ptr()
                row0s[2 * t + comp], ins[2 * t + comp] = ptr, ptr + N * 8   # the dropped limb is the first row; the survivors follow it
        dev = self.ntt.devices[d]
        self._same_stream(d)
        results = []
        cap = self.backend.wsum_max_outputs
        for g0 in range(0, G, cap):
            part = int_matrix[g0:g0 + cap]
            cpart = None if const_ints is None else const_ints[g0:g0 + cap]
            # the device tables of these integers at this level: kept (the coefficients of an activation are evaluated again
            # and again; building them costs G k (l + 1) big-integer reductions on the host), the least recently used dropped
            cache = self._wsum_tables
            key = (l, d, tuple(map(tuple, part)), None if cpart is None else tuple(cpart))
            hit = cache.get(key)
            if hit is None:
                tab = self._t64([[[s * R2 % q[i] for i in primes] for s in row] for row in part], d)
                cst = None if cpart is None else self._t64([[c % q[i] for i in primes[1:]] for c in cpart], d)
                hit = cache[key] = (tab, cst)
                if len(cache) > 64:
                    self._retire(cache.popitem(last=False)[1], d)     # (today the blocking copy above has drained its readers)
            else:
                cache.move_to_end(key)
            tab, cst = hit
            # (one allocation per component, as rescale makes them: an output kept alive pins no other)
            out = [[torch.empty((rows, N), dtype=torch.int64, device=dev) for _ in range(2)] for _ in part]
            self.backend.weighted_sums_native(ins, row0s, [out[g][comp] for g in range(len(part)) for comp in range(2)], k, len(part),
                                              rows, self.ctx.logN, tab, cst, self.rescale_scales[l][d], round_at,
                                              self._consts(d, l, False))
            results += [self._new(([out[g][0]], [out[g][1]]), types.origins["ct"], level=l + 1) for g in range(len(part))]
        return results

    # =============================================================================================
    # Paterson-Stockmeyer polynomial evaluation
    # =============================================================================================
    def poly_depth(self, degree: int, basis: str = "power", interval=None, n1=None) -> int:
        """Levels poly_eval consumes for a polynomial of this degree (result level - operand level); the Chebyshev basis on
        an interval other than (-1, 1) spends one more, on the change of variable."""
        if basis not in ("power", "chebyshev"):
            raise ValueError(f"poly_eval: basis must be 'power' or 'chebyshev', got {basis!r}")
        n1 = encdec.poly_split(degree) if n1 is None else n1
        extra = 1 if basis == "chebyshev" and interval is not None and tuple(interval) != (-1, 1) else 0
        return encdec.poly_schedule(degree, n1)["depth"] + extra

    def _power_tree(self, powers: dict, top: int, evk, cheb: bool):
        """powers {1: p_1} -> every p_b, b <= top (x^b, or T_b with cheb), by the tree rule: p_{2^j} from p_{2^(j-1)}, any other
        b from p_hi and p_{b - hi} with hi the top power of two of b; the products of one hi share one cc_mult_batch."""
        hi = 1
        while 2 * hi <= top:
            sq = self.square(powers[hi], evk)
            powers[2 * hi] = self.level_sum([(sq, 2)], const=-1) if cheb else sq
            hi *= 2
        hi = 2
        while hi < top:
            los = [b - hi for b in range(hi + 1, min(2 * hi, top + 1))]
            if los:
                pairs = [self.auto_level(powers[hi], powers[lo]) for lo in los]
                prods = self.cc_mult_batch(pairs, evk) if len(pairs) > 1 else [self.cc_mult(pairs[0][0], pairs[0][1], evk)]
                for lo, p in zip(los, prods):
                    powers[hi + lo] = self.level_sum([(p, 2), (powers[hi - lo], -1)]) if cheb else p
            hi *= 2
        return powers

    def _at_level(self, cts, level):
        """[ct if ct.level == level else level_up(ct, level) for ct in cts]: the level_ups as ONE level_up_batch"""
        cts = list(cts)
        low = [i for i, ct in enumerate(cts) if ct.level != level]
        for i, up in zip(low, self.level_up_batch([cts[i] for i in low], level) if low else []):
            cts[i] = up
        return cts

    # The glue between the products goes through level_sum (levelsum.py), whose words are those of the chains the docstrings
    # below write out: add_scalar(mult_int_scalar(sq, 2), -1) = level_sum([(sq, 2)], const=-1);
    # auto_cc_sub(mult_int_scalar(prod, 2), p) = level_sum([(prod, 2), (p, -1)]) (prod stands deeper than p, and both forms leave
    # the canonical residue of 2 prod - level_up(p)); cc_add(r, level_up(q_0, L)) = level_sum([(r, 1), (q_0, 1)]).

    def _power_tree_batch(self, trees: list, top: int, evk, cheb: bool):
        """_power_tree on one dictionary per ciphertext, walked once: the squares of a step, and the products of one hi, of ALL
        ciphertexts share one cc_mult_batch (whose results are cc_mult's, bit for bit)."""
        hi = 1
        while 2 * hi <= top:
            sqs = self.cc_mult_batch([(t[hi], t[hi]) for t in trees], evk)
            if cheb:
                sqs = self.level_sum_batch([([(sq, 2)], -1) for sq in sqs])
            for t, sq in zip(trees, sqs):
                t[2 * hi] = sq
            hi *= 2
        hi = 2
        while hi < top:
            los = [b - hi for b in range(hi + 1, min(2 * hi, top + 1))]
            if los:
                prods = self.cc_mult_batch([self.auto_level(t[hi], t[lo]) for t in trees for lo in los], evk)
                if cheb:
                    prods = self.level_sum_batch([([(prods[i * len(los) + j], 2), (t[hi - lo], -1)], None)
                                                  for i, t in enumerate(trees) for j, lo in enumerate(los)])
                for i, t in enumerate(trees):
                    for j, lo in enumerate(los):
                        t[hi + lo] = prods[i * len(los) + j]
            hi *= 2
        return trees

    def poly_eval(self, ct, coeffs, evk, basis="power", interval=None, n1=None):
        """p(ct) for p = sum_i coeffs[i] x^i (basis="power") or sum_i coeffs[i] T_i((2x - a - b) / (b - a)) (basis="chebyshev",
        interval=(a, b), default (-1, 1)), degree d = len(coeffs) - 1 >= 1, by Paterson-Stockmeyer: with n1 a power of two
        (encdec.poly_split(d) unless given) and G = ceil((d + 1) / n1), p = sum_g q_g(x) y^g, y = x^n1 resp. T_n1.  The result,
        poly_depth(d, basis, interval, n1) levels above ct, has exactly the words of this composition of public ops:
          chebyshev, interval != (-1, 1):  x = add_scalar(mult_scalar(ct, 2 / (b - a)), -(a + b) / (b - a))
          babies p_b, b < n1:  p_1 = x;  power: p_2h = square(p_h), other b: auto_cc_mult(p_hi, p_{b - hi}), hi the top power of two
              of b;  chebyshev: p_2h = add_scalar(mult_int_scalar(square(p_h), 2), -1), other b:
              auto_cc_sub(mult_int_scalar(auto_cc_mult(p_hi, p_{b - hi}), 2), p_{2 hi - b});  each level_up'd to the deepest, L_b
          q_g = weighted_sums(babies, [[r_{g, b}] b >= 1], consts=[r_{g, 0}]), r the host coefficients: coeffs[g n1 + b] (power),
              or the remainders of repeated numpy chebdiv by T_n1 (chebyshev: encdec.cheb_blocks)
          giants: y = p_n1 by the same rule from p_{n1 / 2}, y^g (plain powers in both bases) by the power rule
          q_g, y^g level_up'd to L_c = max(level of y^(G - 1), L_b + 1);  r = cc_dot([(q_g, y^g) g >= 1], evk)
          result = cc_add(r, level_up(q_0, L_c + 1));  G = 1: q_0."""
        self._enter()
        if not is_struct(ct) or ct.origin != types.origins["ct"]:
            raise errors.NotMatchType(origin=getattr(ct, "origin", type(ct).__name__), to=types.origins["ct"])
        if ct.ntt_state or ct.include_special:
            raise errors.NotMatchDataStructState(origin=ct.origin)
        c = np.asarray(coeffs, dtype=np.float64)
        if c.ndim != 1 or c.size < 2:
            raise ValueError("poly_eval: coefficients of a polynomial of degree >= 1")
        d = c.size - 1
        depth = self.poly_depth(d, basis, interval, n1)
        if ct.level + depth >= self.num_levels:
            raise errors.MaximumLevelError(level=ct.level, level_max=self.num_levels)
        cheb = basis == "chebyshev"
        if not cheb and interval is not None:
            raise ValueError("poly_eval: an interval belongs to basis='chebyshev'; the power basis has no change of variable")
        n1 = encdec.poly_split(d) if n1 is None else int(n1)
        sched = encdec.poly_schedule(d, n1)
        G = sched["G"]
        if cheb:
            blocks = encdec.cheb_blocks(c, n1)
            if interval is not None and tuple(interval) != (-1, 1):
                a, b = (float(v) for v in interval)
                ct = self.add_scalar(self.mult_scalar(ct, 2.0 / (b - a)), -(a + b) / (b - a))
        else:
            padded = np.concatenate([c, np.zeros(G * n1 - c.size)])
            blocks = padded.reshape(G, n1)
        base = ct.level
        powers = self._power_tree({1: ct}, n1 - 1, evk, cheb)
        Lb = base + sched["baby"]
        babies = self._at_level([powers[b] for b in range(1, n1)], Lb)
        q = self.weighted_sums(babies, blocks[:, 1:], consts=blocks[:, 0])
        if G == 1:
            return q[0]
        half = powers[n1 // 2]
        y = self.square(half, evk)
        if cheb:
            y = self.level_sum([(y, 2)], const=-1)
        ys = self._power_tree({1: y}, G - 1, evk, False)
        Lc = base + sched["common"]
        ups = self._at_level([q[g] for g in range(1, G)] + [ys[g] for g in range(1, G)], Lc)
        r = self.cc_dot(list(zip(ups[:G - 1], ups[G - 1:])), evk)
        return self.level_sum([(r, 1), (q[0], 1)])

    def poly_eval_batch(self, cts: list, coeffs, evk, basis="power", interval=None, n1=None) -> list:
        """The same polynomial on B ciphertexts of one level (an activation over a layer's outputs): returns
        [poly_eval(ct, coeffs, evk, basis, interval, n1) for ct in cts], bit for bit.  poly_eval's schedule, walked once for all B
        ciphertexts, so that the key is streamed once per group of up to 4 ciphertexts instead of once per ciphertext:
          chebyshev, interval != (-1, 1):  the change of variable per ciphertext, as poly_eval makes it
          babies: every square p_2h = square(p_h) of all B ciphertexts in ONE cc_mult_batch per step h, every product
              p_hi * p_{b - hi} of one hi of all B ciphertexts in ONE cc_mult_batch; the Chebyshev corrections of a step and the
              level_ups of all ciphertexts through level_sum_batch / level_up_batch (levelsum.py: the words of the chains above)
          q_g: weighted_sums per ciphertext (the sets share nothing: a batched entry would only save launches)
          giants: y = p_n1 from p_{n1 / 2} in ONE cc_mult_batch of B squares, y^g by the same batched tree
          r = cc_dot_batch of B dots [(q_g, y^g) g >= 1], ONE call;  result = cc_add(r, level_up(q_0, L_c + 1)), ONE level_sum_batch;
          G = 1: q_0, no dot.
        cc_mult_batch and cc_dot_batch return the words of cc_mult and cc_dot, so each result has the words of poly_eval's
        composition.  An empty list: ValueError; ciphertexts of different levels: NotMatchDataStructState; the other refusals are
        poly_eval's, before any work."""
        self._enter()
        cts = list(cts)
        if not cts:
            raise ValueError("poly_eval_batch: at least one ciphertext")
        for ct in cts:
            if not is_struct(ct) or ct.origin != types.origins["ct"]:
                raise errors.NotMatchType(origin=getattr(ct, "origin", type(ct).__name__), to=types.origins["ct"])
        base = cts[0].level
        for ct in cts:
            if ct.level != base:
                raise errors.NotMatchDataStructState(origin=f"{ct.origin} at level {ct.level} beside level {base}")
            if ct.ntt_state or ct.include_special:
                raise errors.NotMatchDataStructState(origin=ct.origin)
        c = np.asarray(coeffs, dtype=np.float64)
        if c.ndim != 1 or c.size < 2:
            raise ValueError("poly_eval: coefficients of a polynomial of degree >= 1")
        d = c.size - 1
        depth = self.poly_depth(d, basis, interval, n1)
        if base + depth >= self.num_levels:
            raise errors.MaximumLevelError(level=base, level_max=self.num_levels)
        cheb = basis == "chebyshev"
        if not cheb and interval is not None:
            raise ValueError("poly_eval: an interval belongs to basis='chebyshev'; the power basis has no change of variable")
        n1 = encdec.poly_split(d) if n1 is None else int(n1)
        sched = encdec.poly_schedule(d, n1)
        G = sched["G"]
        if cheb:
            blocks = encdec.cheb_blocks(c, n1)
            if interval is not None and tuple(interval) != (-1, 1):
                a, b = (float(v) for v in interval)
                cts = [self.add_scalar(self.mult_scalar(ct, 2.0 / (b - a)), -(a + b) / (b - a)) for ct in cts]
        else:
            padded = np.concatenate([c, np.zeros(G * n1 - c.size)])
            blocks = padded.reshape(G, n1)
        base = cts[0].level
        trees = self._power_tree_batch([{1: ct} for ct in cts], n1 - 1, evk, cheb)
        Lb = base + sched["baby"]
        babies = self._at_level([t[b] for t in trees for b in range(1, n1)], Lb)
        qs = [self.weighted_sums(babies[i * (n1 - 1):(i + 1) * (n1 - 1)], blocks[:, 1:], consts=blocks[:, 0]) for i in range(len(trees))]
        if G == 1:
            return [q[0] for q in qs]
        ys = self.cc_mult_batch([(t[n1 // 2], t[n1 // 2]) for t in trees], evk)
        if cheb:
            ys = self.level_sum_batch([([(y, 2)], -1) for y in ys])
        giants = self._power_tree_batch([{1: y} for y in ys], G - 1, evk, False)
        Lc = base + sched["common"]
        ups = self._at_level([x[g] for q, yt in zip(qs, giants) for x in (q, yt) for g in range(1, G)], Lc)
        n = G - 1
        rs = self.cc_dot_batch([list(zip(ups[2 * n * i:2 * n * i + n], ups[2 * n * i + n:2 * n * (i + 1)])) for i in range(len(qs))], evk)
        return self.level_sum_batch([([(r, 1), (q[0], 1)], None) for r, q in zip(rs, qs)])
