"""mod_raise, linear_transform_conj and the coefficient / slot transforms, mixed into `ckks_engine`: the linear half of a CKKS
bootstrap (the reference has none of it).

    mod_raise(ct)                         the base-prime residue of ct, lifted to every limb of level 0
    linear_transform_conj(ct, D, E, ..)   sum d_s roll(m, s) + sum e_s roll(conj(m), s): a REAL-linear map of the slots
    coeffs_to_slots / slots_to_coeffs     the plaintext polynomial's coefficients into the slots, two to a slot, and back

mod_raise's words are DEFINED by exact int64 arithmetic (written out in its docstring), which is what runs, through torch on each
device, wherever the native call (lf_mod_raise) does not apply.  The transforms are compositions of public ops:
lt_matmul_bsgs over [ct, conjugate(ct)] with the dense matrices of encdec.coeff_slot_matrices.  DESIGN.md §4.2.
"""
from __future__ import annotations

import numpy as np
import torch

from . import encdec
from .evaluator import is_struct
from .presets import errors, types


class ModRaiseOps:
    # the native call where it applies; False keeps every ciphertext on the torch chain (tools/mod_raise.py times one against
    # the other)
    mod_raise_native = True

    # ---------------------------------------------------------------------------------------------
    # mod_raise
    # ---------------------------------------------------------------------------------------------
    def _base_row_at(self, level):
        """(logical device, row index in its tensor) of the base-prime row at `level`."""
        base = self.ntt.p.base_prime_idx
        for d, dest in enumerate(self.ntt.p.destination_arrays[level]):
            if base in dest:
                return d, list(dest).index(base)
        raise ValueError(f"mod_raise: no base-prime row at level {level}")

    def _mod_raise_checked(self, ct):
        if not is_struct(ct) or ct.origin != types.origins["ct"]:
            raise errors.NotMatchType(origin=getattr(ct, "origin", type(ct).__name__), to=types.origins["ct"])
        if ct.ntt_state or ct.montgomery_state or ct.include_special:
            raise errors.NotMatchDataStructState(origin=ct.origin)
        return ct

    def _mod_raise_primes(self, d):
        """[rows, 1] column of the primes of level 0 on device d (cached)."""
        key = ("raise_q", d)
        hit = self._tables.get(key)
        if hit is None:
            hit = self._tables[key] = self._t64([[self.ctx.q[i]] for i in self.ntt.p.destination_arrays[0][d]], d)
        return hit

    def _mod_raise_centre(self, w):
        qb = self.base_prime
        r = torch.remainder(w, qb)
        return torch.where(r > (qb - 1) // 2, r - qb, r)

    def _mod_raise_torch(self, ct):
        """The definition, through torch on each device that holds rows at level 0."""
        N = self.ctx.N
        src, row = self._base_row_at(ct.level)
        loc0 = self._loc(0)
        per_dev = {}
        if self._multi:
            # one process per GPU: the two base rows travel from their owner to every rank in one message
            me = self.local_ids[0]
            buf = self._ws("mod_raise_rows", (2, N), me)
            if src == me:
                for comp in range(2):
                    buf[comp].copy_(ct.data[comp][0][row])
            self.comm.fanout_into(buf, src, list(range(self.len_devices[0])))
            if me in loc0:
                per_dev[me] = [self._mod_raise_centre(buf[comp]) for comp in range(2)]
        else:
            li = self._loc(ct.level).index(src)
            v = [self._mod_raise_centre(ct.data[comp][li][row]) for comp in range(2)]
            for d in loc0:
                dev = self.ntt.devices[d]
                per_dev[d] = [x if str(x.device) == dev else x.to(dev) for x in v]
        data = [[torch.remainder(per_dev[d][comp][None, :], self._mod_raise_primes(d)) for d in loc0] for comp in range(2)]
        return self._new(tuple(data), types.origins["ct"], level=0)

    def _mod_raise_device(self, ct):
        """The device the native call of this ciphertext runs on, or None: the torch chain."""
        be = self.backend
        if not self.mod_raise_native or not hasattr(be, "mod_raise_call") or self._multi or self.len_devices[0] != 1:
            return None
        loc0 = self._loc(0)
        src, row = self._base_row_at(ct.level)
        if loc0 != [src] or self.base_prime >= (1 << 62):
            return None
        li = self._loc(ct.level).index(src)
        for comp in range(2):
            t = ct.data[comp][li]
            if not (t.is_cuda and t.dtype == torch.int64 and t.dim() == 2 and t.size(1) == self.ctx.N and t.is_contiguous()
                    and t.data_ptr() % 16 == 0 and str(t.device) == str(self.ntt.psi[src].device)):
                return None
        return src

    def _mod_raise_native(self, cts, d):
        N = self.ctx.N
        rows = len(self.ntt.p.destination_arrays[0][d])
        dev = self.ntt.devices[d]
        self._same_stream(d)
        base, outs = [], []
        for ct in cts:
            _, row = self._base_row_at(ct.level)
            li = self._loc(ct.level).index(d)
            base.append((ct.data[0][li][row], ct.data[1][li][row]))
            # (one allocation per component, as rescale makes them: an output kept alive pins no other)
            outs.append([torch.empty((rows, N), dtype=torch.int64, device=dev) for _ in range(2)])
        mont_one = self._row_scalars(1, 0, True)[self._loc(0).index(d)]
        self.backend.mod_raise_call(base, outs, rows, self.base_prime, mont_one, self._consts(d, 0, False))
        return [self._new(([o[0]], [o[1]]), types.origins["ct"], level=0) for o in outs]

    def mod_raise_batch(self, cts) -> list:
        """[mod_raise(ct) for ct in cts], word for word and in order; the members the native call takes share launches of up to
        backend.mod_raise_max_cts ciphertexts whatever their levels, the others take the torch chain one by one.  The same
        object may appear any number of times.  Refused as a whole, before any work, where any member would be."""
        self._enter()
        cts = [self._mod_raise_checked(ct) for ct in list(cts)]
        out = [None] * len(cts)
        groups = {}
        for i, ct in enumerate(cts):
            d = self._mod_raise_device(ct)
            if d is None:
                out[i] = self._mod_raise_torch(ct)
            else:
                groups.setdefault(d, []).append(i)
        cap = getattr(self.backend, "mod_raise_max_cts", 1)
        for d, idx in groups.items():
            for i0 in range(0, len(idx), cap):
                part = idx[i0:i0 + cap]
                for i, r in zip(part, self._mod_raise_native([cts[i] for i in part], d)):
                    out[i] = r
        return out

    def mod_raise(self, ct):
        """A spent ciphertext lifted back to the full modulus: reads ONLY the base-prime row of c0 and c1 (a coefficient-domain
        ciphertext without special limbs at any level; its residue mod q_b is a ciphertext mod q_b of the same plaintext
        polynomial, so no level is consumed on the way in) and returns a ciphertext at level 0.  Per coefficient, with w the
        stored word (a lazy word in [0, 2 q_b), or the word in (-q_b / 2, 0) a rescale leaves now and then: any -q_b < w < 2 q_b)
            r = w mod q_b  in [0, q_b);     v = r - q_b  if r > (q_b - 1) / 2  else r;     row i = v mod q_i  in [0, q_i)
        — canonical words, coefficient domain, no Montgomery form, the flags of a level_up output.  In exact int64 arithmetic
        (|v| < 2^61) that is torch.remainder(v, q_i), which is also what runs, on each device that holds rows of level 0, where
        the native call does not apply: several devices or ranks, a checker backend, non-contiguous operands.  Otherwise ONE
        native launch (lf_mod_raise) for both components.
        The result decrypts over Z to T = lift(c0) + lift(c1) s = t + q_b I: t the centred plaintext mod q_b, |I_j| at most
        (h + 1) / 2 for a secret of Hamming weight h (create_secret_key(hamming_weight=h)) — the overflow the sine step of a
        bootstrap removes.  The type and state refusals are level_up's and level_sum's, before any work."""
        return self.mod_raise_batch([ct])[0]

    # ---------------------------------------------------------------------------------------------
    # linear_transform_conj
    # ---------------------------------------------------------------------------------------------
    @staticmethod
    def _lt_conj_row(diags_z, diags_conj):
        if diags_z is None and diags_conj is None:
            raise ValueError("linear_transform_conj: both blocks are None")
        return [[diags_z, diags_conj]]

    def linear_transform_conj_steps(self, diags_z, diags_conj, n1=None) -> tuple:
        """(n1, baby steps, giant steps) of linear_transform_conj(.., diags_z, diags_conj, .., n1): lt_matmul_bsgs_steps of the
        one-row matrix.  A rotation key for every non-zero entry of either list, and the conjugation key."""
        return self.lt_matmul_bsgs_steps(self._lt_conj_row(diags_z, diags_conj), n1)

    def linear_transform_conj(self, ct, diags_z, diags_conj, rotks, conjk, n1=None):
        """A real-linear map of the slots as ONE ciphertext at ct.level + 1: decrypts to
            sum_s d_s * roll(m, s) + sum_s e_s * roll(conj(m), s),
        d = diags_z, e = diags_conj: each an encode_diagonals(.., bsgs=n1) object of ct's level, a plain {step: vector} mapping,
        or None for a zero block (not both).  Defined as, and implemented by,
            lt_matmul_bsgs([[diags_z, diags_conj]], [ct, conjugate(ct, conjk)], rotks, n1)[0]
        — exactly that composition's words: both blocks are summed before anything comes down, under one rescale.  With
        diags_conj=None the conjugation is not computed and the words are those of lt_matmul_bsgs([[diags_z]], [ct], ..).  A
        missing rotation key is named by its step (lt_matmul_bsgs's error)."""
        W = self._lt_conj_row(diags_z, diags_conj)
        if diags_conj is None:
            return self.lt_matmul_bsgs([[diags_z]], [ct], rotks, n1)[0]
        return self.lt_matmul_bsgs(W, [ct, self.conjugate(ct, conjk)], rotks, n1)[0]

    # ---------------------------------------------------------------------------------------------
    # coefficients <-> slots
    # ---------------------------------------------------------------------------------------------
    # below this factor on the matrices the one-level form would encode entries with fewer bits than the default's, and the
    # constant is taken out in a scalar multiplication of its own (one more level)
    coeff_slot_min_factor = 0.25

    def coeff_slot_steps(self, n1=None) -> tuple:
        """(n1, baby steps, giant steps) of coeffs_to_slots / slots_to_coeffs: the dense matrices have every diagonal, so the
        steps are those of 0 .. num_slots - 1 split at n1 (None: the power of two with the fewest keys, capped at what one
        hoisted set of baby steps holds).  A rotation key for every non-zero entry of either list, and the conjugation key."""
        if n1 is None:
            n1 = encdec.bsgs_split(range(self.num_slots), self.num_slots, None)[0]
            n1 = min(n1, getattr(self.backend, "bsgs_max_baby_keys", 63) + 1)
        return encdec.bsgs_split(range(self.num_slots), self.num_slots, n1)

    def _plain_scale(self, level):
        """What a unit of message is in the plaintext polynomial c0 + c1 s of `level`: encode scales by scale * deviations[level]
        and encrypt by scale once more."""
        return float(self.scale) * float(self.scale) * float(self.deviations[level])

    @staticmethod
    def _divisor(divisor):
        d = float(divisor)
        if not np.isfinite(d) or d <= 0:
            raise ValueError(f"coefficient / slot transform: the divisor must be a positive number, got {divisor!r}")
        return d

    def _c2s_factor(self, level, divisor):
        return 1.0 if divisor is None else self._plain_scale(level) / self._divisor(divisor)

    def _s2c_factor(self, level, divisor, depth):
        return 1.0 if divisor is None else self._divisor(divisor) / self._plain_scale(min(level + depth, self.num_levels - 1))

    def _coeff_slot_depth(self, factor):
        return 1 if factor >= self.coeff_slot_min_factor else 2

    def coeffs_to_slots_depth(self, divisor=None, level=0) -> int:
        """Levels coeffs_to_slots(ct at `level`, .., divisor) consumes: 1 where the matrices times the constant
        (scale^2 deviations[level] / divisor) keep the bits of the default's entries (a constant of 1/4 or more: the default,
        and divisor = base_prime at the presets' scales), else 2."""
        return self._coeff_slot_depth(self._c2s_factor(level, divisor))

    def slots_to_coeffs_depth(self, divisor=None, level=0) -> int:
        """Levels slots_to_coeffs(ct at `level`, .., divisor) consumes: as coeffs_to_slots_depth, for the constant
        divisor / (scale^2 deviations[output level])."""
        return self._coeff_slot_depth(self._s2c_factor(level, divisor, 1))

    def _coeff_slot_blocks(self, which, level, factor, n1):
        """The two encoded blocks of a transform — (B, C) times `factor` for "c2s", (E, F) for "s2c" — encoded once per
        (which, level, factor, n1) and kept on the engine (the least recently used of 8 dropped: a block is num_slots diagonals)."""
        cache = self.__dict__.setdefault("_coeff_slot_cache", {})
        key = (which, level, float(factor), n1)
        hit = cache.get(key)
        if hit is not None:
            return hit
        B, C, E, F = encdec.coeff_slot_matrices(self.ctx.N, self.norm)
        pair = (B, C) if which == "c2s" else (E, F)
        hit = cache[key] = tuple(self.encode_diagonals(encdec.matrix_diagonals(M * factor), level, bsgs=n1) for M in pair)
        while len(cache) > 8:
            cache.pop(next(iter(cache)))
        return hit

    def _coeff_slot_apply(self, which, ct, rotks, conjk, factor, depth, n1):
        n1 = self.coeff_slot_steps(n1)[0]
        if depth == 1:
            return self.linear_transform_conj(ct, *self._coeff_slot_blocks(which, ct.level, factor, n1), rotks, conjk, n1)
        # the constant on its own level: the integer mult_scalar would multiply by, its rounding folded back into the matrices
        lvl = ct.level + 1
        unit = float(self.scale) * float(np.sqrt(self.deviations[lvl + 1]))
        k_int = max(1, int(factor * unit + 0.5))
        out = self.linear_transform_conj(ct, *self._coeff_slot_blocks(which, ct.level, factor * unit / k_int, n1), rotks, conjk, n1)
        return self.rescale(self._scale_rows(out, self._row_scalars(k_int, lvl, True)))

    def coeffs_to_slots(self, ct, rotks, conjk, divisor=None, n1=None):
        """The coefficients of ct's plaintext polynomial into the slots, two to a slot: with P = c0 + c1 s the integer polynomial
        ct decrypts to over its modulus, slot j of the result holds (P_j + i P_{j + n}) / divisor, n = num_slots.
        divisor=None: the level's own plaintext scale, scale^2 deviations[level] (encode's scale * deviations[level] times the
        scale encrypt multiplies by) — the slots are then the coefficients in message units, what
        encode(m, return_without_scaling=True) computes.  For a raised ciphertext pass divisor = engine.base_prime: slot j is
        I_j + (message part) / q_b.
        linear_transform_conj with the dense matrices (B, C) of encdec.coeff_slot_matrices times scale^2 deviations[level] /
        divisor, encoded once per (level, divisor, n1) and kept; coeffs_to_slots_depth levels (1, or 2 where the constant is
        small and goes through a scalar multiplication of its own).  Keys: coeff_slot_steps(n1) and the conjugation key."""
        factor = self._c2s_factor(self._mod_raise_checked(ct).level, divisor)
        return self._coeff_slot_apply("c2s", ct, rotks, conjk, factor, self._coeff_slot_depth(factor), n1)

    def slots_to_coeffs(self, ct, rotks, conjk, divisor=None, n1=None):
        """The inverse of coeffs_to_slots: the result's plaintext polynomial has the coefficients P_j = divisor Re(u_j),
        P_{j + n} = divisor Im(u_j), u the slots of ct.  divisor=None: the OUTPUT level's own plaintext scale, so
        slots_to_coeffs(coeffs_to_slots(ct)) decrypts to ct's message.  The matrices (E, F) times divisor / (scale^2
        deviations[output level]); slots_to_coeffs_depth levels."""
        level = self._mod_raise_checked(ct).level
        depth = self.slots_to_coeffs_depth(divisor, level)
        return self._coeff_slot_apply("s2c", ct, rotks, conjk, self._s2c_factor(level, divisor, depth), depth, n1)
