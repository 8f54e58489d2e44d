"""lt_matmul, mixed into `ckks_engine`: a k_out x k_in matrix of diagonal sets times k_in ciphertexts — a matrix larger than one
ciphertext's slots, or a layer applied to several packed inputs:

    y_o = sum_i sum_{step in steps(W[o][i])} diag_{o,i,step} * rot(x_i, step)

It is the union of pc_matmul (a matrix of plaintexts, no rotations) and linear_transform (one ciphertext under a sum of diagonals
times rotations).  The key-switched rotations of x_i do not depend on the output: they are formed once per input and shared by
all outputs; the sums over the inputs stay in Q P and every output is brought down once.  Like the engine's other options beyond
the reference, the words are DEFINED as a composition of steps the engine already has (written out in lt_matmul's docstring), and
that composition is what runs wherever the native call (lf_lt_matmul) does not apply.  DESIGN.md §4.2.

lt_matmul_batch is lt_matmul over many token vectors under one matrix and one key set: the loop's words, the tokens in groups
of 4 and 2 through one native call (lf_lt_matmul_batch) that reads every key once per group and every diagonal once per pair.

lt_matmul_bsgs is the same matrix over baby-step / giant-step blocks (encode_diagonals(.., bsgs=n1)): the baby rotations are formed
once per input, the inner sums of all inputs of one output are added in Q P before the giant key switch, and the outputs that share
a giant step share the stream of its key (lf_lt_matmul_bsgs).

lt_matmul_bsgs_batch is lt_matmul_bsgs over many token vectors under one matrix and one key set: the loop's words, the tokens in
groups of 4 and 2 through one native call (lf_lt_matmul_bsgs_batch) that reads every baby key once per group, every diagonal once per
pair, and every giant key once per 4 (token, output) members.

The four ops are ONE driver: a flat block is a baby-step / giant-step block with n1 = num_slots (steps are taken mod num_slots, so
every step is its own baby step and the only giant step is 0), and the single op is the batch of one token.  `name` ("lt_matmul" or
"lt_matmul_bsgs") selects the messages, the blocks that are accepted and the backend's entries; everything else is shared.
"""
from __future__ import annotations

from collections.abc import Mapping

import torch

from . import encdec
from .backend import HipBackend
from .evaluator import is_struct
from .presets import errors, types


class LtMatmulOps:
    # include/ckks_hip.h: LF_LT_MATMUL_MAX_INPUTS and LF_BSGS_MAX_BABY_KEYS (the keyed steps of one column), refused on every path
    # (the outputs of one native call are the backend's lt_matmul_max_outputs: more are split over calls)
    lt_matmul_max_inputs = HipBackend.lt_matmul_max_inputs
    lt_matmul_max_column_keys = HipBackend.bsgs_max_baby_keys

    def _lt_matmul_blocks(self, name, W, n1=None):
        """(W as a list of rows, per block its steps in the order of its data or None, n1): the checks that need nothing but the
        matrix and n1; n1 = num_slots for the flat ops.  Nothing is encoded or allocated here."""
        flat = name == "lt_matmul"
        want = types.origins["diag" if flat else "diag_bsgs"]
        W = [list(row) for row in W]
        if not flat and n1 is not None:
            n1 = encdec.bsgs_split([0], self.num_slots, n1)[0]            # (ValueError for anything but an integer >= 1)
        if not W:
            raise ValueError(f"{name}: at least one row of blocks")
        k_in = len(W[0])
        steps, tagged = [], set()
        for row in W:
            if len(row) != k_in:
                raise ValueError(f"{name}: a row of {len(row)} blocks beside one of {k_in}")
            if all(b is None for b in row):
                raise ValueError(f"{name}: a row without a block")
            srow = []
            for b in row:
                if b is None:
                    srow.append(None)
                elif is_struct(b):
                    if flat and b.origin.startswith(types.origins["diag_bsgs"]):
                        raise NotImplementedError("lt_matmul: flat diagonals only (giant steps inside a block are out of scope)")
                    if not b.origin.startswith(want):
                        raise errors.NotMatchType(origin=b.origin, to=want)
                    if not flat:
                        tagged.add(int(b.origin.split(":", 1)[1].split(";")[0]))
                    srow.append(self.diagonal_steps(b))
                elif isinstance(b, Mapping):
                    s = sorted(int(k) % self.num_slots for k in b)
                    if not s:
                        raise ValueError(f"{name}: a block without a diagonal")
                    if len(set(s)) != len(s):
                        raise ValueError(f"{name}: a step given twice in one block (steps are taken mod {self.num_slots})")
                    srow.append(s)
                else:
                    raise errors.NotMatchType(origin=getattr(b, "origin", type(b).__name__), to=want)
            steps.append(srow)
        if k_in < 1:
            raise ValueError(f"{name}: at least one ciphertext")
        if flat:
            n1 = self.num_slots
        else:
            if len(tagged) > 1:
                raise ValueError(f"{name}: blocks encoded for different n1 ({sorted(tagged)})")
            if tagged and n1 is not None and n1 not in tagged:
                raise ValueError(f"{name}: n1 = {n1} beside blocks encoded for n1 = {min(tagged)}")
            if not tagged and n1 is None:
                raise ValueError(f"{name}: n1 is required when every block is a plain mapping")
            n1 = min(tagged) if tagged else n1
        if k_in > self.lt_matmul_max_inputs:
            raise ValueError(f"{name}: {k_in} inputs, at most {self.lt_matmul_max_inputs}")
        for i in range(k_in):
            keyed = {s % n1 for srow in steps if srow[i] is not None for s in srow[i] if s % n1}
            if len(keyed) > self.lt_matmul_max_column_keys:
                raise ValueError(f"{name}: column {i} needs {len(keyed)} keyed {'' if flat else 'baby '}steps, "
                                 f"at most {self.lt_matmul_max_column_keys}")
        return W, steps, n1

    def _lt_matmul_operands(self, name, W, cts, rotks):
        """(cts as a list, {step: key}, level): the checks of lt_matmul and lt_matmul_bsgs on the ciphertexts, the keys and the
        levels, in their order; nothing is encoded or allocated here."""
        cts = list(cts)
        k_in = len(W[0])
        if len(cts) != k_in:
            raise ValueError(f"{name}: rows of {k_in} blocks beside {len(cts)} ciphertexts")
        for ct in cts:
            if not is_struct(ct) or ct.origin != types.origins["ct"]:
                raise errors.NotMatchType(origin=getattr(ct, "origin", type(ct).__name__), to=types.origins["ct"])
        keys = list(rotks.values()) if isinstance(rotks, dict) else list(rotks)
        by_step = {}
        for k in keys:
            if not is_struct(k) or types.origins["rotk"] not in k.origin:
                raise errors.NotMatchType(origin=getattr(k, "origin", type(k).__name__), to=types.origins["rotk"])
            by_step.setdefault(int(k.origin.split(":")[-1]) % self.num_slots, k)
        for ct in cts:
            if ct.ntt_state or ct.include_special:
                raise NotImplementedError(f"{name}: coefficient-domain ciphertexts without special limbs only")
        level = cts[0].level
        for ct in cts:
            if ct.level != level:
                raise errors.NotMatchDataStructState(origin=f"{ct.origin} at level {ct.level} beside level {level}")
        for row in W:
            for b in row:
                if is_struct(b) and b.level != level:
                    raise errors.NotMatchDataStructState(origin=f"{b.origin} at level {b.level}, ciphertexts at level {level}")
        if level + 1 >= self.num_levels:
            raise errors.MaximumLevelError(level=level, level_max=self.num_levels)
        return cts, by_step, level

    @staticmethod
    def _lt_matmul_keys_ok(steps, n1, by_step):
        """NotMatchType for the first non-zero baby or giant step (ascending) that has no key"""
        flat = [s for srow in steps for b in srow if b is not None for s in b]
        for s in sorted({s % n1 for s in flat} | {s - s % n1 for s in flat}):
            if s and s not in by_step:
                raise errors.NotMatchType(origin=f"no key for step {s}", to=types.origins["rotk"] + str(s))

    def _lt_matmul_encode(self, W, level, bsgs):
        """(a copy of W with every mapping block encoded at `level`, each distinct mapping object ONCE; per block its steps in the
        order of its data or None).  bsgs: n1, or None for flat diagonals."""
        encoded, W = {}, [list(row) for row in W]
        for row in W:
            for i, b in enumerate(row):
                if b is not None and not is_struct(b):
                    if id(b) not in encoded:
                        encoded[id(b)] = self.encode_diagonals(b, level, bsgs=bsgs) if bsgs else self.encode_diagonals(b, level)
                    row[i] = encoded[id(b)]
        return W, [[None if b is None else self.diagonal_steps(b) for b in row] for row in W]

    def _lt_matmul_calls(self, name, steps, n1):
        """The outputs of one native path as consecutive ranges (first, past the last): lt_matmul's 64 per call, lt_matmul_bsgs's
        _lt_matmul_bsgs_calls (None where a row is beyond one call)."""
        if name == "lt_matmul_bsgs":
            return self._lt_matmul_bsgs_calls(steps, n1)
        step = getattr(self.backend, "lt_matmul_max_outputs", len(steps))
        return [(o0, o0 + step) for o0 in range(0, len(steps), step)]

    def _lt_matmul_single(self, name, W, cts, rotks, n1=None):
        """lt_matmul / lt_matmul_bsgs behind their docstrings: the refusals, the encoding, then the native call(s) where they apply
        and the orchestrated steps where they do not."""
        bsgs = name == "lt_matmul_bsgs"
        W, steps, n1 = self._lt_matmul_blocks(name, W, n1)
        cts, by_step, level = self._lt_matmul_operands(name, W, cts, rotks)
        self._lt_matmul_keys_ok(steps, n1, by_step)
        # (every refusal is behind us: from here on things are encoded, allocated and launched)
        W, steps = self._lt_matmul_encode(W, level, n1 if bsgs else None)

        d = self._native_level(level)
        if d is not None and hasattr(self.backend, name + "_native") and \
                all(s is None or s == sorted(s) for srow in steps for s in srow) and \
                all(ct.data[c][0].is_contiguous() for i, ct in enumerate(cts) if any(s[i] is not None for s in steps) for c in range(2)):
            calls = self._lt_matmul_calls(name, steps, n1)
            if calls is not None:
                return [out for o0, o1 in calls
                        for out in self._lt_matmul_native(name, W[o0:o1], steps[o0:o1], n1, [cts], by_step, level, d, batch=False)[0]]
        return self._lt_matmul_steps(W, steps, n1, cts, by_step, level)

    def _lt_matmul_batch(self, name, W, X, rotks, n1=None):
        """lt_matmul_batch / lt_matmul_bsgs_batch behind their docstrings: the loop's refusals in the loop's order, per level one
        encoding, the tokens that qualify in groups through the native batch call, the others through the single op in place."""
        bsgs = name == "lt_matmul_bsgs"
        X = [list(cts) for cts in X]
        if not X:
            return []
        W, steps, n1 = self._lt_matmul_blocks(name, W, n1)
        if not isinstance(rotks, dict):
            rotks = list(rotks)
        levels = []
        for t, cts in enumerate(X):                  # the loop's order: token 0's operands, the keys, then the other tokens' operands
            X[t], by_step, level = self._lt_matmul_operands(name, W, cts, rotks)
            levels.append(level)
            if t == 0:
                self._lt_matmul_keys_ok(steps, n1, by_step)
        # (every refusal is behind us: from here on things are encoded, allocated and launched)
        out = [None] * len(X)
        entry = "lt_matmul_bsgs_batch_call" if bsgs else "lt_matmul_batch_native"
        sizes = [k for k in getattr(self, name + "_batch_sizes") if k in getattr(self.backend, name + "_batch_sizes", ())]
        for level in sorted(set(levels)):
            Wl, lsteps = self._lt_matmul_encode(W, level, n1 if bsgs else None)
            toks = [t for t, l in enumerate(levels) if l == level]
            d = self._native_level(level)
            ready, calls = [], None
            if sizes and d is not None and hasattr(self.backend, name + "_native") and hasattr(self.backend, entry) and \
                    all(s is None or s == sorted(s) for srow in lsteps for s in srow):
                calls = self._lt_matmul_calls(name, lsteps, n1)
                if calls is not None:
                    used = [i for i in range(len(W[0])) if any(s[i] is not None for s in lsteps)]
                    ready = [t for t in toks if all(X[t][i].data[c][0].is_contiguous() for i in used for c in range(2))]
            while ready:
                g = next((k for k in sizes if k <= len(ready)), None)
                if g is None:
                    break
                group, ready = ready[:g], ready[g:]
                parts = [self._lt_matmul_native(name, Wl[o0:o1], lsteps[o0:o1], n1, [X[t] for t in group], by_step, level, d, batch=True)
                         for o0, o1 in calls]
                for j, t in enumerate(group):
                    out[t] = [o for part in parts for o in part[j]]
            for t in toks:
                if out[t] is None:
                    out[t] = self.lt_matmul_bsgs(Wl, X[t], rotks, n1) if bsgs else self.lt_matmul(Wl, X[t], rotks)
        return out

    def _lt_matmul_native_args(self, W, steps, n1, by_step, level, d):
        """What a native call takes of the matrix and the keys alone: (per input whether some block uses it, col_exps, col_keys,
        giant_exps, giant_keys, blocks, the longest column's keyed baby steps, the keyed inner sums, whether two outputs share a
        keyed giant step, round_at), as HipBackend.lt_matmul_bsgs_native names them."""
        N, k_in = self.ctx.N, len(W[0])
        giants = sorted({s - s % n1 for srow in steps for b in srow if b is not None for s in b})   # (0 sorts first)
        rows_of = {g: sum(any(b is not None and any(s - s % n1 == g for s in b) for b in srow) for srow in steps) for g in giants}
        shared = any(g and rows_of[g] >= 2 for g in giants)
        i0 = self._loc(0, special=True).index(d)
        li = self.local_ids.index(d)
        owner = self.ntt.p.rescaler_loc[level]
        round_at = self.ctx.q[self.ntt.p.destination_arrays[level][owner][0]] // 2
        used, col_exps, col_keys, slot = [], [], [], []
        for i in range(k_in):
            col = [s for s in steps if s[i] is not None]
            keyed = sorted({t % n1 for s in col for t in s[i] if t % n1})
            used.append(bool(col))
            col_exps.append([encdec.galois_exponent(N, t) for t in keyed])
            col_keys.append([self._key_pack(by_step[t])[i0] for t in keyed])
            slot.append({0: 0, **{t: 1 + j for j, t in enumerate(keyed)}})

        def per_giant(i, s):
            """per giant step None, or (the index of its first diagonal in the block's pack, the column slots of its diagonals)"""
            out = []
            for g in giants:
                at = [k for k, t in enumerate(s) if t - t % n1 == g]      # (ascending steps: one slice of the pack)
                out.append((at[0], [slot[i][s[k] % n1] for k in at]) if at else None)
            return out

        blocks = [[None if b is None else (self._diag_pack(b)[li], per_giant(i, s[i])) for i, b in enumerate(row)]
                  for row, s in zip(W, steps)]
        return (used, col_exps, col_keys, [encdec.galois_exponent(N, g) if g else 0 for g in giants],
                [self._key_pack(by_step[g])[i0] if g else None for g in giants], blocks, max(len(c) for c in col_keys),
                sum(rows_of[g] for g in giants if g), shared, round_at)

    def _lt_matmul_native(self, name, W, steps, n1, toks, by_step, level, d, batch):
        """ONE native call of the family for the token vectors `toks` (the batch entry where `batch`, else the single entry for the
        one token): per token the list of its output ciphertexts at level + 1."""
        N, bsgs = self.ctx.N, name == "lt_matmul_bsgs"
        sized = batch or not bsgs                    # (the plan of the single BSGS call is sized by what the matrix shares)
        if sized:
            plan, _, first_part, row_off = self._op_plan(level, d, nct=4 if batch else 1)
        used, col_exps, col_keys, giant_exps, giant_keys, blocks, nb_max, keyed_sums, shared, round_at = \
            self._lt_matmul_native_args(W, steps, n1, by_step, level, d)
        if not sized:
            if self.lt_matmul_bsgs_group not in (1, 2, 4):
                raise ValueError("lt_matmul_bsgs_group: 1, 2 or 4")
            plan, _, first_part, row_off = self._op_plan(level, d, nct=self.lt_matmul_bsgs_group if shared else 1)
        ins = [[(ct.data[0][0], ct.data[1][0]) if u else None for ct, u in zip(cts, used)] for cts in toks]
        key = name + ("_batch_ws" if batch else "_ws")
        sizes = (nb_max, len(W)) + ((keyed_sums,) if bsgs else ()) + ((len(toks),) if batch else ())
        ws = self._ws(key, (getattr(self.backend, key + "_words")(plan, *sizes),), d)
        outs = [[torch.empty((2, plan.ell - 1, N), dtype=torch.int64, device=self.ntt.devices[d]) for _ in W] for _ in toks]
        if bsgs:
            giants = (giant_exps, giant_keys)
        else:                                        # the flat entries: no giant steps, per block the slots of the one giant step 0
            giants = ()
            blocks = [[None if b is None else (b[0], b[1][0][1]) for b in row] for row in blocks]
        call = getattr(self.backend, "lt_matmul_bsgs_batch_call" if bsgs and batch else name + ("_batch_native" if batch else "_native"))
        call(plan, ins if batch else ins[0], col_exps, col_keys, *giants, first_part, row_off, blocks, self.rescale_scales[level][d],
             round_at, outs if batch else outs[0], ws)
        return [[self._new(([o[0]], [o[1]]), types.origins["ct"], level=level + 1) for o in tok] for tok in outs]

    def _lt_matmul_steps(self, W, steps, n1, cts, by_step, level):
        """The same words through the engine's steps — the pieces of _linear_transform_bsgs (_lt_chat, _lt_forward, _lt_inner,
        _lt_giant, _lt_tail): per used input the digits of c1 and their exchange once, per baby step of the column the gather, the
        key's inner product and the products with the diagonals of EVERY (output, giant step) that has it in this column; per
        keyed (o, g) S_1 down to Q, its digits, the giant key's inner product and S_0 gathered on all rows into A^o; per output
        ONE inverse NTT, mod-down and rescale.  (The flat ops: n1 = num_slots, the one giant step 0.)"""
        N = self.ctx.N
        loc, n = self._loc(level), self.ntt
        S = {}                                                            # (o, g) -> per device [S_0, S_1]

        def accumulate(di, li, i, b, t):
            mont = [x[li:li + 1] for x in n.mont_prepack[-2][level][0]]
            _2q = [n._2q_prepack[-2][level][0][li]]
            for o, (row, srow) in enumerate(zip(W, steps)):
                if srow[i] is None:
                    continue
                for k, step in enumerate(srow[i]):
                    if step % n1 != b:
                        continue
                    acc = S.setdefault((o, step - b), [[None, None] for _ in loc])[di]
                    for comp in range(2):
                        prod = n.ops.mont_mult([row[i].data[k][li]], [t[comp]], *mont)[0]
                        acc[comp] = prod if acc[comp] is None else n.ops.mont_add([acc[comp]], [prod], _2q)[0]

        for i, ct in enumerate(cts):
            B = sorted({t % n1 for srow in steps if srow[i] is not None for t in srow[i]})
            if not B:
                continue                                                  # an input no output uses
            keyed = [b for b in B if b]
            c1 = [t if t.is_contiguous() else t.contiguous() for t in ct.data[1]]   # (the digit launch takes a raw pointer)
            digits = self._ks_digits_exchanged(c1, level, galois=(1, True)) if keyed else {}
            for di, d in enumerate(loc):
                li = self.local_ids.index(d)
                rows, ell = self._rows(d, level, True), self._rows(d, level, False)
                chat = self._lt_chat(level, d, ct, di)
                if 0 in B:
                    t = torch.zeros((2, rows, N), dtype=torch.int64, device=self.ntt.devices[d])
                    t[:, :ell] = chat
                    accumulate(di, li, i, 0, t)
                if not keyed:
                    continue
                self._lt_forward(level, d, digits)
                _2q = n._2q_prepack[-2][level][0][li]
                for b in keyed:
                    idx = self._galois_index(encdec.galois_exponent(N, b), d)
                    t = self._lt_inner(level, d, idx, by_step[b])
                    t[0, :ell] = n.ops.mont_add([t[0, :ell]], [chat[0].index_select(1, idx)], [_2q[:ell]])[0]
                    accumulate(di, li, i, b, t)

        outs = []
        for o in range(len(W)):
            A = [[None, None] for _ in loc]
            for g in sorted(g for (oo, g) in S if oo == o):
                Sg = S.pop((o, g))
                if g:
                    Sg = self._lt_giant(level, Sg, g, by_step[g])
                for di, d in enumerate(loc):
                    _2q = [n._2q_prepack[-2][level][0][self.local_ids.index(d)]]
                    for comp in range(2):
                        A[di][comp] = Sg[di][comp] if A[di][comp] is None else n.ops.mont_add([A[di][comp]], [Sg[di][comp]], _2q)[0]
            outs.append(self._lt_tail(level, A))
        return outs

    # =============================================================================================
    # the public ops
    # =============================================================================================
    def lt_matmul_steps(self, W) -> list:
        """The sorted non-zero steps lt_matmul(W, ..) needs a rotation key for (one key per step serves every input)."""
        _, steps, _ = self._lt_matmul_blocks("lt_matmul", W)
        return sorted({s for srow in steps for b in srow if b is not None for s in b if s})

    def lt_matmul(self, W, cts, rotks) -> list:
        """A matrix of linear transforms times a vector of ciphertexts: the list of the k_out ciphertexts
            y_o = sum_i sum_{step in steps(W[o][i])} diag_{o,i,step} * rotate(cts[i], step)
        at level + 1 (rotate_single's direction, as linear_transform).  W: k_out rows of k_in entries, each a flat
        encode_diagonals object of the ciphertexts' level, a plain {step: vector} mapping (encoded here, as linear_transform
        does) or None for a zero block; every row needs a block.  cts: k_in ciphertexts of one level (coefficient domain, no
        special limbs); rotks: a list or mapping of rotation keys looked up by the step in their origin — one key per step serves
        every input, step 0 needs none (lt_matmul_steps).  Rows, cts and rotks may be any iterables, objects may repeat anywhere;
        an input no output uses is legal and costs nothing.
        The words are those of: per input i that some block uses c0, c1 made canonical, E_i and c^_i as linear_transform forms
        them; per step != 0 of U_i = the union of the column's steps t^{i,step}_c = sum over the parts of E_i gathered by pi_step
        times the key part, t_0 += c^_{i,0} gathered on the ordinary rows (step 0: t_c = c^_{i,c}, zero on the special rows); per
        output S^o_c = sum_i sum_step mont_mult(pt_{o,i,step}, t^{i,step}_c); intt_exit_reduce, mod-down without addend,
        rescale.  Only residues of t and S reach the result, so the grouping of the additions is free.  With k_in = 1 output o has
        word for word the words of linear_transform(cts[0], W[o][0], rotks); for k_in > 1 the words are the op's own — NOT those
        of cc_add over separate transforms, which round once per block.
        One native call (lf_lt_matmul) per 64 outputs where every limb of the level is on one device of this process — each call
        repeats the rotations of its inputs, so more than 64 outputs pay them again; otherwise the same words through the
        engine's steps, the rotated sums formed once per input and step and accumulated into every output that uses them."""
        self._enter()
        return self._lt_matmul_single("lt_matmul", W, cts, rotks)

    # group sizes of lt_matmul_batch's native path, largest first (filtered by backend.lt_matmul_batch_sizes), as
    # pc_matmul_batch_sizes: a size that does not beat the loop of lt_matmul is left out here and its tokens take lt_matmul one by
    # one — the words are the same (DESIGN.md §4.2 has the numbers; tools/lt_matmul_batch.py --ab measures every size)
    lt_matmul_batch_sizes = (4, 2)

    def lt_matmul_batch(self, W, X, rotks) -> list:
        """lt_matmul of many token vectors under the SAME matrix and keys (a layer over the tokens of a sequence or the samples of
        a batch): returns exactly [lt_matmul(W, cts, rotks) for cts in X], word for word and in order — B lists of k_out
        ciphertexts at level + 1; an empty X gives [].  W, rotks: as lt_matmul takes them (lt_matmul_steps(W) names the keys); X:
        B token vectors of k_in ciphertexts each (the same object may appear in any number of tokens and positions).  What
        lt_matmul refuses for any token is refused for the whole call before anything is encoded, allocated or launched, with the
        error the loop would have raised first.  A mapping block is encoded once per level of the tokens, not once per token:
        encode draws its rounding at random, so a loop would multiply every token by other words; here the tokens of a level
        share ONE encoding of each mapping object, and the words are those of the loop over these encoded objects.
        Where lt_matmul's own native call applies (every limb of the level on one device of this process, ascending steps,
        contiguous operands) and the backend has lf_lt_matmul_batch, the tokens of one level that qualify go, in order, in groups
        of lt_matmul_batch_sizes through ONE native call per group and per 64 outputs: a group shares every launch, the baby sums
        read each rotation key and the block products each diagonal once for the tokens of a launch instead of once per token.
        A token that does not qualify, the one the groups leave over, and every token on a backend without the entry or on a
        sharded or multi-device engine take lt_matmul and keep their place."""
        self._enter()
        return self._lt_matmul_batch("lt_matmul", W, X, rotks)

    # the largest group of outputs whose giant step under one key goes through ONE mod-down, digit launch, forward pass and key
    # stream (4, 2 or 1: the batch the plan of the native call is asked for; 1 takes the single kernel everywhere: same words)
    lt_matmul_bsgs_group = 4

    def lt_matmul_bsgs_steps(self, W, n1=None) -> tuple:
        """(n1, baby steps, giant steps) of lt_matmul_bsgs(W, .., n1): both sorted, 0 included where present, each the union over
        all blocks in the sense of bsgs_steps.  A rotation key is needed for every non-zero entry of either list (one key per
        step serves every input and every output, as a baby and as a giant step)."""
        _, steps, n1 = self._lt_matmul_blocks("lt_matmul_bsgs", W, n1)
        flat = [s for srow in steps for b in srow if b is not None for s in b]
        return n1, sorted({s % n1 for s in flat}), sorted({s - s % n1 for s in flat})

    def lt_matmul_bsgs(self, W, cts, rotks, n1=None) -> list:
        """A matrix of baby-step / giant-step linear transforms times a vector of ciphertexts: the list of the k_out ciphertexts
            y_o = sum_i sum_{step in steps(W[o][i])} diag_{o,i,step} * rotate(cts[i], step)
        at level + 1 — lt_matmul for blocks of hundreds of diagonals, from the keys of the non-zero baby steps b = step mod n1 and
        giant steps g = step - b alone (lt_matmul_bsgs_steps).  W: k_out rows of k_in entries, each an encode_diagonals(..,
        bsgs=n1) object of the ciphertexts' level, a plain {step: vector} mapping (encoded here with bsgs=n1, each distinct
        mapping object once) or None for a zero block; every row needs a block.  All blocks share one n1: that of the tagged
        objects, with which the argument must agree if it is given; it is required when every block is a mapping.  cts and rotks
        as in lt_matmul: one key per step serves every input and every output, and the same key may serve as a baby and as a
        giant step; an input no output uses is legal and is not read.
        The words are those of: per input i that some block uses c0, c1 made canonical, E_i and c^_i as linear_transform forms
        them; per keyed baby step b of B_i = the union of the column's baby steps u^{i,b}_c = sum over the parts of E_i gathered
        by pi_b times key b's part, u^{i,b}_0 += c^_{i,0} gathered on the ordinary rows (b = 0: u^{i,0}_c = c^_{i,c}, zero on the
        special rows); per output o and giant step g of G_o = the union of the row's giant steps
            S^{o,g}_c = sum_i sum_{b : g + b in steps(W[o][i])} mont_mult(pt_{o,i,g+b}, u^{i,b}_c),
        summed over the inputs BEFORE anything comes down; g = 0: S^{o,0} joins the accumulator A^o; g != 0: w = mod-down without
        addend of intt_exit_reduce(S^{o,g}_1), made canonical, E^{o,g} its digits extended and transformed, v_c = sum over the
        parts of E^{o,g} gathered by pi_g times key g's part, v_0 += S^{o,g}_0 gathered on all ell + K rows, A^o += v; then
        intt_exit_reduce(A^o), mod-down without addend, rescale.  Only residues of u, S, v and A reach the result, so the grouping
        of the additions is free.  Hence: with k_in = 1 output o has word for word the words of linear_transform(cts[0], W[o][0],
        rotks) in its baby-step / giant-step form; when every step is below n1 (the only giant step is 0) those of lt_matmul on
        the same packs tagged flat; and output o depends on row o only.  For k_in > 1 with keyed giant steps the words are the
        op's own — NOT those of cc_add over separate transforms.
        One native call (lf_lt_matmul_bsgs) per 64 outputs, 64 giant steps and 256 keyed inner sums where every limb of the level
        is on one device of this process (more outputs or keyed sums are split over calls, each of which repeats the baby steps);
        otherwise the same words through the engine's steps (_lt_matmul_steps) — which is also where a matrix goes that has
        a single row beyond the caps of one call, more than 64 giant steps in one row: it is not run natively."""
        self._enter()
        return self._lt_matmul_single("lt_matmul_bsgs", W, cts, rotks, n1)

    def _lt_matmul_bsgs_calls(self, steps, n1):
        """The outputs as consecutive ranges (first, past the last), each within what one native call takes (outputs, giant steps,
        keyed inner sums); None where a single row is beyond it (lt_matmul_bsgs then takes the orchestrated steps for the whole
        matrix)."""
        be = self.backend
        calls, o0, giants, sums = [], 0, set(), 0
        for o, srow in enumerate(steps):
            g = {s - s % n1 for b in srow if b is not None for s in b}
            keyed = len(g - {0})
            if len(g) > be.lt_matmul_bsgs_max_giants or keyed > be.lt_matmul_bsgs_max_sums:
                return None
            if o > o0 and (o - o0 == be.lt_matmul_max_outputs or len(giants | g) > be.lt_matmul_bsgs_max_giants or
                           sums + keyed > be.lt_matmul_bsgs_max_sums):
                calls.append((o0, o))
                o0, giants, sums = o, set(), 0
            giants |= g
            sums += keyed
        calls.append((o0, len(steps)))
        return calls

    # group sizes of lt_matmul_bsgs_batch's native path, largest first (filtered by backend.lt_matmul_bsgs_batch_sizes), as
    # lt_matmul_batch_sizes: a size that does not beat the loop of lt_matmul_bsgs is left out here and its tokens take lt_matmul_bsgs
    # one by one — the words are the same (DESIGN.md §4.2 has the numbers; tools/lt_matmul_bsgs_batch.py --ab measures every size)
    lt_matmul_bsgs_batch_sizes = (4, 2)

    def lt_matmul_bsgs_batch(self, W, X, rotks, n1=None) -> list:
        """lt_matmul_bsgs of many token vectors under the SAME matrix and keys (a layer of large blocks over the tokens of a
        sequence): returns exactly [lt_matmul_bsgs(W, cts, rotks, n1) for cts in X], word for word and in order — B lists of k_out
        ciphertexts at level + 1; an empty X gives [].  W, rotks, n1: as lt_matmul_bsgs takes them (lt_matmul_bsgs_steps(W, n1)
        names the keys); X: B token vectors of k_in ciphertexts each (the same object may appear in any number of tokens and
        positions; tokens may sit at different levels).  What lt_matmul_bsgs refuses for any token is refused for the whole call
        before anything is encoded, allocated or launched, with the error the loop would have raised first.  A mapping block is
        encoded once per level of the tokens with bsgs=n1, not once per token: encode draws its rounding at random, so a loop would
        multiply every token by other words; here the tokens of a level share ONE encoding of each mapping object, and the words
        are those of the loop over these encoded objects.
        Where lt_matmul_bsgs's own native call applies (every limb of the level on one device of this process, ascending steps,
        contiguous operands of the used inputs, no row beyond the caps of one call) and the backend has lf_lt_matmul_bsgs_batch,
        the tokens of one level that qualify go, in order, in groups of lt_matmul_bsgs_batch_sizes through ONE native call per
        group and per range of outputs (the caps count per token): a group shares every launch of the baby sums (each baby key
        read once for the group), the block products read each diagonal once per pair of tokens, and the tokens of an output
        fill the giant step's chunk of 4, so a giant key is read once per 4 members whatever k_out is.  A token that does not
        qualify, the one the groups leave over, and every token on a backend without the entry or on a sharded or multi-device
        engine take lt_matmul_bsgs and keep their place."""
        self._enter()
        return self._lt_matmul_batch("lt_matmul_bsgs", W, X, rotks, n1)
