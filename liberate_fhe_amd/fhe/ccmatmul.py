"""cc_matmul, mixed into `ckks_engine`: a matrix of ciphertexts times a matrix of ciphertexts under one evaluation key,

    C[i][j] = sum_t A[i][t] * B[t][j]        (slot-wise products, one level down)

— attention scores, a bilinear layer, many small matrix products packed slot-wise.  As m n dots of k pairs (cc_dot_batch) the
per-pair work is done once per PAIR: A[i][t] stands in n dots and B[t][j] in m, so 2 m k n ciphertexts are rescaled and
transformed where m k + k n are distinct, and the tensor kernel reads four operand polynomials per product.  The native call
(lf_cc_matmul) transforms every distinct operand once into a resident store and sums the triplets of a tile of 2 x 2 (1 x 4,
4 x 1, ..) outputs over the whole inner dimension in one launch (matmul_tensor_kernel), reading the operands of an inner index
once for the tile; everything behind the tensor products is cc_dot_batch's, per tile.  Like the engine's other options beyond
the reference, the words are DEFINED by a composition the engine already has — cc_dot of every output's pairs — and that is
what runs wherever the native call does not apply.  DESIGN.md §4.2.
"""
from __future__ import annotations

import ctypes

import torch

from . import encdec
from .data_struct import data_struct
from .presets import types


class CcMatmulOps:
    def cc_matmul(self, A: list, B: list, evk: data_struct) -> list:
        """C = A B for A of m rows of k ciphertexts and B of k rows of n: the list of m rows of n ciphertexts
        C[i][j] = sum_t A[i][t] * B[t][j] (slot-wise), at level + 1.  Entries: ciphertexts of one level, coefficient domain, no
        special limbs, or None for a zero entry; the same object may stand anywhere in A and B, any number of times
        (cc_matmul(A, A, evk) is legal).  C[i][j] has exactly the words of
            cc_dot([(A[i][t], B[t][j]) for t in range(k) if A[i][t] is not None and B[t][j] is not None], evk)
        which is also what runs (through cc_dot_batch) where the native call does not apply: several devices or ranks, logN
        outside 13..17, a checker backend, operands that are not contiguous, relin_fold off, an inner dimension above
        encdec.CC_MATMUL_MAX_INNER.  One native call (lf_cc_matmul) per row block of A holding at most
        encdec.CC_MATMUL_MAX_OPERANDS distinct operands (encdec.cc_matmul_plan): usually one for the whole product.
        ValueError for an empty matrix, ragged rows, mismatched inner dimensions, an output with no term; the entries' checks
        are cc_dot's."""
        self._enter()
        A, B = [list(r) for r in A], [list(r) for r in B]
        m, k, n, calls = encdec.cc_matmul_plan(A, B)
        distinct = list({id(x): x for M in (A, B) for row in M for x in row if x is not None}.values())
        pairs, l = self._cc_dot_pairs([(x, x) for x in distinct])        # every operand a ciphertext of ONE level, cc_dot's states
        level = l + 1
        d = self._cc_dot_device(pairs, level) if calls is not None and hasattr(self.backend, "cc_matmul_native") else None
        if d is None:
            dots = [[(A[i][t], B[t][j]) for t in range(k) if A[i][t] is not None and B[t][j] is not None]
                    for i in range(m) for j in range(n)]
            flat = self.cc_dot_batch(dots, evk)
            return [flat[i * n:(i + 1) * n] for i in range(m)]
        out = []
        for call in calls:
            flat = self._cc_matmul_call(call, k, n, evk, level, d)
            out += [flat[i * n:(i + 1) * n] for i in range(call["rows"][1] - call["rows"][0])]
        return out

    def _cc_matmul_call(self, call, k, n, evk, level, d):
        """One row block of C INTO `level` on device d as ONE native call (lf_cc_matmul); one allocation per output."""
        N = self.ctx.N
        rows, ops = call["rows"][1] - call["rows"][0], call["operands"]
        nout, nu = rows * n, len(ops)
        nct = next((s for s in getattr(self.backend, "ks_batch_sizes", ()) if s <= nout), 1)   # outputs per tile: the plan's stacks
        plan, _, first_part, row_off = self._op_plan(level, d, nct)
        ins, row0s = (ctypes.c_void_p * (2 * nu))(), (ctypes.c_void_p * (2 * nu))()
        for u, ct in enumerate(ops):
            for comp in range(2):
                ptr = ct.data[comp][0].data_ptr()
                row0s[2 * u + comp], ins[2 * u + comp] = ptr, ptr + N * 8     # the dropped limb is the first row; the survivors follow it
        kpack = self._key_pack(evk)[self._loc(0, special=True).index(d)]
        # the store grows with the number of distinct operands: ONE scratch tensor per lane, replaced by a larger one when needed
        # (_ws keeps a tensor per shape)
        self._same_stream(d)
        words, key = self.backend.cc_matmul_ws_words(plan, nu), ("matmul_ws", d, self._lane)
        ws = self._workspace.get(key)
        if ws is None or ws.numel() < words:
            if ws is not None:
                self._retire([ws], d)       # the smaller store may still be read by a call pending on another stream
            ws = self._workspace[key] = torch.empty((words,), dtype=torch.int64, device=self.ntt.devices[d])
        outs = [torch.empty((2, plan.ell, N), dtype=torch.int64, device=self.ntt.devices[d]) for _ in range(nout)]
        self.backend.cc_matmul_native(plan, rows, k, n, ins, row0s, call["ia"], call["ib"], kpack, first_part, row_off, outs, ws)
        return [self._new(([o[0]], [o[1]]), types.origins["ct"], level=level) for o in outs]
