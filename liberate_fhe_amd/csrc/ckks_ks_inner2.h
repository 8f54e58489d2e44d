// ckks_ks_inner2.h — the body of the key switch's inner-product kernel (ckks_ks.hip: K3), included once per kernel that shares it:
// ks_inner2_kernel<NCT, FOLD, PLANES, DPL> (PRESUM = false), ks_inner2_presum_kernel<PLANES, DPL> (NCT = 1, FOLD, PRESUM = true) and
// ks_dotb_inner_kernel<NCT, PLANES, DPL> (NCT = 2 or 4, FOLD, PRESUM = true).
// Text inclusion, not a function: the existing instantiations keep the very code they had (a shared __device__ body moved a
// register or two in a dozen of them; profiles/r06_kernel_resources.txt).  The including kernel provides the compile-time
// constants NCT, FOLD, PLANES, DPL, PRESUM and the parameters ext, ksk, part_stride, comp_stride, row_off, s, nparts, rows, N,
// fold, spl, ql, qh, kl, kh.
// PRESUM (cc_dot): fold.x points at a triplet T = [3][ell][N] already summed over many pairs (dot_tensor_kernel: fp64-class rows
// plain canonical residues, integer-class rows Montgomery-form words below 2q, raw words on every row), so the sums take
// REDC(T0 * PR) and REDC(T1 * PR) and the own-limb digit words are T2's, read as they lie; xpl is unused.  cc_dot_batch: the
// triplet of ciphertext t lies at fold.x + t * fold.ct_stride (NCT = 1: t = 0, the stride is never read).
    // spl: the sums of fp64-class rows leave as planes (the inverse passes behind read them so: ks_tail)
    // each thread owns KI_V 16-byte column pairs 4 KiB apart: every block streams KI_V x 4 KiB contiguous runs
    // from 3 x nparts arrays, enough bytes in flight to keep HBM busy
    constexpr int KI_V = KI_COLS;
    const int r = blockIdx.y;
    const i64 j0 = (i64)blockIdx.x * (512 * KI_V) + threadIdx.x * 2;
    if (j0 >= N) return;
    const RowMod m = load_mod(ql, qh, kl, kh, r);
    const RowDp d = make_dp(m);
    const i64 *e = ext + (i64)r * N + j0;
    const i64 *k = ksk + (row_off + r) * N + j0;
    const i64 ct_ext = (i64)nparts * rows * N;   // words between the ciphertexts' extended digits
    const i64 ct_s = 2 * (i64)rows * N;          // .. and between their output pairs
    if (m.q < SMALL_PRIME_LIMIT) {
        double acc[NCT][2][2];
#pragma unroll
        for (int t = 0; t < NCT; ++t) acc[t][0][0] = acc[t][0][1] = acc[t][1][0] = acc[t][1][1] = 0.0;
        const int p_own = (FOLD && fold.own != nullptr && r < fold.ell) ? (int)fold.own[r] : -1;
        const unsigned bo_lo = (unsigned)j0 * 4u, bo_hi = (unsigned)j0 * 2u;   // DPL: byte offsets of the thread's pair in the planes
        // the own digit's words: x1 * y1, plain canonical.  SCALAR arrays, selected by value below: a choice between a 16-byte
        // struct in registers and one in global memory is compiled to a load through select(private address, global address),
        // and an array whose address is taken that way lives in scratch memory (48 .. 128 bytes per lane in the batched kernels
        // until round 6; profiles/r06_kernel_resources.txt)
        i64 xo_x[NCT], xo_y[NCT];
        if (p_own >= 0) {
#pragma unroll
            for (int t = 0; t < NCT; ++t) {
                if constexpr (PRESUM) {
                    const longlong2 T2 = *reinterpret_cast<const longlong2 *>(fold.x + t * fold.ct_stride + (2 * (i64)fold.ell + r) * N + j0);
                    xo_x[t] = T2.x, xo_y[t] = T2.y;
                } else {
                    const i64 *xs = fold.x + t * fold.ct_stride + (i64)r * N + (i64)fold.ell * N;
                    double x1a, x1b, y1a, y1b;
                    ld_pair_dp(xs, j0, N, fold.xpl, x1a, x1b);
                    ld_pair_dp(xs + 2 * (i64)fold.ell * N, j0, N, fold.xpl, y1a, y1b);
                    xo_x[t] = dp_to_word(dp_mulmod(x1a, y1a, d));
                    xo_y[t] = dp_to_word(dp_mulmod(x1b, y1b, d));
                }
                if constexpr (DPL) {   // in the register form of a pair read from the planes: one conversion for every digit
                    const u64 a = (u64)xo_x[t], b = (u64)xo_y[t];
                    xo_x[t] = (i64)((a & 0xffffffffull) | (b << 32));
                    xo_y[t] = (i64)((a >> 32) | ((b >> 32) << 16));
                }
            }
        }
#pragma unroll KI_UNROLL
        for (int p = 0; p < nparts; ++p) {
            longlong2 x[NCT];   // DPL: .x = the two low words, low half of .y = the two high halves (8 + 4 bytes, fwd_tile16<.., PLN>)
            if constexpr (DPL) {   // SGPR row base + one per-thread byte offset per plane
#pragma unroll
                for (int t = 0; t < NCT; ++t) {
                    const char *er = reinterpret_cast<const char *>(uniform_ptr(ext + (((i64)t * nparts + p) * rows + r) * N));
                    if (p == p_own) {
                        x[t].x = xo_x[t], x[t].y = xo_y[t];
                    } else {
                        x[t].x = *reinterpret_cast<const i64 *>(er + bo_lo);
                        x[t].y = (i64)*reinterpret_cast<const unsigned *>(er + 4 * N + bo_hi);
                    }
                }
            } else {
#pragma unroll
                for (int t = 0; t < NCT; ++t) {
                    if (p == p_own) {
                        x[t].x = xo_x[t], x[t].y = xo_y[t];
                    } else {
                        const longlong2 v = *reinterpret_cast<const longlong2 *>(e + t * ct_ext + (i64)p * rows * N);
                        x[t].x = v.x, x[t].y = v.y;
                    }
                }
            }
            double k0x, k0y, k1x, k1y;
            if (PLANES) {   // 16 + 8 bytes for both components (see lf_key_planes)
                const i64 *kr = k - j0 + (i64)p * part_stride;
                const lf_u4_t l = __builtin_nontemporal_load(reinterpret_cast<const lf_u4_t *>(reinterpret_cast<const unsigned *>(kr) + 2 * j0));
                const lf_u2_t h = __builtin_nontemporal_load(reinterpret_cast<const lf_u2_t *>(reinterpret_cast<const unsigned *>(kr + comp_stride) + j0));
                k0x = dp_from_planes(l.x, h.x & 0xffffu), k0y = dp_from_planes(l.y, h.x >> 16);
                k1x = dp_from_planes(l.z, h.y & 0xffffu), k1y = dp_from_planes(l.w, h.y >> 16);
            } else {
                const longlong2 k0 = ld_nt(k + (i64)p * part_stride);
                const longlong2 k1 = ld_nt(k + (i64)p * part_stride + comp_stride);
                k0x = dp_from_word(k0.x), k0y = dp_from_word(k0.y), k1x = dp_from_word(k1.x), k1y = dp_from_word(k1.y);
            }
#pragma unroll
            for (int t = 0; t < NCT; ++t) {
                double x0, x1;
                if constexpr (DPL) {
                    const unsigned h = (unsigned)x[t].y;
                    x0 = dp_from_planes((unsigned)x[t].x, h & 0xffffu);
                    x1 = dp_from_planes((unsigned)((u64)x[t].x >> 32), h >> 16);
                } else {
                    x0 = dp_from_word(x[t].x), x1 = dp_from_word(x[t].y);
                }
                acc[t][0][0] += dp_mulmod_bal(x0, k0x, d);
                acc[t][0][1] += dp_mulmod_bal(x1, k0y, d);
                acc[t][1][0] += dp_mulmod_bal(x0, k1x, d);
                acc[t][1][1] += dp_mulmod_bal(x1, k1y, d);
            }
        }
        if (FOLD && r < fold.ell) {
            const double pr = dp_from_word(fold.PR[r]);
            const i64 pstride = (i64)fold.ell * N;
#pragma unroll
            for (int t = 0; t < NCT; ++t) {
                if constexpr (PRESUM) {   // plain canonical words: one product with PR each
                    const longlong2 T0 = *reinterpret_cast<const longlong2 *>(fold.x + t * fold.ct_stride + (i64)r * N + j0);
                    const longlong2 T1 = *reinterpret_cast<const longlong2 *>(fold.x + t * fold.ct_stride + pstride + (i64)r * N + j0);
                    acc[t][0][0] += dp_mulmod_bal(dp_from_word(T0.x), pr, d);
                    acc[t][0][1] += dp_mulmod_bal(dp_from_word(T0.y), pr, d);
                    acc[t][1][0] += dp_mulmod_bal(dp_from_word(T1.x), pr, d);
                    acc[t][1][1] += dp_mulmod_bal(dp_from_word(T1.y), pr, d);
                    continue;
                }
                const i64 *xs = fold.x + t * fold.ct_stride + (i64)r * N;
                double x0[2], x1[2], y0[2], y1[2];
                ld_pair_dp(xs, j0, N, fold.xpl, x0[0], x0[1]);
                ld_pair_dp(xs + pstride, j0, N, fold.xpl, x1[0], x1[1]);
                ld_pair_dp(xs + 2 * pstride, j0, N, fold.xpl, y0[0], y0[1]);
                ld_pair_dp(xs + 3 * pstride, j0, N, fold.xpl, y1[0], y1[1]);
#pragma unroll
                for (int e = 0; e < 2; ++e) {   // balanced terms: |d0| <= q / 2, |d1| <= q
                    const double d0 = dp_mulmod_bal(x0[e], y0[e], d);
                    const double d1 = dp_mulmod_bal(x0[e], y1[e], d) + dp_mulmod_bal(x1[e], y0[e], d);
                    acc[t][0][e] += dp_mulmod_bal(d0, pr, d);
                    acc[t][1][e] += dp_mulmod_bal(d1, pr, d);
                }
            }
        }
#pragma unroll
        for (int t = 0; t < NCT; ++t)
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                longlong2 o;
                o.x = dp_to_word(dp_reduce(acc[t][c][0], d.q, d.qinv));
                o.y = dp_to_word(dp_reduce(acc[t][c][1], d.q, d.qinv));
                i64 *srow = s + t * ct_s + ((i64)c * rows + r) * N;
                if (spl) {
                    const lf_u2_t l = {(unsigned)o.x, (unsigned)o.y};
                    *reinterpret_cast<lf_u2_t *>(reinterpret_cast<unsigned *>(srow) + j0) = l;
                    *reinterpret_cast<unsigned *>(reinterpret_cast<unsigned short *>(srow + (N >> 1)) + j0) =
                        (unsigned)((u64)o.x >> 32) | ((unsigned)((u64)o.y >> 32) << 16);
                } else {
                    *reinterpret_cast<longlong2 *>(srow + j0) = o;
                }
            }
    } else {
        i64 acc[NCT][2][2];
#pragma unroll
        for (int t = 0; t < NCT; ++t) acc[t][0][0] = acc[t][0][1] = acc[t][1][0] = acc[t][1][1] = 0;
        const int p_own = (FOLD && fold.own != nullptr && r < fold.ell) ? (int)fold.own[r] : -1;
        i64 xo_x[NCT], xo_y[NCT];   // the own digit's words: REDC62(x1 * y1), Montgomery form below 2q (scalars: see above)
        if (p_own >= 0) {
#pragma unroll
            for (int t = 0; t < NCT; ++t) {
                if constexpr (PRESUM) {
                    const longlong2 T2 = *reinterpret_cast<const longlong2 *>(fold.x + t * fold.ct_stride + (2 * (i64)fold.ell + r) * N + j0);
                    xo_x[t] = T2.x, xo_y[t] = T2.y;
                } else {
                    const i64 *xs = fold.x + t * fold.ct_stride + (i64)r * N + j0 + (i64)fold.ell * N;
                    const longlong2 X1 = *reinterpret_cast<const longlong2 *>(xs), Y1 = *reinterpret_cast<const longlong2 *>(xs + 2 * (i64)fold.ell * N);
                    xo_x[t] = mm62u((u64)X1.x, (u64)Y1.x, m.q, m.k);
                    xo_y[t] = mm62u((u64)X1.y, (u64)Y1.y, m.q, m.k);
                }
            }
        }
        for (int p = 0; p < nparts; ++p) {
            const longlong2 k0 = ld_nt(k + (i64)p * part_stride);
            const longlong2 k1 = ld_nt(k + (i64)p * part_stride + comp_stride);
#pragma unroll
            for (int t = 0; t < NCT; ++t) {
                longlong2 x;
                if (p == p_own) {
                    x.x = xo_x[t], x.y = xo_y[t];
                } else {
                    const longlong2 v = *reinterpret_cast<const longlong2 *>(e + t * ct_ext + (i64)p * rows * N);
                    x.x = v.x, x.y = v.y;
                }
                acc[t][0][0] = csub(acc[t][0][0] + mm62u((u64)x.x, (u64)k0.x, m.q, m.k), m.q2);
                acc[t][0][1] = csub(acc[t][0][1] + mm62u((u64)x.y, (u64)k0.y, m.q, m.k), m.q2);
                acc[t][1][0] = csub(acc[t][1][0] + mm62u((u64)x.x, (u64)k1.x, m.q, m.k), m.q2);
                acc[t][1][1] = csub(acc[t][1][1] + mm62u((u64)x.y, (u64)k1.y, m.q, m.k), m.q2);
            }
        }
        if (FOLD && r < fold.ell) {
            const u64 pr = (u64)fold.PR[r];
            const i64 pstride = (i64)fold.ell * N;
#pragma unroll
            for (int t = 0; t < NCT; ++t) {
                if constexpr (PRESUM) {   // Montgomery-form words below 2q
                    const longlong2 T0 = *reinterpret_cast<const longlong2 *>(fold.x + t * fold.ct_stride + (i64)r * N + j0);
                    const longlong2 T1 = *reinterpret_cast<const longlong2 *>(fold.x + t * fold.ct_stride + pstride + (i64)r * N + j0);
                    acc[t][0][0] = csub(acc[t][0][0] + mm62u((u64)T0.x, pr, m.q, m.k), m.q2);
                    acc[t][0][1] = csub(acc[t][0][1] + mm62u((u64)T0.y, pr, m.q, m.k), m.q2);
                    acc[t][1][0] = csub(acc[t][1][0] + mm62u((u64)T1.x, pr, m.q, m.k), m.q2);
                    acc[t][1][1] = csub(acc[t][1][1] + mm62u((u64)T1.y, pr, m.q, m.k), m.q2);
                    continue;
                }
                const i64 *xs = fold.x + t * fold.ct_stride + (i64)r * N + j0;
                const longlong2 X0 = *reinterpret_cast<const longlong2 *>(xs), X1 = *reinterpret_cast<const longlong2 *>(xs + pstride);
                const longlong2 Y0 = *reinterpret_cast<const longlong2 *>(xs + 2 * pstride), Y1 = *reinterpret_cast<const longlong2 *>(xs + 3 * pstride);
                const u64 x0[2] = {(u64)X0.x, (u64)X0.y}, x1[2] = {(u64)X1.x, (u64)X1.y};
                const u64 y0[2] = {(u64)Y0.x, (u64)Y0.y}, y1[2] = {(u64)Y1.x, (u64)Y1.y};
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const i64 d0 = mm62u(x0[e], y0[e], m.q, m.k);
                    const i64 d1 = csub(mm62u(x0[e], y1[e], m.q, m.k) + mm62u(x1[e], y0[e], m.q, m.k), m.q2);
                    acc[t][0][e] = csub(acc[t][0][e] + mm62u((u64)d0, pr, m.q, m.k), m.q2);
                    acc[t][1][e] = csub(acc[t][1][e] + mm62u((u64)d1, pr, m.q, m.k), m.q2);
                }
            }
        }
#pragma unroll
        for (int t = 0; t < NCT; ++t)
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                longlong2 o;
                o.x = acc[t][c][0];
                o.y = acc[t][c][1];
                *reinterpret_cast<longlong2 *>(s + t * ct_s + ((i64)c * rows + r) * N + j0) = o;
            }
    }
