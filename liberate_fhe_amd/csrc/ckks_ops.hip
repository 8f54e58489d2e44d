// ckks_ops.hip — whole engine ops behind ONE C entry each: lf_cc_mult_evk, lf_switch_key.
//
// The reference issues a cc_mult + relinearize as ~250 Python-level calls into its extension (ckks_engine.py:1072-1151,
// 746-961); this library's engine brought that down to a dozen fused launches, but each still cost a Python -> ctypes
// round trip with twenty-odd marshalled arguments (117 us of host time per silver cc_mult, more than the device time of
// a rank of the limb-sharded path).  Here the launches of an op are enqueued by one native call: everything that does
// not change between calls — constants, twiddle tables, key-switch descriptors, scratch — sits in an `lf_ks_plan` the
// caller fills once per (device, level).  The entries only compose the library's own exported steps (same kernels, same
// results); they apply when every limb of the level lives on this device (no exchange step in the middle).
#include "../../include/ckks_hip.h"
#include "ckks_common.h"
#include "ckks_launch.h"

#include <vector>

// what always travels together into the launchers of ckks_ks.hip (ckks_launch.h), from the plan
static LfMod plan_mod(const lf_ks_plan *p) { return {p->ql, p->qh, p->kl, p->kh, p->q_host}; }
static LfFwdTab plan_fwd(const lf_ks_plan *p) { return {p->psi, p->psi_dp}; }
static LfInvTab plan_inv(const lf_ks_plan *p) { return {p->ipsi, p->ipsi_dp, p->Ninv}; }

extern "C" {

static int plan_ok(const lf_ks_plan *p) {
    return p && p->logN > NTT_TILE_LOG_MAX && p->logN <= KS_LOGN_MAX && p->ell >= 1 && p->K >= 1 && p->K <= KS_MAX_K &&
           p->nparts >= 1 && p->dig_nparts >= 0 && p->max_nct >= 1 && p->ql && p->qh && p->kl && p->kh && p->_2q && p->Rs && p->Ninv && p->q_host &&
           p->psi && p->ipsi && p->psi_dp && p->ipsi_dp && p->dig_desc && p->dig_tab && p->ext_desc && p->E && p->Ed && p->PiR &&
           p->state && p->ext && p->sum && p->md_ws &&
           // (every op behind a plan ends in an fp64-class inner product where a row is of that class: refused here, before any launch)
           p->ell + p->K <= MAX_LIST_ROWS && lf_fp64_digits_ok(p->nparts, p->ell + p->K, p->q_host);
}

// cc_mult's operand stack x4 in planes format (include/ckks_hip.h LF_NTT_PLANES): decided per call from lf_tune's knob; the pieces
// of a sharded op are separate calls, and a stack written under one setting is refused by a reader under the other (LF_ERR_STATE)
static int stack_planes(const lf_ks_plan *p) { return lf_stack_planes(p->logN, p->ell, p->q_host); }

static int batch_ok(const lf_ks_plan *p, int nct) {
    return plan_ok(p) && (nct == 1 || nct == 2 || nct == 4) && nct <= p->max_nct;
}

static int moddown_any(const lf_ks_plan *p, const int64_t *const *ss, int64_t *const *outs, const int64_t *const *adds, int count,
                       int64_t gal_pinv, const int64_t *g2q, void *stream) {
    const int64_t N = (int64_t)1 << p->logN;
    // up to two special primes (bronze, silver): the elimination among the special rows is at most one product per
    // coefficient — done inside the mod-down launch (lf_ks_moddown_one), which only READS the level constants
    // lf_ks_moddown_consts wrote behind the pivots of `md_consts` polynomials.  A plan whose workspace was never primed
    // (md_consts = 0) or primed for another count takes the two-launch form, which writes them where its own count puts them.
    if (p->K <= LF_MODDOWN_ONE_MAX_K && count == p->md_consts)
        return lf_ks_moddown_one(ss, outs, adds, count, p->ell, p->K, N, p->md_ws, p->md_ws_words, p->PiR, p->PiP, p->Rs, gal_pinv, g2q,
                                 p->ql, p->qh, p->kl, p->kh, p->device, stream);
    return lf_ks_moddown_ws(ss, outs, adds, count, p->ell, p->K, N, p->md_ws, p->md_ws_words, p->PiR, p->PiP, p->Rs, gal_pinv, g2q, p->ql,
                            p->qh, p->kl, p->kh, p->device, stream);
}

// one mod-down of n (<= 4) pairs of sums [n][2][rows][N] at `sums` into the pairs out0[t], out1[t]; c0 (may be NULL): c0[t] (may be
// NULL) joins component 0 of pair t, through the Galois map gal_pinv where that is set
static int moddown_pairs(const lf_ks_plan *p, const int64_t *sums, int n, int64_t *const *out0, int64_t *const *out1,
                         const int64_t *const *c0, int64_t gal_pinv, const int64_t *g2q, void *stream) {
    const int64_t half = (int64_t)(p->ell + p->K) << p->logN;
    const int64_t *ss[8], *adds[8];
    int64_t *outs[8];
    for (int t = 0; t < n; ++t) {
        ss[2 * t] = sums + (2 * t) * half, ss[2 * t + 1] = sums + (2 * t + 1) * half;
        outs[2 * t] = out0[t], outs[2 * t + 1] = out1[t];
        adds[2 * t] = c0 ? c0[t] : nullptr, adds[2 * t + 1] = nullptr;
    }
    return moddown_any(p, ss, outs, c0 ? adds : nullptr, 2 * n, gal_pinv, g2q, stream);
}

// .. into md [n][2][ell][N] instead, then ONE rescale of the 2 n polynomials into the pairs out0[t], out1[t] of [ell - 1][N]; the
// mod-down runs in the workspace mdws (a count the plan's own is not primed for), or in the plan's own where mdws is NULL
static int moddown_rescale_pairs(const lf_ks_plan *p, const int64_t *sums, int n, int64_t *md, int64_t *mdws, int64_t mdws_words,
                                 int64_t *const *out0, int64_t *const *out1, const int64_t *rescale_scales, int64_t round_at,
                                 void *stream) {
    const int ell = p->ell;
    const int64_t N = (int64_t)1 << p->logN, poly = (int64_t)ell * N, half = (int64_t)(ell + p->K) * N;
    const int64_t *ss[8], *ins[8], *row0[8];
    int64_t *mds[8], *outs[8];
    for (int t = 0; t < 2 * n; ++t) {
        ss[t] = sums + t * half;
        mds[t] = md + t * poly, row0[t] = mds[t], ins[t] = mds[t] + N;
        outs[t] = (t & 1) ? out1[t / 2] : out0[t / 2];
    }
    if (int e = mdws ? lf_ks_moddown_ws(ss, mds, nullptr, 2 * n, ell, p->K, N, mdws, mdws_words, p->PiR, p->PiP, p->Rs, 0, nullptr, p->ql,
                                        p->qh, p->kl, p->kh, p->device, stream)
                     : moddown_any(p, ss, mds, nullptr, 2 * n, 0, nullptr, stream))
        return e;
    return lf_rescale_batch(ins, row0, outs, 2 * n, ell - 1, N, rescale_scales, round_at, p->ql + 1, p->qh + 1, p->kl + 1, p->kh + 1,
                            p->device, stream);
}

// P NTT(c) of n (<= 8) polynomials srcs[i] on the plan's ordinary rows into base + i * stride: a canonical copy, enter_ntt (exact:
// lazy Montgomery words below 2q on rows of both classes, what the kernels add unreduced), times P R.  ONE forward transform
// where the results lie back to back (stride = ell N), one per polynomial otherwise
static int p_ntt(const lf_ks_plan *p, const int64_t *const *srcs, int n, int64_t *base, int64_t stride, void *stream) {
    const int ell = p->ell, logN = p->logN, dev = p->device;
    const int64_t N = (int64_t)1 << logN;
    const bool packed = stride == (int64_t)ell * N;
    int64_t *dsts[8];
    if (n < 1 || n > 8) return LF_ERR_ARG;
    for (int i = 0; i < n; ++i) dsts[i] = base + i * stride;
    if (int e = lf_galois_batch(srcs, dsts, n, ell, logN, 1, p->_2q, dev, stream)) return e;
    if (packed)
        if (int e = lf_ntt(base, n, ell, logN, p->psi, p->psi_dp, p->q_host, p->Rs, 0, p->_2q, p->ql, p->qh, p->kl, p->kh, dev, stream))
            return e;
    for (int i = 0; i < n; ++i) {
        if (!packed)
            if (int e = lf_ntt(dsts[i], 1, ell, logN, p->psi, p->psi_dp, p->q_host, p->Rs, 0, p->_2q, p->ql, p->qh, p->kl, p->kh, dev, stream))
                return e;
        if (int e = lf_mont_enter(dsts[i], p->PR, ell, N, p->ql, p->qh, p->kl, p->kh, dev, stream)) return e;
    }
    return 0;
}

// d2 = x1 * y1 -> inverse transform -> digits of the plan's `nct` operand stacks: in ONE launch behind the tiled pass where a
// digit's limbs fit a column thread (lf_intt_mul_digits: silver, bronze), else the inverse transform and lf_ks_digits(_batch)
static int product_digits(const lf_ks_plan *p, int nct, void *stream) {
    const int ell = p->ell, logN = p->logN, dev = p->device;
    const int64_t N = (int64_t)1 << logN, poly = (int64_t)ell * N;
    const int relaxed_plain = LF_NTT_RELAXED | LF_NTT_PLAIN | (stack_planes(p) ? LF_NTT_PLANES : 0);
    const int64_t xs = nct > 1 ? 4 * poly : poly;   // stride between the operand stacks of a batch
    const int e = !lf_g_intt_digits ? LF_ERR_ARG : lf_intt_mul_digits(p->d2, p->x4 + poly, xs, p->x4 + 3 * poly, xs, nct, ell, logN, p->state, p->dig_nparts, p->K, p->dig_desc,
                                     p->dig_tab, p->ipsi, p->ipsi_dp, p->q_host, p->Ninv, relaxed_plain, p->ql, p->qh, p->kl, p->kh, dev, stream);
    if (e != LF_ERR_ARG) return e;   // launched (0) or a runtime error; LF_ERR_ARG: the shape does not qualify, nothing was launched
    if (int e2 = lf_intt_mul(p->d2, p->x4 + poly, xs, p->x4 + 3 * poly, xs, nct, ell, logN, p->ipsi, p->ipsi_dp, p->q_host, p->Ninv, 2,
                             relaxed_plain, p->ql, p->qh, p->kl, p->kh, dev, stream))
        return e2;
    if (nct == 1)
        return lf_ks_digits(p->d2, p->state, p->dig_nparts, p->dig_desc, p->dig_tab, N, p->ql, p->qh, p->kl, p->kh, dev, stream);
    const int64_t *srcs[4];
    int64_t *states[4];
    for (int t = 0; t < nct; ++t) srcs[t] = p->d2 + t * poly, states[t] = p->state + t * poly;
    return lf_ks_digits_batch(srcs, states, nct, p->dig_nparts, p->dig_desc, p->dig_tab, N, 0, nullptr, p->ql, p->qh, p->kl, p->kh, dev, stream);
}

int lf_cc_mult_evk(const lf_ks_plan *p, const int64_t *const *in, const int64_t *const *row0, const int64_t *ksk,
                   int64_t part_stride, int64_t comp_stride, int64_t row_off, int key_format, int64_t *out0, int64_t *out1,
                   void *stream) {
    if (!plan_ok(p) || !p->rescale_scales || !p->PR || !p->x4 || !p->d2 || !in || !row0 || !ksk || !out0 || !out1) return LF_ERR_ARG;
    const int ell = p->ell, rows = p->ell + p->K, logN = p->logN, dev = p->device;
    const int64_t N = (int64_t)1 << logN, poly = (int64_t)ell * N;
    const int xpl = stack_planes(p);
    const int relaxed_plain = LF_NTT_RELAXED | LF_NTT_PLAIN | (xpl ? LF_NTT_PLANES : 0);
    // x0, x1, y0, y1: both rescales inside the first pass of one batched forward transform (ckks_engine.py:1085-1093)
    if (int e = lf_rescale_ntt(in, row0, 4, p->x4, ell, logN, p->rescale_scales, p->round_at, p->psi, p->psi_dp, p->q_host, p->Rs,
                               relaxed_plain, p->_2q, p->ql, p->qh, p->kl, p->kh, dev, stream))
        return e;
    // d2 = x1 * y1 straight into its inverse transform (1099-1101, 1129), its digits (654-705)
    if (int e = product_digits(p, 1, stream)) return e;
    // key switch of d2 with d0, d1 folded into its sums (654-961, 1117-1151)
    if (int e = lf_relin_core_batch(p->state, 0, 1, p->nparts, rows, logN, p->ext_desc, p->E, p->Ed, ksk, part_stride, comp_stride,
                                    row_off, key_format | (xpl ? LF_STACK_PLANES : 0), p->ext, p->sum, p->psi, p->psi_dp, p->ipsi, p->ipsi_dp, p->Ninv, p->x4, 0, p->PR, ell,
                                    p->own, p->q_host, p->ql, p->qh, p->kl, p->kh, dev, stream))
        return e;
    return moddown_pairs(p, p->sum, 1, &out0, &out1, nullptr, 0, nullptr, stream);
}

/* ---- cc_dot: sum_i a_i * b_i under ONE relinearisation (include/ckks_hip.h).  Everything of a cc_mult but the tensor products is
 * linear in the triplet (d0, d1, d2), so the triplets are summed in the NTT domain and the inverse transform, the digits, their
 * extension, the inner product with the key, the sums' inverse transform and the mod-down run once, on the sum. ---- */
static int dot_ok(const lf_ks_plan *p) { return plan_ok(p) && p->rescale_scales && p->PR && p->x4 && p->d2; }

// the accumulated triplet T = [3][ell][N]
int64_t lf_cc_dot_ws_words(const lf_ks_plan *p) {
    if (!dot_ok(p)) return 0;
    return ((int64_t)3 * p->ell) << p->logN;
}

// steps 1 and 2 of lf_cc_dot for one dot: the tensor products of its np pairs summed into the triplet T; a copy of T2 into t2
static int dot_triplet(const lf_ks_plan *p, int np, const int64_t *const *in, const int64_t *const *row0, int64_t *T, int64_t *t2,
                       void *stream) {
    const int ell = p->ell, logN = p->logN, dev = p->device;
    const int64_t poly = (int64_t)ell << logN;
    const int xpl = stack_planes(p);
    const int relaxed_plain = LF_NTT_RELAXED | LF_NTT_PLAIN | (xpl ? LF_NTT_PLANES : 0);
    const int gmax = p->max_nct >= 4 ? 4 : p->max_nct >= 2 ? 2 : 1;
    for (int i0 = 0; i0 < np;) {
        const int left = np - i0;
        const int g = left >= 4 && gmax >= 4 ? 4 : left >= 2 && gmax >= 2 ? 2 : 1;
        // 1. x0, x1, y0, y1 of the chunk's pairs: rescale inside the forward transform, two pairs (8 polynomials) per call
        for (int t0 = 0; t0 < g; t0 += 2) {
            const int n = g - t0 < 2 ? g - t0 : 2;
            if (int e = lf_rescale_ntt(in + 4 * (i0 + t0), row0 + 4 * (i0 + t0), 4 * n, p->x4 + (int64_t)t0 * 4 * poly, ell, logN,
                                       p->rescale_scales, p->round_at, p->psi, p->psi_dp, p->q_host, p->Rs, relaxed_plain, p->_2q, p->ql,
                                       p->qh, p->kl, p->kh, dev, stream))
                return e;
        }
        // 2. their tensor products into the one triplet; the last launch leaves a copy of T2 where its inverse transform runs
        if (int e = lf_dot_tensor(g, p->x4, T, i0 + g == np ? t2 : nullptr, ell, logN, xpl, i0 == 0, plan_mod(p), (hipStream_t)stream)) return e;
        i0 += g;
    }
    return 0;
}

// steps 3 to 5 of lf_cc_dot (nd = 1) resp. lf_cc_dot_batch (nd = 2, 4) on nd summed triplets at T, their T2 copies in plan->d2
static int dot_tail(const lf_ks_plan *p, int nd, const int64_t *T, const LfKeys &key, int64_t *const *out0, int64_t *const *out1,
                    void *stream) {
    const int ell = p->ell, rows = p->ell + p->K, logN = p->logN, dev = p->device;
    const int64_t N = (int64_t)1 << logN, poly = (int64_t)ell * N;
    // 3. the nd copies of T2 -> canonical coefficients in one inverse transform (the words lf_intt_mul leaves), their digits in one launch
    if (int e = lf_intt(p->d2, nd, ell, logN, p->ipsi, p->ipsi_dp, p->q_host, p->Ninv, 2, LF_NTT_RELAXED | LF_NTT_PLAIN, p->_2q, p->ql, p->qh,
                        p->kl, p->kh, dev, stream))
        return e;
    if (nd == 1) {
        if (int e = lf_ks_digits(p->d2, p->state, p->dig_nparts, p->dig_desc, p->dig_tab, N, p->ql, p->qh, p->kl, p->kh, dev, stream)) return e;
    } else {
        const int64_t *srcs[4];
        int64_t *states[4];
        for (int d = 0; d < nd; ++d) srcs[d] = p->d2 + d * poly, states[d] = p->state + d * poly;
        if (int e = lf_ks_digits_batch(srcs, states, nd, p->dig_nparts, p->dig_desc, p->dig_tab, N, 0, nullptr, p->ql, p->qh, p->kl, p->kh,
                                       dev, stream))
            return e;
    }
    // 4. the key switch of the nd T2 with P T0, P T1 folded into their sums, own-limb digit words from T2: every key word read once
    if (int e = lf_dot_relin(p->state, nd, p->nparts, rows, logN, p->ext_desc, p->E, p->Ed, key, p->ext, p->sum, plan_fwd(p), plan_inv(p), T,
                             p->PR, ell, p->own, plan_mod(p), (hipStream_t)stream))
        return e;
    // 5. one mod-down of the 2 nd sums, no addend
    return moddown_pairs(p, p->sum, nd, out0, out1, nullptr, 0, nullptr, stream);
}

int lf_cc_dot(const lf_ks_plan *p, int np, const int64_t *const *in, const int64_t *const *row0, const int64_t *ksk,
              int64_t part_stride, int64_t comp_stride, int64_t row_off, int key_format, int64_t *ws, int64_t ws_words, int64_t *out0,
              int64_t *out1, void *stream) {
    const LfKeys key{&ksk, 1, part_stride, comp_stride, row_off, key_format};
    if (!dot_ok(p) || np < 1 || !in || !row0 || !out0 || !out1 || !lf_keys_ok(key)) return LF_ERR_ARG;
    for (int64_t i = 0; i < (int64_t)4 * np; ++i)
        if (!in[i] || !row0[i]) return LF_ERR_ARG;
    const int64_t need = lf_cc_dot_ws_words(p);
    if (need && (!ws || ws_words < need || ((uintptr_t)ws & 15))) return LF_ERR_ARG;   // (dot_tensor_kernel: 16-byte column pairs of T)
    if (int e = lf_set_device(p->device)) return e;
    // 1., 2. the pairs' tensor products into the one triplet
    if (int e = dot_triplet(p, np, in, row0, ws, p->d2, stream)) return e;
    return dot_tail(p, 1, ws, key, &out0, &out1, stream);
}

/* ---- cc_dot_batch: nd = 1, 2 or 4 independent dots under ONE key (include/ckks_hip.h): lf_cc_dot's launches with everything behind
 * the tensor products covering all nd summed triplets, the key read once for them. ---- */
int64_t lf_cc_dot_batch_ws_words(const lf_ks_plan *p, int nd) {
    if (!dot_ok(p) || !batch_ok(p, nd)) return 0;
    return ((int64_t)3 * nd * p->ell) << p->logN;
}

int lf_cc_dot_batch(const lf_ks_plan *p, int nd, const int64_t *np_host, const int64_t *const *in, const int64_t *const *row0,
                    const int64_t *ksk, int64_t part_stride, int64_t comp_stride, int64_t row_off, int key_format, int64_t *ws,
                    int64_t ws_words, int64_t *const *out0, int64_t *const *out1, void *stream) {
    const LfKeys key{&ksk, 1, part_stride, comp_stride, row_off, key_format};
    if (!dot_ok(p) || !batch_ok(p, nd) || !np_host || !in || !row0 || !out0 || !out1 || !lf_keys_ok(key)) return LF_ERR_ARG;
    int64_t pairs = 0;
    for (int d = 0; d < nd; ++d) {
        if (np_host[d] < 1 || np_host[d] > INT32_MAX || !out0[d] || !out1[d]) return LF_ERR_ARG;
        pairs += np_host[d];
    }
    for (int64_t i = 0; i < 4 * pairs; ++i)
        if (!in[i] || !row0[i]) return LF_ERR_ARG;
    const int64_t need = lf_cc_dot_batch_ws_words(p, nd);
    if (!ws || ws_words < need || ((uintptr_t)ws & 15)) return LF_ERR_ARG;
    if (nd == 1)
        return lf_cc_dot(p, (int)np_host[0], in, row0, ksk, part_stride, comp_stride, row_off, key_format, ws, ws_words, out0[0], out1[0],
                         stream);
    const int64_t poly = (int64_t)p->ell << p->logN;
    if (int e = lf_set_device(p->device)) return e;
    // 1., 2. per dot: its pairs' tensor products into its triplet T_d; the copy of T2_d into slot d of plan->d2
    int64_t first = 0;
    for (int d = 0; d < nd; ++d) {
        if (int e = dot_triplet(p, (int)np_host[d], in + 4 * first, row0 + 4 * first, ws + d * 3 * poly, p->d2 + d * poly, stream)) return e;
        first += np_host[d];
    }
    return dot_tail(p, nd, ws, key, out0, out1, stream);
}

/* ---- cc_matmul: C = A B over ciphertexts under ONE key (include/ckks_hip.h): every distinct operand transformed once into a
 * resident store, the triplets of a tile of outputs summed over the whole inner dimension in one launch, and lf_cc_dot_batch's
 * steps behind the tensor products per tile. ---- */
static int matmul_group(const lf_ks_plan *p) { return p->max_nct >= 4 ? 4 : p->max_nct >= 2 ? 2 : 1; }

int64_t lf_cc_matmul_ws_words(const lf_ks_plan *p, int nu) {
    if (!dot_ok(p) || nu < 1 || nu > LF_CC_MATMUL_MAX_OPERANDS) return 0;
    return ((int64_t)(2 * nu + 3 * matmul_group(p)) * p->ell) << p->logN;
}

struct MatmulTile {
    int i0, j0, R, C;
};

// a strip of `len` outputs from (i0, j0), along a row (1 x g tiles) or down a column (g x 1): g = 4, 2, 1, at most gmax
static void matmul_strip(std::vector<MatmulTile> &tiles, int i0, int j0, int len, bool along_row, int gmax) {
    for (int s = 0; s < len;) {
        const int left = len - s, g = left >= 4 && gmax >= 4 ? 4 : left >= 2 && gmax >= 2 ? 2 : 1;
        tiles.push_back(along_row ? MatmulTile{i0, j0 + s, 1, g} : MatmulTile{i0 + s, j0, g, 1});
        s += g;
    }
}

// the tiling of an m x n matrix of outputs (encdec.cc_matmul_tiles is the same rule): 2 x 2 where both dimensions allow it and a
// tile may hold 4 outputs; strips along a vector, an odd last column and an odd last row
static void matmul_tiles(std::vector<MatmulTile> &tiles, int m, int n, int gmax) {
    if (n == 1 && m > 1) {
        matmul_strip(tiles, 0, 0, m, false, gmax);
    } else if (m == 1 || gmax < 4) {
        for (int i = 0; i < m; ++i) matmul_strip(tiles, i, 0, n, true, gmax);
    } else {
        const int m2 = m & ~1, n2 = n & ~1;
        for (int i = 0; i < m2; i += 2)
            for (int j = 0; j < n2; j += 2) tiles.push_back(MatmulTile{i, j, 2, 2});
        if (n & 1) matmul_strip(tiles, 0, n - 1, m, false, gmax);
        if (m & 1) matmul_strip(tiles, m - 1, 0, n2, true, gmax);
    }
}

int lf_cc_matmul(const lf_ks_plan *p, int m, int k, int n, int nu, const int64_t *const *in, const int64_t *const *row0,
                 const int64_t *ia, const int64_t *ib, const int64_t *ksk, int64_t part_stride, int64_t comp_stride, int64_t row_off,
                 int key_format, int64_t *ws, int64_t ws_words, int64_t *const *out0, int64_t *const *out1, void *stream) {
    const LfKeys key{&ksk, 1, part_stride, comp_stride, row_off, key_format};
    if (!dot_ok(p) || m < 1 || k < 1 || n < 1 || k > LF_CC_MATMUL_MAX_INNER || nu < 1 || nu > LF_CC_MATMUL_MAX_OPERANDS || !in || !row0 ||
        !ia || !ib || !out0 || !out1 || !lf_keys_ok(key))
        return LF_ERR_ARG;
    if ((int64_t)m * k > INT32_MAX || (int64_t)k * n > INT32_MAX || (int64_t)m * n > INT32_MAX) return LF_ERR_ARG;
    std::vector<char> used((size_t)nu, 0);
    for (int64_t i = 0; i < (int64_t)m * k; ++i) {
        if (ia[i] < -1 || ia[i] >= nu) return LF_ERR_ARG;
        if (ia[i] >= 0) used[(size_t)ia[i]] = 1;
    }
    for (int64_t i = 0; i < (int64_t)k * n; ++i) {
        if (ib[i] < -1 || ib[i] >= nu) return LF_ERR_ARG;
        if (ib[i] >= 0) used[(size_t)ib[i]] = 1;
    }
    for (int u = 0; u < nu; ++u)   // every operand of the store is transformed: one that nothing uses is a mistake of the caller's
        if (!used[(size_t)u] || !in[2 * u] || !in[2 * u + 1] || !row0[2 * u] || !row0[2 * u + 1]) return LF_ERR_ARG;
    for (int i = 0; i < m; ++i)
        for (int j = 0; j < n; ++j) {
            bool term = false;
            for (int t = 0; t < k && !term; ++t) term = ia[(int64_t)i * k + t] >= 0 && ib[(int64_t)t * n + j] >= 0;
            if (!term || !out0[(int64_t)i * n + j] || !out1[(int64_t)i * n + j]) return LF_ERR_ARG;
        }
    const int64_t need = lf_cc_matmul_ws_words(p, nu);
    if (!ws || ws_words < need || ((uintptr_t)ws & 15)) return LF_ERR_ARG;
    const int ell = p->ell, logN = p->logN, dev = p->device;
    const int64_t poly = (int64_t)ell << logN;
    const int xpl = stack_planes(p);
    const int relaxed_plain = LF_NTT_RELAXED | LF_NTT_PLAIN | (xpl ? LF_NTT_PLANES : 0);
    if (int e = lf_set_device(dev)) return e;
    // 1. the store: c0, c1 of every distinct operand, rescale inside the forward transform, 4 operands (8 polynomials) per call
    int64_t *store = ws, *T = ws + (int64_t)2 * nu * poly;
    for (int u0 = 0; u0 < nu; u0 += 4) {
        const int g = nu - u0 < 4 ? nu - u0 : 4;
        if (int e = lf_rescale_ntt(in + 2 * u0, row0 + 2 * u0, 2 * g, store + (int64_t)2 * u0 * poly, ell, logN, p->rescale_scales, p->round_at,
                                   p->psi, p->psi_dp, p->q_host, p->Rs, relaxed_plain, p->_2q, p->ql, p->qh, p->kl, p->kh, dev, stream))
            return e;
    }
    // 2., 3. per tile: its summed triplets in one launch, then everything behind the tensor products as lf_cc_dot_batch runs it
    int ta[LF_CC_MATMUL_MAX_INNER * 4], tb[LF_CC_MATMUL_MAX_INNER * 4];
    std::vector<MatmulTile> tiles;
    matmul_tiles(tiles, m, n, matmul_group(p));
    for (const MatmulTile &tl : tiles) {
        for (int t = 0; t < k; ++t) {
            for (int i = 0; i < tl.R; ++i) ta[t * tl.R + i] = (int)ia[(int64_t)(tl.i0 + i) * k + t];
            for (int j = 0; j < tl.C; ++j) tb[t * tl.C + j] = (int)ib[(int64_t)t * n + tl.j0 + j];
        }
        if (int e = lf_matmul_tensor(tl.R, tl.C, k, nu, store, ta, tb, T, p->d2, ell, logN, xpl, plan_mod(p), (hipStream_t)stream)) return e;
        int64_t *o0[4], *o1[4];
        for (int i = 0; i < tl.R; ++i)
            for (int j = 0; j < tl.C; ++j) {
                const int64_t at = (int64_t)(tl.i0 + i) * n + tl.j0 + j;
                o0[i * tl.C + j] = out0[at], o1[i * tl.C + j] = out1[at];
            }
        if (int e = dot_tail(p, tl.R * tl.C, T, key, o0, o1, stream)) return e;
    }
    return 0;
}

/* ---- pc_dot: sum_i pt_i * ct_i (+ bias) for plaintexts encoded once, under ONE rescale (include/ckks_hip.h).  Plan-free, like
 * lf_weighted_sums: no key, no digits.  The product with a plaintext is linear in the ciphertext, so the products are summed
 * in the NTT domain and the inverse transform and the rescale run once, on the sum. ---- */
int64_t lf_pc_dot_ws_words(int k, int rows, int logN) {
    if (k < 1 || rows < 2 || rows > MAX_LIST_ROWS || logN < 13 || logN > KS_LOGN_MAX) return 0;
    return ((int64_t)(2 * (k < 4 ? k : 4) + 2) * rows) << logN;   // the chunk's transformed pairs + S
}

int lf_pc_dot(int k, const int64_t *const *in, const int64_t *const *pt, const int64_t *bias, int64_t *out0, int64_t *out1, int rows,
              int logN, const int64_t *psi_br, const double *psi_dp, const int64_t *ipsi_br, const double *ipsi_dp,
              const int64_t *q_host, const int64_t *Rs, const int64_t *Ninv, const int64_t *mont_one, const int64_t *zero_row,
              const int64_t *rescale_scales, int64_t round_at, int64_t *ws, int64_t ws_words, const int64_t *ql, const int64_t *qh,
              const int64_t *kl, const int64_t *kh, int device, void *stream) {
    const int64_t need = lf_pc_dot_ws_words(k, rows, logN);
    if (!need || !in || !pt || !out0 || !out1 || !psi_br || !psi_dp || !ipsi_br || !ipsi_dp || !q_host || !Rs || !Ninv || !mont_one ||
        !zero_row || !rescale_scales || !ql || !qh || !kl || !kh)
        return LF_ERR_ARG;
    if (!ws || ws_words < need || ((uintptr_t)ws & 15)) return LF_ERR_ARG;
    for (int64_t i = 0; i < (int64_t)2 * k; ++i)
        if (!in[i]) return LF_ERR_ARG;
    for (int i = 0; i < k; ++i)
        if (!pt[i]) return LF_ERR_ARG;
    const int64_t N = (int64_t)1 << logN, poly = (int64_t)rows * N;
    const int xpl = lf_stack_planes(logN, rows, q_host);
    const int relaxed_plain = LF_NTT_RELAXED | LF_NTT_PLAIN | (xpl ? LF_NTT_PLANES : 0);
    if (int e = lf_set_device(device)) return e;
    int64_t *x = ws, *S = ws + (int64_t)2 * (k < 4 ? k : 4) * poly;
    const int64_t *zeros[8];
    for (int i = 0; i < 8; ++i) zeros[i] = zero_row;
    for (int i0 = 0; i0 < k;) {
        const int left = k - i0, g = left >= 4 ? 4 : left >= 2 ? 2 : 1;
        // 1. c0, c1 of the chunk's ciphertexts, all rows of their level, through the forward transform that reads its operands
        //    where they lie (the form lf_cc_dot fills its operand stack with: the only column pass that writes planes): its
        //    rescale step is handed the identity — a dropped row of zeros, the scale R (REDC(w R) = w), a threshold out of reach
        if (int e = lf_rescale_ntt(in + 2 * i0, zeros, 2 * g, x, rows, logN, mont_one, INT64_MAX, psi_br, psi_dp, q_host, Rs, relaxed_plain,
                                   nullptr, ql, qh, kl, kh, device, stream))
            return e;
        // 2. their products with the plaintexts into the one pair S
        if (int e = lf_pc_dot_products(g, x, pt + i0, S, rows, logN, xpl, i0 == 0, {ql, qh, kl, kh, q_host}, (hipStream_t)stream)) return e;
        i0 += g;
    }
    // 3. S -> canonical coefficients (intt_exit_reduce's words)
    if (int e = lf_intt(S, 2, rows, logN, ipsi_br, ipsi_dp, q_host, Ninv, 2, LF_NTT_RELAXED | LF_NTT_PLAIN, nullptr, ql, qh, kl, kh, device,
                        stream))
        return e;
    // 4. one rescale of the pair (the dropped limb is the first row), 5. the bias on component 0
    const int64_t *ins[2] = {S + N, S + poly + N}, *row0[2] = {S, S + poly};
    int64_t *outs[2] = {out0, out1};
    if (int e = lf_rescale_batch(ins, row0, outs, 2, rows - 1, N, rescale_scales, round_at, ql + 1, qh + 1, kl + 1, kh + 1, device, stream))
        return e;
    if (!bias) return 0;
    return lf_pc_bias(out0, bias, Rs + 1, rows - 1, logN, {ql + 1, qh + 1, kl + 1, kh + 1, q_host + 1}, (hipStream_t)stream);
}

/* ---- pc_matmul: k_out sums of plaintext-ciphertext products over the SAME k_in ciphertexts (include/ckks_hip.h): lf_pc_dot's
 * launches with the forward transforms shared by all outputs and every transformed word read once per group of 4 outputs. ---- */
int64_t lf_pc_matmul_ws_words(int k_in, int k_out, int rows, int logN) {
    if (k_in < 1 || k_out < 1 || k_out > LF_PC_MATMUL_MAX_OUTPUTS || rows < 2 || rows > MAX_LIST_ROWS || logN < 13 || logN > KS_LOGN_MAX)
        return 0;
    const int64_t ci = k_in < LF_PC_MATMUL_CI ? k_in : LF_PC_MATMUL_CI;
    return ((2 * ci + 2 * (int64_t)k_out) * rows) << logN;   // the chunk's transformed pairs + the k_out pairs of S
}

int64_t lf_pc_matmul_batch_ws_words(int nt, int k_in, int k_out, int rows, int logN) {
    if (nt < 1 || nt > LF_PC_MATMUL_BATCH_MAX_TOKENS) return 0;
    return nt * lf_pc_matmul_ws_words(k_in, k_out, rows, logN);
}

// lf_pc_matmul (nt = 1) and lf_pc_matmul_batch: `in` [token][input][component], out0 / out1 [token][output]; `need`: the words
// of the workspace the entry asks for (0: a refused shape).  x = [nt][ci][2][rows][N] with ci = min(k_in, LF_PC_MATMUL_CI) slots
// per token, S = [nt][k_out][2][rows][N] behind it.  planes: every non-NULL pt a compact plaintext (lf_plain_planes) — the products
// read it through pc_planes_matmul_kernel; everything else is the same.
static int pc_matmul_tokens(bool planes, int nt, int64_t need, int k_in, int k_out, const int64_t *const *in, const int64_t *const *pt,
                            const int64_t *const *bias, int64_t *const *out0, int64_t *const *out1, int rows, int logN,
                            const int64_t *psi_br, const double *psi_dp, const int64_t *ipsi_br, const double *ipsi_dp,
                            const int64_t *q_host, const int64_t *Rs, const int64_t *Ninv, const int64_t *mont_one,
                            const int64_t *zero_row, const int64_t *rescale_scales, int64_t round_at, int64_t *ws, int64_t ws_words,
                            const int64_t *ql, const int64_t *qh, const int64_t *kl, const int64_t *kh, int device, void *stream) {
    if (!need || !in || !pt || !out0 || !out1 || !psi_br || !psi_dp || !ipsi_br || !ipsi_dp || !q_host || !Rs || !Ninv || !mont_one ||
        !zero_row || !rescale_scales || !ql || !qh || !kl || !kh)
        return LF_ERR_ARG;
    if (!ws || ws_words < need || ((uintptr_t)ws & 15)) return LF_ERR_ARG;
    for (int64_t i = 0; i < (int64_t)nt * 2 * k_in; ++i)
        if (!in[i]) return LF_ERR_ARG;
    // the inputs some output uses, in their order (a column of NULLs is not transformed); every output needs a term
    std::vector<int> used;
    for (int i = 0; i < k_in; ++i)
        for (int o = 0; o < k_out; ++o)
            if (pt[(int64_t)o * k_in + i]) {
                used.push_back(i);
                break;
            }
    for (int o = 0; o < k_out; ++o) {
        for (int t = 0; t < nt; ++t)
            if (!out0[(int64_t)t * k_out + o] || !out1[(int64_t)t * k_out + o]) return LF_ERR_ARG;
        bool any = false;
        for (int i = 0; i < k_in && !any; ++i) any = pt[(int64_t)o * k_in + i] != nullptr;
        if (!any) return LF_ERR_ARG;
    }
    const int64_t N = (int64_t)1 << logN, poly = (int64_t)rows * N;
    const int xpl = lf_stack_planes(logN, rows, q_host);
    const int relaxed_plain = LF_NTT_RELAXED | LF_NTT_PLAIN | (xpl ? LF_NTT_PLANES : 0);
    uint64_t small = 0;
    if (planes && !lf_plain_planes_mask(rows, q_host, &small)) return LF_ERR_ARG;
    if (int e = lf_set_device(device)) return e;
    const LfMod mod{ql, qh, kl, kh, q_host};
    const int64_t xtok = 2 * (int64_t)(k_in < LF_PC_MATMUL_CI ? k_in : LF_PC_MATMUL_CI) * poly, stok = 2 * (int64_t)k_out * poly;
    int64_t *x = ws, *S = ws + nt * xtok;
    const int64_t *zeros[8];
    for (int i = 0; i < 8; ++i) zeros[i] = zero_row;
    const int na = (int)used.size();
    for (int a0 = 0; a0 < na; a0 += LF_PC_MATMUL_CI) {
        const int n = na - a0 < LF_PC_MATMUL_CI ? na - a0 : LF_PC_MATMUL_CI;
        // 1. the chunk's forward transforms into consecutive slots, as lf_pc_dot runs them: 4, 2 or 1 ciphertexts per call
        for (int tk = 0; tk < nt; ++tk) {
            const int64_t *const *tin = in + (int64_t)tk * 2 * k_in;
            for (int t0 = 0; t0 < n;) {
                const int left = n - t0, g = left >= 4 ? 4 : left >= 2 ? 2 : 1;
                const int64_t *ins[8];
                for (int t = 0; t < g; ++t) ins[2 * t] = tin[2 * used[a0 + t0 + t]], ins[2 * t + 1] = tin[2 * used[a0 + t0 + t] + 1];
                if (int e = lf_rescale_ntt(ins, zeros, 2 * g, x + tk * xtok + (int64_t)t0 * 2 * poly, rows, logN, mont_one, INT64_MAX, psi_br,
                                           psi_dp, q_host, Rs, relaxed_plain, nullptr, ql, qh, kl, kh, device, stream))
                    return e;
                t0 += g;
            }
        }
        // 2. per group of 4, 2 or 1 outputs ONE launch over the chunk per tile of 2 tokens (an odd token left: a tile of 1, which
        //    is lf_pc_matmul's launch): the group's pairs of S
        for (int o0 = 0; o0 < k_out;) {
            const int go = lf_pc_matmul_batch_outputs(k_out - o0, nt);   // (one token: 4, 2 or 1 of the outputs left, as ever)
            const int64_t *tab[LF_PC_MATMUL_CI * 4];
            for (int i = 0; i < n; ++i)
                for (int g = 0; g < go; ++g) tab[4 * i + g] = pt[(int64_t)(o0 + g) * k_in + used[a0 + i]];
            for (int tk = 0; tk < nt;) {
                const int gt = lf_pc_matmul_batch_tile(go, nt - tk);
                int64_t *Sg = S + tk * stok + (int64_t)o0 * 2 * poly;
                if (int e = lf_pc_matmul_products(planes, go, gt, n, x + tk * xtok, xtok, tab, 4, Sg, stok, rows, logN, xpl, a0 == 0, small, mod,
                                                  (hipStream_t)stream))
                    return e;
                tk += gt;
            }
            o0 += go;
        }
    }
    // 3. the polynomials of S -> canonical coefficients: one inverse transform up to 128 polynomials (what lf_pc_matmul hands it
    //    at 64 outputs), one per token beyond
    const int per = 2 * k_out * nt <= 2 * LF_PC_MATMUL_MAX_OUTPUTS ? nt : 1;
    for (int tk = 0; tk < nt; tk += per)
        if (int e = lf_intt(S + tk * stok, 2 * k_out * per, rows, logN, ipsi_br, ipsi_dp, q_host, Ninv, 2, LF_NTT_RELAXED | LF_NTT_PLAIN,
                            nullptr, ql, qh, kl, kh, device, stream))
            return e;
    // 4. the rescales, four outputs (8 polynomials) per launch; 5. the bias on component 0 of the outputs that have one
    for (int tk = 0; tk < nt; ++tk) {
        int64_t *St = S + tk * stok;
        int64_t *const *o0s = out0 + (int64_t)tk * k_out, *const *o1s = out1 + (int64_t)tk * k_out;
        for (int o0 = 0; o0 < k_out; o0 += 4) {
            const int go = k_out - o0 < 4 ? k_out - o0 : 4;
            const int64_t *ins[8], *row0[8];
            int64_t *outs[8];
            for (int g = 0; g < go; ++g)
                for (int c = 0; c < 2; ++c) {
                    row0[2 * g + c] = St + (2 * (int64_t)(o0 + g) + c) * poly;
                    ins[2 * g + c] = row0[2 * g + c] + N;
                    outs[2 * g + c] = c ? o1s[o0 + g] : o0s[o0 + g];
                }
            if (int e = lf_rescale_batch(ins, row0, outs, 2 * go, rows - 1, N, rescale_scales, round_at, ql + 1, qh + 1, kl + 1, kh + 1,
                                         device, stream))
                return e;
        }
        if (!bias) continue;
        for (int o = 0; o < k_out; ++o)
            if (bias[o])
                if (int e = lf_pc_bias(o0s[o], bias[o], Rs + 1, rows - 1, logN, {ql + 1, qh + 1, kl + 1, kh + 1, q_host + 1}, (hipStream_t)stream))
                    return e;
    }
    return 0;
}

int lf_pc_matmul(int k_in, int k_out, const int64_t *const *in, const int64_t *const *pt, const int64_t *const *bias,
                 int64_t *const *out0, int64_t *const *out1, int rows, int logN, const int64_t *psi_br, const double *psi_dp,
                 const int64_t *ipsi_br, const double *ipsi_dp, const int64_t *q_host, const int64_t *Rs, const int64_t *Ninv,
                 const int64_t *mont_one, const int64_t *zero_row, const int64_t *rescale_scales, int64_t round_at, int64_t *ws,
                 int64_t ws_words, const int64_t *ql, const int64_t *qh, const int64_t *kl, const int64_t *kh, int device, void *stream) {
    return pc_matmul_tokens(false, 1, lf_pc_matmul_ws_words(k_in, k_out, rows, logN), k_in, k_out, in, pt, bias, out0, out1, rows, logN, psi_br,
                            psi_dp, ipsi_br, ipsi_dp, q_host, Rs, Ninv, mont_one, zero_row, rescale_scales, round_at, ws, ws_words, ql, qh,
                            kl, kh, device, stream);
}

/* ---- pc_matmul_batch: lf_pc_matmul over nt token vectors that share the matrix (include/ckks_hip.h): every plaintext word is
 * read once per tile of 2 tokens instead of once per token. ---- */
int lf_pc_matmul_batch(int nt, int k_in, int k_out, const int64_t *const *in, const int64_t *const *pt, const int64_t *const *bias,
                       int64_t *const *out0, int64_t *const *out1, int rows, int logN, const int64_t *psi_br, const double *psi_dp,
                       const int64_t *ipsi_br, const double *ipsi_dp, const int64_t *q_host, const int64_t *Rs, const int64_t *Ninv,
                       const int64_t *mont_one, const int64_t *zero_row, const int64_t *rescale_scales, int64_t round_at, int64_t *ws,
                       int64_t ws_words, const int64_t *ql, const int64_t *qh, const int64_t *kl, const int64_t *kh, int device,
                       void *stream) {
    if (nt < 1 || nt > LF_PC_MATMUL_BATCH_MAX_TOKENS) return LF_ERR_ARG;
    return pc_matmul_tokens(false, nt, lf_pc_matmul_batch_ws_words(nt, k_in, k_out, rows, logN), k_in, k_out, in, pt, bias, out0, out1, rows,
                            logN, psi_br, psi_dp, ipsi_br, ipsi_dp, q_host, Rs, Ninv, mont_one, zero_row, rescale_scales, round_at, ws,
                            ws_words, ql, qh, kl, kh, device, stream);
}

/* ---- pc_matmul_batch over compact plaintexts (include/ckks_hip.h: lf_plain_planes): lf_pc_matmul_batch with the plaintext stream of
 * the product launches at 6 bytes per word on fp64-class rows and no REDC per word read. ---- */
int64_t lf_pc_matmul_batch_planes_ws_words(int nt, int k_in, int k_out, int rows, int logN) {
    if (rows > LF_PLAIN_PLANES_MAX_ROWS) return 0;
    return lf_pc_matmul_batch_ws_words(nt, k_in, k_out, rows, logN);
}

int lf_pc_matmul_batch_planes(int nt, int k_in, int k_out, const int64_t *const *in, const int64_t *const *pt, const int64_t *const *bias,
                              int64_t *const *out0, int64_t *const *out1, int rows, int logN, const int64_t *psi_br, const double *psi_dp,
                              const int64_t *ipsi_br, const double *ipsi_dp, const int64_t *q_host, const int64_t *Rs, const int64_t *Ninv,
                              const int64_t *mont_one, const int64_t *zero_row, const int64_t *rescale_scales, int64_t round_at, int64_t *ws,
                              int64_t ws_words, const int64_t *ql, const int64_t *qh, const int64_t *kl, const int64_t *kh, int device,
                              void *stream) {
    if (nt < 1 || nt > LF_PC_MATMUL_BATCH_MAX_TOKENS) return LF_ERR_ARG;
    return pc_matmul_tokens(true, nt, lf_pc_matmul_batch_planes_ws_words(nt, k_in, k_out, rows, logN), k_in, k_out, in, pt, bias, out0, out1,
                            rows, logN, psi_br, psi_dp, ipsi_br, ipsi_dp, q_host, Rs, Ninv, mont_one, zero_row, rescale_scales, round_at, ws,
                            ws_words, ql, qh, kl, kh, device, stream);
}

int lf_switch_key(const lf_ks_plan *p, const int64_t *c0, const int64_t *c1, int64_t gal_pinv, int gal_canonical,
                  const int64_t *ksk, int64_t part_stride, int64_t comp_stride, int64_t row_off, int key_format, int64_t *out0,
                  int64_t *out1, void *stream) {
    if (!plan_ok(p) || !c1 || !ksk || !out0 || !out1) return LF_ERR_ARG;
    const int ell = p->ell, rows = p->ell + p->K, logN = p->logN, dev = p->device;
    const int64_t N = (int64_t)1 << logN;
    const int64_t *g2q = (gal_pinv && gal_canonical) ? p->_2q : nullptr;
    if (int e = lf_ks_digits_galois(c1, p->state, p->dig_nparts, p->dig_desc, p->dig_tab, N, gal_pinv, g2q, p->ql, p->qh, p->kl, p->kh,
                                    dev, stream))
        return e;
    if (int e = lf_ks_core(p->state, p->nparts, rows, logN, p->ext_desc, p->E, p->Ed, ksk, part_stride, comp_stride, row_off, key_format, p->ext,
                           p->sum, p->psi, p->psi_dp, p->ipsi, p->ipsi_dp, p->Ninv, p->q_host, p->ql, p->qh, p->kl, p->kh, dev, stream))
        return e;
    return moddown_pairs(p, p->sum, 1, &out0, &out1, &c0, gal_pinv, g2q, stream);
}

/* ---- hoisted rotations: ONE ciphertext under nr keys, the digits of c1 extended and transformed once (include/ckks_hip.h) ---- */
// groups of up to 4 keys share one inner-product launch; their 2 x group sums sit in the plan's sum pairs
static int hoist_group_max(const lf_ks_plan *p) { return p->max_nct >= 4 ? 4 : p->max_nct; }

// where the sums of a group pass through their tiled inverse pass: the plan's ext slots behind the first (nct > 1 plans), else `ws`
static int64_t hoist_need(const lf_ks_plan *p) { return ((int64_t)2 * hoist_group_max(p) * (p->ell + p->K)) << p->logN; }
static int64_t hoist_spare(const lf_ks_plan *p) { return ((int64_t)(p->max_nct - 1) * p->nparts * (p->ell + p->K)) << p->logN; }

int64_t lf_rotate_hoisted_ws_words(const lf_ks_plan *p) {
    if (!plan_ok(p) || p->max_nct < 1) return 0;
    return hoist_spare(p) >= hoist_need(p) ? 0 : hoist_need(p);
}

int lf_rotate_hoisted(const lf_ks_plan *p, const int64_t *c0, const int64_t *c1, int nr, const int64_t *p_host, int gal_canonical,
                      const int64_t *const *ksk, int64_t part_stride, int64_t comp_stride, int64_t row_off, int key_format, int64_t *ws,
                      int64_t ws_words, int64_t *const *out0, int64_t *const *out1, void *stream) {
    if (!plan_ok(p) || nr < 1 || !c0 || !c1 || !out0 || !out1 || !lf_keys_ok({ksk, nr, part_stride, comp_stride, row_off, key_format}) ||
        !lf_exponents_ok(p_host, nr, p->logN))
        return LF_ERR_ARG;
    const int rows = p->ell + p->K, logN = p->logN, dev = p->device;
    const int64_t N = (int64_t)1 << logN, twoN = 2 * N;
    for (int i = 0; i < nr; ++i)
        if (!out0[i] || !out1[i]) return LF_ERR_ARG;
    const int64_t need = lf_rotate_hoisted_ws_words(p);
    if (need && (!ws || ws_words < need)) return LF_ERR_ARG;
    int64_t *scratch = need ? ws : p->ext + ((int64_t)p->nparts * rows << logN);
    const int64_t scratch_words = need ? ws_words : hoist_spare(p);
    const int64_t *g2q = gal_canonical ? p->_2q : nullptr;
    // 1. digits of c1, made canonical as rotate_single makes c1(X^p) (gal_pinv = 1: the identity map)
    if (int e = lf_ks_digits_galois(c1, p->state, p->dig_nparts, p->dig_desc, p->dig_tab, N, 1, g2q, p->ql, p->qh, p->kl, p->kh, dev,
                                    stream))
        return e;
    // 2. extension + forward NTT of every digit, once, into the first ext slot
    if (int e = lf_ks_fwd(p->state, p->nparts, rows, logN, p->ext_desc, p->E, p->Ed, p->ext, p->psi, p->psi_dp, p->q_host, p->ql, p->qh,
                          p->kl, p->kh, dev, stream))
        return e;
    // 3. per group of 4, 2 or 1 keys: gathered inner product + inverse NTT, then one mod-down per rotation with c0(X^p_i)
    for (int i0 = 0; i0 < nr;) {
        const int left = nr - i0, gmax = hoist_group_max(p);
        const int g = left >= 4 && gmax >= 4 ? 4 : left >= 2 && gmax >= 2 ? 2 : 1;
        if (int e = lf_ks_tail_hoisted(p_host + i0, p->nparts, rows, logN, {ksk + i0, g, part_stride, comp_stride, row_off, key_format}, p->ext,
                                       p->sum, scratch, scratch_words, plan_inv(p), plan_mod(p), (hipStream_t)stream))
            return e;
        for (int t = 0; t < g; ++t) {
            uint64_t x = (uint64_t)p_host[i0 + t], inv = x;   // p^-1 mod 2^64 by Newton's iteration (p odd), then mod 2N
            for (int k = 0; k < 6; ++k) inv *= 2 - x * inv;
            const int64_t pinv = (int64_t)(inv & (uint64_t)(twoN - 1));
            if (int e = moddown_pairs(p, p->sum + (int64_t)(2 * t) * rows * N, 1, out0 + i0 + t, out1 + i0 + t, &c0, pinv, g2q, stream)) return e;
        }
        i0 += g;
    }
    return 0;
}

/* ---- linear transform: sum_i diag_i * rot(ct, step_i), multiplied and summed in the NTT domain over Q P, ONE inverse NTT,
 * mod-down and rescale for the whole sum (include/ckks_hip.h) ---- */
// P NTT(c0), P NTT(c1) and the mod-down's [2][ell][N] result: the plan's operand stack x4 (free during this op), else `ws`
int64_t lf_linear_transform_ws_words(const lf_ks_plan *p) {
    if (!plan_ok(p) || p->x4) return 0;
    return ((int64_t)4 * p->ell) << p->logN;
}

int lf_linear_transform(const lf_ks_plan *p, const int64_t *c0, const int64_t *c1, int nr, const int64_t *p_host,
                        const int64_t *const *ksk, int64_t part_stride, int64_t comp_stride, int64_t row_off, int key_format,
                        const int64_t *pt, int64_t pt_stride, const int64_t *pt0, const int64_t *rescale_scales, int64_t round_at,
                        int64_t *ws, int64_t ws_words, int64_t *out0, int64_t *out1, void *stream) {
    const LfKeys key{ksk, nr, part_stride, comp_stride, row_off, key_format};
    if (!plan_ok(p) || !p->PR || p->ell < 2 || (nr == 0 && !pt0) || !c0 || !c1 || !rescale_scales || !out0 || !out1 || !lf_keys_ok(key) ||
        !lf_exponents_ok(p_host, nr, p->logN))
        return LF_ERR_ARG;
    const int ell = p->ell, rows = p->ell + p->K, logN = p->logN, dev = p->device;
    const int64_t N = (int64_t)1 << logN, poly = (int64_t)ell * N;
    if (nr && (!pt || pt_stride < (int64_t)rows * N)) return LF_ERR_ARG;
    const int64_t need = lf_linear_transform_ws_words(p);
    if (need && (!ws || ws_words < need || ((uintptr_t)ws & 15))) return LF_ERR_ARG;   // (ks_inner_lt_kernel: 16-byte column pairs of c^)
    int64_t *chat = need ? ws : p->x4, *md = chat + 2 * poly;
    // 1. P NTT(c0) (and P NTT(c1) for the step-0 term) on the ordinary rows
    const int64_t *srcs[2] = {c0, c1};
    if (int e = p_ntt(p, srcs, pt0 ? 2 : 1, chat, poly, stream)) return e;
    // 2. digits of c1 (canonical, no permutation), their extension + forward NTT: once, as lf_rotate_hoisted
    if (nr) {
        if (int e = lf_ks_digits_galois(c1, p->state, p->dig_nparts, p->dig_desc, p->dig_tab, N, 1, p->_2q, p->ql, p->qh, p->kl, p->kh, dev,
                                        stream))
            return e;
        if (int e = lf_ks_fwd(p->state, p->nparts, rows, logN, p->ext_desc, p->E, p->Ed, p->ext, p->psi, p->psi_dp, p->q_host, p->ql, p->qh,
                              p->kl, p->kh, dev, stream))
            return e;
    }
    // 3. the groups' launches into the one pair of sums, its inverse NTT (planes through the spent digits, two slots or more)
    const int64_t spare = p->nparts >= 2 ? ((int64_t)p->nparts * rows) << logN : 0;
    if (int e = lf_ks_tail_lt(p_host, p->nparts, rows, ell, logN, key, pt, pt_stride, pt0, chat, p->ext, p->sum, spare ? p->ext : nullptr, spare,
                              plan_inv(p), plan_mod(p), (hipStream_t)stream))
        return e;
    // 4. one mod-down, one rescale into the caller's [ell - 1][N] pair
    return moddown_rescale_pairs(p, p->sum, 1, md, nullptr, 0, &out0, &out1, rescale_scales, round_at, stream);
}

/* ---- linear transform of many ciphertexts under the same diagonals and keys (include/ckks_hip.h): groups of 4, 2 or 1; a group
 * of g shares every launch, and its inner product reads each key and diagonal word once for the g ciphertexts ---- */
static int lt_batch_group(const lf_ks_plan *p, int left) {
    return left >= 4 && p->max_nct >= 4 ? 4 : left >= 2 && p->max_nct >= 2 ? 2 : 1;
}

// per ciphertext of the largest group P NTT(c0), P NTT(c1) and the mod-down's [2][ell][N] result: the plan's operand stacks x4
// (free during this op), else `ws`
int64_t lf_linear_transform_batch_ws_words(const lf_ks_plan *p, int nct) {
    if (!plan_ok(p) || nct < 1 || nct > LF_LT_BATCH_MAX_CTS || p->x4) return 0;
    return ((int64_t)4 * lt_batch_group(p, nct) * p->ell) << p->logN;
}

int lf_linear_transform_batch(const lf_ks_plan *p, int nct, const int64_t *const *c0, const int64_t *const *c1, int nr,
                              const int64_t *p_host, const int64_t *const *ksk, int64_t part_stride, int64_t comp_stride,
                              int64_t row_off, int key_format, const int64_t *pt, int64_t pt_stride, const int64_t *pt0,
                              const int64_t *rescale_scales, int64_t round_at, int64_t *ws, int64_t ws_words, int64_t *const *out0,
                              int64_t *const *out1, void *stream) {
    const LfKeys key{ksk, nr, part_stride, comp_stride, row_off, key_format};
    if (!plan_ok(p) || !p->PR || p->ell < 2 || nct < 1 || nct > LF_LT_BATCH_MAX_CTS || (nr == 0 && !pt0) || !c0 || !c1 || !rescale_scales ||
        !out0 || !out1 || !lf_keys_ok(key) || !lf_exponents_ok(p_host, nr, p->logN))
        return LF_ERR_ARG;
    const int ell = p->ell, rows = p->ell + p->K, logN = p->logN, dev = p->device;
    const int64_t N = (int64_t)1 << logN, poly = (int64_t)ell * N;
    if (nr && (!pt || pt_stride < (int64_t)rows * N)) return LF_ERR_ARG;
    for (int t = 0; t < nct; ++t)
        if (!c0[t] || !c1[t] || !out0[t] || !out1[t]) return LF_ERR_ARG;
    const int64_t need = lf_linear_transform_batch_ws_words(p, nct);
    if (need && (!ws || ws_words < need || ((uintptr_t)ws & 15))) return LF_ERR_ARG;
    int64_t *base = need ? ws : p->x4;
    const int nc = pt0 ? 2 : 1;
    for (int t0 = 0; t0 < nct;) {
        const int g = lt_batch_group(p, nct - t0);
        if (g == 1) {   // a straggler: the flat op, whose scratch is the first slot of this one's
            if (int e = lf_linear_transform(p, c0[t0], c1[t0], nr, p_host, ksk, part_stride, comp_stride, row_off, key_format, pt, pt_stride, pt0,
                                            rescale_scales, round_at, ws, ws_words, out0[t0], out1[t0], stream))
                return e;
            t0 += 1;
            continue;
        }
        // 1. c^_t = P NTT(c0_t) (and P NTT(c1_t) for the step-0 term) on the ordinary rows, as lf_linear_transform forms them:
        //    chat [g][nc][ell][N], one canonical copy and one forward transform for the group
        int64_t *chat = base, *md = base + 2 * g * poly;
        {
            const int64_t *srcs[8];
            for (int t = 0; t < g; ++t)
                for (int c = 0; c < nc; ++c) srcs[t * nc + c] = c ? c1[t0 + t] : c0[t0 + t];
            if (int e = p_ntt(p, srcs, g * nc, chat, poly, stream)) return e;
        }
        // 2. the digits of the g c1 (canonical, no permutation), ONE extension + forward NTT of all of them
        if (nr) {
            const int64_t *srcs[4];
            int64_t *states[4];
            for (int t = 0; t < g; ++t) srcs[t] = c1[t0 + t], states[t] = p->state + t * poly;
            if (int e = lf_ks_digits_batch(srcs, states, g, p->dig_nparts, p->dig_desc, p->dig_tab, N, 1, p->_2q, p->ql, p->qh, p->kl, p->kh, dev,
                                           stream))
                return e;
            if (int e = lf_ks_fwd_batch(p->state, poly, g, p->nparts, rows, logN, p->ext_desc, p->E, p->Ed, p->ext, plan_fwd(p), plan_mod(p),
                                        (hipStream_t)stream))
                return e;
        }
        // 3. the launches into the g pairs of sums, ONE inverse NTT of the 2 g polynomials (planes through the spent digits)
        const int64_t spare = p->nparts >= 2 ? ((int64_t)g * p->nparts * rows) << logN : 0;
        if (int e = lf_ks_tail_ltb(g, p_host, p->nparts, rows, ell, logN, key, pt, pt_stride, pt0, chat, nc * poly, p->ext, p->sum,
                                   spare ? p->ext : nullptr, spare, plan_inv(p), plan_mod(p), (hipStream_t)stream))
            return e;
        // 4. one mod-down and one rescale of the 2 g polynomials into the callers' [ell - 1][N] pairs
        if (int e = moddown_rescale_pairs(p, p->sum, g, md, nullptr, 0, out0 + t0, out1 + t0, rescale_scales, round_at, stream)) return e;
        t0 += g;
    }
    return 0;
}

/* ---- rotation sum: sum_i rot(ct, step_i) [+ ct], summed in the NTT domain over Q P, ONE inverse NTT and mod-down for the
 * whole sum, no rescale: the result is at the ciphertext's own level (include/ckks_hip.h) ---- */
// P NTT(c0), P NTT(c1): the plan's operand stack x4 (free during this op), else `ws`
int64_t lf_rotate_sum_ws_words(const lf_ks_plan *p) {
    if (!plan_ok(p) || p->x4) return 0;
    return ((int64_t)2 * p->ell) << p->logN;
}

int lf_rotate_sum(const lf_ks_plan *p, const int64_t *c0, const int64_t *c1, int nr, const int64_t *p_host,
                  const int64_t *const *ksk, int64_t part_stride, int64_t comp_stride, int64_t row_off, int key_format,
                  int with_self, int64_t *ws, int64_t ws_words, int64_t *out0, int64_t *out1, void *stream) {
    const LfKeys key{ksk, nr, part_stride, comp_stride, row_off, key_format};
    if (!plan_ok(p) || !p->PR || (nr == 0 && !with_self) || !c0 || !c1 || !out0 || !out1 || !lf_keys_ok(key) ||
        !lf_exponents_ok(p_host, nr, p->logN))
        return LF_ERR_ARG;
    const int ell = p->ell, rows = p->ell + p->K, logN = p->logN, dev = p->device;
    const int64_t N = (int64_t)1 << logN, poly = (int64_t)ell * N;
    const int64_t need = lf_rotate_sum_ws_words(p);
    if (need && (!ws || ws_words < need || ((uintptr_t)ws & 15))) return LF_ERR_ARG;   // (ks_inner_rsum_kernel: 16-byte column pairs of c^)
    int64_t *chat = need ? ws : p->x4;
    // 1. P NTT(c0) (and P NTT(c1) for the self term) on the ordinary rows, as lf_linear_transform forms them
    const int64_t *srcs[2] = {c0, c1};
    if (int e = p_ntt(p, srcs, with_self ? 2 : 1, chat, poly, stream)) return e;
    // 2. digits of c1 (canonical, no permutation), their extension + forward NTT: once, as lf_rotate_hoisted
    if (nr) {
        if (int e = lf_ks_digits_galois(c1, p->state, p->dig_nparts, p->dig_desc, p->dig_tab, N, 1, p->_2q, p->ql, p->qh, p->kl, p->kh, dev,
                                        stream))
            return e;
        if (int e = lf_ks_fwd(p->state, p->nparts, rows, logN, p->ext_desc, p->E, p->Ed, p->ext, p->psi, p->psi_dp, p->q_host, p->ql, p->qh,
                              p->kl, p->kh, dev, stream))
            return e;
    }
    // 3. the groups' launches into the one pair of sums, its inverse NTT (planes through the spent digits, two slots or more)
    const int64_t spare = p->nparts >= 2 ? ((int64_t)p->nparts * rows) << logN : 0;
    if (int e = lf_ks_tail_rsum(p_host, p->nparts, rows, ell, logN, key, with_self, chat, p->ext, p->sum, spare ? p->ext : nullptr, spare,
                                plan_inv(p), plan_mod(p), (hipStream_t)stream))
        return e;
    // 4. one mod-down, straight into the caller's [ell][N] pair: no rescale, the level stays
    return moddown_pairs(p, p->sum, 1, &out0, &out1, nullptr, 0, nullptr, stream);
}

/* ---- rotation sum of many ciphertexts under the same keys (include/ckks_hip.h): groups of 4, 2 or 1 as lt_batch_group takes
 * them; a group of g shares every launch, and its inner product reads each key word once for the g ciphertexts ---- */
// per ciphertext of the largest group P NTT(c0), P NTT(c1): the plan's operand stacks x4 (free during this op), else `ws`
int64_t lf_rotate_sum_batch_ws_words(const lf_ks_plan *p, int nct) {
    if (!plan_ok(p) || nct < 1 || nct > LF_LT_BATCH_MAX_CTS || p->x4) return 0;
    return ((int64_t)2 * lt_batch_group(p, nct) * p->ell) << p->logN;
}

int lf_rotate_sum_batch(const lf_ks_plan *p, int nct, const int64_t *const *c0, const int64_t *const *c1, int nr,
                        const int64_t *p_host, const int64_t *const *ksk, int64_t part_stride, int64_t comp_stride, int64_t row_off,
                        int key_format, int with_self, int64_t *ws, int64_t ws_words, int64_t *const *out0, int64_t *const *out1,
                        void *stream) {
    const LfKeys key{ksk, nr, part_stride, comp_stride, row_off, key_format};
    if (!plan_ok(p) || !p->PR || nct < 1 || nct > LF_LT_BATCH_MAX_CTS || (nr == 0 && !with_self) || !c0 || !c1 || !out0 || !out1 ||
        !lf_keys_ok(key) || !lf_exponents_ok(p_host, nr, p->logN))
        return LF_ERR_ARG;
    const int ell = p->ell, rows = p->ell + p->K, logN = p->logN, dev = p->device;
    const int64_t N = (int64_t)1 << logN, poly = (int64_t)ell * N;
    for (int t = 0; t < nct; ++t)
        if (!c0[t] || !c1[t] || !out0[t] || !out1[t]) return LF_ERR_ARG;
    const int64_t need = lf_rotate_sum_batch_ws_words(p, nct);
    if (need && (!ws || ws_words < need || ((uintptr_t)ws & 15))) return LF_ERR_ARG;
    int64_t *chat = need ? ws : p->x4;
    const int nc = with_self ? 2 : 1;
    for (int t0 = 0; t0 < nct;) {
        const int g = lt_batch_group(p, nct - t0);
        if (g == 1) {   // a straggler: the op itself, whose scratch is the first slot of this one's
            if (int e = lf_rotate_sum(p, c0[t0], c1[t0], nr, p_host, ksk, part_stride, comp_stride, row_off, key_format, with_self, ws, ws_words,
                                      out0[t0], out1[t0], stream))
                return e;
            t0 += 1;
            continue;
        }
        // 1. c^_t = P NTT(c0_t) (and P NTT(c1_t) for the self term) on the ordinary rows, as lf_rotate_sum forms them:
        //    chat [g][nc][ell][N], one canonical copy and one forward transform for the group
        {
            const int64_t *srcs[8];
            for (int t = 0; t < g; ++t)
                for (int c = 0; c < nc; ++c) srcs[t * nc + c] = c ? c1[t0 + t] : c0[t0 + t];
            if (int e = p_ntt(p, srcs, g * nc, chat, poly, stream)) return e;
        }
        // 2. the digits of the g c1 (canonical, no permutation), ONE extension + forward NTT of all of them
        if (nr) {
            const int64_t *srcs[4];
            int64_t *states[4];
            for (int t = 0; t < g; ++t) srcs[t] = c1[t0 + t], states[t] = p->state + t * poly;
            if (int e = lf_ks_digits_batch(srcs, states, g, p->dig_nparts, p->dig_desc, p->dig_tab, N, 1, p->_2q, p->ql, p->qh, p->kl, p->kh, dev,
                                           stream))
                return e;
            if (int e = lf_ks_fwd_batch(p->state, poly, g, p->nparts, rows, logN, p->ext_desc, p->E, p->Ed, p->ext, plan_fwd(p), plan_mod(p),
                                        (hipStream_t)stream))
                return e;
        }
        // 3. the launches into the g pairs of sums, ONE inverse NTT of the 2 g polynomials (planes through the spent digits)
        const int64_t spare = p->nparts >= 2 ? ((int64_t)g * p->nparts * rows) << logN : 0;
        if (int e = lf_ks_tail_rsumb(g, p_host, p->nparts, rows, ell, logN, key, with_self, chat, nc * poly, p->ext, p->sum,
                                     spare ? p->ext : nullptr, spare, plan_inv(p), plan_mod(p), (hipStream_t)stream))
            return e;
        // 4. one mod-down of the 2 g polynomials, straight into the callers' [ell][N] pairs: no rescale, the level stays
        if (int e = moddown_pairs(p, p->sum, g, out0 + t0, out1 + t0, nullptr, 0, nullptr, stream)) return e;
        t0 += g;
    }
    return 0;
}

/* ---- linear transform, baby-step / giant-step: y = sum_g rot(sum_b pt_{g,b} * rot(x, b), g) (include/ckks_hip.h) ---- */
// LF_BSGS_MAX_BABY_KEYS (include/ckks_hip.h): slots 0 .. 63 are the bits of lt_diag_products_kernel's masks
#define LF_BSGS_S_PAIRS 4          // giant steps per launch of the diagonal products

int64_t lf_linear_transform_bsgs_ws_words(const lf_ks_plan *p, int nb) {
    if (!plan_ok(p) || nb < 0 || nb > LF_BSGS_MAX_BABY_KEYS) return 0;
    const int64_t N = (int64_t)1 << p->logN, pair = 2 * (int64_t)(p->ell + p->K) * N, poly = (int64_t)p->ell * N;
    // baby pairs (slot 0: the ciphertext), the S pairs of one launch, the accumulator A, w, the final mod-down's result, the
    // workspace of the one-polynomial mod-down (the plan's own is primed for pairs)
    return pair * (nb + 1 + LF_BSGS_S_PAIRS + 1) + poly + 2 * poly + lf_ks_moddown_ws_words(1, p->ell, p->K, N);
}

// n keyed steps of a baby-step / giant-step op: their keys (lf_keys_ok) and their exponents (lf_exponents_ok)
static bool keyed_steps_ok(const int64_t *const *ksk, const int64_t *p_host, int n, int64_t part_stride, int64_t comp_stride, int key_format,
                           int logN) {
    return lf_keys_ok({ksk, n, part_stride, comp_stride, 0, key_format}) && lf_exponents_ok(p_host, n, logN);
}

// steps 1 and 2 of the baby-step / giant-step ops and of the lf_lt_matmul family for one input of nt (1, 2 or 4) ciphertexts,
// c[t * c_tstride + comp] ciphertext t's polynomials, u + t * u_tstride its pairs: slot 0 = P NTT(c0), P NTT(c1) on the ordinary
// rows (the special rows of slot 0 are the caller's to zero), slot 1 + j the baby sum under the column's key j.
// nt = 1: the forward NTT straight into slot 0; the digits of c1 extended and transformed once, ONE launch over all the keys.
// nt > 1: canonical copies and ONE forward NTT of the 2 nt polynomials in `tmp` (2 nt [ell][N]), times P R, then into the slots;
//         the digits of the nt c1 (canonical, no permutation), ONE extension + forward NTT of all of them, per key of the column
//         ONE launch into slot 1 + j of every ciphertext: the key crosses HBM once for the group
static int column_pairs(const lf_ks_plan *p, int nt, const int64_t *const *c, int64_t c_tstride, const int64_t *p_host, const LfKeys &key,
                        int64_t *u, int64_t u_tstride, int64_t *tmp, void *stream) {
    const int ell = p->ell, rows = p->ell + p->K, logN = p->logN, dev = p->device;
    const int64_t N = (int64_t)1 << logN, poly = (int64_t)ell * N, half = (int64_t)rows * N, pair = 2 * half;
    hipStream_t st = (hipStream_t)stream;
    if (nt == 1) {
        if (int e = p_ntt(p, c, 2, u, half, stream)) return e;
        if (!key.n) return 0;
        if (int e = lf_ks_digits_galois(c[1], p->state, p->dig_nparts, p->dig_desc, p->dig_tab, N, 1, p->_2q, p->ql, p->qh, p->kl, p->kh, dev,
                                        stream))
            return e;
        if (int e = lf_ks_fwd(p->state, p->nparts, rows, logN, p->ext_desc, p->E, p->Ed, p->ext, p->psi, p->psi_dp, p->q_host, p->ql, p->qh,
                              p->kl, p->kh, dev, stream))
            return e;
        return lf_ks_baby_sums(p_host, p->nparts, rows, ell, logN, key, u, p->ext, u + pair, plan_mod(p), st);
    }
    {
        const int64_t *srcs[2 * LF_LT_MATMUL_BATCH_MAX_TOKENS];
        for (int t = 0; t < nt; ++t)
            for (int k = 0; k < 2; ++k) srcs[2 * t + k] = c[t * c_tstride + k];
        if (int e = p_ntt(p, srcs, 2 * nt, tmp, poly, stream)) return e;
        for (int k = 0; k < 2 * nt; ++k)
            if (hipError_t e = hipMemcpyAsync(u + (k / 2) * u_tstride + (k & 1) * half, tmp + k * poly, (size_t)poly * 8,
                                              hipMemcpyDeviceToDevice, st))
                return (int)e;
    }
    if (!key.n) return 0;
    const int64_t *srcs[LF_LT_MATMUL_BATCH_MAX_TOKENS], *chat0[LF_LT_MATMUL_BATCH_MAX_TOKENS];
    int64_t *states[LF_LT_MATMUL_BATCH_MAX_TOKENS], *us[LF_LT_MATMUL_BATCH_MAX_TOKENS];
    for (int t = 0; t < nt; ++t) srcs[t] = c[t * c_tstride + 1], states[t] = p->state + t * poly, chat0[t] = u + t * u_tstride;
    if (int e = lf_ks_digits_batch(srcs, states, nt, p->dig_nparts, p->dig_desc, p->dig_tab, N, 1, p->_2q, p->ql, p->qh, p->kl, p->kh, dev,
                                   stream))
        return e;
    if (int e = lf_ks_fwd_batch(p->state, poly, nt, p->nparts, rows, logN, p->ext_desc, p->E, p->Ed, p->ext, plan_fwd(p), plan_mod(p), st))
        return e;
    for (int j = 0; j < key.n; ++j) {
        for (int t = 0; t < nt; ++t) us[t] = u + t * u_tstride + (j + 1) * pair;
        if (int e = lf_ks_baby_sums_batch(nt, p_host[j], p->nparts, rows, ell, logN,
                                          {key.ksk + j, 1, key.part_stride, key.comp_stride, key.row_off, key.key_format}, p->ext, chat0, us,
                                          plan_mod(p), st))
            return e;
    }
    return 0;
}

// what lf_linear_transform_bsgs refuses in its keys, giant steps and diagonals (everything but the ciphertext, the outputs and the
// workspace): 0 or LF_ERR_ARG, nothing launched
static int bsgs_args_ok(const lf_ks_plan *p, int nb, const int64_t *bp_host, const int64_t *const *bksk, int ng, const int64_t *gp_host,
                        const int64_t *const *gksk, int64_t part_stride, int64_t comp_stride, int key_format, const int64_t *pt,
                        int64_t pt_stride, const int64_t *gcount, const int64_t *bidx, const int64_t *rescale_scales) {
    if (!plan_ok(p) || !p->PR || p->ell < 2 || nb < 0 || nb > LF_BSGS_MAX_BABY_KEYS || ng < 1 || !rescale_scales || !pt || !gp_host ||
        !gksk || !gcount || !bidx || (nb && (!bp_host || !bksk)) || (key_format != LF_KEY_RAW && key_format != LF_KEY_PLANES))
        return LF_ERR_ARG;
    const int64_t N = (int64_t)1 << p->logN;
    if (pt_stride < (int64_t)(p->ell + p->K) * N) return LF_ERR_ARG;
    if (!keyed_steps_ok(bksk, bp_host, nb, part_stride, comp_stride, key_format, p->logN)) return LF_ERR_ARG;
    int64_t ndiag = 0;
    for (int i = 0; i < ng; ++i) {
        // (giant step 0: first, so at most once)
        if (gp_host[i] == 0 ? i != 0 : !keyed_steps_ok(gksk + i, gp_host + i, 1, part_stride, comp_stride, key_format, p->logN)) return LF_ERR_ARG;
        if (gcount[i] < 1 || gcount[i] > nb + 1) return LF_ERR_ARG;
        for (int64_t k = 0; k < gcount[i]; ++k) {
            const int64_t slot = bidx[ndiag + k];
            if (slot < 0 || slot > nb || (k && slot <= bidx[ndiag + k - 1])) return LF_ERR_ARG;
        }
        ndiag += gcount[i];
    }
    return 0;
}

int lf_linear_transform_bsgs(const lf_ks_plan *p, const int64_t *c0, const int64_t *c1, int nb, const int64_t *bp_host,
                             const int64_t *const *bksk, int ng, const int64_t *gp_host, const int64_t *const *gksk,
                             int64_t part_stride, int64_t comp_stride, int64_t row_off, int key_format, const int64_t *pt,
                             int64_t pt_stride, const int64_t *gcount, const int64_t *bidx, const int64_t *rescale_scales,
                             int64_t round_at, int64_t *ws, int64_t ws_words, int64_t *out0, int64_t *out1, void *stream) {
    if (!c0 || !c1 || !out0 || !out1) return LF_ERR_ARG;
    if (int e = bsgs_args_ok(p, nb, bp_host, bksk, ng, gp_host, gksk, part_stride, comp_stride, key_format, pt, pt_stride, gcount, bidx,
                             rescale_scales))
        return e;
    const int ell = p->ell, rows = p->ell + p->K, logN = p->logN, dev = p->device;
    const int64_t N = (int64_t)1 << logN, poly = (int64_t)ell * N, pair = 2 * (int64_t)rows * N;
    const int64_t need = lf_linear_transform_bsgs_ws_words(p, nb);
    if (!ws || ws_words < need || ((uintptr_t)ws & 15)) return LF_ERR_ARG;   // (lt_diag_products_kernel: 16-byte column pairs of u, S, A)
    hipStream_t st = (hipStream_t)stream;
    int64_t *u = ws, *S = u + (nb + 1) * pair, *A = S + LF_BSGS_S_PAIRS * pair, *w = A + pair, *md = w + poly, *md1 = md + 2 * poly;
    const int64_t md1_words = lf_ks_moddown_ws_words(1, ell, p->K, N);
    if (int e = lf_set_device(dev)) return e;
    // 1., 2. slot 0 = P NTT(c0), P NTT(c1) on the ordinary rows (canonical copy, enter_ntt, times P R), zero on the special rows;
    // the baby steps: the digits of c1 extended and transformed once, one launch into the slots 1 .. nb
    {
        const int64_t *srcs[2] = {c0, c1};
        for (int c = 0; c < 2; ++c)
            if (hipError_t e = hipMemsetAsync(u + c * (int64_t)rows * N + poly, 0, (size_t)p->K * N * 8, st)) return (int)e;
        if (int e = column_pairs(p, 1, srcs, 0, bp_host, {bksk, nb, part_stride, comp_stride, row_off, key_format}, u, 0, nullptr, stream))
            return e;
    }
    // 3. giant steps, LF_BSGS_S_PAIRS per launch of the diagonal products; giant step 0 writes the accumulator itself
    if (gp_host[0] != 0)
        if (hipError_t e = hipMemsetAsync(A, 0, (size_t)pair * 8, st)) return (int)e;
    int64_t first = 0;   // first diagonal of the giant step in the pack
    for (int i0 = 0; i0 < ng;) {
        const int left = ng - i0, g = left >= 4 ? 4 : left >= 2 ? 2 : 1;
        const int64_t *pts[4];
        int64_t *outs[4];
        unsigned long long slots[4];
        for (int t = 0; t < g; ++t) {
            pts[t] = pt + first * pt_stride;
            slots[t] = 0;
            for (int64_t k = 0; k < gcount[i0 + t]; ++k) slots[t] |= 1ull << bidx[first + k];
            outs[t] = gp_host[i0 + t] == 0 ? A : S + t * pair;
            first += gcount[i0 + t];
        }
        if (int e = lf_lt_diag_products(g, u, nb + 1, pts, slots, pt_stride, outs, rows, logN, plan_mod(p), st)) return e;
        for (int t = 0; t < g; ++t) {
            if (gp_host[i0 + t] == 0) continue;
            int64_t *S0 = S + t * pair, *S1 = S0 + (int64_t)rows * N;
            // S^g_1 down to Q: inverse NTT, mod-down of the one polynomial, its digits (canonical), extended and transformed
            if (int e = lf_intt(S1, 1, rows, logN, p->ipsi, p->ipsi_dp, p->q_host, p->Ninv, 2, 0, p->_2q, p->ql, p->qh, p->kl, p->kh, dev, stream))
                return e;
            const int64_t *ss[1] = {S1};
            int64_t *ws1[1] = {w};
            if (int e = lf_ks_moddown_ws(ss, ws1, nullptr, 1, ell, p->K, N, md1, md1_words, p->PiR, p->PiP, p->Rs, 0, nullptr, p->ql, p->qh,
                                         p->kl, p->kh, dev, stream))
                return e;
            if (int e = lf_ks_digits_galois(w, p->state, p->dig_nparts, p->dig_desc, p->dig_tab, N, 1, p->_2q, p->ql, p->qh, p->kl, p->kh, dev,
                                            stream))
                return e;
            if (int e = lf_ks_fwd(p->state, p->nparts, rows, logN, p->ext_desc, p->E, p->Ed, p->ext, p->psi, p->psi_dp, p->q_host, p->ql,
                                  p->qh, p->kl, p->kh, dev, stream))
                return e;
            if (int e = lf_ks_giant_sums(gp_host[i0 + t], p->nparts, rows, logN, {gksk + i0 + t, 1, part_stride, comp_stride, row_off, key_format},
                                         p->ext, S0, A, plan_mod(p), st))
                return e;
        }
        i0 += g;
    }
    // 4. one exact inverse NTT of the accumulator (intt_exit_reduce), one mod-down, one rescale into the caller's [ell - 1][N] pair
    if (int e = lf_intt(A, 2, rows, logN, p->ipsi, p->ipsi_dp, p->q_host, p->Ninv, 2, 0, p->_2q, p->ql, p->qh, p->kl, p->kh, dev, stream))
        return e;
    return moddown_rescale_pairs(p, A, 1, md, nullptr, 0, &out0, &out1, rescale_scales, round_at, stream);
}

/* ---- the lf_lt_matmul family (include/ckks_hip.h): a matrix of linear transforms times a vector of ciphertexts,
 *     y_o = sum_g rot(sum_i sum_b pt_{o,i,g+b} * rot(x_i, b), g),
 * over nt token vectors and ng giant steps.  ONE body, lt_matmul_body, behind the four entries:
 *     lf_lt_matmul            nt = 1,          ng = 1 (the giant step 0: every step is its own baby step)
 *     lf_lt_matmul_batch      nt = 1, 2 or 4,  ng = 1
 *     lf_lt_matmul_bsgs       nt = 1,          ng giant steps
 *     lf_lt_matmul_bsgs_batch nt = 1, 2 or 4,  ng giant steps
 * Input-major: the baby sums of one input are formed once, for every output, in the slots of the BSGS path's baby pairs
 * (column_pairs); the inner sums S^{o,g} of the pairs (output, giant step) stay in Q P over ALL inputs — giant step 0's is the
 * accumulator A^o itself — so an output pays one key switch per keyed giant step and the members that share a giant step share the
 * stream of its key (bsgs_giant_step); every accumulator comes down once (matmul_tail).
 * nt selects the launches: nt = 1 takes the single-ciphertext kernels (the NTT straight into slot 0, one multi-key launch of the
 * baby sums, lf_lt_block_products over giant-step-0 and keyed targets alike); nt > 1 shares every launch among the tokens (each key
 * word read once for the group, each diagonal word once per pair of tokens: lf_lt_block_productsb, whose one token stride puts the
 * accumulators and the keyed sums in launches of their own), and the tokens of one output fill the giant step's group.
 * ng = 1 with the giant step 0 has no keyed sum: the giant phase does nothing, and the flat entries leave its scratch out. ---- */
#define LF_LT_MATMUL_GROUP 4       // outputs per launch of the block products and per inverse NTT / mod-down / rescale

// the tail of the lf_lt_matmul family: n sums [n][2][rows][N] at S in Q P, in groups of up to LF_LT_MATMUL_GROUP: one exact inverse
// NTT (intt_exit_reduce) of the group's 2 g polynomials, one mod-down in mdws, one rescale into the pairs out0[s], out1[s]
static int matmul_tail(const lf_ks_plan *p, int64_t *S, int n, int64_t *md, int64_t *mdws, int64_t mdws_words, int64_t *const *out0,
                       int64_t *const *out1, const int64_t *rescale_scales, int64_t round_at, void *stream) {
    const int rows = p->ell + p->K;
    const int64_t pair = (2 * (int64_t)rows) << p->logN;
    for (int s0 = 0; s0 < n; s0 += LF_LT_MATMUL_GROUP) {
        const int g = n - s0 < LF_LT_MATMUL_GROUP ? n - s0 : LF_LT_MATMUL_GROUP;
        int64_t *Sg = S + s0 * pair;
        if (int e = lf_intt(Sg, 2 * g, rows, p->logN, p->ipsi, p->ipsi_dp, p->q_host, p->Ninv, 2, 0, p->_2q, p->ql, p->qh, p->kl, p->kh,
                            p->device, stream))
            return e;
        if (int e = moddown_rescale_pairs(p, Sg, g, md, mdws, mdws_words, out0 + s0, out1 + s0, rescale_scales, round_at, stream)) return e;
    }
    return 0;
}

// polynomials the giant phase brings down at once: groups of 4, 2 or 1 outputs within the batch the plan is sized for
static int bsgs_giant_group(const lf_ks_plan *p) { return p->max_nct < 4 ? p->max_nct : 4; }

// the giant step of n (4, 2 or 1) pairs S^g under ONE key, added into their accumulators: per pair the inverse NTT of S^g_1 (the pair
// layout stays), then for the group ONE mod-down into w, ONE digit launch, ONE extension + forward pass and ONE launch of the key
// switch, with each pair's S^g_0 gathered on all rows.  w: n [ell][N] polynomials; mdws: the workspace of a mod-down of n
static int bsgs_giant_step(const lf_ks_plan *p, int n, int64_t *const *S, int64_t *const *accs, int64_t gp, const LfKeys &key, int64_t *w,
                           int64_t *mdws, int64_t mdws_words, void *stream) {
    const int ell = p->ell, rows = p->ell + p->K, logN = p->logN, dev = p->device;
    const int64_t N = (int64_t)1 << logN, poly = (int64_t)ell * N;
    hipStream_t st = (hipStream_t)stream;
    const int64_t *ss[4], *s0s[4], *srcs[4];
    int64_t *ws1[4], *states[4];
    for (int t = 0; t < n; ++t) {
        int64_t *S0 = S[t], *S1 = S0 + (int64_t)rows * N;
        if (int e = lf_intt(S1, 1, rows, logN, p->ipsi, p->ipsi_dp, p->q_host, p->Ninv, 2, 0, p->_2q, p->ql, p->qh, p->kl, p->kh, dev, stream))
            return e;
        ss[t] = S1, s0s[t] = S0, ws1[t] = w + t * poly, srcs[t] = ws1[t], states[t] = p->state + t * poly;
    }
    if (int e = lf_ks_moddown_ws(ss, ws1, nullptr, n, ell, p->K, N, mdws, mdws_words, p->PiR, p->PiP, p->Rs, 0, nullptr, p->ql, p->qh, p->kl,
                                 p->kh, dev, stream))
        return e;
    if (int e = lf_ks_digits_batch(srcs, states, n, p->dig_nparts, p->dig_desc, p->dig_tab, N, 1, p->_2q, p->ql, p->qh, p->kl, p->kh, dev,
                                   stream))
        return e;
    if (n == 1) {
        if (int e = lf_ks_fwd(p->state, p->nparts, rows, logN, p->ext_desc, p->E, p->Ed, p->ext, p->psi, p->psi_dp, p->q_host, p->ql, p->qh,
                              p->kl, p->kh, dev, stream))
            return e;
        return lf_ks_giant_sums(gp, p->nparts, rows, logN, key, p->ext, s0s[0], accs[0], plan_mod(p), st);
    }
    if (int e = lf_ks_fwd_batch(p->state, poly, n, p->nparts, rows, logN, p->ext_desc, p->E, p->Ed, p->ext, plan_fwd(p), plan_mod(p), st))
        return e;
    return lf_ks_giant_sums_batch(n, gp, p->nparts, rows, logN, key, p->ext, s0s, accs, plan_mod(p), st);
}

// what the family learns of its arguments while it checks them: the first key of every column, the inputs some output uses, the
// blocks' slot masks, the pairs (o, j) that have a diagonal, the index of every keyed inner sum (giant step after giant step), the
// longest used column and the number of keyed sums
struct BsgsShape {
    std::vector<int64_t> koff;
    std::vector<char> used, has;
    std::vector<unsigned long long> masks;
    std::vector<int> sidx;
    int nb_max = 0, keyed_sums = 0;
};

// the family's checks on everything but the workspace, for nt tokens (in: [token][input][component], those of a used input are
// checked for every token; out0 / out1: [token][output]).  gp_host is the caller's to check for NULL; gksk is read for keyed giant
// steps alone (the flat entries have none and pass NULL)
static int lt_matmul_bsgs_args(const lf_ks_plan *p, int nt, int k_in, int k_out, const int64_t *const *in, const int64_t *ncol,
                               const int64_t *bp_host, const int64_t *const *bksk, int ng, const int64_t *gp_host,
                               const int64_t *const *gksk, int64_t part_stride, int64_t comp_stride, int key_format,
                               const int64_t *const *pt, const int64_t *pt_stride, const int64_t *gcount, const int64_t *bidx,
                               const int64_t *rescale_scales, int64_t *const *out0, int64_t *const *out1, BsgsShape &sh) {
    if (!plan_ok(p) || !p->PR || p->ell < 2 || k_in < 1 || k_in > LF_LT_MATMUL_MAX_INPUTS || k_out < 1 || k_out > LF_LT_MATMUL_MAX_OUTPUTS ||
        ng < 1 || ng > LF_LT_MATMUL_BSGS_MAX_GIANTS || !in || !ncol || !pt || !pt_stride || !gcount || !bidx || !rescale_scales || !out0 || !out1 || (key_format != LF_KEY_RAW && key_format != LF_KEY_PLANES))
        return LF_ERR_ARG;
    const int rows = p->ell + p->K, logN = p->logN;
    const int64_t N = (int64_t)1 << logN;
    auto block = [&](int o, int i, int j) { return ((int64_t)o * k_in + i) * ng + j; };
    for (int j = 0; j < ng; ++j)   // (giant step 0: first, so at most once)
        if (gp_host[j] == 0 ? j != 0 : !keyed_steps_ok(gksk + j, gp_host + j, 1, part_stride, comp_stride, key_format, logN)) return LF_ERR_ARG;
    // the columns: keyed baby steps per input, the inputs some output uses, their keys
    sh.koff.assign(k_in + 1, 0);
    sh.used.assign(k_in, 0);
    sh.nb_max = 0;
    for (int i = 0; i < k_in; ++i) {
        if (ncol[i] < 0 || ncol[i] > LF_BSGS_MAX_BABY_KEYS) return LF_ERR_ARG;
        sh.koff[i + 1] = sh.koff[i] + ncol[i];
        for (int o = 0; o < k_out && !sh.used[i]; ++o)
            for (int j = 0; j < ng && !sh.used[i]; ++j) sh.used[i] = pt[block(o, i, j)] != nullptr;
        if (!sh.used[i]) continue;
        for (int t = 0; t < nt; ++t)
            if (!in[2 * ((int64_t)t * k_in + i)] || !in[2 * ((int64_t)t * k_in + i) + 1]) return LF_ERR_ARG;
        if (ncol[i] && (!bp_host || !bksk)) return LF_ERR_ARG;
        if (ncol[i] && !keyed_steps_ok(bksk + sh.koff[i], bp_host + sh.koff[i], (int)ncol[i], part_stride, comp_stride, key_format, logN))
            return LF_ERR_ARG;
        if (ncol[i] > sh.nb_max) sh.nb_max = (int)ncol[i];
    }
    // the diagonals: per (output, input, giant step) its slots inside the column's set, ascending
    sh.masks.assign((size_t)k_out * k_in * ng, 0);
    sh.has.assign((size_t)k_out * ng, 0);
    int64_t first = 0;
    for (int o = 0; o < k_out; ++o) {
        for (int t = 0; t < nt; ++t)
            if (!out0[(int64_t)t * k_out + o] || !out1[(int64_t)t * k_out + o]) return LF_ERR_ARG;
        bool any = false;
        for (int i = 0; i < k_in; ++i)
            for (int j = 0; j < ng; ++j) {
                const int64_t b = block(o, i, j);
                if (!pt[b]) {
                    if (gcount[b] != 0) return LF_ERR_ARG;
                    continue;
                }
                any = true, sh.has[(size_t)o * ng + j] = 1;
                if (gcount[b] < 1 || gcount[b] > ncol[i] + 1 || pt_stride[b] < (int64_t)rows * N) return LF_ERR_ARG;
                for (int64_t k = 0; k < gcount[b]; ++k) {
                    const int64_t slot = bidx[first + k];
                    if (slot < 0 || slot > ncol[i] || (k && slot <= bidx[first + k - 1])) return LF_ERR_ARG;
                    sh.masks[b] |= 1ull << slot;
                }
                first += gcount[b];
            }
        if (!any) return LF_ERR_ARG;
    }
    sh.sidx.assign((size_t)k_out * ng, -1);
    sh.keyed_sums = 0;
    for (int j = 0; j < ng; ++j) {
        if (gp_host[j] == 0) continue;
        bool any = false;
        for (int o = 0; o < k_out; ++o)
            if (sh.has[(size_t)o * ng + j]) sh.sidx[(size_t)o * ng + j] = sh.keyed_sums++, any = true;
        if (!any) return LF_ERR_ARG;   // a keyed giant step no output uses
    }
    return sh.keyed_sums > LF_LT_MATMUL_BSGS_MAX_SUMS ? LF_ERR_ARG : 0;
}

// the family's workspace, in words from its start (total = 0: an argument out of range): per token one input's pairs U [nt][nb_max
// + 1] (slot 0: the ciphertext; `member` words a token), the accumulators A [nt][k_out] (one run: a group of the tail may span two
// tokens), the keyed inner sums S [nt][keyed_sums], w of one giant group, the mod-down's results md of one group of accumulators,
// and the workspace of either mod-down (the plan's own is primed for pairs).  The flat entries (bsgs = false, keyed_sums = 0) have no
// giant phase: no w, and mdws sized for the tail alone
struct LtMatmulLayout {
    int64_t member, A, S, w, md, mdws, mdws_words, total;
};

static LtMatmulLayout lt_matmul_layout(const lf_ks_plan *p, int nt, int nb_max, int k_out, int keyed_sums, bool bsgs) {
    LtMatmulLayout L = {};
    if (!plan_ok(p) || nb_max < 0 || nb_max > LF_BSGS_MAX_BABY_KEYS || k_out < 1 || k_out > LF_LT_MATMUL_MAX_OUTPUTS || keyed_sums < 0 ||
        keyed_sums > LF_LT_MATMUL_BSGS_MAX_SUMS)
        return L;
    const int64_t N = (int64_t)1 << p->logN, pair = 2 * (int64_t)(p->ell + p->K) * N, poly = (int64_t)p->ell * N;
    const int na = nt * k_out, g4 = na < LF_LT_MATMUL_GROUP ? na : LF_LT_MATMUL_GROUP, gw = bsgs ? bsgs_giant_group(p) : 0;
    const int64_t md_w = bsgs ? lf_ks_moddown_ws_words(gw, p->ell, p->K, N) : 0, md_t = lf_ks_moddown_ws_words(2 * g4, p->ell, p->K, N);
    L.member = (nb_max + 1) * pair;
    L.A = nt * L.member;
    L.S = L.A + na * pair;
    L.w = L.S + (int64_t)nt * keyed_sums * pair;
    L.md = L.w + gw * poly;
    L.mdws = L.md + 2 * g4 * poly;
    L.mdws_words = md_w > md_t ? md_w : md_t;
    L.total = L.mdws + L.mdws_words;
    return L;
}

int64_t lf_lt_matmul_ws_words(const lf_ks_plan *p, int nb_max, int k_out) { return lt_matmul_layout(p, 1, nb_max, k_out, 0, false).total; }

int64_t lf_lt_matmul_batch_ws_words(const lf_ks_plan *p, int nb_max, int k_out, int nt) {
    if (!batch_ok(p, nt) || nt > LF_LT_MATMUL_BATCH_MAX_TOKENS) return 0;
    return lt_matmul_layout(p, nt, nb_max, k_out, 0, false).total;
}

int64_t lf_lt_matmul_bsgs_ws_words(const lf_ks_plan *p, int nb_max, int k_out, int keyed_sums) {
    return lt_matmul_layout(p, 1, nb_max, k_out, keyed_sums, true).total;
}

int64_t lf_lt_matmul_bsgs_batch_ws_words(const lf_ks_plan *p, int nb_max, int k_out, int keyed_sums, int nt) {
    if (!batch_ok(p, nt) || nt > LF_LT_MATMUL_BSGS_BATCH_MAX_TOKENS) return 0;
    return lt_matmul_layout(p, nt, nb_max, k_out, keyed_sums, true).total;
}

// the body of the family (the comment at its head): nt tokens, ng giant steps; bsgs: the layout of the BSGS entries
static int lt_matmul_body(const lf_ks_plan *p, bool bsgs, int nt, int k_in, int k_out, const int64_t *const *in, const int64_t *ncol,
                          const int64_t *bp_host, const int64_t *const *bksk, int ng, const int64_t *gp_host, const int64_t *const *gksk,
                          int64_t part_stride, int64_t comp_stride, int64_t row_off, int key_format, const int64_t *const *pt,
                          const int64_t *pt_stride, const int64_t *gcount, const int64_t *bidx, const int64_t *rescale_scales,
                          int64_t round_at, int64_t *ws, int64_t ws_words, int64_t *const *out0, int64_t *const *out1, void *stream) {
    BsgsShape sh;
    if (int e = lt_matmul_bsgs_args(p, nt, k_in, k_out, in, ncol, bp_host, bksk, ng, gp_host, gksk, part_stride, comp_stride, key_format, pt,
                                    pt_stride, gcount, bidx, rescale_scales, out0, out1, sh))
        return e;
    const int rows = p->ell + p->K, logN = p->logN;
    const int64_t N = (int64_t)1 << logN, poly = (int64_t)p->ell * N, half = (int64_t)rows * N, pair = 2 * half;
    const int keyed_sums = sh.keyed_sums;
    const LtMatmulLayout L = lt_matmul_layout(p, nt, sh.nb_max, k_out, keyed_sums, bsgs);
    if (!L.total || !ws || ws_words < L.total || ((uintptr_t)ws & 15)) return LF_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    int64_t *w = ws + L.w, *md = ws + L.md, *mdws = ws + L.mdws;
    auto block = [&](int o, int i, int j) { return ((int64_t)o * k_in + i) * ng + j; };
    auto U = [&](int t) { return ws + t * L.member; };
    auto acc = [&](int t, int o) { return ws + L.A + ((int64_t)t * k_out + o) * pair; };
    auto sum = [&](int t, int o, int j) { return ws + L.S + ((int64_t)t * keyed_sums + sh.sidx[(size_t)o * ng + j]) * pair; };
    // per (output, giant step) the target of its inner sum: the accumulator A^o itself for giant step 0, else its pair of S
    auto target = [&](int o, int j) { return gp_host[j] == 0 ? acc(0, o) : sum(0, o, j); };
    if (int e = lf_set_device(p->device)) return e;
    // slot 0 holds nothing on the special rows, for every input and token; an output without giant step 0 starts from zero accumulators
    for (int t = 0; t < nt; ++t)
        for (int c = 0; c < 2; ++c)
            if (hipError_t e = hipMemsetAsync(U(t) + c * half + poly, 0, (size_t)p->K * N * 8, st)) return (int)e;
    for (int o = 0; o < k_out; ++o)
        if (!(gp_host[0] == 0 && sh.has[(size_t)o * ng]))
            for (int t = 0; t < nt; ++t)
                if (hipError_t e = hipMemsetAsync(acc(t, o), 0, (size_t)pair * 8, st)) return (int)e;
    // 1. input-major
    std::vector<char> written((size_t)k_out * ng, 0);
    for (int i = 0; i < k_in; ++i) {
        if (!sh.used[i]) continue;
        const int nb = (int)ncol[i];
        // slot 0 of every token and the column's baby sums into the slots 1 .. nb (`md` is free until the tail; nt <= its group)
        if (int e = column_pairs(p, nt, in + 2 * i, 2 * k_in, nb ? bp_host + sh.koff[i] : nullptr,
                                 {nb ? bksk + sh.koff[i] : nullptr, nb, part_stride, comp_stride, row_off, key_format}, U(0), L.member, md, stream))
            return e;
        // the targets o * ng + j with a diagonal in this column, 4, 2 or 1 per launch over the input's pairs.  nt = 1: all of them in
        // one grouping.  nt > 1: A and S have different token strides and a launch takes one, so those of giant step 0 (the
        // accumulators) are grouped first, then the keyed ones
        for (int keyed = 0; keyed < (nt == 1 ? 1 : 2); ++keyed) {
            std::vector<int> ts;
            for (int o = 0; o < k_out; ++o)
                for (int j = 0; j < ng; ++j)
                    if (pt[block(o, i, j)] && (nt == 1 || (gp_host[j] != 0) == (keyed != 0))) ts.push_back(o * ng + j);
            for (size_t a0 = 0; a0 < ts.size();) {
                const size_t left = ts.size() - a0;
                const int g = left >= 4 ? 4 : left >= 2 ? 2 : 1;
                const int64_t *pts[4];
                int64_t *outs[4], strides[4];
                unsigned long long slots[4];
                int fresh[4];
                for (int k = 0; k < g; ++k) {
                    const int o = ts[a0 + k] / ng, j = ts[a0 + k] % ng;
                    const int64_t b = block(o, i, j);
                    pts[k] = pt[b], strides[k] = pt_stride[b], slots[k] = sh.masks[b], outs[k] = target(o, j), fresh[k] = !written[ts[a0 + k]];
                    written[ts[a0 + k]] = 1;
                }
                if (int e = nt == 1 ? lf_lt_block_products(g, U(0), nb + 1, pts, slots, strides, outs, fresh, rows, logN, plan_mod(p), st)
                                    : lf_lt_block_productsb(nt, g, U(0), L.member, nb + 1, pts, slots, strides, outs,
                                                            (keyed ? keyed_sums : k_out) * pair, fresh, rows, logN, plan_mod(p), st))
                    return e;
                a0 += g;
            }
        }
    }
    // 2. giant-step-major: the members (o, t) that have the giant step, output-major with the tokens of an output adjacent, 4, 2 or 1
    //    per key stream within the batch the plan is sized for (nothing where no giant step is keyed)
    const int gw = bsgs_giant_group(p);
    for (int j = 0; j < ng; ++j) {
        if (gp_host[j] == 0) continue;
        std::vector<int> ms;   // o * nt + t
        for (int o = 0; o < k_out; ++o)
            if (sh.has[(size_t)o * ng + j])
                for (int t = 0; t < nt; ++t) ms.push_back(o * nt + t);
        for (size_t a0 = 0; a0 < ms.size();) {
            const size_t left = ms.size() - a0;
            const int n = (left >= 4 && gw >= 4) ? 4 : (left >= 2 && gw >= 2) ? 2 : 1;
            int64_t *Ss[4], *accs[4];
            for (int k = 0; k < n; ++k) Ss[k] = sum(ms[a0 + k] % nt, ms[a0 + k] / nt, j), accs[k] = acc(ms[a0 + k] % nt, ms[a0 + k] / nt);
            if (int e = bsgs_giant_step(p, n, Ss, accs, gp_host[j], {gksk + j, 1, part_stride, comp_stride, row_off, key_format}, w, mdws,
                                        L.mdws_words, stream))
                return e;
            a0 += n;
        }
    }
    // 3. the tail: the nt k_out accumulators, token-major, in groups of up to 4 (a group may span two tokens): per group one exact
    //    inverse NTT (intt_exit_reduce) of its 2 g polynomials, one mod-down, one rescale into the callers' [ell - 1][N] pairs
    return matmul_tail(p, acc(0, 0), nt * k_out, md, mdws, L.mdws_words, out0, out1, rescale_scales, round_at, stream);
}

static const int64_t lt_flat_giant = 0;   // the flat entries' giant steps: the one step 0, which has no key

int lf_lt_matmul_batch(const lf_ks_plan *p, int nt, int k_in, int k_out, const int64_t *const *in, const int64_t *ncol,
                       const int64_t *p_host, const int64_t *const *ksk, int64_t part_stride, int64_t comp_stride, int64_t row_off,
                       int key_format, const int64_t *const *pt, const int64_t *pt_stride, const int64_t *bcount, const int64_t *bidx,
                       const int64_t *rescale_scales, int64_t round_at, int64_t *ws, int64_t ws_words, int64_t *const *out0,
                       int64_t *const *out1, void *stream) {
    if (!batch_ok(p, nt) || nt > LF_LT_MATMUL_BATCH_MAX_TOKENS) return LF_ERR_ARG;
    return lt_matmul_body(p, false, nt, k_in, k_out, in, ncol, p_host, ksk, 1, &lt_flat_giant, nullptr, part_stride, comp_stride, row_off,
                          key_format, pt, pt_stride, bcount, bidx, rescale_scales, round_at, ws, ws_words, out0, out1, stream);
}

int lf_lt_matmul(const lf_ks_plan *p, int k_in, int k_out, const int64_t *const *in, const int64_t *ncol, const int64_t *p_host,
                 const int64_t *const *ksk, int64_t part_stride, int64_t comp_stride, int64_t row_off, int key_format,
                 const int64_t *const *pt, const int64_t *pt_stride, const int64_t *bcount, const int64_t *bidx,
                 const int64_t *rescale_scales, int64_t round_at, int64_t *ws, int64_t ws_words, int64_t *const *out0,
                 int64_t *const *out1, void *stream) {
    return lt_matmul_body(p, false, 1, k_in, k_out, in, ncol, p_host, ksk, 1, &lt_flat_giant, nullptr, part_stride, comp_stride, row_off,
                          key_format, pt, pt_stride, bcount, bidx, rescale_scales, round_at, ws, ws_words, out0, out1, stream);
}

int lf_lt_matmul_bsgs_batch(const lf_ks_plan *p, int nt, int k_in, int k_out, const int64_t *const *in, const int64_t *ncol,
                            const int64_t *bp_host, const int64_t *const *bksk, int ng, const int64_t *gp_host,
                            const int64_t *const *gksk, int64_t part_stride, int64_t comp_stride, int64_t row_off, int key_format,
                            const int64_t *const *pt, const int64_t *pt_stride, const int64_t *gcount, const int64_t *bidx,
                            const int64_t *rescale_scales, int64_t round_at, int64_t *ws, int64_t ws_words, int64_t *const *out0,
                            int64_t *const *out1, void *stream) {
    if (!batch_ok(p, nt) || nt > LF_LT_MATMUL_BSGS_BATCH_MAX_TOKENS || !gp_host || !gksk) return LF_ERR_ARG;
    return lt_matmul_body(p, true, nt, k_in, k_out, in, ncol, bp_host, bksk, ng, gp_host, gksk, part_stride, comp_stride, row_off, key_format, pt,
                          pt_stride, gcount, bidx, rescale_scales, round_at, ws, ws_words, out0, out1, stream);
}

int lf_lt_matmul_bsgs(const lf_ks_plan *p, int k_in, int k_out, const int64_t *const *in, const int64_t *ncol, const int64_t *bp_host,
                      const int64_t *const *bksk, int ng, const int64_t *gp_host, const int64_t *const *gksk, int64_t part_stride,
                      int64_t comp_stride, int64_t row_off, int key_format, const int64_t *const *pt, const int64_t *pt_stride,
                      const int64_t *gcount, const int64_t *bidx, const int64_t *rescale_scales, int64_t round_at, int64_t *ws,
                      int64_t ws_words, int64_t *const *out0, int64_t *const *out1, void *stream) {
    if (!gp_host || !gksk) return LF_ERR_ARG;
    return lt_matmul_body(p, true, 1, k_in, k_out, in, ncol, bp_host, bksk, ng, gp_host, gksk, part_stride, comp_stride, row_off, key_format, pt,
                          pt_stride, gcount, bidx, rescale_scales, round_at, ws, ws_words, out0, out1, stream);
}

/* ---- baby-step / giant-step linear transform of many ciphertexts under the same diagonals and keys (include/ckks_hip.h): groups
 * of 4, 2 or 1 as lf_linear_transform_batch; a group of g shares every launch but the diagonal products, and each baby and giant
 * key crosses HBM once for the g ciphertexts ---- */
int64_t lf_linear_transform_bsgs_batch_ws_words(const lf_ks_plan *p, int nb, int nct) {
    if (!plan_ok(p) || nb < 0 || nb > LF_BSGS_MAX_BABY_KEYS || nct < 1 || nct > LF_LT_BATCH_MAX_CTS) return 0;
    const int g = lt_batch_group(p, nct);
    if (g == 1) return lf_linear_transform_bsgs_ws_words(p, nb);
    const int64_t N = (int64_t)1 << p->logN, pair = 2 * (int64_t)(p->ell + p->K) * N, poly = (int64_t)p->ell * N;
    const int64_t md_w = lf_ks_moddown_ws_words(g, p->ell, p->K, N), md_t = lf_ks_moddown_ws_words(2 * g, p->ell, p->K, N);
    // per member its baby pairs (slot 0: the ciphertext), the S pairs of one launch and the accumulator A; the g polynomials w, the
    // final mod-down's 2 g results, and the workspace of either mod-down (the plan's own is primed for pairs)
    return g * pair * (nb + 1 + LF_BSGS_S_PAIRS + 1) + g * poly + 2 * g * poly + (md_w > md_t ? md_w : md_t);
}

int lf_linear_transform_bsgs_batch(const lf_ks_plan *p, int nct, const int64_t *const *c0, const int64_t *const *c1, int nb,
                                   const int64_t *bp_host, const int64_t *const *bksk, int ng, const int64_t *gp_host,
                                   const int64_t *const *gksk, int64_t part_stride, int64_t comp_stride, int64_t row_off, int key_format,
                                   const int64_t *pt, int64_t pt_stride, const int64_t *gcount, const int64_t *bidx,
                                   const int64_t *rescale_scales, int64_t round_at, int64_t *ws, int64_t ws_words, int64_t *const *out0,
                                   int64_t *const *out1, void *stream) {
    if (nct < 1 || nct > LF_LT_BATCH_MAX_CTS || !c0 || !c1 || !out0 || !out1) return LF_ERR_ARG;
    if (int e = bsgs_args_ok(p, nb, bp_host, bksk, ng, gp_host, gksk, part_stride, comp_stride, key_format, pt, pt_stride, gcount, bidx,
                             rescale_scales))
        return e;
    for (int t = 0; t < nct; ++t)
        if (!c0[t] || !c1[t] || !out0[t] || !out1[t]) return LF_ERR_ARG;
    const int64_t need = lf_linear_transform_bsgs_batch_ws_words(p, nb, nct);
    if (!need || !ws || ws_words < need || ((uintptr_t)ws & 15)) return LF_ERR_ARG;
    const int ell = p->ell, rows = p->ell + p->K, logN = p->logN, dev = p->device;
    const int64_t N = (int64_t)1 << logN, poly = (int64_t)ell * N, half = (int64_t)rows * N, pair = 2 * half;
    hipStream_t st = (hipStream_t)stream;
    if (int e = lf_set_device(dev)) return e;
    for (int t0 = 0; t0 < nct;) {
        const int g = lt_batch_group(p, nct - t0);
        if (g == 1) {   // a straggler: the single op, whose workspace is the head of this one's
            if (int e = lf_linear_transform_bsgs(p, c0[t0], c1[t0], nb, bp_host, bksk, ng, gp_host, gksk, part_stride, comp_stride, row_off,
                                                 key_format, pt, pt_stride, gcount, bidx, rescale_scales, round_at, ws, ws_words, out0[t0],
                                                 out1[t0], stream))
                return e;
            t0 += 1;
            continue;
        }
        // member t: its pairs u_t [nb + 1], S_t [LF_BSGS_S_PAIRS]; then the g accumulators (one run of 2 g polynomials), w, md, mdws
        const int64_t member = (nb + 1 + LF_BSGS_S_PAIRS) * pair;
        int64_t *A = ws + g * member, *w = A + g * pair, *md = w + g * poly, *mdws = md + 2 * g * poly;
        const int64_t md_w = lf_ks_moddown_ws_words(g, ell, p->K, N), md_t = lf_ks_moddown_ws_words(2 * g, ell, p->K, N);
        const int64_t mdws_words = md_w > md_t ? md_w : md_t;
        auto U = [&](int t) { return ws + t * member; };
        auto S = [&](int t) { return ws + t * member + (nb + 1) * pair; };
        // 1., 2. slot 0 of every member = P NTT(c0), P NTT(c1) on the ordinary rows (through `md`, free until the tail), zero on the
        //    special rows; the baby steps: per baby key ONE launch into the g slots of that key
        {
            const int64_t *srcs[8];
            for (int t = 0; t < g; ++t) srcs[2 * t] = c0[t0 + t], srcs[2 * t + 1] = c1[t0 + t];
            for (int i = 0; i < 2 * g; ++i)
                if (hipError_t e = hipMemsetAsync(U(i / 2) + (i & 1) * half + poly, 0, (size_t)p->K * N * 8, st)) return (int)e;
            if (int e = column_pairs(p, g, srcs, 2, bp_host, {bksk, nb, part_stride, comp_stride, row_off, key_format}, U(0), member, md, stream))
                return e;
        }
        // 3. giant steps, LF_BSGS_S_PAIRS per launch of each member's diagonal products; giant step 0 writes the accumulators
        if (gp_host[0] != 0)
            if (hipError_t e = hipMemsetAsync(A, 0, (size_t)g * pair * 8, st)) return (int)e;
        int64_t first = 0;   // first diagonal of the giant step in the pack
        for (int i0 = 0; i0 < ng;) {
            const int left = ng - i0, gc = left >= 4 ? 4 : left >= 2 ? 2 : 1;
            const int64_t *pts[4];
            unsigned long long slots[4];
            for (int i = 0; i < gc; ++i) {
                pts[i] = pt + first * pt_stride;
                slots[i] = 0;
                for (int64_t k = 0; k < gcount[i0 + i]; ++k) slots[i] |= 1ull << bidx[first + k];
                first += gcount[i0 + i];
            }
            for (int t = 0; t < g; ++t) {
                int64_t *outs[4];
                for (int i = 0; i < gc; ++i) outs[i] = gp_host[i0 + i] == 0 ? A + t * pair : S(t) + i * pair;
                if (int e = lf_lt_diag_products(gc, U(t), nb + 1, pts, slots, pt_stride, outs, rows, logN, plan_mod(p), st)) return e;
            }
            for (int i = 0; i < gc; ++i) {
                if (gp_host[i0 + i] == 0) continue;
                int64_t *Ss[4], *accs[4];
                for (int t = 0; t < g; ++t) Ss[t] = S(t) + i * pair, accs[t] = A + t * pair;
                if (int e = bsgs_giant_step(p, g, Ss, accs, gp_host[i0 + i], {gksk + i0 + i, 1, part_stride, comp_stride, row_off, key_format}, w,
                                            mdws, mdws_words, stream))
                    return e;
            }
            i0 += gc;
        }
        // 4. the tail: ONE exact inverse NTT of the g accumulator pairs, ONE mod-down of the 2 g polynomials, ONE rescale into the
        //    callers' [ell - 1][N] pairs
        if (int e = lf_intt(A, 2 * g, rows, logN, p->ipsi, p->ipsi_dp, p->q_host, p->Ninv, 2, 0, p->_2q, p->ql, p->qh, p->kl, p->kh, dev, stream))
            return e;
        if (int e = moddown_rescale_pairs(p, A, g, md, mdws, mdws_words, out0 + t0, out1 + t0, rescale_scales, round_at, stream)) return e;
        t0 += g;
    }
    return 0;
}

/* ---- batches under one key: nct = 1, 2 or 4 ciphertexts per launch set (plan->max_nct >= nct; scratch of ciphertext t at
 * t times the single-ciphertext size).  The compositions the engine's Python used to issue step by step (_ks_batch,
 * _cc_mult_group) behind one call each. ---- */
int lf_switch_key_batch(const lf_ks_plan *p, int nct, const int64_t *const *c0, const int64_t *const *c1, int64_t gal_pinv,
                        int gal_canonical, const int64_t *ksk, int64_t part_stride, int64_t comp_stride, int64_t row_off,
                        int key_format, int64_t *const *out0, int64_t *const *out1, void *stream) {
    if (!batch_ok(p, nct) || !c1 || !ksk || !out0 || !out1) return LF_ERR_ARG;
    const int ell = p->ell, rows = p->ell + p->K, logN = p->logN, dev = p->device;
    const int64_t N = (int64_t)1 << logN, st_stride = (int64_t)ell * N;
    const int64_t *g2q = (gal_pinv && gal_canonical) ? p->_2q : nullptr;
    int64_t *states[4];
    for (int t = 0; t < nct; ++t) states[t] = p->state + t * st_stride;
    if (int e = lf_ks_digits_batch(c1, states, nct, p->dig_nparts, p->dig_desc, p->dig_tab, N, gal_pinv, g2q, p->ql, p->qh, p->kl, p->kh,
                                   dev, stream))
        return e;
    if (int e = lf_ks_core_batch(p->state, st_stride, nct, p->nparts, rows, logN, p->ext_desc, p->E, p->Ed, ksk, part_stride, comp_stride,
                                 row_off, key_format, p->ext, p->sum, p->psi, p->psi_dp, p->ipsi, p->ipsi_dp, p->Ninv, p->q_host, p->ql,
                                 p->qh, p->kl, p->kh, dev, stream))
        return e;
    const int64_t *const none[4] = {};   // (without c0 the mod-down still takes a list of addends, all NULL)
    return moddown_pairs(p, p->sum, nct, out0, out1, c0 ? c0 : none, gal_pinv, g2q, stream);
}

int lf_cc_mult_evk_batch(const lf_ks_plan *p, int nct, const int64_t *const *in, const int64_t *const *row0, const int64_t *ksk,
                         int64_t part_stride, int64_t comp_stride, int64_t row_off, int key_format, int64_t *const *out0,
                         int64_t *const *out1, void *stream) {
    if (!batch_ok(p, nct) || !p->rescale_scales || !p->PR || !p->x4 || !p->d2 || !in || !row0 || !ksk || !out0 || !out1) return LF_ERR_ARG;
    const int ell = p->ell, rows = p->ell + p->K, logN = p->logN, dev = p->device;
    const int64_t N = (int64_t)1 << logN, poly = (int64_t)ell * N;
    const int xpl = stack_planes(p);
    const int relaxed_plain = LF_NTT_RELAXED | LF_NTT_PLAIN | (xpl ? LF_NTT_PLANES : 0);
    for (int t0 = 0; t0 < nct; t0 += 2) {   // rescale + forward transform of the operands, two pairs (8 polynomials) per launch
        const int n = nct - t0 < 2 ? nct - t0 : 2;
        if (int e = lf_rescale_ntt(in + 4 * t0, row0 + 4 * t0, 4 * n, p->x4 + (int64_t)t0 * 4 * poly, ell, logN, p->rescale_scales,
                                   p->round_at, p->psi, p->psi_dp, p->q_host, p->Rs, relaxed_plain, p->_2q, p->ql, p->qh, p->kl, p->kh, dev,
                                   stream))
            return e;
    }
    // the nct products x1 * y1 through one inverse transform (product on load), their digits
    if (int e = product_digits(p, nct, stream)) return e;
    if (int e = lf_relin_core_batch(p->state, poly, nct, p->nparts, rows, logN, p->ext_desc, p->E, p->Ed, ksk, part_stride, comp_stride,
                                    row_off, key_format | (xpl ? LF_STACK_PLANES : 0), p->ext, p->sum, p->psi, p->psi_dp, p->ipsi, p->ipsi_dp, p->Ninv, p->x4, 4 * poly,
                                    p->PR, ell, p->own, p->q_host, p->ql, p->qh, p->kl, p->kh, dev, stream))
        return e;
    return moddown_pairs(p, p->sum, nct, out0, out1, nullptr, 0, nullptr, stream);
}

/* ---- the halves of an op around the digit exchange of a limb-sharded engine (one process per GPU; ckks_engine.py:746-904:
 * the reference gathers every digit on every GPU before it extends).  The plan describes THIS rank's rows at the level:
 * dig_nparts = the digits it owns, nparts = all digits, state = its own digit rows.
 *   pre    everything up to the digits this rank owns (cc_mult: rescale + forward NTT, x1 * y1, inverse NTT, digits);
 *   fwd    extension + forward NTT of digits first .. first + count - 1 of the gathered buffer (own digits while the
 *          others travel, the foreign runs after the wait);
 *   post   inner product over all digits + inverse NTT + mod-down. ---- */
int lf_cc_mult_evk_pre(const lf_ks_plan *p, const int64_t *const *in, const int64_t *const *row0, int which, void *stream) {
    if (!plan_ok(p) || !p->rescale_scales || !p->x4 || !p->d2 || !(which & 3) || (which & ~3) || ((which & 1) && (!in || !row0)))
        return LF_ERR_ARG;
    const int ell = p->ell, logN = p->logN, dev = p->device;
    const int64_t N = (int64_t)1 << logN, poly = (int64_t)ell * N;
    const int relaxed_plain = LF_NTT_RELAXED | LF_NTT_PLAIN | (stack_planes(p) ? LF_NTT_PLANES : 0);
    // which = 3: everything.  1: only the launch that reads the operands (rescale + column pass) — the one launch of this half
    // whose addresses change from call to call; 2: the rest (fixed addresses of the plan: a caller may replay it from a graph)
    const int64_t *const none[8] = {};   // (lf_rescale_ntt takes up to 8 polynomials; unused by the tiled pass)
    if (which & 1)
        if (int e = lf_rescale_ntt(in, row0, 4, p->x4, ell, logN, p->rescale_scales, p->round_at, p->psi, p->psi_dp, p->q_host, p->Rs,
                                   relaxed_plain | (which == 3 ? 0 : LF_NTT_ONLY_COLS), p->_2q, p->ql, p->qh, p->kl, p->kh, dev, stream))
            return e;
    if (!(which & 2)) return 0;
    if (which == 2)
        if (int e = lf_rescale_ntt(none, none, 4, p->x4, ell, logN, p->rescale_scales, p->round_at, p->psi, p->psi_dp, p->q_host, p->Rs,
                                   relaxed_plain | LF_NTT_ONLY_TILED, p->_2q, p->ql, p->qh, p->kl, p->kh, dev, stream))
            return e;
    return product_digits(p, 1, stream);
}

int lf_switch_key_pre(const lf_ks_plan *p, const int64_t *c1, int64_t gal_pinv, int gal_canonical, void *stream) {
    if (!plan_ok(p) || !c1) return LF_ERR_ARG;
    const int64_t *g2q = (gal_pinv && gal_canonical) ? p->_2q : nullptr;
    return lf_ks_digits_galois(c1, p->state, p->dig_nparts, p->dig_desc, p->dig_tab, (int64_t)1 << p->logN, gal_pinv, g2q, p->ql, p->qh,
                               p->kl, p->kh, p->device, stream);
}

int lf_ks_plan_fwd(const lf_ks_plan *p, const int64_t *digits, int first, int count, int relin, void *stream) {
    if (!plan_ok(p) || !digits || first < 0 || count < 0 || first + count > p->nparts) return LF_ERR_ARG;
    const int rows = p->ell + p->K;
    if (relin)
        return lf_relin_fwd(digits, first, count, rows, p->logN, p->ext_desc, p->E, p->Ed, p->ext, p->psi, p->psi_dp, p->own, p->q_host,
                            p->ql, p->qh, p->kl, p->kh, p->device, stream);
    return lf_ks_fwd(digits, count, rows, p->logN, p->ext_desc + 3 * (int64_t)first, p->E, p->Ed,
                     p->ext + (((int64_t)first * rows) << p->logN), p->psi, p->psi_dp, p->q_host, p->ql, p->qh, p->kl, p->kh, p->device, stream);
}

int lf_cc_mult_evk_post(const lf_ks_plan *p, const int64_t *ksk, int64_t part_stride, int64_t comp_stride, int64_t row_off,
                        int key_format, int64_t *out0, int64_t *out1, int which, void *stream) {
    if (!plan_ok(p) || !p->PR || !p->x4 || !(which & 3) || (which & ~3) || ((which & 1) && !ksk) || ((which & 2) && (!out0 || !out1)))
        return LF_ERR_ARG;
    const int rows = p->ell + p->K;
    // which: 1 = inner product + inverse NTT (fixed addresses: plan scratch and the key), 2 = the mod-down that writes out0 / out1
    if (which & 1)
        if (int e = lf_relin_tail(p->nparts, rows, p->logN, ksk, part_stride, comp_stride, row_off,
                                  key_format | (stack_planes(p) ? LF_STACK_PLANES : 0), p->ext, p->sum, p->ipsi,
                                  p->ipsi_dp, p->Ninv, p->x4, p->PR, p->ell, p->own, p->q_host, p->ql, p->qh, p->kl, p->kh, p->device, stream))
            return e;
    if (!(which & 2)) return 0;
    return moddown_pairs(p, p->sum, 1, &out0, &out1, nullptr, 0, nullptr, stream);
}

int lf_switch_key_post(const lf_ks_plan *p, const int64_t *c0, int64_t gal_pinv, int gal_canonical, const int64_t *ksk,
                       int64_t part_stride, int64_t comp_stride, int64_t row_off, int key_format, int64_t *out0, int64_t *out1,
                       int which, void *stream) {
    if (!plan_ok(p) || !(which & 3) || (which & ~3) || ((which & 1) && !ksk) || ((which & 2) && (!out0 || !out1))) return LF_ERR_ARG;
    const int rows = p->ell + p->K;
    const int64_t *g2q = (gal_pinv && gal_canonical) ? p->_2q : nullptr;
    if (which & 1)   // see lf_cc_mult_evk_post
        if (int e = lf_ks_tail(p->nparts, rows, p->logN, ksk, part_stride, comp_stride, row_off, key_format, p->ext, p->sum, p->ipsi, p->ipsi_dp,
                               p->Ninv, p->q_host, p->ql, p->qh, p->kl, p->kh, p->device, stream))
            return e;
    if (!(which & 2)) return 0;
    return moddown_pairs(p, p->sum, 1, &out0, &out1, &c0, gal_pinv, g2q, stream);
}

}  // extern "C"
