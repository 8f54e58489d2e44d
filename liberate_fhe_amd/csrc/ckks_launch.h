// ckks_launch.h — the host-side launch layer between the .hip files of the library: what always travels together as small value
// types, the validators of a key list and of a list of rotation exponents, and ONE declaration of every function or variable that
// one .hip file defines and another uses.  Both sides include this header, so definition and use are checked against the same
// text (tests/test_abi_cpu.py: no .hip file declares another one's symbols itself).  Host only: nothing here reaches a kernel.
#pragma once
#include "../../include/ckks_hip.h"
#include "ckks_common.h"

// the per-row moduli and Montgomery constants of the rows a launch covers (31-bit halves), and the primes themselves on the host
// (q_host: read where the rows are sorted into the two arithmetic classes; NULL where a launcher does not sort)
struct LfMod {
    const int64_t *ql, *qh, *kl, *kh, *q_host;
};
// the tables of the forward / inverse transform of those rows
struct LfFwdTab {
    const int64_t *psi_br;
    const double *psi_dp;
};
struct LfInvTab {
    const int64_t *ipsi_br;
    const double *ipsi_dp;
    const int64_t *Ninv;
};
// n switching keys of one layout: key i at ksk[i], its parts part_stride words apart, its two components comp_stride, the rows of
// this level from row_off; key_format LF_KEY_RAW or LF_KEY_PLANES
struct LfKeys {
    const int64_t *const *ksk;
    int n;
    int64_t part_stride, comp_stride, row_off;
    int key_format;
};

// every key of the list present, the format known, and a key in planes format aligned for its 16-byte loads (pointer and both
// strides); an empty list (n = 0) needs no array
static inline bool lf_keys_ok(const LfKeys &k) {
    if (k.n < 0 || (k.n && !k.ksk) || (k.key_format != LF_KEY_RAW && k.key_format != LF_KEY_PLANES)) return false;
    for (int i = 0; i < k.n; ++i) {
        if (!k.ksk[i]) return false;
        if (k.key_format == LF_KEY_PLANES && ((((uintptr_t)k.ksk[i] | (uintptr_t)(k.part_stride * 8) | (uintptr_t)(k.comp_stride * 8)) & 15)))
            return false;
    }
    return true;
}
// n rotation exponents: odd, in (0, 2N)
static inline bool lf_exponents_ok(const int64_t *p_host, int n, int logN) {
    if (n < 0 || (n && !p_host)) return false;
    for (int i = 0; i < n; ++i)
        if (p_host[i] <= 0 || p_host[i] >= ((int64_t)2 << logN) || !(p_host[i] & 1)) return false;
    return true;
}

// ---- ckks_ntt.hip ----
extern int lf_g_ws_extra_stage;   // lf_ntt_ws: the column pass takes the tiles' first stage too (lf_tune)

// ---- ckks_ks.hip ----
extern int lf_g_intt_digits;      // cc_mult's product -> digits in one launch behind the tiled pass where it qualifies (lf_tune)
// false when a row is of the fp64 class and nparts exceeds LF_FP64_MAX_DIGITS (reads q_host[0 .. rows))
bool lf_fp64_digits_ok(int nparts, int rows, const int64_t *q_host);

// Each launcher below refuses bad arguments with LF_ERR_ARG before anything is launched and before it holds the digits to their
// format (LF_ERR_STATE); its comment in ckks_ks.hip has the layouts.  key.n is the number of keys of the call.
// the key-dependent half of lf_rotate_hoisted (gathered inner product of 1, 2 or 4 keys + inverse NTT of their sums)
int lf_ks_tail_hoisted(const int64_t *p_host, int nparts, int rows, int logN, const LfKeys &key, const int64_t *ext, int64_t *s,
                       int64_t *scratch, int64_t scratch_words, const LfInvTab &it, const LfMod &m, hipStream_t st);
// the key-dependent part of lf_linear_transform (the groups' launches into one pair of sums + its inverse NTT)
int lf_ks_tail_lt(const int64_t *p_host, int nparts, int rows, int ell, int logN, const LfKeys &key, const int64_t *pt, int64_t pt_stride,
                  const int64_t *pt0, const int64_t *chat, const int64_t *ext, int64_t *s, int64_t *scratch, int64_t scratch_words,
                  const LfInvTab &it, const LfMod &m, hipStream_t st);
// .. of lf_linear_transform_batch for a group of 2 or 4 ciphertexts (the launches into the group's pairs of sums + their one inverse NTT)
int lf_ks_tail_ltb(int nct, const int64_t *p_host, int nparts, int rows, int ell, int logN, const LfKeys &key, const int64_t *pt,
                   int64_t pt_stride, const int64_t *pt0, const int64_t *chat, int64_t chat_stride, const int64_t *ext, int64_t *s,
                   int64_t *scratch, int64_t scratch_words, const LfInvTab &it, const LfMod &m, hipStream_t st);
// .. of lf_rotate_sum, and of lf_rotate_sum_batch for a group of 2 or 4 ciphertexts
int lf_ks_tail_rsum(const int64_t *p_host, int nparts, int rows, int ell, int logN, const LfKeys &key, int with_self, const int64_t *chat,
                    const int64_t *ext, int64_t *s, int64_t *scratch, int64_t scratch_words, const LfInvTab &it, const LfMod &m,
                    hipStream_t st);
int lf_ks_tail_rsumb(int nct, const int64_t *p_host, int nparts, int rows, int ell, int logN, const LfKeys &key, int with_self,
                     const int64_t *chat, int64_t chat_stride, const int64_t *ext, int64_t *s, int64_t *scratch, int64_t scratch_words,
                     const LfInvTab &it, const LfMod &m, hipStream_t st);
// the launches of lf_linear_transform_bsgs, lf_lt_matmul(_batch), lf_lt_matmul_bsgs and lf_linear_transform_bsgs_batch
int lf_ks_baby_sums(const int64_t *p_host, int nparts, int rows, int ell, int logN, const LfKeys &key, const int64_t *chat0,
                    const int64_t *ext, int64_t *u, const LfMod &m, hipStream_t st);
int lf_ks_baby_sums_batch(int nct, int64_t p, int nparts, int rows, int ell, int logN, const LfKeys &key, const int64_t *ext,
                          const int64_t *const *chat0, int64_t *const *u, const LfMod &m, hipStream_t st);
int lf_ks_giant_sums(int64_t p, int nparts, int rows, int logN, const LfKeys &key, const int64_t *ext, const int64_t *s0, int64_t *acc,
                     const LfMod &m, hipStream_t st);
int lf_ks_giant_sums_batch(int nct, int64_t p, int nparts, int rows, int logN, const LfKeys &key, const int64_t *ext,
                           const int64_t *const *s0, int64_t *const *acc, const LfMod &m, hipStream_t st);
int lf_ks_fwd_batch(const int64_t *state, int64_t state_stride, int nct, int nparts, int rows, int logN, const int64_t *desc,
                    const int64_t *E, const double *Ed, int64_t *tmp, const LfFwdTab &ft, const LfMod &m, hipStream_t st);
int lf_lt_diag_products(int ng, const int64_t *u, int nslots, const int64_t *const *pt, const unsigned long long *slots, int64_t pt_stride,
                        int64_t *const *out, int rows, int logN, const LfMod &m, hipStream_t st);
int lf_lt_block_products(int no, const int64_t *u, int nslots, const int64_t *const *pt, const unsigned long long *slots,
                         const int64_t *pt_stride, int64_t *const *out, const int *fresh, int rows, int logN, const LfMod &m,
                         hipStream_t st);
int lf_lt_block_productsb(int nt, int no, const int64_t *u, int64_t u_tstride, int nslots, const int64_t *const *pt,
                          const unsigned long long *slots, const int64_t *pt_stride, int64_t *const *out, int64_t out_tstride,
                          const int *fresh, int rows, int logN, const LfMod &m, hipStream_t st);
// the launches of lf_cc_dot(_batch) and lf_cc_matmul that are their own
int lf_dot_tensor(int g, const int64_t *x, int64_t *T, int64_t *t2, int ell, int logN, int xpl, int first, const LfMod &m, hipStream_t st);
int lf_dot_relin(const int64_t *state, int nct, int nparts, int rows, int logN, const int64_t *desc, const int64_t *E, const double *Ed,
                 const LfKeys &key, int64_t *tmp, int64_t *s, const LfFwdTab &ft, const LfInvTab &it, const int64_t *T, const int64_t *PR,
                 int ell, const uint8_t *own, const LfMod &m, hipStream_t st);
int lf_matmul_tensor(int R, int C, int k, int nu, const int64_t *x, const int *ta, const int *tb, int64_t *T, int64_t *t2, int ell,
                     int logN, int xpl, const LfMod &m, hipStream_t st);
// the launches of lf_pc_dot, lf_pc_matmul, lf_pc_matmul_batch and lf_pc_matmul_batch_planes that are their own: the tile of tokens /
// outputs a product launch takes, the fp64-class rows of a compact plaintext as a bit mask (false: more rows than it has bits), and
// the products of go outputs x gt tokens (1, 2 or 4 each) over raw or (planes) compact plaintexts
int lf_pc_dot_products(int g, const int64_t *x, const int64_t *const *pt, int64_t *S, int rows, int logN, int xpl, int first,
                       const LfMod &m, hipStream_t st);
int lf_pc_bias(int64_t *c0, const int64_t *pt, const int64_t *Rs, int rows, int logN, const LfMod &m, hipStream_t st);
int lf_pc_matmul_batch_tile(int go, int left);
int lf_pc_matmul_batch_outputs(int left, int nt);
bool lf_plain_planes_mask(int rows, const int64_t *q_host, uint64_t *mask);
int lf_pc_matmul_products(bool planes, int go, int gt, int n, const int64_t *x, int64_t xtok, const int64_t *const *pt, int pt_stride,
                          int64_t *S, int64_t stok, int rows, int logN, int xpl, int first, uint64_t small, const LfMod &m, hipStream_t st);
