// ckks_ks.hip — fused hybrid key-switch core: lf_ks_core.
//
// Replaces, for ring degrees with a two-pass NTT (logN >= 13), the chain
//     lf_ks_extend -> lf_ntt(batch = parts) -> lf_ks_inner -> lf_intt(batch = 2, tail 2)
// (reference: ckks_engine.py extend 707-743, ntt 919, mont_mult x2 931-934, sum over parts 832-840,
// intt_exit_reduce 847-848) by a pipeline that never materialises the extended digits in the
// coefficient domain and does every 40-bit-limb product with one fp64 modular multiplication:
//
//   K2  ks_ext_pass1     : every (digit p, target limb r, column tile): the tile's coefficients are
//                          computed on the fly from the digit's Garner words (extend), taken through the
//                          strided NTT pass and written once                [parts x rows x N words out]
//   P2  ntt_fwd_pass     : the stock contiguous pass, in place
//   K3  ks_inner2_kernel : per coefficient, the digits' products with the two key polynomials accumulated
//                          in registers; the key is streamed exactly once
//   K4  ntt_inv_pass_io  : the stock inverse passes (relaxed, tail 2) -> canonical coefficients
// (Variants that fuse P2 with K3 — transform a tile, multiply, accumulate over the digits in registers — were
// measured twice: round 1 on the 8-words-per-thread tile 1.6x SLOWER; round 2 on the 16-words tile, with the contiguous
// inverse pass fused in as well (one block = one (ciphertext, limb, tile), 154 / 168 VGPRs, 3 blocks per CU): gold 231 us
// against 224 us for the three launches it replaces, silver 152 against 95 us (170 blocks for 256 CUs), batches of 16
// and 64 ciphertexts +1-2 %.  Too few, too long blocks for one ciphertext, and no gain from the 490 MB of HBM traffic it
// saves once the grid is full: these passes are bound by their LDS exchanges and barriers, not by HBM; see DESIGN.md.)
//
// All of it is "relaxed" arithmetic: only residues matter because the consumer (mod-down) needs the
// canonical coefficients, which the inverse chain's tail produces.  For limbs with a prime below 2^41
// the extension and the inner product are done in the PLAIN domain with fp64 FMAs — ext = sum y_i L_{i-1}
// (no Montgomery factor), NTT with plain twiddles, times the key word k*R gives (ext*k)*R, exactly the
// Montgomery-form residue the reference's REDC(ext*R * k*R) yields — so each product is ONE fp64
// modular multiplication.  60-bit limbs keep the reference's Montgomery integer arithmetic.
#include "../../include/ckks_hip.h"
#include "ckks_ntt_core.h"
#include "ckks_ntt_tile16.h"
#include "ckks_launch.h"

#include <type_traits>

#define KS_WORDS ((1 << NTT_TILE_LOG_MAX) / NTT_THREADS)   // tile words owned by one thread (8)

// streaming stores of the extension kernels (ckks_ntt_core.h: "Streaming accesses")
#define KS_ST(p, v)                                                  \
    do {                                                             \
        if (NT_KS_EXT) __builtin_nontemporal_store((i64)(v), p);     \
        else *(p) = (v);                                             \
    } while (0)

// the same word into a row in planes format (u32 low[N] at byte 0, u16 high[N] at byte 4 N); rowb = the row's first word
#define KS_ST_PL(rowb, N, idx, v)                                                                                \
    do {                                                                                                         \
        const i64 v_ = (i64)(v);                                                                                 \
        unsigned *lo_ = uniform_at(reinterpret_cast<unsigned *>(rowb) + (idx), lane);                            \
        unsigned short *hi_ = uniform_at(reinterpret_cast<unsigned short *>((rowb) + ((N) >> 1)) + (idx), lane); \
        if (NT_KS_EXT) {                                                                                         \
            __builtin_nontemporal_store((unsigned)v_, lo_);                                                      \
            __builtin_nontemporal_store((unsigned short)(v_ >> 32), hi_);                                        \
        } else {                                                                                                 \
            *lo_ = (unsigned)v_;                                                                                 \
            *hi_ = (unsigned short)(v_ >> 32);                                                                   \
        }                                                                                                        \
    } while (0)

namespace {

struct KsGeom {
    int logN, tl, S1;
    int rows;        // target limbs on this device (with special)
    int nparts;      // digits
    i64 N;
    int nct;         // ciphertexts switched under the same key in this call (lf_ks_core_batch)
    i64 state_stride;   // words between their digit states
    // relinearisation inside cc_mult: the limbs a digit is made of are not extended (the inner product takes them from
    // the NTT-domain operands, RelinFold); own[r] = digit (numbered from the first digit of the key switch, this call
    // starting at p0) that limb r belongs to, 255 for the special limbs; nullptr: every (digit, limb) pair is extended
    const unsigned char *own;
    int p0;
    int planes;      // fp64-class rows of tmp in planes format (digit_planes(), ckks_ntt_tile16.h fwd_tile16<.., PLN>)
};

// ---- K2: extend + strided NTT pass -----------------------------------------------------------------
// desc[p] = {row_start, alpha, e_off}; E (Montgomery consts, int class) / Ed (plain consts as doubles,
// fp64 class) hold, at [e_off + i*rows + r], L_{i-1} R^2 mod q_r resp. L_{i-1} mod q_r (i = 0: R^2, 1).
template <bool DP>
__device__ __forceinline__ void ks_ext_body(i64 *sm, int b, const i64 *__restrict__ state, i64 *__restrict__ tmp,
                                            const KsGeom &kg, const RowList &rl, const i64 *__restrict__ desc,
                                            const i64 *__restrict__ E, const double *__restrict__ Ed,
                                            const i64 *__restrict__ psi_br, const double *__restrict__ psi_dp,
                                            const i64 *__restrict__ ql, const i64 *__restrict__ qh,
                                            const i64 *__restrict__ kl, const i64 *__restrict__ kh) {
    const int T = 1 << kg.tl;
    const int tiles = 1 << (kg.logN - kg.tl);
    // ciphertexts of a batch are the outermost index: each one is the single-ciphertext grid over its own state
    const int per_ct = tiles * kg.nparts * rl.n;
    const int ct = b / per_ct;
    b -= ct * per_ct;
    state += (i64)ct * kg.state_stride;
    tmp += ((i64)ct * kg.nparts * kg.rows) << kg.logN;
    // the blocks of one (digit, tile) pair differ in the target limb and re-read the same digit columns: they are
    // placed on ONE XCD (blocks b, b + 8, .. share an XCD), so those columns are fetched into one L2, once
    int ri, pt;
    if (((tiles * kg.nparts) & 7) == 0) {
        const int x = b & 7, r = b >> 3;
        ri = r % rl.n;
        pt = (r / rl.n) * 8 + x;
    } else {
        ri = b % rl.n;
        pt = b / rl.n;
    }
    const int tile = pt % tiles, p = pt / tiles;
    const int crow = rl.id[ri];
    if (kg.own != nullptr && (int)kg.own[crow] == kg.p0 + p) return;   // the digit's own limb: nothing to extend
    const PassGeom g{kg.logN, kg.tl, 1, kg.S1, 0, kg.tl - kg.S1, kg.rows, kg.nparts, 1, 0, 0, nullptr, 0, 0};

    Ctx c;
    c.m = load_mod(ql, qh, kl, kh, crow);
    c.tw_mont = psi_br + ((i64)crow << kg.logN);
    set_aux<DP>(c, psi_dp, crow, kg.logN);
    c.d = DP ? make_dp_tab(c.m, c.tw_dp) : make_dp(c.m);
    c.relaxed = 1;
    c.inv_reduce = 0;
    // desc[p] = {row_start, alpha | wide << 8, e_off}; wide = the digit's words exceed 53 bits (a digit made of
    // 60-bit primes, i.e. the base-prime digit): they are split into 31-bit halves before entering fp64
    const int row_start = (int)desc[p * 3 + 0], alpha = (int)desc[p * 3 + 1] & 0xff;
    const bool wide = ((int)desc[p * 3 + 1] >> 8) & 1;
    const i64 e_off = desc[p * 3 + 2] + crow;
    i64 *row = tmp + ((i64)(p * kg.rows + crow) << kg.logN);

    if (DP) {
        double *smd = reinterpret_cast<double *>(sm);
        double cst[KS_MAX_ALPHA], cst31[KS_MAX_ALPHA];
#pragma unroll
        for (int i = 0; i < KS_MAX_ALPHA; ++i) {
            cst[i] = i < alpha ? Ed[e_off + (i64)i * kg.rows] : 0.0;
            cst31[i] = wide ? dp_mulmod(cst[i], 2147483648.0, c.d) : 0.0;
        }
        for (int L = threadIdx.x * 2; L < T; L += NTT_THREADS * 2) {
            const i64 j = tile_gaddr(g, tile, L);
            double a0 = 0.0, a1 = 0.0;
#pragma unroll
            for (int i = 0; i < KS_MAX_ALPHA; ++i) {
                if (i < alpha) {
                    const longlong2 y = *reinterpret_cast<const longlong2 *>(state + (i64)(row_start + i) * kg.N + j);
                    if (!wide) {
                        a0 += dp_mulmod_bal(dp_from_signed(y.x), cst[i], c.d);    // signed digit words (|y| < 2^43): the formula is sign-agnostic
                        a1 += dp_mulmod_bal(dp_from_signed(y.y), cst[i], c.d);
                    } else {
                        // 31-bit halves through the native 32-bit conversions
                        a0 += dp_mulmod_bal((double)(int)(y.x >> 31), cst31[i], c.d) + dp_mulmod_bal((double)(unsigned)(y.x & 0x7fffffffll), cst[i], c.d);
                        a1 += dp_mulmod_bal((double)(int)(y.y >> 31), cst31[i], c.d) + dp_mulmod_bal((double)(unsigned)(y.y & 0x7fffffffll), cst[i], c.d);
                    }
                }
            }
            smd[PAD(L)] = a0;        // |.| < alpha * q (balanced terms)
            smd[PAD(L + 1)] = a1;
        }
        lds_barrier();
        run_fwd_stages<ArithDpR, true>(smd, g, tile, c);
        for (int L = threadIdx.x * 2; L < T; L += NTT_THREADS * 2) {
            longlong2 o;
            o.x = dp_to_word(dp_reduce(smd[PAD(L)], c.d.q, c.d.qinv));
            o.y = dp_to_word(dp_reduce(smd[PAD(L + 1)], c.d.q, c.d.qinv));
            const i64 j = tile_gaddr(g, tile, L);   // even: words j, j + 1 are neighbours (logC >= 7: the entries stop at KS_LOGN_MAX)
            if (kg.planes) {   // 8 + 4 bytes for the pair (digit_planes(): fwd_tile16<.., PLN> and the inner product read planes)
                const lf_u2_t lo = {(unsigned)o.x, (unsigned)o.y};
                *reinterpret_cast<lf_u2_t *>(reinterpret_cast<unsigned *>(row) + j) = lo;
                *reinterpret_cast<unsigned *>(reinterpret_cast<unsigned short *>(row + (kg.N >> 1)) + j) =
                    (unsigned)((u64)o.x >> 32) | ((unsigned)((u64)o.y >> 32) << 16);
            } else {
                *reinterpret_cast<longlong2 *>(row + j) = o;
            }
        }
    } else {
        i64 cst[KS_MAX_ALPHA];
#pragma unroll
        for (int i = 0; i < KS_MAX_ALPHA; ++i) cst[i] = i < alpha ? E[e_off + (i64)i * kg.rows] : 0;
        for (int L = threadIdx.x * 2; L < T; L += NTT_THREADS * 2) {
            const i64 j = tile_gaddr(g, tile, L);
            i64 a0, a1;
            if (wide && alpha > 1) {
                // several 60-bit limbs in one digit (no preset has that): term by term, as the reference extends
                a0 = a1 = 0;
#pragma unroll
                for (int i = 0; i < KS_MAX_ALPHA; ++i) {
                    if (i < alpha) {
                        const longlong2 y = *reinterpret_cast<const longlong2 *>(state + (i64)(row_start + i) * kg.N + j);
                        const i64 t0 = mm62s(y.x, cst[i], c.m.q, c.m.k), t1 = mm62s(y.y, cst[i], c.m.q, c.m.k);
                        a0 = i == 0 ? t0 : csub(a0 + t0, c.m.q2);
                        a1 = i == 0 ? t1 : csub(a1 + t1, c.m.q2);
                    }
                }
            } else {
                // sum_i y_i * (L_{i-1} R^2 mod q) in 128 bits, ONE REDC: |y_i| < 2^44 for digits of 40-bit limbs
                // (<= 8 terms, constants < 2^60: |sum| < 2^107), or a single term |y| < 2^61 — the result lies in
                // (-2^59, q + 2^59), inside the (-2q, 2q) the fold below expects
                i128 x0 = 0, x1 = 0;
#pragma unroll
                for (int i = 0; i < KS_MAX_ALPHA; ++i) {
                    if (i < alpha) {
                        const longlong2 y = *reinterpret_cast<const longlong2 *>(state + (i64)(row_start + i) * kg.N + j);
                        x0 += (i128)y.x * (i128)cst[i];
                        x1 += (i128)y.y * (i128)cst[i];
                    }
                }
                a0 = redc62_wide(x0, c.m.q, c.m.k);
                a1 = redc62_wide(x1, c.m.q, c.m.k);
            }
            sm[PAD(L)] = a0 < 0 ? a0 + c.m.q2 : a0;       // residues only: fold into [0, 2q)
            sm[PAD(L + 1)] = a1 < 0 ? a1 + c.m.q2 : a1;
        }
        lds_barrier();
        run_fwd_stages<ArithShoup, true>(sm, g, tile, c);            // residues only: Shoup products, lazy words < 8q
        for (int L = threadIdx.x * 2; L < T; L += NTT_THREADS * 2) {
            longlong2 o;
            o.x = ArithShoup::canon(c, sm[PAD(L)]);
            o.y = ArithShoup::canon(c, sm[PAD(L + 1)]);
            *reinterpret_cast<longlong2 *>(row + tile_gaddr(g, tile, L)) = o;
        }
    }
}

template <bool DP>
__global__ void __launch_bounds__(NTT_THREADS, DP ? 6 : 4) ks_ext_pass1(const i64 *__restrict__ state, i64 *__restrict__ tmp,
                                                                          KsGeom kg, RowList rl, const i64 *__restrict__ desc,
                                                                          const i64 *__restrict__ E, const double *__restrict__ Ed,
                                                                          const i64 *__restrict__ psi_br,
                                                                          const double *__restrict__ psi_dp,
                                                                          const i64 *__restrict__ ql, const i64 *__restrict__ qh,
                                                                          const i64 *__restrict__ kl, const i64 *__restrict__ kh) {
    __shared__ i64 sm[NTT_LDS_WORDS + 1];
    ks_ext_body<DP>(sm, blockIdx.x, state, tmp, kg, rl, desc, E, Ed, psi_br, psi_dp, ql, qh, kl, kh);
}

// both arithmetic classes in one launch (integer-class blocks first), see ntt_fwd_pass_mixed
#define KS_EXT_WAVES 8   // waves per SIMD the kernel is compiled for: 63 VGPRs, no spill, four blocks per CU (LDS) instead of
                         // the three of the 6-wave build (80 VGPRs); measured at gold: rotate 409-414 -> 402 us, cc_mult 557 -> 540-545 us
__global__ void __launch_bounds__(NTT_THREADS, KS_EXT_WAVES) ks_ext_pass1_mixed(const i64 *__restrict__ state, i64 *__restrict__ tmp,
                                                                       KsGeom kg, ClassLists cl, const i64 *__restrict__ desc,
                                                                       const i64 *__restrict__ E, const double *__restrict__ Ed,
                                                                       const i64 *__restrict__ psi_br,
                                                                       const double *__restrict__ psi_dp,
                                                                       const i64 *__restrict__ ql, const i64 *__restrict__ qh,
                                                                       const i64 *__restrict__ kl, const i64 *__restrict__ kh) {
    __shared__ i64 sm[NTT_LDS_WORDS + 1];
    const int b = blockIdx.x;
    if (b < cl.in_blocks) {
        if (b < cl.in_real) ks_ext_body<false>(sm, b, state, tmp, kg, cl.in, desc, E, Ed, psi_br, psi_dp, ql, qh, kl, kh);
    } else {
        ks_ext_body<true>(sm, b - cl.in_blocks, state, tmp, kg, cl.dp, desc, E, Ed, psi_br, psi_dp, ql, qh, kl, kh);
    }
}

// ---- K2, column form (used for S1 = logN - 12 <= 3): extend + the S1 leading stages as ONE register step per column ---------
// Thread = one column of one (digit, target limb): its 2^S1 words sit N / 2^S1 apart and every one of them is the
// extension sum over the digit's alpha limbs at that coefficient, so the step needs no LDS, no barrier and no
// per-lane twiddle (the 2^S1 - 1 twiddles are the table entries 1 .. 2^S1 - 1, scalar loads) — the shape of
// ntt_fwd_cols with the rescale-free extension as its source.  A wave reads / writes 512 contiguous bytes per row.
// The blocks of one (digit, column chunk) pair differ in the target limb and re-read the same digit words: they sit
// on one XCD (as in ks_ext_body).
template <bool DP, int K>
__device__ __forceinline__ void ks_ext_cols_body(int b, const i64 *__restrict__ state, i64 *__restrict__ tmp, const KsGeom &kg,
                                                 const RowList &rl, const i64 *__restrict__ desc, const i64 *__restrict__ E,
                                                 const double *__restrict__ Ed, const i64 *__restrict__ psi_br,
                                                 const double *__restrict__ psi_dp, const i64 *__restrict__ ql,
                                                 const i64 *__restrict__ qh, const i64 *__restrict__ kl,
                                                 const i64 *__restrict__ kh) {
    constexpr int R = 1 << K;
    const int logC = kg.logN - K;
    const int chunks = (1 << logC) / NTT_COL_THREADS;
    const int per_ct = chunks * kg.nparts * rl.n;
    const int ct = b / per_ct;
    b -= ct * per_ct;
    int ri, pc;
    if (((chunks * kg.nparts) & 7) == 0) {
        const int x = b & 7, r = b >> 3;
        ri = r % rl.n;
        pc = (r / rl.n) * 8 + x;
    } else {
        ri = b % rl.n;
        pc = b / rl.n;
    }
    // (integer divisions run on the VALU: pin the wave-uniform coordinates back into SGPRs)
    const int chunk = __builtin_amdgcn_readfirstlane(pc % chunks), p = __builtin_amdgcn_readfirstlane(pc / chunks);
    const int crow = __builtin_amdgcn_readfirstlane((int)rl.id[ri]);
    const int ctu = __builtin_amdgcn_readfirstlane(ct);
    if (kg.own != nullptr && (int)kg.own[crow] == kg.p0 + p) return;   // the digit's own limb: nothing to extend

    Ctx c;
    c.m = load_mod(ql, qh, kl, kh, crow);
    c.tw_mont = psi_br + ((i64)crow << kg.logN);
    set_aux<DP>(c, psi_dp, crow, kg.logN);
    c.d = DP ? make_dp_tab(c.m, c.tw_dp) : make_dp(c.m);
    c.relaxed = 1;
    c.inv_reduce = 0;
    // (pinned to SGPRs: the digit loop below runs on the scalar unit and feeds SGPR row pointers)
    const int row_start = __builtin_amdgcn_readfirstlane((int)desc[p * 3 + 0]);
    const int alpha = __builtin_amdgcn_readfirstlane((int)desc[p * 3 + 1] & 0xff);
    const bool wide = __builtin_amdgcn_readfirstlane(((int)desc[p * 3 + 1] >> 8) & 1) != 0;
    const i64 e_off = desc[p * 3 + 2] + crow;
    const unsigned lane = threadIdx.x;
    const i64 *src = state + (i64)ctu * kg.state_stride + (i64)row_start * kg.N + chunk * NTT_COL_THREADS;
    i64 *rowb = tmp + ((((i64)ctu * kg.nparts + p) * kg.rows + crow) << kg.logN);
    const i64 col0 = (i64)chunk * NTT_COL_THREADS;
    i64 *dst = rowb + col0;

    if (DP) {
        // the digit loop is a RUNTIME loop with wave-uniform constants (scalar loads): at most R loads in flight beside the
        // R accumulated words — the unrolled form kept 8 x R loads alive (90 VGPRs at R = 16, measured slower at logN 16)
        double x[R];
        // Horner form (desc[p][1] >> 16 = offset of the table of the digit's OWN primes m_i mod q_r behind the L table, 0: none):
        //     y_0 + L_0 y_1 + L_1 y_2 + ..  =  y_0 + m_0 (y_1 + m_1 (y_2 + ..)),   L_i = m_0 .. m_i
        // alpha - 1 modular products per word instead of alpha (the first constant of the sum form is 1: a wasted product)
        const int hoff = __builtin_amdgcn_readfirstlane((int)(desc[p * 3 + 1] >> 16));
        if (!wide && hoff != 0) {
            {
                const i64 *rowl = src + ((i64)(alpha - 1) << kg.logN);
#pragma unroll
                for (int k = 0; k < R; ++k) x[k] = dp_from_signed(rowl[((i64)k << logC) + lane]);
            }
            for (int i = alpha - 2; i >= 0; --i) {
                const double mi = Ed[hoff + e_off + (i64)i * kg.rows];
                const i64 *rowi = src + ((i64)i << kg.logN);   // wave-uniform (scalar base + lane offset in the loads below)
#pragma unroll
                for (int k = 0; k < R; ++k)   // |x| < 2^44 throughout: balanced product (< q / 2) + a signed digit word (< 2^43)
                    x[k] = dp_from_signed(rowi[((i64)k << logC) + lane]) + dp_mulmod_bal(x[k], mi, c.d);
            }
            cols_fwd_stages<ArithDpR, K>(x, c);
            if (kg.planes) {
#pragma unroll
                for (int k = 0; k < R; ++k) KS_ST_PL(rowb, kg.N, col0 + ((i64)k << logC), dp_to_word(dp_reduce(x[k], c.d.q, c.d.qinv)));
                return;
            }
#pragma unroll
            for (int k = 0; k < R; ++k) KS_ST(uniform_at(dst + ((i64)k << logC), lane), dp_to_word(dp_reduce(x[k], c.d.q, c.d.qinv)));
            return;
        }
#pragma unroll
        for (int k = 0; k < R; ++k) x[k] = 0.0;
        for (int i = 0; i < alpha; ++i) {
            const double cst = Ed[e_off + (i64)i * kg.rows];
            const i64 *rowi = src + ((i64)i << kg.logN);   // wave-uniform (scalar base + lane offset in the loads below)
            if (!wide) {
#pragma unroll
                for (int k = 0; k < R; ++k)   // signed digit words (|y| < 2^43): the formula is sign-agnostic
                    x[k] += dp_mulmod_bal(dp_from_signed(rowi[((i64)k << logC) + lane]), cst, c.d);
            } else {
                const double cst31 = dp_mulmod(cst, 2147483648.0, c.d);
#pragma unroll
                for (int k = 0; k < R; ++k) {   // 60-bit digit words: 31-bit halves through the native 32-bit conversions
                    const i64 y = rowi[((i64)k << logC) + lane];
                    x[k] += dp_mulmod_bal((double)(int)(y >> 31), cst31, c.d) + dp_mulmod_bal((double)(unsigned)(y & 0x7fffffffll), cst, c.d);
                }
            }
        }
        cols_fwd_stages<ArithDpR, K>(x, c);          // |x| < alpha * q on the way in (balanced terms)
        if (kg.planes) {
#pragma unroll
            for (int k = 0; k < R; ++k) KS_ST_PL(rowb, kg.N, col0 + ((i64)k << logC), dp_to_word(dp_reduce(x[k], c.d.q, c.d.qinv)));
            return;
        }
#pragma unroll
        for (int k = 0; k < R; ++k) KS_ST(uniform_at(dst + ((i64)k << logC), lane), dp_to_word(dp_reduce(x[k], c.d.q, c.d.qinv)));
    } else {
        i64 w[R];
        if (wide && alpha > 1) {   // several 60-bit limbs in one digit (no preset has that): term by term
#pragma unroll
            for (int k = 0; k < R; ++k) w[k] = 0;
            for (int i = 0; i < alpha; ++i) {
                const i64 cst = E[e_off + (i64)i * kg.rows];
                const i64 *rowi = src + ((i64)i << kg.logN);   // wave-uniform (scalar base + lane offset in the loads below)
#pragma unroll
                for (int k = 0; k < R; ++k) {
                    const i64 t = mm62s(rowi[((i64)k << logC) + lane], cst, c.m.q, c.m.k);
                    w[k] = i == 0 ? t : csub(w[k] + t, c.m.q2);
                }
            }
        } else {                   // sum_i y_i * (L_{i-1} R^2 mod q) in 128 bits, ONE REDC (see ks_ext_body); 8 words at a time
#pragma unroll
            for (int g0 = 0; g0 < R; g0 += 8) {
                constexpr int G = R < 8 ? R : 8;
                i128 acc[G];
#pragma unroll
                for (int k = 0; k < G; ++k) acc[k] = 0;
                for (int i = 0; i < alpha; ++i) {
                    const i64 cst = E[e_off + (i64)i * kg.rows];
                    const i64 *rowi = src + ((i64)i << kg.logN);   // wave-uniform (scalar base + lane offset in the loads below)
#pragma unroll
                    for (int k = 0; k < G; ++k)
                        acc[k] += (i128)rowi[((i64)(g0 + k) << logC) + lane] * (i128)cst;
                }
#pragma unroll
                for (int k = 0; k < G; ++k) w[g0 + k] = redc62_wide(acc[k], c.m.q, c.m.k);
            }
        }
#pragma unroll
        for (int k = 0; k < R; ++k) w[k] = w[k] < 0 ? w[k] + c.m.q2 : w[k];   // residues only: fold into [0, 2q)
        cols_fwd_stages<ArithShoup, K>(w, c);
#pragma unroll
        for (int k = 0; k < R; ++k) KS_ST(dst + ((i64)k << logC) + lane, ArithShoup::canon(c, w[k]));
    }
}

#ifndef KS_EXT_COLS_WAVES
#define KS_EXT_COLS_WAVES 4
#endif
template <int K>
__global__ void __launch_bounds__(NTT_COL_THREADS) __attribute__((amdgpu_waves_per_eu(K == 5 ? 2 : KS_EXT_COLS_WAVES))) ks_ext_cols_mixed(const i64 *__restrict__ state, i64 *__restrict__ tmp,
                                                                     KsGeom kg, ClassLists cl, const i64 *__restrict__ desc,
                                                                     const i64 *__restrict__ E, const double *__restrict__ Ed,
                                                                     const i64 *__restrict__ psi_br,
                                                                     const double *__restrict__ psi_dp,
                                                                     const i64 *__restrict__ ql, const i64 *__restrict__ qh,
                                                                     const i64 *__restrict__ kl, const i64 *__restrict__ kh) {
    const int b = blockIdx.x;
    if (b < cl.in_blocks) {
        if (b < cl.in_real) ks_ext_cols_body<false, K>(b, state, tmp, kg, cl.in, desc, E, Ed, psi_br, psi_dp, ql, qh, kl, kh);
    } else {
        ks_ext_cols_body<true, K>(b - cl.in_blocks, state, tmp, kg, cl.dp, desc, E, Ed, psi_br, psi_dp, ql, qh, kl, kh);
    }
}

// ---- the key in PLANES format (lf_key_planes): the HBM-bound launch reads fewer key bytes ------------------------------
// ks_inner2_kernel streams the key at the rate HBM delivers (gold cc_mult: 687 MB in 112 us, 450 MB of them key words), so
// only fewer BYTES make it shorter.  A word of an fp64-class key row is a residue below 2^41.  lf_key_planes stores the two
// components (b, a) of such a row, once per key, as
//     slot of component 0 (8 N bytes):         N / 2 groups of 16 bytes  { lo32 b[j], lo32 b[j+1], lo32 a[j], lo32 a[j+1] }
//     slot of component 1, first 4 N bytes:    N / 2 groups of  8 bytes  { hi16 b[j], hi16 b[j+1], hi16 a[j], hi16 a[j+1] }
// of the CANONICAL residues — 12 N bytes per row pair instead of 16 N; integer-class rows stay raw words in their slots.
// A thread of the inner product (two coefficients) then issues, per digit, ONE 16-byte and ONE 8-byte key load for both
// components where the raw layout needs two 16-byte loads: fewer bytes AND no more load instructions, at the register
// count of the raw kernel (a first version with four coefficients per thread and per-component planes read 25 % fewer key
// bytes at 96 .. 256 VGPRs and was no faster).  The double is assembled in registers — exponent | high word in the upper
// dword, the low word below, minus 2^52 — for the price of the raw word's conversion.  Same sums modulo q: same outputs.
// lf_key_planes: one row pair per blockIdx.y, two coefficients per thread
__global__ void __launch_bounds__(256) key_planes_kernel(const i64 *__restrict__ src_b, const i64 *__restrict__ src_a,
                                                         i64 *__restrict__ dst_b, i64 *__restrict__ dst_a, i64 N,
                                                         const i64 *__restrict__ ql, const i64 *__restrict__ qh) {
    const int r = blockIdx.y;
    const i64 j = ((i64)blockIdx.x * 256 + threadIdx.x) * 2;
    if (j >= N) return;
    const i64 q = (qh[r] << 31) | ql[r];
    const longlong2 b = *reinterpret_cast<const longlong2 *>(src_b + (i64)r * N + j);
    const longlong2 a = *reinterpret_cast<const longlong2 *>(src_a + (i64)r * N + j);
    if ((u64)q >= SMALL_PRIME_LIMIT) {
        *reinterpret_cast<longlong2 *>(dst_b + (i64)r * N + j) = b;
        *reinterpret_cast<longlong2 *>(dst_a + (i64)r * N + j) = a;
        return;
    }
    const i64 w[4] = {b.x, b.y, a.x, a.y};
    unsigned lo[4], hi[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        i64 c = w[v] % q;            // any word (lazy, signed-lazy): its canonical residue; once per key
        c = c < 0 ? c + q : c;
        lo[v] = (unsigned)c;
        hi[v] = (unsigned)(c >> 32);
    }
    const lf_u4_t l = {lo[0], lo[1], lo[2], lo[3]};
    const lf_u2_t h = {hi[0] | (hi[1] << 16), hi[2] | (hi[3] << 16)};
    *reinterpret_cast<lf_u4_t *>(reinterpret_cast<unsigned *>(dst_b + (i64)r * N) + 2 * j) = l;
    *reinterpret_cast<lf_u2_t *>(reinterpret_cast<unsigned *>(dst_a + (i64)r * N) + j) = h;
}

// The key (gold: 429 MB per key switch) is read exactly once: nontemporal loads (global_load_dwordx4 .. nt) keep it
// from displacing the digits, which the forward pass has just written, out of L2 / Infinity Cache
// (measured at gold: 124.8 -> 96.2 us together with one 16-byte column per thread instead of two).
#define KI_COLS 1
#ifndef KI_UNROLL
#define KI_UNROLL 2   // digits of the fp64-class inner product in flight per thread (measured: profiles / LAB_NOTES round 4)
#endif
__device__ __forceinline__ longlong2 ld_nt(const i64 *p) {
    longlong2 v;
    v.x = __builtin_nontemporal_load(p);
    v.y = __builtin_nontemporal_load(p + 1);
    return v;
}

// ---- K3: inner product with the key, summed over digits, on the relaxed NTT-domain words --------------
// fp64 rows: words are plain canonical residues x; x * (k R) mod q is the Montgomery-form product the
// reference's REDC(xR * kR) yields, one fp64 modular multiplication each.  Integer rows: REDC as the reference.
// grid = (N / 1024, rows); the digits' products are accumulated in registers, the key is read exactly once.
// NCT ciphertexts switched under the same key share every key word: it is read once for all of them.
// FOLD (relinearisation inside cc_mult, lf_relin_*): the first two components of the tensor product never get an inverse
// transform of their own.  Dividing by P is linear and P * d vanishes modulo every special prime, so
//     moddown(s) + d  ==  moddown(s + P * d  on the ordinary rows)
// and the addends enter HERE, in the NTT domain, from the four transformed operand polynomials:
//     s0 += P (x0 y0),   s1 += P (x0 y1 + x1 y0)          (ckks_engine.py:1095-1101, 1135-1140)
// in the representation of the accumulators (Montgomery-form residues): fp64 rows hold plain residues, so the factor is
// the number PR = P * R mod q as a double; integer rows hold Montgomery-form words and take REDC(d * PR).
struct RelinFold {
    const i64 *x;       // [nct][4][ell][N] = x0, x1, y0, y1 per ciphertext pair, as lf_rescale_ntt(RELAXED | PLAIN) leaves them
    i64 ct_stride;      // words between the stacks of consecutive pairs (the pre-summed forms: between the triplets [3][ell][N])
    const i64 *PR;      // [ell]  P * R mod q_r
    int ell;            // ordinary rows: the first `ell` of the `rows` limbs
    // own[r] = the digit limb r belongs to (nullptr: none skipped): that digit's extension to limb r IS the third tensor
    // component x1 * y1 in the NTT domain — the extension (mod q_r) of a digit's mixed-radix form to one of its own primes
    // is the residue it was built from — so it is formed here from the operands instead of being read from `ext`
    const unsigned char *own;
    int xpl;            // 1: fp64-class rows of x are planes (lf_rescale_ntt with LF_NTT_PLANES; key_format | LF_STACK_PLANES)
};

// the two words at coefficients j0, j0 + 1 of an fp64-class row: raw 16 bytes, or 8 + 4 bytes of its planes
static __device__ __forceinline__ void ld_pair_dp(const i64 *row, i64 j0, i64 N, int planes, double &a, double &b) {
    if (planes) {
        const lf_u2_t l = *reinterpret_cast<const lf_u2_t *>(reinterpret_cast<const unsigned *>(row) + j0);
        const unsigned h = *reinterpret_cast<const unsigned *>(reinterpret_cast<const unsigned short *>(row + (N >> 1)) + j0);
        a = dp_from_planes(l.x, h & 0xffffu), b = dp_from_planes(l.y, h >> 16);
    } else {
        const longlong2 v = *reinterpret_cast<const longlong2 *>(row + j0);
        a = dp_from_word(v.x), b = dp_from_word(v.y);
    }
}

template <int NCT, bool FOLD, bool PLANES, bool DPL>   // DPL: fp64-class rows of `ext` in planes format (digit_planes())
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(NCT == 4 ? ((DPL && !FOLD) ? 5 : 4) : 1))) ks_inner2_kernel(const i64 *__restrict__ ext, const i64 *__restrict__ ksk,
                                                        i64 part_stride, i64 comp_stride, i64 row_off, i64 *__restrict__ s,
                                                        int nparts, int rows, i64 N, RelinFold fold, int spl,
                                                        const i64 *__restrict__ ql, const i64 *__restrict__ qh,
                                                        const i64 *__restrict__ kl, const i64 *__restrict__ kh) {
    constexpr bool PRESUM = false;
#include "ckks_ks_inner2.h"
}

// the pre-summed form of the fold (ckks_ks_inner2.h: PRESUM): the relinearising key switch of cc_dot, one triplet
template <bool PLANES, bool DPL>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1))) ks_inner2_presum_kernel(const i64 *__restrict__ ext, const i64 *__restrict__ ksk,
                                                        i64 part_stride, i64 comp_stride, i64 row_off, i64 *__restrict__ s,
                                                        int nparts, int rows, i64 N, RelinFold fold, int spl,
                                                        const i64 *__restrict__ ql, const i64 *__restrict__ qh,
                                                        const i64 *__restrict__ kl, const i64 *__restrict__ kh) {
    constexpr int NCT = 1;
    constexpr bool FOLD = true, PRESUM = true;
#include "ckks_ks_inner2.h"
}

// the pre-summed fold for NCT = 2 or 4 triplets under one key (cc_dot_batch): a key word is read once for all of them; triplet t at
// fold.x + t * fold.ct_stride.  A name of its own, the same body.  amdgpu_waves_per_eu as ks_inner2_kernel<NCT, true, ..> (the
// folded form of the same NCT, whose register needs this one shares): that choice is carried over, NOT measured for this kernel.
template <int NCT, bool PLANES, bool DPL>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(NCT == 4 ? 4 : 1))) ks_dotb_inner_kernel(const i64 *__restrict__ ext, const i64 *__restrict__ ksk,
                                                        i64 part_stride, i64 comp_stride, i64 row_off, i64 *__restrict__ s,
                                                        int nparts, int rows, i64 N, RelinFold fold, int spl,
                                                        const i64 *__restrict__ ql, const i64 *__restrict__ qh,
                                                        const i64 *__restrict__ kl, const i64 *__restrict__ kh) {
    static_assert(NCT == 2 || NCT == 4, "one triplet: ks_inner2_presum_kernel");
    constexpr bool FOLD = true, PRESUM = true;
#include "ckks_ks_inner2.h"
}

// ---- cc_dot: the tensor products of G ciphertext pairs, summed into ONE triplet T = [3][ell][N] -----------------------------
// x = [G][4][ell][N]: x0, x1, y0, y1 per pair as lf_rescale_ntt(RELAXED | PLAIN) leaves them (xpl: fp64-class rows as planes).
//     T0 += sum x0 y0,   T1 += sum (x0 y1 + x1 y0),   T2 += sum x1 y1
// grid = (N / 512, ell) as ks_inner2_kernel; a thread owns one 16-byte column pair: it reads the 4 G operand words of each of
// its two coefficients once, sums the 3 G products in registers and makes one read-modify-write of T (first: the first chunk
// writes without reading).  Only the residues of T reach the result (the pre-summed fold above and the inverse transform of T2
// reduce), so the words are kept in the cheapest form that stays in range:
//   fp64-class rows  balanced products (|.| <= q / 2); a coefficient's sum is at most 4 pairs x 2 balanced terms plus the one
//                    canonical word read back, |.| < 4 q + q < 2^44 for q < 2^41 — far inside the exact range 2^53 of fp64 and
//                    dp_reduce's |x| < 64 q; stored as the plain canonical residue;
//   integer rows     REDC62 products, a conditional subtraction after every addition: Montgomery form below 2q throughout,
//                    the range of the existing fold's own-digit words.
// t2: where the launch of the LAST chunk leaves a second copy of T2 (its inverse transform runs in place there, while the fold
// still reads the NTT-domain words in T); nullptr otherwise.
template <int G>
__global__ void __launch_bounds__(256) dot_tensor_kernel(const i64 *__restrict__ x, i64 ct_stride, i64 *__restrict__ T, i64 *__restrict__ t2,
                                                         int ell, i64 N, int xpl, int first, const i64 *__restrict__ ql,
                                                         const i64 *__restrict__ qh, const i64 *__restrict__ kl, const i64 *__restrict__ kh) {
    const int r = blockIdx.y;
    const i64 j0 = (i64)blockIdx.x * 512 + threadIdx.x * 2;
    if (j0 >= N) return;
    const RowMod m = load_mod(ql, qh, kl, kh, r);
    const i64 pstride = (i64)ell * N;
    i64 *t = T + (i64)r * N + j0;
    longlong2 o[3];
    if (m.q < SMALL_PRIME_LIMIT) {
        const RowDp d = make_dp(m);
        double a[3][2] = {{0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}};
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const i64 *xs = x + g * ct_stride + (i64)r * N;
            double x0[2], x1[2], y0[2], y1[2];
            ld_pair_dp(xs, j0, N, xpl, x0[0], x0[1]);
            ld_pair_dp(xs + pstride, j0, N, xpl, x1[0], x1[1]);
            ld_pair_dp(xs + 2 * pstride, j0, N, xpl, y0[0], y0[1]);
            ld_pair_dp(xs + 3 * pstride, j0, N, xpl, y1[0], y1[1]);
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                a[0][e] += dp_mulmod_bal(x0[e], y0[e], d);
                a[1][e] += dp_mulmod_bal(x0[e], y1[e], d) + dp_mulmod_bal(x1[e], y0[e], d);
                a[2][e] += dp_mulmod_bal(x1[e], y1[e], d);
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (!first) {
                const longlong2 v = *reinterpret_cast<const longlong2 *>(t + c * pstride);
                a[c][0] += dp_from_word(v.x), a[c][1] += dp_from_word(v.y);
            }
            o[c].x = dp_to_word(dp_reduce(a[c][0], d.q, d.qinv));
            o[c].y = dp_to_word(dp_reduce(a[c][1], d.q, d.qinv));
        }
    } else {
        i64 a[3][2];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const i64 *xs = x + g * ct_stride + (i64)r * N + j0;
            const longlong2 X0 = *reinterpret_cast<const longlong2 *>(xs), X1 = *reinterpret_cast<const longlong2 *>(xs + pstride);
            const longlong2 Y0 = *reinterpret_cast<const longlong2 *>(xs + 2 * pstride), Y1 = *reinterpret_cast<const longlong2 *>(xs + 3 * pstride);
            const u64 x0[2] = {(u64)X0.x, (u64)X0.y}, x1[2] = {(u64)X1.x, (u64)X1.y};
            const u64 y0[2] = {(u64)Y0.x, (u64)Y0.y}, y1[2] = {(u64)Y1.x, (u64)Y1.y};
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const i64 d0 = mm62u(x0[e], y0[e], m.q, m.k);
                const i64 d1 = csub(mm62u(x0[e], y1[e], m.q, m.k) + mm62u(x1[e], y0[e], m.q, m.k), m.q2);
                const i64 d2 = mm62u(x1[e], y1[e], m.q, m.k);
                a[0][e] = g == 0 ? d0 : csub(a[0][e] + d0, m.q2);
                a[1][e] = g == 0 ? d1 : csub(a[1][e] + d1, m.q2);
                a[2][e] = g == 0 ? d2 : csub(a[2][e] + d2, m.q2);
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (!first) {
                const longlong2 v = *reinterpret_cast<const longlong2 *>(t + c * pstride);
                a[c][0] = csub(a[c][0] + v.x, m.q2), a[c][1] = csub(a[c][1] + v.y, m.q2);
            }
            o[c].x = a[c][0], o[c].y = a[c][1];
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) *reinterpret_cast<longlong2 *>(t + c * pstride) = o[c];
    if (t2 != nullptr) *reinterpret_cast<longlong2 *>(t2 + (i64)r * N + j0) = o[2];
}

// ---- pc_dot: the products of G ciphertexts with an encoded plaintext each, summed into ONE pair S = [2][rows][N] ------------
// x = [G][2][rows][N]: c0, c1 per term as lf_rescale_ntt(RELAXED | PLAIN) leaves them (xpl: fp64-class rows as planes);
// pt[g] = [rows][N]: the plaintext of term g as mc_mult builds it (NTT domain, Montgomery form on every row, lazy words below 2q).
//     S0 += sum_g pt_g c0_g,   S1 += sum_g pt_g c1_g
// grid = (N / 512, rows) as dot_tensor_kernel; a thread owns one 16-byte column pair: it reads the 2 G transformed words and the G
// plaintext words of each of its two coefficients once, sums both components in registers and makes one read-modify-write of S
// (first: the first chunk writes without reading).  Only the residues of S reach the result (its inverse transform reduces):
//   fp64-class rows  the plaintext's Montgomery word m R goes through one REDC to the plain m (a word in [0, q]), so that c m is
//                    the plain product the plain-domain inverse transform expects (ks_inner_lt_kernel treats a diagonal the same
//                    way); balanced products (|.| <= q / 2): for G = 4 a coefficient's sum is 4 balanced terms plus the one
//                    canonical word read back, |.| <= 4 q / 2 + q = 3 q < 2^43 for q < 2^41 — inside dp_reduce's |x| < 64 q and
//                    the exact range of fp64; stored as the plain canonical residue, below q < 2^41: far under the 2^46 a
//                    relaxed inverse transform takes on these rows;
//   integer rows     REDC62 products of a canonical word and a lazy one (below 2q), a conditional subtraction after every
//                    addition: Montgomery form below 2q throughout, what the relaxed inverse transform takes on these rows.
struct PcTerms {
    const i64 *pt[4];   // plaintext of term g, [rows][N]
};

template <int G>
__global__ void __launch_bounds__(256) pc_dot_kernel(const i64 *__restrict__ x, PcTerms pa, i64 *__restrict__ S, int rows, i64 N, int xpl,
                                                     int first, const i64 *__restrict__ ql, const i64 *__restrict__ qh,
                                                     const i64 *__restrict__ kl, const i64 *__restrict__ kh) {
    const int r = blockIdx.y;
    const i64 j0 = (i64)blockIdx.x * 512 + threadIdx.x * 2;
    if (j0 >= N) return;
    const RowMod m = load_mod(ql, qh, kl, kh, r);
    const i64 pstride = (i64)rows * N;
    i64 *s = S + (i64)r * N + j0;
    longlong2 o[2];
    if (m.q < SMALL_PRIME_LIMIT) {
        const RowDp d = make_dp(m);
        double a[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const i64 *xs = x + (i64)g * 2 * pstride + (i64)r * N;
            double c0[2], c1[2];
            ld_pair_dp(xs, j0, N, xpl, c0[0], c0[1]);
            ld_pair_dp(xs + pstride, j0, N, xpl, c1[0], c1[1]);
            const longlong2 w = *reinterpret_cast<const longlong2 *>(pa.pt[g] + (i64)r * N + j0);
            const double wp[2] = {dp_from_word(mm62u((u64)w.x, 1ull, m.q, m.k)), dp_from_word(mm62u((u64)w.y, 1ull, m.q, m.k))};
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                a[0][e] += dp_mulmod_bal(c0[e], wp[e], d);
                a[1][e] += dp_mulmod_bal(c1[e], wp[e], d);
            }
        }
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            if (!first) {
                const longlong2 v = *reinterpret_cast<const longlong2 *>(s + c * pstride);
                a[c][0] += dp_from_word(v.x), a[c][1] += dp_from_word(v.y);
            }
            o[c].x = dp_to_word(dp_reduce(a[c][0], d.q, d.qinv));
            o[c].y = dp_to_word(dp_reduce(a[c][1], d.q, d.qinv));
        }
    } else {
        i64 a[2][2];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const i64 *xs = x + (i64)g * 2 * pstride + (i64)r * N + j0;
            const longlong2 C0 = *reinterpret_cast<const longlong2 *>(xs), C1 = *reinterpret_cast<const longlong2 *>(xs + pstride);
            const longlong2 w = *reinterpret_cast<const longlong2 *>(pa.pt[g] + (i64)r * N + j0);
            const u64 c0[2] = {(u64)C0.x, (u64)C0.y}, c1[2] = {(u64)C1.x, (u64)C1.y}, wm[2] = {(u64)w.x, (u64)w.y};
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const i64 d0 = mm62u(c0[e], wm[e], m.q, m.k), d1 = mm62u(c1[e], wm[e], m.q, m.k);
                a[0][e] = g == 0 ? d0 : csub(a[0][e] + d0, m.q2);
                a[1][e] = g == 0 ? d1 : csub(a[1][e] + d1, m.q2);
            }
        }
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            if (!first) {
                const longlong2 v = *reinterpret_cast<const longlong2 *>(s + c * pstride);
                a[c][0] = csub(a[c][0] + v.x, m.q2), a[c][1] = csub(a[c][1] + v.y, m.q2);
            }
            o[c].x = a[c][0], o[c].y = a[c][1];
        }
    }
#pragma unroll
    for (int c = 0; c < 2; ++c) *reinterpret_cast<longlong2 *>(s + c * pstride) = o[c];
}

// pc_dot's bias: mc_add's chain on component 0 of the rescaled sum, word for word —
//     reduce_2q(mont_redc(mont_add(pt, mont_enter(c0))))
// c0 [rows][N] canonical, in place; pt [rows][N] the "add" plaintext (Montgomery form, lazy words below 2q).
__global__ void __launch_bounds__(256) pc_bias_kernel(i64 *__restrict__ c0, const i64 *__restrict__ pt, const i64 *__restrict__ Rs, i64 N,
                                                      const i64 *__restrict__ ql, const i64 *__restrict__ qh,
                                                      const i64 *__restrict__ kl, const i64 *__restrict__ kh) {
    const int r = blockIdx.y;
    const i64 j = ((i64)blockIdx.x * 256 + threadIdx.x) * 2;
    if (j >= N) return;
    const RowMod m = load_mod(ql, qh, kl, kh, r);
    const i64 rs = Rs[r], off = (i64)r * N + j;
    const longlong2 v = *reinterpret_cast<const longlong2 *>(c0 + off), w = *reinterpret_cast<const longlong2 *>(pt + off);
    longlong2 o;
    i64 t = redc62(csub(mm62s(v.x, rs, m.q, m.k) + w.x, m.q2), m.q, m.k);
    o.x = t < (i64)m.q ? t : t - (i64)m.q;
    t = redc62(csub(mm62s(v.y, rs, m.q, m.k) + w.y, m.q2), m.q, m.k);
    o.y = t < (i64)m.q ? t : t - (i64)m.q;
    *reinterpret_cast<longlong2 *>(c0 + off) = o;
}

// ---- plain planes: a "mult" plaintext with its fp64-class rows as 6-byte planes (lf_plain_planes, include/ckks_hip.h) ----------
// Rows back to back in row order: an fp64-class row is 6 N bytes — u32 lo[N], then u16 hi[N] — of v = mm62u(w, 1, q, k), the plain
// word in [0, q] pc_matmul_kernel forms from the Montgomery word w on every read; an integer-class row is its 8 N bytes as they
// are.  `small`: bit r set where row r is fp64-class (from the host primes: the offsets follow from it alone, and so does every
// address below).  Row r starts N / 4 words earlier for every fp64-class row before it.
static __device__ __forceinline__ i64 plain_planes_row(unsigned long long small, int r, i64 N) {
    return (i64)r * N - (i64)__popcll(small & ((1ull << r) - 1ull)) * (N >> 2);
}

// lf_plain_planes / lf_plain_unplanes: one row per blockIdx.y, two coefficients per thread (grid.x = N / 512)
__global__ void __launch_bounds__(256) plain_planes_kernel(const i64 *__restrict__ src, i64 *__restrict__ dst, i64 N, unsigned long long small,
                                                           const i64 *__restrict__ ql, const i64 *__restrict__ qh,
                                                           const i64 *__restrict__ kl, const i64 *__restrict__ kh) {
    const int r = blockIdx.y;
    const i64 j = ((i64)blockIdx.x * 256 + threadIdx.x) * 2;
    if (j >= N) return;
    const longlong2 w = *reinterpret_cast<const longlong2 *>(src + (i64)r * N + j);
    i64 *row = dst + plain_planes_row(small, r, N);
    if (!((small >> r) & 1ull)) {
        *reinterpret_cast<longlong2 *>(row + j) = w;
        return;
    }
    const RowMod m = load_mod(ql, qh, kl, kh, r);
    const u64 v0 = (u64)mm62u((u64)w.x, 1ull, m.q, m.k), v1 = (u64)mm62u((u64)w.y, 1ull, m.q, m.k);   // in [0, q], q < 2^41
    const lf_u2_t l = {(unsigned)v0, (unsigned)v1};
    *reinterpret_cast<lf_u2_t *>(reinterpret_cast<unsigned *>(row) + j) = l;
    *reinterpret_cast<unsigned *>(reinterpret_cast<unsigned short *>(row + (N >> 1)) + j) = (unsigned)(v0 >> 32) | ((unsigned)(v1 >> 32) << 16);
}

// the inverse: the canonical Montgomery residue on every row — v R mod q on fp64-class rows (R = 2^62: 62 doublings, once per
// plaintext), the stored word reduced once on integer-class rows (a lazy word below 2q)
__global__ void __launch_bounds__(256) plain_unplanes_kernel(const i64 *__restrict__ src, i64 *__restrict__ dst, i64 N, unsigned long long small,
                                                             const i64 *__restrict__ ql, const i64 *__restrict__ qh) {
    const int r = blockIdx.y;
    const i64 j = ((i64)blockIdx.x * 256 + threadIdx.x) * 2;
    if (j >= N) return;
    const i64 q = (qh[r] << 31) | ql[r];
    const i64 *row = src + plain_planes_row(small, r, N);
    longlong2 o;
    if (!((small >> r) & 1ull)) {
        const longlong2 w = *reinterpret_cast<const longlong2 *>(row + j);
        o.x = csub(w.x, q), o.y = csub(w.y, q);
    } else {
        const lf_u2_t l = *reinterpret_cast<const lf_u2_t *>(reinterpret_cast<const unsigned *>(row) + j);
        const unsigned h = *reinterpret_cast<const unsigned *>(reinterpret_cast<const unsigned short *>(row + (N >> 1)) + j);
        i64 a = csub((i64)(((u64)(h & 0xffffu) << 32) | l.x), q), b = csub((i64)(((u64)(h >> 16) << 32) | l.y), q);
        for (int s = 0; s < 62; ++s) a = csub(a << 1, q), b = csub(b << 1, q);
        o.x = a, o.y = b;
    }
    *reinterpret_cast<longlong2 *>(dst + (i64)r * N + j) = o;
}

// ---- pc_matmul, pc_matmul_batch and both over plain planes: GO outputs' sums over the SAME n transformed ciphertexts, for each of
// GT token vectors that share the plaintexts (a plaintext matrix times a vector resp. a matrix of ciphertexts) --------------------
// x: token t's chunk [n][2][rows][N] at x + t * xtok, the transformed pairs as pc_dot_kernel reads them (xpl: fp64-class rows as
// planes); pa.pt[i][g]: the plaintext of input i for output g of the group, the SAME table for every token, nullptr for an absent
// term (kernel arguments: the test is uniform over the launch); S: token t's group [GO][2][rows][N] at S + t * stok (first: written
// without being read, zeros where an output has no term in the chunk).
//     S0_{t,g} += sum_i pt_{i,g} c0_{t,i},   S1_{t,g} += sum_i pt_{i,g} c1_{t,i}
// grid and thread as pc_dot_kernel; the loop over the inputs is a run-time one.  Per input a thread loads the two transformed pairs
// of each of its GT tokens ONCE for its GO outputs (ordinary loads: the next group reads them again) and, per non-NULL output of
// its group, the plaintext pair ONCE (nontemporal), and forms the GO GT 2 2 products from registers: the plaintext stream, the
// larger one at GT = 1, is divided by GT.  The plaintext side:
//   PLANES = false  pt = [rows][N] Montgomery words (lazy, below 2q), one 16-byte pair per thread; a row is fp64-class where its
//                   prime is below SMALL_PRIME_LIMIT, and there the pair goes through one REDC to the plain word (mm62u(w, 1)) — once
//                   per read, not once per token;
//   PLANES = true   pt in the format above, `small` marking its fp64-class rows: the class is bit r of `small` and the row starts at
//                   plain_planes_row.  On fp64-class rows a thread loads the lo pair (8 bytes) and the hi pair (4 bytes) and
//                   assembles the plain word with dp_from_planes: the REDC ran once, in the packer.  On integer-class rows it reads
//                   the 16-byte pair at the row's compact offset.  The words that enter the sums are those of PLANES = false on the
//                   plaintexts the planes were packed from.
// The arithmetic is pc_dot_kernel's; only the residues of S reach the result, so the grouping of the additions is free.  Bounds per
// (token, output) accumulator over a chunk of n <= LF_PC_MATMUL_CI inputs:
//   fp64-class rows  n balanced products (|.| <= q / 2 each) plus the one canonical word read back:
//                    |.| <= LF_PC_MATMUL_CI q / 2 + q <= 9 q < 2^45 for q < 2^41 — inside dp_reduce's |x| < 64 q (which holds up to
//                    a chunk of 125) and the exact range of fp64; stored as the plain canonical residue;
//   integer rows     a conditional subtraction after every addition: Montgomery form below 2q throughout.
// So output (t, g) of any (GT, PLANES) has the words GT = 1, PLANES = false gives on token t.
struct PcMatTerms {
    const i64 *pt[LF_PC_MATMUL_CI][4];   // [input of the chunk][output of the group], [rows][N] each or nullptr
};
static_assert(LF_PC_MATMUL_CI >= 1 && LF_PC_MATMUL_CI / 2 + 1 < 64, "pc_products: a chunk's sum must stay inside dp_reduce's |x| < 64 q");

template <int GO, int GT, bool PLANES>
static __device__ __forceinline__ void pc_products(const i64 *__restrict__ x, i64 xtok, PcMatTerms pa, i64 *__restrict__ S, i64 stok, int n,
                                                   int rows, i64 N, int xpl, int first, unsigned long long small,
                                                   const i64 *__restrict__ ql, const i64 *__restrict__ qh, const i64 *__restrict__ kl,
                                                   const i64 *__restrict__ kh) {
    const int r = blockIdx.y;
    const i64 j0 = (i64)blockIdx.x * 512 + threadIdx.x * 2;
    if (j0 >= N) return;
    const RowMod m = load_mod(ql, qh, kl, kh, r);
    const i64 pstride = (i64)rows * N, o0 = (i64)r * N + j0;
    i64 po = (i64)r * N;   // where row r of a plaintext starts (uniform over the block)
    if constexpr (PLANES) po = plain_planes_row(small, r, N);
    i64 *s = S + o0;
    if (PLANES ? (small >> r) & 1ull : m.q < SMALL_PRIME_LIMIT) {
        const RowDp d = make_dp(m);
        double a[GT][GO][2][2];
#pragma unroll
        for (int t = 0; t < GT; ++t)
#pragma unroll
            for (int g = 0; g < GO; ++g) a[t][g][0][0] = a[t][g][0][1] = a[t][g][1][0] = a[t][g][1][1] = 0.0;
        for (int i = 0; i < n; ++i) {
            double c0[GT][2], c1[GT][2];
#pragma unroll
            for (int t = 0; t < GT; ++t) {
                const i64 *xs = x + t * xtok + (i64)i * 2 * pstride + (i64)r * N;
                ld_pair_dp(xs, j0, N, xpl, c0[t][0], c0[t][1]);
                ld_pair_dp(xs + pstride, j0, N, xpl, c1[t][0], c1[t][1]);
            }
#pragma unroll
            for (int g = 0; g < GO; ++g) {
                const i64 *p = pa.pt[i][g];
                if (p == nullptr) continue;   // (uniform: a kernel argument)
                double wp[2];
                if constexpr (PLANES) {
                    const lf_u2_t l = __builtin_nontemporal_load(reinterpret_cast<const lf_u2_t *>(reinterpret_cast<const unsigned *>(p + po) + j0));
                    const unsigned h = __builtin_nontemporal_load(
                        reinterpret_cast<const unsigned *>(reinterpret_cast<const unsigned short *>(p + po + (N >> 1)) + j0));
                    wp[0] = dp_from_planes(l.x, h & 0xffffu), wp[1] = dp_from_planes(l.y, h >> 16);
                } else {
                    const longlong2 w = ld_nt(p + po + j0);
                    wp[0] = dp_from_word(mm62u((u64)w.x, 1ull, m.q, m.k)), wp[1] = dp_from_word(mm62u((u64)w.y, 1ull, m.q, m.k));
                }
#pragma unroll
                for (int t = 0; t < GT; ++t)
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        a[t][g][0][e] += dp_mulmod_bal(c0[t][e], wp[e], d);
                        a[t][g][1][e] += dp_mulmod_bal(c1[t][e], wp[e], d);
                    }
            }
        }
#pragma unroll
        for (int t = 0; t < GT; ++t)
#pragma unroll
            for (int g = 0; g < GO; ++g)
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    i64 *at = s + t * stok + (2 * g + c) * pstride;
                    if (!first) {
                        const longlong2 v = *reinterpret_cast<const longlong2 *>(at);
                        a[t][g][c][0] += dp_from_word(v.x), a[t][g][c][1] += dp_from_word(v.y);
                    }
                    longlong2 o;
                    o.x = dp_to_word(dp_reduce(a[t][g][c][0], d.q, d.qinv));
                    o.y = dp_to_word(dp_reduce(a[t][g][c][1], d.q, d.qinv));
                    *reinterpret_cast<longlong2 *>(at) = o;
                }
    } else {
        i64 a[GT][GO][2][2];
#pragma unroll
        for (int t = 0; t < GT; ++t)
#pragma unroll
            for (int g = 0; g < GO; ++g) a[t][g][0][0] = a[t][g][0][1] = a[t][g][1][0] = a[t][g][1][1] = 0;
        for (int i = 0; i < n; ++i) {
            u64 c0[GT][2], c1[GT][2];
#pragma unroll
            for (int t = 0; t < GT; ++t) {
                const i64 *xs = x + t * xtok + (i64)i * 2 * pstride + o0;
                const longlong2 C0 = *reinterpret_cast<const longlong2 *>(xs), C1 = *reinterpret_cast<const longlong2 *>(xs + pstride);
                c0[t][0] = (u64)C0.x, c0[t][1] = (u64)C0.y, c1[t][0] = (u64)C1.x, c1[t][1] = (u64)C1.y;
            }
#pragma unroll
            for (int g = 0; g < GO; ++g) {
                const i64 *p = pa.pt[i][g];
                if (p == nullptr) continue;
                const longlong2 w = ld_nt(p + po + j0);
                const u64 wm[2] = {(u64)w.x, (u64)w.y};
#pragma unroll
                for (int t = 0; t < GT; ++t)
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        a[t][g][0][e] = csub(a[t][g][0][e] + mm62u(c0[t][e], wm[e], m.q, m.k), m.q2);
                        a[t][g][1][e] = csub(a[t][g][1][e] + mm62u(c1[t][e], wm[e], m.q, m.k), m.q2);
                    }
            }
        }
#pragma unroll
        for (int t = 0; t < GT; ++t)
#pragma unroll
            for (int g = 0; g < GO; ++g)
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    i64 *at = s + t * stok + (2 * g + c) * pstride;
                    if (!first) {
                        const longlong2 v = *reinterpret_cast<const longlong2 *>(at);
                        a[t][g][c][0] = csub(a[t][g][c][0] + v.x, m.q2), a[t][g][c][1] = csub(a[t][g][c][1] + v.y, m.q2);
                    }
                    longlong2 o;
                    o.x = a[t][g][c][0], o.y = a[t][g][c][1];
                    *reinterpret_cast<longlong2 *>(at) = o;
                }
    }
}

// The kernels under the names profiles, traces and the tracked resource table know them by: one token and raw plaintexts
// (lf_pc_matmul), GT = 2 | 4 tokens and raw plaintexts (lf_pc_matmul_batch), GT = 1 | 2 | 4 tokens and compact plaintexts
// (lf_pc_matmul_batch_planes).
template <int GO>
__global__ void __launch_bounds__(256) pc_matmul_kernel(const i64 *__restrict__ x, PcMatTerms pa, i64 *__restrict__ S, int n, int rows, i64 N,
                                                        int xpl, int first, const i64 *__restrict__ ql, const i64 *__restrict__ qh,
                                                        const i64 *__restrict__ kl, const i64 *__restrict__ kh) {
    pc_products<GO, 1, false>(x, 0, pa, S, 0, n, rows, N, xpl, first, 0ull, ql, qh, kl, kh);
}

template <int GO, int GT>
__global__ void __launch_bounds__(256) pc_matmulb_kernel(const i64 *__restrict__ x, i64 xtok, PcMatTerms pa, i64 *__restrict__ S, i64 stok,
                                                         int n, int rows, i64 N, int xpl, int first, const i64 *__restrict__ ql,
                                                         const i64 *__restrict__ qh, const i64 *__restrict__ kl,
                                                         const i64 *__restrict__ kh) {
    pc_products<GO, GT, false>(x, xtok, pa, S, stok, n, rows, N, xpl, first, 0ull, ql, qh, kl, kh);
}

template <int GO, int GT>
__global__ void __launch_bounds__(256) pc_planes_matmul_kernel(const i64 *__restrict__ x, i64 xtok, PcMatTerms pa, i64 *__restrict__ S, i64 stok,
                                                               int n, int rows, i64 N, int xpl, int first, unsigned long long small,
                                                               const i64 *__restrict__ ql, const i64 *__restrict__ qh,
                                                               const i64 *__restrict__ kl, const i64 *__restrict__ kh) {
    pc_products<GO, GT, true>(x, xtok, pa, S, stok, n, rows, N, xpl, first, small, ql, qh, kl, kh);
}

// ---- cc_matmul: the summed triplets of an R x C tile of C = A B, every operand of the tile read once per inner index ----------
// x = [nu][2][ell][N]: the resident store of the DISTINCT operands, c0, c1 of each as lf_rescale_ntt(RELAXED | PLAIN) leaves them
// (xpl: fp64-class rows as planes).  ix.a[t][i] / ix.b[t][j]: the operand that is A[i0 + i][t] resp. B[t][j0 + j], or -1 for a zero
// entry (kernel arguments: every test on them is uniform over the launch).  Output d = i C + j of the tile:
//     T0_d = sum_t x0 y0,   T1_d = sum_t (x0 y1 + x1 y0),   T2_d = sum_t x1 y1      (x = A[i0 + i][t], y = B[t][j0 + j])
// written ONCE to T + d * 3 ell N (no read-modify-write: the whole inner dimension is summed in registers), T2_d a second time to
// t2 + d * ell N, where its inverse transform runs in place.  grid and thread as dot_tensor_kernel; the loop over t is a run-time
// one: a thread loads the R + C operand pairs of an inner index once and forms the R C products of that index from registers —
// dot_tensor_kernel reads four operand polynomials per product.  The arithmetic is dot_tensor_kernel's, and only the residues of T
// reach the result, so the words are those of lf_cc_dot on each output's pairs:
//   fp64-class rows  balanced products (|.| <= q / 2): one inner index adds at most q / 2 to |T0|, |T2| and q to |T1|.  dp_reduce
//                    takes |x| < 64 q, so at most 63 indices could be summed between two reductions; the accumulators are reduced
//                    in registers (to [0, q)) after every LF_MATMUL_REDUCE_EVERY = 32 indices: |.| < q + 32 q = 33 q < 2^47 for
//                    q < 2^41 — inside dp_reduce's range and the exact range 2^53 of fp64 for any inner dimension; stored as the
//                    plain canonical residue, which does not depend on where the reductions fell;
//   integer rows     REDC62 products of words below 2q are below 2q (q < 2^60); a conditional subtraction after every addition
//                    makes every sum an addition mod 2q of words below 2q — associative and commutative, so the words do not
//                    depend on the grouping (dot_tensor_kernel's chunks of 4) and the zero the accumulators start from changes
//                    none: Montgomery form below 2q throughout.
#define LF_MATMUL_REDUCE_EVERY 32
static_assert(LF_MATMUL_REDUCE_EVERY + 1 < 64, "matmul_tensor_kernel: a run of inner indices must stay inside dp_reduce's |x| < 64 q");
static_assert(LF_CC_MATMUL_MAX_OPERANDS <= 32767, "MatmulIdx keeps operand indices in 16 bits");
struct MatmulIdx {
    short a[LF_CC_MATMUL_MAX_INNER][4];   // [inner index][row of the tile]
    short b[LF_CC_MATMUL_MAX_INNER][4];   // [inner index][column of the tile]
};

template <int R, int C>
__global__ void __launch_bounds__(256) matmul_tensor_kernel(const i64 *__restrict__ x, MatmulIdx ix, int k, i64 *__restrict__ T,
                                                            i64 *__restrict__ t2, int ell, i64 N, int xpl, const i64 *__restrict__ ql,
                                                            const i64 *__restrict__ qh, const i64 *__restrict__ kl,
                                                            const i64 *__restrict__ kh) {
    static_assert(R * C == 1 || R * C == 2 || R * C == 4, "a tile has 1, 2 or 4 outputs");
    constexpr int D = R * C;
    const int r = blockIdx.y;
    const i64 j0 = (i64)blockIdx.x * 512 + threadIdx.x * 2;
    if (j0 >= N) return;
    const RowMod m = load_mod(ql, qh, kl, kh, r);
    const i64 pstride = (i64)ell * N, o0 = (i64)r * N + j0;
    longlong2 o[D][3];
    if (m.q < SMALL_PRIME_LIMIT) {
        const RowDp d = make_dp(m);
        double acc[D][3][2];
#pragma unroll
        for (int i = 0; i < D; ++i)
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[i][c][0] = acc[i][c][1] = 0.0;
        for (int tb = 0; tb < k; tb += LF_MATMUL_REDUCE_EVERY) {
            const int te = tb + LF_MATMUL_REDUCE_EVERY < k ? tb + LF_MATMUL_REDUCE_EVERY : k;
            if (tb) {   // (uniform) the run before this one left |.| <= 33 q: back to [0, q)
#pragma unroll
                for (int i = 0; i < D; ++i)
#pragma unroll
                    for (int c = 0; c < 3; ++c)
#pragma unroll
                        for (int e = 0; e < 2; ++e) acc[i][c][e] = dp_reduce(acc[i][c][e], d.q, d.qinv);
            }
            for (int t = tb; t < te; ++t) {
                double a0[R][2], a1[R][2], b0[C][2], b1[C][2];
#pragma unroll
                for (int i = 0; i < R; ++i) {
                    a0[i][0] = a0[i][1] = a1[i][0] = a1[i][1] = 0.0;
                    const int u = ix.a[t][i];
                    if (u < 0) continue;
                    const i64 *p = x + (i64)u * 2 * pstride + (i64)r * N;
                    ld_pair_dp(p, j0, N, xpl, a0[i][0], a0[i][1]);
                    ld_pair_dp(p + pstride, j0, N, xpl, a1[i][0], a1[i][1]);
                }
#pragma unroll
                for (int j = 0; j < C; ++j) {
                    b0[j][0] = b0[j][1] = b1[j][0] = b1[j][1] = 0.0;
                    const int u = ix.b[t][j];
                    if (u < 0) continue;
                    const i64 *p = x + (i64)u * 2 * pstride + (i64)r * N;
                    ld_pair_dp(p, j0, N, xpl, b0[j][0], b0[j][1]);
                    ld_pair_dp(p + pstride, j0, N, xpl, b1[j][0], b1[j][1]);
                }
#pragma unroll
                for (int i = 0; i < R; ++i)
#pragma unroll
                    for (int j = 0; j < C; ++j) {
                        if (ix.a[t][i] < 0 || ix.b[t][j] < 0) continue;   // a zero entry: no product
#pragma unroll
                        for (int e = 0; e < 2; ++e) {
                            acc[i * C + j][0][e] += dp_mulmod_bal(a0[i][e], b0[j][e], d);
                            acc[i * C + j][1][e] += dp_mulmod_bal(a0[i][e], b1[j][e], d) + dp_mulmod_bal(a1[i][e], b0[j][e], d);
                            acc[i * C + j][2][e] += dp_mulmod_bal(a1[i][e], b1[j][e], d);
                        }
                    }
            }
        }
#pragma unroll
        for (int i = 0; i < D; ++i)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                o[i][c].x = dp_to_word(dp_reduce(acc[i][c][0], d.q, d.qinv));
                o[i][c].y = dp_to_word(dp_reduce(acc[i][c][1], d.q, d.qinv));
            }
    } else {
        i64 acc[D][3][2];
#pragma unroll
        for (int i = 0; i < D; ++i)
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[i][c][0] = acc[i][c][1] = 0;
        for (int t = 0; t < k; ++t) {
            u64 a0[R][2], a1[R][2], b0[C][2], b1[C][2];
#pragma unroll
            for (int i = 0; i < R; ++i) {
                a0[i][0] = a0[i][1] = a1[i][0] = a1[i][1] = 0;
                const int u = ix.a[t][i];
                if (u < 0) continue;
                const i64 *p = x + (i64)u * 2 * pstride + o0;
                const longlong2 v0 = *reinterpret_cast<const longlong2 *>(p), v1 = *reinterpret_cast<const longlong2 *>(p + pstride);
                a0[i][0] = (u64)v0.x, a0[i][1] = (u64)v0.y, a1[i][0] = (u64)v1.x, a1[i][1] = (u64)v1.y;
            }
#pragma unroll
            for (int j = 0; j < C; ++j) {
                b0[j][0] = b0[j][1] = b1[j][0] = b1[j][1] = 0;
                const int u = ix.b[t][j];
                if (u < 0) continue;
                const i64 *p = x + (i64)u * 2 * pstride + o0;
                const longlong2 v0 = *reinterpret_cast<const longlong2 *>(p), v1 = *reinterpret_cast<const longlong2 *>(p + pstride);
                b0[j][0] = (u64)v0.x, b0[j][1] = (u64)v0.y, b1[j][0] = (u64)v1.x, b1[j][1] = (u64)v1.y;
            }
#pragma unroll
            for (int i = 0; i < R; ++i)
#pragma unroll
                for (int j = 0; j < C; ++j) {
                    if (ix.a[t][i] < 0 || ix.b[t][j] < 0) continue;
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        const i64 d0 = mm62u(a0[i][e], b0[j][e], m.q, m.k);
                        const i64 d1 = csub(mm62u(a0[i][e], b1[j][e], m.q, m.k) + mm62u(a1[i][e], b0[j][e], m.q, m.k), m.q2);
                        const i64 d2 = mm62u(a1[i][e], b1[j][e], m.q, m.k);
                        acc[i * C + j][0][e] = csub(acc[i * C + j][0][e] + d0, m.q2);
                        acc[i * C + j][1][e] = csub(acc[i * C + j][1][e] + d1, m.q2);
                        acc[i * C + j][2][e] = csub(acc[i * C + j][2][e] + d2, m.q2);
                    }
                }
        }
#pragma unroll
        for (int i = 0; i < D; ++i)
#pragma unroll
            for (int c = 0; c < 3; ++c) o[i][c].x = acc[i][c][0], o[i][c].y = acc[i][c][1];
    }
#pragma unroll
    for (int i = 0; i < D; ++i) {
#pragma unroll
        for (int c = 0; c < 3; ++c) *reinterpret_cast<longlong2 *>(T + (i64)(3 * i + c) * pstride + o0) = o[i][c];
        *reinterpret_cast<longlong2 *>(t2 + (i64)i * pstride + o0) = o[i][2];
    }
}

// ---- K3 of hoisted rotations (lf_rotate_hoisted): ONE ciphertext's extended digits, NR keys with an exponent each ----------
// X -> X^p permutes the NTT slots: NTT(a(X^p))[k] = NTT(a)[pi_p(k)], pi_p(k) = brev(((2 brev(k) + 1) p mod 2N - 1) / 2) (the forward
// transform stores the evaluation at psi^(2 brev(k) + 1) at index k).  So the digits of c1, extended and transformed ONCE, serve every
// rotation: key i reads them gathered by pi_{p_i}.  pi maps every aligned block of 2^m slots onto an aligned block, permuted inside:
// the thread's pair (j0, j0 + 1) is the pair at pi(j0) & ~1, its two words swapped where pi(j0) is odd, and the 64 pairs of a wave
// are one aligned run of 128 slots under every p — the NR keys of a group read the same runs, and ext crosses HBM about once per group.
// pi is computed in registers (two bit reversals, a multiply, a mask per pair and key: issue slots this HBM-bound launch has spare).
struct HoistKeys {
    const i64 *ksk[4];   // key i, at its first part (row_off and the part / component strides are those of every key)
    unsigned p[4];       // its exponent (odd, < 2N)
};

template <int NR, bool PLANES, bool DPL>   // DPL: fp64-class rows of `ext` in planes format (digit_planes())
__global__ void __launch_bounds__(256) ks_inner_hoist_kernel(const i64 *__restrict__ ext, HoistKeys hk, i64 part_stride, i64 comp_stride,
                                                             i64 row_off, i64 *__restrict__ s, int nparts, int rows, int logN, int spl,
                                                             const i64 *__restrict__ ql, const i64 *__restrict__ qh,
                                                             const i64 *__restrict__ kl, const i64 *__restrict__ kh) {
    const int r = blockIdx.y;
    const i64 N = (i64)1 << logN;
    const i64 j0 = (i64)blockIdx.x * 512 + threadIdx.x * 2;
    if (j0 >= N) return;
    const RowMod m = load_mod(ql, qh, kl, kh, r);
    const unsigned sh = 32u - (unsigned)logN, mask = (2u << logN) - 1u;
    const unsigned bj = (2u * (__builtin_bitreverse32((unsigned)j0) >> sh) + 1u);
    unsigned src[NR];   // first slot of the source pair of key i
    bool sw[NR];        // its words swapped
#pragma unroll
    for (int i = 0; i < NR; ++i) {
        const unsigned t = (bj * hk.p[i]) & mask;   // (2 brev(j0) + 1) p mod 2N: odd
        const unsigned mi = __builtin_bitreverse32((t - 1u) >> 1) >> sh;
        src[i] = mi & ~1u;
        sw[i] = (mi & 1u) != 0;
    }
    const i64 ct_s = 2 * (i64)rows * N;   // words between the keys' output pairs
    const i64 krow = (row_off + r) * N;
    if (m.q < SMALL_PRIME_LIMIT) {
        const RowDp d = make_dp(m);
        double acc[NR][2][2];
#pragma unroll
        for (int i = 0; i < NR; ++i) acc[i][0][0] = acc[i][0][1] = acc[i][1][0] = acc[i][1][1] = 0.0;
#pragma unroll KI_UNROLL
        for (int p = 0; p < nparts; ++p) {
            const i64 *er = ext + ((i64)p * rows + r) * N;
#pragma unroll
            for (int i = 0; i < NR; ++i) {
                double xa, xb;
                ld_pair_dp(er, (i64)src[i], N, DPL ? 1 : 0, xa, xb);
                const double x0 = sw[i] ? xb : xa, x1 = sw[i] ? xa : xb;
                const i64 *kr = hk.ksk[i] + krow + (i64)p * part_stride;
                double k0x, k0y, k1x, k1y;
                if (PLANES) {   // 16 + 8 bytes for both components (see lf_key_planes)
                    const lf_u4_t l = __builtin_nontemporal_load(reinterpret_cast<const lf_u4_t *>(reinterpret_cast<const unsigned *>(kr) + 2 * j0));
                    const lf_u2_t h = __builtin_nontemporal_load(reinterpret_cast<const lf_u2_t *>(reinterpret_cast<const unsigned *>(kr + comp_stride) + j0));
                    k0x = dp_from_planes(l.x, h.x & 0xffffu), k0y = dp_from_planes(l.y, h.x >> 16);
                    k1x = dp_from_planes(l.z, h.y & 0xffffu), k1y = dp_from_planes(l.w, h.y >> 16);
                } else {
                    const longlong2 k0 = ld_nt(kr + j0);
                    const longlong2 k1 = ld_nt(kr + j0 + comp_stride);
                    k0x = dp_from_word(k0.x), k0y = dp_from_word(k0.y), k1x = dp_from_word(k1.x), k1y = dp_from_word(k1.y);
                }
                acc[i][0][0] += dp_mulmod_bal(x0, k0x, d);
                acc[i][0][1] += dp_mulmod_bal(x1, k0y, d);
                acc[i][1][0] += dp_mulmod_bal(x0, k1x, d);
                acc[i][1][1] += dp_mulmod_bal(x1, k1y, d);
            }
        }
#pragma unroll
        for (int i = 0; i < NR; ++i)
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                longlong2 o;
                o.x = dp_to_word(dp_reduce(acc[i][c][0], d.q, d.qinv));
                o.y = dp_to_word(dp_reduce(acc[i][c][1], d.q, d.qinv));
                i64 *srow = s + i * ct_s + ((i64)c * rows + r) * N;
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
        i64 acc[NR][2][2];
#pragma unroll
        for (int i = 0; i < NR; ++i) acc[i][0][0] = acc[i][0][1] = acc[i][1][0] = acc[i][1][1] = 0;
        for (int p = 0; p < nparts; ++p) {
            const i64 *er = ext + ((i64)p * rows + r) * N;
#pragma unroll
            for (int i = 0; i < NR; ++i) {
                const longlong2 v = *reinterpret_cast<const longlong2 *>(er + src[i]);
                const u64 x0 = (u64)(sw[i] ? v.y : v.x), x1 = (u64)(sw[i] ? v.x : v.y);
                const i64 *kr = hk.ksk[i] + krow + (i64)p * part_stride + j0;
                const longlong2 k0 = ld_nt(kr);
                const longlong2 k1 = ld_nt(kr + comp_stride);
                acc[i][0][0] = csub(acc[i][0][0] + mm62u(x0, (u64)k0.x, m.q, m.k), m.q2);
                acc[i][0][1] = csub(acc[i][0][1] + mm62u(x1, (u64)k0.y, m.q, m.k), m.q2);
                acc[i][1][0] = csub(acc[i][1][0] + mm62u(x0, (u64)k1.x, m.q, m.k), m.q2);
                acc[i][1][1] = csub(acc[i][1][1] + mm62u(x1, (u64)k1.y, m.q, m.k), m.q2);
            }
        }
#pragma unroll
        for (int i = 0; i < NR; ++i)
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                longlong2 o;
                o.x = acc[i][c][0];
                o.y = acc[i][c][1];
                *reinterpret_cast<longlong2 *>(s + i * ct_s + ((i64)c * rows + r) * N + j0) = o;
            }
    }
}

// ---- K3 of a linear transform (lf_linear_transform): sum_i pt_i * (key switch sums of rotation i + P c0(X^p_i)) in Q P ----------
// The hoisted inner product above, with the rotations never leaving the NTT domain over the extended basis: per key the sums
// over the digits as there; on the ordinary rows + P c0 gathered by the same pi (the fold moddown(s) + d = moddown(s + P d));
// both components times the key's encoded diagonal (NTT domain, Montgomery form, all rows) and added into ONE running pair
// shared by every key.  The first group adds the step-0 term pt0 * P (c0, c1) (ordinary rows, no key); later groups add the
// pair the previous group left in `s`.  The pair leaves in the format the sums' inverse pass reads (spl).
// fp64 class: the sums t R are balanced; the diagonal's Montgomery word m R goes through one REDC to the plain m, so that
// (t R) m is the Montgomery-form product; |running sums| <= (NR + 2) q, inside dp_reduce's 64 q.
struct LtArgs {
    HoistKeys hk;
    const i64 *pt[4];    // encoded diagonal of key i, [rows][N]
    const i64 *pt0;      // step-0 diagonal or nullptr (read by the first group only)
    const i64 *chat;     // P NTT(c0), P NTT(c1): [2][ell][N], Montgomery form, words below 2q
    int ell;             // ordinary rows (the first `ell` of the rows)
    int first;           // first group: `s` is not read
};

template <int NR, bool PLANES, bool DPL>
__global__ void __launch_bounds__(256) ks_inner_lt_kernel(const i64 *__restrict__ ext, LtArgs la, i64 part_stride, i64 comp_stride,
                                                          i64 row_off, i64 *__restrict__ s, int nparts, int rows, int logN, int spl,
                                                          const i64 *__restrict__ ql, const i64 *__restrict__ qh,
                                                          const i64 *__restrict__ kl, const i64 *__restrict__ kh) {
    constexpr int NA = NR ? NR : 1;
    const int r = blockIdx.y;
    const i64 N = (i64)1 << logN;
    const i64 j0 = (i64)blockIdx.x * 512 + threadIdx.x * 2;
    if (j0 >= N) return;
    const RowMod m = load_mod(ql, qh, kl, kh, r);
    const unsigned sh = 32u - (unsigned)logN, mask = (2u << logN) - 1u;
    const unsigned bj = (2u * (__builtin_bitreverse32((unsigned)j0) >> sh) + 1u);
    unsigned src[NA];
    bool sw[NA];
#pragma unroll
    for (int i = 0; i < NR; ++i) {
        const unsigned t = (bj * la.hk.p[i]) & mask;
        const unsigned mi = __builtin_bitreverse32((t - 1u) >> 1) >> sh;
        src[i] = mi & ~1u;
        sw[i] = (mi & 1u) != 0;
    }
    const i64 krow = (row_off + r) * N;
    const bool ord = r < la.ell;
    const i64 *c0row = la.chat + (i64)r * N, *c1row = c0row + (i64)la.ell * N;   // (read on ordinary rows only)
    i64 *srow0 = s + (i64)r * N, *srow1 = s + ((i64)rows + r) * N;
    if (m.q < SMALL_PRIME_LIMIT) {
        const RowDp d = make_dp(m);
        double acc[NA][2][2];
#pragma unroll
        for (int i = 0; i < NR; ++i) acc[i][0][0] = acc[i][0][1] = acc[i][1][0] = acc[i][1][1] = 0.0;
#pragma unroll KI_UNROLL
        for (int p = 0; p < nparts; ++p) {
            const i64 *er = ext + ((i64)p * rows + r) * N;
#pragma unroll
            for (int i = 0; i < NR; ++i) {
                double xa, xb;
                ld_pair_dp(er, (i64)src[i], N, DPL ? 1 : 0, xa, xb);
                const double x0 = sw[i] ? xb : xa, x1 = sw[i] ? xa : xb;
                const i64 *kr = la.hk.ksk[i] + krow + (i64)p * part_stride;
                double k0x, k0y, k1x, k1y;
                if (PLANES) {   // 16 + 8 bytes for both components (see lf_key_planes)
                    const lf_u4_t l = __builtin_nontemporal_load(reinterpret_cast<const lf_u4_t *>(reinterpret_cast<const unsigned *>(kr) + 2 * j0));
                    const lf_u2_t h = __builtin_nontemporal_load(reinterpret_cast<const lf_u2_t *>(reinterpret_cast<const unsigned *>(kr + comp_stride) + j0));
                    k0x = dp_from_planes(l.x, h.x & 0xffffu), k0y = dp_from_planes(l.y, h.x >> 16);
                    k1x = dp_from_planes(l.z, h.y & 0xffffu), k1y = dp_from_planes(l.w, h.y >> 16);
                } else {
                    const longlong2 k0 = ld_nt(kr + j0);
                    const longlong2 k1 = ld_nt(kr + j0 + comp_stride);
                    k0x = dp_from_word(k0.x), k0y = dp_from_word(k0.y), k1x = dp_from_word(k1.x), k1y = dp_from_word(k1.y);
                }
                acc[i][0][0] += dp_mulmod_bal(x0, k0x, d);
                acc[i][0][1] += dp_mulmod_bal(x1, k0y, d);
                acc[i][1][0] += dp_mulmod_bal(x0, k1x, d);
                acc[i][1][1] += dp_mulmod_bal(x1, k1y, d);
            }
        }
        double S[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
        if (!la.first) {   // the pair the previous group left (canonical words)
            ld_pair_dp(srow0, j0, N, spl, S[0][0], S[0][1]);
            ld_pair_dp(srow1, j0, N, spl, S[1][0], S[1][1]);
        } else if (la.pt0 != nullptr && ord) {
            const longlong2 w = ld_nt(la.pt0 + (i64)r * N + j0);
            const double wa = dp_from_word(mm62u((u64)w.x, 1ull, m.q, m.k)), wb = dp_from_word(mm62u((u64)w.y, 1ull, m.q, m.k));
            double a0, b0, a1, b1;
            ld_pair_dp(c0row, j0, N, 0, a0, b0);
            ld_pair_dp(c1row, j0, N, 0, a1, b1);
            S[0][0] = dp_mulmod_bal(a0, wa, d), S[0][1] = dp_mulmod_bal(b0, wb, d);
            S[1][0] = dp_mulmod_bal(a1, wa, d), S[1][1] = dp_mulmod_bal(b1, wb, d);
        }
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            if (ord) {
                double ca, cb;
                ld_pair_dp(c0row, (i64)src[i], N, 0, ca, cb);
                acc[i][0][0] += sw[i] ? cb : ca;
                acc[i][0][1] += sw[i] ? ca : cb;
            }
            const longlong2 w = ld_nt(la.pt[i] + (i64)r * N + j0);
            const double wa = dp_from_word(mm62u((u64)w.x, 1ull, m.q, m.k)), wb = dp_from_word(mm62u((u64)w.y, 1ull, m.q, m.k));
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                S[c][0] += dp_mulmod_bal(dp_reduce_bal(acc[i][c][0], d), wa, d);
                S[c][1] += dp_mulmod_bal(dp_reduce_bal(acc[i][c][1], d), wb, d);
            }
        }
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            longlong2 o;
            o.x = dp_to_word(dp_reduce(S[c][0], d.q, d.qinv));
            o.y = dp_to_word(dp_reduce(S[c][1], d.q, d.qinv));
            i64 *srow = c ? srow1 : srow0;
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
        i64 acc[NA][2][2];
#pragma unroll
        for (int i = 0; i < NR; ++i) acc[i][0][0] = acc[i][0][1] = acc[i][1][0] = acc[i][1][1] = 0;
        for (int p = 0; p < nparts; ++p) {
            const i64 *er = ext + ((i64)p * rows + r) * N;
#pragma unroll
            for (int i = 0; i < NR; ++i) {
                const longlong2 v = *reinterpret_cast<const longlong2 *>(er + src[i]);
                const u64 x0 = (u64)(sw[i] ? v.y : v.x), x1 = (u64)(sw[i] ? v.x : v.y);
                const i64 *kr = la.hk.ksk[i] + krow + (i64)p * part_stride + j0;
                const longlong2 k0 = ld_nt(kr);
                const longlong2 k1 = ld_nt(kr + comp_stride);
                acc[i][0][0] = csub(acc[i][0][0] + mm62u(x0, (u64)k0.x, m.q, m.k), m.q2);
                acc[i][0][1] = csub(acc[i][0][1] + mm62u(x1, (u64)k0.y, m.q, m.k), m.q2);
                acc[i][1][0] = csub(acc[i][1][0] + mm62u(x0, (u64)k1.x, m.q, m.k), m.q2);
                acc[i][1][1] = csub(acc[i][1][1] + mm62u(x1, (u64)k1.y, m.q, m.k), m.q2);
            }
        }
        i64 S[2][2] = {{0, 0}, {0, 0}};   // lazy words below 2q throughout
        if (!la.first) {
            const longlong2 a = *reinterpret_cast<const longlong2 *>(srow0 + j0), b = *reinterpret_cast<const longlong2 *>(srow1 + j0);
            S[0][0] = a.x, S[0][1] = a.y, S[1][0] = b.x, S[1][1] = b.y;
        } else if (la.pt0 != nullptr && ord) {
            const longlong2 w = ld_nt(la.pt0 + (i64)r * N + j0);
            const longlong2 a = *reinterpret_cast<const longlong2 *>(c0row + j0), b = *reinterpret_cast<const longlong2 *>(c1row + j0);
            S[0][0] = mm62u((u64)a.x, (u64)w.x, m.q, m.k), S[0][1] = mm62u((u64)a.y, (u64)w.y, m.q, m.k);
            S[1][0] = mm62u((u64)b.x, (u64)w.x, m.q, m.k), S[1][1] = mm62u((u64)b.y, (u64)w.y, m.q, m.k);
        }
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            if (ord) {
                const longlong2 v = *reinterpret_cast<const longlong2 *>(c0row + src[i]);
                acc[i][0][0] = csub(acc[i][0][0] + (sw[i] ? v.y : v.x), m.q2);
                acc[i][0][1] = csub(acc[i][0][1] + (sw[i] ? v.x : v.y), m.q2);
            }
            const longlong2 w = ld_nt(la.pt[i] + (i64)r * N + j0);
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                S[c][0] = csub(S[c][0] + mm62u((u64)acc[i][c][0], (u64)w.x, m.q, m.k), m.q2);
                S[c][1] = csub(S[c][1] + mm62u((u64)acc[i][c][1], (u64)w.y, m.q, m.k), m.q2);
            }
        }
        longlong2 o0, o1;
        o0.x = S[0][0], o0.y = S[0][1], o1.x = S[1][0], o1.y = S[1][1];
        *reinterpret_cast<longlong2 *>(srow0 + j0) = o0;
        *reinterpret_cast<longlong2 *>(srow1 + j0) = o1;
    }
}

// ---- K3 of a batched linear transform (lf_linear_transform_batch): ks_inner_lt_kernel for NCT ciphertexts under the SAME keys ---
// and diagonals.  The grid, the pi computation and the key / digit formats are ks_inner_lt_kernel's.  The kernel loops over the
// keys of its launch itself (la.nk <= LF_LTB_KEYS; keys, exponents and diagonals travel in the argument struct): per key and part
// the key's four words are loaded once and multiplied into NCT x 4 accumulators (ciphertext t's digits at ext + t * ext_stride,
// gathered by the key's pi); then the diagonal's two words are loaded once, REDCed once on the fp64-class rows, and multiplied
// into the NCT running pairs S, which stay in registers across the key loop and cross HBM once per launch: the first launch
// starts them from the step-0 term pt0 * P (c^0_t, c^1_t) (ordinary rows, no key; zero without pt0), later launches from the
// pair the previous launch left at s + t * sum_stride.  The pairs leave in the format the sums' inverse pass reads (spl).
// NK = keys whose digit loops run together.  pi differs from key to key, and the 512 words a block gathers are one contiguous
// segment of the row, ANOTHER one per key: two keys never share a digit word in registers, only in cache, which the key loop
// already arranges (every block of a row re-reads that row's digits once per key).  NK = 2 doubles the accumulators for
// nothing the cache does not give: NK = 1 is what runs.
// fp64 class: per key and ciphertext the sums are ks_inner_lt_kernel's (nparts balanced products + one word below 2q, reduced
// with dp_reduce_bal); a running pair takes per launch one start term — the step-0 balanced product, |.| <= q / 2, or the
// canonical word below q of the previous launch — and la.nk balanced products: |S| <= (LF_LTB_KEYS / 2 + 1) q = 5 q, inside
// dp_reduce's 64 q without a reduction inside the loop (it would be needed from 126 keys a launch on).
#define LF_LTB_KEYS 8   // keys per launch (backend.lt_batch_keys_per_launch): the pairs' trip is 2 x 2 rows N words per 8 keys' streams
static_assert(LF_LTB_KEYS / 2 + 1 < 64, "running pairs of ks_inner_ltb_kernel: (keys / 2 + 1) q must stay inside dp_reduce's 64 q");
struct LtbArgs {
    const i64 *ksk[LF_LTB_KEYS];   // key i, at its first part
    const i64 *pt[LF_LTB_KEYS];    // its encoded diagonal, [rows][N]
    unsigned p[LF_LTB_KEYS];       // its exponent (odd, < 2N)
    const i64 *pt0;                // step-0 diagonal or nullptr (read by the first launch only)
    const i64 *chat;               // ciphertext t at chat + t * chat_stride: P NTT(c0), P NTT(c1), [2][ell][N], words below 2q
    i64 chat_stride, ext_stride, sum_stride;   // words between the ciphertexts' c^, extended digits and running pairs
    int nk;                        // keys of this launch (0: the step-0 term alone)
    int ell;                       // ordinary rows (the first `ell` of the rows)
    int first;                     // first launch: `s` is not read
};

template <int NCT, int NK, bool PLANES, bool DPL>
__global__ void __launch_bounds__(256) ks_inner_ltb_kernel(const i64 *__restrict__ ext, LtbArgs la, i64 part_stride, i64 comp_stride,
                                                           i64 row_off, i64 *__restrict__ s, int nparts, int rows, int logN, int spl,
                                                           const i64 *__restrict__ ql, const i64 *__restrict__ qh,
                                                           const i64 *__restrict__ kl, const i64 *__restrict__ kh) {
    static_assert((NCT == 2 || NCT == 4) && (NK == 1 || NK == 2), "ks_inner_ltb_kernel: 2 or 4 ciphertexts, 1 or 2 keys together");
    const int r = blockIdx.y;
    const i64 N = (i64)1 << logN;
    const i64 j0 = (i64)blockIdx.x * 512 + threadIdx.x * 2;
    if (j0 >= N) return;
    const RowMod m = load_mod(ql, qh, kl, kh, r);
    const unsigned sh = 32u - (unsigned)logN, mask = (2u << logN) - 1u;
    const unsigned bj = (2u * (__builtin_bitreverse32((unsigned)j0) >> sh) + 1u);
    const i64 krow = (row_off + r) * N;
    const bool ord = r < la.ell;
    const i64 *c0row = la.chat + (i64)r * N, *c1row = c0row + (i64)la.ell * N;   // (read on ordinary rows only)
    i64 *srow0 = s + (i64)r * N, *srow1 = s + ((i64)rows + r) * N;
    constexpr int DIGITS_IN_FLIGHT = NCT * NK >= 4 ? 1 : KI_UNROLL;   // (NCT x NK digit pairs are in flight per key word already)
    if (m.q < SMALL_PRIME_LIMIT) {
        const RowDp d = make_dp(m);
        double S[NCT][2][2];
        if (!la.first) {   // the pairs the previous launch left (canonical words)
#pragma unroll
            for (int t = 0; t < NCT; ++t) {
                ld_pair_dp(srow0 + t * la.sum_stride, j0, N, spl, S[t][0][0], S[t][0][1]);
                ld_pair_dp(srow1 + t * la.sum_stride, j0, N, spl, S[t][1][0], S[t][1][1]);
            }
        } else if (la.pt0 != nullptr && ord) {
            const longlong2 w = ld_nt(la.pt0 + (i64)r * N + j0);
            const double wa = dp_from_word(mm62u((u64)w.x, 1ull, m.q, m.k)), wb = dp_from_word(mm62u((u64)w.y, 1ull, m.q, m.k));
#pragma unroll
            for (int t = 0; t < NCT; ++t) {
                double a0, b0, a1, b1;
                ld_pair_dp(c0row + t * la.chat_stride, j0, N, 0, a0, b0);
                ld_pair_dp(c1row + t * la.chat_stride, j0, N, 0, a1, b1);
                S[t][0][0] = dp_mulmod_bal(a0, wa, d), S[t][0][1] = dp_mulmod_bal(b0, wb, d);
                S[t][1][0] = dp_mulmod_bal(a1, wa, d), S[t][1][1] = dp_mulmod_bal(b1, wb, d);
            }
        } else {
#pragma unroll
            for (int t = 0; t < NCT; ++t) S[t][0][0] = S[t][0][1] = S[t][1][0] = S[t][1][1] = 0.0;
        }
        for (int k0 = 0; k0 < la.nk; k0 += NK) {
            i64 src[NK];
            bool sw[NK];
            double acc[NK][NCT][2][2];
#pragma unroll
            for (int i = 0; i < NK; ++i) {
                const int ki = k0 + i < la.nk ? k0 + i : k0;   // (an odd count: the last pair's second key repeats the first and is dropped)
                const unsigned t = (bj * la.p[ki]) & mask;
                const unsigned mi = __builtin_bitreverse32((t - 1u) >> 1) >> sh;
                src[i] = (i64)(mi & ~1u);
                sw[i] = (mi & 1u) != 0;
#pragma unroll
                for (int t2 = 0; t2 < NCT; ++t2) acc[i][t2][0][0] = acc[i][t2][0][1] = acc[i][t2][1][0] = acc[i][t2][1][1] = 0.0;
            }
#pragma unroll DIGITS_IN_FLIGHT
            for (int p = 0; p < nparts; ++p) {
                const i64 *er = ext + ((i64)p * rows + r) * N;
#pragma unroll
                for (int i = 0; i < NK; ++i) {
                    if (NK > 1 && k0 + i >= la.nk) break;
                    const i64 *kr = la.ksk[k0 + i] + krow + (i64)p * part_stride;
                    double k0x, k0y, k1x, k1y;
                    if (PLANES) {   // 16 + 8 bytes for both components (see lf_key_planes)
                        const lf_u4_t l = __builtin_nontemporal_load(reinterpret_cast<const lf_u4_t *>(reinterpret_cast<const unsigned *>(kr) + 2 * j0));
                        const lf_u2_t h = __builtin_nontemporal_load(reinterpret_cast<const lf_u2_t *>(reinterpret_cast<const unsigned *>(kr + comp_stride) + j0));
                        k0x = dp_from_planes(l.x, h.x & 0xffffu), k0y = dp_from_planes(l.y, h.x >> 16);
                        k1x = dp_from_planes(l.z, h.y & 0xffffu), k1y = dp_from_planes(l.w, h.y >> 16);
                    } else {
                        const longlong2 w0 = ld_nt(kr + j0);
                        const longlong2 w1 = ld_nt(kr + j0 + comp_stride);
                        k0x = dp_from_word(w0.x), k0y = dp_from_word(w0.y), k1x = dp_from_word(w1.x), k1y = dp_from_word(w1.y);
                    }
#pragma unroll
                    for (int t = 0; t < NCT; ++t) {
                        double xa, xb;
                        ld_pair_dp(er + t * la.ext_stride, src[i], N, DPL ? 1 : 0, xa, xb);
                        const double x0 = sw[i] ? xb : xa, x1 = sw[i] ? xa : xb;
                        acc[i][t][0][0] += dp_mulmod_bal(x0, k0x, d);
                        acc[i][t][0][1] += dp_mulmod_bal(x1, k0y, d);
                        acc[i][t][1][0] += dp_mulmod_bal(x0, k1x, d);
                        acc[i][t][1][1] += dp_mulmod_bal(x1, k1y, d);
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < NK; ++i) {
                if (NK > 1 && k0 + i >= la.nk) break;
                const longlong2 w = ld_nt(la.pt[k0 + i] + (i64)r * N + j0);
                const double wa = dp_from_word(mm62u((u64)w.x, 1ull, m.q, m.k)), wb = dp_from_word(mm62u((u64)w.y, 1ull, m.q, m.k));
#pragma unroll
                for (int t = 0; t < NCT; ++t) {
                    if (ord) {
                        double ca, cb;
                        ld_pair_dp(c0row + t * la.chat_stride, src[i], N, 0, ca, cb);
                        acc[i][t][0][0] += sw[i] ? cb : ca;
                        acc[i][t][0][1] += sw[i] ? ca : cb;
                    }
#pragma unroll
                    for (int c = 0; c < 2; ++c) {
                        S[t][c][0] += dp_mulmod_bal(dp_reduce_bal(acc[i][t][c][0], d), wa, d);
                        S[t][c][1] += dp_mulmod_bal(dp_reduce_bal(acc[i][t][c][1], d), wb, d);
                    }
                }
            }
        }
#pragma unroll
        for (int t = 0; t < NCT; ++t)
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                longlong2 o;   // |S| <= (LF_LTB_KEYS / 2 + 1) q, inside dp_reduce's 64 q
                o.x = dp_to_word(dp_reduce(S[t][c][0], d.q, d.qinv));
                o.y = dp_to_word(dp_reduce(S[t][c][1], d.q, d.qinv));
                i64 *srow = (c ? srow1 : srow0) + t * la.sum_stride;
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
        i64 S[NCT][2][2];   // lazy words below 2q throughout
        if (!la.first) {
#pragma unroll
            for (int t = 0; t < NCT; ++t) {
                const longlong2 a = *reinterpret_cast<const longlong2 *>(srow0 + t * la.sum_stride + j0);
                const longlong2 b = *reinterpret_cast<const longlong2 *>(srow1 + t * la.sum_stride + j0);
                S[t][0][0] = a.x, S[t][0][1] = a.y, S[t][1][0] = b.x, S[t][1][1] = b.y;
            }
        } else if (la.pt0 != nullptr && ord) {
            const longlong2 w = ld_nt(la.pt0 + (i64)r * N + j0);
#pragma unroll
            for (int t = 0; t < NCT; ++t) {
                const longlong2 a = *reinterpret_cast<const longlong2 *>(c0row + t * la.chat_stride + j0);
                const longlong2 b = *reinterpret_cast<const longlong2 *>(c1row + t * la.chat_stride + j0);
                S[t][0][0] = mm62u((u64)a.x, (u64)w.x, m.q, m.k), S[t][0][1] = mm62u((u64)a.y, (u64)w.y, m.q, m.k);
                S[t][1][0] = mm62u((u64)b.x, (u64)w.x, m.q, m.k), S[t][1][1] = mm62u((u64)b.y, (u64)w.y, m.q, m.k);
            }
        } else {
#pragma unroll
            for (int t = 0; t < NCT; ++t) S[t][0][0] = S[t][0][1] = S[t][1][0] = S[t][1][1] = 0;
        }
        for (int k0 = 0; k0 < la.nk; k0 += NK) {
            i64 src[NK];
            bool sw[NK];
            i64 acc[NK][NCT][2][2];
#pragma unroll
            for (int i = 0; i < NK; ++i) {
                const int ki = k0 + i < la.nk ? k0 + i : k0;
                const unsigned t = (bj * la.p[ki]) & mask;
                const unsigned mi = __builtin_bitreverse32((t - 1u) >> 1) >> sh;
                src[i] = (i64)(mi & ~1u);
                sw[i] = (mi & 1u) != 0;
#pragma unroll
                for (int t2 = 0; t2 < NCT; ++t2) acc[i][t2][0][0] = acc[i][t2][0][1] = acc[i][t2][1][0] = acc[i][t2][1][1] = 0;
            }
            for (int p = 0; p < nparts; ++p) {
                const i64 *er = ext + ((i64)p * rows + r) * N;
#pragma unroll
                for (int i = 0; i < NK; ++i) {
                    if (NK > 1 && k0 + i >= la.nk) break;
                    const i64 *kr = la.ksk[k0 + i] + krow + (i64)p * part_stride + j0;
                    const longlong2 w0 = ld_nt(kr);
                    const longlong2 w1 = ld_nt(kr + comp_stride);
#pragma unroll
                    for (int t = 0; t < NCT; ++t) {
                        const longlong2 v = *reinterpret_cast<const longlong2 *>(er + t * la.ext_stride + src[i]);
                        const u64 x0 = (u64)(sw[i] ? v.y : v.x), x1 = (u64)(sw[i] ? v.x : v.y);
                        acc[i][t][0][0] = csub(acc[i][t][0][0] + mm62u(x0, (u64)w0.x, m.q, m.k), m.q2);
                        acc[i][t][0][1] = csub(acc[i][t][0][1] + mm62u(x1, (u64)w0.y, m.q, m.k), m.q2);
                        acc[i][t][1][0] = csub(acc[i][t][1][0] + mm62u(x0, (u64)w1.x, m.q, m.k), m.q2);
                        acc[i][t][1][1] = csub(acc[i][t][1][1] + mm62u(x1, (u64)w1.y, m.q, m.k), m.q2);
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < NK; ++i) {
                if (NK > 1 && k0 + i >= la.nk) break;
                const longlong2 w = ld_nt(la.pt[k0 + i] + (i64)r * N + j0);
#pragma unroll
                for (int t = 0; t < NCT; ++t) {
                    if (ord) {
                        const longlong2 v = *reinterpret_cast<const longlong2 *>(c0row + t * la.chat_stride + src[i]);
                        acc[i][t][0][0] = csub(acc[i][t][0][0] + (sw[i] ? v.y : v.x), m.q2);
                        acc[i][t][0][1] = csub(acc[i][t][0][1] + (sw[i] ? v.x : v.y), m.q2);
                    }
#pragma unroll
                    for (int c = 0; c < 2; ++c) {
                        S[t][c][0] = csub(S[t][c][0] + mm62u((u64)acc[i][t][c][0], (u64)w.x, m.q, m.k), m.q2);
                        S[t][c][1] = csub(S[t][c][1] + mm62u((u64)acc[i][t][c][1], (u64)w.y, m.q, m.k), m.q2);
                    }
                }
            }
        }
#pragma unroll
        for (int t = 0; t < NCT; ++t) {
            longlong2 o0, o1;
            o0.x = S[t][0][0], o0.y = S[t][0][1], o1.x = S[t][1][0], o1.y = S[t][1][1];
            *reinterpret_cast<longlong2 *>(srow0 + t * la.sum_stride + j0) = o0;
            *reinterpret_cast<longlong2 *>(srow1 + t * la.sum_stride + j0) = o1;
        }
    }
}

// ---- K3 of a rotation sum (lf_rotate_sum): sum_i (key switch sums of rotation i + P c0(X^p_i)) [+ P (c0, c1)] in Q P ------------
// ks_inner_lt_kernel without the diagonals: the same grid, pi computation and key / digit formats, and ONE accumulator pair per
// thread for the whole group — the digits x key products of all NR keys go into the same acc[2][2]; on the ordinary rows c^0
// gathered by each pi_{p_i} joins component 0.  The first group adds the self term P (c^0, c^1), ungathered, on the ordinary
// rows when asked to (self); later groups add the pair the previous group left in `s`.  The pair leaves in the format the sums'
// inverse pass reads (spl).  Only residues reach the result, so the additions come in the order that suits the loads.
// fp64 class: the accumulator takes NR nparts balanced products (|.| <= q / 2 each), NR gathered words of c^0 and one word of
// c^ (all below 2q) or of the previous pair (canonical, below q): NR nparts + NR + 2 terms, |acc| <= (NR nparts / 2 + 2 NR + 2) q.
// With NR = 4 that passes dp_reduce's 64 q from nparts = 27 on, and LF_FP64_MAX_DIGITS allows 119: (238 + 10) q < 2^8 q < 2^49.
// So the sum is first brought to a balanced residue by dp_reduce_bal (exact for |x| < 2^52; every partial sum is an integer
// below 2^49, exact in fp64) and that residue, |.| <= q / 2, goes through dp_reduce: two more fp64 instructions per word, once.
struct RsumArgs {
    HoistKeys hk;
    const i64 *chat;     // P NTT(c0), P NTT(c1): [2][ell][N], Montgomery form, words below 2q (c1 is read for the self term only)
    int ell;             // ordinary rows (the first `ell` of the rows)
    int first;           // first group: `s` is not read
    int self;            // the first group adds P (c^0, c^1) on the ordinary rows
};

template <int NR, bool PLANES, bool DPL>
__global__ void __launch_bounds__(256) ks_inner_rsum_kernel(const i64 *__restrict__ ext, RsumArgs ra, i64 part_stride, i64 comp_stride,
                                                            i64 row_off, i64 *__restrict__ s, int nparts, int rows, int logN, int spl,
                                                            const i64 *__restrict__ ql, const i64 *__restrict__ qh,
                                                            const i64 *__restrict__ kl, const i64 *__restrict__ kh) {
    constexpr int NA = NR ? NR : 1;
    const int r = blockIdx.y;
    const i64 N = (i64)1 << logN;
    const i64 j0 = (i64)blockIdx.x * 512 + threadIdx.x * 2;
    if (j0 >= N) return;
    const RowMod m = load_mod(ql, qh, kl, kh, r);
    const unsigned sh = 32u - (unsigned)logN, mask = (2u << logN) - 1u;
    const unsigned bj = (2u * (__builtin_bitreverse32((unsigned)j0) >> sh) + 1u);
    unsigned src[NA];
    bool sw[NA];
#pragma unroll
    for (int i = 0; i < NR; ++i) {
        const unsigned t = (bj * ra.hk.p[i]) & mask;
        const unsigned mi = __builtin_bitreverse32((t - 1u) >> 1) >> sh;
        src[i] = mi & ~1u;
        sw[i] = (mi & 1u) != 0;
    }
    const i64 krow = (row_off + r) * N;
    const bool ord = r < ra.ell;
    const i64 *c0row = ra.chat + (i64)r * N, *c1row = c0row + (i64)ra.ell * N;   // (read on ordinary rows only)
    i64 *srow0 = s + (i64)r * N, *srow1 = s + ((i64)rows + r) * N;
    if (m.q < SMALL_PRIME_LIMIT) {
        const RowDp d = make_dp(m);
        double acc[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
#pragma unroll KI_UNROLL
        for (int p = 0; p < nparts; ++p) {
            const i64 *er = ext + ((i64)p * rows + r) * N;
#pragma unroll
            for (int i = 0; i < NR; ++i) {
                double xa, xb;
                ld_pair_dp(er, (i64)src[i], N, DPL ? 1 : 0, xa, xb);
                const double x0 = sw[i] ? xb : xa, x1 = sw[i] ? xa : xb;
                const i64 *kr = ra.hk.ksk[i] + krow + (i64)p * part_stride;
                double k0x, k0y, k1x, k1y;
                if (PLANES) {   // 16 + 8 bytes for both components (see lf_key_planes)
                    const lf_u4_t l = __builtin_nontemporal_load(reinterpret_cast<const lf_u4_t *>(reinterpret_cast<const unsigned *>(kr) + 2 * j0));
                    const lf_u2_t h = __builtin_nontemporal_load(reinterpret_cast<const lf_u2_t *>(reinterpret_cast<const unsigned *>(kr + comp_stride) + j0));
                    k0x = dp_from_planes(l.x, h.x & 0xffffu), k0y = dp_from_planes(l.y, h.x >> 16);
                    k1x = dp_from_planes(l.z, h.y & 0xffffu), k1y = dp_from_planes(l.w, h.y >> 16);
                } else {
                    const longlong2 k0 = ld_nt(kr + j0);
                    const longlong2 k1 = ld_nt(kr + j0 + comp_stride);
                    k0x = dp_from_word(k0.x), k0y = dp_from_word(k0.y), k1x = dp_from_word(k1.x), k1y = dp_from_word(k1.y);
                }
                acc[0][0] += dp_mulmod_bal(x0, k0x, d);
                acc[0][1] += dp_mulmod_bal(x1, k0y, d);
                acc[1][0] += dp_mulmod_bal(x0, k1x, d);
                acc[1][1] += dp_mulmod_bal(x1, k1y, d);
            }
        }
        if (!ra.first) {   // the pair the previous group left (canonical words)
            double a0, b0, a1, b1;
            ld_pair_dp(srow0, j0, N, spl, a0, b0);
            ld_pair_dp(srow1, j0, N, spl, a1, b1);
            acc[0][0] += a0, acc[0][1] += b0, acc[1][0] += a1, acc[1][1] += b1;
        } else if (ra.self && ord) {
            double a0, b0, a1, b1;
            ld_pair_dp(c0row, j0, N, 0, a0, b0);
            ld_pair_dp(c1row, j0, N, 0, a1, b1);
            acc[0][0] += a0, acc[0][1] += b0, acc[1][0] += a1, acc[1][1] += b1;
        }
        if (ord) {
#pragma unroll
            for (int i = 0; i < NR; ++i) {
                double ca, cb;
                ld_pair_dp(c0row, (i64)src[i], N, 0, ca, cb);
                acc[0][0] += sw[i] ? cb : ca;
                acc[0][1] += sw[i] ? ca : cb;
            }
        }
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            longlong2 o;
            o.x = dp_to_word(dp_reduce(dp_reduce_bal(acc[c][0], d), d.q, d.qinv));
            o.y = dp_to_word(dp_reduce(dp_reduce_bal(acc[c][1], d), d.q, d.qinv));
            i64 *srow = c ? srow1 : srow0;
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
        i64 acc[2][2] = {{0, 0}, {0, 0}};   // lazy words below 2q throughout
        for (int p = 0; p < nparts; ++p) {
            const i64 *er = ext + ((i64)p * rows + r) * N;
#pragma unroll
            for (int i = 0; i < NR; ++i) {
                const longlong2 v = *reinterpret_cast<const longlong2 *>(er + src[i]);
                const u64 x0 = (u64)(sw[i] ? v.y : v.x), x1 = (u64)(sw[i] ? v.x : v.y);
                const i64 *kr = ra.hk.ksk[i] + krow + (i64)p * part_stride + j0;
                const longlong2 k0 = ld_nt(kr);
                const longlong2 k1 = ld_nt(kr + comp_stride);
                acc[0][0] = csub(acc[0][0] + mm62u(x0, (u64)k0.x, m.q, m.k), m.q2);
                acc[0][1] = csub(acc[0][1] + mm62u(x1, (u64)k0.y, m.q, m.k), m.q2);
                acc[1][0] = csub(acc[1][0] + mm62u(x0, (u64)k1.x, m.q, m.k), m.q2);
                acc[1][1] = csub(acc[1][1] + mm62u(x1, (u64)k1.y, m.q, m.k), m.q2);
            }
        }
        if (!ra.first || (ra.self && ord)) {   // the previous group's pair, or the self term (both below 2q)
            const i64 *a = ra.first ? c0row : srow0, *b = ra.first ? c1row : srow1;
            const longlong2 va = *reinterpret_cast<const longlong2 *>(a + j0), vb = *reinterpret_cast<const longlong2 *>(b + j0);
            acc[0][0] = csub(acc[0][0] + va.x, m.q2), acc[0][1] = csub(acc[0][1] + va.y, m.q2);
            acc[1][0] = csub(acc[1][0] + vb.x, m.q2), acc[1][1] = csub(acc[1][1] + vb.y, m.q2);
        }
        if (ord) {
#pragma unroll
            for (int i = 0; i < NR; ++i) {
                const longlong2 v = *reinterpret_cast<const longlong2 *>(c0row + src[i]);
                acc[0][0] = csub(acc[0][0] + (sw[i] ? v.y : v.x), m.q2);
                acc[0][1] = csub(acc[0][1] + (sw[i] ? v.x : v.y), m.q2);
            }
        }
        longlong2 o0, o1;
        o0.x = acc[0][0], o0.y = acc[0][1], o1.x = acc[1][0], o1.y = acc[1][1];
        *reinterpret_cast<longlong2 *>(srow0 + j0) = o0;
        *reinterpret_cast<longlong2 *>(srow1 + j0) = o1;
    }
}

// ---- K3 of a batched rotation sum (lf_rotate_sum_batch): ks_inner_rsum_kernel for NCT ciphertexts under the SAME keys -----------
// The grid, the pi computation and the key / digit formats are ks_inner_rsum_kernel's.  The kernel loops over the keys of its
// launch itself (ra.nk <= LF_RSB_KEYS; keys and exponents travel in the argument struct, as in LtbArgs): per key and part the
// key's four words are loaded once and multiplied into the NCT accumulator pairs acc[NCT][2][2] (ciphertext t's digits at
// ext + t * ext_stride, gathered by that key's pi); on the ordinary rows c^0 of ciphertext t gathered by pi joins component 0.
// ONE accumulator set per ciphertext serves ALL keys of the launch — ks_inner_rsum_kernel's single pair, times NCT — so there is
// no running pair beside the accumulators (half the live doubles of ks_inner_ltb_kernel).  The first launch starts the pairs from
// the self term P (c^0_t, c^1_t), ungathered, on the ordinary rows when asked to (self), else from zero; later launches start
// from the pair the previous launch left at s + t * sum_stride.  The pairs leave in the format the sums' inverse pass reads (spl).
// Only residues reach the result, so the additions come in the order that suits the loads.
// fp64 class: an accumulator takes nk nparts balanced products (|.| <= q / 2 each), nk gathered words of c^0 and one start word
// (all below 2q): |acc| <= (nk nparts / 2 + 2 nk + 2) q.  With nk = LF_RSB_KEYS = 8 and nparts = LF_FP64_MAX_DIGITS = 119 that is
// 494 q < 2^9 q < 2^50 for q < 2^41: every partial sum is an integer below 2^52, exact in fp64, and the ONE dp_reduce_bal (exact
// for |x| < 2^52) brings it to a balanced residue for dp_reduce, as in ks_inner_rsum_kernel.
#define LF_RSB_KEYS 8   // keys per launch (backend.rsum_batch_keys_per_launch): the pairs' trip is 2 x 2 rows N words per 8 keys' streams
static_assert(((unsigned long long)(LF_RSB_KEYS * LF_FP64_MAX_DIGITS / 2 + 2 * LF_RSB_KEYS + 2) << 41) < (1ull << 52),
              "accumulators of ks_inner_rsumb_kernel: (keys nparts / 2 + 2 keys + 2) q must stay below dp_reduce_bal's 2^52");
struct RsbArgs {
    const i64 *ksk[LF_RSB_KEYS];   // key i, at its first part
    unsigned p[LF_RSB_KEYS];       // its exponent (odd, < 2N)
    const i64 *chat;               // ciphertext t at chat + t * chat_stride: P NTT(c0), P NTT(c1), [2][ell][N], words below 2q
    i64 chat_stride, ext_stride, sum_stride;   // words between the ciphertexts' c^, extended digits and pairs of sums
    int nk;                        // keys of this launch (0: the self term alone)
    int ell;                       // ordinary rows (the first `ell` of the rows)
    int first;                     // first launch: `s` is not read
    int self;                      // the first launch starts from P (c^0_t, c^1_t) on the ordinary rows
};

template <int NCT, bool PLANES, bool DPL>
__global__ void __launch_bounds__(256) ks_inner_rsumb_kernel(const i64 *__restrict__ ext, RsbArgs ra, i64 part_stride, i64 comp_stride,
                                                             i64 row_off, i64 *__restrict__ s, int nparts, int rows, int logN, int spl,
                                                             const i64 *__restrict__ ql, const i64 *__restrict__ qh,
                                                             const i64 *__restrict__ kl, const i64 *__restrict__ kh) {
    static_assert(NCT == 2 || NCT == 4, "ks_inner_rsumb_kernel: 2 or 4 ciphertexts");
    const int r = blockIdx.y;
    const i64 N = (i64)1 << logN;
    const i64 j0 = (i64)blockIdx.x * 512 + threadIdx.x * 2;
    if (j0 >= N) return;
    const RowMod m = load_mod(ql, qh, kl, kh, r);
    const unsigned sh = 32u - (unsigned)logN, mask = (2u << logN) - 1u;
    const unsigned bj = (2u * (__builtin_bitreverse32((unsigned)j0) >> sh) + 1u);
    const i64 krow = (row_off + r) * N;
    const bool ord = r < ra.ell;
    const i64 *c0row = ra.chat + (i64)r * N, *c1row = c0row + (i64)ra.ell * N;   // (read on ordinary rows only)
    i64 *srow0 = s + (i64)r * N, *srow1 = s + ((i64)rows + r) * N;
    constexpr int DIGITS_IN_FLIGHT = NCT >= 4 ? 1 : KI_UNROLL;   // (NCT digit pairs are in flight per key word already)
    if (m.q < SMALL_PRIME_LIMIT) {
        const RowDp d = make_dp(m);
        double acc[NCT][2][2];
        if (!ra.first) {   // the pairs the previous launch left (canonical words)
#pragma unroll
            for (int t = 0; t < NCT; ++t) {
                ld_pair_dp(srow0 + t * ra.sum_stride, j0, N, spl, acc[t][0][0], acc[t][0][1]);
                ld_pair_dp(srow1 + t * ra.sum_stride, j0, N, spl, acc[t][1][0], acc[t][1][1]);
            }
        } else if (ra.self && ord) {
#pragma unroll
            for (int t = 0; t < NCT; ++t) {
                ld_pair_dp(c0row + t * ra.chat_stride, j0, N, 0, acc[t][0][0], acc[t][0][1]);
                ld_pair_dp(c1row + t * ra.chat_stride, j0, N, 0, acc[t][1][0], acc[t][1][1]);
            }
        } else {
#pragma unroll
            for (int t = 0; t < NCT; ++t) acc[t][0][0] = acc[t][0][1] = acc[t][1][0] = acc[t][1][1] = 0.0;
        }
        for (int k = 0; k < ra.nk; ++k) {
            const unsigned tk = (bj * ra.p[k]) & mask;
            const unsigned mi = __builtin_bitreverse32((tk - 1u) >> 1) >> sh;
            const i64 src = (i64)(mi & ~1u);
            const bool sw = (mi & 1u) != 0;
            const i64 *kbase = ra.ksk[k] + krow;
#pragma unroll DIGITS_IN_FLIGHT
            for (int p = 0; p < nparts; ++p) {
                const i64 *er = ext + ((i64)p * rows + r) * N;
                const i64 *kr = kbase + (i64)p * part_stride;
                double k0x, k0y, k1x, k1y;
                if (PLANES) {   // 16 + 8 bytes for both components (see lf_key_planes)
                    const lf_u4_t l = __builtin_nontemporal_load(reinterpret_cast<const lf_u4_t *>(reinterpret_cast<const unsigned *>(kr) + 2 * j0));
                    const lf_u2_t h = __builtin_nontemporal_load(reinterpret_cast<const lf_u2_t *>(reinterpret_cast<const unsigned *>(kr + comp_stride) + j0));
                    k0x = dp_from_planes(l.x, h.x & 0xffffu), k0y = dp_from_planes(l.y, h.x >> 16);
                    k1x = dp_from_planes(l.z, h.y & 0xffffu), k1y = dp_from_planes(l.w, h.y >> 16);
                } else {
                    const longlong2 w0 = ld_nt(kr + j0);
                    const longlong2 w1 = ld_nt(kr + j0 + comp_stride);
                    k0x = dp_from_word(w0.x), k0y = dp_from_word(w0.y), k1x = dp_from_word(w1.x), k1y = dp_from_word(w1.y);
                }
#pragma unroll
                for (int t = 0; t < NCT; ++t) {
                    double xa, xb;
                    ld_pair_dp(er + t * ra.ext_stride, src, N, DPL ? 1 : 0, xa, xb);
                    const double x0 = sw ? xb : xa, x1 = sw ? xa : xb;
                    acc[t][0][0] += dp_mulmod_bal(x0, k0x, d);
                    acc[t][0][1] += dp_mulmod_bal(x1, k0y, d);
                    acc[t][1][0] += dp_mulmod_bal(x0, k1x, d);
                    acc[t][1][1] += dp_mulmod_bal(x1, k1y, d);
                }
            }
            if (ord) {
#pragma unroll
                for (int t = 0; t < NCT; ++t) {
                    double ca, cb;
                    ld_pair_dp(c0row + t * ra.chat_stride, src, N, 0, ca, cb);
                    acc[t][0][0] += sw ? cb : ca;
                    acc[t][0][1] += sw ? ca : cb;
                }
            }
        }
#pragma unroll
        for (int t = 0; t < NCT; ++t)
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                longlong2 o;   // |acc| <= (LF_RSB_KEYS nparts / 2 + 2 LF_RSB_KEYS + 2) q < 2^52: dp_reduce_bal first
                o.x = dp_to_word(dp_reduce(dp_reduce_bal(acc[t][c][0], d), d.q, d.qinv));
                o.y = dp_to_word(dp_reduce(dp_reduce_bal(acc[t][c][1], d), d.q, d.qinv));
                i64 *srow = (c ? srow1 : srow0) + t * ra.sum_stride;
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
        i64 acc[NCT][2][2];   // lazy words below 2q throughout
        if (!ra.first || (ra.self && ord)) {   // the previous launch's pairs, or the self term (both below 2q)
            const i64 *a = ra.first ? c0row : srow0, *b = ra.first ? c1row : srow1;
            const i64 stride = ra.first ? ra.chat_stride : ra.sum_stride;
#pragma unroll
            for (int t = 0; t < NCT; ++t) {
                const longlong2 va = *reinterpret_cast<const longlong2 *>(a + t * stride + j0);
                const longlong2 vb = *reinterpret_cast<const longlong2 *>(b + t * stride + j0);
                acc[t][0][0] = va.x, acc[t][0][1] = va.y, acc[t][1][0] = vb.x, acc[t][1][1] = vb.y;
            }
        } else {
#pragma unroll
            for (int t = 0; t < NCT; ++t) acc[t][0][0] = acc[t][0][1] = acc[t][1][0] = acc[t][1][1] = 0;
        }
        for (int k = 0; k < ra.nk; ++k) {
            const unsigned tk = (bj * ra.p[k]) & mask;
            const unsigned mi = __builtin_bitreverse32((tk - 1u) >> 1) >> sh;
            const i64 src = (i64)(mi & ~1u);
            const bool sw = (mi & 1u) != 0;
            const i64 *kbase = ra.ksk[k] + krow + j0;
            for (int p = 0; p < nparts; ++p) {
                const i64 *er = ext + ((i64)p * rows + r) * N;
                const i64 *kr = kbase + (i64)p * part_stride;
                const longlong2 w0 = ld_nt(kr);
                const longlong2 w1 = ld_nt(kr + comp_stride);
#pragma unroll
                for (int t = 0; t < NCT; ++t) {
                    const longlong2 v = *reinterpret_cast<const longlong2 *>(er + t * ra.ext_stride + src);
                    const u64 x0 = (u64)(sw ? v.y : v.x), x1 = (u64)(sw ? v.x : v.y);
                    acc[t][0][0] = csub(acc[t][0][0] + mm62u(x0, (u64)w0.x, m.q, m.k), m.q2);
                    acc[t][0][1] = csub(acc[t][0][1] + mm62u(x1, (u64)w0.y, m.q, m.k), m.q2);
                    acc[t][1][0] = csub(acc[t][1][0] + mm62u(x0, (u64)w1.x, m.q, m.k), m.q2);
                    acc[t][1][1] = csub(acc[t][1][1] + mm62u(x1, (u64)w1.y, m.q, m.k), m.q2);
                }
            }
            if (ord) {
#pragma unroll
                for (int t = 0; t < NCT; ++t) {
                    const longlong2 v = *reinterpret_cast<const longlong2 *>(c0row + t * ra.chat_stride + src);
                    acc[t][0][0] = csub(acc[t][0][0] + (sw ? v.y : v.x), m.q2);
                    acc[t][0][1] = csub(acc[t][0][1] + (sw ? v.x : v.y), m.q2);
                }
            }
        }
#pragma unroll
        for (int t = 0; t < NCT; ++t) {
            longlong2 o0, o1;
            o0.x = acc[t][0][0], o0.y = acc[t][0][1], o1.x = acc[t][1][0], o1.y = acc[t][1][1];
            *reinterpret_cast<longlong2 *>(srow0 + t * ra.sum_stride + j0) = o0;
            *reinterpret_cast<longlong2 *>(srow1 + t * ra.sum_stride + j0) = o1;
        }
    }
}

// ---- baby-step / giant-step linear transform (lf_linear_transform_bsgs): y = sum_g rot(sum_b pt_{g,b} * rot(x, b), g) ------------
// Three launches on the grid, the pi computation and the key / digit formats of the two kernels above, under names of their own:
//   ks_inner_baby_kernel     per group of 4 / 2 / 1 baby keys the gathered sums over the digits, + P c0 gathered on the ordinary
//                            rows, written out as one pair PER KEY (the flat kernel's t_c, kept instead of multiplied and summed);
//   lt_diag_products_kernel  S^g_c = sum_b pt_{g,b} * u^b_c for up to 4 giant steps per launch, pure streaming;
//   ks_inner_giant_kernel    one key, the digits of the giant step's polynomial gathered by pi_g, + S^g_0 gathered on ALL rows
//                            (it lives in Q P and never comes down), read - add - write into the accumulator pair.
// Every buffer between them holds raw 8-byte words whose residues are the Montgomery-form words of the orchestrated steps:
// canonical from the fp64-class rows (the balanced sums reduced once), lazy below 2q from the integer rows.  Only residues
// reach the result: each pair next meets a product, a sum, or the exact inverse transform.

// the gathered sums over the digits of NR keys for the thread's pair (j0, j0 + 1) of row r: fp64 class (balanced sums) ...
template <int NR, bool PLANES, bool DPL>
static __device__ __forceinline__ void gathered_sums_dp(const i64 *__restrict__ ext, const HoistKeys &hk, const unsigned (&src)[NR],
                                                        const bool (&sw)[NR], i64 part_stride, i64 comp_stride, i64 krow, i64 j0,
                                                        int nparts, int rows, int r, i64 N, const RowDp &d, double (&acc)[NR][2][2]) {
#pragma unroll
    for (int i = 0; i < NR; ++i) acc[i][0][0] = acc[i][0][1] = acc[i][1][0] = acc[i][1][1] = 0.0;
#pragma unroll KI_UNROLL
    for (int p = 0; p < nparts; ++p) {
        const i64 *er = ext + ((i64)p * rows + r) * N;
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            double xa, xb;
            ld_pair_dp(er, (i64)src[i], N, DPL ? 1 : 0, xa, xb);
            const double x0 = sw[i] ? xb : xa, x1 = sw[i] ? xa : xb;
            const i64 *kr = hk.ksk[i] + krow + (i64)p * part_stride;
            double k0x, k0y, k1x, k1y;
            if (PLANES) {   // 16 + 8 bytes for both components (see lf_key_planes)
                const lf_u4_t l = __builtin_nontemporal_load(reinterpret_cast<const lf_u4_t *>(reinterpret_cast<const unsigned *>(kr) + 2 * j0));
                const lf_u2_t h = __builtin_nontemporal_load(reinterpret_cast<const lf_u2_t *>(reinterpret_cast<const unsigned *>(kr + comp_stride) + j0));
                k0x = dp_from_planes(l.x, h.x & 0xffffu), k0y = dp_from_planes(l.y, h.x >> 16);
                k1x = dp_from_planes(l.z, h.y & 0xffffu), k1y = dp_from_planes(l.w, h.y >> 16);
            } else {
                const longlong2 k0 = ld_nt(kr + j0);
                const longlong2 k1 = ld_nt(kr + j0 + comp_stride);
                k0x = dp_from_word(k0.x), k0y = dp_from_word(k0.y), k1x = dp_from_word(k1.x), k1y = dp_from_word(k1.y);
            }
            acc[i][0][0] += dp_mulmod_bal(x0, k0x, d);
            acc[i][0][1] += dp_mulmod_bal(x1, k0y, d);
            acc[i][1][0] += dp_mulmod_bal(x0, k1x, d);
            acc[i][1][1] += dp_mulmod_bal(x1, k1y, d);
        }
    }
}

// ... and integer class (lazy words below 2q)
template <int NR>
static __device__ __forceinline__ void gathered_sums_int(const i64 *__restrict__ ext, const HoistKeys &hk, const unsigned (&src)[NR],
                                                         const bool (&sw)[NR], i64 part_stride, i64 comp_stride, i64 krow, i64 j0,
                                                         int nparts, int rows, int r, i64 N, const RowMod &m, i64 (&acc)[NR][2][2]) {
#pragma unroll
    for (int i = 0; i < NR; ++i) acc[i][0][0] = acc[i][0][1] = acc[i][1][0] = acc[i][1][1] = 0;
    for (int p = 0; p < nparts; ++p) {
        const i64 *er = ext + ((i64)p * rows + r) * N;
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            const longlong2 v = *reinterpret_cast<const longlong2 *>(er + src[i]);
            const u64 x0 = (u64)(sw[i] ? v.y : v.x), x1 = (u64)(sw[i] ? v.x : v.y);
            const i64 *kr = hk.ksk[i] + krow + (i64)p * part_stride + j0;
            const longlong2 k0 = ld_nt(kr);
            const longlong2 k1 = ld_nt(kr + comp_stride);
            acc[i][0][0] = csub(acc[i][0][0] + mm62u(x0, (u64)k0.x, m.q, m.k), m.q2);
            acc[i][0][1] = csub(acc[i][0][1] + mm62u(x1, (u64)k0.y, m.q, m.k), m.q2);
            acc[i][1][0] = csub(acc[i][1][0] + mm62u(x0, (u64)k1.x, m.q, m.k), m.q2);
            acc[i][1][1] = csub(acc[i][1][1] + mm62u(x1, (u64)k1.y, m.q, m.k), m.q2);
        }
    }
}

struct BabyArgs {
    HoistKeys hk;
    i64 *u[4];           // key i's pair [2][rows][N]
    const i64 *chat0;    // P NTT(c0): [ell][N], Montgomery form, words below 2q
    int ell;             // ordinary rows (the first `ell` of the rows)
};

template <int NR, bool PLANES, bool DPL>
__global__ void __launch_bounds__(256) ks_inner_baby_kernel(const i64 *__restrict__ ext, BabyArgs ba, i64 part_stride, i64 comp_stride,
                                                            i64 row_off, int nparts, int rows, int logN,
                                                            const i64 *__restrict__ ql, const i64 *__restrict__ qh,
                                                            const i64 *__restrict__ kl, const i64 *__restrict__ kh) {
    const int r = blockIdx.y;
    const i64 N = (i64)1 << logN;
    const i64 j0 = (i64)blockIdx.x * 512 + threadIdx.x * 2;
    if (j0 >= N) return;
    const RowMod m = load_mod(ql, qh, kl, kh, r);
    const unsigned sh = 32u - (unsigned)logN, mask = (2u << logN) - 1u;
    const unsigned bj = (2u * (__builtin_bitreverse32((unsigned)j0) >> sh) + 1u);
    unsigned src[NR];
    bool sw[NR];
#pragma unroll
    for (int i = 0; i < NR; ++i) {
        const unsigned t = (bj * ba.hk.p[i]) & mask;
        const unsigned mi = __builtin_bitreverse32((t - 1u) >> 1) >> sh;
        src[i] = mi & ~1u;
        sw[i] = (mi & 1u) != 0;
    }
    const i64 krow = (row_off + r) * N;
    const bool ord = r < ba.ell;
    const i64 *c0row = ba.chat0 + (i64)r * N;   // (read on ordinary rows only)
    const i64 o0 = (i64)r * N + j0, o1 = ((i64)rows + r) * N + j0;
    if (m.q < SMALL_PRIME_LIMIT) {
        const RowDp d = make_dp(m);
        double acc[NR][2][2];
        gathered_sums_dp<NR, PLANES, DPL>(ext, ba.hk, src, sw, part_stride, comp_stride, krow, j0, nparts, rows, r, N, d, acc);
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            if (ord) {
                double ca, cb;
                ld_pair_dp(c0row, (i64)src[i], N, 0, ca, cb);
                acc[i][0][0] += sw[i] ? cb : ca;
                acc[i][0][1] += sw[i] ? ca : cb;
            }
            longlong2 a, b;
            a.x = dp_to_word(dp_reduce(acc[i][0][0], d.q, d.qinv)), a.y = dp_to_word(dp_reduce(acc[i][0][1], d.q, d.qinv));
            b.x = dp_to_word(dp_reduce(acc[i][1][0], d.q, d.qinv)), b.y = dp_to_word(dp_reduce(acc[i][1][1], d.q, d.qinv));
            *reinterpret_cast<longlong2 *>(ba.u[i] + o0) = a;
            *reinterpret_cast<longlong2 *>(ba.u[i] + o1) = b;
        }
    } else {
        i64 acc[NR][2][2];
        gathered_sums_int<NR>(ext, ba.hk, src, sw, part_stride, comp_stride, krow, j0, nparts, rows, r, N, m, acc);
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            if (ord) {
                const longlong2 v = *reinterpret_cast<const longlong2 *>(c0row + src[i]);
                acc[i][0][0] = csub(acc[i][0][0] + (sw[i] ? v.y : v.x), m.q2);
                acc[i][0][1] = csub(acc[i][0][1] + (sw[i] ? v.x : v.y), m.q2);
            }
            longlong2 a, b;
            a.x = acc[i][0][0], a.y = acc[i][0][1], b.x = acc[i][1][0], b.y = acc[i][1][1];
            *reinterpret_cast<longlong2 *>(ba.u[i] + o0) = a;
            *reinterpret_cast<longlong2 *>(ba.u[i] + o1) = b;
        }
    }
}

// S^g_c = sum_b pt_{g,b} * u^b_c for NG giant steps: every row in the integer arithmetic (REDC62 holds for the small primes
// too, and the launch streams: per slot one baby pair, per diagonal 16 bytes per thread).  The baby pairs are read once per
// launch, whatever NG; a slot no giant step of the launch uses is not read.
struct DiagArgs {
    const i64 *u;                  // baby pairs [slots][2][rows][N] (slot 0: P NTT(c0), P NTT(c1), zero on the special rows)
    const i64 *pt[4];              // giant step i: the first diagonal of its slice of the pack, ascending slots
    unsigned long long slots[4];   // bit t: giant step i has a diagonal for baby slot t
    i64 *out[4];                   // its pair [2][rows][N] (giant step 0: the accumulator)
    i64 pt_stride;                 // words between the diagonals of the pack
    int nslots;
};

template <int NG>
__global__ void __launch_bounds__(256) lt_diag_products_kernel(DiagArgs da, int rows, int logN, const i64 *__restrict__ ql,
                                                               const i64 *__restrict__ qh, const i64 *__restrict__ kl,
                                                               const i64 *__restrict__ kh) {
    const int r = blockIdx.y;
    const i64 N = (i64)1 << logN;
    const i64 j0 = (i64)blockIdx.x * 512 + threadIdx.x * 2;
    if (j0 >= N) return;
    const RowMod m = load_mod(ql, qh, kl, kh, r);
    const i64 o0 = (i64)r * N + j0, pair = 2 * (i64)rows * N;
    i64 S[NG][2][2];
    const i64 *pt[NG];
    unsigned long long any = 0;
#pragma unroll
    for (int i = 0; i < NG; ++i) {
        S[i][0][0] = S[i][0][1] = S[i][1][0] = S[i][1][1] = 0;
        pt[i] = da.pt[i] + o0;
        any |= da.slots[i];
    }
    for (int t = 0; t < da.nslots; ++t) {
        if (!((any >> t) & 1ull)) continue;   // (wave-uniform: kernel arguments)
        const i64 *ur = da.u + (i64)t * pair + o0;
        const longlong2 u0 = *reinterpret_cast<const longlong2 *>(ur);
        const longlong2 u1 = *reinterpret_cast<const longlong2 *>(ur + (i64)rows * N);
#pragma unroll
        for (int i = 0; i < NG; ++i) {
            if (!((da.slots[i] >> t) & 1ull)) continue;
            const longlong2 w = ld_nt(pt[i]);
            pt[i] += da.pt_stride;
            S[i][0][0] = csub(S[i][0][0] + mm62u((u64)u0.x, (u64)w.x, m.q, m.k), m.q2);
            S[i][0][1] = csub(S[i][0][1] + mm62u((u64)u0.y, (u64)w.y, m.q, m.k), m.q2);
            S[i][1][0] = csub(S[i][1][0] + mm62u((u64)u1.x, (u64)w.x, m.q, m.k), m.q2);
            S[i][1][1] = csub(S[i][1][1] + mm62u((u64)u1.y, (u64)w.y, m.q, m.k), m.q2);
        }
    }
#pragma unroll
    for (int i = 0; i < NG; ++i) {
        longlong2 a, b;
        a.x = S[i][0][0], a.y = S[i][0][1], b.x = S[i][1][0], b.y = S[i][1][1];
        *reinterpret_cast<longlong2 *>(da.out[i] + o0) = a;
        *reinterpret_cast<longlong2 *>(da.out[i] + o0 + (i64)rows * N) = b;
    }
}

// ---- a matrix of linear transforms (lf_lt_matmul): S^o_c (+)= sum over the diagonals of block (o, i) of pt * t^{i,step}_c -----------
// lt_diag_products_kernel's streaming loop over the baby pairs of ONE input for NO outputs that have a block in its column: integer
// arithmetic on every row, each pair read once per launch whatever NO, a slot no output of the launch uses not read.  Every output
// brings its own pack (pointer and stride), its own slot mask, and a flag: its pair is written (the first input that contributes
// to it) or read - added - written (words below 2q both ways: the sums stay lazy Montgomery words whose residues alone count).
struct BlockArgs {
    const i64 *u;                  // the input's pairs [slots][2][rows][N] (slot 0: P NTT(c0), P NTT(c1), zero on the special rows)
    const i64 *pt[4];              // output i: the first diagonal of its block, ascending slots
    unsigned long long slots[4];   // bit t: the block has a diagonal for slot t
    i64 *out[4];                   // the output's pair S^o [2][rows][N]
    i64 pt_stride[4];              // words between the diagonals of the block's pack
    int fresh[4];                  // non-zero: S^o is written; zero: read, added to, written
    int nslots;
    i64 u_tstride, out_tstride;    // lt_block_productsb_kernel: the words from one token's `u` resp. `out[i]` to the next token's
};

template <int NO>
__global__ void __launch_bounds__(256) lt_block_products_kernel(BlockArgs ba, int rows, int logN, const i64 *__restrict__ ql,
                                                                const i64 *__restrict__ qh, const i64 *__restrict__ kl,
                                                                const i64 *__restrict__ kh) {
    const int r = blockIdx.y;
    const i64 N = (i64)1 << logN;
    const i64 j0 = (i64)blockIdx.x * 512 + threadIdx.x * 2;
    if (j0 >= N) return;
    const RowMod m = load_mod(ql, qh, kl, kh, r);
    const i64 o0 = (i64)r * N + j0, pair = 2 * (i64)rows * N;
    i64 S[NO][2][2];
    const i64 *pt[NO];
    unsigned long long any = 0;
#pragma unroll
    for (int i = 0; i < NO; ++i) {
        S[i][0][0] = S[i][0][1] = S[i][1][0] = S[i][1][1] = 0;
        pt[i] = ba.pt[i] + o0;
        any |= ba.slots[i];
    }
    for (int t = 0; t < ba.nslots; ++t) {
        if (!((any >> t) & 1ull)) continue;   // (wave-uniform: kernel arguments)
        const i64 *ur = ba.u + (i64)t * pair + o0;
        const longlong2 u0 = *reinterpret_cast<const longlong2 *>(ur);
        const longlong2 u1 = *reinterpret_cast<const longlong2 *>(ur + (i64)rows * N);
#pragma unroll
        for (int i = 0; i < NO; ++i) {
            if (!((ba.slots[i] >> t) & 1ull)) continue;
            const longlong2 w = ld_nt(pt[i]);
            pt[i] += ba.pt_stride[i];
            S[i][0][0] = csub(S[i][0][0] + mm62u((u64)u0.x, (u64)w.x, m.q, m.k), m.q2);
            S[i][0][1] = csub(S[i][0][1] + mm62u((u64)u0.y, (u64)w.y, m.q, m.k), m.q2);
            S[i][1][0] = csub(S[i][1][0] + mm62u((u64)u1.x, (u64)w.x, m.q, m.k), m.q2);
            S[i][1][1] = csub(S[i][1][1] + mm62u((u64)u1.y, (u64)w.y, m.q, m.k), m.q2);
        }
    }
#pragma unroll
    for (int i = 0; i < NO; ++i) {
        i64 *s0 = ba.out[i] + o0, *s1 = s0 + (i64)rows * N;
        longlong2 a, b;
        a.x = S[i][0][0], a.y = S[i][0][1], b.x = S[i][1][0], b.y = S[i][1][1];
        if (!ba.fresh[i]) {   // (wave-uniform)
            const longlong2 x = *reinterpret_cast<const longlong2 *>(s0), y = *reinterpret_cast<const longlong2 *>(s1);
            a.x = csub(a.x + x.x, m.q2), a.y = csub(a.y + x.y, m.q2);
            b.x = csub(b.x + y.x, m.q2), b.y = csub(b.y + y.y, m.q2);
        }
        *reinterpret_cast<longlong2 *>(s0) = a;
        *reinterpret_cast<longlong2 *>(s1) = b;
    }
}

// ---- lf_lt_matmul over NT tokens (lf_lt_matmul_batch): lt_block_products_kernel<NO> for NT tokens that share the blocks --------
// The same grid, the same loop over the slots of ONE input: per slot the NT pairs of the tokens (token k's pairs lie u_tstride
// words behind token k - 1's), then per output the diagonal word ONCE (ld_nt, 16 bytes per thread) multiplied into the NT
// accumulator sets; token k's sums go to out[i] + k * out_tstride, `fresh` per output as in the single kernel (the outputs of all
// tokens of a call have seen the same inputs).  Per (token, output) the products, their order and the conditional subtractions are
// those of lt_block_products_kernel<NO> on that token, so the words written are its words.
// Range: a pair word is below 2q (slot 0: mont_enter's; slots 1 ..: the baby sums' csub / dp_to_word), a diagonal word below 2q, q < 2^60,
// so the product a b < 4 q^2 < 2^122 is inside REDC62 and mm62u returns a b / 2^62 + q + 1 < 2q; S < 2q before every addition,
// S + product < 4q < 2^62, csub brings it below 2q again; the read - add - write of fresh = 0 adds two words below 2q likewise.  Nothing depends on
// the number of terms: every accumulator is reduced after each one.
template <int NO, int NT>
__global__ void __launch_bounds__(256) lt_block_productsb_kernel(BlockArgs ba, int rows, int logN, const i64 *__restrict__ ql,
                                                                 const i64 *__restrict__ qh, const i64 *__restrict__ kl,
                                                                 const i64 *__restrict__ kh) {
    const int r = blockIdx.y;
    const i64 N = (i64)1 << logN;
    const i64 j0 = (i64)blockIdx.x * 512 + threadIdx.x * 2;
    if (j0 >= N) return;
    const RowMod m = load_mod(ql, qh, kl, kh, r);
    const i64 o0 = (i64)r * N + j0, pair = 2 * (i64)rows * N;
    i64 S[NT][NO][2][2];
    const i64 *pt[NO];
    unsigned long long any = 0;
#pragma unroll
    for (int i = 0; i < NO; ++i) {
#pragma unroll
        for (int k = 0; k < NT; ++k) S[k][i][0][0] = S[k][i][0][1] = S[k][i][1][0] = S[k][i][1][1] = 0;
        pt[i] = ba.pt[i] + o0;
        any |= ba.slots[i];
    }
    for (int t = 0; t < ba.nslots; ++t) {
        if (!((any >> t) & 1ull)) continue;   // (wave-uniform: kernel arguments)
        longlong2 u0[NT], u1[NT];
#pragma unroll
        for (int k = 0; k < NT; ++k) {
            const i64 *ur = ba.u + (i64)k * ba.u_tstride + (i64)t * pair + o0;
            u0[k] = *reinterpret_cast<const longlong2 *>(ur);
            u1[k] = *reinterpret_cast<const longlong2 *>(ur + (i64)rows * N);
        }
#pragma unroll
        for (int i = 0; i < NO; ++i) {
            if (!((ba.slots[i] >> t) & 1ull)) continue;
            const longlong2 w = ld_nt(pt[i]);
            pt[i] += ba.pt_stride[i];
#pragma unroll
            for (int k = 0; k < NT; ++k) {
                S[k][i][0][0] = csub(S[k][i][0][0] + mm62u((u64)u0[k].x, (u64)w.x, m.q, m.k), m.q2);
                S[k][i][0][1] = csub(S[k][i][0][1] + mm62u((u64)u0[k].y, (u64)w.y, m.q, m.k), m.q2);
                S[k][i][1][0] = csub(S[k][i][1][0] + mm62u((u64)u1[k].x, (u64)w.x, m.q, m.k), m.q2);
                S[k][i][1][1] = csub(S[k][i][1][1] + mm62u((u64)u1[k].y, (u64)w.y, m.q, m.k), m.q2);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < NO; ++i) {
#pragma unroll
        for (int k = 0; k < NT; ++k) {
            i64 *s0 = ba.out[i] + (i64)k * ba.out_tstride + o0, *s1 = s0 + (i64)rows * N;
            longlong2 a, b;
            a.x = S[k][i][0][0], a.y = S[k][i][0][1], b.x = S[k][i][1][0], b.y = S[k][i][1][1];
            if (!ba.fresh[i]) {   // (wave-uniform)
                const longlong2 x = *reinterpret_cast<const longlong2 *>(s0), y = *reinterpret_cast<const longlong2 *>(s1);
                a.x = csub(a.x + x.x, m.q2), a.y = csub(a.y + x.y, m.q2);
                b.x = csub(b.x + y.x, m.q2), b.y = csub(b.y + y.y, m.q2);
            }
            *reinterpret_cast<longlong2 *>(s0) = a;
            *reinterpret_cast<longlong2 *>(s1) = b;
        }
    }
}

struct GiantArgs {
    HoistKeys hk;        // (one key)
    const i64 *s0;       // S^g_0: [rows][N], raw words below 2q
    i64 *acc;            // the accumulator pair [2][rows][N]: read, added to, written
};

template <bool PLANES, bool DPL>   // (the waves asked for are those of ks_inner_lt_kernel<1, PLANES, DPL>: one VGPR over 64 without)
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(PLANES ? 6 : 8))) ks_inner_giant_kernel(const i64 *__restrict__ ext, GiantArgs ga, i64 part_stride, i64 comp_stride,
                                                             i64 row_off, int nparts, int rows, int logN,
                                                             const i64 *__restrict__ ql, const i64 *__restrict__ qh,
                                                             const i64 *__restrict__ kl, const i64 *__restrict__ kh) {
    const int r = blockIdx.y;
    const i64 N = (i64)1 << logN;
    const i64 j0 = (i64)blockIdx.x * 512 + threadIdx.x * 2;
    if (j0 >= N) return;
    const RowMod m = load_mod(ql, qh, kl, kh, r);
    const unsigned sh = 32u - (unsigned)logN, mask = (2u << logN) - 1u;
    const unsigned bj = (2u * (__builtin_bitreverse32((unsigned)j0) >> sh) + 1u);
    const unsigned t = (bj * ga.hk.p[0]) & mask;
    const unsigned mi = __builtin_bitreverse32((t - 1u) >> 1) >> sh;
    const unsigned src[1] = {mi & ~1u};
    const bool sw[1] = {(mi & 1u) != 0};
    const i64 krow = (row_off + r) * N;
    const i64 *s0row = ga.s0 + (i64)r * N;
    i64 *a0 = ga.acc + (i64)r * N + j0, *a1 = ga.acc + ((i64)rows + r) * N + j0;
    if (m.q < SMALL_PRIME_LIMIT) {
        const RowDp d = make_dp(m);
        double acc[1][2][2];
        gathered_sums_dp<1, PLANES, DPL>(ext, ga.hk, src, sw, part_stride, comp_stride, krow, j0, nparts, rows, r, N, d, acc);
        double ca, cb, x0, y0, x1, y1;
        ld_pair_dp(s0row, (i64)src[0], N, 0, ca, cb);
        ld_pair_dp(a0, 0, N, 0, x0, y0);
        ld_pair_dp(a1, 0, N, 0, x1, y1);
        longlong2 a, b;   // |sums| < (digits / 2 + 4) q, inside dp_reduce's 64 q
        a.x = dp_to_word(dp_reduce(acc[0][0][0] + (sw[0] ? cb : ca) + x0, d.q, d.qinv));
        a.y = dp_to_word(dp_reduce(acc[0][0][1] + (sw[0] ? ca : cb) + y0, d.q, d.qinv));
        b.x = dp_to_word(dp_reduce(acc[0][1][0] + x1, d.q, d.qinv));
        b.y = dp_to_word(dp_reduce(acc[0][1][1] + y1, d.q, d.qinv));
        *reinterpret_cast<longlong2 *>(a0) = a;
        *reinterpret_cast<longlong2 *>(a1) = b;
    } else {
        i64 acc[1][2][2];
        gathered_sums_int<1>(ext, ga.hk, src, sw, part_stride, comp_stride, krow, j0, nparts, rows, r, N, m, acc);
        const longlong2 v = *reinterpret_cast<const longlong2 *>(s0row + src[0]);
        longlong2 a = *reinterpret_cast<const longlong2 *>(a0), b = *reinterpret_cast<const longlong2 *>(a1);
        a.x = csub(a.x + csub(acc[0][0][0] + (sw[0] ? v.y : v.x), m.q2), m.q2);
        a.y = csub(a.y + csub(acc[0][0][1] + (sw[0] ? v.x : v.y), m.q2), m.q2);
        b.x = csub(b.x + acc[0][1][0], m.q2);
        b.y = csub(b.y + acc[0][1][1], m.q2);
        *reinterpret_cast<longlong2 *>(a0) = a;
        *reinterpret_cast<longlong2 *>(a1) = b;
    }
}

// ---- a matrix of baby-step / giant-step transforms (lf_lt_matmul_bsgs): the giant step of NCT outputs under ONE key -------------
// ks_inner_giant_kernel for the NCT (2 or 4) outputs that share a giant step: its grid and its key / digit formats, one key and
// hence ONE pi for the whole group (src / sw once per thread).  Per part the key's four words are loaded once and multiplied into
// NCT x 4 accumulators; then per output the gathered word of its S^g_0 on all rows and the read - add - write of its accumulator
// pair, exactly as the single kernel does: dp_reduce once on the fp64-class rows (|sums| < (digits / 2 + 4) q: lf_fp64_digits_ok),
// lazy words below 2q on the integer rows.  The key stream of the giant step crosses HBM once for the group.
struct GiantBatchArgs {
    const i64 *ksk;      // the key, at its first part
    unsigned p;          // its exponent (odd, < 2N)
    i64 ext_stride;      // words between the outputs' stacks of extended digits ([nparts][rows][N] each)
    const i64 *s0[4];    // output t: S^g_0 [rows][N], raw words below 2q
    i64 *acc[4];         // .. its accumulator pair [2][rows][N]: read, added to, written
};

template <int NCT, bool PLANES, bool DPL>   // (four outputs already have four digit pairs in flight per key word: their digit loop is not unrolled)
__global__ void __launch_bounds__(256) ks_inner_giantb_kernel(const i64 *__restrict__ ext, GiantBatchArgs ga, i64 part_stride, i64 comp_stride,
                                                              i64 row_off, int nparts, int rows, int logN,
                                                              const i64 *__restrict__ ql, const i64 *__restrict__ qh,
                                                              const i64 *__restrict__ kl, const i64 *__restrict__ kh) {
    const int r = blockIdx.y;
    const i64 N = (i64)1 << logN;
    const i64 j0 = (i64)blockIdx.x * 512 + threadIdx.x * 2;
    if (j0 >= N) return;
    const RowMod m = load_mod(ql, qh, kl, kh, r);
    const unsigned sh = 32u - (unsigned)logN, mask = (2u << logN) - 1u;
    const unsigned bj = (2u * (__builtin_bitreverse32((unsigned)j0) >> sh) + 1u);
    const unsigned t0 = (bj * ga.p) & mask;
    const unsigned mi = __builtin_bitreverse32((t0 - 1u) >> 1) >> sh;
    const i64 src = (i64)(mi & ~1u);
    const bool sw = (mi & 1u) != 0;
    const i64 *krow = ga.ksk + (row_off + r) * N;
    const i64 a0 = (i64)r * N + j0, a1 = ((i64)rows + r) * N + j0;
    if (m.q < SMALL_PRIME_LIMIT) {
        const RowDp d = make_dp(m);
        constexpr int DIGITS_IN_FLIGHT = NCT == 4 ? 1 : KI_UNROLL;
        double acc[NCT][2][2];
#pragma unroll
        for (int t = 0; t < NCT; ++t) acc[t][0][0] = acc[t][0][1] = acc[t][1][0] = acc[t][1][1] = 0.0;
#pragma unroll DIGITS_IN_FLIGHT
        for (int p = 0; p < nparts; ++p) {
            const i64 *kr = krow + (i64)p * part_stride;
            double k0x, k0y, k1x, k1y;
            if (PLANES) {   // 16 + 8 bytes for both components (see lf_key_planes)
                const lf_u4_t l = __builtin_nontemporal_load(reinterpret_cast<const lf_u4_t *>(reinterpret_cast<const unsigned *>(kr) + 2 * j0));
                const lf_u2_t h = __builtin_nontemporal_load(reinterpret_cast<const lf_u2_t *>(reinterpret_cast<const unsigned *>(kr + comp_stride) + j0));
                k0x = dp_from_planes(l.x, h.x & 0xffffu), k0y = dp_from_planes(l.y, h.x >> 16);
                k1x = dp_from_planes(l.z, h.y & 0xffffu), k1y = dp_from_planes(l.w, h.y >> 16);
            } else {
                const longlong2 k0 = ld_nt(kr + j0);
                const longlong2 k1 = ld_nt(kr + j0 + comp_stride);
                k0x = dp_from_word(k0.x), k0y = dp_from_word(k0.y), k1x = dp_from_word(k1.x), k1y = dp_from_word(k1.y);
            }
            const i64 *er = ext + ((i64)p * rows + r) * N;
#pragma unroll
            for (int t = 0; t < NCT; ++t) {
                double xa, xb;
                ld_pair_dp(er + (i64)t * ga.ext_stride, src, N, DPL ? 1 : 0, xa, xb);
                const double x0 = sw ? xb : xa, x1 = sw ? xa : xb;
                acc[t][0][0] += dp_mulmod_bal(x0, k0x, d);
                acc[t][0][1] += dp_mulmod_bal(x1, k0y, d);
                acc[t][1][0] += dp_mulmod_bal(x0, k1x, d);
                acc[t][1][1] += dp_mulmod_bal(x1, k1y, d);
            }
        }
#pragma unroll
        for (int t = 0; t < NCT; ++t) {
            double ca, cb, x0, y0, x1, y1;
            ld_pair_dp(ga.s0[t] + (i64)r * N, src, N, 0, ca, cb);
            ld_pair_dp(ga.acc[t] + a0, 0, N, 0, x0, y0);
            ld_pair_dp(ga.acc[t] + a1, 0, N, 0, x1, y1);
            longlong2 a, b;   // |sums| < (digits / 2 + 4) q, inside dp_reduce's 64 q
            a.x = dp_to_word(dp_reduce(acc[t][0][0] + (sw ? cb : ca) + x0, d.q, d.qinv));
            a.y = dp_to_word(dp_reduce(acc[t][0][1] + (sw ? ca : cb) + y0, d.q, d.qinv));
            b.x = dp_to_word(dp_reduce(acc[t][1][0] + x1, d.q, d.qinv));
            b.y = dp_to_word(dp_reduce(acc[t][1][1] + y1, d.q, d.qinv));
            *reinterpret_cast<longlong2 *>(ga.acc[t] + a0) = a;
            *reinterpret_cast<longlong2 *>(ga.acc[t] + a1) = b;
        }
    } else {
        i64 acc[NCT][2][2];
#pragma unroll
        for (int t = 0; t < NCT; ++t) acc[t][0][0] = acc[t][0][1] = acc[t][1][0] = acc[t][1][1] = 0;
        for (int p = 0; p < nparts; ++p) {
            const i64 *kr = krow + (i64)p * part_stride + j0;
            const longlong2 k0 = ld_nt(kr);
            const longlong2 k1 = ld_nt(kr + comp_stride);
            const i64 *er = ext + ((i64)p * rows + r) * N + src;
#pragma unroll
            for (int t = 0; t < NCT; ++t) {
                const longlong2 v = *reinterpret_cast<const longlong2 *>(er + (i64)t * ga.ext_stride);
                const u64 x0 = (u64)(sw ? v.y : v.x), x1 = (u64)(sw ? v.x : v.y);
                acc[t][0][0] = csub(acc[t][0][0] + mm62u(x0, (u64)k0.x, m.q, m.k), m.q2);
                acc[t][0][1] = csub(acc[t][0][1] + mm62u(x1, (u64)k0.y, m.q, m.k), m.q2);
                acc[t][1][0] = csub(acc[t][1][0] + mm62u(x0, (u64)k1.x, m.q, m.k), m.q2);
                acc[t][1][1] = csub(acc[t][1][1] + mm62u(x1, (u64)k1.y, m.q, m.k), m.q2);
            }
        }
#pragma unroll
        for (int t = 0; t < NCT; ++t) {
            const longlong2 v = *reinterpret_cast<const longlong2 *>(ga.s0[t] + (i64)r * N + src);
            longlong2 a = *reinterpret_cast<const longlong2 *>(ga.acc[t] + a0), b = *reinterpret_cast<const longlong2 *>(ga.acc[t] + a1);
            a.x = csub(a.x + csub(acc[t][0][0] + (sw ? v.y : v.x), m.q2), m.q2);
            a.y = csub(a.y + csub(acc[t][0][1] + (sw ? v.x : v.y), m.q2), m.q2);
            b.x = csub(b.x + acc[t][1][0], m.q2);
            b.y = csub(b.y + acc[t][1][1], m.q2);
            *reinterpret_cast<longlong2 *>(ga.acc[t] + a0) = a;
            *reinterpret_cast<longlong2 *>(ga.acc[t] + a1) = b;
        }
    }
}

// ---- baby-step / giant-step transform of many ciphertexts (lf_linear_transform_bsgs_batch): the baby step of NCT ciphertexts
// under ONE key -------------
// ks_inner_baby_kernel<1, ..> for the NCT (2 or 4) ciphertexts of a group: the grid, the pi computation (one key, hence ONE pi:
// src / sw once per thread) and the key / digit formats of ks_inner_giantb_kernel.  Per part the key's four words are loaded once
// and multiplied into NCT x 4 accumulators; then per ciphertext the gathered word of its own P NTT(c0) on the ordinary rows, and
// its pair u^{t,b} written in the format lt_diag_products_kernel reads, exactly as the single kernel writes it: dp_reduce once per
// word to a canonical word on the fp64-class rows (the sums are per ciphertext: |sums| < (digits / 2 + 2) q, lf_fp64_digits_ok),
// lazy words below 2q on the integer rows.  No read - add - write: the baby key's stream crosses HBM once for the group.
static_assert(LF_FP64_MAX_DIGITS / 2 + 2 < 64, "ks_inner_babyb_kernel: digits / 2 + 2 (the word of P c0) must stay inside dp_reduce's 64 q");
struct BabyBatchArgs {
    const i64 *ksk;        // the key, at its first part
    unsigned p;            // its exponent (odd, < 2N)
    int ell;               // ordinary rows (the first `ell` of the rows)
    i64 ext_stride;        // words between the ciphertexts' stacks of extended digits ([nparts][rows][N] each)
    const i64 *chat0[4];   // ciphertext t: P NTT(c0) [ell][N], Montgomery form, words below 2q
    i64 *u[4];             // .. its pair under this key [2][rows][N]: written
};

template <int NCT, bool PLANES, bool DPL>   // (the digit loop as in ks_inner_giantb_kernel: not unrolled for four ciphertexts)
__global__ void __launch_bounds__(256) ks_inner_babyb_kernel(const i64 *__restrict__ ext, BabyBatchArgs ba, i64 part_stride, i64 comp_stride,
                                                             i64 row_off, int nparts, int rows, int logN,
                                                             const i64 *__restrict__ ql, const i64 *__restrict__ qh,
                                                             const i64 *__restrict__ kl, const i64 *__restrict__ kh) {
    const int r = blockIdx.y;
    const i64 N = (i64)1 << logN;
    const i64 j0 = (i64)blockIdx.x * 512 + threadIdx.x * 2;
    if (j0 >= N) return;
    const RowMod m = load_mod(ql, qh, kl, kh, r);
    const unsigned sh = 32u - (unsigned)logN, mask = (2u << logN) - 1u;
    const unsigned bj = (2u * (__builtin_bitreverse32((unsigned)j0) >> sh) + 1u);
    const unsigned t0 = (bj * ba.p) & mask;
    const unsigned mi = __builtin_bitreverse32((t0 - 1u) >> 1) >> sh;
    const i64 src = (i64)(mi & ~1u);
    const bool sw = (mi & 1u) != 0;
    const i64 *krow = ba.ksk + (row_off + r) * N;
    const bool ord = r < ba.ell;   // (wave-uniform; P NTT(c0) is read on ordinary rows only)
    const i64 o0 = (i64)r * N + j0, o1 = ((i64)rows + r) * N + j0;
    if (m.q < SMALL_PRIME_LIMIT) {
        const RowDp d = make_dp(m);
        constexpr int DIGITS_IN_FLIGHT = NCT == 4 ? 1 : KI_UNROLL;
        double acc[NCT][2][2];
#pragma unroll
        for (int t = 0; t < NCT; ++t) acc[t][0][0] = acc[t][0][1] = acc[t][1][0] = acc[t][1][1] = 0.0;
#pragma unroll DIGITS_IN_FLIGHT
        for (int p = 0; p < nparts; ++p) {
            const i64 *kr = krow + (i64)p * part_stride;
            double k0x, k0y, k1x, k1y;
            if (PLANES) {   // 16 + 8 bytes for both components (see lf_key_planes)
                const lf_u4_t l = __builtin_nontemporal_load(reinterpret_cast<const lf_u4_t *>(reinterpret_cast<const unsigned *>(kr) + 2 * j0));
                const lf_u2_t h = __builtin_nontemporal_load(reinterpret_cast<const lf_u2_t *>(reinterpret_cast<const unsigned *>(kr + comp_stride) + j0));
                k0x = dp_from_planes(l.x, h.x & 0xffffu), k0y = dp_from_planes(l.y, h.x >> 16);
                k1x = dp_from_planes(l.z, h.y & 0xffffu), k1y = dp_from_planes(l.w, h.y >> 16);
            } else {
                const longlong2 k0 = ld_nt(kr + j0);
                const longlong2 k1 = ld_nt(kr + j0 + comp_stride);
                k0x = dp_from_word(k0.x), k0y = dp_from_word(k0.y), k1x = dp_from_word(k1.x), k1y = dp_from_word(k1.y);
            }
            const i64 *er = ext + ((i64)p * rows + r) * N;
#pragma unroll
            for (int t = 0; t < NCT; ++t) {
                double xa, xb;
                ld_pair_dp(er + (i64)t * ba.ext_stride, src, N, DPL ? 1 : 0, xa, xb);
                const double x0 = sw ? xb : xa, x1 = sw ? xa : xb;
                acc[t][0][0] += dp_mulmod_bal(x0, k0x, d);
                acc[t][0][1] += dp_mulmod_bal(x1, k0y, d);
                acc[t][1][0] += dp_mulmod_bal(x0, k1x, d);
                acc[t][1][1] += dp_mulmod_bal(x1, k1y, d);
            }
        }
#pragma unroll
        for (int t = 0; t < NCT; ++t) {
            if (ord) {
                double ca, cb;
                ld_pair_dp(ba.chat0[t] + (i64)r * N, src, N, 0, ca, cb);
                acc[t][0][0] += sw ? cb : ca;
                acc[t][0][1] += sw ? ca : cb;
            }
            longlong2 a, b;   // |sums| < (digits / 2 + 2) q, inside dp_reduce's 64 q
            a.x = dp_to_word(dp_reduce(acc[t][0][0], d.q, d.qinv)), a.y = dp_to_word(dp_reduce(acc[t][0][1], d.q, d.qinv));
            b.x = dp_to_word(dp_reduce(acc[t][1][0], d.q, d.qinv)), b.y = dp_to_word(dp_reduce(acc[t][1][1], d.q, d.qinv));
            *reinterpret_cast<longlong2 *>(ba.u[t] + o0) = a;
            *reinterpret_cast<longlong2 *>(ba.u[t] + o1) = b;
        }
    } else {
        i64 acc[NCT][2][2];
#pragma unroll
        for (int t = 0; t < NCT; ++t) acc[t][0][0] = acc[t][0][1] = acc[t][1][0] = acc[t][1][1] = 0;
        for (int p = 0; p < nparts; ++p) {
            const i64 *kr = krow + (i64)p * part_stride + j0;
            const longlong2 k0 = ld_nt(kr);
            const longlong2 k1 = ld_nt(kr + comp_stride);
            const i64 *er = ext + ((i64)p * rows + r) * N + src;
#pragma unroll
            for (int t = 0; t < NCT; ++t) {
                const longlong2 v = *reinterpret_cast<const longlong2 *>(er + (i64)t * ba.ext_stride);
                const u64 x0 = (u64)(sw ? v.y : v.x), x1 = (u64)(sw ? v.x : v.y);
                acc[t][0][0] = csub(acc[t][0][0] + mm62u(x0, (u64)k0.x, m.q, m.k), m.q2);
                acc[t][0][1] = csub(acc[t][0][1] + mm62u(x1, (u64)k0.y, m.q, m.k), m.q2);
                acc[t][1][0] = csub(acc[t][1][0] + mm62u(x0, (u64)k1.x, m.q, m.k), m.q2);
                acc[t][1][1] = csub(acc[t][1][1] + mm62u(x1, (u64)k1.y, m.q, m.k), m.q2);
            }
        }
#pragma unroll
        for (int t = 0; t < NCT; ++t) {
            if (ord) {
                const longlong2 v = *reinterpret_cast<const longlong2 *>(ba.chat0[t] + (i64)r * N + src);
                acc[t][0][0] = csub(acc[t][0][0] + (sw ? v.y : v.x), m.q2);
                acc[t][0][1] = csub(acc[t][0][1] + (sw ? v.x : v.y), m.q2);
            }
            longlong2 a, b;
            a.x = acc[t][0][0], a.y = acc[t][0][1], b.x = acc[t][1][0], b.y = acc[t][1][1];
            *reinterpret_cast<longlong2 *>(ba.u[t] + o0) = a;
            *reinterpret_cast<longlong2 *>(ba.u[t] + o1) = b;
        }
    }
}

// largest number of leading stages (logN - 12) whose extension + strided pass runs as the column kernel (lf_tune).
// With the digit loop as a runtime loop (R loads in flight, 100 VGPRs at R = 16) the column form also wins at logN 16:
// gold cc_mult 2 104-2 130 -> 2 168-2 183 ops/s, rotate 2 653-2 695 -> 2 733-2 763, 64 rotations under one key
// 3 110 -> 3 300 /s (tools/eo.py --ext-cols-max 3 | 4, one box); round 2's fully unrolled form had lost there (116 vs 95 us).
// And at logN 17 (platinum, 32 words per thread: 173 VGPRs, 2 waves per SIMD — the kernel's waves_per_eu follows K), together with
// the column form of the sums' last inverse pass: cc_mult 2 163 -> 2 054 us, rotate 1 845 -> 1 740 us, same words.
int g_ks_ext_cols_max = 5;

// The extended digits between ks_forward and ks_tail (tmp: scratch of the key switch, opaque to the caller) keep the
// fp64-class rows in planes format — 6 bytes per word on each of their three trips — at every two-pass ring degree (the column
// kernel and the LDS-tiled extension both write it) where both classes are present.  BOTH halves decide with this function: the
// knob must not change between an lf_ks_fwd and its lf_ks_tail (lf_tune is a start-up / A-B facility, see the header).
int g_digit_planes = 1;
int g_more_planes = 3;   // LF_TUNE_MORE_PLANES: bit 0 = the sums of a key switch, bit 1 = cc_mult's operand stack (with g_digit_planes)
bool digit_planes(int logN, const RowList &dp, const RowList &in) {
    return g_digit_planes && logN > NTT_TILE_LOG_MAX && dp.n && in.n;
}

}  // namespace

// LF_FP64_MAX_DIGITS (include/ckks_hip.h): every fp64-class inner product adds `nparts` balanced products (|.| <= q / 2 each)
// and reduces once with dp_reduce, exact for |x| < 64 q.  What else joins the sum before that reduction, per kernel:
//   ks_inner_hoist_kernel                  nothing                                    nparts / 2     < 64:  nparts <= 127
//   ks_inner2(_presum)_kernel, ks_dotb_    the fold's balanced product with PR        nparts / 2 + 1/2 < 64: nparts <= 126
//     inner_kernel (the same body)
//   ks_inner_baby_kernel, ks_inner_lt_     one word of P c0 below 2q                  nparts / 2 + 2 < 64:  nparts <= 123
//     kernel (it reduces there with dp_reduce_bal, |x| < 2^52, and its running pair stays within (NR + 2) q)
//   ks_inner_babyb_kernel                  per ciphertext as ks_inner_baby_kernel: one word of P c0 below 2q (the NCT sums of a
//                                          launch are separate accumulators)          nparts / 2 + 2 < 64:  nparts <= 123
//   ks_inner_ltb_kernel                    per key and ciphertext as ks_inner_lt_kernel               nparts <= 123
//     (its NCT running pairs stay in registers over the LF_LTB_KEYS keys of a launch: one start term — a balanced product or a
//     canonical word below q — and LF_LTB_KEYS balanced products, |S| <= (LF_LTB_KEYS / 2 + 1) q = 5 q < 64 q, reduced once
//     with dp_reduce when the launch ends; a launch of 126 keys or more would have to reduce inside its loop: static_assert there)
//   ks_inner_giant_kernel                  a word of S^g_0 and one of the accumulator, both below 2q
//                                                                                     nparts / 2 + 4 < 64:  nparts <= 119
//   ks_inner_rsum_kernel                   NR nparts products, NR + 1 words below 2q: reduced first with dp_reduce_bal
//                                          (|x| < 2^52), so no bound of its own below 119 (see the kernel)
//   ks_inner_rsumb_kernel                  per ciphertext nk nparts products, nk + 1 words below 2q over the nk <= LF_RSB_KEYS keys
//                                          of a launch: (8 x 119 / 2 + 18) q = 494 q < 2^52, reduced once with dp_reduce_bal
//                                          (static_assert there), so no bound of its own below 119
// The tightest holds for all of them.  Integer-class rows reduce after every addition and have no such bound.
bool lf_fp64_digits_ok(int nparts, int rows, const int64_t *q_host) {
    if (nparts <= LF_FP64_MAX_DIGITS || !q_host) return true;
    for (int r = 0; r < rows; ++r)
        if ((uint64_t)q_host[r] < SMALL_PRIME_LIMIT) return false;
    return true;
}
extern "C" int lf_stack_planes(int logN, int rows, const int64_t *q_host) {
    if (!g_digit_planes || !(g_more_planes & 2) || logN <= NTT_TILE_LOG_MAX || logN > KS_LOGN_MAX || !q_host || rows < 1) return 0;
    int small = 0, large = 0;
    for (int r = 0; r < rows; ++r) ((uint64_t)q_host[r] < SMALL_PRIME_LIMIT ? small : large)++;
    return small && large ? 1 : 0;
}
namespace {
void classify_rows(int rows, const int64_t *q_host, RowList &dp, RowList &in) {
    dp.n = in.n = 0;
    for (int r = 0; r < rows; ++r) {
        RowList &dst = (q_host && (uint64_t)q_host[r] < SMALL_PRIME_LIMIT) ? dp : in;
        dst.id[dst.n++] = (unsigned short)r;
    }
}

// K2 + P2 of `nparts` digits (descriptors desc[0 .. nparts), extended digits into tmp[nct][nparts][rows][N])
int ks_forward(const int64_t *state, int64_t state_stride, int nct, int nparts, int rows, int logN, const int64_t *desc,
               const int64_t *E, const double *Ed, int64_t *tmp, const LfFwdTab &ft, const LfMod &m, hipStream_t st,
               const unsigned char *own = nullptr, int p0 = 0) {
    const int64_t *psi_br = ft.psi_br, *ql = m.ql, *qh = m.qh, *kl = m.kl, *kh = m.kh;
    const double *psi_dp = ft.psi_dp;
    if (!psi_dp) return LF_ERR_ARG;   // the relaxed arithmetic of both classes lives in the auxiliary table
    const int tl = NTT_TILE_LOG_MAX, S1 = logN - tl;
    RowList dp, in;
    classify_rows(rows, m.q_host, dp, in);
    const bool dplanes = digit_planes(logN, dp, in);
    lf_fmt_note(tmp, ((size_t)nct * nparts * rows << logN) * 8, dplanes ? LF_FMT_PLANES : LF_FMT_RAW);
    const KsGeom kg{logN, tl, S1, rows, nparts, (i64)1 << logN, nct, (i64)state_stride, own, p0, dplanes ? 1 : 0};
    const unsigned tiles = 1u << (logN - tl);
    const unsigned polys = (unsigned)nparts * (unsigned)nct;   // extended digits of all ciphertexts: one stack
    const bool mixed = dp.n && in.n;   // both arithmetic classes in one launch per step
    // K2: extend + strided pass — as one register step per column when the strided pass has at most 4 stages
    // (measured on MI355X, extension kernel alone: silver / logN 15 22.5 -> 20.0 us; gold / logN 16 see g_ks_ext_cols_max)
    if (S1 <= g_ks_ext_cols_max) {
        const unsigned per_limb = ((1u << tl) / NTT_COL_THREADS) * polys;   // column chunks x digits x ciphertexts
        const ClassLists cl = class_lists(in, dp, per_limb * (unsigned)in.n);   // either list may be empty
        const dim3 grid((unsigned)cl.in_blocks + per_limb * (unsigned)dp.n), block(NTT_COL_THREADS);
#define LF_EXT_COLS_CASE(KK)                                                                                            \
    case KK:                                                                                                            \
        hipLaunchKernelGGL((ks_ext_cols_mixed<KK>), grid, block, 0, st, (const i64 *)state, (i64 *)tmp, kg, cl,          \
                           (const i64 *)desc, (const i64 *)E, Ed, (const i64 *)psi_br, psi_dp, (const i64 *)ql,         \
                           (const i64 *)qh, (const i64 *)kl, (const i64 *)kh);                                         \
        break;
        switch (S1) { LF_EXT_COLS_CASE(1) LF_EXT_COLS_CASE(2) LF_EXT_COLS_CASE(3) LF_EXT_COLS_CASE(4) LF_EXT_COLS_CASE(5) }
#undef LF_EXT_COLS_CASE
    } else if (mixed) {
        const ClassLists cl = class_lists(in, dp, tiles * in.n * polys);
        hipLaunchKernelGGL(ks_ext_pass1_mixed, dim3((unsigned)cl.in_blocks + tiles * dp.n * polys), dim3(NTT_THREADS), 0, st,
                           (const i64 *)state, (i64 *)tmp, kg, cl, (const i64 *)desc, (const i64 *)E, Ed, (const i64 *)psi_br,
                           psi_dp, (const i64 *)ql, (const i64 *)qh, (const i64 *)kl, (const i64 *)kh);
    } else if (dp.n)
        hipLaunchKernelGGL(ks_ext_pass1<true>, dim3(tiles * dp.n * polys), dim3(NTT_THREADS), 0, st, (const i64 *)state,
                           (i64 *)tmp, kg, dp, (const i64 *)desc, (const i64 *)E, Ed, (const i64 *)psi_br, psi_dp,
                           (const i64 *)ql, (const i64 *)qh, (const i64 *)kl, (const i64 *)kh);
    if (in.n && !mixed)
        hipLaunchKernelGGL(ks_ext_pass1<false>, dim3(tiles * in.n * polys), dim3(NTT_THREADS), 0, st, (const i64 *)state,
                           (i64 *)tmp, kg, in, (const i64 *)desc, (const i64 *)E, Ed, (const i64 *)psi_br, psi_dp,
                           (const i64 *)ql, (const i64 *)qh, (const i64 *)kl, (const i64 *)kh);
    // contiguous forward pass, in place on tmp (relaxed)
    {
        const PassGeom g{logN, tl, 0, tl, S1, 0, rows, (int)polys, 1, 1, 0, own, nparts, p0};
        launch_pass16(false, 1, (int)polys, st, (const i64 *)tmp, (i64 *)tmp, g, in, dp, (const i64 *)psi_br, psi_dp,
                      (const i64 *)ql, (const i64 *)qh, (const i64 *)kl, (const i64 *)kh, nullptr, dplanes);
    }
    return (int)hipGetLastError();
}

// How the sums of ONE key switch travel, decided here and nowhere else: every launcher of an inner-product kernel takes its grid,
// its DPL template flag and the `spl` argument from this, holds the digits to `digit_fmt`, and hands it to ks_inv_sums.  The
// launchers whose sums stay in the NTT domain (baby and giant steps) ask for no pairs and use dplanes, digit_fmt and the grid alone.
struct KsSums {
    int logN, rows, pairs;   // pairs of sums [pairs][2][rows][N] the inverse transform takes
    RowList dp, in;          // the rows of the fp64 class / of the integer class
    bool mixed;              // both classes present: one launch per step covers both
    bool dplanes;            // the digits' fp64-class rows are in planes format (digit_planes())
    bool cols_last;          // the last inverse pass runs as the column kernel
    bool spl;                // the sums' fp64-class rows travel as planes too
    dim3 grid;               // of the inner-product kernels: 512 coefficients per block x rows
    int digit_fmt;           // what lf_fmt_expect is asked about the digits
    // the digits of `cts` ciphertexts must be in the format this half is about to read (lf_tune flipped between lf_ks_fwd and
    // here: LF_ERR_STATE)
    int expect_digits(const int64_t *ext, int cts, int nparts) const {
        return lf_fmt_expect(ext, ((size_t)cts * nparts * rows << logN) * 8, digit_fmt);
    }
};
KsSums ks_sums(int logN, int rows, const int64_t *q_host, int pairs, const int64_t *scratch, int64_t scratch_words) {
    KsSums k{};
    k.logN = logN, k.rows = rows, k.pairs = pairs;
    classify_rows(rows, q_host, k.dp, k.in);
    const int S1 = logN - NTT_TILE_LOG_MAX;
    k.mixed = k.dp.n && k.in.n;
    k.dplanes = digit_planes(logN, k.dp, k.in);
    k.cols_last = S1 <= 4 || (S1 == 5 && k.mixed && g_ks_ext_cols_max > 4);   // column form of the last inverse pass
    // The SUMS travel the same way as the digits: the inner product writes fp64-class rows as planes into s, the tiled inverse
    // pass carries them s -> scratch (a pass that changes the format cannot run in place; ks_tail hands the digits' own buffer,
    // spent by then), the column pass reads the planes and leaves canonical words in s.  6 instead of 8 bytes per word on three
    // of the sums' four trips; needs room for the 2 x pairs polynomials in scratch and the column form of the last pass, else
    // the sums stay raw words: same outputs.
    k.spl = k.dplanes && (g_more_planes & 1) && k.cols_last && pairs && scratch && scratch_words >= ((int64_t)2 * pairs * rows << logN);
    const i64 N = (i64)1 << logN;
    k.grid = dim3((unsigned)((N + 512 * KI_COLS - 1) / (512 * KI_COLS)), (unsigned)rows);
    k.digit_fmt = k.dplanes ? LF_FMT_PLANES : LF_FMT_RAW;
    return k;
}

// the two formats of a launch as compile-time constants: f(PLANES, DPL) with the key in planes format / the digits' fp64-class rows
// in planes format; LF_CT(X) is the constant an argument X carries
#define LF_CT(X) std::remove_reference_t<decltype(X)>::value
template <class F>
void with_formats(bool planes, bool dplanes, F &&f) {
    if (planes && dplanes) f(std::true_type{}, std::true_type{});
    else if (planes) f(std::true_type{}, std::false_type{});
    else if (dplanes) f(std::false_type{}, std::true_type{});
    else f(std::false_type{}, std::false_type{});
}
// .. and a group size out of Gs (keys, ciphertexts or outputs of one launch): f(G); false, nothing called, for any other size
template <int... Gs, class F>
bool with_count(int g, F &&f) {
    return ((g == Gs ? (f(std::integral_constant<int, Gs>{}), true) : false) || ...);
}
// the keys of one launch of the lt, rsum and baby kernels: 4 while 4 are left, then 2, then 1 (tests/test_accumulating_ops_edges_cpu.py
// mirrors it)
int key_group(int left) { return left >= 4 ? 4 : left >= 2 ? 2 : left > 0 ? 1 : 0; }
// keys i0 .. i0 + g - 1 of the list and their exponents, as the kernels take them
HoistKeys hoist_keys(const LfKeys &key, const int64_t *p_host, int i0, int g) {
    HoistKeys hk{};
    for (int t = 0; t < g; ++t) {
        hk.ksk[t] = (const i64 *)key.ksk[i0 + t];
        hk.p[t] = (unsigned)p_host[i0 + t];
    }
    return hk;
}
// the four per-row constant arrays as a kernel takes them
#define LF_MOD_ARGS(m) (const i64 *)(m).ql, (const i64 *)(m).qh, (const i64 *)(m).kl, (const i64 *)(m).kh

// K4: inverse transform of the 2 x ks.pairs sums [2 pairs][rows][N] -> canonical coefficients (relaxed, tail 2), in place on s;
// ks.spl: the sums' fp64-class rows arrive as planes and the tiled pass carries them through tmp (room for all of them)
int ks_inv_sums(const KsSums &ks, i64 *tmp, i64 *s, const LfInvTab &it, const LfMod &m, hipStream_t st) {
    const int inv_polys = 2 * ks.pairs, rows = ks.rows, logN = ks.logN;
    const bool spl = ks.spl, cols_last = ks.cols_last, mixed = ks.mixed;
    const RowList &in = ks.in, &dp = ks.dp;
    const int64_t *ipsi_br = it.ipsi_br, *Ninv = it.Ninv, *ql = m.ql, *qh = m.qh, *kl = m.kl, *kh = m.kh;
    const double *ipsi_dp = it.ipsi_dp;
    const int tl = NTT_TILE_LOG_MAX, S1 = logN - tl;
    const unsigned per_row2 = (unsigned)inv_polys << (logN - tl);
    for (int pass = 0; pass < 2; ++pass) {
        PassGeom g = pass == 0 ? PassGeom{logN, tl, 0, tl, 0, 0, rows, inv_polys, 1, 0, 0}
                               : PassGeom{logN, tl, 1, S1, tl, tl - S1, rows, inv_polys, 1, 1, 0};
        if (pass == 0) {
            launch_pass16(true, 1, inv_polys, st, (const i64 *)s, spl ? (i64 *)tmp : (i64 *)s, g, in, dp, (const i64 *)ipsi_br, ipsi_dp,
                          (const i64 *)ql, (const i64 *)qh, (const i64 *)kl, (const i64 *)kh, nullptr, spl);
            continue;
        }
        if (pass == 1 && cols_last) {   // (logN 17: the column form of both ends goes with the knob)
            if (spl) {
                g.pln = PLN_IN;
                g.pln_src = (const i64 *)tmp;
            }
            if (mixed) {
                launch_inv_cols_mixed(S1, inv_polys, st, (i64 *)s, g, in, dp, (const i64 *)ipsi_br, ipsi_dp, (const i64 *)Ninv, 2,
                                      (const i64 *)ql, (const i64 *)qh, (const i64 *)kl, (const i64 *)kh);
                continue;
            }
            if (dp.n)
                launch_inv_cols<true>(S1, inv_polys, st, (i64 *)s, g, dp, (const i64 *)ipsi_br, ipsi_dp, (const i64 *)Ninv, 2,
                                      (const i64 *)ql, (const i64 *)qh, (const i64 *)kl, (const i64 *)kh);
            if (in.n)
                launch_inv_cols<false>(S1, inv_polys, st, (i64 *)s, g, in, (const i64 *)ipsi_br, ipsi_dp, (const i64 *)Ninv, 2,
                                       (const i64 *)ql, (const i64 *)qh, (const i64 *)kl, (const i64 *)kh);
            continue;
        }
        if (mixed) {
            const ClassLists cl = class_lists(in, dp, per_row2 * (unsigned)in.n);
            hipLaunchKernelGGL((ntt_inv_pass_mixed<true>), dim3((unsigned)cl.in_blocks + per_row2 * dp.n), dim3(NTT_THREADS), 0, st,
                               (const i64 *)s, (i64 *)s, g, cl, (const i64 *)ipsi_br, ipsi_dp, (const i64 *)Ninv,
                               pass == 1 ? 2 : TAIL_NONE, (const i64 *)ql, (const i64 *)qh, (const i64 *)kl, (const i64 *)kh);
            continue;
        }
        if (dp.n)
            hipLaunchKernelGGL((ntt_inv_pass_io<true, true>), dim3(per_row2 * dp.n), dim3(NTT_THREADS), 0, st, (const i64 *)s, (i64 *)s,
                               g, dp, (const i64 *)ipsi_br, ipsi_dp, (const i64 *)Ninv, pass == 1 ? 2 : TAIL_NONE,
                               (const i64 *)ql, (const i64 *)qh, (const i64 *)kl, (const i64 *)kh);
        if (in.n)
            hipLaunchKernelGGL((ntt_inv_pass_io<false, true>), dim3(per_row2 * in.n), dim3(NTT_THREADS), 0, st, (const i64 *)s, (i64 *)s,
                               g, in, (const i64 *)ipsi_br, ipsi_dp, (const i64 *)Ninv, pass == 1 ? 2 : TAIL_NONE,
                               (const i64 *)ql, (const i64 *)qh, (const i64 *)kl, (const i64 *)kh);
    }
    return (int)hipGetLastError();
}

// K3 + K4: inner product of the nparts extended digits with the key, inverse transform to canonical coefficients
int ks_tail(int nct, int nparts, int rows, int logN, const LfKeys &key, int64_t *tmp, int64_t *s, const LfInvTab &it, const LfMod &m,
            hipStream_t st, const RelinFold *fold = nullptr, bool presum = false) {
    if (!it.ipsi_dp || key.n != 1 || !lf_keys_ok(key) || (presum && !fold)) return LF_ERR_ARG;
    // the sums' planes pass through tmp: the digits are spent by then, and two digits or more leave room for 2 nct polynomials
    const KsSums ks = ks_sums(logN, rows, m.q_host, nct, tmp, ((int64_t)nct * nparts * rows) << logN);
    if (int e = ks.expect_digits(tmp, nct, nparts)) return e;
    // K3: inner product with the key, summed over the digits
    const i64 N = (i64)1 << logN;
    const RelinFold nofold{nullptr, 0, nullptr, 0, nullptr, 0};
    const bool planes = key.key_format == LF_KEY_PLANES;
    auto launch = [&](auto kernel, const RelinFold &f) {
        hipLaunchKernelGGL(kernel, ks.grid, dim3(256), 0, st, (const i64 *)tmp, (const i64 *)key.ksk[0], (i64)key.part_stride,
                           (i64)key.comp_stride, (i64)key.row_off, (i64 *)s, nparts, rows, N, f, ks.spl ? 1 : 0, LF_MOD_ARGS(m));
    };
    if (presum && nct == 1) {   // cc_dot: the fold reads a triplet already summed (one ciphertext)
        with_formats(planes, ks.dplanes, [&](auto PL, auto DPL) { launch(ks_inner2_presum_kernel<LF_CT(PL), LF_CT(DPL)>, *fold); });
    } else if (presum) {   // cc_dot_batch: nct summed triplets, fold->ct_stride apart
        if (!with_count<2, 4>(nct, [&](auto NCT) {
                with_formats(planes, ks.dplanes,
                             [&](auto PL, auto DPL) { launch(ks_dotb_inner_kernel<LF_CT(NCT), LF_CT(PL), LF_CT(DPL)>, *fold); });
            }))
            return LF_ERR_ARG;
    } else
        with_count<1, 2, 4>(nct, [&](auto NCT) {
            with_formats(planes, ks.dplanes, [&](auto PL, auto DPL) {
                if (fold) launch(ks_inner2_kernel<LF_CT(NCT), true, LF_CT(PL), LF_CT(DPL)>, *fold);
                else launch(ks_inner2_kernel<LF_CT(NCT), false, LF_CT(PL), LF_CT(DPL)>, nofold);
            });
        });
    // K4: inverse transform -> canonical coefficients (relaxed, tail 2), in place on s
    return ks_inv_sums(ks, (i64 *)tmp, (i64 *)s, it, m, st);
}

}  // namespace

// The launches of lf_cc_dot that are its own (ckks_ops.hip checks the arguments).
// lf_dot_tensor: the tensor products of g (1, 2 or 4) pairs' operand stacks x = [g][4][ell][N] (pair stride 4 ell N; xpl: fp64-class
// rows as planes) added into T = [3][ell][N] (first: written); t2 (may be NULL): a second copy of the new T2.
int lf_dot_tensor(int g, const int64_t *x, int64_t *T, int64_t *t2, int ell, int logN, int xpl, int first, const LfMod &m, hipStream_t st) {
    if ((g != 1 && g != 2 && g != 4) || !x || !T || ell < 1 || ell > 65535 || logN < 9) return LF_ERR_ARG;
    const i64 N = (i64)1 << logN;
    const dim3 grid((unsigned)(N / 512), (unsigned)ell);
#define LF_DOT_CASE(GG)                                                                                                 \
    case GG:                                                                                                            \
        hipLaunchKernelGGL((dot_tensor_kernel<GG>), grid, dim3(256), 0, st, (const i64 *)x, (i64)4 * ell * N, (i64 *)T, (i64 *)t2, ell, N, \
                           xpl, first, LF_MOD_ARGS(m));                                                                \
        break;
    switch (g) { LF_DOT_CASE(1) LF_DOT_CASE(2) LF_DOT_CASE(4) }
#undef LF_DOT_CASE
    return (int)hipGetLastError();
}

// The launches of lf_pc_dot that are its own (ckks_ops.hip checks the arguments).
// lf_pc_dot_products: the products of g (1, 2 or 4) terms' transformed pairs x = [g][2][rows][N] (xpl: fp64-class rows as planes)
// with their plaintexts pt[0 .. g), added into S = [2][rows][N] (first: written).
int lf_pc_dot_products(int g, const int64_t *x, const int64_t *const *pt, int64_t *S, int rows, int logN, int xpl, int first,
                       const LfMod &m, hipStream_t st) {
    if ((g != 1 && g != 2 && g != 4) || !x || !pt || !S || rows < 1 || rows > 65535 || logN < 9) return LF_ERR_ARG;
    const i64 N = (i64)1 << logN;
    PcTerms pa{};
    for (int i = 0; i < g; ++i) {
        if (!pt[i]) return LF_ERR_ARG;
        pa.pt[i] = (const i64 *)pt[i];
    }
    const dim3 grid((unsigned)(N / 512), (unsigned)rows);
#define LF_PCDOT_CASE(GG)                                                                                                         \
    case GG:                                                                                                                      \
        hipLaunchKernelGGL((pc_dot_kernel<GG>), grid, dim3(256), 0, st, (const i64 *)x, pa, (i64 *)S, rows, N, xpl, first,         \
                           LF_MOD_ARGS(m));                                                                                       \
        break;
    switch (g) { LF_PCDOT_CASE(1) LF_PCDOT_CASE(2) LF_PCDOT_CASE(4) }
#undef LF_PCDOT_CASE
    return (int)hipGetLastError();
}

// lf_pc_bias: c0 [rows][N] (canonical) <- mc_add's chain with the "add" plaintext pt, in place; constants of those rows.
int lf_pc_bias(int64_t *c0, const int64_t *pt, const int64_t *Rs, int rows, int logN, const LfMod &m, hipStream_t st) {
    if (!c0 || !pt || !Rs || rows < 1 || rows > 65535 || logN < 9) return LF_ERR_ARG;
    const i64 N = (i64)1 << logN;
    const dim3 grid((unsigned)(N / 512), (unsigned)rows);
    hipLaunchKernelGGL(pc_bias_kernel, grid, dim3(256), 0, st, (i64 *)c0, (const i64 *)pt, (const i64 *)Rs, N, LF_MOD_ARGS(m));
    return (int)hipGetLastError();
}

// The launches of lf_pc_matmul, lf_pc_matmul_batch and lf_pc_matmul_batch_planes that are their own (ckks_ops.hip checks the
// arguments).
// lf_pc_matmul_batch_tile: the tile of tokens (2 or 1; 4 under LF_TUNE_PC_MATMUL_TILE) one launch takes for `left` tokens still to
// go.  Every (go, gt) this can return is instantiated below for raw and for compact plaintexts (tests/test_pc_matmul_batch_cpu.py
// and tests/test_compact_plain_cpu.py hold each of them to scratch 0 and no spill).  Measured on MI355X: a tile
// of 4 tokens — 246 VGPRs at 4 outputs, 2 waves per SIMD — is slower than two tiles of 2, so the default never takes it.
static int g_pc_matmul_tile = 0;   // LF_TUNE_PC_MATMUL_TILE
int lf_pc_matmul_batch_tile(int go, int left) {
    (void)go;
    if (left >= 4 && g_pc_matmul_tile != 0) return 4;
    return left >= 2 ? 2 : 1;
}
// .. and the outputs (4, 2 or 1) a launch takes for `left` outputs still to go over nt tokens
int lf_pc_matmul_batch_outputs(int left, int nt) {
    if (left >= 4 && nt >= 4 && g_pc_matmul_tile == 2) return 2;
    return left >= 4 ? 4 : left >= 2 ? 2 : 1;
}

// lf_plain_planes_mask: bit r set where row r of a compact plaintext is fp64-class; false for more rows than the mask has bits
bool lf_plain_planes_mask(int rows, const int64_t *q_host, uint64_t *mask) {
    if (rows < 1 || rows > LF_PLAIN_PLANES_MAX_ROWS || !q_host) return false;
    uint64_t m = 0;
    for (int r = 0; r < rows; ++r)
        if ((uint64_t)q_host[r] < SMALL_PRIME_LIMIT) m |= 1ull << r;
    *mask = m;
    return true;
}

// lf_pc_matmul_products: go (1, 2 or 4) outputs over the n <= LF_PC_MATMUL_CI transformed pairs of each of gt (1, 2 or 4) tokens in
// one launch: token t's pairs [n][2][rows][N] at x + t * xtok (xpl: fp64-class rows as planes — refused where the library's note of
// that range says another format), its group's pairs [go][2][rows][N] of S at S + t * stok (first: written; otherwise added into);
// pt[i * pt_stride + g]: the plaintext of input i for output g, or NULL, shared by the tokens.  planes: every non-NULL pt a compact
// plaintext (lf_plain_planes) whose fp64-class rows `small` marks.  The token strides are in words, multiples of 2 (16-byte
// accesses); one token over raw plaintexts (pc_matmul_kernel) takes none, so there they are not looked at.
int lf_pc_matmul_products(bool planes, int go, int gt, int n, const int64_t *x, int64_t xtok, const int64_t *const *pt, int pt_stride,
                          int64_t *S, int64_t stok, int rows, int logN, int xpl, int first, uint64_t small, const LfMod &m, hipStream_t st) {
    if ((go != 1 && go != 2 && go != 4) || (gt != 1 && gt != 2 && gt != 4) || n < 1 || n > LF_PC_MATMUL_CI || !x || !pt || pt_stride < go ||
        !S || rows < 1 || rows > (planes ? LF_PLAIN_PLANES_MAX_ROWS : 65535) || logN < 9)
        return LF_ERR_ARG;
    if ((planes || gt > 1) &&
        (xtok < ((int64_t)2 * n * rows << logN) || stok < ((int64_t)2 * go * rows << logN) || (xtok & 1) || (stok & 1)))
        return LF_ERR_ARG;
    const i64 N = (i64)1 << logN;
    for (int t = 0; t < gt; ++t)
        if (int e = lf_fmt_expect(x + t * xtok, ((size_t)2 * n * rows << logN) * 8, xpl ? LF_FMT_PLANES : LF_FMT_RAW)) return e;
    PcMatTerms pa{};
    for (int i = 0; i < n; ++i)
        for (int g = 0; g < go; ++g) pa.pt[i][g] = (const i64 *)pt[(size_t)i * pt_stride + g];
    const dim3 grid((unsigned)(N / 512), (unsigned)rows);
#define LF_PCMM_CASE(GG)                                                                                                          \
    case GG * 8 + 1:                                                                                                              \
        hipLaunchKernelGGL((pc_matmul_kernel<GG>), grid, dim3(256), 0, st, (const i64 *)x, pa, (i64 *)S, n, rows, N, xpl, first,   \
                           LF_MOD_ARGS(m));                                                                                       \
        break;
#define LF_PCMMB_CASE(GG, TT)                                                                                                     \
    case GG * 8 + TT:                                                                                                             \
        hipLaunchKernelGGL((pc_matmulb_kernel<GG, TT>), grid, dim3(256), 0, st, (const i64 *)x, (i64)xtok, pa, (i64 *)S, (i64)stok, n, \
                           rows, N, xpl, first, LF_MOD_ARGS(m));                                                                  \
        break;
#define LF_PCPL_CASE(GG, TT)                                                                                                      \
    case 64 + GG * 8 + TT:                                                                                                        \
        hipLaunchKernelGGL((pc_planes_matmul_kernel<GG, TT>), grid, dim3(256), 0, st, (const i64 *)x, (i64)xtok, pa, (i64 *)S,     \
                           (i64)stok, n, rows, N, xpl, first, (unsigned long long)small, LF_MOD_ARGS(m));                          \
        break;
    switch ((planes ? 64 : 0) + go * 8 + gt) {
        LF_PCMM_CASE(1) LF_PCMM_CASE(2) LF_PCMM_CASE(4)
        LF_PCMMB_CASE(1, 2) LF_PCMMB_CASE(2, 2) LF_PCMMB_CASE(4, 2) LF_PCMMB_CASE(1, 4) LF_PCMMB_CASE(2, 4) LF_PCMMB_CASE(4, 4)
        LF_PCPL_CASE(1, 1) LF_PCPL_CASE(2, 1) LF_PCPL_CASE(4, 1) LF_PCPL_CASE(1, 2) LF_PCPL_CASE(2, 2) LF_PCPL_CASE(4, 2)
        LF_PCPL_CASE(1, 4) LF_PCPL_CASE(2, 4) LF_PCPL_CASE(4, 4)
    }
#undef LF_PCMM_CASE
#undef LF_PCMMB_CASE
#undef LF_PCPL_CASE
    return (int)hipGetLastError();
}

// The launch of lf_cc_matmul that is its own (ckks_ops.hip checks the arguments).
// lf_matmul_tensor: the summed triplets of an R x C tile (R C = 1, 2 or 4) over the inner dimension k <= LF_CC_MATMUL_MAX_INNER from the
// store x = [nu][2][ell][N] of transformed operands (xpl: fp64-class rows as planes — refused where the library's note of that range
// says another format); ta[t * R + i] / tb[t * C + j]: the operand of row i / column j of the tile at inner index t, in 0 .. nu - 1,
// or -1; written to T = [R C][3][ell][N], the T2 copies to t2 = [R C][ell][N].
int lf_matmul_tensor(int R, int C, int k, int nu, const int64_t *x, const int *ta, const int *tb, int64_t *T, int64_t *t2, int ell,
                     int logN, int xpl, const LfMod &m, hipStream_t st) {
    if (R < 1 || C < 1 || R > 4 || C > 4 || (R * C != 1 && R * C != 2 && R * C != 4) || (R > 1 && C > 1 && R != C) || k < 1 ||
        k > LF_CC_MATMUL_MAX_INNER || nu < 1 || nu > LF_CC_MATMUL_MAX_OPERANDS || !x || !ta || !tb || !T || !t2 || ell < 1 || ell > 65535 ||
        logN < 9)
        return LF_ERR_ARG;
    const i64 N = (i64)1 << logN;
    if (int e = lf_fmt_expect(x, ((size_t)2 * nu * ell << logN) * 8, xpl ? LF_FMT_PLANES : LF_FMT_RAW)) return e;
    MatmulIdx ix{};
    for (int t = 0; t < k; ++t) {
        for (int i = 0; i < 4; ++i) ix.a[t][i] = ix.b[t][i] = -1;
        for (int i = 0; i < R; ++i) {
            if (ta[t * R + i] < -1 || ta[t * R + i] >= nu) return LF_ERR_ARG;
            ix.a[t][i] = (short)ta[t * R + i];
        }
        for (int j = 0; j < C; ++j) {
            if (tb[t * C + j] < -1 || tb[t * C + j] >= nu) return LF_ERR_ARG;
            ix.b[t][j] = (short)tb[t * C + j];
        }
    }
    const dim3 grid((unsigned)(N / 512), (unsigned)ell);
#define LF_MM_LAUNCH(RR, CC)                                                                                                      \
    hipLaunchKernelGGL((matmul_tensor_kernel<RR, CC>), grid, dim3(256), 0, st, (const i64 *)x, ix, k, (i64 *)T, (i64 *)t2, ell, N, xpl, \
                       LF_MOD_ARGS(m))
    switch (R * 8 + C) {
        case 1 * 8 + 1: LF_MM_LAUNCH(1, 1); break;
        case 1 * 8 + 2: LF_MM_LAUNCH(1, 2); break;
        case 2 * 8 + 1: LF_MM_LAUNCH(2, 1); break;
        case 1 * 8 + 4: LF_MM_LAUNCH(1, 4); break;
        case 4 * 8 + 1: LF_MM_LAUNCH(4, 1); break;
        case 2 * 8 + 2: LF_MM_LAUNCH(2, 2); break;
        default: return LF_ERR_ARG;
    }
#undef LF_MM_LAUNCH
    return (int)hipGetLastError();
}

// lf_dot_relin: lf_relin_core_batch whose fold reads nct (1, 2 or 4) summed triplets T + t * 3 ell N instead of operand stacks: the
// digits of triplet t at state + t * ell N are those of its T2's inverse transform; the (digit, own limb) pairs are not extended,
// the inner product takes T2's words for them; the sums s [nct][2][rows][N] receive P T0 and P T1 on the ordinary rows.  ONE
// extension + forward NTT of all digits, ONE launch of the inner product (every key word read once for the nct triplets), ONE
// inverse NTT of the 2 nct sums.  Internal: ckks_ops.hip checks the arguments.
int lf_dot_relin(const int64_t *state, int nct, int nparts, int rows, int logN, const int64_t *desc, const int64_t *E, const double *Ed,
                 const LfKeys &key, int64_t *tmp, int64_t *s, const LfFwdTab &ft, const LfInvTab &it, const int64_t *T, const int64_t *PR,
                 int ell, const uint8_t *own, const LfMod &m, hipStream_t st) {
    if ((nct != 1 && nct != 2 && nct != 4) || nparts < 1 || nparts > 254 || rows < 1 || rows > MAX_LIST_ROWS || logN <= NTT_TILE_LOG_MAX ||
        logN > KS_LOGN_MAX || !m.q_host || !ft.psi_dp || !it.ipsi_dp || !Ed || !T || !PR || ell < 0 || ell > rows)
        return LF_ERR_ARG;
    if (!lf_fp64_digits_ok(nparts, rows, m.q_host)) return LF_ERR_ARG;
    const int64_t poly = nct > 1 ? (int64_t)ell << logN : 0;   // (one triplet: no stride)
    if (int e = ks_forward(state, poly, nct, nparts, rows, logN, desc, E, Ed, tmp, ft, m, st, (const unsigned char *)own, 0)) return e;
    const RelinFold fold{(const i64 *)T, (i64)(3 * poly), (const i64 *)PR, ell, (const unsigned char *)own, 0};
    return ks_tail(nct, nparts, rows, logN, key, tmp, s, it, m, st, &fold, true);
}

namespace {
// what the launchers of the gathered inner products refuse alike: the tables, the keys, the rows, the digits' count for fp64 rows
bool gathered_args_ok(const LfKeys &key, const int64_t *p_host, int nparts, int rows, const LfInvTab *it, const LfMod &m) {
    if ((it && !it->ipsi_dp) || !lf_keys_ok(key) || (key.n && !p_host)) return false;
    return rows >= 1 && rows <= MAX_LIST_ROWS && lf_fp64_digits_ok(nparts, rows, m.q_host);
}
}  // namespace

// The key-dependent half of key.n (1, 2 or 4) hoisted rotations of ONE ciphertext (lf_rotate_hoisted, ckks_ops.hip): inner product of
// the extended digits `ext` [nparts][rows][N] (lf_ks_fwd) gathered by pi_{p_i} with key i, then the inverse transform of the
// 2 n sums s [n][2][rows][N].  `ext` is only read, so it serves every group; the sums' planes pass through `scratch`
// (scratch_words >= 2 n rows N, else the sums stay raw words: same outputs).  Internal: ckks_ops.hip checks the arguments.
int lf_ks_tail_hoisted(const int64_t *p_host, int nparts, int rows, int logN, const LfKeys &key, const int64_t *ext, int64_t *s,
                       int64_t *scratch, int64_t scratch_words, const LfInvTab &it, const LfMod &m, hipStream_t st) {
    const int nr = key.n;
    if ((nr != 1 && nr != 2 && nr != 4) || !gathered_args_ok(key, p_host, nparts, rows, &it, m)) return LF_ERR_ARG;
    const KsSums ks = ks_sums(logN, rows, m.q_host, nr, scratch, scratch_words);
    if (int e = ks.expect_digits(ext, 1, nparts)) return e;
    const HoistKeys hk = hoist_keys(key, p_host, 0, nr);
    with_count<1, 2, 4>(nr, [&](auto NR) {
        with_formats(key.key_format == LF_KEY_PLANES, ks.dplanes, [&](auto PL, auto DPL) {
            hipLaunchKernelGGL((ks_inner_hoist_kernel<LF_CT(NR), LF_CT(PL), LF_CT(DPL)>), ks.grid, dim3(256), 0, st, (const i64 *)ext, hk,
                               (i64)key.part_stride, (i64)key.comp_stride, (i64)key.row_off, (i64 *)s, nparts, rows, logN, ks.spl ? 1 : 0,
                               LF_MOD_ARGS(m));
        });
    });
    return ks_inv_sums(ks, (i64 *)scratch, (i64 *)s, it, m, st);
}

// The key-dependent part of lf_linear_transform (ckks_ops.hip): per group of up to 4 keys (key_group) ONE launch of
// ks_inner_lt_kernel over the shared extended digits `ext` (no keys: the step-0 term alone, one launch without keys), all of them
// adding into the one pair of sums s [2][rows][N]; then the inverse transform of that pair.  `scratch` (>= 2 rows N words, or
// NULL: the sums stay raw words, same outputs) carries the sums' planes through the tiled inverse pass; it may be `ext` itself,
// which is spent once the last group has read it.  chat = P NTT(c0), P NTT(c1) on the `ell` ordinary rows.  Internal:
// ckks_ops.hip checks the arguments (odd exponents below 2N, pt0 != NULL without keys).
int lf_ks_tail_lt(const int64_t *p_host, int nparts, int rows, int ell, int logN, const LfKeys &key, const int64_t *pt, int64_t pt_stride,
                  const int64_t *pt0, const int64_t *chat, const int64_t *ext, int64_t *s, int64_t *scratch, int64_t scratch_words,
                  const LfInvTab &it, const LfMod &m, hipStream_t st) {
    const int nr = key.n;
    if (!gathered_args_ok(key, p_host, nparts, rows, &it, m) || (nr == 0 && !pt0) || (nr && !pt) || !chat || ell < 0 || ell > rows)
        return LF_ERR_ARG;
    const KsSums ks = ks_sums(logN, rows, m.q_host, 1, scratch, scratch_words);
    if (nr)   // (without keys nothing reads the digits)
        if (int e = ks.expect_digits(ext, 1, nparts)) return e;
    for (int i0 = 0; i0 < nr || i0 == 0;) {
        const int g = key_group(nr - i0);
        LtArgs la{};
        la.hk = hoist_keys(key, p_host, i0, g);
        for (int t = 0; t < g; ++t) la.pt[t] = (const i64 *)pt + (i64)(i0 + t) * pt_stride;
        la.pt0 = (const i64 *)pt0, la.chat = (const i64 *)chat, la.ell = ell, la.first = i0 == 0;
        auto launch = [&](auto NR, auto PL, auto DPL) {
            hipLaunchKernelGGL((ks_inner_lt_kernel<LF_CT(NR), LF_CT(PL), LF_CT(DPL)>), ks.grid, dim3(256), 0, st, (const i64 *)ext, la,
                               (i64)key.part_stride, (i64)key.comp_stride, (i64)key.row_off, (i64 *)s, nparts, rows, logN, ks.spl ? 1 : 0,
                               LF_MOD_ARGS(m));
        };
        if (!g) launch(std::integral_constant<int, 0>{}, std::false_type{}, std::false_type{});   // (no key: no format to tell apart)
        with_count<1, 2, 4>(g, [&](auto NR) {
            with_formats(key.key_format == LF_KEY_PLANES, ks.dplanes, [&](auto PL, auto DPL) { launch(NR, PL, DPL); });
        });
        i0 += g ? g : 1;
    }
    return ks_inv_sums(ks, (i64 *)scratch, (i64 *)s, it, m, st);
}

// The key-dependent part of lf_linear_transform_batch (ckks_ops.hip) for nct (2 or 4) ciphertexts: per LF_LTB_KEYS keys ONE launch
// of ks_inner_ltb_kernel over the ciphertexts' extended digits ext [nct][nparts][rows][N] (no keys: the step-0 term alone, one
// launch without keys), all of them adding into the nct pairs of sums s [nct][2][rows][N]; then ONE inverse transform of the
// 2 nct polynomials.  `scratch` (>= 2 nct rows N words, or NULL: the sums stay raw words, same outputs) as in lf_ks_tail_lt.
// Ciphertext t's c^ = P NTT(c0), P NTT(c1) on the `ell` ordinary rows at chat + t * chat_stride.  Internal: ckks_ops.hip checks
// the arguments (odd exponents below 2N, pt0 != NULL without keys).
int lf_ks_tail_ltb(int nct, const int64_t *p_host, int nparts, int rows, int ell, int logN, const LfKeys &key, const int64_t *pt,
                   int64_t pt_stride, const int64_t *pt0, const int64_t *chat, int64_t chat_stride, const int64_t *ext, int64_t *s,
                   int64_t *scratch, int64_t scratch_words, const LfInvTab &it, const LfMod &m, hipStream_t st) {
    const int nr = key.n;
    if ((nct != 2 && nct != 4) || !gathered_args_ok(key, p_host, nparts, rows, &it, m) || (nr == 0 && !pt0) || (nr && !pt) || !chat ||
        !ext || !s || ell < 0 || ell > rows || nparts < 1 || logN <= NTT_TILE_LOG_MAX || logN > KS_LOGN_MAX)
        return LF_ERR_ARG;
    const KsSums ks = ks_sums(logN, rows, m.q_host, nct, scratch, scratch_words);
    if (nr)
        if (int e = ks.expect_digits(ext, nct, nparts)) return e;
    for (int i0 = 0; i0 < nr || i0 == 0; i0 += LF_LTB_KEYS) {
        const int g = nr - i0 < LF_LTB_KEYS ? nr - i0 : LF_LTB_KEYS;
        LtbArgs la{};
        for (int t = 0; t < g; ++t) {
            la.ksk[t] = (const i64 *)key.ksk[i0 + t];
            la.p[t] = (unsigned)p_host[i0 + t];
            la.pt[t] = (const i64 *)pt + (i64)(i0 + t) * pt_stride;
        }
        la.pt0 = (const i64 *)pt0, la.chat = (const i64 *)chat, la.chat_stride = (i64)chat_stride;
        la.ext_stride = ((i64)nparts * rows) << logN, la.sum_stride = ((i64)2 * rows) << logN;
        la.nk = g, la.ell = ell, la.first = i0 == 0;
        with_count<2, 4>(nct, [&](auto NCT) {
            with_formats(key.key_format == LF_KEY_PLANES, ks.dplanes, [&](auto PL, auto DPL) {
                hipLaunchKernelGGL((ks_inner_ltb_kernel<LF_CT(NCT), 1, LF_CT(PL), LF_CT(DPL)>), ks.grid, dim3(256), 0, st, (const i64 *)ext,
                                   la, (i64)key.part_stride, (i64)key.comp_stride, (i64)key.row_off, (i64 *)s, nparts, rows, logN,
                                   ks.spl ? 1 : 0, LF_MOD_ARGS(m));
            });
        });
    }
    return ks_inv_sums(ks, (i64 *)scratch, (i64 *)s, it, m, st);
}

// The key-dependent part of lf_rotate_sum (ckks_ops.hip): per group of up to 4 keys (key_group) ONE launch of ks_inner_rsum_kernel
// over the shared extended digits `ext` (no keys: the self term alone, one launch without keys), all of them adding into the one
// pair of sums s [2][rows][N]; then the inverse transform of that pair.  `scratch` as in lf_ks_tail_lt.  chat = P NTT(c0),
// P NTT(c1) on the `ell` ordinary rows (c1 only with `with_self`).  Internal: ckks_ops.hip checks the arguments (odd exponents
// below 2N, with_self without keys).
int lf_ks_tail_rsum(const int64_t *p_host, int nparts, int rows, int ell, int logN, const LfKeys &key, int with_self, const int64_t *chat,
                    const int64_t *ext, int64_t *s, int64_t *scratch, int64_t scratch_words, const LfInvTab &it, const LfMod &m,
                    hipStream_t st) {
    const int nr = key.n;
    if (!gathered_args_ok(key, p_host, nparts, rows, &it, m) || (nr == 0 && !with_self) || !chat || ell < 0 || ell > rows) return LF_ERR_ARG;
    const KsSums ks = ks_sums(logN, rows, m.q_host, 1, scratch, scratch_words);
    if (nr)
        if (int e = ks.expect_digits(ext, 1, nparts)) return e;
    for (int i0 = 0; i0 < nr || i0 == 0;) {
        const int g = key_group(nr - i0);
        RsumArgs ra{};
        ra.hk = hoist_keys(key, p_host, i0, g);
        ra.chat = (const i64 *)chat, ra.ell = ell, ra.first = i0 == 0, ra.self = with_self ? 1 : 0;
        auto launch = [&](auto NR, auto PL, auto DPL) {
            hipLaunchKernelGGL((ks_inner_rsum_kernel<LF_CT(NR), LF_CT(PL), LF_CT(DPL)>), ks.grid, dim3(256), 0, st, (const i64 *)ext, ra,
                               (i64)key.part_stride, (i64)key.comp_stride, (i64)key.row_off, (i64 *)s, nparts, rows, logN, ks.spl ? 1 : 0,
                               LF_MOD_ARGS(m));
        };
        if (!g) launch(std::integral_constant<int, 0>{}, std::false_type{}, std::false_type{});
        with_count<1, 2, 4>(g, [&](auto NR) {
            with_formats(key.key_format == LF_KEY_PLANES, ks.dplanes, [&](auto PL, auto DPL) { launch(NR, PL, DPL); });
        });
        i0 += g ? g : 1;
    }
    return ks_inv_sums(ks, (i64 *)scratch, (i64 *)s, it, m, st);
}

// The key-dependent part of lf_rotate_sum_batch (ckks_ops.hip) for nct (2 or 4) ciphertexts: per LF_RSB_KEYS keys ONE launch of
// ks_inner_rsumb_kernel over the ciphertexts' extended digits ext [nct][nparts][rows][N] (no keys: the self term alone, one launch
// without keys), all of them adding into the nct pairs of sums s [nct][2][rows][N]; then ONE inverse transform of the 2 nct
// polynomials.  `scratch` (>= 2 nct rows N words, or NULL: the sums stay raw words, same outputs) as in lf_ks_tail_lt.
// Ciphertext t's c^ = P NTT(c0), P NTT(c1) on the `ell` ordinary rows at chat + t * chat_stride (c1 only with `with_self`).
// Internal: ckks_ops.hip checks the arguments (odd exponents below 2N, with_self without keys).
int lf_ks_tail_rsumb(int nct, const int64_t *p_host, int nparts, int rows, int ell, int logN, const LfKeys &key, int with_self,
                     const int64_t *chat, int64_t chat_stride, const int64_t *ext, int64_t *s, int64_t *scratch, int64_t scratch_words,
                     const LfInvTab &it, const LfMod &m, hipStream_t st) {
    const int nr = key.n;
    if ((nct != 2 && nct != 4) || !gathered_args_ok(key, p_host, nparts, rows, &it, m) || (nr == 0 && !with_self) || !chat || !ext || !s ||
        ell < 0 || ell > rows || nparts < 1 || logN <= NTT_TILE_LOG_MAX || logN > KS_LOGN_MAX)
        return LF_ERR_ARG;
    const KsSums ks = ks_sums(logN, rows, m.q_host, nct, scratch, scratch_words);
    if (nr)
        if (int e = ks.expect_digits(ext, nct, nparts)) return e;
    for (int i0 = 0; i0 < nr || i0 == 0; i0 += LF_RSB_KEYS) {
        const int g = nr - i0 < LF_RSB_KEYS ? nr - i0 : LF_RSB_KEYS;
        RsbArgs ra{};
        for (int t = 0; t < g; ++t) {
            ra.ksk[t] = (const i64 *)key.ksk[i0 + t];
            ra.p[t] = (unsigned)p_host[i0 + t];
        }
        ra.chat = (const i64 *)chat, ra.chat_stride = (i64)chat_stride;
        ra.ext_stride = ((i64)nparts * rows) << logN, ra.sum_stride = ((i64)2 * rows) << logN;
        ra.nk = g, ra.ell = ell, ra.first = i0 == 0, ra.self = with_self ? 1 : 0;
        with_count<2, 4>(nct, [&](auto NCT) {
            with_formats(key.key_format == LF_KEY_PLANES, ks.dplanes, [&](auto PL, auto DPL) {
                hipLaunchKernelGGL((ks_inner_rsumb_kernel<LF_CT(NCT), LF_CT(PL), LF_CT(DPL)>), ks.grid, dim3(256), 0, st, (const i64 *)ext,
                                   ra, (i64)key.part_stride, (i64)key.comp_stride, (i64)key.row_off, (i64 *)s, nparts, rows, logN,
                                   ks.spl ? 1 : 0, LF_MOD_ARGS(m));
            });
        });
    }
    return ks_inv_sums(ks, (i64 *)scratch, (i64 *)s, it, m, st);
}

// ---- the launches of lf_linear_transform_bsgs (ckks_ops.hip checks the arguments and owns the order) ----
// baby steps: key i's gathered sums over the shared digits `ext`, + chat0 gathered on the ordinary rows, into u + i * 2 rows N
int lf_ks_baby_sums(const int64_t *p_host, int nparts, int rows, int ell, int logN, const LfKeys &key, const int64_t *chat0,
                    const int64_t *ext, int64_t *u, const LfMod &m, hipStream_t st) {
    const int nr = key.n;
    if (!gathered_args_ok(key, p_host, nparts, rows, nullptr, m) || !chat0 || !u || ell < 0 || ell > rows) return LF_ERR_ARG;
    if (!nr) return 0;
    const KsSums ks = ks_sums(logN, rows, m.q_host, 0, nullptr, 0);
    if (int e = ks.expect_digits(ext, 1, nparts)) return e;
    const i64 pair = (i64)2 * rows << logN;
    for (int i0 = 0; i0 < nr;) {
        const int g = key_group(nr - i0);
        BabyArgs ba{};
        ba.hk = hoist_keys(key, p_host, i0, g);
        for (int t = 0; t < g; ++t) ba.u[t] = (i64 *)u + (i64)(i0 + t) * pair;
        ba.chat0 = (const i64 *)chat0, ba.ell = ell;
        with_count<1, 2, 4>(g, [&](auto NR) {
            with_formats(key.key_format == LF_KEY_PLANES, ks.dplanes, [&](auto PL, auto DPL) {
                hipLaunchKernelGGL((ks_inner_baby_kernel<LF_CT(NR), LF_CT(PL), LF_CT(DPL)>), ks.grid, dim3(256), 0, st, (const i64 *)ext, ba,
                                   (i64)key.part_stride, (i64)key.comp_stride, (i64)key.row_off, nparts, rows, logN, LF_MOD_ARGS(m));
            });
        });
        i0 += g;
    }
    return (int)hipGetLastError();
}

// diagonal products of ng (1, 2 or 4) giant steps: out[i] = sum over the set bits t of slots[i] of pt[i][k-th diagonal] * u[t]
int lf_lt_diag_products(int ng, const int64_t *u, int nslots, const int64_t *const *pt, const unsigned long long *slots, int64_t pt_stride,
                        int64_t *const *out, int rows, int logN, const LfMod &m, hipStream_t st) {
    if ((ng != 1 && ng != 2 && ng != 4) || !u || nslots < 1 || nslots > 64) return LF_ERR_ARG;
    DiagArgs da{};
    da.u = (const i64 *)u, da.pt_stride = (i64)pt_stride, da.nslots = nslots;
    for (int i = 0; i < ng; ++i) {
        if (!pt[i] || !out[i] || !slots[i]) return LF_ERR_ARG;
        da.pt[i] = (const i64 *)pt[i], da.slots[i] = slots[i], da.out[i] = (i64 *)out[i];
    }
    const dim3 grid((unsigned)((((i64)1 << logN) + 511) / 512), (unsigned)rows);
#define LF_DIAG_LAUNCH(NG)                                                                                                 \
    hipLaunchKernelGGL((lt_diag_products_kernel<NG>), grid, dim3(256), 0, st, da, rows, logN, LF_MOD_ARGS(m))
    switch (ng) {
        case 1: LF_DIAG_LAUNCH(1); break;
        case 2: LF_DIAG_LAUNCH(2); break;
        case 4: LF_DIAG_LAUNCH(4); break;
    }
#undef LF_DIAG_LAUNCH
    return (int)hipGetLastError();
}

// ---- the launch of lf_lt_matmul that is its own (ckks_ops.hip checks the arguments and owns the order) ----
// block products of no (1, 2 or 4) outputs over one input's pairs u: out[i] (+)= sum over the set bits t of slots[i] of
// pt[i][k-th diagonal] * u[t]; fresh[i] != 0 writes out[i], 0 adds to it
int lf_lt_block_products(int no, const int64_t *u, int nslots, const int64_t *const *pt, const unsigned long long *slots,
                         const int64_t *pt_stride, int64_t *const *out, const int *fresh, int rows, int logN, const LfMod &m,
                         hipStream_t st) {
    if ((no != 1 && no != 2 && no != 4) || !u || nslots < 1 || nslots > 64 || rows < 1 || rows > 65535) return LF_ERR_ARG;
    BlockArgs ba{};
    ba.u = (const i64 *)u, ba.nslots = nslots;
    for (int i = 0; i < no; ++i) {
        if (!pt[i] || !out[i] || !slots[i] || (nslots < 64 && (slots[i] >> nslots))) return LF_ERR_ARG;
        ba.pt[i] = (const i64 *)pt[i], ba.slots[i] = slots[i], ba.out[i] = (i64 *)out[i], ba.pt_stride[i] = (i64)pt_stride[i];
        ba.fresh[i] = fresh[i];
    }
    const dim3 grid((unsigned)((((i64)1 << logN) + 511) / 512), (unsigned)rows);
#define LF_BLOCK_LAUNCH(NO)                                                                                                 \
    hipLaunchKernelGGL((lt_block_products_kernel<NO>), grid, dim3(256), 0, st, ba, rows, logN, LF_MOD_ARGS(m))
    switch (no) {
        case 1: LF_BLOCK_LAUNCH(1); break;
        case 2: LF_BLOCK_LAUNCH(2); break;
        case 4: LF_BLOCK_LAUNCH(4); break;
    }
#undef LF_BLOCK_LAUNCH
    return (int)hipGetLastError();
}

// ---- the launch of lf_lt_matmul_batch that is its own ----
// lf_lt_block_products for nt (2 or 4) tokens that share the blocks: token k reads u + k * u_tstride and writes (or adds to)
// out[i] + k * out_tstride.  One launch of lt_block_productsb_kernel<no, 2> per tile of 2 tokens: a diagonal word is read once per tile
int lf_lt_block_productsb(int nt, int no, const int64_t *u, int64_t u_tstride, int nslots, const int64_t *const *pt,
                          const unsigned long long *slots, const int64_t *pt_stride, int64_t *const *out, int64_t out_tstride,
                          const int *fresh, int rows, int logN, const LfMod &m, hipStream_t st) {
    if ((nt != 2 && nt != 4) || (no != 1 && no != 2 && no != 4) || !u || nslots < 1 || nslots > 64 || rows < 1 || rows > 65535)
        return LF_ERR_ARG;
    const int64_t pair = (2 * (int64_t)rows) << logN;
    if (u_tstride < nslots * pair || out_tstride < pair) return LF_ERR_ARG;   // (the tokens' pairs and sums do not overlap)
    BlockArgs ba{};
    ba.nslots = nslots, ba.u_tstride = (i64)u_tstride, ba.out_tstride = (i64)out_tstride;
    for (int i = 0; i < no; ++i) {
        if (!pt[i] || !out[i] || !slots[i] || (nslots < 64 && (slots[i] >> nslots))) return LF_ERR_ARG;
        ba.pt[i] = (const i64 *)pt[i], ba.slots[i] = slots[i], ba.pt_stride[i] = (i64)pt_stride[i], ba.fresh[i] = fresh[i];
    }
    const dim3 grid((unsigned)((((i64)1 << logN) + 511) / 512), (unsigned)rows);
#define LF_BLOCKB_LAUNCH(NO)                                                                                                    \
    hipLaunchKernelGGL((lt_block_productsb_kernel<NO, 2>), grid, dim3(256), 0, st, ba, rows, logN, LF_MOD_ARGS(m))
    for (int t0 = 0; t0 < nt; t0 += 2) {
        ba.u = (const i64 *)u + t0 * u_tstride;
        for (int i = 0; i < no; ++i) ba.out[i] = (i64 *)out[i] + t0 * out_tstride;
        switch (no) {
            case 1: LF_BLOCKB_LAUNCH(1); break;
            case 2: LF_BLOCKB_LAUNCH(2); break;
            case 4: LF_BLOCKB_LAUNCH(4); break;
        }
    }
#undef LF_BLOCKB_LAUNCH
    return (int)hipGetLastError();
}

// giant step: acc += (sum over the parts of `ext` gathered by pi_p times the key part, + s0 gathered on all rows on component 0)
int lf_ks_giant_sums(int64_t p, int nparts, int rows, int logN, const LfKeys &key, const int64_t *ext, const int64_t *s0, int64_t *acc,
                     const LfMod &m, hipStream_t st) {
    if (key.n != 1 || !gathered_args_ok(key, &p, nparts, rows, nullptr, m) || !s0 || !acc) return LF_ERR_ARG;
    const KsSums ks = ks_sums(logN, rows, m.q_host, 0, nullptr, 0);
    if (int e = ks.expect_digits(ext, 1, nparts)) return e;
    GiantArgs ga{};
    ga.hk = hoist_keys(key, &p, 0, 1), ga.s0 = (const i64 *)s0, ga.acc = (i64 *)acc;
    with_formats(key.key_format == LF_KEY_PLANES, ks.dplanes, [&](auto PL, auto DPL) {
        hipLaunchKernelGGL((ks_inner_giant_kernel<LF_CT(PL), LF_CT(DPL)>), ks.grid, dim3(256), 0, st, (const i64 *)ext, ga,
                           (i64)key.part_stride, (i64)key.comp_stride, (i64)key.row_off, nparts, rows, logN, LF_MOD_ARGS(m));
    });
    return (int)hipGetLastError();
}

// ---- the launches of lf_lt_matmul_bsgs that are its own (ckks_ops.hip checks the arguments and owns the order) ----
// extension + forward NTT of the digits of nct polynomials (state + t * state_stride) into tmp [nct][nparts][rows][N]
int lf_ks_fwd_batch(const int64_t *state, int64_t state_stride, int nct, int nparts, int rows, int logN, const int64_t *desc,
                    const int64_t *E, const double *Ed, int64_t *tmp, const LfFwdTab &ft, const LfMod &m, hipStream_t st) {
    if ((nct != 2 && nct != 4) || nparts < 1 || rows < 1 || rows > MAX_LIST_ROWS || logN <= NTT_TILE_LOG_MAX || logN > KS_LOGN_MAX ||
        !m.q_host || !ft.psi_dp || !Ed || !state || !tmp)
        return LF_ERR_ARG;
    return ks_forward(state, state_stride, nct, nparts, rows, logN, desc, E, Ed, tmp, ft, m, st);
}

namespace {
// what the two launchers of nct (2 or 4) ciphertexts under ONE key refuse alike; dst: the nct pairs they write or add to
bool one_key_batch_ok(int nct, int64_t p, int nparts, int rows, int logN, const LfKeys &key, const int64_t *ext,
                      const int64_t *const *src, int64_t *const *dst, const LfMod &m) {
    if ((nct != 2 && nct != 4) || key.n != 1 || !gathered_args_ok(key, &p, nparts, rows, nullptr, m) || !ext || !src || !dst || nparts < 1 ||
        logN <= NTT_TILE_LOG_MAX || logN > KS_LOGN_MAX || !lf_exponents_ok(&p, 1, logN))
        return false;
    for (int t = 0; t < nct; ++t) {
        if (!src[t] || !dst[t]) return false;
        for (int k = 0; k < t; ++k)
            if (dst[k] == dst[t]) return false;   // (two ciphertexts of one launch never share a pair or an accumulator)
    }
    return true;
}
}  // namespace

// giant step of nct (2 or 4) outputs under one key: acc[t] += (sum over the parts of output t's digits ext + t * nparts rows N
// gathered by pi_p times the key part, + s0[t] gathered on all rows on component 0); every key word is read once for the group
int lf_ks_giant_sums_batch(int nct, int64_t p, int nparts, int rows, int logN, const LfKeys &key, const int64_t *ext,
                           const int64_t *const *s0, int64_t *const *acc, const LfMod &m, hipStream_t st) {
    if (!one_key_batch_ok(nct, p, nparts, rows, logN, key, ext, s0, acc, m)) return LF_ERR_ARG;
    const KsSums ks = ks_sums(logN, rows, m.q_host, 0, nullptr, 0);
    if (int e = ks.expect_digits(ext, nct, nparts)) return e;
    GiantBatchArgs ga{};
    ga.ksk = (const i64 *)key.ksk[0], ga.p = (unsigned)p, ga.ext_stride = ((i64)nparts * rows) << logN;
    for (int t = 0; t < nct; ++t) ga.s0[t] = (const i64 *)s0[t], ga.acc[t] = (i64 *)acc[t];
    with_count<2, 4>(nct, [&](auto NCT) {
        with_formats(key.key_format == LF_KEY_PLANES, ks.dplanes, [&](auto PL, auto DPL) {
            hipLaunchKernelGGL((ks_inner_giantb_kernel<LF_CT(NCT), LF_CT(PL), LF_CT(DPL)>), ks.grid, dim3(256), 0, st, (const i64 *)ext, ga,
                               (i64)key.part_stride, (i64)key.comp_stride, (i64)key.row_off, nparts, rows, logN, LF_MOD_ARGS(m));
        });
    });
    return (int)hipGetLastError();
}

// ---- the launch of lf_linear_transform_bsgs_batch that is its own (ckks_ops.hip checks the arguments and owns the order) ----
// baby step of nct (2 or 4) ciphertexts under one key: u[t] = the sum over the parts of ciphertext t's digits ext + t * nparts rows N
// gathered by pi_p times the key part, + chat0[t] gathered on the ordinary rows on component 0; every key word is read once for
// the group
int lf_ks_baby_sums_batch(int nct, int64_t p, int nparts, int rows, int ell, int logN, const LfKeys &key, const int64_t *ext,
                          const int64_t *const *chat0, int64_t *const *u, const LfMod &m, hipStream_t st) {
    if (!one_key_batch_ok(nct, p, nparts, rows, logN, key, ext, chat0, u, m) || ell < 0 || ell > rows) return LF_ERR_ARG;
    const KsSums ks = ks_sums(logN, rows, m.q_host, 0, nullptr, 0);
    if (int e = ks.expect_digits(ext, nct, nparts)) return e;
    BabyBatchArgs ba{};
    ba.ksk = (const i64 *)key.ksk[0], ba.p = (unsigned)p, ba.ell = ell, ba.ext_stride = ((i64)nparts * rows) << logN;
    for (int t = 0; t < nct; ++t) ba.chat0[t] = (const i64 *)chat0[t], ba.u[t] = (i64 *)u[t];
    with_count<2, 4>(nct, [&](auto NCT) {
        with_formats(key.key_format == LF_KEY_PLANES, ks.dplanes, [&](auto PL, auto DPL) {
            hipLaunchKernelGGL((ks_inner_babyb_kernel<LF_CT(NCT), LF_CT(PL), LF_CT(DPL)>), ks.grid, dim3(256), 0, st, (const i64 *)ext, ba,
                               (i64)key.part_stride, (i64)key.comp_stride, (i64)key.row_off, nparts, rows, logN, LF_MOD_ARGS(m));
        });
    });
    return (int)hipGetLastError();
}

// cc_mult's product -> digits in one launch behind the tiled pass where it qualifies (ckks_ops.hip: product_digits): 0 = never
int lf_g_intt_digits = 1;

extern "C" {

int lf_tune(int which, int value) {
    int *knob = which == LF_TUNE_KS_EXT_COLS_MAX ? &g_ks_ext_cols_max : which == LF_TUNE_INTT_DIGITS ? &lf_g_intt_digits
                : which == LF_TUNE_DIGIT_PLANES ? &g_digit_planes : which == LF_TUNE_WS_EXTRA_STAGE ? &lf_g_ws_extra_stage
                : which == LF_TUNE_MORE_PLANES ? &g_more_planes : which == LF_TUNE_PC_MATMUL_TILE ? &g_pc_matmul_tile : nullptr;
    if (!knob) return -1;
    const int old = *knob;
    if (value < 0) return old;
    if (which == LF_TUNE_KS_EXT_COLS_MAX && value > 5) return old;
    if (which == LF_TUNE_MORE_PLANES && value > 3) return old;
    if (which == LF_TUNE_PC_MATMUL_TILE && value > 2) return old;
    if ((which == LF_TUNE_INTT_DIGITS || which == LF_TUNE_DIGIT_PLANES || which == LF_TUNE_WS_EXTRA_STAGE) && value > 1) return old;
    if (*knob != value && (which == LF_TUNE_DIGIT_PLANES || which == LF_TUNE_WS_EXTRA_STAGE || which == LF_TUNE_MORE_PLANES))
        lf_fmt_epoch_bump(which == LF_TUNE_WS_EXTRA_STAGE ? LF_FMT_WS_SPLIT0 : LF_FMT_RAW);   // scratch of that family so far: another setting
    *knob = value;
    return old;
}

int lf_key_planes(const int64_t *src_b, const int64_t *src_a, int64_t *dst_b, int64_t *dst_a, int rows, int64_t N,
                  const int64_t *ql, const int64_t *qh, int device, void *stream) {
    if (rows < 0 || rows > 65535 || N < 2 || (N & 1) || !src_b || !src_a || !dst_b || !dst_a || dst_b == dst_a || src_b == dst_b ||
        src_a == dst_a || src_a == dst_b || src_b == dst_a || !ql || !qh ||
        (((uintptr_t)src_b | (uintptr_t)src_a | (uintptr_t)dst_b | (uintptr_t)dst_a) & 15))
        return LF_ERR_ARG;
    if (rows == 0) return 0;
    if (int e = lf_set_device(device)) return e;
    hipLaunchKernelGGL(key_planes_kernel, dim3((unsigned)((N / 2 + 255) / 256), (unsigned)rows), dim3(256), 0, (hipStream_t)stream,
                       (const i64 *)src_b, (const i64 *)src_a, (i64 *)dst_b, (i64 *)dst_a, (i64)N, (const i64 *)ql, (const i64 *)qh);
    return (int)hipGetLastError();
}

int64_t lf_plain_planes_words(int rows, int64_t N, const int64_t *q_host) {
    uint64_t small;
    if (N < ((int64_t)1 << 13) || N > ((int64_t)1 << KS_LOGN_MAX) || (N & (N - 1)) || !lf_plain_planes_mask(rows, q_host, &small)) return 0;
    return (int64_t)rows * N - (int64_t)__builtin_popcountll(small) * (N >> 2);
}

static int plain_planes_launch(bool pack, const int64_t *src, int64_t *dst, int rows, int64_t N, const int64_t *q_host, const int64_t *ql,
                               const int64_t *qh, const int64_t *kl, const int64_t *kh, int device, void *stream) {
    uint64_t small;
    if (!lf_plain_planes_words(rows, N, q_host) || !src || !dst || src == dst || !ql || !qh || !kl || !kh ||
        (((uintptr_t)src | (uintptr_t)dst) & 15) || !lf_plain_planes_mask(rows, q_host, &small))
        return LF_ERR_ARG;
    if (int e = lf_set_device(device)) return e;
    const dim3 grid((unsigned)(N / 512), (unsigned)rows);
    if (pack)
        hipLaunchKernelGGL(plain_planes_kernel, grid, dim3(256), 0, (hipStream_t)stream, (const i64 *)src, (i64 *)dst, (i64)N,
                           (unsigned long long)small, (const i64 *)ql, (const i64 *)qh, (const i64 *)kl, (const i64 *)kh);
    else
        hipLaunchKernelGGL(plain_unplanes_kernel, grid, dim3(256), 0, (hipStream_t)stream, (const i64 *)src, (i64 *)dst, (i64)N,
                           (unsigned long long)small, (const i64 *)ql, (const i64 *)qh);
    return (int)hipGetLastError();
}

int lf_plain_planes(const int64_t *src, int64_t *dst, int rows, int64_t N, const int64_t *q_host, const int64_t *ql, const int64_t *qh,
                    const int64_t *kl, const int64_t *kh, int device, void *stream) {
    return plain_planes_launch(true, src, dst, rows, N, q_host, ql, qh, kl, kh, device, stream);
}

int lf_plain_unplanes(const int64_t *src, int64_t *dst, int rows, int64_t N, const int64_t *q_host, const int64_t *ql, const int64_t *qh,
                      const int64_t *kl, const int64_t *kh, int device, void *stream) {
    return plain_planes_launch(false, src, dst, rows, N, q_host, ql, qh, kl, kh, device, stream);
}

int lf_ks_core_batch(const int64_t *state, int64_t state_stride, int nct, int nparts, int rows, int logN, const int64_t *desc,
                     const int64_t *E, const double *Ed, const int64_t *ksk, int64_t part_stride, int64_t comp_stride,
                     int64_t row_off, int key_format, int64_t *tmp, int64_t *s, const int64_t *psi_br, const double *psi_dp,
                     const int64_t *ipsi_br, const double *ipsi_dp, const int64_t *Ninv, const int64_t *q_host, const int64_t *ql, const int64_t *qh, const int64_t *kl, const int64_t *kh, int device,
                     void *stream) {
    if (nparts < 1 || rows < 1 || rows > MAX_LIST_ROWS || logN <= NTT_TILE_LOG_MAX || logN > KS_LOGN_MAX ||
        !q_host || !psi_dp || !ipsi_dp || !Ed || (nct != 1 && nct != 2 && nct != 4))
        return LF_ERR_ARG;
    if (!lf_fp64_digits_ok(nparts, rows, q_host)) return LF_ERR_ARG;
    if (int e = lf_set_device(device)) return e;
    hipStream_t st = (hipStream_t)stream;
    const LfMod m{ql, qh, kl, kh, q_host};
    if (int e = ks_forward(state, state_stride, nct, nparts, rows, logN, desc, E, Ed, tmp, {psi_br, psi_dp}, m, st)) return e;
    return ks_tail(nct, nparts, rows, logN, {&ksk, 1, part_stride, comp_stride, row_off, key_format}, tmp, s, {ipsi_br, ipsi_dp, Ninv}, m, st);
}

/* The two halves of lf_ks_core as separate calls, so that a limb-sharded engine can start on the digits that have
 * arrived while the others are still travelling ("gather part p+1 while extending part p"):
 *   lf_ks_fwd   extension + forward NTT of `nparts` digits, descriptors desc[0 .. nparts) (the caller offsets desc and
 *               tmp to the first digit of the group: tmp_group = tmp + first * rows * N);
 *   lf_ks_tail  once every group is done: inner product of ALL nparts digits with the key + inverse NTT. */
int lf_ks_fwd(const int64_t *state, int nparts, int rows, int logN, const int64_t *desc, const int64_t *E, const double *Ed,
              int64_t *tmp, const int64_t *psi_br, const double *psi_dp, const int64_t *q_host, const int64_t *ql,
              const int64_t *qh, const int64_t *kl, const int64_t *kh, int device, void *stream) {
    if (nparts < 0 || rows < 1 || rows > MAX_LIST_ROWS || logN <= NTT_TILE_LOG_MAX || logN > KS_LOGN_MAX ||
        !q_host || !psi_dp || !Ed)
        return LF_ERR_ARG;
    if (nparts == 0) return 0;
    if (int e = lf_set_device(device)) return e;
    return ks_forward(state, 0, 1, nparts, rows, logN, desc, E, Ed, tmp, {psi_br, psi_dp}, {ql, qh, kl, kh, q_host}, (hipStream_t)stream);
}

int lf_ks_tail(int nparts, int rows, int logN, const int64_t *ksk, int64_t part_stride, int64_t comp_stride, int64_t row_off,
               int key_format, int64_t *tmp, int64_t *s, const int64_t *ipsi_br, const double *ipsi_dp, const int64_t *Ninv,
               const int64_t *q_host, const int64_t *ql, const int64_t *qh, const int64_t *kl,
               const int64_t *kh, int device, void *stream) {
    if (nparts < 1 || rows < 1 || rows > MAX_LIST_ROWS || logN <= NTT_TILE_LOG_MAX || logN > KS_LOGN_MAX ||
        !q_host || !ipsi_dp)
        return LF_ERR_ARG;
    if (!lf_fp64_digits_ok(nparts, rows, q_host)) return LF_ERR_ARG;
    if (int e = lf_set_device(device)) return e;
    return ks_tail(1, nparts, rows, logN, {&ksk, 1, part_stride, comp_stride, row_off, key_format}, tmp, s, {ipsi_br, ipsi_dp, Ninv},
                   {ql, qh, kl, kh, q_host}, (hipStream_t)stream);
}

/* Relinearisation inside cc_mult (see RelinFold): lf_ks_core_batch / lf_ks_fwd / lf_ks_tail whose sums additionally
 * receive P * (x0 y0) and P * (x0 y1 + x1 y0) on the `ell` ordinary rows, from the stack x = [nct][4][ell][N]; with `own`
 * the (digit, own limb) pairs are neither extended nor transformed: the inner product forms x1 y1 for them. */
int lf_relin_core_batch(const int64_t *state, int64_t state_stride, int nct, int nparts, int rows, int logN, const int64_t *desc,
                        const int64_t *E, const double *Ed, const int64_t *ksk, int64_t part_stride, int64_t comp_stride,
                        int64_t row_off, int key_format, int64_t *tmp, int64_t *s, const int64_t *psi_br, const double *psi_dp,
                        const int64_t *ipsi_br, const double *ipsi_dp, const int64_t *Ninv, const int64_t *x, int64_t x_ct_stride,
                        const int64_t *PR, int ell, const uint8_t *own, const int64_t *q_host,
                        const int64_t *ql, const int64_t *qh, const int64_t *kl, const int64_t *kh, int device, void *stream) {
    if (nparts < 1 || nparts > 254 || rows < 1 || rows > MAX_LIST_ROWS || logN <= NTT_TILE_LOG_MAX || logN > KS_LOGN_MAX ||
        !q_host || !psi_dp || !ipsi_dp || !Ed || (nct != 1 && nct != 2 && nct != 4) || !x || !PR || ell < 0 || ell > rows)
        return LF_ERR_ARG;
    if (!lf_fp64_digits_ok(nparts, rows, q_host)) return LF_ERR_ARG;
    if (int e = lf_set_device(device)) return e;
    hipStream_t st = (hipStream_t)stream;
    const LfMod m{ql, qh, kl, kh, q_host};
    if (int e = ks_forward(state, state_stride, nct, nparts, rows, logN, desc, E, Ed, tmp, {psi_br, psi_dp}, m, st, (const unsigned char *)own, 0))
        return e;
    const int xpl = (key_format & LF_STACK_PLANES) ? 1 : 0;
    for (int t = 0; t < nct; ++t)   // the operand stacks must be in the format the caller says (see lf_fmt_expect)
        if (int e = lf_fmt_expect(x + t * x_ct_stride, ((size_t)4 * ell << logN) * 8, xpl ? LF_FMT_PLANES : LF_FMT_RAW)) return e;
    const RelinFold fold{(const i64 *)x, (i64)x_ct_stride, (const i64 *)PR, ell, (const unsigned char *)own, xpl};
    return ks_tail(nct, nparts, rows, logN, {&ksk, 1, part_stride, comp_stride, row_off, key_format & ~LF_STACK_PLANES}, tmp, s,
                   {ipsi_br, ipsi_dp, Ninv}, m, st, &fold);
}

int lf_relin_fwd(const int64_t *state, int first, int nparts, int rows, int logN, const int64_t *desc, const int64_t *E,
                 const double *Ed, int64_t *tmp, const int64_t *psi_br, const double *psi_dp, const uint8_t *own,
                 const int64_t *q_host, const int64_t *ql, const int64_t *qh, const int64_t *kl, const int64_t *kh, int device,
                 void *stream) {
    if (first < 0 || nparts < 0 || first + nparts > 254 || rows < 1 || rows > MAX_LIST_ROWS || logN <= NTT_TILE_LOG_MAX ||
        logN > KS_LOGN_MAX || !q_host || !psi_dp || !Ed)
        return LF_ERR_ARG;
    if (nparts == 0) return 0;
    if (int e = lf_set_device(device)) return e;
    return ks_forward(state, 0, 1, nparts, rows, logN, desc + 3 * (int64_t)first, E, Ed, tmp + (((int64_t)first * rows) << logN),
                      {psi_br, psi_dp}, {ql, qh, kl, kh, q_host}, (hipStream_t)stream, (const unsigned char *)own, first);
}

int lf_relin_tail(int nparts, int rows, int logN, const int64_t *ksk, int64_t part_stride, int64_t comp_stride, int64_t row_off,
                  int key_format, int64_t *tmp, int64_t *s, const int64_t *ipsi_br, const double *ipsi_dp, const int64_t *Ninv,
                  const int64_t *x, const int64_t *PR, int ell, const uint8_t *own, const int64_t *q_host, const int64_t *ql, const int64_t *qh, const int64_t *kl, const int64_t *kh, int device,
                  void *stream) {
    if (nparts < 1 || nparts > 254 || rows < 1 || rows > MAX_LIST_ROWS || logN <= NTT_TILE_LOG_MAX || logN > KS_LOGN_MAX ||
        !q_host || !ipsi_dp || !x || !PR || ell < 0 || ell > rows)
        return LF_ERR_ARG;
    if (!lf_fp64_digits_ok(nparts, rows, q_host)) return LF_ERR_ARG;
    if (int e = lf_set_device(device)) return e;
    const int xpl = (key_format & LF_STACK_PLANES) ? 1 : 0;
    if (int e = lf_fmt_expect(x, ((size_t)4 * ell << logN) * 8, xpl ? LF_FMT_PLANES : LF_FMT_RAW)) return e;
    const RelinFold fold{(const i64 *)x, 0, (const i64 *)PR, ell, (const unsigned char *)own, xpl};
    return ks_tail(1, nparts, rows, logN, {&ksk, 1, part_stride, comp_stride, row_off, key_format & ~LF_STACK_PLANES}, tmp, s,
                   {ipsi_br, ipsi_dp, Ninv}, {ql, qh, kl, kh, q_host}, (hipStream_t)stream, &fold);
}

int lf_ks_core(const int64_t *state, int nparts, int rows, int logN, const int64_t *desc, const int64_t *E,
               const double *Ed, const int64_t *ksk, int64_t part_stride, int64_t comp_stride, int64_t row_off,
               int key_format, int64_t *tmp, int64_t *s, const int64_t *psi_br, const double *psi_dp,
               const int64_t *ipsi_br, const double *ipsi_dp, const int64_t *Ninv, const int64_t *q_host, const int64_t *ql, const int64_t *qh, const int64_t *kl, const int64_t *kh, int device,
               void *stream) {
    return lf_ks_core_batch(state, 0, 1, nparts, rows, logN, desc, E, Ed, ksk, part_stride, comp_stride, row_off, key_format, tmp, s, psi_br,
                            psi_dp, ipsi_br, ipsi_dp, Ninv, q_host, ql, qh, kl, kh, device, stream);
}

}  // extern "C"
