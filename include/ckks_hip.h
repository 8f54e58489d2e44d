/*
 * ckks_hip.h — C ABI of libckks_hip.so, the MI355X (gfx950) RNS-CKKS arithmetic library.
 *
 * This is the drop-in boundary for the reference's pybind11 module `liberate.ntt.ntt_cuda`
 * (reference: src/liberate/ntt/ntt.cpp:421-437 exports 15 functions over std::vector<torch::Tensor>,
 * one tensor per GPU).  Each entry point below replaces ONE of those functions for ONE device: the
 * per-GPU loop of ntt.cpp:130-141 lives in the caller (one process per GPU, or the Python shim
 * liberate_fhe_amd/ntt/ntt_cuda.py which walks the tensor lists).
 *
 * Conventions
 *   - all pointers are DEVICE pointers on `device`; data and constants are int64 (the reference's
 *     62-bit word mode, Montgomery radix R = 2^62, values lazily in [0, 2q));
 *   - polynomials are row-major [rows][N], one RNS limb per row, row pitch = N words;
 *   - per-row constant vectors are indexed by row id exactly as the reference kernels do
 *     (K.cu = src/liberate/ntt/ntt_cuda_kernel.cu): ql/qh = q & (2^31-1), q >> 31; kl/kh likewise
 *     for k = -q^-1 mod 2^62; _2q = 2q;
 *   - the reference's implicit extent rules are explicit arguments: elementwise ops run over
 *     `rows` = a.size(0) (K.cu:110-114), NTT-family ops over `rows` = ql.size(0) (K.cu:298);
 *   - twiddles are the compact table psi_br[rows][N] (entry x = Montgomery form of psi^brev(x)),
 *     not the reference's [rows][logN][N/2] per-stage table; the butterfly DAG and per-butterfly
 *     formulas are the reference's, so every lazy output word is bit-identical;
 *   - `stream` is a hipStream_t (0 = the null stream); launches are asynchronous, nothing syncs;
 *   - return value: 0 on success, otherwise the hipError_t of the failed call/launch, or
 *     LF_ERR_ARG for an invalid argument.  (The reference returns nothing and checks nothing.)
 */
#ifndef CKKS_HIP_H
#define CKKS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LF_ERR_ARG 10001
/* Two halves of one operation were called under different lf_tune settings: the scratch the first half left is in another
 * format than the second half is about to read (lf_ks_fwd -> lf_ks_tail, lf_cc_mult_evk_pre -> _post, lf_ntt_pass_ws 1 -> 2).
 * Nothing is launched; repeat the first half. */
#define LF_ERR_STATE 10002

/* Library probe: returns the ABI version (currently LF_ABI_VERSION; __graft_entry__.build() asserts it). */
#define LF_ABI_VERSION 15
int lf_abi_version(void);

/* Compile-time capacities of the fused kernels, so that callers can refuse a parameter set BEFORE any launch
 * (the digit width alpha and K live in device-side descriptors the ABI cannot check):
 *   which = 0: limbs per key-switch digit (alpha), 1: special primes K, 2: limb rows per call (`rows`),
 *           3: operand sets per batched call (count), 4: largest logN of the NTT family,
 *           6: log2 of the bound of the fp64 class — a row whose prime is below 2^41 is computed in fp64 and, where a format keeps
 *              such rows as 6-byte planes (lf_key_planes, lf_plain_planes), stored so; a caller that lays such a format out reads the
 *              bound here.  Other (5 among them): -1. */
#define LF_LIMIT_DIGIT_LIMBS 0
#define LF_LIMIT_SPECIAL_PRIMES 1
#define LF_LIMIT_ROWS 2
#define LF_LIMIT_BATCH 3
#define LF_LIMIT_LOGN 4
#define LF_LIMIT_SMALL_PRIME_BITS 6
int lf_limits(int which);

/* Key-switch digits (`nparts`) where a limb row is of the fp64 class (prime below 2^41): a constant of the ABI, not a capacity
 * lf_limits reports (its answers stay as they are).  The inner products of
 * that class add one balanced product (|.| <= q / 2) per digit and reduce once, with a reduction that is exact for |x| < 64 q.
 * The kernel that adds most besides (the giant step of lf_linear_transform_bsgs: a gathered word and an accumulator word, both
 * below 2q) needs nparts / 2 + 4 < 64, so 119 digits is the most for which every such sum is proven in range.  Every entry that
 * launches such a kernel - lf_ks_core(_batch), lf_ks_tail, lf_relin_core_batch, lf_relin_tail and every entry that takes an
 * lf_ks_plan - returns LF_ERR_ARG before any launch when q_host holds a prime of that class and nparts is larger.  Parameter
 * sets whose rows are all of the integer class keep the entries' own limit (254 where one is stated): they reduce after every
 * addition. */
#define LF_FP64_MAX_DIGITS 119

/* Keyed baby steps of one lf_linear_transform_bsgs call: slot 0 is the ciphertext and slots 1 .. 63 the keys, one bit each of the
 * 64-bit masks of the diagonal products.  lf_linear_transform_bsgs and lf_linear_transform_bsgs_ws_words refuse more. */
#define LF_BSGS_MAX_BABY_KEYS 63

/* Every entry that takes an lf_ks_plan also refuses a plan with more than lf_limits(LF_LIMIT_ROWS) rows (ell + K), as the step
 * entries do for their `rows`. */

/* Launch-shape thresholds (never results: every setting produces the same words).  Returns the previous value, -1 for an
 * unknown `which`; value < 0 only reads.  PROCESS-WIDE mutable state, read by every entry at launch time on whatever
 * thread calls it and not synchronised: set it once, before any other thread launches (the engine never touches it; only
 * the A/B tools under tools/ do).
 *   LF_TUNE_KS_EXT_COLS_MAX   largest logN - 12 (0 .. 5, default 5) for which the key switch's extension + leading stages run as
 *                             the column kernel (one register step per column, no LDS); above it the LDS-tiled form.
 *   LF_TUNE_INTT_DIGITS       1 (default): lf_cc_mult_evk(_batch / _pre) form the digits of x1 * y1 inside the last inverse pass
 *                             where a digit's limbs fit a column thread (lf_intt_mul_digits); 0: always the two launches.
 *   LF_TUNE_DIGIT_PLANES      1 (default): between the halves of a key switch (lf_ks_fwd -> lf_ks_tail and every entry built on
 *                             them) the fp64-class rows of the scratch `tmp` hold their words as two planes, 6 bytes per word
 *                             (u32 low[N], u16 high[N] behind them) instead of 8, at logN >= 13 when the limbs are of both
 *                             classes; 0: raw words.  `tmp` is scratch either way; the knob must not change
 *                             between an lf_ks_fwd and its lf_ks_tail: the tail then returns LF_ERR_STATE instead of reading the wrong format.
 *   LF_TUNE_WS_EXTRA_STAGE    1 (default): in lf_ntt_ws at logN 13 .. 16 the column pass takes one stage more than logN - 12 (it is
 *                             HBM-bound with issue slots to spare) and the tiled pass, which is issue-bound, skips its first; 0: the
 *                             split of lf_ntt.  A change between the two launches of a transform (lf_ntt_pass_ws 1 -> 2): LF_ERR_STATE.
 *   (knob 0 was the one-launch key-switch transform of round 3: slower at every preset size on MI355X, removed.) */
#define LF_TUNE_KS_EXT_COLS_MAX 1
#define LF_TUNE_INTT_DIGITS 2
#define LF_TUNE_DIGIT_PLANES 3
#define LF_TUNE_WS_EXTRA_STAGE 4
/*   LF_TUNE_MORE_PLANES       with LF_TUNE_DIGIT_PLANES on: bit 0 (default 1) the SUMS of a key switch travel from the inner product through
 *                             the tiled inverse pass to the column pass as planes (through `tmp`, two digits or more); bit 1
 *                             (default 1) lf_stack_planes() answers 1: the op entries keep cc_mult's operand stack as planes. */
#define LF_TUNE_MORE_PLANES 5
/*   LF_TUNE_PC_MATMUL_TILE    how lf_pc_matmul_batch covers 4 tokens of a chunk: 0 (default) two launches of pc_matmulb_kernel<GO, 2>
 *                             (2 tokens each, the plaintext words read twice); 1: ONE launch of <GO, 4>; 2: as 1, with 4 outputs
 *                             as two launches of <2, 4> (the transformed words read twice).  1 and 2 measured slower on MI355X
 *                             (DESIGN.md section 4.2); kept for tools/pc_matmul_batch.py --ab. */
#define LF_TUNE_PC_MATMUL_TILE 6
int lf_tune(int which, int value);

/* Measurement entry (not one of the reference's ops; the engine never calls it): ONE wave, launched on `stream`, takes
 * `samples` readings of the shader clock — out[2 i] = core-clock cycles (s_memtime) that passed during out[2 i + 1] ticks
 * (>= `ticks`) of the constant 100 MHz counter (s_memrealtime), so MHz = 100 * out[2 i] / out[2 i + 1].  Launched on a
 * second stream beside a kernel under test it reports the clock that kernel actually runs at (bench.py: the headline
 * kernels run with the package at its 1 400 W cap).  out: device, 2 * samples 64-bit words;
 * samples <= 4096, samples * ticks <= 10^9 (ten seconds of spinning), else LF_ERR_ARG. */
int lf_clock_probe(uint64_t *out, int samples, uint64_t ticks, int device, void *stream);

/* ---- elementwise family --------------------------------------------------------------------- */

/* ntt_cuda.mont_mult (ntt.cpp:120-144, K.cu:66-146): c[i][j] = REDC62(a[i][j] * b[i][j]). */
int lf_mont_mult(const int64_t *a, const int64_t *b, int64_t *c, int rows, int64_t N,
                 const int64_t *ql, const int64_t *qh, const int64_t *kl, const int64_t *kh,
                 int device, void *stream);

/* ntt_cuda.mont_enter (ntt.cpp:146-163, K.cu:154-226): a[i][j] = REDC62(a[i][j] * Rs[i]) in place. */
int lf_mont_enter(int64_t *a, const int64_t *Rs, int rows, int64_t N,
                  const int64_t *ql, const int64_t *qh, const int64_t *kl, const int64_t *kh,
                  int device, void *stream);

/* ntt_cuda.mont_redc (ntt.cpp:248-263, K.cu:559-653): a = (a + ((a*k) mod R) * q) / R in place. */
int lf_mont_redc(int64_t *a, int rows, int64_t N,
                 const int64_t *ql, const int64_t *qh, const int64_t *kl, const int64_t *kh,
                 int device, void *stream);

/* ntt_cuda.reduce_2q (K.cu:664-680, 1187-1191): a = a < q ? a : a - q, q = _2q >> 1. */
int lf_reduce_2q(int64_t *a, int rows, int64_t N, const int64_t *_2q, int device, void *stream);
/* ntt_cuda.make_signed (K.cu:682-699): a = a <= q/2 ? a : a - q. */
int lf_make_signed(int64_t *a, int rows, int64_t N, const int64_t *_2q, int device, void *stream);
/* ntt_cuda.make_unsigned (K.cu:980-995): a += q. */
int lf_make_unsigned(int64_t *a, int rows, int64_t N, const int64_t *_2q, int device, void *stream);
/* ntt_cuda.tile_unsigned (K.cu:997-1014, 1205-1214): dst[i][j] = a[j] + q_i, rows = _2q.size(0). */
int lf_tile_unsigned(const int64_t *a, int64_t *dst, int rows, int64_t N, const int64_t *_2q,
                     int device, void *stream);
/* ntt_cuda.mont_add / mont_sub (K.cu:1016-1058): c = (a +/- b) csub 2q. */
int lf_mont_add(const int64_t *a, const int64_t *b, int64_t *c, int rows, int64_t N, const int64_t *_2q,
                int device, void *stream);
int lf_mont_sub(const int64_t *a, const int64_t *b, int64_t *c, int rows, int64_t N, const int64_t *_2q,
                int device, void *stream);

/* ---- NTT family -------------------------------------------------------------------------------
 * `batch` polynomials of `rows` limbs each, stored back to back ([batch][rows][N]); limb i of every
 * polynomial uses constant/twiddle row i.  The reference API is batch = 1.
 *
 * psi_dp / ipsi_dp (optional for the exact ops, may be NULL; REQUIRED with LF_NTT_RELAXED and by lf_ks_*): the
 * AUXILIARY twiddle table, one row of 2N 8-byte words per limb, filled by lf_twiddle_dp.  Limbs whose prime is
 * below 2^41 hold the plain canonical twiddles as doubles in words [0, N) and run the fp64-FMA butterfly path;
 * results are bit-identical to the integer path.  Limbs with a larger prime hold N pairs (floor(w 2^64 / q), w)
 * with w the plain twiddle: the Shoup products of the relaxed transforms (the exact ops never read them).
 * q_host (optional for the exact ops, may be NULL; REQUIRED with LF_NTT_RELAXED): HOST array of the `rows` primes,
 * used to split the rows into the two arithmetic classes at launch time (each class has its own kernel
 * instantiation); with NULL every row of an exact op runs the integer class.  A relaxed call without psi_dp or
 * without q_host returns LF_ERR_ARG before anything is launched: lf_twiddle_dp lays each auxiliary row out by the
 * size of its prime, so the launch must know the primes to read it.
 * flags: LF_NTT_RELAXED = the caller only needs the result modulo q (outputs are then canonical
 * residues instead of the reference's lazy representatives; exception: the integer-class limbs of a relaxed FORWARD
 * transform at logN <= 12, one pass, come out as lazy words in [0, 2q)) — for fused internal use, never for the
 * drop-in ops.  A relaxed FORWARD transform accepts the reference's signed-lazy words (|a| < 2q); a relaxed
 * INVERSE transform takes non-negative words: below 2^46 on fp64-class limbs, lazy words in [0, 2q) on integer-class
 * limbs (what lf_tensor / lf_ks_inner / the fused core write).  The fp64 bound: the words enter as doubles unreduced,
 * every stage of the inverse at most doubles them, and the schedule folds them (dp_reduce_bal, exact for |x| < 2^52)
 * only after every second radix-8 step, so six stages run between folds: 2^6 * (2^46 - 1) < 2^52.  Larger words
 * leave the exact integer range of fp64 before the first fold (tests/test_class_edges_gpu.py holds the bound). */
#define LF_NTT_RELAXED 1
/* with LF_NTT_RELAXED: fp64-class limbs stay in the PLAIN domain — lf_ntt applies Rs to integer-class limbs
 * only, lf_intt (tail >= 2) multiplies fp64-class limbs by N^-1 instead of N^-1 R^-1.  Used by the fused
 * cc_mult, whose tensor product then needs one plain modular product per term (lf_tensor, plain = 1). */
#define LF_NTT_PLAIN 2
/* lf_rescale_ntt at two-launch ring degrees (logN 13 .. 16) only: enqueue ONE of its two launches — the column pass, the only
 * one that reads `in` / `row0` (addresses that change from call to call), or the tiled pass, which touches `x` alone (a
 * caller may keep it, with the launches behind it, in a HIP graph: lf_cc_mult_evk_pre's `which`).  Not both. */
#define LF_NTT_ONLY_COLS 4
#define LF_NTT_ONLY_TILED 8
/* The operand stack of the fused cc_mult — what lf_rescale_ntt writes with LF_NTT_RELAXED | LF_NTT_PLAIN and only lf_intt_mul(_digits)
 * and lf_relin_* read — may keep its fp64-class rows (primes below 2^41: canonical words below 2^41) as two PLANES: u32 low[N] at
 * byte 0 of the row's 8 N bytes, u16 high[N] at byte 4 N, 6 bytes per word on each of the stack's four trips through HBM;
 * integer-class rows stay raw words.  lf_rescale_ntt with LF_NTT_PLANES writes that format (two-launch ring degrees, rows of both
 * classes: lf_stack_planes() says when; otherwise LF_ERR_ARG), lf_intt_mul(_digits) with LF_NTT_PLANES read their factors in
 * it, lf_relin_core_batch / lf_relin_tail with LF_STACK_PLANES OR-ed into `key_format` read `x` in it.  A stack written in one
 * format and read in the other: LF_ERR_STATE. */
#define LF_NTT_PLANES 16
#define LF_STACK_PLANES 4
/* 1 when internal stacks of the rows [0, rows) of q_host (HOST) keep fp64-class rows as planes: lf_tune(LF_TUNE_DIGIT_PLANES)
 * is on, 13 <= logN <= 17 (a column pass of at most 5 stages: the ring degrees where lf_rescale_ntt accepts LF_NTT_PLANES), and
 * the rows hold primes of both arithmetic classes; 0 otherwise.  (The engine-op entries ask this themselves.) */
int lf_stack_planes(int logN, int rows, const int64_t *q_host);

/* The auxiliary table from the Montgomery-form compact table mont[rows][N]: out[rows][2N] (8-byte words).
 * Primes below 2^41: out[r][j] = (double)reduce_q(redc(mont[r][j])) for j < N; entry 0 of the row (psi^0 = 1, which
 * no butterfly stage reads) receives 1 / q_row instead — the fp64-class kernels take the reciprocal from there; words
 * [N, 2N) are unused.  Larger primes: pairs (out[r][2j], out[r][2j + 1]) = (floor(w 2^64 / q), w), w = reduce_q(redc(
 * mont[r][j])), as unsigned 64-bit integers.  Tables handed to lf_ntt / lf_intt / lf_ks_* must come from here. */
int lf_twiddle_dp(const int64_t *mont, double *out, int rows, int64_t N, const int64_t *ql, const int64_t *qh,
                  const int64_t *kl, const int64_t *kh, int device, void *stream);

/* ntt_cuda.ntt (ntt.cpp:166-188, K.cu:236-342): forward negacyclic NTT, natural in -> bit-reversed out.
 * ntt_cuda.enter_ntt (ntt.cpp:191-216, K.cu:349-423) when Rs != NULL: mont_enter(Rs) first. */
int lf_ntt(int64_t *a, int batch, int rows, int logN, const int64_t *psi_br, const double *psi_dp,
           const int64_t *q_host, const int64_t *Rs, int flags, const int64_t *_2q, const int64_t *ql,
           const int64_t *qh, const int64_t *kl, const int64_t *kh, int device, void *stream);

/* lf_ntt through a caller-provided WORKSPACE (exact transforms; same result words as lf_ntt, `a` in place).  The two passes
 * of a logN >= 13 transform hand every word over through HBM; with a workspace the column pass leaves the words of the
 * fp64-class limbs (primes below 2^41: lazy words below 2^42) there as 6-byte planes instead of 8-byte words and the tiled
 * pass reads those — 12.5 % fewer bytes per pass; operands outside [0, 2q), whose words can be anything, travel with a third
 * plane and a flag per column wave, so the reference's result on ANY int64 input is reproduced as by lf_ntt.
 * ws: lf_ntt_ws_words(batch, rows, logN) words of device memory, 16-byte aligned, contents irrelevant before and scratch
 * after; it must not be used by another stream while the call runs.  ws = NULL, logN <= 12 or > 17: lf_ntt.  The reference's
 * ntt (ntt.cpp:421-437) allocates nothing because it makes logN passes in place; the workspace is this design's price for
 * making two.  LF_NTT_RELAXED: LF_ERR_ARG. */
int64_t lf_ntt_ws_words(int batch, int rows, int logN);
int lf_ntt_ws(int64_t *a, int64_t *ws, int batch, int rows, int logN, const int64_t *psi_br, const double *psi_dp,
              const int64_t *q_host, const int64_t *Rs, int flags, const int64_t *ql, const int64_t *qh, const int64_t *kl,
              const int64_t *kh, int device, void *stream);
/* The inverse chains the same way (lf_intt with tail 0 .. 3 = intt / intt_exit / intt_exit_reduce / intt_exit_reduce_signed): the
 * tiled pass comes first and writes the workspace, the column pass with the chain tail reads it; a tile that meets an operand
 * outside [0, 2q) ships the third plane and raises its flag.  Same words as lf_intt on any input; same `ws` rules as lf_ntt_ws. */
int lf_intt_ws(int64_t *a, int64_t *ws, int batch, int rows, int logN, const int64_t *ipsi_br, const double *ipsi_dp,
               const int64_t *q_host, const int64_t *Ninv, int tail, int flags, const int64_t *ql, const int64_t *qh,
               const int64_t *kl, const int64_t *kh, int device, void *stream);
/* (measurement, as lf_ntt_pass: one of the two launches of lf_ntt_ws; which = 1 reads `a` and writes `ws`, 2 the reverse) */
int lf_ntt_pass_ws(int64_t *a, int64_t *ws, int batch, int rows, int logN, const int64_t *psi_br, const double *psi_dp,
                   const int64_t *q_host, const int64_t *Rs, int flags, int which, const int64_t *ql, const int64_t *qh,
                   const int64_t *kl, const int64_t *kh, int device, void *stream);

/* Measurement entry (not one of the reference's ops; the engine never calls it): launch exactly ONE of the two
 * pass kernels of a two-pass forward transform (logN >= 13) with the grid it has inside lf_ntt —
 * which = 1: the column pass, 2: the tiled pass — so that bench.py / tools can time the dominant kernel alone
 * with HIP events.  `a` is scratch afterwards (half a transform).  lf_ntt itself has no knobs. */
int lf_ntt_pass(int64_t *a, int batch, int rows, int logN, const int64_t *psi_br, const double *psi_dp,
                const int64_t *q_host, const int64_t *Rs, int flags, int which, const int64_t *ql, const int64_t *qh,
                const int64_t *kl, const int64_t *kh, int device, void *stream);

/* ntt_cuda.intt / intt_exit / intt_exit_reduce / intt_exit_reduce_signed
 * (ntt.cpp:219-345, K.cu:433-548, 709-973): inverse NTT, bit-reversed in -> natural out, then
 * x Ninv (= N^-1 * R mod q); `tail` selects the fused chain:
 *   0 intt, 1 + mont_redc, 2 + reduce (canonical [0,q)), 3 + make_signed.
 * LF_NTT_RELAXED requires tail >= 2 (whose outputs are canonical anyway). */
int lf_intt(int64_t *a, int batch, int rows, int logN, const int64_t *ipsi_br, const double *ipsi_dp,
            const int64_t *q_host, const int64_t *Ninv, int tail, int flags, const int64_t *_2q,
            const int64_t *ql, const int64_t *qh, const int64_t *kl, const int64_t *kh, int device, void *stream);

/* lf_intt of an element-wise PRODUCT, formed as the first pass reads its tiles (no product tensor in HBM):
 *   dst[p] = intt(a[p] * b[p]),  polynomial p of `a` / `b` at a + p * a_stride / b + p * b_stride (words), dst [batch][rows][N].
 * cc_mult's third tensor component x1 * y1 (ckks_engine.py:1099-1101, 1129) enters the key switch this way.  Requires
 * LF_NTT_RELAXED (tail >= 2) and logN >= 13; with LF_NTT_PLAIN the fp64-class limbs hold plain residues and get a plain
 * product, integer-class limbs Montgomery-form words (below 2q) and the REDC62 product — lf_tensor's d2 (plain = 1).
 * LF_NTT_PLANES (factors in the planes format) at logN <= 17 only, like lf_stack_planes. */
int lf_intt_mul(int64_t *dst, const int64_t *a, int64_t a_stride, const int64_t *b, int64_t b_stride, int batch, int rows, int logN,
                const int64_t *ipsi_br, const double *ipsi_dp, const int64_t *q_host, const int64_t *Ninv, int tail, int flags,
                const int64_t *ql, const int64_t *qh, const int64_t *kl, const int64_t *kh, int device, void *stream);

/* Not one of the reference's ops: `count` (<= 8) rows of N words, each anywhere in device memory (16-byte aligned; HOST array
 * of device pointers), into the consecutive rows of dst — one launch.  The engine stages the dropped limb's rows of all
 * operands of a rescale with it before they fan out to the other ranks (ckks_engine.py:999-1011 stages them through the host). */
int lf_gather_rows(const int64_t *const *src, int64_t *dst, int count, int64_t N, int device, void *stream);

/* Galois automorphism of coefficient-domain rows (reference: encdec.py:224-270 `rotate`/`conjugate`,
 * done there with torch advanced indexing): dst[i][(p*n mod 2N) mod N] = +/- a[i][n], sign - iff
 * (p*n mod 2N) >= N.  If _2q != NULL the reference's follow-up make_unsigned + reduce_2q
 * (ckks_engine.py:1198-1200) is fused: the stored value is canonical in [0, q). */
int lf_galois(const int64_t *a, int64_t *dst, int rows, int logN, int64_t p, const int64_t *_2q,
              int device, void *stream);

/* ---- engine-level fused ops -------------------------------------------------------------------
 * Each replaces a run of ntt_cuda calls + torch elementwise ops issued by the reference's Python
 * engine (ckks_engine.py = src/liberate/fhe/ckks_engine.py); arithmetic is op-for-op the reference's. */

/* ckks_engine.rescale body (ckks_engine.py:1017-1041): out[i] = reduce_q(REDC((in[i] - row0) * scales[i])
 * + [row0 > round_at]); `in` points at the first surviving row, constants are those of the surviving rows. */
int lf_rescale(const int64_t *in, const int64_t *row0, int64_t *out, int rows, int64_t N, const int64_t *scales,
               int64_t round_at, const int64_t *ql, const int64_t *qh, const int64_t *kl, const int64_t *kh,
               int device, void *stream);

/* cc_mult's tensor product (ckks_engine.py:1095-1101): d0 = x0*y0, d1 = x0*y1 (+) x1*y0, d2 = x1*y1 (REDC, lazy).
 * plain = 1 (operands from lf_ntt with LF_NTT_RELAXED|LF_NTT_PLAIN): limbs with a prime below 2^41 hold plain
 * canonical residues and get plain fp64 products (canonical outputs); other limbs as above. */
int lf_tensor(const int64_t *x0, const int64_t *x1, const int64_t *y0, const int64_t *y1, int64_t *d0, int64_t *d1,
              int64_t *d2, int rows, int64_t N, int plain, const int64_t *ql, const int64_t *qh, const int64_t *kl,
              const int64_t *kh, int device, void *stream);

/* pre_extend (ckks_engine.py:654-705) for all local key-switch digits at once: mixed-radix (Garner) digits.
 * desc[p] = {row_start, alpha, y_off, l_off} (int64 x4); tab holds Y_scalar / L_scalar (ntt_context.py:328-345). */
int lf_ks_digits(const int64_t *a, int64_t *state, int nparts, const int64_t *desc, const int64_t *tab, int64_t N,
                 const int64_t *ql, const int64_t *qh, const int64_t *kl, const int64_t *kh, int device, void *stream);

/* extend (ckks_engine.py:707-743) of every digit to every local target row: ext[p][r] in Montgomery form.
 * desc[p] = {row_start, alpha, e_off} (int64 x3); E[e_off + i*rows + r] = R^2 (i = 0) or L_{i-1} R^2 mod q_r. */
int lf_ks_extend(const int64_t *state, int64_t *ext, int nparts, int rows, int64_t N, const int64_t *desc,
                 const int64_t *E, const int64_t *ql, const int64_t *qh, const int64_t *kl, const int64_t *kh,
                 int device, void *stream);

/* switcher_later_part's two mont_mults + the sum over digits (ckks_engine.py:931-934, 832-840); the key is
 * addressed as ksk[p*part_stride + comp*comp_stride + (row_off + r)*N + j], comp 0 = b, 1 = a. */
int lf_ks_inner(const int64_t *ext, const int64_t *ksk, int64_t part_stride, int64_t comp_stride, int64_t row_off,
                int64_t *s0, int64_t *s1, int nparts, int rows, int64_t N, const int64_t *ql, const int64_t *qh,
                const int64_t *kl, const int64_t *kh, int device, void *stream);

/* division by P = prod(special primes) (ckks_engine.py:850-901) on canonical coefficient rows s[ell+K][N];
 * PiR[P_ind][row] = P_j^-1 R mod q_row ([K][ell+K], specials last-first); optional addend:
 * out = reduce_q(result + addend) (relinearize 1135-1140 / switch_key 952-953).
 * PiP (optional, may be NULL): the same table as plain residues P_j^-1 mod q_row in doubles; when given,
 * rows with a prime below 2^41 take the fp64 path (identical canonical output). */
int lf_ks_moddown(const int64_t *s, int64_t *out, const int64_t *addend, int ell, int K, int64_t N,
                  const int64_t *PiR, const double *PiP, const int64_t *Rs, const int64_t *ql, const int64_t *qh, const int64_t *kl,
                  const int64_t *kh, int device, void *stream);

/* Fused key-switch core for two-pass ring degrees up to a column pass of 5 stages (13 <= logN <= 17; any other logN: LF_ERR_ARG,
 * nothing launched — the same holds for lf_ks_core_batch, lf_ks_fwd, lf_ks_tail and lf_relin_*): extend + NTT + inner product with the key +
 * sum over digits + inverse NTT to canonical coefficients, i.e. lf_ks_extend -> lf_ntt -> lf_ks_inner ->
 * lf_intt(tail 2) (ckks_engine.py:707-743, 919, 931-934, 832-848) without materialising the extended digits.
 *   state      [*, N] Garner digits in storage order (output of lf_ks_digits, gathered)
 *   desc, E    as for lf_ks_extend (alpha field: bit 8 set = the digit's words exceed 53 bits, i.e. a digit of
 *              60-bit primes; lf_ks_extend ignores the flag); Ed = the same constants as PLAIN residues in doubles
 *              (Ed[e_off + i*rows + r] = L_{i-1} mod q_r, i = 0: 1.0) for the fp64 class
 *   ksk        key, addressed as in lf_ks_inner
 *   tmp        scratch [nparts][rows][N]; s out [2][rows][N]
 *   q_host     HOST primes of the `rows` limbs (required: selects the arithmetic class per limb) */
int lf_ks_core(const int64_t *state, int nparts, int rows, int logN, const int64_t *desc, const int64_t *E,
               const double *Ed, const int64_t *ksk, int64_t part_stride, int64_t comp_stride, int64_t row_off,
               int key_format, int64_t *tmp, int64_t *s, const int64_t *psi_br, const double *psi_dp,
               const int64_t *ipsi_br, const double *ipsi_dp, const int64_t *Ninv, const int64_t *q_host, const int64_t *ql, const int64_t *qh, const int64_t *kl, const int64_t *kh, int device,
               void *stream);

/* Key formats of the fused key-switch entries (`key_format`).  The inner product with the key is the one launch of a key
 * switch that runs at the HBM rate, and most of what it reads is the key (gold: 450 of 687 MB), read once per call and never
 * modified: a binding may therefore keep a second, smaller copy of a key for these entries.
 *   LF_KEY_RAW     the reference's layout: 64-bit words, ksk[p*part_stride + comp*comp_stride + (row_off + r)*N + j];
 *   LF_KEY_PLANES  what lf_key_planes writes: same strides and row slots, but for a row r whose prime is below 2^41 the
 *                  slot of component 0 holds N / 2 groups of 16 bytes { lo32 b[j], lo32 b[j+1], lo32 a[j], lo32 a[j+1] } and
 *                  the first 4 N bytes of the slot of component 1 hold N / 2 groups of 8 bytes { hi16 b[j], hi16 b[j+1],
 *                  hi16 a[j], hi16 a[j+1] } (j even) of the CANONICAL residues of both components: 12 N instead of 16 N
 *                  bytes, and one 16-byte + one 8-byte load per thread and digit instead of two 16-byte ones.  Rows of
 *                  larger primes are raw words in their own slots.  16-byte aligned base and strides.
 * The sums are the same residues either way, so every output word of the entries below is identical.
 * lf_key_planes converts the `rows` rows of ONE key part (src_b / src_a: its two components, any lazy / signed-lazy words;
 * dst_b / dst_a: the part's two slots in a tensor of the raw key's shape, distinct from the sources; ql / qh: DEVICE 31-bit
 * halves of the rows' primes as everywhere in this header); a key is converted part by part. */
#define LF_KEY_RAW 0
#define LF_KEY_PLANES 1
int lf_key_planes(const int64_t *src_b, const int64_t *src_a, int64_t *dst_b, int64_t *dst_a, int rows, int64_t N,
                  const int64_t *ql, const int64_t *qh, int device, void *stream);

/* lf_ks_digits(_galois) of `count` (<= 8) polynomials in one launch: a / state are HOST arrays of device pointers
 * (gal_pinv = 0: no Galois map). */
int lf_ks_digits_batch(const int64_t *const *a, int64_t *const *state, int count, int nparts, const int64_t *desc,
                       const int64_t *tab, int64_t N, int64_t gal_pinv, const int64_t *gal_2q, const int64_t *ql,
                       const int64_t *qh, const int64_t *kl, const int64_t *kh, int device, void *stream);

/* lf_ks_core for `nct` (1, 2 or 4) ciphertexts switched under the SAME key (a batch of rotations by one step,
 * config "rotate batched 64 ciphertexts"): every launch covers all of them and the inner product reads each key
 * word once for the whole batch.  state: nct digit states `state_stride` words apart; tmp scratch
 * [nct][nparts][rows][N]; s out [nct][2][rows][N].  Results equal nct calls of lf_ks_core. */
int lf_ks_core_batch(const int64_t *state, int64_t state_stride, int nct, int nparts, int rows, int logN, const int64_t *desc,
                     const int64_t *E, const double *Ed, const int64_t *ksk, int64_t part_stride, int64_t comp_stride,
                     int64_t row_off, int key_format, int64_t *tmp, int64_t *s, const int64_t *psi_br, const double *psi_dp,
                     const int64_t *ipsi_br, const double *ipsi_dp, const int64_t *Ninv, const int64_t *q_host, const int64_t *ql, const int64_t *qh, const int64_t *kl, const int64_t *kh, int device,
                     void *stream);

/* The two halves of lf_ks_core as separate calls (single ciphertext), so that a limb-sharded engine can start on the
 * digits that have already arrived while the others are still travelling over xGMI (ckks_engine.py:778-829 stages
 * every digit through the host before any extension starts):
 *   lf_ks_fwd   extension + forward NTT of `nparts` digits, descriptors desc[0 .. nparts); the caller offsets desc
 *               and tmp to the first digit of the group (desc + 3 * first, tmp + first * rows * N);
 *   lf_ks_tail  after the last group: inner product of ALL nparts digits in tmp with the key + inverse NTT (tmp is scratch
 *               afterwards: with two digits or more the sums' inverse transform passes through it).
 * lf_ks_fwd over all digits followed by lf_ks_tail == lf_ks_core. */
int lf_ks_fwd(const int64_t *state, int nparts, int rows, int logN, const int64_t *desc, const int64_t *E, const double *Ed,
              int64_t *tmp, const int64_t *psi_br, const double *psi_dp, const int64_t *q_host, const int64_t *ql,
              const int64_t *qh, const int64_t *kl, const int64_t *kh, int device, void *stream);
int lf_ks_tail(int nparts, int rows, int logN, const int64_t *ksk, int64_t part_stride, int64_t comp_stride, int64_t row_off,
               int key_format, int64_t *tmp, int64_t *s, const int64_t *ipsi_br, const double *ipsi_dp, const int64_t *Ninv,
               const int64_t *q_host, const int64_t *ql, const int64_t *qh, const int64_t *kl,
               const int64_t *kh, int device, void *stream);

/* Relinearisation inside cc_mult (ckks_engine.py:1095-1101, 1117-1151) without inverse transforms of d0 and d1:
 * dividing by P is linear and P * d vanishes modulo every special prime, so moddown(s) + d == moddown(s + P * d on the
 * ordinary rows).  lf_relin_core_batch / lf_relin_tail are lf_ks_core_batch / lf_ks_tail whose sums additionally receive,
 * in the NTT domain, on the first `ell` (ordinary) of the `rows` limbs,
 *     s[0] += P * (x0 * y0),    s[1] += P * (x0 * y1 + x1 * y0),
 * from x = [nct][4][ell][N] (x0, x1, y0, y1 as lf_rescale_ntt with LF_NTT_RELAXED | LF_NTT_PLAIN leaves them; stacks of
 * consecutive ciphertext pairs x_ct_stride words apart) and PR[r] = P * R mod q_r.  lf_ks_moddown_* of the result, with no
 * addend, is the relinearised ciphertext: the same canonical words as the reference's chain. */
int lf_relin_core_batch(const int64_t *state, int64_t state_stride, int nct, int nparts, int rows, int logN, const int64_t *desc,
                        const int64_t *E, const double *Ed, const int64_t *ksk, int64_t part_stride, int64_t comp_stride,
                        int64_t row_off, int key_format, int64_t *tmp, int64_t *s, const int64_t *psi_br, const double *psi_dp,
                        const int64_t *ipsi_br, const double *ipsi_dp, const int64_t *Ninv, const int64_t *x, int64_t x_ct_stride,
                        const int64_t *PR, int ell, const uint8_t *own, const int64_t *q_host,
                        const int64_t *ql, const int64_t *qh, const int64_t *kl, const int64_t *kh, int device, void *stream);
/* own (optional DEVICE table of `rows` bytes, may be NULL): own[r] = the digit (storage order) whose primes include limb
 * r, 255 for the special limbs.  The extension of a digit's mixed-radix form to one of its own primes is the residue it
 * was built from, i.e. the switched polynomial x1 * y1 itself: those (digit, limb) pairs are neither extended nor
 * transformed, and the inner product forms x1 * y1 from the stack in their place (35 of gold's 390 limb transforms).
 * lf_relin_fwd = lf_ks_fwd of digits first .. first + nparts - 1 with that table (desc / tmp are NOT offset by the caller). */
int lf_relin_fwd(const int64_t *state, int first, int nparts, int rows, int logN, const int64_t *desc, const int64_t *E,
                 const double *Ed, int64_t *tmp, const int64_t *psi_br, const double *psi_dp, const uint8_t *own,
                 const int64_t *q_host, const int64_t *ql, const int64_t *qh, const int64_t *kl, const int64_t *kh, int device,
                 void *stream);
int lf_relin_tail(int nparts, int rows, int logN, const int64_t *ksk, int64_t part_stride, int64_t comp_stride, int64_t row_off,
                  int key_format, int64_t *tmp, int64_t *s, const int64_t *ipsi_br, const double *ipsi_dp, const int64_t *Ninv,
                  const int64_t *x, const int64_t *PR, int ell, const uint8_t *own, const int64_t *q_host, const int64_t *ql, const int64_t *qh, const int64_t *kl, const int64_t *kh, int device,
                  void *stream);

/* Batched forms: `count` (<= 8) independent operand sets in ONE launch — the two components of a ciphertext, the
 * four polynomials cc_mult rescales.  The arrays of pointers are HOST arrays of device pointers; constants are
 * shared by all sets.  addend may be NULL, or hold NULL entries. */
int lf_rescale_batch(const int64_t *const *in, const int64_t *const *row0, int64_t *const *out, int count, int rows,
                     int64_t N, const int64_t *scales, int64_t round_at, const int64_t *ql, const int64_t *qh,
                     const int64_t *kl, const int64_t *kh, int device, void *stream);
int lf_ks_moddown_batch(const int64_t *const *s, int64_t *const *out, const int64_t *const *addend, int count, int ell, int K,
                        int64_t N, const int64_t *PiR, const double *PiP, const int64_t *Rs, int64_t gal_pinv,
                        const int64_t *gal_2q, const int64_t *ql, const int64_t *qh, const int64_t *kl, const int64_t *kh,
                        int device, void *stream);

/* lf_ks_moddown_batch with a caller-provided workspace `ws` of at least lf_ks_moddown_ws_words(count, ell, K, N)
 * int64 words: the elimination among the K special rows (ckks_engine.py:850-870) is evaluated once per coefficient
 * by a first launch instead of once per row chunk, and the fp64-class rows take the closed form
 * (s - sum_j p_j prod_{i<j} P_i) / P.  Same canonical outputs; s is not modified. */
int64_t lf_ks_moddown_ws_words(int count, int ell, int K, int64_t N);
int lf_ks_moddown_ws(const int64_t *const *s, int64_t *const *out, const int64_t *const *addend, int count, int ell, int K,
                     int64_t N, int64_t *ws, int64_t ws_words, const int64_t *PiR, const double *PiP, const int64_t *Rs,
                     int64_t gal_pinv, const int64_t *gal_2q, const int64_t *ql, const int64_t *qh, const int64_t *kl,
                     const int64_t *kh, int device, void *stream);
/* The same in ONE launch for K <= LF_MODDOWN_ONE_MAX_K special primes: every block eliminates the special rows for its own
 * coefficients (K = 2: one REDC product per coefficient and row chunk — cheaper than a launch).  The per-row constants that
 * lf_ks_moddown_ws writes behind the pivots on every call are level constants: lf_ks_moddown_consts writes them ONCE into a
 * workspace, lf_ks_moddown_one only reads them (the pivot part of the workspace is not used).  Same outputs. */
#define LF_MODDOWN_ONE_MAX_K 2
int lf_ks_moddown_consts(int64_t *ws, int64_t ws_words, int count, int ell, int K, int64_t N, const double *PiP, const int64_t *ql,
                         const int64_t *qh, const int64_t *kl, const int64_t *kh, int device, void *stream);
int lf_ks_moddown_one(const int64_t *const *s, int64_t *const *out, const int64_t *const *addend, int count, int ell, int K,
                      int64_t N, const int64_t *ws, int64_t ws_words, const int64_t *PiR, const double *PiP, const int64_t *Rs,
                      int64_t gal_pinv, const int64_t *gal_2q, const int64_t *ql, const int64_t *qh, const int64_t *kl,
                      const int64_t *kh, int device, void *stream);

/* Galois permutation in gather form, so that rotate / conjugate need no permutation pass of their own
 * (switch_key / rotate_single, ckks_engine.py:939-961, 1180-1206; encdec.py:224-270):
 *   lf_ks_digits_galois  = lf_ks_digits of a(X^p);  lf_ks_moddown_batch with gal_pinv != 0 adds addend(X^p).
 * gal_pinv = p^-1 mod 2N (0: no permutation); gal_2q != NULL: the permuted words are made canonical as
 * rotate_single does (make_unsigned + reduce_2q), NULL: they stay signed as conjugate leaves them. */
int lf_ks_digits_galois(const int64_t *a, int64_t *state, int nparts, const int64_t *desc, const int64_t *tab, int64_t N,
                        int64_t gal_pinv, const int64_t *gal_2q, const int64_t *ql, const int64_t *qh, const int64_t *kl,
                        const int64_t *kh, int device, void *stream);
int lf_galois_batch(const int64_t *const *a, int64_t *const *dst, int count, int rows, int logN, int64_t p,
                    const int64_t *_2q, int device, void *stream);

/* lf_intt_mul (relaxed, tail 2) followed by lf_ks_digits of its result in ONE launch behind the tiled pass: the column thread of
 * the last inverse pass takes the columns of all `alpha` limbs of its digit, runs the Garner step on the canonical words it holds
 * and stores the digit state — the coefficient-domain product is never written (cc_mult: ckks_engine.py:1099-1101, 1129, 654-705).
 * `scratch` [batch][rows][N] receives the tiled pass's output; `state` [batch][rows][N]; desc / tab = lf_ks_digits' tables for
 * `nparts` digits of at most `max_alpha` limbs.  Applies to two-pass ring degrees with max_alpha * 2^(logN - 12) <= 32 (silver,
 * bronze; <= 64 at logN 16 — gold — when batch >= 2); otherwise returns LF_ERR_ARG with nothing launched and the caller takes the two calls.  Same words in `state`. */
int lf_intt_mul_digits(int64_t *scratch, const int64_t *a, int64_t a_stride, const int64_t *b, int64_t b_stride, int batch, int rows,
                       int logN, int64_t *state, int nparts, int max_alpha, const int64_t *desc, const int64_t *tab,
                       const int64_t *ipsi_br, const double *ipsi_dp, const int64_t *q_host, const int64_t *Ninv, int flags,
                       const int64_t *ql, const int64_t *qh, const int64_t *kl, const int64_t *kh, int device, void *stream);

/* cc_mult's opening (ckks_engine.py:1085-1093): rescale `count` (<= 8) polynomials and transform them, i.e.
 * lf_rescale_batch(in, row0, {x + i*rows*N}, ...) followed by lf_ntt(x, count, ...) with the same constants.
 * For two-pass ring degrees (logN 13..17) the rescale is evaluated inside the first NTT pass: no launch and no
 * trip through HBM of its own; other degrees run the two steps one after the other.  Same results either way. */
int lf_rescale_ntt(const int64_t *const *in, const int64_t *const *row0, int count, int64_t *x, int rows, int logN,
                   const int64_t *scales, int64_t round_at, const int64_t *psi_br, const double *psi_dp,
                   const int64_t *q_host, const int64_t *Rs, int flags, const int64_t *_2q, const int64_t *ql,
                   const int64_t *qh, const int64_t *kl, const int64_t *kh, int device, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Whole engine ops behind one entry each (csrc/ckks_ops.hip).  The reference's Python engine issues ~250 extension calls
 * per cc_mult + relinearize (ckks_engine.py:1072-1151 over 654-961); a binding that wants the host side of an op to be ONE
 * native call fills an lf_ks_plan once per (device, level) — everything that does not change from call to call — and
 * hands the operands and the key per call.  The entries enqueue exactly the steps above (lf_rescale_ntt, lf_intt_mul,
 * lf_ks_digits(_galois), lf_relin_core_batch / lf_ks_core, lf_ks_moddown_ws) on `stream` and return the first failure.
 * They apply when every limb of the level lives on this device (no exchange between the digits and their extension), at the
 * key switch's ring degrees 13 <= logN <= 17: a plan with another logN gets LF_ERR_ARG before anything is launched.
 * `rows` = ell + K limbs, ordinary first: the per-row vectors and twiddle tables are those of lf_ks_core.
 * ---------------------------------------------------------------------------------------------- */
typedef struct lf_ks_plan {
    int32_t logN, ell, K, nparts;        /* ring degree, ordinary limbs at the op's level, special primes, digits */
    int32_t dig_nparts, device;          /* digits lf_ks_digits builds here (= nparts on one device) */
    int32_t max_nct;                     /* ciphertexts per batched call the scratch below is sized for (1, 2 or 4) */
    int32_t md_consts;                   /* `count` md_ws was primed for by lf_ks_moddown_consts (the op entries run
                                            lf_ks_moddown_one only for exactly that many polynomials: 2 x the ciphertexts
                                            of the call); 0 = never primed: every entry takes lf_ks_moddown_ws, which
                                            needs no preparation.  A zero-filled struct is therefore always safe. */
    int64_t round_at;                    /* cc_mult: rescale rounding threshold q_l / 2 (lf_rescale) */
    int64_t md_ws_words;
    const int64_t *ql, *qh, *kl, *kh, *_2q, *Rs, *Ninv;      /* device, [rows] */
    const int64_t *q_host;                                    /* HOST, [rows] */
    const int64_t *psi, *ipsi;                                /* compact twiddle tables of the rows */
    const double *psi_dp, *ipsi_dp;                           /* their auxiliary tables (lf_twiddle_dp) */
    const int64_t *dig_desc, *dig_tab;                        /* lf_ks_digits */
    const int64_t *ext_desc, *E;                              /* lf_ks_core */
    const double *Ed;
    const int64_t *PiR;                                       /* lf_ks_moddown */
    const double *PiP;
    const uint8_t *own;                                       /* lf_relin_*: may be NULL */
    const int64_t *rescale_scales, *PR;                       /* cc_mult only: [ell] q_l^-1 R and P R mod q_r */
    int64_t *state, *ext, *sum, *md_ws;                       /* scratch: max_nct x ([ell][N], [nparts][rows][N], [2][rows][N]); md_ws_words for 2 max_nct polynomials */
    int64_t *x4, *d2;                                         /* cc_mult only: max_nct x ([4][ell][N], [ell][N]) */
} lf_ks_plan;

/* ckks_engine.cc_mult(a, b, evk) with relinearisation, level l -> l + 1 (ckks_engine.py:1072-1151): in[0..3] = first
 * SURVIVING row of a.c0, a.c1, b.c0, b.c1 (HOST array of device pointers, as lf_rescale_batch), row0[0..3] their dropped
 * rows; the plan describes level l + 1; key addressed as in lf_ks_inner, in `key_format`; out0 / out1 [ell][N] canonical. */
int lf_cc_mult_evk(const lf_ks_plan *plan, const int64_t *const *in, const int64_t *const *row0, const int64_t *ksk,
                   int64_t part_stride, int64_t comp_stride, int64_t row_off, int key_format, int64_t *out0, int64_t *out1,
                   void *stream);

/* ckks_engine.switch_key / rotate_single / conjugate of a coefficient-domain ciphertext (c0, c1), [ell][N] each
 * (ckks_engine.py:939-961, 1180-1206, 1718-1734): out = (c0(X^p) + ks_0, ks_1) with ks = key switch of c1(X^p);
 * gal_pinv = p^-1 mod 2N (0: no automorphism), gal_canonical != 0: rotate_single's make_unsigned + reduce_2q. */
int lf_switch_key(const lf_ks_plan *plan, const int64_t *c0, const int64_t *c1, int64_t gal_pinv, int gal_canonical,
                  const int64_t *ksk, int64_t part_stride, int64_t comp_stride, int64_t row_off, int key_format, int64_t *out0,
                  int64_t *out1, void *stream);

/* The same ops for nct = 1, 2 or 4 ciphertexts under ONE key (plan->max_nct >= nct): every launch covers all of them and the
 * inner product reads each key word once for the group (lf_ks_core_batch / lf_relin_core_batch).  c0 / c1 / out0 / out1: HOST
 * arrays of nct device pointers; in / row0: 4 per ciphertext pair, in the order of lf_cc_mult_evk.  Results equal nct single calls. */
int lf_switch_key_batch(const lf_ks_plan *plan, int nct, const int64_t *const *c0, const int64_t *const *c1, int64_t gal_pinv,
                        int gal_canonical, const int64_t *ksk, int64_t part_stride, int64_t comp_stride, int64_t row_off,
                        int key_format, int64_t *const *out0, int64_t *const *out1, void *stream);
int lf_cc_mult_evk_batch(const lf_ks_plan *plan, int nct, const int64_t *const *in, const int64_t *const *row0, const int64_t *ksk,
                         int64_t part_stride, int64_t comp_stride, int64_t row_off, int key_format, int64_t *const *out0,
                         int64_t *const *out1, void *stream);

/* Hoisted rotations: ONE ciphertext (c0, c1) rotated under nr >= 1 keys, key i with the odd exponent p_host[i] < 2N (HOST array;
 * ksk / out0 / out1: HOST arrays of nr device pointers, keys addressed as in lf_ks_inner, all with the same strides and format).
 * X -> X^p permutes the NTT slots: NTT(a(X^p))[k] = NTT(a)[pi_p(k)], pi_p(k) = brev(((2 brev(k) + 1) p mod 2N - 1) / 2).  So the
 * digits of c1 are formed, extended and transformed ONCE; rotation i reads them gathered by pi_{p_i}.  Result i has exactly the words
 * of: c1' = c1 made canonical (gal_canonical: make_unsigned + reduce_2q; no permutation) -> per digit pre_extend, extend, exact
 * forward NTT -> gathered by pi_{p_i} -> mont_mult with key i's part, mont_add over the digits, intt_exit_reduce -> mod-down with
 * addend c0(X^{p_i}) made canonical as rotate_single does.  These are NOT rotate_single's words (extending the digits does not
 * commute with the sign flips of X -> X^p: the two differ by key-switch noise and decrypt alike), except for p = 1, where they are.
 * Enqueued: lf_ks_digits_galois (gal_pinv = 1) and lf_ks_fwd once, then per group of 4, 2 or 1 keys one inner-product launch over
 * the shared digits and the inverse NTT of the group's sums (plan->sum holds max_nct pairs: groups of up to min(4, max_nct) keys),
 * and one mod-down per rotation.  The digits stay in the plan's first ext slot for every group; the sums' inverse transform
 * passes through the ext slots behind it, or, where they are too small (two digits and four keys, a plan of max_nct 1),
 * through `ws` of at least lf_rotate_hoisted_ws_words(plan) words (0: ws may be NULL).  LF_ERR_ARG before any launch for a
 * plan lf_switch_key refuses, nr < 1, a NULL pointer, an even exponent or one outside (0, 2N), or a workspace too small. */
int64_t lf_rotate_hoisted_ws_words(const lf_ks_plan *plan);
int lf_rotate_hoisted(const lf_ks_plan *plan, const int64_t *c0, const int64_t *c1, int nr, const int64_t *p_host, int gal_canonical,
                      const int64_t *const *ksk, int64_t part_stride, int64_t comp_stride, int64_t row_off, int key_format, int64_t *ws,
                      int64_t ws_words, int64_t *const *out0, int64_t *const *out1, void *stream);

/* Linear transform by the diagonal method ("double hoisting"): out = rescale(moddown(sum_i pt_i * (ks_i + P c0(X^p_i)))), the
 * ciphertext that decrypts to sum_i diag_i * rot(m, step_i) one level below (c0, c1).  nr >= 0 keys with odd exponents p_host[i]
 * < 2N (HOST arrays as lf_rotate_hoisted); pt: the nr encoded diagonals in key order, pt + i * pt_stride = [ell + K][N] words in
 * the NTT domain and Montgomery form over the ordinary AND the special rows; pt0: the diagonal of step 0 or NULL — that term
 * needs no key (nr = 0 with pt0 is legal).  Multiplication by a plaintext and addition commute with the mod-down, so the diagonals
 * are multiplied in while the key-switch sums are still in the NTT domain over Q P and everything behind the inner product happens
 * once.  The result has exactly the words of: c0, c1 made canonical; E = per digit pre_extend(c1), extend, exact forward NTT;
 * c^ = P * enter_ntt(c) on the ordinary rows; per key t_c = sum over the digits of E gathered by pi_{p_i} times the key part
 * (mont_mult, mont_add), t_0 += c^0 gathered by pi_{p_i} on the ordinary rows; step 0: t_c = c^c, zero on the special rows;
 * S_c = sum_i mont_mult(pt_i, t_c); intt_exit_reduce, mod-down (no addend), ckks_engine.rescale.  Only the residues of S_c reach
 * the result, so the kernels use the relaxed arithmetic of the other fused ops.
 * Enqueued: a canonical copy of c0 (c1 with pt0), ONE forward NTT of it (enter_ntt) on the ell ordinary rows and the product with
 * plan->PR; lf_ks_digits_galois (gal_pinv = 1) and lf_ks_fwd once (nr > 0); per group of 4, 2 or 1 keys one launch of
 * ks_inner_lt_kernel, all groups adding into the ONE pair plan->sum (nr = 0: one launch without keys); one inverse NTT of the
 * pair (its planes pass through plan->ext, which is spent by then); one mod-down; one lf_rescale_batch with rescale_scales /
 * round_at of the level the ciphertext leaves ([ell - 1] words q_l^-1 R; plan->rescale_scales is the level's INCOMING one) into
 * out0 / out1 [ell - 1][N].  P c^ and the mod-down's [2][ell][N] result live in plan->x4 (free during this op) or, with
 * plan->x4 = NULL, in `ws` of at least lf_linear_transform_ws_words(plan) words (0: ws may be NULL).
 * LF_ERR_ARG before any launch for everything lf_rotate_hoisted refuses (nr < 0 instead of nr < 1), a NULL pt with nr > 0,
 * nr = 0 without pt0, a NULL rescale_scales, plan->PR = NULL, ell < 2 (no level left to rescale into) and, where words are needed,
 * a workspace not 16-byte aligned (ks_inner_lt_kernel reads P c^ in 16-byte column pairs). */
int64_t lf_linear_transform_ws_words(const lf_ks_plan *plan);
int lf_linear_transform(const lf_ks_plan *plan, const int64_t *c0, const int64_t *c1, int nr, const int64_t *p_host,
                        const int64_t *const *ksk, int64_t part_stride, int64_t comp_stride, int64_t row_off, int key_format,
                        const int64_t *pt, int64_t pt_stride, const int64_t *pt0, const int64_t *rescale_scales, int64_t round_at,
                        int64_t *ws, int64_t ws_words, int64_t *out0, int64_t *out1, void *stream);

/* lf_linear_transform for nct ciphertexts under the SAME diagonals and keys.  c0 / c1 / out0 / out1: HOST arrays of nct device
 * pointers (a ciphertext may appear several times); everything else means what it means in lf_linear_transform.  Output t has
 * exactly the words of lf_linear_transform on ciphertext t.  The ciphertexts are taken in groups of min(4, plan->max_nct), then 2,
 * then 1; a group of one IS lf_linear_transform.  Enqueued per group of g = 4 or 2: canonical copies of the g c0 (c1 with pt0),
 * ONE forward NTT of them (enter_ntt) on the ell ordinary rows and the products with plan->PR; lf_ks_digits_batch (gal_pinv = 1)
 * into plan->state + t ell N and ONE extension + forward NTT of all g nparts digits into plan->ext (nr > 0); per chunk of
 * 8 keys (csrc/ckks_ks.hip: LF_LTB_KEYS) one launch of ks_inner_ltb_kernel, which loops over the chunk's keys itself, loads every key and diagonal word once for the g ciphertexts and keeps their g running pairs in
 * registers, all launches adding into the g pairs plan->sum (nr = 0: one launch without keys); ONE inverse NTT of the 2 g
 * polynomials (their planes pass through plan->ext, which is spent by then); ONE mod-down and ONE lf_rescale_batch of the 2 g
 * polynomials into out0[t] / out1[t] [ell - 1][N].  The g (P c^0, P c^1) and the mod-down's [2 g][ell][N] result live in the
 * group's slots of plan->x4 ([max_nct][4][ell][N], free during this op) or, with plan->x4 = NULL, in `ws` of at least
 * lf_linear_transform_batch_ws_words(plan, nct) words (0: ws may be NULL; it grows with the largest group, not with nct; 0 also
 * for a plan or an nct the op refuses), 16-byte aligned.
 * LF_ERR_ARG before any launch for everything lf_linear_transform refuses, nct < 1 or > LF_LT_BATCH_MAX_CTS, a NULL among the
 * pointer arrays or their entries, and a workspace that is NULL where words are needed, misaligned or too small. */
#define LF_LT_BATCH_MAX_CTS 64
int64_t lf_linear_transform_batch_ws_words(const lf_ks_plan *plan, int nct);
int lf_linear_transform_batch(const lf_ks_plan *plan, int nct, const int64_t *const *c0, const int64_t *const *c1,
                              int nr, const int64_t *p_host, const int64_t *const *ksk, int64_t part_stride,
                              int64_t comp_stride, int64_t row_off, int key_format, const int64_t *pt, int64_t pt_stride,
                              const int64_t *pt0, const int64_t *rescale_scales, int64_t round_at, int64_t *ws,
                              int64_t ws_words, int64_t *const *out0, int64_t *const *out1, void *stream);

/* Rotation sum: out = moddown(sum_i (ks_i + P c0(X^p_i)) [+ P (c0, c1)]), the ciphertext that decrypts to sum_i rot(m, step_i)
 * [+ m] at the SAME level as (c0, c1): lf_linear_transform without the diagonals and without the rescale.  nr >= 0 keys with odd
 * exponents p_host[i] < 2N (HOST arrays as lf_rotate_hoisted; a key may repeat, p = 1 is legal, and so is the conjugation's
 * p = 2N - 1 with its key); with_self != 0 adds the ciphertext itself, which needs no key (nr = 0 with with_self is legal).
 * Addition commutes with the mod-down, so the key-switch sums of all rotations are added while still in the NTT domain over Q P
 * and everything behind the inner product happens once.  The result has exactly the words of: c0, c1 made canonical; E = per
 * digit pre_extend(c1), extend, exact forward NTT; c^ = P * enter_ntt(c) on the ordinary rows; per key t_c = sum over the digits
 * of E gathered by pi_{p_i} times the key part (mont_mult, mont_add), t_0 += c^0 gathered by pi_{p_i} on the ordinary rows; self
 * term: t_c = c^c, zero on the special rows; S_c = sum of the t_c; intt_exit_reduce, mod-down (no addend).  Only the residues of
 * S_c reach the result, so the kernel is free in the order of its additions and uses the relaxed arithmetic of the other fused ops.
 * Enqueued: a canonical copy of c0 (and of c1 with with_self), ONE forward NTT of it (enter_ntt) on the ell ordinary rows and the
 * product with plan->PR; lf_ks_digits_galois (gal_pinv = 1) and lf_ks_fwd once (nr > 0); per group of 4, 2 or 1 keys one launch
 * of ks_inner_rsum_kernel, all groups adding into the ONE pair plan->sum (nr = 0: one launch without keys); one inverse NTT of
 * the pair (its planes pass through plan->ext, which is spent by then); one mod-down without addend straight into out0 / out1
 * [ell][N], canonical.  No rescale.  P c^ lives in plan->x4 (free during this op) or, with plan->x4 = NULL, in `ws` of at least
 * lf_rotate_sum_ws_words(plan) words (0: ws may be NULL).
 * LF_ERR_ARG before any launch for everything lf_rotate_hoisted refuses (nr < 0 instead of nr < 1), nr = 0 without with_self,
 * plan->PR = NULL and a workspace too small or, where words are needed, not 16-byte aligned (ks_inner_rsum_kernel reads P c^ in
 * 16-byte column pairs). */
int64_t lf_rotate_sum_ws_words(const lf_ks_plan *plan);
int lf_rotate_sum(const lf_ks_plan *plan, const int64_t *c0, const int64_t *c1, int nr, const int64_t *p_host,
                  const int64_t *const *ksk, int64_t part_stride, int64_t comp_stride, int64_t row_off, int key_format,
                  int with_self, int64_t *ws, int64_t ws_words, int64_t *out0, int64_t *out1, void *stream);

/* lf_rotate_sum for nct ciphertexts under the SAME keys.  c0 / c1 / out0 / out1: HOST arrays of nct device pointers (a ciphertext
 * may appear several times); everything else means what it means in lf_rotate_sum.  Output t has exactly the words of
 * lf_rotate_sum on ciphertext t.  The ciphertexts are taken in groups of min(4, plan->max_nct), then 2, then 1, as
 * lf_linear_transform_batch takes them; a group of one IS lf_rotate_sum, with the first slot of this call's scratch as its own.
 * Enqueued per group of g = 4 or 2: canonical copies of the g c0 (c1 with with_self), ONE forward NTT of them (enter_ntt) on the
 * ell ordinary rows and the products with plan->PR; lf_ks_digits_batch (gal_pinv = 1) into plan->state + t ell N and ONE
 * extension + forward NTT of all g nparts digits into plan->ext (nr > 0); per chunk of 8 keys (csrc/ckks_ks.hip: LF_RSB_KEYS) one
 * launch of ks_inner_rsumb_kernel, which loops over the chunk's keys itself, loads every key word once for the g ciphertexts and
 * keeps ONE accumulator pair per ciphertext for all keys of the launch, all launches adding into the g pairs plan->sum (nr = 0:
 * one launch without keys); ONE inverse NTT of the 2 g polynomials (their planes pass through plan->ext, which is spent by
 * then); ONE mod-down without addend of the 2 g polynomials straight into out0[t] / out1[t] [ell][N], canonical.  No rescale.
 * The g (P c^0, P c^1) live in the group's slots of plan->x4 ([max_nct][4][ell][N], free during this op) or, with
 * plan->x4 = NULL, in `ws` of at least lf_rotate_sum_batch_ws_words(plan, nct) words (2 g ell N for the largest group; 0: ws may
 * be NULL; it grows with the largest group, not with nct; 0 also for a plan or an nct the op refuses), 16-byte aligned.
 * LF_ERR_ARG before any launch for everything lf_rotate_sum refuses, nct < 1 or > LF_LT_BATCH_MAX_CTS, a NULL among the pointer
 * arrays or their entries, and a workspace that is NULL where words are needed, misaligned or too small. */
int64_t lf_rotate_sum_batch_ws_words(const lf_ks_plan *plan, int nct);
int lf_rotate_sum_batch(const lf_ks_plan *plan, int nct, const int64_t *const *c0, const int64_t *const *c1,
                        int nr, const int64_t *p_host, const int64_t *const *ksk, int64_t part_stride,
                        int64_t comp_stride, int64_t row_off, int key_format, int with_self, int64_t *ws,
                        int64_t ws_words, int64_t *const *out0, int64_t *const *out1, void *stream);

/* Linear transform by the diagonal method in its baby-step / giant-step form: out decrypts to
 *     sum_g rot( sum_b diag_{g+b}(rolled by -g) * rot(m, b), g )        b = step mod n1, g = step - b,
 * so that k diagonals need about n1 + k / n1 rotation keys (and key streams) instead of k.  nb >= 0 baby keys with odd
 * exponents bp_host[i] < 2N and ng >= 1 giant steps (HOST arrays): gp_host[i] is the exponent of giant step i and gksk[i] its
 * key, or gp_host[i] = 0 for the giant step 0, which has no key (gksk[i] is not read), comes first and at most once.  Baby SLOT
 * 0 is the ciphertext itself (baby step 0, no key), slot 1 + i is baby key i.  pt: the pack of encoded diagonals as
 * ckks_engine.encode_diagonals(.., bsgs=n1) lays it out — [ell + K][N] words each at stride pt_stride, NTT domain, Montgomery
 * form, giant step after giant step: gcount[i] >= 1 diagonals belong to giant step i, and bidx holds, in pack order, the baby
 * slot of every diagonal (0 .. nb, strictly ascending inside a giant step).
 * The result has exactly the words of: c0, c1 made canonical; E and c^ as lf_linear_transform forms them; per baby key
 * u^b_c = sum over the digits of E gathered by pi_b times the key part, u^b_0 += c^0 gathered on the ordinary rows (slot 0:
 * u_c = c^c, zero on the special rows); per giant step S^g_c = sum_b mont_mult(pt_{g,b}, u^b_c); giant step 0: S joins the
 * accumulator A; else w = mod-down (no addend) of intt_exit_reduce(S^g_1), made canonical, E^g its digits extended and
 * transformed, v_c = sum over the digits of E^g gathered by pi_g times key g's part, v_0 += S^g_0 gathered on ALL ell + K rows
 * (S^g_0 stays in Q P), A += v; intt_exit_reduce(A), mod-down (no addend), ckks_engine.rescale.  The gather stands before the
 * key product because rotation keys here switch s(X^p) -> s.  Only residues of u, S, v and A reach the result.
 * Enqueued: the canonical copies, enter_ntt and the product with plan->PR of c0 and c1 into slot 0; lf_ks_digits_galois and
 * lf_ks_fwd once (nb > 0) and per group of 4, 2 or 1 baby keys one launch of ks_inner_baby_kernel; per group of 4, 2 or 1 giant
 * steps one launch of lt_diag_products_kernel (the baby pairs cross HBM once per launch), then per keyed giant step the inverse
 * NTT of S^g_1, lf_ks_moddown_ws for one polynomial, lf_ks_digits_galois (gal_pinv = 1), lf_ks_fwd and one launch of
 * ks_inner_giant_kernel into A; one inverse NTT of A, one mod-down, one lf_rescale_batch into out0 / out1 [ell - 1][N].
 * The baby pairs, four S pairs, A, w and the mod-down's buffers do not fit the plan's scratch: `ws` of at least
 * lf_linear_transform_bsgs_ws_words(plan, nb) words is lent by the caller (0 for a plan or an nb the entry refuses).
 * LF_ERR_ARG before any launch for everything lf_linear_transform refuses, nb < 0 or > 63, ng < 1, a baby slot out of range or
 * not ascending inside its giant step, a giant step without diagonals, a second or a late giant step 0, a workspace too small
 * or not 16-byte aligned (lt_diag_products_kernel reads the baby pairs and writes S and A in 16-byte column pairs). */
int64_t lf_linear_transform_bsgs_ws_words(const lf_ks_plan *plan, int nb);
int lf_linear_transform_bsgs(const lf_ks_plan *plan, const int64_t *c0, const int64_t *c1, int nb, const int64_t *bp_host,
                             const int64_t *const *bksk, int ng, const int64_t *gp_host, const int64_t *const *gksk,
                             int64_t part_stride, int64_t comp_stride, int64_t row_off, int key_format, const int64_t *pt,
                             int64_t pt_stride, const int64_t *gcount, const int64_t *bidx, const int64_t *rescale_scales,
                             int64_t round_at, int64_t *ws, int64_t ws_words, int64_t *out0, int64_t *out1, void *stream);

/* lf_linear_transform_bsgs for nct ciphertexts under the SAME diagonals and keys.  c0 / c1 / out0 / out1: HOST arrays of nct
 * device pointers (a ciphertext may appear several times); everything else means what it means in lf_linear_transform_bsgs.
 * Output t has exactly the words of lf_linear_transform_bsgs on ciphertext t.  The ciphertexts are taken in groups of
 * min(4, plan->max_nct), then 2, then 1, as lf_linear_transform_batch takes them; a group of one IS lf_linear_transform_bsgs.
 * Enqueued per group of g = 4 or 2: canonical copies of the 2 g polynomials, ONE forward NTT of them (enter_ntt) on the ell
 * ordinary rows, the products with plan->PR, each copied into slot 0 of its member, zero on the special rows; with nb > 0
 * lf_ks_digits_batch (gal_pinv = 1) into plan->state + t ell N, ONE extension + forward NTT of all g nparts digits into
 * plan->ext, and per baby key ONE launch of ks_inner_babyb_kernel<g> into the g slots of that key (the key crosses HBM once for
 * the group); per group of 4, 2 or 1 giant steps one launch of lt_diag_products_kernel PER MEMBER (the diagonals are read once
 * per member), then per keyed giant step of that group the inverse NTT of each member's S^g_1, ONE lf_ks_moddown_ws of the g
 * polynomials, ONE lf_ks_digits_batch, ONE extension + forward NTT and ONE launch of ks_inner_giantb_kernel<g> adding into the
 * g accumulators (the steps lf_lt_matmul_bsgs takes for outputs that share a giant step); ONE inverse NTT of the g accumulator
 * pairs, ONE mod-down of the 2 g polynomials, ONE lf_rescale_batch into out0[t] / out1[t] [ell - 1][N].
 * `ws`, lent by the caller and 16-byte aligned, holds at least lf_linear_transform_bsgs_batch_ws_words(plan, nb, nct) words:
 * per member of the largest group its nb + 1 baby pairs, four S pairs and the accumulator, then the g polynomials w, the
 * mod-down's [2 g][ell][N] result and the larger of the two mod-down workspaces.  It grows with the largest group, not with nct;
 * for nct = 1 it is lf_linear_transform_bsgs_ws_words(plan, nb); it is 0 for a plan, an nb or an nct the entry refuses.
 * LF_ERR_ARG before any launch for everything lf_linear_transform_bsgs refuses, nct < 1 or > LF_LT_BATCH_MAX_CTS, a NULL among
 * the pointer arrays or their entries, and a workspace that is NULL, misaligned or too small. */
int64_t lf_linear_transform_bsgs_batch_ws_words(const lf_ks_plan *plan, int nb, int nct);
int lf_linear_transform_bsgs_batch(const lf_ks_plan *plan, int nct, const int64_t *const *c0, const int64_t *const *c1, int nb,
                                   const int64_t *bp_host, const int64_t *const *bksk, int ng, const int64_t *gp_host,
                                   const int64_t *const *gksk, int64_t part_stride, int64_t comp_stride, int64_t row_off,
                                   int key_format, const int64_t *pt, int64_t pt_stride, const int64_t *gcount,
                                   const int64_t *bidx, const int64_t *rescale_scales, int64_t round_at, int64_t *ws,
                                   int64_t ws_words, int64_t *const *out0, int64_t *const *out1, void *stream);

/* A matrix of linear transforms times a vector of ciphertexts (a matrix larger than one ciphertext's slots, or a layer over
 * several packed inputs): for o < k_out, out_o decrypts to
 *     sum_{i < k_in} sum_{step in steps(o, i)} diag_{o,i,step} * rot(m_i, step),
 * level l -> l + 1.  The rotations of input i do not depend on the output: they are formed once per input and shared by every
 * output; the sums over the inputs stay in Q P and come down once per output.
 * in: HOST array of 2 k_in device pointers, [input][component] (c0, c1 of ciphertext i at the plan's level, [ell][N]); the two
 * pointers of an input NO block uses are not read (that input costs nothing).  Column i has ncol[i] in 0 .. LF_BSGS_MAX_BABY_KEYS
 * keyed steps (HOST array of k_in entries): SLOT 0 of a column is the ciphertext itself (step 0, no key), slot 1 + j its j-th
 * keyed step.  p_host / ksk: HOST arrays of sum_i ncol[i] odd exponents < 2N resp. key pointers, column after column, one key
 * layout for all (part_stride .. key_format as lf_rotate_hoisted; the same key may appear in any number of columns).
 * pt / pt_stride / bcount: HOST arrays of k_out k_in entries, row-major ([output][input]): the first diagonal of block (o, i) or
 * NULL for a zero block (bcount 0), the words between its diagonals ([ell + K][N] words each, NTT domain, Montgomery form, as
 * ckks_engine.encode_diagonals lays them out) and their number >= 1; bidx: HOST array holding, block after block in the same
 * order, the column slot of every diagonal, strictly ascending inside a block.  The same pack may serve any number of blocks.
 * out0 / out1: HOST arrays of k_out pointers, [ell - 1][N] each, canonical.
 * Output o has exactly the words of: per input i that some block uses c0, c1 made canonical, E_i and c^_i as lf_linear_transform
 * forms them; per keyed step of the column t^{i,step}_c = sum over the digits of E_i gathered by pi_step times the key part,
 * t_0 += c^_{i,0} gathered on the ordinary rows (slot 0: t_c = c^_{i,c}, zero on the special rows);
 * S^o_c = sum_i sum_step mont_mult(pt_{o,i,step}, t^{i,step}_c); intt_exit_reduce, mod-down (no addend), ckks_engine.rescale.
 * Only residues of t and S reach the result, so the grouping of the additions is free and the kernels use the relaxed arithmetic
 * of the other fused ops.  k_in = 1: output o has the words of lf_linear_transform over block (o, 0).  For k_in > 1 the words are
 * the op's own — not those of adding separate transforms, which round once per block.
 * Enqueued, input-major: per used input the canonical copies, enter_ntt and the product with plan->PR into slot 0 (as
 * lf_linear_transform_bsgs), lf_ks_digits_galois and lf_ks_fwd once and per group of 4, 2 or 1 of the column's keys one launch of
 * ks_inner_baby_kernel (ncol[i] > 0); per group of 4, 2 or 1 outputs with a block in the column ONE launch of
 * lt_block_products_kernel<4 | 2 | 1> (lt_diag_products_kernel's streaming loop: every pair of the input read once per launch,
 * each output with its own pack, stride and slot mask; the first contributing input of an output writes S^o, later ones add).
 * After the last input, per group of up to 4 outputs: one lf_intt of its 2 g polynomials, one lf_ks_moddown_ws, one
 * lf_rescale_batch.  ws: lf_lt_matmul_ws_words(plan, nb_max, k_out) words, nb_max the largest ncol[i] of a used input, 16-byte
 * aligned, lent by the caller: (nb_max + 1 + k_out) pairs [2][ell + K][N] + 2 g [ell][N] + lf_ks_moddown_ws_words(2 g, ..),
 * g = min(k_out, 4) — it does not grow with k_in; 0 for what the entry refuses.  An engine with more than
 * LF_LT_MATMUL_MAX_OUTPUTS outputs splits them over calls (each call repeats the inputs' rotations).
 * LF_ERR_ARG before any launch for everything lf_linear_transform refuses, k_in < 1 or > LF_LT_MATMUL_MAX_INPUTS, k_out < 1 or
 * > LF_LT_MATMUL_MAX_OUTPUTS, an ncol[i] out of range, a NULL among the pointers that are read (in and keys of used inputs only),
 * an output with no block, a NULL block with bcount != 0, a block with bcount < 1, a stride below (ell + K) N, a slot outside its
 * column's 0 .. ncol[i] or slots not ascending, a planes key not 16-byte aligned, ws NULL, misaligned or too small. */
#define LF_LT_MATMUL_MAX_INPUTS 64
#define LF_LT_MATMUL_MAX_OUTPUTS 64
int64_t lf_lt_matmul_ws_words(const lf_ks_plan *plan, int nb_max, int k_out);
int lf_lt_matmul(const lf_ks_plan *plan, int k_in, int k_out, const int64_t *const *in, const int64_t *ncol, const int64_t *p_host,
                 const int64_t *const *ksk, int64_t part_stride, int64_t comp_stride, int64_t row_off, int key_format,
                 const int64_t *const *pt, const int64_t *pt_stride, const int64_t *bcount, const int64_t *bidx,
                 const int64_t *rescale_scales, int64_t round_at, int64_t *ws, int64_t ws_words, int64_t *const *out0,
                 int64_t *const *out1, void *stream);

/* lf_lt_matmul over nt token vectors that share the matrix and the keys (a layer over the tokens of a sequence or the samples of
 * a batch): for t < nt, o < k_out, out_{t,o} decrypts to sum_i sum_step diag_{o,i,step} * rot(m_{t,i}, step).  ONE call is one
 * group of nt in {1, 2, 4} tokens, nt <= plan->max_nct.  in: HOST array of nt 2 k_in device pointers, [token][input][component]
 * (the pointers of an input no block uses are not read, for any token); out0 / out1: HOST arrays of nt k_out pointers,
 * [token][output]; everything else is lf_lt_matmul's, shared by all tokens.  The same polynomial may appear any number of times
 * among `in`, in one token or several.
 * Output (t, o) has exactly the words of lf_lt_matmul on token t: per (token, output) the products and the order of their
 * additions are those of the single kernels, and the transforms act on each polynomial by itself.  nt = 1 IS lf_lt_matmul (the
 * same launches).
 * Enqueued for nt = 2 | 4, input-major as lf_lt_matmul; per input some block uses: the canonical copies of the 2 nt polynomials,
 * ONE forward NTT of them on the ell ordinary rows and the products with plan->PR, into slot 0 of every token (zero on the special
 * rows); where the column has keys ONE lf_ks_digits_batch of the nt c1 into plan->state, ONE extension + forward NTT of the
 * nt nparts digits into plan->ext, and per key of the column ONE launch of ks_inner_babyb_kernel<nt> into slot 1 + j of every
 * token (lf_linear_transform_bsgs_batch's baby step: the key crosses HBM once for the group); per group of 4, 2 or 1 outputs
 * with a block in the column ONE launch of lt_block_productsb_kernel<4 | 2 | 1, 2> per tile of 2 tokens
 * (lt_block_products_kernel's loop: a thread reads the pairs of its two tokens and each diagonal word ONCE for both).  After the
 * last input the nt k_out sums S^{t,o}, token-major, in groups of up to 4: one lf_intt of the group's 2 g polynomials, one
 * lf_ks_moddown_ws, one lf_rescale_batch.
 * ws: lf_lt_matmul_batch_ws_words(plan, nb_max, k_out, nt) words, 16-byte aligned, lent by the caller: nt (nb_max + 1 + k_out)
 * pairs [2][ell + K][N] + 2 g [ell][N] + lf_ks_moddown_ws_words(2 g, ..), g = min(nt k_out, 4) — it does not grow with k_in; for
 * nt = 1 it is lf_lt_matmul_ws_words(plan, nb_max, k_out); 0 for what the entry refuses.
 * LF_ERR_ARG before any launch for everything lf_lt_matmul refuses, nt not in {1, 2, 4} or above plan->max_nct, a NULL among the
 * entries of in (used inputs) / out0 / out1 of any token, ws NULL, misaligned or too small. */
#define LF_LT_MATMUL_BATCH_MAX_TOKENS 4
int64_t lf_lt_matmul_batch_ws_words(const lf_ks_plan *plan, int nb_max, int k_out, int nt);
int lf_lt_matmul_batch(const lf_ks_plan *plan, int nt, int k_in, int k_out, const int64_t *const *in, const int64_t *ncol,
                       const int64_t *p_host, const int64_t *const *ksk, int64_t part_stride, int64_t comp_stride, int64_t row_off,
                       int key_format, const int64_t *const *pt, const int64_t *pt_stride, const int64_t *bcount, const int64_t *bidx,
                       const int64_t *rescale_scales, int64_t round_at, int64_t *ws, int64_t ws_words, int64_t *const *out0,
                       int64_t *const *out1, void *stream);

/* A matrix of baby-step / giant-step transforms times a vector of ciphertexts: lf_lt_matmul for blocks of hundreds of diagonals,
 * from the keys of the baby and the giant steps alone.  For o < k_out, out_o decrypts to
 *     sum_{i < k_in} sum_{step in steps(o, i)} diag_{o,i,step} * rot(m_i, step),   step = g + b, b = step mod n1,
 * level l -> l + 1, with the diagonals encoded as ckks_engine.encode_diagonals(.., bsgs=n1) does (rolled by -g).  The baby
 * rotations of input i do not depend on the output and are formed once per input; the giant rotation is linear, so the inner sums
 * of ALL inputs of one output are added in Q P before the giant key switch: an output pays one key switch per giant step, not one
 * per giant step and input; and the outputs that share a giant step share the stream of its key.
 * in / ncol / bp_host / bksk: the columns and their baby keys, exactly as in / ncol / p_host / ksk of lf_lt_matmul (SLOT 0 of a
 * column is the ciphertext itself, slot 1 + j its j-th keyed baby step).  ng / gp_host / gksk: the giant steps as in
 * lf_linear_transform_bsgs: gp_host[j] = 0 marks giant step 0, which comes first, at most once, and has no key.  One key layout
 * for all (part_stride .. key_format as lf_rotate_hoisted); the same key may serve as a baby and as a giant step.
 * pt / pt_stride / gcount: HOST arrays of k_out k_in ng entries, [output][input][giant]: the first diagonal of block (o, i) in
 * giant step j or NULL (gcount 0), the words between its diagonals, their number >= 1; bidx: HOST array holding, in the same
 * order, the column slot of every diagonal, strictly ascending inside one (o, i, j).
 * Output o has exactly the words of: per input i that some block uses c0, c1 made canonical, E_i and c^_i as lf_linear_transform
 * forms them; per keyed baby step b of the column u^{i,b}_c = sum over the digits of E_i gathered by pi_b times key b's part,
 * u^{i,b}_0 += c^_{i,0} gathered on the ordinary rows (b = 0: u^{i,0}_c = c^_{i,c}, zero on the special rows); per output o and
 * giant step g of its row S^{o,g}_c = sum_i sum_{b : g + b in steps(o, i)} mont_mult(pt_{o,i,g+b}, u^{i,b}_c), summed over the
 * inputs BEFORE anything comes down; g = 0: S^{o,0} joins the accumulator A^o; g != 0: w = mod-down (no addend) of
 * intt_exit_reduce(S^{o,g}_1), made canonical, E^{o,g} its digits extended and transformed, v_c = sum over the digits of E^{o,g}
 * gathered by pi_g times key g's part, v_0 += S^{o,g}_0 gathered on ALL ell + K rows, A^o += v; then intt_exit_reduce(A^o),
 * mod-down (no addend), ckks_engine.rescale.  Only residues of u, S, v and A reach the result, so the grouping of the additions
 * is free.  k_in = 1: output o has the words of lf_linear_transform_bsgs over block (o, 0); giant step 0 alone: those of
 * lf_lt_matmul over the same packs; output o depends on row o only.
 * Enqueued: (1) input-major, steps 1 - 3 of lf_lt_matmul with the pairs (o, j) that have a diagonal in the place of the outputs:
 * per used input slot 0, lf_ks_digits_galois, lf_ks_fwd and ks_inner_baby_kernel per group of its keys, then
 * lt_block_products_kernel<4 | 2 | 1> per group of targets; the target of (o, giant step 0) is the accumulator A^o itself, an
 * output without giant step 0 has A^o zeroed by one hipMemsetAsync.  (2) giant-step-major: per keyed giant step the outputs that
 * have it in groups of n = 4, 2 or 1 (n <= plan->max_nct): per polynomial one lf_intt of S_1, ONE lf_ks_moddown_ws for the n
 * polynomials, ONE lf_ks_digits_batch into plan->state, ONE extension + forward NTT of all n nparts digits into plan->ext, ONE
 * launch of ks_inner_giantb_kernel<n> (every key word read once for the group; n = 1: ks_inner_giant_kernel).  (3) per group of
 * up to 4 outputs one lf_intt of its 2 g accumulator polynomials, one lf_ks_moddown_ws, one lf_rescale_batch.
 * ws: lf_lt_matmul_bsgs_ws_words(plan, nb_max, k_out, keyed_sums) words, 16-byte aligned, lent by the caller — nb_max the largest
 * ncol[i] of a used input, keyed_sums the pairs (o, j) with gp_host[j] != 0 that have a diagonal:
 *     (nb_max + 1 + k_out + keyed_sums) pairs [2][ell + K][N] + gw [ell][N] + 2 g4 [ell][N]
 *         + max(lf_ks_moddown_ws_words(gw, ..), lf_ks_moddown_ws_words(2 g4, ..)),   g4 = min(k_out, 4), gw = min(4, plan->max_nct);
 * 0 for what the entry refuses.  An engine with more outputs, giant steps or keyed sums than one call takes splits the outputs
 * over calls (each call repeats the inputs' baby steps).
 * LF_ERR_ARG before any launch for everything lf_lt_matmul and lf_linear_transform_bsgs refuse, ng < 1 or
 * > LF_LT_MATMUL_BSGS_MAX_GIANTS, more than LF_LT_MATMUL_BSGS_MAX_SUMS keyed sums, an (o, i, j) with a NULL pack and a count or
 * the other way round, an output with no diagonal at all, a keyed giant step no output uses. */
#define LF_LT_MATMUL_BSGS_MAX_GIANTS 64
#define LF_LT_MATMUL_BSGS_MAX_SUMS 256
int64_t lf_lt_matmul_bsgs_ws_words(const lf_ks_plan *plan, int nb_max, int k_out, int keyed_sums);
int lf_lt_matmul_bsgs(const lf_ks_plan *plan, int k_in, int k_out, const int64_t *const *in, const int64_t *ncol, const int64_t *bp_host,
                      const int64_t *const *bksk, int ng, const int64_t *gp_host, const int64_t *const *gksk, int64_t part_stride,
                      int64_t comp_stride, int64_t row_off, int key_format, const int64_t *const *pt, const int64_t *pt_stride,
                      const int64_t *gcount, const int64_t *bidx, const int64_t *rescale_scales, int64_t round_at, int64_t *ws,
                      int64_t ws_words, int64_t *const *out0, int64_t *const *out1, void *stream);

/* lf_lt_matmul_bsgs over nt token vectors that share the matrix, the baby keys and the giant keys: for t < nt, o < k_out,
 * out_{t,o} decrypts to sum_i sum_step diag_{o,i,step} * rot(m_{t,i}, step).  ONE call is one group of nt in {1, 2, 4} tokens,
 * nt <= plan->max_nct.  in: HOST array of nt 2 k_in device pointers, [token][input][component] (the pointers of an input no block
 * uses are not read, for any token); out0 / out1: HOST arrays of nt k_out pointers, [token][output]; everything else is
 * lf_lt_matmul_bsgs's, shared by all tokens; keyed_sums and the caps (LF_LT_MATMUL_MAX_OUTPUTS, LF_LT_MATMUL_BSGS_MAX_GIANTS,
 * LF_LT_MATMUL_BSGS_MAX_SUMS) count per token.  The same polynomial may appear any number of times among `in`.
 * Output (t, o) has exactly the words of lf_lt_matmul_bsgs on token t: only residues of u, S, v and A reach the result, and the
 * transforms act on each polynomial by itself.  nt = 1 IS lf_lt_matmul_bsgs (the same launches).
 * Enqueued for nt = 2 | 4: (1) input-major, per input some block uses, steps 1 - 2 of lf_lt_matmul_batch: the canonical copies
 * and ONE forward NTT of the 2 nt polynomials into slot 0 of every token (zero on the special rows); where the column has baby
 * keys ONE lf_ks_digits_batch, ONE extension + forward NTT of the nt nparts digits and per baby key ONE launch of
 * ks_inner_babyb_kernel<nt> into slot 1 + j of every token.  Then lf_lt_matmul_bsgs's products: the pairs (o, j) that have a
 * diagonal in the column, those of giant step 0 and the keyed ones apart (the accumulators A [nt][k_out] and the keyed sums
 * S [nt][keyed_sums] have different token strides and a launch takes one), each kind in groups of 4, 2 or 1 through
 * lt_block_productsb_kernel<4 | 2 | 1, 2>, one launch per tile of 2 tokens; the target of (o, giant step 0) is token t's
 * accumulator A^{t,o} itself, an accumulator without giant step 0 is zeroed by one hipMemsetAsync.  (2) giant-step-major: per
 * keyed giant step the members (t, o) that have it, output-major with the tokens of an output adjacent, in chunks of n = 4, 2 or 1
 * (n <= plan->max_nct), each through lf_lt_matmul_bsgs's giant step: per member one lf_intt of S_1, then for the chunk ONE
 * lf_ks_moddown_ws, ONE lf_ks_digits_batch, ONE extension + forward NTT and ONE launch of ks_inner_giantb_kernel<n> — with
 * nt = 4 a chunk is the four tokens of one output, with nt = 2 a chunk of 4 is two outputs x two tokens: the giant key is read
 * once for 4 members whatever k_out is.  (3) the nt k_out accumulators, token-major, in groups of up to 4 (a group may span two
 * tokens): one lf_intt of the group's 2 g polynomials, one lf_ks_moddown_ws, one lf_rescale_batch.
 * ws: lf_lt_matmul_bsgs_batch_ws_words(plan, nb_max, k_out, keyed_sums, nt) words, 16-byte aligned, lent by the caller:
 *     nt (nb_max + 1 + k_out + keyed_sums) pairs [2][ell + K][N] + gw [ell][N] + 2 g4 [ell][N]
 *         + max(lf_ks_moddown_ws_words(gw, ..), lf_ks_moddown_ws_words(2 g4, ..)),   g4 = min(nt k_out, 4), gw = min(4, plan->max_nct)
 * — it does not grow with k_in; for nt = 1 it is lf_lt_matmul_bsgs_ws_words(plan, nb_max, k_out, keyed_sums); 0 for what the
 * entry refuses.
 * LF_ERR_ARG before any launch for everything lf_lt_matmul_bsgs refuses, nt not in {1, 2, 4} or above plan->max_nct, a NULL among
 * the entries of in (used inputs) / out0 / out1 of any token, ws NULL, misaligned or too small. */
#define LF_LT_MATMUL_BSGS_BATCH_MAX_TOKENS 4
int64_t lf_lt_matmul_bsgs_batch_ws_words(const lf_ks_plan *plan, int nb_max, int k_out, int keyed_sums, int nt);
int lf_lt_matmul_bsgs_batch(const lf_ks_plan *plan, int nt, int k_in, int k_out, const int64_t *const *in, /* [token][input][component] */
                            const int64_t *ncol, const int64_t *bp_host, const int64_t *const *bksk, int ng, const int64_t *gp_host,
                            const int64_t *const *gksk, int64_t part_stride, int64_t comp_stride, int64_t row_off, int key_format,
                            const int64_t *const *pt, const int64_t *pt_stride, const int64_t *gcount, const int64_t *bidx,
                            const int64_t *rescale_scales, int64_t round_at, int64_t *ws, int64_t ws_words,
                            int64_t *const *out0, int64_t *const *out1 /* [token][output] */, void *stream);

/* Sum of ciphertext products under ONE relinearisation ("lazy relinearisation"): out decrypts to sum_i a_i * b_i, level l -> l + 1.
 * np >= 1 pairs; in / row0: HOST arrays of 4 np device pointers, four per pair in the order of lf_cc_mult_evk (first surviving
 * row resp. dropped row of a_i.c0, a_i.c1, b_i.c0, b_i.c1; the same polynomial may appear any number of times); the plan
 * describes level l + 1; key as for lf_cc_mult_evk; out0 / out1 [ell][N] canonical.
 * The result has exactly the words of ckks_engine's
 *     t = cc_mult(a_0, b_0, relin=False);  t = cc_add_triplet(t, cc_mult(a_i, b_i, relin=False)) for i >= 1;  relinearize(t, evk)
 * i.e. per pair rescale, exact forward NTT, tensor product (d0, d1, d2); mont_add of the triplets; intt_exit_reduce of the three
 * sums; key switch of d2 with the addends d0, d1.  np = 1: lf_cc_mult_evk's words.  Everything but the tensor products is linear
 * in the triplet and runs once, on the sum; only the residues of the summed triplet T reach the result (its consumers — the
 * inverse transform of T2 and the folded inner product — reduce), so T is kept in the relaxed representation of the other
 * fused ops: plain canonical residues on fp64-class rows, Montgomery-form words below 2q on integer-class rows.
 * Enqueued: per chunk of 4, 2 or 1 pairs (at most plan->max_nct) lf_rescale_ntt of up to 8 polynomials per call into plan->x4
 * (RELAXED | PLAIN, PLANES where lf_stack_planes says so) and ONE launch of dot_tensor_kernel adding the chunk's triplets into
 * T = [3][ell][N] (the first chunk writes; the last also leaves a copy of T2 in plan->d2); lf_intt (tail 2, relaxed, plain) of
 * that copy and lf_ks_digits into plan->state; the extension + forward NTT of the digits (own-limb pairs skipped, as
 * lf_relin_fwd) and ONE launch of ks_inner2_presum_kernel — the inner product with the key whose sums receive P T0 and P T1 on
 * the ordinary rows and whose own-limb digit words are T2's — with the inverse NTT of plan->sum; one mod-down, no addend.
 * T lives in `ws` of at least lf_cc_dot_ws_words(plan) = 3 ell N words, lent by the caller (0 for a plan the entry refuses).
 * LF_ERR_ARG before any launch for everything lf_cc_mult_evk refuses, np < 1, a NULL among the 4 np pointers of in or row0, a
 * key_format that is neither LF_KEY_RAW nor LF_KEY_PLANES (or a planes key not 16-byte aligned), ws NULL, not 16-byte aligned (dot_tensor_kernel reads and writes T in
 * 16-byte column pairs) or too small. */
int64_t lf_cc_dot_ws_words(const lf_ks_plan *plan);
int lf_cc_dot(const lf_ks_plan *plan, int np, const int64_t *const *in, const int64_t *const *row0, const int64_t *ksk,
              int64_t part_stride, int64_t comp_stride, int64_t row_off, int key_format, int64_t *ws, int64_t ws_words, int64_t *out0,
              int64_t *out1, void *stream);

/* nd = 1, 2 or 4 independent dots under ONE key (nd <= plan->max_nct, the rule of lf_cc_mult_evk_batch): dot d has np_host[d] >= 1
 * pairs (HOST array of nd entries); in / row0: HOST arrays of 4 sum_d np_host[d] device pointers, four per pair in lf_cc_dot's
 * order, all pairs of dot 0, then those of dot 1, and so on; out0 / out1: HOST arrays of nd device pointers, [ell][N] each, canonical.
 * Output d has exactly the words of lf_cc_dot on dot d's pairs.
 * Enqueued: per dot lf_cc_dot's chunks — lf_rescale_ntt into plan->x4 and dot_tensor_kernel into that dot's triplet
 * T_d = ws + d * 3 ell N, the last chunk of dot d leaving its copy of T2 at plan->d2 + d * ell N; ONE lf_intt (batch nd, tail 2,
 * relaxed, plain) of the nd copies and ONE lf_ks_digits_batch into plan->state (stride ell N); ONE extension + forward NTT of all
 * nd x nparts digits (own-limb pairs skipped) and ONE launch of ks_dotb_inner_kernel<nd> — the pre-summed fold of
 * ks_inner2_presum_kernel for nd triplets, every key word read once for all of them — with the inverse NTT of the 2 nd sums in
 * plan->sum; ONE mod-down of the 2 nd sums, no addend (in one launch where plan->md_consts = 2 nd).  nd = 1: lf_cc_dot's launches.
 * The triplets live in `ws` of at least lf_cc_dot_batch_ws_words(plan, nd) = 3 nd ell N words, lent by the caller (0 for a plan
 * or an nd the entry refuses).
 * LF_ERR_ARG before any launch for everything lf_cc_dot refuses, nd not 1, 2 or 4 or above plan->max_nct, np_host NULL or an entry
 * below 1, a NULL among the 4 sum np pointers of in or row0 or among the nd of out0 or out1, ws NULL, not 16-byte aligned or too small. */
int64_t lf_cc_dot_batch_ws_words(const lf_ks_plan *plan, int nd);
int lf_cc_dot_batch(const lf_ks_plan *plan, int nd, const int64_t *np_host, const int64_t *const *in, const int64_t *const *row0,
                    const int64_t *ksk, int64_t part_stride, int64_t comp_stride, int64_t row_off, int key_format, int64_t *ws,
                    int64_t ws_words, int64_t *const *out0, int64_t *const *out1, void *stream);

/* A matrix of ciphertexts times a matrix of ciphertexts under ONE key: C[i][j] = sum_t A[i][t] * B[t][j], slot-wise, level l -> l + 1;
 * A is m x k, B is k x n (attention scores, a bilinear layer, many small matrix products packed slot-wise).
 * The nu DISTINCT operand ciphertexts: in / row0 are HOST arrays of 2 nu device pointers, [operand][component], in lf_cc_dot's
 * convention (first surviving row resp. dropped row of c0, c1 at level l).  ia[i * k + t] / ib[t * n + j]: HOST tables of the
 * operand in 0 .. nu - 1 that is A[i][t] resp. B[t][j], or -1 for a zero entry; an operand may appear anywhere in both, any number
 * of times.  Key as for lf_cc_dot; out0 / out1: HOST arrays of m n device pointers, [i * n + j], [ell][N] each, canonical.
 * Output (i, j) has exactly the words of lf_cc_dot on the pairs (A[i][t], B[t][j]) over the t where neither is a zero entry.
 * Enqueued: (1) every distinct operand rescaled and forward-transformed ONCE — lf_rescale_ntt (RELAXED | PLAIN, PLANES where
 * lf_stack_planes says so), 4 operands (8 polynomials) per call — into a resident store [nu][2][ell][N] at the head of `ws`
 * (lf_cc_dot_batch transforms both operands of every pair of every dot: 2 m k n ciphertexts where m k + k n are distinct).
 * (2) C is cut into tiles of R x C outputs, R C = 4, 2 or 1 and at most plan->max_nct: 2 x 2 where both dimensions allow it (and
 * max_nct >= 4), strips of 1 x 4 / 4 x 1, 1 x 2 / 2 x 1 and 1 x 1 along a vector, an odd last column or row; per tile ONE launch
 * of matmul_tensor_kernel<R, C>, which loads the R + C operands of an inner index once, sums the R C triplets over the whole inner
 * dimension in registers and writes each once: T_d at ws + (2 nu + 3 d) ell N, its copy of T2 at plan->d2 + d ell N.  (3) per tile
 * steps 3 to 5 of lf_cc_dot_batch for nd = R C (nd = 1: of lf_cc_dot): lf_intt of the copies, their digits, the pre-summed fold
 * under the key, one mod-down.
 * ws: lf_cc_matmul_ws_words(plan, nu) = (2 nu + 3 g) ell N words, g = min(4, plan->max_nct), 16-byte aligned, lent by the caller
 * (0 for a plan or an nu the entry refuses).  An engine with more distinct operands than one call takes splits C by row blocks of
 * A over several calls; the inner dimension is never split.
 * LF_ERR_ARG before any launch for everything lf_cc_dot refuses, m, k or n below 1, k above LF_CC_MATMUL_MAX_INNER, nu outside
 * 1 .. LF_CC_MATMUL_MAX_OPERANDS, ia or ib NULL or an entry outside -1 .. nu - 1, an operand that no entry uses, a NULL among the
 * 2 nu pointers of in or row0, an output with no term, a NULL among the m n pointers of out0 or out1, ws NULL, not 16-byte
 * aligned or too small. */
#define LF_CC_MATMUL_MAX_INNER 64
#define LF_CC_MATMUL_MAX_OPERANDS 256
int64_t lf_cc_matmul_ws_words(const lf_ks_plan *plan, int nu);
int lf_cc_matmul(const lf_ks_plan *plan, int m, int k, int n, int nu, const int64_t *const *in, const int64_t *const *row0,
                 const int64_t *ia, const int64_t *ib, const int64_t *ksk, int64_t part_stride, int64_t comp_stride, int64_t row_off,
                 int key_format, int64_t *ws, int64_t ws_words, int64_t *const *out0, int64_t *const *out1, void *stream);

/* Several weighted sums of the same ciphertexts under ONE rescale (the baby-step sums of a polynomial evaluation): for
 * g < G, out_g = rescale(sum_{t < k} s_{g,t} ct_t) (+ a constant), level l -> l + 1, one launch per group of 4, 2 or 1 outputs
 * (weighted_sums_kernel<4 | 2 | 1>: every input word is read once per group).
 * in / row0: HOST arrays of 2 k device pointers, [term][component]: the first surviving row ([rows][N]) resp. the dropped row
 * of ct_t.c0, ct_t.c1 at level l, lazy words in [0, 2q); the same polynomial may appear any number of times.  out: HOST array of
 * 2 G device pointers, [output][component], [rows][N] each, canonical.  rows = limbs of level l + 1; ql .. kh hold rows + 1
 * entries, those of level l: entry 0 is the dropped limb.  scales / round_at as lf_rescale_batch (rows entries).
 * tab: DEVICE table [G][k][rows + 1] of s_{g,t} R^2 mod q_row (R = 2^62: the kernel sums x_t * tab in 128 bits and reduces
 * twice); consts: NULL or DEVICE table [G][rows] of plain residues added to coefficient 0 of component 0 after the rescale.
 * The result has exactly the words of ckks_engine's
 *     acc = scale_rows(ct_0, s_{g,0});  acc = cc_add(acc, scale_rows(ct_t, s_{g,t})) for t >= 1;  rescale(acc);  add_scalar
 * (scale_rows = mont_enter_scalar + reduce_2q: mult_int_scalar) for every prime below 2^60.
 * LF_ERR_ARG before any device call for k < 1 or > LF_WSUM_MAX_TERMS, G < 1 or > LF_WSUM_MAX_OUTPUTS, rows < 0 or
 * rows + 1 > lf_limits(LF_LIMIT_ROWS), logN outside 13 .. 17, a NULL among in / row0 / out, their entries, tab, scales, ql .. kh. */
#define LF_WSUM_MAX_TERMS 16
#define LF_WSUM_MAX_OUTPUTS 64
int lf_weighted_sums(const int64_t *const *in, const int64_t *const *row0, int64_t *const *out, int k, int G, int rows, int logN,
                     const int64_t *tab, const int64_t *consts, const int64_t *scales, int64_t round_at, const int64_t *ql,
                     const int64_t *qh, const int64_t *kl, const int64_t *kh, int device, void *stream);

/* A sum of ciphertexts that stand at different levels, brought to ONE level L (a residual connection, the corrections of a
 * Chebyshev recurrence, level_up itself): for each of nsets sets, out_s = sum_{t < k_s} s_t u_t (+ a constant), where u_t is
 * ct_t itself if it stands at L and level_up(ct_t, L) if it stands above it (level l < L: one rescale, the rows of L kept, times
 * level_up's integer delta).  ONE launch for all sets and both components; every surviving input word is read once, every
 * output word written once.
 * k: HOST array of nsets term counts.  The per-term arrays are HOST arrays packed set after set, term after term (n = sum k_s
 * terms in all): in / row0 hold 2 n device pointers, [term][component]: the first row of ct_t.c0, ct_t.c1 that survives at L
 * ([rows][N]; L - l rows into a tensor at level l) and the dropped row (the tensor's first row), NULL for a term at L; scales
 * holds n device pointers: the term's rescale constants of the rows at L (the tail of lf_rescale_batch's table at level l), NULL
 * for a term at L; round_at holds n words, as lf_rescale_batch takes it (ignored for a term at L).  Input words are lazy words
 * in [0, 2q) or what a rescale leaves; the same polynomial may appear any number of times.
 * tab: HOST array of nsets device pointers, each a DEVICE table [k_s][rows] of s_t R^2 mod q_row (a term at L) or
 * s_t delta_t R^2 mod q_row (a levelled one), R = 2^62: the kernel sums word * tab in 128 bits and reduces twice.  consts: NULL,
 * or a HOST array of nsets device pointers, each NULL or a DEVICE table [rows] of plain residues added to coefficient 0 of
 * component 0.  out: HOST array of 2 nsets device pointers, [set][component], [rows][N] each, canonical.  rows = limbs of level
 * L; ql .. kh hold its rows entries.
 * The result has exactly the words of ckks_engine's
 *     u_t = ct_t or level_up(ct_t, L);  v_t = u_t or mult_int_scalar(u_t, s_t);  acc = v_0;  acc = cc_add(acc, v_t);  add_scalar
 * for every prime below 2^60 (a single term with s = 1 at L is a copy: the engine refuses it).
 * LF_ERR_ARG before any device call for nsets < 1 or > LF_LSUM_MAX_SETS, a k_s < 1 or > LF_LSUM_MAX_TERMS, rows < 0 or
 * > lf_limits(LF_LIMIT_ROWS), logN outside 13 .. 17, a NULL among k / in / row0 / scales / round_at / tab / out / ql .. kh, among
 * the entries of in, tab and out, and a term whose two dropped rows and scales are not all NULL or all given. */
#define LF_LSUM_MAX_TERMS 8
#define LF_LSUM_MAX_SETS 8
int lf_level_sum(int nsets, const int64_t *k, const int64_t *const *in, const int64_t *const *row0, const int64_t *const *scales,
                 const int64_t *round_at, const int64_t *const *tab, const int64_t *const *consts, int64_t *const *out, int rows,
                 int logN, const int64_t *ql, const int64_t *qh, const int64_t *kl, const int64_t *kh, int device, void *stream);

/* mod_raise: the base-prime residue of `count` ciphertexts lifted to every limb of level 0 — the first step of a bootstrap.  ONE
 * launch for both components of all of them.
 * in0 / in1: HOST arrays of count device pointers: the base-prime row (N words) of c0 / c1 of ciphertext i, at whatever level it
 * stands; a word w is a lazy word in [0, 2 q_b) or what a rescale leaves, -q_b < w < 2 q_b.  out0 / out1: HOST arrays of count
 * device pointers, [rows][N] each.  rows = limbs of level 0 on this device; mont_one[r] = R mod q_r (R = 2^62) and ql .. kh hold
 * its rows entries (DEVICE).  Every pointer of in / out 16-byte aligned.  Per coefficient, with r = w mod q_b in [0, q_b) and
 * v = r - q_b if r > (q_b - 1) / 2 else r, row i of the output holds v mod q_i in [0, q_i): exactly the words of int64
 * remainder(v, q_i).  The same polynomial may appear any number of times among the inputs; outputs must be distinct.
 * LF_ERR_ARG before any device call for count < 1 or > LF_MOD_RAISE_MAX_CTS, rows < 0 or > lf_limits(LF_LIMIT_ROWS), N < 2 or
 * odd, q_b < 3 or >= 2^62, a NULL among the arrays, their entries, mont_one, ql .. kh, and a misaligned entry of in / out. */
#define LF_MOD_RAISE_MAX_CTS 64
int lf_mod_raise(int count, const int64_t *const *in0, const int64_t *const *in1, int64_t *const *out0, int64_t *const *out1,
                 int rows, int64_t N, int64_t q_b, const int64_t *mont_one, const int64_t *ql, const int64_t *qh,
                 const int64_t *kl, const int64_t *kh, int device, void *stream);

/* Sum of plaintext-ciphertext products under ONE rescale, for plaintexts encoded once (ckks_engine.encode_plain): out decrypts to
 * sum_i pt_i * ct_i (+ bias), level l -> l + 1.  Plan-free: no key, no digits.
 * k >= 1 terms; in: HOST array of 2 k device pointers, [term][component]: ct_i.c0, ct_i.c1, each [rows][N] at level l (all its
 * rows, the dropped limb first), lazy words in [0, 2q), 16-byte aligned; pt: HOST array of k device pointers, [rows][N] each: the
 * plaintext mc_mult builds (NTT domain, Montgomery form, lazy words below 2q); the same polynomial may appear any number of times.
 * bias: NULL or the plaintext mc_add builds at level l + 1, [rows - 1][N].  out0 / out1 [rows - 1][N], canonical.
 * Tables of level l, `rows` entries each, the dropped limb first: psi_br / psi_dp, ipsi_br / ipsi_dp, q_host (HOST), Rs, Ninv,
 * ql .. kh, and mont_one[r] = R mod q_r (DEVICE); zero_row: N zero words (DEVICE).  rescale_scales / round_at as lf_rescale_batch
 * (rows - 1 entries).
 * The result has exactly the words of ckks_engine's
 *     S_c = mont_mult(pt_0, enter_ntt(ct_0.c));  S_c = mont_add(S_c, mont_mult(pt_i, enter_ntt(ct_i.c))) for i >= 1, c = 0, 1;
 *     intt_exit_reduce(S_c);  rescale((S_0, S_1));  then mc_add's chain with `bias` on component 0
 * (k = 1 without bias: mc_mult's words behind its encode).  Only the residues of S reach the result — intt_exit_reduce leaves
 * canonical words — so S is kept in the relaxed representation of the other fused ops: plain canonical residues on fp64-class
 * rows, Montgomery-form words below 2q on integer-class rows.
 * Enqueued: per chunk of 4, 2 or 1 terms ONE lf_rescale_ntt of its 2 g polynomials into the workspace (RELAXED | PLAIN, PLANES
 * where lf_stack_planes says so; the rescale step of that transform is handed the identity: zero_row as every dropped row,
 * mont_one as the scales — it is the forward transform that reads its operands where they lie) and ONE launch of
 * pc_dot_kernel<4 | 2 | 1> adding the chunk's products into S = [2][rows][N] (the first chunk writes); lf_intt (tail 2, relaxed,
 * plain) of S; ONE lf_rescale_batch of the pair; with a bias one element-wise launch (pc_bias_kernel) on out0.
 * (k = 1 takes the same launches: lf_intt_mul's product-on-load multiplies PLAIN residues on fp64-class rows, and the plaintext
 * is in Montgomery form there.)
 * ws: lf_pc_dot_ws_words(k, rows, logN) = (2 min(k, 4) + 2) rows N words (0 for shapes the entry refuses), 16-byte aligned, lent
 * by the caller.  LF_ERR_ARG before any device call for k < 1, rows < 2 or > lf_limits(LF_LIMIT_ROWS), logN outside 13 .. 17, a
 * NULL among the pointers (bias excepted), the 2 k entries of `in`, the k of `pt` or the tables, ws NULL, too small or misaligned. */
int64_t lf_pc_dot_ws_words(int k, int rows, int logN);
int lf_pc_dot(int k, const int64_t *const *in, const int64_t *const *pt, const int64_t *bias, int64_t *out0, int64_t *out1, int rows,
              int logN, const int64_t *psi_br, const double *psi_dp, const int64_t *ipsi_br, const double *ipsi_dp,
              const int64_t *q_host, const int64_t *Rs, const int64_t *Ninv, const int64_t *mont_one, const int64_t *zero_row,
              const int64_t *rescale_scales, int64_t round_at, int64_t *ws, int64_t ws_words, const int64_t *ql, const int64_t *qh,
              const int64_t *kl, const int64_t *kh, int device, void *stream);

/* A plaintext matrix times a vector of ciphertexts under ONE rescale per output (a layer over feature-per-ciphertext packing):
 * for o < k_out, out_o decrypts to sum_{i < k_in} pt_{o,i} * ct_i (+ bias_o), level l -> l + 1.  Plan-free, the tables of lf_pc_dot.
 * in: HOST array of 2 k_in device pointers, [input][component], as lf_pc_dot's; pt: HOST array of k_out k_in device pointers,
 * row-major ([output][input]), NULL for an absent term (a zero weight); bias: NULL, or a HOST array of k_out pointers, each NULL or
 * the plaintext mc_add builds at level l + 1; out0 / out1: HOST arrays of k_out pointers, [rows - 1][N] each, canonical.  The same
 * polynomial may appear any number of times among `in` and among `pt`.
 * Output o has exactly the words of lf_pc_dot over the terms (pt_{o,i}, ct_i) with a non-NULL plaintext, in the order of i, with
 * bias_o: only the residues of that entry's S reach its result, so the order and grouping of the additions are free.
 * Enqueued: per chunk of at most LF_PC_MATMUL_CI of the inputs some output uses (an input whose column of pt is all NULL is not
 * transformed) their forward transforms as lf_pc_dot runs them — lf_rescale_ntt with the identity rescale, RELAXED | PLAIN,
 * PLANES where lf_stack_planes says so, 4, 2 or 1 ciphertexts per call — into consecutive slots of the workspace: every input is
 * transformed ONCE per call of the entry, whatever k_out; per chunk and per group of 4, 2 or 1 outputs ONE launch of
 * pc_matmul_kernel<4 | 2 | 1> (the product body shared with lf_pc_matmul_batch and lf_pc_matmul_batch_planes, at one token and raw
 * plaintexts; grid N / 512 x rows; a thread reads the two transformed pairs of an input once for its group's outputs and each
 * plaintext pair once) adding the chunk's products into the group's pairs of S = [k_out][2][rows][N] (the first
 * chunk writes); ONE lf_intt (tail 2, relaxed, plain) of the 2 k_out polynomials of S; lf_rescale_batch per 4 outputs; one
 * pc_bias_kernel launch per output that has a bias.
 * ws: lf_pc_matmul_ws_words(k_in, k_out, rows, logN) = (2 min(k_in, LF_PC_MATMUL_CI) + 2 k_out) rows N words (0 for shapes the
 * entry refuses), 16-byte aligned, lent by the caller.  LF_ERR_ARG before any device call for k_in < 1, k_out < 1 or
 * > LF_PC_MATMUL_MAX_OUTPUTS, rows < 2 or > lf_limits(LF_LIMIT_ROWS), logN outside 13 .. 17, a NULL among the tables, in, out0,
 * out1 or their entries, an output whose k_in entries of pt are all NULL, ws NULL, too small or misaligned.  LF_ERR_STATE where
 * the library's note of a chunk's slots says another format than the one this call's products read (a knob flipped by another
 * thread between the two). */
#define LF_PC_MATMUL_CI 16            /* inputs per chunk: fp64-class rows sum CI balanced products + one word, < 64 q up to 125 */
#define LF_PC_MATMUL_MAX_OUTPUTS 64
int64_t lf_pc_matmul_ws_words(int k_in, int k_out, int rows, int logN);
int lf_pc_matmul(int k_in, int k_out, const int64_t *const *in, const int64_t *const *pt, const int64_t *const *bias,
                 int64_t *const *out0, int64_t *const *out1, int rows, int logN, const int64_t *psi_br, const double *psi_dp,
                 const int64_t *ipsi_br, const double *ipsi_dp, const int64_t *q_host, const int64_t *Rs, const int64_t *Ninv,
                 const int64_t *mont_one, const int64_t *zero_row, const int64_t *rescale_scales, int64_t round_at, int64_t *ws,
                 int64_t ws_words, const int64_t *ql, const int64_t *qh, const int64_t *kl, const int64_t *kh, int device, void *stream);

/* lf_pc_matmul over nt token vectors that share the matrix (a dense layer over the tokens of a sequence or the samples of a
 * batch): for t < nt, o < k_out, out_{t,o} decrypts to sum_i pt_{o,i} * ct_{t,i} (+ bias_o).  nt: 1 .. LF_PC_MATMUL_BATCH_MAX_TOKENS;
 * in: HOST array of nt 2 k_in device pointers, [token][input][component]; out0 / out1: HOST arrays of nt k_out pointers,
 * [token][output]; pt, bias and the tables: lf_pc_matmul's, shared by all tokens.  The same polynomial may appear any number of
 * times among `in` (in one token or several) and among `pt`.
 * Output (t, o) has exactly the words of lf_pc_matmul on token t: only the residues of that entry's S reach its result, so the
 * order and grouping of the additions — and which other tokens share a launch — are free.
 * Enqueued, for the inputs some output uses, in chunks of at most LF_PC_MATMUL_CI: per token the chunk's forward transforms as
 * lf_pc_matmul runs them, into x = [nt][n][2][rows][N] (a token's slots 2 min(k_in, LF_PC_MATMUL_CI) polynomials apart): every
 * (token, input) is transformed once per call; per chunk and per group of 4, 2 or 1 outputs ONE launch of pc_matmulb_kernel<GO, 2>
 * per tile of 2 tokens (the same body with two accumulator sets: a thread reads the two transformed pairs of each of its tokens
 * once and each plaintext pair ONCE for both) and lf_pc_matmul's pc_matmul_kernel<GO> for an odd token left (3 tokens: 2 + 1; 4: 2 + 2 — one launch of <GO, 4> measured
 * slower, LF_TUNE_PC_MATMUL_TILE), into S = [nt][k_out][2][rows][N] (the first chunk writes); lf_intt (tail
 * 2, relaxed, plain) of the 2 k_out nt polynomials of S in ONE call up to 128 polynomials (the largest batch lf_pc_matmul hands
 * it), per token beyond; lf_rescale_batch per 4 outputs and pc_bias_kernel per output with a bias, per token.  nt = 1 enqueues
 * exactly what lf_pc_matmul does.
 * ws: lf_pc_matmul_batch_ws_words(nt, k_in, k_out, rows, logN) = nt lf_pc_matmul_ws_words(k_in, k_out, rows, logN) words (0 for
 * shapes the entry refuses), 16-byte aligned.  LF_ERR_ARG before any device call for nt < 1 or > the maximum, everything
 * lf_pc_matmul refuses, a NULL among the nt 2 k_in inputs or the nt k_out outputs of either array.  LF_ERR_STATE as lf_pc_matmul. */
#define LF_PC_MATMUL_BATCH_MAX_TOKENS 4
int64_t lf_pc_matmul_batch_ws_words(int nt, int k_in, int k_out, int rows, int logN);
int lf_pc_matmul_batch(int nt, int k_in, int k_out, const int64_t *const *in, const int64_t *const *pt, const int64_t *const *bias,
                       int64_t *const *out0, int64_t *const *out1, int rows, int logN, const int64_t *psi_br, const double *psi_dp,
                       const int64_t *ipsi_br, const double *ipsi_dp, const int64_t *q_host, const int64_t *Rs, const int64_t *Ninv,
                       const int64_t *mont_one, const int64_t *zero_row, const int64_t *rescale_scales, int64_t round_at, int64_t *ws,
                       int64_t ws_words, const int64_t *ql, const int64_t *qh, const int64_t *kl, const int64_t *kh, int device,
                       void *stream);

/* "Plain planes": the compact form of a "mult" plaintext (the [rows][N] tensor mc_mult builds: NTT domain, Montgomery form, lazy words
 * below 2q) — the operand in which a layer's memory and the product launches' stream go.  Rows lie back to back in row order:
 *   fp64-class row (prime below 2^lf_limits(LF_LIMIT_SMALL_PRIME_BITS))   6 N bytes: u32 lo[N], then u16 hi[N], the low 32 bits and
 *       bits 32 .. 47 of v = REDC62(w) — the plain residue in [0, q] pc_matmul_kernel forms from the Montgomery word w on every read;
 *   integer-class row                                                     8 N bytes: the word as it is.
 * 6 N and 8 N are multiples of 16, so every row starts 16-byte aligned; the row offsets follow from the primes alone.
 * lf_plain_planes_words(rows, N, q_host): the size in 8-byte words, rows N - N / 4 per fp64-class row; 0 for what the format refuses:
 * rows < 1 or > LF_PLAIN_PLANES_MAX_ROWS (the kernels take the classes as a 64-bit mask), N no power of two in 2^13 .. 2^17, q_host NULL.
 * lf_plain_planes: src [rows][N] -> dst (lf_plain_planes_words words), ONE launch.  lf_plain_unplanes: the inverse, ONE launch, writes
 * the CANONICAL Montgomery residue w mod q on every row (v R mod q on fp64-class rows, the stored word reduced once on the others).
 * q_host: HOST primes of the rows; ql .. kh: their device constants.  LF_ERR_ARG before any device call for a size the format refuses,
 * a NULL pointer, src == dst, src or dst not 16-byte aligned. */
#define LF_PLAIN_PLANES_MAX_ROWS 64
int64_t lf_plain_planes_words(int rows, int64_t N, const int64_t *q_host);
int lf_plain_planes(const int64_t *src, int64_t *dst, int rows, int64_t N, const int64_t *q_host, const int64_t *ql, const int64_t *qh,
                    const int64_t *kl, const int64_t *kh, int device, void *stream);
int lf_plain_unplanes(const int64_t *src, int64_t *dst, int rows, int64_t N, const int64_t *q_host, const int64_t *ql, const int64_t *qh,
                      const int64_t *kl, const int64_t *kh, int device, void *stream);

/* lf_pc_matmul_batch with every non-NULL entry of pt a compact plaintext (lf_plain_planes of the rows of q_host): signature, semantics,
 * chunking, output groups, token tiles, transforms, rescales and biases are lf_pc_matmul_batch's (nt = 1: lf_pc_matmul; nt = 1,
 * k_out = 1: lf_pc_dot's sum), and so are the words of every output — those of lf_pc_matmul_batch on the plaintexts the planes were
 * packed from: the stored fp64-class word is the one the raw kernels compute on load.  The product launches are
 * pc_planes_matmul_kernel<GO, GT> (the body of the raw kernels with the plaintext side chosen at compile time; GT = 1, 2: the tiles
 * of lf_pc_matmul_batch; 4 under LF_TUNE_PC_MATMUL_TILE): per plaintext and pair of
 * coefficients an 8-byte and a 4-byte nontemporal load on fp64-class rows and no REDC, the 16-byte pair at the row's compact offset
 * on integer-class rows; the offset is derived in the kernel from a bit mask of the fp64-class rows (a kernel argument built from
 * q_host: no table, no copy).  ws: lf_pc_matmul_batch_planes_ws_words = lf_pc_matmul_batch_ws_words, 0 also for rows >
 * LF_PLAIN_PLANES_MAX_ROWS.  LF_ERR_ARG / LF_ERR_STATE as lf_pc_matmul_batch. */
int64_t lf_pc_matmul_batch_planes_ws_words(int nt, int k_in, int k_out, int rows, int logN);
int lf_pc_matmul_batch_planes(int nt, int k_in, int k_out, const int64_t *const *in, const int64_t *const *pt, const int64_t *const *bias,
                              int64_t *const *out0, int64_t *const *out1, int rows, int logN, const int64_t *psi_br, const double *psi_dp,
                              const int64_t *ipsi_br, const double *ipsi_dp, const int64_t *q_host, const int64_t *Rs, const int64_t *Ninv,
                              const int64_t *mont_one, const int64_t *zero_row, const int64_t *rescale_scales, int64_t round_at, int64_t *ws,
                              int64_t ws_words, const int64_t *ql, const int64_t *qh, const int64_t *kl, const int64_t *kh, int device,
                              void *stream);

/* The halves of an op around the digit exchange of a limb-sharded engine (one process per GPU; the reference gathers every
 * digit on every GPU through the host before it extends any, ckks_engine.py:778-829).  The plan describes THIS rank's rows
 * at the level (dig_nparts = the digits it owns, nparts = all digits, state = its own digit rows):
 *   lf_cc_mult_evk_pre / lf_switch_key_pre   everything up to the digits this rank owns, into plan->state;
 *   lf_ks_plan_fwd                           extension + forward NTT of digits first .. first + count - 1 of the gathered
 *                                            storage-order buffer `digits` (own digits while the others travel, foreign runs
 *                                            after the wait); relin != 0: inside cc_mult (own-limb pairs skipped);
 *   lf_cc_mult_evk_post / lf_switch_key_post inner product over ALL digits + inverse NTT + mod-down (+ c0(X^p)).
 * pre, fwd over every digit, post == lf_cc_mult_evk / lf_switch_key.
 * `which` (bit mask, 3 = the whole half) separates the launches whose ADDRESSES change from call to call from those that only
 * touch the plan's scratch, tables and the key — the second kind can be captured once into a HIP graph and replayed (the
 * engine does: a rank of a sharded gold cc_mult enqueues in ~55 us of host time instead of 140, profiles/r05_host_overhead.txt):
 *   lf_cc_mult_evk_pre   1 = the launch that reads in / row0 (rescale + column pass), 2 = the rest (tiled pass, x1 * y1,
 *                        inverse NTT, digits);  lf_switch_key_pre is one launch, it reads c1;
 *   lf_*_post            1 = inner product + inverse NTT, 2 = the mod-down (reads c0, writes out0 / out1). */
int lf_cc_mult_evk_pre(const lf_ks_plan *plan, const int64_t *const *in, const int64_t *const *row0, int which, void *stream);
int lf_switch_key_pre(const lf_ks_plan *plan, const int64_t *c1, int64_t gal_pinv, int gal_canonical, void *stream);
int lf_ks_plan_fwd(const lf_ks_plan *plan, const int64_t *digits, int first, int count, int relin, void *stream);
int lf_cc_mult_evk_post(const lf_ks_plan *plan, const int64_t *ksk, int64_t part_stride, int64_t comp_stride, int64_t row_off,
                        int key_format, int64_t *out0, int64_t *out1, int which, void *stream);
int lf_switch_key_post(const lf_ks_plan *plan, const int64_t *c0, int64_t gal_pinv, int gal_canonical, const int64_t *ksk,
                       int64_t part_stride, int64_t comp_stride, int64_t row_off, int key_format, int64_t *out0, int64_t *out1,
                       int which, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Samplers: the reference's csprng extensions, src/liberate/csprng/.
 * A ChaCha20 state is 16 int64 words holding 32-bit values (csprng.py:124-160); words 12/13 are
 * the 64-bit block counter, advanced by `step` after every draw.  All tables below are DEVICE
 * pointers except q_host / btree_host, which the reference also takes as host pointers.
 * Row counts need not be multiples of the block size (the reference silently drops the tail).
 * ---------------------------------------------------------------------------------------------- */

/* chacha20_cuda.chacha20 (chacha20.cpp:17-40, chacha20_cuda_kernel.cu:10-46): dest[i] = block(states[i])
 * for n states [n][16]; states' counters advance. */
int lf_chacha20(int64_t *states, int64_t *dest, int64_t n, uint64_t step, int device, void *stream);

/* randint_cuda.randint_fast (randint.cpp:38-52, randint_cuda_kernel.cu:22-101): fused ChaCha20 +
 * floor(q_c * X / 2^128) + shift, four samples per state; states [channels][L][16] -> dst [channels][4L]. */
int lf_randint_fast(int64_t *states, int64_t *dst, int channels, int64_t L, const uint64_t *q_host, int64_t shift,
                    uint64_t step, int device, void *stream);

/* randint_cuda.randint (randint.cpp:21-33, randint_cuda_kernel.cu:108-152): the same map in place on
 * random words rand_bytes [channels][n][16]; word 4j of each row receives the sample of words 4j..4j+3. */
int lf_randint(int64_t *rand_bytes, int channels, int64_t n, const uint64_t *q_host, int device, void *stream);

/* discrete_gaussian_cuda.discrete_gaussian_fast (discrete_gaussian_cuda_kernel.cu:28-109, 186-215): fused
 * ChaCha20 + CDT binary-tree walk, four samples per state; states [n][16] -> dst [4n].
 * btree_host: btree_size low words in level order, then btree_size high words
 * (discrete_gaussian_sampler.py:96-118); 2*btree_size <= 128. */
int lf_discrete_gaussian_fast(int64_t *states, int64_t *dst, int64_t n, const uint64_t *btree_host, int btree_size,
                              int depth, uint64_t step, int device, void *stream);

/* discrete_gaussian_cuda.discrete_gaussian (discrete_gaussian_cuda_kernel.cu:118-168, 222-240): in place on
 * rand_bytes [n][16]. */
int lf_discrete_gaussian(int64_t *rand_bytes, int64_t n, const uint64_t *btree_host, int btree_size, int depth,
                         int device, void *stream);

/* randround_cuda.randround (randround_cuda_kernel.cu:8-56): rand_bytes[i] = sign(c) * (floor|c| +
 * [rand_bytes[i] < rn(frac|c| * 2^32)]), c = coef[i]; rand_bytes holds 32-bit random words. */
int lf_randround(const double *coef, int64_t *rand_bytes, int64_t n, int device, void *stream);

/* ------------------------------------------------------------------------------------------------
 * The reference's 30-bit / int32 word mode of the same 15 functions (ckks_context.py:213-216 buffer_bit_length = 30:
 * R = 2^30, 15-bit halves ql / qh / kl / kh, 28-bit message primes; K.cu:141, 223, 339 dispatch the kernel templates for
 * int32 as well).  No preset, test or example of the reference selects it; it is served for the completeness of the
 * boundary (csrc/ckks_w30.hip: one plain launch per step of the reference's own chain, its exact lazy words), the fused
 * engine entries above are 62-bit only.  Arguments as their lf_* counterparts, words and per-row vectors int32;
 * psi_br / ipsi_br = the compact [rows][N] tables in Montgomery form (R = 2^30).
 *   mont_mult, mont_enter, mont_redc (ntt.cpp:120-163, 248-263); reduce_2q, make_signed, make_unsigned, tile_unsigned,
 *   mont_add, mont_sub (347-419); lf30_ntt: Rs = NULL ntt, Rs != NULL enter_ntt (166-216); lf30_intt: tail 0 intt, 1 intt_exit,
 *   2 intt_exit_reduce, 3 intt_exit_reduce_signed (219-345).
 * ---------------------------------------------------------------------------------------------- */
int lf30_mont_mult(const int32_t *a, const int32_t *b, int32_t *c, int rows, int64_t N, const int32_t *ql, const int32_t *qh,
                   const int32_t *kl, const int32_t *kh, int device, void *stream);
int lf30_mont_enter(int32_t *a, const int32_t *Rs, int rows, int64_t N, const int32_t *ql, const int32_t *qh, const int32_t *kl,
                    const int32_t *kh, int device, void *stream);
int lf30_mont_redc(int32_t *a, int rows, int64_t N, const int32_t *ql, const int32_t *qh, const int32_t *kl, const int32_t *kh,
                   int device, void *stream);
int lf30_reduce_2q(int32_t *a, int rows, int64_t N, const int32_t *_2q, int device, void *stream);
int lf30_make_signed(int32_t *a, int rows, int64_t N, const int32_t *_2q, int device, void *stream);
int lf30_make_unsigned(int32_t *a, int rows, int64_t N, const int32_t *_2q, int device, void *stream);
int lf30_tile_unsigned(const int32_t *a, int32_t *dst, int rows, int64_t N, const int32_t *_2q, int device, void *stream);
int lf30_mont_add(const int32_t *a, const int32_t *b, int32_t *c, int rows, int64_t N, const int32_t *_2q, int device, void *stream);
int lf30_mont_sub(const int32_t *a, const int32_t *b, int32_t *c, int rows, int64_t N, const int32_t *_2q, int device, void *stream);
int lf30_ntt(int32_t *a, int batch, int rows, int logN, const int32_t *psi_br, const int32_t *Rs, const int32_t *_2q,
             const int32_t *ql, const int32_t *qh, const int32_t *kl, const int32_t *kh, int device, void *stream);
int lf30_intt(int32_t *a, int batch, int rows, int logN, const int32_t *ipsi_br, const int32_t *Ninv, int tail, const int32_t *_2q,
              const int32_t *ql, const int32_t *qh, const int32_t *kl, const int32_t *kh, int device, void *stream);

#ifdef __cplusplus
}
#endif
#endif
