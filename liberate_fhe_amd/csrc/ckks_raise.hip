// ckks_raise.hip — mod_raise: a ciphertext's base-prime residue lifted to every limb of level 0 (the first step of a CKKS
// bootstrap; the reference has no such entry).
//
// The residue mod q_b of a ciphertext (c0, c1) of ANY level is a ciphertext mod q_b of the same plaintext polynomial.  Its
// centred lift v in [-(q_b - 1) / 2, (q_b - 1) / 2], reduced mod every prime of level 0, is a ciphertext of t + q_b I there:
// t the plaintext mod q_b, I the small integer overflow of c0 + c1 s over Z (bounded by the weight of the secret).
#include "../../include/ckks_hip.h"
#include "ckks_common.h"

namespace {

// Per coefficient, on the stored word w of the base row — a lazy word in [0, 2 q_b), or what a rescale leaves: REDC of a negative
// product gives a word in (-q_b / 2, 0) about once in 2^22 words (ckks_fused.hip, level_sum_kernel) — taken as -q_b < w < 2 q_b:
//     r = w mod q_b in [0, q_b): one addition on the sign, one conditional subtraction;
//     v = r - q_b if r > (q_b - 1) / 2, else r:  |v| <= (q_b - 1) / 2 < 2^61;
//     row i: x = REDC(v * (R mod q_i)) = (v one_i + s q_i) / R, = v (mod q_i):  |v one_i| / R < q_i / 2 and 0 <= s q_i / R < q_i,
//            so -q_i / 2 < x < 3 q_i / 2: one addition on the sign and one conditional subtraction leave v mod q_i in [0, q_i).
// The same REDC on both prime classes: |v| is beyond the 2^52 of the fp64 products, and the kernel is bound by its stores (16
// bytes read per 16 * rows written), not by the four REDCs per row of a thread.
// A thread owns a PAIR of coefficients of one ciphertext: it loads the base words of both components once (two 16-byte loads)
// and walks MRAISE_ROWS rows of both outputs with 16-byte stores, coalesced along N.  blockIdx.y = the row chunk (a chunk
// re-reads the 32 bytes: L2), blockIdx.z = the ciphertext.
#define MRAISE_ROWS 4
struct RaiseBatch {
    const i64 *in[2 * LF_MOD_RAISE_MAX_CTS];   // [ct][component]: the base row, N words
    i64 *out[2 * LF_MOD_RAISE_MAX_CTS];        // [ct][component]: [rows][N]
};

static __device__ __forceinline__ i64 raise_centre(i64 w, i64 qb, i64 half) {
    w += (w >> 63) & qb;
    w = w < qb ? w : w - qb;
    return w > half ? w - qb : w;
}

static __device__ __forceinline__ i64 raise_word(i64 v, i64 one, const RowMod m) {
    i64 x = mm62s(v, one, m.q, m.k);
    x += (x >> 63) & (i64)m.q;
    return x < (i64)m.q ? x : x - (i64)m.q;
}

__global__ void __launch_bounds__(256) mod_raise_kernel(RaiseBatch pb, int rows, i64 N, i64 qb, const i64 *__restrict__ mont_one,
                                                        const i64 *__restrict__ ql, const i64 *__restrict__ qh,
                                                        const i64 *__restrict__ kl, const i64 *__restrict__ kh) {
    const int ct = blockIdx.z;
    const i64 j = ((i64)blockIdx.x * 256 + threadIdx.x) * 2;
    if (j >= N) return;
    const i64 half = (qb - 1) >> 1;
    longlong2 a = *reinterpret_cast<const longlong2 *>(pb.in[2 * ct] + j);
    longlong2 b = *reinterpret_cast<const longlong2 *>(pb.in[2 * ct + 1] + j);
    a.x = raise_centre(a.x, qb, half), a.y = raise_centre(a.y, qb, half);
    b.x = raise_centre(b.x, qb, half), b.y = raise_centre(b.y, qb, half);
    i64 *__restrict__ o0 = pb.out[2 * ct];
    i64 *__restrict__ o1 = pb.out[2 * ct + 1];
    const int r0 = blockIdx.y * MRAISE_ROWS;
    const int r1 = r0 + MRAISE_ROWS < rows ? r0 + MRAISE_ROWS : rows;
    for (int r = r0; r < r1; ++r) {
        const RowMod m = load_mod(ql, qh, kl, kh, r);
        const i64 one = mont_one[r];
        const i64 off = (i64)r * N + j;
        longlong2 x, y;
        x.x = raise_word(a.x, one, m), x.y = raise_word(a.y, one, m);
        y.x = raise_word(b.x, one, m), y.y = raise_word(b.y, one, m);
        *reinterpret_cast<longlong2 *>(o0 + off) = x;
        *reinterpret_cast<longlong2 *>(o1 + off) = y;
    }
}

}  // namespace

extern "C" {

int lf_mod_raise(int count, const int64_t *const *in0, const int64_t *const *in1, int64_t *const *out0, int64_t *const *out1,
                 int rows, int64_t N, int64_t q_b, const int64_t *mont_one, const int64_t *ql, const int64_t *qh,
                 const int64_t *kl, const int64_t *kh, int device, void *stream) {
    if (count < 1 || count > LF_MOD_RAISE_MAX_CTS || rows < 0 || rows > MAX_LIST_ROWS) return LF_ERR_ARG;
    if (N < 2 || (N & 1) || q_b < 3 || q_b >= ((int64_t)1 << 62)) return LF_ERR_ARG;
    if (!in0 || !in1 || !out0 || !out1 || !mont_one || !ql || !qh || !kl || !kh) return LF_ERR_ARG;
    RaiseBatch pb;
    for (int i = 0; i < count; ++i) {
        if (!in0[i] || !in1[i] || !out0[i] || !out1[i]) return LF_ERR_ARG;
        if (((uintptr_t)in0[i] | (uintptr_t)in1[i] | (uintptr_t)out0[i] | (uintptr_t)out1[i]) & 15) return LF_ERR_ARG;
        pb.in[2 * i] = (const i64 *)in0[i], pb.in[2 * i + 1] = (const i64 *)in1[i];
        pb.out[2 * i] = (i64 *)out0[i], pb.out[2 * i + 1] = (i64 *)out1[i];
    }
    for (int i = 2 * count; i < 2 * LF_MOD_RAISE_MAX_CTS; ++i) pb.in[i] = nullptr, pb.out[i] = nullptr;
    if (rows == 0) return 0;
    if (int e = lf_set_device(device)) return e;
    dim3 grid((unsigned)((N / 2 + 255) / 256), (unsigned)((rows + MRAISE_ROWS - 1) / MRAISE_ROWS), (unsigned)count);
    hipLaunchKernelGGL(mod_raise_kernel, grid, dim3(256), 0, (hipStream_t)stream, pb, rows, (i64)N, (i64)q_b, (const i64 *)mont_one,
                       (const i64 *)ql, (const i64 *)qh, (const i64 *)kl, (const i64 *)kh);
    return (int)hipGetLastError();
}

}  // extern "C"
