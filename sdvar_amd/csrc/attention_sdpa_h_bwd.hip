// Backward of the operator-seam attention under torch.autocast (attention_sdpa_h.hip, sdvar_op_sdpa_hm_lse): given out = softmax(scale q k^T + bias) v in fp16 / bf16,
// its log-sum-exp rows and dout,
//     P = exp(scale q k^T + bias - lse),  D_i = sum_d dO_id O_id,  dV = P^T dO,  dP = dO V^T,  dS = P o (dP - D),  dQ = scale dS K,  dK = scale dS^T Q
// on the half-precision matrix cores (v_mfma_f32_32x32x16_f16 / _bf16).  It is attention_sdpa_bwd.hip's structure (three launches, no score-sized matrix in memory, the
// forward's skip map, no atomics: every output element is reduced in one lane in a fixed order, so repeats are bit-identical) with attention_sdpa_h.hip's operand
// handling (strided operands, fp32 q / k rounded as they are read, bias kinds 0 - 3, XOR-swizzled 128-byte LDS rows, ds_read_b64_tr_b16 for transposed fragments).
//
// Arithmetic contract (what tests/test_gpu_seam_amp_grad.py holds the kernels to):
//   * dtype (1 fp16, 2 bf16) is the type of v, out, dout and dv.  q and k may each be fp32 (q_f32 / k_f32) and are then rounded to dtype (nearest even) as they are
//     read: the bits the forward multiplied.
//   * P = exp(scale q k^T + bias - lse) is recomputed in fp32 from the half-precision matrix-core scores with the forward's score expression in base 2,
//     exp2(fma(s, scale log2 e, bias log2 e) - lse log2 e), so that it agrees with the forward's weights.
//   * D_i = sum_d dout_id out_id accumulates in fp32 from the stored half values.
//   * dV = P^T dout with P rounded to dtype (nearest even), fp32 accumulation.   dP = dout v^T on the half matrix cores, fp32 accumulation.
//   * dS = P o (dP - D) in fp32, rounded ONCE to dtype (nearest even).   dQ = scale (dS K), dK = scale (dS^T Q) with fp32 accumulation; `scale` multiplies the fp32
//     accumulator, never a half value.
//   * every gradient is stored once: dv in dtype; dq in q's type and dk in k's type - fp32 (unrounded) when that operand was fp32, else rounded once to dtype.
//   * no clamping anywhere: a value beyond fp16's range becomes +-inf exactly as a cast would (a GradScaler relies on seeing inf to skip the step).
//   * a -inf bias entry inside a visited tile gives P = dS = 0 (dS is forced to 0 where P is 0, whatever dP is).  Skipped tiles have P = 0 exactly, so the skip map
//     changes no bit.  A query row with every key masked (lse = -inf) has no defined gradient; it contributes P = 0 to dK / dV, does not fault and does not disturb
//     other rows.
//
// Three kernels:
//   sdpa_h_bwd_delta_kernel  D (B, H, Lq) from out and dout: 8 lanes per row, 16 bytes of each per lane.
//   sdpa_h_bwd_dkdv_kernel   one workgroup per (128-key block, head, batch), one wave per 32 keys, the key on the lane: its K and V rows are resident as MFMA B operands
//                            (8 halves per 16-channel k-step).  Q / dO tiles of 64 queries stream through LDS, double-buffered with their lse and D, each tile stored
//                            TWICE: once with the row swizzle (chunk ^= (row >> 1) & 7) for the ds_read_b128 A operands of S = Q K^T and dP = dO V^T, once with the
//                            transpose swizzle (chunk ^= 4 ((row >> 1) & 1)) for the ds_read_b64_tr_b16 A operands of dV^T += dO^T P and dK^T += Q^T dS.  S and dP land
//                            as [query = register][key = lane], so the rounded P / dS registers ARE the B operands of the second products (the forward's trick with the
//                            roles of queries and keys exchanged).  A 128-key block is two skip-map columns: the workgroup walks the 128-query blocks either column
//                            needs and a wave computes only where its own column's byte is 0.
//   sdpa_h_bwd_dq_kernel     one workgroup per (128-query block, head, batch), one wave per 32 queries, the query on the lane (Q and dO fragments resident), the forward's
//                            walk over the unmasked 64-key tiles: K (row swizzle), V (row swizzle) and K again (transpose swizzle) double-buffered in LDS;
//                            S^T = K Q^T and dP^T = V dO^T as [key = register][query = lane], dQ^T += K^T dS^T.
// Tails: K / V rows past Lk are zero-filled in staging and their scores set to -inf (P = 0); Q / dO rows past Lq are zero-filled and their P forced to 0; lanes past
// the last row compute on a clamped row and never store.
#include "common.h"

namespace sdvar {

namespace {

constexpr int KT = 64;              // rows per LDS tile (keys in the dQ kernel, queries in the dK/dV kernel)
constexpr int QB = 128;             // queries per skip-map row / per dQ workgroup
constexpr int KB = 128;             // keys per dK/dV workgroup (two skip-map columns)
constexpr int TILE = KT * 8;        // 16-byte chunks per tile (64 rows x 128 bytes)
constexpr float L2E = 1.4426950408889634f;

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2p __attribute__((ext_vector_type(2)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

enum { HB_NONE = 0, HB_F32 = 1, HB_U8 = 2, HB_HALF = 3 };

struct SdpaHBwdArgs {
    const void *q, *k; const uint16_t *v, *out, *dout;
    const float* lse; float* delta;
    void *dq, *dk; uint16_t* dv;
    long long qs[3], ks[3], vs[3], os[3], gs[3], dqs[3], dks[3], dvs[3];          // element strides: batch, head, token (gs: dout)
    const void* bias; long long bs[3];          // element strides: batch, head, query row (0 = broadcast)
    int bias_vec;                               // bias rows allow 4-element vector loads along the keys
    const uint8_t* skip; int nkt;               // skip map (ceil(Lq/128), nkt) or nullptr
    int q_f32, k_f32;
    int B, H, Lq, Lk;
    float scale, scale_l2e;
};

// register r of an MFMA result block is row (r & 3) + 8 (r >> 2) + 4 * (lane >> 5)
__device__ __forceinline__ int mrow(int r, int lh) { return (r & 3) + 8 * (r >> 2) + 4 * lh; }

// two fp32 -> one packed word of two halves, round to nearest even (overflow -> inf)
template <bool BF16>
__device__ __forceinline__ uint32_t pack2(float a, float b) {
    const f32x2p v = {a, b};
    if (BF16) return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2p));         // v_cvt_pk_bf16_f32
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, f16x2p));                     // v_cvt_pk_f16_f32
}

// eight fp32 -> eight halves (one 16-byte chunk), round to nearest even
template <bool BF16>
__device__ __forceinline__ u32x4 pack8(u32x4 lo, u32x4 hi) {
    const f32x4 a = __builtin_bit_cast(f32x4, lo), b = __builtin_bit_cast(f32x4, hi);
    const u32x4 r = {pack2<BF16>(a[0], a[1]), pack2<BF16>(a[2], a[3]), pack2<BF16>(b[0], b[1]), pack2<BF16>(b[2], b[3])};
    return r;
}

template <bool BF16>
__device__ __forceinline__ float half_bits_to_float(uint32_t h) {
    if (BF16) return __uint_as_float(h << 16);
    return (float)__builtin_bit_cast(_Float16, (uint16_t)h);
}

template <bool BF16>
__device__ __forceinline__ f32x16 mfma_h(u32x4 a, u32x4 b, f32x16 c) {
    if (BF16) return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

// The transposed A fragment of one 32-channel block of a tile stored with the transpose swizzle: rows `row` + {0..3} and `row` + 8 + {0..3} of this lane's 16-lane
// group (attention_sdpa_h_kernel's V^T fragment).  Needs EXEC all ones.
__device__ __forceinline__ u32x4 read_tr(const uint16_t* t16, int row, int ch, int p4) {
    typedef __attribute__((address_space(3))) s16x4* lds_s16x4;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)(t16 + row * 64 + ch * 8 + 4 * (p4 & 1)));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)(t16 + (row + 8) * 64 + ch * 8 + 4 * (p4 & 1)));
    const u32x2 l2 = __builtin_bit_cast(u32x2, lo), h2 = __builtin_bit_cast(u32x2, hi);
    const u32x4 r = {l2[0], l2[1], h2[0], h2[1]};
    return r;
}

// the 64 channels of one token row as four B-operand fragments: k-step c, lane half lh holds channels 16 c + 8 lh + 0..7; an fp32 row is rounded as it is read
template <bool BF16>
__device__ __forceinline__ void load_row_frags(const void* base, long long off, int is_f32, int lh, u32x4 (&f)[4]) {
    if (is_f32) {
        const float* p = reinterpret_cast<const float*>(base) + off + 8 * lh;
#pragma unroll
        for (int c = 0; c < 4; ++c) f[c] = pack8<BF16>(*reinterpret_cast<const u32x4*>(p + 16 * c), *reinterpret_cast<const u32x4*>(p + 16 * c + 4));
    } else {
        const uint16_t* p = reinterpret_cast<const uint16_t*>(base) + off + 8 * lh;
#pragma unroll
        for (int c = 0; c < 4; ++c) f[c] = *reinterpret_cast<const u32x4*>(p + 16 * c);
    }
}

// one gradient row of this lane: accumulators x0 / x1 hold channels db * 32 + 8 g + 4 lh + e in register 4 g + e; `po` points at the row
template <bool BF16>
__device__ __forceinline__ void store_row(void* po, int is_f32, int lh, const f32x16& x0, const f32x16& x1, float mul) {
    if (is_f32) {
        float* p = reinterpret_cast<float*>(po) + 4 * lh;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            f32x4 v0, v1;
#pragma unroll
            for (int e = 0; e < 4; ++e) { v0[e] = x0[4 * g + e] * mul; v1[e] = x1[4 * g + e] * mul; }
            *reinterpret_cast<f32x4*>(p + 8 * g) = v0;
            *reinterpret_cast<f32x4*>(p + 32 + 8 * g) = v1;
        }
    } else {
        uint16_t* p = reinterpret_cast<uint16_t*>(po) + 4 * lh;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            u32x2 w0, w1;
            w0[0] = pack2<BF16>(x0[4 * g] * mul, x0[4 * g + 1] * mul); w0[1] = pack2<BF16>(x0[4 * g + 2] * mul, x0[4 * g + 3] * mul);
            w1[0] = pack2<BF16>(x1[4 * g] * mul, x1[4 * g + 1] * mul); w1[1] = pack2<BF16>(x1[4 * g + 2] * mul, x1[4 * g + 3] * mul);
            *reinterpret_cast<u32x2*>(p + 8 * g) = w0;
            *reinterpret_cast<u32x2*>(p + 32 + 8 * g) = w1;
        }
    }
}

// D[b][h][i] = sum_d dout[b][h][i][d] * out[b][h][i][d]: 8 lanes per row (16 bytes of each operand per lane), 32 rows per workgroup
template <bool BF16>
__global__ __launch_bounds__(256) void sdpa_h_bwd_delta_kernel(SdpaHBwdArgs a) {
    const long long rows = (long long)a.B * a.H * a.Lq;
    const long long row = (long long)blockIdx.x * 32 + (threadIdx.x >> 3);
    const long long rc = row < rows ? row : rows - 1;
    const int i = (int)(rc % a.Lq);
    const long long bh = rc / a.Lq;
    const int h = (int)(bh % a.H), b = (int)(bh / a.H);
    const int col = (threadIdx.x & 7) * 8;
    const u32x4 o = *reinterpret_cast<const u32x4*>(a.out + (long long)b * a.os[0] + (long long)h * a.os[1] + (long long)i * a.os[2] + col);
    const u32x4 g = *reinterpret_cast<const u32x4*>(a.dout + (long long)b * a.gs[0] + (long long)h * a.gs[1] + (long long)i * a.gs[2] + col);
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        s += half_bits_to_float<BF16>(o[w] & 0xFFFFu) * half_bits_to_float<BF16>(g[w] & 0xFFFFu);
        s += half_bits_to_float<BF16>(o[w] >> 16) * half_bits_to_float<BF16>(g[w] >> 16);
    }
#pragma unroll
    for (int m = 4; m > 0; m >>= 1) s += __shfl_xor(s, m, 64);
    if (row < rows && (threadIdx.x & 7) == 0) a.delta[row] = s;
}

// ---- dK, dV ----------------------------------------------------------------------------------------------------------------------------------------------
// LDS per stage (16-byte chunks): Q row-swizzled, dO row-swizzled, Q transpose-swizzled, dO transpose-swizzled, then 64 lse (base 2) and 64 D as floats
constexpr int DKDV_STAGE = 4 * TILE + 2 * KT / 4;

template <bool BF16, int BIAS>
__global__ __launch_bounds__(256, 2) void sdpa_h_bwd_dkdv_kernel(SdpaHBwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) u32x4 dsm[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int kb = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int key_raw = kb * KB + wave * 32 + li;
    const int key = min(key_raw, a.Lk - 1);
    const bool wave_active = (kb * KB + wave * 32) < a.Lk;
    const int my_kt = 2 * kb + (wave >> 1);                 // this wave's skip-map column

    // resident B operands of this lane's key
    u32x4 kf[4], vf[4];
    load_row_frags<BF16>(a.k, (long long)b * a.ks[0] + (long long)h * a.ks[1] + (long long)key * a.ks[2], a.k_f32, lh, kf);
    load_row_frags<BF16>(a.v, (long long)b * a.vs[0] + (long long)h * a.vs[1] + (long long)key * a.vs[2], 0, lh, vf);
    const long long boff = BIAS != HB_NONE ? (long long)b * a.bs[0] + (long long)h * a.bs[1] + key : 0;

    // staging: 64 queries x 8 chunks per operand, 2 chunks per thread (row = tid / 8 + 32 i, chunk = tid % 8); lse by threads 0..63, D by threads 64..127
    const int qes = a.q_f32 ? 4 : 2;                // bytes per Q element
    const char* qbase = reinterpret_cast<const char*>(a.q) + ((long long)b * a.qs[0] + (long long)h * a.qs[1]) * qes;
    const uint16_t* gbase = a.dout + (long long)b * a.gs[0] + (long long)h * a.gs[1];
    const float* lbase = (tid < KT ? a.lse : a.delta) + ((long long)b * a.H + h) * a.Lq;
    const int srow = tid >> 3, sch = tid & 7;
    u32x4 rq[2], rqh[2] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}}, rg[2];
    float rl = 0.f;
    auto load_tile = [&](int q0) {
        const char* pq[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int rc = min(q0 + srow + 32 * i, a.Lq - 1);
            pq[i] = qbase + ((long long)rc * a.qs[2] + 8 * sch) * qes;
            rq[i] = *reinterpret_cast<const u32x4*>(pq[i]);
            rg[i] = *reinterpret_cast<const u32x4*>(gbase + (long long)rc * a.gs[2] + 8 * sch);
        }
        if (a.q_f32) {
            rqh[0] = *reinterpret_cast<const u32x4*>(pq[0] + 16);
            rqh[1] = *reinterpret_cast<const u32x4*>(pq[1] + 16);
        }
        if (tid < 2 * KT) {
            const int r = q0 + (tid & (KT - 1));
            const float t = lbase[min(r, a.Lq - 1)];
            rl = r < a.Lq ? t : 0.f;
        }
    };
    auto store_tile = [&](int buf, int q0) {
        const u32x4 zero = {0u, 0u, 0u, 0u};
        u32x4* st = dsm + buf * DKDV_STAGE;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int row = srow + 32 * i;
            u32x4 qq = rq[i];
            if (a.q_f32) qq = pack8<BF16>(rq[i], rqh[i]);
            const bool in = q0 + row < a.Lq;
            qq = in ? qq : zero;
            const u32x4 gg = in ? rg[i] : zero;
            const int ir = row * 8 + (sch ^ ((row >> 1) & 7)), itr = row * 8 + (sch ^ (((row >> 1) & 1) << 2));
            st[ir] = qq; st[TILE + ir] = gg; st[2 * TILE + itr] = qq; st[3 * TILE + itr] = gg;
        }
        if (tid < 2 * KT) {
            float x = rl;
            // lse goes to base 2; a fully masked row (lse = -inf) gets +inf, so that its P = exp2(-inf - inf) = 0 and never exp2(-inf + inf)
            if (tid < KT) x = (x == -INFINITY) ? INFINITY : x * L2E;
            reinterpret_cast<float*>(st + 4 * TILE)[tid] = x;
        }
    };

    const int kswz = (li >> 1) & 7;
    // transposed-fragment addresses as in attention_sdpa_h_kernel
    const int q4 = (lane & 15) >> 2, p4 = lane & 3;
    const int vrow = 4 * lh + q4;
    const int vch[2] = {((0 ^ ((q4 >> 1) << 2)) + 2 * (li >> 4) + (p4 >> 1)), ((4 ^ ((q4 >> 1) << 2)) + 2 * (li >> 4) + (p4 >> 1))};

    f32x16 dk0, dk1, dv0, dv1;            // dK^T / dV^T accumulators: channel = db*32 + mrow(reg), column = this key
#pragma unroll
    for (int i = 0; i < 16; ++i) { dk0[i] = 0.f; dk1[i] = 0.f; dv0[i] = 0.f; dv1[i] = 0.f; }

    // the 64-query chunks this workgroup visits: both halves of every 128-query block that one of its two skip-map columns needs
    const int nch = (a.Lq + KT - 1) / KT;
    const bool mapped = BIAS != HB_NONE && a.skip != nullptr;
    const bool two_cols = 2 * kb + 1 < a.nkt;
    auto block_skipped = [&](int qb) {
        const uint8_t* r = a.skip + (size_t)qb * a.nkt + 2 * kb;
        return r[0] && (!two_cols || r[1]);
    };
    auto next_chunk = [&](int c) {
        if (mapped)
            while (c < nch && block_skipped(c >> 1)) c = ((c >> 1) + 1) * 2;
        return c;
    };

    int ch = next_chunk(0);
    if (ch < nch) {
        load_tile(ch * KT);
        store_tile(0, ch * KT);
    }
    __syncthreads();
    int buf = 0;
    while (ch < nch) {
        const int q0 = ch * KT;
        const int nxt = next_chunk(ch + 1);
        const int qn = (nxt < nch ? nxt : ch) * KT;
        load_tile(qn);                                      // always issues; dropped past the last chunk
        const bool mine = wave_active && !(mapped && my_kt < a.nkt && a.skip[(size_t)(ch >> 1) * a.nkt + my_kt]);
        if (mine) {                                         // wave-uniform: EXEC is all ones inside (the transposed reads need that)
            const u32x4* Qr = dsm + buf * DKDV_STAGE;
            const u32x4* Gr = Qr + TILE;
            const uint16_t* Qt = reinterpret_cast<const uint16_t*>(Qr + 2 * TILE);
            const uint16_t* Gt = reinterpret_cast<const uint16_t*>(Qr + 3 * TILE);
            const float* Lt = reinterpret_cast<const float*>(Qr + 4 * TILE);
#pragma unroll
            for (int sub = 0; sub < 2; ++sub) {
                // S = Q K^T and dP = dO V^T: [query mrow(r)][this key]
                f32x16 s, dp;
#pragma unroll
                for (int r = 0; r < 16; ++r) { s[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int idx = (32 * sub + li) * 8 + ((2 * c + lh) ^ kswz);
                    s = mfma_h<BF16>(Qr[idx], kf[c], s);
                    dp = mfma_h<BF16>(Gr[idx], vf[c], dp);
                }
                // P = exp2(score - lse) (0 for rows past Lq), dS = P (dP - D) (0 where P is 0)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = sub * 32 + mrow(r, lh);
                    const int qr = q0 + row;
                    float x;
                    if (BIAS == HB_NONE) x = s[r] * a.scale_l2e;
                    else {
                        const long long off = boff + (long long)min(qr, a.Lq - 1) * a.bs[2];
                        float bv;
                        if (BIAS == HB_F32) bv = reinterpret_cast<const float*>(a.bias)[off];
                        else if (BIAS == HB_U8) bv = reinterpret_cast<const uint8_t*>(a.bias)[off] ? 0.f : -INFINITY;
                        else bv = half_bits_to_float<BF16>(reinterpret_cast<const uint16_t*>(a.bias)[off]);
                        x = __builtin_fmaf(s[r], a.scale_l2e, bv * L2E);
                    }
                    const float p = qr < a.Lq ? __builtin_amdgcn_exp2f(x - Lt[row]) : 0.f;
                    s[r] = p;
                    dp[r] = p > 0.f ? p * (dp[r] - Lt[KT + row]) : 0.f;
                }
                // dV^T += dO^T P, dK^T += Q^T dS: k-step st = queries 32 sub + 16 st + {8 (j >> 2) + 4 lh + (j & 3)} = registers 8 st .. 8 st + 7
#pragma unroll
                for (int st = 0; st < 2; ++st) {
                    u32x4 pf, df;
#pragma unroll
                    for (int w = 0; w < 4; ++w) {
                        pf[w] = pack2<BF16>(s[8 * st + 2 * w], s[8 * st + 2 * w + 1]);
                        df[w] = pack2<BF16>(dp[8 * st + 2 * w], dp[8 * st + 2 * w + 1]);
                    }
                    const int row = 32 * sub + 16 * st + vrow;
                    dv0 = mfma_h<BF16>(read_tr(Gt, row, vch[0], p4), pf, dv0);
                    dv1 = mfma_h<BF16>(read_tr(Gt, row, vch[1], p4), pf, dv1);
                    dk0 = mfma_h<BF16>(read_tr(Qt, row, vch[0], p4), df, dk0);
                    dk1 = mfma_h<BF16>(read_tr(Qt, row, vch[1], p4), df, dk1);
                }
            }
        }
        if (nxt < nch) store_tile(buf ^ 1, qn);             // the other buffer: last read before the barrier that ended the previous iteration
        __syncthreads();
        ch = nxt; buf ^= 1;
    }

    if (wave_active && key_raw < a.Lk) {
        if (a.dk) {
            const long long off = (long long)b * a.dks[0] + (long long)h * a.dks[1] + (long long)key_raw * a.dks[2];
            store_row<BF16>(reinterpret_cast<char*>(a.dk) + off * (a.k_f32 ? 4 : 2), a.k_f32, lh, dk0, dk1, a.scale);
        }
        if (a.dv) store_row<BF16>(a.dv + (long long)b * a.dvs[0] + (long long)h * a.dvs[1] + (long long)key_raw * a.dvs[2], 0, lh, dv0, dv1, 1.0f);
    }
}

// ---- dQ --------------------------------------------------------------------------------------------------------------------------------------------------
template <bool BF16, int BIAS>
__global__ __launch_bounds__(256, 2) void sdpa_h_bwd_dq_kernel(SdpaHBwdArgs a) {
    // [stage][K row-swizzled | V row-swizzled | K transpose-swizzled][64 keys x 8 chunks of 16 bytes]
    __shared__ __attribute__((aligned(16))) u32x4 smem[2][3][TILE];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int qt = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int q0 = qt * QB;
    const int qi_raw = q0 + wave * 32 + li;
    const int qi = min(qi_raw, a.Lq - 1);
    const bool wave_active = (q0 + wave * 32) < a.Lq;

    // Q and dO fragments of this lane's query (B operands of S^T = K Q^T and dP^T = V dO^T)
    u32x4 qf[4], gf[4];
    load_row_frags<BF16>(a.q, (long long)b * a.qs[0] + (long long)h * a.qs[1] + (long long)qi * a.qs[2], a.q_f32, lh, qf);
    load_row_frags<BF16>(a.dout, (long long)b * a.gs[0] + (long long)h * a.gs[1] + (long long)qi * a.gs[2], 0, lh, gf);
    const long long rowid = ((long long)b * a.H + h) * a.Lq + qi;
    const float lse_n = a.lse[rowid], dlt = a.delta[rowid];
    const float lse2 = (lse_n == -INFINITY) ? INFINITY : lse_n * L2E;          // a fully masked row: P = exp2(-inf - inf) = 0
    const char* brow = nullptr;
    if (BIAS != HB_NONE) {
        const long long off = (long long)b * a.bs[0] + (long long)h * a.bs[1] + (long long)qi * a.bs[2];
        brow = reinterpret_cast<const char*>(a.bias) + off * (BIAS == HB_F32 ? 4 : BIAS == HB_U8 ? 1 : 2);
    }

    // staging as in attention_sdpa_hm_kernel
    const int kes = a.k_f32 ? 4 : 2;                // bytes per K element
    const char* kbase = reinterpret_cast<const char*>(a.k) + ((long long)b * a.ks[0] + (long long)h * a.ks[1]) * kes;
    const uint16_t* vbase = a.v + (long long)b * a.vs[0] + (long long)h * a.vs[1];
    const int skey = tid >> 3, sch = tid & 7;
    u32x4 rk[2], rkh[2] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}}, rv[2];
    auto load_tile = [&](int k0) {
        const char* pk[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int kc = min(k0 + skey + 32 * i, a.Lk - 1);
            pk[i] = kbase + ((long long)kc * a.ks[2] + 8 * sch) * kes;
            rk[i] = *reinterpret_cast<const u32x4*>(pk[i]);
            rv[i] = *reinterpret_cast<const u32x4*>(vbase + (long long)kc * a.vs[2] + 8 * sch);
        }
        if (a.k_f32) {
            rkh[0] = *reinterpret_cast<const u32x4*>(pk[0] + 16);
            rkh[1] = *reinterpret_cast<const u32x4*>(pk[1] + 16);
        }
    };
    auto store_tile = [&](int buf, int k0) {
        const u32x4 zero = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int key = skey + 32 * i;
            u32x4 kk = rk[i];
            if (a.k_f32) kk = pack8<BF16>(rk[i], rkh[i]);
            const bool in = k0 + key < a.Lk;
            kk = in ? kk : zero;
            const int ir = key * 8 + (sch ^ ((key >> 1) & 7));
            smem[buf][0][ir] = kk;
            smem[buf][1][ir] = in ? rv[i] : zero;
            smem[buf][2][key * 8 + (sch ^ (((key >> 1) & 1) << 2))] = kk;
        }
    };
    // The bias of a tile, raw bits: this lane's keys k0 + 32 sub + 8 g + 4 lh + e -> bq[4 sub + g], e = 0..3 (attention_sdpa_hm_kernel's two workgroup-uniform paths)
    auto fetch_bias = [&](int k0, u32x4 (&bq)[8]) {
        if (BIAS == HB_NONE) return;
        if (a.bias_vec && k0 + KT <= a.Lk) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int key = k0 + (j >> 2) * 32 + 8 * (j & 3) + 4 * lh;
                if (BIAS == HB_F32) bq[j] = *reinterpret_cast<const u32x4*>(brow + 4 * (long long)key);
                else if (BIAS == HB_U8) bq[j][0] = *reinterpret_cast<const uint32_t*>(brow + key);
                else { const u32x2 t2 = *reinterpret_cast<const u32x2*>(brow + 2 * (long long)key); bq[j][0] = t2[0]; bq[j][1] = t2[1]; }
            }
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int kc = min(k0 + (j >> 2) * 32 + 8 * (j & 3) + 4 * lh + e, a.Lk - 1);
                    if (BIAS == HB_F32) bq[j][e] = reinterpret_cast<const uint32_t*>(brow)[kc];
                    else if (BIAS == HB_U8) bq[j][e] = reinterpret_cast<const uint8_t*>(brow)[kc];
                    else bq[j][e] = reinterpret_cast<const uint16_t*>(brow)[kc];
                }
        }
    };
    auto bias_value = [&](const u32x4 (&bq)[8], int j, int e, bool packed) -> float {
        if (BIAS == HB_F32) return __uint_as_float(bq[j][e]);
        if (BIAS == HB_U8) return ((packed ? (bq[j][0] >> (8 * e)) & 0xFFu : bq[j][e]) != 0u) ? 0.f : -INFINITY;
        return half_bits_to_float<BF16>(packed ? (bq[j][e >> 1] >> (16 * (e & 1))) & 0xFFFFu : bq[j][e]);
    };

    const int kswz = (li >> 1) & 7;
    const int q4 = (lane & 15) >> 2, p4 = lane & 3;
    const int vrow = 4 * lh + q4;
    const int vch[2] = {((0 ^ ((q4 >> 1) << 2)) + 2 * (li >> 4) + (p4 >> 1)), ((4 ^ ((q4 >> 1) << 2)) + 2 * (li >> 4) + (p4 >> 1))};

    f32x16 dq0, dq1;                      // dQ^T accumulators: channel = db*32 + mrow(reg), column = this query
#pragma unroll
    for (int i = 0; i < 16; ++i) { dq0[i] = 0.f; dq1[i] = 0.f; }

    // the tiles this workgroup visits: the forward's walk
    const int ntiles = (a.Lk + KT - 1) / KT;
    const uint8_t* skip_row = (BIAS != HB_NONE && a.skip) ? a.skip + (size_t)qt * a.nkt : nullptr;
    auto next_tile = [&](int t) {
        if (BIAS != HB_NONE && skip_row)
            while (t < ntiles && skip_row[t]) ++t;
        return t;
    };

    int t = next_tile(0);
    if (t < ntiles) {
        load_tile(t * KT);
        store_tile(0, t * KT);
    }
    __syncthreads();
    int buf = 0;
    while (t < ntiles) {
        const int k0 = t * KT;
        const int nxt = next_tile(t + 1);
        u32x4 bq[8];
        if (wave_active) fetch_bias(k0, bq);
        const int kn = (nxt < ntiles ? nxt : t) * KT;
        load_tile(kn);                                      // always issues; dropped past the last tile
        if (wave_active) {                                  // wave-uniform: EXEC is all ones inside (the transposed reads need that)
            const u32x4* Kr = smem[buf][0];
            const u32x4* Vr = smem[buf][1];
            const uint16_t* Kt = reinterpret_cast<const uint16_t*>(smem[buf][2]);
            const bool full = k0 + KT <= a.Lk;
            const bool packed = a.bias_vec && full;
#pragma unroll
            for (int sub = 0; sub < 2; ++sub) {
                // S^T = K Q^T and dP^T = V dO^T: [key mrow(r)][this query]
                f32x16 s, dp;
#pragma unroll
                for (int r = 0; r < 16; ++r) { s[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int idx = (32 * sub + li) * 8 + ((2 * c + lh) ^ kswz);
                    s = mfma_h<BF16>(Kr[idx], qf[c], s);
                    dp = mfma_h<BF16>(Vr[idx], gf[c], dp);
                }
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int key = k0 + 32 * sub + mrow(i, lh);
                    float x;
                    if (BIAS == HB_NONE) x = s[i] * a.scale_l2e;
                    else x = __builtin_fmaf(s[i], a.scale_l2e, bias_value(bq, 4 * sub + (i >> 2), i & 3, packed) * L2E);
                    x = (!full && key >= a.Lk) ? -INFINITY : x;
                    const float p = __builtin_amdgcn_exp2f(x - lse2);
                    dp[i] = p > 0.f ? p * (dp[i] - dlt) : 0.f;
                }
                // dQ^T += K^T dS^T: k-step st = keys 32 sub + 16 st + {8 (j >> 2) + 4 lh + (j & 3)} = registers 8 st .. 8 st + 7
#pragma unroll
                for (int st = 0; st < 2; ++st) {
                    u32x4 df;
#pragma unroll
                    for (int w = 0; w < 4; ++w) df[w] = pack2<BF16>(dp[8 * st + 2 * w], dp[8 * st + 2 * w + 1]);
                    const int row = 32 * sub + 16 * st + vrow;
                    dq0 = mfma_h<BF16>(read_tr(Kt, row, vch[0], p4), df, dq0);
                    dq1 = mfma_h<BF16>(read_tr(Kt, row, vch[1], p4), df, dq1);
                }
            }
        }
        if (nxt < ntiles) store_tile(buf ^ 1, kn);          // the other buffer: last read before the barrier that ended the previous iteration
        __syncthreads();
        t = nxt; buf ^= 1;
    }

    if (wave_active && qi_raw < a.Lq) {
        const long long off = (long long)b * a.dqs[0] + (long long)h * a.dqs[1] + (long long)qi_raw * a.dqs[2];
        store_row<BF16>(reinterpret_cast<char*>(a.dq) + off * (a.q_f32 ? 4 : 2), a.q_f32, lh, dq0, dq1, a.scale);
    }
}

bool strides_ok(const long long* s, int mult) { return s[0] % mult == 0 && s[1] % mult == 0 && s[2] % mult == 0 && s[0] >= 0 && s[1] >= 0 && s[2] >= 0; }

typedef void (*SdpaHBwdKernel)(SdpaHBwdArgs);
template <bool BF16>
SdpaHBwdKernel dkdv_variant(int kind) {
    switch (kind) {
        case HB_F32: return sdpa_h_bwd_dkdv_kernel<BF16, HB_F32>;
        case HB_U8: return sdpa_h_bwd_dkdv_kernel<BF16, HB_U8>;
        case HB_HALF: return sdpa_h_bwd_dkdv_kernel<BF16, HB_HALF>;
        default: return sdpa_h_bwd_dkdv_kernel<BF16, HB_NONE>;
    }
}
template <bool BF16>
SdpaHBwdKernel dq_variant(int kind) {
    switch (kind) {
        case HB_F32: return sdpa_h_bwd_dq_kernel<BF16, HB_F32>;
        case HB_U8: return sdpa_h_bwd_dq_kernel<BF16, HB_U8>;
        case HB_HALF: return sdpa_h_bwd_dq_kernel<BF16, HB_HALF>;
        default: return sdpa_h_bwd_dq_kernel<BF16, HB_NONE>;
    }
}

}  // namespace

// strides: 24 element strides, (batch, head, token) of q, k, v, out, dout, dq, dk, dv in that order, each in ITS tensor's elements (q, dq / k, dk: fp32 where flagged);
// dtype 1 = fp16, 2 = bf16; delta: workspace of B*H*Lq floats
int attention_sdpa_h_bwd(const void* q, const void* k, const void* v, const void* out, const void* dout, const float* lse, float* delta, void* dq, void* dk, void* dv,
                         const long long* strides, int dtype, int q_f32, int k_f32, const void* bias, int kind, const long long* bs, const uint8_t* skip, int B, int H,
                         int Lq, int Lk, int head_dim, double scale, hipStream_t stream) {
    SDVAR_CHECK_ARG(q && k && v && out && dout && strides, "sdpa_h_bwd: null operand");
    SDVAR_CHECK_ARG(lse, "sdpa_h_bwd: null lse");
    SDVAR_CHECK_ARG(delta, "sdpa_h_bwd: null delta workspace");
    SDVAR_CHECK_ARG(dq || dk || dv, "sdpa_h_bwd: dq, dk and dv are all NULL - nothing to compute");
    SDVAR_CHECK_ARG(dtype == 1 || dtype == 2, "sdpa_h_bwd: dtype %d (1 = fp16, 2 = bf16)", dtype);
    SDVAR_CHECK_ARG((q_f32 == 0 || q_f32 == 1) && (k_f32 == 0 || k_f32 == 1), "sdpa_h_bwd: q_f32 = %d, k_f32 = %d (0 or 1)", q_f32, k_f32);
    SDVAR_CHECK_ARG(head_dim == 64, "sdpa_h_bwd: head dim %d (only 64 is built)", head_dim);
    SDVAR_CHECK_ARG(B >= 1 && H >= 1 && Lq >= 1 && Lk >= 1 && B <= 65535 && H <= 65535, "sdpa_h_bwd: bad extents B=%d H=%d Lq=%d Lk=%d", B, H, Lq, Lk);
    SDVAR_CHECK_ARG(((long long)B * H * Lq + 31) / 32 <= 2147483647LL, "sdpa_h_bwd: B*H*Lq too large");
    static const char* const names[8] = {"q", "k", "v", "out", "dout", "dq", "dk", "dv"};
    const void* const ptrs[8] = {q, k, v, out, dout, dq, dk, dv};
    const bool f32[8] = {q_f32 != 0, k_f32 != 0, false, false, false, q_f32 != 0, k_f32 != 0, false};
    for (int i = 0; i < 8; ++i) {
        if (!ptrs[i]) continue;             // an absent gradient
        SDVAR_CHECK_ARG(strides_ok(strides + 3 * i, f32[i] ? 4 : 8),
                        "sdpa_h_bwd: %s strides (%lld, %lld, %lld) - token rows must be 16-byte aligned (every stride a non-negative multiple of %d elements)", names[i],
                        strides[3 * i], strides[3 * i + 1], strides[3 * i + 2], f32[i] ? 4 : 8);
        SDVAR_CHECK_ARG(((uintptr_t)ptrs[i] & 15) == 0, "sdpa_h_bwd: %s is not 16-byte aligned", names[i]);
    }
    SDVAR_CHECK_ARG((((uintptr_t)lse | (uintptr_t)delta) & 3) == 0, "sdpa_h_bwd: lse / delta is not 4-byte aligned");
    SDVAR_CHECK_ARG(kind >= HB_NONE && kind <= HB_HALF, "sdpa_h_bwd: bias kind %d (0 = none, 1 = fp32 additive, 2 = uint8 keep-mask, 3 = additive in dtype)", kind);
    SDVAR_CHECK_ARG((kind == HB_NONE) == (bias == nullptr), "sdpa_h_bwd: bias pointer and bias kind %d disagree", kind);
    SDVAR_CHECK_ARG(kind == HB_NONE || (bs && bs[0] >= 0 && bs[1] >= 0 && bs[2] >= 0), "sdpa_h_bwd: bias strides missing or negative");
    SDVAR_CHECK_ARG(kind != HB_HALF || ((uintptr_t)bias & 1) == 0, "sdpa_h_bwd: a half bias at an odd address");
    SDVAR_CHECK_ARG(kind != HB_F32 || ((uintptr_t)bias & 3) == 0, "sdpa_h_bwd: an fp32 bias that is not 4-byte aligned");
    SDVAR_CHECK_ARG(kind != HB_NONE || !skip, "sdpa_h_bwd: a skip map needs a bias");
    SdpaHBwdArgs a;
    a.q = q; a.k = k; a.v = (const uint16_t*)v; a.out = (const uint16_t*)out; a.dout = (const uint16_t*)dout; a.lse = lse; a.delta = delta;
    a.dq = dq; a.dk = dk; a.dv = (uint16_t*)dv;
    for (int i = 0; i < 3; ++i) {
        a.qs[i] = strides[i]; a.ks[i] = strides[3 + i]; a.vs[i] = strides[6 + i]; a.os[i] = strides[9 + i]; a.gs[i] = strides[12 + i];
        a.dqs[i] = strides[15 + i]; a.dks[i] = strides[18 + i]; a.dvs[i] = strides[21 + i]; a.bs[i] = kind ? bs[i] : 0;
    }
    a.bias = bias; a.skip = skip; a.nkt = (Lk + KT - 1) / KT;
    const uintptr_t balign = kind == HB_F32 ? 15 : kind == HB_U8 ? 3 : 7;
    a.bias_vec = kind != HB_NONE && ((uintptr_t)bias & balign) == 0 && bs[0] % 4 == 0 && bs[1] % 4 == 0 && bs[2] % 4 == 0;
    a.q_f32 = q_f32; a.k_f32 = k_f32;
    a.B = B; a.H = H; a.Lq = Lq; a.Lk = Lk; a.scale = (float)scale; a.scale_l2e = (float)(scale * 1.4426950408889634);

    const long long rows = (long long)B * H * Lq;
    if (dtype == 2) hipLaunchKernelGGL(sdpa_h_bwd_delta_kernel<true>, dim3((unsigned)((rows + 31) / 32)), dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(sdpa_h_bwd_delta_kernel<false>, dim3((unsigned)((rows + 31) / 32)), dim3(256), 0, stream, a);
    SDVAR_LAUNCH_CHECK();
    if (dk || dv) {
        const size_t lds = 2 * (size_t)DKDV_STAGE * sizeof(u32x4);
        static LdsOptIn opt_in;
        SDVAR_LDS_OPT_IN(opt_in, lds, (const void*)dkdv_variant<false>(HB_NONE), (const void*)dkdv_variant<false>(HB_F32), (const void*)dkdv_variant<false>(HB_U8),
                         (const void*)dkdv_variant<false>(HB_HALF), (const void*)dkdv_variant<true>(HB_NONE), (const void*)dkdv_variant<true>(HB_F32),
                         (const void*)dkdv_variant<true>(HB_U8), (const void*)dkdv_variant<true>(HB_HALF));
        const dim3 grid((Lk + KB - 1) / KB, H, B);
        hipLaunchKernelGGL(dtype == 2 ? dkdv_variant<true>(kind) : dkdv_variant<false>(kind), grid, dim3(256), lds, stream, a);
        SDVAR_LAUNCH_CHECK();
    }
    if (dq) {
        const dim3 grid((Lq + QB - 1) / QB, H, B);
        hipLaunchKernelGGL(dtype == 2 ? dq_variant<true>(kind) : dq_variant<false>(kind), grid, dim3(256), 0, stream, a);
        SDVAR_LAUNCH_CHECK();
    }
    return SDVAR_OK;
}

}  // namespace sdvar
