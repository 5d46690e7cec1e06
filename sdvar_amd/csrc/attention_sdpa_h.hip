// Operator-seam attention on half-precision operands: out = softmax(scale q k^T) v for the reference's flash_attn_func slot (models/basic_var.py:23, called at
// :113 when KV caching is on and qkv is not fp32, :97-98).  q, k, v and out are all fp16 or all bf16; the products run on the native half-precision matrix
// cores (v_mfma_f32_32x32x16_f16 / _bf16), everything between them in fp32.  No bias, no mask (the reference never passes one to this slot).
//
// Arithmetic contract (what tests/test_gpu_seam_flash.py holds the kernel to):
//   * scores accumulate in fp32 from the half operands; `scale` multiplies the fp32 score (Q stays as given, it is never rescaled in half precision);
//   * online softmax in fp32 over 64-key tiles; the row sum l is the sum of the fp32 weights p (NOT of the rounded ones);
//   * p is rounded to the operand dtype with round-to-nearest-even (v_cvt_pk_f16_f32 / v_cvt_pk_bf16_f32) for the P V product; O accumulates in fp32;
//   * one final rounding of O / l to the operand dtype (RNE).  No atomics: repeated calls are bit-identical.
//
// Shape: 128 queries of one (batch, head) per 4-wave workgroup, 32 per wave, the query on the lane.  S^T = K Q^T, so the 32 keys of a sub-tile sit in the 16
// accumulator registers of the two lane halves (key = (reg & 3) + 8 (reg >> 2) + 4 half): the row maximum is an in-lane reduction plus one exchange with the
// other half, and the converted accumulators ARE the B operand of O^T = V^T P^T (registers 8s .. 8s+7 = the 16 keys of k-step s, in the order
// 16 s + 8 (j >> 2) + 4 half + (j & 3)); P never goes through LDS.  The V^T fragments with that key order come from the row-major V tile by two
// ds_read_b64_tr_b16 per fragment (4 keys x 16 channels per 16-lane group, delivered channel on the lane).
// K and V tiles (64 keys x 128 bytes each) are double-buffered in LDS, staged through registers one tile ahead.  16-byte chunks are XOR-swizzled so that both
// read patterns are bank-conflict-free on unpadded 128-byte rows:  K chunk ^= (key >> 1) & 7 (ds_read_b128, one key per lane);  V chunk ^= 4 ((key >> 1) & 1)
// (transposed reads: the four keys of a block land on four different 16-bank quarters).
// Operands are STRIDED like sdvar_op_sdpa's: element strides for (batch, head, token), channel stride 1; every token row is moved with 16-byte accesses, so base
// pointers % 16 == 0 and every stride % 8 == 0 (elements of 2 bytes).  Lq and Lk are independent, any value >= 1: K/V rows past Lk are zero-filled in
// staging and their scores set to -inf; query rows past Lq compute on a clamped row and are never stored.
#include "common.h"

namespace sdvar {

namespace {

constexpr int KT = 64;              // keys per LDS tile
constexpr int QB = 128;             // queries per workgroup

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2p __attribute__((ext_vector_type(2)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

struct SdpaHArgs {
    const uint16_t *q, *k, *v; uint16_t* out;
    long long qs[3], ks[3], vs[3], os[3];       // element strides: batch, head, token
    int B, H, Lq, Lk;
    float scale_l2e;                            // scale * log2(e): the softmax runs in base 2
};

// two fp32 -> one packed word of two halves, round to nearest even
template <bool BF16>
__device__ __forceinline__ uint32_t pack2(float a, float b) {
    const f32x2p v = {a, b};
    if (BF16) return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2p));         // v_cvt_pk_bf16_f32
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, f16x2p));                     // v_cvt_pk_f16_f32
}

template <bool BF16>
__device__ __forceinline__ f32x16 mfma_h(u32x4 a, u32x4 b, f32x16 c) {
    if (BF16) return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

template <bool BF16>
__global__ __launch_bounds__(256, 2) void attention_sdpa_h_kernel(SdpaHArgs a) {
    // [stage][K | V][64 keys x 8 chunks of 16 bytes]
    __shared__ __attribute__((aligned(16))) u32x4 smem[2][2][KT * 8];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int qt = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int q0 = qt * QB;

    const int qi_raw = q0 + wave * 32 + li;
    const int qi = min(qi_raw, a.Lq - 1);
    const bool wave_active = (q0 + wave * 32) < a.Lq;

    // Q fragments (B operand of S^T = K Q^T): k-step c, lane (query li, half lh) holds channels 16 c + 8 lh + 0..7
    u32x4 qf[4];
    {
        const uint16_t* pq = a.q + (long long)b * a.qs[0] + (long long)h * a.qs[1] + (long long)qi * a.qs[2] + 8 * lh;
#pragma unroll
        for (int c = 0; c < 4; ++c) qf[c] = *reinterpret_cast<const u32x4*>(pq + 16 * c);
    }

    // staging: 64 keys x 8 chunks per operand, 2 chunks per thread (key = tid / 8 + 32 i, chunk = tid % 8): 8 consecutive threads move one 128-byte row
    const uint16_t* kbase = a.k + (long long)b * a.ks[0] + (long long)h * a.ks[1];
    const uint16_t* vbase = a.v + (long long)b * a.vs[0] + (long long)h * a.vs[1];
    const int skey = tid >> 3, sch = tid & 7;
    u32x4 rk[2], rv[2];
    // branch-free: rows past Lk read the last row and are zeroed
    auto load_tile = [&](int k0) {
        const u32x4 zero = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int key = k0 + skey + 32 * i, kc = min(key, a.Lk - 1);
            const u32x4 tk = *reinterpret_cast<const u32x4*>(kbase + (long long)kc * a.ks[2] + 8 * sch);
            const u32x4 tv = *reinterpret_cast<const u32x4*>(vbase + (long long)kc * a.vs[2] + 8 * sch);
            rk[i] = key < a.Lk ? tk : zero; rv[i] = key < a.Lk ? tv : zero;
        }
    };
    auto store_tile = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int key = skey + 32 * i;
            smem[buf][0][key * 8 + (sch ^ ((key >> 1) & 7))] = rk[i];
            smem[buf][1][key * 8 + (sch ^ (((key >> 1) & 1) << 2))] = rv[i];
        }
    };

    // K fragment of sub-tile `sub`, k-step c: key 32 sub + li, chunk 2 c + lh.  (32 sub does not change (key >> 1) & 7 beyond li's bits: 32 >> 1 = 16.)
    const int kswz = (li >> 1) & 7;
    // V^T fragment addresses: this lane supplies row q4 of a 4-key block, channels 16 (li >> 4) + 4 p4 .. + 3 of a 32-channel block (cdna T10); the block's
    // first key is a multiple of 4, so the row's swizzle bit is q4 >> 1 for every block.
    const int q4 = (lane & 15) >> 2, p4 = lane & 3;
    const int vrow = 4 * lh + q4;                                   // + 32 sub + 16 s (+ 8 for the second half of the fragment)
    const int vch[2] = {((0 ^ ((q4 >> 1) << 2)) + 2 * (li >> 4) + (p4 >> 1)), ((4 ^ ((q4 >> 1) << 2)) + 2 * (li >> 4) + (p4 >> 1))};

    f32x16 o0, o1;                        // O^T accumulators: d = db*32 + (reg&3) + 8*(reg>>2) + 4*lh, column = this query
#pragma unroll
    for (int i = 0; i < 16; ++i) { o0[i] = 0.f; o1[i] = 0.f; }
    float m_run = -INFINITY, l_run = 0.f;           // m_run in the base-2 domain (scaled score * log2 e)

    const int ntiles = (a.Lk + KT - 1) / KT;
    load_tile(0);
    store_tile(0);
    __syncthreads();
    for (int t = 0; t < ntiles; ++t) {
        const int k0 = t * KT, buf = t & 1;
        const bool more = t + 1 < ntiles;
        if (more) load_tile(k0 + KT);                       // in flight under this tile's arithmetic
        if (wave_active) {                                  // wave-uniform: EXEC is all ones inside (the transposed reads need that)
            const u32x4* ks = smem[buf][0];
            const uint16_t* vs16 = reinterpret_cast<const uint16_t*>(smem[buf][1]);
            // ---- S^T = K Q^T: two 32-key sub-tiles x four 16-channel k-steps
            f32x16 s[2];
#pragma unroll
            for (int sub = 0; sub < 2; ++sub) {
#pragma unroll
                for (int i = 0; i < 16; ++i) s[sub][i] = 0.f;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const u32x4 kf = ks[(32 * sub + li) * 8 + ((2 * c + lh) ^ kswz)];
                    s[sub] = mfma_h<BF16>(kf, qf[c], s[sub]);
                }
            }
            // ---- scale in fp32, keys past Lk -> -inf (last tile only)
            const bool full = k0 + KT <= a.Lk;
#pragma unroll
            for (int sub = 0; sub < 2; ++sub)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int key = k0 + 32 * sub + (i & 3) + 8 * (i >> 2) + 4 * lh;
                    const float x = s[sub][i] * a.scale_l2e;
                    s[sub][i] = (!full && key >= a.Lk) ? -INFINITY : x;
                }
            // ---- online softmax (this lane: one query; the other half of its keys lives in lane ^ 32)
            float mloc = -INFINITY;
#pragma unroll
            for (int sub = 0; sub < 2; ++sub)
#pragma unroll
                for (int i = 0; i < 16; ++i) mloc = fmaxf(mloc, s[sub][i]);
            mloc = fmaxf(mloc, __shfl_xor(mloc, 32, 64));
            const float m_new = fmaxf(m_run, mloc);         // finite: every visited tile has at least one key < Lk
            const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
            float lsum = 0.f;
#pragma unroll
            for (int sub = 0; sub < 2; ++sub)
#pragma unroll
                for (int i = 0; i < 16; ++i) { s[sub][i] = __builtin_amdgcn_exp2f(s[sub][i] - m_new); lsum += s[sub][i]; }
            lsum += __shfl_xor(lsum, 32, 64);
            l_run = l_run * alpha + lsum;
            m_run = m_new;
#pragma unroll
            for (int i = 0; i < 16; ++i) { o0[i] *= alpha; o1[i] *= alpha; }
            // ---- O^T += V^T P^T: k-step (sub, st) = keys 32 sub + 16 st + {8 (j >> 2) + 4 lh + (j & 3)}
#pragma unroll
            for (int sub = 0; sub < 2; ++sub)
#pragma unroll
                for (int st = 0; st < 2; ++st) {
                    u32x4 pf;
#pragma unroll
                    for (int w = 0; w < 4; ++w) pf[w] = pack2<BF16>(s[sub][8 * st + 2 * w], s[sub][8 * st + 2 * w + 1]);
                    const int row = 32 * sub + 16 * st + vrow;
#pragma unroll
                    for (int db = 0; db < 2; ++db) {
                        typedef __attribute__((address_space(3))) s16x4* lds_s16x4;
                        const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)(vs16 + row * 64 + vch[db] * 8 + 4 * (p4 & 1)));
                        const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)(vs16 + (row + 8) * 64 + vch[db] * 8 + 4 * (p4 & 1)));
                        const u32x2 l2 = __builtin_bit_cast(u32x2, lo), h2 = __builtin_bit_cast(u32x2, hi);
                        const u32x4 vf = {l2[0], l2[1], h2[0], h2[1]};
                        if (db == 0) o0 = mfma_h<BF16>(vf, pf, o0);
                        else o1 = mfma_h<BF16>(vf, pf, o1);
                    }
                }
        }
        if (more) store_tile(buf ^ 1);                      // the other buffer: last read before the barrier that ended the previous iteration
        __syncthreads();
    }

    if (wave_active && qi_raw < a.Lq) {
        const float inv = 1.0f / l_run;
        uint16_t* po = a.out + (long long)b * a.os[0] + (long long)h * a.os[1] + (long long)qi_raw * a.os[2] + 4 * lh;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            u32x2 w0, w1;
            w0[0] = pack2<BF16>(o0[4 * g] * inv, o0[4 * g + 1] * inv); w0[1] = pack2<BF16>(o0[4 * g + 2] * inv, o0[4 * g + 3] * inv);
            w1[0] = pack2<BF16>(o1[4 * g] * inv, o1[4 * g + 1] * inv); w1[1] = pack2<BF16>(o1[4 * g + 2] * inv, o1[4 * g + 3] * inv);
            *reinterpret_cast<u32x2*>(po + 8 * g) = w0;
            *reinterpret_cast<u32x2*>(po + 32 + 8 * g) = w1;
        }
    }
}

bool aligned_strides_h(const long long* s) { return s[0] % 8 == 0 && s[1] % 8 == 0 && s[2] % 8 == 0 && s[0] >= 0 && s[1] >= 0 && s[2] >= 0; }

// ---------------------------------------------------------------------------------------------------------------------------------------------------------------
// The masked, mixed-operand variant (sdvar_op_sdpa_hm; the reference's slow_attn / memory_efficient_attention slots under torch.autocast, basic_var.py:115-117):
// out = softmax(scale q k^T + bias) v.  Shape, MFMA mapping, LDS image, swizzles and arithmetic contract are attention_sdpa_h_kernel's; what is new:
//   * q and k are EACH either the half dtype or fp32 (a.q_f32 / a.k_f32, uniform over the launch).  An fp32 operand is read with 16-byte loads (two per 8 channels)
//     and rounded to the half dtype with v_cvt_pk_*_f32 (RNE) on its way into the Q fragments / out of the K staging registers: the bits of a prior .to(dtype).
//     v and out are always the half dtype.  fp32 rows follow sdvar_op_sdpa's alignment rule (pointer % 16 == 0, strides % 4 == 0).
//   * bias kinds (template): 1 fp32 additive (finite or -inf), 2 uint8 keep-mask (0 -> -inf), 3 additive in the half dtype; element strides (batch, head, query
//     row), 0 = broadcast, key stride 1, rows of any alignment.  The raw bits of a tile (this lane: 8 groups of 4 consecutive keys) are loaded BEFORE the K/V
//     prefetch and the score MFMAs - 8 vector loads where rows are aligned and the tile is whole, else 32 clamped element loads, both free of per-lane branches -
//     and enter the fp32 score AFTER the MFMAs as fma(s, scale log2 e, bias log2 e): they land under the MFMAs instead of in front of them.
//   * online softmax under -inf: while a query's running maximum is still -inf (a visited tile fully masked for THIS query) the exponent reference is 0, so the
//     tile contributes exp2(-inf) = 0 and never exp2(-inf - (-inf)).  A row with every key masked ends as 0 / 0 (unspecified; no fault, other rows untouched).
//   * skip map (sdpa_skip_map's format: one byte per (128-query block, 64-key tile)): marked tiles are never staged, prefetched or multiplied; the one-tile-ahead
//     prefetch targets the next UNMARKED tile.
//   * LSE (template, sdvar_op_sdpa_hm_lse): each stored query row also writes lse = ln 2 (m_run + log2 l_run), the natural log-sum-exp of its fp32 scores, what the
//     backward (attention_sdpa_h_bwd.hip) recomputes P from.  A compile-time flag: the instantiations without it keep their code and their bits, and the ones with it
//     change nothing in front of the final store, so `out` is the same bits.
enum { HB_NONE = 0, HB_F32 = 1, HB_U8 = 2, HB_HALF = 3 };

struct SdpaHmArgs {
    const void *q, *k; const uint16_t* v; uint16_t* out;
    long long qs[3], ks[3], vs[3], os[3];       // element strides: batch, head, token
    const void* bias; long long bs[3];          // element strides: batch, head, query row (0 = broadcast)
    int bias_vec;                               // bias rows allow 4-element vector loads (16 bytes fp32 / 4 bytes uint8 / 8 bytes half)
    const uint8_t* skip; int nkt;               // skip map (ceil(Lq/128), nkt) or nullptr
    int q_f32, k_f32;
    int B, H, Lq, Lk;
    float scale_l2e;
    float* lse;                                 // LSE instantiations only: (B, H, Lq) dense fp32; last, so the other instantiations' argument offsets do not move
};

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

template <bool BF16, int BIAS, bool LSE>
__global__ __launch_bounds__(256, 2) void attention_sdpa_hm_kernel(SdpaHmArgs a) {
    // [stage][K | V][64 keys x 8 chunks of 16 bytes]
    __shared__ __attribute__((aligned(16))) u32x4 smem[2][2][KT * 8];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int qt = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int q0 = qt * QB;

    const int qi_raw = q0 + wave * 32 + li;
    const int qi = min(qi_raw, a.Lq - 1);
    const bool wave_active = (q0 + wave * 32) < a.Lq;

    // Q fragments (B operand of S^T = K Q^T): k-step c, lane (query li, half lh) holds channels 16 c + 8 lh + 0..7
    u32x4 qf[4];
    {
        const long long qoff = (long long)b * a.qs[0] + (long long)h * a.qs[1] + (long long)qi * a.qs[2] + 8 * lh;
        if (a.q_f32) {
            const float* pq = reinterpret_cast<const float*>(a.q) + qoff;
#pragma unroll
            for (int c = 0; c < 4; ++c)
                qf[c] = pack8<BF16>(*reinterpret_cast<const u32x4*>(pq + 16 * c), *reinterpret_cast<const u32x4*>(pq + 16 * c + 4));
        } else {
            const uint16_t* pq = reinterpret_cast<const uint16_t*>(a.q) + qoff;
#pragma unroll
            for (int c = 0; c < 4; ++c) qf[c] = *reinterpret_cast<const u32x4*>(pq + 16 * c);
        }
    }
    // this lane's bias row (byte address)
    const char* brow = nullptr;
    if (BIAS != HB_NONE) {
        const long long off = (long long)b * a.bs[0] + (long long)h * a.bs[1] + (long long)qi * a.bs[2];
        brow = reinterpret_cast<const char*>(a.bias) + off * (BIAS == HB_F32 ? 4 : BIAS == HB_U8 ? 1 : 2);
    }

    // staging: 64 keys x 8 chunks per operand, 2 chunks per thread (key = tid / 8 + 32 i, chunk = tid % 8): 8 consecutive threads move one row (128 bytes of
    // halves or 256 bytes of fp32).  The raw registers are held across the tile's arithmetic; fp32 K is rounded in store_tile, after the wait.
    const int kes = a.k_f32 ? 4 : 2;                // bytes per K element
    const char* kbase = reinterpret_cast<const char*>(a.k) + ((long long)b * a.ks[0] + (long long)h * a.ks[1]) * kes;
    const uint16_t* vbase = a.v + (long long)b * a.vs[0] + (long long)h * a.vs[1];
    const int skey = tid >> 3, sch = tid & 7;
    u32x4 rk[2], rkh[2] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}}, rv[2];              // rkh: the second 16 bytes of an fp32 K chunk
    // branch-free per lane: rows past Lk read the last row and are zeroed in store_tile.  One address serves both K formats (chunk sch of the row is 8 elements);
    // only the second 16 bytes of an fp32 chunk sit behind a launch-uniform branch.
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
            smem[buf][0][key * 8 + (sch ^ ((key >> 1) & 7))] = in ? kk : zero;
            smem[buf][1][key * 8 + (sch ^ (((key >> 1) & 1) << 2))] = in ? rv[i] : zero;
        }
    };
    // The bias of a tile, raw bits: this lane's keys k0 + 32 sub + 8 g + 4 lh + e -> bq[4 sub + g], e = 0..3.  Two workgroup-uniform paths, both free of per-lane
    // branches: 8 vector loads (fp32: bq[j] = 4 floats; uint8: bq[j][0] = 4 bytes; half: bq[j][0..1] = 4 halves) or 32 clamped element loads (bq[j][e] = one
    // element, zero-extended).
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
    // the additive value (natural-log domain) of element e of group j; `packed` = the vector path filled bq
    auto bias_value = [&](const u32x4 (&bq)[8], int j, int e, bool packed) -> float {
        if (BIAS == HB_F32) return __uint_as_float(bq[j][e]);
        if (BIAS == HB_U8) return ((packed ? (bq[j][0] >> (8 * e)) & 0xFFu : bq[j][e]) != 0u) ? 0.f : -INFINITY;
        return half_bits_to_float<BF16>(packed ? (bq[j][e >> 1] >> (16 * (e & 1))) & 0xFFFFu : bq[j][e]);
    };

    // K fragment of sub-tile `sub`, k-step c: key 32 sub + li, chunk 2 c + lh.  (32 sub does not change (key >> 1) & 7 beyond li's bits: 32 >> 1 = 16.)
    const int kswz = (li >> 1) & 7;
    // V^T fragment addresses as in attention_sdpa_h_kernel
    const int q4 = (lane & 15) >> 2, p4 = lane & 3;
    const int vrow = 4 * lh + q4;
    const int vch[2] = {((0 ^ ((q4 >> 1) << 2)) + 2 * (li >> 4) + (p4 >> 1)), ((4 ^ ((q4 >> 1) << 2)) + 2 * (li >> 4) + (p4 >> 1))};

    f32x16 o0, o1;                        // O^T accumulators: d = db*32 + (reg&3) + 8*(reg>>2) + 4*lh, column = this query
#pragma unroll
    for (int i = 0; i < 16; ++i) { o0[i] = 0.f; o1[i] = 0.f; }
    float m_run = -INFINITY, l_run = 0.f;           // m_run in the base-2 domain (scaled score * log2 e)

    // the tiles this workgroup visits: every tile the skip map does not mark (workgroup-uniform walk)
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
    // The Q loads retire HERE: left to their first use inside the loop, the compiler's wait for them sits in front of the score MFMAs of every tile, where it also
    // drains the bias loads (loads retire in order).
#pragma unroll
    for (int c = 0; c < 4; ++c) asm volatile("" : "+v"(qf[c]));
    int buf = 0;
    while (t < ntiles) {
        const int k0 = t * KT;
        const int nxt = next_tile(t + 1);
        // The bias loads go out first, then the K/V prefetch of the next unmarked tile, which ALWAYS issues (past the last tile it re-reads the current one and is
        // dropped): loads retire in order, so the bias add after the score MFMAs waits for "all but the prefetch" and the prefetch stays in flight.
        u32x4 bq[8];
        if (wave_active) fetch_bias(k0, bq);
        const int kn = (nxt < ntiles ? nxt : t) * KT;
        load_tile(kn);
        __builtin_amdgcn_sched_barrier(0);
        if (wave_active) {                                  // wave-uniform: EXEC is all ones inside (the transposed reads need that)
            const u32x4* ks = smem[buf][0];
            const uint16_t* vs16 = reinterpret_cast<const uint16_t*>(smem[buf][1]);
            // ---- S^T = K Q^T: two 32-key sub-tiles x four 16-channel k-steps
            f32x16 s[2];
#pragma unroll
            for (int sub = 0; sub < 2; ++sub) {
#pragma unroll
                for (int i = 0; i < 16; ++i) s[sub][i] = 0.f;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const u32x4 kf = ks[(32 * sub + li) * 8 + ((2 * c + lh) ^ kswz)];
                    s[sub] = mfma_h<BF16>(kf, qf[c], s[sub]);
                }
            }
            // ---- scale and bias in fp32 (base-2 domain), keys past Lk -> -inf (last tile only).  The fence keeps the bias arithmetic, and with it the wait for
            // the bias loads, behind the score MFMAs.
            if (BIAS != HB_NONE) __builtin_amdgcn_sched_barrier(0);
            const bool full = k0 + KT <= a.Lk;
            const bool packed = a.bias_vec && full;
            const float L2E = 1.4426950408889634f;
#pragma unroll
            for (int sub = 0; sub < 2; ++sub)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int key = k0 + 32 * sub + (i & 3) + 8 * (i >> 2) + 4 * lh;
                    float x;
                    if (BIAS == HB_NONE) x = s[sub][i] * a.scale_l2e;
                    else x = __builtin_fmaf(s[sub][i], a.scale_l2e, bias_value(bq, 4 * sub + (i >> 2), i & 3, packed) * L2E);
                    s[sub][i] = (!full && key >= a.Lk) ? -INFINITY : x;
                }
            // ---- online softmax (this lane: one query; the other half of its keys lives in lane ^ 32)
            float mloc = -INFINITY;
#pragma unroll
            for (int sub = 0; sub < 2; ++sub)
#pragma unroll
                for (int i = 0; i < 16; ++i) mloc = fmaxf(mloc, s[sub][i]);
            mloc = fmaxf(mloc, __shfl_xor(mloc, 32, 64));
            const float m_new = fmaxf(m_run, mloc);
            // every key so far masked for this query: exponent reference 0, so this tile's weights are exp2(-inf) = 0 and alpha = exp2(-inf) = 0
            const float m_ref = (m_new == -INFINITY) ? 0.f : m_new;
            const float alpha = __builtin_amdgcn_exp2f(m_run - m_ref);
            float lsum = 0.f;
#pragma unroll
            for (int sub = 0; sub < 2; ++sub)
#pragma unroll
                for (int i = 0; i < 16; ++i) { s[sub][i] = __builtin_amdgcn_exp2f(s[sub][i] - m_ref); lsum += s[sub][i]; }
            lsum += __shfl_xor(lsum, 32, 64);
            l_run = l_run * alpha + lsum;
            m_run = m_new;
#pragma unroll
            for (int i = 0; i < 16; ++i) { o0[i] *= alpha; o1[i] *= alpha; }
            // ---- O^T += V^T P^T: k-step (sub, st) = keys 32 sub + 16 st + {8 (j >> 2) + 4 lh + (j & 3)}
#pragma unroll
            for (int sub = 0; sub < 2; ++sub)
#pragma unroll
                for (int st = 0; st < 2; ++st) {
                    u32x4 pf;
#pragma unroll
                    for (int w = 0; w < 4; ++w) pf[w] = pack2<BF16>(s[sub][8 * st + 2 * w], s[sub][8 * st + 2 * w + 1]);
                    const int row = 32 * sub + 16 * st + vrow;
#pragma unroll
                    for (int db = 0; db < 2; ++db) {
                        typedef __attribute__((address_space(3))) s16x4* lds_s16x4;
                        const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)(vs16 + row * 64 + vch[db] * 8 + 4 * (p4 & 1)));
                        const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)(vs16 + (row + 8) * 64 + vch[db] * 8 + 4 * (p4 & 1)));
                        const u32x2 l2 = __builtin_bit_cast(u32x2, lo), h2 = __builtin_bit_cast(u32x2, hi);
                        const u32x4 vf = {l2[0], l2[1], h2[0], h2[1]};
                        if (db == 0) o0 = mfma_h<BF16>(vf, pf, o0);
                        else o1 = mfma_h<BF16>(vf, pf, o1);
                    }
                }
        }
        if (nxt < ntiles) store_tile(buf ^ 1, kn);          // the other buffer: last read before the barrier that ended the previous iteration
        __syncthreads();
        t = nxt; buf ^= 1;
    }

    if (wave_active && qi_raw < a.Lq) {
        const float inv = 1.0f / l_run;                     // a fully masked row: 0 * inf (unspecified by contract)
        uint16_t* po = a.out + (long long)b * a.os[0] + (long long)h * a.os[1] + (long long)qi_raw * a.os[2] + 4 * lh;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            u32x2 w0, w1;
            w0[0] = pack2<BF16>(o0[4 * g] * inv, o0[4 * g + 1] * inv); w0[1] = pack2<BF16>(o0[4 * g + 2] * inv, o0[4 * g + 3] * inv);
            w1[0] = pack2<BF16>(o1[4 * g] * inv, o1[4 * g + 1] * inv); w1[1] = pack2<BF16>(o1[4 * g + 2] * inv, o1[4 * g + 3] * inv);
            *reinterpret_cast<u32x2*>(po + 8 * g) = w0;
            *reinterpret_cast<u32x2*>(po + 32 + 8 * g) = w1;
        }
        // both halves of the lane pair hold the same m_run and l_run; a fully masked row writes -inf + log2(0) = -inf
        if (LSE && lh == 0) a.lse[((long long)b * a.H + h) * a.Lq + qi_raw] = (m_run + __builtin_amdgcn_logf(l_run)) * 0.6931471805599453f;
    }
}

bool aligned_strides_f(const long long* s) { return s[0] % 4 == 0 && s[1] % 4 == 0 && s[2] % 4 == 0 && s[0] >= 0 && s[1] >= 0 && s[2] >= 0; }

typedef void (*SdpaHmKernel)(SdpaHmArgs);
template <bool BF16, bool LSE>
SdpaHmKernel sdpa_hm_variant(int kind) {
    switch (kind) {
        case HB_F32: return attention_sdpa_hm_kernel<BF16, HB_F32, LSE>;
        case HB_U8: return attention_sdpa_hm_kernel<BF16, HB_U8, LSE>;
        case HB_HALF: return attention_sdpa_hm_kernel<BF16, HB_HALF, LSE>;
        default: return attention_sdpa_hm_kernel<BF16, HB_NONE, LSE>;
    }
}

}  // namespace

// strides: 12 element strides, (batch, head, token) of q, k, v, out in that order; dtype 1 = fp16, 2 = bf16
int attention_sdpa_h(const void* q, const void* k, const void* v, void* out, const long long* strides, int dtype, int B, int H, int Lq, int Lk, int head_dim, double scale,
                     hipStream_t stream) {
    SDVAR_CHECK_ARG(q && k && v && out && strides, "sdpa_h: null operand");
    SDVAR_CHECK_ARG(dtype == 1 || dtype == 2, "sdpa_h: dtype %d (1 = fp16, 2 = bf16)", dtype);
    SDVAR_CHECK_ARG(head_dim == 64, "sdpa_h: head dim %d (only 64 is built)", head_dim);
    SDVAR_CHECK_ARG(B >= 1 && H >= 1 && Lq >= 1 && Lk >= 1 && B <= 65535 && H <= 65535, "sdpa_h: bad extents B=%d H=%d Lq=%d Lk=%d", B, H, Lq, Lk);
    static const char* const names[4] = {"q", "k", "v", "out"};
    const void* const ptrs[4] = {q, k, v, out};
    for (int i = 0; i < 4; ++i) {
        SDVAR_CHECK_ARG(aligned_strides_h(strides + 3 * i), "sdpa_h: %s strides (%lld, %lld, %lld) - token rows must be 16-byte aligned (every stride a non-negative multiple of 8 elements)",
                        names[i], strides[3 * i], strides[3 * i + 1], strides[3 * i + 2]);
        SDVAR_CHECK_ARG(((uintptr_t)ptrs[i] & 15) == 0, "sdpa_h: %s is not 16-byte aligned", names[i]);
    }
    SdpaHArgs a;
    a.q = (const uint16_t*)q; a.k = (const uint16_t*)k; a.v = (const uint16_t*)v; a.out = (uint16_t*)out;
    for (int i = 0; i < 3; ++i) { a.qs[i] = strides[i]; a.ks[i] = strides[3 + i]; a.vs[i] = strides[6 + i]; a.os[i] = strides[9 + i]; }
    a.B = B; a.H = H; a.Lq = Lq; a.Lk = Lk; a.scale_l2e = (float)(scale * 1.4426950408889634);
    const dim3 grid((Lq + QB - 1) / QB, H, B);
    if (dtype == 2) hipLaunchKernelGGL(attention_sdpa_h_kernel<true>, grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(attention_sdpa_h_kernel<false>, grid, dim3(256), 0, stream, a);
    SDVAR_LAUNCH_CHECK();
    return SDVAR_OK;
}

// strides: 12 element strides, (batch, head, token) of q, k, v, out in that order (q / k in THEIR elements: fp32 where flagged); dtype 1 = fp16, 2 = bf16 (v, out and
// the unflagged operands); bias kind 0 none | 1 fp32 additive | 2 uint8 keep | 3 additive in dtype; bs: (batch, head, query row) element strides, 0 = broadcast
// lse: nullptr = sdvar_op_sdpa_hm; else sdvar_op_sdpa_hm_lse, which also writes the (B, H, Lq) log-sum-exp rows
static int sdpa_hm_launch(const void* q, const void* k, const void* v, void* out, float* lse, const long long* strides, int dtype, int q_f32, int k_f32, const void* bias,
                          int kind, const long long* bs, const uint8_t* skip, int B, int H, int Lq, int Lk, int head_dim, double scale, hipStream_t stream) {
    SDVAR_CHECK_ARG(q && k && v && out && strides, "sdpa_hm: null operand");
    SDVAR_CHECK_ARG(dtype == 1 || dtype == 2, "sdpa_hm: dtype %d (1 = fp16, 2 = bf16)", dtype);
    SDVAR_CHECK_ARG((q_f32 == 0 || q_f32 == 1) && (k_f32 == 0 || k_f32 == 1), "sdpa_hm: q_f32 = %d, k_f32 = %d (0 or 1)", q_f32, k_f32);
    SDVAR_CHECK_ARG(head_dim == 64, "sdpa_hm: head dim %d (only 64 is built)", head_dim);
    SDVAR_CHECK_ARG(B >= 1 && H >= 1 && Lq >= 1 && Lk >= 1 && B <= 65535 && H <= 65535, "sdpa_hm: bad extents B=%d H=%d Lq=%d Lk=%d", B, H, Lq, Lk);
    static const char* const names[4] = {"q", "k", "v", "out"};
    const void* const ptrs[4] = {q, k, v, out};
    const bool f32[4] = {q_f32 != 0, k_f32 != 0, false, false};
    for (int i = 0; i < 4; ++i) {
        if (f32[i])
            SDVAR_CHECK_ARG(aligned_strides_f(strides + 3 * i), "sdpa_hm: fp32 %s strides (%lld, %lld, %lld) - token rows must be 16-byte aligned (every stride a non-negative multiple of 4 floats)",
                            names[i], strides[3 * i], strides[3 * i + 1], strides[3 * i + 2]);
        else
            SDVAR_CHECK_ARG(aligned_strides_h(strides + 3 * i), "sdpa_hm: %s strides (%lld, %lld, %lld) - token rows must be 16-byte aligned (every stride a non-negative multiple of 8 elements)",
                            names[i], strides[3 * i], strides[3 * i + 1], strides[3 * i + 2]);
        SDVAR_CHECK_ARG(((uintptr_t)ptrs[i] & 15) == 0, "sdpa_hm: %s is not 16-byte aligned", names[i]);
    }
    SDVAR_CHECK_ARG(kind >= HB_NONE && kind <= HB_HALF, "sdpa_hm: bias kind %d (0 = none, 1 = fp32 additive, 2 = uint8 keep-mask, 3 = additive in dtype)", kind);
    SDVAR_CHECK_ARG((kind == HB_NONE) == (bias == nullptr), "sdpa_hm: bias pointer and bias kind %d disagree", kind);
    SDVAR_CHECK_ARG(kind == HB_NONE || (bs && bs[0] >= 0 && bs[1] >= 0 && bs[2] >= 0), "sdpa_hm: bias strides missing or negative");
    SDVAR_CHECK_ARG(kind != HB_HALF || ((uintptr_t)bias & 1) == 0, "sdpa_hm: a half bias at an odd address");
    SDVAR_CHECK_ARG(kind != HB_F32 || ((uintptr_t)bias & 3) == 0, "sdpa_hm: an fp32 bias that is not 4-byte aligned");
    SDVAR_CHECK_ARG(kind != HB_NONE || !skip, "sdpa_hm: a skip map needs a bias");
    SdpaHmArgs a;
    a.q = q; a.k = k; a.v = (const uint16_t*)v; a.out = (uint16_t*)out;
    for (int i = 0; i < 3; ++i) { a.qs[i] = strides[i]; a.ks[i] = strides[3 + i]; a.vs[i] = strides[6 + i]; a.os[i] = strides[9 + i]; a.bs[i] = kind ? bs[i] : 0; }
    a.bias = bias; a.skip = skip; a.nkt = (Lk + KT - 1) / KT;
    const uintptr_t balign = kind == HB_F32 ? 15 : kind == HB_U8 ? 3 : 7;
    a.bias_vec = kind != HB_NONE && ((uintptr_t)bias & balign) == 0 && bs[0] % 4 == 0 && bs[1] % 4 == 0 && bs[2] % 4 == 0;
    a.q_f32 = q_f32; a.k_f32 = k_f32;
    a.B = B; a.H = H; a.Lq = Lq; a.Lk = Lk; a.scale_l2e = (float)(scale * 1.4426950408889634);
    const dim3 grid((Lq + QB - 1) / QB, H, B);
    a.lse = lse;
    const SdpaHmKernel kern = lse ? (dtype == 2 ? sdpa_hm_variant<true, true>(kind) : sdpa_hm_variant<false, true>(kind))
                                  : (dtype == 2 ? sdpa_hm_variant<true, false>(kind) : sdpa_hm_variant<false, false>(kind));
    hipLaunchKernelGGL(kern, grid, dim3(256), 0, stream, a);
    SDVAR_LAUNCH_CHECK();
    return SDVAR_OK;
}

int attention_sdpa_hm(const void* q, const void* k, const void* v, void* out, const long long* strides, int dtype, int q_f32, int k_f32, const void* bias, int kind,
                      const long long* bs, const uint8_t* skip, int B, int H, int Lq, int Lk, int head_dim, double scale, hipStream_t stream) {
    return sdpa_hm_launch(q, k, v, out, nullptr, strides, dtype, q_f32, k_f32, bias, kind, bs, skip, B, H, Lq, Lk, head_dim, scale, stream);
}

// attention_sdpa_hm that also writes lse (device, (B, H, Lq) dense fp32); with kind 0 and three half operands `out` has attention_sdpa_h's bits (the same arithmetic:
// no bias, so the running maximum is finite from the first tile on)
int attention_sdpa_hm_lse(const void* q, const void* k, const void* v, void* out, float* lse, const long long* strides, int dtype, int q_f32, int k_f32, const void* bias,
                          int kind, const long long* bs, const uint8_t* skip, int B, int H, int Lq, int Lk, int head_dim, double scale, hipStream_t stream) {
    SDVAR_CHECK_ARG(lse && ((uintptr_t)lse & 3) == 0, "sdpa_hm_lse: lse is NULL or not 4-byte aligned");
    return sdpa_hm_launch(q, k, v, out, lse, strides, dtype, q_f32, k_f32, bias, kind, bs, skip, B, H, Lq, Lk, head_dim, scale, stream);
}

}  // namespace sdvar
