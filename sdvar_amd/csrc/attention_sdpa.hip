// Operator-seam attention: out = softmax(scale q k^T + bias) v for the reference's module-level slots slow_attn / memory_efficient_attention
// (models/basic_var.py:25-30, called at :113-117).  fp32 operands, fp32 arithmetic on the fp32 matrix cores, flash-style (no score
// matrix in HBM).  Same MFMA mapping, LDS layout and double-buffered 64-key K/V staging as attention_f32_kernel (attention.hip); what that kernel
// derives from the stage table comes from the caller here:
//   * q, k, v, out are STRIDED: element strides for (batch, head, token), channel stride 1, head dim 64.  The reference's permuted views of one
//     (B, L, 3, H, 64) buffer, its (B, H, L, 64) concatenated caches and xformers' (B, L, H, 64) tensors are all just strides.  Every token row must
//     be 16-byte aligned (base pointers % 16 == 0, every stride % 4 == 0): rows are moved with 16-byte accesses.
//   * `scale` is an argument (folded into the Q fragment once, in fp32).  Lq and Lk are independent, any value >= 1; K/V rows past Lk are zero-filled
//     in staging and their scores set to -inf.
//   * optional bias: fp32 additive (any finite value or -inf) or a uint8 keep-mask (SDPA's bool semantics: 0 = -inf, else 0), element strides for
//     (batch, head, query row) with 0 = broadcast, key stride 1.  The bias value is the INITIAL accumulator of the score MFMAs, so it costs no
//     extra adds.
//   * skip map (optional, sdpa_skip_map below): one byte per (128-query block, 64-key tile), 1 = every element of the tile is masked for EVERY
//     (batch, head) slice the bias holds.  Such a tile is never staged and never multiplied: the tile loop walks the unmasked tiles only.  The map is
//     built on the device and read on the device: no host round trip.
// Online softmax under -inf: the running maximum of a query may still be -inf after a tile that other queries of the workgroup needed; the
// exponent reference is then 0 instead of the maximum, so that tile contributes exp(-inf) = 0 and never exp(-inf - (-inf)).
// A query row whose keys are ALL masked has no defined softmax: its output is unspecified (0 / 0 here, like torch); it does not fault and does not
// touch other rows (every row lives in its own lanes).
// Every workgroup (128 queries of one batch and head) streams the K and V rows of the tiles it visits once: B*H*ceil(Lq/128) * visited tiles * 32 KiB.
#include "common.h"

#include <type_traits>

namespace sdvar {

namespace {

constexpr int KT = 64;              // keys per LDS tile
constexpr int KSTR = 68;            // padded K row (floats)
constexpr int QB = 128;             // queries per workgroup

enum { BIAS_NONE = 0, BIAS_F32 = 1, BIAS_U8 = 2, BIAS_F16 = 3, BIAS_BF16 = 4 };          // 3, 4: the skip map only (additive half biases of sdvar_op_sdpa_hm)

struct SdpaArgs {
    const float *q, *k, *v; float* out;
    long long qs[3], ks[3], vs[3], os[3];       // element strides: batch, head, token
    const void* bias; long long bs[3];          // element strides: batch, head, query row (0 = broadcast)
    int bias_vec;                               // bias rows allow 4-element vector loads (16 bytes fp32 / 4 bytes uint8)
    const uint8_t* skip; int nkt;               // skip map (ceil(Lq/128), nkt) or nullptr
    int B, H, Lq, Lk;
    float scale;
};
struct SdpaLseArgs : SdpaArgs {
    float* lse;                                 // (B, H, Lq) dense, natural log
};

// LSE: each stored query row also writes lse = m_run + ln(l_run), what the backward (attention_sdpa_bwd.hip) recomputes P from.  A compile-time flag with an
// argument block of its own: the instantiations without it take the arguments they always took and are the kernels they were, instruction for instruction.
template <int BIAS, bool LSE>
__global__ __launch_bounds__(256, 2) void attention_sdpa_kernel(typename std::conditional<LSE, SdpaLseArgs, SdpaArgs>::type a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int STAGE = KT * KSTR + KT * 64;              // floats per pipeline stage: K tile then V tile

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int qt = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int q0 = qt * QB;

    const int qi_raw = q0 + wave * 32 + li;
    const int qi = min(qi_raw, a.Lq - 1);
    const bool wave_active = (q0 + wave * 32) < a.Lq;

    // Q fragment: lane (query li, half lh) holds d = 8c + 4lh + e, c = 0..7, e = 0..3; scale folded in
    f32x4 qf[8];
    {
        const float* pq = a.q + (long long)b * a.qs[0] + (long long)h * a.qs[1] + (long long)qi * a.qs[2] + 4 * lh;
#pragma unroll
        for (int c = 0; c < 8; ++c) qf[c] = *reinterpret_cast<const f32x4*>(pq + 8 * c) * a.scale;
    }
    // this lane's bias row
    const float* brow_f = nullptr; const uint8_t* brow_u = nullptr;
    if (BIAS != BIAS_NONE) {
        const long long off = (long long)b * a.bs[0] + (long long)h * a.bs[1] + (long long)qi * a.bs[2];
        brow_f = reinterpret_cast<const float*>(a.bias) + off; brow_u = reinterpret_cast<const uint8_t*>(a.bias) + off;
    }

    // staging: 64 keys x 64 channels per operand, 4 float4 per thread (key = tid/16 + 16 i, col = 4 (tid%16))
    const float* kbase = a.k + (long long)b * a.ks[0] + (long long)h * a.ks[1];
    const float* vbase = a.v + (long long)b * a.vs[0] + (long long)h * a.vs[1];
    const int skey = tid >> 4, scol = (tid & 15) * 4;
    f32x4 rk[4], rv[4];
    // branch-free (rows past Lk read the last row and are zeroed): the loads always issue, so the compiler can count them (see the tile loop)
    auto load_tile = [&](int k0) {
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int key = k0 + skey + 16 * i, kc = min(key, a.Lk - 1);
            const f32x4 tk = *reinterpret_cast<const f32x4*>(kbase + (long long)kc * a.ks[2] + scol);
            const f32x4 tv = *reinterpret_cast<const f32x4*>(vbase + (long long)kc * a.vs[2] + scol);
            rk[i] = key < a.Lk ? tk : zero; rv[i] = key < a.Lk ? tv : zero;
        }
    };
    auto store_tile = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            *reinterpret_cast<f32x4*>(smem + buf * STAGE + (skey + 16 * i) * KSTR + scol) = rk[i];
            *reinterpret_cast<f32x4*>(smem + buf * STAGE + KT * KSTR + (skey + 16 * i) * 64 + scol) = rv[i];
        }
    };
    // The bias of a tile in two steps, so that its loads are in flight while the K/V prefetch issues and the K fragments are read:
    //   fetch_bias: loads only, raw bits into bq (this lane: keys k0 + sub*32 + 8g + 4lh + e -> bq[4 sub + g][e]).  Two workgroup-uniform paths, both free of
    //               per-lane branches: 8 vector loads (aligned rows, whole tile inside Lk) or 32 clamped element loads.
    //   init_scores: the initial score accumulators = the bias (or 0), -inf past the last key; register 4g + e of sub-tile `sub`.
    auto fetch_bias = [&](int k0, f32x4 (&bq)[8]) {
        if (BIAS == BIAS_NONE) return;
        if (a.bias_vec && k0 + KT <= a.Lk) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int key = k0 + (j >> 2) * 32 + 8 * (j & 3) + 4 * lh;
                if (BIAS == BIAS_F32) bq[j] = *reinterpret_cast<const f32x4*>(brow_f + key);
                else bq[j][0] = __uint_as_float(*reinterpret_cast<const uint32_t*>(brow_u + key));
            }
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int kc = min(k0 + (j >> 2) * 32 + 8 * (j & 3) + 4 * lh + e, a.Lk - 1);
                    bq[j][e] = BIAS == BIAS_F32 ? brow_f[kc] : __uint_as_float((uint32_t)brow_u[kc]);
                }
        }
    };
    auto init_scores = [&](int k0, const f32x4 (&bq)[8], f32x16 (&s)[2]) {
        const bool full = k0 + KT <= a.Lk;
        const bool packed = BIAS == BIAS_U8 && a.bias_vec && full;          // four keep bytes in bq[j][0]
#pragma unroll
        for (int j = 0; j < 8; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float val = 0.f;
                if (BIAS == BIAS_F32) val = bq[j][e];
                if (BIAS == BIAS_U8) val = (packed ? ((__float_as_uint(bq[j][0]) >> (8 * e)) & 0xFFu) : __float_as_uint(bq[j][e])) ? 0.f : -INFINITY;
                const int key = k0 + (j >> 2) * 32 + 8 * (j & 3) + 4 * lh + e;
                s[j >> 2][4 * (j & 3) + e] = (!full && key >= a.Lk) ? -INFINITY : val;
            }
    };

    f32x16 o0, o1;                        // O^T accumulators: d = db*32 + (reg&3) + 8*(reg>>2) + 4*lh, column = this query
#pragma unroll
    for (int i = 0; i < 16; ++i) { o0[i] = 0.f; o1[i] = 0.f; }
    float m_run = -INFINITY, l_run = 0.f;

    // the tiles this workgroup visits: every tile the skip map does not mark (workgroup-uniform walk)
    const int ntiles = (a.Lk + KT - 1) / KT;
    const uint8_t* skip_row = (BIAS != BIAS_NONE && a.skip) ? a.skip + (size_t)qt * a.nkt : nullptr;
    auto next_tile = [&](int t) {
        if (BIAS != BIAS_NONE && skip_row)
            while (t < ntiles && skip_row[t]) ++t;
        return t;
    };

    int t = next_tile(0);
    if (t < ntiles) {
        load_tile(t * KT);
        store_tile(0);
    }
    __syncthreads();
    int buf = 0;
    while (t < ntiles) {
        const int k0 = t * KT;
        const int nxt = next_tile(t + 1);
        f32x16 s[2];
        // The bias loads go out BEFORE the K/V prefetch and the prefetch ALWAYS issues (past the last tile it re-reads the current one and is dropped): the
        // score MFMAs then wait for "all but the 8 newest loads" and the prefetch stays in flight under them (vmcnt counts in order).
        f32x4 bq[8];
        if (wave_active) fetch_bias(k0, bq);
        load_tile((nxt < ntiles ? nxt : t) * KT);
        __builtin_amdgcn_sched_barrier(0);
        if (wave_active) {
            // LDS reads are hand-placed (inline asm + counted lgkmcnt), as in attention_f32_kernel
            typedef __attribute__((address_space(3))) float* lds_f;
            const uint32_t kb = (uint32_t)(uintptr_t)(lds_f)(smem + buf * STAGE) + 4u * (li * KSTR + 4 * lh);
            const uint32_t vb = (uint32_t)(uintptr_t)(lds_f)(smem + buf * STAGE + KT * KSTR) + 4u * (4 * lh * 64 + li);
            // ---- K fragments of both 32-key sub-tiles (16 x b128), then the 64 score MFMAs
            f32x4 kf[2][8];
#define SDVAR_RD128(dst, addr, off) asm volatile("ds_read_b128 %0, %1 offset:" #off : "=v"(dst) : "v"(addr) : "memory")
            SDVAR_RD128(kf[0][0], kb, 0);    SDVAR_RD128(kf[0][1], kb, 32);   SDVAR_RD128(kf[0][2], kb, 64);   SDVAR_RD128(kf[0][3], kb, 96);
            SDVAR_RD128(kf[0][4], kb, 128);  SDVAR_RD128(kf[0][5], kb, 160);  SDVAR_RD128(kf[0][6], kb, 192);  SDVAR_RD128(kf[0][7], kb, 224);
            SDVAR_RD128(kf[1][0], kb, 8704); SDVAR_RD128(kf[1][1], kb, 8736); SDVAR_RD128(kf[1][2], kb, 8768); SDVAR_RD128(kf[1][3], kb, 8800);
            SDVAR_RD128(kf[1][4], kb, 8832); SDVAR_RD128(kf[1][5], kb, 8864); SDVAR_RD128(kf[1][6], kb, 8896); SDVAR_RD128(kf[1][7], kb, 8928);
#undef SDVAR_RD128
            init_scores(k0, bq, s);
#pragma unroll
            for (int sub = 0; sub < 2; ++sub) {
                if (sub == 0) asm volatile("s_waitcnt lgkmcnt(8)" ::: "memory");
                else asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int c = 0; c < 8; ++c)
#pragma unroll
                    for (int e = 0; e < 4; ++e) s[sub] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[sub][c][e], qf[c][e], s[sub], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
            // ---- V operands of the whole tile: 32 x ds_read2st64_b32 (two key rows, 256 B apart, per instruction), issued
            // before the softmax arithmetic so their latency hides under it.  vf[db][sub][i] = V[key(sub, i, lh)][32 db + li].
            typedef float f32x2 __attribute__((ext_vector_type(2)));
            f32x2 vf[2][2][8];
#define SDVAR_RDV(dst, addr, r0, r1) asm volatile("ds_read2st64_b32 %0, %1 offset0:" #r0 " offset1:" #r1 : "=v"(dst) : "v"(addr) : "memory")
#define SDVAR_RDV_SUB(db, sub, base)                                                                                      \
            SDVAR_RDV(vf[db][sub][0], vb + 128u * db, base + 0, base + 1);   SDVAR_RDV(vf[db][sub][1], vb + 128u * db, base + 2, base + 3);   \
            SDVAR_RDV(vf[db][sub][2], vb + 128u * db, base + 8, base + 9);   SDVAR_RDV(vf[db][sub][3], vb + 128u * db, base + 10, base + 11); \
            SDVAR_RDV(vf[db][sub][4], vb + 128u * db, base + 16, base + 17); SDVAR_RDV(vf[db][sub][5], vb + 128u * db, base + 18, base + 19); \
            SDVAR_RDV(vf[db][sub][6], vb + 128u * db, base + 24, base + 25); SDVAR_RDV(vf[db][sub][7], vb + 128u * db, base + 26, base + 27);
            SDVAR_RDV_SUB(0, 0, 0) SDVAR_RDV_SUB(1, 0, 0) SDVAR_RDV_SUB(0, 1, 32) SDVAR_RDV_SUB(1, 1, 32)
#undef SDVAR_RDV_SUB
#undef SDVAR_RDV
            // ---- online softmax (this lane: one query, keys k0 + sub*32 + (i&3) + 8*(i>>2) + 4*lh)
            float mloc = -INFINITY;
#pragma unroll
            for (int sub = 0; sub < 2; ++sub)
#pragma unroll
                for (int i = 0; i < 16; ++i) mloc = fmaxf(mloc, s[sub][i]);
            mloc = fmaxf(mloc, __shfl_xor(mloc, 32, 64));
            const float m_new = fmaxf(m_run, mloc);
            // every key so far masked for this query: exponent reference 0, so this tile's weights are exp(-inf) = 0 and alpha = exp(-inf) = 0
            const float m_ref = (m_new == -INFINITY) ? 0.f : m_new;
            const float L2E = 1.4426950408889634f;
            const float alpha = __builtin_amdgcn_exp2f((m_run - m_ref) * L2E);
            float lsum = 0.f;
#pragma unroll
            for (int sub = 0; sub < 2; ++sub)
#pragma unroll
                for (int i = 0; i < 16; ++i) { s[sub][i] = __builtin_amdgcn_exp2f((s[sub][i] - m_ref) * L2E); lsum += s[sub][i]; }
            lsum += __shfl_xor(lsum, 32, 64);
            l_run = l_run * alpha + lsum;
            m_run = m_new;
#pragma unroll
            for (int i = 0; i < 16; ++i) { o0[i] *= alpha; o1[i] *= alpha; }
            // ---- O^T += V^T P^T : step i pairs key (i&3)+8*(i>>2) (half 0) with the same +4 (half 1)
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int sub = 0; sub < 2; ++sub) {
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int slot = 2 * (i >> 2) + ((i & 3) >> 1), half = i & 1;
                    o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(vf[0][sub][slot][half], s[sub][i], o0, 0, 0, 0);
                    o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(vf[1][sub][slot][half], s[sub][i], o1, 0, 0, 0);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        if (nxt < ntiles) store_tile(buf ^ 1);
        __syncthreads();
        t = nxt; buf ^= 1;
    }

    if (wave_active && qi_raw < a.Lq) {
        const float inv = 1.0f / l_run;             // a fully masked row: 0 * inf (unspecified by contract)
        float* po = a.out + (long long)b * a.os[0] + (long long)h * a.os[1] + (long long)qi_raw * a.os[2] + 4 * lh;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            f32x4 v0, v1;
#pragma unroll
            for (int e = 0; e < 4; ++e) { v0[e] = o0[4 * g + e] * inv; v1[e] = o1[4 * g + e] * inv; }
            *reinterpret_cast<f32x4*>(po + 8 * g) = v0;
            *reinterpret_cast<f32x4*>(po + 32 + 8 * g) = v1;
        }
        if constexpr (LSE) {
            if (lh == 0) a.lse[((long long)b * a.H + h) * a.Lq + qi_raw] = m_run + logf(l_run);          // both halves of a query hold the same m_run, l_run
        }
    }
}

// map[qb * nkt + kt] = 1 when bias[bb][hh][128 qb .. ][64 kt ..] is masked (-inf / keep == 0) for every (bb, hh) of the bias's own extent.
// One workgroup per tile; a thread stops reading at its first visible element.
template <int BIAS>
__global__ __launch_bounds__(256) void sdpa_skip_map_kernel(const void* bias, long long sb, long long sh, long long sr, int Bb, int Hb, int Lq, int Lk,
                                                            uint8_t* map, int nkt) {
    const int kt = blockIdx.x, qb = blockIdx.y;
    const int rows = min(QB, Lq - qb * QB), keys = min(KT, Lk - kt * KT);
    const long long items = (long long)Bb * Hb * rows * KT;
    int visible = 0;
    for (long long it = threadIdx.x; it < items && !visible; it += 256) {
        const int key = (int)(it & (KT - 1));
        const long long rr = it >> 6;
        const int row = (int)(rr % rows);
        const long long bh = rr / rows;
        const int hh = (int)(bh % Hb), bb = (int)(bh / Hb);
        if (key >= keys) continue;
        const long long off = bb * sb + hh * sh + (long long)(qb * QB + row) * sr + kt * KT + key;
        if (BIAS == BIAS_F32) visible = reinterpret_cast<const float*>(bias)[off] != -INFINITY;
        else if (BIAS == BIAS_F16) visible = reinterpret_cast<const uint16_t*>(bias)[off] != 0xFC00u;         // -inf in fp16
        else if (BIAS == BIAS_BF16) visible = reinterpret_cast<const uint16_t*>(bias)[off] != 0xFF80u;        // -inf in bf16
        else visible = reinterpret_cast<const uint8_t*>(bias)[off] != 0;
    }
    const int any = __syncthreads_or(visible);
    if (threadIdx.x == 0) map[(size_t)qb * nkt + kt] = any ? 0 : 1;
}

bool aligned_strides(const long long* s) { return s[0] % 4 == 0 && s[1] % 4 == 0 && s[2] % 4 == 0 && s[0] >= 0 && s[1] >= 0 && s[2] >= 0; }

}  // namespace

int sdpa_skip_map(const void* bias, int kind, const long long* bs, int Bb, int Hb, int Lq, int Lk, uint8_t* map, hipStream_t stream) {
    SDVAR_CHECK_ARG(bias && bs && map, "sdpa_skip_map: null operand");
    SDVAR_CHECK_ARG(kind >= BIAS_F32 && kind <= BIAS_BF16, "sdpa_skip_map: bias kind %d (1 = fp32 additive, 2 = uint8 keep-mask, 3 = fp16 additive, 4 = bf16 additive)", kind);
    SDVAR_CHECK_ARG(Bb >= 1 && Hb >= 1 && Lq >= 1 && Lk >= 1, "sdpa_skip_map: bad extents Bb=%d Hb=%d Lq=%d Lk=%d", Bb, Hb, Lq, Lk);
    SDVAR_CHECK_ARG(bs[0] >= 0 && bs[1] >= 0 && bs[2] >= 0, "sdpa_skip_map: negative bias stride");
    const int nkt = (Lk + KT - 1) / KT, nqb = (Lq + QB - 1) / QB;
    SDVAR_CHECK_ARG(nqb <= 65535, "sdpa_skip_map: Lq=%d too long", Lq);
    if (kind == BIAS_F32) hipLaunchKernelGGL(sdpa_skip_map_kernel<BIAS_F32>, dim3(nkt, nqb), dim3(256), 0, stream, bias, bs[0], bs[1], bs[2], Bb, Hb, Lq, Lk, map, nkt);
    else if (kind == BIAS_F16) hipLaunchKernelGGL(sdpa_skip_map_kernel<BIAS_F16>, dim3(nkt, nqb), dim3(256), 0, stream, bias, bs[0], bs[1], bs[2], Bb, Hb, Lq, Lk, map, nkt);
    else if (kind == BIAS_BF16) hipLaunchKernelGGL(sdpa_skip_map_kernel<BIAS_BF16>, dim3(nkt, nqb), dim3(256), 0, stream, bias, bs[0], bs[1], bs[2], Bb, Hb, Lq, Lk, map, nkt);
    else hipLaunchKernelGGL(sdpa_skip_map_kernel<BIAS_U8>, dim3(nkt, nqb), dim3(256), 0, stream, bias, bs[0], bs[1], bs[2], Bb, Hb, Lq, Lk, map, nkt);
    SDVAR_LAUNCH_CHECK();
    return SDVAR_OK;
}

// strides: 12 element strides, (batch, head, token) of q, k, v, out in that order.  want_lse: the sdvar_op_sdpa_lse entry (lse must then be given).
static int attention_sdpa_impl(const float* q, const float* k, const float* v, float* out, const long long* strides, const void* bias, int kind, const long long* bs,
                               const uint8_t* skip, int B, int H, int Lq, int Lk, int head_dim, float scale, bool want_lse, float* lse, hipStream_t stream) {
    SDVAR_CHECK_ARG(q && k && v && out && strides, "sdpa: null operand");
    SDVAR_CHECK_ARG(!want_lse || lse, "sdpa: null lse");
    SDVAR_CHECK_ARG(!want_lse || ((uintptr_t)lse & 3) == 0, "sdpa: lse is not 4-byte aligned");
    SDVAR_CHECK_ARG(head_dim == 64, "sdpa: head dim %d (only 64 is built)", head_dim);
    SDVAR_CHECK_ARG(B >= 1 && H >= 1 && Lq >= 1 && Lk >= 1 && B <= 65535 && H <= 65535, "sdpa: bad extents B=%d H=%d Lq=%d Lk=%d", B, H, Lq, Lk);
    static const char* const names[4] = {"q", "k", "v", "out"};
    const void* const ptrs[4] = {q, k, v, out};
    for (int i = 0; i < 4; ++i) {
        SDVAR_CHECK_ARG(aligned_strides(strides + 3 * i), "sdpa: %s strides (%lld, %lld, %lld) - token rows must be 16-byte aligned (every stride a non-negative multiple of 4 floats)",
                        names[i], strides[3 * i], strides[3 * i + 1], strides[3 * i + 2]);
        SDVAR_CHECK_ARG(((uintptr_t)ptrs[i] & 15) == 0, "sdpa: %s is not 16-byte aligned", names[i]);
    }
    SDVAR_CHECK_ARG(kind >= BIAS_NONE && kind <= BIAS_U8, "sdpa: bias kind %d (0 = none, 1 = fp32 additive, 2 = uint8 keep-mask)", kind);
    SDVAR_CHECK_ARG((kind == BIAS_NONE) == (bias == nullptr), "sdpa: bias pointer and bias kind %d disagree", kind);
    SDVAR_CHECK_ARG(kind == BIAS_NONE || (bs && bs[0] >= 0 && bs[1] >= 0 && bs[2] >= 0), "sdpa: bias strides missing or negative");
    SDVAR_CHECK_ARG(kind != BIAS_NONE || !skip, "sdpa: a skip map needs a bias");
    SdpaLseArgs a;
    a.q = q; a.k = k; a.v = v; a.out = out;
    for (int i = 0; i < 3; ++i) { a.qs[i] = strides[i]; a.ks[i] = strides[3 + i]; a.vs[i] = strides[6 + i]; a.os[i] = strides[9 + i]; a.bs[i] = kind ? bs[i] : 0; }
    a.bias = bias; a.skip = skip; a.nkt = (Lk + KT - 1) / KT;
    const uintptr_t balign = kind == BIAS_F32 ? 15 : 3;
    a.bias_vec = kind != BIAS_NONE && ((uintptr_t)bias & balign) == 0 && bs[0] % 4 == 0 && bs[1] % 4 == 0 && bs[2] % 4 == 0;
    a.B = B; a.H = H; a.Lq = Lq; a.Lk = Lk; a.scale = scale; a.lse = want_lse ? lse : nullptr;
    const size_t lds = 2 * (size_t)(KT * KSTR + KT * 64) * sizeof(float);
    const dim3 grid((Lq + QB - 1) / QB, H, B);
    if (want_lse) {
        static LdsOptIn opt_in_lse;
        SDVAR_LDS_OPT_IN(opt_in_lse, lds, (const void*)attention_sdpa_kernel<BIAS_NONE, true>, (const void*)attention_sdpa_kernel<BIAS_F32, true>,
                         (const void*)attention_sdpa_kernel<BIAS_U8, true>);
        if (kind == BIAS_F32) hipLaunchKernelGGL((attention_sdpa_kernel<BIAS_F32, true>), grid, dim3(256), lds, stream, a);
        else if (kind == BIAS_U8) hipLaunchKernelGGL((attention_sdpa_kernel<BIAS_U8, true>), grid, dim3(256), lds, stream, a);
        else hipLaunchKernelGGL((attention_sdpa_kernel<BIAS_NONE, true>), grid, dim3(256), lds, stream, a);
        SDVAR_LAUNCH_CHECK();
        return SDVAR_OK;
    }
    const SdpaArgs& p = a;
    static LdsOptIn opt_in;
    SDVAR_LDS_OPT_IN(opt_in, lds, (const void*)attention_sdpa_kernel<BIAS_NONE, false>, (const void*)attention_sdpa_kernel<BIAS_F32, false>,
                     (const void*)attention_sdpa_kernel<BIAS_U8, false>);
    if (kind == BIAS_F32) hipLaunchKernelGGL((attention_sdpa_kernel<BIAS_F32, false>), grid, dim3(256), lds, stream, p);
    else if (kind == BIAS_U8) hipLaunchKernelGGL((attention_sdpa_kernel<BIAS_U8, false>), grid, dim3(256), lds, stream, p);
    else hipLaunchKernelGGL((attention_sdpa_kernel<BIAS_NONE, false>), grid, dim3(256), lds, stream, p);
    SDVAR_LAUNCH_CHECK();
    return SDVAR_OK;
}

int attention_sdpa(const float* q, const float* k, const float* v, float* out, const long long* strides, const void* bias, int kind, const long long* bs,
                   const uint8_t* skip, int B, int H, int Lq, int Lk, int head_dim, float scale, hipStream_t stream) {
    return attention_sdpa_impl(q, k, v, out, strides, bias, kind, bs, skip, B, H, Lq, Lk, head_dim, scale, false, nullptr, stream);
}

int attention_sdpa_lse(const float* q, const float* k, const float* v, float* out, float* lse, const long long* strides, const void* bias, int kind, const long long* bs,
                       const uint8_t* skip, int B, int H, int Lq, int Lk, int head_dim, float scale, hipStream_t stream) {
    return attention_sdpa_impl(q, k, v, out, strides, bias, kind, bs, skip, B, H, Lq, Lk, head_dim, scale, true, lse, stream);
}

}  // namespace sdvar
