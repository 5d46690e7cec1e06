// Backward of the operator-seam attention (attention_sdpa.hip): given out = softmax(scale q k^T + bias) v, its log-sum-exp rows and dout,
//     P = exp(scale q k^T + bias - lse),  D_i = sum_d dO_id O_id,  dV = P^T dO,  dP = dO V^T,  dS = P o (dP - D),  dQ = scale dS K,  dK = scale dS^T Q
// (the reference trains through slow_attn at models/basic_var.py:117 under the block-causal mask of models/var.py:108-113).  fp32 operands, fp32 arithmetic on
// v_mfma_f32_32x32x2f32, head dim 64, every tensor strided as in the forward (element strides for batch, head, token; channel stride 1; rows 16-byte aligned), the same
// bias kinds and the same skip map.  No score-sized matrix ever reaches memory, no atomics: every output element is reduced in one lane in a fixed order, so repeats
// are bit-identical.  Three launches:
//   sdpa_bwd_delta_kernel  D (B, H, Lq) from out and dout: 16 lanes per row.
//   sdpa_bwd_dkdv_kernel   one workgroup per (128-key block, head, batch), one wave per 32 keys: a lane keeps the K row (scaled) and V row of ITS key in registers as MFMA
//                          B operands; the Q / dO rows stream through LDS 64 queries at a time (double-buffered, with their lse and D).  It is the forward's loop with
//                          the roles of queries and keys exchanged: S = Q K^T and dP = dO V^T land as [query][key = lane], dV^T += dO^T P and dK^T += Q^T dS accumulate
//                          as [channel][key = lane] and are stored once.  A 128-key block is two 64-key columns of the skip map: the workgroup walks the 128-query
//                          blocks that either column needs, and a wave computes only where its own column's byte is 0.
//   sdpa_bwd_dq_kernel     one workgroup per (128-query block, head, batch), one wave per 32 queries, the forward's walk over the unmasked 64-key tiles with K and V
//                          double-buffered in LDS: S^T = K Q^T and dP^T = V dO^T as [key][query = lane], dQ^T += K^T dS^T as [channel][query = lane].
// Skipped tiles have P = 0 exactly (every bias entry is -inf), so skipping them changes no bit.  A -inf bias entry inside a visited tile gives P = exp(-inf) = 0
// and dS = 0 * (finite) = 0.  Query rows past Lq of the last chunk enter the dK/dV reduction with score -inf, dO = 0, lse = 0, D = 0: P = dS = 0.
// A query row whose keys are ALL masked has no defined lse and no defined gradient (as in the forward).
#include "common.h"

namespace sdvar {

namespace {

constexpr int KT = 64;              // rows per LDS tile (keys in the dQ kernel, queries in the dK/dV kernel)
constexpr int KSTR = 68;            // padded row (floats): row fragments are read 16 bytes per lane, columns 4 bytes per lane
constexpr int QB = 128;             // queries per skip-map row / per dQ workgroup
constexpr int KB = 128;             // keys per dK/dV workgroup (two skip-map columns)
constexpr int TILE = KT * KSTR;
constexpr float L2E = 1.4426950408889634f;

enum { BIAS_NONE = 0, BIAS_F32 = 1, BIAS_U8 = 2 };

struct SdpaBwdArgs {
    const float *q, *k, *v, *out, *dout, *lse;
    float *delta, *dq, *dk, *dv;
    long long qs[3], ks[3], vs[3], os[3], gs[3], dqs[3], dks[3], dvs[3];          // element strides: batch, head, token (gs: dout)
    const void* bias; long long bs[3];          // element strides: batch, head, query row (0 = broadcast)
    int bias_vec;                               // bias rows allow 4-element vector loads along the keys
    const uint8_t* skip; int nkt;               // skip map (ceil(Lq/128), nkt) or nullptr
    int B, H, Lq, Lk;
    float scale;
};

// register r of an MFMA result block is row (r & 3) + 8 (r >> 2) + 4 * (lane >> 5)
__device__ __forceinline__ int mrow(int r, int lh) { return (r & 3) + 8 * (r >> 2) + 4 * lh; }

template <int BIAS>
__device__ __forceinline__ float bias_value(const void* bias, long long off) {
    if (BIAS == BIAS_F32) return reinterpret_cast<const float*>(bias)[off];
    if (BIAS == BIAS_U8) return reinterpret_cast<const uint8_t*>(bias)[off] ? 0.f : -INFINITY;
    return 0.f;
}

// D[b][h][i] = sum_d dout[b][h][i][d] * out[b][h][i][d]; 16 lanes per row (one float4 of each operand per lane), 16 rows per workgroup
__global__ __launch_bounds__(256) void sdpa_bwd_delta_kernel(SdpaBwdArgs a) {
    const long long rows = (long long)a.B * a.H * a.Lq;
    const long long row = (long long)blockIdx.x * 16 + (threadIdx.x >> 4);
    const long long rc = row < rows ? row : rows - 1;
    const int i = (int)(rc % a.Lq);
    const long long bh = rc / a.Lq;
    const int h = (int)(bh % a.H), b = (int)(bh / a.H);
    const int col = (threadIdx.x & 15) * 4;
    const f32x4 o = *reinterpret_cast<const f32x4*>(a.out + (long long)b * a.os[0] + (long long)h * a.os[1] + (long long)i * a.os[2] + col);
    const f32x4 g = *reinterpret_cast<const f32x4*>(a.dout + (long long)b * a.gs[0] + (long long)h * a.gs[1] + (long long)i * a.gs[2] + col);
    float s = (o[0] * g[0] + o[1] * g[1]) + (o[2] * g[2] + o[3] * g[3]);
#pragma unroll
    for (int m = 8; m > 0; m >>= 1) s += __shfl_xor(s, m, 64);
    if (row < rows && (threadIdx.x & 15) == 0) a.delta[row] = s;
}

// ---- dK, dV ----------------------------------------------------------------------------------------------------------------------------------------------
template <int BIAS>
__global__ __launch_bounds__(256, 2) void sdpa_bwd_dkdv_kernel(SdpaBwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int STAGE = 2 * TILE + 2 * KT;                // floats per pipeline stage: Q tile, dO tile, 64 lse, 64 D

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int kb = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int key_raw = kb * KB + wave * 32 + li;
    const int key = min(key_raw, a.Lk - 1);
    const bool wave_active = (kb * KB + wave * 32) < a.Lk;
    const int my_kt = 2 * kb + (wave >> 1);                 // this wave's skip-map column

    // resident fragments of this lane's key: channels 8c + 4lh + e; the scale is folded into K (S = scale q k^T)
    f32x4 kf[8], vf[8];
    {
        const float* pk = a.k + (long long)b * a.ks[0] + (long long)h * a.ks[1] + (long long)key * a.ks[2] + 4 * lh;
        const float* pv = a.v + (long long)b * a.vs[0] + (long long)h * a.vs[1] + (long long)key * a.vs[2] + 4 * lh;
#pragma unroll
        for (int c = 0; c < 8; ++c) { kf[c] = *reinterpret_cast<const f32x4*>(pk + 8 * c) * a.scale; vf[c] = *reinterpret_cast<const f32x4*>(pv + 8 * c); }
    }
    const long long boff = BIAS != BIAS_NONE ? (long long)b * a.bs[0] + (long long)h * a.bs[1] + key : 0;

    // staging: 64 queries x 64 channels per operand, 4 float4 per thread (row = tid/16 + 16 i, col = 4 (tid%16)); lse by threads 0..63, D by threads 64..127
    const float* qbase = a.q + (long long)b * a.qs[0] + (long long)h * a.qs[1];
    const float* gbase = a.dout + (long long)b * a.gs[0] + (long long)h * a.gs[1];
    const float* lbase = (tid < KT ? a.lse : a.delta) + ((long long)b * a.H + h) * a.Lq;
    const int srow = tid >> 4, scol = (tid & 15) * 4;
    f32x4 rq[4], rg[4];
    float rl = 0.f;
    auto load_tile = [&](int q0) {
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = q0 + srow + 16 * i, rc = min(r, a.Lq - 1);
            const f32x4 tq = *reinterpret_cast<const f32x4*>(qbase + (long long)rc * a.qs[2] + scol);
            const f32x4 tg = *reinterpret_cast<const f32x4*>(gbase + (long long)rc * a.gs[2] + scol);
            rq[i] = r < a.Lq ? tq : zero; rg[i] = r < a.Lq ? tg : zero;
        }
        if (tid < 2 * KT) {
            const int r = q0 + (tid & (KT - 1));
            const float t = lbase[min(r, a.Lq - 1)];
            rl = r < a.Lq ? t : 0.f;
        }
    };
    auto store_tile = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            *reinterpret_cast<f32x4*>(smem + buf * STAGE + (srow + 16 * i) * KSTR + scol) = rq[i];
            *reinterpret_cast<f32x4*>(smem + buf * STAGE + TILE + (srow + 16 * i) * KSTR + scol) = rg[i];
        }
        if (tid < 2 * KT) smem[buf * STAGE + 2 * TILE + tid] = rl;
    };

    f32x16 dk0, dk1, dv0, dv1;            // dK^T / dV^T accumulators: channel = db*32 + mrow(reg), column = this key
#pragma unroll
    for (int i = 0; i < 16; ++i) { dk0[i] = 0.f; dk1[i] = 0.f; dv0[i] = 0.f; dv1[i] = 0.f; }

    // the 64-query chunks this workgroup visits: both halves of every 128-query block that one of its two skip-map columns needs
    const int nch = (a.Lq + KT - 1) / KT;
    const bool mapped = BIAS != BIAS_NONE && a.skip != nullptr;
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
        store_tile(0);
    }
    __syncthreads();
    int buf = 0;
    while (ch < nch) {
        const int q0 = ch * KT;
        const int nxt = next_chunk(ch + 1);
        load_tile((nxt < nch ? nxt : ch) * KT);             // always issues; dropped past the last chunk
        const bool mine = wave_active && !(mapped && my_kt < a.nkt && a.skip[(size_t)(ch >> 1) * a.nkt + my_kt]);
        if (mine) {
            const float* Qt = smem + buf * STAGE;
            const float* Gt = Qt + TILE;
            const float* Lt = Qt + 2 * TILE;
#pragma unroll
            for (int sub = 0; sub < 2; ++sub) {
                // S[query mrow(r)][this key]: the bias is the initial accumulator, -inf for rows past Lq
                f32x16 s, dp;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int qr = q0 + sub * 32 + mrow(r, lh);
                    const float bv = BIAS != BIAS_NONE ? bias_value<BIAS>(a.bias, boff + (long long)min(qr, a.Lq - 1) * a.bs[2]) : 0.f;
                    s[r] = qr < a.Lq ? bv : -INFINITY;
                    dp[r] = 0.f;
                }
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    const f32x4 aq = *reinterpret_cast<const f32x4*>(Qt + (sub * 32 + li) * KSTR + 8 * c + 4 * lh);
                    const f32x4 ag = *reinterpret_cast<const f32x4*>(Gt + (sub * 32 + li) * KSTR + 8 * c + 4 * lh);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        s = __builtin_amdgcn_mfma_f32_32x32x2f32(aq[e], kf[c][e], s, 0, 0, 0);
                        dp = __builtin_amdgcn_mfma_f32_32x32x2f32(ag[e], vf[c][e], dp, 0, 0, 0);
                    }
                }
                // P = exp(S - lse), dS = P (dP - D); then dV^T += dO^T P, dK^T += Q^T dS: step r pairs query mrow(r, 0) (half 0) with mrow(r, 1) (half 1)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = sub * 32 + mrow(r, lh);
                    const float p = __builtin_amdgcn_exp2f((s[r] - Lt[row]) * L2E);
                    const float ds = p * (dp[r] - Lt[KT + row]);
                    const float g0 = Gt[row * KSTR + li], g1 = Gt[row * KSTR + 32 + li];
                    const float x0 = Qt[row * KSTR + li], x1 = Qt[row * KSTR + 32 + li];
                    dv0 = __builtin_amdgcn_mfma_f32_32x32x2f32(g0, p, dv0, 0, 0, 0);
                    dv1 = __builtin_amdgcn_mfma_f32_32x32x2f32(g1, p, dv1, 0, 0, 0);
                    dk0 = __builtin_amdgcn_mfma_f32_32x32x2f32(x0, ds, dk0, 0, 0, 0);
                    dk1 = __builtin_amdgcn_mfma_f32_32x32x2f32(x1, ds, dk1, 0, 0, 0);
                }
            }
        }
        if (nxt < nch) store_tile(buf ^ 1);
        __syncthreads();
        ch = nxt; buf ^= 1;
    }

    if (wave_active && key_raw < a.Lk) {
        auto store = [&](float* base, const long long* st, const f32x16& x0, const f32x16& x1, float mul) {
            float* po = base + (long long)b * st[0] + (long long)h * st[1] + (long long)key_raw * st[2] + 4 * lh;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                f32x4 v0, v1;
#pragma unroll
                for (int e = 0; e < 4; ++e) { v0[e] = x0[4 * g + e] * mul; v1[e] = x1[4 * g + e] * mul; }
                *reinterpret_cast<f32x4*>(po + 8 * g) = v0;
                *reinterpret_cast<f32x4*>(po + 32 + 8 * g) = v1;
            }
        };
        if (a.dk) store(a.dk, a.dks, dk0, dk1, a.scale);
        if (a.dv) store(a.dv, a.dvs, dv0, dv1, 1.0f);
    }
}

// ---- dQ --------------------------------------------------------------------------------------------------------------------------------------------------
template <int BIAS>
__global__ __launch_bounds__(256, 2) void sdpa_bwd_dq_kernel(SdpaBwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int STAGE = 2 * TILE;                         // floats per pipeline stage: K tile then V tile (both with padded rows)

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int qt = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int q0 = qt * QB;
    const int qi_raw = q0 + wave * 32 + li;
    const int qi = min(qi_raw, a.Lq - 1);
    const bool wave_active = (q0 + wave * 32) < a.Lq;

    // Q (scale folded in) and dO fragments of this lane's query: channels 8c + 4lh + e
    f32x4 qf[8], gf[8];
    {
        const float* pq = a.q + (long long)b * a.qs[0] + (long long)h * a.qs[1] + (long long)qi * a.qs[2] + 4 * lh;
        const float* pg = a.dout + (long long)b * a.gs[0] + (long long)h * a.gs[1] + (long long)qi * a.gs[2] + 4 * lh;
#pragma unroll
        for (int c = 0; c < 8; ++c) { qf[c] = *reinterpret_cast<const f32x4*>(pq + 8 * c) * a.scale; gf[c] = *reinterpret_cast<const f32x4*>(pg + 8 * c); }
    }
    const long long rowid = ((long long)b * a.H + h) * a.Lq + qi;
    const float lse = a.lse[rowid], dlt = a.delta[rowid];
    const float* brow_f = nullptr; const uint8_t* brow_u = nullptr;
    if (BIAS != BIAS_NONE) {
        const long long off = (long long)b * a.bs[0] + (long long)h * a.bs[1] + (long long)qi * a.bs[2];
        brow_f = reinterpret_cast<const float*>(a.bias) + off; brow_u = reinterpret_cast<const uint8_t*>(a.bias) + off;
    }

    const float* kbase = a.k + (long long)b * a.ks[0] + (long long)h * a.ks[1];
    const float* vbase = a.v + (long long)b * a.vs[0] + (long long)h * a.vs[1];
    const int skey = tid >> 4, scol = (tid & 15) * 4;
    f32x4 rk[4], rv[4];
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
            *reinterpret_cast<f32x4*>(smem + buf * STAGE + TILE + (skey + 16 * i) * KSTR + scol) = rv[i];
        }
    };
    // initial score accumulators of one 32-key sub-tile = the bias (or 0), -inf past the last key; register 4g + e holds key k0 + 8g + 4lh + e
    auto init_scores = [&](int k0, f32x16& s) {
        const bool full = k0 + 32 <= a.Lk;
        if (BIAS != BIAS_NONE && a.bias_vec && full) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int key = k0 + 8 * g + 4 * lh;
                if (BIAS == BIAS_F32) {
                    const f32x4 t = *reinterpret_cast<const f32x4*>(brow_f + key);
#pragma unroll
                    for (int e = 0; e < 4; ++e) s[4 * g + e] = t[e];
                } else {
                    const uint32_t t = *reinterpret_cast<const uint32_t*>(brow_u + key);
#pragma unroll
                    for (int e = 0; e < 4; ++e) s[4 * g + e] = ((t >> (8 * e)) & 0xFFu) ? 0.f : -INFINITY;
                }
            }
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = k0 + mrow(r, lh), kc = min(key, a.Lk - 1);
                float val = 0.f;
                if (BIAS == BIAS_F32) val = brow_f[kc];
                if (BIAS == BIAS_U8) val = brow_u[kc] ? 0.f : -INFINITY;
                s[r] = key < a.Lk ? val : -INFINITY;
            }
        }
    };

    f32x16 dq0, dq1;                      // dQ^T accumulators: channel = db*32 + mrow(reg), column = this query
#pragma unroll
    for (int i = 0; i < 16; ++i) { dq0[i] = 0.f; dq1[i] = 0.f; }

    // the tiles this workgroup visits: the forward's walk
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
        load_tile((nxt < ntiles ? nxt : t) * KT);           // always issues; dropped past the last tile
        if (wave_active) {
            const float* Kt = smem + buf * STAGE;
            const float* Vt = Kt + TILE;
#pragma unroll
            for (int sub = 0; sub < 2; ++sub) {
                f32x16 s, dp;
                init_scores(k0 + sub * 32, s);
#pragma unroll
                for (int r = 0; r < 16; ++r) dp[r] = 0.f;
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    const f32x4 ak = *reinterpret_cast<const f32x4*>(Kt + (sub * 32 + li) * KSTR + 8 * c + 4 * lh);
                    const f32x4 av = *reinterpret_cast<const f32x4*>(Vt + (sub * 32 + li) * KSTR + 8 * c + 4 * lh);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        s = __builtin_amdgcn_mfma_f32_32x32x2f32(ak[e], qf[c][e], s, 0, 0, 0);
                        dp = __builtin_amdgcn_mfma_f32_32x32x2f32(av[e], gf[c][e], dp, 0, 0, 0);
                    }
                }
                // dQ^T += K^T dS^T: step r pairs key mrow(r, 0) (half 0) with mrow(r, 1) (half 1)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = sub * 32 + mrow(r, lh);
                    const float p = __builtin_amdgcn_exp2f((s[r] - lse) * L2E);
                    const float ds = p * (dp[r] - dlt);
                    const float x0 = Kt[row * KSTR + li], x1 = Kt[row * KSTR + 32 + li];
                    dq0 = __builtin_amdgcn_mfma_f32_32x32x2f32(x0, ds, dq0, 0, 0, 0);
                    dq1 = __builtin_amdgcn_mfma_f32_32x32x2f32(x1, ds, dq1, 0, 0, 0);
                }
            }
        }
        if (nxt < ntiles) store_tile(buf ^ 1);
        __syncthreads();
        t = nxt; buf ^= 1;
    }

    if (wave_active && qi_raw < a.Lq) {
        float* po = a.dq + (long long)b * a.dqs[0] + (long long)h * a.dqs[1] + (long long)qi_raw * a.dqs[2] + 4 * lh;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            f32x4 v0, v1;
#pragma unroll
            for (int e = 0; e < 4; ++e) { v0[e] = dq0[4 * g + e] * a.scale; v1[e] = dq1[4 * g + e] * a.scale; }
            *reinterpret_cast<f32x4*>(po + 8 * g) = v0;
            *reinterpret_cast<f32x4*>(po + 32 + 8 * g) = v1;
        }
    }
}

bool aligned_strides(const long long* s) { return s[0] % 4 == 0 && s[1] % 4 == 0 && s[2] % 4 == 0 && s[0] >= 0 && s[1] >= 0 && s[2] >= 0; }

}  // namespace

// strides: 24 element strides, (batch, head, token) of q, k, v, out, dout, dq, dk, dv in that order; delta: workspace of B*H*Lq floats
int attention_sdpa_bwd(const float* q, const float* k, const float* v, const float* out, const float* dout, const float* lse, float* delta, float* dq, float* dk,
                       float* dv, const long long* strides, const void* bias, int kind, const long long* bs, const uint8_t* skip, int B, int H, int Lq, int Lk,
                       int head_dim, float scale, hipStream_t stream) {
    SDVAR_CHECK_ARG(q && k && v && out && dout && strides, "sdpa_bwd: null operand");
    SDVAR_CHECK_ARG(lse, "sdpa_bwd: null lse");
    SDVAR_CHECK_ARG(delta, "sdpa_bwd: null delta workspace");
    SDVAR_CHECK_ARG(dq || dk || dv, "sdpa_bwd: dq, dk and dv are all NULL - nothing to compute");
    SDVAR_CHECK_ARG(head_dim == 64, "sdpa_bwd: head dim %d (only 64 is built)", head_dim);
    SDVAR_CHECK_ARG(B >= 1 && H >= 1 && Lq >= 1 && Lk >= 1 && B <= 65535 && H <= 65535, "sdpa_bwd: bad extents B=%d H=%d Lq=%d Lk=%d", B, H, Lq, Lk);
    SDVAR_CHECK_ARG(((long long)B * H * Lq + 15) / 16 <= 2147483647LL, "sdpa_bwd: B*H*Lq too large");
    static const char* const names[8] = {"q", "k", "v", "out", "dout", "dq", "dk", "dv"};
    const void* const ptrs[8] = {q, k, v, out, dout, dq, dk, dv};
    for (int i = 0; i < 8; ++i) {
        if (!ptrs[i]) continue;             // an absent gradient
        SDVAR_CHECK_ARG(aligned_strides(strides + 3 * i), "sdpa_bwd: %s strides (%lld, %lld, %lld) - token rows must be 16-byte aligned (every stride a non-negative multiple of 4 floats)",
                        names[i], strides[3 * i], strides[3 * i + 1], strides[3 * i + 2]);
        SDVAR_CHECK_ARG(((uintptr_t)ptrs[i] & 15) == 0, "sdpa_bwd: %s is not 16-byte aligned", names[i]);
    }
    SDVAR_CHECK_ARG((((uintptr_t)lse | (uintptr_t)delta) & 3) == 0, "sdpa_bwd: lse / delta is not 4-byte aligned");
    SDVAR_CHECK_ARG(kind >= BIAS_NONE && kind <= BIAS_U8, "sdpa_bwd: bias kind %d (0 = none, 1 = fp32 additive, 2 = uint8 keep-mask)", kind);
    SDVAR_CHECK_ARG((kind == BIAS_NONE) == (bias == nullptr), "sdpa_bwd: bias pointer and bias kind %d disagree", kind);
    SDVAR_CHECK_ARG(kind == BIAS_NONE || (bs && bs[0] >= 0 && bs[1] >= 0 && bs[2] >= 0), "sdpa_bwd: bias strides missing or negative");
    SDVAR_CHECK_ARG(kind != BIAS_NONE || !skip, "sdpa_bwd: a skip map needs a bias");
    SdpaBwdArgs a;
    a.q = q; a.k = k; a.v = v; a.out = out; a.dout = dout; a.lse = lse; a.delta = delta; a.dq = dq; a.dk = dk; a.dv = dv;
    for (int i = 0; i < 3; ++i) {
        a.qs[i] = strides[i]; a.ks[i] = strides[3 + i]; a.vs[i] = strides[6 + i]; a.os[i] = strides[9 + i]; a.gs[i] = strides[12 + i];
        a.dqs[i] = strides[15 + i]; a.dks[i] = strides[18 + i]; a.dvs[i] = strides[21 + i]; a.bs[i] = kind ? bs[i] : 0;
    }
    a.bias = bias; a.skip = skip; a.nkt = (Lk + KT - 1) / KT;
    const uintptr_t balign = kind == BIAS_F32 ? 15 : 3;
    a.bias_vec = kind != BIAS_NONE && ((uintptr_t)bias & balign) == 0 && bs[0] % 4 == 0 && bs[1] % 4 == 0 && bs[2] % 4 == 0;
    a.B = B; a.H = H; a.Lq = Lq; a.Lk = Lk; a.scale = scale;

    const long long rows = (long long)B * H * Lq;
    hipLaunchKernelGGL(sdpa_bwd_delta_kernel, dim3((unsigned)((rows + 15) / 16)), dim3(256), 0, stream, a);
    SDVAR_LAUNCH_CHECK();
    if (dk || dv) {
        const size_t lds = 2 * (size_t)(2 * TILE + 2 * KT) * sizeof(float);
        static LdsOptIn opt_in;
        SDVAR_LDS_OPT_IN(opt_in, lds, (const void*)sdpa_bwd_dkdv_kernel<BIAS_NONE>, (const void*)sdpa_bwd_dkdv_kernel<BIAS_F32>, (const void*)sdpa_bwd_dkdv_kernel<BIAS_U8>);
        const dim3 grid((Lk + KB - 1) / KB, H, B);
        if (kind == BIAS_F32) hipLaunchKernelGGL(sdpa_bwd_dkdv_kernel<BIAS_F32>, grid, dim3(256), lds, stream, a);
        else if (kind == BIAS_U8) hipLaunchKernelGGL(sdpa_bwd_dkdv_kernel<BIAS_U8>, grid, dim3(256), lds, stream, a);
        else hipLaunchKernelGGL(sdpa_bwd_dkdv_kernel<BIAS_NONE>, grid, dim3(256), lds, stream, a);
        SDVAR_LAUNCH_CHECK();
    }
    if (dq) {
        const size_t lds = 2 * (size_t)(2 * TILE) * sizeof(float);
        static LdsOptIn opt_in;
        SDVAR_LDS_OPT_IN(opt_in, lds, (const void*)sdpa_bwd_dq_kernel<BIAS_NONE>, (const void*)sdpa_bwd_dq_kernel<BIAS_F32>, (const void*)sdpa_bwd_dq_kernel<BIAS_U8>);
        const dim3 grid((Lq + QB - 1) / QB, H, B);
        if (kind == BIAS_F32) hipLaunchKernelGGL(sdpa_bwd_dq_kernel<BIAS_F32>, grid, dim3(256), lds, stream, a);
        else if (kind == BIAS_U8) hipLaunchKernelGGL(sdpa_bwd_dq_kernel<BIAS_U8>, grid, dim3(256), lds, stream, a);
        else hipLaunchKernelGGL(sdpa_bwd_dq_kernel<BIAS_NONE>, grid, dim3(256), lds, stream, a);
        SDVAR_LAUNCH_CHECK();
    }
    return SDVAR_OK;
}

}  // namespace sdvar
