// The conditioning linears of a trained block under autograd: ada_lin = Sequential(SiLU, Linear(D, 6C)) (basic_var.py:147, 156) and the head norm's
// Sequential(SiLU, Linear(D, 2C)) (:170, 173), both directions:
//
//   forward    y[m, n]  = sum_k s[m, k] w[n, k] + b[n],   s = silu(c)
//   backward   dW[n, k] = sum_m dy[m, n] s[m, k],   db[n] = sum_m dy[m, n],   dc[m, k] = (sum_n dy[m, n] w[n, k]) silu'(c[m, k])
//
// M is the batch (1 .. 64), so the shape is a bundle of matrix-vector products: all the bytes are in W (N x K), the work is ~0.1 GFLOP, and the kernels are plain fp32
// vector code that streams W once per direction.  No matrix cores, no operand planes, no cache, no atomics.
//
// The lane map of both directions: a lane owns KL consecutive k of a chunk of 64 KL (forward: KL = 4; backward: 4 for M <= 16, 2 beyond; M > 32: dc's sums from one launch per 32 rows, dW and db from a launch of their own), so a wave reads a row of W in
// whole 16- or 8-byte pieces, 1 KB - 256 B per instruction, and everything that is per (m, k) - s, the dc partial sums - is lane-local.  s is computed once per
// workgroup and chunk into LDS (fp32 words; in the half modes they hold the rounded value) and read back 16 / 8 bytes per lane, conflict-free.
//
//   forward   a workgroup owns CL_FSLAB = 16 rows of W, a wave CL_FR = 4 of them, and walks the chunks of K: acc[r][m] += s[m][k] w[n + r][k] with one fmaf per product,
//             k ascending inside the lane; the 4 MP sums of a wave are then added over the 64 lanes at once (cl_reduce_lanes: the butterfly's additions, a sixth of
//             its exchanges) and each lane stores the outputs it ends up with.  The order of a sum depends on K alone.  s sits in two LDS buffers: the next chunk's
//             words of c and rows of W are loaded, and its s written, under this chunk's arithmetic - one barrier per chunk.  The accumulators are a template width
//             MP = 8 / 16; M > 16 takes further passes of 16 rows over the workgroup's own 16 rows of W, which it has just read (assumed to come from a cache; a 32-wide
//             accumulator left one wave per SIMD and was slower in every shape but one).
//   backward  a workgroup owns (slab of CL_BSLAB = 64 rows of W) x (one chunk of K); wave v takes the row groups v, v + 4, v + 8, v + 12 of 4 rows.  Per group: W is loaded once
//             (the next group's rows are in flight meanwhile), dW[n + r][k] = sum_m dy[m][n + r] s[m][k] stays in the lane and is stored in W's dtype; p[m][k] +=
//             dy[m][n + r] w[n + r][k] accumulates in MP x KL registers over the wave's 16 rows.  The four waves are added through LDS as ((v0 + v1) + v2) + v3 into the
//             workspace [slab][m][k]; cond_lin_dc_kernel adds the slabs (slice t of 4: slabs t, t + 4, .. in index order; the slices as ((t0 + t1) + t2) + t3),
//             multiplies by silu'(c) and rounds once to c's dtype.  dy of the slab sits in LDS transposed, [n][m], and is read as broadcast words.  Without dc, W is
//             not read at all.
// The arithmetic dtype and "dc / dW asked for" are template arguments: decided at run time they put a branch around every conversion and every fmaf.
// Nothing here synchronises with the host or allocates.
#include <type_traits>

#include "common.h"

namespace sdvar {

constexpr int CL_MAX_M = 64, CL_MAX_K = 4096;
constexpr int CL_FKC = 256;          // k per chunk of the forward: 64 lanes x 4
constexpr int CL_FR = 4;             // rows of W per wave of the forward
constexpr int CL_FSLAB = 16;         // rows of W per workgroup of the forward (4 waves)
constexpr int CL_BSLAB = 64;         // rows of W per workgroup of the backward: fixes the workspace size and the order of dc's sum over n

// silu(x) = x / (1 + expf(-x)): libm's expf and a correctly rounded division, as cl_silu_grad below.  expf(-x) is +inf for x < -88.7: x / inf = -0; it is 0 for
// large x: the result is x.  A workgroup evaluates this for every (m, k) of its chunk - per element of c, not of W.
__device__ __forceinline__ float cl_silu(float x) { return x / (1.0f + expf(-x)); }
__device__ __forceinline__ float cl_silu_grad(float x) {
    const float sg = 1.0f / (1.0f + expf(-x));          // 0 where expf overflows, 1 where it underflows: both ends finite
    return sg * (1.0f + x * (1.0f - sg));
}
__device__ __forceinline__ float cl_round(float v, bool bf) { return half_lo(half_pack2(v, 0.0f, bf), bf); }
__device__ __forceinline__ float cl_widen(uint16_t h, bool bf) { return half_lo((uint32_t)h, bf); }

// KL (4 or 2) consecutive values at element e of a matrix, widened to fp32; ROUND: an fp32 source is rounded to the half dtype (nearest even) as it is read
template <int KL, bool H, bool ROUND>
__device__ __forceinline__ void cl_load(const void* __restrict__ p, size_t e, bool bf, float* v) {
    if (H) {
        if (KL == 4) {
            const uint2 w = *reinterpret_cast<const uint2*>(reinterpret_cast<const uint16_t*>(p) + e);
            v[0] = half_lo(w.x, bf); v[1] = half_hi(w.x, bf); v[2] = half_lo(w.y, bf); v[3] = half_hi(w.y, bf);
        } else {
            const uint32_t w = *reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint16_t*>(p) + e);
            v[0] = half_lo(w, bf); v[1] = half_hi(w, bf);
        }
        return;
    }
    if (KL == 4) {
        const f32x4 w = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(p) + e);
        v[0] = w[0]; v[1] = w[1]; v[2] = w[2]; v[3] = w[3];
    } else {
        const f32x2p w = *reinterpret_cast<const f32x2p*>(reinterpret_cast<const float*>(p) + e);
        v[0] = w[0]; v[1] = w[1];
    }
    if (ROUND) {
#pragma unroll
        for (int i = 0; i < KL; i += 2) { const uint32_t q = half_pack2(v[i], v[i + 1], bf); v[i] = half_lo(q, bf); v[i + 1] = half_hi(q, bf); }
    }
}
// KL consecutive values -> memory at element e, fp32 or rounded once to the half dtype
template <int KL, bool H>
__device__ __forceinline__ void cl_store(void* __restrict__ p, size_t e, bool bf, const float* v) {
    if (H) {
        if (KL == 4) *reinterpret_cast<uint2*>(reinterpret_cast<uint16_t*>(p) + e) = uint2{half_pack2(v[0], v[1], bf), half_pack2(v[2], v[3], bf)};
        else *reinterpret_cast<uint32_t*>(reinterpret_cast<uint16_t*>(p) + e) = half_pack2(v[0], v[1], bf);
    } else {
        if (KL == 4) *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(p) + e) = f32x4{v[0], v[1], v[2], v[3]};
        else *reinterpret_cast<f32x2p*>(reinterpret_cast<float*>(p) + e) = f32x2p{v[0], v[1]};
    }
}

// s = silu(c) of rows m0 .. m0 + mcount - 1, columns k0 .. k0 + KC - 1 -> sS[m][KC] (fp32 words; AH: holding the value rounded to half); columns past K are zeros.
// The one place s is computed, in both directions: the same bits.  Two steps, so that a kernel can put other work between them: cl_stage_load issues every load of
// the thread at once (MP KC / 1024 quads of 4 values; a quad outside the rows or columns reads a clamped, valid address and is dropped later - a loop of guarded loads
// waits for each of them in turn), cl_stage_store evaluates the SiLU and writes LDS.
template <int MP, int KC, bool CH>
__device__ __forceinline__ void cl_stage_load_t(u32x4* raw, const void* __restrict__ c, long long ldc, int m0, int mcount, int k0, int K) {
    constexpr int QR = KC / 4, NQ = MP * QR / 256;
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
        const int q = threadIdx.x + 256 * i, m = min(q / QR, mcount - 1), k = min(k0 + (q % QR) * 4, K - 4);
        const size_t e = (size_t)(m0 + m) * (size_t)ldc + k;
        if (CH) { const uint2 w = *reinterpret_cast<const uint2*>(reinterpret_cast<const uint16_t*>(c) + e); raw[i] = u32x4{w.x, w.y, 0u, 0u}; }
        else raw[i] = *reinterpret_cast<const u32x4*>(reinterpret_cast<const float*>(c) + e);
    }
}
template <int MP, int KC>
__device__ __forceinline__ void cl_stage_load(u32x4* raw, const void* __restrict__ c, int cdt, long long ldc, int m0, int mcount, int k0, int K) {
    if (cdt != 0) cl_stage_load_t<MP, KC, true>(raw, c, ldc, m0, mcount, k0, K);          // wave-uniform, outside the loops over W
    else cl_stage_load_t<MP, KC, false>(raw, c, ldc, m0, mcount, k0, K);
}
template <int MP, int KC, bool AH>
__device__ __forceinline__ void cl_stage_store(float* sS, const u32x4* raw, int cdt, int mcount, int k0, int K, bool bf) {
    constexpr int QR = KC / 4, NQ = MP * QR / 256;
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
        const int q = threadIdx.x + 256 * i, m = q / QR, kq = (q % QR) * 4;
        {
            float v[4] = {0.f, 0.f, 0.f, 0.f};          // rows past mcount and columns past K are zeros: the backward multiplies such a row by its zero dy
            if (m < mcount && k0 + kq < K) {
                if (cdt != 0) { const bool cb = cdt == 2; v[0] = half_lo(raw[i][0], cb); v[1] = half_hi(raw[i][0], cb); v[2] = half_lo(raw[i][1], cb); v[3] = half_hi(raw[i][1], cb); }
                else { v[0] = __uint_as_float(raw[i][0]); v[1] = __uint_as_float(raw[i][1]); v[2] = __uint_as_float(raw[i][2]); v[3] = __uint_as_float(raw[i][3]); }
#pragma unroll
                for (int j = 0; j < 4; ++j) { v[j] = cl_silu(v[j]); if (AH) v[j] = cl_round(v[j], bf); }
            }
            *reinterpret_cast<f32x4*>(sS + m * KC + kq) = f32x4{v[0], v[1], v[2], v[3]};
        }
    }
}

// The sum over the 64 lanes of CNT values per lane, all at once: at the level of lane bit MSK a lane keeps one value of each pair and hands the other to its partner,
// so a level costs CNT / 2 exchanges instead of CNT and the whole reduction ~CNT instead of 6 CNT.  Every value is still added as the butterfly
// (xor 32, 16, .., 1) adds it - x[l] + x[l ^ MSK] per level, and an fp32 add commutes - so the bits are wave_sum's.  Afterwards value i of lane l is the sum of the
// original value i 2^L + rev, L = min(6, log2 CNT), rev = the L top bits of l reversed (bit 5 of the lane is bit 0 of the index); with CNT < 64 the last levels are plain
// butterflies and 64 / CNT lanes hold each sum.
template <int CNT, int MSK>
__device__ __forceinline__ void cl_reduce_lanes(float* v, int lane) {
    if constexpr (MSK >= 1) {
        if constexpr (CNT > 1) {
            const bool up = (lane & MSK) != 0;
#pragma unroll
            for (int i = 0; i < CNT / 2; ++i) {
                const float keep = up ? v[2 * i + 1] : v[2 * i], send = up ? v[2 * i] : v[2 * i + 1];
                v[i] = keep + __shfl_xor(send, MSK, 64);
            }
            cl_reduce_lanes<CNT / 2, MSK / 2>(v, lane);
        } else {
            v[0] += __shfl_xor(v[0], MSK, 64);
            cl_reduce_lanes<1, MSK / 2>(v, lane);
        }
    }
}
constexpr int cl_log2(int v) { return v <= 1 ? 0 : 1 + cl_log2(v / 2); }

// ------------------------------------------------------------------------------------------------ forward
// grid: ceil(N / 16) workgroups of 256 threads.  MP = rows of c per pass (accumulators per row of W; 8 and 16 are launched); WH: w is half; ADT: the arithmetic code.
template <int MP, bool WH, int ADT>
__global__ __launch_bounds__(256) void cond_lin_fwd_kernel(const void* __restrict__ c, int cdt, long long ldc, const void* __restrict__ w, const float* __restrict__ b,
                                                           void* __restrict__ y, int M, int N, int K) {
    constexpr bool AH = ADT != 0, bf = ADT == 2;          // compile-time: a run-time dtype put a branch around every conversion
    __shared__ __attribute__((aligned(16))) float sS[2][MP * CL_FKC];          // s of two chunks: one is read while the next is written
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int n0 = blockIdx.x * CL_FSLAB + wv * CL_FR;          // N % 4 == 0: a wave's 4 rows are all inside or all outside
    const bool rows_live = n0 < N;
    const int nchunk = (K + CL_FKC - 1) / CL_FKC;
    const int kl = 4 * lane;                                     // K % 8 == 0: a lane's 4 columns of a chunk are all inside or all outside
    constexpr int NQ = MP * (CL_FKC / 4) / 256;
    constexpr bool CPF = MP <= 16;          // a wider accumulator has no registers for loads in flight under the arithmetic
#pragma unroll 1
    for (int m0 = 0; m0 < M; m0 += MP) {
        const int mcount = min(MP, M - m0);
        float acc[CL_FR][MP];
#pragma unroll
        for (int r = 0; r < CL_FR; ++r)
#pragma unroll
            for (int m = 0; m < MP; ++m) acc[r][m] = 0.f;
        u32x4 raw[NQ];
        float wn[CL_FR][4];                  // the next chunk's W, in flight while this one is multiplied
        cl_stage_load<MP, CL_FKC>(raw, c, cdt, ldc, m0, mcount, 0, K);
        if (CPF && rows_live && kl < K) {
#pragma unroll
            for (int r = 0; r < CL_FR; ++r) cl_load<4, WH, AH>(w, (size_t)(n0 + r) * K + kl, bf, wn[r]);
        }
        cl_stage_store<MP, CL_FKC, AH>(sS[0], raw, cdt, mcount, 0, K, bf);          // the last pass's reads ended at its closing barrier
        __syncthreads();
#pragma unroll 1
        for (int ch = 0; ch < nchunk; ++ch) {
            const int k = ch * CL_FKC + kl;
            const bool live = rows_live && k < K, more = ch + 1 < nchunk;
            const float* sC = sS[ch & 1];
            float wc[CL_FR][4];
            if (!CPF && live) {
#pragma unroll
                for (int r = 0; r < CL_FR; ++r) cl_load<4, WH, AH>(w, (size_t)(n0 + r) * K + k, bf, wn[r]);
            }
#pragma unroll
            for (int r = 0; r < CL_FR; ++r)
#pragma unroll
                for (int e = 0; e < 4; ++e) wc[r][e] = wn[r][e];
            // the next chunk's loads, in flight under the arithmetic below
            if (CPF && more) cl_stage_load<MP, CL_FKC>(raw, c, cdt, ldc, m0, mcount, (ch + 1) * CL_FKC, K);
            if (CPF && rows_live && k + CL_FKC < K) {
#pragma unroll
                for (int r = 0; r < CL_FR; ++r) cl_load<4, WH, AH>(w, (size_t)(n0 + r) * K + k + CL_FKC, bf, wn[r]);
            }
            if (live) {
#pragma unroll
                for (int m = 0; m < MP; ++m)
                    if (m < mcount) {
                        const f32x4 s4 = *reinterpret_cast<const f32x4*>(sC + m * CL_FKC + kl);
#pragma unroll
                        for (int r = 0; r < CL_FR; ++r)
#pragma unroll
                            for (int e = 0; e < 4; ++e) acc[r][m] = __builtin_fmaf(s4[e], wc[r][e], acc[r][m]);
                    }
            }
            if (more) {
                if (!CPF) cl_stage_load<MP, CL_FKC>(raw, c, cdt, ldc, m0, mcount, (ch + 1) * CL_FKC, K);
                cl_stage_store<MP, CL_FKC, AH>(sS[(ch + 1) & 1], raw, cdt, mcount, (ch + 1) * CL_FKC, K, bf);          // last read before the previous barrier
            }
            __syncthreads();
        }
        // the 4 MP sums of the wave at once; value index o = 4 m + r
        constexpr int V = CL_FR * MP, LV = V >= 64 ? 6 : cl_log2(V), PER = V >= 64 ? V / 64 : 1;
        float v[V];
#pragma unroll
        for (int m = 0; m < MP; ++m)
#pragma unroll
            for (int r = 0; r < CL_FR; ++r) v[4 * m + r] = acc[r][m];
        cl_reduce_lanes<V, 32>(v, lane);
        const int rev = (int)(__brev((unsigned)(lane >> (6 - LV))) >> (32 - LV));
        if (rows_live && (lane & ((1 << (6 - LV)) - 1)) == 0) {
#pragma unroll
            for (int i = 0; i < PER; ++i) {
                const int o = (i << LV) + rev, m = o >> 2, r = o & 3;
                if (m < mcount) {
                    float t = v[i];
                    if (b) t += b[n0 + r];
                    const size_t e = (size_t)(m0 + m) * N + n0 + r;
                    if (AH) reinterpret_cast<uint16_t*>(y)[e] = (uint16_t)(half_pack2(t, 0.f, bf) & 0xFFFFu);
                    else reinterpret_cast<float*>(y)[e] = t;
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ backward, pass 1
// grid: (ceil(N / 64), ceil(K / (64 KL))) workgroups of 256 threads; M <= MP.  DC: the dc partial sums are asked for (W is read); DWF: dW is.
// A lane whose columns are past K (the last chunk) runs the same instructions on a clamped address and stores nothing: a lane-divergent exit from the loops
// made hipcc predicate every accumulator (more v_cndmask and v_mov than fmaf).
template <int MP, int KL, bool WH, int ADT, bool DC, bool DWF>
__global__ __launch_bounds__(256) void cond_lin_bwd_kernel(const void* __restrict__ dy, const void* __restrict__ c, int cdt, long long ldc, const void* __restrict__ w,
                                                           void* __restrict__ dW, float* __restrict__ db, float* __restrict__ ws, int ws_rows, int ws_row0, int M, int N, int K) {
    constexpr int KC = 64 * KL;
    constexpr bool AH = ADT != 0, bf = ADT == 2;
    __shared__ __attribute__((aligned(16))) float sS[MP * KC];          // s of the chunk; afterwards the running sum of the waves' dc partials
    __shared__ __attribute__((aligned(16))) float dS[CL_BSLAB * MP];    // dy of the slab, transposed: [n][m], zeros outside (M, N)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int slab = blockIdx.x, k0 = blockIdx.y * KC, nb = slab * CL_BSLAB;
    constexpr int NQ = MP * (KC / 4) / 256, ND = MP * CL_BSLAB / 256;
    u32x4 raw[NQ];
    float dv[ND];
    cl_stage_load<MP, KC>(raw, c, cdt, ldc, 0, M, k0, K);
#pragma unroll
    for (int i = 0; i < ND; ++i) {          // every load of the thread at once, from clamped addresses; what is outside (M, N) becomes a zero below
        const int idx = threadIdx.x + 256 * i;
        const size_t e = (size_t)min(idx >> 6, M - 1) * N + min(nb + (idx & 63), N - 1);
        dv[i] = AH ? cl_widen(reinterpret_cast<const uint16_t*>(dy)[e], bf) : reinterpret_cast<const float*>(dy)[e];
    }
    const int k = k0 + KL * lane, kc = min(k, K - KL);          // kc: where the lane loads from
    const bool klive = k < K;          // K % 8 == 0: a lane's KL columns are all inside or all outside
    constexpr bool PF = MP <= 32;       // the next group's W in flight under this group's arithmetic (MP = 64 has no registers left for it)
    float wn[4][KL];
    if (DC && PF && nb + 4 * wv < N) {
#pragma unroll
        for (int r = 0; r < 4; ++r) cl_load<KL, WH, AH>(w, (size_t)(nb + 4 * wv + r) * K + kc, bf, wn[r]);
    }
#pragma unroll
    for (int i = 0; i < ND; ++i) {
        const int idx = threadIdx.x + 256 * i, m = idx >> 6, nn = idx & 63;
        dS[nn * MP + m] = (m < M && nb + nn < N) ? dv[i] : 0.f;
    }
    cl_stage_store<MP, KC, AH>(sS, raw, cdt, M, k0, K, bf);
    __syncthreads();
    if (db && blockIdx.y == 0 && threadIdx.x < CL_BSLAB && nb + (int)threadIdx.x < N) {
        float t = 0.f;
        for (int m = 0; m < M; ++m) t += dS[threadIdx.x * MP + m];
        db[nb + threadIdx.x] = t;
    }
    float p[MP][KL];
#pragma unroll
    for (int m = 0; m < MP; ++m)
#pragma unroll
        for (int e = 0; e < KL; ++e) p[m][e] = 0.f;
#pragma unroll 1
    for (int i = 0; i < CL_BSLAB / 16; ++i) {
        const int nl = 4 * (wv + 4 * i), n = nb + nl;          // N % 4 == 0: a group's 4 rows are all inside or all outside
        if (n >= N) break;                                      // wave-uniform; no barrier inside the loop
        float wr[4][KL], dwa[4][KL];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (DC) {
                if (!PF) cl_load<KL, WH, AH>(w, (size_t)(n + r) * K + kc, bf, wn[r]);
#pragma unroll
                for (int e = 0; e < KL; ++e) wr[r][e] = wn[r][e];
            }
#pragma unroll
            for (int e = 0; e < KL; ++e) dwa[r][e] = 0.f;
        }
        if (DC && PF && n + 16 < N && i + 1 < CL_BSLAB / 16) {
#pragma unroll
            for (int r = 0; r < 4; ++r) cl_load<KL, WH, AH>(w, (size_t)(n + 16 + r) * K + kc, bf, wn[r]);
        }
#pragma unroll
        for (int mq = 0; mq < MP / 4; ++mq) {
            if (4 * mq < M) {
                f32x4 d4[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) d4[r] = *reinterpret_cast<const f32x4*>(dS + (nl + r) * MP + 4 * mq);          // one address per wave: a broadcast
#pragma unroll
                for (int mm = 0; mm < 4; ++mm) {
                    const int m = 4 * mq + mm;          // a row in [M, 4 ceil(M / 4)) has zeros in dS and sS: no guard per row (64 of them held 64 SGPR pairs)
                    {
                        float sv[KL];
                        if (DWF) {
                            if (KL == 4) { const f32x4 t = *reinterpret_cast<const f32x4*>(sS + m * KC + 4 * lane); sv[0] = t[0]; sv[1] = t[1]; sv[KL - 2] = t[2]; sv[KL - 1] = t[3]; }
                            else { const f32x2p t = *reinterpret_cast<const f32x2p*>(sS + m * KC + 2 * lane); sv[0] = t[0]; sv[1] = t[1]; }
                        }
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const float d = d4[r][mm];
#pragma unroll
                            for (int e = 0; e < KL; ++e) {
                                if (DC) p[m][e] = __builtin_fmaf(d, wr[r][e], p[m][e]);
                                if (DWF) dwa[r][e] = __builtin_fmaf(d, sv[e], dwa[r][e]);
                            }
                        }
                    }
                }
            }
        }
        if (DWF && klive) {
#pragma unroll
            for (int r = 0; r < 4; ++r) cl_store<KL, WH>(dW, (size_t)(n + r) * K + k, bf, dwa[r]);
        }
    }
    // ((v0 + v1) + v2) + v3 through the LDS words of s: a lane of every wave owns the same (m, k).  Every wave takes part, also one of the last slab whose row groups
    // all lie past N (its p is zero); a lane past K holds sums of clamped loads in p and never writes them (klive).
    if (DC) {
#pragma unroll 1
        for (int v = 0; v < 4; ++v) {
            __syncthreads();
            if (wv == v && klive) {
#pragma unroll
                for (int m = 0; m < MP; ++m)
                    if (m < M) {
                        float t[KL];
#pragma unroll
                        for (int e = 0; e < KL; ++e) t[e] = v == 0 ? p[m][e] : sS[m * KC + KL * lane + e] + p[m][e];
                        if (v < 3) {
#pragma unroll
                            for (int e = 0; e < KL; ++e) sS[m * KC + KL * lane + e] = t[e];
                        } else {
                            cl_store<KL, false>(ws, ((size_t)slab * ws_rows + ws_row0 + m) * K + k, false, t);          // the rows of this launch inside the slab's ws_rows
                        }
                    }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ backward, pass 2
// dc[m, k .. k + 3] = (sum over the slabs of ws[slab][m][k ..]) silu'(c[m, k ..]), dense (M, K) in c's dtype.  256 threads = 64 quads x 4 slices.
__global__ __launch_bounds__(256) void cond_lin_dc_kernel(const float* __restrict__ ws, const void* __restrict__ c, int cdt, long long ldc, void* __restrict__ dc, int nslab,
                                                          int M, int K) {
    __shared__ f32x4 red[4][64];
    const int qx = threadIdx.x & 63, sl = threadIdx.x >> 6, q = blockIdx.x * 64 + qx, qr = K >> 2;
    const bool live = q < M * qr;
    const int m = live ? q / qr : 0, k = live ? (q - m * qr) * 4 : 0;
    f32x4 a = {0.f, 0.f, 0.f, 0.f};
    if (live) {
        const float* p = ws + (size_t)m * K + k;
#pragma unroll 8
        for (int s = sl; s < nslab; s += 4) a += *reinterpret_cast<const f32x4*>(p + (size_t)s * M * K);
    }
    red[sl][qx] = a;
    __syncthreads();
    if (sl == 0 && live) {
        const f32x4 t = ((red[0][qx] + red[1][qx]) + red[2][qx]) + red[3][qx];
        float x[4], o[4];
        if (cdt != 0) cl_load<4, true, false>(c, (size_t)m * (size_t)ldc + k, cdt == 2, x);
        else cl_load<4, false, false>(c, (size_t)m * (size_t)ldc + k, false, x);
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = t[e] * cl_silu_grad(x[e]);
        if (cdt != 0) cl_store<4, true>(dc, (size_t)m * K + k, cdt == 2, o);
        else cl_store<4, false>(dc, (size_t)m * K + k, false, o);
    }
}

// ------------------------------------------------------------------------------------------------ host side
static inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

static int check_args(const char* who, const void* c, int cdt, long long ldc, const void* w, int wdt, int adt, int M, int N, int K) {
    SDVAR_CHECK_ARG(M >= 1 && M <= CL_MAX_M, "%s: M=%d must be in [1, %d] (the batch; larger products belong to the GEMM seam)", who, M, CL_MAX_M);
    SDVAR_CHECK_ARG(K >= 8 && K <= CL_MAX_K && K % 8 == 0, "%s: K=%d must be a multiple of 8 in [8, %d]", who, K, CL_MAX_K);
    SDVAR_CHECK_ARG(N >= 8 && N % 8 == 0 && (long long)N * K <= 0x7FFFFFFFll, "%s: N=%d must be a multiple of 8, at least 8, with N * K below 2^31", who, N);
    SDVAR_CHECK_ARG(adt >= 0 && adt <= 2, "%s: arithmetic code dtype=%d (0 fp32, 1 fp16, 2 bf16)", who, adt);
    SDVAR_CHECK_ARG((cdt == 0 || cdt == adt) && (wdt == 0 || wdt == adt) && cdt >= 0 && wdt >= 0,
                    "%s: dtype codes c=%d w=%d next to arithmetic code %d: each must be 0 (fp32) or the arithmetic code", who, cdt, wdt, adt);
    SDVAR_CHECK_ARG(c && w, "%s: null c or w", who);
    SDVAR_CHECK_ARG(al16(c) && al16(w), "%s: c and w must be 16-byte aligned", who);
    SDVAR_CHECK_ARG(ldc >= K && ldc % (cdt == 0 ? 4 : 8) == 0, "%s: ldc=%lld must be at least K=%d and a multiple of 16 bytes", who, ldc, K);
    return SDVAR_OK;
}

long long cond_lin_bwd_ws_bytes(int M, int N, int K) {
    const bool ok = M >= 1 && M <= CL_MAX_M && K >= 8 && K <= CL_MAX_K && K % 8 == 0 && N >= 8 && N % 8 == 0 && (long long)N * K <= 0x7FFFFFFFll;
    if (!ok) { set_error("cond_lin_bwd_ws_bytes: M=%d, N=%d, K=%d: 1 <= M <= %d, K %% 8 == 0 in [8, %d], N %% 8 == 0, N * K < 2^31", M, N, K, CL_MAX_M, CL_MAX_K); return -1; }
    return (long long)((N + CL_BSLAB - 1) / CL_BSLAB) * M * K * (long long)sizeof(float);
}

// compile-time dispatch: "w is half" and the arithmetic code (w half implies its own dtype's arithmetic)
template <typename F>
static inline void with_arith(int wdt, int adt, F f) {
    if (adt == 0) f(std::false_type{}, std::integral_constant<int, 0>{});
    else if (adt == 1) { if (wdt == 0) f(std::false_type{}, std::integral_constant<int, 1>{}); else f(std::true_type{}, std::integral_constant<int, 1>{}); }
    else { if (wdt == 0) f(std::false_type{}, std::integral_constant<int, 2>{}); else f(std::true_type{}, std::integral_constant<int, 2>{}); }
}

int cond_lin_fwd(const void* c, int cdt, long long ldc, const void* w, int wdt, const float* b, void* y, int adt, int M, int N, int K, hipStream_t stream) {
    if (int rc = check_args("cond_lin_fwd", c, cdt, ldc, w, wdt, adt, M, N, K)) return rc;
    SDVAR_CHECK_ARG(y && al16(y) && al16(b), "cond_lin_fwd: y must be given, y and b 16-byte aligned");
    const dim3 grid((unsigned)((N + CL_FSLAB - 1) / CL_FSLAB)), blk(256);
    with_arith(wdt, adt, [&](auto wh, auto ah) {
        constexpr bool WH = decltype(wh)::value;
        constexpr int AD = decltype(ah)::value;
        if (M <= 8) hipLaunchKernelGGL((cond_lin_fwd_kernel<8, WH, AD>), grid, blk, 0, stream, c, cdt, ldc, w, b, y, M, N, K);
        else hipLaunchKernelGGL((cond_lin_fwd_kernel<16, WH, AD>), grid, blk, 0, stream, c, cdt, ldc, w, b, y, M, N, K);          // M > 16: passes of 16 rows
    });
    SDVAR_LAUNCH_CHECK();
    return SDVAR_OK;
}

template <int MP, int KL, bool WH, int AH>
static inline void launch_bwd(bool need_dc, dim3 grid, hipStream_t stream, const void* dy, const void* c, int cdt, long long ldc, const void* w, void* dW, float* db, float* ws,
                              int ws_rows, int ws_row0, int M, int N, int K) {
    const dim3 blk(256);
    if (need_dc && dW) hipLaunchKernelGGL((cond_lin_bwd_kernel<MP, KL, WH, AH, true, true>), grid, blk, 0, stream, dy, c, cdt, ldc, w, dW, db, ws, ws_rows, ws_row0, M, N, K);
    else if (need_dc) hipLaunchKernelGGL((cond_lin_bwd_kernel<MP, KL, WH, AH, true, false>), grid, blk, 0, stream, dy, c, cdt, ldc, w, dW, db, ws, ws_rows, ws_row0, M, N, K);
    else if (dW) hipLaunchKernelGGL((cond_lin_bwd_kernel<MP, KL, WH, AH, false, true>), grid, blk, 0, stream, dy, c, cdt, ldc, w, dW, db, ws, ws_rows, ws_row0, M, N, K);
    else hipLaunchKernelGGL((cond_lin_bwd_kernel<MP, KL, WH, AH, false, false>), grid, blk, 0, stream, dy, c, cdt, ldc, w, dW, db, ws, ws_rows, ws_row0, M, N, K);
}
// M > 32: dW and db from one launch over all the rows (64 accumulators per lane would be 256 registers beside dc's sums and spilled scalar registers), dc's partial
// sums from one launch per 32 rows of c and dy - each reads W once more; such batches are outside the traffic condition
template <bool WH, int AH>
static inline void launch_bwd_wide(bool need_dc, dim3 grid, hipStream_t stream, const void* dy, const void* c, int cdt, long long ldc, const void* w, void* dW, float* db,
                                   float* ws, int adt, int M, int N, int K) {
    const dim3 blk(256);
    if (dW) hipLaunchKernelGGL((cond_lin_bwd_kernel<64, 2, WH, AH, false, true>), grid, blk, 0, stream, dy, c, cdt, ldc, w, dW, db, ws, M, 0, M, N, K);
    else if (db) hipLaunchKernelGGL((cond_lin_bwd_kernel<64, 2, WH, AH, false, false>), grid, blk, 0, stream, dy, c, cdt, ldc, w, dW, db, ws, M, 0, M, N, K);
    if (!need_dc) return;
    const size_t cel = cdt == 0 ? 4 : 2, yel = adt == 0 ? 4 : 2;
    for (int m0 = 0; m0 < M; m0 += 32)
        hipLaunchKernelGGL((cond_lin_bwd_kernel<32, 2, WH, AH, true, false>), grid, blk, 0, stream, (const char*)dy + (size_t)m0 * N * yel, (const char*)c + (size_t)m0 * ldc * cel,
                           cdt, ldc, w, (void*)nullptr, (float*)nullptr, ws, M, m0, min(32, M - m0), N, K);
}

int cond_lin_bwd(const void* dy, const void* c, int cdt, long long ldc, const void* w, int wdt, void* dc, void* dW, float* db, float* ws, int adt, int M, int N, int K,
                 hipStream_t stream) {
    if (int rc = check_args("cond_lin_bwd", c, cdt, ldc, w, wdt, adt, M, N, K)) return rc;
    SDVAR_CHECK_ARG(dy && al16(dy), "cond_lin_bwd: dy must be given and 16-byte aligned");
    SDVAR_CHECK_ARG(dc || dW || db, "cond_lin_bwd: no output asked for (dc, dW and db are all null)");
    SDVAR_CHECK_ARG(al16(dc) && al16(dW) && al16(db) && al16(ws), "cond_lin_bwd: dc, dW, db and the workspace must be 16-byte aligned");
    SDVAR_CHECK_ARG(!dc || ws, "cond_lin_bwd: dc needs the workspace (sdvar_op_cond_lin_bwd_ws_bytes)");
    const int nslab = (N + CL_BSLAB - 1) / CL_BSLAB, kl = M <= 16 ? 4 : 2;
    const dim3 grid((unsigned)nslab, (unsigned)((K + 64 * kl - 1) / (64 * kl)));
    const bool need_dc = dc != nullptr;
    with_arith(wdt, adt, [&](auto wh, auto ah) {
        constexpr bool WH = decltype(wh)::value;
        constexpr int AH = decltype(ah)::value;
        if (M <= 8) launch_bwd<8, 4, WH, AH>(need_dc, grid, stream, dy, c, cdt, ldc, w, dW, db, ws, M, 0, M, N, K);
        else if (M <= 16) launch_bwd<16, 4, WH, AH>(need_dc, grid, stream, dy, c, cdt, ldc, w, dW, db, ws, M, 0, M, N, K);
        else if (M <= 32) launch_bwd<32, 2, WH, AH>(need_dc, grid, stream, dy, c, cdt, ldc, w, dW, db, ws, M, 0, M, N, K);
        else launch_bwd_wide<WH, AH>(need_dc, grid, stream, dy, c, cdt, ldc, w, dW, db, ws, adt, M, N, K);
    });
    SDVAR_LAUNCH_CHECK();
    if (need_dc) {
        hipLaunchKernelGGL(cond_lin_dc_kernel, dim3((unsigned)((M * (K >> 2) + 63) / 64)), dim3(256), 0, stream, ws, c, cdt, ldc, dc, nslab, M, K);
        SDVAR_LAUNCH_CHECK();
    }
    return SDVAR_OK;
}

}  // namespace sdvar
