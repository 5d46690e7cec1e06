// The prologue of a teacher-forced training step under autograd (VAR.forward, var.py:225-243), both directions:
//
//   forward    j_b = condition drop (r[b] < rate ? num_classes : label[b]);  cond[b] = class_emb[j_b];  e[l] = lvl_embed[lvl[l]] + pos_1LC[l]
//              x[b, l] = (class_emb[j_b] + pos_start[l]) + e[l]                          l <  first_l
//              x[b, l] = (sum_k xv[b, l - first_l, k] W[:, k] + bias) + e[l]             l >= first_l         (word_embed, K = Cvae <= 64)
//   backward   column sums of g over b (dpos_1LC, dpos_start), over b and the tokens of a stage (dlvl), over b and the word rows (dbias), g^T xv (dW), the rows of
//              class_emb that were gathered (dclass) and, when asked, g W (dxv)
//
// K is at most 64, so this is plain fp32 vector code bound by the bytes of x / g: no matrix cores, no operand planes, no atomics.
//
// The lane map of both big kernels: a lane owns CPT consecutive columns c (CPT = 4 for K <= 32, 2 beyond: CPT x KP = 128 registers hold the lane's rows of W in the
// forward and its rows of dW in the backward), a wave 64 CPT columns, and the four waves of a workgroup share those columns and split the tokens of a chunk: wave w
// takes tokens l0 + w, l0 + w + 4, ...  For a token the wave walks the images b = 0 .. B - 1 in order, so e[l] is formed once per token, and the token and the image are
// wave-uniform: xv[b, l - first_l, :] - 32 floats that every lane needs - is read through the scalar cache into scalar registers, not through LDS or per lane.
//
//   forward   a = fmaf(xv[k], W[c, k], a) for k = 0 .. K - 1 in order, then (a + bias[c]) + e[l, c]: the order of a sum depends on K alone, a row's bits do not depend
//             on B.  The half output is rounded once from that fp32 value.
//   backward  pass 1 (embed_bwd_kernel): a workgroup owns EMB_BWD_TOK = 8 tokens.  p[l, c] = sum_b g[b, l, c], b ascending from 0.0f, is complete inside one lane: it is
//             dpos_1LC[l], dpos_start[l] and row l of the workspace.  dW's partial sum of a wave: dwa[c, k] = fmaf(g[b, l, c], xv[b, l - first_l, k], dwa[c, k]) over its
//             tokens in order, b ascending inside a token; the four waves are added through LDS as ((w0 + w1) + w2) + w3 into the workspace [chunk][c][k].
//             pass 2: embed_sum_parts_kernel adds the chunks of dW (slice s of 4: chunks s, s + 4, .. in index order; the slices as ((s0 + s1) + s2) + s3);
//             embed_rows_kernel adds rows of p the same way (slice s: tokens s, s + 4, .. that qualify): dlvl[stage] over the tokens of the stage, dbias over l >= first_l.
//             embed_dclass_kernel: one lane owns a column of a row j of dclass and adds (gc[b, c] + sum_{l < first_l} g[b, l, c]) over the images with j_b = j, b ascending
//             (a read-modify-write of its own element in memory: no other lane touches it).
//             embed_dxv_kernel: one wave per row of xv; lane adds c = 4 lane + 256 i + e in the order i, e with one fmaf per term, then six butterfly levels.
// Nothing here synchronises with the host or allocates.
#include <type_traits>

#include "common.h"

namespace sdvar {

constexpr int EMB_MAX_C = 3072, EMB_MAX_K = 64;
constexpr int EMB_FWD_TOK = 16;         // tokens per workgroup of the forward (4 per wave): W is re-read from cache once per 16 B rows of output
constexpr int EMB_BWD_TOK = 8;          // tokens per workgroup of the backward: fixes the workspace size and the order of dW's sum
constexpr int EMB_CLS_SLAB = 16;        // rows of dclass per workgroup

__device__ __forceinline__ float emb_nan() { return __uint_as_float(0x7FC00000u); }

// the effective label of image b, or -1 when it is outside [0, NC1): the one place it is computed, in both directions
__device__ __forceinline__ int emb_label(const void* __restrict__ label, int i64, const float* __restrict__ r, float rate, int b, int NC1) {
    if (r && r[b] < rate) return NC1 - 1;
    const long long j = i64 ? reinterpret_cast<const long long*>(label)[b] : (long long)reinterpret_cast<const int*>(label)[b];
    return (j >= 0 && j < NC1) ? (int)j : -1;
}

// CPT (4 or 2) consecutive fp32 values
template <int CPT>
__device__ __forceinline__ void emb_load(const float* __restrict__ p, size_t e, float* v) {
    if (CPT == 4) { const f32x4 w = *reinterpret_cast<const f32x4*>(p + e); v[0] = w[0]; v[1] = w[1]; v[CPT - 2] = w[2]; v[CPT - 1] = w[3]; }
    else { const f32x2p w = *reinterpret_cast<const f32x2p*>(p + e); v[0] = w[0]; v[1] = w[1]; }
}
// CPT consecutive values of x / g: fp32, or half widened to fp32
template <int CPT, bool H>
__device__ __forceinline__ void emb_load_x(const void* __restrict__ p, size_t e, bool bf, float* v) {
    if (!H) { emb_load<CPT>(reinterpret_cast<const float*>(p), e, v); return; }
    if (CPT == 4) {
        const uint2 w = *reinterpret_cast<const uint2*>(reinterpret_cast<const uint16_t*>(p) + e);
        v[0] = half_lo(w.x, bf); v[1] = half_hi(w.x, bf); v[CPT - 2] = half_lo(w.y, bf); v[CPT - 1] = half_hi(w.y, bf);
    } else {
        const uint32_t w = *reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint16_t*>(p) + e);
        v[0] = half_lo(w, bf); v[1] = half_hi(w, bf);
    }
}
template <int CPT>
__device__ __forceinline__ void emb_store(float* __restrict__ p, size_t e, const float* v) {
    if (CPT == 4) *reinterpret_cast<f32x4*>(p + e) = f32x4{v[0], v[1], v[CPT - 2], v[CPT - 1]};
    else *reinterpret_cast<f32x2p*>(p + e) = f32x2p{v[0], v[1]};
}
// ... fp32, or rounded once (nearest even) to the half dtype
template <int CPT, bool H>
__device__ __forceinline__ void emb_store_x(void* __restrict__ p, size_t e, bool bf, const float* v) {
    if (!H) { emb_store<CPT>(reinterpret_cast<float*>(p), e, v); return; }
    if (CPT == 4) *reinterpret_cast<uint2*>(reinterpret_cast<uint16_t*>(p) + e) = uint2{half_pack2(v[0], v[1], bf), half_pack2(v[CPT - 2], v[CPT - 1], bf)};
    else *reinterpret_cast<uint32_t*>(reinterpret_cast<uint16_t*>(p) + e) = half_pack2(v[0], v[1], bf);
}

// 16 values of a row of xv -> xs, zeros past the krem values that remain (krem % 4 == 0, may be <= 0).  The row is wave-uniform, so these are scalar loads into scalar
// registers; a full group has no branch inside and leaves as one wide load.  The big kernels keep two groups: the next one's loads are issued before the current one is
// multiplied, so their latency is under 16 CPT fmaf.  FULL (K == KP, the reference's K = 32) is a template argument of the kernels: no run-time test of K is left in
// them.  Zeros past K add nothing: fmaf(0, 0, a) = a for every a these sums can hold (a starts at +0 and is never -0).
template <bool FULL>
__device__ __forceinline__ void emb_load16(const float* __restrict__ xr, int krem, float* xs) {
    if (FULL || krem >= 16) {
#pragma unroll
        for (int k = 0; k < 16; ++k) xs[k] = xr[k];
        return;
    }
#pragma unroll
    for (int k4 = 0; k4 < 16; k4 += 4) {
        if (k4 < krem) { xs[k4] = xr[k4]; xs[k4 + 1] = xr[k4 + 1]; xs[k4 + 2] = xr[k4 + 2]; xs[k4 + 3] = xr[k4 + 3]; }
        else { xs[k4] = 0.f; xs[k4 + 1] = 0.f; xs[k4 + 2] = 0.f; xs[k4 + 3] = 0.f; }
    }
}

// ------------------------------------------------------------------------------------------------ forward
// grid: (ceil(C / (64 CPT)), ceil(T / 16)) workgroups of 256 threads.  KP: K rounded up to 32 or 64; OH: x is half.
template <int KP, int CPT, bool OH, bool FULL>
__global__ __launch_bounds__(256) void embed_fwd_kernel(const void* __restrict__ label, int i64, const float* __restrict__ r, float rate, const long long* __restrict__ lvl,
                                                        const float* __restrict__ xv, long long xbs, long long xrs, const float* __restrict__ class_emb,
                                                        const float* __restrict__ pos_start, const float* __restrict__ W, const float* __restrict__ bias,
                                                        const float* __restrict__ lvl_emb, const float* __restrict__ pos, void* __restrict__ x, int bf,
                                                        float* __restrict__ cond, int B, int T, int first_l, int C, int K, int S, int NC1) {
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c0 = (blockIdx.x * 64 + lane) * CPT;          // C % 4 == 0: a lane's columns are all inside or all outside
    if (c0 >= C) return;                                     // no barrier in this kernel
    const int l0 = blockIdx.y * EMB_FWD_TOK, l1 = min(T, l0 + EMB_FWD_TOK);
    float wr[CPT][KP], bv[CPT];
#pragma unroll
    for (int cc = 0; cc < CPT; ++cc) {
        bv[cc] = 0.f;
#pragma unroll
        for (int k = 0; k < KP; ++k) wr[cc][k] = 0.f;
    }
    if (l1 > first_l) {          // the workgroup has word rows: the lane's rows of W stay in registers for all of them
        emb_load<CPT>(bias, c0, bv);
#pragma unroll
        for (int cc = 0; cc < CPT; ++cc)
#pragma unroll
            for (int k4 = 0; k4 < KP; k4 += 4)
                if (FULL || k4 < K) {
                    const f32x4 w = *reinterpret_cast<const f32x4*>(W + (size_t)(c0 + cc) * K + k4);
                    wr[cc][k4] = w[0]; wr[cc][k4 + 1] = w[1]; wr[cc][k4 + 2] = w[2]; wr[cc][k4 + 3] = w[3];
                }
    }
#pragma unroll 1
    for (int l = l0 + wv; l < l1; l += 4) {
        const long long lv = lvl[l];
        float e[CPT];
        if (lv >= 0 && lv < S) {
            float a[CPT], p[CPT];
            emb_load<CPT>(lvl_emb, (size_t)lv * C + c0, a);
            emb_load<CPT>(pos, (size_t)l * C + c0, p);
#pragma unroll
            for (int cc = 0; cc < CPT; ++cc) e[cc] = a[cc] + p[cc];
        } else {
#pragma unroll
            for (int cc = 0; cc < CPT; ++cc) e[cc] = emb_nan();          // a level outside [0, S): nothing is gathered, the token's rows are NaN
        }
        if (l < first_l) {
            float ps[CPT];
            emb_load<CPT>(pos_start, (size_t)l * C + c0, ps);
#pragma unroll 1
            for (int b = 0; b < B; ++b) {
                const int j = emb_label(label, i64, r, rate, b, NC1);
                float cv[CPT], o[CPT];
                if (j >= 0) emb_load<CPT>(class_emb, (size_t)j * C + c0, cv);
                else {
#pragma unroll
                    for (int cc = 0; cc < CPT; ++cc) cv[cc] = emb_nan();          // a label outside [0, NC1)
                }
#pragma unroll
                for (int cc = 0; cc < CPT; ++cc) o[cc] = (cv[cc] + ps[cc]) + e[cc];
                emb_store_x<CPT, OH>(x, ((size_t)b * T + l) * C + c0, bf != 0, o);
                if (l == 0) emb_store<CPT>(cond, (size_t)b * C + c0, cv);
            }
        } else {
            const float* __restrict__ xr0 = xv + (size_t)(l - first_l) * (size_t)xrs;          // wave-uniform: scalar loads
            float xa[16], xb[16];
            emb_load16<FULL>(xr0, K, xa);
#pragma unroll 1
            for (int b = 0; b < B; ++b) {
                const float* __restrict__ xr = xr0 + (size_t)b * (size_t)xbs;
                float a[CPT], o[CPT];
#pragma unroll
                for (int cc = 0; cc < CPT; ++cc) a[cc] = 0.f;
#pragma unroll
                for (int ch = 0; ch < KP / 16; ch += 2) {
                    emb_load16<FULL>(xr + 16 * (ch + 1), K - 16 * (ch + 1), xb);          // in flight under the arithmetic below
#pragma unroll
                    for (int k = 0; k < 16; ++k)
#pragma unroll
                        for (int cc = 0; cc < CPT; ++cc) a[cc] = __builtin_fmaf(xa[k], wr[cc][16 * ch + k], a[cc]);
                    if (ch + 2 < KP / 16) emb_load16<FULL>(xr + 16 * (ch + 2), K - 16 * (ch + 2), xa);
                    else if (b + 1 < B) emb_load16<FULL>(xr + (size_t)xbs, K, xa);
#pragma unroll
                    for (int k = 0; k < 16; ++k)
#pragma unroll
                        for (int cc = 0; cc < CPT; ++cc) a[cc] = __builtin_fmaf(xb[k], wr[cc][16 * (ch + 1) + k], a[cc]);
                }
#pragma unroll
                for (int cc = 0; cc < CPT; ++cc) o[cc] = (a[cc] + bv[cc]) + e[cc];
                emb_store_x<CPT, OH>(x, ((size_t)b * T + l) * C + c0, bf != 0, o);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ backward, pass 1
// grid: (ceil(C / (64 CPT)), chunks of 8 tokens: over [0, L) when dpos is asked for - its rows l >= T are zeros - else over [0, T)).  GH: g is half; DW: dW's partial sums.
template <int KP, int CPT, bool GH, bool DW, bool FULL>
__global__ __launch_bounds__(256) void embed_bwd_kernel(const void* __restrict__ g, int bf, const float* __restrict__ xv, long long xbs, long long xrs,
                                                        float* __restrict__ dpos, float* __restrict__ dpos_start, float* __restrict__ wsP, float* __restrict__ wsW, int B, int T,
                                                        int L, int first_l, int C, int K, int nchunkT) {
    __shared__ float red[DW ? CPT * KP * 64 : 1];          // [value][lane]: conflict-free words
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c0 = (blockIdx.x * 64 + lane) * CPT;
    const bool live = c0 < C;
    const int chunk = blockIdx.y, l0 = chunk * EMB_BWD_TOK, l1 = min(dpos ? L : T, l0 + EMB_BWD_TOK);
    float dwa[DW ? CPT : 1][DW ? KP : 1];
    if (DW) {
#pragma unroll
        for (int cc = 0; cc < CPT; ++cc)
#pragma unroll
            for (int k = 0; k < KP; ++k) dwa[cc][k] = 0.f;
    }
#pragma unroll 1
    for (int l = l0 + wv; l < l1; l += 4) {
        if (!live) break;
        float p[CPT];
#pragma unroll
        for (int cc = 0; cc < CPT; ++cc) p[cc] = 0.f;
        if (l >= T) {          // only with dpos: the zero tail
            emb_store<CPT>(dpos, (size_t)l * C + c0, p);
            continue;
        }
        const bool word = DW && l >= first_l;
        const float* __restrict__ xr0 = word ? xv + (size_t)(l - first_l) * (size_t)xrs : nullptr;          // wave-uniform: scalar loads
        float gn[CPT], xa[16], xb[16];
        emb_load_x<CPT, GH>(g, (size_t)l * C + c0, bf != 0, gn);
        if (DW && word) emb_load16<FULL>(xr0, K, xa);
#pragma unroll 1
        for (int b = 0; b < B; ++b) {
            float gv[CPT];
#pragma unroll
            for (int cc = 0; cc < CPT; ++cc) gv[cc] = gn[cc];
            if (b + 1 < B) emb_load_x<CPT, GH>(g, ((size_t)(b + 1) * T + l) * C + c0, bf != 0, gn);          // in flight under the arithmetic below
#pragma unroll
            for (int cc = 0; cc < CPT; ++cc) p[cc] += gv[cc];
            if (DW && word) {
                const float* __restrict__ xr = xr0 + (size_t)b * (size_t)xbs;
#pragma unroll
                for (int ch = 0; ch < KP / 16; ch += 2) {          // a column past K holds 0 + g 0 and is never stored
                    emb_load16<FULL>(xr + 16 * (ch + 1), K - 16 * (ch + 1), xb);
#pragma unroll
                    for (int k = 0; k < 16; ++k)
#pragma unroll
                        for (int cc = 0; cc < CPT; ++cc) dwa[cc][16 * ch + k] = __builtin_fmaf(gv[cc], xa[k], dwa[cc][16 * ch + k]);
                    if (ch + 2 < KP / 16) emb_load16<FULL>(xr + 16 * (ch + 2), K - 16 * (ch + 2), xa);
                    else if (b + 1 < B) emb_load16<FULL>(xr + (size_t)xbs, K, xa);
#pragma unroll
                    for (int k = 0; k < 16; ++k)
#pragma unroll
                        for (int cc = 0; cc < CPT; ++cc) dwa[cc][16 * (ch + 1) + k] = __builtin_fmaf(gv[cc], xb[k], dwa[cc][16 * (ch + 1) + k]);
                }
            }
        }
        emb_store<CPT>(wsP, (size_t)l * C + c0, p);
        if (dpos) emb_store<CPT>(dpos, (size_t)l * C + c0, p);
        if (dpos_start && l < first_l) emb_store<CPT>(dpos_start, (size_t)l * C + c0, p);
    }
    if (DW && chunk < nchunkT) {          // the same in every thread of the workgroup: the barriers inside are met by all
        // ((w0 + w1) + w2) + w3 through LDS: a lane of every wave owns the same (c, k).  A wave without a token and a lane past C add the zeros they started with.
#pragma unroll 1
        for (int v = 0; v < 4; ++v) {
            __syncthreads();
            if (wv != v) continue;
            if (v > 0) {
#pragma unroll
                for (int cc = 0; cc < CPT; ++cc)
#pragma unroll
                    for (int k = 0; k < KP; ++k) dwa[cc][k] = red[(cc * KP + k) * 64 + lane] + dwa[cc][k];
            }
            if (v < 3) {
#pragma unroll
                for (int cc = 0; cc < CPT; ++cc)
#pragma unroll
                    for (int k = 0; k < KP; ++k) red[(cc * KP + k) * 64 + lane] = dwa[cc][k];
            }
        }
        if (wv == 3 && live) {
            float* __restrict__ dst = wsW + ((size_t)chunk * C + c0) * (size_t)K;
#pragma unroll
            for (int cc = 0; cc < CPT; ++cc)
#pragma unroll
                for (int k4 = 0; k4 < KP; k4 += 4)
                    if (FULL || k4 < K) *reinterpret_cast<f32x4*>(dst + (size_t)cc * K + k4) = f32x4{dwa[cc][k4], dwa[cc][k4 + 1], dwa[cc][k4 + 2], dwa[cc][k4 + 3]};
        }
    }
}

// ------------------------------------------------------------------------------------------------ backward, pass 2
// out[q] = sum over the nparts parts of parts[n][q], q a float4 of n4 per part.  grid ceil(n4 / 64), 256 threads = 64 float4 x 4 slices.
__global__ __launch_bounds__(256) void embed_sum_parts_kernel(const float* __restrict__ parts, int nparts, long long n4, float* __restrict__ out) {
    __shared__ f32x4 red[4][64];
    const int qx = threadIdx.x & 63, sl = threadIdx.x >> 6;
    const long long q = (long long)blockIdx.x * 64 + qx;
    const bool live = q < n4;
    f32x4 a = {0.f, 0.f, 0.f, 0.f};
    if (live) {
        const f32x4* p = reinterpret_cast<const f32x4*>(parts) + q;
#pragma unroll 4
        for (int n = sl; n < nparts; n += 4) a += p[(size_t)n * (size_t)n4];
    }
    red[sl][qx] = a;
    __syncthreads();
    if (sl == 0 && live) reinterpret_cast<f32x4*>(out)[q] = ((red[0][qx] + red[1][qx]) + red[2][qx]) + red[3][qx];
}

// row y < S: dlvl[y][c] = sum of p[l][c] over the tokens l < T of stage y; row y == S: dbias[c] = sum over first_l <= l < T.  grid (ceil(C / 64), S + 1), 256 threads = 64
// columns x 4 slices; slice s walks the tokens s, s + 4, .. in index order.  Which tokens qualify is staged in LDS 256 tokens at a time (one per thread), and a token
// that does not qualify adds +0.0f - the sum starts at +0.0f and can never be -0, so that changes no bit - which leaves the loads of p free of branches and in flight
// several at a time.  A stage no token reaches and a dbias without word rows are sums of nothing: +0.0f.
__global__ __launch_bounds__(256) void embed_rows_kernel(const float* __restrict__ wsP, const long long* __restrict__ lvl, float* __restrict__ dlvl, float* __restrict__ dbias,
                                                         int T, int first_l, int C, int S) {
    __shared__ float red[4][64];
    __shared__ int take[256];
    const int cx = threadIdx.x & 63, sl = threadIdx.x >> 6, c = blockIdx.x * 64 + cx, y = blockIdx.y;
    float* __restrict__ out = y < S ? (dlvl ? dlvl + (size_t)y * C : nullptr) : dbias;
    if (!out) return;          // the same in every thread of the workgroup
    const int cc = min(c, C - 1);          // a column past C reads a valid address and stores nothing
    float acc = 0.f;
#pragma unroll 1
    for (int l0 = 0; l0 < T; l0 += 256) {
        __syncthreads();          // the walk over the previous 256 tokens is over
        const int l = l0 + (int)threadIdx.x;
        if (l < T) take[threadIdx.x] = y < S ? (lvl[l] == (long long)y) : (l >= first_l);
        __syncthreads();
        const int n = min(256, T - l0);
#pragma unroll 4
        for (int i = sl; i < n; i += 4) {          // 256 % 4 == 0: token l0 + i is one of the slice's own
            const float v = wsP[(size_t)(l0 + i) * C + cc];
            acc += take[i] ? v : 0.f;
        }
    }
    red[sl][cx] = acc;
    __syncthreads();
    if (sl == 0 && c < C) out[c] = ((red[0][cx] + red[1][cx]) + red[2][cx]) + red[3][cx];
}

// dclass[j][c] = sum over the images b with j_b = j, b ascending from 0.0f, of (gc[b][c] + t_b[c]), t_b = sum_{l < first_l} g[b][l][c], l ascending from 0.0f (gc NULL: t_b;
// g NULL: gc[b][c]).  grid (ceil(C / 1024), ceil(NC1 / 16)), 256 threads x 4 columns.  A workgroup owns 16 rows of dclass: it writes them as zeros, then walks the images
// once - their effective labels staged 256 at a time in LDS, one per thread, so that the walk does not wait for a load per image - and adds an image that selects one of
// its rows into that row in memory: the lane that owns the columns reads what it wrote itself, in program order.  Every row of dclass is written.
template <bool GH>
__global__ __launch_bounds__(256) void embed_dclass_kernel(const void* __restrict__ g, int bf, const float* __restrict__ gc, const void* __restrict__ label, int i64,
                                                           const float* __restrict__ r, float rate, float* dclass, int B, int T, int first_l, int C, int NC1) {
    __shared__ int sJ[256];
    const int c0 = (blockIdx.x * 256 + threadIdx.x) * 4;
    const bool live = c0 < C;
    const int j0 = blockIdx.y * EMB_CLS_SLAB, j1 = min(NC1, j0 + EMB_CLS_SLAB);
    if (live) {
        const float z[4] = {0.f, 0.f, 0.f, 0.f};
        for (int j = j0; j < j1; ++j) emb_store<4>(dclass, (size_t)j * C + c0, z);
    }
#pragma unroll 1
    for (int bb = 0; bb < B; bb += 256) {
        __syncthreads();          // the walk over the previous 256 labels is over
        if (bb + (int)threadIdx.x < B) sJ[threadIdx.x] = emb_label(label, i64, r, rate, bb + (int)threadIdx.x, NC1);
        __syncthreads();
        const int n = min(256, B - bb);
        if (!live) continue;
#pragma unroll 1
        for (int i = 0; i < n; ++i) {
            const int j = sJ[i], b = bb + i;          // one address for the whole workgroup: a broadcast
            if (j < j0 || j >= j1) continue;
            float t[4] = {0.f, 0.f, 0.f, 0.f}, acc[4];
            if (g) {
#pragma unroll 1
                for (int l = 0; l < first_l; ++l) {
                    float gv[4];
                    emb_load_x<4, GH>(g, ((size_t)b * T + l) * C + c0, bf != 0, gv);
#pragma unroll
                    for (int e = 0; e < 4; ++e) t[e] += gv[e];
                }
            }
            if (gc) {
                float cv[4];
                emb_load<4>(gc, (size_t)b * C + c0, cv);
#pragma unroll
                for (int e = 0; e < 4; ++e) t[e] = g ? cv[e] + t[e] : cv[e];
            }
            emb_load<4>(dclass, (size_t)j * C + c0, acc);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] += t[e];
            emb_store<4>(dclass, (size_t)j * C + c0, acc);
        }
    }
}

// dxv[b][t][k] = sum_c g[b][t + first_l][c] W[c][k] for t < T - first_l, zeros for the other rows of xv.  One wave per row of dxv (B x xv_rows of them).
template <int KP, bool GH>
__global__ __launch_bounds__(256) void embed_dxv_kernel(const void* __restrict__ g, int bf, const float* __restrict__ W, float* __restrict__ dxv, int rows, int xv_rows, int T,
                                                        int first_l, int C, int K) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (row >= rows) return;
    const int b = row / xv_rows, t = row - b * xv_rows;
    float acc[KP];
#pragma unroll
    for (int k = 0; k < KP; ++k) acc[k] = 0.f;
    if (t < T - first_l) {
        const size_t go = ((size_t)b * T + t + first_l) * (size_t)C;
#pragma unroll 1
        for (int c = 4 * lane; c < C; c += 256) {
            float gv[4];
            emb_load_x<4, GH>(g, go + c, bf != 0, gv);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int k4 = 0; k4 < KP; k4 += 4)
                    if (k4 < K) {
                        const f32x4 w = *reinterpret_cast<const f32x4*>(W + (size_t)(c + e) * K + k4);
                        acc[k4] = __builtin_fmaf(gv[e], w[0], acc[k4]); acc[k4 + 1] = __builtin_fmaf(gv[e], w[1], acc[k4 + 1]);
                        acc[k4 + 2] = __builtin_fmaf(gv[e], w[2], acc[k4 + 2]); acc[k4 + 3] = __builtin_fmaf(gv[e], w[3], acc[k4 + 3]);
                    }
        }
    }
    float mine = 0.f;          // lane k keeps the sum of column k
#pragma unroll
    for (int k = 0; k < KP; ++k) {
        const float s = wave_sum(acc[k]);
        if (lane == k) mine = s;
    }
    if (lane < K) dxv[(size_t)row * K + lane] = mine;
}

// ------------------------------------------------------------------------------------------------ host side
static inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static inline int bwd_chunks(int n) { return (n + EMB_BWD_TOK - 1) / EMB_BWD_TOK; }

static int check_shape(const char* who, int B, int T, int C, int K) {
    SDVAR_CHECK_ARG(C >= 4 && C <= EMB_MAX_C && C % 4 == 0, "%s: C=%d must be a multiple of 4 in [4, %d]", who, C, EMB_MAX_C);
    SDVAR_CHECK_ARG(K >= 4 && K <= EMB_MAX_K && K % 4 == 0, "%s: K=%d must be a multiple of 4 in [4, %d]", who, K, EMB_MAX_K);
    SDVAR_CHECK_ARG(B >= 1 && T >= 1 && (long long)B * T <= (1ll << 29), "%s: B=%d, T=%d: both must be at least 1 and B * T at most 2^29", who, B, T);
    return SDVAR_OK;
}
static int check_tokens(const char* who, int T, int L, int first_l, int S, int NC1) {
    SDVAR_CHECK_ARG(first_l >= 1 && first_l <= T && T <= L && L <= (1 << 19), "%s: first_l=%d, T=%d, L=%d: 1 <= first_l <= T <= L <= 2^19", who, first_l, T, L);
    SDVAR_CHECK_ARG(S >= 1 && NC1 >= 1, "%s: S=%d stages and NC1=%d rows of class_emb: both must be at least 1", who, S, NC1);
    return SDVAR_OK;
}
static int check_xv(const char* who, const float* xv, long long xbs, long long xrs, int B, int T, int first_l, int K) {
    if (T == first_l) return SDVAR_OK;          // no word rows: xv is not read
    SDVAR_CHECK_ARG(xv && al16(xv), "%s: xv must be given (T > first_l) and 16-byte aligned", who);
    SDVAR_CHECK_ARG(xrs >= K && xrs % 4 == 0 && xbs >= 0 && xbs % 4 == 0 && (B == 1 || xbs >= (long long)(T - first_l - 1) * xrs + K),
                    "%s: xv strides (batch %lld, row %lld): multiples of 4 elements, a row stride of at least K=%d, a batch stride that holds the %d rows used", who, xbs, xrs, K,
                    T - first_l);
    return SDVAR_OK;
}

long long embed_bwd_ws_bytes(int B, int T, int C, int K) {
    if (check_shape("embed_bwd_ws_bytes", B, T, C, K)) return -1;
    return ((long long)T * C + (long long)bwd_chunks(T) * C * K) * (long long)sizeof(float);
}

template <typename F>
static inline void with_k(int K, F f) {
    if (K <= 32) f(std::integral_constant<int, 32>{}, std::integral_constant<int, 4>{});
    else f(std::integral_constant<int, 64>{}, std::integral_constant<int, 2>{});
}
template <typename F>
static inline void with_flag(bool v, F f) {
    if (v) f(std::true_type{}); else f(std::false_type{});
}

int embed_fwd(const void* label, int i64, const float* r, double rate, const long long* lvl, const float* xv, long long xbs, long long xrs, const float* class_emb,
              const float* pos_start, const float* W, const float* bias, const float* lvl_emb, const float* pos, void* x, int xdt, float* cond, int B, int T, int L, int first_l,
              int C, int K, int S, int NC1, hipStream_t stream) {
    const char* who = "embed_fwd";
    if (int rc = check_shape(who, B, T, C, K)) return rc;
    if (int rc = check_tokens(who, T, L, first_l, S, NC1)) return rc;
    SDVAR_CHECK_ARG(xdt >= 0 && xdt <= 2, "%s: x_dtype=%d (0 fp32, 1 fp16, 2 bf16)", who, xdt);
    SDVAR_CHECK_ARG(label && lvl && class_emb && pos_start && W && bias && lvl_emb && pos && x && cond,
                    "%s: null label, lvl, class_emb, pos_start, W, bias, lvl_emb, pos_1LC, x or cond", who);
    SDVAR_CHECK_ARG(al16(label) && al16(r) && al16(lvl) && al16(class_emb) && al16(pos_start) && al16(W) && al16(bias) && al16(lvl_emb) && al16(pos) && al16(x) && al16(cond),
                    "%s: every pointer must be 16-byte aligned", who);
    if (int rc = check_xv(who, xv, xbs, xrs, B, T, first_l, K)) return rc;
    with_k(K, [&](auto kp, auto cpt) { with_flag(xdt != 0, [&](auto oh) { with_flag(K == decltype(kp)::value, [&](auto full) {
        constexpr int KP = decltype(kp)::value, CPT = decltype(cpt)::value;
        const dim3 grid((unsigned)((C + 64 * CPT - 1) / (64 * CPT)), (unsigned)((T + EMB_FWD_TOK - 1) / EMB_FWD_TOK));
        hipLaunchKernelGGL((embed_fwd_kernel<KP, CPT, decltype(oh)::value, decltype(full)::value>), grid, dim3(256), 0, stream, label, i64, r, (float)rate, lvl, xv, xbs, xrs, class_emb, pos_start, W,
                           bias, lvl_emb, pos, x, xdt == 2 ? 1 : 0, cond, B, T, first_l, C, K, S, NC1);
    }); }); });
    SDVAR_LAUNCH_CHECK();
    return SDVAR_OK;
}

int embed_bwd(const void* g, int gdt, const float* gc, const void* label, int i64, const float* r, double rate, const long long* lvl, const float* xv, long long xbs,
              long long xrs, const float* W, float* dpos, float* dpos_start, float* dlvl, float* dclass, float* dbias, float* dW, float* dxv, int xv_rows, float* ws, int B, int T,
              int L, int first_l, int C, int K, int S, int NC1, hipStream_t stream) {
    const char* who = "embed_bwd";
    if (int rc = check_shape(who, B, T, C, K)) return rc;
    if (int rc = check_tokens(who, T, L, first_l, S, NC1)) return rc;
    SDVAR_CHECK_ARG(gdt >= 0 && gdt <= 2, "%s: g_dtype=%d (0 fp32, 1 fp16, 2 bf16)", who, gdt);
    SDVAR_CHECK_ARG(dpos || dpos_start || dlvl || dclass || dbias || dW || dxv, "%s: no output asked for (every output pointer is null)", who);
    SDVAR_CHECK_ARG(al16(g) && al16(gc) && al16(label) && al16(r) && al16(lvl) && al16(W) && al16(dpos) && al16(dpos_start) && al16(dlvl) && al16(dclass) && al16(dbias) &&
                        al16(dW) && al16(dxv) && al16(ws),
                    "%s: every pointer must be 16-byte aligned", who);
    SDVAR_CHECK_ARG(!dclass || (label && (g || gc)), "%s: dclass needs label and at least one of g and gc", who);
    SDVAR_CHECK_ARG(!dlvl || lvl, "%s: dlvl needs lvl", who);
    const bool cols = dpos || dpos_start || dlvl || dbias || dW;          // what pass 1 serves
    SDVAR_CHECK_ARG(!(cols && g) || ws, "%s: dpos_1LC, dpos_start, dlvl, dbias and dW need the workspace (sdvar_op_embed_bwd_ws_bytes)", who);
    SDVAR_CHECK_ARG(!dxv || (xv_rows >= T - first_l && xv_rows >= 1 && (long long)B * xv_rows <= (1ll << 29)), "%s: xv_rows=%d must hold the %d rows used (B * xv_rows <= 2^29)",
                    who, xv_rows, T - first_l);
    SDVAR_CHECK_ARG(!(dxv && g) || W, "%s: dxv needs W", who);
    const bool words = T > first_l;
    if (dW && g && words) { if (int rc = check_xv(who, xv, xbs, xrs, B, T, first_l, K)) return rc; }
    const int bf = gdt == 2 ? 1 : 0;
    if (!g) {          // no gradient reached x: exact zeros, and dclass from gc alone
        if (dpos) SDVAR_HIP(hipMemsetAsync(dpos, 0, (size_t)L * C * sizeof(float), stream));
        if (dpos_start) SDVAR_HIP(hipMemsetAsync(dpos_start, 0, (size_t)first_l * C * sizeof(float), stream));
        if (dlvl) SDVAR_HIP(hipMemsetAsync(dlvl, 0, (size_t)S * C * sizeof(float), stream));
        if (dbias) SDVAR_HIP(hipMemsetAsync(dbias, 0, (size_t)C * sizeof(float), stream));
        if (dW) SDVAR_HIP(hipMemsetAsync(dW, 0, (size_t)C * K * sizeof(float), stream));
        if (dxv) SDVAR_HIP(hipMemsetAsync(dxv, 0, (size_t)B * xv_rows * K * sizeof(float), stream));
    } else {
        if (cols) {
            const int nchunkT = bwd_chunks(T);
            float* wsP = ws;
            float* wsW = ws + (size_t)T * C;
            const bool dw = dW && words;
            with_k(K, [&](auto kp, auto cpt) { with_flag(gdt != 0, [&](auto gh) { with_flag(dw, [&](auto dwf) { with_flag(K == decltype(kp)::value, [&](auto full) {
                constexpr int KP = decltype(kp)::value, CPT = decltype(cpt)::value;
                const dim3 grid((unsigned)((C + 64 * CPT - 1) / (64 * CPT)), (unsigned)(dpos ? bwd_chunks(L) : nchunkT));
                hipLaunchKernelGGL((embed_bwd_kernel<KP, CPT, decltype(gh)::value, decltype(dwf)::value, decltype(full)::value>), grid, dim3(256), 0, stream, g, bf, xv, xbs, xrs, dpos, dpos_start, wsP,
                                   wsW, B, T, L, first_l, C, K, nchunkT);
            }); }); }); });
            SDVAR_LAUNCH_CHECK();
            if (dW) {
                if (dw) {
                    const long long n4 = (long long)C * K / 4;
                    hipLaunchKernelGGL(embed_sum_parts_kernel, dim3((unsigned)((n4 + 63) / 64)), dim3(256), 0, stream, wsW, nchunkT, n4, dW);
                    SDVAR_LAUNCH_CHECK();
                } else {
                    SDVAR_HIP(hipMemsetAsync(dW, 0, (size_t)C * K * sizeof(float), stream));
                }
            }
            if (dlvl || dbias) {
                hipLaunchKernelGGL(embed_rows_kernel, dim3((unsigned)((C + 63) / 64), (unsigned)(S + 1)), dim3(256), 0, stream, wsP, lvl, dlvl, dbias, T, first_l, C, S);
                SDVAR_LAUNCH_CHECK();
            }
        }
        if (dxv) {
            const int rows = B * xv_rows;
            with_flag(K > 32, [&](auto wide) { with_flag(gdt != 0, [&](auto gh) {
                hipLaunchKernelGGL((embed_dxv_kernel<decltype(wide)::value ? 64 : 32, decltype(gh)::value>), dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, g, bf, W, dxv,
                                   rows, xv_rows, T, first_l, C, K);
            }); });
            SDVAR_LAUNCH_CHECK();
        }
    }
    if (dclass) {
        const dim3 grid((unsigned)((C + 1023) / 1024), (unsigned)((NC1 + EMB_CLS_SLAB - 1) / EMB_CLS_SLAB));
        with_flag(gdt != 0, [&](auto gh) {
            hipLaunchKernelGGL((embed_dclass_kernel<decltype(gh)::value>), grid, dim3(256), 0, stream, g, bf, gc, label, i64, r, (float)rate, dclass, B, T, first_l, C, NC1);
        });
        SDVAR_LAUNCH_CHECK();
    }
    return SDVAR_OK;
}

}  // namespace sdvar
