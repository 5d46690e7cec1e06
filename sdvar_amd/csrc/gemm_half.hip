// Plain half-precision "NT" GEMM on the gfx950 matrix cores, for the FFN of a model run under torch.autocast (seam.fused_mlp_func_amp / _amp_grad):
//     out[M,N] = epilogue( X[M,K] . W[N,K]^T + bias[N] ),   X, W fp16 or bf16 (one dtype per call), fp32 accumulation, fp32 bias
// ONE plane per operand, K-blocked [K/32][rows][32] (common.h kb_index) - the f16x2 operand of gemm_f16x2.hip without its low plane - and ONE
// v_mfma_f32_32x32x16_f16 / _bf16 per (32 x 32 tile, k16 step) where the f16x2 GEMM issues three.  Nothing is scaled or clamped: an fp16 overflow is +-inf in
// the result, which a GradScaler has to see.
//
// Kernel: gemm_f16x2_v2_kernel's plain ring with the low-plane DMA and two of its three MFMAs removed.  128 x 128 tile, 8 waves (2 x 4, 64 x 32 outputs each),
// K-steps of 32 streamed global -> LDS by the LDS-DMA, one raw s_barrier per K-step, counted vmcnt waits, transposed accumulators (lane = output row, so a lane
// owns four consecutive columns per register group).
//   stage (16 KB) = 2 sub-arrays [128 rows][64 B]: X then W; unpadded rows, the 16-byte chunk c of row r is stored at chunk c ^ ((r >> 2) & 3) (applied on the
//   DMA source address and on the ds_read address), as in the f16x2 kernel.  Every wave issues 2 DMA instructions per K-step (rows 16 w .. 16 w + 15 of X, of W).
//   Ring: a K-step is 4 MFMAs per wave (128 matrix-pipe cycles; 512 per SIMD and K-step with the 4 waves two resident workgroups put on it), a third of the
//   f16x2 kernel's, while the latency of a DMA is what it was.  The f16x2 ring keeps 2 K-steps in flight behind 3 x the matrix work; to cover the same time the
//   ring here is NS = 4 stages (64 KB, two workgroups per CU) with 3 K-steps = 6 DMA instructions per wave in flight: K-step t has landed when at most
//   2 * min(2, K-steps behind it) instructions are outstanding (vmcnt 4 / 2 / 0).  A deeper ring would cost the second resident workgroup (5 x 16 KB x 2 is the
//   whole LDS), which hides the barrier and the epilogue.
// Edge rows are clamped on load (row min(m, M - 1)) and never stored; N % 8 == 0 makes every 4-column register group lie inside or outside N as a whole.  No
// split-K, no atomics: repeats are bit-identical, and an output element's value does not depend on M, N or the tile it falls into (each element is one fp32
// MFMA chain over k in ascending order).
//
// The engine's GEMM mode f16 (api.hip plane_gemm) launches the same kernel on the HIGH planes of f16x2 operands - plane 0 of an activation is fp16(clamp(x)), of a
// weight fp16(w 2^S), both in this layout: the EX instances (gemm_half_ex, sdvar_op_gemm_h_ex; fp16 only) multiply the fp32 sum by the weight's 2^-S before the bias,
// saturate the GELU's pre-activation at +-65504 like every f16x2 producer, and add the gated-residual epilogue.  The seam's instances (EX = false) are unchanged.
#include "../../include/sdvar_hip.h"
#include "common.h"

namespace sdvar {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) void* lds_ptr_t;

enum { GH_EPI_BIAS = 0, GH_EPI_GELU = 1, GH_EPI_GATED_RES = 2 };
constexpr int GH_BM = 128, GH_BN = 128, GH_BK = 32, GH_NS = 4;
constexpr int GH_STAGE = 2 * 128 * 32;          // half elements per stage (16 KB)
#define SDVAR_GH_RD(dst, addr, off) asm volatile("ds_read_b128 %0, %1 offset:" #off : "=v"(dst) : "v"(addr) : "memory")

struct GemmHalfArgs {
    const uint16_t* X; const uint16_t* W;        // K-blocked [K/32][M][32], [K/32][N][32]
    const float* bias;                           // (N) fp32 or null
    void* out; int out_half; int ldo;            // GH_EPI_BIAS: row-major fp32 or half
    uint16_t* h_out; uint16_t* p_out;            // GH_EPI_GELU: h as the K-blocked (M x N) operand; p row-major (M, N) or null
    int M, N, K;
    // the engine's tier (EX kernels, sdvar_op_gemm_h_ex; fp16 only): v = acc * *scale + bias in every epilogue, and
    const float* scale;                          // device scalar (the 2^-S of an f16x2 weight's high plane) or null = 1
    const float* res; int ldres;                 // GH_EPI_GATED_RES: out = res + v * gate[(m / rows_per_gate) * gate_stride + n], all fp32; res may be out
    const float* gate; int rows_per_gate, gate_stride;
};

template <bool BF16>
__device__ __forceinline__ f32x16 gh_mfma(const f16x8& a, const f16x8& b, const f32x16& c) {
    if (BF16) return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}

// One 32 x 32 accumulator tile (transposed layout): this lane's row m, columns nb + 8 g + {0..3} for g = 0..3 (nb already holds the lane half's + 4 lh).
// EX (the engine's tier): sc = *a.scale multiplies the fp32 sum before the bias (a power of two, so the fused form rounds like mul + add), the GELU's
// pre-activation saturates at the fp16 range like every other f16x2 operand producer (split2h), and GH_EPI_GATED_RES exists.
template <bool BF16, int EPI, bool EX>
__device__ __forceinline__ void gh_store_tile(const GemmHalfArgs& a, const f32x16& acc, float sc, int m, int nb) {
    if (m >= a.M) return;
    const size_t grow = (EPI == GH_EPI_GATED_RES) ? (size_t)(m / a.rows_per_gate) * a.gate_stride : 0;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int n = nb + 8 * g;
        if (n >= a.N) continue;                  // N % 8 == 0 and n % 4 == 0: the four columns are inside together
        f32x4 v = {acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]};
        if (EX) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] *= sc;
        }
        if (a.bias) {
            const f32x4 bv = *reinterpret_cast<const f32x4*>(a.bias + n);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] += bv[e];
        }
        if (EPI == GH_EPI_GATED_RES) {           // each lane reads its four residuals before it writes them: res == out is fine
            const f32x4 rv = *reinterpret_cast<const f32x4*>(a.res + (size_t)m * a.ldres + n);
            const f32x4 gv = *reinterpret_cast<const f32x4*>(a.gate + grow + n);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = rv[e] + v[e] * gv[e];
            *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(a.out) + (size_t)m * a.ldo + n) = v;
        } else if (EPI == GH_EPI_GELU) {
            if (EX) {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = clamp_f16_range(v[e]);
            }
            uint2 p;                             // p = half(acc + b1); h = half(gelu_tanh(float(p)))
            p.x = half_pack2(v[0], v[1], BF16); p.y = half_pack2(v[2], v[3], BF16);
            if (a.p_out) *reinterpret_cast<uint2*>(a.p_out + (size_t)m * a.N + n) = p;
            uint2 h;
            h.x = half_pack2(gelu_tanh_h(half_lo(p.x, BF16)), gelu_tanh_h(half_hi(p.x, BF16)), BF16);
            h.y = half_pack2(gelu_tanh_h(half_lo(p.y, BF16)), gelu_tanh_h(half_hi(p.y, BF16)), BF16);
            *reinterpret_cast<uint2*>(a.h_out + kb_index(m, n, a.M)) = h;
        } else if (a.out_half) {
            uint2 o;
            o.x = half_pack2(v[0], v[1], BF16); o.y = half_pack2(v[2], v[3], BF16);
            *reinterpret_cast<uint2*>(reinterpret_cast<uint16_t*>(a.out) + (size_t)m * a.ldo + n) = o;
        } else {
            *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(a.out) + (size_t)m * a.ldo + n) = v;
        }
    }
}

template <bool BF16, int EPI, bool EX>
__global__ __launch_bounds__(512, 2) void gemm_half_kernel(GemmHalfArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint16_t ghsm[];
    constexpr int NS = GH_NS;
    const int tiles_m = (a.M + GH_BM - 1) / GH_BM, tiles_n = (a.N + GH_BN - 1) / GH_BN, ntile = tiles_m * tiles_n;
    const int lid = xcd_remap(blockIdx.x, ntile);
    const int G = 8, per_group = tiles_m * G;               // column panels of 8 tiles: the row tiles of a panel share its weight slices in L2
    const int g = lid / per_group, rem = lid - g * per_group;
    const int gw = min(G, tiles_n - g * G);
    const int tm = rem / gw, tn = g * G + rem % gw;
    const int m0 = tm * GH_BM, n0 = tn * GH_BN;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 2, wn = wave & 3, li = lane & 31, lh = lane >> 5;

    const int drow = 16 * wave + (lane >> 2);
    const int dchunk = (lane & 3) ^ ((drow >> 2) & 3);
    const int xrow = min(m0 + drow, a.M - 1), wrow = min(n0 + drow, a.N - 1);   // clamped: rows past the edge are never stored
    const int nk = a.K / GH_BK;
    const int swave = __builtin_amdgcn_readfirstlane(wave);
    const uint32_t lx = (uint32_t)(xrow * 32 + 8 * dchunk) * 2u, lw = (uint32_t)(wrow * 32 + 8 * dchunk) * 2u;
    const char* const bx = reinterpret_cast<const char*>(a.X);
    const char* const bw = reinterpret_cast<const char*>(a.W);
    // DMA instruction q of K-step t -> stage t % NS: q = 0 is X, q = 1 is W
    auto issue_one = [&](int t, int q) {
        uint16_t* st = ghsm + (t % NS) * GH_STAGE + swave * 512;
        if (q) SDVAR_DMA16(lw, bw + (size_t)t * a.N * 64, SDVAR_LDS_ADDR(st + 4096));
        else SDVAR_DMA16(lx, bx + (size_t)t * a.M * 64, SDVAR_LDS_ADDR(st));
    };

    f32x16 acc[2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;

    // fragment read offsets (elements) inside a sub-array: row * 32 + 8 * ((2 s + lh) ^ ((li >> 2) & 3))
    const int sw = (li >> 2) & 3;
    const int offa0 = (wm * 64 + li) * 32, offb = (wn * 32 + li) * 32;
    const int ch0 = 8 * ((0 + lh) ^ sw), ch1 = 8 * ((2 + lh) ^ sw);

    for (int tt = 0; tt < NS - 1 && tt < nk; ++tt) { issue_one(tt, 0); issue_one(tt, 1); }
    for (int t = 0; t < nk; ++t) {
        // K-step t has landed when at most the min(NS - 2, K-steps behind it) newest K-steps (2 instructions each) are still in flight
        const int behind = min(NS - 2, nk - 1 - t);
        if (behind >= 2) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        else if (behind == 1) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();            // every wave's share of K-step t is in LDS, and every wave is done reading the stage of K-step t - 1 ...
        const bool pf = t + NS - 1 < nk;         // ... which K-step t + NS - 1 overwrites
        const uint32_t sb = (uint32_t)(uintptr_t)(lds_ptr_t)(ghsm + (t % NS) * GH_STAGE);
        const uint32_t aa0 = sb + 2 * (offa0 + ch0), aa1 = sb + 2 * (offa0 + ch1), ab0 = sb + 2 * (offb + ch0), ab1 = sb + 2 * (offb + ch1);
        // fa[s][row tile], fb[s]: second 32-row tile of X at +2048 bytes, W at +8192
        f16x8 fa[2][2], fb[2];
        SDVAR_GH_RD(fb[0], ab0, 8192); SDVAR_GH_RD(fa[0][0], aa0, 0); SDVAR_GH_RD(fa[0][1], aa0, 2048);
        SDVAR_GH_RD(fb[1], ab1, 8192); SDVAR_GH_RD(fa[1][0], aa1, 0); SDVAR_GH_RD(fa[1][1], aa1, 2048);
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            if (s == 0) asm volatile("s_waitcnt lgkmcnt(3)" ::: "memory");
            else asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < 2; ++i) acc[i] = gh_mfma<BF16>(fb[s], fa[s][i], acc[i]);          // W fragment = A operand: the accumulator holds out^T
            __builtin_amdgcn_sched_barrier(0);
            if (pf) issue_one(t + NS - 1, s);    // the 2 DMA instructions of the K-step NS - 1 ahead, one behind each MFMA pair
            __builtin_amdgcn_sched_barrier(0);
        }
    }

    const float sc = (EX && a.scale) ? *a.scale : 1.0f;
#pragma unroll
    for (int i = 0; i < 2; ++i) gh_store_tile<BF16, EPI, EX>(a, acc[i], sc, m0 + wm * 64 + i * 32 + li, n0 + wn * 32 + 4 * lh);
}

template <bool BF16, int EPI, bool EX>
static int gh_launch(const GemmHalfArgs& a, hipStream_t stream) {
    const long long ntile = (long long)((a.M + GH_BM - 1) / GH_BM) * ((a.N + GH_BN - 1) / GH_BN);
    SDVAR_CHECK_ARG(ntile <= 0x7fffffffLL, "gemm_h: too many tiles");
    hipLaunchKernelGGL((gemm_half_kernel<BF16, EPI, EX>), dim3((unsigned)ntile), dim3(512), (size_t)GH_NS * GH_STAGE * 2, stream, a);
    SDVAR_LAUNCH_CHECK();
    return SDVAR_OK;
}

int gemm_half(const void* x, const void* w, int dtype, const float* bias, void* out, int out_dtype, int ldo, void* h_out, void* p_out, int M, int N, int K, int epi,
              hipStream_t stream) {
    auto al16 = [](const void* q) { return ((uintptr_t)q % 16) == 0; };
    SDVAR_CHECK_ARG(dtype == 1 || dtype == 2, "gemm_h: dtype %d (1 = fp16, 2 = bf16)", dtype);
    SDVAR_CHECK_ARG(epi == GH_EPI_BIAS || epi == GH_EPI_GELU, "gemm_h: epilogue %d (0 = bias, 1 = bias + GELU -> operand)", epi);
    SDVAR_CHECK_ARG(x && w, "gemm_h: null operand");
    SDVAR_CHECK_ARG(M >= 1 && N >= 8 && N % 8 == 0 && K >= 32 && K % 32 == 0 && M <= (1 << 24) && N <= (1 << 24), "gemm_h: need M >= 1, N %% 8 == 0 and K %% 32 == 0 (M=%d N=%d K=%d)", M, N, K);
    SDVAR_CHECK_ARG(al16(x) && al16(w) && al16(bias) && al16(out) && al16(h_out) && al16(p_out), "gemm_h: operands must be 16-byte aligned");
    if (epi == GH_EPI_BIAS) {
        SDVAR_CHECK_ARG(out && !h_out && !p_out, "gemm_h: epilogue 0 writes `out` only");
        SDVAR_CHECK_ARG(out_dtype == 0 || out_dtype == dtype, "gemm_h: out_dtype %d (0 = fp32, or the operands' dtype %d)", out_dtype, dtype);
        SDVAR_CHECK_ARG(ldo >= N && ldo % 4 == 0, "gemm_h: need ldo >= N and ldo %% 4 == 0 (ldo=%d N=%d)", ldo, N);
    } else {
        SDVAR_CHECK_ARG(h_out && !out, "gemm_h: epilogue 1 writes h_out (and p_out on request), not `out`");
        SDVAR_CHECK_ARG(N % 32 == 0, "gemm_h: epilogue 1 writes the next GEMM's operand: N %% 32 == 0 (N=%d)", N);
    }
    const GemmHalfArgs a{reinterpret_cast<const uint16_t*>(x), reinterpret_cast<const uint16_t*>(w), bias, out, out_dtype != 0, ldo,
                         reinterpret_cast<uint16_t*>(h_out), reinterpret_cast<uint16_t*>(p_out), M, N, K, nullptr, nullptr, 0, nullptr, 1, 0};
    if (dtype == 2) return epi == GH_EPI_GELU ? gh_launch<true, GH_EPI_GELU, false>(a, stream) : gh_launch<true, GH_EPI_BIAS, false>(a, stream);
    return epi == GH_EPI_GELU ? gh_launch<false, GH_EPI_GELU, false>(a, stream) : gh_launch<false, GH_EPI_BIAS, false>(a, stream);
}

// The engine's tier (GEMM mode f16, api.hip plane_gemm) and sdvar_op_gemm_h_ex: fp16 operands, fp32 `out`, an optional per-tensor scale and the gated residual.
int gemm_half_ex(const void* x, const void* w, int dtype, const float* w_scale, const float* bias, float* out, int ldo, void* h_out, void* p_out, const float* res, int ldres,
                 const float* gate, int rows_per_gate, int gate_stride, int M, int N, int K, int epi, hipStream_t stream) {
    auto al16 = [](const void* q) { return ((uintptr_t)q % 16) == 0; };
    SDVAR_CHECK_ARG(dtype == 1, "gemm_h_ex: dtype %d (1 = fp16; bf16 has no engine tier)", dtype);
    SDVAR_CHECK_ARG(epi >= GH_EPI_BIAS && epi <= GH_EPI_GATED_RES, "gemm_h_ex: epilogue %d (0 = bias, 1 = bias + GELU -> operand, 2 = gated residual)", epi);
    SDVAR_CHECK_ARG(x && w, "gemm_h_ex: null operand");
    SDVAR_CHECK_ARG(M >= 1 && N >= 8 && N % 8 == 0 && K >= 32 && K % 32 == 0 && M <= (1 << 24) && N <= (1 << 24), "gemm_h_ex: need M >= 1, N %% 8 == 0 and K %% 32 == 0 (M=%d N=%d K=%d)", M, N, K);
    SDVAR_CHECK_ARG(al16(x) && al16(w) && al16(bias) && al16(out) && al16(h_out) && al16(p_out) && al16(res) && al16(gate), "gemm_h_ex: operands must be 16-byte aligned");
    SDVAR_CHECK_ARG(((uintptr_t)w_scale % 4) == 0, "gemm_h_ex: w_scale must be 4-byte aligned");
    if (epi == GH_EPI_GELU) {
        SDVAR_CHECK_ARG(h_out && !out, "gemm_h_ex: epilogue 1 writes h_out (and pre_out on request), not `out`");
        SDVAR_CHECK_ARG(N % 32 == 0, "gemm_h_ex: epilogue 1 writes the next GEMM's operand: N %% 32 == 0 (N=%d)", N);
    } else {
        SDVAR_CHECK_ARG(out && !h_out && !p_out, "gemm_h_ex: epilogue %d writes `out` only", epi);
        SDVAR_CHECK_ARG(ldo >= N && ldo % 4 == 0, "gemm_h_ex: need ldo >= N and ldo %% 4 == 0 (ldo=%d N=%d)", ldo, N);
    }
    if (epi == GH_EPI_GATED_RES) {
        SDVAR_CHECK_ARG(res && gate, "gemm_h_ex: epilogue 2 needs res and gate");
        SDVAR_CHECK_ARG(rows_per_gate >= 1, "gemm_h_ex: rows_per_gate %d", rows_per_gate);
        SDVAR_CHECK_ARG(ldres >= N && ldres % 4 == 0 && gate_stride >= 0 && gate_stride % 4 == 0, "gemm_h_ex: need ldres >= N, ldres %% 4 == 0 and gate_stride %% 4 == 0 (ldres=%d gate_stride=%d)", ldres, gate_stride);
    } else {
        SDVAR_CHECK_ARG(!res && !gate, "gemm_h_ex: res / gate belong to epilogue 2");
    }
    const GemmHalfArgs a{reinterpret_cast<const uint16_t*>(x), reinterpret_cast<const uint16_t*>(w), bias, out, 0, ldo,
                         reinterpret_cast<uint16_t*>(h_out), reinterpret_cast<uint16_t*>(p_out), M, N, K, w_scale, res, ldres, gate, rows_per_gate > 0 ? rows_per_gate : 1, gate_stride};
    if (epi == GH_EPI_GATED_RES) return gh_launch<false, GH_EPI_GATED_RES, true>(a, stream);
    return epi == GH_EPI_GELU ? gh_launch<false, GH_EPI_GELU, true>(a, stream) : gh_launch<false, GH_EPI_BIAS, true>(a, stream);
}

}  // namespace sdvar

extern "C" {
int sdvar_op_gemm_h(const void* x, const void* w, int32_t dtype, const float* bias, void* out, int32_t out_dtype, int32_t ldo, void* h_out, void* p_out, int32_t M, int32_t N,
                    int32_t K, int32_t epilogue, void* stream) {
    return sdvar::gemm_half(x, w, dtype, bias, out, out_dtype, ldo, h_out, p_out, M, N, K, epilogue, (hipStream_t)stream);
}
int sdvar_op_gemm_h_ex(const void* x, const void* w, int32_t dtype, const float* w_scale, const float* bias, float* out, int32_t ldo, void* h_out, void* pre_out, const float* res,
                       int32_t ldres, const float* gate, int32_t rows_per_gate, int32_t gate_stride, int32_t M, int32_t N, int32_t K, int32_t epilogue, void* stream) {
    return sdvar::gemm_half_ex(x, w, dtype, w_scale, bias, out, ldo, h_out, pre_out, res, ldres, gate, rows_per_gate, gate_stride, M, N, K, epilogue, (hipStream_t)stream);
}
}  // extern "C"
