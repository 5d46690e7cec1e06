// Operand producers of the half-precision FFN (seam.fused_mlp_func_amp / fused_mlp_func_amp_grad; the GEMM is gemm_half.hip), in the style of mlp_bwd.hip:
//     p = half(x_h W1_h^T + b1),  h = half(gelu_tanh(p)),  y = half(h W2_h^T + b2)
//     dh = dy W2_h,  dpre = half(dh o gelu_tanh'(p)),  dx = dpre W1_h,  dW2 = dy^T h,  dW1 = dpre^T x_h,  db2 = sum_m dy,  db1 = sum_m dpre
// An operand is ONE K-blocked plane [K/32][rows][32] of fp16 or bf16 (common.h kb_index).
//
//   half_operand   row-major fp32 or half (rows, cols) with a leading dimension -> the operand of the matrix (rows x cols, cols % 32 == 0) or of its TRANSPOSE
//                  (cols x Kp, Kp = rows rounded up to 32; the tail k >= rows is written as zeros by the kernel itself).  fp32 input is rounded to nearest even -
//                  the bits of .to(dtype); an fp16 overflow is inf.  The transposing form can also write the column sums of the ROUNDED input per block of 32 rows
//                  (db2's partials, taken from the dy^T pass), with or without the operand.
//   gelu_bwd_h     dh fp32 and the saved half pre-activation p (M, N), read once -> dpre = half(dh g'(float(p))) as the row-major operand, dpre^T and
//                  h^T = half(gelu_tanh(float(p)))^T as transposed, zero-padded operands, and the column sums of the ROUNDED dpre per 32-row block (db1's partials);
//                  every output optional.  g and g' are gelu_val_grad's exp / rcp form (common.h): h has the bits of the fc1 epilogue, g' is finite at both ends.
//
// Bandwidth kernels: 16 or 32 bytes per lane and load, 16 bytes per lane and store.  The transposing kernels move a 32 (k) x 64 tile through LDS with rows
// padded to 65 floats (the bank argument of mlp_bwd.hip holds unchanged); the tile holds the values AFTER rounding, as floats, so the store's conversion is exact
// and the partial sums add what the operands hold.  Nothing is clamped.
#include "../../include/sdvar_hip.h"
#include "common.h"

namespace sdvar {

constexpr int HK = OPT_K, HC = OPT_C, HS = OPT_S;          // the transposing tile of common.h (hp_store_tile_t)

// hp_pack8 / hp_unpack8 (eight values <-> one packed 16-byte word of the dtype) and hp_store_tile_t live in common.h: linear_train.hip shares them.
// eight consecutive values of a row, rounded to the operand dtype, as floats and as the packed word; x_dtype 0 = fp32 input, else the input already has the operand dtype
__device__ __forceinline__ u32x4 hp_load8(const void* x, int x_dtype, size_t off, bool bf, float* v) {
    u32x4 w;
    if (x_dtype == 0) {
        const float* p = reinterpret_cast<const float*>(x) + off;
        const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
        const float f[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
        w = hp_pack8(f, bf);
    } else {
        w = *reinterpret_cast<const u32x4*>(reinterpret_cast<const uint16_t*>(x) + off);
    }
    hp_unpack8(w, bf, v);
    return w;
}

// ------------------------------------------------------------------------------------------------ half_operand, as stored
__global__ __launch_bounds__(256) void half_operand_kernel(const void* __restrict__ x, int x_dtype, int ldx, int rows, int cols, int bf, uint16_t* __restrict__ out) {
    const int c8 = cols >> 3;
    const size_t total = (size_t)rows * c8, i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int r = (int)(i / c8), k = (int)(i % c8) * 8;
    float v[8];
    const u32x4 w = hp_load8(x, x_dtype, (size_t)r * ldx + k, bf != 0, v);
    *reinterpret_cast<u32x4*>(out + kb_index(r, k, rows)) = w;
}

// ------------------------------------------------------------------------------------------------ half_operand, transposed
__global__ __launch_bounds__(256) void half_operand_t_kernel(const void* __restrict__ x, int x_dtype, int ldx, int rows, int cols, int bf, uint16_t* __restrict__ out,
                                                             float* __restrict__ part) {
    __shared__ float tile[HK * HS];
    const int r = threadIdx.x >> 3, cg = threadIdx.x & 7;
    const int c0 = blockIdx.x * HC, kb = blockIdx.y;
    const int row = kb * HK + r, col = c0 + 8 * cg;
    float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (row < rows && col < cols) (void)hp_load8(x, x_dtype, (size_t)row * ldx + col, bf != 0, v);          // cols % 8 == 0: a group of 8 is inside or outside as a whole
#pragma unroll
    for (int e = 0; e < 8; ++e) tile[r * HS + 8 * cg + e] = v[e];
    __syncthreads();
    if (out) hp_store_tile_t(tile, out, bf != 0, c0, kb, cols);
    if (part && threadIdx.x < HC && c0 + threadIdx.x < cols) {          // this block's 32 rows, summed in row order
        float s = 0.f;
#pragma unroll
        for (int rr = 0; rr < HK; ++rr) s += tile[rr * HS + threadIdx.x];
        part[(size_t)kb * cols + c0 + threadIdx.x] = s;
    }
}

int half_operand(const void* x, int x_dtype, int ldx, int rows, int cols, int dtype, int transpose, void* out, float* part, hipStream_t stream) {
    SDVAR_CHECK_ARG(dtype == 1 || dtype == 2, "half_operand: dtype %d (1 = fp16, 2 = bf16)", dtype);
    SDVAR_CHECK_ARG(x_dtype == 0 || x_dtype == dtype, "half_operand: input dtype %d (0 = fp32, or the operand dtype %d)", x_dtype, dtype);
    SDVAR_CHECK_ARG(transpose == 0 || transpose == 1, "half_operand: transpose %d (0 or 1)", transpose);
    SDVAR_CHECK_ARG(x && (out || (transpose && part)), "half_operand: null input, or no output");
    SDVAR_CHECK_ARG(transpose || !part, "half_operand: the 32-row column sums come with the transposed form only");
    const int lda = x_dtype == 0 ? 4 : 8;
    SDVAR_CHECK_ARG(rows > 0 && cols > 0 && ldx >= cols && ldx % lda == 0 && (transpose ? cols % 8 == 0 : cols % 32 == 0),
                    "half_operand: need cols %% 32 == 0 (transposed: cols %% 8 == 0) and ldx %% %d == 0 (rows=%d cols=%d ldx=%d)", lda, rows, cols, ldx);
    SDVAR_CHECK_ARG(((uintptr_t)x % 16) == 0 && ((uintptr_t)out % 16) == 0, "half_operand: operands must be 16-byte aligned");
    if (!transpose) {
        const size_t total = (size_t)rows * (cols / 8);
        SDVAR_CHECK_ARG((total + 255) / 256 <= 0x7fffffffull, "half_operand: too large");
        hipLaunchKernelGGL(half_operand_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, x, x_dtype, ldx, rows, cols, (int)(dtype == 2), reinterpret_cast<uint16_t*>(out));
    } else {
        const int kblocks = (rows + 31) / 32;
        SDVAR_CHECK_ARG(kblocks <= 65535, "half_operand: rows %d too many for the transposed form", rows);
        hipLaunchKernelGGL(half_operand_t_kernel, dim3((cols + HC - 1) / HC, kblocks), dim3(256), 0, stream, x, x_dtype, ldx, rows, cols, (int)(dtype == 2),
                           reinterpret_cast<uint16_t*>(out), part);
    }
    SDVAR_LAUNCH_CHECK();
    return SDVAR_OK;
}

// ------------------------------------------------------------------------------------------------ gelu_bwd_h
struct GeluBwdHArgs {
    const float* dh; const uint16_t* p;
    uint16_t* dpre; uint16_t* dpre_t; uint16_t* h_t; float* part;           // any may be null
    int M, N, bf;
};

__global__ __launch_bounds__(256) void gelu_bwd_h_kernel(GeluBwdHArgs a) {
    __shared__ float dt[HK * HS];
    __shared__ float ht[HK * HS];
    const int r = threadIdx.x >> 3, cg = threadIdx.x & 7;
    const int c0 = blockIdx.x * HC, kb = blockIdx.y;
    const int m = kb * HK + r, n = c0 + 8 * cg;
    const bool live = m < a.M && n < a.N, bf = a.bf != 0;
    float pv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    f32x4 d0 = {0.f, 0.f, 0.f, 0.f}, d1 = d0;
    if (live) {
        const size_t o = (size_t)m * a.N + n;
        hp_unpack8(*reinterpret_cast<const u32x4*>(a.p + o), bf, pv);
        if (a.dh) { d0 = *reinterpret_cast<const f32x4*>(a.dh + o); d1 = *reinterpret_cast<const f32x4*>(a.dh + o + 4); }
    }
    float dv[8], hv[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        float g, dg;
        gelu_val_grad(pv[e], 1, g, dg);
        hv[e] = g;                                          // rows past M: g(0) = 0, the zero tail of h^T
        dv[e] = (e < 4 ? d0[e] : d1[e - 4]) * dg;           // rows past M: 0 * g'(0) = 0
    }
    const u32x4 dw = hp_pack8(dv, bf), hw = hp_pack8(hv, bf);
    if (a.dpre && live) *reinterpret_cast<u32x4*>(a.dpre + kb_index(m, n, a.M)) = dw;
    if (!a.dpre_t && !a.h_t && !a.part) return;
    hp_unpack8(dw, bf, dv); hp_unpack8(hw, bf, hv);        // the tiles hold the ROUNDED values
#pragma unroll
    for (int e = 0; e < 8; ++e) { dt[r * HS + 8 * cg + e] = dv[e]; ht[r * HS + 8 * cg + e] = hv[e]; }
    __syncthreads();
    if (a.dpre_t) hp_store_tile_t(dt, a.dpre_t, bf, c0, kb, a.N);
    if (a.h_t) hp_store_tile_t(ht, a.h_t, bf, c0, kb, a.N);
    if (a.part && threadIdx.x < HC && c0 + threadIdx.x < a.N) {         // db1's partial: this block's 32 rows of the rounded dpre, summed in row order
        float s = 0.f;
#pragma unroll
        for (int rr = 0; rr < HK; ++rr) s += dt[rr * HS + threadIdx.x];
        a.part[(size_t)kb * a.N + c0 + threadIdx.x] = s;
    }
}

int gelu_bwd_h(const float* dh, const void* p, int M, int N, int dtype, void* dpre, void* dpre_t, void* h_t, float* part, hipStream_t stream) {
    SDVAR_CHECK_ARG(dtype == 1 || dtype == 2, "gelu_bwd_h: dtype %d (1 = fp16, 2 = bf16)", dtype);
    SDVAR_CHECK_ARG(p && M > 0 && N > 0 && N % 32 == 0, "gelu_bwd_h: need the pre-activation and N %% 32 == 0 (M=%d N=%d)", M, N);
    SDVAR_CHECK_ARG(dpre || dpre_t || h_t || part, "gelu_bwd_h: no output");
    SDVAR_CHECK_ARG(dh || (!dpre && !dpre_t && !part), "gelu_bwd_h: dpre, dpre^T and the column sums need dh");
    auto al16 = [](const void* q) { return ((uintptr_t)q % 16) == 0; };
    SDVAR_CHECK_ARG(al16(dh) && al16(p) && al16(dpre) && al16(dpre_t) && al16(h_t), "gelu_bwd_h: operands must be 16-byte aligned");
    const int kblocks = (M + 31) / 32;
    SDVAR_CHECK_ARG(kblocks <= 65535, "gelu_bwd_h: M %d too large", M);
    const GeluBwdHArgs a{dh, reinterpret_cast<const uint16_t*>(p), reinterpret_cast<uint16_t*>(dpre), reinterpret_cast<uint16_t*>(dpre_t), reinterpret_cast<uint16_t*>(h_t), part, M, N,
                         (int)(dtype == 2)};
    hipLaunchKernelGGL(gelu_bwd_h_kernel, dim3((N + HC - 1) / HC, kblocks), dim3(256), 0, stream, a);
    SDVAR_LAUNCH_CHECK();
    return SDVAR_OK;
}

}  // namespace sdvar

extern "C" {
int sdvar_op_half_operand(const void* x, int32_t x_dtype, int32_t ldx, int32_t rows, int32_t cols, int32_t dtype, int32_t transpose, void* out, float* colsum_part, void* stream) {
    return sdvar::half_operand(x, x_dtype, ldx, rows, cols, dtype, transpose, out, colsum_part, (hipStream_t)stream);
}
int sdvar_op_gelu_bwd_h(const float* dh, const void* pre, int32_t M, int32_t N, int32_t dtype, void* dpre, void* dpre_t, void* h_t, float* colsum_part, void* stream) {
    return sdvar::gelu_bwd_h(dh, pre, M, N, dtype, dpre, dpre_t, h_t, colsum_part, (hipStream_t)stream);
}
}  // extern "C"
