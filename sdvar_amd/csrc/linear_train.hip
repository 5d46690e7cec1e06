// Operand producers of the dense linears' backward (seam.linear_grad / linear_amp_grad; the reference's mat_qkv, proj, ada_lin, word_embed and head under autograd):
//     y = x W^T + b,   dx = dy W,   dW = dy^T x,   db = sum_m dy
// Both gradient products are NT GEMMs of the existing family once dy exists as the row-major operand (K = N, for dx) and as the transposed, zero-padded operand
// (K = M rounded up to 32, for dW).  The kernels here make ONE pass over dy and write both, plus db's 32-row partials, where the FFN backward's single-purpose entries
// (split_planes* + transpose_operand + colsum, or two half_operand calls) read dy three times, resp. twice.  Formats and bits are those entries' (mlp_bwd.hip, mlp_half.hip):
//
//   grad_operands      dy fp32 (rows, cols) with a leading dimension, read once -> the row-major operand (formats 2 / 3: K-blocked planes of dy * 2^S; format 0 has none:
//                      dy itself is the operand), the operand of dy^T (cols x Mp, zero tail written here) and the column sums of the UNSCALED dy per block of 32 rows
//   grad_operands_h    the same pass for the half matrix cores: dy fp16 / bf16, or fp32 rounded to nearest even as it is read; ONE plane per operand; the column sums
//                      add the ROUNDED values
//   operand_transpose_h   a K-blocked 16-bit operand (rows x K) -> the operand of its transpose (K x Mp), zero tail included; the bits move untouched, so the forward's
//                      operand of x (2 M K bytes) is all the half backward needs of x
//
// Bandwidth kernels: 16 or 32 bytes per lane and load, 16 bytes per lane and store.  A workgroup moves a 32 (k) x 64 tile through LDS with rows padded to 65 words
// (the bank argument of mlp_bwd.hip holds unchanged).  No atomics, nothing is clamped beyond what the f16x2 split itself does; every output is optional.
#include "../../include/sdvar_hip.h"
#include "common.h"

namespace sdvar {

constexpr int LK = OPT_K, LC = OPT_C, LS = OPT_S;          // the transposing tile of common.h

// ------------------------------------------------------------------------------------------------ grad_operands (fp32 modes)
struct GradOperandsArgs {
    const float* dy; const float* scale;            // scale: device {2^S, 2^-S, ..} multiplying dy in its operands (f16x2), or null
    void* out; void* out_t; float* part;            // any may be null
    size_t out_ps, out_t_ps;
    int ld, rows, cols, fmt;
};

__global__ __launch_bounds__(256) void grad_operands_kernel(GradOperandsArgs a) {
    __shared__ float tile[LK * LS];                 // the UNSCALED values: the partial sums add what dy holds, the operands multiply as they leave
    const int r = threadIdx.x >> 3, cg = threadIdx.x & 7;
    const int c0 = blockIdx.x * LC, kb = blockIdx.y;
    const int row = kb * LK + r, col = c0 + 8 * cg;
    const bool live = row < a.rows && col < a.cols;             // cols % 8 == 0: a group of 8 is inside or outside as a whole
    const float sc = a.scale ? a.scale[0] : 1.0f;
    f32x4 p = {0.f, 0.f, 0.f, 0.f}, q = p;
    if (live) {
        const float* s = a.dy + (size_t)row * a.ld + col;
        p = *reinterpret_cast<const f32x4*>(s); q = *reinterpret_cast<const f32x4*>(s + 4);
    }
    if (a.out) {
        const float v[8] = {p[0] * sc, p[1] * sc, p[2] * sc, p[3] * sc, q[0] * sc, q[1] * sc, q[2] * sc, q[3] * sc};
        store_operand8(a.out, a.out_ps, a.fmt, row, col, a.rows, a.cols, v, live);
    }
    if (!a.out_t && !a.part) return;
#pragma unroll
    for (int e = 0; e < 4; ++e) { tile[r * LS + 8 * cg + e] = p[e]; tile[r * LS + 8 * cg + 4 + e] = q[e]; }
    __syncthreads();
    if (a.out_t) store_tile_t<true>(tile, a.out_t, a.out_t_ps, a.fmt, c0, kb, a.cols, ((a.rows + 31) / 32) * 32, sc);
    if (a.part && threadIdx.x < LC && c0 + threadIdx.x < a.cols) {          // this block's 32 rows, summed in row order
        float s = 0.f;
#pragma unroll
        for (int rr = 0; rr < LK; ++rr) s += tile[rr * LS + threadIdx.x];
        a.part[(size_t)kb * a.cols + c0 + threadIdx.x] = s;
    }
}

static bool al16(const void* q) { return ((uintptr_t)q % 16) == 0; }

int grad_operands(const float* dy, int ld, int rows, int cols, int fmt, const float* scale, void* out, size_t out_ps, void* out_t, size_t out_t_ps, float* part,
                  hipStream_t stream) {
    SDVAR_CHECK_ARG(fmt == OPF_F32 || fmt == PLANES_F16X2 || fmt == PLANES_BF16X3, "grad_operands: format %d (0 fp32, 2 f16x2, 3 bf16x3)", fmt);
    SDVAR_CHECK_ARG(!scale || fmt == PLANES_F16X2, "grad_operands: a scale goes with format 2 (f16x2) only");
    SDVAR_CHECK_ARG(dy && rows > 0 && cols > 0 && cols % 32 == 0 && ld >= cols && ld % 4 == 0, "grad_operands: need dy, cols %% 32 == 0 and ld %% 4 == 0 (rows=%d cols=%d ld=%d)",
                    rows, cols, ld);
    SDVAR_CHECK_ARG(out || out_t || part, "grad_operands: no output");
    SDVAR_CHECK_ARG(!out || fmt != OPF_F32, "grad_operands: format 0 has no row-major operand (dy itself is the operand); pass out = NULL");
    SDVAR_CHECK_ARG(al16(dy) && al16(out) && al16(out_t) && ((uintptr_t)part % 4) == 0 && ((uintptr_t)scale % 4) == 0, "grad_operands: operands must be 16-byte aligned");
    const int kblocks = (rows + 31) / 32;
    SDVAR_CHECK_ARG(kblocks <= 65535, "grad_operands: rows %d too many", rows);
    if (fmt != OPF_F32)
        SDVAR_CHECK_ARG((!out || (out_ps % 8 == 0 && out_ps >= (size_t)rows * cols)) && (!out_t || (out_t_ps % 8 == 0 && out_t_ps >= (size_t)cols * kblocks * 32)),
                        "grad_operands: a plane stride is below its operand (rows cols row-major, cols * padded rows transposed) or no multiple of 8");
    const GradOperandsArgs a{dy, scale, out, out_t, part, out_ps, out_t_ps, ld, rows, cols, fmt};
    hipLaunchKernelGGL(grad_operands_kernel, dim3((cols + LC - 1) / LC, kblocks), dim3(256), 0, stream, a);
    SDVAR_LAUNCH_CHECK();
    return SDVAR_OK;
}

// ------------------------------------------------------------------------------------------------ grad_operands_h (half matrix cores)
__global__ __launch_bounds__(256) void grad_operands_h_kernel(const void* __restrict__ dy, int x_dtype, int ld, int rows, int cols, int bfi, uint16_t* __restrict__ out,
                                                              uint16_t* __restrict__ out_t, float* __restrict__ part) {
    __shared__ float tile[LK * LS];                 // the values AFTER rounding, as floats: the store's conversion is exact, the sums add what the operands hold
    const bool bf = bfi != 0;
    const int r = threadIdx.x >> 3, cg = threadIdx.x & 7;
    const int c0 = blockIdx.x * LC, kb = blockIdx.y;
    const int row = kb * LK + r, col = c0 + 8 * cg;
    const bool live = row < rows && col < cols;
    u32x4 w = {0u, 0u, 0u, 0u};
    if (live) {
        const size_t off = (size_t)row * ld + col;
        if (x_dtype == 0) {
            const float* s = reinterpret_cast<const float*>(dy) + off;
            const f32x4 p = *reinterpret_cast<const f32x4*>(s), q = *reinterpret_cast<const f32x4*>(s + 4);
            const float f[8] = {p[0], p[1], p[2], p[3], q[0], q[1], q[2], q[3]};
            w = hp_pack8(f, bf);
        } else {
            w = *reinterpret_cast<const u32x4*>(reinterpret_cast<const uint16_t*>(dy) + off);
        }
        if (out) *reinterpret_cast<u32x4*>(out + kb_index(row, col, rows)) = w;
    }
    if (!out_t && !part) return;
#pragma unroll
    for (int e = 0; e < 4; ++e) { tile[r * LS + 8 * cg + 2 * e] = half_lo(w[e], bf); tile[r * LS + 8 * cg + 2 * e + 1] = half_hi(w[e], bf); }
    __syncthreads();
    if (out_t) hp_store_tile_t(tile, out_t, bf, c0, kb, cols);
    if (part && threadIdx.x < LC && c0 + threadIdx.x < cols) {
        float s = 0.f;
#pragma unroll
        for (int rr = 0; rr < LK; ++rr) s += tile[rr * LS + threadIdx.x];
        part[(size_t)kb * cols + c0 + threadIdx.x] = s;
    }
}

int grad_operands_h(const void* dy, int x_dtype, int ld, int rows, int cols, int dtype, void* out, void* out_t, float* part, hipStream_t stream) {
    SDVAR_CHECK_ARG(dtype == 1 || dtype == 2, "grad_operands_h: dtype %d (1 = fp16, 2 = bf16)", dtype);
    SDVAR_CHECK_ARG(x_dtype == 0 || x_dtype == dtype, "grad_operands_h: input dtype %d (0 = fp32, or the operand dtype %d)", x_dtype, dtype);
    const int lda = x_dtype == 0 ? 4 : 8;
    SDVAR_CHECK_ARG(dy && rows > 0 && cols > 0 && cols % 32 == 0 && ld >= cols && ld % lda == 0, "grad_operands_h: need dy, cols %% 32 == 0 and ld %% %d == 0 (rows=%d cols=%d ld=%d)",
                    lda, rows, cols, ld);
    SDVAR_CHECK_ARG(out || out_t || part, "grad_operands_h: no output");
    SDVAR_CHECK_ARG(al16(dy) && al16(out) && al16(out_t) && ((uintptr_t)part % 4) == 0, "grad_operands_h: operands must be 16-byte aligned");
    const int kblocks = (rows + 31) / 32;
    SDVAR_CHECK_ARG(kblocks <= 65535, "grad_operands_h: rows %d too many", rows);
    hipLaunchKernelGGL(grad_operands_h_kernel, dim3((cols + LC - 1) / LC, kblocks), dim3(256), 0, stream, dy, x_dtype, ld, rows, cols, (int)(dtype == 2),
                       reinterpret_cast<uint16_t*>(out), reinterpret_cast<uint16_t*>(out_t), part);
    SDVAR_LAUNCH_CHECK();
    return SDVAR_OK;
}

// ------------------------------------------------------------------------------------------------ operand_transpose_h
__global__ __launch_bounds__(256) void operand_transpose_h_kernel(const uint16_t* __restrict__ in, int rows, int K, uint16_t* __restrict__ out) {
    __shared__ uint32_t tile[LK * LS];              // one 16-bit element per word: the bits, whatever the dtype
    const int r = threadIdx.x >> 3, cg = threadIdx.x & 7;
    const int c0 = blockIdx.x * LC, kb = blockIdx.y;
    const int row = kb * LK + r, col = c0 + 8 * cg;
    u32x4 w = {0u, 0u, 0u, 0u};
    if (row < rows && col < K) w = *reinterpret_cast<const u32x4*>(in + kb_index(row, col, rows));          // col % 8 == 0: eight k of one 32-block, 16 contiguous bytes
#pragma unroll
    for (int e = 0; e < 4; ++e) { tile[r * LS + 8 * cg + 2 * e] = w[e] & 0xFFFFu; tile[r * LS + 8 * cg + 2 * e + 1] = w[e] >> 16; }
    __syncthreads();
    const int cl = threadIdx.x >> 2, kq = threadIdx.x & 3;
    if (c0 + cl >= K) return;
    u32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = tile[(8 * kq + 2 * e) * LS + cl] | (tile[(8 * kq + 2 * e + 1) * LS + cl] << 16);
    *reinterpret_cast<u32x4*>(out + kb_index(c0 + cl, kb * LK + 8 * kq, K)) = o;
}

int operand_transpose_h(const void* in, int rows, int K, void* out, hipStream_t stream) {
    SDVAR_CHECK_ARG(in && out && rows > 0 && K > 0 && K % 32 == 0, "operand_transpose_h: need both operands and K %% 32 == 0 (rows=%d K=%d)", rows, K);
    SDVAR_CHECK_ARG(al16(in) && al16(out), "operand_transpose_h: operands must be 16-byte aligned");
    const int kblocks = (rows + 31) / 32;
    SDVAR_CHECK_ARG(kblocks <= 65535, "operand_transpose_h: rows %d too many", rows);
    hipLaunchKernelGGL(operand_transpose_h_kernel, dim3((K + LC - 1) / LC, kblocks), dim3(256), 0, stream, reinterpret_cast<const uint16_t*>(in), rows, K,
                       reinterpret_cast<uint16_t*>(out));
    SDVAR_LAUNCH_CHECK();
    return SDVAR_OK;
}

}  // namespace sdvar

extern "C" {
int sdvar_op_grad_operands(const float* dy, int32_t ld, int32_t rows, int32_t cols, int32_t format, const float* scale, void* out, uint64_t out_plane_stride, void* out_t,
                           uint64_t out_t_plane_stride, float* colsum_part, void* stream) {
    return sdvar::grad_operands(dy, ld, rows, cols, format, scale, out, (size_t)out_plane_stride, out_t, (size_t)out_t_plane_stride, colsum_part, (hipStream_t)stream);
}
int sdvar_op_grad_operands_h(const void* dy, int32_t x_dtype, int32_t ld, int32_t rows, int32_t cols, int32_t dtype, void* out, void* out_t, float* colsum_part, void* stream) {
    return sdvar::grad_operands_h(dy, x_dtype, ld, rows, cols, dtype, out, out_t, colsum_part, (hipStream_t)stream);
}
int sdvar_op_operand_transpose_h(const void* in, int32_t rows, int32_t K, void* out, void* stream) {
    return sdvar::operand_transpose_h(in, rows, K, out, (hipStream_t)stream);
}
}  // extern "C"
