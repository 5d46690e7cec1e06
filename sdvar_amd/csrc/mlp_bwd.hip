// Operand producers of the FFN backward (seam.fused_mlp_func_grad; the reference's FFN, basic_var.py:33-52):
//     pre = x W1^T + b1,  h = gelu_tanh(pre),  y = h W2^T + b2
//     dh = dy W2,  dpre = dh o gelu_tanh'(pre),  dx = dpre W1,  dW2 = dy^T h,  dW1 = dpre^T x,  db2 = sum_m dy,  db1 = sum_m dpre
// Every product is an NT GEMM of the existing family (out[M',N'] = A[M',K'] B[N',K']^T) once its operands exist in the right orientation; the kernels here
// produce those operands, in the format of the GEMM mode (OPF_F32: plain fp32 row-major; PLANES_BF16X3 / PLANES_F16X2: K-blocked planes, common.h kb_index):
//
//   transpose_operand   fp32 (rows, cols) -> the operand of its TRANSPOSE, (cols x Kp), Kp = rows rounded up to 32 (the GEMMs' K step); the tail k >= rows is
//                       written as zeros by the kernel itself in every plane.  W1^T, W2^T, x^T, dy^T.
//   gelu_operand        pre (M, N) -> the operand of gelu_tanh(pre) (the forward under grad: fc1 runs with the bias epilogue and leaves pre in memory)
//   gelu_bwd            dh, pre (M, N), read once -> dpre = dh g'(pre) as the row-major operand (K = N), dpre^T and h^T = g(pre)^T as transposed, zero-padded
//                       operands (K = M), and the column sums of dpre per 32-row block (db1's partials); every output optional
//   colsum              fp32 (M, N) -> (N) column sums, fixed order, no atomics, double accumulation
//   scale_pair          one thread: the device scalars of a GEMM whose two operands both carry a power-of-two scale (f16x2)
//
// All are bandwidth kernels: 32 bytes per lane and load (two float4), 16 bytes per lane and store into a plane.  The transposing kernels move a 32 (k) x 64 tile
// through LDS with rows padded to 65 floats: thread (row r = tid / 8, column group tid % 8) writes tile[r][8 cg + e], thread (column cl = tid / 4, k group
// kq = tid % 4) reads tile[8 kq + e][cl].  With 4-byte LDS accesses the bank is (address / 4) % 32 and lanes conflict inside a 32-lane half: the reads touch
// banks 8 kq + cl + e with cl in 8 consecutive values - 32 different banks; the writes touch r + 8 cg + e with r in 4 consecutive values - two lanes per bank,
// which a ds_write_b32 absorbs (its cycles are set by the data transfer, MI355X_MICROARCH.md "LDS").
#include "../../include/sdvar_hip.h"
#include "common.h"

namespace sdvar {

int weight_scale_f16(const float* w, size_t n, float* sc, hipStream_t stream);          // gemm_f16x2.hip

constexpr int TK = OPT_K, TC = OPT_C, TS = OPT_S;          // the transposing tile of common.h (store_tile_t)

// gelu_val_grad (g and g' of both GELU forms), OPF_F32, store_operand8 and store_tile_t live in common.h: mlp_half.hip and linear_train.hip share them.

// ------------------------------------------------------------------------------------------------ transpose_operand
__global__ __launch_bounds__(256) void transpose_operand_kernel(const float* __restrict__ x, int ldx, int rows, int cols, int fmt, void* __restrict__ out, size_t ps,
                                                                const float* __restrict__ scale) {
    __shared__ float tile[TK * TS];
    const int r = threadIdx.x >> 3, cg = threadIdx.x & 7;
    const int c0 = blockIdx.x * TC, kb = blockIdx.y;
    const int row = kb * TK + r, col = c0 + 8 * cg;
    const float sc = scale ? *scale : 1.0f;
    f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = a;
    if (row < rows && col < cols) {                     // cols % 8 == 0: a group of 8 is inside or outside as a whole
        const float* p = x + (size_t)row * ldx + col;
        a = *reinterpret_cast<const f32x4*>(p); b = *reinterpret_cast<const f32x4*>(p + 4);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) { tile[r * TS + 8 * cg + e] = a[e] * sc; tile[r * TS + 8 * cg + 4 + e] = b[e] * sc; }
    __syncthreads();
    store_tile_t(tile, out, ps, fmt, c0, kb, cols, ((rows + 31) / 32) * 32);
}

static bool fmt_ok(int fmt) { return fmt == OPF_F32 || fmt == PLANES_F16X2 || fmt == PLANES_BF16X3; }

int transpose_operand(const float* x, int ldx, int rows, int cols, int fmt, void* out, size_t ps, const float* scale, hipStream_t stream) {
    SDVAR_CHECK_ARG(x && out && rows > 0 && cols > 0 && cols % 8 == 0 && ldx >= cols && ldx % 4 == 0, "transpose_operand: need cols %% 8 == 0 and ldx %% 4 == 0 (rows=%d cols=%d ldx=%d)", rows, cols, ldx);
    SDVAR_CHECK_ARG(fmt_ok(fmt) && (fmt == PLANES_F16X2 || !scale), "transpose_operand: format %d (0 fp32, 2 f16x2, 3 bf16x3; a scale goes with 2 only)", fmt);
    SDVAR_CHECK_ARG(((uintptr_t)x % 16) == 0 && ((uintptr_t)out % 16) == 0 && (fmt == OPF_F32 || ps % 8 == 0), "transpose_operand: operands must be 16-byte aligned");
    const int kblocks = (rows + 31) / 32;
    SDVAR_CHECK_ARG(kblocks <= 65535 && (fmt == OPF_F32 || ps >= (size_t)cols * kblocks * 32), "transpose_operand: rows %d too many, or plane stride below cols * padded rows", rows);
    hipLaunchKernelGGL(transpose_operand_kernel, dim3((cols + TC - 1) / TC, kblocks), dim3(256), 0, stream, x, ldx, rows, cols, fmt, out, ps, scale);
    SDVAR_LAUNCH_CHECK();
    return SDVAR_OK;
}

// ------------------------------------------------------------------------------------------------ gelu_operand
__global__ __launch_bounds__(256) void gelu_operand_kernel(const float* __restrict__ pre, int M, int N, int fmt, int kind, void* __restrict__ out, size_t ps) {
    const int n8 = N >> 3;
    const size_t total = (size_t)M * n8, i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = i < total;
    const int m = live ? (int)(i / n8) : 0, n = live ? (int)(i % n8) * 8 : 0;
    const float* p = pre + (size_t)m * N + n;
    const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);          // a dead lane re-reads element 0
    float v[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) { v[e] = kind ? gelu_tanh_h(a[e]) : gelu_tanh(a[e]); v[4 + e] = kind ? gelu_tanh_h(b[e]) : gelu_tanh(b[e]); }
    store_operand8(out, ps, fmt, m, n, M, N, v, live);
}

int gelu_operand(const float* pre, int M, int N, int fmt, int kind, void* out, size_t ps, hipStream_t stream) {
    SDVAR_CHECK_ARG(pre && out && M > 0 && N > 0 && N % 32 == 0 && fmt_ok(fmt) && (kind == 0 || kind == 1), "gelu_operand: need N %% 32 == 0 (M=%d N=%d format %d kind %d)", M, N, fmt, kind);
    SDVAR_CHECK_ARG(((uintptr_t)pre % 16) == 0 && ((uintptr_t)out % 16) == 0 && (fmt == OPF_F32 || (ps % 8 == 0 && ps >= (size_t)M * N)), "gelu_operand: operands must be 16-byte aligned, plane stride >= M N");
    const size_t total = (size_t)M * (N / 8);
    hipLaunchKernelGGL(gelu_operand_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, pre, M, N, fmt, kind, out, ps);
    SDVAR_LAUNCH_CHECK();
    return SDVAR_OK;
}

// ------------------------------------------------------------------------------------------------ gelu_bwd
struct GeluBwdArgs {
    const float* dh; const float* pre; const float* scale;      // scale: device {2^S, 2^-S} multiplying dpre in its operands (f16x2), or null
    void* dpre; void* dpre_t; void* h_t; float* part;           // any may be null
    size_t dpre_ps, dpre_t_ps, h_t_ps;
    int M, N, fmt, kind;
};

__global__ __launch_bounds__(256) void gelu_bwd_kernel(GeluBwdArgs a) {
    __shared__ float dt[TK * TS];
    __shared__ float ht[TK * TS];
    const int r = threadIdx.x >> 3, cg = threadIdx.x & 7;
    const int c0 = blockIdx.x * TC, kb = blockIdx.y;
    const int m = kb * TK + r, n = c0 + 8 * cg;
    const bool live = m < a.M && n < a.N;
    const float sc = a.scale ? a.scale[0] : 1.0f;
    f32x4 p0 = {0.f, 0.f, 0.f, 0.f}, p1 = p0, d0 = p0, d1 = p0;
    if (live) {
        const size_t o = (size_t)m * a.N + n;
        p0 = *reinterpret_cast<const f32x4*>(a.pre + o); p1 = *reinterpret_cast<const f32x4*>(a.pre + o + 4);
        if (a.dh) { d0 = *reinterpret_cast<const f32x4*>(a.dh + o); d1 = *reinterpret_cast<const f32x4*>(a.dh + o + 4); }
    }
    float dv[8], hv[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        float g, dg;
        gelu_val_grad(e < 4 ? p0[e] : p1[e - 4], a.kind, g, dg);
        hv[e] = g;                                          // rows past M: g(0) = 0, the zero tail of h^T
        dv[e] = ((e < 4 ? d0[e] : d1[e - 4]) * dg) * sc;
    }
    if (a.dpre) store_operand8(a.dpre, a.dpre_ps, a.fmt, m, n, a.M, a.N, dv, live);
    if (!a.dpre_t && !a.h_t && !a.part) return;
#pragma unroll
    for (int e = 0; e < 8; ++e) { dt[r * TS + 8 * cg + e] = dv[e]; ht[r * TS + 8 * cg + e] = hv[e]; }
    __syncthreads();
    const int Kp = ((a.M + 31) / 32) * 32;
    if (a.dpre_t) store_tile_t(dt, a.dpre_t, a.dpre_t_ps, a.fmt, c0, kb, a.N, Kp);
    if (a.h_t) store_tile_t(ht, a.h_t, a.h_t_ps, a.fmt, c0, kb, a.N, Kp);
    if (a.part && threadIdx.x < TC && c0 + threadIdx.x < a.N) {         // db1's partial: this block's 32 rows, summed in row order; the power-of-two scale comes off exactly
        float s = 0.f;
#pragma unroll
        for (int rr = 0; rr < TK; ++rr) s += dt[rr * TS + threadIdx.x];
        a.part[(size_t)kb * a.N + c0 + threadIdx.x] = a.scale ? s * a.scale[1] : s;
    }
}

int gelu_bwd(const float* dh, const float* pre, int M, int N, int fmt, int kind, const float* scale, void* dpre, size_t dpre_ps, void* dpre_t, size_t dpre_t_ps, void* h_t,
             size_t h_t_ps, float* part, hipStream_t stream) {
    SDVAR_CHECK_ARG(pre && M > 0 && N > 0 && N % 32 == 0 && fmt_ok(fmt) && (kind == 0 || kind == 1), "gelu_bwd: need N %% 32 == 0 (M=%d N=%d format %d kind %d)", M, N, fmt, kind);
    SDVAR_CHECK_ARG(dpre || dpre_t || h_t || part, "gelu_bwd: no output");
    SDVAR_CHECK_ARG(dh || (!dpre && !dpre_t && !part), "gelu_bwd: dpre, dpre^T and the column sums need dh");
    SDVAR_CHECK_ARG(!scale || fmt == PLANES_F16X2, "gelu_bwd: a scale goes with format 2 (f16x2) only");
    const int kblocks = (M + 31) / 32;
    const size_t need = (size_t)N * kblocks * 32;
    auto al16 = [](const void* q) { return ((uintptr_t)q % 16) == 0; };
    SDVAR_CHECK_ARG(al16(dh) && al16(pre) && al16(dpre) && al16(dpre_t) && al16(h_t), "gelu_bwd: operands must be 16-byte aligned");
    if (fmt != OPF_F32)
        SDVAR_CHECK_ARG((!dpre || (dpre_ps % 8 == 0 && dpre_ps >= (size_t)M * N)) && (!dpre_t || (dpre_t_ps % 8 == 0 && dpre_t_ps >= need)) && (!h_t || (h_t_ps % 8 == 0 && h_t_ps >= need)),
                        "gelu_bwd: a plane stride is below its operand (M N row-major, N * padded M transposed) or no multiple of 8");
    SDVAR_CHECK_ARG(kblocks <= 65535, "gelu_bwd: M %d too large", M);
    const GeluBwdArgs a{dh, pre, scale, dpre, dpre_t, h_t, part, dpre_ps, dpre_t_ps, h_t_ps, M, N, fmt, kind};
    hipLaunchKernelGGL(gelu_bwd_kernel, dim3((N + TC - 1) / TC, kblocks), dim3(256), 0, stream, a);
    SDVAR_LAUNCH_CHECK();
    return SDVAR_OK;
}

// ------------------------------------------------------------------------------------------------ colsum
// One workgroup per 32 columns: thread (row lane ry = tid / 8, float4 column cx = tid % 8) adds rows ry, ry + 32, .. in double; the 32 row lanes are then added in
// lane order by the first 32 threads.  The order depends on M and N only.
__global__ __launch_bounds__(256) void colsum_kernel(const float* __restrict__ x, int ldx, int M, int N, float* __restrict__ out) {
    __shared__ double part[32 * 33];
    const int ry = threadIdx.x >> 3, cx = threadIdx.x & 7;
    const int n = blockIdx.x * 32 + 4 * cx;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    if (n < N) {                                            // N % 4 == 0
        int m = ry;
        for (; m + 96 < M; m += 128) {                      // four rows in flight
            f32x4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const f32x4*>(x + (size_t)(m + 32 * u) * ldx + n);
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e] += (double)v[u][e];
        }
        for (; m < M; m += 32) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(x + (size_t)m * ldx + n);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] += (double)v[e];
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) part[ry * 33 + 4 * cx + e] = acc[e];
    __syncthreads();
    if (threadIdx.x < 32 && blockIdx.x * 32 + threadIdx.x < N) {
        double s = 0.0;
        for (int rr = 0; rr < 32; ++rr) s += part[rr * 33 + threadIdx.x];
        out[blockIdx.x * 32 + threadIdx.x] = (float)s;
    }
}

int colsum(const float* x, int ldx, int M, int N, float* out, hipStream_t stream) {
    SDVAR_CHECK_ARG(x && out && M > 0 && N > 0 && N % 4 == 0 && ldx >= N && ldx % 4 == 0 && ((uintptr_t)x % 16) == 0, "colsum: need N %% 4 == 0, ldx %% 4 == 0 and a 16-byte aligned input (M=%d N=%d ldx=%d)", M, N, ldx);
    hipLaunchKernelGGL(colsum_kernel, dim3((N + 31) / 32), dim3(256), 0, stream, x, ldx, M, N, out);
    SDVAR_LAUNCH_CHECK();
    return SDVAR_OK;
}

// ------------------------------------------------------------------------------------------------ scale_pair
// sc = {2^S, 2^-S, scratch, -} (weight_scale_f16).  halve: S -= 1.  sc[3] = 2^-S * (other ? other[1] : 1): what a GEMM undoes when both operands are scaled.
__global__ void scale_pair_kernel(float* sc, int halve, const float* other) {
    if (halve) { sc[0] *= 0.5f; sc[1] *= 2.0f; }
    sc[3] = sc[1] * (other ? other[1] : 1.0f);
}

int scale_pair(const float* x, size_t n, float* sc, int halve, const float* other, hipStream_t stream) {
    SDVAR_CHECK_ARG(sc, "scale_pair: null scale");
    if (x) { const int rc = weight_scale_f16(x, n, sc, stream); if (rc != SDVAR_OK) return rc; }
    hipLaunchKernelGGL(scale_pair_kernel, dim3(1), dim3(1), 0, stream, sc, halve, other);
    SDVAR_LAUNCH_CHECK();
    return SDVAR_OK;
}

}  // namespace sdvar

extern "C" {

int sdvar_op_transpose_operand(const float* x, int32_t ldx, int32_t rows, int32_t cols, int32_t format, void* out, uint64_t plane_stride, const float* scale, void* stream) {
    return sdvar::transpose_operand(x, ldx, rows, cols, format, out, (size_t)plane_stride, scale, (hipStream_t)stream);
}
int sdvar_op_gelu_operand(const float* pre, int32_t M, int32_t N, int32_t format, int32_t gelu_kind, void* out, uint64_t plane_stride, void* stream) {
    return sdvar::gelu_operand(pre, M, N, format, gelu_kind, out, (size_t)plane_stride, (hipStream_t)stream);
}
int sdvar_op_gelu_bwd(const float* dh, const float* pre, int32_t M, int32_t N, int32_t format, int32_t gelu_kind, const float* scale, void* dpre, uint64_t dpre_plane_stride,
                      void* dpre_t, uint64_t dpre_t_plane_stride, void* h_t, uint64_t h_t_plane_stride, float* colsum_part, void* stream) {
    return sdvar::gelu_bwd(dh, pre, M, N, format, gelu_kind, scale, dpre, (size_t)dpre_plane_stride, dpre_t, (size_t)dpre_t_plane_stride, h_t, (size_t)h_t_plane_stride,
                           colsum_part, (hipStream_t)stream);
}
int sdvar_op_colsum(const float* x, int32_t ldx, int32_t M, int32_t N, float* out, void* stream) { return sdvar::colsum(x, ldx, M, N, out, (hipStream_t)stream); }
int sdvar_op_scale_pair(const float* x, uint64_t n, float* scale, int32_t halve, const float* other, void* stream) {
    return sdvar::scale_pair(x, (size_t)n, scale, halve, other, (hipStream_t)stream);
}
}  // extern "C"
