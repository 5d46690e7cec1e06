// Validation statistics of teacher-forced logits (VARTrainer.eval_ep, trainer.py:66-75): per token the cross-entropy
// against the ground-truth id and the argmax, and the four sums eval_ep accumulates.  HBM-bound row kernel: one wave64 per (image, token)
// row streams its V fp32 logits once with 16-byte loads.
//
//   lse      running max + rescaled sum in ONE pass (per lane over its float4 chunks, then a butterfly over the wave)
//   nll      lse - logit[target] in fp32 (log_softmax + nll_loss); a target outside [0, V) is never read: nll = NaN
//   argmax   (value, index) with the lowest index on ties, as torch.argmax
//   sums     {sum nll, sum tail nll, #correct, #tail correct} in double: per-workgroup partials, then one workgroup adds them in a fixed
//            order - no atomics, so two runs are bit-identical
#include "common.h"

namespace sdvar {

constexpr int XR = 4;             // rows (waves) per workgroup

// merge two (max, sum of exp(x - max)) pairs; an empty side has (-inf, 0)
__device__ __forceinline__ void lse_merge(float& m, float& s, float m2, float s2) {
    const float mn = fmaxf(m, m2);
    if (mn == -INFINITY) return;                      // both empty (or all -inf so far): nothing to rescale
    s = s * expf(m - mn) + s2 * expf(m2 - mn);
    m = mn;
}

__device__ __forceinline__ void arg_merge(float& v, int& i, float v2, int i2) {
    if (v2 > v || (v2 == v && i2 < i)) { v = v2; i = i2; }
}

__global__ __launch_bounds__(256) void xent_rows_kernel(const float* __restrict__ logits, const long long* __restrict__ targets, int rows, int L, int V, int tail,
                                                        float* __restrict__ nll_out, long long* __restrict__ argmax_out, double* __restrict__ part) {
    __shared__ double red[XR][4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int row = blockIdx.x * XR + w;
    double nll_d = 0.0, tnll_d = 0.0, cor = 0.0, tcor = 0.0;
    if (row < rows) {
        const f32x4* p = reinterpret_cast<const f32x4*>(logits + (size_t)row * V);
        float m = -INFINITY, s = 0.f, bv = -INFINITY;
        int bi = 0x7FFFFFFF;
#pragma unroll 4
        for (int c = lane; c < V / 4; c += 64) {
            const f32x4 v = p[c];
            const float cm = fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3]));
            if (cm > m) { s = s * expf(m - cm); m = cm; }      // s == 0 while m == -inf: exp(-inf) = 0 keeps it so
            if (m != -INFINITY) s += (expf(v[0] - m) + expf(v[1] - m)) + (expf(v[2] - m) + expf(v[3] - m));
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (v[k] > bv) { bv = v[k]; bi = 4 * c + k; }   // indices rise within a lane: strict > keeps the lowest
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64), v2 = __shfl_xor(bv, o, 64);
            const int i2 = __shfl_xor(bi, o, 64);
            lse_merge(m, s, m2, s2);
            arg_merge(bv, bi, v2, i2);
        }
        if (bi == 0x7FFFFFFF) bi = 0;                    // every logit NaN / -inf: torch.argmax's index 0 for an all -inf row
        const long long tg = targets[row];
        const bool ok = tg >= 0 && tg < V;
        const float lse = m + logf(s);
        const float nll = ok ? lse - logits[(size_t)row * V + tg] : __builtin_nanf("");
        if (lane == 0) {
            if (nll_out) nll_out[row] = nll;
            if (argmax_out) argmax_out[row] = bi;
        }
        const bool in_tail = (row % L) >= L - tail;
        const double c1 = (ok && bi == tg) ? 1.0 : 0.0;
        nll_d = (double)nll; cor = c1;
        if (in_tail) { tnll_d = (double)nll; tcor = c1; }
    }
    if (lane == 0) { red[w][0] = nll_d; red[w][1] = tnll_d; red[w][2] = cor; red[w][3] = tcor; }
    __syncthreads();
    if (threadIdx.x < 4) {
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < XR; ++k) acc += red[k][threadIdx.x];
        part[(size_t)blockIdx.x * 4 + threadIdx.x] = acc;
    }
}

// sums[k] (+)= sum over the n partial rows of part[.][k], in a fixed order: thread t adds rows t, t + 256, ... then a fixed tree
__global__ __launch_bounds__(256) void xent_sum_kernel(const double* __restrict__ part, int n, double* __restrict__ sums, int accumulate) {
    __shared__ double red[4][256];
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < n; i += 256)
#pragma unroll
        for (int k = 0; k < 4; ++k) a[k] += part[(size_t)i * 4 + k];
#pragma unroll
    for (int k = 0; k < 4; ++k) red[k][threadIdx.x] = a[k];
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (threadIdx.x < h)
#pragma unroll
            for (int k = 0; k < 4; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x < 4) sums[threadIdx.x] = (accumulate ? sums[threadIdx.x] : 0.0) + red[threadIdx.x][0];
}

static thread_local double* g_part = nullptr;           // per-workgroup partial sums, one buffer per host thread (sdvar_hip.h threading contract)
static thread_local size_t g_part_n = 0;

int xent_stats(const float* logits, const long long* targets, int B, int L, int V, int tail, float* nll_out, long long* argmax_out, double* sums, int accumulate,
               hipStream_t stream) {
    SDVAR_CHECK_ARG(logits && targets && sums, "xent_stats: null logits, targets or sums");
    SDVAR_CHECK_ARG(B >= 1 && L >= 1 && tail >= 0 && tail <= L, "xent_stats: B=%d L=%d tail=%d", B, L, tail);
    SDVAR_CHECK_ARG(V >= 4 && V % 4 == 0 && (size_t)B * L <= 0x7FFFFFFF, "xent_stats: V=%d must be a positive multiple of 4", V);
    SDVAR_CHECK_ARG(((uintptr_t)logits & 15) == 0, "xent_stats: logits must be 16-byte aligned (float4 loads)");
    const int rows = B * L, nblk = (rows + XR - 1) / XR;
    if (g_part_n < (size_t)nblk * 4) {
        if (g_part) SDVAR_HIP(hipFree(g_part));
        g_part = nullptr; g_part_n = 0;
        SDVAR_HIP(hipMalloc((void**)&g_part, (size_t)nblk * 4 * sizeof(double)));
        g_part_n = (size_t)nblk * 4;
    }
    hipLaunchKernelGGL(xent_rows_kernel, dim3(nblk), dim3(64 * XR), 0, stream, logits, targets, rows, L, V, tail, nll_out, argmax_out, g_part);
    SDVAR_LAUNCH_CHECK();
    hipLaunchKernelGGL(xent_sum_kernel, dim3(1), dim3(256), 0, stream, (const double*)g_part, nblk, sums, accumulate);
    SDVAR_LAUNCH_CHECK();
    return SDVAR_OK;
}

}  // namespace sdvar
