// The trainer's label-smoothed cross-entropy (VARTrainer, trainer.py:37-38, called at :112 and reduced at :116-120) in both directions.  HBM-bound row
// kernels: one wave64 per row of V fp32 logits, 16-byte loads and stores, rows at a stride `ld` (a row-sliced view is read in place).
//
//   forward   ONE pass: running max + rescaled sum (lse) and, with eps > 0, sumx = sum_j x_j beside it;
//                 loss = (1 - eps) (lse - x_t) + eps (lse - sumx / V)            (torch's definition of label_smoothing = eps)
//             eps == 0 evaluates lse - x_t alone (a -inf logit elsewhere in the row leaves the loss finite, as in torch).  A target == ignore_index: loss 0, not
//             counted.  Any other target outside [0, V): NaN, x_t never read, counted.  Saved for the backward: lse, one float per row.
//   reduce    per-workgroup double partials {sum loss, counted rows}, then one workgroup adds them in a fixed order (no atomics: two runs are bit-identical) and
//             writes {sum, count} and the float the caller returns ('mean': sum / count, 'sum': sum)
//   backward  ONE read of the logits, one write: dlogits[row, j] = g_row (exp(x_j - lse_row) - (1 - eps) [j == t] - eps / V), every element written by exactly
//             one lane.  g_row = grad[row] ('none'), grad[0] ('sum') or grad[0] / count ('mean', count read from the forward's sums on the device).
//             Ignored rows: zeros (the logits are not read).  Out-of-range rows: NaN.
// Nothing here synchronises with the host or allocates: the partials live in a workspace of the caller.
#include "common.h"

namespace sdvar {

constexpr int XTR = 4;            // rows (waves) per workgroup

__global__ __launch_bounds__(256) void xent_train_fwd_kernel(const float* __restrict__ logits, long long ld, const long long* __restrict__ targets, long long rows, int V,
                                                             float eps, long long ignore_index, float* __restrict__ loss_out, float* __restrict__ lse_out,
                                                             double* __restrict__ part) {
    __shared__ double red[XTR][2];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long row = (long long)blockIdx.x * XTR + w;
    double loss_d = 0.0, cnt = 0.0;
    if (row < rows) {
        const float* x = logits + (size_t)row * (size_t)ld;
        const f32x4* p = reinterpret_cast<const f32x4*>(x);
        float m = -INFINITY, s = 0.f, sx = 0.f;
#pragma unroll 4
        for (int c = lane; c < V / 4; c += 64) {
            const f32x4 v = p[c];
            const float cm = fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3]));
            if (cm > m) { s = s * expf(m - cm); m = cm; }      // s == 0 while m == -inf: exp(-inf) = 0 keeps it so
            if (m != -INFINITY) s += (expf(v[0] - m) + expf(v[1] - m)) + (expf(v[2] - m) + expf(v[3] - m));
            sx += (v[0] + v[1]) + (v[2] + v[3]);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
            const float mn = fmaxf(m, m2);
            if (mn != -INFINITY) { s = s * expf(m - mn) + s2 * expf(m2 - mn); m = mn; }
            sx += __shfl_xor(sx, o, 64);
        }
        const float lse = m + logf(s);
        const long long tg = targets[row];
        float loss;
        if (tg == ignore_index) {
            loss = 0.f;
        } else if (tg < 0 || tg >= V) {
            loss = __builtin_nanf("");
            cnt = 1.0;
        } else {
            const float nll = lse - x[tg];
            loss = eps == 0.f ? nll : (1.0f - eps) * nll + eps * (lse - sx / (float)V);
            cnt = 1.0;
        }
        if (lane == 0) {
            loss_out[row] = loss;
            if (lse_out) lse_out[row] = lse;
        }
        loss_d = (double)loss;
    }
    if (part) {
        if (lane == 0) { red[w][0] = loss_d; red[w][1] = cnt; }
        __syncthreads();
        if (threadIdx.x < 2) {
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < XTR; ++k) acc += red[k][threadIdx.x];
            part[(size_t)blockIdx.x * 2 + threadIdx.x] = acc;
        }
    }
}

// sums = {sum, count} over the n partial pairs in a fixed order (thread t adds pairs t, t + 256, ... then a fixed tree); reduced = sum / count (mean != 0) or sum
__global__ __launch_bounds__(256) void xent_train_sum_kernel(const double* __restrict__ part, long long n, double* __restrict__ sums, float* __restrict__ reduced, int mean) {
    __shared__ double red[2][256];
    double a0 = 0.0, a1 = 0.0;
    for (long long i = threadIdx.x; i < n; i += 256) { a0 += part[(size_t)i * 2]; a1 += part[(size_t)i * 2 + 1]; }
    red[0][threadIdx.x] = a0; red[1][threadIdx.x] = a1;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (threadIdx.x < h) { red[0][threadIdx.x] += red[0][threadIdx.x + h]; red[1][threadIdx.x] += red[1][threadIdx.x + h]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double s = red[0][0], c = red[1][0];
        sums[0] = s; sums[1] = c;
        if (reduced) reduced[0] = (float)(mean ? s / c : s);           // no counted row: 0 / 0 = NaN, as torch
    }
}

template <bool NT>
__global__ __launch_bounds__(256) void xent_train_bwd_kernel(const float* __restrict__ logits, long long ld, const long long* __restrict__ targets,
                                                             const float* __restrict__ lse, const float* __restrict__ grad, int reduction,
                                                             const double* __restrict__ sums, long long rows, int V, float eps, long long ignore_index,
                                                             float* __restrict__ dlogits) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long row = (long long)blockIdx.x * XTR + w;
    if (row >= rows) return;
    f32x4* d = reinterpret_cast<f32x4*>(dlogits + (size_t)row * (size_t)V);
    const long long tg = targets[row];
    if (tg == ignore_index || tg < 0 || tg >= V) {
        const float f = tg == ignore_index ? 0.f : __builtin_nanf("");
        const f32x4 fill = {f, f, f, f};
        for (int c = lane; c < V / 4; c += 64) {
            if (NT) __builtin_nontemporal_store(fill, d + c); else d[c] = fill;
        }
        return;
    }
    float g;
    if (reduction == 0) g = grad[row];
    else if (reduction == 1) g = (float)((double)grad[0] / sums[1]);
    else g = grad[0];
    const f32x4* p = reinterpret_cast<const f32x4*>(logits + (size_t)row * (size_t)ld);
    const float l = lse[row], keep = 1.0f - eps, sm = eps / (float)V;
    const int t = (int)tg;
#pragma unroll 4
    for (int c = lane; c < V / 4; c += 64) {
        const f32x4 v = p[c];
        f32x4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float q = expf(v[k] - l);
            if (4 * c + k == t) q -= keep;
            o[k] = g * (q - sm);
        }
        if (NT) __builtin_nontemporal_store(o, d + c); else d[c] = o;
    }
}

static int check_common(const char* who, const void* logits, long long ld, const void* targets, long long rows, int V, double eps) {
    SDVAR_CHECK_ARG(logits && targets, "%s: null logits or targets", who);
    SDVAR_CHECK_ARG(V >= 4 && V % 4 == 0, "%s: V=%d must be a positive multiple of 4 (float4 loads)", who, V);
    SDVAR_CHECK_ARG(ld >= V && ld % 4 == 0, "%s: row stride ld=%lld must be >= V=%d and a multiple of 4", who, ld, V);
    SDVAR_CHECK_ARG(rows >= 1 && rows <= 0x7FFFFFFFll, "%s: rows=%lld must be in [1, 2^31-1]", who, rows);
    SDVAR_CHECK_ARG(eps >= 0.0 && eps <= 1.0, "%s: label_smoothing=%g must be in [0, 1]", who, eps);       // a NaN fails both comparisons
    SDVAR_CHECK_ARG(((uintptr_t)logits & 15) == 0, "%s: logits must be 16-byte aligned (float4 loads)", who);
    SDVAR_CHECK_ARG(((uintptr_t)targets & 7) == 0, "%s: targets must be 8-byte aligned", who);
    return SDVAR_OK;
}

int xent_train_fwd(const float* logits, long long ld, const long long* targets, long long rows, int V, double eps, long long ignore_index, float* loss, float* lse,
                   double* part, double* sums, float* reduced, int mean, hipStream_t stream) {
    if (int rc = check_common("xent_train_fwd", logits, ld, targets, rows, V, eps)) return rc;
    SDVAR_CHECK_ARG(loss, "xent_train_fwd: null loss");
    SDVAR_CHECK_ARG((part != nullptr) == (sums != nullptr), "xent_train_fwd: part (workspace) and sums go together: both or neither");
    SDVAR_CHECK_ARG(!reduced || sums, "xent_train_fwd: a reduced value needs part and sums");
    SDVAR_CHECK_ARG((((uintptr_t)loss | (uintptr_t)lse | (uintptr_t)reduced) & 3) == 0 && (((uintptr_t)part | (uintptr_t)sums) & 7) == 0,
                    "xent_train_fwd: loss, lse and reduced must be 4-byte aligned, part and sums 8-byte aligned");
    const long long nblk = (rows + XTR - 1) / XTR;
    hipLaunchKernelGGL(xent_train_fwd_kernel, dim3((unsigned)nblk), dim3(64 * XTR), 0, stream, logits, ld, targets, rows, V, (float)eps, ignore_index, loss, lse, part);
    SDVAR_LAUNCH_CHECK();
    if (part) {
        hipLaunchKernelGGL(xent_train_sum_kernel, dim3(1), dim3(256), 0, stream, (const double*)part, nblk, sums, reduced, mean);
        SDVAR_LAUNCH_CHECK();
    }
    return SDVAR_OK;
}

int xent_train_bwd(const float* logits, long long ld, const long long* targets, const float* lse, const float* grad, int reduction, const double* sums, long long rows,
                   int V, double eps, long long ignore_index, float* dlogits, int flags, hipStream_t stream) {
    if (int rc = check_common("xent_train_bwd", logits, ld, targets, rows, V, eps)) return rc;
    SDVAR_CHECK_ARG(lse && grad && dlogits, "xent_train_bwd: null lse, grad or dlogits");
    SDVAR_CHECK_ARG(reduction >= 0 && reduction <= 2, "xent_train_bwd: reduction=%d (0 none, 1 mean, 2 sum)", reduction);
    SDVAR_CHECK_ARG(reduction != 1 || sums, "xent_train_bwd: reduction mean needs the forward's sums");
    SDVAR_CHECK_ARG(((uintptr_t)dlogits & 15) == 0, "xent_train_bwd: dlogits must be 16-byte aligned (float4 stores)");
    SDVAR_CHECK_ARG((((uintptr_t)lse | (uintptr_t)grad) & 3) == 0 && ((uintptr_t)sums & 7) == 0, "xent_train_bwd: lse and grad must be 4-byte aligned, sums 8-byte aligned");
    SDVAR_CHECK_ARG((flags & ~1) == 0, "xent_train_bwd: flags=%d (bit 0: non-temporal stores)", flags);
    const long long nblk = (rows + XTR - 1) / XTR;
    if (flags & 1)
        hipLaunchKernelGGL(xent_train_bwd_kernel<true>, dim3((unsigned)nblk), dim3(64 * XTR), 0, stream, logits, ld, targets, lse, grad, reduction, sums, rows, V, (float)eps,
                           ignore_index, dlogits);
    else
        hipLaunchKernelGGL(xent_train_bwd_kernel<false>, dim3((unsigned)nblk), dim3(64 * XTR), 0, stream, logits, ld, targets, lse, grad, reduction, sums, rows, V, (float)eps,
                           ignore_index, dlogits);
    SDVAR_LAUNCH_CHECK();
    return SDVAR_OK;
}

}  // namespace sdvar
