// The optimizer step of the reference's trainer (AmpOptimizer.backward_clip_step, utils/amp_sc.py:39-75): GradScaler.unscale_, clip_grad_norm_ and AdamW.step over a
// list of float32 tensors as two HBM-bound passes.  The contract is in include/sdvar_hip.h (sdvar_optim_grad_stats, sdvar_optim_adamw_step).
//
//   stats     reads g once: per-workgroup float64 partial of sum g^2 (one workgroup = one chunk of OPT_CH elements of one tensor), written to the workspace
//   finalize  ONE workgroup per launch.  The first launch adds the partials in a fixed order and writes the record {norm, coef, skip, gscale}; every launch advances the
//             step counters of its own tensors by 1 - skip and leaves lr / (1 - beta1^step) and sqrt(1 - beta2^step) per tensor, computed once in float64 (two pow per
//             TENSOR, none per element).  A thread reads and writes only its own tensor's counter; the update kernels never read a counter.
//   update    one read of g, p, m, v, one write of p, m, v; returns at once when the record says skip (one uniform load per workgroup)
// Descriptor lifetime: the descriptors of at most OPT_T tensors travel BY VALUE in the kernel arguments (OptimTable, 3.3 KB of the 4 KB a launch may carry), so nothing a
// launch reads is in memory that a later call could overwrite: two steps enqueued back to back without a sync cannot disturb each other.  blk0 maps a workgroup to its
// (tensor, chunk): tensor t owns workgroups [blk0[t], blk0[t + 1]), found by a binary search over scalar loads.
// No atomics (the partials are added in index order: repeats are bit-identical), no host synchronisation, no allocation.
#include <math.h>
#include <string.h>

#include "../../include/sdvar_hip.h"
#include "common.h"

namespace sdvar {

constexpr int OPT_T = SDVAR_OPTIM_TENSORS_PER_LAUNCH, OPT_CH = SDVAR_OPTIM_CHUNK;
struct OptimTable {
    sdvar_optim_tensor_t t[OPT_T];
    int blk0[OPT_T + 1];
};
static_assert(sizeof(sdvar_optim_tensor_t) == 64 && sizeof(OptimTable) + 96 <= 4096, "the table and the other arguments must fit the 4 KB of kernel arguments");
static_assert(OPT_CH % 1024 == 0, "a chunk is a whole number of 256-thread float4 rounds, so every chunk of an aligned tensor starts 16-byte aligned");

// tensor of workgroup b: blk0[t] <= b < blk0[t + 1] (an empty tensor owns no workgroup and is never returned)
__device__ __forceinline__ int optim_find(const OptimTable& tab, int nt, int b) {
    int lo = 0, hi = nt;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tab.blk0[mid] <= b) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void optim_stats_kernel(const OptimTable tab, int nt, double* __restrict__ part) {
    __shared__ double red[4];
    const int b = blockIdx.x, t = optim_find(tab, nt, b);
    const long long start = (long long)(b - tab.blk0[t]) * OPT_CH, rem = tab.t[t].numel - start;
    const int len = (int)(rem < OPT_CH ? rem : OPT_CH);
    const float* __restrict__ g = tab.t[t].grad + start;
    double acc = 0.0;
    if (((uintptr_t)g & 15) == 0) {
        const f32x4* g4 = reinterpret_cast<const f32x4*>(g);
        const int n4 = len >> 2;
#pragma unroll 4
        for (int i = threadIdx.x; i < n4; i += 256) {
            const f32x4 x = g4[i];
            const double d0 = x[0], d1 = x[1], d2 = x[2], d3 = x[3];
            acc += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
        }
        for (int i = (n4 << 2) + threadIdx.x; i < len; i += 256) { const double d = g[i]; acc += d * d; }
    } else {
        for (int i = threadIdx.x; i < len; i += 256) { const double d = g[i]; acc += d * d; }
    }
    acc = wave_sum_d(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[b] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(256) void optim_finalize_kernel(const OptimTable tab, int nt, int tbase, int do_sum, const double* __restrict__ part, long long npart,
                                                             const float* __restrict__ grad_scale, const float* __restrict__ found_inf, float max_norm, double beta1,
                                                             double beta2, float* rec, float* __restrict__ bc) {
    __shared__ double red[256];
    __shared__ float skip_s;
    if (do_sum) {
        double a = 0.0;
        for (long long i = threadIdx.x; i < npart; i += 256) a += part[i];
        red[threadIdx.x] = a;
        __syncthreads();
        for (int h = 128; h > 0; h >>= 1) {
            if (threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            const float inv_scale = grad_scale ? (float)(1.0 / (double)grad_scale[0]) : 1.0f;
            const float norm = (float)(sqrt(red[0]) * (double)inv_scale);
            const float coef = max_norm <= 0.f ? 1.0f : fminf(1.0f, max_norm / (norm + 1e-6f));
            const bool finite = fabsf(norm) <= 3.4028234663852886e38f;                      // false for inf and for NaN
            const float skip = (!finite || (found_inf && found_inf[0] > 0.f)) ? 1.0f : 0.0f;
            rec[0] = norm; rec[1] = coef; rec[2] = skip; rec[3] = inv_scale * coef;
            skip_s = skip;
        }
    } else if (threadIdx.x == 0) {
        skip_s = rec[2];                    // written by the first finalising launch of this call, earlier on the stream
    }
    __syncthreads();
    const float skip = skip_s;
    if ((int)threadIdx.x < nt && tab.t[threadIdx.x].numel > 0) {
        const sdvar_optim_tensor_t& d = tab.t[threadIdx.x];
        float s = d.step[0];
        if (skip == 0.f) { s += 1.0f; d.step[0] = s; }
        const double bc1 = 1.0 - pow(beta1, (double)s), bc2 = 1.0 - pow(beta2, (double)s);
        bc[2 * (size_t)(tbase + threadIdx.x)] = (float)(d.lr / bc1);
        bc[2 * (size_t)(tbase + threadIdx.x) + 1] = (float)sqrt(bc2);
    }
}

struct AdamCoef { float gs, decay, b1, omb1, b2, omb2, ss, rb, eps; };

// One element.  Every line is ONE float32 operation (-ffp-contract=off keeps them apart), in the order the header states and the tests' error bound counts:
//   g' (1 rounding), p1 (1), m' (3), v' (4), denominator (3: sqrt, /, +), p' (3: /, *, -).
__device__ __forceinline__ void adamw_elem(float g, float& p, float& m, float& v, const AdamCoef& c) {
    const float gp = g * c.gs;
    const float p1 = p * c.decay;
    const float t1 = c.b1 * m;
    const float t2 = c.omb1 * gp;
    const float mn = t1 + t2;
    const float u1 = c.b2 * v;
    const float u2 = c.omb2 * gp;
    const float u3 = u2 * gp;
    const float vn = u1 + u3;
    const float sq = sqrtf(vn);
    const float dn = sq / c.rb;
    const float de = dn + c.eps;
    const float q = mn / de;
    const float r = c.ss * q;
    p = p1 - r;
    m = mn;
    v = vn;
}

__device__ __forceinline__ void adamw_chunk(const float* __restrict__ g, float* __restrict__ p, float* __restrict__ m, float* __restrict__ v, int len, const AdamCoef& c) {
    int i0 = 0;
    if ((((uintptr_t)g | (uintptr_t)p | (uintptr_t)m | (uintptr_t)v) & 15) == 0) {
        const f32x4* g4 = reinterpret_cast<const f32x4*>(g);
        f32x4 *p4 = reinterpret_cast<f32x4*>(p), *m4 = reinterpret_cast<f32x4*>(m), *v4 = reinterpret_cast<f32x4*>(v);
        const int n4 = len >> 2;
#pragma unroll 2
        for (int i = threadIdx.x; i < n4; i += 256) {
            const f32x4 gv = __builtin_nontemporal_load(g4 + i);          // the last read of g in a step: measured 2.5 % faster than a plain load
            f32x4 pv = p4[i], mv = m4[i], vv = v4[i];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float pe = pv[k], me = mv[k], ve = vv[k];
                adamw_elem(gv[k], pe, me, ve, c);
                pv[k] = pe; mv[k] = me; vv[k] = ve;
            }
            p4[i] = pv; m4[i] = mv; v4[i] = vv;
        }
        i0 = n4 << 2;
    }
    for (int i = i0 + threadIdx.x; i < len; i += 256) {          // the numel % 4 tail, or the whole chunk of a tensor with a misaligned pointer
        float pe = p[i], me = m[i], ve = v[i];
        adamw_elem(g[i], pe, me, ve, c);
        p[i] = pe; m[i] = me; v[i] = ve;
    }
}

__global__ __launch_bounds__(256) void optim_adamw_kernel(const OptimTable tab, int nt, int tbase, const float* __restrict__ rec, const float* __restrict__ bc, float b1,
                                                          float omb1, float b2, float omb2, float eps) {
    if (rec[2] != 0.f) return;              // skip: p, m and v keep their bits
    const int b = blockIdx.x, t = optim_find(tab, nt, b);
    const sdvar_optim_tensor_t& d = tab.t[t];
    const long long start = (long long)(b - tab.blk0[t]) * OPT_CH, rem = d.numel - start;
    const int len = (int)(rem < OPT_CH ? rem : OPT_CH);
    AdamCoef c;
    c.gs = rec[3]; c.decay = (float)(1.0 - d.lr * d.weight_decay);
    c.b1 = b1; c.omb1 = omb1; c.b2 = b2; c.omb2 = omb2; c.eps = eps;
    c.ss = bc[2 * (size_t)(tbase + t)]; c.rb = bc[2 * (size_t)(tbase + t) + 1];
    adamw_chunk(d.grad + start, d.param + start, d.exp_avg + start, d.exp_avg_sq + start, len, c);
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------------------------------
static int optim_check(const char* who, const sdvar_optim_tensor_t* ts, int n, double beta1, double beta2, const void* ws, unsigned long long ws_bytes, long long* nblk_out) {
    SDVAR_CHECK_ARG(ts, "%s: null tensor list", who);
    SDVAR_CHECK_ARG(n >= 1, "%s: n=%d tensors; at least 1", who, n);
    SDVAR_CHECK_ARG(beta1 >= 0.0 && beta1 < 1.0, "%s: beta1=%g must be in [0, 1)", who, beta1);          // a NaN fails both comparisons
    SDVAR_CHECK_ARG(beta2 >= 0.0 && beta2 < 1.0, "%s: beta2=%g must be in [0, 1)", who, beta2);
    long long nblk = 0;
    for (int i = 0; i < n; ++i) {
        const sdvar_optim_tensor_t& d = ts[i];
        SDVAR_CHECK_ARG(d.param && d.grad && d.exp_avg && d.exp_avg_sq && d.step, "%s: tensor %d: null %s pointer", who, i,
                        !d.param ? "param" : !d.grad ? "grad" : !d.exp_avg ? "exp_avg" : !d.exp_avg_sq ? "exp_avg_sq" : "step");
        SDVAR_CHECK_ARG((((uintptr_t)d.param | (uintptr_t)d.grad | (uintptr_t)d.exp_avg | (uintptr_t)d.exp_avg_sq | (uintptr_t)d.step) & 3) == 0,
                        "%s: tensor %d: param, grad, exp_avg, exp_avg_sq and step must be 4-byte aligned", who, i);
        SDVAR_CHECK_ARG(d.numel >= 0, "%s: tensor %d: numel=%lld is negative", who, i, (long long)d.numel);
        SDVAR_CHECK_ARG(d.lr >= 0.0, "%s: tensor %d: lr=%g must be >= 0", who, i, d.lr);
        SDVAR_CHECK_ARG(d.weight_decay >= 0.0, "%s: tensor %d: weight_decay=%g must be >= 0", who, i, d.weight_decay);
        nblk += (d.numel + OPT_CH - 1) / OPT_CH;
        SDVAR_CHECK_ARG(nblk <= 0x7FFFFFFFll, "%s: tensor %d: numel=%lld brings the list to more than 2^31 - 1 chunks of %d elements", who, i, (long long)d.numel, OPT_CH);
    }
    const unsigned long long need = 16ull + 8ull * (unsigned long long)n + 8ull * (unsigned long long)nblk;
    SDVAR_CHECK_ARG(ws, "%s: null workspace", who);
    SDVAR_CHECK_ARG(ws_bytes >= need, "%s: workspace of %llu bytes is too small: %d tensors in %lld chunks need %llu", who, ws_bytes, n, nblk, need);
    SDVAR_CHECK_ARG(((uintptr_t)ws & 7) == 0, "%s: workspace must be 8-byte aligned", who);
    *nblk_out = nblk;
    return SDVAR_OK;
}

// the table of tensors [t0, t0 + nt): the descriptors and the first workgroup of each
static int optim_table(const sdvar_optim_tensor_t* ts, int t0, int n, OptimTable* tab) {
    memset(tab, 0, sizeof(*tab));
    const int nt = n - t0 < OPT_T ? n - t0 : OPT_T;
    for (int i = 0; i < nt; ++i) {
        tab->t[i] = ts[t0 + i];
        tab->blk0[i + 1] = tab->blk0[i] + (int)((ts[t0 + i].numel + OPT_CH - 1) / OPT_CH);
    }
    for (int i = nt; i < OPT_T; ++i) tab->blk0[i + 1] = tab->blk0[nt];
    return nt;
}

int optim_grad_stats(const sdvar_optim_tensor_t* ts, int n, const float* grad_scale, const float* found_inf, double max_norm, double beta1, double beta2, void* ws,
                     unsigned long long ws_bytes, hipStream_t stream) {
    const char* who = "optim_grad_stats";
    long long nblk;
    if (int rc = optim_check(who, ts, n, beta1, beta2, ws, ws_bytes, &nblk)) return rc;
    SDVAR_CHECK_ARG(max_norm == max_norm, "%s: max_norm=%g is not a number", who, max_norm);
    SDVAR_CHECK_ARG((((uintptr_t)grad_scale | (uintptr_t)found_inf) & 3) == 0, "%s: grad_scale and found_inf must be 4-byte aligned", who);
    float* rec = (float*)ws;
    float* bc = rec + 4;
    double* part = (double*)((char*)ws + 16 + 8 * (size_t)n);
    OptimTable tab;
    long long pbase = 0;
    for (int t0 = 0; t0 < n; t0 += OPT_T) {
        const int nt = optim_table(ts, t0, n, &tab);
        const int nb = tab.blk0[nt];
        if (nb) {
            hipLaunchKernelGGL(optim_stats_kernel, dim3((unsigned)nb), dim3(256), 0, stream, tab, nt, part + pbase);
            SDVAR_LAUNCH_CHECK();
        }
        pbase += nb;
    }
    for (int t0 = 0; t0 < n; t0 += OPT_T) {
        const int nt = optim_table(ts, t0, n, &tab);
        hipLaunchKernelGGL(optim_finalize_kernel, dim3(1), dim3(256), 0, stream, tab, nt, t0, (int)(t0 == 0), (const double*)part, nblk, grad_scale, found_inf,
                           (float)max_norm, beta1, beta2, rec, bc);
        SDVAR_LAUNCH_CHECK();
    }
    return SDVAR_OK;
}

int optim_adamw_step(const sdvar_optim_tensor_t* ts, int n, double beta1, double beta2, double eps, void* ws, unsigned long long ws_bytes, hipStream_t stream) {
    const char* who = "optim_adamw_step";
    long long nblk;
    if (int rc = optim_check(who, ts, n, beta1, beta2, ws, ws_bytes, &nblk)) return rc;
    SDVAR_CHECK_ARG(eps >= 0.0, "%s: eps=%g must be >= 0", who, eps);
    const float* rec = (const float*)ws;
    const float* bc = rec + 4;
    OptimTable tab;
    for (int t0 = 0; t0 < n; t0 += OPT_T) {
        const int nt = optim_table(ts, t0, n, &tab);
        const int nb = tab.blk0[nt];
        if (!nb) continue;
        hipLaunchKernelGGL(optim_adamw_kernel, dim3((unsigned)nb), dim3(256), 0, stream, tab, nt, t0, rec, bc, (float)beta1, (float)(1.0 - beta1), (float)beta2,
                           (float)(1.0 - beta2), (float)eps);
        SDVAR_LAUNCH_CHECK();
    }
    return SDVAR_OK;
}

}  // namespace sdvar
