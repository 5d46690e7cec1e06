// VQVAE token -> feature accumulation between scales (the quant.py half of the loop), fp32.
// Replaces VectorQuantizer2.embedding + get_next_autoregressive_input + Phi.forward
// (/root/reference/models/quant.py:39, 187-196, 205-206, 223-226; call site models/var.py:205-211):
//     h      = codebook[ids]                         (B, 32, pn, pn)
//     h      = bicubic_up(h, HW)            (stage < S-1)          = Wup h Wup^T   (constant per-stage matrix)
//     h      = 0.5 h + 0.5 (conv3x3(h) + bias)       (shared Phi_k)
//     f_hat += h
//     next   = area_down(f_hat, pn_next)    (stage < S-1)          = Wdn f Wdn^T   (adaptive average pooling)
// Three small launches per stage, each with B*32 workgroups so the serial inter-stage dependency costs microseconds:
//   quant_up_kernel   (image, channel): gather + separable up-sampling           -> up (B,32,HW,HW)
//   quant_phi_kernel  (image, out-channel): Phi conv + residual mix + f_hat +=   -> f_hat (B,32,HW,HW) in place
//   quant_down_kernel (image, channel): separable area pooling, transposed store -> next (B, pn'^2, 32)
#include "common.h"

namespace sdvar {

#define SDVAR_TRY_Q(call) do { int rc_ = (call); if (rc_ != SDVAR_OK) return rc_; } while (0)
constexpr int QMAX_HW = 64;

// up (b, c): tmp[Y][x] = sum_y Wup[Y][y] h[y][x];  out[Y][X] = sum_x tmp[Y][x] Wup[X][x]
// hvec != null: the stage's feature vectors are given directly as (B, pn*pn, Cv) instead of token ids (more_smooth=True mixes the
// codebook softly, models/var.py:206-208)
__global__ __launch_bounds__(256) void quant_up_kernel(const long long* __restrict__ ids, int ids_stride, const float* __restrict__ codebook,
                                                       const float* __restrict__ hvec, const float* __restrict__ Wup, float* __restrict__ up, int pn,
                                                       int HW, int Cv, int identity) {
    extern __shared__ float sm[];
    float* hs = sm;                  // pn*pn
    float* tmp = sm + pn * pn;       // HW*pn
    const int c = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    if (hvec) for (int p = tid; p < pn * pn; p += blockDim.x) hs[p] = hvec[((size_t)b * pn * pn + p) * Cv + c];
    else for (int p = tid; p < pn * pn; p += blockDim.x) hs[p] = codebook[(size_t)ids[(size_t)b * ids_stride + p] * Cv + c];
    __syncthreads();
    float* dst = up + ((size_t)b * Cv + c) * HW * HW;
    if (identity) {                  // last stage: no interpolation (quant.py:193-196)
        for (int p = tid; p < HW * HW; p += blockDim.x) dst[p] = hs[p];
        return;
    }
    for (int e = tid; e < HW * pn; e += blockDim.x) {
        const int Y = e / pn, x = e % pn;
        float acc = 0.f;
        for (int y = 0; y < pn; ++y) acc = fmaf(Wup[Y * pn + y], hs[y * pn + x], acc);
        tmp[e] = acc;
    }
    __syncthreads();
    for (int e = tid; e < HW * HW; e += blockDim.x) {
        const int Y = e / HW, X = e % HW;
        float acc = 0.f;
        for (int x = 0; x < pn; ++x) acc = fmaf(tmp[Y * pn + x], Wup[X * pn + x], acc);
        dst[e] = acc;
    }
}

// phi (b, co): f_hat[b][co] += 0.5*up[b][co] + 0.5*(bias[co] + sum_{ci,dy,dx} w[co][ci][dy][dx] up[b][ci][Y+dy-1][X+dx-1])
// f_out = f_in + Phi mix (f_in == f_out: the in-place form of quant.py:191; distinct buffers keep the per-stage snapshots of a draft round
// without extra copies)
// STAGED: the image's up-sampled planes (Cv HW^2 floats: 32 KB at HW = 16, 128 KB at 32) and the output channel's 9 Cv weights are copied to LDS
// first - every one of them is read HW^2 / 9 times by the workgroup - and the 288 multiply-adds of a pixel (same order as the unstaged form, so the
// results are the same bits) read LDS: 31.6 -> 7 us per launch at HW = 16, on the serial path between two stages.
template <bool STAGED>
__global__ __launch_bounds__(256) void quant_phi_kernel(const float* __restrict__ up, const float* __restrict__ w, const float* __restrict__ bias,
                                                        const float* f_in, float* f_hat, int HW, int Cv) {
    extern __shared__ __attribute__((aligned(16))) float psm[];
    const int co = blockIdx.x, b = blockIdx.y;
    const float* ub = up + (size_t)b * Cv * HW * HW;
    const float* wc = w + (size_t)co * Cv * 9;
    if (STAGED) {
        const int n4 = Cv * HW * HW / 4;                // HW * HW is a multiple of 4 on this path (host)
        for (int i = threadIdx.x; i < n4; i += blockDim.x) reinterpret_cast<f32x4*>(psm)[i] = reinterpret_cast<const f32x4*>(ub)[i];
        for (int i = threadIdx.x; i < 9 * Cv; i += blockDim.x) psm[Cv * HW * HW + i] = wc[i];
        __syncthreads();
        ub = psm; wc = psm + Cv * HW * HW;
    }
    for (int e = threadIdx.x; e < HW * HW; e += blockDim.x) {
        const int Y = e / HW, X = e % HW;
        float acc = 0.f;
        for (int ci = 0; ci < Cv; ++ci) {
            const float* uc = ub + (size_t)ci * HW * HW;
            const float* wk = wc + ci * 9;
#pragma unroll
            for (int dy = 0; dy < 3; ++dy) {
                const int yy = Y + dy - 1;
                if (yy < 0 || yy >= HW) continue;
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) {
                    const int xx = X + dx - 1;
                    if (xx < 0 || xx >= HW) continue;
                    acc = fmaf(wk[dy * 3 + dx], uc[yy * HW + xx], acc);
                }
            }
        }
        const float h = ub[(size_t)co * HW * HW + e];
        const float mixed = h * 0.5f + (acc + bias[co]) * 0.5f;
        const size_t o = ((size_t)b * Cv + co) * HW * HW + e;
        f_hat[o] = f_in[o] + mixed;
    }
}

// down (b, c): tmp[y'][X] = sum_Y Wdn[y'][Y] f[Y][X];  next[b][y'*pn2 + x'][c] = sum_X tmp[y'][X] Wdn[x'][X]
__global__ __launch_bounds__(256) void quant_down_kernel(const float* __restrict__ f_hat, const float* __restrict__ Wdn, float* __restrict__ nxt,
                                                         int HW, int pn2, int Cv) {
    extern __shared__ float sm[];
    float* fs = sm;                  // HW*HW
    float* tmp = sm + HW * HW;       // pn2*HW
    const int c = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const float* src = f_hat + ((size_t)b * Cv + c) * HW * HW;
    for (int p = tid; p < HW * HW; p += blockDim.x) fs[p] = src[p];
    __syncthreads();
    for (int e = tid; e < pn2 * HW; e += blockDim.x) {
        const int y2 = e / HW, X = e % HW;
        float acc = 0.f;
        for (int Y = 0; Y < HW; ++Y) acc = fmaf(Wdn[y2 * HW + Y], fs[Y * HW + X], acc);
        tmp[e] = acc;
    }
    __syncthreads();
    for (int e = tid; e < pn2 * pn2; e += blockDim.x) {
        const int y2 = e / pn2, x2 = e % pn2;
        float acc = 0.f;
        for (int X = 0; X < HW; ++X) acc = fmaf(tmp[y2 * HW + X], Wdn[x2 * HW + X], acc);
        nxt[((size_t)b * pn2 * pn2 + e) * Cv + c] = acc;
    }
}

int quant_next(const long long* ids, int ids_stride, const float* hvec, const float* codebook, const float* Wup, const float* phi_w, const float* phi_b,
               const float* Wdn, float* up_scratch, const float* f_in, float* f_hat, float* nxt, int B, int pn, int pn_next, int HW, int Cv, int last,
               hipStream_t stream) {
    SDVAR_CHECK_ARG((ids || hvec) && codebook && phi_w && phi_b && up_scratch && f_hat, "quant_next: null operand");
    SDVAR_CHECK_ARG(B > 0 && pn > 0 && pn <= HW && HW <= QMAX_HW && (!last || pn == HW), "quant_next: bad sizes pn=%d HW=%d", pn, HW);
    const size_t lds_up = (size_t)(pn * pn + HW * pn) * sizeof(float);
    hipLaunchKernelGGL(quant_up_kernel, dim3(Cv, B), dim3(256), lds_up, stream, ids, ids_stride, codebook, hvec, Wup, up_scratch, pn, HW, Cv, last);
    SDVAR_LAUNCH_CHECK();
    const size_t lds_phi = ((size_t)Cv * HW * HW + 9 * (size_t)Cv) * sizeof(float);
    if ((HW * HW) % 4 == 0 && lds_phi <= 140 * 1024 && ((uintptr_t)up_scratch % 16) == 0) {
        static LdsOptIn opt_in;
        SDVAR_LDS_OPT_IN(opt_in, 140 * 1024, (const void*)quant_phi_kernel<true>);       // once per device: the largest size this path takes
        hipLaunchKernelGGL(quant_phi_kernel<true>, dim3(Cv, B), dim3(256), lds_phi, stream, up_scratch, phi_w, phi_b, f_in ? f_in : f_hat, f_hat, HW, Cv);
    } else hipLaunchKernelGGL(quant_phi_kernel<false>, dim3(Cv, B), dim3(256), 0, stream, up_scratch, phi_w, phi_b, f_in ? f_in : f_hat, f_hat, HW, Cv);
    SDVAR_LAUNCH_CHECK();
    if (!last) {
        SDVAR_CHECK_ARG(Wdn && nxt && pn_next > 0 && pn_next <= HW, "quant_next: missing down table");
        const size_t lds_dn = (size_t)(HW * HW + pn_next * HW) * sizeof(float);
        hipLaunchKernelGGL(quant_down_kernel, dim3(Cv, B), dim3(256), lds_dn, stream, f_hat, Wdn, nxt, HW, pn_next, Cv);
        SDVAR_LAUNCH_CHECK();
    }
    return SDVAR_OK;
}

// ---------------------------------------------------------------------------------------------------- encoding (f_to_idxBl_or_fhat, quant.py:135-166)
// Per scale si of the residual quantisation (using_znorm = False):
//     z       = area_down(f_rest, pn_si) as rows (B pn^2, 32)      quant_down_kernel (the last scale: f_rest itself, quant_rows_kernel)
//     idx     = argmin_v |z|^2 + |e_v|^2 - 2 z.e_v                   quant_nearest_kernel (fp32, ties -> lowest index as torch.argmin)
//     h       = Phi(bicubic_up(codebook[idx]))                       quant_up_kernel + quant_phi_rest_kernel
//     f_hat  += h,  f_rest -= h                                      (both in the phi launch; f_rest is its own tensor as quant.py:162-163)

// |e_v|^2 (sequential fp32 chain over the channels), once at bind
__global__ __launch_bounds__(256) void quant_code_norms_kernel(const float* __restrict__ codebook, float* __restrict__ e2, int V, int Cv) {
    for (int v = blockIdx.x * blockDim.x + threadIdx.x; v < V; v += gridDim.x * blockDim.x) {
        const float* e = codebook + (size_t)v * Cv;
        float a = 0.f;
        for (int c = 0; c < Cv; ++c) a = fmaf(e[c], e[c], a);
        e2[v] = a;
    }
}

// Nearest code for QN_ROWS rows of z (N, 32) per workgroup.  Thread t scans the codes t, t + 256, ... in increasing order (strict < keeps the
// first of equal distances), holding the rows' |z|^2 and the 32 channels of the code in registers: 32 FMAs per row and code, the rows broadcast
// from LDS.  The (d, v) pairs are reduced lexicographically across the wave (DPP-free shuffles) and the 4 waves (LDS).  Output row n = b P + p
// goes to ids[b ids_stride + p].  The codebook (512 KB at V = 4096) is read from L2 by every workgroup.
constexpr int QN_ROWS = 8;
__device__ __forceinline__ void qn_better(float& d, int& v, float d2, int v2) {
    if (d2 < d || (d2 == d && v2 < v) || (d != d && d2 == d2)) { d = d2; v = v2; }     // NaN distances lose to any number
}
__global__ __launch_bounds__(256) void quant_nearest_kernel(const float* __restrict__ z, const float* __restrict__ codebook, const float* __restrict__ e2,
                                                            long long* __restrict__ ids, int N, int P, int ids_stride, int V) {
    __shared__ __attribute__((aligned(16))) float zs[QN_ROWS][32];
    __shared__ float z2s[QN_ROWS];
    __shared__ float rd[4][QN_ROWS];
    __shared__ int rv[4][QN_ROWS];
    const int n0 = blockIdx.x * QN_ROWS, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nr = N - n0 < QN_ROWS ? N - n0 : QN_ROWS;
    for (int i = tid; i < QN_ROWS * 32; i += 256) zs[i >> 5][i & 31] = (i >> 5) < nr ? z[(size_t)(n0 + (i >> 5)) * 32 + (i & 31)] : 0.f;
    __syncthreads();
    if (tid < QN_ROWS) {
        float a = 0.f;
        for (int c = 0; c < 32; ++c) a = fmaf(zs[tid][c], zs[tid][c], a);
        z2s[tid] = a;
    }
    __syncthreads();
    float bd[QN_ROWS]; int bv[QN_ROWS];
#pragma unroll
    for (int r = 0; r < QN_ROWS; ++r) { bd[r] = INFINITY; bv[r] = 0x7fffffff; }
    for (int v = tid; v < V; v += 256) {
        f32x4 e[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) e[k] = *reinterpret_cast<const f32x4*>(codebook + (size_t)v * 32 + 4 * k);
        const float ev = e2[v];
#pragma unroll
        for (int r = 0; r < QN_ROWS; ++r) {
            float dot = 0.f;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const f32x4 zq = *reinterpret_cast<const f32x4*>(&zs[r][4 * k]);
#pragma unroll
                for (int j = 0; j < 4; ++j) dot = fmaf(zq[j], e[k][j], dot);
            }
            const float d = (z2s[r] + ev) - 2.0f * dot;
            if (d < bd[r] || (bd[r] != bd[r] && d == d) || bv[r] == 0x7fffffff) { bd[r] = d; bv[r] = v; }
        }
    }
#pragma unroll
    for (int r = 0; r < QN_ROWS; ++r) {
        float d = bd[r]; int vv = bv[r];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const float d2 = __shfl_xor(d, off, 64);
            const int v2 = __shfl_xor(vv, off, 64);
            qn_better(d, vv, d2, v2);
        }
        if (lane == 0) { rd[wave][r] = d; rv[wave][r] = vv; }
    }
    __syncthreads();
    if (tid < nr) {
        float d = rd[0][tid]; int vv = rv[0][tid];
        for (int w = 1; w < 4; ++w) qn_better(d, vv, rd[w][tid], rv[w][tid]);
        const int n = n0 + tid, b = n / P, p = n - b * P;
        ids[(size_t)b * ids_stride + p] = vv;
    }
}

// f_rest (B, Cv, HW, HW) -> rows (B HW^2, Cv)
__global__ __launch_bounds__(256) void quant_rows_kernel(const float* __restrict__ f, float* __restrict__ z, int B, int HW, int Cv) {
    const size_t total = (size_t)B * HW * HW * Cv;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % Cv);
        const size_t row = i / Cv;
        const int p = (int)(row % ((size_t)HW * HW)), b = (int)(row / ((size_t)HW * HW));
        z[i] = f[((size_t)b * Cv + c) * HW * HW + p];
    }
}

// quant_phi_kernel with both accumulators: h = 0.5 up + 0.5 (conv3x3(up) + bias); f_hat += h; f_rest -= h (same multiply-add order as quant_phi_kernel)
template <bool STAGED>
__global__ __launch_bounds__(256) void quant_phi_rest_kernel(const float* __restrict__ up, const float* __restrict__ w, const float* __restrict__ bias,
                                                             float* __restrict__ f_hat, float* __restrict__ f_rest, int HW, int Cv) {
    extern __shared__ __attribute__((aligned(16))) float psm[];
    const int co = blockIdx.x, b = blockIdx.y;
    const float* ub = up + (size_t)b * Cv * HW * HW;
    const float* wc = w + (size_t)co * Cv * 9;
    if (STAGED) {
        const int n4 = Cv * HW * HW / 4;
        for (int i = threadIdx.x; i < n4; i += blockDim.x) reinterpret_cast<f32x4*>(psm)[i] = reinterpret_cast<const f32x4*>(ub)[i];
        for (int i = threadIdx.x; i < 9 * Cv; i += blockDim.x) psm[Cv * HW * HW + i] = wc[i];
        __syncthreads();
        ub = psm; wc = psm + Cv * HW * HW;
    }
    for (int e = threadIdx.x; e < HW * HW; e += blockDim.x) {
        const int Y = e / HW, X = e % HW;
        float acc = 0.f;
        for (int ci = 0; ci < Cv; ++ci) {
            const float* uc = ub + (size_t)ci * HW * HW;
            const float* wk = wc + ci * 9;
#pragma unroll
            for (int dy = 0; dy < 3; ++dy) {
                const int yy = Y + dy - 1;
                if (yy < 0 || yy >= HW) continue;
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) {
                    const int xx = X + dx - 1;
                    if (xx < 0 || xx >= HW) continue;
                    acc = fmaf(wk[dy * 3 + dx], uc[yy * HW + xx], acc);
                }
            }
        }
        const float h = ub[(size_t)co * HW * HW + e];
        const float mixed = h * 0.5f + (acc + bias[co]) * 0.5f;
        const size_t o = ((size_t)b * Cv + co) * HW * HW + e;
        f_hat[o] = f_hat[o] + mixed;
        f_rest[o] = f_rest[o] - mixed;
    }
}

int quant_code_norms(const float* codebook, float* e2, int V, int Cv, hipStream_t stream) {
    SDVAR_CHECK_ARG(codebook && e2 && V >= 1 && Cv >= 1, "quant_code_norms: bad arguments");
    hipLaunchKernelGGL(quant_code_norms_kernel, dim3((V + 255) / 256), dim3(256), 0, stream, codebook, e2, V, Cv);
    SDVAR_LAUNCH_CHECK();
    return SDVAR_OK;
}

int quant_nearest(const float* z, int N, int P, const float* codebook, const float* e2, int V, int Cv, long long* ids, int ids_stride, hipStream_t stream) {
    SDVAR_CHECK_ARG(z && codebook && e2 && ids && N >= 1 && P >= 1 && V >= 1, "quant_nearest: bad arguments (N %d V %d)", N, V);
    SDVAR_CHECK_ARG(Cv == 32, "quant_nearest: Cvae %d (the kernel holds 32 channels per code)", Cv);
    SDVAR_CHECK_ARG(((uintptr_t)codebook % 16) == 0, "quant_nearest: the codebook must be 16-byte aligned");
    hipLaunchKernelGGL(quant_nearest_kernel, dim3((N + QN_ROWS - 1) / QN_ROWS), dim3(256), 0, stream, z, codebook, e2, ids, N, P, ids_stride, V);
    SDVAR_LAUNCH_CHECK();
    return SDVAR_OK;
}

// one scale of the residual quantisation.  Wdn_si: area table HW -> pn (null at the last scale, pn == HW).  ids: this scale's first id, row stride ids_stride.
int quant_encode_stage(float* f_rest, float* f_hat, float* z, float* up_scratch, const float* codebook, const float* e2, const float* Wdn_si, const float* Wup_si,
                       const float* phi_w, const float* phi_b, long long* ids, int ids_stride, int B, int pn, int HW, int V, int Cv, int last, hipStream_t stream) {
    SDVAR_CHECK_ARG(f_rest && f_hat && z && up_scratch && codebook && e2 && phi_w && phi_b && ids, "quant_encode: null operand");
    SDVAR_CHECK_ARG(B > 0 && pn > 0 && pn <= HW && HW <= QMAX_HW && (!last || pn == HW) && (last || (Wdn_si && Wup_si)), "quant_encode: bad sizes pn=%d HW=%d", pn, HW);
    if (last) {
        const size_t total = (size_t)B * HW * HW * Cv;
        hipLaunchKernelGGL(quant_rows_kernel, dim3((unsigned)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048)), dim3(256), 0, stream, f_rest, z, B, HW, Cv);
    } else {
        const size_t lds_dn = (size_t)(HW * HW + pn * HW) * sizeof(float);
        hipLaunchKernelGGL(quant_down_kernel, dim3(Cv, B), dim3(256), lds_dn, stream, f_rest, Wdn_si, z, HW, pn, Cv);
    }
    SDVAR_LAUNCH_CHECK();
    SDVAR_TRY_Q(quant_nearest(z, B * pn * pn, pn * pn, codebook, e2, V, Cv, ids, ids_stride, stream));
    const size_t lds_up = (size_t)(pn * pn + HW * pn) * sizeof(float);
    hipLaunchKernelGGL(quant_up_kernel, dim3(Cv, B), dim3(256), lds_up, stream, ids, ids_stride, codebook, nullptr, Wup_si, up_scratch, pn, HW, Cv, last);
    SDVAR_LAUNCH_CHECK();
    const size_t lds_phi = ((size_t)Cv * HW * HW + 9 * (size_t)Cv) * sizeof(float);
    if ((HW * HW) % 4 == 0 && lds_phi <= 140 * 1024 && ((uintptr_t)up_scratch % 16) == 0) {
        static LdsOptIn opt_in;
        SDVAR_LDS_OPT_IN(opt_in, 140 * 1024, (const void*)quant_phi_rest_kernel<true>);
        hipLaunchKernelGGL(quant_phi_rest_kernel<true>, dim3(Cv, B), dim3(256), lds_phi, stream, up_scratch, phi_w, phi_b, f_hat, f_rest, HW, Cv);
    } else hipLaunchKernelGGL(quant_phi_rest_kernel<false>, dim3(Cv, B), dim3(256), 0, stream, up_scratch, phi_w, phi_b, f_hat, f_rest, HW, Cv);
    SDVAR_LAUNCH_CHECK();
    return SDVAR_OK;
}

// ---------------------------------------------------------------------------------------------------- statistics (VectorQuantizer2.forward, quant.py:77, 95, 98)
// The numbers the reference's forward() reports besides f_hat, and the image error of a reconstruction: sums over a pair of equally shaped fp32 tensors.
//     d        = a - b in fp32 (the tensor F.mse_loss squares)
//     part     {sum |d|, sum d^2} of one workgroup, in fp64: a thread adds its 16-byte chunks i, i + grid, ... in that order, the 64 lanes of a wave are
//              added by a butterfly (wave_sum_d), the 4 waves through LDS in wave order -> one partial per workgroup
//     sums     diff_stats_sum_kernel: thread t adds the partials t, t + 256, ... and a fixed tree adds the 256 threads.  The grid is a function of n alone
//              and nothing is an atomic, so two calls give the same bits.
//     st       (optional) d + b: the straight-through f_hat of quant.py:98, (f_hat - f) + f, from the values this pass has in registers anyway
// HBM/L2-bound: 8 bytes read (+ 4 written) per element.
constexpr int DS_MAX_BLOCKS = 1024;                    // 4 workgroups per CU on 256 CUs; beyond that a thread loops

__global__ __launch_bounds__(256) void diff_stats_kernel(const float* __restrict__ a, const float* __restrict__ b, size_t n4, size_t n, float* __restrict__ st,
                                                         double* __restrict__ part) {
    __shared__ double red[4][2];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const size_t stride = (size_t)gridDim.x * 256, t0 = (size_t)blockIdx.x * 256 + threadIdx.x;
    double s1 = 0.0, s2 = 0.0;
    for (size_t i = t0; i < n4; i += stride) {
        const f32x4 va = reinterpret_cast<const f32x4*>(a)[i], vb = reinterpret_cast<const f32x4*>(b)[i];
        const f32x4 d = va - vb;
#pragma unroll
        for (int k = 0; k < 4; ++k) { s1 += (double)fabsf(d[k]); s2 += (double)d[k] * (double)d[k]; }
        if (st) reinterpret_cast<f32x4*>(st)[i] = d + vb;
    }
    for (size_t i = 4 * n4 + t0; i < n; i += stride) {           // the elements past the last whole chunk (all of them when a pointer is not 16-byte aligned)
        const float vb = b[i], d = a[i] - vb;
        s1 += (double)fabsf(d); s2 += (double)d * (double)d;
        if (st) st[i] = d + vb;
    }
    s1 = wave_sum_d(s1); s2 = wave_sum_d(s2);
    if (lane == 0) { red[w][0] = s1; red[w][1] = s2; }
    __syncthreads();
    if (threadIdx.x < 2) part[(size_t)blockIdx.x * 2 + threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// workgroup g: out[g ncomp + k] (+)= sum over the nblk partial rows of part[g group_stride + 2 i + comp0 + k], k < ncomp <= 2, in a fixed order
__global__ __launch_bounds__(256) void diff_stats_sum_kernel(const double* __restrict__ part, int nblk, size_t group_stride, int comp0, int ncomp, double* __restrict__ out,
                                                             int accumulate) {
    __shared__ double red[2][256];
    const double* p = part + (size_t)blockIdx.x * group_stride;
    double acc[2] = {0.0, 0.0};
    for (int i = threadIdx.x; i < nblk; i += 256)
        for (int k = 0; k < ncomp; ++k) acc[k] += p[(size_t)i * 2 + comp0 + k];
    red[0][threadIdx.x] = acc[0]; red[1][threadIdx.x] = acc[1];
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (threadIdx.x < h) { red[0][threadIdx.x] += red[0][threadIdx.x + h]; red[1][threadIdx.x] += red[1][threadIdx.x + h]; }
        __syncthreads();
    }
    if ((int)threadIdx.x < ncomp) {
        double* o = out + (size_t)blockIdx.x * ncomp + threadIdx.x;
        *o = (accumulate ? *o : 0.0) + red[threadIdx.x][0];
    }
}

int diff_stats_blocks(size_t n) {
    const size_t nb = (n / 4 + 255) / 256;
    return (int)(nb < 1 ? 1 : (nb > (size_t)DS_MAX_BLOCKS ? (size_t)DS_MAX_BLOCKS : nb));
}

// part: 2 * diff_stats_blocks(n) doubles
int diff_stats_partials(const float* a, const float* b, size_t n, float* st, double* part, hipStream_t stream) {
    SDVAR_CHECK_ARG(a && b && part && n >= 1, "diff_stats: null operand or n = 0");
    const bool vec = (((uintptr_t)a | (uintptr_t)b | (uintptr_t)st) & 15) == 0;
    hipLaunchKernelGGL(diff_stats_kernel, dim3(diff_stats_blocks(n)), dim3(256), 0, stream, a, b, vec ? n / 4 : (size_t)0, n, st, part);
    SDVAR_LAUNCH_CHECK();
    return SDVAR_OK;
}

int diff_stats_sum(const double* part, int nblk, int groups, size_t group_stride, int comp0, int ncomp, double* out, int accumulate, hipStream_t stream) {
    SDVAR_CHECK_ARG(part && out && nblk >= 1 && groups >= 1 && comp0 >= 0 && ncomp >= 1 && comp0 + ncomp <= 2, "diff_stats_sum: bad arguments");
    hipLaunchKernelGGL(diff_stats_sum_kernel, dim3(groups), dim3(256), 0, stream, part, nblk, group_stride, comp0, ncomp, out, accumulate);
    SDVAR_LAUNCH_CHECK();
    return SDVAR_OK;
}

// The partials of img_err_stats: one buffer per (host thread, device), allocated on the device that is current at the call and kept for the thread's life
// (sdvar_hip.h threading contract; calls of one thread on one device share it, so they must be on one stream or ordered by the caller).
constexpr int DS_MAX_DEVICES = 64;
static thread_local double* g_ds_part[DS_MAX_DEVICES] = {};

int img_err_stats(const float* a, const float* b, size_t n, double* sums, int accumulate, hipStream_t stream) {
    SDVAR_CHECK_ARG(a && b && sums && n >= 1, "img_err_stats: null operand or n = 0");
    int dev = 0;
    SDVAR_HIP(hipGetDevice(&dev));
    SDVAR_CHECK_ARG(dev >= 0 && dev < DS_MAX_DEVICES, "img_err_stats: device %d", dev);
    if (!g_ds_part[dev]) SDVAR_HIP(hipMalloc((void**)&g_ds_part[dev], (size_t)DS_MAX_BLOCKS * 2 * sizeof(double)));
    SDVAR_TRY_Q(diff_stats_partials(a, b, n, nullptr, g_ds_part[dev], stream));
    return diff_stats_sum(g_ds_part[dev], diff_stats_blocks(n), 1, 0, 0, 2, sums, accumulate, stream);
}

// hits[s][v] += 1 for every id v of scale s (ids (B, L), scale s = tokens [end[s-1], end[s]) of a row).  Integer atomics: the counts do not depend on
// the order; an id outside [0, V) (all-NaN distances) is not counted.
struct QuantScaleEnds { int end[16]; };
__global__ __launch_bounds__(256) void quant_hits_kernel(const long long* __restrict__ ids, int B, int L, int S, QuantScaleEnds e, int V, int* __restrict__ hits) {
    const int total = B * L;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int p = i % L;
        int s = 0;
        while (s < S - 1 && p >= e.end[s]) ++s;
        const long long id = ids[i];
        if (id >= 0 && id < V) atomicAdd(hits + (size_t)s * V + id, 1);
    }
}

int quant_hits(const long long* ids, int B, int L, int S, const int* pn, int V, int* hits, hipStream_t stream) {
    SDVAR_CHECK_ARG(ids && hits && pn && B >= 1 && S >= 1 && S <= 16 && V >= 1 && (size_t)B * L <= 0x7FFFFFFF, "quant_hits: bad arguments");
    QuantScaleEnds e;
    int acc = 0;
    for (int s = 0; s < 16; ++s) { if (s < S) acc += pn[s] * pn[s]; e.end[s] = acc; }
    SDVAR_CHECK_ARG(acc == L, "quant_hits: L %d != sum pn^2 %d", L, acc);
    SDVAR_HIP(hipMemsetAsync(hits, 0, (size_t)S * V * sizeof(int), stream));
    const int total = B * L;
    hipLaunchKernelGGL(quant_hits_kernel, dim3((total + 255) / 256 < 1024 ? (total + 255) / 256 : 1024), dim3(256), 0, stream, ids, B, L, S, e, V, hits);
    SDVAR_LAUNCH_CHECK();
    return SDVAR_OK;
}

}  // namespace sdvar
