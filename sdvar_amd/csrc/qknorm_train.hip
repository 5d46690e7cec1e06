// What SelfAttention.forward does between the QKV GEMM and the attention call when attn_l2_norm is on (basic_var.py:93-105), under autograd, both directions:
//
//   xq = qkv[.., 0, ..] + q_bias,  xk = qkv[.., 1, ..],  s_h = expf(min(scale_log[h], max_log))
//   q = (xq / max(|xq|, 1e-12)) * s_h,   k = xk / max(|xk|, 1e-12),   v = qkv[.., 2, ..] + v_bias       (norms per head of 64 channels; v written only with a v_bias)
//
// HBM-bound row kernels: one wave64 per row (b, l) of the dense (B, L, 3, H, 64) buffer, fp32 / fp16 / bf16 (dtype codes 0 / 1 / 2), widened to fp32 before any
// arithmetic.  Lane map: a step covers 4 heads; in step t lane i holds channels 4 (i % 16) .. + 3 of head 4 t + i / 16 - 16 bytes of fp32 or 8 bytes of half per lane,
// a head = 16 consecutive lanes (one DPP row).  H need not be a multiple of 4: the 16-lane groups past H load and store nothing and carry zeros.
// Sum of squares of a head: the lane's four products added left to right, then four cross-lane levels (xor 8, 4, 2, 1) inside the 16-lane group; the order is fixed, so
// the backward recomputes the forward's norm - and x / max(norm, eps) - bit for bit and nothing but qkv, the biases and scale_log is saved.
//
//   backward, n = max(|x|, eps), xh = x / n, g the upstream gradient of q resp. k (fp32, (b, h, l) strides):
//       |x| >= eps: dx = (s / n) (g - xh (xh . g))      else: dx = (s g) / eps          (k: s = 1)
//       dqkv (B, L, 3, H, 64) in qkv's dtype = [dx_q, dx_k, dv]: every slot written by the one kernel (an absent gradient is a zero slot)
//       dscale_log[h] = [scale_log[h] <= max_log] sum_{b, l, c in h} g q,   dq_bias[c] = sum_{b, l} dx_q,   dv_bias[c] = sum_{b, l} dv        (fp32)
//
// The sums are the two-pass fixed-order column sums of adaln_train.hip.  Pass 1: a workgroup owns 4 heads of QKN_CHUNK = 32 consecutive rows of ONE image, wave w takes rows
// w, w + 4, ..., the four waves are added through LDS as ((w0 + w1) + w2) + w3 into the workspace [b][chunk][3][C].  Pass 2: slice s of 4 adds the partial rows
// s, s + 4, ... of all images in index order, the slices are added as ((s0 + s1) + s2) + s3; the per-head sum adds its 64 column sums by six wave levels.
// No atomics, no scratch, nothing clamped (an fp16 overflow of dqkv is +-inf), no allocation and no host synchronisation; repeats are bit-identical.
#include <type_traits>

#include "common.h"

namespace sdvar {

namespace {

constexpr int QKN_MAX_H = 48;
constexpr int QKN_CHUNK = 32;          // rows of one image per workgroup of the backward kernel (8 per wave): adaln_train.hip's TRAIN_CHUNK
constexpr float QKN_EPS = 1e-12f;      // F.normalize's eps

template <bool HF>
__device__ __forceinline__ f32x4 qkn_load4(const void* __restrict__ p, int dt, size_t e) {
    if (!HF) return *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(p) + e);
    const uint2 w = *reinterpret_cast<const uint2*>(reinterpret_cast<const uint16_t*>(p) + e);
    const bool bf = dt == 2;
    return f32x4{half_lo(w.x, bf), half_hi(w.x, bf), half_lo(w.y, bf), half_hi(w.y, bf)};
}
template <bool HF>
__device__ __forceinline__ void qkn_store4(void* __restrict__ p, int dt, size_t e, f32x4 v) {
    if (!HF) { *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(p) + e) = v; return; }
    const bool bf = dt == 2;
    *reinterpret_cast<uint2*>(reinterpret_cast<uint16_t*>(p) + e) = uint2{half_pack2(v[0], v[1], bf), half_pack2(v[2], v[3], bf)};
}

// the sum over the 16 lanes of a head; every lane of the group gets it.  Called by all 64 lanes.
__device__ __forceinline__ float group16_sum(float v) {
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float dot4(f32x4 a, f32x4 b) { return ((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]) + a[3] * b[3]; }
// |x| of the head this lane's group holds: both directions go through here
__device__ __forceinline__ float head_norm(f32x4 x) { return sqrtf(group16_sum(dot4(x, x))); }
// s_h of head `lane` (lanes past H: 0), fetched per step with a shuffle: one expf per wave
__device__ __forceinline__ float lane_scale(const float* __restrict__ scale_log, float max_log, int lane, int H) {
    return lane < H ? expf(fminf(scale_log[lane], max_log)) : 0.f;
}

// ------------------------------------------------------------------------------------------------ forward
template <bool HF>
__global__ __launch_bounds__(256) void qknorm_fwd_kernel(const void* __restrict__ qkv, int dt, const float* __restrict__ q_bias, const float* __restrict__ v_bias,
                                                         const float* __restrict__ scale_log, float max_log, float* __restrict__ q, float* __restrict__ k,
                                                         void* __restrict__ v, int rows, int H) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;          // wave-uniform
    const int C = H * 64, sub = lane >> 4, c4 = (lane & 15) * 4;
    const float s_lane = lane_scale(scale_log, max_log, lane, H);
    const size_t ri = (size_t)row * 3 * (size_t)C, ro = (size_t)row * (size_t)C;
    for (int h0 = 0; h0 < H; h0 += 4) {
        const int h = h0 + sub, co = h * 64 + c4;
        const bool act = h < H;
        const float s = __shfl(s_lane, h, 64);
        f32x4 xq = {0.f, 0.f, 0.f, 0.f}, xk = {0.f, 0.f, 0.f, 0.f};
        if (act) {
            xq = qkn_load4<HF>(qkv, dt, ri + co);
            xk = qkn_load4<HF>(qkv, dt, ri + C + co);
            if (q_bias) xq = xq + *reinterpret_cast<const f32x4*>(q_bias + co);
        }
        const float dq = fmaxf(head_norm(xq), QKN_EPS), dk = fmaxf(head_norm(xk), QKN_EPS);
        if (act) {
            f32x4 oq, ok;
#pragma unroll
            for (int e = 0; e < 4; ++e) { oq[e] = (xq[e] / dq) * s; ok[e] = xk[e] / dk; }
            *reinterpret_cast<f32x4*>(q + ro + co) = oq;
            *reinterpret_cast<f32x4*>(k + ro + co) = ok;
            if (v_bias) qkn_store4<HF>(v, dt, ro + co, qkn_load4<HF>(qkv, dt, ri + 2 * C + co) + *reinterpret_cast<const f32x4*>(v_bias + co));
        }
    }
}

// ------------------------------------------------------------------------------------------------ backward, pass 1
struct QknStrides { long long qb, qh, ql, kb, kh, kl, vb, vh, vl; };

// grid (B * nchunk, ceil(H / 4)): a workgroup owns ONE step of 4 heads of its 32 rows, so the column sums a lane carries are three float4 whatever H is, a wave reads
// 1 KB (fp32) per row and slot, and there are enough workgroups to fill the machine at the training shapes (B 8, L 680, H 16: 704).
// need_q / need_k / need_v (wave-uniform): the gradient is given AND something asked for depends on it
template <bool HF>
__global__ __launch_bounds__(256) void qknorm_bwd_kernel(const void* __restrict__ qkv, int dt, const float* __restrict__ q_bias, const float* __restrict__ scale_log,
                                                         float max_log, const float* __restrict__ gq, const float* __restrict__ gk, const void* __restrict__ gv,
                                                         QknStrides st, void* __restrict__ dqkv, float* __restrict__ ws, int need_q, int need_k, int need_v, int L,
                                                         int H, int nchunk) {
    __shared__ f32x4 red[3][4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int b = blockIdx.x / nchunk, ch = blockIdx.x - b * nchunk;
    const int C = H * 64, sub = lane >> 4, c4 = (lane & 15) * 4;
    const int l0 = ch * QKN_CHUNK, l1 = min(L, l0 + QKN_CHUNK);
    const float s_lane = lane_scale(scale_log, max_log, lane, H);
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    const int h = blockIdx.y * 4 + sub, co = h * 64 + c4;
    const bool act = h < H;
    const float s = __shfl(s_lane, h, 64);
    f32x4 bq = z;
    if (need_q && act && q_bias) bq = *reinterpret_cast<const f32x4*>(q_bias + co);
    f32x4 as = z, ab = z, av = z;          // column sums of g q, dx_q and dv over the rows this wave takes
#pragma unroll 1
    for (int l = l0 + w; l < l1; l += 4) {
        const size_t ri = ((size_t)b * L + l) * 3 * (size_t)C;
        f32x4 dxq = z, dxk = z, dvv = z;
        if (need_q) {
            f32x4 x = z, g = z;
            if (act) {
                x = qkn_load4<HF>(qkv, dt, ri + co) + bq;
                g = *reinterpret_cast<const f32x4*>(gq + (size_t)b * st.qb + (size_t)h * st.qh + (size_t)l * st.ql + c4);
            }
            const float n = head_norm(x), d = fmaxf(n, QKN_EPS);
            f32x4 xh;
#pragma unroll
            for (int e = 0; e < 4; ++e) xh[e] = x[e] / d;
            const float dot = group16_sum(dot4(xh, g)), sd = s / d;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                as[e] += g[e] * (xh[e] * s);          // xh s: the forward's q
                dxq[e] = n >= QKN_EPS ? sd * (g[e] - xh[e] * dot) : (s * g[e]) / QKN_EPS;
                ab[e] += dxq[e];
            }
        }
        if (need_k) {
            f32x4 x = z, g = z;
            if (act) {
                x = qkn_load4<HF>(qkv, dt, ri + C + co);
                g = *reinterpret_cast<const f32x4*>(gk + (size_t)b * st.kb + (size_t)h * st.kh + (size_t)l * st.kl + c4);
            }
            const float n = head_norm(x), d = fmaxf(n, QKN_EPS);
            f32x4 xh;
#pragma unroll
            for (int e = 0; e < 4; ++e) xh[e] = x[e] / d;
            const float dot = group16_sum(dot4(xh, g)), sd = 1.0f / d;
#pragma unroll
            for (int e = 0; e < 4; ++e) dxk[e] = n >= QKN_EPS ? sd * (g[e] - xh[e] * dot) : g[e] / QKN_EPS;
        }
        if (need_v && act) {
            dvv = qkn_load4<HF>(gv, dt, (size_t)b * st.vb + (size_t)h * st.vh + (size_t)l * st.vl + c4);
            av = av + dvv;
        }
        if (dqkv && act) {
            qkn_store4<HF>(dqkv, dt, ri + co, dxq);
            qkn_store4<HF>(dqkv, dt, ri + C + co, dxk);
            qkn_store4<HF>(dqkv, dt, ri + 2 * C + co, dvv);
        }
    }
    if (ws) {          // the same in every wave of the workgroup: the barrier is met by all.  The four waves are added in wave order
        red[0][w][lane] = as; red[1][w][lane] = ab; red[2][w][lane] = av;
        __syncthreads();
        if (threadIdx.x < 192) {
            const int qn = threadIdx.x >> 6;
            if (act) {          // lane < 64: the same (h, c4) as this thread's own
                float* dst = ws + (((size_t)b * nchunk + ch) * 3 + qn) * (size_t)C + co;
                *reinterpret_cast<f32x4*>(dst) = ((red[qn][0][lane] + red[qn][1][lane]) + red[qn][2][lane]) + red[qn][3][lane];
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ backward, pass 2
// grid (H, 3): workgroup (h, q) sums quantity q of the 64 columns of head h over the nparts = B * nchunk partial rows; 256 threads = 64 columns x 4 slices.
__global__ __launch_bounds__(256) void qknorm_finish_kernel(const float* __restrict__ ws, int nparts, int C, const float* __restrict__ scale_log, float max_log,
                                                            float* __restrict__ dscale_log, float* __restrict__ dq_bias, float* __restrict__ dv_bias) {
    __shared__ float red[4][64];
    const int q = blockIdx.y, h = blockIdx.x;
    float* out = q == 0 ? dscale_log : (q == 1 ? dq_bias : dv_bias);
    if (!out) return;          // the same for the whole workgroup
    const int cx = threadIdx.x & 63, sl = threadIdx.x >> 6, c = h * 64 + cx;
    const float* p = ws + (size_t)q * C + c;
    float acc = 0.f;
#pragma unroll 8
    for (int n = sl; n < nparts; n += 4) acc += p[(size_t)n * 3 * (size_t)C];
    red[sl][cx] = acc;
    __syncthreads();
    if (sl == 0) {          // wave 0
        const float t = ((red[0][cx] + red[1][cx]) + red[2][cx]) + red[3][cx];
        if (q != 0) out[c] = t;
        else {
            const float sum = wave_sum(t);
            if (cx == 0) out[h] = scale_log[h] <= max_log ? sum : 0.f;          // clamp_max passes the gradient at equality and blocks it above
        }
    }
}

template <typename F>
inline void with_half(int dt, F f) {
    if (dt != 0) f(std::true_type{}); else f(std::false_type{});
}
inline int n_chunks(int L) { return (L + QKN_CHUNK - 1) / QKN_CHUNK; }

int check_shape(const char* who, int B, int L, int H) {
    SDVAR_CHECK_ARG(H >= 1 && H <= QKN_MAX_H, "%s: H=%d heads of 64 channels must be in [1, %d]", who, H, QKN_MAX_H);
    SDVAR_CHECK_ARG(B >= 1 && L >= 1 && (long long)B * L <= 0x7FFFFFFFll / 4 && (long long)B * n_chunks(L) <= 0x7FFFFFFFll,
                    "%s: B=%d, L=%d: both must be at least 1 and B * L at most 2^29", who, B, L);
    return SDVAR_OK;
}
// a gradient read through (b, h, l) strides in elements: non-negative multiples of 4, the base aligned to one lane's load
bool grad_ok(const void* p, const long long* s, int bytes) {
    return ((uintptr_t)p & (uintptr_t)(bytes - 1)) == 0 && s[0] >= 0 && s[1] >= 0 && s[2] >= 0 && s[0] % 4 == 0 && s[1] % 4 == 0 && s[2] % 4 == 0;
}

}  // namespace

long long qknorm_bwd_ws_bytes(int B, int L, int H) {
    if (check_shape("qknorm_bwd_ws_bytes", B, L, H)) return -1;
    return (long long)B * n_chunks(L) * 3 * (64ll * H) * (long long)sizeof(float);
}

int qknorm_fwd(const void* qkv, int dt, const float* q_bias, const float* v_bias, const float* scale_log, double max_log, float* q, float* k, void* v, int B, int L, int H,
               hipStream_t stream) {
    if (int rc = check_shape("qknorm_fwd", B, L, H)) return rc;
    SDVAR_CHECK_ARG(qkv && scale_log && q && k, "qknorm_fwd: null qkv, scale_log, q or k");
    SDVAR_CHECK_ARG(dt >= 0 && dt <= 2, "qknorm_fwd: dtype code %d (0 fp32, 1 fp16, 2 bf16)", dt);
    SDVAR_CHECK_ARG((v_bias != nullptr) == (v != nullptr), "qknorm_fwd: v is written with a v_bias and only then: give both or neither");
    SDVAR_CHECK_ARG((((uintptr_t)qkv | (uintptr_t)q_bias | (uintptr_t)v_bias | (uintptr_t)q | (uintptr_t)k | (uintptr_t)v) & 15) == 0 && ((uintptr_t)scale_log & 3) == 0,
                    "qknorm_fwd: qkv, the biases, q, k and v must be 16-byte aligned, scale_log 4-byte aligned");
    const int rows = B * L;
    with_half(dt, [&](auto hf) {
        hipLaunchKernelGGL((qknorm_fwd_kernel<decltype(hf)::value>), dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, qkv, dt, q_bias, v_bias, scale_log, (float)max_log,
                           q, k, v, rows, H);
    });
    SDVAR_LAUNCH_CHECK();
    return SDVAR_OK;
}

int qknorm_bwd(const void* qkv, int dt, const float* q_bias, const float* scale_log, double max_log, const float* dq, const float* dk, const void* dv,
               const long long* strides, void* dqkv, float* dscale_log, float* dq_bias, float* dv_bias, float* ws, int B, int L, int H, hipStream_t stream) {
    if (int rc = check_shape("qknorm_bwd", B, L, H)) return rc;
    SDVAR_CHECK_ARG(qkv && scale_log && strides, "qknorm_bwd: null qkv, scale_log or strides");
    SDVAR_CHECK_ARG(dqkv || dscale_log || dq_bias || dv_bias, "qknorm_bwd: no output asked for (dqkv, dscale_log, dq_bias and dv_bias are all null)");
    SDVAR_CHECK_ARG(dt >= 0 && dt <= 2, "qknorm_bwd: dtype code %d (0 fp32, 1 fp16, 2 bf16)", dt);
    SDVAR_CHECK_ARG((((uintptr_t)qkv | (uintptr_t)q_bias | (uintptr_t)dqkv | (uintptr_t)ws) & 15) == 0 &&
                        (((uintptr_t)scale_log | (uintptr_t)dscale_log | (uintptr_t)dq_bias | (uintptr_t)dv_bias) & 3) == 0,
                    "qknorm_bwd: qkv, q_bias, dqkv and the workspace must be 16-byte aligned, scale_log and the three sums 4-byte aligned");
    SDVAR_CHECK_ARG((!dq || grad_ok(dq, strides, 16)) && (!dk || grad_ok(dk, strides + 3, 16)) && (!dv || grad_ok(dv, strides + 6, dt == 0 ? 16 : 8)),
                    "qknorm_bwd: dq, dk and dv need (b, h, l) strides that are non-negative multiples of 4 elements, a unit last stride and a base aligned to 4 elements");
    SDVAR_CHECK_ARG(!(dscale_log || dq_bias || dv_bias) || ws, "qknorm_bwd: dscale_log / dq_bias / dv_bias need the workspace (sdvar_op_qknorm_bwd_ws_bytes)");
    const int nchunk = n_chunks(L), C = 64 * H;
    const bool sums = dscale_log || dq_bias || dv_bias;
    const int need_q = dq && (dqkv || dscale_log || dq_bias), need_k = dk && dqkv, need_v = dv && (dqkv || dv_bias);
    const QknStrides st{strides[0], strides[1], strides[2], strides[3], strides[4], strides[5], strides[6], strides[7], strides[8]};
    float* wsk = sums ? ws : nullptr;
    with_half(dt, [&](auto hf) {
        hipLaunchKernelGGL((qknorm_bwd_kernel<decltype(hf)::value>), dim3((unsigned)(B * nchunk), (unsigned)((H + 3) / 4)), dim3(256), 0, stream, qkv, dt, q_bias, scale_log,
                           (float)max_log, dq, dk, dv, st, dqkv, wsk, need_q, need_k, need_v, L, H, nchunk);
    });
    SDVAR_LAUNCH_CHECK();
    if (sums) {
        hipLaunchKernelGGL(qknorm_finish_kernel, dim3((unsigned)H, 3u), dim3(256), 0, stream, ws, B * nchunk, C, scale_log, (float)max_log, dscale_log, dq_bias, dv_bias);
        SDVAR_LAUNCH_CHECK();
    }
    return SDVAR_OK;
}

}  // namespace sdvar
