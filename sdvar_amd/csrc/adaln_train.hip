// The glue of a transformer block under autograd (AdaLNSelfAttn.forward, basic_var.py:152-159; AdaLNBeforeHead.forward, :172-174), both directions:
//
//   adaln     h = ((x - mean) * rstd) * (scale + 1) + shift              LayerNorm without affine (eps inside the root, biased two-pass variance) + modulation
//   gate_add  out = x + (y * gamma) * row_scale[b]                       the gated residual; row_scale = DropPath's per-image factor (NULL: the product as it is)
//
// HBM-bound row kernels: one wave64 per row of C fp32 values, float4 number lane + 64 i of the row in v[i] (the non-paired lane map of elementwise.hip), 16-byte loads
// and stores, the row held in registers between the passes over it.  The statistics are ln_row_finish's operations in its order, so the backward recomputes mean and
// rstd with the forward's bits and nothing but x and scale is saved.  The modulation vectors (scale, shift, gamma) are rows of C values per image, fp32 / fp16 / bf16
// each on its own (dtype codes 0 / 1 / 2), at a batch stride in elements (0: one row for every image); a half value is widened to fp32 before any arithmetic.
//
//   backward of adaln     a = g (1 + scale), xhat = (x - mean) rstd:   dx = rstd (a - mean_c(a) - xhat mean_c(a xhat)),
//                         dscale[b, c] = sum_l g xhat,  dshift[b, c] = sum_l g      (also summed over b when the operand has one row)
//   backward of gate_add  dx = g (no kernel),  dy = (g gamma) row_scale[b] in y's dtype,  dgamma[b, c] = row_scale[b] sum_l g y
//
// The column sums take two passes and no atomics.  Pass 1: a workgroup owns TRAIN_CHUNK consecutive rows of ONE image; wave w takes rows w, w + 4, ... of them and
// keeps fp32 partial sums for the columns its lanes hold; the four waves are added through LDS as ((w0 + w1) + w2) + w3 and one partial row per quantity goes to the
// workspace [b][chunk][nq][C].  Pass 2 (colsum_parts_kernel): slice s of 4 adds the partial rows s, s + 4, ... of an output row in index order (images in index
// order when the operand's batch is 1), the slices are added as ((s0 + s1) + s2) + s3, and the sum is rounded once to the operand's dtype (an fp16 overflow is inf).
// TRAIN_CHUNK is a compile-time constant: the order of every sum depends on (B, L, C) alone, and repeats are bit-identical.
// Nothing here synchronises with the host or allocates.
#include <type_traits>

#include "common.h"

namespace sdvar {

constexpr int TRAIN_MAX_C = 3072;
constexpr int TRAIN_CHUNK = 32;          // rows of one image per workgroup of the backward kernels (8 per wave)

// four consecutive values of a modulation vector / a half y, widened to fp32.  H (the operand is fp16 or bf16, dt says which: wave-uniform) is a template argument of
// every kernel: with the fp32 / half choice made at run time hipcc issued the loads of both forms and held both results (256 registers and scratch at C <= 2048)
template <bool H>
__device__ __forceinline__ f32x4 load4_as_f32(const void* __restrict__ p, int dt, size_t e) {
    if (!H) return *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(p) + e);
    const uint2 w = *reinterpret_cast<const uint2*>(reinterpret_cast<const uint16_t*>(p) + e);
    const bool bf = dt == 2;
    return f32x4{half_lo(w.x, bf), half_hi(w.x, bf), half_lo(w.y, bf), half_hi(w.y, bf)};
}
template <bool H>
__device__ __forceinline__ void store4_as(void* __restrict__ p, int dt, size_t e, f32x4 v) {
    if (!H) { *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(p) + e) = v; return; }
    const bool bf = dt == 2;
    *reinterpret_cast<uint2*>(reinterpret_cast<uint16_t*>(p) + e) = uint2{half_pack2(v[0], v[1], bf), half_pack2(v[2], v[3], bf)};
}

// mean and rstd of the row a wave holds: the operations of ln_row_finish (elementwise.hip), in its order
template <int NV4>
__device__ __forceinline__ void row_stats(const f32x4* v, int lane, int nv, int C, float eps, float& mean, float& rstd) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV4; ++i)
        if (lane + 64 * i < nv) s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
    mean = wave_sum(s) / (float)C;
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < NV4; ++i)
        if (lane + 64 * i < nv) {
#pragma unroll
            for (int e = 0; e < 4; ++e) { const float d = v[i][e] - mean; ss += d * d; }
        }
    rstd = 1.0f / sqrtf(wave_sum(ss) / (float)C + eps);
}

// ------------------------------------------------------------------------------------------------ adaln forward
template <int NV4, bool SH, bool HH>
__global__ __launch_bounds__(256) void adaln_fwd_kernel(const float* __restrict__ x, const void* __restrict__ scale, int sdt, long long sbs, const void* __restrict__ shift,
                                                        int hdt, long long hbs, float* __restrict__ out, int rows, int L, int C, float eps) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int nv = C >> 2, b = row / L;
    constexpr bool HOLD = NV4 == 4;          // the modulation loads first while they fit beside the row: nothing depends on them until the last pass
    f32x4 v[NV4], sc[HOLD ? NV4 : 1], sh[HOLD ? NV4 : 1];
    const size_t so = (size_t)b * (size_t)sbs, ho = (size_t)b * (size_t)hbs;
    if (HOLD) {
#pragma unroll
        for (int i = 0; i < NV4; ++i)
            if (lane + 64 * i < nv) { sc[i] = load4_as_f32<SH>(scale, sdt, so + 4 * (lane + 64 * i)); sh[i] = load4_as_f32<HH>(shift, hdt, ho + 4 * (lane + 64 * i)); }
    }
    const f32x4* px = reinterpret_cast<const f32x4*>(x + (size_t)row * C);
#pragma unroll
    for (int i = 0; i < NV4; ++i)
        if (lane + 64 * i < nv) v[i] = px[lane + 64 * i];
    float mean, rstd;
    row_stats<NV4>(v, lane, nv, C, eps, mean, rstd);
    f32x4* po = reinterpret_cast<f32x4*>(out + (size_t)row * C);
#pragma unroll
    for (int i = 0; i < NV4; ++i)
        if (lane + 64 * i < nv) {
            const f32x4 s4 = HOLD ? sc[i] : load4_as_f32<SH>(scale, sdt, so + 4 * (lane + 64 * i));
            const f32x4 h4 = HOLD ? sh[i] : load4_as_f32<HH>(shift, hdt, ho + 4 * (lane + 64 * i));
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = ((v[i][e] - mean) * rstd) * (s4[e] + 1.0f) + h4[e];
            po[lane + 64 * i] = o;
        }
}

// the four waves' partial sums of one quantity -> one partial row of the workspace, added in wave order; `mul` scales the sum (gate_add: row_scale[b])
template <int NV4>
__device__ __forceinline__ void chunk_combine(f32x4 (*red)[64 * NV4], const f32x4* acc, int lane, int w, int nv, float* __restrict__ dst, bool has_mul, float mul) {
#pragma unroll
    for (int i = 0; i < NV4; ++i)
        if (lane + 64 * i < nv) red[w][lane + 64 * i] = acc[i];
    __syncthreads();
    for (int idx = threadIdx.x; idx < nv; idx += 256) {
        f32x4 t = ((red[0][idx] + red[1][idx]) + red[2][idx]) + red[3][idx];
        if (has_mul) t = t * mul;
        reinterpret_cast<f32x4*>(dst)[idx] = t;
    }
    __syncthreads();
}

// ------------------------------------------------------------------------------------------------ adaln backward, pass 1
template <int NV4, bool SH>
__global__ __launch_bounds__(256) void adaln_bwd_kernel(const float* __restrict__ x, const void* __restrict__ scale, int sdt, long long sbs, const float* __restrict__ g,
                                                        float* __restrict__ dx, float* __restrict__ ws, int L, int C, int nchunk, float eps) {
    __shared__ f32x4 red[4][64 * NV4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int b = blockIdx.x / nchunk, ch = blockIdx.x - b * nchunk;
    const int nv = C >> 2, l0 = ch * TRAIN_CHUNK, l1 = min(L, l0 + TRAIN_CHUNK);
    const size_t so = (size_t)b * (size_t)sbs;
    f32x4 sc1[NV4], ps[NV4], ph[NV4];          // 1 + scale stays in registers for the workgroup's rows
#pragma unroll
    for (int i = 0; i < NV4; ++i) {
        ps[i] = f32x4{0.f, 0.f, 0.f, 0.f}; ph[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (lane + 64 * i < nv) sc1[i] = load4_as_f32<SH>(scale, sdt, so + 4 * (lane + 64 * i)) + 1.0f;
    }
#pragma unroll 1
    for (int l = l0 + w; l < l1; l += 4) {
        const size_t ro = ((size_t)b * L + l) * (size_t)C;
        const f32x4* px = reinterpret_cast<const f32x4*>(x + ro);
        const f32x4* pg = reinterpret_cast<const f32x4*>(g + ro);
        f32x4 v[NV4], gv[NV4];
#pragma unroll
        for (int i = 0; i < NV4; ++i)
            if (lane + 64 * i < nv) { v[i] = px[lane + 64 * i]; gv[i] = pg[lane + 64 * i]; }
        float mean, rstd;
        row_stats<NV4>(v, lane, nv, C, eps, mean, rstd);
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < NV4; ++i)
            if (lane + 64 * i < nv) {
                const f32x4 s4 = sc1[i];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float xh = (v[i][e] - mean) * rstd, a = gv[i][e] * s4[e];
                    ps[i][e] += gv[i][e] * xh; ph[i][e] += gv[i][e];
                    s1 += a; s2 += a * xh;
                    v[i][e] = xh;          // the row's registers now hold xhat
                    gv[i][e] = a;          // ... and g's hold a
                }
            }
        const float m1 = wave_sum(s1) / (float)C, m2 = wave_sum(s2) / (float)C;
        if (dx) {
            f32x4* pd = reinterpret_cast<f32x4*>(dx + ro);
#pragma unroll
            for (int i = 0; i < NV4; ++i)
                if (lane + 64 * i < nv) {
                    f32x4 o;
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[e] = rstd * ((gv[i][e] - m1) - v[i][e] * m2);
                    pd[lane + 64 * i] = o;
                }
        }
    }
    if (ws) {          // wave-uniform and the same in every wave of the workgroup: the barriers inside are met by all
        float* dst = ws + ((size_t)b * nchunk + ch) * 2 * (size_t)C;
        chunk_combine<NV4>(red, ps, lane, w, nv, dst, false, 1.0f);
        chunk_combine<NV4>(red, ph, lane, w, nv, dst + C, false, 1.0f);
    }
}

// ------------------------------------------------------------------------------------------------ pass 2 of both backwards
// out[bo][c] (dense, dtype odt) = sum over the nparts partial rows of output row bo, quantity q of nq: partial row n is at ws[((bo * nparts + n) * nq + q) * C + c].
// grid (ceil(C / 64), output rows), 256 threads = 64 columns x 4 slices.
__global__ __launch_bounds__(256) void colsum_parts_kernel(const float* __restrict__ ws, int nq, int q, int nparts, int C, void* __restrict__ out, int odt) {
    __shared__ float red[4][64];
    const int cx = threadIdx.x & 63, sl = threadIdx.x >> 6, c = blockIdx.x * 64 + cx, bo = blockIdx.y;
    float acc = 0.f;
    if (c < C) {
        const float* p = ws + (((size_t)bo * nparts) * nq + q) * (size_t)C + c;
#pragma unroll 8
        for (int n = sl; n < nparts; n += 4) acc += p[(size_t)n * nq * (size_t)C];
    }
    red[sl][cx] = acc;
    __syncthreads();
    if (sl == 0 && c < C) {
        const float t = ((red[0][cx] + red[1][cx]) + red[2][cx]) + red[3][cx];
        const size_t o = (size_t)bo * C + c;
        if (odt == 0) reinterpret_cast<float*>(out)[o] = t;
        else reinterpret_cast<uint16_t*>(out)[o] = (uint16_t)(half_pack2(t, 0.f, odt == 2) & 0xFFFFu);
    }
}

// ------------------------------------------------------------------------------------------------ gate_add
template <bool YH, bool GH>
__global__ __launch_bounds__(256) void gate_add_fwd_kernel(const float* __restrict__ x, const void* __restrict__ y, int ydt, const void* __restrict__ gamma, int gdt,
                                                           long long gbs, const float* __restrict__ row_scale, float* __restrict__ out, int rows, int L, int C) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int nv = C >> 2, b = row / L;
    const float r = row_scale ? row_scale[b] : 1.0f;
    const size_t ro = (size_t)row * C, go = (size_t)b * (size_t)gbs;
#pragma unroll 4
    for (int idx = lane; idx < nv; idx += 64) {
        const f32x4 gm = load4_as_f32<GH>(gamma, gdt, go + 4 * idx);
        const f32x4 xv = *reinterpret_cast<const f32x4*>(x + ro + 4 * idx);
        const f32x4 yv = load4_as_f32<YH>(y, ydt, ro + 4 * idx);
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float t = yv[e] * gm[e];
            if (row_scale) t = t * r;
            o[e] = xv[e] + t;
        }
        *reinterpret_cast<f32x4*>(out + ro + 4 * idx) = o;
    }
}

template <int NV4, bool YH, bool GH>
__global__ __launch_bounds__(256) void gate_add_bwd_kernel(const float* __restrict__ g, const void* __restrict__ y, int ydt, const void* __restrict__ gamma, int gdt,
                                                           long long gbs, const float* __restrict__ row_scale, void* __restrict__ dy, float* __restrict__ ws, int L, int C,
                                                           int nchunk) {
    __shared__ f32x4 red[4][64 * NV4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int b = blockIdx.x / nchunk, ch = blockIdx.x - b * nchunk;
    const int nv = C >> 2, l0 = ch * TRAIN_CHUNK, l1 = min(L, l0 + TRAIN_CHUNK);
    const float r = row_scale ? row_scale[b] : 1.0f;
    constexpr bool HOLD = NV4 == 4;          // as adaln_bwd_kernel: gamma stays in registers for C <= 1024 and is reloaded per row (cache resident) beyond
    const size_t go = (size_t)b * (size_t)gbs;
    f32x4 gm[HOLD ? NV4 : 1], acc[NV4];
#pragma unroll
    for (int i = 0; i < NV4; ++i) {
        acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (HOLD && lane + 64 * i < nv) gm[i] = load4_as_f32<GH>(gamma, gdt, go + 4 * (lane + 64 * i));
    }
#pragma unroll 1
    for (int l = l0 + w; l < l1; l += 4) {
        const size_t ro = ((size_t)b * L + l) * (size_t)C;
        f32x4 gv[NV4], yv[NV4];
#pragma unroll
        for (int i = 0; i < NV4; ++i)
            if (lane + 64 * i < nv) {
                gv[i] = *reinterpret_cast<const f32x4*>(g + ro + 4 * (lane + 64 * i));
                if (ws) yv[i] = load4_as_f32<YH>(y, ydt, ro + 4 * (lane + 64 * i));
            }
#pragma unroll
        for (int i = 0; i < NV4; ++i)
            if (lane + 64 * i < nv) {
                if (ws) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[i][e] += gv[i][e] * yv[i][e];
                }
                if (dy) {
                    const f32x4 g4 = HOLD ? gm[i] : load4_as_f32<GH>(gamma, gdt, go + 4 * (lane + 64 * i));
                    f32x4 o;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float t = gv[i][e] * g4[e];
                        if (row_scale) t = t * r;
                        o[e] = t;
                    }
                    store4_as<YH>(dy, ydt, ro + 4 * (lane + 64 * i), o);
                }
            }
    }
    if (ws) chunk_combine<NV4>(red, acc, lane, w, nv, ws + ((size_t)b * nchunk + ch) * (size_t)C, row_scale != nullptr, r);
}

// ------------------------------------------------------------------------------------------------ host side
// compile-time dispatch of the row width (4 / 8 / 12 float4 per lane: C <= 1024 / 2048 / 3072) and of "this operand is half"
template <typename F>
static inline void with_width(int C, F f) {
    if (C <= 1024) f(std::integral_constant<int, 4>{});
    else if (C <= 2048) f(std::integral_constant<int, 8>{});
    else f(std::integral_constant<int, 12>{});
}
// adaln_bwd_kernel: hipcc spills the 8-float4 instantiation to scratch (256 VGPRs + 256 AGPRs + 648 bytes per lane) and not the 12 one (256 + 34, none), so
// 1024 < C <= 2048 runs the 12-wide kernel; the float4 a lane does not own are guarded off, so the bits are those of any width
template <typename F>
static inline void with_width_mod_bwd(int C, F f) {
    if (C <= 1024) f(std::integral_constant<int, 4>{});
    else f(std::integral_constant<int, 12>{});
}
template <typename F>
static inline void with_half(int dt, F f) {
    if (dt != 0) f(std::true_type{}); else f(std::false_type{});
}

static inline int n_chunks(int L) { return (L + TRAIN_CHUNK - 1) / TRAIN_CHUNK; }
static inline bool dt_ok(int dt) { return dt >= 0 && dt <= 2; }
static inline bool row_ok(const void* p, int dt, long long bs) { return ((uintptr_t)p & 15) == 0 && bs >= 0 && bs % (dt == 0 ? 4 : 8) == 0; }

static int check_shape(const char* who, int B, int L, int C) {
    SDVAR_CHECK_ARG(C >= 4 && C <= TRAIN_MAX_C && C % 4 == 0, "%s: C=%d must be a multiple of 4 in [4, %d] (float4 loads, one row per wave)", who, C, TRAIN_MAX_C);
    SDVAR_CHECK_ARG(B >= 1 && L >= 1 && (long long)B * L <= 0x7FFFFFFFll / 4 && (long long)B * n_chunks(L) <= 0x7FFFFFFFll,
                    "%s: B=%d, L=%d: both must be at least 1 and B * L at most 2^29", who, B, L);
    return SDVAR_OK;
}

long long adaln_bwd_ws_bytes(int B, int L, int C) {
    if (check_shape("adaln_bwd_ws_bytes", B, L, C)) return -1;
    return (long long)B * n_chunks(L) * 2 * C * (long long)sizeof(float);
}
long long gate_add_bwd_ws_bytes(int B, int L, int C) {
    if (check_shape("gate_add_bwd_ws_bytes", B, L, C)) return -1;
    return (long long)B * n_chunks(L) * C * (long long)sizeof(float);
}

int adaln_fwd(const float* x, const void* scale, int sdt, long long sbs, const void* shift, int hdt, long long hbs, float* out, int B, int L, int C, double eps,
              hipStream_t stream) {
    if (int rc = check_shape("adaln_fwd", B, L, C)) return rc;
    SDVAR_CHECK_ARG(x && scale && shift && out, "adaln_fwd: null x, scale, shift or out");
    SDVAR_CHECK_ARG(dt_ok(sdt) && dt_ok(hdt), "adaln_fwd: dtype codes scale=%d shift=%d (0 fp32, 1 fp16, 2 bf16)", sdt, hdt);
    SDVAR_CHECK_ARG((((uintptr_t)x | (uintptr_t)out) & 15) == 0, "adaln_fwd: x and out must be 16-byte aligned (float4 accesses)");
    SDVAR_CHECK_ARG(row_ok(scale, sdt, sbs) && row_ok(shift, hdt, hbs),
                    "adaln_fwd: scale and shift rows must be 16-byte aligned: base address and a batch stride (%lld, %lld) that is a non-negative multiple of 16 bytes", sbs, hbs);
    SDVAR_CHECK_ARG(eps > 0.0, "adaln_fwd: eps=%g must be positive", eps);
    const int rows = B * L;
    const dim3 grid((unsigned)((rows + 3) / 4)), blk(256);
    with_width(C, [&](auto nv4) { with_half(sdt, [&](auto s_half) { with_half(hdt, [&](auto h_half) {
        hipLaunchKernelGGL((adaln_fwd_kernel<decltype(nv4)::value, decltype(s_half)::value, decltype(h_half)::value>), grid, blk, 0, stream, x, scale, sdt, sbs, shift, hdt,
                           hbs, out, rows, L, C, (float)eps);
    }); }); });
    SDVAR_LAUNCH_CHECK();
    return SDVAR_OK;
}

// dense (out_rows, C) column sums of quantity q of the workspace, out_rows = B or 1
static int colsum_parts(const float* ws, int nq, int q, int B, int nchunk, int C, void* out, int odt, int out_rows, hipStream_t stream) {
    const int nparts = out_rows == 1 ? B * nchunk : nchunk;
    hipLaunchKernelGGL(colsum_parts_kernel, dim3((unsigned)((C + 63) / 64), (unsigned)out_rows), dim3(256), 0, stream, ws, nq, q, nparts, C, out, odt);
    SDVAR_LAUNCH_CHECK();
    return SDVAR_OK;
}

int adaln_bwd(const float* x, const void* scale, int sdt, long long sbs, const float* g, float* dx, void* dscale, int dscale_rows, void* dshift, int hdt, int dshift_rows,
              float* ws, int B, int L, int C, double eps, hipStream_t stream) {
    if (int rc = check_shape("adaln_bwd", B, L, C)) return rc;
    SDVAR_CHECK_ARG(x && scale && g, "adaln_bwd: null x, scale or g");
    SDVAR_CHECK_ARG(dx || dscale || dshift, "adaln_bwd: no output asked for (dx, dscale and dshift are all null)");
    SDVAR_CHECK_ARG(dt_ok(sdt) && dt_ok(hdt), "adaln_bwd: dtype codes scale=%d shift=%d (0 fp32, 1 fp16, 2 bf16)", sdt, hdt);
    SDVAR_CHECK_ARG((((uintptr_t)x | (uintptr_t)g | (uintptr_t)dx | (uintptr_t)ws) & 15) == 0, "adaln_bwd: x, g, dx and the workspace must be 16-byte aligned (float4 accesses)");
    SDVAR_CHECK_ARG(row_ok(scale, sdt, sbs), "adaln_bwd: scale rows must be 16-byte aligned: base address and a batch stride (%lld) that is a non-negative multiple of 16 bytes", sbs);
    SDVAR_CHECK_ARG(!(dscale || dshift) || ws, "adaln_bwd: dscale / dshift need the workspace (sdvar_op_adaln_bwd_ws_bytes)");
    SDVAR_CHECK_ARG((!dscale || dscale_rows == 1 || dscale_rows == B) && (!dshift || dshift_rows == 1 || dshift_rows == B),
                    "adaln_bwd: dscale_rows=%d and dshift_rows=%d must each be 1 or B=%d", dscale_rows, dshift_rows, B);
    SDVAR_CHECK_ARG((((uintptr_t)dscale | (uintptr_t)dshift) & 3) == 0, "adaln_bwd: dscale and dshift must be 4-byte aligned");
    SDVAR_CHECK_ARG(eps > 0.0, "adaln_bwd: eps=%g must be positive", eps);
    const int nchunk = n_chunks(L);
    float* wsk = (dscale || dshift) ? ws : nullptr;
    const dim3 grid((unsigned)(B * nchunk)), blk(256);
    with_width_mod_bwd(C, [&](auto nv4) { with_half(sdt, [&](auto s_half) {
        hipLaunchKernelGGL((adaln_bwd_kernel<decltype(nv4)::value, decltype(s_half)::value>), grid, blk, 0, stream, x, scale, sdt, sbs, g, dx, wsk, L, C, nchunk, (float)eps);
    }); });
    SDVAR_LAUNCH_CHECK();
    if (dscale) { if (int rc = colsum_parts(ws, 2, 0, B, nchunk, C, dscale, sdt, dscale_rows, stream)) return rc; }
    if (dshift) { if (int rc = colsum_parts(ws, 2, 1, B, nchunk, C, dshift, hdt, dshift_rows, stream)) return rc; }
    return SDVAR_OK;
}

int gate_add_fwd(const float* x, const void* y, int ydt, const void* gamma, int gdt, long long gbs, const float* row_scale, float* out, int B, int L, int C,
                 hipStream_t stream) {
    if (int rc = check_shape("gate_add_fwd", B, L, C)) return rc;
    SDVAR_CHECK_ARG(x && y && gamma && out, "gate_add_fwd: null x, y, gamma or out");
    SDVAR_CHECK_ARG(dt_ok(ydt) && dt_ok(gdt), "gate_add_fwd: dtype codes y=%d gamma=%d (0 fp32, 1 fp16, 2 bf16)", ydt, gdt);
    SDVAR_CHECK_ARG((((uintptr_t)x | (uintptr_t)y | (uintptr_t)out) & 15) == 0 && ((uintptr_t)row_scale & 3) == 0,
                    "gate_add_fwd: x, y and out must be 16-byte aligned (float4 accesses), row_scale 4-byte aligned");
    SDVAR_CHECK_ARG(row_ok(gamma, gdt, gbs), "gate_add_fwd: gamma rows must be 16-byte aligned: base address and a batch stride (%lld) that is a non-negative multiple of 16 bytes", gbs);
    const int rows = B * L;
    with_half(ydt, [&](auto y_half) { with_half(gdt, [&](auto g_half) {
        hipLaunchKernelGGL((gate_add_fwd_kernel<decltype(y_half)::value, decltype(g_half)::value>), dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, x, y, ydt, gamma, gdt,
                           gbs, row_scale, out, rows, L, C);
    }); });
    SDVAR_LAUNCH_CHECK();
    return SDVAR_OK;
}

int gate_add_bwd(const float* g, const void* y, int ydt, const void* gamma, int gdt, long long gbs, const float* row_scale, void* dy, void* dgamma, int dgamma_rows,
                 float* ws, int B, int L, int C, hipStream_t stream) {
    if (int rc = check_shape("gate_add_bwd", B, L, C)) return rc;
    SDVAR_CHECK_ARG(g && y && gamma, "gate_add_bwd: null g, y or gamma");
    SDVAR_CHECK_ARG(dy || dgamma, "gate_add_bwd: no output asked for (dy and dgamma are both null)");
    SDVAR_CHECK_ARG(dt_ok(ydt) && dt_ok(gdt), "gate_add_bwd: dtype codes y=%d gamma=%d (0 fp32, 1 fp16, 2 bf16)", ydt, gdt);
    SDVAR_CHECK_ARG((((uintptr_t)g | (uintptr_t)y | (uintptr_t)dy | (uintptr_t)ws) & 15) == 0 && ((uintptr_t)row_scale & 3) == 0,
                    "gate_add_bwd: g, y, dy and the workspace must be 16-byte aligned (float4 accesses), row_scale 4-byte aligned");
    SDVAR_CHECK_ARG(row_ok(gamma, gdt, gbs), "gate_add_bwd: gamma rows must be 16-byte aligned: base address and a batch stride (%lld) that is a non-negative multiple of 16 bytes", gbs);
    SDVAR_CHECK_ARG(!dgamma || ws, "gate_add_bwd: dgamma needs the workspace (sdvar_op_gate_add_bwd_ws_bytes)");
    SDVAR_CHECK_ARG(!dgamma || dgamma_rows == 1 || dgamma_rows == B, "gate_add_bwd: dgamma_rows=%d must be 1 or B=%d", dgamma_rows, B);
    SDVAR_CHECK_ARG(((uintptr_t)dgamma & 3) == 0, "gate_add_bwd: dgamma must be 4-byte aligned");
    const int nchunk = n_chunks(L);
    float* wsk = dgamma ? ws : nullptr;
    const dim3 grid((unsigned)(B * nchunk)), blk(256);
    with_width(C, [&](auto nv4) { with_half(ydt, [&](auto y_half) { with_half(gdt, [&](auto g_half) {
        hipLaunchKernelGGL((gate_add_bwd_kernel<decltype(nv4)::value, decltype(y_half)::value, decltype(g_half)::value>), grid, blk, 0, stream, g, y, ydt, gamma, gdt, gbs,
                           row_scale, dy, wsk, L, C, nchunk);
    }); }); });
    SDVAR_LAUNCH_CHECK();
    if (dgamma) return colsum_parts(ws, 1, 0, B, nchunk, C, dgamma, gdt, dgamma_rows, stream);
    return SDVAR_OK;
}

}  // namespace sdvar
