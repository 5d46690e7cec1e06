// Shared device/host helpers for the gfx950 (CDNA4, wave64) kernels of libsdvar_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <atomic>

#define SDVAR_OK 0
#define SDVAR_ERR_ARG 1
#define SDVAR_ERR_HIP 2
#define SDVAR_ERR_STATE 3

namespace sdvar {

void set_error(const char* fmt, ...);

#define SDVAR_CHECK_ARG(cond, ...)                        \
    do {                                                  \
        if (!(cond)) {                                    \
            sdvar::set_error(__VA_ARGS__);                \
            return SDVAR_ERR_ARG;                         \
        }                                                 \
    } while (0)

#define SDVAR_HIP(call)                                                                         \
    do {                                                                                        \
        hipError_t e_ = (call);                                                                 \
        if (e_ != hipSuccess) {                                                                 \
            sdvar::set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
            return SDVAR_ERR_HIP;                                                               \
        }                                                                                       \
    } while (0)

#define SDVAR_LAUNCH_CHECK() SDVAR_HIP(hipGetLastError())

// Opt-in to more than 64 KiB of dynamic LDS, once per (launch site, device): one bit per device in an atomic mask, so a second
// GPU driven from the same process gets the attribute too and concurrent host threads race only on an idempotent call.
struct LdsOptIn {
    std::atomic<uint64_t> done[4];
    bool pending(int* dev) {
        if (hipGetDevice(dev) != hipSuccess) *dev = 0;
        return !((done[(*dev >> 6) & 3].load(std::memory_order_acquire) >> (*dev & 63)) & 1ull);
    }
    void mark(int dev) { done[(dev >> 6) & 3].fetch_or(1ull << (dev & 63), std::memory_order_release); }
};
#define SDVAR_LDS_OPT_IN(flag, bytes, ...)                                                                                       \
    do {                                                                                                                         \
        int dev_;                                                                                                                \
        if ((flag).pending(&dev_)) {                                                                                             \
            const void* fns_[] = {__VA_ARGS__};                                                                                  \
            for (const void* f_ : fns_) SDVAR_HIP(hipFuncSetAttribute(f_, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(bytes))); \
            (flag).mark(dev_);                                                                                                   \
        }                                                                                                                        \
    } while (0)

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---- wave64 reductions (DPP/shuffle based; every lane gets the result) -------------------------------------------
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// XCD-aware remap of a 1-D block id: blocks that share an XCD (bid % 8 equal) get a contiguous range of logical
// ids, so neighbouring tiles hit the same per-XCD L2 (bijective for any grid size; cdna_hip_programming.md T1).
__device__ __forceinline__ int xcd_remap(int bid, int nblk) {
    const int q = nblk >> 3, r = nblk & 7, x = bid & 7;
    const int base = (x < r) ? x * (q + 1) : r * (q + 1) + (x - r) * q;
    return base + (bid >> 3);
}

// ---- fp32 -> three bf16 planes holding 8 significand bits each (truncation split): x == p0 + p1 + p2 exactly for
// finite normal x (each residual is exact in fp32 and the last one has at most 8 significant bits).
__device__ __forceinline__ void split3(float x, uint16_t& p0, uint16_t& p1, uint16_t& p2) {
    const uint32_t u0 = __float_as_uint(x) & 0xFFFF0000u;
    const float r1 = x - __uint_as_float(u0);
    const uint32_t u1 = __float_as_uint(r1) & 0xFFFF0000u;
    const float r2 = r1 - __uint_as_float(u1);
    p0 = (uint16_t)(u0 >> 16); p1 = (uint16_t)(u1 >> 16); p2 = (uint16_t)(__float_as_uint(r2) >> 16);
}

// ---- fp32 -> two fp16 planes (f16x2 operands, gemm_f16x2.hip): h = fp16(x) round-to-nearest, l = fp16(x - h); a finite x saturates at the
// fp16 range instead of turning into inf - inf = NaN, and a NaN stays a NaN in both planes (v_max / v_min return their non-NaN operand: a bare
// clamp would turn an upstream divergence into a finite -65504).  Saturated / NaN elements are counted by the f16x2 guard (api.hip).
__device__ __forceinline__ float clamp_f16_range(float x) {
    const float c = fminf(fmaxf(x, -65504.0f), 65504.0f);
    return x != x ? x : c;
}
__device__ __forceinline__ void split2h(float x, uint16_t& h, uint16_t& l) {
    x = clamp_f16_range(x);
    const _Float16 hh = (_Float16)x;
    const _Float16 ll = (_Float16)(x - (float)hh);
    h = __builtin_bit_cast(uint16_t, hh); l = __builtin_bit_cast(uint16_t, ll);
}
// ---- the same split two / four values at a time, in packed instructions (v_cvt_pk_f16_f32, v_pk_add_f32): 2.5 vector instructions per value instead of ~11.
// split2h_pk_raw does NO range handling: |x| <= 65504 or NaN only (a NaN flows through both conversions by itself; an inf would turn into inf - inf).
typedef _Float16 f16x2p __attribute__((ext_vector_type(2)));
typedef float f32x2p __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void split2h_pk_raw(float x0, float x1, uint32_t& h, uint32_t& l) {
    const f32x2p v = {x0, x1};
    const f16x2p hh = __builtin_convertvector(v, f16x2p);               // v_cvt_pk_f16_f32: round to nearest even, as (_Float16)x
    const f32x2p r = v - __builtin_convertvector(hh, f32x2p);
    const f16x2p ll = __builtin_convertvector(r, f16x2p);
    h = __builtin_bit_cast(uint32_t, hh); l = __builtin_bit_cast(uint32_t, ll);
    // (Tried in round 3: l by v_fma_mixlo_f16 / v_fma_mixhi_f16 in inline asm - h as an fp16 source, x as an fp32 source, one rounding: 3 instead of 5 instructions
    //  per pair, bit-identical on 1 M random pairs incl. subnormal low planes, tools/micro/fma_mix_probe.hip.  Not used: hipcc pads no hazards around an asm
    //  statement (cdna_hip_programming.md 5.7) and gfx950 has a transcendental-result and a partial-register-write forwarding hazard, both of which these two
    //  instructions can meet wherever the scheduler puts them; the saving is ~2 issue slots per pair.)
}
// max(|a|, |b|, |c|) ignoring NaNs (v_max3_f32 with source modifiers: one instruction, no canonicalisation)
__device__ __forceinline__ float absmax3(float a, float b, float c) {
    float m;
    asm("v_max3_f32 %0, |%1|, |%2|, |%3|" : "=v"(m) : "v"(a), "v"(b), "v"(c));
    return m;
}
// Range handling for a whole wave at once: `m` = this lane's max |x| over the values it is about to split (NaNs ignored).  Almost always every lane is inside
// the fp16 range and the clamp (4 instructions per value) is skipped by a wave-uniform branch; if ANY lane is outside, every lane clamps (finite values
// saturate at +-65504, NaN stays NaN: clamp_f16_range).
__device__ __forceinline__ bool wave_needs_clamp(float m) { return __builtin_amdgcn_ballot_w64(m > 65504.0f) != 0ull; }
// four consecutive values -> the packed words of the two planes
__device__ __forceinline__ void split4h_pk(const float* v, uint2& h, uint2& l) {
    float c[4] = {v[0], v[1], v[2], v[3]};
    if (wave_needs_clamp(fmaxf(absmax3(v[0], v[1], v[2]), fabsf(v[3])))) {
#pragma unroll
        for (int e = 0; e < 4; ++e) c[e] = clamp_f16_range(v[e]);
    }
    split2h_pk_raw(c[0], c[1], h.x, l.x); split2h_pk_raw(c[2], c[3], h.y, l.y);
}

// ---- one fp16 / bf16 plane (gemm_half.hip, mlp_half.hip): two fp32 -> the packed halves of the dtype, round to nearest even (v_cvt_pk_f16_f32: an overflow is inf, nothing
// is clamped; v_cvt_pk_bf16_f32), and the two halves of a packed word back as fp32 (exact).  bf is a compile-time constant or wave-uniform.
typedef __bf16 bf16x2h __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t half_pack2(float a, float b, bool bf) {
    const f32x2p v = {a, b};
    if (bf) return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2h));
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, f16x2p));
}
__device__ __forceinline__ float half_lo(uint32_t w, bool bf) { return bf ? __uint_as_float(w << 16) : (float)__builtin_bit_cast(_Float16, (uint16_t)(w & 0xFFFFu)); }
__device__ __forceinline__ float half_hi(uint32_t w, bool bf) { return bf ? __uint_as_float(w & 0xFFFF0000u) : (float)__builtin_bit_cast(_Float16, (uint16_t)(w >> 16)); }

// ---- GELU(tanh), the two forms of the GEMM epilogues (gemm.hip / gemm_bf16x3.hip: gelu_tanh; gemm_f16x2.hip: gelu_tanh_h) - here so that the FFN backward's
// producers (mlp_bwd.hip) recompute the forward's h bit for bit
__device__ __forceinline__ float gelu_tanh(float x) {
    // 0.5 x (1 + tanh( sqrt(2/pi) (x + 0.044715 x^3) ))   (nn.GELU(approximate='tanh'))
    const float k0 = 0.7978845608028654f, k1 = 0.044715f;
    const float inner = k0 * (x + k1 * x * x * x);
    return 0.5f * x * (1.0f + tanhf(inner));
}
// GELU(tanh) (basic_var.py:40): 0.5 x (1 + tanh(u)) = x sigmoid(2u) = x / (1 + 2^(-2u log2 e)) with v_exp_f32 and v_rcp_f32 (1 ulp each, ~2e-7
// relative on the result): libm's tanhf costs ~40 vector instructions per value and the epilogue of a 256 x 128 tile evaluates 64 of them per lane
// with nothing to hide them under (12 us per round of workgroups at M = 4096, fc1)
__device__ __forceinline__ float gelu_tanh_h(float x) {
    // -2 u log2 e = x (C0 + C1 x^2), C0 = -2 log2(e) sqrt(2 / pi), C1 = 0.044715 C0: 7 vector instructions (mul, fma, mul, exp2, add, rcp, mul)
    const float C0 = -2.3022081986f, C1 = -0.10294324f;
    const float w = x * __builtin_fmaf(x * x, C1, C0);
    const float e = __builtin_amdgcn_exp2f(w);                               // exp(-2u); +inf for very negative x: the quotient is then 0
    return x * __builtin_amdgcn_rcpf(1.0f + e);
}

// g(x) as the forward of the mode computes it (kind 0: gelu_tanh, modes f32 and bf16x3; 1: gelu_tanh_h, mode f16x2) and g'(x).  With u = sqrt(2/pi)(x + 0.044715 x^3) and
// s = sigmoid(2u) = 1 / (1 + e), e = exp(-2u):  g = x s,  g' = s + x s (1 - s) 2u',  1 - s = e s.  e is +inf for very negative x (s = 0) and 0 for very positive x;
// e is clamped to 2^126 and x to +-1e5 in the second term, so every factor is finite and the term is exactly 0 at both ends (no 0 * inf): g' -> 0 / 1.
__device__ __forceinline__ void gelu_val_grad(float x, int kind, float& g, float& dg) {
    const float C0 = -2.3022081986f, C1 = -0.10294324f;            // gelu_tanh_h's constants: -2 u log2 e = x (C0 + C1 x^2)
    const float e = __builtin_amdgcn_exp2f(x * __builtin_fmaf(x * x, C1, C0));
    const float s = __builtin_amdgcn_rcpf(1.0f + e);
    g = kind ? x * s : gelu_tanh(x);
    const float xc = fminf(fmaxf(x, -1e5f), 1e5f);
    const float q = xc * (1.5957691216f + 0.2140644488f * (xc * xc));       // x 2u' = x 2 sqrt(2/pi) (1 + 3 * 0.044715 x^2)
    const float t = fminf(e, 0x1p126f) * s;                                 // 1 - s
    dg = s + (q * t) * s;
    dg = x != x ? x : dg;
}

// Output-plane format of the producers of GEMM operands (ln_modulate, attention, GELU epilogues): none, three bf16 planes, two fp16 planes
enum { PLANES_NONE = 0, PLANES_F16X2 = 2, PLANES_BF16X3 = 3 };
// conv_planes only: operands are PLANES_F16X2 planes (written by the producers under that code), multiplied as ONE product, X plane 0 x W plane 0
enum { PLANES_F16X2_HH = 6 };
// four consecutive values of one row -> the packed 8-byte words of each plane, written at the K-blocked position
__device__ __forceinline__ void store_planes4(uint16_t* outp, size_t ops, size_t o, const float* v, int fmt) {
    if (fmt == PLANES_F16X2) {
        uint2 h, l;
        split4h_pk(v, h, l);
        *reinterpret_cast<uint2*>(outp + o) = h;
        *reinterpret_cast<uint2*>(outp + ops + o) = l;
    } else {
        uint16_t q[3][4];
#pragma unroll
        for (int e = 0; e < 4; ++e) split3(v[e], q[0][e], q[1][e], q[2][e]);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            uint2 w;
            w.x = (uint32_t)q[k][0] | ((uint32_t)q[k][1] << 16); w.y = (uint32_t)q[k][2] | ((uint32_t)q[k][3] << 16);
            *reinterpret_cast<uint2*>(outp + k * ops + o) = w;
        }
    }
}

// eight consecutive values -> three packed bf16x8 words (same split); the top halves of two values are packed with one v_perm_b32
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void split8_packed(const float* v, u32x4& a, u32x4& b, u32x4& c) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float x0 = v[2 * e], x1 = v[2 * e + 1];
        const float r0 = x0 - __uint_as_float(__float_as_uint(x0) & 0xFFFF0000u), r1 = x1 - __uint_as_float(__float_as_uint(x1) & 0xFFFF0000u);
        const float s0 = r0 - __uint_as_float(__float_as_uint(r0) & 0xFFFF0000u), s1 = r1 - __uint_as_float(__float_as_uint(r1) & 0xFFFF0000u);
        a[e] = __builtin_amdgcn_perm(__float_as_uint(x1), __float_as_uint(x0), 0x07060302u);
        b[e] = __builtin_amdgcn_perm(__float_as_uint(r1), __float_as_uint(r0), 0x07060302u);
        c[e] = __builtin_amdgcn_perm(__float_as_uint(s1), __float_as_uint(s0), 0x07060302u);
    }
}

// LDS-DMA of 16 bytes per lane with the address as "wave-uniform 64-bit base (SGPRs) + per-lane 32-bit byte offset (one VGPR)":
// the __builtin_amdgcn_global_load_lds lowering always builds a 64-bit vector address (v_lshl_add_u64 + moves per instruction)
// and reads the LDS address back through v_readfirstlane; vector ALU work does not hide under MFMAs on gfx950, so the K-loops
// keep all of it in scalar registers.  lds_byte_addr must be wave-uniform (M0 = LDS base of the wave's 1 KB slot).
#define SDVAR_DMA16(voff_u32, sbase_ptr, lds_byte_addr)                                                                     \
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"((uint32_t)(voff_u32)), "s"(sbase_ptr), \
                 "s"((uint32_t)(lds_byte_addr)) : "memory")
#define SDVAR_LDS_ADDR(p) ((uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)(p))

// Planar bf16x3 tensors are K-BLOCKED: element (row, k) of plane p of a (rows x K) matrix lives at
//     plane_base[p] + ((k / 32) * rows + row) * 32 + (k % 32)
// i.e. for every block of 32 k the rows are contiguous 64-byte segments, so the (tile rows) x (32 k) slab a GEMM workgroup
// loads per K-step is ONE contiguous run of full 128-byte lines (a [rows][K] row-major plane would give half-line, 64-byte
// fragments at stride 2K: twice the L1/TA requests per byte).
__device__ __forceinline__ size_t kb_index(int row, int k, int rows) { return ((size_t)(k >> 5) * rows + row) * 32 + (k & 31); }

// ---- shared by the operand producers of the seam's backward passes (mlp_bwd.hip, mlp_half.hip, linear_train.hip)
enum { OPF_F32 = 0 };               // an operand format next to PLANES_F16X2 / PLANES_BF16X3: plain fp32 row-major
// eight consecutive values of one operand row -> memory, at element (row, k) of a (rows x K) operand; k % 8 == 0
__device__ __forceinline__ void store_operand8(void* out, size_t ps, int fmt, int row, int k, int rows, int ldo, const float* v, bool live) {
    if (fmt == OPF_F32) {
        if (live) {
            float* p = reinterpret_cast<float*>(out) + (size_t)row * ldo + k;
            *reinterpret_cast<f32x4*>(p) = f32x4{v[0], v[1], v[2], v[3]}; *reinterpret_cast<f32x4*>(p + 4) = f32x4{v[4], v[5], v[6], v[7]};
        }
        return;
    }
    uint16_t* outp = reinterpret_cast<uint16_t*>(out);
    const size_t o = kb_index(row, k, rows);
    if (fmt == PLANES_F16X2) {
        uint2 h0, l0, h1, l1;
        split4h_pk(v, h0, l0); split4h_pk(v + 4, h1, l1);             // wave-uniform range test inside: called by every lane
        if (live) {
            *reinterpret_cast<u32x4*>(outp + o) = u32x4{h0.x, h0.y, h1.x, h1.y};
            *reinterpret_cast<u32x4*>(outp + ps + o) = u32x4{l0.x, l0.y, l1.x, l1.y};
        }
    } else {
        u32x4 a, b, c;
        split8_packed(v, a, b, c);
        if (live) { *reinterpret_cast<u32x4*>(outp + o) = a; *reinterpret_cast<u32x4*>(outp + ps + o) = b; *reinterpret_cast<u32x4*>(outp + 2 * ps + o) = c; }
    }
}
// eight values <-> one packed 16-byte word of fp16 (bf = false) or bf16
__device__ __forceinline__ u32x4 hp_pack8(const float* v, bool bf) {
    return u32x4{half_pack2(v[0], v[1], bf), half_pack2(v[2], v[3], bf), half_pack2(v[4], v[5], bf), half_pack2(v[6], v[7], bf)};
}
__device__ __forceinline__ void hp_unpack8(const u32x4& w, bool bf, float* v) {
#pragma unroll
    for (int e = 0; e < 4; ++e) { v[2 * e] = half_lo(w[e], bf); v[2 * e + 1] = half_hi(w[e], bf); }
}
// The transposing producers move a 32 (k) x 64 (c) tile through LDS with rows padded to 65 words (the bank argument is in mlp_bwd.hip); 256 threads.
constexpr int OPT_K = 32, OPT_C = 64, OPT_S = 65;
// the LDS tile -> rows c0 .. c0 + 63 of the transposed operand (R rows, K = Kp), k block kb; SCALED: the values are multiplied by sc as they leave the tile
template <bool SCALED = false>
__device__ __forceinline__ void store_tile_t(const float* tile, void* out, size_t ps, int fmt, int c0, int kb, int R, int Kp, float sc = 1.0f) {
    const int cl = threadIdx.x >> 2, kq = threadIdx.x & 3;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = SCALED ? tile[(8 * kq + e) * OPT_S + cl] * sc : tile[(8 * kq + e) * OPT_S + cl];
    store_operand8(out, ps, fmt, c0 + cl, kb * OPT_K + 8 * kq, R, Kp, v, c0 + cl < R);
}
// the LDS tile of rounded values -> rows c0 .. c0 + 63 of the transposed half operand (R rows), k block kb
__device__ __forceinline__ void hp_store_tile_t(const float* tile, uint16_t* out, bool bf, int c0, int kb, int R) {
    const int cl = threadIdx.x >> 2, kq = threadIdx.x & 3;
    if (c0 + cl >= R) return;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = tile[(8 * kq + e) * OPT_S + cl];
    *reinterpret_cast<u32x4*>(out + kb_index(c0 + cl, kb * OPT_K + 8 * kq, R)) = hp_pack8(v, bf);
}

// ---- Philox4x32-10 (must match sdvar_amd/noise.py bit for bit) ----------------------------------------------------
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t out[4]) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0, hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

}  // namespace sdvar
