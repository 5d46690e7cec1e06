// fp32 "NT" GEMM on the gfx950 matrix cores:  out[M,N] = epilogue( X[M,K] . W[N,K]^T + bias[N] ).
//
// Replaces the reference's F.linear calls on the sampling path (/root/reference/models/basic_var.py:93 QKV, :119 proj,
// :52 fc1/fc2, :156 ada_lin; models/var.py:125 head, :187 word_embed).  The reference computes them in fp32, and the
// parity bar is bit-exact token ids, so the MFMA form used is v_mfma_f32_32x32x2_f32: fp32 in / fp32 accumulate,
// bitwise a k-ordered fmaf chain (MI355X_MICROARCH.md "Matrix cores"), 157 TFLOP/s peak.
//
// Tiling (wave64, 4 waves / 256 threads per workgroup):
//   block tile BM x BN (128x128, 64x128 or 32x128), K-step 32, both operands K-contiguous in HBM;
//   X and W tiles are staged global -> registers -> LDS (double buffered, one barrier per K-step) with rows padded to
//   36 floats so that the per-lane ds_read_b128 of 4 consecutive k is bank-conflict free;
//   the 4 k of one ds_read_b128 feed 4 MFMAs: lane (i, h) supplies k = 8c + 4h + e for MFMA e of chunk c on BOTH
//   operands, i.e. the K order inside a tile is permuted identically for X and W (sum unchanged, order fixed).
//   Output: lane holds column n = lane & 31 of 16 rows -> 128-byte row segments per store instruction.
// Split-K: the sampler's GEMMs have M = 2B * (tokens of the stage) = 16 .. 4096 rows and N as small as C, so most
//   launches have far fewer output tiles than the 256 CUs and a single workgroup walking all of K is latency-bound
//   (measured: 116 us for any grid of 8..200 workgroups at K = 4096).  When tiles < ~256 the K range is cut into
//   `split` slices (grid = tiles x split), each slice stores its raw fp32 partial tile into a workspace slab, and
//   splitk_reduce_kernel sums the slabs in slice order (deterministic, no atomics) and applies the epilogue.
// Epilogues (fused, the reference's elementwise ops around each linear):
//   EPI_BIAS        out = acc + bias
//   EPI_BIAS_GELU   out = gelu_tanh(acc + bias)                         (basic_var.py:40,52)
//   EPI_GATED_RES   out = res + (acc + bias) * gate[row / rows_per_gate] (basic_var.py:157-158: x + f(.)*gamma)
#include "common.h"
#include "gemm_plan.h"

namespace sdvar {

enum { EPI_BIAS = 0, EPI_BIAS_GELU = 1, EPI_GATED_RES = 2, EPI_PARTIAL = 3 };

constexpr int BK = 32;
constexpr int LDS_STRIDE = BK + 4;   // floats

struct GemmArgs {
    const float* X; const float* W; const float* bias; float* out;
    const float* res; const float* gate;
    int M, N, K, ldx, ldo, ldres;
    int rows_per_gate, gate_stride;
    int split, k_per_split;     // split-K: slice ks covers K-tiles [ks*k_per_split, ...) and writes slab ks of `out`
};

template <int BM, int BN, int WAVES_M, int WAVES_N, int EPI>
__global__ __launch_bounds__(256) void gemm_f32_nt_kernel(GemmArgs a) {
    static_assert(WAVES_M * WAVES_N == 4, "4 waves per workgroup");
    constexpr int WM = BM / WAVES_M, WN = BN / WAVES_N;     // wave tile
    constexpr int TM = WM / 32, TN = WN / 32;               // 32x32 MFMA tiles per wave
    static_assert(TM >= 1 && TN >= 1, "wave tile too small");
    constexpr int XV = BM / 32, WV = BN / 32;                // float4 loads per thread per K-step

    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int STAGE = (BM + BN) * LDS_STRIDE;           // floats per pipeline stage: X tile then W tile

    const int tiles_m = (a.M + BM - 1) / BM, tiles_n = (a.N + BN - 1) / BN;
    const int ntile = tiles_m * tiles_n;
    const int ks = blockIdx.x / ntile;                      // K slice (0 when not split)
    const int lid = xcd_remap(blockIdx.x - ks * ntile, ntile);
    const int tm = lid % tiles_m, tn = lid / tiles_m;       // m fastest: neighbours share the W panel
    const int m0 = tm * BM, n0 = tn * BN;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;
    const int li = lane & 31, lh = lane >> 5;

    // staging assignment: thread -> (row = tid/8 + 32*i, 4 floats at col 4*(tid%8))
    const int srow = tid >> 3, scol = (tid & 7) * 4;
    f32x4 rx[XV], rw[WV];

    auto load_tile = [&](int k0) {
#pragma unroll
        for (int i = 0; i < XV; ++i) {
            const int m = m0 + srow + 32 * i;
            rx[i] = (m < a.M) ? *reinterpret_cast<const f32x4*>(a.X + (size_t)m * a.ldx + k0 + scol) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int i = 0; i < WV; ++i) {
            const int n = n0 + srow + 32 * i;
            rw[i] = (n < a.N) ? *reinterpret_cast<const f32x4*>(a.W + (size_t)n * a.K + k0 + scol) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };
    auto store_tile = [&](int buf) {
#pragma unroll
        for (int i = 0; i < XV; ++i) *reinterpret_cast<f32x4*>(smem + buf * STAGE + (srow + 32 * i) * LDS_STRIDE + scol) = rx[i];
#pragma unroll
        for (int i = 0; i < WV; ++i) *reinterpret_cast<f32x4*>(smem + buf * STAGE + (BM + srow + 32 * i) * LDS_STRIDE + scol) = rw[i];
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int kt0 = ks * a.k_per_split;
    const int nk = min(a.K / BK - kt0, a.k_per_split);
    load_tile(kt0 * BK);
    store_tile(0);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < nk) load_tile((kt0 + kt + 1) * BK);
        const float* px = smem + buf * STAGE + (wm * WM + li) * LDS_STRIDE + 4 * lh;
        const float* pw = smem + buf * STAGE + (BM + wn * WN + li) * LDS_STRIDE + 4 * lh;
#pragma unroll
        for (int c = 0; c < BK / 8; ++c) {
            f32x4 fa[TM], fb[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) fa[i] = *reinterpret_cast<const f32x4*>(px + i * 32 * LDS_STRIDE + 8 * c);
#pragma unroll
            for (int j = 0; j < TN; ++j) fb[j] = *reinterpret_cast<const f32x4*>(pw + j * 32 * LDS_STRIDE + 8 * c);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i][e], fb[j][e], acc[i][j], 0, 0, 0);
        }
        if (kt + 1 < nk) store_tile(buf ^ 1);
        __syncthreads();
    }

    // epilogue: lane owns column n, rows (r&3) + 8*(r>>2) + 4*lh of each 32x32 tile
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int n = n0 + wn * WN + j * 32 + li;
        if (n >= a.N) continue;
        const float bv = (EPI != EPI_PARTIAL && a.bias) ? a.bias[n] : 0.f;
        float* outp = (EPI == EPI_PARTIAL) ? a.out + (size_t)ks * a.M * a.ldo : a.out;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wm * WM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                if (m >= a.M) continue;
                float v = acc[i][j][r] + bv;
                if (EPI == EPI_BIAS_GELU) v = gelu_tanh(v);
                if (EPI == EPI_GATED_RES) {
                    const float g = a.gate[(size_t)(m / a.rows_per_gate) * a.gate_stride + n];
                    v = a.res[(size_t)m * a.ldres + n] + v * g;
                }
                outp[(size_t)m * a.ldo + n] = v;
            }
        }
    }
}

// out = epi( sum_s ws[s] + bias ), 4 columns per thread, slabs summed in slice order
template <int EPI>
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const float* __restrict__ ws, int split, const float* __restrict__ bias, float* out,
                                                            const float* res, const float* __restrict__ gate, int M, int N, int ldo, int ldres,
                                                            int rows_per_gate, int gate_stride) {
    const int nv = N >> 2;
    const size_t total = (size_t)M * nv, slab = (size_t)M * N;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int m = (int)(i / nv), n = (int)(i % nv) * 4;
        f32x4 acc = *reinterpret_cast<const f32x4*>(ws + (size_t)m * N + n);
        for (int s = 1; s < split; ++s) {
            const f32x4 p = *reinterpret_cast<const f32x4*>(ws + s * slab + (size_t)m * N + n);
            acc[0] += p[0]; acc[1] += p[1]; acc[2] += p[2]; acc[3] += p[3];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float v = acc[e] + (bias ? bias[n + e] : 0.f);
            if (EPI == EPI_BIAS_GELU) v = gelu_tanh(v);
            if (EPI == EPI_GATED_RES) v = res[(size_t)m * ldres + n + e] + v * gate[(size_t)(m / rows_per_gate) * gate_stride + n + e];
            out[(size_t)m * ldo + n + e] = v;
        }
    }
}

static thread_local float* g_ws = nullptr;         // split-K slabs, one workspace per host thread (= per model object / stream: sdvar_hip.h)
constexpr size_t WS_FLOATS = (size_t)24 << 20;     // 96 MiB

static thread_local float* g_ws_model = nullptr;   // a model object's own slabs while one of its calls is on the stack (api.hip)
float* set_splitk_workspace(float* p) { float* old = g_ws_model; g_ws_model = p; return old; }
size_t splitk_workspace_floats() { return WS_FLOATS; }

float* splitk_workspace(size_t* floats) {          // shared with gemm_bf16x3.hip and gemm_f16x2.hip
    if (floats) *floats = WS_FLOATS;
    if (g_ws_model) return g_ws_model;
    if (!g_ws && hipMalloc((void**)&g_ws, WS_FLOATS * sizeof(float)) != hipSuccess) { set_error("split-K workspace allocation failed"); return nullptr; }
    return g_ws;
}

// every process-wide switch with a setter: name (sdvar_debug_set_variant), environment variable, default, legal range, value an out-of-range environment maps to
std::atomic<unsigned> g_variant_epoch{0};
Variant g_variants[VAR_COUNT] = {
    {"gemm_h4_var", "SDVAR_GEMM_H4_VAR", 3, 0, 3, 3, false, false},             // which 256 x 256 kernel: 3 = 16x16x32 MFMAs, 0 - 2 = 32x32x16 and its DMA placements
    {"gemm_h2_stages", "SDVAR_GEMM_H2_STAGES", 6, 2, 6, 6, false, false},       // ring of the 128 x 128 kernel
    {"gemm_small_pp", "SDVAR_GEMM_SMALL_PP", 2, 0, 2, 2, false, false},         // 0 = ring kernel for every small tile, 1 = ping-pong kernel for 64-row tiles, 2 = for 32-row tiles too
    {"attn_pp_sched", "SDVAR_ATTN_PP_SCHED", 1, 0, 3, 1, false, false},         // schedule of the 8-wave attention kernel
    {"conv_pp", "SDVAR_CONV_PP", 2, 0, 2, 2, true, false},                      // decoder convolution loop
    {"conv_tap_reuse", "SDVAR_CONV_TAP_REUSE", 1, 0, 1, 1, true, false},        // decoder convolution: X staged once per row of taps where the shape allows it
    {"rowblk", "SDVAR_ROWBLK", 1, 0, 2, 1, false, false},                       // 0 off, 1 from 32 rows, 2 every call of at most 80 rows (sdvar_debug_set_rowblk)
    {"qkv_fuse", "SDVAR_NO_QKV_FUSE", 1, 0, 1, 1, false, true},                 // QKV finish in the GEMM epilogue (sdvar_debug_set_qkv_fuse)
    {"gemm_v2", nullptr, 1, 0, 1, 1, false, false},                             // bf16x3 128-row tile on the LDS-DMA kernel
    {"stage0_table", "SDVAR_STAGE0_TABLE", 1, 0, 1, 1, false, false},           // stage 0 of a label-conditioned call from the per-class table (api.hip: sdvar_stage_first); 0 = always computed
    {"stage0_table_mb", "SDVAR_STAGE0_TABLE_MB", 1024, 0, 1 << 20, 1024, false, false},      // size cap of that table in MiB; a larger table is not built and stage 0 is computed
    {"h16_min_m", "SDVAR_H16_MIN_M", 2704, 1, 1 << 30, 2704, false, false},     // GEMM mode f16: rows from which a call runs on the half kernel (gemm_plan.h use_half)
    {nullptr, nullptr, 0, 0, 768, 0, false, false},                             // forced tile, in f16x2's codes (sdvar_debug_set_gemm_cfg); 0 = automatic
    {nullptr, nullptr, 0, -64, 64, 0, false, false},                            // forced K split; < 0 with tile 256: hybrid tail split
};

template <int BM, int BN, int WAVES_M, int WAVES_N, int EPI>
static int launch_f32_kernel(const GemmArgs& a, int grid, hipStream_t stream) {
    const size_t lds = 2 * (size_t)(BM + BN) * LDS_STRIDE * sizeof(float);
    static LdsOptIn opt_in;         // > 64 KiB of dynamic LDS needs the opt-in once per kernel and device
    SDVAR_LDS_OPT_IN(opt_in, lds, (const void*)gemm_f32_nt_kernel<BM, BN, WAVES_M, WAVES_N, EPI>);
    hipLaunchKernelGGL((gemm_f32_nt_kernel<BM, BN, WAVES_M, WAVES_N, EPI>), dim3(grid), dim3(256), lds, stream, a);
    SDVAR_LAUNCH_CHECK();
    return SDVAR_OK;
}

static int launch_reduce(const GemmArgs& a, const float* ws, int split, int epi, hipStream_t stream) {
    return dispatch_epi(epi, [&](auto e) {
        hipLaunchKernelGGL(splitk_reduce_kernel<decltype(e)::value>, dim3(splitk_reduce_grid(a.M, a.N)), dim3(256), 0, stream, ws, split, a.bias, a.out, a.res, a.gate, a.M, a.N, a.ldo, a.ldres,
                           a.rows_per_gate, a.gate_stride);
        SDVAR_LAUNCH_CHECK();
        return SDVAR_OK;
    });
}

template <int BM, int BN, int WAVES_M, int WAVES_N>
static int launch_cfg(const GemmArgs& a, int epi, int split, hipStream_t stream) {
    const int tiles = ((a.M + BM - 1) / BM) * ((a.N + BN - 1) / BN);
    return launch_splitk(a, epi, split, tiles, nullptr,
                         [&](const GemmArgs& x, int grid, auto e) { return launch_f32_kernel<BM, BN, WAVES_M, WAVES_N, decltype(e)::value>(x, grid, stream); },
                         [&](const GemmArgs& x, const float* ws, int sp, int ep) { return launch_reduce(x, ws, sp, ep, stream); });
}

// Host entry used by the model code and by the op-level C-ABI.
int gemm_f32_nt(const float* X, int ldx, const float* W, const float* bias, float* out, int ldo, int M, int N, int K, int epi,
                const float* res, int ldres, const float* gate, int rows_per_gate, int gate_stride, hipStream_t stream) {
    SDVAR_CHECK_ARG(X && W && out, "gemm: null operand");
    SDVAR_CHECK_ARG(M > 0 && N > 0 && K > 0 && K % BK == 0, "gemm: need K %% 32 == 0 (M=%d N=%d K=%d)", M, N, K);
    SDVAR_CHECK_ARG(ldx >= K && ldx % 4 == 0 && ldo >= N, "gemm: bad leading dims ldx=%d ldo=%d", ldx, ldo);
    SDVAR_CHECK_ARG(((uintptr_t)X % 16) == 0 && ((uintptr_t)W % 16) == 0, "gemm: operands must be 16-byte aligned");
    SDVAR_CHECK_ARG(epi >= EPI_BIAS && epi <= EPI_GATED_RES, "gemm: unknown epilogue %d", epi);
    if (epi == EPI_GATED_RES) SDVAR_CHECK_ARG(res && gate && rows_per_gate > 0 && ldres >= N, "gemm: gated-residual epilogue needs res/gate");
    const GemmArgs a{X, W, bias, out, res, gate, M, N, K, ldx, ldo, ldres, rows_per_gate > 0 ? rows_per_gate : 1, gate_stride, 1, K / BK};
    const GemmPlan p = plan_f32(M, N, K, WS_FLOATS);
    if (p.kernel == 32) return launch_cfg<32, 128, 1, 4>(a, epi, p.split, stream);
    if (p.kernel == 64) return launch_cfg<64, 128, 2, 2>(a, epi, p.split, stream);
    return launch_cfg<128, 128, 2, 2>(a, epi, p.split, stream);
}

}  // namespace sdvar
