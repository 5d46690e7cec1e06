// Host-only part of the GEMM dispatch, shared by gemm.hip, gemm_bf16x3.hip, gemm_f16x2.hip and api.hip:
//   * the table of process-wide kernel-variant switches (variant(), set_variant_by_name());
//   * the planner: which kernel, K split and hybrid tail a shape gets, as a pure function of (M, N, K), the call's flags and the switches.  No HIP call is made
//     here, so the choice can be checked without a GPU (sdvar_debug_plan_gemm);
//   * the launch sequence every tile family shares (launch_splitk, launch_hybrid_tail, dispatch_epi).
#pragma once
#include <limits.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <type_traits>

#include "common.h"

namespace sdvar {

// ---- variant table -----------------------------------------------------------------------------------------------------------------------------------------
// One entry per switch that has a setter.  The value is env-or-default until a setter stores one; a setter value < 0 goes back to env-or-default.  An environment
// value outside [lo, hi] maps to `fallback`.  The atomics make reads from concurrent host threads safe; the setters are still meant for single-threaded tools.
enum VariantId { VAR_GEMM_H4, VAR_GEMM_H2_STAGES, VAR_GEMM_SMALL_PP, VAR_ATTN_PP_SCHED, VAR_CONV_PP, VAR_CONV_TAP_REUSE, VAR_ROWBLK, VAR_QKV_FUSE, VAR_GEMM_V2, VAR_STAGE0_TABLE, VAR_STAGE0_TABLE_MB, VAR_H16_MIN_M, VAR_FORCE_BM, VAR_FORCE_SPLIT, VAR_COUNT };

struct Variant {
    const char* name;           // sdvar_debug_set_variant's name; null: set only through its own ABI function
    const char* env;            // null: no environment variable
    int def, lo, hi, fallback;
    bool env_per_call;          // read the environment at every use (tests change SDVAR_CONV_PP / SDVAR_CONV_TAP_REUSE inside one process)
    bool env_switches_off;      // the variable's presence means 0, whatever a setter said (SDVAR_NO_QKV_FUSE)
    std::atomic<int> set{INT_MIN}, cached{INT_MIN};

    int from_env() const {
        const char* e = env ? getenv(env) : nullptr;
        if (!e) return def;
        if (env_switches_off) return 0;
        const int v = atoi(e);
        return v < lo || v > hi ? fallback : v;
    }
    int get() {
        const int s = set.load(std::memory_order_relaxed);
        if (s != INT_MIN && !env_switches_off) return s;
        int c = env_per_call ? from_env() : cached.load(std::memory_order_relaxed);
        if (c == INT_MIN) { c = from_env(); cached.store(c, std::memory_order_relaxed); }
        return (s == INT_MIN || c == 0) ? c : s;       // env_switches_off: the variable's 0 wins over a setter
    }
    void store(int v) { set.store(v, std::memory_order_relaxed); }                     // as is (the forced split is signed)
    void put(int v) { store(v < 0 ? INT_MIN : v); }                                    // a setter's value: < 0 = back to env-or-default
};
extern Variant g_variants[VAR_COUNT];       // gemm.hip
inline int variant(VariantId id) { return g_variants[id].get(); }
// Bumped by every setter that can change which kernel, K split or launch sequence a call gets: results cached across calls (the stage-0 table of api.hip) carry the
// epoch they were computed under and are rebuilt when it has moved.  The two stage-0 switches only choose between the table and the computed path: no bump.
extern std::atomic<unsigned> g_variant_epoch;       // gemm.hip
inline unsigned variant_epoch() { return g_variant_epoch.load(std::memory_order_relaxed); }
inline void bump_variant_epoch() { g_variant_epoch.fetch_add(1, std::memory_order_relaxed); }
inline int set_variant_by_name(const char* name, int value) {
    for (Variant& v : g_variants) {
        if (!v.name || strcmp(v.name, name)) continue;
        SDVAR_CHECK_ARG(value <= v.hi && (value < 0 || value >= v.lo), "%s %d", name, value);
        v.put(value);
        if (&v != &g_variants[VAR_STAGE0_TABLE] && &v != &g_variants[VAR_STAGE0_TABLE_MB]) bump_variant_epoch();
        return SDVAR_OK;
    }
    set_error("debug_set_variant: unknown variant '%s'", name);
    return SDVAR_ERR_ARG;
}

// env-only A/B switches of the planner (read once)
inline bool env_flag(const char* name) { return getenv(name) != nullptr; }
inline bool gemm_no_hybrid() { static const bool v = env_flag("SDVAR_GEMM_NO_HYBRID"); return v; }
inline bool gemm_no_v4() { static const bool v = env_flag("SDVAR_GEMM_NO_V4"); return v; }
inline bool gemm_no_v7() { static const bool v = env_flag("SDVAR_GEMM_NO_V7"); return v; }
inline int gemm_skinny_max() { static const int v = getenv("SDVAR_GEMM_SKINNY_MAX") ? atoi(getenv("SDVAR_GEMM_SKINNY_MAX")) : 80; return v; }          // 0 switches the skinny kernel off
inline bool gemm_trace() { static const bool v = env_flag("SDVAR_GEMM_TRACE"); return v; }

size_t splitk_workspace_floats();            // gemm.hip: size of the split-K slab workspace (a constant)
float* splitk_workspace(size_t* floats);     // gemm.hip: the calling model's slabs, or this host thread's (allocated at first use)

// ---- planner -----------------------------------------------------------------------------------------------------------------------------------------------
constexpr int PLAN_BK = 32, PLAN_BN = 128;   // K-step and column tile of every tile family the cost model ranks

// kernel codes: 16 skinny, 17 row-block (never planned: its callers ask for it), 32 / 64 / 128 / 256 = rows of a (rows x 128) tile, 512 = 256 x 256, 768 = 256 x 192,
// 1128 = gemm_half.hip's 128 x 128 kernel on the high planes (GEMM mode f16 only: PLAN_KERNEL_HALF below)
struct GemmPlan { int kernel; int split; int tail; bool qkv_fused; };

// What a call hands down to its launcher besides the operands: where to report a deferred K-slice sum (null: launch the reduce), the QKV finish the epilogue may
// take over (null: none offered) and where to report that it did.
struct QkvEpi;
struct GemmCall { int* defer; const QkvEpi* qkv; int* fused; };

// Cost in matrix-pipe cycles per CU: a workgroup spends `kstep * (bm / 32) * kfac * ppfac + kover` per K-step; workgroups are dealt evenly over the 256 CUs, `resident`
// of them share a CU (lat[n]: slowdown of n co-resident ones - a lone workgroup cannot hide its LDS / barrier latency), every workgroup pays fix + fixbm * bm, and
// split > 1 pays the reduce launch and the slab round trip (or, deferred, the consumer's slab reads).
struct GemmCostModel {
    int ntile; int bm[4]; int resident[4];
    double kstep, kfac[4], ppfac[4], lat[5];
    double kover, fix, fixbm, red0, redbw, defbw;
};

// gemm.hip, calibrated with tools/gemm_bench.py --sweep: 64 cycles x 16 MFMAs per 32x32 sub-tile and K-step; narrower tiles re-read more LDS / L2 per MFMA (+3 % / +12 %)
constexpr GemmCostModel COST_F32 = {3, {128, 64, 32, 0}, {2, 2, 3, 0}, 64.0 * 16.0, {1.0, 1.03, 1.12, 0.0}, {1.0, 1.0, 1.0, 1.0}, {0.0, 1.35, 1.08, 1.0, 1.0},
                                    0.0, 2500.0, 40.0, 6000.0, 1800.0, 0.0};
// gemm_bf16x3.hip: 6 MFMAs x 32 cycles x 2 k16-steps per sub-tile (tools/fit_gemm_model.py on profiles/r01_e_gemm_sweep_bf16x3.jsonl: geometric-mean regret 1.8 %,
// worst case 21 %, over the d12 / d16 shapes incl. gamma = 2 chunks)
constexpr GemmCostModel COST_BF16X3 = {4, {256, 128, 64, 32}, {1, 1, 3, 3}, 384.0, {1.1, 1.0, 1.3, 1.3}, {1.0, 1.0, 1.0, 1.0}, {0.0, 1.2, 1.0, 1.0, 1.0},
                                       260.0, 1500.0, 20.0, 2000.0, 5000.0, 0.0};
// gemm_f16x2.hip: half the matrix work per K-step.  Fitted to a sweep with HBM-COLD weights (tools/micro/gemm_sweep_cold.sh: rotating weight tensors, as inside a model
// pass) in which the launches whose K-slice sum a consumer kernel takes over are timed as the slab launch alone and charged the consumer's slab reads (defbw: bytes per
// cycle at which ln_modulate / qk_norm_append read the slabs, not fitted) instead of a reduce launch:
// `tools/fit_gemm_model.py profiles/r02_gemm_sweep_cold_full.jsonl 192 profiles/r02_gemm_sweep_cold_slab.jsonl`: geometric-mean regret 1.1 %, worst case 16 %
constexpr GemmCostModel COST_F16X2 = {4, {256, 128, 64, 32}, {1, 1, 2, 2}, 192.0, {1.0, 1.0, 1.1, 1.8}, {1.0, 1.0, 1.0, 1.0}, {0.0, 1.0, 0.8, 1.0, 1.0},
                                      260.0, 8000.0, 80.0, 4000.0, 5000.0, 2000.0};
// the 256 x 256 kernel of gemm_f16x2.hip: cost per K-step in the units of the other tiles (3072 matrix-pipe cycles per K-step, at the higher clock the 16x16x32 shape
// holds), and its prologue + epilogue + launch (calibrated on M = 2704 / 4096 / 6800, profiles/r03_gemm_tile_ab.log)
constexpr double COST_K4 = 2850.0, COST_FIX4 = 50000.0;

// (row tile, K slices, hybrid tail) of the cheapest launch: the summation order, hence every output bit, depends only on the arguments.  The floating-point
// expressions keep the order they were fitted in - the choice is an argmin and a re-associated sum can flip a near-tie.
inline GemmPlan plan_tiles(const GemmCostModel& cm, int M, int N, int K, size_t ws_floats, bool allow_hybrid, bool deferred, double* cost = nullptr) {
    const int nkt = K / PLAN_BK, tiles_n = (N + PLAN_BN - 1) / PLAN_BN;
    double best = 1e30;
    GemmPlan p{128, 1, 0, false};
    for (int bi = 0; bi < cm.ntile; ++bi) {
        const int bm = cm.bm[bi], res = cm.resident[bi];
        const int tiles = ((M + bm - 1) / bm) * tiles_n;
        const double ktile = cm.kstep * (bm / 32) * cm.kfac[bi] * cm.ppfac[bi];
        for (int split = 1; split <= 32 && split <= nkt / 2; ++split) {
            if (split > 1 && ((size_t)split * M * N > ws_floats || N % 4)) break;
            const int kps = (nkt + split - 1) / split;
            if ((nkt + kps - 1) / kps != split) continue;               // would leave empty trailing slices
            const long blocks = (long)tiles * split;
            const long per_cu = (blocks + 255) / 256;                    // workgroups the busiest CU executes
            const double T = kps * (ktile + cm.kover) + cm.fix + cm.fixbm * bm;    // one workgroup alone on the matrix pipes: K-steps with their sync / refill, prologue + epilogue
            const long full = per_cu / res, rem = per_cu % res;
            const double l_full = (bm == 256) ? 1.0 : cm.lat[res < 4 ? res : 4], l_rem = (bm == 256) ? 1.0 : cm.lat[rem < 4 ? rem : 4];
            double cyc = full * res * T * l_full + (rem ? rem * T * l_rem : 0.0);
            if (split > 1) cyc += deferred ? (double)split * M * N * 4.0 / cm.defbw : cm.red0 + (double)(split + 1) * M * N * 4.0 / cm.redbw;
            if (cyc < best) { best = cyc; p.kernel = bm; p.split = split; p.tail = 0; }
        }
        // hybrid for the 256-row tile: the full rounds run unsplit, only the last, partial round is split along K so that it, too,
        // spreads over the CUs (264 tiles = 256 + 8: the 8 cost a whole second round otherwise)
        if (allow_hybrid && bm == 256 && tiles > 256 && tiles % 256 && N % 4 == 0) {
            const long fullr = tiles / 256, remt = tiles % 256;
            const double Tfull = nkt * (ktile + cm.kover) + cm.fix + cm.fixbm * bm;
            const int cand[7] = {2, 3, 4, 6, 8, 12, 16};
            for (int ci = 0; ci < 7; ++ci) {
                const int ts = cand[ci];
                if (ts > nkt / 2 || (size_t)ts * remt * (256 * 128) > ws_floats) continue;
                const int kps = (nkt + ts - 1) / ts;
                if ((nkt + kps - 1) / kps != ts) continue;
                const long rounds = (remt * ts + 255) / 256;
                // the two extra launches are not free: ~10 us of prologue / slab epilogue / launch latency for the tail kernel, ~6 us for the reduce
                const double cyc = fullr * Tfull + rounds * (kps * (ktile + cm.kover) + 20000.0) + 12000.0 + (double)(ts + 1) * remt * (256.0 * 128.0) * 4.0 / cm.redbw;
                if (cyc < best) { best = cyc; p.kernel = 256; p.split = 1; p.tail = ts; }
            }
        }
    }
    if (cost) *cost = best;
    return p;
}

// a forced K split (tools/gemm_bench.py --sweep, tests): clipped to the K-steps and the workspace, no empty trailing slice
inline int clip_forced_split(int split, int M, int N, int K, size_t ws_floats) {
    const int nkt = K / PLAN_BK;
    if (split > nkt) split = nkt;
    while (split > 1 && (size_t)split * M * N > ws_floats) --split;
    const int kps = (nkt + split - 1) / split;
    return (nkt + kps - 1) / kps;
}
// sdvar_debug_set_gemm_cfg speaks f16x2's codes; the other modes take their nearest tile and know no hybrid forcing
inline int forced_bm_plain() { const int bm = variant(VAR_FORCE_BM); return bm >= 512 ? 256 : bm == 16 ? 32 : bm; }
inline int forced_split_plain() { const int s = variant(VAR_FORCE_SPLIT); return s < 0 ? 0 : s; }

inline GemmPlan plan_f32(int M, int N, int K, size_t ws_floats) {
    GemmPlan p = plan_tiles(COST_F32, M, N, K, ws_floats, false, false);
    const int fbm = forced_bm_plain(), fsplit = forced_split_plain();
    if (fbm && fbm <= 128) p.kernel = fbm;
    if (fsplit) p.split = clip_forced_split(fsplit, M, N, K, ws_floats);
    return p;
}

inline GemmPlan plan_bf16x3(int M, int N, int K, size_t ws_floats) {
    GemmPlan p = plan_tiles(COST_BF16X3, M, N, K, ws_floats, !gemm_no_hybrid(), false);
    const int fbm = forced_bm_plain(), fsplit = forced_split_plain();
    if (fbm) { p.kernel = fbm; p.tail = 0; }
    if (fsplit) p.split = clip_forced_split(fsplit, M, N, K, ws_floats);
    return p;
}

// deferred: the caller sums the K slices itself; qkv_offered: the call comes with a QKV finish its epilogue may take over; vec: every output pointer and leading
// dimension allows 16-byte accesses.  *tiled (optional): the choice among the tile kernels, before a forced K split and the skinny rule - what the first trace line reports.
inline GemmPlan plan_f16x2(int M, int N, int K, size_t ws_floats, bool deferred, bool qkv_offered, bool vec, GemmPlan* tiled = nullptr) {
    const int nkt = K / PLAN_BK;
    const int fbm = variant(VAR_FORCE_BM), fsplit = variant(VAR_FORCE_SPLIT);
    // a QKV launch that can finish q and k in its epilogue stays off the hybrid tail split (whose tail tiles go through slabs): the fused epilogue saves more
    const bool qkv = qkv_offered && vec;
    // the 64-row (32-row) tile on gemm_f16x2_small_pp_kernel: 144 KB of LDS = ONE workgroup per CU, K-step ~0.8 of the ring kernel's (profiles/r03_x_smallpp_ab.log)
    GemmCostModel cm = COST_F16X2;
    const int spp = variant(VAR_GEMM_SMALL_PP);
    if (spp >= 1) { cm.resident[2] = 1; cm.ppfac[2] = 0.8; }
    if (spp >= 2) { cm.resident[3] = 1; cm.ppfac[3] = 0.8; }
    double best;
    GemmPlan p = plan_tiles(cm, M, N, K, ws_floats, !gemm_no_hybrid() && !qkv, deferred, &best);
    // the 256 x 256 ping-pong kernel (code 512): its K loop runs at the matrix pipe's issue rate (3072 cycles per K-step for twice the tile, in-kernel stamps:
    // tools/micro/gemm_v4_stamps.py) but it needs one workgroup per CU and whole rounds of 256 tiles; unsplit only
    if (!gemm_no_v4() && N >= 256 && M > 512) {
        const long tiles4 = (long)((M + 255) / 256) * ((N + 255) / 256), rounds = (tiles4 + 255) / 256;
        const double cyc = rounds * (nkt * COST_K4 + COST_FIX4);
        if (cyc < best) { best = cyc; p = GemmPlan{512, 1, 0, false}; }
    }
    // the 256 x 192 ping-pong kernel (code 768): 3/4 of the 256 x 256 tile's matrix work per K-step and whole rounds where N / 192 x M / 256 fills the chip better
    // than N / 256 does (N = 3 C); same conditions.  Constants: the 256 x 256 kernel's scaled by the MFMA count (72 of 96 per wave and K-step) and
    // the epilogue's share of the fixed part; checked against tools/gemm_bench.py --force on the d12 / d16 shapes (profiles/r04_n_v7_ab.log)
    if (!gemm_no_v4() && !gemm_no_v7() && N >= 192 && N % 64 == 0 && M > 512) {      // a ragged last column tile is fine (N = 4096: 22 tiles; d16 fc1 at M = 2704: 68.7 against 78.0 us)
        const long tiles7 = (long)((M + 255) / 256) * ((N + 191) / 192), rounds = (tiles7 + 255) / 256;
        const double cyc = rounds * (nkt * (0.75 * COST_K4) + 0.85 * COST_FIX4);
        if (cyc < best) { best = cyc; p = GemmPlan{768, 1, 0, false}; }
    }
    if (fbm) { p.kernel = fbm; p.tail = 0; }
    if (fbm == 256 && fsplit < 0) {        // test aid: force the hybrid tail split -split ways (where the shape has a partial last round)
        const int tiles = ((M + 255) / 256) * ((N + PLAN_BN - 1) / PLAN_BN), remt = tiles % 256;
        int ts = -fsplit;
        if (ts > nkt / 2) ts = nkt / 2;
        const int kps = ts > 0 ? (nkt + ts - 1) / ts : nkt;
        if (tiles > 256 && remt && !qkv && N % 4 == 0 && ts >= 2 && (nkt + kps - 1) / kps == ts && (size_t)ts * remt * (256 * 128) <= ws_floats) { p.tail = ts; p.split = 1; }
    }
    if (tiled) *tiled = p;
    if (fsplit > 0) p.split = clip_forced_split(fsplit, M, N, K, ws_floats);
    // the skinny kernel (code 16; M <= 80 rows, N % 16 == 0): chosen for every such shape unless a tile is forced; its own K split (a wave streams <= 8 K-steps)
    if ((fbm == 16 || (!fbm && M <= gemm_skinny_max())) && M <= 80 && N % 16 == 0) {
        int sp = (nkt + 31) / 32;                            // 4 waves x 8 K-steps per workgroup (a 16-wave workgroup for K = 4096 is capped at 128 VGPRs and spills)
        if (fbm == 16 && fsplit > sp) sp = fsplit;
        while (sp > 1 && (size_t)sp * M * N > ws_floats) --sp;
        const int kps = (nkt + sp - 1) / sp;
        // automatic choice: only where ONE workgroup streams the whole K (K <= 1024): with a split over workgroups (fc2, K = 4096) the slab path of the ring kernels is
        // as fast or faster (M = 64: 13.5 against 14.9 us, profiles/r03_s_skinny_ab.log); a forced tile (tests) takes any K
        if (kps <= 32 && (sp == 1 || (fbm == 16 && N % 4 == 0))) return GemmPlan{16, (nkt + kps - 1) / kps, 0, false};
    }
    if (p.kernel == 16) p.kernel = 32;      // forced, but the shape is outside the skinny kernel's range
    p.qkv_fused = qkv && p.split == 1 && p.tail == 0;
    return p;
}

// GEMM mode 3 ("f16"): an f16x2 model whose GEMM launches of at least h16_min_m rows run as one fp16 product on the high planes (gemm_half.hip, kernel code
// PLAN_KERNEL_HALF).  The rule depends on the mode and M only, so that fc1 and fc2 of one call (same M) agree on whether the hidden operand has a low plane.
constexpr int PLAN_KERNEL_HALF = 1128;
inline bool use_half(int mode, int M) { return mode == 3 && M >= variant(VAR_H16_MIN_M); }
inline GemmPlan plan_f16(int M, int N, int K, size_t ws_floats, bool deferred, bool qkv_offered, bool vec) {
    if (use_half(3, M)) return GemmPlan{PLAN_KERNEL_HALF, 1, 0, false};
    return plan_f16x2(M, N, K, ws_floats, deferred, qkv_offered, vec);
}

// ---- launch sequence ---------------------------------------------------------------------------------------------------------------------------------------
// The epilogue codes 0 / 1 / 2 (bias, bias + GELU, gated residual) and 3 (raw K-slice partials) mean the same in the three GEMM files.
template <int E> using EpiTag = std::integral_constant<int, E>;
constexpr int EPI_CODE_PARTIAL = 3;

// f(EpiTag<epi>{}) for the three epilogues a caller can ask for (the entry points have checked the range)
template <class F>
static int dispatch_epi(int epi, F&& f) {
    switch (epi) {
        case 0: return f(EpiTag<0>{});
        case 1: return f(EpiTag<1>{});
        default: return f(EpiTag<2>{});
    }
}

// One tile family's launch.  kern(args, workgroups, EpiTag) launches the family's kernel with that epilogue; reduce(args, slabs, split, epi) launches its reduce.
// split > 1: point the kernel at the slabs and launch the raw-partials kernel on tiles x split workgroups, then either hand the slice count to the deferring
// caller or reduce (skip_reduce: timing experiments, the slab launch alone); else the kernel with the caller's epilogue.
template <class Args, class Kern, class Reduce>
static int launch_splitk(Args a, int epi, int split, int tiles, int* defer, Kern&& kern, Reduce&& reduce, bool skip_reduce = false) {
    const int nkt = a.K / PLAN_BK;
    if (split > 1) {
        float* const ws = splitk_workspace(nullptr);
        if (!ws) return SDVAR_ERR_HIP;
        Args p = a;
        p.out = ws; p.ldo = a.N; p.split = split; p.k_per_split = (nkt + split - 1) / split;
        const int rc = kern(p, tiles * split, EpiTag<EPI_CODE_PARTIAL>{});
        if (rc) return rc;
        if (defer) { *defer = split; return SDVAR_OK; }
        if (skip_reduce) return SDVAR_OK;
        return reduce(a, ws, split, epi);
    }
    a.split = 1; a.k_per_split = nkt;
    return dispatch_epi(epi, [&](auto e) { return kern(a, tiles, e); });
}

// The 256 x 128 families' hybrid: full rounds of 256 tiles unsplit + the partial last round split `tail` ways along K (compact slabs) + a reduce over the tail
// tiles only.  reduce_tiles(slabs, tail, args, tail tiles, EpiTag) launches the per-tile reduce.
template <class Args, class Kern, class ReduceTiles>
static int launch_hybrid_tail(const Args& a, int epi, int tail, Kern&& kern, ReduceTiles&& reduce_tiles) {
    const int tiles = ((a.M + 255) / 256) * ((a.N + PLAN_BN - 1) / PLAN_BN), full = tiles / 256 * 256, remt = tiles - full;
    const int nkt = a.K / PLAN_BK;
    float* const ws = splitk_workspace(nullptr);
    if (!ws) return SDVAR_ERR_HIP;
    Args f = a;
    f.split = 1; f.k_per_split = nkt; f.tile_off = 0; f.tile_cnt = full;
    int rc = dispatch_epi(epi, [&](auto e) { return kern(f, full, e); });
    if (rc) return rc;
    Args p = a;
    p.out = ws; p.split = tail; p.k_per_split = (nkt + tail - 1) / tail; p.tile_off = full; p.tile_cnt = remt;
    rc = kern(p, remt * tail, EpiTag<EPI_CODE_PARTIAL>{});
    if (rc) return rc;
    Args r = a;
    r.tile_off = full; r.tile_cnt = remt;
    return dispatch_epi(epi, [&](auto e) { return reduce_tiles(ws, tail, r, remt, e); });
}

// grid of the row-per-4-columns reduce kernels
inline int splitk_reduce_grid(int M, int N) {
    const size_t total = (size_t)M * (N / 4);
    return (int)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
}

}  // namespace sdvar
