/* libsdvar_hip.so - C ABI of the MI355X (gfx950) speculative draft-verify sampler kernels for VAR.
 *
 * The reference (lijrjyan/SDVAR) is pure Python/PyTorch and has no FFI; the boundary it exposes for this path is its
 * Python API.  Each entry point below replaces the op sequence of the reference lines cited on
 * it; sdvar_amd/engine.py is the ctypes binding and sdvar_amd/var.py mirrors VAR / SDVAR on top of it.
 *
 * Conventions: every pointer is a DEVICE pointer unless marked "host"; tensors are dense row-major fp32, ids int64;
 * all work is enqueued on the caller's `stream` (a hipStream_t passed as void*, NULL = default stream) and returns
 * without synchronising; return value 0 = ok, otherwise see sdvar_last_error().  The library never owns caller
 * memory; the KV cache, adaLN table and workspaces it allocates itself are freed by the *_destroy calls.
 * One host thread per model object (same contract as the reference's module-attribute caches, basic_var.py:85-87); different
 * host threads may drive different objects on different streams concurrently (per-thread split-K workspaces, no shared mutable state
 * outside the objects; the sdvar_debug_* / sdvar_prof_* switches are process-wide and meant for single-threaded tools: the kernel-variant
 * switches live in one table of atomics (csrc/gemm_plan.h), so a GEMM call that reads one while a tool sets it sees the old or the new value).
 */
#ifndef SDVAR_HIP_H
#define SDVAR_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDVAR_ABI_VERSION 5      /* 5: sdvar_debug_plan_gemm (the GEMM planner, callable without a GPU), and, added later WITHOUT a bump (purely additive), sdvar_op_sdpa_lse, sdvar_op_sdpa_bwd, sdvar_op_sdpa_hm_lse and sdvar_op_sdpa_h_bwd, and after them sdvar_xent_train_fwd and sdvar_xent_train_bwd, and the six sdvar_op_adaln_* / sdvar_op_gate_add_* entry points, the three sdvar_op_qknorm_* ones, and sdvar_optim_grad_stats and sdvar_optim_adamw_step; 4 (round 4): sdvar_cfg_combine, sdvar_op_gemm_rowblk, sdvar_debug_set_rowblk; 3 (round 3): the f16-plane KV-cache formats 3 / 4 store V row-major like K; new debug entry points (guard, gemm cfg getter) */
#define SDVAR_MAX_STAGES 16

typedef struct sdvar_model sdvar_model_t;   /* one VAR transformer: weights (borrowed), KV cache, workspaces */
typedef struct sdvar_quant sdvar_quant_t;   /* VectorQuantizer2 inference side: codebook, Phi convs, resample tables */
typedef struct sdvar_vae sdvar_vae_t;       /* VQVAE image decoder (fhat_to_img): conv weights as bf16x3 planes, activation workspaces */
typedef struct sdvar_vae_enc sdvar_vae_enc_t; /* VQVAE image encoder (quant_conv(encoder(img))): same planes and workspaces as the decoder */

typedef struct {
    int32_t depth;                          /* d: width C = 64 d, heads H = d   (models/__init__.py:26-27) */
    int32_t n_stages;                       /* S */
    int32_t patch_nums[SDVAR_MAX_STAGES];   /* the scale ladder                (models/__init__.py:18) */
    int32_t vocab;                          /* V = 4096 */
    int32_t cvae;                           /* 32 */
    int32_t num_classes;                    /* 1000; class_emb has num_classes + 1 rows (var.py:62) */
    int32_t max_batch;                      /* B; the CFG batch is R = 2B rows (var.py:162,188) */
    int32_t max_chunk_stages;               /* largest number of stages one forward may cover (gamma) */
    int32_t kv_dtype;                       /* KV-cache storage: 0 = fp32 (reference CPU path), 1 = fp16 (BASELINE config P4) */
    int32_t gemm_mode;                      /* 0 = fp32 MFMA (v_mfma_f32_32x32x2_f32), 1 = bf16x3 split operands on the bf16 MFMA
                                               (fp32-accurate: x = x1+x2+x3 exactly, 6 of 9 plane products, fp32 accumulate), 2 = f16x2 split
                                               operands on the f16 MFMA (x ~ xh + xl to 2^-22, 3 of 4 plane products, weights scaled by a power of
                                               two per tensor, activations saturate at +-65504: csrc/gemm_f16x2.hip), 3 = f16: a mode-2 model in every
                                               respect (planes, caches, tables, small-M kernels) whose block and head GEMMs run as ONE fp16 product
                                               on the high planes (csrc/gemm_half.hip) in calls of at least "h16_min_m" rows; NOT fp32-accurate */
} sdvar_model_desc;

int sdvar_abi_version(void);
const char* sdvar_last_error(void);        /* host string, valid until the next failing call on this thread */

/* ---- model object -------------------------------------------------------------------------------------------- */
int sdvar_model_create(const sdvar_model_desc* desc /*host*/, sdvar_model_t** out /*host*/);
int sdvar_model_destroy(sdvar_model_t* m);
/* state_dict tensors of models/var.py:56-78: class_emb (num_classes+1, C), pos_start (1,1,C), pos_1LC (1,L,C),
 * lvl_embed (S,C), word_embed.{weight (C,cvae), bias (C)}.  Builds lvl_pos = lvl_embed[lvl] + pos_1LC (var.py:164). */
int sdvar_model_bind_embed(sdvar_model_t* m, const float* class_emb, const float* pos_start, const float* pos_1LC,
                           const float* lvl_embed, const float* word_w, const float* word_b, void* stream);
/* one AdaLNSelfAttn block (basic_var.py:128-159): ada_lin.1.{weight (6C,C), bias}, attn.mat_qkv.weight (3C,C),
 * attn.q_bias, attn.v_bias, attn.scale_mul_1H11 (H), attn.proj.{weight,bias}, ffn.fc1.{weight (4C,C),bias},
 * ffn.fc2.{weight (C,4C),bias}.  ada_w may be NULL for a shared_aln block (see sdvar_model_bind_shared_aln); scale_mul may be NULL for an
 * attn_l2_norm=False model (basic_var.py:66-72: no q/k normalisation, softmax scale 0.25 / sqrt(64)). */
int sdvar_model_bind_block(sdvar_model_t* m, int32_t block, const float* ada_w, const float* ada_b, const float* qkv_w,
                           const float* q_bias, const float* v_bias, const float* scale_mul, const float* proj_w,
                           const float* proj_b, const float* fc1_w, const float* fc1_b, const float* fc2_w,
                           const float* fc2_b, void* stream);
/* shared_aln=True models (VAR-d36-s; var.py:16-19, 81, 192): shared_ada_lin.1.{weight (6C,C), bias (6C)}; their blocks are bound with
 * ada_w = NULL and ada_b = blocks.i.ada_gss (1,1,6,C)  (basic_var.py:143-144, 153-154). */
int sdvar_model_bind_shared_aln(sdvar_model_t* m, const float* shared_w, const float* shared_b);
/* head_nm.ada_lin.1.{weight (2C,C), bias}, head.{weight (V,C), bias}  (basic_var.py:165-174, var.py:116-117) */
int sdvar_model_bind_head(sdvar_model_t* m, const float* nm_w, const float* nm_b, const float* head_w, const float* head_b, void* stream);

/* Per-call prologue (var.py:162-183, 580-601): cond = class_emb[labels ; uncond], first-token map, adaLN parameters
 * of every block and of the head hoisted out of the stage loop (basic_var.py:156, :173 - cond never changes), KV
 * length cursor reset (basic_var.py:87).  labels: (B) int64. */
int sdvar_model_begin(sdvar_model_t* m, int32_t B, const int64_t* labels, void* stream);
/* The same prologue from the conditioning rows themselves: cond (2B, C) device = `sos` / `cond_BD` as SDVAR.init_param returned it
 * (var.py:580-601) and VAR.autoregressive_infer_cfg_sd_helper1 receives it (var.py:319-345) - no label lookup. */
int sdvar_model_begin_cond(sdvar_model_t* m, int32_t B, const float* cond, void* stream);
/* The prologue for R UNPAIRED rows (teacher-forced VAR.forward, var.py:217-259): row r is conditioned on labels[r] (int64 device; num_classes =
 * unconditional), adaLN rows from the per-class table or, for shared_aln models, the GEMM path.  R <= 2 * max_batch.  Resets the KV cache; the
 * call's sdvar_stage_forward / sdvar_head_forward / export_prologue then work on R rows, and sdvar_embed_next (the CFG pair) is refused. */
int sdvar_model_begin_rows(sdvar_model_t* m, int32_t R, const int64_t* labels, void* stream);
/* the tensors SDVAR.init_param returns (var.py:580-601), copied out of the model object: cond (2B,C), lvl_pos (L,C),
 * first-token map (2B,C); any pointer may be NULL */
int sdvar_model_export_prologue(sdvar_model_t* m, float* cond, float* lvl_pos, float* first, void* stream);
/* copy the first-token map (R,1,C) into a chunk input x (R, ltot, C) at token 0 */
int sdvar_model_place_first(sdvar_model_t* m, float* x, int32_t ltot, void* stream);
/* KV-cache cursor: number of valid keys; set_len(n) with n <= current is the rollback after a rejected round. */
int sdvar_kv_len(const sdvar_model_t* m);
int sdvar_kv_set_len(sdvar_model_t* m, int32_t len);
/* Hand-off sampler (var.py:817-824, sd_mask = 0): the target starts at stage `stage` with an EMPTY cache - it never sees the
 * draft's prefix - so cache slot 0 holds the first token of that stage.  Needs kv_len == 0; sdvar_model_begin resets it to stage 0. */
int sdvar_kv_set_origin(sdvar_model_t* m, int32_t stage);
/* next-stage input embedding + CFG duplication (var.py:186-188): nxt (B, l', cvae) -> x rows b and B+b,
 * x[(r*ltot + tok_off + t)*C + :] = word_embed(nxt[b][t]) + lvl_pos[begin(s_next) + t]. */
int sdvar_embed_next(sdvar_model_t* m, const float* nxt, int32_t s_next, float* x, int32_t ltot, int32_t tok_off, void* stream);
/* The same with the lvl_pos rows pos_begin .. pos_begin + l' - 1 instead of the stage's own.  VAR.autoregressive_infer_cfg_sd_helper1 counts
 * `cur_L` from the stage it is resumed at (var.py:352, 369-371, 385, 389: the skipped stages never advance it), so a call resumed at stage c
 * embeds stage s with the rows begin(s) - begin(c); the mirror of that entry point reproduces it through this call. */
int sdvar_embed_next_at(sdvar_model_t* m, const float* nxt, int32_t s_next, int32_t pos_begin, float* x, int32_t ltot, int32_t tok_off, void* stream);
/* Teacher-forcing input of the current call (var.py:230-235), x (R, L, C): token 0 = (class_emb[label] + pos_start) + lvl_pos[0] from the prologue,
 * token t >= 1 = word_embed(xv[r][t-1]) + lvl_pos[t] with xv (R, L-1, cvae) = VectorQuantizer2.idxBl_to_var_input.  Two launches. */
int sdvar_embed_teacher(sdvar_model_t* m, const float* xv, float* x, void* stream);
/* All blocks + head over the stages s0 .. s0+n_stages-1 in ONE pass (var.py:195-197; verify chunk var.py:1051-1055
 * with the mask rows of var.py:108-113 derived from the stage table).  x (R, lsum, C) is the input and is CLOBBERED
 * (it is the residual stream); logits (R, lsum, V).  Requires kv_len == begin(s0); appends lsum keys. */
int sdvar_stage_forward(sdvar_model_t* m, float* x, int32_t s0, int32_t n_stages, float* logits, void* stream);
/* Stage 0 of the current call from the model's OWN first-token map (var.py:162-183: class_emb[label | uncond] + pos_start + lvl_pos[0]) - no x argument;
 * logits (R, 1, V).  Requires kv_len == 0 at origin 0 and a one-token first stage; appends one key.  The result equals
 * sdvar_model_place_first + sdvar_stage_forward(x, 0, 1) bit for bit.  After sdvar_model_begin (labels) stage 0 is a pure function of (weights, class): the
 * first such call after a bind computes it for every class - by the ordinary launch sequence, in batches of the call's R rows - into a per-class table
 * (logits row + the bytes left at cache position 0 of every block's K and V), and this call then is ONE launch that copies the R rows out.  The table is
 * rebuilt when R, the weights or a kernel-variant switch change; it is not used after _begin_cond / _begin_rows, for shared_aln models, with the f16x2 guard
 * on, with "stage0_table" 0 (SDVAR_STAGE0_TABLE=0) or above "stage0_table_mb" MiB (SDVAR_STAGE0_TABLE_MB, default 1024): then the pass is computed. */
int sdvar_stage_first(sdvar_model_t* m, float* logits, void* stream);
/* The same pass under an EXPLICIT additive attention mask instead of the block-causal rows: bias (lsum, kv_len + lsum) fp32, 0 or -inf, the
 * reference's (1, 1, l, K) attn_bias.  For the ablation masks of the hand-off sampler (var.py:557-578 attn_bias_for_sdmasking /
 * attn_bias_for_block, applied at var.py:777-804). */
int sdvar_stage_forward_masked(sdvar_model_t* m, float* x, int32_t s0, int32_t n_stages, const float* bias, float* logits, void* stream);

/* Final adaLN + vocabulary projection only (VAR.get_logits, var.py:119-125; basic_var.py:172-174) on a residual-stream tensor
 * x (R, l, C) -> logits (R, l, V); x is left untouched.  The hand-off sampler with a prefill mask takes its entry-stage logits from
 * the INPUT token map (var.py:809-811), which is this call. */
int sdvar_head_forward(sdvar_model_t* m, const float* x, int32_t l, float* logits, void* stream);

/* ---- quantizer ----------------------------------------------------------------------------------------------- */
int sdvar_quant_create(int32_t n_stages, const int32_t* patch_nums /*host*/, int32_t cvae, int32_t vocab, int32_t max_batch,
                       int32_t n_phi, sdvar_quant_t** out /*host*/);
int sdvar_quant_destroy(sdvar_quant_t* q);
/* quantize.embedding.weight (V,cvae); the Phi convolutions {weight (cvae,cvae,3,3), bias} as host arrays of n_phi device pointers
 * (quant.py:39, 199-243).  n_phi follows the layout the checkpoint was built with (quant.py:27-32): share_quant_resi >= 2 ->
 * quant_resi.qresi_ls.<k> (PhiPartiallyShared, n_phi = share_quant_resi), 1 -> quant_resi.qresi (PhiShared, n_phi = 1),
 * 0 -> quant_resi.<k> (PhiNonShared, n_phi = n_stages); stage s uses the Phi whose tick is nearest to s / (n_stages - 1). */
int sdvar_quant_bind(sdvar_quant_t* q, const float* codebook, const float* const* phi_w /*host*/, const float* const* phi_b /*host*/);
/* quant.py:187-196 for stage si: f_hat (B,cvae,HW,HW) += Phi(up(codebook[ids])) in place; nxt (B, pn_{si+1}^2, cvae)
 * = area_down(f_hat) (not written for the last stage; may be NULL there).  ids[b*ids_stride + p]. */
int sdvar_quant_next(sdvar_quant_t* q, int32_t si, const int64_t* ids, int32_t ids_stride, float* f_hat, float* nxt, int32_t B, void* stream);
/* the same with separate input and output accumulators: f_out = f_in + Phi(up(codebook[ids])); a draft round keeps one f_hat snapshot
 * per drafted stage (var.py:1013-1022 recomputes them) without copies */
int sdvar_quant_next_from(sdvar_quant_t* q, int32_t si, const int64_t* ids, int32_t ids_stride, const float* f_in, float* f_out, float* nxt,
                          int32_t B, void* stream);
/* the same from explicit feature vectors h (B, pn_si^2, cvae) instead of token ids (more_smooth=True, var.py:206-210) */
int sdvar_quant_next_h(sdvar_quant_t* q, int32_t si, const float* h, float* f_hat, float* nxt, int32_t B, void* stream);
/* f_to_idxBl_or_fhat (quant.py:135-166, using_znorm = False): multi-scale residual quantisation of f (B,cvae,HW,HW).  Per scale s:
 * z = area_down(f_rest, pn_s) (f_rest itself at the last scale); ids = argmin_v |z|^2 + |e_v|^2 - 2 z.e_v in fp32, ties to the lowest index;
 * h = Phi(bicubic_up(codebook[ids])); f_hat += h; f_rest -= h.  ids_out (B, L) int64 (L = sum pn^2, scales in order); f_hat_out (B,cvae,HW,HW)
 * the final f_hat; f_hat_per_scale (S,B,cvae,HW,HW) or NULL: f_hat after every scale.  cvae = 32 only.  |e_v|^2 is computed once per bind,
 * on the stream of the first call. */
int sdvar_quant_encode(sdvar_quant_t* q, const float* f, int32_t B, int64_t* ids_out, float* f_hat_out, float* f_hat_per_scale, void* stream);
/* VectorQuantizer2.forward in eval mode (quant.py:52-104): the chain of sdvar_quant_encode (same kernels, same order: ids_out, f_hat_out and
 * f_hat_per_scale are the same bits) plus the statistics of that method.  hits (S, V) int32: hits[s][v] = rows of scale s assigned to code v,
 * idx_N.bincount(minlength=V) of quant.py:77 (integer atomics: order-independent).  sqerr (S) double: sqerr[s] = sum over the B*cvae*HW^2 elements of
 * (f_hat_s - f)^2 with f_hat_s the accumulator after scale s - each difference in fp32, squared and summed in fp64 - so that
 * F.mse_loss(f_hat, f) of quant.py:95 is sqerr[s] / numel.  One partial per workgroup, then a fixed-order pass; no floating-point atomics: repeated
 * calls are bit-identical.  f_st (B,cvae,HW,HW) or NULL: the straight-through value of quant.py:98, fl(fl(f_hat - f) + f), which is what the reference
 * hands to its decoder (not bit-equal to f_hat); written by the last scale's statistics pass.  f_st must not alias f or f_hat_out. */
int sdvar_quant_encode_stats(sdvar_quant_t* q, const float* f, int32_t B, int64_t* ids_out, float* f_hat_out, float* f_hat_per_scale, int32_t* hits,
                             double* sqerr, float* f_st, void* stream);
/* more_smooth=True (var.py:206-208 + helpers.py:22-36): h (B,l,cvae) = softmax((masked * (1 + ratio) + g) / tau) @ codebook,
 * g = -log(E), E ~ Exp(1): e_noise (B,l,V) explicit, or NULL for the Philox stream at (seed, draw, image_offset).  `masked_logits`
 * (B,l,V) are the CFG logits as sample_with_top_k_top_p_ leaves them (helpers.py:10,15 mask in place): sdvar_cfg_sample's dbg_masked. */
int sdvar_gumbel_mix(sdvar_quant_t* q, const float* masked_logits, int32_t B, int32_t l, double ratio, double tau, const float* e_noise,
                     uint64_t seed, uint32_t draw, uint32_t image_offset, float* h_out, void* stream);

/* ---- VQVAE decoder: f_hat -> image (the caller side of the sampler) ------------------ */
typedef struct {
    int32_t ch;                             /* base width (160 for vae_ch160v4096z32)          models/vqvae.py:30-33 */
    int32_t z_channels;                     /* Cvae = 32 */
    int32_t n_mult;                         /* number of resolution levels */
    int32_t ch_mult[8];                     /* (1, 1, 2, 2, 4)                                 models/vqvae.py:31 */
    int32_t num_res_blocks;                 /* 2: every decoder level has num_res_blocks + 1 ResnetBlocks (basic_vae.py:196) */
    int32_t max_batch;
    int32_t latent_hw;                      /* side of f_hat: 16 for 256^2 images, 32 for 512^2 */
    int32_t plane_format;                   /* operands of the convolutions: 0 or 2 = f16x2 (two fp16 planes, three MFMA products), 3 = bf16x3;
                                               sdvar_vae_create only: 6 = an f16x2 decoder whose conv_planes launches multiply plane 0 with plane 0 and nothing else
                                               (opt-in: NOT fp32-accurate; conv_out, GroupNorm and attention are unchanged).  sdvar_vae_enc_create rejects 6 */
} sdvar_vae_desc;
int sdvar_vae_create(const sdvar_vae_desc* desc /*host*/, sdvar_vae_t** out /*host*/);
int sdvar_vae_destroy(sdvar_vae_t* v);
/* number of tensors sdvar_vae_bind expects for this descriptor */
int sdvar_vae_tensor_count(const sdvar_vae_desc* desc /*host*/);
/* Host array of device pointers to the fp32 state_dict tensors, in execution order (weight then bias each):
 * post_quant_conv; decoder.conv_in; decoder.mid.block_1 {norm1, conv1, norm2, conv2}; decoder.mid.attn_1 {norm, qkv,
 * proj_out}; decoder.mid.block_2; then for level = n_mult-1 .. 0: for i = 0 .. num_res_blocks: up.level.block.i {norm1,
 * conv1, norm2, conv2, [nin_shortcut if the width changes]}, [up.level.attn.i at the top level]; [up.level.upsample.conv
 * for level > 0]; decoder.norm_out; decoder.conv_out.   (models/basic_vae.py:163-226)
 * Conv weights are re-packed into bf16x3 planes (owned copies); biases and GroupNorm affine tensors stay borrowed. */
int sdvar_vae_bind(sdvar_vae_t* v, const float* const* tensors /*host*/, int32_t n_tensors, void* stream);
/* vqvae.py:62-63: img (B,3,H,W) = clamp(decoder(post_quant_conv(f_hat (B,Cvae,h,w))), -1, 1), H = h << (n_mult-1) */
int sdvar_vae_decode(sdvar_vae_t* v, const float* f_hat, int32_t B, float* img, void* stream);
/* vqvae.py:59 (VQVAE.forward): img = decoder(post_quant_conv(f_hat)) WITHOUT the clamp - the launches of sdvar_vae_decode with the clamp compiled
 * out of the last kernel, so clamp(raw, -1, 1) is sdvar_vae_decode's image bit for bit. */
int sdvar_vae_decode_raw(sdvar_vae_t* v, const float* f_hat, int32_t B, float* img, void* stream);

/* ---- VQVAE encoder: image -> f = quant_conv(encoder(img)) (models/vqvae.py:65-67, models/basic_vae.py:99-161) ------------- */
/* The decoder's descriptor: images are latent_hw << (n_mult-1) pixels square (256^2 -> latent 16^2, 512^2 -> 32^2), any B <= max_batch. */
int sdvar_vae_enc_create(const sdvar_vae_desc* desc /*host*/, sdvar_vae_enc_t** out /*host*/);
int sdvar_vae_enc_destroy(sdvar_vae_enc_t* e);
/* number of tensors sdvar_vae_enc_bind expects for this descriptor */
int sdvar_vae_enc_tensor_count(const sdvar_vae_desc* desc /*host*/);
/* Host array of device pointers to the fp32 state_dict tensors, in execution order (weight then bias each):
 * encoder.conv_in; for level = 0 .. n_mult-1: for i = 0 .. num_res_blocks-1: down.level.block.i {norm1, conv1, norm2, conv2,
 * [nin_shortcut if the width changes]}, [down.level.attn.i {norm, qkv, proj_out} at the top level]; [down.level.downsample.conv for
 * level < n_mult-1]; encoder.mid.block_1; encoder.mid.attn_1; encoder.mid.block_2; encoder.norm_out; encoder.conv_out; quant_conv.
 * conv_in is zero-padded to 32 input channels and every Downsample2x weight is re-packed for the space-to-depth form at bind. */
int sdvar_vae_enc_bind(sdvar_vae_enc_t* e, const float* const* tensors /*host*/, int32_t n_tensors, void* stream);
/* f (B,z,h,h) = quant_conv(encoder(img (B,3,H,W))), H = W = h << (n_mult-1) */
int sdvar_vae_enc_encode(sdvar_vae_enc_t* e, const float* img, int32_t B, float* f, void* stream);

/* ---- sampling / acceptance -------------------------------------------------------------------------------------- */
/* var.py:199-202 + helpers.py:6-19: CFG with t = cfg*si/(S-1), top-k, top-p, draw = argmax(p/q).
 * q: explicit Exp(1) noise (B*l, V), or NULL to generate the Philox stream of sdvar_amd/noise.py in-kernel from
 * (seed, draw, image_offset).  ids_out[b*ids_stride + tok].  dbg_masked: optional (B,l,V) masked logits. */
int sdvar_cfg_sample(const float* logits, int32_t B, int32_t l, int32_t V, double t, int32_t top_k, double top_p, const float* q,
                     uint64_t seed, uint32_t draw, uint32_t image_offset, int64_t* ids_out, int32_t ids_stride, float* dbg_masked,
                     void* stream);
/* var.py:1062-1067 + 1199-1222 over a verified chunk: per stage CFG (t[j], host doubles) -> argmax_V -> compare with
 * the draft ids -> matched count; n_accept = leading stages with float32 match rate >= thr.
 * counts (40 x int32, device): [0..16) matched per stage, [16] n_accept, [17..33) tokens per stage. */
int sdvar_verify_accept(const float* logits, int32_t B, int32_t lsum, int32_t V, int32_t n_stages, const int32_t* stage_lens /*host*/,
                        const double* t /*host*/, const int64_t* draft_ids, int32_t ids_stride, double thr, int32_t* counts,
                        int64_t* argmax_out, void* stream);

/* The richer acceptance rules sketched in SDVAR.advanced_token_matching (var.py:1229-1243).  rule 0: draft id == argmax (as above);
 * 1: draft id among the target's top `match_top_k` (fewer than k entries score strictly higher); 2: KL(softmax target || softmax draft)
 * <= kl_thr, with the draft's raw logits of the chunk in draft_logits (stage j stored as (2B, l_j, V) at element offset 2*B*V*qbeg_j).
 * match_out (B, lsum) u8: per-token verdict; corrected_out (B, lsum): draft id where the rule holds, the target's argmax elsewhere
 * (token-level partial acceptance).  Any of argmax_out / match_out / corrected_out may be NULL. */
int sdvar_verify_accept_ex(const float* logits, int32_t B, int32_t lsum, int32_t V, int32_t n_stages, const int32_t* stage_lens /*host*/,
                           const double* t /*host*/, const int64_t* draft_ids, int32_t ids_stride, double thr, int32_t rule, int32_t match_top_k,
                           double kl_thr, const float* draft_logits, int32_t* counts, int64_t* argmax_out, uint8_t* match_out,
                           int64_t* corrected_out, void* stream);

/* var.py:1062-1067 alone: out (B, lsum, V) = (1 + t_j) * logits[b] - t_j * logits[B + b] for every stage j of a verified chunk (float32 roundings of torch's
 * scalar ops): the per-stage CFG logits SDVAR.target_verify_batch returns to a caller that drives the reference's step functions itself. */
int sdvar_cfg_combine(const float* logits, int32_t B, int32_t lsum, int32_t V, int32_t n_stages, const int32_t* stage_lens /*host*/, const double* t /*host*/,
                      float* out, void* stream);
/* ---- per-image sampling parameters (an extension: the reference's arguments are scalars) ------------------------------------------
 * Image b of a batch is sampled with its own (cfg_b, top_k_b, top_p_b, seed_b, index_b).  The *_rows entry points below take them from two
 * tables in DEVICE memory, which the caller builds on the host and uploads once per sampler call; the kernels only read them, one row per
 * workgroup (a workgroup serves one image).  Nothing is copied or synchronised per launch.
 *   image table   sdvar_row_image[n_rows]: 32-byte rows, one per image
 *   factor table  float[n_stages][n_rows][2]: { float32(1 + t), float32(t) } with t = cfg_b * s / (S - 1) of (stage s, image b) - the two
 *                 roundings sdvar_cfg_sample / sdvar_verify_accept_ex / sdvar_cfg_combine apply to their scalar t, done by the caller.
 *                 A one-stage call takes the (n_rows, 2) slice of its stage, a chunk call the slices of its n_stages consecutive stages.
 * n_rows is the number of images the tables were built for and must equal B (the factor table is strided by it).
 * With equal values in every row the *_rows entry points produce the bits of their scalar twins. */
typedef struct {
    int32_t  top_k;                         /* 0 = off; < 0 is rejected */
    int32_t  use_top_p;                     /* top_p_b > 0 */
    float    top_p_thr;                     /* float32(1 - top_p_b) */
    uint32_t seed_lo, seed_hi;              /* Philox key of image b: seed_b (the kernels apply the key xor of sdvar_amd/noise.py) */
    uint32_t index;                         /* Philox image counter of image b (the scalar entry points use image_offset + b) */
    uint32_t reserved[2];                   /* 0 */
} sdvar_row_image;
/* sdvar_cfg_sample with per-image parameters.  fac (B,2) and img (B) are DEVICE tables; img_host is the host copy of img the caller built
 * (checked here: a negative top_k gives SDVAR_ERR_ARG; never handed to the GPU). */
int sdvar_cfg_sample_rows(const float* logits, int32_t B, int32_t l, int32_t V, const float* fac, const sdvar_row_image* img,
                          const sdvar_row_image* img_host /*host*/, int32_t n_rows, const float* q, uint32_t draw, int64_t* ids_out, int32_t ids_stride,
                          float* dbg_masked, void* stream);
/* sdvar_verify_accept_ex with the CFG factors of (stage j of the chunk, image b) from fac (n_stages, B, 2), DEVICE.  The acceptance decision is
 * unchanged: per-stage batch match rate against thr. */
int sdvar_verify_accept_rows(const float* logits, int32_t B, int32_t lsum, int32_t V, int32_t n_stages, const int32_t* stage_lens /*host*/, const float* fac,
                             int32_t n_rows, const int64_t* draft_ids, int32_t ids_stride, double thr, int32_t rule, int32_t match_top_k, double kl_thr,
                             const float* draft_logits, int32_t* counts, int64_t* argmax_out, uint8_t* match_out, int64_t* corrected_out, void* stream);
/* sdvar_cfg_combine with fac (n_stages, B, 2), DEVICE */
int sdvar_cfg_combine_rows(const float* logits, int32_t B, int32_t lsum, int32_t V, int32_t n_stages, const int32_t* stage_lens /*host*/, const float* fac,
                           int32_t n_rows, float* out, void* stream);
/* sdvar_gumbel_mix with the Philox key and image counter of image b from img (B), DEVICE; ratio and tau belong to the stage */
int sdvar_gumbel_mix_rows(sdvar_quant_t* q, const float* masked_logits, int32_t B, int32_t l, double ratio, double tau, const float* e_noise,
                          const sdvar_row_image* img, int32_t n_rows, uint32_t draw, float* h_out, void* stream);

/* ---- masked sampling (an extension: in-painting, out-painting, class editing; the reference has no such call) ---------------------------
 * sdvar_cfg_sample with forced tokens.  gen (uint8) and force_ids (int64) are DEVICE tables read at [b * force_stride + tok], tok in [0, l).
 * gen == 0: the token is not sampled; ids_out[b * ids_stride + tok] = force_ids[..] clamped into [0, V) (memory safety only: the next kernel
 * gathers codebook rows by it; callers validate their ids), and the token's row of dbg_masked is NOT written.  gen != 0: the token is sampled
 * exactly as sdvar_cfg_sample samples it - the Philox counter is (vocab chunk, token, image, draw), so it draws what an unmasked launch on the
 * same logits draws.  With gen all ones the outputs carry the bits of sdvar_cfg_sample.  ids_out may alias force_ids. */
int sdvar_cfg_sample_forced(const float* logits, int32_t B, int32_t l, int32_t V, double t, int32_t top_k, double top_p, const float* q,
                            uint64_t seed, uint32_t draw, uint32_t image_offset, int64_t* ids_out, int32_t ids_stride, float* dbg_masked,
                            const uint8_t* gen, const int64_t* force_ids, int32_t force_stride, void* stream);
/* sdvar_cfg_sample_rows with forced tokens (gen, force_ids, force_stride as above) */
int sdvar_cfg_sample_rows_forced(const float* logits, int32_t B, int32_t l, int32_t V, const float* fac, const sdvar_row_image* img,
                                 const sdvar_row_image* img_host /*host*/, int32_t n_rows, const float* q, uint32_t draw, int64_t* ids_out,
                                 int32_t ids_stride, float* dbg_masked, const uint8_t* gen, const int64_t* force_ids, int32_t force_stride, void* stream);
/* sdvar_verify_accept_ex / sdvar_verify_accept_rows over a chunk that holds forced tokens (the speculative sampler under a mask).  gen (uint8, DEVICE) is read at
 * [b * gen_stride + tok_in_chunk], tok_in_chunk in [0, lsum): the pointer is already advanced to the chunk's first token, exactly as draft_ids is; gen_stride >= lsum.
 * gen == 0, a forced token: it is no draft prediction, so it is verified by nobody - its workgroup reads no logit, adds nothing to counts[j], and writes (where given)
 * match_out = 1, corrected_out = the draft id, argmax_out = -1.  gen != 0, a sampled token: everything as in the unforced entry points, for all three rules.
 * counts[17 + j] = the number of SAMPLED tokens of stage j over the batch (not B * l_j); the scan accepts a stage with none, and otherwise applies
 * float32(matched) / float32(sampled) promoted to double >= thr, stopping at the first failure.  Integer counters: repeated calls are bit-identical.  With gen all ones
 * every counter and output carries the bits of the unforced entry point.  No host synchronisation. */
int sdvar_verify_accept_forced(const float* logits, int32_t B, int32_t lsum, int32_t V, int32_t n_stages, const int32_t* stage_lens /*host*/,
                               const double* t /*host*/, const int64_t* draft_ids, int32_t ids_stride, double thr, int32_t rule, int32_t match_top_k,
                               double kl_thr, const float* draft_logits, int32_t* counts, int64_t* argmax_out, uint8_t* match_out,
                               int64_t* corrected_out, const uint8_t* gen, int32_t gen_stride, void* stream);
int sdvar_verify_accept_rows_forced(const float* logits, int32_t B, int32_t lsum, int32_t V, int32_t n_stages, const int32_t* stage_lens /*host*/, const float* fac,
                                    int32_t n_rows, const int64_t* draft_ids, int32_t ids_stride, double thr, int32_t rule, int32_t match_top_k, double kl_thr,
                                    const float* draft_logits, int32_t* counts, int64_t* argmax_out, uint8_t* match_out, int64_t* corrected_out,
                                    const uint8_t* gen, int32_t gen_stride, void* stream);
/* Pixel mask -> token table.  mask_px (B, H, H) uint8, DEVICE: non-zero = regenerate this pixel.  gen (B, L) uint8, L = sum pn_s^2, stage s at
 * columns [begin(s), begin(s) + pn_s^2), row-major (i, j).  Token (i, j) of a stage with side pn owns pixel rows [floor(i H / pn), ceil((i + 1) H / pn))
 * and the same span of columns (the windows of area interpolation; they overlap where pn does not divide H); gen = 1 iff
 * 2 * (non-zero pixels in the window) >= (pixels in the window) - a tie is sampled.  Integer arithmetic, one wave64 per token, no atomics:
 * repeated calls are bit-identical.  1 <= n_stages <= SDVAR_MAX_STAGES, 1 <= pn_s <= H. */
int sdvar_mask_tokens(const uint8_t* mask_px, int32_t B, int32_t H, int32_t n_stages, const int32_t* patch_nums /*host*/, uint8_t* gen, void* stream);
/* out[b,c,y,x] = mask_px[b,y,x] ? fl(fl(gen_img + 1) * 0.5) : fl(fl(orig + 1) * 0.5): gen_img, orig, out (B, C, H, W) fp32, mask_px (B, H, W) uint8, hw = H * W.
 * Two roundings each, as torch's x.add(1).mul(0.5).  16-byte accesses when hw % 4 == 0, the three float pointers are 16-byte aligned and mask_px is
 * 4-byte aligned; one element per thread otherwise.  out may alias gen_img (or orig): every element is read before it is written, by the same thread. */
int sdvar_img_composite(const float* gen_img, const float* orig, const uint8_t* mask_px, int32_t B, int32_t C, int64_t hw, float* out, void* stream);

/* Validation statistics of VARTrainer.eval_ep (trainer.py:66-75) on logits (B, L, V) fp32 against targets (B, L) int64, one wave64 per token:
 * nll = lse - logit[target] (fp32; a target outside [0, V) gives NaN and is never read), argmax with the lowest index on ties.  nll_out (B*L) fp32 and
 * argmax_out (B*L) int64 may be NULL.  sums (4 doubles) = {sum nll, sum nll of the last `tail` tokens of each image, #argmax == target, #tail
 * correct}, overwritten or (accumulate != 0) added to.  Fixed-order reduction, no atomics: repeated calls are bit-identical.  V % 4 == 0, logits
 * 16-byte aligned.  Uses a per-host-thread scratch of 4 doubles per 4 tokens (grown on demand). */
int sdvar_xent_stats(const float* logits, const int64_t* targets, int32_t B, int32_t L, int32_t V, int32_t tail, float* nll_out, int64_t* argmax_out,
                     double* sums, int32_t accumulate, void* stream);
/* Reconstruction error of a validation batch (the L1 / L2 terms of the VAE objective on VQVAE.forward's output, vqvae.py:56-59): over the n fp32
 * elements of a and b, sums (2 doubles) = {sum |a - b|, sum (a - b)^2}, overwritten or (accumulate != 0) added to.  Each difference in fp32, |.| and the
 * square summed in fp64: per-workgroup partials, then one workgroup adds them in a fixed order (no atomics: repeated calls are bit-identical).
 * 16-byte loads when a and b are 16-byte aligned.  Uses a scratch of 2048 doubles per (host thread, device), on the device that is current at the call:
 * calls of one host thread on one device share it and must be on one stream, or ordered by the caller. */
int sdvar_img_err_stats(const float* a, const float* b, int64_t n, double* sums, int32_t accumulate, void* stream);
/* The trainer's loss (VARTrainer, trainer.py:37-38: nn.CrossEntropyLoss(label_smoothing=eps, reduction='none') and (label_smoothing=0, reduction='mean'); called at
 * trainer.py:112 and weighted, summed and averaged at :116-120) on logits (rows, V) fp32 with row stride `ld` elements (unit column stride; a row-sliced view is read in
 * place) against targets (rows) int64, one wave64 per row, ONE pass over the logits:
 *     loss = (1 - eps) (lse - x_t) + eps (lse - sum_j x_j / V)          (torch's label_smoothing = eps; eps == 0 evaluates lse - x_t alone)
 * loss (rows) fp32; lse (rows) fp32 or NULL - the only thing the backward needs beside logits and targets.  target == ignore_index: loss 0, row not counted; any other
 * target outside [0, V): loss NaN (x_t is never read), row counted.  part / sums / reduced may be NULL (all three; reduction 'none'): otherwise part is a caller workspace
 * of 2 * ceil(rows / 4) doubles receiving per-workgroup partials, and a second, single-workgroup launch adds them in a fixed order (no atomics: repeats are
 * bit-identical) into sums (2 doubles) = {sum of loss over counted rows, counted rows} and, if given, reduced (1 float) = sum / count (mean != 0; 0 / 0 = NaN as torch)
 * or sum (mean == 0).  V >= 4, V % 4 == 0, ld >= V, ld % 4 == 0, logits 16-byte aligned, 1 <= rows <= 2^31 - 1, 0 <= eps <= 1: argument errors otherwise, checked
 * before any GPU call.  No allocation, no host synchronisation.  Added without an ABI bump (purely additive).  csrc/xent_train.hip */
int sdvar_xent_train_fwd(const float* logits, int64_t ld, const int64_t* targets, int64_t rows, int32_t V, double label_smoothing, int64_t ignore_index, float* loss,
                         float* lse, double* part /*workspace*/, double* sums, float* reduced, int32_t mean, void* stream);
/* The backward of sdvar_xent_train_fwd (loss.backward() of trainer.py:120 reaching the logits of :112): one read of the logits, one write,
 *     dlogits[row, j] = g_row (exp(x_j - lse_row) - (1 - eps) [j == t_row] - eps / V),
 * dlogits (rows, V) fp32 dense, 16-byte aligned, every element written by exactly one lane.  reduction 0 ('none'): g_row = grad[row]; 2 ('sum'): g_row = grad[0];
 * 1 ('mean'): g_row = grad[0] / sums[1], the counted-row count the forward left on the device.  grad and sums are DEVICE pointers: nothing is read on the host.
 * Ignored rows get zeros (their logits are not read), out-of-range rows NaN.  logits, ld, targets, V, label_smoothing and ignore_index as given to the forward, lse as
 * it wrote it; the same argument checks.  flags bit 0: non-temporal stores for dlogits (same values).  Deterministic. */
int sdvar_xent_train_bwd(const float* logits, int64_t ld, const int64_t* targets, const float* lse, const float* grad, int32_t reduction, const double* sums, int64_t rows,
                         int32_t V, double label_smoothing, int64_t ignore_index, float* dlogits, int32_t flags, void* stream);

/* ---- single operators (kernel-level parity tests and micro-benchmarks) ---------------------------------------------- */
/* out[M,N] = epi(X[M,K] W[N,K]^T + bias); epi 0 bias, 1 bias+GELU(tanh), 2 res + (.)*gate[row / rows_per_gate] */
int sdvar_op_gemm(const float* X, int32_t ldx, const float* W, const float* bias, float* out, int32_t ldo, int32_t M, int32_t N, int32_t K,
                  int32_t epilogue, const float* res, int32_t ldres, const float* gate, int32_t rows_per_gate, int32_t gate_stride, void* stream);
/* bf16x3 plane tensors are K-blocked: element (row, k) of plane p is at p*plane_stride + ((k/32)*rows + row)*32 + k%32.
 * out (fp32) or out_planes (planes of the (rows, C) result, plane stride in elements) */
int sdvar_op_ln_modulate(const float* x, const float* scale, const float* shift, float* out, uint16_t* out_planes, uint64_t plane_stride,
                         int32_t plane_format /* 3 = bf16x3, 2 = f16x2 */, int32_t rows, int32_t C, int32_t rows_per_img, int32_t mod_stride, void* stream);
/* fp32 (rows, cols) row-major -> three K-blocked bf16 planes of 8 significand bits each, x == p0 + p1 + p2 exactly */
int sdvar_op_split_planes(const float* x, uint16_t* planes, int32_t rows, int32_t cols, uint64_t plane_stride, void* stream);
/* the bf16x3 split-operand GEMM on K-blocked planes of X (M,K) and W (N,K); epi 0 bias -> out, 1 bias+GELU -> out_planes of (M,N), 2 gated residual -> out */
int sdvar_op_gemm_bf16x3(const uint16_t* Xp, uint64_t x_plane_stride, const uint16_t* Wp, uint64_t w_plane_stride, const float* bias, float* out,
                         int32_t ldo, uint16_t* out_planes, uint64_t out_plane_stride, int32_t M, int32_t N, int32_t K, int32_t epilogue,
                         const float* res, int32_t ldres, const float* gate, int32_t rows_per_gate, int32_t gate_stride, void* stream);
/* f16x2 operands: fp32 (rows, cols) -> two K-blocked fp16 planes of x * 2^S; scale (4 device floats, may be NULL = no scaling) receives
 * {2^S, 2^-S, scratch, -} with max|x| 2^S in (2^12, 2^13] (weights); the GEMM takes the same pointer and undoes the scale in its epilogue */
int sdvar_op_split_planes_f16(const float* x, uint16_t* planes, int32_t rows, int32_t cols, uint64_t plane_stride, float* scale, void* stream);
int sdvar_op_gemm_f16x2(const uint16_t* Xp, uint64_t x_plane_stride, const uint16_t* Wp, uint64_t w_plane_stride, const float* w_scale, const float* bias, float* out,
                        int32_t ldo, uint16_t* out_planes, uint64_t out_plane_stride, int32_t M, int32_t N, int32_t K, int32_t epilogue,
                        const float* res, int32_t ldres, const float* gate, int32_t rows_per_gate, int32_t gate_stride, void* stream);
/* Single-operator entry points of the attention path (models/basic_var.py:101-117).  kv_f16 = cache format:
 *   0  fp32   K, V (R, H, Lmax, 64)                    1  fp16, same shape (the reference's half-precision cache)
 *   2  bf16x3 planes: K (R, H, 3, Lmax, 64), V^T (R, H, 3, 64, Lmax) with bits 2 and 3 of the key position swapped inside every 16 keys (attention_bf16x3.hip)
 *   3  f16x2 planes:  K AND V (R, H, 2, Lmax, 64) fp16, high plane then low plane, one 128-byte row per position (gemm mode f16x2, the default)
 *   4  one fp16 plane: K and V (R, H, 1, Lmax, 64) = the fp16 KV cache of BASELINE config P4 in the layout of format 3
 * Formats 2-4 need Lmax % 64 == 0 and a zero-initialised cache (whole 32-key tiles are streamed; rows past the valid keys must be finite).
 * "Finite" is all that is asked of rows [Ktot, Lmax): after sdvar_kv_set_len rolls the cursor back (a rejected round of the speculative sampler) they still hold that
 * round's keys and values, and the next append overwrites only its own window.  Attention replaces the scores of those rows before the softmax and gives them a weight
 * of exactly 0: outputs over +-65504 (formats 3, 4) or +-3e38 (format 2) in every plane of the tail are bit-identical to outputs over a zero tail; an inf or NaN there
 * (0 x inf) is not.  Formats 0 and 1 never read past Ktot.
 * Range: formats 3 AND 4 store a finite |k| or |v| beyond 65504 as +-65504 (the append clamps before the fp16 cast; the low plane of format 3 is then zero), so no
 * append of finite values can put an inf into the planes; format 1 casts as torch's .half() does (inf beyond 65520).  Format 2 has no range limit.
 * Every format normalises with the same fp32 arithmetic: q_out and the fp32 value of k that the format then rounds or splits are the same bits in all five formats
 * (format 2 sums to format 0's bits exactly, format 3 to 2^-21.9 relative / 2^-24.9 absolute, formats 1 and 4 are its fp16 rounding).
 * scale_mul == NULL (attn_l2_norm = False): q_out = q * 2^-5 exactly, k is stored as it comes; a zero q or k vector gives zeros (the norm is clamped at 1e-12). */
int sdvar_op_qk_norm_append(const float* qkv, const float* scale_mul, float* q_out, void* k_cache, void* v_cache, int32_t kv_f16, int32_t R,
                            int32_t l, int32_t H, int32_t Lmax, int32_t pos0, void* stream);
/* q (R,H,l,64), caches in format kv_f16 (above) with Ktot valid keys, out (R,l,H*64) fp32 or out_planes (K-blocked operand planes); queries >= qbeg[j] see keys < vis[j] */
int sdvar_op_attention(const float* q, const void* k_cache, const void* v_cache, int32_t kv_f16, float* out, uint16_t* out_planes, uint64_t plane_stride,
                       int32_t plane_format, int32_t R, int32_t H, int32_t l, int32_t Lmax, int32_t Ktot, int32_t n_stages, const int32_t* qbeg /*host*/,
                       const int32_t* vis /*host*/, void* stream);
int sdvar_op_noise_fill(float* q, int32_t B, int32_t l, int32_t V, uint64_t seed, uint32_t draw, uint32_t image_offset, void* stream);
/* The reference's operator slots slow_attn / memory_efficient_attention (models/basic_var.py:27-30, called at :113-117; sdvar_amd/seam.py is the Python side):
 * out = softmax(scale q k^T + bias) v, fp32, head_dim = 64 (anything else is an argument error).  q / out hold Lq tokens, k / v hold Lk tokens, any Lq, Lk >= 1.
 * strides (host, 12 x int64, in ELEMENTS): (batch, head, token) of q, then k, v, out; the channel stride is 1.  Token rows must be 16-byte aligned: every pointer
 * % 16 == 0 and every stride a non-negative multiple of 4.  (B, H, L, 64) tensors, permuted views of a (B, L, 3, H, 64) buffer and (B, L, H, 64) tensors are all strides.
 * bias_kind 0: no bias (bias = NULL); 1: fp32 additive, finite or -inf; 2: uint8 keep-mask (0 = masked, SDPA's bool mask).  bias_strides (host, 3 x int64, elements):
 * (batch, head, query row), 0 = broadcast; the key stride is 1, no alignment rule (rows of a sliced mask work in place).
 * skip_map (device, may be NULL): what sdvar_op_sdpa_skip_map wrote for THIS bias, Lq and Lk; marked tiles cost no K/V traffic and no matrix work.
 * A query row with every key masked has no defined value (NaN here); it does not fault and does not disturb other rows.  No host synchronisation. */
int sdvar_op_sdpa(const float* q, const float* k, const float* v, float* out, const int64_t* strides /*host*/, const void* bias, int32_t bias_kind,
                  const int64_t* bias_strides /*host*/, const uint8_t* skip_map, int32_t B, int32_t H, int32_t Lq, int32_t Lk, int32_t head_dim, double scale, void* stream);
/* skip_map (device, ceil(Lq / 128) * ceil(Lk / 64) bytes): byte (qb, kt) = 1 when bias[bb][hh][128 qb ..][64 kt ..] is masked (-inf / 0) for EVERY bb < Bb, hh < Hb -
 * Bb, Hb = the bias's own batch and head extents (1 where it broadcasts), so a tile that one head needs is never skipped for another.
 * bias_kind 1 / 2 as above; 3 = fp16 additive, 4 = bf16 additive (masked = -inf), for the half biases of sdvar_op_sdpa_hm. */
int sdvar_op_sdpa_skip_map(const void* bias, int32_t bias_kind, const int64_t* bias_strides /*host*/, int32_t Bb, int32_t Hb, int32_t Lq, int32_t Lk, uint8_t* skip_map,
                           void* stream);
/* sdvar_op_sdpa under autograd (the reference's trainer, trainer.py, runs loss.backward() through the teacher-forced slow_attn call of models/basic_var.py:117 with the
 * mask of models/var.py:108-113).  sdvar_op_sdpa_lse = sdvar_op_sdpa (same arguments, same rules, `out` bit-identical) that also writes lse (device, (B, H, Lq) dense
 * fp32): lse[b][h][i] = ln sum_j exp(scale q_i k_j + bias_ij), for every query row it stores; rows of other buffers are never touched.  A fully masked row: unspecified. */
int sdvar_op_sdpa_lse(const float* q, const float* k, const float* v, float* out, float* lse, const int64_t* strides /*host, 12*/, const void* bias, int32_t bias_kind,
                      const int64_t* bias_strides /*host*/, const uint8_t* skip_map, int32_t B, int32_t H, int32_t Lq, int32_t Lk, int32_t head_dim, double scale,
                      void* stream);
/* The backward of sdvar_op_sdpa_lse: with P = exp(scale q k^T + bias - lse) and D_i = sum_d dout_id out_id:  dv = P^T dout,  dS = P o (dout v^T - D),  dq = scale dS k,
 * dk = scale dS^T q.  q, k, v, bias, bias_kind, bias_strides, skip_map, extents and scale exactly as given to the forward; out and lse as the forward wrote them; dout the
 * gradient of out.  strides (host, 24 x int64, elements): (batch, head, token) of q, k, v, out, dout, dq, dk, dv; channel stride 1; the forward's alignment rule for every
 * tensor that is given (pointer % 16 == 0, strides non-negative multiples of 4).  delta (device): workspace of B * H * Lq floats, receives D.  Any of dq, dk, dv may be
 * NULL and is then not computed (its strides are ignored); with dk and dv both NULL the dK/dV kernel is not launched, with dq NULL the dQ kernel is not; all three NULL is
 * an argument error.  fp32 arithmetic on the fp32 matrix cores, no score-sized matrix in memory, tiles the skip map marks are not visited (P = 0 there exactly).
 * Deterministic (no atomics: repeats are bit-identical); no gradient for the bias; a fully masked query row has no defined gradient.  No host synchronisation. */
int sdvar_op_sdpa_bwd(const float* q, const float* k, const float* v, const float* out, const float* dout, const float* lse, float* delta /*workspace*/, float* dq, float* dk,
                      float* dv, const int64_t* strides /*host, 24*/, const void* bias, int32_t bias_kind, const int64_t* bias_strides /*host*/, const uint8_t* skip_map,
                      int32_t B, int32_t H, int32_t Lq, int32_t Lk, int32_t head_dim, double scale, void* stream);
/* Operand producers of the FFN backward (models/basic_var.py:33-52 under autograd; sdvar_amd/seam.py fused_mlp_func_grad; csrc/mlp_bwd.hip).  `format` is the GEMM mode's
 * operand format: 0 = plain fp32 row-major (sdvar_op_gemm), 2 = two K-blocked fp16 planes (sdvar_op_gemm_f16x2), 3 = three K-blocked bf16 planes (sdvar_op_gemm_bf16x3), with
 * the arithmetic of sdvar_op_split_planes_f16 / sdvar_op_split_planes.  Plane strides are in elements, multiples of 8; every pointer 16-byte aligned.  Added without an ABI
 * bump (purely additive).
 * sdvar_op_transpose_operand: x fp32 (rows, cols) with leading dimension ldx (cols % 8 == 0, ldx % 4 == 0) -> the operand of x^T: (cols x Kp), Kp = rows rounded up to 32;
 * format 0: out = float[cols][Kp]; 2 / 3: planes with element (c, k) at ((k/32)*cols + c)*32 + k%32, plane_stride >= cols * Kp.  The tail k >= rows is written as zeros by
 * this kernel in every plane.  scale (format 2 only, may be NULL): device float multiplied into x before the split (element 0 of a scale quadruple). */
int sdvar_op_transpose_operand(const float* x, int32_t ldx, int32_t rows, int32_t cols, int32_t format, void* out, uint64_t plane_stride, const float* scale, void* stream);
/* pre fp32 (M, N) dense, N % 32 == 0 -> the row-major operand of gelu_tanh(pre): format 0 float[M][N], else planes of (M x N).  gelu_kind: 0 = the tanhf form of
 * sdvar_op_gemm / sdvar_op_gemm_bf16x3's epilogue 1, 1 = the exp / rcp form of sdvar_op_gemm_f16x2's - the result has the bits that epilogue writes. */
int sdvar_op_gelu_operand(const float* pre, int32_t M, int32_t N, int32_t format, int32_t gelu_kind, void* out, uint64_t plane_stride, void* stream);
/* dh, pre fp32 (M, N) dense, N % 32 == 0, read once: dpre = dh * gelu_tanh'(pre), h = gelu_tanh(pre) (gelu_kind as above; the derivative is 0 / 1 and finite at large |pre|).
 * Outputs, each may be NULL: dpre = row-major operand (M x N); dpre_t, h_t = transposed operands (N x Mp), Mp = M rounded up to 32, zero tail written here;
 * colsum_part = float[Mp/32][N], the column sums of dpre over each block of 32 rows (finish with sdvar_op_colsum).  scale (format 2 only, may be NULL): device
 * {2^S, 2^-S}; the dpre operands hold dpre * 2^S, h_t and colsum_part are unscaled.  dh may be NULL when only h_t is asked for. */
int sdvar_op_gelu_bwd(const float* dh, const float* pre, int32_t M, int32_t N, int32_t format, int32_t gelu_kind, const float* scale, void* dpre, uint64_t dpre_plane_stride,
                      void* dpre_t, uint64_t dpre_t_plane_stride, void* h_t, uint64_t h_t_plane_stride, float* colsum_part, void* stream);
/* out[n] = sum_m x[m][n], x fp32 (M, N) with leading dimension ldx (N % 4 == 0, ldx % 4 == 0): double accumulation in a fixed order, no atomics (repeats are bit-identical) */
int sdvar_op_colsum(const float* x, int32_t ldx, int32_t M, int32_t N, float* out, void* stream);
/* The scale quadruple {2^S, 2^-S, scratch, 2^-S * other[1]} of an f16x2 operand (4 device floats).  x != NULL: S from max|x| over n values as sdvar_op_split_planes_f16
 * chooses it (all-zero x: S = 0); x == NULL: scale[0..1] are kept.  halve: S -= 1.  scale[3] = 2^-S * (other ? other[1] : 1) is what a GEMM whose two operands are both
 * scaled must undo: hand it `scale + 2` as w_scale. */
int sdvar_op_scale_pair(const float* x, uint64_t n, float* scale, int32_t halve, const float* other, void* stream);
/* The reference's flash_attn_func slot (models/basic_var.py:23, called at :112-113 when KV caching is on and qkv is not fp32, :97-98): out = softmax(scale q k^T) v on
 * fp16 or bf16 operands (dtype 1 = fp16, 2 = bf16; q, k, v and out all of it), no bias.  head_dim must be 64; Lq and Lk are independent, any value >= 1.
 * strides as for sdvar_op_sdpa (host, 12 x int64, elements: (batch, head, token) of q, k, v, out; channel stride 1).  A 64-element row is 128 bytes and is moved with 16-byte
 * accesses: every pointer % 16 == 0 and every stride a non-negative multiple of 8 elements.  Scores, softmax and the output accumulate in fp32 (scale multiplies the fp32
 * score); the softmax weights are rounded to dtype (nearest even) for the P V product and the result is rounded once.  Deterministic; no host synchronisation. */
int sdvar_op_sdpa_h(const void* q, const void* k, const void* v, void* out, const int64_t* strides /*host*/, int32_t dtype, int32_t B, int32_t H, int32_t Lq, int32_t Lk,
                    int32_t head_dim, double scale, void* stream);

/* conv weight (Cout, Cin, kh, kw) with kh*kw = taps (1 or 9) -> K-blocked planes [3][taps*Cin/32][Cout][32], k = tap*Cin + cin */
int sdvar_op_conv_weight_planes(const float* w, uint16_t* planes, int32_t Cout, int32_t Cin, int32_t taps, uint64_t plane_stride, int32_t plane_format /* 3 | 2 */,
                                float* scale /* f16x2: receives {2^S, 2^-S, ..} (4 device floats), may be NULL */, void* stream);
/* fp32 channel-last rows [B H W][C] of a (B,C,H,W) tensor -> planes [3][C/32][guard + B(Ho+2)(Wo+2) + guard][32] of the
 * (B,C,H<<up,W<<up) tensor over padded pixel rows (prow(b,y,x) = (b(Ho+2)+y+1)(Wo+2)+x+1, zero frame and guards).
 * mode bit 0: GroupNorm(32 groups) with stats (B,32,{mean,rstd}), gamma, beta; bit 1: SiLU. */
int sdvar_op_vae_prep(const float* in, const float* stats, const float* gamma, const float* beta, uint16_t* planes, uint64_t plane_stride, int32_t plane_format, int32_t B,
                      int32_t C, int32_t H, int32_t W, int32_t up, int32_t mode, int32_t guard, void* stream);
/* encoder conv_in operand: img (B,3,H,W) fp32 -> planes [npl][1][guard + B(H+2)(W+2) + guard][32] (channels 3..31 zero) */
int sdvar_op_vae_img_planes(const float* img, uint16_t* planes, uint64_t plane_stride, int32_t plane_format, int32_t B, int32_t H, int32_t W, int32_t guard, void* stream);
/* Downsample2x operand: rows [B H W][C] -> planes of the space-to-depth tensor (B, 4C, H/2, W/2), channel (2py+px)C + c = x[2y+py][2x+px][c] */
int sdvar_op_vae_s2d_planes(const float* in, uint16_t* planes, uint64_t plane_stride, int32_t plane_format, int32_t B, int32_t C, int32_t H, int32_t W, int32_t guard,
                            void* stream);
/* Downsample2x weight (Cout, C, 3, 3) -> the 3x3 weight (Cout, 4C, 3, 3) over the space-to-depth tensor (fp32) */
int sdvar_op_vae_s2d_weights(const float* w, float* w_s2d, int32_t Cout, int32_t C, void* stream);
/* nearest code of z (N, cvae = 32) in codebook (V, cvae): ids (N) int64, ties to the lowest index; e2 (V floats) receives |e_v|^2 */
int sdvar_op_quant_nearest(const float* z, int32_t N, const float* codebook, int32_t V, int32_t cvae, float* e2, int64_t* ids, void* stream);
/* out[B H W][N] = conv(x planes of a (B,Cin,H,W) tensor, w planes) + bias (+ res[B H W][N]); taps = 9: 3x3 pad 1, taps = 1: 1x1.  x_row0 =
 * guard rows (>= W+3).  workspace: split-K slabs (may be NULL: no split); force_split > 0 overrides the heuristic.
 * plane_format: 3 = bf16x3, 2 = f16x2 (three fp16 products), 6 = f16x2 planes multiplied as ONE product, x plane 0 times w plane 0 (plane 1 of either operand is never
 * read; fp32 accumulation, same epilogues; N % 4 == 0 or SDVAR_ERR_ARG).  The operands of format 6 are format-2 planes: pack and produce them with plane_format 2.
 * Format 6 runs the one-product instances of the "conv_pp" 2 loop and of the tap-reuse loop (same eligibility rule) whatever "conv_pp" says; "conv_tap_reuse" 0 still
 * forces the per-tap loop. */
int sdvar_op_conv_planes(const uint16_t* x_planes, uint64_t x_plane_stride, uint64_t x_rows, int32_t x_row0, const uint16_t* w_planes, uint64_t w_plane_stride,
                         int32_t plane_format, const float* w_scale, const float* bias, const float* res, float* out, int32_t B, int32_t H, int32_t W, int32_t N,
                         int32_t Cin, int32_t taps, float* workspace, uint64_t workspace_floats, int32_t force_split, void* stream);
/* sdvar_op_conv_planes with the decoder's two extras.  up_phase >= 0 (taps = 4, no res, no split): the convolution of the nearest-2x up-sampled
 * (B, Cin, 2H, 2W) tensor into out[B 2H 2W][N], from the x planes of the (B, Cin, H, W) input and four phase weight sets (sdvar_op_upconv_weights),
 * w_phase_stride elements apart.  gn_part (device, B (H W / 256) 64 doubles, x4 with up_phase; may be NULL): when the convolution can fuse the
 * GroupNorm statistics of its output into the epilogue (no split-K, H W % 256 == 0, N % 32 == 0 and (N / 32) | 160), it does, finalises them into
 * stats (device, (B, 32, {mean, rstd}), eps 1e-6) and sets *gn_done (host) = 1; else *gn_done = 0 and stats is untouched. */
int sdvar_op_conv_planes_ex(const uint16_t* x_planes, uint64_t x_plane_stride, uint64_t x_rows, int32_t x_row0, const uint16_t* w_planes, uint64_t w_plane_stride,
                            int32_t plane_format, const float* w_scale, const float* bias, const float* res, float* out, int32_t B, int32_t H, int32_t W, int32_t N,
                            int32_t Cin, int32_t taps, float* workspace, uint64_t workspace_floats, int32_t force_split, int32_t up_phase, uint64_t w_phase_stride,
                            double* gn_part, float* stats, int32_t* gn_done, void* stream);
/* Upsample2x weight (Cout, Cin, 3, 3) -> weff [4 phases (py, px)][Cout][Cin][4 taps (ty, tx)] fp32: the 2x2 convolution of each output phase on the
 * input grid.  The decoder packs phase p with conv weight planes (taps = 4, plane stride wps = 4 Cin Cout) at planes + p * npl * wps (npl = 3 bf16x3 |
 * 2 f16x2 planes), so w_phase_stride = npl * wps; in f16x2 one weight scale (sdvar_op_split_planes_f16 over all of weff) serves all four phases. */
int sdvar_op_upconv_weights(const float* w, float* weff, int32_t Cout, int32_t Cin, void* stream);
/* The decoder's stand-alone GroupNorm statistics of rows [B H W][C] ((C/4) | 320): stats (B, 32, {mean, rstd}), eps 1e-6.  part_ws: B min(H, 64) 64 doubles. */
int sdvar_op_vae_gn_stats(const float* x_rows, int32_t B, int32_t C, int32_t H, int32_t W, double* part_ws, float* stats, void* stream);
/* AttnBlock core of the decoder: qkv rows [B N][3C] (q | k | v) -> out rows [B N][C] = softmax(q k^T / sqrt(C)) v.  kernel: -1 = the decoder's choice
 * (1 for N in {256, 1024} and C % 64 == 0, else 0 while its LDS fits, else 2); 0 = fp32 FMA, probabilities in LDS (N <= 1612); 1 = fp32 matrix cores
 * (N in {256, 1024}, C % 64 == 0); 2 = probabilities in workspace (ceil(N / 16) N 20 floats per image; as many images per launch as ws_floats holds).
 * A forced kernel that cannot take the shape returns SDVAR_ERR_ARG. */
int sdvar_op_vae_attn(const float* qkv, float* out, int32_t B, int32_t C, int32_t N, float* workspace, uint64_t ws_floats, int32_t kernel, void* stream);
/* norm_out + SiLU + conv_out (3 x C x 3 x 3, pad 1) + bias, clamped to [-1, 1]: x rows [B H W][C], stats (B, 32, {mean, rstd}) -> img (B, 3, H, W).
 * workspace: (C + B H W) 28 floats. */
int sdvar_op_vae_conv_out(const float* x_rows, const float* stats, const float* gamma, const float* beta, const float* w, const float* bias, float* img, int32_t B,
                          int32_t C, int32_t H, int32_t W, float* workspace, void* stream);
/* tuning / test aid (tools/gemm_bench.py --sweep): force the GEMM row tile (32/64/128/256) and K-slice count; 0 = automatic.  f16x2 mode only: bm 512 = the
 * 256 x 256 tile kernel; bm 256 with split = -T forces the hybrid tail split T ways on shapes that have a partial last round. */
int sdvar_debug_set_gemm_cfg(int32_t bm, int32_t split);
/* test aid: 0 = the QKV launch of sdvar_stage_forward never finishes q and k in its epilogue (qk_norm_append does all three), 1 (default) = it does
 * whenever the launch comes out unsplit on the f16x2 planes cache */
int sdvar_debug_set_qkv_fuse(int32_t on);
/* 1 (default): stage_forward calls with 32 .. 80 rows (stage 1, the first verify chunk at B = 8) in GEMM mode f16x2 run five launches per transformer block - LayerNorm +
 * modulation in the operand prologue of the QKV / fc1 / head launch, q / k / v finished by the QKV launch, fc2 unsplit (csrc/gemm_f16x2.hip gemm_f16x2_rowblk_kernel);
 * 0: the launch sequence of every other row count (ln_modulate, GEMM, qk_norm_append: eight launches); 2: five launches at every row count up to 80 (below 32 rows they are SLOWER than the eight: measured).
 * Test / A-B aid (SDVAR_ROWBLK in the environment does the same). */
int sdvar_debug_set_rowblk(int32_t on);
/* The row-block launch alone (M <= 80).  x != NULL: out = epi( (LayerNorm(x; eps 1e-6)(1 + scale[g]) + shift[g]) W^T + bias ), g = row / rows_per_img, K <= 1024, epi 0 (-> out) or
 * 1 (GELU -> out_planes); with q_out != NULL the QKV finish instead (N = 3 H 64; q -> (R, H, l, 64) fp32, k normalised / v -> the cache planes at pos0 + t, kv_fmt 3 | 4) and nothing
 * goes to `out`.  x == NULL: the operand is Xp (K-blocked f16x2 planes, K <= 4096), epi 0 or 2 (gated residual). */
int sdvar_op_gemm_rowblk(const float* x, int32_t ldx, const float* scale, const float* shift, int32_t rows_per_img, int32_t mod_stride, const uint16_t* Xp, uint64_t x_plane_stride,
                         const uint16_t* Wp, uint64_t w_plane_stride, const float* w_scale, const float* bias, float* out, int32_t ldo, uint16_t* out_planes, uint64_t out_plane_stride,
                         int32_t M, int32_t N, int32_t K, int32_t epilogue, const float* res, int32_t ldres, const float* gate, int32_t rows_per_gate, int32_t gate_stride,
                         const float* scale_mul, float* q_out, void* k_cache, void* v_cache, int32_t l, int32_t H, int32_t Lp, int32_t pos0, int32_t kv_fmt, void* stream);
/* Select a kernel variant that otherwise only an environment variable (read at first use) selects - tests run the non-default variants in one process.
 * name: "gemm_h4_var" 0..3, "gemm_h2_stages" 2..6, "gemm_small_pp" 0..2, "attn_pp_sched" 0..3, "conv_pp" 0..2, "conv_tap_reuse" 0..1 (SDVAR_CONV_TAP_REUSE, read per call like
 * SDVAR_CONV_PP: 1 = the f16x2 decoder convolution stages X once per row of taps where the shape allows it, 0 = never); value < 0 restores the environment / default.
 * A lookup in the library's one table of process-wide switches (csrc/gemm_plan.h), which sdvar_debug_set_rowblk ("rowblk" 0..2), sdvar_debug_set_qkv_fuse
 * ("qkv_fuse" 0..1) and sdvar_debug_set_gemm_cfg write too; "gemm_v2" 0..1 (bf16x3: the 128-row tile on the LDS-DMA kernel, default 1) has no other setter.
 * "stage0_table" 0..1 (SDVAR_STAGE0_TABLE) and "stage0_table_mb" 0..2^20 (SDVAR_STAGE0_TABLE_MB, default 1024): sdvar_stage_first's per-class table and its size cap.
 * "h16_min_m" 1..2^30 (SDVAR_H16_MIN_M): rows from which a call of a gemm_mode 3 model takes the half kernel; below it the call is mode 2's, bit for bit.
 * Every one of these setters except the two stage-0 ones moves an epoch that makes the next sdvar_model_begin rebuild that table. */
int sdvar_debug_set_variant(const char* name, int32_t value);
/* test aid: out4 = {kernel code (as sdvar_debug_plan_gemm; 17 = row-block launch) of the LAST f16x2 GEMM call of this host thread, its K split, number of launches that took the hybrid tail
 * split since the last read, number of QKV launches that finished q and k in their epilogue since the last read}; reading resets the two counters.
 * Tests assert with it that the path they mean to cover is the one that ran. */
int sdvar_debug_get_gemm_cfg(int32_t* out4);
/* test aid: out1[0] = 1 if the LAST convolution launch (sdvar_op_conv_planes / _ex, the decoder's convolutions) of this host thread took the tap-reuse K loop
 * (f16x2 planes, "conv_pp" 2, "conv_tap_reuse" 1, 3x3 or fused up-sampling taps, no split-K, H W % 256 == 0, W % 256 == 0 or 256 % W == 0 with W >= 64), else 0. */
int sdvar_debug_get_conv_cfg(int32_t* out1);
/* test aid: out4 = what the LAST convolution launch of this host thread ran: {kernel: 0 bf16x3 | 1 f16x2 | 2 f16x2 tap-reuse | 3 one-product per-tap | 4 one-product
 * tap-reuse (plane_format 6); the "conv_pp" loop actually used (2 falls back to 1 when N % 4 != 0; 0 for bf16x3, which has one loop; always 2 for plane_format 6); the K split actually used (1 = none; a forced split is rounded to the number of non-empty slices);
 * 1 if the GroupNorm statistics were fused into the epilogue}.  All four are -1 before the first launch.  Thread-local, like sdvar_debug_get_conv_cfg. */
int sdvar_debug_get_conv_plan(int32_t* out4);
/* The GEMM planner (csrc/gemm_plan.h) on its own: what a GEMM of this shape would launch.  Pure host code - no HIP call, no GPU needed; a pure function of the
 * arguments, the switches above and the SDVAR_GEMM_* environment.  mode: 0 f32, 1 bf16x3, 2 f16x2.  flags: bit 0 = the caller defers the K-slice sum to its
 * consumer kernel, bit 1 = the call offers a QKV finish for the epilogue (sdvar_stage_forward's QKV launch), bit 2 = every output pointer and leading dimension
 * allows 16-byte accesses (bits 0 and 1 matter in mode 2 only).  out4 = {kernel code, K split, hybrid tail split (0 = none), 1 if the QKV finish runs in the
 * epilogue}; kernel codes: 16 = skinny (M <= 80), 32 / 64 / 128 / 256 = rows of a (rows x 128) tile, 512 = 256 x 256, 768 = 256 x 192 (17, the row-block
 * launch, is asked for by its callers and never planned).  After an f16x2 GEMM call sdvar_debug_get_gemm_cfg reports the same kernel code and split.
 * The f16 tier (sdvar_model_desc.gemm_mode 3) is a mode-2 model with one flag, and is planned as such: mode 2 with flags bit 3 (value 8) gives {1128, 1, 0, 0} = the
 * 128 x 128 half kernel when M >= "h16_min_m", else mode 2's plan for the other flag bits; sdvar_debug_get_gemm_cfg reports 1128 after such a launch.  `mode` itself stays
 * 0..2: 3 is rejected as before. */
int sdvar_debug_plan_gemm(int32_t mode, int32_t M, int32_t N, int32_t K, int32_t flags, int32_t* out4);
/* f16x2 guard (debug, off by default; mode f16x2 only).  The f16x2 operand format of the default GEMM mode saturates finite activations at +-65504 and loses
 * relative precision below ~1e-3 (the reference computes these GEMMs in fp32: basic_var.py:44-52, 87-119).  With the guard on, every producer of GEMM operand
 * planes inside sdvar_stage_forward (ln_modulate, attention, the fc1 GELU epilogue) is followed by a counting pass over the plane it wrote.
 * sdvar_debug_get_f16x2_guard synchronises the device and returns out4 = {elements seen, saturated (|h| == 65504), NaN / Inf, tiny (0 < |h| < 2^-10)};
 * reset != 0 zeroes the counters.  A non-zero `saturated` or `NaN` count means the run left the range f16x2 is exact in: use gemm_mode bf16x3 (no range limit). */
int sdvar_debug_set_f16x2_guard(int32_t on);
int sdvar_debug_get_f16x2_guard(uint64_t* out4, int32_t reset);
/* diagnostic: per-workgroup stamps of the LDS-DMA GEMM kernels; NULL disables.  bf16x3 kernel: 4 x u64 per workgroup (s_memtime at entry, main loop
 * start, main loop end, exit); f16x2 small-M and 128 x 128 kernels: 8 x u64 (s_memrealtime at entry, first K-step landed, loop end, exit; then s_memtime) */
int sdvar_debug_set_gemm_stamps(uint64_t* stamps);

/* ---- per-kernel-class timing with HIP events on the launch stream (bench.py roofline leg) ----------------------------- */
#define SDVAR_PROF_CLASSES 10  /* 0 gemm with M >= 1024 rows (matrix-pipe regime), 1 attention with more than 36 queries per (row, head) (matrix-pipe bound),
                                  2 ln_modulate, 3 qk_norm_append, 4 sampler, 5 verify, 6 quant, 7 embed/misc, 8 attention with <= 36 queries (stages 0-5: HBM /
                                  latency bound), 9 gemm with M < 1024 rows (stages 0-5, adaLN hoist: weight-streaming / launch-latency regime) */
int sdvar_prof_enable(int32_t on);
/* synchronises the recorded events and accumulates: ms, launches, algorithmic flops, algorithmic bytes per class */
int sdvar_prof_collect(double* ms /*host[SDVAR_PROF_CLASSES]*/, int64_t* launches, double* flops, double* bytes);

/* The slow_attn / memory_efficient_attention slots under torch.autocast (sdvar_amd/seam.py: slow_attn_amp, memory_efficient_attention_amp): out = softmax(scale q k^T + bias) v
 * with the arithmetic of sdvar_op_sdpa_h (native fp16 / bf16 matrix cores, fp32 scores / softmax / accumulation, one RNE rounding of the softmax weights and of the
 * result).  dtype (1 = fp16, 2 = bf16) is the type of v, of out and of the matrix-core operands; q (q_f32 = 1) and k (k_f32 = 1) may each be fp32 instead and are then
 * rounded to dtype (nearest even) as they are read: the same bits as a prior cast.  strides as for sdvar_op_sdpa (host, 12 x int64: (batch, head, token) of q, k, v, out),
 * each in ITS operand's elements; every pointer % 16 == 0; strides of a half operand are non-negative multiples of 8, of an fp32 operand of 4.  head_dim must be 64.
 * bias_kind 0: none (bias = NULL); 1: fp32 additive, finite or -inf; 2: uint8 keep-mask (0 = masked); 3: additive in dtype.  bias_strides (host, 3 x int64, elements):
 * (batch, head, query row), 0 = broadcast; key stride 1; rows need no alignment (sliced masks are read in place).  The bias is added to the fp32 score.
 * skip_map (device, may be NULL; needs a bias): what sdvar_op_sdpa_skip_map wrote for THIS bias, Lq and Lk (its kind 3 / 4 for a half bias); marked tiles are never
 * read or multiplied, and the result is the same bits with and without the map.  A query row with every key masked has no defined value (NaN here); it does not
 * fault and does not disturb other rows.  Deterministic; no host synchronisation. */
int sdvar_op_sdpa_hm(const void* q, const void* k, const void* v, void* out, const int64_t* strides /*host, 12*/, int32_t dtype /*1 fp16 | 2 bf16*/, int32_t q_f32,
                     int32_t k_f32, const void* bias, int32_t bias_kind /*0 none | 1 fp32 | 2 uint8 keep | 3 additive in dtype*/, const int64_t* bias_strides /*host, 3*/,
                     const uint8_t* skip_map, int32_t B, int32_t H, int32_t Lq, int32_t Lk, int32_t head_dim, double scale, void* stream);

/* The same slots under torch.autocast AND autograd (the reference's mixed-precision trainer: utils/amp_sc.py wraps the step in torch.autocast; sdvar_amd/seam.py:
 * slow_attn_amp_grad, memory_efficient_attention_amp_grad, flash_attn_func_grad).  Both entries were added WITHOUT an ABI bump (purely additive).
 * sdvar_op_sdpa_hm_lse = sdvar_op_sdpa_hm (same arguments and rules; it also accepts bias_kind 0 with three half operands, and `out` is then bit-identical to
 * sdvar_op_sdpa_h's, otherwise to sdvar_op_sdpa_hm's) that also writes lse (device, (B, H, Lq) dense fp32): lse[b][h][i] = ln sum_j exp(scale q_i k_j + bias_ij) from the
 * fp32 scores of the rounded operands (the kernel's running maximum and fp32 row sum, converted from base 2), for every query row it stores; rows past Lq are never
 * written.  A fully masked row: -inf. */
int sdvar_op_sdpa_hm_lse(const void* q, const void* k, const void* v, void* out, float* lse, const int64_t* strides /*host, 12*/, int32_t dtype /*1 fp16 | 2 bf16*/,
                         int32_t q_f32, int32_t k_f32, const void* bias, int32_t bias_kind /*0 none | 1 fp32 | 2 uint8 keep | 3 additive in dtype*/,
                         const int64_t* bias_strides /*host, 3*/, const uint8_t* skip_map, int32_t B, int32_t H, int32_t Lq, int32_t Lk, int32_t head_dim, double scale,
                         void* stream);
/* The backward of sdvar_op_sdpa_hm_lse on the half-precision matrix cores (csrc/attention_sdpa_h_bwd.hip).  q, k, v, dtype, q_f32, k_f32, bias, bias_kind, bias_strides,
 * skip_map, extents and scale exactly as given to the forward; out and lse as the forward wrote them; dout the gradient of out.  Three launches (D, dK/dV, dQ), no
 * score-sized matrix in memory, tiles the skip map marks are not visited, no atomics (every output element is reduced in a fixed order: repeats are bit-identical), no
 * host synchronisation.  delta (device): workspace of B * H * Lq floats, receives D.  Any of dq, dk, dv may be NULL and is then not computed (its strides are ignored);
 * with dk and dv both NULL the dK/dV kernel is not launched, with dq NULL the dQ kernel is not; all three NULL is an argument error.
 * strides (host, 24 x int64): (batch, head, token) of q, k, v, out, dout, dq, dk, dv, each in ITS tensor's elements; channel stride 1; every given pointer % 16 == 0;
 * strides of a half tensor are non-negative multiples of 8, of an fp32 tensor of 4.  head_dim must be 64; any Lq, Lk >= 1.
 * Arithmetic contract:
 *   - dtype (1 fp16, 2 bf16) is the type of v, out, dout and dv.  q and k may each be fp32 (q_f32 / k_f32) and are then rounded to dtype (nearest even) as they are read:
 *     the same bits as in the forward.
 *   - P = exp(scale q k^T + bias - lse) is recomputed in fp32 from the half-precision matrix-core scores, with the forward's score expression in base 2.
 *   - D_i = sum_d dout_id out_id, accumulated in fp32 from the stored half values.
 *   - dV = P^T dout with P rounded to dtype (nearest even), fp32 accumulation.  dP = dout v^T on the half matrix cores, fp32 accumulation.
 *   - dS = P o (dP - D) in fp32, rounded once to dtype (nearest even).  dQ = scale (dS K), dK = scale (dS^T Q), fp32 accumulation; scale multiplies the fp32 accumulator.
 *   - each gradient is stored once: dv in dtype; dq in q's type and dk in k's type - fp32 (unrounded) when that operand was fp32, else rounded once to dtype.
 *   - no clamping: a value beyond fp16's range becomes +-inf exactly as a cast would (a GradScaler relies on seeing inf to skip a step).
 *   - a -inf bias entry inside a visited tile gives P = dS = 0.  A fully masked query row has no defined gradient; it does not fault and does not disturb other rows.
 * No gradient for the bias. */
int sdvar_op_sdpa_h_bwd(const void* q, const void* k, const void* v, const void* out, const void* dout, const float* lse, float* delta /*workspace*/, void* dq, void* dk,
                        void* dv, const int64_t* strides /*host, 24*/, int32_t dtype /*1 fp16 | 2 bf16*/, int32_t q_f32, int32_t k_f32, const void* bias,
                        int32_t bias_kind /*0 none | 1 fp32 | 2 uint8 keep | 3 additive in dtype*/, const int64_t* bias_strides /*host, 3*/, const uint8_t* skip_map,
                        int32_t B, int32_t H, int32_t Lq, int32_t Lk, int32_t head_dim, double scale, void* stream);

/* The half-precision FFN of a model run under torch.autocast (sdvar_amd/seam.py fused_mlp_func_amp / fused_mlp_func_amp_grad; csrc/gemm_half.hip, csrc/mlp_half.hip).
 * Added without an ABI bump (purely additive).  dtype: 1 = fp16, 2 = bf16.  An OPERAND is one K-blocked plane of that dtype: element (row, k) of a (rows x K) matrix at
 * ((k/32)*rows + row)*32 + k%32, K % 32 == 0, rows * K elements; every pointer 16-byte aligned.  Nothing is scaled or clamped anywhere: an fp16 overflow is +-inf.
 *
 * sdvar_op_gemm_h: out[M,N] = epilogue(X[M,K] . W[N,K]^T + bias[N]), x = operand (M x K), w = operand (N x K).  Arithmetic contract:
 *   - every product on the half matrix cores (v_mfma_f32_32x32x16_f16 / _bf16: exact products, fp32 accumulation over k in ascending order, one chain per output element;
 *     fp16 subnormal inputs are kept); the fp32 bias (may be NULL) is added to the fp32 sum; nothing is rounded before that.
 *   - epilogue 0: out (row-major, leading dimension ldo, ldo % 4 == 0) = that fp32 value (out_dtype 0) or the value rounded once to dtype, nearest even, overflow = inf
 *     (out_dtype = dtype).  h_out and pre_out must be NULL.
 *   - epilogue 1 (fc1; N % 32 == 0): p = dtype(sum + bias); h = dtype(gelu_tanh(float(p))) with the exp / rcp form of sdvar_op_gemm_f16x2's GELU; h_out = the OPERAND
 *     (M x N) of the next GEMM; pre_out (may be NULL) = p row-major dense (M, N) in dtype.  out must be NULL.
 *   - any M >= 1 (edge rows are clamped on load and never stored), N % 8 == 0, K % 32 == 0.  No split-K, no atomics: repeats are bit-identical, and an element's bits do
 *     not depend on M or N.  Argument errors (NULL / misaligned pointers, K % 32, N % 8, unknown dtype / epilogue / out_dtype) are reported before any launch. */
int sdvar_op_gemm_h(const void* x, const void* w, int32_t dtype, const float* bias, void* out, int32_t out_dtype, int32_t ldo, void* h_out, void* pre_out, int32_t M, int32_t N,
                    int32_t K, int32_t epilogue, void* stream);
/* The same kernel as the engine's GEMM mode 3 ("f16") launches it on the HIGH planes of f16x2 operands (added without an ABI bump; fp16 only: dtype must be 1).  Differences
 * from sdvar_op_gemm_h:
 *   - w_scale (device float, may be NULL = 1): the fp32 sum is multiplied by *w_scale before the bias is added, in every epilogue.  The engine passes the 2^-S entry of an
 *     f16x2 weight scale (the high plane of such a weight is fp16(w * 2^S)); a power of two makes the product exact.
 *   - out is fp32 only (no out_dtype).
 *   - epilogue 1 saturates the pre-activation at +-65504 before it is rounded to fp16, as every f16x2 operand producer does; finite results are those of sdvar_op_gemm_h.
 *   - epilogue 2 (gated residual): out[m,n] = res[m,n] + (sum * *w_scale + bias[n]) * gate[(m / rows_per_gate) * gate_stride + n]; res, gate, out fp32 row-major with leading
 *     dimensions ldres / ldo (each >= N, % 4 == 0; gate_stride % 4 == 0), rows_per_gate >= 1.  res == out (in place) is allowed: an element is read and written by one lane.
 *     h_out and pre_out must be NULL; res and gate must be NULL for epilogues 0 and 1.
 * Argument errors, also a NULL res / gate with epilogue 2, rows_per_gate < 1 and a pointer that is not 16-byte aligned, are reported before any launch. */
int sdvar_op_gemm_h_ex(const void* x, const void* w, int32_t dtype, const float* w_scale, const float* bias, float* out, int32_t ldo, void* h_out, void* pre_out, const float* res,
                       int32_t ldres, const float* gate, int32_t rows_per_gate, int32_t gate_stride, int32_t M, int32_t N, int32_t K, int32_t epilogue, void* stream);
/* x row-major (rows, cols), leading dimension ldx, fp32 (x_dtype 0; ldx % 4 == 0) or already of dtype (x_dtype = dtype; ldx % 8 == 0) -> an OPERAND of dtype.  fp32 values are
 * rounded to nearest even - the bits of a cast - and an fp16 overflow becomes inf; half values are copied bit for bit.  transpose 0: the operand (rows x cols), cols % 32 == 0.
 * transpose 1: the operand of x^T, (cols x Kp), Kp = rows rounded up to 32, cols % 8 == 0; the tail k >= rows is written as zeros by this kernel.  colsum_part (transpose 1 only,
 * may be NULL) = float[Kp/32][cols]: the column sums of the ROUNDED x over each block of 32 rows, added in row order in fp32 (finish with sdvar_op_colsum); with it, out may be
 * NULL. */
int sdvar_op_half_operand(const void* x, int32_t x_dtype, int32_t ldx, int32_t rows, int32_t cols, int32_t dtype, int32_t transpose, void* out, float* colsum_part, void* stream);
/* dh fp32 (M, N) dense and pre = the half pre-activation p (M, N) dense in dtype (sdvar_op_gemm_h epilogue 1), N % 32 == 0, read once:
 *   dpre = dtype(dh * g'(float(p))), h = dtype(gelu_tanh(float(p))) - the bits the fc1 epilogue wrote; g' is the exp / rcp formulation of sdvar_op_gelu_bwd (gelu_kind 1): finite
 *   at both ends (0 / 1 at large |p|, no 0 * inf), so dpre is inf or NaN only where dh is.
 * Outputs, each may be NULL: dpre = OPERAND (M x N); dpre_t, h_t = OPERANDS (N x Mp) of the transposes, Mp = M rounded up to 32, zero tail written here; colsum_part =
 * float[Mp/32][N], the column sums of the ROUNDED dpre over each block of 32 rows, added in row order in fp32 (finish with sdvar_op_colsum).  dh may be NULL when only h_t is
 * asked for. */
int sdvar_op_gelu_bwd_h(const float* dh, const void* pre, int32_t M, int32_t N, int32_t dtype, void* dpre, void* dpre_t, void* h_t, float* colsum_part, void* stream);

/* ---- the dense linears under autograd (the reference's mat_qkv, proj, ada_lin, word_embed and head; sdvar_amd/seam.py linear_grad / linear_amp_grad) ------------------
 * csrc/linear_train.hip.  Added without an ABI bump (purely additive).  y = x W^T + b, dx = dy W, dW = dy^T x, db = sum_m dy: the three entries below make ONE pass over dy
 * and write everything the two gradient GEMMs and db read.  Every pointer 16-byte aligned; argument errors (NULL or misaligned pointers, cols % 32, an unknown format or
 * dtype, every output NULL) are reported before any launch.  No atomics, no host synchronisation.
 * sdvar_op_grad_operands: dy fp32 (rows, cols) with leading dimension ld (cols % 32 == 0, ld % 4 == 0, rows >= 1), read once.  Outputs, each may be NULL:
 *   out         the row-major operand (rows x cols) of dy * scale[0]: format 2 = the bits of sdvar_op_split_planes_f16 with that scale, 3 = those of sdvar_op_split_planes;
 *               format 0 has none (dy itself is the operand: out must be NULL).  Plane strides in elements, multiples of 8, at least the operand.
 *   out_t       the operand of dy^T, (cols x Mp), Mp = rows rounded up to 32, zero tail written here: the bits of sdvar_op_transpose_operand in formats 0 / 2 / 3.
 *   colsum_part float[Mp/32][cols]: the column sums of the UNSCALED dy over each block of 32 rows, added in row order in fp32 (finish with sdvar_op_colsum).
 * scale (format 2 only, may be NULL): a device scale pair {2^S, 2^-S, ..} as sdvar_op_gelu_bwd takes it. */
int sdvar_op_grad_operands(const float* dy, int32_t ld, int32_t rows, int32_t cols, int32_t format, const float* scale, void* out, uint64_t out_plane_stride, void* out_t,
                           uint64_t out_t_plane_stride, float* colsum_part, void* stream);
/* The same pass for the half matrix cores.  dtype: 1 = fp16, 2 = bf16; x_dtype: 0 = fp32 input, rounded to nearest even as it is read, else = dtype (ld % 8 == 0 then).
 * out = OPERAND (rows x cols), out_t = OPERAND (cols x Mp) of the transpose: the bits sdvar_op_half_operand writes with transpose 0 / 1; colsum_part = the bits of that
 * entry's colsum_part (sums of the ROUNDED values).  Each may be NULL, not all three. */
int sdvar_op_grad_operands_h(const void* dy, int32_t x_dtype, int32_t ld, int32_t rows, int32_t cols, int32_t dtype, void* out, void* out_t, float* colsum_part, void* stream);
/* in = a K-blocked operand (rows x K) of 16-bit elements (either dtype: the bits move untouched), K % 32 == 0 -> out = the operand of its transpose, (K x Mp), Mp = rows
 * rounded up to 32, zero tail written here: bit-identical to sdvar_op_half_operand(.., transpose = 1) on the row-major matrix the operand was made from. */
int sdvar_op_operand_transpose_h(const void* in, int32_t rows, int32_t K, void* out, void* stream);

/* ---- the adaLN modulation and the gated residual of a block under autograd (AdaLNSelfAttn.forward, basic_var.py:152-159; AdaLNBeforeHead.forward, :172-174) ----------
 * csrc/adaln_train.hip.  Added without an ABI bump (purely additive).  Common to the six entry points:
 *   - x, out, g, dx are (B, L, C) fp32, dense, 16-byte aligned; C % 4 == 0, 4 <= C <= 3072, B, L >= 1, B * L <= 2^29.  One wave64 per row, float4 accesses.
 *   - a modulation vector (scale, shift, gamma) is one row of C values per image: dtype code 0 fp32, 1 fp16, 2 bf16 (each vector on its own), row b at
 *     base + b * batch_stride ELEMENTS (0: one row for every image); the base and every row 16-byte aligned.  A half value is widened to fp32 before any arithmetic.
 *   - argument errors (shape, NULL, dtype code, alignment) are reported before any launch; no allocation, no host synchronisation, no atomics: repeats are
 *     bit-identical.  Nothing is clamped.
 * sdvar_op_adaln_fwd: out = ((x - mean) * rstd) * (scale + 1) + shift, mean = the row mean, rstd = 1 / sqrt(biased two-pass variance + eps), every operation in fp32 in the
 * order of sdvar_op_ln_modulate's row kernel (its lane map for C % 8 != 0). */
int sdvar_op_adaln_fwd(const float* x, const void* scale, int32_t scale_dtype, int64_t scale_batch_stride, const void* shift, int32_t shift_dtype, int64_t shift_batch_stride,
                       float* out, int32_t B, int32_t L, int32_t C, double eps, void* stream);
/* Bytes of the workspace of sdvar_op_adaln_bwd: B * ceil(L / 32) * 2 * C floats (32 = rows of one image per workgroup, a compile-time constant); -1 on a bad shape.  Host only. */
int64_t sdvar_op_adaln_bwd_ws_bytes(int32_t B, int32_t L, int32_t C);
/* The backward of sdvar_op_adaln_fwd for the upstream gradient g.  mean and rstd are recomputed from x with the forward's code (the same bits).  With a = g (1 + scale) and
 * xhat = (x - mean) rstd:
 *     dx = rstd (a - mean_c(a) - xhat mean_c(a xhat));   dscale[b, c] = sum_l g xhat;   dshift[b, c] = sum_l g
 * dx (B, L, C) fp32, dscale (dscale_rows, C) dense in scale_dtype, dshift (dshift_rows, C) dense in shift_dtype; *_rows is B, or 1 to sum over the images as well.  Each of the
 * three may be NULL: it is then not stored (at least one must be given).  The sums are fp32 in a fixed order that depends on (B, L, C) alone - per workgroup of 32 rows of one
 * image: rows w, w + 4, ... per wave, the waves in order; then the partial rows s, s + 4, ... per slice in index order, the 4 slices in order - and are rounded once to the
 * operand's dtype (an fp16 overflow is inf).  ws: the workspace above, needed for dscale / dshift. */
int sdvar_op_adaln_bwd(const float* x, const void* scale, int32_t scale_dtype, int64_t scale_batch_stride, const float* g, float* dx, void* dscale, int32_t dscale_rows,
                       void* dshift, int32_t shift_dtype, int32_t dshift_rows, float* ws /*workspace*/, int32_t B, int32_t L, int32_t C, double eps, void* stream);
/* out = x + (y * gamma) * row_scale[b]  (row_scale NULL: x + y * gamma).  y (B, L, C) dense in y_dtype (0 fp32, 1 fp16, 2 bf16), 16-byte aligned, widened to fp32; row_scale
 * (B) fp32 or NULL: DropPath's per-image factor.  The products and the sum are fp32 operations in this order. */
int sdvar_op_gate_add_fwd(const float* x, const void* y, int32_t y_dtype, const void* gamma, int32_t gamma_dtype, int64_t gamma_batch_stride, const float* row_scale, float* out,
                          int32_t B, int32_t L, int32_t C, void* stream);
/* Bytes of the workspace of sdvar_op_gate_add_bwd: B * ceil(L / 32) * C floats; -1 on a bad shape.  Host only. */
int64_t sdvar_op_gate_add_bwd_ws_bytes(int32_t B, int32_t L, int32_t C);
/* The backward of sdvar_op_gate_add_fwd (the gradient of x is g itself): dy = (g * gamma) * row_scale[b], (B, L, C) dense in y_dtype; dgamma[b, c] = sum_l row_scale[b] g y,
 * (dgamma_rows, C) dense in gamma_dtype, dgamma_rows = B, or 1 to sum over the images as well; row_scale[b] multiplies each 32-row partial sum, the order of the sums is
 * sdvar_op_adaln_bwd's.  dy or dgamma may be NULL (not stored; y is then not read for a NULL dgamma). */
int sdvar_op_gate_add_bwd(const float* g, const void* y, int32_t y_dtype, const void* gamma, int32_t gamma_dtype, int64_t gamma_batch_stride, const float* row_scale, void* dy,
                          void* dgamma, int32_t dgamma_rows, float* ws /*workspace*/, int32_t B, int32_t L, int32_t C, void* stream);

/* ---- attn_l2_norm's QK normalisation between the QKV GEMM and the attention call under autograd (SelfAttention.forward, basic_var.py:93-105) ---------------------------
 * csrc/qknorm_train.hip.  Added without an ABI bump (purely additive).  Common to the three entry points:
 *   - qkv and dqkv are (B, L, 3, H, 64), dense, 16-byte aligned, dtype code 0 fp32, 1 fp16, 2 bf16 (widened to fp32 before any arithmetic); the head dimension is 64,
 *     1 <= H <= 48, B, L >= 1, B * L <= 2^29.  One wave64 per row (b, l); a lane holds 4 consecutive channels, a head is 16 consecutive lanes, a step covers 4 heads
 *     (H need not be a multiple of 4).
 *   - q_bias, v_bias (C = 64 H, fp32, 16-byte aligned, each may be NULL) are added in fp32; scale_log (H) fp32 is the raw per-head parameter:
 *     s_h = expf(min(scale_log[h], max_log)).
 *   - the sum of squares of a head: the lane's four products added left to right, then four cross-lane levels (xor 8, 4, 2, 1) inside the 16 lanes.  The backward
 *     recomputes the forward's norms bit for bit.
 *   - argument errors (shape, NULL, dtype code, alignment, strides) are reported before any launch; no allocation, no host synchronisation, no atomics: repeats are
 *     bit-identical.  Nothing is clamped.
 * sdvar_op_qknorm_fwd: q = (xq / max(|xq|, 1e-12)) * s_h with xq = qkv[.., 0, ..] + q_bias, k = xk / max(|xk|, 1e-12); q and k are dense (B, L, H, 64) fp32.  With a v_bias
 * (and only then; v is NULL exactly when v_bias is) v = qkv[.., 2, ..] + v_bias, dense (B, L, H, 64) in dtype, rounded once.  A head with a norm below 1e-12 gives
 * x / 1e-12: a zero head gives exact zeros. */
int sdvar_op_qknorm_fwd(const void* qkv, int32_t dtype, const float* q_bias, const float* v_bias, const float* scale_log, double max_log, float* q, float* k, void* v,
                        int32_t B, int32_t L, int32_t H, void* stream);
/* Bytes of the workspace of sdvar_op_qknorm_bwd: B * ceil(L / 32) * 3 * 64 H floats (32 = rows of one image per workgroup, a compile-time constant); -1 on a bad shape.
 * Host only. */
int64_t sdvar_op_qknorm_bwd_ws_bytes(int32_t B, int32_t L, int32_t H);
/* The backward of sdvar_op_qknorm_fwd for the upstream gradients dq, dk (fp32) and dv (in dtype), each read through grad_strides = {dq: b, h, l; dk: b, h, l; dv: b, h, l}
 * in ELEMENTS (non-negative multiples of 4; unit channel stride; base aligned to 4 elements); each of the three may be NULL: zero, not read.  v_bias does not enter.
 * With n = max(|x|, eps), xh = x / n:   |x| >= eps: dx = (s / n) (g - xh (xh . g)),  else dx = (s g) / eps   (k: s = 1).
 *   dqkv = [dx_q, dx_k, dv] in dtype, all three slots written by the one kernel (an fp16 overflow is +-inf);
 *   dscale_log[h] = [scale_log[h] <= max_log] sum_{b, l, c in h} dq q;   dq_bias[c] = sum_{b, l} dx_q;   dv_bias[c] = sum_{b, l} dv     - fp32, (H), (C), (C).
 * Each of the four outputs may be NULL: it is then not computed and the inputs only it needs are not read (at least one must be given).  The sums are fp32 in a fixed order
 * that depends on (B, L, H) alone - sdvar_op_adaln_bwd's: per workgroup of 32 rows of one image rows w, w + 4, ... per wave, the waves in order; then the partial rows
 * s, s + 4, ... of all images per slice in index order, the 4 slices in order; a head's 64 column sums by six wave levels.  ws: the workspace above, needed for the sums. */
int sdvar_op_qknorm_bwd(const void* qkv, int32_t dtype, const float* q_bias, const float* scale_log, double max_log, const float* dq, const float* dk, const void* dv,
                        const int64_t* grad_strides, void* dqkv, float* dscale_log, float* dq_bias, float* dv_bias, float* ws /*workspace*/, int32_t B, int32_t L, int32_t H,
                        void* stream);

/* ---- the conditioning linears under autograd: ada_lin = Sequential(SiLU, Linear(D, 6C)) of a block (basic_var.py:147, 156) and Sequential(SiLU, Linear(D, 2C)) of the
 * head norm (:170, 173); sdvar_amd/seam.py ada_lin ------------------------------------------------------------------------------------------------------------------
 * csrc/cond_train.hip.  Added without an ABI bump (purely additive).  A skinny product: M = the batch, all the bytes are in W.  No matrix cores, no operand planes, no
 * cache: W is streamed once per direction and the SiLU is folded into the read of c.  Common to the entry points:
 *   - c is (M, K) with leading dimension ldc ELEMENTS (ldc >= K, a multiple of 4 for fp32 and of 8 for half), c_dtype 0 fp32, 1 fp16, 2 bf16; w is (N, K) dense, w_dtype
 *     0 fp32 or the half code; `dtype` is the ARITHMETIC code.  0: c and w fp32, true fp32 - every product enters the sum by one fp32 fmaf, in a fixed order.  1 / 2
 *     (autocast's contract): c and w each fp32 or that half dtype; s is rounded once to the half dtype, an fp32 w is rounded to it as it is read (nearest even, the bits
 *     of .to(dtype)), the sums are fp32, results are rounded once to half and an overflow is +-inf.
 *   - s = silu(c) = x / (1 + expf(-x)) on the widened fp32 value (libm's expf, a correctly rounded division), the same code - the same bits - in both directions: -0
 *     where expf overflows (x < -88.7), x where it underflows.
 *   - 1 <= M <= 64, K % 8 == 0 with 8 <= K <= 4096, N % 8 == 0 with N >= 8, N * K < 2^31; every pointer 16-byte aligned.  Argument errors (shape, NULL, dtype codes,
 *     alignment) are reported before any launch.  No allocation, no host synchronisation, no atomics: repeats are bit-identical.  Nothing is clamped.
 * sdvar_op_cond_lin_fwd: y[m, n] = sum_k s[m, k] w[n, k] + b[n]; b fp32 (N) or NULL (nothing added); y (M, N) dense, fp32 for dtype 0, else half.  The sum over k of one
 * output: lane l of a wave adds k = 4 l + 256 j + e in the order j = 0, 1, .., e = 0 .. 3, then six butterfly levels (xor 32, 16, .., 1) add the 64 lanes; the fp32 bias is
 * added to that fp32 sum.  The order depends on K alone: a row's output bits do not depend on M, on N or on the other rows.  Up to 16 rows of c, W
 * is read once.  Rows 16 .. 63 are further passes of 16 rows over the 16 rows of W a workgroup owns and has just read; that those reads are served by a cache and not by
 * memory is assumed, not measured. */
int sdvar_op_cond_lin_fwd(const void* c, int32_t c_dtype, int64_t ldc, const void* w, int32_t w_dtype, const float* b, void* y, int32_t dtype, int32_t M, int32_t N, int32_t K,
                          void* stream);
/* Bytes of the workspace of sdvar_op_cond_lin_bwd: ceil(N / 64) * M * K floats (64 = rows of W per workgroup, a compile-time constant); -1 on a bad shape.  Host only. */
int64_t sdvar_op_cond_lin_bwd_ws_bytes(int32_t M, int32_t N, int32_t K);
/* The backward of sdvar_op_cond_lin_fwd for the upstream gradient dy (M, N) dense, fp32 for dtype 0 and the half dtype otherwise.  Each output may be NULL (not computed),
 * not all three:
 *   dW[n, k] = sum_m dy[m, n] s[m, k]     m ascending, fp32; s as the forward has it (rounded in the half modes); (N, K) dense in w's own dtype: unrounded fp32 for fp32
 *                                         master weights.
 *   db[n]    = sum_m dy[m, n]             m ascending, fp32 (N).
 *   dc[m, k] = (sum_n dy[m, n] w[n, k]) silu'(c[m, k])      w rounded as in the forward; (M, K) dense in c's dtype, rounded once.  The sum over n is fp32 in a fixed
 *              order that depends on N alone: inside a workgroup's slab of 64 rows of W, wave v adds its rows 4 (v + 4 i) + r in the order i = 0 .. 3, r = 0 .. 3, the four
 *              waves are added as ((v0 + v1) + v2) + v3 and the partial row goes to the workspace [slab][m][k]; a second kernel adds the slabs (slice t of 4: slabs t, t + 4,
 *              .. in index order; the slices as ((t0 + t1) + t2) + t3), multiplies by silu'(x) = sg (1 + x (1 - sg)), sg = 1 / (1 + expf(-x)) - finite for every finite x, tending to 0 and 1 - and rounds.  The sum is NOT rounded to half
 *              before the derivative (torch's autocast rounds dy W to half first): this side is the more accurate one.
 * An output asked for alone has the bits it has in the full run.  W is read only when dc is asked for - once for M <= 32, once per 32 rows beyond (dc's partial sums
 * then come from one launch per 32 rows, dW and db from a launch of their own); dW is written once.  ws: the workspace above, needed
 * for dc only. */
int sdvar_op_cond_lin_bwd(const void* dy, const void* c, int32_t c_dtype, int64_t ldc, const void* w, int32_t w_dtype, void* dc, void* dW, float* db, float* ws /*workspace*/,
                          int32_t dtype, int32_t M, int32_t N, int32_t K, void* stream);

/* ---- the teacher-forcing input embedding under autograd (the prologue of VAR.forward, var.py:225-243) ----------------------------------------------------------------
 * csrc/embed_train.hip; sdvar_amd/seam.py teacher_embed.  Added without an ABI bump (purely additive).  Plain fp32 vector code: no matrix cores, no operand planes, no
 * atomics.  S stages, lvl[l] the stage of token l; L tokens, T of them used; first_l = patch_nums[0]^2; K = Cvae; NC1 = num_classes + 1 rows of class_emb.
 *   - label (B) int32 (label_i64 = 0) or int64 (1); r (B) fp32 or NULL; lvl (L) int64; xv fp32 with dense rows of K values at a batch stride and a row stride in elements
 *     (multiples of 4, row stride >= K), NULL allowed when T == first_l; class_emb (NC1, C), pos_start (first_l, C), w (C, K), bias (C), lvl_emb (S, C), pos_1LC (L, C):
 *     dense fp32.
 *   - C % 4 == 0 with 4 <= C <= 3072; K % 4 == 0 with 4 <= K <= 64; B >= 1, B * T <= 2^29; 1 <= first_l <= T <= L <= 2^19; every pointer 16-byte aligned.  Argument errors
 *     are reported before any launch.  No allocation, no host synchronisation: repeats are bit-identical.  Nothing is clamped.
 *   - j_b, the effective label of image b: (r != NULL && r[b] < (float)rate) ? NC1 - 1 : label[b], a float32 comparison.  A label outside [0, NC1) and a level lvl[l]
 *     outside [0, S) are never used as an index: cond[b] and the rows l < first_l of such an image, and all B rows of such a token, are written as quiet NaN; in the
 *     backward such an image adds nothing to dclass and such a token nothing to dlvl (the other gradients are the plain sums below over whatever g holds).
 * sdvar_op_embed_fwd writes x (B, T, C) - fp32 for x_dtype 0, fp16 / bf16 for 1 / 2, rounded once (nearest even) from the fp32 value - and cond (B, C) fp32:
 *     e[l, c]    = lvl_emb[lvl[l], c] + pos_1LC[l, c]
 *     l <  first_l:  x[b, l, c] = (class_emb[j_b, c] + pos_start[l, c]) + e[l, c]
 *     l >= first_l:  a = 0; for k = 0 .. K - 1: a = fmaf(xv[b, l - first_l, k], w[c, k], a);   x[b, l, c] = (a + bias[c]) + e[l, c]
 *     cond[b, c] = class_emb[j_b, c]
 * One launch.  The order of a sum depends on K alone: a row's bits do not depend on B or on the other rows. */
int sdvar_op_embed_fwd(const void* label, int32_t label_i64, const float* r, double rate, const int64_t* lvl, const float* xv, int64_t xv_batch_stride, int64_t xv_row_stride,
                       const float* class_emb, const float* pos_start, const float* w, const float* bias, const float* lvl_emb, const float* pos_1LC, void* x, int32_t x_dtype,
                       float* cond, int32_t B, int32_t T, int32_t L, int32_t first_l, int32_t C, int32_t K, int32_t S, int32_t NC1, void* stream);
/* Bytes of the workspace of sdvar_op_embed_bwd: (T * C + ceil(T / 8) * C * K) floats (8 = tokens per workgroup, a compile-time constant); -1 on a bad shape.  Host only. */
int64_t sdvar_op_embed_bwd_ws_bytes(int32_t B, int32_t T, int32_t C, int32_t K);
/* The backward of sdvar_op_embed_fwd for the upstream gradients g (B, T, C) of x, dense in x's dtype (g_dtype) and widened to fp32 as it is read, and gc (B, C) fp32 of
 * cond; either may be NULL (no gradient reached that output).  label, r, rate, lvl, xv, w: the forward's, so that j_b is recomputed with the forward's code.  Each output
 * may be NULL (not computed), not all of them; all are dense fp32:
 *   dpos_1LC[l, c]   = p[l, c] = sum_b g[b, l, c]            b ascending from 0.0f, for l < T; exactly 0 for T <= l < L                      (L, C)
 *   dpos_start[l, c] = p[l, c]                                for l < first_l                                                                  (first_l, C)
 *   dlvl[s, c]       = sum of p[l, c] over l < T with lvl[l] = s: slice t of 4 adds the qualifying tokens among t, t + 4, .. in index order from 0.0f, the slices are added as
 *                      ((t0 + t1) + t2) + t3; exactly 0 for a stage no token reaches                                                          (S, C)
 *   dbias[c]         = sum of p[l, c] over first_l <= l < T, in dlvl's order                                                                  (C)
 *   dclass[j, c]     = sum over the images with j_b = j, b ascending from 0.0f, of (gc[b, c] + t_b[c]), t_b[c] = sum_{l < first_l} g[b, l, c] with l ascending from 0.0f
 *                      (gc NULL: t_b; g NULL: gc[b, c]); rows no image selects are 0; every row is written                                    (NC1, C)
 *   dW[c, k]         = sum_b sum_{l >= first_l} g[b, l, c] xv[b, l - first_l, k], one fmaf per term: a workgroup owns the 8 tokens 8 i .. 8 i + 7, its wave v adds tokens
 *                      8 i + v and 8 i + v + 4 in that order, b ascending inside a token; the four waves are added as ((v0 + v1) + v2) + v3 into the workspace; a second kernel
 *                      adds the workgroups' partial matrices (slice t of 4: workgroups t, t + 4, .. in index order; the slices as ((t0 + t1) + t2) + t3)   (C, K)
 *   dxv[b, t, k]     = sum_c g[b, t + first_l, c] w[c, k] for t < T - first_l, exactly 0 for the other rows: lane n of a wave adds c = 4 n + 256 i + e in the order i = 0, 1,
 *                      .., e = 0 .. 3 with one fmaf per term, then six butterfly levels (xor 32, 16, .., 1) add the lanes                     (B, xv_rows, K), xv_rows >= T - first_l
 * Every order depends on (B, T, first_l, C, K) and lvl alone.  An output asked for alone has the bits it has in the full run.  With T == first_l, dW and dbias are exact
 * zeros; with g == NULL everything but dclass is.  An fp16 g arrives as it is: an inf propagates.  ws: the workspace above (needed with g for everything but dclass and
 * dxv).  One launch over g, plus one each for dW, for dlvl / dbias, for dclass and for dxv. */
int sdvar_op_embed_bwd(const void* g, int32_t g_dtype, const float* gc, const void* label, int32_t label_i64, const float* r, double rate, const int64_t* lvl, const float* xv,
                       int64_t xv_batch_stride, int64_t xv_row_stride, const float* w, float* dpos_1LC, float* dpos_start, float* dlvl, float* dclass, float* dbias, float* dW,
                       float* dxv, int32_t xv_rows, float* ws /*workspace*/, int32_t B, int32_t T, int32_t L, int32_t first_l, int32_t C, int32_t K, int32_t S, int32_t NC1,
                       void* stream);

/* ---- the optimizer step of the reference's trainer (AmpOptimizer.backward_clip_step, utils/amp_sc.py:39-75: unscale_, clip_grad_norm_, AdamW.step) -------------------
 * csrc/optim.hip; sdvar_amd/seam.py AdamW.  Added without an ABI bump (purely additive).  Two calls over a HOST list of n tensor descriptors: float32 param, grad,
 * exp_avg, exp_avg_sq (device, 4-byte aligned, numel elements each, dense), the tensor's float32 `step` counter (device) and its lr and weight_decay.  The descriptors
 * are copied into the kernel arguments of each launch (SDVAR_OPTIM_TENSORS_PER_LAUNCH per launch, as many launches as needed): the list may be freed or rewritten as soon
 * as a call returns, and calls enqueued back to back never share descriptor memory.  A workgroup handles one chunk of SDVAR_OPTIM_CHUNK elements of one tensor.
 * ws (device, 8-byte aligned): 16 + 8 n + 8 sum_t ceil(numel_t / SDVAR_OPTIM_CHUNK) bytes = {record: 4 floats; 2 floats per tensor; one double per workgroup}; hand the
 * SAME ws and list to both calls.  record = {norm, coef, skip, gscale}.  Argument errors (NULL list, n < 1, a NULL or misaligned pointer in a descriptor, numel < 0,
 * beta outside [0, 1), a negative or NaN eps / lr / weight_decay, a NaN max_norm, a ws that is too small) are reported before any GPU call.  No allocation, no host
 * synchronisation, no atomics: repeats are bit-identical.  The gradients are only read. */
#define SDVAR_OPTIM_CHUNK 32768
#define SDVAR_OPTIM_TENSORS_PER_LAUNCH 48
typedef struct sdvar_optim_tensor {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    float* step;
    int64_t numel;
    double lr;
    double weight_decay;
} sdvar_optim_tensor_t;
/* Pass 1 (reads the gradients once): S = sum of g^2 over all tensors, each square and every sum in float64 (a float32 square is exact there and the sum can neither
 * overflow nor underflow: S is non-finite exactly when an element is) - per lane, six wave levels, the four waves of a workgroup in order, then ONE workgroup adds the
 * per-workgroup partials in a fixed order (thread t: partials t, t + 256, ...; then a fixed tree).  With inv_scale = float(1 / double(*grad_scale)) (grad_scale NULL: 1):
 *     norm = float(sqrt(S) * inv_scale);   coef = max_norm <= 0 ? 1 : min(1, float(max_norm) / (norm + 1e-6f))       (clip_grad_norm_'s definition, float32)
 *     skip = 1 when norm is not finite or *found_inf > 0 (found_inf may be NULL), else 0;   gscale = inv_scale * coef
 * The same finalising launches advance every tensor's step by 1 - skip (a skipped step keeps its bits; numel == 0: untouched) and leave per tensor, computed in float64
 * from the advanced step: float(lr / (1 - beta1^step)) and float(sqrt(1 - beta2^step)). */
int sdvar_optim_grad_stats(const sdvar_optim_tensor_t* tensors /*host*/, int32_t n, const float* grad_scale, const float* found_inf, double max_norm, double beta1,
                           double beta2, void* ws, uint64_t ws_bytes, void* stream);
/* Pass 2, after pass 1 on the same stream with the same list and ws: torch's decoupled AdamW (no amsgrad, no maximize) with one read of g, p, m, v and one write of p, m, v,
 * 16-byte accesses where all four pointers of a tensor are 16-byte aligned (scalar otherwise, and for the numel % 4 tail).  Each line is one float32 operation, in this
 * order (-ffp-contract=off), with ss and rb the two per-tensor floats of pass 1:
 *     g' = g * gscale;   p1 = p * float(1 - lr * weight_decay);   m' = float(beta1) * m + float(1 - beta1) * g';   v' = float(beta2) * v + (float(1 - beta2) * g') * g'
 *     p' = p1 - ss * (m' / (sqrt(v') / rb + float(eps)))                  (division and square root correctly rounded)
 * record.skip != 0: nothing is written, p, m and v keep their bits. */
int sdvar_optim_adamw_step(const sdvar_optim_tensor_t* tensors /*host*/, int32_t n, double beta1, double beta2, double eps, void* ws, uint64_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SDVAR_HIP_H */
