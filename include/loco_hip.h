/*
 * loco_hip.h -- C ABI of libloco_hip.so, the MI355X (gfx950) engine behind the
 * LOCO-Edit null-space-projection hot path.
 *
 * The reference (ChicyChen/LOCO-Edit) has no FFI layer: its boundary is Python
 * duck typing.  Each entry point below names the
 * reference interface it replaces; the Python host (loco-edit_amd/) binds them
 * with ctypes (INTEGRATION.md shows the stub).
 *
 * Conventions: every tensor pointer is a DEVICE pointer owned by the caller
 * (torch `tensor.data_ptr()`), fp32, contiguous NCHW unless stated.  The ctx
 * owns only its parameter copies, workspace and activation caches.  All work is
 * enqueued on the caller-supplied hipStream_t (passed as void*).  Return 0 on
 * success, negative on error (message via loco_last_error).  One ctx per
 * (process, GPU); not thread-safe.  No exceptions cross the ABI.
 */
#ifndef LOCO_HIP_H
#define LOCO_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct loco_ctx loco_ctx;

/* Architecture of the denoiser: reference src/configs/custom_celeba_ddpm.yml
 * `model:` block + DDPM.__init__ (src/models/ddpm/diffusion.py:22-126). */
typedef struct loco_unet_cfg {
    int32_t struct_size;       /* = sizeof(loco_unet_cfg) of the header the caller was built against; loco_create
                                  refuses a mismatch instead of reading past an older binding's struct */
    int32_t resolution;        /* data.image_size */
    int32_t in_channels;       /* model.in_channels */
    int32_t out_ch;            /* model.out_ch */
    int32_t ch;                /* model.ch */
    int32_t num_levels;        /* len(model.ch_mult) */
    int32_t ch_mult[8];        /* model.ch_mult */
    int32_t num_res_blocks;    /* model.num_res_blocks */
    int32_t num_attn_res;      /* len(model.attn_resolutions) */
    int32_t attn_resolutions[8];
    int32_t gn_groups;         /* 32  (diffusion.py:810) */
    float   gn_eps;            /* 1e-6 */
    int32_t max_batch;         /* largest image / probe batch one call may carry */
    /* 0: Ho-DDPM U-Net (models/ddpm/diffusion.py); 1: guided-diffusion / P2 U-Net
     * (models/guided_diffusion/unet.py:398-684 with P2_DICT, script_util.py:166-190:
     * scale-shift norm, ResBlock up/down, legacy multi-head attention, [cos,sin] embedding);
     * 2: latent decoder -- the network behind `self.vae.decode(z).sample` of the Stable Diffusion path
     * (src/modules/edit.py:750, 770-771; diffusers AutoencoderKL decoder, un-vendored): conv_in, mid block/attn/block,
     * up levels of num_res_blocks+1 ResnetBlocks + nearest-x2 conv, norm_out/SiLU/conv_out; no skips, no time
     * embedding.  `resolution` is the latent resolution, the output is [out_ch, resolution << (num_levels-1), same];
     * loco_unet_forward ignores t; loco_pmp_primal needs use_et = 1 (raw network Jacobian, mask on the OUTPUT) and
     * loco_pmp_jvp / _vjp then map [k, in] -> [k, out] / [k, out] -> [k, in]; loco_ddim_step is refused;
     * 3: latent encoder -- the network behind `self.vae.encode(x0).latent_dist` of the latent inversion
     * (src/modules/edit.py:594-597): conv_in, down levels of num_res_blocks ResnetBlocks + pad (0,1,0,1) conv stride 2,
     * mid block/attn/block, norm_out/SiLU/conv_out, 1x1 quant_conv.  `resolution` is the IMAGE resolution, the output is
     * the posterior's moments [out_ch = 2 z, resolution >> (num_levels-1), same]; used through loco_unet_forward (t ignored) */
    int32_t arch;
    int32_t num_head_channels; /* arch 1: channels per attention head (P2: 64) */
    int32_t learn_sigma;       /* arch 1: the head emits 2*out_ch channels, eps = first out_ch (unet.py:680-684) */
    /* arch 1, text-to-image stand-ins: when context_dim > 0 every attention block is followed by a text
     * cross-attention stage  h += proj(softmax(q(GN(h))^T k(ctx) / sqrt(d)) applied to v(ctx))  over the
     * context_len x context_dim encoder states given to loco_set_context (the role of encoder_hidden_states in
     * edit.py:636-674 / 1286-1373; the reference's cross-attention lives in un-vendored diffusers blocks) */
    int32_t context_dim;
    int32_t context_len;
    /* arch 1 variants of the same guided-diffusion skeleton (unet.py constructor switches).  The latent-diffusion /
     * Stable Diffusion v1 denoiser is arch 1 with scale_shift_norm = 0, resblock_updown = 0, num_heads = 8,
     * transformer_depth = 1, context_dim = 768 (859 520 964 parameters at 320 x (1,2,4,4)):
     *   scale_shift_norm  1: GN(h) * (1 + scale) + shift (unet.py:250-254, P2)   0: GN(h + emb_out) (unet.py:255-257)
     *   resblock_updown   1: ResBlock(up/down=True) between levels (P2)            0: Downsample / Upsample with a 3x3 conv
     *                        (stride 2 padding 1 / nearest x2 + conv; unet.py:83-142)
     *   num_heads         > 0: that many heads in every attention (head width = C / num_heads); else num_head_channels
     *   transformer_depth 0: AttentionBlock (unet.py:261-307) [+ the cross-attention stage when context_dim > 0]
     *                     1: SpatialTransformer of latent-diffusion (GroupNorm eps 1e-6 -> 1x1 proj_in -> LayerNorm ->
     *                        self-attention, LayerNorm -> cross-attention over the loco_set_context states, LayerNorm ->
     *                        GEGLU feed-forward, residuals -> 1x1 proj_out -> + input); needs context_dim > 0 */
    int32_t scale_shift_norm;
    int32_t resblock_updown;
    int32_t num_heads;
    int32_t transformer_depth;
    /* arch 1, the DeepFloyd-IF stage-I denoiser (`self.unet = self.stage_1.unet`, src/modules/edit.py:1213-1222: diffusers
     * UNet2DConditionModel with ResnetDownsampleBlock2D / SimpleCrossAttn*Block2D, un-vendored; the same tree as the
     * UNetModel of the deepfloyd_if package) = the guided-diffusion skeleton with scale-shift norm and ResBlock resampling plus:
     *   act        0: SiLU   1: exact (erf) GELU in every norm -> activation -> conv chain and in the time embedding
     *                 (`act_fn = "gelu"`; the per-block embedding projections read act(emb) once: `resnet_skip_time_act`)
     *   res_scale  ResBlock output = (shortcut + h) * res_scale (`resnet_out_scale_factor` = sqrt 2 -> 0.70710678);
     *                 0 reads as 1
     *   added_kv   1: every AttentionBlock attends over [text ; image] keys / values in ONE softmax
     *                 (`AttnAddedKVProcessor`: key = cat([add_k_proj(GN(ctx)), to_k(h)])): the context_len x context_dim
     *                 states of loco_set_context (after the host's `encoder_hid_proj`) go through the block's own
     *                 GroupNorm (`norm_encoder`) and `encoder_kv` projection; needs context_dim > 0, transformer_depth = 0 */
    int32_t act;
    float   res_scale;
    int32_t added_kv;
    /* arch 1, latent-consistency distilled denoisers (diffusers UNet2DConditionModel `time_cond_proj_dim`; LCM_Dreamshaper_v7:
     * 256): P > 0 adds the parameter `time_embed.cond_proj.weight` [ch][P] (no bias) and the call loco_set_time_cond, whose
     * result is added to the sinusoid before the first dense layer of the time embedding
     * (`t_emb + cond_proj(timestep_cond)` ahead of `linear_1`).  0: neither exists. */
    int32_t time_cond_proj_dim;
} loco_unet_cfg;

/* Library / device probes (no ctx). */
const char* loco_version(void);
int  loco_device_count(void);

/* Replaces PullBackDDPM(args) construction (diffusion.py:128-143). */
int  loco_create(const loco_unet_cfg* cfg, loco_ctx** out);
void loco_destroy(loco_ctx* ctx);
/* A second context on the SAME parameters (round 6): the reference runs all classifier-free-guidance branches through ONE
 * U-Net object -- one set of weights (src/modules/edit.py:1319-1322, :655-667).  The fork shares the device copies of the
 * parent's parameters in every layout and owns only its activation arenas (max_batch samples; <= 0: the parent's), statistics,
 * scratch and per-prompt constants (loco_set_context / loco_set_cond); results are bit-identical to an independent context
 * loaded with the same state_dict.  The parent must have all parameters loaded; it may be destroyed first (its parameters are
 * freed with the last fork). */
int  loco_fork(loco_ctx* parent, int32_t max_batch, loco_ctx** out);
const char* loco_last_error(loco_ctx* ctx);

/* Replaces model.load_state_dict (src/utils/utils.py:102-105): one call per
 * state_dict entry, names exactly as in the reference module tree.  `data` is a
 * host OR device pointer to fp32 values (is_device says which). */
int  loco_load_param(loco_ctx* ctx, const char* name, const void* data,
                     const int64_t* shape, int32_t ndim, int32_t is_device);
/* 0 when every parameter of the architecture has been loaded, else the count
 * still missing (first missing name in loco_last_error). */
int  loco_params_missing(loco_ctx* ctx);

/* eps = unet(x, t): PullBackDDPM.forward (diffusion.py:145-200) as called at
 * edit.py:2151, 2375, 2572.  x, eps: [B,C,H,W].  t is the float timestep fed
 * to the time embedding. */
int  loco_unet_forward(loco_ctx* ctx, const float* x, float t, int32_t B,
                       float* eps, void* stream);

/* One DDIM update fused with the denoiser call: scheduler.step
 * (src/utils/utils.py:342-383) after unet(xt,t), the body of HOT LOOPs A/A'/C
 * (edit.py:2146-2160, 2568-2584).  at/at_next are alpha-bar at floor(t),
 * floor(t_next) (utils.py:444-461).  eta==0: deterministic; eta!=0 needs
 * `noise` [B,C,H,W] (the randn_like draw of utils.py:374).  x_next may alias x. */
int  loco_ddim_step(loco_ctx* ctx, const float* x, float t, float at, float at_next,
                    float eta, const float* noise, int32_t B, float* x_next, void* stream);

/* The scheduler update alone, for callers that hold eps already (seam 3 of
 * scheduler.step(et, t, xt, eta).prev_sample / .x0, utils.py:342-383).
 * x0_out (optional) receives P_xt = (xt - et*sqrt(1-at))/sqrt(at). */
int  loco_sched_step(loco_ctx* ctx, const float* x, const float* et, float at, float at_next,
                     float eta, const float* noise, int64_t count, float* x_next, float* x0_out,
                     void* stream);

/* The eta = 0 scheduler update with two network outputs (Asyrp's asymmetric step, asyrp.py): the x0 estimate from et_edit,
 * the direction term from et_src,
 *     x0 = (x - sqrt(1 - at) et_edit) / sqrt(at),   x_next = sqrt(at_next) x0 + sqrt(1 - at_next) et_src.
 * One launch; with et_edit == et_src bit-identical to loco_sched_step(eta = 0).  x0_out (optional) receives x0. */
int  loco_sched_step_asym(loco_ctx* ctx, const float* x, const float* et_edit, const float* et_src, float at, float at_next,
                          int64_t count, float* x_next, float* x0_out, void* stream);

/* --- PMP-Jacobian operator J = d x0_hat[mask] / d x_t  (edit.py:2369-2391) ---
 * loco_pmp_primal evaluates the denoiser once at (x,t), caching what the
 * tangent and cotangent passes need; `mask` is uint8 [C*H*W] (nullptr = all
 * ones), use_et!=0 selects get_et (edit.py:2394-2403) instead of get_x0. */
int  loco_pmp_primal(loco_ctx* ctx, const float* x, float t, float at,
                     const uint8_t* mask, int32_t use_et, void* stream);
/* Two subspace solves on the same (x, t) with different masks -- the modify-space solve on `mask` and the null-space
 * solve on `~mask` of run_edit_null_space_projection (edit.py:2290-2310) -- can share one probe batch: after
 * loco_pmp_primal(mask), rows >= from_row of every later loco_pmp_jvp / loco_pmp_vjp call use `mask2` (device, [n])
 * instead.  The Jacobian products of the rows are independent, so each solve's iterates are what it would compute
 * alone; the wider batch fills the deep levels of the network better (5 + 5 probes: 14 % less time per probe).
 * mask2 == NULL switches it off; the next loco_pmp_primal also does.  loco_mask_count / loco_mask_gather keep
 * referring to the first mask. */
int  loco_pmp_set_second_mask(loco_ctx* ctx, const uint8_t* mask2, int32_t from_row, void* stream);
/* U = J V  (replaces torch.func.jacfwd at edit.py:2451-2455).  V: [k, n];
 * U: dense [k, n] with zeros outside the mask. */
int  loco_pmp_jvp(loco_ctx* ctx, const float* V, int32_t k, float* U, void* stream);
/* A = U^T J (replaces torch.autograd.functional.jacobian at edit.py:2460-2480).
 * U: dense [k, n] (entries outside the mask are ignored); A: [k, n]. */
int  loco_pmp_vjp(loco_ctx* ctx, const float* U, int32_t k, float* A, void* stream);
/* loco_pmp_vjp plus the gradient with respect to the states given to loco_set_context:
 * G[p] = U[p]^T d f / d tokens, f = the function the last loco_pmp_primal selected (x0_hat[mask] or eps[mask]).
 * A [k, n] may be NULL; G is [k, context_len, context_dim].  A is what loco_pmp_vjp writes, to the bit; a row of G does not
 * depend on k or on the row's position: the rows of G are taken from one single-probe cotangent pass each (the batched pass
 * plans its convolutions by k), so k > 1 costs k such passes on top of loco_pmp_vjp's, k = 1 is one pass for A and G, and
 * without A a pass stops behind the first op that reads the states.  The x_t term of x0_hat does not depend on the states,
 * so G = c_e . U^T d eps / d tokens.
 * Refused (-2, text in loco_last_error): context_dim == 0; no valid primal (loco_set_context invalidates it); a primal of an
 * h-space tap (loco_pmp_primal_tap, tap 1 / 2); cfg.added_kv; G == NULL. */
int  loco_pmp_vjp_context(loco_ctx* ctx, const float* U, int32_t k, float* A, float* G, void* stream);

/* --- h-space tap: the U-Net bottleneck h of a denoiser (arch 0 / 1) ---
 * h is the output of the middle block's last op, PullBackDDPM.get_h(x, t, op='mid', block_idx=0)
 * (models/ddpm/diffusion.py:203-260); n_h = C*H*W.  The latent decoder and encoder (arch 2 / 3) have no tap: every
 * entry below refuses them (-2, text in loco_last_error).  Eager launches only: no captured-graph variant. */
int  loco_h_dims(loco_ctx* ctx, int32_t* C, int32_t* H, int32_t* W);
/* h_out [B, n_h] = get_h(x, t): the ops up to the tap only.  Invalidates the cached primal, like loco_unet_forward. */
int  loco_unet_get_h(loco_ctx* ctx, const float* x, float t, int32_t B, float* h_out, void* stream);
/* eps = PullBackDDPM.forward(x, t, u=dh, op='mid', block_idx=0) (diffusion.py:145-200): h[b] += dh[b] between the tap
 * op and the op behind it; everything behind the tap sees the shifted h, its GroupNorm statistics included.
 * dh: device [B, n_h], 16-byte aligned (it is read as float4, like every row the engine copies), NULL = plain forward.
 * Invalidates the cached primal. */
int  loco_unet_forward_dh(loco_ctx* ctx, const float* x, float t, int32_t B, const float* dh, float* eps, void* stream);
/* loco_pmp_primal with the operator that the later loco_pmp_jvp / loco_pmp_vjp calls apply; the next
 * loco_pmp_primal* call replaces it.
 *   tap 0: exactly loco_pmp_primal.
 *   tap 1 (encoder): J = d h / d x_t, [n_h x n_in] (local_encoder_pullback_xt, diffusion.py:484-560).  mask must be
 *          NULL; at and use_et are not read.  jvp: V [k, n_in] -> U [k, n_h]; vjp: U [k, n_h] -> A [k, n_in].
 *   tap 2 (decoder): J = mask . c . d eps / d h with x_t, the skip tensors and the embedding held fixed, [n_out x n_h]
 *          (what get_h_to_e differentiates).  use_et != 0: c = 1 (local_decoder_pullback_xt); use_et == 0:
 *          c = -sqrt(1 - at) / sqrt(at) (local_x0_decoder_pullback_xt: the x_t term of x0 does not depend on h).
 *          mask (optional) selects outputs.  jvp: V [k, n_h] -> U [k, n_out]; vjp: U [k, n_out] -> A [k, n_h].
 * The solver algebra (loco_orthonormalize, loco_qr_rows, loco_convergence_rows, loco_krylov_*) takes rows of up to
 * max(n_in, n_out, n_h) elements on a context with a tap.  loco_mask_count / loco_mask_gather follow the operator's
 * output: without a mask L = n_h and rows of n_h floats after a tap 1 primal, n_out otherwise.  V, U and A rows are
 * read and written as float4: 16-byte aligned pointers. */
int  loco_pmp_primal_tap(loco_ctx* ctx, const float* x, float t, float at, const uint8_t* mask, int32_t use_et,
                         int32_t tap, void* stream);
/* The tap 2 (decoder) primal of loco_pmp_primal_tap at a SHIFTED bottleneck: the forward pass runs with h <- h + dh, dh [n_h]
 * injected where loco_unet_forward_dh injects it, so every record the later loco_pmp_jvp / loco_pmp_vjp / loco_pmp_primal_eps
 * read -- the tensors behind the tap and the GroupNorm statistics over them -- is taken at h + dh: J = mask . c . d eps / d h
 * at h(x_t) + dh, and loco_pmp_primal_eps returns what loco_unet_forward_dh(x, t, dh) returns.  dh == NULL: exactly
 * loco_pmp_primal_tap(.., tap = 2).  Refused like loco_unet_forward_dh: a network without a tap, a tap op that is not an
 * identity-shortcut ResBlock. */
int  loco_pmp_primal_tap_dh(loco_ctx* ctx, const float* x, float t, float at, const uint8_t* mask, int32_t use_et,
                            const float* dh, void* stream);
/* eps[n_out] = the network output the last loco_pmp_primal / _tap (tap 0 or 2) evaluated at its linearisation point: a copy
 * out of the cached state, no second evaluation.  Valid until the next call that runs the network on this context. */
int  loco_pmp_primal_eps(loco_ctx* ctx, float* eps, void* stream);

/* Thin SVD re-orthonormalisation of the k x n block (replaces torch.linalg.svd
 * at edit.py:2482): on return A holds Vh (orthonormal rows, descending
 * singular value, sign: largest-|.| entry of each row positive), s[k] the
 * singular values of the input. k <= 64.
 * Rows are found through the double-precision Gram A A^T, which resolves singular values down to about 1e-7 of
 * the largest.  A row whose s_i >= 1e-6 s_0 is determined: unit norm, orthogonal to the others to fp32 rounding,
 * the singular vector of the input.  Below that a row is either a unit vector orthogonal to every row before it
 * (its direction is then not meaningful) or, when its eigenvalue is at the Gram's rounding floor (2^-47 of the
 * largest: rank-deficient input, more probes than directions, A = 0), exactly zero with s_i = 0.  No row is ever
 * longer than a unit vector and no output is non-finite for finite input. */
int  loco_orthonormalize(loco_ctx* ctx, float* A, int32_t k, int64_t n, float* s, void* stream);
/* Q = thin-QR orthonormal basis of the rows of A (replaces torch.linalg.qr at
 * edit.py:2436 on the transposed layout): A [k,n] in, orthonormal rows out,
 * row i in span(rows 0..i) with positive pivot. */
int  loco_qr_rows(loco_ctx* ctx, float* A, int32_t k, int64_t n, void* stream);
/* Convergence test of edit.py:2489-2492: out[0] = ||Vp - V||_F,
 * out[1] = 1.0 if allclose(Vp, V, atol, rtol=1e-5) else 0.0 (device floats). */
int  loco_convergence(loco_ctx* ctx, const float* Vprev, const float* V, int64_t count,
                      float atol, float* out2, void* stream);
/* The same test row by row and up to each row's sign: the reference compares LAPACK's singular vectors
 * (edit.py:2482-2492), whose signs are LAPACK's choice and, for k >= 2, change from one iteration to the next
 * (tests/golden/converge.pt records it); the rows computed here carry no sign of their own.  Vprev, V: [k, n];
 * out[0] = sqrt(sum_rows min(||vp - v||^2, ||vp + v||^2)), out[1] = 1.0 if every row is allclose(atol, rtol=1e-5)
 * to +-its predecessor. k <= 64. */
int  loco_convergence_rows(loco_ctx* ctx, const float* Vprev, const float* V, int32_t k, int64_t n,
                           float atol, float* out2, void* stream);

/* Block Krylov solver for the same basis (opt-in; DESIGN.md "Block Krylov solver"): Rayleigh-Ritz on J^T J over every
 * block of iterates instead of the last one.  The caller keeps Q [m, n] (orthonormal fp32 rows in blocks of k, block 0
 * = the QR'd start) and Ustore [m, n_out] (the rows J Q); the context keeps, per `slot` (0 or 1: two solves may be in
 * flight, e.g. the modify-space and null-space solves of one edit), T = Q J^T J Q^T, its Ritz pairs, the Gram of the
 * residual block and the signs of the returned rows, all in double.  1 <= k <= 32, m a multiple of k, m <= 64,
 * n <= C*H*W of the context (max(C*H*W, n_h) on a context with an h-space tap); every pointer is device memory of the caller; nothing is allocated and the only values
 * meant to be read back per step are the four floats of `stat`:
 *   stat[0], stat[1]  distance and allclose flag of loco_convergence_rows between Y and Yprev (-1, 0 without Yprev)
 *   stat[2]           the largest residual estimate of this step
 *   stat[3]           1 when the next block is entirely zero (the Krylov space is invariant), else 0
 *
 * loco_krylov_extend: A [k, n] = J^T J (newest k rows of Q), overwritten.  Fills T's newest block column and row from
 * A Q^T, orthogonalises A against the m rows of Q (block Gram-Schmidt, two passes) into the residual block R, keeps
 * G = R R^T and the Ritz pairs of T[:m, :m], and -- when `next` is not NULL -- writes the next block to next [k, n]
 * (rows m .. m+k of Q, or A itself): R orthonormalised within itself, a direction whose singular value is below
 * 1e-6 of the largest Ritz value left as a ZERO row in place, then projected once more against Q.  Sets stat[3]. */
int  loco_krylov_extend(loco_ctx* ctx, float* A, int32_t k, const float* Q, int32_t m, int64_t n, float* next,
                        float* stat, int32_t slot, void* stream);
/* After loco_krylov_extend with the same Q, m, slot: Y [k, n] = the top-k Ritz vectors W[:k] Q (sign: largest-|.| entry
 * of each row positive), resid[k] = sqrt(w_i^T G w_i) / theta_0 with w_i the last k entries of Ritz vector i -- the
 * norm of J^T J y_i - theta_i y_i relative to the largest Ritz value, at no further pass -- and, with Yprev [k, n]
 * (NULL: none), the row-wise convergence test against it.  Sets stat[0..2]. */
int  loco_krylov_ritz(loco_ctx* ctx, const float* Q, int32_t m, int64_t n, int32_t k, float* Y, const float* Yprev,
                      float atol, float* resid, float* stat, int32_t slot, void* stream);
/* After loco_krylov_ritz: UY [k, n_out] = the same combination and signs of the rows of Ustore [m, n_out] (= J Y), and
 * s[k] = ||UY_i||^2, the Rayleigh quotient of J^T J on the rows themselves.  n_out may exceed the context's width. */
int  loco_krylov_left(loco_ctx* ctx, const float* Ustore, int32_t m, int64_t n_out, int32_t k, float* UY, float* s,
                      int32_t slot, void* stream);

/* Null-space projection + row normalisation (edit.py:2317-2323):
 * out = normalize_rows(Vm - (Vn^T (Vn Vm^T))^T); Vn==nullptr: normalise only. */
int  loco_null_project(loco_ctx* ctx, const float* Vm, int32_t k, const float* Vn, int32_t k0,
                       int64_t n, float* out, void* stream);
/* Edit step x + alpha*v (x_space_guidance_direct, edit.py:2618-2625), batched:
 * out[b] = x + alphas[b]*v for b < B (alphas on host). */
int  loco_edit_axpy(loco_ctx* ctx, const float* x, const float* v, const float* alphas,
                    int32_t B, int64_t n, float* out, void* stream);
/* Compact the masked entries: out[k, L] = U[k, mask] (P_xt[:, mask], edit.py:2390). */
int  loco_mask_gather(loco_ctx* ctx, const float* U, int32_t k, float* out, void* stream);
/* L = number of selected mask elements of the last loco_pmp_primal (C*H*W without a mask).  The gather list is built
 * on the device; the first call after a primal reads L back (one 4-byte copy + stream sync). */
int64_t loco_mask_count(loco_ctx* ctx);

/* Measurement helper for bench.py: enqueue a one-lane kernel that writes {shader-clock counter (s_memtime),
 * 100 MHz counter (s_memrealtime)} to out2 (device, 2 x uint64).  Two stamps around a timed region give the average
 * shader clock over it: (d s_memtime / d s_memrealtime) x 100 MHz -- MI355X lowers its clock under matrix load and
 * boxes differ by several percent, which otherwise hides kernel changes in box-to-box comparisons. */
int  loco_clock_stamp(loco_ctx* ctx, uint64_t* out2, void* stream);

/* Work model helpers for bench.py: 2*MAC of one denoiser evaluation (B=1). */
double loco_unet_flops(loco_ctx* ctx);
/* Bytes of device memory the ctx holds. */
int64_t loco_workspace_bytes(loco_ctx* ctx);

/* HIP-event timing on the stream the kernels run on (bench.py roofline leg):
 * average duration in ms of kernels whose name contains `substr` is not
 * available from the API; instead these bracket a region. */
int  loco_timer_start(loco_ctx* ctx, void* stream);
int  loco_timer_stop(loco_ctx* ctx, void* stream, float* ms);

/* Arithmetic of the convolutions: 0 = exact fp32 (v_mfma_f32_32x32x2_f32, the parity
 * anchor), 1 = split-bf16 "bf16x3" (3 x v_mfma_f32_32x32x16_bf16 per product, fp32
 * accumulate, fp32-faithful to ~2^-16; the default), 2 = "f16" (one v_mfma_f32_32x32x16_f16
 * per product: operands rounded to 11 significant bits -- the precision class of the TF32
 * convolutions the reference's CUDA path runs by PyTorch default --, fp32 accumulate and
 * fp32 tensors in HBM).  Env LOCO_PRECISION=f32|bf16x3|f16 sets the initial mode.
 * Invalidates the cached primal. */
int  loco_set_precision(loco_ctx* ctx, int32_t mode);
/* Probe groups of one tangent / cotangent pass on n = 1 (default) or 2 HIP streams: the probes of a batch are independent,
 * so with n = 2 a batch of >= 4 is cut in two groups enqueued on two streams (the bandwidth-bound statistics / apply
 * kernels of one group run beside the convolutions of the other; results identical).  Env LOCO_STREAMS sets the initial
 * value.  Per-kernel durations measured while two streams overlap are not kernel properties: bench.py keeps n = 1 for
 * the headline and its roofline, and reports n = 2 as an extra line. */
int  loco_set_streams(loco_ctx* ctx, int32_t n);
/* The second stream of the n = 2 mode, supplied by the caller (nullptr: the context's own).  HIP hands hardware queues out
 * round-robin over a few (GPU_MAX_HW_QUEUES, 4 by default): a stream created by the library may land on the queue of the
 * caller's stream and then runs strictly behind it -- same results, no overlap.  The host can measure which of its streams
 * runs beside its current one (loco_edit_amd.tloco.BranchStreams._pick: two spin kernels) and hand that one over. */
int  loco_set_side_stream(loco_ctx* ctx, void* stream);
/* n = number of engine contexts whose passes the host enqueues SIDE BY SIDE on different streams (the guidance branches of
 * T-LOCO: loco_edit_amd.tloco.BranchStreams; reference: the prompts of one batched U-Net call, edit.py:1319-1322).  A launch
 * then has about 1 / n of the chip, and the split-K choice of the small-image convolutions aims at 256 / n workgroups instead
 * of 256: fewer partial tiles and less reduce work for the same occupancy (config 5: 315 -> 296 ms per solve at n = 2).
 * Default 1.  Results change by the summation order of the split only. */
int  loco_set_chip_share(loco_ctx* ctx, int32_t n);
int  loco_get_precision(loco_ctx* ctx);

/* Conditional denoisers (T-LOCO, reference edit.py:1286-1373 `self.unet(x, t, encoder_hidden_states=...)`): a
 * conditioning embedding of temb_ch = 4*ch floats (device pointer) that is added to the time embedding before its
 * SiLU -- the slot guided-diffusion uses for `label_emb(y)` (unet.py:660-662) and diffusers' UNet2DConditionModel for
 * `addition_embed_type="text"`.  NULL clears it.  Invalidates the cached primal. */
int  loco_set_cond(loco_ctx* ctx, const float* emb_add, void* stream);
/* Guidance-scale embedding of a latent-consistency denoiser (cfg.time_cond_proj_dim = P > 0; the `timestep_cond` of
 * `self.unet(latents, t, timestep_cond=w_embedding, ...)`, src/modules/edit.py:126-132): w_emb = device pointer to P floats.
 * Computes cond_in[ch] = cond_proj.weight . w_emb once (exact fp32, one wave per row) into a buffer this context owns; every
 * later time embedding adds it to the sinusoid.  Per context, not per parameter store: forks of one store keep their own
 * (a fork starts without one).  The buffer's address never changes, so a captured forward graph stays valid across calls.
 * NULL clears it (evaluations are then bit-identical to a context that never had one).  Constant in x: the tangent and
 * cotangent passes are unchanged.  Invalidates the cached primal; refused when time_cond_proj_dim == 0. */
int  loco_set_time_cond(loco_ctx* ctx, const float* w_emb, void* stream);
/* out[k, n] = mask * (cv * V + ce * E) with the mask of the last loco_pmp_primal (all ones without one): the
 * x0_hat = (x - eps sqrt(1-at)) / sqrt(at) algebra of edit.py:1574 / 2385 applied to tangents or cotangents when eps is a
 * CFG combination assembled by the caller.  V, E: [k, n]; out may alias either. */
int  loco_masked_axpby(loco_ctx* ctx, const float* V, const float* E, float cv, float ce, int32_t k, float* out,
                       void* stream);
/* Latent encoder contexts (arch 3): z[B, Z, h, w] = scale * (mean + exp(0.5 clamp(logvar, -30, 20)) * noise) from the
 * moments [B, 2 Z, h, w] loco_unet_forward returned (mean | logvar) -- `self.vae.encode(x0).latent_dist.sample() * 0.18215`
 * of the latent inversion (src/modules/edit.py:594-597; DiagonalGaussianDistribution of diffusers, un-vendored).
 * noise: [B, Z, h, w] standard normal, or NULL for the posterior mean (`.mode()`). */
int  loco_latent_sample(loco_ctx* ctx, const float* moments, const float* noise, float scale, int32_t B, float* z, void* stream);
/* out = sum_{i<n} coef[i] * src[i], n <= 4: the classifier-free-guidance combination of eps / J V / J^T U terms of
 * several conditions (edit.py:1324-1372).  src: host array of device pointers, coef: host array; out may alias a src. */
/* Encoder states of the prompt for the cross-attention stages (context_dim > 0): tokens = device pointer to
 * [context_len][context_dim] fp32.  Projects them to the per-block keys / values once; the cached primal is
 * invalidated.  Replaces `encoder_hidden_states=prompt_emb` of self.unet(...) (edit.py:664-667, 1319-1322).
 * With cfg.added_kv (the DeepFloyd-IF U-Net) the tokens are the states AFTER the model's `encoder_hid_proj` (the host computes
 * that projection and the pooled `add_embedding` for loco_set_cond once per prompt): every attention block passes them
 * through its own GroupNorm (`norm_cross`) and key / value projections (`add_k_proj`, `add_v_proj`) here, and attends over
 * [these ; its image tokens] in one softmax. */
int  loco_set_context(loco_ctx* ctx, const float* tokens, void* stream);

int  loco_lincomb(loco_ctx* ctx, const float* const* src, const float* coef, int32_t n, float* out, int64_t count,
                  void* stream);

/* DiffEdit mask from two guided noise predictions: the body of EditDeepFloydIF.mask_diffedit after its denoiser calls
 * (edit.py:1401-1402).  eps_a, eps_b: [B, C, HW] device tensors;
 *   m[p] = mean_c( mean_b( scale * (eps_a[b,c,p] - eps_b[b,c,p]) ) )     (batch first, then channels, as the reference)
 * rule 0 ("reference"): mask = round(m - min / (max - min)) != 0 with round-half-to-even, i.e. |m - min/(max - min)| > 0.5
 *                       -- edit.py:1402 as its parentheses stand;
 * rule 1 ("intended"):  mask = (m - min) / (max - min) > 0.5.
 * m_out: [HW] floats or NULL, mask_out: [HW] uint8.  Two launches; min and max stay on the device, the call ends with one
 * read-back of a status word (it synchronises the stream): a constant map (max == min, where the reference divides by zero
 * and returns an all-True mask out of NaN) returns -4, a non-finite map -5, the cause in loco_last_error. */
int  loco_diffedit_mask(loco_ctx* ctx, const float* eps_a, const float* eps_b, float scale, int32_t B, int32_t C,
                        int64_t HW, int32_t rule, float* m_out, uint8_t* mask_out, void* stream);
/* One step of EditDeepFloydIF.MaskedDDPMforwardsteps after the denoiser calls (edit.py:1540-1548), fused:
 *   eF = n + g (f - n), eE = n + g (e - n)          (edit.py:1336, 1341: guidance_scale for both)
 *   x_next = mask ? step(x, eE) : step(x, eF)        step = the eta = 0 update of loco_sched_step
 * x, eps_for, eps_edit, eps_null, x_next: [B, n]; mask: uint8 [n] (the format loco_pmp_primal takes), broadcast over B.
 * A select, so a non-finite value of the half not taken does not reach x_next.  x_next may alias x. */
int  loco_cfg_masked_step(loco_ctx* ctx, const float* x, const float* eps_for, const float* eps_edit,
                          const float* eps_null, float g, float at, float at_next, const uint8_t* mask, int32_t B,
                          int64_t n, float* x_next, void* stream);

/* One step of the latent-consistency scheduler after the denoiser call (LCMScheduler.step as src/modules/edit.py:135, 194, 235
 * use it), one launch, per element in fp32:
 *   x0       = (x - sqrt(1 - at) eps) / sqrt(at)
 *   denoised = c_out x0 + c_skip x                                  (boundary-condition scalings)
 *   x_prev   = noise ? sqrt(at_prev) denoised + sqrt(1 - at_prev) noise : denoised
 * x, eps, noise, x_prev, denoised: `count` floats; noise NULL on the last step; x_prev and denoised may each be NULL (not
 * written), x_prev may alias x.  No scratch.  Replaces loco_sched_step + two loco_lincomb (three launches, two intermediates). */
int  loco_lcm_step(loco_ctx* ctx, const float* x, const float* eps, float at, float at_prev, float c_skip, float c_out,
                   const float* noise, int64_t count, float* x_prev, float* denoised, void* stream);

/* Per-kernel HIP-event profile of the convolution launches (bench.py roofline
 * leg).  While enabled every conv launch is bracketed by two events on the
 * caller's stream; loco_profile_report synchronises, then writes one line per
 * kernel variant: "name launches total_ms total_flops" (algorithmic 2*MAC). */
int  loco_profile_enable(loco_ctx* ctx, int32_t on);
int  loco_profile_report(loco_ctx* ctx, char* buf, int64_t cap);

/* --- CLIP text encoder (Stable Diffusion prompt embeddings) ---
 * The CLIPTextModel of transformers as diffusers' StableDiffusionPipeline.encode_prompt runs it (reference
 * src/modules/edit.py:1187-1194): token + position embedding, `layers` pre-LN blocks (LayerNorm -> causal multi-head
 * self-attention, scale head_dim^-0.5 -> residual; LayerNorm -> fc1 -> act -> fc2 -> residual), final_layer_norm; output
 * last_hidden_state.  Exact fp32 throughout (independent of loco_set_precision / LOCO_PRECISION).  Its own handle: it shares
 * nothing with a loco_ctx. */
typedef struct loco_text loco_text;
typedef struct loco_text_cfg {
    int32_t vocab;        /* rows of embeddings.token_embedding (49408 for the SD checkpoints) */
    int32_t width;        /* hidden_size: 768 (SD 1.x), 1024 (SD 2.x) */
    int32_t layers;       /* num_hidden_layers: 12 / 23 */
    int32_t heads;        /* num_attention_heads: 12 / 16 */
    int32_t ffn;          /* intermediate_size: 3072 / 4096 */
    int32_t positions;    /* max_position_embeddings = the token count L of every prompt (77), <= 128 */
    int32_t act;          /* hidden_act: 0 quick_gelu x sigmoid(1.702 x) (SD 1.x), 1 exact erf gelu (SD 2.x) */
    float   ln_eps;       /* layer_norm_eps (1e-5) */
} loco_text_cfg;
/* max_prompts: the largest n one loco_text_encode call may carry (the device workspace is sized for it). */
int  loco_text_create(const loco_text_cfg* cfg, int32_t device, int32_t max_prompts, loco_text** out);
/* One call per state_dict entry in CLIPTextTransformer naming, without a `text_model.` prefix (embeddings.token_embedding.weight,
 * encoder.layers.{i}.self_attn.q_proj.weight, ..., final_layer_norm.bias).  `host`: fp32 values, a host or a device pointer. */
int  loco_text_load_param(loco_text* t, const char* name, const float* host, const int64_t* shape, int32_t ndim);
/* 0 when every parameter has been loaded, else the count still missing (first missing name in loco_text_last_error). */
int  loco_text_params_missing(loco_text* t);
/* out_dev[n][positions][width] = last_hidden_state of the n prompts ids_dev[n][positions] (int32 token ids, device).  One batch:
 * every layer's weights are read once per call.  The ids are range-checked on the host (one copy + stream synchronisation
 * before the first kernel), nothing synchronises between layers.  Each row is bit-identical whatever n and its position. */
int  loco_text_encode(loco_text* t, const int32_t* ids_dev, int32_t n, float* out_dev, void* stream);
/* Message of the last failed call on t; t == NULL: of the last failed loco_text_create. */
const char* loco_text_last_error(loco_text* t);
void loco_text_destroy(loco_text* t);

/* --- T5 text encoder (DeepFloyd IF prompt embeddings) ---
 * The encoder of transformers' T5EncoderModel (T5 v1.1) as diffusers' IFPipeline.encode_prompt runs it (reference
 * src/modules/edit.py:1274-1284): token embedding (no position embedding, no scale), `layers` blocks of
 * RMS norm -> q / k / v without bias to heads * d_kv channels -> scores q k^T (no 1 / sqrt(d)) + relative position bias
 * (bidirectional buckets, the table of block 0 serves every block) + key padding mask -> fp32 softmax -> P v -> o -> residual;
 * RMS norm -> wo(gelu_new(wi_0 x) * (wi_1 x)) -> residual; final RMS norm; output last_hidden_state.  Exact fp32 throughout,
 * fp32 storage (4.76e9 parameters = 19.0 GB at the XXL geometry).  The handle is a loco_text: loco_text_load_param,
 * loco_text_params_missing, loco_text_last_error and loco_text_destroy serve it as they serve a CLIP handle. */
typedef struct loco_t5_cfg {
    int32_t vocab;         /* rows of shared.weight (32128) */
    int32_t d_model;       /* 4096 at XXL */
    int32_t d_kv;          /* channels per head (64); heads * d_kv need not equal d_model */
    int32_t heads;         /* num_heads (64) */
    int32_t d_ff;          /* 10240 */
    int32_t layers;        /* num_layers (24) */
    int32_t positions;     /* L: the token count every prompt is padded to (77 for IF), <= 128 */
    int32_t buckets;       /* relative_attention_num_buckets (32) */
    int32_t max_distance;  /* relative_attention_max_distance (128) */
    int32_t act;           /* feed_forward_proj: 0 gated-gelu (the only one built) */
    float   ln_eps;        /* layer_norm_epsilon (1e-6) */
} loco_t5_cfg;
/* Parameter names for loco_text_load_param are the T5EncoderModel state_dict names: shared.weight,
 * encoder.block.{i}.layer.0.SelfAttention.{q,k,v,o}.weight, encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight,
 * encoder.block.{i}.layer.0.layer_norm.weight, encoder.block.{i}.layer.1.DenseReluDense.{wi_0,wi_1,wo}.weight,
 * encoder.block.{i}.layer.1.layer_norm.weight, encoder.final_layer_norm.weight. */
int  loco_t5_create(const loco_t5_cfg* cfg, int32_t device, int32_t max_prompts, loco_text** out);
/* out_dev[n][positions][d_model] of the n prompts ids_dev[n][positions] (device, padded with any valid id, 0 for IF) whose
 * first lens[p] tokens are real: keys at positions >= lens[p] are excluded from every softmax of prompt p, the padded query
 * rows are still computed and returned (as transformers does with an attention mask).  lens: host int32[n], each in
 * [1, positions], or NULL = every prompt is `positions` long.  ids and lens are checked on the host once per call; each
 * output row is bit-identical whatever n, its position in the batch and the lengths of the other prompts.  On a CLIP handle
 * this call is an error; loco_text_encode on a T5 handle means lens == NULL. */
int  loco_text_encode_masked(loco_text* t, const int32_t* ids_dev, const int32_t* lens, int32_t n, float* out_dev, void* stream);

/* --- Segment Anything image encoder (edit masks) ---
 * The SamVisionEncoder of transformers, which the reference's mask_segmentation.py runs inside the mask-generation pipeline:
 * 16 x 16 patch embedding + learned absolute position embedding; `depth` pre-LN blocks whose attention runs inside
 * window_size x window_size windows (the normalised map zero-padded at the bottom and right to a multiple of the window; the
 * padded tokens take part as keys and queries, unmasked) or, at the layers listed in global_attn, over the whole map; scores
 * (q scale) k^T + rel_h[q, row(k)] + rel_w[q, col(k)] with rel_h[q, j] = q . rel_pos_h[row(q) - j + size - 1] from the unscaled
 * query (decomposed relative position bias), fp32 softmax; erf-GELU MLP; neck: 1x1 conv -> channel LayerNorm (eps 1e-6) ->
 * 3x3 conv pad 1 -> channel LayerNorm.  Exact fp32 throughout (independent of loco_set_precision / LOCO_PRECISION), sums in
 * a fixed order, no host synchronisation inside a call.  Its own handle; the workspace for one image is allocated at create. */
#define LOCO_SAM_MAX_GLOBAL 16
typedef struct loco_sam loco_sam;
typedef struct loco_sam_cfg {
    int32_t image_size;    /* S: side of pixel_values (1024) */
    int32_t patch_size;    /* 16; the token grid is G = S / patch_size */
    int32_t width;         /* hidden_size D: 768 (ViT-B), 1024 (ViT-L), 1280 (ViT-H) */
    int32_t depth;         /* num_hidden_layers: 12 / 24 / 32 */
    int32_t heads;         /* num_attention_heads: 12 / 16 / 16; head width hd = D / heads.  The attention kernel's LDS,
                            * 4 (144 hd + 32 max(G, window_size) + 1088) bytes, must fit 64 KiB: hd <= 92 at G 64 (ViT-H has 80),
                            * hd <= 106 at the smallest grid; loco_sam_create refuses the rest */
    int32_t mlp_dim;       /* 4 D */
    int32_t window_size;   /* 14 */
    int32_t num_global;    /* entries of global_attn, <= LOCO_SAM_MAX_GLOBAL */
    int32_t global_attn[LOCO_SAM_MAX_GLOBAL];   /* global_attn_indexes: [2,5,8,11] / [5,11,17,23] / [7,15,23,31] */
    int32_t out_channels;  /* output_channels C_out of the neck (256) */
    float   ln_eps;        /* layer_norm_eps of the blocks (1e-6) */
} loco_sam_cfg;
int  loco_sam_create(const loco_sam_cfg* cfg, int32_t device, loco_sam** out);
/* One call per state_dict entry in SamVisionEncoder naming, without a `vision_encoder.` prefix (patch_embed.projection.weight,
 * pos_embed, layers.{i}.attn.qkv.weight, layers.{i}.attn.rel_pos_h, ..., neck.layer_norm2.bias).  rel_pos_h / rel_pos_w must
 * have 2 window_size - 1 rows in a windowed layer and 2 G - 1 in a global one (transformers would interpolate another
 * length; here it is a shape error).  `host`: fp32 values, a host or a device pointer. */
int  loco_sam_load_param(loco_sam* t, const char* name, const float* host, const int64_t* shape, int32_t ndim);
int  loco_sam_params_missing(loco_sam* t);
/* out_dev[C_out][G][G] = image embeddings of pixel_values[3][S][S] (device, preprocessed: normalised and zero-padded). */
int  loco_sam_encode(loco_sam* t, const float* pixel_values, float* out_dev, void* stream);
/* on != 0: the following encodes bracket their launches with events; loco_sam_profile_read waits for the last one and returns
 * its milliseconds in ms4 = { GEMMs, windowed attention, global attention, everything else } (the attention entries include
 * the relative position tables). */
int  loco_sam_profile(loco_sam* t, int32_t on);
int  loco_sam_profile_read(loco_sam* t, float* ms4);
/* Message of the last failed call on t; t == NULL: of the last failed loco_sam_create. */
const char* loco_sam_last_error(loco_sam* t);
void loco_sam_destroy(loco_sam* t);

/* --- Segment Anything prompt encoder + mask decoder + mask scoring (edit masks) ---
 * The head of transformers' SamModel for point prompts with multimask_output = true, as mask_segmentation.SamHead states it:
 * one foreground point and the padding point per prompt (random-Fourier features of the shared positional matrix, accurate
 * sinf / cosf), the two-way transformer (`layers` blocks: token self-attention, token -> image attention, MLP, image -> token
 * attention, each with its LayerNorm; the final token -> image attention), two stride-2 transposed convolutions with a channel
 * LayerNorm and erf-GELUs, the hypernetwork product and the IoU head.  NQ = num_multimask_outputs + 4 tokens per prompt.
 * Exact fp32 throughout (independent of loco_set_precision / LOCO_PRECISION), sums in a fixed order, no atomics on floats, no
 * host synchronisation inside a call; a prompt's rows are bit-identical whatever P and its position.  Its own handle; the
 * workspace for max_prompts prompts is allocated at create: the per-prompt image tokens [P][C][G^2] and one more tensor of
 * that size for the projections of them the algorithm needs, never a [P][G^2] x NQ score tensor nor the maps after the second
 * transposed convolution. */
typedef struct loco_samdec loco_samdec;
typedef struct loco_samdec_cfg {
    int32_t grid;                      /* G: side of the image embedding (64) */
    int32_t image_size;                /* S = G * patch (1024): recorded, the coordinates arrive normalised */
    int32_t hidden;                    /* C: 256; 32, 64, 128 or 256 (the upscaling kernel is built for C / 4 = 8 ... 64) */
    int32_t layers;                    /* num_hidden_layers of the two-way transformer (2) */
    int32_t heads;                     /* num_attention_heads (8): C and C / attention_downsample_rate are multiples of it; the
                                        * cross-attention head width C / rate / heads must be a power of two <= 64 */
    int32_t mlp_dim;                   /* 2048, a multiple of 4 */
    int32_t attention_downsample_rate; /* 2 */
    int32_t num_multimask_outputs;     /* 3 (<= 4: 8 tokens per prompt at most) */
    int32_t iou_head_depth;            /* 3 (>= 2) */
    int32_t iou_head_hidden_dim;       /* 256, a multiple of 4 */
    float   layer_norm_eps;            /* 1e-6 (the LayerNorm after the final attention uses 1e-5, as transformers' default) */
    int32_t hidden_act;                /* activation of the transformer's MLP: 0 relu, 1 erf gelu */
    int32_t max_prompts;               /* the largest P of a predict call (64) */
} loco_samdec_cfg;
int  loco_samdec_create(const loco_samdec_cfg* cfg, int32_t device, loco_samdec** out);
/* One call per entry in SamModel naming: shared_image_embedding.positional_embedding, prompt_encoder.{no_mask_embed,
 * not_a_point_embed,point_embed.1}.weight, mask_decoder.* (mask_segmentation.head_param_shapes lists them). */
int  loco_samdec_load_param(loco_samdec* t, const char* name, const float* host, const int64_t* shape, int32_t ndim);
int  loco_samdec_params_missing(loco_samdec* t);
/* Once per image, emb_dev[C][G][G]: src = emb + no_mask_embed, the grid's positional encoding pos, layer 0's k / v projections
 * of src + pos / src and its image -> token query projection, and pos W for the later projections of keys + pos (the image
 * tokens of layer 0 are the same for every prompt; (keys + pos) W is evaluated as keys W + pos W from layer 1 on). */
int  loco_samdec_set_image(loco_samdec* t, const float* emb_dev, void* stream);
/* coords_dev[P][2]: (x, y) of the foreground points as 2 (p + 0.5) / S - 1 in fp32, 1 <= P <= max_prompts.
 * masks_out[P][num_multimask_outputs][4G][4G], iou_out[P][num_multimask_outputs]: mask token 0 is dropped. */
int  loco_samdec_predict(loco_samdec* t, const float* coords_dev, int32_t P, float* masks_out, float* iou_out, void* stream);
/* The automatic mask generator's view of low_res_dev[N][h][w] at the original size: each logit is the bilinear resampling
 * (align_corners = false) to image_size x image_size, cropped to reshaped h x w, resampled to orig h x w; neither map is
 * stored.  counts_out[N][2] = pixels above thr + offset and above thr - offset, boxes_out[N][4] = inclusive XYXY box of
 * logit > thr, 0 0 0 0 for an empty mask.  Works on a handle without parameters. */
int  loco_samdec_score(loco_samdec* t, const float* low_res_dev, int32_t N, int32_t h, int32_t w, int32_t orig_h, int32_t orig_w,
                       int32_t reshaped_h, int32_t reshaped_w, int32_t image_size, float thr, float offset, int32_t* counts_out,
                       int32_t* boxes_out, void* stream);
/* masks_out[K][orig_h][orig_w] (uint8 0 / 1) = logit > thr of the rows rows_dev[K] (int32, each in [0, N)) of low_res_dev. */
int  loco_samdec_binarize(loco_samdec* t, const float* low_res_dev, int32_t N, const int32_t* rows_dev, int32_t K, int32_t h, int32_t w,
                          int32_t orig_h, int32_t orig_w, int32_t reshaped_h, int32_t reshaped_w, int32_t image_size, float thr,
                          uint8_t* masks_out, void* stream);
/* Message of the last failed call on t; t == NULL: of the last failed loco_samdec_create. */
const char* loco_samdec_last_error(loco_samdec* t);
void loco_samdec_destroy(loco_samdec* t);

/* --- CLIP image encoder (scores of the text-guided edits) ---
 * The CLIPVisionModelWithProjection of transformers: patch embedding (no bias) + class token + learned position embedding,
 * pre_layrnorm, `layers` pre-LN blocks (LayerNorm -> full multi-head self-attention, scale head_dim^-0.5 -> residual;
 * LayerNorm -> fc1 -> act -> fc2 -> residual), post_layernorm of the class token, visual_projection.  Exact fp32 throughout
 * (independent of loco_set_precision / LOCO_PRECISION), sums in a fixed order, no host synchronisation inside an encode.  Its
 * own handle; the workspace for max_images images is allocated at create. */
typedef struct loco_clipvis loco_clipvis;
typedef struct loco_clipvis_cfg {
    int32_t image_size;      /* S: side of pixel_values (224) */
    int32_t patch_size;      /* 14 / 16 / 32; the token grid is G = S / patch_size, T = 1 + G^2 tokens per image */
    int32_t width;           /* hidden_size D: 768 (ViT-B), 1024 (ViT-L) */
    int32_t layers;          /* num_hidden_layers: 12 / 24 */
    int32_t heads;           /* num_attention_heads: 12 / 16; head width hd = D / heads <= 106 (the attention kernel's LDS,
                              * 4 (144 hd + 1088) bytes, must fit 64 KiB); loco_clipvis_create refuses the rest */
    int32_t mlp_dim;         /* intermediate_size: 4 D */
    int32_t projection_dim;  /* P: rows of visual_projection (512 / 768) */
    int32_t act;             /* hidden_act: 0 quick_gelu x sigmoid(1.702 x) (the OpenAI checkpoints), 1 exact erf gelu */
    float   ln_eps;          /* layer_norm_eps (1e-5) */
    float   image_mean[3];   /* loco_clipvis_preprocess: the normalisation of CLIPImageProcessor */
    float   image_std[3];    /* (0.48145466, 0.4578275, 0.40821073) / (0.26862954, 0.26130258, 0.27577711) */
} loco_clipvis_cfg;
/* max_images: the largest n one loco_clipvis_encode call may carry (the device workspace is sized for it). */
int  loco_clipvis_create(const loco_clipvis_cfg* cfg, int32_t device, int32_t max_images, loco_clipvis** out);
/* One call per state_dict entry in CLIPVisionModelWithProjection naming without the `vision_model.` prefix
 * (embeddings.class_embedding, embeddings.patch_embedding.weight, embeddings.position_embedding.weight, pre_layrnorm.* (sic),
 * encoder.layers.{i}.{layer_norm1,self_attn.{q,k,v,out}_proj,layer_norm2,mlp.fc1,mlp.fc2}.*, post_layernorm.*,
 * visual_projection.weight).  `host`: fp32 values, a host or a device pointer. */
int  loco_clipvis_load_param(loco_clipvis* t, const char* name, const float* host, const int64_t* shape, int32_t ndim);
int  loco_clipvis_params_missing(loco_clipvis* t);
/* out_dev[n][3][S][S] (fp32) from frames_dev[n][H][W][3] (uint8, device), the steps of CLIPImageProcessor in float arithmetic:
 * shortest edge -> S (the other edge int(long S / short)) by bicubic interpolation with antialiasing (a = -0.5, support
 * 2 max(scale, 1), weights normalised per output pixel: torch's interpolate(mode="bicubic", antialias=True)), centre crop
 * S x S at offset (size - S) / 2, / 255, (v - image_mean) / image_std.  One pass per axis, only the cropped columns and rows
 * are computed; the row buffer between the passes belongs to the handle and grows on demand (a growing call waits for the
 * device).  PIL, through which transformers resizes, rounds to uint8 after each pass: its result differs by up to a few grey
 * levels where a resize happens.  n is not bound by max_images. */
int  loco_clipvis_preprocess(loco_clipvis* t, const uint8_t* frames_dev, int32_t n, int32_t H, int32_t W, float* out_dev, void* stream);
/* embeds_dev[n][P] = the un-normalised image_embeds of pixel_values[n][3][S][S] (device), 1 <= n <= max_images.  Optional
 * (NULL to skip): hidden_dev[n][T][D] = last_hidden_state (the last block's output, before post_layernorm), pooled_dev[n][D] =
 * pooler_output (post_layernorm of the class token).  Each image's rows are bit-identical whatever n and its position. */
int  loco_clipvis_encode(loco_clipvis* t, const float* pixel_values, int32_t n, float* embeds_dev, float* hidden_dev, float* pooled_dev,
                         void* stream);
/* The residual stream after chosen layers (the activations a CLIPSeg decoder reads): taps_dev[n_taps][n][T][D], token-major as
 * hidden_dev, slot j = the output of layer layers[j] (0-based) = hidden_states[layers[j] + 1] of transformers.  `layers`: host
 * array, strictly increasing, inside [0, cfg.layers).  The tower stops after the last tapped layer; no pooling, no records
 * (a handle with grad enabled keeps those of its last loco_clipvis_encode).  The launches are those of loco_clipvis_encode:
 * each image's taps are bit-identical whatever n and its position. */
int  loco_clipvis_encode_taps(loco_clipvis* t, const float* pixel_values, int32_t n, const int32_t* layers, int32_t n_taps,
                              float* taps_dev, void* stream);
/* --- cotangent of the image tower with respect to the pixels (the text guidance of the Blended Diffusion baseline) ---
 * on != 0: allocates, per layer, the records a backward pass reads -- the layer input and the residual stream after the
 * attention [D][Tp], qkv [3 D][Tp], the attention output [D][Tp], the statistics of both LayerNorms, the softmax row max and
 * row sum per head and token -- and the gradient workspace, (6 D + 4 + 2 heads) Tp floats per layer (ViT-L/14 at max_images 8:
 * 51 MB per layer, 1.3 GB with the workspace; loco_clipvis_grad_bytes tells).  The fc1 pre-activation is recomputed, not kept.
 * From then on every loco_clipvis_encode keeps the records of its call; its three outputs stay bit-identical to those of a
 * handle without grad.  on == 0 frees them.  A handle that never calls this allocates and computes what it always did. */
int  loco_clipvis_enable_grad(loco_clipvis* t, int32_t on);
int64_t loco_clipvis_grad_bytes(loco_clipvis* t);
/* g_pixel_dev[n][3][S][S] = (d image_embeds / d pixel_values)^T g_embeds_dev[n][P] for the images of the last kept
 * loco_clipvis_encode (n must be that call's).  No weight gradients.  Exact fp32, no atomics: an image's gradient is the same
 * bits whatever n and its position, and from call to call.  Refused without grad enabled or before a kept encode. */
int  loco_clipvis_encode_vjp(loco_clipvis* t, const float* g_embeds_dev, int32_t n, float* g_pixel_dev, void* stream);
/* The differentiable preprocessing: out_dev[n][3][S][S] from fp32 frames_dev[nf][3][H][W] in [-1, 1], nf = 1 (one frame seen
 * through n windows) or n.  boxes_dev: int32 [n][4] = (top, left, h, w) on the device, or NULL for the centred largest square
 * of every frame; a box that leaves the frame is refused (the boxes are read back: the call waits for the stream).  A window is
 * resized straight to S x S, each axis through the tap rule of loco_clipvis_preprocess on the window's extent (antialiased
 * bicubic, a = -0.5, positions and weight sums in double; no tap reads outside the window), then (v / 2 + 1 / 2 - mean) / std. */
int  loco_clipvis_preprocess_f32(loco_clipvis* t, const float* frames_dev, int32_t nf, const int32_t* boxes_dev, int32_t n, int32_t H,
                                 int32_t W, float* out_dev, void* stream);
/* Its exact transpose, two gather passes without atomics: g_frames_dev[nf][3][H][W] (every pixel written; with nf = 1 the n
 * windows are summed in window order) from g_pixel_dev[n][3][S][S]. */
int  loco_clipvis_preprocess_f32_vjp(loco_clipvis* t, const float* g_pixel_dev, const int32_t* boxes_dev, int32_t n, int32_t nf, int32_t H,
                                     int32_t W, float* g_frames_dev, void* stream);
/* Message of the last failed call on t; t == NULL: of the last failed loco_clipvis_create. */
const char* loco_clipvis_last_error(loco_clipvis* t);
void loco_clipvis_destroy(loco_clipvis* t);

/* --- CLIPSeg decoder (text-prompted edit masks) ---
 * The CLIPSegDecoder of transformers on the taps of the CLIP image tower (loco_clipvis_encode_taps) and one conditional
 * embedding per mask: taps deepest first; at stage i the state becomes reduces[i](tap) + state; at i == conditional_layer
 * film_mul(c) * x + film_add(c); then a post-norm block x = LN1(x + attn(x)), x = LN2(x + fc2(relu(fc1(x)))) (full attention,
 * scale head_dim^-0.5); the class token is dropped and the head runs: one ConvTranspose2d(reduce_dim, 1, ps, stride ps), or
 * (complex_head) Conv2d 3x3 pad 1, ReLU, ConvTranspose2d(rd, rd / 2, ps / 4, stride ps / 4), ReLU, ConvTranspose2d(rd / 2, 1,
 * ps / 4, stride ps / 4).  Logit side: G ps (simple) or G (ps / 4)^2 (complex), as those layers give it.  Exact fp32
 * (independent of loco_set_precision / LOCO_PRECISION), sums in a fixed order, no atomics: a mask's logits are bit-identical
 * whatever M and its position.  Its own handle; the workspace for max_masks masks is allocated at create. */
typedef struct loco_clipseg loco_clipseg;
typedef struct loco_clipseg_cfg {
    int32_t width;              /* D of the tower the taps come from */
    int32_t grid;               /* G: the tower's token grid at the run size, T = 1 + G^2 <= 2048 */
    int32_t patch_size;         /* ps of the tower (16); complex_head needs ps % 4 == 0 */
    int32_t reduce_dim;         /* rd (64); even with complex_head */
    int32_t heads;              /* decoder_num_attention_heads (4); head width rd / heads in {4, 8, 16, 32, 64} */
    int32_t ffn;                /* decoder_intermediate_size (2048) */
    int32_t n_taps;             /* len(extract_layers) = decoder blocks (3) */
    int32_t conditional_layer;  /* stage at which FiLM is applied (0), inside [0, n_taps) */
    int32_t projection_dim;     /* P: width of a conditional embedding (512) */
    int32_t complex_head;       /* use_complex_transposed_convolution (rd64-refined: 1) */
    float   ln_eps;             /* layer_norm_eps of the vision config (1e-5) */
    int32_t max_masks;          /* the largest M one decode may carry */
} loco_clipseg_cfg;
int  loco_clipseg_create(const loco_clipseg_cfg* cfg, int32_t device, loco_clipseg** out);
/* One call per entry of transformers' `decoder.*` without that prefix: film_mul.*, film_add.*, reduces.{i}.*,
 * layers.{i}.{self_attn.{q,k,v,out}_proj,layer_norm1,mlp.fc1,mlp.fc2,layer_norm2}.*, transposed_convolution.{weight,bias}
 * (simple head) or transposed_convolution.{0,2,4}.{weight,bias} (complex head).  `host`: fp32, a host or a device pointer. */
int  loco_clipseg_load_param(loco_clipseg* t, const char* name, const float* host, const int64_t* shape, int32_t ndim);
int  loco_clipseg_params_missing(loco_clipseg* t);
/* The side of the logits: G ps or G (ps / 4)^2. */
int32_t loco_clipseg_logit_size(loco_clipseg* t);
/* logits_dev[M][s][s] from taps_dev[n_taps][n_images][T][D] (loco_clipvis_encode_taps), cond_dev[M][P] and image_of_mask[M]
 * (host array: the image mask m looks at, inside [0, n_images)); 1 <= M <= max_masks.  The reduces run once per image. */
int  loco_clipseg_decode(loco_clipseg* t, const float* taps_dev, int32_t n_images, const float* cond_dev, const int32_t* image_of_mask,
                         int32_t M, float* logits_dev, void* stream);
/* out_dev[n][3][S][S] (fp32) from frames_dev: is_u8 == 0: fp32 [n][3][H][W] in [-1, 1] (v / 2 + 1 / 2); else uint8 [n][H][W][3]
 * (v / 255).  Each axis is resized to S on its own (no shortest-edge rule, no crop: ViTImageProcessor), antialiased, two
 * passes with the tap rule of loco_clipvis_preprocess; resample 2: the triangle filter (PIL BILINEAR), 3: cubic a = -0.5
 * (BICUBIC), any other value is refused; then (v - mean[c]) / stdev[c] (host arrays of 3). */
int  loco_clipseg_preprocess(loco_clipseg* t, const void* frames_dev, int32_t is_u8, int32_t n, int32_t H, int32_t W, int32_t S,
                             int32_t resample, const float* mean, const float* stdev, float* out_dev, void* stream);
/* One launch: mask_dev[M][res][res] (uint8 0 / 1) = bilinear resize (align_corners = False, no antialias, positions and
 * blend in double) of logits_dev[M][s][s] > threshold_logit (= log(thr / (1 - thr)), the caller's), area_dev[M] (int32) = the
 * set pixels of every mask, counted in a fixed order by the workgroup that owns the mask. */
int  loco_clipseg_masks(loco_clipseg* t, const float* logits_dev, int32_t M, int32_t s, int32_t res, double threshold_logit,
                        uint8_t* mask_dev, int32_t* area_dev, void* stream);
/* Message of the last failed call on t; t == NULL: of the last failed loco_clipseg_create. */
const char* loco_clipseg_last_error(loco_clipseg* t);
void loco_clipseg_destroy(loco_clipseg* t);

/* --- Edit-quality scores of decoded frames (the unconditional drivers' --quality_metrics, eval.py --backend hip) ---
 * LPIPS with the AlexNet backbone, SSIM and mask-restricted MSE between the images of a[n] and b[n], pair by pair, as
 * eval.py defines them.  Independent of loco_set_precision / LOCO_PRECISION, sums in a fixed order, no atomics, no host
 * synchronisation inside a call; a pair's results are bit-identical whatever n and wherever the pair sits in the batch.  Its
 * own handle; the workspace for max_pairs pairs of max_h x max_w images is allocated at create.  SSIM and masked MSE work on
 * a handle without parameters, LPIPS needs all of them. */
typedef struct loco_quality loco_quality;
typedef struct loco_quality_cfg {
    int32_t max_h, max_w;        /* the largest image a call may carry */
    double  ssim_window[11];     /* the 1-D Gaussian window of SSIM (sigma 1.5, normalised to sum 1), computed by the host in
                                  * float64; the 2-D window is its outer product */
} loco_quality_cfg;
int  loco_quality_create(const loco_quality_cfg* cfg, int32_t device, int32_t max_pairs, loco_quality** out);
/* One call per entry of the LPIPS weights under the names of eval.lpips_weight_names(): features.{0,3,6,8,10}.{weight,bias}
 * (torchvision AlexNet: [64,3,11,11], [192,64,5,5], [384,192,3,3], [256,384,3,3], [256,256,3,3]) and lin{0..4}.model.1.weight
 * ([1,C,1,1], the non-negative heads of the lpips package).  `host`: fp32 values, a host or a device pointer. */
int  loco_quality_load_param(loco_quality* q, const char* name, const float* host, const int64_t* shape, int32_t ndim);
int  loco_quality_params_missing(loco_quality* q);
/* out_dev[n] = LPIPS of a_dev[n][3][H][W] and b_dev[n][3][H][W] (device, fp32, in [-1, 1]; normalize != 0: in [0, 1]).  Input
 * scaling (x - shift) / scale; five convolutions with bias and ReLU (11x11 stride 4 pad 2, 5x5 pad 2, three 3x3 pad 1; 3x3
 * stride-2 max-pool before the second and the third) as implicit GEMMs on the exact-fp32 matrix instruction; after each,
 * x / (sqrt(sum_c x^2) + 1e-10), squared difference of the pair, the 1x1 head, spatial mean; the sum of the five taps.  Optional
 * (NULL to skip): taps_dev[n][5], the five terms.  Refused: H or W below 31 (the last taps would be empty) or above the
 * configured maximum, n outside [1, max_pairs], parameters missing. */
int  loco_quality_lpips(loco_quality* q, const float* a_dev, const float* b_dev, int32_t n, int32_t H, int32_t W, int32_t normalize,
                        float* out_dev, float* taps_dev, void* stream);
/* out_dev[n] = mean SSIM of a_dev[n][C][H][W] and b_dev (fp32): 11x11 Gaussian window, reflect padding of 5, k1 = 0.01,
 * k2 = 0.03, the 5-pixel border of the map cropped when H > 10 and W > 10, mean over channels and pixels.  The window moments
 * are summed in double from the fp32 inputs (E[x^2] - mu^2 cancels to the order of c2 in fp32).  Refused: a side below 6
 * (reflect padding undefined) or above the configured maximum, n outside [1, max_pairs], n C above 3 max_pairs planes of the
 * configured size. */
int  loco_quality_ssim(loco_quality* q, const float* a_dev, const float* b_dev, int32_t n, int32_t C, int32_t H, int32_t W,
                       double data_range, double* out_dev, void* stream);
/* sum_dev[i] = sum over mask_dev[i][e] != 0 of (a_dev[i][e] - b_dev[i][e])^2 in double, count_dev[i] = the masked elements of
 * image i (e < elems).  The mean is the caller's: a count may be zero. */
int  loco_quality_masked_mse(loco_quality* q, const float* a_dev, const float* b_dev, const uint8_t* mask_dev, int32_t n, int64_t elems,
                             double* sum_dev, int64_t* count_dev, void* stream);
/* Message of the last failed call on q; q == NULL: of the last failed loco_quality_create. */
const char* loco_quality_last_error(loco_quality* q);
void loco_quality_destroy(loco_quality* q);

/* --- Randomized, centred low-rank PCA of a sample matrix on the device (the h-space PCA baselines, hspace_pca.py) ---
 * Its own handle: the sample store H [n_max][d] (fp32), its centred copy and every workspace are allocated at create.
 * Algorithm, with Omega [d][q] from the caller (so the result is a deterministic function of the store and Omega):
 *     Q = orth(Hc Omega);  niter times: Z = orth(Hc^T Q), Q = orth(Hc Z);  B = Hc^T Q;  B^T B = E diag(lambda) E^T;
 *     s = sqrt(lambda) descending, V = B E / s, every column of V flipped so that its entry of largest magnitude is positive.
 * Hc = fp32(H - mean) formed in double from column means summed in double; orth = CholeskyQR2 with the Gram summed in double
 * over parts of the long dimension whose boundaries depend on its length alone, joined in order (no atomics); the q x q
 * Cholesky, its inverse and the eigendecomposition run in double on the host (each call synchronises `stream` for them).  The
 * products are exact fp32.  Independent of loco_set_precision / LOCO_PRECISION.  Results are bit-identical from call to
 * call and whatever chunks the rows arrived in.  The unit's limit for q is 512. */
typedef struct loco_pca loco_pca;
int  loco_pca_create(int32_t device, int64_t n_max, int64_t d, int32_t q_max, loco_pca** out);
/* Forget the rows (the capacity stays). */
int  loco_pca_reset(loco_pca* p);
/* The rows held, or -1. */
int64_t loco_pca_rows(loco_pca* p);
/* Appends rows_dev [b][d] (device, fp32).  Refused, with the bytes in the message: d other than the handle's, more rows
 * than n_max in all. */
int  loco_pca_add_rows(loco_pca* p, const float* rows_dev, int64_t b, int64_t d, void* stream);
/* s_dev [q], v_dev [d][q], mean_dev [d] (optional; zeros when center == 0) of the rows held.  omega_dev [d][q].  Refused: q
 * above min(N - 1, d) with centring or min(N, d) without, q above q_max or 512, niter < 0; a pivot of a Cholesky
 * factor below 2^-30 of its column's squared norm (or such an eigenvalue of B^T B): the message names the numerical rank
 * and q, and no output is written. */
int  loco_pca_fit(loco_pca* p, int32_t q, int32_t niter, const float* omega_dev, int32_t center, float* s_dev, float* v_dev, float* mean_dev,
                  void* stream);
/* The parts of loco_pca_fit on their own (tests, profiles).  loco_pca_center: centered_dev [N][d] and mean_dev [d] (either may be
 * NULL) of the rows held; center == 0: the rows as they are, mean 0.  loco_pca_gram: g_dev [q][q] (double) = y_dev^T y_dev for
 * y_dev [rows][q], rows <= max(n_max, d).  loco_pca_project: out_dev [N][q] = Hc w_dev (w_dev [d][q]) or, transpose != 0,
 * out_dev [d][q] = Hc^T w_dev (w_dev [N][q]). */
int  loco_pca_center(loco_pca* p, int32_t center, float* centered_dev, float* mean_dev, void* stream);
int  loco_pca_gram(loco_pca* p, const float* y_dev, int64_t rows, int32_t q, double* g_dev, void* stream);
int  loco_pca_project(loco_pca* p, const float* w_dev, int32_t q, int32_t transpose, int32_t center, float* out_dev, void* stream);
/* Route of the two large products: 0 = launch_gemm where the 64 x 64 output grid has 256 tiles or more, else the
 * split-contraction kernel (default); 1 = launch_gemm always; 2 = the split-contraction kernel always. */
int  loco_pca_set_route(loco_pca* p, int32_t route);
/* The routes the last loco_pca_fit / loco_pca_project took, "HW:<route> HtQ:<route>" with gemm, split (contraction in parts)
 * or tile (one part). */
const char* loco_pca_routes(loco_pca* p);
/* Message of the last failed call on p; p == NULL: of the last failed loco_pca_create. */
const char* loco_pca_last_error(loco_pca* p);
void loco_pca_destroy(loco_pca* p);

/* --- The trainable h-space block f_t of the Asyrp baseline (asyrp.py) ---
 * For h [B][C][H][W] (the U-Net bottleneck) and a time vector e [E], with a scalar s per call:
 *     a1 = swish(GroupNorm32(h; g1, b1));   y1 = W1 a1 + c1 + (Wt swish(e) + ct);
 *     a2 = swish(GroupNorm32(y1; g2, b2));  dh = s (W2 a2 + c2)
 * Parameters (loco_asyrp_load_param names): g1 b1 c1 ct g2 b2 c2 [C], W1 W2 [C][C] (1x1 convs), Wt [C][E].  Its own handle:
 * the parameters, their gradient store, Adam's two moments (zero at create) and the records of the last forward live on
 * the device.  Exact fp32 products; every contraction, GroupNorm moment and per-channel sum is accumulated in double in a
 * fixed order and rounded once (no atomics): two identical call sequences give bit-identical results.  Independent of
 * loco_set_precision / LOCO_PRECISION.  Refused at create: C not a positive multiple of 32 or above 2048, a map outside
 * 1 x 1 .. 64 x 64, E outside [1, 8192], max_batch outside [1, 64], gn_eps <= 0. */
typedef struct loco_asyrp loco_asyrp;
int  loco_asyrp_create(int32_t device, int32_t C, int32_t H, int32_t W, int32_t E, int32_t max_batch, float gn_eps, loco_asyrp** out);
/* fp32 values behind a host or a device pointer; shape as listed above. */
int  loco_asyrp_load_param(loco_asyrp* p, const char* name, const float* data, const int64_t* shape, int32_t ndim);
/* The count of parameters not loaded yet (0: complete); the first one's name goes to the last error. */
int  loco_asyrp_params_missing(loco_asyrp* p);
/* Copies parameter `name` / its accumulated gradient to dst (host or device, `count` floats = the parameter's size) after
 * waiting for the device. */
int  loco_asyrp_read_param(loco_asyrp* p, const char* name, float* dst, int64_t count);
int  loco_asyrp_read_grad(loco_asyrp* p, const char* name, float* dst, int64_t count);
/* dh_dev [B][C][H][W] = f_t(h_dev [B][C][H][W], e_dev [E]) scaled by s.  keep_records != 0: the records loco_asyrp_backward
 * reads (the repacked h, a1, y1, a2, both norms' statistics, swish(e), B and s) stay valid until the next forward;
 * keep_records == 0 leaves the handle without records.  Refused: B outside [1, max_batch], parameters missing. */
int  loco_asyrp_forward(loco_asyrp* p, const float* h_dev, const float* e_dev, int32_t B, float s, float* dh_dev, int32_t keep_records,
                        void* stream);
/* For the cotangent g_dh_dev [B][C][H][W] of dh: ADDS the gradients of the ten parameters to the gradient store, from the
 * records of the last forward, and writes the cotangent of h to g_h_dev [B][C][H][W] unless it is NULL.  Refused: no
 * records, B other than the records'. */
int  loco_asyrp_backward(loco_asyrp* p, const float* g_dh_dev, int32_t B, float* g_h_dev, void* stream);
int  loco_asyrp_zero_grad(loco_asyrp* p, void* stream);
/* One Adam step of every parameter from the gradient store, in one launch (torch.optim.Adam's arithmetic, no weight decay):
 *     m = beta1 m + (1 - beta1) g;  v = beta2 v + (1 - beta2) g^2;
 *     p -= lr / (1 - beta1^step) * m / (sqrt(v) / sqrt(1 - beta2^step) + eps)
 * step counts from 1 and is the caller's.  loco_asyrp_reset_moments zeroes m and v. */
int  loco_asyrp_adam_step(loco_asyrp* p, float lr, float beta1, float beta2, float eps, int32_t step, void* stream);
int  loco_asyrp_reset_moments(loco_asyrp* p, void* stream);
/* Message of the last failed call on p; p == NULL: of the last failed loco_asyrp_create. */
const char* loco_asyrp_last_error(loco_asyrp* p);
void loco_asyrp_destroy(loco_asyrp* p);

#ifdef __cplusplus
}
#endif
#endif /* LOCO_HIP_H */
