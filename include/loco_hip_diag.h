/* Diagnostics of libloco_hip -- NOT part of the drop-in boundary (include/loco_hip.h).
 *
 * These entry points live in units of their own, loco-edit_amd/csrc/engine_diag.hip and enc_attn_diag.hip, which are linked only
 * into the diagnostics library (`make -C loco-edit_amd/csrc diag` -> loco-edit_amd/libloco_hip_diag.so: the product's objects +
 * those units, every unit that includes this header built with -DLOCO_DIAG); the by-hand tuning scripts under tests/ load that build through
 * LOCO_HIP_LIB.  The shipped libloco_hip.so does not export them. */
#ifndef LOCO_HIP_DIAG_H
#define LOCO_HIP_DIAG_H
#include "loco_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Tuning hook: average ms of one convolution shape (random scratch data) over `iters` launches.
 * mode: 0 raw, 1 GN+SiLU, 2 GN, 3 tangent, 4 cotangent; tile: -1 auto or a variant id. */
int  loco_bench_conv(loco_ctx* ctx, int32_t cin, int32_t cout, int32_t H, int32_t W, int32_t B, int32_t mode,
                     int32_t taps, int32_t tile, int32_t iters, float* ms_avg, void* stream);

/* Test hook: ONE convolution on caller-supplied operands, through the same run_conv -> plan_conv path the engine's passes use
 * (tests/test_gpu_conv_oracle.py compares it with a float64 reference, tests/conv_oracle.py).
 *
 * Geometry is that of the LAUNCH (ConvArgs): Cin channels of Hin x Win go in, Cout channels of Hout x Wout come out with
 *   Hout = Hin / 2 (stride 2, or pool2), 2 Hin (upsample or zins), Hin (otherwise); Wout likewise.
 * The output map must be one the kernels' tiles cover exactly: Hout and Wout powers of two from 8 (what loco_create admits), or
 * Wout a multiple of 32 with Hout a multiple of 8 and Hout Wout a multiple of 256; other maps are refused.
 * pad < 0 picks what the engine sets: 1 for 3x3 stride 1, 0 for 3x3 stride 2 (the zero row / column sits at the bottom / right)
 * and for 1x1, 2 for zins.
 *
 * Weights are HOST pointers in the torch layout of the module the operator belongs to:
 *   transposed = 0: weight [Cout][Cin][k][k] -- the launch is conv2d(a, weight)
 *   transposed = 1: weight [Cin][Cout][k][k] -- the launch is the data gradient of that module, conv_transpose2d(a, weight),
 *                   on the dgrad layouts with flipped taps (what setw(..., dgrad = true) picks).  bias stays per launch Cout.
 * They are packed by make_conv into all six layouts (fp32, split-bf16 records, f16 records; forward and dgrad) and released
 * when the call returns.
 *
 * Every other operand is a DEVICE pointer to contiguous fp32; null = absent.  Samples are dense ([B][...]).
 *   in [B][Cin][Hin][Win]; bias2 [B][Cout]; res [B][Cout][Hout][Wout]; out [B][Cout][Hout][Wout]
 *   prologue (mode != CM_NONE): sc, sh [Cin] (y = sc x + sh), and for the tangent / cotangent modes (3, 4) the primal
 *   prim [Cin][Hin][Win] (B = 1), mr [Cin / cpg][2] = {mean, rstd} per group, gamma [Cin], tst [B][Cin / cpg][2] = {m1, m2} per
 *   group and tc [B][Cin][2] = the same {m1, m2} per channel -- both in their MATHEMATICAL meaning, unscaled.
 *   second operator (Cin2 > 0; the ResBlock shortcut, a 1x1 conv onto the same output): in2 [B][Cin2][Hout][Wout],
 *   w2 [Cout][Cin2] (host), bias2nd [Cout] (host) or null.
 *   norm-cotangent term (cot_d != null): out += S d - (rstd m1 + xhat rstd m2) for the GroupNorm + SiLU whose input is the
 *   output tensor: d = cot_d [B][Cout][Hout][Wout], primal cot_prim [Cout][Hout][Wout], cot_sc, cot_sh [Cout],
 *   cot_mr [Cout / cot_cpg][2], cot_tc [B][Cout][2] = {m1, m2} per channel, unscaled.
 *
 * The one convention the engine's statistics kernels add (launch_gn_tstats, launch_gn_lin_fused_finalize) and this entry point
 * reproduces: the per-channel array a low-precision kernel reads (ConvArgs::tc, ::cot_tc) holds {m1, m2} for the tangent mode
 * and {rstd m1, rstd m2} for the cotangent mode and the norm-cotangent term; the per-group array the exact-fp32 kernel reads
 * (ConvArgs::tst) is never scaled.  The {S = sc act'(sc x + sh), xhat} records of prim / cot_prim are built by launch_gn_cache.
 *
 *   pool2 = 1 (raw 3x3 stride-1 launches, even maps): the launch is conv + 2x2 sum-pool, the cotangent of the nearest-x2 up conv
 *   (ConvArgs::pool2); out [B][Cout][Hin / 2][Win / 2] (accumulate applies to it), the full-resolution intermediate is this call's.
 *   tangent statistics request (st_prim != null; mode CM_NONE launches): the launch carries the request the tangent pass attaches
 *   for the next norm over one part of a concatenation (raw {sum d, sum x d} row partials kept from the conv epilogue where
 *   the planner routes them there), x = st_prim [Cout][Hout][Wout] the primal of the output tensor, st_mr [Cout / st_cpg][2] =
 *   {mean, rstd} of that norm's groups.  st_out [2][B][Cout / st_cpg][2] receives {m1, m2} per (sample, group): [0] merged from
 *   the kept partials (all-ones bit patterns, i.e. NaN, where the launch kept none), [1] by the standalone pass over the finished tensor.
 *
 *   statistics request with a consuming norm (st_kind = 1 ST_FWD, 2 ST_TAN, 3 ST_COT; 0: the kept-partials request above): the
 *   launch carries the StatReq the engine's passes attach for the norm that consumes the output tensor, and the route is whatever
 *   plan_conv picks (epilogue partials + finalize, the split-K epilogue, the standalone kernels, both across a tail-probe split).
 *   The norm has the ENGINE's group count G = cfg.gn_groups (run_conv takes it from there): st_gamma, st_beta [Cout], st_eps, and
 *   for ST_FWD optionally st_ss_scale, st_ss_shift [Cout]; for ST_TAN / ST_COT the primal st_prim [Cout][Hout][Wout] of the output
 *   tensor and that norm's primal st_sc, st_sh [Cout], st_mr [G][2] (the {S, xhat} records of ST_COT are built by launch_gn_cache).
 *   What the statistics arena receives per sample is copied out: ST_FWD st_o_mr [B][G][2], st_o_sc, st_o_sh [B][Cout];
 *   ST_TAN / ST_COT st_o_tst [B][G][2], st_o_tc [B][Cout][2] (all-ones bit patterns where nothing was written).
 *   st_keep = 1 (ST_FWD, ST_TAN): the launch finishes one part of a concatenation; the row-tile partials it kept are copied to
 *   st_keep_out [B][Cout][keep_ntile][2] (st_keep_cap floats, fewer than were kept: -4 after the launch; keep_ntile is in the plan's
 *   closing line, 0: none kept).
 *   Refused before any launch: Cout not a multiple of G, 4 Cout + 4 G floats beyond a sample's statistics slot, Hout Wout not a
 *   multiple of 4, B beyond max_batch, ST_COT records beyond the record cache.  (Another cpg: an engine with another gn_groups.)
 *
 * in_arena = 1: `in` (and in2, prim, cot_d) are copied into the engine's padded arenas, as every inner conv sees them;
 * in_arena = 0: the kernel reads the caller's `in` (ConvArgs::in_padded = 0: the network's first conv on the user's tensor).
 *
 * plan (cap bytes, may be null) receives one line per launch and part, as planned by plan_conv:
 *   "launch=L part=P kernel=<conv_variant_name> tile=T nsplit=S B=b s0=first sample gemm=0|1 gemm_tm=M pair=0|1 Cin2=C
 *    sc_first=0|1 cot=0|1 stats=none|epi|splitk|alone|keep ntile=N\n"   (a shortcut that runs first is a plan of its own, listed first)
 *   and one closing line per plan: "stats_all=0|1 keep_ntile=N\n" (a standalone statistics pass over the whole batch follows;
 *   tiles per row of the kept partials)
 * Returns 0, or 1 when a norm-cotangent term was asked for and the planner declined it (out then holds the plain result and
 * loco_last_error says "declined"); < 0 on errors (shapes that exceed the arenas or the workspace among them). */
typedef struct loco_conv_desc {
    int32_t struct_size;
    int32_t Cin, Cout, Hin, Win, B, taps;
    int32_t stride, upsample, zins, mode, cpg;
    int32_t transposed, accumulate, in_arena, pad;
    int32_t Cin2, cot_cpg;
    float   res_scale;
    int32_t st_cpg;
    const float *weight, *bias;                                  /* host */
    const float *in, *bias2, *res;
    const float *prim, *sc, *sh, *mr, *gamma, *tst, *tc;
    const float *in2, *w2, *bias2nd;                             /* in2: device; w2, bias2nd: host */
    const float *cot_d, *cot_prim, *cot_sc, *cot_sh, *cot_mr, *cot_tc;
    float* out;
    const float *st_prim, *st_mr;                                /* tangent statistics request, see above */
    float* st_out;
    int32_t pool2;                                               /* 1: a 2x2 sum-pool follows the conv, see above */
    /* statistics request WITH a consuming norm (st_kind 1, 2, 3; see above).  All zero: none of it, the call is what it was. */
    int32_t st_kind, st_keep;
    float   st_eps;                                              /* 0: the engine's gn_eps */
    int32_t st_keep_cap;                                         /* floats st_keep_out can take */
    const float *st_gamma, *st_beta, *st_ss_scale, *st_ss_shift; /* the consuming norm, [Cout]; scale-shift optional (FWD) */
    const float *st_sc, *st_sh;                                  /* TAN / COT: the norm's primal sc, sh [Cout] (with st_prim, st_mr) */
    float *st_o_mr, *st_o_sc, *st_o_sh;                          /* FWD: [B][G][2], [B][Cout], [B][Cout] */
    float *st_o_tst, *st_o_tc;                                   /* TAN / COT: [B][G][2], [B][Cout][2] */
    float *st_keep_out;                                          /* st_keep: [B][Cout][keep_ntile][2] */
} loco_conv_desc;
int  loco_debug_conv(loco_ctx* ctx, const loco_conv_desc* desc, char* plan, int64_t cap, void* stream);

/* Test hook: ONE pass of ONE attention stage on caller-supplied tensors, through the functions the engine's passes call
 * (attn_forward / attn_tangent / attn_cotangent, xa_forward / xa_linear), route selection included
 * (tests/test_gpu_attn_oracle.py compares it with a float64 reference, tests/attn_oracle.py).
 *
 * Every operand is a DEVICE pointer to contiguous fp32 in the engine's [channel][token] layout; C = NH * CH, head h owns the
 * channels h CH ... h CH + CH - 1.  Samples / probes are dense ([B][...]).
 *
 * kind 0, the self-attention core:  P = softmax_j(scale q^T [K_text | k]),  o = [V_text | v] P^T,  scale = CH^-1/2.
 *   Lt = 0: no text keys.  Lt > 0 (a multiple of 64): kt, vt [C][Lt], L <= Lt real columns, the rest zero and masked out of the
 *   softmax; a score row is [Lt text columns | T image columns], Tk = Lt + T.
 *   pair = 1: the AttentionBlock form (the tangent may K-concatenate its two product pairs); 0: the transformer form.
 *   pass 0 forward:    reads q, k, v [B][C][T] (kt, vt); writes P [B][NH][T][Tk] and o [B][C][T].
 *   pass 1 tangent:    reads the primal q, k, v [C][T], P [NH][T][Tk], o [C][T] (B = 1) and dq, dk, dv [B][C][T]; writes out = do [B][C][T].
 *   pass 2 cotangent:  reads the primal q, k, v, P, o and go [B][C][T]; writes gq, gk, gv [B][C][T].
 *   no_workspace = 1 withholds the record workspace of the flash kernels: they then take the kernels that convert their operands
 *   themselves, as the product does when its workspace is too small.
 * kind 1, the text cross-attention:  P = softmax_l(scale q^T K_ctx),  o = V_ctx P^T  over L real context rows,
 *   Lp = 64 ceil(L / 64) padded ones: kt = K_ctx, vt = V_ctx [C][Lp], zero beyond L; k, v, Lt, pair are ignored.
 *   pass 0: reads q [B][C][T]; writes P [B][NH][T][Lp] (padding columns zero) and o [B][C][T].
 *   pass 1: reads P (B = 1) and dq [B][C][T]; writes out = do.      pass 2: reads P and go [B][C][T]; writes gq.
 *
 * P and o of the linear passes come from the caller, so each pass is one unit under test.  Scratch (per-probe score matrices, the
 * flash cotangent's delta, the record workspace, the column mask built from L) is this call's, allocated and freed per call.
 *
 * Refused with an error before any launch: T not a multiple of 64, Lt not a multiple of 64, L > Lt, CH < 1, NH or B < 1, a null
 * required operand.
 *
 * route (cap bytes, may be null) receives one line per launch, in launch order:
 *   "kernel=<name>\n"  for attn_split, flash_dma_tan|cotq|cotk, flash_tan|cotq|cotk, softmax_rows, softmax_jac, xattn_fused_fwd|lin
 *   "kernel=<name> M=m N=n K=k batch=b heads=h kcat=0|1\n"  for gemm_rec, gemm_bf16x3, gemm_f32
 * Returns 0; < 0 on errors. */
typedef struct loco_attn_desc {
    int32_t struct_size;
    int32_t kind, pass;
    int32_t T, NH, CH, B;
    int32_t Lt, L, pair, no_workspace;
    const float *q, *k, *v;
    const float *kt, *vt;
    float *P, *o;                                               /* written by pass 0, read by passes 1 and 2 */
    const float *dq, *dk, *dv;
    float* out;
    const float* go;
    float *gq, *gk, *gv;
} loco_attn_desc;
int  loco_debug_attn(loco_ctx* ctx, const loco_attn_desc* desc, char* route, int64_t cap, void* stream);

/* Test hook: ONE launch of ONE standalone GroupNorm launcher (kernels.h) on caller-supplied DEVICE tensors
 * (tests/test_gpu_stats_oracle.py compares it with the float64 reference of tests/stats_oracle.py).  Strides are in floats and the
 * caller's; scratch is the engine's reduction buffer where the launcher wants one.
 *   op 0 launch_gn_stats:              x [B][C][HW] (x_bs), gamma, beta, eps, ss_scale / ss_shift or null -> o_mr, o_sc, o_sh (o_bs)
 *   op 1 launch_gn_tstats:             kind 0 / 1 / 2, act; d (d_bs), x (x_bs, 0: broadcast), sc, sh (pbs_c), mr (pbs_g) -> o_tst, o_tc (o_bs)
 *   op 2 launch_gn_apply:              kind 0 - 5, act; d, x, base (base_bs, base_scale), sc, sh, mr, tst (t_bs), accumulate -> out (out_bs)
 *   op 3 launch_gn_cache:              x [C][HW], sc, sh, mr, act -> out [C][HW][2]
 *   op 4 launch_gn_fused_finalize:     partA [B][C][ntA][2] -> o_mr, o_sc, o_sh
 *   op 5 launch_gn_fused_finalize_cat: partA [B][C1][ntA][2], partB [B][C - C1][ntB][2] -> o_mr, o_sc, o_sh
 *   op 6 launch_gn_lin_fused_finalize: kind 2 (ST_TAN) / 3 (ST_COT); partA (C1, ntA), partB or null (then C1 = C), mr [G][2] -> o_tst, o_tc
 *   op 7 launch_ctx_groupnorm:         x = tok [HW = L][C = D], gamma, beta, eps -> out [L][D]
 * Refused before any launch: C not a multiple of G, HW not a multiple of 4 (ops 0 - 6), more than 256 channels per group (the
 * kernels expand per channel with one thread each), B G > 8192 (the reduction buffer), a kind out of the launcher's range, tile
 * counts that do not divide HW, C1 outside (0, C), one of ss_scale / ss_shift without the other, a null required operand. */
typedef struct loco_norm_desc {
    int32_t struct_size;
    int32_t op, kind, act, B, C, HW, G, C1, ntA, ntB, accumulate;
    float   eps, base_scale;
    int64_t x_bs, d_bs, base_bs, out_bs, pbs_c, pbs_g, o_bs, t_bs;
    const float *x, *d, *base, *gamma, *beta, *ss_scale, *ss_shift, *sc, *sh, *mr, *tst, *partA, *partB;
    float *o_mr, *o_sc, *o_sh, *o_tst, *o_tc, *out;
} loco_norm_desc;
int  loco_debug_norm(loco_ctx* ctx, const loco_norm_desc* desc, void* stream);

/* Test hook: ONE call of ONE strided batched GEMM launcher (kernels.h, gemm.hip / gemm_rec.hip) on caller-supplied DEVICE tensors
 * (tests/test_gpu_gemm_oracle.py compares it with the float64 reference of tests/gemm_oracle.py).
 *   op 0 launch_gemm          op 1 launch_gemm_fixed (with act: 0 none, 1 quick-GELU, 2 GELU)      op 2 launch_gemm_bf16x3
 *   op 3 launch_gemm_rec      (the workspace of gemm_rec_ws_bytes is allocated and freed by the call)
 *   op 4 launch_gemm_pair     (problem slots 0 and 1; every other op uses slot 0)
 * A problem slot is GemmArgs field by field: out(b, h, m, n) = act(alpha (A B + A2 B2) + beta C + bias[m] + colbias[n] + R), every
 * stride in floats; A2 / B2 share the row, k and head strides of A / B and have batch strides of their own; R shares C's row, column
 * and head strides and has its batch stride srb; batch2 (heads) < 1 counts as 1.  n_* is the number of floats the caller owns from
 * the pointer on.
 * Refused with an error before any launch: M, N, K or batch < 1; a null A, B or C, A2 without B2; a stride that is negative or
 * beyond 2^28; an operand whose largest addressed offset (from the dimensions and strides) is not below its n_*; act with A2
 * (launch_gemm_fixed drops the activation there); op 3 with bias, colbias or R, or with K < 256, M < 128 or N < 256 (the structural
 * part of gemm_rec_eligible -- its 4e9-MAC threshold is a performance rule and not applied); op 4 with A2 in either slot or with
 * outputs whose address ranges overlap.
 *
 * route (cap bytes, may be null) receives one line per launch, in launch order, written from the predicates the launchers
 * themselves branch on (gemm_f32_variant, gemm_pair_grouped, gemm_bf16x3_tile, gemm_rec_route):
 *   "kernel=<name> M=m N=n K=k batch=b heads=h nseg=1|2 akm=0|1 bkm=0|1 tm=t ksplit=s\n"   (akm / bkm: unit stride along m / n;
 *    tm, ksplit: 0 except for gemm_rec) for gemm_f32_64, gemm_f32_small, gemm_f32_small_pipe, gemm_f32_fixed, gemm_bf16x3_64,
 *    gemm_bf16x3_128, gemm_rec, and for gemm_f32_pair: the ONE launch of a grouped pair has one such line per problem slot;
 *   "kernel=rec_split operand=0|1|2|3 kcontig=0|1 z=count\n"  before gemm_rec, per record set (A, B, A2, B2);
 *   "kernel=gemm_rec_reduce ksplit=s\n"  after a gemm_rec with a K split.
 * Returns 0; < 0 on errors. */
typedef struct loco_gemm_prob {
    const float *A, *B, *A2, *B2, *bias, *colbias, *R;
    float* C;
    int64_t sam, sak, sab, sah;
    int64_t sbk, sbn, sbb, sbh;
    int64_t scm, scn, scb, sch;
    int64_t srb, sab2, sbb2;
    int64_t n_A, n_B, n_A2, n_B2, n_bias, n_colbias, n_R, n_C;
    int32_t M, N, K, batch, batch2;
    float   alpha, beta;
    int32_t pad_;
} loco_gemm_prob;
typedef struct loco_gemm_desc {
    int32_t struct_size;
    int32_t op, act, pad_;
    loco_gemm_prob p[2];
} loco_gemm_desc;
int  loco_debug_gemm(loco_ctx* ctx, const loco_gemm_desc* desc, char* route, int64_t cap, void* stream);

/* Test hook: ONE launch of ONE token-wise or pointwise launcher (kernels.h; xfmr.hip, misc.hip) on caller-supplied DEVICE tensors
 * (tests/test_gpu_token_oracle.py compares it with the float64 reference of tests/token_oracle.py).  Strides are in floats and the
 * caller's; null = absent.  LayerNorm and GEGLU tensors are in the engine's [channel][token] layout.
 *   op 0  launch_ln_fwd:        x [B][C][T] (in_bs), gamma, beta [C], eps -> out [B][C][T] (out_bs), out2 = stats [B][2][T] (st_bs)
 *                               = {mean, rstd} per token; out == x with out_bs == in_bs is the in-place call
 *   op 1  launch_ln_tan:        x = dx [B][C][T] (in_bs), y = the primal [C][T], stats [2][T] (B = 1), gamma -> out [B][C][T] (out_bs)
 *   op 2  launch_ln_cot:        x = gy (in_bs), y = the primal, stats, gamma, base [B][C][T] (aux_bs) or null -> out = gx (out_bs)
 *   op 3  launch_geglu:         kind 0: x = f [B][2 count] (in_bs) = [value | gate] -> out [B][count] (out_bs)
 *                               kind 1: x = df [B][2 count], y = the primal f [2 count] -> out [B][count]
 *                               kind 2: x = g [B][count], y = the primal f -> out [B][2 count] = [g gelu(gate) | g value gelu'(gate)]
 *   op 4  launch_temb:          C = ch, n = temb_ch, t, freq [ch / 2], w0 [n][ch], b0 [n], w1 [n][n], b1 [n], add [n] or null,
 *                               add_in [ch] or null, act (0 SiLU, 1 GELU), cos_first -> out [n].  t_dev (one float) non-null: the call
 *                               fills it with t (launch_set_scalar) and the kernel reads the timestep from there
 *   op 5  launch_temb_proj:     x = tact [n], w0 = w [C = cout][n], b0 = bias [cout] or null -> out [cout]
 *   op 6  launch_pool2x2_sum:   x [B][C][2 H][2 W] (in_bs) -> out [B][C][H][W] (out_bs) (+)= scale * the 2x2 sums; H, W of the OUTPUT
 *   op 7  launch_upsample2x:    x [B][C][H][W] (in_bs) -> out [B][C][2 H][2 W] (out_bs) (+)= scale * nearest; H, W of the INPUT
 *   op 8  launch_copy:          x [B][count] (in_bs) -> out [B][count] (out_bs) (+)= x
 *   op 9  launch_masked_axpby:  x = V [k][count] or null, y = dE [k][count], mask, mask2 [count] (uint8) or null, split, cv, ce -> out = U
 *   op 10 launch_cot_seed:      x = U [k][count], mask, mask2, split, cv, ce -> out = gE [k][count], out2 = gX0 [k][count] or null
 *   op 11 launch_ddim_step:     x, y = eps, base = noise or null [count]; f[0 ... 4] = c_x0_x, c_x0_e, c_next_x0, c_next_e, c_noise
 *                               -> out [count], out2 = x0_out [count] or null
 *   op 12 launch_latent_sample: x = moments [B][2 count] (mean | logvar), base = noise [B][count] or null, scale -> out = z [B][count]
 *   op 13 launch_lincomb:       src[0 ... n - 1] [count], f[0 ... n - 1] the coefficients -> out [count]; a source may be out itself
 *   op 14 launch_add:           x, y [count] -> out [count]
 * Refused before any launch: an op outside 0 ... 14; B, C, count or k < 1 where the op uses them; a negative stride; a null required
 * operand.  LayerNorm: T not a positive multiple of 16, st_bs < 2 T with B > 1, an output that overlaps an input (the in-place
 * ln_fwd excepted).  GEGLU: kind outside 0 ... 2, in_bs / out_bs (B > 1) smaller than the kind reads / writes.  temb: ch + temb_ch
 * floats beyond the 64 KiB of LDS a workgroup takes without opting in.  pool2x2 / upsample2x: H or W < 1; pool2x2: an odd in_bs or an
 * x not aligned to 8 bytes (float2 loads).  copy: count, in_bs or out_bs not a multiple of 4, or a pointer not aligned to 16 bytes
 * (float4).  lincomb: n outside 1 ... 4, a pointer not aligned to 16 bytes.  masked_axpby / cot_seed: split outside [0, k], mask2
 * without mask. */
typedef struct loco_pointwise_desc {
    int32_t struct_size;
    int32_t op, kind, act, B, C, T, H, W, n, k, accumulate, cos_first;
    float   eps, scale, t, cv, ce;
    float   f[5];
    int32_t pad_;
    int64_t count, split, in_bs, out_bs, aux_bs, st_bs;
    const float *x, *y, *stats, *gamma, *beta, *base;
    const float *freq, *w0, *b0, *w1, *b1, *add, *add_in;
    const float *src[4];
    const uint8_t *mask, *mask2;
    float *out, *out2, *t_dev;
} loco_pointwise_desc;
int  loco_debug_pointwise(loco_ctx* ctx, const loco_pointwise_desc* desc, void* stream);

/* Test hook: ONE launch of ONE attention kernel of the encoders on caller-supplied DEVICE tensors, through the launcher the
 * product's call site uses (tests/test_gpu_enc_attn_oracle.py compares it with the float64 reference of
 * tests/enc_attn_oracle.py).  No engine: every tensor is the caller's, contiguous fp32 (lens: int32); err (err_cap bytes, may be
 * null) receives the message of a refusal or a HIP error.  The call returns after the launch has finished.
 *
 * Activations are channel-major [rows][ld], head h owns the rows h hd ... h hd + hd - 1, group g the columns g nk + [0, nk).
 *   op 0  launch_enc_attn, no tables, no statistics:  qkv [3 D][ld] = q | k | v -> out [D][ld];  score (q scale) . k over the nk
 *         keys of the query's own group
 *   op 1  the same keeping the statistics:            -> out, ml [2][heads][ld] = row max | row sum of exp(score - max)
 *   op 2  the same with the tables relh, relw [heads][Tall][size] (nk = size^2): the score of key (row, col) gains
 *         relh[h][g nk + i][row] + relw[h][g nk + i][col]
 *   op 3  launch_prompt_attn, causal and scaled:      qkv [3 D][ld], nk = L, groups = n prompts -> out [D][ld];  keys j <= i
 *   op 4  launch_prompt_attn, length mask + bias:     qkv, bias_tab [heads][2 L - 1], lens [n] -> out;  keys j < lens[p], score
 *         q . k + bias_tab[h][j - i + L - 1], no scale; padded query rows are outputs
 *   op 5  launch_clipvis_attn_cot_q:   qkv, o, go [D][ld], ml (read) -> the q block of gqkv [3 D][ld], delta [heads][ld] (written)
 *   op 6  launch_clipvis_attn_cot_kv:  qkv, go, ml, delta (all read) -> the k and v blocks of gqkv
 *         P = exp((q scale) . k - m) / l,  delta_i = <go_i, o_i>,  dS = P o (go v^T - delta),  dQ = scale dS k,  dK = scale dS^T q,
 *         dV = P^T go;  nk = T, groups = n images
 *   op 7  launch_seg_attn:             qkv [3 D][ld] (D = reduce_dim), nk = T, groups = M masks -> out [D][ld]
 *   op 8  launch_sd_t2i:   q = qx [P][8][D] (rows NQ ... 7 unread), k, v [D][ld] per prompt at a stride of kbs floats (0: shared),
 *         nk = T, groups = P -> out [P][8][D], rows NQ ... 7 untouched
 *   op 9  launch_sd_i2t:   q [D][ld] per prompt at a stride of qbs floats (0: shared), k = kx, v = vx [P][8][D], nk = T, Tp >= T the
 *         padded columns -> out [P][D][ld], columns T ... Tp - 1 zero; out may be q when groups = 1
 *
 * Refused (-2) before any launch: an op outside 0 ... 9; a null required operand; a non-positive dimension; D != heads hd; relh
 * or relw together with ml, or one table without the other (ops 0 - 2); hd > 128 (ops 0 - 2, 5, 6); nk != size^2 or Tall < groups
 * nk (op 2); more than 65536 bytes of LDS by the launcher's own carve-up (ops 0 - 6, 8); L > 128 (ops 3, 4); a lens entry outside
 * [1, L] (op 4: lens is read back); a head width outside {4, 8, 16, 32, 64} or T > 2048 (op 7); hd not a power of two <= 64 or NQ
 * outside [1, 8] (ops 8, 9); ld smaller than the columns addressed (groups nk; T for op 8; Tp for op 9, and Tp < T); out == q with
 * groups > 1 (op 9).
 *
 * route (cap bytes, may be null) receives one line per launch, written from the predicates the launcher itself branches on:
 *   "kernel=enc_attn bias=0|1 keep=0|1\n"   "kernel=prompt_attn causal=0|1\n"   "kernel=clipvis_attn_cot_q chunk=64|32\n"
 *   "kernel=clipvis_attn_cot_kv chunk=64|32\n"   "kernel=seg_attn hd=<instantiation>\n"   "kernel=sd_t2i\n"   "kernel=sd_i2t\n"
 * Returns 0; -2 refused; -1 a HIP error; -4 route buffer too small. */
typedef struct loco_enc_attn_desc {
    int32_t struct_size;
    int32_t op;
    int32_t D, hd, heads, nk, groups;                           /* D: D / inner / reduce_dim / Ci; nk: nk / L / T; groups: groups / n / M / P */
    int32_t size, NQ, Tp;
    int64_t ld, Tall, kbs, qbs;
    float   scale;
    int32_t pad2_;
    const float *qkv, *relh, *relw, *bias_tab, *o, *go, *q, *k, *v;
    const int32_t* lens;
    float *out, *ml, *gqkv, *delta;
} loco_enc_attn_desc;
int  loco_debug_enc_attn(const loco_enc_attn_desc* desc, char* route, int64_t cap, char* err, int64_t err_cap, void* stream);

/* Debug / test hook: copy an internal primal activation ("down.0.block.0" ...)
 * of the last forward/primal call into dst (device), returns element count or <0. */
int64_t loco_debug_tensor(loco_ctx* ctx, const char* name, float* dst, int64_t cap, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LOCO_HIP_DIAG_H */
