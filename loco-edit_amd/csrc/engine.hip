// loco_ctx: the device side of the U-Net program (program.h / program.hip build it on the host): parameter store and
// upload, activation arenas, per-context state, the three passes (forward / tangent / cotangent) of the PMP-Jacobian
// operator, and the C ABI of include/loco_hip.h.
//
// Memory plan (HBM): the program gives every logical tensor a fixed offset in a per-sample layout; an arena holds max_batch
// samples of that layout, so all tensors share one batch stride.  Arena P holds the primal pass (B images for DDIM loops,
// B=1 cached for the Jacobian), arena T is shared by the tangent and the cotangent pass of a probe batch.
//
// Three lifetimes, three places: the Program (immutable, one per configuration, shared by a context and its forks), the
// Weights (device parameters in kernel layouts, written once by finalize_params of the root context, shared by its forks) and
// the per-context state (arenas, statistics flags, kept partials, projected prompt states), which lives in the context's own
// Tens / Op views of the program.
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "conv_plan_text.h"
#include "engine_internal.h"

using namespace loco;
using namespace loco::eng;

// The functions engine_internal.h declares are loco::eng's; what only this unit uses sits in anonymous namespaces between them.
namespace loco {
namespace eng {

int upload(loco_ctx* c, float** dst, const std::vector<float>& h) {
    if (dalloc(c, dst, h.size() ? h.size() : 1)) return -1;
    HIPCHK(c, hipMemcpy(*dst, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
    return 0;
}

namespace {
// ---------------------------------------------------------------------------
struct Pass {
    loco_ctx* c;
    hipStream_t st;
    int B;
    float* arena;      // activation arena of this pass
    float* stats;      // stats arena of this pass
    TView T(int id) const { return tview(c, arena, id); }
};

// attention products: exact fp32 MFMA in the f32 mode and for the short / small ones, split-bf16 on the bf16 matrix
// pipe for the long contractions of the low-precision modes (decoder mid attention at 4096 tokens)
// the captured forward graphs (LOCO_GRAPH=1) hold raw pointers: dropped whenever a buffer they may name is replaced
static void drop_graphs(loco_ctx* c) {
    for (auto& kv : c->fwd_graphs) {
        if (kv.second.exec) (void)hipGraphExecDestroy(kv.second.exec);
        if (kv.second.graph) (void)hipGraphDestroy(kv.second.graph);
    }
    c->fwd_graphs.clear();
}
inline unsigned char* gemm_ws_get(loco_ctx* c, size_t need, hipStream_t st) {
    const int l = c->lane;
    if (c->gemm_ws_bytes[l] >= need) return c->gemm_ws[l];
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return nullptr;
    if (c->gemm_ws[l]) {
        // a captured forward graph (LOCO_GRAPH=1) may hold this pointer: the graphs go before the buffer does;
        // the context's byte count follows the buffer it replaces
        (void)hipDeviceSynchronize();
        drop_graphs(c);
        (void)hipFree(c->gemm_ws[l]);
        c->bytes -= c->gemm_ws_bytes[l];
        c->gemm_ws[l] = nullptr; c->gemm_ws_bytes[l] = 0;
    }
    void* p = nullptr;
    if (hipMalloc(&p, need) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    c->gemm_ws[l] = static_cast<unsigned char*>(p); c->gemm_ws_bytes[l] = need; c->bytes += need;
    return c->gemm_ws[l];
}
// diag (loco_debug_attn): one line per launch of an attention stage, the counterpart of run_conv's plan_log
inline void attn_note(loco_ctx* c, const char* kernel, const GemmArgs* g = nullptr) {
    if (!c->attn_log) return;
    char line[192];
    if (g) snprintf(line, sizeof(line), "kernel=%s M=%d N=%d K=%d batch=%d heads=%d kcat=%d\n", kernel, g->M, g->N, g->K, g->batch,
                    g->batch2 > 0 ? g->batch2 : 1, g->A2 ? 1 : 0);
    else snprintf(line, sizeof(line), "kernel=%s\n", kernel);
    *c->attn_log += line;
}
inline bool attn_gemm_rec(const loco_ctx* c, const GemmArgs& g) { return c->prec >= 1 && c->gemm_lowp && gemm_rec_eligible(g); }
inline void attn_gemm_f32(loco_ctx* c, const GemmArgs& g, hipStream_t st) { attn_note(c, "gemm_f32", &g); launch_gemm(g, st); }
inline void attn_gemm(loco_ctx* c, const GemmArgs& g, hipStream_t st) {
    if (attn_gemm_rec(c, g)) {        // both operands pre-split into records, LDS-DMA fed (gemm_rec.hip)
        if (unsigned char* ws = gemm_ws_get(c, gemm_rec_ws_bytes(g), st)) { attn_note(c, "gemm_rec", &g); launch_gemm_rec(g, ws, st); return; }
    }
    if (c->prec >= 1 && c->gemm_lowp && gemm_prefers_bf16x3(g)) { attn_note(c, "gemm_bf16x3", &g); launch_gemm_bf16x3(g, st); }
    else attn_gemm_f32(c, g, st);
}
// two independent products of one pass: one launch where both are exact-fp32 launches of the small tiling (launch_gemm_pair);
// the route text has its line per product either way
inline void attn_gemm_pair(loco_ctx* c, const GemmArgs& g0, const GemmArgs& g1, hipStream_t st) {
    auto f32 = [&](const GemmArgs& g) { return !attn_gemm_rec(c, g) && !(c->prec >= 1 && c->gemm_lowp && gemm_prefers_bf16x3(g)); };
    if (!f32(g0) || !f32(g1)) { attn_gemm(c, g0, st); attn_gemm(c, g1, st); return; }
    attn_note(c, "gemm_f32", &g0); attn_note(c, "gemm_f32", &g1);
    launch_gemm_pair(g0, g1, st);
}
inline void attn_softmax_rows(loco_ctx* c, float* S, long rows, int T, hipStream_t st, int B, long bs) {
    attn_note(c, "softmax_rows"); launch_softmax_rows(S, rows, T, st, B, bs);
}
inline void attn_softmax_jac(loco_ctx* c, float* dS, const float* P, long rows, int T, float scale, hipStream_t st, int B, long bs) {
    attn_note(c, "softmax_jac"); launch_softmax_jac(dS, P, rows, T, rows, scale, st, B, bs);
}
}  // namespace

NS nstats(const loco_ctx* c, float* base, const NormP& n) {
    NS s;
    s.sc = base + n.soff; s.sh = s.sc + n.C; s.mr = s.sh + n.C; s.tst = s.mr + 2 * c->cfg.gn_groups;
    s.tc = s.tst + 2 * c->cfg.gn_groups;
    return s;
}

static void stats_standalone(loco_ctx* c, const StatReq& rq, const float* x, long xbs, int B, int HW, int s0, hipStream_t st) {
    const NormP& n = *rq.n;
    const long SB = c->prog->stats_per_sample;
    const int G = c->cfg.gn_groups;
    if (rq.kind == ST_FWD) {
        NS s = nstats(c, rq.stats + (long)s0 * SB, n);
        launch_gn_stats(x, xbs, B, n.C, HW, G, eps_of(c, n), n.gamma, n.beta, s.mr, s.sc, s.sh, SB, c->red, st, rq.ss_scale,
                        rq.ss_shift);
    } else {
        NS sp = nstats(c, c->statsP, n);
        NS stt = nstats(c, rq.stats + (long)s0 * SB, n);
        launch_gn_tstats(x, xbs, rq.prim, 0, B, n.C, HW, G, sp.sc, sp.sh, sp.mr, 0, 0, rq.kind == ST_TAN ? 0 : 1, stt.tst,
                         stt.tc, SB, c->red, st, c->cfg.act);
    }
}

// run a conv as plan_conv (conv_plan.hip) decides: split-K, kernel, tail-probe split, statistics route.
// `second`: a prepared 1x1 operator on the same output tensor (the ResBlock shortcut, `second->out == a.out`) that `a` then
// reads as its residual: K-concatenated into `a`'s kernel where the launch allows it, else run first.  Returns whether the
// norm-cotangent term asked for in a.cot_d rides in the epilogue (false: the caller applies it).
bool run_conv(loco_ctx* c, const ConvArgs& a0, int taps, hipStream_t st, const StatReq* rq, const ConvArgs* second) {
    const size_t span = (size_t)c->cfg.max_batch * c->prog->per_sample;
    auto padded = [&](const float* p) { return (p >= c->arenaP && p < c->arenaP + span) || (p >= c->arenaT && p < c->arenaT + span); };
    ConvArgs a = a0, sc;
    a.act = c->cfg.act;
    if (a.mode == CM_GN_SILU && c->cfg.act == ACT_GELU) a.mode = CM_GN_GELU;     // the forward prologue of a GELU network
    a.in_padded = padded(a.in);
    if (second) { sc = *second; sc.in_padded = padded(sc.in); }
    ConvEnv e;
    e.prec = c->prec; e.chip_share = c->chip_share; e.lanes = c->lanes_active; e.lane_s0 = c->lane_s0;
    e.partial = c->partial; e.partial_floats = c->partial_floats; e.stpart = c->stpart; e.stpart_floats = c->stpart_floats;
    e.fuse_stats = c->fuse_stats; e.fuse_lin = c->fuse_lin; e.deep1 = c->deep1; e.max_batch = c->cfg.max_batch;
    StatAsk q;
    if (rq) {
        q.kind = rq->kind; q.norm = rq->n != nullptr; q.prim = rq->prim; q.keep = rq->keep; q.keep_floats = rq->keep_floats;
        if (rq->n && rq->n->sx_off >= 0 && c->sxcache) q.sx = c->sxcache + rq->n->sx_off;
    }
    const ConvPlan p = plan_conv(e, a, taps, rq ? &q : nullptr, second ? &sc : nullptr);
    if (p.sc_first) run_conv(c, *second, 1, st);
    if (c->plan_log) conv_plan_text(p, taps, c->prec, *c->plan_log);
    if (rq && rq->kind != ST_NONE && rq->n) rq->n->ready = true;
    if (rq && rq->keep_ntile) *rq->keep_ntile = p.keep_ntile;
    const int HWo = a.Hout * a.Wout, Gn = c->cfg.gn_groups;
    const long SBs = c->prog->stats_per_sample;
    // each kernel (+ its split-K reduce) timed as its own profile record, so the per-kernel averages agree with rocprofv3's
    auto timed = [&](const char* name, double flops, const ConvArgs& y, auto&& launch) {
        loco_ctx::ProfRec r;
        if (c->prof_on) {
            r.name = name; r.flops = flops;
            r.cin = y.Cin; r.cout = y.Cout; r.h = y.Hout; r.b = y.B; r.ns = y.nsplit; r.mode = y.mode; r.taps = taps;
            r.e0 = c->next_event(); r.e1 = c->next_event();
            (void)hipEventRecord(r.e0, st);
        }
        launch();
        if (c->prof_on) { (void)hipEventRecord(r.e1, st); c->prof.push_back(r); }
    };
    for (int li = 0; li < p.nl; ++li) {
        const ConvLaunch& l = p.l[li];
        const ConvArgs& x = l.args;
        double flops = 2.0 * (x.Cin * taps + x.Cin2) * x.Cout * (double)x.Hout * x.Wout * x.B;
        if (x.zins) flops *= 0.25;     // algorithmic work of the stride-2 data gradient
        if (x.poly == 2) flops *= 4.0;    // (Hout x Wout is the pooled map: the 3x3 conv runs at full resolution)
        timed(c->prof_on ? conv_variant_name(x, taps, c->prec) : nullptr, flops, x, [&] {
            if (c->prec == 1) launch_conv_bf16x3(x, taps, st);
            else if (c->prec == 2) launch_conv_f16(x, taps, st);
            else launch_conv(x, taps, st);
        });
        if (x.nsplit > 1) {
            timed("conv_splitk_reduce", 0.0, x, [&] {
                if (l.stats != SR_SPLITK) { launch_conv_splitk_reduce(x, st); return; }
                const NormP& n = *rq->n;
                NS sp = nstats(c, c->statsP, n);
                NS so = nstats(c, rq->stats + (long)l.s0 * SBs, n);
                launch_conv_splitk_reduce_stats(x, rq->kind, Gn, eps_of(c, n), n.gamma, n.beta, so.mr, so.sc, so.sh, SBs, rq->ss_scale,
                                                rq->ss_shift, rq->prim, sp.sc, sp.sh, sp.mr, so.tst, so.tc, SBs, c->red, st);
            });
        }
        if (l.stats == SR_ALONE) stats_standalone(c, *rq, x.out, x.out_bs, x.B, HWo, l.s0, st);
        if (l.stats == SR_EPI) {
            const NormP& n = *rq->n;
            NS so = nstats(c, rq->stats + (long)l.s0 * SBs, n);
            if (rq->kind != ST_FWD) {
                NS sp = nstats(c, c->statsP, n);
                launch_gn_lin_fused_finalize(rq->kind, x.st_part, n.C, l.ntile, nullptr, 0, x.B, n.C, HWo, Gn, sp.mr, so.tst, so.tc,
                                             SBs, st);
            } else {
                launch_gn_fused_finalize(x.st_part, l.ntile, x.B, n.C, HWo, Gn, eps_of(c, n), n.gamma, n.beta, so.mr, so.sc, so.sh,
                                         SBs, rq->ss_scale, rq->ss_shift, st);
            }
        }
    }
    if (p.stats_all) stats_standalone(c, *rq, a.out, a.out_bs, a.B, HWo, 0, st);
    if (p.pool_after)      // ConvArgs::pool2 on the 3x3 route: the launches wrote pool_tmp
        launch_pool2x2_sum(a.pool_tmp, a.pool_tmp_bs, p.pool_out, p.pool_out_bs, p.pool_acc, a.B, a.Cout, a.Hout, a.Wout, st);
    return p.cot;
}

namespace {
// the norm (if any) that takes its statistics over exactly tensor `tid`
NormP* consumer_norm(loco_ctx* c, int tid) {
    const Tens& t = c->tens[tid];
    if (t.cons_op < 0) return nullptr;
    Op& op = c->ops[t.cons_op];
    return t.cons_norm == 2 ? &op.nx : &op.n1;
}
StatReq req_fwd(NormP* n, float* stats, const float* ss_scale = nullptr, const float* ss_shift = nullptr) {
    StatReq r;
    if (n) { r.kind = ST_FWD; r.n = n; r.stats = stats; r.ss_scale = ss_scale; r.ss_shift = ss_shift; }
    return r;
}
StatReq req_lin(loco_ctx* c, int kind, NormP* n, const float* prim) {       // tangent / cotangent statistics into statsT
    StatReq r;
    if (n) { r.kind = kind; r.n = n; r.stats = c->statsT; r.prim = prim; }
    return r;
}
void clear_ready(loco_ctx* c) {
    for (auto& op : c->ops) op.n1.ready = op.n2.ready = op.nx.ready = false;
    for (auto& t : c->tens) t.keep_ntile = 0;
}
// forward statistics for the consumer of tensor `tid` and / or, when `tid` is one part of a concatenation, its tile partials
StatReq req_fwd_of(loco_ctx* c, int tid, float* stats) {
    StatReq r = req_fwd(consumer_norm(c, tid), stats);
    Tens& t = c->tens[tid];
    if (t.cat_of >= 0 && t.keep) {
        r.kind = ST_FWD; r.stats = stats;
        r.keep = t.keep; r.keep_floats = t.keep_floats; r.keep_ntile = &t.keep_ntile;
    }
    return r;
}
// norm over a concatenation whose two parts both kept their producers' tile partials in this pass: finalise from those
bool cat_fused_stats(loco_ctx* c, const NormP& n, int tid, float* stats, int B, hipStream_t st) {
    const Tens& q = c->tens[tid];
    if (q.cat_a < 0 || c->prec < 1 || !c->fuse_stats) return false;
    const Tens& A = c->tens[q.cat_a];
    const Tens& Bt = c->tens[q.cat_b];
    if (A.keep_ntile <= 0 || Bt.keep_ntile <= 0) return false;
    NS s = nstats(c, stats, n);
    launch_gn_fused_finalize_cat(A.keep, A.C, A.keep_ntile, Bt.keep, Bt.keep_ntile, B, q.C, q.H * q.W, c->cfg.gn_groups,
                                 eps_of(c, n), n.gamma, n.beta, s.mr, s.sc, s.sh, c->prog->stats_per_sample, st);
    return true;
}

// the tangent group means of a norm over a concatenation whose two producers both kept their raw {sum d, sum x d} tile partials
// in this pass (run_conv, ST_TAN): finalised from those instead of a pass over the concatenation (round 6)
bool cat_fused_tstats(loco_ctx* c, const NormP& n, int tid, int B, hipStream_t st) {
    const Tens& q = c->tens[tid];
    if (q.cat_a < 0 || c->prec < 1 || !c->fuse_stats || !c->fuse_lin) return false;
    const Tens& A = c->tens[q.cat_a];
    const Tens& Bt = c->tens[q.cat_b];
    if (A.keep_ntile <= 0 || Bt.keep_ntile <= 0) return false;
    NS sp = nstats(c, c->statsP, n);
    NS stt = nstats(c, c->statsT, n);
    const size_t MB = c->cfg.max_batch;      // this lane's rows (conv_plan.hip stats_route: keep_floats / max_batch apart)
    launch_gn_lin_fused_finalize(ST_TAN, A.keep + c->lane_s0 * (A.keep_floats / MB), A.C, A.keep_ntile,
                                 Bt.keep + c->lane_s0 * (Bt.keep_floats / MB), Bt.keep_ntile, B, q.C, q.H * q.W,
                                 c->cfg.gn_groups, sp.mr, stt.tst, stt.tc, c->prog->stats_per_sample, st);
    return true;
}


// ------------------------------ text cross-attention stage of an attention block ------------------------------
// out = xmid + proj(o),  o = V_ctx P^T,  P = softmax_l(scale q^T K_ctx),  q = Wq GN(xmid); K_ctx / V_ctx [C][Lp] are the
// projected encoder states (loco_set_context), constant with respect to the image, so the tangent / cotangent only
// travel through q.  Generic GEMM + row kernels: the score rows are only Lp (<= 128) long.  (struct XA: engine_internal.h)
XA xa_of(loco_ctx* c, const Op& op, int B, hipStream_t st) {
    XA x; x.c = c; x.st = st; x.B = B;
    const Tens& t = c->tens[op.in];
    x.C = t.C; x.T = t.H * t.W; x.NH = op.heads; x.CH = x.C / x.NH; x.L = c->cfg.context_len; x.Lp = c->prog->ctx_Lp;
    x.scale = 1.0f / std::sqrt((float)x.CH);
    x.xK = op.xK; x.xV = op.xV; x.colbias = c->ctx_colbias;
    x.xs = x.ss = c->prog->per_sample;
    return x;
}
// S[b][h][i][l] = alpha * sum_c X[b][h*CH+c][i] K[h*CH+c][l]      (X: q / dq / g_o, K: K_ctx or V_ctx)
void xa_scores(const XA& x, const float* X, long x_bs, const float* K, float* S, long s_bs, float alpha, bool mask, bool fixed = false) {
    GemmArgs g; std::memset(&g, 0, sizeof(g));
    g.A = X; g.sam = 1; g.sak = x.T; g.sab = x_bs; g.sah = (long)x.CH * x.T;
    g.Bm = K; g.sbk = x.Lp; g.sbn = 1; g.sbb = 0; g.sbh = (long)x.CH * x.Lp;
    g.C = S; g.scm = x.Lp; g.scn = 1; g.scb = s_bs; g.sch = (long)x.T * x.Lp;
    g.M = x.T; g.N = x.Lp; g.K = x.CH; g.batch = x.B; g.batch2 = x.NH; g.alpha = alpha; g.beta = 0.f;
    g.colbias = mask ? x.colbias : nullptr;
    if (fixed) { attn_note(x.c, "gemm_f32_fixed", &g); launch_gemm_fixed(g, GEMM_ACT_NONE, x.st); }      // the same bits whatever B is
    else attn_gemm_f32(x.c, g, x.st);
}
// O[b][h*CH+c][i] = sum_l K[h*CH+c][l] S[b][h][i][l]              (K: V_ctx or K_ctx, S: P / dP / g_S)
void xa_values(const XA& x, const float* K, const float* S, long s_bs, float* O, long o_bs) {
    GemmArgs g; std::memset(&g, 0, sizeof(g));
    g.A = K; g.sam = x.Lp; g.sak = 1; g.sab = 0; g.sah = (long)x.CH * x.Lp;
    g.Bm = S; g.sbk = 1; g.sbn = x.Lp; g.sbb = s_bs; g.sbh = (long)x.T * x.Lp;
    g.C = O; g.scm = x.T; g.scn = 1; g.scb = o_bs; g.sch = (long)x.CH * x.T;
    g.M = x.CH; g.N = x.T; g.K = x.Lp; g.batch = x.B; g.batch2 = x.NH; g.alpha = 1.f; g.beta = 0.f;
    attn_gemm_f32(x.c, g, x.st);
}
// the three steps of one pass (scores, row operation, values) as one kernel where the shape allows (LOCO_FUSE_XATTN=0: off)
//   kind 0 forward: P = softmax(scale X^T K1) -> Pout (per sample), O = K2 P^T
//   kind 1 tangent / cotangent: R = scale P o (X^T K1 - <P, X^T K1>) with the primal P, O = K2 R^T
bool xa_fused(const XA& x, int kind, const float* X, long x_bs, const float* K1, const float* K2, float* P, long p_bs,
              float* O, long o_bs) {
    loco_ctx* c = x.c;
    if (!c->fuse_xattn || !xattn_fused_supported(x.T, x.CH, x.L, x.Lp)) return false;
    XAttnArgs a; std::memset(&a, 0, sizeof(a));
    a.T = x.T; a.NH = x.NH; a.B = x.B; a.CH = x.CH; a.L = x.L; a.Lp = x.Lp; a.fwd = kind == 0;
    a.alpha = x.scale; a.X = X; a.x_bs = x_bs; a.K1 = K1; a.K2 = K2; a.P = P; a.p_bs = p_bs; a.O = O; a.o_bs = o_bs;
    attn_note(c, kind == 0 ? "xattn_fused_fwd" : "xattn_fused_lin");
    launch_xattn_fused(a, x.st);
    return true;
}
}  // namespace
// the row step of one pass, fused where the shape allows: P = softmax(scale Xq^T K_ctx) per sample, O = V_ctx P^T
void xa_forward(const XA& x, const float* Xq, float* P, float* O) {
    if (xa_fused(x, 0, Xq, x.xs, x.xK, x.xV, P, x.ss, O, x.xs)) return;
    xa_scores(x, Xq, x.xs, x.xK, P, x.ss, x.scale, true);
    attn_softmax_rows(x.c, P, (long)x.NH * x.T, x.Lp, x.st, x.B, x.ss);
    xa_values(x, x.xV, P, x.ss, O, x.xs);
}
// ... and of the two linear passes, per probe through the softmax Jacobian at the primal P (B = 1), S = this pass's scores:
// tangent X = dq, K1 = K_ctx, K2 = V_ctx -> O = do;  cotangent X = g_o, K1 = V_ctx, K2 = K_ctx -> O = g_q
void xa_linear(const XA& x, const float* X, const float* K1, const float* K2, float* P, float* S, float* O) {
    if (xa_fused(x, 1, X, x.xs, K1, K2, P, 0, O, x.xs)) return;
    xa_scores(x, X, x.xs, K1, S, x.ss, 1.f, false);
    attn_softmax_jac(x.c, S, P, (long)x.NH * x.T, x.Lp, x.scale, x.st, x.B, x.ss);
    xa_values(x, K2, S, x.ss, O, x.xs);
}

// ------------------------------ cotangent to the prompt states ------------------------------
// The states enter a stage through K_ctx = Wk tokens^T + bk and V_ctx = Wv tokens^T + bv only, so with this pass's g_o, the primal
// P and q, and R = scale P o (g_o^T V_ctx - <P, g_o^T V_ctx>) (the row operation xa_linear just applied),
//     g_V[c][l] = sum_t g_o[c][t] P[t][l],   g_K[c][l] = sum_t q[c][t] R[t][l],   G[l][d] += sum_c Wk[c][d] g_K[c][l] + Wv[c][d] g_V[c][l]
// (the biases drop out).  The two token contractions: xattn_ctx.hip where the shape allows, else strided GEMMs over the pass's
// S buffer, which the unfused xa_linear left holding R (it is recomputed into S where xa_linear ran fused).  Every product is on a
// tiling that does not depend on the batch (launch_gemm_fixed), so a probe's row of G has the same bits wherever it stands.
// Called from the single-probe passes of loco_pmp_vjp_context only (x.B = 1, the caller's stream, no probe lanes).
// Workspace: the split-K scratch (c->partial), [2][C][W] reduced rows + the token-block partials [NH][blocks / walk][2][CH][W]:
// 2 C W (1 + blocks / walk) floats.  The launch arguments keep a probe index (strides x.xs / red_bs) for a batched G, which
// nothing runs and no test covers.
int xa_context_grad(const XA& x, const Op& op, const float* go, const float* q, const float* P, float* S) {
    loco_ctx* c = x.c;
    const int D = c->cfg.context_dim;
    const bool fused = c->fuse_xattn && xattn_fused_supported(x.T, x.CH, x.L, x.Lp);      // what xa_linear took
    const bool kern = fused && xattn_ctx_supported(x.T, x.CH, x.L, x.Lp);
    const int W = kern ? xattn_ctx_width(x.L) : x.Lp;
    const size_t avail = c->partial_floats;
    float* red = c->partial;                                      // [B][2][C][W]
    const long red_bs = 2L * x.C * W;
    if ((size_t)x.B * red_bs > avail) { c->err = "loco_pmp_vjp_context: the split-K workspace is too small for the prompt-state rows"; return -1; }
    if (kern) {
        XCtxArgs a; std::memset(&a, 0, sizeof(a));
        a.T = x.T; a.NH = x.NH; a.B = x.B; a.CH = x.CH; a.L = x.L; a.Lp = x.Lp; a.alpha = x.scale;
        a.walk = xattn_ctx_walk(x.T, x.NH, x.CH, x.L, x.B, avail);
        if (a.walk <= 0) { c->err = "loco_pmp_vjp_context: the split-K workspace is too small for the token-block partials"; return -1; }
        a.nchunk = (x.T / 64 + a.walk - 1) / a.walk;
        a.go = go; a.go_bs = x.xs; a.q = q; a.V = x.xV; a.P = P;
        a.out = red; a.out_bs = red_bs; a.part = red + (size_t)x.B * red_bs;
        attn_note(c, "xattn_ctx");
        launch_xattn_ctx(a, x.st);
    } else {
        if (fused) {      // R into S, as the unfused xa_linear leaves it
            xa_scores(x, go, x.xs, x.xV, S, x.ss, 1.f, false, true);
            attn_softmax_jac(c, S, P, (long)x.NH * x.T, x.Lp, x.scale, x.st, x.B, x.ss);
        }
        for (int w = 0; w < 2; ++w) {       // g_K = q R, g_V = g_o P: [CH][Lp] per head, contracted over the tokens
            GemmArgs g; std::memset(&g, 0, sizeof(g));
            g.A = w ? go : q; g.sam = x.T; g.sak = 1; g.sab = w ? x.xs : 0; g.sah = (long)x.CH * x.T;
            g.Bm = w ? P : S; g.sbk = x.Lp; g.sbn = 1; g.sbb = w ? 0 : x.ss; g.sbh = (long)x.T * x.Lp;
            g.C = red + (long)w * x.C * W; g.scm = W; g.scn = 1; g.scb = red_bs; g.sch = (long)x.CH * W;
            g.M = x.CH; g.N = x.Lp; g.K = x.T; g.batch = x.B; g.batch2 = x.NH; g.alpha = 1.f; g.beta = 0.f;
            attn_note(c, "gemm_f32_fixed", &g);
            launch_gemm_fixed(g, GEMM_ACT_NONE, x.st);
        }
    }
    // G[b][l][d] (+)= sum_c g_K[b][c][l] Wk[c][d] + g_V[b][c][l] Wv[c][d]
    GemmArgs g; std::memset(&g, 0, sizeof(g));
    g.A = red; g.sam = 1; g.sak = W; g.sab = red_bs;
    g.Bm = op.xkw; g.sbk = D; g.sbn = 1; g.sbb = 0;
    g.A2 = red + (long)x.C * W; g.sab2 = red_bs; g.Bm2 = op.xvw; g.sbb2 = 0;
    g.C = c->ctx_G; g.scm = D; g.scn = 1; g.scb = (long)x.L * D;
    g.M = x.L; g.N = D; g.K = x.C; g.batch = x.B; g.alpha = 1.f; g.beta = c->ctx_G_first ? 0.f : 1.f;
    attn_note(c, "gemm_f32_fixed", &g);
    launch_gemm_fixed(g, GEMM_ACT_NONE, x.st);
    c->ctx_G_first = false;
    return 0;
}

// ------------------------------ multi-head self-attention core ------------------------------
// Between the fused q/k/v map (per-head rows [q_h | k_h | v_h] of `op.qkv`) and the attended values `op.o`, for the
// AttentionBlock (OP_ATTN) and the SpatialTransformer's attn1 (OP_XFMR):  P = softmax_j(scale q^T k), o = v P^T.
// With cfg.added_kv (the DeepFloyd-IF AttentionBlock, diffusers AttnAddedKVProcessor) the keys / values are [text ; image]:
// P = softmax_j(scale q^T [K_text | k]) over Lt + T columns (the Lt - L padding columns carry -1e30), o = [V_text | v] P^T.
// K_text / V_text [C][Lt] are constants of the prompt (loco_set_context), so tangents / cotangents reach them through q only.
// Strided products on column ranges of one score matrix S [NH][T][Tk] per sample, the text columns first.  (struct Attn:
// engine_internal.h)
namespace {
// `arena` holds this pass's tensors, `bs` apart per sample: the forward's own arena, else (nullptr) the tangent / cotangent arena
Attn attn_of(loco_ctx* c, const Op& op, int B, hipStream_t st, float* arena = nullptr, long bs = 0) {
    Attn s; s.c = c; s.st = st; s.B = B;
    const Tens& t = c->tens[op.in];
    s.T = t.H * t.W; s.NH = op.heads; s.CH = t.C / op.heads; s.Lt = op.added_kv ? c->prog->ctx_Lp : 0; s.Tk = s.Lt + s.T;
    s.HS = 3L * s.CH * s.T; s.SS = (long)s.T * s.Tk; s.OS = (long)s.CH * s.T; s.KS = (long)s.CH * s.Lt;
    s.scale = 1.0f / std::sqrt((float)s.CH);
    s.pair = op.kind == OP_ATTN && !op.added_kv;
    if (!arena) { arena = c->arenaT; bs = c->prog->per_sample; }
    s.q = c->arenaP + c->tens[op.qkv].off; s.k = s.q + s.OS; s.v = s.k + s.OS;
    s.P = c->arenaP + c->tens[op.S].off; s.o = c->arenaP + c->tens[op.o].off;
    s.tq = arena + c->tens[op.qkv].off; s.tk = s.tq + s.OS; s.tv = s.tk + s.OS;
    s.tS = arena + c->tens[op.S].off; s.to = arena + c->tens[op.o].off;
    s.bq = s.bS = s.bo = bs;
    s.kt = s.Lt ? op.xK : nullptr; s.vt = s.Lt ? op.xV : nullptr; s.colbias = c->ctx_colbias;
    s.delta = c->attn_delta;
    s.ws = reinterpret_cast<unsigned char*>(c->partial); s.ws_bytes = c->partial_floats * sizeof(float);
    return s;
}
// The three products.  `text`: over the Lt text columns of S, against K_text / V_text ([CH][Lt] per head, KS apart) -- these go
// to launch_gemm (exact fp32) in every precision; else over the T image columns, against k / v-like operands ([CH][T] per
// head, HS apart) through attn_gemm.  Operands of the primal pass have batch stride 0, per-probe ones per_sample.
constexpr bool TEXT = true, IMAGE = false;
// S[b][h][i][col0 + j] (+)= alpha * sum_c X[b][h][c][i] K[.][h][c][j]  (+ X2^T K2, K-concatenated);  X: [CH][T] per head, xh apart
GemmArgs attn_scores(const Attn& s, bool text, const float* X, long xb, long xh, const float* K, long kb, float* S, long sb,
                     float alpha, float beta, bool mask = false, const float* X2 = nullptr, long xb2 = 0,
                     const float* K2 = nullptr, long kb2 = 0) {
    const int n = text ? s.Lt : s.T;
    GemmArgs g; std::memset(&g, 0, sizeof(g));
    g.A = X; g.sam = 1; g.sak = s.T; g.sab = xb; g.sah = xh;
    g.Bm = K; g.sbk = n; g.sbn = 1; g.sbb = kb; g.sbh = text ? s.KS : s.HS;
    g.C = S + (text ? 0 : s.Lt); g.scm = s.Tk; g.scn = 1; g.scb = sb; g.sch = s.SS;
    g.M = s.T; g.N = n; g.K = s.CH; g.batch = s.B; g.batch2 = s.NH; g.alpha = alpha; g.beta = beta;
    g.colbias = mask ? s.colbias : nullptr;                   // key padding of the prompt: forward text scores only
    g.A2 = X2; g.sab2 = xb2; g.Bm2 = K2; g.sbb2 = kb2;
    return g;
}
// O[b][h][c][i] (+)= sum_j V[.][h][c][j] S[b][h][i][col0 + j]  (+ V2 S2^T, K-concatenated);  O: [CH][T] per head, oh apart
GemmArgs attn_values(const Attn& s, bool text, const float* V, long vb, const float* S, long sb, float* O, long ob, long oh,
                     float beta, const float* V2 = nullptr, long vb2 = 0, const float* S2 = nullptr, long sb2 = 0) {
    const int n = text ? s.Lt : s.T, col0 = text ? 0 : s.Lt;
    GemmArgs g; std::memset(&g, 0, sizeof(g));
    g.A = V; g.sam = n; g.sak = 1; g.sab = vb; g.sah = text ? s.KS : s.HS;
    g.Bm = S + col0; g.sbk = 1; g.sbn = s.Tk; g.sbb = sb; g.sbh = s.SS;
    g.C = O; g.scm = s.T; g.scn = 1; g.scb = ob; g.sch = oh;
    g.M = s.CH; g.N = s.T; g.K = n; g.batch = s.B; g.batch2 = s.NH; g.alpha = 1.f; g.beta = beta;
    g.A2 = V2; g.sab2 = vb2; g.Bm2 = S2 ? S2 + col0 : nullptr; g.sbb2 = sb2;
    return g;
}
// G[b][h][c][j] = sum_i X[.][h][c][i] S[b][h][i][Lt + j]  over the image columns  (g_v = g_o P, g_k = q g_S);  G inside op.qkv
GemmArgs attn_keys(const Attn& s, const float* X, long xb, long xh, const float* S, long sb, float* G, long gb) {
    GemmArgs g; std::memset(&g, 0, sizeof(g));
    g.A = X; g.sam = s.T; g.sak = 1; g.sab = xb; g.sah = xh;
    g.Bm = S + s.Lt; g.sbk = s.Tk; g.sbn = 1; g.sbb = sb; g.sbh = s.SS;
    g.C = G; g.scm = s.T; g.scn = 1; g.scb = gb; g.sch = s.HS;
    g.M = s.CH; g.N = s.T; g.K = s.T; g.batch = s.B; g.batch2 = s.NH; g.alpha = 1.f; g.beta = 0.f;
    return g;
}
}  // namespace
// what the flash tangent and cotangent share: the shape, the primal q / k / v / P / o and the text keys / values; the caller
// adds its per-probe tensors
AttnFlashArgs attn_flash_args(const Attn& s) {
    AttnFlashArgs fa; std::memset(&fa, 0, sizeof(fa));
    fa.ws = s.ws; fa.ws_bytes = s.ws_bytes;      // (records of the operands: attn_flash.hip)
    fa.T = s.T; fa.NH = s.NH; fa.B = s.B; fa.CH = s.CH; fa.scale = s.scale;
    fa.q = s.q; fa.k = s.k; fa.v = s.v; fa.hs = s.HS;
    fa.P = s.P; fa.o = s.o;
    if (s.Lt) { fa.Lt = s.Lt; fa.kt = s.kt; fa.vt = s.vt; }
    return fa;
}
// diag: the kernels a flash launch takes, by the launchers' own predicate (attn_flash_dma_route)
static inline void attn_note_flash(loco_ctx* c, const AttnFlashArgs& fa, bool tan) {
    if (!c->attn_log) return;
    const bool dma = attn_flash_dma_route(fa.ws, fa.ws_bytes, attn_flash_ws_bytes(fa), attn_flash_dma_enabled());
    if (dma) attn_note(c, "attn_split");
    if (tan) attn_note(c, dma ? "flash_dma_tan" : "flash_tan");
    else { attn_note(c, dma ? "flash_dma_cotq" : "flash_cotq"); attn_note(c, dma ? "flash_dma_cotk" : "flash_cotk"); }
}
void attn_forward(const Attn& s) {      // q, k, v (s.tq, s.tk, s.tv) -> P in s.tS, o in s.to
    loco_ctx* c = s.c;
    float *q = s.tq, *k = s.tk, *v = s.tv, *S = s.tS, *o = s.to;
    if (s.Lt) attn_gemm_f32(c, attn_scores(s, TEXT, q, s.bq, s.HS, s.kt, 0, S, s.bS, s.scale, 0.f, true), s.st);
    attn_gemm(c, attn_scores(s, IMAGE, q, s.bq, s.HS, k, s.bq, S, s.bS, s.scale, 0.f), s.st);
    attn_softmax_rows(c, S, (long)s.NH * s.T, s.Tk, s.st, s.B, s.bS);
    attn_gemm(c, attn_values(s, IMAGE, v, s.bq, S, s.bS, o, s.bo, s.OS, 0.f), s.st);
    if (s.Lt) attn_gemm_f32(c, attn_values(s, TEXT, s.vt, 0, S, s.bS, o, s.bo, s.OS, 1.f), s.st);
}
void attn_tangent(const Attn& s) {      // dq, dk, dv (s.tq, s.tk, s.tv) -> do in s.to; the primal q, k, v, P, o: B = 1
    loco_ctx* c = s.c;
    const float *q = s.q, *k = s.k, *v = s.v, *SP = s.P;
    float *dq = s.tq, *dk = s.tk, *dv = s.tv, *ST = s.tS, *oT = s.to;
    if (s.flash()) {        // do from dq, dk, dv and the primal P / o in one kernel
        AttnFlashArgs fa = attn_flash_args(s);
        fa.dq = dq; fa.dk = dk; fa.dv = dv; fa.bs_d = s.bq; fa.out = oT; fa.bs_out = s.bo;
        attn_note_flash(c, fa, true);
        launch_attn_flash_tangent(fa, s.st);
        return;
    }
    // dS = dq^T k + q^T dk and do = dv P^T + v dP^T: one launch per pair (K-concatenation) where the launches
    // are latency-shaped (T <= 256: 327.7 vs 330.0 ms per headline step); at 1024 tokens two launches with
    // beta = 1 measured faster (616 vs 639 ms per tloco_if64 step)
    // -- and where the record GEMM takes the product (the decoder's 4096-token head): one write of dS instead of a write
    // and a read-modify-write (500 vs 276 + 586 us, tests/diag/gemm_rec_bench.hip)
    // The AttentionBlock without text keys only (s.pair): the others always issue two launches.
    const GemmArgs dS2 = attn_scores(s, IMAGE, dq, s.bq, s.HS, k, 0, ST, s.bS, 1.f, 0.f, false, q, 0, dk, s.bq);
    const bool kcat = s.pair && (s.T <= 256 || attn_gemm_rec(c, dS2));
    if (s.Lt) attn_gemm_f32(c, attn_scores(s, TEXT, dq, s.bq, s.HS, s.kt, 0, ST, s.bS, 1.f, 0.f), s.st);      // dS_text = dq^T K_text
    if (kcat) attn_gemm(c, dS2, s.st);                                                                  // dS = dq^T k + q^T dk
    else {
        attn_gemm(c, attn_scores(s, IMAGE, dq, s.bq, s.HS, k, 0, ST, s.bS, 1.f, 0.f), s.st);            // dS_img = dq^T k
        attn_gemm(c, attn_scores(s, IMAGE, q, 0, s.HS, dk, s.bq, ST, s.bS, 1.f, 1.f), s.st);            //        + q^T dk
    }
    attn_softmax_jac(c, ST, SP, (long)s.NH * s.T, s.Tk, s.scale, s.st, s.B, s.bS);
    if (kcat) attn_gemm(c, attn_values(s, IMAGE, dv, s.bq, SP, 0, oT, s.bo, s.OS, 0.f, v, 0, ST, s.bS), s.st);   // do = dv P^T + v dP^T
    else {
        attn_gemm(c, attn_values(s, IMAGE, dv, s.bq, SP, 0, oT, s.bo, s.OS, 0.f), s.st);                // do = dv P_img^T
        attn_gemm(c, attn_values(s, IMAGE, v, 0, ST, s.bS, oT, s.bo, s.OS, 1.f), s.st);                 //    + v dP_img^T
    }
    if (s.Lt) attn_gemm_f32(c, attn_values(s, TEXT, s.vt, 0, ST, s.bS, oT, s.bo, s.OS, 1.f), s.st);     //    + V_text dP_text^T
}
void attn_cotangent(const Attn& s) {    // g_o in s.to -> g_q, g_k, g_v in s.tq, s.tk, s.tv
    loco_ctx* c = s.c;
    const float *q = s.q, *k = s.k, *v = s.v, *SP = s.P;
    float *gq = s.tq, *gk = s.tk, *gv = s.tv, *SG = s.tS, *oG = s.to;
    if (s.flash()) {        // g_q, g_k, g_v from g_o and the primal q / k / v / P / o
        AttnFlashArgs fa = attn_flash_args(s);
        fa.go = oG; fa.bs_go = s.bo; fa.gq = gq; fa.gk = gk; fa.gv = gv; fa.bs_g = s.bq; fa.delta = s.delta;
        attn_note_flash(c, fa, false);
        launch_attn_flash_cotangent(fa, s.st);
        return;
    }
    if (!s.Lt) {            // g_v, g_P depend on g_o alone and g_q, g_k on g_S alone: one launch per pair where the launches are small
        attn_gemm_pair(c, attn_keys(s, oG, s.bo, s.OS, SP, 0, gv, s.bq),                                // g_v = g_o P
                       attn_scores(s, IMAGE, oG, s.bo, s.OS, v, 0, SG, s.bS, 1.f, 0.f), s.st);          // g_P = g_o^T v
        attn_softmax_jac(c, SG, SP, (long)s.NH * s.T, s.Tk, s.scale, s.st, s.B, s.bS);
        attn_gemm_pair(c, attn_values(s, IMAGE, k, 0, SG, s.bS, gq, s.bq, s.HS, 0.f),                   // g_q = k g_S^T
                       attn_keys(s, q, 0, s.HS, SG, s.bS, gk, s.bq), s.st);                             // g_k = q g_S
        return;
    }
    attn_gemm(c, attn_keys(s, oG, s.bo, s.OS, SP, 0, gv, s.bq), s.st);                                  // g_v = g_o P_img
    if (s.Lt) attn_gemm_f32(c, attn_scores(s, TEXT, oG, s.bo, s.OS, s.vt, 0, SG, s.bS, 1.f, 0.f), s.st);      // g_P_text = g_o^T V_text
    attn_gemm(c, attn_scores(s, IMAGE, oG, s.bo, s.OS, v, 0, SG, s.bS, 1.f, 0.f), s.st);                // g_P_img = g_o^T v
    attn_softmax_jac(c, SG, SP, (long)s.NH * s.T, s.Tk, s.scale, s.st, s.B, s.bS);
    attn_gemm(c, attn_values(s, IMAGE, k, 0, SG, s.bS, gq, s.bq, s.HS, 0.f), s.st);                     // g_q = k g_S_img^T
    if (s.Lt) attn_gemm_f32(c, attn_values(s, TEXT, s.kt, 0, SG, s.bS, gq, s.bq, s.HS, 1.f), s.st);     //     + K_text g_S_text^T
    attn_gemm(c, attn_keys(s, q, 0, s.HS, SG, s.bS, gk, s.bq), s.st);                                   // g_k = q g_S_img
}

}  // namespace eng
}  // namespace loco

namespace {

// y[Cout][T] (+ bias, + residual) = W x[Cin][T] as a 1x1 conv; dgrad: the transposed map
void lin1x1(loco_ctx* c, const ConvP& w, bool dgrad, const TView& in, const TView& out, int B, hipStream_t st,
            const float* bias = nullptr, const float* res = nullptr, const StatReq* rq = nullptr) {
    ConvArgs a = conv_args(in, w, dgrad, out, B, 1);
    a.bias = bias; a.res = res; a.res_bs = res ? out.bs : 0;
    run_conv(c, a, 1, st, rq);
}

// Statistics unless a producer already delivered them: the conv that finished tensor `tid` may have carried the request of the
// norm that consumes it (StatReq -> ready); else, `cat`, the kept partials of a concatenation's two parts may serve; else the
// standalone pass over the tensor.  Either way the flag is spent.
void need_fwd_stats(const Pass& p, NormP& n, int tid, bool cat = false) {
    loco_ctx* c = p.c;
    if (!n.ready && !(cat && cat_fused_stats(c, n, tid, p.stats, p.B, p.st))) {
        const TView x = p.T(tid);
        NS s = nstats(c, p.stats, n);
        launch_gn_stats(x, x.bs, p.B, n.C, x.H * x.W, c->cfg.gn_groups, eps_of(c, n), n.gamma, n.beta, s.mr, s.sc, s.sh,
                        c->prog->stats_per_sample, c->red, p.st);
    }
    n.ready = false;
}

// ------------------------------ linear passes ------------------------------
// primal: arenaP/statsP with B = 1 (broadcast); tangents / cotangents: arenaT/statsT with B = k (the Pass of a linear pass)
// group means of a norm's tangent (kind 0) / cotangent (1: behind the activation, 2: plain) d at the primal x
void lin_stats(const Pass& p, const NormP& n, int kind, const TView& d, const float* x) {
    loco_ctx* c = p.c;
    NS sp = nstats(c, c->statsP, n);
    NS stt = nstats(c, p.stats, n);
    launch_gn_tstats(d, d.bs, x, 0, p.B, n.C, d.H * d.W, c->cfg.gn_groups, sp.sc, sp.sh, sp.mr, 0, 0, kind, stt.tst,
                     stt.tc, c->prog->stats_per_sample, c->red, p.st, kind ? c->cfg.act : 0);
}
void need_tan_stats(const Pass& p, NormP& n, int tid, bool cat = false) {      // of the tangent of tensor `tid`
    loco_ctx* c = p.c;
    if (!n.ready && !(cat && cat_fused_tstats(c, n, tid, p.B, p.st))) lin_stats(p, n, 0, p.T(tid), tview(c, c->arenaP, tid));
    n.ready = false;
}
void need_cot_stats(const Pass& p, NormP& n, const TView& d, const float* x) {
    if (!n.ready) lin_stats(p, n, 1, d, x);
    n.ready = false;
}
// The linearised GroupNorm (launch_gn_apply kinds 1 / 5: tangent without / with the activation, 2 / 3: cotangent with / without)
// of the differential d at the primal x: out (+)= [base_scale * base +] norm'(x) d, from the primal statistics and the means
// lin_stats (or a conv epilogue) left in the pass's stats arena
void gn_lin_apply(const Pass& p, const NormP& n, int kind, const TView& d, const float* x, const float* base, float* out,
                  int accumulate = 0, float base_scale = 1.0f) {
    loco_ctx* c = p.c;
    NS sp = nstats(c, c->statsP, n);
    NS stt = nstats(c, p.stats, n);
    launch_gn_apply(kind, d, d.bs, x, 0, base, base ? d.bs : 0, out, d.bs, accumulate, p.B, d.C, d.H * d.W, c->cfg.gn_groups,
                    sp.sc, sp.sh, sp.mr, 0, 0, stt.tst, c->prog->stats_per_sample, p.st, kind == 2 || kind == 5 ? c->cfg.act : 0,
                    base_scale);
}
void set_tan(loco_ctx* c, ConvArgs& a, const NormP& n, const float* prim) {
    NS sp = nstats(c, c->statsP, n);
    NS stt = nstats(c, c->statsT, n);
    a.mode = CM_TAN_SILU; a.prim = prim; a.prim_bs = 0;
    a.sc = sp.sc; a.sh = sp.sh; a.scsh_bs = 0; a.mr = sp.mr; a.mr_bs = 0; a.gamma_ = n.gamma;
    a.tst = stt.tst; a.tst_bs = c->prog->stats_per_sample; a.cpg = n.C / c->cfg.gn_groups;
    a.tc = stt.tc; a.tc_bs = c->prog->stats_per_sample;
    a.sx = (n.sx_off >= 0 && c->sxcache) ? c->sxcache + n.sx_off : nullptr;
}

constexpr size_t RED_BYTES = (size_t)4 << 20;   // reduction scratch (GN partial sums)

// ------------------------------ forward ------------------------------------
// `op_hi` >= 0: stop after that op (the encoder half of loco_unet_get_h and of the encoder tap's primal).  `dh` [B][n_h]: added to
// the tap tensor h as the tap op writes it -- the op is an identity-shortcut ResBlock, out = conv2(..) + in, so conv2 takes
// in + dh (staged in the block's cotangent scratch a1, idle in a forward pass) as its residual and the statistics its epilogue
// delivers or keeps for the norm over cat([h, skip]) are those of the modified h, on the launch list of the plain forward.
int forward_pass(loco_ctx* c, const float* x, float t, int B, float* arena, float* stats, hipStream_t st,
                 const float* t_ptr = nullptr, int op_hi = -1, const float* dh = nullptr) {
    const loco_unet_cfg& cfg = c->cfg;
    const Pass p{c, st, B, arena, stats};
    const long PS = c->prog->per_sample, SB = c->prog->stats_per_sample;
    auto T = [&](int id) { return p.T(id); };
    const TView xv = tview_in(x, c->prog->n_in, cfg.in_channels, cfg.resolution, cfg.resolution);      // the network input
    clear_ready(c);
    auto next_fwd = [&](int tid) { return req_fwd_of(c, tid, stats); };   // forward statistics for the consumer of `tid` (+ kept partials of a concatenation part)
    auto gn_prologue = [&](ConvArgs& a, int mode, const NS& s) { a.mode = mode; a.sc = s.sc; a.sh = s.sh; a.scsh_bs = SB; };
    if (cfg.arch < 2) {
        launch_temb(t, cfg.ch, cfg.ch * 4, c->wts->freq, c->wts->td0w, c->wts->td0b, c->wts->td1w, c->wts->td1b, c->tact, st, cfg.arch == 1,
                    c->has_cond ? c->cond_add : nullptr, t_ptr, cfg.act, c->has_tcond ? c->cond_in : nullptr);
        launch_temb_proj(c->tact, cfg.ch * 4, c->wts->tp_w, c->wts->tp_b, (int)c->wts->tproj_total, c->tproj, st);
    }
    const int op_end = op_hi >= 0 ? op_hi : (int)c->ops.size() - 1;
    for (int oi = 0; oi <= op_end; ++oi) {
        Op& op = c->ops[oi];
        const Tens& to = c->tens[op.out];
        switch (op.kind) {
            case OP_CONV_IN: case OP_CONV: {
                ConvArgs a = conv_args(op.kind == OP_CONV_IN ? xv : T(op.in), op.conv, false, T(op.out), B, op.ksize);
                a.bias = op.conv.bias;
                const StatReq rq = next_fwd(op.out);
                run_conv(c, a, op.ksize == 1 ? 1 : 9, st, &rq);
                break;
            }
            case OP_RES: {
                const Tens& ti = c->tens[op.in];
                need_fwd_stats(p, op.n1, op.in, true);
                NS s1 = nstats(c, stats, op.n1);
                if (op.updown == 1) {
                    // h = conv(avg_pool(silu(gn(x)))), x' = avg_pool(x)      (unet.py:198-200, 239-244)
                    launch_gn_apply(4, nullptr, 0, T(op.in), PS, nullptr, 0, T(op.a1), PS, 0, B, ti.C, ti.H * ti.W,
                                    cfg.gn_groups, s1.sc, s1.sh, s1.mr, SB, SB, nullptr, 0, st, cfg.act);
                    launch_pool2x2_sum(T(op.a1), PS, T(op.ap), PS, 0, B, ti.C, to.H, to.W, st, 0.25f);
                    launch_pool2x2_sum(T(op.in), PS, T(op.xu), PS, 0, B, ti.C, to.H, to.W, st, 0.25f);
                } else if (op.updown == 2) {
                    launch_upsample2x(T(op.in), PS, T(op.xu), PS, 0, 1.0f, B, ti.C, ti.H, ti.W, st);
                }
                // conv1 of a down block runs on the pooled activation op.ap, at the output resolution; else norm + activation (and
                // the nearest x2 of an up block) are its prologue on the block's input
                ConvArgs a = conv_args(op.updown == 1 ? T(op.ap) : T(op.in), op.c1, false, T(op.h1), B, 3);
                a.bias = op.c1.bias;
                if (!op.scale_shift && op.has_temb) { a.bias2 = c->tproj + op.tproj_off; a.bias2_bs = 0; }
                if (op.updown != 1) { gn_prologue(a, CM_GN_SILU, s1); a.upsample = op.updown == 2; }
                {   // conv1 also delivers norm2's statistics of its output (scale-shift folded in for the ADM blocks)
                    const float* ssc = op.scale_shift ? c->tproj + op.tproj_off : nullptr;
                    const StatReq rq2 = req_fwd(&op.n2, stats, ssc, ssc ? ssc + to.C : nullptr);
                    run_conv(c, a, 9, st, &rq2);
                    op.n2.ready = false;
                }
                TView xin = op.updown ? T(op.xu) : T(op.in);              // shortcut input after x_upd, at the output resolution
                if (dh && oi == c->prog->h_last_op) {                     // h + dh: (xin + dh / res_scale + conv2) * res_scale
                    launch_add_rows(xin, PS, dh, c->prog->n_h, 1.f / c->prog->res_scale, T(op.a1), PS, B, c->prog->n_h, st);
                    xin = T(op.a1);
                }
                ConvArgs n{};                                             // the 1x1 shortcut (diffusion.py:887-912), if any
                if (op.has_nin) { n = conv_args(xin, op.nin, false, T(op.out), B, 1); n.bias = op.nin.bias; }
                ConvArgs b = conv_args(T(op.h1), op.c2, false, T(op.out), B, 3);
                b.bias = op.c2.bias; b.res = xin; b.res_bs = PS;
                b.res_scale = op.has_nin ? 1.f : c->prog->res_scale;        // (shortcut + h) * res_scale: c2 / nin carry it in their weights
                gn_prologue(b, CM_GN_SILU, nstats(c, stats, op.n2));
                const StatReq rq = next_fwd(op.out);
                run_conv(c, b, 9, st, &rq, op.has_nin ? &n : nullptr);     // shortcut K-concatenated, or run first as the residual
                break;
            }
            case OP_ATTN: {
                const int so = op.has_x ? op.xmid : op.out;       // output tensor of the self-attention stage
                need_fwd_stats(p, op.n1, op.in);
                ConvArgs a = conv_args(T(op.in), op.qkvc, false, T(op.qkv), B, 1);
                a.bias = op.qkvc.bias;
                gn_prologue(a, CM_GN, nstats(c, stats, op.n1));
                run_conv(c, a, 1, st);
                // per head h: q = qkv[h*3*CH ...], k = +CH, v = +2CH channels (QKVAttentionLegacy, unet.py:346;
                // with one head this is the [q|k|v] stacking of the fused DDPM projection)
                if (op.added_kv && !c->has_ctx) { c->err = "this architecture attends over the prompt's states: call loco_set_context first"; return -1; }
                attn_forward(attn_of(c, op, B, st, arena, PS));
                {
                    const StatReq rq = next_fwd(so);
                    lin1x1(c, op.proj, false, T(op.o), T(so), B, st, op.proj.bias, T(op.in), &rq);
                }
                if (op.has_x) {
                    if (!c->has_ctx) { c->err = "this architecture has cross-attention stages: call loco_set_context first"; return -1; }
                    const XA x = xa_of(c, op, B, st);
                    need_fwd_stats(p, op.nx, op.xmid);
                    ConvArgs qa = conv_args(T(op.xmid), op.xqc, false, T(op.xq), B, 1);
                    qa.bias = op.xqc.bias;
                    gn_prologue(qa, CM_GN, nstats(c, stats, op.nx));
                    run_conv(c, qa, 1, st);
                    xa_forward(x, T(op.xq), T(op.xS), T(op.xo));
                    const StatReq rqx = next_fwd(op.out);
                    lin1x1(c, op.xproj, false, T(op.xo), T(op.out), B, st, op.xproj.bias, T(op.xmid), &rqx);
                }
                break;
            }
            case OP_XFMR: {      // latent-diffusion SpatialTransformer (oracle/loco_oracle.py _ldm_spatial_transformer)
                if (!c->has_ctx) { c->err = "this architecture has cross-attention stages: call loco_set_context first"; return -1; }
                const int C = to.C, HW = to.H * to.W;
                auto X = [&](int i) { return T(op.xt[i]); };
                need_fwd_stats(p, op.n1, op.in);
                {   // h0 = proj_in(GN(x))
                    ConvArgs a = conv_args(T(op.in), op.pj_in, false, X(X_H0), B, 1);
                    a.bias = op.pj_in.bias;
                    gn_prologue(a, CM_GN, nstats(c, stats, op.n1));
                    run_conv(c, a, 1, st);
                }
                const XA xa = xa_of(c, op, B, st);
                // x = x + attn1(LN1(x))
                launch_ln_fwd(X(X_H0), PS, B, C, HW, op.lng[0], op.lnb[0], 1e-5f, X(X_A1), PS, X(X_LN1), PS, st);
                lin1x1(c, op.qkvc, false, X(X_A1), X(X_QKV), B, st);
                attn_forward(attn_of(c, op, B, st, arena, PS));
                lin1x1(c, op.to_out1, false, X(X_O), X(X_H1), B, st, op.to_out1.bias, X(X_H0));
                // x = x + attn2(LN2(x), context)
                launch_ln_fwd(X(X_H1), PS, B, C, HW, op.lng[1], op.lnb[1], 1e-5f, X(X_A2), PS, X(X_LN2), PS, st);
                lin1x1(c, op.xqc, false, X(X_A2), X(X_XQ), B, st);
                xa_forward(xa, X(X_XQ), X(X_XS), X(X_XO));
                lin1x1(c, op.to_out2, false, X(X_XO), X(X_H2), B, st, op.to_out2.bias, X(X_H1));
                // x = x + Linear(GEGLU(LN3(x)))
                launch_ln_fwd(X(X_H2), PS, B, C, HW, op.lng[2], op.lnb[2], 1e-5f, X(X_A3), PS, X(X_LN3), PS, st);
                lin1x1(c, op.ff1, false, X(X_A3), X(X_F), B, st, op.ff1.bias);
                launch_geglu(0, X(X_F), PS, nullptr, B, 4L * C * HW, X(X_GG), PS, st);
                lin1x1(c, op.ff2, false, X(X_GG), X(X_H3), B, st, op.ff2.bias, X(X_H2));
                // out = input + proj_out(x)
                const StatReq rq = next_fwd(op.out);
                lin1x1(c, op.pj_out, false, X(X_H3), T(op.out), B, st, op.pj_out.bias, T(op.in), &rq);
                break;
            }
            case OP_DOWN: case OP_UP: {
                ConvArgs a = conv_args(T(op.in), op.conv, false, T(op.out), B, 3);
                a.bias = op.conv.bias;
                if (op.kind == OP_DOWN) { a.stride = 2; a.pad = op.sym_down ? 1 : 0; } else { a.upsample = 1; }
                const StatReq rq = next_fwd(op.out);
                run_conv(c, a, 9, st, &rq);
                break;
            }
            case OP_OUT: {
                need_fwd_stats(p, op.n1, op.in);
                ConvArgs a = conv_args(T(op.in), op.conv, false, T(op.out), B, 3);
                a.bias = op.conv.bias;
                gn_prologue(a, CM_GN_SILU, nstats(c, stats, op.n1));
                run_conv(c, a, 9, st);
                break;
            }
        }
    }
    return 0;
}

// ------------------------------ tangent ------------------------------------
// ops op_lo..op_hi (op_hi < 0: the last).  A pass that starts behind the encoder half (op_lo > 0: the decoder tap) finds the
// tangent of h and of the skip tensors in arena T (loco_pmp_jvp puts them there); V is not read.
int tangent_pass(loco_ctx* c, const float* V, int B, hipStream_t st, int op_lo = 0, int op_hi = -1) {
    const loco_unet_cfg& cfg = c->cfg;
    const long PS = c->prog->per_sample;
    const Pass p{c, st, B, c->arenaT, c->statsT};
    auto TP = [&](int id) { return tview(c, c->arenaP, id); };   // primal
    auto TT = [&](int id) { return p.T(id); };                   // tangent
    const TView Vv = tview_in(V, c->prog->n_in, cfg.in_channels, cfg.resolution, cfg.resolution);      // of the network input
    clear_ready(c);
    // tangent group means for the norm that consumes tensor `tid`, delivered with the conv that finishes it
    // (+ the kept raw partials of a concatenation part: the up-path norm over torch.cat([h, skip]) is finalised from both parts')
    auto next_tan = [&](int tid) {
        StatReq r = req_lin(c, ST_TAN, consumer_norm(c, tid), TP(tid));
        Tens& t = c->tens[tid];
        if (t.cat_of >= 0 && t.keep && c->fuse_lin) {
            r.kind = ST_TAN; r.stats = c->statsT; r.prim = TP(tid);
            r.keep = t.keep; r.keep_floats = t.keep_floats; r.keep_ntile = &t.keep_ntile;
        }
        return r;
    };
    const int op_end = op_hi >= 0 ? op_hi : (int)c->ops.size() - 1;
    for (int oi = op_lo; oi <= op_end; ++oi) {
        Op& op = c->ops[oi];
        const Tens& to = c->tens[op.out];
        switch (op.kind) {
            case OP_CONV_IN: case OP_CONV: {
                const ConvArgs a = conv_args(op.kind == OP_CONV_IN ? Vv : TT(op.in), op.conv, false, TT(op.out), B, op.ksize);
                const StatReq rq = next_tan(op.out);
                run_conv(c, a, op.ksize == 1 ? 1 : 9, st, &rq);
                break;
            }
            case OP_RES: {
                const Tens& ti = c->tens[op.in];
                need_tan_stats(p, op.n1, op.in, true);
                if (op.updown == 1) {
                    gn_lin_apply(p, op.n1, 5, TT(op.in), TP(op.in), nullptr, TT(op.a1));
                    launch_pool2x2_sum(TT(op.a1), PS, TT(op.ap), PS, 0, B, ti.C, to.H, to.W, st, 0.25f);
                    launch_pool2x2_sum(TT(op.in), PS, TT(op.xu), PS, 0, B, ti.C, to.H, to.W, st, 0.25f);
                } else if (op.updown == 2) {
                    launch_upsample2x(TT(op.in), PS, TT(op.xu), PS, 0, 1.0f, B, ti.C, ti.H, ti.W, st);
                }
                // conv1 as in the forward: on the pooled op.ap at the output resolution (down block), else norm1's tangent in the staging
                ConvArgs a = conv_args(op.updown == 1 ? TT(op.ap) : TT(op.in), op.c1, false, TT(op.h1), B, 3);
                if (op.updown != 1) { set_tan(c, a, op.n1, TP(op.in)); a.upsample = op.updown == 2; }
                {
                    const StatReq rq2 = req_lin(c, ST_TAN, &op.n2, TP(op.h1));       // norm2's group means with conv1
                    run_conv(c, a, 9, st, &rq2);
                    op.n2.ready = false;
                }
                const TView xin = op.updown ? TT(op.xu) : TT(op.in);
                ConvArgs n{};
                if (op.has_nin) n = conv_args(xin, op.nin, false, TT(op.out), B, 1);
                ConvArgs b = conv_args(TT(op.h1), op.c2, false, TT(op.out), B, 3);
                b.res = xin; b.res_bs = PS;
                b.res_scale = op.has_nin ? 1.f : c->prog->res_scale;
                set_tan(c, b, op.n2, TP(op.h1));
                const StatReq rq = next_tan(op.out);
                run_conv(c, b, 9, st, &rq, op.has_nin ? &n : nullptr);
                break;
            }
            case OP_ATTN: {
                const int so = op.has_x ? op.xmid : op.out;
                need_tan_stats(p, op.n1, op.in);
                gn_lin_apply(p, op.n1, 1, TT(op.in), TP(op.in), nullptr, TT(op.hn));
                lin1x1(c, op.qkvc, false, TT(op.hn), TT(op.qkv), B, st);
                attn_tangent(attn_of(c, op, B, st));
                {
                    const StatReq rq = next_tan(so);
                    lin1x1(c, op.proj, false, TT(op.o), TT(so), B, st, nullptr, TT(op.in), &rq);
                }
                if (op.has_x) {
                    const XA x = xa_of(c, op, B, st);
                    need_tan_stats(p, op.nx, op.xmid);
                    gn_lin_apply(p, op.nx, 1, TT(op.xmid), TP(op.xmid), nullptr, TT(op.xhn));
                    lin1x1(c, op.xqc, false, TT(op.xhn), TT(op.xq), B, st);
                    xa_linear(x, TT(op.xq), op.xK, op.xV, TP(op.xS), TT(op.xS), TT(op.xo));           // dq -> do
                    const StatReq rqx = next_tan(op.out);
                    lin1x1(c, op.xproj, false, TT(op.xo), TT(op.out), B, st, nullptr, TT(op.xmid), &rqx);
                }
                break;
            }
            case OP_XFMR: {
                const int C = to.C, HW = to.H * to.W;
                auto XP = [&](int i) { return TP(op.xt[i]); };
                auto XT_ = [&](int i) { return TT(op.xt[i]); };
                need_tan_stats(p, op.n1, op.in);
                gn_lin_apply(p, op.n1, 1, TT(op.in), TP(op.in), nullptr, XT_(X_G0));
                lin1x1(c, op.pj_in, false, XT_(X_G0), XT_(X_H0), B, st);
                const XA xa = xa_of(c, op, B, st);
                launch_ln_tan(XT_(X_H0), PS, XP(X_H0), XP(X_LN1), B, C, HW, op.lng[0], XT_(X_A1), PS, st);
                lin1x1(c, op.qkvc, false, XT_(X_A1), XT_(X_QKV), B, st);
                attn_tangent(attn_of(c, op, B, st));
                lin1x1(c, op.to_out1, false, XT_(X_O), XT_(X_H1), B, st, nullptr, XT_(X_H0));
                launch_ln_tan(XT_(X_H1), PS, XP(X_H1), XP(X_LN2), B, C, HW, op.lng[1], XT_(X_A2), PS, st);
                lin1x1(c, op.xqc, false, XT_(X_A2), XT_(X_XQ), B, st);
                xa_linear(xa, XT_(X_XQ), op.xK, op.xV, XP(X_XS), XT_(X_XS), XT_(X_XO));             // dq -> do
                lin1x1(c, op.to_out2, false, XT_(X_XO), XT_(X_H2), B, st, nullptr, XT_(X_H1));
                launch_ln_tan(XT_(X_H2), PS, XP(X_H2), XP(X_LN3), B, C, HW, op.lng[2], XT_(X_A3), PS, st);
                lin1x1(c, op.ff1, false, XT_(X_A3), XT_(X_F), B, st);
                launch_geglu(1, XT_(X_F), PS, XP(X_F), B, 4L * C * HW, XT_(X_GG), PS, st);
                lin1x1(c, op.ff2, false, XT_(X_GG), XT_(X_H3), B, st, nullptr, XT_(X_H2));
                const StatReq rq = next_tan(op.out);
                lin1x1(c, op.pj_out, false, XT_(X_H3), TT(op.out), B, st, nullptr, TT(op.in), &rq);
                break;
            }
            case OP_DOWN: case OP_UP: {
                ConvArgs a = conv_args(TT(op.in), op.conv, false, TT(op.out), B, 3);
                if (op.kind == OP_DOWN) { a.stride = 2; a.pad = op.sym_down ? 1 : 0; } else { a.upsample = 1; }
                const StatReq rq = next_tan(op.out);
                run_conv(c, a, 9, st, &rq);
                break;
            }
            case OP_OUT: {
                need_tan_stats(p, op.n1, op.in);
                ConvArgs a = conv_args(TT(op.in), op.conv, false, TT(op.out), B, 3);
                set_tan(c, a, op.n1, TP(op.in));
                run_conv(c, a, 9, st);
                break;
            }
        }
    }
    return 0;
}

// ------------------------------ cotangent ----------------------------------
// ge: cotangent of eps [B][n]; result A[B][n] = conv_in^T(...) + gx0
// ops op_hi (< 0: the last) down to op_lo.  A pass that starts at the tap (op_hi = h_last_op) finds the cotangent of h and zeros in
// the skip slots in arena T; one that stops behind it (op_lo = h_last_op + 1) leaves the cotangent of h there (loco_pmp_vjp).
// Every conv here is the transposed map: its `in` view is the op's output tensor, its `out` view the op's input tensor.
int cotangent_pass(loco_ctx* c, const float* ge, const float* gx0, float* Aout, int B, hipStream_t st, int op_lo = 0,
                   int op_hi = -1) {
    const loco_unet_cfg& cfg = c->cfg;
    const long PS = c->prog->per_sample;
    const Pass p{c, st, B, c->arenaT, c->statsT};
    auto TP = [&](int id) { return tview(c, c->arenaP, id); };
    auto TG = [&](int id) { return p.T(id); };                   // cotangent of tensor id
    // the op that produces the network output takes the caller's cotangent (conv_out; the encoder's quant_conv)
    auto GO = [&](const Op& o) {
        const Tens& t = c->tens[o.out];
        return o.out == c->prog->eps_t ? tview_in(ge, c->prog->n_out, t.C, t.H, t.W) : TG(o.out);
    };
    const TView Av{Aout, c->prog->n_in, cfg.in_channels, cfg.resolution, cfg.resolution};      // the caller's result
    clear_ready(c);
    for (int oi = op_hi >= 0 ? op_hi : (int)c->ops.size() - 1; oi >= op_lo; --oi) {
        Op& op = c->ops[oi];
        const Tens& to = c->tens[op.out];
        const int acc = op.in_is_skip ? 1 : 0;      // the skip's other consumer wrote the input's cotangent first
        switch (op.kind) {
            case OP_OUT: {
                const ConvArgs a = conv_args(GO(op), op.conv, true, TG(op.a1), B, 3);
                {
                    const StatReq rq = req_lin(c, ST_COT, &op.n1, TP(op.in));        // the norm's cotangent means with the conv
                    run_conv(c, a, 9, st, &rq);
                    op.n1.ready = false;
                }
                gn_lin_apply(p, op.n1, 2, TG(op.a1), TP(op.in), nullptr, TG(op.in));
                break;
            }
            case OP_UP: {
                ConvArgs a = conv_args(TG(op.out), op.conv, true, TG(op.in), B, 3);
                // nearest^T (conv^T g): one polyphase launch where plan_conv takes it, else the conv into op.up and the pooling pass
                a.pool2 = 1; a.pool_tmp = TG(op.up); a.pool_tmp_bs = PS;
                run_conv(c, a, 9, st);
                break;
            }
            case OP_DOWN: {
                ConvArgs a = conv_args(TG(op.out), op.conv, true, TG(op.in), B, 3);
                a.zins = 1; a.pad = op.sym_down ? 1 : 2; a.accumulate = acc;
                run_conv(c, a, 9, st);
                break;
            }
            case OP_RES: {
                const Tens& ti = c->tens[op.in];
                {   // g_a2 = dgrad conv2 (g_out)  -> slot h1
                    const ConvArgs a = conv_args(TG(op.out), op.c2, true, TG(op.h1), B, 3);
                    const StatReq rq2 = req_lin(c, ST_COT, &op.n2, TP(op.h1));
                    run_conv(c, a, 9, st, &rq2);
                    op.n2.ready = false;
                }
                // dgrad conv1 of the norm2/silu cotangent of g_a2 (fused in the staging), at conv1's resolution: the input's channels
                // at the OUTPUT resolution -- g_a1 itself, or the cotangent of the pooled (op.ap) / nearest-upsampled (op.xu) activation
                ConvArgs b = conv_args(TG(op.h1), op.c1, true, TG(op.updown == 0 ? op.a1 : op.updown == 1 ? op.ap : op.xu), B, 3);
                set_tan(c, b, op.n2, TP(op.h1));
                b.mode = CM_COT_SILU;
                if (op.updown == 0) {
                    const StatReq rq1 = req_lin(c, ST_COT, &op.n1, TP(op.in));
                    run_conv(c, b, 9, st, &rq1);
                } else if (op.updown == 1) {
                    run_conv(c, b, 9, st);
                    launch_upsample2x(TG(op.ap), PS, TG(op.a1), PS, 0, 0.25f, B, ti.C, to.H, to.W, st);   // avg-pool^T
                } else {
                    run_conv(c, b, 9, st);
                    launch_pool2x2_sum(TG(op.xu), PS, TG(op.a1), PS, 0, B, ti.C, ti.H, ti.W, st);           // nearest^T
                }
                need_cot_stats(p, op.n1, TG(op.a1), TP(op.in));
                // shortcut cotangent at the block's output resolution: identity or nin^T
                bool cot_in_epilogue = false;
                if (op.has_nin) {      // (resampling blocks never change channels: no nin there)
                    ConvArgs n = conv_args(TG(op.out), op.nin, true, TG(op.in), B, 1);
                    n.accumulate = acc;
                    // g_in = nin^T g_out + norm1^T g_a1: the norm-cotangent term in the shortcut conv's epilogue instead of a
                    // read-modify-write pass of gn_apply_kernel<2> over g_in where plan_conv takes it (from norm1's {S, xhat}
                    // records and the per-channel {rstd m1, rstd m2} its cotangent statistics left)
                    if (op.updown == 0 && c->prec >= 1 && c->fuse_cot && op.n1.sx_off >= 0 && c->sxcache) {
                        n.cot_d = TG(op.a1); n.cot_d_bs = PS; n.cot_sx = c->sxcache + op.n1.sx_off;
                        n.cot_tc = nstats(c, c->statsT, op.n1).tc; n.cot_tc_bs = c->prog->stats_per_sample;
                    }
                    cot_in_epilogue = run_conv(c, n, 1, st);
                }
                if (op.updown == 0) {
                    if (cot_in_epilogue) { /* done by the shortcut conv */ }
                    else if (op.has_nin) gn_lin_apply(p, op.n1, 2, TG(op.a1), TP(op.in), nullptr, TG(op.in), 1);
                    else        // identity shortcut: g_in = res_scale * g_out + norm1^T g_a1
                        gn_lin_apply(p, op.n1, 2, TG(op.a1), TP(op.in), TG(op.out), TG(op.in), acc, c->prog->res_scale);
                } else {
                    gn_lin_apply(p, op.n1, 2, TG(op.a1), TP(op.in), nullptr, TG(op.in), acc);
                    if (op.updown == 1) launch_upsample2x(TG(op.out), PS, TG(op.in), PS, 1, 0.25f * c->prog->res_scale, B, ti.C, to.H, to.W, st);
                    else launch_pool2x2_sum(TG(op.out), PS, TG(op.in), PS, 1, B, ti.C, ti.H, ti.W, st, c->prog->res_scale);
                }
                break;
            }
            case OP_ATTN: {
                const int so = op.has_x ? op.xmid : op.out;       // output tensor of the self-attention stage
                if (op.has_x) {
                    // cotangent of the cross-attention stage: g_out -> g_xmid (residual + the q path through GN)
                    const XA x = xa_of(c, op, B, st);
                    lin1x1(c, op.xproj, true, TG(op.out), TG(op.xo), B, st);
                    xa_linear(x, TG(op.xo), op.xV, op.xK, TP(op.xS), TG(op.xS), TG(op.xq));           // g_o -> g_q
                    if (c->ctx_G && xa_context_grad(x, op, TG(op.xo), TP(op.xq), TP(op.xS), TG(op.xS))) return -1;
                    lin1x1(c, op.xqc, true, TG(op.xq), TG(op.xhn), B, st);
                    lin_stats(p, op.nx, 2, TG(op.xhn), TP(op.xmid));
                    gn_lin_apply(p, op.nx, 3, TG(op.xhn), TP(op.xmid), TG(op.out), TG(op.xmid));
                }
                lin1x1(c, op.proj, true, TG(so), TG(op.o), B, st);                  // g_o = proj^T g_out
                attn_cotangent(attn_of(c, op, B, st));      // g_q, g_k, g_v = the transposes of q^T k -> P -> v P^T
                lin1x1(c, op.qkvc, true, TG(op.qkv), TG(op.hn), B, st);             // g_hn = Wqkv^T g_qkv
                lin_stats(p, op.n1, 2, TG(op.hn), TP(op.in));
                gn_lin_apply(p, op.n1, 3, TG(op.hn), TP(op.in), TG(so), TG(op.in), acc);
                break;
            }
            case OP_XFMR: {      // transposes of the forward chain, last map first
                const int C = to.C, HW = to.H * to.W;
                auto XP = [&](int i) { return TP(op.xt[i]); };
                auto XG = [&](int i) { return TG(op.xt[i]); };
                const XA xa = xa_of(c, op, B, st);
                lin1x1(c, op.pj_out, true, TG(op.out), XG(X_H3), B, st);            // g_h3
                // feed-forward: h3 = h2 + ff2(geglu(ff1(LN3(h2))))
                lin1x1(c, op.ff2, true, XG(X_H3), XG(X_GG), B, st);
                launch_geglu(2, XG(X_GG), PS, XP(X_F), B, 4L * C * HW, XG(X_F), PS, st);
                lin1x1(c, op.ff1, true, XG(X_F), XG(X_A3), B, st);
                launch_ln_cot(XG(X_A3), PS, XP(X_H2), XP(X_LN3), B, C, HW, op.lng[2], XG(X_H3), PS, XG(X_H2), PS, st);  // g_h2
                // cross-attention: h2 = h1 + to_out2(V P^T), q = to_q(LN2(h1))
                lin1x1(c, op.to_out2, true, XG(X_H2), XG(X_XO), B, st);
                xa_linear(xa, XG(X_XO), op.xV, op.xK, XP(X_XS), XG(X_XS), XG(X_XQ));                // g_o -> g_q
                if (c->ctx_G && xa_context_grad(xa, op, XG(X_XO), XP(X_XQ), XP(X_XS), XG(X_XS))) return -1;
                lin1x1(c, op.xqc, true, XG(X_XQ), XG(X_A2), B, st);
                launch_ln_cot(XG(X_A2), PS, XP(X_H1), XP(X_LN2), B, C, HW, op.lng[1], XG(X_H2), PS, XG(X_H1), PS, st);  // g_h1
                // self-attention: h1 = h0 + to_out1(attn(qkv(LN1(h0))))
                lin1x1(c, op.to_out1, true, XG(X_H1), XG(X_O), B, st);
                attn_cotangent(attn_of(c, op, B, st));
                lin1x1(c, op.qkvc, true, XG(X_QKV), XG(X_A1), B, st);
                launch_ln_cot(XG(X_A1), PS, XP(X_H0), XP(X_LN1), B, C, HW, op.lng[0], XG(X_H1), PS, XG(X_H0), PS, st);  // g_h0
                // proj_in of GN(x), and the residual  out = x + ...
                lin1x1(c, op.pj_in, true, XG(X_H0), XG(X_G0), B, st);
                lin_stats(p, op.n1, 2, XG(X_G0), TP(op.in));
                gn_lin_apply(p, op.n1, 3, XG(X_G0), TP(op.in), TG(op.out), TG(op.in), acc);
                break;
            }
            case OP_CONV_IN: case OP_CONV: {
                const bool first = op.kind == OP_CONV_IN;      // conv_in^T writes the caller's A and adds the direct term gx0
                ConvArgs a = conv_args(GO(op), op.conv, true, first ? Av : TG(op.in), B, op.ksize);
                if (first) { a.res = gx0; a.res_bs = c->prog->n_in; }
                run_conv(c, a, op.ksize == 1 ? 1 : 9, st);
                break;
            }
        }
    }
    return 0;
}

}  // namespace

// Probe groups on two streams.  The probes of a batch are independent, so a batch of B >= 4 is cut in two groups whose
// passes are enqueued on two streams: the MFMA-bound convolutions of one group then run beside the bandwidth-bound
// statistics / apply / reduce kernels of the other, and the two groups' 256-workgroup rounds drift out of phase (the
// write burst of one group's epilogue overlaps the other's stage loops).  Lane 1 works on its own samples of the T
// arena and its own reduction / split-K scratch; the host enqueues lane 0 completely, then lane 1.
namespace {
struct LaneSwap {
    loco_ctx* c; float *arenaT, *statsT, *partial, *eps_buf, *ge, *gx0, *stpart, *attn_delta; double* red; size_t partial_floats;
    LaneSwap(loco_ctx* c_, int s0) : c(c_) {
        arenaT = c->arenaT; statsT = c->statsT; partial = c->partial; eps_buf = c->eps_buf; ge = c->ge; gx0 = c->gx0;
        // the flash cotangent indexes its delta scratch by the lane-local sample: lane 1 gets the slots of ITS samples
        attn_delta = c->attn_delta; c->attn_delta += (long)s0 * c->prog->attn_dmax;
        red = c->red; partial_floats = c->partial_floats; stpart = c->stpart; c->stpart = c->stpart2;
        c->arenaT += (long)s0 * c->prog->per_sample; c->statsT += (long)s0 * c->prog->stats_per_sample;
        c->eps_buf += (long)s0 * c->prog->n_out; c->ge += (long)s0 * c->prog->n_out; c->gx0 += (long)s0 * c->prog->n_in;
        c->partial += partial_floats / 2; c->partial_floats = partial_floats / 2;
        c->red = c->red2;
        c->lane = 1; c->lane_s0 = s0;
    }
    ~LaneSwap() {
        c->arenaT = arenaT; c->statsT = statsT; c->partial = partial; c->eps_buf = eps_buf; c->ge = ge; c->gx0 = gx0;
        c->red = red; c->partial_floats = partial_floats; c->stpart = stpart; c->attn_delta = attn_delta;
        c->lane = 0; c->lane_s0 = 0;
    }
};
template <typename F>
int run_lanes(loco_ctx* c, int B, hipStream_t st, F body) {      // body(first sample, count, stream)
    if (c->n_streams < 2 || c->prof_on || B < 4) return body(0, B, st);
    const int nA = (B + 1) / 2;
    const size_t pf = c->partial_floats;
    HIPCHK(c, hipEventRecord(c->ev_fork, st));
    c->partial_floats = pf / 2;                    // lane 0 keeps the lower half of the split-K workspace
    c->lanes_active = 2;
    int rc = body(0, nA, st);
    c->partial_floats = pf;
    if (rc) { c->lanes_active = 1; return rc; }
    hipStream_t s2 = c->st2_user ? c->st2_user : c->st2;
    if (hipStreamWaitEvent(s2, c->ev_fork, 0) != hipSuccess) { c->lanes_active = 1; c->err = "run_lanes: hipStreamWaitEvent"; return -1; }
    {
        LaneSwap sw(c, nA);
        rc = body(nA, B - nA, s2);
    }
    c->lanes_active = 1;
    if (rc) return rc;
    HIPCHK(c, hipEventRecord(c->ev_join, s2));
    HIPCHK(c, hipStreamWaitEvent(st, c->ev_join, 0));
    return 0;
}
// The skip tensors' rows of arena T (this lane's samples) set to zero, for the passes over half of the program: the decoder tangent
// pass reads them as the skips' tangents (x_t fixed: zero), the encoder cotangent pass accumulates into them (nothing wrote them first).
void tap_zero_skips(loco_ctx* c, int B, hipStream_t st) {
    for (const Tens& t : c->tens)
        if (t.cat_of >= 0 && c->tens[t.cat_of].cat_b == (int)(&t - c->tens.data()))
            launch_zero_rows(c->arenaT + t.off, c->prog->per_sample, B, (long)t.C * t.H * t.W, st);
}
// Per-context state of the program's tensors and ops, in this context's views of them: the one place that allocates it, for a
// created and a forked context alike.
int alloc_state(loco_ctx* c) {
    const Program& P = *c->prog;
    const size_t MB = (size_t)c->cfg.max_batch;
    c->tens.resize(P.tens.size());
    c->ops.resize(P.ops.size());
    for (size_t i = 0; i < P.tens.size(); ++i) {
        Tens& t = c->tens[i];
        static_cast<TensPlan&>(t) = P.tens[i];
        if (t.cat_of < 0) continue;      // kept tile partials of the concatenation parts: [B][C][<= HW / 64 tiles][2]
        t.keep_floats = MB * (size_t)t.C * ((size_t)t.H * t.W / 64 + 1) * 2;
        if (dalloc(c, &t.keep, t.keep_floats)) return -1;
    }
    for (size_t i = 0; i < P.ops.size(); ++i) {
        const OpPlan& plan = P.ops[i];
        Op& v = c->ops[i];
        static_cast<OpPlan&>(v) = plan;
        static_cast<NormPlan&>(v.n1) = plan.n1; static_cast<NormPlan&>(v.n2) = plan.n2; static_cast<NormPlan&>(v.nx) = plan.nx;
        if (!plan.has_ctx_kv()) continue;      // the projected prompt states are per context (loco_set_context)
        const size_t kv = (size_t)P.tens[plan.in].C * P.ctx_Lp;
        if (dalloc(c, &v.xK, kv) || dalloc(c, &v.xV, kv)) return -1;
    }
    return 0;
}

// Everything a context owns, for the program `prog` (its own for loco_create, the root's for loco_fork)
int create_ctx(loco_ctx* c, const loco_unet_cfg* cfg, std::shared_ptr<const Program> prog) {
    c->cfg = *cfg;
    c->prog = std::move(prog);
    const size_t MB = (size_t)cfg->max_batch;
    {   // 64-float guard bands: the vector halo loads of the convs may touch 1 float before / 3 after a tensor
        float *p0 = nullptr, *p1 = nullptr;
        if (dalloc(c, &p0, MB * c->prog->per_sample + 128) || dalloc(c, &p1, MB * c->prog->per_sample + 128)) return -1;
        c->arenaP = p0 + 64; c->arenaT = p1 + 64;
    }
    if (dalloc(c, &c->statsP, MB * c->prog->stats_per_sample) || dalloc(c, &c->statsT, MB * c->prog->stats_per_sample)) return -1;
    if (dalloc(c, &c->red, RED_BYTES) || dalloc(c, &c->red2, RED_BYTES)) return -1;
    if (alloc_state(c)) return -1;
    {   // row partials of the epilogue statistics: [B][C][pixel tiles >= HW / 64][2] of the largest tensor
        c->stpart_floats = MB * (size_t)(c->prog->max_tensor / 64 + 1) * 2;
        if (dalloc(c, &c->stpart, c->stpart_floats) || dalloc(c, &c->stpart2, c->stpart_floats)) return -1;
        const char* e = getenv("LOCO_FUSE_STATS");
        c->fuse_stats = !(e && atoi(e) == 0);
        e = getenv("LOCO_FUSE_LIN");
        c->fuse_lin = !(e && atoi(e) == 0);
        e = getenv("LOCO_FUSE_COT");
        c->fuse_cot = !(e && atoi(e) == 0) && cfg->act == ACT_SILU;     // the epilogue term is written for SiLU
        e = getenv("LOCO_DEEP1");
        c->deep1 = !(e && atoi(e) == 0);
        e = getenv("LOCO_FUSE_XATTN");
        c->fuse_xattn = !(e && atoi(e) == 0);
        const char* fa = getenv("LOCO_FLASH_ATTN");
        c->flash_attn = !(fa && atoi(fa) == 0);
        if (dalloc(c, &c->attn_delta, MB * (size_t)c->prog->attn_dmax)) return -1;
    }
    c->partial_floats = (size_t)64 << 20;   // 256 MB split-K workspace
    if (dalloc(c, &c->partial, c->partial_floats)) return -1;
    if (dalloc(c, &c->xin_buf, MB * c->prog->n_in) || dalloc(c, &c->t_dev, 4)) return -1;
    if (dalloc(c, &c->eps_buf, MB * c->prog->n_out) || dalloc(c, &c->gx0, MB * c->prog->n_in) || dalloc(c, &c->ge, MB * c->prog->n_out))
        return -1;
    c->n_ws = std::max((long)c->prog->n_in, (long)c->prog->n_h);      // (a network with a tap is a denoiser: n_out = n_in)
    if (dalloc(c, &c->tmpA, (size_t)64 * c->n_ws)) return -1;
    if (dalloc(c, &c->G, 64 * 64) || dalloc(c, &c->Q, 64 * 64) || dalloc(c, &c->W, SOLVER_W_GATE + 1)) return -1;
    {
        size_t nblk = ((size_t)c->n_ws + 255) / 256;
        if (dalloc(c, &c->gscratch, nblk * 64 * 64 + 4096)) return -1;
    }
    if (dalloc(c, &c->kry[0], KRY_STATE) || dalloc(c, &c->kry[1], KRY_STATE)) return -1;
    if (dalloc(c, &c->alphas, 256) || dalloc(c, &c->cond_add, (size_t)cfg->ch * 4)) return -1;
    if (dalloc(c, &c->cond_in, (size_t)cfg->ch)) return -1;
    {
        float2* sx0 = nullptr;
        if (dalloc(c, &sx0, (size_t)c->prog->sx_total + 64)) return -1;
        c->sxcache = sx0 + 32;
    }
    {
        const char* e = getenv("LOCO_PRECISION");
        c->prec = (e && std::string(e) == "f32") ? 0 : (e && std::string(e) == "f16") ? 2 : 1;   // default: split-bf16
    }
    if (dalloc(c, &c->mask2, (size_t)c->prog->n_out)) return -1;
    if (dalloc(c, &c->mask, (size_t)c->prog->n_out) || dalloc(c, &c->mask_idx, (size_t)c->prog->n_out) ||
        dalloc(c, &c->mask_L_dev, 4)) return -1;
    HIPCHK(c, hipEventCreate(&c->ev0));
    HIPCHK(c, hipEventCreate(&c->ev1));
    {
        const char* e = getenv("LOCO_STREAMS");
        c->n_streams = (e && atoi(e) == 2) ? 2 : 1;
        HIPCHK(c, hipStreamCreateWithFlags(&c->st2, hipStreamNonBlocking));
        HIPCHK(c, hipStreamCreateWithFlags(&c->cap_st, hipStreamNonBlocking));
        const char* gl = getenv("LOCO_GEMM_LOWP");
        if (gl) c->gemm_lowp = atoi(gl) != 0;
        const char* gr = getenv("LOCO_GRAPH");
        c->graph_on = gr && atoi(gr) == 1;
        HIPCHK(c, hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
        HIPCHK(c, hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming));
    }
    return 0;
}

}  // namespace

// =============================== C ABI =======================================
extern "C" {

const char* loco_version(void) { return "loco_hip 0.2 (gfx950; conv arithmetic: f32 MFMA | bf16x3 split-bf16 MFMA | f16 MFMA)"; }

int loco_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int loco_create(const loco_unet_cfg* cfg, loco_ctx** out) {
    if (!cfg || !out) return -2;
    loco_ctx* c = new loco_ctx();
    *out = c;
    if (cfg->struct_size != (int32_t)sizeof(loco_unet_cfg)) {
        // a binding built against another revision of include/loco_hip.h: refuse before reading past its struct
        c->err = "loco_unet_cfg.struct_size = " + std::to_string(cfg->struct_size) + ", this library expects " +
                 std::to_string(sizeof(loco_unet_cfg)) + " (binding and library built from different headers)";
        return -2;
    }
    auto prog = std::make_shared<Program>();
    if (const int rc = build_program(*cfg, prog.get(), &c->err)) return rc;
    for (const ParamDecl& d : prog->params) c->params[d.name].shape = d.shape;
    c->wts = std::make_shared<Weights>();
    c->wts->op.resize(prog->ops.size());
    return create_ctx(c, cfg, std::move(prog));
}

int loco_fork(loco_ctx* parent, int32_t max_batch, loco_ctx** out) {
    if (!parent || !out) return -2;
    *out = nullptr;
    if (finalize_params(parent)) return -3;
    loco_ctx* root = parent->weights_of ? parent->weights_of : parent;      // forks of a fork share the root's store
    loco_unet_cfg cfg = parent->cfg;
    if (max_batch > 0) cfg.max_batch = max_batch;
    loco_ctx* c = new loco_ctx();
    *out = c;
    if (const int rc = create_ctx(c, &cfg, root->prog)) return rc;
    c->wts = root->wts;
    if (bind_weights(c)) return -1;
    c->prec = parent->prec;
    c->weights_of = root;
    ++root->forks;
    return 0;
}

static void destroy_now(loco_ctx* c);
void loco_destroy(loco_ctx* c) {
    if (!c) return;
    if (c->forks > 0) { c->zombie = true; return; }      // its forks still read its parameters: freed with the last of them
    loco_ctx* root = c->weights_of;
    destroy_now(c);
    if (root && --root->forks == 0 && root->zombie) destroy_now(root);
}
static void destroy_now(loco_ctx* c) {
    for (float* p : c->owned) (void)hipFree(p);
    for (unsigned char* p : c->gemm_ws) if (p) (void)hipFree(p);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    if (c->ev_join) (void)hipEventDestroy(c->ev_join);
    if (c->st2) (void)hipStreamDestroy(c->st2);
    drop_graphs(c);
    if (c->cap_st) (void)hipStreamDestroy(c->cap_st);
    for (hipEvent_t e : c->ev_pool) (void)hipEventDestroy(e);
    delete c;
}

const char* loco_last_error(loco_ctx* c) { return c ? c->err.c_str() : "null ctx"; }

int loco_load_param(loco_ctx* c, const char* name, const void* data, const int64_t* shape, int32_t ndim,
                    int32_t is_device) {
    if (!c) return -2;
    if (c->finalized) { c->err = "parameters already finalised"; return -2; }
    auto it = c->params.find(name);
    if (it == c->params.end()) { c->err = std::string("unknown parameter: ") + name; return -3; }
    HostParam& hp = it->second;
    if ((int)hp.shape.size() != ndim) { c->err = std::string("rank mismatch for ") + name; return -3; }
    size_t cnt = 1;
    for (int i = 0; i < ndim; ++i) {
        if (hp.shape[i] != shape[i]) { c->err = std::string("shape mismatch for ") + name; return -3; }
        cnt *= (size_t)shape[i];
    }
    hp.data.resize(cnt);
    if (is_device) HIPCHK(c, hipMemcpy(hp.data.data(), data, cnt * sizeof(float), hipMemcpyDeviceToHost));
    else std::memcpy(hp.data.data(), data, cnt * sizeof(float));
    hp.loaded = true;
    return 0;
}

int loco_params_missing(loco_ctx* c) {
    if (!c) return -2;
    if (c->finalized) return 0;
    int miss = 0;
    for (const ParamDecl& d : c->prog->params)
        if (!c->params[d.name].loaded) { if (!miss) c->err = "missing parameter: " + d.name; ++miss; }
    return miss;
}

// Capture one denoiser evaluation of batch B (fixed input xin_buf, timestep read from t_dev, output in the primal
// arena) on the engine's own stream; nothing executes during the capture.
static int capture_forward(loco_ctx* c, int B, loco_ctx::FwdGraph& g) {
    HIPCHK(c, hipStreamBeginCapture(c->cap_st, hipStreamCaptureModeThreadLocal));
    int rc = forward_pass(c, c->xin_buf, 0.f, B, c->arenaP, c->statsP, c->cap_st, c->t_dev);
    hipError_t e = hipStreamEndCapture(c->cap_st, &g.graph);
    if (rc) { if (g.graph) { (void)hipGraphDestroy(g.graph); g.graph = nullptr; } return rc; }
    HIPCHK(c, e);
    HIPCHK(c, hipGraphInstantiate(&g.exec, g.graph, nullptr, nullptr, 0));
    return 0;
}

int loco_unet_forward(loco_ctx* c, const float* x, float t, int32_t B, float* eps, void* stream) {
    if (!c) return -2;
    if (B < 1 || B > c->cfg.max_batch) { c->err = "batch exceeds max_batch"; return -2; }
    if (finalize_params(c)) return -3;
    hipStream_t st = (hipStream_t)stream;
    c->primal_ok = false;
    if (c->graph_on && !c->prof_on) {
        // key: batch, conditions on/off, arithmetic (all change the launch list; the contents of cond_add / cond_in do not)
        loco_ctx::FwdGraph& g = c->fwd_graphs[(B << 4) | (c->has_tcond ? 8 : 0) | (c->has_cond ? 4 : 0) | c->prec];
        // the first evaluation of a key runs eagerly (one-time lazy setup inside the launchers), the second is captured
        if (!g.exec && g.calls++ >= 1 && capture_forward(c, B, g)) return -1;
        if (g.exec) {
            launch_copy(x, c->prog->n_in, c->xin_buf, c->prog->n_in, 0, B, c->prog->n_in, st);
            launch_set_scalar(c->t_dev, t, st);
            HIPCHK(c, hipGraphLaunch(g.exec, st));
            c->primal_B = B;
            launch_copy(c->arenaP + c->tens[c->prog->eps_t].off, c->prog->per_sample, eps, c->prog->n_out, 0, B, c->prog->n_out, st);
            HIPCHK(c, hipGetLastError());
            return 0;
        }
    }
    if (forward_pass(c, x, t, B, c->arenaP, c->statsP, st)) return -1;
    c->primal_B = B;
    launch_copy(c->arenaP + c->tens[c->prog->eps_t].off, c->prog->per_sample, eps, c->prog->n_out, 0, B, c->prog->n_out, st);
    HIPCHK(c, hipGetLastError());
    return 0;
}

// ---- h-space tap: the bottleneck tensor h of a denoiser, read, shifted, and differentiated to and from ----
static int tap_refuse(loco_ctx* c, const char* who) {
    if (c->prog->h_t >= 0) return 0;
    c->err = std::string(who) + ": this network has no h-space tap (the latent decoder and encoder, arch 2 / 3, have no U-Net bottleneck)";
    return -2;
}

int loco_h_dims(loco_ctx* c, int32_t* C_, int32_t* H, int32_t* W) {
    if (!c) return -2;
    if (tap_refuse(c, "loco_h_dims")) return -2;
    const TensPlan& t = c->prog->tens[c->prog->h_t];
    if (C_) *C_ = t.C;
    if (H) *H = t.H;
    if (W) *W = t.W;
    return 0;
}

int loco_unet_get_h(loco_ctx* c, const float* x, float t, int32_t B, float* h_out, void* stream) {
    if (!c) return -2;
    if (tap_refuse(c, "loco_unet_get_h")) return -2;
    if (B < 1 || B > c->cfg.max_batch) { c->err = "batch exceeds max_batch"; return -2; }
    if (finalize_params(c)) return -3;
    hipStream_t st = (hipStream_t)stream;
    c->primal_ok = false;
    if (forward_pass(c, x, t, B, c->arenaP, c->statsP, st, nullptr, c->prog->h_last_op)) return -1;
    c->primal_B = 0;      // no whole forward pass in the arena: the tensors behind the tap were not written
    launch_copy(c->arenaP + c->tens[c->prog->h_t].off, c->prog->per_sample, h_out, c->prog->n_h, 0, B, c->prog->n_h, st);
    HIPCHK(c, hipGetLastError());
    return 0;
}

int loco_unet_forward_dh(loco_ctx* c, const float* x, float t, int32_t B, const float* dh, float* eps, void* stream) {
    if (!c) return -2;
    if (tap_refuse(c, "loco_unet_forward_dh")) return -2;
    if (B < 1 || B > c->cfg.max_batch) { c->err = "batch exceeds max_batch"; return -2; }
    if (finalize_params(c)) return -3;
    {
        const Op& op = c->ops[c->prog->h_last_op];
        if (op.kind != OP_RES || op.has_nin || op.updown) { c->err = "loco_unet_forward_dh: the tap op is not an identity-shortcut ResBlock"; return -2; }
    }
    hipStream_t st = (hipStream_t)stream;
    c->primal_ok = false;
    if (forward_pass(c, x, t, B, c->arenaP, c->statsP, st, nullptr, -1, dh)) return -1;
    c->primal_B = B;
    launch_copy(c->arenaP + c->tens[c->prog->eps_t].off, c->prog->per_sample, eps, c->prog->n_out, 0, B, c->prog->n_out, st);
    HIPCHK(c, hipGetLastError());
    return 0;
}

static void sched_coeffs(float at, float at_next, float eta, float* s1, float* s2, float* s3, float* ce, float* cn) {
    // fp32 arithmetic in the op order of reference utils.py:362-374
    *s1 = std::sqrt(1.0f - at); *s2 = std::sqrt(at); *s3 = std::sqrt(at_next);
    *cn = 0.f;
    if (eta == 0.f) {
        *ce = std::sqrt(1.0f - at_next);
    } else {
        float sigma = std::sqrt((1.0f - at / at_next) * (1.0f - at_next) / (1.0f - at));
        *ce = std::sqrt(1.0f - at_next - eta * (sigma * sigma));
        *cn = eta * sigma;
    }
}

int loco_sched_step(loco_ctx* c, const float* x, const float* et, float at, float at_next, float eta,
                    const float* noise, int64_t count, float* x_next, float* x0_out, void* stream) {
    if (!c) return -2;
    if (eta != 0.f && !noise) { c->err = "eta != 0 needs a noise tensor"; return -2; }
    float s1, s2, s3, ce, cn;
    sched_coeffs(at, at_next, eta, &s1, &s2, &s3, &ce, &cn);
    launch_ddim_step(x, et, eta == 0.f ? nullptr : noise, x_next, x0_out, (long)count, s2, s1, s3, ce, cn,
                     (hipStream_t)stream);
    HIPCHK(c, hipGetLastError());
    return 0;
}

int loco_sched_step_asym(loco_ctx* c, const float* x, const float* et_edit, const float* et_src, float at, float at_next, int64_t count,
                         float* x_next, float* x0_out, void* stream) {
    if (!c) return -2;
    if (!x || !et_edit || !et_src || !x_next) { c->err = "loco_sched_step_asym: null argument"; return -2; }
    float s1, s2, s3, ce, cn;
    sched_coeffs(at, at_next, 0.f, &s1, &s2, &s3, &ce, &cn);
    launch_asym_step(x, et_edit, et_src, x_next, x0_out, (long)count, s2, s1, s3, ce, (hipStream_t)stream);
    HIPCHK(c, hipGetLastError());
    return 0;
}

int loco_ddim_step(loco_ctx* c, const float* x, float t, float at, float at_next, float eta, const float* noise,
                   int32_t B, float* x_next, void* stream) {
    if (!c) return -2;
    if (eta != 0.f && !noise) { c->err = "eta != 0 needs a noise tensor"; return -2; }
    if (c->prog->n_out != c->prog->n_in) { c->err = "loco_ddim_step: this network is not a denoiser (output and input sizes differ)"; return -2; }
    int rc = loco_unet_forward(c, x, t, B, c->eps_buf, stream);
    if (rc) return rc;
    return loco_sched_step(c, x, c->eps_buf, at, at_next, eta, noise, (int64_t)B * c->prog->n_in, x_next, nullptr, stream);
}

int loco_pmp_primal(loco_ctx* c, const float* x, float t, float at, const uint8_t* mask, int32_t use_et,
                    void* stream) {
    return loco_pmp_primal_tap(c, x, t, at, mask, use_et, 0, stream);
}

// the primal of every tap; `dh` (tap 2 only, may be null): the shift of the bottleneck the forward pass injects, so that every record
// behind the tap -- the arena tensors, the GroupNorm statistics, the {S, xhat} caches -- is taken at h + dh
static int pmp_primal_at(loco_ctx* c, const float* x, float t, float at, const uint8_t* mask, int32_t use_et, int32_t tap, const float* dh,
                         void* stream) {
    if (tap < 0 || tap > 2) { c->err = "loco_pmp_primal_tap: tap must be 0 (x_t -> x0 / eps), 1 (encoder, x_t -> h) or 2 (decoder, h -> eps)"; return -2; }
    if (tap && tap_refuse(c, "loco_pmp_primal_tap")) return -2;
    if (tap == 1 && mask) { c->err = "loco_pmp_primal_tap: the encoder tap (x_t -> h) takes no mask: h has no pixel positions to select"; return -2; }
    if (finalize_params(c)) return -3;
    if (dh) {
        const Op& op = c->ops[c->prog->h_last_op];
        if (op.kind != OP_RES || op.has_nin || op.updown) { c->err = "loco_pmp_primal_tap_dh: the tap op is not an identity-shortcut ResBlock"; return -2; }
    }
    if (tap == 1) use_et = 1;     // (no x0 combination at the tap: `at` and use_et are not read)
    if (c->prog->n_out != c->prog->n_in && !use_et) {
        c->err = "loco_pmp_primal: a network whose output size differs from its input has no x0 combination; use_et = 1 "
                 "(raw network Jacobian)";
        return -2;
    }
    hipStream_t st = (hipStream_t)stream;
    // the ops whose linearisation the products of this primal run: all, the encoder half, or the decoder half (whose primal needs
    // the whole forward pass)
    const int op_lo = tap == 2 ? c->prog->h_last_op + 1 : 0, op_hi = tap == 1 ? c->prog->h_last_op : (int)c->ops.size() - 1;
    if (forward_pass(c, x, t, 1, c->arenaP, c->statsP, st, nullptr, tap == 1 ? op_hi : -1, dh)) return -1;
    c->primal_B = 1;
    if (c->prec >= 1) {
        // {S, xhat} cache for the tangent / cotangent staging of the split-bf16 convs
        for (int oi = op_lo; oi <= op_hi; ++oi) {
            Op& op = c->ops[oi];
            if (op.kind != OP_RES && op.kind != OP_OUT) continue;
            const Tens& ti = c->tens[op.in];
            const int HW = ti.H * ti.W, G = c->cfg.gn_groups;
            NS s1 = nstats(c, c->statsP, op.n1);
            launch_gn_cache(c->arenaP + ti.off, op.n1.C, HW, op.n1.C / G, s1.sc, s1.sh, s1.mr,
                            c->sxcache + op.n1.sx_off, st, c->cfg.act);
            if (op.kind == OP_RES) {
                const Tens& th = c->tens[op.h1];
                NS s2 = nstats(c, c->statsP, op.n2);
                launch_gn_cache(c->arenaP + th.off, op.n2.C, th.H * th.W, op.n2.C / G, s2.sc, s2.sh, s2.mr,
                                c->sxcache + op.n2.sx_off, st, c->cfg.act);
            }
        }
    }
    if (use_et) { c->p_cv = 0.f; c->p_ce = 1.f; }
    else { c->p_cv = 1.0f / std::sqrt(at); c->p_ce = -std::sqrt(1.0f - at) / std::sqrt(at); }
    if (tap == 2) c->p_cv = 0.f;   // x0 = (x_t - sqrt(1 - at) eps) / sqrt(at): the x_t term does not depend on h
    c->tap = tap;
    c->has_mask = (mask != nullptr);
    c->has_mask2 = false;
    c->mask_L = tap == 1 ? c->prog->n_h : c->prog->n_out;      // width of the rows of J V without a mask
    if (mask) {
        // masked-latent gather list built on the device (ordered prefix-sum compaction, one launch, no host sync);
        // L is read back lazily by loco_mask_count / loco_mask_gather
        HIPCHK(c, hipMemcpyAsync(c->mask, mask, (size_t)c->prog->n_out, hipMemcpyDeviceToDevice, st));
        launch_mask_compact(c->mask, c->prog->n_out, c->mask_idx, c->mask_L_dev, st);
        c->mask_L = -1;
        c->mask_stream = st;
    }
    HIPCHK(c, hipGetLastError());
    c->primal_ok = true;
    return 0;
}

int loco_pmp_primal_tap(loco_ctx* c, const float* x, float t, float at, const uint8_t* mask, int32_t use_et, int32_t tap,
                        void* stream) {
    if (!c) return -2;
    return pmp_primal_at(c, x, t, at, mask, use_et, tap, nullptr, stream);
}

int loco_pmp_primal_tap_dh(loco_ctx* c, const float* x, float t, float at, const uint8_t* mask, int32_t use_et, const float* dh,
                           void* stream) {
    if (!c) return -2;
    if (tap_refuse(c, "loco_pmp_primal_tap_dh")) return -2;
    return pmp_primal_at(c, x, t, at, mask, use_et, 2, dh, stream);
}

int loco_pmp_primal_eps(loco_ctx* c, float* eps, void* stream) {
    if (!c) return -2;
    if (!eps) { c->err = "loco_pmp_primal_eps: eps is NULL"; return -2; }
    if (!c->primal_ok) { c->err = "loco_pmp_primal has not been called"; return -2; }
    if (c->tap == 1) { c->err = "loco_pmp_primal_eps: the encoder tap's primal stops at h, there is no network output to hand out"; return -2; }
    launch_copy(c->arenaP + c->tens[c->prog->eps_t].off, c->prog->per_sample, eps, c->prog->n_out, 0, 1, c->prog->n_out, (hipStream_t)stream);
    HIPCHK(c, hipGetLastError());
    return 0;
}

int loco_pmp_set_second_mask(loco_ctx* c, const uint8_t* mask2, int32_t from_row, void* stream) {
    if (!c) return -2;
    if (!c->primal_ok) { c->err = "loco_pmp_primal has not been called"; return -2; }
    if (!mask2) { c->has_mask2 = false; return 0; }
    if (!c->has_mask) { c->err = "a second mask needs a first one (loco_pmp_primal with mask)"; return -2; }
    if (from_row < 0) { c->err = "from_row must be >= 0"; return -2; }
    HIPCHK(c, hipMemcpyAsync(c->mask2, mask2, (size_t)c->prog->n_out, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    c->has_mask2 = true;
    c->mask2_from = from_row;
    return 0;
}

int loco_pmp_jvp(loco_ctx* c, const float* V, int32_t k, float* U, void* stream) {
    if (!c) return -2;
    if (!c->primal_ok) { c->err = "loco_pmp_primal has not been called"; return -2; }
    hipStream_t st = (hipStream_t)stream;
    const int MB = c->cfg.max_batch;
    for (int b0 = 0; b0 < k; b0 += MB) {
        int B = (k - b0 < MB) ? k - b0 : MB;
        int rc = run_lanes(c, B, st, [&](int s0, int nb, hipStream_t ls) -> int {
            const Program& P = *c->prog;
            if (c->tap == 1) {         // x_t -> h: the encoder half, then the tap tangent out of the arena
                if (tangent_pass(c, V + (long)(b0 + s0) * P.n_in, nb, ls, 0, P.h_last_op)) return -1;
                launch_copy(c->arenaT + c->tens[P.h_t].off, P.per_sample, U + (long)(b0 + s0) * P.n_h, P.n_h, 0, nb, P.n_h, ls);
                return 0;
            }
            if (c->tap == 2) {         // h -> eps with x_t, the skips and the embedding fixed: V is the tap tangent, the skips' are zero
                tap_zero_skips(c, nb, ls);
                launch_copy(V + (long)(b0 + s0) * P.n_h, P.n_h, c->arenaT + c->tens[P.h_t].off, P.per_sample, 0, nb, P.n_h, ls);
                if (tangent_pass(c, nullptr, nb, ls, P.h_last_op + 1)) return -1;
                launch_copy(c->arenaT + c->tens[P.eps_t].off, P.per_sample, c->eps_buf, P.n_out, 0, nb, P.n_out, ls);
                launch_masked_axpby(nullptr, c->eps_buf, c->has_mask ? c->mask : nullptr, 0.f, c->p_ce, U + (long)(b0 + s0) * P.n_out, nb,
                                    P.n_out, ls, c->has_mask2 ? c->mask2 : nullptr, (long)c->mask2_from - (b0 + s0));
                return 0;
            }
            const float* Vc = V + (long)(b0 + s0) * c->prog->n_in;
            if (tangent_pass(c, Vc, nb, ls)) return -1;
            // U = mask * (cv*V + ce*dEps); dEps lives strided in arena T -> gather through eps_buf
            launch_copy(c->arenaT + c->tens[c->prog->eps_t].off, c->prog->per_sample, c->eps_buf, c->prog->n_out, 0, nb, c->prog->n_out, ls);
            launch_masked_axpby(c->prog->n_out == c->prog->n_in ? Vc : nullptr, c->eps_buf, c->has_mask ? c->mask : nullptr, c->p_cv,
                                c->p_ce, U + (long)(b0 + s0) * c->prog->n_out, nb, c->prog->n_out, ls,
                                c->has_mask2 ? c->mask2 : nullptr, (long)c->mask2_from - (b0 + s0));
            return 0;
        });
        if (rc) return rc;
    }
    HIPCHK(c, hipGetLastError());
    return 0;
}

static int pmp_vjp_run(loco_ctx* c, const float* U, int32_t k, float* A, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const int MB = c->cfg.max_batch;
    for (int b0 = 0; b0 < k; b0 += MB) {
        int B = (k - b0 < MB) ? k - b0 : MB;
        int rc = run_lanes(c, B, st, [&](int s0, int nb, hipStream_t ls) -> int {
            const Program& P = *c->prog;
            if (c->tap == 1) {         // h -> x_t: U seeds the tap cotangent; the skip slots the encoder ops accumulate into start at zero
                tap_zero_skips(c, nb, ls);
                launch_copy(U + (long)(b0 + s0) * P.n_h, P.n_h, c->arenaT + c->tens[P.h_t].off, P.per_sample, 0, nb, P.n_h, ls);
                return cotangent_pass(c, nullptr, nullptr, A + (long)(b0 + s0) * P.n_in, nb, ls, 0, P.h_last_op);
            }
            if (c->tap == 2) {         // eps -> h: the decoder half, then the tap cotangent out of the arena
                launch_cot_seed(U + (long)(b0 + s0) * P.n_out, c->has_mask ? c->mask : nullptr, 0.f, c->p_ce, c->ge, nullptr, nb, P.n_out,
                                ls, c->has_mask2 ? c->mask2 : nullptr, (long)c->mask2_from - (b0 + s0));
                if (cotangent_pass(c, c->ge, nullptr, nullptr, nb, ls, P.h_last_op + 1)) return -1;
                launch_copy(c->arenaT + c->tens[P.h_t].off, P.per_sample, A + (long)(b0 + s0) * P.n_h, P.n_h, 0, nb, P.n_h, ls);
                return 0;
            }
            const bool same = c->prog->n_out == c->prog->n_in;
            launch_cot_seed(U + (long)(b0 + s0) * c->prog->n_out, c->has_mask ? c->mask : nullptr, c->p_cv, c->p_ce, c->ge,
                            same ? c->gx0 : nullptr, nb, c->prog->n_out, ls, c->has_mask2 ? c->mask2 : nullptr,
                            (long)c->mask2_from - (b0 + s0));
            return cotangent_pass(c, c->ge, same ? c->gx0 : nullptr, A + (long)(b0 + s0) * c->prog->n_in, nb, ls);
        });
        if (rc) return rc;
    }
    HIPCHK(c, hipGetLastError());
    return 0;
}

int loco_pmp_vjp(loco_ctx* c, const float* U, int32_t k, float* A, void* stream) {
    if (!c) return -2;
    if (!c->primal_ok) { c->err = "loco_pmp_primal has not been called"; return -2; }
    return pmp_vjp_run(c, U, k, A, stream);
}

int loco_pmp_vjp_context(loco_ctx* c, const float* U, int32_t k, float* A, float* G, void* stream) {
    if (!c) return -2;
    if (c->cfg.context_dim <= 0) { c->err = "loco_pmp_vjp_context: this architecture has no cross-attention stages (context_dim = 0)"; return -2; }
    if (c->cfg.added_kv) {
        c->err = "loco_pmp_vjp_context: the added_kv attention blocks (DeepFloyd IF) pass the states through a per-block GroupNorm and "
                 "the pooled time embedding: their gradient is not built";
        return -2;
    }
    if (!G) { c->err = "loco_pmp_vjp_context: G is NULL"; return -2; }
    if (!c->primal_ok) { c->err = "loco_pmp_vjp_context: no valid primal (loco_pmp_primal has not been called since the last loco_set_context)"; return -2; }
    if (c->tap != 0) { c->err = "loco_pmp_vjp_context: the cached primal is an h-space tap's (tap = 1 / 2); the prompt-state gradient is of the whole network (tap = 0)"; return -2; }
    // The convolutions of a cotangent pass are planned by its batch (tile, split-K factor: conv_plan.hip), so the bits of g_o at
    // a stage -- and of A -- depend on k and on a probe's place in the batch.  A keeps loco_pmp_vjp's batched passes; the rows
    // of G come from one single-probe pass each, which is what makes a row the same bits wherever it stands.  k = 1 (null-text
    // inversion) is one pass for both; without A a pass stops behind the first op that reads the states.
    hipStream_t st = (hipStream_t)stream;
    const Program& P = *c->prog;
    const bool withA = A && k == 1;
    if (A && k > 1)
        if (int rc = pmp_vjp_run(c, U, k, A, stream)) return rc;
    float* gx0 = withA && P.n_out == P.n_in ? c->gx0 : nullptr;
    int ctx_lo = 0;
    if (!withA)
        while (ctx_lo < (int)c->ops.size() && !c->ops[ctx_lo].has_ctx_kv()) ++ctx_lo;
    for (int p = 0; p < k; ++p) {
        c->ctx_G = G + (long)p * c->cfg.context_len * c->cfg.context_dim; c->ctx_G_first = true;
        launch_cot_seed(U + (long)p * P.n_out, c->has_mask ? c->mask : nullptr, c->p_cv, c->p_ce, c->ge, gx0, 1, P.n_out, st,
                        c->has_mask2 ? c->mask2 : nullptr, (long)c->mask2_from - p);
        const int rc = cotangent_pass(c, c->ge, gx0, withA ? A : nullptr, 1, st, ctx_lo);
        c->ctx_G = nullptr;
        if (rc) return rc;
    }
    HIPCHK(c, hipGetLastError());
    return 0;
}

int loco_orthonormalize(loco_ctx* c, float* A, int32_t k, int64_t n, float* s, void* stream) {
    if (!c) return -2;
    if (k < 1 || k > 64 || n > c->n_ws) { c->err = "orthonormalize: need k <= 64 and n <= max(C*H*W, n_h) of the context"; return -2; }
    hipStream_t st = (hipStream_t)stream;
    launch_gram(A, k, n, c->G, c->gscratch, st);
    launch_jacobi_eig(c->G, k, c->W, c->Q, st);
    launch_rotate_rows(A, c->tmpA, k, n, c->Q, c->W, 0, st);
    // The Gram squares the condition number: rows rotated by its eigenvectors are orthonormal to about
    // k 2^-53 w_max / (s_i s_j), which on a graded spectrum is far from fp32 rounding.  The eigensolver raises
    // W[SOLVER_W_GATE] for such a spectrum and the rows then take one Cholesky pass, in the order of descending singular
    // value so that each row is corrected against the better determined ones only; a row with less than a quarter of
    // its norm left after that has no direction of its own and is dropped (zero row, s = 0).  With the gate down these
    // launches return at once and the last one only copies tmpA back: decided on the device, nothing is read back.
    const double* gate = c->W + SOLVER_W_GATE;
    launch_gram(c->tmpA, k, n, c->G, c->gscratch, st, gate);
    launch_cholesky(c->G, k, st, 0.25, c->W, gate);
    launch_trsm_rows(c->tmpA, A, k, n, c->G, st, gate);
    // singular values of the input = sqrt(eigenvalues of A A^T)
    launch_sign_fix(A, k, n, s, c->W, reinterpret_cast<float*>(c->red), st);
    HIPCHK(c, hipGetLastError());
    return 0;
}

int loco_qr_rows(loco_ctx* c, float* A, int32_t k, int64_t n, void* stream) {
    if (!c) return -2;
    if (k < 1 || k > 64 || n > c->n_ws) { c->err = "qr_rows: need k <= 64 and n <= max(C*H*W, n_h) of the context"; return -2; }
    hipStream_t st = (hipStream_t)stream;
    for (int rep = 0; rep < 2; ++rep) {   // CholeskyQR2
        launch_gram(A, k, n, c->G, c->gscratch, st);
        launch_cholesky(c->G, k, st);
        launch_trsm_rows(A, c->tmpA, k, n, c->G, st);
        HIPCHK(c, hipMemcpyAsync(A, c->tmpA, (size_t)k * n * sizeof(float), hipMemcpyDeviceToDevice, st));
    }
    HIPCHK(c, hipGetLastError());
    return 0;
}

int loco_convergence(loco_ctx* c, const float* Vprev, const float* V, int64_t count, float atol, float* out2,
                     void* stream) {
    if (!c) return -2;
    launch_convergence(Vprev, V, count, atol, 1e-5f, out2, c->gscratch, (hipStream_t)stream);
    HIPCHK(c, hipGetLastError());
    return 0;
}

int loco_convergence_rows(loco_ctx* c, const float* Vprev, const float* V, int32_t k, int64_t n, float atol,
                          float* out2, void* stream) {
    if (!c) return -2;
    if (k < 1 || k > 64 || n < 1) { c->err = "convergence_rows: need 1 <= k <= 64"; return -2; }
    // the kernel leaves k * min(64, ceil(n / 256)) * 4 doubles in gscratch, which is sized for rows of the context's own width
    if (n > c->n_ws) { c->err = "convergence_rows: rows longer than max(C*H*W, n_h) of the context"; return -2; }
    {
        const size_t nseg = (size_t)((n + 255) / 256) < 64 ? (size_t)((n + 255) / 256) : 64;
        const size_t cap = (((size_t)c->n_ws + 255) / 256) * 64 * 64 + 4096;       // doubles in gscratch (finalize_params)
        if ((size_t)k * nseg * 4 > cap) { c->err = "convergence_rows: k rows of this length exceed the reduction workspace"; return -2; }
    }
    launch_convergence_rows(Vprev, V, k, n, atol, 1e-5f, out2, c->gscratch, (hipStream_t)stream);
    HIPCHK(c, hipGetLastError());
    return 0;
}

// ---- block Krylov solver (DESIGN.md "Block Krylov solver"): one step = loco_krylov_extend + loco_krylov_ritz ----
static const char* krylov_sizes(loco_ctx* c, int32_t k, int32_t m, int64_t n, int32_t slot, bool n_is_input) {
    if (slot < 0 || slot > 1) return "krylov: slot must be 0 or 1";
    if (k < 1 || k > KRYLOV_MAX_BLOCK) return "krylov: need 1 <= k <= 32 (two blocks must fit in 64 rows)";
    if (m < k || m > 64 || m % k != 0) return "krylov: m must be a multiple of k with k <= m <= 64";
    if (n < 1) return "krylov: empty rows";
    if (n_is_input && n > c->n_ws) return "krylov: rows longer than max(C*H*W, n_h) of the context";
    return nullptr;
}

int loco_krylov_extend(loco_ctx* c, float* A, int32_t k, const float* Q, int32_t m, int64_t n, float* next, float* stat,
                       int32_t slot, void* stream) {
    if (!c) return -2;
    if (const char* e = krylov_sizes(c, k, m, n, slot, true)) { c->err = e; return -2; }
    if (!A || !Q || !stat) { c->err = "krylov_extend: null pointer"; return -2; }
    hipStream_t st = (hipStream_t)stream;
    double* S = c->kry[slot];
    // projection coefficients Ct [m][k] = Q A^T: T's newest block column / row, and the first Gram-Schmidt pass
    launch_cross_gram(Q, m, A, k, n, c->G, c->gscratch, st);
    launch_krylov_fill_t(c->G, m, k, S + KRY_T, c->Q, st);
    launch_project_rows(A, k, Q, m, n, c->G, A, st);
    launch_cross_gram(Q, m, A, k, n, c->G, c->gscratch, st);          // second pass ("twice is enough")
    launch_project_rows(A, k, Q, m, n, c->G, A, st);
    launch_gram(A, k, n, S + KRY_G, c->gscratch, st);                 // G = R R^T: the residual estimate and the next block's Gram
    launch_jacobi_eig(c->Q, m, S + KRY_THETA, S + KRY_W, st);         // Ritz pairs of T[:m][:m]
    c->kry_m[slot] = m;
    c->kry_k[slot] = k;
    if (next) {
        // next block = R orthonormalised within itself (loco_orthonormalize's sequence on the Gram already at hand),
        // directions below KRYLOV_DROP * theta_0 zeroed in place, then one more projection against Q
        launch_jacobi_eig(S + KRY_G, k, c->W, c->Q, st);
        launch_krylov_floor(c->W, k, S + KRY_THETA, stat, st);
        launch_rotate_rows(A, c->tmpA, k, n, c->Q, c->W, 0, st);
        const double* gate = c->W + SOLVER_W_GATE;
        launch_gram(c->tmpA, k, n, c->G, c->gscratch, st, gate);
        launch_cholesky(c->G, k, st, 0.25, c->W, gate);
        launch_trsm_rows(c->tmpA, next, k, n, c->G, st, gate);
        launch_cross_gram(Q, m, next, k, n, c->G, c->gscratch, st);
        launch_project_rows(next, k, Q, m, n, c->G, next, st);
    } else {
        HIPCHK(c, hipMemsetAsync(stat + 3, 0, sizeof(float), st));
    }
    HIPCHK(c, hipGetLastError());
    return 0;
}

int loco_krylov_ritz(loco_ctx* c, const float* Q, int32_t m, int64_t n, int32_t k, float* Y, const float* Yprev, float atol,
                     float* resid, float* stat, int32_t slot, void* stream) {
    if (!c) return -2;
    if (const char* e = krylov_sizes(c, k, m, n, slot, true)) { c->err = e; return -2; }
    if (!Q || !Y || !resid || !stat) { c->err = "krylov_ritz: null pointer"; return -2; }
    if (c->kry_m[slot] != m || c->kry_k[slot] != k) { c->err = "krylov_ritz: loco_krylov_extend has not been called for these m rows in blocks of k"; return -2; }
    hipStream_t st = (hipStream_t)stream;
    double* S = c->kry[slot];
    launch_rotate_rect(Q, Y, k, m, n, S + KRY_W, m, nullptr, st);
    launch_sign_fix(Y, k, n, nullptr, nullptr, reinterpret_cast<float*>(c->red), st, S + KRY_SIGN);
    launch_krylov_resid(S + KRY_W, m, k, S + KRY_G, S + KRY_THETA, resid, stat, Yprev != nullptr, st);
    if (Yprev) launch_convergence_rows(Yprev, Y, k, n, atol, 1e-5f, stat, c->gscratch, st);
    HIPCHK(c, hipGetLastError());
    return 0;
}

int loco_krylov_left(loco_ctx* c, const float* Ustore, int32_t m, int64_t n_out, int32_t k, float* UY, float* s, int32_t slot,
                     void* stream) {
    if (!c) return -2;
    if (const char* e = krylov_sizes(c, k, m, n_out, slot, false)) { c->err = e; return -2; }
    if (!Ustore || !UY || !s) { c->err = "krylov_left: null pointer"; return -2; }
    if (c->kry_m[slot] != m || c->kry_k[slot] != k) { c->err = "krylov_left: loco_krylov_extend and loco_krylov_ritz have not been called for these m rows in blocks of k"; return -2; }
    hipStream_t st = (hipStream_t)stream;
    double* S = c->kry[slot];
    launch_rotate_rect(Ustore, UY, k, m, n_out, S + KRY_W, m, S + KRY_SIGN, st);
    launch_row_sqnorm(UY, k, n_out, s, c->gscratch, st);
    HIPCHK(c, hipGetLastError());
    return 0;
}

int loco_null_project(loco_ctx* c, const float* Vm, int32_t k, const float* Vn, int32_t k0, int64_t n, float* out,
                      void* stream) {
    if (!c) return -2;
    if (k < 1 || k > 64 || k0 > 64 || n > c->prog->n_in) { c->err = "null_project: bad sizes"; return -2; }
    hipStream_t st = (hipStream_t)stream;
    if (Vn && k0 > 0) {
        launch_cross_gram(Vn, k0, Vm, k, n, c->G, c->gscratch, st);
        launch_project_rows(Vm, k, Vn, k0, n, c->G, out, st);
    } else if (out != Vm) {
        HIPCHK(c, hipMemcpyAsync(out, Vm, (size_t)k * n * sizeof(float), hipMemcpyDeviceToDevice, st));
    }
    launch_normalize_rows(out, k, n, c->gscratch, st);
    HIPCHK(c, hipGetLastError());
    return 0;
}

int loco_edit_axpy(loco_ctx* c, const float* x, const float* v, const float* alphas, int32_t B, int64_t n, float* out,
                   void* stream) {
    if (!c) return -2;
    if (B > 256) { c->err = "edit_axpy: B > 256"; return -2; }
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(c, hipMemcpyAsync(c->alphas, alphas, B * sizeof(float), hipMemcpyHostToDevice, st));
    launch_edit_axpy(x, v, c->alphas, B, n, out, st);
    HIPCHK(c, hipGetLastError());
    return 0;
}

static long mask_count_lazy(loco_ctx* c) {
    if (c->mask_L < 0) {
        int L = 0;
        if (hipMemcpyAsync(&L, c->mask_L_dev, sizeof(int), hipMemcpyDeviceToHost, c->mask_stream) != hipSuccess ||
            hipStreamSynchronize(c->mask_stream) != hipSuccess) return -1;
        c->mask_L = L;
    }
    return c->mask_L;
}
int64_t loco_mask_count(loco_ctx* c) { return c ? mask_count_lazy(c) : -1; }

int loco_mask_gather(loco_ctx* c, const float* U, int32_t k, float* out, void* stream) {
    if (!c) return -2;
    if (!c->primal_ok) { c->err = "loco_pmp_primal has not been called"; return -2; }
    hipStream_t st = (hipStream_t)stream;
    if (!c->has_mask) {      // rows of J V as they are: n_h wide for the encoder tap (which takes no mask), else n_out
        const size_t w = c->tap == 1 ? c->prog->n_h : c->prog->n_out;
        HIPCHK(c, hipMemcpyAsync(out, U, (size_t)k * w * sizeof(float), hipMemcpyDeviceToDevice, st));
        return 0;
    }
    const long L = mask_count_lazy(c);
    if (L < 0) { c->err = "mask count readback failed"; return -1; }
    if (L > 0) launch_mask_gather(U, c->mask_idx, L, c->prog->n_out, k, out, st);
    HIPCHK(c, hipGetLastError());
    return 0;
}

int loco_clock_stamp(loco_ctx* c, uint64_t* out2, void* stream) {
    if (!c || !out2) return -2;
    launch_clock_stamp(reinterpret_cast<unsigned long long*>(out2), (hipStream_t)stream);
    HIPCHK(c, hipGetLastError());
    return 0;
}

double loco_unet_flops(loco_ctx* c) {
    if (!c) return 0.0;
    if (!c->finalized && finalize_params(c)) return 0.0;
    return c->wts->flops;
}
int64_t loco_workspace_bytes(loco_ctx* c) { return c ? (int64_t)c->bytes : 0; }

int loco_timer_start(loco_ctx* c, void* stream) {
    if (!c) return -2;
    HIPCHK(c, hipEventRecord(c->ev0, (hipStream_t)stream));
    return 0;
}
int loco_timer_stop(loco_ctx* c, void* stream, float* ms) {
    if (!c) return -2;
    HIPCHK(c, hipEventRecord(c->ev1, (hipStream_t)stream));
    HIPCHK(c, hipEventSynchronize(c->ev1));
    HIPCHK(c, hipEventElapsedTime(ms, c->ev0, c->ev1));
    return 0;
}

int loco_set_precision(loco_ctx* c, int32_t mode) {
    if (!c) return -2;
    if (mode < 0 || mode > 2) { c->err = "precision mode must be 0 (f32), 1 (bf16x3) or 2 (f16)"; return -2; }
    c->prec = mode;
    c->primal_ok = false;   // the {S, xhat} cache belongs to the mode it was built in
    return 0;
}
int loco_get_precision(loco_ctx* c) { return c ? c->prec : -2; }

int loco_set_cond(loco_ctx* c, const float* emb_add, void* stream) {
    if (!c) return -2;
    c->primal_ok = false;           // cached activations belong to the previous condition
    if (!emb_add) { c->has_cond = false; return 0; }
    HIPCHK(c, hipMemcpyAsync(c->cond_add, emb_add, (size_t)c->cfg.ch * 4 * sizeof(float), hipMemcpyDeviceToDevice,
                             (hipStream_t)stream));
    c->has_cond = true;
    return 0;
}

int loco_set_time_cond(loco_ctx* c, const float* w_emb, void* stream) {
    if (!c) return -2;
    const int P = c->cfg.time_cond_proj_dim;
    if (P <= 0) { c->err = "loco_set_time_cond: this architecture has no guidance-scale embedding (time_cond_proj_dim = 0)"; return -2; }
    c->primal_ok = false;           // cached activations belong to the previous embedding
    if (!w_emb) { c->has_tcond = false; return 0; }
    if (finalize_params(c)) return -3;
    // cond_in[ch] = cond_proj.weight [ch][P] . w_emb [P]: the per-block projection kernel without a bias
    launch_temb_proj(w_emb, P, c->wts->tcw, nullptr, c->cfg.ch, c->cond_in, (hipStream_t)stream);
    HIPCHK(c, hipGetLastError());
    c->has_tcond = true;
    return 0;
}

int loco_set_context(loco_ctx* c, const float* tokens, void* stream) {
    if (!c) return -2;
    if (c->cfg.context_dim <= 0) { c->err = "this architecture has no cross-attention stages (context_dim = 0)"; return -2; }
    if (!tokens) { c->err = "loco_set_context: null tokens"; return -2; }
    if (finalize_params(c)) return -3;
    hipStream_t st = (hipStream_t)stream;
    c->primal_ok = false;
    const int L = c->cfg.context_len, D = c->cfg.context_dim, Lp = c->prog->ctx_Lp;
    if (!c->ctx_colbias) {
        std::vector<float> cb(Lp, -1e30f);
        for (int l = 0; l < L; ++l) cb[l] = 0.f;
        if (upload(c, &c->ctx_colbias, cb)) return -1;
    }
    if (c->cfg.added_kv && !c->ctx_norm && dalloc(c, &c->ctx_norm, (size_t)L * D)) return -1;
    for (auto& op : c->ops) {
        if (!op.has_ctx_kv()) continue;
        const int C = c->tens[op.in].C;
        const float* tok = tokens;
        if (op.added_kv) {      // the block's own GroupNorm over the states [D][L] (norm_encoder), then encoder_kv
            launch_ctx_groupnorm(tokens, L, D, c->cfg.gn_groups, c->cfg.gn_eps, op.xng, op.xnb, c->ctx_norm, st);
            tok = c->ctx_norm;
        }
        for (int w = 0; w < 2; ++w) {
            float* dst = w ? op.xV : op.xK;
            HIPCHK(c, hipMemsetAsync(dst, 0, (size_t)C * Lp * sizeof(float), st));
            // dst[c][l] = sum_d W[c][d] tokens[l][d] + b[c]
            GemmArgs g; std::memset(&g, 0, sizeof(g));
            g.A = w ? op.xvw : op.xkw; g.sam = D; g.sak = 1;
            g.Bm = tok; g.sbk = 1; g.sbn = D;
            g.C = dst; g.scm = Lp; g.scn = 1;
            g.bias = w ? op.xvb : op.xkb;
            g.M = C; g.N = L; g.K = D; g.batch = 1; g.alpha = 1.f; g.beta = 0.f;
            launch_gemm(g, st);
        }
    }
    HIPCHK(c, hipGetLastError());
    c->has_ctx = true;
    return 0;
}

int loco_masked_axpby(loco_ctx* c, const float* V, const float* E, float cv, float ce, int32_t k, float* out,
                      void* stream) {
    if (!c) return -2;
    if (!c->primal_ok) { c->err = "loco_pmp_primal has not been called"; return -2; }
    launch_masked_axpby(V, E, c->has_mask ? c->mask : nullptr, cv, ce, out, k, c->prog->n_out, (hipStream_t)stream);
    HIPCHK(c, hipGetLastError());
    return 0;
}

int loco_latent_sample(loco_ctx* c, const float* moments, const float* noise, float scale, int32_t B, float* z, void* stream) {
    if (!c) return -2;
    if (c->cfg.arch != 3 || (c->cfg.out_ch & 1)) { c->err = "latent_sample: the context must be a latent encoder (arch 3) with out_ch = 2 z"; return -2; }
    if (B < 1 || !moments || !z) { c->err = "latent_sample: bad arguments"; return -2; }
    launch_latent_sample(moments, noise, scale, z, B, c->prog->n_out / 2, (hipStream_t)stream);
    HIPCHK(c, hipGetLastError());
    return 0;
}

int loco_lincomb(loco_ctx* c, const float* const* src, const float* coef, int32_t n, float* out, int64_t count,
                 void* stream) {
    if (!c) return -2;
    if (n < 1 || n > 4) { c->err = "lincomb: 1..4 terms"; return -2; }
    launch_lincomb(src, coef, n, out, (long)count, (hipStream_t)stream);
    HIPCHK(c, hipGetLastError());
    return 0;
}

int loco_diffedit_mask(loco_ctx* c, const float* eps_a, const float* eps_b, float scale, int32_t B, int32_t C, int64_t HW,
                       int32_t rule, float* m_out, uint8_t* mask_out, void* stream) {
    if (!c) return -2;
    if (!eps_a || !eps_b || !mask_out || B < 1 || C < 1 || HW < 1) { c->err = "diffedit_mask: bad arguments"; return -2; }
    if (rule != 0 && rule != 1) { c->err = "diffedit_mask: rule is 0 (reference) or 1 (intended)"; return -2; }
    // reduction workspace (doubles, create_ctx) read as floats: [0, 768) block partials, [768, 772) status, [1024, ..) the map
    // when the caller does not ask for it
    float* ws = reinterpret_cast<float*>(c->gscratch);
    const size_t cap = 2 * ((((size_t)c->prog->n_in + 255) / 256) * 64 * 64 + 4096);
    float* m = m_out;
    if (!m) {
        if (1024 + (size_t)HW > cap) { c->err = "diffedit_mask: map larger than the reduction workspace; pass m_out"; return -2; }
        m = ws + 1024;
    }
    hipStream_t st = (hipStream_t)stream;
    launch_diffedit_mask(eps_a, eps_b, scale, B, C, (long)HW, rule, m, mask_out, ws, ws + 768, st);
    HIPCHK(c, hipGetLastError());
    float status[3] = {0.f, 0.f, 0.f};      // the one read-back, after both launches: a constant map is an error, not a mask
    HIPCHK(c, hipMemcpyAsync(status, ws + 768, sizeof(status), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (status[0] == 1.f) {
        c->err = "diffedit_mask: constant map (max == min = " + std::to_string(status[1]) + "): the two noise predictions do not differ";
        return -4;
    }
    if (status[0] != 0.f) { c->err = "diffedit_mask: non-finite map"; return -5; }
    return 0;
}

int loco_cfg_masked_step(loco_ctx* c, const float* x, const float* eps_for, const float* eps_edit, const float* eps_null,
                         float g, float at, float at_next, const uint8_t* mask, int32_t B, int64_t n, float* x_next,
                         void* stream) {
    if (!c) return -2;
    if (!x || !eps_for || !eps_edit || !eps_null || !mask || !x_next || B < 1 || n < 1) {
        c->err = "cfg_masked_step: bad arguments";
        return -2;
    }
    float s1, s2, s3, ce, cn;
    sched_coeffs(at, at_next, 0.f, &s1, &s2, &s3, &ce, &cn);
    launch_cfg_masked_step(x, eps_for, eps_edit, eps_null, mask, x_next, B, (long)n, g, s2, s1, s3, ce, (hipStream_t)stream);
    HIPCHK(c, hipGetLastError());
    return 0;
}

int loco_lcm_step(loco_ctx* c, const float* x, const float* eps, float at, float at_prev, float c_skip, float c_out,
                  const float* noise, int64_t count, float* x_prev, float* denoised, void* stream) {
    if (!c) return -2;
    if (!x || !eps || count < 1 || (!x_prev && !denoised)) { c->err = "lcm_step: bad arguments"; return -2; }
    if (!(at > 0.f && at <= 1.f) || !(at_prev >= 0.f && at_prev <= 1.f)) { c->err = "lcm_step: alpha-bar outside (0, 1]"; return -2; }
    launch_lcm_step(x, eps, noise, x_prev, denoised, (long)count, std::sqrt(at), std::sqrt(1.0f - at), std::sqrt(at_prev),
                    std::sqrt(1.0f - at_prev), c_skip, c_out, (hipStream_t)stream);
    HIPCHK(c, hipGetLastError());
    return 0;
}

int loco_set_streams(loco_ctx* c, int32_t n) {
    if (!c || (n != 1 && n != 2)) return -2;
    c->n_streams = n;
    return 0;
}

int loco_set_chip_share(loco_ctx* c, int32_t n) {
    if (!c || n < 1 || n > 8) return -2;
    c->chip_share = n;
    return 0;
}

int loco_set_side_stream(loco_ctx* c, void* stream) {
    if (!c) return -2;
    c->st2_user = (hipStream_t)stream;          // nullptr: back to the context's own stream
    return 0;
}

int loco_profile_enable(loco_ctx* c, int32_t on) {
    if (!c) return -2;
    c->prof_on = on != 0;
    c->prof_shapes = on == 2;     // 2: aggregate per layer shape instead of per kernel variant
    if (on) { c->prof.clear(); c->ev_used = 0; }
    return 0;
}

int loco_profile_report(loco_ctx* c, char* buf, int64_t cap) {
    if (!c || !buf || cap < 1) return -2;
    HIPCHK(c, hipDeviceSynchronize());
    std::map<std::string, std::array<double, 3>> agg;   // launches, ms, flops
    for (auto& r : c->prof) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, r.e0, r.e1) != hipSuccess) continue;
        std::string key = r.name;
        if (c->prof_shapes) {
            char sb[96];
            snprintf(sb, sizeof(sb), "|t%d_m%d_ci%d_co%d_h%d_b%d_s%d", r.taps, r.mode, r.cin, r.cout, r.h, r.b, r.ns);
            key += sb;
        }
        auto& a = agg[key];
        a[0] += 1.0; a[1] += ms; a[2] += r.flops;
    }
    std::string out;
    char line[256];
    for (auto& kv : agg) {
        snprintf(line, sizeof(line), "%s %.0f %.6f %.6e\n", kv.first.c_str(), kv.second[0], kv.second[1], kv.second[2]);
        out += line;
    }
    if ((int64_t)out.size() + 1 > cap) { c->err = "profile buffer too small"; return -4; }
    std::memcpy(buf, out.c_str(), out.size() + 1);
    return 0;
}

}  // extern "C"
