// What the engine's units share (engine.hip: launch execution, attention core, passes, C ABI; engine_params.hip: host-side
// weight packing; engine_diag.hip: the hooks of include/loco_hip_diag.h): the context, its views of the program, and the
// functions more than one of them calls.  Internal to csrc/: never installed, one layout of loco_ctx in every build.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../include/loco_hip.h"
#include "kernels.h"
#include "program.h"

#define HIPCHK(ctx, call)                                                                    \
    do {                                                                                     \
        hipError_t e_ = (call);                                                              \
        if (e_ != hipSuccess) {                                                              \
            (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_);                  \
            return -1;                                                                       \
        }                                                                                    \
    } while (0)

namespace loco {
namespace eng {

struct ConvP {       // one convolution's parameters in kernel layouts
    float* wf = nullptr;    // forward  [Cin][taps][CoutP]
    float* wd = nullptr;    // dgrad    [Cout][taps][CinP]  (flipped taps)
    float* wbf = nullptr;   // split-bf16 forward records [Cin/16][taps][CoutP][32 x u16]
    float* wbd = nullptr;   // split-bf16 dgrad records   [Cout/16][taps][CinP][32 x u16]
    float* whf = nullptr;   // f16 forward records        [Cin/16][taps][CoutP][16 x f16]
    float* whd = nullptr;   // f16 dgrad records          [Cout/16][taps][CinP][16 x f16]
    // polyphase form of an up / down-sampling conv (kernels.h polyphase_fold): records of the folded operator, 4 taps x 4 couts
    // virtual couts -- of the forward operator for the nearest-x2 conv, of the dgrad operator (poly_dgrad) for the stride-2
    // conv's zero-insert data gradient; nullptr: none (the 3x3 route)
    float* wpb = nullptr;   // split-bf16
    float* wph = nullptr;   // f16
    bool poly_dgrad = false;
    // the up conv's cotangent as one launch (kernels.h ConvArgs::pool2, polyphase_fold_in): records of the dgrad operator folded
    // with the 2x2 sum-pool, [4 Cout/16][4][CinP]
    float* wqb = nullptr;   // split-bf16
    float* wqh = nullptr;   // f16
    float* bias = nullptr;
    int cin = 0, cout = 0, taps = 0;
};
struct NormW { float* gamma = nullptr; float* beta = nullptr; };

// One op's device parameters: written by finalize_params of the root context, read-only afterwards, copied as one value into
// the Op views of the root and of every fork (bind_weights).  A field added here reaches the forks without further code.
struct OpWeights {
    ConvP c1, c2, nin, qkvc, proj, conv;     // conv: CONV_IN / DOWN / UP / OUT
    ConvP xqc, xproj;                        // cross-attention q and output projection
    ConvP pj_in, to_out1, to_out2, ff1, ff2, pj_out;   // XFMR linear maps (as 1x1 convs over [C][T]); qkvc = fused [to_q; to_k; to_v]
                                                       // of attn1 (per-head rows), xqc = attn2.to_q
    NormW g1, g2, gx;                        // gamma / beta of the plan's n1 / n2 / nx
    float *xkw = nullptr, *xkb = nullptr, *xvw = nullptr, *xvb = nullptr;   // key / value projections of the context [C][D], [C]
    float *xng = nullptr, *xnb = nullptr;    // added_kv: `norm_encoder` of the states
    float *lng[3] = {nullptr, nullptr, nullptr}, *lnb[3] = {nullptr, nullptr, nullptr};   // XFMR LayerNorms
    long tproj_off = 0;                      // RES: offset into the concatenated temb projections
};
struct Weights {
    std::vector<OpWeights> op;               // indexed like Program::ops
    float *freq = nullptr, *td0w = nullptr, *td0b = nullptr, *td1w = nullptr, *td1b = nullptr;   // time embedding
    float* tcw = nullptr;          // time_embed.cond_proj.weight [ch][time_cond_proj_dim] (cfg.time_cond_proj_dim > 0)
    float *tp_w = nullptr, *tp_b = nullptr;  // concatenated temb_proj
    long tproj_total = 0;
    double flops = 0.0;
};

// A context's views of the program, indexed like Program::tens / ::ops: the plan (copied), the weights (bound by bind_weights)
// and the state that belongs to this context alone (allocated by alloc_state).
struct Tens : TensPlan {
    // a concatenation part keeps the {mean, M2} tile partials its producer's epilogue took (keep_ntile > 0 in the forward pass
    // that wrote them) so the norm over the concatenation can be finalised from both parts' partials instead of re-reading the
    // tensor (gn_fused_finalize_cat_kernel)
    float* keep = nullptr; size_t keep_floats = 0; int keep_ntile = 0;
};
struct NormP : NormPlan, NormW {
    bool ready = false; // statistics of the current pass were delivered with the producing conv (run_conv StatReq)
};
struct Op : OpPlan, OpWeights {
    NormP n1, n2, nx;                        // OpPlan's norms (hidden by these) + their gamma / beta + this context's flags
    float *xK = nullptr, *xV = nullptr;      // projected context [C][Lp] (loco_set_context)
};

struct HostParam { std::vector<float> data; std::vector<int64_t> shape; bool loaded = false; };

}  // namespace eng
}  // namespace loco


struct loco_ctx {
    loco_unet_cfg cfg;             // prog->cfg with this context's max_batch
    std::string err;
    std::map<std::string, loco::eng::HostParam> params;
    bool finalized = false;

    std::shared_ptr<const loco::Program> prog;   // a fork shares its root's (same configuration; max_batch does not enter the layout)
    std::shared_ptr<loco::eng::Weights> wts;           // the root's; written by its finalize_params only
    std::vector<loco::eng::Tens> tens;                // this context's views, see Tens / Op
    std::vector<loco::eng::Op> ops;


    float *arenaP = nullptr, *arenaT = nullptr;
    float *statsP = nullptr, *statsT = nullptr;
    double* red = nullptr;         // reduction scratch (doubles)
    bool fuse_cot = true;          // norm-cotangent term in the shortcut conv's epilogue (LOCO_FUSE_COT=0: standalone gn_apply pass)
    float *stpart = nullptr, *stpart2 = nullptr;   // row partials of the statistics taken in conv epilogues (lane 0 / lane 1)
    size_t stpart_floats = 0;
    bool fuse_stats = true;        // LOCO_FUSE_STATS=0: every statistics pass as its own kernels (A/B timing)
    bool fuse_xattn = true;        // LOCO_FUSE_XATTN=0: cross-attention as strided GEMM + row kernel + strided GEMM (A/B)
    bool deep1 = true;             // LOCO_DEEP1=0: 1x1 operators on the two-buffer stage loop instead of the register ring (A/B)
    bool flash_attn = true;        // LOCO_FLASH_ATTN=0: tangent / cotangent attention on the generic GEMM + softmax-Jacobian path
    float* attn_delta = nullptr;   // [max_batch][heads][tokens] scratch of the flash cotangent (a lane's samples start at its first sample: LaneSwap)
    float* partial = nullptr;      // split-K workspace
    size_t partial_floats = 0;
    const float* bench_out = nullptr; int64_t bench_out_count = 0;      // diag: output tensor of the last loco_bench_conv
    std::string* plan_log = nullptr;                                    // diag: run_conv appends the text of every plan it executes (loco_debug_conv)
    std::string* attn_log = nullptr;                                    // diag: the attention stages append one line per launch (loco_debug_attn)
    float *tact = nullptr, *tproj = nullptr;
    float* eps_buf = nullptr;      // [max_batch][n]
    float* gx0 = nullptr;          // [max_batch][n] direct cotangent term
    float* ge = nullptr;           // [max_batch][n] cotangent seed of eps
    float* tmpA = nullptr;         // [64][n] temp for solver rotations
    double *G = nullptr, *Q = nullptr, *W = nullptr, *gscratch = nullptr;
    double* kry[2] = {nullptr, nullptr};   // block Krylov solver: state of up to two solves in flight (kernels.h KRY_*)
    int kry_m[2] = {0, 0}, kry_k[2] = {0, 0};   // rows and block size the Ritz vectors of each slot were computed for (0: none yet)
    float* alphas = nullptr;
    float* ctx_colbias = nullptr;  // [Lp]: 0 for real tokens, -1e30 for the padding
    bool has_ctx = false;
    // loco_pmp_vjp_context: where the cotangent pass being enqueued adds its probes' rows of G [B][context_len][context_dim]
    // (nullptr: no gradient asked for), and whether its next cross-attention stage is the first to write them
    float* ctx_G = nullptr;
    bool ctx_G_first = false;
    float* cond_add = nullptr;     // [temb_ch] conditioning embedding of the time embedding (loco_set_cond)
    float* ctx_norm = nullptr;     // [context_len][context_dim] scratch: the states behind one block's norm_encoder (added_kv)
    bool has_cond = false;
    float* cond_in = nullptr;      // [ch] cond_proj(w_emb), added to the sinusoid of the time embedding (loco_set_time_cond); this context's own
    bool has_tcond = false;
    float2* sxcache = nullptr;     // primal {S, xhat} per GroupNorm+SiLU input (bf16x3 path)
    int prec = 0;                  // 0: exact fp32 MFMA, 1: split-bf16 (bf16x3) MFMA, 2: single f16 MFMA
    std::vector<float*> owned;     // everything to hipFree
    size_t bytes = 0;

    // PMP state
    bool primal_ok = false;
    float p_cv = 0.f, p_ce = 0.f;
    int tap = 0;                   // operator of the cached primal (loco_pmp_primal_tap): 0 x_t -> x0 / eps, 1 x_t -> h, 2 h -> eps
    long n_ws = 0;                 // longest row the solver algebra takes: max(n_in, n_out, n_h) of a denoiser (n_in where there is no tap)
    uint8_t* mask = nullptr;       // device, [n] (owned copy)
    bool has_mask = false;
    uint8_t* mask2 = nullptr;      // device, [n] (owned copy): mask of the probe rows >= mask2_from (loco_pmp_set_second_mask)
    bool has_mask2 = false;
    int mask2_from = 0;
    int* mask_idx = nullptr;       // device: indices of the selected elements, ascending
    int* mask_L_dev = nullptr;     // device: their count
    long mask_L = 0;               // host copy, -1 = not read back yet
    hipStream_t mask_stream = nullptr;
    int primal_B = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // second lane (probe groups of one tangent / cotangent pass on two streams, see run_lanes)
    int n_streams = 1;
    hipStream_t st2 = nullptr;       // the context's own second stream
    hipStream_t st2_user = nullptr;  // caller-supplied second stream (loco_set_side_stream): used instead of st2 when set
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    double* red2 = nullptr;
    // B = 1..max_batch denoiser evaluations replayed as HIP graphs (loco_unet_forward / loco_ddim_step): the DDIM
    // opt-in (LOCO_GRAPH=1).  Measured: no gain on an idle host -- the eager launch list already runs back to back
    // (B = 1: 363 kernels, 5.29 ms busy of 5.31 ms span per evaluation) -- it only takes the ~360 launches per
    // evaluation off the host thread.
    struct FwdGraph { hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr; int calls = 0; };
    std::map<int, FwdGraph> fwd_graphs;
    bool graph_on = false;
    bool gemm_lowp = true;         // LOCO_GEMM_LOWP=0: every attention product on the exact f32-input kernel (A/B timing)
    // workspace of the record GEMM (gemm_rec.hip: the operands' split records + K-split partial tiles), one per stream lane, grown
    // on demand outside stream capture
    unsigned char* gemm_ws[2] = {nullptr, nullptr}; size_t gemm_ws_bytes[2] = {0, 0}; int lane = 0;
    // Shared parameter store (loco_fork, round 6): a forked context uses the device copies of its root's parameters (all six
    // layouts) and owns only its arenas, statistics, scratch and per-prompt constants.  The root stays allocated until its last
    // fork is destroyed (`forks`, `zombie`).
    loco_ctx* weights_of = nullptr;
    int forks = 0;
    bool zombie = false;
    bool fuse_lin = true;          // tangent / cotangent group means taken in the conv epilogues (LOCO_FUSE_LIN=0: standalone passes)
    int lanes_active = 1;          // 2 while run_lanes enqueues the two probe groups of a pass on two streams (split-K then aims below the whole chip)
    int lane_s0 = 0;               // first sample of the lane being enqueued (run_lanes): where its rows of a kept partial buffer start
    int chip_share = 1;            // contexts whose passes the host enqueues side by side on other streams (loco_set_chip_share): split-K aims at 256 / share workgroups
    hipStream_t cap_st = nullptr;  // capture stream (the caller's may be the legacy default stream)
    float* xin_buf = nullptr;      // [max_batch][n] fixed graph input
    float* t_dev = nullptr;        // timestep read by the captured time-embedding kernel
    // per-launch conv profile
    bool prof_on = false;
    struct ProfRec { const char* name; double flops; hipEvent_t e0, e1; int cin, cout, h, b, ns, mode, taps; };
    bool prof_shapes = false;
    std::vector<ProfRec> prof;
    std::vector<hipEvent_t> ev_pool;
    size_t ev_used = 0;
    hipEvent_t next_event() {
        if (ev_used == ev_pool.size()) {
            hipEvent_t e; (void)hipEventCreate(&e); ev_pool.push_back(e);
        }
        return ev_pool[ev_used++];
    }
};

namespace loco {
namespace eng {

template <typename T>
int dalloc(loco_ctx* c, T** p, size_t count) {
    void* q = nullptr;
    HIPCHK(c, hipMalloc(&q, count * sizeof(T)));
    *p = reinterpret_cast<T*>(q);
    c->owned.push_back(reinterpret_cast<float*>(q));
    c->bytes += count * sizeof(T);
    return 0;
}

inline float eps_of(const loco_ctx* c, const NormP& n) { return n.eps > 0.f ? n.eps : c->cfg.gn_eps; }
int upload(loco_ctx* c, float** dst, const std::vector<float>& h);

// engine_params.hip: a checkpoint's tensors into the kernels' layouts
int make_conv(loco_ctx* c, const std::vector<const HostParam*>& ws, const std::vector<const HostParam*>& bs,
              ConvP* out, int row_limit = -1, int poly_kind = -1, bool poly_dgrad = false);
int make_conv1(loco_ctx* c, const std::string& name, ConvP* out, int row_limit = -1, int poly_kind = -1, bool poly_dgrad = false);
int make_conv1_scaled(loco_ctx* c, const std::string& name, ConvP* out, float s);
int make_norm(loco_ctx* c, const std::string& name, NormW* n);
int bind_weights(loco_ctx* c);
int finalize_params(loco_ctx* c);

// sc / sh / mr / tst pointers of a norm inside a stats arena
struct NS { float *sc, *sh, *mr, *tst, *tc; };
NS nstats(const loco_ctx* c, float* base, const NormP& n);

// Statistics the NEXT consumer of a conv's output needs (GroupNorm forward statistics, or the tangent / cotangent group
// means), handed to run_conv with the conv that finishes the tensor: taken in the conv epilogue (whole cout tiles), in the
// split-K epilogue (reduce + statistics in one kernel), or -- where neither applies -- by the standalone kernels behind the
// conv.  Either way they are complete when run_conv returns, and the norm is marked `ready` for its consumer.
struct StatReq {
    int kind = ST_NONE;                       // ST_FWD / ST_TAN / ST_COT
    NormP* n = nullptr;
    float* stats = nullptr;                   // stats arena receiving the result (FWD: this pass's; TAN / COT: statsT)
    const float* prim = nullptr;              // primal of the conv's output tensor, B = 1 (TAN / COT)
    const float* ss_scale = nullptr; const float* ss_shift = nullptr;   // FWD: scale-shift norm (ADM)
    // FWD, output tensor is one part of a concatenation: its tile partials go to (and stay in) `keep`; *keep_ntile receives
    // the tile count, 0 when this launch could not take them.  n may be nullptr (no norm over the part alone).
    float* keep = nullptr; size_t keep_floats = 0; int* keep_ntile = nullptr;
};

inline void conv_defaults(ConvArgs& a) {
    std::memset(&a, 0, sizeof(a));
    a.stride = 1; a.pad = 1; a.nsplit = 1; a.mode = CM_NONE; a.res_scale = 1.f;
}
inline void setw(ConvArgs& a, const ConvP& p, bool dgrad) {
    a.w = dgrad ? p.wd : p.wf;
    a.wb = dgrad ? (const void*)p.wbd : (const void*)p.wbf;
    a.wh = dgrad ? (const void*)p.whd : (const void*)p.whf;
    const bool folded = p.wpb && p.poly_dgrad == dgrad;      // (plan_conv takes them on the up / zero-insert launches it routes polyphase)
    a.wpb = folded ? p.wpb : nullptr;
    a.wph = folded ? p.wph : nullptr;
    a.wqb = dgrad ? p.wqb : nullptr;
    a.wqh = dgrad ? p.wqh : nullptr;
}

// A tensor as one launch sees it: base, sample stride, extents.  Stands in for its base pointer where a launcher takes one.
struct TView {
    float* p; long bs; int C, H, W;
    operator float*() const { return p; }
};
// tensor `id` of the program in an activation arena
inline TView tview(const loco_ctx* c, float* arena, int id) {
    const Tens& t = c->tens[id];
    return {arena + t.off, c->prog->per_sample, t.C, t.H, t.W};
}
// a caller's read-only buffer (x, V, ge): only ever the `in` of a launch
inline TView tview_in(const float* p, long bs, int C, int H, int W) { return {const_cast<float*>(p), bs, C, H, W}; }
// The geometry every conv launch has: defaults, in / out, the operator's weights (dgrad: of the transposed map), B, and no
// padding for a 1x1.  Everything else stays at conv_defaults' value for the call site to set: bias, residual, mode, resampling.
inline ConvArgs conv_args(const TView& in, const ConvP& w, bool dgrad, const TView& out, int B, int ksize) {
    ConvArgs a; conv_defaults(a);
    a.in = in.p; a.in_bs = in.bs; a.Cin = in.C; a.Hin = in.H; a.Win = in.W;
    setw(a, w, dgrad);
    a.out = out.p; a.out_bs = out.bs; a.Cout = out.C; a.Hout = out.H; a.Wout = out.W; a.B = B;
    if (ksize == 1) a.pad = 0;
    return a;
}
bool run_conv(loco_ctx* c, const ConvArgs& a0, int taps, hipStream_t st, const StatReq* rq = nullptr,
              const ConvArgs* second = nullptr);

// the text cross-attention stage of an attention block (engine.hip)
struct XA {                     // shape and constants of one stage; the tensors of a pass are arguments of xa_forward / xa_linear
    loco_ctx* c; hipStream_t st; int B; int C, T, NH, CH, L, Lp;       // L real context rows of the Lp padded ones
    float scale;
    const float *xK, *xV;       // K_ctx, V_ctx [C][Lp]
    const float* colbias;       // [Lp]: 0 / -1e30, the key padding of the forward scores
    long xs, ss;                // sample stride of the [C][T] tensors (q, o, their tangents / cotangents) and of the score matrices
};
void xa_forward(const XA& x, const float* Xq, float* P, float* O);
void xa_linear(const XA& x, const float* X, const float* K1, const float* K2, float* P, float* S, float* O);
// behind the cotangent's xa_linear: the stage's term of c->ctx_G (engine.hip)
int xa_context_grad(const XA& x, const Op& op, const float* go, const float* q, const float* P, float* S);

// the multi-head self-attention core (engine.hip)
struct Attn {
    loco_ctx* c; hipStream_t st;
    int B, T, NH, CH, Lt, Tk;       // Lt text key columns (0: none) ahead of the T image ones, Tk = Lt + T
    long HS, SS, OS, KS;            // head strides: q / k / v (inside op.qkv in the engine), S, o, K_text / V_text
    float scale;
    bool pair;                      // the tangent may K-concatenate its two product pairs (attn_tangent)
    // the primal (B = 1) q, k, v, P = softmax, o -- read by the tangent and the cotangent
    const float *q, *k, *v, *P, *o;
    // this pass's tensors, B samples / probes: the forward's q, k, v -> S (scores, then P), o; the tangent's dq, dk, dv -> do with
    // the scratch dS; the cotangent's g_o -> g_q, g_k, g_v with the scratch g_S.  Sample strides: bq (q-like), bS (scores), bo (o-like)
    float *tq, *tk, *tv, *tS, *to;
    long bq, bS, bo;
    const float *kt, *vt;           // K_text, V_text [NH][CH][Lt] (Lt > 0)
    const float* colbias;           // [Lt]: 0 / -1e30, the key padding of the forward text scores
    float* delta;                   // scratch [B][NH][T] of the flash cotangent
    unsigned char* ws; size_t ws_bytes;      // record workspace of the flash kernels (nullptr / too small: the converting kernels)
    // the tangent / cotangent kernels of attn_flash.hip take this shape (no [T x Tk] matrix per probe)
    bool flash() const {
        return c->flash_attn && c->prec >= 1 && (Lt ? attn_flash_text_supported(T, CH, Lt) : attn_flash_supported(T, CH));
    }
};
AttnFlashArgs attn_flash_args(const Attn& s);
void attn_forward(const Attn& s);
void attn_tangent(const Attn& s);
void attn_cotangent(const Attn& s);

}  // namespace eng
}  // namespace loco
