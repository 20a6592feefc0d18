// Host-side weight packing of the engine: a checkpoint's tensors (loco_load_param) into the layouts the kernels read -- fp32
// forward / dgrad, split-bf16 and f16 records, the folded polyphase operators -- uploaded once by finalize_params of the root
// context and bound into every context's Op views by bind_weights.  Decides nothing at run time.
#include <atomic>
#include <cmath>
#include <cstring>
#include <thread>

#include "engine_internal.h"

namespace loco {
namespace eng {

static inline uint16_t f2bf(float f) {
    uint32_t u; std::memcpy(&u, &f, 4);
    u += 0x7FFFu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
static inline float bf2f(uint16_t h) {
    uint32_t u = (uint32_t)h << 16; float f; std::memcpy(&f, &u, 4); return f;
}
// Host-side layout building is split over threads (independent output rows): an 860 M-parameter denoiser has six layouts of
// every operator to build, single-threaded 22 s per engine context (three contexts per T-LOCO object).
template <typename F>
static void parallel_for(int n, size_t work, F fn) {
    unsigned nt = std::thread::hardware_concurrency();
    if (nt > 16) nt = 16;
    if ((int)nt > n) nt = (unsigned)n;
    if (nt <= 1 || work < ((size_t)1 << 18)) { for (int i = 0; i < n; ++i) fn(i); return; }
    std::atomic<int> next{0};
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; ++t)
        th.emplace_back([&]() { int i; while ((i = next.fetch_add(1)) < n) fn(i); });
    for (auto& t : th) t.join();
}

// split-bf16 records: W(o, i, t) for o < nout, i < nin -> [ceil(nin/16)][taps][noutP][32 x u16], 64-byte record
// per (chunk, tap, o): logical 16-byte pieces {hi k0-7, hi k8-15, lo k0-7, lo k8-15} stored at piece ^ ((o>>2)&3)
template <typename F>
static std::vector<float> build_records(int nin, int nout, int taps, F get) {
    int nch = (nin + 15) / 16, noutP = (nout + 31) & ~31;
    std::vector<uint16_t> rec((size_t)nch * taps * noutP * 32, 0);
    parallel_for(nch, (size_t)nin * nout * taps, [&](int ck) {
        for (int t = 0; t < taps; ++t)
            for (int o = 0; o < nout; ++o) {
                uint16_t* r = rec.data() + (((size_t)ck * taps + t) * noutP + o) * 32;
                int sw = (o >> 2) & 3;
                for (int k = 0; k < 16; ++k) {
                    int i = ck * 16 + k;
                    float v = (i < nin) ? get(o, i, t) : 0.f;
                    uint16_t h = f2bf(v);
                    uint16_t l = f2bf(v - bf2f(h));
                    int qh = (k >> 3) ^ sw, ql = (2 + (k >> 3)) ^ sw;
                    r[qh * 8 + (k & 7)] = h;
                    r[ql * 8 + (k & 7)] = l;
                }
            }
    });
    std::vector<float> out(rec.size() / 2);
    std::memcpy(out.data(), rec.data(), rec.size() * 2);
    return out;
}

// f16 records: W(o, i, t) -> [ceil(nin/16)][taps][noutP][16 x f16], 32-byte record per (chunk, tap, o): logical 16-byte
// pieces {k0-7, k8-15} stored at piece ^ ((o>>3)&1)
template <typename F>
static std::vector<float> build_records_f16(int nin, int nout, int taps, F get) {
    int nch = (nin + 15) / 16, noutP = (nout + 31) & ~31;
    std::vector<_Float16> rec((size_t)nch * taps * noutP * 16, (_Float16)0.f);
    parallel_for(nch, (size_t)nin * nout * taps, [&](int ck) {
        for (int t = 0; t < taps; ++t)
            for (int o = 0; o < nout; ++o) {
                _Float16* r = rec.data() + (((size_t)ck * taps + t) * noutP + o) * 16;
                int sw = (o >> 3) & 1;
                for (int k = 0; k < 16; ++k) {
                    int i = ck * 16 + k;
                    float v = (i < nin) ? get(o, i, t) : 0.f;
                    r[((k >> 3) ^ sw) * 8 + (k & 7)] = (_Float16)v;     // round to nearest even
                }
            }
    });
    std::vector<float> out(rec.size() / 2);
    std::memcpy(out.data(), rec.data(), rec.size() * 2);
    return out;
}

// weights [cout][cin][k][k] -> forward [cin][taps][coutP], dgrad [cout][taps][cinP] with flipped taps
// poly_kind >= 0 (PolyKind): also the folded polyphase operator of the forward (poly_dgrad false) or dgrad form
int make_conv(loco_ctx* c, const std::vector<const HostParam*>& ws, const std::vector<const HostParam*>& bs,
              ConvP* out, int row_limit, int poly_kind, bool poly_dgrad) {
    int cin = (int)ws[0]->shape[1], k = ws[0]->shape.size() > 2 ? (int)ws[0]->shape[2] : 1;
    int taps = ws[0]->shape.size() == 4 ? k * k : k;      // Conv2d, Conv1d (k=1) or Linear
    int cout = 0;
    for (auto* w : ws) cout += (int)w->shape[0];
    if (row_limit > 0 && ws.size() == 1 && row_limit < cout) cout = row_limit;   // eps half of a learn_sigma head
    int coutP = (cout + 31) & ~31, cinP = (cin + 31) & ~31;
    std::vector<float> wf((size_t)cin * taps * coutP, 0.f), wd((size_t)cout * taps * cinP, 0.f), bias(cout);
    int co0 = 0;
    for (size_t wi = 0; wi < ws.size(); ++wi) {
        const HostParam* w = ws[wi];
        int co_n = (int)w->shape[0];
        if (co_n > cout - co0) co_n = cout - co0;
        parallel_for(co_n, (size_t)co_n * cin * taps, [&](int co) {      // dgrad layout: one row block per cout
            for (int ci = 0; ci < cin; ++ci)
                for (int t = 0; t < taps; ++t)
                    wd[((size_t)(co0 + co) * taps + (taps - 1 - t)) * cinP + ci] = w->data[((size_t)co * cin + ci) * taps + t];
        });
        parallel_for(cin, (size_t)co_n * cin * taps, [&](int ci) {       // forward layout: one row block per cin
            for (int t = 0; t < taps; ++t)
                for (int co = 0; co < co_n; ++co)
                    wf[((size_t)ci * taps + t) * coutP + co0 + co] = w->data[((size_t)co * cin + ci) * taps + t];
        });
        for (int co = 0; co < co_n; ++co) bias[co0 + co] = bs[wi]->data[co];
        co0 += co_n;
    }
    out->cin = cin; out->cout = cout; out->taps = taps;
    if (upload(c, &out->wf, wf) || upload(c, &out->wd, wd) || upload(c, &out->bias, bias)) return -1;
    // the same two operators as split-bf16 records (read back from the fp32 layouts built above)
    auto fwd = [&](int o, int i, int t) { return wf[((size_t)i * taps + t) * coutP + o]; };
    auto dgr = [&](int o, int i, int t) { return wd[((size_t)i * taps + t) * cinP + o]; };   // o: cin index, i: cout index
    std::vector<float> rf = build_records(cin, cout, taps, fwd);
    std::vector<float> rd = build_records(cout, cin, taps, dgr);
    if (upload(c, &out->wbf, rf) || upload(c, &out->wbd, rd)) return -1;
    std::vector<float> hf = build_records_f16(cin, cout, taps, fwd);
    std::vector<float> hd = build_records_f16(cout, cin, taps, dgr);
    if (upload(c, &out->whf, hf) || upload(c, &out->whd, hd)) return -1;
    const int pin = poly_dgrad ? cout : cin, pout = poly_dgrad ? cin : cout;      // channels the folded operator reads / writes
    if (poly_kind >= 0 && taps == 9 && pin % 16 == 0 && pout % 128 == 0) {
        const int poutP = poly_dgrad ? cinP : coutP;
        std::vector<float> pf((size_t)pin * 16 * pout);
        polyphase_fold(poly_kind, pin, pout, (poly_dgrad ? wd : wf).data(), 1, 9L * poutP, poutP, pf.data());
        auto fold = [&](int o, int i, int t) { return pf[((size_t)i * 4 + t) * 4 * pout + o]; };
        std::vector<float> rp = build_records(pin, 4 * pout, 4, fold), hp = build_records_f16(pin, 4 * pout, 4, fold);
        if (upload(c, &out->wpb, rp) || upload(c, &out->wph, hp)) return -1;
        out->poly_dgrad = poly_dgrad;
    }
    if (poly_kind == POLY_UP && !poly_dgrad && taps == 9 && cout % 16 == 0 && cin % 128 == 0) {
        std::vector<float> qf((size_t)4 * cout * 4 * cinP, 0.f);      // [4 phases x cout][4][cinP]: the forward layout of a 4-tap operator
        polyphase_fold_in(cout, cin, wd.data(), 1, 9L * cinP, cinP, qf.data(), cinP);
        auto fold = [&](int o, int i, int t) { return qf[((size_t)i * 4 + t) * cinP + o]; };
        std::vector<float> rq = build_records(4 * cout, cin, 4, fold), hq = build_records_f16(4 * cout, cin, 4, fold);
        if (upload(c, &out->wqb, rq) || upload(c, &out->wqh, hq)) return -1;
    }
    return 0;
}
int make_conv1(loco_ctx* c, const std::string& name, ConvP* out, int row_limit, int poly_kind, bool poly_dgrad) {
    return make_conv(c, {&c->params[name + ".weight"]}, {&c->params[name + ".bias"]}, out, row_limit, poly_kind, poly_dgrad);
}
// the same operator with weight and bias multiplied by `s` (the ResBlock output scale of cfg.res_scale lives in conv2 / the shortcut)
int make_conv1_scaled(loco_ctx* c, const std::string& name, ConvP* out, float s) {
    if (s == 1.f) return make_conv1(c, name, out);
    HostParam w = c->params[name + ".weight"], b = c->params[name + ".bias"];
    for (float& v : w.data) v *= s;
    for (float& v : b.data) v *= s;
    return make_conv(c, {&w}, {&b}, out);
}
int make_norm(loco_ctx* c, const std::string& name, NormW* n) {
    if (upload(c, &n->gamma, c->params[name + ".weight"].data)) return -1;
    if (upload(c, &n->beta, c->params[name + ".bias"].data)) return -1;
    return 0;
}

// The weights of c->wts enter this context's Op views, and the buffers sized by them are allocated: the end of
// finalize_params for a created context, all a forked one needs.
int bind_weights(loco_ctx* c) {
    const Weights& W = *c->wts;
    for (size_t i = 0; i < c->ops.size(); ++i) {
        Op& v = c->ops[i];
        static_cast<OpWeights&>(v) = W.op[i];
        static_cast<NormW&>(v.n1) = v.g1; static_cast<NormW&>(v.n2) = v.g2; static_cast<NormW&>(v.nx) = v.gx;
    }
    if (dalloc(c, &c->tact, (size_t)c->cfg.ch * 4) || dalloc(c, &c->tproj, (size_t)(W.tproj_total > 0 ? W.tproj_total : 1))) return -1;
    c->finalized = true;
    return 0;
}

int finalize_params(loco_ctx* c) {
    if (c->finalized) return 0;
    for (const ParamDecl& d : c->prog->params)
        if (!c->params[d.name].loaded) { c->err = "parameter not loaded: " + d.name; return -1; }
    Weights& W = *c->wts;
    const loco_unet_cfg& cfg = c->cfg;
    int temb_ch = cfg.ch * 4;
    const bool adm = cfg.arch == 1;
    const std::string te0 = adm ? "time_embed.0" : "temb.dense.0", te1 = adm ? "time_embed.2" : "temb.dense.1";
    if (cfg.arch < 2) {
        if (upload(c, &W.td0w, c->params[te0 + ".weight"].data)) return -1;
        if (upload(c, &W.td0b, c->params[te0 + ".bias"].data)) return -1;
        if (upload(c, &W.td1w, c->params[te1 + ".weight"].data)) return -1;
        if (upload(c, &W.td1b, c->params[te1 + ".bias"].data)) return -1;
        if (cfg.time_cond_proj_dim > 0 && upload(c, &W.tcw, c->params["time_embed.cond_proj.weight"].data)) return -1;
    }
    // sinusoid frequencies exactly as torch computes them in fp32:
    //   DDPM: exp(float32(i) * float32(-ln(1e4)/(half-1)))            (diffusion.py:797-798)
    //   ADM : exp(float32(-ln(1e4)) * float32(i) / float32(half))     (guided_diffusion/nn.py:113-115)
    {
        int half = cfg.ch / 2;
        std::vector<float> f(half);
        for (int i = 0; i < half; ++i) {
            float x;
            if (adm) x = ((float)(-std::log(10000.0)) * (float)i) / (float)half;
            else x = (float)i * (float)(-(std::log(10000.0) / (double)(half - 1)));
            f[i] = (float)std::exp((double)x);
        }
        if (upload(c, &W.freq, f)) return -1;
    }
    std::vector<float> tpw, tpb;
    for (size_t oi = 0; oi < W.op.size(); ++oi) {
        const OpPlan& op = c->prog->ops[oi];
        OpWeights& ow = W.op[oi];
        switch (op.kind) {
            case OP_CONV_IN: case OP_CONV: if (make_conv1(c, op.pn_conv, &ow.conv)) return -1; break;
            case OP_RES: {
                if (make_norm(c, op.pn_n1, &ow.g1) || make_norm(c, op.pn_n2, &ow.g2)) return -1;
                if (make_conv1(c, op.pn_c1, &ow.c1) || make_conv1_scaled(c, op.pn_c2, &ow.c2, c->prog->res_scale)) return -1;
                if (op.has_nin && make_conv1_scaled(c, op.pn_skip, &ow.nin, c->prog->res_scale)) return -1;
                if (!op.has_temb) break;
                ow.tproj_off = (long)tpb.size();
                auto& w = c->params[op.pn_emb + ".weight"].data;
                auto& b = c->params[op.pn_emb + ".bias"].data;
                tpw.insert(tpw.end(), w.begin(), w.end());
                tpb.insert(tpb.end(), b.begin(), b.end());
                break;
            }
            case OP_ATTN: {
                if (make_norm(c, op.pn_n1, &ow.g1)) return -1;
                if (adm) {
                    if (make_conv1(c, op.pn_qkv, &ow.qkvc)) return -1;
                } else if (make_conv(c, {&c->params[op.name + ".q.weight"], &c->params[op.name + ".k.weight"],
                                         &c->params[op.name + ".v.weight"]},
                                     {&c->params[op.name + ".q.bias"], &c->params[op.name + ".k.bias"],
                                      &c->params[op.name + ".v.bias"]}, &ow.qkvc)) return -1;
                if (make_conv1(c, op.pn_proj, &ow.proj)) return -1;
                if (op.added_kv) {
                    // encoder_kv rows of head h are [k_h (CH) | v_h (CH)] (QKVAttention of deepfloyd_if: the states' projection is
                    // split per head like qkv): un-interleave into the key and the value map, rows ordered (head, channel)
                    const int C = c->tens[op.in].C, NH = op.heads, CH = C / NH, D = c->cfg.context_dim;
                    const HostParam& w = c->params[op.name + ".encoder_kv.weight"];
                    const HostParam& b = c->params[op.name + ".encoder_kv.bias"];
                    std::vector<float> kw((size_t)C * D), vw((size_t)C * D), kb(C), vb(C);
                    for (int h = 0; h < NH; ++h)
                        for (int i = 0; i < CH; ++i) {
                            const size_t rk = (size_t)h * 2 * CH + i, rv = rk + CH, r = (size_t)h * CH + i;
                            std::copy(w.data.begin() + rk * D, w.data.begin() + (rk + 1) * D, kw.begin() + r * D);
                            std::copy(w.data.begin() + rv * D, w.data.begin() + (rv + 1) * D, vw.begin() + r * D);
                            kb[r] = b.data[rk]; vb[r] = b.data[rv];
                        }
                    if (upload(c, &ow.xkw, kw) || upload(c, &ow.xkb, kb) || upload(c, &ow.xvw, vw) || upload(c, &ow.xvb, vb) ||
                        upload(c, &ow.xng, c->params[op.name + ".norm_encoder.weight"].data) ||
                        upload(c, &ow.xnb, c->params[op.name + ".norm_encoder.bias"].data)) return -1;
                }
                if (op.has_x) {
                    const std::string x = op.name + ".xattn";
                    if (make_norm(c, x + ".norm", &ow.gx) || make_conv1(c, x + ".q", &ow.xqc) ||
                        make_conv1(c, x + ".proj_out", &ow.xproj)) return -1;
                    if (upload(c, &ow.xkw, c->params[x + ".k.weight"].data) || upload(c, &ow.xkb, c->params[x + ".k.bias"].data) ||
                        upload(c, &ow.xvw, c->params[x + ".v.weight"].data) || upload(c, &ow.xvb, c->params[x + ".v.bias"].data))
                        return -1;
                }
                break;
            }
            case OP_DOWN: case OP_UP: {
                // (the folded polyphase operators: the up conv's forward form, the down conv's zero-insert data gradient)
                const int pk = op.kind == OP_UP ? POLY_UP : (op.sym_down ? POLY_ZINS_PAD1 : POLY_ZINS_PAD2);
                if (make_conv1(c, op.pn_conv, &ow.conv, -1, pk, op.kind == OP_DOWN)) return -1;
                break;
            }
            case OP_XFMR: {
                const int C = c->tens[op.in].C, NH = op.heads, CH = C / NH;
                const std::string b = op.name + ".transformer_blocks.0";
                HostParam zb; zb.shape = {8 * C}; zb.data.assign((size_t)8 * C, 0.f);       // bias of the bias-free maps
                auto nobias = [&](const std::string& w, ConvP* out) { return make_conv(c, {&c->params[w + ".weight"]}, {&zb}, out); };
                if (make_norm(c, op.pn_n1, &ow.g1) || make_conv1(c, op.name + ".proj_in", &ow.pj_in) ||
                    make_conv1(c, op.name + ".proj_out", &ow.pj_out)) return -1;
                const char* lnn[3] = {".norm1", ".norm2", ".norm3"};
                for (int i = 0; i < 3; ++i)
                    if (upload(c, &ow.lng[i], c->params[b + lnn[i] + ".weight"].data) ||
                        upload(c, &ow.lnb[i], c->params[b + lnn[i] + ".bias"].data)) return -1;
                {   // attn1: to_q / to_k / to_v fused into one [3C][C] map whose rows follow the per-head [q_h | k_h | v_h] layout
                    // the attention products address (head h of 'b n (h d)' = channels h*d .. h*d+d-1)
                    HostParam w; w.shape = {3 * C, C}; w.data.resize((size_t)3 * C * C);
                    const char* nm[3] = {".attn1.to_q.weight", ".attn1.to_k.weight", ".attn1.to_v.weight"};
                    for (int which = 0; which < 3; ++which) {
                        const std::vector<float>& src = c->params[b + nm[which]].data;
                        for (int h = 0; h < NH; ++h)
                            for (int j = 0; j < CH; ++j)
                                std::memcpy(&w.data[((size_t)(h * 3 + which) * CH + j) * C], &src[(size_t)(h * CH + j) * C], (size_t)C * 4);
                    }
                    if (make_conv(c, {&w}, {&zb}, &ow.qkvc)) return -1;
                }
                if (make_conv1(c, b + ".attn1.to_out.0", &ow.to_out1) || nobias(b + ".attn2.to_q", &ow.xqc) ||
                    make_conv1(c, b + ".attn2.to_out.0", &ow.to_out2) || make_conv1(c, b + ".ff.net.0.proj", &ow.ff1) ||
                    make_conv1(c, b + ".ff.net.2", &ow.ff2)) return -1;
                std::vector<float> z0((size_t)C, 0.f);
                if (upload(c, &ow.xkw, c->params[b + ".attn2.to_k.weight"].data) || upload(c, &ow.xkb, z0) ||
                    upload(c, &ow.xvw, c->params[b + ".attn2.to_v.weight"].data) || upload(c, &ow.xvb, z0)) return -1;
                break;
            }
            case OP_OUT:
                if (make_norm(c, op.pn_n1, &ow.g1) || make_conv1(c, op.pn_conv, &ow.conv, cfg.out_ch)) return -1;
                break;
        }
    }
    W.tproj_total = (long)tpb.size();
    if (upload(c, &W.tp_w, tpw) || upload(c, &W.tp_b, tpb)) return -1;
    // FLOP model (2*MAC): convolutions + attention products
    double fl = 0.0;
    for (size_t oi = 0; oi < W.op.size(); ++oi) {
        const OpPlan& op = c->prog->ops[oi];
        const OpWeights& ow = W.op[oi];
        auto convf = [&](const ConvP& p, int H, int W) { fl += 2.0 * p.cin * p.cout * p.taps * (double)H * W; };
        const Tens& to = c->tens[op.out];
        switch (op.kind) {
            case OP_CONV_IN: case OP_CONV: case OP_DOWN: case OP_UP: case OP_OUT: convf(ow.conv, to.H, to.W); break;
            case OP_RES:
                convf(ow.c1, to.H, to.W); convf(ow.c2, to.H, to.W);
                if (op.has_nin) convf(ow.nin, to.H, to.W);
                break;
            case OP_XFMR: {
                for (const ConvP* p : {&ow.pj_in, &ow.qkvc, &ow.to_out1, &ow.xqc, &ow.to_out2, &ow.ff1, &ow.ff2, &ow.pj_out}) convf(*p, to.H, to.W);
                double T = (double)to.H * to.W;
                fl += 2.0 * 2.0 * T * T * to.C + 2.0 * 2.0 * T * c->cfg.context_len * to.C;
                break;
            }
            case OP_ATTN: {
                convf(ow.qkvc, to.H, to.W); convf(ow.proj, to.H, to.W);
                double T = (double)to.H * to.W;
                fl += 2.0 * 2.0 * T * T * to.C;
                if (op.has_x) {
                    convf(ow.xqc, to.H, to.W); convf(ow.xproj, to.H, to.W);
                    fl += 2.0 * 2.0 * T * c->cfg.context_len * to.C;
                }
                break;
            }
        }
    }
    W.flops = fl;
    // host copies are no longer needed
    for (auto& kv : c->params) { std::vector<float>().swap(kv.second.data); }
    return bind_weights(c);
}

}  // namespace eng
}  // namespace loco
