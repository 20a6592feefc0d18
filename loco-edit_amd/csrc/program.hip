// build_program: configuration -> Program (program.h).  Host code only, like conv_plan.hip: no kernels, no HIP runtime calls;
// compiles with plain g++ (tests/test_program_host.py sweeps every preset on the CPU).
//
// Memory plan: every logical tensor of the network has a fixed offset in a per-sample layout, assigned in creation order.
// Skip tensors are placed directly inside the concatenation buffer of the up-block that consumes them (torch.cat of reference
// diffusion.py:186 is never materialised).
//
// Four architectures, one set of block constructors (Builder): 0 Ho-DDPM (reference diffusion.py:22-200), 1 the
// guided-diffusion family (guided_diffusion/unet.py:398-684: ADM / P2, latent-diffusion, DeepFloyd-IF), 2 / 3 the decoder /
// encoder of the latent autoencoder (diffusers AutoencoderKL: the DDPM module tree without skips and time embedding).
#include "program.h"

#include <algorithm>

namespace loco {
namespace {

// parameter-name stems of the two state_dict families
struct Names {
    const char *n1, *c1, *emb, *n2, *c2, *skip;   // ResBlock
    const char *qkv;                              // attention: fused qkv Conv1d, or nullptr for separate q / k / v 1x1 convs
    const char *out_norm, *out_conv, *te0, *te1;  // output head, time-embedding MLP
};
const Names DDPM_NAMES = {".norm1", ".conv1", ".temb_proj", ".norm2", ".conv2", ".nin_shortcut", nullptr,
                          "norm_out", "conv_out", "temb.dense.0", "temb.dense.1"};
const Names ADM_NAMES = {".in_layers.0", ".in_layers.2", ".emb_layers.1", ".out_layers.0", ".out_layers.3", ".skip_connection", ".qkv",
                         "out.0", "out.2", "time_embed.0", "time_embed.2"};

long align64(long v) { return (v + 63) & ~63L; }
std::string num(int v) { return std::to_string(v); }

struct Builder {
    Program& p;
    const loco_unet_cfg& cfg;
    const bool adm;
    const Names& nm;
    Builder(Program& prog) : p(prog), cfg(prog.cfg), adm(prog.cfg.arch == 1), nm(adm ? ADM_NAMES : DDPM_NAMES) {}

    int tensor(int C, int H, int W, long off = -1) {
        TensPlan t;
        t.C = C; t.H = H; t.W = W; t.off = off;
        if (off < 0) { t.off = p.per_sample; p.per_sample += align64((long)C * H * W); }
        p.tens.push_back(t);
        return (int)p.tens.size() - 1;
    }
    int like(int id, int C = 0) { const TensPlan t = p.tens[id]; return tensor(C ? C : t.C, t.H, t.W); }
    // stats layout per norm: sc[C], sh[C], mr[2G], tst[2G], tc[2C]; `cache_hw` > 0: the norm's input keeps a primal {S, xhat} cache
    NormPlan norm(int C, int cache_hw = 0) {
        NormPlan n;
        n.C = C;
        n.soff = p.stats_per_sample;
        p.stats_per_sample += align64(4L * C + 4L * cfg.gn_groups);
        if (cache_hw) { n.sx_off = p.sx_total; p.sx_total += (long)C * cache_hw; }
        return n;
    }
    bool attn_at(int res) const {
        for (int i = 0; i < cfg.num_attn_res; ++i)
            if (cfg.attn_resolutions[i] == res) return true;
        return false;
    }
    int push(const OpPlan& op) { p.ops.push_back(op); return op.out; }
    // the h-space tap: `tid` is the output of the op pushed last (the middle block's last op)
    void tap(int tid) {
        const TensPlan& t = p.tens[tid];
        p.h_t = tid; p.h_last_op = (int)p.ops.size() - 1; p.n_h = t.C * t.H * t.W;
    }

    // plain conv ops: CONV_IN (in = -1), CONV, DOWN, UP; the parameter stem is the op's name
    OpPlan conv_op(OpKind kind, const std::string& name, int in_t, int out_t) {
        OpPlan o; o.kind = kind; o.name = o.pn_conv = name; o.in = in_t; o.out = out_t;
        return o;
    }
    int up_conv(const std::string& name, int in_t, int out_t) {      // nearest x2 + conv3
        OpPlan u = conv_op(OP_UP, name, in_t, out_t);
        u.up = like(out_t);
        return push(u);
    }
    // ResBlock in_t -> out_t (both exist): scratch tensors, norms, names.  updown: 1 avg-pool / 2 nearest on both branches
    int resblock(const std::string& name, int in_t, int out_t, bool in_is_skip = false, int updown = 0) {
        OpPlan r; r.kind = OP_RES; r.name = name; r.in = in_t; r.out = out_t; r.updown = updown; r.in_is_skip = in_is_skip;
        r.has_temb = cfg.arch < 2;
        r.scale_shift = adm && cfg.scale_shift_norm != 0;
        const TensPlan ti = p.tens[in_t], to = p.tens[out_t];
        r.has_nin = (ti.C != to.C);
        r.h1 = like(out_t);
        r.a1 = like(in_t);
        if (updown) r.xu = tensor(ti.C, to.H, to.W);
        if (updown == 1) r.ap = tensor(ti.C, to.H, to.W);
        r.n1 = norm(ti.C, ti.H * ti.W); r.n2 = norm(to.C, to.H * to.W);
        r.pn_n1 = name + nm.n1; r.pn_c1 = name + nm.c1; r.pn_n2 = name + nm.n2; r.pn_c2 = name + nm.c2; r.pn_skip = name + nm.skip;
        if (r.has_temb) r.pn_emb = name + nm.emb;
        return push(r);
    }
    int resblock_new(const std::string& name, int in_t, int cout) { return resblock(name, in_t, like(in_t, cout)); }   // output allocated here
    int heads_of(int C) const {
        if (!adm) return 1;
        return cfg.num_heads > 0 ? cfg.num_heads : (cfg.num_head_channels > 0 ? C / cfg.num_head_channels : 1);
    }
    // attention block in_t -> out_t: plain self-attention; with added text keys / values (cfg.added_kv); with a text
    // cross-attention stage behind it (cfg.context_dim > 0); or, with cfg.transformer_depth > 0, the SpatialTransformer
    int attn(const std::string& name, int in_t, int out_t) {
        if (adm && cfg.transformer_depth > 0) return xfmr(name, in_t, out_t);
        OpPlan a; a.kind = OP_ATTN; a.name = name; a.in = in_t; a.out = out_t;
        const TensPlan t = p.tens[in_t];
        const int T = t.H * t.W;
        a.heads = heads_of(t.C);
        a.added_kv = adm && cfg.added_kv != 0;
        a.hn = like(in_t);
        a.qkv = like(in_t, 3 * t.C);
        a.S = tensor(a.heads, T, a.added_kv ? p.ctx_Lp + T : T);
        a.o = like(in_t);
        a.n1 = norm(t.C);
        a.pn_n1 = name + ".norm"; a.pn_proj = name + ".proj_out";
        if (nm.qkv) a.pn_qkv = name + nm.qkv;
        if (adm && cfg.context_dim > 0 && !a.added_kv) {
            a.has_x = true;
            a.xmid = like(in_t); a.xhn = like(in_t); a.xq = like(in_t);
            a.xS = tensor(a.heads, T, p.ctx_Lp);
            a.xo = like(in_t);
            a.nx = norm(t.C);
        }
        return push(a);
    }
    int attn_new(const std::string& name, int in_t) { return attn(name, in_t, like(in_t)); }
    int xfmr(const std::string& name, int in_t, int out_t) {
        OpPlan a; a.kind = OP_XFMR; a.name = name; a.in = in_t; a.out = out_t;
        const TensPlan t = p.tens[in_t];
        const int T = t.H * t.W, C = t.C;
        a.heads = heads_of(C);
        a.has_x = true;
        const int chan[X_NT] = {C, C, C, 3 * C, 0, C, C, C, C, 0, C, C, C, 8 * C, 4 * C, C, 0, 0, 0};   // 0: not [C][T], below
        for (int k = 0; k < X_NT; ++k) {
            if (chan[k]) a.xt[k] = like(in_t, chan[k]);
            else if (k == X_S) a.xt[k] = tensor(a.heads, T, T);
            else if (k == X_XS) a.xt[k] = tensor(a.heads, T, p.ctx_Lp);
            else a.xt[k] = tensor(2, 1, T);      // LayerNorm {mean, rstd} per token
        }
        // the attention helpers address the block through the ATTN field names
        a.qkv = a.xt[X_QKV]; a.S = a.xt[X_S]; a.o = a.xt[X_O]; a.xq = a.xt[X_XQ]; a.xS = a.xt[X_XS]; a.xo = a.xt[X_XO];
        a.n1 = norm(C); a.n1.eps = 1e-6f;
        a.pn_n1 = name + ".norm";
        return push(a);
    }
    // output head: GroupNorm, activation, conv3 to out_ch at R x R
    int head(const std::string& name, int in_t, int R) {
        OpPlan o; o.kind = OP_OUT; o.name = name; o.in = in_t;
        const int C = p.tens[in_t].C;
        o.out = tensor(cfg.out_ch, R, R);
        o.a1 = tensor(C, R, R);
        o.n1 = norm(C, p.tens[in_t].H * p.tens[in_t].W);
        o.pn_n1 = nm.out_norm; o.pn_conv = nm.out_conv;
        return p.eps_t = push(o);
    }

    // Skip stack of a U-Net (DDPM and ADM): the down path pushes conv_in (c0 channels), every block's output and every
    // downsample's; up block j pops from the back and reads [h_prev | skip], so both are placed inside its concatenation buffer.
    struct Skips { std::vector<int> cat, skip, hprev; };
    bool place_skips(int c0, Skips* s, std::string* err) {
        const int nlev = cfg.num_levels;
        struct Sk { int C, H; };
        std::vector<Sk> hs;
        int res = cfg.resolution, c = c0;
        hs.push_back({c, res});
        for (int l = 0; l < nlev; ++l) {
            for (int b = 0; b < cfg.num_res_blocks; ++b) hs.push_back({c = cfg.ch * cfg.ch_mult[l], res});
            if (l != nlev - 1) hs.push_back({c, res /= 2});
        }
        const int n = (int)hs.size();
        s->cat.assign(n, -1); s->skip.assign(n, -1); s->hprev.assign(n, -1);
        int C1 = c, j = 0;
        for (int l = nlev - 1; l >= 0; --l) {
            for (int b = 0; b < cfg.num_res_blocks + 1; ++b, ++j) {
                const Sk& sk = hs[n - 1 - j];
                if (sk.H != res) { *err = "internal: skip resolution mismatch"; return false; }
                const int cat = tensor(C1 + sk.C, res, res);
                const long base = p.tens[cat].off;
                const int a = s->hprev[j] = tensor(C1, res, res, base);
                const int b_ = s->skip[n - 1 - j] = tensor(sk.C, res, res, base + (long)C1 * res * res);
                s->cat[j] = cat;
                p.tens[cat].cat_a = a; p.tens[cat].cat_b = b_;
                p.tens[a].cat_of = p.tens[b_].cat_of = cat;
                C1 = cfg.ch * cfg.ch_mult[l];
            }
            if (l != 0) res *= 2;
        }
        return true;
    }

    bool ddpm(std::string* err);
    bool adm_unet(std::string* err);
    void decoder();
    void encoder();
    void analyse();
    void declare();
};

// mirrors DDPM.__init__ / forward, reference diffusion.py:22-200
bool Builder::ddpm(std::string* err) {
    const int ch = cfg.ch, nres = cfg.num_levels, R = cfg.resolution;
    Skips s;
    if (!place_skips(ch, &s, err)) return false;
    int res = R, si = 0;
    int cur = push(conv_op(OP_CONV_IN, "conv_in", -1, s.skip[si++]));
    for (int l = 0; l < nres; ++l) {
        const int block_out = ch * cfg.ch_mult[l];
        const std::string lv = "down." + num(l);
        for (int b = 0; b < cfg.num_res_blocks; ++b) {
            const bool at = attn_at(res);
            const int out_t = at ? tensor(block_out, res, res) : s.skip[si];
            resblock(lv + ".block." + num(b), cur, out_t, true);
            if (at) attn(lv + ".attn." + num(b), out_t, s.skip[si]);
            cur = s.skip[si++];
        }
        if (l != nres - 1) {
            OpPlan d = conv_op(OP_DOWN, lv + ".downsample.conv", cur, s.skip[si++]);
            d.in_is_skip = true;
            cur = push(d);
            res /= 2;
        }
    }
    cur = resblock("mid.block_1", cur, like(cur), true);
    {
        const int a_out = like(cur);
        cur = attn("mid.attn_1", cur, a_out);
    }
    cur = resblock("mid.block_2", cur, s.hprev[0]);
    tap(cur);
    int j = 0;
    for (int l = nres - 1; l >= 0; --l) {
        const int block_out = ch * cfg.ch_mult[l];
        const std::string lv = "up." + num(l);
        for (int b = 0; b < cfg.num_res_blocks + 1; ++b) {
            const bool at = attn_at(res), last_of_level = (b == cfg.num_res_blocks);
            // where the block's (or its attention's) output goes: the next concatenation, or a tensor of its own in front of
            // the upsample conv / the output head
            const int dest = last_of_level ? tensor(block_out, res, res) : s.hprev[j + 1];
            const int out_t = at ? tensor(block_out, res, res) : dest;
            resblock(lv + ".block." + num(b), s.cat[j], out_t);
            if (at) attn(lv + ".attn." + num(b), out_t, dest);
            cur = dest;
            ++j;
            if (last_of_level && l != 0) {
                cur = up_conv(lv + ".upsample.conv", cur, s.hprev[j]);
                res *= 2;
            }
        }
    }
    head("conv_out", cur, R);
    return true;
}

// guided-diffusion / P2 U-Net (reference guided_diffusion/unet.py:398-684 with P2_DICT script_util.py:166-190):
// input_blocks = conv, then per level {ResBlock [+Attention]} x num_res_blocks and a ResBlock(down) between levels;
// middle = Res, Attn, Res; output_blocks = {ResBlock(cat) [+Attention] [+ResBlock(up)]}; out = GN, SiLU, conv.
bool Builder::adm_unet(std::string* err) {
    const int mc = cfg.ch, nlev = cfg.num_levels, R = cfg.resolution;
    p.ctx_Lp = cfg.context_dim > 0 ? ((cfg.context_len + 63) / 64) * 64 : 0;
    Skips s;
    if (!place_skips(mc * cfg.ch_mult[0], &s, err)) return false;
    int si = 0, res = R, ib = 1;
    int cur = push(conv_op(OP_CONV_IN, "input_blocks.0.0", -1, s.skip[si++]));
    for (int l = 0; l < nlev; ++l) {
        for (int b = 0; b < cfg.num_res_blocks; ++b, ++ib) {
            const bool at = attn_at(res);
            const std::string nm_ = "input_blocks." + num(ib);
            const int out_t = at ? tensor(mc * cfg.ch_mult[l], res, res) : s.skip[si];
            resblock(nm_ + ".0", cur, out_t, true);
            if (at) attn(nm_ + ".1", out_t, s.skip[si]);
            cur = s.skip[si++];
        }
        if (l != nlev - 1) {
            const std::string nm_ = "input_blocks." + num(ib++);
            if (cfg.resblock_updown) {
                resblock(nm_ + ".0", cur, s.skip[si], true, 1);
            } else {        // Downsample(use_conv=True): conv3 stride 2 padding 1 (unet.py:113-142)
                OpPlan d = conv_op(OP_DOWN, nm_ + ".0.op", cur, s.skip[si]);
                d.in_is_skip = true; d.sym_down = true;
                push(d);
            }
            cur = s.skip[si++];
            res /= 2;
        }
    }
    cur = resblock("middle_block.0", cur, like(cur), true);
    {
        const int a_out = like(cur);
        cur = attn("middle_block.1", cur, a_out);
    }
    cur = resblock("middle_block.2", cur, s.hprev[0]);
    tap(cur);
    int j = 0;
    for (int l = nlev - 1; l >= 0; --l) {
        for (int i = 0; i < cfg.num_res_blocks + 1; ++i, ++j) {
            const int cout = mc * cfg.ch_mult[l];
            const bool at = attn_at(res);
            const bool has_up = (l != 0 && i == cfg.num_res_blocks), final_block = (l == 0 && i == cfg.num_res_blocks);
            const std::string nm_ = "output_blocks." + num(j);
            // destination of the block's last op: the next concatenation, or (final block) a tensor in front of the output head
            const int dest = final_block ? tensor(cout, res, res) : s.hprev[j + 1];
            int sub = 1;
            int last = resblock(nm_ + ".0", s.cat[j], (at || has_up) ? tensor(cout, res, res) : dest);
            if (at) {
                const int a_out = has_up ? tensor(cout, res, res) : dest;
                last = attn(nm_ + "." + num(sub++), last, a_out);
            }
            if (has_up) {
                if (cfg.resblock_updown) last = resblock(nm_ + "." + num(sub++), last, dest, false, 2);
                else last = up_conv(nm_ + "." + num(sub++) + ".conv", last, dest);   // Upsample(use_conv=True) (unet.py:83-110)
                res *= 2;
            }
            cur = last;
        }
    }
    head("out", cur, R);
    return true;
}

// Latent decoder (arch 2): the `Decoder` of the latent-diffusion autoencoder that `vae.decode` runs in the reference's
// Stable Diffusion path (edit.py:750, 770-771): post_quant_conv (1x1) and conv_in (z_channels -> ch*ch_mult[-1]) at the
// latent resolution R; mid.block_1, mid.attn_1, mid.block_2; for each level from the coarsest: num_res_blocks + 1
// ResnetBlocks [+ attention at cfg.attn_resolutions] and, except at level 0, nearest x2 + conv3; norm_out, SiLU,
// conv_out.  Output [out_ch, R * 2^(levels-1), same].
void Builder::decoder() {
    const int ch = cfg.ch, nlev = cfg.num_levels;
    int res = cfg.resolution;
    const int block_in = ch * cfg.ch_mult[nlev - 1];
    OpPlan pq = conv_op(OP_CONV_IN, "post_quant_conv", -1, tensor(cfg.in_channels, res, res));
    pq.ksize = 1;
    int cur = push(pq);
    cur = push(conv_op(OP_CONV, "conv_in", cur, tensor(block_in, res, res)));
    cur = resblock_new("mid.block_1", cur, block_in);
    cur = attn_new("mid.attn_1", cur);
    cur = resblock_new("mid.block_2", cur, block_in);
    for (int l = nlev - 1; l >= 0; --l) {
        const std::string lv = "up." + num(l);
        for (int b = 0; b < cfg.num_res_blocks + 1; ++b) {
            cur = resblock_new(lv + ".block." + num(b), cur, ch * cfg.ch_mult[l]);
            if (attn_at(res)) cur = attn_new(lv + ".attn." + num(b), cur);
        }
        if (l != 0) {
            res *= 2;
            cur = up_conv(lv + ".upsample.conv", cur, tensor(p.tens[cur].C, res, res));
        }
    }
    head("conv_out", cur, res);
}

// Latent encoder (arch 3): `vae.encode` of the reference's latent inversion (edit.py:594-597): conv_in at the image
// resolution R; per level num_res_blocks embedding-free ResnetBlocks and, except on the last level, pad (0,1,0,1) + conv3
// stride 2; mid block / attention / block; norm_out, SiLU, conv_out (2 z channels: mean | log-variance), 1x1 quant_conv.
// Output [out_ch, R >> (levels-1), same].
void Builder::encoder() {
    const int ch = cfg.ch, nlev = cfg.num_levels;
    int res = cfg.resolution;
    int cur = push(conv_op(OP_CONV_IN, "conv_in", -1, tensor(ch, res, res)));
    for (int l = 0; l < nlev; ++l) {
        const std::string lv = "down." + num(l);
        for (int b = 0; b < cfg.num_res_blocks; ++b) cur = resblock_new(lv + ".block." + num(b), cur, ch * cfg.ch_mult[l]);
        if (l != nlev - 1) {
            res /= 2;
            cur = push(conv_op(OP_DOWN, lv + ".downsample.conv", cur, tensor(ch * cfg.ch_mult[l], res, res)));
        }
    }
    const int block_in = p.tens[cur].C;
    cur = resblock_new("mid.block_1", cur, block_in);
    cur = attn_new("mid.attn_1", cur);
    cur = resblock_new("mid.block_2", cur, block_in);
    cur = head("conv_out", cur, res);
    OpPlan q = conv_op(OP_CONV, "quant_conv", cur, like(cur));
    q.ksize = 1;
    p.eps_t = push(q);
}

// Which norm takes its statistics over exactly which tensor (the conv that finishes that tensor delivers them), and the sizes
// the engine's scratch is cut from.  (Every concatenation place_skips made is the input of an up-path ResBlock, so a norm reads it.)
void Builder::analyse() {
    for (size_t i = 0; i < p.ops.size(); ++i) {
        const OpPlan& op = p.ops[i];
        if ((op.kind == OP_RES || op.kind == OP_ATTN || op.kind == OP_OUT || op.kind == OP_XFMR) && op.in >= 0) {
            p.tens[op.in].cons_op = (int)i; p.tens[op.in].cons_norm = 1;
        }
        if (op.kind == OP_ATTN && op.has_x) { p.tens[op.xmid].cons_op = (int)i; p.tens[op.xmid].cons_norm = 2; }
        if (op.kind == OP_ATTN || op.kind == OP_XFMR)
            p.attn_dmax = std::max(p.attn_dmax, (long)op.heads * p.tens[op.in].H * p.tens[op.in].W);
    }
    for (const TensPlan& t : p.tens) p.max_tensor = std::max(p.max_tensor, (long)t.C * t.H * t.W);
}

void Builder::declare() {
    auto param = [&](const std::string& name, std::vector<int64_t> shape) { p.params.push_back({name, std::move(shape)}); };
    auto conv = [&](const std::string& n, int cin, int cout, int k) { param(n + ".weight", {cout, cin, k, k}); param(n + ".bias", {cout}); };
    auto conv1d = [&](const std::string& n, int cin, int cout) { param(n + ".weight", {cout, cin, 1}); param(n + ".bias", {cout}); };
    auto lin = [&](const std::string& n, int cin, int cout) { param(n + ".weight", {cout, cin}); param(n + ".bias", {cout}); };
    auto gn = [&](const std::string& n, int C) { param(n + ".weight", {C}); param(n + ".bias", {C}); };
    const int temb_ch = cfg.ch * 4, D = cfg.context_dim;
    if (cfg.arch < 2) {
        lin(nm.te0, cfg.ch, temb_ch);
        lin(nm.te1, temb_ch, temb_ch);
        if (cfg.time_cond_proj_dim > 0) param("time_embed.cond_proj.weight", {cfg.ch, cfg.time_cond_proj_dim});   // no bias
    }
    for (const OpPlan& op : p.ops) {
        const int cin = op.in >= 0 ? p.tens[op.in].C : cfg.in_channels, cout = p.tens[op.out].C, C = cin;
        switch (op.kind) {
            case OP_CONV_IN: case OP_CONV: conv(op.pn_conv, cin, cout, op.ksize); break;
            case OP_DOWN: case OP_UP: conv(op.pn_conv, C, C, 3); break;
            case OP_RES:
                gn(op.pn_n1, cin);
                conv(op.pn_c1, cin, cout, 3);
                if (op.has_temb) lin(op.pn_emb, temb_ch, op.scale_shift ? 2 * cout : cout);
                gn(op.pn_n2, cout);
                conv(op.pn_c2, cout, cout, 3);
                if (op.has_nin) conv(op.pn_skip, cin, cout, 1);
                break;
            case OP_ATTN:
                gn(op.pn_n1, C);
                if (!adm) {
                    for (const char* q : {".q", ".k", ".v"}) conv(op.name + q, C, C, 1);
                    conv(op.pn_proj, C, C, 1);
                    break;
                }
                conv1d(op.pn_qkv, C, 3 * C);      // Conv1d weights [3C, C, 1] / [C, C, 1] (unet.py:286,296)
                conv1d(op.pn_proj, C, C);
                if (op.added_kv) {   // deepfloyd_if AttentionBlock: norm_encoder (GroupNorm over the states), encoder_kv Conv1d
                    gn(op.name + ".norm_encoder", D);
                    conv1d(op.name + ".encoder_kv", D, 2 * C);
                }
                if (op.has_x) {
                    const std::string x = op.name + ".xattn";
                    gn(x + ".norm", C);
                    conv1d(x + ".q", C, C);
                    lin(x + ".k", D, C);
                    lin(x + ".v", D, C);
                    conv1d(x + ".proj_out", C, C);
                }
                break;
            case OP_XFMR: {      // latent-diffusion SpatialTransformer, depth 1 (ldm/modules/attention.py parameter names)
                const std::string b = op.name + ".transformer_blocks.0";
                gn(op.pn_n1, C);
                conv(op.name + ".proj_in", C, C, 1);
                for (const char* n : {".norm1", ".norm2", ".norm3"}) gn(b + n, C);
                for (const char* n : {".attn1.to_q", ".attn1.to_k", ".attn1.to_v"}) param(b + n + ".weight", {C, C});
                lin(b + ".attn1.to_out.0", C, C);
                param(b + ".attn2.to_q.weight", {C, C});
                param(b + ".attn2.to_k.weight", {C, D});
                param(b + ".attn2.to_v.weight", {C, D});
                lin(b + ".attn2.to_out.0", C, C);
                lin(b + ".ff.net.0.proj", C, 8 * C);
                lin(b + ".ff.net.2", 4 * C, C);
                conv(op.name + ".proj_out", C, C, 1);
                break;
            }
            case OP_OUT:
                gn(op.pn_n1, C);
                conv(op.pn_conv, C, cfg.out_ch * (cfg.learn_sigma ? 2 : 1), 3);
                break;
        }
    }
}

const char* refuse(const loco_unet_cfg& cfg) {
    if (cfg.max_batch < 1 || cfg.num_levels < 1 || cfg.num_levels > 8) return "bad config";
    int r = cfg.resolution;
    for (int l = 0; l < cfg.num_levels - 1; ++l) r /= 2;
    if (cfg.arch == 2) r = cfg.resolution;      // decoder: `resolution` is the coarsest (latent) level
    if (cfg.arch > 3 || cfg.arch < 0) return "arch must be 0 (Ho-DDPM), 1 (guided-diffusion family), 2 (latent decoder) or 3 (latent encoder)";
    if (r < 8 || (cfg.resolution & (cfg.resolution - 1))) return "resolution must be a power of two with >= 8x8 at the coarsest level";
    if (cfg.ch % 32) return "ch must be a multiple of 32";
    if (cfg.act != 0 && cfg.act != 1) return "act must be 0 (SiLU) or 1 (GELU)";
    const bool scaled = cfg.res_scale != 0.f && cfg.res_scale != 1.f;
    if ((cfg.act != 0 || scaled || cfg.added_kv) && cfg.arch != 1) return "act / res_scale / added_kv belong to the guided-diffusion family (arch 1)";
    if (cfg.added_kv && (cfg.context_dim <= 0 || cfg.context_len <= 0 || cfg.transformer_depth != 0 || cfg.context_dim % cfg.gn_groups))
        return "added_kv needs context_dim (a multiple of gn_groups) and context_len > 0 and transformer_depth = 0";
    if (cfg.time_cond_proj_dim < 0 || (cfg.time_cond_proj_dim > 0 && cfg.arch != 1))
        return "time_cond_proj_dim must be >= 0 and belongs to the guided-diffusion family (arch 1)";
    return nullptr;
}

}  // namespace

int build_program(const loco_unet_cfg& cfg, Program* out, std::string* err) {
    if (const char* why = refuse(cfg)) { *err = why; return -2; }
    Program p;
    p.cfg = cfg;
    p.res_scale = cfg.res_scale == 0.f ? 1.f : cfg.res_scale;
    const int R = cfg.resolution, lev = cfg.num_levels - 1;
    p.n_in = cfg.in_channels * R * R;
    const int Rout = cfg.arch == 2 ? R << lev : cfg.arch == 3 ? R >> lev : R;
    p.n_out = cfg.out_ch * Rout * Rout;
    Builder b(p);
    switch (cfg.arch) {
        case 0: if (!b.ddpm(err)) return -2; break;
        case 1: if (!b.adm_unet(err)) return -2; break;
        case 2: b.decoder(); break;
        default: b.encoder(); break;
    }
    for (const OpPlan& op : p.ops)
        if (op.kind == OP_RES && op.updown && op.has_nin) { *err = "resampling ResBlock with a channel change is not supported"; return -2; }
    b.analyse();
    b.declare();
    *out = std::move(p);
    return 0;
}

}  // namespace loco
