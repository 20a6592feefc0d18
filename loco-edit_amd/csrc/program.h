// The U-Net program: which tensors exist and where they live in the per-sample arena, which ops run in which order, which
// statistics blocks and {S, xhat} cache ranges their norms own, and the ordered parameter list.  Host data only: no type here
// holds a pointer, and a Program is immutable once build_program has returned.  engine.hip binds device weights and
// per-context state to it; tests/c/program_check.cpp checks it on the CPU.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/loco_hip.h"

namespace loco {

struct TensPlan {
    long off; int C, H, W;             // offset (floats) in the per-sample layout, shape
    int cons_op = -1, cons_norm = 0;   // op whose norm (1: n1, 2: nx) takes its statistics over exactly this tensor, or -1
    // channel concatenation [cat_a | cat_b] consumed by a norm (the up-path ResBlocks read torch.cat([h, skip])): the two parts
    // are tensors of their own inside the concatenation's storage, each written by its own conv
    int cat_a = -1, cat_b = -1, cat_of = -1;
};

struct NormPlan {
    int C = 0;
    long soff = 0;      // offset into a stats arena
    long sx_off = -1;   // offset (in float2) into the primal {S, xhat} cache, -1: none
    float eps = 0.f;    // 0: cfg.gn_eps; the SpatialTransformer's GroupNorm has its own (1e-6)
};

enum OpKind { OP_CONV_IN, OP_RES, OP_ATTN, OP_DOWN, OP_UP, OP_OUT, OP_CONV, OP_XFMR };   // OP_CONV: plain conv, tensor -> tensor
// OP_XFMR tensors (latent-diffusion SpatialTransformer, depth 1), all [C][T] unless noted
enum XT { X_G0, X_H0, X_A1, X_QKV, X_S, X_O, X_H1, X_A2, X_XQ, X_XS, X_XO, X_H2, X_A3, X_F, X_GG, X_H3, X_LN1, X_LN2, X_LN3, X_NT };

struct OpPlan {
    OpKind kind;
    std::string name;
    int in = -1, out = -1;        // tensor ids
    int h1 = -1, a1 = -1;         // RES: conv1 output; cotangent scratch with the input's shape
    int hn = -1, qkv = -1, S = -1, o = -1;   // ATTN
    int up = -1;                  // UP: cotangent scratch at the upsampled size
    int ap = -1, xu = -1;         // ADM up/down ResBlock: pooled activation (down), resampled shortcut input
    int updown = 0;               // RES: 0 none, 1 down (avg-pool 2x2 on both branches), 2 up (nearest x2)
    bool scale_shift = false;     // RES: GN(h)*(1+scale)+shift from the embedding (ADM); else conv1 += Linear(temb) (DDPM)
    int heads = 1;                // ATTN
    int ksize = 3;                // CONV_IN / CONV: 3, or 1 (post_quant_conv / quant_conv of the latent autoencoder)
    // ATTN with a text cross-attention stage behind it (cfg.context_dim > 0): xmid = output of the self-attention
    // stage, xhn = GN(xmid), xq = q projection [C][T], xS = scores / probabilities [heads][T][Lp], xo = attended values
    bool has_x = false;
    int xmid = -1, xhn = -1, xq = -1, xS = -1, xo = -1;
    // DeepFloyd-IF attention (cfg.added_kv): keys / values = [text ; image] in one softmax behind the block's own GroupNorm of
    // the states (`norm_encoder`); S is [heads][T][Lp + T] with the (padded, masked) text columns first
    bool added_kv = false;
    bool in_is_skip = false;
    bool has_nin = false;
    bool has_temb = true;         // RES: false for the embedding-free blocks of the latent autoencoder (arch 2, 3)
    bool sym_down = false;        // DOWN: conv3 stride 2 with symmetric padding 1 (guided-diffusion Downsample) instead of (0,1,0,1)
    int xt[X_NT] = {};            // XFMR: tensors
    NormPlan n1, n2, nx;          // RES norm1 / norm2, ATTN norm (n1) and cross-attention norm (nx), OUT norm_out (n1)
    // parameter name stems in the reference state_dict
    std::string pn_n1, pn_c1, pn_emb, pn_n2, pn_c2, pn_skip, pn_qkv, pn_proj, pn_conv;
    bool has_ctx_kv() const { return kind == OP_XFMR || (kind == OP_ATTN && (has_x || added_kv)); }   // projects the prompt states
};

struct ParamDecl { std::string name; std::vector<int64_t> shape; };

struct Program {
    loco_unet_cfg cfg;
    float res_scale = 1.f;         // cfg.res_scale (0 -> 1): ResBlock output = (shortcut + h) * res_scale
    std::vector<TensPlan> tens;
    std::vector<OpPlan> ops;
    long per_sample = 0;           // floats per sample in an activation arena
    long stats_per_sample = 0;     // floats per sample in a stats arena
    long sx_total = 0;             // float2 entries of the primal {S, xhat} cache
    int n_in = 0;                  // C*H*W of the network input (image / latent)
    int n_out = 0;                 // C*H*W of the network output (= n_in for the denoisers; the decoded image for arch 2)
    int eps_t = -1;                // tensor id of the network output
    // h-space tap (the reference's get_h(op='mid', block_idx=0)): the output of the middle block's last op, which is the first part
    // of the first up-path concatenation.  -1 / -1 / 0 for the latent decoder and encoder (arch 2, 3), which have no tap.
    int h_t = -1;                  // tensor id of h
    int h_last_op = -1;            // index of the op that writes it: ops 0..h_last_op are the encoder half, the rest the decoder half
    int n_h = 0;                   // C*H*W of h
    int ctx_Lp = 0;                // context length padded to a multiple of 64 (score row length of the cross-attention)
    long attn_dmax = 1;            // heads * tokens of the largest attention
    long max_tensor = 0;           // C*H*W of the largest tensor
    std::vector<ParamDecl> params; // in state_dict order of the reference
};

// Validates the configuration and builds its program.  0, or -2 with *err set (the refusals loco_create reports).
int build_program(const loco_unet_cfg& cfg, Program* out, std::string* err);

}  // namespace loco
