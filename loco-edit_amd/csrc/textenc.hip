// CLIP text encoder of the Stable Diffusion paths (include/loco_hip.h loco_text_*): the CLIPTextModel that diffusers'
// StableDiffusionPipeline.encode_prompt runs (reference src/modules/edit.py:1187-1194), exact fp32 throughout.
//
// Layout: the activations of all n prompts of a call live channel-major in ONE [D][Tp] tensor, token column p * L + t
// (Tp = n * L rounded up to 16; the padding columns carry zeros through the embedding and stay independent of the real
// ones).  In that layout the linear layers are one launch_gemm_fixed each over all prompts (W [out][in] row-major as
// stored, so each layer's weights are read once per call), and LayerNorm is xfmr.hip's launch_ln_fwd unchanged.  New
// here, and shared with the T5 encoder (t5enc.hip) through textenc.h: the embedding gather, the self-attention of one
// (prompt, head) per workgroup in its two forms, and the staging of the token ids.  The layer's parameters and its seven
// launches are encoder_common.h's add_clip_layer / pre_ln_block, which the image tower (clipvis.hip) uses too; the transpose
// of the final states to [n][L][D] is encoder_kernels.hip's.  Every kernel computes a token column from that column (and,
// in the attention, from the columns of its own prompt) alone, in a fixed order: a prompt's rows are bit-identical whatever
// n and its position in the batch.
//
// Also here: the six loco_text_* functions of the handle base (textenc.h), which serve both encoders.
#include "textenc.h"

#include <cmath>

namespace loco {
namespace {

constexpr int PA_THREADS = 256, PA_WAVES = PA_THREADS / 64;

__global__ __launch_bounds__(256) void text_embed_kernel(const int* ids, int T, int Tp, int L, int D, const float* tok,
                                                         const float* pos, float* h) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)D * Tp) return;
    const int c = (int)(e / Tp), col = (int)(e % Tp);
    float v = 0.f;
    if (col < T) {
        v = tok[(long)ids[col] * D + c];
        if (pos) v += pos[(long)(col % L) * D + c];
    }
    h[e] = v;
}

// One workgroup per (prompt p, head h): K and V of the head ([hd][L] each) in LDS; each wave owns the query rows
// i = i0 + wave, lane j (and j + 64) the score against the live keys; fp32 softmax over the row (max / sum by shuffles),
// then lane c accumulates o[c] = sum_j P[j] V[c][j] in key order.  CAUSAL_SCALED (CLIP): key j is live for j <= i, score
// q_i . k_j * scale.  Otherwise (T5): live for j < len = lens[p] (1 <= len <= L, checked on the host), score
// q_i . k_j + bias_tab[h][j - i + L - 1], no scale; padded query rows (i >= len) are computed like the others.
template <bool CAUSAL_SCALED>
__global__ __launch_bounds__(PA_THREADS)
void prompt_attn_kernel(const float* qkv, long ld, int L, int inner, int hd, float scale, const float* bias_tab, const int* lens,
                        float* out) {
    extern __shared__ float sm[];
    float* Ks = sm;
    float* Vs = sm + hd * L;
    float* Ps = Vs + hd * L;               // [PA_WAVES][L]
    const int p = blockIdx.x, h = blockIdx.y;
    int len = 0;
    const float* bh = nullptr;
    if constexpr (!CAUSAL_SCALED) {
        len = lens[p];
        bh = bias_tab + (long)h * (2 * L - 1) + (L - 1);
    }
    const long col0 = (long)p * L;
    const float* q = qkv + (long)(h * hd) * ld + col0;
    const float* k = qkv + (long)(inner + h * hd) * ld + col0;
    const float* v = qkv + (long)(2 * inner + h * hd) * ld + col0;
    for (int e = threadIdx.x; e < hd * L; e += PA_THREADS) {
        const int c = e / L, t = e - c * L;
        Ks[e] = k[(long)c * ld + t];
        Vs[e] = v[(long)c * ld + t];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    float* pw = Ps + w * L;
    for (int i0 = 0; i0 < L; i0 += PA_WAVES) {
        const int i = i0 + w;                      // wave-uniform
        auto live = [&](int j) { return CAUSAL_SCALED ? j <= i : j < len; };
        if (i < L) {
            float s[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int j = lane + 64 * u;
                s[u] = -INFINITY;
                if (live(j)) {
                    float acc = 0.f;
                    for (int c = 0; c < hd; ++c) acc = fmaf(q[(long)c * ld + i], Ks[c * L + j], acc);
                    if constexpr (CAUSAL_SCALED) s[u] = acc * scale;
                    else s[u] = acc + bh[j - i];
                }
            }
            const float m = wave_max(fmaxf(s[0], s[1]));
            float e[2], sum = 0.f;
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                e[u] = live(lane + 64 * u) ? expf(s[u] - m) : 0.f;
                sum += e[u];
            }
            const float inv = 1.0f / wave_sum(sum);
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int j = lane + 64 * u;
                if (live(j)) pw[j] = e[u] * inv;
            }
        }
        __syncthreads();
        if (i < L) {
            for (int c = lane; c < hd; c += 64) {
                float acc = 0.f;
                for (int j = 0; live(j); ++j) acc = fmaf(pw[j], Vs[c * L + j], acc);
                out[(long)(h * hd + c) * ld + col0 + i] = acc;
            }
        }
        __syncthreads();
    }
}

}  // namespace

thread_local std::string g_text_create_err;

void launch_text_embed(const int* ids, int T, int Tp, int L, int D, const float* tok, const float* pos, float* h, hipStream_t st) {
    hipLaunchKernelGGL(text_embed_kernel, dim3(blocks256((long)D * Tp)), dim3(256), 0, st, ids, T, Tp, L, D, tok, pos, h);
}

size_t prompt_attn_lds_bytes(int hd, int L) { return (size_t)(2 * hd * L + PA_WAVES * L) * sizeof(float); }

void launch_prompt_attn(bool causal_scaled, const float* qkv, long ld, int n, int heads, int L, int inner, int hd, float scale,
                        const float* bias_tab, const int* lens, float* out, hipStream_t st) {
    auto kernel = causal_scaled ? prompt_attn_kernel<true> : prompt_attn_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(n, heads), dim3(PA_THREADS), prompt_attn_lds_bytes(hd, L), st, qkv, ld, L, inner, hd, scale, bias_tab,
                       lens, out);
}

int text_check_call(loco_text* t, const int32_t* ids_dev, int32_t n, const float* out_dev) {
    if (!ids_dev || !out_dev) return t->fail("loco_text_encode: null ids or out");
    if (n <= 0 || n > t->max_prompts)
        return t->fail("loco_text_encode: n = " + std::to_string(n) + " outside [1, max_prompts = " + std::to_string(t->max_prompts) + "]");
    return t->table.missing(t->err) ? -1 : 0;
}

int stage_ids(loco_text* t, const int32_t* ids_dev, int T, int L, int vocab, hipStream_t st) {
    if (hipMemcpyAsync(t->ids_host.data(), ids_dev, (size_t)T * sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return t->fail("loco_text_encode: reading the token ids failed");
    // an index past the table would read outside it
    for (int i = 0; i < T; ++i) {
        const int id = t->ids_host[i];
        if (id < 0 || id >= vocab)
            return t->fail("loco_text_encode: token id " + std::to_string(id) + " at prompt " + std::to_string(i / L) +
                           ", position " + std::to_string(i % L) + " outside [0, vocab = " + std::to_string(vocab) + ")");
    }
    if (hipMemcpyAsync(t->ids, t->ids_host.data(), (size_t)T * sizeof(int), hipMemcpyHostToDevice, st) != hipSuccess)
        return t->fail("loco_text_encode: copy of the token ids failed");
    return 0;
}

}  // namespace loco

using namespace loco;

namespace {

struct ClipText final : loco_text {
    loco_text_cfg cfg;
    float *pos = nullptr, *lnf_b = nullptr, *stats = nullptr;
    std::vector<PreLnLayer> layer;

    int encode(const int32_t* ids_dev, const int32_t* lens, int32_t n, float* out_dev, hipStream_t st) override;
    int encode_masked(const int32_t*, const int32_t*, int32_t, float*, hipStream_t) override {
        return fail("loco_text_encode_masked: this handle is a CLIP encoder (causal, no padding mask); use loco_text_encode");
    }
};

int ClipText::encode(const int32_t* ids_dev, const int32_t*, int32_t n, float* out_dev, hipStream_t st) {
    if (text_check_call(this, ids_dev, n, out_dev)) return -1;
    DeviceGuard dg(device);
    const int F = cfg.ffn, T = n * L, Tp = (T + 15) / 16 * 16;
    if (stage_ids(this, ids_dev, T, L, cfg.vocab, st)) return -1;
    launch_text_embed(ids, T, Tp, L, D, tok, pos, h, st);
    const float scale = 1.0f / std::sqrt((float)hd);
    const int gact = cfg.act == 0 ? GEMM_ACT_QUICK_GELU : GEMM_ACT_GELU;
    const PreLnBufs bufs{h, x, qkv, attn, h, f, h, stats, stats};      // every block in place on h
    for (const PreLnLayer& ly : layer)
        pre_ln_block(ly, bufs, D, F, Tp, cfg.ln_eps, gact, st, [&](const float* qkv_, float* attn_) {
            launch_prompt_attn(true, qkv_, (long)Tp, n, cfg.heads, L, D, hd, scale, nullptr, nullptr, attn_, st);
        });
    launch_ln_fwd(h, 0, 1, D, Tp, lnf_g, lnf_b, cfg.ln_eps, x, 0, stats, 0, st);
    launch_enc_transpose(x, Tp, T, D, out_dev, st);
    if (hipGetLastError() != hipSuccess) return fail("loco_text_encode: kernel launch failed");
    return 0;
}

}  // namespace

extern "C" {

int loco_text_create(const loco_text_cfg* cfg, int32_t device, int32_t max_prompts, loco_text** out) {
    auto refuse = [&](const loco_text_cfg& c) -> std::string {
        if (c.vocab <= 0 || c.width <= 0 || c.layers <= 0 || c.heads <= 0 || c.ffn <= 0 || c.positions <= 0 || max_prompts <= 0)
            return "vocab, width, layers, heads, ffn, positions and max_prompts must be positive";
        if (c.width % c.heads) return "width is not a multiple of heads";
        if (c.positions > 128) return "positions > 128 (the attention kernel holds 2 keys per lane)";
        if (c.act != 0 && c.act != 1) return "act must be 0 (quick_gelu) or 1 (gelu)";
        if (prompt_attn_lds_bytes(c.width / c.heads, c.positions) > 65536)
            return "head width x positions too large for the attention kernel's LDS (64 KiB)";
        return "";
    };
    return encoder_create<ClipText>("loco_text_create", g_text_create_err, cfg, device, out, refuse, [&](ClipText& t) {
        const loco_text_cfg& c = t.cfg = *cfg;
        t.max_prompts = max_prompts;
        t.L = c.positions; t.D = c.width; t.hd = c.width / c.heads;
        t.Tmax = (max_prompts * c.positions + 15) / 16 * 16;
        const long D = c.width, F = c.ffn, Tm = t.Tmax;
        // parameter table (names of transformers' CLIPTextTransformer)
        ParamTable& pt = t.table;
        pt.add("embeddings.token_embedding.weight", {c.vocab, D}, &t.tok);
        pt.add("embeddings.position_embedding.weight", {c.positions, D}, &t.pos);
        t.layer.resize(c.layers);
        for (int l = 0; l < c.layers; ++l) add_clip_layer(pt, "encoder.layers." + std::to_string(l) + ".", D, F, t.layer[l]);
        pt.add("final_layer_norm.weight", {D}, &t.lnf_g);
        pt.add("final_layer_norm.bias", {D}, &t.lnf_b);
        t.ids_host.resize((size_t)max_prompts * c.positions);
        using B = EncoderBase;
        // attn zeroed: the attention writes only the real token columns, the padding columns of its output stay zero
        return t.alloc({B::buf(&t.h, D * Tm), B::buf(&t.x, D * Tm), B::buf(&t.qkv, 3 * D * Tm), B::buf(&t.attn, D * Tm, true),
                        B::buf(&t.f, F * Tm), B::buf(&t.stats, 2 * Tm), B::buf(&t.ids, (size_t)max_prompts * c.positions)});
    });
}

int loco_text_load_param(loco_text* t, const char* name, const float* host, const int64_t* shape, int32_t ndim) {
    if (!t) return -1;
    const float* dst = nullptr;
    if (t->table.load(name, host, shape, ndim, t->device, "loco_text_load_param", t->err, &dst)) return -1;
    return t->param_loaded(dst);
}

int loco_text_params_missing(loco_text* t) { return t ? t->table.missing(t->err) : -1; }

int loco_text_encode(loco_text* t, const int32_t* ids_dev, int32_t n, float* out_dev, void* stream) {
    return t ? t->encode(ids_dev, nullptr, n, out_dev, (hipStream_t)stream) : -1;
}

int loco_text_encode_masked(loco_text* t, const int32_t* ids_dev, const int32_t* lens, int32_t n, float* out_dev, void* stream) {
    return t ? t->encode_masked(ids_dev, lens, n, out_dev, (hipStream_t)stream) : -1;
}

const char* loco_text_last_error(loco_text* t) { return t ? t->err.c_str() : g_text_create_err.c_str(); }

void loco_text_destroy(loco_text* t) { delete t; }

}  // extern "C"
