// CLIP text encoder of the Stable Diffusion paths (include/loco_hip.h loco_text_*): the CLIPTextModel that diffusers'
// StableDiffusionPipeline.encode_prompt runs (reference src/modules/edit.py:1187-1194), exact fp32 throughout.
//
// Layout: the activations of all n prompts of a call live channel-major in ONE [D][Tp] tensor, token column p * L + t
// (Tp = n * L rounded up to 16; the padding columns carry zeros through the embedding and stay independent of the real
// ones).  In that layout the linear layers are one launch_gemm_fixed each over all prompts (W [out][in] row-major as
// stored, so each layer's weights are read once per call), and LayerNorm is xfmr.hip's launch_ln_fwd unchanged.  New
// here: the token + position embedding gather, the causal self-attention of one (prompt, head) per workgroup, and the
// transpose of the final states to [n][L][D].  Every kernel computes a token column from that column (and, in the
// attention, from the columns of its own prompt) alone, in a fixed order: a prompt's rows are bit-identical whatever n
// and its position in the batch.
#include "textenc.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

namespace loco {
namespace {

constexpr int TA_THREADS = 256, TA_WAVES = TA_THREADS / 64;

// h[c][col] = tok[ids[col]][c] + pos[col % L][c] for col < T, 0 for the padding columns T <= col < Tp
__global__ __launch_bounds__(256) void text_embed_kernel(const int* ids, int T, int Tp, int L, int D, const float* tok,
                                                         const float* pos, float* h) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)D * Tp) return;
    const int c = (int)(e / Tp), col = (int)(e % Tp);
    float v = 0.f;
    if (col < T) v = tok[(long)ids[col] * D + c] + pos[(long)(col % L) * D + c];
    h[e] = v;
}

// One workgroup per (prompt p, head h): K and V of the head ([hd][L] each) in LDS; each wave owns the query rows
// i = i0 + wave, lane j (and j + 64) the score against key j <= i; fp32 softmax over the row (max / sum by shuffles),
// then lane c accumulates o[c] = sum_j P[j] V[c][j] in key order.  qkv: [3 D][ld] = q | k | v channel rows, out [D][ld].
__global__ __launch_bounds__(TA_THREADS) void text_attn_kernel(const float* qkv, long ld, int L, int D, int hd, float scale,
                                                               float* out) {
    extern __shared__ float sm[];
    float* Ks = sm;
    float* Vs = sm + hd * L;
    float* Ps = Vs + hd * L;               // [TA_WAVES][L]
    const int p = blockIdx.x, h = blockIdx.y;
    const long col0 = (long)p * L;
    const float* q = qkv + (long)(h * hd) * ld + col0;
    const float* k = qkv + (long)(D + h * hd) * ld + col0;
    const float* v = qkv + (long)(2 * D + h * hd) * ld + col0;
    for (int e = threadIdx.x; e < hd * L; e += TA_THREADS) {
        const int c = e / L, t = e - c * L;
        Ks[e] = k[(long)c * ld + t];
        Vs[e] = v[(long)c * ld + t];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    float* pw = Ps + w * L;
    for (int i0 = 0; i0 < L; i0 += TA_WAVES) {
        const int i = i0 + w;                      // wave-uniform
        if (i < L) {
            float s[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int j = lane + 64 * u;
                s[u] = -INFINITY;
                if (j <= i) {
                    float acc = 0.f;
                    for (int c = 0; c < hd; ++c) acc = fmaf(q[(long)c * ld + i], Ks[c * L + j], acc);
                    s[u] = acc * scale;
                }
            }
            float m = fmaxf(s[0], s[1]);
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
            float e[2], sum = 0.f;
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                e[u] = (lane + 64 * u <= i) ? expf(s[u] - m) : 0.f;
                sum += e[u];
            }
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o);
            const float inv = 1.0f / sum;
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int j = lane + 64 * u;
                if (j <= i) pw[j] = e[u] * inv;
            }
        }
        __syncthreads();
        if (i < L) {
            for (int c = lane; c < hd; c += 64) {
                float acc = 0.f;
                for (int j = 0; j <= i; ++j) acc = fmaf(pw[j], Vs[c * L + j], acc);
                out[(long)(h * hd + c) * ld + col0 + i] = acc;
            }
        }
        __syncthreads();
    }
}

// out[col][c] = x[c][col] for the T real columns
__global__ __launch_bounds__(256) void text_transpose_kernel(const float* x, int Tp, int T, int D, float* out) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)T * D) return;
    const int col = (int)(e / D), c = (int)(e % D);
    out[e] = x[(long)c * Tp + col];
}

}  // namespace

void launch_text_transpose(const float* x, int Tp, int T, int D, float* out, hipStream_t st) {
    const long TD = (long)T * D;
    hipLaunchKernelGGL(text_transpose_kernel, dim3((unsigned)((TD + 255) / 256)), dim3(256), 0, st, x, Tp, T, D, out);
}
}  // namespace loco

using namespace loco;

namespace {
thread_local std::string g_text_create_err;
using DeviceGuard = loco::TextDeviceGuard;

size_t attn_lds_bytes(int hd, int L) { return (size_t)(2 * hd * L + TA_WAVES * L) * sizeof(float); }

void free_text(loco_text* t) {
    (void)hipFree(t->params); (void)hipFree(t->h); (void)hipFree(t->x); (void)hipFree(t->qkv); (void)hipFree(t->attn);
    (void)hipFree(t->f); (void)hipFree(t->stats); (void)hipFree(t->ids);
    t5_free(t);
}
}  // namespace

namespace loco {
void text_set_create_error(const std::string& m) { g_text_create_err = m; }
}  // namespace loco

extern "C" {

int loco_text_create(const loco_text_cfg* cfg, int32_t device, int32_t max_prompts, loco_text** out) {
    if (!out) { g_text_create_err = "loco_text_create: out is NULL"; return -1; }
    *out = nullptr;
    if (!cfg) { g_text_create_err = "loco_text_create: cfg is NULL"; return -1; }
    const loco_text_cfg c = *cfg;
    if (c.vocab <= 0 || c.width <= 0 || c.layers <= 0 || c.heads <= 0 || c.ffn <= 0 || c.positions <= 0 || max_prompts <= 0) {
        g_text_create_err = "loco_text_create: vocab, width, layers, heads, ffn, positions and max_prompts must be positive";
        return -1;
    }
    if (c.width % c.heads) { g_text_create_err = "loco_text_create: width is not a multiple of heads"; return -1; }
    if (c.positions > 128) { g_text_create_err = "loco_text_create: positions > 128 (the attention kernel holds 2 keys per lane)"; return -1; }
    if (c.act != 0 && c.act != 1) { g_text_create_err = "loco_text_create: act must be 0 (quick_gelu) or 1 (gelu)"; return -1; }
    const int hd = c.width / c.heads;
    if (attn_lds_bytes(hd, c.positions) > 65536) {
        g_text_create_err = "loco_text_create: head width x positions too large for the attention kernel's LDS (64 KiB)";
        return -1;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) {
        g_text_create_err = "loco_text_create: no such HIP device";
        return -1;
    }
    DeviceGuard dg(device);
    loco_text* t = new loco_text();
    t->cfg = c; t->device = device; t->max_prompts = max_prompts;
    t->L = c.positions; t->D = c.width; t->hd = hd;
    t->Tmax = (max_prompts * c.positions + 15) / 16 * 16;
    const long D = c.width, F = c.ffn;
    // parameter table (names of transformers' CLIPTextTransformer); q / k / v land in one packed [3 D][D] operator
    size_t total = 0;
    struct Spec { std::string name; std::vector<int64_t> shape; size_t off; };
    std::vector<Spec> specs;
    auto add = [&](const std::string& n, std::vector<int64_t> s) {
        size_t cnt = 1;
        for (auto d : s) cnt *= (size_t)d;
        specs.push_back({n, s, total});
        total += (cnt + 63) / 64 * 64;
        return specs.back().off;
    };
    const size_t o_tok = add("embeddings.token_embedding.weight", {c.vocab, D});
    const size_t o_pos = add("embeddings.position_embedding.weight", {c.positions, D});
    struct LOff { size_t v[12]; };
    std::vector<LOff> loff(c.layers);
    for (int l = 0; l < c.layers; ++l) {
        const std::string p = "encoder.layers." + std::to_string(l) + ".";
        LOff& o = loff[l];
        o.v[0] = add(p + "layer_norm1.weight", {D});
        o.v[1] = add(p + "layer_norm1.bias", {D});
        const size_t wq = total; total += (size_t)3 * D * D;
        const size_t bq = total; total += (size_t)(3 * D + 63) / 64 * 64;
        const char* qkvn[3] = {"q_proj", "k_proj", "v_proj"};
        for (int j = 0; j < 3; ++j) {
            specs.push_back({p + "self_attn." + qkvn[j] + ".weight", {D, D}, wq + (size_t)j * D * D});
            specs.push_back({p + "self_attn." + qkvn[j] + ".bias", {D}, bq + (size_t)j * D});
        }
        o.v[2] = wq; o.v[3] = bq;
        o.v[4] = add(p + "self_attn.out_proj.weight", {D, D});
        o.v[5] = add(p + "self_attn.out_proj.bias", {D});
        o.v[6] = add(p + "layer_norm2.weight", {D});
        o.v[7] = add(p + "layer_norm2.bias", {D});
        o.v[8] = add(p + "mlp.fc1.weight", {F, D});
        o.v[9] = add(p + "mlp.fc1.bias", {F});
        o.v[10] = add(p + "mlp.fc2.weight", {D, F});
        o.v[11] = add(p + "mlp.fc2.bias", {D});
    }
    const size_t o_lg = add("final_layer_norm.weight", {D});
    const size_t o_lb = add("final_layer_norm.bias", {D});
    const long Tm = t->Tmax;
    bool ok = hipMalloc(&t->params, total * sizeof(float)) == hipSuccess &&
              hipMalloc(&t->h, D * Tm * sizeof(float)) == hipSuccess && hipMalloc(&t->x, D * Tm * sizeof(float)) == hipSuccess &&
              hipMalloc(&t->qkv, 3 * D * Tm * sizeof(float)) == hipSuccess &&
              hipMalloc(&t->attn, D * Tm * sizeof(float)) == hipSuccess && hipMalloc(&t->f, F * Tm * sizeof(float)) == hipSuccess &&
              hipMalloc(&t->stats, 2 * Tm * sizeof(float)) == hipSuccess &&
              hipMalloc(&t->ids, (size_t)max_prompts * c.positions * sizeof(int)) == hipSuccess;
    // the attention writes only the real token columns: the padding columns of its output stay zero
    ok = ok && hipMemset(t->attn, 0, D * Tm * sizeof(float)) == hipSuccess;
    if (!ok) {
        free_text(t);
        delete t;
        g_text_create_err = "loco_text_create: hipMalloc failed";
        return -1;
    }
    for (const Spec& s : specs) t->table.push_back({s.name, s.shape, t->params + s.off, false});
    t->tok = t->params + o_tok; t->pos = t->params + o_pos;
    t->lnf_g = t->params + o_lg; t->lnf_b = t->params + o_lb;
    for (int l = 0; l < c.layers; ++l) {
        float* P = t->params;
        const size_t* v = loff[l].v;
        t->layer.push_back({P + v[0], P + v[1], P + v[2], P + v[3], P + v[4], P + v[5], P + v[6], P + v[7], P + v[8], P + v[9],
                            P + v[10], P + v[11]});
    }
    t->ids_host.resize((size_t)max_prompts * c.positions);
    *out = t;
    return 0;
}

int loco_text_load_param(loco_text* t, const char* name, const float* host, const int64_t* shape, int32_t ndim) {
    if (!t) return -1;
    if (!name || !host || (ndim > 0 && !shape) || ndim < 0) return t->fail("loco_text_load_param: null argument");
    for (TextParam& p : t->table) {
        if (p.name != name) continue;
        if ((size_t)ndim != p.shape.size() || !std::equal(p.shape.begin(), p.shape.end(), shape)) {
            std::string m = "loco_text_load_param: " + p.name + " has shape [";
            for (size_t i = 0; i < p.shape.size(); ++i) m += (i ? ", " : "") + std::to_string(p.shape[i]);
            return t->fail(m + "], got another");
        }
        size_t cnt = 1;
        for (auto d : p.shape) cnt *= (size_t)d;
        DeviceGuard dg(t->device);
        if (hipMemcpy(p.dst, host, cnt * sizeof(float), hipMemcpyDefault) != hipSuccess)
            return t->fail("loco_text_load_param: copy of " + p.name + " failed");
        p.loaded = true;
        return t->kind == TEXT_KIND_T5 ? t5_param_loaded(t, p.dst) : 0;
    }
    return t->fail(std::string("loco_text_load_param: unknown parameter ") + name);
}

int loco_text_params_missing(loco_text* t) {
    if (!t) return -1;
    int miss = 0;
    for (const TextParam& p : t->table) {
        if (!p.loaded) {
            if (!miss) t->err = "missing parameter " + p.name;
            ++miss;
        }
    }
    return miss;
}

int loco_text_encode(loco_text* t, const int32_t* ids_dev, int32_t n, float* out_dev, void* stream) {
    if (!t) return -1;
    if (t->kind == TEXT_KIND_T5) return t5_encode(t, ids_dev, nullptr, n, out_dev, (hipStream_t)stream);
    if (!ids_dev || !out_dev) return t->fail("loco_text_encode: null ids or out");
    if (n <= 0 || n > t->max_prompts)
        return t->fail("loco_text_encode: n = " + std::to_string(n) + " outside [1, max_prompts = " + std::to_string(t->max_prompts) + "]");
    if (loco_text_params_missing(t)) return -1;
    DeviceGuard dg(t->device);
    hipStream_t st = (hipStream_t)stream;
    const int L = t->L, D = t->D, F = t->cfg.ffn, T = n * L, Tp = (T + 15) / 16 * 16;
    // range check of the ids (an index past the table would read outside it): the one host synchronisation of a call
    if (hipMemcpyAsync(t->ids_host.data(), ids_dev, (size_t)T * sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return t->fail("loco_text_encode: reading the token ids failed");
    for (int i = 0; i < T; ++i) {
        const int id = t->ids_host[i];
        if (id < 0 || id >= t->cfg.vocab)
            return t->fail("loco_text_encode: token id " + std::to_string(id) + " at prompt " + std::to_string(i / L) +
                           ", position " + std::to_string(i % L) + " outside [0, vocab = " + std::to_string(t->cfg.vocab) + ")");
    }
    if (hipMemcpyAsync(t->ids, t->ids_host.data(), (size_t)T * sizeof(int), hipMemcpyHostToDevice, st) != hipSuccess)
        return t->fail("loco_text_encode: copy of the token ids failed");
    const long DT = (long)D * Tp;
    hipLaunchKernelGGL(text_embed_kernel, dim3((unsigned)((DT + 255) / 256)), dim3(256), 0, st, t->ids, T, Tp, L, D, t->tok, t->pos,
                       t->h);
    const float scale = 1.0f / std::sqrt((float)t->hd);
    const size_t lds = attn_lds_bytes(t->hd, L);
    const int gact = t->cfg.act == 0 ? GEMM_ACT_QUICK_GELU : GEMM_ACT_GELU;
    for (const TextLayer& ly : t->layer) {
        launch_ln_fwd(t->h, 0, 1, D, Tp, ly.ln1_g, ly.ln1_b, t->cfg.ln_eps, t->x, 0, t->stats, 0, st);
        launch_gemm_fixed(text_linear(ly.wqkv, ly.bqkv, t->x, t->qkv, nullptr, 3 * D, D, Tp), GEMM_ACT_NONE, st);
        hipLaunchKernelGGL(text_attn_kernel, dim3(n, t->cfg.heads), dim3(TA_THREADS), lds, st, t->qkv, (long)Tp, L, D, t->hd, scale,
                           t->attn);
        launch_gemm_fixed(text_linear(ly.wo, ly.bo, t->attn, t->h, t->h, D, D, Tp), GEMM_ACT_NONE, st);
        launch_ln_fwd(t->h, 0, 1, D, Tp, ly.ln2_g, ly.ln2_b, t->cfg.ln_eps, t->x, 0, t->stats, 0, st);
        launch_gemm_fixed(text_linear(ly.w1, ly.b1, t->x, t->f, nullptr, F, D, Tp), gact, st);
        launch_gemm_fixed(text_linear(ly.w2, ly.b2, t->f, t->h, t->h, D, F, Tp), GEMM_ACT_NONE, st);
    }
    launch_ln_fwd(t->h, 0, 1, D, Tp, t->lnf_g, t->lnf_b, t->cfg.ln_eps, t->x, 0, t->stats, 0, st);
    launch_text_transpose(t->x, Tp, T, D, out_dev, st);
    if (hipGetLastError() != hipSuccess) return t->fail("loco_text_encode: kernel launch failed");
    return 0;
}

const char* loco_text_last_error(loco_text* t) { return t ? t->err.c_str() : g_text_create_err.c_str(); }

void loco_text_destroy(loco_text* t) {
    if (!t) return;
    {
        DeviceGuard dg(t->device);
        free_text(t);
    }
    delete t;
}

}  // extern "C"
