// T5 (v1.1) encoder of the DeepFloyd IF path (include/loco_hip.h loco_t5_create / loco_text_encode_masked): the
// T5EncoderModel that diffusers' IFPipeline.encode_prompt runs (reference src/modules/edit.py:1274-1284), exact fp32
// throughout, fp32 storage.
//
// Layout: that of the CLIP encoder (textenc.hip) -- the activations of all n prompts of a call channel-major in ONE [D][Tp]
// tensor, token column p * L + t, Tp = n * L rounded up to 16, padding columns zero-fed.  The linear layers are
// launch_gemm_fixed over all prompts (no bias anywhere in T5): q | k | v as one packed [3 inner][D] operator, o and wo with
// the residual in the epilogue, wi_0 | wi_1 as one packed [2 F][D] operator.  New here: the embedding gather, the RMS norm
// over channel-major columns, the bidirectional self-attention of one (prompt, head) per workgroup with the relative
// position bias and the key padding mask, and the gate gelu_new(a) * b.  Every kernel computes a token column from that
// column (the attention: from the columns and the length of its own prompt) alone, in a fixed order: a prompt's rows are
// bit-identical whatever n, its position in the batch and the lengths of the other prompts.
#include "textenc.h"

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

namespace loco {
namespace {

constexpr int T5A_THREADS = 256, T5A_WAVES = T5A_THREADS / 64;
constexpr int RN_COLS = 16, RN_SLICES = 64;       // RMS norm: 16 columns x 64 channel slices per workgroup

// h[c][col] = tok[ids[col]][c] for col < T, 0 for the padding columns T <= col < Tp
__global__ __launch_bounds__(256) void t5_embed_kernel(const int* ids, int T, int Tp, int D, const float* tok, float* h) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)D * Tp) return;
    const int c = (int)(e / Tp), col = (int)(e % Tp);
    h[e] = col < T ? tok[(long)ids[col] * D + c] : 0.f;
}

// y[c][col] = x[c][col] * rsqrt(mean_c x[c][col]^2 + eps) * w[c].  A workgroup owns 16 columns (Tp is a multiple of 16);
// thread (cx, cy) sums the squares of channels cy, cy + 64, ... of column cx in that order, the 64 partial sums of a column
// are added in slice order: the same chain for every column wherever it sits.
__global__ __launch_bounds__(RN_COLS * RN_SLICES) void t5_rmsnorm_kernel(const float* x, const float* w, float eps, int D, int Tp,
                                                                           float* y) {
    __shared__ float part[RN_SLICES][RN_COLS + 1];
    __shared__ float rs[RN_COLS];
    const int cx = threadIdx.x % RN_COLS, cy = threadIdx.x / RN_COLS;
    const long col = (long)blockIdx.x * RN_COLS + cx;           // < Tp by the grid
    float s = 0.f;
    for (int c = cy; c < D; c += RN_SLICES) {
        const float v = x[(long)c * Tp + col];
        s = fmaf(v, v, s);
    }
    part[cy][cx] = s;
    __syncthreads();
    if (threadIdx.x < RN_COLS) {
        float tot = 0.f;
        for (int k = 0; k < RN_SLICES; ++k) tot += part[k][threadIdx.x];
        rs[threadIdx.x] = 1.0f / sqrtf(tot / (float)D + eps);
    }
    __syncthreads();
    const float r = rs[cx];
    for (int c = cy; c < D; c += RN_SLICES) y[(long)c * Tp + col] = x[(long)c * Tp + col] * r * w[c];
}

// One workgroup per (prompt p, head h): K and V of the head ([hd][L] each) in LDS; each wave owns the query rows
// i = i0 + wave, lane j (and j + 64) the score against key j < len: q_i . k_j + bias[h][j - i + L - 1], no scale; fp32 softmax
// over the row (max / sum by shuffles), then lane c accumulates o[c] = sum_j P[j] V[c][j] in key order.  Padded query rows
// (i >= len) are computed like the others.  qkv: [3 inner][ld] = q | k | v channel rows, out [inner][ld].
__global__ __launch_bounds__(T5A_THREADS) void t5_attn_kernel(const float* qkv, long ld, int L, int inner, int hd,
                                                              const float* bias_tab, const int* lens, float* out) {
    extern __shared__ float sm[];
    float* Ks = sm;
    float* Vs = sm + hd * L;
    float* Ps = Vs + hd * L;               // [T5A_WAVES][L]
    const int p = blockIdx.x, h = blockIdx.y;
    const int len = lens[p];               // 1 <= len <= L (checked on the host)
    const long col0 = (long)p * L;
    const float* q = qkv + (long)(h * hd) * ld + col0;
    const float* k = qkv + (long)(inner + h * hd) * ld + col0;
    const float* v = qkv + (long)(2 * inner + h * hd) * ld + col0;
    const float* bh = bias_tab + (long)h * (2 * L - 1) + (L - 1);
    for (int e = threadIdx.x; e < hd * L; e += T5A_THREADS) {
        const int c = e / L, t = e - c * L;
        Ks[e] = k[(long)c * ld + t];
        Vs[e] = v[(long)c * ld + t];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    float* pw = Ps + w * L;
    for (int i0 = 0; i0 < L; i0 += T5A_WAVES) {
        const int i = i0 + w;                      // wave-uniform
        if (i < L) {
            float s[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int j = lane + 64 * u;
                s[u] = -INFINITY;
                if (j < len) {
                    float acc = 0.f;
                    for (int c = 0; c < hd; ++c) acc = fmaf(q[(long)c * ld + i], Ks[c * L + j], acc);
                    s[u] = acc + bh[j - i];
                }
            }
            float m = fmaxf(s[0], s[1]);
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
            float e[2], sum = 0.f;
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                e[u] = (lane + 64 * u < len) ? expf(s[u] - m) : 0.f;
                sum += e[u];
            }
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o);
            const float inv = 1.0f / sum;
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int j = lane + 64 * u;
                if (j < len) pw[j] = e[u] * inv;
            }
        }
        __syncthreads();
        if (i < L) {
            for (int c = lane; c < hd; c += 64) {
                float acc = 0.f;
                for (int j = 0; j < len; ++j) acc = fmaf(pw[j], Vs[c * L + j], acc);
                out[(long)(h * hd + c) * ld + col0 + i] = acc;
            }
        }
        __syncthreads();
    }
}

// f [2 F][Tp] = wi_0 x | wi_1 x  ->  f[r][col] = gelu_new(f[r][col]) * f[F + r][col] (tanh form), in place in the first F rows
__global__ __launch_bounds__(256) void t5_gate_kernel(float* f, long FT) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= FT) return;
    const float a = f[e], b = f[FT + e];
    const float g = 0.5f * a * (1.0f + tanhf(0.7978845608028654f * (a + 0.044715f * a * a * a)));
    f[e] = g * b;
}

size_t t5_attn_lds_bytes(int hd, int L) { return (size_t)(2 * hd * L + T5A_WAVES * L) * sizeof(float); }

// T5Attention._relative_position_bucket(k - q, bidirectional=True) of transformers, in double precision
int t5_bucket(int rel, int buckets, int max_distance) {
    const int nb = buckets / 2;
    int ret = rel > 0 ? nb : 0;
    const int n = rel < 0 ? -rel : rel;
    const int max_exact = nb / 2;
    if (n < max_exact) return ret + n;
    int large = max_exact + (int)(std::log((double)n / max_exact) / std::log((double)max_distance / max_exact) * (nb - max_exact));
    return ret + std::min(large, nb - 1);
}

}  // namespace

void t5_free(loco_text* t) {
    (void)hipFree(t->bias_tab); (void)hipFree(t->lens);
    t->bias_tab = nullptr; t->lens = nullptr;
}

int t5_param_loaded(loco_text* t, const float* dst) {
    if (dst != t->relw) return 0;
    // the bias depends on k - q only: bias_tab[h][o] = weight[bucket(o - (L - 1))][h], built once here
    const int L = t->L, H = t->t5.heads, NO = 2 * L - 1;
    std::vector<float> w((size_t)t->t5.buckets * H), tab((size_t)H * NO);
    if (hipMemcpy(w.data(), t->relw, w.size() * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)
        return t->fail("loco_text_load_param: reading relative_attention_bias back failed");
    for (int h = 0; h < H; ++h)
        for (int o = 0; o < NO; ++o) tab[(size_t)h * NO + o] = w[(size_t)t->bucket[o] * H + h];
    if (hipMemcpy(t->bias_tab, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
        return t->fail("loco_text_load_param: copy of the relative position bias table failed");
    return 0;
}

int t5_encode(loco_text* t, const int32_t* ids_dev, const int32_t* lens, int32_t n, float* out_dev, hipStream_t st) {
    if (!ids_dev || !out_dev) return t->fail("loco_text_encode: null ids or out");
    if (n <= 0 || n > t->max_prompts)
        return t->fail("loco_text_encode: n = " + std::to_string(n) + " outside [1, max_prompts = " + std::to_string(t->max_prompts) + "]");
    if (loco_text_params_missing(t)) return -1;
    const int L = t->L, D = t->D, F = t->t5.d_ff, inner = t->inner, T = n * L, Tp = (T + 15) / 16 * 16;
    for (int p = 0; p < n; ++p) {
        const int len = lens ? lens[p] : L;
        if (len < 1 || len > L)
            return t->fail("loco_text_encode: length " + std::to_string(len) + " of prompt " + std::to_string(p) + " outside [1, positions = " +
                           std::to_string(L) + "]");
        t->lens_host[p] = len;
    }
    TextDeviceGuard dg(t->device);
    // range check of the ids (an index past the table would read outside it): the one host synchronisation of a call
    if (hipMemcpyAsync(t->ids_host.data(), ids_dev, (size_t)T * sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return t->fail("loco_text_encode: reading the token ids failed");
    for (int i = 0; i < T; ++i) {
        const int id = t->ids_host[i];
        if (id < 0 || id >= t->t5.vocab)
            return t->fail("loco_text_encode: token id " + std::to_string(id) + " at prompt " + std::to_string(i / L) +
                           ", position " + std::to_string(i % L) + " outside [0, vocab = " + std::to_string(t->t5.vocab) + ")");
    }
    if (hipMemcpyAsync(t->ids, t->ids_host.data(), (size_t)T * sizeof(int), hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(t->lens, t->lens_host.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, st) != hipSuccess)
        return t->fail("loco_text_encode: copy of the token ids / lengths failed");
    const long DT = (long)D * Tp, FT = (long)F * Tp;
    const float eps = t->t5.ln_eps;
    const size_t lds = t5_attn_lds_bytes(t->hd, L);
    const dim3 rn_grid(Tp / RN_COLS), rn_block(RN_COLS * RN_SLICES);
    hipLaunchKernelGGL(t5_embed_kernel, dim3((unsigned)((DT + 255) / 256)), dim3(256), 0, st, t->ids, T, Tp, D, t->tok, t->h);
    for (const T5Layer& ly : t->t5layer) {
        hipLaunchKernelGGL(t5_rmsnorm_kernel, rn_grid, rn_block, 0, st, t->h, ly.ln1, eps, D, Tp, t->x);
        launch_gemm_fixed(text_linear(ly.wqkv, nullptr, t->x, t->qkv, nullptr, 3 * inner, D, Tp), GEMM_ACT_NONE, st);
        hipLaunchKernelGGL(t5_attn_kernel, dim3(n, t->t5.heads), dim3(T5A_THREADS), lds, st, t->qkv, (long)Tp, L, inner, t->hd,
                           t->bias_tab, t->lens, t->attn);
        launch_gemm_fixed(text_linear(ly.wo, nullptr, t->attn, t->h, t->h, D, inner, Tp), GEMM_ACT_NONE, st);
        hipLaunchKernelGGL(t5_rmsnorm_kernel, rn_grid, rn_block, 0, st, t->h, ly.ln2, eps, D, Tp, t->x);
        launch_gemm_fixed(text_linear(ly.wi, nullptr, t->x, t->f, nullptr, 2 * F, D, Tp), GEMM_ACT_NONE, st);
        hipLaunchKernelGGL(t5_gate_kernel, dim3((unsigned)((FT + 255) / 256)), dim3(256), 0, st, t->f, FT);
        launch_gemm_fixed(text_linear(ly.wff, nullptr, t->f, t->h, t->h, D, F, Tp), GEMM_ACT_NONE, st);
    }
    hipLaunchKernelGGL(t5_rmsnorm_kernel, rn_grid, rn_block, 0, st, t->h, t->lnf_g, eps, D, Tp, t->x);
    launch_text_transpose(t->x, Tp, T, D, out_dev, st);
    if (hipGetLastError() != hipSuccess) return t->fail("loco_text_encode: kernel launch failed");
    return 0;
}

}  // namespace loco

using namespace loco;

extern "C" {

int loco_t5_create(const loco_t5_cfg* cfg, int32_t device, int32_t max_prompts, loco_text** out) {
    auto report = [](const std::string& m) { text_set_create_error(m); return -1; };      // read by loco_text_last_error(NULL)
    if (!out) return report("loco_t5_create: out is NULL");
    *out = nullptr;
    if (!cfg) return report("loco_t5_create: cfg is NULL");
    const loco_t5_cfg c = *cfg;
    if (c.vocab <= 0 || c.d_model <= 0 || c.d_kv <= 0 || c.heads <= 0 || c.d_ff <= 0 || c.layers <= 0 || c.positions <= 0 ||
        max_prompts <= 0)
        return report("loco_t5_create: vocab, d_model, d_kv, heads, d_ff, layers, positions and max_prompts must be positive");
    if (c.positions > 128) return report("loco_t5_create: positions > 128 (the attention kernel holds 2 keys per lane)");
    if (c.buckets < 4 || c.buckets % 4) return report("loco_t5_create: buckets must be a positive multiple of 4");
    if (c.max_distance <= c.buckets / 4) return report("loco_t5_create: max_distance must exceed buckets / 4");
    if (c.act != 0) return report("loco_t5_create: act must be 0 (gated-gelu: the only feed_forward_proj built)");
    if (!(c.ln_eps > 0.f)) return report("loco_t5_create: ln_eps must be positive");
    if (t5_attn_lds_bytes(c.d_kv, c.positions) > 65536)
        return report("loco_t5_create: d_kv x positions too large for the attention kernel's LDS (64 KiB)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return report("loco_t5_create: no such HIP device");
    TextDeviceGuard dg(device);
    loco_text* t = new loco_text();
    t->kind = TEXT_KIND_T5;
    std::memset(&t->cfg, 0, sizeof(t->cfg));
    t->t5 = c; t->device = device; t->max_prompts = max_prompts;
    t->L = c.positions; t->D = c.d_model; t->hd = c.d_kv; t->inner = c.heads * c.d_kv;
    t->Tmax = (max_prompts * c.positions + 15) / 16 * 16;
    const long D = c.d_model, F = c.d_ff, I = t->inner;
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
    const size_t o_tok = add("shared.weight", {c.vocab, D});
    size_t o_rel = 0;
    struct LOff { size_t v[6]; };
    std::vector<LOff> loff(c.layers);
    for (int l = 0; l < c.layers; ++l) {
        const std::string p = "encoder.block." + std::to_string(l) + ".layer.";
        LOff& o = loff[l];
        o.v[0] = add(p + "0.layer_norm.weight", {D});
        o.v[1] = total; total += (size_t)3 * I * D;
        const char* qkvn[3] = {"q", "k", "v"};
        for (int j = 0; j < 3; ++j) specs.push_back({p + "0.SelfAttention." + qkvn[j] + ".weight", {I, D}, o.v[1] + (size_t)j * I * D});
        o.v[2] = add(p + "0.SelfAttention.o.weight", {D, I});
        if (l == 0) o_rel = add(p + "0.SelfAttention.relative_attention_bias.weight", {c.buckets, c.heads});
        o.v[3] = add(p + "1.layer_norm.weight", {D});
        o.v[4] = total; total += (size_t)2 * F * D;
        specs.push_back({p + "1.DenseReluDense.wi_0.weight", {F, D}, o.v[4]});
        specs.push_back({p + "1.DenseReluDense.wi_1.weight", {F, D}, o.v[4] + (size_t)F * D});
        o.v[5] = add(p + "1.DenseReluDense.wo.weight", {D, F});
    }
    const size_t o_lnf = add("encoder.final_layer_norm.weight", {D});
    const long Tm = t->Tmax;
    const int NO = 2 * c.positions - 1;
    bool ok = hipMalloc(&t->params, total * sizeof(float)) == hipSuccess &&
              hipMalloc(&t->h, D * Tm * sizeof(float)) == hipSuccess && hipMalloc(&t->x, D * Tm * sizeof(float)) == hipSuccess &&
              hipMalloc(&t->qkv, 3 * I * Tm * sizeof(float)) == hipSuccess &&
              hipMalloc(&t->attn, I * Tm * sizeof(float)) == hipSuccess && hipMalloc(&t->f, 2 * F * Tm * sizeof(float)) == hipSuccess &&
              hipMalloc(&t->ids, (size_t)max_prompts * c.positions * sizeof(int)) == hipSuccess &&
              hipMalloc(&t->lens, (size_t)max_prompts * sizeof(int)) == hipSuccess &&
              hipMalloc(&t->bias_tab, (size_t)c.heads * NO * sizeof(float)) == hipSuccess;
    // the attention writes only the real token columns: the padding columns of its output stay zero
    ok = ok && hipMemset(t->attn, 0, I * Tm * sizeof(float)) == hipSuccess;
    if (!ok) {
        loco_text_destroy(t);
        return report("loco_t5_create: hipMalloc failed");
    }
    for (const Spec& s : specs) t->table.push_back({s.name, s.shape, t->params + s.off, false});
    t->tok = t->params + o_tok; t->relw = t->params + o_rel; t->lnf_g = t->params + o_lnf;
    for (int l = 0; l < c.layers; ++l) {
        float* P = t->params;
        const size_t* v = loff[l].v;
        t->t5layer.push_back({P + v[0], P + v[1], P + v[2], P + v[3], P + v[4], P + v[5]});
    }
    t->bucket.resize(NO);
    for (int o = 0; o < NO; ++o) t->bucket[o] = t5_bucket(o - (c.positions - 1), c.buckets, c.max_distance);
    t->ids_host.resize((size_t)max_prompts * c.positions);
    t->lens_host.resize((size_t)max_prompts);
    *out = t;
    return 0;
}

int loco_text_encode_masked(loco_text* t, const int32_t* ids_dev, const int32_t* lens, int32_t n, float* out_dev, void* stream) {
    if (!t) return -1;
    if (t->kind != TEXT_KIND_T5)
        return t->fail("loco_text_encode_masked: this handle is a CLIP encoder (causal, no padding mask); use loco_text_encode");
    return t5_encode(t, ids_dev, lens, n, out_dev, (hipStream_t)stream);
}

}  // extern "C"
