// T5 (v1.1) encoder of the DeepFloyd IF path (include/loco_hip.h loco_t5_create / loco_text_encode_masked): the
// T5EncoderModel that diffusers' IFPipeline.encode_prompt runs (reference src/modules/edit.py:1274-1284), exact fp32
// throughout, fp32 storage.
//
// Layout: that of the CLIP encoder (textenc.hip) -- the activations of all n prompts of a call channel-major in ONE [D][Tp]
// tensor, token column p * L + t, Tp = n * L rounded up to 16, padding columns zero-fed.  The linear layers are
// launch_gemm_fixed over all prompts (no bias anywhere in T5): q | k | v as one packed [3 inner][D] operator, o and wo with
// the residual in the epilogue, wi_0 | wi_1 as one packed [2 F][D] operator.  The embedding gather (without positions), the
// self-attention of one (prompt, head) per workgroup (its bidirectional form: relative position bias and key padding mask),
// and the id staging are textenc.hip's, through textenc.h; the transpose is encoder_kernels.hip's.  New here: the RMS norm over channel-major columns
// and the gate gelu_new(a) * b.  Every kernel computes a token column from that column (the attention: from the columns and
// the length of its own prompt) alone, in a fixed order: a prompt's rows are bit-identical whatever n, its position in the
// batch and the lengths of the other prompts.
#include "textenc.h"

#include <cmath>

namespace loco {
namespace {

constexpr int RN_COLS = 16, RN_SLICES = 64;       // RMS norm: 16 columns x 64 channel slices per workgroup

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

// f [2 F][Tp] = wi_0 x | wi_1 x  ->  f[r][col] = gelu_new(f[r][col]) * f[F + r][col] (tanh form), in place in the first F rows
__global__ __launch_bounds__(256) void t5_gate_kernel(float* f, long FT) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= FT) return;
    const float a = f[e], b = f[FT + e];
    const float g = 0.5f * a * (1.0f + tanhf(0.7978845608028654f * (a + 0.044715f * a * a * a)));
    f[e] = g * b;
}

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

// T5 block: RMS-norm weights, q | k | v packed [3 inner][D], o [D][inner], wi_0 | wi_1 packed [2 F][D], wo [D][F]
struct T5Layer { float *ln1, *wqkv, *wo, *ln2, *wi, *wff; };

struct T5Text final : loco_text {
    loco_t5_cfg cfg;
    int inner = 0;                        // heads * d_kv
    float* relw = nullptr;                // relative_attention_bias.weight [buckets][heads] (inside params)
    float* bias_tab = nullptr;            // [heads][2 L - 1]: the bias of key offset k - q + L - 1, built when relw is loaded
    std::vector<int> bucket;              // [2 L - 1] bucket of every offset
    std::vector<T5Layer> layer;
    int* lens = nullptr;                  // device [max_prompts]
    std::vector<int> lens_host;

    int encode(const int32_t* ids_dev, const int32_t* lens, int32_t n, float* out_dev, hipStream_t st) override;
    int param_loaded(const float* dst) override;
};

int T5Text::param_loaded(const float* dst) {
    if (dst != relw) return 0;
    // the bias depends on k - q only: bias_tab[h][o] = weight[bucket(o - (L - 1))][h], built once here
    const int H = cfg.heads, NO = 2 * L - 1;
    std::vector<float> w((size_t)cfg.buckets * H), tab((size_t)H * NO);
    DeviceGuard dg(device);
    if (hipMemcpy(w.data(), relw, w.size() * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)
        return fail("loco_text_load_param: reading relative_attention_bias back failed");
    for (int h = 0; h < H; ++h)
        for (int o = 0; o < NO; ++o) tab[(size_t)h * NO + o] = w[(size_t)bucket[o] * H + h];
    if (hipMemcpy(bias_tab, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
        return fail("loco_text_load_param: copy of the relative position bias table failed");
    return 0;
}

int T5Text::encode(const int32_t* ids_dev, const int32_t* lens_in, int32_t n, float* out_dev, hipStream_t st) {
    if (text_check_call(this, ids_dev, n, out_dev)) return -1;
    const int F = cfg.d_ff, T = n * L, Tp = (T + 15) / 16 * 16;
    for (int p = 0; p < n; ++p) {
        const int len = lens_in ? lens_in[p] : L;
        if (len < 1 || len > L)
            return fail("loco_text_encode: length " + std::to_string(len) + " of prompt " + std::to_string(p) + " outside [1, positions = " +
                        std::to_string(L) + "]");
        lens_host[p] = len;
    }
    DeviceGuard dg(device);
    if (stage_ids(this, ids_dev, T, L, cfg.vocab, st)) return -1;
    if (hipMemcpyAsync(lens, lens_host.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, st) != hipSuccess)
        return fail("loco_text_encode: copy of the token ids / lengths failed");
    const long FT = (long)F * Tp;
    const float eps = cfg.ln_eps;
    const dim3 rn_grid(Tp / RN_COLS), rn_block(RN_COLS * RN_SLICES);
    launch_text_embed(ids, T, Tp, L, D, tok, nullptr, h, st);
    for (const T5Layer& ly : layer) {
        hipLaunchKernelGGL(t5_rmsnorm_kernel, rn_grid, rn_block, 0, st, h, ly.ln1, eps, D, Tp, x);
        launch_gemm_fixed(enc_linear(ly.wqkv, nullptr, x, qkv, nullptr, 3 * inner, D, Tp), GEMM_ACT_NONE, st);
        launch_prompt_attn(false, qkv, (long)Tp, n, cfg.heads, L, inner, hd, 0.f, bias_tab, lens, attn, st);
        launch_gemm_fixed(enc_linear(ly.wo, nullptr, attn, h, h, D, inner, Tp), GEMM_ACT_NONE, st);
        hipLaunchKernelGGL(t5_rmsnorm_kernel, rn_grid, rn_block, 0, st, h, ly.ln2, eps, D, Tp, x);
        launch_gemm_fixed(enc_linear(ly.wi, nullptr, x, f, nullptr, 2 * F, D, Tp), GEMM_ACT_NONE, st);
        hipLaunchKernelGGL(t5_gate_kernel, dim3(blocks256(FT)), dim3(256), 0, st, f, FT);
        launch_gemm_fixed(enc_linear(ly.wff, nullptr, f, h, h, D, F, Tp), GEMM_ACT_NONE, st);
    }
    hipLaunchKernelGGL(t5_rmsnorm_kernel, rn_grid, rn_block, 0, st, h, lnf_g, eps, D, Tp, x);
    launch_enc_transpose(x, Tp, T, D, out_dev, st);
    if (hipGetLastError() != hipSuccess) return fail("loco_text_encode: kernel launch failed");
    return 0;
}

}  // namespace
}  // namespace loco

using namespace loco;

extern "C" int loco_t5_create(const loco_t5_cfg* cfg, int32_t device, int32_t max_prompts, loco_text** out) {
    auto refuse = [&](const loco_t5_cfg& c) -> std::string {
        if (c.vocab <= 0 || c.d_model <= 0 || c.d_kv <= 0 || c.heads <= 0 || c.d_ff <= 0 || c.layers <= 0 || c.positions <= 0 ||
            max_prompts <= 0)
            return "vocab, d_model, d_kv, heads, d_ff, layers, positions and max_prompts must be positive";
        if (c.positions > 128) return "positions > 128 (the attention kernel holds 2 keys per lane)";
        if (c.buckets < 4 || c.buckets % 4) return "buckets must be a positive multiple of 4";
        if (c.max_distance <= c.buckets / 4) return "max_distance must exceed buckets / 4";
        if (c.act != 0) return "act must be 0 (gated-gelu: the only feed_forward_proj built)";
        if (!(c.ln_eps > 0.f)) return "ln_eps must be positive";
        if (prompt_attn_lds_bytes(c.d_kv, c.positions) > 65536) return "d_kv x positions too large for the attention kernel's LDS (64 KiB)";
        return "";
    };
    // the message is read by loco_text_last_error(NULL)
    return encoder_create<T5Text>("loco_t5_create", g_text_create_err, cfg, device, out, refuse, [&](T5Text& t) {
        const loco_t5_cfg& c = t.cfg = *cfg;
        t.max_prompts = max_prompts;
        t.L = c.positions; t.D = c.d_model; t.hd = c.d_kv; t.inner = c.heads * c.d_kv;
        t.Tmax = (max_prompts * c.positions + 15) / 16 * 16;
        const long D = c.d_model, F = c.d_ff, I = t.inner, Tm = t.Tmax;
        ParamTable& pt = t.table;
        pt.add("shared.weight", {c.vocab, D}, &t.tok);
        t.layer.resize(c.layers);
        for (int l = 0; l < c.layers; ++l) {
            const std::string p = "encoder.block." + std::to_string(l) + ".layer.";
            T5Layer& ly = t.layer[l];
            pt.add(p + "0.layer_norm.weight", {D}, &ly.ln1);
            const size_t wq = pt.reserve((size_t)3 * I * D, &ly.wqkv);
            const char* qkvn[3] = {"q", "k", "v"};
            for (int j = 0; j < 3; ++j) pt.view(p + "0.SelfAttention." + qkvn[j] + ".weight", {I, D}, wq + (size_t)j * I * D);
            pt.add(p + "0.SelfAttention.o.weight", {D, I}, &ly.wo);
            if (l == 0) pt.add(p + "0.SelfAttention.relative_attention_bias.weight", {c.buckets, c.heads}, &t.relw);
            pt.add(p + "1.layer_norm.weight", {D}, &ly.ln2);
            const size_t wi = pt.reserve((size_t)2 * F * D, &ly.wi);
            pt.view(p + "1.DenseReluDense.wi_0.weight", {F, D}, wi);
            pt.view(p + "1.DenseReluDense.wi_1.weight", {F, D}, wi + (size_t)F * D);
            pt.add(p + "1.DenseReluDense.wo.weight", {D, F}, &ly.wff);
        }
        pt.add("encoder.final_layer_norm.weight", {D}, &t.lnf_g);
        const int NO = 2 * c.positions - 1;
        t.bucket.resize(NO);
        for (int o = 0; o < NO; ++o) t.bucket[o] = t5_bucket(o - (c.positions - 1), c.buckets, c.max_distance);
        t.ids_host.resize((size_t)max_prompts * c.positions);
        t.lens_host.resize((size_t)max_prompts);
        using B = EncoderBase;
        // attn zeroed: the attention writes only the real token columns, the padding columns of its output stay zero
        return t.alloc({B::buf(&t.h, D * Tm), B::buf(&t.x, D * Tm), B::buf(&t.qkv, 3 * I * Tm), B::buf(&t.attn, I * Tm, true),
                        B::buf(&t.f, 2 * F * Tm), B::buf(&t.ids, (size_t)max_prompts * c.positions),
                        B::buf(&t.lens, (size_t)max_prompts), B::buf(&t.bias_tab, (size_t)c.heads * NO)});
    });
}
