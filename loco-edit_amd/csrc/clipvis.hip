// CLIP image encoder of the edit scores (include/loco_hip.h loco_clipvis_*): the CLIPVisionModelWithProjection of transformers
// -- patch embedding without bias, class token, learned position embedding, pre_layrnorm, `layers` pre-LN blocks of full
// (unmasked) multi-head self-attention and an MLP, post_layernorm of the class token, visual_projection -- and the image
// preprocessing of CLIPImageProcessor in float arithmetic.  Exact fp32 throughout, fp32 storage.
//
// Layout: that of the text encoders (textenc.hip) -- the T = 1 + G^2 tokens of all n images of a call channel-major in ONE
// [D][Tp] tensor, token column i * T + t (t = 0: the class token, t = 1 + row * G + col: a patch), Tp = n * T rounded up to
// 16; the padding columns are zero-fed and stay independent of the real ones.  The patch projection, the packed q | k | v
// operator, out_proj, fc1 (with its activation), fc2 and visual_projection are launch_gemm_fixed, the LayerNorms xfmr.hip's
// launch_ln_fwd; the layer's parameters and its seven launches are encoder_common.h's add_clip_layer / pre_ln_block, as in
// the text tower.  The batched patch gather, the attention (the streamed kernel samenc.hip runs with its bias tables, here
// without them) and the transposes of the results are encoder_kernels.hip's.  New here: the class / position add, the class
// column gather and the two resize passes of the preprocessing.  Every kernel computes a token column from the columns of
// its own image alone, in a fixed order: an image's rows are bit-identical whatever n and its position.
//
// The cotangent pass (loco_clipvis_enable_grad / _encode_vjp: the pixel gradient of a CLIP score) walks the same
// launches backwards on records the forward keeps per layer: every W^T is launch_gemm_fixed on the forward's weight with A's
// strides swapped, the LayerNorms xfmr.hip's launch_ln_cot; new are the two attention cotangent kernels, the activation
// derivative, the class column scatter and the patch adjoint.  No atomics, the forward's invariant carries over.  The float
// preprocessing (loco_clipvis_preprocess_f32 and its transpose) resizes windows of [-1, 1] frames by the same tap rule.
#include "enc_attn_launch.h"

#include <cmath>

// What the cotangent pass keeps of a layer: its input h and the residual stream after the attention (h_mid), both [D][Tp];
// qkv [3 D][Tp]; the attention output [D][Tp]; the statistics of the two LayerNorms [2][Tp]; the softmax row max and row sum
// [2][heads][Tp].  The fc1 pre-activation is not kept: the pass recomputes it from h_mid (one LayerNorm and one GEMM).
struct ClipVisRec { float *h_in, *qkv, *attn, *h_mid, *st1, *st2, *ml; };

struct loco_clipvis : loco::EncoderBase {
    loco_clipvis_cfg cfg;
    int max_images = 0, G = 0, T = 0, Tmax = 0, Nmax = 0, hd = 0;
    long frows = 0;                                // rows of f: max(mlp_dim, 3 patch^2)
    float *cls = nullptr, *patch_w = nullptr, *pos = nullptr, *pre_g = nullptr, *pre_b = nullptr, *post_g = nullptr,
          *post_b = nullptr, *proj = nullptr;
    std::vector<loco::PreLnLayer> layer;
    float *h = nullptr, *x = nullptr, *qkv = nullptr, *attn = nullptr, *f = nullptr, *stats = nullptr, *pool = nullptr,
          *pooln = nullptr, *emb = nullptr;
    float* rows = nullptr;                         // the preprocessing's horizontally resized rows, grown on demand
    size_t rows_floats = 0;
    // the cotangent pass (loco_clipvis_enable_grad): the records of the last encode and the gradient workspace, one allocation
    bool grad = false;
    int kept_n = 0;                                // images of the kept encode (0: none kept)
    float* grad_mem = nullptr;
    size_t grad_bytes = 0;
    std::vector<ClipVisRec> rec;
    float *xemb = nullptr, *st_pre = nullptr, *st_post = nullptr;
    float *gA = nullptr, *gB = nullptr, *gC = nullptr, *gqkv = nullptr, *gf = nullptr, *delta = nullptr, *gE = nullptr,
          *gpn = nullptr, *gpool = nullptr;
    ~loco_clipvis() override {
        loco::DeviceGuard dg(device);
        if (rows) (void)hipFree(rows);
        if (grad_mem) (void)hipFree(grad_mem);
    }
};

namespace loco {
namespace {

// h[c][i T + t] += pos[t][c] (+ cls[c] at t = 0) for the real columns
__global__ __launch_bounds__(256) void clipvis_embed_kernel(float* h, const float* cls, const float* pos, int D, int T, int nT, int Tp) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)D * nT) return;
    const int c = (int)(e / nT), col = (int)(e % nT), t = col % T;
    float v = h[(long)c * Tp + col] + pos[(long)t * D + c];
    if (t == 0) v += cls[c];
    h[(long)c * Tp + col] = v;
}

// ---- cotangent of the attention.  Given g_o, the kept q, k, v, o and the row max m / row sum l of the forward kernel:
// P_ij = exp((q_i scale) . k_j - m_i) / l_i (enc_attn_kernel's own chain of FMAs, so the same scores), delta_i = <g_o_i, o_i>,
// dS = P o (g_o v^T - delta), dQ = scale dS k, dK = scale dS^T q, dV = P^T g_o.  Two kernels, both in the scheme of the forward
// one (4 rows per wave, chunks of the other side streamed through LDS in order, fp32 FMAs), no atomics: every output element
// has one owner that sums in a fixed order, over the columns of its own image alone.
//   * the streamed side lies token-major [chunk][hd + 1] in LDS: the odd row stride makes both the score phase (lane = token,
//     walk over the channels) and the accumulation phase (lane = channel, walk over the tokens) free of bank conflicts, so one
//     copy of K serves both (the forward kernel keeps K channel-major and only V padded);
//   * the chunk is 64 tokens where the carve-up fits the 64 KiB the forward kernel allows itself, else 32 (head widths above
//     95 / 88; lanes 32 .. 63 then idle in the score phase).  Two streamed tensors and two owned ones are resident, against the
//     forward's two and one.
constexpr int CV_COT_ROWS = ENC_ATTN_QB;     // queries (dQ kernel) / keys (dK, dV kernel) a workgroup owns

// dQ and delta: one workgroup per (query block of 16, head, image), keys and values streamed in order
template <int KC>
__global__ __launch_bounds__(ENC_ATTN_THREADS) void clipvis_attn_cot_q_kernel(const float* qkv, const float* o, const float* go, const float* ml,
                                                                        long ld, int D, int hd, int T, float scale, float* gqkv,
                                                                        float* delta) {
    extern __shared__ __align__(16) float cv_sm[];
    const int hdp = hd + 1;
    float* Kt = cv_sm;                                     // [KC][hd + 1]
    float* Vt = Kt + enc_r4(KC * hdp);                      // [KC][hd + 1]
    float* Qs = Vt + enc_r4(KC * hdp);                      // [hd][16], scaled
    float* Gs = Qs + enc_r4(hd * ENC_ATTN_QB);                    // [hd][16]
    float* Ps = Gs + enc_r4(hd * ENC_ATTN_QB);                    // [waves][64][4]: dS
    const int qb = blockIdx.x, h = blockIdx.y, img = blockIdx.z, heads = gridDim.y;
    const long col0 = (long)img * T;
    const int q0 = qb * ENC_ATTN_QB;
    const float* q = qkv + (long)(h * hd) * ld + col0;
    const float* k = qkv + (long)(D + h * hd) * ld + col0;
    const float* v = qkv + (long)(2 * D + h * hd) * ld + col0;
    const float* op = o + (long)(h * hd) * ld + col0;
    const float* gp = go + (long)(h * hd) * ld + col0;
    for (int e = threadIdx.x; e < hd * ENC_ATTN_QB; e += ENC_ATTN_THREADS) {
        const int c = e / ENC_ATTN_QB, ql = min(q0 + e % ENC_ATTN_QB, T - 1);
        Qs[e] = q[(long)c * ld + ql] * scale;
        Gs[e] = gp[(long)c * ld + ql];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int c0 = lane < hd ? lane : 0, c1 = lane + 64 < hd ? lane + 64 : 0;
    float* pw = Ps + wv * (64 * ENC_ATTN_QW);
    float mq[ENC_ATTN_QW], il[ENC_ATTN_QW], dl[ENC_ATTN_QW], a0[ENC_ATTN_QW], a1[ENC_ATTN_QW];
#pragma unroll
    for (int u = 0; u < ENC_ATTN_QW; ++u) {
        const int qr = q0 + wv * ENC_ATTN_QW + u, ql = min(qr, T - 1);
        float a = 0.f;
        for (int c = lane; c < hd; c += 64) a = fmaf(Gs[c * ENC_ATTN_QB + wv * ENC_ATTN_QW + u], op[(long)c * ld + ql], a);
        dl[u] = wave_sum(a);
        mq[u] = ml[(long)h * ld + col0 + ql];
        il[u] = 1.0f / ml[(long)(heads + h) * ld + col0 + ql];
        a0[u] = 0.f; a1[u] = 0.f;
        if (lane == 0 && qr < T) delta[(long)h * ld + col0 + qr] = dl[u];
    }
    for (int k0 = 0; k0 < T; k0 += KC) {
        __syncthreads();
        for (int e = threadIdx.x; e < hd * KC; e += ENC_ATTN_THREADS) {
            const int c = e / KC, j = e % KC, kj = k0 + j;
            const bool ok = kj < T;
            Kt[j * hdp + c] = ok ? k[(long)c * ld + kj] : 0.f;
            Vt[j * hdp + c] = ok ? v[(long)c * ld + kj] : 0.f;
        }
        __syncthreads();
        const bool valid = lane < KC && k0 + lane < T;
        const int jl = lane < KC ? lane : 0;
        float s[ENC_ATTN_QW], dp[ENC_ATTN_QW];
#pragma unroll
        for (int u = 0; u < ENC_ATTN_QW; ++u) { s[u] = 0.f; dp[u] = 0.f; }
        for (int c = 0; c < hd; ++c) {
            const float kv = Kt[jl * hdp + c], vv = Vt[jl * hdp + c];
            const float4 qv = *reinterpret_cast<const float4*>(Qs + c * ENC_ATTN_QB + wv * ENC_ATTN_QW);
            const float4 gv = *reinterpret_cast<const float4*>(Gs + c * ENC_ATTN_QB + wv * ENC_ATTN_QW);
            s[0] = fmaf(qv.x, kv, s[0]);
            s[1] = fmaf(qv.y, kv, s[1]);
            s[2] = fmaf(qv.z, kv, s[2]);
            s[3] = fmaf(qv.w, kv, s[3]);
            dp[0] = fmaf(gv.x, vv, dp[0]);
            dp[1] = fmaf(gv.y, vv, dp[1]);
            dp[2] = fmaf(gv.z, vv, dp[2]);
            dp[3] = fmaf(gv.w, vv, dp[3]);
        }
#pragma unroll
        for (int u = 0; u < ENC_ATTN_QW; ++u) {
            const float p = valid ? expf(s[u] - mq[u]) * il[u] : 0.f;
            pw[lane * ENC_ATTN_QW + u] = p * (dp[u] - dl[u]);
        }
        __syncthreads();
        for (int j = 0; j < KC; ++j) {
            const float4 dv = *reinterpret_cast<const float4*>(pw + j * ENC_ATTN_QW);
            const float k0v = Kt[j * hdp + c0];
            a0[0] = fmaf(dv.x, k0v, a0[0]);
            a0[1] = fmaf(dv.y, k0v, a0[1]);
            a0[2] = fmaf(dv.z, k0v, a0[2]);
            a0[3] = fmaf(dv.w, k0v, a0[3]);
            if (hd > 64) {                                 // uniform
                const float k1v = Kt[j * hdp + c1];
                a1[0] = fmaf(dv.x, k1v, a1[0]);
                a1[1] = fmaf(dv.y, k1v, a1[1]);
                a1[2] = fmaf(dv.z, k1v, a1[2]);
                a1[3] = fmaf(dv.w, k1v, a1[3]);
            }
        }
    }
#pragma unroll
    for (int u = 0; u < ENC_ATTN_QW; ++u) {
        const int ql = q0 + wv * ENC_ATTN_QW + u;
        if (ql >= T) continue;
        if (lane < hd) gqkv[(long)(h * hd + lane) * ld + col0 + ql] = a0[u] * scale;
        if (lane + 64 < hd) gqkv[(long)(h * hd + lane + 64) * ld + col0 + ql] = a1[u] * scale;
    }
}

// dK and dV: one workgroup per (key block of 16, head, image), the queries (q scaled, g_o, m, l, delta) streamed in order
template <int QC>
__global__ __launch_bounds__(ENC_ATTN_THREADS) void clipvis_attn_cot_kv_kernel(const float* qkv, const float* go, const float* ml,
                                                                         const float* delta, long ld, int D, int hd, int T, float scale,
                                                                         float* gqkv) {
    extern __shared__ __align__(16) float cv_sm[];
    const int hdp = hd + 1;
    float* Qt = cv_sm;                                     // [QC][hd + 1], scaled
    float* Gt = Qt + enc_r4(QC * hdp);                      // [QC][hd + 1]
    float* Ks = Gt + enc_r4(QC * hdp);                      // [hd][16]
    float* Vs = Ks + enc_r4(hd * CV_COT_ROWS);              // [hd][16]
    float* Ps = Vs + enc_r4(hd * CV_COT_ROWS);              // [waves][64][4]: P
    float* Ds = Ps + ENC_ATTN_WAVES * 64 * ENC_ATTN_QW;                // [waves][64][4]: dS
    const int kb = blockIdx.x, h = blockIdx.y, img = blockIdx.z, heads = gridDim.y;
    const long col0 = (long)img * T;
    const int kb0 = kb * CV_COT_ROWS;
    const float* q = qkv + (long)(h * hd) * ld + col0;
    const float* k = qkv + (long)(D + h * hd) * ld + col0;
    const float* v = qkv + (long)(2 * D + h * hd) * ld + col0;
    const float* gp = go + (long)(h * hd) * ld + col0;
    for (int e = threadIdx.x; e < hd * CV_COT_ROWS; e += ENC_ATTN_THREADS) {
        const int c = e / CV_COT_ROWS, kl = min(kb0 + e % CV_COT_ROWS, T - 1);
        Ks[e] = k[(long)c * ld + kl];
        Vs[e] = v[(long)c * ld + kl];
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int c0 = lane < hd ? lane : 0, c1 = lane + 64 < hd ? lane + 64 : 0;
    float* pw = Ps + wv * (64 * ENC_ATTN_QW);
    float* dw = Ds + wv * (64 * ENC_ATTN_QW);
    float dk0[ENC_ATTN_QW], dk1[ENC_ATTN_QW], dv0[ENC_ATTN_QW], dv1[ENC_ATTN_QW];
#pragma unroll
    for (int u = 0; u < ENC_ATTN_QW; ++u) { dk0[u] = 0.f; dk1[u] = 0.f; dv0[u] = 0.f; dv1[u] = 0.f; }
    for (int i0 = 0; i0 < T; i0 += QC) {
        __syncthreads();
        for (int e = threadIdx.x; e < hd * QC; e += ENC_ATTN_THREADS) {
            const int c = e / QC, i = e % QC, qi = i0 + i;
            const bool ok = qi < T;
            Qt[i * hdp + c] = ok ? q[(long)c * ld + qi] * scale : 0.f;
            Gt[i * hdp + c] = ok ? gp[(long)c * ld + qi] : 0.f;
        }
        __syncthreads();
        const bool valid = lane < QC && i0 + lane < T;
        const int il = lane < QC ? lane : 0, qi = valid ? i0 + lane : 0;
        const float mi = ml[(long)h * ld + col0 + qi], inv = 1.0f / ml[(long)(heads + h) * ld + col0 + qi];
        const float di = delta[(long)h * ld + col0 + qi];
        float s[ENC_ATTN_QW], dp[ENC_ATTN_QW];
#pragma unroll
        for (int u = 0; u < ENC_ATTN_QW; ++u) { s[u] = 0.f; dp[u] = 0.f; }
        for (int c = 0; c < hd; ++c) {
            const float qv = Qt[il * hdp + c], gv = Gt[il * hdp + c];
            const float4 kv = *reinterpret_cast<const float4*>(Ks + c * CV_COT_ROWS + wv * ENC_ATTN_QW);
            const float4 vv = *reinterpret_cast<const float4*>(Vs + c * CV_COT_ROWS + wv * ENC_ATTN_QW);
            s[0] = fmaf(qv, kv.x, s[0]);
            s[1] = fmaf(qv, kv.y, s[1]);
            s[2] = fmaf(qv, kv.z, s[2]);
            s[3] = fmaf(qv, kv.w, s[3]);
            dp[0] = fmaf(gv, vv.x, dp[0]);
            dp[1] = fmaf(gv, vv.y, dp[1]);
            dp[2] = fmaf(gv, vv.z, dp[2]);
            dp[3] = fmaf(gv, vv.w, dp[3]);
        }
#pragma unroll
        for (int u = 0; u < ENC_ATTN_QW; ++u) {
            const float p = valid ? expf(s[u] - mi) * inv : 0.f;
            pw[lane * ENC_ATTN_QW + u] = p;
            dw[lane * ENC_ATTN_QW + u] = p * (dp[u] - di);
        }
        __syncthreads();
        for (int i = 0; i < QC; ++i) {
            const float4 pv = *reinterpret_cast<const float4*>(pw + i * ENC_ATTN_QW);
            const float4 dv = *reinterpret_cast<const float4*>(dw + i * ENC_ATTN_QW);
            const float g0 = Gt[i * hdp + c0], q0v = Qt[i * hdp + c0];
            dv0[0] = fmaf(pv.x, g0, dv0[0]);
            dv0[1] = fmaf(pv.y, g0, dv0[1]);
            dv0[2] = fmaf(pv.z, g0, dv0[2]);
            dv0[3] = fmaf(pv.w, g0, dv0[3]);
            dk0[0] = fmaf(dv.x, q0v, dk0[0]);
            dk0[1] = fmaf(dv.y, q0v, dk0[1]);
            dk0[2] = fmaf(dv.z, q0v, dk0[2]);
            dk0[3] = fmaf(dv.w, q0v, dk0[3]);
            if (hd > 64) {                                 // uniform
                const float g1 = Gt[i * hdp + c1], q1v = Qt[i * hdp + c1];
                dv1[0] = fmaf(pv.x, g1, dv1[0]);
                dv1[1] = fmaf(pv.y, g1, dv1[1]);
                dv1[2] = fmaf(pv.z, g1, dv1[2]);
                dv1[3] = fmaf(pv.w, g1, dv1[3]);
                dk1[0] = fmaf(dv.x, q1v, dk1[0]);
                dk1[1] = fmaf(dv.y, q1v, dk1[1]);
                dk1[2] = fmaf(dv.z, q1v, dk1[2]);
                dk1[3] = fmaf(dv.w, q1v, dk1[3]);
            }
        }
    }
    // q came in scaled: dk already carries the softmax scale
#pragma unroll
    for (int u = 0; u < ENC_ATTN_QW; ++u) {
        const int kl = kb0 + wv * ENC_ATTN_QW + u;
        if (kl >= T) continue;
        if (lane < hd) {
            gqkv[(long)(D + h * hd + lane) * ld + col0 + kl] = dk0[u];
            gqkv[(long)(2 * D + h * hd + lane) * ld + col0 + kl] = dv0[u];
        }
        if (lane + 64 < hd) {
            gqkv[(long)(D + h * hd + lane + 64) * ld + col0 + kl] = dk1[u];
            gqkv[(long)(2 * D + h * hd + lane + 64) * ld + col0 + kl] = dv1[u];
        }
    }
}

// gf *= act'(f): quick_gelu y = v sigmoid(1.702 v), gelu y = v Phi(v)
__global__ __launch_bounds__(256) void clipvis_dact_kernel(const float* f, long count, int act, float* gf) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= count) return;
    const float v = f[e];
    float d;
    if (act == 0) {
        const float sg = 1.0f / (1.0f + expf(-1.702f * v));
        d = sg * (1.0f + 1.702f * v * (1.0f - sg));
    } else {
        d = 0.5f * (1.0f + erff(v * 0.70710678118654752f)) + v * 0.39894228040143268f * expf(-0.5f * v * v);
    }
    gf[e] *= d;
}

// out[c][i] = in[i][c] for i < n, 0 in the padding columns (the transpose of launch_enc_transpose)
__global__ __launch_bounds__(256) void clipvis_columns_kernel(const float* in, int n, int C, int Np, float* out) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)C * Np) return;
    const int c = (int)(e / Np), i = (int)(e % Np);
    out[e] = i < n ? in[(long)i * C + c] : 0.f;
}

// the adjoint of clipvis_pool_kernel: gh[c][i T] = gpool[c][i], 0 in every other column
__global__ __launch_bounds__(256) void clipvis_pool_cot_kernel(const float* gpool, int D, int T, int Tp, int nT, int Np, float* gh) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)D * Tp) return;
    const int c = (int)(e / Tp), col = (int)(e % Tp);
    gh[e] = col < nT && col % T == 0 ? gpool[(long)c * Np + col / T] : 0.f;
}

// the adjoint of launch_enc_patch (cls = 1): patches do not overlap, every pixel reads the one element it was copied to
__global__ __launch_bounds__(256) void clipvis_patch_cot_kernel(const float* gP, int n, int S, int ps, int G, int T, int Tp, float* gpix) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)n * 3 * S * S) return;
    const int x = (int)(e % S), y = (int)((e / S) % S), ci = (int)((e / ((long)S * S)) % 3), i = (int)(e / ((long)S * S * 3));
    const int r = (ci * ps + y % ps) * ps + x % ps;
    gpix[e] = gP[(long)r * Tp + (long)i * T + 1 + (y / ps) * G + x / ps];
}

// pool[c][i] = h[c][i T] (the class column of image i) for i < n, 0 in the padding columns
__global__ __launch_bounds__(256) void clipvis_pool_kernel(const float* h, int D, int T, int Tp, int n, int Np, float* pool) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)D * Np) return;
    const int c = (int)(e / Np), i = (int)(e % Np);
    pool[e] = i < n ? h[(long)c * Tp + (long)i * T] : 0.f;
}

// ---- preprocessing: the antialiased bicubic resize of PIL / torch (a = -0.5) as two passes, then crop, / 255, normalise
__device__ __forceinline__ double cv_cubic(double x) {
    x = fabs(x);
    if (x < 1.0) return ((1.5 * x - 2.5) * x) * x + 1.0;
    if (x < 2.0) return (((x - 5.0) * x + 8.0) * x - 4.0) * -0.5;
    return 0.0;
}

// The taps of output pixel o of an axis resized from `in` to `out` pixels: input pixels [lo, lo + cnt), weight of tap j =
// cubic((lo + j - center + 0.5) / max(scale, 1)) / (their sum).  Positions and the sum in double, so that a weight is the
// float nearest to its exact value (a float position at 512 pixels would move it by 1e-5).
struct CvTaps { int lo, cnt; double center, inv, total; };
__device__ __forceinline__ CvTaps cv_taps(int o, int in, int out) {
    CvTaps t;
    const double scale = (double)in / (double)out;
    const double support = 2.0 * fmax(scale, 1.0);
    t.inv = 1.0 / fmax(scale, 1.0);
    t.center = ((double)o + 0.5) * scale;
    t.lo = max((int)(t.center - support + 0.5), 0);
    t.cnt = min((int)(t.center + support + 0.5), in) - t.lo;
    t.total = 0.0;
    for (int j = 0; j < t.cnt; ++j) t.total += cv_cubic(((double)(t.lo + j) - t.center + 0.5) * t.inv);
    return t;
}
__device__ __forceinline__ float cv_weight(const CvTaps& t, int j) {
    return (float)(cv_cubic(((double)(t.lo + j) - t.center + 0.5) * t.inv) / t.total);
}

// rows[i][c][y][x] = sum_j w_j frames[i][y][lo + j][c] for the S kept columns x (resized column left + x) of every input row
__global__ __launch_bounds__(256) void clipvis_resize_x_kernel(const unsigned char* frames, int n, int H, int W, int Wn, int left, int S,
                                                               float* rows) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)n * 3 * H * S) return;
    const int x = (int)(e % S), y = (int)((e / S) % H), c = (int)((e / ((long)S * H)) % 3), i = (int)(e / ((long)S * H * 3));
    const unsigned char* src = frames + (((long)i * H + y) * W) * 3 + c;
    float acc;
    if (Wn == W) {
        acc = (float)src[(long)(left + x) * 3];
    } else {
        const CvTaps t = cv_taps(left + x, W, Wn);
        acc = 0.f;
        for (int j = 0; j < t.cnt; ++j) acc = fmaf(cv_weight(t, j), (float)src[(long)(t.lo + j) * 3], acc);
    }
    rows[e] = acc;
}

// out[i][c][y][x] = (sum_j w_j rows[i][c][lo + j][x] / 255 - mean_c) / std_c for the S kept rows y (resized row top + y)
__global__ __launch_bounds__(256) void clipvis_resize_y_kernel(const float* rows, int n, int H, int Hn, int top, int S, float m0, float m1,
                                                               float m2, float s0, float s1, float s2, float* out) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)n * 3 * S * S) return;
    const int x = (int)(e % S), y = (int)((e / S) % S), c = (int)((e / ((long)S * S)) % 3), i = (int)(e / ((long)S * S * 3));
    const float* src = rows + ((long)i * 3 + c) * H * S + x;
    float acc;
    if (Hn == H) {
        acc = src[(long)(top + y) * S];
    } else {
        const CvTaps t = cv_taps(top + y, H, Hn);
        acc = 0.f;
        for (int j = 0; j < t.cnt; ++j) acc = fmaf(cv_weight(t, j), src[(long)(t.lo + j) * S], acc);
    }
    const float mean = c == 0 ? m0 : c == 1 ? m1 : m2, sd = c == 0 ? s0 : c == 1 ? s1 : s2;
    out[e] = (acc / 255.0f - mean) / sd;
}

// ---- the float path: window i = (top, left, h, w) of a [-1, 1] frame resized straight to S x S, each axis through cv_taps(o,
// window extent, S) (so no tap leaves the window), then (v / 2 + 1 / 2 - mean_c) / std_c; and its exact transpose, as gathers
struct CvBox { int top, left, h, w; };
__device__ __forceinline__ CvBox cv_box(const int* boxes, int i, int H, int W) {
    CvBox b;
    if (boxes) { b.top = boxes[4 * i]; b.left = boxes[4 * i + 1]; b.h = boxes[4 * i + 2]; b.w = boxes[4 * i + 3]; }
    else { const int s = min(H, W); b.top = (H - s) / 2; b.left = (W - s) / 2; b.h = s; b.w = s; }
    return b;
}
// the outputs o in [lo, hi] of an axis resized from `in` to `out` pixels whose taps may reach input pixel r (a superset: the
// caller asks cv_taps of each)
__device__ __forceinline__ void cv_reach(int r, int in, int out, int& lo, int& hi) {
    const double scale = (double)in / (double)out, support = 2.0 * fmax(scale, 1.0) + 1.0;
    lo = max((int)floor(((double)r + 0.5 - support) / scale - 0.5), 0);
    hi = min((int)ceil(((double)r + 0.5 + support) / scale - 0.5), out - 1);
}

// rows[i][c][y][x] = sum_j w_j frame[c][top + y][left + lo + j] for the h rows of window i (rows of H x S floats per plane)
__global__ __launch_bounds__(256) void clipvis_win_x_kernel(const float* frames, int nf, const int* boxes, int n, int H, int W, int S,
                                                            float* rows) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)n * 3 * H * S) return;
    const int x = (int)(e % S), y = (int)((e / S) % H), c = (int)((e / ((long)S * H)) % 3), i = (int)(e / ((long)S * H * 3));
    const CvBox b = cv_box(boxes, i, H, W);
    if (y >= b.h) return;
    const float* src = frames + (((long)(nf == 1 ? 0 : i) * 3 + c) * H + b.top + y) * W + b.left;
    const CvTaps t = cv_taps(x, b.w, S);
    float acc = 0.f;
    for (int j = 0; j < t.cnt; ++j) acc = fmaf(cv_weight(t, j), src[t.lo + j], acc);
    rows[e] = acc;
}

// out[i][c][y][x] = ((sum_j w_j rows[i][c][lo + j][x]) / 2 + 1 / 2 - mean_c) / std_c
__global__ __launch_bounds__(256) void clipvis_win_y_kernel(const float* rows, const int* boxes, int n, int H, int W, int S, float m0,
                                                            float m1, float m2, float s0, float s1, float s2, float* out) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)n * 3 * S * S) return;
    const int x = (int)(e % S), y = (int)((e / S) % S), c = (int)((e / ((long)S * S)) % 3), i = (int)(e / ((long)S * S * 3));
    const CvBox b = cv_box(boxes, i, H, W);
    const float* src = rows + ((long)i * 3 + c) * H * S + x;
    const CvTaps t = cv_taps(y, b.h, S);
    float acc = 0.f;
    for (int j = 0; j < t.cnt; ++j) acc = fmaf(cv_weight(t, j), src[(long)(t.lo + j) * S], acc);
    const float mean = c == 0 ? m0 : c == 1 ? m1 : m2, sd = c == 0 ? s0 : c == 1 ? s1 : s2;
    out[e] = (acc * 0.5f + 0.5f - mean) / sd;
}

// transpose of clipvis_win_y_kernel: grows[i][c][r][x] = (1 / (2 std_c)) sum_y w_y(r) gpix[i][c][y][x], y ascending
__global__ __launch_bounds__(256) void clipvis_win_y_cot_kernel(const float* gpix, const int* boxes, int n, int H, int W, int S, float s0,
                                                                float s1, float s2, float* grows) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)n * 3 * H * S) return;
    const int x = (int)(e % S), r = (int)((e / S) % H), c = (int)((e / ((long)S * H)) % 3), i = (int)(e / ((long)S * H * 3));
    const CvBox b = cv_box(boxes, i, H, W);
    if (r >= b.h) return;
    const float* src = gpix + ((long)i * 3 + c) * S * S + x;
    int ylo, yhi;
    cv_reach(r, b.h, S, ylo, yhi);
    float acc = 0.f;
    for (int y = ylo; y <= yhi; ++y) {
        const CvTaps t = cv_taps(y, b.h, S);
        if (r < t.lo || r >= t.lo + t.cnt) continue;
        acc = fmaf(cv_weight(t, r - t.lo), src[(long)y * S], acc);
    }
    const float sd = c == 0 ? s0 : c == 1 ? s1 : s2;
    grows[e] = acc * (0.5f / sd);
}

// transpose of clipvis_win_x_kernel: gframes[f][c][Y][X] = sum over the windows of frame f that hold (Y, X), in window order,
// of sum_x w_x(X - left) grows[i][c][Y - top][x], x ascending; 0 where no window reaches
__global__ __launch_bounds__(256) void clipvis_win_x_cot_kernel(const float* grows, const int* boxes, int n, int nf, int H, int W, int S,
                                                                float* gframes) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)nf * 3 * H * W) return;
    const int X = (int)(e % W), Y = (int)((e / W) % H), c = (int)((e / ((long)W * H)) % 3), f = (int)(e / ((long)W * H * 3));
    const int i0 = nf == 1 ? 0 : f, i1 = nf == 1 ? n : f + 1;
    float acc = 0.f;
    for (int i = i0; i < i1; ++i) {
        const CvBox b = cv_box(boxes, i, H, W);
        const int r = X - b.left, y = Y - b.top;
        if (r < 0 || r >= b.w || y < 0 || y >= b.h) continue;
        const float* src = grows + (((long)i * 3 + c) * H + y) * S;
        int xlo, xhi;
        cv_reach(r, b.w, S, xlo, xhi);
        float a = 0.f;
        for (int x = xlo; x <= xhi; ++x) {
            const CvTaps t = cv_taps(x, b.w, S);
            if (r < t.lo || r >= t.lo + t.cnt) continue;
            a = fmaf(cv_weight(t, r - t.lo), src[x], a);
        }
        acc += a;
    }
    gframes[e] = acc;
}

}  // namespace

void launch_clipvis_attn_cot_q(const float* qkv, const float* o, const float* go, const float* ml, long ld, int D, int hd, int T, int heads,
                               int n, float scale, float* gqkv, float* delta, hipStream_t st) {
    const int kc = clipvis_attn_cot_chunk(hd, 1);
    const size_t lds = clipvis_attn_cot_lds_floats(hd, kc, 1) * sizeof(float);
    const dim3 grid((T + CV_COT_ROWS - 1) / CV_COT_ROWS, heads, n);
    if (kc == 64)
        hipLaunchKernelGGL(clipvis_attn_cot_q_kernel<64>, grid, dim3(ENC_ATTN_THREADS), lds, st, qkv, o, go, ml, ld, D, hd, T, scale, gqkv, delta);
    else
        hipLaunchKernelGGL(clipvis_attn_cot_q_kernel<32>, grid, dim3(ENC_ATTN_THREADS), lds, st, qkv, o, go, ml, ld, D, hd, T, scale, gqkv, delta);
}

void launch_clipvis_attn_cot_kv(const float* qkv, const float* go, const float* ml, const float* delta, long ld, int D, int hd, int T,
                                int heads, int n, float scale, float* gqkv, hipStream_t st) {
    const int kc = clipvis_attn_cot_chunk(hd, 2);
    const size_t lds = clipvis_attn_cot_lds_floats(hd, kc, 2) * sizeof(float);
    const dim3 grid((T + CV_COT_ROWS - 1) / CV_COT_ROWS, heads, n);
    if (kc == 64)
        hipLaunchKernelGGL(clipvis_attn_cot_kv_kernel<64>, grid, dim3(ENC_ATTN_THREADS), lds, st, qkv, go, ml, delta, ld, D, hd, T, scale, gqkv);
    else
        hipLaunchKernelGGL(clipvis_attn_cot_kv_kernel<32>, grid, dim3(ENC_ATTN_THREADS), lds, st, qkv, go, ml, delta, ld, D, hd, T, scale, gqkv);
}

}  // namespace loco

using namespace loco;

namespace {
thread_local std::string g_clipvis_create_err;

// W^T: the operator of enc_linear read through swapped strides (gemm_f32_kernel stages either order)
GemmArgs enc_linear_t(const float* W, const float* X, float* Y, int rows, int cols, int Tp) {
    GemmArgs g = enc_linear(W, nullptr, X, Y, nullptr, cols, rows, Tp);
    g.sam = 1; g.sak = cols;
    return g;
}

// the checks of a window call; boxes_dev is read back (a small synchronous copy behind the stream's work)
int clipvis_check_windows(loco_clipvis* t, const char* fn, const int32_t* boxes_dev, int n, int nf, int H, int W, hipStream_t st) {
    const std::string f = fn;
    if (n <= 0 || H <= 0 || W <= 0) return t->fail(f + ": n, H and W must be positive");
    if (nf != 1 && nf != n) return t->fail(f + ": nf = " + std::to_string(nf) + " must be 1 or n = " + std::to_string(n));
    const int S = t->cfg.image_size;
    if ((long)n * 3 * std::max(H, S) * std::max((long)W, (long)S) > (1L << 31)) return t->fail(f + ": n x 3 x H x W > 2^31 (split the batch)");
    if (!boxes_dev) return 0;
    std::vector<int32_t> b((size_t)4 * n);
    if (hipStreamSynchronize(st) != hipSuccess || hipMemcpy(b.data(), boxes_dev, b.size() * sizeof(int32_t), hipMemcpyDefault) != hipSuccess)
        return t->fail(f + ": reading the boxes failed");
    for (int i = 0; i < n; ++i) {
        const long top = b[4 * i], left = b[4 * i + 1], h = b[4 * i + 2], w = b[4 * i + 3];
        if (top < 0 || left < 0 || h < 1 || w < 1 || top + h > H || left + w > W)
            return t->fail(f + ": box " + std::to_string(i) + " (top " + std::to_string(top) + ", left " + std::to_string(left) + ", h " +
                           std::to_string(h) + ", w " + std::to_string(w) + ") leaves the " + std::to_string(H) + " x " + std::to_string(W) +
                           " frame");
    }
    return 0;
}

// patch projection, class / position add, pre_layrnorm: pixel_values -> xe (the embeddings) -> h0
void clipvis_embed_fwd(loco_clipvis* t, const float* pixel_values, int n, int Tp, float* xe, float* h0, float* st_pre, hipStream_t st) {
    const loco_clipvis_cfg& c = t->cfg;
    const int D = c.width, ps = c.patch_size, PK = 3 * ps * ps, T = t->T, nT = n * T;
    launch_enc_patch(pixel_values, n, c.image_size, ps, t->G, 1, Tp, t->f, st);
    launch_gemm_fixed(enc_linear(t->patch_w, nullptr, t->f, xe, nullptr, D, PK, Tp), GEMM_ACT_NONE, st);
    hipLaunchKernelGGL(clipvis_embed_kernel, dim3(blocks256((long)D * nT)), dim3(256), 0, st, xe, t->cls, t->pos, D, T, nT, Tp);
    launch_ln_fwd(xe, 0, 1, D, Tp, t->pre_g, t->pre_b, c.ln_eps, h0, 0, st_pre, 0, st);
}

// one block of the tower on n images: b's tensors, the row max / sum of the attention to ml unless null
void clipvis_block(loco_clipvis* t, const PreLnLayer& ly, const PreLnBufs& b, float* ml, int n, int Tp, hipStream_t st) {
    const loco_clipvis_cfg& c = t->cfg;
    const int D = c.width, T = t->T, hd = t->hd;
    const float scale = 1.0f / std::sqrt((float)hd);
    pre_ln_block(ly, b, D, c.mlp_dim, Tp, c.ln_eps, c.act == 0 ? GEMM_ACT_QUICK_GELU : GEMM_ACT_GELU, st, [&](const float* qkv, float* attn) {
        launch_enc_attn({qkv, (long)Tp, D, hd, T, n, c.heads, scale, attn, nullptr, nullptr, 0, 0, ml}, st);
    });
}
// the block in place on the shared buffers (no records): t->h -> t->h
PreLnBufs clipvis_plain_bufs(loco_clipvis* t) { return {t->h, t->x, t->qkv, t->attn, t->h, t->f, t->h, t->stats, t->stats}; }

int clipvis_grow_rows(loco_clipvis* t, const char* fn, size_t need) {
    return EncoderBase::grow(&t->rows, &t->rows_floats, need) ? 0 : t->fail(std::string(fn) + ": hipMalloc failed");
}
}  // namespace

extern "C" {

int loco_clipvis_create(const loco_clipvis_cfg* cfg, int32_t device, int32_t max_images, loco_clipvis** out) {
    auto refuse = [&](const loco_clipvis_cfg& c) -> std::string {
        if (c.image_size <= 0 || c.patch_size <= 0 || c.width <= 0 || c.layers <= 0 || c.heads <= 0 || c.mlp_dim <= 0 ||
            c.projection_dim <= 0 || max_images <= 0)
            return "image_size, patch_size, width, layers, heads, mlp_dim, projection_dim and max_images must be positive";
        if (c.image_size % c.patch_size) return "image_size is not a multiple of patch_size";
        if (c.width % c.heads) return "width is not a multiple of heads";
        if (c.act != 0 && c.act != 1) return "act must be 0 (quick_gelu) or 1 (gelu)";
        if (!(c.ln_eps > 0.f)) return "ln_eps must be positive";
        const long G = c.image_size / c.patch_size, hd = c.width / c.heads;
        if (hd > 128) return "head width > 128 (the attention kernel holds 2 channels per lane)";
        if (enc_attn_lds_floats((int)hd, 0) * sizeof(float) > 65536)
            return "head width too large for the attention kernel's LDS (64 KiB)";
        if ((1 + G * G) * (long)max_images > (1L << 24)) return "max_images x tokens > 2^24";
        return "";
    };
    return encoder_create<loco_clipvis>("loco_clipvis_create", g_clipvis_create_err, cfg, device, out, refuse, [&](loco_clipvis& t) {
        const loco_clipvis_cfg& c = t.cfg = *cfg;
        t.max_images = max_images;
        t.G = c.image_size / c.patch_size; t.T = 1 + t.G * t.G; t.hd = c.width / c.heads;
        t.Tmax = (max_images * t.T + 15) / 16 * 16;
        t.Nmax = (max_images + 15) / 16 * 16;
        const long D = c.width, F = c.mlp_dim, P = c.projection_dim, ps = c.patch_size, Tm = t.Tmax, Nm = t.Nmax;
        t.frows = std::max(F, 3 * ps * ps);
        // names of transformers' CLIPVisionModelWithProjection without the `vision_model.` prefix
        ParamTable& pt = t.table;
        pt.add("embeddings.class_embedding", {D}, &t.cls);
        pt.add("embeddings.patch_embedding.weight", {D, 3, ps, ps}, &t.patch_w);
        pt.add("embeddings.position_embedding.weight", {t.T, D}, &t.pos);
        pt.add("pre_layrnorm.weight", {D}, &t.pre_g);
        pt.add("pre_layrnorm.bias", {D}, &t.pre_b);
        t.layer.resize(c.layers);
        for (int l = 0; l < c.layers; ++l) add_clip_layer(pt, "encoder.layers." + std::to_string(l) + ".", D, F, t.layer[l]);
        pt.add("post_layernorm.weight", {D}, &t.post_g);
        pt.add("post_layernorm.bias", {D}, &t.post_b);
        pt.add("visual_projection.weight", {P, D}, &t.proj);
        using B = EncoderBase;
        // attn zeroed: the attention writes only the real token columns, the padding columns of its output stay finite
        return t.alloc({B::buf(&t.h, D * Tm), B::buf(&t.x, D * Tm), B::buf(&t.qkv, 3 * D * Tm), B::buf(&t.attn, D * Tm, true),
                        B::buf(&t.f, t.frows * Tm), B::buf(&t.stats, 2 * Tm), B::buf(&t.pool, D * Nm), B::buf(&t.pooln, D * Nm),
                        B::buf(&t.emb, P * Nm)});
    });
}

int loco_clipvis_load_param(loco_clipvis* t, const char* name, const float* host, const int64_t* shape, int32_t ndim) {
    return t ? t->table.load(name, host, shape, ndim, t->device, "loco_clipvis_load_param", t->err) : -1;
}

int loco_clipvis_params_missing(loco_clipvis* t) { return t ? t->table.missing(t->err) : -1; }

int loco_clipvis_preprocess(loco_clipvis* t, const uint8_t* frames_dev, int32_t n, int32_t H, int32_t W, float* out_dev, void* stream) {
    if (!t) return -1;
    if (!frames_dev || !out_dev) return t->fail("loco_clipvis_preprocess: null frames or out");
    if (n <= 0 || H <= 0 || W <= 0) return t->fail("loco_clipvis_preprocess: n, H and W must be positive");
    const int S = t->cfg.image_size;
    if ((long)n * 3 * std::max(H, S) * std::max((long)W, (long)S) > (1L << 31))
        return t->fail("loco_clipvis_preprocess: n x 3 x H x W > 2^31 (split the batch)");
    // shortest edge -> S, the other edge int(long S / short); centre crop S x S
    const int shortest = std::min(H, W);
    const int Hn = H == shortest ? S : (int)((long)H * S / shortest), Wn = W == shortest ? S : (int)((long)W * S / shortest);
    const int top = (Hn - S) / 2, left = (Wn - S) / 2;
    DeviceGuard dg(t->device);
    hipStream_t st = (hipStream_t)stream;
    const size_t need = (size_t)n * 3 * H * S;
    if (clipvis_grow_rows(t, "loco_clipvis_preprocess", need)) return -1;
    hipLaunchKernelGGL(clipvis_resize_x_kernel, dim3(blocks256((long)need)), dim3(256), 0, st, frames_dev, n, H, W, Wn, left, S, t->rows);
    hipLaunchKernelGGL(clipvis_resize_y_kernel, dim3(blocks256((long)n * 3 * S * S)), dim3(256), 0, st, t->rows, n, H, Hn, top, S,
                       t->cfg.image_mean[0], t->cfg.image_mean[1], t->cfg.image_mean[2], t->cfg.image_std[0], t->cfg.image_std[1],
                       t->cfg.image_std[2], out_dev);
    if (hipGetLastError() != hipSuccess) return t->fail("loco_clipvis_preprocess: kernel launch failed");
    return 0;
}

int loco_clipvis_encode(loco_clipvis* t, const float* pixel_values, int32_t n, float* embeds_dev, float* hidden_dev, float* pooled_dev,
                        void* stream) {
    if (!t) return -1;
    if (!pixel_values || !embeds_dev) return t->fail("loco_clipvis_encode: null pixel_values or out");
    if (n <= 0 || n > t->max_images)
        return t->fail("loco_clipvis_encode: n = " + std::to_string(n) + " outside [1, max_images = " + std::to_string(t->max_images) + "]");
    if (t->table.missing(t->err)) return -1;
    DeviceGuard dg(t->device);
    hipStream_t st = (hipStream_t)stream;
    const loco_clipvis_cfg& c = t->cfg;
    const int D = c.width, P = c.projection_dim;
    const int T = t->T, nT = n * T, Tp = (nT + 15) / 16 * 16, Np = (n + 15) / 16 * 16;
    // with grad enabled the same launches write the layer's tensors into its record instead of the shared buffers
    const bool keep = t->grad;
    if (keep) t->kept_n = 0;
    float* xe = keep ? t->xemb : t->x;
    clipvis_embed_fwd(t, pixel_values, n, Tp, xe, keep ? t->rec[0].h_in : t->h, keep ? t->st_pre : t->stats, st);
    for (size_t l = 0; l < t->layer.size(); ++l) {
        if (!keep) {
            clipvis_block(t, t->layer[l], clipvis_plain_bufs(t), nullptr, n, Tp, st);
            continue;
        }
        const ClipVisRec& r = t->rec[l];
        float* hout = l + 1 < t->layer.size() ? t->rec[l + 1].h_in : t->h;
        clipvis_block(t, t->layer[l], {r.h_in, t->x, r.qkv, r.attn, r.h_mid, t->f, hout, r.st1, r.st2}, r.ml, n, Tp, st);
    }
    if (hidden_dev) launch_enc_transpose(t->h, Tp, nT, D, hidden_dev, st);
    // pooling and heads: class columns -> post_layernorm -> visual_projection
    hipLaunchKernelGGL(clipvis_pool_kernel, dim3(blocks256((long)D * Np)), dim3(256), 0, st, t->h, D, T, Tp, n, Np, t->pool);
    launch_ln_fwd(t->pool, 0, 1, D, Np, t->post_g, t->post_b, c.ln_eps, t->pooln, 0, keep ? t->st_post : t->stats, 0, st);
    if (pooled_dev) launch_enc_transpose(t->pooln, Np, n, D, pooled_dev, st);
    launch_gemm_fixed(enc_linear(t->proj, nullptr, t->pooln, t->emb, nullptr, P, D, Np), GEMM_ACT_NONE, st);
    launch_enc_transpose(t->emb, Np, n, P, embeds_dev, st);
    if (hipGetLastError() != hipSuccess) return t->fail("loco_clipvis_encode: kernel launch failed");
    if (keep) t->kept_n = n;
    return 0;
}

int loco_clipvis_encode_taps(loco_clipvis* t, const float* pixel_values, int32_t n, const int32_t* layers, int32_t n_taps, float* taps_dev,
                             void* stream) {
    if (!t) return -1;
    if (!pixel_values || !taps_dev || !layers) return t->fail("loco_clipvis_encode_taps: null pixel_values, layers or taps");
    if (n <= 0 || n > t->max_images)
        return t->fail("loco_clipvis_encode_taps: n = " + std::to_string(n) + " outside [1, max_images = " + std::to_string(t->max_images) + "]");
    const int L = (int)t->layer.size();
    if (n_taps <= 0 || n_taps > L) return t->fail("loco_clipvis_encode_taps: n_taps = " + std::to_string(n_taps) + " outside [1, layers = " + std::to_string(L) + "]");
    for (int j = 0; j < n_taps; ++j) {
        if (layers[j] < 0 || layers[j] >= L)
            return t->fail("loco_clipvis_encode_taps: layer " + std::to_string(layers[j]) + " outside [0, " + std::to_string(L) + ")");
        if (j && layers[j] <= layers[j - 1]) return t->fail("loco_clipvis_encode_taps: the layers must be strictly increasing");
    }
    if (t->table.missing(t->err)) return -1;
    DeviceGuard dg(t->device);
    hipStream_t st = (hipStream_t)stream;
    const int D = t->cfg.width, T = t->T, nT = n * T, Tp = (nT + 15) / 16 * 16;
    clipvis_embed_fwd(t, pixel_values, n, Tp, t->x, t->h, t->stats, st);
    int j = 0;
    for (int l = 0; l <= layers[n_taps - 1]; ++l) {
        clipvis_block(t, t->layer[l], clipvis_plain_bufs(t), nullptr, n, Tp, st);
        if (l == layers[j]) {
            launch_enc_transpose(t->h, Tp, nT, D, taps_dev + (size_t)j * nT * D, st);
            ++j;
        }
    }
    if (hipGetLastError() != hipSuccess) return t->fail("loco_clipvis_encode_taps: kernel launch failed");
    return 0;
}

int loco_clipvis_enable_grad(loco_clipvis* t, int32_t on) {
    if (!t) return -1;
    DeviceGuard dg(t->device);
    t->kept_n = 0;
    if (!on) {
        if (t->grad_mem) (void)hipFree(t->grad_mem);     // (waits for the launches that use it)
        t->grad_mem = nullptr; t->grad_bytes = 0; t->grad = false;
        t->rec.clear();
        return 0;
    }
    if (t->grad) return 0;
    const loco_clipvis_cfg& c = t->cfg;
    const size_t D = c.width, P = c.projection_dim, Tm = t->Tmax, Nm = t->Nmax, L = t->layer.size(), heads = c.heads;
    if (clipvis_attn_cot_lds_floats(t->hd, clipvis_attn_cot_chunk(t->hd, 2), 2) * sizeof(float) > 65536)
        return t->fail("loco_clipvis_enable_grad: head width too large for the attention cotangent's LDS (64 KiB)");
    // every part a multiple of 16 floats (Tm and Nm are)
    const size_t per_layer = (6 * D + 4 + 2 * heads) * Tm;
    const size_t shared = D * Tm + 2 * Tm + 2 * Nm                       // xemb, st_pre, st_post
                          + 3 * D * Tm + 3 * D * Tm + (size_t)t->frows * Tm + heads * Tm + P * Nm + 2 * D * Nm;
    const size_t total = L * per_layer + shared;
    float* base = nullptr;
    if (hipMalloc(&base, total * sizeof(float)) != hipSuccess) {
        (void)hipGetLastError();
        return t->fail("loco_clipvis_enable_grad: hipMalloc of " + std::to_string(total * sizeof(float) >> 20) + " MiB failed");
    }
    // zeroed: the attention kernels write the real token columns only, the padding columns stay finite
    if (hipMemset(base, 0, total * sizeof(float)) != hipSuccess) {
        (void)hipFree(base);
        return t->fail("loco_clipvis_enable_grad: hipMemset failed");
    }
    float* p = base;
    auto take = [&](size_t n) { float* r = p; p += n; return r; };
    t->rec.resize(L);
    for (ClipVisRec& r : t->rec) {
        r.h_in = take(D * Tm); r.qkv = take(3 * D * Tm); r.attn = take(D * Tm); r.h_mid = take(D * Tm);
        r.st1 = take(2 * Tm); r.st2 = take(2 * Tm); r.ml = take(2 * heads * Tm);
    }
    t->xemb = take(D * Tm); t->st_pre = take(2 * Tm); t->st_post = take(2 * Nm);
    t->gA = take(D * Tm); t->gB = take(D * Tm); t->gC = take(D * Tm); t->gqkv = take(3 * D * Tm);
    t->gf = take((size_t)t->frows * Tm); t->delta = take(heads * Tm);
    t->gE = take(P * Nm); t->gpn = take(D * Nm); t->gpool = take(D * Nm);
    t->grad_mem = base; t->grad_bytes = total * sizeof(float); t->grad = true;
    return 0;
}

int64_t loco_clipvis_grad_bytes(loco_clipvis* t) { return t ? (int64_t)t->grad_bytes : -1; }

int loco_clipvis_encode_vjp(loco_clipvis* t, const float* g_embeds_dev, int32_t n, float* g_pixel_dev, void* stream) {
    if (!t) return -1;
    if (!g_embeds_dev || !g_pixel_dev) return t->fail("loco_clipvis_encode_vjp: null g_embeds or g_pixel");
    if (!t->grad) return t->fail("loco_clipvis_encode_vjp: the handle keeps no records (loco_clipvis_enable_grad first)");
    if (t->kept_n <= 0) return t->fail("loco_clipvis_encode_vjp: no kept loco_clipvis_encode to differentiate");
    if (n != t->kept_n)
        return t->fail("loco_clipvis_encode_vjp: n = " + std::to_string(n) + ", the kept encode carried " + std::to_string(t->kept_n) + " images");
    DeviceGuard dg(t->device);
    hipStream_t st = (hipStream_t)stream;
    const loco_clipvis_cfg& c = t->cfg;
    const int D = c.width, F = c.mlp_dim, P = c.projection_dim, ps = c.patch_size, PK = 3 * ps * ps, S = c.image_size;
    const int G = t->G, T = t->T, hd = t->hd, nT = n * T, Tp = (nT + 15) / 16 * 16, Np = (n + 15) / 16 * 16;
    const float scale = 1.0f / std::sqrt((float)hd);
    // visual_projection^T, post_layernorm on the class columns, back to column i T
    hipLaunchKernelGGL(clipvis_columns_kernel, dim3(blocks256((long)P * Np)), dim3(256), 0, st, g_embeds_dev, n, P, Np, t->gE);
    launch_gemm_fixed(enc_linear_t(t->proj, t->gE, t->gpn, P, D, Np), GEMM_ACT_NONE, st);
    launch_ln_cot(t->gpn, 0, t->pool, t->st_post, 1, D, Np, t->post_g, nullptr, 0, t->gpool, 0, st);
    hipLaunchKernelGGL(clipvis_pool_cot_kernel, dim3(blocks256((long)D * Tp)), dim3(256), 0, st, t->gpool, D, T, Tp, nT, Np, t->gA);
    for (int l = (int)t->layer.size() - 1; l >= 0; --l) {
        const PreLnLayer& ly = t->layer[l];
        const ClipVisRec& r = t->rec[l];
        // the MLP: its input and the fc1 pre-activation are computed again from h_mid
        launch_ln_fwd(r.h_mid, 0, 1, D, Tp, ly.ln2_g, ly.ln2_b, c.ln_eps, t->x, 0, t->stats, 0, st);
        launch_gemm_fixed(enc_linear(ly.w1, ly.b1, t->x, t->f, nullptr, F, D, Tp), GEMM_ACT_NONE, st);
        launch_gemm_fixed(enc_linear_t(ly.w2, t->gA, t->gf, D, F, Tp), GEMM_ACT_NONE, st);
        hipLaunchKernelGGL(clipvis_dact_kernel, dim3(blocks256((long)F * Tp)), dim3(256), 0, st, t->f, (long)F * Tp, c.act, t->gf);
        launch_gemm_fixed(enc_linear_t(ly.w1, t->gf, t->gB, F, D, Tp), GEMM_ACT_NONE, st);
        launch_ln_cot(t->gB, 0, r.h_mid, r.st2, 1, D, Tp, ly.ln2_g, t->gA, 0, t->gC, 0, st);
        // the attention
        launch_gemm_fixed(enc_linear_t(ly.wo, t->gC, t->gB, D, D, Tp), GEMM_ACT_NONE, st);
        launch_clipvis_attn_cot_q(r.qkv, r.attn, t->gB, r.ml, (long)Tp, D, hd, T, c.heads, n, scale, t->gqkv, t->delta, st);
        launch_clipvis_attn_cot_kv(r.qkv, t->gB, r.ml, t->delta, (long)Tp, D, hd, T, c.heads, n, scale, t->gqkv, st);
        launch_gemm_fixed(enc_linear_t(ly.wqkv, t->gqkv, t->gB, 3 * D, D, Tp), GEMM_ACT_NONE, st);
        launch_ln_cot(t->gB, 0, r.h_in, r.st1, 1, D, Tp, ly.ln1_g, t->gC, 0, t->gA, 0, st);
    }
    // pre_layrnorm; the class / position add is the identity; patch projection^T and the patch adjoint
    launch_ln_cot(t->gA, 0, t->xemb, t->st_pre, 1, D, Tp, t->pre_g, nullptr, 0, t->gB, 0, st);
    launch_gemm_fixed(enc_linear_t(t->patch_w, t->gB, t->gf, D, PK, Tp), GEMM_ACT_NONE, st);
    hipLaunchKernelGGL(clipvis_patch_cot_kernel, dim3(blocks256((long)n * 3 * S * S)), dim3(256), 0, st, t->gf, n, S, ps, G, T, Tp, g_pixel_dev);
    if (hipGetLastError() != hipSuccess) return t->fail("loco_clipvis_encode_vjp: kernel launch failed");
    return 0;
}

int loco_clipvis_preprocess_f32(loco_clipvis* t, const float* frames_dev, int32_t nf, const int32_t* boxes_dev, int32_t n, int32_t H,
                                int32_t W, float* out_dev, void* stream) {
    if (!t) return -1;
    if (!frames_dev || !out_dev) return t->fail("loco_clipvis_preprocess_f32: null frames or out");
    DeviceGuard dg(t->device);
    hipStream_t st = (hipStream_t)stream;
    if (clipvis_check_windows(t, "loco_clipvis_preprocess_f32", boxes_dev, n, nf, H, W, st)) return -1;
    const int S = t->cfg.image_size;
    const size_t need = (size_t)n * 3 * H * S;
    if (clipvis_grow_rows(t, "loco_clipvis_preprocess_f32", need)) return -1;
    hipLaunchKernelGGL(clipvis_win_x_kernel, dim3(blocks256((long)need)), dim3(256), 0, st, frames_dev, nf, boxes_dev, n, H, W, S, t->rows);
    hipLaunchKernelGGL(clipvis_win_y_kernel, dim3(blocks256((long)n * 3 * S * S)), dim3(256), 0, st, t->rows, boxes_dev, n, H, W, S,
                       t->cfg.image_mean[0], t->cfg.image_mean[1], t->cfg.image_mean[2], t->cfg.image_std[0], t->cfg.image_std[1],
                       t->cfg.image_std[2], out_dev);
    if (hipGetLastError() != hipSuccess) return t->fail("loco_clipvis_preprocess_f32: kernel launch failed");
    return 0;
}

int loco_clipvis_preprocess_f32_vjp(loco_clipvis* t, const float* g_pixel_dev, const int32_t* boxes_dev, int32_t n, int32_t nf, int32_t H,
                                    int32_t W, float* g_frames_dev, void* stream) {
    if (!t) return -1;
    if (!g_pixel_dev || !g_frames_dev) return t->fail("loco_clipvis_preprocess_f32_vjp: null g_pixel or g_frames");
    DeviceGuard dg(t->device);
    hipStream_t st = (hipStream_t)stream;
    if (clipvis_check_windows(t, "loco_clipvis_preprocess_f32_vjp", boxes_dev, n, nf, H, W, st)) return -1;
    const int S = t->cfg.image_size;
    const size_t need = (size_t)n * 3 * H * S;
    if (clipvis_grow_rows(t, "loco_clipvis_preprocess_f32_vjp", need)) return -1;
    hipLaunchKernelGGL(clipvis_win_y_cot_kernel, dim3(blocks256((long)need)), dim3(256), 0, st, g_pixel_dev, boxes_dev, n, H, W, S,
                       t->cfg.image_std[0], t->cfg.image_std[1], t->cfg.image_std[2], t->rows);
    hipLaunchKernelGGL(clipvis_win_x_cot_kernel, dim3(blocks256((long)nf * 3 * H * W)), dim3(256), 0, st, t->rows, boxes_dev, n, nf, H, W, S,
                       g_frames_dev);
    if (hipGetLastError() != hipSuccess) return t->fail("loco_clipvis_preprocess_f32_vjp: kernel launch failed");
    return 0;
}

const char* loco_clipvis_last_error(loco_clipvis* t) { return t ? t->err.c_str() : g_clipvis_create_err.c_str(); }

void loco_clipvis_destroy(loco_clipvis* t) { delete t; }

}  // extern "C"
