// CLIP image encoder of the edit scores (include/loco_hip.h loco_clipvis_*): the CLIPVisionModelWithProjection of transformers
// -- patch embedding without bias, class token, learned position embedding, pre_layrnorm, `layers` pre-LN blocks of full
// (unmasked) multi-head self-attention and an MLP, post_layernorm of the class token, visual_projection -- and the image
// preprocessing of CLIPImageProcessor in float arithmetic.  Exact fp32 throughout, fp32 storage.
//
// Layout: that of the text encoders (textenc.hip) -- the T = 1 + G^2 tokens of all n images of a call channel-major in ONE
// [D][Tp] tensor, token column i * T + t (t = 0: the class token, t = 1 + row * G + col: a patch), Tp = n * T rounded up to
// 16; the padding columns are zero-fed and stay independent of the real ones.  The patch projection, the packed q | k | v
// operator, out_proj, fc1 (with its activation), fc2 and visual_projection are launch_gemm_fixed, the LayerNorms xfmr.hip's
// launch_ln_fwd.  New here: the batched patch gather, the class / position add, the attention (the scheme of samenc.hip's
// sam_attn_kernel without its bias tables, written again in this unit: samenc.hip is untouched), the class column gather,
// the transposes of the results, and the two resize passes of the preprocessing.  Every kernel computes a token column
// from the columns of its own image alone, in a fixed order: an image's rows are bit-identical whatever n and its position.
#include "encoder_common.h"

#include <cmath>

struct ClipVisLayer { float *ln1_g, *ln1_b, *wqkv, *bqkv, *wo, *bo, *ln2_g, *ln2_b, *w1, *b1, *w2, *b2; };

struct loco_clipvis : loco::EncoderBase {
    loco_clipvis_cfg cfg;
    int max_images = 0, G = 0, T = 0, Tmax = 0, Nmax = 0, hd = 0;
    long frows = 0;                                // rows of f: max(mlp_dim, 3 patch^2)
    float *cls = nullptr, *patch_w = nullptr, *pos = nullptr, *pre_g = nullptr, *pre_b = nullptr, *post_g = nullptr,
          *post_b = nullptr, *proj = nullptr;
    std::vector<ClipVisLayer> layer;
    float *h = nullptr, *x = nullptr, *qkv = nullptr, *attn = nullptr, *f = nullptr, *stats = nullptr, *pool = nullptr,
          *pooln = nullptr, *emb = nullptr;
    float* rows = nullptr;                         // the preprocessing's horizontally resized rows, grown on demand
    size_t rows_floats = 0;
    ~loco_clipvis() override {
        loco::DeviceGuard dg(device);
        if (rows) (void)hipFree(rows);
    }
};

namespace loco {
namespace {

constexpr int CV_THREADS = 256, CV_WAVES = CV_THREADS / 64, CV_QW = 4, CV_QB = CV_WAVES * CV_QW, CV_KC = 64;

// P[(ci ps + ky) ps + kx][i T + 1 + ty G + tx] = pix[i][ci][ty ps + ky][tx ps + kx]; 0 in the class and the padding columns
__global__ __launch_bounds__(256) void clipvis_patch_kernel(const float* pix, int S, int ps, int G, int T, int nT, int Tp, float* P) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)3 * ps * ps * Tp) return;
    const int r = (int)(e / Tp), col = (int)(e % Tp);
    float v = 0.f;
    const int i = col / T, t = col % T;
    if (col < nT && t > 0) {
        const int ci = r / (ps * ps), ky = (r / ps) % ps, kx = r % ps, ty = (t - 1) / G, tx = (t - 1) % G;
        v = pix[(((long)i * 3 + ci) * S + ty * ps + ky) * S + tx * ps + kx];
    }
    P[e] = v;
}

// h[c][i T + t] += pos[t][c] (+ cls[c] at t = 0) for the real columns
__global__ __launch_bounds__(256) void clipvis_embed_kernel(float* h, const float* cls, const float* pos, int D, int T, int nT, int Tp) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)D * nT) return;
    const int c = (int)(e / nT), col = (int)(e % nT), t = col % T;
    float v = h[(long)c * Tp + col] + pos[(long)t * D + c];
    if (t == 0) v += cls[c];
    h[(long)c * Tp + col] = v;
}

// parts of clipvis_attn_kernel's LDS start at multiples of 4 floats (float4 reads of Qs and Ps)
__host__ __device__ constexpr size_t cv_r4(size_t n) { return (n + 3) / 4 * 4; }

// One workgroup per (query block of 16, head, image): the T keys of the image are streamed in order in chunks of 64 -- K
// [hd][64] and V [64][hd + 1] of the chunk in LDS.  A wave owns 4 queries; lane j scores key k0 + j against them,
// (q scale) . k, then the running max / sum update (fp32, max and sum over the chunk by shuffles), then lane c (and c + 64)
// adds P V of the chunk to its output channel in key order.  qkv: [3 D][ld] = q | k | v channel rows, out [D][ld]; hd <= 128.
__global__ __launch_bounds__(CV_THREADS) void clipvis_attn_kernel(const float* qkv, long ld, int D, int hd, int T, float scale, float* out) {
    extern __shared__ __align__(16) float cv_sm[];
    const int hdp = hd + 1;
    float* Ks = cv_sm;                                     // [hd][64]
    float* Vs = Ks + cv_r4(hd * CV_KC);                    // [64][hd + 1]
    float* Qs = Vs + cv_r4(CV_KC * hdp);                   // [hd][16]
    float* Ps = Qs + cv_r4(hd * CV_QB);                    // [waves][64][4]
    const int qb = blockIdx.x, h = blockIdx.y, img = blockIdx.z;
    const long col0 = (long)img * T;
    const int q0 = qb * CV_QB;
    const float* q = qkv + (long)(h * hd) * ld + col0;
    const float* k = qkv + (long)(D + h * hd) * ld + col0;
    const float* v = qkv + (long)(2 * D + h * hd) * ld + col0;
    for (int e = threadIdx.x; e < hd * CV_QB; e += CV_THREADS) {
        const int c = e / CV_QB, ql = min(q0 + e % CV_QB, T - 1);
        Qs[e] = q[(long)c * ld + ql] * scale;
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int c0 = lane < hd ? lane : 0, c1 = lane + 64 < hd ? lane + 64 : 0;
    float* pw = Ps + wv * (CV_KC * CV_QW);
    float m[CV_QW], l[CV_QW], o0[CV_QW], o1[CV_QW];
#pragma unroll
    for (int u = 0; u < CV_QW; ++u) { m[u] = -INFINITY; l[u] = 0.f; o0[u] = 0.f; o1[u] = 0.f; }
    for (int k0 = 0; k0 < T; k0 += CV_KC) {
        __syncthreads();
        for (int e = threadIdx.x; e < hd * CV_KC; e += CV_THREADS) {
            const int c = e / CV_KC, j = e % CV_KC, kj = k0 + j;
            const bool ok = kj < T;
            Ks[e] = ok ? k[(long)c * ld + kj] : 0.f;
            Vs[j * hdp + c] = ok ? v[(long)c * ld + kj] : 0.f;
        }
        __syncthreads();
        const bool valid = k0 + lane < T;
        float s[CV_QW];
#pragma unroll
        for (int u = 0; u < CV_QW; ++u) s[u] = 0.f;
        for (int c = 0; c < hd; ++c) {
            const float kv = Ks[c * CV_KC + lane];
            const float4 qv = *reinterpret_cast<const float4*>(Qs + c * CV_QB + wv * CV_QW);
            s[0] = fmaf(qv.x, kv, s[0]);
            s[1] = fmaf(qv.y, kv, s[1]);
            s[2] = fmaf(qv.z, kv, s[2]);
            s[3] = fmaf(qv.w, kv, s[3]);
        }
#pragma unroll
        for (int u = 0; u < CV_QW; ++u) {
            const float sc = valid ? s[u] : -INFINITY;     // key k0 is always live: the chunk's max is finite
            const float mn = fmaxf(m[u], wave_max(sc));
            const float corr = expf(m[u] - mn);
            const float p = valid ? expf(sc - mn) : 0.f;
            l[u] = l[u] * corr + wave_sum(p);
            o0[u] *= corr;
            o1[u] *= corr;
            m[u] = mn;
            pw[lane * CV_QW + u] = p;
        }
        __syncthreads();
        for (int j = 0; j < CV_KC; ++j) {
            const float4 pv = *reinterpret_cast<const float4*>(pw + j * CV_QW);
            const float v0 = Vs[j * hdp + c0];
            o0[0] = fmaf(pv.x, v0, o0[0]);
            o0[1] = fmaf(pv.y, v0, o0[1]);
            o0[2] = fmaf(pv.z, v0, o0[2]);
            o0[3] = fmaf(pv.w, v0, o0[3]);
            if (hd > 64) {                                 // uniform
                const float v1 = Vs[j * hdp + c1];
                o1[0] = fmaf(pv.x, v1, o1[0]);
                o1[1] = fmaf(pv.y, v1, o1[1]);
                o1[2] = fmaf(pv.z, v1, o1[2]);
                o1[3] = fmaf(pv.w, v1, o1[3]);
            }
        }
    }
#pragma unroll
    for (int u = 0; u < CV_QW; ++u) {
        const int ql = q0 + wv * CV_QW + u;
        if (ql >= T) continue;
        const float inv = 1.0f / l[u];
        if (lane < hd) out[(long)(h * hd + lane) * ld + col0 + ql] = o0[u] * inv;
        if (lane + 64 < hd) out[(long)(h * hd + lane + 64) * ld + col0 + ql] = o1[u] * inv;
    }
}

// pool[c][i] = h[c][i T] (the class column of image i) for i < n, 0 in the padding columns
__global__ __launch_bounds__(256) void clipvis_pool_kernel(const float* h, int D, int T, int Tp, int n, int Np, float* pool) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)D * Np) return;
    const int c = (int)(e / Np), i = (int)(e % Np);
    pool[e] = i < n ? h[(long)c * Tp + (long)i * T] : 0.f;
}

// out[col][c] = x[c][col] for the first `cols` columns of x [C][ld]
__global__ __launch_bounds__(256) void clipvis_transpose_kernel(const float* x, int ld, int cols, int C, float* out) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)cols * C) return;
    const int col = (int)(e / C), c = (int)(e % C);
    out[e] = x[(long)c * ld + col];
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

}  // namespace
}  // namespace loco

using namespace loco;

namespace {
thread_local std::string g_clipvis_create_err;

// the carve-up of clipvis_attn_kernel's LDS
size_t clipvis_attn_lds_floats(int hd) {
    return cv_r4((size_t)hd * CV_KC) + cv_r4((size_t)CV_KC * (hd + 1)) + cv_r4((size_t)hd * CV_QB) + (size_t)CV_WAVES * CV_KC * CV_QW;
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
        if (clipvis_attn_lds_floats((int)hd) * sizeof(float) > 65536)
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
        // names of transformers' CLIPVisionModelWithProjection without the `vision_model.` prefix; q / k / v land in one packed
        // [3 D][D] operator
        ParamTable& pt = t.table;
        pt.add("embeddings.class_embedding", {D}, &t.cls);
        pt.add("embeddings.patch_embedding.weight", {D, 3, ps, ps}, &t.patch_w);
        pt.add("embeddings.position_embedding.weight", {t.T, D}, &t.pos);
        pt.add("pre_layrnorm.weight", {D}, &t.pre_g);
        pt.add("pre_layrnorm.bias", {D}, &t.pre_b);
        t.layer.resize(c.layers);
        for (int l = 0; l < c.layers; ++l) {
            const std::string p = "encoder.layers." + std::to_string(l) + ".";
            ClipVisLayer& ly = t.layer[l];
            pt.add(p + "layer_norm1.weight", {D}, &ly.ln1_g);
            pt.add(p + "layer_norm1.bias", {D}, &ly.ln1_b);
            const size_t wq = pt.reserve((size_t)3 * D * D, &ly.wqkv), bq = pt.reserve(round64(3 * D), &ly.bqkv);
            const char* qkvn[3] = {"q_proj", "k_proj", "v_proj"};
            for (int j = 0; j < 3; ++j) {
                pt.view(p + "self_attn." + qkvn[j] + ".weight", {D, D}, wq + (size_t)j * D * D);
                pt.view(p + "self_attn." + qkvn[j] + ".bias", {D}, bq + (size_t)j * D);
            }
            pt.add(p + "self_attn.out_proj.weight", {D, D}, &ly.wo);
            pt.add(p + "self_attn.out_proj.bias", {D}, &ly.bo);
            pt.add(p + "layer_norm2.weight", {D}, &ly.ln2_g);
            pt.add(p + "layer_norm2.bias", {D}, &ly.ln2_b);
            pt.add(p + "mlp.fc1.weight", {F, D}, &ly.w1);
            pt.add(p + "mlp.fc1.bias", {F}, &ly.b1);
            pt.add(p + "mlp.fc2.weight", {D, F}, &ly.w2);
            pt.add(p + "mlp.fc2.bias", {D}, &ly.b2);
        }
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
    if (need > t->rows_floats) {
        if (t->rows) (void)hipFree(t->rows);         // (waits for the launches that read it)
        t->rows = nullptr; t->rows_floats = 0;
        if (hipMalloc(&t->rows, need * sizeof(float)) != hipSuccess) return t->fail("loco_clipvis_preprocess: hipMalloc failed");
        t->rows_floats = need;
    }
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
    const int D = c.width, F = c.mlp_dim, P = c.projection_dim, ps = c.patch_size, PK = 3 * ps * ps;
    const int G = t->G, T = t->T, hd = t->hd, nT = n * T, Tp = (nT + 15) / 16 * 16, Np = (n + 15) / 16 * 16;
    const float scale = 1.0f / std::sqrt((float)hd);
    const int gact = c.act == 0 ? GEMM_ACT_QUICK_GELU : GEMM_ACT_GELU;
    hipLaunchKernelGGL(clipvis_patch_kernel, dim3(blocks256((long)PK * Tp)), dim3(256), 0, st, pixel_values, c.image_size, ps, G, T, nT, Tp,
                       t->f);
    launch_gemm_fixed(enc_linear(t->patch_w, nullptr, t->f, t->x, nullptr, D, PK, Tp), GEMM_ACT_NONE, st);
    hipLaunchKernelGGL(clipvis_embed_kernel, dim3(blocks256((long)D * nT)), dim3(256), 0, st, t->x, t->cls, t->pos, D, T, nT, Tp);
    launch_ln_fwd(t->x, 0, 1, D, Tp, t->pre_g, t->pre_b, c.ln_eps, t->h, 0, t->stats, 0, st);
    for (const ClipVisLayer& ly : t->layer) {
        launch_ln_fwd(t->h, 0, 1, D, Tp, ly.ln1_g, ly.ln1_b, c.ln_eps, t->x, 0, t->stats, 0, st);
        launch_gemm_fixed(enc_linear(ly.wqkv, ly.bqkv, t->x, t->qkv, nullptr, 3 * D, D, Tp), GEMM_ACT_NONE, st);
        hipLaunchKernelGGL(clipvis_attn_kernel, dim3((T + CV_QB - 1) / CV_QB, c.heads, n), dim3(CV_THREADS),
                           clipvis_attn_lds_floats(hd) * sizeof(float), st, t->qkv, (long)Tp, D, hd, T, scale, t->attn);
        launch_gemm_fixed(enc_linear(ly.wo, ly.bo, t->attn, t->h, t->h, D, D, Tp), GEMM_ACT_NONE, st);
        launch_ln_fwd(t->h, 0, 1, D, Tp, ly.ln2_g, ly.ln2_b, c.ln_eps, t->x, 0, t->stats, 0, st);
        launch_gemm_fixed(enc_linear(ly.w1, ly.b1, t->x, t->f, nullptr, F, D, Tp), gact, st);
        launch_gemm_fixed(enc_linear(ly.w2, ly.b2, t->f, t->h, t->h, D, F, Tp), GEMM_ACT_NONE, st);
    }
    if (hidden_dev) hipLaunchKernelGGL(clipvis_transpose_kernel, dim3(blocks256((long)nT * D)), dim3(256), 0, st, t->h, Tp, nT, D, hidden_dev);
    // pooling and heads: class columns -> post_layernorm -> visual_projection
    hipLaunchKernelGGL(clipvis_pool_kernel, dim3(blocks256((long)D * Np)), dim3(256), 0, st, t->h, D, T, Tp, n, Np, t->pool);
    launch_ln_fwd(t->pool, 0, 1, D, Np, t->post_g, t->post_b, c.ln_eps, t->pooln, 0, t->stats, 0, st);
    if (pooled_dev) hipLaunchKernelGGL(clipvis_transpose_kernel, dim3(blocks256((long)n * D)), dim3(256), 0, st, t->pooln, Np, n, D, pooled_dev);
    launch_gemm_fixed(enc_linear(t->proj, nullptr, t->pooln, t->emb, nullptr, P, D, Np), GEMM_ACT_NONE, st);
    hipLaunchKernelGGL(clipvis_transpose_kernel, dim3(blocks256((long)n * P)), dim3(256), 0, st, t->emb, Np, n, P, embeds_dev);
    if (hipGetLastError() != hipSuccess) return t->fail("loco_clipvis_encode: kernel launch failed");
    return 0;
}

const char* loco_clipvis_last_error(loco_clipvis* t) { return t ? t->err.c_str() : g_clipvis_create_err.c_str(); }

void loco_clipvis_destroy(loco_clipvis* t) { delete t; }

}  // extern "C"
