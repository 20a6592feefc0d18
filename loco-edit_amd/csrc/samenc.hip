// Image encoder of Segment Anything (include/loco_hip.h loco_sam_*): the SamVisionEncoder of transformers (a ViT with
// windowed and global attention, decomposed relative position bias and a convolutional neck) that the reference's
// mask_segmentation.py runs through the mask-generation pipeline.  Exact fp32 throughout, fp32 storage.
//
// Layout: that of the text encoders (textenc.hip) -- the G x G tokens of the one image channel-major in [D][Tp], token
// column row * G + col, Tp = G * G rounded up to 16.  A windowed layer works on a second column order, [D][Twp]: column
// w * ws^2 + r * ws + c of window w, the map zero-padded at the bottom and right to a multiple of ws AFTER the LayerNorm (so
// the padded tokens' k and v are the qkv biases, as in transformers); its attention output goes through proj in that
// order and is scattered back (cropped) with the residual.  The linear layers, the 1x1 neck conv and the 3x3 neck conv
// (im2col) are launch_gemm_fixed, the LayerNorms -- the per-pixel channel LayerNorm of the neck included -- xfmr.hip's
// launch_ln_fwd.  New here: the partition / un-partition, the relative position tables rel_h / rel_w [heads][T][size] from
// the unscaled queries, and the im2col.  The patch gather and the attention of both regimes are encoder_kernels.hip's, shared
// with the CLIP image tower: a workgroup owns 16 queries of one (window, head) and streams the keys in order in chunks of 64
// through LDS with a running max and sum -- here with the two tables added to the score -- so the T x T scores never reach
// memory.  Every sum runs in a fixed order set by compile-time constants.
#include "encoder_common.h"

#include <cmath>

struct SamLayer {
    float *ln1_g, *ln1_b, *wqkv, *bqkv, *rel_h, *rel_w, *wo, *bo, *ln2_g, *ln2_b, *w1, *b1, *w2, *b2;
    bool global = false;
};
struct SamTimed { int cat; hipEvent_t a, b; };

struct loco_sam : loco::EncoderBase {
    loco_sam_cfg cfg;
    int G = 0, T = 0, Tp = 0, hd = 0;
    int nwx = 0, Tw = 0, Twp = 0, ld = 0;        // windows per side, tokens of the padded windowed order, max(Tp, Twp)
    long frows = 0;                                // rows of f: max(mlp_dim, 9 out_channels, 3 patch^2)
    float *patch_w = nullptr, *patch_b = nullptr, *pos = nullptr, *neck_w1 = nullptr, *neck_g1 = nullptr, *neck_b1 = nullptr,
          *neck_w2 = nullptr, *neck_g2 = nullptr, *neck_b2 = nullptr;
    std::vector<SamLayer> layer;
    float *h = nullptr, *x = nullptr, *xw = nullptr, *qkv = nullptr, *attn = nullptr, *y = nullptr, *f = nullptr, *stats = nullptr,
          *relh = nullptr, *relw = nullptr, *n1 = nullptr, *n2 = nullptr;
    bool profile = false;
    std::vector<SamTimed> timed;                   // event pairs of the last profiled encode
    std::vector<hipEvent_t> pool;
    ~loco_sam() override {
        loco::DeviceGuard dg(device);
        for (hipEvent_t e : pool) (void)hipEventDestroy(e);
    }
};

namespace loco {
namespace {

// h[c][t] += pos[t][c] (pos_embed is stored token-major [G][G][D])
__global__ __launch_bounds__(256) void sam_add_pos_kernel(float* h, const float* pos, int D, int T, int Tp) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)D * T) return;
    const int c = (int)(e / T), t = (int)(e % T);
    h[(long)c * Tp + t] += pos[(long)t * D + c];
}

// xw[c][w ws^2 + r ws + cc] = x[c][(wr ws + r) G + wc ws + cc] inside the map, 0 in the padding and in the columns >= Tw
__global__ __launch_bounds__(256) void sam_partition_kernel(const float* x, int D, int G, int Tp, int ws, int nwx, int Tw, int Twp,
                                                            float* xw) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)D * Twp) return;
    const int c = (int)(e / Twp), col = (int)(e % Twp);
    float v = 0.f;
    if (col < Tw) {
        const int w = col / (ws * ws), l = col % (ws * ws);
        const int row = (w / nwx) * ws + l / ws, cc = (w % nwx) * ws + l % ws;
        if (row < G && cc < G) v = x[(long)c * Tp + row * G + cc];
    }
    xw[e] = v;
}

// h[c][t] += y[c][column of token t in the windowed order]: un-partition, crop and residual in one pass
__global__ __launch_bounds__(256) void sam_unpartition_kernel(const float* y, int D, int G, int T, int Tp, int ws, int nwx, int Twp,
                                                              float* h) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)D * T) return;
    const int c = (int)(e / T), t = (int)(e % T);
    const int row = t / G, cc = t % G;
    const int col = ((row / ws) * nwx + cc / ws) * ws * ws + (row % ws) * ws + cc % ws;
    h[(long)c * Tp + t] += y[(long)c * Twp + col];
}

// rel_h[h][t][j] = sum_c q[h hd + c][t] Rh[row(t) - j + size - 1][c], rel_w likewise with the column of t; t runs over the
// Tall tokens of the layer's column order, row / column inside its window (size = ws) or the map (size = G); c in order
__global__ __launch_bounds__(256) void sam_relpos_kernel(const float* q, long ld, int hd, int heads, long Tall, int size,
                                                         const float* Rh, const float* Rw, float* relh, float* relw) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)heads * Tall * size) return;
    const int j = (int)(e % size);
    const long ht = e / size;
    const int h = (int)(ht / Tall);
    const long t = ht % Tall;
    const int l = (int)(t % ((long)size * size)), qr = l / size, qc = l % size;
    const float* qp = q + (long)(h * hd) * ld + t;
    const float* rh = Rh + (long)(qr - j + size - 1) * hd;
    const float* rw = Rw + (long)(qc - j + size - 1) * hd;
    float ah = 0.f, aw = 0.f;
    for (int c = 0; c < hd; ++c) {
        const float qv = qp[(long)c * ld];
        ah = fmaf(qv, rh[c], ah);
        aw = fmaf(qv, rw[c], aw);
    }
    relh[e] = ah;
    relw[e] = aw;
}

// col[(ci 9 + ky 3 + kx)][t] = x[ci][(row + ky - 1) G + col + kx - 1] inside the map, 0 outside and in the padding columns
__global__ __launch_bounds__(256) void sam_im2col3_kernel(const float* x, int C, int G, int T, int Tp, float* colbuf) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)C * 9 * Tp) return;
    const int r = (int)(e / Tp), t = (int)(e % Tp);
    float v = 0.f;
    if (t < T) {
        const int ci = r / 9, ky = (r % 9) / 3, kx = r % 3, row = t / G + ky - 1, cc = t % G + kx - 1;
        if (row >= 0 && row < G && cc >= 0 && cc < G) v = x[(long)ci * Tp + row * G + cc];
    }
    colbuf[e] = v;
}

// out[c][t] = x[c][t] for the T real columns of x [C][Tp]
__global__ __launch_bounds__(256) void sam_crop_kernel(const float* x, int C, int T, int Tp, float* out) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)C * T) return;
    out[e] = x[(e / T) * Tp + e % T];
}

}  // namespace
}  // namespace loco

using namespace loco;

namespace {
thread_local std::string g_sam_create_err;

struct SamTimer {             // brackets a run of launches with two events while the profile is on
    loco_sam* t; hipStream_t st; int at = -1;
    SamTimer(loco_sam* t_, hipStream_t st_, int cat) : t(t_), st(st_) {
        if (!t->profile) return;
        hipEvent_t a = nullptr, b = nullptr;
        if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return;
        t->pool.push_back(a); t->pool.push_back(b);
        (void)hipEventRecord(a, st);
        at = (int)t->timed.size();
        t->timed.push_back({cat, a, b});
    }
    ~SamTimer() { if (at >= 0) (void)hipEventRecord(t->timed[at].b, st); }
};
enum { SAM_CAT_GEMM = 0, SAM_CAT_WIN_ATTN = 1, SAM_CAT_GLOBAL_ATTN = 2, SAM_CAT_OTHER = 3 };
}  // namespace

extern "C" {

int loco_sam_create(const loco_sam_cfg* cfg, int32_t device, loco_sam** out) {
    auto refuse = [](const loco_sam_cfg& c) -> std::string {
        if (c.image_size <= 0 || c.patch_size <= 0 || c.width <= 0 || c.depth <= 0 || c.heads <= 0 || c.mlp_dim <= 0 ||
            c.window_size <= 0 || c.out_channels <= 0)
            return "image_size, patch_size, width, depth, heads, mlp_dim, window_size and out_channels must be positive";
        if (c.image_size % c.patch_size) return "image_size is not a multiple of patch_size";
        if (c.width % c.heads) return "width is not a multiple of heads";
        if (c.num_global < 0 || c.num_global > LOCO_SAM_MAX_GLOBAL) return "num_global outside [0, 16]";
        for (int i = 0; i < c.num_global; ++i)
            if (c.global_attn[i] < 0 || c.global_attn[i] >= c.depth) return "a global attention index is outside [0, depth)";
        if (!(c.ln_eps > 0.f)) return "ln_eps must be positive";
        const int G = c.image_size / c.patch_size, hd = c.width / c.heads;
        if (hd > 128) return "head width > 128 (the attention kernel holds 2 channels per lane)";
        if (enc_attn_lds_floats(hd, std::max(G, c.window_size)) * sizeof(float) > 65536)
            return "head width x grid too large for the attention kernel's LDS (64 KiB)";
        return "";
    };
    return encoder_create<loco_sam>("loco_sam_create", g_sam_create_err, cfg, device, out, refuse, [&](loco_sam& t) {
        const loco_sam_cfg& c = t.cfg = *cfg;
        const int G = c.image_size / c.patch_size, hd = c.width / c.heads, ws = c.window_size;
        t.G = G; t.T = G * G; t.Tp = (t.T + 15) / 16 * 16; t.hd = hd;
        t.nwx = (G + ws - 1) / ws; t.Tw = t.nwx * t.nwx * ws * ws; t.Twp = (t.Tw + 15) / 16 * 16;
        t.ld = std::max(t.Tp, t.Twp);
        const long D = c.width, F = c.mlp_dim, Co = c.out_channels, ps = c.patch_size;
        t.frows = std::max(std::max(F, 9 * Co), 3 * ps * ps);
        // names of transformers' SamVisionEncoder, without a `vision_encoder.` prefix
        ParamTable& pt = t.table;
        pt.add("patch_embed.projection.weight", {D, 3, ps, ps}, &t.patch_w);
        pt.add("patch_embed.projection.bias", {D}, &t.patch_b);
        pt.add("pos_embed", {1, G, G, D}, &t.pos);
        t.layer.resize(c.depth);
        for (int i = 0; i < c.num_global; ++i) t.layer[c.global_attn[i]].global = true;
        for (int l = 0; l < c.depth; ++l) {
            const std::string p = "layers." + std::to_string(l) + ".";
            SamLayer& ly = t.layer[l];
            const long rel = 2 * (ly.global ? G : ws) - 1;       // transformers would interpolate another length: refused by the shape
            pt.add(p + "layer_norm1.weight", {D}, &ly.ln1_g);
            pt.add(p + "layer_norm1.bias", {D}, &ly.ln1_b);
            pt.add(p + "attn.qkv.weight", {3 * D, D}, &ly.wqkv);
            pt.add(p + "attn.qkv.bias", {3 * D}, &ly.bqkv);
            pt.add(p + "attn.rel_pos_h", {rel, hd}, &ly.rel_h);
            pt.add(p + "attn.rel_pos_w", {rel, hd}, &ly.rel_w);
            pt.add(p + "attn.proj.weight", {D, D}, &ly.wo);
            pt.add(p + "attn.proj.bias", {D}, &ly.bo);
            pt.add(p + "layer_norm2.weight", {D}, &ly.ln2_g);
            pt.add(p + "layer_norm2.bias", {D}, &ly.ln2_b);
            pt.add(p + "mlp.lin1.weight", {F, D}, &ly.w1);
            pt.add(p + "mlp.lin1.bias", {F}, &ly.b1);
            pt.add(p + "mlp.lin2.weight", {D, F}, &ly.w2);
            pt.add(p + "mlp.lin2.bias", {D}, &ly.b2);
        }
        pt.add("neck.conv1.weight", {Co, D, 1, 1}, &t.neck_w1);
        pt.add("neck.layer_norm1.weight", {Co}, &t.neck_g1);
        pt.add("neck.layer_norm1.bias", {Co}, &t.neck_b1);
        pt.add("neck.conv2.weight", {Co, Co, 3, 3}, &t.neck_w2);
        pt.add("neck.layer_norm2.weight", {Co}, &t.neck_g2);
        pt.add("neck.layer_norm2.bias", {Co}, &t.neck_b2);
        const long Tp = t.Tp, Twp = t.Twp, ld = t.ld;
        const size_t rel_floats = (size_t)c.heads * std::max((long)t.Tw * ws, (long)t.T * G);
        using B = EncoderBase;
        // zeroed: the padding columns of every buffer hold finite values from the first call on
        return t.alloc({B::buf(&t.h, D * Tp, true), B::buf(&t.x, D * Tp, true), B::buf(&t.xw, D * Twp, true), B::buf(&t.qkv, 3 * D * ld, true),
                        B::buf(&t.attn, D * ld, true), B::buf(&t.y, D * Twp, true), B::buf(&t.f, t.frows * Tp, true),
                        B::buf(&t.stats, 2 * ld, true), B::buf(&t.relh, rel_floats, true), B::buf(&t.relw, rel_floats, true),
                        B::buf(&t.n1, Co * Tp, true), B::buf(&t.n2, Co * Tp, true)});
    });
}

int loco_sam_load_param(loco_sam* t, const char* name, const float* host, const int64_t* shape, int32_t ndim) {
    return t ? t->table.load(name, host, shape, ndim, t->device, "loco_sam_load_param", t->err) : -1;
}

int loco_sam_params_missing(loco_sam* t) { return t ? t->table.missing(t->err) : -1; }

int loco_sam_encode(loco_sam* t, const float* pixel_values, float* out_dev, void* stream) {
    if (!t) return -1;
    if (!pixel_values || !out_dev) return t->fail("loco_sam_encode: null pixel_values or out");
    if (t->table.missing(t->err)) return -1;
    DeviceGuard dg(t->device);
    hipStream_t st = (hipStream_t)stream;
    const loco_sam_cfg& c = t->cfg;
    const int D = c.width, F = c.mlp_dim, Co = c.out_channels, ps = c.patch_size, ws = c.window_size, heads = c.heads;
    const int G = t->G, T = t->T, Tp = t->Tp, Tw = t->Tw, Twp = t->Twp, hd = t->hd, PK = 3 * ps * ps;
    const float scale = 1.0f / std::sqrt((float)hd);
    if (t->profile) {
        for (hipEvent_t e : t->pool) (void)hipEventDestroy(e);
        t->pool.clear();
        t->timed.clear();
    }
    {
        SamTimer tm(t, st, SAM_CAT_OTHER);
        launch_enc_patch(pixel_values, 1, c.image_size, ps, G, 0, Tp, t->f, st);
    }
    {
        SamTimer tm(t, st, SAM_CAT_GEMM);
        launch_gemm_fixed(enc_linear(t->patch_w, t->patch_b, t->f, t->h, nullptr, D, PK, Tp), GEMM_ACT_NONE, st);
    }
    {
        SamTimer tm(t, st, SAM_CAT_OTHER);
        hipLaunchKernelGGL(sam_add_pos_kernel, dim3(blocks256((long)D * T)), dim3(256), 0, st, t->h, t->pos, D, T, Tp);
    }
    for (const SamLayer& ly : t->layer) {
        const bool gl = ly.global;
        const int ldl = gl ? Tp : Twp, size = gl ? G : ws, nk = size * size, nwin = gl ? 1 : t->nwx * t->nwx;
        const long Tall = gl ? T : Tw;
        const float* xin = gl ? t->x : t->xw;
        const int acat = gl ? SAM_CAT_GLOBAL_ATTN : SAM_CAT_WIN_ATTN;
        {
            SamTimer tm(t, st, SAM_CAT_OTHER);
            launch_ln_fwd(t->h, 0, 1, D, Tp, ly.ln1_g, ly.ln1_b, c.ln_eps, t->x, 0, t->stats, 0, st);
            if (!gl) hipLaunchKernelGGL(sam_partition_kernel, dim3(blocks256((long)D * Twp)), dim3(256), 0, st, t->x, D, G, Tp, ws, t->nwx, Tw, Twp, t->xw);
        }
        {
            SamTimer tm(t, st, SAM_CAT_GEMM);
            launch_gemm_fixed(enc_linear(ly.wqkv, ly.bqkv, xin, t->qkv, nullptr, 3 * D, D, ldl), GEMM_ACT_NONE, st);
        }
        {
            SamTimer tm(t, st, acat);
            hipLaunchKernelGGL(sam_relpos_kernel, dim3(blocks256((long)heads * Tall * size)), dim3(256), 0, st, t->qkv, (long)ldl, hd, heads,
                               Tall, size, ly.rel_h, ly.rel_w, t->relh, t->relw);
            launch_enc_attn({t->qkv, (long)ldl, D, hd, nk, nwin, heads, scale, t->attn, t->relh, t->relw, Tall, size, nullptr}, st);
        }
        if (gl) {
            SamTimer tm(t, st, SAM_CAT_GEMM);
            launch_gemm_fixed(enc_linear(ly.wo, ly.bo, t->attn, t->h, t->h, D, D, Tp), GEMM_ACT_NONE, st);
        } else {
            {
                SamTimer tm(t, st, SAM_CAT_GEMM);
                launch_gemm_fixed(enc_linear(ly.wo, ly.bo, t->attn, t->y, nullptr, D, D, Twp), GEMM_ACT_NONE, st);
            }
            SamTimer tm(t, st, SAM_CAT_OTHER);
            hipLaunchKernelGGL(sam_unpartition_kernel, dim3(blocks256((long)D * T)), dim3(256), 0, st, t->y, D, G, T, Tp, ws, t->nwx, Twp, t->h);
        }
        {
            SamTimer tm(t, st, SAM_CAT_OTHER);
            launch_ln_fwd(t->h, 0, 1, D, Tp, ly.ln2_g, ly.ln2_b, c.ln_eps, t->x, 0, t->stats, 0, st);
        }
        SamTimer tm(t, st, SAM_CAT_GEMM);
        launch_gemm_fixed(enc_linear(ly.w1, ly.b1, t->x, t->f, nullptr, F, D, Tp), GEMM_ACT_GELU, st);
        launch_gemm_fixed(enc_linear(ly.w2, ly.b2, t->f, t->h, t->h, D, F, Tp), GEMM_ACT_NONE, st);
    }
    // neck: 1x1 conv -> LayerNorm over channels -> 3x3 conv (im2col) -> LayerNorm, eps 1e-6 as SamLayerNorm's default
    {
        SamTimer tm(t, st, SAM_CAT_GEMM);
        launch_gemm_fixed(enc_linear(t->neck_w1, nullptr, t->h, t->n1, nullptr, Co, D, Tp), GEMM_ACT_NONE, st);
    }
    {
        SamTimer tm(t, st, SAM_CAT_OTHER);
        launch_ln_fwd(t->n1, 0, 1, Co, Tp, t->neck_g1, t->neck_b1, 1e-6f, t->n2, 0, t->stats, 0, st);
        hipLaunchKernelGGL(sam_im2col3_kernel, dim3(blocks256((long)Co * 9 * Tp)), dim3(256), 0, st, t->n2, Co, G, T, Tp, t->f);
    }
    {
        SamTimer tm(t, st, SAM_CAT_GEMM);
        launch_gemm_fixed(enc_linear(t->neck_w2, nullptr, t->f, t->n1, nullptr, Co, 9 * Co, Tp), GEMM_ACT_NONE, st);
    }
    {
        SamTimer tm(t, st, SAM_CAT_OTHER);
        launch_ln_fwd(t->n1, 0, 1, Co, Tp, t->neck_g2, t->neck_b2, 1e-6f, t->n2, 0, t->stats, 0, st);
        hipLaunchKernelGGL(sam_crop_kernel, dim3(blocks256((long)Co * T)), dim3(256), 0, st, t->n2, Co, T, Tp, out_dev);
    }
    if (hipGetLastError() != hipSuccess) return t->fail("loco_sam_encode: kernel launch failed");
    return 0;
}

int loco_sam_profile(loco_sam* t, int32_t on) {
    if (!t) return -1;
    t->profile = on != 0;
    return 0;
}

int loco_sam_profile_read(loco_sam* t, float* ms4) {
    if (!t) return -1;
    if (!ms4) return t->fail("loco_sam_profile_read: ms4 is NULL");
    DeviceGuard dg(t->device);
    for (int i = 0; i < 4; ++i) ms4[i] = 0.f;
    for (const SamTimed& e : t->timed) {
        float ms = 0.f;
        if (hipEventSynchronize(e.b) != hipSuccess || hipEventElapsedTime(&ms, e.a, e.b) != hipSuccess)
            return t->fail("loco_sam_profile_read: reading an event failed");
        ms4[e.cat] += ms;
    }
    return 0;
}

const char* loco_sam_last_error(loco_sam* t) { return t ? t->err.c_str() : g_sam_create_err.c_str(); }

void loco_sam_destroy(loco_sam* t) { delete t; }

}  // extern "C"
