// Prompt encoder, mask decoder and mask scoring of Segment Anything (include/loco_hip.h loco_samdec_*): what
// mask_segmentation.SamHead and MaskGenerator.upsample / stability_score / mask_to_box compute, for point prompts with
// multimask_output = true.  Exact fp32 throughout, fp32 storage, every sum in an order fixed at compile time.
//
// Layout: the image tokens of prompt p channel-major in keys[p][C][Tp] (token column row * G + col, Tp = G * G rounded up to
// 16), as in the encoders, so the wide projections are launch_gemm_fixed with the prompt as the batch and the LayerNorm of
// the image tokens is xfmr.hip's launch_ln_fwd.  The NQ <= 8 tokens of a prompt (IoU token, mask tokens, the point, the
// padding point) live token-major in [P][8][C]; everything on their side -- embedding, self-attention, LayerNorms, MLP, the
// small projections, hypernetwork MLPs, IoU head -- is sd_tok_kernel, one workgroup per prompt with the rows in LDS.
//
//   set_image   src = emb + no_mask_embed, pos, layer 0's k / v of (src + pos, src) and its image -> token queries (the same
//               for every prompt), pos W_k / pos W_q of the later layers: (keys + pos) W = keys W + pos W, the second term
//               enters the projection as its residual operand.
//   token -> image attention   sd_t2i_kernel, a workgroup per (head, prompt): the 8 query rows against the T keys streamed in
//               chunks of 64 per wave with a running max / sum; the four waves' partial results merge in wave order.
//   image -> token attention   sd_i2t_kernel: a thread per image token and head turns its query (the projection's output) into
//               the attention output in place -- 8 scores in registers, never a T x NQ tensor.
//   upscaling   the first transposed convolution is a GEMM ([C / 4 * 4][C] x keys); sd_up_kernel reads one of its four
//               sub-pixels per thread, applies the channel LayerNorm + GELU, the second transposed convolution + GELU and the
//               product with the hyper-vectors: the maps at 4G x 4G x C / 8 stay in registers.
//   score / binarize   the two bilinear stages of MaskGenerator.upsample evaluated per output pixel from the low-resolution
//               logits; counts and boxes reduce in integers.
#include "enc_attn_launch.h"

#include <cmath>

namespace {
struct SdAttn { float *wq, *bq, *wk, *bk, *wv, *bv, *wo, *bo; };
struct SdLayer {
    SdAttn self, t2i, i2t;
    float *ln_g[4], *ln_b[4], *w1, *b1, *w2, *b2;
    float *posk = nullptr, *posq = nullptr;        // pos W_k (token -> image) and pos W_q (image -> token), [Ci][Tp]; layers >= 1
};
constexpr int SD_MAX_NM = 5, SD_MAX_MID = 4;
struct SdMlp { float *w_in, *b_in, *w_mid[SD_MAX_MID], *b_mid[SD_MAX_MID], *w_out, *b_out; };
}  // namespace

struct loco_samdec : loco::EncoderBase {
    loco_samdec_cfg cfg;
    int G = 0, T = 0, Tp = 0, C = 0, Ci = 0, NM = 0, NQ = 0, hmax = 0;
    float *pe = nullptr, *no_mask = nullptr, *nap = nullptr, *point1 = nullptr, *iou_tok = nullptr, *mask_tok = nullptr;
    std::vector<SdLayer> layer;
    SdAttn fin;
    float *lnf_g = nullptr, *lnf_b = nullptr, *up1_w = nullptr, *up1_b = nullptr, *up2_w = nullptr, *up2_b = nullptr, *upln_g = nullptr,
          *upln_b = nullptr, *fin_posk = nullptr;
    SdMlp hyper[SD_MAX_NM], iou;
    // per image
    float *src = nullptr, *pos = nullptr, *srcpos = nullptr, *k0 = nullptr, *v0 = nullptr, *q0 = nullptr, *posw = nullptr, *w2t = nullptr;
    // per prompt
    float *keys = nullptr, *proj = nullptr, *stats = nullptr, *tok = nullptr, *qry = nullptr, *qx = nullptr, *ox = nullptr, *kx = nullptr,
          *vx = nullptr, *hbuf = nullptr, *hyp = nullptr;
    bool image_set = false;
};

namespace loco {
namespace {

constexpr int SD_TH = 256, SD_WAVES = SD_TH / 64, SD_Q = 8, SD_KC = 64;

__device__ __forceinline__ float sd_gelu(float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752f)); }

// ------------------------------------------------------------------------------------------------------- per image
// src[c][t] = emb[c][t] + no_mask[c]; pos[c][t] = sin | cos (2 pi (x pe[0][j] + y pe[1][j])), j = c mod C / 2, x / y the cell
// centres of the grid in [-1, 1]; srcpos = src + pos; the padding columns t >= T are 0
__global__ __launch_bounds__(256) void sd_src_kernel(const float* emb, const float* no_mask, const float* pe, int C, int G, int T, int Tp,
                                                     float* src, float* pos, float* srcpos) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)C * Tp) return;
    const int c = (int)(e / Tp), t = (int)(e % Tp);
    float s = 0.f, p = 0.f;
    if (t < T) {
        const int half = C / 2, j = c % half;
        const float x = 2.0f * (((float)(t % G) + 0.5f) / (float)G) - 1.0f, y = 2.0f * (((float)(t / G) + 0.5f) / (float)G) - 1.0f;
        const float a = 6.283185307179586f * (x * pe[j] + y * pe[half + j]);
        p = c < half ? sinf(a) : cosf(a);
        s = emb[(long)c * T + t] + no_mask[c];
    }
    src[e] = s;
    pos[e] = p;
    srcpos[e] = s + p;
}

// w2t[(s * C8 + o) * C4 + c] = w2[(c * C8 + o) * 4 + s]: the second transposed convolution with the input channel fastest
__global__ __launch_bounds__(256) void sd_w2t_kernel(const float* w2, int C4, int C8, float* w2t) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= 4 * C8 * C4) return;
    const int c = e % C4, o = (e / C4) % C8, s = e / (C4 * C8);
    w2t[e] = w2[(c * C8 + o) * 4 + s];
}

// ------------------------------------------------------------------------------------------------------ token side
// out[r][o] = act(bias[o] + sum_k W[o][k] in[r][k]) (+ res[r][o]) for the R rows; k in order, K a multiple of 4, rows 16-byte
// aligned.  act: 0 none, 1 relu, 2 erf gelu.  in / out / res: LDS or global; out may be res.
template <int R>
__device__ __forceinline__ void sd_linear(const float* W, const float* bias, const float* in, int ldi, float* out, int ldo, int M, int K,
                                          int act, const float* res = nullptr, int ldr = 0) {
    for (int o = threadIdx.x; o < M; o += SD_TH) {
        float acc[R];
        const float b = bias[o];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = b;
        const float4* w4 = reinterpret_cast<const float4*>(W + (long)o * K);
        for (int k = 0; k < K; k += 4) {
            const float4 w = w4[k >> 2];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const float4 x = *reinterpret_cast<const float4*>(in + r * ldi + k);
                acc[r] = fmaf(w.x, x.x, acc[r]);
                acc[r] = fmaf(w.y, x.y, acc[r]);
                acc[r] = fmaf(w.z, x.z, acc[r]);
                acc[r] = fmaf(w.w, x.w, acc[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            float v = acc[r];
            if (act == 1) v = fmaxf(v, 0.f);
            else if (act == 2) v = sd_gelu(v);
            if (res) v += res[r * ldr + o];
            out[r * ldo + o] = v;
        }
    }
}

// LayerNorm of the rows r < nq of x[8][C] in place: wave w takes rows w, w + 4
__device__ __forceinline__ void sd_ln(float* x, int C, int nq, const float* g, const float* b, float eps) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int r = wv; r < nq; r += SD_WAVES) {
        float* xr = x + r * C;
        float s = 0.f;
        for (int c = lane; c < C; c += 64) s += xr[c];
        const float mean = wave_sum(s) / (float)C;
        float m2 = 0.f;
        for (int c = lane; c < C; c += 64) { const float d = xr[c] - mean; m2 += d * d; }
        const float rstd = rsqrtf(wave_sum(m2) / (float)C + eps);
        for (int c = lane; c < C; c += 64) xr[c] = (xr[c] - mean) * rstd * g[c] + b[c];
    }
}

// softmax(scale q k^T) v over the nq rows, per head: thread (head, query)
__device__ __forceinline__ void sd_self_attn(const float* q, const float* k, const float* v, float* out, int C, int H, int nq, float scale) {
    const int hd = C / H;
    for (int e = threadIdx.x; e < H * nq; e += SD_TH) {
        const int h = e / nq, qi = e % nq;
        const float* qp = q + qi * C + h * hd;
        float s[SD_Q];
#pragma unroll
        for (int j = 0; j < SD_Q; ++j) s[j] = 0.f;
        for (int c = 0; c < hd; ++c) {
            const float qv = qp[c];
#pragma unroll
            for (int j = 0; j < SD_Q; ++j) s[j] = fmaf(qv, k[j * C + h * hd + c], s[j]);
        }
        float m = -INFINITY;
#pragma unroll
        for (int j = 0; j < SD_Q; ++j) { s[j] = j < nq ? s[j] * scale : -INFINITY; m = fmaxf(m, s[j]); }
        float l = 0.f;
#pragma unroll
        for (int j = 0; j < SD_Q; ++j) { s[j] = expf(s[j] - m); l += s[j]; }
        const float inv = 1.0f / l;
        for (int c = 0; c < hd; ++c) {
            float o = 0.f;
#pragma unroll
            for (int j = 0; j < SD_Q; ++j) o = fmaf(s[j], v[j * C + h * hd + c], o);
            out[qi * C + h * hd + c] = o * inv;
        }
    }
}

struct SdAttnP { const float *wq, *bq, *wk, *bk, *wv, *bv, *wo, *bo; };
struct SdMlpP { const float *w_in, *b_in, *w_mid[SD_MAX_MID], *b_mid[SD_MAX_MID], *w_out, *b_out; };
enum { SD_ST_PRE = 0, SD_ST_MID = 1, SD_ST_FINAL_PRE = 2, SD_ST_FINAL_POST = 3 };
struct SdTok {
    int first, C, Ci, H, NQ, NM, mlp, act, iou_hid, iou_mid, hmax;
    float eps;
    const float *coords, *pe, *point1, *nap, *iou_tok, *mask_tok;
    SdAttnP self, cross, i2t;                  // cross: the token -> image attention of the stage (q_proj before, out_proj after)
    const float *ln1_g, *ln1_b, *ln2_g, *ln2_b, *ln3_g, *ln3_b, *w1, *b1, *w2, *b2;
    SdMlpP hyper[SD_MAX_NM], iou;
    float *tok, *qry, *qx, *ox, *kx, *vx, *hbuf, *hyp, *iou_out;
};

// One workgroup per prompt; LDS: six [8][C] row blocks X (queries), TK (tokens), A, B, Cc, D.  Rows >= NQ hold zeros or other
// finite values and are never keys.
//   PRE (layer l):   l = 0: the prompt's tokens; self-attention (+ residual from layer 1 on), LayerNorm 1, the token -> image
//                    queries qx = W_q (queries + tokens)
//   MID (layer l):   queries += out_proj(ox); LayerNorm 2; MLP; LayerNorm 3; kx / vx for the image -> token attention
//   FINAL_PRE:       qx of the final attention
//   FINAL_POST:      queries += out_proj(ox); the final LayerNorm; hyper-vectors; IoU head
template <int ST>
__global__ __launch_bounds__(SD_TH) void sd_tok_kernel(SdTok a) {
    extern __shared__ __align__(16) float sd_sm[];
    const int C = a.C, Ci = a.Ci, NQ = a.NQ, p = blockIdx.x, RB = SD_Q * C;
    float *X = sd_sm, *TK = X + RB, *A = TK + RB, *B = A + RB, *Cc = B + RB, *D = Cc + RB;
    float* tok = a.tok + (long)p * RB;
    float* qry = a.qry + (long)p * RB;
    float* qx = a.qx + (long)p * SD_Q * Ci;
    const float* ox = a.ox + (long)p * SD_Q * Ci;
    for (int e = threadIdx.x; e < 6 * RB; e += SD_TH) sd_sm[e] = 0.f;
    __syncthreads();
    if (ST == SD_ST_PRE && a.first) {
        const float cx = a.coords[2 * p], cy = a.coords[2 * p + 1];
        const int half = C / 2;
        for (int e = threadIdx.x; e < NQ * C; e += SD_TH) {
            const int r = e / C, c = e % C;
            float v;
            if (r == 0) v = a.iou_tok[c];
            else if (r <= a.NM) v = a.mask_tok[(r - 1) * C + c];
            else if (r == a.NM + 1) {
                const int j = c % half;
                const float ang = 6.283185307179586f * (cx * a.pe[j] + cy * a.pe[half + j]);
                v = (c < half ? sinf(ang) : cosf(ang)) + a.point1[c];
            } else v = a.nap[c];
            TK[e] = v;
            X[e] = v;
            tok[e] = v;
        }
    } else {
        for (int e = threadIdx.x; e < NQ * C; e += SD_TH) { X[e] = qry[e]; TK[e] = tok[e]; }
    }
    __syncthreads();
    if constexpr (ST == SD_ST_PRE) {
        const float* qk = X;
        if (!a.first) {
            for (int e = threadIdx.x; e < NQ * C; e += SD_TH) D[e] = X[e] + TK[e];
            __syncthreads();
            qk = D;
        }
        sd_linear<SD_Q>(a.self.wq, a.self.bq, qk, C, A, C, C, C, 0);
        sd_linear<SD_Q>(a.self.wk, a.self.bk, qk, C, B, C, C, C, 0);
        sd_linear<SD_Q>(a.self.wv, a.self.bv, X, C, Cc, C, C, C, 0);
        __syncthreads();
        sd_self_attn(A, B, Cc, D, C, a.H, NQ, 1.0f / sqrtf((float)(C / a.H)));
        __syncthreads();
        sd_linear<SD_Q>(a.self.wo, a.self.bo, D, C, X, C, C, C, 0, a.first ? nullptr : X, C);
        __syncthreads();
        sd_ln(X, C, NQ, a.ln1_g, a.ln1_b, a.eps);
        __syncthreads();
    } else if constexpr (ST == SD_ST_MID || ST == SD_ST_FINAL_POST) {
        for (int e = threadIdx.x; e < NQ * Ci; e += SD_TH) A[e] = ox[e];
        __syncthreads();
        sd_linear<SD_Q>(a.cross.wo, a.cross.bo, A, Ci, X, C, C, Ci, 0, X, C);
        __syncthreads();
        sd_ln(X, C, NQ, a.ln2_g, a.ln2_b, ST == SD_ST_MID ? a.eps : 1e-5f);
        __syncthreads();
    }
    if constexpr (ST == SD_ST_MID) {
        float* hb = a.hbuf + (long)p * SD_Q * a.hmax;
        sd_linear<SD_Q>(a.w1, a.b1, X, C, hb, a.hmax, a.mlp, C, a.act);
        __syncthreads();
        sd_linear<SD_Q>(a.w2, a.b2, hb, a.hmax, X, C, C, a.mlp, 0, X, C);
        __syncthreads();
        sd_ln(X, C, NQ, a.ln3_g, a.ln3_b, a.eps);
        __syncthreads();
        for (int e = threadIdx.x; e < NQ * C; e += SD_TH) D[e] = X[e] + TK[e];
        __syncthreads();
        sd_linear<SD_Q>(a.i2t.wk, a.i2t.bk, D, C, a.kx + (long)p * SD_Q * Ci, Ci, Ci, C, 0);
        sd_linear<SD_Q>(a.i2t.wv, a.i2t.bv, X, C, a.vx + (long)p * SD_Q * Ci, Ci, Ci, C, 0);
    }
    if constexpr (ST == SD_ST_PRE || ST == SD_ST_FINAL_PRE) {
        for (int e = threadIdx.x; e < NQ * C; e += SD_TH) D[e] = X[e] + TK[e];
        __syncthreads();
        sd_linear<SD_Q>(a.cross.wq, a.cross.bq, D, C, qx, Ci, Ci, C, 0);
    }
    if constexpr (ST == SD_ST_FINAL_POST) {
        const int C8 = C / 8;
#pragma unroll
        for (int i = 0; i < SD_MAX_NM; ++i) {              // hyper-vector of mask token i (row 1 + i)
            if (i >= a.NM) break;
            sd_linear<1>(a.hyper[i].w_in, a.hyper[i].b_in, X + (1 + i) * C, 0, A, 0, C, C, 1);
            __syncthreads();
            sd_linear<1>(a.hyper[i].w_mid[0], a.hyper[i].b_mid[0], A, 0, B, 0, C, C, 1);
            __syncthreads();
            sd_linear<1>(a.hyper[i].w_out, a.hyper[i].b_out, B, 0, a.hyp + ((long)p * a.NM + i) * C8, 0, C8, C, 0);
            __syncthreads();
        }
        float *u = A, *w = B;                               // the IoU head on row 0
        sd_linear<1>(a.iou.w_in, a.iou.b_in, X, 0, u, 0, a.iou_hid, C, 1);
        __syncthreads();
#pragma unroll
        for (int j = 0; j < SD_MAX_MID; ++j) {
            if (j >= a.iou_mid) break;
            sd_linear<1>(a.iou.w_mid[j], a.iou.b_mid[j], u, 0, w, 0, a.iou_hid, a.iou_hid, 1);
            __syncthreads();
            float* s = u; u = w; w = s;
        }
        sd_linear<1>(a.iou.w_out, a.iou.b_out, u, 0, w, 0, a.NM, a.iou_hid, 0);
        __syncthreads();
        for (int e = threadIdx.x; e < a.NM - 1; e += SD_TH) a.iou_out[(long)p * (a.NM - 1) + e] = w[1 + e];
    } else {
        for (int e = threadIdx.x; e < NQ * C; e += SD_TH) qry[e] = X[e];
    }
}

// ------------------------------------------------------------------------------------- token -> image attention
// parts of the LDS start at multiples of 4 floats
__host__ __device__ constexpr size_t sd_r4(size_t n) { return (n + 3) / 4 * 4; }
__host__ __device__ constexpr size_t sd_t2i_lds_floats(int hd) {
    return sd_r4((size_t)SD_Q * hd) + SD_WAVES * (sd_r4((size_t)SD_KC * (hd + 1)) + SD_KC * SD_Q + SD_Q) + 2 * SD_WAVES * SD_Q +
           (size_t)SD_WAVES * SD_Q * hd;
}

// One workgroup per (head, prompt).  Wave w takes the key chunks w, w + 4, ... of 64 keys: lane j scores key k0 + j against the 8
// query rows (k read from memory, coalesced), the running max is the wave's, the running sum stays per lane until the end;
// the chunk's v goes through LDS as [64][hd + 1] and lane (c = lane mod hd, g = lane / hd) adds P V for channel c and the
// queries g qpg ... g qpg + qpg - 1 (qpg = 8 hd / 64 rounded up) in key order.  The waves' (max, sum, output) merge in wave order.
// qx / out [P][8][Ci], K / V [Ci][ld] per prompt (kbs = 0: the same for every prompt), hd a power of two <= 64.
__global__ __launch_bounds__(SD_TH) void sd_t2i_kernel(const float* qx, const float* K, const float* V, long kbs, long ld, int T, int Ci,
                                                       int hd, int NQ, float scale, float* out) {
    extern __shared__ __align__(16) float sd_sm[];
    const int h = blockIdx.x, p = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6, hdp = hd + 1;
    float* Qs = sd_sm;                                                       // [8][hd]
    float* Vs = Qs + sd_r4((size_t)SD_Q * hd) + wv * sd_r4((size_t)SD_KC * hdp);    // per wave [64][hd + 1]
    float* Pw = sd_sm + sd_r4((size_t)SD_Q * hd) + SD_WAVES * sd_r4((size_t)SD_KC * hdp) + wv * (SD_KC * SD_Q);   // per wave [64][8]
    float* Cw = sd_sm + sd_r4((size_t)SD_Q * hd) + SD_WAVES * (sd_r4((size_t)SD_KC * hdp) + SD_KC * SD_Q) + wv * SD_Q;   // per wave [8]
    float* Mm = sd_sm + sd_r4((size_t)SD_Q * hd) + SD_WAVES * (sd_r4((size_t)SD_KC * hdp) + SD_KC * SD_Q + SD_Q);   // [waves][8]
    float* Ll = Mm + SD_WAVES * SD_Q;                                       // [waves][8]
    float* Oo = Ll + SD_WAVES * SD_Q;                                       // [waves][8][hd]
    const float* kp = K + (long)p * kbs + (long)(h * hd) * ld;
    const float* vp = V + (long)p * kbs + (long)(h * hd) * ld;
    for (int e = threadIdx.x; e < SD_Q * hd; e += SD_TH) {
        const int r = e / hd, c = e % hd;
        Qs[e] = r < NQ ? qx[((long)p * SD_Q + r) * Ci + h * hd + c] * scale : 0.f;
    }
    __syncthreads();
    const int ng = 64 / hd, qpg = (SD_Q + ng - 1) / ng, c = lane % hd, q0 = (lane / hd) * qpg;
    float m[SD_Q], l[SD_Q], o[SD_Q];
#pragma unroll
    for (int u = 0; u < SD_Q; ++u) { m[u] = -INFINITY; l[u] = 0.f; o[u] = 0.f; }
    const int nchunk = (T + SD_KC - 1) / SD_KC;
    for (int ch0 = 0; ch0 < nchunk; ch0 += SD_WAVES) {
        const int k0 = (ch0 + wv) * SD_KC;
        const bool active = k0 < T;                        // uniform in the wave
        if (active) {
            const int kj = k0 + lane;
            const bool valid = kj < T;
            float s[SD_Q];
#pragma unroll
            for (int u = 0; u < SD_Q; ++u) s[u] = 0.f;
            for (int cc = 0; cc < hd; ++cc) {
                const float kv = valid ? kp[(long)cc * ld + kj] : 0.f;
                Vs[lane * hdp + cc] = valid ? vp[(long)cc * ld + kj] : 0.f;
#pragma unroll
                for (int u = 0; u < SD_Q; ++u) s[u] = fmaf(Qs[u * hd + cc], kv, s[u]);
            }
#pragma unroll
            for (int u = 0; u < SD_Q; ++u) {
                const float sc = valid ? s[u] : -INFINITY;
                const float mn = fmaxf(m[u], wave_max(sc));
                const float corr = expf(m[u] - mn);
                const float pr = valid ? expf(sc - mn) : 0.f;
                l[u] = l[u] * corr + pr;
                m[u] = mn;
                Pw[lane * SD_Q + u] = pr;
                if (lane == u) Cw[u] = corr;
            }
        }
        __syncthreads();
        if (active) {
#pragma unroll
            for (int u = 0; u < SD_Q; ++u) {
                if (u < qpg && q0 + u < SD_Q) {
                    const int q = q0 + u;
                    float acc = o[u] * Cw[q];
                    for (int j = 0; j < SD_KC; ++j) acc = fmaf(Pw[j * SD_Q + q], Vs[j * hdp + c], acc);
                    o[u] = acc;
                }
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int u = 0; u < SD_Q; ++u) {
        const float lu = wave_sum(l[u]);
        if (lane == u) { Mm[wv * SD_Q + u] = m[u]; Ll[wv * SD_Q + u] = lu; }
        if (u < qpg && q0 + u < SD_Q) Oo[(wv * SD_Q + q0 + u) * hd + c] = o[u];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < NQ * hd; e += SD_TH) {
        const int q = e / hd, cc = e % hd;
        float mx = -INFINITY;
#pragma unroll
        for (int w = 0; w < SD_WAVES; ++w) mx = fmaxf(mx, Mm[w * SD_Q + q]);
        float num = 0.f, den = 0.f;
#pragma unroll
        for (int w = 0; w < SD_WAVES; ++w) {
            const float f = expf(Mm[w * SD_Q + q] - mx);
            num = fmaf(f, Oo[(w * SD_Q + q) * hd + cc], num);
            den = fmaf(f, Ll[w * SD_Q + q], den);
        }
        out[((long)p * SD_Q + q) * Ci + h * hd + cc] = num / den;
    }
}

// ------------------------------------------------------------------------------------- image -> token attention
// Thread (image token t, head h, prompt p): the query q[h hd ...][t] against the NQ token keys kx, the softmax over them and
// the sum of the token values vx, written to out[h hd ...][t] (out may be q: a thread reads its whole query first).
// q [Ci][ld] per prompt (qbs = 0: the same for every prompt), out [P][Ci][ld], kx / vx [P][8][Ci]; columns t >= T become 0.
__global__ __launch_bounds__(SD_TH) void sd_i2t_kernel(const float* q, long qbs, const float* kx, const float* vx, long ld, int T, int Tp,
                                                       int Ci, int hd, int NQ, float scale, float* out) {
    extern __shared__ __align__(16) float sd_sm[];
    float *ks = sd_sm, *vs = sd_sm + SD_Q * hd;                             // [8][hd] each
    const int h = blockIdx.y, p = blockIdx.z, t = blockIdx.x * SD_TH + threadIdx.x;
    for (int e = threadIdx.x; e < SD_Q * hd; e += SD_TH) {
        const int r = e / hd, c = e % hd;
        const long o = ((long)p * SD_Q + r) * Ci + h * hd + c;
        ks[e] = r < NQ ? kx[o] : 0.f;
        vs[e] = r < NQ ? vx[o] : 0.f;
    }
    __syncthreads();
    if (t >= Tp) return;
    const float* qp = q + (long)p * qbs + (long)(h * hd) * ld + t;
    float* op = out + ((long)p * Ci + h * hd) * ld + t;
    if (t >= T) {
        for (int c = 0; c < hd; ++c) op[(long)c * ld] = 0.f;
        return;
    }
    float s[SD_Q];
#pragma unroll
    for (int j = 0; j < SD_Q; ++j) s[j] = 0.f;
    for (int c = 0; c < hd; ++c) {
        const float qv = qp[(long)c * ld];
#pragma unroll
        for (int j = 0; j < SD_Q; ++j) s[j] = fmaf(qv, ks[j * hd + c], s[j]);
    }
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < SD_Q; ++j) { s[j] = j < NQ ? s[j] * scale : -INFINITY; m = fmaxf(m, s[j]); }
    float l = 0.f;
#pragma unroll
    for (int j = 0; j < SD_Q; ++j) { s[j] = expf(s[j] - m); l += s[j]; }
    const float inv = 1.0f / l;
    for (int c = 0; c < hd; ++c) {
        float o = 0.f;
#pragma unroll
        for (int j = 0; j < SD_Q; ++j) o = fmaf(s[j], vs[j * hd + c], o);
        op[(long)c * ld] = o * inv;
    }
}

// ------------------------------------------------------------------------------------------------------- upscaling
// Thread (image token t, sub-pixel s1 = 2 dy + dx of the first transposed convolution, prompt p): the C4 = C / 4 channels
// u1[p][c 4 + s1][t] + b1[c] -> LayerNorm over c (eps 1e-6) -> GELU -> the second transposed convolution's four sub-pixels s2
// and C8 = C4 / 2 channels (+ b2, GELU) -> the product with the hyper-vectors of the mask tokens 1 ... NM - 1.
// masks[p][k - 1][4 ty + 2 dy1 + dy2][4 tx + 2 dx1 + dx2].  LDS: w2t [4][C8][C4], the hyper-vectors, biases and LayerNorm.
template <int C4>
__global__ __launch_bounds__(SD_TH) void sd_up_kernel(const float* u1, long ld, int T, int G, const float* b1, const float* lg, const float* lb,
                                                      const float* w2t, const float* b2, const float* hyp, int NM, float* masks) {
    constexpr int C8 = C4 / 2, NMO = SD_MAX_NM - 1;
    __shared__ __align__(16) float Ws[4 * C8 * C4];
    __shared__ float Hs[SD_MAX_NM * C8], B1[C4], Lg[C4], Lb[C4], B2[C8];
    const int s1 = blockIdx.y, p = blockIdx.z, t = blockIdx.x * SD_TH + threadIdx.x;
    for (int e = threadIdx.x; e < 4 * C8 * C4; e += SD_TH) Ws[e] = w2t[e];
    for (int e = threadIdx.x; e < SD_MAX_NM * C8; e += SD_TH) Hs[e] = e < NM * C8 ? hyp[(long)p * NM * C8 + e] : 0.f;
    for (int e = threadIdx.x; e < C4; e += SD_TH) { B1[e] = b1[e]; Lg[e] = lg[e]; Lb[e] = lb[e]; }
    for (int e = threadIdx.x; e < C8; e += SD_TH) B2[e] = b2[e];
    __syncthreads();
    if (t >= T) return;
    const float* up = u1 + (long)p * (4 * C4) * ld + (long)s1 * ld + t;
    float a[C4];
    float sum = 0.f;
#pragma unroll
    for (int c = 0; c < C4; ++c) { a[c] = up[(long)(4 * c) * ld] + B1[c]; sum += a[c]; }
    const float mean = sum / (float)C4;
    float m2 = 0.f;
#pragma unroll
    for (int c = 0; c < C4; ++c) { const float d = a[c] - mean; m2 += d * d; }
    const float rstd = rsqrtf(m2 / (float)C4 + 1e-6f);
#pragma unroll
    for (int c = 0; c < C4; ++c) a[c] = sd_gelu((a[c] - mean) * rstd * Lg[c] + Lb[c]);
    const int side = 4 * G, y0 = 4 * (t / G) + 2 * (s1 >> 1), x0 = 4 * (t % G) + 2 * (s1 & 1);
#pragma unroll
    for (int s2 = 0; s2 < 4; ++s2) {
        float acc[NMO];
#pragma unroll
        for (int k = 0; k < NMO; ++k) acc[k] = 0.f;
        for (int o = 0; o < C8; ++o) {
            const float4* w4 = reinterpret_cast<const float4*>(Ws + (s2 * C8 + o) * C4);
            float v = B2[o];
#pragma unroll
            for (int c = 0; c < C4; c += 4) {
                const float4 w = w4[c >> 2];
                v = fmaf(a[c], w.x, v);
                v = fmaf(a[c + 1], w.y, v);
                v = fmaf(a[c + 2], w.z, v);
                v = fmaf(a[c + 3], w.w, v);
            }
            v = sd_gelu(v);
#pragma unroll
            for (int k = 0; k < NMO; ++k) acc[k] = fmaf(Hs[(k + 1) * C8 + o], v, acc[k]);
        }
        const long pix = (long)(y0 + (s2 >> 1)) * side + x0 + (s2 & 1);
#pragma unroll
        for (int k = 0; k < NMO; ++k)
            if (k < NM - 1) masks[((long)p * (NM - 1) + k) * side * side + pix] = acc[k];
    }
}

// ----------------------------------------------------------------------------------------------- score / binarize
struct SdGeo { int h, w, oh, ow, rh, rw; float s1y, s1x, s2y, s2x; };

// source index pair and weight of output index d of a bilinear resampling with align_corners = false from n samples
__device__ __forceinline__ void sd_axis(int d, float scale, int n, int& i0, int& i1, float& l1) {
    const float src = fmaxf(scale * ((float)d + 0.5f) - 0.5f, 0.f);
    i0 = min((int)src, n - 1);
    i1 = min(i0 + 1, n - 1);
    l1 = fminf(fmaxf(src - (float)i0, 0.f), 1.f);
}
// the logit at (row Y, column X) of the map at image_size, from the low-resolution map
__device__ __forceinline__ float sd_stage1(const float* low, const SdGeo& g, int Y, int X) {
    int y0, y1, x0, x1;
    float ly, lx;
    sd_axis(Y, g.s1y, g.h, y0, y1, ly);
    sd_axis(X, g.s1x, g.w, x0, x1, lx);
    const float a = low[y0 * g.w + x0], b = low[y0 * g.w + x1], c = low[y1 * g.w + x0], d = low[y1 * g.w + x1];
    return (1.f - ly) * ((1.f - lx) * a + lx * b) + ly * ((1.f - lx) * c + lx * d);
}
// the logit at (y, x) of the original size: the second stage over the map cropped to rh x rw
__device__ __forceinline__ float sd_logit(const float* low, const SdGeo& g, int y, int x) {
    int y0, y1, x0, x1;
    float ly, lx;
    sd_axis(y, g.s2y, g.rh, y0, y1, ly);
    sd_axis(x, g.s2x, g.rw, x0, x1, lx);
    const float a = sd_stage1(low, g, y0, x0), b = sd_stage1(low, g, y0, x1), c = sd_stage1(low, g, y1, x0), d = sd_stage1(low, g, y1, x1);
    return (1.f - ly) * ((1.f - lx) * a + lx * b) + ly * ((1.f - lx) * c + lx * d);
}

__device__ __forceinline__ int sd_wave_isum(int v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ int sd_wave_imin(int v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ int sd_wave_imax(int v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}

// One workgroup per candidate n: counts[n] = { #(logit > thr + off), #(logit > thr - off) }, boxes[n] = inclusive XYXY box of
// logit > thr, 0 0 0 0 when empty.  Integer reductions: shuffles, then the waves through LDS.
__global__ __launch_bounds__(SD_TH) void sd_score_kernel(const float* low, SdGeo g, float thr, float off, int* counts, int* boxes) {
    __shared__ int red[SD_WAVES][6];
    const int n = blockIdx.x;
    const float* lp = low + (long)n * g.h * g.w;
    const float hi = thr + off, lo = thr - off;
    int chi = 0, clo = 0, xmin = g.ow, ymin = g.oh, xmax = -1, ymax = -1;
    for (int pix = threadIdx.x; pix < g.oh * g.ow; pix += SD_TH) {
        const int y = pix / g.ow, x = pix - y * g.ow;
        const float v = sd_logit(lp, g, y, x);
        chi += v > hi;
        clo += v > lo;
        if (v > thr) { xmin = min(xmin, x); ymin = min(ymin, y); xmax = max(xmax, x); ymax = max(ymax, y); }
    }
    chi = sd_wave_isum(chi); clo = sd_wave_isum(clo);
    xmin = sd_wave_imin(xmin); ymin = sd_wave_imin(ymin); xmax = sd_wave_imax(xmax); ymax = sd_wave_imax(ymax);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) { red[wv][0] = chi; red[wv][1] = clo; red[wv][2] = xmin; red[wv][3] = ymin; red[wv][4] = xmax; red[wv][5] = ymax; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < SD_WAVES; ++w) {
            chi += red[w][0]; clo += red[w][1];
            xmin = min(xmin, red[w][2]); ymin = min(ymin, red[w][3]); xmax = max(xmax, red[w][4]); ymax = max(ymax, red[w][5]);
        }
        const bool empty = xmax < xmin || ymax < ymin;
        counts[2 * n] = chi;
        counts[2 * n + 1] = clo;
        boxes[4 * n] = empty ? 0 : xmin;
        boxes[4 * n + 1] = empty ? 0 : ymin;
        boxes[4 * n + 2] = empty ? 0 : xmax;
        boxes[4 * n + 3] = empty ? 0 : ymax;
    }
}

// masks[k][y][x] = logit of row rows[k] > thr (a row outside [0, N) gives an empty mask)
__global__ __launch_bounds__(SD_TH) void sd_binarize_kernel(const float* low, int N, const int* rows, SdGeo g, float thr, unsigned char* masks) {
    const int k = blockIdx.y, pix = blockIdx.x * SD_TH + threadIdx.x;
    if (pix >= g.oh * g.ow) return;
    const int n = rows[k];
    unsigned char v = 0;
    if (n >= 0 && n < N) {
        const int y = pix / g.ow, x = pix - y * g.ow;
        v = sd_logit(low + (long)n * g.h * g.w, g, y, x) > thr;
    }
    masks[(long)k * g.oh * g.ow + pix] = v;
}

}  // namespace

size_t sd_t2i_lds_bytes(int hd) { return sd_t2i_lds_floats(hd) * sizeof(float); }

void launch_sd_t2i(const float* qx, const float* K, const float* V, long kbs, long ld, int T, int Ci, int hd, int heads, int P, int NQ,
                   float scale, float* out, hipStream_t st) {
    hipLaunchKernelGGL(sd_t2i_kernel, dim3(heads, P), dim3(SD_TH), sd_t2i_lds_bytes(hd), st, qx, K, V, kbs, ld, T, Ci, hd, NQ, scale, out);
}

void launch_sd_i2t(const float* q, long qbs, const float* kx, const float* vx, long ld, int T, int Tp, int Ci, int hd, int heads, int P,
                   int NQ, float scale, float* out, hipStream_t st) {
    hipLaunchKernelGGL(sd_i2t_kernel, dim3((Tp + SD_TH - 1) / SD_TH, heads, P), dim3(SD_TH), (size_t)2 * SD_Q * hd * sizeof(float), st, q, qbs,
                       kx, vx, ld, T, Tp, Ci, hd, NQ, scale, out);
}

}  // namespace loco

using namespace loco;

namespace {
thread_local std::string g_samdec_create_err;

SdAttnP attn_p(const SdAttn& a) { return {a.wq, a.bq, a.wk, a.bk, a.wv, a.bv, a.wo, a.bo}; }
SdMlpP mlp_p(const SdMlp& m) {
    SdMlpP r;
    r.w_in = m.w_in; r.b_in = m.b_in; r.w_out = m.w_out; r.b_out = m.b_out;
    for (int i = 0; i < SD_MAX_MID; ++i) { r.w_mid[i] = m.w_mid[i]; r.b_mid[i] = m.b_mid[i]; }
    return r;
}

// Y[b] [M][Tp] = W [M][K] X[b] [K][Tp] + bias (+ R[b]) for b < P; xbs / rbs = 0: the same operand for every prompt
GemmArgs sd_proj(const float* W, const float* bias, const float* X, long xbs, float* Y, const float* R, long rbs, int M, int K, int Tp, int P) {
    GemmArgs g = enc_linear(W, bias, X, Y, R, M, K, Tp);
    g.batch = P;
    g.sbb = xbs;
    g.scb = (long)M * Tp;
    g.srb = rbs;
    return g;
}

const char* sd_check_geo(int N, int h, int w, int oh, int ow, int rh, int rw, int S) {
    if (N < 0 || h <= 0 || w <= 0 || oh <= 0 || ow <= 0 || rh <= 0 || rw <= 0 || S <= 0) return "sizes must be positive";
    if (rh > S || rw > S) return "the reshaped size exceeds image_size";
    if ((long)oh * ow > (1L << 30) || (long)N * h * w > (1L << 40)) return "size out of range";
    return nullptr;
}
SdGeo sd_geo(int h, int w, int oh, int ow, int rh, int rw, int S) {
    return {h, w, oh, ow, rh, rw, (float)h / (float)S, (float)w / (float)S, (float)rh / (float)oh, (float)rw / (float)ow};
}
}  // namespace

extern "C" {

int loco_samdec_create(const loco_samdec_cfg* cfg, int32_t device, loco_samdec** out) {
    auto refuse = [](const loco_samdec_cfg& c) -> std::string {
        if (c.grid <= 0 || c.image_size <= 0 || c.hidden <= 0 || c.layers <= 0 || c.heads <= 0 || c.mlp_dim <= 0 ||
            c.attention_downsample_rate <= 0 || c.num_multimask_outputs <= 0 || c.iou_head_hidden_dim <= 0 || c.max_prompts <= 0)
            return "grid, image_size, hidden, layers, heads, mlp_dim, attention_downsample_rate, num_multimask_outputs, "
                   "iou_head_hidden_dim and max_prompts must be positive";
        if (c.hidden != 32 && c.hidden != 64 && c.hidden != 128 && c.hidden != 256)
            return "hidden must be 32, 64, 128 or 256 (the upscaling kernel is built for these; the token kernel's LDS holds 48 hidden floats)";
        if (c.hidden % c.attention_downsample_rate) return "hidden is not a multiple of attention_downsample_rate";
        const int Ci = c.hidden / c.attention_downsample_rate;
        if (c.hidden % c.heads || Ci % c.heads) return "hidden or hidden / attention_downsample_rate is not a multiple of heads";
        const int hd = Ci / c.heads;
        if (hd > 64 || (hd & (hd - 1))) return "cross-attention head width hidden / attention_downsample_rate / heads must be a power of two <= 64";
        if (Ci % 4 || c.mlp_dim % 4 || c.iou_head_hidden_dim % 4) return "hidden / attention_downsample_rate, mlp_dim and iou_head_hidden_dim must be multiples of 4";
        if (c.iou_head_hidden_dim > 8 * c.hidden) return "iou_head_hidden_dim > 8 hidden (the token kernel's LDS rows)";
        if (c.num_multimask_outputs > SD_MAX_NM - 1) return "num_multimask_outputs > 4 (8 tokens per prompt at most)";
        if (c.iou_head_depth < 2 || c.iou_head_depth > 2 + SD_MAX_MID) return "iou_head_depth outside [2, 6]";
        if (c.hidden_act != 0 && c.hidden_act != 1) return "hidden_act must be 0 (relu) or 1 (gelu)";
        if (!(c.layer_norm_eps > 0.f)) return "layer_norm_eps must be positive";
        if (c.grid > 1024) return "grid > 1024";
        if (sd_t2i_lds_floats(hd) * sizeof(float) > 65536) return "head width too large for the token -> image attention kernel's LDS (64 KiB)";
        return "";
    };
    return encoder_create<loco_samdec>("loco_samdec_create", g_samdec_create_err, cfg, device, out, refuse, [&](loco_samdec& t) {
        const loco_samdec_cfg& c = t.cfg = *cfg;
        const long C = c.hidden, Ci = C / c.attention_downsample_rate, F = c.mlp_dim, hid = c.iou_head_hidden_dim, G = c.grid;
        t.G = (int)G; t.T = (int)(G * G); t.Tp = (t.T + 15) / 16 * 16; t.C = (int)C; t.Ci = (int)Ci;
        t.NM = c.num_multimask_outputs + 1; t.NQ = t.NM + 3;
        t.hmax = (int)std::max(std::max(F, hid), C);
        ParamTable& pt = t.table;
        pt.add("shared_image_embedding.positional_embedding", {2, C / 2}, &t.pe);
        pt.add("prompt_encoder.no_mask_embed.weight", {1, C}, &t.no_mask);
        pt.add("prompt_encoder.not_a_point_embed.weight", {1, C}, &t.nap);
        pt.add("prompt_encoder.point_embed.1.weight", {1, C}, &t.point1);
        const std::string M = "mask_decoder.";
        pt.add(M + "iou_token.weight", {1, C}, &t.iou_tok);
        pt.add(M + "mask_tokens.weight", {(long)t.NM, C}, &t.mask_tok);
        auto lin = [&](const std::string& p, long o, long i, float** w, float** b) {
            pt.add(p + ".weight", {o, i}, w);
            pt.add(p + ".bias", {o}, b);
        };
        auto attn = [&](const std::string& p, long inner, SdAttn& a) {
            lin(p + ".q_proj", inner, C, &a.wq, &a.bq);
            lin(p + ".k_proj", inner, C, &a.wk, &a.bk);
            lin(p + ".v_proj", inner, C, &a.wv, &a.bv);
            lin(p + ".out_proj", C, inner, &a.wo, &a.bo);
        };
        t.layer.resize(c.layers);
        for (int l = 0; l < c.layers; ++l) {
            const std::string p = M + "transformer.layers." + std::to_string(l) + ".";
            SdLayer& ly = t.layer[l];
            attn(p + "self_attn", C, ly.self);
            attn(p + "cross_attn_token_to_image", Ci, ly.t2i);
            attn(p + "cross_attn_image_to_token", Ci, ly.i2t);
            for (int j = 0; j < 4; ++j) {
                pt.add(p + "layer_norm" + std::to_string(j + 1) + ".weight", {C}, &ly.ln_g[j]);
                pt.add(p + "layer_norm" + std::to_string(j + 1) + ".bias", {C}, &ly.ln_b[j]);
            }
            lin(p + "mlp.lin1", F, C, &ly.w1, &ly.b1);
            lin(p + "mlp.lin2", C, F, &ly.w2, &ly.b2);
        }
        attn(M + "transformer.final_attn_token_to_image", Ci, t.fin);
        pt.add(M + "transformer.layer_norm_final_attn.weight", {C}, &t.lnf_g);
        pt.add(M + "transformer.layer_norm_final_attn.bias", {C}, &t.lnf_b);
        pt.add(M + "upscale_conv1.weight", {C, C / 4, 2, 2}, &t.up1_w);
        pt.add(M + "upscale_conv1.bias", {C / 4}, &t.up1_b);
        pt.add(M + "upscale_conv2.weight", {C / 4, C / 8, 2, 2}, &t.up2_w);
        pt.add(M + "upscale_conv2.bias", {C / 8}, &t.up2_b);
        pt.add(M + "upscale_layer_norm.weight", {C / 4}, &t.upln_g);
        pt.add(M + "upscale_layer_norm.bias", {C / 4}, &t.upln_b);
        auto mlp3 = [&](const std::string& p, long o, long h, int mid, SdMlp& m) {
            for (int j = 0; j < SD_MAX_MID; ++j) m.w_mid[j] = m.b_mid[j] = nullptr;
            lin(p + ".proj_in", h, C, &m.w_in, &m.b_in);
            for (int j = 0; j < mid; ++j) lin(p + ".layers." + std::to_string(j), h, h, &m.w_mid[j], &m.b_mid[j]);
            lin(p + ".proj_out", o, h, &m.w_out, &m.b_out);
        };
        for (int i = 0; i < t.NM; ++i) mlp3(M + "output_hypernetworks_mlps." + std::to_string(i), C / 8, C, 1, t.hyper[i]);
        mlp3(M + "iou_prediction_head", t.NM, hid, c.iou_head_depth - 2, t.iou);
        const long Tp = t.Tp, MP = c.max_prompts;
        const long npos = 2L * (c.layers - 1) + 1;                  // pos W_k, pos W_q of the layers >= 1 and the final pos W_k
        using B = EncoderBase;
        // zeroed: the padding columns and the token rows >= NQ hold finite values from the first call on
        if (!t.alloc({B::buf(&t.src, C * Tp, true), B::buf(&t.pos, C * Tp, true), B::buf(&t.srcpos, C * Tp, true), B::buf(&t.k0, Ci * Tp, true),
                      B::buf(&t.v0, Ci * Tp, true), B::buf(&t.q0, Ci * Tp, true), B::buf(&t.posw, npos * Ci * Tp, true),
                      B::buf(&t.w2t, C * C / 8, true), B::buf(&t.keys, MP * C * Tp, true), B::buf(&t.proj, MP * std::max(2 * Ci, C) * Tp, true),
                      B::buf(&t.stats, MP * 2 * Tp, true), B::buf(&t.tok, MP * SD_Q * C, true), B::buf(&t.qry, MP * SD_Q * C, true),
                      B::buf(&t.qx, MP * SD_Q * Ci, true), B::buf(&t.ox, MP * SD_Q * Ci, true), B::buf(&t.kx, MP * SD_Q * Ci, true),
                      B::buf(&t.vx, MP * SD_Q * Ci, true), B::buf(&t.hbuf, MP * SD_Q * t.hmax, true), B::buf(&t.hyp, MP * t.NM * (C / 8), true)}))
            return false;
        for (int l = 1; l < c.layers; ++l) {
            t.layer[l].posk = t.posw + (2L * (l - 1)) * Ci * Tp;
            t.layer[l].posq = t.posw + (2L * (l - 1) + 1) * Ci * Tp;
        }
        t.fin_posk = t.posw + (npos - 1) * Ci * Tp;
        return true;
    });
}

int loco_samdec_load_param(loco_samdec* t, const char* name, const float* host, const int64_t* shape, int32_t ndim) {
    if (!t) return -1;
    t->image_set = false;                                  // what set_image derived from the parameters is stale
    return t->table.load(name, host, shape, ndim, t->device, "loco_samdec_load_param", t->err);
}

int loco_samdec_params_missing(loco_samdec* t) { return t ? t->table.missing(t->err) : -1; }

int loco_samdec_set_image(loco_samdec* t, const float* emb_dev, void* stream) {
    if (!t) return -1;
    if (!emb_dev) return t->fail("loco_samdec_set_image: null emb");
    if (t->table.missing(t->err)) return -1;
    DeviceGuard dg(t->device);
    hipStream_t st = (hipStream_t)stream;
    const int C = t->C, Ci = t->Ci, Tp = t->Tp;
    hipLaunchKernelGGL(sd_src_kernel, dim3(blocks256((long)C * Tp)), dim3(256), 0, st, emb_dev, t->no_mask, t->pe, C, t->G, t->T, Tp, t->src,
                       t->pos, t->srcpos);
    hipLaunchKernelGGL(sd_w2t_kernel, dim3(blocks256((long)C * C / 8)), dim3(256), 0, st, t->up2_w, C / 4, C / 8, t->w2t);
    const SdLayer& l0 = t->layer[0];
    launch_gemm_fixed(enc_linear(l0.t2i.wk, l0.t2i.bk, t->srcpos, t->k0, nullptr, Ci, C, Tp), GEMM_ACT_NONE, st);
    launch_gemm_fixed(enc_linear(l0.t2i.wv, l0.t2i.bv, t->src, t->v0, nullptr, Ci, C, Tp), GEMM_ACT_NONE, st);
    launch_gemm_fixed(enc_linear(l0.i2t.wq, l0.i2t.bq, t->srcpos, t->q0, nullptr, Ci, C, Tp), GEMM_ACT_NONE, st);
    for (size_t l = 1; l < t->layer.size(); ++l) {
        launch_gemm_fixed(enc_linear(t->layer[l].t2i.wk, nullptr, t->pos, t->layer[l].posk, nullptr, Ci, C, Tp), GEMM_ACT_NONE, st);
        launch_gemm_fixed(enc_linear(t->layer[l].i2t.wq, nullptr, t->pos, t->layer[l].posq, nullptr, Ci, C, Tp), GEMM_ACT_NONE, st);
    }
    launch_gemm_fixed(enc_linear(t->fin.wk, nullptr, t->pos, t->fin_posk, nullptr, Ci, C, Tp), GEMM_ACT_NONE, st);
    if (hipGetLastError() != hipSuccess) return t->fail("loco_samdec_set_image: kernel launch failed");
    t->image_set = true;
    return 0;
}

int loco_samdec_predict(loco_samdec* t, const float* coords_dev, int32_t P, float* masks_out, float* iou_out, void* stream) {
    if (!t) return -1;
    if (!coords_dev || !masks_out || !iou_out) return t->fail("loco_samdec_predict: null coords, masks or iou");
    if (P < 1 || P > t->cfg.max_prompts)
        return t->fail("loco_samdec_predict: P = " + std::to_string(P) + " outside [1, max_prompts = " + std::to_string(t->cfg.max_prompts) + "]");
    if (t->table.missing(t->err)) return -1;
    if (!t->image_set) return t->fail("loco_samdec_predict: no image set (loco_samdec_set_image comes first, and again after loading parameters)");
    DeviceGuard dg(t->device);
    hipStream_t st = (hipStream_t)stream;
    const loco_samdec_cfg& c = t->cfg;
    const int C = t->C, Ci = t->Ci, Tp = t->Tp, T = t->T, H = c.heads, hd = Ci / H, NQ = t->NQ, L = c.layers;
    const long kst = (long)C * Tp, pst = (long)Ci * Tp;
    const float scale = 1.0f / std::sqrt((float)hd);
    float *pa = t->proj, *pb = t->proj + (long)c.max_prompts * pst;
    SdTok a;
    std::memset(&a, 0, sizeof(a));
    a.C = C; a.Ci = Ci; a.H = H; a.NQ = NQ; a.NM = t->NM; a.mlp = c.mlp_dim; a.act = c.hidden_act == 0 ? 1 : 2;
    a.iou_hid = c.iou_head_hidden_dim; a.iou_mid = c.iou_head_depth - 2; a.hmax = t->hmax; a.eps = c.layer_norm_eps;
    a.coords = coords_dev; a.pe = t->pe; a.point1 = t->point1; a.nap = t->nap; a.iou_tok = t->iou_tok; a.mask_tok = t->mask_tok;
    a.tok = t->tok; a.qry = t->qry; a.qx = t->qx; a.ox = t->ox; a.kx = t->kx; a.vx = t->vx; a.hbuf = t->hbuf; a.hyp = t->hyp; a.iou_out = iou_out;
    for (int i = 0; i < t->NM; ++i) a.hyper[i] = mlp_p(t->hyper[i]);
    a.iou = mlp_p(t->iou);
    const size_t tok_lds = (size_t)6 * SD_Q * C * sizeof(float);
    auto tok = [&](int stage) {
        if (stage == SD_ST_PRE) hipLaunchKernelGGL(sd_tok_kernel<SD_ST_PRE>, dim3(P), dim3(SD_TH), tok_lds, st, a);
        else if (stage == SD_ST_MID) hipLaunchKernelGGL(sd_tok_kernel<SD_ST_MID>, dim3(P), dim3(SD_TH), tok_lds, st, a);
        else if (stage == SD_ST_FINAL_PRE) hipLaunchKernelGGL(sd_tok_kernel<SD_ST_FINAL_PRE>, dim3(P), dim3(SD_TH), tok_lds, st, a);
        else hipLaunchKernelGGL(sd_tok_kernel<SD_ST_FINAL_POST>, dim3(P), dim3(SD_TH), tok_lds, st, a);
    };
    auto t2i = [&](const float* K, const float* V, long kbs) {
        launch_sd_t2i(t->qx, K, V, kbs, (long)Tp, T, Ci, hd, H, P, NQ, scale, t->ox, st);
    };
    for (int l = 0; l < L; ++l) {
        const SdLayer& ly = t->layer[l];
        a.first = l == 0;
        a.self = attn_p(ly.self); a.cross = attn_p(ly.t2i); a.i2t = attn_p(ly.i2t);
        a.ln1_g = ly.ln_g[0]; a.ln1_b = ly.ln_b[0]; a.ln2_g = ly.ln_g[1]; a.ln2_b = ly.ln_b[1]; a.ln3_g = ly.ln_g[2]; a.ln3_b = ly.ln_b[2];
        a.w1 = ly.w1; a.b1 = ly.b1; a.w2 = ly.w2; a.b2 = ly.b2;
        tok(SD_ST_PRE);
        if (l == 0) {
            t2i(t->k0, t->v0, 0);
        } else {
            launch_gemm_fixed(sd_proj(ly.t2i.wk, ly.t2i.bk, t->keys, kst, pa, ly.posk, 0, Ci, C, Tp, P), GEMM_ACT_NONE, st);
            launch_gemm_fixed(sd_proj(ly.t2i.wv, ly.t2i.bv, t->keys, kst, pb, nullptr, 0, Ci, C, Tp, P), GEMM_ACT_NONE, st);
            t2i(pa, pb, pst);
        }
        tok(SD_ST_MID);
        const float* q = t->q0;
        long qbs = 0;
        if (l > 0) {
            launch_gemm_fixed(sd_proj(ly.i2t.wq, ly.i2t.bq, t->keys, kst, pa, ly.posq, 0, Ci, C, Tp, P), GEMM_ACT_NONE, st);
            q = pa;
            qbs = pst;
        }
        launch_sd_i2t(q, qbs, t->kx, t->vx, (long)Tp, T, Tp, Ci, hd, H, P, NQ, scale, pa, st);
        // keys = LayerNorm 4 (keys + out_proj(attention)); layer 0's keys are src for every prompt
        launch_gemm_fixed(sd_proj(ly.i2t.wo, ly.i2t.bo, pa, pst, t->keys, l == 0 ? t->src : t->keys, l == 0 ? 0 : kst, C, Ci, Tp, P),
                          GEMM_ACT_NONE, st);
        launch_ln_fwd(t->keys, kst, P, C, Tp, ly.ln_g[3], ly.ln_b[3], c.layer_norm_eps, t->keys, kst, t->stats, 2L * Tp, st);
    }
    a.cross = attn_p(t->fin);
    a.ln2_g = t->lnf_g; a.ln2_b = t->lnf_b;
    tok(SD_ST_FINAL_PRE);
    launch_gemm_fixed(sd_proj(t->fin.wk, t->fin.bk, t->keys, kst, pa, t->fin_posk, 0, Ci, C, Tp, P), GEMM_ACT_NONE, st);
    launch_gemm_fixed(sd_proj(t->fin.wv, t->fin.bv, t->keys, kst, pb, nullptr, 0, Ci, C, Tp, P), GEMM_ACT_NONE, st);
    t2i(pa, pb, pst);
    tok(SD_ST_FINAL_POST);
    // u1[p][co 4 + ky 2 + kx][t] = sum_ci up1_w[ci][co][ky][kx] keys[p][ci][t]: the operator read as [C][C] with the rows strided
    {
        GemmArgs g = sd_proj(t->up1_w, nullptr, t->keys, kst, t->proj, nullptr, 0, C, C, Tp, P);
        g.sam = 1;
        g.sak = C;
        launch_gemm_fixed(g, GEMM_ACT_NONE, st);
    }
    const dim3 ug((T + SD_TH - 1) / SD_TH, 4, P);
#define SD_UP(N) hipLaunchKernelGGL(sd_up_kernel<N>, ug, dim3(SD_TH), 0, st, t->proj, (long)Tp, T, t->G, t->up1_b, t->upln_g, t->upln_b, t->w2t, \
                                    t->up2_b, t->hyp, t->NM, masks_out)
    if (C == 256) SD_UP(64);
    else if (C == 128) SD_UP(32);
    else if (C == 64) SD_UP(16);
    else SD_UP(8);
#undef SD_UP
    if (hipGetLastError() != hipSuccess) return t->fail("loco_samdec_predict: kernel launch failed");
    return 0;
}

int loco_samdec_score(loco_samdec* t, const float* low_res_dev, int32_t N, int32_t h, int32_t w, int32_t orig_h, int32_t orig_w,
                      int32_t reshaped_h, int32_t reshaped_w, int32_t image_size, float thr, float offset, int32_t* counts_out,
                      int32_t* boxes_out, void* stream) {
    if (!t) return -1;
    if (!low_res_dev || !counts_out || !boxes_out) return t->fail("loco_samdec_score: null low_res, counts or boxes");
    if (const char* why = sd_check_geo(N, h, w, orig_h, orig_w, reshaped_h, reshaped_w, image_size)) return t->fail(std::string("loco_samdec_score: ") + why);
    if (N == 0) return 0;
    DeviceGuard dg(t->device);
    hipLaunchKernelGGL(sd_score_kernel, dim3(N), dim3(SD_TH), 0, (hipStream_t)stream, low_res_dev,
                       sd_geo(h, w, orig_h, orig_w, reshaped_h, reshaped_w, image_size), thr, offset, counts_out, boxes_out);
    if (hipGetLastError() != hipSuccess) return t->fail("loco_samdec_score: kernel launch failed");
    return 0;
}

int loco_samdec_binarize(loco_samdec* t, const float* low_res_dev, int32_t N, const int32_t* rows_dev, int32_t K, int32_t h, int32_t w,
                         int32_t orig_h, int32_t orig_w, int32_t reshaped_h, int32_t reshaped_w, int32_t image_size, float thr,
                         uint8_t* masks_out, void* stream) {
    if (!t) return -1;
    if (K == 0) return 0;
    if (!low_res_dev || !rows_dev || !masks_out) return t->fail("loco_samdec_binarize: null low_res, rows or masks");
    if (const char* why = sd_check_geo(N, h, w, orig_h, orig_w, reshaped_h, reshaped_w, image_size)) return t->fail(std::string("loco_samdec_binarize: ") + why);
    if (K < 0 || K > 65535) return t->fail("loco_samdec_binarize: K outside [0, 65535]");
    DeviceGuard dg(t->device);
    hipLaunchKernelGGL(sd_binarize_kernel, dim3(((long)orig_h * orig_w + SD_TH - 1) / SD_TH, K), dim3(SD_TH), 0, (hipStream_t)stream, low_res_dev, N,
                       rows_dev, sd_geo(h, w, orig_h, orig_w, reshaped_h, reshaped_w, image_size), thr, masks_out);
    if (hipGetLastError() != hipSuccess) return t->fail("loco_samdec_binarize: kernel launch failed");
    return 0;
}

const char* loco_samdec_last_error(loco_samdec* t) { return t ? t->err.c_str() : g_samdec_create_err.c_str(); }

void loco_samdec_destroy(loco_samdec* t) { delete t; }

}  // extern "C"
