// CLIPSeg decoder of the text-prompted edit masks (include/loco_hip.h loco_clipseg_*): the CLIPSegDecoder of transformers on
// the taps of the CLIP image tower (clipvis.hip, loco_clipvis_encode_taps) and one conditional embedding per mask, the image
// preprocessing of ViTImageProcessor in float arithmetic, and the resize + threshold that turns logits into masks.  Exact
// fp32 throughout, fp32 storage.
//
// Layout: that of the other encoders -- the T = 1 + G^2 tokens of all M masks of a call channel-major in ONE [rd][Tp] tensor,
// token column m * T + t, Tp = M * T rounded up to 16; the padding columns are zero-fed and stay independent of the real ones.
// The reduces (once per IMAGE, straight from the token-major taps), the FiLM operator, the packed q | k | v operator,
// out_proj, fc1 (with its ReLU epilogue) and fc2 are launch_gemm_fixed, the LayerNorms xfmr.hip's launch_ln_fwd.  New here:
// the stage combine (reduce of the mask's image + running state, FiLM), an attention kernel for the decoder's narrow heads
// (one wave per query), the heads (every transposed convolution has stride = kernel: an output pixel has ONE source token,
// a gather without atomics), the two resize passes and the mask kernel.  Every kernel computes a mask's columns from the
// columns of that mask alone, in a fixed order: a mask's logits are bit-identical whatever M and its position.
#include "enc_attn_launch.h"

#include <cmath>

struct ClipSegLayer { float *wqkv, *bqkv, *wo, *bo, *ln1_g, *ln1_b, *w1, *b1, *w2, *b2, *ln2_g, *ln2_b; };

struct loco_clipseg : loco::EncoderBase {
    loco_clipseg_cfg cfg;
    int T = 0, Tmax = 0, hd = 0, logit = 0;
    float *film_w = nullptr, *film_b = nullptr;    // [2 rd][P] = film_mul | film_add, [2 rd]
    std::vector<float*> red_w, red_b;
    std::vector<ClipSegLayer> layer;
    float *head_w = nullptr, *head_b = nullptr;                                         // simple head
    float *c0_w = nullptr, *c0_b = nullptr, *c2_w = nullptr, *c2_b = nullptr, *c4_w = nullptr, *c4_b = nullptr;   // complex head
    float *x = nullptr, *y = nullptr, *qkv = nullptr, *attn = nullptr, *f = nullptr, *stats = nullptr, *red = nullptr, *film = nullptr,
          *h1 = nullptr, *h2 = nullptr;
    float* rows = nullptr;                         // the preprocessing's horizontally resized rows, grown on demand
    size_t rows_floats = 0;
    ~loco_clipseg() override {
        loco::DeviceGuard dg(device);
        if (rows) (void)hipFree(rows);
    }
};

namespace loco {
namespace {

constexpr int SEG_MAX_MASKS = 64, SEG_MAX_TOKENS = 2048, SEG_QW = 4;

struct SegMap { int img[SEG_MAX_MASKS]; };     // image of every mask, by value in the kernel arguments

// x[r][m T + t] = red[r][img(m) T + t] (+ x[r][m T + t] unless `first`), then film_mul * x + film_add with `film` [2 rd][M];
// 0 in the padding columns
__global__ __launch_bounds__(256) void seg_combine_kernel(const float* red, long ldr, SegMap map, int R, int T, int MT, int Tp, int M,
                                                          int first, const float* film, float* x) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)R * Tp) return;
    const int r = (int)(e / Tp), col = (int)(e % Tp);
    float v = 0.f;
    if (col < MT) {
        const int m = col / T, t = col % T;
        v = red[(long)r * ldr + (long)map.img[m] * T + t];
        if (!first) v = __fadd_rn(v, x[e]);
        if (film) v = __fadd_rn(__fmul_rn(film[(long)r * M + m], v), film[(long)(R + r) * M + m]);
    }
    x[e] = v;
}

// One wave per query, 4 queries per workgroup, grid (ceil(T / 4), heads, M).  Lane j scores keys j, j + 64, ... against its
// wave's query ((q scale) . k, fp32 FMAs in channel order) into the wave's LDS row; max and sum over the row by shuffles; then
// lane (part, c) sums p v over the keys part, part + 64 / HD, ... of channel c and the parts are added by shuffles, all in a
// fixed order.  qkv: [3 rd][ld] = q | k | v channel rows, out [rd][ld].
template <int HD>
__global__ __launch_bounds__(256) void seg_attn_kernel(const float* qkv, long ld, int R, int T, float scale, float* out) {
    extern __shared__ __align__(16) float seg_sm[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int q = blockIdx.x * SEG_QW + wv, h = blockIdx.y, m = blockIdx.z;
    const int ql = min(q, T - 1);
    const long col0 = (long)m * T;
    float* pw = seg_sm + (long)wv * T;
    const float* qp = qkv + (long)(h * HD) * ld + col0;
    const float* kp = qkv + (long)(R + h * HD) * ld + col0;
    const float* vp = qkv + (long)(2 * R + h * HD) * ld + col0;
    float qv[HD];
#pragma unroll
    for (int c = 0; c < HD; ++c) qv[c] = qp[(long)c * ld + ql] * scale;
    float mx = -INFINITY;
    for (int j = lane; j < T; j += 64) {
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < HD; ++c) s = fmaf(qv[c], kp[(long)c * ld + j], s);
        pw[j] = s;
        mx = fmaxf(mx, s);
    }
    mx = wave_max(mx);                     // T >= 2: lane 0 always holds a key
    float sum = 0.f;
    for (int j = lane; j < T; j += 64) {
        const float p = expf(pw[j] - mx);
        pw[j] = p;
        sum += p;
    }
    sum = wave_sum(sum);
    __syncthreads();
    constexpr int PARTS = 64 / HD;
    const int c = lane % HD, part = lane / HD;
    float acc = 0.f;
    for (int j = part; j < T; j += PARTS) acc = fmaf(pw[j], vp[(long)c * ld + j], acc);
#pragma unroll
    for (int o = 32; o >= HD; o >>= 1) acc += __shfl_xor(acc, o);
    if (q < T && lane < HD) out[(long)(h * HD + c) * ld + col0 + q] = acc / sum;
}

// simple head: logits[m][ty ps + ky][tx ps + kx] = b + sum_r x[r][m T + 1 + ty G + tx] W[r][0][ky][kx]
__global__ __launch_bounds__(256) void seg_head_simple_kernel(const float* x, int Tp, int R, int G, int ps, int T, int M, const float* W,
                                                              const float* b, float* logits) {
    const int s = G * ps;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)M * s * s) return;
    const int X = (int)(e % s), Y = (int)((e / s) % s), m = (int)(e / ((long)s * s));
    const long col = (long)m * T + 1 + (Y / ps) * G + X / ps;
    const int k = (Y % ps) * ps + X % ps;
    float acc = b[0];
    for (int r = 0; r < R; ++r) acc = fmaf(x[(long)r * Tp + col], W[(long)r * ps * ps + k], acc);
    logits[e] = acc;
}

// complex head, first layer: c1[m][co][y][x] = relu(b[co] + sum_ci sum_ky sum_kx W[co][ci][ky][kx] x[ci][m T + 1 + (y + ky - 1) G + x + kx - 1])
__global__ __launch_bounds__(256) void seg_conv3_kernel(const float* x, int Tp, int R, int G, int T, int M, const float* W, const float* b,
                                                        float* c1) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)M * R * G * G) return;
    const int px = (int)(e % G), py = (int)((e / G) % G), co = (int)((e / ((long)G * G)) % R), m = (int)(e / ((long)G * G * R));
    const long col0 = (long)m * T + 1;
    float acc = b[co];
    for (int ci = 0; ci < R; ++ci) {
        const float* w = W + ((long)co * R + ci) * 9;
        const float* xr = x + (long)ci * Tp + col0;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int yy = py + ky - 1;
            if (yy < 0 || yy >= G) continue;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int xx = px + kx - 1;
                if (xx < 0 || xx >= G) continue;
                acc = fmaf(w[ky * 3 + kx], xr[yy * G + xx], acc);
            }
        }
    }
    c1[e] = fmaxf(acc, 0.f);
}

// a transposed convolution with stride = kernel k: out[m][co][y k + ky][x k + kx] = act(b[co] + sum_ci in[m][ci][y][x] W[ci][co][ky][kx])
__global__ __launch_bounds__(256) void seg_tconv_kernel(const float* in, int Cin, int Cout, int side, int k, int M, const float* W,
                                                        const float* b, int relu, float* out) {
    const int so = side * k;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)M * Cout * so * so) return;
    const int X = (int)(e % so), Y = (int)((e / so) % so), co = (int)((e / ((long)so * so)) % Cout), m = (int)(e / ((long)so * so * Cout));
    const float* src = in + (long)m * Cin * side * side + (long)(Y / k) * side + X / k;
    const float* w = W + ((long)co * k + Y % k) * k + X % k;
    float acc = b[co];
    for (int ci = 0; ci < Cin; ++ci) acc = fmaf(src[(long)ci * side * side], w[(long)ci * Cout * k * k], acc);
    out[e] = relu ? fmaxf(acc, 0.f) : acc;
}

// ---- preprocessing: the antialiased resize of PIL / torch as two passes, each axis on its own; the tap rule of clipvis.hip
// with a second filter
__device__ __forceinline__ double sg_filter(double x, int resample) {
    x = fabs(x);
    if (resample == 2) return x < 1.0 ? 1.0 - x : 0.0;
    if (x < 1.0) return ((1.5 * x - 2.5) * x) * x + 1.0;
    if (x < 2.0) return (((x - 5.0) * x + 8.0) * x - 4.0) * -0.5;
    return 0.0;
}
struct SgTaps { int lo, cnt; double center, inv, total; };
__device__ __forceinline__ SgTaps sg_taps(int o, int in, int out, int resample) {
    SgTaps t;
    const double scale = (double)in / (double)out;
    const double support = (resample == 2 ? 1.0 : 2.0) * fmax(scale, 1.0);
    t.inv = 1.0 / fmax(scale, 1.0);
    t.center = ((double)o + 0.5) * scale;
    t.lo = max((int)(t.center - support + 0.5), 0);
    t.cnt = min((int)(t.center + support + 0.5), in) - t.lo;
    t.total = 0.0;
    for (int j = 0; j < t.cnt; ++j) t.total += sg_filter(((double)(t.lo + j) - t.center + 0.5) * t.inv, resample);
    return t;
}
__device__ __forceinline__ float sg_weight(const SgTaps& t, int j, int resample) {
    return (float)(sg_filter(((double)(t.lo + j) - t.center + 0.5) * t.inv, resample) / t.total);
}

// rows[i][c][y][x] = sum_j w_j frame[i][c][y][lo + j]: U8 frames [n][H][W][3] in grey levels, else fp32 [n][3][H][W]
template <bool U8>
__global__ __launch_bounds__(256) void seg_resize_x_kernel(const void* frames, int n, int H, int W, int S, int resample, float* rows) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)n * 3 * H * S) return;
    const int x = (int)(e % S), y = (int)((e / S) % H), c = (int)((e / ((long)S * H)) % 3), i = (int)(e / ((long)S * H * 3));
    const SgTaps t = sg_taps(x, W, S, resample);
    float acc = 0.f;
    if (U8) {
        const unsigned char* src = (const unsigned char*)frames + (((long)i * H + y) * W) * 3 + c;
        for (int j = 0; j < t.cnt; ++j) acc = fmaf(sg_weight(t, j, resample), (float)src[(long)(t.lo + j) * 3], acc);
    } else {
        const float* src = (const float*)frames + (((long)i * 3 + c) * H + y) * W;
        for (int j = 0; j < t.cnt; ++j) acc = fmaf(sg_weight(t, j, resample), src[t.lo + j], acc);
    }
    rows[e] = acc;
}

// out[i][c][y][x] = (unit(sum_j w_j rows[i][c][lo + j][x]) - mean_c) / std_c, unit(v) = v / 255 (U8) or v / 2 + 1 / 2
template <bool U8>
__global__ __launch_bounds__(256) void seg_resize_y_kernel(const float* rows, int n, int H, int S, int resample, float m0, float m1, float m2,
                                                           float s0, float s1, float s2, float* out) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)n * 3 * S * S) return;
    const int x = (int)(e % S), y = (int)((e / S) % S), c = (int)((e / ((long)S * S)) % 3), i = (int)(e / ((long)S * S * 3));
    const float* src = rows + ((long)i * 3 + c) * H * S + x;
    const SgTaps t = sg_taps(y, H, S, resample);
    float acc = 0.f;
    for (int j = 0; j < t.cnt; ++j) acc = fmaf(sg_weight(t, j, resample), src[(long)(t.lo + j) * S], acc);
    const float mean = c == 0 ? m0 : c == 1 ? m1 : m2, sd = c == 0 ? s0 : c == 1 ? s1 : s2;
    const float v = U8 ? acc / 255.0f : acc * 0.5f + 0.5f;
    out[e] = (v - mean) / sd;
}

// ---- masks: workgroup m owns mask m.  Bilinear resize (align_corners = False: source (o + 1 / 2) s / res - 1 / 2, clamped at
// 0; no antialias) in double, > thr; the set pixels are counted per thread, then per wave by shuffles, then in wave order.
__global__ __launch_bounds__(256) void seg_masks_kernel(const float* logits, int s, int res, double thr, unsigned char* mask, int* area) {
    __shared__ int part[4];
    const int m = blockIdx.x;
    const float* src = logits + (long)m * s * s;
    unsigned char* dst = mask + (long)m * res * res;
    const double scale = (double)s / (double)res;
    int cnt = 0;
    for (int p = threadIdx.x; p < res * res; p += 256) {
        const int Y = p / res, X = p % res;
        const double sy = fmax(((double)Y + 0.5) * scale - 0.5, 0.0), sx = fmax(((double)X + 0.5) * scale - 0.5, 0.0);
        const int y0 = min((int)sy, s - 1), x0 = min((int)sx, s - 1), y1 = min(y0 + 1, s - 1), x1 = min(x0 + 1, s - 1);
        const double ly = sy - (double)y0, lx = sx - (double)x0;
        const double top = (1.0 - lx) * (double)src[(long)y0 * s + x0] + lx * (double)src[(long)y0 * s + x1];
        const double bot = (1.0 - lx) * (double)src[(long)y1 * s + x0] + lx * (double)src[(long)y1 * s + x1];
        const int bit = (1.0 - ly) * top + ly * bot > thr ? 1 : 0;
        dst[p] = (unsigned char)bit;
        cnt += bit;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) cnt += __shfl_xor(cnt, o);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) area[m] = part[0] + part[1] + part[2] + part[3];
}

template <int HD>
void seg_attn_launch(dim3 grid, size_t lds, hipStream_t st, const float* qkv, long ld, int R, int T, float scale, float* out) {
    hipLaunchKernelGGL(seg_attn_kernel<HD>, grid, dim3(256), lds, st, qkv, ld, R, T, scale, out);
}

}  // namespace

void launch_seg_attn(const float* qkv, long ld, int R, int hd, int heads, int T, int M, float scale, float* out, hipStream_t st) {
    const dim3 grid((T + SEG_QW - 1) / SEG_QW, heads, M);
    const size_t lds = (size_t)SEG_QW * T * sizeof(float);
    switch (seg_attn_instance(hd)) {
        case 4: seg_attn_launch<4>(grid, lds, st, qkv, ld, R, T, scale, out); break;
        case 8: seg_attn_launch<8>(grid, lds, st, qkv, ld, R, T, scale, out); break;
        case 16: seg_attn_launch<16>(grid, lds, st, qkv, ld, R, T, scale, out); break;
        case 32: seg_attn_launch<32>(grid, lds, st, qkv, ld, R, T, scale, out); break;
        default: seg_attn_launch<64>(grid, lds, st, qkv, ld, R, T, scale, out); break;
    }
}

}  // namespace loco

using namespace loco;

namespace {
thread_local std::string g_clipseg_create_err;
}

extern "C" {

int loco_clipseg_create(const loco_clipseg_cfg* cfg, int32_t device, loco_clipseg** out) {
    auto refuse = [&](const loco_clipseg_cfg& c) -> std::string {
        if (c.width <= 0 || c.grid <= 0 || c.patch_size <= 0 || c.reduce_dim <= 0 || c.heads <= 0 || c.ffn <= 0 || c.n_taps <= 0 ||
            c.projection_dim <= 0 || c.max_masks <= 0)
            return "width, grid, patch_size, reduce_dim, heads, ffn, n_taps, projection_dim and max_masks must be positive";
        if (c.conditional_layer < 0 || c.conditional_layer >= c.n_taps)
            return "conditional_layer " + std::to_string(c.conditional_layer) + " outside [0, n_taps = " + std::to_string(c.n_taps) + ")";
        if (c.reduce_dim % c.heads) return "reduce_dim is not a multiple of heads";
        const int hd = c.reduce_dim / c.heads;
        if (hd != 4 && hd != 8 && hd != 16 && hd != 32 && hd != 64)
            return "head width " + std::to_string(hd) + ": the attention kernel is built for 4, 8, 16, 32 and 64";
        if (1 + (long)c.grid * c.grid > SEG_MAX_TOKENS)
            return "1 + grid^2 > " + std::to_string(SEG_MAX_TOKENS) + " tokens (the attention kernel keeps a row of scores per query in LDS)";
        if (c.max_masks > SEG_MAX_MASKS) return "max_masks > " + std::to_string(SEG_MAX_MASKS);
        if (c.complex_head && (c.patch_size % 4 || c.reduce_dim % 2))
            return "the complex head needs patch_size a multiple of 4 and an even reduce_dim";
        if (!(c.ln_eps > 0.f)) return "ln_eps must be positive";
        const long k = c.patch_size / 4, side = c.complex_head ? (long)c.grid * k * k : (long)c.grid * c.patch_size;
        if (side * side * c.max_masks * std::max(1, c.reduce_dim / 2) > (1L << 31)) return "max_masks x logits > 2^31";
        return "";
    };
    return encoder_create<loco_clipseg>("loco_clipseg_create", g_clipseg_create_err, cfg, device, out, refuse, [&](loco_clipseg& t) {
        const loco_clipseg_cfg& c = t.cfg = *cfg;
        t.T = 1 + c.grid * c.grid; t.hd = c.reduce_dim / c.heads;
        t.Tmax = (c.max_masks * t.T + 15) / 16 * 16;
        const long D = c.width, R = c.reduce_dim, F = c.ffn, P = c.projection_dim, ps = c.patch_size, G = c.grid, k = ps / 4, Tm = t.Tmax,
                   Mm = c.max_masks;
        t.logit = (int)(c.complex_head ? G * k * k : G * ps);
        ParamTable& pt = t.table;
        const size_t fw = pt.reserve((size_t)2 * R * P, &t.film_w), fb = pt.reserve(round64(2 * R), &t.film_b);
        const char* filmn[2] = {"film_mul", "film_add"};
        for (int j = 0; j < 2; ++j) {
            pt.view(std::string(filmn[j]) + ".weight", {R, P}, fw + (size_t)j * R * P);
            pt.view(std::string(filmn[j]) + ".bias", {R}, fb + (size_t)j * R);
        }
        t.red_w.resize(c.n_taps); t.red_b.resize(c.n_taps); t.layer.resize(c.n_taps);
        for (int i = 0; i < c.n_taps; ++i) {
            pt.add("reduces." + std::to_string(i) + ".weight", {R, D}, &t.red_w[i]);
            pt.add("reduces." + std::to_string(i) + ".bias", {R}, &t.red_b[i]);
            const std::string p = "layers." + std::to_string(i) + ".";
            ClipSegLayer& ly = t.layer[i];
            const size_t wq = pt.reserve((size_t)3 * R * R, &ly.wqkv), bq = pt.reserve(round64(3 * R), &ly.bqkv);
            const char* qkvn[3] = {"q_proj", "k_proj", "v_proj"};
            for (int j = 0; j < 3; ++j) {
                pt.view(p + "self_attn." + qkvn[j] + ".weight", {R, R}, wq + (size_t)j * R * R);
                pt.view(p + "self_attn." + qkvn[j] + ".bias", {R}, bq + (size_t)j * R);
            }
            pt.add(p + "self_attn.out_proj.weight", {R, R}, &ly.wo);
            pt.add(p + "self_attn.out_proj.bias", {R}, &ly.bo);
            pt.add(p + "layer_norm1.weight", {R}, &ly.ln1_g);
            pt.add(p + "layer_norm1.bias", {R}, &ly.ln1_b);
            pt.add(p + "mlp.fc1.weight", {F, R}, &ly.w1);
            pt.add(p + "mlp.fc1.bias", {F}, &ly.b1);
            pt.add(p + "mlp.fc2.weight", {R, F}, &ly.w2);
            pt.add(p + "mlp.fc2.bias", {R}, &ly.b2);
            pt.add(p + "layer_norm2.weight", {R}, &ly.ln2_g);
            pt.add(p + "layer_norm2.bias", {R}, &ly.ln2_b);
        }
        size_t h1 = 16, h2 = 16;
        if (c.complex_head) {
            pt.add("transposed_convolution.0.weight", {R, R, 3, 3}, &t.c0_w);
            pt.add("transposed_convolution.0.bias", {R}, &t.c0_b);
            pt.add("transposed_convolution.2.weight", {R, R / 2, k, k}, &t.c2_w);
            pt.add("transposed_convolution.2.bias", {R / 2}, &t.c2_b);
            pt.add("transposed_convolution.4.weight", {R / 2, 1, k, k}, &t.c4_w);
            pt.add("transposed_convolution.4.bias", {1}, &t.c4_b);
            h1 = (size_t)(Mm * R * G * G);
            h2 = (size_t)(Mm * (R / 2) * G * k * G * k);
        } else {
            pt.add("transposed_convolution.weight", {R, 1, ps, ps}, &t.head_w);
            pt.add("transposed_convolution.bias", {1}, &t.head_b);
        }
        using B = EncoderBase;
        // attn zeroed: the attention writes only the real token columns, the padding columns of its output stay finite
        return t.alloc({B::buf(&t.x, R * Tm), B::buf(&t.y, R * Tm), B::buf(&t.qkv, 3 * R * Tm), B::buf(&t.attn, R * Tm, true),
                        B::buf(&t.f, F * Tm), B::buf(&t.stats, 2 * Tm), B::buf(&t.red, R * Mm * t.T), B::buf(&t.film, 2 * R * Mm),
                        B::buf(&t.h1, h1), B::buf(&t.h2, h2)});
    });
}

int loco_clipseg_load_param(loco_clipseg* t, const char* name, const float* host, const int64_t* shape, int32_t ndim) {
    return t ? t->table.load(name, host, shape, ndim, t->device, "loco_clipseg_load_param", t->err) : -1;
}

int loco_clipseg_params_missing(loco_clipseg* t) { return t ? t->table.missing(t->err) : -1; }

int32_t loco_clipseg_logit_size(loco_clipseg* t) { return t ? t->logit : -1; }

int loco_clipseg_decode(loco_clipseg* t, const float* taps_dev, int32_t n_images, const float* cond_dev, const int32_t* image_of_mask,
                        int32_t M, float* logits_dev, void* stream) {
    if (!t) return -1;
    if (!taps_dev || !cond_dev || !image_of_mask || !logits_dev) return t->fail("loco_clipseg_decode: null taps, cond, image_of_mask or logits");
    const loco_clipseg_cfg& c = t->cfg;
    if (M <= 0 || M > c.max_masks)
        return t->fail("loco_clipseg_decode: M = " + std::to_string(M) + " outside [1, max_masks = " + std::to_string(c.max_masks) + "]");
    if (n_images <= 0 || n_images > c.max_masks)
        return t->fail("loco_clipseg_decode: n_images = " + std::to_string(n_images) + " outside [1, max_masks = " + std::to_string(c.max_masks) + "]");
    SegMap map;
    for (int m = 0; m < M; ++m) {
        if (image_of_mask[m] < 0 || image_of_mask[m] >= n_images)
            return t->fail("loco_clipseg_decode: image_of_mask[" + std::to_string(m) + "] = " + std::to_string(image_of_mask[m]) +
                           " outside [0, n_images = " + std::to_string(n_images) + ")");
        map.img[m] = image_of_mask[m];
    }
    for (int m = M; m < SEG_MAX_MASKS; ++m) map.img[m] = 0;
    if (t->table.missing(t->err)) return -1;
    DeviceGuard dg(t->device);
    hipStream_t st = (hipStream_t)stream;
    const int D = c.width, R = c.reduce_dim, F = c.ffn, P = c.projection_dim, G = c.grid, ps = c.patch_size, T = t->T, hd = t->hd;
    const int MT = M * T, Tp = (MT + 15) / 16 * 16, nT = n_images * T;
    const float scale = 1.0f / std::sqrt((float)hd);
    // film [2 rd][M] = (film_mul | film_add) cond^T + bias
    {
        GemmArgs g = enc_linear(t->film_w, t->film_b, cond_dev, t->film, nullptr, 2 * R, P, M);
        g.sbk = 1; g.sbn = P;
        launch_gemm_fixed(g, GEMM_ACT_NONE, st);
    }
    for (int i = 0; i < c.n_taps; ++i) {
        const ClipSegLayer& ly = t->layer[i];
        // red [rd][n T] = reduces[i] on the token-major tap of every image, deepest tap first
        GemmArgs g = enc_linear(t->red_w[i], t->red_b[i], taps_dev + (size_t)(c.n_taps - 1 - i) * nT * D, t->red, nullptr, R, D, nT);
        g.sbk = 1; g.sbn = D;
        launch_gemm_fixed(g, GEMM_ACT_NONE, st);
        hipLaunchKernelGGL(seg_combine_kernel, dim3(blocks256((long)R * Tp)), dim3(256), 0, st, t->red, (long)nT, map, R, T, MT, Tp, M,
                           i == 0 ? 1 : 0, i == c.conditional_layer ? t->film : (const float*)nullptr, t->x);
        launch_gemm_fixed(enc_linear(ly.wqkv, ly.bqkv, t->x, t->qkv, nullptr, 3 * R, R, Tp), GEMM_ACT_NONE, st);
        launch_seg_attn(t->qkv, (long)Tp, R, hd, c.heads, T, M, scale, t->attn, st);
        launch_gemm_fixed(enc_linear(ly.wo, ly.bo, t->attn, t->y, t->x, R, R, Tp), GEMM_ACT_NONE, st);
        launch_ln_fwd(t->y, 0, 1, R, Tp, ly.ln1_g, ly.ln1_b, c.ln_eps, t->x, 0, t->stats, 0, st);
        launch_gemm_fixed(enc_linear(ly.w1, ly.b1, t->x, t->f, nullptr, F, R, Tp), GEMM_ACT_RELU, st);
        launch_gemm_fixed(enc_linear(ly.w2, ly.b2, t->f, t->y, t->x, R, F, Tp), GEMM_ACT_NONE, st);
        launch_ln_fwd(t->y, 0, 1, R, Tp, ly.ln2_g, ly.ln2_b, c.ln_eps, t->x, 0, t->stats, 0, st);
    }
    if (c.complex_head) {
        const int k = ps / 4, s1 = G * k;
        hipLaunchKernelGGL(seg_conv3_kernel, dim3(blocks256((long)M * R * G * G)), dim3(256), 0, st, t->x, Tp, R, G, T, M, t->c0_w, t->c0_b,
                           t->h1);
        hipLaunchKernelGGL(seg_tconv_kernel, dim3(blocks256((long)M * (R / 2) * s1 * s1)), dim3(256), 0, st, t->h1, R, R / 2, G, k, M,
                           t->c2_w, t->c2_b, 1, t->h2);
        hipLaunchKernelGGL(seg_tconv_kernel, dim3(blocks256((long)M * t->logit * t->logit)), dim3(256), 0, st, t->h2, R / 2, 1, s1, k, M,
                           t->c4_w, t->c4_b, 0, logits_dev);
    } else {
        hipLaunchKernelGGL(seg_head_simple_kernel, dim3(blocks256((long)M * t->logit * t->logit)), dim3(256), 0, st, t->x, Tp, R, G, ps, T, M,
                           t->head_w, t->head_b, logits_dev);
    }
    if (hipGetLastError() != hipSuccess) return t->fail("loco_clipseg_decode: kernel launch failed");
    return 0;
}

int loco_clipseg_preprocess(loco_clipseg* t, const void* frames_dev, int32_t is_u8, int32_t n, int32_t H, int32_t W, int32_t S,
                            int32_t resample, const float* mean, const float* sd, float* out_dev, void* stream) {
    if (!t) return -1;
    if (!frames_dev || !out_dev || !mean || !sd) return t->fail("loco_clipseg_preprocess: null frames, mean, std or out");
    if (n <= 0 || H <= 0 || W <= 0 || S <= 0) return t->fail("loco_clipseg_preprocess: n, H, W and S must be positive");
    if (resample != 2 && resample != 3)
        return t->fail("loco_clipseg_preprocess: resample " + std::to_string(resample) + ": 2 (bilinear) and 3 (bicubic) are built");
    if ((long)n * 3 * std::max(H, S) * std::max((long)W, (long)S) > (1L << 31))
        return t->fail("loco_clipseg_preprocess: n x 3 x H x W > 2^31 (split the batch)");
    DeviceGuard dg(t->device);
    hipStream_t st = (hipStream_t)stream;
    const size_t need = (size_t)n * 3 * H * S;
    if (!EncoderBase::grow(&t->rows, &t->rows_floats, need)) return t->fail("loco_clipseg_preprocess: hipMalloc failed");
    const dim3 gx(blocks256((long)need)), gy(blocks256((long)n * 3 * S * S));
    if (is_u8) {
        hipLaunchKernelGGL(seg_resize_x_kernel<true>, gx, dim3(256), 0, st, frames_dev, n, H, W, S, resample, t->rows);
        hipLaunchKernelGGL(seg_resize_y_kernel<true>, gy, dim3(256), 0, st, t->rows, n, H, S, resample, mean[0], mean[1], mean[2], sd[0], sd[1],
                           sd[2], out_dev);
    } else {
        hipLaunchKernelGGL(seg_resize_x_kernel<false>, gx, dim3(256), 0, st, frames_dev, n, H, W, S, resample, t->rows);
        hipLaunchKernelGGL(seg_resize_y_kernel<false>, gy, dim3(256), 0, st, t->rows, n, H, S, resample, mean[0], mean[1], mean[2], sd[0], sd[1],
                           sd[2], out_dev);
    }
    if (hipGetLastError() != hipSuccess) return t->fail("loco_clipseg_preprocess: kernel launch failed");
    return 0;
}

int loco_clipseg_masks(loco_clipseg* t, const float* logits_dev, int32_t M, int32_t s, int32_t res, double threshold_logit,
                       uint8_t* mask_dev, int32_t* area_dev, void* stream) {
    if (!t) return -1;
    if (!logits_dev || !mask_dev || !area_dev) return t->fail("loco_clipseg_masks: null logits, mask or area");
    if (M <= 0 || s <= 0 || res <= 0) return t->fail("loco_clipseg_masks: M, s and res must be positive");
    if (M > 65535 || (long)res * res > (1L << 30) || (long)s * s > (1L << 30)) return t->fail("loco_clipseg_masks: M > 65535 or a side above 2^15");
    if (!(threshold_logit == threshold_logit)) return t->fail("loco_clipseg_masks: the threshold is not a number");
    DeviceGuard dg(t->device);
    hipLaunchKernelGGL(seg_masks_kernel, dim3(M), dim3(256), 0, (hipStream_t)stream, logits_dev, s, res, threshold_logit, mask_dev, area_dev);
    if (hipGetLastError() != hipSuccess) return t->fail("loco_clipseg_masks: kernel launch failed");
    return 0;
}

const char* loco_clipseg_last_error(loco_clipseg* t) { return t ? t->err.c_str() : g_clipseg_create_err.c_str(); }

void loco_clipseg_destroy(loco_clipseg* t) { delete t; }

}  // extern "C"
