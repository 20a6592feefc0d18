// Edit-quality scores of decoded frames (include/loco_hip.h loco_quality_*): LPIPS (AlexNet), SSIM and mask-restricted MSE,
// the three metrics of eval.py on the device.  Independent of loco_set_precision / LOCO_PRECISION, sums in a fixed order, no
// atomics, no host synchronisation inside a call.
//
// LPIPS: the 2 n images of a call (a[0..n), then b[0..n)) go through the five AlexNet convolutions as implicit GEMMs on the
// exact-fp32 matrix instruction (v_mfma_f32_32x32x2_f32): per image D[Cout][Ho Wo] = W[Cout][K] X[K][Ho Wo], K = Cin kh kw.  A
// block owns a 64 x 64 tile of ONE image's D (four waves, one 32 x 32 accumulator each) and walks K in chunks of 32: the
// weight tile and the image tile -- the im2col columns of its 64 output positions, gathered from the feature map with the
// zero padding, for the first layer with the input scaling -- are staged in LDS, never in HBM.  Every 8 values of k (four
// instructions) are summed in a fresh accumulator -- one k-ordered fp32 fma chain of 8 terms, what the instruction computes --
// and that partial sum is added to a running total kept in double: the rounding error of a feature is that of the short
// chains only and does not grow with the running sum (K reaches 3456; the perceptual distance of a one-grey-level edit is a
// difference of nearly equal features, so feature error is what limits it).  Bias, one rounding to fp32 and ReLU in the epilogue.
// The max-pools are a kernel of their own.  After each convolution one block per pair normalises both feature maps over the
// channels, applies the 1x1 head to the squared difference and averages over the positions, from the fp32 features in
// double, each thread its positions in order and then a fixed tree over the block.
//
// SSIM: a block owns a 16 x 16 tile of one plane's map, stages the 26 x 26 reflect-padded patches of both images in LDS and
// sums the five window moments of its pixel in double (121 products each, the window w[ky] w[kx] from the 11 float64 weights
// the host passes in); the tile's sum goes to the workspace, a second kernel sums an image's tiles in order.
//
// Masked MSE: one block per image, each thread its elements in order in double, then a fixed tree.
//
// Every block reads the data of one image (or one pair) only and its place in the grid does not enter the arithmetic: a
// pair's results are bit-identical whatever n and wherever the pair sits in the batch.
#include "encoder_common.h"

#include <cmath>

struct QualityLayer { float *w, *b, *lin; };

struct loco_quality : loco::EncoderBase {
    loco_quality_cfg cfg;
    int max_pairs = 0;
    QualityLayer layer[5];
    float *feat0 = nullptr, *feat1 = nullptr, *pool = nullptr;
    double *taps = nullptr, *ssim_part = nullptr;
    long ssim_part_cap = 0;
};

namespace loco {
namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

// AlexNet feature stack: out channels, in channels, kernel, stride, padding, 3x3 stride-2 max-pool before
struct AlexLayer { int cout, cin, ks, stride, pad, pool; };
constexpr AlexLayer ALEX[5] = {{64, 3, 11, 4, 2, 0}, {192, 64, 5, 1, 2, 1}, {384, 192, 3, 1, 1, 1}, {256, 384, 3, 1, 1, 0},
                               {256, 256, 3, 1, 1, 0}};
constexpr int ALEX_INDEX[5] = {0, 3, 6, 8, 10};          // index of the convolution in torchvision's `features`

struct AlexGeom { int h[5], w[5], ph[2], pw[2]; };       // map of each convolution's output, of each pool's output
inline AlexGeom alex_geom(int H, int W) {
    AlexGeom g{};
    int h = H, w = W, np = 0;
    for (int l = 0; l < 5; ++l) {
        const AlexLayer& a = ALEX[l];
        if (a.pool) {
            h = h >= 3 ? (h - 3) / 2 + 1 : 0; w = w >= 3 ? (w - 3) / 2 + 1 : 0;
            g.ph[np] = h; g.pw[np] = w; ++np;
        }
        h = h > 0 && h + 2 * a.pad >= a.ks ? (h + 2 * a.pad - a.ks) / a.stride + 1 : 0;
        w = w > 0 && w + 2 * a.pad >= a.ks ? (w + 2 * a.pad - a.ks) / a.stride + 1 : 0;
        g.h[l] = h; g.w[l] = w;
    }
    return g;
}

constexpr int QC_LDA = 33;          // the weight tile's row stride in LDS: 32 k + 1, the 32 rows a wave reads fall on 32 banks

// out[img][co][oy][ox] = relu(bias[co] + sum_k w[co][k] x[img][k -> (ci, ky, kx)] at (oy STRIDE - PAD + ky, ox STRIDE - PAD + kx)).
// grid (ceil(Ho Wo / 64), Cout / 64, images); FIRST: x = ((normalize ? 2 v - 1 : v) - shift[ci]) / scale[ci] of the frames
// in (images below n_pairs) and in_b (the others)
template <int KS, int STRIDE, int PAD, bool FIRST>
__global__ __launch_bounds__(256) void quality_conv_kernel(const float* in, const float* in_b, int n_pairs, int Cin, int Hin, int Win,
                                                           int Ho, int Wo, const float* w, const float* bias, int Cout, int normalize,
                                                           float* out) {
    __shared__ float As[64 * QC_LDA];
    __shared__ float Bs[32 * 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const int P = Ho * Wo, K = Cin * KS * KS;
    const int p0 = blockIdx.x * 64, co0 = blockIdx.y * 64, img = blockIdx.z;
    const long plane = (long)Hin * Win;
    const float* src = FIRST && img >= n_pairs ? in_b + (long)(img - n_pairs) * Cin * plane : in + (long)img * Cin * plane;
    // the column of the image tile this thread gathers
    const int j = tid & 63, pos = p0 + j;
    const bool live = pos < P;
    const int oy = live ? pos / Wo : 0, ox = live ? pos % Wo : 0;
    const int iy0 = oy * STRIDE - PAD, ix0 = ox * STRIDE - PAD;
    double total[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) total[r] = 0.0;
    for (int k0 = 0; k0 < K; k0 += 32) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int e = tid + 256 * i, row = e >> 5, kk = e & 31, k = k0 + kk;
            As[row * QC_LDA + kk] = k < K ? w[(long)(co0 + row) * K + k] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int kk = (tid >> 6) + 4 * i, k = k0 + kk;
            float v = 0.f;
            if (live && k < K) {
                const int ci = k / (KS * KS), r = k % (KS * KS), iy = iy0 + r / KS, ix = ix0 + r % KS;
                if (iy >= 0 && iy < Hin && ix >= 0 && ix < Win) {
                    v = src[ci * plane + (long)iy * Win + ix];
                    if (FIRST) {
                        if (normalize) v = 2.f * v - 1.f;
                        const float shift = ci == 0 ? -0.030f : ci == 1 ? -0.088f : -0.188f;
                        const float scale = ci == 0 ? 0.458f : ci == 1 ? 0.448f : 0.450f;
                        v = (v - shift) / scale;
                    }
                }
            }
            Bs[kk * 64 + j] = v;
        }
        __syncthreads();
        const float* ap = As + (wm * 32 + (lane & 31)) * QC_LDA + (lane >> 5);
        const float* bp = Bs + (lane >> 5) * 64 + wn * 32 + (lane & 31);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
            for (int s = 4 * q; s < 4 * q + 4; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[2 * s], bp[2 * s * 64], acc, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 16; ++r) total[r] += (double)acc[r];
        }
        __syncthreads();
    }
    // accumulator element r of lane l: row (r & 3) + 8 (r >> 2) + 4 (l >> 5), column l & 31
    const int opos = p0 + wn * 32 + (lane & 31);
    if (opos < P) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int co = co0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            out[((long)img * Cout + co) * P + opos] = fmaxf((float)(total[r] + (double)bias[co]), 0.f);
        }
    }
}

// 3x3 stride-2 max-pool with floor, no padding: every window lies inside the map
__global__ __launch_bounds__(256) void quality_pool_kernel(const float* in, long planes, int Hin, int Win, int Ho, int Wo, float* out) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= planes * Ho * Wo) return;
    const int ox = (int)(e % Wo), oy = (int)((e / Wo) % Ho);
    const float* p = in + (e / ((long)Ho * Wo)) * Hin * Win + (long)(2 * oy) * Win + 2 * ox;
    float m = p[0];
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) m = fmaxf(m, p[dy * Win + dx]);
    out[e] = m;
}

constexpr int QT_THREADS = 1024;

// sum over the block in a fixed tree; the result is valid in thread 0
__device__ __forceinline__ double block_tree_sum(double v, double* sh, int threads) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int o = threads / 2; o >= 1; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    return sh[0];
}

// taps[pair][tap] = mean_p sum_c lin[c] (fa[c][p] / (|fa[:, p]| + 1e-10) - fb[c][p] / (|fb[:, p]| + 1e-10))^2; one block per pair
__global__ __launch_bounds__(QT_THREADS) void quality_tap_kernel(const float* feat, int n_pairs, int C, int P, const float* lin, int tap,
                                                                 double* taps) {
    // every product is rounded on its own: with a fused multiply-subtract in fa ia - fb ib equal features would not give exactly
    // 0, and a - b would not be -(b - a)
#pragma clang fp contract(off)
    __shared__ double sh[QT_THREADS];
    const int pair = blockIdx.x;
    const float* fa = feat + (long)pair * C * P;
    const float* fb = feat + (long)(n_pairs + pair) * C * P;
    double sum = 0.0;
    for (int p = threadIdx.x; p < P; p += QT_THREADS) {
        double sa = 0.0, sb = 0.0;
        for (int c = 0; c < C; ++c) {
            const double a = fa[(long)c * P + p], b = fb[(long)c * P + p];
            sa += a * a; sb += b * b;
        }
        const double ia = 1.0 / (sqrt(sa) + 1e-10), ib = 1.0 / (sqrt(sb) + 1e-10);
        double d = 0.0;
        for (int c = 0; c < C; ++c) {
            const double t = (double)fa[(long)c * P + p] * ia - (double)fb[(long)c * P + p] * ib;
            d += (double)lin[c] * (t * t);
        }
        sum += d;
    }
    const double tot = block_tree_sum(sum, sh, QT_THREADS);
    if (threadIdx.x == 0) taps[pair * 5 + tap] = tot / (double)P;
}

__global__ __launch_bounds__(256) void quality_lpips_out_kernel(const double* taps, int n, float* out, float* taps_out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double t = 0.0;
    for (int k = 0; k < 5; ++k) {
        t += taps[i * 5 + k];
        if (taps_out) taps_out[i * 5 + k] = (float)taps[i * 5 + k];
    }
    out[i] = (float)t;
}

struct SsimWindow { double g[11]; };
constexpr int SS_T = 16, SS_P = SS_T + 10;

__device__ __forceinline__ int reflect(int i, int n) { return i < 0 ? -i : i >= n ? 2 * n - 2 - i : i; }

// part[(img C + c) tiles + tile] = sum of the SSIM map over the tile; grid (tiles_x, tiles_y, n C); (y0, x0), mh x mw: the
// map's corner in the plane and its size (the 5-pixel border cropped or not)
__global__ __launch_bounds__(256) void quality_ssim_kernel(const float* a, const float* b, int H, int W, int y0, int x0, int mh, int mw,
                                                           SsimWindow win, double c1, double c2, double* part) {
    __shared__ float pa[SS_P * SS_P], pb[SS_P * SS_P];
    __shared__ double sh[256];
    const long plane = (long)blockIdx.z * H * W;
    const int ty0 = y0 + blockIdx.y * SS_T, tx0 = x0 + blockIdx.x * SS_T;
    for (int e = threadIdx.x; e < SS_P * SS_P; e += 256) {
        const int yy = reflect(min(ty0 + e / SS_P - 5, H + 4), H), xx = reflect(min(tx0 + e % SS_P - 5, W + 4), W);
        pa[e] = a[plane + (long)yy * W + xx];
        pb[e] = b[plane + (long)yy * W + xx];
    }
    __syncthreads();
    const int ly = threadIdx.x / SS_T, lx = threadIdx.x % SS_T;
    double v = 0.0;
    if ((int)blockIdx.y * SS_T + ly < mh && (int)blockIdx.x * SS_T + lx < mw) {
        double mp = 0.0, mt = 0.0, epp = 0.0, ett = 0.0, ept = 0.0;
        for (int ky = 0; ky < 11; ++ky)
            for (int kx = 0; kx < 11; ++kx) {
                const double wgt = win.g[ky] * win.g[kx];
                const double p = pa[(ly + ky) * SS_P + lx + kx], t = pb[(ly + ky) * SS_P + lx + kx];
                mp += wgt * p; mt += wgt * t; epp += wgt * (p * p); ett += wgt * (t * t); ept += wgt * (p * t);
            }
        const double spp = epp - mp * mp, stt = ett - mt * mt, spt = ept - mp * mt;
        v = ((2.0 * mp * mt + c1) * (2.0 * spt + c2)) / ((mp * mp + mt * mt + c1) * (spp + stt + c2));
    }
    const double tot = block_tree_sum(v, sh, 256);
    if (threadIdx.x == 0) part[(long)blockIdx.z * gridDim.x * gridDim.y + blockIdx.y * gridDim.x + blockIdx.x] = tot;
}

// out[img] = sum of the image's `count` partial sums / elems; one block per image
__global__ __launch_bounds__(256) void quality_ssim_mean_kernel(const double* part, long count, double elems, double* out) {
    __shared__ double sh[256];
    const double* p = part + (long)blockIdx.x * count;
    double s = 0.0;
    for (long e = threadIdx.x; e < count; e += 256) s += p[e];
    const double tot = block_tree_sum(s, sh, 256);
    if (threadIdx.x == 0) out[blockIdx.x] = tot / elems;
}

// sum[img] = sum over mask != 0 of (a - b)^2, count[img] = the masked elements; one block per image
__global__ __launch_bounds__(QT_THREADS) void quality_mmse_kernel(const float* a, const float* b, const unsigned char* mask, long elems,
                                                                  double* sum, long long* count) {
    __shared__ double sh[QT_THREADS];
    const long base = (long)blockIdx.x * elems;
    double s = 0.0, c = 0.0;
    for (long e = threadIdx.x; e < elems; e += QT_THREADS)
        if (mask[base + e]) {
            const double d = (double)a[base + e] - (double)b[base + e];
            s += d * d; c += 1.0;
        }
    const double ts = block_tree_sum(s, sh, QT_THREADS);
    __syncthreads();
    const double tc = block_tree_sum(c, sh, QT_THREADS);       // counts below 2^53: exact
    if (threadIdx.x == 0) { sum[blockIdx.x] = ts; count[blockIdx.x] = (long long)tc; }
}

template <int KS, int STRIDE, int PAD, bool FIRST>
void launch_conv(const float* in, const float* in_b, int n_pairs, int Cin, int Hin, int Win, int Ho, int Wo, const QualityLayer& ly,
                 int Cout, int normalize, float* out, hipStream_t st) {
    hipLaunchKernelGGL((quality_conv_kernel<KS, STRIDE, PAD, FIRST>), dim3((Ho * Wo + 63) / 64, Cout / 64, 2 * n_pairs), dim3(256), 0, st,
                       in, in_b, n_pairs, Cin, Hin, Win, Ho, Wo, ly.w, ly.b, Cout, normalize, out);
}

}  // namespace
}  // namespace loco

using namespace loco;

namespace {
thread_local std::string g_quality_create_err;

long ssim_tiles(int H, int W) {
    const bool crop = H > 10 && W > 10;
    const long mh = crop ? H - 10 : H, mw = crop ? W - 10 : W;
    return ((mh + SS_T - 1) / SS_T) * ((mw + SS_T - 1) / SS_T);
}
// the most tiles a plane of at most H x W can have: the cropped map of the largest plane, or an uncropped strip (a side of at
// most 10: one row or column of tiles along the other side)
long ssim_tiles_max(int H, int W) {
    return std::max(ssim_tiles(H, W), std::max(ssim_tiles(std::min(H, 10), W), ssim_tiles(H, std::min(W, 10))));
}
}  // namespace

extern "C" {

int loco_quality_create(const loco_quality_cfg* cfg, int32_t device, int32_t max_pairs, loco_quality** out) {
    auto refuse = [&](const loco_quality_cfg& c) -> std::string {
        if (c.max_h <= 0 || c.max_w <= 0 || max_pairs <= 0) return "max_h, max_w and max_pairs must be positive";
        if ((long)c.max_h * c.max_w > (1L << 24)) return "max_h x max_w > 2^24";
        if ((long)c.max_h * c.max_w * max_pairs > (1L << 28)) return "max_pairs x max_h x max_w > 2^28";
        double s = 0.0;
        for (double g : c.ssim_window) {
            if (!(g > 0.0)) return "ssim_window must hold 11 positive weights";
            s += g;
        }
        if (std::fabs(s - 1.0) > 1e-9) return "ssim_window must sum to 1";
        return "";
    };
    return encoder_create<loco_quality>("loco_quality_create", g_quality_create_err, cfg, device, out, refuse, [&](loco_quality& t) {
        t.cfg = *cfg;
        t.max_pairs = max_pairs;
        // names of eval.lpips_weight_names(): torchvision AlexNet convolutions and the 1x1 heads of the lpips package
        ParamTable& pt = t.table;
        for (int l = 0; l < 5; ++l) {
            const AlexLayer& a = ALEX[l];
            const std::string f = "features." + std::to_string(ALEX_INDEX[l]) + ".";
            pt.add(f + "weight", {a.cout, a.cin, a.ks, a.ks}, &t.layer[l].w);
            pt.add(f + "bias", {a.cout}, &t.layer[l].b);
        }
        for (int l = 0; l < 5; ++l) pt.add("lin" + std::to_string(l) + ".model.1.weight", {1, ALEX[l].cout, 1, 1}, &t.layer[l].lin);
        // feature maps of 2 max_pairs images: the convolutions write feat0 and feat1 in turn
        const AlexGeom g = alex_geom(cfg->max_h, cfg->max_w);
        long f0 = 1, f1 = 1, pl = 1;
        for (int l = 0; l < 5; ++l) {
            long& f = l % 2 ? f1 : f0;
            f = std::max(f, (long)ALEX[l].cout * g.h[l] * g.w[l]);
        }
        for (int i = 0; i < 2; ++i) pl = std::max(pl, (long)ALEX[i].cout * g.ph[i] * g.pw[i]);
        const long imgs = 2L * max_pairs;
        t.ssim_part_cap = 3L * max_pairs * ssim_tiles_max(cfg->max_h, cfg->max_w);
        using B = EncoderBase;
        return t.alloc({B::buf(&t.feat0, f0 * imgs), B::buf(&t.feat1, f1 * imgs), B::buf(&t.pool, pl * imgs),
                        B::buf(&t.taps, 5L * max_pairs), B::buf(&t.ssim_part, t.ssim_part_cap)});
    });
}

int loco_quality_load_param(loco_quality* q, const char* name, const float* host, const int64_t* shape, int32_t ndim) {
    return q ? q->table.load(name, host, shape, ndim, q->device, "loco_quality_load_param", q->err) : -1;
}

int loco_quality_params_missing(loco_quality* q) { return q ? q->table.missing(q->err) : -1; }

int loco_quality_lpips(loco_quality* q, const float* a_dev, const float* b_dev, int32_t n, int32_t H, int32_t W, int32_t normalize,
                       float* out_dev, float* taps_dev, void* stream) {
    if (!q) return -1;
    if (!a_dev || !b_dev || !out_dev) return q->fail("loco_quality_lpips: null a, b or out");
    if (n <= 0 || n > q->max_pairs)
        return q->fail("loco_quality_lpips: n = " + std::to_string(n) + " outside [1, max_pairs = " + std::to_string(q->max_pairs) + "]");
    if (H < 31 || W < 31)
        return q->fail("loco_quality_lpips: H = " + std::to_string(H) + ", W = " + std::to_string(W) + " below 31 (the last taps would be empty)");
    if (H > q->cfg.max_h || W > q->cfg.max_w)
        return q->fail("loco_quality_lpips: H x W = " + std::to_string(H) + " x " + std::to_string(W) + " above the configured " +
                       std::to_string(q->cfg.max_h) + " x " + std::to_string(q->cfg.max_w));
    if (q->table.missing(q->err)) {
        q->err = "loco_quality_lpips: " + q->err;
        return -1;
    }
    DeviceGuard dg(q->device);
    hipStream_t st = (hipStream_t)stream;
    const AlexGeom g = alex_geom(H, W);
    const long imgs = 2L * n;
    auto tap = [&](int l, const float* feat) {
        hipLaunchKernelGGL(quality_tap_kernel, dim3(n), dim3(QT_THREADS), 0, st, feat, n, ALEX[l].cout, g.h[l] * g.w[l], q->layer[l].lin, l,
                           q->taps);
    };
    auto pool = [&](int i, const float* feat, int l) {
        hipLaunchKernelGGL(quality_pool_kernel, dim3(blocks256(imgs * ALEX[l].cout * g.ph[i] * g.pw[i])), dim3(256), 0, st, feat,
                           imgs * ALEX[l].cout, g.h[l], g.w[l], g.ph[i], g.pw[i], q->pool);
    };
    launch_conv<11, 4, 2, true>(a_dev, b_dev, n, 3, H, W, g.h[0], g.w[0], q->layer[0], 64, normalize, q->feat0, st);
    tap(0, q->feat0);
    pool(0, q->feat0, 0);
    launch_conv<5, 1, 2, false>(q->pool, nullptr, n, 64, g.ph[0], g.pw[0], g.h[1], g.w[1], q->layer[1], 192, 0, q->feat1, st);
    tap(1, q->feat1);
    pool(1, q->feat1, 1);
    launch_conv<3, 1, 1, false>(q->pool, nullptr, n, 192, g.ph[1], g.pw[1], g.h[2], g.w[2], q->layer[2], 384, 0, q->feat0, st);
    tap(2, q->feat0);
    launch_conv<3, 1, 1, false>(q->feat0, nullptr, n, 384, g.h[2], g.w[2], g.h[3], g.w[3], q->layer[3], 256, 0, q->feat1, st);
    tap(3, q->feat1);
    launch_conv<3, 1, 1, false>(q->feat1, nullptr, n, 256, g.h[3], g.w[3], g.h[4], g.w[4], q->layer[4], 256, 0, q->feat0, st);
    tap(4, q->feat0);
    hipLaunchKernelGGL(quality_lpips_out_kernel, dim3(blocks256(n)), dim3(256), 0, st, q->taps, n, out_dev, taps_dev);
    if (hipGetLastError() != hipSuccess) return q->fail("loco_quality_lpips: kernel launch failed");
    return 0;
}

int loco_quality_ssim(loco_quality* q, const float* a_dev, const float* b_dev, int32_t n, int32_t C, int32_t H, int32_t W,
                      double data_range, double* out_dev, void* stream) {
    if (!q) return -1;
    if (!a_dev || !b_dev || !out_dev) return q->fail("loco_quality_ssim: null a, b or out");
    if (n <= 0 || n > q->max_pairs)
        return q->fail("loco_quality_ssim: n = " + std::to_string(n) + " outside [1, max_pairs = " + std::to_string(q->max_pairs) + "]");
    if (C <= 0) return q->fail("loco_quality_ssim: C must be positive");
    if (H < 6 || W < 6)
        return q->fail("loco_quality_ssim: H = " + std::to_string(H) + ", W = " + std::to_string(W) + " below 6 (reflect padding of 5 is undefined)");
    if (H > q->cfg.max_h || W > q->cfg.max_w)
        return q->fail("loco_quality_ssim: H x W = " + std::to_string(H) + " x " + std::to_string(W) + " above the configured " +
                       std::to_string(q->cfg.max_h) + " x " + std::to_string(q->cfg.max_w));
    if (!(data_range > 0.0)) return q->fail("loco_quality_ssim: data_range must be positive");
    const long tiles = ssim_tiles(H, W);
    if ((long)n * C * tiles > q->ssim_part_cap || (long)n * C > 65535)
        return q->fail("loco_quality_ssim: n x C = " + std::to_string((long)n * C) + " planes exceed the workspace of 3 max_pairs planes at the configured size");
    DeviceGuard dg(q->device);
    hipStream_t st = (hipStream_t)stream;
    const bool crop = H > 10 && W > 10;
    const int y0 = crop ? 5 : 0, x0 = crop ? 5 : 0, mh = crop ? H - 10 : H, mw = crop ? W - 10 : W;
    SsimWindow win;
    for (int i = 0; i < 11; ++i) win.g[i] = q->cfg.ssim_window[i];
    const double c1 = (0.01 * data_range) * (0.01 * data_range), c2 = (0.03 * data_range) * (0.03 * data_range);
    hipLaunchKernelGGL(quality_ssim_kernel, dim3((mw + SS_T - 1) / SS_T, (mh + SS_T - 1) / SS_T, n * C), dim3(256), 0, st, a_dev, b_dev, H, W,
                       y0, x0, mh, mw, win, c1, c2, q->ssim_part);
    hipLaunchKernelGGL(quality_ssim_mean_kernel, dim3(n), dim3(256), 0, st, q->ssim_part, (long)C * tiles, (double)C * mh * mw, out_dev);
    if (hipGetLastError() != hipSuccess) return q->fail("loco_quality_ssim: kernel launch failed");
    return 0;
}

int loco_quality_masked_mse(loco_quality* q, const float* a_dev, const float* b_dev, const uint8_t* mask_dev, int32_t n, int64_t elems,
                            double* sum_dev, int64_t* count_dev, void* stream) {
    if (!q) return -1;
    if (!a_dev || !b_dev || !mask_dev || !sum_dev || !count_dev) return q->fail("loco_quality_masked_mse: null a, b, mask, sum or count");
    if (n <= 0 || n > q->max_pairs)
        return q->fail("loco_quality_masked_mse: n = " + std::to_string(n) + " outside [1, max_pairs = " + std::to_string(q->max_pairs) + "]");
    if (elems <= 0) return q->fail("loco_quality_masked_mse: elems must be positive");
    DeviceGuard dg(q->device);
    hipLaunchKernelGGL(quality_mmse_kernel, dim3(n), dim3(QT_THREADS), 0, (hipStream_t)stream, a_dev, b_dev, mask_dev, (long)elems, sum_dev,
                       (long long*)count_dev);
    if (hipGetLastError() != hipSuccess) return q->fail("loco_quality_masked_mse: kernel launch failed");
    return 0;
}

const char* loco_quality_last_error(loco_quality* q) { return q ? q->err.c_str() : g_quality_create_err.c_str(); }

void loco_quality_destroy(loco_quality* q) { delete q; }

}  // extern "C"
