// The trainable h-space block f_t of the Asyrp baseline (include/loco_hip.h loco_asyrp_*): forward, the
// gradients of its ten parameters and of its input, and the Adam step, all on the device.  For h [B][C][H][W] and a time
// vector e [E]:
//     a1 = swish(GroupNorm32(h; g1, b1))
//     y1 = W1 a1 + c1 + (Wt swish(e) + ct)            W1 [C][C] (a 1x1 conv), Wt [C][E]
//     a2 = swish(GroupNorm32(y1; g2, b2))
//     dh = s (W2 a2 + c2)                              W2 [C][C]
//
// Layout: inside the unit every activation is channel-major [C][N] with N = B HW and n = b HW + hw, so each of the six
// products is ONE matrix product (the weight gradients contract over all of N); h and g_dh are repacked on the way in,
// dh and g_h are written NCHW by the kernel that forms them.
//
// Arithmetic: the maps are 8x8 .. 16x16 with C <= 1280, so every launch is latency-shaped and nothing here is near a
// rate limit; the unit spends that slack on accuracy.  Products of fp32 operands are formed exactly (a product of two
// fp32 values is exact in double) and every sum -- the contractions of the six products, GroupNorm's moments (two
// passes), the per-channel sums behind the gain / offset / bias gradients, Wt swish(e) -- is accumulated in double and
// rounded to fp32 once.  (launch_gemm's fp32 accumulation chain of length K = C is what the unit would otherwise add to
// each of them; this is pca.hip's Gram arithmetic.)  GroupNorm's {mean, rstd} stay in double.
// Determinism: no atomics; every reduction is a fixed tree (wave shuffle, then waves / samples in index order), the tile
// shape of the product kernel does not depend on the data, and gradient accumulation is "store += this call's sum".
#include "encoder_common.h"

#include <cmath>

constexpr int ASYRP_GROUPS = 32;
constexpr int ASYRP_MAX_CPG = 64;       // channels per group the statistics kernels hold in LDS: C <= 2048

struct loco_asyrp : loco::EncoderBase {
    int C = 0, H = 0, W = 0, E = 0, max_batch = 0;
    float eps = 1e-6f;
    // parameters (inside `params`, see the table) and their views inside the gradient store
    float *g1 = nullptr, *b1 = nullptr, *W1 = nullptr, *c1 = nullptr, *Wt = nullptr, *ct = nullptr, *g2 = nullptr, *b2 = nullptr,
          *W2 = nullptr, *c2 = nullptr;
    float *grad = nullptr, *m = nullptr, *v = nullptr;             // table.total floats each, the table's layout
    // records of the last forward, channel-major [C][N]
    float *hc = nullptr, *a1 = nullptr, *y1 = nullptr, *a2 = nullptr, *se = nullptr, *bias1 = nullptr, *bias2 = nullptr;
    double *st1 = nullptr, *st2 = nullptr;                         // [B][32]{mean, rstd}
    // backward workspace
    float *t0 = nullptr, *t1 = nullptr;                            // [C][N]
    double *S = nullptr, *tst = nullptr, *rs = nullptr;            // [B][C]{S1, S2}, [B][32]{m1, m2}, [C]
    int rec_B = 0;                                                 // 0: no records
    float rec_s = 1.f;
    float* gp(const float* p) const { return grad + (p - params); }
};

namespace loco {
namespace {

std::string g_asyrp_create_err;

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
// sum over the 256 threads of a block, waves added in order; sh: 4 doubles
__device__ __forceinline__ double block_sum_d(double v, double* sh) {
    v = wave_sum_d(v);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    const double r = ((sh[0] + sh[1]) + sh[2]) + sh[3];
    __syncthreads();
    return r;
}
__device__ __forceinline__ float swish_f(float y) { return y / (1.0f + expf(-y)); }
__device__ __forceinline__ float swish_d(float y) {
    const float sg = 1.0f / (1.0f + expf(-y));
    return sg * (1.0f + y * (1.0f - sg));
}

// out[c][b HW + hw] = scale x[b][c][hw]
__global__ __launch_bounds__(256) void asyrp_pack_kernel(const float* x, float scale, int C, int HW, int B, float* out) {
    const long N = (long)B * HW, total = (long)C * N;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int c = (int)(e / N);
    const long n = e % N;
    const int b = (int)(n / HW), hw = (int)(n % HW);
    out[e] = scale * x[((long)b * C + c) * HW + hw];
}

// st[b][g] = {mean, rstd} of group g of sample b of x [C][N], two passes in double.  grid (32, B)
__global__ __launch_bounds__(256) void asyrp_gn_stats_kernel(const float* x, int HW, long N, int cpg, double eps, double* st) {
    __shared__ double sh[4];
    const int g = blockIdx.x, b = blockIdx.y;
    const int cnt = cpg * HW;
    const float* xb = x + (long)g * cpg * N + (long)b * HW;
    double s = 0.0;
    for (int i = threadIdx.x; i < cnt; i += 256) s += (double)xb[(long)(i / HW) * N + i % HW];
    const double mean = block_sum_d(s, sh) / cnt;
    double q = 0.0;
    for (int i = threadIdx.x; i < cnt; i += 256) {
        const double d = (double)xb[(long)(i / HW) * N + i % HW] - mean;
        q = fma(d, d, q);
    }
    const double var = block_sum_d(q, sh) / cnt;
    if (threadIdx.x == 0) {
        st[((long)b * ASYRP_GROUPS + g) * 2] = mean;
        st[((long)b * ASYRP_GROUPS + g) * 2 + 1] = 1.0 / sqrt(var + eps);
    }
}

// a = swish(gamma xhat + beta), x and a [C][N]
__global__ __launch_bounds__(256) void asyrp_gn_act_kernel(const float* x, const double* st, const float* gamma, const float* beta, int C,
                                                           int HW, long N, int cpg, float* a) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)C * N) return;
    const int c = (int)(e / N);
    const int b = (int)((e % N) / HW);
    const double* s = st + ((long)b * ASYRP_GROUPS + c / cpg) * 2;
    const float xh = (float)(((double)x[e] - s[0]) * s[1]);
    a[e] = swish_f(fmaf(gamma[c], xh, beta[c]));
}

// se[j] = swish(e[j]);  bias1[c] = c1[c] + (Wt[c] . se + ct[c]);  bias2[c] = s c2[c].  One wave per channel, grid ceil(C / 4)
__global__ __launch_bounds__(256) void asyrp_time_kernel(const float* Wt, const float* ct, const float* c1, const float* c2, const float* e,
                                                         int E, int C, float s, float* se, float* bias1, float* bias2) {
    const int lane = threadIdx.x & 63, c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (blockIdx.x == 0)
        for (int j = threadIdx.x; j < E; j += 256) se[j] = swish_f(e[j]);
    if (c >= C) return;
    double acc = 0.0;
    for (int j = lane; j < E; j += 64) acc = fma((double)Wt[(long)c * E + j], (double)swish_f(e[j]), acc);
    acc = wave_sum_d(acc);
    if (lane == 0) {
        bias1[c] = (float)((double)c1[c] + (acc + (double)ct[c]));
        bias2[c] = s * c2[c];
    }
}

// out(m, n) = alpha sum_k A(m, k) B(k, n) + bias[m] + beta out(m, n), with A(m, k) = A[m sam + k sak], B(k, n) = B[k sbk + n sbn]
// and out(m, n) = out[m scm + (n / nb) scb + n % nb] (nb = HW, scb = C HW: an NCHW tensor; nb >= Nn: a plain matrix).
// Exact products summed in double in k order, one rounding.  32 x 32 tile, 2 x 2 per thread.  grid (ceil(Nn / 32), ceil(M / 32))
struct AsyrpGemm {
    const float* A; long sam, sak;
    const float* B; long sbk, sbn;
    int M, Nn, K;
    float alpha, beta;
    const float* bias;
    float* out; long scm, scb; int nb;
};
__global__ __launch_bounds__(256) void asyrp_gemm_kernel(AsyrpGemm g) {
    __shared__ float As[32][33], Bs[32][33];      // [k][m], [k][n]
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int m0 = blockIdx.y * 32, n0 = blockIdx.x * 32;
    double acc[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
    for (int kb = 0; kb < g.K; kb += 32) {
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int e = threadIdx.x + it * 256;
            int am, ak, bn, bk;                   // the fast index of the thread order follows the operand's unit stride
            if (g.sak == 1) { ak = e & 31; am = e >> 5; } else { am = e & 31; ak = e >> 5; }
            if (g.sbk == 1) { bk = e & 31; bn = e >> 5; } else { bn = e & 31; bk = e >> 5; }
            const bool va = m0 + am < g.M && kb + ak < g.K, vb = n0 + bn < g.Nn && kb + bk < g.K;
            As[ak][am] = va ? g.A[(long)(m0 + am) * g.sam + (long)(kb + ak) * g.sak] : 0.f;
            Bs[bk][bn] = vb ? g.B[(long)(kb + bk) * g.sbk + (long)(n0 + bn) * g.sbn] : 0.f;
        }
        __syncthreads();
#pragma unroll 8
        for (int k = 0; k < 32; ++k) {
            const double a0 = As[k][ty * 2], a1 = As[k][ty * 2 + 1], b0 = Bs[k][tx * 2], b1 = Bs[k][tx * 2 + 1];
            acc[0][0] = fma(a0, b0, acc[0][0]); acc[0][1] = fma(a0, b1, acc[0][1]);
            acc[1][0] = fma(a1, b0, acc[1][0]); acc[1][1] = fma(a1, b1, acc[1][1]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int m = m0 + ty * 2 + i, n = n0 + tx * 2 + j;
            if (m >= g.M || n >= g.Nn) continue;
            float* o = g.out + (long)m * g.scm + (long)(n / g.nb) * g.scb + n % g.nb;
            double v = (double)g.alpha * acc[i][j];
            if (g.bias) v += (double)g.bias[m];
            if (g.beta != 0.f) v += (double)g.beta * (double)*o;
            *o = (float)v;
        }
}

// The sums behind the cotangent of a = swish(gamma xhat + beta) for the cotangent ga of a (both [C][N]):
//     S[b][c] = {sum_hw d, sum_hw d xhat},  d = swish'(y) ga           (offset / gain gradient of sample b)
//     tst[b][g] = {mean_g(gamma d), mean_g(gamma d xhat)}
// One wave per channel of the group, channels in order by one thread.  grid (32, B)
__global__ __launch_bounds__(256) void asyrp_gn_bwd_sums_kernel(const float* ga, const float* x, const double* st, const float* gamma,
                                                                const float* beta, int C, int HW, long N, int cpg, double* S, double* tst) {
    __shared__ double sc[ASYRP_MAX_CPG][2];
    const int g = blockIdx.x, b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double mean = st[((long)b * ASYRP_GROUPS + g) * 2], rstd = st[((long)b * ASYRP_GROUPS + g) * 2 + 1];
    for (int cl = wave; cl < cpg; cl += 4) {
        const int c = g * cpg + cl;
        const long row = (long)c * N + (long)b * HW;
        const float gm = gamma[c], bt = beta[c];
        double s1 = 0.0, s2 = 0.0;
        for (int hw = lane; hw < HW; hw += 64) {
            const float xh = (float)(((double)x[row + hw] - mean) * rstd);
            const double d = (double)(swish_d(fmaf(gm, xh, bt)) * ga[row + hw]);
            s1 += d;
            s2 = fma(d, (double)xh, s2);
        }
        s1 = wave_sum_d(s1); s2 = wave_sum_d(s2);
        if (lane == 0) {
            sc[cl][0] = s1; sc[cl][1] = s2;
            S[((long)b * C + c) * 2] = s1; S[((long)b * C + c) * 2 + 1] = s2;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double m1 = 0.0, m2 = 0.0;
        for (int cl = 0; cl < cpg; ++cl) {
            const double gm = (double)gamma[g * cpg + cl];
            m1 = fma(gm, sc[cl][0], m1);
            m2 = fma(gm, sc[cl][1], m2);
        }
        tst[((long)b * ASYRP_GROUPS + g) * 2] = m1 / ((double)cpg * HW);
        tst[((long)b * ASYRP_GROUPS + g) * 2 + 1] = m2 / ((double)cpg * HW);
    }
}
// dgamma[c] += sum_b S[b][c][1], dbeta[c] += sum_b S[b][c][0], samples in order
__global__ __launch_bounds__(256) void asyrp_gn_param_grad_kernel(const double* S, int B, int C, float* dgamma, float* dbeta) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    double s1 = 0.0, s2 = 0.0;
    for (int b = 0; b < B; ++b) { s1 += S[((long)b * C + c) * 2]; s2 += S[((long)b * C + c) * 2 + 1]; }
    dbeta[c] = (float)((double)dbeta[c] + s1);
    dgamma[c] = (float)((double)dgamma[c] + s2);
}
// gx = rstd (gamma swish'(y) ga - m1 - xhat m2), written at out[c ocs + (n / nb) obs + n % nb]
__global__ __launch_bounds__(256) void asyrp_gn_bwd_apply_kernel(const float* ga, const float* x, const double* st, const float* gamma,
                                                                 const float* beta, const double* tst, int C, int HW, long N, int cpg,
                                                                 float* out, long ocs, long obs, long nb) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)C * N) return;
    const int c = (int)(e / N);
    const long n = e % N;
    const long sg = ((long)(n / HW) * ASYRP_GROUPS + c / cpg) * 2;
    const double rstd = st[sg + 1];
    const float xh = (float)(((double)x[e] - st[sg]) * rstd);
    const double z = (double)(gamma[c] * swish_d(fmaf(gamma[c], xh, beta[c]))) * (double)ga[e];
    out[(long)c * ocs + (n / nb) * obs + n % nb] = (float)(rstd * (z - tst[sg] - (double)xh * tst[sg + 1]));
}

// r = sum_n g[c][n]:  d0[c] += r, d1[c] += r (d1 may be null), rs[c] = r (may be null).  One wave per channel, grid ceil(C / 4)
__global__ __launch_bounds__(256) void asyrp_bias_grad_kernel(const float* g, int C, long N, float* d0, float* d1, double* rs) {
    const int lane = threadIdx.x & 63, c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= C) return;
    double r = 0.0;
    for (long n = lane; n < N; n += 64) r += (double)g[(long)c * N + n];
    r = wave_sum_d(r);
    if (lane == 0) {
        d0[c] = (float)((double)d0[c] + r);
        if (d1) d1[c] = (float)((double)d1[c] + r);
        if (rs) rs[c] = r;
    }
}
// dWt[c][j] += rs[c] se[j]
__global__ __launch_bounds__(256) void asyrp_outer_kernel(const double* rs, const float* se, int C, int E, float* dWt) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)C * E) return;
    dWt[e] = (float)fma(rs[e / E], (double)se[e % E], (double)dWt[e]);
}

// Adam (Kingma & Ba; torch.optim.Adam's arithmetic without weight decay / amsgrad) over the whole parameter block:
//     m = b1 m + (1 - b1) g,  v = b2 v + (1 - b2) g^2,  p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps)
__global__ __launch_bounds__(256) void asyrp_adam_kernel(float* p, const float* g, float* m, float* v, long total, float lr_bc1, float rsq_bc2,
                                                         float b1, float b2, float eps) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const float ge = g[e];
    const float me = fmaf(b1, m[e], (1.0f - b1) * ge);
    const float ve = fmaf(b2, v[e], (1.0f - b2) * ge * ge);
    m[e] = me; v[e] = ve;
    p[e] -= lr_bc1 * me / (sqrtf(ve) * rsq_bc2 + eps);
}

void asyrp_gemm(const float* A, long sam, long sak, const float* B, long sbk, long sbn, int M, int Nn, int K, float alpha, float beta,
                const float* bias, float* out, long scm, long scb, int nb, hipStream_t st) {
    AsyrpGemm g{A, sam, sak, B, sbk, sbn, M, Nn, K, alpha, beta, bias, out, scm, scb, nb};
    hipLaunchKernelGGL(asyrp_gemm_kernel, dim3((Nn + 31) / 32, (M + 31) / 32), dim3(256), 0, st, g);
}

bool asyrp_ok(loco_asyrp* p, hipError_t e, const char* what) {
    if (e == hipSuccess) return true;
    p->err = std::string(what) + ": " + hipGetErrorString(e);
    return false;
}

ParamTable::Param* asyrp_find(loco_asyrp* p, const char* name) {
    if (!name) return nullptr;
    for (auto& q : p->table.params)
        if (q.name == name) return &q;
    return nullptr;
}

}  // namespace
}  // namespace loco

using namespace loco;

extern "C" {

int loco_asyrp_create(int32_t device, int32_t C, int32_t H, int32_t W, int32_t E, int32_t max_batch, float gn_eps, loco_asyrp** out) {
    struct Cfg { int32_t C, H, W, E, max_batch; float eps; } cfg{C, H, W, E, max_batch, gn_eps};
    return encoder_create<loco_asyrp>("loco_asyrp_create", g_asyrp_create_err, &cfg, device, out,
        [](const Cfg& c) -> std::string {
            if (c.C < ASYRP_GROUPS || c.C % ASYRP_GROUPS)
                return "C = " + std::to_string(c.C) + " is not a positive multiple of the " + std::to_string(ASYRP_GROUPS) + " GroupNorm groups";
            if (c.C > ASYRP_GROUPS * ASYRP_MAX_CPG) return "C = " + std::to_string(c.C) + " is above the unit's limit of " + std::to_string(ASYRP_GROUPS * ASYRP_MAX_CPG);
            if (c.H < 1 || c.W < 1 || c.H > 64 || c.W > 64) return "the map must be 1 x 1 .. 64 x 64";
            if (c.E < 1 || c.E > 8192) return "the time vector's width E must be in [1, 8192]";
            if (c.max_batch < 1 || c.max_batch > 64) return "max_batch must be in [1, 64]";
            if (!(c.eps > 0.f)) return "gn_eps must be positive";
            return "";
        },
        [&](loco_asyrp& p) {
            p.C = C; p.H = H; p.W = W; p.E = E; p.max_batch = max_batch; p.eps = gn_eps;
            ParamTable& t = p.table;
            t.add("g1", {C}, &p.g1); t.add("b1", {C}, &p.b1); t.add("W1", {C, C}, &p.W1); t.add("c1", {C}, &p.c1);
            t.add("Wt", {C, E}, &p.Wt); t.add("ct", {C}, &p.ct); t.add("g2", {C}, &p.g2); t.add("b2", {C}, &p.b2);
            t.add("W2", {C, C}, &p.W2); t.add("c2", {C}, &p.c2);
            const size_t cn = (size_t)C * max_batch * H * W, bg = (size_t)max_batch * ASYRP_GROUPS * 2;
            using EB = EncoderBase;
            // the parameter block is zeroed too: the padding between parameters takes part in the Adam launch
            if (!p.alloc({EB::buf(&p.grad, t.total, true), EB::buf(&p.m, t.total, true), EB::buf(&p.v, t.total, true), EB::buf(&p.hc, cn),
                          EB::buf(&p.a1, cn), EB::buf(&p.y1, cn), EB::buf(&p.a2, cn), EB::buf(&p.se, (size_t)E), EB::buf(&p.bias1, (size_t)C),
                          EB::buf(&p.bias2, (size_t)C), EB::buf(&p.st1, bg), EB::buf(&p.st2, bg), EB::buf(&p.t0, cn), EB::buf(&p.t1, cn),
                          EB::buf(&p.S, (size_t)max_batch * C * 2), EB::buf(&p.tst, bg), EB::buf(&p.rs, (size_t)C)}))
                return false;
            return hipMemset(p.params, 0, t.total * sizeof(float)) == hipSuccess;
        });
}

int loco_asyrp_load_param(loco_asyrp* p, const char* name, const float* data, const int64_t* shape, int32_t ndim) {
    if (!p) return -2;
    return p->table.load(name, data, shape, ndim, p->device, "loco_asyrp_load_param", p->err);
}

int loco_asyrp_params_missing(loco_asyrp* p) {
    if (!p) return -2;
    std::string m;
    const int miss = p->table.missing(m);
    if (miss) p->err = "loco_asyrp: " + m;
    return miss;
}

static int asyrp_read(loco_asyrp* p, const char* fn, const char* name, float* dst, int64_t count, const float* base) {
    ParamTable::Param* q = asyrp_find(p, name);
    if (!q) return p->fail(std::string(fn) + ": unknown parameter " + (name ? name : "(null)"));
    if (!dst) return p->fail(std::string(fn) + ": null argument");
    const size_t cnt = ParamTable::count(q->shape);
    if (count != (int64_t)cnt) return p->fail(std::string(fn) + ": " + q->name + " has " + std::to_string(cnt) + " values, the buffer holds " + std::to_string(count));
    DeviceGuard dg(p->device);
    if (!asyrp_ok(p, hipDeviceSynchronize(), fn) || !asyrp_ok(p, hipMemcpy(dst, base + q->off, cnt * sizeof(float), hipMemcpyDefault), fn)) return -1;
    return 0;
}
int loco_asyrp_read_param(loco_asyrp* p, const char* name, float* dst, int64_t count) {
    if (!p) return -2;
    return asyrp_read(p, "loco_asyrp_read_param", name, dst, count, p->params);
}
int loco_asyrp_read_grad(loco_asyrp* p, const char* name, float* dst, int64_t count) {
    if (!p) return -2;
    return asyrp_read(p, "loco_asyrp_read_grad", name, dst, count, p->grad);
}

int loco_asyrp_forward(loco_asyrp* p, const float* h_dev, const float* e_dev, int32_t B, float s, float* dh_dev, int32_t keep_records, void* stream) {
    if (!p) return -2;
    if (!h_dev || !e_dev || !dh_dev) return p->fail("loco_asyrp_forward: null argument");
    if (B < 1 || B > p->max_batch) return p->fail("loco_asyrp_forward: B = " + std::to_string(B) + " is outside [1, max_batch = " + std::to_string(p->max_batch) + "]");
    std::string m;
    if (p->table.missing(m)) return p->fail("loco_asyrp_forward: " + m);
    DeviceGuard dg(p->device);
    hipStream_t st = (hipStream_t)stream;
    const int C = p->C, HW = p->H * p->W, cpg = C / ASYRP_GROUPS;
    const long N = (long)B * HW;
    const unsigned eb = blocks256((long)C * N);
    p->rec_B = 0;
    hipLaunchKernelGGL(asyrp_pack_kernel, dim3(eb), dim3(256), 0, st, h_dev, 1.0f, C, HW, (int)B, p->hc);
    hipLaunchKernelGGL(asyrp_time_kernel, dim3((C + 3) / 4), dim3(256), 0, st, p->Wt, p->ct, p->c1, p->c2, e_dev, p->E, C, s, p->se, p->bias1, p->bias2);
    hipLaunchKernelGGL(asyrp_gn_stats_kernel, dim3(ASYRP_GROUPS, B), dim3(256), 0, st, p->hc, HW, N, cpg, (double)p->eps, p->st1);
    hipLaunchKernelGGL(asyrp_gn_act_kernel, dim3(eb), dim3(256), 0, st, p->hc, p->st1, p->g1, p->b1, C, HW, N, cpg, p->a1);
    asyrp_gemm(p->W1, C, 1, p->a1, N, 1, C, (int)N, C, 1.f, 0.f, p->bias1, p->y1, N, 0, (int)N, st);
    hipLaunchKernelGGL(asyrp_gn_stats_kernel, dim3(ASYRP_GROUPS, B), dim3(256), 0, st, p->y1, HW, N, cpg, (double)p->eps, p->st2);
    hipLaunchKernelGGL(asyrp_gn_act_kernel, dim3(eb), dim3(256), 0, st, p->y1, p->st2, p->g2, p->b2, C, HW, N, cpg, p->a2);
    asyrp_gemm(p->W2, C, 1, p->a2, N, 1, C, (int)N, C, s, 0.f, p->bias2, dh_dev, HW, (long)C * HW, HW, st);
    if (!asyrp_ok(p, hipGetLastError(), "loco_asyrp_forward: launch")) return -1;
    if (keep_records) { p->rec_B = B; p->rec_s = s; }
    return 0;
}

int loco_asyrp_backward(loco_asyrp* p, const float* g_dh_dev, int32_t B, float* g_h_dev, void* stream) {
    if (!p) return -2;
    if (!g_dh_dev) return p->fail("loco_asyrp_backward: null argument");
    if (p->rec_B < 1) return p->fail("loco_asyrp_backward: no records (run loco_asyrp_forward with keep_records first)");
    if (B != p->rec_B) return p->fail("loco_asyrp_backward: B = " + std::to_string(B) + ", the records are of a forward with B = " + std::to_string(p->rec_B));
    DeviceGuard dg(p->device);
    hipStream_t st = (hipStream_t)stream;
    const int C = p->C, HW = p->H * p->W, cpg = C / ASYRP_GROUPS, E = p->E;
    const long N = (long)B * HW;
    const unsigned eb = blocks256((long)C * N), cb4 = (unsigned)((C + 3) / 4), cb = blocks256(C);
    float *go = p->t0, *ga = p->t1, *gy1 = p->t0;
    // o = W2 a2 + c2, dh = s o
    hipLaunchKernelGGL(asyrp_pack_kernel, dim3(eb), dim3(256), 0, st, g_dh_dev, p->rec_s, C, HW, (int)B, go);
    hipLaunchKernelGGL(asyrp_bias_grad_kernel, dim3(cb4), dim3(256), 0, st, go, C, N, p->gp(p->c2), (float*)nullptr, (double*)nullptr);
    asyrp_gemm(go, N, 1, p->a2, 1, N, C, C, (int)N, 1.f, 1.f, nullptr, p->gp(p->W2), C, 0, C, st);             // dW2 += go a2^T
    asyrp_gemm(p->W2, 1, C, go, N, 1, C, (int)N, C, 1.f, 0.f, nullptr, ga, N, 0, (int)N, st);                   // g_a2 = W2^T go
    // a2 = swish(GroupNorm(y1))
    hipLaunchKernelGGL(asyrp_gn_bwd_sums_kernel, dim3(ASYRP_GROUPS, B), dim3(256), 0, st, ga, p->y1, p->st2, p->g2, p->b2, C, HW, N, cpg, p->S, p->tst);
    hipLaunchKernelGGL(asyrp_gn_param_grad_kernel, dim3(cb), dim3(256), 0, st, p->S, (int)B, C, p->gp(p->g2), p->gp(p->b2));
    hipLaunchKernelGGL(asyrp_gn_bwd_apply_kernel, dim3(eb), dim3(256), 0, st, ga, p->y1, p->st2, p->g2, p->b2, p->tst, C, HW, N, cpg, gy1, N, 0L, N);
    // y1 = W1 a1 + c1 + Wt swish(e) + ct
    hipLaunchKernelGGL(asyrp_bias_grad_kernel, dim3(cb4), dim3(256), 0, st, gy1, C, N, p->gp(p->c1), p->gp(p->ct), p->rs);
    hipLaunchKernelGGL(asyrp_outer_kernel, dim3(blocks256((long)C * E)), dim3(256), 0, st, p->rs, p->se, C, E, p->gp(p->Wt));
    asyrp_gemm(gy1, N, 1, p->a1, 1, N, C, C, (int)N, 1.f, 1.f, nullptr, p->gp(p->W1), C, 0, C, st);             // dW1 += g_y1 a1^T
    asyrp_gemm(p->W1, 1, C, gy1, N, 1, C, (int)N, C, 1.f, 0.f, nullptr, ga, N, 0, (int)N, st);                  // g_a1 = W1^T g_y1
    // a1 = swish(GroupNorm(h))
    hipLaunchKernelGGL(asyrp_gn_bwd_sums_kernel, dim3(ASYRP_GROUPS, B), dim3(256), 0, st, ga, p->hc, p->st1, p->g1, p->b1, C, HW, N, cpg, p->S, p->tst);
    hipLaunchKernelGGL(asyrp_gn_param_grad_kernel, dim3(cb), dim3(256), 0, st, p->S, (int)B, C, p->gp(p->g1), p->gp(p->b1));
    if (g_h_dev)
        hipLaunchKernelGGL(asyrp_gn_bwd_apply_kernel, dim3(eb), dim3(256), 0, st, ga, p->hc, p->st1, p->g1, p->b1, p->tst, C, HW, N, cpg, g_h_dev,
                           (long)HW, (long)C * HW, (long)HW);
    return asyrp_ok(p, hipGetLastError(), "loco_asyrp_backward: launch") ? 0 : -1;
}

int loco_asyrp_zero_grad(loco_asyrp* p, void* stream) {
    if (!p) return -2;
    DeviceGuard dg(p->device);
    return asyrp_ok(p, hipMemsetAsync(p->grad, 0, p->table.total * sizeof(float), (hipStream_t)stream), "loco_asyrp_zero_grad") ? 0 : -1;
}

int loco_asyrp_adam_step(loco_asyrp* p, float lr, float beta1, float beta2, float eps, int32_t step, void* stream) {
    if (!p) return -2;
    if (step < 1) return p->fail("loco_asyrp_adam_step: step counts from 1");
    if (!(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f) || !(eps > 0.f))
        return p->fail("loco_asyrp_adam_step: need 0 <= beta1, beta2 < 1 and eps > 0");
    std::string m;
    if (p->table.missing(m)) return p->fail("loco_asyrp_adam_step: " + m);
    DeviceGuard dg(p->device);
    const double bc1 = 1.0 - std::pow((double)beta1, (double)step), bc2 = 1.0 - std::pow((double)beta2, (double)step);
    const long total = (long)p->table.total;
    hipLaunchKernelGGL(asyrp_adam_kernel, dim3(blocks256(total)), dim3(256), 0, (hipStream_t)stream, p->params, p->grad, p->m, p->v, total,
                       (float)((double)lr / bc1), (float)(1.0 / std::sqrt(bc2)), beta1, beta2, eps);
    return asyrp_ok(p, hipGetLastError(), "loco_asyrp_adam_step: launch") ? 0 : -1;
}

int loco_asyrp_reset_moments(loco_asyrp* p, void* stream) {
    if (!p) return -2;
    DeviceGuard dg(p->device);
    hipStream_t st = (hipStream_t)stream;
    return asyrp_ok(p, hipMemsetAsync(p->m, 0, p->table.total * sizeof(float), st), "loco_asyrp_reset_moments") &&
           asyrp_ok(p, hipMemsetAsync(p->v, 0, p->table.total * sizeof(float), st), "loco_asyrp_reset_moments") ? 0 : -1;
}

const char* loco_asyrp_last_error(loco_asyrp* p) { return p ? p->err.c_str() : g_asyrp_create_err.c_str(); }

void loco_asyrp_destroy(loco_asyrp* p) { delete p; }

}  // extern "C"
