// The kernels the ViT encoders share (declared in encoder_common.h): the streamed attention of samenc.hip (with the relative
// position tables) and clipvis.hip (without, optionally keeping the softmax statistics), the patch gather of both, and the
// transpose of channel-major results that the text encoders use too.  Exact fp32; every sum runs in a fixed order set by
// compile-time constants.
#include "enc_attn_launch.h"

#include <cmath>

namespace loco {
namespace {

// One workgroup per (query block of 16, head, group): the nk keys of the group -- a window or the whole map of SAM, an image
// of CLIP, at columns group * nk + [0, nk) -- are streamed in order in chunks of 64, K [hd][64] and V [64][hd + 1] of the chunk
// in LDS.  A wave owns 4 queries; lane j scores key k0 + j against them, (q scale) . k, then the running max / sum update
// (fp32, max and sum over the chunk by shuffles), then lane c (and c + 64) adds P V of the chunk to its output channel in
// key order.  qkv: [3 D][ld] = q | k | v channel rows, out [D][ld]; hd <= 128.
// BIAS: the score of key (kr, kc) of a size x size group gains relh[q][kr] + relw[q][kc] (tables [heads][Tall][size], staged
// for the 16 queries).  KEEP: the row max and the row sum of every query go to ml [2][heads][ld]; the arithmetic is the same.
template <bool BIAS, bool KEEP>
__global__ __launch_bounds__(ENC_ATTN_THREADS) void enc_attn_kernel(const float* qkv, long ld, int D, int hd, int nk, int size, float scale,
                                                                    const float* relh, const float* relw, long Tall, float* out,
                                                                    float* ml) {
    constexpr int THREADS = ENC_ATTN_THREADS, QW = ENC_ATTN_QW, QB = ENC_ATTN_QB, KC = ENC_ATTN_KC;
    extern __shared__ __align__(16) float enc_sm[];
    const int hdp = hd + 1;
    float* Ks = enc_sm;                                    // [hd][64]
    float* Vs = Ks + enc_r4(hd * KC);                      // [64][hd + 1]
    float* Qs = Vs + enc_r4(KC * hdp);                     // [hd][16]
    const int tsize = BIAS ? size : 0;                     // no tables: Ps starts where Bh would
    float* Bh = Qs + enc_r4(hd * QB);                      // [16][size]
    float* Bw = Bh + QB * tsize;                           // [16][size]
    float* Ps = Bh + enc_r4(2 * QB * tsize);               // [waves][64][4]
    const int qb = blockIdx.x, h = blockIdx.y, w = blockIdx.z;
    const long col0 = (long)w * nk;
    const int q0 = qb * QB;
    const float* q = qkv + (long)(h * hd) * ld + col0;
    const float* k = qkv + (long)(D + h * hd) * ld + col0;
    const float* v = qkv + (long)(2 * D + h * hd) * ld + col0;
    for (int e = threadIdx.x; e < hd * QB; e += THREADS) {
        const int c = e / QB, ql = min(q0 + e % QB, nk - 1);
        Qs[e] = q[(long)c * ld + ql] * scale;
    }
    if constexpr (BIAS) {
        for (int e = threadIdx.x; e < QB * size; e += THREADS) {
            const int ql = min(q0 + e / size, nk - 1), j = e % size;
            const long o = ((long)h * Tall + col0 + ql) * size + j;
            Bh[e] = relh[o];
            Bw[e] = relw[o];
        }
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int c0 = lane < hd ? lane : 0, c1 = lane + 64 < hd ? lane + 64 : 0;
    float* pw = Ps + wv * (KC * QW);
    float m[QW], l[QW], o0[QW], o1[QW];
#pragma unroll
    for (int u = 0; u < QW; ++u) { m[u] = -INFINITY; l[u] = 0.f; o0[u] = 0.f; o1[u] = 0.f; }
    for (int k0 = 0; k0 < nk; k0 += KC) {
        __syncthreads();
        for (int e = threadIdx.x; e < hd * KC; e += THREADS) {
            const int c = e / KC, j = e % KC, kj = k0 + j;
            const bool ok = kj < nk;
            Ks[e] = ok ? k[(long)c * ld + kj] : 0.f;
            Vs[j * hdp + c] = ok ? v[(long)c * ld + kj] : 0.f;
        }
        __syncthreads();
        const int kj = k0 + lane;
        const bool valid = kj < nk;
        int kr = 0, kc = 0;
        if constexpr (BIAS) {
            kr = valid ? kj / size : 0;
            kc = valid ? kj - kr * size : 0;
        }
        float s[QW];
#pragma unroll
        for (int u = 0; u < QW; ++u) s[u] = 0.f;
        for (int c = 0; c < hd; ++c) {
            const float kv = Ks[c * KC + lane];
            const float4 qv = *reinterpret_cast<const float4*>(Qs + c * QB + wv * QW);
            s[0] = fmaf(qv.x, kv, s[0]);
            s[1] = fmaf(qv.y, kv, s[1]);
            s[2] = fmaf(qv.z, kv, s[2]);
            s[3] = fmaf(qv.w, kv, s[3]);
        }
#pragma unroll
        for (int u = 0; u < QW; ++u) {
            float sc = -INFINITY;                          // key k0 is always live: the chunk's max is finite
            if constexpr (BIAS) {
                const int qi = wv * QW + u;
                if (valid) sc = s[u] + Bh[qi * size + kr] + Bw[qi * size + kc];
            } else {
                if (valid) sc = s[u];
            }
            const float mn = fmaxf(m[u], wave_max(sc));
            const float corr = expf(m[u] - mn);
            const float p = valid ? expf(sc - mn) : 0.f;
            l[u] = l[u] * corr + wave_sum(p);
            o0[u] *= corr;
            o1[u] *= corr;
            m[u] = mn;
            pw[lane * QW + u] = p;
        }
        __syncthreads();
        for (int j = 0; j < KC; ++j) {
            const float4 pv = *reinterpret_cast<const float4*>(pw + j * QW);
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
    for (int u = 0; u < QW; ++u) {
        const int ql = q0 + wv * QW + u;
        if (ql >= nk) continue;
        const float inv = 1.0f / l[u];
        if (lane < hd) out[(long)(h * hd + lane) * ld + col0 + ql] = o0[u] * inv;
        if (lane + 64 < hd) out[(long)(h * hd + lane + 64) * ld + col0 + ql] = o1[u] * inv;
        if constexpr (KEEP) {
            if (lane == 0) {
                ml[(long)h * ld + col0 + ql] = m[u];
                ml[(long)(gridDim.y + h) * ld + col0 + ql] = l[u];
            }
        }
    }
}

// P[(ci ps + ky) ps + kx][i T + cls + ty G + tx] = pix[i][ci][ty ps + ky][tx ps + kx], T = cls + G^2; 0 in the class and the
// padding columns
__global__ __launch_bounds__(256) void enc_patch_kernel(const float* pix, int S, int ps, int G, int cls, int T, int nT, int Tp, float* P) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)3 * ps * ps * Tp) return;
    const int r = (int)(e / Tp), col = (int)(e % Tp);
    float v = 0.f;
    const int i = col / T, t = col % T;
    if (col < nT && t >= cls) {
        const int ci = r / (ps * ps), ky = (r / ps) % ps, kx = r % ps, ty = (t - cls) / G, tx = (t - cls) % G;
        v = pix[(((long)i * 3 + ci) * S + ty * ps + ky) * S + tx * ps + kx];
    }
    P[e] = v;
}

__global__ __launch_bounds__(256) void enc_transpose_kernel(const float* x, int ld, int cols, int C, float* out) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)cols * C) return;
    const int col = (int)(e / C), c = (int)(e % C);
    out[e] = x[(long)c * ld + col];
}

}  // namespace

void launch_enc_attn(const EncAttnArgs& a, hipStream_t st) {
    const bool bias = enc_attn_bias(a);
    auto kernel = bias ? enc_attn_kernel<true, false> : enc_attn_keep(a) ? enc_attn_kernel<false, true> : enc_attn_kernel<false, false>;
    const int size = bias ? a.size : 0;
    hipLaunchKernelGGL(kernel, dim3((a.nk + ENC_ATTN_QB - 1) / ENC_ATTN_QB, a.heads, a.groups), dim3(ENC_ATTN_THREADS),
                       enc_attn_lds_floats(a.hd, size) * sizeof(float), st, a.qkv, a.ld, a.D, a.hd, a.nk, size, a.scale, a.relh, a.relw, a.Tall,
                       a.out, a.ml);
}

void launch_enc_patch(const float* pix, int n, int S, int ps, int G, int cls, int Tp, float* P, hipStream_t st) {
    const int T = cls + G * G;
    hipLaunchKernelGGL(enc_patch_kernel, dim3(blocks256((long)3 * ps * ps * Tp)), dim3(256), 0, st, pix, S, ps, G, cls, T, n * T, Tp, P);
}

void launch_enc_transpose(const float* x, int ld, int cols, int C, float* out, hipStream_t st) {
    hipLaunchKernelGGL(enc_transpose_kernel, dim3(blocks256((long)cols * C)), dim3(256), 0, st, x, ld, cols, C, out);
}

}  // namespace loco
