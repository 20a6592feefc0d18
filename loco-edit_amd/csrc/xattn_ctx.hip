// Cotangent of a text cross-attention stage with respect to the projected prompt states (loco_pmp_vjp_context: the gradient
// of the denoiser output with respect to the encoder states of loco_set_context).  With the cotangent pass's g_o [C][T], the
// primal P [NH][T][Lp] and the primal q [C][T] of one stage (xattn.hip: o = V P^T, P = softmax_l(scale q^T K)),
//     R = scale P o (g_o^T V - <P, g_o^T V>)          (the row operation of the cotangent, as xattn_fused_kernel<.., false>)
//     g_V[c][l] = sum_t g_o[c][t] P[t][l]             g_K[c][l] = sum_t q[c][t] R[t][l]
// Both products contract over the tokens: T = 4096 at the largest Stable Diffusion level against an output of 40 x 77 per
// head, so the token contraction is the whole cost and is what the grid is cut along.  A workgroup owns 64 tokens of one
// (probe, head), laid out like xattn_fused_kernel: V of the head in LDS, a token's score row over 4 adjacent lanes, R by the
// forward's own chain of FMAs.  R and P rows then go to LDS token-major, the q / g_o tiles sit there channel-major, and the
// workgroup contracts both products over its tokens -- a thread owns a 4 channel x 4 column tile of each, tokens in order --
// and writes one partial [2][CH][4 LG] per token block.  xattn_ctx_reduce_kernel adds the partials of a (probe, head) in block
// order.  Exact fp32 VALU in every arithmetic mode, no atomics, every sum in a fixed order: a probe's row does not depend on
// the batch around it.
// Where the partials would not fit the workspace a workgroup walks `walk` consecutive token blocks and adds each block's sum
// to the partial it wrote for the previous one (same thread, same address).
// The engine calls this with one probe (loco_pmp_vjp_context takes the rows of G from single-probe passes); the probe index
// (blockIdx.z, go_bs, out_bs) is kept for a batched G and is exercised by no caller and no test.
#include <algorithm>

#include "kernels.h"

namespace loco {

namespace {

constexpr int XC_TOK = 64;            // tokens per block (256 threads = 64 tokens x 4 column groups)
constexpr int XC_QS = XC_TOK + 4;     // row stride of the channel-major q / g_o tiles: 16-byte aligned rows, 4 banks apart

struct XCtxLds { size_t v, go, q, r, p, total; bool alias; };      // offsets in floats
// V [CH][LW] is read by the score phase only and the q tile [CH][XC_QS] by the contraction only: they share one region when
// keeping both would leave less than two workgroups per CU (80 KB each; the wide heads of the small levels: CH = 80, 160)
XCtxLds xctx_lds(int CH, int LG) {
    const size_t LW = 4 * (size_t)LG, RS = LW + 4;
    XCtxLds o;
    const size_t fixed = (size_t)CH * XC_QS + 2 * XC_TOK * RS;
    o.alias = ((size_t)CH * LW + (size_t)CH * XC_QS + fixed) * sizeof(float) > 80 * 1024;
    o.v = 0;
    const size_t a = o.alias ? (size_t)CH * std::max<size_t>(LW, XC_QS) : (size_t)CH * LW;
    o.go = a;
    o.q = o.alias ? 0 : o.go + (size_t)CH * XC_QS;
    o.r = (o.alias ? o.go : o.q) + (size_t)CH * XC_QS;
    o.p = o.r + XC_TOK * RS;
    o.total = o.p + XC_TOK * RS;
    return o;
}

template <int LG>
__global__ __launch_bounds__(256) void xattn_ctx_kernel(XCtxArgs a, int o_go, int o_q, int o_r, int alias) {
    extern __shared__ __attribute__((aligned(16))) float xc_sm[];
    constexpr int LW = 4 * LG, RS = LW + 4, QS = XC_QS;
    const int CH = a.CH;
    float* const Vs = xc_sm;                 // [CH][LW], columns >= L zero
    float* const gos = xc_sm + o_go;         // [CH][QS]
    float* const qs = xc_sm + o_q;           // [CH][QS]  (alias: the V region)
    float* const Rs = xc_sm + o_r;           // [64][RS]
    float* const Ps = Rs + XC_TOK * RS;      // [64][RS]
    const int tid = threadIdx.x, g = tid & 3, tl = tid >> 2;
    const int chunk = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int nblk = a.T / XC_TOK;
    const float* gop = a.go + (long)b * a.go_bs + (long)h * CH * a.T;
    const float* qp = a.q + (long)h * CH * a.T;
    float* part = a.part + (((long)b * a.NH + h) * a.nchunk + chunk) * 2L * CH * LW;
    for (int w = 0; w < a.walk; ++w) {
        const int blk = chunk * a.walk + w;
        if (blk >= nblk) break;               // (uniform over the workgroup)
        const int t0 = blk * XC_TOK;
        if (w == 0 || alias) {
            for (int e = tid; e < CH * LW; e += 256) {
                const int c = e / LW, l = e - c * LW;
                Vs[e] = l < a.L ? a.V[(long)(h * CH + c) * a.Lp + l] : 0.f;
            }
        }
        for (int e = tid; e < CH * XC_TOK; e += 256) {
            const int c = e >> 6, tt = e & 63;
            gos[c * QS + tt] = gop[(long)c * a.T + t0 + tt];
            if (!alias) qs[c * QS + tt] = qp[(long)c * a.T + t0 + tt];
        }
        __syncthreads();
        {   // ---- R and P rows of this block's tokens -> LDS (the chain of xattn_fused_kernel's cotangent form)
            float S[LG], P[LG];
#pragma unroll
            for (int j = 0; j < LG; ++j) S[j] = 0.f;
            for (int c = 0; c < CH; ++c) {
                const float x = gos[c * QS + tl];
                const float4* kr = reinterpret_cast<const float4*>(Vs + c * LW + g * LG);
#pragma unroll
                for (int j = 0; j < LG / 4; ++j) {
                    const float4 k = kr[j];
                    S[4 * j] = fmaf(x, k.x, S[4 * j]); S[4 * j + 1] = fmaf(x, k.y, S[4 * j + 1]);
                    S[4 * j + 2] = fmaf(x, k.z, S[4 * j + 2]); S[4 * j + 3] = fmaf(x, k.w, S[4 * j + 3]);
                }
            }
            const float* prow = a.P + ((long)h * a.T + t0 + tl) * a.Lp + g * LG;
#pragma unroll
            for (int j = 0; j < LG / 4; ++j) {
                float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
                if (g * LG + 4 * j < a.Lp) p = *reinterpret_cast<const float4*>(prow + 4 * j);
                P[4 * j] = p.x; P[4 * j + 1] = p.y; P[4 * j + 2] = p.z; P[4 * j + 3] = p.w;
            }
            float dot = 0.f;
#pragma unroll
            for (int j = 0; j < LG; ++j) dot = fmaf(P[j], S[j], dot);
            dot += __shfl_xor(dot, 1); dot += __shfl_xor(dot, 2);
#pragma unroll
            for (int j = 0; j < LG; ++j) S[j] = a.alpha * P[j] * (S[j] - dot);
            float4* rr = reinterpret_cast<float4*>(Rs + tl * RS + g * LG);
            float4* pr = reinterpret_cast<float4*>(Ps + tl * RS + g * LG);
#pragma unroll
            for (int j = 0; j < LG / 4; ++j) {
                rr[j] = make_float4(S[4 * j], S[4 * j + 1], S[4 * j + 2], S[4 * j + 3]);
                pr[j] = make_float4(P[4 * j], P[4 * j + 1], P[4 * j + 2], P[4 * j + 3]);
            }
        }
        __syncthreads();
        if (alias) {          // V is spent: its region takes the q tile
            for (int e = tid; e < CH * XC_TOK; e += 256) {
                const int c = e >> 6, tt = e & 63;
                qs[c * QS + tt] = qp[(long)c * a.T + t0 + tt];
            }
            __syncthreads();
        }
        // ---- g_K = q R, g_V = g_o P over the block's tokens: a 4 channel x 4 column tile of both per item
        for (int it = tid; it < (CH / 4) * LG; it += 256) {
            const int c4 = it / LG, lq = it - c4 * LG;
            float aK[4][4], aV[4][4];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) aK[i][j] = aV[i][j] = 0.f;
            for (int tt = 0; tt < XC_TOK; tt += 4) {
                float qv[4][4], gv[4][4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float4 x = *reinterpret_cast<const float4*>(qs + (c4 * 4 + i) * QS + tt);
                    const float4 y = *reinterpret_cast<const float4*>(gos + (c4 * 4 + i) * QS + tt);
                    qv[i][0] = x.x; qv[i][1] = x.y; qv[i][2] = x.z; qv[i][3] = x.w;
                    gv[i][0] = y.x; gv[i][1] = y.y; gv[i][2] = y.z; gv[i][3] = y.w;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float4 r = *reinterpret_cast<const float4*>(Rs + (tt + u) * RS + lq * 4);
                    const float4 p = *reinterpret_cast<const float4*>(Ps + (tt + u) * RS + lq * 4);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        aK[i][0] = fmaf(qv[i][u], r.x, aK[i][0]); aK[i][1] = fmaf(qv[i][u], r.y, aK[i][1]);
                        aK[i][2] = fmaf(qv[i][u], r.z, aK[i][2]); aK[i][3] = fmaf(qv[i][u], r.w, aK[i][3]);
                        aV[i][0] = fmaf(gv[i][u], p.x, aV[i][0]); aV[i][1] = fmaf(gv[i][u], p.y, aV[i][1]);
                        aV[i][2] = fmaf(gv[i][u], p.z, aV[i][2]); aV[i][3] = fmaf(gv[i][u], p.w, aV[i][3]);
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float4* dk = reinterpret_cast<float4*>(part + (long)(c4 * 4 + i) * LW + lq * 4);
                float4* dv = reinterpret_cast<float4*>(part + (long)(CH + c4 * 4 + i) * LW + lq * 4);
                float4 k = make_float4(aK[i][0], aK[i][1], aK[i][2], aK[i][3]);
                float4 v = make_float4(aV[i][0], aV[i][1], aV[i][2], aV[i][3]);
                if (w > 0) {      // a walked block: the sum so far + this block's sum
                    const float4 k0 = *dk, v0 = *dv;
                    k = make_float4(k0.x + k.x, k0.y + k.y, k0.z + k.z, k0.w + k.w);
                    v = make_float4(v0.x + v.x, v0.y + v.y, v0.z + v.z, v0.w + v.w);
                }
                *dk = k; *dv = v;
            }
        }
        __syncthreads();      // the next block's staging overwrites the tiles
    }
}

// out[b][w][h CH + c][l] = sum over the chunks of (b, h), in chunk order, of part[b][h][chunk][w][c][l]   (w: 0 g_K, 1 g_V)
__global__ __launch_bounds__(256) void xattn_ctx_reduce_kernel(const float* part, float* out, long out_bs, int NH, int CH, int LW,
                                                               int nchunk) {
    const long n = 2L * NH * CH * LW;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const int b = blockIdx.y;
    const int l = (int)(e % LW), c = (int)((e / LW) % CH), h = (int)((e / ((long)LW * CH)) % NH), w = (int)(e / ((long)LW * CH * NH));
    const long cs = 2L * CH * LW;
    const float* src = part + ((long)b * NH + h) * nchunk * cs + (long)w * CH * LW + (long)c * LW + l;
    float s = src[0];
    for (int k = 1; k < nchunk; ++k) s += src[k * cs];
    out[(long)b * out_bs + ((long)w * NH * CH + (long)h * CH + c) * LW + l] = s;
}

template <int LG>
void xctx_launch(const XCtxArgs& a, hipStream_t st) {
    const XCtxLds o = xctx_lds(a.CH, LG);
    const size_t lds = o.total * sizeof(float);
    auto k = &xattn_ctx_kernel<LG>;
    if (lds > 64 * 1024) {
        static DeviceOnce once;
        if (first_on_device(once))
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    }
    hipLaunchKernelGGL(k, dim3(a.nchunk, a.NH, a.B), dim3(256), lds, st, a, (int)o.go, (int)o.q, (int)o.r, o.alias ? 1 : 0);
    const long n = 2L * a.NH * a.CH * 4 * LG;
    hipLaunchKernelGGL(xattn_ctx_reduce_kernel, dim3((unsigned)((n + 255) / 256), a.B), dim3(256), 0, st, a.part, a.out, a.out_bs,
                       a.NH, a.CH, 4 * LG, a.nchunk);
}

}  // namespace

bool xattn_ctx_supported(int T, int CH, int L, int Lp) {
    const int lg = xattn_lg(L);
    return lg > 0 && (T % XC_TOK) == 0 && (Lp % 4) == 0 && (CH % 4) == 0 && xctx_lds(CH, lg).total * sizeof(float) <= 160 * 1024;
}

int xattn_ctx_width(int L) { return 4 * xattn_lg(L); }

int xattn_ctx_walk(int T, int NH, int CH, int L, int probes, size_t avail_floats) {
    const size_t LW = (size_t)xattn_ctx_width(L), nblk = (size_t)T / XC_TOK;
    const size_t red = (size_t)probes * 2 * NH * CH * LW;
    for (size_t walk = 1; walk <= nblk; ++walk) {
        const size_t nchunk = (nblk + walk - 1) / walk;
        if (red + (size_t)probes * NH * nchunk * 2 * CH * LW <= avail_floats) return (int)walk;
    }
    return 0;
}

void launch_xattn_ctx(const XCtxArgs& a, hipStream_t st) {
    switch (xattn_lg(a.L)) {
        case 4: xctx_launch<4>(a, st); break;
        case 8: xctx_launch<8>(a, st); break;
        case 12: xctx_launch<12>(a, st); break;
        case 20: xctx_launch<20>(a, st); break;
        default: xctx_launch<32>(a, st); break;
    }
}

}  // namespace loco
