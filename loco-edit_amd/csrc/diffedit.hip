// DiffEdit on the DeepFloyd-IF path: the mask derived from two guided noise predictions (reference
// src/modules/edit.py:1395-1407 `mask_diffedit`, lines 1401-1402) and one step of the masked sampler
// (`MaskedDDPMforwardsteps` :1540-1548).  Both are elementwise / small-reduction kernels around denoiser evaluations
// that exist already; an IF frame is 12 288 floats, so what matters is the number of launches, not the bandwidth.
#include <hip/hip_runtime.h>
#include <cfloat>
#include <cstdint>
#include "kernels.h"

namespace loco {

namespace {

constexpr int DE_THREADS = 256;
constexpr int DE_MAX_BLOCKS = 256;      // partials the threshold kernel re-reduces in one pass of one block

// m[p] = mean_c( mean_b( scale (a[b,c,p] - b[b,c,p]) ) ): batch first, then channels, the order of the reference's two
// .mean calls (edit.py:1401).  One thread owns V adjacent pixels and sums in that fixed order: the map does not depend on
// the launch geometry.  V = 4: 16-byte loads (HW % 4 == 0 and 16-byte aligned tensors), V = 1 otherwise.
// part[3 blk + {0,1,2}] = {min, max, non-finite flag} of the block's pixels (wave shuffle -> LDS -> one value per block).
template <int V>
__global__ void __launch_bounds__(DE_THREADS)
diffedit_map_kernel(const float* __restrict__ ea, const float* __restrict__ eb, float scale, int B, int C, long HW,
                    float* __restrict__ m, float* __restrict__ part) {
    const float rB = 1.0f / (float)B, rC = 1.0f / (float)C;
    float mn = FLT_MAX, mx = -FLT_MAX, bad = 0.f;
    for (long p = ((long)blockIdx.x * blockDim.x + threadIdx.x) * V; p < HW; p += (long)gridDim.x * blockDim.x * V) {
        float acc[V];
#pragma unroll
        for (int j = 0; j < V; ++j) acc[j] = 0.f;
        for (int c = 0; c < C; ++c) {
            float sb[V];
#pragma unroll
            for (int j = 0; j < V; ++j) sb[j] = 0.f;
            for (int b = 0; b < B; ++b) {
                const long off = ((long)b * C + c) * HW + p;
                if constexpr (V == 4) {
                    const float4 a4 = *reinterpret_cast<const float4*>(ea + off);
                    const float4 b4 = *reinterpret_cast<const float4*>(eb + off);
                    sb[0] += scale * (a4.x - b4.x); sb[1] += scale * (a4.y - b4.y);
                    sb[2] += scale * (a4.z - b4.z); sb[3] += scale * (a4.w - b4.w);
                } else {
                    sb[0] += scale * (ea[off] - eb[off]);
                }
            }
#pragma unroll
            for (int j = 0; j < V; ++j) acc[j] += sb[j] * rB;
        }
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float v = acc[j] * rC;
            m[p + j] = v;
            if (fabsf(v) <= FLT_MAX) { mn = fminf(mn, v); mx = fmaxf(mx, v); } else bad = 1.f;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, o, 64));
        mx = fmaxf(mx, __shfl_xor(mx, o, 64));
        bad = fmaxf(bad, __shfl_xor(bad, o, 64));
    }
    __shared__ float red[3][DE_THREADS / 64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) { red[0][wave] = mn; red[1][wave] = mx; red[2][wave] = bad; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < DE_THREADS / 64; ++w) {
            mn = fminf(mn, red[0][w]); mx = fmaxf(mx, red[1][w]); bad = fmaxf(bad, red[2][w]);
        }
        part[3 * blockIdx.x + 0] = mn; part[3 * blockIdx.x + 1] = mx; part[3 * blockIdx.x + 2] = bad;
    }
}

// Second launch: every block reduces the <= DE_MAX_BLOCKS partials again (min / max are order-independent, so every block
// holds the same two numbers), then thresholds its pixels.
//   rule 0 "reference": z = m - min / (max - min), mask = round_half_even(z) != 0, i.e. |z| > 0.5   (edit.py:1402 as written)
//   rule 1 "intended":  z = (m - min) / (max - min), mask = z > 0.5
// status[0] = 0 fine, 1 constant map (max == min: the reference divides by zero here), 2 non-finite map; the mask is all
// zero then.  status[1..2] = min, max.
__global__ void __launch_bounds__(DE_THREADS)
diffedit_threshold_kernel(const float* __restrict__ m, const float* __restrict__ part, int nblk, long HW, int rule,
                          uint8_t* __restrict__ mask, float* __restrict__ status) {
    float mn = FLT_MAX, mx = -FLT_MAX, bad = 0.f;
    for (int i = threadIdx.x; i < nblk; i += blockDim.x) {
        mn = fminf(mn, part[3 * i]); mx = fmaxf(mx, part[3 * i + 1]); bad = fmaxf(bad, part[3 * i + 2]);
    }
    for (int o = 32; o > 0; o >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, o, 64));
        mx = fmaxf(mx, __shfl_xor(mx, o, 64));
        bad = fmaxf(bad, __shfl_xor(bad, o, 64));
    }
    __shared__ float red[3][DE_THREADS / 64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) { red[0][wave] = mn; red[1][wave] = mx; red[2][wave] = bad; }
    __syncthreads();
    mn = red[0][0]; mx = red[1][0]; bad = red[2][0];
    for (int w = 1; w < DE_THREADS / 64; ++w) {
        mn = fminf(mn, red[0][w]); mx = fmaxf(mx, red[1][w]); bad = fmaxf(bad, red[2][w]);
    }
    const int st = bad != 0.f ? 2 : (mx > mn ? 0 : 1);
    if (blockIdx.x == 0 && threadIdx.x == 0) { status[0] = (float)st; status[1] = mn; status[2] = mx; }
    const float range = mx - mn;
    const float cst = mn / range;
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < HW; p += (long)gridDim.x * blockDim.x) {
        const float v = m[p];
        bool on;
        if (rule == 0) on = fabsf(v - cst) > 0.5f;
        else on = (v - mn) / range > 0.5f;
        mask[p] = (st == 0 && on) ? 1 : 0;
    }
}

// One step of the masked sampler after the denoiser calls (edit.py:1540-1548), per element and in the reference's operation
// order: eF = n + g (f - n), eE = n + g (e - n) (edit.py:1336 / 1341: `guidance_scale` for both), each through the eta = 0
// DDIM update as ddim_step_kernel writes it, result = mask ? xE : xF.  A select, not a product with 0 / 1: a NaN / Inf of the
// half that is not taken must not reach the frame (masked_axpby_kernel).  mask: uint8 [n], broadcast over the batch.
__device__ __forceinline__ float masked_step_one(float x, float f, float e, float nn, uint8_t mk, float g, float sq1mat,
                                                 float sqat, float sqatn, float ce) {
    const float eF = nn + g * (f - nn);
    const float eE = nn + g * (e - nn);
    const float pF = (x - eF * sq1mat) / sqat;
    const float pE = (x - eE * sq1mat) / sqat;
    const float vF = sqatn * pF + ce * eF;
    const float vE = sqatn * pE + ce * eE;
    return mk ? vE : vF;
}

template <int V>
__global__ void __launch_bounds__(DE_THREADS)
cfg_masked_step_kernel(const float* x, const float* __restrict__ ef, const float* __restrict__ ee,
                       const float* __restrict__ en, const uint8_t* __restrict__ mask, float* out, long n, long total,
                       float g, float sq1mat, float sqat, float sqatn, float ce) {
    // x / out without __restrict__: the output may alias x (each thread reads its elements before it writes them)
    for (long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * V; i < total; i += (long)gridDim.x * blockDim.x * V) {
        const long j = i % n;               // V == 4: n % 4 == 0, so the four elements share a frame
        if constexpr (V == 4) {
            const float4 x4 = *reinterpret_cast<const float4*>(x + i);
            const float4 f4 = *reinterpret_cast<const float4*>(ef + i);
            const float4 e4 = *reinterpret_cast<const float4*>(ee + i);
            const float4 n4 = *reinterpret_cast<const float4*>(en + i);
            const uchar4 m4 = *reinterpret_cast<const uchar4*>(mask + j);
            float4 o;
            o.x = masked_step_one(x4.x, f4.x, e4.x, n4.x, m4.x, g, sq1mat, sqat, sqatn, ce);
            o.y = masked_step_one(x4.y, f4.y, e4.y, n4.y, m4.y, g, sq1mat, sqat, sqatn, ce);
            o.z = masked_step_one(x4.z, f4.z, e4.z, n4.z, m4.z, g, sq1mat, sqat, sqatn, ce);
            o.w = masked_step_one(x4.w, f4.w, e4.w, n4.w, m4.w, g, sq1mat, sqat, sqatn, ce);
            *reinterpret_cast<float4*>(out + i) = o;
        } else {
            out[i] = masked_step_one(x[i], ef[i], ee[i], en[i], mask[j], g, sq1mat, sqat, sqatn, ce);
        }
    }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

int diffedit_map_blocks(long HW) {
    long blocks = (HW + DE_THREADS - 1) / DE_THREADS;
    if (blocks > DE_MAX_BLOCKS) blocks = DE_MAX_BLOCKS;
    return blocks < 1 ? 1 : (int)blocks;
}

void launch_diffedit_mask(const float* eps_a, const float* eps_b, float scale, int B, int C, long HW, int rule, float* m,
                          uint8_t* mask, float* part, float* status, hipStream_t st) {
    const bool vec = (HW % 4 == 0) && aligned16(eps_a) && aligned16(eps_b) && aligned16(m);
    int blocks;
    if (vec) {
        long b4 = (HW / 4 + DE_THREADS - 1) / DE_THREADS;
        blocks = (int)(b4 > DE_MAX_BLOCKS ? DE_MAX_BLOCKS : b4);
        hipLaunchKernelGGL(diffedit_map_kernel<4>, dim3(blocks), dim3(DE_THREADS), 0, st, eps_a, eps_b, scale, B, C, HW, m, part);
    } else {
        blocks = diffedit_map_blocks(HW);
        hipLaunchKernelGGL(diffedit_map_kernel<1>, dim3(blocks), dim3(DE_THREADS), 0, st, eps_a, eps_b, scale, B, C, HW, m, part);
    }
    hipLaunchKernelGGL(diffedit_threshold_kernel, dim3(diffedit_map_blocks(HW)), dim3(DE_THREADS), 0, st, m, part, blocks, HW,
                       rule, mask, status);
}

void launch_cfg_masked_step(const float* x, const float* ef, const float* ee, const float* en, const uint8_t* mask, float* out,
                            int B, long n, float g, float c_x0_x, float c_x0_e, float c_next_x0, float c_next_e,
                            hipStream_t st) {
    const long total = (long)B * n;
    const bool vec = (n % 4 == 0) && aligned16(x) && aligned16(ef) && aligned16(ee) && aligned16(en) && aligned16(out) &&
                     (reinterpret_cast<uintptr_t>(mask) & 3) == 0;
    if (vec) {
        long blocks = (total / 4 + DE_THREADS - 1) / DE_THREADS;
        if (blocks > 2048) blocks = 2048;
        hipLaunchKernelGGL(cfg_masked_step_kernel<4>, dim3((int)blocks), dim3(DE_THREADS), 0, st, x, ef, ee, en, mask, out, n,
                           total, g, c_x0_e, c_x0_x, c_next_x0, c_next_e);
    } else {
        long blocks = (total + DE_THREADS - 1) / DE_THREADS;
        if (blocks > 2048) blocks = 2048;
        hipLaunchKernelGGL(cfg_masked_step_kernel<1>, dim3((int)blocks), dim3(DE_THREADS), 0, st, x, ef, ee, en, mask, out, n,
                           total, g, c_x0_e, c_x0_x, c_next_x0, c_next_e);
    }
}

}  // namespace loco
