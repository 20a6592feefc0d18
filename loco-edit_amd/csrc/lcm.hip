// The latent-consistency scheduler's update after the denoiser call (diffusers LCMScheduler.step as the reference's
// EditLatentConsistency uses it, src/modules/edit.py:135, 194, 235): predicted x0 from the noise prediction, the
// boundary-condition combination with the sample, and the re-injection of noise at the previous timestep.  One elementwise
// launch over a latent batch (a Stable Diffusion latent is 16 384 floats): what matters is the number of launches -- it
// replaces loco_sched_step + two loco_lincomb and their two intermediates.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "kernels.h"

namespace loco {

namespace {

constexpr int LCM_THREADS = 256;

// fp32, in the operation order of LCMScheduler.step: (x - sqrt(1-a) eps) / sqrt(a); c_out x0 + c_skip x;
// sqrt(a_prev) den + sqrt(1-a_prev) noise.  (c_skip, c_out) = (1, 0) returns x exactly.
__device__ __forceinline__ float lcm_denoised(float x, float e, float sat, float s1mat, float c_skip, float c_out) {
    const float x0 = (x - s1mat * e) / sat;
    return c_out * x0 + c_skip * x;
}

// NOISE: prev = satp den + s1matp noise, else prev = den.  V = 4: 16-byte loads / stores (count % 4 == 0, aligned tensors).
template <int V, bool NOISE>
__global__ void __launch_bounds__(LCM_THREADS)
lcm_step_kernel(const float* x, const float* __restrict__ eps, const float* __restrict__ noise, float* prev, float* den,
                long count, float sat, float s1mat, float satp, float s1matp, float c_skip, float c_out) {
    // x / prev / den without __restrict__: prev may alias x (each thread reads its elements before it writes them)
    for (long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * V; i < count; i += (long)gridDim.x * blockDim.x * V) {
        if constexpr (V == 4) {
            const float4 x4 = *reinterpret_cast<const float4*>(x + i);
            const float4 e4 = *reinterpret_cast<const float4*>(eps + i);
            float4 d, p;
            d.x = lcm_denoised(x4.x, e4.x, sat, s1mat, c_skip, c_out);
            d.y = lcm_denoised(x4.y, e4.y, sat, s1mat, c_skip, c_out);
            d.z = lcm_denoised(x4.z, e4.z, sat, s1mat, c_skip, c_out);
            d.w = lcm_denoised(x4.w, e4.w, sat, s1mat, c_skip, c_out);
            p = d;
            if constexpr (NOISE) {
                const float4 n4 = *reinterpret_cast<const float4*>(noise + i);
                p.x = satp * d.x + s1matp * n4.x; p.y = satp * d.y + s1matp * n4.y;
                p.z = satp * d.z + s1matp * n4.z; p.w = satp * d.w + s1matp * n4.w;
            }
            if (den) *reinterpret_cast<float4*>(den + i) = d;
            if (prev) *reinterpret_cast<float4*>(prev + i) = p;
        } else {
            const float d = lcm_denoised(x[i], eps[i], sat, s1mat, c_skip, c_out);
            float p = d;
            if constexpr (NOISE) p = satp * d + s1matp * noise[i];
            if (den) den[i] = d;
            if (prev) prev[i] = p;
        }
    }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }   // nullptr counts as aligned

template <int V>
void launch_v(const float* x, const float* eps, const float* noise, float* prev, float* den, long count, float sat, float s1mat,
              float satp, float s1matp, float c_skip, float c_out, hipStream_t st) {
    long blocks = ((count + V - 1) / V + LCM_THREADS - 1) / LCM_THREADS;
    if (blocks > 2048) blocks = 2048;
    if (noise)
        hipLaunchKernelGGL((lcm_step_kernel<V, true>), dim3((int)blocks), dim3(LCM_THREADS), 0, st, x, eps, noise, prev, den, count,
                           sat, s1mat, satp, s1matp, c_skip, c_out);
    else
        hipLaunchKernelGGL((lcm_step_kernel<V, false>), dim3((int)blocks), dim3(LCM_THREADS), 0, st, x, eps, noise, prev, den, count,
                           sat, s1mat, satp, s1matp, c_skip, c_out);
}

}  // namespace

void launch_lcm_step(const float* x, const float* eps, const float* noise, float* prev, float* den, long count, float sat,
                     float s1mat, float satp, float s1matp, float c_skip, float c_out, hipStream_t st) {
    const bool vec = (count % 4 == 0) && aligned16(x) && aligned16(eps) && aligned16(noise) && aligned16(prev) && aligned16(den);
    if (vec) launch_v<4>(x, eps, noise, prev, den, count, sat, s1mat, satp, s1matp, c_skip, c_out, st);
    else launch_v<1>(x, eps, noise, prev, den, count, sat, s1mat, satp, s1matp, c_skip, c_out, st);
}

}  // namespace loco
