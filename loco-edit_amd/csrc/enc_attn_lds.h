// The geometry of the streamed attention kernel of the ViT encoders (encoder_kernels.hip enc_attn_kernel) and the carve-up of
// its LDS.  Plain C++ (no HIP types): the create functions' 64 KiB refusals and tests/c/enc_attn_lds_check.cpp read it.
#pragma once
#include <cstddef>

namespace loco {

// 256 threads = 4 waves; a wave owns 4 queries, a workgroup 16; the keys are streamed in chunks of 64
constexpr int ENC_ATTN_THREADS = 256, ENC_ATTN_WAVES = ENC_ATTN_THREADS / 64, ENC_ATTN_QW = 4, ENC_ATTN_QB = ENC_ATTN_WAVES * ENC_ATTN_QW,
              ENC_ATTN_KC = 64;

// parts of the LDS start at multiples of 4 floats (float4 reads of Qs and Ps)
constexpr size_t enc_r4(size_t n) { return (n + 3) / 4 * 4; }

// K [hd][64] | V [64][hd + 1] | Q [hd][16] | the two bias tables [16][size] each (size = 0: none) | P [waves][64][4]
constexpr size_t enc_attn_lds_floats(int hd, int size) {
    return enc_r4((size_t)hd * ENC_ATTN_KC) + enc_r4((size_t)ENC_ATTN_KC * (hd + 1)) + enc_r4((size_t)hd * ENC_ATTN_QB) +
           enc_r4((size_t)2 * ENC_ATTN_QB * size) + (size_t)ENC_ATTN_WAVES * ENC_ATTN_KC * ENC_ATTN_QW;
}

}  // namespace loco
