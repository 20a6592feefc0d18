// The launchers of the encoders' hand-written attention kernels beyond launch_enc_attn (encoder_common.h) and
// launch_prompt_attn (textenc.h), with the predicates they branch on and the LDS carve-ups their create functions refuse by.
// The product's call sites and the diagnostics unit (enc_attn_diag.hip, loco_debug_enc_attn) call the same functions, so a
// single launch under test is the product's launch.
#pragma once
#include "encoder_common.h"

namespace loco {

// ---- encoder_kernels.hip: the form of enc_attn_kernel<BIAS, KEEP> that launch_enc_attn takes
inline bool enc_attn_bias(const EncAttnArgs& a) { return a.relh != nullptr; }
inline bool enc_attn_keep(const EncAttnArgs& a) { return !a.relh && a.ml != nullptr; }

// ---- clipvis.hip: the cotangent of the CLIP image tower's attention (the comment above clipvis_attn_cot_q_kernel)
// the carve-ups of the two cotangent kernels at a chunk of `kc` tokens; `tables`: 1 (dS) or 2 (P and dS) per-wave tables
inline size_t clipvis_attn_cot_lds_floats(int hd, int kc, int tables) {
    return 2 * enc_r4((size_t)kc * (hd + 1)) + 2 * enc_r4((size_t)hd * ENC_ATTN_QB) + (size_t)tables * ENC_ATTN_WAVES * 64 * ENC_ATTN_QW;
}
inline int clipvis_attn_cot_chunk(int hd, int tables) { return clipvis_attn_cot_lds_floats(hd, 64, tables) * sizeof(float) <= 65536 ? 64 : 32; }
// qkv [3 D][ld], o, go [D][ld], ml [2][heads][ld] of n images of T tokens each at columns i T + [0, T):
// dQ -> the q block of gqkv [3 D][ld], delta [heads][ld]
void launch_clipvis_attn_cot_q(const float* qkv, const float* o, const float* go, const float* ml, long ld, int D, int hd, int T, int heads,
                               int n, float scale, float* gqkv, float* delta, hipStream_t st);
// dK, dV -> the k and v blocks of gqkv, from the delta of the dQ launch
void launch_clipvis_attn_cot_kv(const float* qkv, const float* go, const float* ml, const float* delta, long ld, int D, int hd, int T,
                                int heads, int n, float scale, float* gqkv, hipStream_t st);

// ---- clipseg.hip: the decoder's attention over qkv [3 R][ld], M masks of T tokens each, out [R][ld]
// the instantiation of seg_attn_kernel<HD> a head width runs on (the create function admits 4, 8, 16, 32 and 64 only)
inline int seg_attn_instance(int hd) { return hd == 4 || hd == 8 || hd == 16 || hd == 32 ? hd : 64; }
void launch_seg_attn(const float* qkv, long ld, int R, int hd, int heads, int T, int M, float scale, float* out, hipStream_t st);

// ---- samdec.hip: the two cross-attentions of the SAM mask decoder (the comments above the kernels)
size_t sd_t2i_lds_bytes(int hd);
// token -> image: qx / out [P][8][Ci], K / V [Ci][ld] per prompt at a stride of kbs floats (0: the same for every prompt)
void launch_sd_t2i(const float* qx, const float* K, const float* V, long kbs, long ld, int T, int Ci, int hd, int heads, int P, int NQ,
                   float scale, float* out, hipStream_t st);
// image -> token: q [Ci][ld] per prompt at a stride of qbs floats (0: the same), kx / vx [P][8][Ci], out [P][Ci][ld] (may be q)
void launch_sd_i2t(const float* q, long qbs, const float* kx, const float* vx, long ld, int T, int Tp, int Ci, int hd, int heads, int P,
                   int NQ, float scale, float* out, hipStream_t st);

}  // namespace loco
