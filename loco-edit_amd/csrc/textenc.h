// The handle behind include/loco_hip.h's loco_text: the base of the two text encoders, CLIP (textenc.hip,
// loco_text_create) and the T5 encoder of DeepFloyd IF (t5enc.hip, loco_t5_create), and the kernels both launch (but for the
// transpose of the final states, encoder_common.h's launch_enc_transpose).  The six loco_text_* functions (textenc.hip) work
// on this base alone: what differs between the encoders is behind its virtuals.
#pragma once
#include "encoder_common.h"

struct loco_text : loco::EncoderBase {
    int max_prompts = 0, L = 0, D = 0, hd = 0, Tmax = 0;
    float *tok = nullptr, *lnf_g = nullptr;
    // workspace [.][Tmax]
    float *h = nullptr, *x = nullptr, *qkv = nullptr, *attn = nullptr, *f = nullptr;
    int* ids = nullptr;
    std::vector<int> ids_host;

    // lens: host [n] or NULL = every prompt is L long
    virtual int encode(const int32_t* ids_dev, const int32_t* lens, int32_t n, float* out_dev, hipStream_t st) = 0;
    virtual int encode_masked(const int32_t* ids_dev, const int32_t* lens, int32_t n, float* out_dev, hipStream_t st) {
        return encode(ids_dev, lens, n, out_dev, st);
    }
    virtual int param_loaded(const float* /*dst*/) { return 0; }      // after loco_text_load_param has copied a parameter to dst
};

namespace loco {

extern thread_local std::string g_text_create_err;        // what loco_text_last_error(NULL) returns (textenc.hip)

// the head of every encode: the arguments, n against max_prompts, the parameters complete
int text_check_call(loco_text* t, const int32_t* ids_dev, int32_t n, const float* out_dev);
// t->ids = the T = n * L ids behind ids_dev, each checked against [0, vocab) on the host: the one host synchronisation of a call
int stage_ids(loco_text* t, const int32_t* ids_dev, int T, int L, int vocab, hipStream_t st);
// h[c][col] = tok[ids[col]][c] (+ pos[col % L][c] unless pos is NULL) for col < T, 0 for the padding columns T <= col < Tp
void launch_text_embed(const int* ids, int T, int Tp, int L, int D, const float* tok, const float* pos, float* h, hipStream_t st);
// Self-attention of one (prompt, head) per workgroup over qkv [3 inner][ld] = q | k | v channel rows, out [inner][ld].
// causal_scaled: keys j <= i, score q_i . k_j * scale (CLIP); else keys j < lens[p], score q_i . k_j + bias_tab[h][j - i + L - 1] (T5)
size_t prompt_attn_lds_bytes(int hd, int L);
void launch_prompt_attn(bool causal_scaled, const float* qkv, long ld, int n, int heads, int L, int inner, int hd, float scale,
                        const float* bias_tab, const int* lens, float* out, hipStream_t st);

}  // namespace loco
