// The handle behind include/loco_hip.h's loco_text, shared by the two text encoders: CLIP (textenc.hip, loco_text_create)
// and the T5 encoder of DeepFloyd IF (t5enc.hip, loco_t5_create).  loco_text_load_param / _params_missing / _last_error /
// _destroy (textenc.hip) work on the parameter table and the allocations alone, so they serve both kinds; loco_text_encode
// and loco_text_encode_masked look at `kind`.
#pragma once
#include "kernels.h"
#include "../../include/loco_hip.h"

#include <cstring>
#include <string>
#include <vector>

struct TextParam {
    std::string name;
    std::vector<int64_t> shape;
    float* dst;
    bool loaded;
};
struct TextLayer { float *ln1_g, *ln1_b, *wqkv, *bqkv, *wo, *bo, *ln2_g, *ln2_b, *w1, *b1, *w2, *b2; };
// T5 block: RMS-norm weights, q | k | v packed [3 inner][D], o [D][inner], wi_0 | wi_1 packed [2 F][D], wo [D][F]
struct T5Layer { float *ln1, *wqkv, *wo, *ln2, *wi, *wff; };

enum TextKind : int { TEXT_KIND_CLIP = 0, TEXT_KIND_T5 = 1 };

struct loco_text {
    int kind = TEXT_KIND_CLIP;
    loco_text_cfg cfg;
    int device = 0, max_prompts = 0, L = 0, D = 0, hd = 0, Tmax = 0;
    std::string err;
    float* params = nullptr;              // one allocation for every parameter
    float *tok = nullptr, *pos = nullptr, *lnf_g = nullptr, *lnf_b = nullptr;
    std::vector<TextLayer> layer;
    std::vector<TextParam> table;
    // workspace [.][Tmax]
    float *h = nullptr, *x = nullptr, *qkv = nullptr, *attn = nullptr, *f = nullptr, *stats = nullptr;
    int* ids = nullptr;
    std::vector<int> ids_host;
    // ---- T5 only (t5enc.hip)
    loco_t5_cfg t5;
    int inner = 0;                        // heads * d_kv
    float* relw = nullptr;                // relative_attention_bias.weight [buckets][heads] (inside params)
    float* bias_tab = nullptr;            // [heads][2 L - 1]: the bias of key offset k - q + L - 1, built when relw is loaded
    std::vector<int> bucket;              // [2 L - 1] bucket of every offset
    std::vector<T5Layer> t5layer;
    int* lens = nullptr;                  // device [max_prompts]
    std::vector<int> lens_host;
    int fail(const std::string& m) { err = m; return -1; }
};

namespace loco {

struct TextDeviceGuard {       // the caller's current device is restored on every return
    int prev = 0;
    explicit TextDeviceGuard(int d) { (void)hipGetDevice(&prev); (void)hipSetDevice(d); }
    ~TextDeviceGuard() { (void)hipSetDevice(prev); }
};

// Y [M][Tp] = W [M][K] X [K][Tp] (+ bias per row) (+ R), channel-major activations
inline GemmArgs text_linear(const float* W, const float* bias, const float* X, float* Y, const float* R, int M, int K, int Tp) {
    GemmArgs g; std::memset(&g, 0, sizeof(g));
    g.A = W; g.sam = K; g.sak = 1;
    g.Bm = X; g.sbk = Tp; g.sbn = 1;
    g.C = Y; g.scm = Tp; g.scn = 1;
    g.bias = bias; g.R = R;
    g.M = M; g.N = Tp; g.K = K; g.batch = 1; g.alpha = 1.f;
    return g;
}

// out[col][c] = x[c][col] for the T real columns of x [D][Tp] (textenc.hip)
void launch_text_transpose(const float* x, int Tp, int T, int D, float* out, hipStream_t st);

void text_set_create_error(const std::string& m);         // what loco_text_last_error(NULL) returns (textenc.hip)

// t5enc.hip
int t5_encode(loco_text* t, const int32_t* ids_dev, const int32_t* lens, int32_t n, float* out_dev, hipStream_t st);
int t5_param_loaded(loco_text* t, const float* dst);      // hook of loco_text_load_param: builds the bias table
void t5_free(loco_text* t);

}  // namespace loco
