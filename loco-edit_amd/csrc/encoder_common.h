// What the encoder units (textenc.hip, t5enc.hip, samenc.hip, clipvis.hip, clipseg.hip) share: the parameter table with its
// loader, the base of their handles (device, last error, parameters, owned device buffers), the prologue of their create
// functions, the small host / device helpers of the channel-major [D][Tp] layout, the pre-LN transformer block of the CLIP
// towers, and the launchers of encoder_kernels.hip.
#pragma once
#include "enc_attn_lds.h"
#include "kernels.h"
#include "../../include/loco_hip.h"

#include <algorithm>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

namespace loco {

struct DeviceGuard {           // the caller's current device is restored on every return
    int prev = 0;
    explicit DeviceGuard(int d) { (void)hipGetDevice(&prev); (void)hipSetDevice(d); }
    ~DeviceGuard() { (void)hipSetDevice(prev); }
};

inline unsigned blocks256(long n) { return (unsigned)((n + 255) / 256); }
inline size_t round64(size_t n) { return (n + 63) / 64 * 64; }

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// Y [M][Tp] = W [M][K] X [K][Tp] (+ bias per row) (+ R), channel-major activations
inline GemmArgs enc_linear(const float* W, const float* bias, const float* X, float* Y, const float* R, int M, int K, int Tp) {
    GemmArgs g; std::memset(&g, 0, sizeof(g));
    g.A = W; g.sam = K; g.sak = 1;
    g.Bm = X; g.sbk = Tp; g.sbn = 1;
    g.C = Y; g.scm = Tp; g.scn = 1;
    g.bias = bias; g.R = R;
    g.M = M; g.N = Tp; g.K = K; g.batch = 1; g.alpha = 1.f;
    return g;
}

// The named parameters of an encoder inside ONE device allocation.  A create function lays the table out (add / reserve /
// view, each optionally with the handle's pointer that is to address the block), allocates `total` floats and binds them.
struct ParamTable {
    struct Param { std::string name; std::vector<int64_t> shape; size_t off; float* dst; bool loaded; };
    struct Slot { float** p; size_t off; };
    std::vector<Param> params;
    std::vector<Slot> slots;
    size_t total = 0;                      // floats laid out so far

    static size_t count(const std::vector<int64_t>& shape) {
        size_t cnt = 1;
        for (auto d : shape) cnt *= (size_t)d;
        return cnt;
    }
    // a raw block of n floats (a packed operator that `view`s name the parts of); the caller rounds n where it wants padding
    size_t reserve(size_t n, float** slot = nullptr) {
        const size_t off = total;
        total += n;
        if (slot) slots.push_back({slot, off});
        return off;
    }
    // a named parameter at a given offset inside a reserved block
    void view(const std::string& name, std::vector<int64_t> shape, size_t off) { params.push_back({name, std::move(shape), off, nullptr, false}); }
    // a named parameter of its own; the running total goes up to the next multiple of 64 floats
    size_t add(const std::string& name, std::vector<int64_t> shape, float** slot = nullptr) {
        const size_t off = reserve(round64(count(shape)), slot);
        view(name, std::move(shape), off);
        return off;
    }
    void bind(float* base) {
        for (Param& p : params) p.dst = base + p.off;
        for (const Slot& s : slots) *s.p = base + s.off;
    }
    // host: fp32 values behind a host or a device pointer.  0, or -1 with the message in err; *loaded_dst: where they went
    int load(const char* name, const float* host, const int64_t* shape, int32_t ndim, int device, const char* fn, std::string& err,
             const float** loaded_dst = nullptr) {
        auto fail = [&](const std::string& m) { err = std::string(fn) + ": " + m; return -1; };
        if (!name || !host || (ndim > 0 && !shape) || ndim < 0) return fail("null argument");
        for (Param& p : params) {
            if (p.name != name) continue;
            if ((size_t)ndim != p.shape.size() || !std::equal(p.shape.begin(), p.shape.end(), shape)) {
                std::string m = p.name + " has shape [";
                for (size_t i = 0; i < p.shape.size(); ++i) m += (i ? ", " : "") + std::to_string(p.shape[i]);
                return fail(m + "], got another");
            }
            DeviceGuard dg(device);
            if (hipMemcpy(p.dst, host, count(p.shape) * sizeof(float), hipMemcpyDefault) != hipSuccess)
                return fail("copy of " + p.name + " failed");
            p.loaded = true;
            if (loaded_dst) *loaded_dst = p.dst;
            return 0;
        }
        return fail(std::string("unknown parameter ") + name);
    }
    // the count of parameters not loaded yet; the first one's name goes to err
    int missing(std::string& err) const {
        int miss = 0;
        for (const Param& p : params) {
            if (!p.loaded) {
                if (!miss) err = "missing parameter " + p.name;
                ++miss;
            }
        }
        return miss;
    }
};

// Base of the encoder handles.  Every device buffer of a handle -- the parameters first -- comes from one alloc() call and
// is freed by the destructor, on the handle's device.
struct EncoderBase {
    int device = 0;
    std::string err;
    float* params = nullptr;               // one allocation for every parameter
    ParamTable table;
    std::vector<void*> owned;

    struct Buf { void** p; size_t bytes; bool zero; };
    template <class T> static Buf buf(T** p, size_t n, bool zero = false) { return {(void**)p, n * sizeof(T), zero}; }

    int fail(const std::string& m) { err = m; return -1; }
    // params (table.total floats, bound to the table) and the listed buffers; false when an allocation failed
    bool alloc(std::initializer_list<Buf> bufs) {
        auto one = [&](const Buf& b) {
            if (hipMalloc(b.p, b.bytes) != hipSuccess) return false;
            owned.push_back(*b.p);
            return !b.zero || hipMemset(*b.p, 0, b.bytes) == hipSuccess;
        };
        if (!one(buf(&params, table.total))) return false;
        for (const Buf& b : bufs)
            if (!one(b)) return false;
        table.bind(params);
        return true;
    }
    // a buffer outside alloc() that grows on demand (the owner's destructor frees it); false when hipMalloc failed
    static bool grow(float** p, size_t* have, size_t need) {
        if (need <= *have) return true;
        if (*p) (void)hipFree(*p);                 // (waits for the launches that read it)
        *p = nullptr; *have = 0;
        if (hipMalloc(p, need * sizeof(float)) != hipSuccess) return false;
        *have = need;
        return true;
    }
    virtual ~EncoderBase() {
        DeviceGuard dg(device);
        for (void* p : owned) (void)hipFree(p);
    }
};

// A create function: the argument checks, `refuse(cfg)` (the reason a geometry is not built, or "" -- it runs before a device
// is asked for), the device check, then `build(handle)` under the device guard (false: an allocation failed).  Messages go
// to create_err as "<fn>: <reason>".
template <class Handle, class Cfg, class Out, class Refuse, class Build>
int encoder_create(const char* fn, std::string& create_err, const Cfg* cfg, int32_t device, Out** out, Refuse refuse, Build build) {
    auto report = [&](const std::string& m) { create_err = std::string(fn) + ": " + m; return -1; };
    if (!out) return report("out is NULL");
    *out = nullptr;
    if (!cfg) return report("cfg is NULL");
    const std::string why = refuse(*cfg);
    if (!why.empty()) return report(why);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return report("no such HIP device");
    DeviceGuard dg(device);
    Handle* t = new Handle();
    t->device = device;
    if (!build(*t)) {
        delete t;
        return report("hipMalloc failed");
    }
    *out = t;
    return 0;
}

// ---- the pre-LN transformer block of the CLIP towers (textenc.hip, clipvis.hip)
struct PreLnLayer { float *ln1_g, *ln1_b, *wqkv, *bqkv, *wo, *bo, *ln2_g, *ln2_b, *w1, *b1, *w2, *b2; };

// the parameters of layer `prefix` under transformers' CLIP names; q / k / v land in one packed [3 D][D] operator
inline void add_clip_layer(ParamTable& pt, const std::string& p, long D, long F, PreLnLayer& ly) {
    pt.add(p + "layer_norm1.weight", {D}, &ly.ln1_g);
    pt.add(p + "layer_norm1.bias", {D}, &ly.ln1_b);
    const size_t wq = pt.reserve((size_t)3 * D * D, &ly.wqkv), bq = pt.reserve(round64(3 * D), &ly.bqkv);
    const char* qkvn[3] = {"q_proj", "k_proj", "v_proj"};
    for (int j = 0; j < 3; ++j) {
        pt.view(p + "self_attn." + qkvn[j] + ".weight", {D, D}, wq + (size_t)j * D * D);
        pt.view(p + "self_attn." + qkvn[j] + ".bias", {D}, bq + (size_t)j * D);
    }
    pt.add(p + "self_attn.out_proj.weight", {D, D}, &ly.wo);
    pt.add(p + "self_attn.out_proj.bias", {D}, &ly.bo);
    pt.add(p + "layer_norm2.weight", {D}, &ly.ln2_g);
    pt.add(p + "layer_norm2.bias", {D}, &ly.ln2_b);
    pt.add(p + "mlp.fc1.weight", {F, D}, &ly.w1);
    pt.add(p + "mlp.fc1.bias", {F}, &ly.b1);
    pt.add(p + "mlp.fc2.weight", {D, F}, &ly.w2);
    pt.add(p + "mlp.fc2.bias", {D}, &ly.b2);
}

// The tensors of one block, [.][Tp] each: h_in -> h_mid (after the attention) -> h_out; x and f are scratch, st1 / st2 the
// statistics of the two LayerNorms.  h_mid and h_out may be h_in (the block in place), st2 may be st1.
struct PreLnBufs { float *h_in, *x, *qkv, *attn, *h_mid, *f, *h_out, *st1, *st2; };

// LN -> packed qkv -> attn(qkv, attn) -> out_proj + h_in -> LN -> fc1 with `act` (a GEMM_ACT_*) -> fc2 + h_mid
template <class Attn>
void pre_ln_block(const PreLnLayer& ly, const PreLnBufs& b, int D, int F, int Tp, float eps, int act, hipStream_t st, Attn attn) {
    launch_ln_fwd(b.h_in, 0, 1, D, Tp, ly.ln1_g, ly.ln1_b, eps, b.x, 0, b.st1, 0, st);
    launch_gemm_fixed(enc_linear(ly.wqkv, ly.bqkv, b.x, b.qkv, nullptr, 3 * D, D, Tp), GEMM_ACT_NONE, st);
    attn(b.qkv, b.attn);
    launch_gemm_fixed(enc_linear(ly.wo, ly.bo, b.attn, b.h_mid, b.h_in, D, D, Tp), GEMM_ACT_NONE, st);
    launch_ln_fwd(b.h_mid, 0, 1, D, Tp, ly.ln2_g, ly.ln2_b, eps, b.x, 0, b.st2, 0, st);
    launch_gemm_fixed(enc_linear(ly.w1, ly.b1, b.x, b.f, nullptr, F, D, Tp), act, st);
    launch_gemm_fixed(enc_linear(ly.w2, ly.b2, b.f, b.h_out, b.h_mid, D, F, Tp), GEMM_ACT_NONE, st);
}

// ---- encoder_kernels.hip
// The streamed attention of the ViT encoders over qkv [3 D][ld] = q | k | v channel rows, out [D][ld]: `groups` groups of nk
// tokens each at columns g * nk + [0, nk), every query against the keys of its own group, score (q scale) . k.  relh / relw
// [heads][Tall][size] (or null): added to the score of key (row, col) of a size x size group (nk = size^2) as relh[q][row] +
// relw[q][col].  ml [2][heads][ld] (or null): receives the row max and the row sum of every query.  Not both (not built).
struct EncAttnArgs {
    const float* qkv; long ld; int D, hd, nk, groups, heads; float scale; float* out;
    const float *relh, *relw; long Tall; int size;
    float* ml;
};
void launch_enc_attn(const EncAttnArgs& a, hipStream_t st);
// P[(ci ps + ky) ps + kx][i T + cls + ty G + tx] = pix[i][ci][ty ps + ky][tx ps + kx] for the n images [3][S][S] of pix, T = cls
// + G^2 tokens each, the first cls (0 or 1) of them class columns; 0 in the class and the padding columns of P [3 ps^2][Tp]
void launch_enc_patch(const float* pix, int n, int S, int ps, int G, int cls, int Tp, float* P, hipStream_t st);
// out[col][c] = x[c][col] for the first `cols` columns of x [C][ld]
void launch_enc_transpose(const float* x, int ld, int cols, int C, float* out, hipStream_t st);

}  // namespace loco
