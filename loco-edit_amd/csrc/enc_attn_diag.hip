// loco_debug_enc_attn (include/loco_hip_diag.h), linked into the diagnostics library only: ONE launch of ONE attention kernel
// of the encoders on the caller's tensors, through the launcher the product's call site uses (encoder_common.h, textenc.h,
// enc_attn_launch.h).  Only the descriptor -> argument mapping, the refusals and the route text live here; the text is written
// from the predicates the launchers branch on.  No engine and no handle: nothing is allocated.
#include "../../include/loco_hip_diag.h"
#include "enc_attn_launch.h"
#include "textenc.h"

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using namespace loco;

namespace {

int enc_diag_say(char* err, int64_t err_cap, const std::string& m, int rc) {
    if (err && err_cap > 0) std::snprintf(err, (size_t)err_cap, "debug_enc_attn: %s", m.c_str());
    return rc;
}

bool pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }

}  // namespace

extern "C" int loco_debug_enc_attn(const loco_enc_attn_desc* d, char* route, int64_t cap, char* err, int64_t err_cap, void* stream) {
    auto refuse = [&](const std::string& m) { return enc_diag_say(err, err_cap, m, -2); };
    if (!d || d->struct_size != (int32_t)sizeof(loco_enc_attn_desc)) return refuse("descriptor size mismatch");
    hipStream_t st = (hipStream_t)stream;
    const int op = d->op, D = d->D, hd = d->hd, heads = d->heads, nk = d->nk, groups = d->groups;
    const long ld = (long)d->ld;
    if (op < 0 || op > 9) return refuse("op outside 0 ... 9");
    if (D < 1 || hd < 1 || heads < 1 || nk < 1 || groups < 1 || ld < 1) return refuse("D, hd, heads, nk, groups and ld must be positive");
    if ((long)heads * hd != D) return refuse("D must be heads x hd");
    const bool streamed = op <= 2 || op == 5 || op == 6;
    if (streamed && hd > 128) return refuse("hd > 128: the streamed kernels give a lane the channels c and c + 64");
    const long cols = op == 8 ? nk : op == 9 ? d->Tp : (long)groups * nk;
    char line[96];
    line[0] = 0;

    if (op <= 2) {
        if (!d->qkv || !d->out) return refuse("a required operand is null");
        if ((d->relh != nullptr) != (d->relw != nullptr)) return refuse("relh and relw come together");
        if (op == 2 && !d->relh) return refuse("a required operand is null");
        if (op == 1 && !d->ml) return refuse("a required operand is null");
        if (d->relh && d->ml) return refuse("relh together with ml is not built");
        if ((op == 0 && (d->relh || d->ml)) || (op == 1 && d->relh)) return refuse("tables are op 2, ml is op 1");
        if (op == 2) {
            if (d->size < 1 || (long)d->size * d->size != nk) return refuse("nk must be size^2");
            if (d->Tall < (long)groups * nk) return refuse("Tall is smaller than the columns addressed");
        }
        if (enc_attn_lds_floats(hd, op == 2 ? d->size : 0) * sizeof(float) > 65536) return refuse("the LDS carve-up exceeds 65536 bytes");
        if (ld < cols) return refuse("ld is smaller than the columns addressed");
        const EncAttnArgs a{d->qkv, ld, D, hd, nk, groups, heads, d->scale, d->out, d->relh, d->relw, (long)d->Tall, d->size, d->ml};
        std::snprintf(line, sizeof(line), "kernel=enc_attn bias=%d keep=%d\n", (int)enc_attn_bias(a), (int)enc_attn_keep(a));
        launch_enc_attn(a, st);
    } else if (op <= 4) {
        const bool causal = op == 3;
        if (!d->qkv || !d->out || (!causal && (!d->bias_tab || !d->lens))) return refuse("a required operand is null");
        if (nk > 128) return refuse("L > 128: a lane scores two keys");
        if (prompt_attn_lds_bytes(hd, nk) > 65536) return refuse("the LDS carve-up exceeds 65536 bytes");
        if (ld < cols) return refuse("ld is smaller than the columns addressed");
        if (!causal) {
            std::vector<int32_t> lens((size_t)groups);
            if (hipStreamSynchronize(st) != hipSuccess ||
                hipMemcpy(lens.data(), d->lens, lens.size() * sizeof(int32_t), hipMemcpyDefault) != hipSuccess)
                return enc_diag_say(err, err_cap, "reading lens failed", -1);
            for (int p = 0; p < groups; ++p)
                if (lens[p] < 1 || lens[p] > nk)
                    return refuse("lens[" + std::to_string(p) + "] = " + std::to_string(lens[p]) + " outside [1, L]");
        }
        std::snprintf(line, sizeof(line), "kernel=prompt_attn causal=%d\n", (int)causal);
        launch_prompt_attn(causal, d->qkv, ld, groups, heads, nk, D, hd, d->scale, d->bias_tab, d->lens, d->out, st);
    } else if (op <= 6) {
        const int tables = op == 5 ? 1 : 2;
        if (!d->qkv || !d->go || !d->ml || !d->delta || !d->gqkv || (op == 5 && !d->o)) return refuse("a required operand is null");
        const int kc = clipvis_attn_cot_chunk(hd, tables);
        if (clipvis_attn_cot_lds_floats(hd, kc, tables) * sizeof(float) > 65536) return refuse("the LDS carve-up exceeds 65536 bytes");
        if (ld < cols) return refuse("ld is smaller than the columns addressed");
        std::snprintf(line, sizeof(line), "kernel=clipvis_attn_cot_%s chunk=%d\n", op == 5 ? "q" : "kv", kc);
        if (op == 5) launch_clipvis_attn_cot_q(d->qkv, d->o, d->go, d->ml, ld, D, hd, nk, heads, groups, d->scale, d->gqkv, d->delta, st);
        else launch_clipvis_attn_cot_kv(d->qkv, d->go, d->ml, d->delta, ld, D, hd, nk, heads, groups, d->scale, d->gqkv, st);
    } else if (op == 7) {
        if (!d->qkv || !d->out) return refuse("a required operand is null");
        if (hd != 4 && hd != 8 && hd != 16 && hd != 32 && hd != 64) return refuse("head width: the kernel is built for 4, 8, 16, 32 and 64");
        if (nk > 2048) return refuse("T > 2048: the kernel keeps a row of scores per query in LDS");
        if (ld < cols) return refuse("ld is smaller than the columns addressed");
        std::snprintf(line, sizeof(line), "kernel=seg_attn hd=%d\n", seg_attn_instance(hd));
        launch_seg_attn(d->qkv, ld, D, hd, heads, nk, groups, d->scale, d->out, st);
    } else {
        if (!d->q || !d->k || !d->v || !d->out) return refuse("a required operand is null");
        if (!pow2(hd) || hd > 64) return refuse("hd must be a power of two <= 64");
        if (d->NQ < 1 || d->NQ > 8) return refuse("NQ outside [1, 8]");
        if (d->kbs < 0 || d->qbs < 0) return refuse("a negative stride");
        if (op == 8) {
            if (sd_t2i_lds_bytes(hd) > 65536) return refuse("the LDS carve-up exceeds 65536 bytes");
            if (ld < cols) return refuse("ld is smaller than the columns addressed");
            std::snprintf(line, sizeof(line), "kernel=sd_t2i\n");
            launch_sd_t2i(d->q, d->k, d->v, (long)d->kbs, ld, nk, D, hd, heads, groups, d->NQ, d->scale, d->out, st);
        } else {
            if (d->Tp < nk) return refuse("Tp is smaller than T");
            if (ld < cols) return refuse("ld is smaller than the columns addressed");
            if (d->out == d->q && groups > 1) return refuse("out may be q for one prompt only");
            std::snprintf(line, sizeof(line), "kernel=sd_i2t\n");
            launch_sd_i2t(d->q, (long)d->qbs, d->k, d->v, ld, nk, d->Tp, D, hd, heads, groups, d->NQ, d->scale, d->out, st);
        }
    }
    hipError_t he = hipGetLastError();
    if (he == hipSuccess) he = hipStreamSynchronize(st);
    if (he == hipSuccess) he = hipGetLastError();
    if (he != hipSuccess) return enc_diag_say(err, err_cap, hipGetErrorString(he), -1);
    if (route && cap > 0) {
        if ((int64_t)std::strlen(line) + 1 > cap) return enc_diag_say(err, err_cap, "route buffer too small", -4);
        std::memcpy(route, line, std::strlen(line) + 1);
    }
    return 0;
}
