// The hooks of include/loco_hip_diag.h: tuning / bring-up entry points on one launch, one attention stage or one tensor of the
// engine, through the engine's own functions (engine_internal.h), so the routes they report are the product's.  Only in
// libloco_hip_diag.so; the plan and route texts arrive through loco_ctx::plan_log / attn_log, null everywhere else.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "../../include/loco_hip_diag.h"
#include "conv_plan_text.h"
#include "engine_internal.h"

using namespace loco;
using namespace loco::eng;

// what a hook allocated since it read `owned0` / `bytes0` (weight layouts, small arrays, scratch), freed behind its launches
static void release_since(loco_ctx* c, hipStream_t st, size_t owned0, size_t bytes0) {
    (void)hipStreamSynchronize(st);
    while (c->owned.size() > owned0) { (void)hipFree(c->owned.back()); c->owned.pop_back(); }
    c->bytes = bytes0;
}

// well-formed split-bf16 weight records of random values (64 bytes: [hi k0-7|hi k8-15|lo k0-7|lo k8-15], pieces XOR-swizzled by
// (record index inside its tap block >> 2) & 3), so that diagnostic launches produce comparable numbers, not Inf / NaN
__global__ void diag_fill_records(unsigned char* rec, long nrec, int wpitch, unsigned seed, float scale) {
    const long r = (long)blockIdx.x * 256 + threadIdx.x;
    if (r >= nrec) return;
    const int idx = (int)(r % wpitch);
    unsigned short hi[16], lo[16];
    for (int k = 0; k < 16; ++k) {
        unsigned h = (unsigned)(r * 16 + k) * 2654435761u + seed * 40503u;
        h ^= h >> 15; h *= 2246822519u; h ^= h >> 13; h *= 3266489917u; h ^= h >> 16;
        const float v = scale * ((float)(h & 0xffffff) * (1.0f / 8388608.0f) - 1.0f);
        const __bf16 hb = (__bf16)v;
        const __bf16 lb = (__bf16)(v - (float)hb);
        hi[k] = __builtin_bit_cast(unsigned short, hb);
        lo[k] = __builtin_bit_cast(unsigned short, lb);
    }
    const int sw = (idx >> 2) & 3;
    unsigned short* base = reinterpret_cast<unsigned short*>(rec + r * 64);
    for (int k = 0; k < 8; ++k) {
        base[((0 ^ sw) << 3) + k] = hi[k];
        base[((1 ^ sw) << 3) + k] = hi[8 + k];
        base[((2 ^ sw) << 3) + k] = lo[k];
        base[((3 ^ sw) << 3) + k] = lo[8 + k];
    }
}
extern "C" {
// Tuning hook: time one convolution shape on scratch data (random inputs), avg ms over `iters` launches.
int loco_bench_conv(loco_ctx* c, int32_t cin, int32_t cout, int32_t H, int32_t W, int32_t B, int32_t mode,
                    int32_t taps, int32_t tile, int32_t iters, float* ms_avg, void* stream) {
    if (!c) return -2;
    if (finalize_params(c)) return -3;
    hipStream_t st = (hipStream_t)stream;
    const long HW = (long)H * W;
    // LOCO_BENCH_GEOM (3x3 only; H x W stays the OUTPUT map): 1 = over a nearest-x2 input, 2 / 3 = over a zero-inserted input with
    // pad 2 / 1 (the stride-2 conv's data gradient) -- the polyphase route where plan_conv takes it (LOCO_POLYPHASE=0: the 3x3 route);
    // 4 = conv + 2x2 sum-pool as ONE polyphase launch (ConvArgs::pool2; H x W is the INPUT map; the 3x3 route of this form is the
    // plain launch + launch_pool2x2_sum)
    const int geom = (taps == 9 && getenv("LOCO_BENCH_GEOM")) ? atoi(getenv("LOCO_BENCH_GEOM")) : 0;
    if (geom < 0 || geom > 4 || (geom && ((H | W) & 1))) { c->err = "bench_conv: bad LOCO_BENCH_GEOM"; return -2; }
    const long in_e = (long)cin * ((geom && geom != 4) ? HW / 4 : HW), out_e = (long)cout * HW;
    if ((in_e + out_e + (geom == 4 ? out_e / 4 : 0)) * B > (long)c->cfg.max_batch * c->prog->per_sample || 2 * in_e > (long)c->prog->per_sample ||
        in_e > c->prog->sx_total) { c->err = "bench_conv: shape exceeds the arenas"; return -2; }
    float* in = c->arenaT;
    float* out = c->arenaT + in_e * B;
    // LOCO_BENCH_ZERO (bit 1: activations, bit 2: weights): all-zero operands draw less power in the matrix pipe -- the time
    // against random data says how much of a launch the chip's clock management decides (MI355X_MICROARCH.md, DVFS give-back)
    const int bz = getenv("LOCO_BENCH_ZERO") ? atoi(getenv("LOCO_BENCH_ZERO")) : 0;
    const float zs = (bz & 1) ? 0.0f : 1.0f, zw = (bz & 2) ? 0.0f : 1.0f;
    launch_fill_random(in, in_e * B, 1u, zs, st);
    launch_fill_random(c->arenaP, in_e, 2u, zs, st);
    launch_fill_random(reinterpret_cast<float*>(c->sxcache), 2 * in_e, 3u, zs, st);
    launch_fill_random(c->statsP, c->prog->stats_per_sample, 4u, 1.0f, st);
    launch_fill_random(c->statsT, c->prog->stats_per_sample * B, 5u, 0.01f, st);
    // weights: any conv of matching size is fine for timing; synthesise records in the split-K workspace
    size_t wfl = (size_t)((cin + 15) / 16) * 16 * (geom ? 16 : taps) * ((cout + 31) & ~31);      // (geom: room for the folded records, 4 taps x 4 couts)
    if (wfl * 2 > c->partial_floats) { c->err = "bench_conv: weights exceed workspace"; return -2; }
    float* wf = c->partial + c->partial_floats - wfl * 2;
    launch_fill_random(wf, (long)wfl * 2, 6u, 0.05f * zw, st);
    if (c->prec == 1) {      // split-bf16 records: well-formed ones
        const long nrec = (long)((cin + 15) / 16) * (geom ? 16 : taps) * ((cout + 31) & ~31);
        hipLaunchKernelGGL(diag_fill_records, dim3((unsigned)((nrec + 255) / 256)), dim3(256), 0, st,
                           reinterpret_cast<unsigned char*>(wf), nrec, (cout + 31) & ~31, 7u, 0.05f * zw);
    }
    ConvArgs a; conv_defaults(a);
    a.in = in; a.in_bs = in_e; a.Cin = cin; a.Hin = H; a.Win = W;
    a.prim = c->arenaP; a.prim_bs = 0; a.sx = c->sxcache;
    a.w = wf; a.wb = wf; a.wh = wf;
    a.out = out; a.out_bs = out_e; a.Cout = cout; a.Hout = H; a.Wout = W; a.B = B;
    a.mode = mode; a.pad = taps == 9 ? 1 : 0; a.in_padded = 1; a.taps = taps;
    if (geom == 4) {
        a.pool2 = 1; a.pool_tmp = out; a.pool_tmp_bs = out_e;
        a.out = out + out_e * B; a.out_bs = out_e / 4; a.Hout = H / 2; a.Wout = W / 2;
        a.wqb = wf; a.wqh = wf;
    } else if (geom) {
        a.Hin = H / 2; a.Win = W / 2;
        if (geom == 1) a.upsample = 1; else { a.zins = 1; a.pad = geom == 2 ? 2 : 1; }
        a.wpb = wf; a.wph = wf;
    }
    a.sc = c->statsP; a.sh = c->statsP + cin; a.scsh_bs = 0; a.mr = c->statsP + 2 * cin; a.mr_bs = 0;
    a.gamma_ = c->statsP; a.tst = c->statsT; a.tst_bs = c->prog->stats_per_sample; a.cpg = cin / c->cfg.gn_groups;
    a.tc = c->statsT + 64; a.tc_bs = c->prog->stats_per_sample;
    if (a.cpg < 1) a.cpg = 1;
    a.nsplit = 1; a.partial = c->partial;
    a.partial_floats = c->partial_floats - wfl * 2;                            // (the synthetic weights sit at the end of the workspace)
    if (getenv("LOCO_BENCH_COT") && atoi(getenv("LOCO_BENCH_COT")) && taps == 1) {
        // the ResBlock shortcut's cotangent form: norm-cotangent term in the epilogue (synthetic operands behind the output tensor)
        if ((in_e + 2 * out_e) * B > (long)c->cfg.max_batch * c->prog->per_sample || out_e > c->prog->sx_total ||
            2L * cout > c->prog->stats_per_sample) { c->err = "bench_conv: cot operands exceed the arenas"; return -2; }
        launch_fill_random(out + out_e * B, out_e * B, 8u, zs, st);
        if (out_e > in_e) launch_fill_random(reinterpret_cast<float*>(c->sxcache), 2 * out_e, 3u, zs, st);
        a.cot_d = out + out_e * B; a.cot_d_bs = out_e; a.cot_sx = c->sxcache; a.cot_tc = c->statsT; a.cot_tc_bs = c->prog->stats_per_sample;
    }
    if (getenv("LOCO_BENCH_ACC") && atoi(getenv("LOCO_BENCH_ACC"))) a.accumulate = 1;
    conv_plan_family(a, c->prec);
    // what-if bits of the lock-step kernel's stamp build (-DLOCO_DUAL_STAMP, tests/diag/lowp_stamps.py): 2 halo loads collapsed,
    // 4 weight DMAs collapsed, 8 no conversions
    if (const char* e = getenv("LOCO_DUAL_WHATIF")) a.no_deep = atoi(e);
    conv_plan_tile_pair(a, c->prec, tile);
    if (geom) {      // the polyphase decision is plan_conv's alone
        ConvEnv e;
        e.prec = c->prec; e.partial = a.partial; e.partial_floats = a.partial_floats; e.max_batch = c->cfg.max_batch;
        a.poly = plan_conv(e, a, taps, nullptr, nullptr).l[0].args.poly;
        if (a.poly) a.nsplit = 1;
        if (geom == 4 && a.poly != 2) { c->err = "bench_conv: the shape does not take the pooled polyphase launch"; return -2; }
    }
    auto run = [&]() {
        if (c->prec == 1) launch_conv_bf16x3(a, taps, st);
        else if (c->prec == 2) launch_conv_f16(a, taps, st);
        else launch_conv(a, taps, st);
        launch_conv_splitk_reduce(a, st);
    };
    run();
    HIPCHK(c, hipEventRecord(c->ev0, st));
    for (int i = 0; i < iters; ++i) run();
    HIPCHK(c, hipEventRecord(c->ev1, st));
    HIPCHK(c, hipEventSynchronize(c->ev1));
    c->bench_out = out; c->bench_out_count = (int64_t)out_e * B;
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
    *ms_avg = ms / iters;
    HIPCHK(c, hipGetLastError());
    return 0;
}

// loco_debug_conv: the per-channel {m1, m2} a low-precision kernel reads, as the engine's statistics kernels leave them
// (launch_gn_tstats): unscaled for the tangent mode, times the group's rstd for the cotangent forms
}  // extern "C"
__global__ void diag_scale_tc(const float* tc, const float* mr, int C, int cpg, long n, int by_rstd, float* out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;      // one {m1, m2} pair of [B][C]
    if (i >= n) return;
    const float f = by_rstd ? mr[2 * (int)((i % C) / cpg) + 1] : 1.0f;
    out[2 * i] = f * tc[2 * i];
    out[2 * i + 1] = f * tc[2 * i + 1];
}
extern "C" {
int loco_debug_conv(loco_ctx* c, const loco_conv_desc* d, char* plan, int64_t cap, void* stream) {
    if (!c) return -2;
    if (!d || d->struct_size != (int32_t)sizeof(loco_conv_desc)) { c->err = "debug_conv: descriptor size mismatch"; return -2; }
    if (finalize_params(c)) return -3;
    hipStream_t st = (hipStream_t)stream;
    const int taps = d->taps, k = taps == 9 ? 3 : 1, B = d->B;
    if ((taps != 9 && taps != 1) || d->Cin < 1 || d->Cout < 1 || d->Hin < 1 || d->Win < 1 || B < 1 || (d->stride != 1 && d->stride != 2) ||
        d->mode < CM_NONE || d->mode > CM_GN_GELU || (d->upsample && d->zins) || (d->stride == 2 && (d->upsample || d->zins)) ||
        !d->weight || !d->in || !d->out) { c->err = "debug_conv: bad descriptor"; return -2; }
    if (d->stride == 2 && ((d->Hin | d->Win) & 1)) { c->err = "debug_conv: stride 2 needs an even map"; return -2; }
    const bool lin = d->mode == CM_TAN_SILU || d->mode == CM_COT_SILU;
    if (d->mode != CM_NONE && (!d->sc || !d->sh)) { c->err = "debug_conv: the prologue modes need sc / sh"; return -2; }
    if (lin && (!d->prim || !d->mr || !d->gamma || !d->tst || !d->tc || d->cpg < 1 || d->Cin % d->cpg)) {
        c->err = "debug_conv: modes 3 / 4 need prim, mr, gamma, tst, tc and cpg"; return -2;
    }
    if (d->Cin2 > 0 && (!d->in2 || !d->w2)) { c->err = "debug_conv: the second operator needs in2 and w2"; return -2; }
    if (d->Cin2 > 0 && (d->res || d->accumulate || taps != 9)) {      // its output IS the residual of the 3x3 operator
        c->err = "debug_conv: the second operator goes with a 3x3 conv without res / accumulate"; return -2;
    }
    if (d->cot_d && (!d->cot_prim || !d->cot_sc || !d->cot_sh || !d->cot_mr || !d->cot_tc || d->cot_cpg < 1 || d->Cout % d->cot_cpg)) {
        c->err = "debug_conv: the norm-cotangent term needs cot_prim, cot_sc, cot_sh, cot_mr, cot_tc and cot_cpg"; return -2;
    }
    if (d->pool2 && (taps != 9 || d->stride != 1 || d->upsample || d->zins || d->mode != CM_NONE || d->Cin2 > 0 || d->res || d->cot_d ||
                     ((d->Hin | d->Win) & 1))) { c->err = "debug_conv: pool2 goes with a raw 3x3 stride-1 conv of an even map"; return -2; }
    const int Hout = (d->stride == 2 || d->pool2) ? d->Hin / 2 : (d->upsample || d->zins) ? 2 * d->Hin : d->Hin;
    const int Wout = (d->stride == 2 || d->pool2) ? d->Win / 2 : (d->upsample || d->zins) ? 2 * d->Win : d->Win;
    {   // Every conv kernel walks the output map in tiles of min(Wout, 32) columns (a power of two) x 64 / 128 / 256 pixels and
        // writes whole tiles: maps as loco_create admits them (powers of two from 8 x 8), or whole 32-column, 8-row tiles.  Any
        // other map (48 x 48, 128 x 144) would be walked past its last row: refused here, never launched.
        auto pow2 = [](int v) { return v >= 8 && (v & (v - 1)) == 0; };
        auto walks = [&](int h, int w) { return (pow2(h) && pow2(w)) || (w % 32 == 0 && h % 8 == 0 && ((long)h * w) % 256 == 0); };
        if (!walks(Hout, Wout) || (d->pool2 && !walks(d->Hin, d->Win))) {
            c->err = "debug_conv: output map outside the tile geometry of the conv kernels"; return -2;
        }
    }
    const long in_e = (long)d->Cin * d->Hin * d->Win, out_e = (long)d->Cout * Hout * Wout, in2_e = (long)d->Cin2 * Hout * Wout;
    if ((in_e | out_e | in2_e) & 3) { c->err = "debug_conv: planes must be whole 16-byte units"; return -2; }
    auto up64 = [](long v) { return (v + 63) & ~63L; };
    // arena T: in | in2 | cot_d (dense samples); arena P: prim; {S, xhat} records: prim | cot_prim
    const long offT_in2 = d->in_arena ? up64(in_e * B) : 0, offT_cot = offT_in2 + up64(in2_e * B);
    const long needT = offT_cot + (d->cot_d ? out_e * B : 0);
    const long sx_cot = lin ? up64(in_e) : 0, need_sx = sx_cot + (d->cot_d ? out_e : 0);
    if (needT > (long)c->cfg.max_batch * c->prog->per_sample || (lin && in_e > (long)c->cfg.max_batch * c->prog->per_sample) ||
        need_sx > c->prog->sx_total) { c->err = "debug_conv: shape exceeds the arenas"; return -2; }
    // the launch's small arrays: one allocation of this call (sc sh mr gamma | tst tc per sample | cot_tc per sample)
    const int G = lin ? d->Cin / d->cpg : 0;
    const long tbs = up64(2L * G) + up64(2L * d->Cin);
    // tangent statistics request (st_prim): kept row partials, a zeroed sc / sh pair for the standalone pass
    const bool st_req = d->st_kind == 0 && d->st_prim != nullptr;
    if (st_req && (!d->st_mr || !d->st_out || d->st_cpg < 1 || d->Cout % d->st_cpg || d->cot_d || d->Cin2 > 0)) {
        c->err = "debug_conv: the statistics request needs st_prim, st_mr, st_out and st_cpg (no second operator, no cot_d)"; return -2;
    }
    // statistics request with a consuming norm (st_kind = ST_FWD / ST_TAN / ST_COT): run_conv takes the group count, the slot
    // layout and the arenas from the engine, so what does not fit them is refused here
    const int stk = d->st_kind, Gs = c->cfg.gn_groups;
    const bool st_norm = stk != 0, st_lin = stk == ST_TAN || stk == ST_COT;
    const long SBs = c->prog->stats_per_sample;
    const long sx_st = need_sx;      // ST_COT: the norm's {S, xhat} records over the output tensor, behind the other records
    if (st_norm) {
        if (stk < ST_FWD || stk > ST_COT) { c->err = "debug_conv: st_kind is 0, 1 (FWD), 2 (TAN) or 3 (COT)"; return -2; }
        if (Gs < 1 || d->Cout % Gs) { c->err = "debug_conv: statistics request: Cout must be a multiple of the engine's gn_groups"; return -2; }
        if (4L * d->Cout + 4L * Gs > SBs) { c->err = "debug_conv: statistics request: 4 Cout + 4 G exceeds a sample's statistics slot"; return -2; }
        if (((long)Hout * Wout) % 4) { c->err = "debug_conv: statistics request: Hout Wout must be a multiple of 4"; return -2; }
        if (B > c->cfg.max_batch) { c->err = "debug_conv: statistics request: B exceeds max_batch"; return -2; }
        if (!d->st_gamma || !d->st_beta) { c->err = "debug_conv: statistics request: st_gamma and st_beta are required"; return -2; }
        if (stk == ST_FWD && (!d->st_o_mr || !d->st_o_sc || !d->st_o_sh || (!d->st_ss_scale != !d->st_ss_shift))) {
            c->err = "debug_conv: ST_FWD needs st_o_mr, st_o_sc, st_o_sh (and st_ss_scale with st_ss_shift)"; return -2;
        }
        if (st_lin && (!d->st_prim || !d->st_sc || !d->st_sh || !d->st_mr || !d->st_o_tst || !d->st_o_tc)) {
            c->err = "debug_conv: ST_TAN / ST_COT need st_prim, st_sc, st_sh, st_mr, st_o_tst and st_o_tc"; return -2;
        }
        if (stk == ST_COT && (!c->sxcache || sx_st + out_e > c->prog->sx_total)) {
            c->err = "debug_conv: ST_COT: the norm's records exceed the record cache"; return -2;
        }
        if (d->st_keep && (stk == ST_COT || !d->st_keep_out || d->st_keep_cap < 1)) {
            c->err = "debug_conv: st_keep goes with ST_FWD / ST_TAN and needs st_keep_out, st_keep_cap"; return -2;
        }
        if (d->pool2) { c->err = "debug_conv: statistics request: not with pool2"; return -2; }
    }
    const bool st_kept = st_norm && d->st_keep;
    const long keep_n = (st_req || st_kept) ? up64((long)B * d->Cout * ((long)Hout * Wout / 64 + 1) * 2) : 0;
    const long small_n = (lin ? (long)B * tbs : 0) + (d->cot_d ? (long)B * up64(2L * d->Cout) : 0) + 64 + keep_n + (st_req ? up64(2L * d->Cout) : 0);
    const size_t owned0 = c->owned.size();
    const size_t bytes0 = c->bytes;
    auto release = [&]() { release_since(c, st, owned0, bytes0); };      // what this call allocated (weight layouts, small arrays)
    auto host_param = [&](const float* p, std::vector<int64_t> shape) {
        HostParam h; h.shape = shape; h.loaded = true;
        size_t n = 1; for (int64_t s : shape) n *= (size_t)s;
        if (p) h.data.assign(p, p + n); else h.data.assign(n, 0.f);
        return h;
    };
    // the module's weight: [Cout][Cin][k][k] forward, [Cin][Cout][k][k] behind the transposed (dgrad) operator
    const int m_out = d->transposed ? d->Cin : d->Cout, m_in = d->transposed ? d->Cout : d->Cin;
    HostParam w = host_param(d->weight, {m_out, m_in, k, k}), wb0 = host_param(nullptr, {m_out});
    HostParam w2 = host_param(d->Cin2 > 0 ? d->w2 : nullptr, {d->Cout, d->Cin2 > 0 ? d->Cin2 : 1, 1, 1}), wb2 = host_param(nullptr, {d->Cout});
    ConvP cp, cp2;
    float *bias_d = nullptr, *bias2nd_d = nullptr, *small = nullptr;
    const int poly_kind = taps != 9 ? -1 : (d->upsample || d->pool2) ? POLY_UP : d->zins ? ((d->pad >= 0 ? d->pad : 2) == 1 ? POLY_ZINS_PAD1 : POLY_ZINS_PAD2) : -1;
    int rc = make_conv(c, {&w}, {&wb0}, &cp, -1, poly_kind, d->transposed != 0 && !d->pool2);
    float* pool_tmp = nullptr;
    if (!rc && d->pool2) rc = dalloc(c, &pool_tmp, (size_t)B * d->Cout * d->Hin * d->Win);
    if (!rc && d->Cin2 > 0) rc = make_conv(c, {&w2}, {&wb2}, &cp2);
    if (!rc && d->bias) rc = upload(c, &bias_d, std::vector<float>(d->bias, d->bias + d->Cout));
    if (!rc && d->Cin2 > 0 && d->bias2nd) rc = upload(c, &bias2nd_d, std::vector<float>(d->bias2nd, d->bias2nd + d->Cout));
    if (!rc) rc = dalloc(c, &small, (size_t)small_n);
    if (rc) { release(); return -1; }
    auto copy = [&](float* dst, const float* src, long n) {
        return hipMemcpyAsync(dst, src, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, st);
    };
    hipError_t he = hipSuccess;
    if (d->in_arena) he = copy(c->arenaT, d->in, in_e * B);
    const TView out{d->out, out_e, d->Cout, Hout, Wout};
    ConvArgs a = conv_args(tview_in(d->in_arena ? c->arenaT : d->in, in_e, d->Cin, d->Hin, d->Win), cp, d->transposed != 0, out, B,
                           taps == 1 ? 1 : 3);
    a.bias = bias_d;
    a.bias2 = d->bias2; a.bias2_bs = d->Cout;
    a.res = d->res; a.res_bs = out_e; a.res_scale = d->res_scale;
    a.mode = d->mode; a.stride = d->stride; a.upsample = d->upsample; a.zins = d->zins; a.accumulate = d->accumulate;
    a.pad = d->pad >= 0 ? d->pad : taps == 1 ? 0 : d->zins ? 2 : d->stride == 2 ? 0 : 1;
    if (d->pool2) { a.pool2 = 1; a.pool_tmp = pool_tmp; a.pool_tmp_bs = (long)d->Cout * d->Hin * d->Win; }
    a.sc = d->sc; a.sh = d->sh; a.scsh_bs = 0; a.cpg = d->cpg;
    if (lin) {
        if (he == hipSuccess) he = copy(c->arenaP, d->prim, in_e);
        a.prim = c->arenaP; a.prim_bs = 0;
        a.mr = d->mr; a.mr_bs = 0; a.gamma_ = d->gamma;
        // per sample: the group means as given (exact-fp32 kernel), then their per-channel expansion as the statistics kernels scale it
        for (int b = 0; b < B && he == hipSuccess; ++b) he = copy(small + b * tbs, d->tst + (long)b * 2 * G, 2L * G);
        a.tst = small; a.tst_bs = tbs;
        for (int b = 0; b < B; ++b)
            hipLaunchKernelGGL(diag_scale_tc, dim3((unsigned)((d->Cin + 255) / 256)), dim3(256), 0, st, d->tc + (long)b * 2 * d->Cin, d->mr,
                               d->Cin, d->cpg, (long)d->Cin, d->mode == CM_COT_SILU ? 1 : 0, small + b * tbs + up64(2L * G));
        a.tc = small + up64(2L * G); a.tc_bs = tbs;
        launch_gn_cache(c->arenaP, d->Cin, d->Hin * d->Win, d->cpg, d->sc, d->sh, d->mr, c->sxcache, st, ACT_SILU);
        a.sx = c->sxcache;
    }
    ConvArgs n2; conv_defaults(n2);
    if (d->Cin2 > 0) {
        float* in2 = c->arenaT + offT_in2;
        if (he == hipSuccess) he = copy(in2, d->in2, in2_e * B);
        n2 = conv_args(TView{in2, in2_e, d->Cin2, Hout, Wout}, cp2, false, out, B, 1);
        n2.bias = bias2nd_d;
        a.res = d->out; a.res_bs = out_e;      // (as the ResBlock: the block output is the shortcut's output + conv2)
    }
    if (d->cot_d) {
        float* cd = c->arenaT + offT_cot;
        float* ctc = small + (lin ? (long)B * tbs : 0);
        const long cbs = up64(2L * d->Cout);
        if (he == hipSuccess) he = copy(cd, d->cot_d, out_e * B);
        for (int b = 0; b < B; ++b)
            hipLaunchKernelGGL(diag_scale_tc, dim3((unsigned)((d->Cout + 255) / 256)), dim3(256), 0, st, d->cot_tc + (long)b * 2 * d->Cout,
                               d->cot_mr, d->Cout, d->cot_cpg, (long)d->Cout, 1, ctc + b * cbs);
        launch_gn_cache(d->cot_prim, d->Cout, Hout * Wout, d->cot_cpg, d->cot_sc, d->cot_sh, d->cot_mr, c->sxcache + sx_cot, st, ACT_SILU);
        a.cot_d = cd; a.cot_d_bs = out_e; a.cot_sx = c->sxcache + sx_cot; a.cot_tc = ctc; a.cot_tc_bs = cbs;
    }
    if (he != hipSuccess) { c->err = std::string("debug_conv: ") + hipGetErrorString(he); release(); return -1; }
    std::string text;
    const int act0 = c->cfg.act;
    if (d->mode == CM_GN_GELU) c->cfg.act = ACT_GELU;      // a GELU network's forward prologue (run_conv hands cfg.act to the kernels)
    c->plan_log = &text;
    StatReq srq;
    int kept_ntile = 0;
    float* const keep_buf = small + (small_n - keep_n - (st_req ? up64(2L * d->Cout) : 0));
    if (st_req) {      // as next_tan asks for one part of a concatenation: the raw row partials stay in `keep`
        srq.kind = ST_TAN; srq.prim = d->st_prim; srq.keep = keep_buf; srq.keep_floats = (size_t)keep_n; srq.keep_ntile = &kept_ntile;
    }
    NormP stn;      // the consuming norm of a statistics request: slot 0 of the arenas, its records behind the launch's own
    if (st_norm) {
        stn.C = d->Cout; stn.soff = 0; stn.eps = d->st_eps;
        stn.gamma = const_cast<float*>(d->st_gamma); stn.beta = const_cast<float*>(d->st_beta);
        srq.kind = stk; srq.n = &stn; srq.stats = c->statsT;
        srq.ss_scale = d->st_ss_scale; srq.ss_shift = d->st_ss_shift;
        (void)hipMemsetAsync(c->statsT, 0xff, (size_t)B * SBs * sizeof(float), st);      // an unwritten slot reads as NaN
        if (st_lin) {
            NS sp = nstats(c, c->statsP, stn);
            (void)copy(sp.sc, d->st_sc, d->Cout); (void)copy(sp.sh, d->st_sh, d->Cout); (void)copy(sp.mr, d->st_mr, 2L * Gs);
            srq.prim = d->st_prim;
            if (stk == ST_COT) {
                stn.sx_off = sx_st;
                launch_gn_cache(d->st_prim, d->Cout, Hout * Wout, d->Cout / Gs, sp.sc, sp.sh, sp.mr, c->sxcache + sx_st, st, c->cfg.act);
            }
        }
        if (st_kept) { srq.keep = keep_buf; srq.keep_floats = (size_t)keep_n; srq.keep_ntile = &kept_ntile; }
    }
    bool keep_short = false;      // the kept partials did not fit st_keep_out
    const bool rode = run_conv(c, a, taps, st, (st_req || st_norm) ? &srq : nullptr, d->Cin2 > 0 ? &n2 : nullptr);
    c->plan_log = nullptr;
    c->cfg.act = act0;
    if (st_norm) {      // what the arena's slots received, per sample
        NS so = nstats(c, c->statsT, stn);
        auto rows = [&](float* dst, const float* src, long w) {
            return hipMemcpy2DAsync(dst, (size_t)w * sizeof(float), src, (size_t)SBs * sizeof(float), (size_t)w * sizeof(float), (size_t)B,
                                    hipMemcpyDeviceToDevice, st);
        };
        if (stk == ST_FWD) { (void)rows(d->st_o_mr, so.mr, 2L * Gs); (void)rows(d->st_o_sc, so.sc, d->Cout); (void)rows(d->st_o_sh, so.sh, d->Cout); }
        else { (void)rows(d->st_o_tst, so.tst, 2L * Gs); (void)rows(d->st_o_tc, so.tc, 2L * d->Cout); }
        if (st_kept && kept_ntile > 0) {
            const long n = (long)B * d->Cout * kept_ntile * 2;
            if (n <= d->st_keep_cap) (void)copy(d->st_keep_out, keep_buf, n);
            else keep_short = true;
        }
    }
    if (st_req) {
        // st_out[0]: {m1, m2} per (sample, group) from the partials the launch kept (NaN where it kept none); st_out[1]: the
        // standalone pass over the finished tensor
        const int G2 = d->Cout / d->st_cpg;
        float* const zero = keep_buf + keep_n;
        (void)hipMemsetAsync(zero, 0, (size_t)up64(2L * d->Cout) * sizeof(float), st);
        (void)hipMemsetAsync(d->st_out, 0xff, (size_t)B * G2 * 2 * sizeof(float), st);
        if (kept_ntile > 0)
            launch_gn_lin_fused_finalize(ST_TAN, keep_buf, d->Cout, kept_ntile, nullptr, 0, B, d->Cout, Hout * Wout, G2, d->st_mr, d->st_out,
                                         nullptr, 2L * G2, st);
        launch_gn_tstats(d->out, out_e, d->st_prim, 0, B, d->Cout, Hout * Wout, G2, zero, zero + d->Cout, d->st_mr, 0, 0, 0,
                         d->st_out + (long)B * G2 * 2, nullptr, 2L * G2, c->red, st, ACT_SILU);
    }
    he = hipGetLastError();
    release();
    if (he == hipSuccess) he = hipGetLastError();
    if (he != hipSuccess) { c->err = std::string("debug_conv: ") + hipGetErrorString(he); return -1; }
    if (plan && cap > 0) {
        if ((int64_t)text.size() + 1 > cap) { c->err = "debug_conv: plan buffer too small"; return -4; }
        std::memcpy(plan, text.c_str(), text.size() + 1);
    }
    if (keep_short) { c->err = "debug_conv: st_keep_out too small for the kept partials (B Cout keep_ntile 2 floats)"; return -4; }
    if (d->cot_d && !rode) { c->err = "debug_conv: norm-cotangent term declined"; return 1; }
    return 0;
}

// loco_debug_norm: one launch of one standalone GroupNorm launcher on the caller's tensors.  Only the descriptor -> argument
// mapping and the launchers' shape contract (checked here, before the launch) live here.
int loco_debug_norm(loco_ctx* c, const loco_norm_desc* d, void* stream) {
    if (!c) return -2;
    if (!d || d->struct_size != (int32_t)sizeof(loco_norm_desc)) { c->err = "debug_norm: descriptor size mismatch"; return -2; }
    if (finalize_params(c)) return -3;
    hipStream_t st = (hipStream_t)stream;
    const int op = d->op, B = d->B, C = d->C, HW = d->HW, G = d->G;
    if (op < 0 || op > 7) { c->err = "debug_norm: op is 0 ... 7"; return -2; }
    if (C < 1 || HW < 1 || G < 1 || C % G) { c->err = "debug_norm: C must be a positive multiple of G"; return -2; }
    if (op != 7 && op != 3 && B < 1) { c->err = "debug_norm: B < 1"; return -2; }
    if (op != 7 && (HW % 4)) { c->err = "debug_norm: HW must be a multiple of 4 (16-byte loads)"; return -2; }
    if (C / G > 256) { c->err = "debug_norm: more than 256 channels per group"; return -2; }
    if (op != 7 && op != 3 && (long)B * G > 8192) { c->err = "debug_norm: B G exceeds the reduction buffer"; return -2; }
    auto need = [&](std::initializer_list<const void*> ps) { for (const void* p : ps) if (!p) return false; return true; };
    const char* null_op = "debug_norm: a required operand is null";
    {   // kind, tile counts, the split of a concatenation and the scale-shift pair, each under its own name
        static const int kind_lo[8] = {0, 0, 0, 0, 0, 0, ST_TAN, 0}, kind_hi[8] = {0, 2, 5, 0, 0, 0, ST_COT, 0};
        if ((op == 1 || op == 2 || op == 6) && (d->kind < kind_lo[op] || d->kind > kind_hi[op])) {
            c->err = "debug_norm: kind out of range (gn_tstats 0 - 2, gn_apply 0 - 5, gn_lin_fused_finalize 2 / 3)"; return -2;
        }
        const bool two = op == 5 || (op == 6 && d->partB);
        if ((op == 4 || op == 5 || op == 6) && (d->ntA < 1 || HW % d->ntA || (two && (d->ntB < 1 || HW % d->ntB)))) {
            c->err = "debug_norm: tile counts must be positive and divide HW"; return -2;
        }
        if (two && (d->C1 < 1 || d->C1 >= C)) { c->err = "debug_norm: C1 must lie inside (0, C)"; return -2; }
        if ((op == 0 || op == 4) && (!d->ss_scale != !d->ss_shift)) { c->err = "debug_norm: ss_scale goes with ss_shift"; return -2; }
    }
    switch (op) {
        case 0:
            if (!need({d->x, d->gamma, d->beta, d->o_mr, d->o_sc, d->o_sh})) { c->err = null_op; return -2; }
            launch_gn_stats(d->x, d->x_bs, B, C, HW, G, d->eps, d->gamma, d->beta, d->o_mr, d->o_sc, d->o_sh, d->o_bs, c->red, st,
                            d->ss_scale, d->ss_shift);
            break;
        case 1:
            if (!need({d->d, d->x, d->sc, d->sh, d->mr, d->o_tst})) { c->err = null_op; return -2; }
            launch_gn_tstats(d->d, d->d_bs, d->x, d->x_bs, B, C, HW, G, d->sc, d->sh, d->mr, d->pbs_c, d->pbs_g, d->kind, d->o_tst,
                             d->o_tc, d->o_bs, c->red, st, d->act);
            break;
        case 2: {
            const bool lin = d->kind != 0 && d->kind != 4;
            if (!need({d->x, d->sc, d->sh, d->out}) || (lin && !need({d->d, d->mr, d->tst}))) { c->err = null_op; return -2; }
            launch_gn_apply(d->kind, d->d, d->d_bs, d->x, d->x_bs, d->base, d->base_bs, d->out, d->out_bs, d->accumulate, B, C, HW, G,
                            d->sc, d->sh, d->mr, d->pbs_c, d->pbs_g, d->tst, d->t_bs, st, d->act, d->base_scale);
            break;
        }
        case 3:
            if (!need({d->x, d->sc, d->sh, d->mr, d->out})) { c->err = null_op; return -2; }
            launch_gn_cache(d->x, C, HW, C / G, d->sc, d->sh, d->mr, reinterpret_cast<float2*>(d->out), st, d->act);
            break;
        case 4:
            if (!need({d->partA, d->gamma, d->beta, d->o_mr, d->o_sc, d->o_sh})) { c->err = null_op; return -2; }
            launch_gn_fused_finalize(d->partA, d->ntA, B, C, HW, G, d->eps, d->gamma, d->beta, d->o_mr, d->o_sc, d->o_sh, d->o_bs,
                                     d->ss_scale, d->ss_shift, st);
            break;
        case 5:
            if (!need({d->partA, d->partB, d->gamma, d->beta, d->o_mr, d->o_sc, d->o_sh})) { c->err = null_op; return -2; }
            launch_gn_fused_finalize_cat(d->partA, d->C1, d->ntA, d->partB, d->ntB, B, C, HW, G, d->eps, d->gamma, d->beta, d->o_mr,
                                         d->o_sc, d->o_sh, d->o_bs, st);
            break;
        case 6: {
            const int C1 = d->partB ? d->C1 : C;
            if (!need({d->partA, d->mr, d->o_tst})) { c->err = null_op; return -2; }
            launch_gn_lin_fused_finalize(d->kind, d->partA, C1, d->ntA, d->partB, d->ntB, B, C, HW, G, d->mr, d->o_tst, d->o_tc, d->o_bs, st);
            break;
        }
        default:
            if (!need({d->x, d->gamma, d->beta, d->out})) { c->err = null_op; return -2; }
            launch_ctx_groupnorm(d->x, HW, C, G, d->eps, d->gamma, d->beta, d->out, st);
            break;
    }
    hipError_t he = hipStreamSynchronize(st);
    if (he == hipSuccess) he = hipGetLastError();
    if (he != hipSuccess) { c->err = std::string("debug_norm: ") + hipGetErrorString(he); return -1; }
    return 0;
}

// loco_debug_pointwise: one launch of one token-wise / pointwise launcher on the caller's tensors.  Only the descriptor -> argument
// mapping and the launchers' contract (checked here, before the launch) live here.
int loco_debug_pointwise(loco_ctx* c, const loco_pointwise_desc* d, void* stream) {
    if (!c) return -2;
    if (!d || d->struct_size != (int32_t)sizeof(loco_pointwise_desc)) { c->err = "debug_pointwise: descriptor size mismatch"; return -2; }
    hipStream_t st = (hipStream_t)stream;
    const int op = d->op, B = d->B, C = d->C, T = d->T;
    const long count = d->count;
    auto fail = [&](const char* why) { c->err = std::string("debug_pointwise: ") + why; return -2; };
    auto need = [&](std::initializer_list<const void*> ps) { for (const void* p : ps) if (!p) return false; return true; };
    auto aligned = [](const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; };
    // [p, p + n) and [q, q + m) floats share an address
    auto overlap = [](const float* p, long n, const float* q, long m) { return p && q && p < q + m && q < p + n; };
    const char* null_op = "a required operand is null";
    if (op < 0 || op > 14) return fail("op is 0 ... 14");
    if (d->in_bs < 0 || d->out_bs < 0 || d->aux_bs < 0 || d->st_bs < 0) return fail("a stride is negative");
    const bool batched = op <= 3 || (op >= 6 && op <= 8) || op == 12;
    if (batched && B < 1) return fail("B < 1");
    const bool counted = op == 3 || op >= 8;
    if (counted && count < 1) return fail("count < 1");
    switch (op) {
        case 0: case 1: case 2: {
            if (C < 1) return fail("C < 1");
            if (T < 16 || T % 16) return fail("T must be a positive multiple of 16 (a workgroup owns 16 tokens)");
            if (!need({d->x, d->gamma, d->out}) || (op == 0 ? !need({d->beta, d->out2}) : !need({d->y, d->stats}))) return fail(null_op);
            const long ext = (long)C * T, xe = (long)(B - 1) * d->in_bs + ext, oe = (long)(B - 1) * d->out_bs + ext;
            const bool in_place = op == 0 && d->out == d->x && d->out_bs == d->in_bs;
            if (!in_place && overlap(d->out, oe, d->x, xe)) return fail("the output overlaps an input (only ln_fwd runs in place, out == x with equal strides)");
            if (op == 0) {
                if (B > 1 && d->st_bs < 2L * T) return fail("st_bs below 2 T: the statistics of two samples overlap");
                const long se = (long)(B - 1) * d->st_bs + 2L * T;
                if (overlap(d->out2, se, d->x, xe) || overlap(d->out2, se, d->out, oe)) return fail("the statistics overlap a tensor");
                launch_ln_fwd(d->x, d->in_bs, B, C, T, d->gamma, d->beta, d->eps, d->out, d->out_bs, d->out2, d->st_bs, st);
            } else {
                if (overlap(d->out, oe, d->y, ext) || overlap(d->out, oe, d->stats, 2L * T)
                    || overlap(d->out, oe, d->base, (long)(B - 1) * d->aux_bs + ext))
                    return fail("the output overlaps an input (only ln_fwd runs in place, out == x with equal strides)");
                if (op == 1) launch_ln_tan(d->x, d->in_bs, d->y, d->stats, B, C, T, d->gamma, d->out, d->out_bs, st);
                else launch_ln_cot(d->x, d->in_bs, d->y, d->stats, B, C, T, d->gamma, d->base, d->aux_bs, d->out, d->out_bs, st);
            }
            break;
        }
        case 3: {
            if (d->kind < 0 || d->kind > 2) return fail("geglu kind is 0 ... 2");
            if (!need({d->x, d->out}) || (d->kind != 0 && !d->y)) return fail(null_op);
            const long rd = d->kind == 2 ? count : 2 * count, wr = d->kind == 2 ? 2 * count : count;
            if (B > 1 && (d->in_bs < rd || d->out_bs < wr)) return fail("in_bs / out_bs smaller than the kind reads / writes (2 n4 or n4)");
            launch_geglu(d->kind, d->x, d->in_bs, d->y, B, count, d->out, d->out_bs, st);
            break;
        }
        case 4: {
            if (C < 1 || d->n < 1) return fail("ch or temb_ch < 1");
            if ((long)C + d->n > 16384) return fail("ch + temb_ch floats exceed the 64 KiB of LDS a workgroup may take");
            if (d->act != ACT_SILU && d->act != ACT_GELU) return fail("act is 0 (SiLU) or 1 (GELU)");
            if (!need({d->w0, d->b0, d->w1, d->b1, d->out}) || (C > 1 && !d->freq)) return fail(null_op);
            if (d->t_dev) launch_set_scalar(d->t_dev, d->t, st);
            launch_temb(d->t_dev ? 0.f : d->t, C, d->n, d->freq, d->w0, d->b0, d->w1, d->b1, d->out, st, d->cos_first, d->add, d->t_dev,
                        d->act, d->add_in);
            break;
        }
        case 5:
            if (C < 1 || d->n < 1) return fail("cout or temb_ch < 1");
            if (!need({d->x, d->w0, d->out})) return fail(null_op);
            launch_temb_proj(d->x, d->n, d->w0, d->b0, C, d->out, st);
            break;
        case 6: case 7:
            if (C < 1 || d->H < 1 || d->W < 1) return fail("C, H and W must be positive");
            if (!need({d->x, d->out})) return fail(null_op);
            if (op == 6) {
                if ((d->in_bs & 1) || !aligned(d->x, 8)) return fail("pool2x2 reads float2 pairs: in_bs must be even and x aligned to 8 bytes");
                launch_pool2x2_sum(d->x, d->in_bs, d->out, d->out_bs, d->accumulate, B, C, d->H, d->W, st, d->scale);
            } else {
                launch_upsample2x(d->x, d->in_bs, d->out, d->out_bs, d->accumulate, d->scale, B, C, d->H, d->W, st);
            }
            break;
        case 8:
            if (!need({d->x, d->out})) return fail(null_op);
            if ((count | d->in_bs | d->out_bs) & 3) return fail("copy moves float4: per_sample, in_bs and out_bs must be multiples of 4");
            if (!aligned(d->x, 16) || !aligned(d->out, 16)) return fail("copy moves float4: x and out must be aligned to 16 bytes");
            launch_copy(d->x, d->in_bs, d->out, d->out_bs, d->accumulate, B, count, st);
            break;
        case 9: case 10:
            if (d->k < 1) return fail("k < 1");
            if (d->split < 0 || d->split > d->k) return fail("split outside [0, k]");
            if (d->mask2 && !d->mask) return fail("mask2 without mask");
            if (!need({d->out}) || (op == 9 ? !d->y : !d->x)) return fail(null_op);
            if (op == 9) launch_masked_axpby(d->x, d->y, d->mask, d->cv, d->ce, d->out, d->k, count, st, d->mask2, d->split);
            else launch_cot_seed(d->x, d->mask, d->cv, d->ce, d->out, d->out2, d->k, count, st, d->mask2, d->split);
            break;
        case 11:
            if (!need({d->x, d->y, d->out})) return fail(null_op);
            launch_ddim_step(d->x, d->y, d->base, d->out, d->out2, count, d->f[0], d->f[1], d->f[2], d->f[3], d->f[4], st);
            break;
        case 12:
            if (!need({d->x, d->out})) return fail(null_op);
            launch_latent_sample(d->x, d->base, d->scale, d->out, B, count, st);
            break;
        case 13: {
            if (d->n < 1 || d->n > 4) return fail("lincomb takes n = 1 ... 4 sources");
            if (!d->out) return fail(null_op);
            if (!aligned(d->out, 16)) return fail("lincomb moves float4: every pointer must be aligned to 16 bytes");
            for (int i = 0; i < d->n; ++i) {
                if (!d->src[i]) return fail(null_op);
                if (!aligned(d->src[i], 16)) return fail("lincomb moves float4: every pointer must be aligned to 16 bytes");
            }
            launch_lincomb(d->src, d->f, d->n, d->out, count, st);
            break;
        }
        default:
            if (!need({d->x, d->y, d->out})) return fail(null_op);
            launch_add(d->x, d->y, d->out, count, st);
            break;
    }
    hipError_t he = hipStreamSynchronize(st);
    if (he == hipSuccess) he = hipGetLastError();
    if (he != hipSuccess) { c->err = std::string("debug_pointwise: ") + hipGetErrorString(he); return -1; }
    return 0;
}

// loco_debug_attn: one pass of one attention stage on the caller's tensors, through attn_forward / attn_tangent / attn_cotangent or
// xa_forward / xa_linear -- the engine's own functions, so the route (flash, record GEMM, bf16x3, fused cross-attention) is the
// product's.  Only the descriptor -> Attn / XA mapping and the scratch live here.
int loco_debug_attn(loco_ctx* c, const loco_attn_desc* d, char* route, int64_t cap, void* stream) {
    if (!c) return -2;
    if (!d || d->struct_size != (int32_t)sizeof(loco_attn_desc)) { c->err = "debug_attn: descriptor size mismatch"; return -2; }
    hipStream_t st = (hipStream_t)stream;
    const int T = d->T, NH = d->NH, CH = d->CH, B = d->B, L = d->L;
    const bool cross = d->kind == 1;
    if ((d->kind != 0 && d->kind != 1) || d->pass < 0 || d->pass > 2) { c->err = "debug_attn: kind is 0 / 1, pass 0 / 1 / 2"; return -2; }
    if (CH < 1) { c->err = "debug_attn: CH < 1"; return -2; }
    if (T < 64 || T % 64) { c->err = "debug_attn: T must be a multiple of 64 (the row kernels and the tiles of the fused kernels)"; return -2; }
    if (NH < 1 || B < 1) { c->err = "debug_attn: NH and B must be positive"; return -2; }
    if (!cross && (d->Lt < 0 || d->Lt % 64)) { c->err = "debug_attn: Lt must be a multiple of 64"; return -2; }
    if (!cross && (L < 0 || L > d->Lt || (d->Lt > 0 && L < 1))) { c->err = "debug_attn: L must lie in 1 ... Lt"; return -2; }
    if (cross && L < 1) { c->err = "debug_attn: the cross-attention needs L >= 1 context rows"; return -2; }
    const int Lt = cross ? ((L + 63) / 64) * 64 : d->Lt;        // cross: Lp, the padded row length (program.hip: ctx_Lp)
    const bool text = cross || Lt > 0;
    bool have = d->P && (!text || (d->kt && d->vt));
    if (!cross) have = have && d->q && d->k && d->v && d->o;
    if (d->pass == 0) have = have && d->o;
    if (d->pass == 0) have = have && d->q;
    if (d->pass == 1) have = have && d->dq && d->out && (cross || (d->dk && d->dv));
    if (d->pass == 2) have = have && d->go && d->gq && (cross || (d->gk && d->gv));
    if (!have) { c->err = "debug_attn: a required operand is null"; return -2; }
    const long CT = (long)NH * CH * T, SB = (long)NH * T * (cross ? Lt : Lt + T);
    const size_t owned0 = c->owned.size(), bytes0 = c->bytes;
    auto release = [&]() { release_since(c, st, owned0, bytes0); };      // what this call allocated
    float* colbias = nullptr;
    if (text) {
        std::vector<float> cb((size_t)Lt, 0.f);
        for (int l = L; l < Lt; ++l) cb[l] = -1e30f;
        if (upload(c, &colbias, cb)) { release(); return -1; }
    }
    std::string text_log;
    float* scratch = nullptr;
    if (cross) {
        XA x; x.c = c; x.st = st; x.B = B; x.C = NH * CH; x.T = T; x.NH = NH; x.CH = CH; x.L = L; x.Lp = Lt;
        x.scale = 1.0f / std::sqrt((float)CH);
        x.xK = d->kt; x.xV = d->vt; x.colbias = colbias; x.xs = CT; x.ss = SB;
        if (d->pass != 0 && dalloc(c, &scratch, (size_t)B * SB)) { release(); return -1; }
        c->attn_log = &text_log;
        if (d->pass == 0) xa_forward(x, d->q, d->P, d->o);
        else if (d->pass == 1) xa_linear(x, d->dq, x.xK, x.xV, d->P, scratch, d->out);        // dq -> do
        else xa_linear(x, d->go, x.xV, x.xK, d->P, scratch, d->gq);                             // g_o -> g_q
    } else {
        Attn s; s.c = c; s.st = st; s.B = B; s.T = T; s.NH = NH; s.CH = CH; s.Lt = Lt; s.Tk = Lt + T;
        s.HS = (long)CH * T; s.SS = (long)T * s.Tk; s.OS = (long)CH * T; s.KS = (long)CH * Lt;      // q, k, v: tensors of their own
        s.scale = 1.0f / std::sqrt((float)CH);
        s.pair = d->pair != 0;
        s.q = d->q; s.k = d->k; s.v = d->v; s.P = d->P; s.o = d->o;
        s.bq = CT; s.bS = SB; s.bo = CT;
        s.kt = d->kt; s.vt = d->vt; s.colbias = colbias;
        s.delta = nullptr; s.ws = nullptr; s.ws_bytes = 0;
        s.tq = s.tk = s.tv = s.tS = s.to = nullptr;
        if (d->pass == 0) {
            s.tq = const_cast<float*>(d->q); s.tk = const_cast<float*>(d->k); s.tv = const_cast<float*>(d->v); s.tS = d->P; s.to = d->o;
        } else {
            if (d->pass == 1) { s.tq = const_cast<float*>(d->dq); s.tk = const_cast<float*>(d->dk); s.tv = const_cast<float*>(d->dv); s.to = d->out; }
            else { s.tq = d->gq; s.tk = d->gk; s.tv = d->gv; s.to = const_cast<float*>(d->go); }
            if (s.flash()) {
                AttnFlashArgs fa = attn_flash_args(s);
                const size_t need = attn_flash_ws_bytes(fa);
                float* wsf = nullptr;
                if (dalloc(c, &s.delta, (size_t)B * NH * T) || (!d->no_workspace && dalloc(c, &wsf, need / sizeof(float) + 16384))) { release(); return -1; }
                if (wsf) { s.ws = reinterpret_cast<unsigned char*>(wsf); s.ws_bytes = need; }
            } else {
                if (dalloc(c, &scratch, (size_t)B * SB)) { release(); return -1; }
                s.tS = scratch;
            }
        }
        c->attn_log = &text_log;
        if (d->pass == 0) attn_forward(s);
        else if (d->pass == 1) attn_tangent(s);
        else attn_cotangent(s);
    }
    c->attn_log = nullptr;
    hipError_t he = hipGetLastError();
    release();
    if (he == hipSuccess) he = hipGetLastError();
    if (he != hipSuccess) { c->err = std::string("debug_attn: ") + hipGetErrorString(he); return -1; }
    if (route && cap > 0) {
        if ((int64_t)text_log.size() + 1 > cap) { c->err = "debug_attn: route buffer too small"; return -4; }
        std::memcpy(route, text_log.c_str(), text_log.size() + 1);
    }
    return 0;
}

// loco_debug_gemm: one call of one GEMM launcher on the caller's tensors.  Only the descriptor -> GemmArgs mapping, the bounds of
// every operand (checked here, before the launch) and the route text live here; the text is written from the functions the
// launchers branch on.
int loco_debug_gemm(loco_ctx* c, const loco_gemm_desc* d, char* route, int64_t cap, void* stream) {
    if (!c) return -2;
    if (!d || d->struct_size != (int32_t)sizeof(loco_gemm_desc)) { c->err = "debug_gemm: descriptor size mismatch"; return -2; }
    hipStream_t st = (hipStream_t)stream;
    const int op = d->op;
    if (op < 0 || op > 4) { c->err = "debug_gemm: op is 0 ... 4"; return -2; }
    if (d->act < 0 || d->act > 2 || (d->act && op != 1)) { c->err = "debug_gemm: act is 0 / 1 / 2 and goes with op 1 only"; return -2; }
    const int nprob = op == 4 ? 2 : 1;
    GemmArgs g[2];
    int64_t c_span[2] = {0, 0};
    for (int i = 0; i < nprob; ++i) {
        const loco_gemm_prob& p = d->p[i];
        if (p.M < 1 || p.N < 1 || p.K < 1 || p.batch < 1) { c->err = "debug_gemm: M, N, K and batch must be positive"; return -2; }
        if (!p.A || !p.B || !p.C || (!p.A2 != !p.B2)) { c->err = "debug_gemm: a required operand is null"; return -2; }
        const int64_t nb2 = p.batch2 > 0 ? p.batch2 : 1;
        const int64_t strides[] = {p.sam, p.sak, p.sab, p.sah, p.sbk, p.sbn, p.sbb, p.sbh, p.scm, p.scn, p.scb, p.sch, p.srb, p.sab2, p.sbb2};
        for (int64_t s : strides)
            if (s < 0 || s > ((int64_t)1 << 28)) { c->err = "debug_gemm: a stride is negative or beyond 2^28"; return -2; }      // (offsets stay far inside int64)
        const int64_t M1 = p.M - 1, N1 = p.N - 1, K1 = p.K - 1, B1 = p.batch - 1, H1 = nb2 - 1;
        const int64_t c_last = M1 * p.scm + N1 * p.scn + H1 * p.sch;
        auto inside = [&](const void* ptr, int64_t last, int64_t count) { return !ptr || (count > 0 && last < count); };
        if (!inside(p.A, M1 * p.sam + K1 * p.sak + H1 * p.sah + B1 * p.sab, p.n_A) ||
            !inside(p.B, K1 * p.sbk + N1 * p.sbn + H1 * p.sbh + B1 * p.sbb, p.n_B) ||
            !inside(p.A2, M1 * p.sam + K1 * p.sak + H1 * p.sah + B1 * p.sab2, p.n_A2) ||
            !inside(p.B2, K1 * p.sbk + N1 * p.sbn + H1 * p.sbh + B1 * p.sbb2, p.n_B2) ||
            !inside(p.C, c_last + B1 * p.scb, p.n_C) || !inside(p.R, c_last + B1 * p.srb, p.n_R) ||
            !inside(p.bias, M1, p.n_bias) || !inside(p.colbias, N1, p.n_colbias)) {
            c->err = "debug_gemm: an operand's largest addressed offset is outside its buffer"; return -2;
        }
        c_span[i] = c_last + B1 * p.scb + 1;
        if (d->act && p.A2) { c->err = "debug_gemm: launch_gemm_fixed applies no activation to a two-segment product (act with A2)"; return -2; }
        if (op == 3 && (p.bias || p.colbias || p.R)) { c->err = "debug_gemm: launch_gemm_rec has no bias, colbias or R"; return -2; }
        if (op == 3 && (p.K < 256 || p.M < 128 || p.N < 256)) { c->err = "debug_gemm: launch_gemm_rec needs K >= 256, M >= 128, N >= 256"; return -2; }
        if (op == 4 && p.A2) { c->err = "debug_gemm: launch_gemm_pair takes single-segment problems (A2 set)"; return -2; }
        GemmArgs& a = g[i];
        std::memset(&a, 0, sizeof(a));
        a.A = p.A; a.sam = p.sam; a.sak = p.sak; a.sab = p.sab;
        a.Bm = p.B; a.sbk = p.sbk; a.sbn = p.sbn; a.sbb = p.sbb;
        a.C = p.C; a.scm = p.scm; a.scn = p.scn; a.scb = p.scb;
        a.bias = p.bias; a.colbias = p.colbias; a.R = p.R; a.srb = p.srb;
        a.M = p.M; a.N = p.N; a.K = p.K; a.batch = p.batch; a.alpha = p.alpha; a.beta = p.beta;
        a.batch2 = p.batch2; a.sah = p.sah; a.sbh = p.sbh; a.sch = p.sch;
        a.A2 = p.A2; a.sab2 = p.sab2; a.Bm2 = p.B2; a.sbb2 = p.sbb2;
    }
    if (op == 4) {
        const float *lo0 = g[0].C, *hi0 = lo0 + c_span[0], *lo1 = g[1].C, *hi1 = lo1 + c_span[1];
        if (lo0 < hi1 && lo1 < hi0) { c->err = "debug_gemm: the outputs of the two problems overlap"; return -2; }
    }
    std::string text;
    auto note = [&](const char* kernel, const GemmArgs& a, int tm, int ksplit) {
        char line[224];
        snprintf(line, sizeof(line), "kernel=%s M=%d N=%d K=%d batch=%d heads=%d nseg=%d akm=%d bkm=%d tm=%d ksplit=%d\n", kernel, a.M, a.N,
                 a.K, a.batch, a.batch2 > 0 ? a.batch2 : 1, a.A2 ? 2 : 1, a.sam == 1 ? 1 : 0, a.sbn == 1 ? 1 : 0, tm, ksplit);
        text += line;
    };
    static const char* const f32_name[3] = {"gemm_f32_64", "gemm_f32_small", "gemm_f32_small_pipe"};
    void* ws = nullptr;
    switch (op) {
        case 0: note(f32_name[gemm_f32_variant(g[0])], g[0], 0, 0); launch_gemm(g[0], st); break;
        case 1: note("gemm_f32_fixed", g[0], 0, 0); launch_gemm_fixed(g[0], d->act, st); break;
        case 2: note(gemm_bf16x3_tile(g[0]) == 128 ? "gemm_bf16x3_128" : "gemm_bf16x3_64", g[0], 0, 0); launch_gemm_bf16x3(g[0], st); break;
        case 3: {
            const GemmRecRoute rt = gemm_rec_route(g[0]);
            char line[96];
            for (int o = 0; o < (g[0].A2 ? 4 : 2); ++o) {
                snprintf(line, sizeof(line), "kernel=rec_split operand=%d kcontig=%d z=%d\n", o, rt.kcontig[o], rt.z[o]);
                text += line;
            }
            note("gemm_rec", g[0], rt.tm, rt.ksplit);
            if (rt.ksplit > 1) { snprintf(line, sizeof(line), "kernel=gemm_rec_reduce ksplit=%d\n", rt.ksplit); text += line; }
            if (hipMalloc(&ws, gemm_rec_ws_bytes(g[0])) != hipSuccess) { (void)hipGetLastError(); c->err = "debug_gemm: workspace allocation failed"; return -1; }
            launch_gemm_rec(g[0], static_cast<unsigned char*>(ws), st);
            break;
        }
        default:
            if (gemm_pair_grouped(g[0], g[1])) { note("gemm_f32_pair", g[0], 0, 0); note("gemm_f32_pair", g[1], 0, 0); }
            else { note(f32_name[gemm_f32_variant(g[0])], g[0], 0, 0); note(f32_name[gemm_f32_variant(g[1])], g[1], 0, 0); }
            launch_gemm_pair(g[0], g[1], st);
            break;
    }
    hipError_t he = hipStreamSynchronize(st);
    if (ws) (void)hipFree(ws);
    if (he == hipSuccess) he = hipGetLastError();
    if (he != hipSuccess) { c->err = std::string("debug_gemm: ") + hipGetErrorString(he); return -1; }
    if (route && cap > 0) {
        if ((int64_t)text.size() + 1 > cap) { c->err = "debug_gemm: route buffer too small"; return -4; }
        std::memcpy(route, text.c_str(), text.size() + 1);
    }
    return 0;
}

int64_t loco_debug_tensor(loco_ctx* c, const char* name, float* dst, int64_t cap, void* stream) {
    if (!c) return -2;
    std::string nm(name);
    if (nm == "bench_out") {     // the output tensor of the last loco_bench_conv ([B][Cout][H][W])
        if (!c->bench_out) { c->err = "no loco_bench_conv yet"; return -3; }
        int64_t cnt = cap < c->bench_out_count ? cap : c->bench_out_count;
        HIPCHK(c, hipMemcpyAsync(dst, c->bench_out, (size_t)cnt * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
        return cnt;
    }
    if (nm == "workspace") {     // head of the split-K workspace (diagnostic kernels leave their cycle stamps there)
        int64_t cnt = cap < (int64_t)c->partial_floats ? cap : (int64_t)c->partial_floats;
        HIPCHK(c, hipMemcpyAsync(dst, c->partial, (size_t)cnt * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
        return cnt;
    }
    int arena = 0;   // "T:" prefix selects the tangent/cotangent arena, "h1:" the conv1 output of a block
    if (nm.rfind("T:", 0) == 0) { arena = 1; nm = nm.substr(2); }
    bool want_h1 = false;
    if (nm.rfind("h1:", 0) == 0) { want_h1 = true; nm = nm.substr(3); }
    for (auto& op : c->ops) {
        if (op.name != nm) continue;
        int id = want_h1 ? op.h1 : op.out;
        if (id < 0) return -3;
        const Tens& t = c->tens[id];
        int64_t cnt = (int64_t)t.C * t.H * t.W;
        int B = arena ? 1 : (c->primal_B > 0 ? c->primal_B : 1);
        if (cnt * B > cap) { c->err = "debug buffer too small"; return -4; }
        float* base = (arena ? c->arenaT : c->arenaP) + t.off;
        launch_copy(base, c->prog->per_sample, dst, cnt, 0, B, cnt, (hipStream_t)stream);
        return cnt * B;
    }
    c->err = "no such op: " + nm;
    return -3;
}

}  // extern "C"
