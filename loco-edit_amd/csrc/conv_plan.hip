// Launch policy of the convolutions: tile, split-K factor, kernel family, tail-probe split, K-concatenated shortcut, statistics
// route and norm-cotangent term -- decided here and nowhere else.  Host code only (no kernels, no HIP calls).
//
// Known inconsistencies, kept as measured (changing them changes speed: a performance change of its own):
//   - the split-K factor of stride-2 launches is sized on the 256-pixel tile (conv_bf16_pick_nsplit) while they run the
//     128-pixel one (bf16_tile_of);
//   - the whole-rounds tests of the tail-probe split and of the norm-cotangent term count 128-cout tiles (short_tail, also
//     for launches on the 64- and 32-cout tiles).
#include "kernels.h"
#include <cstdio>
#include <cstdlib>

namespace loco {

constexpr int BKC = 16;   // channels per K chunk of the low-precision kernels
constexpr int BKF = 8;    // ... of the exact-fp32 kernel

// tile variants: 0: 128 x 128, 1: 128 x 64, 2: 32 x 128, 3: 64 x 64, 4: 128 x 256 (four waves, mapped to 5), 5: 128 x 256;
// couts x pixels
static const int kMT[6] = {128, 128, 32, 64, 128, 128}, kNT[6] = {128, 64, 128, 64, 256, 256};

static int env_int(const char* name, int dflt) {
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
}
// the exact-fp32 kernel's tiles (variants 0 - 3)
static int pick_tile(int Cout, int HW) {
    if (HW >= 128) return Cout > 32 ? 0 : 2;
    return Cout > 64 ? 1 : 3;      // HW == 64
}

static int conv_pick_nsplit(int Cin, int Cout, int Hout, int Wout, int B) {
    const int t = pick_tile(Cout, Hout * Wout);
    long blocks = (long)((Hout * Wout) / kNT[t]) * ((Cout + kMT[t] - 1) / kMT[t]) * B;
    int nchunks = (Cin + BKF - 1) / BKF;
    if (blocks >= 384 || nchunks < 8) return 1;
    int want = (int)((512 + blocks - 1) / blocks);
    int maxs = nchunks / 4;            // at least 4 chunks (32 channels) per split
    if (want > maxs) want = maxs;
    if (want > 32) want = 32;
    return want < 1 ? 1 : want;
}

// B = samples of the launch (NOT multiplied by a split-K factor: the choice must not depend on the factor it determines)
static int conv_bf16_pick_tile(int Cout, int HW, int B, int tile_override) {
    // single-sample passes (the B = 1 inversion / to-t chains) up to 32 x 32: 64 x 64 tiles fill the chip with a quarter of the
    // split-K of the 128 x 256 tile (4.29 vs 4.51 ms per evaluation; probe groups of 2 - 3 samples measured no gain)
    if (B <= 1 && HW <= 1024 && HW >= 64 && (Cout % 64) == 0) return 3;
    int t = pick_tile(Cout, HW);
    if (t == 0 && HW >= 256) {
        if (tile_override >= 0) return tile_override;
        return 5;      // 128 x 256 tile, 8 waves: fastest measured variant down to 160 workgroups
    }
    return t;
}

// 1x1 operators on B >= 2 run the 128 x 128 tile of four waves (two workgroups per CU: one's write-out under the other's K
// loop) instead of 128 x 256: r05, 5 probes: 256 -> 256 @128^2 74.7 -> 63.5 us, 512 -> 512 @64^2 73.2 -> 64.7, 128 -> 128 @256^2
// 87.2 -> 81.5 (headline step 290.8 -> 289.2 ms up to 128^2; with the stage loop freed of its address arithmetic also at 256^2, -0.3 %)
constexpr int kTile0MaxHW = 65536;

static int bf16_tile_of(const ConvArgs& a, int tile_override = -1) {
    int tile = conv_bf16_pick_tile(a.Cout, a.Hout * a.Wout, a.B, tile_override);
    if (tile == 4) tile = 5;
    if (tile == 5 && a.taps == 1 && !a.gemm && a.B >= 2 && a.Hout * a.Wout <= kTile0MaxHW) return 0;
    if (a.stride == 2 && tile == 5) tile = 0;   // the double-buffered stride-2 halo of a 256-pixel tile exceeds LDS
    return tile;
}
static int tile_for(const ConvArgs& a, int prec, int tile_override) {
    return prec ? bf16_tile_of(a, tile_override) : pick_tile(a.Cout, a.Hout * a.Wout);
}
// (polyphase: a workgroup finishes 256 low-resolution pixels in both column phases = 512 output pixels of 64 channels; its
//  epilogue statistics are per channel row, so whole 128-cout tiles of the lock-step kernel are whole tiles of it too)
static int conv_bf16_tile_pixels(const ConvArgs& a) { return a.poly == 1 ? 512 : a.gemm ? 256 : kNT[a.tile]; }
int conv_bf16_tile_couts(const ConvArgs& a) { return a.gemm ? 64 * a.gemm_tm : kMT[a.tile]; }

// Polyphase form of the 3x3 convs over a nearest-x2 or zero-inserted input (conv_bf16_kernel.h, TAPS = 4): per output phase a
// 2x2 conv of the low-resolution tensor on folded weights (polyphase_fold) -- 16 tap products per low-resolution pixel where the
// 3x3 route issues 36, on the vector staging of an arena tensor instead of the per-pixel staging that fabricates the duplicates /
// zeros.  Raw launches of whole 128-cout tiles on maps of whole 32 x 8 low-resolution tiles, probe batches, never split-K; the
// epilogue takes bias, bias2 and accumulate, no residual.  LOCO_POLYPHASE=0: the 3x3 route.
static bool conv_poly_ok(const ConvEnv& e, const ConvArgs& a, int taps) {
    static const bool on = env_int("LOCO_POLYPHASE", 1) != 0;
    if (!on || e.prec < 1 || taps != 9 || a.mode != CM_NONE || !(a.upsample || a.zins) || a.stride != 1) return false;
    if (!(e.prec == 2 ? a.wph : a.wpb) || !a.in_padded || a.res || a.Cin2 > 0 || a.cot_d) return false;
    if (a.upsample ? a.pad != 1 : (a.pad != 1 && a.pad != 2)) return false;
    if ((a.Cin % BKC) != 0 || (a.Cout % 128) != 0 || a.B < 2) return false;
    if (a.Hin * a.Win < 4096 || a.Win < 32 || (a.Win % 32) != 0 || (a.Hin % 8) != 0) return false;
    return a.Hout == 2 * a.Hin && a.Wout == 2 * a.Win;
}
// The up conv's cotangent, pool2x2_sum(conv3x3_pad1(g)) (ConvArgs::pool2), as ONE launch of the polyphase input form: a 4x4
// stride-2 conv, 16 tap products per low-resolution pixel for the 36 of the 3x3 conv at full resolution, no full-resolution
// intermediate and no pooling pass.  Same shape rules as conv_poly_ok on the low-resolution (output) map.
static bool conv_poly_in_ok(const ConvEnv& e, const ConvArgs& a, int taps) {
    static const bool on = env_int("LOCO_POLYPHASE", 1) != 0;
    if (!on || e.prec < 1 || taps != 9 || a.mode != CM_NONE || !a.pool2 || a.upsample || a.zins || a.stride != 1 || a.pad != 1) return false;
    if (!(e.prec == 2 ? a.wqh : a.wqb) || a.res || a.bias2 || a.Cin2 > 0 || a.cot_d) return false;
    if ((a.Cin % BKC) != 0 || (a.Cout % 128) != 0 || a.B < 2 || ((a.Hin | a.Win) & 1)) return false;
    if (a.Hout * a.Wout < 4096 || a.Wout < 32 || (a.Wout % 32) != 0 || (a.Hout % 8) != 0) return false;
    return a.Hin == 2 * a.Hout && a.Win == 2 * a.Wout;
}

// split-K factor for the split-bf16 kernels: splitting costs a partial round trip + a reduce launch, so only
// split when the un-split grid would leave more than half of the CUs idle
static int conv_bf16_pick_nsplit(int Cin, int Cout, int Hout, int Wout, int B, int chip_share, int taps, int lanes) {
    const int HW = Hout * Wout;
    int t = conv_bf16_pick_tile(Cout, HW, B, -1);
    if (t == 4) t = 5;
    // (the 1x1 operators' 128 x 128 tile: bf16_tile_of -- twice the workgroups of the 128 x 256 tile this count assumed until round 6)
    if (taps == 1 && t == 5 && B >= 2 && HW <= kTile0MaxHW) t = 0;
    long blocks = (long)(HW / kNT[t]) * ((Cout + kMT[t] - 1) / kMT[t]) * B;
    int nchunks = (Cin + BKC - 1) / BKC;
    // Workgroups a launch should reach: one per CU, or one per CU of the launch's SHARE of the chip -- two guidance branches
    // enqueue their passes side by side on two streams (tloco.BranchStreams -> loco_set_chip_share(ctx, 2)): each launch then
    // has about half of the chip, and half the splits mean half the partial traffic and reduce work (config 5: 315 -> 296 ms
    // per solve).
    // (lanes == 2: the launch belongs to one of the two probe groups a pass runs side by side on two streams (run_lanes): the other
    //  group's launches want CUs too, and a factor that fills all 256 serialises the two -- 240 measured best, 251.2 - 251.6 against
    //  253.5 - 254.0 ms per step at 256 and 251.5 - 252.5 at 224; on ONE stream 256 is: 259.2 - 259.8 against 260.4 - 261.2 at 224)
    int target = chip_share > 1 ? 256 / chip_share : (lanes == 2 ? 240 : 256);
    if (target < 32) target = 32;
    // (aiming the two-per-CU 1x1 tile at two workgroups per CU measured +0.5 %: more partial traffic than overlap)
    if (blocks >= target / 2 || nchunks < 8) return 1;
    // Round 6: the LARGEST factor whose workgroups still fit the target in one round (floor).  The rounded-up quotient put 20 tiles x
    // 13 splits = 260 workgroups on 256 CUs (1024 -> 512 @16^2, 5 probes): four of them ran as a second round of a launch whose
    // workgroups hold one CU each, and 86 - 127 tiles got 3 splits = two rounds of thirds instead of one round of halves.
    int want = (int)(target / blocks);
    int maxs = nchunks / 4;            // at least 4 chunks per split
    if (want > maxs) want = maxs;
    if (want > 32) want = 32;
    return want < 1 ? 1 : want;
}

static bool conv_lowp_can_kcat(const ConvArgs& a) {
    static const bool on = env_int("LOCO_KCAT", 1) != 0;
    return on && a.Cin2 > 0 && a.nsplit == 1 && bf16_tile_of(a) == 5 && a.stride == 1 && !a.upsample && !a.zins && a.pad == 1 &&
           (a.Cin % BKC) == 0 && (a.Cin2 % BKC) == 0 && a.in_padded &&
           (a.mode == CM_GN_SILU || a.mode == CM_GN_GELU || a.mode == CM_TAN_SILU);
}
// the epilogue statistics exist on the LDS-staged path of whole cout tiles (conv_bf16_kernel.h) and need the finished
// sums, i.e. no split-K
static bool conv_lowp_can_fuse_stats(const ConvArgs& a) {
    return a.nsplit <= 1 && !a.gemm && (a.Cout % conv_bf16_tile_couts(a)) == 0;      // (the DMA-fed GEMM's epilogue takes none)
}

// The 16x16x32 tap-pair kernel (conv_pair_kernel.h, round 6) takes the launches the 128 x 256 tile of the lock-step kernel would
// take when the shape allows: 3x3, stride 1, padded arena input, whole 16-channel chunks in an even number, whole 128-cout tiles,
// image rows a multiple of the 32-pixel tile width, no split-K, no K-concatenated shortcut, from 128^2 up (r06,
// tests/diag/pair_check.py, 5 probes: -5.7 ... -6.2 % raw, -1.3 ... -5.6 % forward, -1.4 ... -4.0 % tangent / cotangent at 256^2
// and 128^2; +-1 % at 64^2, where its two-latency prologue shows).  LOCO_CONV_PAIR=0: the 32x32x16 kernel.
static bool conv_pair_ok(const ConvArgs& a) {
    static const bool on = env_int("LOCO_CONV_PAIR", 1) != 0;
    if (!on || a.poly || a.Hout * a.Wout < 16384 || a.taps != 9 || a.Cin2 > 0 || a.nsplit != 1 || a.stride != 1 || a.upsample || a.zins ||
        a.pad != 1 || !a.in_padded || (a.Cin % (2 * BKC)) != 0 || (a.Cout % 128) != 0 || (a.Wout % 32) != 0 || (a.Hout % 8) != 0)
        return false;
    if (!(a.mode == CM_NONE || a.mode == CM_GN_SILU || a.mode == CM_TAN_SILU || a.mode == CM_COT_SILU)) return false;
    return a.tile == 5;
}

// `a` restricted to its samples nb .. B - 1
static ConvArgs conv_shift_batch(const ConvArgs& a, int nb) {
    ConvArgs t = a;
    t.B = a.B - nb;
    t.in += (long)nb * a.in_bs; t.out += (long)nb * a.out_bs;
    if (t.prim) t.prim += (long)nb * a.prim_bs;
    if (t.bias2) t.bias2 += (long)nb * a.bias2_bs;
    if (t.res) t.res += (long)nb * a.res_bs;
    if (t.sc) { t.sc += (long)nb * a.scsh_bs; t.sh += (long)nb * a.scsh_bs; }
    if (t.mr) t.mr += (long)nb * a.mr_bs;
    if (t.tst) t.tst += (long)nb * a.tst_bs;
    if (t.tc) t.tc += (long)nb * a.tc_bs;
    if (t.in2) t.in2 += (long)nb * a.in2_bs;
    if (t.cot_d) { t.cot_d += (long)nb * a.cot_d_bs; t.cot_tc += (long)nb * a.cot_tc_bs; }
    if (t.st_part) t.st_part += (long)nb * a.Cout * ((a.Hout * a.Wout) / conv_bf16_tile_pixels(a)) * 2;
    return t;
}

// Compute-shaped 1x1 operators on the DMA-fed GEMM kernel: eligibility, the cout tile and the split-K factor (overwrites
// a.nsplit); else the launch stays on the per-pixel kernel with the split-K factor it had.  LOCO_CONV_GEMM=0 switches it off (A/B).
static void conv_gemm_plan(ConvArgs& a) {
    static const bool on = env_int("LOCO_CONV_GEMM", 1) != 0;
    a.gemm = 0;
    const long HW = (long)a.Hout * a.Wout;
    if (!on || a.stride != 1 || a.upsample || a.zins || (a.Cin % BKC) != 0 || a.Cin < 320 || (HW % 256) != 0 || (a.Wout % 16) != 0 ||
        a.Cout < 128 || !a.partial || a.Cin2 > 0 || !(a.mode == CM_NONE || a.mode == CM_GN) || a.cot_d)
        return;      // (cot_d: the norm-cotangent term lives in the per-pixel 1x1 kernels' epilogue; this kernel's takes neither it nor statistics)
    {   // the kernel's 256-pixel tile is TW = min(Wout, 32) columns x 256 / TW rows: both must divide the map (a 48 x 48 map passes
        // the tests above and would be walked out of bounds: ADVICE r05)
        const int TW = a.Wout < 32 ? a.Wout : 32;
        if ((256 % TW) != 0 || (a.Wout % TW) != 0 || (a.Hout % (256 / TW)) != 0) return;
    }
    // Where it pays (tests/diag/gemm_check.py, 5 probes, us per launch old -> new incl. the split pass): the split pass costs 8 bytes
    // per input element, so the map must have many cout tiles to spread it over (320 -> 2560 @64^2 190 -> 150, 640 -> 5120 @32^2
    // 180 -> 121, 1280 -> 10240 @16^2 164 -> 104) or be one of the K-heavy, pixel-poor maps the per-pixel kernel runs at 64 - 118
    // TFLOP/s behind split-K (2560 -> 640 @32^2 144 -> 125, 5120 -> 1280 @16^2 272 -> 82).  It does not pay for the q/k/v maps
    // (3 C couts: 84 -> 105), the C -> C maps and the wide-input, narrow-output maps at 64^2 (2560 -> 320: 160 -> 218).
    static const int all_shapes = env_int("LOCO_GEMM_ALL", 0);      // LOCO_GEMM_ALL=1: every eligible shape (A/B)
    if (!all_shapes && !(a.Cout >= 640 && (a.Cout >= 4 * a.Cin || a.Cin >= 2560))) return;
    // cout tile: 256 where the padding to whole tiles costs < 10 %, else 128
    const int pad256 = (a.Cout + 255) / 256 * 256;
    const int tm = (pad256 * 10 <= a.Cout * 11) ? 4 : 2;
    const int mt = 64 * tm;
    const long tiles = (HW / 256) * ((a.Cout + mt - 1) / mt) * a.B;
    const size_t rec_floats = (size_t)a.B * a.Cin * HW;
    int ns = 1;
    if (tiles < 192) {
        const int nchunks = a.Cin / BKC;
        ns = (int)((256 + tiles - 1) / tiles);
        if (ns > 8) ns = 8;
        while (ns > 1 && nchunks / ns < 8) --ns;
        while (ns > 1 && (size_t)ns * a.B * a.Cout * HW + rec_floats > a.partial_floats) --ns;
    }
    if ((ns > 1 ? (size_t)ns * a.B * a.Cout * HW : 0) + rec_floats > a.partial_floats) return;
    a.gemm = 1; a.gemm_tm = tm; a.nsplit = ns;
}

void conv_plan_family(ConvArgs& a, int prec) {
    if (prec == 1 && a.taps == 1) conv_gemm_plan(a);     // compute-shaped 1x1 operators (the transformer's linear layers)
}

void conv_plan_tile_pair(ConvArgs& a, int prec, int tile_override) {
    a.tile = tile_for(a, prec, tile_override);
    a.pair = prec == 1 && conv_pair_ok(a);
}

// the grid of B probes x `per_probe` workgroups (128-cout tiles) ends in a short round of r <= 160 workgroups (tail_split)
static bool short_tail(long per_probe, int B) {
    const long total = per_probe * B, r = total % 256;
    return total > 256 && r > 0 && r <= 160;
}

// Tail-probe split (low precision): when the workgroups of the launch fill whole rounds of the 256 CUs plus a short tail made of
// the last probes (5 probes x 64 tiles = 320 = 256 + 64), those probes are launched separately with split-K so the tail round is
// as wide as the chip: 1 + 1/s rounds + a one-sample reduce instead of 2 (measured 331.0 vs 334.1 ms per step).  Returns the
// number of tail probes (0: none) and their split factor.
static int tail_split(const ConvArgs& a, size_t partial_floats, int* split) {
    const long per_probe = (long)((a.Hout * a.Wout) / conv_bf16_tile_pixels(a)) * ((a.Cout + 127) / 128);
    const long r = per_probe * a.B % 256;
    if (!short_tail(per_probe, a.B) || per_probe <= 0 || r % per_probe != 0 || r / per_probe >= a.B) return 0;
    int s = (int)(256 / r);
    if (s > 4) s = 4;
    const int nchunks = (a.Cin + 15) / 16;
    while (s > 1 && nchunks / s < 4) --s;
    const size_t one = (size_t)(r / per_probe) * a.Cout * a.Hout * a.Wout;
    while (s > 1 && (size_t)s * one > partial_floats) --s;
    *split = s;
    return s > 1 ? (int)(r / per_probe) : 0;
}

// statistics of samples [s0, s0 + x.B) of the conv (batch B) by the cheapest route that applies; sets x's sink
static int stats_route(const ConvEnv& e, const StatAsk* q, bool want, ConvArgs& x, int s0, int B, int* keep_ntile) {
    if (!q || q->kind == ST_NONE) return SR_NONE;
    const int alone = q->norm ? SR_ALONE : SR_NONE;
    if (!want) return alone;
    if (x.nsplit > 1) return !q->norm ? SR_NONE : ((x.Hout * x.Wout) % 4 == 0 ? SR_SPLITK : SR_ALONE);
    const int ntile = (x.Hout * x.Wout) / conv_bf16_tile_pixels(x);
    const size_t need = (size_t)x.B * x.Cout * ntile * 2;
    const int epi = q->norm ? SR_EPI : SR_KEEP;
    const bool kept = q->keep && s0 == 0 && x.B == B && need <= q->keep_floats;      // the whole batch in one launch
    if (q->kind == ST_FWD && x.poly != 1 && conv_lowp_can_fuse_stats(x) && (kept || (q->norm && need <= e.stpart_floats))) {
        x.st_part = kept ? q->keep : e.stpart; x.st_kind = ST_FWD;
        if (kept) *keep_ntile = ntile;
        return epi;
    }
    // Tangent / cotangent group means in the conv epilogue (round 6, LOCO_FUSE_LIN=0: off): whole cout tiles, no split-K, not next
    // to a norm-cotangent term (the epilogue holds one of the two in its record registers).  A tangent launch that finishes one
    // part of a concatenation keeps its (norm-independent) raw sums in the part's buffer, at this lane's samples: lane rows are
    // keep_floats / max_batch floats apart whatever tile either lane runs.
    const bool cot_cache = q->kind == ST_COT && q->norm && q->sx && x.poly != 1;      // (the polyphase output form's epilogue takes the tangent kind only)
    if ((q->kind == ST_TAN || cot_cache) && e.fuse_lin && !x.cot_d && conv_lowp_can_fuse_stats(x)) {
        const size_t lane_off = (size_t)e.lane_s0 * (q->keep_floats / e.max_batch);
        const bool keptl = q->kind == ST_TAN && q->keep && s0 == 0 && x.B == B && lane_off + need <= q->keep_floats;
        if (keptl || (q->norm && need <= e.stpart_floats)) {
            x.st_part = keptl ? q->keep + lane_off : e.stpart; x.st_kind = q->kind; x.st_x = q->prim;
            if (q->kind == ST_COT) x.st_sx = q->sx;
            if (keptl) *keep_ntile = ntile;
            return epi;
        }
    }
    return alone;
}

static ConvLaunch plan_launch(const ConvEnv& e, const StatAsk* q, bool want, const ConvArgs& x, int s0, int B, int* keep_ntile) {
    ConvLaunch l;
    l.args = x;
    l.s0 = s0;
    l.args.tile = tile_for(x, e.prec, -1);
    l.stats = stats_route(e, q, want, l.args, s0, B, keep_ntile);
    if (l.stats == SR_EPI || l.stats == SR_KEEP) l.ntile = (x.Hout * x.Wout) / conv_bf16_tile_pixels(l.args);
    conv_plan_tile_pair(l.args, e.prec, -1);
    return l;
}

ConvPlan plan_conv(const ConvEnv& e, const ConvArgs& a0, int taps, const StatAsk* q, const ConvArgs* sc) {
    ConvPlan p;
    ConvArgs a = a0;
    a.taps = taps;
    a.gemm = 0;
    a.poly = 0;
    if (a.pool2) {
        if (conv_poly_in_ok(e, a, taps)) a.poly = 2;
        else {      // the 3x3 conv at full resolution into pool_tmp, then the pooling pass (run_conv)
            p.pool_after = true; p.pool_out = a.out; p.pool_out_bs = a.out_bs; p.pool_acc = a.accumulate;
            a.out = a.pool_tmp; a.out_bs = a.pool_tmp_bs; a.Hout = a.Hin; a.Wout = a.Win; a.accumulate = 0; a.pool2 = 0;
        }
    }
    if (sc) {
        // the shortcut K-concatenated into this 3x3 launch (conv_lowp_kcat: one write-out, no read-modify-write of the block
        // output, one launch less) where the launch allows it -- one round of whole probes (no tail-probe split) -- else run first
        ConvArgs t = a;
        t.nsplit = e.prec >= 1 ? conv_bf16_pick_nsplit(a.Cin, a.Cout, a.Hout, a.Wout, a.B, e.chip_share, 9, e.lanes) : 2;
        t.in2 = sc->in; t.in2_bs = sc->in_bs; t.Cin2 = sc->Cin;
        const long per_probe = (long)((a.Hout * a.Wout) / 256) * ((a.Cout + 127) / 128);
        if (e.prec >= 1 && taps == 9 && !short_tail(per_probe, a.B) && !a.bias2 && conv_lowp_can_kcat(t)) {
            a.in2 = sc->in; a.in2_bs = sc->in_bs; a.Cin2 = sc->Cin; a.in2_padded = sc->in_padded;
            a.wb2 = e.prec == 2 ? sc->wh : sc->wb;
            a.bias2 = sc->bias; a.bias2_bs = 0;          // the shortcut's bias (the forward pass; tangents carry none)
            a.res = nullptr;
        } else {
            p.sc_first = true;
            a.res = sc->out; a.res_bs = sc->out_bs;
        }
    }
    if (e.prec == 2) a.wb = a.wh;
    a.no_deep = e.deep1 ? 0 : 1;
    a.nsplit = e.prec >= 1 ? conv_bf16_pick_nsplit(a.Cin, a.Cout, a.Hout, a.Wout, a.B, e.chip_share, taps, e.lanes)
                           : conv_pick_nsplit(a.Cin, a.Cout, a.Hout, a.Wout, a.B);
    if (a.cot_d) {
        // The norm-cotangent term exists in ONE place: the staged epilogue of the per-pixel 1x1 kernels (EPI_COT1), un-split
        // launches of whole cout tiles in whole rounds of the chip (no tail-probe split).  Declined: planned as never asked for.
        ConvArgs t = a;
        t.tile = bf16_tile_of(t);
        const long per_probe = (long)((a.Hout * a.Wout) / conv_bf16_tile_pixels(t)) * ((a.Cout + 127) / 128);
        p.cot = e.prec >= 1 && taps == 1 && a.nsplit == 1 && !short_tail(per_probe, a.B) && conv_lowp_can_fuse_stats(t);
        if (!p.cot) { a.cot_d = nullptr; a.cot_d_bs = 0; a.cot_sx = nullptr; a.cot_tc = nullptr; a.cot_tc_bs = 0; }
    }
    while (a.nsplit > 1 && (size_t)a.nsplit * a.B * a.Cout * a.Hout * a.Wout > e.partial_floats) a.nsplit >>= 1;
    if (a.nsplit < 1) a.nsplit = 1;
    a.partial = e.partial;
    a.partial_floats = e.partial_floats;
    if (!a.poly && conv_poly_ok(e, a, taps)) a.poly = 1;
    if (a.poly == 1) { a.nsplit = 1; a.wb = e.prec == 2 ? a.wph : a.wpb; }
    if (a.poly == 2) { a.nsplit = 1; a.wb = e.prec == 2 ? a.wqh : a.wqb; }
    conv_plan_family(a, e.prec);
    a.tile = tile_for(a, e.prec, -1);
    int split = 1;
    const int tail = e.prec >= 1 && a.nsplit == 1 && a.B >= 2 && !a.gemm && !a.poly ? tail_split(a, e.partial_floats, &split) : 0;
    const bool want = q && q->kind != ST_NONE && e.prec >= 1 && e.fuse_stats;
    if (!tail) {
        p.l[0] = plan_launch(e, q, want, a, 0, a.B, &p.keep_ntile);
        return p;
    }
    // tail-probe split: two launches finish the tensor.  FORWARD statistics are per sample and come with both launches: the main
    // launch's epilogue partials (+ one merge launch for its samples), the tail's split-K epilogue -- no pass over the finished
    // tensor; the tangent / cotangent means likewise (round 6) where the split-K epilogue takes them (LOCO_FUSE_LIN=0: one
    // standalone pass over the whole batch behind the launches).
    const bool per_part = want && q->norm && (q->kind == ST_FWD || (e.fuse_lin && (a.Hout * a.Wout) % 4 == 0));
    p.stats_all = !per_part && q && q->kind != ST_NONE && q->norm;
    const StatAsk* ql = per_part ? q : nullptr;
    const int nb = a.B - tail;
    ConvArgs m = a, t = conv_shift_batch(a, nb);
    m.B = nb;
    t.nsplit = split;
    p.nl = 2;      // (neither launch holds the whole batch: nothing is kept)
    p.l[0] = plan_launch(e, ql, want, m, 0, a.B, &p.keep_ntile);
    p.l[1] = plan_launch(e, ql, want, t, nb, a.B, &p.keep_ntile);
    return p;
}

// Folded operators of the polyphase form (kernels.h).  Per dimension, output phase p reads the two low-resolution rows
// y + p - 1 + {0, 1} with the row-tap sets below (the column rule is the same):
//   nearest x2, pad 1 (out row 2y+p reads up-sampled rows 2y+p-1+k = low rows y + floor((p-1+k)/2)):
//       p = 0: {w0}, {w1 + w2}     p = 1: {w0 + w1}, {w2}
//   zero insertion, pad P (tap k reads inserted row 2y+p-P+k: data only where that is even, low row y + (p-P+k)/2):
//       P = 2:  p = 0: {w0}, {w2}   p = 1: {w1}, {}        P = 1:  p = 0: {}, {w1}   p = 1: {w0}, {w2}
void polyphase_fold(int kind, int nin, int nout, const float* w, long so, long si, long st, float* out) {
    // sel[p][t][k]: tap k of the 3-tap row operator contributes to footprint row t of phase p
    static const int sel[3][2][2][3] = {
        {{{1, 0, 0}, {0, 1, 1}}, {{1, 1, 0}, {0, 0, 1}}},
        {{{1, 0, 0}, {0, 0, 1}}, {{0, 1, 0}, {0, 0, 0}}},
        {{{0, 0, 0}, {0, 1, 0}}, {{1, 0, 0}, {0, 0, 1}}}};
    const long V = 4L * nout;
    for (int i = 0; i < nin; ++i)
        for (int pa = 0; pa < 2; ++pa)
            for (int pb = 0; pb < 2; ++pb)
                for (int ty = 0; ty < 2; ++ty)
                    for (int tx = 0; tx < 2; ++tx)
                        for (int o = 0; o < nout; ++o) {
                            double acc = 0.0;
                            for (int ky = 0; ky < 3; ++ky)
                                for (int kx = 0; kx < 3; ++kx)
                                    if (sel[kind][pa][ty][ky] && sel[kind][pb][tx][kx]) acc += (double)w[o * so + i * si + (3 * ky + kx) * st];
                            out[((long)i * 4 + 2 * ty + tx) * V + polyphase_vcout(nout, pa, pb, o)] = (float)acc;
                        }
}

void polyphase_fold_in(int nin, int nout, const float* w, long so, long si, long st, float* out, int noutP) {
    for (int p = 0; p < 2; ++p)
        for (int q = 0; q < 2; ++q)
            for (int i = 0; i < nin; ++i)
                for (int ty = 0; ty < 2; ++ty)
                    for (int tx = 0; tx < 2; ++tx) {
                        const int m = 2 * ty + 1 - p, n = 2 * tx + 1 - q;      // tap of the 4x4 operator
                        for (int o = 0; o < nout; ++o) {
                            double acc = 0.0;
                            for (int a = 0; a < 2; ++a)
                                for (int b = 0; b < 2; ++b) {
                                    const int ky = m - a, kx = n - b;
                                    if (ky >= 0 && ky < 3 && kx >= 0 && kx < 3) acc += (double)w[o * so + i * si + (3 * ky + kx) * st];
                                }
                            out[((((long)(2 * p + q) * nin + i) * 4) + 2 * ty + tx) * noutP + o] = (float)acc;
                        }
                    }
}

const char* conv_variant_name(const ConvArgs& a, int taps, int prec) {
    static const char* tiles[6] = {"2,2,2,2", "4,1,1,2", "1,4,1,1", "2,2,1,1", "2,2,2,4", "2,4,2,2"};
    static char names[3][2][6][6][56];      // lock-step tiles: [prec][3x3 / 1x1][tile][mode]
    static char others[3][3][6][40];        // the other kernels: [kernel][prec][mode or gemm_tm]
    const int mode = (a.mode < 0 || a.mode > 5) ? 2 : a.mode;
    const char* other = nullptr;
    int k = 0, v = mode;
    if (prec && taps == 9 && a.poly) {      // the polyphase launch: the lock-step kernel's 4-tap instance (raw, vector staging)
        static const char* pn[2][3] = {{"", "conv_mfma_bf16x3<4,2,4,2,2,0>", "conv_mfma_f16<4,2,4,2,2,0>"},
                                       {"", "conv_mfma_bf16x3<4,2,4,2,2,0>+pool", "conv_mfma_f16<4,2,4,2,2,0>+pool"}};
        return pn[a.poly == 2][prec];
    }
    if (prec && taps == 9 && a.Cin2 > 0) other = prec == 1 ? "conv_kcat_bf16x3<2,4,2,2,%d>" : "conv_kcat_f16<2,4,2,2,%d>";
    else if (prec == 1 && taps == 1 && a.gemm) { k = 1; other = "conv_gemm_bf16x3<%d>"; v = a.gemm_tm; }
    else if (prec == 1 && taps == 9 && a.pair) { k = 2; other = "conv_pair_bf16x3<%d>"; }      // the 16x16x32 tap-pair kernel
    if (other) {
        char* n = others[k][prec][v];
        if (!n[0]) snprintf(n, 40, other, v);
        return n;
    }
    int t = a.tile;
    if (t < 0 || t > 5) t = 0;
    int m = mode;
    if (taps != 9 && m != CM_NONE) m = CM_GN;
    if (!prec && m == CM_GN_GELU) m = CM_GN_SILU;      // the exact-fp32 kernel takes the activation at run time
    char* n = names[prec][taps == 9 ? 0 : 1][t][m];
    static const char* kn[3] = {"conv_mfma_f32", "conv_mfma_bf16x3", "conv_mfma_f16"};
    if (!n[0]) snprintf(n, 56, "%s<%d,%s,%d>", kn[prec], taps, tiles[t], m);
    return n;
}

}  // namespace loco
