// Host check of the conv launch planner (loco-edit_amd/csrc/conv_plan.hip): sweeps plan_conv over precisions, shapes, batches,
// lanes, statistics requests, norm-cotangent requests and shortcuts and asserts the invariants the launches rely on.  Built with
// plain g++ together with conv_plan.hip by tests/test_conv_plan_host.py; prints the coverage and exits non-zero on a failure.
#include "../../loco-edit_amd/csrc/kernels.h"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>

using namespace loco;

static int g_fail = 0;
static std::map<std::string, long> g_cov;
#define CHECK(cond, ...)                                                                       \
    do {                                                                                       \
        if (!(cond)) {                                                                         \
            if (g_fail++ < 20) { printf("FAIL %s:%d: %s | ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
        }                                                                                      \
    } while (0)

static const int kMT[6] = {128, 128, 32, 64, 128, 128}, kNT[6] = {128, 64, 128, 64, 256, 256};
static const char* kTileName[6] = {"2,2,2,2", "4,1,1,2", "1,4,1,1", "2,2,1,1", "2,2,2,4", "2,4,2,2"};

// never dereferenced: distinct addresses so pointer shifts can be checked
template <class T> static T* fake(uintptr_t base) { return reinterpret_cast<T*>(base << 32); }

struct Case {
    int prec, taps, Cin, Cout, H, W, B, mode, geom, lanes, lane_s0, chip_share, max_batch, kind, norm, sx, keep, cot, shortcut, bias2;
    size_t partial_floats, stpart_floats;
    bool fuse_stats = true, fuse_lin = true;
};

struct Built { ConvEnv e; ConvArgs a; ConvArgs sc; StatAsk q; };

static Built build(const Case& k) {
    Built b;
    ConvArgs& a = b.a;
    memset(&a, 0, sizeof(a));
    a.stride = 1; a.pad = 1; a.nsplit = 1; a.mode = k.mode; a.res_scale = 1.f;
    const long HW = (long)k.H * k.W;
    a.in = fake<const float>(1); a.in_bs = (long)k.Cin * HW + 7; a.Cin = k.Cin;
    a.out = fake<float>(2); a.out_bs = (long)k.Cout * HW + 11; a.Cout = k.Cout; a.Hout = k.H; a.Wout = k.W; a.B = k.B;
    a.Hin = k.H; a.Win = k.W;
    if (k.taps == 1) a.pad = 0;
    if (k.geom == 1) { a.stride = 2; a.pad = 0; a.Hin = 2 * k.H; a.Win = 2 * k.W; }
    if (k.geom == 2) { a.upsample = 1; a.Hin = k.H / 2; a.Win = k.W / 2; }
    if (k.geom == 3) { a.zins = 1; a.pad = 2; a.Hin = k.H / 2; a.Win = k.W / 2; }
    a.in_padded = k.geom != 3;
    a.prim = fake<const float>(3); a.prim_bs = 13;
    a.sc = fake<const float>(4); a.sh = fake<const float>(5); a.scsh_bs = 17;
    a.mr = fake<const float>(6); a.mr_bs = 19;
    a.tst = fake<const float>(7); a.tst_bs = 23;
    a.tc = fake<const float>(8); a.tc_bs = 29;
    a.res = fake<const float>(9); a.res_bs = 31;
    if (k.bias2) { a.bias2 = fake<const float>(10); a.bias2_bs = 37; }
    a.w = fake<const float>(11); a.wb = fake<const void>(12); a.wh = fake<const void>(13);
    if (k.cot) {
        a.cot_d = fake<const float>(14); a.cot_d_bs = 41; a.cot_sx = fake<const float2>(15); a.cot_tc = fake<const float>(16);
        a.cot_tc_bs = 43;
    }
    ConvArgs& s = b.sc;
    memset(&s, 0, sizeof(s));
    s.stride = 1; s.pad = 0; s.nsplit = 1; s.res_scale = 1.f;
    s.in = fake<const float>(17); s.in_bs = (long)(k.Cin / 2) * HW; s.Cin = k.Cin / 2 > 0 ? k.Cin / 2 : 1; s.Hin = k.H; s.Win = k.W;
    s.out = a.out; s.out_bs = a.out_bs; s.Cout = k.Cout; s.Hout = k.H; s.Wout = k.W; s.B = k.B;
    s.wb = fake<const void>(18); s.wh = fake<const void>(19); s.bias = fake<const float>(20); s.in_padded = 1;
    ConvEnv& e = b.e;
    e.prec = k.prec; e.chip_share = k.chip_share; e.lanes = k.lanes; e.lane_s0 = k.lane_s0;
    e.partial = fake<float>(21); e.partial_floats = k.partial_floats;
    e.stpart = fake<float>(22); e.stpart_floats = k.stpart_floats;
    e.fuse_stats = k.fuse_stats; e.fuse_lin = k.fuse_lin; e.deep1 = true; e.max_batch = k.max_batch;
    StatAsk& q = b.q;
    q.kind = k.kind; q.norm = k.norm; q.prim = fake<const float>(23);
    if (k.sx) q.sx = fake<const float2>(24);
    if (k.keep) { q.keep = fake<float>(25); q.keep_floats = (size_t)k.max_batch * k.Cout * (HW / 64 + 1) * 2; }
    return b;
}

static ConvPlan plan(const Built& b, const Case& k) {
    return plan_conv(b.e, b.a, k.taps, k.kind || k.keep ? &b.q : nullptr, k.shortcut ? &b.sc : nullptr);
}

// the decisions of a plan, as text (equal plans <=> equal signatures)
static std::string sig(const ConvPlan& p) {
    char buf[160];
    std::string s;
    snprintf(buf, sizeof buf, "sc%d nl%d all%d keep%d cot%d|", p.sc_first, p.nl, p.stats_all, p.keep_ntile, p.cot);
    s += buf;
    for (int i = 0; i < p.nl; ++i) {
        const ConvLaunch& l = p.l[i];
        snprintf(buf, sizeof buf, "B%d s0%d ns%d st%d nt%d cin2 %d stp%lx|", l.args.B, l.s0, l.args.nsplit, l.stats, l.ntile, l.args.Cin2,
                 (unsigned long)(uintptr_t)l.args.st_part);
        s += buf;
        const ConvArgs& y = l.args;
        snprintf(buf, sizeof buf, "[B%d t%d pr%d g%d/%d ns%d]", y.B, y.tile, y.pair, y.gemm, y.gemm_tm, y.nsplit);
        s += buf;
    }
    return s;
}

static bool kcat_allowed(const ConvArgs& a, int taps) {
    return taps == 9 && a.tile == 5 && a.stride == 1 && !a.upsample && !a.zins && a.pad == 1 && a.Cin % 16 == 0 && a.Cin2 % 16 == 0 &&
           a.in_padded && (a.mode == CM_GN_SILU || a.mode == CM_GN_GELU || a.mode == CM_TAN_SILU) && a.nsplit == 1;
}

static void check_case(const Case& k) {
    const Built b = build(k);
    const ConvPlan p = plan(b, k);
    const long HW = (long)k.H * k.W;
    g_cov["prec" + std::to_string(k.prec)]++;
    CHECK(sig(p) == sig(plan(b, k)), "plan not deterministic");
    CHECK(p.nl == 1 || p.nl == 2, "nl %d", p.nl);
    if (p.sc_first) g_cov["shortcut first"]++;
    if (p.stats_all) g_cov["stats over the whole batch"]++;
    if (k.shortcut) CHECK(p.sc_first == (p.l[0].args.Cin2 == 0), "shortcut neither first nor K-concatenated");
    for (int i = 0; i < p.nl; ++i) {
        const ConvLaunch& l = p.l[i];
        const ConvArgs& x = l.args;
        CHECK(x.nsplit >= 1, "nsplit %d", x.nsplit);
        // split-K and GEMM-record workspace
        if (x.gemm) {
            g_cov["gemm"]++;
            const size_t need = (x.nsplit > 1 ? (size_t)x.nsplit * x.B * x.Cout * HW : 0) + (size_t)x.B * x.Cin * HW;
            CHECK(need <= k.partial_floats, "gemm workspace %zu > %zu", need, k.partial_floats);
            CHECK(k.prec == 1 && k.taps == 1, "gemm on prec %d taps %d", k.prec, k.taps);
        } else if (x.nsplit > 1) {
            g_cov["split-K"]++;
            CHECK((size_t)x.nsplit * x.B * x.Cout * HW <= k.partial_floats, "split-K workspace");
        }
        // statistics route
        g_cov["route " + std::to_string(l.stats)]++;
        if (x.st_part) {
            CHECK(l.stats == SR_EPI || l.stats == SR_KEEP, "st_part on route %d", l.stats);
            CHECK(x.nsplit == 1 && !x.gemm && k.prec >= 1, "epilogue statistics on a split / GEMM launch");
            CHECK(x.Cout % kMT[x.tile] == 0, "epilogue statistics on partial cout tiles");
            CHECK(l.ntile == HW / kNT[x.tile], "ntile %d", l.ntile);
            const size_t need = (size_t)x.B * x.Cout * l.ntile * 2;
            if (x.st_part == b.e.stpart) CHECK(need <= k.stpart_floats, "stpart overflow");
            else {
                CHECK(k.keep && x.st_part >= b.q.keep, "st_part outside the known buffers");
                const size_t off = (size_t)(x.st_part - b.q.keep);
                CHECK(off + need <= b.q.keep_floats, "keep overflow");
                CHECK(p.keep_ntile == l.ntile, "kept partials without keep_ntile");
                g_cov[k.lane_s0 ? "kept, lane 1" : "kept, lane 0"]++;
            }
        } else {
            CHECK(l.stats != SR_EPI && l.stats != SR_KEEP, "epilogue route without a sink");
        }
        if (l.stats == SR_SPLITK) CHECK(x.nsplit > 1, "split-K statistics without split-K");
        if (!k.kind) CHECK(l.stats == SR_NONE, "statistics nobody asked for");
        // K-concatenated shortcut
        if (x.Cin2 > 0) {
            g_cov["kcat"]++;
            CHECK(k.shortcut && k.prec >= 1 && !k.bias2 && p.nl == 1 && kcat_allowed(x, k.taps), "kcat outside its conditions");
            CHECK(x.res == nullptr && x.in2 == b.sc.in && x.bias2 == b.sc.bias, "kcat operands");
        }
        if (p.sc_first) CHECK(x.res == b.sc.out + (x.out - b.a.out), "residual of a shortcut run first");
        // kernel of the launch
        const ConvArgs& y = x;
        g_cov["tile " + std::to_string(y.tile)]++;
        if (y.pair) {
            g_cov["tap-pair"]++;
            CHECK(k.prec == 1 && k.taps == 9 && y.tile == 5 && y.nsplit == 1 && !y.Cin2, "pair");
        }
        if (y.cot_d) CHECK(p.cot, "cot_d on a launch although declined");
        // the profile name is the kernel that runs
        const std::string name = conv_variant_name(y, k.taps, k.prec);
        if (!y.gemm && !y.Cin2 && !y.pair) {
            const std::string want = std::string(k.prec == 0 ? "conv_mfma_f32" : k.prec == 1 ? "conv_mfma_bf16x3" : "conv_mfma_f16") +
                                     "<" + std::to_string(k.taps) + "," + kTileName[y.tile] + ",";
            CHECK(name.compare(0, want.size(), want) == 0, "name %s, tile %d", name.c_str(), y.tile);
            if (k.taps == 1 && y.tile == 0 && k.prec) g_cov["1x1 named on the 128 x 128 tile"]++;
        }
        if (y.gemm) CHECK(name.find("conv_gemm_bf16x3") == 0, "gemm name %s", name.c_str());
        if (y.pair) CHECK(name.find("conv_pair_bf16x3") == 0, "pair name %s", name.c_str());
    }
    // tail-probe split
    if (p.nl == 2) {
        g_cov["tail split"]++;
        const ConvArgs &m = p.l[0].args, &t = p.l[1].args;
        const long nb = m.B;
        CHECK(m.B + t.B == k.B && m.nsplit == 1 && t.nsplit >= 2 && t.nsplit <= 4 && p.l[1].s0 == nb, "tail split %d + %d, ns %d / %d", m.B,
              t.B, m.nsplit, t.nsplit);
        CHECK(!m.Cin2 && !m.gemm && k.prec >= 1, "tail split of a kcat / gemm launch");
        const ConvArgs& a = m;
        CHECK(t.in == a.in + nb * a.in_bs && t.out == a.out + nb * a.out_bs && t.prim == a.prim + nb * a.prim_bs &&
                  t.sc == a.sc + nb * a.scsh_bs && t.sh == a.sh + nb * a.scsh_bs && t.mr == a.mr + nb * a.mr_bs &&
                  t.tst == a.tst + nb * a.tst_bs && t.tc == a.tc + nb * a.tc_bs && t.res == a.res + nb * a.res_bs,
              "tail pointers");
        if (a.bias2) CHECK(t.bias2 == a.bias2 + nb * a.bias2_bs, "tail bias2");
        CHECK(p.keep_ntile == 0, "kept partials across a tail split");
    }
    // norm-cotangent term
    if (k.cot) {
        if (p.cot) {
            g_cov["cot taken"]++;
            const ConvArgs& x = p.l[0].args;
            CHECK(k.prec >= 1 && k.taps == 1 && p.nl == 1 && x.nsplit == 1 && !x.gemm && x.Cout % kMT[x.tile] == 0 && x.cot_d &&
                      x.st_kind != ST_TAN && x.st_kind != ST_COT,
                  "cot_d kept on a launch without the term");
        } else {
            g_cov["cot declined"]++;
            for (int i = 0; i < p.nl; ++i) CHECK(!p.l[i].args.cot_d, "declined cot_d still set");
            Case n = k; n.cot = 0;
            CHECK(sig(p) == sig(plan(build(n), n)), "a declined cot_d request plans differently from none");
        }
    } else {
        CHECK(!p.cot, "cot taken without a request");
    }
}

// two lanes of a tangent pass keep their raw partials in one buffer: disjoint rows inside it for every batch split
static void check_lanes(Case k) {
    k.kind = ST_TAN; k.keep = 1; k.norm = 0; k.lanes = 2; k.cot = 0; k.shortcut = 0;
    for (int B = 4; B <= k.max_batch; ++B) {
        for (int b0 = 1; b0 < B; ++b0) {
            Case l0 = k, l1 = k;
            l0.B = b0; l0.lane_s0 = 0;
            l1.B = B - b0; l1.lane_s0 = b0;
            const Built x0 = build(l0), x1 = build(l1);
            const ConvPlan p0 = plan(x0, l0), p1 = plan(x1, l1);
            if (!p0.keep_ntile || !p1.keep_ntile) continue;
            g_cov["two lanes kept"]++;
            const ConvArgs &a0 = p0.l[0].args, &a1 = p1.l[0].args;
            const size_t o0 = a0.st_part - x0.q.keep, o1 = a1.st_part - x1.q.keep;
            const size_t n0 = (size_t)a0.B * a0.Cout * p0.l[0].ntile * 2, n1 = (size_t)a1.B * a1.Cout * p1.l[0].ntile * 2;
            CHECK(o0 + n0 <= o1 || o1 + n1 <= o0, "lane regions overlap: [%zu, +%zu) [%zu, +%zu), B %d = %d + %d, HW %d, Cout %d", o0, n0, o1,
                  n1, B, b0, B - b0, k.H * k.W, k.Cout);
            CHECK(o0 + n0 <= x0.q.keep_floats && o1 + n1 <= x1.q.keep_floats, "lane regions outside keep");
        }
    }
}

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static int pick(int n) {
    g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
    return (int)(g_rng % (uint64_t)n);
}

int main() {
    static const int chans[] = {3, 4, 32, 64, 96, 128, 192, 256, 320, 384, 512, 640, 768, 1024, 1280, 2560, 5120};
    static const int sides[] = {8, 16, 32, 48, 64, 128, 256};
    static const int batches[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 64};
    static const size_t partials[] = {(size_t)64 << 20, (size_t)32 << 20, (size_t)1 << 20};
    const int N = 400000;
    for (int it = 0; it < N; ++it) {
        Case k;
        k.prec = pick(3);
        k.taps = pick(2) ? 9 : 1;
        k.Cin = chans[pick(17)]; k.Cout = chans[pick(17)];
        k.H = k.W = sides[pick(7)];
        if (pick(8) == 0) k.W = sides[pick(7)];
        k.B = batches[pick(17)];
        k.geom = k.taps == 9 ? (pick(3) ? 0 : 1 + pick(3)) : 0;
        static const int modes9[] = {CM_NONE, CM_GN_SILU, CM_GN, CM_TAN_SILU, CM_COT_SILU, CM_GN_GELU};
        k.mode = k.taps == 9 ? modes9[pick(6)] : (pick(2) ? CM_NONE : CM_GN);
        k.lanes = 1 + pick(2);
        k.lane_s0 = k.lanes == 2 && pick(2) ? 1 + pick(4) : 0;
        k.chip_share = 1 + pick(2);
        k.max_batch = k.B > 16 ? 64 : 16;
        if (k.lane_s0 + k.B > k.max_batch) k.lane_s0 = 0;
        static const int kinds[] = {ST_NONE, ST_FWD, ST_TAN, ST_COT};
        k.kind = kinds[pick(4)];
        k.norm = k.kind ? pick(4) != 0 : 0;
        k.sx = pick(4) != 0;
        k.keep = (k.kind == ST_FWD || k.kind == ST_TAN) && pick(2);
        if (k.kind && !k.norm && !k.keep) k.norm = 1;
        k.cot = k.taps == 1 && pick(3) == 0;
        k.shortcut = k.taps == 9 && k.kind != ST_COT && pick(3) == 0;
        k.bias2 = pick(4) == 0;
        k.partial_floats = partials[pick(3)];
        const size_t big = (size_t)k.Cout * k.H * k.W;
        k.stpart_floats = pick(6) ? (size_t)k.max_batch * (big / 64 + 1) * 2 : 4096;
        k.fuse_stats = pick(8) != 0;
        k.fuse_lin = pick(8) != 0;
        check_case(k);
        if (it % 2000 == 0) check_lanes(k);
    }
    {   // the lane rule on the shapes of the up-path concatenations, both lane splits, all tiles
        Case k{};
        k.prec = 1; k.taps = 9; k.mode = CM_TAN_SILU; k.chip_share = 1; k.max_batch = 16; k.sx = 1;
        k.partial_floats = (size_t)32 << 20; k.stpart_floats = 1 << 26;
        for (int c : {64, 128, 256, 320, 512, 640})
            for (int s : {8, 16, 32, 64, 128}) {
                k.Cin = k.Cout = c; k.H = k.W = s;
                for (int t : {9, 1}) { k.taps = t; k.mode = t == 9 ? CM_TAN_SILU : CM_NONE; check_lanes(k); }
            }
    }
    // the two decisions whose reasons the comments record, with the values the parent computed
    {   // round-6 floor rule: 1024 -> 512 @16^2, 5 probes: 12 splits (20 tiles x 12 = 240 workgroups, one round)
        Case k{};
        k.prec = 1; k.taps = 9; k.Cin = 1024; k.Cout = 512; k.H = k.W = 16; k.B = 5; k.mode = CM_GN_SILU; k.lanes = 1; k.chip_share = 1;
        k.max_batch = 16; k.partial_floats = (size_t)64 << 20; k.stpart_floats = 1 << 20;
        const ConvPlan p = plan(build(k), k);
        CHECK(p.nl == 1 && p.l[0].args.nsplit == 12, "1024 -> 512 @16^2 x 5: nsplit %d", p.l[0].args.nsplit);
    }
    {   // tail-probe split: 5 probes x 64 tiles (128 -> 128 @128^2) = 256 + 64: the last probe on its own with 2 splits
        Case k{};
        k.prec = 1; k.taps = 9; k.Cin = 128; k.Cout = 128; k.H = k.W = 128; k.B = 5; k.mode = CM_GN_SILU; k.lanes = 1; k.chip_share = 1;
        k.max_batch = 16; k.partial_floats = (size_t)64 << 20; k.stpart_floats = 1 << 24;
        const ConvPlan p = plan(build(k), k);
        CHECK(p.nl == 2 && p.l[0].args.B == 4 && p.l[0].args.nsplit == 1 && p.l[1].args.B == 1 && p.l[1].args.nsplit == 2,
              "tail split: nl %d, B %d + %d, ns %d", p.nl, p.l[0].args.B, p.l[1].args.B, p.l[1].args.nsplit);
    }
    // every kind of decision is reached
    std::string need[] = {"prec0", "prec1", "prec2", "gemm", "split-K", "tail split", "kcat", "shortcut first", "tap-pair",
                          "route 0", "route 1", "route 2", "route 3", "route 4", "stats over the whole batch", "kept, lane 0",
                          "kept, lane 1", "two lanes kept", "cot taken", "cot declined", "tile 0", "tile 1", "tile 2", "tile 3",
                          "tile 5", "1x1 named on the 128 x 128 tile"};
    for (const std::string& s : need) CHECK(g_cov[s] > 0, "never reached: %s", s.c_str());
    for (const auto& kv : g_cov) printf("%-36s %ld\n", kv.first.c_str(), kv.second);
    printf("%s: %d failure(s)\n", g_fail ? "FAILED" : "ok", g_fail);
    return g_fail ? 1 : 0;
}
