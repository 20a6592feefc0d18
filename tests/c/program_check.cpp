// CPU check of the U-Net program (loco-edit_amd/csrc/program.hip, host code only).  Reads "<name> <hex bytes of loco_unet_cfg>"
// lines, builds each program, asserts the layout / ordering invariants the passes rely on, and prints per config one
//   CFG <name> rc=0 tensors= ops= params= elements= per_sample= stats_per_sample= sx_total= hash=<fnv-1a 64 of the dump>
// line followed by its "P <name> <dims>" parameter list, or "CFG <name> rc=<code> <message>" for a refused configuration.
// A second argument names a config whose canonical dump is printed in full (to diff a digest mismatch).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <set>
#include <string>
#include <vector>

#include "../../loco-edit_amd/csrc/program.h"

using namespace loco;

// canonical text dump of a program: every tensor, every op, the counters, the ordered parameter list
static uint64_t fnv64(const std::string& s) {
    uint64_t h = 1469598103934665603ull;
    for (unsigned char b : s) { h ^= b; h *= 1099511628211ull; }
    return h;
}
template <class NormT>
static void dump_norm(std::string& o, const char* tag, const NormT& n) {
    char b[128];
    snprintf(b, sizeof b, " %s=%d,%ld,%ld,%.9g", tag, n.C, (long)n.soff, (long)n.sx_off, (double)n.eps);
    o += b;
}
template <class TensV, class OpV, class ParamV>
static std::string dump_program(const TensV& tens, const OpV& ops, long per_sample, long stats_per_sample, long sx_total, int n_in,
                                int n_out, int eps_t, int ctx_Lp, long attn_dmax, long max_tensor, const ParamV& params) {
    std::string o;
    char b[512];
    snprintf(b, sizeof b, "per_sample=%ld stats_per_sample=%ld sx_total=%ld n_in=%d n_out=%d eps_t=%d ctx_Lp=%d attn_dmax=%ld max_tensor=%ld\n",
             per_sample, stats_per_sample, sx_total, n_in, n_out, eps_t, ctx_Lp, attn_dmax, max_tensor);
    o += b;
    for (size_t i = 0; i < tens.size(); ++i) {
        const auto& t = tens[i];
        snprintf(b, sizeof b, "T%zu off=%ld C=%d H=%d W=%d cons=%d,%d cat=%d,%d,%d\n", i, (long)t.off, t.C, t.H, t.W, t.cons_op, t.cons_norm,
                 t.cat_a, t.cat_b, t.cat_of);
        o += b;
    }
    for (size_t i = 0; i < ops.size(); ++i) {
        const auto& p = ops[i];
        snprintf(b, sizeof b, "O%zu kind=%d name=%s in=%d out=%d h1=%d a1=%d hn=%d qkv=%d S=%d o=%d up=%d ap=%d xu=%d updown=%d scale_shift=%d heads=%d "
                 "ksize=%d has_x=%d xmid=%d xhn=%d xq=%d xS=%d xo=%d added_kv=%d in_is_skip=%d has_nin=%d has_temb=%d sym_down=%d xt=",
                 i, (int)p.kind, p.name.c_str(), p.in, p.out, p.h1, p.a1, p.hn, p.qkv, p.S, p.o, p.up, p.ap, p.xu, p.updown, (int)p.scale_shift,
                 p.heads, p.ksize, (int)p.has_x, p.xmid, p.xhn, p.xq, p.xS, p.xo, (int)p.added_kv, (int)p.in_is_skip, (int)p.has_nin,
                 (int)p.has_temb, (int)p.sym_down);
        o += b;
        for (size_t k = 0; k < sizeof(p.xt) / sizeof(p.xt[0]); ++k) { snprintf(b, sizeof b, "%s%d", k ? "," : "", p.xt[k]); o += b; }
        dump_norm(o, "n1", p.n1); dump_norm(o, "n2", p.n2); dump_norm(o, "nx", p.nx);
        const std::string* pn[9] = {&p.pn_n1, &p.pn_c1, &p.pn_emb, &p.pn_n2, &p.pn_c2, &p.pn_skip, &p.pn_qkv, &p.pn_proj, &p.pn_conv};
        o += " pn=";
        for (int k = 0; k < 9; ++k) { o += k ? "," : ""; o += pn[k]->empty() ? "-" : *pn[k]; }
        o += "\n";
    }
    for (const auto& pr : params) {
        o += "P " + pr.name;
        for (auto s : pr.shape) { snprintf(b, sizeof b, " %lld", (long long)s); o += b; }
        o += "\n";
    }
    return o;
}

static int g_bad = 0;
#define REQUIRE(cond, ...) do { if (!(cond)) { ++g_bad; printf("BAD %s: ", name.c_str()); printf(__VA_ARGS__); printf("\n"); } } while (0)

struct Range { long lo, hi; const char* what; size_t op; };
static void disjoint_inside(const std::string& name, std::vector<Range> r, long total, const char* arena) {
    std::sort(r.begin(), r.end(), [](const Range& a, const Range& b) { return a.lo < b.lo; });
    for (size_t i = 0; i < r.size(); ++i) {
        REQUIRE(r[i].lo >= 0 && r[i].hi <= total, "%s range of op %zu %s [%ld, %ld) outside [0, %ld)", arena, r[i].op, r[i].what, r[i].lo, r[i].hi, total);
        if (i) REQUIRE(r[i - 1].hi <= r[i].lo, "%s ranges of op %zu %s and op %zu %s overlap", arena, r[i - 1].op, r[i - 1].what, r[i].op, r[i].what);
    }
}

static void check_invariants(const std::string& name, const Program& p) {
    const int T = (int)p.tens.size();
    auto numel = [&](const TensPlan& t) { return (long)t.C * t.H * t.W; };
    // every tensor inside the per-sample layout at a 64-float-aligned offset
    for (int i = 0; i < T; ++i) {
        const TensPlan& t = p.tens[i];
        REQUIRE(t.off >= 0 && t.off % 64 == 0 && t.off + numel(t) <= p.per_sample, "tensor %d [%ld, +%ld) misplaced (per_sample %ld)", i, t.off,
                numel(t), p.per_sample);
        REQUIRE(numel(t) <= p.max_tensor, "tensor %d larger than max_tensor", i);
    }
    // two tensors overlap only as a concatenation and its two parts, and the parts tile the whole exactly
    std::vector<int> order(T);
    for (int i = 0; i < T; ++i) order[i] = i;
    std::sort(order.begin(), order.end(), [&](int a, int b) { return p.tens[a].off < p.tens[b].off; });
    for (int x = 0; x < T; ++x)
        for (int y = x + 1; y < T && p.tens[order[y]].off < p.tens[order[x]].off + numel(p.tens[order[x]]); ++y) {
            const int i = order[x], j = order[y];
            const TensPlan &a = p.tens[i], &b = p.tens[j];
            const bool rel = a.cat_a == j || a.cat_b == j || b.cat_a == i || b.cat_b == i;
            REQUIRE(rel, "tensors %d and %d overlap and are not a concatenation and its part", i, j);
        }
    for (int q = 0; q < T; ++q) {
        const TensPlan& Q = p.tens[q];
        REQUIRE((Q.cat_a >= 0) == (Q.cat_b >= 0), "tensor %d has one concatenation part", q);
        if (Q.cat_of >= 0) REQUIRE(Q.cat_of < T && (p.tens[Q.cat_of].cat_a == q || p.tens[Q.cat_of].cat_b == q), "tensor %d: cat_of does not point back", q);
        if (Q.cat_a < 0) continue;
        REQUIRE(Q.cat_a < T && Q.cat_b < T && Q.cat_a != Q.cat_b, "tensor %d: bad concatenation parts", q);
        if (Q.cat_a >= T || Q.cat_b >= T) continue;
        const TensPlan &A = p.tens[Q.cat_a], &B = p.tens[Q.cat_b];
        REQUIRE(A.cat_of == q && B.cat_of == q, "parts of tensor %d do not point back", q);
        REQUIRE(A.off == Q.off && B.off == Q.off + numel(A) && A.C + B.C == Q.C && A.H == Q.H && A.W == Q.W && B.H == Q.H && B.W == Q.W,
                "parts %d | %d do not tile concatenation %d", Q.cat_a, Q.cat_b, q);
        REQUIRE(Q.cons_op >= 0, "concatenation %d is recorded although no norm reads it", q);
    }
    // ops: valid tensor ids, input written before it is read
    std::vector<char> written(T, 0);
    std::vector<Range> stats, sx;
    for (size_t i = 0; i < p.ops.size(); ++i) {
        const OpPlan& op = p.ops[i];
        std::vector<int> ids = {op.in, op.out, op.h1, op.a1, op.hn, op.qkv, op.S, op.o, op.up, op.ap, op.xu, op.xmid, op.xhn, op.xq, op.xS, op.xo};
        if (op.kind == OP_XFMR) ids.insert(ids.end(), op.xt, op.xt + X_NT);
        bool valid = op.out >= 0 && (op.in >= 0 || op.kind == OP_CONV_IN);
        for (int id : ids) valid = valid && id >= -1 && id < T;
        REQUIRE(valid, "op %zu %s names a tensor that does not exist", i, op.name.c_str());
        if (!valid) continue;
        if (op.in >= 0) {
            const TensPlan& t = p.tens[op.in];
            REQUIRE(written[op.in] || (t.cat_a >= 0 && written[t.cat_a] && written[t.cat_b]), "op %zu %s reads tensor %d before it is written", i,
                    op.name.c_str(), op.in);
        }
        written[op.out] = 1;
        const long G = p.cfg.gn_groups;
        const NormPlan* ns[3] = {&op.n1, &op.n2, &op.nx};
        const char* nn[3] = {"n1", "n2", "nx"};
        const bool has[3] = {op.kind == OP_RES || op.kind == OP_ATTN || op.kind == OP_OUT || op.kind == OP_XFMR, op.kind == OP_RES,
                             op.kind == OP_ATTN && op.has_x};
        const int over[3] = {op.in, op.kind == OP_RES ? op.h1 : -1, op.xmid};      // the tensor each norm reads
        for (int k = 0; k < 3; ++k) {
            if (!has[k]) { REQUIRE(ns[k]->C == 0 && ns[k]->sx_off < 0, "op %zu %s: norm %s exists on an op that has none", i, op.name.c_str(), nn[k]); continue; }
            REQUIRE(ns[k]->C == p.tens[over[k]].C, "op %zu %s: norm %s has %d channels, its tensor %d", i, op.name.c_str(), nn[k], ns[k]->C, p.tens[over[k]].C);
            stats.push_back({ns[k]->soff, ns[k]->soff + 4L * ns[k]->C + 4L * G, nn[k], i});
            if (ns[k]->sx_off >= 0) sx.push_back({ns[k]->sx_off, ns[k]->sx_off + (long)ns[k]->C * p.tens[over[k]].H * p.tens[over[k]].W, nn[k], i});
        }
    }
    disjoint_inside(name, stats, p.stats_per_sample, "stats");
    disjoint_inside(name, sx, p.sx_total, "{S, xhat} cache");
    REQUIRE(p.eps_t >= 0 && p.eps_t < T && written[p.eps_t] && (long)p.n_out == (long)p.tens[p.eps_t].C * p.tens[p.eps_t].H * p.tens[p.eps_t].W,
            "network output tensor %d is not written or not n_out elements", p.eps_t);
    // consumers: cons_op / cons_norm point at an op whose in (or xmid) is that tensor
    for (int i = 0; i < T; ++i) {
        const TensPlan& t = p.tens[i];
        if (t.cons_op < 0) continue;
        bool ok = t.cons_op < (int)p.ops.size();
        if (ok) {
            const OpPlan& op = p.ops[t.cons_op];
            ok = (t.cons_norm == 1 && op.in == i) || (t.cons_norm == 2 && op.kind == OP_ATTN && op.has_x && op.xmid == i);
        }
        REQUIRE(ok, "tensor %d: consumer op %d norm %d does not read it", i, t.cons_op, t.cons_norm);
    }
    std::set<std::string> seen;
    for (const ParamDecl& d : p.params) REQUIRE(seen.insert(d.name).second, "parameter %s declared twice", d.name.c_str());
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: program_check <configs> [config to dump]\n"); return 2; }
    std::ifstream f(argv[1]);
    const std::string want = argc > 2 ? argv[2] : "";
    std::string name, hex;
    while (f >> name >> hex) {
        loco_unet_cfg cfg;
        if (hex.size() != 2 * sizeof(cfg)) { printf("CFG %s rc=-9 config is %zu bytes, loco_unet_cfg has %zu\n", name.c_str(), hex.size() / 2, sizeof(cfg)); ++g_bad; continue; }
        for (size_t i = 0; i < sizeof(cfg); ++i) ((unsigned char*)&cfg)[i] = (unsigned char)strtol(hex.substr(2 * i, 2).c_str(), nullptr, 16);
        Program p;
        std::string err;
        const int rc = build_program(cfg, &p, &err);
        if (rc) { printf("CFG %s rc=%d %s\n", name.c_str(), rc, err.c_str()); continue; }
        check_invariants(name, p);
        long elements = 0;
        for (const ParamDecl& d : p.params) { long k = 1; for (int64_t s : d.shape) k *= s; elements += k; }
        const std::string d = dump_program(p.tens, p.ops, p.per_sample, p.stats_per_sample, p.sx_total, p.n_in, p.n_out, p.eps_t, p.ctx_Lp, p.attn_dmax,
                                           p.max_tensor, p.params);
        printf("CFG %s rc=0 tensors=%zu ops=%zu params=%zu elements=%ld per_sample=%ld stats_per_sample=%ld sx_total=%ld hash=%016llx\n", name.c_str(),
               p.tens.size(), p.ops.size(), p.params.size(), elements, p.per_sample, p.stats_per_sample, p.sx_total, (unsigned long long)fnv64(d));
        for (const ParamDecl& q : p.params) {
            printf("P %s", q.name.c_str());
            for (int64_t s : q.shape) printf(" %lld", (long long)s);
            printf("\n");
        }
        if (name == want) fputs(d.c_str(), stdout);
    }
    return g_bad ? 1 : 0;
}
