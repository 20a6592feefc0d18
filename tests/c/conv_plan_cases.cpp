// Host-only plan printer for the case table of tests/conv_oracle.py (tests/test_conv_oracle_host.py): builds the ConvArgs of
// each case as loco_debug_conv (engine_diag.hip) + run_conv (engine.hip) do, asks plan_conv (conv_plan.hip, compiled with plain g++) and prints the
// plan in the words of conv_plan_text.h -- the text loco_debug_conv returns on the GPU.
//
// stdin, one case per line:
//   prec taps Cin Cout Hin Win B mode stride pad upsample zins in_padded Cin2 has_bias2 has_cot accumulate [st_kind st_norm st_keep]
// (the optional three: the statistics ask of the consumer of the output tensor -- kind 1 FWD / 2 TAN / 3 COT, whether a norm takes
//  them, whether the launch finishes one part of a concatenation and keeps its tile partials; a COT ask has the norm's records)
// stdout: "case <n>" followed by the plan's lines (a shortcut that runs first: its own plan ahead of the main operator's).
#include "../../loco-edit_amd/csrc/conv_plan_text.h"
#include <cstdint>
#include <cstring>
#include <iostream>
#include <sstream>

using namespace loco;

template <typename T>
static T* fake(int region) { return reinterpret_cast<T*>((uintptr_t)region << 40); }      // never dereferenced

int main() {
    std::string line;
    int n = 0;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream is(line);
        int prec, taps, Cin, Cout, Hin, Win, B, mode, stride, pad, ups, zins, in_padded, Cin2, has_bias2, has_cot, acc;
        if (!(is >> prec >> taps >> Cin >> Cout >> Hin >> Win >> B >> mode >> stride >> pad >> ups >> zins >> in_padded >> Cin2 >>
              has_bias2 >> has_cot >> acc)) {
            std::cerr << "bad case line: " << line << "\n";
            return 2;
        }
        int st_kind = 0, st_norm = 0, st_keep = 0;
        is >> st_kind >> st_norm >> st_keep;
        const int Hout = stride == 2 ? Hin / 2 : (ups || zins) ? 2 * Hin : Hin, Wout = stride == 2 ? Win / 2 : (ups || zins) ? 2 * Win : Win;
        ConvArgs a;
        std::memset(&a, 0, sizeof(a));
        a.nsplit = 1; a.res_scale = 1.f;
        a.in = fake<const float>(1); a.in_bs = (long)Cin * Hin * Win; a.Cin = Cin; a.Hin = Hin; a.Win = Win;
        a.out = fake<float>(2); a.out_bs = (long)Cout * Hout * Wout; a.Cout = Cout; a.Hout = Hout; a.Wout = Wout; a.B = B;
        a.w = fake<const float>(3); a.wb = fake<const void>(4); a.wh = fake<const void>(5);
        if (taps == 9 && (ups || zins)) { a.wpb = fake<const void>(19); a.wph = fake<const void>(20); }      // make_conv folds these operators
        a.mode = mode; a.stride = stride; a.pad = pad; a.upsample = ups; a.zins = zins; a.in_padded = in_padded; a.accumulate = acc;
        if (has_bias2) { a.bias2 = fake<const float>(6); a.bias2_bs = Cout; }
        if (has_cot) {
            a.cot_d = fake<const float>(7); a.cot_d_bs = a.out_bs; a.cot_sx = fake<const float2>(8); a.cot_tc = fake<const float>(9);
            a.cot_tc_bs = 2 * Cout;
        }
        ConvArgs s;
        std::memset(&s, 0, sizeof(s));
        if (Cin2 > 0) {
            s.nsplit = 1; s.res_scale = 1.f; s.stride = 1; s.pad = 0; s.in_padded = 1;
            s.in = fake<const float>(10); s.in_bs = (long)Cin2 * Hout * Wout; s.Cin = Cin2; s.Hin = Hout; s.Win = Wout;
            s.out = a.out; s.out_bs = a.out_bs; s.Cout = Cout; s.Hout = Hout; s.Wout = Wout; s.B = B;
            s.wb = fake<const void>(11); s.wh = fake<const void>(12); s.bias = fake<const float>(13);
            a.res = a.out; a.res_bs = a.out_bs;
        }
        ConvEnv e;      // a context as loco_create leaves it: one lane, the whole chip, the 256 MB workspace
        e.prec = prec; e.partial = fake<float>(14); e.partial_floats = (size_t)64 << 20; e.max_batch = 10;
        e.stpart = fake<float>(15); e.stpart_floats = (size_t)1 << 22;
        StatAsk q;
        if (st_kind) {
            q.kind = st_kind; q.norm = st_norm != 0;
            if (st_kind != ST_FWD) q.prim = fake<const float>(16);
            if (st_kind == ST_COT && st_norm) q.sx = fake<const float2>(17);
            if (st_keep) { q.keep = fake<float>(18); q.keep_floats = (size_t)1 << 24; }
        }
        const ConvPlan p = plan_conv(e, a, taps, st_kind ? &q : nullptr, Cin2 > 0 ? &s : nullptr);
        std::string text;
        if (p.sc_first) conv_plan_text(plan_conv(e, s, 1, nullptr, nullptr), 1, prec, text);
        conv_plan_text(p, taps, prec, text);
        std::cout << "case " << n++ << "\n" << text;
    }
    return 0;
}
