// A conv plan (conv_plan.hip) as text: one line per launch (`part` is always 0: a launch is one kernel) and one closing line
// about the statistics of the whole plan.  Shared by run_conv (engine.hip: appends it to loco_ctx::plan_log where the diagnostics
// entry point loco_debug_conv, engine_diag.hip, has set one) and the host-only plan printer of the tests (tests/c/conv_plan_cases.cpp), so that both speak of a plan in the same words.  Host code only;
// reads the plan, decides nothing.
#pragma once
#include "kernels.h"
#include <cstdio>
#include <string>

namespace loco {

inline const char* stat_route_name(int r) {
    static const char* names[5] = {"none", "epi", "splitk", "alone", "keep"};
    return r >= 0 && r < 5 ? names[r] : "?";
}

inline void conv_plan_text(const ConvPlan& p, int taps, int prec, std::string& out) {
    char line[384];
    for (int li = 0; li < p.nl; ++li) {
        const ConvLaunch& l = p.l[li];
        const ConvArgs& y = l.args;
        snprintf(line, sizeof(line),
                 "launch=%d part=0 kernel=%s tile=%d nsplit=%d B=%d s0=%d gemm=%d gemm_tm=%d pair=%d Cin2=%d sc_first=%d cot=%d "
                 "stats=%s ntile=%d\n",
                 li, conv_variant_name(y, taps, prec), y.tile, y.nsplit, y.B, l.s0, y.gemm, y.gemm ? y.gemm_tm : 0, y.pair, y.Cin2,
                 p.sc_first ? 1 : 0, p.cot ? 1 : 0, stat_route_name(l.stats), l.ntile);
        out += line;
    }
    snprintf(line, sizeof(line), "stats_all=%d keep_ntile=%d\n", p.stats_all ? 1 : 0, p.keep_ntile);
    out += line;
}

}  // namespace loco
