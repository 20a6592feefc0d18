// A conv plan (conv_plan.hip) as text: one line per launch (`part` is always 0: a launch is one kernel).  Shared by the
// diagnostics entry point loco_debug_conv (engine.hip) and the host-only plan printer of the tests
// (tests/c/conv_plan_cases.cpp), so that both speak of a plan in the same words.  Host code only; reads the plan, decides nothing.
#pragma once
#include "kernels.h"
#include <cstdio>
#include <string>

namespace loco {

inline void conv_plan_text(const ConvPlan& p, int taps, int prec, std::string& out) {
    char line[320];
    for (int li = 0; li < p.nl; ++li) {
        const ConvLaunch& l = p.l[li];
        const ConvArgs& y = l.args;
        snprintf(line, sizeof(line),
                 "launch=%d part=0 kernel=%s tile=%d nsplit=%d B=%d s0=%d gemm=%d gemm_tm=%d pair=%d Cin2=%d sc_first=%d cot=%d\n",
                 li, conv_variant_name(y, taps, prec), y.tile, y.nsplit, y.B, l.s0, y.gemm, y.gemm ? y.gemm_tm : 0, y.pair, y.Cin2,
                 p.sc_first ? 1 : 0, p.cot ? 1 : 0);
        out += line;
    }
}

}  // namespace loco
