// Split-bf16 ("bf16x3") and f16 convolution: dispatch of the launches conv_plan.hip planned to the kernel templates of
// conv_bf16_kernel.h, conv_pair_kernel.h and conv_gemm_kernel.h (instantiated in conv_bf16_inst_*.hip).
#include "kernels.h"
#include <cstdio>
#include <cstdlib>

namespace loco {

enum : int { PR_BF16X3 = 0, PR_F16 = 1 };
template <int PR, int TAPS, int MODE> void launch_tile_b(const ConvArgs& a, hipStream_t st);   // conv_bf16_inst_*.hip
template <int PR, int MODE> void launch_kcat_b(const ConvArgs& a, hipStream_t st);            // conv_bf16_inst_*.hip
template <int PR, int MODE> void launch_pair_b(const ConvArgs& a, hipStream_t st);            // conv_bf16_inst_k.hip (conv_pair_kernel.h)
void launch_conv_gemm(const ConvArgs& a, hipStream_t st);      // conv_bf16_inst_j.hip (conv_gemm_kernel.h)
template <int PR> void launch_poly_b(const ConvArgs& a, hipStream_t st);                      // conv_bf16_inst_p*.hip
template <int PR> void launch_poly_in_b(const ConvArgs& a, hipStream_t st);                   // conv_bf16_inst_p*.hip

template <int PR>
static void launch_lowp(const ConvArgs& a, int taps, hipStream_t st) {
#ifdef LOCO_DIAG
    // Tripwire: the norm-cotangent term exists in ONE place, the staged epilogue of the per-pixel 1x1 kernels (EPI_COT1) on
    // un-split launches of whole cout tiles; plan_conv keeps it on such launches only.
    if (a.cot_d && (taps != 1 || a.gemm || a.nsplit > 1 || a.Cin2 > 0 || (a.Cout % conv_bf16_tile_couts(a)) != 0 || a.st_kind == ST_TAN || a.st_kind == ST_COT)) {
        fprintf(stderr, "loco: ConvArgs::cot_d on a launch whose epilogue has no norm-cotangent term (taps %d, gemm %d, nsplit %d, Cout %d, st_kind %d)\n",
                taps, a.gemm, a.nsplit, a.Cout, a.st_kind);
        abort();
    }
#endif
    if constexpr (PR == PR_BF16X3) {
        if (taps == 1 && a.gemm) { launch_conv_gemm(a, st); return; }
    }
    if (taps == 9 && a.poly == 2) { launch_poly_in_b<PR>(a, st); return; }      // transposed up conv + 2x2 pool (conv_plan.hip conv_poly_in_ok)
    if (taps == 9 && a.poly) { launch_poly_b<PR>(a, st); return; }      // polyphase up / zero-insert conv (conv_plan.hip conv_poly_ok)
    if (taps == 9 && a.Cin2 > 0) {       // K-concatenated shortcut (plan_conv checked conv_lowp_can_kcat)
        if (a.mode == CM_GN_SILU) launch_kcat_b<PR, CM_GN_SILU>(a, st);
        else if (a.mode == CM_GN_GELU) launch_kcat_b<PR, CM_GN_GELU>(a, st);      // forward pass of a GELU network (DeepFloyd IF)
        else launch_kcat_b<PR, CM_TAN_SILU>(a, st);
        return;
    }
    if constexpr (PR == PR_BF16X3) {
        if (taps == 9 && a.pair) {           // the 16x16x32 tap-pair kernel (conv_plan.hip conv_pair_ok)
            switch (a.mode) {
                case CM_NONE: launch_pair_b<PR, CM_NONE>(a, st); break;
                case CM_GN_SILU: launch_pair_b<PR, CM_GN_SILU>(a, st); break;
                case CM_TAN_SILU: launch_pair_b<PR, CM_TAN_SILU>(a, st); break;
                default: launch_pair_b<PR, CM_COT_SILU>(a, st); break;
            }
            return;
        }
    }
    if (taps == 9) {
        switch (a.mode) {
            case CM_NONE: launch_tile_b<PR, 9, CM_NONE>(a, st); break;
            case CM_GN_SILU: launch_tile_b<PR, 9, CM_GN_SILU>(a, st); break;
            case CM_GN_GELU: launch_tile_b<PR, 9, CM_GN_GELU>(a, st); break;
            case CM_TAN_SILU: launch_tile_b<PR, 9, CM_TAN_SILU>(a, st); break;
            case CM_COT_SILU: launch_tile_b<PR, 9, CM_COT_SILU>(a, st); break;
            default: launch_tile_b<PR, 9, CM_GN>(a, st); break;
        }
    } else {
        switch (a.mode) {
            case CM_NONE: launch_tile_b<PR, 1, CM_NONE>(a, st); break;
            default: launch_tile_b<PR, 1, CM_GN>(a, st); break;
        }
    }
}
void launch_conv_bf16x3(const ConvArgs& a, int taps, hipStream_t st) { launch_lowp<PR_BF16X3>(a, taps, st); }
void launch_conv_f16(const ConvArgs& a, int taps, hipStream_t st) { launch_lowp<PR_F16>(a, taps, st); }

}  // namespace loco
