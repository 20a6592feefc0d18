// CPU: conv_args (loco-edit_amd/csrc/engine_internal.h), the one place the passes fill a launch's geometry, against the field
// list the passes used to type out per launch -- kept here only.  A swapped field (Hin taken from the output view, a transposed
// launch that forgets to swap) compiles and is right on every square same-level conv, so the cases are not square: a forward
// 3x3, a transposed 3x3 across a resampling level, and a 1x1.  Every byte of the struct is compared.
#include <cstdio>
#include <cstring>

#include "../../loco-edit_amd/csrc/engine_internal.h"

using namespace loco;
using namespace loco::eng;

static ConvArgs by_hand(const float* in, long in_bs, int Cin, int Hin, int Win, const ConvP& w, bool dgrad, float* out, long out_bs,
                        int Cout, int Hout, int Wout, int B, int ksize) {
    ConvArgs a; conv_defaults(a);
    a.in = in; a.in_bs = in_bs; a.Cin = Cin; a.Hin = Hin; a.Win = Win;
    setw(a, w, dgrad);
    a.out = out; a.out_bs = out_bs; a.Cout = Cout; a.Hout = Hout; a.Wout = Wout; a.B = B;
    if (ksize == 1) a.pad = 0;
    return a;
}

int main() {
    static float buf[64];
    ConvP w;      // every layout a distinct address; the folded records belong to the dgrad operator
    w.wf = buf + 1; w.wd = buf + 2; w.wbf = buf + 3; w.wbd = buf + 4; w.whf = buf + 5; w.whd = buf + 6;
    w.wpb = buf + 7; w.wph = buf + 8; w.poly_dgrad = true; w.wqb = buf + 9; w.wqh = buf + 10; w.bias = buf + 11;
    int bad = 0;
    auto same = [&](const char* what, const ConvArgs& got, const ConvArgs& want) {
        if (std::memcmp(&got, &want, sizeof(ConvArgs)) != 0) { std::printf("FAIL %s\n", what); ++bad; }
        if (got.bias || got.res || got.mode != CM_NONE || got.accumulate || got.upsample || got.zins || got.pool2 || got.stride != 1) {
            std::printf("FAIL %s: a field the constructor does not own left its default\n", what); ++bad;
        }
    };
    const TView x{buf + 20, 1000, 3, 24, 40}, y{buf + 30, 2000, 32, 12, 20}, z{buf + 40, 3000, 96, 12, 20};
    same("forward 3x3", conv_args(x, w, false, y, 5, 3), by_hand(x.p, x.bs, x.C, x.H, x.W, w, false, y.p, y.bs, y.C, y.H, y.W, 5, 3));
    same("transposed 3x3", conv_args(y, w, true, x, 4, 3), by_hand(y.p, y.bs, y.C, y.H, y.W, w, true, x.p, x.bs, x.C, x.H, x.W, 4, 3));
    same("1x1", conv_args(y, w, false, z, 2, 1), by_hand(y.p, y.bs, y.C, y.H, y.W, w, false, z.p, z.bs, z.C, z.H, z.W, 2, 1));
    same("transposed 1x1", conv_args(z, w, true, y, 2, 1), by_hand(z.p, z.bs, z.C, z.H, z.W, w, true, y.p, y.bs, y.C, y.H, y.W, 2, 1));
    const ConvArgs t = conv_args(y, w, true, x, 4, 3);
    if (t.Hin != 12 || t.Win != 20 || t.Hout != 24 || t.Wout != 40 || t.Cin != 32 || t.Cout != 3 || t.w != w.wd || t.pad != 1 ||
        conv_args(y, w, false, z, 2, 1).pad != 0) { std::printf("FAIL literal extents\n"); ++bad; }
    const float* ro = buf + 50;
    const TView v = tview_in(ro, 7, 1, 2, 3);
    if (v.p != ro || v.bs != 7 || v.C != 1 || v.H != 2 || v.W != 3 || (float*)v != ro) { std::printf("FAIL tview_in\n"); ++bad; }
    std::printf(bad ? "conv_args_check: %d FAILED\n" : "conv_args_check: ok\n", bad);
    return bad ? 1 : 0;
}
