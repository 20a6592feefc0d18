// Host dump of the folded polyphase operators (loco-edit_amd/csrc/conv_plan.hip polyphase_fold): built with plain g++ together with
// conv_plan.hip by tests/test_polyphase_host.py.
//   polyphase_fold_dump KIND NIN NOUT in.f32 out.f32
// in:  the 3x3 operator as the launch receives it, [NOUT][NIN][3][3] float32 (a correlation);
// KIND 0 - 2 (PolyKind: nearest x2, zero insertion with pad 2 / pad 1), out: the folded operator in a layout-neutral order, [pa][pb][ty][tx][NOUT][NIN] float32 -- output phase (pa, pb), footprint tap
//      (ty, tx) reading low-resolution pixel (y + pa - 1 + ty, x + pb - 1 + tx) -- read through polyphase_vcout.
// KIND 3 (polyphase_fold_in: the conv followed by the 2x2 sum-pool), out: [p][q][ty][tx][NOUT][NIN] -- input phase image
//      g[2u+p][2v+q] read at (y - p + ty, x - q + tx).
#include "../../loco-edit_amd/csrc/kernels.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace loco;

int main(int argc, char** argv) {
    if (argc != 6) { fprintf(stderr, "usage: %s KIND NIN NOUT in.f32 out.f32\n", argv[0]); return 2; }
    const int kind = atoi(argv[1]), nin = atoi(argv[2]), nout = atoi(argv[3]);
    if (kind < 0 || kind > 3 || nin < 1 || nout < 64 || nout % 64) { fprintf(stderr, "bad arguments\n"); return 2; }
    std::vector<float> w((size_t)nout * nin * 9), folded((size_t)nin * 16 * nout), out(folded.size());
    FILE* f = fopen(argv[4], "rb");
    if (!f || fread(w.data(), sizeof(float), w.size(), f) != w.size()) { fprintf(stderr, "cannot read %s\n", argv[4]); return 1; }
    fclose(f);
    if (kind == 3) {
        polyphase_fold_in(nin, nout, w.data(), 9L * nin, 9, 1, folded.data(), nout);
        for (int ph = 0; ph < 4; ++ph)
            for (int t = 0; t < 4; ++t)
                for (int o = 0; o < nout; ++o)
                    for (int i = 0; i < nin; ++i)
                        out[(((size_t)ph * 4 + t) * nout + o) * nin + i] = folded[(((size_t)ph * nin + i) * 4 + t) * nout + o];
        f = fopen(argv[5], "wb");
        if (!f || fwrite(out.data(), sizeof(float), out.size(), f) != out.size()) { fprintf(stderr, "cannot write %s\n", argv[5]); return 1; }
        fclose(f);
        return 0;
    }
    polyphase_fold(kind, nin, nout, w.data(), 9L * nin, 9, 1, folded.data());
    // every slot of the folded layout is written exactly once: the virtual couts are a permutation of 0 .. 4 NOUT - 1
    std::vector<int> seen((size_t)4 * nout, 0);
    for (int pa = 0; pa < 2; ++pa)
        for (int pb = 0; pb < 2; ++pb)
            for (int o = 0; o < nout; ++o) {
                const int v = polyphase_vcout(nout, pa, pb, o);
                if (v < 0 || v >= 4 * nout || seen[v]++) { fprintf(stderr, "virtual couts are no permutation at (%d, %d, %d)\n", pa, pb, o); return 1; }
                for (int ty = 0; ty < 2; ++ty)
                    for (int tx = 0; tx < 2; ++tx)
                        for (int i = 0; i < nin; ++i)
                            out[((((size_t)(pa * 2 + pb) * 2 + ty) * 2 + tx) * nout + o) * nin + i] =
                                folded[((size_t)i * 4 + 2 * ty + tx) * 4 * nout + v];
            }
    f = fopen(argv[5], "wb");
    if (!f || fwrite(out.data(), sizeof(float), out.size(), f) != out.size()) { fprintf(stderr, "cannot write %s\n", argv[5]); return 1; }
    fclose(f);
    return 0;
}
