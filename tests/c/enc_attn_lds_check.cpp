// CPU: enc_attn_lds_floats (loco-edit_amd/csrc/enc_attn_lds.h), the one carve-up of the streamed attention kernel's LDS, against the
// two formulas it replaced -- restated here only: the SAM kernel's (with its two bias tables of 16 x size floats each) for every
// head width 1..128 and table size 0..64, and the CLIP kernel's (no tables) at size 0.  The create functions refuse a geometry
// when this count exceeds 64 KiB, so equal counts mean the refusals fire at exactly the geometries they fired at before.
#include <cstddef>
#include <cstdio>

#include "../../loco-edit_amd/csrc/enc_attn_lds.h"

// the kernels' constants and rounding as the two units spelled them
static constexpr int THREADS = 256, WAVES = THREADS / 64, QW = 4, QB = WAVES * QW, KC = 64;
static size_t r4(size_t n) { return (n + 3) / 4 * 4; }

static size_t sam_formula(int hd, int size) {
    return r4((size_t)hd * KC) + r4((size_t)KC * (hd + 1)) + r4((size_t)hd * QB) + r4((size_t)2 * QB * size) + (size_t)WAVES * KC * QW;
}
static size_t clip_formula(int hd) { return r4((size_t)hd * KC) + r4((size_t)KC * (hd + 1)) + r4((size_t)hd * QB) + (size_t)WAVES * KC * QW; }

// usable in a constant expression, as the header promises
static_assert(loco::enc_attn_lds_floats(64, 0) == 64 * 64 + 64 * 65 + 64 * 16 + 4 * 64 * 4, "enc_attn_lds_floats(64, 0)");
static_assert(loco::ENC_ATTN_THREADS == THREADS && loco::ENC_ATTN_WAVES == WAVES && loco::ENC_ATTN_QW == QW && loco::ENC_ATTN_QB == QB &&
                  loco::ENC_ATTN_KC == KC,
              "the shared constants");

int main() {
    int bad = 0, refused_sam = 0, refused_clip = 0;
    for (int hd = 1; hd <= 128; ++hd) {
        for (int size = 0; size <= 64; ++size) {
            const size_t got = loco::enc_attn_lds_floats(hd, size), want = sam_formula(hd, size);
            if (got != want) {
                if (bad++ < 10) std::printf("FAIL hd %d size %d: %zu floats, the SAM formula gives %zu\n", hd, size, got, want);
            }
            refused_sam += got * sizeof(float) > 65536;
        }
        const size_t got = loco::enc_attn_lds_floats(hd, 0), want = clip_formula(hd);
        if (got != want) {
            if (bad++ < 10) std::printf("FAIL hd %d: %zu floats without tables, the CLIP formula gives %zu\n", hd, got, want);
        }
        refused_clip += got * sizeof(float) > 65536;
    }
    // both ranges cross the 64 KiB line, so the comparison covers the refusals' edge
    if (refused_sam == 0 || refused_sam == 128 * 65 || refused_clip == 0 || refused_clip == 128) {
        std::printf("FAIL the ranges do not cross 64 KiB (%d, %d)\n", refused_sam, refused_clip);
        ++bad;
    }
    std::printf(bad ? "enc_attn_lds_check: %d FAILED\n" : "enc_attn_lds_check: ok\n", bad);
    return bad ? 1 : 0;
}
