// anchor_check.cpp -- CPU check of 3dscan_amd/csrc/sl3d_anchor.h, the header k_subpixel<true>, k_subpixel_coords<true>, k_subpixel_fused<true>,
// sl3d_create and sl3d_group_create compile (no HIP here).
//   anchor_check               the rules around the formula: where it applies (anchor_applies), which flag combinations are refused and
//                              what the refusals say (anchor_refusal), the constants; exit 0 iff all are right
//   anchor_check <in> <out>    the anchored coordinate over a lattice
//   <in>:  int64 n_w, n_code; int32 fw; float w[n_w]; int32 code[n_code]
//   <out>: double xs[2][n_code][n_w]: anchor_coordinate(w, code, fw, n_fringe) for n_fringe = 3, then 4
// tests/test_anchor_arith.py compares <out> with the NumPy restatement bit for bit, also under ASan / UBSan.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../3dscan_amd/csrc/sl3d_anchor.h"

static int failures = 0;
#define EXPECT(cond)                                                         \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);          \
            failures++;                                                      \
        }                                                                    \
    } while (0)

static bool says(const char *text, const char *word) { return text && std::strstr(text, word); }

static int self_check()
{
    // stage 4's loop: frame positions 1 .. full - 2, and only an axis with Gray planes
    EXPECT(!anchor_applies(7, 0, 320) && anchor_applies(7, 1, 320) && anchor_applies(7, 318, 320) && !anchor_applies(7, 319, 320));
    EXPECT(!anchor_applies(0, 100, 320) && anchor_applies(1, 100, 320) && !anchor_applies(-1, 100, 320));
    EXPECT(!anchor_applies(7, 0, 2) && !anchor_applies(7, 1, 2) && anchor_applies(7, 1, 3));
    // (anchor, subpixel, repair)
    EXPECT(!anchor_refusal(false, false, false) && !anchor_refusal(false, true, false) && !anchor_refusal(false, true, true) && !anchor_refusal(false, false, true));
    EXPECT(!anchor_refusal(true, true, false));
    const char *alone = anchor_refusal(true, false, false), *both = anchor_refusal(true, true, true), *all_wrong = anchor_refusal(true, false, true);
    EXPECT(says(alone, "SL3D_FLAG_ANCHOR_PERIODS") && says(alone, "SL3D_FLAG_SUBPIXEL") && says(alone, "add SL3D_FLAG_SUBPIXEL"));
    EXPECT(says(both, "SL3D_FLAG_ANCHOR_PERIODS") && says(both, "SL3D_FLAG_REPAIR_PERIODS") && says(both, "choose one"));
    EXPECT(all_wrong == alone);
    // the constants, and a pixel in the middle of its cell: code 5 of 16-pixel cells, phase pi from the cell's start -> 5.5 cells
    EXPECT(SL3D_ANCHOR_P2 == 44.0 / 7.0 && SL3D_ANCHOR_TWOPI == 6.283185307179586 && anchor_phase_offset(3) == 0.0 && anchor_phase_offset(5) == 0.0);
    EXPECT(anchor_phase_offset(4) < -9.4e-4 && anchor_phase_offset(4) > -9.6e-4);
    const float w = (float)(5.5 * SL3D_ANCHOR_TWOPI - 5.0 * SL3D_ANCHOR_TWOPI);
    EXPECT(anchor_period((double)w, 5) == 5.0);
    const double xs = anchor_coordinate(w, 5, 16, 3), want = 16.0 * (5.5 * SL3D_ANCHOR_TWOPI / SL3D_ANCHOR_P2);
    EXPECT(xs > want - 1e-5 && xs < want + 1e-5);
    // the period is the fringe's, not the cell's: far out the nearest fringe period is no longer the code (2,484.5 cells hold one period more)
    EXPECT(anchor_period(3.0, 100) == 100.0 && anchor_period(3.0, 4000) == 4002.0);
    return failures ? 1 : 0;
}

int main(int argc, char **argv)
{
    if (argc == 1) return self_check();
    if (argc != 3) return 2;
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t n_w = 0, n_code = 0;
    int32_t fw = 0;
    bool ok = std::fread(&n_w, sizeof n_w, 1, f) == 1 && std::fread(&n_code, sizeof n_code, 1, f) == 1 && std::fread(&fw, sizeof fw, 1, f) == 1 && n_w >= 0 &&
              n_code >= 0 && n_w <= (1 << 20) && n_code <= (1 << 20);
    std::vector<float> w(ok ? (size_t)n_w : 0);
    std::vector<int32_t> code(ok ? (size_t)n_code : 0);
    ok = ok && std::fread(w.data(), sizeof(float), w.size(), f) == w.size() && std::fread(code.data(), sizeof(int32_t), code.size(), f) == code.size();
    std::fclose(f);
    if (!ok) return 2;
    std::vector<double> out(2 * code.size() * w.size());
    size_t o = 0;
    for (int n_fringe = 3; n_fringe <= 4; n_fringe++)
        for (size_t c = 0; c < code.size(); c++)
            for (size_t i = 0; i < w.size(); i++) out[o++] = anchor_coordinate(w[i], code[c], fw, n_fringe);
    f = std::fopen(argv[2], "wb");
    if (!f) return 2;
    ok = std::fwrite(out.data(), sizeof(double), out.size(), f) == out.size();
    return std::fclose(f) == 0 && ok ? 0 : 2;
}
