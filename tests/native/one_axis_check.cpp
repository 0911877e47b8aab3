// one_axis_check.cpp -- CPU check of 3dscan_amd/csrc/sl3d_one_axis.h, the header k_one_axis, k_subpixel_one, sl3d_create, sl3d_group_create
// and sl3d_set_calibration compile (no HIP here).
//   one_axis_check               the rules around the solve: the coded axis of a flag word, which flag combinations and calibrations are
//                                refused and what the refusals say, a ray and a plane whose intersection is known, the singular system;
//                                exit 0 iff all are right
//   one_axis_check <in> <out>    the solve over a list of pixels
//   <in>:  int64 n; int32 axis; double Ac[12], Ap[12], f, c; double u[n], v[n], s[n]
//   <out>: double X[n][3]: one_axis_solve(Ac, Ap, axis, u, v, one_axis_project(s, f, 1.0 / f, c))
// tests/test_one_axis_arith.py compares <out> with the NumPy restatement at the project's 1e-5 bar, also under ASan / UBSan.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../3dscan_amd/csrc/sl3d_one_axis.h"

static int failures = 0;
#define EXPECT(cond)                                                         \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);          \
            failures++;                                                      \
        }                                                                    \
    } while (0)

static bool says(const char *text, const char *word) { return text && std::strstr(text, word); }
static bool near(double a, double b) { return a > b - 1e-9 && a < b + 1e-9; }

static int self_check()
{
    // the coded axis of a flag word
    EXPECT(one_axis_of_flags(0u) == -1 && one_axis_of_flags(128u | 512u | 1u) == -1 && one_axis_of_flags(1024u | 128u) == 0 && one_axis_of_flags(2048u | 128u) == 1);
    // (only_v, only_h, subpixel, repair)
    EXPECT(!one_axis_refusal(false, false, false, false) && !one_axis_refusal(false, false, true, true) && !one_axis_refusal(false, false, false, true));
    EXPECT(!one_axis_refusal(true, false, true, false) && !one_axis_refusal(false, true, true, false));
    const char *both = one_axis_refusal(true, true, true, false);
    EXPECT(says(both, "SL3D_FLAG_ONLY_VERTICAL") && says(both, "SL3D_FLAG_ONLY_HORIZONTAL") && says(both, "choose one"));
    EXPECT(one_axis_refusal(true, true, false, true) == both);  // (everything wrong: the first refusal)
    const char *v_alone = one_axis_refusal(true, false, false, false), *h_alone = one_axis_refusal(false, true, false, false);
    EXPECT(says(v_alone, "SL3D_FLAG_ONLY_VERTICAL") && says(v_alone, "add SL3D_FLAG_SUBPIXEL") && !says(v_alone, "HORIZONTAL"));
    EXPECT(says(h_alone, "SL3D_FLAG_ONLY_HORIZONTAL") && says(h_alone, "add SL3D_FLAG_SUBPIXEL") && !says(h_alone, "VERTICAL"));
    const char *v_rep = one_axis_refusal(true, false, true, true), *h_rep = one_axis_refusal(false, true, true, true);
    EXPECT(says(v_rep, "SL3D_FLAG_ONLY_VERTICAL") && says(v_rep, "SL3D_FLAG_REPAIR_PERIODS") && says(v_rep, "no one-axis form"));
    EXPECT(says(h_rep, "SL3D_FLAG_ONLY_HORIZONTAL") && says(h_rep, "SL3D_FLAG_REPAIR_PERIODS") && says(h_rep, "no one-axis form"));
    EXPECT(one_axis_refusal(true, false, false, true) == v_alone);
    // calibrations: a two-axis context takes anything; a one-axis one only a plain, undistorted projector
    const double plain[9] = {400, 0, 256, 0, 410, 192, 0, 0, 1}, none[5] = {0, 0, 0, 0, 0};
    EXPECT(!one_axis_calibration_refusal(0, plain, none) && !one_axis_calibration_refusal(1, plain, none));
    for (int i = 0; i < 5; i++) {
        double d[5] = {0, 0, 0, 0, 0};
        d[i] = 1e-9;
        EXPECT(!one_axis_calibration_refusal(-1, plain, d));
        const char *why0 = one_axis_calibration_refusal(0, plain, d), *why1 = one_axis_calibration_refusal(1, plain, d);
        EXPECT(says(why0, "SL3D_FLAG_ONLY_VERTICAL") && says(why0, "a curve and not a line") && says(why0, "previous calibration"));
        EXPECT(says(why1, "SL3D_FLAG_ONLY_HORIZONTAL") && says(why1, "a curve and not a line") && says(why1, "previous calibration"));
    }
    const int not_plain[5] = {1, 3, 6, 7, 8};
    for (int i = 0; i < 5; i++) {
        double K[9];
        std::memcpy(K, plain, sizeof K);
        K[not_plain[i]] += 0.5;
        EXPECT(!one_axis_calibration_refusal(-1, K, none));
        const char *why0 = one_axis_calibration_refusal(0, K, none), *why1 = one_axis_calibration_refusal(1, K, none);
        EXPECT(says(why0, "SL3D_FLAG_ONLY_VERTICAL") && says(why0, "plain projector matrix") && says(why0, "a curve and not a line"));
        EXPECT(says(why1, "SL3D_FLAG_ONLY_HORIZONTAL") && says(why1, "plain projector matrix") && says(why1, "a curve and not a line"));
    }
    // t: the coordinate itself up to rounding
    EXPECT(near(one_axis_project(300.25, 400.0, 1.0 / 400.0, 256.0), 300.25) && one_axis_project(256.0, 400.0, 1.0 / 400.0, 256.0) == 256.0);
    // a camera at the origin looking down Z (K = identity), a projector 100 to its right with the same orientation: the point (10, 20, 500)
    // is seen at u = 10 / 500, v = 20 / 500 and lit by column (10 - 100) / 500, row 20 / 500
    const double Ac[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}, Ap[12] = {1, 0, 0, -100, 0, 1, 0, 0, 0, 0, 1, 0};
    double X[3];
    one_axis_solve(Ac, Ap, 0, 10.0 / 500, 20.0 / 500, -90.0 / 500, X);
    EXPECT(near(X[0], 10) && near(X[1], 20) && near(X[2], 500));
    // the row of that rig is the camera's own row: its plane holds the camera ray, the system is singular -> X = 0 (cvInvert's zero matrix)
    one_axis_solve(Ac, Ap, 1, 10.0 / 500, 20.0 / 500, 20.0 / 500, X);
    EXPECT(X[0] == 0 && X[1] == 0 && X[2] == 0);
    // ... and with the projector 80 BELOW the camera the row decides
    const double Aq[12] = {1, 0, 0, 0, 0, 1, 0, -80, 0, 0, 1, 0};
    one_axis_solve(Ac, Aq, 1, 10.0 / 500, 20.0 / 500, -60.0 / 500, X);
    EXPECT(near(X[0], 10) && near(X[1], 20) && near(X[2], 500));
    return failures ? 1 : 0;
}

int main(int argc, char **argv)
{
    if (argc == 1) return self_check();
    if (argc != 3) return 2;
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t n = 0;
    int32_t axis = -1;
    double Ac[12], Ap[12], fc[2];
    bool ok = std::fread(&n, sizeof n, 1, f) == 1 && std::fread(&axis, sizeof axis, 1, f) == 1 && std::fread(Ac, sizeof(double), 12, f) == 12 &&
              std::fread(Ap, sizeof(double), 12, f) == 12 && std::fread(fc, sizeof(double), 2, f) == 2 && n >= 0 && n <= (1 << 24) && (axis == 0 || axis == 1);
    std::vector<double> in(ok ? 3 * (size_t)n : 0);
    ok = ok && std::fread(in.data(), sizeof(double), in.size(), f) == in.size();
    std::fclose(f);
    if (!ok) return 2;
    std::vector<double> out(3 * (size_t)n);
    const double *u = in.data(), *v = u + n, *s = v + n;
    for (int64_t i = 0; i < n; i++) one_axis_solve(Ac, Ap, axis, u[i], v[i], one_axis_project(s[i], fc[0], 1.0 / fc[0], fc[1]), &out[3 * (size_t)i]);
    f = std::fopen(argv[2], "wb");
    if (!f) return 2;
    ok = std::fwrite(out.data(), sizeof(double), out.size(), f) == out.size();
    return std::fclose(f) == 0 && ok ? 0 : 2;
}
