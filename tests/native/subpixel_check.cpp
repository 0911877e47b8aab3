// subpixel_check.cpp -- CPU check of 3dscan_amd/csrc/sl3d_subpixel.h, the header k_subpixel and sl3d_capi_subpixel.cpp compile (no HIP here).
//   subpixel_check               the argument checks of sl3d_triangulate_subpixel (subpixel_check_args) over every documented refusal and
//                                the rejection rule (subpixel_rejected) at its edges; exit 0 iff all are right
//   subpixel_check <in> <out>    the residual of n pixels
//   <in>:  double A_cam[12], A_proj[12]; int64 n; n x double {X, Y, Z, u, v, u', v'}
//   <out>: n x float residual
// tests/test_subpixel_arith.py compares <out> with the NumPy restatement, also under ASan / UBSan.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../3dscan_amd/csrc/sl3d_subpixel.h"

static int failures = 0;
#define EXPECT(cond)                                                         \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);          \
            failures++;                                                      \
        }                                                                    \
    } while (0)

static int self_check()
{
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    // (first_view, n_views, max_views, keep, have_cal, max_residual)
    EXPECT(subpixel_check_args(0, 1, 1, 1, 1, inf) == 0);
    EXPECT(subpixel_check_args(1, 2, 3, 1, 1, 0.25) == 0);
    EXPECT(subpixel_check_args(0, 1, 1, 1, 1, 5e-324) == 0);
    EXPECT(subpixel_check_args(-1, 1, 3, 1, 1, inf) == -1);
    EXPECT(subpixel_check_args(0, 0, 3, 1, 1, inf) == -1);
    EXPECT(subpixel_check_args(0, -1, 3, 1, 1, inf) == -1);
    EXPECT(subpixel_check_args(2, 2, 3, 1, 1, inf) == -1);
    EXPECT(subpixel_check_args(3, 1, 3, 1, 1, inf) == -1);
    EXPECT(subpixel_check_args(1, std::numeric_limits<int>::max(), 3, 1, 1, inf) == -1);  // (no overflow on the way)
    EXPECT(subpixel_check_args(0, 1, 1, 0, 1, inf) == -4);
    EXPECT(subpixel_check_args(0, 1, 1, 1, 0, inf) == -4);
    EXPECT(subpixel_check_args(0, 1, 1, 1, 1, 0.0) == -1);
    EXPECT(subpixel_check_args(0, 1, 1, 1, 1, -0.0) == -1);
    EXPECT(subpixel_check_args(0, 1, 1, 1, 1, -1.0) == -1);
    EXPECT(subpixel_check_args(0, 1, 1, 1, 1, -inf) == -1);
    EXPECT(subpixel_check_args(0, 1, 1, 1, 1, nan) == -1);
    // the order: views, KEEP_STAGES, max_residual, calibration
    EXPECT(subpixel_check_args(5, 1, 1, 0, 0, nan) == -1);
    EXPECT(subpixel_check_args(0, 1, 1, 0, 0, nan) == -4);
    EXPECT(subpixel_check_args(0, 1, 1, 1, 0, nan) == -1);
    // the rejection: on the float, <= keeps, NaN goes, +infinity never rejects
    const float fnan = std::numeric_limits<float>::quiet_NaN(), finf = std::numeric_limits<float>::infinity();
    EXPECT(!subpixel_rejected(0.25f, 0.25) && subpixel_rejected(std::nextafter(0.25f, 1.0f), 0.25) && !subpixel_rejected(0.0f, 0.25));
    EXPECT(subpixel_rejected(0.1f, 0.1) && !subpixel_rejected(0.1f, (double)0.1f));  // ((double)0.1f > 0.1: the decision is the float's)
    EXPECT(subpixel_rejected(fnan, 1e300) && subpixel_rejected(finf, 1e300));
    EXPECT(!subpixel_rejected(fnan, inf) && !subpixel_rejected(finf, inf) && !subpixel_rejected(3.0f, inf));
    EXPECT(subpixel_rejects(1e308) && !subpixel_rejects(inf));
    // a point that both devices see where it projects has no residual
    const double A[12] = {800, 0, 320, 10, 0, 800, 240, -20, 0, 0, 1, 100}, X[3] = {3, -4, 50};
    const double w = X[2] + 100;
    EXPECT(subpixel_reproj_err2(A, X, (800 * X[0] + 320 * X[2] + 10) / w, (800 * X[1] + 240 * X[2] - 20) / w) < 1e-24);
    EXPECT(std::fabs(subpixel_reproj_err2(A, X, (800 * X[0] + 320 * X[2] + 10) / w + 3, (800 * X[1] + 240 * X[2] - 20) / w - 4) - 25) < 1e-9);
    EXPECT(subpixel_residual(9.0, 16.0) == 5.0f);
    return failures ? 1 : 0;
}

int main(int argc, char **argv)
{
    if (argc == 1) return self_check();
    if (argc != 3) return 2;
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    double Ac[12], Ap[12];
    int64_t n = 0;
    bool ok = std::fread(Ac, sizeof(double), 12, f) == 12 && std::fread(Ap, sizeof(double), 12, f) == 12 && std::fread(&n, sizeof n, 1, f) == 1 && n >= 0;
    std::vector<double> in(ok ? 7 * (size_t)n : 0);
    ok = ok && std::fread(in.data(), sizeof(double), in.size(), f) == in.size();
    std::fclose(f);
    if (!ok) return 2;
    std::vector<float> out((size_t)n);
    for (size_t i = 0; i < (size_t)n; i++) {
        const double *p = &in[7 * i];
        out[i] = subpixel_residual(subpixel_reproj_err2(Ac, p, p[3], p[4]), subpixel_reproj_err2(Ap, p, p[5], p[6]));
    }
    f = std::fopen(argv[2], "wb");
    if (!f) return 2;
    ok = std::fwrite(out.data(), sizeof(float), out.size(), f) == out.size();
    return std::fclose(f) == 0 && ok ? 0 : 2;
}
