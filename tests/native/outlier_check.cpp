// CPU side of tests/test_outlier_arith.py: the arithmetic of the radius outlier filter in 3dscan_amd/csrc/sl3d_outlier.h (the header the
// kernels compile) over pitched planes the test wrote, as raw arrays the test compares with its NumPy restatement.
//   outlier_check IN OUT
//   IN   int32 n_cases, then per case: int32 W, H, pitch, radius, min_neighbours; float32 max_dist; uint8 valid[H * pitch];
//        float32 points[H * pitch * 3] -- the padding columns [W, pitch) hold whatever the test poisoned them with
//   OUT  per case: uint8 support[H * W] (outlier_support of every window pixel), uint8 rejected[H * W] (outlier_rejected of every sample)
// Every plane is a heap allocation of exactly its size.  Built twice by the test: plainly, and with -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../3dscan_amd/csrc/sl3d_outlier.h"

static bool read_all(FILE *f, void *p, size_t bytes) { return bytes == 0 || std::fread(p, 1, bytes, f) == bytes; }

int main(int argc, char **argv)
{
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
        return 2;
    }
    FILE *in = std::fopen(argv[1], "rb"), *out = std::fopen(argv[2], "wb");
    if (!in || !out) return 1;
    int32_t n_cases = 0;
    if (!read_all(in, &n_cases, sizeof n_cases)) return 1;
    for (int32_t k = 0; k < n_cases; k++) {
        int32_t h[5];
        float max_dist;
        if (!read_all(in, h, sizeof h) || !read_all(in, &max_dist, sizeof max_dist)) return 1;
        const int W = h[0], H = h[1], pitch = h[2], radius = h[3], min_neighbours = h[4];
        if (W < 1 || H < 1 || pitch < W || radius < 1 || radius > SL3D_OUTLIER_MAX_RADIUS || min_neighbours < 0 ||
            min_neighbours > outlier_max_support(radius))
            return 3;
        std::vector<uint8_t> valid((size_t)H * pitch);
        std::vector<float> points((size_t)H * pitch * 3);
        if (!read_all(in, valid.data(), valid.size()) || !read_all(in, points.data(), points.size() * sizeof(float))) return 1;
        const double thr2 = mesh_thr2(max_dist);
        std::vector<uint8_t> support((size_t)H * W), rejected((size_t)H * W);
        for (int r = 0; r < H; r++)
            for (int c = 0; c < W; c++) {
                const unsigned s = outlier_support(valid.data(), points.data(), W, H, pitch, r, c, radius, thr2);
                if (s != SL3D_OUTLIER_NO_SAMPLE && s > (unsigned)outlier_max_support(radius)) return 4;
                support[(size_t)r * W + c] = (uint8_t)s;
                rejected[(size_t)r * W + c] = (uint8_t)(s != SL3D_OUTLIER_NO_SAMPLE && outlier_rejected(s, min_neighbours));
            }
        if (std::fwrite(support.data(), 1, support.size(), out) != support.size() || std::fwrite(rejected.data(), 1, rejected.size(), out) != rejected.size())
            return 1;
    }
    std::fclose(in);
    return std::fclose(out) != 0;
}
