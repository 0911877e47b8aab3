// period_check.cpp -- CPU check of 3dscan_amd/csrc/sl3d_period.h, the header the kernels of sl3d_period.hip compile (no HIP here).
//   period_check                 the argument checks of sl3d_repair_periods (period_check_args): every documented refusal, exit 0 iff right
//   period_check <in> <out>      one pass over one axis of a frame, walked with the kernels' indexing -- AXIS 0: runs of 256 pixels of 8
//                                rows staged with R halo pixels each side, AXIS 1: tiles of 64 columns x 32 rows with R halo rows, 8
//                                consecutive rows per wave, the window slid over 8 + 2R values -- and in their two passes: the jump
//                                plane (a byte per pixel, the wide plane where j does not fit), then the pointwise apply.
//   <in>:  int32 W, H, axis, radius, n_gray; int32 code[H][W]; float wrapped[H][W]; float unwrapped[H][W]; uint8 valid[H][W]
//   <out>: int32 code[H][W]; float unwrapped[H][W]; uint32 repaired, unrepairable
// tests/test_period_repair_arith.py compares <out> with the NumPy restatement bit for bit, also under ASan / UBSan.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../3dscan_amd/csrc/sl3d_period.h"

struct Frame {
    int W, H, axis, radius, n_gray;
    std::vector<int32_t> code;
    std::vector<float> wrapped, unw;
    std::vector<uint8_t> valid;
    std::vector<int8_t> jump;
    std::vector<int> wide;
    uint32_t counts[2] = {0, 0};
};

static float load(const Frame &f, int axis, int col, int row)
{
    const bool in_range = axis == 0 ? (col >= 1 && col <= f.W - 2 && row < f.H) : (row >= 1 && row <= f.H - 2 && col < f.W);
    if (!in_range) return period_no_sample();
    const size_t px = (size_t)row * f.W + col;
    return f.valid[px] == 1 ? f.unw[px] : period_no_sample();
}

template <int R>
static int pixel(Frame &f, const float (&v)[2 * R + 1], size_t px)
{
    if (!(v[R] < period_no_sample())) return 0;
    int n;
    const float m = period_median<2 * R + 1>(v, &n);
    const long j = period_sample_jump(v[R], m, n, R);
    if (j == 0) return 0;
    if (!period_in_range((long)f.code[px] - j, f.n_gray)) {
        f.counts[1]++;
        return 0;
    }
    const int b = period_byte(j);
    if (b == SL3D_PERIOD_WIDE) f.wide[px] = (int)j;
    f.counts[0]++;
    return b;
}

template <int R>
static void jumps(Frame &f)
{
    if (f.axis == 0) {
        constexpr int ROWS0 = 8, RUN = 256 + 2 * R;
        for (int r0 = 0; r0 < f.H; r0 += ROWS0)
            for (int c0 = 0; c0 < f.W; c0 += 256) {
                std::vector<float> s((size_t)ROWS0 * RUN);
                for (int i = 0; i < ROWS0 * RUN; i++) s[(size_t)i] = load(f, 0, c0 - R + i % RUN, r0 + i / RUN);
                for (int k = 0; k < ROWS0 && r0 + k < f.H; k++)
                    for (int t = 0; t < 256 && c0 + t < f.W; t++) {
                        float v[2 * R + 1];
                        for (int d = 0; d < 2 * R + 1; d++) v[d] = s[(size_t)(k * RUN + t + d)];
                        const size_t px = (size_t)(r0 + k) * f.W + c0 + t;
                        f.jump[px] = (int8_t)pixel<R>(f, v, px);
                    }
            }
        return;
    }
    constexpr int BAND = 32, ROWS = BAND / 4;
    for (int r0 = 0; r0 < f.H; r0 += BAND)
        for (int col = 0; col < f.W; col++) {
            std::vector<float> s(BAND + 2 * R);
            for (int i = 0; i < BAND + 2 * R; i++) s[(size_t)i] = load(f, 1, col, r0 - R + i);
            for (int wave = 0; wave < 4; wave++) {
                float w[ROWS + 2 * R];
                for (int i = 0; i < ROWS + 2 * R; i++) w[i] = s[(size_t)(wave * ROWS + i)];
                for (int k = 0; k < ROWS; k++) {
                    const int row = r0 + wave * ROWS + k;
                    if (row >= f.H) continue;
                    float v[2 * R + 1];
                    for (int d = 0; d < 2 * R + 1; d++) v[d] = w[k + d];
                    const size_t px = (size_t)row * f.W + col;
                    f.jump[px] = (int8_t)pixel<R>(f, v, px);
                }
            }
        }
}

static void apply(Frame &f)
{
    for (size_t px = 0; px < f.jump.size(); px++) {
        const int b = f.jump[px];
        if (!b) continue;
        const long k = (long)f.code[px] - (b == SL3D_PERIOD_WIDE ? (long)f.wide[px] : (long)b);
        f.code[px] = (int32_t)k;
        f.unw[px] = period_value(f.wrapped[px], k);
    }
}

static int check_args()
{
    int bad = 0;
    const auto expect = [&](int got, int want, const char *what) {
        if (got != want) {
            fprintf(stderr, "period_check_args: %s: %d, expected %d\n", what, got, want);
            bad++;
        }
    };
    // (view, max_views, keep, axis, radius, N_v, N_h)
    expect(period_check_args(0, 1, 1, 0, 4, 3, 3), 0, "a good call");
    expect(period_check_args(2, 3, 1, 1, 1, 3, 3), 0, "the last view, radius 1");
    expect(period_check_args(0, 1, 1, 1, 8, 0, 3), 0, "radius 8, the other axis without Gray planes");
    expect(period_check_args(-1, 1, 1, 0, 4, 3, 3), -1, "view -1");
    expect(period_check_args(3, 3, 1, 0, 4, 3, 3), -1, "view == max_views");
    expect(period_check_args(0, 1, 0, 0, 4, 3, 3), -4, "no KEEP_STAGES");
    expect(period_check_args(0, 1, 0, 2, 0, 0, 0), -4, "no KEEP_STAGES comes before the other refusals");
    expect(period_check_args(5, 1, 0, 0, 4, 3, 3), -1, "a bad view comes first");
    expect(period_check_args(0, 1, 1, 2, 4, 3, 3), -1, "axis 2");
    expect(period_check_args(0, 1, 1, -1, 4, 3, 3), -1, "axis -1");
    expect(period_check_args(0, 1, 1, 0, 0, 3, 3), -1, "radius 0");
    expect(period_check_args(0, 1, 1, 0, 9, 3, 3), -1, "radius 9");
    expect(period_check_args(0, 1, 1, 0, 4, 0, 3), -5, "N_v == 0");
    expect(period_check_args(0, 1, 1, 1, 4, 3, 0), -5, "N_h == 0");
    // the byte of the jump plane
    expect(period_byte(127), 127, "period_byte(127)");
    expect(period_byte(-127), -127, "period_byte(-127)");
    expect(period_byte(128), SL3D_PERIOD_WIDE, "period_byte(128)");
    expect(period_byte(-128), SL3D_PERIOD_WIDE, "period_byte(-128)");
    expect(period_byte(65535), SL3D_PERIOD_WIDE, "period_byte(65535)");
    expect((int)period_in_range(65535, 16), 1, "the last code of 16 planes");
    expect((int)period_in_range(65536, 16), 0, "one beyond it");
    expect((int)period_in_range(-1, 3), 0, "code -1");
    return bad ? 1 : 0;
}

int main(int argc, char **argv)
{
    if (argc == 1) return check_args();
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb");
    if (!in) return 2;
    Frame f;
    int32_t hdr[5];
    if (fread(hdr, sizeof(int32_t), 5, in) != 5) return 2;
    f.W = hdr[0], f.H = hdr[1], f.axis = hdr[2], f.radius = hdr[3], f.n_gray = hdr[4];
    if (f.W < 1 || f.H < 1 || f.W > 4096 || f.H > 4096 || period_check_args(0, 1, 1, f.axis, f.radius, f.n_gray, f.n_gray)) return 2;
    const size_t n = (size_t)f.W * f.H;
    f.code.resize(n), f.wrapped.resize(n), f.unw.resize(n), f.valid.resize(n), f.jump.assign(n, 0), f.wide.assign(n, 0);
    if (fread(f.code.data(), 4, n, in) != n || fread(f.wrapped.data(), 4, n, in) != n || fread(f.unw.data(), 4, n, in) != n ||
        fread(f.valid.data(), 1, n, in) != n)
        return 2;
    fclose(in);
    switch (f.radius) {
    case 1: jumps<1>(f); break;
    case 2: jumps<2>(f); break;
    case 3: jumps<3>(f); break;
    case 4: jumps<4>(f); break;
    case 5: jumps<5>(f); break;
    case 6: jumps<6>(f); break;
    case 7: jumps<7>(f); break;
    case 8: jumps<8>(f); break;
    }
    apply(f);
    FILE *out = fopen(argv[2], "wb");
    if (!out) return 2;
    const bool ok = fwrite(f.code.data(), 4, n, out) == n && fwrite(f.unw.data(), 4, n, out) == n && fwrite(f.counts, 4, 2, out) == 2;
    return fclose(out) == 0 && ok ? 0 : 2;
}
