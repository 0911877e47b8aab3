// direct_gray_check.cpp -- CPU check of 3dscan_amd/csrc/sl3d_direct_gray.h, the header k_unwrap_direct, k_direct_gray, sl3d_create and
// sl3d_group_create compile (no HIP here).
//   direct_gray_check               the rules around the bit: which flag combinations are refused and what the refusals say, the planes read,
//                                   the bit over every (gray, I0, I2), and the packed forms (two pixels per word) against the scalar ones in
//                                   every byte position with hostile neighbours; exit 0 iff all are right
//   direct_gray_check <in> <out>    the decode over a list of pixels
//   <in>:  int64 n (a multiple of 4); int32 N; uint8 i0[n], i2[n], gray[N][n]
//   <out>: int32 code[n]: direct_gray_code per pixel; int32 packed[n]: the same through direct_gray_sum2 / _step2 / _field, four
//          consecutive pixels as the bytes of one dword
// tests/test_direct_gray_arith.py compares <out> with the NumPy restatement, also under ASan / UBSan.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../3dscan_amd/csrc/sl3d_direct_gray.h"

static int failures = 0;
#define EXPECT(cond)                                                         \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);          \
            failures++;                                                      \
        }                                                                    \
    } while (0)

static bool says(const char *text, const char *word) { return text && std::strstr(text, word); }

static unsigned dword(const unsigned char b[4]) { return (unsigned)b[0] | (unsigned)b[1] << 8 | (unsigned)b[2] << 16 | (unsigned)b[3] << 24; }

static int self_check()
{
    // (direct, subpixel, repair)
    EXPECT(!direct_gray_refusal(false, false, false) && !direct_gray_refusal(false, true, true) && !direct_gray_refusal(false, false, true));
    EXPECT(!direct_gray_refusal(true, true, false));
    const char *alone = direct_gray_refusal(true, false, false), *rep = direct_gray_refusal(true, true, true);
    EXPECT(says(alone, "SL3D_FLAG_DIRECT_GRAY") && says(alone, "add SL3D_FLAG_SUBPIXEL"));
    EXPECT(says(rep, "SL3D_FLAG_DIRECT_GRAY") && says(rep, "SL3D_FLAG_REPAIR_PERIODS") && says(rep, "no direct form"));
    EXPECT(direct_gray_refusal(true, false, true) == alone);  // (everything wrong: the first refusal)
    EXPECT(SL3D_DIRECT_GRAY_BIT == 4096u);
    EXPECT(direct_gray_planes(3, 10) == 13 && direct_gray_planes(4, 0) == 4);
    // the bit, ties -> 1
    EXPECT(direct_gray_bit(0, 0, 0) == 1 && direct_gray_bit(0, 1, 0) == 0 && direct_gray_bit(255, 255, 255) == 1 && direct_gray_bit(254, 255, 254) == 0);
    EXPECT(direct_gray_bit(17, 17, 17) == 1 && direct_gray_bit(17, 18, 17) == 0 && direct_gray_bit(17, 16, 17) == 1);
    long checked = 0;
    for (int g = 0; g < 256; g++)
        for (int i0 = 0; i0 < 256; i0++)
            for (int i2 = 0; i2 < 256; i2++) {
                const int want = 2 * g >= i0 + i2 ? 1 : 0;
                if (direct_gray_bit(g, i0, i2) != want) failures++;
                checked++;
            }
    EXPECT(checked == 256L * 256 * 256);
    // the packed bit: pixel k's field against the scalar bit, the other three bytes of every dword at both extremes
    for (int g = 0; g < 256; g++)
        for (int s = 0; s <= 510; s++) {
            const int i0 = s < 255 ? s : 255, i2 = s - i0;
            for (int k = 0; k < 4; k++)
                for (int fill = 0; fill < 4; fill++) {
                    unsigned char bg[4], b0[4], b2[4];
                    for (int j = 0; j < 4; j++) {
                        bg[j] = fill & 1 ? 255 : 0;
                        b0[j] = b2[j] = fill & 2 ? 255 : 0;
                    }
                    bg[k] = (unsigned char)g, b0[k] = (unsigned char)i0, b2[k] = (unsigned char)i2;
                    const unsigned s2 = direct_gray_sum2(dword(b0), dword(b2), k & 1);
                    const unsigned bit2 = direct_gray_bit2(dword(bg), s2, k & 1);
                    if ((bit2 & ~0x00010001u) != 0u) failures++;
                    if ((int)((bit2 >> (16 * (k >> 1))) & 0xffffu) != direct_gray_bit(g, i0, i2)) failures++;
                    const int other = direct_gray_bit(bg[k ^ 2], b0[k ^ 2], b2[k ^ 2]);  // the other field of the word
                    if ((int)((bit2 >> (16 * ((k >> 1) ^ 1))) & 0xffffu) != other) failures++;
                }
        }
    // the packed chain: 16 planes fill a field exactly (code 0xffff beside code 0, in both arrangements)
    for (int arrangement = 0; arrangement < 2; arrangement++) {
        unsigned char i0[4] = {10, 10, 10, 10}, i2[4] = {10, 10, 10, 10};
        unsigned be = 0, bo = 0, ce = 0, co = 0;
        const unsigned se = direct_gray_sum2(dword(i0), dword(i2), 0), so = direct_gray_sum2(dword(i0), dword(i2), 1);
        unsigned char col[4][16];
        for (int i = 0; i < 16; i++) {
            unsigned char g[4];
            for (int k = 0; k < 4; k++) {
                const bool ones = (k >> 1) == arrangement;  // G = 1, 0, 0, ... keeps b at 1: code 0xffff; all dark gives 0
                g[k] = ones && i == 0 ? 200 : 0;
                col[k][i] = g[k];
            }
            direct_gray_step2(dword(g), se, 0, be, ce);
            direct_gray_step2(dword(g), so, 1, bo, co);
        }
        for (int k = 0; k < 4; k++) EXPECT(direct_gray_field(ce, co, k) == direct_gray_code(col[k], 16, 10, 10));
        int full = 0;
        for (int k = 0; k < 4; k++) full += direct_gray_field(ce, co, k) == 0xffff;
        EXPECT(full == 2);
    }
    if (failures) std::fprintf(stderr, "%d checks failed\n", failures);
    return failures ? 1 : 0;
}

int main(int argc, char **argv)
{
    if (argc == 1) return self_check();
    if (argc != 3) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t n = 0;
    int32_t N = 0;
    if (std::fread(&n, sizeof n, 1, f) != 1 || std::fread(&N, sizeof N, 1, f) != 1 || n < 4 || n % 4 || N < 0 || N > 16) return 2;
    std::vector<unsigned char> i0((size_t)n), i2((size_t)n), gray((size_t)N * (size_t)n);
    if (std::fread(i0.data(), 1, (size_t)n, f) != (size_t)n || std::fread(i2.data(), 1, (size_t)n, f) != (size_t)n) return 2;
    if (N && std::fread(gray.data(), 1, gray.size(), f) != gray.size()) return 2;
    std::fclose(f);
    std::vector<int32_t> code((size_t)n), packed((size_t)n);
    std::vector<unsigned char> column((size_t)N + 1);
    for (int64_t p = 0; p < n; p++) {
        for (int i = 0; i < N; i++) column[(size_t)i] = gray[(size_t)i * (size_t)n + (size_t)p];
        code[(size_t)p] = direct_gray_code(column.data(), N, i0[(size_t)p], i2[(size_t)p]);
    }
    for (int64_t q = 0; q < n; q += 4) {
        const unsigned se = direct_gray_sum2(dword(&i0[(size_t)q]), dword(&i2[(size_t)q]), 0), so = direct_gray_sum2(dword(&i0[(size_t)q]), dword(&i2[(size_t)q]), 1);
        unsigned be = 0, bo = 0, ce = 0, co = 0;
        for (int i = 0; i < N; i++) {
            const unsigned g = dword(&gray[(size_t)i * (size_t)n + (size_t)q]);
            direct_gray_step2(g, se, 0, be, ce);
            direct_gray_step2(g, so, 1, bo, co);
        }
        for (int k = 0; k < 4; k++) packed[(size_t)q + k] = direct_gray_field(ce, co, k);
    }
    f = std::fopen(argv[2], "wb");
    if (!f) return 2;
    const bool ok = std::fwrite(code.data(), sizeof(int32_t), (size_t)n, f) == (size_t)n && std::fwrite(packed.data(), sizeof(int32_t), (size_t)n, f) == (size_t)n;
    return std::fclose(f) == 0 && ok ? 0 : 1;
}
