// CPU side of tests/test_exposure_arith.py: the arithmetic of the exposure fusion in 3dscan_amd/csrc/sl3d_exposure.h (the header the kernel
// compiles), written as raw arrays the test compares with its NumPy restatement.
//   exposure_check score3 OUT        uint32[2^24]   exp_score(3, I0, I1, I2, 0) of every triple, t = I0 << 16 | I1 << 8 | I2
//   exposure_check score4 OUT        uint32[2^20]   exp_score(4, I0, I1, I2, I3) of the bytes of hash(t), t = 0 .. 2^20 - 1 (I0 the lowest)
//   exposure_check keys OUT          uint32[73*4*8] exp_key(n, q, e) over n = 0 .. 72, q in {0, 1, 325124, 325125}, e = 0 .. 7, e fastest
//   exposure_check clipped OUT       uint8[256*256] byte 0 of exp_clipped4 for saturation s = 1 .. 256 (row s - 1) and byte x in all four
//                                                   places of the dword among other bytes; 255 if the four places disagree
//   exposure_check equal OUT         uint8[8*8]     byte 0 .. 3 of exp_bytes_equal agree with c == e, for c, e = 0 .. 7 (1 = as expected)
// Built twice by the test: plainly, and with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../3dscan_amd/csrc/sl3d_exposure.h"

static unsigned hash32(unsigned t)
{
    t ^= t >> 16, t *= 0x7feb352du, t ^= t >> 15, t *= 0x846ca68bu, t ^= t >> 16;
    return t;
}

static int write_all(const char *path, const void *p, size_t bytes)
{
    FILE *f = std::fopen(path, "wb");
    if (!f) return 1;
    const size_t w = std::fwrite(p, 1, bytes, f);
    return (std::fclose(f) != 0 || w != bytes) ? 1 : 0;
}

int main(int argc, char **argv)
{
    if (argc == 3 && !std::strcmp(argv[1], "score3")) {
        std::vector<unsigned> s(1u << 24);
        for (unsigned t = 0; t < (1u << 24); t++) s[t] = exp_score(3, (int)(t >> 16), (int)((t >> 8) & 0xffu), (int)(t & 0xffu), 0);
        return write_all(argv[2], s.data(), s.size() * sizeof(unsigned));
    }
    if (argc == 3 && !std::strcmp(argv[1], "score4")) {
        std::vector<unsigned> s(1u << 20);
        for (unsigned t = 0; t < (1u << 20); t++) {
            const unsigned h = hash32(t);
            s[t] = exp_score(4, (int)(h & 0xffu), (int)((h >> 8) & 0xffu), (int)((h >> 16) & 0xffu), (int)(h >> 24));
        }
        return write_all(argv[2], s.data(), s.size() * sizeof(unsigned));
    }
    if (argc == 3 && !std::strcmp(argv[1], "keys")) {
        static const unsigned Q[4] = {0u, 1u, SL3D_EXP_MAX_SCORE - 1u, SL3D_EXP_MAX_SCORE};
        std::vector<unsigned> k;
        for (unsigned n = 0; n <= 72; n++)
            for (unsigned q = 0; q < 4; q++)
                for (unsigned e = 0; e < 8; e++) {
                    const unsigned key = exp_key(n, Q[q], e);
                    if (exp_key_exposure(key) != e || exp_key_clipped(key) != n) return 3;
                    k.push_back(key);
                }
        return write_all(argv[2], k.data(), k.size() * sizeof(unsigned));
    }
    if (argc == 3 && !std::strcmp(argv[1], "clipped")) {
        std::vector<unsigned char> c(256 * 256);
        for (int s = 1; s <= 256; s++) {
            const struct ExpClipTest T = exp_clip_test(s);
            for (unsigned x = 0; x < 256; x++) {
                const unsigned others = hash32((unsigned)s * 256u + x);
                unsigned got = 2u;
                for (int k = 0; k < 4; k++) {
                    const unsigned w = (others & ~(0xffu << (8 * k))) | (x << (8 * k));
                    const unsigned r = exp_clipped4(w, T);
                    unsigned ok = (r & 0xfefefefeu) == 0u;  // nothing but bit 0 of a byte
                    for (int j = 0; j < 4; j++) ok &= ((r >> (8 * j)) & 1u) == (unsigned)((int)((w >> (8 * j)) & 0xffu) >= s);
                    const unsigned bit = (r >> (8 * k)) & 1u;
                    got = !ok ? 255u : got == 2u ? bit : got == bit ? bit : 255u;
                }
                c[(size_t)(s - 1) * 256 + x] = (unsigned char)got;
            }
        }
        return write_all(argv[2], c.data(), c.size());
    }
    if (argc == 3 && !std::strcmp(argv[1], "equal")) {
        std::vector<unsigned char> c(64);
        for (unsigned a = 0; a < 8; a++)
            for (unsigned e = 0; e < 8; e++) {
                unsigned ok = 1u;
                for (int k = 0; k < 4; k++) {
                    const unsigned w = (0x03060105u & ~(0xffu << (8 * k))) | (a << (8 * k));
                    const unsigned m = exp_bytes_equal(w, e);
                    for (int j = 0; j < 4; j++) ok &= ((m >> (8 * j)) & 0xffu) == ((((w >> (8 * j)) & 0xffu) == e) ? 0xffu : 0u);
                }
                c[a * 8 + e] = (unsigned char)ok;
            }
        return write_all(argv[2], c.data(), c.size());
    }
    std::fprintf(stderr, "usage: %s score3 | score4 | keys | clipped | equal  OUT\n", argv[0]);
    return 2;
}
