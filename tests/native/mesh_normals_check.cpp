// mesh_normals_check -- walks a frame through the vertex-normal arithmetic of 3dscan_amd/csrc/sl3d_mesh.h (the header k_mesh_normals
// compiles) with the kernel's own indexing: chunks of `chunk` pixels of one row, one lane per quad, valid bits and points of rows r - 1,
// r, r + 1 and columns c0 - 1 .. c0 + 4 (nothing beyond the frame), a normal's position = its chunk's vertex offset + the valid pixels
// of the chunk in front of it.
//   mesh_normals_check XYZ VALID H W MAX_EDGE CHUNK OUT_NORMALS
// XYZ: H*W*3 float32, VALID: H*W bytes (0 / 1), MAX_EDGE: a float as strtof reads it (hex floats, inf), CHUNK: a multiple of 4.
// Writes one float32 triple per valid pixel.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../3dscan_amd/csrc/sl3d_mesh.h"

static bool read_all(const char *path, void *dst, size_t bytes)
{
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    const bool ok = fread(dst, 1, bytes, f) == bytes;
    fclose(f);
    return ok;
}

int main(int argc, char **argv)
{
    if (argc != 8) return 2;
    const int H = atoi(argv[3]), W = atoi(argv[4]);
    const float max_edge = strtof(argv[5], nullptr);
    const int chunk = atoi(argv[6]);
    if (H < 1 || W < 1 || chunk < 4 || chunk % 4) return 2;
    std::vector<float> xyz((size_t)H * W * 3);
    std::vector<uint8_t> valid((size_t)H * W);
    if (!read_all(argv[1], xyz.data(), xyz.size() * 4) || !read_all(argv[2], valid.data(), valid.size())) return 3;
    const double thr2 = mesh_thr2(max_edge);
    const int nck = (W + chunk - 1) / chunk, lanes = chunk / 4;
    // count + scan
    std::vector<unsigned long long> off((size_t)H * nck);
    unsigned long long nv = 0;
    for (int r = 0; r < H; r++)
        for (int k = 0; k < nck; k++) {
            off[(size_t)r * nck + k] = nv;
            for (int c = k * chunk; c < W && c < (k + 1) * chunk; c++) nv += valid[(size_t)r * W + c] & 1;
        }
    std::vector<float> normals(3 * nv, -1.0f);
    for (int r = 0; r < H; r++)
        for (int k = 0; k < nck; k++) {
            unsigned long long at = off[(size_t)r * nck + k];  // (the block's lanes get this from the wave scans)
            for (int t = 0; t < lanes; t++) {
                const int c0 = k * chunk + 4 * t;
                if (c0 >= W) break;
                // what the lane of k_mesh_normals gathers
                unsigned v[3] = {0u, 0u, 0u};
                float q[3][18] = {};
                for (int i = 0; i < 3; i++) {
                    const int rr = r - 1 + i;
                    if (rr < 0 || rr >= H) continue;
                    for (int j = 0; j < 6; j++) {
                        const int c = c0 - 1 + j;
                        if (c < 0 || c >= W || !(valid[(size_t)rr * W + c] & 1)) continue;
                        v[i] |= 1u << j;
                        for (int d = 0; d < 3; d++) q[i][3 * j + d] = xyz[3 * ((size_t)rr * W + c) + d];
                    }
                }
                const unsigned own = v[1] >> 1 & 15u;
                if (!own) continue;
                double acc[12];
                mesh_quad_sums(v, q[0], q[1], q[2], thr2, acc);
                for (int j = 0; j < 4; j++)
                    if (own >> j & 1u) {
                        mesh_normal_from_sum(&acc[3 * j], &normals[3 * at]);
                        at++;
                    }
            }
            const unsigned long long end = (size_t)r * nck + k + 1 < off.size() ? off[(size_t)r * nck + k + 1] : nv;
            if (at != end) return 4;
        }
    FILE *f = fopen(argv[7], "wb");
    if (!f) return 6;
    fwrite(normals.data(), 4, normals.size(), f);
    fclose(f);
    return 0;
}
