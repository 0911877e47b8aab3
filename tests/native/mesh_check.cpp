// mesh_check -- walks a frame through 3dscan_amd/csrc/sl3d_mesh.h (the header k_mesh_count / k_mesh_emit compile) with the kernels' own
// indexing: chunks of `chunk` pixels of one row, one lane per quad, the vertex id of a pixel = its chunk's offset + the valid pixels of
// the chunk in front of it, a face's position = its chunk's face offset + its rank in the chunk.
//   mesh_check XYZ VALID H W MAX_EDGE CHUNK OUT_VERTICES OUT_FACES
// XYZ: H*W*3 float32, VALID: H*W bytes (0 / 1), MAX_EDGE: a float as strtof reads it (hex floats, inf), CHUNK: a multiple of 4.
// Writes the compacted cloud (float32 triples) and the faces (int32 triples).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../3dscan_amd/csrc/sl3d_mesh.h"

struct Frame {
    int H, W;
    std::vector<float> xyz;
    std::vector<uint8_t> valid;
};

// what mesh_lane of sl3d_mesh.hip computes for the quad at (r, c0)
static void lane(const Frame &F, int r, int c0, double thr2, unsigned &v0, unsigned &v1, unsigned cell[4])
{
    v0 = v1 = 0;
    cell[0] = cell[1] = cell[2] = cell[3] = 0;
    if (c0 >= F.W) return;
    for (int j = 0; j < 5; j++)
        if (c0 + j < F.W) {
            v0 |= (unsigned)(F.valid[(size_t)r * F.W + c0 + j] & 1) << j;
            if (r + 1 < F.H) v1 |= (unsigned)(F.valid[(size_t)(r + 1) * F.W + c0 + j] & 1) << j;
        }
    if (!v0 || !v1) return;
    static const float none[3] = {0.0f, 0.0f, 0.0f};
    for (int k = 0; k < 4; k++) {
        const unsigned vb = (v0 >> k & 3u) | (v1 >> k & 3u) << 2;
        const bool right = c0 + k + 1 < F.W;
        const float *a = &F.xyz[3 * ((size_t)r * F.W + c0 + k)], *d = &F.xyz[3 * ((size_t)(r + 1) * F.W + c0 + k)];
        cell[k] = mesh_cell(vb, a, right ? a + 3 : none, d, right ? d + 3 : none, thr2);
    }
}

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
    if (argc != 9) return 2;
    Frame F;
    F.H = atoi(argv[3]), F.W = atoi(argv[4]);
    const float max_edge = strtof(argv[5], nullptr);
    const int chunk = atoi(argv[6]);
    if (F.H < 1 || F.W < 1 || chunk < 4 || chunk % 4) return 2;
    F.xyz.resize((size_t)F.H * F.W * 3);
    F.valid.resize((size_t)F.H * F.W);
    if (!read_all(argv[1], F.xyz.data(), F.xyz.size() * 4) || !read_all(argv[2], F.valid.data(), F.valid.size())) return 3;
    const double thr2 = mesh_thr2(max_edge);
    const int nck = (F.W + chunk - 1) / chunk, lanes = chunk / 4;
    // count
    std::vector<unsigned> cnt_v((size_t)F.H * nck, 0), cnt_f((size_t)F.H * nck, 0);
    for (int r = 0; r < F.H; r++)
        for (int k = 0; k < nck; k++)
            for (int t = 0; t < lanes; t++) {
                unsigned v0, v1, cell[4];
                lane(F, r, k * chunk + 4 * t, thr2, v0, v1, cell);
                cnt_v[(size_t)r * nck + k] += __builtin_popcount(v0 & 15u);
                for (int c = 0; c < 4; c++) cnt_f[(size_t)r * nck + k] += cell[c] & 3u;
            }
    // scan
    std::vector<unsigned long long> off_v(cnt_v.size()), off_f(cnt_f.size());
    unsigned long long nv = 0, nf = 0;
    for (size_t i = 0; i < cnt_v.size(); i++) {
        off_v[i] = nv, off_f[i] = nf;
        nv += cnt_v[i], nf += cnt_f[i];
    }
    // vertices: the valid pixels in scan order
    std::vector<float> verts;
    for (size_t i = 0; i < F.valid.size(); i++)
        if (F.valid[i] & 1) verts.insert(verts.end(), &F.xyz[3 * i], &F.xyz[3 * i] + 3);
    if (verts.size() != 3 * nv) return 4;
    // emit
    std::vector<int32_t> faces(3 * nf, -1);
    for (int r = 0; r + 1 < F.H; r++)
        for (int k = 0; k < nck; k++) {
            const size_t ch = (size_t)r * nck + k;
            unsigned pre0 = 0, pre1 = 0, rank = 0;  // the prefixes the block's lanes get from the wave scans
            for (int t = 0; t < lanes; t++) {
                unsigned v0, v1, cell[4];
                lane(F, r, k * chunk + 4 * t, thr2, v0, v1, cell);
                int id[2][5];
                for (int j = 0; j < 5; j++) {
                    id[0][j] = (int)off_v[ch] + (int)pre0 + __builtin_popcount(v0 & ((1u << j) - 1u));
                    id[1][j] = (int)off_v[ch + nck] + (int)pre1 + __builtin_popcount(v1 & ((1u << j) - 1u));
                }
                for (int c = 0; c < 4; c++)
                    for (int f = 0; f < (int)(cell[c] & 3u); f++) {
                        for (int j = 0; j < 3; j++) {
                            const unsigned cn = mesh_corner(cell[c], f, j);
                            faces[3 * (off_f[ch] + rank) + j] = id[cn >> 1][c + (cn & 1u)];
                        }
                        rank++;
                    }
                pre0 += __builtin_popcount(v0 & 15u);
                pre1 += __builtin_popcount(v1 & 15u);
            }
            if (rank != cnt_f[ch]) return 5;
        }
    FILE *fv = fopen(argv[7], "wb"), *ff = fopen(argv[8], "wb");
    if (!fv || !ff) return 6;
    fwrite(verts.data(), 4, verts.size(), fv);
    fwrite(faces.data(), 4, faces.size(), ff);
    fclose(fv);
    fclose(ff);
    return 0;
}
