// mesh_lod_check -- walks a frame through 3dscan_amd/csrc/sl3d_mesh_lod.h (the header k_lod_blocks compiles) with the kernel's own tile
// and lane indexing: per coarse row, tiles of lod_tile_cols(step, TILE_W) coarse columns; a tile row staged quad by quad (lane l: quad l),
// candidate bytes masked to the window, quads beyond it 0, the quad prefixes and the candidates between the chunk's start and the tile;
// then the kernel's three passes.  What the kernel never writes (points of quads beyond the window, rows beyond the frame) holds NaN
// and bytes of 0xfc: a position or byte the definition does not look at must not reach a result.  The ids come from the chunk offsets
// (MESH_CHUNK columns of one row) as in the kernel: the candidates are the frame's valid pixels.
//   mesh_lod_check XYZ CAND H W STEP LOD_EDGE MEAN TILE_W OUT_XYZ OUT_VALID OUT_IDS
// XYZ: H*W*3 float32, CAND: H*W bytes (bit 0), LOD_EDGE: a float as strtof reads it (hex floats, inf), TILE_W: a multiple of 4.  Writes
// H'*W' float32 triples, bytes and int32 ids (-1 under an invalid coarse pixel).
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "../../3dscan_amd/csrc/sl3d_mesh_lod.h"

static bool read_all(const char *path, void *dst, size_t bytes)
{
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    const bool ok = fread(dst, 1, bytes, f) == bytes;
    fclose(f);
    return ok;
}

static bool write_all(const char *path, const void *src, size_t bytes)
{
    FILE *f = fopen(path, "wb");
    if (!f) return false;
    const bool ok = !bytes || fwrite(src, 1, bytes, f) == bytes;
    return fclose(f) == 0 && ok;
}

int main(int argc, char **argv)
{
    if (argc != 12) return 2;
    const int H = atoi(argv[3]), W = atoi(argv[4]), step = atoi(argv[5]);
    const float lod_edge = strtof(argv[6], nullptr);
    const int mean = atoi(argv[7]), tile_w = atoi(argv[8]);
    if (H < 1 || W < 1 || step < 1 || step > LOD_MAX_STEP || tile_w < 4 || tile_w % 4 || tile_w > MESH_CHUNK) return 2;
    const size_t n_px = (size_t)H * W;
    std::vector<float> xyz(3 * n_px);
    std::vector<uint8_t> cand(n_px);
    if (!read_all(argv[1], xyz.data(), xyz.size() * 4) || !read_all(argv[2], cand.data(), cand.size())) return 3;
    const double thr2 = mesh_thr2(lod_edge);
    const int Hc = lod_coarse(H, step), Wc = lod_coarse(W, step);
    const int tc = lod_tile_cols(step, tile_w), tw = tc * step, nq = tw / 4, tiles = (Wc + tc - 1) / tc;
    if (tw % 4 || tw > MESH_CHUNK) return 2;

    // the cell pass's counts per chunk and their scan
    const int nck = (W + MESH_CHUNK - 1) / MESH_CHUNK;
    std::vector<unsigned long long> off((size_t)H * nck);
    unsigned long long nv = 0;
    for (int r = 0; r < H; r++)
        for (int k = 0; k < nck; k++) {
            off[(size_t)r * nck + k] = nv;
            for (int c = k * MESH_CHUNK; c < W && c < (k + 1) * MESH_CHUNK; c++) nv += cand[(size_t)r * W + c] & 1u;
        }

    std::vector<float> out_xyz(3 * (size_t)Hc * Wc, -1.0f);
    std::vector<uint8_t> out_valid((size_t)Hc * Wc, 0xff);
    std::vector<int32_t> out_ids((size_t)Hc * Wc, -2);
    std::vector<uint8_t> s_cand((size_t)step * tw);
    std::vector<float> s_pts(3 * (size_t)step * tw);
    std::vector<unsigned> s_qpre((size_t)step * nq), s_front(step);
    for (int R = 0; R < Hc; R++)
        for (int b = 0; b < tiles; b++) {
            const int col0 = b * tw, r0 = R * step, rows = step < H - r0 ? step : H - r0;
            std::fill(s_cand.begin(), s_cand.end(), 0xfc);
            std::fill(s_pts.begin(), s_pts.end(), NAN);
            std::fill(s_qpre.begin(), s_qpre.end(), 0xdeadu);
            std::fill(s_front.begin(), s_front.end(), 0xdeadu);
            for (int i = 0; i < rows; i++) {
                const size_t row = (size_t)(r0 + i) * W;
                unsigned before = 0;
                for (int lane = 0; lane < nq; lane++) {
                    const int c = col0 + 4 * lane;
                    unsigned n = 0;
                    for (int j = 0; j < 4; j++) {
                        const bool in = c + j < W;
                        const uint8_t v = in ? (uint8_t)(cand[row + c + j] & 1u) : 0;
                        s_cand[(size_t)i * tw + 4 * lane + j] = v;
                        n += v;
                        if (in)
                            for (int x = 0; x < 3; x++) s_pts[3 * ((size_t)i * tw + 4 * lane + j) + x] = xyz[3 * (row + c + j) + x];
                    }
                    s_qpre[(size_t)i * nq + lane] = before;
                    before += n;
                }
                unsigned front = 0;
                for (int c1 = col0 & ~(MESH_CHUNK - 1); c1 < col0; c1++) front += cand[row + c1] & 1u;
                s_front[i] = front;
            }
            // the kernel's passes: a key per block row, per block; with the mean a member bit per pixel; then a "thread" per block
            std::vector<unsigned> s_key((size_t)rows * tc), s_rep(tc);
            for (int u = 0; u < rows * tc; u++) s_key[u] = lod_row_key(s_cand.data(), tw, (u % tc) * step, u / tc, step);
            for (int t = 0; t < tc; t++) {
                unsigned key = LOD_NONE;
                for (int dr = rows - 1; dr >= 0; dr--) key = lod_key_min(key, s_key[(size_t)dr * tc + t]);  // (any order)
                s_rep[t] = key;
                if (key != lod_block_rep(s_cand.data(), tw, t * step, rows, step)) return 6;
            }
            if (mean)
                for (int p = rows * tw - 1; p >= 0; p--) {                                                  // (any order)
                    const int dr = p / tw, col = p - dr * tw, t = col / step;
                    s_cand[p] |= (uint8_t)lod_member_bit(s_cand.data(), s_pts.data(), tw, t * step, dr, col - t * step, step, s_rep[t], thr2);
                }
            for (int t = 0; t < tc; t++) {
                const int C = b * tc + t;
                if (C >= Wc) break;
                const unsigned key = s_rep[t];
                float o[3] = {0.0f, 0.0f, 0.0f};
                int32_t id = -1;
                if (key != LOD_NONE) {
                    lod_block_position(s_cand.data(), s_pts.data(), tw, t * step, rows, step, key, mean, o);
                    const int at = (int)(key & 255u), dr = at / step, c = t * step + (at - dr * step), r = r0 + dr;
                    if (col0 + c >= W || r >= H) return 5;  // a representative outside the window
                    id = (int32_t)off[(size_t)r * nck + ((col0 + c) >> 10)] +
                         (int32_t)lod_rank_in_chunk(s_cand.data() + (size_t)dr * tw, s_qpre.data() + (size_t)dr * nq, s_front[dr], col0, c);
                }
                const size_t px = (size_t)R * Wc + C;
                out_valid[px] = key != LOD_NONE;
                for (int x = 0; x < 3; x++) out_xyz[3 * px + x] = o[x];
                out_ids[px] = id;
            }
        }
    return write_all(argv[9], out_xyz.data(), out_xyz.size() * 4) && write_all(argv[10], out_valid.data(), out_valid.size()) &&
                   write_all(argv[11], out_ids.data(), out_ids.size() * 4)
               ? 0
               : 8;
}
