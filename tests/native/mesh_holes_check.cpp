// mesh_holes_check -- walks a frame through 3dscan_amd/csrc/sl3d_mesh_holes.h (the header the kernels of sl3d_mesh_holes.hip compile) with
// the kernels' own chunk and lane indexing: per row, chunks of CHUNK_W columns; a pixel starts as the child of the first pixel of its
// row run inside the chunk or as HOLE_OUTSIDE (k_hole_init); a run joins the run across the chunk seam and the runs it overlaps in the
// next row (k_hole_union); every non-candidate pixel stores its root and the root's size grows (k_hole_flatten); the pixels of a
// qualifying component walk to their rim and take hole_position (k_hole_fill).  With THREADS > 1 the chunks of a pass are dealt out to
// threads over std::atomic labels, with every iteration bound armed, and a pass ends before the next begins -- as kernels do.  Rows are
// PITCH = W rounded up to 16 apart; the padding columns hold candidate bytes of 1 and NaN points, and every point under a non-candidate
// is NaN: what the definition does not look at must not reach a result.
//   mesh_holes_check XYZ CAND H W MAX_HOLE FILL_EDGE CHUNK_W THREADS OUT_XYZ OUT_VALID OUT_STATS
// XYZ: H*W*3 float32, CAND: H*W bytes (bit 0), FILL_EDGE: a float as strtof reads it (hex floats, inf), CHUNK_W: a multiple of 4.
// Writes H*W float32 triples (0 under an invalid pixel of the filled grid), H*W bytes and two int64: holes, filled pixels.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <atomic>
#include <functional>
#include <thread>
#include <vector>

static inline int atomic_fetch_min(std::atomic<int> *p, int v)
{
    int old = p->load(std::memory_order_relaxed);
    while (v < old && !p->compare_exchange_weak(old, v, std::memory_order_relaxed)) {}
    return old;
}
#define CC_LABEL_T std::atomic<int>
#define CC_LOAD(p) ((p)->load(std::memory_order_relaxed))
#define CC_FETCH_MIN(p, v) atomic_fetch_min((p), (v))
#include "../../3dscan_amd/csrc/sl3d_mesh_holes.h"

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

// body(row, chunk) over every chunk of the frame: thread t takes chunks t, t + threads, ...; returns when all are done
static void every_chunk(int rows, int nck, int threads, const std::function<void(int, int)> &body)
{
    auto run = [&](int first) {
        for (int i = first; i < rows * nck; i += threads) body(i / nck, i % nck);
    };
    if (threads <= 1) return run(0);
    std::vector<std::thread> pool;
    for (int t = 0; t < threads; t++) pool.emplace_back(run, t);
    for (auto &t : pool) t.join();
}

int main(int argc, char **argv)
{
    if (argc != 12) return 2;
    const int H = atoi(argv[3]), W = atoi(argv[4]);
    const long long max_hole_ll = atoll(argv[5]);
    const float fill_edge = strtof(argv[6], nullptr);
    const int chunk_w = atoi(argv[7]), threads = atoi(argv[8]);
    if (H < 1 || W < 1 || max_hole_ll < 0 || chunk_w < 4 || chunk_w % 4 || threads < 1) return 2;
    const int max_hole = (int)std::min<long long>(max_hole_ll, INT32_MAX), walk = std::min(max_hole, std::max(W, H));
    const int pitch = (W + 15) & ~15, nck = (W + chunk_w - 1) / chunk_w, bound = pitch * H;
    const size_t n_px = (size_t)H * W, n_pitched = (size_t)H * pitch;
    std::vector<float> xyz(3 * n_px), pts(3 * n_pitched, NAN);
    std::vector<uint8_t> in(n_px), cand(n_pitched, 1);
    if (!read_all(argv[1], xyz.data(), xyz.size() * 4) || !read_all(argv[2], in.data(), in.size())) return 3;
    for (int r = 0; r < H; r++)
        for (int c = 0; c < W; c++) {
            const size_t p = (size_t)r * pitch + c, q = (size_t)r * W + c;
            cand[p] = in[q] & 1u;
            if (cand[p])
                for (int x = 0; x < 3; x++) pts[3 * p + x] = xyz[3 * q + x];
        }
    std::vector<std::atomic<int>> L(n_pitched), sizes(n_pitched);
    std::atomic<int> any_failed{0};
    std::atomic<long long> n_holes{0}, n_filled{0};

    // k_hole_init: the runs of a chunk, left to right
    every_chunk(H, nck, threads, [&](int r, int k) {
        const int c_end = std::min(W, (k + 1) * chunk_w);
        for (int c = k * chunk_w; c < c_end;) {
            const size_t p = (size_t)r * pitch + c;
            sizes[p].store(0, std::memory_order_relaxed);
            if (cand[p]) {
                L[p].store(HOLE_NONE, std::memory_order_relaxed);
                c++;
                continue;
            }
            int e = c;
            while (e < c_end && !cand[(size_t)r * pitch + e]) e++;
            const int lab = hole_run_outside(r, c, e, W, H, max_hole) ? HOLE_OUTSIDE : r * pitch + c;
            for (int j = c; j < e; j++) {
                L[(size_t)r * pitch + j].store(lab, std::memory_order_relaxed);
                sizes[(size_t)r * pitch + j].store(0, std::memory_order_relaxed);
            }
            c = e;
        }
    });
    // k_hole_union: a lane per quad, its pixels in turn
    every_chunk(H, nck, threads, [&](int r, int k) {
        const int c_end = std::min(W, (k + 1) * chunk_w);
        int failed = 0;
        for (int c = k * chunk_w; c < c_end && !failed; c++) {
            const size_t p = (size_t)r * pitch + c;
            if (cand[p]) continue;
            const int left = c > 0 && !cand[p - 1], below = r + 1 < H && !cand[p + pitch], below_left = r + 1 < H && c > 0 && !cand[p + pitch - 1];
            hole_pixel_unions(L.data(), (int)p, pitch, c == k * chunk_w && c > 0, left, below, below_left, bound, &failed);
        }
        if (failed) any_failed.store(1);
    });
    // k_hole_flatten
    every_chunk(H, nck, threads, [&](int r, int k) {
        const int c_end = std::min(W, (k + 1) * chunk_w);
        int failed = 0;
        for (int c = k * chunk_w; c < c_end && !failed; c++) {
            const int p = r * pitch + c;
            if (cand[p] || L[p].load(std::memory_order_relaxed) == HOLE_OUTSIDE) continue;  // (as the kernel: the background is final)
            const int root = hole_find(L.data(), p, bound, &failed);
            if (failed) break;
            if (root != p) CC_FETCH_MIN(L.data() + p, root);
            if (root != HOLE_OUTSIDE) sizes[root].fetch_add(1, std::memory_order_relaxed);
        }
        if (failed) any_failed.store(1);
    });
    // k_hole_fill
    std::vector<float> out_xyz(3 * n_px, -1.0f);
    std::vector<uint8_t> out_valid(n_px, 0xff);
    every_chunk(H, nck, threads, [&](int r, int k) {
        const int c_end = std::min(W, (k + 1) * chunk_w);
        int failed = 0;
        for (int c = k * chunk_w; c < c_end; c++) {
            const int p = r * pitch + c;
            const size_t q = (size_t)r * W + c;
            float o[3] = {0.0f, 0.0f, 0.0f};
            int valid = cand[p];
            if (cand[p]) {
                for (int x = 0; x < 3; x++) o[x] = pts[3 * (size_t)p + x];
            } else {
                const int root = L[p].load(std::memory_order_relaxed);
                if (root != HOLE_OUTSIDE && hole_qualifies(root, sizes[root].load(std::memory_order_relaxed), max_hole)) {
                    if (root == p) n_holes.fetch_add(1);
                    if (hole_fill_pixel(cand.data(), pts.data(), r, c, W, H, pitch, walk, fill_edge, o, &failed)) {
                        valid = 1;
                        n_filled.fetch_add(1);
                    }
                }
            }
            out_valid[q] = (uint8_t)valid;
            for (int x = 0; x < 3; x++) out_xyz[3 * q + x] = o[x];
        }
        if (failed) any_failed.store(1);
    });
    if (any_failed.load()) return 7;  // an iteration bound ran out
    const int64_t stats[2] = {n_holes.load(), n_filled.load()};
    return write_all(argv[9], out_xyz.data(), out_xyz.size() * 4) && write_all(argv[10], out_valid.data(), out_valid.size()) &&
                   write_all(argv[11], stats, sizeof(stats))
               ? 0
               : 8;
}
