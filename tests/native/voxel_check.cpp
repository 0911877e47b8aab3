// CPU side of tests/test_voxel_arith.py: the arithmetic of the voxel grid in 3dscan_amd/csrc/sl3d_voxel.h (the header k_voxel_insert,
// k_voxel_count and k_voxel_scatter compile) as a stand-alone program, built by g++ plainly and with -fsanitize=address,undefined.
//   voxel_check cells    in out : in = float leaf, float x[n]                              out = {double c, int64 q, int32 ok, int32 0}[n]
//   voxel_check keys     in out : in = int32 c[n][3], in range                             out = {uint64 key, uint64 hash}[n]
//   voxel_check centroid in out : in = {double c, int64 S, uint32 count, float leaf}[n]    out = float[n]
//   voxel_check capacity in out : in = int64 n[m]                                          out = uint64[m]
// q is computed for the coordinates that are in range only (the kernels do the same), 0 otherwise.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../3dscan_amd/csrc/sl3d_voxel.h"

struct CellOut {
    double c;
    int64_t q;
    int32_t ok, pad;
};
struct CentroidIn {
    double c;
    int64_t S;
    uint32_t count;
    float leaf;
};
struct KeyOut {
    uint64_t key, hash;
};

static std::vector<char> slurp(const char *path)
{
    std::vector<char> b;
    FILE *f = fopen(path, "rb");
    if (!f) return b;
    char buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) b.insert(b.end(), buf, buf + n);
    fclose(f);
    return b;
}

template <typename T>
static int dump(const char *path, const std::vector<T> &v)
{
    FILE *f = fopen(path, "wb");
    if (!f) return 1;
    const size_t n = fwrite(v.data(), sizeof(T), v.size(), f);
    return (fclose(f) != 0 || n != v.size()) ? 1 : 0;
}

int main(int argc, char **argv)
{
    if (argc != 4) return 2;
    const std::string what = argv[1];
    const std::vector<char> in = slurp(argv[2]);
    if (what == "cells") {
        if (in.size() < sizeof(float)) return 2;
        float leaf;
        memcpy(&leaf, in.data(), sizeof leaf);
        const size_t n = in.size() / sizeof(float) - 1;
        std::vector<CellOut> out(n);
        for (size_t i = 0; i < n; i++) {
            float x;
            memcpy(&x, in.data() + (i + 1) * sizeof(float), sizeof x);
            CellOut o = {0.0, 0, 0, 0};
            o.ok = voxel_cell(x, (double)leaf, &o.c);
            if (o.ok) o.q = voxel_q(x, o.c, (double)leaf);
            out[i] = o;
        }
        return dump(argv[3], out);
    }
    if (what == "keys") {
        const size_t n = in.size() / (3 * sizeof(int32_t));
        std::vector<KeyOut> out(n);
        for (size_t i = 0; i < n; i++) {
            int32_t c[3];
            memcpy(c, in.data() + i * sizeof c, sizeof c);
            out[i].key = voxel_key((double)c[0], (double)c[1], (double)c[2]);
            out[i].hash = voxel_hash(out[i].key);
        }
        return dump(argv[3], out);
    }
    if (what == "centroid") {
        const size_t n = in.size() / sizeof(CentroidIn);
        std::vector<float> out(n);
        for (size_t i = 0; i < n; i++) {
            CentroidIn r;
            memcpy(&r, in.data() + i * sizeof r, sizeof r);
            out[i] = voxel_centroid(r.c, (double)r.leaf, r.S, r.count);
        }
        return dump(argv[3], out);
    }
    if (what == "capacity") {
        const size_t n = in.size() / sizeof(int64_t);
        std::vector<uint64_t> out(n);
        for (size_t i = 0; i < n; i++) {
            int64_t v;
            memcpy(&v, in.data() + i * sizeof v, sizeof v);
            out[i] = voxel_table_capacity(v);
        }
        return dump(argv[3], out);
    }
    return 2;
}
