// CPU side of tests/test_tsdf_arith.py: the arithmetic of the TSDF volume in 3dscan_amd/csrc/sl3d_tsdf.h (the header k_tsdf_integrate,
// k_tsdf_count and k_tsdf_scatter compile) as a stand-alone program, built by g++ plainly and with -fsanitize=address,undefined.
//   tsdf_check fuse in out : in  = Head, float points[V][H][W][3], uint8 valid[V][H][W]
//                            out = int64 {samples, occupied, voxels, known, m}, int32 sum[n], uint32 weight[n], float xyz[m][3], float normals[m][3],
//                                  int32 edge[m]
//   tsdf_check quant in out : in = {double z[4], a, b, zc, T}[n]   out = {int32 ok, q}[n]
// fuse walks the voxels as the kernels do: every voxel in ascending v, the views in order inside; then every known voxel and its three
// + edges.  The rotations come from the recurrence, as on the host side of the library.  Every sample is taken twice -- through the views'
// depth planes (tsdf_pixel_depth, tsdf_sample_plane: what the kernels run) and by the direct lookup (tsdf_sample) -- and the program ends
// with status 3 if the two ever differ.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../3dscan_amd/csrc/sl3d_tsdf.h"

struct Head {
    double cam[26], est[4];
    float origin[3], voxel, trunc;
    int32_t dims[3], W, H, col0, row0, V, first_step;
    int64_t min_weight;
};
struct QuantIn {
    double z[4], a, b, zc, T;
};
struct QuantOut {
    int32_t ok, q;
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
static bool put(FILE *f, const std::vector<T> &v)
{
    return v.empty() || fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
}

int main(int argc, char **argv)
{
    if (argc != 4) return 2;
    const std::string what = argv[1];
    const std::vector<char> in = slurp(argv[2]);
    if (what == "quant") {
        const size_t n = in.size() / sizeof(QuantIn);
        std::vector<QuantOut> out(n);
        for (size_t i = 0; i < n; i++) {
            QuantIn r;
            memcpy(&r, in.data() + i * sizeof r, sizeof r);
            int32_t q = 0;
            out[i].ok = tsdf_quant(r.z, r.a, r.b, r.zc, r.T, &q);
            out[i].q = out[i].ok ? q : 0;
        }
        FILE *f = fopen(argv[3], "wb");
        if (!f) return 1;
        const bool ok = put(f, out);
        return (fclose(f) != 0 || !ok) ? 1 : 0;
    }
    if (what != "fuse" || in.size() < sizeof(Head)) return 2;
    Head h;
    memcpy(&h, in.data(), sizeof h);
    if (h.W < 1 || h.H < 1 || h.V < 1 || h.first_step < 0 || h.dims[0] < 1 || h.dims[1] < 1 || h.dims[2] < 1 || h.min_weight < 1) return 2;
    const size_t px = (size_t)h.W * h.H, n = (size_t)h.dims[0] * h.dims[1] * h.dims[2];
    if (in.size() != sizeof h + (size_t)h.V * px * 13) return 2;
    std::vector<float> points((size_t)h.V * px * 3);
    std::vector<uint8_t> valid((size_t)h.V * px);
    memcpy(points.data(), in.data() + sizeof h, points.size() * sizeof(float));
    memcpy(valid.data(), in.data() + sizeof h + points.size() * sizeof(float), valid.size());
    AlignCam cam;
    static_assert(sizeof cam == sizeof h.cam, "26 doubles");
    memcpy(&cam, h.cam, sizeof cam);
    TsdfVolume vol;
    for (int a = 0; a < 3; a++) vol.o[a] = (double)h.origin[a], vol.n[a] = h.dims[a];
    vol.L = (double)h.voxel, vol.T = (double)h.trunc;
    std::vector<TsdfTurn> turns((size_t)h.V);
    TsdfTurn t = {1.0, 0.0};
    for (int m = 0; m < h.first_step + h.V; m++) {
        if (m >= h.first_step) turns[(size_t)(m - h.first_step)] = t;
        t = tsdf_next_turn(t, h.est[0], h.est[1]);
    }
    std::vector<double> depth((size_t)h.V * px);
    for (int m = 0; m < h.V; m++) {
        const TsdfFrame f = {valid.data() + (size_t)m * px, points.data() + 3 * (size_t)m * px, h.W, h.H, h.W, h.col0, h.row0};
        for (size_t i = 0; i < px; i++) depth[(size_t)m * px + i] = tsdf_pixel_depth(&f, i, &cam);
    }
    std::vector<int32_t> sum(n, 0);
    std::vector<uint32_t> weight(n, 0);
    int64_t words[5] = {0, 0, (int64_t)n, 0, 0};
    for (size_t v = 0; v < n; v++) {
        const int ijk[3] = {(int)(v % h.dims[0]), (int)(v / h.dims[0] % h.dims[1]), (int)(v / h.dims[0] / h.dims[1])};
        const double X[3] = {tsdf_centre(ijk[0], vol.L, vol.o[0]), tsdf_centre(ijk[1], vol.L, vol.o[1]), tsdf_centre(ijk[2], vol.L, vol.o[2])};
        for (int m = 0; m < h.V; m++) {
            const AlignPass a = {turns[(size_t)m].c, -turns[(size_t)m].s, h.est[2], h.est[3], 0.0, 0.0, 0.0, 0.0};
            const TsdfFrame f = {valid.data() + (size_t)m * px, points.data() + 3 * (size_t)m * px, h.W, h.H, h.W, h.col0, h.row0};
            int32_t q = 0, q2 = 0;
            const int took = tsdf_sample_plane(X, &a, &cam, &f, depth.data() + (size_t)m * px, vol.T, &q);
            if (took != tsdf_sample(X, &a, &cam, &f, vol.T, &q2) || (took && q != q2)) return 3;
            if (took) sum[v] += q, weight[v]++, words[0]++;
        }
        words[1] += weight[v] > 0;
    }
    const TsdfPlanes P = {sum.data(), weight.data(), (unsigned long long)h.min_weight};
    std::vector<float> xyz, nrm;
    std::vector<int32_t> edge;
    for (size_t v = 0; v < n; v++) {
        if (!tsdf_known(&P, v)) continue;
        words[3]++;
        const int ijk[3] = {(int)(v % h.dims[0]), (int)(v / h.dims[0] % h.dims[1]), (int)(v / h.dims[0] / h.dims[1])};
        for (int axis = 0; axis < 3; axis++) {
            double tt;
            if (!tsdf_crossing(&P, vol.n, v, ijk, axis, &tt)) continue;
            float p[3], g[3];
            tsdf_edge(&P, &vol, v, ijk, axis, tt, p, g);
            xyz.insert(xyz.end(), p, p + 3);
            nrm.insert(nrm.end(), g, g + 3);
            edge.push_back((int32_t)(3 * v + (size_t)axis));
        }
    }
    words[4] = (int64_t)edge.size();
    FILE *f = fopen(argv[3], "wb");
    if (!f) return 1;
    const bool ok = fwrite(words, sizeof words, 1, f) == 1 && put(f, sum) && put(f, weight) && put(f, xyz) && put(f, nrm) && put(f, edge);
    return (fclose(f) != 0 || !ok) ? 1 : 0;
}
