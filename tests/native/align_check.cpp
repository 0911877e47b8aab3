// CPU side of tests/test_align_arith.py: the arithmetic of the turntable refinement in 3dscan_amd/csrc/sl3d_align.h (the header k_align_pass
// compiles) as a stand-alone program, built by g++ plainly and with -fsanitize=address,undefined.
//   align_check centre in out : in = {double cam[26], est[4]; int32 col0, row0}, float p[n][3]    out = {double ph[3], cc, rr; int32 finite, ok}[n]
//   align_check d2     in out : in = {double ph[3]; float q[3]; float 0}[n]                       out = double[n]
//   align_check accept in out : in = {double ox, oz; float range, max_dist}, {double d2; float p[3], q[3]}[n]
//                                                                                                  out = {int64 t[5]; int64 ok}[n]
//   align_check solve  in out : in = {double ox, oz, est[4]; float range; int32 n_pairs}, int64 sums[n_pairs][12]
//                                                                                                  out = double est[4], stats[4]
// centre: ph is computed for every p, cc / rr / ok only for a finite p (the kernel steps no other); they are 0 where ok is 0.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../3dscan_amd/csrc/sl3d_align.h"

struct CentreHead {
    double cam[26], est[4];
    int32_t col0, row0;
};
struct CentreOut {
    double ph[3], cc, rr;
    int32_t finite, ok;
};
struct D2In {
    double ph[3];
    float q[3], pad;
};
struct AcceptHead {
    double ox, oz;
    float range, max_dist;
};
struct AcceptIn {
    double d2;
    float p[3], q[3];
};
struct AcceptOut {
    int64_t t[5], ok;
};
struct SolveHead {
    double ox, oz, est[4];
    float range;
    int32_t n_pairs;
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
    if (what == "centre") {
        if (in.size() < sizeof(CentreHead)) return 2;
        CentreHead h;
        memcpy(&h, in.data(), sizeof h);
        AlignCam cam;
        static_assert(sizeof cam == sizeof h.cam, "26 doubles");
        memcpy(&cam, h.cam, sizeof cam);
        const AlignPass a = {h.est[0], h.est[1], h.est[2], h.est[3], 0.0, 0.0, 1.0, 1.0};
        const size_t n = (in.size() - sizeof h) / (3 * sizeof(float));
        std::vector<CentreOut> out(n);
        for (size_t i = 0; i < n; i++) {
            float p[3];
            memcpy(p, in.data() + sizeof h + i * sizeof p, sizeof p);
            CentreOut o;
            memset(&o, 0, sizeof o);
            align_step(p, &a, o.ph);
            o.finite = align_finite(p);
            if (o.finite) {
                double cc = 0.0, rr = 0.0;
                o.ok = align_centre(o.ph, &cam, h.col0, h.row0, &cc, &rr);
                if (o.ok) o.cc = cc, o.rr = rr;
            }
            out[i] = o;
        }
        return dump(argv[3], out);
    }
    if (what == "d2") {
        const size_t n = in.size() / sizeof(D2In);
        std::vector<double> out(n);
        for (size_t i = 0; i < n; i++) {
            D2In r;
            memcpy(&r, in.data() + i * sizeof r, sizeof r);
            out[i] = align_d2(r.q, r.ph);
        }
        return dump(argv[3], out);
    }
    if (what == "accept") {
        if (in.size() < sizeof(AcceptHead)) return 2;
        AcceptHead h;
        memcpy(&h, in.data(), sizeof h);
        const AlignPass a = {1.0, 0.0, 0.0, 0.0, h.ox, h.oz, align_Q(h.range), align_thr2(h.max_dist)};
        const size_t n = (in.size() - sizeof h) / sizeof(AcceptIn);
        std::vector<AcceptOut> out(n);
        for (size_t i = 0; i < n; i++) {
            AcceptIn r;
            memcpy(&r, in.data() + sizeof h + i * sizeof r, sizeof r);
            AcceptOut o;
            memset(&o, 0, sizeof o);
            int64_t t[5] = {0, 0, 0, 0, 0};
            o.ok = align_accept(r.p, r.q, r.d2, &a, t);
            if (o.ok) memcpy(o.t, t, sizeof t);
            out[i] = o;
        }
        return dump(argv[3], out);
    }
    if (what == "solve") {
        if (in.size() < sizeof(SolveHead)) return 2;
        SolveHead h;
        memcpy(&h, in.data(), sizeof h);
        if (h.n_pairs < 1 || in.size() != sizeof h + (size_t)h.n_pairs * ALIGN_WORDS * sizeof(int64_t)) return 2;
        std::vector<int64_t> sums((size_t)h.n_pairs * ALIGN_WORDS);
        memcpy(sums.data(), in.data() + sizeof h, sums.size() * sizeof(int64_t));
        std::vector<double> out(8);
        align_solve(sums.data(), h.n_pairs, align_Q(h.range), h.ox, h.oz, h.est, out.data(), out.data() + 4);
        return dump(argv[3], out);
    }
    return 2;
}
