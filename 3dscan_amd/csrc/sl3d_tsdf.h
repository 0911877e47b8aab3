// sl3d_tsdf.h -- the arithmetic of the TSDF volume (sl3d_tsdf_reset, sl3d_tsdf_integrate, sl3d_tsdf_extract; the rule: include/sl3d_tsdf.h):
// a voxel's centre, its turn into a view's own frame, its projection into the camera, the four pixels under it, their depths, the
// truncated signed distance and its 16-bit quantisation; a voxel's value, the crossing of an edge, its position and its normal.
//
// Shared by k_tsdf_depth / k_tsdf_integrate / k_tsdf_count / k_tsdf_scatter (sl3d_tsdf.hip), by the host code (sl3d_capi_tsdf.cpp) and by the CPU check
// the test suite runs (tests/native/tsdf_check.cpp): plain C, no HIP types, each piece spelled once.  Every operation is one IEEE double
// operation, no contraction (the library is built with -ffp-contract=off), in the order the parentheses give:
//
//   X_a      = ((double)i_a + 0.5) * L + (double)origin[a]                                                                  (tsdf_centre)
//   P        = (c_m * x - (-s_m) * z) + tx, X.y, ((-s_m) * x + c_m * z) + tz with x = X.x - tx, z = X.z - tz                 (tsdf_step)
//   xc, u, v = P into the camera as a pass takes p^ there, u and v left unrounded                                          (align_project, sl3d_align.h)
//   fu, fv   = floor(u) - col0, floor(v) - row0: a cell iff 0 <= fu, fu + 1 < W, 0 <= fv, fv + 1 < H; a, b = u - floor(u), v - floor(v)
//   z_dxdy   = ((Rc[6] * q.x + Rc[7] * q.y) + Rc[8] * q.z) + tc[2] of a pixel with valid == 1 and a finite q               (tsdf_depth)
//   zq       = ((z00 * (1 - a) + z10 * a) * (1 - b)) + ((z01 * (1 - a) + z11 * a) * b) unless max z - min z > T
//   sdf      = zq - xc.z, a sample iff sdf >= -T;  d = sdf / T, at most 1;  q = (int32)rint(d * 32767.0)                    (tsdf_quant)
//   f        = (double)sum / (double)weight of a voxel with weight >= min_weight                                           (tsdf_value)
//   t        = f0 / (f0 - f1) on an edge with (f0 < 0) != (f1 < 0);  the normal from the gradients of the two ends          (tsdf_edge)
#pragma once
#include <math.h>
#include <stdint.h>

#include "sl3d_align.h"  // AlignCam, AlignPass, align_finite, SL3D_MESH_FN

#define TSDF_MAX_VOXELS 268435456  // 2^28: 3 * v + 2 fits an int32
#define TSDF_MAX_STEPS 65535       // views since the last reset, and turntable indices: |sum| <= 65535 * 32767 < 2^31
#define TSDF_Q_ONE 32767.0
// the 64-bit words of the calls: the samples an integration took, the voxels with weight > 0 behind it; the known voxels of an
// extraction and its crossings (the scan's total)
enum { TSDF_WORD_SAMPLES, TSDF_WORD_OCCUPIED, TSDF_WORD_KNOWN, TSDF_WORD_CROSSINGS, TSDF_WORDS };

// the volume as the arithmetic uses it: origin, voxel and trunc as doubles, the dims
struct TsdfVolume {
    double o[3], L, T;
    int n[3];
};
// the rotation of one view of a call: (c_m, s_m) of its turntable index m
struct TsdfTurn {
    double c, s;
};
// a frame's dense planes as a sample reads them: rows pitch pixels apart, a window of W x H at (col0, row0) of the camera frame
struct TsdfFrame {
    const uint8_t *valid;
    const float *points;
    int W, H, pitch, col0, row0;
};

SL3D_MESH_FN double tsdf_centre(int i, double L, double o) { return ((double)i + 0.5) * L + o; }

// c_{m+1}, s_{m+1} from c_m, s_m and the estimate's (c, s)
SL3D_MESH_FN struct TsdfTurn tsdf_next_turn(struct TsdfTurn t, double c, double s)
{
    const struct TsdfTurn n = {t.c * c - t.s * s, t.s * c + t.c * s};
    return n;
}

// step 1: align_step (sl3d_align.h) over a double point -- a: (c_m, -s_m, tx, tz).  Its own text for the reason given there
SL3D_MESH_FN void tsdf_step(const double *p, const struct AlignPass *a, double *ph)
{
    const double x = p[0] - a->tx, z = p[2] - a->tz;
    ph[0] = (a->c * x - a->s * z) + a->tx;
    ph[1] = p[1];
    ph[2] = (a->s * x + a->c * z) + a->tz;
}

// step 2 is align_project (sl3d_align.h).  step 3: the window pixel (c, r) of the upper left of the four, the weights a and b.  0: no sample
// (NaN fails every comparison)
SL3D_MESH_FN int tsdf_cell(double u, double v, int W, int H, int col0, int row0, int *c, int *r, double *a, double *b)
{
    const double flu = floor(u), flv = floor(v);
    const double fu = flu - (double)col0, fv = flv - (double)row0;
    if (!(0.0 <= fu && fu + 1.0 < (double)W && 0.0 <= fv && fv + 1.0 < (double)H)) return 0;
    *c = (int)fu, *r = (int)fv;
    *a = u - flu, *b = v - flv;
    return 1;
}

// step 4: the camera depth of a pixel's point
SL3D_MESH_FN double tsdf_depth(const float *q, const struct AlignCam *m)
{
    return ((m->Rc[6] * (double)q[0] + m->Rc[7] * (double)q[1]) + m->Rc[8] * (double)q[2]) + m->tc[2];
}

// steps 5 to 7: z = z00, z10, z01, z11; zc = xc.z.  1: a sample, *q its vote
SL3D_MESH_FN int tsdf_quant(const double *z, double a, double b, double zc, double T, int32_t *q)
{
    double lo = z[0], hi = z[0];
    for (int i = 1; i < 4; i++) {
        if (z[i] < lo) lo = z[i];
        if (z[i] > hi) hi = z[i];
    }
    if (!(hi - lo <= T)) return 0;
    const double zq = ((z[0] * (1.0 - a) + z[1] * a) * (1.0 - b)) + ((z[2] * (1.0 - a) + z[3] * a) * b);
    const double sdf = zq - zc;
    if (!(sdf >= -T)) return 0;
    double d = sdf / T;
    if (d > 1.0) d = 1.0;
    *q = (int32_t)rint(d * TSDF_Q_ONE);
    return 1;
}

// steps 1 to 7 of one voxel centre X and one view: a = (c_m, -s_m, tx, tz)
SL3D_MESH_FN int tsdf_sample(const double *X, const struct AlignPass *a, const struct AlignCam *m, const struct TsdfFrame *f, double T, int32_t *q)
{
    double P[3], u, v, zc, wa, wb, z[4];
    int c, r;
    tsdf_step(X, a, P);
    if (!align_project(P, m, &u, &v, &zc)) return 0;
    if (!tsdf_cell(u, v, f->W, f->H, f->col0, f->row0, &c, &r, &wa, &wb)) return 0;
    for (int k = 0; k < 4; k++) {  // (dx, dy) = (0, 0), (1, 0), (0, 1), (1, 1)
        const size_t px = (size_t)(r + (k >> 1)) * (size_t)f->pitch + (size_t)(c + (k & 1));
        if (f->valid[px] != 1) return 0;
        const float p[3] = {f->points[3 * px], f->points[3 * px + 1], f->points[3 * px + 2]};
        if (!align_finite(p)) return 0;
        z[k] = tsdf_depth(p, m);
    }
    return tsdf_quant(z, wa, wb, zc, T, q);
}

// The same through a view's depth plane -- what k_tsdf_integrate runs: a pre-pass (k_tsdf_depth) leaves per pixel of the window its camera
// depth as a double, NaN where the pixel is not usable (valid != 1 or a coordinate that is not finite), and a sample gathers four doubles
// instead of four bytes and four points.  The depth of a usable pixel is finite (a finite camera, finite floats), so the NaN is the
// pixel's state and nothing else, and both forms give the same bits (tests/native/tsdf_check.cpp runs one against the other).
SL3D_MESH_FN double tsdf_pixel_depth(const struct TsdfFrame *f, size_t px, const struct AlignCam *m)
{
    const float p[3] = {f->points[3 * px], f->points[3 * px + 1], f->points[3 * px + 2]};
    return f->valid[px] == 1 && align_finite(p) ? tsdf_depth(p, m) : (double)NAN;
}

SL3D_MESH_FN int tsdf_sample_plane(const double *X, const struct AlignPass *a, const struct AlignCam *m, const struct TsdfFrame *f, const double *zp,
                                   double T, int32_t *q)
{
    double P[3], u, v, zc, wa, wb, z[4];
    int c, r;
    tsdf_step(X, a, P);
    if (!align_project(P, m, &u, &v, &zc)) return 0;
    if (!tsdf_cell(u, v, f->W, f->H, f->col0, f->row0, &c, &r, &wa, &wb)) return 0;
    for (int k = 0; k < 4; k++) {
        z[k] = zp[(size_t)(r + (k >> 1)) * (size_t)f->pitch + (size_t)(c + (k & 1))];
        if (z[k] != z[k]) return 0;
    }
    return tsdf_quant(z, wa, wb, zc, T, q);
}

// ---- extraction ---------------------------------------------------------------------------------------------------------------------------
// the planes of a volume as extraction reads them; mw: min_weight (>= 1)
struct TsdfPlanes {
    const int32_t *sum;
    const uint32_t *weight;
    unsigned long long mw;
};

SL3D_MESH_FN int tsdf_known(const struct TsdfPlanes *p, size_t v) { return (unsigned long long)p->weight[v] >= p->mw; }
SL3D_MESH_FN double tsdf_value(const struct TsdfPlanes *p, size_t v) { return (double)p->sum[v] / (double)p->weight[v]; }

// elements between a voxel and its + neighbour along axis
SL3D_MESH_FN size_t tsdf_stride(const int *n, int axis) { return axis == 0 ? (size_t)1 : axis == 1 ? (size_t)n[0] : (size_t)n[0] * (size_t)n[1]; }

// the gradient component along `axis` of the known voxel v, whose coordinate along that axis is c
SL3D_MESH_FN double tsdf_gradient(const struct TsdfPlanes *p, const int *n, size_t v, int c, int axis)
{
    const size_t s = tsdf_stride(n, axis);
    const int minus = c > 0 && tsdf_known(p, v - s), plus = c + 1 < n[axis] && tsdf_known(p, v + s);
    if (minus && plus) return (tsdf_value(p, v + s) - tsdf_value(p, v - s)) * 0.5;
    if (plus) return tsdf_value(p, v + s) - tsdf_value(p, v);
    if (minus) return tsdf_value(p, v) - tsdf_value(p, v - s);
    return 0.0;
}

// does the edge from the known voxel v0 = (ijk) along `axis` carry a crossing?  *t then
SL3D_MESH_FN int tsdf_crossing(const struct TsdfPlanes *p, const int *n, size_t v0, const int *ijk, int axis, double *t)
{
    if (!(ijk[axis] + 1 < n[axis])) return 0;
    const size_t v1 = v0 + tsdf_stride(n, axis);
    if (!tsdf_known(p, v1)) return 0;
    const double f0 = tsdf_value(p, v0), f1 = tsdf_value(p, v1);
    if ((f0 < 0.0) == (f1 < 0.0)) return 0;
    *t = f0 / (f0 - f1);
    return 1;
}

// the position and the normal of the crossing at t on that edge
SL3D_MESH_FN void tsdf_edge(const struct TsdfPlanes *p, const struct TsdfVolume *vol, size_t v0, const int *ijk, int axis, double t, float *xyz, float *nrm)
{
    const int *n = vol->n;
    const size_t v1 = v0 + tsdf_stride(n, axis);
    double g[3];
    for (int b = 0; b < 3; b++) {
        const double X = tsdf_centre(ijk[b], vol->L, vol->o[b]);
        xyz[b] = b == axis ? (float)(X + t * vol->L) : (float)X;
        const int c1 = b == axis ? ijk[b] + 1 : ijk[b];
        g[b] = (tsdf_gradient(p, n, v0, ijk[b], b) * (1.0 - t)) + (tsdf_gradient(p, n, v1, c1, b) * t);
    }
    const double len = sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);
    const int ok = len > 0.0 && isfinite(len);
    for (int b = 0; b < 3; b++) nrm[b] = ok ? (float)(g[b] / len) : (float)NAN;
}
