// sl3d_exposure.hip -- gfx950 (MI355X, wave64) kernel of the exposure fusion (sl3d_fuse_exposures; the rule: include/sl3d_fuse.h, its arithmetic:
// sl3d_exposure.h):
//   k_fuse_exposures : per window pixel the exposure with the fewest clipped planes, among those the best modulated, among those the
//                      first; the planes in use of dst_view get that exposure's bytes, the exposure map its index, counts[] the tallies
// One launch per call, HBM bound: every plane in use of every exposure is read once, every plane in use of dst_view written once.
// One lane = 4 * D consecutive pixels of one row (rows start on 16-byte boundaries, the pitch is a multiple of 16): D = 1 is the dword
// form of sl3d_modulation.hip, D = 4 the 16-byte form.  The library launches D = 1 (registers and occupancy of both).
//   pass 1  walks the planes in use of each exposure: the clip count of 4 pixels is one packed dword (exp_clipped4), the fringe bytes are
//           unpacked for the score, the best key of each pixel is kept (exp_key).
//   pass 2  writes each plane in use of dst_view.  A lane whose pixels all chose one exposure -- nearly every lane -- does one load and
//           one store per plane; any other loads from each distinct chosen exposure and selects bytes.  The re-read comes out of L2 only
//           while the resident blocks' planes fit there: a whole 1080p launch is resident at once and re-reads from further away.
//   Both passes load in batches of 8 planes (clip_planes, copy_planes): 8 loads in flight per lane.
//   map     one byte per pixel, stored as D dwords.
//   counts  the waves' sums (wave_sum, sl3d_block.h) through one LDS word per count and wave, one integer atomic add per count and block
//           into words the host zeroed on the stream: integer sums, so the result does not depend on the order.
// No scratch, no LDS beyond those words, no inline assembly.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sl3d_block.h"
#include "sl3d_exposure.h"
#include "sl3d_internal.h"

namespace sl3d {

template <int D>
struct Run {
    unsigned w[D];
};

template <int D>
__device__ __forceinline__ Run<D> load_run(const uint8_t *p)
{
    Run<D> r;
    if constexpr (D == 1) {
        r.w[0] = *(const unsigned *)p;
    } else {
        typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
        const u32x4 v = *(const u32x4 *)p;
        r.w[0] = v.x, r.w[1] = v.y, r.w[2] = v.z, r.w[3] = v.w;
    }
    return r;
}

template <int D>
__device__ __forceinline__ void store_run(uint8_t *p, const Run<D> &r)
{
    if constexpr (D == 1) {
        *(unsigned *)p = r.w[0];
    } else {
        typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
        u32x4 v;
        v.x = r.w[0], v.y = r.w[1], v.z = r.w[2], v.w = r.w[3];
        *(u32x4 *)p = v;
    }
}

__device__ __forceinline__ int byte_of(unsigned w, int k) { return (int)((w >> (8 * k)) & 0xffu); }

// the clip counts of B planes of a lane's run added to n: B loads in flight
template <int D, int B>
__device__ __forceinline__ void clip_planes(const uint8_t *g, size_t plane_stride, const ExpClipTest T, unsigned (&n)[D])
{
    Run<D> r[B];
#pragma unroll
    for (int i = 0; i < B; i++) r[i] = load_run<D>(g + (size_t)i * plane_stride);
#pragma unroll
    for (int i = 0; i < B; i++)
#pragma unroll
        for (int j = 0; j < D; j++) n[j] += exp_clipped4(r[i].w[j], T);
}

// B planes of a lane's run from s to d (plane_stride bytes apart): all B loads, then the B stores.  Spelled as a batch because d and s
// are both the frame stack to the compiler: a load behind a store waits for it, and a plain copy loop has one load in flight per lane.
template <int D, int B>
__device__ __forceinline__ void copy_planes(uint8_t *d, const uint8_t *s, size_t plane_stride)
{
    Run<D> r[B];
#pragma unroll
    for (int i = 0; i < B; i++) r[i] = load_run<D>(s + (size_t)i * plane_stride);
#pragma unroll
    for (int i = 0; i < B; i++) store_run<D>(d + (size_t)i * plane_stride, r[i]);
}

// Lane t owns run (t mod lpr) of window row (t / lpr), lpr = runs of 4 * D pixels that hold window pixels.  Exposure e is view first_view + e
// (E of them, 1 .. SL3D_MAX_EXPOSURES; dst_view is none of them).  map: the map plane of dst_view ([row][pitch]); counts: E + 1 words.
// Pixels of the last run behind the window's last column are chosen like any other from the padding bytes (they are written inside the
// pitch, where dst_view's bytes are unspecified) and are not counted.
template <int D>
__global__ __launch_bounds__(256) void k_fuse_exposures(const KParams P, const ExposurePlan X, int first_view, int E, int dst_view, const ExpClipTest T,
                                                        uint8_t *__restrict__ map, unsigned *__restrict__ counts)
{
    __shared__ unsigned s_cnt[SL3D_EXPOSURE_COUNTS][4];
    const int lpr = (P.W + 4 * D - 1) / (4 * D);
    const unsigned t = blockIdx.x * 256u + threadIdx.x;
    const int row = (int)(t / (unsigned)lpr), q = (int)(t - (unsigned)row * (unsigned)lpr);
    const bool active = row < P.H;
    unsigned chosen[D], in_window[D];  // per pixel a byte: exposure | 0x80 if clipped there / 0x80 if the pixel is inside the window
#pragma unroll
    for (int j = 0; j < D; j++) chosen[j] = in_window[j] = 0u;
    if (active) {
        const size_t px = (size_t)row * P.pitch + (size_t)(4 * D) * q;
        // ---- pass 1: the best key of every pixel
        unsigned best[4 * D];
#pragma unroll
        for (int k = 0; k < 4 * D; k++) best[k] = 0u;
        for (int e = 0; e < E; e++) {
            const uint8_t *v = P.frames + (size_t)(first_view + e) * P.view_stride + px;
            unsigned n[D], qmin[4 * D];
#pragma unroll
            for (int j = 0; j < D; j++) n[j] = 0u;
#pragma unroll
            for (int k = 0; k < 4 * D; k++) qmin[k] = ~0u;
            for (int a = 0; a < X.n_axes; a++) {
                const uint8_t *f = v + (size_t)X.base[a] * P.plane_stride;
                const Run<D> i0 = load_run<D>(f), i1 = load_run<D>(f + P.plane_stride), i2 = load_run<D>(f + 2 * P.plane_stride);
                const Run<D> i3 = P.F == 4 ? load_run<D>(f + 3 * P.plane_stride) : i0;
#pragma unroll
                for (int j = 0; j < D; j++) {
                    n[j] += exp_clipped4(i0.w[j], T) + exp_clipped4(i1.w[j], T) + exp_clipped4(i2.w[j], T);
                    if (P.F == 4) n[j] += exp_clipped4(i3.w[j], T);
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const unsigned s = exp_score(P.F, byte_of(i0.w[j], k), byte_of(i1.w[j], k), byte_of(i2.w[j], k), byte_of(i3.w[j], k));
                        qmin[4 * j + k] = min(qmin[4 * j + k], s);
                    }
                }
                const uint8_t *g = f + (size_t)P.F * P.plane_stride;  // the Gray (and inverse) planes: clip counts only
                int left = X.count[a] - P.F;
                for (; left >= 8; left -= 8, g += 8 * P.plane_stride) clip_planes<D, 8>(g, P.plane_stride, T, n);
                if (left & 4) clip_planes<D, 4>(g, P.plane_stride, T, n), g += 4 * P.plane_stride;
                if (left & 2) clip_planes<D, 2>(g, P.plane_stride, T, n), g += 2 * P.plane_stride;
                if (left & 1) clip_planes<D, 1>(g, P.plane_stride, T, n);
            }
#pragma unroll
            for (int k = 0; k < 4 * D; k++) best[k] = max(best[k], exp_key((unsigned)byte_of(n[k >> 2], k & 3), qmin[k], (unsigned)e));
        }
        // ---- the choice: the exposure bytes, the map bytes
        unsigned who[D];
        const unsigned e0 = exp_key_exposure(best[0]);
        bool one = true;
#pragma unroll
        for (int j = 0; j < D; j++) {
            who[j] = 0u;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const unsigned e = exp_key_exposure(best[4 * j + k]);
                one = one && e == e0;
                who[j] |= e << (8 * k);
                chosen[j] |= (e | (exp_key_clipped(best[4 * j + k]) > 0u ? 0x80u : 0u)) << (8 * k);
            }
            const int inside = P.W - (4 * D * q + 4 * j);  // pixels of this dword inside the window
            in_window[j] = inside >= 4 ? 0x80808080u : inside <= 0 ? 0u : 0x80808080u >> (8 * (4 - inside));
        }
        // ---- pass 2: the planes in use of dst_view
        uint8_t *dst = const_cast<uint8_t *>(P.frames) + (size_t)dst_view * P.view_stride + px;
        const uint8_t *src = P.frames + (size_t)first_view * P.view_stride + px;
        if (one) {
            const uint8_t *s = src + (size_t)e0 * P.view_stride;
            for (int a = 0; a < X.n_axes; a++) {
                size_t off = (size_t)X.base[a] * P.plane_stride;
                int left = X.count[a];
                for (; left >= 8; left -= 8, off += 8 * P.plane_stride) copy_planes<D, 8>(dst + off, s + off, P.plane_stride);
                if (left & 4) copy_planes<D, 4>(dst + off, s + off, P.plane_stride), off += 4 * P.plane_stride;
                if (left & 2) copy_planes<D, 2>(dst + off, s + off, P.plane_stride), off += 2 * P.plane_stride;
                if (left & 1) copy_planes<D, 1>(dst + off, s + off, P.plane_stride);
            }
        } else {
            for (int a = 0; a < X.n_axes; a++) {
                size_t off = (size_t)X.base[a] * P.plane_stride;
                for (int p = 0; p < X.count[a]; p++, off += P.plane_stride) {
                    Run<D> out;
#pragma unroll
                    for (int j = 0; j < D; j++) out.w[j] = 0u;
                    for (int e = 0; e < E; e++) {
                        unsigned m[D], any = 0u;
#pragma unroll
                        for (int j = 0; j < D; j++) any |= m[j] = exp_bytes_equal(who[j], (unsigned)e);
                        if (any) {
                            const Run<D> w = load_run<D>(src + (size_t)e * P.view_stride + off);
#pragma unroll
                            for (int j = 0; j < D; j++) out.w[j] |= w.w[j] & m[j];
                        }
                    }
                    store_run<D>(dst + off, out);
                }
            }
        }
        Run<D> mrun;
#pragma unroll
        for (int j = 0; j < D; j++) mrun.w[j] = chosen[j];
        store_run<D>(map + px, mrun);
    }
    // ---- counts: window pixels taken from exposure e (e < E), and (e == E) those clipped in the exposure chosen
    for (int e = 0; e <= E; e++) {
        unsigned c = 0u;
#pragma unroll
        for (int j = 0; j < D; j++) c += (unsigned)__popc((e < E ? exp_bytes_equal(chosen[j] & 0x07070707u, (unsigned)e) : chosen[j]) & in_window[j]);
        c = wave_sum(c);
        if ((threadIdx.x & 63) == 0) s_cnt[e][threadIdx.x >> 6] = c;
    }
    __syncthreads();
    if ((int)threadIdx.x <= E) {
        const unsigned c = BLOCK_SUM_TOTAL(s_cnt[threadIdx.x]);
        if (c) atomicAdd(counts + threadIdx.x, c);
    }
}

int launch_fuse_exposures(const KParams &P, const ExposurePlan &X, int first_view, int n_exposures, int dst_view, int saturation, uint8_t *map,
                          unsigned *counts, void *stream)
{
    constexpr int D = 1;
    const unsigned blocks = (unsigned)(((long)((P.W + 4 * D - 1) / (4 * D)) * P.H + 255) / 256);
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_fuse_exposures<D>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, P, X, first_view, n_exposures, dst_view, exp_clip_test(saturation),
                       map, counts);
    return (int)hipGetLastError();
}

}  // namespace sl3d
