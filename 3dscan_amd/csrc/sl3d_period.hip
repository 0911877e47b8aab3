// sl3d_period.hip -- gfx950 (MI355X, wave64) kernels of sl3d_repair_periods: whole 2*Pi periods taken out of the absolute phase
// of one axis of one view, against the lower median of the samples along the coded direction.  The arithmetic of a pixel: sl3d_period.h.
// Two launches, because every pixel decides from the planes as they were when the call was enqueued (a Jacobi pass):
//   k_period_jumps<AXIS, R>  reads the absolute phase and the valid bytes, writes j of every pixel into a byte plane (0: left alone) and
//                            adds the repaired / unrepairable pixels to two words -- integer atomics, one pair per block
//   k_period_apply           pointwise: where j != 0, code -= j and the absolute phase is recomputed by stage 4's expression
// The radius is a template argument: the window of 2R + 1 values lives in registers, the median is a selection by counting over it
// (period_median), every index is a compile-time constant; no instantiation uses scratch.  Measured: DESIGN 4m.
// Compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sl3d_block.h"
#include "sl3d_internal.h"
#include "sl3d_period.h"

namespace sl3d {

// the planes of one axis of one view (row-major, `pitch` elements per row) and what the call writes
struct PeriodArgs {
    const float *unwrapped;
    const uint8_t *valid;
    const int *code;
    int8_t *jump;      // [H][pitch]
    int *wide;         // [H][pitch] j where jump == SL3D_PERIOD_WIDE; NULL for N < 8 (no such j exists)
    unsigned *counts;  // repaired, unrepairable
    int W, H, pitch, n_gray;
};

// What pixel (col, row) brings into a window: its absolute phase if it is a sample, +infinity otherwise (also outside the window).  In two
// halves, so that a lane can have the requests of ALL the pixels it stages in flight together: period_request issues both loads without
// a branch -- a pixel that cannot be a sample reads element 0 of the planes instead, and the phase does not wait for the valid byte --
// and period_staged turns the pair into the staged value.  Why: `valid == 1 ? phase : inf` written per pixel compiles to the phase loaded
// behind the byte, one pair after the other -- ~20 dependent loads per lane.
struct PeriodRequest {
    float u;
    unsigned ok;
};
template <int AXIS>
__device__ __forceinline__ PeriodRequest period_request(const PeriodArgs &a, int col, int row)
{
    const bool in_range = AXIS == 0 ? (col >= 1 && col <= a.W - 2 && row < a.H) : (row >= 1 && row <= a.H - 2 && col < a.W);
    const size_t px = in_range ? (size_t)row * a.pitch + col : 0;
    PeriodRequest q;
    q.u = a.unwrapped[px];
    q.ok = (unsigned)a.valid[px] | (in_range ? 0u : 2u);  // (1 iff in range and valid)
    return q;
}
__device__ __forceinline__ float period_staged(const PeriodRequest &q) { return q.ok == 1u ? q.u : period_no_sample(); }

// A pixel's decision in two halves, so that a lane that owns several pixels reads their codes together: period_pixel_jump gives j from the
// window v (v[R] = the pixel itself; 0: left alone), period_code requests the code of a pixel with j != 0 without a branch (the others
// read element 0), period_pixel_byte gives the byte of the jump plane; c gets the pixel's repaired (bit 0) or unrepairable (bit 16) count
template <int R>
__device__ __forceinline__ long period_pixel_jump(const float (&v)[2 * R + 1])
{
    if (!(v[R] < period_no_sample())) return 0;  // no sample
    int n;
    const float m = period_median<2 * R + 1>(v, &n);
    return period_sample_jump(v[R], m, n, R);
}
__device__ __forceinline__ int period_code(const PeriodArgs &a, long j, size_t px) { return a.code[j != 0 ? px : 0]; }
__device__ __forceinline__ int period_pixel_byte(const PeriodArgs &a, long j, int code, size_t px, unsigned &c)
{
    if (j == 0) return 0;
    const int b = period_byte(j);
    // (N < 8 has no j beyond a byte and no wide plane; the second test keeps a null plane from ever being written)
    if (!period_in_range((long)code - j, a.n_gray) || (b == SL3D_PERIOD_WIDE && !a.wide)) {
        c += 1u << 16;
        return 0;
    }
    if (b == SL3D_PERIOD_WIDE) a.wide[px] = (int)j;
    c += 1u;
    return b;
}

constexpr int PERIOD_ROWS = 8;   // AXIS 0: rows of a block's tile, 256 columns wide
constexpr int PERIOD_BAND = 32;  // AXIS 1: rows of a block's tile (8 consecutive rows per wave), 64 columns wide

// AXIS 0 (the vertical axis: windows along a row).  Block (x, y) owns a run of 256 pixels of each of PERIOD_ROWS rows: their phases and R
//   halo pixels each side are staged in LDS (a non-sample as +infinity: the valid byte needs no LDS of its own), a lane takes one pixel of
//   every row and reads its 2R + 1 consecutive words -- lanes read consecutive addresses, no bank conflict.  Eight rows, not one,
//   because every block ends in a pair of atomic adds on the same two words: with a row per block (8,640 blocks at 1080p) the adds alone
//   take 115 us per call, whatever the radius.
// AXIS 1 (windows along a column).  Block (x, y) owns 64 columns x PERIOD_BAND rows plus R halo rows above and below; a wave loads whole
//   rows of the tile (256 contiguous bytes per plane) and owns 8 consecutive rows, a lane one column: it reads its 8 + 2R words down the
//   column once -- 64 lanes, 64 consecutive words of one LDS row, no bank conflict -- and slides the window over them in registers.
template <int AXIS, int R>
__global__ __launch_bounds__(256) void k_period_jumps(const PeriodArgs a)
{
    __shared__ unsigned s_cnt[4];
    unsigned c = 0u;
    if constexpr (AXIS == 0) {
        constexpr int RUN = 256 + 2 * R;
        __shared__ float s_u[PERIOD_ROWS][RUN];
        const int r0 = (int)blockIdx.y * PERIOD_ROWS, c0 = (int)blockIdx.x * 256;
        constexpr int LOADS = (PERIOD_ROWS * RUN + 255) / 256;
        PeriodRequest q[LOADS];
#pragma unroll
        for (int k = 0; k < LOADS; k++) {
            const int i = min((int)threadIdx.x + 256 * k, PERIOD_ROWS * RUN - 1);  // (the last round's spare lanes repeat the last pixel)
            q[k] = period_request<0>(a, c0 - R + i % RUN, r0 + i / RUN);
        }
#pragma unroll
        for (int k = 0; k < LOADS; k++) {
            const int i = min((int)threadIdx.x + 256 * k, PERIOD_ROWS * RUN - 1);
            s_u[i / RUN][i % RUN] = period_staged(q[k]);
        }
        __syncthreads();
        const int col = c0 + (int)threadIdx.x;
        long j[PERIOD_ROWS];
        int code[PERIOD_ROWS];
#pragma unroll
        for (int k = 0; k < PERIOD_ROWS; k++) {
            float v[2 * R + 1];
#pragma unroll
            for (int d = 0; d < 2 * R + 1; d++) v[d] = s_u[k][threadIdx.x + d];
            j[k] = period_pixel_jump<R>(v);  // (0 beyond the window: nothing but infinities was staged there)
        }
#pragma unroll
        for (int k = 0; k < PERIOD_ROWS; k++) code[k] = period_code(a, j[k], (size_t)(r0 + k) * a.pitch + col);
#pragma unroll
        for (int k = 0; k < PERIOD_ROWS; k++) {
            const size_t px = (size_t)(r0 + k) * a.pitch + col;
            if (r0 + k < a.H && col < a.pitch) a.jump[px] = (int8_t)period_pixel_byte(a, j[k], code[k], px, c);
        }
    } else {
        constexpr int ROWS = PERIOD_BAND / 4;
        __shared__ float s_u[PERIOD_BAND + 2 * R][64];
        const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
        const int col = (int)blockIdx.x * 64 + lane, r0 = (int)blockIdx.y * PERIOD_BAND;
        constexpr int LOADS = (PERIOD_BAND + 2 * R + 3) / 4;
        PeriodRequest q[LOADS];
#pragma unroll
        for (int k = 0; k < LOADS; k++) q[k] = period_request<1>(a, col, r0 - R + min(wave + 4 * k, PERIOD_BAND + 2 * R - 1));  // (as above)
#pragma unroll
        for (int k = 0; k < LOADS; k++) s_u[min(wave + 4 * k, PERIOD_BAND + 2 * R - 1)][lane] = period_staged(q[k]);
        __syncthreads();
        float w[ROWS + 2 * R];
#pragma unroll
        for (int i = 0; i < ROWS + 2 * R; i++) w[i] = s_u[wave * ROWS + i][lane];
        long j[ROWS];
        int code[ROWS];
#pragma unroll
        for (int k = 0; k < ROWS; k++) {
            float v[2 * R + 1];
#pragma unroll
            for (int d = 0; d < 2 * R + 1; d++) v[d] = w[k + d];
            j[k] = period_pixel_jump<R>(v);
        }
#pragma unroll
        for (int k = 0; k < ROWS; k++) code[k] = period_code(a, j[k], (size_t)(r0 + wave * ROWS + k) * a.pitch + col);
#pragma unroll
        for (int k = 0; k < ROWS; k++) {
            const int row = r0 + wave * ROWS + k;
            const size_t px = (size_t)row * a.pitch + col;
            if (row < a.H && col < a.pitch) a.jump[px] = (int8_t)period_pixel_byte(a, j[k], code[k], px, c);
        }
    }
    BLOCK_SUM(c, s_cnt);
    if (threadIdx.x == 0) {
        const unsigned tot = BLOCK_SUM_TOTAL(s_cnt);  // (at most 2048 pixels of either kind per block: the halves cannot carry)
        if (tot & 0xffffu) atomicAdd(&a.counts[0], tot & 0xffffu);
        if (tot >> 16) atomicAdd(&a.counts[1], tot >> 16);
    }
}

// a lane takes the 4 pixels of one dword of the jump plane (pitch is a multiple of 16: a dword never straddles two rows)
__global__ __launch_bounds__(256) void k_period_apply(const int8_t *__restrict__ jump, const int *__restrict__ wide, const float *__restrict__ wrapped,
                                                      int *__restrict__ code, float *__restrict__ unwrapped, size_t n_quads)
{
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= n_quads) return;
    const unsigned word = *(const unsigned *)(jump + 4 * q);
    if (!word) return;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int b = (int)(int8_t)(word >> (8 * k));
        if (!b) continue;
        const size_t px = 4 * q + k;
        const long kk = (long)code[px] - (b == SL3D_PERIOD_WIDE ? (long)wide[px] : (long)b);
        code[px] = (int)kk;
        unwrapped[px] = period_value(wrapped[px], kk);
    }
}

template <int AXIS, int R>
static void period_jumps(dim3 grid, hipStream_t st, const PeriodArgs &a)
{
    hipLaunchKernelGGL((k_period_jumps<AXIS, R>), grid, dim3(256), 0, st, a);
}

template <int AXIS>
static bool period_jumps_radius(int radius, dim3 grid, hipStream_t st, const PeriodArgs &a)
{
    switch (radius) {
    case 1: period_jumps<AXIS, 1>(grid, st, a); return true;
    case 2: period_jumps<AXIS, 2>(grid, st, a); return true;
    case 3: period_jumps<AXIS, 3>(grid, st, a); return true;
    case 4: period_jumps<AXIS, 4>(grid, st, a); return true;
    case 5: period_jumps<AXIS, 5>(grid, st, a); return true;
    case 6: period_jumps<AXIS, 6>(grid, st, a); return true;
    case 7: period_jumps<AXIS, 7>(grid, st, a); return true;
    case 8: period_jumps<AXIS, 8>(grid, st, a); return true;
    }
    return false;  // (a missing kernel is an error, never another path)
}

int launch_period_repair(const KParams &P, int view, int axis, int radius, const PeriodPlanes &b, void *stream)
{
    (void)hipGetLastError();
    const size_t v0 = (size_t)view * P.px_view_stride;
    const PeriodArgs a = {P.unwrapped[axis] + v0, P.valid_axis[axis] + v0, P.code[axis] + v0, b.jump, b.wide, b.counts, P.W, P.H, P.pitch, axis == 0 ? P.Nv : P.Nh};
    const dim3 grid = axis == 0 ? dim3((unsigned)((P.pitch + 255) / 256), (unsigned)((P.H + PERIOD_ROWS - 1) / PERIOD_ROWS)) : dim3((unsigned)((P.pitch + 63) / 64), (unsigned)((P.H + PERIOD_BAND - 1) / PERIOD_BAND));
    if (!(axis == 0 ? period_jumps_radius<0>(radius, grid, (hipStream_t)stream, a) : period_jumps_radius<1>(radius, grid, (hipStream_t)stream, a)))
        return (int)hipErrorInvalidValue;
    int e = (int)hipGetLastError();
    if (e) return e;
    const size_t n_quads = P.px_view_stride / 4;
    hipLaunchKernelGGL(k_period_apply, dim3((unsigned)((n_quads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, b.jump, b.wide, P.wrapped[axis] + v0,
                       P.code[axis] + v0, P.unwrapped[axis] + v0, n_quads);
    return (int)hipGetLastError();
}

}  // namespace sl3d
