// Counter-based dropout (the Dropout(0.1) of the reference's clip_text.py / clip_img.py heads): the mask is a pure function of
// (seed, step, tower, global row, column), so the CPU can restate it bit for bit, a train-mode step can be compared with float64, and
// a data-parallel rank that passes row0 = rank * B_local draws the rows the single-process global batch would draw.
//
//   w(r, c)  = word (c & 3) of Philox4x32-10(key = (seed & 0xffffffff, seed >> 32),
//                                            counter = (c >> 2, (row0 + r) & 0xffffffff, used[0] & 0xffffffff, tower))
//   m(r, c)  = 0 when (w >> 8) < threshold, else `scale`          (threshold = round(p * 2^24): 24 uniform bits against p)
//   y[r][c]  = x[r][c] * m(r, c)                                    one fp32 multiply: inf * 0 = NaN, NaN stays NaN, as in torch
//
// The step is read from DEVICE memory: tri_dropout_tick copies the module's counter to `used` and advances it, one launch ahead of
// the apply on the same stream, so a step captured into a HIP graph draws a new mask on every replay, and the backward (the same
// call on dy, with the `used` its forward saved) meets its own forward's mask whatever ticked in between.
// One thread owns four consecutive columns of a row = one Philox call.  No LDS, no atomics; two runs give the same bits.
#include "common.h"
#include "../../include/tricolo_hip.h"

#define DO_THREADS 256
#define DO_MAX_BLOCKS 4096

__global__ void dropout_tick_kernel(long long* __restrict__ step, long long* __restrict__ used) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const long long s = step[0];
        used[0] = s;
        step[0] = s + 1;
    }
}

extern "C" int tri_dropout_tick(long long* step, long long* used, void* stream) {
    if (!step || !used) { tri_set_error("tri_dropout_tick: null pointer"); return TRI_ERR_ARG; }
    dropout_tick_kernel<<<1, 64, 0, (hipStream_t)stream>>>(step, used);
    return tri_check_launch("tri_dropout_tick");
}

// VEC: cols % 4 == 0 and both pointers 16-byte aligned -> every group of four is one aligned 16-byte access; otherwise dwords, the
// last group of a row cut at `cols`.
template <bool VEC>
__global__ __launch_bounds__(DO_THREADS) void dropout_apply_kernel(const float* __restrict__ x, float* __restrict__ y, long rows, int cols,
                                                                   int groups, uint32_t threshold, float scale, uint32_t k0, uint32_t k1,
                                                                   const long long* __restrict__ used, uint32_t row0, uint32_t tower) {
    const uint32_t step = (uint32_t)(unsigned long long)used[0];
    const long total = rows * groups;
    for (long i = (long)blockIdx.x * DO_THREADS + threadIdx.x; i < total; i += (long)gridDim.x * DO_THREADS) {
        const long r = i / groups;
        const int g = (int)(i - r * groups);
        const Philox4 w = philox4x32_10((uint32_t)g, row0 + (uint32_t)r, step, tower, k0, k1);
        float m[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) m[k] = (w.x[k] >> 8) < threshold ? 0.f : scale;
        const size_t at = (size_t)r * cols + (size_t)g * 4;
        if (VEC) {
            const float4 v = *(const float4*)(x + at);
            *(float4*)(y + at) = make_float4(v.x * m[0], v.y * m[1], v.z * m[2], v.w * m[3]);
        } else {
            const int n = min(4, cols - g * 4);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < n) y[at + k] = x[at + k] * m[k];
        }
    }
}

extern "C" int tri_dropout_apply(const float* x, float* y, long rows, int cols, unsigned threshold, float scale, unsigned long long seed,
                                 const long long* used, unsigned long long row0, unsigned tower, void* stream) {
    if (threshold > (1u << 24)) { tri_set_error("tri_dropout_apply: threshold above 2^24"); return TRI_ERR_ARG; }
    if (cols < 1 || rows < 0) { tri_set_error("tri_dropout_apply: cols >= 1 and rows >= 0"); return TRI_ERR_ARG; }
    if (rows == 0) return TRI_OK;
    if (!x || !y || !used) { tri_set_error("tri_dropout_apply: null pointer"); return TRI_ERR_ARG; }
    const int groups = (cols + 3) / 4;
    if (rows > (((long)1 << 62) / groups)) { tri_set_error("tri_dropout_apply: rows * cols overflows"); return TRI_ERR_ARG; }
    const long total = rows * groups;
    const unsigned blocks = (unsigned)min((total + DO_THREADS - 1) / DO_THREADS, (long)DO_MAX_BLOCKS);
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    const bool vec = cols % 4 == 0 && (((uintptr_t)x | (uintptr_t)y) & 15) == 0;
    if (vec)
        dropout_apply_kernel<true><<<blocks, DO_THREADS, 0, (hipStream_t)stream>>>(x, y, rows, cols, groups, threshold, scale, k0, k1, used,
                                                                                   (uint32_t)row0, tower);
    else
        dropout_apply_kernel<false><<<blocks, DO_THREADS, 0, (hipStream_t)stream>>>(x, y, rows, cols, groups, threshold, scale, k0, k1, used,
                                                                                    (uint32_t)row0, tower);
    return tri_check_launch("tri_dropout_apply");
}
