// What the convolution families share: the MFMA accumulator fragment and the BatchNorm-statistics records their epilogues write.
//
// Fragment.  acc[..][r] of a v_mfma_f32_16x16x32 result holds row `lane & 15` (fr) and column `4 * (lane >> 4) + r` (4 fq + r) of a 16x16
// tile.  Every epilogue here has output positions on fr and channels on (fq, r), so the 16 positions of a channel are the 16 lanes of one
// DPP row.
//
// Records.  A conv launch writes [rec][2][C] floats for tri_bn_finalize (`stats`, or the `partial` buffer of tri_conv_dgrad_bn): per record
// the C column sums first, the C sums of squares second (conv_c64_kernel's BatchNorm-backward form: sums of g and of g * y).  What a
// record covers - a row tile, a unit of images, a persistent workgroup - is the family's; the consumer adds the records up.
//   * A statistics value is the value AS STORED, i.e. as BatchNorm will read it back: Act<AT>::rnd(v) for 16-bit storage, never the fp32
//     accumulator.
//   * The order of additions is fixed (every one is fp32, and replayed steps are compared byte for byte): a lane adds its own rows as it
//     stores them; the DPP ladder 8, 4, 2, 1 over the 16 lanes of the row (stat_row_sum); the lanes with fr == 0 park the pair in LDS at
//     red[(slot * ncols + col) * 2 + {0, 1}], slot = the wave (stat_stage); after a barrier one thread per channel adds the slots in
//     ascending order, starting from 0.f (stat_wave_sum), and stores the pair (stat_store).
// The writers differ in the column they pass, the slots they sum (all four waves, WAVES_M, the WK partners of a channel column), the barrier
// between staging and summing (__syncthreads(); inside conv_halo2d_kernel's tile loop a raw s_barrier behind lgkmcnt(0) only, which must not
// wait for the LDS-DMA in flight), where `red` lives and which record they write.
//
// A writer uses a piece where that leaves its instructions as they were: integer index arithmetic is not reassociated across the call, and
// the kernels were compared instruction by instruction (profiles/r16/NOTES_conv_helpers.md).  Written out in the kernel, with the same
// layout and order: the staging stores of conv_s2g / conv_voxg / conv_c64 / conv_vox0 (their index is one flat expression), the wave sums
// of conv_s2g / conv_voxg / conv_vox0 and conv_c64 (waves c and c + 2, no 0.f term), the record stores of halo_store_stats, conv_voxg,
// conv_voxb and conv_vox0, the ladder of conv_voxg_kernel, and all of conv_splitk_finish_kernel (16 row groups through LDS, no ladder).
#pragma once
#include "common.h"

// v rotated right by N lanes inside its row of 16 lanes (DPP row_ror)
template <int N>
__device__ __forceinline__ float row_ror(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x120 + N, 0xf, 0xf, false));
}

// (s, q) summed over the 16 lanes of a DPP row = the 16 rows of a fragment; every lane of the row ends up with the total.
// Rotate-and-add on the VALU instead of 8 ds_bpermute round trips per column (measured: statistics were 3,300 of a tile's ~31,000 cycles).
__device__ __forceinline__ void stat_row_sum(float& s, float& q) {
    s += row_ror<8>(s); q += row_ror<8>(q);
    s += row_ror<4>(s); q += row_ror<4>(q);
    s += row_ror<2>(s); q += row_ror<2>(q);
    s += row_ror<1>(s); q += row_ror<1>(q);
}

// red is [wave slots][ncols][2]: the lanes with fr == 0 park their row's reduced pair of column `col`
__device__ __forceinline__ void stat_stage(float* red, int slot, int ncols, int col, int fr, float s, float q) {
    if (fr == 0) {
        red[(slot * ncols + col) * 2 + 0] = s;
        red[(slot * ncols + col) * 2 + 1] = q;
    }
}

// column `col` summed over the wave slots slot0 .. slot0 + NW - 1, in that order
template <int NW>
__device__ __forceinline__ void stat_wave_sum(const float* red, int slot0, int ncols, int col, float& s, float& q) {
    s = 0.f; q = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) { s += red[((slot0 + w) * ncols + col) * 2]; q += red[((slot0 + w) * ncols + col) * 2 + 1]; }
}

// channel c0 + c of record rec of a [..][2][C] buffer (c0: the workgroup's first channel, c: the thread's; two terms, as the writers had them)
__device__ __forceinline__ void stat_store(float* stats, size_t rec, int C, int c0, int c, float s, float q) {
    stats[(rec * 2 + 0) * C + c0 + c] = s;
    stats[(rec * 2 + 1) * C + c0 + c] = q;
}
