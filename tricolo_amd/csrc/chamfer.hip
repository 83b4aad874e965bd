// Shape F1 / chamfer on point clouds (the reference's calculate_f1.py): batched one-sided nearest neighbour, then counts
// below the distance thresholds, the chamfer sums and precision / recall / F1 - all on the device.
//
//   d2[n][i]  = min over valid j of (P[n][i].x - Q[n][j].x)^2 + (.y)^2 + (.z)^2        fp32, from the DIFFERENCES like pytorch3d's
//               knn_points (the expanded |a|^2 + |b|^2 - 2ab form loses four digits at |a|^2 ~ 75 against d^2 = 0.01)
//   idx[n][i] = the lowest j that attains it (-1 when Q[n] is empty)
// A VALU kernel: each thread keeps R points of P in registers, Q streams through LDS in tiles of NN_TQ padded float4 points
// that every lane reads at the same address (one broadcast ds_read_b128 per point of Q), the running minimum stays in
// registers: 3 sub, 1 mul, 2 fma, 1 min per point pair.  No floating-point atomics; every reduction has a fixed order.
#include "common.h"
#include "../../include/tricolo_hip.h"

#define NN_THREADS 256
#define NN_TQ 2048                     // points of Q per LDS tile (32 KiB: five workgroups per CU)
#define NN_MAX_BLOCKS (1 << 23)        // per launch: grid x block must stay below 2^32 threads

template <int R, bool IDX>
__global__ __launch_bounds__(NN_THREADS) void nn_dist2_kernel(const float* __restrict__ P, const float* __restrict__ Q,
                                                              const long* __restrict__ len_p, const long* __restrict__ len_q, int S1,
                                                              int S2, long p_stride, long q_stride, int tiles, long n0,
                                                              float* __restrict__ d2, long* __restrict__ idx) {
    __shared__ float4 sq[NN_TQ];
    const int t = threadIdx.x;
    const long n = n0 + blockIdx.x / (unsigned)tiles;
    const int base = (int)(blockIdx.x % (unsigned)tiles) * (R * NN_THREADS);
    const int lp = len_p ? (int)min(max(len_p[n], 0L), (long)S1) : S1;
    const int lq = len_q ? (int)min(max(len_q[n], 0L), (long)S2) : S2;
    const float* p = P + n * p_stride;
    const float* q = Q + n * q_stride;
    float px[R], py[R], pz[R], best[R];
    int bi[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int i = base + r * NN_THREADS + t;
        const bool ok = i < lp;                                        // rows at and beyond the length are never read
        px[r] = ok ? p[(size_t)i * 3 + 0] : 0.f;
        py[r] = ok ? p[(size_t)i * 3 + 1] : 0.f;
        pz[r] = ok ? p[(size_t)i * 3 + 2] : 0.f;
        best[r] = INFINITY;
        bi[r] = -1;
    }
    const int lq_run = base < lp ? lq : 0;                             // a tile of padding rows only: nothing to search
    for (int q0 = 0; q0 < lq_run; q0 += NN_TQ) {
        const int cnt = min(NN_TQ, lq_run - q0);
        const int cnt8 = (cnt + 7) & ~7;                               // the tail is filled with +inf points: d = inf never wins
        __syncthreads();
        for (int j = t; j < cnt8; j += NN_THREADS) {
            float4 v = make_float4(INFINITY, INFINITY, INFINITY, 0.f);
            if (j < cnt) {
                const float* s = q + (size_t)(q0 + j) * 3;
                v = make_float4(s[0], s[1], s[2], 0.f);
            }
            sq[j] = v;
        }
        __syncthreads();
#pragma unroll 8
        for (int j = 0; j < cnt8; ++j) {
            f32x4 v = *(const f32x4*)&sq[j];
            asm volatile("" : "+v"(v));                                // keep the read one ds_read_b128 (4 LDS cycles), not a b96 (8)
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const float dx = px[r] - v[0], dy = py[r] - v[1], dz = pz[r] - v[2];
                const float d = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
                if (IDX) {
                    if (d < best[r]) { best[r] = d; bi[r] = q0 + j; }
                } else {
                    best[r] = fminf(best[r], d);
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int i = base + r * NN_THREADS + t;
        if (i < S1) {
            const bool ok = i < lp;
            d2[(size_t)n * S1 + i] = ok ? best[r] : 0.f;
            if (IDX) idx[(size_t)n * S1 + i] = ok ? (long)bi[r] : -1L;
        }
    }
}

template <int R>
static int nn_launch(const float* P, const float* Q, const long* len_p, const long* len_q, long N, int S1, int S2, long p_stride,
                     long q_stride, float* d2, long* idx, hipStream_t st) {
    const int tiles = (S1 + R * NN_THREADS - 1) / (R * NN_THREADS);
    const long per_launch = max(1L, (long)NN_MAX_BLOCKS / tiles);
    for (long n0 = 0; n0 < N; n0 += per_launch) {
        const unsigned blocks = (unsigned)(min(per_launch, N - n0) * tiles);
        if (idx)
            nn_dist2_kernel<R, true><<<blocks, NN_THREADS, 0, st>>>(P, Q, len_p, len_q, S1, S2, p_stride, q_stride, tiles, n0, d2, idx);
        else
            nn_dist2_kernel<R, false><<<blocks, NN_THREADS, 0, st>>>(P, Q, len_p, len_q, S1, S2, p_stride, q_stride, tiles, n0, d2, idx);
    }
    return tri_check_launch("tri_nn_dist2");
}

extern "C" int tri_nn_dist2(const float* P, const float* Q, const long* len_p, const long* len_q, int N, int S1, int S2, int p_shared,
                            int q_shared, float* d2, long* idx, void* stream) {
    if (N < 0 || S1 < 0 || S2 < 0) { tri_set_error("tri_nn_dist2: negative size"); return TRI_ERR_ARG; }
    if (S1 > (1 << 28) || S2 > (1 << 28)) { tri_set_error("tri_nn_dist2: more than 2^28 points in a cloud"); return TRI_ERR_UNSUPPORTED; }
    if (N == 0 || S1 == 0) return TRI_OK;
    const long ps = p_shared ? 0 : (long)S1 * 3, qs = q_shared ? 0 : (long)S2 * 3;
    // Four points per thread quarter the LDS reads per pair; below two such workgroups per CU (256 CUs) one point per thread
    // spreads a small batch over four times as many workgroups instead.
    const long big_tiles = (long)N * ((S1 + 4 * NN_THREADS - 1) / (4 * NN_THREADS));
    if (big_tiles >= 512) return nn_launch<4>(P, Q, len_p, len_q, N, S1, S2, ps, qs, d2, idx, (hipStream_t)stream);
    return nn_launch<1>(P, Q, len_p, len_q, N, S1, S2, ps, qs, d2, idx, (hipStream_t)stream);
}

// ---- counts below the thresholds and the chamfer sum: one workgroup per cloud, fixed order ---------------------------------
struct F1Thresholds {
    float t[TRI_F1_MAX_THRESHOLDS];
};

__global__ __launch_bounds__(256) void f1_counts_kernel(const float* __restrict__ d2, const long* __restrict__ lengths, int N, int S,
                                                        F1Thresholds thr, int T, int* __restrict__ counts, float* __restrict__ sums) {
    __shared__ int wc[4][TRI_F1_MAX_THRESHOLDS];
    __shared__ float wsum[4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    for (int n = blockIdx.x; n < N; n += gridDim.x) {
        const int len = lengths ? (int)min(max(lengths[n], 0L), (long)S) : S;
        const float* row = d2 + (size_t)n * S;
        int c[TRI_F1_MAX_THRESHOLDS];
#pragma unroll
        for (int k = 0; k < TRI_F1_MAX_THRESHOLDS; ++k) c[k] = 0;
        float s = 0.f;
        for (int i = t; i < len; i += 256) {
            const float v = row[i];
            s += v;
            const float d = __fsqrt_rn(v);
#pragma unroll
            for (int k = 0; k < TRI_F1_MAX_THRESHOLDS; ++k) c[k] += (k < T && d < thr.t[k]) ? 1 : 0;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            s += __shfl_xor(s, o);
#pragma unroll
            for (int k = 0; k < TRI_F1_MAX_THRESHOLDS; ++k) c[k] += __shfl_xor(c[k], o);
        }
        if (lane == 0) {
            wsum[wave] = s;
#pragma unroll
            for (int k = 0; k < TRI_F1_MAX_THRESHOLDS; ++k) wc[wave][k] = c[k];
        }
        __syncthreads();
        if (t < T) counts[(size_t)n * T + t] = wc[0][t] + wc[1][t] + wc[2][t] + wc[3][t];
        if (t == 0) sums[n] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
        __syncthreads();
    }
}

extern "C" int tri_f1_counts(const float* d2, const long* lengths, int N, int S, const float* thresholds, int T, int* counts, float* sums,
                             void* stream) {
    if (N < 0 || S < 0 || T < 0 || T > TRI_F1_MAX_THRESHOLDS) { tri_set_error("tri_f1_counts: need N, S >= 0 and 0 <= T <= 8"); return TRI_ERR_ARG; }
    if (N == 0) return TRI_OK;
    F1Thresholds thr;
    for (int k = 0; k < TRI_F1_MAX_THRESHOLDS; ++k) thr.t[k] = k < T ? thresholds[k] : 0.f;
    f1_counts_kernel<<<min(N, 1 << 20), 256, 0, (hipStream_t)stream>>>(d2, lengths, N, S, thr, T, counts, sums);
    return tri_check_launch("tri_f1_counts");
}

// ---- precision / recall / F1 / chamfer in the reference's order of operations -------------------------------------------------
// precision = 100 * (count_p / len_p) is `100.0 * (dists < t).float().mean(dim=1)`: the mean divides first.  Every operation is
// rounded on its own as torch does: contraction is off in this kernel (precision + recall would otherwise become
// fma(100, count / len, recall), one rounding less and an F1 one ulp off), and the divisions are the correctly rounded ones.
__global__ __launch_bounds__(256) void f1_finalize_kernel(const int* __restrict__ count_p, const int* __restrict__ count_q,
                                                          const float* __restrict__ sum_p, const float* __restrict__ sum_q,
                                                          const long* __restrict__ len_p, const long* __restrict__ len_q, int S1, int S2,
                                                          long N, int T, float eps, float* __restrict__ precision,
                                                          float* __restrict__ recall, float* __restrict__ f1, float* __restrict__ chamfer) {
#pragma clang fp contract(off)
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < N * T; e += (long)gridDim.x * 256) {
    const long n = e / T;
    const int k = (int)(e % T);
    const float lp = (float)(len_p ? min(max(len_p[n], 0L), (long)S1) : (long)S1);
    const float lq = (float)(len_q ? min(max(len_q[n], 0L), (long)S2) : (long)S2);
    const float pr = 100.0f * __fdiv_rn((float)count_p[e], lp);
    const float rc = 100.0f * __fdiv_rn((float)count_q[e], lq);
    precision[(size_t)k * N + n] = pr;
    recall[(size_t)k * N + n] = rc;
    f1[(size_t)k * N + n] = __fdiv_rn((2.0f * pr) * rc, (pr + rc) + eps);
    if (k == 0 && chamfer) chamfer[n] = __fdiv_rn(sum_p[n], lp) + __fdiv_rn(sum_q[n], lq);
    }
}

extern "C" int tri_f1_finalize(const int* count_p, const int* count_q, const float* sum_p, const float* sum_q, const long* len_p,
                               const long* len_q, int N, int S1, int S2, int T, float eps, float* precision, float* recall, float* f1,
                               float* chamfer, void* stream) {
    if (N < 0 || T < 1 || T > TRI_F1_MAX_THRESHOLDS) { tri_set_error("tri_f1_finalize: need N >= 0 and 1 <= T <= 8"); return TRI_ERR_ARG; }
    if (N == 0) return TRI_OK;
    const long total = (long)N * T;
    f1_finalize_kernel<<<(unsigned)min((total + 255) / 256, 1L << 20), 256, 0, (hipStream_t)stream>>>(count_p, count_q, sum_p, sum_q, len_p, len_q, S1, S2,
                                                                                         N, T, eps, precision, recall, f1, chamfer);
    return tri_check_launch("tri_f1_finalize");
}
