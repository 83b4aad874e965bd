// Text -> shape retrieval against a gallery of any size: a tile of queries per workgroup, running top-k lists, no per-query storage in Ns.
//
// Same ranking as retrieval.hip (its head states the semantics): float64 similarities, larger first, equal similarities with the HIGHER
// shape index first, first_hit[q] = number of shapes that rank before shape label[q].  What differs is the plan:
//   * a workgroup owns QT queries, held as float64 in LDS ([QT][D]; QT = 8 / 4 / 2 / 1 for D <= 512 / 1024 / 2048 / 4096, so the tile is
//     at most 32 KiB), and every shape row a wave loads is multiplied against all QT of them;
//   * wave w streams the shape rows in blocks of GALLERY_ROWS (w * GALLERY_ROWS + r, then every 4 * GALLERY_ROWS further on), lane l
//     reading d = l, l + 64, ... of a row: one coalesced 256-byte load per 64 columns;
//   * a similarity is the value retrieval_topk_kernel forms for the pair: lane l accumulates fma((double)t[d], (double)s[d], acc) over
//     d = l, l + 64, ... ascending, then the 32, 16, ..., 1 butterfly of wave_sum_d - so the two entry points agree bit for bit (the
//     GALLERY_ROWS * QT accumulators of a trip go through the butterfly together, gallery_reduce: the same additions, fewer shuffles);
//   * each wave keeps, per query, a sorted list of its k best (similarity, index) pairs in LDS - and the last entry of a full list in
//     registers, so a row that does not make the list costs one comparison - and, with labels, counts the rows that rank before the
//     query's own shape, whose similarity is computed before the stream starts;
//   * at the end one pass ranks the at most 4 k list entries of a query against each other (one entry per thread, k <= 64) and writes
//     the k first; the four counters are summed.
// The order on (similarity, index) is strict and total, so the result does not depend on which wave saw which row.
// tri_retrieval_classes (shape -> text: several candidates are correct for a query) is the same kernel, CLS = true: the "own shape" is the
// row of the query's class that ranks first, found by a pass over the class's rows before the stream starts - one row at a time, by the
// same lanes in the same order, so its similarity has the stream's bits -, and first_hit counts the rows ranking before it.
// LDS: QT * D * 8 (queries) + 4 * QT * k * 12 (lists) + QT * 28 + 16 bytes <= 57,584: below 64 KiB, no attribute to raise.
#include "common.h"
#include "../../include/tricolo_hip.h"
#include <stdio.h>

#define GALLERY_ROWS 2                                  // shape rows a wave holds accumulators for at a time
#define GALLERY_MAX_D 4096

// retrieval.hip's order, restated (that file stays as it is): larger sim first, equal sims -> larger index first
__device__ __forceinline__ bool gallery_ranks_before(double sa, int ia, double sb, int ib) { return sa > sb || (sa == sb && ia > ib); }

// The 32, 16, ..., 1 butterfly of wave_sum_d for N = 2^m accumulators at once.  While more than one is left, a step pairs accumulators
// (i, i + half): the lanes with bit `o` clear keep i and hand their value of i + half to the partner lane, the others the reverse, so each
// lane adds its own value and its partner's of ONE accumulator - the very addition wave_sum_d makes for it - and half as many values
// are left.  After m steps every lane holds one accumulator (gallery_lane_of), and the remaining steps are wave_sum_d's own.  N + 4
// shuffles for 16 accumulators instead of 96, the same bits.
template <int N>
__device__ __forceinline__ void gallery_reduce(double (&v)[N], int lane) {
    int left = N;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        if (left > 1) {
            const int half = left >> 1;
            const bool up = (lane & o) != 0;
#pragma unroll
            for (int i = 0; i < N / 2; ++i) {
                if (i < half) {
                    const double keep = up ? v[i + half] : v[i], send = up ? v[i] : v[i + half];
                    v[i] = keep + __shfl_xor(send, o);
                }
            }
            left = half;
        } else {
            v[0] += __shfl_xor(v[0], o);
        }
    }
}
// the lowest lane that holds accumulator a after gallery_reduce<N>: step j (o = 32 >> j) chose by bit m - 1 - j of a
template <int N>
__device__ __forceinline__ constexpr int gallery_lane_of(int a) {
    int lane = 0, o = 32;
    for (int half = N >> 1; half > 0; half >>= 1, o >>= 1)
        if (a & half) lane |= o;
    return lane;
}
__device__ __forceinline__ double gallery_readlane(double x, int src) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), src), __builtin_amdgcn_readlane(__double2loint(x), src));
}
// a value every lane holds, told to the compiler (scalar registers: the per-query state must not cost vector registers)
__device__ __forceinline__ double gallery_uniform(double x) {
    return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(x)), __builtin_amdgcn_readfirstlane(__double2loint(x)));
}

// CLS: label[q] names a CLASS of shape rows (class_rows[class_off[g] .. class_off[g + 1]), tri_retrieval_classes) instead of one row; the
// "own shape" of a query is then the row of its class that ranks first, found by a pass over the class before the stream starts
template <int QT, bool CLS>
__global__ __launch_bounds__(256) void retrieval_gallery_kernel(const float* __restrict__ text, const float* __restrict__ shape,
                                                                const int* __restrict__ label, const int* __restrict__ class_off,
                                                                const int* __restrict__ class_rows, int ncls, int Nq, int Ns, int D, int k,
                                                                int* __restrict__ topk_idx, double* __restrict__ topk_sim,
                                                                int* __restrict__ first_hit) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* tq = (double*)smem;                                    // [QT][D] the query tile in float64
    volatile double* lsim = tq + (size_t)QT * D;                   // [4][QT][k] per-wave lists, best first
    volatile double* osim = lsim + 4 * QT * k;                     // [QT] similarity of the query's own shape
    volatile int* lidx = (volatile int*)(osim + QT);               // [4][QT][k]
    volatile int* oidx = lidx + 4 * QT * k;                        // [QT] label, -1: none (no labels, or a query past Nq)
    volatile int* wcnt = oidx + QT;                                // [4][QT] rows ranking before the own shape, per wave
    volatile int* wn = wcnt + 4 * QT;                              // [4] entries in each wave's lists
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int q0 = blockIdx.x * QT;
    for (int i = t; i < QT * D; i += 256) {
        const int q = q0 + i / D;
        tq[i] = q < Nq ? (double)text[(size_t)q0 * D + i] : 0.0;
    }
    __syncthreads();
    // the own shape's similarity, by the same lanes in the same order as every other pair
    for (int q = wave; q < QT; q += 4) {
        int c = -1;
        double acc = 0.0;
        if constexpr (CLS) {
            // the best row of the query's class: one row at a time (a class may hold any number of rows), everything wave-uniform
            int lo = 0, hi = 0;
            if (label && q0 + q < Nq) {
                const int g = label[q0 + q];
                if (g >= 0 && g < ncls) {                          // no such class: first_hit reports -1, nothing is read
                    lo = max(class_off[g], 0);
                    hi = min(class_off[g + 1], Ns);                // class_rows holds at most Ns entries
                }
            }
            const double* tr = tq + (size_t)q * D;
            for (int j = lo; j < hi; ++j) {
                const int r = __builtin_amdgcn_readfirstlane(class_rows[j]);
                if (r < 0 || r >= Ns) continue;                    // no such row: skipped, never dereferenced
                const float* row = shape + (size_t)r * D;
                double a = 0.0;
                for (int d = lane; d < D; d += 64) a = fma(tr[d], (double)row[d], a);
                a = gallery_uniform(wave_sum_d(a));
                if (c < 0 || gallery_ranks_before(a, r, acc, c)) { acc = a; c = r; }
            }
        } else {
            if (label && q0 + q < Nq) {
                c = label[q0 + q];
                if (c < 0 || c >= Ns) c = -1;                      // no such shape: first_hit reports -1, nothing is read
            }
            if (c >= 0) {
                const float* row = shape + (size_t)c * D;
                const double* tr = tq + (size_t)q * D;
                for (int d = lane; d < D; d += 64) acc = fma(tr[d], (double)row[d], acc);
                acc = wave_sum_d(acc);
            }
        }
        if (lane == 0) { osim[q] = acc; oidx[q] = c; }
    }
    __syncthreads();
    int n = 0;                                                     // entries in this wave's lists: the same for every query
    // lane q < QT keeps query q's state: its own shape, the rows counted before it, and the last entry of its list once that is full
    // (thr: what a row has to beat to enter), so a row is tested against all QT queries at once and one that enters no list costs no more
    const int ql = lane < QT ? lane : 0;
    const int own_c = lane < QT ? oidx[ql] : -1;
    const double own_s = osim[ql];
    int cnt = 0, thr_i = -1;
    double thr_s = 0.0;
    int src[GALLERY_ROWS];                                         // the lane that holds (row r, query `lane`) after gallery_reduce
#pragma unroll
    for (int r = 0; r < GALLERY_ROWS; ++r) src[r] = gallery_lane_of<GALLERY_ROWS * QT>(r * QT + ql);
    volatile double* ls = lsim + (size_t)wave * QT * k;
    volatile int* li = lidx + (size_t)wave * QT * k;
    const int nfull = D >> 6;                                      // trips of the dot product in which every lane has a column
    for (int base = wave * GALLERY_ROWS; base < Ns; base += 4 * GALLERY_ROWS) {
        double acc[GALLERY_ROWS * QT];
        const float* row[GALLERY_ROWS];
#pragma unroll
        for (int r = 0; r < GALLERY_ROWS; ++r) row[r] = shape + (size_t)min(base + r, Ns - 1) * D + lane;   // past the end: the last row, not ranked
#pragma unroll
        for (int a = 0; a < GALLERY_ROWS * QT; ++a) acc[a] = 0.0;
        const double* tl = tq + lane;
#pragma unroll 4
        for (int i = 0; i < nfull; ++i) {
            double s[GALLERY_ROWS];
#pragma unroll
            for (int r = 0; r < GALLERY_ROWS; ++r) s[r] = (double)row[r][i * 64];
#pragma unroll
            for (int q = 0; q < QT; ++q) {
                const double tv = tl[(size_t)q * D + i * 64];
#pragma unroll
                for (int r = 0; r < GALLERY_ROWS; ++r) acc[r * QT + q] = fma(tv, s[r], acc[r * QT + q]);
            }
        }
        if (nfull * 64 + lane < D) {                               // D % 64 columns left: the low lanes take one more
#pragma unroll
            for (int q = 0; q < QT; ++q) {
                const double tv = tl[(size_t)q * D + nfull * 64];
#pragma unroll
                for (int r = 0; r < GALLERY_ROWS; ++r) acc[r * QT + q] = fma(tv, (double)row[r][nfull * 64], acc[r * QT + q]);
            }
        }
        gallery_reduce<GALLERY_ROWS * QT>(acc, lane);              // acc[0] of lane gallery_lane_of(a) = wave_sum_d of accumulator a
#pragma unroll
        for (int r = 0; r < GALLERY_ROWS; ++r) {
            const int s = base + r;
            if (s >= Ns) break;                                    // wave-uniform
            const double val = __shfl(acc[0], src[r]);             // lane q: the similarity of (query q, shape s)
            if (own_c >= 0 && s != own_c && gallery_ranks_before(val, s, own_s, own_c)) ++cnt;
            unsigned long long todo = __ballot(lane < QT && (n < k || gallery_ranks_before(val, s, thr_s, thr_i)));
            while (todo) {                                         // the queries whose list this row enters: rare once the lists are full
                const int q = __builtin_ctzll(todo);
                todo &= todo - 1;
                const double v = gallery_readlane(val, q);
                // insert (v, s): lane j looks at entry j; the entries ranking before the candidate are a prefix of the sorted list
                double e = 0.0;
                int ei = -1;
                bool before = false;
                if (lane < n) {
                    e = ls[q * k + lane];
                    ei = li[q * k + lane];
                    before = gallery_ranks_before(e, ei, v, s);
                }
                const int pos = __popcll(__ballot(before));
                if (lane >= pos && lane < n && lane + 1 < k) { ls[q * k + lane + 1] = e; li[q * k + lane + 1] = ei; }
                if (lane == 0) { ls[q * k + pos] = v; li[q * k + pos] = s; }
                __builtin_amdgcn_wave_barrier();
                if (n + 1 >= k && lane == q) { thr_s = ls[q * k + k - 1]; thr_i = li[q * k + k - 1]; }
            }
            n = min(n + 1, k);
        }
    }
    if (lane == 0) wn[wave] = n;
    if (lane < QT) wcnt[wave * QT + lane] = cnt;
    __syncthreads();
    // thread (wave, lane) owns entry `lane` of that wave's list: its place among all entries of the query is its place in the result
    for (int q = 0; q < QT && q0 + q < Nq; ++q) {
        if (lane < wn[wave]) {
            const double e = lsim[((size_t)wave * QT + q) * k + lane];
            const int ei = lidx[((size_t)wave * QT + q) * k + lane];
            int rank = 0;
            for (int w = 0; w < 4; ++w) {
                const int nw = wn[w];
                for (int j = 0; j < nw; ++j)
                    rank += gallery_ranks_before(lsim[((size_t)w * QT + q) * k + j], lidx[((size_t)w * QT + q) * k + j], e, ei) ? 1 : 0;
            }
            if (rank < k) {
                topk_idx[(size_t)(q0 + q) * k + rank] = ei;
                topk_sim[(size_t)(q0 + q) * k + rank] = e;
            }
        }
        if (first_hit && t == 0)
            first_hit[q0 + q] = oidx[q] >= 0 ? wcnt[q] + wcnt[QT + q] + wcnt[2 * QT + q] + wcnt[3 * QT + q] : -1;
    }
}

template <int QT, bool CLS>
static void launch_gallery(const float* text, const float* shape, const int* label, const int* class_off, const int* class_rows, int ncls,
                           int Nq, int Ns, int D, int k, int* topk_idx, double* topk_sim, int* first_hit, hipStream_t stream) {
    const size_t smem = (size_t)QT * D * 8 + (size_t)4 * QT * k * 12 + (size_t)QT * 28 + 16;
    retrieval_gallery_kernel<QT, CLS><<<(Nq + QT - 1) / QT, 256, smem, stream>>>(text, shape, label, class_off, class_rows, ncls, Nq, Ns, D, k,
                                                                                 topk_idx, topk_sim, first_hit);
}

// the argument checks and the tile choice of both entry points (name: whose message it is)
template <bool CLS>
static int gallery_call(const char* name, const float* text, const float* shape, const int* label, const int* class_off,
                        const int* class_rows, int ncls, int Nq, int Ns, int D, int k, int* topk_idx, double* topk_sim, int* first_hit,
                        void* stream) {
    char msg[160];
    if (Nq <= 0) return TRI_OK;
    if (k < 1 || k > Ns) { snprintf(msg, sizeof msg, "%s: need 1 <= k <= number of shapes", name); tri_set_error(msg); return TRI_ERR_ARG; }
    if (k > TRI_GALLERY_MAX_K) { snprintf(msg, sizeof msg, "%s: k > 64 (TRI_GALLERY_MAX_K): a wave keeps one list entry per lane", name); tri_set_error(msg); return TRI_ERR_UNSUPPORTED; }
    if (first_hit && (!label || (CLS && (!class_off || !class_rows || ncls < 0)))) {
        snprintf(msg, sizeof msg, CLS ? "%s: first_hit needs query_class, class_off and class_rows" : "%s: first_hit needs label", name);
        tri_set_error(msg);
        return TRI_ERR_ARG;
    }
    if (D < 1) { snprintf(msg, sizeof msg, "%s: need D >= 1", name); tri_set_error(msg); return TRI_ERR_ARG; }
    if (D > GALLERY_MAX_D) { snprintf(msg, sizeof msg, "%s: D > 4096 does not fit the 32 KiB float64 query tile in LDS", name); tri_set_error(msg); return TRI_ERR_UNSUPPORTED; }
    if (CLS && !first_hit) label = nullptr;                        // nothing to count: no pass over the classes either
    hipStream_t st = (hipStream_t)stream;
    if (D <= 512) launch_gallery<8, CLS>(text, shape, label, class_off, class_rows, ncls, Nq, Ns, D, k, topk_idx, topk_sim, first_hit, st);
    else if (D <= 1024) launch_gallery<4, CLS>(text, shape, label, class_off, class_rows, ncls, Nq, Ns, D, k, topk_idx, topk_sim, first_hit, st);
    else if (D <= 2048) launch_gallery<2, CLS>(text, shape, label, class_off, class_rows, ncls, Nq, Ns, D, k, topk_idx, topk_sim, first_hit, st);
    else launch_gallery<1, CLS>(text, shape, label, class_off, class_rows, ncls, Nq, Ns, D, k, topk_idx, topk_sim, first_hit, st);
    return tri_check_launch(name);
}

extern "C" int tri_retrieval_gallery(const float* text, const float* shape, const int* label, int Nq, int Ns, int D, int k, int* topk_idx,
                                     double* topk_sim, int* first_hit, void* stream) {
    return gallery_call<false>("tri_retrieval_gallery", text, shape, label, nullptr, nullptr, 0, Nq, Ns, D, k, topk_idx, topk_sim, first_hit, stream);
}

// Shape -> text: several candidates are correct for a query, named by a class.  first_hit[q] = the rows ranking before the best row of
// class query_class[q] (-1: no such class, or an empty one); the top k are tri_retrieval_gallery's.
extern "C" int tri_retrieval_classes(const float* query, const float* cand, const int* query_class, const int* class_off, const int* class_rows,
                                     int Nq, int Nc, int D, int ncls, int k, int* topk_idx, double* topk_sim, int* first_hit, void* stream) {
    return gallery_call<true>("tri_retrieval_classes", query, cand, query_class, class_off, class_rows, ncls, Nq, Nc, D, k, topk_idx, topk_sim,
                              first_hit, stream);
}
