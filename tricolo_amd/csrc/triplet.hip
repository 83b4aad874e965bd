// Semi-hard triplet loss with a hard-negative fallback, forward + backward, for gfx950 - the reference's second loss
// (tricolo/loss/triplet.py: a Python double loop over B x B that reads the distance matrix element by element).
//
//   sq[i][j] = |zls[j]|^2 - 2 <zls[i], zis[j]> + |zis[i]|^2      (the reference's formula, its swapped norms included)
//   d = sqrt(max(sq, 0)), gradient 0 where sq <= 0
//   S = {(i, j), j != i : d[i][i] < d[i][j] < d[i][i] + margin},  H = {(i, j), j != i : d[i][j] < d[i][i]}
//   loss = mean over S (over H when S is empty) of d[i][i] - d[i][j] + margin;  both empty: 0 / 0 = NaN, every gradient NaN
//
// The sets are thresholds on differences of distances, and sq cancels (1 + 1 - 1.9996 for a close pair), so the norms, the dot
// products, the distances and the sums are float64 from the fp32 inputs (as retrieval.hip forms its similarities): B * B * D FMAs
// per pair, launch latency and not arithmetic.  Three launches forward (squared norms; one block per row: distances, then that
// row's sums and counts for BOTH sets; a finalize that picks the branch on the device) and one backward.  No atomics, every
// reduction in a fixed order, the branch and the counts never leave the device: the step stays one captured graph and a replay
// takes whichever branch its inputs call for.
#include <stdio.h>
#include "common.h"
#include "../../include/tricolo_hip.h"

#define TRP_MAX_MOD 3
struct TrpMulti {
    const float* z[TRP_MAX_MOD];
    double* n2[TRP_MAX_MOD];             // per modality: squared row norms
    double* dist[TRP_MAX_MOD];           // per pair: d [B][B]
    double* rowsum[TRP_MAX_MOD];         //           [B][2] sums of d_ii - d_ij + margin over row i's members of S / of H
    int* rowcnt[TRP_MAX_MOD];            //           [B][2] their numbers
    double* fin[TRP_MAX_MOD];            //           [0] 1 / N of the chosen set (NaN when N = 0); ((int*)(fin + 1))[0] branch (0 S, 1 H), [1] N
    const float* dpair[TRP_MAX_MOD];     // backward: upstream gradient of each pair's loss (device scalars, may be NULL)
    const float* dtotal;                 //           ... and of the total
    float* dz[TRP_MAX_MOD];
    int pa[TRP_MAX_MOD], pb[TRP_MAX_MOD];        // pair q = loss_fn(zis = z[pa], zls = z[pb])
    int M, P, B, D;
    double margin;
};

// one wave per row, block (4 rows, modality m)
__global__ __launch_bounds__(256) void trp_norm_kernel(const TrpMulti p) {
    const int m = blockIdx.y, row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= p.B) return;
    const float* x = p.z[m] + (long)row * p.D;
    double s = 0.0;
#pragma unroll 8
    for (int k = lane; k < p.D; k += 64) { const double v = (double)x[k]; s = fma(v, v, s); }
    s = wave_sum_d(s);
    if (lane == 0) p.n2[m][row] = s;
}

// membership of candidate (i, j), j != i, in S (bit 0) and H (bit 1), from the stored distances: the forward and the backward
// take the same decision from the same doubles
__device__ __forceinline__ int trp_member(double dii, double dij, double margin) {
    return ((dii < dij && dij < dii + margin) ? 1 : 0) | (dij < dii ? 2 : 0);
}

// block (row i, pair q): d[i][:] (each wave four columns at a time, as ntxm_sim_rows_kernel), then the row's sums and counts.
// VEC: D % 4 == 0, 16-byte loads.
template <bool VEC>
__global__ __launch_bounds__(256) void trp_dist_kernel(const TrpMulti p) {
    extern __shared__ float sl[];                                  // zls[i]
    __shared__ double shd[4];
    __shared__ int shi[4];
    const int i = blockIdx.x, q = blockIdx.y, t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int B = p.B, D = p.D;
    const float* zis = p.z[p.pa[q]];
    const float* zls = p.z[p.pb[q]];
    const double* nis = p.n2[p.pa[q]];
    const double* nls = p.n2[p.pb[q]];
    double* drow = p.dist[q] + (long)i * B;
    if (VEC) { for (int k = t * 4; k < D; k += 1024) *(float4*)(sl + k) = *(const float4*)(zls + (long)i * D + k); }
    else     { for (int k = t; k < D; k += 256) sl[k] = zls[(long)i * D + k]; }
    __syncthreads();
    const double ni = nis[i];
    for (int jb = wave * 4; jb < B; jb += 16) {
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        if (VEC) {
            for (int k = lane * 4; k < D; k += 256) {
                const float4 av = *(const float4*)(sl + k);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int j = jb + u < B ? jb + u : B - 1;
                    const float4 bv = *(const float4*)(zis + (long)j * D + k);
                    acc[u] = fma((double)av.x, (double)bv.x, fma((double)av.y, (double)bv.y,
                             fma((double)av.z, (double)bv.z, fma((double)av.w, (double)bv.w, acc[u]))));
                }
            }
        } else {
            for (int k = lane; k < D; k += 64) {
                const double av = (double)sl[k];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int j = jb + u < B ? jb + u : B - 1;
                    acc[u] = fma(av, (double)zis[(long)j * D + k], acc[u]);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const double dot = wave_sum_d(acc[u]);
            const int j = jb + u;
            if (lane == 0 && j < B) {
                const double sq = (nls[j] - 2.0 * dot) + ni;       // the reference's order of operations
                drow[j] = sq > 0.0 ? sqrt(sq) : 0.0;
            }
        }
    }
    __syncthreads();                                               // the row, written by this block, is read back by this block
    const double dii = drow[i];
    double ssum = 0.0, hsum = 0.0;
    int scnt = 0, hcnt = 0;
    for (int j = t; j < B; j += 256) {
        if (j == i) continue;
        const double dij = drow[j];
        const int mem = trp_member(dii, dij, p.margin);
        const double term = dii - dij + p.margin;
        if (mem & 1) { ssum += term; ++scnt; }
        if (mem & 2) { hsum += term; ++hcnt; }
    }
    ssum = block_sum_d(ssum, shd);
    hsum = block_sum_d(hsum, shd);
    scnt = block_sum_i(scnt, shi);
    hcnt = block_sum_i(hcnt, shi);
    if (t == 0) {
        p.rowsum[q][2 * i] = ssum; p.rowsum[q][2 * i + 1] = hsum;
        p.rowcnt[q][2 * i] = scnt; p.rowcnt[q][2 * i + 1] = hcnt;
    }
}

// one wave per pair sums the rows (fixed order per lane + shuffle tree), picks the branch and writes loss, 1 / N and the counts;
// thread 0 forms the total as Python's sum() does, (l0 + l1) + l2 in fp32
__global__ void trp_finalize_kernel(const TrpMulti p, float* __restrict__ losses, int* __restrict__ counts, int write_total) {
    __shared__ float lp[TRP_MAX_MOD];
    const int q = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (q < p.P) {
        double ss = 0.0, hs = 0.0;
        int sc = 0, hc = 0;
        for (int i = lane; i < p.B; i += 64) {
            ss += p.rowsum[q][2 * i]; hs += p.rowsum[q][2 * i + 1];
            sc += p.rowcnt[q][2 * i]; hc += p.rowcnt[q][2 * i + 1];
        }
        ss = wave_sum_d(ss); hs = wave_sum_d(hs);
        sc = wave_sum_i(sc); hc = wave_sum_i(hc);
        if (lane == 0) {
            const int branch = sc > 0 ? 0 : 1, n = sc > 0 ? sc : hc;
            const double nan = __longlong_as_double(0x7ff8000000000000LL);
            const double loss = n > 0 ? (branch == 0 ? ss : hs) / (double)n : nan;      // sum([]) / 0 in IEEE arithmetic
            p.fin[q][0] = n > 0 ? 1.0 / (double)n : nan;
            int* fi = (int*)(p.fin[q] + 1);
            fi[0] = branch; fi[1] = n;
            lp[q] = (float)loss;
            losses[q] = (float)loss;
            if (counts) { counts[2 * q] = sc; counts[2 * q + 1] = hc; }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && write_total) {
        float tot = 0.f;
        for (int q2 = 0; q2 < p.P; ++q2) tot += lp[q2];
        losses[p.P] = tot;
    }
}

// block (row x, modality m): d z_m[x] summed over the pairs m takes part in.  With c = d loss / d sq (coefficient matrix of a pair):
//   m is the pair's zls:  dzls[x] = -2 sum_j c[x][j] zis[j] + 2 (sum_i c[i][x]) zls[x]     (row x contracted, column x summed)
//   m is the pair's zis:  dzis[x] = -2 sum_i c[i][x] zls[i] + 2 (sum_j c[x][j]) zis[x]     (column x contracted, row x summed)
// c[i][j] = -g / (N 2 d[i][j]) on the chosen set, c[i][i] = g n_i / (N 2 d[i][i]), 0 where d = 0.
__device__ __forceinline__ double trp_coef(const double* __restrict__ dist, const int* __restrict__ rowcnt, int B, int i, int j, int branch,
                                           double margin, double scale /* g / N */) {
    const double dii = dist[(long)i * B + i];
    if (i == j) return dii > 0.0 ? scale * (double)rowcnt[2 * i + branch] / (2.0 * dii) : 0.0;
    const double dij = dist[(long)i * B + j];
    const bool sel = (trp_member(dii, dij, margin) >> branch) & 1;
    return (sel && dij > 0.0) ? -scale / (2.0 * dij) : 0.0;
}

__global__ __launch_bounds__(256) void trp_grad_kernel(const TrpMulti p) {
    extern __shared__ double w[];                // [np][B] coefficients contracted with the other modality's rows
    __shared__ double shd[4];
    const int x = blockIdx.x, m = blockIdx.y, t = threadIdx.x, B = p.B, D = p.D;
    const float* other[2] = {nullptr, nullptr};
    double selfc[2] = {0.0, 0.0};
    bool empty[2] = {false, false};
    int np = 0;
    const float gt = p.dtotal ? *p.dtotal : 0.f;
    for (int q = 0; q < p.P; ++q) {
        const int side = p.pa[q] == m ? 0 : (p.pb[q] == m ? 1 : -1);
        if (side < 0) continue;
        const float up = gt + (p.dpair[q] ? *p.dpair[q] : 0.f);
        const int* fi = (const int*)(p.fin[q] + 1);
        const int branch = fi[0];
        const double scale = (double)up * p.fin[q][0];
        double other_sum = 0.0;                  // the sum along the direction that is NOT contracted
        for (int j = t; j < B; j += 256) {
            const double crow = trp_coef(p.dist[q], p.rowcnt[q], B, x, j, branch, p.margin, scale);     // c[x][j]
            const double ccol = trp_coef(p.dist[q], p.rowcnt[q], B, j, x, branch, p.margin, scale);     // c[j][x]
            w[np * B + j] = side == 1 ? crow : ccol;
            other_sum += side == 1 ? ccol : crow;
        }
        selfc[np] = block_sum_d(other_sum, shd);
        empty[np] = fi[1] == 0;
        other[np] = p.z[side == 1 ? p.pa[q] : p.pb[q]];
        ++np;
    }
    __syncthreads();
    const float* self = p.z[m] + (long)x * D;
    const float nanf_ = __int_as_float(0x7fc00000);
#pragma unroll
    for (int u = 0; u < 8; ++u) {                // D <= 2048
        const int c = t + u * 256;
        if (c < D) {
            float tot = 0.f;
            for (int k = 0; k < np; ++k) {       // pair by pair, each rounded to fp32 as the single-pair call leaves it, then summed
                double acc = 0.0;
                const float* ot = other[k];
                const double* wk = w + k * B;
#pragma unroll 8
                for (int j = 0; j < B; ++j) acc = fma(wk[j], (double)ot[(long)j * D + c], acc);
                const float v = (float)(2.0 * selfc[k] * (double)self[c] - 2.0 * acc);
                tot += empty[k] ? nanf_ : v;
            }
            p.dz[m][(long)x * D + c] = tot;
        }
    }
}

static size_t trp_workspace(int M, int B) {
    const int P = M * (M - 1) / 2;
    return (size_t)M * al256((size_t)B * 8) + (size_t)P * (al256((size_t)B * B * 8) + al256((size_t)B * 16) + al256((size_t)B * 8) + 256);
}

// multi: the fused range of the all-pairs forms; the single-pair forms take any 1 <= D <= 2048 and B up to 4096
static int trp_setup(TrpMulti& p, const float* const* z, int M, int B, int D, double margin, void* workspace, size_t workspace_bytes,
                     bool multi, const char* who) {
    char msg[160];
    if (M < 2 || M > TRP_MAX_MOD) { tri_set_error("tri_triplet_multi: 2 or 3 modalities"); return TRI_ERR_ARG; }
    if (multi ? (B < 2 || B > 512 || D < 4 || D > 2048 || D % 4) : (B < 2 || B > 4096 || D < 1 || D > 2048)) {
        snprintf(msg, sizeof(msg), multi ? "%s: need 2<=B<=512, 4<=D<=2048, D%%4==0 (else use tri_triplet_fwd per pair)"
                                         : "%s: need 2<=B<=4096, 1<=D<=2048", who);
        tri_set_error(msg);
        return TRI_ERR_UNSUPPORTED;
    }
    if (!z || !workspace || workspace_bytes < trp_workspace(M, B)) { snprintf(msg, sizeof(msg), "%s: workspace too small", who); tri_set_error(msg); return TRI_ERR_ARG; }
    p.M = M; p.P = M * (M - 1) / 2; p.B = B; p.D = D; p.margin = margin;
    char* w = (char*)workspace;
    for (int m = 0; m < M; ++m) {
        if (!z[m]) { snprintf(msg, sizeof(msg), "%s: NULL embedding", who); tri_set_error(msg); return TRI_ERR_ARG; }
        p.z[m] = z[m];
        p.n2[m] = (double*)w; w += al256((size_t)B * 8);
    }
    int q = 0;
    for (int a = 0; a < M; ++a)                    // itertools.combinations order: loss_fn(z[a], z[b])
        for (int b = a + 1; b < M; ++b, ++q) {
            p.pa[q] = a; p.pb[q] = b;
            p.dist[q] = (double*)w; w += al256((size_t)B * B * 8);
            p.rowsum[q] = (double*)w; w += al256((size_t)B * 16);
            p.rowcnt[q] = (int*)w; w += al256((size_t)B * 8);
            p.fin[q] = (double*)w; w += 256;
        }
    return 0;
}

static int trp_forward(const TrpMulti& p, float* losses, int* counts, int write_total, hipStream_t s, const char* who) {
    trp_norm_kernel<<<dim3((p.B + 3) / 4, p.M), 256, 0, s>>>(p);
    if (p.D % 4 == 0) trp_dist_kernel<true><<<dim3(p.B, p.P), 256, (size_t)p.D * sizeof(float), s>>>(p);
    else trp_dist_kernel<false><<<dim3(p.B, p.P), 256, (size_t)p.D * sizeof(float), s>>>(p);
    trp_finalize_kernel<<<1, 64 * TRP_MAX_MOD, 0, s>>>(p, losses, counts, write_total);
    return tri_check_launch(who);
}

static int trp_backward(const TrpMulti& p, hipStream_t s, const char* who) {
    const int np = p.M == 3 ? 2 : 1;
    trp_grad_kernel<<<dim3(p.B, p.M), 256, (size_t)np * p.B * sizeof(double), s>>>(p);
    return tri_check_launch(who);
}

extern "C" size_t tri_triplet_workspace(int B, int D) { (void)D; return B < 1 ? 0 : trp_workspace(2, B); }

extern "C" int tri_triplet_fwd(const float* zis, const float* zls, int B, int D, double margin, float* loss, int* counts, void* workspace,
                               size_t workspace_bytes, void* stream) {
    TrpMulti p{};
    const float* z[2] = {zis, zls};
    int rc = trp_setup(p, z, 2, B, D, margin, workspace, workspace_bytes, false, "tri_triplet_fwd");
    if (rc) return rc;
    if (!loss) { tri_set_error("tri_triplet_fwd: loss is NULL"); return TRI_ERR_ARG; }
    return trp_forward(p, loss, counts, 0, (hipStream_t)stream, "tri_triplet_fwd");
}

extern "C" int tri_triplet_bwd(const float* zis, const float* zls, int B, int D, double margin, const float* dloss, float* dzis, float* dzls,
                               const void* workspace, size_t workspace_bytes, void* stream) {
    TrpMulti p{};
    const float* z[2] = {zis, zls};
    int rc = trp_setup(p, z, 2, B, D, margin, (void*)workspace, workspace_bytes, false, "tri_triplet_bwd");
    if (rc) return rc;
    if (!dloss || !dzis || !dzls) { tri_set_error("tri_triplet_bwd: NULL dloss / gradient buffer"); return TRI_ERR_ARG; }
    p.dz[0] = dzis; p.dz[1] = dzls;
    p.dpair[0] = dloss;
    return trp_backward(p, (hipStream_t)stream, "tri_triplet_bwd");
}

extern "C" size_t tri_triplet_multi_workspace(int M, int B, int D) { (void)D; return (M < 2 || M > TRP_MAX_MOD || B < 1) ? 0 : trp_workspace(M, B); }

extern "C" int tri_triplet_multi_fwd(const float* const* z, int M, int B, int D, double margin, float* losses, int* counts, void* workspace,
                                     size_t workspace_bytes, void* stream) {
    TrpMulti p{};
    int rc = trp_setup(p, z, M, B, D, margin, workspace, workspace_bytes, true, "tri_triplet_multi_fwd");
    if (rc) return rc;
    if (!losses) { tri_set_error("tri_triplet_multi_fwd: losses is NULL"); return TRI_ERR_ARG; }
    return trp_forward(p, losses, counts, 1, (hipStream_t)stream, "tri_triplet_multi_fwd");
}

extern "C" int tri_triplet_multi_bwd(const float* const* z, int M, int B, int D, double margin, const float* const* dpair, const float* dtotal,
                                     float* const* dz, const void* workspace, size_t workspace_bytes, void* stream) {
    TrpMulti p{};
    int rc = trp_setup(p, z, M, B, D, margin, (void*)workspace, workspace_bytes, true, "tri_triplet_multi_bwd");
    if (rc) return rc;
    if (!dz) { tri_set_error("tri_triplet_multi_bwd: dz is NULL"); return TRI_ERR_ARG; }
    for (int m = 0; m < M; ++m) {
        if (!dz[m]) { tri_set_error("tri_triplet_multi_bwd: NULL gradient buffer"); return TRI_ERR_ARG; }
        p.dz[m] = dz[m];
    }
    for (int q = 0; q < p.P; ++q) p.dpair[q] = dpair ? dpair[q] : nullptr;
    p.dtotal = dtotal;
    return trp_backward(p, (hipStream_t)stream, "tri_triplet_multi_bwd");
}
